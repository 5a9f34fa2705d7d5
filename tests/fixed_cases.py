"""Inputs, oracle references and the route table of the per-shape tests of the FIXED-step loss and gradient kernels
(tests/test_gpu_fixed_shapes.py on the device, tests/test_fixed_cases_host.py for the inputs and the table themselves).

Inputs: adaptive_cases.cpep_case / supp_case -- live biases, scaled age column (the docstring there says why not
conftest.make_cpep_case / make_supp_case) -- with 70 subjects for EVERY shape (a second workgroup whose wave has six live
lanes; also the smallest population the mixed launch "3:1:L" accepts: it needs a block behind the one-lane ones), S = 30
steps, and three parameter sets per shape that share no weight and no conditional parameter.

Which kernel a launch lands on is not observable through the engine.  The device module relies on the rules below, each
quoted from the source line it rests on; tests/test_fixed_cases_host.py reads the quoted constants out of the .hip files,
so a reworded rule fails there instead of silently sending the device module to another instance.

c-peptide, tanh / softplus network of one of the 24 CPEP_SHAPES, option "cpep_path" set BEFORE the population
(cude_select.hip setup_chunks: `if (forced == 1) return CUDE_OK;`, `if (forced == 2) { L = c->opt.path_chunks; blk0 = 0; }`,
`if (forced == 3) {`):

  "1"  one lane per subject (cude_cpep.hip launch_one)
    * forward(...)                       cpep_kernel<Net, NS, false>, grid (blocks, 1)
        `hipLaunchKernelGGL((cpep_kernel<Net, NS, GRAD>), dim3((unsigned)nblocks, n_sets), dim3(kBlock), lds, s, a);`
    * loss_grad()                        cpep_kernel<Net, NS, true> -- the same line with GRAD = true.  Shapes with
                                         Net::HAS_LEAN hold the sweeps twice; "lean_clamp" = 0 keeps every wave on the
                                         clamped form, -1 (the rule) sends a wave whose weights pass Mlp::lean_ok -- every
                                         set here does -- to the clamp-free one:
        `if (a.lean_clamp != 0 && Net::lean_ok(launder(as_const(a.nn + (int64_t)blockIdx.y * a.set_stride_nn))))`
    * loss_grad(), "cpep_keep" = 1 / 2   cpep_kernel<Net, NS, true, 1> / <Net, NS, true, 2> where the shape has the
                                         variant (cpep_can_keep: `return Net::HAS_VW && Net::DEPTH >= 2 && Net::HAS_TAB;`),
                                         single parameter set only; any other shape: cpep_keep_mode returns 0
                                         (`return (m == 1 || m == 2) && cpep_act_doubles(c) > 0 ? m : 0;`), the plain kernel:
        `if (a.act != nullptr && n_sets == 1) {` / `if (a.keep_mode == 2)`
    * multistart_forward(sets)           cpep_kernel<Net, NS, false>, set = blockIdx.y -- on EVERY path: cude_batch.hip
                                         cude_multistart_forward reserves with `reserve_sets_forward(c, chunk, false, d_part)`
                                         and leaves SetsForward::split false
    * multistart_loss_grad(sets)         cpep_kernel<Net, NS, true>, set = blockIdx.y (chunks = 1, so not time-split:
                                         cude_launch.hip eval_sets_device `} else if (!supp) {`)

  "2:L"  time-split, L chunks (cude_cpep2.hip run_shape); forward(want_traj=True) stays on the one-lane kernel
         (cude_launch.hip: `} else if (c->chunks > 1 && (grad || traj_dev == nullptr)) {`)
    * forward(want_sse=True)             cpep2_fwd_kernel<NIN, W, D, NS, VWR> + scan
    * loss_grad()                        cpep2_fwd_kernel + scan + cpep2_rev_kernel<NIN, W, D>
      VWR (the weights in VGPRs) where the shape has it (Mlp::HAS_VW_SMALL) and the grid is small:
        `const bool vwr = Net::HAS_VW_SMALL && !no_vw && nblocks * a.L * n_sets <= 2 * 1024;`
      2 blocks x L <= 30 chunks x 1 set = at most 60 waves: the VWR instance.
      Scan: the eight-wave bulk scan where the chunks are even, otherwise the plain one-wave scan:
        `const bool bulk = a.scan_bulk_blocks > 0 && scan_blocks <= a.scan_bulk_blocks && a.base.blk0 == 0 && a.base.S % a.L == 0 &&`
      "2:3" even chunks of 10 steps (bulk); "2:7" 30 / 7 uneven (plain scan; chunks of 4 or 5 steps over observation
      times 7.5 steps apart: chunks 2 and 4 -- steps [8, 12) and [17, 21) -- hold no observation); "2:30" one step per
      chunk (even: bulk, its 3 L + ... rows fitting the 156 KB of `lds_bulk <= kScanBulkMaxLds`).
    * multistart_loss_grad(36 sets) on "2:30"   time-split, set = blockIdx.z, by eval_sets_device:
        `const bool split = !supp && L > 1 && c->blk0 == 0 && nb * (int64_t)std::min<int64_t>(n_sets, 64) <= 512 &&`
      2 x min(36, 64) = 72 <= 512, and the grid is 2 x 30 x 36 = 2160 waves > 2048: the NON-VWR instance
      cpep2_fwd_kernel<NIN, W, D, NS>
        `hipLaunchKernelGGL((cpep2_fwd_kernel<NIN, W, D, 2>), grid2, dim3(kBlock), lds_b, s, a);`
      -- the one a time-split population above ~9 000 subjects runs.  (multistart_loss_grad of 3 sets on "2:30": 180 waves, VWR.)

  "3:1:5"  mixed: block 0 on cpep_kernel<Net, NS, true> (blk_count = 1), block 1 time-split in 5 chunks with the plain
           scan (blk0 > 0 fails `a.base.blk0 == 0` above), on a second stream
        `if (c->chunks > 1 && c->blk0 > 0 && grad) {`

suppression, (4, w, d) of the 16 SUPP_SHAPES (cude_supp.hip launch_supp); "supp_store" and "supp_ckpt" set BEFORE the
population (the kept-activation buffer is sized there):
        `return !grad ? launch_one<W, D, false, false>(a, s)`
        `: (a.ckpt_steps_only ? launch_one<W, D, true, false, true>(a, s)`
        `: (a.act != nullptr ? launch_one<W, D, true, true>(a, s) : launch_one<W, D, true, false>(a, s)));`
    * forward(...), multistart_forward   supp_kernel<W, D, false, false>
    * loss_grad / multistart_loss_grad   "supp_ckpt" = "steps": supp_kernel<W, D, true, false, /*YONLY=*/true>
                                         (cude_select.hip `bool supp_steps_only(const cude_ctx* c) { return c->opt.supp_ckpt_steps != 0; }`)
                                         otherwise by cude_select.hip supp_keep_activations:
        `if (c->opt.supp_store == 0 || c->opt.supp_store == 1) return c->opt.supp_store == 1;`
        `return (double)n_sets * (double)supp_act_doubles(c) * 8.0 <= 256e6;`
                                         "supp_store" = 1: supp_kernel<W, D, true, /*STORE=*/true>; = 0:
                                         supp_kernel<W, D, true, false> -- the kernel 1e5 subjects run, which no population
                                         of test size reaches by the size rule (3 sets x 70 subjects x 181 evaluations x
                                         (d w + 1) values x 8 B < 6 MB).

other activation functions (options "hidden_activation" / "output_activation"): the one-lane kernels only
(cude_cpep2.hip `if (net.general() || net.generic()) return false;`; cude_supp.hip
`return grad ? launch_one<W, D, true, false, false, HA, OA>(a, s) : launch_one<W, D, false, false, false, HA, OA>(a, s);`)."""
import numpy as np

import adaptive_cases as ac

CPEP_SHAPES, SUPP_SHAPES = ac.CPEP_SHAPES, ac.SUPP_SHAPES
N_SUBJECTS = 70
N_STEPS = 30
SUPP_LAMBDA = 0.01
N_SETS = 3
MANY_SETS = 36                          # parameter sets of the large time-split grid
FORWARD_ORACLE_MAX = 128                # oracle/cude_oracle.c NPMAX: partials (P + 1) the forward-mode oracle carries

# ----------------------------------------------------------------------------- the launch rules the route table rests on
BLOCK = 64                              # csrc/cude_kernels.h kBlock: subjects per workgroup
VWR_MAX_WAVES = 2 * 1024                # cude_cpep2.hip run_shape
SPLIT_SET_CAP, SPLIT_MAX_WAVES = 64, 512    # cude_launch.hip eval_sets_device
SUPP_KEEP_BYTES = 256e6                 # cude_select.hip supp_keep_activations


def n_blocks(N=N_SUBJECTS):
    return (N + BLOCK - 1) // BLOCK


def forward_chunk_waves(L, n_sets, N=N_SUBJECTS):
    """Grid of cpep2_fwd_kernel: (blocks, chunks, sets)."""
    return n_blocks(N) * L * n_sets


def runs_vwr(L, n_sets, N=N_SUBJECTS):
    """run_shape's choice for a shape that HAS the VWR instance (the others run the plain one whatever the grid)."""
    return forward_chunk_waves(L, n_sets, N) <= VWR_MAX_WAVES


def sets_run_time_split(n_sets, N=N_SUBJECTS):
    """eval_sets_device on a time-split context without one-lane blocks (default "ms_split")."""
    return n_blocks(N) * min(n_sets, SPLIT_SET_CAP) <= SPLIT_MAX_WAVES


def supp_kept_bytes(shape, n_sets, N=N_SUBJECTS, S=N_STEPS):
    w, d = shape
    return n_sets * (6 * S + 1) * (d * w + 1) * N * 8.0


def cpep_has_keep(arch):
    """cude_cpep.hip cpep_can_keep for CpepNet<nin, w, d> (cude_device.h: HAS_TAB widths 6 and 7; HAS_VW: the
    NVW = (d - 1)(w w + w) + w + 1 upper-layer weights fit 49 VGPRs): does the shape have the "cpep_keep" kernels?"""
    nin, w, d = arch
    has_tab = 6 <= w <= 7
    has_vw = (d - 1) * (w * w + w) + w + 1 <= 49 and (w >= 6 or d >= 3)
    return has_vw and d >= 2 and has_tab


def chunk_starts(S, L):
    """cude_select.hip chunk_starts: first step of each of L chunks of S steps, and S."""
    return [k * S // L for k in range(L + 1)]


# ----------------------------------------------------------------------------- inputs
_CASES = {}


def _freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


def _sets(model, k, c, cond, draw):
    """(nn_sets (3, P), cond_sets (3, N)): set 0 the case's own, sets 1 and 2 biased_params of other seeds (the cases use
    seeds below 50) with the conditional parameters redrawn."""
    nn, cd = [c["nn"]], [c[cond]]
    for j in (1, 2):
        nn.append(ac.biased_params(c["arch"], 1000 + 100 * j + k))
        cd.append(draw(np.random.default_rng([0xF1ED, model, k, j])))
    nn, cd = np.stack(nn), np.stack(cd)
    _freeze(nn, cd)
    return c, nn, cd


def cpep_fixed_case(k):
    """(case, nn_sets, beta_sets) of CPEP_SHAPES[k]: adaptive_cases.cpep_case on the five-knot grid, 70 subjects."""
    if ("cpep", k) not in _CASES:
        c = ac.cpep_case(CPEP_SHAPES[k], k, ac.TP5, N_SUBJECTS)
        _CASES["cpep", k] = _sets(0, k, c, "beta", lambda rng: rng.normal(-0.6, 0.5, N_SUBJECTS))
    return _CASES["cpep", k]


def supp_fixed_case(k):
    """(case, nn_sets, theta_sets) of SUPP_SHAPES[k]: adaptive_cases.supp_case, 70 subjects (lambda = SUPP_LAMBDA)."""
    if ("supp", k) not in _CASES:
        s = ac.supp_case(SUPP_SHAPES[k], k, N_SUBJECTS)
        _CASES["supp", k] = _sets(1, k, s, "theta", lambda rng: 0.5 * rng.standard_normal(N_SUBJECTS))
    return _CASES["supp", k]


def rotate_biases(nn, arch):
    """nn with every layer's biases rotated by one unit: what a kernel that fetched bias j - 1 for unit j would compute
    with.  (The output unit's single bias stays.)"""
    nn = np.array(nn)
    for name, s in ac.layer_blocks(arch):
        if name.startswith("b") and s.stop - s.start > 1:
            nn[s] = np.roll(nn[s], 1)
    return nn


# ----------------------------------------------------------------------------- oracle references
_REFS = {}


def oracle_method(P):
    """The forward-mode C oracle (the reference's own AD) while it can carry P + 1 partials, else the reverse-mode one."""
    return "forward" if P + 1 <= FORWARD_ORACLE_MAX else "reverse"


def _keep(key, r, g_cond, traj):
    out = dict(loss=r["loss"], sse=r["sse"], g_nn=r["g_nn"], g_cond=r[g_cond], traj=traj, n_failed=r["n_failed"])
    _freeze(*out.values())
    _REFS[key] = out
    return out


def cpep_ref(k, n_state, j, method=None):
    """Oracle of set j of cpep_fixed_case(k): dict(loss, sse (N,), g_nn (P,), g_cond (N,), traj (n_state, T, N) -- every
    state, the quadrature state with n_state = 3 --, n_failed); computed once."""
    import c_oracle as co
    c, nn_sets, cond_sets = cpep_fixed_case(k)
    method = method or oracle_method(nn_sets.shape[1])
    key = ("cpep", k, n_state, j, method)
    if key in _REFS:
        return _REFS[key]
    args = (c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], c["arch"], nn_sets[j], cond_sets[j], N_STEPS, n_state)
    cov = c["arch"][0] == 3
    r = co.cpep(*args, covariate=cov, method=method, want_traj=(method == "forward"))
    traj = r["traj"] if method == "forward" else co.cpep(*args, covariate=cov, want_grad=False, want_traj=True)["traj"]
    return _keep(key, r, "g_beta", np.ascontiguousarray(traj.transpose(2, 1, 0)))


def supp_ref(k, j, method=None):
    """The same for set j of supp_fixed_case(k); traj (3, T, N)."""
    import c_oracle as co
    s, nn_sets, cond_sets = supp_fixed_case(k)
    method = method or oracle_method(nn_sets.shape[1])
    key = ("supp", k, j, method)
    if key in _REFS:
        return _REFS[key]
    args = (s["tp"], s["data"], s["arch"], nn_sets[j], cond_sets[j], SUPP_LAMBDA, N_STEPS)
    r = co.supp(*args, method=method, want_traj=(method == "forward"))
    traj = r["traj"] if method == "forward" else co.supp(*args, want_grad=False, want_traj=True)["traj"]
    return _keep(key, r, "g_theta", np.ascontiguousarray(traj))


def cpep_general_ref(shape, acts):
    """torch-autograd oracle of cpep_fixed_case's set 0 for a shape of CPEP_GENERAL_SHAPES with the (hidden, output)
    activation functions `acts`: dict(loss, sse, g_nn, g_cond).  (The quadrature state carries no loss: one reference
    for both state counts.)"""
    import cude_oracle as o
    key = ("cpep", tuple(shape), tuple(acts))
    if key not in _REFS:
        c, _, _ = cpep_fixed_case(CPEP_SHAPES.index(tuple(shape)))
        loss, g_nn, g_cond, sse = o.cpep_loss_grad_torch(c["nn"], c["beta"], ac.cpep_population(c), tuple(shape) + tuple(acts),
                                                         N_STEPS, n_state=2)
        _REFS[key] = dict(loss=loss, sse=sse, g_nn=g_nn, g_cond=g_cond)
        _freeze(*_REFS[key].values())
    return _REFS[key]


def supp_general_ref(shape, acts):
    import cude_oracle as o
    key = ("supp", tuple(shape), tuple(acts))
    if key not in _REFS:
        s, _, _ = supp_fixed_case(SUPP_SHAPES.index(tuple(shape)))
        loss, g_nn, g_cond, sse = o.supp_loss_grad_torch(s["nn"], s["theta"], s["data"], s["tp"], s["arch"] + tuple(acts),
                                                         N_STEPS, SUPP_LAMBDA)
        _REFS[key] = dict(loss=loss, sse=sse, g_nn=g_nn, g_cond=g_cond)
        _freeze(*_REFS[key].values())
    return _REFS[key]
