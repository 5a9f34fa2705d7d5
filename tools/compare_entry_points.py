"""Bit-for-bit comparison of two builds of libcude_hip.so through every entry point that batches launches
(csrc/cude_batch.hip, csrc/cude_replicates.hip, csrc/cude_mh.hip): one fresh process per library writes every output array of seeded calls to an
.npz, a third step compares the two files with numpy.array_equal (NaN positions included).

    python tools/compare_entry_points.py run <libcude_hip.so> <out.npz>      # once per library (selects cude._lib.LIB_PATH)
    python tools/compare_entry_points.py cmp <a.npz> <b.npz>                 # exit status 1 on any difference

Covered: c-peptide populations (2-6-6-1) of 57 and 700 subjects, time-split (30 steps) and one lane per subject
(cpep_path = 1) with 3 states, adaptive with the 2 states that mode integrates; the suppression model (4-3x5-1, 57
subjects), fixed step and adaptive.  Every entry point runs with the default chunking and again with the chunk options forcing several launches; mh_chain runs 11 steps for
gamma in {1, 0.35} x mh_spec in {0, 2, -1} with the caller's draws, mh_estep with the device's.  The replicate simulations
run 9 replicates / simulations: bootstrap_conditional with ranks, with the caller's noise and with the device's draws,
bootstrap_noise, npde and vpc (3 groups, one subject left out) with the caller's sets and noise and with the device's draws,
npde_draws; the chunked round splits them by bootstrap_chunk = 2, bootstrap_subjects = npde_subjects = 64, vpc_sims = 2 and
sends every vpc column through the radix select (vpc_select = 1).  A call the library
refuses is recorded by its message, which must agree as well."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synthetic_cpep(n, seed):
    import bench
    tp, G, c0, age, t2dm, beta, rng = bench.synthetic_population(n, seed)
    shape = np.array([1.0, 2.6, 3.1, 2.7, 2.2])         # a meal response, scaled per subject; no device solve involved
    obs = c0[:, None] * (1.0 + (shape[None, :] - 1.0) * np.exp(0.4 * beta)[:, None]) * (1.0 + 0.05 * rng.standard_normal((n, 5)))
    obs[:, 0] = c0
    return dict(tp=tp, G=G, obs=obs, age=age, t2dm=t2dm, cond=beta + 0.3 * rng.standard_normal(n), rng=rng)


def run(lib_path, out_path):
    import torch  # noqa: F401  (first: shared HIP runtime)
    sys.path.insert(0, os.path.join(ROOT, "conditional-ude_amd"))
    sys.path.insert(0, ROOT)
    from cude import _lib
    _lib.LIB_PATH = os.path.abspath(lib_path)
    import bench
    from cude.engine import Engine
    out = {}

    def keep(tag, value):
        if isinstance(value, dict):
            for k, v in value.items():
                keep(f"{tag}.{k}", v)
        elif isinstance(value, (tuple, list)):
            for k, v in enumerate(value):
                keep(f"{tag}.{k}", v)
        elif value is not None:
            out[tag] = np.asarray(value)

    def call(tag, fn):
        try:
            keep(tag, fn())
        except Exception as e:      # a refusal (an unsupported shape, say) is a result too
            keep(tag + ".error", np.frombuffer(str(e).encode(), dtype=np.uint8))

    cases = [("cpep", N, mode) for N in (57, 700) for mode in ("split", "onelane", "adaptive")] + \
            [("supp", 57, mode) for mode in ("fixed", "adaptive")]
    for model, N, mode in cases:
        cpep = model == "cpep"
        arch = (2, 6, 2) if cpep else (4, 3, 5)
        nn = bench.glorot(arch, 99)
        n_state = (2 if mode == "adaptive" else 3) if cpep else None
        eng = Engine(model, arch, n_steps=0 if mode == "adaptive" else 30, n_state=n_state)
        if mode == "onelane":
            eng.set_option("cpep_path", 1)
        if cpep:
            pop = synthetic_cpep(N, 780 + N)
            eng.set_population_cpep(pop["tp"], pop["G"], pop["obs"], pop["age"], pop["t2dm"])
            tp, cond, rng = pop["tp"], pop["cond"], pop["rng"]
        else:
            tp, data, cond = bench.synthetic_suppression(N, 7)
            cond = 0.5 * cond
            eng.set_population_supp(tp, data)
            rng = np.random.default_rng(11)
        P = eng.P
        sets = cond[None, :] + 0.2 * rng.standard_normal((7, N))
        nn_sets = nn[None, :] * (1.0 + 0.05 * rng.standard_normal((7, P)))
        weights = rng.random((7, N))
        times = np.sort(np.concatenate([[tp[0], tp[-1], 0.37 * tp[-1], 0.37 * tp[-1]], np.linspace(tp[0], tp[-1], 13)[1:-1]]))
        values = np.linspace(-2.5, 1.5, 9)
        cov = np.eye(P) * 0.01 + 0.001
        z, u = rng.standard_normal((11, N)), rng.random((11, N))
        nodes, logw = np.array([-1.7, -0.6, 0.0, 0.6, 1.7]), np.log(np.array([0.05, 0.25, 0.4, 0.25, 0.05]))
        # the replicate simulations: 9 replicates / simulations, 3 groups with one subject left out
        rep_rng = np.random.default_rng(2024 + N)
        B, R = 9, len(tp) - 1
        sigma = 0.05 * (1.0 + rep_rng.random(N))
        boot_noise = rep_rng.standard_normal((B, eng._residual_rows(), N))
        sim_sets = cond[None, :] + 0.3 * rep_rng.standard_normal((B, N))
        sim_noise = rep_rng.standard_normal((B, R, N))
        groups = (np.arange(N) % 3).astype(np.int32)
        groups[N // 2] = -1

        def candidates(first, count):
            r = np.random.default_rng(1000 + first)
            return nn[None, :] * (1.0 + 0.05 * r.standard_normal((count, P))), cond[None, :] + 0.3 * r.standard_normal((count, N))

        for chunked in (False, True):
            tag = f"{model}{N}.{mode}.{'chunked' if chunked else 'whole'}"
            for name, value in (("dense_chunk", 5), ("profile_chunk", 3), ("predictive_subjects", 64), ("predictive_times", 4),
                                ("bootstrap_chunk", 2), ("bootstrap_subjects", 64), ("npde_subjects", 64), ("vpc_sims", 2),
                                ("vpc_select", 1)):
                eng.set_option(name, value if chunked else 0)
            eng.set_params(nn, cond)
            call(tag + ".simulate", lambda: eng.simulate(times))
            call(tag + ".predictive_bands", lambda: eng.predictive_bands(sets, times, [0, 3, 6], state=0))
            call(tag + ".evaluate_conditional_sets", lambda: eng.evaluate_conditional_sets(sets, 0.1, -0.5, want_sse=True))
            call(tag + ".marginal.rule", lambda: eng.marginal_likelihood(0.3, -0.6, 0.9, nodes=nodes, log_weights=logw, scale=0.4,
                                                                          want_points=True, want_terms=True))
            eng.set_rng(12345, 0)
            call(tag + ".marginal.draws", lambda: eng.marginal_likelihood(0.3, -0.6, 0.9, n_draws=7, first_step=3, scale=0.4,
                                                                           want_points=True, want_terms=True))
            call(tag + ".subject_scores", lambda: eng.subject_scores(sets, weights))
            call(tag + ".subject_scores.own", lambda: eng.subject_scores())
            call(tag + ".network_information", lambda: eng.network_information(
                penalty_weight=0.2, cov=cov, profiled=True, want=Engine.INFO_OUTPUTS))
            call(tag + ".network_information.cond", lambda: eng.network_information(cond=sets[1]))
            call(tag + ".sensitivity", lambda: eng.sensitivity())
            call(tag + ".curvature", lambda: eng.curvature())
            call(tag + ".multistart_forward", lambda: eng.multistart_forward(nn_sets, sets))
            call(tag + ".screen_candidates", lambda: eng.screen_candidates(40, 5, candidates))
            call(tag + ".multistart_loss_grad", lambda: eng.multistart_loss_grad(nn_sets, sets))
            call(tag + ".profile_conditional", lambda: eng.profile_conditional(values))
            call(tag + ".profile_intervals", lambda: eng.profile_intervals(values, delta=1.9, penalty_weight=0.1,
                                                                            penalty_center=-0.5, rounds=3, sections=3))
            call(tag + ".profile_intervals.argmin", lambda: eng.profile_intervals(values, argmin_only=True))
            for spec in ((0, -1, 2) if not chunked else (-1,)):
                eng.set_option("fit_spec", spec)
                call(tag + f".fit_conditional.spec{spec}", lambda: eng.fit_conditional(-4.0, 3.0, 11, 9, 0.1, -0.5))
            call(tag + ".refine_conditional", lambda: eng.refine_conditional(max_evals=8, penalty_weight=0.1, penalty_center=-0.5))
            call(tag + ".refine_conditional.x0", lambda: eng.refine_conditional(x0=sets[2], max_evals=8))
            eng.set_params(nn, cond)
            eng.set_rng(4242, 0)
            call(tag + ".bootstrap_conditional.noise", lambda: eng.bootstrap_conditional(
                sigma, B, ranks=[0, 4, 8], noise=boot_noise, max_evals=8, penalty_weight=0.1, penalty_center=-0.5, want_replicates=True))
            call(tag + ".bootstrap_conditional.draws", lambda: eng.bootstrap_conditional(
                sigma, B, center=sets[1], first_rep=5, max_evals=8, want_replicates=True))
            call(tag + ".bootstrap_noise", lambda: eng.bootstrap_noise(5, B))
            call(tag + ".npde.given", lambda: eng.npde(sigma, B, sim_sets, noise=sim_noise, want_sims=True))
            call(tag + ".npde.draws", lambda: eng.npde(sigma, B, prior_mean=-0.6, prior_sd=0.9, first_rep=3, want_sims=True))
            call(tag + ".npde_draws", lambda: eng.npde_draws(3, B))
            call(tag + ".vpc.given", lambda: eng.vpc(sigma, B, sim_sets, noise=sim_noise, groups=groups, n_groups=3))
            call(tag + ".vpc.draws", lambda: eng.vpc(sigma, B, prior_mean=-0.6, prior_sd=0.9, first_rep=3, groups=groups, n_groups=3))
            if chunked:
                continue
            for gamma in (1.0, 0.35):
                for spec in (0, 2, -1):
                    eng.set_option("mh_spec", spec)
                    eng.set_params(nn, cond)
                    call(tag + f".mh_chain.g{gamma}.spec{spec}", lambda: eng.mh_chain(z, u, 0.3, -0.6, 0.9, 0.2, 1.0, gamma))
                    eng.set_rng(777, 0)
                    call(tag + f".mh_estep.g{gamma}.spec{spec}", lambda: eng.mh_estep(None, None, 0.3, -0.6, 0.9, 0.2, 1.0, gamma, n_mc=11))
                    call(tag + f".mh_estep.g{gamma}.spec{spec}.state", lambda: eng.get_params())
            if mode == "adaptive":      # once more in a re-grouped launch order
                eng.set_params(nn, cond)
                call(tag + ".regroup.loss_grad", lambda: eng.loss_grad())
                call(tag + ".regroup", lambda: eng.adaptive_regroup())
                call(tag + ".regroup.simulate", lambda: eng.simulate(times))
                call(tag + ".regroup.predictive_bands", lambda: eng.predictive_bands(sets, times, [0, 3, 6], state=0))
                call(tag + ".regroup.subject_scores", lambda: eng.subject_scores(sets, weights))
                call(tag + ".regroup.mh_chain", lambda: eng.mh_chain(z, u, 0.3, -0.6, 0.9, 0.2, 1.0, 1.0))
        eng.close()
        print(f"{model} {N} {mode}: {len(out)} arrays so far", flush=True)
    np.savez(out_path, **out)
    n_err = sum(k.endswith(".error") for k in out)
    print(f"wrote {len(out)} arrays ({n_err} refusals) to {out_path}")


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        if a[k].shape != b[k].shape or a[k].dtype != b[k].dtype or not np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"):
            bad.append(k)
    refusals = [k for k in a.files if k.endswith(".error")]
    print(f"{len(a.files)} / {len(b.files)} arrays, {len(refusals)} refusals, {len(bad)} differ")
    for k in refusals:
        print("  refused:", k, bytes(a[k]).decode()[:100])
    for k in bad:
        print("  DIFFERS:", k)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "cmp":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
