"""Inputs, 50-digit references and bars for the numerics probe (tests/hip/numerics_probe.hip, run on the device by
tests/test_gpu_numerics.py) and its host twin (tests/hip/numerics_twin.cpp, tests/test_math_host.py).

The elementwise bars are the host twin's maxima on the inputs below (noted next to each bar), rounded up by less than
2x; the device must meet the same bars.  The network bar is NET_C u S: u = 2^-53 and S the absolute-value propagation
of the evaluation (|W| |h| + |b| per layer, each activation adding one unit of its own error), computed alongside the
50-digit value."""
import ctypes
import os
import subprocess

import mpmath
import numpy as np

HIP_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip")
U = 2.0 ** -53
DPS = 50

# probe_elementwise / twin_elementwise operations
TANH, TANH_TAB, EXP2X, EXP2X_CS, SOFTPLUS, SOFTPLUS_LONE, RCP = range(7)
OP_NAMES = ["m_tanh", "m_tanh_tab", "m_exp2x_t<false>", "m_exp2x_t<true>", "m_softplus_t<false>", "m_softplus_t<true>",
            "m_rcp"]
# probe_layer kinds
L_TANH_EXP, L_TANH_TAB, L_RELU, L_SIGMOID, L_TANH_FROM_EXP = range(5)
LAYER_NAMES = ["m_tanh_vec", "m_tanh_vec_tab", "relu", "sigmoid", "m_tanh_from_exp"]

# Elementwise bars: (value, logistic derivative).  Error measures: tanh forms absolute; exponential and reciprocal
# relative; softplus |y - ref| / max(1, |ref|) (as tests/test_math_host.py), its derivative absolute.
ELEM_BARS = {                           # host twin maxima on elementwise_inputs():
    TANH: (4.5e-16, None),              # 3.03e-16
    TANH_TAB: (4.5e-16, None),          # 2.87e-16
    EXP2X: (6.5e-16, None),             # 4.48e-16
    EXP2X_CS: (6.5e-16, None),          # 4.48e-16
    SOFTPLUS: (4.5e-16, 4.5e-16),       # 2.48e-16, 2.57e-16
    SOFTPLUS_LONE: (4.5e-16, 4.5e-16),  # 2.68e-16, 2.42e-16
    RCP: (2.2e-16, None),               # 1.11e-16
}
# Layer bars (absolute): W units through one shared reciprocal, W = 1..8 on layer_inputs() (host twin maxima in the
# comments; relu is exact; the logistic layer is device code only: its bar is the exponential form's).  The derivative
# act_hidden_deriv is formed from the layer's own output and compared with the exact derivative at z (twin: 1.14e-15).
LAYER_BARS = {L_TANH_EXP: 1.1e-15,      # 5.73e-16
              L_TANH_TAB: 8.5e-16,      # 4.44e-16
              L_RELU: 0.0,
              L_SIGMOID: 1.1e-15,
              L_TANH_FROM_EXP: 1.1e-15}  # 5.55e-16
DERIV_BAR = 2.2e-15
NET_C = 16                               # network value and gradient: error <= NET_C * u * S (device maximum 5.3)
ULP_AGREE = 2                            # device vs host twin, per element


def build(*targets, timeout=300):
    """Builds the probe and the host twin (or the given targets) through tests/hip/Makefile: make rebuilds what is
    missing or older than its sources or the product headers."""
    jobs = min(16, os.cpu_count() or 4)
    subprocess.run(["make", "-s", "-C", HIP_DIR, f"-j{jobs}", *targets], check=True, timeout=timeout)


def _lib(name, protos):
    lib = ctypes.CDLL(os.path.join(HIP_DIR, name))
    for fn, args in protos.items():
        f = getattr(lib, fn)
        f.argtypes = args
        f.restype = ctypes.c_int
    return lib


def load_twin():
    P, I = ctypes.c_void_p, ctypes.c_int
    return _lib("libnumerics_twin.so", {"twin_elementwise": [I, P, P, P, I], "twin_tanh_table": [P, I],
                                        "twin_layer": [I, I, P, P, I]})


def load_probe(path=None):
    P, I = ctypes.c_void_p, ctypes.c_int
    return _lib(path or "libnumerics_probe.so", {
        "probe_elementwise": [I, P, P, P, I], "probe_tanh_table": [P, I], "probe_layer": [I, I, P, P, P, I],
        "probe_net_info": [I, I, I, I, I, I, P],
        "probe_net": [I, I, I, I, I, I, P, P, P, I, I, P, P, P, P, P],
        "probe_param_check": [I, I, I, I, I, I, P, I, P]})


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def elementwise(fn, op, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y, s = np.empty_like(x), np.empty_like(x)
    rc = fn(op, ptr(x), ptr(y), ptr(s), x.size)
    assert rc == 0, (OP_NAMES[op], rc)
    return y, s


# ------------------------------------------------------------------------------------ inputs
def _steps(points, k=2):
    """every point and its neighbours up to k ulps away on either side"""
    p = np.asarray(points, dtype=np.float64)
    out = [p]
    up, dn = p.copy(), p.copy()
    for _ in range(k):
        up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
        out += [up, dn]
    return np.concatenate(out)


def _both_signs(a):
    return np.concatenate([a, -a])


SPECIALS = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308, -2.2250738585072014e-308,
                     709.0, -709.0, 710.0, -710.0, 1e300, -1e300, np.inf, -np.inf])
LN2_HALF = 0.34657359027997265470861606072908828      # ln2/2: the step of the exponential's range reduction
X_SQRT2 = 0.88137358701954302523260932497979230       # |x| where 1 + exp(-|x|) = sqrt2 (softplus branch)


def elementwise_inputs(op, seed=20261016, n_rand=6000):
    """log-uniform random points plus the edges of the primitive (grid points, midpoints, clamps, branch and
    range-reduction switch points, each +-1 and +-2 ulp; zeros, subnormals, huge values, infinities)"""
    rng = np.random.default_rng(seed + op)
    if op in (TANH, TANH_TAB):
        r = 10.0 ** rng.uniform(-9, 2.5, n_rand) * rng.choice([-1.0, 1.0], n_rand)
        k = np.arange(161.0)
        grid = np.concatenate([k / 8, (k + 0.5) / 8, (k[1:] - 0.5) / 8])
        edges = _both_signs(_steps(np.concatenate([grid, [20.0]])))
        return np.concatenate([r, edges, SPECIALS])
    if op in (EXP2X, EXP2X_CS):             # contract: x in [-354, 354]
        r = np.concatenate([rng.uniform(-354, 354, n_rand // 2),
                            10.0 ** rng.uniform(-9, 2.5, n_rand // 2) * rng.choice([-1.0, 1.0], n_rand // 2)])
        n = np.concatenate([np.arange(-1022, 1022, 7), np.arange(-8, 8)])
        switch = (n + 0.5) * LN2_HALF           # x * 2 log2(e) = n + 1/2
        edges = _steps(np.concatenate([switch, [354.0, -354.0, -350.0, 350.0]]))
        edges = edges[np.abs(edges) <= 354.0]
        return np.concatenate([r, edges, [0.0, -0.0, 5e-324, -5e-324, 1e-310]])
    if op in (SOFTPLUS, SOFTPLUS_LONE):
        r = 10.0 ** rng.uniform(-9, 3, n_rand) * rng.choice([-1.0, 1.0], n_rand)
        n = np.arange(-1010, 0, 9)
        switch = -2 * (n + 0.5) * LN2_HALF      # -|x|/2 at a switch point of the exponential of exp(-|x|)
        edges = _both_signs(_steps(np.concatenate([[X_SQRT2, 700.0], switch])))
        return np.concatenate([r, edges, SPECIALS])
    if op == RCP:                                   # contract: d in [1, 1e290]
        r = 10.0 ** rng.uniform(0, 290, n_rand)
        p2 = 2.0 ** np.arange(0, 963)
        edges = _steps(np.concatenate([p2[::5], [1e290, 1.5, 3.0]]))
        edges = edges[(edges >= 1.0) & (edges <= 1e290)]
        return np.concatenate([r, edges])
    raise ValueError(op)


# ------------------------------------------------------------------------------------ references
def _mp(x):
    return mpmath.mpf(float(x))


def elementwise_errors(op, x, y, sig=None):
    """per-element errors of (y, sig) against the 50-digit reference, in the measures of ELEM_BARS"""
    ev = np.zeros(x.size)
    es = np.zeros(x.size)
    with mpmath.workdps(DPS):
        for i, (xv, yv) in enumerate(zip(x.tolist(), y.tolist())):
            if op in (TANH, TANH_TAB):
                ref = mpmath.tanh(_mp(xv)) if np.isfinite(xv) else mpmath.mpf(np.sign(xv))
                ev[i] = abs(float(_mp(yv) - ref)) if np.isfinite(yv) else np.inf
            elif op in (EXP2X, EXP2X_CS):
                ev[i] = abs(float(_mp(yv) / mpmath.exp(2 * _mp(xv)) - 1)) if np.isfinite(yv) else np.inf
            elif op == RCP:
                ev[i] = abs(float(_mp(yv) * _mp(xv) - 1)) if np.isfinite(yv) else np.inf
            else:
                sv = sig[i]
                if np.isinf(xv):                    # softplus(+Inf) = +Inf, softplus(-Inf) = 0; logistic 1, 0
                    ok = yv == np.inf if xv > 0 else (np.isfinite(yv) and abs(yv) <= 1e-300)
                    ev[i] = 0.0 if ok else np.inf
                    es[i] = abs(sv - (1.0 if xv > 0 else 0.0)) if np.isfinite(sv) else np.inf
                    continue
                xm = _mp(xv)
                ref = mpmath.log1p(mpmath.exp(xm)) if xv < 0 else xm + mpmath.log1p(mpmath.exp(-xm))
                sref = 1 / (1 + mpmath.exp(-xm))
                ev[i] = abs(float((_mp(yv) - ref) / max(1, abs(ref)))) if np.isfinite(yv) else np.inf
                es[i] = abs(float(_mp(sv) - sref)) if np.isfinite(sv) else np.inf
    return ev, es


def tanh_table_reference():
    """tanh(k/8), k = 0..160, correctly rounded to double"""
    with mpmath.workdps(DPS):
        return np.array([float(mpmath.tanh(mpmath.mpf(k) / 8)) for k in range(161)])


def ulp_distance(a, b):
    """|a - b| in units of the last place of max(|a|, |b|); 0 where a and b are the same double (NaN with NaN), inf
    where only one of them is finite or they are zeros of opposite sign"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    same = ((a == b) & (np.signbit(a) == np.signbit(b))) | (np.isnan(a) & np.isnan(b))
    m = np.maximum(np.abs(a), np.abs(b))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = np.abs(a - b) / np.spacing(np.where(np.isfinite(m), m, 1.0))
    d = np.where(np.isfinite(a) & np.isfinite(b), d, np.inf)
    return np.where(same, 0.0, d)


# ------------------------------------------------------------------------------------ layers
E_CLAMP = 2.35385266837019985408e17                   # m_tanh_from_exp's clamp of exp(2 z): z = 20


def layer_inputs(kind, W, seed=7, n_rand=48):
    """[n, W] pre-activations (kind L_TANH_FROM_EXP: E = exp(2 z)).  Random lanes, then lanes with one unit at 0, one
    at -0, one saturated and the rest random, and lanes with every unit at or beyond the clamp (the widest prefix
    product of the shared reciprocal), both signs."""
    rng = np.random.default_rng(seed + 10 * W + kind)
    z = 10.0 ** rng.uniform(-6, 1.6, (n_rand, W)) * rng.choice([-1.0, 1.0], (n_rand, W))
    mixed = z[:8].copy()
    mixed[:, 0] = [0.0, -0.0, 0.0, -0.0, 0.0, 0.0, -0.0, 0.0]
    if W > 1:
        mixed[:, -1] = [25.0, -25.0, 19.99, -300.0, 1e300, -1e300, 20.0, 40.0]
    clamp = [np.full(W, v) for v in (20.0, -20.0, np.nextafter(20.0, 0), np.nextafter(20.0, 99), 19.999, 21.0, -30.0,
                                     700.0, -1e300, 1e300)]
    alt = np.where(np.arange(W) % 2 == 0, 20.0, -20.0)
    z = np.concatenate([z, mixed, np.array(clamp), alt[None, :]])
    if kind == L_TANH_FROM_EXP:
        with np.errstate(over="ignore"):
            E = np.exp(2 * np.clip(z, -350, 350))
        E[-3] = E_CLAMP
        E[-2] = np.nextafter(E_CLAMP, np.inf)
        E[-4] = np.nextafter(E_CLAMP, 0)
        E[-5] = 0.0
        return E
    return z


def layer_reference(kind, z):
    """exact h of the layer and the exact derivative f'(z) (kind L_TANH_FROM_EXP: z holds E = exp(2 z))"""
    h = np.empty(z.shape)
    dh = np.empty(z.shape)
    with mpmath.workdps(DPS):
        for idx, v in np.ndenumerate(z):
            if kind == L_RELU:
                h[idx] = max(v, 0.0)
                dh[idx] = 1.0 if v > 0 else 0.0
                continue
            if kind == L_TANH_FROM_EXP:
                E = _mp(v)
                t = (E - 1) / (E + 1) if np.isfinite(v) else mpmath.mpf(1)
            elif kind == L_SIGMOID:
                t = 1 / (1 + mpmath.exp(-_mp(v)))
            else:
                t = mpmath.tanh(_mp(v))
            h[idx] = float(t)
            dh[idx] = float(t * (1 - t)) if kind == L_SIGMOID else float(1 - t * t)
    return h, dh


def tanh_deriv_from_output(h):
    """fma(-h, h, 1) of act_hidden_deriv (one rounding)"""
    with mpmath.workdps(DPS):
        return np.array([float(1 - _mp(v) * _mp(v)) for v in np.ravel(h)]).reshape(np.shape(h))


# ------------------------------------------------------------------------------------ networks
def net_reference(nin, nv, W, D, ha, oa, p, x, cst):
    """One evaluation of the network in the oracle's (SimpleChains) parameter layout -- layer l: W_l[j, i] at
    o + j + W i, bias at o + W n_in + j -- forward and reverse at 50 digits.  Returns the value, the gradient, dcond
    (cst0 d/dcst0) and dx, each with its scale S (the bar is NET_C u S).  S bounds first-order propagation plus the
    product of two errors (e2 = NET_C u): where a saturated unit's exact derivative vanishes, the rounded one does not,
    and the error of its input is all that is left downstream."""
    mp = mpmath.mpf
    P = p.size
    with mpmath.workdps(DPS):
        e2 = mp(NET_C) * mp(U)
        pm = [mp(float(v)) for v in p]
        pa = [abs(v) for v in pm]
        v = [mp(float(t)) for t in x] + [mp(float(t)) for t in cst]
        sv = [abs(t) for t in v]
        layers = []
        h, Sh = v, sv
        o = 0
        for l in range(D):
            n_in = nin if l == 0 else W
            hn, Shn, tau, Stau = [], [], [], []
            for j in range(W):
                z, S = pm[o + W * n_in + j], pa[o + W * n_in + j]
                for i in range(n_in):
                    z += pm[o + j + W * i] * h[i]
                    S += pa[o + j + W * i] * Sh[i]
                if ha == 0:                        # tanh: derivative 1 - h^2 from the output
                    t = mpmath.tanh(z)
                    St = (1 - t * t) * S + e2 * S * S + 1
                    tau.append(1 - t * t)
                    Stau.append(2 * abs(t) * St + 1)
                elif ha == 1:                      # relu
                    t = z if z > 0 else mp(0)
                    St = S
                    tau.append(mp(1) if z > 0 else mp(0))
                    Stau.append(mp(0))
                else:                              # logistic: derivative h (1 - h)
                    t = 1 / (1 + mpmath.exp(-z))
                    St = t * (1 - t) * S + e2 * S * S + 1
                    tau.append(t * (1 - t))
                    Stau.append(abs(1 - 2 * t) * St + 1)
                hn.append(t)
                Shn.append(St)
            layers.append((o, n_in, h, Sh, tau, Stau))
            o += W * n_in + W
            h, Sh = hn, Shn
        zo, Szo = pm[o + W], pa[o + W]
        for i in range(W):
            zo += pm[o + i] * h[i]
            Szo += pa[o + i] * Sh[i]
        if oa == 0:                                # softplus and its logistic derivative
            y = mpmath.log1p(mpmath.exp(zo)) if zo < 0 else zo + mpmath.log1p(mpmath.exp(-zo))
            sig = 1 / (1 + mpmath.exp(-zo))
            Sy = sig * Szo + max(1, abs(y))
            Ssig = 1 + sig * (1 - sig) * Szo + e2 * Szo * Szo
        else:
            y, sig, Sy, Ssig = zo, mp(1), Szo, mp(1)
        g, Sg = [mp(0)] * P, [mp(0)] * P
        g[o + W], Sg[o + W] = sig, Ssig
        dh, Sdh = [], []
        for i in range(W):
            g[o + i] = sig * h[i]
            Sg[o + i] = Ssig * (abs(h[i]) + e2 * Sh[i]) + sig * Sh[i]
            dh.append(sig * pm[o + i])
            Sdh.append(Ssig * pa[o + i])
        for ol, n_in, hp, Shp, tau, Stau in reversed(layers):
            d = [dh[j] * tau[j] for j in range(W)]
            Sd = [Sdh[j] * (tau[j] + e2 * Stau[j]) + abs(dh[j]) * Stau[j] for j in range(W)]
            for j in range(W):
                g[ol + W * n_in + j], Sg[ol + W * n_in + j] = d[j], Sd[j]
                for i in range(n_in):
                    g[ol + j + W * i] = d[j] * hp[i]
                    Sg[ol + j + W * i] = Sd[j] * (abs(hp[i]) + e2 * Shp[i]) + abs(d[j]) * Shp[i]
            dh = [mpmath.fsum(pm[ol + j + W * i] * d[j] for j in range(W)) for i in range(n_in)]
            Sdh = [mpmath.fsum(pa[ol + j + W * i] * Sd[j] for j in range(W)) for i in range(n_in)]
        if nin > nv:
            dcond, Sdcond = v[nv] * dh[nv], sv[nv] * Sdh[nv]
        else:
            dcond, Sdcond = mp(0), mp(0)

        def f(a):
            return np.array([float(t) for t in a])
        return dict(y=float(y), Sy=float(Sy), g=f(g), Sg=f(Sg), dcond=float(dcond), Sdcond=float(Sdcond),
                    dx=f(dh[:nv]), Sdx=f(Sdh[:nv]))
