"""Host-side mirror of the reference's Julia API for the accelerated path (same names, argument
meaning and error behaviour), implemented on top of the C ABI (libcude_hip.so).  No numerics live
here except optimiser bookkeeping on small vectors; every loss, gradient and trajectory comes from
the HIP kernels, and a missing library / GPU raises CudeError (there is no CPU fallback).

Reference items mirrored (paths relative to the reference repo):
  chain / softplus                         src/neural-network.jl:13-15,42-58,85-87,105-107
  neural_network_model                     suppression/src/suppression_model.jl:78-85
  CPeptideConditionalUDEModel (+Covariate) src/c-peptide-models.jl:170-220, src/types.jl:16-19
  CPeptideUDEModel, its loss and train     src/c-peptide-models.jl:76-84,144-168; src/parameter-estimation.jl:56-68,144-159,205-247
  loss / loss_sigma (3 methods each)       src/parameter-estimation.jl:56-75,93-109,126-140
  initial_parameters                       src/parameter-estimation.jl:22-24,36-38
  train (population / fixed-NN), train_with_sigma, evaluate_model
                                           src/parameter-estimation.jl:272-307,340-433
  suppression_loss / simul / fit_suppression_model
                                           suppression/src/suppression_model.jl:107-177
  individual_log_likelihood / mcmc_step / total_nll / update_population_parameters / SAEM
                                           src/saem.jl:55-66,86-131,134-237
  likelihood_profile                       src/likelihood-profiles.jl:4-17
  CPeptideODEModel / production (symbolic) src/c-peptide-models.jl:68-75,118-142; c-peptide/03-symreg.jl:37-40
  train_symbolic (per-subject k, sigma)    c-peptide/03-symreg.jl:94-106
  SAEM_symbolic                            src/saem-symreg.jl:31-66,86-131,134-229
Discretisation: every function here solves, like the reference, with ADAPTIVE Tsit5 at OrdinaryDiffEq's default
tolerances unless told otherwise (`default_steps`; the gradient is that of the accepted step sequence taken as fixed
arithmetic, which is what ForwardDiff through `solve` yields up to the controller's weighting of the partials,
INTEGRATION.md).  The fixed-step mode -- a smooth loss with an exact discrete adjoint and the time-split kernels for small
populations, 1e-4 ... 1e-3 away from the reference's values -- is the explicit fast option: `n_steps=
fixed_steps(timepoints)` (c-peptide: 8 steps per observation interval; suppression: 30) per call, or
`set_default_steps("fixed")` for the module.  julia/CUDEHip.jl has the same default and the same functions.
Deliberate differences, documented in DESIGN.md: gradients are a discrete adjoint instead of ForwardDiff; the
per-subject 1-D fits use a bracketing search instead of
Fminbox(LBFGS).
"""
import hashlib
import math
from collections import OrderedDict
from statistics import NormalDist
from types import SimpleNamespace

import numpy as np

from .engine import Engine
from .lbfgs import lbfgs, lbfgs_batched

DEFAULT_STEPS = 30
ADAPTIVE = 0      # n_steps = ADAPTIVE: the reference's own adaptive Tsit5 (abstol 1e-6, reltol 1e-3)
_DEFAULT_MODE = [ADAPTIVE]      # what default_steps returns: ADAPTIVE, "fixed" or a step count (set_default_steps)


def fixed_steps(timepoints, per_interval=8):
    """The fixed-step grid of the fast mode (`n_steps=fixed_steps(timepoints)`): `per_interval` Tsit5 steps per
    observation interval when the observation times are equidistant, so that every step boundary coincides with a knot
    of the piecewise-linear glucose forcing (on the Ohashi data S=32 is ~8x more accurate than S=30, whose steps
    straddle the knots at 30 and 90 min: max rel. trajectory error 6e-6 vs 5e-5); otherwise DEFAULT_STEPS.
    julia/CUDEHip.jl `fixed_steps` is the same rule."""
    tp = np.asarray(timepoints, dtype=np.float64)
    d = np.diff(tp)
    if tp.size >= 2 and np.allclose(d, d[0], rtol=1e-12, atol=0.0):
        return per_interval * (tp.size - 1)
    return DEFAULT_STEPS


def default_steps(timepoints=None, per_interval=8):
    """Discretisation of every function of this module whose caller passes no `n_steps`: ADAPTIVE -- the reference's
    `solve(prob, Tsit5())` at OrdinaryDiffEq's default tolerances (src/parameter-estimation.jl:59,
    suppression_model.jl:113,123, saem.jl:52), the mode that reproduces the reference's stored numbers (2e-9 on its 75
    stored suppression objectives).  The fixed-step mode (a smooth loss, exact discrete adjoint, time-split kernels for
    small populations; 1e-4 ... 1e-3 away from the reference's values) is asked for explicitly: `n_steps=
    fixed_steps(timepoints)` per call or `set_default_steps("fixed")` for the module.  julia/CUDEHip.jl
    `default_steps` / `set_default_steps!` are the same functions (tests/test_julia_shim.py compares the mirrors)."""
    mode = _DEFAULT_MODE[0]
    if mode == "fixed":
        if timepoints is None:
            return DEFAULT_STEPS
        return fixed_steps(timepoints, per_interval)
    return int(mode)


def set_default_steps(mode):
    """mode: ADAPTIVE (0, the default), "fixed" (fixed_steps(timepoints) per population; 30 for the suppression model)
    or a positive step count.  Returns the previous mode."""
    if not (mode == "fixed" or (isinstance(mode, (int, np.integer)) and mode >= 0)):
        raise ValueError('set_default_steps: ADAPTIVE (0), "fixed" or a positive step count')
    prev = _DEFAULT_MODE[0]
    _DEFAULT_MODE[0] = mode if mode == "fixed" else int(mode)
    return prev


# ----------------------------------------------------------------------------- network
def softplus(x):
    return np.log1p(np.exp(-np.abs(x))) + np.maximum(x, 0.0)


class Chain:
    """SimpleChain(static(input_dims), TurboDense{true}(tanh, width) x depth, TurboDense{true}(softplus, 1)).

    `widths` (unequal hidden widths, src/neural-network.jl:42-58): the network is carried as the equal-width network
    of width max(widths) whose extra units have zero weights, frozen by the library's parameter mask
    (cude_set_param_mask): parameter vectors have THAT layout (n_params entries, `mask` marks the live ones;
    pad_network / unpad_network convert to and from SimpleChains' own layout)."""

    def __init__(self, input_dims, width, depth, widths=None, activation="tanh", output_activation="softplus",
                 layer_activations=None):
        self.input_dims, self.width, self.depth = int(input_dims), int(width), int(depth)
        self.widths = None if widths is None else [int(w) for w in widths]
        # hidden tanh | relu | sigmoid, output softplus | identity: what the tuned kernels compile (the reference's
        # scripts build tanh / softplus networks only; src/neural-network.jl:42-58 accepts any function)
        self.activation, self.output_activation = activation, output_activation
        # the general form -- one activation function PER hidden layer, any of ACTIVATIONS, any widths: evaluated by the
        # library's fallback kernel (cude_set_network); parameter vectors then have SimpleChains' own layout, unpadded
        self.layer_activations = None if layer_activations is None else [str(a) for a in layer_activations]
        if self.layer_activations is not None and self.widths is None:
            self.widths = [self.width] * self.depth

    @property
    def general(self):
        return self.layer_activations is not None

    @property
    def mask(self):
        """1 for the live entries of the padded parameter vector, 0 for the padding; None for equal widths."""
        if self.widths is None or self.general:
            return None
        n = sum(w * f + w for w, f in zip(self.widths + [1], [self.input_dims] + self.widths))
        return (pad_network(self.widths, np.ones(n), input_dims=self.input_dims)[1] != 0.0).astype(np.float64)

    @property
    def arch(self):
        if self.general:        # (Engine: (nn_in, [widths], [activation per hidden layer], output activation))
            return (self.input_dims, tuple(self.widths), tuple(self.layer_activations), self.output_activation)
        return (self.input_dims, self.width, self.depth)

    @property
    def key(self):
        if self.general:
            return self.arch
        return self.arch + (tuple(self.widths) if self.widths else ()) + (self.activation, self.output_activation)

    def configure(self, engine):
        """tell a fresh engine the activation functions (before the population is uploaded)"""
        if self.general:        # (the engine was built from `arch`: cude_set_network has been called)
            return
        if self.activation != "tanh":
            engine.set_option("hidden_activation", self.activation)
        if self.output_activation != "softplus":
            engine.set_option("output_activation", self.output_activation)

    @property
    def n_params(self):
        if self.general:
            return _layer_slices(self.input_dims, self.widths)[1]
        p, fan = 0, self.input_dims
        for _ in range(self.depth):
            p += self.width * fan + self.width
            fan = self.width
        return p + fan + 1


_HIDDEN = ("tanh", "relu", "sigmoid")
_OUTPUT = ("softplus", "identity")
ACTIVATIONS = ("tanh", "relu", "sigmoid", "softplus", "identity")       # the fallback kernel: any of these in any layer


def chain(width, depth=None, activation="tanh", *, input_dims=2, output_dims=1, output_activation="softplus"):
    """chain(width, depth, act) / chain(widths::Vector, act) / chain(widths, acts::Vector) (src/neural-network.jl:42-58,
    85-87, 105-107).  What the kernels implement is accepted: ONE activation function for all hidden layers out of tanh,
    relu, sigmoid (functions are recognised by name: `sigmoid` also as `σ`, `sigmoid_fast`), one output unit with softplus
    or identity; unequal hidden widths with tanh / softplus only (zero-padded + masked, class Chain)."""
    if isinstance(width, (list, tuple, np.ndarray)):
        widths = list(width)
        if depth is not None and not isinstance(depth, (int, np.integer)):
            activation = depth
        if len(widths) == 0:
            raise ValueError("Input widths must be non-empty.")
        if output_dims != 1:
            raise NotImplementedError("the models of the reference use ONE network output (output_dims = 1)")
        per_layer = None
        if isinstance(activation, (list, tuple)):
            if len(activation) != len(widths):
                raise ValueError("The number of widths must match the number of activation functions.")
            per_layer = [_act_name(a) for a in activation]
            if len(set(per_layer)) == 1:
                activation, per_layer = per_layer[0], None
        out = _act_name(output_activation)
        act = None if per_layer is not None else _act_name(activation)
        # what only the fallback kernel evaluates: different functions per layer, softplus / identity hidden layers, other
        # output functions, unequal widths with anything but tanh / softplus
        if (per_layer is not None or act not in _HIDDEN or out not in _OUTPUT
                or (len(set(widths)) != 1 and (act != "tanh" or out != "softplus"))):
            names = per_layer if per_layer is not None else [act] * len(widths)
            bad = [a for a in names + [out] if a not in ACTIVATIONS]
            if bad:
                raise NotImplementedError(f"activation functions of the library: {ACTIVATIONS} (got {bad})")
            return Chain(input_dims, max(widths), len(widths), widths=widths, output_activation=out, layer_activations=names)
        if len(set(widths)) != 1:
            return Chain(input_dims, max(widths), len(widths), widths=widths)     # zero-padded + masked (class Chain)
        width, depth = widths[0], len(widths)
    act, out = _act_name(activation), _act_name(output_activation)
    if output_dims != 1:
        raise NotImplementedError("the models of the reference use ONE network output (output_dims = 1)")
    if act not in _HIDDEN or out not in _OUTPUT:
        if act not in ACTIVATIONS or out not in ACTIVATIONS:
            raise NotImplementedError(f"activation functions of the library: {ACTIVATIONS} (got {act!r}, {out!r})")
        return Chain(input_dims, width, depth, output_activation=out, layer_activations=[act] * int(depth))
    return Chain(input_dims, width, depth, activation=act, output_activation=out)


def _layer_slices(input_dims, widths):
    """(weight slice, bias slice, out, in) of every layer of a SimpleChains parameter vector, output layer last."""
    out, at, fan = [], 0, int(input_dims)
    for w in list(widths) + [1]:
        out.append((slice(at, at + w * fan), slice(at + w * fan, at + w * fan + w), w, fan))
        at += w * fan + w
        fan = w
    return out, at


def pad_network(widths, params, *, input_dims=2):
    """Unequal hidden widths, `chain([w1, w2, ...], tanh)` (src/neural-network.jl:42-58), on kernels that are compiled
    for equal widths: the network IS the equal-width network of width W = max(widths) whose extra units have zero
    weights and biases: nothing they compute reaches the output, and the gradient entries touching them vanish --
    exactly for the weights into a padded unit, at the rounding of the device's tanh(0) (~1e-16) for the weights
    leaving one.  Use it for loss / gradient / simulation calls and optimise in the UNPADDED parameters (gradient =
    unpad_network(gradient of the padded network): exact).  The library's own optimisers (train, cude_train_restarts)
    work on the padded vector, and Adam's scale invariance amplifies those ~1e-17 gradients until the padding comes
    alive: they then train the equal-width network, not the unequal-width one (tests/test_gpu_api.py).
    Returns (Chain(input_dims, W, depth), padded parameter vector)."""
    widths = [int(w) for w in widths]
    p = np.asarray(params, dtype=np.float64).reshape(-1)
    small, n_small = _layer_slices(input_dims, widths)
    if p.size != n_small:
        raise ValueError(f"expected {n_small} parameters for widths {widths}, got {p.size}")
    W = max(widths)
    big, n_big = _layer_slices(input_dims, [W] * len(widths))
    out = np.zeros(n_big)
    for (ws, bs, o, i), (wb, bb, ob, ib) in zip(small, big):
        M = np.zeros((ob, ib))
        M[:o, :i] = p[ws].reshape(i, o).T                    # SimpleChains stores W column-major: vec(W)[j + o*k] = W[j,k]
        out[wb] = M.T.reshape(-1)
        out[bb][:o] = p[bs]
    return Chain(input_dims, W, len(widths)), out


def unpad_network(widths, padded, *, input_dims=2):
    """Inverse of pad_network for a parameter (or gradient) vector of the padded network."""
    widths = [int(w) for w in widths]
    P = np.asarray(padded, dtype=np.float64).reshape(-1)
    small, n_small = _layer_slices(input_dims, widths)
    big, n_big = _layer_slices(input_dims, [max(widths)] * len(widths))
    if P.size != n_big:
        raise ValueError(f"expected {n_big} parameters of the padded network, got {P.size}")
    out = np.empty(n_small)
    for (ws, bs, o, i), (wb, bb, ob, ib) in zip(small, big):
        out[ws] = P[wb].reshape(ib, ob).T[:o, :i].T.reshape(-1)
        out[bs] = P[bb][:o]
    return out


def _act_name(a):
    name = a if isinstance(a, str) else getattr(a, "__name__", str(a))
    return {"σ": "sigmoid", "sigmoid_fast": "sigmoid", "tanh_fast": "tanh", "identity": "identity"}.get(name, name)


def neural_network_model(depth, width, *, input_dims=2):
    return Chain(input_dims, width, depth)


def init_params(net, rng=None):
    """SimpleChains.init_params restated.  A `TurboDense{true}` layer keeps weights and bias in ONE out x (in + 1)
    matrix [W b] and initialises all of it Glorot-normal, sigma = sqrt(2 / (out + in + 1)) -- the biases are random
    too.  (SimpleChains is third-party; this reading is the one under which the reference's suppression experiment
    is reproduced in distribution -- with zero biases 4 ... 9 of the 25 kept runs stall on the constant-production
    plateau above 0.7, which none of the reference's 125 stored runs does: profiles/r02/e2e_suppression.txt.)"""
    rng = np.random.default_rng() if rng is None else rng
    parts, fan = [], net.input_dims
    for out in (net.widths if getattr(net, "widths", None) else [net.width] * net.depth) + [1]:
        sigma = math.sqrt(2.0 / (out + fan + 1))
        parts += [rng.standard_normal(out * fan) * sigma, rng.standard_normal(out) * sigma]
        fan = out
    p = np.concatenate(parts)
    if getattr(net, "general", False):
        return p
    return pad_network(net.widths, p, input_dims=net.input_dims)[1] if getattr(net, "widths", None) else p


def ComponentArray(**kw):
    """ComponentArrays.ComponentArray stand-in: attribute access to named parts (neural, conditional, ...)."""
    return SimpleNamespace(**{k: (np.array(v, dtype=np.float64) if not np.isscalar(v) else float(v)) for k, v in kw.items()})


class OptimizationSolution(SimpleNamespace):
    """Fields used downstream of `train` in the reference: .u (ComponentArray) and .objective."""


# ----------------------------------------------------------------------------- c-peptide models
class CPeptideConditionalUDEModel:
    """CPeptideConditionalUDEModel(glucose, timepoints, age, chain, cpeptide, t2dm) -- holds one subject's data;
    the ODE problem itself lives on the GPU once the subject is part of a population."""

    def __init__(self, glucose_data, glucose_timepoints, age, network, cpeptide_data, t2dm, *, covariate=False):
        self.glucose = np.asarray(glucose_data, dtype=np.float64)
        self.timepoints = np.asarray(glucose_timepoints, dtype=np.float64)
        self.age = float(age)
        self.chain = network
        self.cpeptide = np.asarray(cpeptide_data, dtype=np.float64)
        self.t2dm = bool(t2dm)
        self.covariate = covariate
        if self.glucose.shape != self.timepoints.shape or self.cpeptide.shape != self.timepoints.shape:
            raise ValueError("glucose, cpeptide and timepoints must have the same length")
        if network.input_dims != (3 if covariate else 2):
            raise ValueError("network input_dims does not match the model (2: [dG, beta]; 3: [dG, beta, age])")
        self._key = _model_key(self, ("cude", network.key, covariate))


CPeptideCUDEModel = CPeptideConditionalUDEModel        # name used in the reference's docstrings / stale script


def embed_single_input(width, params):
    """Parameter (or mask) vector of a 1-input network -> that of its 2-input carrier: the first layer [vec(W1); b1]
    with W1 of shape W x 1 becomes W x 2 with a zero second column (column-major: W zeros behind the first W entries)."""
    q = np.asarray(params, dtype=np.float64).reshape(-1)
    return np.concatenate([q[:width], np.zeros(width), q[width:]])


def extract_single_input(width, carried):
    """Inverse of embed_single_input (parameters or gradients of the carrier -> those of the 1-input network)."""
    q = np.asarray(carried, dtype=np.float64).reshape(-1)
    return np.concatenate([q[:width], q[2 * width:]])


class CPeptideUDEModel:
    """CPeptideUDEModel(glucose, timepoints, age, chain(...; input_dims = 1), cpeptide, t2dm) -- the non-conditional
    UDE (src/c-peptide-models.jl:144-168): production = network([dG]) - network([0]) (neural_network_production,
    :76-84), parameters = the network's alone.

    On the device it IS the conditional model's kernel: the 1-input network is carried as the 2-input network whose
    first-layer weights of the second input are zero and frozen by the library's parameter mask, so that
    network([dG; e^beta]) == network([dG]) exactly (a product with an exact zero adds +0.0) and the conditional
    parameter -- kept at 0 -- has a vanishing gradient.  Parameter vectors handed in and out have the 1-input
    SimpleChains layout (embed_single_input / extract_single_input convert)."""

    def __init__(self, glucose_data, glucose_timepoints, age, network, cpeptide_data, t2dm):
        self.glucose = np.asarray(glucose_data, dtype=np.float64)
        self.timepoints = np.asarray(glucose_timepoints, dtype=np.float64)
        self.age = float(age)
        self.chain = network
        self.cpeptide = np.asarray(cpeptide_data, dtype=np.float64)
        self.t2dm = bool(t2dm)
        self.covariate = False
        if self.glucose.shape != self.timepoints.shape or self.cpeptide.shape != self.timepoints.shape:
            raise ValueError("glucose, cpeptide and timepoints must have the same length")
        if network.input_dims != 1:
            raise ValueError("network input_dims does not match the model (1: [dG])")
        W = network.width
        base = network.mask if network.mask is not None else np.ones(network.n_params)
        mask = embed_single_input(W, base)                     # (zero where the second input's weights sit)
        self._carrier = SimpleNamespace(arch=(2, W, network.depth), mask=mask, key=("ude",) + tuple(network.key),
                                        configure=network.configure)
        self._key = _model_key(self, ("ude", network.key))

    def embed(self, params):
        return embed_single_input(self.chain.width, params)

    def extract(self, carried):
        return extract_single_input(self.chain.width, carried)


def CPeptideConditionalCovariateUDEModel(glucose_data, glucose_timepoints, age, network, cpeptide_data, t2dm):
    return CPeptideConditionalUDEModel(glucose_data, glucose_timepoints, age, network, cpeptide_data, t2dm,
                                       covariate=True)


class MichaelisMentenProduction:
    """production(dG, k) = dG >= 0 ? 1.78dG/(dG + k[1]) : 0.0 -- the analytic production term found by symbolic
    regression (c-peptide/03-symreg.jl:37-40).  The reference passes an arbitrary Julia function to
    CPeptideODEModel; this is the one form compiled into the HIP kernel (vmax generalises the literal 1.78)."""

    def __init__(self, vmax=1.78):
        self.vmax = float(vmax)

    def __call__(self, dG, k):
        dG = np.asarray(dG, dtype=np.float64)
        k = np.asarray(k, dtype=np.float64)
        pos = dG >= 0
        return np.where(pos, self.vmax * dG / np.where(pos, dG + k, 1.0), 0.0)


production = MichaelisMentenProduction()


class CPeptideODEModel:
    """CPeptideODEModel(glucose, timepoints, age, production, cpeptide, t2dm) (src/c-peptide-models.jl:118-142):
    van Cauter kinetics + analytic production; the model parameter is the per-subject k."""

    def __init__(self, glucose_data, glucose_timepoints, age, production_function, cpeptide_data, t2dm):
        if not isinstance(production_function, MichaelisMentenProduction):
            raise NotImplementedError("only MichaelisMentenProduction (vmax*dG/(dG+k)) is compiled for the GPU")
        self.glucose = np.asarray(glucose_data, dtype=np.float64)
        self.timepoints = np.asarray(glucose_timepoints, dtype=np.float64)
        self.age = float(age)
        self.production = production_function
        self.cpeptide = np.asarray(cpeptide_data, dtype=np.float64)
        self.t2dm = bool(t2dm)
        if self.glucose.shape != self.timepoints.shape or self.cpeptide.shape != self.timepoints.shape:
            raise ValueError("glucose, cpeptide and timepoints must have the same length")
        self._key = _model_key(self, ("sym", production_function.vmax))


def _model_key(m, tag):
    """Content digest of one subject's model (what the device population is built from)."""
    h = hashlib.blake2b(repr(tag).encode(), digest_size=16)
    for a in (m.glucose, m.timepoints, m.cpeptide, [m.age, float(m.t2dm)]):
        h.update(np.ascontiguousarray(a, dtype=np.float64))
    return h.digest()


class _Pop:
    """Device-resident population built from a list of models (cached by content, see _population)."""

    def __init__(self, models, timepoints, cpeptide_data, n_steps, n_state, device, cond_space="log"):
        tp = np.asarray(timepoints, dtype=np.float64)
        for m in models:
            # the reference solves model.problem (glucose knots = the model's timepoints) and saves at `timepoints`;
            # the kernels take ONE grid for both
            if m.timepoints.shape != tp.shape or not np.array_equal(m.timepoints, tp):
                raise ValueError("timepoints must equal the timepoints the models were built with")
        if isinstance(models[0], CPeptideODEModel):
            self.engine = Engine("cpep_sym", n_steps=n_steps, n_state=n_state, device=device, cond_space=cond_space)
            self.shared = np.array([models[0].production.vmax])
        else:
            net = getattr(models[0], "_carrier", models[0].chain)      # (CPeptideUDEModel: its 2-input carrier)
            self.engine = Engine("cpep", net.arch, n_steps=n_steps, n_state=n_state, device=device)
            net.configure(self.engine)
            if net.mask is not None:
                self.engine.set_param_mask(net.mask)
        G = np.stack([m.glucose for m in models])
        cp = np.asarray(cpeptide_data, dtype=np.float64).reshape(len(models), -1)
        self.engine.set_population_cpep(tp, G, cp, [m.age for m in models], [m.t2dm for m in models])
        self.N, self.T = cp.shape


_CACHE = OrderedDict()        # content key -> population, least recently used first
_CACHE_MAX = 8                # engines kept alive; an evicted one is closed (stream + device buffers freed)
_DEVICE = 0


def set_device(device):
    global _DEVICE
    _DEVICE = int(device)


def clear_cache():
    for p in _CACHE.values():
        p.engine.close()
    _CACHE.clear()


def _cached(key, build):
    pop = _CACHE.get(key)
    if pop is None:
        pop = build()
        _CACHE[key] = pop
        while len(_CACHE) > _CACHE_MAX:
            _, old = _CACHE.popitem(last=False)
            old.engine.close()
    else:
        _CACHE.move_to_end(key)
    return pop


def _digest(*arrays):
    h = hashlib.blake2b(digest_size=16)
    for a in arrays:
        a = np.ascontiguousarray(a, dtype=np.float64)
        h.update(str(a.shape).encode())
        h.update(a)
    return h.digest()


def _population(models, timepoints, cpeptide_data, n_steps=None, n_state=2, cond_space="log"):
    """The device population of (models, timepoints, data), built once per CONTENT: the key is a digest of every
    model's data (a fresh list of the same models -- `[model]`, `[model] * steps` -- is the same population), of the
    time grid and of all observations, so that calling `loss` in a loop neither rebuilds nor leaks engines, and
    changed data is never answered from a stale population."""
    if n_steps is None:       # (fixed mode: the analytic production has a kink at dG = 0: twice the steps of the smooth model)
        n_steps = default_steps(timepoints, 16 if isinstance(models[0], CPeptideODEModel) else 8)
    cp = np.asarray(cpeptide_data, dtype=np.float64)
    h = hashlib.blake2b(digest_size=16)
    for m in models:
        h.update(m._key)
    key = ("cpep", len(models), h.digest(), int(n_steps), n_state, cond_space, _digest(timepoints, cp))
    return _cached(key, lambda: _Pop(models, timepoints, cp, n_steps, n_state, _DEVICE, cond_space))


def _is_model(x):
    return isinstance(x, (CPeptideConditionalUDEModel, CPeptideODEModel, CPeptideUDEModel))


def _first(theta):
    """theta[1] of a Julia ComponentArray(ode=[k], sigma=s) / vector / scalar."""
    return float(np.ravel(getattr(theta, "ode", theta))[0])


def loss(theta, args, *, n_steps=None):
    """loss(theta, (models, timepoints, cpeptide_data))            population, mean SSE (:126-140)
       loss(theta, (model, timepoints, cpeptide_data))             single subject SSE (:56-68)
       loss(beta,  (model, timepoints, cpeptide_data, nn_params))  single subject, fixed network (:93-99)
    Returns +Inf when any trajectory is non-finite (the reference's solver-failure convention)."""
    if len(args) == 4:
        model, timepoints, data, nn = args
        pop = _population([model], timepoints, np.asarray(data)[None, :], n_steps)
        pop.engine.set_params(nn, np.atleast_1d(np.asarray(theta, dtype=np.float64))[:1])
        out = pop.engine.forward(want_sse=True)
        return out["sse"][0] if np.isfinite(out["loss"]) else np.inf
    models, timepoints, data = args
    if isinstance(models, CPeptideUDEModel):        # theta = the network's parameters (:56-68 with neural_network_production)
        pop = _population([models], timepoints, np.asarray(data)[None, :], n_steps)
        pop.engine.set_params(models.embed(theta), [0.0])
        return pop.engine.forward()["loss"]           # N = 1: mean SSE == SSE
    if isinstance(models, CPeptideODEModel):        # p = theta, production(dG, p) reads p[1] (03-symreg.jl:38)
        pop = _population([models], timepoints, np.asarray(data)[None, :], n_steps, cond_space="raw")
        pop.engine.set_params(pop.shared, [_first(theta)])
        return pop.engine.forward()["loss"]
    if _is_model(models):
        pop = _population([models], timepoints, np.asarray(data)[None, :], n_steps)
        pop.engine.set_params(theta.neural, np.atleast_1d(theta.conditional)[:1])
        return pop.engine.forward()["loss"]           # N = 1: mean SSE == SSE
    pop = _population(models, timepoints, data, n_steps)
    pop.engine.set_params(theta.neural, np.asarray(theta.conditional).reshape(-1)[:pop.N])
    return pop.engine.forward()["loss"]


def loss_sigma(theta, args, *, n_steps=None):
    """(n/2) log sigma^2 + SSE / (2 sigma^2)   (src/parameter-estimation.jl:70-75,101-109)."""
    n = len(args[1])
    if len(args) == 4:
        err = loss(theta.ode, args, n_steps=n_steps)
    else:
        err = loss(theta, args, n_steps=n_steps)
    return (n / 2) * math.log(theta.sigma ** 2) + err / (2 * theta.sigma ** 2)


def loss_and_gradient(theta, args, *, n_steps=None):
    """Replaces ForwardDiff.gradient(loss, theta) (AutoForwardDiff, :370) for the population loss (and, for a
    CPeptideUDEModel, :232: value and gradient with respect to the network's parameters)."""
    models, timepoints, data = args
    if isinstance(models, CPeptideUDEModel):
        pop = _population([models], timepoints, np.asarray(data)[None, :], n_steps)
        pop.engine.set_params(models.embed(theta), [0.0])
        val, g_nn, _ = pop.engine.loss_grad()
        return val, models.extract(g_nn)
    pop = _population(models, timepoints, data, n_steps)
    pop.engine.set_params(theta.neural, np.asarray(theta.conditional).reshape(-1)[:pop.N])
    val, g_nn, g_cond = pop.engine.loss_grad()
    return val, ComponentArray(neural=g_nn, conditional=g_cond.reshape(np.asarray(theta.conditional).shape))


def initial_parameters(*args, rng=None):
    """initial_parameters(chain, n_initials; rng) -> list of network parameter vectors
       initial_parameters(n_models, lhs_lb, lhs_ub, n_initials, rng) -> (n_models x n_initials) Latin hypercube."""
    if isinstance(args[0], Chain):
        net, n = args[0], args[1]
        return [init_params(net, rng) for _ in range(n)]
    n_models, lb, ub, n = args[:4]
    rng = args[4] if len(args) > 4 else (np.random.default_rng() if rng is None else rng)
    # QuasiMonteCarlo.LatinHypercubeSample: one stratified draw per interval and dimension, shuffled
    u = (rng.permuted(np.tile(np.arange(n), (n_models, 1)), axis=1) + rng.random((n_models, n))) / n
    return lb + (ub - lb) * u


class _LatinHypercube:
    """QuasiMonteCarlo.LatinHypercubeSample(n_models x n_initials) generated column block by column block: the
    stratum permutations (int32) are drawn once, the jitter per block, so the (n_models x n_initials) sample itself
    is never held (above 2^28 entries even the permutations are dropped for independent uniform draws)."""

    def __init__(self, n_models, n, rng):
        self.n_models, self.n, self.rng = n_models, n, rng
        self.perm = rng.permuted(np.tile(np.arange(n, dtype=np.int32), (n_models, 1)), axis=1) \
            if n_models * n <= 2 ** 28 else None

    def columns(self, first, count):
        """(n_models, count) block of the unit-cube sample."""
        u = self.rng.random((self.n_models, count))
        return u if self.perm is None else (self.perm[:, first:first + count] + u) / self.n


class _Columns:
    """ode_inits[:, k] of the selected candidates only (the full table no longer exists)."""

    def __init__(self, cols):
        self.cols = cols

    def __getitem__(self, key):
        return self.cols[key[1]]


# ----------------------------------------------------------------------------- training drivers
def _adam_then_lbfgs(eng, nn0, cond0, adam_iters, lbfgs_iters, lr, callback=None):
    eng.set_params(nn0, cond0)
    eng.adam_init(lr)
    if callback is None and adam_iters > 0:
        trace = eng.adam_run(adam_iters)          # all iterations queued as one replayed hipGraph
        if not np.all(np.isfinite(trace)):
            raise FloatingPointError("solver failure (non-finite loss) during Adam")
    else:
        for _ in range(adam_iters):
            last = eng.adam_step()
            if callback(None, last):
                break
            if not np.isfinite(last):
                raise FloatingPointError("solver failure (non-finite loss) during Adam")
    nn, cond = eng.get_params()
    P = nn.size

    def fg(x):
        eng.set_params(x[:P], x[P:])
        val, g_nn, g_cond = eng.loss_grad()
        return val, np.concatenate([g_nn, g_cond])

    res = lbfgs(fg, np.concatenate([nn, cond]), maxiters=lbfgs_iters, callback=callback)
    return res["x"][:P], res["x"][P:], res["f"]


LM_STATUS = ("grad", "decrease", "stalled", "max_iters", "failed")      # cude_train_lm's status codes 0 ... 4, by name


def _second_stage(second_stage):
    if second_stage not in ("lbfgs", "lm"):
        raise ValueError('second_stage must be "lbfgs" or "lm"')
    return second_stage == "lm"


def _adam_then_lm(eng, nn0, cond0, adam_iters, lm_iters, lr, trace=None):
    """The Adam stage of _adam_then_lbfgs, then Levenberg-Marquardt on the expected-information matrices (cude_train_lm) in
    place of L-BFGS; it ends at a relative decrease of 1e-10 or after lm_iters iterations."""
    eng.set_params(nn0, cond0)
    if adam_iters > 0:
        eng.adam_init(lr)
        losses = eng.adam_run(adam_iters)
        if not np.all(np.isfinite(losses)):
            raise FloatingPointError("solver failure (non-finite loss) during Adam")
        if trace is not None:
            trace.extend(float(v) for v in losses)
    res = eng.train_lm(max_iters=lm_iters, ftol=1e-10)
    if LM_STATUS[res["status"]] == "failed":
        raise FloatingPointError("solver failure (non-finite loss or a failed subject) during Levenberg-Marquardt")
    if trace is not None:
        trace.extend(float(v) for v in res["trace"])
    nn, cond = eng.get_params()
    return nn, cond, float(res["trace"][-1])


def _batched_adam_then_lbfgs(eng, nn_inits, cond_inits, adam_iters, lbfgs_iters, lr, traces=None, native=True):
    """The K selected restarts trained SIDE BY SIDE instead of one after the other (the reference's loop,
    src/parameter-estimation.jl:372-383 / suppression_model.jl:140-170): every optimiser iteration evaluates the K
    current points with one cude_multistart_loss_grad launch.  Adam (Optimisers.jl update rule) is vectorised over
    the restarts; the K L-BFGS runs are the serial algorithm driven in lock step (cude.lbfgs.lbfgs_batched), so each
    restart follows the path it would follow alone.  A restart whose loss becomes non-finite during Adam is
    dropped, as the reference skips a failed optimisation.  Returns a list of (nn, cond, objective) or None."""
    if native:                                # the same two stages inside the library (cude_train_restarts)
        out = eng.train_restarts(nn_inits, cond_inits, adam_iters, lr, lbfgs_iters, want_trace=traces is not None)
        nn, cond, obj = out[:3]
        if traces is not None:
            for k in range(len(obj)):
                traces[k].extend(float(v) for v in out[3][k] if not np.isnan(v))
        return [(nn[k], cond[k], float(obj[k])) if np.isfinite(obj[k]) else None for k in range(len(obj))]
    X = np.concatenate([np.asarray(nn_inits, dtype=np.float64), np.asarray(cond_inits, dtype=np.float64)], axis=1)
    K, P = X.shape[0], eng.P
    alive = np.ones(K, bool)
    M, V = np.zeros_like(X), np.zeros_like(X)
    b1, b2, eps = 0.9, 0.999, 1e-8
    for t in range(1, adam_iters + 1):
        f, g_nn, g_cond = eng.multistart_loss_grad(X[:, :P], X[:, P:])
        alive &= np.isfinite(f)
        if traces is not None:
            for k in range(K):
                if alive[k]:
                    traces[k].append(float(f[k]))
        G = np.concatenate([g_nn, g_cond], axis=1)
        G[~alive] = 0.0
        M = b1 * M + (1 - b1) * G
        V = b2 * V + (1 - b2) * G * G
        step = lr * (M / (1 - b1 ** t)) / (np.sqrt(V / (1 - b2 ** t)) + eps)
        X[alive] -= step[alive]
    if not alive.any():
        return [None] * K
    idx = np.flatnonzero(alive)
    Xa = X[idx]

    def fg_batch(Xq):
        f, g_nn, g_cond = eng.multistart_loss_grad(Xq[:, :P], Xq[:, P:])
        return f, np.concatenate([g_nn, g_cond], axis=1)
    cbs = None if traces is None else [(lambda _x, l, k=k: traces[k].append(float(l)) and False) for k in idx]
    res = lbfgs_batched(fg_batch, Xa, maxiters=lbfgs_iters, callbacks=cbs)
    out = [None] * K
    for k, r in zip(idx, res):
        out[k] = (r["x"][:P], r["x"][P:], r["f"])
    return out


def train(models, timepoints, cpeptide_data, rng_or_nn, *, initial_guesses=None, selected_initials=None,
          lhs_lower_bound=-2.0, lhs_upper_bound=0.0, n_conditional_parameters=1, number_of_iterations_adam=1000,
          number_of_iterations_lbfgs=1000, learning_rate_adam=1e-2, initial_beta=-2.0, lbfgs_lower_bound=-4.0,
          lbfgs_upper_bound=1.0, lbfgs_iterations=1000, n_steps=None, side_by_side=True, method="search",
          second_stage="lbfgs"):
    """Three methods of the reference, selected by the types of the 1st and 4th argument as Julia's dispatch does:
    * a single CPeptideUDEModel + rng: the conventional UDE on one (mean) subject (:205-247): `initial_guesses`
      (default 10 000) initialisations screened by their loss, the best `selected_initials` (10) -> Adam -> L-BFGS.
    * rng (numpy Generator): population training, unknown network (:340-386): LHS + init screening of
      `initial_guesses` candidates (forward-only), best `selected_initials` -> Adam -> L-BFGS; the selected
      restarts are trained side by side (one launch per optimiser iteration for all of them) unless
      side_by_side=False.
    * array of network parameters: per-subject estimation of the conditional parameter with the network
      frozen (:272-288); `method` as estimate_conditional.
    second_stage="lm" (population training only): every selected restart runs its Adam iterations, then train_lm's
    Levenberg-Marquardt loop (at most number_of_iterations_lbfgs iterations) in place of L-BFGS, one restart after the other."""
    lm = _second_stage(second_stage)
    if isinstance(models, CPeptideUDEModel):
        return _train_ude(models, timepoints, cpeptide_data, rng_or_nn,
                          initial_guesses=10_000 if initial_guesses is None else initial_guesses,
                          selected_initials=10 if selected_initials is None else selected_initials,
                          number_of_iterations_adam=number_of_iterations_adam,
                          number_of_iterations_lbfgs=number_of_iterations_lbfgs, learning_rate_adam=learning_rate_adam,
                          n_steps=n_steps, side_by_side=side_by_side)
    initial_guesses = 25_000 if initial_guesses is None else initial_guesses
    selected_initials = 25 if selected_initials is None else selected_initials
    if isinstance(rng_or_nn, np.random.Generator):
        rng = rng_or_nn
        pop = _population(models, timepoints, cpeptide_data, n_steps)
        eng, N = pop.engine, pop.N
        # screening (:351-372): candidates are generated chunk by chunk and never held all at once; the losses and the
        # selection `partialsortperm(losses_initial, 1:selected_initials)` stay on the device (cude_screen_candidates)
        strata = _LatinHypercube(N, initial_guesses, rng)
        net = models[0].chain

        def candidates(first, count):
            nn = np.stack([init_params(net, rng) for _ in range(count)])
            return nn, lhs_lower_bound + (lhs_upper_bound - lhs_lower_bound) * strata.columns(first, count).T
        order, _, nn_sel, cond_sel = eng.screen_candidates(initial_guesses, selected_initials, candidates)
        nn_inits = dict(zip(order, nn_sel))
        ode_inits = _Columns(dict(zip(order, cond_sel)))
        sols = []
        if side_by_side and len(order) > 1 and not lm:
            fits = _batched_adam_then_lbfgs(eng, nn_sel, cond_sel,
                                            number_of_iterations_adam, number_of_iterations_lbfgs, learning_rate_adam)
            for fit in fits:
                if fit is None:
                    print("Optimization failed... Skipping")
                    continue
                nn, cond, obj = fit
                sols.append(OptimizationSolution(
                    u=ComponentArray(neural=nn, conditional=np.repeat(cond[:, None], n_conditional_parameters, 1)),
                    objective=obj))
            return sols
        for k in order:
            try:
                nn, cond, obj = (_adam_then_lm if lm else _adam_then_lbfgs)(
                    eng, nn_inits[k], ode_inits[:, k], number_of_iterations_adam, number_of_iterations_lbfgs,
                    learning_rate_adam)
                sols.append(OptimizationSolution(
                    u=ComponentArray(neural=nn, conditional=np.repeat(cond[:, None], n_conditional_parameters, 1)),
                    objective=obj))
            except FloatingPointError:
                print("Optimization failed... Skipping")
        return sols
    nn = np.asarray(rng_or_nn, dtype=np.float64)
    beta, sse = estimate_conditional(models, timepoints, cpeptide_data, nn, initial_beta=initial_beta,
                                     lower=lbfgs_lower_bound, upper=lbfgs_upper_bound, n_steps=n_steps, method=method)
    return [OptimizationSolution(u=np.array([b]), objective=s) for b, s in zip(beta, sse)]


def _train_ude(model, timepoints, cpeptide_data, rng, *, initial_guesses, selected_initials, number_of_iterations_adam,
               number_of_iterations_lbfgs, learning_rate_adam, n_steps, side_by_side):
    """train(model::CPeptideUDEModel, timepoints, cpeptide_data, rng) (src/parameter-estimation.jl:205-247): the
    screening loop, `partialsortperm(losses_initial, 1:selected_initials)` and the two optimiser stages of
    `_optimize` (:144-159) run through the same device paths as the conditional model's (cude_screen_candidates,
    cude_train_restarts) on a population of one subject; solutions carry the 1-input parameter vector."""
    if not isinstance(rng, np.random.Generator):
        raise TypeError("train(model::CPeptideUDEModel, timepoints, cpeptide_data, rng): rng must be a numpy Generator")
    pop = _population([model], timepoints, np.asarray(cpeptide_data, dtype=np.float64)[None, :], n_steps)
    eng, net = pop.engine, model.chain

    def candidates(first, count):
        return np.stack([model.embed(init_params(net, rng)) for _ in range(count)]), np.zeros((count, 1))
    order, _, nn_sel, cond_sel = eng.screen_candidates(initial_guesses, selected_initials, candidates)
    sols = []
    if side_by_side and len(order) > 1:
        fits = _batched_adam_then_lbfgs(eng, nn_sel, cond_sel, number_of_iterations_adam, number_of_iterations_lbfgs,
                                        learning_rate_adam)
    else:
        fits = []
        for k in range(len(order)):
            try:
                fits.append(_adam_then_lbfgs(eng, nn_sel[k], cond_sel[k], number_of_iterations_adam,
                                             number_of_iterations_lbfgs, learning_rate_adam))
            except FloatingPointError:
                fits.append(None)
    for fit in fits:
        if fit is None:
            print("Optimization failed... Skipping")
            continue
        sols.append(OptimizationSolution(u=model.extract(fit[0]), objective=fit[2]))
    return sols


def _fit_box(eng, lower, upper, n_grid, iters, method, *, start=None, penalty_weight=0.0, penalty_center=0.0,
             max_evals=40):
    """The per-subject fits behind every frozen-network estimate: (x, objective, sse, info or None).
    method = "search": cude_fit_conditional (coarse scan + golden section), today's behaviour bit for bit.
    method = "newton": the coarse scan as ONE profile launch (n_grid values), then cude_refine_conditional from every
    subject's argmin; n_grid = 0: no scan, the refinement starts from `start` (scalar or (N,)) -- the reference's own
    semantics of a local solver from an initial point."""
    if method == "search":
        return eng.fit_conditional(lower, upper, n_grid, iters, penalty_weight, penalty_center) + (None,)
    if method != "newton":
        raise ValueError(f'method must be "search" or "newton", not {method!r}')
    if n_grid > 0:
        values = np.linspace(lower, upper, n_grid)
        prof = eng.profile_conditional(values) + penalty_weight * (values[:, None] - penalty_center) ** 2
        start = values[np.argmin(np.where(np.isfinite(prof), prof, np.inf), axis=0)]
        del prof            # (a multi-megabyte read-back kept alive across the next call was measured to stall it)
    elif start is None:
        raise ValueError("n_grid = 0 needs a start")
    r = eng.refine_conditional(np.asarray(start, dtype=np.float64), lower, upper, max_evals=max_evals,
                               penalty_weight=penalty_weight, penalty_center=penalty_center)
    return r["x"], r["objective"], r["sse"], r["info"]


def estimate_conditional(models, timepoints, cpeptide_data, nn, *, initial_beta=-2.0, lower=-4.0, upper=1.0,
                         n_steps=None, n_grid=41, iters=48, method="search", return_info=False):
    """All N independent 1-D problems min_beta SSE_i(beta) at once.  Box [lower, upper]; infinite bounds are replaced by
    initial_beta -/+ 6.  method = "search" (cude_fit_conditional: coarse scan + golden section with the search state on
    the device, one forward launch over the population per probe) or "newton" (one profile launch of n_grid values, then
    cude_refine_conditional from every subject's argmin; n_grid = 0: from initial_beta, as the reference's LBFGS run).
    Returns (beta[N], SSE[N]), with return_info also info[N] at the result ("newton": the fit's own; "search": None)."""
    pop = _population(models, timepoints, cpeptide_data, n_steps)
    eng = pop.engine
    lo = lower if np.isfinite(lower) else np.min(initial_beta) - 6.0
    hi = upper if np.isfinite(upper) else np.max(initial_beta) + 6.0
    eng.set_params(nn, None)
    x, _, sse, info = _fit_box(eng, lo, hi, n_grid, iters, method, start=initial_beta)
    return (x, sse, info) if return_info else (x, sse)


def train_with_sigma(models, timepoints, cpeptide_data, nn, *, initial_beta=-2.0, lbfgs_lower_bound=-4.0,
                     lbfgs_upper_bound=1.0, lbfgs_iterations=1000, n_steps=None, method="search"):
    """Joint (beta, sigma) estimate per subject (:290-307).  For fixed beta the NLL is minimised by
    sigma^2 = SSE/n, and beta minimises SSE, so the 2-D problem separates.  `method` as estimate_conditional."""
    beta, sse = estimate_conditional(models, timepoints, cpeptide_data, nn, initial_beta=initial_beta,
                                     lower=lbfgs_lower_bound, upper=lbfgs_upper_bound, n_steps=n_steps, method=method)
    n = len(timepoints)
    sigma = np.sqrt(np.maximum(sse, 1e-300) / n)
    obj = (n / 2) * np.log(sigma ** 2) + sse / (2 * sigma ** 2)
    return [OptimizationSolution(u=ComponentArray(ode=np.array([b]), sigma=s), objective=o)
            for b, s, o in zip(beta, sigma, obj)]


def evaluate_model(models, timepoints, cpeptide_data, neural_network_parameters, betas_train, *, n_steps=None):
    """Validation objectives of every candidate network (:406-433): (n_subjects x n_networks)."""
    cols = []
    for betas, p_nn in zip(betas_train, neural_network_parameters):
        try:
            sols = train(models, timepoints, cpeptide_data, np.asarray(p_nn), initial_beta=float(np.mean(betas)),
                         lbfgs_lower_bound=-np.inf, lbfgs_upper_bound=np.inf, n_steps=n_steps)
            cols.append([s.objective for s in sols])
        except Exception:
            cols.append([np.inf] * len(models))
    return np.array(cols).T


def likelihood_profile(beta, neural_network_parameters, model, timepoints, cpeptide_data, lower_bound, upper_bound,
                       sigma, *, steps=1000, n_steps=None):
    """src/likelihood-profiles.jl:4-17 -- the `steps` probes run as ONE population of copies of the subject."""
    copies = [model] * steps
    data = np.tile(np.asarray(cpeptide_data, dtype=np.float64), (steps, 1))
    pop = _population(copies, timepoints, data, n_steps)
    values = np.linspace(lower_bound, upper_bound, steps)
    pop.engine.set_params(neural_network_parameters, values)
    nll = pop.engine.forward(want_sse=True)["sse"] / (2 * sigma ** 2)
    nll_min = loss(beta, (model, timepoints, cpeptide_data, neural_network_parameters), n_steps=n_steps) / (2 * sigma ** 2)
    return nll, nll_min, values


_CI_THRESHOLDS = {"cantelli95": 7.16, "cantelli90": 5.24, "raue95": 3.841458820694124}   # last: quantile(Chisq(1), 0.95)


def find_confidence_intervals(loss_values, loss_minimum, parameter_values, *, target="cantelli95"):
    """src/likelihood-profiles.jl:34-59: the outermost profile points whose value is within the target's threshold of
    the minimum; an end of the interval that coincides with an end of the profiled range is reported as -/+Inf.
    An unknown target falls back to raue95, as the reference does."""
    loss_values = np.asarray(loss_values, dtype=np.float64)
    threshold = loss_minimum + _CI_THRESHOLDS.get(target, _CI_THRESHOLDS["raue95"])
    idx = np.flatnonzero(loss_values <= threshold)
    if idx.size == 0:
        raise ValueError("no profile point lies within the threshold of the minimum")     # Julia: minimum of empty
    lo = -np.inf if idx[0] == 0 else float(parameter_values[idx[0]])
    hi = np.inf if idx[-1] == len(loss_values) - 1 else float(parameter_values[idx[-1]])
    return lo, hi


def likelihood_profiles(betas, neural_network_parameters, models, timepoints, cpeptide_data, lower_bound, upper_bound,
                        sigma, *, steps=1000, n_steps=None):
    """The loop `[likelihood_profile(betas[i], nn, models[i], ...) for i in ...]` of c-peptide/02-conditional.jl:186-188
    for ALL models with one launch (cude_profile_conditional: the scan value is the grid's second dimension).
    Returns (nll (N, steps), nll_min (N,), values (steps,)) -- row i is likelihood_profile of subject i."""
    pop = _population(models, timepoints, cpeptide_data, n_steps)
    eng = pop.engine
    values = np.linspace(lower_bound, upper_bound, steps)
    eng.set_params(neural_network_parameters, np.asarray(betas, dtype=np.float64).reshape(-1))
    nll_min = eng.forward(want_sse=True)["sse"] / (2 * sigma ** 2)
    nll = eng.profile_conditional(values).T / (2 * sigma ** 2)
    return nll, nll_min, values


def _profile_intervals(eng, center, values, sigma, target, rounds, sections, return_details):
    """Intervals of every subject of `eng` at the threshold of `target`: the reference's nll <= nll_min + Delta with
    nll = SSE / (2 sigma^2) is SSE <= SSE(centre) + 2 sigma^2 Delta, which is what the device compares."""
    sig = np.asarray(sigma, dtype=np.float64)
    d = 2.0 * sig ** 2 * _CI_THRESHOLDS.get(target, _CI_THRESHOLDS["raue95"])
    r = eng.profile_intervals(values, center, float(d) if d.ndim == 0 else 0.0,
                              delta_per_subject=None if d.ndim == 0 else d.reshape(-1), rounds=rounds, sections=sections)
    cis = [(float(lo), float(hi)) for lo, hi in zip(r["lower"], r["upper"])]
    return (cis, r) if return_details else cis


def profile_confidence_intervals(betas, neural_network_parameters, models, timepoints, cpeptide_data, lower_bound,
                                 upper_bound, sigma, *, steps=1000, target="cantelli95", rounds=0, sections=3,
                                 n_steps=None, return_details=False):
    """The loop `find_confidence_intervals(likelihood_profile(...)...; target)` over all subjects
    (src/likelihood-profiles.jl:34-59 on the profiles of c-peptide/02-conditional.jl:186-188) with the profiles kept on
    the device (cude_profile_intervals): a list of (lower, upper) per subject, -/+Inf where the interval reaches an end of
    [lower_bound, upper_bound], (nan, nan) where no profile point lies within the threshold (the reference raises there)
    or the solve at betas[i] failed.  rounds = 0: find_confidence_intervals on row i of likelihood_profiles (up to a
    tie to rounding between nll and SSE units).  rounds > 0: every closed end is then tightened by `rounds` sectioning
    rounds of `sections` interior points, to (upper_bound - lower_bound) / (steps - 1) / (sections + 1) ** rounds; the
    ends reported lie inside the threshold.  sigma: scalar or (N,).  An unknown target falls back to raue95, as the
    reference does.  A list of CPeptideODEModel profiles the raw k, as `sensitivities` does.  return_details: also the
    dict of Engine.profile_intervals (argmin, min, center_objective, n_inside, status)."""
    if _is_model(models):
        models, cpeptide_data = [models], np.asarray(cpeptide_data)[None, :]
    center = np.asarray(betas, dtype=np.float64).reshape(-1)
    if isinstance(models[0], CPeptideODEModel):
        pop = _population(models, timepoints, cpeptide_data, n_steps, cond_space="raw")
        nn = pop.shared if neural_network_parameters is None else neural_network_parameters
    else:
        pop = _population(models, timepoints, cpeptide_data, n_steps)
        nn = neural_network_parameters
    pop.engine.set_params(nn, None)
    return _profile_intervals(pop.engine, center[:pop.N], np.linspace(lower_bound, upper_bound, steps), sigma, target,
                              rounds, sections, return_details)


# ----------------------------------------------------------------------------- sensitivities, Fisher information
def sensitivities(theta, args, *, n_steps=None):
    """Output sensitivities of every subject to its own conditional parameter, by the library's tangent-linear solve
    (cude_sensitivity) -- the partials the reference's solves carry under ForwardDiff (src/parameter-estimation.jl:59,165).
    args = (models, timepoints, cpeptide_data), theta.neural / theta.conditional as `loss`.  Returns
    (sens (n_state, T, N) = d u_s(t_j) / d beta_i, info (N,) = sum_j (d yhat_j / d beta_i)^2, score (N,) = half the
    derivative of SSE_i, sse (N,)).  The derivative is with respect to the parameter as stored (log-space beta; k itself
    for a list of CPeptideODEModel).  Failed subjects are NaN."""
    models, timepoints, data = args
    if _is_model(models):
        models, data = [models], np.asarray(data)[None, :]
    if isinstance(models[0], CPeptideODEModel):
        pop = _population(models, timepoints, data, n_steps, cond_space="raw")
        nn = getattr(theta, "neural", None)
        cond = getattr(theta, "conditional", getattr(theta, "ode", theta))
        pop.engine.set_params(pop.shared if nn is None else nn, np.asarray(cond, dtype=np.float64).reshape(-1)[:pop.N])
    else:
        pop = _population(models, timepoints, data, n_steps)
        pop.engine.set_params(theta.neural, np.asarray(theta.conditional, dtype=np.float64).reshape(-1)[:pop.N])
    out = pop.engine.sensitivity()
    return out["sens"], out["info"], out["score"], out["sse"]


def curvatures(theta, args, *, n_steps=None):
    """Exact curvature of every subject's objective in its own conditional parameter, by the library's order-2
    forward-mode solve (cude_curvature) -- what ForwardDiff.hessian of the per-subject objective gives.  args and theta as
    `sensitivities`.  Returns (sens2 (n_state, T, N) = d^2 u_s(t_j) / d beta_i^2, curv (N,) = sum_j [(d yhat_j / d beta_i)^2
    + (yhat_j - y_j) d^2 yhat_j / d beta_i^2] = half the second derivative of SSE_i, info, score, sse (N,) as
    `sensitivities`).  curv / sigma^2 is the OBSERVED information; unlike info it may be <= 0 (the point is then no minimum
    of SSE_i).  Failed subjects are NaN."""
    out = _params_set(theta, args, n_steps).engine.curvature()
    return out["sens2"], out["curv"], out["info"], out["score"], out["sse"]


def _information_kind(information):
    if information not in ("expected", "observed"):
        raise ValueError('information must be "expected" or "observed"')
    return information == "observed"


def conditional_standard_errors(betas, neural_network_parameters, models, timepoints, cpeptide_data, *, sigma=None,
                                n_steps=None, info=None, sse=None, information="expected"):
    """Asymptotic standard error of every subject's conditional parameter: sigma / sqrt(info_i), the inverse square root
    of the Fisher information info_i / sigma^2 of a Gaussian error model.  sigma = None: the per-subject maximum-likelihood
    value sigma_i^2 = SSE_i / n_i, the closed form loss_sigma (src/parameter-estimation.jl:70-75) is minimised by.  A
    subject whose data do not identify the parameter (info = 0) gets inf.  info (and sse, unless sigma is given): what a
    fit with method = "newton" returned at betas (estimate_conditional(..., return_info=True)) -- no second solve.
    information = "observed": the observed information curv_i / sigma^2 of `curvatures` takes the place of the expected
    one (one cude_curvature call; `info` is not used): se = sigma / sqrt(curv_i) where curv_i > 0, inf where curv_i <= 0
    (betas_i is no minimum of SSE_i), NaN for a failed subject."""
    if _information_kind(information):
        theta = ComponentArray(neural=neural_network_parameters, conditional=np.asarray(betas, dtype=np.float64).reshape(-1))
        _, curv, _, _, sse = curvatures(theta, (models, timepoints, cpeptide_data), n_steps=n_steps)
        return _standard_errors(curv, sse, len(timepoints), sigma)
    if info is not None and (sigma is not None or sse is not None):
        return _standard_errors(info, np.zeros_like(info) if sse is None else sse, len(timepoints), sigma)
    theta = ComponentArray(neural=neural_network_parameters, conditional=np.asarray(betas, dtype=np.float64).reshape(-1))
    _, info, _, sse = sensitivities(theta, (models, timepoints, cpeptide_data), n_steps=n_steps)
    return _standard_errors(info, sse, len(timepoints), sigma)


def _standard_errors(info, sse, n_obs, sigma):
    info, sse = np.asarray(info, dtype=np.float64), np.asarray(sse, dtype=np.float64)
    sig = np.sqrt(sse / n_obs) if sigma is None else np.broadcast_to(np.asarray(sigma, dtype=np.float64), info.shape)
    se = np.full(info.shape, np.inf)
    ok = info > 0.0
    se[ok] = sig[ok] / np.sqrt(info[ok])
    se[np.isnan(info)] = np.nan
    return se


def _wald(betas, se, level):
    z = NormalDist().inv_cdf(0.5 + level / 2)
    return [(float(b - z * s), float(b + z * s)) for b, s in zip(np.asarray(betas, dtype=np.float64).reshape(-1), se)]


def wald_confidence_intervals(betas, neural_network_parameters, models, timepoints, cpeptide_data, *, sigma=None,
                              level=0.95, n_steps=None, information="expected"):
    """Wald intervals beta_i -/+ z_level * se_i, one (lower, upper) pair per subject as find_confidence_intervals returns
    for a profile; (-inf, inf) where the data do not identify the parameter.  information: as
    conditional_standard_errors."""
    se = conditional_standard_errors(betas, neural_network_parameters, models, timepoints, cpeptide_data, sigma=sigma,
                                     n_steps=n_steps, information=information)
    return _wald(betas, se, level)


def _bootstrap(eng, center, sigma, n_rows, n_reps, level, seed, noise, lower, upper, return_replicates):
    """The percentile interval, spread and bias of every subject's refitted conditional parameter, from the order statistics
    and summaries cude_bootstrap_conditional leaves (the context's shared parameters are set; `center` (N,) its centre)."""
    if not 0.0 < level < 1.0:
        raise ValueError("level must lie inside (0, 1)")
    B = int(n_reps)
    if sigma is None:                                      # the per-subject maximum-likelihood value SSE_i / n_i
        eng.set_params(None, center)
        sigma = np.sqrt(eng.forward(want_sse=True)["sse"] / n_rows)
        sigma = np.where(np.isfinite(sigma), sigma, 0.0)   # (a failed subject fails through its centre's solve)
    if noise is None and seed is not None:
        eng.set_rng(seed)
    ranks, lo, hi, g = quantile_ranks([0.5 - level / 2, 0.5 + level / 2], B)
    r = eng.bootstrap_conditional(sigma, B, center, ranks=ranks, noise=noise, lower=lower, upper=upper,
                                  want_replicates=return_replicates)
    bounds = quantile_lerp(r["order"][lo], r["order"][hi], g[:, None])        # (2, N)
    bounds[:, r["n_used"] < B] = np.nan                    # fewer values than asked for: not the requested quantiles
    out = SimpleNamespace(lower=bounds[0], upper=bounds[1], se=r["sd"], bias=r["mean"] - center, mean=r["mean"],
                          n_used=r["n_used"], sigma=np.broadcast_to(np.asarray(sigma, dtype=np.float64), center.shape).copy(),
                          level=float(level))
    if return_replicates:
        out.replicates, out.status = r["replicates"], r["status"]
    return out


def bootstrap_conditional(betas, nn, models, timepoints, cpeptide_data, *, sigma=None, n_reps=200, level=0.95, seed=None,
                          noise=None, lower=-4.0, upper=1.0, n_steps=None, return_replicates=False):
    """Parametric bootstrap of every subject's conditional parameter on the device (cude_bootstrap_conditional) -- the
    finite-sample counterpart of conditional_standard_errors / wald_confidence_intervals, by the reference's own way of
    validating an estimate (simulate noisy data from the model, fit again: suppression/src/suppression_model.jl:39-63,
    :179-222): n_reps times per subject, c-peptide observations are drawn around the model's prediction at betas with
    standard deviation sigma_i (None: sqrt(SSE_i(betas_i) / n_i), conditional_standard_errors' convention) and the
    parameter is refitted from betas_i inside [lower, upper] by estimate_conditional's method = "newton" iteration.
    noise (n_reps, T, N) standard normals (the t_0 row is ignored), or None: the device's counter-based stream, seeded by
    `seed` when given.  Returns a namespace: lower, upper (N,) -- the type-7 percentile interval at `level` --, se (the
    replicates' standard deviation), bias (their mean - betas), mean, n_used (replicates whose fit did not fail; the
    interval is NaN where that is < n_reps), sigma [, replicates (n_reps, N), status (n_reps, N)]."""
    pop = _population(models, timepoints, cpeptide_data, n_steps)
    center = np.ascontiguousarray(np.asarray(betas, dtype=np.float64).reshape(-1)[:pop.N])
    pop.engine.set_params(nn, None)
    return _bootstrap(pop.engine, center, sigma, len(timepoints), n_reps, level, seed, noise, lower, upper, return_replicates)


def _npde(eng, sigma, prior_eta, prior_omega, n_sims, seed, samples, noise, state):
    """The namespace npde / suppression_npde return, from what cude_npde leaves (the context's shared parameters are set)."""
    if seed is not None and (samples is None or noise is None):
        eng.set_rng(seed)
    r = eng.npde(sigma, n_sims, samples, prior_mean=prior_eta, prior_sd=prior_omega, noise=noise, state=state)
    ok = np.isfinite(r["npde"])
    pooled = r["npde"][ok]
    return SimpleNamespace(pd=r["pd"], npde=r["npde"], pred_mean=r["pred_mean"], pred_sd=np.sqrt(r["pred_var"]),
                           status=r["status"], n_used=r["n_used"],
                           npde_mean=float(np.mean(pooled)) if pooled.size else float("nan"),
                           npde_var=float(np.var(pooled, ddof=1)) if pooled.size > 1 else float("nan"))


def npde(p_neural, models, timepoints, cpeptide_data, sigma, prior_eta, prior_omega, *, n_sims=1000, seed=None, samples=None,
         noise=None, n_steps=None):
    """Simulation-based prediction discrepancies and normalised prediction distribution errors of the fitted population
    model (cude_npde; Brendel et al. 2006, Comets et al. 2008 -- what Monolix, saemix and NONMEM report after a SAEM fit):
    n_sims times per subject a random effect eta ~ Normal(prior_eta, prior_omega) is drawn (or taken from samples (n_sims,
    N)), the c-peptide model is solved at the data's times and residual noise of standard deviation sigma (a number or
    (N,)) is added (noise (n_sims, T - 1, N) standard normals, or the device's counter-based stream, seeded by `seed` when
    given); every observation after t_0 is ranked among its simulations -- pd -- and, after the subject's rows are
    decorrelated by the Cholesky factor of the simulations' covariance, again -- npde = Phi^-1 of that rank.  Under the
    model the pooled npde are standard normal.  Returns a namespace: pd, npde, pred_mean, pred_sd (T - 1, N), status (N,)
    NPDE_* bits, n_used (N,), npde_mean, npde_var (pooled over the finite entries)."""
    pop = _population(models, timepoints, cpeptide_data, n_steps)
    pop.engine.set_params(p_neural, None)
    return _npde(pop.engine, sigma, prior_eta, prior_omega, n_sims, seed, samples, noise, 0)


def _vpc_groups(groups, N):
    """(ids (N,) int32 or None, number of groups, labels or None): integer ids as they are (negative = left out), anything
    else mapped to 0, 1, ... in order of first appearance."""
    if groups is None:
        return None, 1, None
    g = np.asarray(groups).reshape(-1)
    if g.shape != (N,):
        raise ValueError(f"expected groups ({N},)")
    if np.issubdtype(g.dtype, np.integer):
        return g.astype(np.int32), max(1, int(g.max()) + 1), None
    labels = list(dict.fromkeys(g.tolist()))
    index = {v: k for k, v in enumerate(labels)}
    return np.array([index[v] for v in g.tolist()], dtype=np.int32), len(labels), labels


def _vpc(eng, sigma, prior_eta, prior_omega, groups, levels, ci, n_sims, seed, samples, noise, state):
    """The namespace vpc / suppression_vpc return, from what cude_vpc leaves (the context's shared parameters are set)."""
    if seed is not None and (samples is None or noise is None):
        eng.set_rng(seed)
    ids, G, labels = _vpc_groups(groups, eng.N)
    r = eng.vpc(sigma, n_sims, samples, prior_mean=prior_eta, prior_sd=prior_omega, noise=noise, state=state, groups=ids,
                n_groups=G, levels=levels, ci_levels=ci, want_sim_q=False)
    obs, band = r["observed"], r["simulated_ci"]
    with np.errstate(invalid="ignore"):
        outside = (obs < band[..., 0]) | (obs > band[..., -1])
    return SimpleNamespace(observed=obs, simulated_ci=band, outside=outside, n_members=r["n_members"],
                           n_sims_used=r["n_sims_used"], status=r["status"], levels=np.asarray(levels, dtype=np.float64),
                           ci_levels=np.asarray(ci, dtype=np.float64), labels=labels)


def vpc(p_neural, models, timepoints, cpeptide_data, sigma, prior_eta, prior_omega, *, groups=None, levels=(0.05, 0.5, 0.95),
        ci=(0.025, 0.5, 0.975), n_sims=1000, seed=None, samples=None, noise=None, n_steps=None):
    """Visual predictive check of the fitted population model by subject group (cude_vpc -- the diagnostic Monolix, saemix,
    NONMEM/PsN and nlmixr plot after a SAEM fit; the reference stratifies its figures by NGT / IGT / T2DM,
    `train_data.types`): n_sims data sets are simulated exactly as npde simulates them (eta ~ Normal(prior_eta, prior_omega)
    or samples (n_sims, N); residual noise of standard deviation sigma, from noise (n_sims, T - 1, N) or the device's stream,
    seeded by `seed` when given).  Inside each group the type-7 quantiles ACROSS SUBJECTS at `levels` are taken of every
    simulated data set and of the observations at every data time after t_0, and of each simulated quantile the quantiles
    at `ci` across the simulations.  groups: (N,) integer ids (negative = left out), or labels (e.g. the reference's type
    strings) mapped to ids in order of first appearance and returned as `labels`; None = one group.  Returns a namespace:
    observed (G, T - 1, L), simulated_ci (G, T - 1, L, C), outside (G, T - 1, L) -- the observed quantile lies below the
    first or above the last `ci` level of its simulated counterpart --, n_members, n_sims_used (G,), status (N,) VPC_* bits,
    levels, ci_levels, labels."""
    pop = _population(models, timepoints, cpeptide_data, n_steps)
    pop.engine.set_params(p_neural, None)
    return _vpc(pop.engine, sigma, prior_eta, prior_omega, groups, levels, ci, n_sims, seed, samples, noise, 0)


# ----------------------------------------------------------------------------- suppression model
class _SuppPop:
    def __init__(self, data, timepoints, net, lam, n_steps, device):
        self.engine = Engine("supp", net.arch, n_steps=n_steps, lam=lam, device=device)
        net.configure(self.engine)
        if net.mask is not None:
            self.engine.set_param_mask(net.mask)
        self.engine.set_population_supp(np.asarray(timepoints, dtype=np.float64), data)
        self.data = data


def _supp_population(prob, data, timepoints, lam, n_steps=None):
    n_steps = default_steps() if n_steps is None else n_steps       # (fixed mode: DEFAULT_STEPS = 30)
    data = np.asarray(data, dtype=np.float64)
    key = ("supp", prob.network.key, float(lam), int(n_steps), _digest(timepoints, data))
    return _cached(key, lambda: _SuppPop(data, timepoints, prob.network, lam, n_steps, _DEVICE))


def lsup(u, p):
    """lsup! (suppression_model.jl:16-20): the ground-truth model that generates the suppression data; u, p: arrays whose
    first axis is the state / parameter index."""
    a = p[1] * u[1] / (1.0 + p[3] * u[2])
    return np.stack([-p[0] * u[0], p[0] * u[0] - a, a - p[2] * u[2]])


def get_group_parameters(mu_sup, n_samples, *, rng):
    """get_group_parameters (:33-37): max(mu + std * randn(4, n), 0.05), mu = [0.4, 0.9, 0.3, mu_sup],
    std = [0.1, 0.1, 0.1, mu_sup / 8].  `rng`: numpy Generator (the reference's StableRNG stream is not reproducible
    here: same distribution, other numbers)."""
    mu = np.array([0.4, 0.9, 0.3, mu_sup])[:, None]
    sd = np.array([0.1, 0.1, 0.1, mu_sup / 8.0])[:, None]
    return np.maximum(mu + sd * rng.standard_normal((4, int(n_samples))), 0.05)


def generate_data(group_means, group_sizes, timepoints, *, noise_additive=0.0, noise_multiplicative=0.0, rng=None,
                  substeps=200):
    """generate_data (:39-63): per group the parameters of get_group_parameters, per subject the solution of lsup! from
    u0 = (10, 0, 0) at `timepoints` plus additive and multiplicative Gaussian noise, clamped at 0.  Returns
    (data 3 x T x N, ground-truth suppression parameters).  Data generation is not on the device path: a classical RK4
    solve with `substeps` steps per observation interval on the host (error ~1e-8 for the reference's grid), draws
    in the reference's order (group parameters, then per subject the additive and the multiplicative field)."""
    rng = np.random.default_rng(232705) if rng is None else rng
    tp = np.asarray(timepoints, dtype=np.float64)
    T, N = tp.size, int(np.sum(group_sizes))
    data, gt, col = np.zeros((3, T, N)), [], 0
    for mean, size in zip(group_means, group_sizes):
        p = get_group_parameters(mean, size, rng=rng)
        u = np.stack([np.full(size, 10.0), np.zeros(size), np.zeros(size)])
        sol = np.empty((3, T, size))
        sol[:, 0] = u
        for k in range(1, T):
            h = (tp[k] - tp[k - 1]) / substeps
            for _ in range(substeps):
                k1 = lsup(u, p)
                k2 = lsup(u + 0.5 * h * k1, p)
                k3 = lsup(u + 0.5 * h * k2, p)
                k4 = lsup(u + h * k3, p)
                u = u + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
            sol[:, k] = u
        for j in range(size):
            s = sol[:, :, j]
            s = s + noise_additive * rng.standard_normal(s.shape) + noise_multiplicative * s * rng.standard_normal(s.shape)
            data[:, :, col] = np.maximum(s, 0.0)
            col += 1
        gt.extend(p[3].tolist())
    return data, np.asarray(gt)


def SuppressionProblem(network, tspan=(0.0, 30.0)):
    """Stand-in for `ODEProblem(ude_lsup!, [10,0,0], (0,30))` with the network closed over
    (suppression/suppression.jl:18-20): carries the network shape and the time span `simul` solves over when it saves
    at times other than the data's; u0 comes from the data (:119)."""
    t0, t1 = float(tspan[0]), float(tspan[1])
    if not t1 > t0:
        raise ValueError("SuppressionProblem: tspan must be increasing")
    return SimpleNamespace(network=network, tspan=(t0, t1))


def suppression_loss(p, args, *, n_steps=None):
    """suppression_loss(p, (prob, individual_data, timepoints, lambda)) with p.theta[N], p.neural[P] (:117-130)."""
    prob, data, timepoints, lam = args
    pop = _supp_population(prob, data, timepoints, lam, n_steps)
    pop.engine.set_params(p.neural, p.theta)
    return pop.engine.forward()["loss"]


def suppression_sensitivities(p, args, *, n_steps=None):
    """sensitivities for the suppression model: args = (prob, individual_data, timepoints, lambda) as suppression_loss.
    Returns (sens (3, T, N) = d u / d theta_i, info, score, sse) with the loss's weights 1 / scale_s."""
    prob, data, timepoints, lam = args
    pop = _supp_population(prob, data, timepoints, lam, n_steps)
    pop.engine.set_params(p.neural, p.theta)
    out = pop.engine.sensitivity()
    return out["sens"], out["info"], out["score"], out["sse"]


def suppression_curvatures(p, args, *, n_steps=None):
    """curvatures for the suppression model: args as suppression_sensitivities.  Returns (sens2 (3, T, N) = d^2 u / d
    theta_i^2 (state 1 exactly 0), curv, info, score, sse) with the loss's weights 1 / scale_s."""
    prob, data, timepoints, lam = args
    pop = _supp_population(prob, data, timepoints, lam, n_steps)
    pop.engine.set_params(p.neural, p.theta)
    out = pop.engine.curvature()
    return out["sens2"], out["curv"], out["info"], out["score"], out["sse"]


def suppression_profile_intervals(p, args, lower_bound, upper_bound, sigma, *, steps=1000, target="cantelli95", rounds=0,
                                  sections=3, n_steps=None, return_details=False):
    """profile_confidence_intervals for the suppression model: args = (prob, individual_data, timepoints, lambda) as
    suppression_loss, centres p.theta, network p.neural; the profiled objective is the per-subject weighted SSE."""
    prob, data, timepoints, lam = args
    pop = _supp_population(prob, data, timepoints, lam, n_steps)
    pop.engine.set_params(p.neural, None)
    return _profile_intervals(pop.engine, np.asarray(p.theta, dtype=np.float64).reshape(-1),
                              np.linspace(lower_bound, upper_bound, steps), sigma, target, rounds, sections, return_details)


def suppression_bootstrap(p, args, *, sigma=None, n_reps=200, level=0.95, seed=None, noise=None, lower=-8.0, upper=5.0,
                          n_steps=None, return_replicates=False):
    """bootstrap_conditional for the suppression model: args = (prob, individual_data, timepoints, lambda) as
    suppression_loss, centres p.theta, network p.neural, the box validate_suppression_model's.  Replicate data: all three
    states around the model's prediction with standard deviation sigma_i times the state's loss scale (sigma = None:
    sqrt(SSE_i / (3 T)) of the weighted SSE); noise (n_reps, 3 T, N) in (3, T, N) order."""
    prob, data, timepoints, lam = args
    pop = _supp_population(prob, data, timepoints, lam, n_steps)
    pop.engine.set_params(p.neural, None)
    center = np.ascontiguousarray(np.asarray(p.theta, dtype=np.float64).reshape(-1))
    return _bootstrap(pop.engine, center, sigma, 3 * len(timepoints), n_reps, level, seed, noise, lower, upper, return_replicates)


def suppression_npde(p, args, sigma, prior_eta, prior_omega, *, state=2, n_sims=1000, seed=None, samples=None, noise=None,
                     n_steps=None):
    """npde for the suppression model: args = (prob, individual_data, timepoints, lambda) as suppression_loss, network
    p.neural, the rows of state `state` (0-based) with residual standard deviation sigma times that state's loss scale."""
    prob, data, timepoints, lam = args
    pop = _supp_population(prob, data, timepoints, lam, n_steps)
    pop.engine.set_params(p.neural, None)
    return _npde(pop.engine, sigma, prior_eta, prior_omega, n_sims, seed, samples, noise, state)


def suppression_vpc(p, args, sigma, prior_eta, prior_omega, *, state=2, groups=None, levels=(0.05, 0.5, 0.95),
                    ci=(0.025, 0.5, 0.975), n_sims=1000, seed=None, samples=None, noise=None, n_steps=None):
    """vpc for the suppression model: args = (prob, individual_data, timepoints, lambda) as suppression_loss, network
    p.neural, the rows of state `state` (0-based) with residual standard deviation sigma times that state's loss scale."""
    prob, data, timepoints, lam = args
    pop = _supp_population(prob, data, timepoints, lam, n_steps)
    pop.engine.set_params(p.neural, None)
    return _vpc(pop.engine, sigma, prior_eta, prior_omega, groups, levels, ci, n_sims, seed, samples, noise, state)


def suppression_loss_and_gradient(p, args, *, n_steps=None):
    prob, data, timepoints, lam = args
    pop = _supp_population(prob, data, timepoints, lam, n_steps)
    pop.engine.set_params(p.neural, p.theta)
    val, g_nn, g_th = pop.engine.loss_grad()
    return val, ComponentArray(theta=g_th, neural=g_nn)


def simul(p, prob, individual_data, timepoints, *, n_steps=None):
    """simul(p, prob, data, timepoints) -> 3 x len(timepoints) x N array (:107-115).  u0 = data[:, 0, :]; the solve runs
    over the data's own times when there is one save time per data column, otherwise over prob.tspan with the states
    saved at `timepoints` (dense output, as the reference's figure script calls it: figures.jl:66-74), which must lie
    inside the span and be non-decreasing."""
    data = np.asarray(individual_data, dtype=np.float64)
    tp = np.asarray(timepoints, dtype=np.float64).reshape(-1)
    if data.ndim != 3 or data.shape[0] != 3:
        raise ValueError("individual_data must be (3, T, N)")
    if tp.size == data.shape[1]:
        pop = _supp_population(prob, individual_data, timepoints, 0.0, n_steps)
        pop.engine.set_params(p.neural, p.theta)
        return pop.engine.forward(want_traj=True)["traj"]
    t0, t1 = getattr(prob, "tspan", (0.0, 30.0))
    if tp.size == 0 or not (np.all(tp >= t0) and np.all(tp <= t1)):
        raise ValueError(f"simul: save times must lie inside the problem's time span ({t0}, {t1})")
    if np.any(np.diff(tp) < 0.0):
        raise ValueError("simul: save times must be non-decreasing")
    # a population over the span whose two columns are the initial state: the same span and step grid as the
    # one-column-per-save-time path over those times
    u0 = np.ascontiguousarray(data[:, :1, :])
    pop = _supp_population(prob, np.concatenate([u0, u0], axis=1), np.array([t0, t1]), 0.0, n_steps)
    pop.engine.set_params(p.neural, p.theta)
    return pop.engine.simulate(tp)


def suppression_predictive(p, theta_samples, prob, individual_data, timepoints, *, levels=(0.025, 0.5, 0.975), state=2,
                           n_steps=None):
    """`simul` for K sampled conditional vectors theta_samples (K, N) at once, summarised on the device
    (cude_predictive_bands): the quantiles at `levels`, the mean, the minimum and the maximum of state `state` (0-based; 1
    and 2 depend on theta) of every (individual, save time) column over the samples -- the suppression counterpart of
    posterior_predictive.  Save times as `simul`'s dense-output form: inside prob.tspan, non-decreasing."""
    data = np.asarray(individual_data, dtype=np.float64)
    tp = np.asarray(timepoints, dtype=np.float64).reshape(-1)
    if data.ndim != 3 or data.shape[0] != 3:
        raise ValueError("individual_data must be (3, T, N)")
    t0, t1 = getattr(prob, "tspan", (0.0, 30.0))
    if tp.size == 0 or not (np.all(tp >= t0) and np.all(tp <= t1)) or np.any(np.diff(tp) < 0.0):
        raise ValueError(f"suppression_predictive: save times must be non-decreasing inside ({t0}, {t1})")
    u0 = np.ascontiguousarray(data[:, :1, :])
    pop = _supp_population(prob, np.concatenate([u0, u0], axis=1), np.array([t0, t1]), 0.0, n_steps)
    pop.engine.set_params(p.neural, None)
    return _predictive(pop.engine, theta_samples, tp, levels, state)


def fit_suppression_model(p_init, prob, data, timepoints, lam, *, select_best_n=1, adam_iters=2000, lbfgs_iters=2000,
                          n_steps=None, side_by_side=True, second_stage="lbfgs"):
    """fit_suppression_model (:132-177): screen all initials, keep the best n, Adam() [eta = 1e-3] then L-BFGS.
    The kept restarts are trained side by side (one launch per optimiser iteration for all of them) unless
    side_by_side=False.  second_stage="lm": train_lm's Levenberg-Marquardt loop (at most lbfgs_iters iterations) in place
    of L-BFGS, one restart after the other."""
    lm = _second_stage(second_stage)
    pop = _supp_population(prob, data, timepoints, lam, n_steps)
    eng = pop.engine
    init_losses = eng.multistart_forward(np.stack([p.neural for p in p_init]), np.stack([p.theta for p in p_init]))
    best = np.argsort(init_losses, kind="stable")[:max(1, select_best_n)]
    sols, traces = [], []
    if side_by_side and len(best) > 1 and not lm:
        traces = [[] for _ in best]
        fits = _batched_adam_then_lbfgs(eng, np.stack([p_init[k].neural for k in best]),
                                        np.stack([p_init[k].theta for k in best]), adam_iters, lbfgs_iters, 1e-3,
                                        traces=traces)
        for fit in fits:
            if fit is None:
                print("Optimization failed")
                continue
            nn, th, obj = fit
            sols.append(OptimizationSolution(u=ComponentArray(theta=th, neural=nn), objective=obj))
        return sols, traces
    for k in best:
        trace = []
        try:
            if lm:
                nn, th, obj = _adam_then_lm(eng, p_init[k].neural, p_init[k].theta, adam_iters, lbfgs_iters, 1e-3, trace)
            else:
                nn, th, obj = _adam_then_lbfgs(eng, p_init[k].neural, p_init[k].theta, adam_iters, lbfgs_iters, 1e-3,
                                               callback=lambda _x, l: trace.append(l) and False)
            sols.append(OptimizationSolution(u=ComponentArray(theta=th, neural=nn), objective=obj))
        except FloatingPointError:
            print("Optimization failed")
        traces.append(trace)
    return sols, traces


def validate_suppression_model(p_init, prob, data, timepoints, network_params, *, n_steps=None, lower=-8.0,
                               upper=5.0, method="search"):
    """validate_suppression_model(p_init, prob, data, timepoints, network_params) (:179-222): conditional parameters
    of new subjects with the network frozen, returns (theta, objective).  With the network fixed the loss separates
    per subject, so instead of one L-BFGS run from the best of `p_init` all subjects are solved together by a
    bracketing search over [lower, upper] (one forward launch per probe) -- the global minimum per subject, hence an
    objective <= the reference's.  p_init is accepted for signature compatibility and only widens the bracket.
    method = "newton": the 161-point scan as one profile launch, then cude_refine_conditional from every argmin."""
    pop = _supp_population(prob, data, timepoints, 0.0, n_steps)
    eng, N = pop.engine, np.asarray(data).shape[2]
    if p_init is not None and len(p_init):
        lower = min(lower, float(np.min(p_init)))
        upper = max(upper, float(np.max(p_init)))
    eng.set_params(network_params, None)
    theta, _, best, _ = _fit_box(eng, lower, upper, 161, 48, method)
    return theta, float(best.sum() / N)


def validate_suppression_model_sigma(p_init, prob, data, timepoints, network_params, *, n_steps=None, lower=-8.0,
                                     upper=5.0, n_grid=261, iters=50):
    """validate_suppression_model_sigma(p_init, prob, data, timepoints, network_params) (:224-275, used by
    suppression/figures.jl:46): theta and one noise level per state for a test subject, minimising
    sum_s (n/2) log sigma_s^2 + SSE_s(theta) / (2 sigma_s^2) on the UNSCALED residuals with the network frozen.
    `data` is one subject (3 x T, as in the reference) or many (3 x T x N: all of them at once).  For given theta the
    optimal sigma_s^2 is SSE_s / n, so the problem is 1-D per subject in theta: a grid over [lower, upper] and
    golden-section refinements, all subjects in lock step, one forward launch (trajectories) per probe.  Returns
    (ComponentArray(ode=theta, sigma=(3,) or (N, 3)), objective) -- the global minimum per subject, hence <= what the
    reference's L-BFGS run from the best of `p_init` reaches; p_init only widens the bracket."""
    data = np.asarray(data, dtype=np.float64)
    single = data.ndim == 2
    if single:
        data = data[:, :, None]
    pop = _supp_population(prob, data, timepoints, 0.0, n_steps)
    eng, N, n = pop.engine, data.shape[2], data.shape[1]
    if p_init is not None and len(p_init):
        lower = min(lower, float(np.min(p_init)))
        upper = max(upper, float(np.max(p_init)))

    def nll(theta):
        eng.set_params(network_params, theta)
        traj = eng.forward(want_traj=True)["traj"]                       # (3, T, N)
        sse = np.sum((traj - data) ** 2, axis=1)                         # (3, N)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.sum(0.5 * n * (np.log(sse / n) + 1.0), axis=0)
        return np.where(np.isfinite(v), v, np.inf), sse

    # sum_s log SSE_s(theta) has a narrow dip wherever one state is fitted well: a fine grid, then the three deepest
    # local minima of every subject are refined and the best kept
    grid = np.linspace(lower, upper, n_grid)
    vals = np.stack([nll(np.full(N, g))[0] for g in grid])              # (n_grid, N)
    pad = np.concatenate([np.full((1, N), np.inf), vals, np.full((1, N), np.inf)])
    is_min = (vals <= pad[:-2]) & (vals <= pad[2:])                      # the ends of the bracket count
    score = np.where(is_min & np.isfinite(vals), vals, np.inf)
    r = (math.sqrt(5.0) - 1.0) / 2.0
    theta, best = np.full(N, grid[0]), np.full(N, np.inf)
    for rank in range(3):
        k = np.argsort(score, axis=0, kind="stable")[rank]              # (N,) grid index of the rank-th deepest minimum
        k = np.where(np.isfinite(score[k, np.arange(N)]), k, np.argmin(vals, axis=0))
        a, b = grid[np.maximum(k - 1, 0)], grid[np.minimum(k + 1, n_grid - 1)]
        x1, x2 = b - r * (b - a), a + r * (b - a)
        f1, f2 = nll(x1)[0], nll(x2)[0]
        for _ in range(iters):
            left = f1 < f2
            b = np.where(left, x2, b)
            a = np.where(left, a, x1)
            probe = np.where(left, b - r * (b - a), a + r * (b - a))    # the surviving interior point is reused
            fp = nll(probe)[0]
            x1, f1, x2, f2 = (np.where(left, probe, x2), np.where(left, fp, f2), np.where(left, x1, probe),
                              np.where(left, f1, fp))
        cand, fc = np.where(f1 < f2, x1, x2), np.minimum(f1, f2)
        gk = vals[k, np.arange(N)]                                       # (a minimum AT an end of the bracket)
        cand, fc = np.where(gk < fc, grid[k], cand), np.minimum(gk, fc)
        theta, best = np.where(fc < best, cand, theta), np.minimum(fc, best)
    best, sse = nll(theta)
    sigma = np.sqrt(sse / n).T                                           # (N, 3)
    if single:
        return ComponentArray(ode=float(theta[0]), sigma=sigma[0]), float(best[0])
    return ComponentArray(ode=theta, sigma=sigma), best


# ----------------------------------------------------------------------------- utilities of the scripts (src/utils.jl)
def stratified_split(rng, types, f_train):
    """stratified_split(rng, types, f_train) (src/utils.jl:15-31): per type, round(f_train * count) subjects sampled
    without replacement for training; returns (sorted training indices, the complement), 0-based.  `rng` is a
    numpy Generator (the reference's StableRNG stream is not reproducible here: the split is of the same
    distribution, not the same subjects)."""
    types = np.asarray(types)
    train = []
    for ty in dict.fromkeys(types.tolist()):                              # unique(), first-occurrence order
        idx = np.flatnonzero(types == ty)
        n_train = int(round(f_train * idx.size))                          # round half to even, as Julia's round
        train.extend(rng.choice(idx, size=n_train, replace=False).tolist())
    train = np.sort(np.asarray(train, dtype=np.int64))
    return train, np.setdiff1d(np.arange(types.size), train)


def argmedian(x):
    """argmin(abs.(x .- median(x))) (src/utils.jl:43-45)."""
    x = np.asarray(x, dtype=np.float64)
    return int(np.argmin(np.abs(x - np.median(x))))


# ----------------------------------------------------------------------------- SAEM
def map_objective(p_individual, sse, n_obs, sigma, omega, *, prior_individual=0.0):
    """map_objective (src/saem.jl:68-72): -(log-likelihood + log N(p; prior_individual, omega)) given the subject's SSE."""
    return -(individual_log_likelihood(sse, n_obs, sigma) + _log_normal(p_individual, prior_individual, omega))


def compute_individual_maps(p_individuals, p_neural, models, timepoints, cpeptide_data, sigma, omega, *,
                            prior_individual=0.0, lower=-6.0, upper=4.0, n_steps=None, method="search"):
    """compute_individual_maps (src/saem.jl:74-84): every subject's maximum-a-posteriori conditional parameter with
    the network frozen.  argmin_x -(ll + logprior) = argmin_x SSE(x) + (sigma / omega)^2 (x - prior)^2: one penalised
    per-subject search on the device for all subjects (cude_fit_conditional) instead of an L-BFGS run per subject;
    p_individuals (the reference's starting points) only widen the bracket.  method = "newton": they ARE the starting
    points of cude_refine_conditional, as in the reference (none given: an 81-point scan first)."""
    models = [models] if _is_model(models) else list(models)
    data = np.asarray(cpeptide_data, dtype=np.float64)
    data = data[None, :] if data.ndim == 1 else data
    pop = _population(models, timepoints, data, n_steps)
    if p_individuals is not None and np.size(p_individuals):
        lower = min(lower, float(np.min(p_individuals)))
        upper = max(upper, float(np.max(p_individuals)))
    pop.engine.set_params(p_neural, None)
    have_start = p_individuals is not None and np.size(p_individuals)
    start = np.asarray(p_individuals, dtype=np.float64).reshape(-1) if have_start else None
    x, _, _, _ = _fit_box(pop.engine, lower, upper, 0 if (method == "newton" and have_start) else 81, 48, method,
                          start=start, penalty_weight=(sigma / omega) ** 2, penalty_center=prior_individual)
    return x


def individual_log_likelihood(sse, n_obs, sigma):
    """-(n/2) log sigma^2 - SSE/(2 sigma^2), -Inf on solver failure (src/saem.jl:55-66)."""
    ll = -(n_obs / 2) * math.log(sigma ** 2) - sse / (2 * sigma ** 2)
    return np.where(np.isfinite(sse), ll, -np.inf)


def _log_normal(x, mu, sd):
    return -0.5 * ((x - mu) / sd) ** 2 - math.log(sd) - 0.5 * math.log(2 * math.pi)


def mcmc_steps(sse_of, p_individual, n_obs, sigma, omega, proposal_std, prior_individual, temperature, gamma,
               normals, uniforms):
    """`mcmc_step` (src/saem.jl:86-108) applied `len(normals)` times to EVERY subject at once, with the
    stochastic-approximation update of the chain state (:185).  `sse_of(beta[N]) -> SSE[N]` is one forward launch
    over the population; normals / uniforms are (steps, N) draws (randn() / rand() of the reference).  As in the
    reference the current state's likelihood is re-evaluated every step.  Returns (p_individual, accepted[N])."""
    p = np.array(p_individual, dtype=np.float64)
    acc_count = np.zeros(p.size, dtype=np.int64)
    for z, u in zip(normals, uniforms):
        prop = p + z * proposal_std
        prior_ratio = _log_normal(prop, prior_individual, omega) - _log_normal(p, prior_individual, omega)
        ll_new = individual_log_likelihood(sse_of(prop), n_obs, sigma)
        ll_cur = individual_log_likelihood(sse_of(p), n_obs, sigma)
        acc = np.log(u) < prior_ratio + (ll_new / temperature - ll_cur / temperature)
        acc_count += acc
        p = (1 - gamma) * p + gamma * np.where(acc, prop, p)
    return p, acc_count


def SAEM(models, timepoints, cpeptide_data, initial_neural_params, *, sigma=1.0, prior_eta=0.0, prior_omega=1.0,
         iterations=500, n_burnin_iterations=100, proposal_std=0.1, proposal_std_bounds=(1e-3, 1.0), alpha=0.7,
         n_mcmc_steps=1, initial_mcmc_steps=None, target_acceptance_rate=0.25, initial_temperature=10.0,
         temperature_decay=0.05, omega_learning_rate=0.04, rng=None, n_steps=None, m_step_iters=5, m_step_lr=1e-2,
         collective=None, device_seed=None, subject_offset=0):
    """SAEM(individuals, initial_neural_params, network; ...) (src/saem.jl:134-237) with the population on the
    GPU: every Metropolis step evaluates all subjects in one forward launch; the M-step's 5 Adam iterations on
    (network, sigma) use the device gradient.  The loop itself is cude.parallel.saem_loop, shared with the
    subject-sharded multi-GPU form (`collective`: this process holds one shard of `models`).  device_seed: the
    Metropolis draws are generated on the device (counter-based, independent of the sharding given subject_offset)
    instead of by `rng` on the host."""
    from .parallel import saem_loop
    pop = _population(models, timepoints, cpeptide_data, n_steps)
    return saem_loop(pop.engine, pop.T, initial_neural_params, collective=collective, sigma=sigma,
                     prior_eta=prior_eta, prior_omega=prior_omega, iterations=iterations,
                     n_burnin_iterations=n_burnin_iterations, proposal_std=proposal_std,
                     proposal_std_bounds=proposal_std_bounds, alpha=alpha, n_mcmc_steps=n_mcmc_steps,
                     initial_mcmc_steps=initial_mcmc_steps, target_acceptance_rate=target_acceptance_rate,
                     initial_temperature=initial_temperature, temperature_decay=temperature_decay,
                     omega_learning_rate=omega_learning_rate, rng=rng, m_step_iters=m_step_iters, m_step_lr=m_step_lr,
                     device_seed=device_seed, subject_offset=subject_offset)


def quantile_ranks(levels, K):
    """The order statistics the type-7 quantiles (Julia's `quantile`, numpy.quantile's default) of K values need: with
    h = (K - 1) q the quantile at level q is x[lo] + g (x[hi] - x[lo]), lo = floor(h), hi = min(lo + 1, K - 1), g = h - lo.
    Returns (ranks, lo, hi, g): ranks = the sorted unique lo / hi of all levels (what cude_predictive_bands is asked for),
    lo / hi = every level's positions IN `ranks`, g = its weight."""
    q = np.asarray(levels, dtype=np.float64).reshape(-1)
    if K < 1 or np.any(~((q >= 0.0) & (q <= 1.0))):
        raise ValueError("quantile_ranks: need K >= 1 and levels inside [0, 1]")
    h = (K - 1) * q
    lo = np.floor(h).astype(np.int64)
    hi = np.minimum(lo + 1, K - 1)
    ranks = np.unique(np.concatenate([lo, hi]))
    return ranks.astype(np.int32), np.searchsorted(ranks, lo), np.searchsorted(ranks, hi), h - lo


def quantile_lerp(x_lo, x_hi, g):
    """The type-7 value x_lo + g (x_hi - x_lo), anchored at the nearer neighbour: evaluated as x_hi - (1 - g) (x_hi - x_lo)
    for g >= 1/2.  The same number; the roundings of the product and of the last operation are then relative to the
    neighbour the result lies next to, not to the far one.  numpy.quantile evaluates its default rule this way too."""
    d = x_hi - x_lo
    return np.where(g >= 0.5, x_hi - d * (1 - g), x_lo + d * g)


def _predictive(eng, samples, times, levels, state):
    """quantiles (N, n_levels, n_times), mean, minimum and maximum (N, n_times) of the sample curves, from the order
    statistics and the mean cude_predictive_bands leaves (the envelope ranks 0 and K - 1 ride along)."""
    s = np.asarray(samples, dtype=np.float64)
    K = s.shape[0]
    ranks, lo, hi, g = quantile_ranks(levels, K)
    all_ranks = np.unique(np.concatenate([ranks, [0, K - 1]])).astype(np.int32)
    r = eng.predictive_bands(s, times, all_ranks, state=state)
    order = r["order"]                                     # (N, n_times, n_ranks)
    pos = np.searchsorted(all_ranks, ranks)
    x_lo, x_hi = order[:, :, pos[lo]], order[:, :, pos[hi]]
    quant = quantile_lerp(x_lo, x_hi, g).transpose(0, 2, 1)
    return SimpleNamespace(quantiles=np.ascontiguousarray(quant), mean=r["mean"], minimum=order[:, :, 0].copy(),
                           maximum=order[:, :, -1].copy(), levels=np.asarray(levels, dtype=np.float64),
                           times=np.asarray(times, dtype=np.float64), bad_sets=r["bad_sets"])


def posterior_predictive(p_neural, samples, models, timepoints, cpeptide_data, *, out_timepoints=None,
                         levels=(0.025, 0.5, 0.975), save_idxs=1, n_steps=None):
    """The posterior-predictive curves of c-peptide/06-saem.jl:209-223 for ALL individuals at once, summarised on the
    device: samples (K, N) -- e.g. the thinned chain `individual_effects(...).samples[999::10]` -- are simulated as
    `simulate` does (state `save_idxs`, 1-based, at `out_timepoints`) and reduced there to the quantiles at `levels` (the
    type-7 rule of Julia's `quantile`), the mean, the minimum and the maximum of every (individual, time) column.
    Returns a namespace: quantiles (N, n_levels, n_times); mean, minimum, maximum (N, n_times); bad_sets (N,) = samples
    whose solve gave a non-finite value (such a column is NaN throughout)."""
    sym = isinstance(models[0], CPeptideODEModel)
    pop = _population(models, timepoints, cpeptide_data, n_steps, cond_space="raw" if sym else "log")
    pop.engine.set_params(pop.shared if sym else p_neural, None)
    times = np.asarray(timepoints if out_timepoints is None else out_timepoints, dtype=np.float64)
    return _predictive(pop.engine, samples, times, levels, save_idxs - 1)


def individual_effects(models, timepoints, cpeptide_data, saem_result, *, n_samples=3000, proposal_std=0.3,
                       rng=None, n_steps=None, lower=-6.0, upper=4.0, predictive_times=None, starts="search",
                       burn_in=None, thin=10, levels=(0.025, 0.5, 0.975)):
    """The per-individual loop that follows SAEM in c-peptide/06-saem.jl:97-135, for ALL individuals at once:
    posterior samples of the conditional parameter (n_samples Metropolis steps from the population mean, every
    state kept, :107-112), the MAP mode (minimiser of -(log-likelihood + log prior), :114-119), the MLE estimate
    (:121-126) and `mse = -2 individual_log_likelihood(mode; sigma = 1)` = the SSE at the mode (:129).  The two 1-D
    optimisations are bracketing searches over [lower, upper] with one forward launch per probe.
    starts = "samples": they are cude_refine_conditional runs from each individual's best kept sample instead -- the
    `argmin(map_objective_values)` / `argmax(likelihood_values)` over `samples[1000:end]` the reference starts its LBFGS
    runs from (:226-236), found on the device (cude_evaluate_conditional_sets).  predictive_times: the result also holds
    `predictive`, the bands of the thinned kept chain `samples[1000:10:end]` at those times (posterior_predictive, :220).
    Kept samples: from `burn_in` on (default 999, a third of the chain when it is shorter than 1000 steps)."""
    if starts not in ("search", "samples"):
        raise ValueError("starts must be 'search' or 'samples'")
    rng = np.random.default_rng() if rng is None else rng
    pop = _population(models, timepoints, cpeptide_data, n_steps)
    eng, N, T = pop.engine, pop.N, pop.T
    prior, omega, sigma = float(saem_result.eta), float(saem_result.Omega), float(saem_result.sigma)
    eng.set_params(saem_result.p_neural, np.full(N, prior))
    acc, samples = eng.mh_chain(rng.standard_normal((n_samples, N)), rng.random((n_samples, N)), sigma, prior, omega,
                                proposal_std)
    burn = (999 if n_samples > 1000 else n_samples // 3) if burn_in is None else int(burn_in)
    kept = samples[burn:]

    # -(log-likelihood + log prior) = [SSE + (sigma/Omega)^2 (b - prior)^2] / (2 sigma^2) + const
    if starts == "search":
        modes, _, mse = eng.fit_conditional(lower, upper, 81, 48, (sigma / omega) ** 2, prior)
        mle, _, _ = eng.fit_conditional(lower, upper, 81, 48)
    else:
        cols = np.arange(N)
        lo, hi = min(lower, float(kept.min())), max(upper, float(kept.max()))
        best = eng.evaluate_conditional_sets(kept, (sigma / omega) ** 2, prior)["index"]
        r = eng.refine_conditional(kept[best, cols], lo, hi, penalty_weight=(sigma / omega) ** 2, penalty_center=prior)
        modes, mse = r["x"], r["sse"]
        best = eng.evaluate_conditional_sets(kept)["index"]
        mle = eng.refine_conditional(kept[best, cols], lo, hi)["x"]
    out = SimpleNamespace(samples=samples, modes=modes, mle=mle, mse=mse,
                          acceptance_rate=float(acc.sum()) / (n_samples * N))
    if predictive_times is not None:
        out.predictive = _predictive(eng, kept[::thin], np.asarray(predictive_times, dtype=np.float64), levels, 0)
    return out


# ----------------------------------------------------------------------------- marginal likelihood
def gauss_hermite_rule(Q):
    """(nodes z, log_weights a) of the Q-point Gauss-Hermite rule in the form cude_marginal_likelihood takes: with the
    physicists' rule (t_k, w_k) for the weight exp(-t^2), z = sqrt(2) t and a = log w + t^2 + log(2) / 2, so that
    integral f(x) dx ~ s sum_k exp(a_k) f(m + s z_k) (the factor s is rule 4's log scale).  Exact for f = a Gaussian
    density of mean m and standard deviation s times a polynomial of degree < 2Q; Q = 1 is the Laplace value
    f(m) s sqrt(2 pi)."""
    t, w = np.polynomial.hermite.hermgauss(int(Q))
    return math.sqrt(2.0) * t, np.log(w) + t * t + 0.5 * math.log(2.0)


def grid_rule(lo, hi, n):
    """(nodes, log_weights) of the trapezoid rule on n >= 2 equidistant points of [lo, hi], for center 0 and scale 1: the
    route that does not depend on where a subject's posterior mass lies."""
    n = int(n)
    if n < 2 or not hi > lo:
        raise ValueError("grid_rule: need n >= 2 and hi > lo")
    x = np.linspace(lo, hi, n)
    w = np.full(n, (hi - lo) / (n - 1))
    w[0] = w[-1] = 0.5 * w[0]
    return x, np.log(w)


def _marginal_solve(betas, nn, models, timepoints, cpeptide_data, sigma, prior_mean, omega, *, method, n_nodes,
                    grid_halfwidth, lower, upper, first_step, seed, n_steps, want=False, center=None, scale=None,
                    curvature="expected", fallback=None):
    """The rule of marginal_likelihood and its device call: (population, the engine's dict, center, scale).  want: the
    points and terms as well.  center / scale given: the rule is placed there instead of at the MAP (not for "grid").
    curvature = "observed": the scale comes from one cude_curvature call at the refined centres; the subjects that keep
    the expected scale (curv + pw <= 0, or no finite curvature) are appended to the list `fallback`."""
    if method not in ("quadrature", "grid", "importance", "laplace"):
        raise ValueError('method must be "quadrature", "grid", "importance" or "laplace"')
    if curvature not in ("expected", "observed"):
        raise ValueError('curvature must be "expected" or "observed"')
    if method == "laplace":
        method, n_nodes = "quadrature", 1
    sym = isinstance(models[0], CPeptideODEModel)
    pop = _population(models, timepoints, cpeptide_data, n_steps, cond_space="raw" if sym else "log")
    eng, N = pop.engine, pop.N
    eng.set_params(pop.shared if sym and nn is None else nn, None)
    sigma, omega, prior_mean = float(sigma), float(omega), float(prior_mean)
    if method == "grid":
        z, a = grid_rule(prior_mean - grid_halfwidth * omega, prior_mean + grid_halfwidth * omega, n_nodes)
        center, scale = np.zeros(N), np.ones(N)
        r = eng.marginal_likelihood(sigma, prior_mean, omega, nodes=z, log_weights=a, center=center, want_points=want,
                                    want_terms=want)
    else:
        if center is None or scale is None:
            pw = (sigma / omega) ** 2
            start = None if betas is None else np.asarray(betas, dtype=np.float64).reshape(-1)[:N]
            center, _, _, info = _fit_box(eng, lower, upper, 81 if start is None else 0, 48, "newton", start=start,
                                          penalty_weight=pw, penalty_center=prior_mean)
            scale = sigma / np.sqrt(info + pw)
            if curvature == "observed":
                eng.set_params(None, center)                  # (the cached engine's conditionals: every call sets its own)
                curv = eng.curvature(want_sens2=False)["curv"]
                with np.errstate(invalid="ignore"):
                    ok = curv + pw > 0.0                      # (False for NaN as well)
                    scale = np.where(ok, sigma / np.sqrt(np.where(ok, curv + pw, 1.0)), scale)
                if fallback is not None:
                    fallback.extend(int(i) for i in np.flatnonzero(~ok))
        if method == "quadrature":
            z, a = gauss_hermite_rule(n_nodes)
            r = eng.marginal_likelihood(sigma, prior_mean, omega, nodes=z, log_weights=a, center=center, scale=scale,
                                        want_points=want, want_terms=want)
        else:
            if seed is not None:
                eng.set_rng(seed)
            r = eng.marginal_likelihood(sigma, prior_mean, omega, n_draws=n_nodes, first_step=first_step, center=center,
                                        scale=scale, want_points=want, want_terms=want)
    return pop, r, center, scale


def marginal_likelihood(betas, nn, models, timepoints, cpeptide_data, sigma, prior_mean, omega, *, method="quadrature",
                        n_nodes=33, grid_halfwidth=8.0, lower=-6.0, upper=4.0, first_step=0, seed=None, normalized=False,
                        n_steps=None, curvature="expected"):
    """Every subject's marginal log-likelihood log integral exp(individual_log_likelihood(eta) + logpdf(Normal(prior_mean,
    omega), eta)) d eta (src/saem.jl:55-66) with the network frozen, on the device (cude_marginal_likelihood).
    method = "quadrature": the n_nodes-point Gauss-Hermite rule centred at every subject's MAP -- refine_conditional with
    penalty weight (sigma / omega)^2 from betas (None: an 81-point scan over [lower, upper] first) -- with the Laplace
    scale sigma / sqrt(info + (sigma / omega)^2).  "importance": n_nodes device draws from that normal (steps first_step
    ... of the device stream; seed: set_rng first), self-normalised.  "grid": the trapezoid rule on n_nodes points over
    prior_mean -/+ grid_halfwidth omega, which needs no centre and misses no mode inside the range.  "laplace": the
    one-point rule ("quadrature" with n_nodes = 1), f(MAP) scale sqrt(2 pi).
    curvature = "observed" ("quadrature", "importance", "laplace"): the scale is sigma / sqrt(curv + (sigma / omega)^2) with
    the exact curvature of `curvatures` at the refined centres (one cude_curvature call) -- with "laplace" the textbook
    Laplace approximation.  A subject with curv + (sigma / omega)^2 <= 0, whose centre is no minimum, keeps the expected
    scale; the result then also has curvature_fallback, the indices of those subjects.
    Returns a namespace: logml, post_mean, post_var, post_sse, ess (N,), n_bad (N,) int32, center, scale (N,), and total =
    the sum of logml in subject order.  The likelihood follows the reference's convention (no 2 pi constant);
    normalized = True adds -(T/2) log(2 pi) per subject."""
    fallback = []
    pop, r, center, scale = _marginal_solve(betas, nn, models, timepoints, cpeptide_data, sigma, prior_mean, omega,
                                            method=method, n_nodes=n_nodes, grid_halfwidth=grid_halfwidth, lower=lower,
                                            upper=upper, first_step=first_step, seed=seed, n_steps=n_steps,
                                            curvature=curvature, fallback=fallback)
    logml = r["logml"] - 0.5 * pop.T * math.log(2.0 * math.pi) if normalized else r["logml"]
    out = SimpleNamespace(logml=logml, total=float(np.add.accumulate(logml)[-1]), post_mean=r["post_mean"],
                          post_var=r["post_var"], post_sse=r["post_sse"], ess=r["ess"], n_bad=r["n_bad"], center=center,
                          scale=scale)
    if curvature == "observed":
        out.curvature_fallback = np.array(fallback, dtype=np.int64)
    return out


def posterior_weights(terms, logml, scale=None):
    """Posterior weights of a rule's nodes from cude_marginal_likelihood's terms (K, N) and logml (N,): w_ik = exp(t_ik -
    (logml_i - log scale_i)); they sum to 1 over k for every subject with a finite logml.  A bad node has t = -Inf and gets
    w = 0 exactly (so does every node of a subject without a finite term)."""
    t = np.asarray(terms, dtype=np.float64)
    lse = np.asarray(logml, dtype=np.float64) - (0.0 if scale is None else np.log(np.asarray(scale, dtype=np.float64)))
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.exp(t - lse[None, :])
    return np.where(np.isneginf(t), 0.0, w)


def subject_scores(theta, args, *, n_steps=None):
    """The (N, P) table of per-subject scores d SSE_i / d theta.neural at the fitted conditionals theta.conditional
    (cude_subject_scores with one set and no weights); args = (models, timepoints, cpeptide_data) as `loss`.  Rows of
    failed subjects are NaN.  These rows hold the conditionals fixed: an information matrix built from them ignores the
    uncertainty of the conditionals (network_standard_errors uses the marginal scores instead)."""
    models, timepoints, data = args
    if _is_model(models):
        models, data = [models], np.asarray(data)[None, :]
    if isinstance(models[0], CPeptideODEModel):
        pop = _population(models, timepoints, data, n_steps, cond_space="raw")
        nn = getattr(theta, "neural", None)
        cond = getattr(theta, "conditional", getattr(theta, "ode", theta))
        pop.engine.set_params(pop.shared if nn is None else nn, np.asarray(cond, dtype=np.float64).reshape(-1)[:pop.N])
    else:
        pop = _population(models, timepoints, data, n_steps)
        pop.engine.set_params(theta.neural, np.asarray(theta.conditional, dtype=np.float64).reshape(-1)[:pop.N])
    return pop.engine.subject_scores(want=("scores",))["scores"]


def marginal_score(betas, nn, models, timepoints, cpeptide_data, sigma, prior_mean, omega, *, method="quadrature",
                   n_nodes=33, grid_halfwidth=8.0, lower=-6.0, upper=4.0, first_step=0, seed=None, normalized=False,
                   n_steps=None, center=None, scale=None):
    """Value and network gradient of the marginal log-likelihood that marginal_likelihood (same arguments) computes, by
    Fisher's identity: the rule is run with its points and terms kept, the posterior weights of the nodes w_ik =
    exp(t_ik - (logml_i - log scale_i)) are formed on the host (a bad node has t = -Inf, so w = 0), and
    cude_subject_scores folds the per-node gradient rows with them: s_i = sum_k w_ik d SSE_i(x_ik) / d theta.
    Returns a namespace: logml (N,), total, scores = -s_i / (2 sigma^2) (N, P) -- every subject's own gradient of logml_i
    --, gradient = -sum_i s_i / (2 sigma^2) (P,), opg = sum_i s_i s_i^T / (4 sigma^4) (P, P), wsse (N,) = the posterior
    expectation of the SSE, n_failed, center, scale.
    This is the derivative of the RULE's value with its points and weights held fixed.  With points re-centred at a MAP
    that itself depends on the network ("quadrature", "importance") it omits the dependence of the nodes on the network;
    that dependence is of the order of the rule's own quadrature error (it vanishes for the exact integral), and it is
    absent for method = "grid", whose nodes do not move.  The K x N weights cross to the host and back once, and the
    forward half of every node's solve runs twice: once for the weights, once under the adjoint."""
    pop, r, center, scale = _marginal_solve(betas, nn, models, timepoints, cpeptide_data, sigma, prior_mean, omega,
                                            method=method, n_nodes=n_nodes, grid_halfwidth=grid_halfwidth, lower=lower,
                                            upper=upper, first_step=first_step, seed=seed, n_steps=n_steps, want=True,
                                            center=center, scale=scale)
    w = posterior_weights(r["terms"], r["logml"], scale)
    s = pop.engine.subject_scores(r["points"], w)
    n_failed = pop.engine.n_failed()
    c = 1.0 / (2.0 * float(sigma) ** 2)
    logml = r["logml"] - 0.5 * pop.T * math.log(2.0 * math.pi) if normalized else r["logml"]
    return SimpleNamespace(logml=logml, total=float(np.add.accumulate(logml)[-1]), scores=-c * s["scores"],
                           gradient=-c * s["sum"], opg=(c * c) * s["cross"], wsse=s["wsse"], n_failed=n_failed,
                           center=center, scale=scale, post_mean=r["post_mean"], post_var=r["post_var"],
                           post_sse=r["post_sse"])


def opg_covariance(opg):
    """(cov, se) from an outer-product-of-gradients information matrix: cov = pinv(opg) (the matrix has rank at most the
    number of subjects, and less with frozen parameters, whose rows and columns are zero), se = sqrt(diag(cov))."""
    m = np.asarray(opg, dtype=np.float64)
    cov = np.linalg.pinv(0.5 * (m + m.T), hermitian=True)
    return cov, np.sqrt(np.clip(np.diag(cov), 0.0, None))


def network_standard_errors(betas, nn, models, timepoints, cpeptide_data, sigma, prior_mean, omega, *, estimator="opg",
                            **kwargs):
    """Standard errors of the network parameters.  estimator = "expected": from the expected (Gauss-Newton) information with
    the conditionals fitted, cov = sigma^2 pinv(S) with S network_information's schur under the prior omega (rank at most N
    (T - 1) - N); returns a namespace cov, se, schur, gn, rank, n_failed (prior_mean is not used; n_steps is the only further
    keyword).  estimator = "opg" (the default), from the cross-product (OPG, "S matrix") estimator of the information:
    opg = sum_i g_i g_i^T with g_i = subject i's gradient of its MARGINAL log-likelihood (marginal_score, same arguments),
    cov = pinv(opg), se = sqrt(diag(cov)).  Returns a namespace: cov (P, P), se (P,), opg, rank, gradient, total.
    The rank of opg is at most N, the number of subjects: with fewer subjects than parameters the pseudo-inverse covers
    the span of the scores only, and se is 0 outside it (rank tells).  Scores taken at fitted conditionals instead
    (subject_scores: the K = 1 table) would ignore the uncertainty of the conditionals and understate these errors; this
    function does not use them."""
    if estimator == "expected":
        info = network_information(betas, nn, models, timepoints, cpeptide_data, sigma=sigma, prior_omega=omega,
                                   n_steps=kwargs.pop("n_steps", None))
        if kwargs:
            raise TypeError(f"estimator='expected' takes no {sorted(kwargs)}")
        cov = float(sigma) ** 2 * _pinv_sym(info["schur"])
        return SimpleNamespace(cov=cov, se=np.sqrt(np.clip(np.diag(cov), 0.0, None)), schur=info["schur"], gn=info["gn"],
                               rank=int(np.linalg.matrix_rank(info["schur"], hermitian=True)), n_failed=info["n_failed"])
    if estimator != "opg":
        raise ValueError(f"estimator must be 'opg' or 'expected', got {estimator!r}")
    ms = marginal_score(betas, nn, models, timepoints, cpeptide_data, sigma, prior_mean, omega, **kwargs)
    cov, se = opg_covariance(ms.opg)
    return SimpleNamespace(cov=cov, se=se, opg=ms.opg, rank=int(np.linalg.matrix_rank(ms.opg, hermitian=True)),
                           gradient=ms.gradient, total=ms.total)


# ----------------------------------------------------------------------------- expected information (Gauss-Newton)
def _params_set(theta, args, n_steps):
    """The population of args = (models, timepoints, cpeptide_data) with theta's parameters set, as subject_scores."""
    models, timepoints, data = args
    if _is_model(models):
        models, data = [models], np.asarray(data)[None, :]
    if isinstance(models[0], CPeptideODEModel):
        pop = _population(models, timepoints, data, n_steps, cond_space="raw")
        nn = getattr(theta, "neural", None)
        cond = getattr(theta, "conditional", getattr(theta, "ode", theta))
        pop.engine.set_params(pop.shared if nn is None else nn, np.asarray(cond, dtype=np.float64).reshape(-1)[:pop.N])
    else:
        pop = _population(models, timepoints, data, n_steps)
        pop.engine.set_params(theta.neural, np.asarray(theta.conditional, dtype=np.float64).reshape(-1)[:pop.N])
    return pop


def output_jacobian(theta, args, *, n_steps=None):
    """(jac (N, T, P), jcond (N, T)): the derivative of every subject's predicted c-peptide at the data's times with respect
    to the shared parameters theta.neural and to its own conditional parameter, at theta (cude_network_information); args =
    (models, timepoints, cpeptide_data) as `loss`.  The column of t_0 is exactly zero; rows of failed subjects are NaN."""
    out = _params_set(theta, args, n_steps).engine.network_information(want=("jac", "jcond"))
    return out["jac"], out["jcond"]


def _penalty_weight(sigma, prior_omega):
    return 0.0 if prior_omega is None else (float(sigma) / float(prior_omega)) ** 2


def _information(eng, pw):
    out = eng.network_information(penalty_weight=pw, want=("gn", "schur", "coupling", "dcond", "status"))
    out = {k: out[k] for k in ("gn", "schur", "coupling", "dcond", "status")}
    out["penalty_weight"], out["n_failed"] = pw, eng.n_failed()
    return out


def network_information(betas, nn, models, timepoints, cpeptide_data, *, sigma, prior_omega=None, n_steps=None):
    """Expected-information (Gauss-Newton) matrices of the network parameters at the fitted conditionals betas: dict(gn (P,
    P) = A = sum_i J_i^T J_i, the information with the conditionals taken as known; schur (P, P) = A - sum_i b_i b_i^T / (d_i
    + pw), the information with the conditionals fitted (the Schur complement of the arrowhead matrix); coupling (N, P) =
    b_i; dcond (N,) = d_i; status (N,): bit 1 failed, bit 2 flat; penalty_weight; n_failed), all in units of 1 / sigma^2.
    pw = sigma^2 / prior_omega^2 when the conditionals have a Gaussian prior of standard deviation prior_omega, else 0."""
    theta = ComponentArray(neural=nn, conditional=np.asarray(betas, dtype=np.float64).reshape(-1))
    pop = _params_set(theta, (models, timepoints, cpeptide_data), n_steps)
    return _information(pop.engine, _penalty_weight(sigma, prior_omega))


def map_curvature(betas, nn, models, timepoints, cpeptide_data, *, sigma, prior_omega=None, n_steps=None):
    """Is every subject's fitted conditional a minimum of its MAP objective SSE_i + pw (beta - prior mean)^2?  One
    cude_curvature call at betas.  Returns a namespace of (N,) arrays: observed = curv + pw (half the second derivative of
    the objective; <= 0: no minimum), expected = info + pw (its Gauss-Newton part, what the fits and the Laplace scale
    use), ratio = observed / expected, and status: "minimum", "not_a_minimum" (observed <= 0) or "failed" (a failed
    subject).  pw = sigma^2 / prior_omega^2 when the conditionals have a Gaussian prior of standard deviation prior_omega,
    else 0 (the prior's mean does not enter a second derivative)."""
    theta = ComponentArray(neural=nn, conditional=np.asarray(betas, dtype=np.float64).reshape(-1))
    _, curv, info, _, _ = curvatures(theta, (models, timepoints, cpeptide_data), n_steps=n_steps)
    pw = _penalty_weight(sigma, prior_omega)
    observed, expected = curv + pw, info + pw
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = observed / expected
        status = np.where(np.isnan(observed), "failed", np.where(observed > 0.0, "minimum", "not_a_minimum"))
    return SimpleNamespace(observed=observed, expected=expected, ratio=ratio, status=status)


def train_lm(models, timepoints, cpeptide_data, nn, betas, *, max_iters=50, n_trials=4, mu0=1e-2, gtol=0.0, ftol=0.0,
             n_steps=None):
    """Levenberg-Marquardt fit of the network parameters and every subject's conditional parameter from (nn, betas) on the
    device (cude_train_lm: Gauss-Newton steps on network_information's matrices, n_trials dampings tried side by side per
    iteration).  Returns dict(nn, betas, objective, trace (n_iters + 1,), mu, n_iters, status = one of LM_STATUS)."""
    theta = ComponentArray(neural=nn, conditional=np.asarray(betas, dtype=np.float64).reshape(-1))
    eng = _params_set(theta, (models, timepoints, cpeptide_data), n_steps).engine
    res = eng.train_lm(max_iters=max_iters, n_trials=n_trials, mu0=mu0, gtol=gtol, ftol=ftol)
    nn_out, cond_out = eng.get_params()
    return {"nn": nn_out, "betas": cond_out, "objective": float(res["trace"][-1]), "trace": res["trace"], "mu": res["mu"],
            "n_iters": res["n_iters"], "status": LM_STATUS[res["status"]]}


def _pinv_sym(m, rcond=1e-12):
    """Pseudo-inverse of a symmetric information matrix.  S = A - sum_i t_i t_i^T is rank-deficient whenever P exceeds N (n_out
    - 2), and its null directions come out of the subtraction as rounding residue of the order of 1e-16 of the largest
    eigenvalue: eigenvalues below rcond of the largest are taken as zero."""
    m = np.asarray(m, dtype=np.float64)
    return np.linalg.pinv(0.5 * (m + m.T), rcond=rcond, hermitian=True)


def network_covariance(betas, nn, models, timepoints, cpeptide_data, *, sigma, prior_omega=None, n_steps=None):
    """sigma^2 pinv(S): the covariance of the network parameters from the expected information with the conditionals
    fitted (network_information's schur)."""
    info = network_information(betas, nn, models, timepoints, cpeptide_data, sigma=sigma, prior_omega=prior_omega,
                               n_steps=n_steps)
    return float(sigma) ** 2 * _pinv_sym(info["schur"])


def _prediction_se(eng, sigma, pw):
    """(se (N, n_out), info): a first call for S, a second with cov = pinv(S) and profiled rows."""
    info = _information(eng, pw)
    out = eng.network_information(penalty_weight=pw, cov=_pinv_sym(info["schur"]), profiled=True,
                                  want=("jcond", "dcond", "qform", "status"))
    den = out["dcond"] + pw
    flat = (out["status"] & 2) != 0
    own = np.where(flat[:, None], 0.0, out["jcond"] ** 2 / np.where(flat, 1.0, den)[:, None])
    return float(sigma) * np.sqrt(np.clip(out["qform"] + own, 0.0, None)), info


def prediction_standard_errors(betas, nn, models, timepoints, cpeptide_data, *, sigma, prior_omega=None, n_steps=None):
    """Delta-method standard errors (N, T) of the predicted c-peptide curves at the data's times, the closed-form companion
    of posterior_predictive: se_io = sigma sqrt(z S^+ z^T + jc_io^2 / (d_i + pw)), z = J_io - jc_io / (d_i + pw) b_i -- the
    variance of yhat_io under the joint Gauss-Newton covariance of the network and subject i's own conditional.  Exactly
    zero at t_0; NaN for failed subjects; a flat subject (status bit 2) contributes the network's term alone."""
    theta = ComponentArray(neural=nn, conditional=np.asarray(betas, dtype=np.float64).reshape(-1))
    pop = _params_set(theta, (models, timepoints, cpeptide_data), n_steps)
    return _prediction_se(pop.engine, sigma, _penalty_weight(sigma, prior_omega))[0]


def suppression_output_jacobian(p, args, *, n_steps=None):
    """output_jacobian for the suppression model: args = (prob, individual_data, timepoints, lambda) as suppression_loss.
    Returns (jac (N, 3 T, P), jcond (N, 3 T)) with output o = s + 3 j (state s at time j); the rows of state 0 and of t_0
    are exactly zero."""
    prob, data, timepoints, lam = args
    pop = _supp_population(prob, data, timepoints, lam, n_steps)
    pop.engine.set_params(p.neural, p.theta)
    out = pop.engine.network_information(want=("jac", "jcond"))
    return out["jac"], out["jcond"]


def suppression_network_information(p, args, *, sigma=1.0, prior_omega=None, n_steps=None):
    """network_information for the suppression model, with the loss's weights 1 / scale_s^2 on the outputs of state s."""
    prob, data, timepoints, lam = args
    pop = _supp_population(prob, data, timepoints, lam, n_steps)
    pop.engine.set_params(p.neural, p.theta)
    return _information(pop.engine, _penalty_weight(sigma, prior_omega))


def _marginal_em_rounds(x0, hyper0, objective, update, rounds, iterations):
    """The loop of train_marginal on any objective: per round L-BFGS (at most `iterations` accepted iterations) on
    x -> objective(x, hyper) = (-total, -gradient, moments), then hyper = update(moments of the round's last accepted
    point).  Returns (x, hyper, trace, starts): trace holds `total` at the start of every round and after every accepted
    iteration, starts the positions in it at which the rounds begin."""
    x, hyper, trace, starts = np.array(x0, dtype=np.float64), hyper0, [], []
    for _ in range(int(rounds)):
        seen = {}
        starts.append(len(trace))

        def fg(p, hyper=hyper, seen=seen):
            f, g, moments = objective(p, hyper)
            seen[p.tobytes()] = moments
            return f, g

        f0, _ = fg(x)
        trace.append(-float(f0))
        if not np.isfinite(f0):
            break
        res = lbfgs(fg, x, maxiters=int(iterations), callback=lambda p, f: trace.append(-float(f)) or False)
        x = res["x"]
        moments = seen.get(x.tobytes())
        if moments is None:
            moments = objective(x, hyper)[2]
        hyper = update(moments)
    return x, hyper, trace, starts


def train_marginal(nn, models, timepoints, cpeptide_data, sigma, prior_mean, omega, *, rounds=1, iterations=5,
                   method="grid", n_nodes=33, grid_halfwidth=8.0, n_steps=None, **kwargs):
    """Direct maximum-marginal-likelihood training of the network (quadrature EM): per round, L-BFGS on -total over the
    network parameters with marginal_score as value and gradient -- the rule's nodes fixed for the round (method = "grid":
    they never move; otherwise the MAP centres of the round's first point are kept) -- then the closed-form EM updates
    (em_updates) of (sigma^2, prior_mean, omega^2) from the posterior moments at the round's last point.  Returns a
    namespace: nn, sigma, prior_mean, omega, trace = `total` at the start of every round and after every accepted L-BFGS
    iteration (inside a round it never decreases: the line search only accepts a decrease of -total), round_starts = where
    in the trace the rounds begin."""
    T = len(timepoints)
    state = {"center": None, "scale": None}

    def objective(p, hyper):
        s, m, o = hyper
        ms = marginal_score(None, p, models, timepoints, cpeptide_data, s, m, o, method=method, n_nodes=n_nodes,
                            grid_halfwidth=grid_halfwidth, n_steps=n_steps, center=state["center"], scale=state["scale"],
                            **kwargs)
        if method != "grid" and state["center"] is None:
            state["center"], state["scale"] = ms.center, ms.scale
        if ms.n_failed > 0 or not np.isfinite(ms.total):
            return np.inf, np.zeros_like(p), None
        return -ms.total, -ms.gradient, (ms.post_mean, ms.post_var, ms.wsse)

    def update(moments):
        state["center"] = state["scale"] = None
        s2, mu, o2 = em_updates(*moments, T)
        return math.sqrt(s2), mu, math.sqrt(o2)

    x, hyper, trace, starts = _marginal_em_rounds(np.asarray(nn, dtype=np.float64).reshape(-1),
                                                  (float(sigma), float(prior_mean), float(omega)), objective, update, rounds,
                                                  iterations)
    return SimpleNamespace(nn=x, sigma=hyper[0], prior_mean=hyper[1], omega=hyper[2], trace=trace, round_starts=starts)


def information_criteria(total_logml, n_params, n_subjects, n_obs):
    """AIC and BIC from a population's marginal log-likelihood (marginal_likelihood(...).total, with normalized = True
    when models of different error structure are compared): dict(aic = -2 logL + 2 p, bic = -2 logL + p log(n_subjects
    n_obs) -- the penalty counts every observation --, bic_subjects = -2 logL + p log(n_subjects), the count of independent
    units some authors prefer for mixed-effects models)."""
    dev = -2.0 * float(total_logml)
    return {"aic": dev + 2.0 * n_params, "bic": dev + n_params * math.log(n_subjects * n_obs),
            "bic_subjects": dev + n_params * math.log(n_subjects)}


def em_updates(post_mean, post_var, post_sse, n_obs):
    """The closed-form EM updates from the posterior moments cude_marginal_likelihood leaves: (sigma2, mu, omega2) with
    sigma2 = sum_i E[SSE_i] / (N n_obs), mu = mean_i E[eta_i], omega2 = mean_i (Var[eta_i] + (E[eta_i] - mu)^2)."""
    m, v, s = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (post_mean, post_var, post_sse))
    mu = float(np.mean(m))
    return float(np.sum(s) / (m.size * n_obs)), mu, float(np.mean(v + (m - mu) ** 2))


# ----------------------------------------------------------------------------- symbolic (Michaelis-Menten) model
def train_symbolic(models, timepoints, cpeptide_data, *, lower=0.0, upper=1000.0, n_steps=None, method="search"):
    """The per-subject loop of c-peptide/03-symreg.jl:94-106: minimise loss_sigma over (k, sigma) with
    0 <= k <= 1000 for every CPeptideODEModel.  For fixed k the optimum is sigma^2 = SSE/n, and k minimises the
    SSE, so all N problems are solved together by a bracketing search on log k (one forward launch per probe).
    Returns OptimizationSolution(u = ComponentArray(ode=[k], sigma), objective) per subject.  method = "newton": the
    61-point scan as one profile launch, then cude_refine_conditional from every argmin."""
    pop = _population(models, timepoints, cpeptide_data, n_steps, cond_space="log")
    eng, N = pop.engine, pop.N
    eng.set_params(pop.shared, np.zeros(N))
    lo = math.log(max(lower, 1e-6))
    hi = math.log(upper)

    logk, _, val, _ = _fit_box(eng, lo, hi, 61, 48, method)
    n = len(timepoints)
    sigma = np.sqrt(np.maximum(val, 1e-300) / n)
    obj = (n / 2) * np.log(sigma ** 2) + val / (2 * sigma ** 2)
    return [OptimizationSolution(u=ComponentArray(ode=np.array([k]), sigma=s), objective=o)
            for k, s, o in zip(np.exp(logk), sigma, obj)]


def SAEM_symbolic(models, timepoints, cpeptide_data, initial_population_parameter, *, sigma=1.0, prior_eta=0.0,
                  prior_omega=1.0, iterations=500, n_burnin_iterations=100, proposal_std=0.1,
                  proposal_std_bounds=(1e-3, 1.0), alpha=0.7, n_mcmc_steps=1, initial_mcmc_steps=None,
                  target_acceptance_rate=0.25, initial_temperature=10.0, temperature_decay=0.05,
                  omega_learning_rate=0.04, rng=None, n_steps=None, m_step_iters=5):
    """SAEM(individuals, initial_population_parameter; ...) of src/saem-symreg.jl:134-229: random effects eta_i
    with k_i = km_pop * exp(eta_i) (:57-59), Metropolis E-step (:86-108) on the device through the log-space
    conditional log k_i = log km_pop + eta_i (prior Normal(0, Omega) on eta), M-step = `m_step_iters` L-BFGS
    iterations on (km, sigma) of total_nll (:110-131) with the device gradient."""
    rng = np.random.default_rng() if rng is None else rng
    initial_mcmc_steps = n_mcmc_steps if initial_mcmc_steps is None else initial_mcmc_steps
    pop = _population(models, timepoints, cpeptide_data, n_steps, cond_space="log")
    eng, N, T = pop.engine, pop.N, pop.T
    eta = np.full(N, float(prior_eta))
    km = float(initial_population_parameter)
    omega = float(prior_omega)
    nll_values, acc_rates = [], []
    for it in range(1, iterations + 1):
        gamma = 1.0 if it <= n_burnin_iterations else 1.0 / (it - n_burnin_iterations) ** alpha
        steps = initial_mcmc_steps if it <= n_burnin_iterations else n_mcmc_steps
        temperature = max(1.0, initial_temperature * math.exp(-temperature_decay * it))
        # E-step: the chain state on the device is log k = log km + eta, so the prior is centred on log km
        eng.set_params(pop.shared, math.log(km) + eta)
        n_acc = eng.mh_estep(rng.standard_normal((steps, N)), rng.random((steps, N)), sigma, math.log(km), omega,
                             proposal_std, temperature, gamma)
        eta = eng.get_params()[1] - math.log(km)
        sse = eng.forward(want_sse=True)["sse"]
        loglik = float(individual_log_likelihood(sse, T, sigma).sum())

        def fg(x):                                   # total_nll(km, eta, individuals, sigma) and its gradient
            k_pop, s = x
            if k_pop <= 0 or s <= 0:
                return np.inf, np.zeros(2)
            eng.set_params(None, math.log(k_pop) + eta)
            mean_sse, _, g_log = eng.loss_grad()
            val = N * T / 2 * math.log(s * s) + N * mean_sse / (2 * s * s)
            return val, np.array([N * g_log.sum() / k_pop / (2 * s * s), N * T / s - N * mean_sse / s ** 3])
        res = lbfgs(fg, np.array([km, sigma]), maxiters=m_step_iters)
        km_new, sigma = float(res["x"][0]), float(res["x"][1])
        km = (1 - gamma) * km + gamma * km_new
        omega = (1 - omega_learning_rate) * omega + omega_learning_rate * float(np.var(eta, ddof=1))
        rate = int(n_acc.sum()) / (N * steps)
        nll_values.append(-loglik)
        acc_rates.append(rate)
        if it > n_burnin_iterations:
            proposal_std = float(np.clip(math.exp(math.log(proposal_std) + gamma * (rate - target_acceptance_rate)),
                                         proposal_std_bounds[0], proposal_std_bounds[1]))
    return SimpleNamespace(km_pop=km, eta=eta, Omega=omega, sigma=sigma, total_nll_values=nll_values,
                           acceptance_rates=acc_rates)


def simulate(p_neural, p_individuals, models, timepoints, cpeptide_data, *, out_timepoints=None, n_steps=None,
             save_idxs=1):
    """`simulate(p_neural, p_individual, individual, network; timepoints)` of src/saem.jl:31-53 (and
    src/saem-symreg.jl:31-53 for CPeptideODEModel lists, p_neural = None) for ALL individuals at once: plasma
    c-peptide (state `save_idxs`, 1-based as in Julia) at `out_timepoints` -- any non-decreasing times inside the
    span of `timepoints`, e.g. the dense grids t0:0.1:tend of the model-fit figures -- as an (N, n_times) array."""
    sym = isinstance(models[0], CPeptideODEModel)
    pop = _population(models, timepoints, cpeptide_data, n_steps, cond_space="raw" if sym else "log")
    if isinstance(models[0], CPeptideUDEModel):      # `solve(model.problem, p = neural_network_parameters)` per subject
        pop.engine.set_params(models[0].embed(p_neural), np.zeros(len(models)))   # (01-non-conditional.jl:64,74)
    else:
        pop.engine.set_params(pop.shared if sym else p_neural, np.asarray(p_individuals, dtype=np.float64).reshape(-1))
    times = np.asarray(timepoints if out_timepoints is None else out_timepoints, dtype=np.float64)
    return pop.engine.simulate(times)[save_idxs - 1].T


# ----------------------------------------------------------------------------- checkpoints / data files (JLD2)
def load_data(path):
    """`jldopen("data/ohashi.jld2") do file; file["train"], file["test"]; end` (c-peptide/02-conditional.jl:15-17):
    every top-level entry of a JLD2 file; NamedTuples become SimpleNamespaces with numpy fields."""
    from . import jld2
    out = {}
    for k, v in jld2.load(path).items():
        out[k] = SimpleNamespace(**v) if isinstance(v, dict) else v
    return out


def save_parameters(path, width, depth, parameters, betas=None, best_model_index=None, **extra):
    """The checkpoint the training scripts write (c-peptide/02-conditional.jl:44-50, 07-covariate-inclusion.jl:59-65):
    width, depth, parameters, betas, best_model_index (1-based, as in the reference).  Lists of vectors are stored
    as Vector{Vector{Float64}}, so the reference's `file["parameters"][best_model_index]` reads them unchanged; with
    the reference's content the file is byte-identical to the one JLD2.jl wrote (tests/test_jld2.py)."""
    from . import jld2
    entries = {"width": int(width), "depth": int(depth), "parameters": parameters}
    if betas is not None:
        entries["betas"] = betas
    if best_model_index is not None:
        entries["best_model_index"] = int(best_model_index)
    entries.update(extra)
    jld2.save(path, entries)


def load_parameters(path):
    """Reads a checkpoint written by the reference or by save_parameters (vectors of vectors; a matrix is taken as
    one vector per column):
    namespace with width, depth, parameters (list of vectors, or one vector), betas, best_model_index."""
    from . import jld2
    d = jld2.load(path)

    def as_list(v):
        if isinstance(v, np.ndarray) and v.ndim == 2:
            return [v[:, j].copy() for j in range(v.shape[1])]
        return v
    return SimpleNamespace(width=d.get("width"), depth=d.get("depth"), parameters=as_list(d.get("parameters")),
                           betas=as_list(d.get("betas")), best_model_index=d.get("best_model_index"),
                           extra={k: v for k, v in d.items()
                                  if k not in ("width", "depth", "parameters", "betas", "best_model_index")})
