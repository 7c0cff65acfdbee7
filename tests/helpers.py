"""Shared helpers for the parity tests."""
import copy
import os

import numpy as np

import scenarios as SC  # tests/golden/scenarios.py
from pcgym_amd.config import EnvSpec

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


GOLD_LOADS = [0]  # tests/conftest.py: which GPU tests check against a committed reference fixture


def gold(name):
    GOLD_LOADS[0] += 1
    return np.load(os.path.join(GOLD, name + ".npz"))


def rel_err(a, b, floor=1e-300):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)) if a.size else 0.0


def close(a, b, rtol, atol=0.0):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.all(np.abs(a - b) <= atol + rtol * np.abs(b))


def scenario_spec(name, **overrides):
    sc = SC.scenarios()[name]
    p = copy.deepcopy(sc["env_params"])
    p.update(overrides)
    return EnvSpec(p), sc


# integrator settings that make the time-discretisation error negligible (<1e-10)
# against the LSODA(1e-12) recordings, so the epilogue parity is tested tightly
TIGHT = {
    "cstr": dict(integrator="rk4", substeps=64),
    "four_tank": dict(integrator="rk4", substeps=128),
    "multistage_extraction": dict(integrator="dopri5", rtol=1e-12, atol=1e-14),
    "multistage_extraction_reactive": dict(integrator="dopri5", rtol=1e-12, atol=1e-14),
    "crystallization": dict(integrator="rk4", substeps=512),
    None: dict(integrator="rk4", substeps=64),
    "complex_cstr": dict(integrator="dopri5", rtol=1e-12, atol=1e-14),
    "photobioreactor": dict(integrator="dopri5", rtol=1e-12, atol=1e-14),
    "distillation_column": dict(integrator="dopri5", rtol=1e-12, atol=1e-14),
    "first_order_system": dict(integrator="rk4", substeps=64),
    "biofilm_reactor": dict(integrator="dopri5", rtol=1e-12, atol=1e-14),
    "heat_exchanger": dict(integrator="dopri5", rtol=1e-12, atol=1e-14),
    "disease": dict(integrator="dopri5", rtol=1e-12, atol=1e-14),
    "batch": dict(integrator="dopri5", rtol=1e-12, atol=1e-14),
    "cstr_series_recycle": dict(integrator="dopri5", rtol=1e-12, atol=1e-14),
    "polymerisation_reactor": dict(integrator="dopri5", rtol=1e-12, atol=1e-14),
    "hydraulic_tank": dict(integrator="rk4", substeps=64),
    "nonsmooth_control": dict(integrator="rk4", substeps=64),
    "invariant_batch": dict(integrator="dopri5", rtol=1e-12, atol=1e-14),
    "coupled_oscillator": dict(integrator="dopri5", rtol=1e-12, atol=1e-14),
}


def tight_for(env_params):
    return TIGHT[env_params.get("model")]


# ---- adaptive (DOPRI5) parity -------------------------------------------------------------------------------------
# The GPU and the oracle take IDENTICAL step sequences -- every env, checked as equality of the accepted / rejected
# counts, states to round-off -- on every adaptive plan.  Two things make that possible (DESIGN.md "Adaptive stepping"):
#   * the step-size factor is quantised (6 mantissa bits), so it does not depend on how E^(-1/5) is evaluated (fp32
#     log2/exp2 units in the kernels, double pow() in the oracle);
#   * the arithmetic that feeds back into the state is an exactly specified sequence of IEEE operations: the stage
#     combinations of the 5(4) pair are explicit FMAs in a fixed order on both sides, the action map follows the
#     reference's own operation order, and the one model that needs it -- the 10-state extraction model, which runs the
#     explicit pair at its STABILITY limit (|lambda| dt ~ 240), where the embedded error estimate is round-off amplified
#     ~1e8 x and a last-bit difference of one RHS evaluation changes the step sequence a few steps later -- has a
#     right-hand side with a fixed operation order and a bit-identical twin in the oracle.
# Measured on the GPU (tools/parity_probe.py, profiles/r2/parity_probe.txt): before the second point, 3-5 % of 4096
# extraction envs took a different (equally valid) sequence and 20-30 % differed by more than 1e-11; after it, 100 %
# identical counts and BIT-IDENTICAL states; the accuracy-limited models were at 100 % / 1e-13 throughout.
# models whose right-hand side is an exactly specified operation sequence with a bit-identical twin in the oracle: the
# step sequences are identical by construction, for every env, always
BIT_EXACT_RHS = ("multistage_extraction",)


def adaptive_check(model_name, x_gpu, x_orc, ns_gpu, ns_orc, tag, tol=1e-11, x_truth=None):
    """x_* (nx, B); ns_* (2, B) accepted / rejected counts."""
    xs = np.maximum(np.abs(x_orc), 1e-6 * np.max(np.abs(x_orc), axis=1, keepdims=True))
    ex = np.max(np.abs(x_gpu - x_orc) / xs, axis=0)
    same = np.all(ns_gpu == ns_orc, axis=0)
    if model_name in BIT_EXACT_RHS:
        assert same.all(), (tag, "identical step counts", same.mean())
        assert ex.max() <= tol, (tag, ex.max())
    else:
        # A right-hand side that is not bit-identical on the two sides (contraction, OCML vs libm) perturbs the error
        # norm by ~1e-8 relative; a decision that lands that close to a threshold (E = 1, or an edge of the 6-bit factor
        # grid) flips.  Soak run, 400 random configurations x 770 envs x ~20 steps (PCG_FUZZ_SEEDS=400): one env step
        # with 8 instead of 9 accepted steps, its state 2.6e-13 from the oracle's.  So: (almost) every env identical,
        # the rest (at most one env, or 0.2 % of a large batch) within the integrator's own accuracy class.
        assert (~same).sum() <= max(1, int(0.002 * same.size)), (tag, "identical step counts", same.mean())
        assert ex[same].max() <= tol, (tag, ex[same].max())
        if not same.all():
            assert ex[~same].max() <= max(1e3 * tol, 1e-9), (tag, "envs with another step sequence", ex[~same].max())
    return ex


# ---- the sweep configurations (tests/test_gpu_sweeps.py, tests/test_gpu_tile_walks.py) ----------------------------------------
FIXED = ("rk4", "cv8")
GUARDED = ("rk4g", "tsit5g")  # models with a guard hook only (pcg_models.hpp: has_guard -- the cstr)
FULL = ("cstr", "four_tank", "multistage_extraction", "multistage_extraction_reactive", "crystallization",
        "first_order_system", "hydraulic_tank", "nonsmooth_control")  # Model::FULL: streaming / pipelined / LDS-stage kernels


def _models():
    """first scenario of every registry model (the tools' rule)"""
    out, seen = [], set()
    for name, sc in SC.scenarios().items():
        p0 = sc["env_params"]
        m = p0.get("model")
        if m is None or m in seen or p0.get("custom_model") is not None:
            continue
        seen.add(m)
        out.append((m, name))
    return out


MODELS = _models()
SCEN = dict(MODELS)
# the extraction models carry two instantiations each: eq_exponent == 2 (the reference's default: multiply-only kernels,
# PCG_KID_ME_SQ / _REACTIVE_SQ) and the pow() form (Model<PCG_MODEL_ME>, <PCG_MODEL_ME_REACTIVE>): "^1.5" selects the latter
MODEL_KEYS = [m for m, _ in MODELS] + ["multistage_extraction^1.5", "multistage_extraction_reactive^1.5"]


def _registry_object(model, **params):
    """an object the way the reference's registry classes look to make_env (pcgym.py:150-153): class name, info()"""
    from pcgym_amd.models import get_model

    mi = get_model(model)
    info = {"parameters": {**mi.parameters, **params}, "states": list(mi.states), "inputs": list(mi.inputs),
            "disturbances": list(mi.disturbances)}
    return type(model, (), {"info": lambda self: info, "int_method": "hip"})()


def sweep_params(key, integ, feat="scen", **over):
    """env_params of the model's first scenario under `integ`, in one of three feature sets:
      scen  as the scenario has it
      lean  nothing beyond the set-point reward (the kernels' lean forms: EXTRAS = false, pipelined / streaming paths)
      cons  lean + one constraint row with the penalty on (EXTRAS = true, the feature-masked kernels of the small models)"""
    model, _, expo = key.partition("^")
    p = copy.deepcopy(SC.scenarios()[SCEN[model]]["env_params"])
    if expo:
        p["custom_model"] = _registry_object(model, eq_exponent=float(expo))
    p.update(integrator=integ, rtol=1e-6, atol=1e-8)
    if integ in FIXED + GUARDED:
        p.pop("rtol"), p.pop("atol")
    if integ == "cv8" and model.startswith("multistage"):
        p["substeps"] = 256  # (the model's default plan is implicit: the order-8 scheme's own default step is unstable here)
    for k in ("uncertainty_percentages", "uncertainty_bounds", "distribution", "empirical_distribution"):
        p.pop(k, None)
    if feat != "scen":
        for k in ("a_delta", "a_0", "a_space_act", "noise", "noise_percentage", "constraints", "done_on_cons_vio",
                  "r_penalty", "custom_reward"):
            p.pop(k, None)
        if not p.get("SP"):  # terminal-reward scenarios: a set point on the first state instead
            from pcgym_amd.models import get_model

            mi = get_model(model)
            nx = len(mi.states)
            x0 = np.asarray(p["x0"], dtype=float)[:nx]
            for k in ("reward_states", "maximise_reward"):
                p.pop(k, None)
            sp = float(x0[0]) if x0[0] != 0 else 0.5
            p["SP"] = {mi.states[0]: [sp] * int(p["N"])}
            p["x0"] = np.concatenate([x0, [sp]])
            lo, hi = np.asarray(p["o_space"]["low"], dtype=float)[:nx], np.asarray(p["o_space"]["high"], dtype=float)[:nx]
            p["o_space"] = {"low": np.concatenate([lo, [min(0.0, 2 * sp)]]), "high": np.concatenate([hi, [max(1.0, 2 * sp)]])}
            p["r_scale"] = {mi.states[0]: 1.0}
    if feat == "cons":
        c0 = float(np.asarray(p["x0"], dtype=float)[0])
        p.update(constraints=lambda x, u, c0=c0: np.array([x[0] - c0]).reshape(-1,), done_on_cons_vio=False, r_penalty=True)
    p.update(over)
    return p


ROS = ("rodas3", "rodas4", "rodas5")


def _bars(key, integ):
    """(largest difference over every lane, share of lanes with the oracle's step sequence) one env step may show.
    The pow() form of the extraction cascades under an EXPLICIT adaptive pair runs at its stability limit, where the
    embedded error estimate is round-off amplified ~1e8 x: pow() of libm here and of OCML there differ in the last bit, a
    few steps later the sequences do, and the results agree to the plan's tolerance (1e-6), not to round-off -- the
    multiply-only form (eq_exponent == 2, the reference's default) has a bit-identical twin and is held to round-off
    like every other model (tests/helpers.py "adaptive parity")."""
    if "^" in key and integ in ("dopri5", "tsit5"):
        return 5e-6, 0.5
    if key == "crystallization" and integ in ROS:
        # moments from 1e-1 to 1e9 in one state vector: the difference-quotient Jacobian's last-bit noise (dJ/J ~ 1e-8)
        # passes through an LU of that conditioning; measured 1.1e-6 on single lanes of the full action box, identical
        # step sequences (the plan's tolerance is 1e-6; every other model stays below 5e-8)
        return 5e-6, 0.98
    return 1e-6, 0.98


def _close(a, b):
    import torch

    a, b = a.double(), b.double()
    fa, fb = torch.isfinite(a), torch.isfinite(b)
    if not torch.equal(fa, fb):
        return float("inf")
    if not fa.any():
        return 0.0
    return ((a[fa] - b[fa]).abs() / b[fa].abs().clamp_min(1e-9)).max().item()


def _unc_over(model, pick=None):
    """env_params entries that make `pick` (default: the model's first two non-zero parameters) uncertain: +-3 %, uniform,
    observed in a box of +-10 %"""
    from pcgym_amd.models import get_model

    mi = get_model(model)
    if pick is None:
        pick = [k for k, v in mi.parameters.items() if float(v) != 0.0 and k not in ("N", "eq_exponent")][:2]
    return dict(uncertainty_percentages={k: 0.03 for k in pick}, distribution="uniform",
                uncertainty_bounds={"low": np.array([min(0.9 * mi.parameters[k], 1.1 * mi.parameters[k]) for k in pick]),
                                    "high": np.array([max(0.9 * mi.parameters[k], 1.1 * mi.parameters[k]) for k in pick])})


def _unc_params(key, integ):
    import pytest
    from pcgym_amd.models import get_model

    model = key.partition("^")[0]
    mi = get_model(model)
    if mi.affine_builder is not None:
        pytest.skip("affine registry models have no per-env parameter kernel")
    p = sweep_params(key, integ, "lean")
    p.update(_unc_over(model))
    return p


# VecEnv arguments of a step dispatch:
#            auto     the library's own choice at this batch size
#            odd      the same with an odd batch (one env per lane in the lean kernels: EPL = 1)
#            classic  PCG_OPT_VARIANT 1: the one-env-per-lane general kernels
#            queue    PCG_OPT_VARIANT 5: the in-workgroup work queue whatever the model and batch (adaptive pairs)
#            lds      PCG_OPT_LDS_STAGES: DOPRI5 with the stage vectors in LDS (Model::FULL)
#            stream1/2  PCG_OPT_VARIANT 2 / 3: the persistent streaming kernels, one / two envs per lane (RK4, Model::FULL)
#            nostatus  the library's own choice for a caller that keeps no per-env status byte (the lean RK4 launches of the
#                      larger full models then take the streaming kernel)
DISPATCH = {"auto": {}, "odd": {}, "classic": {"variant": 1}, "queue": {"variant": 5}, "lds": {"lds_stages": True},
            "stream1": {"variant": 2, "track_status": False}, "stream2": {"variant": 3, "track_status": False},
            "nostatus": {"track_status": False}}


def sweep_actions(spec, rng, B, lo=-1.0):
    """uniform actions over [lo, 1] of the normalised box (the full box by default), physical when the plan wants them"""
    a = rng.uniform(lo, 1, (spec.na, B))
    if not spec.normalise_a:
        a = (a + 1) * (spec.a_high - spec.a_low)[:, None] / 2 + spec.a_low[:, None]
    return a


def worst_rel(xg, xo):
    """largest difference over every lane, relative to max(|x|, 1e-6 of the component's range over the batch)"""
    ok = np.isfinite(xo).all(axis=0)
    assert np.array_equal(np.isfinite(xg).all(axis=0), ok), "failure pattern differs from the oracle's"
    if not ok.any():
        return 0.0
    xs = np.maximum(np.abs(xo[:, ok]), 1e-6 * np.max(np.abs(xo[:, ok]), axis=1, keepdims=True))
    xs = np.maximum(xs, 1e-300)
    return float(np.max(np.abs(xg[:, ok] - xo[:, ok]) / xs))


# feature-masked pipelined kernels (pcg_step_feat.hpp: RK4 plans of the two small models):
# name -> (env_params changes, VecEnv arguments, pass the `viol` buffer although no constraint is configured)
def feat_sets(model):
    p0 = SC.scenarios()[SCEN[model]]["env_params"]
    c0 = float(np.asarray(p0["x0"], dtype=float)[0])
    cons = dict(constraints=lambda x, u, c0=c0: np.array([x[0] - c0]).reshape(-1,), done_on_cons_vio=False, r_penalty=True)
    track = dict(custom_reward={"kind": "sp_track", "R": 0.05})
    return {
        "viol_only": ({}, {}, True),                    # mask 0: the lean step with the `viol` output
        "viol_autoreset": ({}, {"auto_reset": True}, True),  # FT_AR
        "cons": (cons, {}, False),                      # FT_CONS
        "track": (track, {}, False),                    # FT_TRACK
        "cons_track": ({**cons, **track}, {}, False),   # FT_CONS | FT_TRACK (the constraint-showcase configuration)
        "a_delta": ({}, {}, False),                     # FT_ALL (the only mask with FT_ADELTA)
    }


def feat_params(model, fs):
    """(env_params, VecEnv arguments, pass `viol`) of feature set `fs` (feat_sets) on the lean RK4 plan of `model`"""
    over, kw, viol = feat_sets(model)[fs]
    p = sweep_params(model, "rk4", "lean")
    p.update(over)
    if fs == "a_delta":
        a_lo, a_hi = np.asarray(p["a_space"]["low"], dtype=float), np.asarray(p["a_space"]["high"], dtype=float)
        p.update(a_delta=True, a_0=(a_lo + a_hi) / 2, a_space_act={"low": a_lo, "high": a_hi},
                 a_space={"low": -(a_hi - a_lo) / 20, "high": (a_hi - a_lo) / 20}, normalise_a=True)
    return p, dict(kw), viol


# ---- the closed-loop fused rollouts (tests/test_gpu_policy_rollout.py, tests/test_gpu_actor_rollout.py) ----------------------
LD = np.longdouble
U = 2.0 ** -53
SHAPES = {"affine": (), "1x16": (16,), "2x64": (64, 64)}
PRE_MAX = 24.0  # the tanh grid covers [-24, 24] (tanh rounds to 1 from 19.1 on); every case asserts its pre-activations lie inside


def _torch():
    import torch

    return torch


def _record(file_name, line):
    """print a measured figure and, when PCG_RECORD_DIR names a directory, append it to `file_name` there"""
    print(line)
    out = os.environ.get("PCG_RECORD_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, file_name), "a") as f:
            f.write(line + "\n")


def _launched(lib, what):
    """whether a kernel whose name contains `what` was launched since the launch record was last reset"""
    import ctypes as C

    n = lib.pcg_coverage_names(None, 0, 0)
    if n <= 1:
        return False
    buf = C.create_string_buffer(int(n))
    lib.pcg_coverage_names(buf, n, 0)
    return what in buf.value.decode()


def _launch_names(lib, reset=False):
    """mangled names of the kernels launched since the launch record was last reset; `reset` clears the record"""
    import ctypes as C

    n = lib.pcg_coverage_names(None, 0, 0)
    if n <= 1:
        if reset:
            lib.pcg_coverage_names(None, 0, 1)
        return []
    buf = C.create_string_buffer(int(n))
    lib.pcg_coverage_names(buf, n, 1 if reset else 0)
    return [s for s in buf.value.decode().split("\n") if s]


def _rollout_routes(names):
    """the open-loop rollout kernels among the mangled `names`: {route: name} with the routes of pcg_rollout_strided --
    lean2 / lean1 (rollout_kernel_lean<M, EPL>), general / lds / unc (rollout_kernel<M, INTEG, LDS, UNC>), hot"""
    import re

    out = {}
    for n in names:
        if "19rollout_kernel_leanI" in n:
            m = re.search(r"ELi([12])EEEvNS_8StepArgsE$", n)
            assert m, f"the launch record does not tell the two lean instantiations apart: {n}"
            out["lean" + m.group(1)] = n
        elif "18rollout_kernel_hotI" in n:
            out["hot"] = n
        elif "14rollout_kernelI" in n:
            m = re.search(r"ELb([01])ELb([01])EEEvNS_8StepArgsE$", n)
            assert m, f"unexpected name of a rollout_kernel instantiation: {n}"
            out["unc" if m.group(2) == "1" else "lds" if m.group(1) == "1" else "general"] = n
    return out


def _make(p, B, **kw):
    from pcgym_amd import VecEnv

    return VecEnv(copy.deepcopy(p), n_envs=B, **kw)


def make_policy(spec, obs0, hidden, seed, activation="tanh", out_map="clip", out_low=None, out_high=None):
    """Fixed-seed weights, scaled by the plan's own boxes so that the units are not saturated and a fair share of the outputs
    lies strictly inside the clip box: the first layer divides each input by the size of its observation box (1 when the plan
    normalises) and is centred on the mean reset observation, the output layer spans about the action box's half width around
    its middle.  `activation` and `out_map` are MLPPolicy's; the clip box is the whole action box unless `out_low` / `out_high`
    say otherwise.  Under out_map "tanh" the output layer spans [-1, 1] whatever the action box (the map's own range).  The
    random draws do not depend on these four arguments."""
    from pcgym_amd import MLPPolicy

    rng = np.random.default_rng(seed)
    n_in, n_out = spec.nobs, spec.na
    if spec.normalise_o:
        s_in = np.ones(n_in)
    else:
        s_in = np.maximum(np.maximum(np.abs(spec.o_low), np.abs(spec.o_high)), 1e-3)
    centre = np.mean(obs0, axis=1)
    if spec.normalise_a or out_map == "tanh":
        lo, hi = -np.ones(n_out), np.ones(n_out)
    else:
        lo, hi = np.asarray(spec.a_low, dtype=float), np.asarray(spec.a_high, dtype=float)
    mid, half = (hi + lo) / 2, np.maximum((hi - lo) / 2, 1e-3)
    dims = [n_in, *hidden, n_out]
    Ws, bs = [], []
    for l in range(len(dims) - 1):
        W = rng.standard_normal((dims[l + 1], dims[l])) / np.sqrt(dims[l])
        b = 0.2 * rng.standard_normal(dims[l + 1])
        if l == len(dims) - 2:  # (fed by tanh units, which are bounded, or directly by the observation, which is not)
            W, b = (0.8 if hidden else 0.3) * half[:, None] * W, mid + 0.3 * half * rng.standard_normal(n_out)
        if l == 0:
            W = W / s_in[None, :]
            b = b - W @ centre
        Ws.append(W), bs.append(b)
    return MLPPolicy(Ws, bs, activation=activation, out_map=out_map, out_low=float(lo.min()) if out_low is None else float(out_low),
                     out_high=float(hi.max()) if out_high is None else float(out_high))


def gamma(n):
    return n * U / (1 - n * U)


def host_reference(pol, obs, k_tanh):
    """obs (n_in, M) float64 -> (policy output in np.longdouble (n_out, M), running error bound of the device's fp64
    evaluation (n_out, M), largest |pre-activation|).  Per layer the device forms fl(b + sum_i w_i x_i) with one rounding
    per FMA: |error| <= gamma_{n+1} (|b| + |W| |x|) + |W| (error of x); tanh and the clip are 1-Lipschitz, the device tanh
    adds k_tanh ulp of its value."""
    h = obs.astype(LD)
    E = np.zeros(obs.shape)
    pre = 0.0
    L = len(pol.weights)
    for l, (W, b) in enumerate(zip(pol.weights, pol.biases)):
        aW = np.abs(W)
        mag = aW @ (np.abs(h).astype(np.float64) + E) + np.abs(b)[:, None]
        E = gamma(W.shape[1] + 1) * mag + aW @ E
        h = W.astype(LD) @ h + b.astype(LD)[:, None]
        if l < L - 1:
            pre = max(pre, float(np.max(np.abs(h))))
            h = np.tanh(h) if pol.activation == "tanh" else np.maximum(h, 0)
            if pol.activation == "tanh":
                E = E + k_tanh * 2.0 ** -52 * (np.abs(h).astype(np.float64) + E)
    if pol.out_map == "clip":
        h = np.clip(h, LD(pol.out_low), LD(pol.out_high))
    elif pol.out_map == "tanh":
        h = np.tanh(h)
        E = E + k_tanh * 2.0 ** -52 * (np.abs(h).astype(np.float64) + E)
    return h, E * (1 + 2.0 ** -10), pre  # (the reference's own 64-bit-mantissa round-off: 2^-11 of the fp64 bound)


_K = {}


def tanh_k():
    """largest error of the device tanh in ulp, measured THROUGH the kernel: a policy whose single hidden unit is tanh of the
    first observation and whose output is that unit (every FMA of it is exact), on a dense grid set into io->obs"""
    if "k" in _K:
        return _K["k"]
    torch = _torch()
    from pcgym_amd import MLPPolicy

    p = copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"])
    p.update(integrator="rk4")
    grid = np.concatenate([np.linspace(-PRE_MAX, PRE_MAX, (1 << 18) + 1), np.linspace(-1.0, 1.0, (1 << 17) + 1),
                           np.geomspace(1e-300, 1.0, 4096), -np.geomspace(1e-300, 1.0, 4096)])
    B = grid.size
    env = _make(p, B, seed=1)
    env.reset()
    n_in = env.spec.nobs
    W0 = np.zeros((1, n_in))
    W0[0, 0] = 1.0
    pol = MLPPolicy([W0, np.ones((1, 1))], [np.zeros(1), np.zeros(1)], activation="tanh", out_map="none")
    env.obs_soa.zero_()
    env.obs_soa[0] = torch.as_tensor(grid, device=env.device)
    a_seq, _, _ = env.rollout_policy(pol, 1, collect_rew=False)
    torch.cuda.synchronize()
    got = a_seq[0, 0].cpu().numpy()
    env.close(), pol.close()
    want = np.tanh(grid.astype(LD))
    ulp = np.spacing(np.abs(want.astype(np.float64)))
    err = np.abs(got.astype(LD) - want).astype(np.float64) / ulp
    k = float(np.max(err))
    assert np.isfinite(k) and k <= 16.0, f"device tanh is {k} ulp off on the grid: not a libm-class tanh"
    _K["k"] = k
    _record("policy_rollout_test.txt", f"device tanh: max error {k:.3f} ulp over {B} points of [-{PRE_MAX:g}, {PRE_MAX:g}] (allowance in the action check: k + 1)")
    return k


def _case_params(key, integ):
    if key == "cstr_noise":  # observation noise: the policy sees the noisy observation, Philox keyed (seed, env, t)
        p = copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"])
        p.update(integrator=integ, noise=True, noise_percentage=0.002)
        return p
    if key == "cstr_raw":  # physical observations in, physical actions out (neither box normalised)
        p = copy.deepcopy(SC.scenarios()["cstr_raw"]["env_params"])
        p.update(integrator=integ)
        return p
    return sweep_params(key, integ, "scen")


def _spread_x0(p, pct=0.02):
    """every env its own initial state (uniform, +- pct of x0): the lanes of a wave do different arithmetic"""
    p.update(uncertainty_percentages={"x0": [pct] * 24}, distribution="uniform")
    return p


CASE_KEYS = MODEL_KEYS + ["cstr_noise", "cstr_raw"]


# ---- the feature plans of the closed-loop rollouts (tests/test_closed_loop_feature_plans.py proves each case non-vacuous on
# the oracle alone; tests/test_gpu_closed_loop_features.py runs them through the kernels) ----------------------------------------
# name -> (scenario of tests/golden/scenarios.py, env_params changes, what the plan is there for).  Kinds:
#   track    the declarative tracking reward (io->u_prev read and written every step)      box   its box-excess term
#   cryst    CV and Ln recomputed from the observed moments                                 dist  a disturbance schedule
#   gauss    Gaussian disturbances on top of the schedule                                   mask  partial observation
#   batch    the terminal batch reward                                                      noise observation noise
#   row1     one affine row over the first state and the action, b = the median of its linear part over the oracle's episode
#   rows8    PCG_MAX_NCON dense rows over a state, the SP slot, every disturbance slot, the action and the model's
#            disturbance inputs, b_r = the 0.9 quantile of row r's linear part over the oracle's episode
#   unc      _unc_over's two uncertain model parameters (q11: one of them is read by an unconfigured disturbance input)
_TRACK_RU = {"kind": "sp_track", "R": 0.1, "R_u": 0.05}  # (R_u defaults to 0, which makes its term vacuous)
FEATURE_PLANS = {
    # the base float64 / float32 families
    "cstr_paper_reward": ("cstr_paper_reward", {}, ("track",)),
    "four_tank_paper_reward_Ru": ("four_tank_paper_reward", dict(custom_reward=_TRACK_RU), ("track", "R_u")),
    "cryst_paper_reward": ("cryst_paper_reward", {}, ("track", "cryst")),
    "cstr_dist_Ti": ("cstr_dist_Ti", {}, ("dist",)),
    "cstr_dist_both": ("cstr_dist_both", {}, ("dist",)),
    "cstr_dist_Ti_gauss": ("cstr_dist_Ti", dict(gaussian_disturbances={"Ti": 1.0}), ("dist", "gauss")),
    "cstr_partial_obs": ("cstr_partial_obs", {}, ("mask",)),
    "cstr_batch_reward": ("cstr_batch_reward", {}, ("batch",)),
    # the constrained family
    "cstr_con_reward": ("cstr_con_reward", {}, ("track", "box", "cons")),
    "cstr_con_reward_noise": ("cstr_con_reward", dict(noise=True, noise_percentage=0.002), ("track", "box", "noise", "cons")),
    "cryst_paper_reward_row": ("cryst_paper_reward", {}, ("track", "cryst", "row1", "cons")),
    "me_dist_cons": ("me_dist_cons", {}, ("dist", "cons")),
    "cstr_dist_both_rows8": ("cstr_dist_both", {}, ("dist", "rows8", "cons")),
    # the per-env-parameter family
    "unc_cstr_paper_reward": ("cstr_paper_reward", {}, ("track", "unc")),
    "unc_cstr_dist_Ti": ("cstr_dist_Ti", {}, ("dist", "unc")),
    "unc_cstr_dist_Ti_Caf": ("cstr_dist_Ti", {}, ("dist", "unc", "q11")),
    "unc_cstr_noise": ("cstr_canonical", dict(noise=True, noise_percentage=0.002), ("noise", "unc")),
    "unc_cryst_adelta": ("cryst_adelta", {}, ("unc",)),
    "unc_cstr_partial_obs": ("cstr_partial_obs", {}, ("mask", "unc")),
}
BASE_FEATURE_PLANS = [n for n, v in FEATURE_PLANS.items() if "cons" not in v[2] and "unc" not in v[2]]
CONS_FEATURE_PLANS = [n for n, v in FEATURE_PLANS.items() if "cons" in v[2]]
UNC_FEATURE_PLANS = [n for n, v in FEATURE_PLANS.items() if "unc" in v[2]]
Q11_PICK = ["q", "Caf"]  # Caf: a disturbance input of the cstr that cstr_dist_Ti leaves unconfigured


def feature_params(name, integ, rows=None):
    """env_params of feature plan `name` under `integ`, every env with its own initial state (_spread_x0); `rows` = (A, b)
    of the affine constraint rows of a row1 / rows8 plan (the plan without them while the bounds are being chosen)"""
    scen, over, kinds = FEATURE_PLANS[name]
    p = copy.deepcopy(SC.scenarios()[scen]["env_params"])
    p.update(copy.deepcopy(over))
    p.update(integrator=integ)
    if integ == "cv8" and p["model"].startswith("multistage"):
        p["substeps"] = 256  # (as in sweep_params: the order-8 scheme's own default step is unstable there)
    _spread_x0(p)
    if "unc" in kinds:
        u = _unc_over(p["model"], Q11_PICK if "q11" in kinds else None)
        u["uncertainty_percentages"].update(p["uncertainty_percentages"])
        p.update(u)
    if rows is not None:
        p.update(constraints={"A": np.asarray(rows[0], dtype=float), "b": np.asarray(rows[1], dtype=float)}, done_on_cons_vio=False,
                 r_penalty=True)
    return p


def _perm_hidden(pol, seed):
    """the same function with the hidden units in another order (another summation order in every layer after the first)"""
    from pcgym_amd import MLPPolicy

    rng = np.random.default_rng(seed)
    Ws, bs = [w.copy() for w in pol.weights], [b.copy() for b in pol.biases]
    for l in range(pol.n_hidden):
        perm = rng.permutation(Ws[l].shape[0])
        Ws[l], bs[l] = Ws[l][perm], bs[l][perm]
        Ws[l + 1] = Ws[l + 1][:, perm]
    return MLPPolicy(Ws, bs, activation=pol.activation, out_map=pol.out_map, out_low=pol.out_low, out_high=pol.out_high)


# plans neither closed-loop entry point takes: name -> (scenario, env_params changes)
UNSUPPORTED_PLANS = {
    "constraints": ("cstr_cons_pen_norm", dict(integrator="rk4")),
    "per_env_parameters": ("cstr_canonical", dict(integrator="rk4", uncertainty_percentages={"q": 0.03}, distribution="uniform",
                                                  uncertainty_bounds={"low": np.array([90.0]), "high": np.array([110.0])})),
    "rodas5": ("me_canonical", dict(integrator="rodas5")),
}


# ---- shared by the closed-loop tests on constrained plans and on plans with per-env parameters ------------------------------------
def _stepped(env, a_seq, T, record_x=True):
    """the per-step route under the callable policy that replays `a_seq`: dict of stacked per-step results"""
    torch = _torch()
    out = {k: [] for k in ("obs", "rew", "g", "viol", "done", "x0")}
    for s in range(T):
        if record_x:
            out["x0"].append(env.x.clone())
        env.step(a_seq[s])
        out["obs"].append(env.obs_soa.clone()), out["rew"].append(env.rew.clone()), out["g"].append(env.g.clone())
        out["viol"].append(env.viol.clone()), out["done"].append(env.done.clone())
        if s == 0 and env.t == 1:
            out["g_pre"] = env.g_pre.clone()
    return {k: (torch.stack(v) if isinstance(v, list) and v else v) for k, v in out.items()}


def _check_final(ef, es):
    torch = _torch()
    for n in ("x", "obs_soa", "rew", "done", "viol", "g", "g_pre"):
        assert torch.equal(getattr(ef, n), getattr(es, n)), f"io->{n} after the call is not what the step loop leaves"
    if ef.spec.a_delta:
        assert torch.equal(ef.a_save_t, es.a_save_t)
    if ef.u_prev is not None:
        assert torch.equal(ef.u_prev, es.u_prev)
    assert ef.t == es.t


def _tols(key):
    hat = "^" in key
    return dict(x1=5e-6 if hat else 1e-8, o_rtol=1e-5 if hat else 1e-8, o_atol=1e-5 if hat else 1e-9, xT=2e-5 if hat else 1e-7)


def _rew_close(r, ref):
    return np.allclose(r, ref, rtol=1e-9, atol=1e-10 * (1 + np.max(np.abs(ref))))


def _final_equal(ea, eb):
    torch = _torch()
    for n in ("x", "obs_soa", "rew", "done", "p_unc"):
        assert torch.equal(getattr(ea, n), getattr(eb, n)), f"io->{n} after the chunks is not what the single call leaves"
    if ea.spec.a_delta:
        assert torch.equal(ea.a_save_t, eb.a_save_t)
    if ea.u_prev is not None:
        assert torch.equal(torch.nan_to_num(ea.u_prev, nan=-7.0), torch.nan_to_num(eb.u_prev, nan=-7.0))
    assert ea.t == eb.t
