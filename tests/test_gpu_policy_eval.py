"""GPU: the in-kernel MLP evaluator (policy_raw / policy_map, pcg_rollout_policy.hpp; its packed weights: pack_policy,
pcg_policy_pack.hpp) on the networks the closed-loop suites never feed it: ragged widths, ReLU, every output map, large arguments of
tanh, non-finite observations, an actor and a critic of different shapes.  Property checks only: no oracle, no golden file.

How the evaluator is driven (helpers.tanh_k's trick): chosen inputs are written into env.obs_soa, one closed-loop call with
T = 1 follows, row 0 of the recorded outputs is the evaluator's result on those inputs.  The env step after it is irrelevant
and nothing about the state is asserted.  B = 1000 (a tail wave), inputs uniform over the plan's observation box (the lanes of
a wave differ), one env per plan for the whole module.  One plan per evaluator template, all RK4: cstr, four_tank (na = 2),
the built-in model with the widest policy input (heat_exchanger: 24 states, one wave per SIMD) and the run-time compiled
size-limit user model (29 of 32 inputs, na = 5).

  1. sweep          15 hidden shapes (one unit; one below, at, one above the 8-block; one below the 4-block of the streamed
                    layer; both widths at 64) x {tanh, relu} x {clip, none, tanh} x 4 plans: every output inside
                    host_reference's running bound with k = tanh_k() + 1, the tolerance of the closed-loop suites.  Each case is
                    non-vacuous by the reference alone (_vacuity): every output component varies over the batch, every ReLU
                    layer of more than one unit has a unit that is on for some lanes and off for others and no layer is dead,
                    under clip >= 5 % of the outputs are cut on each side and >= 25 % lie strictly inside.  The clip box is the
                    20 % / 80 % quantile pair of the reference's unclipped outputs; the weights' seed of every case is in SEEDS
                    (found on the host: tools/policy_eval_seeds.py).
  2. zero-widening  every ragged shape widened by zero rows, zero biases and zero columns to the next multiple of 8 and to 64
                    gives BITWISE the same outputs; pcg_policy_update to other weights of a ragged shape gives bitwise a fresh
                    policy's outputs.
  3. large tanh     +-[18, 20] in 4097 points, +-{24, 25, 50, 354, 355, 356, 709, 710, 711, 1e4, 1e100, 1e300}, +-0 through the
                    hidden activation and through the output map: finite, at most 1 in magnitude, the sign of the argument,
                    within tanh_k's 16-ulp ceiling of np.tanh in np.longdouble.  (The sign of a ZERO result is held against the
                    reference network's: the output layer adds its +0 bias and +0 padding products, so tanh(-0) = -0 leaves the
                    network as +0 on the host and on the device alike.)
  4. non-finite     cstr, B = 1023, T = 3, a NaN and an Inf planted in the state (test_gpu_round2._plant_nonfinite) against an
                    unplanted twin, {policy, actor} x {tanh, relu}: exactly the two planted envs are flagged, every other lane
                    of everything recorded is bitwise the twin's; the NaN lane's later actions are clip(output bias) under ReLU
                    (pol_act: NaN -> 0) and NaN under tanh.
  5. actor / critic of different shapes and activations on four_tank, and on the size-limit model (the actor kernel's first
                    run there; na = 5 leaves the last pair of normal variates half used): test_actor_rollout's sample, value and
                    logp checks on rows 0 and 1, the noise from pcg_policy_noise.

Measured figures are printed and, when PCG_RECORD_DIR names a directory, appended to policy_eval_test.txt there (the copy
under profiles/r12/policy_eval_test.txt).
First run on an MI355X: output error at most 0.53 x its running bound on cstr (at the affine shape: the fewest terms, the
tightest bound), 0.35 on four_tank, 0.14 on heat_exchanger, 0.09 on the size-limit model; device tanh at the large arguments
0.500 ulp at both sites; actor sample / value error at most 0.07 / 0.04 x their bounds; the whole file in 12 s.
Two deliberately wrong builds (not committed) turn it red: pack_policy filling its padding with 0.5 instead of 0 fails 1, 2, 3
and 5 (37 of 50 tests); pol_act's ReLU replaced by the identity fails the ReLU cases of 1, 3 and 4.
"""
import copy
from fractions import Fraction

import numpy as np
import pytest

import scenarios as SC
from helpers import LD, MODEL_KEYS, PRE_MAX, U, _case_params, _make, _spread_x0, _torch, host_reference, make_policy, tanh_k
from helpers import _record as _record_to
from pcgym_amd.config import EnvSpec
from test_gpu_actor_rollout import action_box, logp_numpy
from test_gpu_closed_loop_jit import _size_limit_params
from test_gpu_round2 import _plant_nonfinite

pytestmark = pytest.mark.gpu

B = 1000
PLANS = ("cstr", "four_tank", "heat_exchanger", "size_limit")
ACTS = ("tanh", "relu")
OUT_MAPS = ("clip", "none", "tanh")
HIDDEN = [(), (1,), (7,), (8,), (9,), (63,), (64,),
          (1, 1), (9, 3), (8, 4), (16, 5), (63, 61), (64, 1), (5, 64), (64, 64)]
RAGGED = [s for s in HIDDEN if any(w % 8 for w in s)]  # a width that is no multiple of the hidden-side block
CLIP_Q = (0.2, 0.8)  # the clip box: these quantiles of the reference's unclipped outputs

# Seed of make_policy's weights per plan and activation, in the order of HIDDEN: the first of 17, 18, ... under which the case
# meets _vacuity's conditions with all three output maps (tools/policy_eval_seeds.py prints this table).
SEEDS = {
    "cstr": {"tanh": [17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17],
             "relu": [17, 51, 17, 17, 17, 17, 17, 163, 19, 17, 17, 17, 26, 17, 17]},
    "four_tank": {"tanh": [17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17],
                  "relu": [17, 19, 17, 17, 17, 17, 17, 18, 17, 17, 17, 17, 18, 17, 17]},
    "heat_exchanger": {"tanh": [17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17],
                       "relu": [17, 19, 17, 17, 17, 17, 17, 22, 17, 17, 17, 17, 18, 17, 17]},
    "size_limit": {"tanh": [17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17],
                   "relu": [17, 17, 17, 17, 17, 17, 17, 19, 17, 17, 17, 17, 19, 17, 17]},
}
# Seed 17, make_policy's usual one, fails under ReLU at the one-unit layers: (1,), (1, 1), (64, 1) give a constant output or a
# dead layer on most plans, cstr (9, 3) clips nothing from above.


def _record(line):
    _record_to("policy_eval_test.txt", line)


def _seed(plan, shape, act):
    return SEEDS[plan][act][HIDDEN.index(tuple(shape))]


# ---- host side: plans, inputs, networks, what makes a case worth running ---------------------------------------------------------
def _params(plan):
    return _size_limit_params("rk4") if plan == "size_limit" else _case_params(plan, "rk4")


_INPUTS = {}


def _inputs(plan):
    """(spec, inputs (nobs, B) float64 uniform over the plan's observation box) -- no GPU involved"""
    if plan not in _INPUTS:
        spec = EnvSpec(copy.deepcopy(_params(plan)))
        if spec.normalise_o:
            lo, hi = -np.ones(spec.nobs), np.ones(spec.nobs)
        else:
            lo, hi = np.asarray(spec.o_low, dtype=float), np.asarray(spec.o_high, dtype=float)
        rng = np.random.default_rng(1000 + PLANS.index(plan))
        _INPUTS[plan] = (spec, rng.uniform(lo[:, None], hi[:, None], (spec.nobs, B)))
    return _INPUTS[plan]


def _layers(pol, obs):
    """the reference's own pre-activations, layer by layer, in np.longdouble; the last entry is the output before its map"""
    h, out = obs.astype(LD), []
    for l, (W, b) in enumerate(zip(pol.weights, pol.biases)):
        h = W.astype(LD) @ h + b.astype(LD)[:, None]
        out.append(h)
        if l < pol.n_hidden:
            h = np.tanh(h) if pol.activation == "tanh" else np.maximum(h, 0)
    return out


_BOX = {}


def _network(plan, shape, act, out_map, seed=None):
    """the case's policy: make_policy's weights under the case's seed; under clip the box of CLIP_Q"""
    spec, obs = _inputs(plan)
    seed = _seed(plan, shape, act) if seed is None else seed
    lo = hi = None
    if out_map == "clip":
        key = (plan, tuple(shape), act, seed)
        if key not in _BOX:
            raw = make_policy(spec, obs, shape, seed, activation=act, out_map="none")
            v = _layers(raw, obs)[-1].astype(np.float64)
            _BOX[key] = (float(np.quantile(v, CLIP_Q[0])), float(np.quantile(v, CLIP_Q[1])))
        lo, hi = _BOX[key]
    return make_policy(spec, obs, shape, seed, activation=act, out_map=out_map, out_low=lo, out_high=hi)


def _vacuity(pol, obs, ref):
    """why this case would check less than it is meant to -- from the reference alone; empty when it is a fair case"""
    why = []
    if not np.all(np.ptp(ref.astype(np.float64), axis=1) > 0):
        why.append("an output component is constant over the batch")
    pre = _layers(pol, obs)
    if pol.activation == "relu":
        for l, h in enumerate(pre[:-1]):
            on = h > 0
            if not on.any():
                why.append(f"hidden layer {l} is dead over the whole batch")
            if h.shape[0] > 1 and not np.any(on.any(axis=1) & (~on).any(axis=1)):
                why.append(f"no unit of hidden layer {l} is active on some lanes and inactive on others")
    raw = pre[-1].astype(np.float64)
    if pol.out_map == "clip":
        below, above = float(np.mean(raw < pol.out_low)), float(np.mean(raw > pol.out_high))
        inside = float(np.mean((raw > pol.out_low) & (raw < pol.out_high)))
        if below < 0.05 or above < 0.05 or inside < 0.25:
            why.append(f"clip: {below:.3f} cut below, {above:.3f} cut above, {inside:.3f} strictly inside")
    if pol.out_map == "tanh" and np.max(np.abs(raw)) > PRE_MAX:
        why.append(f"arguments of the output tanh up to {np.max(np.abs(raw)):.1f}: outside the grid its error was measured on")
    return why


def _widen(pol, to):
    """the same function with every hidden layer widened to `to(width)` units by zero rows, zero biases and zero columns"""
    from pcgym_amd import MLPPolicy

    Ws, bs = [w.copy() for w in pol.weights], [b.copy() for b in pol.biases]
    for l in range(pol.n_hidden):
        w = Ws[l].shape[0]
        n = to(w)
        assert n >= w
        Ws[l] = np.vstack([Ws[l], np.zeros((n - w, Ws[l].shape[1]))])
        bs[l] = np.concatenate([bs[l], np.zeros(n - w)])
        Ws[l + 1] = np.hstack([Ws[l + 1], np.zeros((Ws[l + 1].shape[0], n - w))])
    return MLPPolicy(Ws, bs, activation=pol.activation, out_map=pol.out_map, out_low=pol.out_low, out_high=pol.out_high)


def _critic(spec, obs, shape, act, seed):
    """make_policy's network, first output row, no output map (test_gpu_actor_rollout.make_ac's critic)"""
    from pcgym_amd import MLPPolicy

    c = make_policy(spec, obs, shape, seed, activation=act, out_map="none")
    return MLPPolicy(c.weights[:-1] + [c.weights[-1][:1]], c.biases[:-1] + [c.biases[-1][:1]], activation=act, out_map="none")


# ---- device side ------------------------------------------------------------------------------------------------------------
_ENVS = {}


def _env(plan):
    """(env of B lanes after its reset, the plan's inputs on the device, the reset state): created once per module"""
    if plan not in _ENVS:
        torch = _torch()
        spec, obs = _inputs(plan)
        env = _make(_params(plan), B, seed=3)
        assert (env.spec.nobs, env.spec.na, env.spec.integrator) == (spec.nobs, spec.na, "rk4")
        if plan == "size_limit":
            env.prepare_closed_loop()
        env.reset()
        torch.cuda.synchronize()
        _ENVS[plan] = (env, torch.as_tensor(obs, device=env.device), env.x.clone())
    return _ENVS[plan]


def _rewind(plan):
    """the plan's env at step 0 with the reset state and the plan's inputs as its observation"""
    env, obs_t, x0 = _env(plan)
    env.x.copy_(x0), env.obs_soa.copy_(obs_t), env.status.zero_()
    env.t = 0
    return env


def _evaluate(plan, pol):
    """policy(inputs) through rollout_policy_kernel: (na, B) device tensor"""
    torch = _torch()
    env = _rewind(plan)
    a_seq, _, _ = env.rollout_policy(pol, 1, collect_rew=False)
    torch.cuda.synchronize()
    assert a_seq.shape == (1, env.spec.na, B)
    return a_seq[0].clone()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def test_the_four_plans_are_the_four_evaluator_templates():
    """cstr and four_tank (8 inputs, one and two outputs), the widest built-in policy input, the run-time compiled model"""
    from pcgym_amd import _abi as abi
    from pcgym_amd.models import get_model

    def n_in(key):  # policy_nin<M>(), pcg_rollout_policy.hpp
        m = get_model(key.partition("^")[0])
        return (len(m.states) + abi.PCG_MAX_NSP + len(m.disturbances) + 3) // 4 * 4

    widest = max(MODEL_KEYS, key=n_in)
    assert widest == PLANS[2] and len(get_model(widest).states) > 10 and [k for k in MODEL_KEYS if n_in(k) == n_in(widest)] == [widest]
    shapes = {plan: (_inputs(plan)[0].nobs, _inputs(plan)[0].na) for plan in PLANS}
    assert shapes["four_tank"][1] == 2 and shapes["size_limit"] == (29, 5) and shapes["cstr"][1] == 1
    for plan in PLANS:
        env, obs_t, _ = _env(plan)
        assert env.B == B and B % 64 and tuple(obs_t.shape) == (shapes[plan][0], B)
        assert float(obs_t.std(dim=1).min()) > 0
    assert _env("size_limit")[0].spec.model.model_id == 17


# ---- 1. the sweep -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_map", OUT_MAPS)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("plan", PLANS)
def test_evaluator_sweep(plan, act, out_map):
    """every hidden shape of HIDDEN on one plan, activation and output map"""
    spec, obs = _inputs(plan)
    k = tanh_k()
    worst, worst_shape, pre_max = 0.0, None, 0.0
    for shape in HIDDEN:
        tag = f"{plan}-{'x'.join(map(str, shape)) or 'affine'}-{act}-{out_map}"
        pol = _network(plan, shape, act, out_map)
        assert pol.validate() == 0 and pol.n_hidden == len(shape) and (pol.activation, pol.out_map) == (act, out_map)
        ref, bound, pre = host_reference(pol, obs, k + 1.0)
        why = _vacuity(pol, obs, ref)
        assert not why, f"{tag} (seed {_seed(plan, shape, act)}): {why}"
        if act == "tanh":
            pre_max = max(pre_max, pre)
            assert pre <= PRE_MAX, f"{tag}: pre-activations up to {pre:.1f}: outside the grid the tanh error was measured on"
        got = _evaluate(plan, pol).cpu().numpy()
        pol.close()
        assert got.shape == (spec.na, B) and np.isfinite(got).all(), tag
        diff = np.abs(got.astype(LD) - ref).astype(np.float64)
        frac = float(np.max(diff / np.maximum(bound, 1e-300)))
        print(f"{tag}: output error {np.max(diff):.3e}, {frac:.3f} x the running bound ({np.max(bound):.3e})")
        assert np.all(diff <= bound), f"{tag}: policy output off by {np.max(diff):.3e}, {frac:.2f} x the running bound ({np.max(bound):.3e})"
        if frac > worst:
            worst, worst_shape = frac, shape
    _record(f"sweep {plan}-{act}-{out_map}: output error <= {worst:.3f} x bound (at {worst_shape}) over {len(HIDDEN)} shapes x {B} lanes"
            + (f", |pre-activation| <= {pre_max:.2f}" if act == "tanh" else "") + f", seeds {SEEDS[plan][act]}")


# ---- 2. zero-widening and the update of a ragged shape ----------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("plan", PLANS)
def test_zero_widening_is_bitwise(plan, act):
    """zero rows, zero biases and zero columns add fma(0, h, acc) = acc and act(0) = 0 to every sum: not one bit may change.
    A kernel that reads past a layer's width, or a pack_policy that pads wrongly, does change some."""
    torch = _torch()
    for shape in RAGGED:
        pol = _network(plan, shape, act, "none")
        to8, to64 = _widen(pol, lambda w: (w + 7) // 8 * 8), _widen(pol, lambda w: 64)
        widths = [[w.shape[0] for w in q.weights[:-1]] for q in (pol, to8, to64)]
        assert widths[0] == list(shape) and widths[1] != widths[0] and all(w % 8 == 0 for w in widths[1]) and set(widths[2]) == {64}
        got, got8, got64 = (_evaluate(plan, q) for q in (pol, to8, to64))
        assert bool(torch.isfinite(got).all()) and float(got.std()) > 0, (plan, shape, act)
        for wide, ws in ((got8, widths[1]), (got64, widths[2])):
            assert torch.equal(wide, got), f"{plan} {shape} {act}: widened to {ws} the outputs differ, by up to {float((wide - got).abs().max()):.3e}"
        for q in (pol, to8, to64):
            q.close()


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("plan", PLANS)
def test_update_of_a_ragged_policy_equals_a_fresh_one_bitwise(plan, act):
    """pcg_policy_update rewrites the device block of a ragged shape, padding included"""
    torch = _torch()
    obs = _inputs(plan)[1]
    for shape in RAGGED:
        pol = _network(plan, shape, act, "none")
        for seed in range(_seed(plan, shape, act) + 1, 1000):  # the next seed that makes a fair case, too
            fresh = _network(plan, shape, act, "none", seed=seed)
            if not _vacuity(fresh, obs, _layers(fresh, obs)[-1]):
                break
        before = _evaluate(plan, pol)
        handle = pol.handle(_env(plan)[0].device).value
        pol.update_(fresh.weights, fresh.biases)
        assert pol.handle(_env(plan)[0].device).value == handle, "update_ made a new device object"
        got, want = _evaluate(plan, pol), _evaluate(plan, fresh)
        assert bool(torch.isfinite(want).all()) and float(want.std()) > 0
        assert torch.equal(got, want), f"{plan} {shape} {act}: the updated policy is not the fresh one"
        assert not torch.equal(got, before), f"{plan} {shape} {act}: the update changed nothing"
        pol.close(), fresh.close()


# ---- 3. large arguments of tanh ---------------------------------------------------------------------------------------------
def _tanh_grid():
    pos = np.concatenate([np.linspace(18.0, 20.0, 4097), [24, 25, 50, 354, 355, 356, 709, 710, 711, 1e4, 1e100, 1e300], [0.0]])
    return np.concatenate([pos, -pos])  # (-0.0 is its last entry)


@pytest.mark.parametrize("site", ["hidden", "output_map"])
def test_tanh_of_large_arguments(site):
    """helpers.tanh_k's one-unit network: hidden = tanh(first observation) -> output = 1 x hidden;  output_map = a ReLU unit of
    weight 1 on the first observation, output weight +1 and then -1 (both signs reach the map), out_map tanh."""
    torch = _torch()
    from pcgym_amd import MLPPolicy

    grid = _tanh_grid()
    assert np.signbit(grid[-1]) and grid[-1] == 0 and grid.size == 2 * (4097 + 13)
    p = copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"])
    p.update(integrator="rk4")
    env = _make(p, grid.size, seed=1)
    env.reset()
    W0 = np.zeros((1, env.spec.nobs))
    W0[0, 0] = 1.0
    runs = []  # (argument of the tanh as the device forms it, what the network returns for tanh(argument) = t)
    if site == "hidden":
        runs.append((MLPPolicy([W0, np.ones((1, 1))], [np.zeros(1), np.zeros(1)], activation="tanh", out_map="none"), grid))
    else:
        relu = np.where(grid > 0, grid, 0.0)  # pol_act
        for w in (1.0, -1.0):
            runs.append((MLPPolicy([W0, np.full((1, 1), w)], [np.zeros(1), np.zeros(1)], activation="relu", out_map="tanh"), w * relu + 0.0))
    worst, seen = 0.0, []
    for pol, arg in runs:
        env.obs_soa.zero_()
        env.obs_soa[0] = torch.as_tensor(grid, device=env.device)
        env.t = 0
        a_seq, _, _ = env.rollout_policy(pol, 1, collect_rew=False)
        torch.cuda.synchronize()
        got = a_seq[0, 0].cpu().numpy()
        pol.close()
        want = np.tanh(arg.astype(LD))
        if site == "hidden":
            want = LD(1) * want + LD(0)  # the output layer: -0 + 0 = +0
        assert np.isfinite(got).all(), f"not finite at {arg[~np.isfinite(got)][:8]}"
        assert np.all(np.abs(got) <= 1.0), f"|tanh| > 1 at {arg[np.abs(got) > 1.0][:8]}"
        nz = arg != 0
        assert np.array_equal(np.sign(got[nz]), np.sign(arg[nz])), "a result has lost the sign of its argument"
        assert np.array_equal(np.signbit(got), np.signbit(want.astype(np.float64))), "sign of a zero result"
        assert np.all(got[~nz] == 0)
        ulp = np.spacing(np.abs(want.astype(np.float64)))
        err = np.abs(got.astype(LD) - want).astype(np.float64) / ulp
        worst = max(worst, float(np.max(err)))
        seen.append(arg)
    env.close()
    seen = np.concatenate(seen)
    for v in (18.0, 20.0, 355.0, 710.0, 1e300):  # both signs of every part of the grid reached the tanh
        assert (seen == v).any() and (seen == -v).any(), v
    _record(f"device tanh as {site}: max error {worst:.3f} ulp over +-[18, 20] (4097 points), +-(24 ... 711, 1e4, 1e100, 1e300), 0")
    assert np.isfinite(worst) and worst <= 16.0, f"device tanh is {worst} ulp off at large arguments: not a libm-class tanh"


# ---- 4. non-finite states in closed loop ------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("head", ["policy", "actor"])
def test_nonfinite_state_in_closed_loop(head, act):
    torch = _torch()
    from pcgym_amd import GaussianActorCritic
    from pcgym_amd import _abi as abi

    Bn, T, NAN, INF = 1023, 3, 5, 1022
    p = copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"])
    p.update(integrator="rk4")
    p = _spread_x0(p)
    env, twin = _make(p, Bn, seed=1), _make(p, Bn, seed=1)
    spec = env.spec
    _plant_nonfinite(env, Bn)
    twin.reset()
    assert torch.equal(env.obs_soa, twin.obs_soa) and not torch.equal(env.x, twin.x)
    obs0 = twin.obs_soa.cpu().numpy().copy()
    pol = make_policy(spec, obs0, (9,), 17, activation=act)
    lo, hi = pol.out_low, pol.out_high
    if head == "policy":
        net = pol

        def run(e):
            a, o, r = e.rollout_policy(pol, T, collect_obs=True, collect_rew=True)
            return {"a": a, "obs": o, "rew": r}
    else:
        a_lo, a_hi = action_box(spec)
        net = GaussianActorCritic(pol, np.log(0.25 * np.maximum((a_hi - a_lo) / 2, 1e-3)), _critic(spec, obs0, (9,), act, 117))

        def run(e):
            return e.rollout_actor(net, T, collect_obs=True, collect_rew=True)
    got, ref = run(env), run(twin)
    torch.cuda.synchronize()

    st = env.status.cpu().numpy()
    assert st[NAN] == abi.PCG_ST_NONFINITE and st[INF] == abi.PCG_ST_NONFINITE and st.sum() == 2 * abi.PCG_ST_NONFINITE
    assert not twin.status.any() and all(bool(torch.isfinite(v).all()) for v in ref.values())
    assert float(ref["a"].std()) > 0
    keep = torch.ones(Bn, dtype=torch.bool, device=env.device)
    keep[[NAN, INF]] = False
    for n in ref:
        assert got[n].shape == ref[n].shape and torch.equal(got[n][..., keep], ref[n][..., keep]), f"{n}: a healthy lane differs from the twin"
    for n in ("x", "obs_soa", "rew"):
        assert torch.equal(getattr(env, n)[..., keep], getattr(twin, n)[..., keep]), f"final {n}: a healthy lane differs from the twin"
    # the NaN lane: its first observation was still the reset's, from the second on it is NaN
    lane = {n: v[..., NAN].cpu().numpy() for n, v in got.items()}
    assert np.array_equal(_bits(lane["a"][0]), _bits(ref["a"][0][..., NAN].cpu().numpy()))
    assert np.isnan(lane["obs"]).any(axis=1).all()
    if act == "tanh":  # a NaN stays a NaN
        for n in [n for n in ("a", "u", "val") if n in lane]:
            assert np.isnan(lane[n][1:]).all(), n
    else:  # every hidden unit is relu(NaN) = 0: the output is its bias
        b_out = pol.biases[-1]
        if head == "policy":
            for s in (1, 2):
                assert np.array_equal(_bits(lane["a"][s]), _bits(np.clip(b_out, lo, hi))), f"row {s}: not the clip of the output bias"
        else:
            for s in (1, 2):
                z = env.policy_noise(s)[:, NAN].cpu().numpy()
                u = np.array([float(Fraction(float(sg)) * Fraction(float(zi)) + Fraction(float(b)))  # fma(sigma, z, bias), one rounding
                              for sg, zi, b in zip(net.sigma, z, b_out)])
                assert np.array_equal(_bits(lane["u"][s]), _bits(u)), f"row {s}: u - sigma z is not the output bias"
                assert np.array_equal(_bits(lane["a"][s]), _bits(np.clip(u, lo, hi)))
                assert np.array_equal(_bits(lane["val"][s]), _bits(net.critic.biases[-1][0]))
                assert np.array_equal(_bits(lane["logp"][s]), _bits(logp_numpy(net, z[:, None])[0]))
    env.close(), twin.close(), net.close()


# ---- 5. actor and critic of different shape ---------------------------------------------------------------------------------
ACTOR_CASES = {
    "four_tank_9x3relu_64tanh": ("four_tank", (9, 3), "relu", (64,), "tanh"),
    "four_tank_64tanh_9x3relu": ("four_tank", (64,), "tanh", (9, 3), "relu"),
    "size_limit_16x5tanh_7relu": ("size_limit", (16, 5), "tanh", (7,), "relu"),
}


@pytest.mark.parametrize("case", list(ACTOR_CASES))
def test_actor_and_critic_of_different_shape(case):
    """rollout_actor_kernel evaluates two networks one after the other in the same registers: two shapes, two activations.
    T = 1 with row T recorded: row 0 on the plan's inputs, row 1 on the kernel's own recorded observation."""
    torch = _torch()
    from pcgym_amd import GaussianActorCritic, MLPPolicy

    plan, a_shape, a_act, c_shape, c_act = ACTOR_CASES[case]
    spec, obs = _inputs(plan)
    k = tanh_k()
    env = _rewind(plan)
    z = np.stack([env.policy_noise(t).cpu().numpy() for t in (0, 1)])  # the draws of counters 0 and 1
    assert z.shape == (2, spec.na, B) and np.std(z, axis=2).min() > 0.5
    a_lo, a_hi = action_box(spec)
    sigma = 0.25 * np.maximum((a_hi - a_lo) / 2, 1e-3)
    raw = _network(plan, a_shape, a_act, "none")
    mu0 = _layers(raw, obs)[-1]
    u0 = (mu0 + sigma[:, None].astype(LD) * z[0].astype(LD)).astype(np.float64)
    lo, hi = float(np.quantile(u0, CLIP_Q[0])), float(np.quantile(u0, CLIP_Q[1]))
    actor = make_policy(spec, obs, a_shape, _seed(plan, a_shape, a_act), activation=a_act, out_map="clip", out_low=lo, out_high=hi)
    assert all(np.array_equal(w, v) for w, v in zip(actor.weights + actor.biases, raw.weights + raw.biases))
    critic = _critic(spec, obs, c_shape, c_act, _seed(plan, c_shape, c_act))
    for net in (raw, critic):
        why = _vacuity(net, obs, host_reference(net, obs, 0.0)[0])
        assert not why, (case, why)
    ac = GaussianActorCritic(actor, np.log(sigma), critic)
    sig = ac.sigma[:, None]

    out = env.rollout_actor(ac, 1, collect_obs=True, record_next_action=True)
    torch.cuda.synchronize()
    a_np, u_np, lp_np, v_np, o_np = (out[n].cpu().numpy() for n in ("a", "u", "logp", "val", "obs"))
    assert a_np.shape == u_np.shape == (2, spec.na, B) and lp_np.shape == v_np.shape == (2, B) and o_np.shape == (1, spec.nobs, B)
    for arr in (a_np, u_np, lp_np, v_np, o_np):
        assert np.isfinite(arr).all()
    worst_u = worst_v = 0.0
    for s, o_in in enumerate((obs, o_np[0])):
        mu, b_mu, pm = host_reference(raw, o_in, k + 1.0)
        assert a_act != "tanh" or pm <= PRE_MAX
        want = mu + sig.astype(LD) * z[s].astype(LD)  # u = fma(sigma, z, mu): one more rounding
        diff = np.abs(u_np[s].astype(LD) - want).astype(np.float64)
        bound = b_mu + U * np.abs(u_np[s])
        assert np.all(diff <= bound), f"row {s}: sample off by {np.max(diff):.3e}, {np.max(diff / np.maximum(bound, 1e-300)):.2f} x its bound"
        worst_u = max(worst_u, float(np.max(diff / np.maximum(bound, 1e-300))))
        assert np.array_equal(lp_np[s], logp_numpy(ac, z[s])), f"row {s}: logp is not fma(-0.5, q, c0) of the same draws"
        vr, b_v, pm = host_reference(critic, o_in, k + 1.0)
        assert c_act != "tanh" or pm <= PRE_MAX
        dv = np.abs(v_np[s].astype(LD) - vr[0]).astype(np.float64)
        assert np.all(dv <= b_v[0]), f"row {s}: value off by {np.max(dv):.3e}, {np.max(dv / np.maximum(b_v[0], 1e-300)):.2f} x its bound"
        worst_v = max(worst_v, float(np.max(dv / np.maximum(b_v[0], 1e-300))))
    assert np.array_equal(a_np, np.clip(u_np, lo, hi)), "a is not clip(u) bitwise"
    assert np.any(u_np[0] < lo) and np.any(u_np[0] > hi) and np.mean((u_np[0] > lo) & (u_np[0] < hi)) >= 0.25
    assert np.std(u_np[0], axis=1).min() > 0 and np.std(v_np[0]) > 0
    _record(f"actor {case}: sample error <= {worst_u:.3f} x bound, value error <= {worst_v:.3f} x bound (rows 0 and 1, {B} lanes)")
    ac.close(), raw.close()

    if plan == "size_limit":  # all five components of the noise, the half-used third pair included
        zero = MLPPolicy([np.zeros((spec.na, spec.nobs))], [np.zeros(spec.na)], out_map="clip", out_low=-0.25, out_high=0.25)
        ac0 = GaussianActorCritic(zero, np.zeros(spec.na))
        assert spec.na == 5 and np.array_equal(ac0.sigma, np.ones(5))
        env = _rewind(plan)
        out = env.rollout_actor(ac0, 1, record_next_action=True)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out["u"].cpu().numpy()), _bits(z)), "the actor kernel's draws are not pcg_policy_noise's"
        assert np.array_equal(out["a"].cpu().numpy(), np.clip(z, -0.25, 0.25))
        assert len(np.unique(z)) > 0.9 * z.size
        ac0.close()
