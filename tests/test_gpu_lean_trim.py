"""The lean step with its wave-uniform work taken off the vector unit (env_step_lean, pcg_lean.hpp): the set-point's state
row chosen by a scalar branch, the action box's half width folded on the host (DevConst::a_w, amap_fold), the chained
kernel mapping its actions where their rows land.  None of it may change a bit.

GPU half: every comparison is bitwise (the bit patterns, so that equal NaNs are equal) against a twin VecEnv on the classic
kernel (variant=1), stepped eagerly with the same actions.  Three routes take the lean step: the eager pipelined step, a
chained replay of 6 steps with the outputs poisoned before each of two replays, and pcg_rollout of 6 steps.  B = 510 is a
partial tile, 514 two tiles of two envs per lane, 511 odd: one env per lane.

CPU half: the folding identity and the rule that refuses it, in numpy, which does not contract a product and a sum."""
import copy

import numpy as np
import pytest

import scenarios as SC

DBL_MIN = float(np.finfo(np.float64).tiny)  # the smallest normal double, 2^-1022
FOLD_MIN_W = 2.0 ** -969                    # amap_fold: |w| below it (and not zero) keeps action_map()
T = 6


# ---- CPU half --------------------------------------------------------------------------------------------------------
def _map(a, lo, hi):
    """action_map(), pcgym.py:372: (a + 1) (high - low) / 2 + low, left to right"""
    return ((a + 1.0) * (hi - lo)) * 0.5 + lo


def _map_folded(a, lo, hi):
    return (a + 1.0) * ((hi - lo) * 0.5) + lo


def _fold_ok(lo, hi):
    """amap_fold (pcg_kernels.hpp)"""
    with np.errstate(all="ignore"):
        d = np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64)
        return (np.abs(d) < np.inf) & ((d == 0.0) | (np.abs(d * 0.5) >= FOLD_MIN_W))


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.int64)


# the edge boxes of the GPU half: (lo, hi, folded?)
EDGE_BOXES = [
    (295.0, 302.0, True),              # cstr canonical
    (-302.0, -295.0, True),            # negative bounds
    (-1.0, 1.0, True),
    (3.0, 3.0, True),                  # no width: w = 0
    (0.0, 1.5 * DBL_MIN, False),       # w = 0.75 x the smallest normal: subnormal
    (0.0, 1.2345678901234567 * DBL_MIN, False),  # ... and with every bit of the width in use: w loses the last one
    (0.0, float("inf"), False),        # hi - lo = inf
    (float("-inf"), float("inf"), False),
    (0.0, float("nan"), False),
    (-1.7e308, 1.7e308, False),        # hi - lo overflows
    (0.0, 2.0 ** -968, True),          # the smallest width the rule folds ...
    (0.0, 2.0 ** -968 * (1 - 2.0 ** -53), False),  # ... and the double below it
]


def test_fold_rule_on_the_edge_boxes():
    for lo, hi, want in EDGE_BOXES:
        assert bool(_fold_ok(lo, hi)) == want, (lo, hi)


def test_folded_map_is_the_map_bit_for_bit():
    """10^6 random (a, lo, hi) the rule accepts -- boxes of every magnitude and sign, actions inside [-1, 1], just outside it
    and far outside it -- and the accepted edge boxes with actions that make a + 1 as small as it gets (2^-53)"""
    rng = np.random.default_rng(23)
    n = 10 ** 6
    mag = 10.0 ** rng.uniform(-12, 12, (2, n))
    lo = mag[0] * rng.choice([-1.0, 1.0], n)
    hi = np.where(rng.random(n) < 0.8, lo + mag[1], mag[1] * rng.choice([-1.0, 1.0], n))  # (a box may be upside down)
    a = np.where(rng.random(n) < 0.7, rng.uniform(-1, 1, n), rng.normal(0, 10.0, n) * 10.0 ** rng.integers(0, 6, n))
    ok = _fold_ok(lo, hi)
    assert ok.all()
    assert np.array_equal(_bits(_map(a, lo, hi)), _bits(_map_folded(a, lo, hi)))
    near = np.concatenate([-1.0 + 2.0 ** -53 * np.arange(0, 4096), rng.uniform(-1, 1, 4096), [1.0, -1.0, 0.0, np.inf, -np.inf, np.nan]])
    with np.errstate(all="ignore"):
        for lo, hi, folded in EDGE_BOXES:
            if folded:
                assert np.array_equal(_bits(_map(near, lo, hi)), _bits(_map_folded(near, lo, hi))), (lo, hi)
        # widths down to the rule's threshold, every bit of them in use
        wide = 2.0 ** rng.integers(-968, -900, 4096).astype(np.float64) * (1.0 + rng.random(4096))
        for lo in (0.0, -(2.0 ** -960)):
            assert _fold_ok(lo, lo + wide).all()
            for av in (near[:4096], near[4096:8192]):
                assert np.array_equal(_bits(_map(av, lo, lo + wide)), _bits(_map_folded(av, lo, lo + wide))), lo


def test_the_rule_refuses_what_does_not_fold():
    """Where w is subnormal it has lost the width's last bit and the two forms differ; they still differ where w is normal
    but (a + 1) w is not, the product being rounded once in one form and twice in the other.  That is why the threshold
    sits 53 binades above the smallest normal.  (Widths with every bit in use: a + 1 is a multiple of 2^-53, and its
    product with a width of two significant bits, such as 1.5 x the smallest normal, is exact in both forms.)"""
    rng = np.random.default_rng(24)
    n = 10 ** 5
    a = rng.uniform(-1, 1, n)
    lo = 0.0
    for scale in (1.0, 4.0):  # w in [1/2, 1) x and in [2, 4) x the smallest normal
        hi = DBL_MIN * scale * (1.0 + rng.random(n))
        assert not _fold_ok(lo, hi).any()
        assert ((hi * 0.5 >= DBL_MIN) == (scale > 1.0)).all()
        assert np.count_nonzero(_bits(_map(a, lo, hi)) != _bits(_map_folded(a, lo, hi))) > 1000, scale


# ---- GPU half --------------------------------------------------------------------------------------------------------
def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU test selected but no GPU visible"
    return torch


def _cstr(**over):
    p = copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"])
    p["integrator"] = "rk4"
    p.update(over)
    return p


def _thirds(N, a, b, c):
    return np.repeat([a, b, c], [N // 3, N // 3, N - 2 * (N // 3)]).astype(np.float64)


def _cstr_sp_T(**over):
    """the set-point on state 1"""
    N = 60
    return _cstr(SP={"T": _thirds(N, 325.0, 331.0, 328.0)}, r_scale={"T": 1e-2},
                 o_space={"low": np.array([0.7, 300, 300]), "high": np.array([1, 350, 350])}, x0=np.array([0.8, 330, 325.0]), **over)


def _cstr_sp_both(**over):
    N = 60
    return _cstr(SP={"Ca": _thirds(N, 0.85, 0.9, 0.87), "T": _thirds(N, 325.0, 331.0, 328.0)}, r_scale={"Ca": 1e3, "T": 1e-2},
                 o_space={"low": np.array([0.7, 300, 0.8, 300]), "high": np.array([1, 350, 0.9, 350])},
                 x0=np.array([0.8, 330, 0.85, 325.0]), **over)


def _four_tank():
    p = copy.deepcopy(SC.scenarios()["four_tank_canonical"]["env_params"])
    p["integrator"] = "rk4"
    return p


def _box(lo, hi, **over):
    """cstr with its coolant temperature mapped into [lo, hi]; a short tsim keeps the state finite next to a 0 K coolant"""
    return _cstr(a_space={"low": np.array([lo]), "high": np.array([hi])}, tsim=0.6, **over)


# (parameters, first recorded step): t0 = 17 runs across the set-point change at t = 20, t0 = 53 ends on the episode's last
# step (N = 60: done is set by step 58)
CASES = {
    "cstr_sp_state0": (_cstr, 17),
    "cstr_sp_state1": (_cstr_sp_T, 17),
    "cstr_sp_both": (_cstr_sp_both, 17),
    "four_tank_rk4": (_four_tank, 27),
    "normalise_a_off": (lambda: _cstr(normalise_a=False), 17),
    "negative_box": (lambda: _box(-302.0, -295.0), 17),
    "subnormal_half_width": (lambda: _box(0.0, 1.5 * DBL_MIN), 17),
    "subnormal_half_width_all_bits": (lambda: _box(0.0, 1.2345678901234567 * DBL_MIN), 17),
    "infinite_width": (lambda: _box(0.0, float("inf")), 17),
    "done_in_last_step": (_cstr, 53),
}
BATCHES = [510, 514, 511]


def _actions(spec, n, B, seed):
    rng = np.random.default_rng(seed)
    if spec.normalise_a:
        lo = -0.5 if spec.model.name == "four_tank" else -1.0  # (no tank drains)
        return rng.uniform(lo, 1.0, (n, spec.na, B))
    return rng.uniform(spec.a_low[None, :, None], spec.a_high[None, :, None], (n, spec.na, B))


def _same(torch, a, b, what):
    if a.dtype.is_floating_point:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    assert torch.equal(a, b), what


def _same_env(torch, ref, env, what):
    assert ref.t == env.t, what
    for k in ("x", "obs_soa", "rew", "done", "status"):
        _same(torch, getattr(ref, k), getattr(env, k), (what, k))


def _poison(env):
    env.obs_soa.fill_(float("nan"))
    env.rew.fill_(float("nan"))
    env.done.fill_(0xFF)


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", list(CASES))
def test_lean_routes_match_the_classic_kernel(case, B):
    torch = _torch()
    from pcgym_amd import VecEnv

    make, t0 = CASES[case]
    p = make()
    ref = VecEnv(copy.deepcopy(p), n_envs=B, seed=3, variant=1)
    envs = {r: VecEnv(copy.deepcopy(p), n_envs=B, seed=3) for r in ("eager", "chain", "rollout")}
    g = None
    try:
        s = ref.spec
        assert s.integrator == "rk4"
        if case == "done_in_last_step":
            assert t0 + T == s.N - 1
        acts = torch.tensor(_actions(s, t0 + T, B, 5), device=ref.device)
        # the classic twin: its outputs after every one of the T steps
        ref.reset()
        for i in range(t0):
            ref.step(acts[i])
        want = []
        for j in range(T):
            ref.step(acts[t0 + j])
            want.append((ref.obs_soa.clone(), ref.rew.clone(), ref.done.clone()))
        torch.cuda.synchronize()
        if case == "done_in_last_step":
            assert bool(ref.done.all()) and not bool(want[-2][2].any())
        if case in ("cstr_sp_state0", "cstr_sp_state1", "cstr_sp_both", "four_tank_rk4", "negative_box"):
            assert bool(torch.isfinite(ref.x).all()) and bool((ref.rew < 0).all()), case  # (a comparison of numbers, not of NaNs)

        def bring(env):
            env.reset()
            for i in range(t0):
                env.step(acts[i])

        # the eager pipelined step, held against the twin after every step
        env = envs["eager"]
        bring(env)
        for j in range(T):
            env.step(acts[t0 + j])
            for k, w in zip(("obs_soa", "rew", "done"), want[j]):
                _same(torch, w, getattr(env, k), (case, B, "eager", j, k))
        _same_env(torch, ref, env, (case, B, "eager"))

        # a chained replay, twice, the outputs poisoned before each
        env = envs["chain"]
        rec = [acts[t0 + j] for j in range(T)]
        for rep in range(2):
            bring(env)
            if g is None:
                g = env.capture_steps(rec)
                assert g.chained == (1, T)
            _poison(env)
            g.replay()
            torch.cuda.synchronize()
            _same_env(torch, ref, env, (case, B, "chain", rep))

        # the fused rollout: every step's observation and reward, then the buffers it leaves
        env = envs["rollout"]
        bring(env)
        _poison(env)
        obs_seq, rew_seq = env.rollout(acts[t0:t0 + T], collect_obs=True, collect_rew=True)
        torch.cuda.synchronize()
        for j in range(T):
            _same(torch, want[j][0], obs_seq[j], (case, B, "rollout", j, "obs"))
            _same(torch, want[j][1], rew_seq[j], (case, B, "rollout", j, "rew"))
        _same_env(torch, ref, env, (case, B, "rollout"))
    finally:
        if g is not None:
            g.destroy()
        ref.close()
        for e in envs.values():
            e.close()
