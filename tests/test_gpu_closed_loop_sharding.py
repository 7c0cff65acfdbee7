"""GPU: the fused closed-loop rollouts on shards of a batch whose global env indices lie past 2^32.

Every random number of the engine is keyed by the GLOBAL env index env_offset + e ("Sharded runs
(env_offset) reproduce the unsharded run bitwise").  The closed loop is restated once per kernel family, and each restatement
forms its own env_id; the per-step and open-loop kernels are held to the contract elsewhere, the closed-loop ones here: the ten
kernels -- base, float32, constrained, per-env-parameter and run-time compiled, each with a policy head and an actor head -- on
plans with something random INSIDE the loop (observation noise, a Gaussian disturbance), and one CV8 case for the second
scheme's instantiations.

Layout: G = 2^33 + 5 (the high Philox counter word is non-zero, the offset is odd), B = 264; `whole` is one env of 264 at
env_offset = G, the shards are 192 envs at G and 72 envs at G + 192 (both even: the rows stay 16-byte aligned and the
constrained rows keep the whole's summation order; the shards span other numbers of waves than the whole).  One seed, T = 5,
1 x 16 tanh networks (helpers.make_policy / test_gpu_actor_rollout.make_ac).  Per case:

  1. precondition  the shards' x, obs_soa (and p_unc) after reset are the whole's slices -- the reset, tested elsewhere, reported
                   as such;
  2. shards == whole, bitwise: every recorded sequence and every buffer the call leaves;
  3. actors: a second call with the all-zero actor and sigma = 1 records u[0..T] == the oracle's orc_rng_normal at the global
     index (test_gpu_actor_rollout.z_twin), bitwise, and logp == logp_numpy of it -- the independent reference that catches a
     truncated index, which shards and whole would share;
  4. the first step is the oracle's: OracleEnv at env_offset = G + lo from the shard's own start state and recorded a[0], under
     the family's existing tolerances (state 1e-12 of max(|x|, 1), observation rtol 1e-10 / atol 1e-11, helpers._rew_close; the
     per-env-parameter family helpers._tols; constrained rows test_closed_loop_feature_plans.G_TOL x the row scale, flags and
     rewards where every row is further than that from zero).  The noise is 2e-3 of the observation: a draw from another
     stream misses these bars by nine orders.  The run-time compiled family takes the step module's open-loop replay of the
     recorded actions, bitwise, instead (test_gpu_closed_loop_jit._replay's check);
  5. non-vacuity: the two shards' draws differ (actors: u; policies: the noise recovered from obs[0] and the oracle's noise-free
     step), the same env at env_offset = 0 records another obs[0] / u, and std(u) > 0.5 under the zero actor.

test_collect_onpolicy_on_shards: the public collector on shard.shard_range's layout, fused routes only.

Measured figures are printed and, when PCG_RECORD_DIR names a directory, appended to closed_loop_sharding_test.txt there.
First run on an MI355X, 19 cases in 5.3 s (1.8 s of it the chemostat's closed-loop module): first step against the oracle at
G + lo, worst per family -- base state 5.1e-16, obs 2.2e-4 x its tolerance, rew 6.3e-15 of 1 + max|r|; float32 4.4e-16, 2.1e-4 x,
9.1e-15; constrained 3.3e-16, 3.8e-6 x, 7.2e-15, rows 8.7e-5 x the row tolerance, no env excluded; per-env parameters 3.4e-16,
2.2e-6 x, 3.5e-15; the CV8 case 5.6e-17, 1.3e-5 x, 4.0e-16; the run-time compiled family's replay bitwise.

Three deliberately wrong builds of the cstr kernels, each run once through the seven existing closed-loop files
(test_gpu_policy_rollout, test_gpu_actor_rollout, test_gpu_policy_f32, test_gpu_cons_rollout, test_gpu_unc_rollout,
test_gpu_closed_loop_jit, test_gpu_closed_loop_features: 887 tests, which passed all three) and through this file:
  (a) env_id = (uint64_t)e in rollout_cons_actor_kernel (pcg_rollout_cons.hpp, the policy draw): [cons-...-actor] fails at 2
      (`a`: the shards' records are not the whole's);
  (b) env_id = (uint32_t)(A.env_offset + e) in rollout_actor_kernel_f32: both [f32-...-actor] cases fail, at 3 only (the
      kernel's draws are not the oracle's at the global index) -- shards and whole still agree, 1 and 2 pass;
  (c) the offset dropped from env_post_cons's env_id (the noise draw): [cons-...-policy] and [cons-...-actor] fail at 2.
"""
import time

import numpy as np
import pytest

from helpers import (EnvSpec, _case_params, _launch_names, _launched, _make, _rew_close, _spread_x0, _tols, _torch, feature_params, make_policy,
                     worst_rel)
from helpers import _record as _record_to
from test_closed_loop_feature_plans import G_TOL, case_params, row_scales, u_box
from test_gpu_actor_rollout import action_box, logp_numpy, make_ac, z_twin
from test_gpu_closed_loop_jit import _chemostat

pytestmark = pytest.mark.gpu

G = (1 << 33) + 5
B, T, SEED = 264, 5, 13
SHARDS = ((0, 192), (192, 264))
NOISE = dict(noise=True, noise_percentage=0.002)

# family -> the plans it runs (RK4)
PLANS = {"base": ("cstr_noise", "cstr_dist_Ti_gauss"), "f32": ("cstr_noise", "cstr_dist_Ti_gauss"), "cons": ("cstr_con_reward_noise",),
         "unc": ("unc_cstr_noise",), "jit": ("chemostat_noise",)}
CASES = [(f, pl, "rk4", h) for f, pls in PLANS.items() for pl in pls for h in ("policy", "actor")] + [("base", "four_tank_noise", "cv8", "actor")]
KERNEL = {"base": "rollout_{}_kernel", "f32": "rollout_{}_kernel_f32", "cons": "rollout_cons_{}_kernel", "unc": "rollout_unc_{}_kernel",
          "jit": "rollout_{}_kernel"}


def _record(line):
    _record_to("closed_loop_sharding_test.txt", line)


def _params(plan, integ, random=True):
    """env_params of `plan`, every env with its own initial state; random=False: the same plan without its draws inside the loop"""
    if plan == "cstr_noise":
        p = _spread_x0(_case_params("cstr_noise", integ))
    elif plan == "four_tank_noise":
        p = _case_params("four_tank", integ)
        p.update(NOISE)
        _spread_x0(p)
    elif plan == "chemostat_noise":
        p = _spread_x0(_chemostat(integ, **NOISE))
    elif plan == "cstr_dist_Ti_gauss":
        return feature_params(plan if random else "cstr_dist_Ti", integ)
    else:
        p = feature_params(plan, integ)
        p = case_params(plan, integ, _spec(p))  # (the constrained plan with its committed rows)
    if not random:
        p.update(noise=False)
    return p


def _spec(p):
    return EnvSpec(p)


def _env(p, lo, hi, offset=G):
    e = _make(p, hi - lo, seed=SEED, env_offset=offset + lo)
    e.reset()
    return e


def _call(env, family, head, net, n, nxt=True):
    """the family's fused call of `n` steps: dict of every recorded sequence (None where the head has none)"""
    kw = dict(collect_obs=True, collect_rew=True, record_next_action=nxt)
    if family in ("base", "f32", "jit"):
        if head == "actor":
            return env.rollout_actor(net, n, **kw)
        a, o, r = env.rollout_policy(net, n, **kw)
    elif family == "cons":
        return (env.rollout_policy_cons if head == "policy" else env.rollout_actor_cons)(net, n, **kw)
    else:
        if head == "actor":
            return env.rollout_actor_unc(net, n, **kw)
        a, o, r = env.rollout_policy_unc(net, n, **kw)
    return {"a": a, "obs": o, "rew": r}


def _network(spec, obs0, family, head):
    net = make_policy(spec, obs0, (16,), seed=17) if head == "policy" else make_ac(spec, obs0, (16,), seed=17)
    if family == "f32":
        from test_gpu_policy_f32 import ac32, to32

        n32 = to32(net) if head == "policy" else ac32(net)
        net.close()
        return n32
    return net


def _zero_actor(spec, family):
    """mu = 0, sigma = 1: u = fma(1, z, 0) = z"""
    from pcgym_amd import GaussianActorCritic, MLPPolicy

    # (applied: the sample clipped to the middle quarter of the action box -- test_noise_is_the_oracle_twin_bitwise's +-0.25 on a
    # normalised box; an action on the edge of its box drains a tank within these few steps, and 0 x NaN is NaN)
    lo, hi = action_box(spec)
    assert np.all(lo == lo[0]) and np.all(hi == hi[0])
    mid, half = (lo[0] + hi[0]) / 2, (hi[0] - lo[0]) / 2
    zero = MLPPolicy([np.zeros((spec.na, spec.nobs))], [np.zeros(spec.na)], out_map="clip", out_low=float(mid - 0.25 * half),
                     out_high=float(mid + 0.25 * half), **({"dtype": "float32"} if family == "f32" else {}))
    ac = GaussianActorCritic(zero, np.zeros(spec.na))
    assert np.array_equal(ac.sigma, np.ones(spec.na))
    return ac


def _cat(parts, name):
    return _torch().cat([getattr(q, name) if not isinstance(q, dict) else q[name] for q in parts], dim=-1)


def _physical(spec, obs, i):
    """slot i of an observation row, un-normalised"""
    if not spec.normalise_o:
        return obs[i]
    return (obs[i] + 1.0) / 2.0 * (spec.o_high[i] - spec.o_low[i]) + spec.o_low[i]


def _loop_draws(spec, obs1, orc_clean):
    """what the loop's first step drew, recovered from the recorded obs[0] and the oracle's noise-free step from the same start
    state with the same action: z of the observation noise (o = x (1 + pct z)) on a noise plan, the disturbance slots'
    deviation from the shared schedule on a Gaussian-disturbance plan"""
    if spec.noise:
        rows = [i for i in range(spec.nx) if spec.noise_pct[i] > 0]
        return np.stack([(_physical(spec, obs1, i) / orc_clean.x[i] - 1.0) / spec.noise_pct[i] for i in rows])
    lo = spec.nx + spec.nsp_obs
    return obs1[lo:lo + spec.nd] - orc_clean.obs[lo:lo + spec.nd]


def _oracle(spec, lo, hi, x_before, p_unc=None):
    from oracle import oracle as O

    if spec.user_rhs_src is not None:
        O.register_user_rhs(spec)
    orc = O.OracleEnv(spec, hi - lo, seed=SEED, env_offset=G + lo)
    orc.reset()
    assert np.allclose(orc.x, x_before, rtol=1e-14, atol=0), "reset at the global index (tested elsewhere) is not the oracle's"
    if p_unc is not None:
        assert np.allclose(orc.p_unc, p_unc, rtol=1e-14, atol=0), "reset at the global index (tested elsewhere): p_unc"
    orc.x[:] = x_before
    return orc


@pytest.mark.parametrize("family,plan,integ,head", CASES, ids=["-".join(c) for c in CASES])
def test_shards_reproduce_the_whole_at_global_indices_past_2_32(family, plan, integ, head):
    torch = _torch()
    t_start = time.perf_counter()
    p, p_clean = _params(plan, integ), _params(plan, integ, random=False)
    whole = _env(p, 0, B)
    shards = [_env(p, lo, hi) for lo, hi in SHARDS]
    spec = whole.spec
    spec_clean = _spec(p_clean)
    assert spec.integrator == integ and (spec.noise or spec.gauss) and not (spec_clean.noise or spec_clean.gauss)
    assert bool(spec.ncon) == (family == "cons") and bool(spec.nunc) == (family == "unc") and (spec.user_rhs_src is not None) == (family == "jit")
    seed = whole._episode_seed()
    assert all(e._episode_seed() == seed and e.env_offset == G + lo for e, (lo, _) in zip(shards, SHARDS)) and whole.env_offset == G

    # ---- 1. precondition: the reset at these offsets (tested elsewhere) ----
    state = ["x", "obs_soa"] + (["p_unc"] if spec.nunc else [])
    for n in state:
        assert torch.equal(_cat(shards, n), getattr(whole, n)), f"PRECONDITION (reset, not the closed loop): the shards' {n} are not the whole's slices"
    assert float(whole.x.std(dim=1).min()) > 0
    before = [{n: getattr(e, n).clone() for n in state} for e in shards]
    obs0 = whole.obs_soa.cpu().numpy().copy()
    net = _network(spec, obs0, family, head)

    # ---- 2. shards == whole, bitwise ----
    whole._lib.pcg_coverage_names(None, 0, 1)
    ref = _call(whole, family, head, net, T)
    parts = [_call(e, family, head, net, T) for e in shards]
    torch.cuda.synchronize()
    kernel = KERNEL[family].format(head)
    names = [n for n in _launch_names(whole._lib) if kernel in n and (family == "f32" or "_f32" not in n)]
    assert names and all(n.startswith("jit:") == (family == "jit") for n in names), (kernel, names)
    keys = [k for k, v in ref.items() if v is not None]
    assert set(keys) >= {"a", "obs", "rew"} | ({"u", "logp", "val"} if head == "actor" else set()) | ({"g", "viol"} if family == "cons" else set())
    for e in [whole] + shards:
        assert not e.status.any() and e.t == T
    for k in keys:
        assert bool(torch.isfinite(ref[k].double()).all()), k
        assert torch.equal(_cat(parts, k), ref[k]), f"{k}: the shards' records are not the whole's"
    for n in ("x", "obs_soa", "rew", "done", "g", "viol", "u_prev", "a_save_t", "p_unc"):
        if getattr(whole, n, None) is not None:
            assert torch.equal(torch.nan_to_num(_cat(shards, n).double(), nan=-7.0), torch.nan_to_num(getattr(whole, n).double(), nan=-7.0)), \
                f"io->{n} after the call: the shards' are not the whole's"
    if spec.nunc:
        assert torch.equal(whole.p_unc, _cat([b for b in before], "p_unc")), "the call wrote io->p_unc"

    # ---- 3. actors: the draws are the oracle's at the global index, bitwise ----
    if head == "actor":
        ac0 = _zero_actor(spec, family)
        us = []
        for lo, hi in SHARDS:
            e = _env(p, lo, hi)
            out = _call(e, family, head, ac0, T)
            torch.cuda.synchronize()
            want = z_twin(seed, G + lo, hi - lo, spec.na, range(T + 1))
            u = out["u"].cpu().numpy()
            assert u.shape == want.shape and np.isfinite(u).all() and bool(torch.isfinite(e.x).all()), "the zero actor's rollout is not finite"
            assert np.std(u) > 0.5, f"std(u) = {np.std(u):.3f} under the zero actor with sigma = 1"
            assert np.array_equal(u, want), f"shard at {lo}: the kernel's draws are not the oracle's at the global index G + {lo} + e"
            assert np.array_equal(out["logp"].cpu().numpy(), np.stack([logp_numpy(ac0, want[s]) for s in range(T + 1)])), "logp of the draws"
            us.append(u)
            e.close()
        assert not np.array_equal(us[0][:, :, :SHARDS[1][1] - SHARDS[1][0]], us[1]), "the two shards drew the same numbers"
        ac0.close()
        u0, u1 = (q["u"].cpu().numpy() for q in parts)
        assert not np.array_equal(u0[:, :, :u1.shape[2]], u1), "the two shards' samples are the same"

    # ---- 4. the first step is the oracle's (run-time compiled plans: the step module's open-loop replay) ----
    gap = {"x": 0.0, "obs": 0.0, "rew": 0.0, "g": 0.0}
    draws = []
    for (lo, hi), e_T, part, b4 in zip(SHARDS, shards, parts, before):
        x_before = b4["x"].cpu().numpy()
        a_np, o_np, r_np = (part[k].cpu().numpy() for k in ("a", "obs", "rew"))
        pu = b4["p_unc"].cpu().numpy() if spec.nunc else None
        clean = _oracle(spec_clean, lo, hi, x_before, pu)
        clean.step(a_np[0])
        draws.append(_loop_draws(spec, o_np[0], clean))
        if family == "jit":
            e_open = _env(p, lo, hi)
            oq, rq = e_open.rollout(part["a"][:T].contiguous(), collect_obs=True, collect_rew=True)
            torch.cuda.synchronize()
            assert torch.equal(oq, part["obs"]), f"shard at {lo}: observations differ from the open-loop replay of the recorded actions"
            assert torch.equal(rq, part["rew"]), f"shard at {lo}: rewards differ from the open-loop replay"
            assert torch.equal(e_open.x, e_T.x) and torch.equal(e_open.done, e_T.done) and torch.equal(e_open.status, e_T.status)
            e_open.close()
            continue
        e_1 = _env(p, lo, hi)  # one step alone: the state after it
        one = _call(e_1, family, head, net, 1, nxt=False)
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(one[k][0], part[k][0]), f"shard at {lo}: {k}[0] of a one-step call"
        orc = _oracle(spec, lo, hi, x_before, pu)
        oc, rc, dc = orc.step(a_np[0])
        assert np.isfinite(orc.x).all() and np.isfinite(rc).all()
        xg = e_1.x.cpu().numpy()
        assert np.array_equal(e_1.done.cpu().numpy(), dc)
        if family == "unc":
            tol = _tols(plan)
            ex = worst_rel(xg, orc.x)
            assert ex <= tol["x1"], f"shard at {lo}: state {ex:.3e} from the oracle at the global index"
            o_rtol, o_atol = tol["o_rtol"], tol["o_atol"]
        else:
            ex = float(np.max(np.abs(xg - orc.x) / np.maximum(np.abs(orc.x), 1.0)))
            assert ex <= 1e-12, f"shard at {lo}: state {ex:.3e} from the oracle (relative to max(|x|, 1))"
            o_rtol, o_atol = 1e-10, 1e-11
        sure = np.ones(hi - lo, dtype=bool)
        if family == "cons":
            gtol = G_TOL * row_scales(spec, orc.x, orc.slots, u_box(spec, a_np[0]))[:, None]
            dg = np.abs(part["g"][0].cpu().numpy() - orc.g)
            gap["g"] = max(gap["g"], float(np.max(dg / gtol)))
            assert np.all(dg <= gtol), f"shard at {lo}: a row {np.max(dg / gtol):.3e} x its tolerance from the oracle"
            sure = np.all(np.abs(orc.g) > gtol, axis=0)
            assert np.sum(~sure) <= 0.01 * sure.size, f"{np.sum(~sure)} of {sure.size} envs have a row within its tolerance of zero"
            assert np.array_equal(part["viol"][0].cpu().numpy()[sure], orc.viol.astype(bool)[sure]), f"shard at {lo}: flags differ from the oracle's"
        gap["x"] = max(gap["x"], ex)
        gap["obs"] = max(gap["obs"], float(np.max(np.abs(o_np[0] - oc) / (o_atol + o_rtol * np.abs(oc)))))
        gap["rew"] = max(gap["rew"], float(np.max(np.abs(r_np[0] - rc)[sure] / (1 + np.max(np.abs(rc))))))
        print(f"shard at {lo}: state {ex:.3e}, obs {gap['obs']:.3e} x its tolerance, rew {gap['rew']:.3e} from the oracle at env_offset = G + {lo}")
        assert np.allclose(o_np[0], oc, rtol=o_rtol, atol=o_atol), f"shard at {lo}: obs[0] is not the oracle's at the global index"
        assert _rew_close(r_np[0][sure], rc[sure]), f"shard at {lo}: rew[0] is not the oracle's at the global index"
        e_1.close()

    # ---- 5. non-vacuity: the shards' draws inside the loop differ, and the offset reaches the kernel ----
    n1 = SHARDS[1][1] - SHARDS[1][0]
    assert np.isfinite(draws[0]).all() and np.std(draws[1]) > 0
    assert not np.allclose(draws[0][:, :n1], draws[1], rtol=1e-3, atol=0), "the two shards' draws inside the loop are the same"
    if spec.noise:
        sd = float(np.std(np.concatenate(draws, axis=1)))
        assert 0.5 < sd < 2.0, f"the recovered observation noise has std {sd:.3f}, not that of a standard normal"
    e0 = _env(p, *SHARDS[1], offset=0)  # the second shard's envs, start state and all, at global index e
    for n in state:
        getattr(e0, n).copy_(before[1][n])
    at0 = _call(e0, family, head, net, T)
    torch.cuda.synchronize()
    what = "u" if head == "actor" else "obs"
    assert not torch.equal(at0[what][0], parts[1][what][0]), f"{what}[0] at env_offset = 0 is what it is at G: the offset does not reach the kernel"
    e0.close()

    dt = time.perf_counter() - t_start
    _record(f"case {family}-{plan}-{integ}-{head}: " + ("the open-loop replay of both shards bitwise" if family == "jit" else
            f"first step vs the oracle at G + lo: state {gap['x']:.2e}, obs {gap['obs']:.2e} x its tolerance, rew {gap['rew']:.2e} (of 1 + max|r|)"
            + (f", rows {gap['g']:.2e} x tolerance" if family == "cons" else "")) + f"; {dt:.2f} s")
    for e in [whole] + shards:
        e.close()
    net.close()


@pytest.mark.parametrize("base", [0, G], ids=["at0", "atG"])
@pytest.mark.parametrize("plan", ["cstr_noise", "unc_cstr_noise"])
def test_collect_onpolicy_on_shards(plan, base):
    """collect_onpolicy on shard.shard_range's layout (two ranks, the global batch starting at `base`), fused routes only:
    the concatenated shards are the unsharded collector's result, bitwise"""
    torch = _torch()
    from oracle import oracle as O
    from pcgym_amd import collect_onpolicy
    from pcgym_amd.shard import shard_range

    p = _params(plan, "rk4")
    ranges = [shard_range(B, r, 2) for r in range(2)]
    assert ranges == [(0, B // 2), (B // 2, B)]
    whole = _env(p, 0, B, offset=base)
    shards = [_env(p, lo, hi, offset=base) for lo, hi in ranges]  # (collect_onpolicy resets again: the envs stay in one RNG epoch)
    spec = whole.spec
    ac = make_ac(spec, whole.obs_soa.cpu().numpy(), (16,), seed=5, sigma_scale=0.1)
    route = dict(fused_unc=True) if spec.nunc else dict(fused=True)
    whole._lib.pcg_coverage_names(None, 0, 1)
    ref = collect_onpolicy(whole, ac, **route)
    parts = [collect_onpolicy(e, ac, **route) for e in shards]
    torch.cuda.synchronize()
    assert _launched(whole._lib, "rollout_unc_actor_kernel" if spec.nunc else "rollout_actor_kernel")
    for n in ("obs", "act", "logp", "val", "rew"):
        assert bool(torch.isfinite(ref[n]).all()) and ref[n].shape[-1] == B
        assert torch.equal(torch.cat([q[n] for q in parts], dim=-1), ref[n]), f"{n}: the sharded collection is not the unsharded one"
    assert float(ref["act"].std()) > 0 and not torch.equal(parts[0]["act"], parts[1]["act"])
    # ... whose first step is the oracle's at the global index (applied action = the clipped sample)
    orc = O.OracleEnv(spec, B, seed=SEED, env_offset=base)
    orc.reset(), orc.reset()
    a0 = np.clip(ref["act"][0].cpu().numpy(), ac.actor.out_low, ac.actor.out_high)
    oc, rc, _ = orc.step(a0)
    tol = _tols(plan) if spec.nunc else dict(o_rtol=1e-10, o_atol=1e-11)
    assert np.allclose(ref["obs"][1].cpu().numpy(), oc, rtol=tol["o_rtol"], atol=tol["o_atol"]) and _rew_close(ref["rew"][0].cpu().numpy(), rc)
    for e in [whole] + shards:
        e.close()
    ac.close()
