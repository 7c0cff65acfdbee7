"""The fused closed-loop rollout with a stochastic actor-critic (pcg_rollout_actor, pcg_rollout_actor.hpp) and the noise kernel of
the per-step route (pcg_policy_noise), against the oracle.  The method is that of tests/test_gpu_policy_rollout.py -- every
comparison TEACHER-FORCED, so that the amplification of a closed loop never enters a tolerance -- with these additions:

  noise twin      pcg_policy_noise, and the `u` the fused kernel records under an all-zero actor with sigma = 1, BITWISE equal to
                  the oracle's orc_rng_normal(seed, env_offset + e, t, 0x400, i): every lane, every component, row T included;
  sample bound    recorded u against mu_ref + sigma z (z: the oracle twin; mu_ref: the actor's raw output in np.longdouble on
                  the kernel's own recorded observation) inside host_reference's running bound + one rounding, 2^-53 |u|;
  clip exact      recorded a == clip(u) bitwise;  value bound: recorded value inside its own running bound;
  logp bitwise    q = 0; q = z_i z_i + q ascending; logp = c0 - q / 2 restated in numpy (z_i z_i is exact in fp64: z is an fp32
                  value; c0 is GaussianActorCritic.logp_const, the library's own constant);
  dynamics        the recorded a[:T] through the open-loop rollout (general kernel): observations, rewards, final state, done,
                  status, a_save bitwise;
  chaining        one call per step bitwise equal to the one call; after every step the state within 1e-12 of max(|x|, 1) of
                  OracleEnv.step on the recorded action from the common start state;
  sharding, the public path (collect_onpolicy fused against its per-step route, 8 x the spread of two per-step runs under
  a hidden-unit permutation + 1e-13), refusals, pcg_policy_update, stream capture.

Measured figures are printed and, when PCG_RECORD_DIR names a directory, appended to actor_rollout_test.txt there.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import scenarios as SC
from helpers import (CASE_KEYS, LD, PRE_MAX, SHAPES, U, UNSUPPORTED_PLANS, _case_params, _launched, _make, _perm_hidden, _spread_x0,
                     _torch, host_reference, make_policy, tanh_k)
from helpers import _record as _record_to

pytestmark = pytest.mark.gpu

RNG_POLICY = 0x400


def _record(line):
    _record_to("actor_rollout_test.txt", line)


def z_twin(seed, env_offset, B, na, ts):
    """(len(ts), na, B): the oracle's restatement of the kernel's draws"""
    from oracle import oracle as O

    f = O.lib().orc_rng_normal
    out = np.empty((len(ts), na, B))
    for k, t in enumerate(ts):
        for i in range(na):
            for e in range(B):
                out[k, i, e] = f(seed, env_offset + e, t, RNG_POLICY, i)
    return out


def action_box(spec):
    if spec.normalise_a:
        lo, hi = -np.ones(spec.na), np.ones(spec.na)
    else:
        lo, hi = np.asarray(spec.a_low, dtype=float), np.asarray(spec.a_high, dtype=float)
    return lo, hi


def make_ac(spec, obs0, hidden, seed, out_map="clip", sigma_scale=0.25, critic=True, centre=0.0, box=1.6):
    """make_policy's actor (weights scaled by the plan's boxes) with the given map, sigma = sigma_scale x the action half
    width, and a critic of the same hidden shape (make_policy's network, first output row)"""
    from pcgym_amd import GaussianActorCritic, MLPPolicy

    pol = make_policy(spec, obs0, hidden, seed)
    lo, hi = action_box(spec)
    sigma = sigma_scale * np.maximum((hi - lo) / 2, 1e-3)
    Ws, bs = [w.copy() for w in pol.weights], [b.copy() for b in pol.biases]
    out_low, out_high = pol.out_low, pol.out_high
    if out_map == "clip":
        # Both branches of the clip have to occur, and the applied actions have to stay mild (a policy leaning on an edge of
        # the action box drains a tank or quenches a reactor within a few steps).  The envs of a case start within a few
        # percent of each other, so their first means nearly coincide: the output bias is shifted so that the mean at the mean
        # reset observation is the middle of the action box (+ `centre` half widths), and the clip box is that point +- `box`
        # sigma -- with the default 1.6 a sample leaves it with probability 0.11 per lane and component and stays inside
        # otherwise; what the env is given lies within 0.4 of the half width around the middle.
        assert np.all(lo == lo[0]) and np.all(hi == hi[0]), "one clip box for all components: the action boxes must coincide"
        o_mean = np.mean(obs0, axis=1, keepdims=True)
        mu_c = host_reference(MLPPolicy(Ws, bs, activation=pol.activation, out_map="none"), o_mean, 0.0)[0][:, 0].astype(np.float64)
        mid = (lo[0] + hi[0]) / 2 + centre * (hi[0] - lo[0]) / 2
        bs[-1] = bs[-1] + (mid - mu_c)
        out_low, out_high = float(mid - box * sigma.min()), float(mid + box * sigma.min())
    actor = MLPPolicy(Ws, bs, activation=pol.activation, out_map=out_map, out_low=out_low, out_high=out_high)
    cr = None
    if critic:
        c = make_policy(spec, obs0, hidden, seed + 100)
        cr = MLPPolicy(c.weights[:-1] + [c.weights[-1][:1]], c.biases[:-1] + [c.biases[-1][:1]], activation=c.activation, out_map="none")
        c.close()
    pol.close()
    return GaussianActorCritic(actor, np.log(sigma), cr)


def _np_raw(pol, obs):
    h = obs
    for l, (W, b) in enumerate(zip(pol.weights, pol.biases)):
        h = W @ h + b[:, None]
        if l < len(pol.weights) - 1:
            h = np.tanh(h) if pol.activation == "tanh" else np.maximum(h, 0)
    return h


def host_conditioning(spec, ac, B, T, env_seed, n_threads=1):
    """The ORACLE's own sensitivity along the case's closed loop, simulated on the host (fp64 numpy actor, the oracle's noise
    twin): the largest change of a step's result, relative to max(|x|, 1), when the step's start state is perturbed by 1e-15
    relative; inf if a state is not finite.  Also the share of clipped samples at the first step.  An explicit step whose
    stages leave the model's physical range (a concentration below zero next to the pole of a Monod term) amplifies round-off
    by many orders of magnitude: no two correct implementations agree to 1e-12 there, and the oracle comparison is only
    meaningful on inputs where this figure is small."""
    from oracle import oracle as O

    o1, o2 = (O.OracleEnv(spec, B, seed=env_seed, n_threads=n_threads) for _ in range(2))
    o1.reset(), o2.reset()
    z = z_twin(o1._seed(), 0, B, spec.na, range(T))
    rng = np.random.default_rng(0)
    obs, worst, clipped0 = o1.obs.copy(), 0.0, None
    lo, hi = ac.actor.out_low, ac.actor.out_high
    for s in range(T):
        u = _np_raw(ac.actor, obs) + ac.sigma[:, None] * z[s]
        if s == 0:
            clipped0 = float(np.mean((u < lo) | (u > hi)))
        a = np.clip(u, lo, hi) if ac.actor.out_map == "clip" else u
        o2.x[:] = o1.x * (1 + 1e-15 * rng.standard_normal(o1.x.shape))
        obs = o1.step(a)[0].copy()
        o2.step(a)
        if not (np.isfinite(o1.x).all() and np.isfinite(o2.x).all()):
            return float("inf"), clipped0
        worst = max(worst, float(np.max(np.abs(o1.x - o2.x) / np.maximum(np.abs(o1.x), 1.0))))
    return worst, clipped0


# where the clip box sits (centre in half widths from the middle of the action box, half width in sigmas): the first entry
# under which the case is well conditioned for the oracle itself.  The narrow boxes keep the applied action within 0.05 of
# the half width around their centre (most samples are clipped, about one in six is not).
BOXES = [(0.0, 1.6), (-0.5, 0.2), (0.5, 0.2), (-0.25, 0.2), (0.25, 0.2)]
WELL_CONDITIONED = 1e-13  # a 1e-15 perturbation grows at most 100-fold: round-off stays two orders below the 1e-12 bar


def pick_ac(spec, obs0, hidden, seed, B, T, env_seed):
    tried = []
    for centre, box in BOXES:
        ac = make_ac(spec, obs0, hidden, seed, centre=centre, box=box)
        amp, clipped0 = host_conditioning(spec, ac, B, T, env_seed)
        tried.append((centre, box, amp, clipped0))
        if amp <= WELL_CONDITIONED and 0.0 < clipped0 < 1.0:
            return ac, (centre, box, amp)
        ac.close()
    raise AssertionError(f"no clip box of {BOXES} gives a well-conditioned case with both clip branches: {tried}")


def raw_twin(pol):
    """the same network without its output map: host_reference then returns the raw output and its bound"""
    from pcgym_amd import MLPPolicy

    return MLPPolicy(pol.weights, pol.biases, activation=pol.activation, out_map="none")


def logp_numpy(ac, z):
    """z (na, M) -> the kernel's statement, operation by operation"""
    q = np.zeros(z.shape[1])
    for i in range(z.shape[0]):
        q = z[i] * z[i] + q  # (the product of two fp32 values is exact in fp64: one rounding, the FMA's)
    return ac.logp_const - 0.5 * q  # (q / 2 is exact: one rounding again)


# ---- 1. noise twin -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,offset", [("cstr", 0), ("four_tank", 1000003), ("distillation_column", (1 << 33) + 5)])
def test_noise_is_the_oracle_twin_bitwise(key, offset):
    torch = _torch()
    from oracle import oracle as O
    from pcgym_amd import GaussianActorCritic, MLPPolicy

    B, T = 200, 3
    p = _spread_x0(_case_params(key, "rk4"))
    env = _make(p, B, seed=11, env_offset=offset)
    spec = env.spec
    env.reset()
    seed = env._episode_seed()
    ts = [0, 1, 2, 3, 57, 100000]
    want = z_twin(seed, offset, B, spec.na, ts)
    assert np.std(want) > 0.5 and len(np.unique(want)) > 0.9 * want.size
    for k, t in enumerate(ts):
        z = env.policy_noise(t)
        torch.cuda.synchronize()
        assert z.shape == (spec.na, B)
        assert np.array_equal(z.cpu().numpy(), want[k]), f"pcg_policy_noise at t = {t} is not the oracle twin"
    # the fused kernel draws the same bits: all-zero actor, sigma = 1 -> u = fma(1, z, 0) = z, row T included
    zero = MLPPolicy([np.zeros((spec.na, spec.nobs))], [np.zeros(spec.na)], out_map="clip", out_low=-0.25, out_high=0.25)
    ac = GaussianActorCritic(zero, np.zeros(spec.na))
    assert np.array_equal(ac.sigma, np.ones(spec.na))
    x_before = env.x.cpu().numpy().copy()
    out = env.rollout_actor(ac, T, record_next_action=True)
    torch.cuda.synchronize()
    assert out["val"] is None and out["u"].shape == (T + 1, spec.na, B)
    assert np.array_equal(out["u"].cpu().numpy(), want[:T + 1]), "the fused kernel's draws are not the oracle twin"
    assert np.array_equal(out["a"].cpu().numpy(), np.clip(want[:T + 1], -0.25, 0.25))
    assert np.array_equal(out["logp"].cpu().numpy(), np.stack([logp_numpy(ac, want[s]) for s in range(T + 1)]))
    # ... and the step it then takes is the oracle's (first step, the recorded action)
    orc = O.OracleEnv(spec, B, seed=11, env_offset=offset)
    orc.reset()
    orc.x[:] = x_before
    orc.step(out["a"][0].cpu().numpy())
    e1 = _make(p, B, seed=11, env_offset=offset)
    e1.reset()
    e1.rollout_actor(ac, 1)
    torch.cuda.synchronize()
    err = float(np.max(np.abs(e1.x.cpu().numpy() - orc.x) / np.maximum(np.abs(orc.x), 1.0)))
    assert err <= 1e-12, err
    env.close(), e1.close(), ac.close()


# ---- 2 / 3. the sweep ----------------------------------------------------------------------------------------------------------
def _sweep_case(key, integ, shape, out_map, sigma_scale):
    torch = _torch()
    from oracle import oracle as O

    B, T = 200, 6
    p = _spread_x0(_case_params(key, integ))
    e_one, e_chain = (_make(p, B, seed=9) for _ in range(2))
    e_open = _make(p, B, seed=9, variant=1)  # PCG_OPT_VARIANT 1: the general kernels
    spec = e_one.spec
    assert spec.integrator == integ and not spec.ncon and not spec.nunc and spec.x0_unc is not None
    for e in (e_one, e_chain, e_open):
        e.reset()
    obs0 = e_one.obs_soa.cpu().numpy().copy()
    x0 = e_one.x.cpu().numpy().copy()
    if out_map == "clip":
        assert sigma_scale == 0.25
        ac, chosen = pick_ac(spec, obs0, SHAPES[shape], 17, B, T, 9)
    else:
        ac, chosen = make_ac(spec, obs0, SHAPES[shape], seed=17, out_map=out_map, sigma_scale=sigma_scale), None
    pol, cr = ac.actor, ac.critic
    assert pol.validate() == 0 and cr.validate() == 0
    raw = raw_twin(pol)
    k = tanh_k()
    seed = e_one._episode_seed()
    z = z_twin(seed, 0, B, spec.na, range(T + 1))
    sig = ac.sigma[:, None]
    lo, hi = pol.out_low, pol.out_high

    if out_map == "clip":
        # branch coverage is a condition on the INPUTS: confirmed on the host for the first step (the reset observation) before
        # the device's records are relied on
        mu0, _, _ = host_reference(raw, obs0, k + 1.0)
        u0 = (mu0 + sig.astype(LD) * z[0].astype(LD)).astype(np.float64)
        assert np.any((u0 < lo) | (u0 > hi)) and np.any((u0 > lo) & (u0 < hi)), \
            f"first step on the host: {np.mean((u0 < lo) | (u0 > hi)):.3f} of the samples outside the box [{lo}, {hi}]"

    # ---- the fused closed loop: one call ----
    out = e_one.rollout_actor(ac, T, collect_obs=True, collect_rew=True, record_next_action=True)
    torch.cuda.synchronize()
    a_seq, u_seq, lp_seq, v_seq, obs_seq, rew_seq = (out[n] for n in ("a", "u", "logp", "val", "obs", "rew"))
    a_np, u_np, lp_np, v_np, o_np = (t.cpu().numpy() for t in (a_seq, u_seq, lp_seq, v_seq, obs_seq))
    assert a_np.shape == u_np.shape == (T + 1, spec.na, B) and lp_np.shape == v_np.shape == (T + 1, B) and o_np.shape == (T, spec.nobs, B)
    for arr in (a_np, u_np, lp_np, v_np, o_np):
        assert np.isfinite(arr).all()
    assert not e_one.status.any()
    assert torch.equal(e_one.obs_soa, obs_seq[T - 1]) and torch.equal(e_one.rew, rew_seq[T - 1]) and e_one.t == T

    # ---- sample bound, value bound: on the kernel's own recorded observation ----
    worst_u, worst_v, pre = 0.0, 0.0, 0.0
    for s in range(T + 1):
        o_in = obs0 if s == 0 else o_np[s - 1]
        mu, b_mu, pm = host_reference(raw, o_in, k + 1.0)
        pre = max(pre, pm)
        ref = mu + sig.astype(LD) * z[s].astype(LD)
        diff = np.abs(u_np[s].astype(LD) - ref).astype(np.float64)
        bound = b_mu + U * np.abs(u_np[s])
        assert np.all(diff <= bound), (f"step {s}: sample off by {np.max(diff):.3e}, {np.max(diff / np.maximum(bound, 1e-300)):.2f} x "
                                       f"the running bound + one rounding ({np.max(bound):.3e})")
        worst_u = max(worst_u, float(np.max(diff / np.maximum(bound, 1e-300))))
        vr, b_v, pm = host_reference(cr, o_in, k + 1.0)
        pre = max(pre, pm)
        dv = np.abs(v_np[s].astype(LD) - vr[0]).astype(np.float64)
        assert np.all(dv <= b_v[0]), f"step {s}: value off by {np.max(dv):.3e}, {np.max(dv / np.maximum(b_v[0], 1e-300)):.2f} x its running bound"
        worst_v = max(worst_v, float(np.max(dv / np.maximum(b_v[0], 1e-300))))
    assert pre <= PRE_MAX, f"pre-activations up to {pre:.1f}: outside the grid the tanh error was measured on"
    assert np.std(u_np) > 0 and np.std(v_np) > 0

    # ---- clip exact; logp bitwise ----
    if out_map == "clip":
        assert np.array_equal(a_np, np.clip(u_np, lo, hi)), "a is not clip(u) bitwise"
        clipped = float(np.mean((u_np < lo) | (u_np > hi)))
        assert 0.0 < clipped < 1.0, f"{clipped:.3f} of the recorded samples were clipped: one branch of the map was never taken"
        assert np.any(a_np != u_np) and np.any((a_np == u_np) & (a_np > lo) & (a_np < hi))
    else:
        assert np.array_equal(a_np, u_np), "out_map none: a is not u bitwise"
        clipped = 0.0
    for s in range(T + 1):
        assert np.array_equal(lp_np[s], logp_numpy(ac, z[s])), f"step {s}: logp is not the specified operation sequence"

    # ---- dynamics: the recorded applied actions through the open-loop rollout, general kernel: bitwise ----
    assert np.array_equal(e_open.x.cpu().numpy(), x0)
    oq, rq = e_open.rollout(a_seq[:T].contiguous(), collect_obs=True, collect_rew=True)
    torch.cuda.synchronize()
    assert torch.equal(oq, obs_seq), "observations differ from the open-loop replay of the recorded actions"
    assert torch.equal(rq, rew_seq), "rewards differ from the open-loop replay"
    assert torch.equal(e_open.x, e_one.x), "final state differs from the open-loop replay"
    assert torch.equal(e_open.done, e_one.done) and torch.equal(e_open.status, e_one.status)
    if spec.a_delta:
        assert torch.equal(e_open.a_save_t, e_one.a_save_t)

    # ---- chaining: one call per step == the one call, bitwise; every step against the oracle, every lane ----
    orc = O.OracleEnv(spec, B, seed=9)
    orc.reset()
    assert np.allclose(orc.x, x0, rtol=1e-14, atol=0)
    worst_x = 0.0
    for s in range(T):
        x_before = e_chain.x.cpu().numpy().copy()
        o1 = e_chain.rollout_actor(ac, 1, collect_obs=True, collect_rew=True, record_next_action=(s == T - 1))
        torch.cuda.synchronize()
        for n, full in (("a", a_seq), ("u", u_seq), ("logp", lp_seq), ("val", v_seq), ("obs", obs_seq), ("rew", rew_seq)):
            assert torch.equal(o1[n][0], full[s]), f"chained call {s}: {n}"
        if s == T - 1:
            for n, full in (("a", a_seq), ("u", u_seq), ("logp", lp_seq), ("val", v_seq)):
                assert torch.equal(o1[n][1], full[T]), f"chained call {s}: row T of {n}"
        orc.x[:] = x_before  # teacher-forced: common start state, the recorded action
        oc, rc, dc = orc.step(a_np[s])
        xg = e_chain.x.cpu().numpy()
        assert np.isfinite(orc.x).all()
        err = float(np.max(np.abs(xg - orc.x) / np.maximum(np.abs(orc.x), 1.0)))
        worst_x = max(worst_x, err)
        assert err <= 1e-12, f"step {s}: state {err:.3e} from the oracle (relative to max(|x|, 1))"
        assert np.array_equal(e_chain.done.cpu().numpy(), dc)
        if not spec.noise:
            assert np.allclose(o1["obs"][0].cpu().numpy(), oc, rtol=1e-10, atol=1e-11)
        assert np.allclose(o1["rew"][0].cpu().numpy(), rc, rtol=1e-9, atol=1e-10 * (1 + np.max(np.abs(rc))))
    assert torch.equal(e_chain.x, e_one.x)
    _record(f"case {key}-{integ}-{shape}-{out_map}: sample error <= {worst_u:.3f} x bound, value error <= {worst_v:.3f} x bound, "
            f"|pre-activation| <= {pre:.2f}, {clipped:.3f} of the samples clipped, state vs oracle {worst_x:.2e}"
            + (f", clip box centre {chosen[0]:+.2f} half widths +- {chosen[1]} sigma (oracle's own 1e-15 sensitivity {chosen[2]:.1e})" if chosen else ""))
    for e in (e_one, e_chain, e_open):
        e.close()
    ac.close(), raw.close()


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("integ", ["rk4", "cv8"])
@pytest.mark.parametrize("key", CASE_KEYS)
def test_actor_rollout(key, integ, shape):
    """every model x {RK4, CV8} x network shape: a clip map, sigma a quarter of the action half width, a critic of the actor's
    hidden shape"""
    _sweep_case(key, integ, shape, "clip", 0.25)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_unbounded_actor(shape):
    """out_map none and a small sigma: the applied action is the sample itself"""
    _sweep_case("cstr", "rk4", shape, "none", 0.02)


# ---- 4. sharding ---------------------------------------------------------------------------------------------------------------
def test_two_shards_reproduce_the_unsharded_run():
    torch = _torch()
    from oracle import oracle as O

    B, T = 200, 5
    p = _spread_x0(_case_params("cstr_noise", "rk4"))
    whole = _make(p, B, seed=13)
    halves = [_make(p, B // 2, seed=13, env_offset=off) for off in (0, B // 2)]
    for e in [whole] + halves:
        e.reset()
    ac = make_ac(whole.spec, whole.obs_soa.cpu().numpy(), (16,), seed=5)
    x0 = whole.x.cpu().numpy().copy()
    ref = whole.rollout_actor(ac, T, collect_obs=True, record_next_action=True)
    parts = [e.rollout_actor(ac, T, collect_obs=True, record_next_action=True) for e in halves]
    torch.cuda.synchronize()
    for n in ("a", "u", "logp", "val", "obs", "rew"):
        assert torch.equal(torch.cat([q[n] for q in parts], dim=-1), ref[n]), n
    assert torch.equal(torch.cat([e.x for e in halves], dim=-1), whole.x)
    assert float(ref["u"].std()) > 0 and not torch.equal(parts[0]["u"], parts[1]["u"])
    orc = O.OracleEnv(whole.spec, B, seed=13)  # (the run the shards reproduce takes the oracle's first step)
    orc.reset()
    orc.x[:] = x0
    _, rc, _ = orc.step(ref["a"][0].cpu().numpy())
    assert np.allclose(ref["rew"][0].cpu().numpy(), rc, rtol=1e-9, atol=1e-10 * (1 + np.max(np.abs(rc))))
    for e in [whole] + halves:
        e.close()
    ac.close()


# ---- 5. the public path --------------------------------------------------------------------------------------------------------
def _gae_numpy(rew, val, gamma, lam, bootstrap_last):
    T = rew.shape[0]
    adv = np.zeros_like(rew)
    last = np.zeros_like(rew[0])
    for t in range(T - 1, -1, -1):
        nxt = val[t + 1] if (t < T - 1 or bootstrap_last) else 0.0
        last = (rew[t] + gamma * nxt - val[t]) + gamma * lam * last
        adv[t] = last
    return adv, adv + val[:T]


def _dist(a, b):
    """largest difference over the collected arrays, each relative to max(1, largest entry of the reference array)"""
    d = 0.0
    for n in ("obs", "act", "logp", "val", "rew"):
        ref = b[n].cpu().numpy()
        d = max(d, float(np.max(np.abs(a[n].cpu().numpy() - ref)) / max(1.0, float(np.max(np.abs(ref))))))
    return d


@pytest.mark.parametrize("bootstrap_last", [False, True])
@pytest.mark.parametrize("scen,integ,shape", [("cstr_canonical", "rk4", "1x16"), ("four_tank_canonical", "cv8", "2x64")])
def test_collect_onpolicy_takes_the_fused_call(scen, integ, shape, bootstrap_last):
    torch = _torch()
    from oracle import oracle as O
    from pcgym_amd import GaussianActorCritic, collect_onpolicy

    B = 4096
    p = copy.deepcopy(SC.scenarios()[scen]["env_params"])
    p.update(integrator=integ)
    envs = [_make(_spread_x0(p, 0.01), B, seed=4) for _ in range(3)]
    spec = envs[0].spec
    N = spec.N
    for e in envs:
        e.reset()  # (collect_onpolicy resets again: the three envs stay in the same RNG epoch)
    ac = make_ac(spec, envs[0].obs_soa.cpu().numpy(), SHAPES[shape], seed=23, sigma_scale=0.1)
    ac2 = GaussianActorCritic(_perm_hidden(ac.actor, 5), ac.log_std, _perm_hidden(ac.critic, 6))
    envs[0]._lib.pcg_coverage_names(None, 0, 1)
    fused = collect_onpolicy(envs[0], ac, bootstrap_last=bootstrap_last)
    torch.cuda.synchronize()
    assert _launched(envs[0]._lib, "rollout_actor_kernel"), "collect_onpolicy did not take the fused call"
    ref = collect_onpolicy(envs[1], ac, bootstrap_last=bootstrap_last, fused=False)
    ref2 = collect_onpolicy(envs[2], ac2, bootstrap_last=bootstrap_last, fused=False)
    torch.cuda.synchronize()
    shapes = {"obs": (N, spec.nobs, B), "act": (N - 1, spec.na, B), "logp": (N - 1, B), "val": (N, B), "rew": (N - 1, B),
              "adv": (N - 1, B), "ret": (N - 1, B)}
    for n, shp in shapes.items():
        assert tuple(fused[n].shape) == shp == tuple(ref[n].shape), n
        assert bool(torch.isfinite(fused[n]).all()), n
    assert envs[0].t == envs[1].t == N - 1
    # logp comes from the same random bits by the same operations on both routes
    assert torch.equal(fused["logp"], ref["logp"])
    spread, dist = _dist(ref2, ref), _dist(fused, ref)
    _record(f"collect_onpolicy {scen}-{integ}-{shape} B={B} N={N}: per-step spread under hidden-unit permutation {spread:.3e}, "
            f"fused vs per-step {dist:.3e} ({dist / max(spread, 1e-300):.2f} x)")
    assert spread > 0, "the permuted run is bitwise the reference run: the spread measures nothing"
    assert dist <= 8 * spread + 1e-13, f"fused result {dist:.3e} from the per-step path; two per-step runs differ by {spread:.3e}"
    # obs row 0 is the reset observation, the policy's input; the samples are the noise twin around the mean
    assert torch.equal(fused["obs"][0], ref["obs"][0])
    z0 = envs[1].policy_noise(0)
    u0 = ac.sample(fused["obs"][0].t(), z0.t()).t()
    assert torch.allclose(fused["act"][0], u0, rtol=1e-12, atol=1e-12)
    # the oracle, teacher-forced on the fused trajectory's first steps: applied action = out_map(sample)
    orc = O.OracleEnv(spec, 64, seed=4)
    orc.reset(), orc.reset()
    for i in range(3):
        a = np.clip(fused["act"][i, :, :64].cpu().numpy(), ac.actor.out_low, ac.actor.out_high)
        _, rc, _ = orc.step(a)
    assert np.allclose(fused["rew"][2, :64].cpu().numpy(), rc, rtol=1e-6, atol=1e-8 * (1 + np.max(np.abs(rc))))
    # adv / ret: the numpy GAE on the returned arrays
    a_ref, r_ref = _gae_numpy(fused["rew"].cpu().numpy(), fused["val"].cpu().numpy(), 0.99, 0.95, bootstrap_last)
    scale = max(1.0, float(np.max(np.abs(a_ref))))
    assert np.max(np.abs(fused["adv"].cpu().numpy() - a_ref)) <= 1e-13 * scale
    assert np.max(np.abs(fused["ret"].cpu().numpy() - r_ref)) <= 1e-13 * scale
    for e in envs:
        e.close()
    ac.close(), ac2.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
UNSUPPORTED = {
    **UNSUPPORTED_PLANS,
    "tanh_map": ("cstr_canonical", dict(integrator="rk4")),
    "wrong_size_critic": ("cstr_canonical", dict(integrator="rk4")),
}


def _raw_call(env, actor_h, critic_h, sigma, bufs, T=2):
    spec, B = env.spec, env.B
    a_out, u_out, lp_out, v_out = bufs
    sg = (C.c_double * len(sigma))(*sigma) if sigma is not None else None
    return env._lib.pcg_rollout_actor(env._plan, env._bufp, actor_h, critic_h, sg, 0, T, a_out.data_ptr(), spec.na * B, B,
                                      u_out.data_ptr(), spec.na * B, B, lp_out.data_ptr(), B, v_out.data_ptr(), B,
                                      None, 0, 0, None, 0, 1, 1, None)


@pytest.mark.parametrize("what", list(UNSUPPORTED))
def test_refusals_launch_nothing_and_collection_still_works(what):
    torch = _torch()
    from oracle import oracle as O
    from pcgym_amd import GaussianActorCritic, MLPPolicy, collect_onpolicy
    from pcgym_amd import _abi as abi

    scen, over = UNSUPPORTED[what]
    p = copy.deepcopy(SC.scenarios()[scen]["env_params"])
    p.update(over)
    B = 256
    env, env2 = _make(p, B, seed=2), _make(p, B, seed=2)
    spec = env.spec
    env.reset(), env2.reset()
    ac = make_ac(spec, env.obs_soa.cpu().numpy(), (16,), seed=3)
    actor_h, critic_h, want = ac.actor.handle(env.device), ac.critic.handle(env.device), abi.PCG_E_UNSUPPORTED
    extra = []
    if what == "tanh_map":
        sq = MLPPolicy(ac.actor.weights, ac.actor.biases, activation="tanh", out_map="tanh")
        extra.append(sq)
        actor_h = sq.handle(env.device)
    if what == "wrong_size_critic":
        two = MLPPolicy([np.zeros((2, spec.nobs))], [np.zeros(2)], out_map="none")       # two outputs
        other = MLPPolicy([np.zeros((1, spec.nobs + 1))], [np.zeros(1)], out_map="none")  # another input size
        extra += [two, other]
        critic_h, want = two.handle(env.device), abi.PCG_E_DIM
    x_before, o_before = env.x.clone(), env.obs_soa.clone()
    bufs = [torch.full(shp, -7.0, dtype=torch.float64, device=env.device) for shp in ((3, spec.na, B), (3, spec.na, B), (3, B), (3, B))]
    env._lib.pcg_coverage_names(None, 0, 1)
    rc = _raw_call(env, actor_h, critic_h, list(ac.sigma), bufs)
    torch.cuda.synchronize()
    assert rc == want
    if what == "wrong_size_critic":
        assert _raw_call(env, actor_h, extra[1].handle(env.device), list(ac.sigma), bufs) == abi.PCG_E_DIM
        # on this plan, which qualifies: sigma must be finite and positive, and must be there
        for bad in (0.0, -0.5, float("inf"), float("nan")):
            assert _raw_call(env, actor_h, ac.critic.handle(env.device), [bad] * spec.na, bufs) == abi.PCG_E_VALUE
        assert _raw_call(env, actor_h, ac.critic.handle(env.device), None, bufs) == abi.PCG_E_NULL
        wrong = MLPPolicy([np.zeros((spec.na, spec.nobs + 1))], [np.zeros(spec.na)])
        extra.append(wrong)
        assert _raw_call(env, wrong.handle(env.device), None, list(ac.sigma), bufs) == abi.PCG_E_DIM
        # pcg_policy_update keeps the shape
        wide = MLPPolicy([np.zeros((17, spec.nobs)), np.zeros((spec.na, 17))], [np.zeros(17), np.zeros(spec.na)])
        cfg, keep = wide.to_cfg()
        assert env._lib.pcg_policy_update(ac.actor.handle(env.device), C.byref(cfg)) == abi.PCG_E_DIM
        deeper = MLPPolicy([np.zeros((16, spec.nobs)), np.zeros((16, 16)), np.zeros((spec.na, 16))], [np.zeros(16), np.zeros(16), np.zeros(spec.na)])
        cfg, keep = deeper.to_cfg()
        assert env._lib.pcg_policy_update(ac.actor.handle(env.device), C.byref(cfg)) == abi.PCG_E_DIM
        with pytest.raises(ValueError):
            ac.update_(actor=(wide.weights, wide.biases))
    torch.cuda.synchronize()
    assert not _launched(env._lib, "rollout_actor_kernel"), "a refused call launched the kernel"
    assert torch.equal(env.x, x_before) and torch.equal(env.obs_soa, o_before), "a refused call wrote the env"
    assert all(bool((b == -7.0).all()) for b in bufs), "a refused call wrote an output buffer"
    # the public path returns through the per-step route (the tanh actor is not an actor-critic at all: ValueError at construction)
    if what == "tanh_map":
        with pytest.raises(ValueError):
            GaussianActorCritic(extra[0], ac.log_std, ac.critic)
    if what == "wrong_size_critic":
        ac_run = ac  # (a critic of the wrong size cannot be evaluated by any route: the fitting one is collected)
    else:
        ac_run = ac
    d1 = collect_onpolicy(env, ac_run)
    d2 = collect_onpolicy(env2, ac_run, fused=False)
    torch.cuda.synchronize()
    fused_taken = _launched(env._lib, "rollout_actor_kernel")
    assert fused_taken == (what in ("tanh_map", "wrong_size_critic"))  # (those two plans qualify; the others do not)
    if not fused_taken:
        for n in d2:
            assert torch.equal(d1[n], d2[n]), n
        with pytest.raises(Exception, match="-6"):
            env.rollout_actor(ac, 2)
        with pytest.raises(ValueError):
            collect_onpolicy(env, ac, fused=True)
    assert d1["obs"].shape == (spec.N, spec.nobs, B)
    orc = O.OracleEnv(spec, B, seed=2)  # ... whose first step is the oracle's
    orc.reset(), orc.reset()
    a0 = np.clip(d1["act"][0].cpu().numpy(), ac.actor.out_low, ac.actor.out_high)
    _, r0, _ = orc.step(a0)
    assert np.allclose(d1["rew"][0].cpu().numpy(), r0, rtol=1e-6, atol=1e-8 * (1 + np.max(np.abs(r0))))
    for e in (env, env2):
        e.close()
    ac.close()
    for q in extra:
        q.close()


# ---- 7. weight update ----------------------------------------------------------------------------------------------------------
def test_update_equals_a_fresh_policy_bitwise():
    torch = _torch()
    from oracle import oracle as O

    B, T = 1024, 8
    p = _spread_x0(_case_params("four_tank", "rk4"))
    e_old, e_upd, e_new = (_make(p, B, seed=21) for _ in range(3))
    spec = e_old.spec
    for e in (e_old, e_upd, e_new):
        e.reset()
    obs0 = e_old.obs_soa.cpu().numpy()
    x0 = e_old.x.cpu().numpy().copy()
    ac = make_ac(spec, obs0, (64, 64), seed=1)
    from pcgym_amd import GaussianActorCritic

    other = make_ac(spec, obs0, (64, 64), seed=2)  # other weights, the same shapes and clip box ...
    fresh = GaussianActorCritic(other.actor, other.log_std - 0.3, other.critic)  # ... and another sigma
    assert (fresh.actor.out_low, fresh.actor.out_high) == (ac.actor.out_low, ac.actor.out_high)
    before = e_old.rollout_actor(ac, T, collect_obs=True, record_next_action=True)
    torch.cuda.synchronize()
    h_a, h_c = ac.actor.handle(e_old.device).value, ac.critic.handle(e_old.device).value
    ac.update_(actor=(fresh.actor.weights, fresh.actor.biases), log_std=fresh.log_std, critic=(fresh.critic.weights, fresh.critic.biases))
    assert (ac.actor.handle(e_old.device).value, ac.critic.handle(e_old.device).value) == (h_a, h_c), "update_ made new device objects"
    assert ac.logp_const == fresh.logp_const
    got = e_upd.rollout_actor(ac, T, collect_obs=True, record_next_action=True)
    want = e_new.rollout_actor(fresh, T, collect_obs=True, record_next_action=True)
    torch.cuda.synchronize()
    for n in ("a", "u", "logp", "val", "obs", "rew"):
        assert torch.equal(got[n], want[n]), f"{n}: the updated policy is not the fresh one"
        assert not torch.equal(got[n], before[n]), f"{n}: the update changed nothing"
    assert torch.equal(e_upd.x, e_new.x)
    assert torch.equal(ac.mean(e_upd.obs), fresh.mean(e_upd.obs))  # the torch callable follows as well
    orc = O.OracleEnv(spec, B, seed=21)
    orc.reset()
    orc.x[:] = x0
    _, rc, _ = orc.step(got["a"][0].cpu().numpy())
    assert np.allclose(got["rew"][0].cpu().numpy(), rc, rtol=1e-9, atol=1e-10 * (1 + np.max(np.abs(rc))))
    for e in (e_old, e_upd, e_new):
        e.close()
    ac.close(), fresh.close()


# ---- 8. stream capture ---------------------------------------------------------------------------------------------------------
def test_stream_capture_replays_the_eager_call():
    """the call holds no mutable plan or policy state: captured into a torch.cuda.graph (default hardware queues, no runtime
    setting touched), replayed twice from the same start state, both replays equal the eager result"""
    torch = _torch()
    from oracle import oracle as O

    B, T = 8192, 12
    p = copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"])
    p.update(integrator="rk4", noise=True, noise_percentage=0.002)
    env = _make(p, B, seed=6)
    spec = env.spec
    env.reset()
    ac = make_ac(spec, env.obs_soa.cpu().numpy(), (16,), seed=29)
    ha, hc = ac.actor.handle(env.device), ac.critic.handle(env.device)
    sg = (C.c_double * spec.na)(*ac.sigma)
    x0, o0 = env.x.clone(), env.obs_soa.clone()
    f64, dev = torch.float64, env.device
    a_seq, u_seq = (torch.zeros((T + 1, spec.na, B), dtype=f64, device=dev) for _ in range(2))
    lp, val = (torch.zeros((T + 1, B), dtype=f64, device=dev) for _ in range(2))
    o_seq = torch.zeros((T, spec.nobs, B), dtype=f64, device=dev)
    r_seq = torch.zeros((T, B), dtype=f64, device=dev)
    seed = env._episode_seed()

    def call(stream):
        return env._lib.pcg_rollout_actor(env._plan, env._bufp, ha, hc, sg, 0, T, a_seq.data_ptr(), spec.na * B, B,
                                          u_seq.data_ptr(), spec.na * B, B, lp.data_ptr(), B, val.data_ptr(), B, o_seq.data_ptr(),
                                          spec.nobs * B, B, r_seq.data_ptr(), B, 1, seed, stream)

    outs = (a_seq, u_seq, lp, val, o_seq, r_seq)
    assert call(torch.cuda.current_stream(dev).cuda_stream) == 0
    torch.cuda.synchronize()
    eager = [t.clone() for t in outs + (env.x, env.obs_soa, env.rew, env.done)]
    assert float(u_seq.std()) > 0 and float(val.std()) > 0
    g = torch.cuda.CUDAGraph()
    env.x.copy_(x0), env.obs_soa.copy_(o0)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        rc = call(torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    for rep in range(2):
        for t in outs:
            t.fill_(-3.0)
        env.x.copy_(x0), env.obs_soa.copy_(o0)
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs + (env.x, env.obs_soa, env.rew, env.done), eager):
            assert torch.equal(got, want), f"replay {rep} differs from the eager call"
    orc = O.OracleEnv(spec, B, seed=6)
    orc.reset()
    orc.step(eager[0][0].cpu().numpy())
    _, r1, _ = orc.step(eager[0][1].cpu().numpy())
    assert np.allclose(eager[5][1].cpu().numpy(), r1, rtol=1e-6, atol=1e-8 * (1 + np.max(np.abs(r1))))
    env.close(), ac.close()
