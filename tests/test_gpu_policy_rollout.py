"""The fused closed-loop rollout with an on-device MLP policy (pcg_rollout_policy, pcg_rollout_policy.hpp) against what it
replaces: the reference's loop  a = policy.predict(obs); obs, r, done = env.step(a)  (policy_evaluation.py:86-128).

Every comparison is TEACHER-FORCED, so that the amplification of a closed loop never enters a tolerance:

  action check    every recorded policy output against MLPPolicy evaluated on the host in np.longdouble on the kernel's OWN
                  recorded observation, inside an a-priori running error bound (gamma_n |W| |x| per layer, propagated, plus
                  the measured error of the device tanh + 1 ulp);
  dynamics check  the recorded actions replayed through the existing open-loop rollout (general kernel) from the same reset:
                  observations, rewards and final state BITWISE equal;
  oracle check    the same rollout taken one call per step (bitwise equal to the one call), every step against the oracle
                  from the common start state with the recorded action: every lane within 1e-12 of max(|x|, 1);
  public path     collect_rollouts(env, policy=MLPPolicy) against the per-step path, within 8 x the spread of two per-step runs
                  that differ only in the order of the hidden units (+ 1e-13);
  unsupported     constraint rows / per-env parameters / another integrator: PCG_E_UNSUPPORTED, collect_rollouts still works;
  bad arguments   both entry points: the status of each refused call and the order of the checks, nothing launched or written;
  stream capture  one call inside torch.cuda.graph, replayed twice, equal to the eager call.

Measured figures are printed and, when PCG_RECORD_DIR names a directory, appended to policy_rollout_test.txt there (the copy
under profiles/r7/policy_rollout.txt).
First run on an MI355X: device tanh 0.846 ulp; action error at most 0.54 x its running bound; state against the oracle at most
1.8e-14; fused against per-step 0.95-1.2 x the spread of two per-step runs (3e-14 cstr, 7e-16 four_tank).
"""
import copy

import numpy as np
import pytest

import scenarios as SC
from helpers import (CASE_KEYS, LD, PRE_MAX, SHAPES, UNSUPPORTED_PLANS, _case_params, _launched, _make, _perm_hidden, _spread_x0,
                     _torch, host_reference, make_policy, tanh_k)
from helpers import _record as _record_to

pytestmark = pytest.mark.gpu


def _record(line):
    _record_to("policy_rollout_test.txt", line)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("integ", ["rk4", "cv8"])
@pytest.mark.parametrize("key", CASE_KEYS)
def test_policy_rollout(key, integ, shape):
    """every model x {RK4, CV8} x policy shape.  The models' first scenarios bring the feature cases with them: four_tank and
    the extraction columns normalise the action, crystallization integrates action increments (a_delta, quirk Q1),
    cstr_raw takes physical observations and actions; cstr_noise adds observation noise."""
    torch = _torch()
    from oracle import oracle as O

    B, T = 200, 6
    p = _spread_x0(_case_params(key, integ))
    e_one, e_chain = (_make(p, B, seed=9) for _ in range(2))
    e_open = _make(p, B, seed=9, variant=1)  # PCG_OPT_VARIANT 1: the general kernels
    spec = e_one.spec
    assert spec.integrator == integ and not spec.ncon and not spec.nunc and spec.x0_unc is not None
    if key == "crystallization":
        assert spec.a_delta and spec.normalise_a
    if key == "four_tank":
        assert spec.normalise_a
    if key == "cstr_noise":
        assert spec.noise
    if key == "cstr_raw":
        assert not spec.normalise_a and not spec.normalise_o
    for e in (e_one, e_chain, e_open):
        e.reset()
    obs0 = e_one.obs_soa.cpu().numpy().copy()
    x0 = e_one.x.cpu().numpy().copy()
    pol = make_policy(spec, obs0, SHAPES[shape], seed=17)
    assert pol.validate() == 0
    k = tanh_k()

    # ---- the fused closed loop: one call ----
    a_seq, obs_seq, rew_seq = e_one.rollout_policy(pol, T, collect_obs=True, collect_rew=True, record_next_action=True)
    torch.cuda.synchronize()
    a_np, o_np = a_seq.cpu().numpy(), obs_seq.cpu().numpy()
    assert a_np.shape == (T + 1, spec.na, B) and o_np.shape == (T, spec.nobs, B)
    assert np.isfinite(a_np).all() and np.isfinite(o_np).all() and not e_one.status.any()
    assert torch.equal(e_one.obs_soa, obs_seq[T - 1]) and torch.equal(e_one.rew, rew_seq[T - 1])  # io-> hold the last step
    assert e_one.t == T

    # ---- 1. action check: recorded a[s] against the host evaluation on the kernel's own obs[s-1] ----
    worst, pre = 0.0, 0.0
    for s in range(T + 1):
        o_in = obs0 if s == 0 else o_np[s - 1]
        ref, bound, pm = host_reference(pol, o_in, k + 1.0)
        pre = max(pre, pm)
        diff = np.abs(a_np[s].astype(LD) - ref).astype(np.float64)
        assert np.all(diff <= bound), (f"step {s}: policy output off by {np.max(diff):.3e}, {np.max(diff / np.maximum(bound, 1e-300)):.2f} x "
                                       f"the running bound ({np.max(bound):.3e})")
        worst = max(worst, float(np.max(diff / np.maximum(bound, 1e-300))))
    assert pre <= PRE_MAX, f"pre-activations up to {pre:.1f}: outside the grid the tanh error was measured on"
    inside = float(np.mean((a_np > pol.out_low) & (a_np < pol.out_high)))
    assert inside >= 0.25, f"only {inside:.2f} of the recorded actions lie strictly inside the clip box"
    assert np.std(a_np) > 0

    # ---- 2. dynamics check: the recorded actions through the open-loop rollout, general kernel: bitwise ----
    assert np.array_equal(e_open.x.cpu().numpy(), x0)
    oq, rq = e_open.rollout(a_seq[:T].contiguous(), collect_obs=True, collect_rew=True)
    torch.cuda.synchronize()
    assert torch.equal(oq, obs_seq), "observations differ from the open-loop replay of the recorded actions"
    assert torch.equal(rq, rew_seq), "rewards differ from the open-loop replay"
    assert torch.equal(e_open.x, e_one.x), "final state differs from the open-loop replay"
    assert torch.equal(e_open.done, e_one.done) and torch.equal(e_open.status, e_one.status)
    if spec.a_delta:
        assert torch.equal(e_open.a_save_t, e_one.a_save_t)

    # ---- 3. oracle check: one call per step == the one call, bitwise; every step against the oracle, every lane ----
    orc = O.OracleEnv(spec, B, seed=9)
    orc.reset()
    assert np.allclose(orc.x, x0, rtol=1e-14, atol=0)
    worst_x = 0.0
    for s in range(T):
        x_before = e_chain.x.cpu().numpy().copy()
        a1, o1, r1 = e_chain.rollout_policy(pol, 1, collect_obs=True, collect_rew=True, record_next_action=(s == T - 1))
        torch.cuda.synchronize()
        assert torch.equal(a1[0], a_seq[s]) and torch.equal(o1[0], obs_seq[s]) and torch.equal(r1[0], rew_seq[s]), f"chained call {s}"
        if s == T - 1:
            assert torch.equal(a1[1], a_seq[T])
        orc.x[:] = x_before  # teacher-forced: common start state, the recorded action
        oc, rc, dc = orc.step(a_np[s])
        xg = e_chain.x.cpu().numpy()
        assert np.isfinite(orc.x).all()
        err = float(np.max(np.abs(xg - orc.x) / np.maximum(np.abs(orc.x), 1.0)))
        worst_x = max(worst_x, err)
        assert err <= 1e-12, f"step {s}: state {err:.3e} from the oracle (relative to max(|x|, 1))"
        assert np.array_equal(e_chain.done.cpu().numpy(), dc)
        if not spec.noise:  # (with noise the observation carries the noise twin's fp32 variates: compared through x and the reward)
            assert np.allclose(o1[0].cpu().numpy(), oc, rtol=1e-10, atol=1e-11)
        assert np.allclose(r1[0].cpu().numpy(), rc, rtol=1e-9, atol=1e-10 * (1 + np.max(np.abs(rc))))
    assert torch.equal(e_chain.x, e_one.x)
    _record(f"case {key}-{integ}-{shape}: action error <= {worst:.3f} x bound, |pre-activation| <= {pre:.2f}, "
            f"{inside:.2f} of the actions inside the box, state vs oracle {worst_x:.2e}")
    for e in (e_one, e_chain, e_open):
        e.close()
    pol.close()


def _dist(a, b):
    """largest difference over x / u / r, each relative to max(1, largest entry of the reference array)"""
    d = 0.0
    for k in ("x", "u", "r"):
        ref = b[k].cpu().numpy()
        d = max(d, float(np.max(np.abs(a[k].cpu().numpy() - ref)) / max(1.0, float(np.max(np.abs(ref))))))
    return d


@pytest.mark.parametrize("shape", ["1x16", "2x64"])
@pytest.mark.parametrize("scen,integ", [("cstr_canonical", "rk4"), ("four_tank_canonical", "cv8")])
def test_collect_rollouts_takes_the_fused_call(scen, integ, shape):
    torch = _torch()
    from oracle import oracle as O
    from pcgym_amd import collect_rollouts

    B = 4096
    p = copy.deepcopy(SC.scenarios()[scen]["env_params"])
    p.update(integrator=integ)
    envs = [_make(_spread_x0(p, 0.01), B, seed=4) for _ in range(3)]  # (cstr: T0 <= 334 K, below the ignition branch)
    spec = envs[0].spec
    N = spec.N
    for e in envs:
        e.reset()  # (collect_rollouts resets again: the three envs stay in the same RNG epoch)
    pol = make_policy(spec, envs[0].obs_soa.cpu().numpy(), SHAPES[shape], seed=23)
    pol2 = _perm_hidden(pol, 5)
    fused = collect_rollouts(envs[0], policy=pol)
    torch.cuda.synchronize()
    assert _launched(envs[0]._lib, "rollout_policy_kernel"), "collect_rollouts did not take the fused closed-loop call"
    ref = collect_rollouts(envs[1], policy=lambda o: pol(o))
    ref2 = collect_rollouts(envs[2], policy=lambda o: pol2(o))
    torch.cuda.synchronize()
    assert fused["x"].shape == (spec.nobs, N, B) and fused["u"].shape == (spec.na, N, B) and fused["r"].shape == (1, N, B)
    for k in ("x", "u", "r"):
        assert fused[k].shape == ref[k].shape and bool(torch.isfinite(fused[k]).all())
    # u in physical units (the action box), its last column the action proposed for the final observation
    u = fused["u"].cpu().numpy()
    assert np.all(u >= spec.a_low[:, None, None] - 1e-12) and np.all(u <= spec.a_high[:, None, None] + 1e-12)
    x_last = fused["x"][:, N - 1].t()  # physical units -> the policy's (normalised) input
    o_last = envs[0].obs
    a_next = pol(o_last)
    if spec.normalise_a:
        a_next = (a_next + 1) * torch.as_tensor(spec.a_high - spec.a_low, device=a_next.device) / 2 + torch.as_tensor(spec.a_low, device=a_next.device)
    assert torch.allclose(fused["u"][:, N - 1].t(), a_next, rtol=1e-12, atol=1e-12), "u[:, N-1] is not policy(final observation)"
    assert x_last.shape == (B, spec.nobs) and torch.equal(fused["r"][0, 0], torch.zeros(B, dtype=torch.float64, device=x_last.device))
    spread, dist = _dist(ref2, ref), _dist(fused, ref)
    _record(f"collect_rollouts {scen}-{integ}-{shape} B={B} N={N}: per-step spread under hidden-unit permutation {spread:.3e}, "
            f"fused vs per-step {dist:.3e} ({dist / max(spread, 1e-300):.2f} x)")
    assert spread > 0, "the permuted run is bitwise the reference run: the spread measures nothing"
    assert dist <= 8 * spread + 1e-13, f"fused result {dist:.3e} from the per-step path; two per-step runs differ by {spread:.3e}"
    # the oracle, teacher-forced on the fused trajectory's first steps (physical u -> policy space)
    orc = O.OracleEnv(spec, 64, seed=4)
    orc.reset(), orc.reset()
    a_hm = ((spec.a_high - spec.a_low) / 2, (spec.a_high + spec.a_low) / 2)
    for i in range(3):
        a = u[:, i, :64]
        if spec.normalise_a:
            a = (a - a_hm[1][:, None]) / a_hm[0][:, None]
        _, rc, _ = orc.step(a)
    assert np.allclose(fused["r"][0, 3, :64].cpu().numpy(), rc, rtol=1e-6, atol=1e-8 * (1 + np.max(np.abs(rc))))
    for e in envs:
        e.close()
    pol.close(), pol2.close()


UNSUPPORTED = UNSUPPORTED_PLANS


@pytest.mark.parametrize("what", list(UNSUPPORTED))
def test_unsupported_plans_are_refused_and_still_collect(what):
    torch = _torch()
    from oracle import oracle as O
    from pcgym_amd import MLPPolicy, collect_rollouts
    from pcgym_amd import _abi as abi

    scen, over = UNSUPPORTED[what]
    p = copy.deepcopy(SC.scenarios()[scen]["env_params"])
    p.update(over)
    B = 256
    env, env2 = _make(p, B, seed=2), _make(p, B, seed=2)
    spec = env.spec
    env.reset(), env2.reset()
    pol = make_policy(spec, env.obs_soa.cpu().numpy(), (16,), seed=3)
    x_before, o_before = env.x.clone(), env.obs_soa.clone()
    a_out = torch.full((3, spec.na, B), -7.0, dtype=torch.float64, device=env.device)
    rc = env._lib.pcg_rollout_policy(env._plan, env._bufp, pol.handle(env.device), 0, 2, a_out.data_ptr(), spec.na * B, B,
                                     None, 0, 0, None, 0, 1, 1, None)
    torch.cuda.synchronize()
    assert rc == abi.PCG_E_UNSUPPORTED
    assert torch.equal(env.x, x_before) and torch.equal(env.obs_soa, o_before) and bool((a_out == -7.0).all()), "something was launched"
    with pytest.raises(Exception, match="-6"):
        env.rollout_policy(pol, 2)
    # the public path falls back to the per-step loop, silently
    d1 = collect_rollouts(env, policy=pol)
    d2 = collect_rollouts(env2, policy=lambda o: pol(o))
    torch.cuda.synchronize()
    for k in d2:
        assert torch.equal(d1[k], d2[k]), k
    assert d1["x"].shape == (spec.nobs, spec.N, B)
    orc = O.OracleEnv(spec, B, seed=2)  # ... whose first step is the oracle's
    orc.reset(), orc.reset()
    u0 = d1["u"][:, 0].cpu().numpy()
    a0 = (u0 - ((spec.a_high + spec.a_low) / 2)[:, None]) / ((spec.a_high - spec.a_low) / 2)[:, None] if spec.normalise_a else u0
    _, r0, _ = orc.step(a0)
    assert np.allclose(d1["r"][0, 1].cpu().numpy(), r0, rtol=1e-6, atol=1e-8 * (1 + np.max(np.abs(r0))))
    # a size mismatch on a plan that qualifies is PCG_E_DIM
    p_ok = copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"])
    p_ok.update(integrator="rk4")
    env3 = _make(p_ok, B, seed=2)
    env3.reset()
    wrong = MLPPolicy([np.zeros((1, env3.spec.nobs + 1))], [np.zeros(1)])
    rc = env3._lib.pcg_rollout_policy(env3._plan, env3._bufp, wrong.handle(env3.device), 0, 2, None, 0, 0, None, 0, 0, None, 0, 0, 1, None)
    assert rc == abi.PCG_E_DIM
    wrong.close()
    for e in (env, env2, env3):
        e.close()
    pol.close()


@pytest.mark.parametrize("entry", ["policy", "actor"])
def test_bad_arguments_are_refused_before_any_launch(entry):
    """the argument checks both entry points share, by return code and in their order of precedence (pcg_abi_policy.hip:
    closed_loop_open, the entry point's own checks, closed_loop_launch).  First a valid call as the positive control; then
    every bad call returns its code, leaves env.x, env.obs_soa and every output buffer as they were, and launches no
    closed-loop kernel.  Every call here is refused by host validation: nothing reaches the device."""
    torch = _torch()
    import ctypes as C

    from pcgym_amd import MLPPolicy
    from pcgym_amd import _abi as abi

    B, T, INT_MAX = 256, 2, 2 ** 31 - 1
    kernel = f"rollout_{entry}_kernel"

    class Case:
        def __init__(self, scen):
            p = copy.deepcopy(SC.scenarios()[scen]["env_params"])
            p.update(integrator="rk4")
            self.env = env = _make(p, B, seed=2)
            env.reset()
            s = self.spec = env.spec
            shapes = {"a": (T + 1, s.na, B), "obs": (T, s.nobs, B), "rew": (T, B)}
            if entry == "actor":
                shapes.update(u=(T + 1, s.na, B), logp=(T + 1, B), val=(T + 1, B))
            self.bufs = {n: torch.full(shp, -7.0, dtype=torch.float64, device=env.device) for n, shp in shapes.items()}
            self.x0, self.o0 = env.x.clone(), env.obs_soa.clone()

        def restore(self):
            self.env.x.copy_(self.x0), self.env.obs_soa.copy_(self.o0)
            for b in self.bufs.values():
                b.fill_(-7.0)
            torch.cuda.synchronize()
            self.env._lib.pcg_coverage_names(None, 0, 1)

        def call(self, pol_h, critic_h=None, sigma=None, t0=0, T=T, a_cs=B, o_cs=B, u_cs=B):
            env, s, b = self.env, self.spec, self.bufs
            if entry == "policy":
                rc = env._lib.pcg_rollout_policy(env._plan, env._bufp, pol_h, t0, T, b["a"].data_ptr(), s.na * B, a_cs,
                                                 b["obs"].data_ptr(), s.nobs * B, o_cs, b["rew"].data_ptr(), B, 1, 1, None)
            else:
                sg = (C.c_double * len(sigma))(*sigma) if sigma is not None else None
                rc = env._lib.pcg_rollout_actor(env._plan, env._bufp, pol_h, critic_h, sg, t0, T, b["a"].data_ptr(), s.na * B, a_cs,
                                                b["u"].data_ptr(), s.na * B, u_cs, b["logp"].data_ptr(), B, b["val"].data_ptr(), B,
                                                b["obs"].data_ptr(), s.nobs * B, o_cs, b["rew"].data_ptr(), B, 1, 1, None)
            torch.cuda.synchronize()
            return rc

        def refused(self, what, want, *args, **kw):
            rc = self.call(*args, **kw)
            assert rc == want, f"{what}: status {rc}, not {want}"
            assert not _launched(self.env._lib, "rollout_policy_kernel") and not _launched(self.env._lib, "rollout_actor_kernel"), \
                f"{what}: a refused call launched a closed-loop kernel"
            assert torch.equal(self.env.x, self.x0) and torch.equal(self.env.obs_soa, self.o0), f"{what}: a refused call wrote the env"
            assert all(bool((b == -7.0).all()) for b in self.bufs.values()), f"{what}: a refused call wrote an output buffer"
            self.restore()

    ok = Case("cstr_canonical")
    spec, dev = ok.spec, ok.env.device
    pol = make_policy(spec, ok.o0.cpu().numpy(), (16,), seed=3)
    closing = [pol]
    h, hc, sigma = pol.handle(dev), None, None
    if entry == "actor":
        c = make_policy(spec, ok.o0.cpu().numpy(), (16,), seed=103)
        critic = MLPPolicy(c.weights[:-1] + [c.weights[-1][:1]], c.biases[:-1] + [c.biases[-1][:1]], activation=c.activation, out_map="none")
        closing += [c, critic]
        hc, sigma = critic.handle(dev), [0.25] * spec.na
    good = (h, hc, sigma)

    # ---- positive control: the valid call runs, writes every buffer, and is seen by the launch record ----
    ok.restore()
    assert ok.call(*good) == abi.PCG_OK
    assert _launched(ok.env._lib, kernel), "the valid call launched nothing"
    assert not torch.equal(ok.env.x, ok.x0) and not torch.equal(ok.env.obs_soa, ok.o0)
    for n, b in ok.bufs.items():
        assert bool((b != -7.0).all()), f"the valid call left part of {n} unwritten"
    ok.restore()

    # ---- the bad calls ----
    ok.refused("policy handle None", abi.PCG_E_NULL, None, hc, sigma)
    ok.refused("T = 0", abi.PCG_E_VALUE, *good, T=0)
    ok.refused("t0 = -1", abi.PCG_E_VALUE, *good, t0=-1)
    ok.refused("t0 + T past 2^31 - 1", abi.PCG_E_VALUE, *good, t0=INT_MAX - 1, T=2)
    ok.refused("action component stride B - 1", abi.PCG_E_DIM, *good, a_cs=B - 1)
    ok.refused("observation component stride B - 1", abi.PCG_E_DIM, *good, o_cs=B - 1)
    if entry == "actor":
        ok.refused("sample component stride B - 1", abi.PCG_E_DIM, *good, u_cs=B - 1)

    # ---- precedence ----
    wrong = MLPPolicy([np.zeros((spec.na, spec.nobs + 1))], [np.zeros(spec.na)])
    closing.append(wrong)
    cons = Case("cstr_cons_pen_norm")
    assert cons.spec.ncon > 0 and (cons.spec.nobs, cons.spec.na) == (spec.nobs, spec.na)
    cons.restore()
    cons.refused("wrong-size policy on a plan with constraint rows", abi.PCG_E_UNSUPPORTED, wrong.handle(dev), hc, sigma)
    ok.refused("wrong-size policy and T = 0", abi.PCG_E_DIM, wrong.handle(dev), hc, sigma, T=0)
    if entry == "actor":
        sq = MLPPolicy(pol.weights, pol.biases, activation="tanh", out_map="tanh")
        closing.append(sq)
        ok.refused("tanh-mapped actor without sigma", abi.PCG_E_UNSUPPORTED, sq.handle(dev), hc, None)
    ok.env.close(), cons.env.close()
    for q in closing:
        q.close()


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
    pol = make_policy(spec, env.obs_soa.cpu().numpy(), (16,), seed=29)
    h = pol.handle(env.device)
    x0, o0 = env.x.clone(), env.obs_soa.clone()
    f64, dev = torch.float64, env.device
    a_seq = torch.zeros((T + 1, spec.na, B), dtype=f64, device=dev)
    o_seq = torch.zeros((T, spec.nobs, B), dtype=f64, device=dev)
    r_seq = torch.zeros((T, B), dtype=f64, device=dev)
    seed = env._episode_seed()

    def call(stream):
        return env._lib.pcg_rollout_policy(env._plan, env._bufp, h, 0, T, a_seq.data_ptr(), spec.na * B, B, o_seq.data_ptr(),
                                           spec.nobs * B, B, r_seq.data_ptr(), B, 1, seed, stream)

    assert call(torch.cuda.current_stream(dev).cuda_stream) == 0
    torch.cuda.synchronize()
    eager = [t.clone() for t in (a_seq, o_seq, r_seq, env.x, env.obs_soa, env.rew, env.done)]
    assert float(a_seq.std()) > 0
    g = torch.cuda.CUDAGraph()
    env.x.copy_(x0), env.obs_soa.copy_(o0)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        rc = call(torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    for rep in range(2):
        for t in (a_seq, o_seq, r_seq):
            t.fill_(-3.0)
        env.x.copy_(x0), env.obs_soa.copy_(o0)
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip((a_seq, o_seq, r_seq, env.x, env.obs_soa, env.rew, env.done), eager):
            assert torch.equal(got, want), f"replay {rep} differs from the eager call"
    # (the eager call against the oracle: first step, recorded action)
    orc = O.OracleEnv(spec, B, seed=6)
    orc.reset()
    orc.step(eager[0][0].cpu().numpy())
    _, r1, _ = orc.step(eager[0][1].cpu().numpy())
    assert np.allclose(eager[2][1].cpu().numpy(), r1, rtol=1e-6, atol=1e-8 * (1 + np.max(np.abs(r1))))
    env.close(), pol.close()
