"""GPU: the fused closed-loop rollouts (pcg_rollout_policy, pcg_rollout_actor) on plans with run-time compiled code -- a
user model (PCG_MODEL_USER) or a reward expression on a built-in model.  Such a plan runs rollout_policy_kernel /
rollout_actor_kernel from a SECOND run-time compiled module, built at the plan's first closed-loop call or by
pcg_plan_prepare_closed_loop (pcg_abi_jit.hip: jit_closed_loop), never at pcg_plan_create.

Every comparison is teacher-forced, as in test_gpu_policy_rollout.py: the policy half is checked on the kernel's own
recorded observations, the env half from the recorded actions, so closed-loop amplification stays out of the tolerances.
B = 200 leaves a tail wave, T = 6.

  replay check   the recorded actions through env.rollout on a twin env (the step module's open-loop rollout_kernel)."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import scenarios as SC
from helpers import (LD, PRE_MAX, SHAPES, U, _launch_names, _make, _perm_hidden, _spread_x0, _torch, host_reference, make_policy,
                     tanh_k, tight_for)
from test_gpu_actor_rollout import logp_numpy, make_ac, raw_twin
from test_gpu_user_model import CSTR_BY_HAND, _chemostat_params

pytestmark = pytest.mark.gpu

B, T = 200, 6


def _chemostat(integ, **kw):
    """the Monod chemostat of test_gpu_user_model.py without its constraint: rk4 with 6 substeps, or cv8"""
    p = _chemostat_params(integrator=integ, **kw)
    if integ == "rk4":
        p["substeps"] = 6
    return p


def _size_limit_params(integ="rk4"):
    """the model of test_user_model_at_the_size_limits: 24 states, 5 inputs, 4 disturbance inputs, 64 parameters"""
    from pcgym_amd import _abi as abi

    nx, na, ndm, npar = abi.PCG_MAX_NX, abi.PCG_MAX_NA, abi.PCG_MAX_NDM, abi.PCG_MAX_USER_PARAMS
    rng = np.random.default_rng(12)
    states, inputs, dist = [f"s{i}" for i in range(nx)], [f"v{j}" for j in range(na)], [f"w{j}" for j in range(ndm)]
    params = {f"k{q}": float(rng.uniform(0.2, 1.0)) for q in range(npar - ndm)}
    params.update({d: 0.1 * (j + 1) for j, d in enumerate(dist)})
    pk = list(params)
    rhs = []
    for i in range(nx):
        a, b, c = pk[i % (npar - ndm)], pk[(2 * i + 7) % (npar - ndm)], pk[(3 * i + 11) % (npar - ndm)]
        rhs.append(f"-{a}*s{i} + 0.3*{b}*(s{(i + 1) % nx} - s{i}) + 0.1*{c}*v{i % na}*s{(i + 5) % nx}/(1.0 + s{i}*s{i}) + {dist[i % ndm]}")
    cm = {"states": states, "inputs": inputs, "disturbances": dist, "parameters": params, "rhs": rhs}
    N = 12
    return {"custom_model": cm, "N": N, "tsim": 6.0, "x0": np.concatenate([rng.uniform(0.2, 1.0, nx), [0.5]]),
            "SP": {"s3": [0.5] * N}, "a_space": {"low": -np.ones(na), "high": np.ones(na)},
            "o_space": {"low": -5 * np.ones(nx + 1), "high": 5 * np.ones(nx + 1)},
            "disturbances": {d: 0.1 * (j + 1) + 0.05 * np.sin(np.arange(N) + j) for j, d in enumerate(dist)},
            "disturbance_bounds": {"low": -np.ones(ndm), "high": np.ones(ndm)}, "integrator": integ,
            "normalise_a": False, "normalise_o": True}


def _jit_closed_loop_launches(lib, kernel):
    """the run-time compiled instantiations of `kernel` in the launch record of this test"""
    return [n for n in _launch_names(lib) if n.startswith("jit:") and kernel in n]


def _gap(got, want):
    return float((got - want).abs().max()) if got.numel() else 0.0


def _replay(e_one, e_open, a_seq, obs_seq, rew_seq, bitwise, tol=None, what=""):
    """check (b): the recorded applied actions through the twin env's open-loop rollout give the closed loop's observations,
    rewards and final state -- bitwise, or within tol = ((obs rtol, atol), (rew rtol, atol), (x rtol, atol))"""
    torch = _torch()
    oq, rq = e_open.rollout(a_seq[:T].contiguous(), collect_obs=True, collect_rew=True)
    torch.cuda.synchronize()
    print(f"replay {what}: largest differences obs {_gap(oq, obs_seq):.3e}, rew {_gap(rq, rew_seq):.3e}, x {_gap(e_open.x, e_one.x):.3e}")
    if bitwise:
        assert torch.equal(oq, obs_seq), "observations differ from the open-loop replay of the recorded actions"
        assert torch.equal(rq, rew_seq), "rewards differ from the open-loop replay"
        assert torch.equal(e_open.x, e_one.x), "final state differs from the open-loop replay"
    else:
        (ro, ao), (rr, ar), (rx, ax) = tol
        assert torch.allclose(oq, obs_seq, rtol=ro, atol=ao) and torch.allclose(rq, rew_seq, rtol=rr, atol=ar)
        assert torch.allclose(e_open.x, e_one.x, rtol=rx, atol=ax)
    assert torch.equal(e_open.done, e_one.done) and torch.equal(e_open.status, e_one.status)


def _action_check(pol, obs0, o_np, a_np, k):
    """check (a): every recorded action inside host_reference's running bound on the kernel's own recorded observation"""
    pre = 0.0
    for s in range(a_np.shape[0]):
        o_in = obs0 if s == 0 else o_np[s - 1]
        ref, bound, pm = host_reference(pol, o_in, k + 1.0)
        pre = max(pre, pm)
        diff = np.abs(a_np[s].astype(LD) - ref).astype(np.float64)
        assert np.all(diff <= bound), (f"step {s}: policy output off by {np.max(diff):.3e}, "
                                       f"{np.max(diff / np.maximum(bound, 1e-300)):.2f} x the running bound ({np.max(bound):.3e})")
    assert pre <= PRE_MAX, f"pre-activations up to {pre:.1f}: outside the grid the tanh error was measured on"
    assert np.std(a_np) > 0


# ---- 1. user model, policy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("integ", ["rk4", "cv8"])
def test_policy_rollout_of_a_user_model(integ, shape):
    """The chemostat under rk4 (6 substeps) and cv8, the three policy shapes.  The replay check holds BITWISE: the closed-loop
    module's env step and the step module's open-loop rollout kernel are the same code, compiled twice."""
    torch = _torch()
    from oracle import oracle as O

    p = _spread_x0(_chemostat(integ))
    e_one, e_chain, e_open = (_make(p, B, seed=9) for _ in range(3))
    spec = e_one.spec
    assert spec.model.model_id == 17 and spec.integrator == integ and not spec.ncon and not spec.nunc and spec.x0_unc is not None
    O.register_user_rhs(spec)
    for e in (e_one, e_chain, e_open):
        e.reset()
    obs0, x0 = e_one.obs_soa.cpu().numpy().copy(), e_one.x.cpu().numpy().copy()
    assert np.std(x0, axis=1).min() > 0
    pol = make_policy(spec, obs0, SHAPES[shape], seed=17)
    assert pol.validate() == 0
    k = tanh_k()

    a_seq, obs_seq, rew_seq = e_one.rollout_policy(pol, T, collect_obs=True, collect_rew=True, record_next_action=True)
    torch.cuda.synchronize()
    assert _jit_closed_loop_launches(e_one._lib, "rollout_policy_kernel"), "no run-time compiled closed-loop kernel was launched"
    a_np, o_np = a_seq.cpu().numpy(), obs_seq.cpu().numpy()
    assert a_np.shape == (T + 1, spec.na, B) and o_np.shape == (T, spec.nobs, B)
    assert np.isfinite(a_np).all() and np.isfinite(o_np).all() and not e_one.status.any()
    assert torch.equal(e_one.obs_soa, obs_seq[T - 1]) and torch.equal(e_one.rew, rew_seq[T - 1]) and e_one.t == T
    _action_check(pol, obs0, o_np, a_np, k)                                                 # (a)
    inside = float(np.mean((a_np > pol.out_low) & (a_np < pol.out_high)))
    assert inside >= 0.25, f"only {inside:.2f} of the recorded actions lie strictly inside the clip box"
    _replay(e_one, e_open, a_seq, obs_seq, rew_seq, bitwise=True, what=f"chemostat-{integ}-{shape}")   # (b)

    orc = O.OracleEnv(spec, B, seed=9)
    orc.reset()
    assert np.allclose(orc.x, x0, rtol=1e-14, atol=0)
    for s in range(T):                                                                      # (c), (d)
        x_before = e_chain.x.cpu().numpy().copy()
        a1, o1, r1 = e_chain.rollout_policy(pol, 1, collect_obs=True, collect_rew=True, record_next_action=(s == T - 1))
        torch.cuda.synchronize()
        assert torch.equal(a1[0], a_seq[s]) and torch.equal(o1[0], obs_seq[s]) and torch.equal(r1[0], rew_seq[s]), f"chained call {s}"
        if s == T - 1:
            assert torch.equal(a1[1], a_seq[T])
        orc.x[:] = x_before  # teacher-forced: common start state, the recorded action
        oc, rc, dc = orc.step(a_np[s])
        xg = e_chain.x.cpu().numpy()
        # (test_user_model_env_steps_vs_oracle's bars)
        assert np.max(np.abs(xg - orc.x) / np.maximum(np.abs(orc.x), 1e-3)) <= 1e-11, s
        assert np.max(np.abs(o1[0].cpu().numpy() - oc) / np.maximum(np.abs(oc), 1e-3)) <= 1e-10, s
        assert np.max(np.abs(r1[0].cpu().numpy() - rc) / np.maximum(np.abs(rc), 1.0)) <= 1e-9, s
        assert np.array_equal(e_chain.done.cpu().numpy(), dc)
    assert torch.equal(e_chain.x, e_one.x) and e_chain.t == T
    for e in (e_one, e_chain, e_open):
        e.close()
    pol.close()


# ---- 2. the cstr written by hand against the built-in cstr ----------------------------------------------------------------------
@pytest.mark.parametrize("integ", ["rk4", "cv8"])
def test_hand_written_cstr_closes_the_loop_like_the_builtin(integ):
    """cstr_dist_both as in test_cstr_written_by_hand_equals_the_builtin_kernel_and_the_reference_recording: the user plan's
    closed loop, its recorded actions replayed open-loop on the BUILT-IN plan, at that test's tolerances"""
    torch = _torch()

    p = copy.deepcopy(SC.scenarios()["cstr_dist_both"]["env_params"])
    p.update(tight_for(p))
    p.update(integrator=integ)
    q = copy.deepcopy(p)
    q.pop("model")
    q["custom_model"] = copy.deepcopy(CSTR_BY_HAND)
    eb, eu = _make(_spread_x0(p, 0.01), B, seed=1), _make(_spread_x0(q, 0.01), B, seed=1)
    assert eu.spec.model.model_id == 17 and eb.spec.model.model_id == 0 and eu.spec.ndm == 2 and not eu.spec.ncon
    eb.reset(), eu.reset()
    assert torch.equal(eb.x, eu.x) and torch.equal(eb.obs_soa, eu.obs_soa)
    pol = make_policy(eu.spec, eu.obs_soa.cpu().numpy(), (16,), seed=3)
    a_seq, obs_seq, rew_seq = eu.rollout_policy(pol, T, collect_obs=True, collect_rew=True)
    torch.cuda.synchronize()
    assert _jit_closed_loop_launches(eu._lib, "rollout_policy_kernel")
    assert bool(torch.isfinite(obs_seq).all()) and float(a_seq.std()) > 0 and not eu.status.any()
    ob, rb = eb.rollout(a_seq.contiguous(), collect_obs=True, collect_rew=True)
    torch.cuda.synchronize()
    print(f"by-hand cstr {integ}: obs {_gap(ob, obs_seq):.3e}, rew {_gap(rb, rew_seq):.3e} from the built-in plan")
    assert torch.allclose(ob, obs_seq, rtol=1e-11, atol=1e-12)
    assert torch.allclose(rb, rew_seq, rtol=1e-9, atol=1e-11)
    eb.close(), eu.close(), pol.close()


# ---- 3. a reward expression on a built-in model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("head", ["policy", "actor"])
def test_reward_expression_plan_closes_the_loop(head):
    """cstr_expr_reward_q3 without its constraints (test_fused_rollout_with_a_reward_expression_matches_stepping's plan, under
    rk4): replay check at that test's tolerances (first run on an MI355X: no difference at all)"""
    torch = _torch()

    p = copy.deepcopy(SC.scenarios()["cstr_expr_reward_q3"]["env_params"])
    p.pop("constraints", None), p.pop("done_on_cons_vio", None), p.pop("r_penalty", None)
    p.update(integrator="rk4")  # (the scenario's own plan is the guarded tsit5g, which no closed-loop kernel takes)
    p = _spread_x0(p, 0.01)
    e_one, e_open = _make(p, B, seed=5), _make(p, B, seed=5)
    spec = e_one.spec
    assert spec.user_reward_src and spec.user_rhs_src is None and not spec.ncon
    e_one.reset(), e_open.reset()
    obs0 = e_one.obs_soa.cpu().numpy().copy()
    if head == "policy":
        net = make_policy(spec, obs0, (16,), seed=7)
        a_seq, obs_seq, rew_seq = e_one.rollout_policy(net, T, collect_obs=True, collect_rew=True)
        kernel = "rollout_policy_kernel"
    else:
        net = make_ac(spec, obs0, (16,), seed=7)
        out = e_one.rollout_actor(net, T, collect_obs=True, collect_rew=True)
        a_seq, obs_seq, rew_seq = out["a"], out["obs"], out["rew"]
        kernel = "rollout_actor_kernel"
    torch.cuda.synchronize()
    assert _jit_closed_loop_launches(e_one._lib, kernel)
    assert bool(torch.isfinite(obs_seq).all()) and bool(torch.isfinite(rew_seq).all()) and float(a_seq.std()) > 0
    assert float(rew_seq.std()) > 0 and not e_one.status.any()
    _replay(e_one, e_open, a_seq, obs_seq, rew_seq, bitwise=False, what=f"reward expression, {head}",
            tol=((1e-11, 1e-12), (1e-10, 1e-12), (1e-11, 1e-12)))
    e_one.close(), e_open.close(), net.close()


# ---- 4. actor-critic on the chemostat -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("critic", [True, False])
@pytest.mark.parametrize("out_map", ["clip", "none"])
def test_actor_rollout_of_a_user_model(out_map, critic):
    """the chemostat under rk4 with a Gaussian actor (clip / none) with and without a critic; replay check bitwise"""
    torch = _torch()

    p = _spread_x0(_chemostat("rk4"))
    e_one, e_open = _make(p, B, seed=9), _make(p, B, seed=9)
    spec = e_one.spec
    e_one.reset(), e_open.reset()
    obs0 = e_one.obs_soa.cpu().numpy().copy()
    ac = make_ac(spec, obs0, (16,), seed=17, out_map=out_map, sigma_scale=0.25 if out_map == "clip" else 0.02, critic=critic)
    raw, k = raw_twin(ac.actor), tanh_k()
    z = np.stack([e_one.policy_noise(t).cpu().numpy() for t in range(T + 1)])  # the draws of counters 0 .. T
    assert np.std(z) > 0.5
    out = e_one.rollout_actor(ac, T, collect_obs=True, collect_rew=True, record_next_action=True)
    torch.cuda.synchronize()
    assert _jit_closed_loop_launches(e_one._lib, "rollout_actor_kernel")
    a_np, u_np, lp_np, o_np = (out[n].cpu().numpy() for n in ("a", "u", "logp", "obs"))
    assert a_np.shape == u_np.shape == (T + 1, spec.na, B) and lp_np.shape == (T + 1, B) and o_np.shape == (T, spec.nobs, B)
    assert (out["val"] is not None) == critic
    assert np.isfinite(a_np).all() and np.isfinite(u_np).all() and np.isfinite(o_np).all() and not e_one.status.any()
    assert torch.equal(e_one.obs_soa, out["obs"][T - 1]) and torch.equal(e_one.rew, out["rew"][T - 1]) and e_one.t == T
    sig = ac.sigma[:, None]
    for s in range(T + 1):  # row T included: recorded ...
        o_in = obs0 if s == 0 else o_np[s - 1]
        mu, b_mu, pm = host_reference(raw, o_in, k + 1.0)
        assert pm <= PRE_MAX
        ref = mu + sig.astype(LD) * z[s].astype(LD)  # u = fma(sigma, z, mu): one more rounding
        diff = np.abs(u_np[s].astype(LD) - ref).astype(np.float64)
        assert np.all(diff <= b_mu + U * np.abs(u_np[s])), f"step {s}: sample off by {np.max(diff):.3e}"
        assert np.array_equal(lp_np[s], logp_numpy(ac, z[s])), f"step {s}: logp is not fma(-0.5, q, c0) of the same draws"
        if critic:
            vr, b_v, pm = host_reference(ac.critic, o_in, k + 1.0)
            assert pm <= PRE_MAX
            dv = np.abs(out["val"][s].cpu().numpy().astype(LD) - vr[0]).astype(np.float64)
            assert np.all(dv <= b_v[0]), f"step {s}: value off by {np.max(dv):.3e}"
    if out_map == "clip":
        lo, hi = ac.actor.out_low, ac.actor.out_high
        assert np.array_equal(a_np, np.clip(u_np, lo, hi)), "a is not clip(u) bitwise"
        assert 0.0 < float(np.mean((u_np < lo) | (u_np > hi))) < 1.0, "one branch of the clip was never taken"
    else:
        assert np.array_equal(a_np, u_np)
    # ... and not applied: T actions take the twin env to the same observations, rewards and final state
    _replay(e_one, e_open, out["a"], out["obs"], out["rew"], bitwise=True, what=f"chemostat actor {out_map} critic={critic}")
    e_one.close(), e_open.close(), ac.close(), raw.close()


# ---- 5. the public route --------------------------------------------------------------------------------------------------------
def _dist(a, b, keys):
    d = 0.0
    for n in keys:
        ref = b[n].cpu().numpy()
        d = max(d, float(np.max(np.abs(a[n].cpu().numpy() - ref)) / max(1.0, float(np.max(np.abs(ref))))))
    return d


def test_collect_rollouts_takes_the_fused_call_on_a_user_model():
    """test_collect_rollouts_takes_the_fused_call's criterion on the chemostat; two hidden layers of 64 units, so that the
    order of the hidden units changes the rounding of every output (the spread is asserted to be nonzero)"""
    torch = _torch()
    from pcgym_amd import collect_rollouts

    p = _spread_x0(_chemostat("rk4"), 0.01)
    envs = [_make(p, B, seed=4) for _ in range(3)]
    spec = envs[0].spec
    for e in envs:
        e.reset()  # (collect_rollouts resets again: the three envs stay in the same RNG epoch)
    pol = make_policy(spec, envs[0].obs_soa.cpu().numpy(), SHAPES["2x64"], seed=23)
    pol2 = _perm_hidden(pol, 5)
    fused = collect_rollouts(envs[0], policy=pol)
    torch.cuda.synchronize()
    assert _jit_closed_loop_launches(envs[0]._lib, "rollout_policy_kernel"), "collect_rollouts did not take the fused closed-loop call"
    ref = collect_rollouts(envs[1], policy=lambda o: pol(o))
    ref2 = collect_rollouts(envs[2], policy=lambda o: pol2(o))
    torch.cuda.synchronize()
    for n in ("x", "u", "r"):
        assert fused[n].shape == ref[n].shape and bool(torch.isfinite(fused[n]).all())
    assert fused["x"].shape == (spec.nobs, spec.N, B) and envs[0].t == spec.N - 1
    spread, dist = _dist(ref2, ref, ("x", "u", "r")), _dist(fused, ref, ("x", "u", "r"))
    print(f"collect_rollouts chemostat: per-step spread {spread:.3e}, fused vs per-step {dist:.3e}")
    assert spread > 0, "the permuted run is bitwise the reference run: the spread measures nothing"
    assert dist <= 8 * spread + 1e-13, f"fused result {dist:.3e} from the per-step path; two per-step runs differ by {spread:.3e}"
    for e in envs:
        e.close()
    pol.close(), pol2.close()


def test_collect_onpolicy_takes_the_fused_call_on_a_user_model():
    torch = _torch()
    from pcgym_amd import GaussianActorCritic, collect_onpolicy

    p = _spread_x0(_chemostat("rk4"), 0.01)
    envs = [_make(p, B, seed=4) for _ in range(4)]
    spec = envs[0].spec
    for e in envs:
        e.reset()
    ac = make_ac(spec, envs[0].obs_soa.cpu().numpy(), SHAPES["2x64"], seed=23, sigma_scale=0.1)
    ac2 = GaussianActorCritic(_perm_hidden(ac.actor, 5), ac.log_std, _perm_hidden(ac.critic, 6))
    fused = collect_onpolicy(envs[0], ac)
    torch.cuda.synchronize()
    assert _jit_closed_loop_launches(envs[0]._lib, "rollout_actor_kernel"), "collect_onpolicy did not take the fused call"
    forced = collect_onpolicy(envs[3], ac, fused=True)  # (raised ValueError before user models qualified)
    ref = collect_onpolicy(envs[1], ac, fused=False)
    ref2 = collect_onpolicy(envs[2], ac2, fused=False)
    torch.cuda.synchronize()
    keys = ("obs", "act", "logp", "val", "rew")
    for n in keys:
        assert torch.equal(forced[n], fused[n]) and bool(torch.isfinite(fused[n]).all()), n
    assert torch.equal(fused["logp"], ref["logp"])  # the same random bits through the same operations on both routes
    spread, dist = _dist(ref2, ref, keys), _dist(fused, ref, keys)
    print(f"collect_onpolicy chemostat: per-step spread {spread:.3e}, fused vs per-step {dist:.3e}")
    assert spread > 0, "the permuted run is bitwise the reference run: the spread measures nothing"
    assert dist <= 8 * spread + 1e-13, f"fused result {dist:.3e} from the per-step path; two per-step runs differ by {spread:.3e}"
    for e in envs:
        e.close()
    ac.close(), ac2.close()


# ---- 6. the size limits ---------------------------------------------------------------------------------------------------------
def test_policy_rollout_at_the_size_limits():
    """24 states, 4 disturbance inputs, 5 actions: a 29-entry observation in a 32-entry policy input, one wave per SIMD.
    The replay check holds bitwise here too."""
    torch = _torch()

    p = _spread_x0(_size_limit_params("rk4"))
    e_one, e_open = _make(p, B, seed=2), _make(p, B, seed=2)
    spec = e_one.spec
    assert (spec.nx, spec.na, spec.ndm) == (24, 5, 4) and spec.nobs == 29 and not spec.ncon
    e_one.reset(), e_open.reset()
    obs0 = e_one.obs_soa.cpu().numpy().copy()
    pol = make_policy(spec, obs0, SHAPES["1x16"], seed=17)
    a_seq, obs_seq, rew_seq = e_one.rollout_policy(pol, T, collect_obs=True, collect_rew=True, record_next_action=True)
    torch.cuda.synchronize()
    assert _jit_closed_loop_launches(e_one._lib, "rollout_policy_kernel")
    a_np, o_np = a_seq.cpu().numpy(), obs_seq.cpu().numpy()
    assert np.isfinite(a_np).all() and np.isfinite(o_np).all() and not e_one.status.any() and e_one.t == T
    _action_check(pol, obs0, o_np, a_np, tanh_k())
    _replay(e_one, e_open, a_seq, obs_seq, rew_seq, bitwise=True, what="size limits")
    e_one.close(), e_open.close(), pol.close()


# ---- 7. refusals: nothing launched, nothing written -----------------------------------------------------------------------------
def _cons_expr(x, u):
    return np.array([x[1] * x[1] - 0.65 * 0.65]).reshape(-1,)  # (not affine: traced into user_cons_src)


REFUSED = {
    # name: (env_params, VecEnv arguments, wrong-size policy, status of the calls, status of pcg_plan_prepare_closed_loop)
    "expression_constraint": (lambda: _chemostat("rk4", constraints=_cons_expr, done_on_cons_vio=False, r_penalty=True), {}, False, -6, -6),
    "dopri5": (lambda: _chemostat("dopri5", rtol=1e-6, atol=1e-8), {}, False, -6, -6),
    "rodas4": (lambda: _chemostat("rodas4", rtol=1e-6, atol=1e-8), {}, False, -6, -6),
    # (the plan itself qualifies in the next two: what is refused is the call)
    "per_env_counters": (lambda: _chemostat("rk4"), {"per_env_t": True}, False, -6, 0),
    "wrong_size_policy": (lambda: _chemostat("rk4"), {}, True, -3, 0),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refusals_launch_nothing(what):
    torch = _torch()
    from pcgym_amd import MLPPolicy
    from pcgym_amd import _abi as abi

    make_p, kw, wrong, want, want_prepare = REFUSED[what]
    assert (abi.PCG_E_UNSUPPORTED, abi.PCG_E_DIM, abi.PCG_OK) == (-6, -3, 0)
    env = _make(make_p(), B, seed=2, **kw)
    spec = env.spec
    if what == "expression_constraint":
        assert spec.user_cons_src and spec.ncon == 1
    env.reset()
    lib = env._lib
    pol = make_policy(spec, env.obs_soa.cpu().numpy(), (16,), seed=3)
    if wrong:
        pol.close()
        pol = MLPPolicy([np.zeros((spec.na, spec.nobs + 1))], [np.zeros(spec.na)])
    crit = MLPPolicy([np.zeros((1, spec.nobs))], [np.zeros(1)], out_map="none")
    x_before, o_before = env.x.clone(), env.obs_soa.clone()
    outs = [torch.full(shape, -7.0, dtype=torch.float64, device=env.device)
            for shape in ((3, spec.na, B), (3, spec.na, B), (3, B), (3, B), (2, spec.nobs, B), (2, B))]
    a_out, u_out, lp_out, v_out, o_out, r_out = outs
    h, hc = pol.handle(env.device), crit.handle(env.device)
    sg = (C.c_double * spec.na)(*([0.1] * spec.na))
    rc_pol = lib.pcg_rollout_policy(env._plan, env._bufp, h, 0, 2, a_out.data_ptr(), spec.na * B, B, o_out.data_ptr(), spec.nobs * B, B,
                                    r_out.data_ptr(), B, 1, 1, None)
    rc_act = lib.pcg_rollout_actor(env._plan, env._bufp, h, hc, sg, 0, 2, a_out.data_ptr(), spec.na * B, B, u_out.data_ptr(),
                                   spec.na * B, B, lp_out.data_ptr(), B, v_out.data_ptr(), B, o_out.data_ptr(), spec.nobs * B, B,
                                   r_out.data_ptr(), B, 1, 1, None)
    torch.cuda.synchronize()
    assert (rc_pol, rc_act) == (want, want)
    assert torch.equal(env.x, x_before) and torch.equal(env.obs_soa, o_before), "the env state changed"
    assert all(bool((t == -7.0).all()) for t in outs), "something was written"
    assert not _jit_closed_loop_launches(lib, "rollout_policy_kernel") and not _jit_closed_loop_launches(lib, "rollout_actor_kernel")
    assert lib.pcg_plan_prepare_closed_loop(env._plan) == want_prepare
    assert lib.pcg_plan_prepare_closed_loop(env._plan) == want_prepare  # idempotent
    # a built-in plan: nothing to prepare, whatever the plan
    for scen, over in (("cstr_canonical", dict(integrator="rk4")), ("cstr_cons_pen_norm", dict(integrator="rk4")),
                       ("cstr_canonical", dict(integrator="dopri5"))):
        q = copy.deepcopy(SC.scenarios()[scen]["env_params"])
        q.update(over)
        eb = _make(q, 64, seed=1)
        assert lib.pcg_plan_prepare_closed_loop(eb._plan) == abi.PCG_OK
        eb.close()
    assert lib.pcg_plan_prepare_closed_loop(None) == abi.PCG_E_PLAN
    env.close(), pol.close(), crit.close()


# ---- 8. stream capture ----------------------------------------------------------------------------------------------------------
def test_capture_needs_the_module_first_and_then_replays_the_eager_call():
    torch = _torch()
    from pcgym_amd import _abi as abi

    env = _make(_spread_x0(_chemostat("cv8")), B, seed=6)  # a fresh plan: its closed-loop module does not exist yet
    spec, dev = env.spec, env.device
    env.reset()
    pol = make_policy(spec, env.obs_soa.cpu().numpy(), (16,), seed=29)
    h = pol.handle(dev)
    x0, o0 = env.x.clone(), env.obs_soa.clone()
    f64 = torch.float64
    a_seq = torch.full((T + 1, spec.na, B), -7.0, dtype=f64, device=dev)
    o_seq = torch.full((T, spec.nobs, B), -7.0, dtype=f64, device=dev)
    r_seq = torch.full((T, B), -7.0, dtype=f64, device=dev)
    marker = torch.zeros(8, dtype=f64, device=dev)
    seed = env._episode_seed()

    def call(stream):
        return env._lib.pcg_rollout_policy(env._plan, env._bufp, h, 0, T, a_seq.data_ptr(), spec.na * B, B, o_seq.data_ptr(),
                                           spec.nobs * B, B, r_seq.data_ptr(), B, 1, seed, stream)

    torch.cuda.synchronize()
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0):
        marker.fill_(1.0)  # (so that the recorded graph is not empty)
        rc = call(torch.cuda.current_stream(dev).cuda_stream)
    assert rc == abi.PCG_E_UNSUPPORTED, "a module cannot be loaded inside a capture: the call has to say so"
    g0.replay()
    torch.cuda.synchronize()
    assert bool((marker == 1.0).all()), "the capture around the refused call did not survive it"
    assert torch.equal(env.x, x0) and torch.equal(env.obs_soa, o0)
    assert all(bool((t == -7.0).all()) for t in (a_seq, o_seq, r_seq)), "the refused call wrote something"
    assert not _jit_closed_loop_launches(env._lib, "rollout_policy_kernel")

    assert env.prepare_closed_loop() is env
    assert call(torch.cuda.current_stream(dev).cuda_stream) == 0
    torch.cuda.synchronize()
    eager = [t.clone() for t in (a_seq, o_seq, r_seq, env.x, env.obs_soa, env.rew, env.done)]
    assert float(a_seq.std()) > 0 and bool(torch.isfinite(o_seq).all())
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
    env.close(), pol.close()


# ---- 9. the caches --------------------------------------------------------------------------------------------------------------
def test_closed_loop_module_is_a_second_cache_entry_written_at_first_use(tmp_path, monkeypatch):
    """creating the plan writes one code object, the first closed-loop call a second one, a second plan of the same source
    none (a source no other test compiles: the in-process cache cannot answer for the disk cache)"""
    torch = _torch()

    cache = tmp_path / "jit"
    monkeypatch.setenv("PCG_JIT_CACHE", str(cache))  # (read at every compilation)

    def files():
        return sorted(f for f in os.listdir(cache) if f.endswith(".pco")) if os.path.isdir(cache) else []

    p = _chemostat("rk4")
    p["custom_model"]["rhs"][0] = "(mu - D)*X*1.0"
    env = _make(p, B, seed=1)
    f1 = files()
    assert len(f1) == 1, f1
    env.reset()
    env.step(torch.zeros((1, B), dtype=torch.float64, device=env.device))
    env.rollout(torch.zeros((2, 1, B), dtype=torch.float64, device=env.device))
    torch.cuda.synchronize()
    assert files() == f1, "stepping and the open-loop rollout need no second module"
    pol = make_policy(env.spec, env.obs_soa.cpu().numpy(), (16,), seed=1)
    env.reset()
    env.rollout_policy(pol, 2)
    torch.cuda.synchronize()
    f2 = files()
    assert len(f2) == 2 and set(f1) < set(f2), f2
    env2 = _make(p, B, seed=1)
    env2.reset()
    env2.prepare_closed_loop()
    a2, _, _ = env2.rollout_policy(pol, 2)
    ac = make_ac(env.spec, env.obs_soa.cpu().numpy(), (16,), seed=1)
    env2.rollout_actor(ac, 2)  # (the actor's kernel sits in the same module)
    torch.cuda.synchronize()
    assert files() == f2 and bool(torch.isfinite(a2).all())
    assert not [f for f in os.listdir(cache) if not f.endswith(".pco")], "a temporary was left behind"
    env.close(), env2.close(), pol.close(), ac.close()
