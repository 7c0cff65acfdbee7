"""The fused closed-loop rollouts on plans with per-env parameters (pcg_rollout_policy_unc / pcg_rollout_actor_unc,
pcg_rollout_unc.hpp) against the oracle, against themselves in chunks, and against the per-step route.

The step kernels and these kernels compile M::prep and the right-hand side under the compiler's default contraction, each on
its own, and two such kernels differ in the last bits (tests/test_gpu_round2.py:
test_fused_rollout_with_per_env_parameters_matches_stepping).  Equal bits are therefore asked only where the SAME kernel runs
twice (one call against chunked calls, eager against a replayed graph); every other comparison uses the project's own
tolerances for per-env parameters (tests/test_gpu_sweeps.py: test_uncertainty_sweep): one step against the oracle 1e-8 (5e-6
for the pow() forms, the "^" keys) on the state by helpers.worst_rel and rtol 1e-8 / atol 1e-9 (1e-5 / 1e-5) on the
observation, T steps against the per-step route 1e-7 (2e-5); rewards under the fused tests' rule, rtol 1e-9 and
atol 1e-10 (1 + max|r|).  The per-step route is TEACHER-FORCED with the recorded actions, as in tests/test_gpu_cons_rollout.py:
the kernel and torch round the networks differently, and the networks are held against helpers.host_reference instead.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import scenarios as SC
from helpers import (LD, MODEL_KEYS, PRE_MAX, U, _final_equal, _launched, _make, _rew_close, _tols, _torch, _unc_params, host_reference,
                     make_policy, sweep_params, tanh_k, worst_rel)
from test_gpu_actor_rollout import logp_numpy, make_ac, pick_ac, raw_twin

pytestmark = pytest.mark.gpu

B = 578  # two full blocks, one partial wave, even
SEED = 9


def _has_kernel(key):
    from pcgym_amd.models import get_model

    return get_model(key.partition("^")[0]).affine_builder is None


KEYS = [k for k in MODEL_KEYS if _has_kernel(k)]


def _params(key):
    """the model's first two non-zero parameters +-3 % (uniform, bounded), and every env its own initial state (+-2 %)"""
    p = _unc_params(key, "rk4")
    p["uncertainty_percentages"] = dict(p["uncertainty_percentages"], x0=[0.02] * 24)
    return p


def _envs(p, n, nb=B):
    envs = [_make(p, nb, seed=SEED) for _ in range(n)]
    for e in envs:
        e.reset()
    return envs


def _call(env, head, net, T, **kw):
    """one fused call through the wrappers -> dict a / obs / rew (+ u / logp / val)"""
    if head == "policy":
        a, o, r = env.rollout_policy_unc(net, T, collect_obs=True, **kw)
        return {"a": a, "obs": o, "rew": r}
    return env.rollout_actor_unc(net, T, collect_obs=True, **kw)


def _net(head, spec, obs0, T, nb=B):
    if head == "policy":
        return make_policy(spec, obs0, (16,), seed=17)
    # (the clip box under which the ORACLE's own steps are well conditioned: tests/test_gpu_actor_rollout.py, pick_ac)
    return pick_ac(spec, obs0, (16,), 17, nb, T, SEED)[0]


# ---- 1. every instantiation, both heads, against the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("head", ["policy", "actor"])
@pytest.mark.parametrize("key", KEYS)
def test_every_instantiation_against_the_oracle(key, head):
    torch = _torch()
    from oracle import oracle as O

    tol = _tols(key)
    (env,) = _envs(_params(key), 1)
    spec = env.spec
    assert spec.nunc >= 1 and not spec.ncon and spec.integrator == "rk4" and spec.x0_unc is not None
    orc = O.OracleEnv(spec, B, seed=SEED)
    orc.reset()
    p_unc = env.p_unc.cpu().numpy().copy()
    assert np.allclose(p_unc, orc.p_unc, rtol=1e-14, atol=0) and np.std(orc.p_unc, axis=1).min() > 0
    assert np.allclose(env.x.cpu().numpy(), orc.x, rtol=1e-14, atol=0)
    obs0 = env.obs_soa.cpu().numpy().copy()
    assert np.std(obs0[spec.nobs - spec.nunc:], axis=1).min() > 0, "the parameter slots of the reset observation do not vary"
    net = _net(head, spec, obs0, 3)
    for c in range(3):
        x_before = env.x.cpu().numpy().copy()
        out = _call(env, head, net, 1)
        torch.cuda.synchronize()
        a = out["a"][0].cpu().numpy()
        assert np.isfinite(a).all()
        orc.x[:] = x_before
        oc, rc, _ = orc.step(a)
        ex = worst_rel(env.x.cpu().numpy(), orc.x)
        o_np, r_np = out["obs"][0].cpu().numpy(), out["rew"][0].cpu().numpy()
        eo = float(np.max(np.abs(o_np - oc) - tol["o_rtol"] * np.abs(oc)))
        print(f"case {key}-{head} chunk {c}: state {ex:.3e} (bar {tol['x1']:.0e}), observation excess over rtol {eo:.3e} "
              f"(atol {tol['o_atol']:.0e}), reward max |diff| {np.max(np.abs(r_np - rc)):.3e} of max |r| {np.max(np.abs(rc)):.3e}")
        assert ex <= tol["x1"], f"chunk {c}: state {ex:.3e} from the oracle"
        assert np.allclose(o_np, oc, rtol=tol["o_rtol"], atol=tol["o_atol"]), f"chunk {c}: observation"
        assert _rew_close(r_np, rc), f"chunk {c}: reward"
        assert torch.equal(env.obs_soa, out["obs"][0]) and torch.equal(env.rew, out["rew"][0]) and env.t == c + 1
    assert _launched(env._lib, f"rollout_unc_{head}_kernel")
    assert torch.equal(env.p_unc.cpu(), torch.as_tensor(p_unc)), "the call wrote io->p_unc"
    assert not env.status.any()
    env.close(), net.close()


# ---- 2. one call equals chunked calls, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", ["policy", "actor"])
@pytest.mark.parametrize("nb", [B, 131])
def test_one_call_equals_chunked_calls_bitwise(nb, head):
    torch = _torch()
    T = 6
    ea, eb, ec = _envs(_params("cstr"), 3, nb)
    spec = ea.spec
    obs0 = ea.obs_soa.clone()
    assert torch.equal(ea.x, eb.x) and torch.equal(ea.p_unc, ec.p_unc)
    net = _net(head, spec, obs0.cpu().numpy(), T, nb)
    one = _call(ea, head, net, T, record_next_action=True)
    keys = [k for k, v in one.items() if v is not None]
    assert set(keys) == ({"a", "obs", "rew"} if head == "policy" else {"a", "u", "logp", "val", "obs", "rew"})
    for env, chunks in ((eb, (1, 2, 3)), (ec, (3, 3))):
        parts, done = [], 0
        for n in chunks:
            assert env.t == done
            parts.append(_call(env, head, net, n, record_next_action=(done + n == T)))
            done += n
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(torch.cat([q[k] for q in parts]), one[k]), f"chunks {chunks}: {k}"
        _final_equal(env, ea)
    assert one["a"].shape == (T + 1, spec.na, nb) and one["obs"].shape == (T, spec.nobs, nb)
    assert torch.isfinite(one["obs"]).all() and not ea.status.any()
    # the parameter slots of every recorded row are the reset observation's, bit for bit
    lo = spec.nobs - spec.nunc
    for s in range(T):
        assert torch.equal(one["obs"][s, lo:], obs0[lo:]), f"step {s}: the recorded parameter slots"
    assert _launched(ea._lib, f"rollout_unc_{head}_kernel")
    for e in (ea, eb, ec):
        e.close()
    net.close()


# ---- 3. against the per-step route, teacher-forced --------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", ["policy", "actor"])
@pytest.mark.parametrize("key", ["cstr", "multistage_extraction^1.5"])
def test_against_the_per_step_route(key, head):
    torch = _torch()
    T, tol = 3, _tols(key)
    ef, es = _envs(_params(key), 2)
    spec = ef.spec
    net = _net(head, spec, ef.obs_soa.cpu().numpy(), T)
    p_before = ef.p_unc.clone()
    out = _call(ef, head, net, T)
    torch.cuda.synchronize()
    assert torch.equal(ef.p_unc, p_before), "the call wrote io->p_unc"
    obs, rew = [], []
    for s in range(T):
        es.step(out["a"][s])
        obs.append(es.obs_soa.clone()), rew.append(es.rew.clone())
    torch.cuda.synchronize()
    assert _launched(ef._lib, f"rollout_unc_{head}_kernel") and _launched(ef._lib, "step_kernel")
    for s in range(T):
        eo = worst_rel(out["obs"][s].cpu().numpy(), obs[s].cpu().numpy())
        r, rr = out["rew"][s].cpu().numpy(), rew[s].cpu().numpy()
        print(f"case {key}-{head} step {s}: observation {eo:.3e} from the per-step route (bar {tol['xT']:.0e}), reward max |diff| "
              f"{np.max(np.abs(r - rr)):.3e}")
        assert eo <= tol["xT"], f"step {s}: observation {eo:.3e} from the per-step route"
        assert _rew_close(r, rr), f"step {s}: reward"
    assert worst_rel(ef.x.cpu().numpy(), es.x.cpu().numpy()) <= tol["xT"]
    assert ef.t == es.t == T and torch.equal(ef.done, es.done)
    ef.close(), es.close(), net.close()


# ---- 4. the networks ---------------------------------------------------------------------------------------------------------------------
def _slot_policy(spec, obs0, slot=None, values=None):
    """make_policy's network with ONE large first-layer weight on `slot` (default: the last parameter slot): a dropped slot
    shows in the output.  `values`: what the slot takes (default: over the batch at reset)"""
    from pcgym_amd import MLPPolicy

    pol = make_policy(spec, obs0, (16,), seed=17)
    Ws, bs = [w.copy() for w in pol.weights], [b.copy() for b in pol.biases]
    slot = spec.nobs - 1 if slot is None else slot
    values = obs0[slot] if values is None else values
    spread = float(np.max(values) - np.min(values))
    assert spread > 0
    w = 4.0 / spread  # the slot alone moves the unit's pre-activation by 4 across the batch
    bs[0][0] -= (w - Ws[0][0, slot]) * float(np.mean(values))
    Ws[0][0, slot] = w
    Ws[1][:, 0] = np.where(Ws[1][:, 0] >= 0, 1.0, -1.0) * max(float(np.max(np.abs(Ws[1]))), 0.1)  # (and the unit reaches the output)
    out = MLPPolicy(Ws, bs, activation=pol.activation, out_map=pol.out_map, out_low=pol.out_low, out_high=pol.out_high)
    pol.close()
    return out, slot


def test_the_policy_reads_the_parameter_slots():
    torch = _torch()
    T = 4
    (env,) = _envs(_params("cstr"), 1)
    spec = env.spec
    obs0 = env.obs_soa.cpu().numpy().copy()
    pol, slot = _slot_policy(spec, obs0)
    k = tanh_k()
    # a condition on the INPUTS: without the slot the reference moves by far more than the bound
    ref0, bound0, _ = host_reference(pol, obs0, k + 1.0)
    dropped = obs0.copy()
    dropped[slot] = 0.0
    gap = np.abs((host_reference(pol, dropped, k + 1.0)[0] - ref0).astype(np.float64))
    assert np.mean(gap > 1e6 * np.max(bound0)) > 0.25, f"the slot moves the output of {np.mean(gap > 1e6 * np.max(bound0)):.2f} of the envs only"
    a, o, _ = env.rollout_policy_unc(pol, T, collect_obs=True, record_next_action=True)
    torch.cuda.synchronize()
    a_np, o_np = a.cpu().numpy(), o.cpu().numpy()
    assert a_np.shape == (T + 1, spec.na, B) and np.isfinite(a_np).all()
    pre = 0.0
    for s in range(T + 1):  # (row T: the policy on the observation after the last step, recorded and not applied)
        ref, bound, pm = host_reference(pol, obs0 if s == 0 else o_np[s - 1], k + 1.0)
        pre = max(pre, pm)
        diff = np.abs(a_np[s].astype(LD) - ref).astype(np.float64)
        assert np.all(diff <= bound), f"step {s}: policy output off by {np.max(diff):.3e} (bound {np.max(bound):.3e})"
    assert pre <= PRE_MAX
    assert torch.equal(env.obs_soa, o[T - 1])  # row T was evaluated on io->obs as the call leaves it
    assert np.any((a_np > pol.out_low) & (a_np < pol.out_high)), "every output sits on the clip box"
    env.close(), pol.close()


def test_the_actor_samples_values_and_log_probabilities():
    torch = _torch()
    T = 4
    (env,) = _envs(_params("cstr"), 1)
    spec = env.spec
    obs0 = env.obs_soa.cpu().numpy().copy()
    ac = _net("actor", spec, obs0, T)
    k = tanh_k()
    out = env.rollout_actor_unc(ac, T, collect_obs=True, record_next_action=True)
    torch.cuda.synchronize()
    a_np, u_np, lp_np, v_np, o_np = (out[n].cpu().numpy() for n in ("a", "u", "logp", "val", "obs"))
    assert u_np.shape == (T + 1, spec.na, B) and lp_np.shape == v_np.shape == (T + 1, B)
    raw, sig = raw_twin(ac.actor), ac.sigma[:, None]
    assert ac.actor.out_map == "clip"
    assert np.array_equal(a_np, np.clip(u_np, ac.actor.out_low, ac.actor.out_high)), "a is not clip(u) bitwise"
    assert np.any(a_np != u_np) and np.any(a_np == u_np)
    pre = 0.0
    for s in range(T + 1):  # (row T: drawn at counter T on the final observation, the bootstrap value)
        z = env.policy_noise(s).cpu().numpy()
        o_in = obs0 if s == 0 else o_np[s - 1]
        mu, b_mu, pm = host_reference(raw, o_in, k + 1.0)
        pre = max(pre, pm)
        diff = np.abs(u_np[s].astype(LD) - (mu + sig.astype(LD) * z.astype(LD))).astype(np.float64)
        assert np.all(diff <= b_mu + U * np.abs(u_np[s])), f"step {s}: sample off by {np.max(diff):.3e}"
        assert np.array_equal(lp_np[s], logp_numpy(ac, z)), f"step {s}: logp is not the specified operation sequence"
        vr, b_v, pm = host_reference(ac.critic, o_in, k + 1.0)
        pre = max(pre, pm)
        assert np.all(np.abs(v_np[s].astype(LD) - vr[0]).astype(np.float64) <= b_v[0]), f"step {s}: value outside its bound"
    assert pre <= PRE_MAX
    env.close(), ac.close(), raw.close()


# ---- 5. collectors -------------------------------------------------------------------------------------------------------------------------
def test_collect_rollouts_takes_the_fused_call():
    torch = _torch()
    from pcgym_amd import collect_rollouts

    ef, es, er = _envs(_params("cstr"), 3)  # (collect_rollouts resets again: the envs stay in the same RNG epoch)
    spec = ef.spec
    N, tol = spec.N, _tols("cstr")
    # (make_ac's actor: its mean at the mean reset observation is the middle of the action box, which keeps every reactor of
    # this 99-step episode away from thermal runaway -- a state that is not finite compares with nothing)
    ac = make_ac(spec, ef.obs_soa.cpu().numpy(), (16,), seed=23, sigma_scale=0.1)
    pol = ac.actor
    fused = collect_rollouts(ef, policy=pol, fused_unc=True)
    torch.cuda.synchronize()
    assert _launched(ef._lib, "rollout_unc_policy_kernel"), "collect_rollouts(fused_unc=True) did not take the fused call"
    assert all(bool(torch.isfinite(fused[k]).all()) for k in ("r", "x", "u")) and not ef.status.any()
    # the callable route, teacher-forced: a callable that replays the policy outputs the same kernel records
    er.reset()
    a_seq = er.rollout_policy_unc(pol, N - 1, record_next_action=True)[0]
    step = iter(range(N))
    ref = collect_rollouts(es, policy=lambda o: a_seq[next(step)])
    torch.cuda.synchronize()
    assert next(step, None) is None
    with pytest.raises(ValueError):
        collect_rollouts(er, policy=lambda o: a_seq[0], fused_unc=True)  # (a callable is no declarative policy)
    open_loop = torch.zeros((N, spec.na, B), dtype=torch.float64, device=er.device)
    for kw in (dict(actions=open_loop), dict(actions=open_loop, policy=pol)):  # (the open loop has no such call; both is refused anyway)
        with pytest.raises(ValueError):
            collect_rollouts(er, fused_unc=True, **kw)
    assert set(fused) == set(ref) == {"r", "x", "u"}
    assert fused["x"].shape == ref["x"].shape == (spec.nobs, N, B) and fused["u"].shape == (spec.na, N, B) and fused["r"].shape == (1, N, B)
    assert torch.equal(fused["u"], ref["u"]) and torch.equal(fused["x"][:, 0], ref["x"][:, 0])
    ex = worst_rel(fused["x"].reshape(spec.nobs, -1).cpu().numpy(), ref["x"].reshape(spec.nobs, -1).cpu().numpy())
    print(f"collect_rollouts: x {ex:.3e} from the callable route over {N - 1} steps (bar {tol['xT']:.0e})")
    assert ex <= tol["xT"]
    assert _rew_close(fused["r"].cpu().numpy(), ref["r"].cpu().numpy())
    lo = spec.nobs - spec.nunc
    assert torch.equal(fused["x"][lo:, 1:], fused["x"][lo:, :1].expand(-1, N - 1, -1)), "the parameter rows of x change along the episode"
    assert ef.t == es.t == N - 1
    for e in (ef, es, er):
        e.close()
    ac.close()


def test_collect_onpolicy_takes_the_fused_call():
    torch = _torch()
    from pcgym_amd import collect_onpolicy

    ef, es = _envs(_params("cstr"), 2)  # (collect_onpolicy resets again: the envs stay in the same RNG epoch)
    spec = ef.spec
    T, tol = spec.N - 1, _tols("cstr")
    ac = make_ac(spec, ef.obs_soa.cpu().numpy(), (16,), seed=23, sigma_scale=0.1)
    fused = collect_onpolicy(ef, ac, fused_unc=True)
    torch.cuda.synchronize()
    assert _launched(ef._lib, "rollout_unc_actor_kernel"), "collect_onpolicy(fused_unc=True) did not take the fused call"
    ref = collect_onpolicy(es, ac, fused=False)
    torch.cuda.synchronize()
    assert set(fused) == set(ref) == {"obs", "act", "logp", "val", "rew", "adv", "ret"}
    shapes = {"obs": (T + 1, spec.nobs, B), "act": (T, spec.na, B), "logp": (T, B), "val": (T + 1, B), "rew": (T, B), "adv": (T, B), "ret": (T, B)}
    for n, shape in shapes.items():
        assert fused[n].shape == ref[n].shape == shape and torch.isfinite(fused[n]).all(), n
    assert torch.equal(fused["logp"], ref["logp"]) and torch.equal(fused["obs"][0], ref["obs"][0])
    eo = worst_rel(fused["obs"].permute(1, 0, 2).reshape(spec.nobs, -1).cpu().numpy(), ref["obs"].permute(1, 0, 2).reshape(spec.nobs, -1).cpu().numpy())
    ea = worst_rel(fused["act"].permute(1, 0, 2).reshape(spec.na, -1).cpu().numpy(), ref["act"].permute(1, 0, 2).reshape(spec.na, -1).cpu().numpy())
    ev = worst_rel(fused["val"].reshape(1, -1).cpu().numpy(), ref["val"].reshape(1, -1).cpu().numpy())
    print(f"collect_onpolicy: obs {eo:.3e}, act {ea:.3e}, val {ev:.3e} from the per-step route over {T} steps (bar {tol['xT']:.0e})")
    assert max(eo, ea, ev) <= tol["xT"]
    assert _rew_close(fused["rew"].cpu().numpy(), ref["rew"].cpu().numpy())
    # per-env parameters AND a constraint row: no fused call takes the plan
    both = copy.deepcopy(SC.scenarios()["cstr_cons_pen_norm"]["env_params"])
    both.update(integrator="rk4", uncertainty_percentages={"q": 0.03}, distribution="uniform",
                uncertainty_bounds={"low": np.array([90.0]), "high": np.array([110.0])})
    eb = _make(both, 64, seed=SEED)
    ac2 = make_ac(eb.spec, eb.reset()[0].t().cpu().numpy(), (16,), seed=23)
    assert eb.spec.nunc and eb.spec.ncon
    for kw in (dict(fused=True), dict(fused=True, record_cons=True), dict(fused_unc=True), dict(fused_unc=True, record_cons=True)):
        with pytest.raises(ValueError):
            collect_onpolicy(eb, ac2, **kw)
    with pytest.raises(ValueError):
        collect_onpolicy(es, ac, fused_unc=True, fused=False)
    ef.close(), es.close(), eb.close(), ac.close(), ac2.close()


# ---- 6. refusals launch nothing and write nothing ----------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    torch = _torch()
    from pcgym_amd import MLPPolicy
    from pcgym_amd import _abi as abi
    from pcgym_amd.models import get_model
    from test_policy_jit_plans import _chemostat

    UNS, DIM, VAL, NUL, PLAN = abi.PCG_E_UNSUPPORTED, abi.PCG_E_DIM, abi.PCG_E_VALUE, abi.PCG_E_NULL, abi.PCG_E_PLAN
    seen = []

    def attempt(env, want, pol, critic="same", sigma="ok", T=3, t0=None, a_cs=None, head="policy", buf=None):
        """one refused call; state, observation, parameters and pre-filled outputs unchanged"""
        s, nb, dev = env.spec, env.B, env.device
        x, o = env.x.clone(), env.obs_soa.clone()
        pu = env.p_unc.clone() if env.p_unc is not None else None
        outs = [torch.full(shape, -5.5, dtype=torch.float64, device=dev) for shape in
                ((T + 1, s.na, nb), (T + 1, s.na, nb), (T + 1, nb), (T + 1, nb), (max(T, 1), s.nobs, nb), (max(T, 1), nb))]
        a, u, lp, val, ob, rw = outs
        acs = nb if a_cs is None else a_cs
        t0 = env.t if t0 is None else t0
        bufp = env._bufp if buf is None else C.byref(buf)
        h = pol.handle(dev) if hasattr(pol, "handle") else pol
        if head == "policy":
            rc = env._lib.pcg_rollout_policy_unc(env._plan, bufp, h, t0, T, a.data_ptr(), s.na * nb, acs, ob.data_ptr(), s.nobs * nb, nb,
                                                 rw.data_ptr(), nb, 1, 7, env._stream())
        else:
            cr = critic.handle(dev) if hasattr(critic, "handle") else critic
            sg = None if sigma is None else np.ascontiguousarray(sigma, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
            rc = env._lib.pcg_rollout_actor_unc(env._plan, bufp, h, cr, sg, t0, T, a.data_ptr(), s.na * nb, acs, u.data_ptr(), s.na * nb, nb,
                                                lp.data_ptr(), nb, val.data_ptr(), nb, ob.data_ptr(), s.nobs * nb, nb, rw.data_ptr(), nb, 1,
                                                7, env._stream())
        torch.cuda.synchronize()
        assert rc == want, (len(seen), rc, want)
        assert torch.equal(env.x, x) and torch.equal(env.obs_soa, o) and (pu is None or torch.equal(env.p_unc, pu))
        assert all(bool((t == -5.5).all()) for t in outs)
        seen.append(rc)

    def nets(spec, dtype="float64"):
        rng = np.random.default_rng(0)
        Ws = [rng.standard_normal((16, spec.nobs)) / 4, rng.standard_normal((spec.na, 16)) / 4]
        bs = [np.zeros(16), np.zeros(spec.na)]
        pol = MLPPolicy(Ws, bs, dtype=dtype)
        cr = MLPPolicy([Ws[0], Ws[1][:1]], [bs[0], bs[1][:1]], out_map="none", dtype=dtype)
        return pol, cr

    # ---- the plans: PCG_E_UNSUPPORTED, in the header's order ----
    # (the run-time compiled plan, the affine registry model and `plain` all have nunc == 0 and are refused by that clause:
    # pcg_plan_create itself refuses nunc > 0 on run-time compiled and on affine / user models, so no plan can reach
    # closed_loop_open's own `unc` checks of those two through the public interface, and this test does not cover them alone)
    unc = _params("cstr")
    plain = copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"])
    plain.update(integrator="rk4")
    both = copy.deepcopy(SC.scenarios()["cstr_cons_pen_norm"]["env_params"])
    both.update(integrator="rk4", uncertainty_percentages={"q": 0.03}, distribution="uniform",
                uncertainty_bounds={"low": np.array([90.0]), "high": np.array([110.0])})
    dopri = copy.deepcopy(unc)
    dopri.update(integrator="dopri5", rtol=1e-6, atol=1e-8)
    affine = next(k for k in MODEL_KEYS if get_model(k.partition("^")[0]).affine_builder is not None)
    sig_of = lambda spec: np.full(spec.na, 0.3)  # noqa: E731
    for params, kw in ((plain, {}), (both, {}), (unc, dict(per_env_t=True)), (dopri, {}), (_chemostat(integrator="rk4"), {}),
                       (sweep_params(affine, "rk4", "lean"), {})):
        env = _make(params, 64, seed=3, **kw)
        env.reset()
        pol, cr = nets(env.spec)
        attempt(env, UNS, pol)
        attempt(env, UNS, pol, critic=cr, sigma=sig_of(env.spec), head="actor")
        env.close(), pol.close(), cr.close()
    env = _make(unc, 64, seed=3)
    env.reset()
    spec = env.spec
    assert spec.nunc >= 1
    pol, cr = nets(spec)
    p32, c32 = nets(spec, "float32")
    sig = sig_of(spec)
    attempt(env, UNS, p32)
    attempt(env, UNS, p32, critic=c32, sigma=sig, head="actor")
    attempt(env, UNS, pol, critic=c32, sigma=sig, head="actor")
    # ---- everything else, in the base calls' order ----
    junk = C.cast(C.create_string_buffer(512), C.c_void_p)
    attempt(env, NUL, None)
    attempt(env, PLAN, junk)
    wrong = MLPPolicy([np.zeros((spec.na, spec.nobs - spec.nunc))], [np.zeros(spec.na)])  # (the observation without its parameter slots)
    attempt(env, DIM, wrong)
    attempt(env, PLAN, pol, critic=junk, sigma=sig, head="actor")
    attempt(env, DIM, pol, critic=pol if spec.na != 1 else wrong, sigma=sig, head="actor")
    cmap = MLPPolicy(cr.weights, cr.biases, out_map="clip")
    attempt(env, VAL, pol, critic=cmap, sigma=sig, head="actor")
    tanh = MLPPolicy(pol.weights, pol.biases, out_map="tanh")
    attempt(env, UNS, tanh, critic=cr, sigma=sig, head="actor")
    attempt(env, NUL, pol, critic=cr, sigma=None, head="actor")
    attempt(env, VAL, pol, critic=cr, sigma=-sig, head="actor")
    for head in ("policy", "actor"):
        kw = dict(critic=cr, sigma=sig, head=head)
        attempt(env, VAL, pol, T=0, **kw)
        attempt(env, VAL, pol, t0=-1, **kw)
        nob = abi.pcg_buffers.from_buffer_copy(env._buf)
        nob.rew = None
        attempt(env, NUL, pol, buf=nob, **kw)
        nop = abi.pcg_buffers.from_buffer_copy(env._buf)
        nop.p_unc = None
        attempt(env, NUL, pol, buf=nop, **kw)            # io->p_unc == NULL
        attempt(env, DIM, pol, a_cs=env.B - 1, **kw)     # a_comp_stride < B
    assert len(seen) == 34 and not _launched(env._lib, "rollout_unc_")
    env.close()
    for q in (pol, cr, p32, c32, wrong, cmap, tanh):
        q.close()


# ---- 7. stream capture ---------------------------------------------------------------------------------------------------------------------
def test_the_call_is_capture_safe():
    torch = _torch()
    ee, eg = _envs(_params("cstr"), 2)
    spec = ee.spec
    T = 6
    pol = make_policy(spec, ee.obs_soa.cpu().numpy(), (16,), seed=23)
    eager = _call(ee, "policy", pol, T)
    pol.handle(eg.device)
    torch.cuda.synchronize()
    x0, o0, t0 = eg.x.clone(), eg.obs_soa.clone(), eg.t
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):  # (one call: a single branch)
            cap = _call(eg, "policy", pol, T)
    torch.cuda.current_stream().wait_stream(side)
    eg.x.copy_(x0), eg.obs_soa.copy_(o0)
    for k in ("a", "obs", "rew"):
        cap[k].fill_(0.0)
    graph.replay()
    torch.cuda.synchronize()
    assert eg.t == t0 + T
    for k in ("a", "obs", "rew"):
        assert torch.equal(cap[k], eager[k]), k
    _final_equal(eg, ee)
    ee.close(), eg.close(), pol.close()
