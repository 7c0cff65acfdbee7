"""The fused closed-loop rollouts on plans with constraint rows (pcg_rollout_policy_cons / pcg_rollout_actor_cons,
pcg_rollout_cons.hpp) against the per-step route and the oracle.

The per-step route of every comparison is TEACHER-FORCED, as in tests/test_gpu_policy_rollout.py: a callable policy that
hands env.step() the actions the fused call recorded.  The kernel evaluates the networks with its own FMA order and tanh,
torch with another (the existing closed-loop tests bound that difference, they never ask for equal bits), and through a
closed loop the last bit of an action reaches every later number; with the recorded actions both routes do the SAME env
arithmetic, and observations, rewards, rows, flags, done, the final state and g_pre must then be equal bit for bit
(torch.equal).  The recorded actions themselves are held against the networks: the policy's against the running bound of
helpers.host_reference on the kernel's own observations; the actor's a == out_map(u) bitwise, u against mu_ref + sigma z
inside the same bound + one rounding, logp restated operation by operation (z: pcg_policy_noise, the oracle's twin --
tests/test_gpu_actor_rollout.py).

Oracle: every step from the per-step route's own start state with the recorded action (OracleEnv.step); rows within
G_TOL x (|b| + sum |A_i| max(|v_i|, 1)) -- the existing fused tests' state tolerance 1e-12 relative to max(|x|, 1), carried
through the row, which is linear in the state -- and rewards under those tests' own rule (rtol 1e-9, atol 1e-10 (1 + max|r|)),
except where the oracle's row is inside that tolerance of zero and the penalty may fall either way.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import scenarios as SC
from helpers import (LD, MODEL_KEYS, PRE_MAX, U, _case_params, _check_final, _launched, _make, _spread_x0, _stepped, _torch, host_reference,
                     make_policy, tanh_k)
from test_gpu_actor_rollout import logp_numpy, make_ac, pick_ac, raw_twin

pytestmark = pytest.mark.gpu

B = 578  # two full blocks, one partial wave, even
G_TOL = 1e-12
_PLANS = {}


def _with_row(p, spec, b):
    """env_params `p` + one dense affine row over [x | SP | d | u]: a state, a set-point slot where the plan has one, an action"""
    nst = spec.nobs - spec.nunc
    A = np.zeros((1, nst + spec.nu))
    width = np.maximum(np.asarray(spec.o_high, dtype=float) - np.asarray(spec.o_low, dtype=float), 1e-6)
    A[0, 0] = 1.0 / width[0]
    if spec.nsp_obs:
        A[0, spec.nx] = -0.5 / width[spec.nx]
    A[0, nst] = 0.3 / max(float(spec.a_high[0] - spec.a_low[0]), 1e-6)
    q = copy.deepcopy(p)
    q.update(constraints={"A": A, "b": np.array([float(b)])}, done_on_cons_vio=False, r_penalty=True)
    return q


def _base(key, integ):
    p = _spread_x0(_case_params(key, integ))
    for k in ("constraints", "done_on_cons_vio", "r_penalty"):
        p.pop(k, None)
    return p


def _plan(key, integ, head="policy"):
    """(the case's env_params with its row, the actor's clip box); b = the median of the row's linear part over a pilot per-step episode of the same
    envs under the head's own torch route (the policy as a callable; the actor sampled from env.policy_noise), so that about
    half the (env, step) entries violate -- chosen from the reference alone"""
    if (key, integ, head) in _PLANS:
        return _PLANS[key, integ, head]
    torch = _torch()
    p0 = _base(key, integ)
    e0 = _make(p0, 2, seed=9)
    try:
        q = _with_row(p0, e0.spec, 0.0)
        env = _make(q, B, seed=9)
    except ValueError:  # (the reference itself cannot combine normalise_a, disturbances and constraints for na > 1)
        p0["reference_compat"] = False
        q = _with_row(p0, e0.spec, 0.0)
        env = _make(q, B, seed=9)
    e0.close()
    env.reset()
    obs0 = env.obs_soa.cpu().numpy()
    box = None
    if head == "policy":
        net = make_policy(env.spec, obs0, (16,), seed=17)
    else:
        # (the clip box under which the ORACLE's own steps are well conditioned along this episode: an explicit step whose
        # stages leave the model's physical range amplifies round-off by orders of magnitude, and no two correct
        # implementations agree to 1e-12 there -- tests/test_gpu_actor_rollout.py: pick_ac)
        net, chosen = pick_ac(env.spec, obs0, (16,), 17, B, env.spec.N - 1, 9)
        box = chosen[:2]
    gs, obs = [], env.obs
    for i in range(env.spec.N - 1):
        a = net(obs) if head == "policy" else net.action(net.sample(obs, env.policy_noise(i).t()))
        obs = env.step(a)[0]
        gs.append(env.g[0].clone())
    g = torch.stack(gs).cpu().numpy()
    assert np.isfinite(g).all() and np.std(g) > 0, f"{key}-{integ}-{head}: the pilot's row does not vary"
    plan = _with_row(p0, env.spec, float(np.median(g)))
    env.close(), net.close()
    _PLANS[key, integ, head] = (plan, box)
    return plan, box


def _row_scale(spec, x, sp_d, u_phys):
    """|b| + sum |A_i| max(|v_i|, 1) per env"""
    A, b = np.abs(spec.con_A[0]), abs(float(spec.con_b[0]))
    return b + np.sum(A) * max(1.0, float(np.max(np.abs(x))), float(np.max(np.abs(sp_d))) if sp_d.size else 0.0, float(np.max(np.abs(u_phys))))


# ---- 1. every instantiation against the per-step route and the oracle ---------------------------------------------------------
@pytest.mark.parametrize("head", ["policy", "actor"])
@pytest.mark.parametrize("integ", ["rk4", "cv8"])
@pytest.mark.parametrize("key", MODEL_KEYS)
def test_every_instantiation(key, integ, head):
    torch = _torch()
    from oracle import oracle as O

    p, box = _plan(key, integ, head)
    ef, es = _make(p, B, seed=9), _make(p, B, seed=9)
    spec = ef.spec
    T = spec.N - 1
    assert spec.ncon == 1 and spec.integrator == integ and spec.r_penalty and spec.user_cons_src is None
    ef.reset(), es.reset()
    obs0 = ef.obs_soa.cpu().numpy().copy()
    assert torch.equal(ef.x, es.x)
    k = tanh_k()
    if head == "policy":
        pol = make_policy(spec, obs0, (16,), seed=17)
        out = ef.rollout_policy_cons(pol, T, collect_obs=True, record_next_action=True)
    else:
        ac = make_ac(spec, obs0, (16,), seed=17, centre=box[0], box=box[1])
        out = ef.rollout_actor_cons(ac, T, collect_obs=True, record_next_action=True)
    torch.cuda.synchronize()
    assert _launched(ef._lib, f"rollout_cons_{head}_kernel")
    assert out["g"].shape == (T, 1, B) and out["viol"].shape == (T, B) and out["viol"].dtype == torch.bool
    a_np, o_np = out["a"].cpu().numpy(), out["obs"].cpu().numpy()
    assert np.isfinite(a_np).all() and np.isfinite(o_np).all() and not ef.status.any()

    # ---- the recorded actions against the networks ----
    pre = 0.0
    if head == "policy":
        for s in range(T + 1):
            ref, bound, pm = host_reference(pol, obs0 if s == 0 else o_np[s - 1], k + 1.0)
            pre = max(pre, pm)
            diff = np.abs(a_np[s].astype(LD) - ref).astype(np.float64)
            assert np.all(diff <= bound), f"step {s}: policy output off by {np.max(diff):.3e} (bound {np.max(bound):.3e})"
    else:
        u_np, lp_np, v_np = (out[n].cpu().numpy() for n in ("u", "logp", "val"))
        raw, sig = raw_twin(ac.actor), ac.sigma[:, None]
        if ac.actor.out_map == "clip":
            assert np.array_equal(a_np, np.clip(u_np, ac.actor.out_low, ac.actor.out_high)), "a is not clip(u) bitwise"
        for s in range(T + 1):
            z = es.policy_noise(s).cpu().numpy()
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

    # ---- the per-step route on the recorded actions: bit for bit ----
    ref = _stepped(es, out["a"], T)
    torch.cuda.synchronize()
    for n in ("obs", "rew", "g"):
        assert torch.equal(out[n], ref[n]), f"{n} differs from the per-step route"
    assert torch.equal(out["viol"], ref["viol"].view(torch.bool)), "viol differs from the per-step route"
    _check_final(ef, es)
    share = float(ref["viol"].float().mean())
    print(f"case {key}-{integ}-{head}: {share:.3f} of the (env, step) entries violate on the per-step route")
    assert 0.05 <= share <= 0.95, f"{share:.3f} of the entries violate: the row does not split the case"
    pen = ref["viol"].bool()
    assert (out["rew"][pen] <= -1000.0 + 1e-9).all() or spec.reward_batch or not spec.nsp, "the penalty does not show where viol is set"

    # ---- the oracle, every step from the per-step route's own start state ----
    orc = O.OracleEnv(spec, B, seed=9)
    orc.reset()
    x0s, g_np, r_np, v_np_ = ref["x0"].cpu().numpy(), ref["g"].cpu().numpy(), ref["rew"].cpu().numpy(), ref["viol"].cpu().numpy()
    assert np.allclose(orc.x, x0s[0], rtol=1e-14, atol=0)
    worst_g = 0.0
    for s in range(T):
        orc.x[:] = x0s[s]
        _, rc, _ = orc.step(a_np[s])
        assert np.isfinite(orc.g).all() and np.isfinite(rc).all()
        u_box = max(abs(float(np.max(np.abs(spec.a_low)))), abs(float(np.max(np.abs(spec.a_high)))), float(np.max(np.abs(a_np[s]))))
        tol = G_TOL * _row_scale(spec, orc.x, orc.slots, np.array([u_box]))
        dg = np.abs(g_np[s] - orc.g)
        worst_g = max(worst_g, float(np.max(dg)) / tol)
        assert np.all(dg <= tol), f"step {s}: row {np.max(dg):.3e} from the oracle (tolerance {tol:.3e})"
        sure = np.abs(orc.g[0]) > tol
        assert np.array_equal(v_np_[s][sure], orc.viol[sure]), f"step {s}: flags differ from the oracle's"
        assert np.allclose(r_np[s][sure], rc[sure], rtol=1e-9, atol=1e-10 * (1 + np.max(np.abs(rc)))), f"step {s}: reward"
    print(f"case {key}-{integ}-{head}: rows within {worst_g:.2e} x the oracle tolerance")
    ef.close(), es.close()
    (pol if head == "policy" else ac).close()


def _pair(p, n=2, nb=B):
    envs = [_make(p, nb, seed=4) for _ in range(n)]
    for e in envs:
        e.reset()
    return envs


# ---- 2. flags that matter --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["r_penalty", "done_on_cons_vio"])
def test_flags_that_matter(flag):
    torch = _torch()
    base = _plan("cstr", "rk4")[0]
    p = copy.deepcopy(base)
    p.update(r_penalty=(flag == "r_penalty"), done_on_cons_vio=(flag == "done_on_cons_vio"))
    ef, es, e5 = _pair(p, 3)
    spec = ef.spec
    T = spec.N - 1
    pol = make_policy(spec, ef.obs_soa.cpu().numpy(), (16,), seed=17)
    out = ef.rollout_policy_cons(pol, T, collect_obs=True)
    ref = _stepped(es, out["a"], T)
    torch.cuda.synchronize()
    for n in ("obs", "rew", "g"):
        assert torch.equal(out[n], ref[n]), n
    assert torch.equal(out["viol"], ref["viol"].view(torch.bool))
    _check_final(ef, es)  # (io->done, g_pre of a call from t0 = 0 among them)
    viol = out["viol"]
    assert 0.05 <= float(viol.float().mean()) <= 0.95
    # the same actions on the twin plan without either flag: what the flag changes
    q = copy.deepcopy(base)
    q.update(r_penalty=False, done_on_cons_vio=False)
    (e0,) = _pair(q, 1)
    ref0 = _stepped(e0, out["a"], T)
    torch.cuda.synchronize()
    assert torch.equal(ref0["g"], out["g"]) and torch.equal(ref0["obs"], out["obs"])
    if flag == "r_penalty":
        assert spec.nsp == 1  # (quirk Q4: the penalty once per SP key)
        assert torch.equal(out["rew"] != ref0["rew"], viol), "the penalty does not show exactly where viol is set"
        assert torch.equal(out["rew"][viol], ref0["rew"][viol] - 1000.0)
    else:
        assert torch.equal(out["rew"], ref0["rew"])
        done = ref["done"].bool()
        assert torch.equal(done[:-1], viol[:-1] | ((ref["g_pre"] > 0).any(0) & (torch.arange(T - 1, device=viol.device) == 0)[:, None]))
        assert done[-1].all()
        # envs go on stepping after `done`: an env that was done at step s still moves, and its rows are the stepped ones
        early = done[: T // 2].any(0)
        assert early.any()
        assert (out["obs"][T // 2 + 1:, :, early] != out["obs"][T // 2:-1, :, early]).any()
    # a call that starts at t0 = 5 leaves io->g_pre alone
    _stepped(e5, out["a"], 5, record_x=False)
    e5.g_pre.fill_(-77.0)
    o5 = e5.rollout_policy_cons(pol, T - 5)
    torch.cuda.synchronize()
    assert (e5.g_pre == -77.0).all(), "a call from t0 = 5 wrote io->g_pre"
    # (its actions are its own policy evaluations on equal observations: the same kernel code, the same bits)
    assert torch.equal(o5["a"], out["a"][5:]) and torch.equal(o5["g"], out["g"][5:]) and torch.equal(o5["viol"], viol[5:])
    for e in (ef, es, e5, e0):
        e.close()
    pol.close()


# ---- 3. chunks and layouts -------------------------------------------------------------------------------------------------------
GUARD = 64


def _guarded(shape, dtype, dev):
    """a buffer of `shape` between two guard zones of a sentinel: (whole, view)"""
    torch = _torch()
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), 123 if dtype == torch.uint8 else -4242.0, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + n].view(*shape)


def _guards_ok(whole, dtype):
    s = 123 if dtype == _torch().uint8 else -4242.0
    return bool((whole[:GUARD] == s).all() and (whole[-GUARD:] == s).all())


def _raw_policy_call(env, pol, T, a, obs, rew, g, g_strides, viol, record_next=0):
    """pcg_rollout_policy_cons on caller-made buffers (step-major a / obs / rew); advances env.t"""
    s, nb = env.spec, env.B
    env._buf.d = None
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = env._lib.pcg_rollout_policy_cons(env._plan, env._bufp, pol.handle(env.device), env.t, T, ptr(a), s.na * nb, nb, ptr(obs),
                                          s.nobs * nb, nb, ptr(rew), nb, record_next, ptr(g), g_strides[0], g_strides[1], ptr(viol), nb,
                                          env._episode_seed(), env._stream())
    if rc == 0:
        env.t += T
    return rc


def test_chunks_layouts_nulls_and_guards():
    torch = _torch()
    p = _plan("cstr", "rk4")[0]
    e1, ec, eg, en = _pair(p, 4)
    spec, dev = e1.spec, e1.device
    T, f64, u8 = spec.N - 1, torch.float64, torch.uint8
    pol = make_policy(spec, e1.obs_soa.cpu().numpy(), (16,), seed=17)
    one = e1.rollout_policy_cons(pol, T, collect_obs=True, record_next_action=True)
    # ---- 1 + 7 + rest steps equal the single call; row T of record_next_action as in the single call ----
    parts, done = [], 0
    for n in (1, 7, T - 8):
        parts.append(ec.rollout_policy_cons(pol, n, collect_obs=True, record_next_action=(done + n == T)))
        done += n
    torch.cuda.synchronize()
    for k in ("obs", "rew", "g", "viol"):
        assert torch.equal(torch.cat([q[k] for q in parts]), one[k]), f"chunked {k}"
    assert torch.equal(torch.cat([parts[0]["a"], parts[1]["a"], parts[2]["a"]]), one["a"]) and one["a"].shape[0] == T + 1
    _check_final(ec, e1)
    # ---- guarded buffers; rows in the reference's axis order (ncon, T, B) against step-major ----
    bufs = {"a": _guarded((T + 1, spec.na, B), f64, dev), "obs": _guarded((T, spec.nobs, B), f64, dev), "rew": _guarded((T, B), f64, dev),
            "g": _guarded((spec.ncon, T, B), f64, dev), "viol": _guarded((T, B), u8, dev)}
    rc = _raw_policy_call(eg, pol, T, bufs["a"][1], bufs["obs"][1], bufs["rew"][1], bufs["g"][1], (B, T * B), bufs["viol"][1], 1)
    torch.cuda.synchronize()
    assert rc == 0
    for k in ("a", "obs", "rew"):
        assert torch.equal(bufs[k][1], one[k]), k
    assert torch.equal(bufs["g"][1].permute(1, 0, 2), one["g"]), "rows in the reference's axis order differ from step-major rows"
    assert torch.equal(bufs["viol"][1].view(torch.bool), one["viol"])
    for k, (whole, view) in bufs.items():
        assert _guards_ok(whole, view.dtype), f"guard bytes around {k} were written"
    _check_final(eg, e1)
    # ---- NULL g_seq, NULL viol_seq, both: the other outputs unchanged ----
    for no_g, no_v in ((True, False), (False, True), (True, True)):
        en.reset(), e1.reset()  # (both open the same next episode: equal RNG epoch; the cstr plan draws only its x0)
        full = e1.rollout_policy_cons(pol, T, collect_obs=True)
        got = en.rollout_policy_cons(pol, T, collect_obs=True, collect_g=not no_g, collect_viol=not no_v)
        torch.cuda.synchronize()
        assert (got["g"] is None) == no_g and (got["viol"] is None) == no_v
        for k in ("a", "obs", "rew") + (() if no_g else ("g",)) + (() if no_v else ("viol",)):
            assert torch.equal(got[k], full[k]), (k, no_g, no_v)
        _check_final(en, e1)
    for e in (e1, ec, eg, en):
        e.close()
    pol.close()


def test_odd_batch_against_the_classic_per_step_kernel():
    """B = 577: the per-step route cannot take the two-envs-per-lane kernel.  Rows within the oracle comparison's tolerance of
    the per-step route's, flags equal except where |g| is below it."""
    torch = _torch()
    p = _plan("cstr", "rk4")[0]
    ef, es = _pair(p, 2, nb=577)
    spec = ef.spec
    T = spec.N - 1
    pol = make_policy(spec, ef.obs_soa.cpu().numpy(), (16,), seed=17)
    out = ef.rollout_policy_cons(pol, T, collect_obs=True)
    ref = _stepped(es, out["a"], T)
    torch.cuda.synchronize()
    assert _launched(ef._lib, "rollout_cons_policy_kernel")
    g, gr = out["g"].cpu().numpy(), ref["g"].cpu().numpy()
    x = ref["x0"].cpu().numpy()
    tol = G_TOL * _row_scale(spec, x, np.asarray(spec.o_high, dtype=float)[spec.nx:], np.abs(np.concatenate([spec.a_low, spec.a_high])))
    print(f"odd batch: rows at most {np.max(np.abs(g - gr)):.3e} from the per-step route (tolerance {tol:.3e})")
    assert np.all(np.abs(g - gr) <= tol)
    sure = np.abs(gr[:, 0]) >= tol
    assert np.array_equal(out["viol"].cpu().numpy()[sure], ref["viol"].cpu().numpy().astype(bool)[sure])
    ef.close(), es.close(), pol.close()


# ---- 4. refusals launch nothing --------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    torch = _torch()
    from pcgym_amd import GaussianActorCritic, MLPPolicy
    from pcgym_amd import _abi as abi
    from test_policy_jit_plans import _chemostat

    UNS, DIM, VAL, NUL, PLAN = abi.PCG_E_UNSUPPORTED, abi.PCG_E_DIM, abi.PCG_E_VALUE, abi.PCG_E_NULL, abi.PCG_E_PLAN
    cons = _plan("cstr", "rk4")[0]
    seen = []

    def attempt(env, want, pol, critic="same", sigma="ok", T=3, t0=None, g_strides=None, v_stride=None, head="policy", buf=None):
        """one refused call of each entry point's kind; state, observation and pre-filled outputs unchanged"""
        s, nb, dev = env.spec, env.B, env.device
        nc = max(s.ncon, 1)
        x, o = env.x.clone(), env.obs_soa.clone()
        outs = [torch.full(shape, -5.5, dtype=torch.float64, device=dev) for shape in
                ((T + 1, s.na, nb), (T + 1, s.na, nb), (T + 1, nb), (T + 1, nb), (T, s.nobs, nb), (T, nb), (T, nc, nb))]
        viol = torch.full((T, nb), 9, dtype=torch.uint8, device=dev)
        a, u, lp, val, ob, rw, g = outs
        gs, gc = g_strides if g_strides else (nc * nb, nb)
        vs = nb if v_stride is None else v_stride
        t0 = env.t if t0 is None else t0
        bufp = env._bufp if buf is None else C.byref(buf)
        h = pol.handle(dev) if hasattr(pol, "handle") else pol
        if head == "policy":
            rc = env._lib.pcg_rollout_policy_cons(env._plan, bufp, h, t0, T, a.data_ptr(), s.na * nb, nb, ob.data_ptr(), s.nobs * nb, nb,
                                                  rw.data_ptr(), nb, 1, g.data_ptr(), gs, gc, viol.data_ptr(), vs, 7, env._stream())
        else:
            cr = critic.handle(dev) if hasattr(critic, "handle") else critic
            sg = None if sigma is None else np.ascontiguousarray(sigma, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
            rc = env._lib.pcg_rollout_actor_cons(env._plan, bufp, h, cr, sg, t0, T, a.data_ptr(), s.na * nb, nb, u.data_ptr(), s.na * nb, nb,
                                                 lp.data_ptr(), nb, val.data_ptr(), nb, ob.data_ptr(), s.nobs * nb, nb, rw.data_ptr(), nb, 1,
                                                 g.data_ptr(), gs, gc, viol.data_ptr(), vs, 7, env._stream())
        torch.cuda.synchronize()
        assert rc == want, (len(seen), rc, want)
        assert torch.equal(env.x, x) and torch.equal(env.obs_soa, o)
        assert all(bool((t == -5.5).all()) for t in outs) and bool((viol == 9).all())
        seen.append(rc)

    def nets(spec, dtype="float64"):
        rng = np.random.default_rng(0)
        Ws = [rng.standard_normal((16, spec.nobs)) / 4, rng.standard_normal((spec.na, 16)) / 4]
        bs = [np.zeros(16), np.zeros(spec.na)]
        pol = MLPPolicy(Ws, bs, dtype=dtype)
        cr = MLPPolicy([Ws[0], Ws[1][:1]], [bs[0], bs[1][:1]], out_map="none", dtype=dtype)
        return pol, cr

    # ---- the plans: PCG_E_UNSUPPORTED, in the header's order ----
    plain = copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"])
    plain.update(integrator="rk4")
    chem0 = _make(_chemostat(integrator="rk4"), 2)
    nst = chem0.spec.nobs
    chem = _chemostat(integrator="rk4", constraints={"A": np.ones((1, nst + chem0.spec.nu)), "b": np.array([1.0])},
                      done_on_cons_vio=False, r_penalty=True)
    chem0.close()
    unc = copy.deepcopy(cons)
    unc.update(uncertainty_percentages={"q": 0.03, "x0": [0.01] * 24}, distribution="uniform",
               uncertainty_bounds={"low": np.array([90.0]), "high": np.array([110.0])})
    dopri = copy.deepcopy(cons)
    dopri.update(integrator="dopri5")
    sig_of = lambda spec: np.full(spec.na, 0.3)  # noqa: E731
    for params, kw in ((plain, {}), (chem, {}), (cons, dict(per_env_t=True)), (unc, {}), (dopri, {})):
        env = _make(params, 64, seed=3, **kw)
        env.reset()
        pol, cr = nets(env.spec)
        attempt(env, UNS, pol)
        attempt(env, UNS, pol, critic=cr, sigma=sig_of(env.spec), head="actor")
        env.close(), pol.close(), cr.close()
    env = _make(cons, 64, seed=3)
    env.reset()
    spec = env.spec
    pol, cr = nets(spec)
    p32, c32 = nets(spec, "float32")
    sig = sig_of(spec)
    attempt(env, UNS, p32)
    attempt(env, UNS, p32, critic=c32, sigma=sig, head="actor")
    attempt(env, UNS, pol, critic=c32, sigma=sig, head="actor")
    # ---- everything else, in the unconstrained calls' order ----
    junk = C.cast(C.create_string_buffer(512), C.c_void_p)
    attempt(env, NUL, None)
    attempt(env, PLAN, junk)
    wrong = MLPPolicy([np.zeros((spec.na, spec.nobs + 1))], [np.zeros(spec.na)])
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
        attempt(env, DIM, pol, g_strides=(spec.ncon * env.B, env.B - 1), **kw)   # g_comp_stride < B
        attempt(env, DIM, pol, v_stride=env.B - 1, **kw)                         # viol_step_stride < B with T > 1
        attempt(env, DIM, pol, g_strides=(env.B - 1, 3 * env.B), **kw)           # rows that overlap: neither layout
    assert len(seen) == 34 and not _launched(env._lib, "rollout_cons_")
    env.close()
    for q in (pol, cr, p32, c32, wrong, cmap, tanh):
        q.close()


# ---- 5. collectors ----------------------------------------------------------------------------------------------------------------
def _showcase():
    p = copy.deepcopy(SC.scenarios()["cstr_cons_pen_norm"]["env_params"])
    p.update(integrator="rk4")
    return _spread_x0(p, 0.01)


def test_collect_rollouts_takes_the_fused_call():
    torch = _torch()
    from pcgym_amd import collect_rollouts

    ef, es, er = _pair(_showcase(), 3)  # (collect_rollouts resets again: the envs stay in the same RNG epoch)
    spec = ef.spec
    N = spec.N
    pol = make_policy(spec, ef.obs_soa.cpu().numpy(), (16,), seed=23)
    fused = collect_rollouts(ef, policy=pol)
    torch.cuda.synchronize()
    assert _launched(ef._lib, "rollout_cons_policy_kernel"), "collect_rollouts did not take the fused constrained call"
    # the callable route, teacher-forced: a callable that replays the policy outputs the same kernel records
    er.reset()
    a_seq = er.rollout_policy_cons(pol, N - 1, record_next_action=True)["a"]
    step = iter(range(N))
    ref = collect_rollouts(es, policy=lambda o: a_seq[next(step)])
    torch.cuda.synchronize()
    assert next(step, None) is None
    assert set(fused) == set(ref) == {"r", "x", "u", "g"}
    assert fused["g"].shape == (spec.ncon, N, 1, B)
    for k in ("r", "x", "u", "g"):
        assert fused[k].shape == ref[k].shape and torch.equal(fused[k], ref[k]), k
    assert 0.0 < float((fused["g"][:, 1:] > 0).float().mean()) < 1.0
    _check_final(ef, es)
    for e in (ef, es, er):
        e.close()
    pol.close()


def test_collect_onpolicy_records_the_rows():
    torch = _torch()
    from helpers import _perm_hidden
    from pcgym_amd import GaussianActorCritic, collect_onpolicy

    ef, es, e2, en = _pair(_showcase(), 4)  # (collect_onpolicy resets again: the envs stay in the same RNG epoch)
    spec = ef.spec
    T = spec.N - 1
    ac = make_ac(spec, ef.obs_soa.cpu().numpy(), (16,), seed=23, sigma_scale=0.1)
    ac2 = GaussianActorCritic(_perm_hidden(ac.actor, 5), ac.log_std, _perm_hidden(ac.critic, 6))
    fused = collect_onpolicy(ef, ac, record_cons=True)
    torch.cuda.synchronize()
    assert _launched(ef._lib, "rollout_cons_actor_kernel"), "collect_onpolicy(record_cons=True) did not take the fused call"
    ref = collect_onpolicy(es, ac, record_cons=True, fused=False)
    ref2 = collect_onpolicy(e2, ac2, record_cons=True, fused=False)
    torch.cuda.synchronize()
    assert set(fused) == set(ref) == {"obs", "act", "logp", "val", "rew", "adv", "ret", "g", "g_pre", "viol"}
    assert fused["g"].shape == (T, spec.ncon, B) and fused["g_pre"].shape == (spec.ncon, B) and fused["viol"].shape == (T, B)
    assert fused["viol"].dtype == ref["viol"].dtype == torch.bool
    # the torch route rounds the networks differently: as in tests/test_gpu_actor_rollout.py the fused result has to lie within
    # 8 x the spread of two per-step runs under a hidden-unit permutation (+ 1e-13), each array relative to max(1, its largest
    # entry); rewards only where no row is that close to zero on any run (the penalty may fall either way there)
    assert torch.equal(fused["logp"], ref["logp"]) and torch.equal(fused["g_pre"], ref["g_pre"]) and torch.equal(fused["obs"][0], ref["obs"][0])

    def dist(a, b, k, mask=None):
        d, scale = (a[k] - b[k]).abs(), max(1.0, float(b[k].abs().max()))
        return float((d if mask is None else d[mask]).max()) / scale

    spread_g = dist(ref2, ref, "g")
    near = ((ref["g"].abs() <= (8 * spread_g + 1e-13) * max(1.0, float(ref["g"].abs().max()))).any(1))
    assert float(near.float().mean()) < 0.01
    for k in ("obs", "act", "val", "g", "rew"):
        mask = ~near if k == "rew" else None
        spread, d = dist(ref2, ref, k, mask), dist(fused, ref, k, mask)
        print(f"collect_onpolicy record_cons {k}: per-step spread {spread:.3e}, fused vs per-step {d:.3e}")
        assert spread > 0 and d <= 8 * spread + 1e-13, (k, d, spread)
    assert torch.equal(fused["viol"][~near], ref["viol"][~near])
    assert torch.equal(fused["viol"], (fused["g"] > 0).any(1)) and torch.equal(ref["viol"], (ref["g"] > 0).any(1))
    # bit for bit: the step loop on the applied actions of the fused record (out_map of the recorded samples)
    en.reset()
    rep = _stepped(en, ac.action(fused["act"]), T)
    torch.cuda.synchronize()
    assert torch.equal(rep["g"], fused["g"]) and torch.equal(rep["viol"].view(torch.bool), fused["viol"])
    assert torch.equal(rep["obs"], fused["obs"][1:]) and torch.equal(rep["rew"], fused["rew"]) and torch.equal(rep["g_pre"], fused["g_pre"])
    _check_final(ef, en)
    with pytest.raises(ValueError):
        collect_onpolicy(en, ac, fused=True)  # without record_cons a constrained plan still has no fused call
    for e in (ef, es, e2, en):
        e.close()
    ac.close(), ac2.close()


def test_record_cons_false_changes_nothing():
    torch = _torch()
    from pcgym_amd import collect_onpolicy

    (env,) = _pair(_showcase(), 1)
    ac = make_ac(env.spec, env.obs_soa.cpu().numpy(), (16,), seed=23)
    out = collect_onpolicy(env, ac)
    torch.cuda.synchronize()
    assert set(out) == {"obs", "act", "logp", "val", "rew", "adv", "ret"}
    assert not _launched(env._lib, "rollout_cons_") and not _launched(env._lib, "rollout_actor_kernel")
    plain = copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"])
    plain.update(integrator="rk4")
    e2 = _make(plain, 64, seed=1)
    ac2 = make_ac(e2.spec, e2.reset()[0].t().cpu().numpy(), (16,), seed=23)
    with pytest.raises(ValueError):
        collect_onpolicy(e2, ac2, record_cons=True)
    env.close(), e2.close(), ac.close(), ac2.close()


def test_the_call_is_capture_safe():
    torch = _torch()
    (ee, eg) = _pair(_showcase(), 2)
    spec = ee.spec
    T = 12
    pol = make_policy(spec, ee.obs_soa.cpu().numpy(), (16,), seed=23)
    eager = ee.rollout_policy_cons(pol, T, collect_obs=True)
    pol.handle(eg.device)
    torch.cuda.synchronize()
    x0, o0, t0 = eg.x.clone(), eg.obs_soa.clone(), eg.t
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            cap = eg.rollout_policy_cons(pol, T, collect_obs=True)
    torch.cuda.current_stream().wait_stream(side)
    eg.x.copy_(x0), eg.obs_soa.copy_(o0)
    for k in ("a", "obs", "rew", "g"):
        cap[k].fill_(0.0)
    graph.replay()
    torch.cuda.synchronize()
    assert eg.t == t0 + T
    for k in ("a", "obs", "rew", "g", "viol"):
        assert torch.equal(cap[k], eager[k]), k
    _check_final(eg, ee)
    ee.close(), eg.close(), pol.close()
