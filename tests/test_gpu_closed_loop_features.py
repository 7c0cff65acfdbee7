"""GPU: the fused closed-loop rollouts on the feature plans of helpers.FEATURE_PLANS -- the tracking reward with io->u_prev, its
box excess and its crystallisation form, disturbance schedules with and without a Gaussian part, dense constraint rows over
disturbance columns, masked observations, the terminal reward, per-env parameters next to disturbance slots (quirk Q11 among
them).  tests/test_closed_loop_feature_plans.py shows on the oracle alone that every case really takes its branch; the cases,
their networks and their row bounds are that file's (feature_case), B = 578, T = N - 1: every schedule change and the terminal
step lie inside the one call.

Each family is held by its own file's method and tolerances; nothing here is new:
  base      tests/test_gpu_policy_rollout.py / test_gpu_actor_rollout.py: recorded outputs inside helpers.host_reference's running
            bound on the kernel's own observations; the recorded actions through the open-loop rollout of a variant-1 env
            bitwise (io->u_prev and a_save_t included); one call per step bitwise the one call; every step against the oracle
            from the common start state: state 1e-12 of max(|x|, 1), reward rtol 1e-9 / atol 1e-10 (1 + max|r|), observation
            rtol 1e-10 / atol 1e-11 where the plan has no observation noise.  After the call io->u_prev against the oracle's
            previous action, rtol 1e-15.
  float32   the same plans under RK4 through tests/test_gpu_policy_f32.py's reference (bound32: the observation rounded to
            float32 first) and bounds.
  cons      tests/test_gpu_cons_rollout.py: the per-step route teacher-forced on the recorded actions, obs / rew / g / viol /
            done and the final buffers bitwise (helpers._check_final, its u_prev branch live here); the oracle per step: every
            row within G_TOL x its row scale, flags and rewards wherever |g| > tol on EVERY row, at most 1 % excluded.
  unc       tests/test_gpu_unc_rollout.py: every step against the oracle at helpers._tols; one call against chunks (1, 2, rest)
            and against one call per step bitwise, u_prev compared as it is; the networks on the kernel's own observations;
            io->p_unc unchanged.

Measured figures are printed in the other files' "case ...:" format and, when PCG_RECORD_DIR names a directory, appended to
closed_loop_features_test.txt there.  First run on an MI355X, 97 cases in 15 s:
  base      32 cases: outputs <= 0.13 x their running bound, state <= 7.0e-15 from the oracle (bar 1e-12)
  float32   16 cases: outputs <= 0.13 x the float32 bound, state <= 7.2e-15
  cons      20 cases: outputs <= 0.49 x bound, rows <= 2.6e-4 x the row tolerance, no entry excluded (cap 1 %); the showcase's box
            term on 492-552 of 34,102 entries on its upper branch and 6,859-22,224 on its lower
  unc       24 cases: outputs <= 0.60 x bound, state <= 8.1e-15 (bar 1e-8)

What the file found: test_constrained_family[cstr_con_reward-rk4-actor] -- rewards of rollout_cons_actor_kernel<cstr, RK4> one
ulp from the feature-masked step kernel's on the same actions, everything else bitwise.  The three restatements of the tracking
reward (env_post, env_step_feat, env_post_cons) were each contracted by the compiler on its own; its accumulating terms are now
the shared contraction-free track_*_cost of pcg_kernels.hpp, in the oracle's order.

Three deliberately wrong builds of the kernels as they were before that change, each run through this file and through
tests/test_gpu_cons_rollout.py + tests/test_gpu_unc_rollout.py (143 tests, which passed all three):
  env_post_cons reads x instead of the noisy on[] for the tracked value: the four cstr_con_reward_noise cases of
      test_constrained_family fail (rew differs from the per-step route);
  policy_input_unc places ounc at nx + nso + j: the eight unc_cstr_dist_Ti / unc_cstr_dist_Ti_Caf cases of
      test_per_env_parameter_family and both cases of test_the_policy_reads_disturbance_and_parameter_slots fail;
  cons_rows skips the dv columns: the four cstr_dist_both_rows8 cases of test_constrained_family and
      test_dense_rows_odd_batch_against_the_classic_per_step_kernel fail.
"""
import numpy as np
import pytest

from helpers import (BASE_FEATURE_PLANS, CONS_FEATURE_PLANS, FEATURE_PLANS, LD, PRE_MAX, U, UNC_FEATURE_PLANS, _check_final, _final_equal,
                     _launched, _make, _perm_hidden, _rew_close, _stepped, _tols, _torch, host_reference, tanh_k, worst_rel)
from helpers import _record as _record_to
from test_closed_loop_feature_plans import B, G_TOL, SEED, THREADS, box_branches, build_net, case_params, feature_case, row_scales, u_box
from test_gpu_actor_rollout import logp_numpy, raw_twin

pytestmark = pytest.mark.gpu


def _record(line):
    _record_to("closed_loop_features_test.txt", line)


def _envs(p, n, nb=B, **kw):
    envs = [_make(p, nb, seed=SEED, **kw) for _ in range(n)]
    for e in envs:
        e.reset()
    return envs


def _forget_launches(env):
    """empty the launch record, so that _launched() afterwards speaks of this test's own calls"""
    env._lib.pcg_coverage_names(None, 0, 1)


def _oracle(spec, nb=B):
    from oracle import oracle as O

    orc = O.OracleEnv(spec, nb, seed=SEED, n_threads=THREADS)
    orc.reset()
    return orc


def _check_networks(head, net, out, obs0, noise, T, f32=False):
    """every recorded row 0 .. T of the networks' outputs on the kernel's OWN observations: the policy inside its running bound;
    the actor's a == out_map(u) and logp bitwise, sample and value inside theirs.  Returns the worst error / bound ratio."""
    if f32:
        from test_gpu_policy_f32 import is_f32, raw32, tanh32_k
        from test_policy_f32 import bound32 as ref_of

        k = tanh32_k()
    else:
        ref_of, k = host_reference, tanh_k()
    a_np, o_np = out["a"].cpu().numpy(), out["obs"].cpu().numpy()
    assert a_np.shape[0] == T + 1 and np.isfinite(a_np).all() and np.isfinite(o_np).all()
    worst, pre = 0.0, 0.0
    if head == "policy":
        for s in range(T + 1):
            ref, bound, pm = ref_of(net, obs0 if s == 0 else o_np[s - 1], k + 1.0)
            pre = max(pre, pm)
            diff = np.abs(a_np[s].astype(LD) - ref).astype(np.float64)
            assert np.all(diff <= bound), f"step {s}: policy output off by {np.max(diff):.3e} (bound {np.max(bound):.3e})"
            worst = max(worst, float(np.max(diff / np.maximum(bound, 1e-300))))
        inside = float(np.mean((a_np > net.out_low) & (a_np < net.out_high)))
        assert inside >= 0.25, f"only {inside:.2f} of the recorded actions lie strictly inside the clip box"
        assert not f32 or is_f32(a_np)
    else:
        u_np, lp_np, v_np = (out[n].cpu().numpy() for n in ("u", "logp", "val"))
        pol, cr = net.actor, net.critic
        raw, sig = (raw32(pol) if f32 else raw_twin(pol)), net.sigma[:, None]
        if pol.out_map == "clip":
            assert np.array_equal(a_np, np.clip(u_np, pol.out_low, pol.out_high)), "a is not clip(u) bitwise"
            assert np.any(a_np != u_np) and np.any(a_np == u_np)
        else:
            assert np.array_equal(a_np, u_np)
        for s in range(T + 1):
            z = noise(s)
            o_in = obs0 if s == 0 else o_np[s - 1]
            mu, b_mu, pm = ref_of(raw, o_in, k + 1.0)
            pre = max(pre, pm)
            diff = np.abs(u_np[s].astype(LD) - (mu + sig.astype(LD) * z.astype(LD))).astype(np.float64)
            bound = b_mu + U * np.abs(u_np[s])
            assert np.all(diff <= bound), f"step {s}: sample off by {np.max(diff):.3e}"
            worst = max(worst, float(np.max(diff / np.maximum(bound, 1e-300))))
            assert np.array_equal(lp_np[s], logp_numpy(net, z)), f"step {s}: logp is not the specified operation sequence"
            vr, b_v, pm = ref_of(cr, o_in, k + 1.0)
            pre = max(pre, pm)
            dv = np.abs(v_np[s].astype(LD) - vr[0]).astype(np.float64)
            assert np.all(dv <= b_v[0]), f"step {s}: value outside its bound"
            worst = max(worst, float(np.max(dv / np.maximum(b_v[0], 1e-300))))
        assert not f32 or (is_f32(v_np) and not is_f32(u_np))
        raw.close()
    assert pre <= PRE_MAX
    assert np.std(a_np) > 0
    return worst


# ---- 1. the base float64 and float32 families -------------------------------------------------------------------------------------
def _call(env, head, net, T, nxt):
    if head == "policy":
        a, o, r = env.rollout_policy(net, T, collect_obs=True, collect_rew=True, record_next_action=nxt)
        return {"a": a, "obs": o, "rew": r}
    return env.rollout_actor(net, T, collect_obs=True, collect_rew=True, record_next_action=nxt)


def _base_case(plan, integ, head, f32):
    torch = _torch()
    spec_h, net, ep, cand = feature_case(plan, integ, head)
    if f32:
        from test_gpu_policy_f32 import ac32, to32

        net = to32(net) if head == "policy" else ac32(net)
    p = case_params(plan, integ, spec_h)
    e_one, e_chain = _envs(p, 2)
    (e_open,) = _envs(p, 1, variant=1)  # PCG_OPT_VARIANT 1: the general kernels
    spec = e_one.spec
    T = spec.N - 1
    assert spec.integrator == integ and not spec.ncon and not spec.nunc and spec.x0_unc is not None and T <= 59
    kinds = FEATURE_PLANS[plan][2]
    assert ("track" in kinds) == (e_one.u_prev is not None) and ("dist" in kinds) == (spec.nd > 0)
    obs0, x0 = e_one.obs_soa.cpu().numpy().copy(), e_one.x.cpu().numpy().copy()
    if e_one.u_prev is not None:
        assert torch.isnan(e_one.u_prev).all()  # "no previous action yet"
    _forget_launches(e_one)
    out = _call(e_one, head, net, T, True)
    torch.cuda.synchronize()
    kernel = f"rollout_{head}_kernel" + ("_f32" if f32 else "")
    assert _launched(e_one._lib, kernel) and (f32 or not _launched(e_one._lib, kernel + "_f32")) and not e_one.status.any()
    a_seq, obs_seq, rew_seq = out["a"], out["obs"], out["rew"]
    assert torch.equal(e_one.obs_soa, obs_seq[T - 1]) and torch.equal(e_one.rew, rew_seq[T - 1]) and e_one.t == T
    worst = _check_networks(head, net, out, obs0, lambda s: e_open.policy_noise(s).cpu().numpy(), T, f32)

    # ---- the recorded actions through the open-loop rollout, general kernel: bitwise, io->u_prev and a_save_t included ----
    assert np.array_equal(e_open.x.cpu().numpy(), x0)
    oq, rq = e_open.rollout(a_seq[:T].contiguous(), collect_obs=True, collect_rew=True)
    torch.cuda.synchronize()
    assert torch.equal(oq, obs_seq), "observations differ from the open-loop replay of the recorded actions"
    assert torch.equal(rq, rew_seq), "rewards differ from the open-loop replay"
    assert torch.equal(e_open.x, e_one.x) and torch.equal(e_open.done, e_one.done) and torch.equal(e_open.status, e_one.status)
    if spec.a_delta:
        assert torch.equal(e_open.a_save_t, e_one.a_save_t)
    if e_one.u_prev is not None:
        assert torch.isfinite(e_one.u_prev).all() and torch.equal(e_open.u_prev, e_one.u_prev), "io->u_prev differs from the replay's"

    # ---- one call per step == the one call, bitwise; every step against the oracle from the common start state ----
    orc = _oracle(spec)
    assert np.allclose(orc.x, x0, rtol=1e-14, atol=0)
    a_np, worst_x = a_seq.cpu().numpy(), 0.0
    for s in range(T):
        x_before = e_chain.x.cpu().numpy().copy()
        o1 = _call(e_chain, head, net, 1, s == T - 1)
        torch.cuda.synchronize()
        for n in o1:
            if o1[n] is not None:
                assert torch.equal(o1[n][0], out[n][s]), f"chained call {s}: {n}"
                assert s < T - 1 or n in ("obs", "rew") or torch.equal(o1[n][1], out[n][T]), f"chained call {s}: row T of {n}"
        orc.x[:] = x_before
        oc, rc, dc = orc.step(a_np[s])
        xg = e_chain.x.cpu().numpy()
        assert np.isfinite(orc.x).all()
        err = float(np.max(np.abs(xg - orc.x) / np.maximum(np.abs(orc.x), 1.0)))
        worst_x = max(worst_x, err)
        assert err <= 1e-12, f"step {s}: state {err:.3e} from the oracle (relative to max(|x|, 1))"
        assert np.array_equal(e_chain.done.cpu().numpy(), dc)
        if not spec.noise:
            assert np.allclose(o1["obs"][0].cpu().numpy(), oc, rtol=1e-10, atol=1e-11), f"step {s}: observation"
        assert np.allclose(o1["rew"][0].cpu().numpy(), rc, rtol=1e-9, atol=1e-10 * (1 + np.max(np.abs(rc)))), f"step {s}: reward"
    assert torch.equal(e_chain.x, e_one.x)
    if e_one.u_prev is not None:
        assert torch.equal(e_chain.u_prev, e_one.u_prev)
        assert np.allclose(e_one.u_prev.cpu().numpy(), orc.u_prev, rtol=1e-15, atol=0), "io->u_prev is not the oracle's previous action"
    if "batch" in kinds:
        assert bool((rew_seq[:-1] == 0).all()) and bool((rew_seq[-1] != 0).all())
    _record(f"case {plan}-{integ}-{head}{'-f32' if f32 else ''}: network {cand}, output error <= {worst:.3f} x bound, state vs oracle {worst_x:.2e}")
    for e in (e_one, e_chain, e_open):
        e.close()
    if f32:
        net.close()


@pytest.mark.parametrize("head", ["policy", "actor"])
@pytest.mark.parametrize("integ", ["rk4", "cv8"])
@pytest.mark.parametrize("plan", BASE_FEATURE_PLANS)
def test_base_family(plan, integ, head):
    _base_case(plan, integ, head, False)


@pytest.mark.parametrize("head", ["policy", "actor"])
@pytest.mark.parametrize("plan", BASE_FEATURE_PLANS)
def test_float32_family(plan, head):
    _base_case(plan, "rk4", head, True)


# ---- 2. the constrained family --------------------------------------------------------------------------------------------------------
def _cons_call(env, head, net, T, **kw):
    return (env.rollout_policy_cons if head == "policy" else env.rollout_actor_cons)(net, T, collect_obs=True, **kw)


@pytest.mark.parametrize("head", ["policy", "actor"])
@pytest.mark.parametrize("integ", ["rk4", "cv8"])
@pytest.mark.parametrize("plan", CONS_FEATURE_PLANS)
def test_constrained_family(plan, integ, head):
    torch = _torch()
    spec_h, net, ep, cand = feature_case(plan, integ, head)
    p = case_params(plan, integ, spec_h)
    ef, es = _envs(p, 2)
    spec = ef.spec
    T = spec.N - 1
    kinds = FEATURE_PLANS[plan][2]
    assert spec.ncon >= 1 and spec.integrator == integ and spec.user_cons_src is None and np.array_equal(spec.con_b, spec_h.con_b)
    assert ("track" in kinds) == (ef.u_prev is not None)
    obs0 = ef.obs_soa.cpu().numpy().copy()
    assert torch.equal(ef.x, es.x)
    _forget_launches(ef)
    out = _cons_call(ef, head, net, T, record_next_action=True)
    torch.cuda.synchronize()
    assert _launched(ef._lib, f"rollout_cons_{head}_kernel") and not ef.status.any()
    assert out["g"].shape == (T, spec.ncon, B) and out["viol"].shape == (T, B) and out["viol"].dtype == torch.bool
    worst = _check_networks(head, net, out, obs0, lambda s: es.policy_noise(s).cpu().numpy(), T)

    # ---- the per-step route on the recorded actions: bit for bit ----
    ref = _stepped(es, out["a"], T)
    torch.cuda.synchronize()
    for n in ("obs", "rew", "g"):
        assert torch.equal(out[n], ref[n]), f"{n} differs from the per-step route"
    assert torch.equal(out["viol"], ref["viol"].view(torch.bool)), "viol differs from the per-step route"
    assert torch.equal(ef.done, ref["done"][-1])
    assert ef.u_prev is None or bool(torch.isfinite(ef.u_prev).all())
    _check_final(ef, es)  # (its u_prev branch is live on the tracking plans)
    share = float(ref["viol"].float().mean())
    assert 0.05 <= share <= 0.95, f"{share:.3f} of the entries violate: the rows do not split the case"
    if "box" in kinds:  # both excess branches of the box term on the device's own record
        upper, lower = box_branches(spec, out["obs"].cpu().numpy(), out["viol"].cpu().numpy())
        print(f"case {plan}-{integ}-{head}: box excess, {int(upper.sum())} of {upper.size} entries on the upper branch, {int(lower.sum())} on the lower")
        assert upper.sum() >= 0.01 * upper.size and lower.sum() >= 0.01 * lower.size

    # ---- the oracle, every step from the per-step route's own start state ----
    orc = _oracle(spec)
    x0s, g_np, r_np, v_np = ref["x0"].cpu().numpy(), ref["g"].cpu().numpy(), ref["rew"].cpu().numpy(), ref["viol"].cpu().numpy()
    a_np = out["a"].cpu().numpy()
    assert np.allclose(orc.x, x0s[0], rtol=1e-14, atol=0)
    worst_g, unsure = 0.0, 0
    for s in range(T):
        orc.x[:] = x0s[s]
        _, rc, _ = orc.step(a_np[s])
        assert np.isfinite(orc.g).all() and np.isfinite(rc).all()
        tol = G_TOL * row_scales(spec, orc.x, orc.slots, u_box(spec, a_np[s]))[:, None]
        dg = np.abs(g_np[s] - orc.g)
        worst_g = max(worst_g, float(np.max(dg / tol)))
        assert np.all(dg <= tol), f"step {s}: a row {np.max(dg / tol):.3e} x its tolerance from the oracle"
        sure = np.all(np.abs(orc.g) > tol, axis=0)
        unsure += int(np.sum(~sure))
        assert np.array_equal(v_np[s][sure], orc.viol[sure]), f"step {s}: flags differ from the oracle's"
        assert np.allclose(r_np[s][sure], rc[sure], rtol=1e-9, atol=1e-10 * (1 + np.max(np.abs(rc)))), f"step {s}: reward"
    assert unsure <= 0.01 * T * B, f"{unsure} of {T * B} entries have a row within its tolerance of zero"
    if ef.u_prev is not None:
        assert np.allclose(ef.u_prev.cpu().numpy(), orc.u_prev, rtol=1e-15, atol=0), "io->u_prev is not the oracle's previous action"
    _record(f"case {plan}-{integ}-{head}: network {cand}, output error <= {worst:.3f} x bound, {share:.3f} of the entries violate, "
            f"rows within {worst_g:.2e} x the oracle tolerance, {unsure} entries excluded")
    ef.close(), es.close()


def test_dense_rows_odd_batch_against_the_classic_per_step_kernel():
    """B = 577: the per-step route cannot take the two-envs-per-lane kernel, so the two routes sum the rows in different orders,
    which differ in where the disturbance columns enter"""
    torch = _torch()
    plan = "cstr_dist_both_rows8"
    spec_h, pol, ep, cand = feature_case(plan, "rk4", "policy")
    ef, es = _envs(case_params(plan, "rk4", spec_h), 2, nb=577)
    spec = ef.spec
    T = spec.N - 1
    _forget_launches(ef)
    out = ef.rollout_policy_cons(pol, T, collect_obs=True)
    ref = _stepped(es, out["a"], T)
    torch.cuda.synchronize()
    assert _launched(ef._lib, "rollout_cons_policy_kernel") and not ef.status.any()
    g, gr, x = out["g"].cpu().numpy(), ref["g"].cpu().numpy(), ref["x0"].cpu().numpy()
    tol = G_TOL * row_scales(spec, x, np.asarray(spec.o_high, dtype=float)[spec.nx:], np.max(np.abs(np.concatenate([spec.a_low, spec.a_high]))))
    worst = float(np.max(np.abs(g - gr) / tol[None, :, None]))
    print(f"case {plan}-odd-batch: rows at most {worst:.3e} x the row tolerance from the classic per-step kernel")
    assert worst <= 1.0
    sure = np.all(np.abs(gr) >= tol[None, :, None], axis=1)
    assert np.mean(sure) >= 0.99
    assert np.array_equal(out["viol"].cpu().numpy()[sure], ref["viol"].cpu().numpy().astype(bool)[sure])
    ef.close(), es.close()


def test_dense_rows_component_major_between_guards():
    """the eight rows written (ncon, T, B), the reference's axis order: strides of the rows r >= 2"""
    torch = _torch()
    from test_gpu_cons_rollout import _guarded, _guards_ok, _raw_policy_call

    plan = "cstr_dist_both_rows8"
    spec_h, pol, ep, cand = feature_case(plan, "rk4", "policy")
    e1, eg = _envs(case_params(plan, "rk4", spec_h), 2)
    spec, dev = e1.spec, e1.device
    T, f64, u8 = spec.N - 1, torch.float64, torch.uint8
    _forget_launches(e1)
    one = e1.rollout_policy_cons(pol, T, collect_obs=True, record_next_action=True)
    bufs = {"a": _guarded((T + 1, spec.na, B), f64, dev), "obs": _guarded((T, spec.nobs, B), f64, dev), "rew": _guarded((T, B), f64, dev),
            "g": _guarded((spec.ncon, T, B), f64, dev), "viol": _guarded((T, B), u8, dev)}
    rc = _raw_policy_call(eg, pol, T, bufs["a"][1], bufs["obs"][1], bufs["rew"][1], bufs["g"][1], (B, T * B), bufs["viol"][1], 1)
    torch.cuda.synchronize()
    assert rc == 0 and spec.ncon == 8 and _launched(e1._lib, "rollout_cons_policy_kernel") and not eg.status.any()
    for k in ("a", "obs", "rew"):
        assert torch.equal(bufs[k][1], one[k]), k
    assert torch.equal(bufs["g"][1].permute(1, 0, 2), one["g"]), "rows in the reference's axis order differ from step-major rows"
    assert torch.equal(bufs["viol"][1].view(torch.bool), one["viol"])
    assert len({float(one["g"][:, r].sum()) for r in range(8)}) == 8  # (eight different rows: a wrong stride would repeat one)
    for k, (whole, view) in bufs.items():
        assert _guards_ok(whole, view.dtype), f"guard bytes around {k} were written"
    _check_final(eg, e1)
    e1.close(), eg.close()


def test_collect_onpolicy_records_the_showcase_rows():
    """collect_onpolicy(record_cons=True) on the constraint showcase, fused against fused=False, as
    test_gpu_cons_rollout.test_collect_onpolicy_records_the_rows"""
    torch = _torch()
    from pcgym_amd import GaussianActorCritic, collect_onpolicy

    plan = "cstr_con_reward"
    spec_h = feature_case(plan, "rk4", "actor")[0]
    ef, es, e2, en = _envs(case_params(plan, "rk4", spec_h), 4)  # (collect_onpolicy resets again: the envs stay in the same RNG epoch)
    spec = ef.spec
    T = spec.N - 1
    # The fused route and the torch route round the networks differently and run FREE here, not teacher-forced: the spread of
    # two per-step runs measures that only on a loop that contracts.  The case's own actor is a switch on the temperature
    # (feedback_policy), which amplifies a last-bit difference near its threshold; this comparison takes make_ac's actor
    # with the clip box at the cold end of the action box instead, under which about 0.4 of the entries violate.
    ac = build_net(spec_h, ef.obs_soa.cpu().numpy(), "actor", "1x16", (17, "clip", -0.7, 0.2))
    ac2 = GaussianActorCritic(_perm_hidden(ac.actor, 5), ac.log_std, _perm_hidden(ac.critic, 6))
    _forget_launches(ef)
    fused = collect_onpolicy(ef, ac, record_cons=True)
    torch.cuda.synchronize()
    assert _launched(ef._lib, "rollout_cons_actor_kernel"), "collect_onpolicy(record_cons=True) did not take the fused call"
    ref = collect_onpolicy(es, ac, record_cons=True, fused=False)
    ref2 = collect_onpolicy(e2, ac2, record_cons=True, fused=False)
    torch.cuda.synchronize()
    assert fused["g"].shape == (T, spec.ncon, B) and fused["viol"].shape == (T, B) and not ef.status.any()
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
        print(f"collect_onpolicy record_cons on {plan} {k}: per-step spread {spread:.3e}, fused vs per-step {d:.3e}")
        assert spread > 0 and d <= 8 * spread + 1e-13, (k, d, spread)
    assert torch.equal(fused["viol"][~near], ref["viol"][~near])
    assert torch.equal(fused["viol"], (fused["g"] > 0).any(1))
    assert 0.05 <= float(fused["viol"].float().mean()) <= 0.95
    en.reset()
    rep = _stepped(en, ac.action(fused["act"]), T)
    torch.cuda.synchronize()
    assert torch.equal(rep["g"], fused["g"]) and torch.equal(rep["viol"].view(torch.bool), fused["viol"])
    assert torch.equal(rep["obs"], fused["obs"][1:]) and torch.equal(rep["rew"], fused["rew"])
    _check_final(ef, en)
    for e in (ef, es, e2, en):
        e.close()
    ac.close(), ac2.close()


# ---- 3. the per-env-parameter family ----------------------------------------------------------------------------------------------------
def _unc_call(env, head, net, T, nxt=False):
    if head == "policy":
        a, o, r = env.rollout_policy_unc(net, T, collect_obs=True, record_next_action=nxt)
        return {"a": a, "obs": o, "rew": r}
    return env.rollout_actor_unc(net, T, collect_obs=True, record_next_action=nxt)


@pytest.mark.parametrize("shape", ["1x16", "affine"])
@pytest.mark.parametrize("head", ["policy", "actor"])
@pytest.mark.parametrize("plan", UNC_FEATURE_PLANS)
def test_per_env_parameter_family(plan, head, shape):
    torch = _torch()
    spec_h, net, ep, cand = feature_case(plan, "rk4", head, shape)
    p = case_params(plan, "rk4", spec_h)
    ea, eb, ec = _envs(p, 3)
    spec = ea.spec
    T, tol = spec.N - 1, _tols(plan)
    kinds = FEATURE_PLANS[plan][2]
    assert spec.nunc >= 2 and not spec.ncon and spec.integrator == "rk4" and ("dist" in kinds) == (spec.nd >= 1)
    orc = _oracle(spec)
    p_unc = ea.p_unc.clone()
    assert np.allclose(p_unc.cpu().numpy(), orc.p_unc, rtol=1e-14, atol=0) and np.allclose(ea.x.cpu().numpy(), orc.x, rtol=1e-14, atol=0)
    obs0 = ea.obs_soa.cpu().numpy().copy()
    _forget_launches(ea)
    one = _unc_call(ea, head, net, T, True)
    torch.cuda.synchronize()
    assert _launched(ea._lib, f"rollout_unc_{head}_kernel") and not ea.status.any()
    keys = [k for k, v in one.items() if v is not None]
    worst = _check_networks(head, net, one, obs0, lambda s: eb.policy_noise(s).cpu().numpy(), T)
    lo = spec.nobs - spec.nunc
    assert torch.equal(one["obs"][:, lo:], torch.as_tensor(obs0[lo:], device=ea.device).expand(T, -1, -1)), "the recorded parameter slots"
    # ---- chunks (1, 2, rest): bitwise; u_prev compared as it is (a step has run: no NaN left) ----
    parts, done = [], 0
    for n in (1, 2, T - 3):
        parts.append(_unc_call(eb, head, net, n, done + n == T))
        done += n
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(torch.cat([q[k] for q in parts]), one[k]), f"chunks (1, 2, rest): {k}"
    _final_equal(eb, ea)
    if ea.u_prev is not None:
        assert torch.isfinite(ea.u_prev).all() and torch.equal(eb.u_prev, ea.u_prev)
    # ---- one call per step: bitwise, and every step against the oracle from the common start state ----
    a_np, worst_x = one["a"].cpu().numpy(), 0.0
    for s in range(T):
        x_before = ec.x.cpu().numpy().copy()
        o1 = _unc_call(ec, head, net, 1)
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(o1[k][0], one[k][s]), f"one call per step, step {s}: {k}"
        orc.x[:] = x_before
        oc, rc, _ = orc.step(a_np[s])
        ex = worst_rel(ec.x.cpu().numpy(), orc.x)
        worst_x = max(worst_x, ex)
        assert ex <= tol["x1"], f"step {s}: state {ex:.3e} from the oracle"
        assert np.allclose(o1["obs"][0].cpu().numpy(), oc, rtol=tol["o_rtol"], atol=tol["o_atol"]), f"step {s}: observation"
        assert _rew_close(o1["rew"][0].cpu().numpy(), rc), f"step {s}: reward"
    _final_equal(ec, ea)
    if ea.u_prev is not None:
        assert np.allclose(ea.u_prev.cpu().numpy(), orc.u_prev, rtol=1e-15, atol=0), "io->u_prev is not the oracle's previous action"
    for e in (ea, eb, ec):
        assert torch.equal(e.p_unc, p_unc), "the call wrote io->p_unc"
    _record(f"case {plan}-{head}-{shape}: network {cand}, output error <= {worst:.3f} x bound, state vs oracle {worst_x:.2e} (bar {tol['x1']:.0e})")
    for e in (ea, eb, ec):
        e.close()


@pytest.mark.parametrize("which", ["last_od", "first_ounc"])
def test_the_policy_reads_disturbance_and_parameter_slots(which):
    """test_gpu_unc_rollout._slot_policy's large weight on the last disturbance slot / the first parameter slot of a plan that has
    both: a swapped or shifted slot shows in the action"""
    torch = _torch()
    from test_gpu_unc_rollout import _slot_policy

    plan = "unc_cstr_dist_Ti"
    spec_h, _, ep, _ = feature_case(plan, "rk4", "policy")
    (env,) = _envs(case_params(plan, "rk4", spec_h), 1)
    spec = env.spec
    T = spec.N - 1
    assert spec.nd >= 1 and spec.nunc >= 2
    slot = spec.nx + spec.nsp_obs + spec.nd + (-1 if which == "last_od" else 0)
    obs0 = env.obs_soa.cpu().numpy().copy()
    pol, slot = _slot_policy(spec, obs0, slot, ep["obs"][:, slot])  # (the disturbance slot varies along the episode, not over the batch)
    k = tanh_k()
    _forget_launches(env)
    a, o, _ = env.rollout_policy_unc(pol, T, collect_obs=True, record_next_action=True)
    torch.cuda.synchronize()
    assert _launched(env._lib, "rollout_unc_policy_kernel") and not env.status.any()
    a_np, o_np = a.cpu().numpy(), o.cpu().numpy()
    moved, pre = 0.0, 0.0
    for s in range(T + 1):
        o_in = obs0 if s == 0 else o_np[s - 1]
        ref, bound, pm = host_reference(pol, o_in, k + 1.0)
        pre = max(pre, pm)
        diff = np.abs(a_np[s].astype(LD) - ref).astype(np.float64)
        assert np.all(diff <= bound), f"step {s}: policy output off by {np.max(diff):.3e} (bound {np.max(bound):.3e})"
        # a condition on the INPUTS: with the neighbouring slot's value in this slot the reference moves by far more than the bound
        swapped = o_in.copy()
        swapped[slot] = o_in[slot + (1 if which == "last_od" else -1)]
        gap = np.abs((host_reference(pol, swapped, k + 1.0)[0] - ref).astype(np.float64))
        moved += float(np.mean(gap > 1e6 * np.max(bound))) / (T + 1)
    assert pre <= PRE_MAX and moved > 0.25, f"the slot's neighbour in its place moves the output of {moved:.2f} of the entries only"
    assert np.any((a_np > pol.out_low) & (a_np < pol.out_high)), "every output sits on the clip box"
    env.close(), pol.close()
