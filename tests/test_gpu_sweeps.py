"""Registry-wide sweeps of the kernel instantiations, inside the gated suite (round 6; rounds 3-5 ran them as builder tools:
tools/integrator_sweep.py, tools/shape_sweep.py -- which is how a silently wrong step_kernel<heat_exchanger, RODAS4|5,
lock-stepped> survived two green rounds).

  test_integrator_sweep     every model x integrator x counter mode x feature set x dispatch: env steps through the step
                            kernels against the oracle, EVERY lane, one-step comparisons from a common state
  test_ros_single_attempt   the Rosenbrock attempt on its own, through the product kernels: a configuration under which the
                            controller takes exactly ONE attempt of size dt and accepts it (huge tolerance, small dt: no
                            decisions) -- every lane at <= 1e-12 (+ 5e-9 of its own increment) against the oracle, for every
                            model x {rodas3, rodas4, rodas5} x both counter modes x {pcg_step, pcg_integrate}
  test_integrate_sweep      pcg_integrate (the boundary of reference_engine.hip_integration_engine) for every model x
                            integrator against the oracle
  test_shape_sweep          fused rollout / HIP graph / same-launch auto-reset of a plan == its own step launches, which are
                            held against the oracle in the same test
  test_uncertainty_sweep    per-env model parameters (step_kernel<..., UNC> / rollout_kernel<..., UNC>) against the oracle
  test_feature_kernels      the feature-masked pipelined kernels of the two small models, mask by mask
  test_queue_shapes         the work-queue launch shapes that only large batches take (512-thread workgroups, one workgroup
                            per CU) against oracle slices

Together with tests/test_zz_kernel_coverage.py (which fails on a shipped kernel that no passing oracle / fixture test
launched) this is the guard of integrator.py:90-107 for every model of pcgym.py:128-148.
"""
import copy
import os

import numpy as np
import pytest

import scenarios as SC
# (the configurations are shared with tests/test_gpu_tile_walks.py)
from helpers import DISPATCH, FIXED, FULL, GUARDED, MODEL_KEYS, ROS, SCEN
from helpers import _bars, _close, _unc_params  # (shared with tests/test_gpu_rollout_layouts.py)
from helpers import feat_params as _feat_params
from helpers import sweep_actions as _actions
from helpers import sweep_params as _params
from helpers import worst_rel as _worst

pytestmark = pytest.mark.gpu

ADAPT = ("dopri5", "tsit5") + ROS


def _make(p, B, **kw):
    from pcgym_amd import VecEnv

    try:
        return VecEnv(copy.deepcopy(p), n_envs=B, **kw)
    except ValueError as e:  # a combination the plan refuses by design
        pytest.skip(f"refused at plan creation: {str(e)[:100]}")


# ---- step kernels ---------------------------------------------------------------------------------------------------------
def _sweep_cases():
    out = []
    for key in MODEL_KEYS:
        model = key.partition("^")[0]
        integs = FIXED + ADAPT + (GUARDED if model == "cstr" else ())
        for integ in integs:
            for pe in (False, True):
                for feat in ("lean", "cons"):
                    ds = ["auto", "classic"]
                    if not pe and feat == "lean" and integ in FIXED and model in FULL:
                        ds.append("odd")
                    if integ in ("dopri5", "rodas4", "rodas5"):
                        ds.append("queue")
                    if integ == "dopri5" and model in FULL:
                        ds.append("lds")
                    if integ == "rk4" and model in FULL and not pe and feat == "lean":
                        ds += ["stream1", "nostatus"] + (["stream2"] if model in ("cstr", "four_tank") else [])
                    for d in ds:
                        out.append(pytest.param(key, integ, pe, feat, d, id=f"{key}-{integ}-{'per_env_t' if pe else 'lockstep'}-{feat}-{d}"))
    return out


@pytest.mark.parametrize("key,integ,pe,feat,dispatch", _sweep_cases())
def test_integrator_sweep(key, integ, pe, feat, dispatch):
    import torch
    from oracle import oracle as O
    from pcgym_amd._lib import PcgError

    B = 131 if dispatch == "odd" else 700 if dispatch in ("stream1", "stream2", "nostatus") else 260
    env = _make(_params(key, integ, feat), B, seed=3, per_env_t=pe, **DISPATCH[dispatch])
    spec = env.spec
    orc = O.OracleEnv(spec, B, seed=3, per_env_t=pe)
    env.reset(), orc.reset()
    rng = np.random.default_rng(1)
    worst, same = 0.0, 1.0
    for i in range(3):
        a = _actions(spec, rng, B)
        try:
            og, rg, dg, _, _ = env.step(torch.tensor(a, device=env.device))
        except PcgError as e:
            if i == 0 and e.status == -6 and dispatch in ("queue", "stream1", "stream2", "lds"):
                pytest.skip("this launch shape does not exist for the combination (PCG_E_UNSUPPORTED)")
            raise
        oc, rc, dc = orc.step(a)
        worst = max(worst, _worst(env.x.cpu().numpy(), orc.x))
        fin = np.isfinite(rc)
        assert fin.mean() >= 0.5, "most envs fail on both sides: the comparison says nothing"
        assert np.allclose(rg.cpu().numpy()[fin], rc[fin], rtol=1e-6, atol=1e-9 * (1 + np.max(np.abs(rc[fin]), initial=0)))
        assert np.array_equal(dg.cpu().numpy().astype(bool), dc.astype(bool))
        assert np.allclose(og.cpu().numpy().T[:, fin], oc[:, fin], rtol=1e-6, atol=1e-6 * max(1.0, np.max(np.abs(oc[:, fin]))))
        if spec.ncon:
            assert np.array_equal(env.viol.cpu().numpy().astype(bool), orc.viol.astype(bool))
        if env.nsteps is not None and orc.nsteps is not None:
            same = min(same, float(np.mean(np.all(env.nsteps.cpu().numpy() == orc.nsteps, axis=0))))
        env.x.copy_(torch.tensor(orc.x, device=env.device))  # the next step starts from a common state
    env.close()
    # measured over all 266 + 228 combinations on the round-5 build: worst 4.8e-8 (a difference-quotient Jacobian through
    # three adaptive steps), identical step sequences >= 0.992
    bar, seq = _bars(key, integ)
    assert worst <= bar, f"worst relative difference over every lane {worst:.2e}"
    assert same >= seq, f"identical step sequences on {same:.3f} of the lanes"


# ---- the Rosenbrock attempt on its own -----------------------------------------------------------------------------------
def _single_attempt_params(key, integ, dt):
    p = _params(key, integ)
    N = int(p["N"])
    p.update(tsim=dt * N, rtol=1.0, atol=1.0)
    return p


# env-step lengths (fractions of the scenario's dt) at which every lane's first attempt IS the env step: h = min(c h0, dt) =
# dt with h0 = 0.01 |x| / |f| in the tolerance-scaled norm, and at tolerance 1 any finite attempt is accepted.  Small ones,
# where W = I / (gamma h) - J is dominated by its diagonal, up to as large as the first-step rule allows (h |J| ~ 0.1 - 1 for
# the stiff models), where the factorisation, the pivoting and every stage's solve carry weight.
@pytest.mark.parametrize("entry", ["step", "integrate"])
@pytest.mark.parametrize("pe", [False, True], ids=["lockstep", "per_env_t"])
@pytest.mark.parametrize("integ", ROS)
@pytest.mark.parametrize("key", MODEL_KEYS)
def test_ros_single_attempt(key, integ, pe, entry):
    import torch
    from oracle import oracle as O

    if entry == "integrate" and pe:
        pytest.skip("pcg_integrate has no counter mode")
    B = 192
    base = SC.scenarios()[SCEN[key.partition("^")[0]]]["env_params"]
    dt0 = float(base["tsim"]) / int(base["N"])
    tested = 0
    for frac in (1e-6, 1e-4, 1e-3, 1e-2):
        dt = dt0 * frac
        p = _single_attempt_params(key, integ, dt)
        env = _make(p, B, seed=11, per_env_t=pe)
        spec = env.spec
        orc = O.OracleEnv(spec, B, seed=11, per_env_t=pe)
        env.reset(), orc.reset()
        rng = np.random.default_rng(5)
        # spread the start states (the scenarios start every env at one x0)
        x0 = orc.x.copy()
        x0 *= 1.0 + 0.2 * rng.uniform(-1, 1, x0.shape)
        a = _actions(spec, rng, B)
        if entry == "step":
            env.x.copy_(torch.tensor(x0, device=env.device))
            orc.x[:] = x0
            env.step(torch.tensor(a, device=env.device))
            orc.step(a)
            xg, xo, ng, no = env.x.cpu().numpy(), orc.x, env.nsteps.cpu().numpy(), orc.nsteps
        else:
            u = np.zeros((spec.nu, B))  # the held input [actions | model disturbance inputs at their parameter values]
            u[:spec.na] = a if not spec.normalise_a else (a + 1) * (spec.a_high - spec.a_low)[:, None] / 2 + spec.a_low[:, None]
            for j, name in enumerate(spec.model.disturbances[: spec.nu - spec.na]):
                u[spec.na + j] = float(spec.model.parameters[name])
            xo, no = O.integrate(spec, x0, u)
            xt, ut = torch.tensor(x0, device=env.device), torch.tensor(u, device=env.device)
            nt = torch.zeros((2, B), dtype=torch.int32, device=env.device)
            assert env._lib.pcg_integrate(env._plan, B, xt.data_ptr(), ut.data_ptr(), nt.data_ptr(), None) == 0
            torch.cuda.synchronize()
            xg, ng = xt.cpu().numpy(), nt.cpu().numpy()
        env.close()
        if not (np.all(no[0] == 1) and np.all(no[1] == 0)):
            continue  # at this dt some lane's first-step rule asks for less than dt: not a single-attempt configuration
        tested += 1
        assert np.array_equal(ng, no), "the kernels took another step sequence than the oracle"
        # EVERY lane, every component.  The bar: 1e-12 of the component's scale, plus 5e-9 of the lane's own increment -- what
        # a difference-quotient Jacobian may legitimately turn a last-bit difference of exp / pow / sqrt into (libm here,
        # OCML there): dJ/J ~ ulp / sqrt(eps) ~ 1e-8, and the attempt passes dJ on as (gamma h |J|) |x' - x| dJ/J.  At the
        # small step sizes the increment is ~1e-6 of the state and the bar IS 1e-12; at the large ones a wrong stage
        # coefficient, a mis-restored spill or a stale pivot changes the increment by O(1), not by 1e-8 of itself.
        scale = np.maximum(np.abs(xo), 1e-6 * np.max(np.abs(xo), axis=1, keepdims=True))
        scale = np.maximum(scale, 1e-300)
        assert np.isfinite(xo).all() and np.isfinite(xg).all()
        err = np.abs(xg - xo) / scale
        inc = np.max(np.abs(xo - x0) / scale, axis=0, keepdims=True)
        bar = 1e-12 + 5e-9 * inc
        worst = float(np.max(err / bar))
        assert worst <= 1.0, (f"dt = {frac:g} x the scenario's: one attempt differs by {err.max():.2e} on some lane "
                              f"({worst:.2f} x the bar; the lanes' increments are {inc.min():.1e} .. {inc.max():.1e})")
        # ... and the attempt moved the state: the comparison is not x == x
        assert np.max(np.abs(xo - x0)) > 0
    assert tested >= 1, "no single-attempt configuration for this model"


# ---- pcg_integrate ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds", [False, True], ids=["regs", "lds_stages"])
@pytest.mark.parametrize("integ", FIXED + ADAPT + GUARDED)
@pytest.mark.parametrize("key", MODEL_KEYS)
def test_integrate_sweep(key, integ, lds):
    import torch
    from oracle import oracle as O
    from pcgym_amd import _abi as abi

    model = key.partition("^")[0]
    if integ in GUARDED and model != "cstr":
        pytest.skip("guarded schemes exist for models with a guard hook")
    if lds and not (integ == "dopri5" and model in FULL):
        pytest.skip("stage store only exists for dopri5 on the full models")
    B = 200
    env = _make(_params(key, integ, "lean"), B, seed=13)
    spec = env.spec
    if lds:
        assert env._lib.pcg_plan_set_option(env._plan, abi.PCG_OPT_LDS_STAGES, 1) == 0
    orc = O.OracleEnv(spec, B, seed=13)
    orc.reset()
    rng = np.random.default_rng(9)
    x0 = orc.x * (1.0 + 0.1 * rng.uniform(-1, 1, orc.x.shape))
    a = _actions(spec, rng, B)
    u = np.zeros((spec.nu, B))
    u[:spec.na] = a if not spec.normalise_a else (a + 1) * (spec.a_high - spec.a_low)[:, None] / 2 + spec.a_low[:, None]
    for j, name in enumerate(spec.model.disturbances[: spec.nu - spec.na]):
        u[spec.na + j] = float(spec.model.parameters[name])
    xo, no = O.integrate(spec, x0, u)
    xt, ut = torch.tensor(x0, device=env.device), torch.tensor(u, device=env.device)
    nt = torch.zeros((2, B), dtype=torch.int32, device=env.device)
    assert env._lib.pcg_integrate(env._plan, B, xt.data_ptr(), ut.data_ptr(), nt.data_ptr(), None) == 0
    torch.cuda.synchronize()
    env.close()
    assert _worst(xt.cpu().numpy(), xo) <= 1e-6
    if integ not in FIXED:
        assert np.mean(np.all(nt.cpu().numpy() == no, axis=0)) >= 0.98


# ---- the other entry points of a plan ----------------------------------------------------------------------------------------
def _shape_cases():
    out = []
    for key in MODEL_KEYS:
        model = key.partition("^")[0]
        for integ in FIXED + ADAPT + (GUARDED if model == "cstr" else ()):
            for feat in ("lean", "cons"):
                ds = ["auto"]
                if feat == "lean":
                    ds.append("classic")
                if feat == "lean" and integ in FIXED and model in FULL:
                    ds.append("odd")
                if integ == "dopri5" and model in FULL and feat == "lean":
                    ds.append("lds")
                for d in ds:
                    out.append(pytest.param(key, integ, feat, d, id=f"{key}-{integ}-{feat}-{d}"))
    return out


@pytest.mark.parametrize("key,integ,feat,dispatch", _shape_cases())
def test_shape_sweep(key, integ, feat, dispatch):
    """rollout (T steps, state in registers) == T step launches; a HIP graph of the T steps == the launches, bitwise;
    same-launch auto-reset through an episode end == step + reset -- and the step launches against the oracle over the
    same T steps."""
    import torch
    from oracle import oracle as O
    from pcgym_amd._lib import PcgError

    B, T = (201 if dispatch == "odd" else 200), 5
    model = key.partition("^")[0]
    base = SC.scenarios()[SCEN[model]]["env_params"]
    p = _params(key, integ, feat)
    p.update(N=T + 2, tsim=float(base["tsim"]) * (T + 2) / base["N"])
    for k in ("SP", "disturbances"):
        if p.get(k):
            p[k] = {kk: list(np.asarray(v, dtype=float)[: T + 2]) for kk, v in p[k].items()}
    kw = DISPATCH[dispatch]
    e_step, e_roll, e_graph = (_make(p, B, seed=5, **kw) for _ in range(3))
    ar = _make(p, B, seed=5, auto_reset=True, **kw)
    ref = _make(p, B, seed=5, **kw)
    spec = e_step.spec
    orc = O.OracleEnv(spec, B, seed=5)
    gen = torch.Generator(device="cuda").manual_seed(7)
    acts = 2 * torch.rand((T + 4, spec.na, B), generator=gen, device="cuda", dtype=torch.float64) - 1
    if not spec.normalise_a:
        lo = torch.tensor(spec.a_low, device="cuda")[None, :, None]
        hi = torch.tensor(spec.a_high, device="cuda")[None, :, None]
        acts = (acts + 1) * (hi - lo) / 2 + lo
    for e in (e_step, e_roll, e_graph, ar, ref, orc):
        e.reset()
    obs_s, rew_s = [], []
    for i in range(T):
        o, r, d, _, _ = e_step.step(acts[i])
        obs_s.append(e_step.obs_soa.clone()), rew_s.append(r.clone())
        orc.step(acts[i].cpu().numpy())
        assert _worst(e_step.x.cpu().numpy(), orc.x) <= 10 * _bars(key, integ)[0], f"step {i}: the step launches leave the oracle"
        orc.x[:] = e_step.x.cpu().numpy()  # one-step comparisons: unstable models amplify round-off from step to step
    try:
        oq, rq = e_roll.rollout(acts[:T], collect_obs=True, collect_rew=True)
        rolled = True
    except PcgError as e:  # no fused rollout for this integrator
        assert e.status == -6, e
        rolled = False
    if rolled:
        # bitwise for most shapes; the fused rollout of some models contracts differently
        ds = [_close(e_roll.x, e_step.x)] + [_close(rq[i], rew_s[i]) for i in range(T)] + [_close(oq[i], obs_s[i]) for i in range(T)]
        assert max(ds) <= 1e-9, f"fused rollout differs from its step launches by {max(ds):.2e}"
        assert torch.equal(e_roll.status, e_step.status)
    g = e_graph.capture_steps([acts[i] for i in range(T)])
    g.replay()
    torch.cuda.synchronize()
    assert _close(e_graph.x, e_step.x) == 0.0 and _close(e_graph.rew, rew_s[-1]) == 0.0, "graph replay != launches"
    assert torch.equal(e_graph.status, e_step.status)
    orc2 = O.OracleEnv(spec, B, seed=5)
    orc2.reset()
    for i in range(T + 2):  # auto-reset through the episode end (N - 1 = T + 1 steps), then one step of the next episode
        o, r, d, _, _ = ar.step(acts[i])
        if ref.t == ref.N - 1:
            ref.reset(), orc2.reset()
        o2, r2, d2, _, _ = ref.step(acts[i])
        _, r3, _ = orc2.step(acts[i].cpu().numpy())
        assert _close(r, r2) == 0.0 and torch.equal(d, d2), f"auto-reset step {i}: reward / done differ"
        fin = np.isfinite(r3)
        assert np.allclose(r.cpu().numpy()[fin], r3[fin], rtol=1e-4, atol=1e-6 * (1 + np.max(np.abs(r3[fin]), initial=0)))
        if ref.t != ref.N - 1:  # (at the episode end `ar` already holds the NEW x0)
            assert _close(ar.x, ref.x) == 0.0, f"auto-reset step {i}: state differs"
            assert _worst(ar.x.cpu().numpy(), orc2.x) <= 10 * _bars(key, integ)[0]
            orc2.x[:] = ar.x.cpu().numpy()
    for e in (e_step, e_roll, e_graph, ar, ref):
        e.close()


# ---- per-env parameters ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pe", [False, True], ids=["lockstep", "per_env_t"])
@pytest.mark.parametrize("integ", ["rk4", "dopri5"])
@pytest.mark.parametrize("key", MODEL_KEYS)
def test_uncertainty_sweep(key, integ, pe):
    """row f-3 for every model: per-env parameters sampled at reset (pcgym.py:212-253, 301-316), the dynamics use each
    env's own values: step kernels and the fused rollout against the oracle"""
    import torch
    from oracle import oracle as O

    B, T = 160, 3
    p = _unc_params(key, integ)
    env = _make(p, B, seed=21, per_env_t=pe, env_offset=1000)
    spec = env.spec
    orc = O.OracleEnv(spec, B, seed=21, per_env_t=pe, env_offset=1000)
    env.reset(), orc.reset()
    assert np.allclose(env.p_unc.cpu().numpy(), orc.p_unc, rtol=1e-14)
    assert np.std(orc.p_unc, axis=1).min() > 0
    rng = np.random.default_rng(2)
    acts = [_actions(spec, rng, B) for _ in range(T)]
    x_start = env.x.clone()
    for a in acts:
        env.step(torch.tensor(a, device=env.device)), orc.step(a)
        assert _worst(env.x.cpu().numpy(), orc.x) <= (1e-8 if "^" not in key else 5e-6)
        assert np.allclose(env.obs_soa.cpu().numpy(), orc.obs, rtol=1e-8 if "^" not in key else 1e-5, atol=1e-9 if "^" not in key else 1e-5)
        env.x.copy_(torch.tensor(orc.x, device=env.device))
    if not pe:  # the fused rollout with per-env parameters (lock-stepped by construction)
        env2 = _make(p, B, seed=21, env_offset=1000)
        env2.reset()
        assert torch.equal(env2.x, x_start)
        orc2 = O.OracleEnv(spec, B, seed=21, env_offset=1000)
        orc2.reset()
        env2.rollout(torch.tensor(np.stack(acts), device=env2.device), collect_rew=True)
        for a in acts:
            orc2.step(a)
        assert _worst(env2.x.cpu().numpy(), orc2.x) <= (1e-7 if "^" not in key else 2e-5)
        env2.close()
    env.close()


# ---- feature-masked pipelined kernels (pcg_step_feat.hpp: RK4 plans of the two small models) -----------------------------------
@pytest.mark.parametrize("fs", ["viol_only", "viol_autoreset", "cons", "track", "cons_track", "a_delta"])
@pytest.mark.parametrize("model", ["cstr", "four_tank"])
def test_feature_kernels(model, fs):
    import torch
    from oracle import oracle as O

    B = 512
    p, kw, viol = _feat_params(model, fs)
    env = _make(p, B, seed=17, **kw)
    spec = env.spec
    if viol:
        env._buf.viol = env.viol.data_ptr()
    orc = O.OracleEnv(spec, B, seed=17)
    env.reset(), orc.reset()
    rng = np.random.default_rng(4)
    for i in range(spec.N + 1 if kw.get("auto_reset") else 4):
        a = _actions(spec, rng, B)
        if kw.get("auto_reset") and orc.t == spec.N - 1:
            orc.reset()
        og, rg, dg, _, _ = env.step(torch.tensor(a, device=env.device))
        oc, rc, dc = orc.step(a)
        assert np.allclose(rg.cpu().numpy(), rc, rtol=1e-9, atol=1e-9 * (1 + np.abs(rc).max()))
        assert np.array_equal(dg.cpu().numpy().astype(bool), dc.astype(bool))
        if not (kw.get("auto_reset") and orc.t == spec.N - 1):  # (at the episode end the env already holds the new x0)
            assert _worst(env.x.cpu().numpy(), orc.x) <= 1e-11
        if spec.ncon:
            assert np.array_equal(env.viol.cpu().numpy().astype(bool), orc.viol.astype(bool))
            assert np.allclose(env.g.cpu().numpy(), orc.g, rtol=1e-10, atol=1e-10)
    env.close()


# ---- launch shapes of the work queue that only large batches take -------------------------------------------------------------
@pytest.mark.parametrize("pe", [False, True], ids=["lockstep", "per_env_t"])
@pytest.mark.parametrize("integ,B", [("dopri5", 1 << 18), ("rodas4", 70_000), ("rodas5", 70_000), ("rodas4", 1 << 18),
                                     ("rodas5", 1 << 18)])
@pytest.mark.parametrize("key", ["multistage_extraction", "multistage_extraction^1.5"])
def test_queue_shapes(key, integ, B, pe):
    """the extraction cascade at the batch sizes that select: 512-thread workgroups (DOPRI5 from 229,376 envs), ONE
    workgroup per CU on the register-only instantiation (the Rosenbrock pairs between 65,536 and 300,000 envs) and two
    workgroups per CU beyond -- one env step of the full batch against the oracle, every env: these shapes place the envs
    into tiles and sub-tiles (queue_shape, pcg_abi_step.hip), and a window would see a few of several hundred workgroups"""
    import torch
    from oracle import oracle as O

    p = _params(key, integ, "lean")
    env = _make(p, B, seed=31, per_env_t=pe)
    spec = env.spec
    env.reset()
    gen = torch.Generator(device="cuda").manual_seed(3)
    a = 2 * torch.rand((spec.na, B), generator=gen, device="cuda", dtype=torch.float64) - 1
    x0 = env.x.clone()
    og, rg, dg, _, _ = env.step(a)
    assert int(env.status.sum().item()) == 0
    orc = O.OracleEnv(spec, B, seed=31, per_env_t=pe, n_threads=_threads())
    orc.reset()
    assert np.allclose(orc.x, x0.cpu().numpy(), rtol=1e-14)
    oc, rc, dc = orc.step(a.cpu().numpy())
    bar, seq = _bars(key, integ)
    xbar = bar if bar > 1e-6 else 1e-7
    assert _worst(env.x.cpu().numpy(), orc.x) <= xbar
    same = np.all(env.nsteps.cpu().numpy() == orc.nsteps, axis=0)
    assert np.mean(same) >= seq
    _assert_outputs_match(og, rg, dg, oc, rc, dc, xbar, same)
    env.close()


def _threads():
    """threads of the oracle: the CPUs this process may use, not the machine's"""
    return int(os.environ.get("OMP_NUM_THREADS", "1") or 1)


def _assert_outputs_match(og, rg, dg, oc, rc, dc, xbar, same):
    """observations at the bar of the state (they are an affine map of it), done exact, and the rewards of the envs that
    took the oracle's step sequence (`same`) at test_integrator_sweep's bar -- an env with another sequence is held to the
    oracle through its state and observation (the pow() form of the extraction cascade may take another sequence on half of
    the envs, _bars)"""
    og, rg = og.cpu().numpy().T, rg.cpu().numpy()
    assert np.isfinite(oc).all() and np.isfinite(rc).all()
    assert np.allclose(og, oc, rtol=xbar, atol=xbar * max(1.0, float(np.max(np.abs(oc)))))
    assert np.allclose(rg[same], rc[same], rtol=1e-6, atol=1e-9 * (1 + np.max(np.abs(rc), initial=0)))
    assert np.array_equal(dg.cpu().numpy().astype(np.uint8), dc)


@pytest.mark.parametrize("pe", [False, True], ids=["lockstep", "per_env_t"])
@pytest.mark.parametrize("integ", GUARDED)
def test_guarded_fixup_shapes(integ, pe):
    """the guarded plans of the cstr in their two-launch form (from 65,536 envs: the general kernel marks the envs it does
    not trust, the work-queue kernel of the adaptive pair finishes exactly those) on the full x0 box of SURVEY.md section
    8(d), a third of which ignites: two env steps of the full batch, every env against the oracle"""
    import torch
    from oracle import oracle as O

    B = 1 << 17
    p = _params("cstr", integ, "lean")
    p.update(x0=np.array([0.85, 330.0, 0.85]), uncertainty_percentages={"x0": [0.15 / 0.85, 20.0 / 330.0]},
             distribution="uniform")
    env = _make(p, B, seed=41, per_env_t=pe)
    spec = env.spec
    env.reset()
    orc = O.OracleEnv(spec, B, seed=41, per_env_t=pe, n_threads=_threads())
    orc.reset()
    gen = torch.Generator(device="cuda").manual_seed(5)
    for _ in range(2):
        a = 2 * torch.rand((spec.na, B), generator=gen, device="cuda", dtype=torch.float64) - 1
        x0 = env.x.clone()
        og, rg, dg, _, _ = env.step(a)
        assert int(env.status.sum().item()) == 0
        assert float((env.nsteps.sum(dim=0) > 0).double().mean().item()) > 0.05  # the fix-up launch had envs to finish
        orc.x[:] = x0.cpu().numpy()
        oc, rc, dc = orc.step(a.cpu().numpy())
        assert _worst(env.x.cpu().numpy(), orc.x) <= 1e-9
        assert np.array_equal(env.nsteps.cpu().numpy(), orc.nsteps)
        _assert_outputs_match(og, rg, dg, oc, rc, dc, 1e-9, np.ones(B, dtype=bool))
    env.close()
