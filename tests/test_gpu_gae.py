"""The GAE kernel (pcg_gae, csrc/pcg_gae.hpp) on the device: bit for bit against the torch loop it replaces (rollout.gae
fused=False, on the same device tensors) and against numpy (tests/test_gae_abi.py: gae_numpy_rows, the header's rounding
sequence), on both lane paths, under stream capture, and -- through collect_onpolicy(terminate_on_violation=True) -- against the
oracle's own episode.

Bits are compared as int64 views with torch.equal.  Where an input infinity makes a NaN (inf - inf, 0 x inf) the position has
to be NaN on both sides and is left out of the bit comparison: NaN payloads are not part of the contract.

The oracle test and the scenario it is asked on.  tests/golden/scenarios.py's cstr_cons_pen_norm feeds its rows the
re-"de-normalised" state of quirk Q3 (pcgym.py:597-608): T = 327 K arrives as 25 T + 325 = 8500, so the scenario's own second
row, x[1] - 331, is positive for every env at every step under ANY actor (the oracle alone, 64 envs, 59 steps: 100 % of the
envs violate at step 0) -- everything is cut, and no choice of actor brings the share of violating envs below 1.  The test
therefore runs twice: on the scenario's rows as they are (every step terminal: adv = rew - val against the oracle), and on the
same plan with the band written in the numbers the rows are really fed, [L, 8600]: 8600 = 25 x 331 + 325 is the scenario's
upper bound in those numbers, and L = 8395.3 is the median over the 64 envs of the lowest value the oracle's own closed-loop
episode reaches (numpy actor, the oracle's noise twin; chosen from the oracle alone, on a CPU).  There the oracle shows 32 of
64 envs violating, first at steps 2 to 7, the closest row 7e-3 from zero; the band of 5 % to 95 % is asserted on that case.
"""
import copy

import numpy as np
import pytest

import scenarios as SC
from helpers import _launched, _make, _spread_x0, _torch
from test_gae_abi import case, gae_numpy_rows
from test_gpu_actor_rollout import make_ac

pytestmark = pytest.mark.gpu

BS = [1, 2, 63, 64, 65, 1000, 4097]  # below a wave, a wave +- 1, several blocks with a partial one, odd and even
TS = [1, 2, 59]                      # a partial group alone (1 and 2 steps), and 59 = a partial group of 1 + 29 whole groups of GAE_DEPTH = 2
PARAMS = [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0)]
SENT = -12345.678


def inputs(T, B, seed=0):
    """case(): normals with signed zeros and subnormals (column 0: nothing else); a +inf and a -inf column where B allows"""
    rew, val = case(T, B, seed)
    if B >= 3:
        rew[:, B // 2] = np.inf
        val[:, B // 2 - 1] = -np.inf
    return rew, val


def terms(T, B, seed=1):
    rng = np.random.default_rng(seed)
    return {"none": None, "random": rng.random((T, B)) < 0.1, "all": np.ones((T, B), dtype=np.uint8), "no": np.zeros((T, B), dtype=bool)}


def dev(a):
    torch = _torch()
    return None if a is None else torch.as_tensor(a, device="cuda")


def same_bits(a, b, what=""):
    torch = _torch()
    a, b = torch.as_tensor(a), torch.as_tensor(b, device=torch.as_tensor(a).device)
    nan = torch.isnan(a)
    assert torch.equal(nan, torch.isnan(b)), f"{what}: NaN in other places"
    assert torch.equal(a.contiguous().view(torch.int64)[nan.logical_not()], b.contiguous().view(torch.int64)[nan.logical_not()]), what


def raw(rew, val, term, adv, ret, gamma=0.99, lam=0.95, bootstrap_last=0, **over):
    """pcg_gae on tensors (views) as they lie in memory: pointers and row strides are the tensors' own unless `over` says otherwise"""
    torch = _torch()
    from pcgym_amd import _lib

    T, B = rew.shape
    a = dict(rew_ss=rew.stride(0), val_ss=val.stride(0), term_ss=term.stride(0) if term is not None else 0, adv_ss=adv.stride(0),
             ret_ss=ret.stride(0) if ret is not None else 0)
    a.update(over)
    return _lib.load().pcg_gae(B, T, rew.data_ptr(), a["rew_ss"], val.data_ptr(), a["val_ss"], term.data_ptr() if term is not None else None,
                               a["term_ss"], gamma, lam, bootstrap_last, adv.data_ptr(), a["adv_ss"],
                               ret.data_ptr() if ret is not None else None, a["ret_ss"], torch.cuda.current_stream().cuda_stream)


# ---- 1. bit for bit against the torch loop and numpy ------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("B", BS)
def test_kernel_equals_the_torch_loop_and_numpy_bitwise(B, T):
    torch = _torch()
    from pcgym_amd import gae

    rew, val = inputs(T, B, seed=B + T)
    r, v = dev(rew), dev(val)
    for kind, term in terms(T, B).items():
        tt = dev(term)
        for gamma, lam in PARAMS:
            for bl in (False, True):
                what = f"B={B} T={T} term={kind} gamma={gamma} lam={lam} bootstrap_last={bl}"
                fused = gae(r, v, gamma, lam, bl, term=tt, fused=True)
                loop = gae(r, v, gamma, lam, bl, term=tt, fused=False)
                ref = gae_numpy_rows(rew, val, gamma, lam, bl, term)
                for k in range(2):
                    assert fused[k].shape == (T, B) and fused[k].dtype == torch.float64
                    same_bits(fused[k], loop[k], what + " vs the torch loop")
                    same_bits(fused[k].cpu(), ref[k], what + " vs numpy")
    # the default takes the kernel on these tensors, and says so
    auto = gae(r, v, term=dev(terms(T, B)["random"]))
    same_bits(auto[0], gae(r, v, term=dev(terms(T, B)["random"]), fused=True)[0])


def test_a_nan_stays_in_its_env():
    torch = _torch()
    from pcgym_amd import gae

    T, B, j = 59, 130, 77
    rew, val = case(T, B, seed=9)
    clean = gae_numpy_rows(rew, val, 0.99, 0.95, True, terms(T, B)["random"])
    rew[T // 2, j] = np.nan
    val[3, j] = np.nan
    for fused in (True, False):
        adv, ret = gae(dev(rew), dev(val), 0.99, 0.95, True, term=dev(terms(T, B)["random"]), fused=fused)
        ref = gae_numpy_rows(rew, val, 0.99, 0.95, True, terms(T, B)["random"])
        for got, want, cl in ((adv, ref[0], clean[0]), (ret, ref[1], clean[1])):
            g = got.cpu().numpy()
            assert np.array_equal(g, want, equal_nan=True)
            assert np.isnan(g).any() and not np.isnan(np.delete(g, j, axis=1)).any()
            assert np.array_equal(np.delete(g, j, axis=1).view(np.int64), np.delete(cl, j, axis=1).view(np.int64))


# ---- 2. both lane paths, padding, alignment ------------------------------------------------------------------------------------------
def _padded(a, stride, offset=0, dtype=None):
    """(view of `a`'s shape inside a sentinel-filled buffer with row stride `stride`, starting `offset` elements in; the buffer)"""
    torch = _torch()
    rows, B = a.shape
    t = torch.as_tensor(a)
    sent = SENT if t.dtype == torch.float64 else 7
    buf = torch.full((offset + rows * stride + 2,), sent, dtype=t.dtype, device="cuda")
    view = buf[offset:offset + rows * stride].view(rows, stride)[:, :B]
    view.copy_(t)
    return view, buf


def _padding_untouched(view, buf, offset, stride):
    torch = _torch()
    rows, B = view.shape
    sent = SENT if buf.dtype == torch.float64 else 7
    body = buf[offset:offset + rows * stride].view(rows, stride)
    return bool((body[:, B:] == sent).all()) and bool((buf[:offset] == sent).all()) and bool((buf[offset + rows * stride:] == sent).all())


@pytest.mark.parametrize("T", [2, 4, 5, 59])  # whole groups after the partial one: none, one, two (the loop's other exit), 29
@pytest.mark.parametrize("B", [64, 65, 1000])
def test_lane_paths_give_the_same_bits_and_leave_the_padding(B, T):
    torch = _torch()
    from pcgym_amd import gae

    rew, val = inputs(T, B, seed=3)
    term = terms(T, B)["random"].astype(np.uint8)
    # contiguous: two envs per lane when B is even (torch's allocations are 16-byte aligned), one when it is odd
    want = gae(dev(rew), dev(val), 0.99, 0.95, True, term=dev(term), fused=True)
    ref = gae_numpy_rows(rew, val, 0.99, 0.95, True, term)
    same_bits(want[0].cpu(), ref[0]), same_bits(want[1].cpu(), ref[1])
    zeros = np.zeros((T, B))
    layouts = [(B + 1, 0), (B + 3, 0), (2 * B, 0), (B, 1), (B + 2, 1)]  # (row stride, elements the view starts into its buffer)
    for stride, off in layouts:
        (r, rb), (v, vb), (tm, tb) = _padded(rew, stride, off), _padded(val, stride, off), _padded(term, stride, off)
        (a, ab), (q, qb) = _padded(zeros + SENT, stride, off), _padded(zeros + SENT, stride, off)
        if off:
            assert r.data_ptr() % 16 == 8 and tm.data_ptr() % 2 == 1  # 8-byte but not 16-byte aligned: one env per lane
        assert raw(r, v, tm, a, q, bootstrap_last=1) == 0
        torch.cuda.synchronize()
        same_bits(a, want[0], f"adv, stride {stride} offset {off}"), same_bits(q, want[1], f"ret, stride {stride} offset {off}")
        for view, buf in ((r, rb), (v, vb), (tm, tb), (a, ab), (q, qb)):
            assert _padding_untouched(view, buf, off, stride), f"stride {stride} offset {off}"
        assert torch.equal(r.contiguous().view(torch.int64), dev(rew).view(torch.int64)) and torch.equal(tm, dev(term))
        # the public call on the same views: strided inputs qualify for the kernel
        pub = gae(r, v, 0.99, 0.95, True, term=tm, fused=True)
        same_bits(pub[0], want[0]), same_bits(pub[1], want[1])
    # only the outputs misaligned, and only the flags: still one env per lane, still the same bits
    r, v, tm = dev(rew), dev(val), dev(term)
    (a, ab), (q, qb) = _padded(zeros + SENT, B, 1), _padded(zeros + SENT, B, 0)
    assert raw(r, v, tm, a, q, bootstrap_last=1) == 0
    same_bits(a, want[0]), same_bits(q, want[1])
    tm1, _ = _padded(term, B, 1)
    a2, q2 = torch.full((T, B), SENT, device="cuda", dtype=torch.float64), torch.full((T, B), SENT, device="cuda", dtype=torch.float64)
    assert raw(r, v, tm1, a2, q2, bootstrap_last=1) == 0
    same_bits(a2, want[0]), same_bits(q2, want[1])


def test_views_that_do_not_qualify():
    torch = _torch()
    from pcgym_amd import gae

    T, B = 5, 8
    rew, val = (dev(a) for a in case(T, B))
    with pytest.raises(ValueError, match="stride"):
        gae(rew.t().contiguous().t(), val, fused=True)  # env axis not unit-stride
    with pytest.raises(ValueError, match="float32"):
        gae(rew.float(), val.float(), fused=True)
    with pytest.raises(ValueError):
        gae(rew, val.cpu(), fused=True)
    # ... and take the torch loop by default, as before
    a = gae(rew.t().contiguous().t(), val)
    same_bits(a[0], gae(rew, val, fused=False)[0])
    assert gae(rew.float(), val.float())[0].dtype == torch.float32


# ---- 3. refusals on the device ------------------------------------------------------------------------------------------------------
def test_null_ret_is_accepted_and_a_short_stride_is_refused():
    torch = _torch()
    from pcgym_amd import _abi as abi
    from pcgym_amd import _lib, gae

    T, B = 7, 66
    rew, val = inputs(T, B)
    r, v = dev(rew), dev(val)
    want = gae(r, v, 0.99, 0.95, False, fused=False)
    adv = torch.full((T, B), SENT, device="cuda", dtype=torch.float64)
    assert raw(r, v, None, adv, None) == 0
    same_bits(adv, want[0])
    lib = _lib.load()
    lib.pcg_coverage_names(None, 0, 1)
    adv.fill_(SENT)
    ret = torch.full((T, B), SENT, device="cuda", dtype=torch.float64)
    tm = dev(np.zeros((T, B), dtype=np.uint8))
    for over in (dict(adv_ss=B - 1), dict(rew_ss=B - 1), dict(val_ss=B - 1), dict(ret_ss=B - 1), dict(term_ss=B - 1), dict(adv_ss=0)):
        assert raw(r, v, tm, adv, ret, **over) == abi.PCG_E_DIM, over
    assert raw(r, v, tm, adv, ret, gamma=float("nan")) == abi.PCG_E_VALUE
    torch.cuda.synchronize()
    assert bool((adv == SENT).all()) and bool((ret == SENT).all()) and not _launched(lib, "gae_kernel")


# ---- 4. stream capture ----------------------------------------------------------------------------------------------------------------
def test_the_call_is_capture_safe():
    torch = _torch()
    from pcgym_amd import gae

    T, B = 59, 1000
    rew, val = inputs(T, B, seed=1)
    r, v, tm = dev(rew), dev(val), dev(terms(T, B)["random"])
    adv, ret = torch.zeros((T, B), device="cuda", dtype=torch.float64), torch.zeros((T, B), device="cuda", dtype=torch.float64)
    assert raw(r, v, tm, adv, ret) == 0  # (the first launch loads the code object: not under capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):  # the one kernel, nothing else
            assert raw(r, v, tm, adv, ret) == 0
    torch.cuda.current_stream().wait_stream(side)
    for seed in (2, 3):
        rew2, val2 = inputs(T, B, seed=seed)
        r.copy_(dev(rew2)), v.copy_(dev(val2)), tm.copy_(dev(terms(T, B, seed)["random"]))
        adv.fill_(SENT), ret.fill_(SENT)
        graph.replay()
        torch.cuda.synchronize()
        eager = gae(r, v, 0.99, 0.95, False, term=tm, fused=True)
        loop = gae(r, v, 0.99, 0.95, False, term=tm, fused=False)
        same_bits(adv, eager[0]), same_bits(ret, eager[1]), same_bits(adv, loop[0]), same_bits(ret, loop[1])


# ---- 5. collect_onpolicy ---------------------------------------------------------------------------------------------------------------
Q3_UPPER = 8600.0  # 25 x 331 + 325: the scenario's upper temperature bound in the numbers its rows are fed (quirk Q3)
Q3_LOWER = 8395.3  # the median over 64 envs of the lowest such number along the oracle's own closed-loop episode (module docstring)


def _showcase(own_rows):
    p = copy.deepcopy(SC.scenarios()["cstr_cons_pen_norm"]["env_params"])
    p.update(integrator="rk4")
    if not own_rows:
        p.update(constraints=lambda x, u: np.array([Q3_LOWER - x[1], x[1] - Q3_UPPER]).reshape(-1,))
    return _spread_x0(p, 0.01)


@pytest.mark.parametrize("rows", ["scenario", "reachable"])
def test_terminate_on_violation_against_the_oracle_episode(rows):
    """adv / ret of the fused collector with the recursion cut at violations, against GAE formed in numpy from the ORACLE's
    rewards and violation flags (teacher-forced on the recorded actions, the whole episode, the first 64 envs) and the collected
    values.

    Tolerance.  Rewards are held to tests/test_gpu_actor_rollout.py's rule, |r - r_orc| <= 1e-6 |r_orc| + 1e-8 (1 + max |r_orc|)
    =: eps per step.  With equal flags and the same values, adv_t - adv_t^orc = sum_k (gamma lam)^k (r_{t+k} - r_{t+k}^orc) over
    the steps up to the next cut, so |adv_t - adv_t^orc| <= F max eps with F = sum_{k<T} (gamma lam)^k <= T (gamma lam <= 1); ret
    adds the same value to both.  Each recursion also rounds five operations per step, each by at most 2^-53 of a magnitude
    <= S = the largest of |rew|, |val|, |adv|, |ret|, carried forward with the same factor: 2 x 5 F 2^-53 S for the two."""
    torch = _torch()
    from oracle import oracle as O
    from pcgym_amd import collect_onpolicy

    B, n, gamma, lam = 256, 64, 0.99, 0.95
    env = _make(_showcase(rows == "scenario"), B, seed=4)
    env.reset()  # (collect_onpolicy resets again: the oracle below is reset twice as well)
    spec = env.spec
    T = spec.N - 1
    ac = make_ac(spec, env.obs_soa.cpu().numpy(), (16,), seed=23, sigma_scale=0.1)
    out = collect_onpolicy(env, ac, gamma=gamma, lam=lam, record_cons=True, terminate_on_violation=True)
    torch.cuda.synchronize()
    assert _launched(env._lib, "rollout_cons_actor_kernel") and _launched(env._lib, "gae_kernel")
    assert set(out) == {"obs", "act", "logp", "val", "rew", "adv", "ret", "g", "g_pre", "viol", "alive"}
    assert out["alive"].shape == (T, B) and out["alive"].dtype == torch.bool and out["adv"].shape == out["ret"].shape == (T, B)
    orc = O.OracleEnv(spec, n, seed=4)
    orc.reset(), orc.reset()
    act = out["act"][:, :, :n].cpu().numpy()
    r_orc, v_orc, eps = np.empty((T, n)), np.empty((T, n), dtype=bool), 0.0
    rew = out["rew"][:, :n].cpu().numpy()
    for i in range(T):
        _, rc, _ = orc.step(np.clip(act[i], ac.actor.out_low, ac.actor.out_high))
        r_orc[i], v_orc[i] = rc, orc.viol != 0
        e = 1e-6 * np.abs(rc) + 1e-8 * (1 + np.max(np.abs(rc)))
        assert np.all(np.abs(rew[i] - rc) <= e), f"step {i}: reward"
        eps = max(eps, float(np.max(e)))
    share = float(v_orc.any(0).mean())
    print(f"terminate_on_violation [{rows}]: the oracle shows {share:.3f} of {n} envs violating, {float(v_orc.mean()):.4f} of all steps")
    if rows == "scenario":
        assert v_orc.all()  # quirk Q3: the scenario's own second row is positive whatever the actor does (module docstring)
    else:
        assert 0.05 <= share <= 0.95  # the cut is exercised, and not everything is cut
    assert np.array_equal(out["viol"][:, :n].cpu().numpy(), v_orc)
    alive = np.ones((T, n), dtype=bool)
    alive[1:] = np.logical_not(np.logical_or.accumulate(v_orc, axis=0)[:-1])
    assert np.array_equal(out["alive"][:, :n].cpu().numpy(), alive)
    val = out["val"][:, :n].cpu().numpy()
    a_ref, q_ref = gae_numpy_rows(r_orc, val, gamma, lam, False, v_orc)
    F = sum((gamma * lam) ** k for k in range(T))
    assert F <= T
    adv, ret = out["adv"][:, :n].cpu().numpy(), out["ret"][:, :n].cpu().numpy()
    S = max(float(np.max(np.abs(a))) for a in (r_orc, val, a_ref, q_ref))
    tol = F * eps + 2 * 5 * F * 2.0 ** -53 * S
    d_adv, d_ret = float(np.max(np.abs(adv - a_ref))), float(np.max(np.abs(ret - q_ref)))
    print(f"terminate_on_violation [{rows}]: |adv - oracle| {d_adv:.3e}, |ret - oracle| {d_ret:.3e}, tolerance {tol:.3e} (F = {F:.2f})")
    assert d_adv <= tol and d_ret <= tol
    # the whole batch: the kernel on the collector's own arrays is the torch loop on them, bit for bit
    from pcgym_amd import gae

    loop = gae(out["rew"], out["val"], gamma, lam, False, term=out["viol"], fused=False)
    same_bits(out["adv"], loop[0]), same_bits(out["ret"], loop[1])
    cut = out["viol"]
    assert torch.equal(out["adv"][cut], (out["rew"] + gamma * 0.0 - out["val"][:T] + gamma * lam * 0.0)[cut])
    env.close(), ac.close()


def test_terminate_on_violation_on_the_per_step_route_and_its_refusal():
    torch = _torch()
    from pcgym_amd import collect_onpolicy, gae

    env = _make(_showcase(False), 66, seed=4)
    env.reset()
    ac = make_ac(env.spec, env.obs_soa.cpu().numpy(), (16,), seed=23, sigma_scale=0.1)
    with pytest.raises(ValueError, match="record_cons"):
        collect_onpolicy(env, ac, terminate_on_violation=True)
    out = collect_onpolicy(env, ac, record_cons=True, terminate_on_violation=True, fused=False)
    torch.cuda.synchronize()
    assert not _launched(env._lib, "rollout_cons_actor_kernel") and _launched(env._lib, "gae_kernel")
    viol = out["viol"]
    assert 0.0 < float(viol.float().mean()) < 1.0
    loop = gae(out["rew"], out["val"], term=viol, fused=False)
    same_bits(out["adv"], loop[0]), same_bits(out["ret"], loop[1])
    alive = torch.ones_like(viol)
    for t in range(1, viol.shape[0]):
        alive[t] = alive[t - 1] & ~viol[t - 1]
    assert torch.equal(out["alive"], alive)
    plain = gae(out["rew"], out["val"], fused=False)
    assert not torch.equal(plain[0], out["adv"])  # the cut changes something
    env.close(), ac.close()


@pytest.mark.parametrize("route", ["fused", "per_step"])
def test_collect_onpolicy_defaults_are_unchanged(route):
    torch = _torch()
    from pcgym_amd import _lib, collect_onpolicy, gae

    p = copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"])
    p.update(integrator="rk4")
    env = _make(_spread_x0(p, 0.01), 130, seed=4)
    env.reset()
    ac = make_ac(env.spec, env.obs_soa.cpu().numpy(), (16,), seed=23, sigma_scale=0.1)
    lib = _lib.load()
    lib.pcg_coverage_names(None, 0, 1)
    out = collect_onpolicy(env, ac, bootstrap_last=True, fused=None if route == "fused" else False)
    torch.cuda.synchronize()
    assert _launched(lib, "rollout_actor_kernel") == (route == "fused") and _launched(lib, "gae_kernel")
    assert set(out) == {"obs", "act", "logp", "val", "rew", "adv", "ret"}
    lib.pcg_coverage_names(None, 0, 1)
    loop = gae(out["rew"], out["val"], bootstrap_last=True, fused=False)
    torch.cuda.synchronize()
    assert not _launched(lib, "gae_kernel")
    same_bits(out["adv"], loop[0]), same_bits(out["ret"], loop[1])
    assert bool(torch.isfinite(out["adv"]).all())
    env.close(), ac.close()
