"""The open-loop fused rollouts (pcg_rollout, pcg_rollout_strided) away from the one shape every other test launches them in
(t0 = 0 right after a reset, the dense layout, both sequences recorded):

  test_rollout_chunks_equal_stepping_and_the_oracle          an episode as step() / rollout() calls in turn -- T = 1, a chunk
                                                             that records nothing, the chunk that ends the episode -- on every
                                                             route of pcg_rollout_strided and every state carried between calls
  test_strided_layouts_write_their_rows_and_nothing_else     pcg_rollout_strided into caller-owned, sentinel-filled buffers:
                                                             padded, odd-strided, 8-byte-offset and reference-order layouts,
                                                             either sequence (or both) left out
  test_strided_refusals_touch_nothing                        the layouts and arguments the entry point refuses
  test_flat_rollout_chunks_and_layouts                       the barrier-free pair at the smallest batch it accepts, in chunks

The kernels index the per-step tables, the Philox counter and `done` with t0 + s: every plan here has set-point (and
disturbance) rows that change at EVERY step, every env its own start state and actions, and every case asserts the kernel
it launched from the library's launch record.  References: T pcg_step launches of a twin env (the 1e-9 bar of
test_shape_sweep; bitwise where the launch record shows the same kernel, and on the flat path) and the oracle stepped from
a common state (10 x the one-step bar of test_gpu_sweeps.py)."""
import copy
import types

import numpy as np
import pytest

from helpers import (FULL, _bars, _close, _launch_names, _make, _record, _rollout_routes, _unc_params, feat_params,
                     sweep_actions, sweep_params, worst_rel)

pytestmark = pytest.mark.gpu

REC = "rollout_layouts.txt"
N_EP = 12          # episode length of parts 1 and 2: the chunk schedule below ends exactly at t = N_EP - 1
SEED, OFFSET = 5, 1000
SENT = -7.25e300   # what a cell no layout owns holds before and after a call
# a disturbance row per model: (input, first value, increment per step, bounds) -- the bounds of the scenarios
# cstr_dist_Ti / me_dist_cons (tests/golden/scenarios.py)
DIST = {"cstr": ("Ti", 340.0, 0.75, 320.0, 360.0), "multistage_extraction": ("X0", 0.55, 0.01, 0.5, 0.8)}


def _torch():
    import torch

    return torch


def _first_full_with_disturbance():
    from pcgym_amd.models import get_model

    return next(m for m in FULL if get_model(m).disturbances)


def _with_disturbance(p, model):
    name, v0, dv, lo, hi = DIST[model]
    p.update(disturbances={name: [v0 + dv * i for i in range(N_EP)]},
             disturbance_bounds={"low": np.array([lo]), "high": np.array([hi])})
    return p


def _case(name):
    """(registry key, integrator, env_params, VecEnv arguments) of a case: the episode cut to N_EP steps, set-point rows
    that change at every step, every env its own start state"""
    kw = {}
    if name == "cstr-rk4-lean":
        key, integ = "cstr", "rk4"
        p = sweep_params(key, integ, "lean")
    elif name == "four_tank-rk4-lean":
        key, integ = "four_tank", "rk4"
        p = sweep_params(key, integ, "lean")
    elif name == "cstr-rk4-cons":
        key, integ = "cstr", "rk4"
        p = sweep_params(key, integ, "cons")
    elif name in ("cstr-rk4-a_delta", "cstr-rk4-track"):
        key, integ = "cstr", "rk4"
        p, kw, _ = feat_params(key, name.rpartition("-")[2])
    elif name == "cstr-rk4-noise":
        key, integ = "cstr", "rk4"
        p = sweep_params(key, integ, "lean", noise=True, noise_percentage=0.001)
    elif name == "cstr-dopri5-dist":
        key, integ = "cstr", "dopri5"
        p = _with_disturbance(sweep_params(key, integ, "lean"), key)
    elif name == "full-cv8-dist":
        key, integ = _first_full_with_disturbance(), "cv8"
        p = _with_disturbance(sweep_params(key, integ, "lean"), key)
    elif name == "me-dopri5-lds":
        key, integ = "multistage_extraction", "dopri5"
        p = _with_disturbance(sweep_params(key, integ, "lean"), key)
        kw = {"lds_stages": True}
    elif name == "cstr-rk4-unc":
        key, integ = "cstr", "rk4"
        p = _unc_params(key, integ)
    elif name == "cstr-tsit5g":
        key, integ = "cstr", "tsit5g"
        p = sweep_params(key, integ, "lean")
    else:
        raise KeyError(name)
    p.update(tsim=float(p["tsim"]) * N_EP / int(p["N"]), N=N_EP)
    p["SP"] = {k: [float(np.asarray(v, dtype=float)[0]) * (1 + 0.004 * (i + 3 * j)) for i in range(N_EP)]
               for j, (k, v) in enumerate(p["SP"].items())}
    # (helpers._spread_x0, beside the per-env parameters of the `unc` case)
    p["uncertainty_percentages"] = {**(p.get("uncertainty_percentages") or {}), "x0": [0.02] * 24}
    p["distribution"] = "uniform"
    return key, integ, p, kw


def _assert_tables_vary(spec, steps):
    """the set-point and disturbance rows take another value at every one of `steps`: a kernel that reads row s where
    row t0 + s is meant cannot pass"""
    for row in list(spec.sp) + list(spec.d_sched):
        vals = [float(row[t]) for t in steps]
        assert len(set(vals)) == len(vals), "a per-step table repeats a value over the steps of this test"


_REF, _DENSE = {}, {}


def _reference(name, B):
    """The stepped twin of case `name` over the whole episode (N_EP - 1 pcg_step launches), every step of it held against
    the oracle from a common state.  Computed once per (case, batch), shared by the tests, never written to."""
    if (name, B) in _REF:
        return _REF[(name, B)]
    torch = _torch()
    from oracle import oracle as O

    key, integ, p, kw = _case(name)
    env = _make(p, B, seed=SEED, env_offset=OFFSET, **kw)
    spec = env.spec
    T = spec.N - 1
    _assert_tables_vary(spec, range(spec.N))
    orc = O.OracleEnv(spec, B, seed=SEED, env_offset=OFFSET)
    env.reset(), orc.reset()
    rng = np.random.default_rng(7)
    acts_np = np.stack([sweep_actions(spec, rng, B) for _ in range(T)])
    r = types.SimpleNamespace(key=key, integ=integ, p=p, kw=kw, spec=spec, T=T, bar=10 * _bars(key, integ)[0],
                              noise=bool(p.get("noise")), acts=torch.tensor(acts_np, device=env.device),
                              x_start=env.x.clone(), x=[], obs=[], rew=[], done=[], status=[], nsteps=[], xo=[], rew_o=[],
                              done_o=[], worst_oracle=0.0)
    for i in range(T):
        og, rg, dg, _, _ = env.step(r.acts[i])
        oc, rc, dc = orc.step(acts_np[i])
        w = worst_rel(env.x.cpu().numpy(), orc.x)
        r.worst_oracle = max(r.worst_oracle, w)
        assert w <= r.bar, f"{name} step {i}: the step launches leave the oracle ({w:.2e})"
        # (rewards, done and observations at the tolerances of test_integrator_sweep; with noise the observation carries
        # the noise twin's fp32 normal variates)
        fin = np.isfinite(rc)
        assert fin.all()
        assert np.allclose(rg.cpu().numpy(), rc, rtol=1e-6, atol=1e-9 * (1 + np.max(np.abs(rc))))
        assert np.array_equal(dg.cpu().numpy().astype(bool), dc.astype(bool))
        if not r.noise:
            assert np.allclose(og.cpu().numpy().T, oc, rtol=1e-6, atol=1e-6 * max(1.0, np.max(np.abs(oc))))
        r.x.append(env.x.clone()), r.obs.append(env.obs_soa.clone()), r.rew.append(env.rew.clone())
        r.done.append(env.done.clone()), r.status.append(env.status.clone())
        r.nsteps.append(env.nsteps.clone() if env.nsteps is not None else None)
        r.xo.append(orc.x.copy()), r.rew_o.append(rc.copy()), r.done_o.append(dc.copy())
        orc.x[:] = env.x.cpu().numpy()  # one-step comparisons: unstable models amplify round-off from step to step
    # distinct envs: a lane that reads its neighbour's row, or a swapped pair of lanes, changes the result
    assert np.std(r.xo[-1], axis=1).min() > 0, "the envs of this case end in the same state"
    assert int(r.done[-1].min().item()) == 1 and int(r.done[-2].max().item()) == 0  # the episode ends with the last step
    env.close()
    _REF[(name, B)] = r
    return r


def _against(env, ref, i, tag, exact=False):
    """the per-step buffers of `env` after step i against the stepped twin (the 1e-9 bar of test_shape_sweep; bitwise when
    `exact`) and against the oracle's step from the twin's state -> (worst difference to stepping, to the oracle)"""
    torch = _torch()
    torch.cuda.synchronize()
    pairs = (("x", env.x, ref.x[i]), ("obs", env.obs_soa, ref.obs[i]), ("rew", env.rew, ref.rew[i]))
    d = max(_close(a, b) for _, a, b in pairs)
    w = worst_rel(env.x.cpu().numpy(), ref.xo[i])
    print(f"  {tag} after step {i}: {d:.2e} from stepping, {w:.2e} from the oracle")
    if exact:
        for what, a, b in pairs:
            assert torch.equal(a, b), f"{tag}: {what} after step {i} is not bitwise what stepping gives"
    assert d <= 1e-9, f"{tag}: {d:.2e} from its step launches after step {i}"
    assert torch.equal(env.done, ref.done[i]), f"{tag}: done after step {i}"
    assert torch.equal(env.status, ref.status[i]), f"{tag}: status after step {i}"
    if ref.nsteps[i] is not None:
        assert torch.equal(env.nsteps, ref.nsteps[i]), f"{tag}: step counts after step {i}"
    assert w <= ref.bar, f"{tag}: {w:.2e} from the oracle after step {i}"
    assert np.array_equal(env.done.cpu().numpy().astype(bool), ref.done_o[i].astype(bool))
    if ref.noise:  # (the flat module's reward tolerance, where the observation is not comparable)
        rc = ref.rew_o[i]
        assert np.allclose(env.rew.cpu().numpy(), rc, rtol=1e-7, atol=1e-7 * (1 + np.abs(rc).max()))
    return d, w


def _rows_against(got_o, got_r, ref, first, tag, exact=False):
    """recorded rows (T, Nobs, B) / (T, B) of the steps first, first + 1, ... against the stepped twin"""
    torch = _torch()
    d = 0.0
    for j in range(got_r.shape[0] if got_r is not None else got_o.shape[0]):
        for what, got, want in (("obs", got_o, ref.obs), ("rew", got_r, ref.rew)):
            if got is None:
                continue
            if exact:
                assert torch.equal(got[j], want[first + j]), f"{tag}: recorded {what} row of step {first + j} is not bitwise stepping's"
            d = max(d, _close(got[j], want[first + j]))
    assert d <= 1e-9, f"{tag}: recorded rows {d:.2e} from the step launches"
    return d


def _rolled(env, fn):
    """run `fn` (one rollout call) -> (its result, the rollout kernels the launch record shows for it)"""
    _launch_names(env._lib, reset=True)
    out = fn()
    _torch().cuda.synchronize()
    return out, _rollout_routes(_launch_names(env._lib))


# ---- 1. mid-episode and chunked rollouts -------------------------------------------------------------------------------------------
# (case, batch, the route every rollout call of it must take).  All eleven plans of the list are accepted at creation.
CHUNK_CASES = [("cstr-rk4-lean", 200, "lean2"), ("cstr-rk4-lean", 201, "lean1"), ("four_tank-rk4-lean", 200, "lean2"),
               ("four_tank-rk4-lean", 201, "lean1"), ("cstr-rk4-cons", 200, "general"), ("cstr-rk4-a_delta", 200, "general"),
               ("cstr-rk4-track", 200, "general"), ("cstr-rk4-noise", 200, "general"), ("cstr-dopri5-dist", 200, "general"),
               ("full-cv8-dist", 200, "general"), ("me-dopri5-lds", 200, "lds"), ("cstr-rk4-unc", 200, "unc"),
               ("cstr-tsit5g", 200, "general")]
# step() x 2, rollout(T = 1), rollout(T = 3) recording nothing, step(), rollout(T = 4) up to t = N_EP - 1
SCHEDULE = (("step", 1, None), ("step", 1, None), ("roll", 1, True), ("roll", 3, False), ("step", 1, None), ("roll", 4, True))


@pytest.mark.parametrize("name,B,route", CHUNK_CASES, ids=[f"{n}-B{b}" for n, b, _ in CHUNK_CASES])
def test_rollout_chunks_equal_stepping_and_the_oracle(name, B, route):
    torch = _torch()
    ref = _reference(name, B)
    assert sum(n for _, n, _ in SCHEDULE) == ref.T == N_EP - 1
    env, whole = (_make(ref.p, B, seed=SEED, env_offset=OFFSET, **ref.kw) for _ in range(2))
    env.reset(), whole.reset()
    assert torch.equal(env.x, ref.x_start)
    worst_d = worst_w = 0.0
    kernels, rows = set(), {}
    for kind, n, record in SCHEDULE:
        t0 = env.t
        if kind == "step":
            env.step(ref.acts[t0])
        else:
            (oq, rq), routes = _rolled(env, lambda: env.rollout(ref.acts[t0:t0 + n], collect_obs=record, collect_rew=record))
            assert set(routes) == {route}, f"rollout(T={n}) at t0={t0} took {sorted(routes)}, not {route}"
            kernels.add(routes[route])
            assert (oq is None) == (rq is None) == (not record)
            if record:
                worst_d = max(worst_d, _rows_against(oq, rq, ref, t0, f"rollout(T={n}) at t0={t0}"))
                rows[t0] = (oq, rq)
        assert env.t == t0 + n
        d, w = _against(env, ref, env.t - 1, f"{kind}(T={n}) at t0={t0}")
        worst_d, worst_w = max(worst_d, d), max(worst_w, w)
    assert env.t == N_EP - 1 and int(env.done.min().item()) == 1, "the last chunk ends the episode"
    # one call for the whole episode from t = 0: the same trajectory -- bitwise where the same kernel ran
    (ow, rw), routes = _rolled(whole, lambda: whole.rollout(ref.acts, collect_obs=True, collect_rew=True))
    assert set(routes) == {route}
    same = {routes[route]} == kernels
    worst_d = max(worst_d, _rows_against(ow, rw, ref, 0, "whole episode"))
    d, w = _against(whole, ref, ref.T - 1, "whole episode")
    worst_d, worst_w = max(worst_d, d), max(worst_w, w)
    pairs = [(whole.x, env.x), (whole.obs_soa, env.obs_soa), (whole.rew, env.rew)]
    for t0, (oq, rq) in rows.items():
        pairs += [(ow[t0:t0 + oq.shape[0]], oq), (rw[t0:t0 + rq.shape[0]], rq)]
    dc = max(_close(a, b) for a, b in pairs)
    if same:
        assert all(torch.equal(a, b) for a, b in pairs), f"the same kernel in chunks and in one call differs by {dc:.2e}"
    assert dc <= 1e-9
    assert torch.equal(whole.done, env.done) and torch.equal(whole.status, env.status)
    _record(REC, f"chunks {name} B={B} ({route}): worst {worst_d:.2e} from stepping, {worst_w:.2e} from the oracle "
                 f"(the twin itself {ref.worst_oracle:.2e}); whole episode vs chunks {dc:.2e}, same kernel: {same}")
    env.close(), whole.close()


# ---- 2. strided layouts with guard cells ----------------------------------------------------------------------------------------
T0, T_L = 2, 5  # the layouts start mid-episode, after two steps
LAYOUTS = ("dense", "ref_order", "padded", "odd", "a_off8", "r_off8", "no_obs", "no_rew", "none")
LAYOUT_PLANS = [("cstr-rk4-lean", 200), ("cstr-rk4-lean", 201), ("cstr-rk4-cons", 200), ("cstr-dopri5-dist", 200)]


def _layout(name, B, na, nobs):
    """{sequence: (offset of its first cell, step stride, component stride) in elements, or None} (+ "size": of a buffer)"""
    dense = {"a": (0, na * B, B), "o": (0, nobs * B, B), "r": (0, B, 0)}
    padded = {"a": (0, na * (B + 2) + 4, B + 2), "o": (0, nobs * (B + 6) + 2, B + 6), "r": (0, B + 8, 0)}
    if name == "ref_order":  # collect_rollouts: x[:, 1:] of (Nobs, N, B), r[:, 1:] of (1, N, B); step t0 + s is column t0 + s + 1
        return {**dense, "o": ((T0 + 1) * B, B, N_EP * B), "r": ((T0 + 1) * B, B, 0), "size": {"o": nobs * N_EP * B, "r": N_EP * B}}
    return {"dense": dense, "padded": padded, "odd": {**padded, "o": (0, nobs * (B + 6) + 2, B + 3)},
            "a_off8": {**dense, "a": (1, na * B, B)}, "r_off8": {**dense, "r": (1, B, 0)}, "no_obs": {**dense, "o": None},
            "no_rew": {**dense, "r": None}, "none": {**dense, "o": None, "r": None}}[name]


def _cells(spec3, T, ncomp, B, dev):
    """flat indices (T, ncomp, B) of the cells a sequence owns"""
    torch = _torch()
    off, ss, cs = spec3
    ar = lambda n: torch.arange(n, device=dev, dtype=torch.int64)  # noqa: E731
    return off + ar(T)[:, None, None] * ss + ar(ncomp)[None, :, None] * cs + ar(B)[None, None, :]


class _Buffers:
    """caller-owned, sentinel-filled storage of the three sequences in a layout; the action cells hold `acts` (T, na, B)"""

    def __init__(self, lay, acts, nobs):
        torch = _torch()
        T, na, B = acts.shape
        dev = acts.device
        self.idx, self.buf, self.ptr, self.stride = {}, {}, {}, {}
        for s, ncomp in (("a", na), ("o", nobs), ("r", 1)):
            if lay[s] is None:
                self.idx[s] = self.buf[s] = self.ptr[s] = None
                self.stride[s] = (0, 0)
                continue
            idx = _cells(lay[s], T, ncomp, B, dev)
            size = lay.get("size", {}).get(s, int(idx.max().item()) + 1 + 16)
            assert int(idx.max().item()) < size and idx.unique().numel() == idx.numel(), "the layout's own rows overlap"
            buf = torch.full((size,), SENT, dtype=torch.float64, device=dev)
            self.idx[s], self.buf[s], self.ptr[s], self.stride[s] = idx, buf, buf[lay[s][0]:].data_ptr(), lay[s][1:]
        self.buf["a"][self.idx["a"]] = acts
        self.a_before = self.buf["a"].clone()

    def call(self, env, t0, T, strides=None):
        """pcg_rollout_strided the way rollout.collect_rollouts calls it -> its status"""
        st = dict(self.stride, **(strides or {}))
        env._buf.d = None
        return env._lib.pcg_rollout_strided(env._plan, env._bufp, t0, T, self.ptr["a"], st["a"][0], st["a"][1], self.ptr["o"],
                                            st["o"][0], st["o"][1], self.ptr["r"], st["r"][0], env._episode_seed(), env._stream())

    def rows(self, s):
        """what the layout's own cells of sequence `s` hold: (T, Nobs, B) / (T, B)"""
        if self.buf[s] is None:
            return None
        got = self.buf[s][self.idx[s]]
        return got[:, 0] if s == "r" else got

    def assert_guards(self, tag, untouched=False):
        """every cell the layout does not own (every cell at all, if `untouched`) holds the sentinel bit for bit; the actions
        are as they were"""
        torch = _torch()
        bits = torch.tensor([SENT], dtype=torch.float64).view(torch.int64).item()
        assert torch.equal(self.buf["a"].view(torch.int64), self.a_before.view(torch.int64)), f"{tag}: the action buffer was written"
        for s in ("o", "r"):
            if self.buf[s] is None:
                continue
            guard = torch.ones(self.buf[s].numel(), dtype=torch.bool, device=self.buf[s].device)
            if not untouched:
                guard[self.idx[s].reshape(-1)] = False
            bad = int((self.buf[s].view(torch.int64)[guard] != bits).sum().item())
            assert bad == 0, f"{tag}: {bad} cells of the {s} buffer outside the layout's rows were written"


def _dense_twin(name, B):
    """pcg_rollout (the dense layout, both sequences) of the steps T0 .. T0 + T_L - 1 on a twin env: once per (plan, batch)"""
    if (name, B) in _DENSE:
        return _DENSE[(name, B)]
    ref = _reference(name, B)
    env = _make(ref.p, B, seed=SEED, env_offset=OFFSET, **ref.kw)
    env.reset()
    for i in range(T0):
        env.step(ref.acts[i])
    (oq, rq), routes = _rolled(env, lambda: env.rollout(ref.acts[T0:T0 + T_L], collect_obs=True, collect_rew=True))
    d = types.SimpleNamespace(oq=oq, rq=rq, routes=routes, x=env.x.clone(), obs=env.obs_soa.clone(), rew=env.rew.clone(),
                              done=env.done.clone(), status=env.status.clone(),
                              nsteps=env.nsteps.clone() if env.nsteps is not None else None)
    _against(env, ref, T0 + T_L - 1, f"dense twin of {name} B={B}")
    env.close()
    _DENSE[(name, B)] = d
    return d


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name,B", LAYOUT_PLANS, ids=[f"{n}-B{b}" for n, b in LAYOUT_PLANS])
def test_strided_layouts_write_their_rows_and_nothing_else(name, B, layout):
    torch = _torch()
    from pcgym_amd import _abi as abi

    ref, dense = _reference(name, B), _dense_twin(name, B)
    _assert_tables_vary(ref.spec, range(T0, T0 + T_L + 1))
    spec = ref.spec
    env = _make(ref.p, B, seed=SEED, env_offset=OFFSET, **ref.kw)
    env.reset()
    for i in range(T0):
        env.step(ref.acts[i])
    bufs = _Buffers(_layout(layout, B, spec.na, spec.nobs), ref.acts[T0:T0 + T_L], spec.nobs)
    rc, routes = _rolled(env, lambda: bufs.call(env, T0, T_L))
    assert rc == abi.PCG_OK
    env.t += T_L
    tag = f"{name} B={B} {layout}"
    # the route: two envs per lane need an even batch, even strides and 16-byte-aligned pointers (the record's names tell
    # the two lean instantiations apart: helpers._rollout_routes)
    if "lean" in name:
        want = "lean1" if (B % 2 or layout in ("odd", "a_off8", "r_off8")) else "lean2"
    else:
        want = "general"
    assert set(routes) == {want}, f"{tag}: took {sorted(routes)}, not {want}"
    same = routes == dense.routes
    bufs.assert_guards(tag)
    worst = 0.0
    pairs = [(bufs.rows("o"), dense.oq), (bufs.rows("r"), dense.rq), (env.x, dense.x), (env.obs_soa, dense.obs), (env.rew, dense.rew)]
    for got, want_t in pairs:
        if got is None:
            continue
        if same:
            assert torch.equal(got, want_t), f"{tag}: differs from the dense rollout of the same kernel by {_close(got, want_t):.2e}"
        worst = max(worst, _close(got, want_t))
    assert worst <= 1e-9, f"{tag}: {worst:.2e} from the dense rollout"
    assert torch.equal(env.done, dense.done) and torch.equal(env.status, dense.status)
    if dense.nsteps is not None:
        assert torch.equal(env.nsteps, dense.nsteps)
    # ... and the per-step buffers hold the last step, whatever was recorded: the stepped twin's and the oracle's
    d, w = _against(env, ref, T0 + T_L - 1, tag)
    d = max(d, _rows_against(bufs.rows("o"), bufs.rows("r"), ref, T0, tag)) if layout != "none" else d
    _record(REC, f"layout {tag} ({want}): {worst:.2e} from the dense rollout (same kernel: {same}), {d:.2e} from stepping, "
                 f"{w:.2e} from the oracle")
    env.close()


def test_strided_refusals_touch_nothing():
    """what pcg_rollout_strided refuses, it refuses before it launches: every buffer as it was"""
    torch = _torch()
    from pcgym_amd import _abi as abi

    name, B = "cstr-rk4-lean", 200
    ref = _reference(name, B)
    spec = ref.spec
    env = _make(ref.p, B, seed=SEED, env_offset=OFFSET, **ref.kw)
    pe = _make(ref.p, B, seed=SEED, env_offset=OFFSET, per_env_t=True, **ref.kw)
    env.reset(), pe.reset()
    for i in range(T0):
        env.step(ref.acts[i])
    na, nobs = spec.na, spec.nobs
    dn = _layout("dense", B, na, nobs)
    # (description, env, t0, T, the layout the buffers are sized for, strides that replace its own, the status)
    cases = [("a_cs < B", env, T0, T_L, "dense", {"a": (dn["a"][1], B - 1)}, abi.PCG_E_DIM),
             ("o_cs < B", env, T0, T_L, "dense", {"o": (dn["o"][1], B - 1)}, abi.PCG_E_DIM),
             ("T = 0", env, T0, 0, "dense", {}, abi.PCG_E_VALUE),
             ("t0 < 0", env, -1, T_L, "dense", {}, abi.PCG_E_VALUE),
             ("per-env t", pe, 0, T_L, "dense", {}, abi.PCG_E_UNSUPPORTED),
             # rows that overlap (every cell they name lies inside the buffers)
             ("r_ss < B", env, T0, T_L, "dense", {"r": (B - 2, 0)}, abi.PCG_E_DIM),
             ("o_ss inside a step's rows", env, T0, T_L, "dense", {"o": (nobs * B - 2, B)}, abi.PCG_E_DIM),
             ("o_ss < B in the reference's order", env, T0, T_L, "ref_order", {"o": (B - 2, N_EP * B)}, abi.PCG_E_DIM)]
    for what, e, t0, T, layout, strides, want in cases:
        bufs = _Buffers(_layout(layout, B, na, nobs), ref.acts[T0:T0 + T_L], nobs)
        before = [t.clone() for t in (e.x, e.obs_soa, e.rew, e.done, e.status)]
        rc, routes = _rolled(e, lambda: bufs.call(e, t0, T, strides))
        assert rc == want, f"{what}: status {rc}, not {want}"
        assert not routes, f"{what}: refused, yet {sorted(routes)} was launched"
        bufs.assert_guards(what, untouched=True)
        for a, b in zip(before, (e.x, e.obs_soa, e.rew, e.done, e.status)):
            assert torch.equal(a, b), f"{what}: a per-step buffer changed"
    # the layouts next to the refused ones are taken: rows that just touch
    bufs = _Buffers(dn, ref.acts[T0:T0 + T_L], nobs)
    assert bufs.call(env, T0, T_L) == abi.PCG_OK
    env.t += T_L
    _against(env, ref, T0 + T_L - 1, "after the refusals")
    env.close(), pe.close()


# ---- 3. the flat pair at its smallest batch ---------------------------------------------------------------------------------------
def test_flat_rollout_chunks_and_layouts():
    """the barrier-free pair (first pass + rollout_kernel_hot) of the cstr's default plan at B = num_cus * 256 + 2, the
    episode in four calls: T = 2 is the shortest the pair takes, T = 1 falls to the single kernel, and in the later chunks
    most handed-over envs are hot from their first step on -- bitwise T pcg_step launches, windows against the oracle"""
    torch = _torch()
    from oracle import oracle as O
    from pcgym_amd import VecEnv
    from pcgym_amd import _abi as abi
    from test_gpu_flat_rollout import _params as flat_params

    B = torch.cuda.get_device_properties(0).multi_processor_count * 256 + 2
    p = flat_params(False)
    e_flat, e_step, e_whole = (VecEnv(copy.deepcopy(p), n_envs=B, seed=7) for _ in range(3))
    spec = e_flat.spec
    assert spec.integrator == "tsit5g"
    N, na, nobs, dev = spec.N, spec.na, spec.nobs, e_flat.device
    T = N - 1
    chunks = ((0, 20, "dense"), (20, 2, "none"), (22, 1, "dense"), (23, N - 1 - 23, "ref_order"))
    assert sum(c[1] for c in chunks) == T
    acts = torch.tensor(np.random.default_rng(11).uniform(-1, 1, (T, na, B)), device=dev)
    for e in (e_flat, e_step, e_whole):
        e.reset()
    x_start = e_flat.x.clone()
    # (a) T step launches; which envs the guard did not trust, step by step
    obs_s, rew_s, hot, ends = [], [], [], {}
    for i in range(T):
        e_step.step(acts[i])
        obs_s.append(e_step.obs_soa.clone()), rew_s.append(e_step.rew.clone())
        hot.append(e_step.nsteps.sum(dim=0) > 0)
        if any(i == t0 + n - 1 for t0, n, _ in chunks):
            ends[i] = [t.clone() for t in (e_step.x, e_step.done, e_step.status, e_step.nsteps)]
    hot = torch.stack(hot)
    first = hot[:20].any(dim=0)
    share = float(first.double().mean().item())
    assert 0.05 <= share <= 0.95, f"{share:.3f} of the envs are handed over in the first chunk"
    # (calm envs rarely ignite later: on the oracle, 3 of these 65,538 envs are calm at step 0 and hot at step 1, none of
    # the first 4,096 -- hence the whole batch and not a sample)
    assert bool(hot[0].any()) and bool((first & ~hot[0]).any()), "hand-overs at step 0 and at a later step"
    assert bool((~hot[20] & ~hot[21]).any()), "an env that stays calm through the T = 2 chunk"
    # (b) the chunks
    got_o, got_r = {}, {}
    for t0, n, layout in chunks:
        tag = f"flat chunk (t0={t0}, T={n}, {layout})"
        if layout == "ref_order":
            lay = {"a": (0, na * B, B), "o": ((t0 + 1) * B, B, N * B), "r": ((t0 + 1) * B, B, 0), "size": {"o": nobs * N * B, "r": N * B}}
        else:
            lay = _layout(layout, B, na, nobs)
        bufs = _Buffers(lay, acts[t0:t0 + n], nobs)
        rc, routes = _rolled(e_flat, lambda: bufs.call(e_flat, t0, n))
        assert rc == abi.PCG_OK
        e_flat.t += n
        assert set(routes) == ({"general", "hot"} if n >= 2 else {"general"}), f"{tag}: took {sorted(routes)}"
        bufs.assert_guards(tag)
        i = t0 + n - 1
        for what, a, b in zip(("x", "done", "status", "nsteps"), (e_flat.x, e_flat.done, e_flat.status, e_flat.nsteps), ends[i]):
            assert torch.equal(a, b), f"{tag}: {what} differs from stepping"
        assert torch.equal(e_flat.obs_soa, obs_s[i]) and torch.equal(e_flat.rew, rew_s[i]), f"{tag}: the last step's outputs"
        got_o[i], got_r[i] = e_flat.obs_soa.clone(), e_flat.rew.clone()
        if layout != "none":
            ro, rr = bufs.rows("o"), bufs.rows("r")
            for j in range(n):
                assert torch.equal(rr[j], rew_s[t0 + j]), f"{tag}: reward of step {t0 + j} differs from stepping"
                assert torch.equal(ro[j], obs_s[t0 + j]), f"{tag}: observation of step {t0 + j} differs from stepping"
                got_o[t0 + j], got_r[t0 + j] = ro[j], rr[j]
    assert int(e_flat.done.min().item()) == 1 and int(e_flat.status.sum().item()) == 0
    # (c) one call for the whole episode: the same bits
    (ow, rw), routes = _rolled(e_whole, lambda: e_whole.rollout(acts, collect_obs=True, collect_rew=True))
    assert set(routes) == {"general", "hot"}
    assert torch.equal(e_whole.x, e_flat.x) and torch.equal(e_whole.obs_soa, e_flat.obs_soa) and torch.equal(e_whole.rew, e_flat.rew)
    assert all(torch.equal(ow[i], got_o[i]) and torch.equal(rw[i], got_r[i]) for i in got_r)
    # (d) windows of the batch against the oracle's per-env loop: the windows and bars of tests/test_gpu_flat_rollout.py
    W = 96
    worst = 0.0
    for lo in (0, B // 2 - 31, B - W):
        orc = O.OracleEnv(spec, W, seed=7, env_offset=lo)
        orc.reset()
        assert np.allclose(orc.x, x_start[:, lo:lo + W].cpu().numpy(), rtol=1e-14)
        orc.x[:] = x_start[:, lo:lo + W].cpu().numpy()
        for i in range(T):
            oc, rc, _ = orc.step(acts[i][:, lo:lo + W].cpu().numpy())
            if i in got_r:  # (every step but the first of the chunk that records nothing)
                assert np.allclose(got_r[i][lo:lo + W].cpu().numpy(), rc, rtol=1e-7, atol=1e-7 * (1 + np.abs(rc).max()))
                assert np.allclose(got_o[i][:, lo:lo + W].cpu().numpy(), oc, rtol=1e-8, atol=1e-9)
        assert np.std(orc.x, axis=1).min() > 0
        xs = np.maximum(np.abs(orc.x), 1e-9)
        worst = max(worst, float(np.max(np.abs(e_flat.x[:, lo:lo + W].cpu().numpy() - orc.x) / xs)))
    assert worst <= 1e-8
    _record(REC, f"flat B={B}: chunks {[c[:2] for c in chunks]} bitwise == {T} step launches == one call; {share:.3f} of the envs "
                 f"handed over in the first chunk; worst final state in the oracle windows {worst:.2e}")
    for e in (e_flat, e_step, e_whole):
        e.close()
