"""The persistent step kernels across tiles: every env of a multi-tile batch against the oracle.

step_kernel_pipe, step_kernel_feat and step_kernel_stream launch min(CUs x blocks per CU, tiles) workgroups, and each
workgroup walks its tiles (it, it + grid, ...): the next tile's rows are loaded while the current one is integrated and
then handed over (cur = nxt, xv[i] = xn[i]), and the walk ends on a ragged last tile (live / live_n).  That code runs only
where a workgroup gets more than one tile.  Here every shipped instantiation of the three families runs at one block per
CU (PCG_OPT_STREAM_BLOCKS_PER_CU) on B = 3 S + tail envs, S = CUs x 256 x envs per lane, so that every workgroup walks
three or four tiles:

  test_tile_walk_vs_oracle       every env, every output, at least four launches from one start state, against the oracle;
                                 the same inputs at 2 blocks per CU and at the plan's own grid are identical bit for bit;
                                 the launch record holds the expected instantiation and no classic fallback of the model
  test_nt_options_are_bitwise    PCG_OPT_NT_STORES 0..7 (non-temporal observation / reward stores, state stores, loads)
                                 against the default 1, bit for bit
  test_layout_fallbacks          odd batches and buffers off their 16-byte (done: 2-byte) alignment take the one-env-per-
                                 lane pipelined kernel instead of the two-env one, and the classic kernel instead of feat
  test_every_persistent_kernel_has_a_case   (CPU) the case table covers exactly the shipped instantiations
  test_lean_kernels_at_the_32_bit_limit     B = 2^28 - 2 (the last batch of the 32-bit lean kernels) and 2^28 (classic)
"""
import copy
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import helpers as H
import scenarios as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# Model<id> of the demangled kernel names (pcg_models.hpp); the "^1.5" keys are the pow() forms of the extraction models
MODEL_ID = {"cstr": 0, "four_tank": 1, "multistage_extraction^1.5": 2, "multistage_extraction_reactive^1.5": 3,
            "crystallization": 4, "first_order_system": 5, "multistage_extraction": 18, "multistage_extraction_reactive": 19}
INTEG_ID = {"rk4": 0, "cv8": 7}
FEAT_MASK = {"viol_only": 0, "viol_autoreset": 256, "cons": 4, "track": 16, "cons_track": 20, "a_delta": 316}
FAMILIES = ("pcg::step_kernel_pipe", "pcg::step_kernel_feat", "pcg::step_kernel_stream")
# RK4 plans of the extraction cascades that are stable over the full action box (tests/test_gpu_parity.py BATCH_CASES):
# the scenarios' own step sits at RK4's stability limit, where a few envs of a large batch leave the finite range
SUBSTEPS = {"multistage_extraction": 160, "multistage_extraction_reactive": 32}
# relative bar on x of one configuration: what tests/test_gpu_parity.py::test_batched_step_vs_oracle and
# tests/test_gpu_erk.py::test_cv8_steps_vs_oracle hold the model's fixed-step plans to (observations: 10 x, rewards: 100 x).
# The first-order system has no such test (test_integrator_sweep: 1e-6); its state crosses zero, where the floor of the
# relative measure (1e-6 of the batch's range) turns last-bit differences into up to 1.4e-11 (measured): 1e-10.
TOL = {"cstr": 1e-12, "four_tank": 1e-12, "first_order_system": 1e-10, "multistage_extraction": 1e-11,
       "multistage_extraction_reactive": 1e-11, "crystallization": 1e-10}
N_AR = 5  # episode length of the auto-reset cases: the fourth launch ends the episode, the fifth starts the next
STEPS = 5


class Case:
    """one shipped instantiation: family, model key, integrator, envs per lane, AR (pipe) / feature set (feat), route"""

    def __init__(self, fam, key, integ, epl, what, route):
        self.fam, self.key, self.integ, self.epl, self.what, self.route = fam, key, integ, epl, what, route
        self.model = key.partition("^")[0]
        mid = MODEL_ID[key]
        if fam == "pipe":
            self.kernel = f"pcg::step_kernel_pipe<pcg::Model<{mid}>, {epl}, {'true' if what else 'false'}, {INTEG_ID[integ]}>"
        elif fam == "feat":
            self.kernel = f"pcg::step_kernel_feat<pcg::Model<{mid}>, 2, {FEAT_MASK[what]}u>"
        else:
            self.kernel = f"pcg::step_kernel_stream<pcg::Model<{mid}>, {INTEG_ID[integ]}, {epl}, 1>"
        self.classic = f"pcg::step_kernel<pcg::Model<{mid}>,"
        tag = {"pipe": "ar" if what else "step", "feat": what, "stream": route}[fam]
        self.id = f"{fam}-{key}-{integ}-epl{epl}-{tag}"

    @property
    def auto_reset(self):
        return (self.fam == "pipe" and self.what) or (self.fam == "feat" and self.what == "viol_autoreset")

    def config(self):
        """(env_params, VecEnv arguments, pass the `viol` buffer, bar on x)"""
        viol = False
        if self.fam == "feat":
            p, kw, viol = H.feat_params(self.key, self.what)
        else:
            p, kw = H.sweep_params(self.key, self.integ, "lean"), dict(H.DISPATCH[self.route])
            if self.model in SUBSTEPS and self.integ == "rk4":
                p["substeps"] = SUBSTEPS[self.model]
            if self.auto_reset:
                kw["auto_reset"] = True
        if self.auto_reset:  # an episode that ends inside the run; every env its own initial state (x0 box)
            from pcgym_amd.models import get_model

            base = SC.scenarios()[H.SCEN[self.model]]["env_params"]
            p.update(N=N_AR, tsim=float(base["tsim"]) * N_AR / base["N"])
            for k in ("SP", "disturbances"):
                if p.get(k):
                    p[k] = {kk: list(np.asarray(v, dtype=float)[:N_AR]) for kk, v in p[k].items()}
            p.update(uncertainty_percentages={"x0": [0.02] * len(get_model(self.model).states)}, distribution="uniform")
        tol = 1e-11 if self.integ == "cv8" else TOL[self.model]
        return p, kw, viol, tol


def _cases():
    out = []
    for key in ("cstr", "four_tank"):
        for integ in ("rk4", "cv8"):
            for epl in (1, 2):
                if key == "four_tank" and integ == "cv8" and epl == 2:
                    continue  # (no two-env-per-lane CV8 kernel of the four_tank)
                for ar in (False, True):
                    out.append(Case("pipe", key, integ, epl, ar, "auto"))
        for fs in FEAT_MASK:
            out.append(Case("feat", key, "rk4", 2, fs, "auto"))
        out += [Case("stream", key, "rk4", 1, None, "stream1"), Case("stream", key, "rk4", 2, None, "stream2")]
    for key in ("multistage_extraction", "multistage_extraction^1.5", "multistage_extraction_reactive",
                "multistage_extraction_reactive^1.5", "crystallization", "first_order_system"):
        out.append(Case("stream", key, "rk4", 1, None, "nostatus"))
    return out


CASES = _cases()


# ---- helpers ------------------------------------------------------------------------------------------------------------------
def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU test selected but no GPU visible"
    return torch


def _cus():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def _batch(epl, tail):
    """3 S + tail envs, S = CUs x 256 x epl: every workgroup of a one-block-per-CU grid walks 3 or 4 tiles of 256 x epl.
      one   the last tile has one live lane
      full  the last tile lacks one lane
      mid   the batch ends in the middle of the fourth sweep: half of the workgroups walk one tile fewer"""
    cus, tile = _cus(), 256 * epl
    S = cus * tile
    t = {"one": epl, "full": tile - epl, "mid": (cus // 2) * tile + tile // 2 + epl}[tail]
    B = 3 * S + t
    assert (B % 2 == 1) == (epl == 1)
    return B


def _threads():
    return int(os.environ.get("OMP_NUM_THREADS", "1") or 1)


@functools.lru_cache(maxsize=1)
def _demangled():
    import kernel_inventory as KI

    return {k["name"]: k["demangled"] for k in KI.inventory()}


def _launched():
    """demangled names of every kernel this test launched so far (the record is not cleared: conftest.py reads it)"""
    from pcgym_amd import _lib

    lib = _lib.load()
    n = lib.pcg_coverage_names(None, 0, 0)
    assert n >= 1, "the launch record is off (PCG_COVERAGE was not set when the library was loaded)"
    buf = C.create_string_buffer(int(n))
    lib.pcg_coverage_names(buf, n, 0)
    names = [s for s in buf.value.decode().split("\n") if s]
    dem = _demangled()
    return {dem.get(s, s) for s in names}


def _assert_route(expect, absent):
    """a kernel whose demangled name starts with `expect` ran in this test, none that starts with one of `absent`"""
    got = _launched()
    assert any(g.startswith(f"void {expect}") for g in got), f"{expect} was not launched: {sorted(got)}"
    bad = [g for g in got if any(g.startswith(f"void {a}") for a in absent)]
    assert not bad, f"launched {bad} besides {expect}"


OUTS = ("x", "obs", "rew", "done", "viol", "g", "g_pre", "a_save", "u_prev", "status")


def _outputs(env):
    """the buffers a step launch writes, as the kernel sees them (env._buf may point at other storage than env.x ...)"""
    return {"x": env.x, "obs": env.obs_soa, "rew": env.rew, "done": env.done,
            "viol": env.viol if env._buf.viol else None, "g": env.g, "g_pre": env.g_pre, "a_save": env.a_save_t,
            "u_prev": env.u_prev, "status": env.status}


def _make(p, B, kw, viol, bpc=1, nt=None):
    from pcgym_amd import VecEnv
    from pcgym_amd import _abi as abi

    env = VecEnv(copy.deepcopy(p), n_envs=B, seed=23, **kw)
    if bpc:
        assert env._lib.pcg_plan_set_option(env._plan, abi.PCG_OPT_STREAM_BLOCKS_PER_CU, bpc) == 0
    if nt is not None:
        assert env._lib.pcg_plan_set_option(env._plan, abi.PCG_OPT_NT_STORES, nt) == 0
    if viol:
        env._buf.viol = env.viol.data_ptr()
    return env


def _start(env):
    """reset, then a start state of its own for every env (2 % around the initial state; the auto-reset plans draw theirs
    from the x0 box at the reset)"""
    torch = _torch()
    env.reset()
    if env.auto_reset:
        return
    gen = torch.Generator(device=env.device).manual_seed(99)
    env.x.mul_(1 + 0.02 * (2 * torch.rand(env.x.shape, generator=gen, device=env.device, dtype=torch.float64) - 1))
    if env.spec.model.name == "crystallization":  # (the moments' consistency, as test_batched_step_vs_oracle keeps it)
        x = env.x
        x[5] = torch.sqrt(x[2] * x[0] / x[1] ** 2 - 1)
        x[6] = x[1] / x[0]


def _actions(spec, B, n):
    """the full action box; the four_tank's lower part of it drains tanks below zero within a few launches, where both
    sides agree on NaN and nothing is compared (tests/test_gpu_erk.py::test_cv8_steps_vs_oracle keeps -0.5 .. 1 too)"""
    rng = np.random.default_rng(7)
    lo = -0.5 if spec.model.name == "four_tank" else -1.0
    return [H.sweep_actions(spec, rng, B, lo) for _ in range(n)]


def _run(env, acts):
    """the launches of `acts` from the start state: (start state, every output after every launch), device copies"""
    torch = _torch()
    _start(env)
    x_start = env.x.clone()
    out = []
    for a in acts:
        env.step(a)
        out.append({k: v.clone() for k, v in _outputs(env).items() if v is not None})
    torch.cuda.synchronize()
    return x_start, out


def _assert_identical(ref, got, tag):
    torch = _torch()
    for i, (r, g) in enumerate(zip(ref, got)):
        assert r.keys() == g.keys()
        for k in r:
            assert torch.equal(r[k], g[k]), f"{tag}: launch {i}: {k} differs"


def _oracle_check(spec, acts, x_start, outs, auto_reset, tol, tag):
    """steps the oracle through `acts` from the GPU's start state and holds every output of every launch to it"""
    from oracle import oracle as O

    B = x_start.shape[1]
    orc = O.OracleEnv(spec, B, seed=23, n_threads=_threads())
    orc.reset()
    orc.x[:] = x_start.cpu().numpy()
    ends = 0
    for i, (a, o) in enumerate(zip(acts, outs)):
        _, rc, dc = orc.step(a.cpu().numpy())
        rc, dc = rc.copy(), dc.copy()
        if auto_reset and orc.t == spec.N - 1:
            orc.reset()  # the launch that ends the episode also resets: state and observation of the new episode
            ends += 1
        g = {k: v.cpu().numpy() for k, v in o.items()}
        t = f"{tag}: launch {i}"
        for k in ("x", "obs", "rew"):
            assert np.isfinite(g[k]).all(), f"{t}: non-finite {k}"
        xs = np.maximum(np.abs(orc.x), 1e-6 * np.max(np.abs(orc.x), axis=1, keepdims=True))
        ex = np.max(np.abs(g["x"] - orc.x) / xs)
        assert ex <= tol, f"{t}: x differs by {ex:.2e} (bar {tol:.0e}) first at env {np.argmax(np.max(np.abs(g['x'] - orc.x) / xs, axis=0))}"
        eo = np.max(np.abs(g["obs"] - orc.obs) / np.maximum(np.abs(orc.obs), 1e-3))
        assert eo <= 10 * tol, f"{t}: obs differs by {eo:.2e}"
        er = np.max(np.abs(g["rew"] - rc) / np.maximum(np.abs(rc), 1.0))
        assert er <= max(100 * tol, 1e-10), f"{t}: rew differs by {er:.2e}"
        assert np.array_equal(g["done"], dc), f"{t}: done differs at {np.flatnonzero(g['done'] != dc)[:5]}"
        if "viol" in g:
            assert np.array_equal(g["viol"], orc.viol), f"{t}: viol differs"
        for k, ok in (("g", orc.g), ("g_pre", orc.g_pre)):
            if k in g:
                gs = np.maximum(np.abs(ok), 1e-3 * max(np.max(np.abs(ok)), 1e-300))
                eg = np.max(np.abs(g[k] - ok) / gs)
                assert eg <= max(100 * tol, 1e-10), f"{t}: {k} differs by {eg:.2e}"
        if "a_save" in g:
            assert np.allclose(g["a_save"], orc.a_save, rtol=1e-13, atol=0), f"{t}: a_save differs"
        if "u_prev" in g:
            assert np.allclose(g["u_prev"], orc.u_prev, rtol=1e-13, atol=0, equal_nan=True), f"{t}: u_prev differs"
        if "status" in g:
            assert np.array_equal(g["status"], orc.status), f"{t}: status differs"
    assert ends == (1 if auto_reset else 0), "the run was to end exactly one episode"


# ---- every instantiation, three tails, against the oracle ----------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("tail", ["one", "full", "mid"])
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_tile_walk_vs_oracle(case, tail):
    torch = _torch()
    B = _batch(case.epl, tail)
    p, kw, viol, tol = case.config()
    env = _make(p, B, kw, viol)
    spec = env.spec
    acts = [torch.tensor(a, device=env.device) for a in _actions(spec, B, STEPS)]
    x_start, ref = _run(env, acts)
    env.close()
    _oracle_check(spec, acts, x_start, ref, case.auto_reset, tol, case.id)
    for bpc in (2, 0):  # the grid does not change a bit of any output (0: the plan's own)
        e2 = _make(p, B, kw, viol, bpc=bpc)
        _assert_identical(ref, _run(e2, acts)[1], f"{case.id} at {bpc or 'the default'} blocks per CU")
        e2.close()
    _assert_route(case.kernel + "(", [case.classic])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_nt_options_are_bitwise(case):
    """PCG_OPT_NT_STORES: bit 0 observation / reward stores, bit 1 state stores, bit 2 loads (step_kernel_pipe) -- every
    combination computes what the default 1 does, on a multi-tile batch"""
    torch = _torch()
    B = _batch(case.epl, "mid")
    p, kw, viol, _ = case.config()
    env = _make(p, B, kw, viol)
    acts = [torch.tensor(a, device=env.device) for a in _actions(env.spec, B, STEPS)]
    _, ref = _run(env, acts)
    env.close()
    for nt in range(8):
        e2 = _make(p, B, kw, viol, nt=nt)
        _assert_identical(ref, _run(e2, acts)[1], f"{case.id} PCG_OPT_NT_STORES={nt}")
        e2.close()
    _assert_route(case.kernel + "(", [case.classic])


# ---- layout fallbacks ------------------------------------------------------------------------------------------------------
def _shifted(t, nbytes):
    """a copy of `t` whose storage starts `nbytes` past an allocation (the allocator's blocks are 256-byte aligned)"""
    torch = _torch()
    flat = torch.zeros(t.numel() + 2, dtype=t.dtype, device=t.device)
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == nbytes, v.data_ptr() % 16
    return v, flat


FALLBACKS = [("pipe", "odd"), ("pipe", "x"), ("pipe", "a"), ("pipe", "obs"), ("pipe", "rew"), ("pipe", "done"),
             ("feat", "x"), ("feat", "a"), ("feat", "obs"), ("feat", "rew"), ("feat", "done")]


@pytest.mark.gpu
@pytest.mark.parametrize("fam,what", FALLBACKS, ids=[f"{f}-{w}" for f, w in FALLBACKS])
def test_layout_fallbacks(fam, what):
    """a batch the two-env-per-lane kernels cannot take: an odd B, or one buffer off its 16-byte alignment (done: off its
    2-byte alignment).  The cstr's lean RK4 step then runs on the one-env-per-lane pipelined kernel, its constraint step
    on the classic kernel -- and computes what the oracle does."""
    torch = _torch()
    cpipe = next(c for c in CASES if c.fam == "pipe" and c.key == "cstr" and c.integ == "rk4" and c.epl == 2 and not c.what)
    cfeat = next(c for c in CASES if c.fam == "feat" and c.key == "cstr" and c.what == "cons")
    case = cpipe if fam == "pipe" else cfeat
    B = _batch(2, "mid") + (1 if what == "odd" else 0)
    p, kw, viol, tol = case.config()
    env = _make(p, B, kw, viol)
    spec = env.spec
    keep = []
    if what in ("x", "done"):
        v, flat = _shifted(getattr(env, what), 8 if what == "x" else 1)
        setattr(env, what, v)
        setattr(env._buf, what, v.data_ptr())
        keep.append(flat)
    elif what in ("obs", "rew"):
        v, flat = _shifted(env.obs_soa if what == "obs" else env.rew, 8)
        env.bind_outputs(**{"obs_soa" if what == "obs" else "rew": v})
        keep.append(flat)
    acts = []
    for a in _actions(spec, B, STEPS):
        a = torch.tensor(a, device=env.device)
        if what == "a":
            a, flat = _shifted(a, 8)
            keep.append(flat)
        acts.append(a)
    x_start, outs = _run(env, acts)
    env.close()
    _oracle_check(spec, acts, x_start, outs, False, tol, f"{fam}-{what}")
    if fam == "pipe":  # the one-env-per-lane pipelined kernel, not the two-env one, not the classic one
        _assert_route("pcg::step_kernel_pipe<pcg::Model<0>, 1, false, 0>(",
                      ["pcg::step_kernel_pipe<pcg::Model<0>, 2,", case.classic])
    else:
        _assert_route(case.classic, ["pcg::step_kernel_feat<pcg::Model<0>,"])


# ---- the case table covers the library ------------------------------------------------------------------------------------
def test_every_persistent_kernel_has_a_case():
    """CPU: every step_kernel_pipe / _feat / _stream the library ships matches exactly one case of the table above (a new
    instantiation without a case fails here), and every case names a shipped instantiation"""
    import kernel_inventory as KI

    shipped = [k["demangled"] for k in KI.inventory() if k["family"] in FAMILIES]
    assert len(shipped) >= 30, shipped
    for d in shipped:
        hit = [c.id for c in CASES if d == f"void {c.kernel}(pcg::StepArgs)"]
        assert len(hit) == 1, f"{d}: cases {hit}"
    names = {f"void {c.kernel}(pcg::StepArgs)" for c in CASES}
    assert len(names) == len(CASES), "two cases name one instantiation"
    assert names <= set(shipped), f"cases of instantiations the library does not ship: {sorted(names - set(shipped))}"


# ---- the 32-bit limit of the lean kernels ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,kernel", [((1 << 28) - 2, "pcg::step_kernel_pipe<pcg::Model<0>, 2, false, 0>("),
                                      (1 << 28, "pcg::step_kernel_feat<pcg::Model<0>, 2, 0u>(")], ids=["2^28-2", "2^28"])
def test_lean_kernels_at_the_32_bit_limit(B, kernel):
    """step_lean takes B < 2^28 (32-bit env indices and row byte offsets in step_kernel_pipe / store_lean): the largest
    such batch on the two-env-per-lane pipelined kernel, oracle windows at its start, middle and end, the whole batch
    finite.  At 2^28 no lean kernel: the step goes to the next route, the feature-masked kernel of mask 0 (64-bit
    indices), and its end window is compared."""
    torch = _torch()
    import gc

    import bench as BN
    from oracle import oracle as O
    from pcgym_amd import VecEnv

    gc.collect()
    torch.cuda.empty_cache()  # (blocks the allocator keeps from earlier tests do not count as free)
    need = 20 << 30  # an estimate: 2 state + 3 observation + action + reward rows of 2 GB, the byte rows, the temporaries
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"needs about {need >> 30} GB of free device memory, {free >> 30} GB free")
    W = 4096
    env = VecEnv(BN.workload_params(B), n_envs=B, seed=11)
    try:
        env.reset()
        gen = torch.Generator(device=env.device).manual_seed(3)
        wins = [0, B // 2 - 77, B - W] if B < (1 << 28) else [B - W]
        orcs = []
        for lo in wins:
            orc = O.OracleEnv(env.spec, W, seed=11, env_offset=lo)
            orc.reset()
            assert np.allclose(env.x[:, lo:lo + W].cpu().numpy(), orc.x, rtol=4e-16, atol=0)
            orcs.append(orc)
        for i in range(2):
            a = 2 * torch.rand((1, B), generator=gen, device=env.device, dtype=torch.float64) - 1
            env.step(a)
            for lo, orc in zip(wins, orcs):
                oc, rc, dc = orc.step(a[:, lo:lo + W].cpu().numpy())
                assert np.max(np.abs(env.x[:, lo:lo + W].cpu().numpy() - orc.x) / np.abs(orc.x)) <= 1e-12, (lo, i)
                assert np.max(np.abs(env.obs_soa[:, lo:lo + W].cpu().numpy() - oc)) <= 1e-11, (lo, i)
                assert np.allclose(env.rew[lo:lo + W].cpu().numpy(), rc, rtol=1e-10, atol=1e-12), (lo, i)
                assert np.array_equal(env.done[lo:lo + W].cpu().numpy(), dc), (lo, i)
            del a
        assert bool(torch.isfinite(env.x).all()) and bool(torch.isfinite(env.obs_soa).all())
        assert bool(torch.isfinite(env.rew).all()) and not bool(env.status.any())
    finally:
        env.close()
        del env
        gc.collect()
        torch.cuda.empty_cache()
    if "pipe" in kernel:
        _assert_route(kernel, ["pcg::step_kernel<pcg::Model<0>,", "pcg::step_kernel_pipe<pcg::Model<0>, 1,"])
    else:
        _assert_route(kernel, ["pcg::step_kernel_pipe<pcg::Model<0>,", "pcg::step_kernel_stream<pcg::Model<0>,"])
