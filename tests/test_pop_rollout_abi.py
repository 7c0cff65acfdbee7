"""CPU: the host side of a policy population (pcg_policy_pop_*, pcg_rollout_policy_pop: declaration, export, ctypes signature,
the statuses decided before the device is touched) and PolicyPopulation / fused_pop_ok without a GPU.  The device side -- the
kernel against the oracle, against rollout_policy member by member, its returns, shards, refusals -- is
tests/test_gpu_pop_rollout.py."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import scenarios as SC
from pcgym_amd import EnvSpec, MLPPolicy, PolicyPopulation
from pcgym_amd import _abi as abi
from pcgym_amd import _lib
from pcgym_amd.policy import fused_pop_ok

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pcgym_hip.h")).read()
NEW = ["pcg_policy_pop_create", "pcg_policy_pop_update", "pcg_policy_pop_destroy", "pcg_policy_pop_size", "pcg_rollout_policy_pop"]


def _members(P, dims, seed=0):
    rng = np.random.default_rng(seed)
    return [MLPPolicy([rng.standard_normal((dims[l + 1], dims[l])) for l in range(len(dims) - 1)],
                      [rng.standard_normal(dims[l + 1]) for l in range(len(dims) - 1)], activation="tanh", out_map="clip",
                      out_low=-0.7, out_high=0.9) for _ in range(P)]


def test_header_declares_and_library_exports():
    assert abi.PCG_ABI_VERSION == 16 and _lib.load().pcg_version() == 16  # additive
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"PCG_API int %s\(" % name, HDR), name
        assert abi.EXPORTS.count(name) == 1
        assert raw[name] is not None  # (AttributeError if the library does not export it)
    assert len(set(abi.EXPORTS)) == len(abi.EXPORTS)
    doc = HDR[:HDR.index("PCG_API int pcg_rollout_policy_pop(")].rsplit("/*", 1)[1]
    assert "m = (env_offset + e) / envs_per_policy" in doc and "J = J + disc * rew_s" in doc and "disc = disc * gamma" in doc


def test_ctypes_signatures_equal_the_header():
    lib = _lib.load()
    vp = C.c_void_p
    ctype = {"const double*": vp, "double*": vp, "void*": vp, "pcg_plan*": vp, "const pcg_buffers*": C.POINTER(abi.pcg_buffers),
             "const pcg_policy_pop*": vp, "pcg_policy_pop*": vp, "pcg_policy_pop**": C.POINTER(vp),
             "const pcg_policy_cfg*": C.POINTER(abi.pcg_policy_cfg), "int32_t": C.c_int32, "int64_t": C.c_int64,
             "uint64_t": C.c_uint64, "double": C.c_double}
    names = {}
    for fn in NEW:
        m = re.search(r"PCG_API (\w+) %s\((.*?)\);" % fn, HDR, re.S)
        assert m and m.group(1) == "int" and getattr(lib, fn).restype is C.c_int
        params = [p_.strip() for p_ in m.group(2).replace("\n", " ").split(",")]
        names[fn] = [re.search(r"(\w+)$", p_).group(1) for p_ in params]
        assert [ctype[re.sub(r"\s*\w+$", "", p_).strip()] for p_ in params] == list(getattr(lib, fn).argtypes), fn
    assert names["pcg_policy_pop_create"] == ["out", "cfg", "P"]
    assert names["pcg_policy_pop_update"] == ["pop", "cfg", "first", "count"]
    assert names["pcg_rollout_policy_pop"] == [
        "plan", "io", "pop", "envs_per_policy", "t0", "T", "a_seq_out", "a_step_stride", "a_comp_stride", "obs_seq",
        "obs_step_stride", "obs_comp_stride", "rew_seq", "rew_step_stride", "record_next_action", "gamma", "ret_out", "seed", "stream"]
    # pcg_rollout_policy's list with envs_per_policy after the handle and gamma / ret_out ahead of the seed
    base = re.search(r"PCG_API int pcg_rollout_policy\((.*?)\);", HDR, re.S).group(1)
    base = [re.search(r"(\w+)$", p_.strip()).group(1) for p_ in base.replace("\n", " ").split(",")]
    got = [n for n in names["pcg_rollout_policy_pop"] if n not in ("envs_per_policy", "gamma", "ret_out")]
    assert got == [("pop" if n == "policy" else n) for n in base]


def test_create_statuses_decided_on_the_host():
    """null, P = 0, width 65, unknown activation, a non-finite weight in a LATER member: refused before the device is touched
    (this process has no GPU; nothing here may reach one)"""
    lib = _lib.load()
    P = 3
    pop = PolicyPopulation.from_policies(_members(P, [4, 16, 2]))
    cfg, keep = pop.to_cfg()
    h = C.c_void_p()
    assert lib.pcg_policy_pop_create(None, C.byref(cfg), P) == abi.PCG_E_NULL
    assert lib.pcg_policy_pop_create(C.byref(h), None, P) == abi.PCG_E_NULL
    assert lib.pcg_policy_pop_create(C.byref(h), C.byref(cfg), 0) == abi.PCG_E_DIM
    assert lib.pcg_policy_pop_create(C.byref(h), C.byref(cfg), -2) == abi.PCG_E_DIM
    wide = PolicyPopulation([np.zeros((P, 65, 4)), np.zeros((P, 2, 65))], [np.zeros((P, 65)), np.zeros((P, 2))])
    wcfg, wkeep = wide.to_cfg()
    assert lib.pcg_policy_pop_create(C.byref(h), C.byref(wcfg), P) == abi.PCG_E_DIM and wide.validate() == abi.PCG_E_DIM
    bad, keep_bad = pop.to_cfg()
    bad.activation = 7
    assert lib.pcg_policy_pop_create(C.byref(h), C.byref(bad), P) == abi.PCG_E_VALUE
    missing, keep_missing = pop.to_cfg()
    missing.b[1] = None
    assert lib.pcg_policy_pop_create(C.byref(h), C.byref(missing), P) == abi.PCG_E_NULL
    pop.weights[1][P - 1, 1, 3] = np.inf  # (the cfg points at these arrays)
    assert lib.pcg_policy_pop_create(C.byref(h), C.byref(cfg), P) == abi.PCG_E_VALUE and pop.validate() == abi.PCG_E_VALUE
    rest = PolicyPopulation([w[:P - 1] for w in pop.weights], [b[:P - 1] for b in pop.biases])
    assert rest.validate() == 0  # (... which only member P - 1 carries)
    assert h.value is None  # every call above was refused
    # what is not a population
    assert lib.pcg_policy_pop_size(None) == abi.PCG_E_NULL and lib.pcg_policy_pop_update(None, C.byref(cfg), 0, 1) == abi.PCG_E_NULL
    assert lib.pcg_policy_pop_destroy(None) == abi.PCG_OK


def test_population_shape_errors():
    z = np.zeros
    with pytest.raises(ValueError):
        PolicyPopulation([], [])
    with pytest.raises(ValueError):
        PolicyPopulation([z((4, 2))], [z(4)])  # a single policy's arrays: no member axis
    with pytest.raises(ValueError):
        PolicyPopulation([z((3, 8, 4)), z((2, 1, 8))], [z((3, 8)), z((2, 1))])  # two member counts
    with pytest.raises(ValueError):
        PolicyPopulation([z((3, 8, 4)), z((3, 1, 7))], [z((3, 8)), z((3, 1))])  # layers that do not chain
    with pytest.raises(ValueError):
        PolicyPopulation([z((3, 8, 4))], [z((3, 7))])  # bias of another size
    with pytest.raises(ValueError):
        PolicyPopulation([z((3, 8, 4))], [z((3, 8)), z((3, 1))])  # one bias too many
    with pytest.raises(ValueError):
        PolicyPopulation([z((3, 1, 4))], [z((3, 1))], activation="gelu")
    with pytest.raises(ValueError):
        PolicyPopulation([z((3, 1, 4))], [z((3, 1))], out_map="softmax")
    a, b = _members(2, [4, 8, 1]), _members(1, [4, 9, 1])
    with pytest.raises(ValueError):
        PolicyPopulation.from_policies(a + b)  # two shapes
    with pytest.raises(ValueError):
        PolicyPopulation.from_policies([])
    other = MLPPolicy(a[0].weights, a[0].biases, activation="relu", out_map="clip", out_low=-0.7, out_high=0.9)
    with pytest.raises(ValueError):
        PolicyPopulation.from_policies([a[0], other])  # two activations
    with pytest.raises(ValueError):
        PolicyPopulation.from_policies([a[0], MLPPolicy(a[0].weights, a[0].biases, dtype="float32")])
    pop = PolicyPopulation.from_policies(a)
    with pytest.raises(ValueError):
        pop.member(2)
    with pytest.raises(ValueError):
        pop.update_([z((1, 8, 4)), z((1, 1, 8))], [z((1, 8)), z((1, 1))], first=2)  # past the last member
    with pytest.raises(ValueError):
        pop.update_([z((1, 9, 4)), z((1, 1, 9))], [z((1, 9)), z((1, 1))])  # another shape
    with pytest.raises(ValueError):
        pop(torch.zeros((200, 4), dtype=torch.float64), 64)  # 200 envs in slices of 64 need four members
    with pytest.raises(ValueError):
        pop(torch.zeros((64, 4), dtype=torch.float64), 64, env_offset=128)


def test_member_round_trips_from_policies_and_update_rewrites_members():
    mem = _members(5, [6, 16, 16, 2], seed=3)
    pop = PolicyPopulation.from_policies(mem)
    assert (pop.P, pop.n_in, pop.n_out, pop.n_hidden) == (5, 6, 2, 2) and pop.validate() == 0
    assert [w.shape for w in pop.weights] == [(5, 16, 6), (5, 16, 16), (5, 2, 16)]
    for i, p in enumerate(mem):
        q = pop.member(i)
        assert all(np.array_equal(a, b) for a, b in zip(q.weights, p.weights))
        assert all(np.array_equal(a, b) for a, b in zip(q.biases, p.biases))
        assert (q.activation, q.out_map, q.out_low, q.out_high, q.dtype) == (p.activation, p.out_map, p.out_low, p.out_high, "float64")
    new = _members(2, [6, 16, 16, 2], seed=4)
    sub = PolicyPopulation.from_policies(new)
    pop.update_(sub.weights, sub.biases, first=2)
    for i in range(5):
        want = new[i - 2] if i in (2, 3) else mem[i]
        assert all(np.array_equal(a, b) for a, b in zip(pop.member(i).weights + pop.member(i).biases, want.weights + want.biases)), i
    # a refused update leaves the population as it was
    sub.weights[0][1, 0, 0] = np.nan
    with pytest.raises(Exception):
        pop.update_(sub.weights, sub.biases, first=0)
    assert np.array_equal(pop.member(0).weights[0], mem[0].weights[0]) and np.array_equal(pop.member(1).weights[0], mem[1].weights[0])


@pytest.mark.parametrize("dims,act,out_map", [([5, 2], "tanh", "clip"), ([5, 16, 2], "tanh", "tanh"), ([5, 64, 64, 2], "relu", "none")])
def test_the_callable_is_its_members_slice_by_slice(dims, act, out_map):
    rng = np.random.default_rng(11)
    mem = [MLPPolicy(p.weights, p.biases, activation=act, out_map=out_map, out_low=-0.7, out_high=0.9) for p in _members(4, dims, seed=5)]
    pop = PolicyPopulation.from_policies(mem)
    obs = torch.as_tensor(rng.standard_normal((200, dims[0])))
    for G, off in ((64, 0), (128, 0), (96, 0), (64, 64), (64, 32)):
        B = min(200, 4 * G - off)
        got = pop(obs[:B], G, env_offset=off)
        assert got.shape == (B, dims[-1]) and got.dtype == torch.float64
        groups = set()
        for m in range(4):
            lo, hi = max(0, m * G - off), min(B, (m + 1) * G - off)
            if hi > lo:
                groups.add(m)
                assert torch.equal(got[lo:hi], mem[m](obs[lo:hi])), (G, off, m)
        assert len(groups) >= 2
    assert not torch.equal(pop(obs[:64], 64), pop(obs[:64], 64, env_offset=64))  # the members really differ


def test_fused_pop_ok_says_which_calls_the_kernel_takes():
    def spec(scen, **over):
        p = copy.deepcopy(SC.scenarios()[scen]["env_params"])
        p.update(over)
        return EnvSpec(p)

    ok = spec("cstr_canonical", integrator="rk4")
    pop = PolicyPopulation.from_policies(_members(4, [ok.nobs, 16, ok.na]))
    assert fused_pop_ok(ok, pop, 64) and fused_pop_ok(ok, pop, 1024) and fused_pop_ok(spec("cstr_canonical", integrator="cv8"), pop, 64)
    assert not fused_pop_ok(ok, pop, 96) and not fused_pop_ok(ok, pop, 32) and not fused_pop_ok(ok, pop, 0)
    cons = spec("cstr_cons_pen_norm", integrator="rk4")
    assert cons.ncon and (cons.nobs, cons.na) == (ok.nobs, ok.na) and not fused_pop_ok(cons, pop, 64)
    assert not fused_pop_ok(spec("cstr_canonical", integrator="dopri5"), pop, 64)
    unc = spec("cstr_canonical", integrator="rk4", uncertainty_percentages={"q": 0.03}, distribution="uniform",
               uncertainty_bounds={"low": np.array([90.0]), "high": np.array([110.0])})
    assert unc.nunc and not fused_pop_ok(unc, PolicyPopulation.from_policies(_members(2, [unc.nobs, 16, unc.na])), 64)
    from test_policy_jit_plans import _chemostat

    cs = EnvSpec(_chemostat(integrator="rk4"))  # a user model: its plan runs from a run-time compiled module
    assert cs.user_rhs_src is not None
    assert not fused_pop_ok(cs, PolicyPopulation.from_policies(_members(2, [cs.nobs, 16, cs.na])), 64)
    # members of another size, a single policy
    assert not fused_pop_ok(ok, PolicyPopulation.from_policies(_members(2, [ok.nobs + 1, 16, ok.na])), 64)
    assert not fused_pop_ok(ok, pop.member(0), 64)
