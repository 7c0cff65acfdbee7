"""CPU: the host side of a FLOAT32 policy population (pcg_policy_pop_create_f32, pcg_policy_pop_dtype: declaration, export,
ctypes binding, the statuses decided before the device is touched) and PolicyPopulation(dtype="float32") / fused_pop_ok without a
GPU: storage, the float32 callable against each member's own float32 MLPPolicy bit for bit, the constructors, update_.  The device
side -- the kernels against the oracle, against rollout_policy member by member, the weights written on the device -- is
tests/test_gpu_pop_f32.py."""
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
NEW = ["pcg_policy_pop_create_f32", "pcg_policy_pop_dtype"]


def _members(P, dims, seed=0, dtype="float32", out_map="clip", activation="tanh"):
    rng = np.random.default_rng(seed)
    return [MLPPolicy([rng.standard_normal((dims[l + 1], dims[l])) for l in range(len(dims) - 1)],
                      [rng.standard_normal(dims[l + 1]) for l in range(len(dims) - 1)], activation=activation, out_map=out_map,
                      out_low=-0.7, out_high=0.9, dtype=dtype) for _ in range(P)]


def test_header_declares_library_exports_and_abi_binds():
    assert abi.PCG_ABI_VERSION == 16 and _lib.load().pcg_version() == 16  # additive
    raw = C.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    vp = C.c_void_p
    for name in NEW:
        assert re.search(r"PCG_API int %s\(" % name, HDR), name
        assert abi.EXPORTS.count(name) == 1
        assert raw[name] is not None  # (AttributeError if the library does not export it)
        assert getattr(lib, name).restype is C.c_int
    assert len(set(abi.EXPORTS)) == len(abi.EXPORTS)
    assert list(lib.pcg_policy_pop_create_f32.argtypes) == list(lib.pcg_policy_pop_create.argtypes) == [C.POINTER(vp), C.POINTER(abi.pcg_policy_cfg), C.c_int32]
    assert list(lib.pcg_policy_pop_dtype.argtypes) == [vp]
    # the header says what an overflowing sample does, next to the paragraph on non-finite members
    doc = HDR[HDR.index("The weights of a population written and read ON the device"):HDR.index("#define PCG_RNG_SEARCH")]
    assert "+-inf" in doc and "round32(mean + std z) - mean" in doc


def test_create_f32_statuses_decided_on_the_host():
    """null, P = 0, a value that overflows float32 in a LATER member, a clip bound that overflows: refused before the device is
    touched (this process has no GPU; nothing here may reach one)"""
    lib = _lib.load()
    P = 3
    pop = PolicyPopulation.from_policies(_members(P, [4, 16, 2]))
    cfg, keep = pop.to_cfg()
    h = C.c_void_p()
    assert lib.pcg_policy_pop_create_f32(None, C.byref(cfg), P) == abi.PCG_E_NULL
    assert lib.pcg_policy_pop_create_f32(C.byref(h), None, P) == abi.PCG_E_NULL
    assert lib.pcg_policy_pop_create_f32(C.byref(h), C.byref(cfg), 0) == abi.PCG_E_DIM
    assert lib.pcg_policy_pop_create_f32(C.byref(h), C.byref(cfg), -2) == abi.PCG_E_DIM
    bad, keep_bad = pop.to_cfg()
    bad.activation = 7
    assert lib.pcg_policy_pop_create_f32(C.byref(h), C.byref(bad), P) == abi.PCG_E_VALUE
    # 1e39 is a finite double (pcg_policy_validate passes it) that is not finite after rounding: the cfg carries doubles
    big, keep_big = pop.to_cfg()
    keep_big[0][1][P - 1, 1, 3] = 1e39
    assert lib.pcg_policy_validate(C.byref(big)) == abi.PCG_OK
    assert lib.pcg_policy_pop_create_f32(C.byref(h), C.byref(big), P) == abi.PCG_E_VALUE
    assert h.value is None
    rest = PolicyPopulation([w[:P - 1] for w in keep_big[0]], [b[:P - 1] for b in keep_big[1]], dtype="float32")
    assert rest.validate() == 0  # (... which only member P - 1 carries)
    bias, keep_bias = pop.to_cfg()
    keep_bias[1][0][0, 2] = -1e39
    assert lib.pcg_policy_pop_create_f32(C.byref(h), C.byref(bias), P) == abi.PCG_E_VALUE
    box, keep_box = pop.to_cfg()
    box.out_high = 1e39
    assert lib.pcg_policy_pop_create_f32(C.byref(h), C.byref(box), P) == abi.PCG_E_VALUE
    # what is not a population
    assert lib.pcg_policy_pop_dtype(None) == abi.PCG_E_NULL
    junk = (C.c_uint32 * 64)()
    assert lib.pcg_policy_pop_dtype(C.cast(junk, C.c_void_p)) == abi.PCG_E_PLAN


def test_storage_is_float32_rounded_to_nearest():
    rng = np.random.default_rng(3)
    Ws, bs = [rng.standard_normal((3, 5, 4)), rng.standard_normal((3, 2, 5))], [rng.standard_normal((3, 5)), rng.standard_normal((3, 2))]
    pop = PolicyPopulation(Ws, bs, out_low=-0.1, out_high=0.3, dtype="float32")
    assert pop.dtype == "float32" and PolicyPopulation(Ws, bs).dtype == "float64"
    for got, want in zip(pop.weights + pop.biases, Ws + bs):
        assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, want.astype(np.float32))
    assert (pop.out_low, pop.out_high) == (float(np.float32(-0.1)), float(np.float32(0.3))) and pop.out_low != -0.1
    cfg, keep = pop.to_cfg()  # float64 copies, exact widenings
    assert (cfg.out_low, cfg.out_high) == (pop.out_low, pop.out_high)
    for l in range(2):
        w = np.ctypeslib.as_array(cfg.W[l], shape=(3 * Ws[l].shape[1] * Ws[l].shape[2],))
        assert np.array_equal(w, pop.weights[l].astype(np.float64).ravel())
    assert pop.validate() == 0 and pop.n_params == 5 * 5 + 2 * 6
    with pytest.raises(ValueError, match="overflows float32"):
        PolicyPopulation([np.full((2, 1, 3), 1e39)], [np.zeros((2, 1))], dtype="float32")
    with pytest.raises(ValueError, match="overflows float32"):
        PolicyPopulation([np.zeros((2, 1, 3))], [np.zeros((2, 1))], out_high=1e39, dtype="float32")
    with pytest.raises(ValueError):
        PolicyPopulation([np.zeros((2, 1, 3))], [np.zeros((2, 1))], dtype="float16")


@pytest.mark.parametrize("out_map", ["clip", "none", "tanh"])
@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("dims", [[4, 2], [4, 16, 2], [4, 7, 3, 1]], ids=lambda d: "x".join(map(str, d)))
def test_callable_on_cpu_tensors_gives_each_members_float32_bits(dims, activation, out_map):
    P, G = 4, 8
    mem = _members(P, dims, seed=1, out_map=out_map, activation=activation)
    pop = PolicyPopulation.from_policies(mem)
    rng = np.random.default_rng(2)
    # (B a multiple of G from offset 0; B no multiple of G; a non-zero env_offset, inside a slice and on a boundary)
    for B, off in ((P * G, 0), (P * G - 3, 0), (2 * G + 5, G), (G + 2, 2 * G + 3)):
        obs = torch.as_tensor(rng.standard_normal((B, dims[0])))
        got = pop(obs, G, off)
        assert got.dtype == torch.float64 and got.shape == (B, dims[-1])
        seen = set()
        for e in range(B):
            m = (off + e) // G
            seen.add(m)
        for m in seen:
            rows = [e for e in range(B) if (off + e) // G == m]
            sl = slice(rows[0], rows[-1] + 1)
            want = mem[m](obs[sl])
            assert torch.equal(got[sl].view(torch.int64), want.view(torch.int64)), (B, off, m)
            # every output is a float32 value unless the clip edge (a rounded bound: a float32 value too) replaced it
            assert torch.equal(got[sl].to(torch.float32).to(torch.float64), got[sl])
        assert len(seen) > 1
    # not the float64 evaluation of the same rounded weights
    wide = PolicyPopulation([w.astype(np.float64) for w in pop.weights], [b.astype(np.float64) for b in pop.biases],
                            activation=activation, out_map=out_map, out_low=pop.out_low, out_high=pop.out_high)
    obs = torch.as_tensor(rng.standard_normal((P * G, dims[0])))
    assert not torch.equal(wide(obs, G), pop(obs, G))


def test_from_policies_round_trips_through_member():
    mem = _members(3, [4, 16, 2], seed=4)
    pop = PolicyPopulation.from_policies(mem)
    assert pop.dtype == "float32" and pop.P == 3 and all(w.dtype == np.float32 for w in pop.weights + pop.biases)
    for i, q in enumerate(mem):
        back = pop.member(i)
        assert back.dtype == "float32" and (back.activation, back.out_map, back.out_low, back.out_high) == (q.activation, q.out_map, q.out_low, q.out_high)
        for got, want in zip(back.weights + back.biases, q.weights + q.biases):
            assert got.dtype == np.float32 and np.array_equal(got, want)
    assert PolicyPopulation.from_policies(_members(2, [4, 16, 2], dtype="float64")).dtype == "float64"
    m64 = _members(2, [4, 16, 2], seed=4, dtype="float64")
    with pytest.raises(ValueError):
        PolicyPopulation.from_policies([mem[0], m64[1]])  # a mix, float32 first
    with pytest.raises(ValueError):
        PolicyPopulation.from_policies([m64[0], mem[1]])  # ... float64 first


def test_update_rounds_first_and_an_overflow_changes_nothing():
    mem = _members(3, [4, 16, 2], seed=5)
    pop = PolicyPopulation.from_policies(mem)
    before = [a.copy() for a in pop.weights + pop.biases]
    rng = np.random.default_rng(6)
    Ws, bs = [rng.standard_normal((1, 16, 4)), rng.standard_normal((1, 2, 16))], [rng.standard_normal((1, 16)), rng.standard_normal((1, 2))]
    bad = [w.copy() for w in Ws]
    bad[1][0, 1, 7] = 1e39
    with pytest.raises(ValueError, match="overflows float32"):
        pop.update_(bad, bs, first=1)
    with pytest.raises(ValueError):
        pop.update_(Ws, bs, first=3)
    for got, want in zip(pop.weights + pop.biases, before):
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    pop.update_(Ws, bs, first=1)
    for l in range(2):
        assert pop.weights[l].dtype == np.float32 and np.array_equal(pop.weights[l][1], Ws[l][0].astype(np.float32))
        assert np.array_equal(pop.biases[l][1], bs[l][0].astype(np.float32))
        assert np.array_equal(pop.weights[l][[0, 2]], before[l][[0, 2]])


def test_fused_pop_ok_takes_a_float32_population_where_it_takes_a_float64_one():
    def spec_of(scen, **over):
        p = copy.deepcopy(SC.scenarios()[scen]["env_params"])
        p.update(**over)
        return EnvSpec(p)

    s = spec_of("cstr_canonical", integrator="rk4")
    pops = {d: PolicyPopulation.from_policies(_members(4, [s.nobs, 16, s.na], dtype=d)) for d in ("float32", "float64")}
    assert fused_pop_ok(s, pops["float32"], 64) and fused_pop_ok(s, pops["float64"], 64)
    assert fused_pop_ok(spec_of("cstr_canonical", integrator="cv8"), pops["float32"], 128)
    other = PolicyPopulation.from_policies(_members(4, [s.nobs + 1, 16, s.na]))
    refused = [(s, pops, 96), (s, pops, 32), (spec_of("cstr_canonical", integrator="dopri5"), pops, 64),
               (spec_of("cstr_cons_pen_norm", integrator="rk4"), pops, 64), (s, {"float32": other, "float64": other}, 64)]
    for spec, pp, g in refused:
        assert not fused_pop_ok(spec, pp["float64"], g) and not fused_pop_ok(spec, pp["float32"], g), (spec.integrator, g)
    assert not fused_pop_ok(s, pops["float32"].member(0), 64)  # (a single policy is not a population)
