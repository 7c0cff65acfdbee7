"""CPU: the host side of a population's weights on the device (pcg_policy_pop_nparams / _sample / _noise_dot / _get_flat /
_set_flat: declaration, export, ctypes signature, the statuses decided before the device is touched), the search purpose of
the RNG contract, PolicyPopulation.flat_layout / n_params against the order of examples/policy_search.py's ``unflatten``, and
rollout.centered_ranks.  The device side -- every kernel against the oracle's Philox and Box-Muller twins -- is
tests/test_gpu_pop_search.py."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from pcgym_amd import PolicyPopulation, centered_ranks
from pcgym_amd import _abi as abi
from pcgym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pcgym_hip.h")).read()
NEW = ["pcg_policy_pop_nparams", "pcg_policy_pop_sample", "pcg_policy_pop_noise_dot", "pcg_policy_pop_get_flat",
       "pcg_policy_pop_set_flat"]
# dims -> n = sum_l rows_l (cols_l + 1): tails of 0, 2, 3, 2 and 2 variates in the last block of four
DIMS = {(5, 2): 12, (3, 16, 2): 98, (4, 7, 3, 1): 63, (5, 64, 64, 2): 4674, (6, 64, 64, 2): 4738}


def test_header_declares_and_library_exports():
    assert abi.PCG_ABI_VERSION == 16 and _lib.load().pcg_version() == 16  # additive
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"PCG_API int %s\(" % name, HDR), name
        assert abi.EXPORTS.count(name) == 1
        assert raw[name] is not None  # (AttributeError if the library does not export it)
    assert len(set(abi.EXPORTS)) == len(abi.EXPORTS)
    doc = HDR[:HDR.index("PCG_API int pcg_policy_pop_nparams(")].rsplit("/*", 1)[1]
    assert "q = antithetic ? m >> 1 : m" in doc and "philox4x32_10(ctr = (q, j >> 2, g, PCG_RNG_SEARCH)" in doc
    assert "acc = acc + (w * z)" in doc and "PCG_ST_NONFINITE" in doc


def test_ctypes_signatures_equal_the_header():
    lib = _lib.load()
    vp = C.c_void_p
    ctype = {"const double*": vp, "double*": vp, "void*": vp, "const int32_t*": vp, "const pcg_policy_pop*": vp,
             "pcg_policy_pop*": vp, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
    names = {}
    for fn in NEW:
        m = re.search(r"PCG_API (\w+) %s\((.*?)\);" % fn, HDR, re.S)
        assert m and m.group(1) == "int" and getattr(lib, fn).restype is C.c_int
        params = [p_.strip() for p_ in m.group(2).replace("\n", " ").split(",")]
        names[fn] = [re.search(r"(\w+)$", p_).group(1) for p_ in params]
        assert [ctype[re.sub(r"\s*\w+$", "", p_).strip()] for p_ in params] == list(getattr(lib, fn).argtypes), fn
    assert names["pcg_policy_pop_nparams"] == ["pop"]
    assert names["pcg_policy_pop_sample"] == ["pop", "first", "count", "mean", "std", "antithetic", "seed", "generation", "stream"]
    assert names["pcg_policy_pop_noise_dot"] == ["pop", "first", "count", "antithetic", "seed", "generation", "w", "partial", "out",
                                                 "stream"]
    assert names["pcg_policy_pop_get_flat"] == ["pop", "members", "first", "count", "theta", "theta_member_stride", "stream"]
    assert names["pcg_policy_pop_set_flat"] == ["pop", "first", "count", "theta", "theta_member_stride", "stream"]


def test_the_search_purpose_is_a_word_of_its_own():
    assert abi.PCG_RNG_SEARCH == 0x500 and abi.PCG_POP_CHUNK == 64
    assert re.search(r"#define PCG_RNG_SEARCH 0x500\b", HDR) and re.search(r"#define PCG_POP_CHUNK 64\b", HDR)
    # the purposes of the engine's streams: the header's, and the kernels' own constants
    srcs = "".join(open(os.path.join(ROOT, "pc-gym_amd", "csrc", f)).read() for f in ("pcg_kernels.hpp", "pcg_rollout_actor.hpp"))
    purposes = {k: int(v, 0) for k, v in re.findall(r"\b(RNG_[A-Z]+) = (0x[0-9A-Fa-f]+)u", srcs)}
    assert {"RNG_NOISE", "RNG_DIST", "RNG_RESET", "RNG_POLICY", "RNG_SEARCH"} <= set(purposes), purposes
    assert purposes["RNG_SEARCH"] == abi.PCG_RNG_SEARCH and purposes["RNG_POLICY"] == abi.PCG_RNG_POLICY
    assert [k for k, v in purposes.items() if v == 0x500] == ["RNG_SEARCH"]
    assert [k for k in dir(abi) if k.startswith("PCG_RNG_") and getattr(abi, k) == 0x500] == ["PCG_RNG_SEARCH"]
    # (a purpose word carries the pair index in its low byte: no other purpose's blocks reach 0x500)
    assert all(v & 0xFF == 0 and (v == 0x500 or v + 0xFF < 0x500) for v in purposes.values())


def test_statuses_decided_on_the_host_for_a_null_population():
    """(this process has no GPU; nothing here may reach one)"""
    lib = _lib.load()
    buf = (C.c_double * 16)()
    idx = (C.c_int32 * 4)()
    d, i = C.addressof(buf), C.addressof(idx)
    assert lib.pcg_policy_pop_nparams(None) == abi.PCG_E_NULL
    assert lib.pcg_policy_pop_sample(None, 0, 1, d, d, 0, 1, 0, None) == abi.PCG_E_NULL
    assert lib.pcg_policy_pop_sample(None, -1, 0, None, None, 7, 1, 0, None) == abi.PCG_E_NULL  # NULL before everything else
    assert lib.pcg_policy_pop_noise_dot(None, 0, 1, 0, 1, 0, d, d, d, None) == abi.PCG_E_NULL
    assert lib.pcg_policy_pop_get_flat(None, i, 0, 1, d, 16, None) == abi.PCG_E_NULL
    assert lib.pcg_policy_pop_get_flat(None, None, 0, 1, d, 16, None) == abi.PCG_E_NULL
    assert lib.pcg_policy_pop_set_flat(None, 0, 1, d, 16, None) == abi.PCG_E_NULL
    # what is not a population (the magic word is read, nothing else)
    junk = (C.c_uint64 * 64)()
    j = C.addressof(junk)
    assert lib.pcg_policy_pop_nparams(j) == abi.PCG_E_PLAN
    assert lib.pcg_policy_pop_sample(j, 0, 1, d, d, 0, 1, 0, None) == abi.PCG_E_PLAN
    assert lib.pcg_policy_pop_sample(j, 0, 1, None, d, 0, 1, 0, None) == abi.PCG_E_NULL  # a NULL pointer before the handle
    assert lib.pcg_policy_pop_noise_dot(j, 0, 1, 0, 1, 0, d, d, d, None) == abi.PCG_E_PLAN
    assert lib.pcg_policy_pop_noise_dot(j, 0, 1, 0, 1, 0, d, None, d, None) == abi.PCG_E_NULL
    assert lib.pcg_policy_pop_get_flat(j, None, 0, 1, d, 16, None) == abi.PCG_E_PLAN
    assert lib.pcg_policy_pop_get_flat(j, None, 0, 1, None, 16, None) == abi.PCG_E_NULL
    assert lib.pcg_policy_pop_set_flat(j, 0, 1, d, 16, None) == abi.PCG_E_PLAN


def _unflatten():
    spec = importlib.util.spec_from_file_location("policy_search_example", os.path.join(ROOT, "examples", "policy_search.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # (main() runs under __main__ only)
    return mod.unflatten


@pytest.mark.parametrize("dims", sorted(DIMS))
def test_flat_layout_is_the_order_of_unflatten(dims):
    dims, n, P = list(dims), DIMS[dims], 3
    theta = np.arange(P * n, dtype=np.float64).reshape(P, n)  # every parameter its own number
    Ws, bs = _unflatten()(theta, dims)
    pop = PolicyPopulation(Ws, bs)
    assert pop.n_params == n == sum(dims[l + 1] * (dims[l] + 1) for l in range(len(dims) - 1))
    lay = pop.flat_layout()
    assert [(name, l) for name, l, *_ in lay] == [(k, l) for l in range(len(dims) - 1) for k in ("W", "b")]
    assert lay[0][2] == 0 and lay[-1][3] == n and all(a[3] == b[2] for a, b in zip(lay, lay[1:]))  # contiguous, ascending
    for name, l, start, stop, shape in lay:
        arr = (pop.weights if name == "W" else pop.biases)[l]
        assert shape == arr.shape[1:] == ((dims[l + 1], dims[l]) if name == "W" else (dims[l + 1],))
        assert np.array_equal(arr.reshape(P, -1), theta[:, start:stop]), (name, l)


def test_centered_ranks():
    s = torch.tensor([0.3, -1.0, 7.0, 0.3, 0.3, -1.0], dtype=torch.float64)
    r = centered_ranks(s)
    assert r.dtype == torch.float64 and r.shape == s.shape
    # ranks ascending in the score, ties in index order: -1.0 (1), -1.0 (5), 0.3 (0), 0.3 (3), 0.3 (4), 7.0 (2)
    want = torch.tensor([2, 0, 5, 3, 4, 1], dtype=torch.float64) / 5 - 0.5
    assert torch.equal(r, want)
    assert float(r.min()) == -0.5 and float(r.max()) == 0.5 and abs(float(r.sum())) < 1e-15
    assert torch.equal(centered_ranks(s), r)  # deterministic
    assert torch.equal(centered_ranks(s.to(torch.float32)), want) and torch.equal(centered_ranks(torch.tensor([4.0])), torch.zeros(1, dtype=torch.float64))
    assert torch.equal(centered_ranks(torch.zeros(4)), torch.tensor([-0.5, -0.5 + 1 / 3, -0.5 + 2 / 3, 0.5], dtype=torch.float64))
    with pytest.raises(ValueError):
        centered_ranks(torch.zeros((2, 2)))
    with pytest.raises(ValueError):
        centered_ranks(torch.zeros(0))


def test_a_population_never_written_from_the_device_reads_nothing_back():
    rng = np.random.default_rng(1)
    pop = PolicyPopulation([rng.standard_normal((4, 8, 3)), rng.standard_normal((4, 1, 8))],
                           [rng.standard_normal((4, 8)), rng.standard_normal((4, 1))])
    assert pop._stale is None and pop.n_params == 8 * 4 + 9
    w = pop.member(2).weights[0]
    pop.update_([x[:1] for x in pop.weights], [x[:1] for x in pop.biases], first=3)
    assert pop._stale is None and np.array_equal(pop.member(3).weights[0], pop.member(0).weights[0]) and np.array_equal(pop.member(2).weights[0], w)
    pop.close()
