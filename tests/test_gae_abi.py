"""CPU: the host side of pcg_gae (declaration, export, ctypes signature, every refusal status without a device) and the torch
loop of rollout.gae with its termination mask, bit for bit against a plain per-env loop.  The device side -- the kernel against
this loop, against numpy and against the oracle's episode -- is tests/test_gpu_gae.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from pcgym_amd import _abi as abi
from pcgym_amd import _lib, gae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pcgym_hip.h")).read()


def gae_numpy(rew, val, gamma, lam, bootstrap_last, term=None):
    """the rounding sequence of include/pcgym_hip.h (pcg_gae), one env at a time in Python floats (IEEE doubles, no
    contraction); np.float64 scalars so that an infinity or a NaN propagates instead of raising"""
    T, B = rew.shape
    adv, ret = np.empty((T, B)), np.empty((T, B))
    g, gl, zero = np.float64(gamma), np.float64(gamma * lam), np.float64(0.0)
    with np.errstate(all="ignore"):
        for e in range(B):
            carry = zero
            for t in range(T - 1, -1, -1):
                cut = (term is not None and term[t, e] != 0) or (t == T - 1 and not bootstrap_last)
                nxt = zero if cut else val[t + 1, e]
                c = zero if cut else carry
                delta = (rew[t, e] + g * nxt) - val[t, e]
                carry = delta + gl * c
                adv[t, e] = carry
                ret[t, e] = carry + val[t, e]
    return adv, ret


def gae_numpy_rows(rew, val, gamma, lam, bootstrap_last, term=None):
    """gae_numpy with every env of a row at once: the same operations element by element (numpy rounds each on its own), for
    the batch sizes of tests/test_gpu_gae.py; held against gae_numpy below"""
    T, B = rew.shape
    adv, ret = np.empty((T, B)), np.empty((T, B))
    g, gl = np.float64(gamma), np.float64(gamma * lam)
    carry, zero = np.zeros(B), np.zeros(B)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            cut = np.full(B, t == T - 1 and not bootstrap_last)
            if term is not None:
                cut |= term[t] != 0
            nxt, c = np.where(cut, zero, val[t + 1]), np.where(cut, zero, carry)
            delta = (rew[t] + g * nxt) - val[t]
            carry = delta + gl * c
            adv[t] = carry
            ret[t] = carry + val[t]
    return adv, ret


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def gae_before(rew, val, gamma=0.99, lam=0.95, bootstrap_last=False):
    """rollout.gae as it stood before `term` and `fused`, restated"""
    T = rew.shape[0]
    adv = torch.empty_like(rew)
    last = torch.zeros_like(rew[0])
    for t in range(T - 1, -1, -1):
        nxt = val[t + 1] if (t < T - 1 or bootstrap_last) else torch.zeros_like(val[t])
        delta = rew[t] + gamma * nxt - val[t]
        last = delta + gamma * lam * last
        adv[t] = last
    return adv, adv + val[:T]


def case(T, B, seed=0):
    """rewards and values with signed zeros and subnormals among them"""
    rng = np.random.default_rng(seed)
    rew, val = rng.standard_normal((T, B)), rng.standard_normal((T + 1, B))
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1030, -(2.0 ** -1040)])
    for a in (rew, val):
        m = rng.random(a.shape) < 0.1
        a[m] = rng.choice(special, int(m.sum()))
    rew[:, 0], val[:, 0] = rng.choice(special, T), rng.choice(special, T + 1)
    return rew, val


def test_header_declares_and_library_exports():
    assert abi.PCG_ABI_VERSION == 16 and _lib.load().pcg_version() == 16  # additive
    assert re.search(r"PCG_API int pcg_gae\(", HDR) and "pcg_gae" in abi.EXPORTS
    assert C.CDLL(_lib.LIB_PATH)["pcg_gae"] is not None  # (AttributeError if the library does not export it)
    doc = HDR[:HDR.index("PCG_API int pcg_gae(")].rsplit("/*", 1)[1]
    assert "compute_returns_and_advantage" in doc and "delta = (rew[t] + gamma * nxt) - val[t]" in doc and "carry = delta + gl * c" in doc


def test_ctypes_signature_equals_the_header():
    lib = _lib.load()
    vp = C.c_void_p
    ctype = {"const double*": vp, "double*": vp, "const uint8_t*": vp, "void*": vp, "int32_t": C.c_int32, "int64_t": C.c_int64,
             "double": C.c_double}
    m = re.search(r"PCG_API (\w+) pcg_gae\((.*?)\);", HDR, re.S)
    assert m and m.group(1) == "int" and lib.pcg_gae.restype is C.c_int
    params = [p_.strip() for p_ in m.group(2).replace("\n", " ").split(",")]
    names = [re.search(r"(\w+)$", p_).group(1) for p_ in params]
    assert names == ["B", "T", "rew", "rew_step_stride", "val", "val_step_stride", "term", "term_step_stride", "gamma", "lam",
                     "bootstrap_last", "adv", "adv_step_stride", "ret", "ret_step_stride", "stream"]
    assert [ctype[re.sub(r"\s*\w+$", "", p_).strip()] for p_ in params] == list(lib.pcg_gae.argtypes)


def test_every_refusal_without_a_device():
    lib = _lib.load()
    B, T = 8, 3
    host = np.zeros(64)  # host memory: every call below is refused before anything could be launched
    p = host.ctypes.data
    inf, nan = float("inf"), float("nan")

    def call(B=B, T=T, rew=p, rs=B, val=p, vs=B, term=None, ts=0, gamma=0.99, lam=0.95, adv=p, as_=B, ret=p, rets=B):
        return lib.pcg_gae(B, T, rew, rs, val, vs, term, ts, gamma, lam, 0, adv, as_, ret, rets, None)

    assert call(rew=None) == call(val=None) == call(adv=None) == abi.PCG_E_NULL
    assert call(rew=None, B=0, gamma=nan) == abi.PCG_E_NULL  # NULL comes first
    assert call(B=0) == call(B=-1) == call(T=0) == call(T=-5) == abi.PCG_E_DIM
    assert call(rs=B - 1) == call(vs=B - 1) == call(as_=B - 1) == call(rets=B - 1) == call(term=p, ts=B - 1) == abi.PCG_E_DIM
    assert call(rs=0) == call(vs=-B) == abi.PCG_E_DIM
    assert call(T=1, vs=B - 1) == abi.PCG_E_DIM  # val has T + 1 rows: its stride counts with a single step too
    assert call(vs=B - 1, gamma=inf) == abi.PCG_E_DIM  # sizes before values
    for g, l in ((inf, 0.95), (-inf, 0.95), (nan, 0.95), (0.99, inf), (0.99, nan)):
        assert call(gamma=g, lam=l) == abi.PCG_E_VALUE
    # a single step has no row stride: only val's is looked at; ret == NULL and term's stride without term are never looked at
    assert call(T=1, rs=0, as_=0, rets=0, term=p, ts=0, gamma=nan) == abi.PCG_E_VALUE
    assert call(ret=None, rets=0, ts=-1, gamma=nan) == abi.PCG_E_VALUE
    assert lib.pcg_strerror(abi.PCG_E_DIM) and host.sum() == 0.0


@pytest.mark.parametrize("bootstrap_last", [False, True])
@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0)])
def test_term_on_cpu_equals_a_plain_loop_bitwise(gamma, lam, bootstrap_last):
    T, B = 23, 17
    rew, val = case(T, B, seed=3)
    val[:, 5] = np.inf
    rew[4, 6] = -np.inf
    rng = np.random.default_rng(1)
    for term in (rng.random((T, B)) < 0.1, np.ones((T, B), dtype=bool), np.zeros((T, B), dtype=bool)):
        want = gae_numpy(rew, val, gamma, lam, bootstrap_last, term)
        rows = gae_numpy_rows(rew, val, gamma, lam, bootstrap_last, term)
        for w, r in zip(want, rows):
            assert np.array_equal(np.isnan(w), np.isnan(r)) and np.array_equal(bits(w)[~np.isnan(w)], bits(r)[~np.isnan(w)])
        for tt in (torch.as_tensor(term), torch.as_tensor(term.astype(np.uint8) * 3)):
            adv, ret = gae(torch.as_tensor(rew), torch.as_tensor(val), gamma, lam, bootstrap_last, term=tt)
            nan = np.isnan(want[0])
            assert np.array_equal(np.isnan(adv.numpy()), nan) and np.array_equal(np.isnan(ret.numpy()), np.isnan(want[1]))
            assert np.array_equal(bits(adv.numpy())[~nan], bits(want[0])[~nan])
            assert np.array_equal(bits(ret.numpy())[~np.isnan(want[1])], bits(want[1])[~np.isnan(want[1])])
    # the cut is a cut: an env's advantage at a terminal step is rew - val there, whatever follows
    term = np.zeros((T, B), dtype=bool)
    term[7] = True
    adv, _ = gae(torch.as_tensor(rew), torch.as_tensor(val), gamma, lam, bootstrap_last, term=torch.as_tensor(term))
    fin = np.isfinite(val[7]) & np.isfinite(rew[7])
    assert np.array_equal(adv.numpy()[7][fin], ((rew[7] + gamma * 0.0) - val[7] + gamma * lam * 0.0)[fin])


@pytest.mark.parametrize("bootstrap_last", [False, True])
def test_without_term_the_values_are_those_of_the_loop_as_it_stood(bootstrap_last):
    rew, val = (torch.as_tensor(a) for a in case(23, 17, seed=4))
    for gamma, lam in ((0.99, 0.95), (1.0, 1.0), (0.9, 0.0)):
        want = gae_before(rew, val, gamma, lam, bootstrap_last)
        for kw in ({}, {"fused": False}, {"term": None}):
            got = gae(rew, val, gamma, lam, bootstrap_last, **kw)
            assert torch.equal(got[0].view(torch.int64), want[0].view(torch.int64))
            assert torch.equal(got[1].view(torch.int64), want[1].view(torch.int64))
        n = gae_numpy(rew.numpy(), val.numpy(), gamma, lam, bootstrap_last)
        assert np.array_equal(bits(want[0].numpy()), bits(n[0])) and np.array_equal(bits(want[1].numpy()), bits(n[1]))


def test_a_true_last_row_is_bootstrap_last_false():
    T, B = 11, 9
    rew, val = (torch.as_tensor(a) for a in case(T, B, seed=5))
    term = torch.zeros((T, B), dtype=torch.bool)
    term[T - 1] = True
    want = gae(rew, val, 0.97, 0.9, bootstrap_last=False)
    for bl in (False, True):
        got = gae(rew, val, 0.97, 0.9, bootstrap_last=bl, term=term)
        assert torch.equal(got[0].view(torch.int64), want[0].view(torch.int64))
        assert torch.equal(got[1].view(torch.int64), want[1].view(torch.int64))
    other = gae(rew, val, 0.97, 0.9, bootstrap_last=True)
    assert not torch.equal(other[0], want[0])


def test_fused_true_on_cpu_tensors_raises_and_bad_masks_are_refused():
    rew, val = (torch.as_tensor(a) for a in case(5, 4))
    with pytest.raises(ValueError, match="GPU"):
        gae(rew, val, fused=True)
    with pytest.raises(ValueError):
        gae(rew, val, term=torch.zeros((4, 4), dtype=torch.bool))  # another shape
    with pytest.raises(ValueError):
        gae(rew, val, term=torch.zeros((5, 4), dtype=torch.float64))  # not a mask
    with pytest.raises(ValueError):
        gae(rew, val[:5])
    # three dimensions stay with the torch loop, as before
    r3, v3 = torch.randn(5, 2, 3, dtype=torch.float64), torch.randn(6, 2, 3, dtype=torch.float64)
    a3, _ = gae(r3, v3)
    a2, _ = gae(r3.reshape(5, 6), v3.reshape(6, 6))
    assert torch.equal(a3.reshape(5, 6), a2)
