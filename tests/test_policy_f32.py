"""CPU: the float32 kind of MLPPolicy / GaussianActorCritic (``dtype="float32"``) and its C ABI additions
(pcg_policy_create_f32, pcg_policy_dtype, PCG_POL_F64 / PCG_POL_F32; ABI 16 unchanged).  The in-kernel evaluation is tested on
the GPU (tests/test_gpu_policy_f32.py); here: storage, rounding, the torch callable, which plans take the fused calls.

The callable is held to the float32 running bound of the GPU tests (helpers.host_reference's recursion with u = 2^-24, the
reference in np.longdouble on the float32 weights and on float32(obs), n 2^-149 per layer for underflow, k + 1 float32 ulps
per tanh): it holds for any summation order, with one rounding per FMA or with products and sums rounded separately (the
classic gamma_n of an n-term inner product).  k of torch's own float32 tanh is measured here, on the grid of the GPU test.
"""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import scenarios as SC
from pcgym_amd import GaussianActorCritic, MLPPolicy, _lib
from pcgym_amd import _abi as abi
from pcgym_amd.config import EnvSpec
from pcgym_amd.policy import fused_actor_ok, fused_policy_ok
from test_policy_jit_plans import _chemostat, _traced_reward

LD = np.longdouble
U32 = 2.0 ** -24
HDR = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "pcgym_hip.h")).read()


def _arrays(dims, seed=0):
    rng = np.random.default_rng(seed)
    Ws = [rng.standard_normal((dims[l + 1], dims[l])) / np.sqrt(dims[l]) for l in range(len(dims) - 1)]
    bs = [0.1 * rng.standard_normal(dims[l + 1]) for l in range(len(dims) - 1)]
    return Ws, bs


def _seq(dims, act=torch.nn.Tanh, seed=0):
    torch.manual_seed(seed)
    mods = []
    for l in range(len(dims) - 1):
        mods.append(torch.nn.Linear(dims[l], dims[l + 1]))
        if l < len(dims) - 2:
            mods.append(act())
    return torch.nn.Sequential(*mods)


def tanh32_grid():
    """float32 values of [-24, 24], dense around [-1, 1], and +-geomspace down to 1e-30"""
    g = np.concatenate([np.linspace(-24.0, 24.0, (1 << 18) + 1), np.linspace(-1.0, 1.0, (1 << 17) + 1),
                        np.geomspace(1e-30, 1.0, 4096), -np.geomspace(1e-30, 1.0, 4096)])
    return g.astype(np.float32)


def tanh32_ulps(got, grid):
    """largest error of float32 results `got` = tanh(grid) in float32 ulps of the exact value"""
    want = np.tanh(grid.astype(LD))
    ulp = np.spacing(np.abs(want.astype(np.float32))).astype(np.float64)
    return float(np.max(np.abs(got.astype(LD) - want).astype(np.float64) / ulp))


def bound32(pol, obs, k_tanh):
    """(reference in np.longdouble (n_out, M) on the float32 weights and float32(obs), running error bound of a float32
    evaluation, any summation order, largest |pre-activation|).  helpers.host_reference with u = 2^-24 and n 2^-149 per
    layer for underflow; the cast of obs to float32 is part of the specification, not an error term."""
    def gamma(n):
        return n * U32 / (1 - n * U32)

    h = obs.astype(np.float32).astype(LD)
    E = np.zeros(obs.shape)
    pre = 0.0
    L = len(pol.weights)
    for l, (W, b) in enumerate(zip(pol.weights, pol.biases)):
        assert W.dtype == np.float32 and b.dtype == np.float32
        aW = np.abs(W).astype(np.float64)
        mag = aW @ (np.abs(h).astype(np.float64) + E) + np.abs(b).astype(np.float64)[:, None]
        E = gamma(W.shape[1] + 1) * mag + aW @ E + W.shape[1] * 2.0 ** -149
        h = W.astype(LD) @ h + b.astype(LD)[:, None]
        if l < L - 1:
            pre = max(pre, float(np.max(np.abs(h))))
            h = np.tanh(h) if pol.activation == "tanh" else np.maximum(h, 0)
            if pol.activation == "tanh":
                E = E + k_tanh * 2.0 ** -23 * (np.abs(h).astype(np.float64) + E)
    if pol.out_map == "clip":
        h = np.clip(h, LD(pol.out_low), LD(pol.out_high))
    elif pol.out_map == "tanh":
        h = np.tanh(h)
        E = E + k_tanh * 2.0 ** -23 * (np.abs(h).astype(np.float64) + E)
    return h, E * (1 + 2.0 ** -10), pre


def test_the_default_dtype_is_float64_and_changes_nothing():
    Ws, bs = _arrays([5, 16, 2])
    pol, pol64 = MLPPolicy(Ws, bs, out_low=-0.3, out_high=0.7), MLPPolicy(Ws, bs, out_low=-0.3, out_high=0.7, dtype="float64")
    for p in (pol, pol64):
        assert p.dtype == "float64" and all(w.dtype == np.float64 for w in p.weights + p.biases)
        assert all(np.array_equal(w, v) for w, v in zip(p.weights + p.biases, Ws + bs))
        assert (p.out_low, p.out_high) == (-0.3, 0.7)
        cfg, keep = p.to_cfg()
        assert (cfg.n_in, cfg.n_out, cfg.n_hidden, cfg.width[0], cfg.out_low, cfg.out_high) == (5, 2, 1, 16, -0.3, 0.7)
        for l in range(2):  # the cfg points at the policy's own arrays, as before
            assert C.addressof(cfg.W[l].contents) == p.weights[l].ctypes.data and C.addressof(cfg.b[l].contents) == p.biases[l].ctypes.data
        assert p.validate() == 0
    obs = torch.as_tensor(np.random.default_rng(1).uniform(-1, 1, (9, 5)))
    out = pol(obs)
    assert out.dtype == torch.float64 and torch.equal(out, pol64(obs))
    h = obs
    for l, (w, b) in enumerate(zip(Ws, bs)):  # today's callable, restated
        h = torch.addmm(torch.as_tensor(b), h, torch.as_tensor(w).t())
        if l == 0:
            h = torch.tanh(h)
    assert torch.equal(out, torch.clamp(h, -0.3, 0.7))
    with pytest.raises(ValueError, match="dtype"):
        MLPPolicy(Ws, bs, dtype="float16")


def test_float32_rounds_to_nearest_and_overflow_raises():
    Ws, bs = _arrays([4, 7, 1], seed=3)
    pol = MLPPolicy(Ws, bs, out_low=-1 / 3, out_high=0.1, dtype="float32")
    assert pol.dtype == "float32" and all(w.dtype == np.float32 for w in pol.weights + pol.biases)
    for got, src in zip(pol.weights + pol.biases, Ws + bs):
        assert np.array_equal(got, src.astype(np.float32)) and not np.array_equal(got.astype(np.float64), src)
        assert np.all(np.abs(got.astype(LD) - src.astype(LD)) <= np.spacing(np.abs(got)).astype(LD) / 2)  # nearest
    assert pol.out_low == float(np.float32(-1 / 3)) and pol.out_high == float(np.float32(0.1))
    assert pol.validate() == 0
    cfg, keep = pol.to_cfg()  # the cfg carries exact widenings
    assert np.array_equal(np.ctypeslib.as_array(cfg.W[0], shape=(7, 4)), pol.weights[0].astype(np.float64))
    for bad in (3.5e38, -1e300):
        W2 = [Ws[0].copy(), Ws[1]]
        W2[0][2, 1] = bad
        with pytest.raises(ValueError, match="overflows float32"):
            MLPPolicy(W2, bs, dtype="float32")
        assert MLPPolicy(W2, bs).validate() == 0  # (a float64 policy holds it)
        b2 = [bs[0], np.array([bad])]
        with pytest.raises(ValueError, match="overflows float32"):
            MLPPolicy(Ws, b2, dtype="float32")
    with pytest.raises(ValueError, match="overflows float32"):
        MLPPolicy(Ws, bs, out_high=1e39, dtype="float32")
    assert MLPPolicy([Ws[0] * 0 + 3.4028234e38, Ws[1]], bs, dtype="float32").weights[0][0, 0] == np.finfo(np.float32).max


def test_from_torch_holds_a_float32_module_bitwise():
    seq = _seq([6, 64, 64, 2])
    pol = MLPPolicy.from_torch(seq, dtype="float32")
    lin = [m for m in seq if isinstance(m, torch.nn.Linear)]
    assert pol.dtype == "float32" and pol.n_hidden == 2
    for l, m in enumerate(lin):
        assert m.weight.dtype == torch.float32
        assert np.array_equal(pol.weights[l].view(np.int32), m.weight.detach().numpy().view(np.int32))
        assert np.array_equal(pol.biases[l].view(np.int32), m.bias.detach().numpy().view(np.int32))
    legacy = MLPPolicy.from_torch(seq)  # dtype=None: today's behaviour
    assert legacy.dtype == "float64" and all(w.dtype == np.float64 for w in legacy.weights)
    assert np.array_equal(legacy.weights[0], lin[0].weight.detach().double().numpy())
    ac = GaussianActorCritic.from_torch(seq, torch.zeros(2), _seq([6, 8, 1], seed=1), dtype="float32")
    assert ac.actor.dtype == ac.critic.dtype == "float32"


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("out_map", ["clip", "none", "tanh"])
@pytest.mark.parametrize("dims", [[6, 2], [6, 16, 2], [6, 64, 64, 2]])
def test_the_float32_callable(dims, out_map, act):
    seq = _seq(dims, torch.nn.Tanh if act == "tanh" else torch.nn.ReLU)
    if out_map == "tanh":
        seq = torch.nn.Sequential(*seq, torch.nn.Tanh())
    obs = torch.as_tensor(np.random.default_rng(2).uniform(-2, 2, (257, dims[0])))  # float64 observations, as the env gives them
    lo, hi = -0.25, 0.25
    if out_map == "clip":  # a box that cuts on both sides: quantiles of the network's own raw outputs
        r0 = MLPPolicy.from_torch(seq, out_map="none", dtype="float32").raw(obs).numpy()
        lo, hi = float(np.float32(np.quantile(r0, 0.2))), float(np.float32(np.quantile(r0, 0.8)))
    pol = MLPPolicy.from_torch(seq, out_map=out_map, out_low=lo, out_high=hi, dtype="float32")
    assert pol.out_map == out_map and (pol.out_low, pol.out_high) == (lo, hi)
    out, raw = pol(obs), pol.raw(obs)
    assert out.dtype == raw.dtype == torch.float64 and out.shape == (257, dims[-1])
    for t in (out, raw):  # exact widenings of float32 results
        assert torch.equal(t, t.to(torch.float32).to(torch.float64))
    if out_map != "clip":
        with torch.no_grad():
            want = seq(obs.float())
        assert want.dtype == torch.float32
        grid = tanh32_grid()
        k = tanh32_ulps(torch.tanh(torch.as_tensor(grid)).numpy(), grid)
        assert np.isfinite(k) and k <= 16.0, f"torch's float32 tanh is {k} ulp off: not a libm-class tanh"
        ref, bound, _ = bound32(pol, obs.numpy().T, k + 1.0)
        for got in (out.numpy().T, want.double().numpy().T):
            assert np.all(np.abs(got.astype(LD) - ref).astype(np.float64) <= bound), float(np.max(np.abs(got.astype(LD) - ref).astype(np.float64) / bound))
        assert float(np.max(bound)) < 1e-4
    else:
        assert torch.equal(out, torch.clamp(raw, lo, hi)) and bool((out == hi).any()) and bool((out == lo).any()) and bool(((out > lo) & (out < hi)).any())
    # not the float64 policy's numbers
    wide = MLPPolicy([w.astype(np.float64) for w in pol.weights], [b.astype(np.float64) for b in pol.biases], activation=act, out_map=out_map,
                     out_low=lo, out_high=hi)
    assert not torch.equal(wide.raw(obs), raw)


def test_update_keeps_the_dtype_and_refuses_a_shape_change():
    Ws, bs = _arrays([4, 9, 2], seed=5)
    W2, b2 = _arrays([4, 9, 2], seed=6)
    pol = MLPPolicy(Ws, bs, dtype="float32")
    obs = torch.as_tensor(np.random.default_rng(0).uniform(-1, 1, (5, 4)))
    before = pol(obs)
    assert pol.update_(W2, b2) is pol and pol.dtype == "float32"
    assert all(np.array_equal(w, v.astype(np.float32)) and w.dtype == np.float32 for w, v in zip(pol.weights + pol.biases, W2 + b2))
    assert torch.equal(pol(obs), MLPPolicy(W2, b2, dtype="float32")(obs)) and not torch.equal(pol(obs), before)
    W3, b3 = _arrays([4, 10, 2], seed=6)
    with pytest.raises(ValueError, match="keeps the shape"):
        pol.update_(W3, b3)
    assert all(np.array_equal(w, v.astype(np.float32)) for w, v in zip(pol.weights, W2))
    bad = [W2[0].copy(), W2[1]]
    bad[0][0, 0] = 1e39
    with pytest.raises(ValueError, match="overflows float32"):
        pol.update_(bad, b2)
    assert all(np.array_equal(w, v.astype(np.float32)) for w, v in zip(pol.weights, W2))
    ac = GaussianActorCritic(MLPPolicy(Ws, bs, dtype="float32"), np.zeros(2))
    ac.update_(actor=_seq([4, 9, 2], seed=4))
    assert ac.actor.dtype == "float32" and ac.actor.weights[0].dtype == np.float32


def test_actor_and_critic_have_one_dtype():
    Ws, bs = _arrays([4, 8, 2])
    Wc, bc = _arrays([4, 8, 1], seed=1)
    for da, dc in (("float32", "float64"), ("float64", "float32")):
        with pytest.raises(ValueError, match="one dtype"):
            GaussianActorCritic(MLPPolicy(Ws, bs, dtype=da), np.zeros(2), MLPPolicy(Wc, bc, out_map="none", dtype=dc))
    ac = GaussianActorCritic(MLPPolicy(Ws, bs, dtype="float32"), np.full(2, -1.0), MLPPolicy(Wc, bc, out_map="none", dtype="float32"))
    obs = torch.as_tensor(np.random.default_rng(0).uniform(-1, 1, (33, 4)))
    z = torch.as_tensor(np.random.default_rng(1).standard_normal((33, 2)))
    mu, v = ac.mean(obs), ac.value(obs)
    assert mu.dtype == v.dtype == torch.float64
    assert torch.equal(mu, mu.float().double()) and torch.equal(v, v.float().double())
    u = ac.sample(obs, z)  # fp64, today's formulas
    assert u.dtype == torch.float64 and torch.equal(u, torch.addcmul(mu, torch.as_tensor(ac.sigma), z))
    assert not torch.equal(u, u.float().double())
    q = z[:, 0] * z[:, 0] + z[:, 1] * z[:, 1]
    assert torch.equal(ac.log_prob_z(z), ac.logp_const - 0.5 * q) and ac.log_prob(obs, u).dtype == torch.float64


def _nets32(spec, hidden=(16,)):
    Ws, bs = _arrays([spec.nobs, *hidden, spec.na])
    pol = MLPPolicy(Ws, bs, dtype="float32")
    critic = MLPPolicy(Ws[:-1] + [Ws[-1][:1]], bs[:-1] + [bs[-1][:1]], out_map="none", dtype="float32")
    return pol, GaussianActorCritic(pol, np.full(spec.na, -1.0), critic)


@pytest.mark.parametrize("integ", ["rk4", "cv8"])
def test_a_float32_policy_takes_the_fused_calls_on_built_in_plans_only(integ):
    p = copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"])
    p.update(integrator=integ)
    spec = EnvSpec(p)
    pol, ac = _nets32(spec)
    assert fused_policy_ok(spec, pol) and fused_actor_ok(spec, ac)
    for make in (_chemostat, _traced_reward):  # run-time compiled code: the fp64 kernels only
        jit = EnvSpec(make(integrator=integ))
        pol, ac = _nets32(jit)
        assert not fused_policy_ok(jit, pol) and not fused_actor_ok(jit, ac)
        p64 = MLPPolicy([w.astype(np.float64) for w in pol.weights], [b.astype(np.float64) for b in pol.biases])
        assert fused_policy_ok(jit, p64)


@pytest.mark.parametrize("over", [
    dict(integrator="dopri5"), dict(integrator="rodas4"), dict(integrator="tsit5"),
    dict(integrator="rk4", uncertainty_percentages={"q": 0.03}, distribution="uniform",
         uncertainty_bounds={"low": np.array([90.0]), "high": np.array([110.0])}),
], ids=["dopri5", "rodas4", "tsit5", "per_env_parameters"])
def test_a_float32_policy_steps_where_a_float64_policy_steps(over):
    p = copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"])
    p.update(over)
    spec = EnvSpec(p)
    pol, ac = _nets32(spec)
    assert not fused_policy_ok(spec, pol) and not fused_actor_ok(spec, ac)
    cons = EnvSpec(dict(copy.deepcopy(SC.scenarios()["cstr_cons_pen_norm"]["env_params"]), integrator="rk4"))
    pol, ac = _nets32(cons)
    assert cons.ncon and not fused_policy_ok(cons, pol) and not fused_actor_ok(cons, ac)
    ok = EnvSpec(dict(copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"]), integrator="rk4"))
    wrong = MLPPolicy([np.zeros((ok.na, ok.nobs + 1))], [np.zeros(ok.na)], dtype="float32")
    assert not fused_policy_ok(ok, wrong)


def test_header_mirror_and_library_agree_on_the_additions():
    assert int(re.search(r"#define PCG_ABI_VERSION (\d+)", HDR).group(1)) == 16 == abi.PCG_ABI_VERSION
    lib = _lib.load()
    assert lib.pcg_version() == 16
    for name, val in (("PCG_POL_F64", 0), ("PCG_POL_F32", 1)):
        assert int(re.search(r"#define %s (\d+)" % name, HDR).group(1)) == val == getattr(abi, name)
    m = re.search(r"PCG_API\s+(\w+)\s+pcg_policy_create_f32\(([^)]*)\);", HDR)
    assert m and m.group(1) == "int" and re.sub(r"\s+", " ", m.group(2)).strip() == "pcg_policy** out, const pcg_policy_cfg* cfg"
    m = re.search(r"PCG_API\s+(\w+)\s+pcg_policy_dtype\(([^)]*)\);", HDR)
    assert m and m.group(1) == "int" and re.sub(r"\s+", " ", m.group(2)).strip() == "const pcg_policy* policy"
    for sym in ("pcg_policy_create_f32", "pcg_policy_dtype"):
        assert sym in abi.EXPORTS and getattr(lib, sym).restype is C.c_int
    assert lib.pcg_policy_dtype(None) == abi.PCG_E_NULL
    junk = C.create_string_buffer(256)
    assert lib.pcg_policy_dtype(C.cast(junk, C.c_void_p)) == abi.PCG_E_PLAN
    # host-side refusals of the new constructor come before the device is touched
    assert lib.pcg_policy_create_f32(None, None) == abi.PCG_E_NULL
    h = C.c_void_p()
    assert lib.pcg_policy_create_f32(C.byref(h), None) == abi.PCG_E_NULL and not h.value
    Ws, bs = _arrays([4, 7, 1])
    Ws[0][1, 1] = 1e39  # finite in double, not after rounding
    cfg, keep = MLPPolicy(Ws, bs).to_cfg()
    assert lib.pcg_policy_validate(C.byref(cfg)) == 0
    assert lib.pcg_policy_create_f32(C.byref(h), C.byref(cfg)) == abi.PCG_E_VALUE and not h.value
    cfg.n_out = 99
    assert lib.pcg_policy_create_f32(C.byref(h), C.byref(cfg)) == abi.PCG_E_DIM
    doc = re.sub(r"\s*\n\s*\*\s*", " ", HDR)
    for phrase in ("rounded to the nearest float32", "run-time compiled code", "different dtypes"):
        assert phrase in doc, phrase
