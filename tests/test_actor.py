"""CPU: the stochastic actor-critic (policy.py GaussianActorCritic), the GAE helper (rollout.py) and the host side of the ABI-16
entry points (pcg_rollout_actor, pcg_policy_noise, pcg_policy_update, pcg_actor_logp_const).  The device side is
tests/test_gpu_actor_rollout.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from pcgym_amd import GaussianActorCritic, MLPPolicy, gae
from pcgym_amd import _abi as abi
from pcgym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pcgym_hip.h")).read()


def make_ac(n_in=5, n_out=2, hidden=(16,), seed=0, out_map="clip", critic=True, log_std=None):
    rng = np.random.default_rng(seed)

    def net(n_last, om):
        dims = [n_in, *hidden, n_last]
        Ws = [rng.standard_normal((dims[l + 1], dims[l])) / np.sqrt(dims[l]) for l in range(len(dims) - 1)]
        bs = [0.1 * rng.standard_normal(dims[l + 1]) for l in range(len(dims) - 1)]
        return MLPPolicy(Ws, bs, activation="tanh", out_map=om, out_low=-0.5, out_high=0.7)

    ls = rng.uniform(-1.5, 0.3, n_out) if log_std is None else log_std
    return GaussianActorCritic(net(n_out, out_map), ls, net(1, "none") if critic else None)


@pytest.mark.parametrize("n_out", [1, 2, 5])
@pytest.mark.parametrize("hidden", [(), (16,), (64, 64)])
def test_log_prob_matches_torch_distributions(n_out, hidden):
    ac = make_ac(n_out=n_out, hidden=hidden, seed=n_out)
    g = torch.Generator().manual_seed(1)
    obs = torch.randn(301, 5, dtype=torch.float64, generator=g)
    z = torch.randn(301, n_out, dtype=torch.float64, generator=g)
    u = ac.sample(obs, z)
    mu = ac.mean(obs)
    ref = torch.distributions.Normal(mu, torch.as_tensor(ac.sigma)).log_prob(u).sum(-1)
    got = ac.log_prob(obs, u)
    assert got.shape == (301,) and got.dtype == torch.float64
    rel = float(torch.max(torch.abs(got - ref) / torch.abs(ref).clamp_min(1.0)))
    assert rel <= 1e-13, rel
    # from the normals themselves: the kernel's statement
    rel = float(torch.max(torch.abs(ac.log_prob_z(z) - ref) / torch.abs(ref).clamp_min(1.0)))
    assert rel <= 1e-13, rel
    # the constant: -(sum log sigma + na/2 log 2 pi), the library's own figure
    want = -(math.fsum(np.log(ac.sigma)) + 0.5 * n_out * math.log(2 * math.pi))
    # (one rounding per log and per addition, each at most 2^-53 of the sum of the terms' magnitudes)
    mag = float(np.sum(np.abs(np.log(ac.sigma)))) + 0.5 * n_out * math.log(2 * math.pi)
    assert abs(ac.logp_const - want) <= (2 * n_out + 2) * 2.0 ** -53 * mag
    assert np.array_equal(ac.sigma, np.exp(ac.log_std))


def test_sample_is_mean_plus_sigma_z_and_raw_precedes_the_map():
    ac = make_ac(seed=4)
    g = torch.Generator().manual_seed(2)
    obs = torch.randn(257, 5, dtype=torch.float64, generator=g)
    z = torch.randn(257, 2, dtype=torch.float64, generator=g)
    mu = ac.mean(obs)
    want = mu + torch.as_tensor(ac.sigma) * z
    got = ac.sample(obs, z)
    assert float(torch.max(torch.abs(got - want))) <= 4 * 2.0 ** -53 * float(torch.max(torch.abs(want)).clamp_min(1.0))
    assert torch.equal(ac.sample(obs, torch.zeros_like(z)), mu)
    # MLPPolicy.raw is the output before the map, __call__ the map of it
    pol = ac.actor
    assert torch.equal(mu, pol.raw(obs)) and torch.equal(pol(obs), torch.clamp(pol.raw(obs), -0.5, 0.7))
    assert torch.equal(ac.action(got), torch.clamp(got, -0.5, 0.7))
    a = ac.action(got)
    inside = float(((a > -0.5) & (a < 0.7)).double().mean())
    assert 0.05 < inside < 1.0  # both branches of the clip
    v = ac.value(obs)
    assert v.shape == (257,) and torch.equal(v, ac.critic.raw(obs)[:, 0])
    with pytest.raises(ValueError):
        make_ac(critic=False).value(obs)


def test_from_torch_and_update_round_trip():
    nn = torch.nn
    torch.manual_seed(0)
    actor = nn.Sequential(nn.Linear(4, 16), nn.Tanh(), nn.Linear(16, 16), nn.Tanh(), nn.Linear(16, 2)).double()
    critic = nn.Sequential(nn.Linear(4, 8), nn.Tanh(), nn.Linear(8, 1)).double()
    log_std = nn.Parameter(torch.tensor([-0.5, 0.25], dtype=torch.float64))
    ac = GaussianActorCritic.from_torch(actor, log_std, critic, out_low=-2.0, out_high=2.0)
    assert (ac.n_in, ac.n_out, ac.actor.out_map, ac.critic.out_map, ac.critic.n_out) == (4, 2, "clip", "none", 1)
    assert np.array_equal(ac.sigma, np.exp([-0.5, 0.25]))
    obs = torch.randn(41, 4, dtype=torch.float64)
    with torch.no_grad():
        assert float(torch.max(torch.abs(ac.mean(obs) - actor(obs)))) <= 1e-14
        assert float(torch.max(torch.abs(ac.value(obs) - critic(obs)[:, 0]))) <= 1e-14
    # an "optimiser step", then update_: the host arrays and the torch callable follow
    with torch.no_grad():
        for prm in list(actor.parameters()) + list(critic.parameters()):
            prm.add_(0.05 * torch.randn_like(prm))
        log_std.add_(0.1)
    c_before = ac.logp_const
    assert ac.update_(actor=actor, log_std=log_std, critic=critic) is ac
    with torch.no_grad():
        assert float(torch.max(torch.abs(ac.mean(obs) - actor(obs)))) <= 1e-14
        assert float(torch.max(torch.abs(ac.value(obs) - critic(obs)[:, 0]))) <= 1e-14
    assert np.allclose(ac.sigma, np.exp([-0.4, 0.35]), rtol=1e-15) and abs((c_before - ac.logp_const) - 0.2) <= 1e-14
    # (weights, biases) pairs work too; a shape change is refused and changes nothing
    w, b = [x.copy() for x in ac.actor.weights], [x.copy() for x in ac.actor.biases]
    w[0][0, 0] = 3.25
    ac.update_(actor=(w, b))
    assert ac.actor.weights[0][0, 0] == 3.25
    wide = nn.Sequential(nn.Linear(4, 17), nn.Tanh(), nn.Linear(17, 16), nn.Tanh(), nn.Linear(16, 2)).double()
    with pytest.raises(ValueError):
        ac.update_(actor=wide)
    assert ac.actor.weights[0].shape == (16, 4) and ac.actor.weights[0][0, 0] == 3.25
    with pytest.raises(ValueError):
        ac.update_(log_std=[0.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        make_ac(critic=False).update_(critic=critic)


def test_construction_errors():
    good = make_ac()
    actor, critic = good.actor, good.critic
    with pytest.raises(ValueError):
        GaussianActorCritic(actor, [0.0, 0.0, 0.0], critic)  # log_std of another length
    with pytest.raises(ValueError):
        GaussianActorCritic(actor, [0.0, np.inf], critic)
    two_out = MLPPolicy([np.zeros((2, 5))], [np.zeros(2)], out_map="none")
    with pytest.raises(ValueError):
        GaussianActorCritic(actor, [0.0, 0.0], two_out)  # a critic with n_out != 1
    clipped = MLPPolicy([np.zeros((1, 5))], [np.zeros(1)], out_map="clip")
    with pytest.raises(ValueError):
        GaussianActorCritic(actor, [0.0, 0.0], clipped)  # a critic with an output map
    other_in = MLPPolicy([np.zeros((1, 6))], [np.zeros(1)], out_map="none")
    with pytest.raises(ValueError):
        GaussianActorCritic(actor, [0.0, 0.0], other_in)
    squashed = MLPPolicy([np.zeros((2, 5))], [np.zeros(2)], out_map="tanh")
    with pytest.raises(ValueError, match="tanh"):
        GaussianActorCritic(squashed, [0.0, 0.0])
    with pytest.raises(ValueError):
        GaussianActorCritic(lambda o: o, [0.0])
    ac = GaussianActorCritic(actor, -0.3)  # a scalar log_std is broadcast
    assert ac.critic is None and np.array_equal(ac.log_std, [-0.3, -0.3])


def _gae_numpy(rew, val, gamma, lam, bootstrap_last):
    T, B = rew.shape
    adv = np.zeros((T, B))
    for b in range(B):
        last = 0.0
        for t in range(T - 1, -1, -1):
            nxt = val[t + 1, b] if (t < T - 1 or bootstrap_last) else 0.0
            delta = rew[t, b] + gamma * nxt - val[t, b]
            last = delta + gamma * lam * last
            adv[t, b] = last
    return adv, adv + val[:T]


@pytest.mark.parametrize("bootstrap_last", [False, True])
@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0)])
def test_gae_against_a_plain_backward_loop(gamma, lam, bootstrap_last):
    rng = np.random.default_rng(5)
    T, B = 23, 17
    rew, val = rng.standard_normal((T, B)), rng.standard_normal((T + 1, B))
    adv, ret = gae(torch.as_tensor(rew), torch.as_tensor(val), gamma, lam, bootstrap_last)
    a_ref, r_ref = _gae_numpy(rew, val, gamma, lam, bootstrap_last)
    assert adv.shape == (T, B) and ret.shape == (T, B)
    scale = max(1.0, float(np.max(np.abs(a_ref))))
    assert np.max(np.abs(adv.numpy() - a_ref)) <= 1e-13 * scale and np.max(np.abs(ret.numpy() - r_ref)) <= 1e-13 * scale
    if lam == 1.0 and gamma == 1.0:  # Monte-Carlo return: ret_t = sum of the later rewards (+ the bootstrap value)
        tail = np.cumsum(rew[::-1], axis=0)[::-1] + (val[T] if bootstrap_last else 0.0)
        assert np.allclose(ret.numpy(), tail, rtol=0, atol=1e-12)
    # the two settings differ exactly by the discounted bootstrap value
    other, _ = gae(torch.as_tensor(rew), torch.as_tensor(val), gamma, lam, not bootstrap_last)
    k = (gamma * lam) ** np.arange(T - 1, -1, -1)[:, None] * gamma * val[T][None, :]
    sign = 1.0 if bootstrap_last else -1.0
    assert np.allclose(adv.numpy() - other.numpy(), sign * k, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        gae(torch.as_tensor(rew), torch.as_tensor(val[:T]))


def test_header_constants_and_signatures():
    assert abi.PCG_ABI_VERSION == 16 and int(re.search(r"#define PCG_ABI_VERSION (\d+)", HDR).group(1)) == 16
    assert abi.PCG_RNG_POLICY == 0x400 == int(re.search(r"#define PCG_RNG_POLICY (\w+)", HDR).group(1), 0)
    lib = _lib.load()
    assert lib.pcg_version() == 16
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    ctype = {"pcg_plan*": vp, "const pcg_buffers*": C.POINTER(abi.pcg_buffers), "const pcg_policy*": vp, "pcg_policy*": vp,
             "const pcg_policy_cfg*": C.POINTER(abi.pcg_policy_cfg), "const double*": C.POINTER(C.c_double), "double*": vp,
             "void*": vp, "int32_t": i32, "int64_t": i64, "uint64_t": u64}
    for name, ret in (("pcg_rollout_actor", C.c_int), ("pcg_policy_noise", C.c_int), ("pcg_policy_update", C.c_int),
                      ("pcg_actor_logp_const", C.c_double)):
        assert name in abi.EXPORTS
        m = re.search(r"PCG_API (\w+) %s\((.*?)\);" % name, HDR, re.S)
        assert m, name
        assert {"int": C.c_int, "double": C.c_double}[m.group(1)] is ret is getattr(lib, name).restype
        params = [re.sub(r"/\*.*?\*/", "", p_).strip() for p_ in m.group(2).replace("\n", " ").split(",")]
        types = [ctype[re.sub(r"\s*\w+$", "", p_).strip()] for p_ in params]
        assert types == list(getattr(lib, name).argtypes), name
    # the record of recorded rows: four optional arrays, the last two without a component stride
    sig = re.search(r"pcg_rollout_actor\((.*?)\);", HDR, re.S).group(1)
    for word in ("a_seq_out", "u_seq_out", "logp_out", "value_out", "record_next_action", "sigma", "critic"):
        assert word in sig
    # pcg_policy_cfg keeps its layout
    assert [f[0] for f in abi.pcg_policy_cfg._fields_] == ["n_in", "n_out", "n_hidden", "width", "activation", "out_map",
                                                           "out_low", "out_high", "W", "b"]
    assert "immutable after creation" not in HDR


def test_host_side_validation_without_a_device():
    lib = _lib.load()
    pd = C.POINTER(C.c_double)
    sig = (C.c_double * 2)(0.5, 2.0)
    # no plan: refused before anything else is looked at
    assert lib.pcg_rollout_actor(None, None, None, None, sig, 0, 1, None, 0, 0, None, 0, 0, None, 0, None, 0, None, 0, 0, None, 0,
                                 0, 1, None) == abi.PCG_E_PLAN
    assert lib.pcg_policy_noise(None, 4, 0, 1, None, None) == abi.PCG_E_PLAN
    pol = MLPPolicy([np.zeros((1, 3))], [np.zeros(1)])
    cfg, keep = pol.to_cfg()
    assert lib.pcg_policy_update(None, C.byref(cfg)) == abi.PCG_E_NULL
    # the log-probability constant: the formula, and NaN for what pcg_rollout_actor refuses with PCG_E_VALUE
    half_log_2pi = float("0.918938533204672741780329736406")  # (the decimal expansion, correctly rounded by the parser)
    one = (C.c_double * 1)(1.0)
    assert lib.pcg_actor_logp_const(one, 1) == -half_log_2pi
    c0 = lib.pcg_actor_logp_const(sig, 2)  # log 0.5 + log 2 = 0 up to the two logs' rounding
    assert abs(c0 + 2 * half_log_2pi) <= 4 * 2.0 ** -53 * (2 * math.log(2.0) + 2 * half_log_2pi)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert math.isnan(lib.pcg_actor_logp_const((C.c_double * 2)(1.0, bad), 2))
    assert math.isnan(lib.pcg_actor_logp_const(None, 1)) and math.isnan(lib.pcg_actor_logp_const(sig, 0))
    assert math.isnan(lib.pcg_actor_logp_const(sig, abi.PCG_MAX_NA + 1))
    assert pd is not None
