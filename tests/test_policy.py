"""CPU: the declarative MLP policy -- host-side validation of the C ABI (pcg_policy_validate), the torch evaluation of
MLPPolicy against a plain numpy evaluation, and from_torch.

Protects the policy half of the reference's closed loop, policy.predict(obs) between two env.step calls
(policy_evaluation.py:86-128), in the form the fused closed-loop rollout evaluates on the device (pcg_rollout_policy).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from pcgym_amd import MLPPolicy
from pcgym_amd import _abi as abi
from pcgym_amd import _lib


def make_policy(n_in, n_out, hidden, seed=0, scale=1.0, **kw):
    rng = np.random.default_rng(seed)
    dims = [n_in, *hidden, n_out]
    Ws = [scale * rng.standard_normal((dims[l + 1], dims[l])) / np.sqrt(dims[l]) for l in range(len(dims) - 1)]
    bs = [0.1 * rng.standard_normal(dims[l + 1]) for l in range(len(dims) - 1)]
    return MLPPolicy(Ws, bs, **kw)


def numpy_eval(pol, obs):
    h = np.asarray(obs, dtype=np.float64)
    for l, (w, b) in enumerate(zip(pol.weights, pol.biases)):
        h = h @ w.T + b
        if l < pol.n_hidden:
            h = np.tanh(h) if pol.activation == "tanh" else np.maximum(h, 0.0)
    if pol.out_map == "clip":
        h = np.clip(h, pol.out_low, pol.out_high)
    elif pol.out_map == "tanh":
        h = np.tanh(h)
    return h


@pytest.mark.parametrize("hidden", [(), (16,), (64, 64), (1,), (7, 3)])
def test_validate_accepts_good_configurations(hidden):
    assert make_policy(3, 1, hidden).validate() == abi.PCG_OK
    assert make_policy(abi.PCG_MAX_NOBS, abi.PCG_MAX_NA, hidden, activation="relu", out_map="tanh").validate() == abi.PCG_OK


def test_validate_rejects_bad_configurations():
    lib = _lib.load()
    assert lib.pcg_policy_validate(None) == abi.PCG_E_NULL
    # width 0 and 65 (the matrices cannot be built for width 0: set the field)
    for w in (0, 65):
        cfg, keep = make_policy(3, 1, (16,)).to_cfg()
        cfg.width[0] = w
        assert lib.pcg_policy_validate(C.byref(cfg)) == abi.PCG_E_DIM, w
    assert make_policy(3, 1, (65,)).validate() == abi.PCG_E_DIM
    assert make_policy(3, 1, (16, 65)).validate() == abi.PCG_E_DIM
    # three hidden layers
    assert make_policy(3, 1, (8, 8, 8)).validate() == abi.PCG_E_DIM
    cfg, keep = make_policy(3, 1, (8, 8)).to_cfg()
    cfg.n_hidden = 3
    assert lib.pcg_policy_validate(C.byref(cfg)) == abi.PCG_E_DIM
    cfg.n_hidden = -1
    assert lib.pcg_policy_validate(C.byref(cfg)) == abi.PCG_E_DIM
    # sizes no plan can have
    assert make_policy(abi.PCG_MAX_NOBS + 1, 1, ()).validate() == abi.PCG_E_DIM
    assert make_policy(3, abi.PCG_MAX_NA + 1, ()).validate() == abi.PCG_E_DIM
    # NULL weights / biases, of a layer that is used
    for field, l in (("W", 0), ("W", 1), ("b", 0), ("b", 1)):
        cfg, keep = make_policy(3, 1, (16,)).to_cfg()
        getattr(cfg, field)[l] = None
        assert lib.pcg_policy_validate(C.byref(cfg)) == abi.PCG_E_NULL, (field, l)
    # an empty clip box; the bounds do not matter under the other maps
    assert make_policy(3, 1, (16,), out_low=1.0, out_high=-1.0).validate() == abi.PCG_E_VALUE
    assert make_policy(3, 1, (16,), out_map="none", out_low=1.0, out_high=-1.0).validate() == abi.PCG_OK
    assert make_policy(3, 1, (16,), out_low=0.5, out_high=0.5).validate() == abi.PCG_OK
    # unknown activation / output map, a weight that is not finite
    for field in ("activation", "out_map"):
        cfg, keep = make_policy(3, 1, (16,)).to_cfg()
        setattr(cfg, field, 7)
        assert lib.pcg_policy_validate(C.byref(cfg)) == abi.PCG_E_VALUE, field
    pol = make_policy(3, 1, (16,))
    pol.weights[1][0, 3] = np.nan
    assert pol.validate() == abi.PCG_E_VALUE


def test_constructor_refuses_inconsistent_shapes():
    with pytest.raises(ValueError):
        MLPPolicy([np.zeros((4, 3)), np.zeros((1, 5))], [np.zeros(4), np.zeros(1)])
    with pytest.raises(ValueError):
        MLPPolicy([np.zeros((4, 3))], [np.zeros(3)])
    with pytest.raises(ValueError):
        MLPPolicy([np.zeros((1, 3))], [np.zeros(1)], activation="gelu")
    with pytest.raises(ValueError):
        MLPPolicy([np.zeros((1, 3))], [np.zeros(1)], out_map="softmax")


@pytest.mark.parametrize("hidden,act,om", [((), "tanh", "clip"), ((16,), "tanh", "clip"), ((64, 64), "tanh", "clip"),
                                           ((16,), "relu", "none"), ((5, 9), "relu", "tanh")])
def test_torch_evaluation_matches_numpy(hidden, act, om):
    pol = make_policy(5, 2, hidden, seed=3, activation=act, out_map=om, out_low=-0.4, out_high=0.6)
    obs = np.random.default_rng(1).uniform(-1.5, 1.5, (257, 5))
    got = pol(torch.as_tensor(obs))
    assert got.shape == (257, 2) and got.dtype == torch.float64
    ref = numpy_eval(pol, obs)
    # same fp64 arithmetic up to summation order: a few ulp of the largest partial sum
    assert np.max(np.abs(got.numpy() - ref)) <= 1e-13
    if om == "clip":
        inside = np.mean((ref > -0.4) & (ref < 0.6))
        assert 0.05 < inside < 1.0  # the box cuts some outputs and not all: both branches of the map are compared


def test_from_torch_round_trips():
    nn = torch.nn
    torch.manual_seed(0)
    seq = nn.Sequential(nn.Linear(4, 16), nn.Tanh(), nn.Linear(16, 8), nn.Tanh(), nn.Linear(8, 2)).double()
    pol = MLPPolicy.from_torch(seq, out_map="none")
    assert (pol.n_in, pol.n_out, pol.n_hidden, pol.activation, pol.out_map) == (4, 2, 2, "tanh", "none")
    assert pol.validate() == abi.PCG_OK
    obs = torch.randn(33, 4, dtype=torch.float64)
    with torch.no_grad():
        ref = seq(obs)
    assert torch.max(torch.abs(pol(obs) - ref)).item() <= 1e-14
    # ReLU, a Linear without bias, a trailing Tanh as the output map, the default clip map
    seq = nn.Sequential(nn.Linear(3, 5, bias=False), nn.ReLU(), nn.Linear(5, 1), nn.Tanh()).double()
    pol = MLPPolicy.from_torch(seq)
    assert (pol.activation, pol.out_map) == ("relu", "tanh") and not pol.biases[0].any()
    obs = torch.randn(9, 3, dtype=torch.float64)
    with torch.no_grad():
        assert torch.max(torch.abs(pol(obs) - seq(obs))).item() <= 1e-14
    lin = nn.Sequential(nn.Linear(3, 1)).double()
    pol = MLPPolicy.from_torch(lin, out_low=-0.5, out_high=0.5)
    assert (pol.n_hidden, pol.out_map, pol.out_low, pol.out_high) == (0, "clip", -0.5, 0.5)
    with torch.no_grad():
        assert torch.max(torch.abs(pol(obs) - torch.clamp(lin(obs), -0.5, 0.5))).item() <= 1e-14
    # float32 modules are taken as their fp64 values
    pol = MLPPolicy.from_torch(nn.Sequential(nn.Linear(3, 4), nn.Tanh(), nn.Linear(4, 1)))
    assert pol.weights[0].dtype == np.float64


def test_from_torch_refuses_unsupported_modules():
    nn = torch.nn
    bad = [
        nn.Sequential(nn.Linear(3, 4), nn.Sigmoid(), nn.Linear(4, 1)),
        nn.Sequential(nn.Linear(3, 4), nn.Tanh(), nn.Dropout(0.1), nn.Linear(4, 1)),
        nn.Sequential(nn.Linear(3, 4), nn.Linear(4, 1)),
        nn.Sequential(nn.Tanh(), nn.Linear(3, 1)),
        nn.Sequential(nn.Linear(3, 4), nn.Tanh(), nn.Linear(4, 4), nn.ReLU(), nn.Linear(4, 1)),
        nn.Sequential(nn.Linear(3, 4), nn.ReLU()),
        nn.Sequential(),
        nn.Linear(3, 1),
    ]
    for m in bad:
        with pytest.raises(ValueError):
            MLPPolicy.from_torch(m)
    with pytest.raises(ValueError):
        MLPPolicy.from_torch(nn.Sequential(nn.Linear(3, 1), nn.Tanh()), out_map="clip")
