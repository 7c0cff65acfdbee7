"""Declarative policies: a small fp64 multi-layer perceptron that the engine can evaluate INSIDE the rollout kernel.

The reference evaluates ``policy.predict(obs)`` on the host between two ``env.step`` calls
(src/pcgym/policy_evaluation.py:86-128); its policies are stable-baselines3 ``MlpPolicy`` networks: a few ``Linear``
layers with ``Tanh`` / ``ReLU`` between them.  :class:`MLPPolicy` states such a network as data --

    h1 = act(W[0] obs + b[0]);  h2 = act(W[1] h1 + b[1]);  a = out_map(W[-1] h + b[-1])

with 0, 1 or 2 hidden layers of at most 64 units (0 = affine state feedback ``a = W obs + b``) -- the way ``sp_track``
states a reward as data.  It is two things at once:

  * a callable ``obs (B, Nobs) -> (B, na)`` doing this arithmetic in torch fp64, on whatever device the observation lives
    on: it works wherever a policy callable works (``VecEnv.step`` loops, the per-step path of ``collect_rollouts``, CPU);
  * the description ``pcg_policy_create`` turns into a device object, so that ``collect_rollouts(env, policy=MLPPolicy)``
    and ``VecEnv.rollout_policy`` run the whole closed loop in ONE launch (``pcg_rollout_policy``, include/pcgym_hip.h).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi as abi
from . import _lib

_ACT = {"tanh": abi.PCG_ACT_TANH, "relu": abi.PCG_ACT_RELU}
_OUT = {"none": abi.PCG_POL_NONE, "clip": abi.PCG_POL_CLIP, "tanh": abi.PCG_POL_TANH}


def _torch():
    import torch

    return torch


class MLPPolicy:
    """weights[l] : (n_next, n_prev) array (``torch.nn.Linear.weight`` layout), biases[l] : (n_next,);
    activation : "tanh" | "relu" between layers; out_map : "none" | "clip" (to [out_low, out_high]) | "tanh"."""

    def __init__(self, weights, biases, activation="tanh", out_map="clip", out_low=-1.0, out_high=1.0):
        if activation not in _ACT:
            raise ValueError(f"activation must be one of {sorted(_ACT)}, not {activation!r}")
        if out_map not in _OUT:
            raise ValueError(f"out_map must be one of {sorted(_OUT)}, not {out_map!r}")
        self.weights = [np.ascontiguousarray(np.asarray(w, dtype=np.float64)) for w in weights]
        self.biases = [np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(-1)) for b in biases]
        if not self.weights or len(self.weights) != len(self.biases):
            raise ValueError("one bias vector per weight matrix, at least one layer")
        for l, (w, b) in enumerate(zip(self.weights, self.biases)):
            if w.ndim != 2 or b.shape != (w.shape[0],):
                raise ValueError(f"layer {l}: weight {w.shape} (n_next, n_prev) does not go with bias {b.shape}")
            if l and w.shape[1] != self.weights[l - 1].shape[0]:
                raise ValueError(f"layer {l}: {w.shape[1]} inputs after a layer of {self.weights[l - 1].shape[0]} units")
        self.activation, self.out_map = activation, out_map
        self.out_low, self.out_high = float(out_low), float(out_high)
        self.n_in, self.n_out = int(self.weights[0].shape[1]), int(self.weights[-1].shape[0])
        self.n_hidden = len(self.weights) - 1
        self._tensors = {}   # device -> ([W], [b]) torch tensors
        self._handles = {}   # device index -> pcg_policy*

    # ---- the callable: torch fp64 on the observation's device ----------------------------------------------------------
    def __call__(self, obs):
        torch = _torch()
        obs = torch.as_tensor(obs)
        key = str(obs.device)
        if key not in self._tensors:
            self._tensors[key] = ([torch.as_tensor(w, device=obs.device) for w in self.weights],
                                  [torch.as_tensor(b, device=obs.device) for b in self.biases])
        Ws, bs = self._tensors[key]
        h = obs.to(torch.float64)
        for l, (w, b) in enumerate(zip(Ws, bs)):
            h = torch.addmm(b, h, w.t())
            if l < self.n_hidden:
                h = torch.tanh(h) if self.activation == "tanh" else torch.relu(h)
        if self.out_map == "clip":
            h = torch.clamp(h, self.out_low, self.out_high)
        elif self.out_map == "tanh":
            h = torch.tanh(h)
        return h

    @classmethod
    def from_torch(cls, module, out_map=None, out_low=-1.0, out_high=1.0):
        """From an ``nn.Sequential`` of ``Linear`` layers with ``Tanh`` or ``ReLU`` between them (one kind).  A ``Tanh``
        after the last ``Linear`` becomes ``out_map="tanh"``; otherwise ``out_map`` defaults to "clip".  Anything else in
        the module raises ValueError."""
        nn = _torch().nn
        if not isinstance(module, nn.Sequential):
            raise ValueError(f"from_torch takes an nn.Sequential, not {type(module).__name__}")
        mods = list(module)
        weights, biases, acts, trailing = [], [], [], None
        expect_linear = True
        for i, m in enumerate(mods):
            if expect_linear:
                if not isinstance(m, nn.Linear):
                    raise ValueError(f"module {i}: expected Linear, found {type(m).__name__}")
                weights.append(m.weight.detach().cpu().double().numpy())
                biases.append(m.bias.detach().cpu().double().numpy() if m.bias is not None else np.zeros(m.out_features))
                expect_linear = False
            else:
                if not isinstance(m, (nn.Tanh, nn.ReLU)):
                    raise ValueError(f"module {i}: only Tanh / ReLU may follow a Linear, found {type(m).__name__}")
                name = "tanh" if isinstance(m, nn.Tanh) else "relu"
                if i == len(mods) - 1:
                    trailing = name
                else:
                    acts.append(name)
                expect_linear = True
        if not weights:
            raise ValueError("no Linear layer in the module")
        if len(set(acts)) > 1:
            raise ValueError(f"one activation kind per policy, found {sorted(set(acts))}")
        if trailing == "relu":
            raise ValueError("a ReLU after the last Linear is not an output map of this policy form")
        if trailing == "tanh":
            if out_map not in (None, "tanh"):
                raise ValueError(f"the module ends in Tanh: out_map={out_map!r} contradicts it")
            out_map = "tanh"
        return cls(weights, biases, activation=acts[0] if acts else "tanh", out_map=out_map or "clip",
                   out_low=out_low, out_high=out_high)

    # ---- the C ABI side ------------------------------------------------------------------------------------------------
    def to_cfg(self):
        """(pcg_policy_cfg, keep-alive list).  Built without checks: pcg_policy_validate is the judge of the contents."""
        cfg = abi.pcg_policy_cfg()
        cfg.n_in, cfg.n_out, cfg.n_hidden = self.n_in, self.n_out, self.n_hidden
        for l in range(min(self.n_hidden, 2)):
            cfg.width[l] = int(self.weights[l].shape[0])
        cfg.activation, cfg.out_map = _ACT[self.activation], _OUT[self.out_map]
        cfg.out_low, cfg.out_high = self.out_low, self.out_high
        pd = C.POINTER(C.c_double)
        for l in range(min(len(self.weights), 3)):
            cfg.W[l] = self.weights[l].ctypes.data_as(pd)
            cfg.b[l] = self.biases[l].ctypes.data_as(pd)
        return cfg, [self.weights, self.biases]

    def validate(self):
        """status of pcg_policy_validate (host only: no GPU needed); 0 = the engine can evaluate this policy on the device"""
        cfg, keep = self.to_cfg()
        return int(_lib.load().pcg_policy_validate(C.byref(cfg)))

    def handle(self, device):
        """the pcg_policy* of this policy on `device` (created at first use, kept until close())"""
        torch = _torch()
        device = torch.device(device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if idx not in self._handles:
            cfg, keep = self.to_cfg()
            h = C.c_void_p()
            with torch.cuda.device(idx):
                _lib.check(_lib.load().pcg_policy_create(C.byref(h), C.byref(cfg)), "pcg_policy_create")
            self._handles[idx] = h
        return self._handles[idx]

    def close(self):
        for h in self._handles.values():
            _lib.load().pcg_policy_destroy(h)
        self._handles = {}

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def fused_policy_ok(spec, policy):
    """the plans pcg_rollout_policy takes (include/pcgym_hip.h): fixed-step RK4 / CV8, no constraint rows, no per-env
    parameters, nothing run-time compiled -- and a policy of the plan's sizes that the device form can hold"""
    return (isinstance(policy, MLPPolicy) and spec.integrator in ("rk4", "cv8") and not spec.ncon and not spec.nunc
            and spec.user_rhs_src is None and not spec.user_reward_src and not spec.user_cons_src
            and policy.n_in == spec.nobs and policy.n_out == spec.na and policy.validate() == 0)
