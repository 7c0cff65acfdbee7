"""Declarative policies: a small fp64 (or, by choice, float32) multi-layer perceptron that the engine can evaluate INSIDE the rollout kernel.

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
_DTYPE = {"float64": np.float64, "float32": np.float32}


def _as(values, np_dtype, what):
    """contiguous array of `np_dtype`, rounded to nearest; a finite value that overflows float32 raises ValueError"""
    v64 = np.asarray(values, dtype=np.float64)
    if np_dtype is np.float64:
        return np.ascontiguousarray(v64) if v64.ndim else v64
    with np.errstate(over="ignore"):
        v = v64.astype(np.float32)
    v = np.ascontiguousarray(v) if v.ndim else v
    if np.any(np.isinf(v) & np.isfinite(v64)):
        raise ValueError(f"{what}: a value overflows float32")
    return v


def _torch():
    import torch

    return torch


class MLPPolicy:
    """weights[l] : (n_next, n_prev) array (``torch.nn.Linear.weight`` layout), biases[l] : (n_next,);
    activation : "tanh" | "relu" between layers; out_map : "none" | "clip" (to [out_low, out_high]) | "tanh".
    dtype : "float64" (default) | "float32".  Under "float32" weights, biases and the clip box are stored as ``np.float32``
    (rounded to nearest; an overflow raises ValueError), the callable computes in torch float32 on ``obs.to(float32)`` and
    returns float64 tensors (exact widening), and the device form is ``pcg_policy_create_f32``: the network is evaluated in
    float32 inside the kernel, as stable-baselines3 evaluates the module it trained."""

    def __init__(self, weights, biases, activation="tanh", out_map="clip", out_low=-1.0, out_high=1.0, dtype="float64"):
        if dtype not in _DTYPE:
            raise ValueError(f"dtype must be one of {sorted(_DTYPE)}, not {dtype!r}")
        self.dtype = dtype
        npd = _DTYPE[dtype]
        if activation not in _ACT:
            raise ValueError(f"activation must be one of {sorted(_ACT)}, not {activation!r}")
        if out_map not in _OUT:
            raise ValueError(f"out_map must be one of {sorted(_OUT)}, not {out_map!r}")
        self.weights = [_as(w, npd, "weights") for w in weights]
        self.biases = [_as(b, npd, "biases").reshape(-1) for b in biases]
        if not self.weights or len(self.weights) != len(self.biases):
            raise ValueError("one bias vector per weight matrix, at least one layer")
        for l, (w, b) in enumerate(zip(self.weights, self.biases)):
            if w.ndim != 2 or b.shape != (w.shape[0],):
                raise ValueError(f"layer {l}: weight {w.shape} (n_next, n_prev) does not go with bias {b.shape}")
            if l and w.shape[1] != self.weights[l - 1].shape[0]:
                raise ValueError(f"layer {l}: {w.shape[1]} inputs after a layer of {self.weights[l - 1].shape[0]} units")
        self.activation, self.out_map = activation, out_map
        self.out_low, self.out_high = float(_as(out_low, npd, "out_low")), float(_as(out_high, npd, "out_high"))
        self.n_in, self.n_out = int(self.weights[0].shape[1]), int(self.weights[-1].shape[0])
        self.n_hidden = len(self.weights) - 1
        self._tensors = {}   # device -> ([W], [b]) torch tensors
        self._handles = {}   # device index -> pcg_policy*

    # ---- the callable: torch fp64 on the observation's device ----------------------------------------------------------
    def raw(self, obs):
        """the last layer's output BEFORE the output map (the mean of a Gaussian actor, a critic's value)"""
        torch = _torch()
        obs = torch.as_tensor(obs)
        key = str(obs.device)
        if key not in self._tensors:
            self._tensors[key] = ([torch.as_tensor(w, device=obs.device) for w in self.weights],
                                  [torch.as_tensor(b, device=obs.device) for b in self.biases])
        Ws, bs = self._tensors[key]
        h = obs.to(torch.float32 if self.dtype == "float32" else torch.float64)
        for l, (w, b) in enumerate(zip(Ws, bs)):
            h = torch.addmm(b, h, w.t())
            if l < self.n_hidden:
                h = torch.tanh(h) if self.activation == "tanh" else torch.relu(h)
        return h.to(torch.float64)

    def map(self, h):
        """the output map alone: what turns ``raw(obs)`` into the policy's output"""
        torch = _torch()
        if self.out_map == "clip":
            h = torch.clamp(h, self.out_low, self.out_high)
        elif self.out_map == "tanh":
            # (a float32 policy's raw output is a float32 value: tanh in float32 before the widening, as in the kernel)
            h = torch.tanh(h.to(torch.float32)).to(torch.float64) if self.dtype == "float32" else torch.tanh(h)
        return h

    def __call__(self, obs):
        return self.map(self.raw(obs))

    def update_(self, weights, biases):
        """New weights of IDENTICAL shape, in place: the host arrays, the cached torch tensors and every live device handle
        (``pcg_policy_update``: the device block is rewritten, nothing is allocated or freed).  A shape change raises
        ValueError and leaves the policy as it was."""
        ws = [_as(w, _DTYPE[self.dtype], "weights") for w in weights]
        bs = [_as(b, _DTYPE[self.dtype], "biases").reshape(-1) for b in biases]
        if [w.shape for w in ws] != [w.shape for w in self.weights] or [b.shape for b in bs] != [b.shape for b in self.biases]:
            raise ValueError(f"update_ keeps the shape: {[w.shape for w in self.weights]}, not {[w.shape for w in ws]}")
        old = (self.weights, self.biases)
        self.weights, self.biases = ws, bs
        cfg, keep = self.to_cfg()
        rc = int(_lib.load().pcg_policy_validate(C.byref(cfg)))
        if rc != 0:
            self.weights, self.biases = old
            _lib.check(rc, "pcg_policy_validate")
        self._tensors = {}
        for h in self._handles.values():
            _lib.check(_lib.load().pcg_policy_update(h, C.byref(cfg)), "pcg_policy_update")
        return self

    @classmethod
    def from_torch(cls, module, out_map=None, out_low=-1.0, out_high=1.0, dtype=None):
        """From an ``nn.Sequential`` of ``Linear`` layers with ``Tanh`` or ``ReLU`` between them (one kind).  A ``Tanh``
        after the last ``Linear`` becomes ``out_map="tanh"``; otherwise ``out_map`` defaults to "clip".  Anything else in
        the module raises ValueError.  ``dtype=None``: a float64 policy (every parameter widened); ``dtype="float32"``: a
        float32 policy, which holds a float32 module's parameters bit for bit."""
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
                   out_low=out_low, out_high=out_high, dtype=dtype or "float64")

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
        # (pcg_policy_cfg carries doubles: a float32 policy passes exact widenings, which pcg_policy_create_f32 rounds back)
        ws, bs = self.weights, self.biases
        if self.dtype == "float32":
            ws, bs = [w.astype(np.float64) for w in ws], [b.astype(np.float64) for b in bs]
        for l in range(min(len(ws), 3)):
            cfg.W[l] = ws[l].ctypes.data_as(pd)
            cfg.b[l] = bs[l].ctypes.data_as(pd)
        return cfg, [ws, bs]

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
                create = "pcg_policy_create_f32" if self.dtype == "float32" else "pcg_policy_create"
                _lib.check(getattr(_lib.load(), create)(C.byref(h), C.byref(cfg)), create)
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
    """the plans pcg_rollout_policy takes (include/pcgym_hip.h): fixed-step RK4 / CV8, no constraint rows (a constraint
    expression is ``ncon`` rows too), no per-env parameters -- user models and reward expressions included, which run the
    kernel from their plan's own run-time compiled module -- and a policy of the plan's sizes that the device form can hold.
    A float32 policy qualifies on the built-in plans only: the run-time compiled module carries the float64 kernels alone,
    and ``collect_*`` step such a plan with the float32 callable instead."""
    return (isinstance(policy, MLPPolicy) and spec.integrator in ("rk4", "cv8") and not spec.ncon and not spec.nunc
            and policy.n_in == spec.nobs and policy.n_out == spec.na and policy.validate() == 0
            and not (policy.dtype == "float32" and _runtime_compiled(spec)))


def fused_cons_ok(spec, policy):
    """the plans pcg_rollout_policy_cons takes (include/pcgym_hip.h): those of pcg_rollout_policy WITH affine constraint rows,
    recorded per step -- fixed-step RK4 / CV8, no per-env parameters, built-in plans only (a user model, a reward or constraint
    expression runs from a module that carries the unconstrained kernels alone), a float64 policy of the plan's sizes"""
    return (isinstance(policy, MLPPolicy) and spec.integrator in ("rk4", "cv8") and bool(spec.ncon) and not spec.nunc
            and not _runtime_compiled(spec) and policy.dtype != "float32"
            and policy.n_in == spec.nobs and policy.n_out == spec.na and policy.validate() == 0)


def fused_unc_ok(spec, policy):
    """the plans pcg_rollout_policy_unc takes (include/pcgym_hip.h): per-env model parameters sampled at reset (``nunc``), RK4, no
    constraint rows, built-in plans only (per-env parameters are refused on run-time compiled ones when the spec is made), a
    float64 policy of the plan's sizes -- whose input counts the parameter slots of the observation.  The collectors take the
    call with ``fused_unc=True``; their default route on such a plan stays the per-step loop."""
    return (isinstance(policy, MLPPolicy) and spec.integrator == "rk4" and bool(spec.nunc) and not spec.ncon
            and not _runtime_compiled(spec) and policy.dtype != "float32"
            and policy.n_in == spec.nobs and policy.n_out == spec.na and policy.validate() == 0)


class PolicyPopulation:
    """P :class:`MLPPolicy` networks of ONE shape and dtype, each driving its own slice of a batch: what derivative-free
    policy search over the weights, the comparison of a set of checkpoints and hyper-parameter sweeps roll -- in ONE launch
    (``pcg_rollout_policy_pop``, ``VecEnv.rollout_population``) instead of P launches of a few workgroups.

    weights[l] : (P, n_next, n_prev) array, biases[l] : (P, n_next); activation, out_map and the clip box are shared.
    dtype : "float64" (default) | "float32", as :class:`MLPPolicy`'s: under "float32" weights, biases and the clip box are
    stored as ``np.float32`` (rounded to nearest; an overflow raises ValueError), the callable computes in torch float32 on
    ``obs.to(float32)`` and returns float64 tensors, and the device form is ``pcg_policy_pop_create_f32``: every member is
    evaluated in float32 inside the kernel, as stable-baselines3 evaluates the checkpoints it trained.
    Env ``e`` of a batch is driven by member ``(env_offset + e) // envs_per_policy`` (the global env index: a sharded batch
    splits a population the way it splits the random streams).

    The weights can also be written and read ON the device, in the flat parameter order of :meth:`flat_layout`
    (include/pcgym_hip.h, csrc/pcg_pop_search.hpp): :meth:`sample_` draws members of a diagonal Gaussian straight into the
    packed blocks, :meth:`noise_dot` forms an evolution strategy's score-weighted noise sum from the same keys,
    :meth:`flat` / :meth:`set_flat_` move flat parameter vectors out and in -- float64 tensors for either dtype: a float32
    population stores each value with one round-to-nearest conversion and hands it back widened exactly.  After a device-side write the host arrays
    ``weights`` / ``biases`` are stale for those members; everything that reads them (``member``, the callable, ``to_cfg``,
    ``update_``, ``close``) first brings them back with one :meth:`flat` and one copy.  A population never written from the
    device behaves as it always did."""

    def __init__(self, weights, biases, activation="tanh", out_map="clip", out_low=-1.0, out_high=1.0, dtype="float64"):
        if dtype not in _DTYPE:
            raise ValueError(f"dtype must be one of {sorted(_DTYPE)}, not {dtype!r}")
        self.dtype = dtype
        if activation not in _ACT:
            raise ValueError(f"activation must be one of {sorted(_ACT)}, not {activation!r}")
        if out_map not in _OUT:
            raise ValueError(f"out_map must be one of {sorted(_OUT)}, not {out_map!r}")
        self.weights, self.biases = self._arrays(weights, biases, _DTYPE[dtype])
        self.activation, self.out_map = activation, out_map
        self.out_low, self.out_high = float(_as(out_low, _DTYPE[dtype], "out_low")), float(_as(out_high, _DTYPE[dtype], "out_high"))
        self.P = int(self.weights[0].shape[0])
        self.n_in, self.n_out = int(self.weights[0].shape[2]), int(self.weights[-1].shape[1])
        self.n_hidden = len(self.weights) - 1
        self._tensors = {}   # device -> ([W], [b]) torch tensors
        self._handles = {}   # device index -> pcg_policy_pop*
        self._valid = None   # validate()'s status, once asked for
        self._stale = None   # (P,) bool: members whose host arrays are behind the device (None: never written from the device)
        self._stale_dev = None  # index of the device that holds them

    @staticmethod
    def _arrays(weights, biases, np_dtype=np.float64):
        """contiguous (P, n_next, n_prev) / (P, n_next) arrays of `np_dtype` (rounded to nearest; a float32 overflow raises) of
        one member count whose layers chain, or ValueError"""
        ws = [np.ascontiguousarray(_as(w, np_dtype, "weights")) for w in weights]
        bs = [np.ascontiguousarray(_as(b, np_dtype, "biases")) for b in biases]
        if not ws or len(ws) != len(bs):
            raise ValueError("one bias array per weight array, at least one layer")
        if ws[0].ndim != 3 or ws[0].shape[0] < 1:
            raise ValueError(f"layer 0: weights must be (P, n_next, n_prev) with P >= 1, not {ws[0].shape}")
        P = ws[0].shape[0]
        for l, (w, b) in enumerate(zip(ws, bs)):
            if w.ndim != 3 or w.shape[0] != P or b.shape != (P, w.shape[1]):
                raise ValueError(f"layer {l}: weights {w.shape} (P, n_next, n_prev) do not go with biases {b.shape} for P = {P}")
            if l and w.shape[2] != ws[l - 1].shape[1]:
                raise ValueError(f"layer {l}: {w.shape[2]} inputs after a layer of {ws[l - 1].shape[1]} units")
        return ws, bs

    @classmethod
    def from_policies(cls, policies):
        """From MLPPolicy objects of one dtype (all float64 or all float32), shape, activation, output map and clip box
        (ValueError otherwise); the population has the members' dtype"""
        policies = list(policies)
        if not policies:
            raise ValueError("from_policies needs at least one policy")
        p0 = policies[0]
        for p in policies:
            if not isinstance(p, MLPPolicy) or not isinstance(p0, MLPPolicy) or p.dtype != p0.dtype:
                raise ValueError("from_policies takes MLPPolicy objects of one dtype: all float64 or all float32")
            if ([w.shape for w in p.weights] != [w.shape for w in p0.weights]
                    or (p.activation, p.out_map, p.out_low, p.out_high) != (p0.activation, p0.out_map, p0.out_low, p0.out_high)):
                raise ValueError("the members of a population share shape, activation, output map and clip box")
        return cls([np.stack([p.weights[l] for p in policies]) for l in range(len(p0.weights))],
                   [np.stack([p.biases[l] for p in policies]) for l in range(len(p0.biases))],
                   activation=p0.activation, out_map=p0.out_map, out_low=p0.out_low, out_high=p0.out_high, dtype=p0.dtype)

    def member(self, i):
        """member ``i`` as an MLPPolicy of its own, of the population's dtype (copies of the weights)"""
        i = int(i)
        if not 0 <= i < self.P:
            raise ValueError(f"member {i} of a population of {self.P}")
        self._refresh()
        return MLPPolicy([w[i].copy() for w in self.weights], [b[i].copy() for b in self.biases], activation=self.activation,
                         out_map=self.out_map, out_low=self.out_low, out_high=self.out_high, dtype=self.dtype)

    # ---- the callable: torch fp64 (float32 for a float32 population) on the observation's device, each slice with its member
    def __call__(self, obs, envs_per_policy, env_offset=0):
        """obs (B, Nobs) -> (B, na): rows ``e`` with ``(env_offset + e) // envs_per_policy == m`` through member ``m``,
        in MLPPolicy's arithmetic: one ``addmm`` per layer and member present -- on CPU tensors the bits of the member's own
        ``MLPPolicy.__call__`` on its slice -- or, for whole slices on a GPU, one ``baddbmm`` per layer over all members.
        A float32 population computes in torch float32 on ``obs.to(float32)`` in both forms, applies a ``tanh`` output map in
        float32 and returns float64 tensors (exact widening)."""
        torch = _torch()
        obs = torch.as_tensor(obs)
        G, off, B = int(envs_per_policy), int(env_offset), int(obs.shape[0])
        if G < 1 or off < 0:
            raise ValueError(f"envs_per_policy must be positive and env_offset non-negative, not {G} / {off}")
        if B and (off + B - 1) // G >= self.P:
            raise ValueError(f"envs {off} .. {off + B - 1} in slices of {G} need {(off + B - 1) // G + 1} members, the population has {self.P}")
        self._refresh()
        key = str(obs.device)
        if key not in self._tensors:
            self._tensors[key] = ([torch.as_tensor(w, device=obs.device) for w in self.weights],
                                  [torch.as_tensor(b, device=obs.device) for b in self.biases])
        Ws, bs = self._tensors[key]
        f32 = self.dtype == "float32"
        tdt = torch.float32 if f32 else torch.float64

        def out_map(h):
            if self.out_map == "tanh":
                return torch.tanh(h).to(torch.float64)  # (in the network's dtype, before the widening: as in the kernel)
            h = h.to(torch.float64)
            return torch.clamp(h, self.out_low, self.out_high) if self.out_map == "clip" else h

        if obs.is_cuda and B and off % G == 0 and B % G == 0:
            # whole slices on a GPU: one batched product per layer over the members present
            m0, n = off // G, B // G
            h = obs.to(tdt).reshape(n, G, self.n_in)
            for l in range(self.n_hidden + 1):
                h = torch.baddbmm(bs[l][m0:m0 + n].unsqueeze(1), h, Ws[l][m0:m0 + n].transpose(1, 2))
                if l < self.n_hidden:
                    h = torch.tanh(h) if self.activation == "tanh" else torch.relu(h)
            return out_map(h.reshape(B, self.n_out))
        out = torch.empty((B, self.n_out), dtype=torch.float64, device=obs.device)
        e = 0
        while e < B:
            m = (off + e) // G
            e1 = min(B, (m + 1) * G - off)
            h = obs[e:e1].to(tdt)
            for l in range(self.n_hidden + 1):
                h = torch.addmm(bs[l][m], h, Ws[l][m].t())
                if l < self.n_hidden:
                    h = torch.tanh(h) if self.activation == "tanh" else torch.relu(h)
            out[e:e1] = out_map(h)
            e = e1
        return out

    def update_(self, weights, biases, first=0):
        """New weights for members ``first .. first + count - 1`` (``count`` = the arrays' leading size), in place: host
        arrays, cached torch tensors and every live device handle (``pcg_policy_pop_update``: the device blocks are
        rewritten, nothing is allocated or freed).  A float32 population rounds first.  Another shape, a range outside the
        population or a value that overflows float32 raises ValueError and leaves the population as it was, host and device."""
        self._refresh()
        ws, bs = self._arrays(weights, biases, _DTYPE[self.dtype])
        first, count = int(first), int(ws[0].shape[0])
        if ([w.shape[1:] for w in ws] != [w.shape[1:] for w in self.weights] or first < 0 or first + count > self.P):
            raise ValueError(f"update_ keeps the shape {[w.shape[1:] for w in self.weights]} and stays inside the {self.P} members: "
                             f"{[w.shape for w in ws]} at first = {first}")
        cfg, keep = self._cfg(ws, bs)
        lib = _lib.load()
        for m in range(count):  # (host only: the judge of the contents, before anything changes)
            one, keep1 = self._cfg([w[m:] for w in ws], [b[m:] for b in bs])
            _lib.check(lib.pcg_policy_validate(C.byref(one)), "pcg_policy_validate")
        for l in range(len(ws)):
            self.weights[l][first:first + count] = ws[l]
            self.biases[l][first:first + count] = bs[l]
        self._tensors = {}
        self._valid = 0 if self._valid == 0 else None  # (the new members were validated above)
        for h in self._handles.values():
            _lib.check(lib.pcg_policy_pop_update(h, C.byref(cfg), first, count), "pcg_policy_pop_update")
        return self

    # ---- the C ABI side ------------------------------------------------------------------------------------------------
    def _cfg(self, ws, bs):
        cfg = abi.pcg_policy_cfg()
        cfg.n_in, cfg.n_out, cfg.n_hidden = self.n_in, self.n_out, self.n_hidden
        for l in range(min(self.n_hidden, 2)):
            cfg.width[l] = int(ws[l].shape[1])
        cfg.activation, cfg.out_map = _ACT[self.activation], _OUT[self.out_map]
        cfg.out_low, cfg.out_high = self.out_low, self.out_high
        pd = C.POINTER(C.c_double)
        # (pcg_policy_cfg carries doubles: a float32 population passes exact widenings, which the float32 device form rounds back)
        ws = [np.ascontiguousarray(w, dtype=np.float64) for w in ws]
        bs = [np.ascontiguousarray(b, dtype=np.float64) for b in bs]
        for l in range(min(len(ws), 3)):
            cfg.W[l] = ws[l].ctypes.data_as(pd)
            cfg.b[l] = bs[l].ctypes.data_as(pd)
        return cfg, [ws, bs]

    def to_cfg(self):
        """(pcg_policy_cfg with member-major float64 arrays, keep-alive list): what ``pcg_policy_pop_create`` /
        ``pcg_policy_pop_create_f32`` take beside ``P``"""
        self._refresh()
        return self._cfg(self.weights, self.biases)

    def validate(self):
        """0 when the device form can hold every member (host only), else the first failing status of pcg_policy_validate.
        (A float32 population's host arrays are float32 values already: what is finite there fits the float32 device form.)
        Remembered: a device-side write keeps the shape, and the values it writes are not inspected (include/pcgym_hip.h says
        what a rollout does with a non-finite member), so it leaves a remembered 0 standing and a search loop reads nothing
        back between generations."""
        if self._valid is None:  # (remembered until update_: a search loop asks before every launch)
            self._refresh()
            lib = _lib.load()
            self._valid = 0
            for m in range(self.P):
                one, keep = self._cfg([w[m:] for w in self.weights], [b[m:] for b in self.biases])
                rc = int(lib.pcg_policy_validate(C.byref(one)))
                if rc != 0:
                    self._valid = rc
                    break
        return self._valid

    def handle(self, device):
        """the pcg_policy_pop* of this population on `device` (created at first use, kept until close())"""
        torch = _torch()
        device = torch.device(device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if idx not in self._handles:
            cfg, keep = self.to_cfg()
            h = C.c_void_p()
            with torch.cuda.device(idx):
                create = "pcg_policy_pop_create_f32" if self.dtype == "float32" else "pcg_policy_pop_create"
                _lib.check(getattr(_lib.load(), create)(C.byref(h), C.byref(cfg), self.P), create)
            self._handles[idx] = h
        return self._handles[idx]

    def close(self):
        self._refresh()  # (the device blocks go: what was written there comes back first)
        for h in self._handles.values():
            _lib.load().pcg_policy_pop_destroy(h)
        self._handles = {}

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    # ---- the weights on the device: flat parameter vectors, sampling, the noise sum ------------------------------------------
    @property
    def n_params(self):
        """parameters per member: sum over the layers of rows (cols + 1)"""
        return sum(int(w.shape[1]) * (int(w.shape[2]) + 1) for w in self.weights)

    def flat_layout(self):
        """[(name, l, start, stop, shape)] in flat parameter order: layer by layer ``("W", l, ...)`` with the matrix row-major
        (n_next, n_prev), then ``("b", l, ...)`` -- parameter ``j`` of :meth:`flat` is entry ``j - start`` of that array.
        Host only."""
        out, j = [], 0
        for l, w in enumerate(self.weights):
            rows, cols = int(w.shape[1]), int(w.shape[2])
            out.append(("W", l, j, j + rows * cols, (rows, cols)))
            j += rows * cols
            out.append(("b", l, j, j + rows, (rows,)))
            j += rows
        return out

    def _search_device(self, device=None, write=False):
        """index of the device the flat entry points work on: `device`, else the one with a live handle, else the current
        one.  A device-side write needs the population to live on no other device."""
        torch = _torch()
        if device is not None:
            device = torch.device(device)
            idx = device.index if device.index is not None else torch.cuda.current_device()
        elif self._stale_dev is not None and self._stale is not None and self._stale.any():
            idx = self._stale_dev
        elif len(self._handles) == 1:
            idx = next(iter(self._handles))
        elif not self._handles:
            idx = torch.cuda.current_device()
        else:
            idx = torch.cuda.current_device()
            if idx not in self._handles:
                raise ValueError(f"the population has handles on devices {sorted(self._handles)}: make one of them current")
        if write and any(d != idx for d in self._handles):
            raise ValueError(f"a population with live handles on devices {sorted(self._handles)} cannot be written from device {idx}: "
                             "a device-side write reaches one device (a sharded run is one process per device)")
        return idx

    def _as_device(self, values, idx, dtype, shape, what):
        """`values` as a tensor of `dtype` and `shape` on device `idx` (numpy arrays and lists are copied there)"""
        torch = _torch()
        dev = torch.device("cuda", idx)
        t = values if isinstance(values, torch.Tensor) else torch.as_tensor(np.asarray(values), device=dev)
        if not t.is_cuda or t.device.index != idx:
            raise ValueError(f"{what} lives on {t.device}, the population on {dev}")
        if t.dtype != dtype:
            raise ValueError(f"{what} must be {dtype}, not {t.dtype}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what} must have shape {tuple(shape)}, not {tuple(t.shape)}")
        return t

    def _range(self, first, count):
        first = int(first)
        count = self.P - first if count is None else int(count)
        if first < 0 or count < 1 or first + count > self.P:
            raise ValueError(f"members {first} .. {first + count - 1} of a population of {self.P}")
        return first, count

    def _written(self, idx, first, count):
        if self._stale is None:
            self._stale = np.zeros(self.P, dtype=bool)
        self._stale[first:first + count] = True
        self._stale_dev = idx
        self._tensors = {}

    def _flat(self, idx, members, first, count):
        """(count, n) tensor on device `idx` from the device blocks (no look at the host arrays)"""
        torch = _torch()
        n = self.n_params
        h = self._handles[idx]
        theta = torch.empty((count, n), dtype=torch.float64, device=torch.device("cuda", idx))
        with torch.cuda.device(idx):
            rc = _lib.load().pcg_policy_pop_get_flat(h, members.data_ptr() if members is not None else None, first, count,
                                                     theta.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "pcg_policy_pop_get_flat")
        return theta

    def _refresh(self):
        """bring the host arrays of the members written on the device back: one flat() and one copy"""
        if self._stale is None or not self._stale.any():
            return
        torch = _torch()
        idx = self._stale_dev
        which = np.flatnonzero(self._stale)
        if which.size == self.P:
            theta = self._flat(idx, None, 0, self.P)
        else:
            members = torch.as_tensor(which.astype(np.int32), device=torch.device("cuda", idx))
            theta = self._flat(idx, members, 0, int(which.size))
        theta = theta.cpu().numpy()
        for name, l, a, b, shape in self.flat_layout():
            # (a float32 population's flat() holds float32 values: the assignment narrows them exactly)
            (self.weights if name == "W" else self.biases)[l][which] = theta[:, a:b].reshape((-1,) + shape)
        self._stale[:] = False
        self._tensors = {}

    def sample_(self, mean, std, seed, generation=0, antithetic=False, first=0, count=None, device=None, check=True):
        """Members ``first .. first + count - 1`` drawn from the diagonal Gaussian N(mean, diag(std^2)) straight into the packed
        device blocks (``pcg_policy_pop_sample``): ``theta[m, j] = mean[j] + std[j] * z(m, j)`` with the search noise of the
        RNG contract (keyed by ``seed``, ``generation``, the member and the parameter), ``antithetic``: members
        ``2q`` and ``2q + 1`` get ``+z`` and ``-z``.  Nothing crosses to the host and no other member is touched.  A float32
        population forms the same float64 sum and stores it with one round-to-nearest conversion: bit for bit ``float32`` of
        what a float64 population holds under the same arguments (an overflow is stored as an infinity, not inspected).

        mean, std : float64 tensors of shape ``(n_params,)`` on the population's device (numpy arrays are copied there).
        check     : True costs one reduction and one synchronisation and raises ValueError unless ``mean`` is finite and
                    ``std`` finite and >= 0; False reads nothing back (what a captured or pipelined loop wants)."""
        torch = _torch()
        idx = self._search_device(device, write=True)
        first, count = self._range(first, count)
        n = self.n_params
        mean = self._as_device(mean, idx, torch.float64, (n,), "mean").contiguous()
        std = self._as_device(std, idx, torch.float64, (n,), "std").contiguous()
        if check and not bool(torch.isfinite(mean).all() & torch.isfinite(std).all() & (std >= 0).all()):
            raise ValueError("sample_ needs a finite mean and a finite, non-negative std")
        if self.validate() != 0:
            raise ValueError(f"the device form cannot hold this population (pcg_policy_validate: {self.validate()})")
        h = self.handle(torch.device("cuda", idx))
        with torch.cuda.device(idx):
            rc = _lib.load().pcg_policy_pop_sample(h, first, count, mean.data_ptr(), std.data_ptr(), int(bool(antithetic)),
                                                   int(seed) & 0xFFFFFFFFFFFFFFFF, int(generation) & 0xFFFFFFFF,
                                                   torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "pcg_policy_pop_sample")
        self._written(idx, first, count)
        return self

    def noise_dot(self, weights, seed, generation=0, antithetic=False, first=0):
        """``out[j] = sum_i weights[i] * z(first + i, j)``: an evolution strategy's score-weighted noise sum over the members
        ``first .. first + len(weights) - 1``, formed from the keys :meth:`sample_` drew with -- the noise is never stored
        (``pcg_policy_pop_noise_dot``: a fixed summation order in chunks of 64 members, the same bits for every launch).
        weights : (count,) float64 tensor on the population's device (numpy arrays are copied).  Returns an ``(n_params,)``
        device tensor; the workspace is allocated by torch here.  The blocks are not read: on a float32 population a member's
        realised perturbation is ``round32(mean + std z) - mean``, the sum uses the unrounded ``z`` (ordinary ES noise)."""
        torch = _torch()
        idx = self._search_device()
        w = self._as_device(weights, idx, torch.float64, None, "weights")
        if w.dim() != 1:
            raise ValueError(f"weights must be one-dimensional, not {tuple(w.shape)}")
        w = w.contiguous()
        first, count = self._range(first, int(w.shape[0]) if w.shape[0] else 0)
        n = self.n_params
        dev = torch.device("cuda", idx)
        chunks = (count + abi.PCG_POP_CHUNK - 1) // abi.PCG_POP_CHUNK
        partial = torch.empty((chunks, n), dtype=torch.float64, device=dev)
        out = torch.empty(n, dtype=torch.float64, device=dev)
        h = self.handle(dev)
        with torch.cuda.device(idx):
            rc = _lib.load().pcg_policy_pop_noise_dot(h, first, count, int(bool(antithetic)), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                      int(generation) & 0xFFFFFFFF, w.data_ptr(), partial.data_ptr(),
                                                      out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "pcg_policy_pop_noise_dot")
        return out

    def flat(self, members=None, first=0, count=None):
        """(count, n_params) float64 device tensor of flat parameter vectors (:meth:`flat_layout`'s order), read from the
        packed device blocks (``pcg_policy_pop_get_flat``): members ``first .. first + count - 1``, or the rows ``members``
        names (a sequence or an int32 / int64 tensor; repeats allowed; an index outside ``[0, P)`` gives a row of NaN).  A
        float32 population's rows hold its float32 values exactly."""
        torch = _torch()
        idx = self._search_device()
        dev = torch.device("cuda", idx)
        self.handle(dev)
        if members is None:
            first, count = self._range(first, count)
            return self._flat(idx, None, first, count)
        m = members if isinstance(members, torch.Tensor) else torch.as_tensor(np.asarray(members, dtype=np.int64))
        if m.dim() != 1 or m.shape[0] < 1 or m.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"members must be a non-empty one-dimensional integer sequence, not {tuple(m.shape)} of {m.dtype}")
        if m.dtype == torch.int64:  # (an index that does not fit 32 bits is outside every population: it stays outside)
            m = m.clamp(-1, 2 ** 31 - 1)
        m = m.to(device=dev, dtype=torch.int32).contiguous()
        return self._flat(idx, m, 0, int(m.shape[0]))

    def set_flat_(self, theta, first=0):
        """Members ``first .. first + count - 1`` from the rows of ``theta`` (count, n_params), float64 on the population's
        device (numpy arrays are copied there): the device-to-device form of :meth:`update_` (``pcg_policy_pop_set_flat``).
        The values are not inspected; a float32 population stores ``float32(theta)``, rounded to nearest."""
        torch = _torch()
        idx = self._search_device(write=True)
        t = self._as_device(theta, idx, torch.float64, None, "theta")
        n = self.n_params
        if t.dim() != 2 or t.shape[1] != n:
            raise ValueError(f"theta must be (count, {n}), not {tuple(t.shape)}")
        first, count = self._range(first, int(t.shape[0]) if t.shape[0] else 0)
        if t.stride(1) != 1 or (count > 1 and t.stride(0) < n):
            t = t.contiguous()
        if self.validate() != 0:
            raise ValueError(f"the device form cannot hold this population (pcg_policy_validate: {self.validate()})")
        h = self.handle(torch.device("cuda", idx))
        with torch.cuda.device(idx):
            rc = _lib.load().pcg_policy_pop_set_flat(h, first, count, t.data_ptr(), t.stride(0) if count > 1 else n,
                                                     torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "pcg_policy_pop_set_flat")
        self._written(idx, first, count)
        return self


def fused_pop_ok(spec, pop, envs_per_policy):
    """the plans, populations and slices pcg_rollout_policy_pop takes (include/pcgym_hip.h): a built-in plan (no user model,
    no reward or constraint expression: the run-time compiled module does not carry the population kernel), fixed-step
    RK4 / CV8, no constraint rows, no per-env parameters; members of the plan's sizes that the device form can hold, float64
    or float32; slices of whole waves (a multiple of 64 envs)"""
    G = int(envs_per_policy)
    return (isinstance(pop, PolicyPopulation) and spec.integrator in ("rk4", "cv8") and not spec.ncon and not spec.nunc
            and not _runtime_compiled(spec) and G >= 64 and G % 64 == 0
            and pop.n_in == spec.nobs and pop.n_out == spec.na and pop.validate() == 0)


def fused_pop_unc_ok(spec, pop, envs_per_policy):
    """the plans, populations and slices pcg_rollout_policy_pop_unc takes (include/pcgym_hip.h): those of
    pcg_rollout_policy_unc -- per-env model parameters sampled at reset (``nunc``), RK4, no constraint rows, built-in plans
    only -- with fused_pop_ok's populations and slices: members of the plan's sizes, whose input counts the parameter slots of
    the observation, float64 or float32; slices of whole waves.  ``evaluate_population`` takes the call with
    ``fused_unc=True``; its default route on such a plan stays the per-step loop."""
    G = int(envs_per_policy)
    return (isinstance(pop, PolicyPopulation) and spec.integrator == "rk4" and bool(spec.nunc) and not spec.ncon
            and not _runtime_compiled(spec) and G >= 64 and G % 64 == 0
            and pop.n_in == spec.nobs and pop.n_out == spec.na and pop.validate() == 0)


def fused_pop_cons_ok(spec, pop, envs_per_policy):
    """the plans, populations and slices pcg_rollout_policy_pop_cons takes (include/pcgym_hip.h): those of
    pcg_rollout_policy_cons -- affine constraint rows (``ncon``), RK4 / CV8, no per-env parameters, built-in plans only (a
    constraint expression is run-time compiled: refused) -- with fused_pop_ok's populations and slices: members of the plan's
    sizes, float64 or float32; slices of whole waves.  ``evaluate_population`` takes the call by default on such a plan."""
    G = int(envs_per_policy)
    return (isinstance(pop, PolicyPopulation) and spec.integrator in ("rk4", "cv8") and bool(spec.ncon) and not spec.nunc
            and not _runtime_compiled(spec) and G >= 64 and G % 64 == 0
            and pop.n_in == spec.nobs and pop.n_out == spec.na and pop.validate() == 0)


def _runtime_compiled(spec):
    """whether the plan of `spec` runs from a run-time compiled module (a user model, a reward or constraint expression)"""
    return bool(spec.user_rhs_src is not None or spec.user_reward_src or spec.user_cons_src)


def _module_arrays(module):
    """(weights, biases) of an ``nn.Sequential`` through MLPPolicy.from_torch's reading of it"""
    pol = MLPPolicy.from_torch(module, out_map="none")
    return pol.weights, pol.biases


class GaussianActorCritic:
    """stable-baselines3's ``MlpPolicy`` as data: a Gaussian actor with a state-independent ``log_std`` plus an optional
    separate value network -- what ``pcg_rollout_actor`` evaluates inside the rollout kernel (include/pcgym_hip.h).

    actor   : :class:`MLPPolicy` whose ``raw`` output is the mean ``mu``; its output map ("none" | "clip") turns the sample
              ``u = mu + sigma z`` into the action the env applies.  "tanh" is refused: a squashed Gaussian's density needs
              the map's Jacobian.
    log_std : (na,) array (a scalar is broadcast).  ``sigma = exp(log_std)``; ``logp_const`` = -(sum log sigma + na/2 log 2 pi)
              is read from the library (``pcg_actor_logp_const``), so that it is the kernel's own constant bit for bit.
    critic  : :class:`MLPPolicy` with ``n_out == 1``, ``out_map="none"`` and the actor's ``n_in``, or None.

    ``log_prob`` is the log-density of the UNMAPPED sample ``u`` under N(mu, sigma^2) -- stable-baselines3 PPO's meaning: the
    env clips, the buffer keeps ``u``.  The torch methods work in fp64 on the observation's device (CPU included), with the
    kernel's formulas and summation order (components ascending).  With float32 networks (actor and critic of one dtype)
    ``mean`` and ``value`` are the widened float32 results; ``sample``, ``log_prob`` and ``log_prob_z`` stay fp64."""

    def __init__(self, actor, log_std, critic=None):
        if not isinstance(actor, MLPPolicy):
            raise ValueError(f"actor must be an MLPPolicy, not {type(actor).__name__}")
        if actor.out_map == "tanh":
            raise ValueError("a tanh output map makes a squashed Gaussian, whose log-probability needs the map's Jacobian: "
                             "use out_map='none' or 'clip'")
        if critic is not None:
            if not isinstance(critic, MLPPolicy):
                raise ValueError(f"critic must be an MLPPolicy, not {type(critic).__name__}")
            if critic.n_out != 1 or critic.out_map != "none":
                raise ValueError(f"the critic has one output and no output map (n_out={critic.n_out}, out_map={critic.out_map!r})")
            if critic.n_in != actor.n_in:
                raise ValueError(f"the critic reads {critic.n_in} inputs, the actor {actor.n_in}")
            if critic.dtype != actor.dtype:
                raise ValueError(f"actor and critic must have one dtype ({actor.dtype} / {critic.dtype}): one kernel evaluates both")
        self.actor, self.critic = actor, critic
        self.n_in, self.n_out = actor.n_in, actor.n_out
        self._set_log_std(log_std)

    def _set_log_std(self, log_std):
        if hasattr(log_std, "detach"):
            log_std = log_std.detach().cpu().double().numpy()
        ls = np.asarray(log_std, dtype=np.float64)
        if ls.ndim == 0:
            ls = np.full(self.n_out, float(ls))
        ls = np.ascontiguousarray(ls.reshape(-1))
        if ls.shape != (self.n_out,):
            raise ValueError(f"log_std has {ls.size} entries, the actor {self.n_out} outputs")
        sigma = np.exp(ls)
        if not (np.isfinite(sigma).all() and (sigma > 0).all()):
            raise ValueError("exp(log_std) must be finite and positive")
        c0 = float(_lib.load().pcg_actor_logp_const(sigma.ctypes.data_as(C.POINTER(C.c_double)), self.n_out))
        if not np.isfinite(c0):
            raise ValueError(f"no log-probability constant for sigma = {sigma} ({self.n_out} outputs)")
        self.log_std, self.sigma, self.logp_const = ls, sigma, c0
        self._sig_t = {}

    def _sigma_on(self, device):
        key = str(device)
        if key not in self._sig_t:
            self._sig_t[key] = _torch().as_tensor(self.sigma, device=device)
        return self._sig_t[key]

    # ---- torch fp64, any device ------------------------------------------------------------------------------------------
    def mean(self, obs):
        """mu (B, na)"""
        return self.actor.raw(obs)

    def sample(self, obs, z):
        """u = mu + sigma z (B, na) for standard normals z (B, na)"""
        mu = self.mean(obs)
        return _torch().addcmul(mu, self._sigma_on(mu.device), z.to(mu.dtype))

    def action(self, u):
        """the action the env applies for the sample u: the actor's output map"""
        return self.actor.map(u)

    def log_prob(self, obs, u):
        """log N(u; mu(obs), sigma^2), (B,): c0 - q / 2 with q the sum of the squared standardised residuals, ascending"""
        mu = self.mean(obs)
        z = (_torch().as_tensor(u, device=mu.device).to(mu.dtype) - mu) / self._sigma_on(mu.device)
        return self.log_prob_z(z)

    def log_prob_z(self, z):
        """the same from the standard normals themselves (B, na) -> (B,): the kernel's statement, fma(-0.5, q, c0)"""
        q = z[:, 0] * z[:, 0]
        for i in range(1, self.n_out):
            q = q + z[:, i] * z[:, i]
        return self.logp_const - 0.5 * q

    def value(self, obs):
        """critic(obs) (B,)"""
        if self.critic is None:
            raise ValueError("this actor-critic has no critic")
        return self.critic.raw(obs)[:, 0]

    @classmethod
    def from_torch(cls, actor_seq, log_std, critic_seq=None, out_map=None, out_low=-1.0, out_high=1.0, dtype=None):
        """From the ``nn.Sequential`` of the actor (MLPPolicy.from_torch's forms; ``out_map`` defaults to "clip"), its
        ``log_std`` (tensor, Parameter or array) and, optionally, the ``nn.Sequential`` of the value network; ``dtype`` as in
        MLPPolicy.from_torch, for both networks."""
        actor = MLPPolicy.from_torch(actor_seq, out_map=out_map, out_low=out_low, out_high=out_high, dtype=dtype)
        critic = MLPPolicy.from_torch(critic_seq, out_map="none", dtype=dtype) if critic_seq is not None else None
        return cls(actor, log_std, critic)

    def update_(self, actor=None, log_std=None, critic=None):
        """Refresh after an optimiser step, in place: ``actor`` / ``critic`` are ``nn.Sequential`` modules or
        ``(weights, biases)`` pairs of the SAME shapes, ``log_std`` as in the constructor.  Host arrays and every live device
        handle follow (``pcg_policy_update``: no device allocation); a shape change raises ValueError."""
        for pol, new in ((self.actor, actor), (self.critic, critic)):
            if new is None:
                continue
            if pol is None:
                raise ValueError("this actor-critic has no critic to update")
            w, b = new if isinstance(new, (tuple, list)) else _module_arrays(new)
            pol.update_(w, b)
        if log_std is not None:
            self._set_log_std(log_std)
        return self

    def close(self):
        self.actor.close()
        if self.critic is not None:
            self.critic.close()


def fused_actor_ok(spec, ac):
    """the plans and networks pcg_rollout_actor takes: those of pcg_rollout_policy for the actor, no tanh map, and a critic
    (if any) of the plan's observation size that the device form can hold"""
    return (isinstance(ac, GaussianActorCritic) and fused_policy_ok(spec, ac.actor) and ac.actor.out_map != "tanh"
            and (ac.critic is None or (ac.critic.n_in == spec.nobs and ac.critic.validate() == 0)))


def fused_actor_cons_ok(spec, ac):
    """the plans and networks pcg_rollout_actor_cons takes: those of pcg_rollout_policy_cons for the actor, no tanh map, and a
    float64 critic (if any) of the plan's observation size that the device form can hold"""
    return (isinstance(ac, GaussianActorCritic) and fused_cons_ok(spec, ac.actor) and ac.actor.out_map != "tanh"
            and (ac.critic is None or (ac.critic.n_in == spec.nobs and ac.critic.dtype != "float32" and ac.critic.validate() == 0)))


def fused_actor_unc_ok(spec, ac):
    """the plans and networks pcg_rollout_actor_unc takes: those of pcg_rollout_policy_unc for the actor, no tanh map, and a
    float64 critic (if any) of the plan's observation size that the device form can hold"""
    return (isinstance(ac, GaussianActorCritic) and fused_unc_ok(spec, ac.actor) and ac.actor.out_map != "tanh"
            and (ac.critic is None or (ac.critic.n_in == spec.nobs and ac.critic.dtype != "float32" and ac.critic.validate() == 0)))
