"""env_params dict -> numeric environment specification.

Mirrors the parsing done by the reference ``make_env.__init__`` and its
``_setup_*`` helpers (pcgym.py:32-253): same keys, same defaults, same
``ValueError`` sites.  The result (``EnvSpec``) is the host-side image of
``pcg_env_cfg`` (include/pcgym_hip.h); ``EnvSpec.to_cfg()`` marshals it for the
C ABI.  Nothing numeric about the hot path happens here.

``EnvSpec.__init__`` is an ordered list of stages, each parsing one group of keys into one group of fields: flags and
spaces, reward kind, grid, model (``adopt_custom_model``), set-points, disturbances, a_delta, noise and partial
observation, uncertainty, constraints, reward boxes, ``integrator_plan`` (a function of plain values), user sources.
Every field is assigned once, before anything reads it; what else a later stage needs is passed to it.

New optional keys (do not exist in the reference):
  integrator   'rk4' | 'cv8' (fixed-step order 8) | 'rk4g' / 'tsit5g' (guarded fixed step with adaptive fallback, cstr) |
               'dopri5' | 'tsit5' | 'rodas3' | 'rodas4' | 'rodas5' (stiff-capable Rosenbrock pairs; 'rodas5' is the
               multistage_extraction default: rtol = atol = 8e-8 / max(1, dt), halved for eq_exponent != 2)
               (default per model, see DEFAULT_INTEGRATOR; integration_method='jax' -> 'tsit5', the reference's own
               method, integrator.py:56-61)
  endpoint_control  rodas4 / rodas5: {'frac': 0.5, 'kmax': 10 | 16} | False -- end-point error control (pcgym_hip.h,
               PCG_INT_RODAS4 / PCG_INT_RODAS5); on by default (kmax 10 under rodas4, 16 under rodas5, whose attempts also
               cap the exponent per remaining step), acts only on models with a contraction-rate hook (extraction cascades)
  cooperative  rodas4 / rodas5 on multistage_extraction with eq_exponent == 2 only: {'thr': 60} | False -- env steps whose
               predicted cost (attempts of the pair, a per-env rule) reaches thr take SEULEX-8, eight lanes per env in the
               work-queue kernel (pcgym_hip.h: coop_thr; pcg_seulex.hpp); on by default under rodas4, OPT-IN under rodas5 (there
               SEULEX-8 runs at 4 x 8e-8: worst 1.4e-6 of a 1e-13 solve over the action box against 8e-7 for the pair alone,
               tests/test_rodas5.py)
  substeps     RK4 sub-steps per env step
  rtol, atol   DOPRI5 tolerances (default 1e-8, integrator.py:61)
  max_steps    DOPRI5 step budget per env step
  reference_compat  replicate reference quirks Q1/Q3 (default True)
  gaussian_disturbances {name: sigma}  in-kernel N(0,1)*sigma added to the schedule,
                    clipped to disturbance_bounds (BASELINE.json configs[4])
"""
from __future__ import annotations

import copy
import ctypes as C
import os
import re
from collections import OrderedDict

import numpy as np

from . import _abi as abi
from . import models as M

# integration_method -> integrator.  'casadi' (CVODES, reltol 1e-6) and the
# default 'hip' map to the per-model default below; 'jax' (diffrax Tsit5,
# rtol=atol=1e-8, integrator.py:56-61) maps to the adaptive 5(4) pair.
DEFAULT_INTEGRATOR = {
    M.COMPLEX_CSTR: "dopri5", M.DISEASE: "dopri5", M.BATCH: "dopri5", M.PHOTO: "dopri5", M.CSTR_SERIES: "dopri5",
    M.DISTILLATION: "dopri5", M.POLYMER: "dopri5",   # no tuned fixed step yet: adaptive by default
    M.BIOFILM: "dopri5", M.HEAT_EX: "dopri5", M.INV_BATCH: "dopri5", M.OSCILLATORS: "dopri5",
    # cstr: adaptive by default.  The reaction ignites for T0 >~ 334 K inside the canonical observation box
    # (o_space T up to 350 K, cstr_train.py:12-47); on that branch |lambda| dt >> 2.78 and fixed-step RK4 returns
    # finite garbage, while the reference's CVODES integrates it.  integrator='rk4' stays available as an explicit
    # opt-in for the canonical closed loop (T < 330 K), where 4 sub-steps reach 6e-8.
    # Round 3: 'rk4g' -- RK4 x 5 under the model's guard (no growing mode, resolved fastest rate, at every sub-step start
    # and at the end state); an env that trips it is re-integrated by the adaptive pair at 1e-10 inside the same step call (round 4: by a
    # second launch -- the pair's work-queue kernel over the marked envs -- when the batch fills the chip).
    # The canonical closed loop never trips it (128 -> ~37 us per 2^20-env step); the ignition and hot branches always do.
    # Later in round 3: 'tsit5g' -- the same guard at every stage state of TWO fixed Tsit5 steps: the accuracy of RK4 x 5
    # (7.5e-7 against 6.9e-7 on the accepted envs, tests/test_erk.py) with 12 right-hand sides instead of 20: 44.7 ->
    # 37.3 us per 2^20-env step of the canonical loop, the same 642 us on the full x0 box (where the escalated envs are
    # the cost).  'rk4g' stays available.
    M.CSTR: "tsit5g",
    # four_tank: one step of the order-8 Cooper-Verner method per canonical dt (11 right-hand sides, 7e-7) instead of
    # RK4 x 5 (20, 1.8e-6 on the same sample): the square roots are what this model costs
    M.FOUR_TANK: "cv8",
    # stiff at high L,G (|lambda| dt up to ~240).  Round 3: the fourth-order Rosenbrock pair with the cascade's
    # structured linear algebra and end-point error control -- what the reference does with CVODES BDF
    # (integrator.py:163-182) -- 19 attempts per env step over the action box against 72 for the explicit pair, same
    # accuracy class (<= 1e-6 of a 1e-13 solve).  integration_method='jax' and plans with per-env uncertain parameters
    # keep the explicit pair.  Round 5: the FIFTH-order pair of the same family (8 stages against 6): the cascade is
    # accuracy-bound under the fourth-order one, and 10.8 attempts replace 20.3 in the same class (6.0e-7 against 6.6e-7;
    # me10 at B = 2^18: 311 -> 222 us per step).  `integrator: 'rodas4'` keeps round 3's plan.
    M.ME: "rodas5",
    M.ME_REACTIVE: "dopri5",
    # crystallization: four order-8 steps per model time unit (44 right-hand sides; 8.9e-9 of a 1e-13 solve over the action
    # box, 3.6e-7 on the LSODA fixture's wider sample) instead of RK4 x 32 (128; 6.2e-8 and 5.6e-7; three steps: 2.5e-6 on
    # the fixture) -- BASELINE configs[3] names the sub-stepped RK4 plan, which stays
    # `integrator='rk4'` (and the bench's `cryst` line)
    M.CRYST: "cv8",
    M.AFFINE: "rk4",
    M.USER: "dopri5",         # nothing is known about a user's right-hand side: adaptive
}
# Default RK4 sub-step length per model (model time units): substeps = ceil(dt / h).  Chosen so that
# the canonical configs (cstr dt=26/60 -> 4, four_tank dt=1000/60 -> 5, cryst dt=1 -> 32, ME dt=1 ->
# 128) reach <=1e-6 relative, the accuracy class of the reference's CVODES defaults (SURVEY.md
# section 8a table).  Fixed-step RK4 is only conditionally stable: outside the canonical operating
# range (cstr thermal runaway, ME at high flows) use integrator='dopri5'.
# four_tank: 5 sub-steps per canonical dt (round 3; 4 before).  Measured on 500,000 (state, action) pairs of episodes under
# the bench's action distribution against a 1e-13 solve: worst relative error 2.5e-6 with 4, 9.8e-7 with 5, 4.6e-7 with 6
# (the square-root outflow makes low tanks the hard cases) -- 5 is the smallest count inside the 1e-6 class.
DEFAULT_RK4_H = {M.CSTR: 26.0 / 60.0 / 4, M.FOUR_TANK: 1000.0 / 60.0 / 5, M.ME: 1.0 / 128,
                 M.ME_REACTIVE: 1.0 / 32, M.CRYST: 1.0 / 32, M.AFFINE: None, M.COMPLEX_CSTR: None, M.DISEASE: None,
                 M.BATCH: None, M.PHOTO: None, M.CSTR_SERIES: None, M.DISTILLATION: None, M.POLYMER: None}


# Default DOPRI5 tolerance (rtol = atol) where it differs from the 1e-8 of the reference's jax path
# (integrator.py:61).  cstr: the ignition front amplifies local errors ~100x; measured over the whole observation
# box U(0.7,1.0) x U(310,350) K at dt = 26/60 against a 1e-13 solve, the worst relative error of one env step is
# 6.5e-5 at 1e-8, 7.2e-6 at 1e-9, 3.5e-7 at 1e-10 -- the last is inside the 1e-6 class of the reference's CVODES
# defaults everywhere, at ~1.8x the steps of 1e-8.
DEFAULT_TOL = {M.CSTR: 1e-10}
# ... and what is owed THROUGH the front (round 5).  The reference's own CVODES (CasADi defaults: reltol 1e-6, abstol 1e-8) is
# ~1e-4 off a 1e-13 solve on an env that ignites inside the step; 1e-10 held such envs to 3.5e-7 at the price of the longest
# chain of any launch (152 attempts of the explicit pair at dt = 1 s: a batch waits for its heaviest env).  The statement
# now: EVERY env of the observation box -- and of the deliberately wide box of tests/test_erk.py (already-ignited states up
# to 600 K) -- ends within 3 x the reference's tolerances (3e-6 |x| + 3e-8) of the 1e-13 solve, the bar the guarded plans
# already hold their trusted envs to.  The front amplifies a local error by a factor that grows with the time left in the
# step, so the tolerance scales with 1 / dt: 1e-9 at dt = 1/60 (worst 0.29 x the reference's tolerances on the box, 1.5 x
# on the wide box -- whose tail rules out 5e-9: 7.7 x --, heaviest env 102 attempts), 1e-10 from dt = 1/6 on (canonical
# dt = 26/60: 0.28 x / 1.2 x as before) (tools/prototypes/cstr_front_tol.py, profiles/r5/cstr_front_tol.txt).
CSTR_TOL_CAL, CSTR_DT_CAL = 1e-9, 1.0 / 60.0


def cstr_default_tol(dt):
    return float(min(CSTR_TOL_CAL, max(DEFAULT_TOL[M.CSTR], CSTR_TOL_CAL * CSTR_DT_CAL / dt)))
# integrator = 'rodas4' (fourth-order Rosenbrock pair with end-point error control): tolerance that keeps one env step
# of the extraction cascade within 1e-6 of a 1e-13 solve over its whole action box (worst lanes: low liquid flow, high
# gas flow -- 6.5e-7 at 3e-8; tests/test_rodas4.py), the class of the explicit pair at 1e-8 (5.5e-7)
ROS4_TOL = {M.ME: 3e-8}
# integrator = 'rodas5' (fifth-order pair, same hooks): worst 6.0e-7 over the action box at 8e-8 with end-point exponents up
# to 16 under the step cap, at 0.53 x the attempts of the fourth-order pair (tests/test_rodas5.py, profiles/r5/rodas5_calib.txt)
ROS5_TOL = {M.ME: 8e-8}
ROS5_NONDEFAULT_CURVE = 0.5  # factor on ROS5_TOL for eq_exponent != 2 (EnvSpec: the round-6 contract, profiles/r6/rodas5_contract.txt)
DEFAULT_COOP_THR = 60.0  # cooperative rule of rodas4 plans: predicted attempts from which an env step takes SEULEX-8 (pcg_seulex.hpp)
ROS4_DT_CAL = 1.0  # the env step (model time units) ROS4_TOL was calibrated at; larger steps tighten it (EnvSpec)


# integrator = 'cv8' (Cooper-Verner order 8, 11 stages): step length per model.  four_tank: ONE step per canonical dt
# (7.2e-7 of a 1e-13 solve against 1.8e-6 for RK4 x 5 on the same sample, tools/prototypes/erk_fixed.py); crystallization:
# four per model time unit (tests/test_erk.py)
DEFAULT_CV8_H = {M.FOUR_TANK: 1000.0 / 60.0, M.CRYST: 1.0 / 4}
# name -> id of the C ABI, in the order the "integrator must be one of ..." message lists them
_INTEGRATOR_ID = {"rk4": abi.PCG_INT_RK4, "rk4g": abi.PCG_INT_RK4G, "tsit5g": abi.PCG_INT_T5G, "cv8": abi.PCG_INT_CV8,
                  "dopri5": abi.PCG_INT_DOPRI5, "tsit5": abi.PCG_INT_TSIT5, "rodas3": abi.PCG_INT_RODAS3,
                  "rodas4": abi.PCG_INT_RODAS4, "rodas5": abi.PCG_INT_RODAS5}
INTEGRATOR_IDS = tuple(_INTEGRATOR_ID)
ROS_PAIRS = ("rodas4", "rodas5")  # the two Rosenbrock pairs: one set of hooks (end-point control, cooperative rule, structured W)


def default_substeps(model_id, dt):
    h = DEFAULT_RK4_H.get(model_id)
    if h is None:
        return 8
    return max(1, int(np.ceil(dt / h - 1e-9)))

_f64 = np.float64
_CTYPE = {np.float64: C.c_double, np.int32: C.c_int32, np.uint8: C.c_uint8}


def _arr(v, dtype=_f64):
    return np.ascontiguousarray(np.asarray(v, dtype=dtype).reshape(-1))


def probe_affine(fn, dims, sample_points, what):
    """Recover (A, c) with fn(z_0, z_1, ...) == A @ concat(z) + c for a Python callable
    that is affine in its arguments; raise ValueError when it is not.

    The reference accepts arbitrary callables for ``constraints`` (pcgym.py:119-125)
    and ``custom_model`` (pcgym.py:150-153); a Python callable cannot run inside a
    kernel, so the engine takes the declarative (affine) subset and says so loudly
    otherwise.  Probing at 0 and the unit vectors is exact for affine maps.
    """
    n = int(sum(dims))

    def call(z):
        parts, o = [], 0
        for d in dims:
            parts.append(np.array(z[o:o + d], dtype=_f64))
            o += d
        with np.errstate(all="ignore"):
            out = np.asarray(fn(*parts), dtype=_f64).reshape(-1)
        return out

    c = call(np.zeros(n))
    m = c.shape[0]
    A = np.zeros((m, n))
    for i in range(n):
        e = np.zeros(n)
        e[i] = 1.0
        A[:, i] = call(e) - c
    if not (np.all(np.isfinite(A)) and np.all(np.isfinite(c))):
        raise ValueError(f"{what}: callable is not affine (non-finite value at the probe points); "
                         "only affine callables can be compiled into the HIP step kernel")
    for z in sample_points:
        z = np.asarray(z, dtype=_f64).reshape(-1)
        want = call(z)
        got = A @ z + c
        tol = 1e-9 * (np.abs(A) @ np.abs(z) + np.abs(c) + 1e-300)
        if not np.all(np.abs(want - got) <= tol):
            raise ValueError(f"{what}: callable is not affine in its arguments; only affine "
                             "callables can be compiled into the HIP step kernel "
                             "(pass the declarative form {'A':..., 'b':...} or an affine function)")
    return A, c


# ---- tracing a Python callable into C expressions ------------------------------------------------------------------
# The reference's callables (custom_model.__call__(x, u), constraints(x, u)) are plain arithmetic over array elements,
# model attributes and a few numpy functions (model_classes.py).  Calling one with symbolic scalars records that
# arithmetic as a C expression; what cannot be recorded -- control flow on values -- raises.  The recorded expressions
# are then evaluated numerically against the callable itself at random points before they are accepted.
class _TraceError(TypeError):
    pass


class _Sym:
    """a scalar whose value is a C expression over x[] / u[]"""
    __slots__ = ("e",)
    __array_priority__ = 1000.0

    def __init__(self, e):
        self.e = e

    @staticmethod
    def _lit(v):
        if isinstance(v, _Sym):
            return v.e
        if isinstance(v, (bool, np.bool_)):
            raise _TraceError("boolean in arithmetic")
        a = np.asarray(v)
        if a.size != 1 or a.dtype == object:
            raise _TraceError("a constant of the callable is not a scalar number")
        f = float(a.reshape(-1)[0])
        if not np.isfinite(f):
            raise _TraceError("non-finite constant")
        r = repr(f)
        return f"({r})" if f < 0 else r

    def _bin(self, o, op, rev=False):
        a, b = (self._lit(o), self.e) if rev else (self.e, self._lit(o))
        return _Sym(f"({a} {op} {b})")

    def __add__(self, o): return self._bin(o, "+")
    def __radd__(self, o): return self._bin(o, "+", True)
    def __sub__(self, o): return self._bin(o, "-")
    def __rsub__(self, o): return self._bin(o, "-", True)
    def __mul__(self, o): return self._bin(o, "*")
    def __rmul__(self, o): return self._bin(o, "*", True)
    def __truediv__(self, o): return self._bin(o, "/")
    def __rtruediv__(self, o): return self._bin(o, "/", True)
    def __neg__(self): return _Sym(f"(-{self.e})")
    def __pos__(self): return self
    def __abs__(self): return _Sym(f"fabs({self.e})")

    def __pow__(self, o):
        if not isinstance(o, _Sym) and float(o) == 2.0:
            return _Sym(f"({self.e} * {self.e})")
        return _Sym(f"pow({self.e}, {self._lit(o)})")

    def __rpow__(self, o): return _Sym(f"pow({self._lit(o)}, {self.e})")

    # numpy ufuncs on object arrays call the method of the same name
    def exp(self): return _Sym(f"exp({self.e})")
    def log(self): return _Sym(f"log({self.e})")
    def sqrt(self): return _Sym(f"sqrt({self.e})")
    def sin(self): return _Sym(f"sin({self.e})")
    def cos(self): return _Sym(f"cos({self.e})")
    def tanh(self): return _Sym(f"tanh({self.e})")
    def fabs(self): return _Sym(f"fabs({self.e})")
    absolute = fabs

    def _no(self, *a, **k):
        raise _TraceError("the callable branches on (or converts) a value that depends on the state / input: "
                          "control flow cannot be compiled into a kernel expression")
    __bool__ = __float__ = __int__ = __index__ = _no
    __lt__ = __le__ = __gt__ = __ge__ = __eq__ = __ne__ = _no
    __hash__ = None


def trace_callable(fn, dims, sample_points, what, arg_names=("x", "u")):
    """Record ``fn(z_0, z_1, ...)`` (arguments of sizes ``dims``) as one C expression per output over ``x[i]`` /
    ``u[j]``; checked numerically against ``fn`` itself at ``sample_points`` (concatenated arguments)."""
    import math

    args = [np.array([_Sym(f"{arg_names[k]}[{i}]") for i in range(d)], dtype=object) for k, d in enumerate(dims)]
    try:
        out = fn(*args)
    except _TraceError as e:
        raise ValueError(f"{what}: {e}") from None
    except Exception as e:  # noqa: BLE001  (whatever numpy makes of an object array the callable did not expect)
        raise ValueError(f"{what}: the callable could not be traced into expressions ({type(e).__name__}: {e})") from None
    flat = list(np.asarray(out, dtype=object).reshape(-1)) if not isinstance(out, _Sym) else [out]
    exprs = [v.e if isinstance(v, _Sym) else _Sym._lit(v) for v in flat]
    env = {k: getattr(math, k) for k in ("exp", "log", "sqrt", "sin", "cos", "tanh", "fabs")}
    env["pow"] = math.pow
    verified = 0
    for z in sample_points:
        z = np.asarray(z, dtype=_f64).reshape(-1)
        parts, o = [], 0
        for d in dims:
            parts.append(np.array(z[o:o + d], dtype=_f64))
            o += d
        with np.errstate(all="ignore"):
            want = np.asarray(fn(*[q.copy() for q in parts]), dtype=_f64).reshape(-1)
        scope = dict(env, **{arg_names[k]: list(map(float, parts[k])) for k in range(len(dims))})
        try:
            got = np.array([float(eval(e, {"__builtins__": {}}, scope)) for e in exprs])  # noqa: S307 (our own text)
        except (ValueError, ZeroDivisionError, OverflowError):
            continue  # outside the callable's domain at this probe point
        ok = np.isfinite(want)
        if want.shape != got.shape or not np.all(np.abs(want[ok] - got[ok]) <= 1e-9 * (np.abs(want[ok]) + 1e-12) + 1e-300):
            raise ValueError(f"{what}: the traced expressions do not reproduce the callable (it probably contains "
                             "control flow or state that tracing cannot see)")
        verified += int(ok.any())
    if verified == 0:  # never compile a trace that no probe point could confirm
        raise ValueError(f"{what}: the traced expressions could not be checked against the callable at any probe point "
                         "(every evaluation left its domain); write the expressions out instead")
    return exprs


class _SPSeries:
    """``self.SP[key]`` inside a traced custom_reward: a set-point schedule that may be scaled / shifted element-wise and
    is finally indexed with ``self.t`` -- which yields the kernel's ``sp[k]`` (the value at the NEW step counter, what the
    reference's callables read after ``self.t += 1``, pcgym.py:441, 470-471)"""
    __array_priority__ = 2000.0

    def __init__(self, elem):
        self.elem = elem  # _Sym over sp[k]

    def _map(self, f):
        return _SPSeries(f(self.elem))

    def __add__(self, o): return self._map(lambda e: e + o)
    def __radd__(self, o): return self._map(lambda e: o + e)
    def __sub__(self, o): return self._map(lambda e: e - o)
    def __rsub__(self, o): return self._map(lambda e: o - e)
    def __mul__(self, o): return self._map(lambda e: e * o)
    def __rmul__(self, o): return self._map(lambda e: o * e)
    def __truediv__(self, o): return self._map(lambda e: e / o)
    def __neg__(self): return self._map(lambda e: -e)

    def __getitem__(self, idx):
        if isinstance(idx, _TStep):
            return self.elem
        raise _TraceError("a set-point schedule may only be indexed with self.t in a custom_reward that is to be compiled")


class _TStep(_Sym):
    """``self.t`` inside a traced custom_reward: the expression variable ``t``; indexes a schedule"""
    __slots__ = ()

    def __init__(self):
        super().__init__("t")


class _RewardSelf:
    """the ``self`` a traced custom_reward sees: the attributes the reference's callables read (pcgym.py:470-471 hands
    them the env itself) -- SP, t, N, dt, tsim, env_params, model, a few sizes.  Anything else (``self.u_prev`` and
    other state kept on the env between calls) is an AttributeError: such a reward is not a function of this step alone
    and cannot be compiled (the declarative ``sp_track`` form covers the paper's family)."""

    def __init__(self, spec, symbolic, t=None):
        self.env_params = spec.env_params
        self.model = _ModelInfo(spec)
        self.N, self.dt, self.tsim = spec.N, spec.dt, spec.tsim
        self.Nx, self.Nx_oracle, self.Nu = spec.nobs, spec.nx, spec.nu
        if symbolic:
            self.t = _TStep()
            self.SP = {k: _SPSeries(_Sym(f"sp[{j}]")) for j, k in enumerate(spec.sp_keys)}
        else:
            self.t = int(t)
            self.SP = {k: np.asarray(spec.sp[j], dtype=_f64) for j, k in enumerate(spec.sp_keys)}


class _ModelInfo:
    def __init__(self, spec):
        self._info = {"states": list(spec.model.states), "inputs": list(spec.model.inputs),
                      "disturbances": list(spec.model.disturbances), "parameters": dict(spec.model.parameters)}

    def info(self):
        return self._info


def trace_reward_callable(fn, spec):
    """``custom_reward(self, obs, uk, violated)`` (pcgym.py:201-205, 470-471) -> ONE C expression over o[], u[], sp[],
    violated, t, N for the batched kernel.  The callable is run twice on symbolic scalars, once per value of
    ``violated`` (a plain bool, so ``if con:`` works), with ``float`` neutralised
    (the usual ``return float(...)``) -- in a COPY of the function over a copy of its globals, the module itself is left
    alone; the result is checked numerically against the callable itself."""
    import math

    # `float(...)` of a symbolic scalar has to hand the scalar back.  The callable's module is NOT touched (another thread
    # may be running it): a copy of the function is executed over a copy of its globals in which `float` is neutral; a
    # callable that is not a plain function / bound method is run as it is (`float()` of a symbolic scalar then raises a
    # trace error, and the caller is told to use the declarative forms).
    import types

    def neutral_float(v=0.0):
        return v if isinstance(v, _Sym) else float(v)

    run = fn
    f0 = getattr(fn, "__func__", fn)
    if isinstance(f0, types.FunctionType):
        g2 = dict(f0.__globals__)
        g2["float"] = neutral_float
        f2 = types.FunctionType(f0.__code__, g2, f0.__name__, f0.__defaults__, f0.__closure__)
        f2.__kwdefaults__ = f0.__kwdefaults__
        run = types.MethodType(f2, fn.__self__) if isinstance(fn, types.MethodType) else f2
    exprs = {}
    for con in (False, True):
        o = np.array([_Sym(f"o[{i}]") for i in range(spec.nobs)], dtype=object)
        u = np.array([_Sym(f"u[{j}]") for j in range(spec.nu)], dtype=object)
        try:
            r = run(_RewardSelf(spec, True), o, u, con)
        except _TraceError as e:
            raise ValueError(f"custom_reward: {e}") from None
        except Exception as e:  # noqa: BLE001
            raise ValueError("custom_reward: the callable could not be traced into an expression "
                             f"({type(e).__name__}: {e}); it probably keeps state on the env (self.u_prev ...) -- use "
                             "the declarative {'kind': 'sp_track'} form or {'expr': ...}") from None
        r = np.asarray(r, dtype=object).reshape(-1)
        if r.size != 1:
            raise ValueError("custom_reward: the callable must return one number")
        exprs[con] = r[0].e if isinstance(r[0], _Sym) else _Sym._lit(r[0])
    text = exprs[False] if exprs[False] == exprs[True] else f"((violated) ? ({exprs[True]}) : ({exprs[False]}))"
    # numeric confirmation against the callable itself: random observations in the observation box, inputs in the
    # action box (+ nominal disturbance inputs), random step counters, both values of `violated`
    rng = np.random.default_rng(0)
    env = {k: getattr(math, k) for k in ("exp", "log", "sqrt", "sin", "cos", "tanh", "fabs")}
    env["pow"] = math.pow
    verified = 0
    for trial in range(8):
        o = spec.o_low + rng.uniform(0.05, 0.95, spec.nobs) * (spec.o_high - spec.o_low)
        u = np.concatenate([spec.a_low + rng.uniform(0, 1, spec.na) * (spec.a_high - spec.a_low),
                            np.asarray(spec.d_default, dtype=_f64)[:spec.ndm]])
        t = int(rng.integers(1, spec.N))
        for con in (False, True):
            with np.errstate(all="ignore"):
                want = float(np.asarray(fn(_RewardSelf(spec, False, t), o.copy(), u.copy(), con), dtype=_f64).reshape(-1)[0])
            scope = dict(env, o=list(map(float, o)), u=list(map(float, u)), sp=[float(spec.sp[j][t]) for j in range(spec.nsp)],
                         violated=int(con), t=t, N=spec.N)
            e = exprs[con]
            try:
                got = float(eval(e, {"__builtins__": {}}, scope))  # noqa: S307 (our own text)
            except (ValueError, ZeroDivisionError, OverflowError):
                continue
            if np.isfinite(want):
                if abs(want - got) > 1e-9 * (abs(want) + 1e-12):
                    raise ValueError("custom_reward: the traced expression does not reproduce the callable (hidden state or "
                                     "control flow that tracing cannot see)")
                verified += 1
    if verified == 0:
        raise ValueError("custom_reward: the traced expression could not be checked against the callable at any probe point")
    return text


_EXPR_FUNCS = {"exp", "log", "sqrt", "pow", "fabs", "fmin", "fmax", "sin", "cos", "tanh"}


def compile_expr(text, names, arrays, scalars, what):
    """One user expression (C syntax) -> C source over the kernel's arrays.

    The reference takes Python callables for ``constraints`` (pcgym.py:119-125) and ``custom_reward``
    (pcgym.py:201-205); a batched kernel cannot call Python, so the non-affine cases are written as C expressions and
    compiled into the step kernel at plan creation (hipRTC).  ``names`` maps model names (states, inputs, 'SP_<key>')
    to array elements; only those, the arrays in ``arrays`` (indexed with integer literals), the scalars in
    ``scalars``, numeric literals, arithmetic / comparison / ?: operators and a few math functions are accepted."""
    if not isinstance(text, str) or not text.strip():
        raise ValueError(f"{what}: expression must be a non-empty string")
    if re.search(r"[;{}\\#\"']|//|/\*", text):
        raise ValueError(f"{what}: only a single expression is accepted (no statements, comments or strings): {text!r}")
    if re.search(r"(?<![=!<>])=(?!=)|\+\+|--", text):
        raise ValueError(f"{what}: assignments / increments are not accepted: {text!r}")
    out, pos = [], 0
    for m in re.finditer(r"[A-Za-z_][A-Za-z_0-9]*", text):
        out.append(text[pos:m.start()])
        w = m.group(0)
        prev = text[:m.start()].rstrip()[-1:] if m.start() else ""
        if prev.isdigit() or prev == ".":  # exponent of a numeric literal: 1e-3
            if re.fullmatch(r"[eE][0-9]*", w):
                out.append(w)
                pos = m.end()
                continue
        if w in names:
            out.append(names[w])
        elif w in arrays or w in scalars or w in _EXPR_FUNCS:
            out.append(w)
        else:
            raise ValueError(f"{what}: unknown name '{w}' in {text!r} (known: {sorted(names)} + {sorted(arrays)} "
                             f"+ {sorted(scalars)} + {sorted(_EXPR_FUNCS)})")
        pos = m.end()
    out.append(text[pos:])
    return "".join(out)


def _name_map(info, state_array, params=(), dist_at=None, sp_lvalues=()):
    """model names -> C lvalues for compile_expr: states -> ``state_array[i]``, inputs -> u[j], parameters -> p[k],
    disturbance inputs -> u[dist_at + j] (they shadow the parameter of the same name), 'SP_<key>' -> ``sp_lvalues``"""
    names = {n: f"{state_array}[{i}]" for i, n in enumerate(info["states"])}
    names.update({n: f"u[{j}]" for j, n in enumerate(info["inputs"])})
    names.update({n: f"p[{k}]" for k, n in enumerate(params)})
    if dist_at is not None:
        names.update({n: f"u[{dist_at + j}]" for j, n in enumerate(info["disturbances"])})
    names.update({f"SP_{k}": lv for k, lv in sp_lvalues})
    return names


def _assign_lines(target, exprs):
    """C expressions -> one ``target[i] = (double)(...);`` statement per line (hashed into the run-time compilation
    cache key: the text is part of the contract)"""
    return "\n".join(f"  {target}[{i}] = (double)({e});" for i, e in enumerate(exprs))


# ---- custom_model (pcgym.py:150-153) ---------------------------------------------------------------------------------
def adopt_custom_model(m, p, a_low, a_high):
    """-> (ModelInfo, affine (A, B, c) | None, (rhs, aux) expressions | None, traced rhs | None).  A declarative
    right-hand side is compiled as written; registry-shaped objects reuse the matching kernel with the object's
    parameter values; any other object is probed -- affine ones become PCG_MODEL_AFFINE, the rest are traced."""
    rhs = m.get("rhs") if isinstance(m, dict) else getattr(m, "rhs_expr", None)
    if rhs is not None:
        mi, exprs = _declarative_model(m, rhs)
        return mi, None, exprs, None
    mi = _registry_shaped_model(m)
    if mi is not None:
        return mi, None, None, None
    return _probed_model(m, p, a_low, a_high)


def _declarative_model(m, rhs):
    """(a) declarative form with an arbitrary right-hand side: C expressions, compiled at plan creation"""
    info = m if isinstance(m, dict) else m.info()
    states, inputs = list(info["states"]), list(info["inputs"])
    dist = [d for d in info.get("disturbances", []) if d != "None"]
    params = OrderedDict((str(k), float(v)) for k, v in dict(info.get("parameters", {})).items())
    aux = (m.get("aux") if isinstance(m, dict) else getattr(m, "aux_expr", None)) or {}
    if len(rhs) != len(states):
        raise ValueError(f"custom_model: {len(rhs)} rhs expressions for {len(states)} states")
    if not (1 <= len(states) <= abi.PCG_MAX_NX) or not (1 <= len(inputs) <= abi.PCG_MAX_NA) \
            or len(dist) > abi.PCG_MAX_NDM or len(params) > abi.PCG_MAX_USER_PARAMS:
        raise ValueError(f"custom_model: at most {abi.PCG_MAX_NX} states, {abi.PCG_MAX_NA} inputs, "
                         f"{abi.PCG_MAX_NDM} disturbance inputs, {abi.PCG_MAX_USER_PARAMS} parameters")
    for d in dist:
        if d not in params:
            raise ValueError(f"custom_model: disturbance input '{d}' needs a parameter of the same name (its value "
                             "when no disturbance is configured; the reference's models do the same, "
                             "model_classes.py:43,51)")
    for k in aux:
        if not re.fullmatch(r"[A-Za-z_][A-Za-z_0-9]*", str(k)) or str(k) in _EXPR_FUNCS | {"x", "u", "p", "dx"}:
            raise ValueError(f"custom_model: aux name {k!r} is not usable")
    names = states + inputs + list(params) + [str(k) for k in aux]
    if len(set(names)) != len(names):
        raise ValueError(f"custom_model: state / input / parameter / aux names must be distinct: {names}")
    exprs = ([str(e) for e in rhs], OrderedDict((str(k), str(v)) for k, v in aux.items()))
    return M.ModelInfo(str(info.get("name", "custom_expr")), M.USER, states, inputs, dist, list(params.items())), exprs


_REGISTRY_SHAPED = ("cstr", "four_tank", "multistage_extraction", "multistage_extraction_reactive", "crystallization")


def _registry_shaped_model(m):
    """an object named like a registry model and with its states: that kernel, the object's parameter values"""
    info = m.info()
    cls = type(m).__name__
    if cls not in _REGISTRY_SHAPED or list(info["states"]) != M.get_model(cls).states:
        return None
    mi = M.get_model(cls)
    for k in mi.parameters:
        if k in info["parameters"]:
            mi.parameters[k] = float(info["parameters"][k])
    return mi


def _probed_model(m, p, a_low, a_high):
    """any other Python model: an affine right-hand side is recovered exactly (PCG_MODEL_AFFINE); otherwise, and beyond
    the affine kernel's matrices, its arithmetic is recorded as C expressions and compiled (PCG_MODEL_USER)"""
    info = m.info()
    cls = type(m).__name__
    nx = len(info["states"])
    nu = len(info["inputs"])
    dist = [d for d in info.get("disturbances", []) if d != "None"]
    if p.get("disturbances") is not None:
        nu += len(dist)
    if nu > abi.PCG_MAX_NU or nx > abi.PCG_MAX_NX:
        raise ValueError(f"custom_model: at most {abi.PCG_MAX_NX} states and {abi.PCG_MAX_NU} inputs")
    rng = np.random.default_rng(11)
    x0 = _arr(p["x0"])[:nx]
    pts = [np.concatenate([x0 * (1 + 0.1 * rng.uniform(-1, 1, nx)) + 0.01 * rng.uniform(-1, 1, nx),
                           rng.uniform(-1, 1, nu)]) for _ in range(3)]
    try:
        A, c = probe_affine(lambda x, u: m(x, u), [nx, nu], pts, "custom_model")
        if nx > 8 or nu > 4:  # beyond the compiled affine kernel's matrices: take the general route
            raise ValueError("custom_model: affine, but larger than the affine kernel (8 states, 4 inputs)")
    except ValueError as not_affine:
        # (a model without inputs -- the reference's coupled_oscillators(N=...) for any ring size, invariant_batch --
        # is carried with one dummy action its right-hand side never reads, as the registry's own no-input models)
        na = len(info["inputs"])
        if not (1 <= nx <= abi.PCG_MAX_NX) or not (0 <= na <= abi.PCG_MAX_NA) or len(dist) > abi.PCG_MAX_NDM:
            raise not_affine
        for d in dist:
            if d not in info.get("parameters", {}):
                raise ValueError(f"custom_model: disturbance input '{d}' needs a parameter of the same name") from None
        lo, hi = a_low[:na], a_high[:na]
        phys = []
        for _ in range(4):
            us = lo + rng.uniform(0, 1, na) * (hi - lo)
            ds = np.array([float(info["parameters"][d]) * (1 + 0.05 * rng.uniform(-1, 1)) for d in dist])[: nu - na]
            phys.append(np.concatenate([x0 * (1 + 0.05 * rng.uniform(-1, 1, nx)), us, ds]))
        try:
            traced = trace_callable(lambda x, u: m(x, u), [nx, nu], phys, "custom_model")
        except ValueError as not_traceable:
            raise ValueError(f"{not_affine}; and {not_traceable}") from None
        if len(traced) != nx:
            raise ValueError(f"custom_model returned {len(traced)} derivatives for {nx} states") from None
        mi = M.ModelInfo(cls, M.USER, info["states"], info["inputs"], dist, [(d, float(info["parameters"][d])) for d in dist])
        return mi, None, None, traced
    mi = M.ModelInfo(cls, M.AFFINE, info["states"], info["inputs"], dist, list(info.get("parameters", {}).items()))
    return mi, (A[:, :nx].copy(), A[:, nx:].copy(), c.copy()), None, None


# ---- integrator plan (new keys) ---------------------------------------------------------------------------------------
def integrator_plan(model_id, params, dt, nunc, integration_method, affine_A, has_user_rhs, user):
    """-> (integrator, substeps, rtol, atol, max_steps, ep_frac, ep_kmax, coop_thr) from plain values: the model id and
    its parameter vector, the env step, the number of per-env uncertain parameters, the affine A (or None), whether the
    right-hand side is run-time compiled, and ``user``, a mapping holding the optional keys 'integrator',
    'endpoint_control', 'cooperative', 'substeps', 'rtol', 'atol', 'max_steps'"""
    integrator = _choose_integrator(model_id, nunc, integration_method, user)
    ep_frac, ep_kmax = _endpoint_control(integrator, user.get("endpoint_control", True))
    # cooperative rule: where the kernels carry it (the 10-state cascade with eq_exponent == 2 through the structured
    # Rosenbrock path, registry parameters or not) it is on; asking for it elsewhere is an error, not a silent no-op
    default_curve = model_id == M.ME and len(params) > 4 and float(params[4]) == 2.0
    coop_ok = integrator in ROS_PAIRS and default_curve and nunc == 0 and not has_user_rhs
    coop_thr = _cooperative_threshold(integrator, coop_ok, user.get("cooperative", None))
    substeps = int(user.get("substeps", _default_substeps(integrator, model_id, dt, affine_A)))
    d_tol = _default_tolerance(integrator, model_id, dt, integration_method, default_curve)
    rtol, atol = float(user.get("rtol", d_tol)), float(user.get("atol", d_tol))
    max_steps = int(user.get("max_steps", 100000))
    if substeps < 0:
        raise ValueError("substeps must be >= 1 (0 = skip the integration: memory-roofline probe only)")
    return integrator, substeps, rtol, atol, max_steps, ep_frac, ep_kmax, coop_thr


def _choose_integrator(model_id, nunc, integration_method, user):
    d_int = DEFAULT_INTEGRATOR[model_id]
    if integration_method == "jax":
        # diffrax.Tsit5 + PIDController(rtol = atol = 1e-8): the same tableau, tolerances and step-size controller
        # family here; plans it has no kernel for (per-env parameters) use the Dormand-Prince pair of the same class
        d_int = "tsit5" if nunc == 0 else "dopri5"
    elif d_int in ("rodas4", "rodas5", "rk4g", "tsit5g") and nunc > 0:
        d_int = "dopri5"
    elif d_int == "cv8" and nunc > 0:
        d_int = "rk4"
    integrator = user.get("integrator", d_int)
    if integrator not in INTEGRATOR_IDS:
        raise ValueError("integrator must be one of " + ", ".join(repr(k) for k in INTEGRATOR_IDS))
    if nunc > 0 and integrator in ("rodas4", "rodas5", "rodas3", "rk4g", "tsit5g", "cv8", "tsit5"):
        raise ValueError(f"integrator '{integrator}' has no kernel for per-env uncertain parameters "
                         "(uncertainty_percentages on model parameters): use 'rk4' or 'dopri5'")
    if integrator in ("rk4g", "tsit5g") and model_id != M.CSTR:
        raise ValueError(f"integrator '{integrator}' (guarded fixed step) needs a model with a guard hook: cstr")
    return integrator


def _endpoint_control(integrator, epc):
    if integrator not in ROS_PAIRS or epc is False or epc is None:
        return 0.0, 0
    epc = {} if epc is True else dict(epc)
    # kmax: the largest relaxation 2^kmax of an early attempt's tolerance.  The fifth-order pair caps the exponent of
    # an attempt at two bits per remaining step of its size (pcg_integrators.hpp: ros_ep_cap -- the steps' own damping
    # |R(h lambda)| is what an early error really meets), and with that cap the exponents can grow to 16: 10.8 attempts
    # per env step over the action box, worst 6.0e-7 - 6.3e-7 on three samples (12: 11.3 attempts, 20: 11.0 -- rejections);
    # without the cap, 2^10 and 2^9 leave single fast envs at 1.0e-6 - 1.8e-6 and 2^8 costs 13.3 attempts
    # (profiles/r5/rodas5_calib.txt)
    ep_frac, ep_kmax = float(epc.get("frac", 0.5)), int(epc.get("kmax", 10 if integrator == "rodas4" else 16))
    if not (0.0 <= ep_frac <= 1.0) or not (0 <= ep_kmax <= 40):
        raise ValueError("endpoint_control: frac must lie in [0, 1] and kmax in [0, 40]")
    return ep_frac, ep_kmax


def _cooperative_threshold(integrator, coop_ok, coop):
    if coop is False:
        return 0.0
    if not coop_ok and coop is not None:
        raise ValueError("cooperative: needs integrator 'rodas4' / 'rodas5' on multistage_extraction with eq_exponent == 2")
    if coop is None or coop is True:
        # on by default under the fourth-order pair, whose heaviest envs take ~100 attempts; the fifth-order pair's take
        # ~45 and the launch does not wait for them (DEFAULT_COOP_THR counts attempts of the FOURTH-order pair)
        return DEFAULT_COOP_THR if (coop_ok and (integrator == "rodas4" or coop is True)) else 0.0
    thr = float(dict(coop).get("thr", DEFAULT_COOP_THR))
    if not (thr > 0.0 and np.isfinite(thr)):
        raise ValueError("cooperative: thr must be a positive finite number")
    return thr


def _default_substeps(integrator, model_id, dt, affine_A):
    if affine_A is not None:
        # affine models: keep |A|_inf * h <= 0.05 (RK4 local error ~ (|A| h)^5 / 120)
        return max(8, int(np.ceil(dt * np.abs(affine_A).sum(axis=1).max() / 0.05)))
    if integrator == "rk4g":  # the guard's calibration: 5 sub-steps per canonical dt = 26/60 (h <= 0.0867)
        return max(1, int(np.ceil(dt / (26.0 / 60.0 / 5) - 1e-9)))
    if integrator == "tsit5g":  # 2 steps per canonical dt (h <= 0.2167): the accuracy of RK4 x 5
        return max(1, int(np.ceil(dt / (26.0 / 60.0 / 2) - 1e-9)))
    d_sub = default_substeps(model_id, dt)
    if integrator == "cv8":
        h8 = DEFAULT_CV8_H.get(model_id)
        return max(1, int(np.ceil(dt / h8 - 1e-9))) if h8 else max(1, (d_sub + 3) // 4)
    return d_sub


def _default_tolerance(integrator, model_id, dt, integration_method, default_curve):
    d_tol = 1e-8 if integration_method == "jax" else DEFAULT_TOL.get(model_id, 1e-8)
    if model_id == M.CSTR and integration_method != "jax":
        d_tol = cstr_default_tol(dt)
    tab = {"rodas4": ROS4_TOL, "rodas5": ROS5_TOL}.get(integrator, {})
    if model_id not in tab:
        return d_tol
    # the global error of an env step is the SUM of the per-attempt budgets (~ attempts x tolerance), and the
    # attempts grow with dt: calibrated at dt = 1 (<= 7e-7 there and at 0.2), the same tolerance gave 1.5e-6
    # at dt = 2 and 3.9e-6 at dt = 5.  Scaled by the calibrated dt it stays at 7.0-7.4e-7 for dt =
    # 2, 5, 10 (tests/test_rodas4.py).
    d_tol = tab[model_id] / max(1.0, dt / ROS4_DT_CAL)
    # Round 6, the contract beyond the sample the tolerance was calibrated on (tools/rodas5_contract.py: 1e6 env
    # steps of 200-step random-action episodes, X0 / Y6 disturbed, eq_exponent 1.5 / 2 / 3, dt 0.2 ... 5, against
    # a 1e-13 solve): the reference's default curve stays within 1.4 x its tolerances everywhere; with
    # eq_exponent = 3 at dt = 5 two steps in 84,000 reached 3.5 x (slow liquid AND slow gas: the end-point
    # weights' coupling bound is the slope of the eq_exponent == 2 curve).  Not re-tuned on that sample: a
    # non-default curve simply runs the fifth-order pair at HALF the tolerance (1.6 x there, ~15 % more attempts)
    if integrator == "rodas5" and model_id == M.ME and not default_curve:
        d_tol *= ROS5_NONDEFAULT_CURVE
    return d_tol


class EnvSpec:
    """Numeric image of env_params (see module docstring).  The constructor is an ordered list of stages; each parses
    one group of keys and assigns one group of fields, and what a later stage needs that is not a field is handed on."""

    def __init__(self, env_params: dict):
        if not isinstance(env_params, dict):
            raise ValueError("env_params must be a dictionary")  # pcgym.py:40-41
        p = self.env_params = copy.deepcopy(env_params)
        a_low, a_high, o_low, o_high = self._parse_flags_and_spaces(p)
        reward_expr = self._parse_reward_kind(p)
        self._parse_grid(p)
        rhs_exprs, rhs_traced = self._parse_model(p, a_low, a_high)
        self._parse_setpoints(p)
        o_low, o_high = self._parse_disturbances(p, o_low, o_high)
        self._parse_a_delta(p)
        self._parse_noise_and_mask(p)
        self._parse_uncertainty(p, o_low, o_high)
        cons_exprs, cons_traced = self._parse_constraints(p)
        self._parse_reward_boxes()
        (self.integrator, self.substeps, self.rtol, self.atol, self.max_steps, self.ep_frac, self.ep_kmax,
         self.coop_thr) = integrator_plan(self.model.model_id, self.model.param_vector(), self.dt, self.nunc,
                                          self.integration_method, None if self.affine_AB is None else self.affine_AB[0],
                                          rhs_exprs is not None or rhs_traced is not None, p)
        self._compile_user_sources(rhs_exprs, rhs_traced, cons_exprs, cons_traced, reward_expr)
        for name, n, lim in (("nx", self.nx, abi.PCG_MAX_NX), ("na", self.na, abi.PCG_MAX_NA),
                             ("ndm", self.ndm, abi.PCG_MAX_NDM), ("nsp", self.nsp, abi.PCG_MAX_NSP)):
            if n > lim:
                raise ValueError(f"{name}={n} exceeds the build limit {lim}")

    def _parse_flags_and_spaces(self, p):
        """flags and spaces, pcgym.py:56-61, 68-92 -> the action and observation boxes as written: the model stage
        settles a_low / a_high / na (models without inputs), the uncertainty stage o_low / o_high (the slots behind x)"""
        self.a_delta, self.reference_compat = bool(p.get("a_delta", False)), bool(p.get("reference_compat", True))
        self.normalise_a, self.normalise_o = bool(p.get("normalise_a", True)), bool(p.get("normalise_o", True))
        a_low, a_high = _arr(p["a_space"]["low"]), _arr(p["a_space"]["high"])
        self.na_user = a_low.shape[0]
        return a_low, a_high, _arr(p["o_space"]["low"]), _arr(p["o_space"]["high"])

    def _parse_reward_kind(self, p):
        """reward kind, pcgym.py:94-103 -> the C expression of custom_reward {'expr': ...}, or None"""
        self.SP = p.get("SP")
        custom_reward, reward_expr, track = p.get("custom_reward"), None, None
        if isinstance(custom_reward, dict) and "expr" in custom_reward:
            # the callable form of custom_reward as a C expression (compiled into the kernel, see compile_expr)
            if set(custom_reward) - {"expr"}:
                raise ValueError("custom_reward {'expr': ...} takes no other keys")
            reward_expr, custom_reward = custom_reward["expr"], None
        if isinstance(custom_reward, dict):
            # A dict in place of the callable selects the in-kernel form of the custom_reward family every paper
            # script uses (pc-gym_paper/train_policies/*/custom_reward.py, constraint_showcase/custom_reward.py):
            #   {"kind": "sp_track", "R": 0.1, "R_u": 0.0, "box": {"T": [lower_bound, upper_bound]}}
            rt = dict(custom_reward)
            kind = rt.pop("kind", "sp_track")
            if kind not in ("sp_track", "cryst_moments"):
                raise ValueError("declarative custom_reward: kinds 'sp_track' and 'cryst_moments' are built")
            # 'cryst_moments' (crystalisation/cryst_train.py:17-48): sp_track on CV and Ln recomputed from the observed
            # moments, unit weights, R = 0.01
            track = {"R": float(rt.pop("R", 0.1 if kind == "sp_track" else 0.01)),
                     "R_u": float(rt.pop("R_u", 0.0)), "box": dict(rt.pop("box", {}) or {}),
                     "cryst": kind == "cryst_moments"}
            if rt:
                raise ValueError(f"declarative custom_reward: unknown keys {sorted(rt)}")
            if self.SP is None:
                raise ValueError("declarative custom_reward 'sp_track' needs set-points (SP)")
            custom_reward = None
        self.custom_reward, self.reward_track = custom_reward, track
        self.reward_batch = self.SP is None
        need = self.reward_batch and custom_reward is None and reward_expr is None  # the terminal reward reads both keys
        self.reward_states = list(p["reward_states"] if need else p.get("reward_states", []))
        self.maximise_reward = bool(p["maximise_reward"] if need else p.get("maximise_reward", True))
        return reward_expr

    # --- simulation grid, pcgym.py:105-111 ---------------------------------------------------------------------------
    def _parse_grid(self, p):
        self.N, self.tsim, self.x0 = int(p["N"]), p["tsim"], _arr(p["x0"])
        self.integration_method = p.get("integration_method", "hip")
        if self.integration_method not in ("hip", "casadi", "jax"):
            raise ValueError("integration_method must be 'hip' (or the reference's 'casadi'/'jax', "
                             "which map onto the HIP integrators)")
        self.dt = float(self.tsim) / self.N
        if not (1 < self.N <= abi.PCG_MAX_N):
            raise ValueError(f"N must be in (1, {abi.PCG_MAX_N}]")

    def _parse_model(self, p, a_low, a_high):
        """model, pcgym.py:127-158 -> (declarative rhs expressions | None, traced rhs | None) of a custom model"""
        affine = rhs_exprs = rhs_traced = None
        if p.get("custom_model") is not None:
            model, affine, rhs_exprs, rhs_traced = adopt_custom_model(p["custom_model"], p, a_low, a_high)
        else:
            model = M.get_model(p.get("model"))
            if model.affine_builder is not None:
                A, Bm, c = model.affine_builder(model.parameters)
                affine = (np.atleast_2d(np.asarray(A, dtype=_f64)), np.atleast_2d(np.asarray(Bm, dtype=_f64)),
                          np.asarray(c, dtype=_f64).reshape(-1))
        self.model, self.nx, self.nu_inputs = model, len(model.states), len(model.inputs)
        # Models without inputs (invariant_batch, coupled_oscillator; model_classes.py:200,282): the kernels carry
        # one dummy action the RHS ignores.  An empty a_space (the literal reading of info()["inputs"] == [])
        # and a 1-entry placeholder a_space (what runs through the reference unchanged) are both accepted.
        if self.nu_inputs == 0 and self.na_user in (0, 1):
            if self.na_user == 0:
                a_low = a_high = np.zeros(1)
            if affine is not None and affine[1].shape[1] == 0:  # affine model without inputs: B = 0 for the dummy
                affine = (affine[0], np.zeros((affine[0].shape[0], 1)), affine[2])
        elif self.nu_inputs != self.na_user:
            raise ValueError(f"a_space has {self.na_user} entries but the model has {self.nu_inputs} inputs")
        self.a_low, self.a_high, self.na = a_low, a_high, a_low.shape[0]
        self.affine_AB = affine
        return rhs_exprs, rhs_traced

    # --- set-points and reward indices -------------------------------------------------------------------------------
    def _parse_setpoints(self, p):
        states = self.model.states
        self.sp_keys = list(self.SP.keys()) if self.SP is not None else []
        self.nsp = len(self.sp_keys)
        self.sp_index = np.array([states.index(k) for k in self.sp_keys], dtype=np.int32)
        self.sp = np.zeros((self.nsp, self.N))
        for j, k in enumerate(self.sp_keys):
            v = _arr(self.SP[k])
            if v.shape[0] < self.N - 1:
                raise ValueError(f"SP['{k}'] has {v.shape[0]} entries, need at least N-1={self.N - 1}")
            n = min(v.shape[0], self.N)
            self.sp[j, :n] = v[:n]
            self.sp[j, n:] = v[n - 1]
        r_scale = p.get("r_scale", {}) or {}
        if self.reward_batch:
            names = [s for s in self.reward_states if str(s) in states]  # pcgym.py:519
            self.rew_index = np.array([states.index(s) for s in names], dtype=np.int32)
            self.r_scale = np.array([float(r_scale.get(s, 1)) for s in names], dtype=_f64)
        else:
            self.rew_index = np.zeros(0, dtype=np.int32)
            cryst = self.reward_track is not None and self.reward_track["cryst"]
            # cryst_train.py:37 has no r_scale
            self.r_scale = np.ones(self.nsp) if cryst else np.array([float(r_scale.get(k, 1)) for k in self.sp_keys], dtype=_f64)
            if cryst and (self.sp_keys != ["CV", "Ln"] or p.get("model") != "crystallization"):
                raise ValueError("custom_reward kind 'cryst_moments' needs model 'crystallization' and SP keys "
                                 "['CV', 'Ln'] (cryst_train.py:34-35)")
        self.nrew = self.rew_index.shape[0]
        # x0 normally carries the SP slots ([x | SP], README.md:47).  With only the nx physical
        # states the reference silently drops the SP slot from state/obs (pcgym.py:438 assigns into
        # an empty slice) -- its own KAT (tests/environment/test_make_env_custom_model.py:66-86) does so.
        if self.x0.shape[0] not in (self.nx + self.nsp, self.nx):
            raise ValueError(f"x0 must have nx+len(SP) = {self.nx + self.nsp} entries "
                             f"(states then SP slots) or nx = {self.nx}, got {self.x0.shape[0]}")
        self.nsp_obs = self.nsp if self.x0.shape[0] == self.nx + self.nsp else 0

    def _parse_disturbances(self, p, o_low, o_high):
        """disturbances, pcgym.py:167-199 -> the observation box over [states | SP | disturbances]"""
        self.disturbances = p.get("disturbances")
        mdist = list(self.model.disturbances) if self.disturbances is not None else []
        for k in self.disturbances or ():
            if k not in mdist:
                raise ValueError(f"disturbance '{k}' is not an input of model '{self.model.name}' "
                                 f"(available: {mdist})")
        self.ndm = len(mdist)
        # state slots follow the MODEL's disturbance order (pcgym.py:292-295, 392-398)
        self.d_keys = [k for k in mdist if k in self.disturbances]
        self.nd = len(self.d_keys)
        if self.disturbances is not None and self.nsp_obs != self.nsp:
            raise ValueError("disturbances need x0 to carry the SP slots (len(x0) == nx+len(SP))")
        self.d_slot = np.array([mdist.index(k) for k in self.d_keys], dtype=np.int32)
        self.d_sched = np.zeros((self.nd, self.N))
        for j, k in enumerate(self.d_keys):
            v = _arr(self.disturbances[k])
            if v.shape[0] < self.N:
                raise ValueError(f"disturbances['{k}'] has {v.shape[0]} entries, need N={self.N}")
            self.d_sched[j] = v[:self.N]
        # an unconfigured disturbance input reads the parameter of the same name (a KeyError when there is none)
        pnames = list(self.model.parameters.keys())
        self.d_default = np.array([float(self.model.parameters[str(k)]) for k in mdist])
        self.d_param_index = np.array([pnames.index(str(k)) for k in mdist], dtype=np.int32)
        if self.disturbances is not None:
            o_low = np.concatenate([o_low, _arr(p["disturbance_bounds"]["low"])])
            o_high = np.concatenate([o_high, _arr(p["disturbance_bounds"]["high"])])
        self.nu = self.na + self.ndm
        nst = self.nx + self.nsp_obs + self.nd
        if o_low.shape[0] != nst or o_high.shape[0] != nst:
            raise ValueError(f"o_space (+disturbance_bounds) must have {nst} entries "
                             f"[states | SP | disturbances], got {o_low.shape[0]}")
        gd = p.get("gaussian_disturbances")
        self.gauss = gd is not None
        for k in gd or ():
            if k not in self.d_keys:
                raise ValueError(f"gaussian_disturbances['{k}'] needs a matching disturbances entry")
        self.d_sigma = np.array([float(gd.get(k, 0.0)) for k in self.d_keys]) if self.gauss else np.zeros(self.nd)
        self.d_clip_lo = o_low[self.nx + self.nsp_obs:].copy()
        self.d_clip_hi = o_high[self.nx + self.nsp_obs:].copy()
        return o_low, o_high

    # --- a_delta, pcgym.py:57-58, 376-383 ----------------------------------------------------------------------------
    def _parse_a_delta(self, p):
        self.a_0 = np.broadcast_to(_arr(p["a_0"]), (self.na,)).astype(_f64).copy() if self.a_delta else np.zeros(self.na)
        self.a_act_low = _arr(p["a_space_act"]["low"]) if self.a_delta else np.full(self.na, -np.inf)
        self.a_act_high = _arr(p["a_space_act"]["high"]) if self.a_delta else np.full(self.na, np.inf)

    # --- noise, pcgym.py:63-66, 453-466; partial observation, pcgym.py:208-211 ---------------------------------------
    def _parse_noise_and_mask(self, p):
        self.noise = bool(p.get("noise", False))
        self.noise_pct = np.zeros(self.nx)
        npct = p.get("noise_percentage")
        if self.noise and isinstance(npct, dict):
            for i, s in enumerate(self.model.states):
                if s in npct:
                    self.noise_pct[i] = float(npct[s])
        elif self.noise and npct is not None:
            self.noise_pct[:] = float(npct)
        self.partial_observation = p.get("partial_observation")
        self.obs_mask = None
        if self.partial_observation:
            self.obs_mask = np.array([1 if s in self.partial_observation else 0 for s in self.model.states], dtype=np.uint8)

    def _parse_uncertainty(self, p, o_low, o_high):
        """uncertainty, pcgym.py:212-253, 284-316.  "x0": fractions per state (reset-time initial-state uncertainty); any
        other key names a model parameter sampled per env at reset and appended to the state/observation
        [x | SP | d | unc].  Settles nobs / o_low / o_high."""
        up = p.get("uncertainty_percentages")
        emp = p.get("empirical_distribution") if up is None else None  # the reference's precedence (pcgym.py:218-229)
        self.unc_empirical = emp is not None
        self.unc_inert = []  # quirk Q15: empirical_distribution['x0'] -- sampled and observed, never applied
        if emp is not None:
            if "x0" in emp:
                # The reference treats 'x0' like every other key of the dict (pcgym.py:311-316): np.random.choice(table) --
                # which needs a 1-D table -- setattr(model, 'x0', sample), and the sample appended to the observation.
                # The model object's x0 attribute is read by nobody (the env starts from env_params['x0'], :282-284), so
                # the sample is OBSERVED but never applied: one more slot behind the state, no effect on the dynamics.
                if np.asarray(emp["x0"]).ndim != 1:
                    raise ValueError("a must be 1-dimensional (empirical_distribution['x0']: np.random.choice, pcgym.py:313)")
                self.unc_inert = ["x0"]
            up = {k: 0.0 for k in emp}  # shares the bookkeeping below; the percentages are unused
        dist = p.get("distribution", "uniform")
        if up is not None and dist not in ("uniform", "normal"):
            raise ValueError("distribution must be 'uniform' or 'normal'")
        self.x0_normal = up is not None and dist == "normal"
        self.x0_unc = None
        if up is not None and "x0" in up and emp is None:
            # the reference walks "for idx, uncertainty in enumerate(x0_uncertainty)" (pcgym.py:286-288): a
            # sequence gives per-state fractions; a dict (tests/models/test_model.py:99) yields its KEYS
            xu = _arr(list(up["x0"]))
            self.x0_unc = np.zeros(self.nx)
            n = min(self.nx, xu.shape[0])
            self.x0_unc[:n] = xu[:n]
        self.unc_keys = [k for k in up or () if k != "x0" or k in self.unc_inert]
        names = list(self.model.parameters.keys())
        if self.unc_keys and self.model.model_id in (M.AFFINE, M.USER):
            raise ValueError("parameter uncertainty is not available for affine / custom models")
        for k in self.unc_keys:
            if k not in names and k not in self.unc_inert:
                raise ValueError(f"uncertain parameter '{k}' is not a parameter of model "
                                 f"'{self.model.name}' (available: {names})")
        # disturbances together with parameter uncertainty: the reference writes the disturbance slots at a
        # different offset in step() than in reset() (pcgym.py:298,310 vs 409-410, quirk Q11); here the reset
        # layout [x | SP | d | unc] holds in both
        self.nunc = len(self.unc_keys)
        if self.nunc > abi.PCG_MAX_NUNC:
            raise ValueError(f"at most {abi.PCG_MAX_NUNC} uncertain parameters are supported")
        # (an inert key takes the first index past the model's parameters: the kernels substitute it into
        # nothing, pcg_abi_cfg.hip accepts it for empirical tables only)
        self.unc_index = np.array([names.index(k) if k in names else len(names) for k in self.unc_keys], dtype=np.int32)
        self.unc_pct = np.array([float(up[k]) for k in self.unc_keys], dtype=_f64)
        self.unc_emp, self.unc_emp_off = _empirical_tables(emp, self.unc_keys)
        self.nobs = self.nx + self.nsp_obs + self.nd + self.nunc
        if self.nunc:
            ub = p["uncertainty_bounds"]
            o_low, o_high = np.concatenate([o_low, _arr(ub["low"])]), np.concatenate([o_high, _arr(ub["high"])])
            if o_low.shape[0] != self.nobs or o_high.shape[0] != self.nobs:
                raise ValueError(f"uncertainty_bounds must have {self.nunc} entries (one per uncertain parameter)")
        self.o_low, self.o_high = o_low, o_high

    def _parse_constraints(self, p):
        """constraints, pcgym.py:113-125 -> (constraint C expressions | None, traced constraint rows | None).  A callable
        sees [x | SP | d] and u, the width the reference hands it; the uncertain-parameter columns of con_A are zero."""
        cons = p.get("constraints")
        self.constraint_active = cons is not None
        self.done_on_constraint = bool(p["done_on_cons_vio"]) if cons is not None else False
        self.r_penalty = bool(p["r_penalty"]) if cons is not None else False
        nst = self.nobs - self.nunc
        exprs = traced = None
        if cons is None:
            A, b = np.zeros((0, nst + self.nu)), np.zeros(0)
        elif isinstance(cons, dict) and "expr" in cons:
            # non-affine g(x,u) as C expressions, one per row (compiled into the kernel, see compile_expr)
            exprs = [cons["expr"]] if isinstance(cons["expr"], str) else list(cons["expr"])
            A, b = np.zeros((len(exprs), nst + self.nu)), np.zeros(len(exprs))
        elif isinstance(cons, dict):
            A, b = np.atleast_2d(np.asarray(cons["A"], dtype=_f64)), _arr(cons["b"])
        elif callable(cons):
            A, b, traced = _probe_constraint(cons, np.concatenate([self.x0, self.d_sched[:, 0]]), self.nu, self.a_low, self.a_high)
        else:
            raise ValueError("constraints must be a callable g(x,u) or {'A':..., 'b':...}")
        if A.shape[1] != nst + self.nu:
            raise ValueError(f"constraint rows must have Nobs+Nu = {nst + self.nu} columns")
        # columns [x | SP | d | unc | u]: no row reads an uncertain parameter (the empty matrix of a plan without rows has
        # never carried those columns)
        pad = np.zeros((A.shape[0], self.nunc if A.shape[0] else 0))
        self.con_A = np.ascontiguousarray(np.concatenate([A[:, :nst], pad, A[:, nst:]], axis=1))
        self.con_b = np.ascontiguousarray(b)
        self.ncon = A.shape[0]
        if self.ncon > abi.PCG_MAX_NCON:
            raise ValueError(f"at most {abi.PCG_MAX_NCON} constraint rows are supported")
        if cons is not None and self.reference_compat and self.normalise_a and self.nu != self.na and self.na != 1:
            # the reference itself raises here (numpy broadcast of a_space against uk, pcgym.py:597-600)
            raise ValueError("operands could not be broadcast together: the reference cannot "
                             "combine normalise_a, disturbances and constraints for na>1 "
                             "(pcgym.py:597-600); set reference_compat=False or normalise_a=False")
        return exprs, traced

    # --- declarative tracking reward: state boxes of the violation term ----------------------------------------------
    def _parse_reward_boxes(self):
        box = self.reward_track["box"] if self.reward_track is not None else {}
        if self.reward_track is not None and self.nd:
            raise ValueError("declarative custom_reward with disturbances is not supported (the reference's "
                             "callables broadcast uk[Nu+Nd] against a_space[Nu])")
        if len(box) > abi.PCG_MAX_RBOX:
            raise ValueError(f"at most {abi.PCG_MAX_RBOX} boxed states are supported")
        for k in box:
            if k not in self.model.states:
                raise ValueError(f"custom_reward box: '{k}' is not a state of model '{self.model.name}'")
        self.rew_box_index = np.array([self.model.states.index(k) for k in box], dtype=np.int32)
        # [lower_bound, upper_bound] in the order the reference's con_reward unpacks them
        # (constraint_showcase/custom_reward.py:45) -- not sorted: its own {'T': [327, 321]} stays as written
        self.rew_box_lo = np.array([float(box[k][0]) for k in box], dtype=_f64)
        self.rew_box_hi = np.array([float(box[k][1]) for k in box], dtype=_f64)

    # --- user expressions -> C source --------------------------------------------------------------------------------
    def _compile_user_sources(self, rhs_exprs, rhs_traced, cons_exprs, cons_traced, reward_expr):
        info = self.model.info()
        self.user_rhs_src = self.user_cons_src = self.user_reward_src = None
        if rhs_exprs is not None:
            # disturbance inputs -> u[na + j] when the env feeds them (else their parameter value, like the reference
            # models' "if u.size == ..." branches)
            rhs, aux = rhs_exprs
            names = _name_map(info, "x", params=self.model.parameters, dist_at=self.na if self.ndm else None)
            lines, local = [], set()
            for k, e in aux.items():
                lines.append(f"  const double {k} = (double)({compile_expr(e, names, set(), local, f'custom_model aux[{k!r}]')});")
                local.add(k)
            rows = [compile_expr(e, names, set(), local, f"custom_model rhs[{i}]") for i, e in enumerate(rhs)]
            self.user_rhs_src = "\n".join(lines + [_assign_lines("dx", rows)])
        elif rhs_traced is not None:  # a Python model recorded by trace_callable
            self.user_rhs_src = _assign_lines("dx", rhs_traced)
        if cons_exprs:
            sp = [(k, f"x[{self.nx + j}]") for j, k in enumerate(self.sp_keys[:self.nsp_obs])]
            names = _name_map(info, "x", sp_lvalues=sp)
            self.user_cons_src = _assign_lines("g", [compile_expr(e, names, {"x", "u"}, set(), f"constraints['expr'][{r}]")
                                                     for r, e in enumerate(cons_exprs)])
        elif cons_traced:  # a Python callable recorded by trace_callable (already over x[] / u[])
            self.user_cons_src = _assign_lines("g", cons_traced)
        if reward_expr is not None:
            names = _name_map(info, "o", sp_lvalues=[(k, f"sp[{j}]") for j, k in enumerate(self.sp_keys)])
            self.user_reward_src = compile_expr(reward_expr, names, {"o", "x", "u", "sp"}, {"violated", "t", "N"},
                                                "custom_reward['expr']")

    # ------------------------------------------------------------------------------
    def x0_full(self):
        """reference reset state [x0 | SP slots | d[:,0] | nominal uncertain parameters] (pcgym.py:284-316)."""
        pv = self.model.param_vector()
        unc = np.array([pv[i] if i < len(pv) else 0.0 for i in self.unc_index], dtype=_f64)
        return np.concatenate([self.x0, self.d_sched[:, 0], unc])

    def param_vector(self):
        if self.model.model_id == M.AFFINE:
            A, Bm, c = self.affine_AB
            return np.concatenate([A.reshape(-1), Bm.reshape(-1), c.reshape(-1)])
        return np.array(self.model.param_vector(), dtype=_f64)

    def flags(self):
        track = self.reward_track is not None
        bits = ((abi.PCG_F_NORMALISE_A, self.normalise_a), (abi.PCG_F_NORMALISE_O, self.normalise_o),
                (abi.PCG_F_A_DELTA, self.a_delta and self.normalise_a),  # pcgym.py:376
                (abi.PCG_F_R_PENALTY, self.r_penalty), (abi.PCG_F_DONE_ON_CONS, self.done_on_constraint),
                (abi.PCG_F_NOISE, self.noise), (abi.PCG_F_REWARD_BATCH, self.reward_batch), (abi.PCG_F_REWARD_TRACK, track),
                (abi.PCG_F_REWARD_CRYST, track and self.reward_track["cryst"]), (abi.PCG_F_MAXIMISE, self.maximise_reward),
                (abi.PCG_F_REF_COMPAT, self.reference_compat), (abi.PCG_F_GAUSS_DIST, self.gauss),
                (abi.PCG_F_X0_NORMAL, self.x0_normal), (abi.PCG_F_UNC_EMPIRICAL, self.unc_empirical and self.nunc))
        return sum(bit for bit, on in bits if on)

    def to_cfg(self):
        """-> (pcg_env_cfg, keepalive list).  The arrays must outlive the call that reads the cfg."""
        keep = []

        def ptr(a, dtype=_f64):
            if a is None or a.size == 0:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            keep.append(a)
            return a.ctypes.data_as(C.POINTER(_CTYPE[dtype]))

        i32 = np.int32
        params = self.param_vector()
        cfg = abi.pcg_env_cfg()
        cfg.model_id = self.model.model_id
        cfg.integrator_id = _INTEGRATOR_ID[self.integrator]
        cfg.ep_frac, cfg.ep_kmax, cfg.coop_thr = self.ep_frac, self.ep_kmax, self.coop_thr
        cfg.nx, cfg.na, cfg.ndm, cfg.nd = self.nx, self.na, self.ndm, self.nd
        cfg.nsp, cfg.ncon, cfg.nrew, cfg.N = self.nsp, self.ncon, self.nrew, self.N
        cfg.nsp_obs, cfg.nunc = self.nsp_obs, self.nunc
        cfg.substeps, cfg.max_steps = self.substeps, self.max_steps
        cfg.flags = self.flags()
        cfg.n_params = params.shape[0]
        cfg.dt, cfg.rtol, cfg.atol = self.dt, self.rtol, self.atol
        # (the keep-alive list follows the order of these calls)
        cfg.params, cfg.x0, cfg.x0_unc = ptr(params), ptr(self.x0), ptr(self.x0_unc)
        cfg.a_low, cfg.a_high = ptr(self.a_low), ptr(self.a_high)
        cfg.a_act_low, cfg.a_act_high, cfg.a_0 = ptr(self.a_act_low), ptr(self.a_act_high), ptr(self.a_0)
        cfg.o_low, cfg.o_high, cfg.obs_mask = ptr(self.o_low), ptr(self.o_high), ptr(self.obs_mask, np.uint8)
        cfg.sp_index, cfg.sp, cfg.r_scale = ptr(self.sp_index, i32), ptr(self.sp), ptr(self.r_scale)
        cfg.rew_index, cfg.d_slot = ptr(self.rew_index, i32), ptr(self.d_slot, i32)
        cfg.d_sched, cfg.d_default = ptr(self.d_sched), ptr(self.d_default)
        cfg.d_param_index = ptr(self.d_param_index, i32)  # empty, hence NULL, unless ndm > 0
        cfg.d_sigma, cfg.d_clip_lo, cfg.d_clip_hi = ptr(self.d_sigma), ptr(self.d_clip_lo), ptr(self.d_clip_hi)
        cfg.con_A, cfg.con_b, cfg.noise_pct = ptr(self.con_A), ptr(self.con_b), ptr(self.noise_pct)
        cfg.unc_index, cfg.unc_pct = ptr(self.unc_index, i32), ptr(self.unc_pct)
        cfg.unc_emp, cfg.unc_emp_off = ptr(self.unc_emp), ptr(self.unc_emp_off, i32)
        if self.reward_track is not None:
            cfg.rew_R_du, cfg.rew_R_u = self.reward_track["R"], self.reward_track["R_u"]
            cfg.rew_nbox = len(self.rew_box_index)
            cfg.rew_box_index = ptr(self.rew_box_index, i32)
            cfg.rew_box_lo, cfg.rew_box_hi = ptr(self.rew_box_lo), ptr(self.rew_box_hi)
        sources = (self.user_rhs_src, self.user_cons_src, self.user_reward_src)
        if any(s is not None for s in sources):
            cfg.user_rhs_src, cfg.user_cons_src, cfg.user_reward_src = (None if s is None else s.encode() for s in sources)
            cfg.jit_include_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc").encode()
        return cfg, keep


def _empirical_tables(emp, keys):
    """empirical_distribution (pcgym.py:226-232) -> (the tables of ``keys`` back to back, their offsets)"""
    if emp is None or not keys:
        return np.zeros(0), np.zeros(1, dtype=np.int32)
    tabs = [_arr(emp[k]) for k in keys]
    if any(t.size == 0 for t in tabs):
        raise ValueError("every empirical_distribution entry needs at least one sample")
    table = np.concatenate(tabs)
    if table.size > abi.PCG_MAX_EMP:
        raise ValueError(f"at most {abi.PCG_MAX_EMP} empirical samples in total are supported")
    return table, np.concatenate([[0], np.cumsum([t.size for t in tabs])]).astype(np.int32)


def _probe_constraint(cons, x_ref, nu, a_low, a_high):
    """a callable g(x, u) over x = [states | SP | disturbances] around ``x_ref`` -> (A, b, None) when it is affine,
    else (zero rows, zero b, its traced C expressions).  One generator serves both attempts: stateful or recording
    callables observe the sequence (three affine probe points, then four physical ones)."""
    nst, na = x_ref.shape[0], a_low.shape[0]
    rng = np.random.default_rng(7)
    pts = []
    for _ in range(3):
        xs = x_ref * (1 + 0.1 * rng.uniform(-1, 1, nst)) + 0.01 * rng.uniform(-1, 1, nst)
        us = rng.uniform(-1, 1, nu)
        pts.append(np.concatenate([xs, us]))
    try:
        A, c = probe_affine(cons, [nst, nu], pts, "constraints")
        return A, -c, None
    except ValueError as not_affine:
        # not affine: record the callable's arithmetic as C expressions (trace_callable) and compile those
        # into the kernel, exactly as if the user had written {'expr': [...]}
        phys = []
        for _ in range(4):  # probe points in physical units: the state box and the action box
            xs = x_ref * (1 + 0.05 * rng.uniform(-1, 1, nst))
            us = np.resize(a_low + rng.uniform(0, 1, na) * (a_high - a_low), nu)
            phys.append(np.concatenate([xs, us]))
        try:
            traced = trace_callable(cons, [nst, nu], phys, "constraints")
        except ValueError as not_traceable:
            raise ValueError(f"{not_affine}; and {not_traceable}") from None
        return np.zeros((len(traced), nst + nu)), np.zeros(len(traced)), traced
