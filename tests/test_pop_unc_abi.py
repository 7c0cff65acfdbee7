"""CPU: pcg_rollout_policy_pop_unc (the fused closed-loop rollout of a policy population on plans with per-env parameters) --
declaration, export, ctypes signature, the ABI version -- and fused_pop_unc_ok / evaluate_population(fused_unc=True) without a
GPU.  The device side -- the kernels against the oracle, the members, the returns, shards, refusals, stream capture -- is
tests/test_gpu_pop_unc_rollout.py."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

import scenarios as SC
from pcgym_amd import EnvSpec, PolicyPopulation
from pcgym_amd import _abi as abi
from pcgym_amd import _lib
from test_pop_rollout_abi import _members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pcgym_hip.h")).read()
NAME = "pcg_rollout_policy_pop_unc"
UNC = dict(uncertainty_percentages={"q": 0.03}, distribution="uniform",
           uncertainty_bounds={"low": np.array([90.0]), "high": np.array([110.0])})


def _spec(scen, **over):
    p = copy.deepcopy(SC.scenarios()[scen]["env_params"])
    p.update(over)
    return EnvSpec(p)


def _params_of(fn):
    m = re.search(r"PCG_API (\w+) %s\((.*?)\);" % fn, HDR, re.S)
    assert m and m.group(1) == "int", fn
    return [p_.strip() for p_ in m.group(2).replace("\n", " ").split(",")]


def test_header_declares_and_library_exports():
    assert abi.PCG_ABI_VERSION == 16 and _lib.load().pcg_version() == 16  # additive
    assert re.search(r"#define PCG_ABI_VERSION 16\b", HDR)
    assert len(re.findall(r"PCG_API int %s\(" % NAME, HDR)) == 1
    assert abi.EXPORTS.count(NAME) == 1 and len(set(abi.EXPORTS)) == len(abi.EXPORTS)
    assert C.CDLL(_lib.LIB_PATH)[NAME] is not None  # (AttributeError if the library does not export it)
    doc = HDR[:HDR.index("PCG_API int %s(" % NAME)].rsplit("/*", 1)[1]
    # the contract the GPU tests assert: to rounding against the single-policy call, to the bit against itself, the order
    for phrase in ("TO ROUNDING, not", "bit for bit reproducible", "io->p_unc", "PCG_E_UNSUPPORTED", "Nobs counts the parameter slots",
                   "safe under stream capture", "pcg_rollout_policy_pop keeps refusing"):
        assert phrase in doc, phrase
    order = [doc.index(s) for s in ("1. plan, io and the handle", "2. PCG_E_UNSUPPORTED", "3. PCG_E_DIM", "4. the slices and gamma", "5. T / t0")]
    assert order == sorted(order)
    # the two "Not here" sentences no longer name per-env parameters as out of scope
    pop_doc = HDR[:HDR.index("PCG_API int pcg_rollout_policy_pop(")].rsplit("/*", 1)[1]
    assert "pcg_rollout_policy_pop_unc" in pop_doc.rsplit("Not here:", 1)[1]
    kern = open(os.path.join(ROOT, "pc-gym_amd", "csrc", "pcg_rollout_pop.hpp")).read()
    assert "pcg_rollout_pop_unc.hpp" in kern.split("#pragma once")[0].rsplit("Out of scope:", 1)[1]


def test_ctypes_signature_equals_the_header():
    lib = _lib.load()
    vp = C.c_void_p
    ctype = {"const double*": vp, "double*": vp, "void*": vp, "pcg_plan*": vp, "const pcg_buffers*": C.POINTER(abi.pcg_buffers),
             "const pcg_policy_pop*": vp, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double}
    params = _params_of(NAME)
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int
    assert [ctype[re.sub(r"\s*\w+$", "", p_).strip()] for p_ in params] == list(fn.argtypes)
    # the same signature as pcg_rollout_policy_pop: types and names
    assert params == _params_of("pcg_rollout_policy_pop")
    assert list(fn.argtypes) == list(lib.pcg_rollout_policy_pop.argtypes)


def test_fused_pop_unc_ok_says_which_calls_the_kernel_takes():
    from pcgym_amd.policy import fused_pop_ok, fused_pop_unc_ok
    from pcgym_amd import rollout
    from test_policy_jit_plans import _chemostat

    assert rollout.fused_pop_unc_ok is fused_pop_unc_ok  # (exported where fused_pop_ok is)
    ok = _spec("cstr_canonical", integrator="rk4", **UNC)
    assert ok.nunc == 1 and not ok.ncon
    for dtype in ("float64", "float32"):
        pop = PolicyPopulation.from_policies(pop_members(ok, dtype) * 2)
        assert pop.dtype == dtype
        assert fused_pop_unc_ok(ok, pop, 64) and fused_pop_unc_ok(ok, pop, 128) and fused_pop_unc_ok(ok, pop, 1024), dtype
        assert not fused_pop_ok(ok, pop, 64)  # (pcg_rollout_policy_pop keeps refusing the plan)
        # G = 96 (no whole waves), and what is smaller than a wave
        assert not fused_pop_unc_ok(ok, pop, 96) and not fused_pop_unc_ok(ok, pop, 32) and not fused_pop_unc_ok(ok, pop, 0), dtype
        assert not fused_pop_unc_ok(ok, pop.member(0), 64)  # (a single policy is not a population)
        # no parameters
        plain = _spec("cstr_canonical", integrator="rk4")
        assert not plain.nunc and not fused_pop_unc_ok(plain, PolicyPopulation.from_policies(pop_members(plain, dtype)), 64)
        # rows
        both = _spec("cstr_cons_pen_norm", integrator="rk4", **UNC)
        assert both.nunc and both.ncon and not fused_pop_unc_ok(both, PolicyPopulation.from_policies(pop_members(both, dtype)), 64)
        # another integrator (cv8 refuses per-env parameters when the plan is made: the rule is on the spec's integrator)
        for integ in ("cv8", "dopri5"):
            other = copy.copy(ok)
            other.integrator = integ
            assert not fused_pop_unc_ok(other, pop, 64), integ
        # a user model: its plan runs from a run-time compiled module (which refuses per-env parameters beside)
        cs = EnvSpec(_chemostat(integrator="rk4"))
        assert cs.user_rhs_src is not None and not fused_pop_unc_ok(cs, PolicyPopulation.from_policies(pop_members(cs, dtype)), 64)
        # a wrong n_in that forgets the parameter slots
        short = PolicyPopulation.from_policies(pop_members(ok, dtype, n_in=ok.nobs - ok.nunc))
        assert not fused_pop_unc_ok(ok, short, 64)


def pop_members(spec, dtype, n_in=None):
    from pcgym_amd import MLPPolicy

    mem = _members(2, [spec.nobs if n_in is None else n_in, 16, spec.na])
    if dtype == "float64":
        return mem
    return [MLPPolicy(q.weights, q.biases, activation=q.activation, out_map=q.out_map, out_low=q.out_low, out_high=q.out_high,
                      dtype="float32") for q in mem]


class _NoDevice:
    """a stand-in VecEnv that fails the test as soon as anything but the plan's description is asked of it"""

    def __init__(self, spec, B=256, env_offset=0):
        self.__dict__.update(spec=spec, B=B, env_offset=env_offset, per_env_t=False)

    def __getattr__(self, name):
        raise AssertionError(f"evaluate_population touched env.{name} before refusing")


def test_evaluate_population_refuses_fused_unc_before_anything_touches_a_device():
    from pcgym_amd import evaluate_population

    ok = _spec("cstr_canonical", integrator="rk4", **UNC)
    plain = _spec("cstr_canonical", integrator="rk4")
    both = _spec("cstr_cons_pen_norm", integrator="rk4", **UNC)
    pop_of = lambda s, n_in=None: PolicyPopulation.from_policies(pop_members(s, "float64", n_in) * 2)  # noqa: E731  (four members)
    cases = [("no parameters", plain, pop_of(plain), 64, 0, {}),
             ("rows", both, pop_of(both), 64, 0, {}),
             ("G = 96", ok, pop_of(ok), 96, 0, {}),
             ("offset 32", ok, pop_of(ok), 64, 32, {}),
             ("n_in without the parameter slots", ok, pop_of(ok, ok.nobs - ok.nunc), 64, 0, {}),
             ("a single policy", ok, pop_of(ok).member(0), 64, 0, {}),
             ("fused=False", ok, pop_of(ok), 64, 0, dict(fused=False))]
    for what, spec, pop, g, off, kw in cases:
        with pytest.raises(ValueError):  # (what)
            evaluate_population(_NoDevice(spec, env_offset=off), pop, g, fused_unc=True, **kw)
