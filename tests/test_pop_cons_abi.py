"""CPU: pcg_rollout_policy_pop_cons (the fused closed-loop rollout of a policy population on plans with constraint rows, with
the per-env violation statistics) -- declaration, export, ctypes signature, the ABI version -- and fused_pop_cons_ok /
evaluate_population(fused=True) without a GPU.  The device side -- the kernels against the per-step route and the oracle, the
statistics, members, shards, refusals, stream capture -- is tests/test_gpu_pop_cons_rollout.py."""
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
from test_pop_unc_abi import UNC, _NoDevice, pop_members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pcgym_hip.h")).read()
NAME = "pcg_rollout_policy_pop_cons"


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
    # the contract the GPU tests assert, the two statistics' definitions and the order of the refusals
    for phrase in ("bit for bit", "pcg_rollout_policy_cons", "nviol_out", "gmax_out", "gmax = (g > gmax) ? g : gmax", "a NaN row leaves",
                   "counts in neither", "io->g_pre", "keeps stepping", "safe under stream capture",
                   "pcg_rollout_policy_pop keeps refusing"):
        assert phrase in doc, phrase
    order = [doc.index(s) for s in ("1. plan, io and the handle", "2. PCG_E_UNSUPPORTED for ncon == 0", "3. PCG_E_UNSUPPORTED for nunc > 0",
                                    "4. PCG_E_UNSUPPORTED for a plan with run-time compiled code", "5. PCG_E_DIM", "6. the slices and gamma",
                                    "7. T / t0")]
    assert order == sorted(order)
    # the "Not here" / "Out of scope" sentences of the plain population call point here
    pop_doc = HDR[:HDR.index("PCG_API int pcg_rollout_policy_pop(")].rsplit("/*", 1)[1]
    assert NAME in pop_doc.rsplit("Not here:", 1)[1]
    kern = open(os.path.join(ROOT, "pc-gym_amd", "csrc", "pcg_rollout_pop.hpp")).read()
    assert "pcg_rollout_pop_cons.hpp" in kern.split("#pragma once")[0].rsplit("Out of scope:", 1)[1]
    new = open(os.path.join(ROOT, "pc-gym_amd", "csrc", "pcg_rollout_pop_cons.hpp")).read().split("#pragma once")[0]
    assert "gmax = (g > gmax) ? g : gmax" in new and "J = J + disc * r" in new and "disc = disc * gamma" in new


def test_ctypes_signature_equals_the_header():
    lib = _lib.load()
    vp = C.c_void_p
    ctype = {"const double*": vp, "double*": vp, "void*": vp, "uint8_t*": vp, "int32_t*": vp, "pcg_plan*": vp,
             "const pcg_buffers*": C.POINTER(abi.pcg_buffers), "const pcg_policy_pop*": vp, "int32_t": C.c_int32, "int64_t": C.c_int64,
             "uint64_t": C.c_uint64, "double": C.c_double}
    params = _params_of(NAME)
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int
    assert [ctype[re.sub(r"\s*\w+$", "", p_).strip()] for p_ in params] == list(fn.argtypes)
    # pcg_rollout_policy_pop's parameters, types and names, with the five g / viol parameters of pcg_rollout_policy_cons after
    # record_next_action and the two statistics after ret_out
    base = _params_of("pcg_rollout_policy_pop")
    cons = _params_of("pcg_rollout_policy_cons")
    five = cons[cons.index("int32_t record_next_action") + 1:-2]
    assert [re.search(r"(\w+)$", p_).group(1) for p_ in five] == ["g_seq", "g_step_stride", "g_comp_stride", "viol_seq", "viol_step_stride"]
    i, j = base.index("int32_t record_next_action") + 1, base.index("double* ret_out") + 1
    assert params == base[:i] + five + base[i:j] + ["int32_t* nviol_out", "double* gmax_out"] + base[j:]


def _expr_params():
    """cstr_cons_pen_norm with its constraint given as a C expression instead of rows"""
    p = copy.deepcopy(SC.scenarios()["cstr_cons_pen_norm"]["env_params"])
    p.update(integrator="rk4", constraints={"expr": ["T - 327.0"]})
    return p


def test_fused_pop_cons_ok_says_which_calls_the_kernel_takes():
    from pcgym_amd import rollout
    from pcgym_amd.policy import fused_pop_cons_ok, fused_pop_ok
    from test_policy_jit_plans import _chemostat

    assert rollout.fused_pop_cons_ok is fused_pop_cons_ok  # (exported where fused_pop_ok is)
    for dtype in ("float64", "float32"):
        for integ in ("rk4", "cv8"):
            ok = _spec("cstr_cons_pen_norm", integrator=integ)
            assert ok.ncon >= 1 and not ok.nunc and ok.user_cons_src is None
            pop = PolicyPopulation.from_policies(pop_members(ok, dtype) * 2)
            assert pop.dtype == dtype
            assert fused_pop_cons_ok(ok, pop, 64) and fused_pop_cons_ok(ok, pop, 128) and fused_pop_cons_ok(ok, pop, 1024), (dtype, integ)
            assert not fused_pop_ok(ok, pop, 64)  # (pcg_rollout_policy_pop keeps refusing the plan)
            # G = 96 (no whole waves), and what is smaller than a wave
            assert not fused_pop_cons_ok(ok, pop, 96) and not fused_pop_cons_ok(ok, pop, 32) and not fused_pop_cons_ok(ok, pop, 0)
            assert not fused_pop_cons_ok(ok, pop.member(0), 64)  # (a single policy is not a population)
        ok = _spec("cstr_cons_pen_norm", integrator="rk4")
        pop = PolicyPopulation.from_policies(pop_members(ok, dtype) * 2)
        # no rows
        plain = _spec("cstr_canonical", integrator="rk4")
        assert not plain.ncon and not fused_pop_cons_ok(plain, PolicyPopulation.from_policies(pop_members(plain, dtype)), 64)
        # rows plus per-env parameters
        both = _spec("cstr_cons_pen_norm", integrator="rk4", **UNC)
        assert both.nunc and both.ncon and not fused_pop_cons_ok(both, PolicyPopulation.from_policies(pop_members(both, dtype)), 64)
        # another integrator
        other = copy.copy(ok)
        other.integrator = "dopri5"
        assert not fused_pop_cons_ok(other, pop, 64)
        # a constraint expression: run-time compiled
        ex = EnvSpec(_expr_params())
        assert ex.user_cons_src and not fused_pop_cons_ok(ex, PolicyPopulation.from_policies(pop_members(ex, dtype)), 64)
        # a user model with affine rows: run-time compiled as well
        cs = EnvSpec(_chemostat(integrator="rk4"))
        row = {"A": np.ones((1, cs.nobs - cs.nunc + cs.nu)), "b": np.array([1.0])}
        cs = EnvSpec(_chemostat(integrator="rk4", constraints=row, done_on_cons_vio=False, r_penalty=True))
        assert cs.ncon == 1 and cs.user_rhs_src is not None and cs.user_cons_src is None
        assert not fused_pop_cons_ok(cs, PolicyPopulation.from_policies(pop_members(cs, dtype)), 64)
        # a wrong n_in
        short = PolicyPopulation.from_policies(pop_members(ok, dtype, n_in=ok.nobs + 1))
        assert not fused_pop_cons_ok(ok, short, 64)


def test_evaluate_population_refuses_fused_before_anything_touches_a_device():
    from pcgym_amd import evaluate_population

    ok = _spec("cstr_cons_pen_norm", integrator="rk4")
    plain = _spec("cstr_canonical", integrator="rk4")
    both = _spec("cstr_cons_pen_norm", integrator="rk4", **UNC)
    pop_of = lambda s: PolicyPopulation.from_policies(pop_members(s, "float64") * 2)  # noqa: E731  (four members)
    # (a plan with neither feature takes pcg_rollout_policy_pop under fused=True: what it refuses there is the slice size)
    cases = [("G = 96", ok, pop_of(ok), 96, 0),
             ("offset 32", ok, pop_of(ok), 64, 32),
             ("a single policy", ok, pop_of(ok).member(0), 64, 0),
             ("neither rows nor parameters, G = 96", plain, pop_of(plain), 96, 0),
             ("rows and per-env parameters", both, pop_of(both), 64, 0),
             ("a constraint expression", EnvSpec(_expr_params()), pop_of(ok), 64, 0)]
    for what, spec, pop, g, off in cases:
        with pytest.raises(ValueError):  # (what)
            evaluate_population(_NoDevice(spec, env_offset=off), pop, g, fused=True)
