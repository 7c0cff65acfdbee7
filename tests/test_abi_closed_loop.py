"""CPU: header <-> python mirror for pcg_plan_prepare_closed_loop (ABI 16 only adds it), and its host-side statuses."""
import ctypes as C
import os
import re

from pcgym_amd import _abi as abi
from pcgym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pcgym_hip.h")).read()


def test_prepare_closed_loop_is_declared_mirrored_and_exported():
    m = re.search(r"PCG_API\s+(\w+)\s+pcg_plan_prepare_closed_loop\(([^)]*)\);", HDR)
    assert m, "the header does not declare pcg_plan_prepare_closed_loop"
    assert m.group(1) == "int" and re.sub(r"\s+", " ", m.group(2)).strip() == "pcg_plan* plan"
    assert "pcg_plan_prepare_closed_loop" in abi.EXPORTS and len(set(abi.EXPORTS)) == len(abi.EXPORTS)
    lib = _lib.load()  # (loads without a GPU: no HIP call is made)
    fn = lib.pcg_plan_prepare_closed_loop
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p]
    # the function only adds to ABI 16
    assert abi.PCG_ABI_VERSION == 16 == lib.pcg_version()
    assert int(re.search(r"#define PCG_ABI_VERSION (\d+)", HDR).group(1)) == 16


def test_prepare_closed_loop_refuses_what_is_not_a_plan():
    lib = _lib.load()
    assert lib.pcg_plan_prepare_closed_loop(None) == abi.PCG_E_PLAN
    not_a_plan = (C.c_uint32 * 64)()
    assert lib.pcg_plan_prepare_closed_loop(C.cast(not_a_plan, C.c_void_p)) == abi.PCG_E_PLAN


def test_header_says_when_the_module_is_built_and_what_a_capture_needs():
    doc = re.sub(r"\s*\n\s*\*\s*", " ", HDR)
    assert "pcg_plan_create() does NOT build" in doc
    assert "call pcg_plan_prepare_closed_loop(), or make one eager call, before capturing" in doc
    # the refusals that stay: constraint rows, per-env parameters, the other integrators
    para = doc[doc.index("T env steps in ONE launch"):doc.index("PCG_API int pcg_rollout_policy")]
    for phrase in ("constraint rows (user_cons_src included)", "per-env parameters", "PCG_INT_RK4 / PCG_INT_CV8"):
        assert phrase in para, phrase
    assert "user expressions or PCG_MODEL_USER" not in para
