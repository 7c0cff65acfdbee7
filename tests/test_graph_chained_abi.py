"""CPU: pcg_graph_chained -- declared in the header and mirrored in _abi.py with the same signature (test_abi.py holds the
export lists against each other), and it refuses what is not a step graph without touching a device."""
import ctypes as C
import os
import re

from pcgym_amd import _abi as abi
from pcgym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_with_the_signature_of_the_mirror():
    hdr = open(os.path.join(ROOT, "include", "pcgym_hip.h")).read()
    m = re.search(r"PCG_API int pcg_graph_chained\(([^)]*)\);", hdr)
    assert m, "pcg_graph_chained is not declared in include/pcgym_hip.h"
    assert [a.strip() for a in m.group(1).split(",")] == ["const pcg_graph* graph", "int32_t* launches", "int32_t* steps"]
    assert "pcg_graph_chained" in abi.EXPORTS
    lib = _lib.load()
    assert lib.pcg_graph_chained.restype is C.c_int
    assert lib.pcg_graph_chained.argtypes == [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    # as pcg_graph_held, its sibling
    assert lib.pcg_graph_chained.argtypes == lib.pcg_graph_held.argtypes


def test_null_and_foreign_handles_are_refused():
    lib = _lib.load()
    nl, ns = C.c_int32(-7), C.c_int32(-7)
    assert lib.pcg_graph_chained(None, C.byref(nl), C.byref(ns)) == abi.PCG_E_PLAN
    foreign = C.create_string_buffer(256)  # zeroed: no step graph's magic
    assert lib.pcg_graph_chained(C.cast(foreign, C.c_void_p), C.byref(nl), C.byref(ns)) == abi.PCG_E_PLAN
    assert lib.pcg_graph_chained(C.cast(foreign, C.c_void_p), None, None) == abi.PCG_E_PLAN
    assert (nl.value, ns.value) == (-7, -7)  # nothing written
