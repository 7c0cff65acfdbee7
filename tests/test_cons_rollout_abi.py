"""CPU: pcg_rollout_policy_cons / pcg_rollout_actor_cons (the fused closed-loop rollouts on plans with constraint rows) --
header <-> python mirror <-> library, and the host-only predicates that route collect_rollouts / collect_onpolicy to them."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

import scenarios as SC
from pcgym_amd import GaussianActorCritic, MLPPolicy, _lib
from pcgym_amd import _abi as abi
from pcgym_amd.config import EnvSpec
from pcgym_amd.policy import fused_actor_cons_ok, fused_actor_ok, fused_cons_ok, fused_policy_ok
from test_policy_jit_plans import _chemostat, _nets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pcgym_hip.h")).read()
TAIL = "double* g_seq, int64_t g_step_stride, int64_t g_comp_stride, uint8_t* viol_seq, int64_t viol_step_stride, uint64_t seed, void* stream"


def _decl(name):
    m = re.search(r"PCG_API\s+(\w+)\s+%s\(([^)]*)\);" % name, HDR)
    assert m, f"the header does not declare {name}"
    return m.group(1), [a.strip() for a in re.sub(r"\s+", " ", m.group(2)).split(",")]


@pytest.mark.parametrize("base", ["pcg_rollout_policy", "pcg_rollout_actor"])
def test_the_entry_points_are_declared_mirrored_and_exported(base):
    name = base + "_cons"
    ret, args = _decl(name)
    _, base_args = _decl(base)
    # every argument of the unconstrained call, in order, up to record_next_action; then the rows, the flags, seed, stream
    assert ret == "int" and base_args[-3].endswith("record_next_action")
    assert args[:len(base_args) - 2] == base_args[:-2]
    assert ", ".join(args[len(base_args) - 2:]) == TAIL
    assert abi.EXPORTS.count(name) == 1 and len(set(abi.EXPORTS)) == len(abi.EXPORTS)
    lib = _lib.load()  # (loads without a GPU: no HIP call is made)
    fn, fb = getattr(lib, name), getattr(lib, base)
    assert fn.restype is C.c_int and len(fn.argtypes) == len(args) == len(fb.argtypes) + 5
    assert list(fn.argtypes[:len(base_args) - 2]) == list(fb.argtypes[:-2])
    assert list(fn.argtypes[len(base_args) - 2:]) == [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p]
    # the functions only add to ABI 16
    assert abi.PCG_ABI_VERSION == 16 == lib.pcg_version()
    assert int(re.search(r"#define PCG_ABI_VERSION (\d+)", HDR).group(1)) == 16
    # host-side refusals come before the device is touched
    assert fn(*[None if t is C.c_void_p or hasattr(t, "contents") else 0 for t in fn.argtypes]) == abi.PCG_E_PLAN


def test_the_header_states_the_semantics():
    doc = re.sub(r"\s*\n\s*\*\s*", " ", HDR)
    para = doc[doc.index("The two closed-loop calls on plans WITH constraint rows"):doc.index("PCG_API int pcg_rollout_policy_cons")]
    for phrase in ("KEEPS STEPPING", "Summation order", "the states ascending", "ncon == 0", "run-time compiled code", "float32 policy",
                   "g_comp_stride < B", "viol_step_stride < B", "safe under stream capture", "still keep only the last step's rows"):
        assert phrase in para, phrase


def _cons(integ, **over):
    p = copy.deepcopy(SC.scenarios()["cstr_cons_pen_norm"]["env_params"])
    p.update(integrator=integ, **over)
    return p


@pytest.mark.parametrize("integ", ["rk4", "cv8"])
def test_the_predicates_take_the_constraint_showcase(integ):
    spec = EnvSpec(_cons(integ))
    assert spec.ncon and spec.user_cons_src is None
    pol, ac = _nets(spec)
    assert fused_cons_ok(spec, pol) and fused_actor_cons_ok(spec, ac)
    assert not fused_policy_ok(spec, pol) and not fused_actor_ok(spec, ac)  # the existing calls keep refusing the plan
    no_critic = GaussianActorCritic(pol, np.full(spec.na, -1.0))
    assert fused_actor_cons_ok(spec, no_critic)
    assert not fused_cons_ok(spec, lambda o: o) and not fused_actor_cons_ok(spec, pol)


def _row(spec):
    """one affine row over [x | SP | d | u] of `spec`"""
    return {"A": np.ones((1, spec.nobs - spec.nunc + spec.nu)), "b": np.array([1.0])}


def test_the_predicates_refuse_what_the_kernels_do_not_carry():
    ok = EnvSpec(_cons("rk4"))
    pol, ac = _nets(ok)
    refused = {}
    # no rows: the existing calls
    plain = EnvSpec(dict(copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"]), integrator="rk4"))
    refused["unconstrained"] = (plain, *_nets(plain))
    assert fused_policy_ok(plain, refused["unconstrained"][1])
    refused["dopri5"] = (EnvSpec(_cons("dopri5")), pol, ac)
    unc = EnvSpec(_cons("rk4", uncertainty_percentages={"q": 0.03}, distribution="uniform",
                        uncertainty_bounds={"low": np.array([90.0]), "high": np.array([110.0])}))
    assert unc.nunc == 1 and unc.ncon
    refused["per_env_parameters"] = (unc, *_nets(unc))
    # float32 networks
    p32 = MLPPolicy(pol.weights, pol.biases, dtype="float32")
    c32 = MLPPolicy(ac.critic.weights, ac.critic.biases, out_map="none", dtype="float32")
    refused["float32"] = (ok, p32, GaussianActorCritic(p32, np.full(ok.na, -1.0), c32))
    # run-time compiled code: a user model with affine rows, a constraint expression
    chem = EnvSpec(_chemostat(integrator="rk4"))
    chem = EnvSpec(_chemostat(integrator="rk4", constraints=_row(chem), done_on_cons_vio=False, r_penalty=True))
    assert chem.ncon == 1 and chem.user_rhs_src is not None and chem.user_cons_src is None
    refused["custom_model"] = (chem, *_nets(chem))
    expr = EnvSpec(_cons("rk4", constraints={"expr": ["T - 327.0"]}))
    assert expr.ncon == 1 and expr.user_cons_src
    refused["expression"] = (expr, *_nets(expr))
    # a policy of another size
    wrong = MLPPolicy([np.zeros((ok.na, ok.nobs + 1))], [np.zeros(ok.na)])
    refused["wrong_size"] = (ok, wrong, GaussianActorCritic(wrong, np.full(ok.na, -1.0)))
    for name, (spec, q, a) in refused.items():
        assert not fused_cons_ok(spec, q), name
        assert not fused_actor_cons_ok(spec, a), name
        if spec.ncon:
            assert not fused_policy_ok(spec, q) and not fused_actor_ok(spec, a), name
    # a tanh-mapped actor: the policy call takes it, the actor call does not (GaussianActorCritic itself refuses to hold one)
    tanh = MLPPolicy(pol.weights, pol.biases, out_map="tanh")
    assert fused_cons_ok(ok, tanh)
    squashed = GaussianActorCritic(pol, np.full(ok.na, -1.0))
    squashed.actor = tanh
    assert not fused_actor_cons_ok(ok, squashed) and not fused_actor_ok(ok, squashed)
