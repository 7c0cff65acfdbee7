"""CPU: pcg_rollout_policy_unc / pcg_rollout_actor_unc (the fused closed-loop rollouts on plans with per-env parameters) --
header <-> python mirror <-> library, and the host-only predicates that route collect_rollouts / collect_onpolicy to them."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

import scenarios as SC
from helpers import UNSUPPORTED_PLANS
from pcgym_amd import GaussianActorCritic, MLPPolicy, _lib
from pcgym_amd import _abi as abi
from pcgym_amd.config import EnvSpec
from pcgym_amd.policy import (fused_actor_cons_ok, fused_actor_ok, fused_actor_unc_ok, fused_cons_ok, fused_policy_ok,
                              fused_unc_ok)
from test_policy_jit_plans import _chemostat, _nets, _traced_reward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pcgym_hip.h")).read()
Q_UNC = dict(uncertainty_percentages={"q": 0.03}, distribution="uniform",
             uncertainty_bounds={"low": np.array([90.0]), "high": np.array([110.0])})


def _decl(name):
    m = re.search(r"PCG_API\s+(\w+)\s+%s\(([^)]*)\);" % name, HDR)
    assert m, f"the header does not declare {name}"
    return m.group(1), [a.strip() for a in re.sub(r"\s+", " ", m.group(2)).split(",")]


@pytest.mark.parametrize("base", ["pcg_rollout_policy", "pcg_rollout_actor"])
def test_the_entry_points_are_declared_mirrored_and_exported(base):
    name = base + "_unc"
    ret, args = _decl(name)
    _, base_args = _decl(base)
    assert ret == "int" and args == base_args  # the base call's exact argument list: nothing new is recorded
    assert abi.EXPORTS.count(name) == 1 and len(set(abi.EXPORTS)) == len(abi.EXPORTS)
    lib = _lib.load()  # (loads without a GPU: no HIP call is made)
    fn, fb = getattr(lib, name), getattr(lib, base)
    assert fn.restype is C.c_int and len(fn.argtypes) == len(args) and list(fn.argtypes) == list(fb.argtypes)
    # the functions only add to ABI 16
    assert abi.PCG_ABI_VERSION == 16 == lib.pcg_version()
    assert int(re.search(r"#define PCG_ABI_VERSION (\d+)", HDR).group(1)) == 16
    # host-side refusals come before the device is touched
    assert fn(*[None if t is C.c_void_p or hasattr(t, "contents") else 0 for t in fn.argtypes]) == abi.PCG_E_PLAN


def test_the_header_states_the_semantics():
    doc = re.sub(r"\s*\n\s*\*\s*", " ", HDR)
    para = doc[doc.index("The two closed-loop calls on plans WITH per-env parameters"):doc.index("PCG_API int pcg_rollout_policy_unc")]
    for phrase in ("nothing new is recorded", "[x | SP | d | unc]", "rebuilt from it every step", "ONCE per call was built and measured", "whatever the preceding pcg_reset wrote",
                   "pcgym.py:300-316", "nunc == 0", "ncon > 0", "io->t != NULL", "any other integrator", "run-time compiled code",
                   "float32 policy", "affine registry models", "io->p_unc == NULL", "safe under stream capture",
                   "per-env parameters together with constraint rows", "per-env counters"):
        assert phrase in para, phrase
    # the paragraphs of the existing calls are where they were
    assert doc.index("The two closed-loop calls on plans WITH constraint rows") < doc.index("The two closed-loop calls on plans WITH per-env")


def _unc(integ="rk4", scenario="cstr_canonical", **over):
    p = copy.deepcopy(SC.scenarios()[scenario]["env_params"])
    p.update(integrator=integ, **copy.deepcopy(Q_UNC))
    p.update(over)
    return p


def _existing_all_false(spec, pol, ac):
    return not (fused_policy_ok(spec, pol) or fused_actor_ok(spec, ac) or fused_cons_ok(spec, pol) or fused_actor_cons_ok(spec, ac))


def test_the_predicates_take_the_per_env_parameter_plan():
    scen, over = UNSUPPORTED_PLANS["per_env_parameters"]  # the plan the existing closed-loop tests hold as refused
    p = copy.deepcopy(SC.scenarios()[scen]["env_params"])
    p.update(copy.deepcopy(over))
    for spec in (EnvSpec(p), EnvSpec(_unc())):
        assert spec.nunc == 1 and not spec.ncon and spec.integrator == "rk4"
        pol, ac = _nets(spec)
        assert pol.n_in == spec.nobs  # (the parameter slot is an input of the network)
        assert fused_unc_ok(spec, pol) and fused_actor_unc_ok(spec, ac)
        no_critic = GaussianActorCritic(pol, np.full(spec.na, -1.0))
        assert fused_actor_unc_ok(spec, no_critic)
        # the four existing predicates keep refusing the plan
        assert _existing_all_false(spec, pol, ac) and _existing_all_false(spec, pol, no_critic)
        assert not fused_unc_ok(spec, lambda o: o) and not fused_actor_unc_ok(spec, pol)


def test_the_predicates_refuse_what_the_kernels_do_not_carry():
    ok = EnvSpec(_unc())
    pol, ac = _nets(ok)
    refused = {}
    # no per-env parameters: the existing calls
    plain = EnvSpec(dict(copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"]), integrator="rk4"))
    refused["nunc == 0"] = (plain, *_nets(plain))
    assert plain.nunc == 0 and fused_policy_ok(plain, refused["nunc == 0"][1])
    # per-env parameters and a constraint row: neither family
    both = EnvSpec(_unc(scenario="cstr_cons_pen_norm"))
    assert both.nunc == 1 and both.ncon
    refused["constraint_row"] = (both, *_nets(both))
    assert _existing_all_false(both, *_nets(both))
    d5 = EnvSpec(_unc("dopri5"))
    assert d5.nunc == 1
    refused["dopri5"] = (d5, *_nets(d5))
    # float32 networks
    p32 = MLPPolicy(pol.weights, pol.biases, dtype="float32")
    c32 = MLPPolicy(ac.critic.weights, ac.critic.biases, out_map="none", dtype="float32")
    refused["float32"] = (ok, p32, GaussianActorCritic(p32, np.full(ok.na, -1.0), c32))
    # a reward expression: today the spec is made (the plan's creation then refuses per-env parameters on run-time compiled code)
    expr = EnvSpec(_traced_reward(integrator="rk4", **copy.deepcopy(Q_UNC)))
    assert expr.nunc == 1 and expr.user_reward_src
    refused["reward_expression"] = (expr, *_nets(expr))
    # ... and a user model refuses them when the spec is made
    with pytest.raises(ValueError, match="uncertainty"):
        EnvSpec(_chemostat(integrator="rk4", uncertainty_percentages={"mumax": 0.1}, distribution="uniform"))
    # a policy of another size (the plan's observation WITHOUT its parameter slot)
    wrong = MLPPolicy([np.zeros((ok.na, ok.nobs - ok.nunc))], [np.zeros(ok.na)])
    refused["wrong_size"] = (ok, wrong, GaussianActorCritic(wrong, np.full(ok.na, -1.0)))
    for name, (spec, q, a) in refused.items():
        assert not fused_unc_ok(spec, q), name
        assert not fused_actor_unc_ok(spec, a), name
    # a critic of another dtype / size alone is enough
    mixed = GaussianActorCritic(pol, np.full(ok.na, -1.0), ac.critic)
    mixed.critic = c32
    assert not fused_actor_unc_ok(ok, mixed)
    # a tanh-mapped actor: the policy call takes it, the actor call does not (GaussianActorCritic itself refuses to hold one)
    tanh = MLPPolicy(pol.weights, pol.biases, out_map="tanh")
    assert fused_unc_ok(ok, tanh)
    squashed = GaussianActorCritic(pol, np.full(ok.na, -1.0))
    squashed.actor = tanh
    assert not fused_actor_unc_ok(ok, squashed) and not fused_actor_ok(ok, squashed)
