"""CPU: which plans collect_rollouts / collect_onpolicy hand to the fused closed-loop calls (fused_policy_ok, fused_actor_ok)
when the plan carries run-time compiled code -- a custom_model, a traced custom_reward callable.  Those plans run the
closed-loop kernels from their own second module (pcg_plan_prepare_closed_loop); what still steps is what the kernels do not
carry: constraint rows (an expression constraint is rows too), per-env parameters, every integrator but rk4 / cv8.
"""
import copy

import numpy as np
import pytest

import scenarios as SC
from pcgym_amd import GaussianActorCritic, MLPPolicy
from pcgym_amd.config import EnvSpec, trace_reward_callable
from pcgym_amd.policy import fused_actor_ok, fused_policy_ok

CHEMOSTAT = {
    "states": ["X", "S"], "inputs": ["D"], "disturbances": ["Sf"],
    "parameters": {"mumax": 0.53, "Ks": 0.12, "Ki": 22.0, "Y": 0.4, "Sf": 4.0},
    "aux": {"mu": "mumax*S/(Ks + S + S*S/Ki)"},
    "rhs": ["(mu - D)*X", "D*(Sf - S) - mu*X/Y"],
}


def _chemostat(**kw):
    N = 30
    p = {"custom_model": copy.deepcopy(CHEMOSTAT), "N": N, "tsim": 15.0, "x0": np.array([1.2, 0.6, 1.4]),
         "SP": {"X": [1.4] * (N // 2) + [1.0] * (N - N // 2)}, "r_scale": {"X": 10.0},
         "a_space": {"low": np.array([0.0]), "high": np.array([0.45])},
         "o_space": {"low": np.array([0.0, 0.0, 0.0]), "high": np.array([3.0, 6.0, 3.0])},
         "normalise_a": True, "normalise_o": True}
    p.update(kw)
    return p


def _traced_reward(**kw):
    """the cstr with the custom_reward callable the reference ran (tests/golden/scenarios.py: reward_cstr_exp), traced"""
    p = copy.deepcopy(SC.scenarios()["cstr_expr_reward_q3"]["ref_env_params"])
    assert callable(p["custom_reward"])
    p.pop("constraints", None), p.pop("done_on_cons_vio", None), p.pop("r_penalty", None)
    p.update(kw)
    s = EnvSpec(p)  # (what VecEnv does with a callable: traced into one expression, compiled like {'expr': ...})
    return dict(s.env_params, custom_reward={"expr": trace_reward_callable(s.custom_reward, s)})


def _nets(spec, hidden=(16,)):
    rng = np.random.default_rng(0)
    dims = [spec.nobs, *hidden, spec.na]
    Ws = [rng.standard_normal((dims[l + 1], dims[l])) / np.sqrt(dims[l]) for l in range(len(dims) - 1)]
    bs = [0.1 * rng.standard_normal(dims[l + 1]) for l in range(len(dims) - 1)]
    pol = MLPPolicy(Ws, bs)
    critic = MLPPolicy(Ws[:-1] + [Ws[-1][:1]], bs[:-1] + [bs[-1][:1]], out_map="none")
    return pol, GaussianActorCritic(pol, np.full(spec.na, -1.0), critic)


@pytest.mark.parametrize("integ", ["rk4", "cv8"])
@pytest.mark.parametrize("make", [_chemostat, _traced_reward])
def test_run_time_compiled_plans_take_the_fused_calls(make, integ):
    spec = EnvSpec(make(integrator=integ))
    assert (spec.user_rhs_src is not None) or spec.user_reward_src, "not a run-time compiled plan"
    assert not spec.ncon and not spec.nunc
    pol, ac = _nets(spec)
    assert fused_policy_ok(spec, pol) and fused_actor_ok(spec, ac)
    # the network still has to fit the plan and the device form
    wrong = MLPPolicy([np.zeros((spec.na, spec.nobs + 1))], [np.zeros(spec.na)])
    assert not fused_policy_ok(spec, wrong) and not fused_policy_ok(spec, lambda o: o)
    squashed = GaussianActorCritic.__new__(GaussianActorCritic)
    squashed.actor, squashed.critic = MLPPolicy(pol.weights, pol.biases, out_map="tanh"), None
    assert not fused_actor_ok(spec, squashed)


@pytest.mark.parametrize("make", [_chemostat, _traced_reward])
@pytest.mark.parametrize("over", [
    dict(integrator="dopri5"), dict(integrator="rodas4"), dict(integrator="tsit5"),
    dict(integrator="rk4", constraints={"A": None, "b": [0.65]}, r_penalty=True, done_on_cons_vio=False),
    dict(integrator="rk4", constraints=lambda x, u: np.array([x[1] * x[1] - 0.4]).reshape(-1,), r_penalty=True, done_on_cons_vio=False),
], ids=["dopri5", "rodas4", "tsit5", "affine_rows", "expression_constraint"])
def test_what_the_closed_loop_kernels_do_not_carry_still_steps(make, over):
    over = dict(over)
    if isinstance(over.get("constraints"), dict):
        n = EnvSpec(make(integrator="rk4")).nobs
        row = [0.0] * (n + EnvSpec(make(integrator="rk4")).na + EnvSpec(make(integrator="rk4")).ndm)
        row[1] = 1.0
        over["constraints"] = {"A": [row], "b": [0.65]}
    spec = EnvSpec(make(**over))
    pol, ac = _nets(spec)
    if "constraints" in over:
        assert spec.ncon == 1
        if callable(over["constraints"]):
            assert spec.user_cons_src
    assert not fused_policy_ok(spec, pol) and not fused_actor_ok(spec, ac)


def test_per_env_parameters_still_step():
    """uncertainty_percentages on a model parameter (a custom_model refuses them at construction: the built-in cstr with the
    traced reward carries the case)"""
    spec = EnvSpec(_traced_reward(integrator="rk4", uncertainty_percentages={"q": 0.03}, distribution="uniform",
                                  uncertainty_bounds={"low": np.array([90.0]), "high": np.array([110.0])}))
    assert spec.nunc == 1 and spec.user_reward_src
    pol, ac = _nets(spec)
    assert not fused_policy_ok(spec, pol) and not fused_actor_ok(spec, ac)
    with pytest.raises(ValueError, match="uncertainty"):
        EnvSpec(_chemostat(integrator="rk4", uncertainty_percentages={"mumax": 0.1}, distribution="uniform"))
