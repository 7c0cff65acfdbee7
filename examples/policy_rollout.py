#!/usr/bin/env python3
"""A trained-policy-shaped network rolled over 65,536 cstr envs in closed loop, two ways:

  1. per step   -- the policy as a torch callable: one env-step launch and one torch evaluation per step
  2. fused      -- the same MLPPolicy handed to collect_rollouts as a declarative policy: the whole episode in ONE launch,
                   the network evaluated inside the rollout kernel between two env steps (pcg_rollout_policy)

Both return the reference's policy_eval.rollout arrays x (Nx, N, reps), u (Nu, N, reps), r (1, N, reps)
(policy_evaluation.py:71-130), reps = the env axis.  The network here is a small torch.nn.Sequential with fixed-seed
weights standing in for a stable-baselines3 MlpPolicy's actor (Linear / Tanh / Linear / Tanh / Linear).

A third section collects ON-POLICY data with the stochastic form of the same network -- stable-baselines3's MlpPolicy:
a Gaussian actor with a state-independent log_std plus a value network -- through collect_onpolicy: sampled actions, their
log-probabilities, values, rewards, GAE advantages and returns, again in one launch per episode (pcg_rollout_actor), and
shows the refresh a training loop does after an optimiser step (GaussianActorCritic.update_: no device allocation).

Needs an MI355X (there is no CPU path):  python examples/policy_rollout.py
"""
import copy
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcgym_amd import GaussianActorCritic, MLPPolicy, collect_onpolicy, collect_rollouts, make_vec_env  # noqa: E402

N = 60
env_params = {
    "model": "cstr", "N": N, "tsim": 26,
    "SP": {"Ca": [0.85] * (N // 3) + [0.9] * (N // 3) + [0.87] * (N - 2 * (N // 3))},
    "o_space": {"low": np.array([0.7, 300.0, 0.8]), "high": np.array([1.0, 350.0, 0.9])},
    "a_space": {"low": np.array([295.0]), "high": np.array([302.0])},
    "x0": np.array([0.8, 330.0, 0.8]), "r_scale": {"Ca": 1e3}, "normalise_a": True, "normalise_o": True,
    "uncertainty_percentages": {"x0": [0.03, 0.005]}, "distribution": "uniform",
    "integrator": "rk4",  # the fused closed loop runs the fixed-step schemes (rk4 / cv8); other plans take the per-step loop
}


def main():
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(3, 16), torch.nn.Tanh(), torch.nn.Linear(16, 16), torch.nn.Tanh(),
                              torch.nn.Linear(16, 1)).double()
    policy = MLPPolicy.from_torch(net, out_map="clip", out_low=-1.0, out_high=1.0)
    B = 1 << 16
    out = {}
    for name, pol in (("per step", lambda obs: policy(obs)), ("fused", policy)):
        env = make_vec_env(env_params, n_envs=B, seed=0)
        collect_rollouts(env, policy=pol)  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out[name] = collect_rollouts(env, policy=pol)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        d = out[name]
        print(f"{name:8s}: {dt * 1e3:7.2f} ms per episode of {B} envs ({B * (N - 1) / dt:.2e} env-steps/s)  "
              f"x {tuple(d['x'].shape)} u {tuple(d['u'].shape)} r {tuple(d['r'].shape)}  mean return {d['r'].sum(dim=1).mean().item():.3f}")
        env.close()
    diff = max(float((out["fused"][k] - out["per step"][k]).abs().max()) for k in ("x", "u", "r"))
    print(f"largest difference between the two routes over x, u, r: {diff:.2e} (two fp64 summation orders through a closed loop)")
    policy.close()
    float32_leg(net, B)
    actor_critic(net, B)
    constrained(net, B)


def float32_leg(net, B):
    """the network as stable-baselines3 holds it -- a float32 module -- evaluated in float32 inside the kernel: its parameters
    are kept bit for bit, every recorded action is a float32 value, the env arithmetic stays fp64"""
    net32 = copy.deepcopy(net).float()  # (the caller's module stays as it is)
    policy32 = MLPPolicy.from_torch(net32, out_map="clip", out_low=-1.0, out_high=1.0, dtype="float32")
    env = make_vec_env(env_params, n_envs=B, seed=0)
    collect_rollouts(env, policy=policy32)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d = collect_rollouts(env, policy=policy32)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"fused, float32 policy: {dt * 1e3:7.2f} ms per episode of {B} envs ({B * (N - 1) / dt:.2e} env-steps/s)  "
          f"mean return {d['r'].sum(dim=1).mean().item():.3f}")
    env.close(), policy32.close()


def actor_critic(actor_net, B):
    """what PPO collects per iteration: the exploration noise is the engine's Philox stream (seed, global env index, t,
    purpose 0x400), so a sharded run samples what the unsharded run samples"""
    critic_net = torch.nn.Sequential(torch.nn.Linear(3, 16), torch.nn.Tanh(), torch.nn.Linear(16, 16), torch.nn.Tanh(),
                                     torch.nn.Linear(16, 1)).double()
    log_std = torch.nn.Parameter(torch.full((1,), -1.0, dtype=torch.float64))
    ac = GaussianActorCritic.from_torch(actor_net, log_std, critic_net, out_map="clip", out_low=-1.0, out_high=1.0)
    out = {}
    for name, fused in (("per step", False), ("fused", None)):
        env = make_vec_env(env_params, n_envs=B, seed=0)
        collect_onpolicy(env, ac, fused=fused)  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out[name] = d = collect_onpolicy(env, ac, gamma=0.99, lam=0.95, fused=fused)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"actor-critic, {name:8s}: {dt * 1e3:7.2f} ms per episode  obs {tuple(d['obs'].shape)} act {tuple(d['act'].shape)} "
              f"logp {tuple(d['logp'].shape)} val {tuple(d['val'].shape)}  mean logp {d['logp'].mean().item():.3f}  "
              f"mean return {d['rew'].sum(dim=0).mean().item():.3f}  adv std {d['adv'].std().item():.3f}")
        env.close()
    diff = max(float((out["fused"][k] - out["per step"][k]).abs().max()) for k in ("obs", "act", "val", "rew"))
    same = torch.equal(out["fused"]["logp"], out["per step"]["logp"])
    print(f"largest difference between the two routes over obs, act, val, rew: {diff:.2e}; log-probabilities bitwise equal: {same}")
    # an "optimiser step", then the refresh: same shapes, same device blocks
    with torch.no_grad():
        for prm in list(actor_net.parameters()) + list(critic_net.parameters()):
            prm.add_(0.01 * torch.randn_like(prm))
        log_std.sub_(0.05)
    ac.update_(actor=actor_net, log_std=log_std, critic=critic_net)
    env = make_vec_env(env_params, n_envs=B, seed=0)
    d = collect_onpolicy(env, ac)
    print(f"after update_: sigma {ac.sigma[0]:.4f}, mean logp {d['logp'].mean().item():.3f}")
    env.close(), ac.close()


def constrained(actor_net, B):
    """the same envs with constraint rows (a temperature band, -1000 penalty while outside): the fused calls record every
    step's rows and violation flags -- `g` of collect_rollouts in the reference's axis order, `g` / `g_pre` / `viol` of
    collect_onpolicy(record_cons=True): a cost signal or a mask for a constrained trainer.  An env that violates keeps
    stepping; with terminate_on_violation=True the advantage recursion is cut at the violating step (one launch, pcg_gae,
    with `viol` as its termination mask) and `alive` marks the steps up to and including it: the mask for the loss."""
    # (reference_compat=False: the rows read the physical state; the reference hands its constraint callable a state it has
    # "de-normalised" a second time when normalise_o is set -- quirk Q3 -- and a band in kelvin means nothing there)
    p = dict(copy.deepcopy(env_params), r_penalty=True, done_on_cons_vio=False, reference_compat=False,
             constraints={"A": np.array([[0.0, 1.0, 0.0, 0.0], [0.0, -1.0, 0.0, 0.0]]), "b": np.array([332.0, -321.0])})
    policy = MLPPolicy.from_torch(actor_net, out_map="clip", out_low=-1.0, out_high=1.0)
    for name, pol in (("per step", lambda obs: policy(obs)), ("fused", policy)):
        env = make_vec_env(p, n_envs=B, seed=0)
        collect_rollouts(env, policy=pol)  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = collect_rollouts(env, policy=pol)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"constrained, {name:8s}: {dt * 1e3:7.2f} ms per episode  g {tuple(d['g'].shape)}  "
              f"entries violated {(d['g'][:, 1:] > 0).any(dim=0).double().mean().item():.3f}  mean return {d['r'].sum(dim=1).mean().item():.1f}")
        env.close()
    critic_net = torch.nn.Sequential(torch.nn.Linear(3, 16), torch.nn.Tanh(), torch.nn.Linear(16, 1)).double()
    ac = GaussianActorCritic.from_torch(actor_net, torch.full((1,), -1.0, dtype=torch.float64), critic_net, out_map="clip",
                                        out_low=-1.0, out_high=1.0)
    env = make_vec_env(p, n_envs=B, seed=0)
    d = collect_onpolicy(env, ac, record_cons=True, terminate_on_violation=True)
    first = torch.where(d["viol"].any(dim=0), d["viol"].double().argmax(dim=0), d["viol"].shape[0])
    print(f"constrained actor-critic: g {tuple(d['g'].shape)} g_pre {tuple(d['g_pre'].shape)} viol {tuple(d['viol'].shape)}  "
          f"envs that violate at some step {d['viol'].any(dim=0).double().mean().item():.3f}, first at step {first.double().mean().item():.1f} on average")
    print(f"terminate_on_violation: alive {tuple(d['alive'].shape)}  steps alive {d['alive'].double().mean().item():.3f}  "
          f"mean |adv| over the alive steps {d['adv'][d['alive']].abs().mean().item():.3f}")
    env.close(), ac.close(), policy.close()


if __name__ == "__main__":
    main()
