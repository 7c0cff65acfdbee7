#!/usr/bin/env python3
"""Domain randomisation: 65,536 cstr envs, each with its OWN heat-transfer coefficient UA and feed concentration Caf
(uniform, +-5 %, sampled by every reset: the reference's uncertainty_percentages on model parameters, pcgym.py:212-316),
rolled in closed loop under a small network -- the configuration under which a robust controller is trained.

  1. per step   -- the policy as a torch callable: one env-step launch and one torch evaluation per step
  2. fused      -- the same MLPPolicy handed to collect_rollouts(fused_unc=True): the whole episode in ONE launch
                   (pcg_rollout_policy_unc).  It is asked for: by default such a plan keeps the per-step loop, whose results
                   the fused kernel matches to rounding, not to the bit.

The observation carries the two parameters as extra slots [Ca, T, Ca_SP, UA, Caf] (normalised by the uncertainty bounds), so
the network has five inputs: a policy may condition on them (here it does), or ignore them with zero weights.

Then collect_onpolicy gathers what PPO needs per iteration with a Gaussian actor and a critic (pcg_rollout_actor_unc), and
shows the weight refresh after an optimiser step; every reset in between draws new parameters.

Needs an MI355X (there is no CPU path):  python examples/domain_randomisation.py
"""
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
    # initial states +-3 % / +-0.5 %, and the two model parameters +-5 % inside their bounds
    "uncertainty_percentages": {"x0": [0.03, 0.005], "UA": 0.05, "Caf": 0.05}, "distribution": "uniform",
    "uncertainty_bounds": {"low": np.array([4e4, 0.9]), "high": np.array([6e4, 1.1])},
    "integrator": "rk4",  # per-env parameters run under rk4 (fused and per step) or dopri5 (per step)
}
NOBS = 5  # Ca, T, the Ca set point, UA, Caf


def mlp(n_out=1):
    return torch.nn.Sequential(torch.nn.Linear(NOBS, 16), torch.nn.Tanh(), torch.nn.Linear(16, 16), torch.nn.Tanh(),
                               torch.nn.Linear(16, n_out)).double()


def main():
    torch.manual_seed(0)
    net = mlp()
    policy = MLPPolicy.from_torch(net, out_map="clip", out_low=-1.0, out_high=1.0)
    B = 1 << 16
    out = {}
    for name, pol, fused in (("per step", lambda obs: policy(obs), False), ("fused", policy, True)):
        env = make_vec_env(env_params, n_envs=B, seed=0)
        assert env.spec.nobs == NOBS and env.spec.nunc == 2
        collect_rollouts(env, policy=pol, fused_unc=fused)  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out[name] = d = collect_rollouts(env, policy=pol, fused_unc=fused)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ua, caf = d["x"][3, 0], d["x"][4, 0]  # (physical units; constant along an episode)
        print(f"{name:8s}: {dt * 1e3:7.2f} ms per episode of {B} envs ({B * (N - 1) / dt:.2e} env-steps/s)  x {tuple(d['x'].shape)}  "
              f"UA in [{ua.min().item():.0f}, {ua.max().item():.0f}]  Caf in [{caf.min().item():.3f}, {caf.max().item():.3f}]  "
              f"mean return {d['r'].sum(dim=1).mean().item():.3f}")
        env.close()
    diff = max(float((out["fused"][k] - out["per step"][k]).abs().max()) for k in ("x", "u", "r"))
    print(f"largest difference between the two routes over x, u, r: {diff:.2e} (two kernels, two fp64 summation orders, a closed loop)")
    policy.close()

    # ---- what PPO collects per iteration, then the refresh after an optimiser step ----
    critic_net = mlp()
    log_std = torch.nn.Parameter(torch.full((1,), -1.0, dtype=torch.float64))
    ac = GaussianActorCritic.from_torch(net, log_std, critic_net, out_map="clip", out_low=-1.0, out_high=1.0)
    env = make_vec_env(env_params, n_envs=B, seed=0)
    for it in range(2):
        collect_onpolicy(env, ac, fused_unc=True)  # warm-up (and another draw of the parameters)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = collect_onpolicy(env, ac, gamma=0.99, lam=0.95, fused_unc=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        # (a reactor with a low UA and a hot start can run away, and the fixed-step integration of a runaway overflows: such
        # an env carries non-finite rewards from then on and a status byte in env.status -- mask it, as a trainer would)
        ok = torch.isfinite(d["rew"]).all(dim=0)
        print(f"actor-critic, iteration {it}: {dt * 1e3:7.2f} ms per episode  obs {tuple(d['obs'].shape)} act {tuple(d['act'].shape)}  "
              f"sigma {ac.sigma[0]:.4f}  mean logp {d['logp'].mean().item():.3f}  envs that ran away {int((~ok).sum())}  "
              f"mean return of the others {d['rew'][:, ok].sum(dim=0).mean().item():.3f}  adv std {d['adv'][:, ok].std().item():.3f}")
        with torch.no_grad():  # an "optimiser step": same shapes, same device blocks
            for prm in list(net.parameters()) + list(critic_net.parameters()):
                prm.add_(0.01 * torch.randn_like(prm))
            log_std.sub_(0.05)
        ac.update_(actor=net, log_std=log_std, critic=critic_net)
    env.close(), ac.close()


if __name__ == "__main__":
    main()
