#!/usr/bin/env python3
"""A trained-policy-shaped network rolled over 65,536 cstr envs in closed loop, two ways:

  1. per step   -- the policy as a torch callable: one env-step launch and one torch evaluation per step
  2. fused      -- the same MLPPolicy handed to collect_rollouts as a declarative policy: the whole episode in ONE launch,
                   the network evaluated inside the rollout kernel between two env steps (pcg_rollout_policy)

Both return the reference's policy_eval.rollout arrays x (Nx, N, reps), u (Nu, N, reps), r (1, N, reps)
(policy_evaluation.py:71-130), reps = the env axis.  The network here is a small torch.nn.Sequential with fixed-seed
weights standing in for a stable-baselines3 MlpPolicy's actor (Linear / Tanh / Linear / Tanh / Linear).

Needs an MI355X (there is no CPU path):  python examples/policy_rollout.py
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcgym_amd import MLPPolicy, collect_rollouts, make_vec_env  # noqa: E402

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


if __name__ == "__main__":
    main()
