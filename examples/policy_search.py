#!/usr/bin/env python3
"""Derivative-free policy search over network weights: a few iterations of the cross-entropy method on the canonical cstr.

Every iteration samples 256 candidate policies (1 x 16 tanh networks) from a diagonal Gaussian over the flattened weights,
scores each on its own 256 envs -- 65,536 envs, ONE launch (pcg_rollout_policy_pop through evaluate_population: each slice of
the batch is driven by its own member of a PolicyPopulation, the discounted returns are accumulated in the kernel) -- and
refits the Gaussian to the best tenth.  The population's device blocks are allocated once and rewritten every iteration
(PolicyPopulation.update_).

--dtype float32 holds the candidates as float32 members (rounded to nearest by the population, evaluated in float32 inside the
kernel); the Gaussian is refitted to the float64 samples as before.

Needs an MI355X (there is no CPU path):  python examples/policy_search.py [iterations] [--dtype float32]
"""
import argparse
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import scenarios as SC  # noqa: E402
from pcgym_amd import PolicyPopulation, evaluate_population, make_vec_env  # noqa: E402

P, G, HIDDEN = 256, 256, 16


def unflatten(theta, dims):
    """theta (P, n) -> ([W_l (P, n_next, n_prev)], [b_l (P, n_next)])"""
    Ws, bs, at = [], [], 0
    for l in range(len(dims) - 1):
        n = dims[l + 1] * dims[l]
        Ws.append(theta[:, at:at + n].reshape(-1, dims[l + 1], dims[l]))
        at += n
        bs.append(theta[:, at:at + dims[l + 1]])
        at += dims[l + 1]
    return Ws, bs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("iterations", nargs="?", type=int, default=5)
    ap.add_argument("--dtype", choices=["float64", "float32"], default="float64")
    args = ap.parse_args()
    iters = args.iterations
    p = copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"])
    p.update(integrator="rk4")
    env = make_vec_env(p, n_envs=P * G, seed=0)
    spec = env.spec
    dims = [spec.nobs, HIDDEN, spec.na]
    n = sum(dims[l + 1] * (dims[l] + 1) for l in range(len(dims) - 1))
    rng = np.random.default_rng(0)
    mean, std = np.zeros(n), np.full(n, 0.5)
    pop = None
    for it in range(iters):
        theta = mean + std * rng.standard_normal((P, n))
        Ws, bs = unflatten(theta, dims)
        if pop is None:
            pop = PolicyPopulation(Ws, bs, activation="tanh", out_map="clip", out_low=-1.0, out_high=1.0, dtype=args.dtype)
        else:
            pop.update_(Ws, bs)
        score = evaluate_population(env, pop, G, gamma=1.0)["score"]
        torch.cuda.synchronize()
        order = torch.argsort(score, descending=True).cpu().numpy()
        elite = theta[order[:P // 10]]
        mean, std = elite.mean(axis=0), elite.std(axis=0) + 0.02
        print(f"iteration {it}: best score {float(score[order[0]]):10.4f}   mean score {float(score.mean()):10.4f}   "
              f"({P} members x {G} envs, {spec.N - 1} steps, one launch)")
    env.close(), pop.close()


if __name__ == "__main__":
    main()
