#!/usr/bin/env python3
"""Derivative-free policy search with the weights born, scored and refitted ON the device: the cross-entropy method of
examples/policy_search.py, then an antithetic evolution strategy, on the canonical cstr.

Every generation is a handful of launches and no weight crosses PCIe after the first one:

  * PolicyPopulation.sample_ draws the 256 members of a diagonal Gaussian straight into the packed device blocks
    (pcg_policy_pop_sample: Philox + Box-Muller keyed by seed, generation, member and parameter);
  * evaluate_population scores each member on its own 256 envs -- 65,536 envs, ONE launch (pcg_rollout_policy_pop);
  * CEM  : PolicyPopulation.flat(members=elite) gathers the best tenth as flat parameter vectors, the refit is two torch
           reductions on the device;
    ES   : centered_ranks(score) weights the noise, PolicyPopulation.noise_dot forms sum_m w_m z(m, .) from the SAME keys
           (pcg_policy_pop_noise_dot: the noise is never stored), the update is one torch statement.

--dtype float32 searches over float32 members (pcg_policy_pop_create_f32): the same calls, the same keys and fp64 mean / std;
each sampled parameter is stored rounded to float32 and every member is evaluated in float32 inside the kernel.

--per-env-params searches for a controller that holds up over a DISTRIBUTION of plants: the heat-transfer coefficient UA and
the feed concentration Caf are drawn per env at every reset (U(+-5 %), bench.py's cstr_unc parameters), each member is scored
on its own 256 randomised plants, still in one launch (pcg_rollout_policy_pop_unc: evaluate_population(..., fused_unc=True)),
and every generation prints the worst per-member score -- each member's worst plant -- beside the mean.

Needs an MI355X (there is no CPU path):  python examples/policy_search_device.py [iterations] [--dtype float32] [--per-env-params]
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
from pcgym_amd import PolicyPopulation, centered_ranks, evaluate_population, make_vec_env  # noqa: E402

P, G, HIDDEN = 256, 256, 16
SEED = 2024
FAIL = -1000.0  # --per-env-params: the return of a plant that ran away (finite returns of this task are above -200)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("iterations", nargs="?", type=int, default=5)
    ap.add_argument("--dtype", choices=["float64", "float32"], default="float64")
    ap.add_argument("--per-env-params", action="store_true", help="UA and Caf ~ U(+-5 %) per env, scored with fused_unc=True")
    args = ap.parse_args()
    iters = args.iterations
    p = copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"])
    p.update(integrator="rk4")
    if args.per_env_params:
        p.update(uncertainty_percentages=dict(p.get("uncertainty_percentages") or {}, UA=0.05, Caf=0.05), distribution="uniform",
                 uncertainty_bounds={"low": np.array([4e4, 0.9]), "high": np.array([6e4, 1.1])})
    env = make_vec_env(p, n_envs=P * G, seed=0)
    spec, dev = env.spec, env.device
    dims = [spec.nobs, HIDDEN, spec.na]
    # the device blocks are allocated once, from zeros; every generation rewrites them in place
    pop = PolicyPopulation([np.zeros((P, dims[l + 1], dims[l])) for l in range(len(dims) - 1)],
                           [np.zeros((P, dims[l + 1])) for l in range(len(dims) - 1)],
                           activation="tanh", out_map="clip", out_low=-1.0, out_high=1.0, dtype=args.dtype)
    pop.handle(dev)
    n = pop.n_params
    what = f"({P} members x {G} envs, {spec.N - 1} steps, one launch; {n} parameters per member, none crossed to the host)"

    def evaluate():
        """(score per member, what to print of the generation).  On randomised plants: also each member's worst plant, and a
        plant the member lets run away (an explicit step of the exothermic reactor past ignition is not finite) scores FAIL"""
        out = evaluate_population(env, pop, G, gamma=1.0, fused_unc=args.per_env_params)
        score, extra = out["score"], ""
        if args.per_env_params:
            ret = out["ret"]
            lost = ~torch.isfinite(ret)
            ret = torch.where(lost, torch.full_like(ret, FAIL), ret).view(-1, G)
            score, worst = ret.mean(1), ret.min(1).values  # (plain torch: member m's mean and its worst plant)
            extra = (f"   worst per-member score {float(worst.min()):10.4f} (the best member's worst plant {float(worst[torch.argmax(score)]):10.4f}; "
                     f"{int(lost.sum())} of {lost.numel()} plants ran away)")
        return score, f"best score {float(score.max()):10.4f}   mean score {float(score.mean()):10.4f}{extra}"

    # ---- cross-entropy method: refit the Gaussian to the best tenth ----
    mean = torch.zeros(n, dtype=torch.float64, device=dev)
    std = torch.full((n,), 0.5, dtype=torch.float64, device=dev)
    for it in range(iters):
        pop.sample_(mean, std, SEED, generation=it, check=False)
        score, line = evaluate()
        elite = torch.topk(score, P // 10).indices
        theta = pop.flat(members=elite)
        mean, std = theta.mean(dim=0), theta.std(dim=0, unbiased=False) + 0.02
        print(f"CEM iteration {it}: {line}   {what}")

    # ---- antithetic evolution strategy with centered ranks, from where CEM stopped ----
    sigma, lr = 0.1, 0.05
    std = torch.full((n,), sigma, dtype=torch.float64, device=dev)
    for it in range(iters):
        gen = iters + it  # (generations already used above keyed other noise)
        pop.sample_(mean, std, SEED, generation=gen, antithetic=True, check=False)
        score, line = evaluate()
        grad = pop.noise_dot(centered_ranks(score), SEED, generation=gen, antithetic=True)  # sum_m w_m z(m, .)
        mean = mean + (lr / (P * sigma)) * grad
        print(f"ES  iteration {it}: {line}   {what}")

    best = pop.member(int(torch.argmax(score)))  # (the first look at the host arrays: one flat() and one copy bring them back)
    print(f"best member of the last generation: layers {[w.shape for w in best.weights]}, |W0| max {np.abs(best.weights[0]).max():.3f}")
    env.close(), pop.close()


if __name__ == "__main__":
    main()
