#!/usr/bin/env python3
"""Constrained derivative-free policy search with everything on the device: the cross-entropy method over 256 networks on the
constraint showcase cstr_cons_pen_norm (temperature rows on the reactor, r_penalty), 65,536 envs, fitness

    score - lam * viol_share

where ``score`` is a member's mean return and ``viol_share`` the share of its (env, step) entries after which a row was
violated.  Every generation is a handful of launches and no weight, reward or flag crosses PCIe:

  * PolicyPopulation.sample_ draws the members of a diagonal Gaussian straight into the packed device blocks;
  * evaluate_population scores each member on its own 256 envs in ONE launch (pcg_rollout_policy_pop_cons): each env's return,
    its number of violating steps and its largest row value are accumulated in registers -- nothing of size T x B is
    recorded or reduced;
  * PolicyPopulation.flat(members=elite) gathers the best tenth, the refit is two torch reductions on the device.

Each generation prints the best and mean return, the violation share of the best member and of the population, and the
largest row value any env of the best member reached (<= 0: that member never violated).

The scenario's own band is violated after every step whatever the controller does (the rows are checked on the state as the
reference hands it to them, which under normalise_o is not the physical temperature the band was written for), so on it
the search can only trade return: the violation share stays 1.  --calibrate shows the trade-off
instead: it keeps the band's upper row and moves its bound to the median, over the envs of the first generation, of the
largest value the row reached (``gmax`` of a one-row pilot evaluation) -- half of the initial population's envs then violate
at some step, and the search has to find members that keep every env under the bound while it raises their return.

Needs an MI355X (there is no CPU path):
    python examples/policy_search_constrained.py [iterations] [--lam 2000] [--dtype float32] [--calibrate]
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
SEED = 2024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("iterations", nargs="?", type=int, default=8)
    ap.add_argument("--lam", type=float, default=2000.0, help="weight of the violation share in the fitness")
    ap.add_argument("--dtype", choices=["float64", "float32"], default="float64")
    ap.add_argument("--calibrate", action="store_true", help="the band's upper row alone, its bound at the first generation's median gmax")
    args = ap.parse_args()
    p = copy.deepcopy(SC.scenarios()["cstr_cons_pen_norm"]["env_params"])
    p.update(integrator="rk4")
    env = make_vec_env(p, n_envs=P * G, seed=0)
    spec, dev = env.spec, env.device
    dims = [spec.nobs, HIDDEN, spec.na]
    # the device blocks are allocated once, from zeros; every generation rewrites them in place
    pop = PolicyPopulation([np.zeros((P, dims[l + 1], dims[l])) for l in range(len(dims) - 1)],
                           [np.zeros((P, dims[l + 1])) for l in range(len(dims) - 1)],
                           activation="tanh", out_map="clip", out_low=-1.0, out_high=1.0, dtype=args.dtype)
    pop.handle(dev)
    n = pop.n_params
    if args.calibrate:
        A, b = np.asarray(spec.con_A)[1:2], np.asarray(spec.con_b)[1:2]  # (the upper row of the band)
        env.close()
        pilot = make_vec_env(dict(p, constraints={"A": A, "b": b}), n_envs=P * G, seed=0)
        pop.sample_(torch.zeros(n, dtype=torch.float64, device=dev), torch.full((n,), 0.5, dtype=torch.float64, device=dev), SEED,
                    generation=0, check=False)
        shift = float(evaluate_population(pilot, pop, G, gamma=1.0)["gmax"].median())
        pilot.close()
        env = make_vec_env(dict(p, constraints={"A": A, "b": b + shift}), n_envs=P * G, seed=0)
        spec = env.spec
        print(f"calibrated: one row, bound moved by {shift:.3f} to {float(b[0] + shift):.3f}")
    print(f"{P} members x {G} envs, {spec.N - 1} steps, {spec.ncon} constraint rows, one launch per generation; "
          f"{n} parameters per member, fitness = score - {args.lam:g} * viol_share")
    mean = torch.zeros(n, dtype=torch.float64, device=dev)
    std = torch.full((n,), 0.5, dtype=torch.float64, device=dev)
    for it in range(args.iterations):
        pop.sample_(mean, std, SEED, generation=it, check=False)
        out = evaluate_population(env, pop, G, gamma=1.0)
        fitness = out["score"] - args.lam * out["viol_share"]
        elite = torch.topk(fitness, P // 10).indices
        theta = pop.flat(members=elite)
        mean, std = theta.mean(dim=0), theta.std(dim=0, unbiased=False) + 0.02
        best = int(torch.argmax(fitness))
        print(f"CEM generation {it}: best fitness {float(fitness[best]):11.3f}   its return {float(out['score'][best]):11.3f}   "
              f"its violation share {float(out['viol_share'][best]):.4f}   its largest row value {float(out['gmax'].view(-1, G)[best].max()):9.4f}   "
              f"|   population: mean return {float(out['score'].mean()):11.3f}   violation share {float(out['viol_share'].mean()):.4f}   "
              f"members that never violate {int((out['nviol'].view(-1, G).sum(1) == 0).sum())}")
    env.close(), pop.close()


if __name__ == "__main__":
    main()
