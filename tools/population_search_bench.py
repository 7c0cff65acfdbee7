#!/usr/bin/env python3
"""One generation of a policy search around pcg_rollout_policy_pop: the weights born and refitted on the host (what the
package offered before pcg_policy_pop_sample) against the weights born and refitted on the device.

    python tools/population_search_bench.py [--G 256] [--P 256,4096] [--shapes affine,1x16,2x64] [--reps 5] [--dtype float32] [--box NAME] [--out FILE]

Workload: the headline's cstr envs (bench.workload_params: RK4, N = 60, dt = 1 s; one episode = 59 closed-loop steps), P
members, each scored on G envs (B = P G).  All routes of a comparison alternate inside one process (`reps` rounds after one
warm-up round); a time is the wall clock between two device synchronisations around the host calls -- it holds the host's
own work, which is what the comparison is about; the figure compared is the median, the repeats are printed.  Every
generation starts from the same mean and std (the refit is computed and dropped), so the repeats time one workload.

  eval    evaluate_population alone: reset, one launch, the per-member scores (what every route contains)
  cem-a   numpy: theta = mean + std * standard_normal((P, n)); PolicyPopulation.update_ (validate and pack member by member,
          pageable copy); evaluate_population; the scores to the host; refit to the best tenth in numpy
  cem-b   PolicyPopulation.sample_(check=False); evaluate_population; torch.topk; flat(members=elite); refit in torch
  es-a    numpy: antithetic eps, theta = mean + sigma * eps; update_; evaluate_population; centered ranks to the host;
          mean += lr / (P sigma) * (w @ eps)
  es-b    sample_(antithetic, check=False); evaluate_population; centered_ranks; noise_dot; the update in torch

--dtype float32 times the device routes (eval, cem-b, es-b) of a float32 population and, interleaved in the same process, of the
fp64 population of the same shape: eval32 / cem32 / es32 against eval64 / cem64 / es64.
"""
import argparse
import os
import socket
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]

SHAPES = {"affine": (), "1x16": (16,), "2x64": (64, 64)}
SEED, SIGMA, LR = 7, 0.1, 0.05


def timed(torch, routes, reps):
    """{name: [ms per call]} of the routes, interleaved, after one warm-up round"""
    times = {k: [] for k in routes}
    for rep in range(reps + 1):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(rep)
            torch.cuda.synchronize()
            if rep:
                times[k].append((time.perf_counter() - t0) * 1e3)
    return times


def case(a, p, name, P, torch, VecEnv, PolicyPopulation, evaluate_population, centered_ranks):
    G = a.G
    env = VecEnv(dict(p), n_envs=P * G, seed=1)
    spec, dev = env.spec, env.device
    dims = [spec.nobs, *SHAPES[name], spec.na]
    L = len(dims) - 1

    def zeros(dtype="float64"):
        q = PolicyPopulation([np.zeros((P, dims[l + 1], dims[l])) for l in range(L)], [np.zeros((P, dims[l + 1])) for l in range(L)],
                             activation="tanh", out_map="clip", out_low=-1.0, out_high=1.0, dtype=dtype)
        q.handle(dev)
        return q

    if a.dtype == "float32":
        return case_f32(a, env, name, P, zeros("float64"), zeros("float32"), torch, evaluate_population, centered_ranks)
    pop_a, pop_b = zeros(), zeros()
    n = pop_b.n_params
    lay = pop_b.flat_layout()
    mean0, std0 = np.zeros(n), np.full(n, 0.5)
    mean_t, std_t = torch.as_tensor(mean0, device=dev), torch.as_tensor(std0, device=dev)
    sig_t = torch.full((n,), SIGMA, dtype=torch.float64, device=dev)
    rng = np.random.default_rng(0)
    keep = {}

    def unflatten(theta):
        return ([theta[:, s:e].reshape((P,) + shp) for k, l, s, e, shp in lay if k == "W"],
                [theta[:, s:e].reshape((P,) + shp) for k, l, s, e, shp in lay if k == "b"])

    def f_eval(rep):
        keep["eval"] = evaluate_population(env, pop_b, G, gamma=1.0)["score"]

    def cem_a(rep):
        theta = mean0 + std0 * rng.standard_normal((P, n))
        pop_a.update_(*unflatten(theta))
        score = evaluate_population(env, pop_a, G, gamma=1.0)["score"]
        order = torch.argsort(score, descending=True).cpu().numpy()
        elite = theta[order[:max(1, P // 10)]]
        keep["cem-a"] = (elite.mean(axis=0), elite.std(axis=0) + 0.02)

    def cem_b(rep):
        pop_b.sample_(mean_t, std_t, SEED, generation=rep, check=False)
        score = evaluate_population(env, pop_b, G, gamma=1.0)["score"]
        theta = pop_b.flat(members=torch.topk(score, max(1, P // 10)).indices)
        keep["cem-b"] = (theta.mean(dim=0), theta.std(dim=0, unbiased=False) + 0.02)

    def es_a(rep):
        half = rng.standard_normal((P // 2, n))
        eps = np.empty((P, n))
        eps[0::2], eps[1::2] = half, -half
        pop_a.update_(*unflatten(mean0 + SIGMA * eps))
        score = evaluate_population(env, pop_a, G, gamma=1.0)["score"]
        w = centered_ranks(score).cpu().numpy()
        keep["es-a"] = mean0 + (LR / (P * SIGMA)) * (w @ eps)

    def es_b(rep):
        pop_b.sample_(mean_t, sig_t, SEED, generation=rep, antithetic=True, check=False)
        score = evaluate_population(env, pop_b, G, gamma=1.0)["score"]
        g = pop_b.noise_dot(centered_ranks(score), SEED, generation=rep, antithetic=True)
        keep["es-b"] = mean_t + (LR / (P * SIGMA)) * g

    times = timed(torch, {"eval": f_eval, "cem-a": cem_a, "cem-b": cem_b, "es-a": es_a, "es-b": es_b}, a.reps)
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"{name:7s} P={P:5d} G={G:4d} n={n:5d}   eval {med['eval']:9.3f}   cem-a {med['cem-a']:10.3f}   cem-b {med['cem-b']:9.3f}   "
             f"es-a {med['es-a']:10.3f}   es-b {med['es-b']:9.3f} ms   over the evaluation: cem-a +{med['cem-a'] - med['eval']:.3f} "
             f"cem-b +{med['cem-b'] - med['eval']:.3f} es-a +{med['es-a'] - med['eval']:.3f} es-b +{med['es-b'] - med['eval']:.3f} ms   "
             f"cem-a / cem-b = {med['cem-a'] / med['cem-b']:.2f}   es-a / es-b = {med['es-a'] / med['es-b']:.2f}",
             "        repeats " + "  ".join(f"{k} {[round(t, 3) for t in v]}" for k, v in times.items())]
    env.close(), pop_a.close(), pop_b.close()
    del env, pop_a, pop_b
    torch.cuda.empty_cache()
    return lines


def case_f32(a, env, name, P, pop64, pop32, torch, evaluate_population, centered_ranks):
    """the device routes of a float32 population and of the fp64 one, interleaved"""
    G, dev, n = a.G, env.device, pop32.n_params
    mean_t = torch.zeros(n, dtype=torch.float64, device=dev)
    std_t = torch.full((n,), 0.5, dtype=torch.float64, device=dev)
    sig_t = torch.full((n,), SIGMA, dtype=torch.float64, device=dev)
    keep = {}

    def routes(pop, tag):
        def f_eval(rep):
            keep["eval" + tag] = evaluate_population(env, pop, G, gamma=1.0)["score"]

        def cem(rep):
            pop.sample_(mean_t, std_t, SEED, generation=rep, check=False)
            score = evaluate_population(env, pop, G, gamma=1.0)["score"]
            theta = pop.flat(members=torch.topk(score, max(1, P // 10)).indices)
            keep["cem" + tag] = (theta.mean(dim=0), theta.std(dim=0, unbiased=False) + 0.02)

        def es(rep):
            pop.sample_(mean_t, sig_t, SEED, generation=rep, antithetic=True, check=False)
            score = evaluate_population(env, pop, G, gamma=1.0)["score"]
            g = pop.noise_dot(centered_ranks(score), SEED, generation=rep, antithetic=True)
            keep["es" + tag] = mean_t + (LR / (P * SIGMA)) * g

        return {"eval" + tag: f_eval, "cem" + tag: cem, "es" + tag: es}

    # (eval runs on what the last generation left in the blocks: one warm-up sample first, so that no route scores zeros)
    for pop in (pop64, pop32):
        pop.sample_(mean_t, std_t, SEED, generation=0, check=False)
    times = timed(torch, {**routes(pop32, "32"), **routes(pop64, "64")}, a.reps)
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"{name:7s} P={P:5d} G={G:4d} n={n:5d}   " + "   ".join(f"{k} {med[k]:9.3f}" for k in med) + " ms   "
             f"eval64 / eval32 = {med['eval64'] / med['eval32']:.2f}   cem64 / cem32 = {med['cem64'] / med['cem32']:.2f}   "
             f"es64 / es32 = {med['es64'] / med['es32']:.2f}   over the evaluation: cem32 +{med['cem32'] - med['eval32']:.3f} "
             f"es32 +{med['es32'] - med['eval32']:.3f} cem64 +{med['cem64'] - med['eval64']:.3f} es64 +{med['es64'] - med['eval64']:.3f} ms",
             "        repeats " + "  ".join(f"{k} {[round(t, 3) for t in v]}" for k, v in times.items())]
    env.close(), pop64.close(), pop32.close()
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", type=int, default=256)
    ap.add_argument("--P", default="256,4096")
    ap.add_argument("--shapes", default="affine,1x16,2x64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", choices=["float64", "float32"], default="float64")
    ap.add_argument("--box", default=socket.gethostname())
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    import bench
    from pcgym_amd import PolicyPopulation, VecEnv, _lib, centered_ranks, evaluate_population

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lib = _lib.load()
    lines = [f"# tools/population_search_bench.py  G={a.G} reps={a.reps} dtype={a.dtype}  box {a.box}  library build {lib.pcg_build_id().decode()} "
             f"({os.path.relpath(_lib.LIB_PATH, ROOT)}, {os.path.getsize(_lib.LIB_PATH)} bytes)  {torch.cuda.get_device_name(0)}",
             "# cstr, RK4 x 1, N = 60: one generation = sample P members, score each on G envs over one episode (59 steps), refit; "
             "wall-clock ms between device synchronisations, median of the interleaved repeats",
             "# eval = evaluate_population alone; -a = weights born and refitted on the host (numpy normals, update_, host refit); "
             "-b = on the device (sample_, flat(members=elite) / noise_dot)"]
    p = bench.workload_params()
    for name in a.shapes.split(","):
        for P in (int(v) for v in a.P.split(",")):
            lines += case(a, p, name, P, torch, VecEnv, PolicyPopulation, evaluate_population, centered_ranks)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
