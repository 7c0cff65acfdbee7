#!/usr/bin/env python3
"""A population of MLP policies in one fused closed-loop launch (pcg_rollout_policy_pop) against what a caller had before it.

    python tools/population_rollout_bench.py [--B 1048576] [--reps 5] [--shapes affine,1x16,2x64] [--parts 1,2,3] [--dtype float32] [--per-env-params | --constraints [--members 16,256,4096]] [--out FILE]

Workload: the headline's cstr envs (bench.workload_params: RK4, N = 60, dt = 1 s; one episode = 59 closed-loop steps).  All
routes of a comparison alternate inside one process (`reps` rounds after one warm-up round); times are device-event times
around the host calls (so they hold the host's launch overhead, which is what many small launches pay); the figure compared
is the median, the repeats are printed.

  1  cost of per-wave members   the population call with P copies of ONE policy at envs_per_policy = 2^14, 1024 and 64 against
                                rollout_policy with that policy on the same envs (nothing recorded on either side)
  2  against what a caller can do today, P in {16, 256, 4096} distinct members, each scored on B / P envs (reset + one episode
     + the return of every env):
         pop   evaluate_population: one reset, one launch, the returns accumulated in the kernel
         seq   P times: reset of an env of B / P envs, rollout_policy with member m (rewards recorded), their sum
         step  evaluate_population(fused=False): one env.step per step with the population's callable form in torch
  3  benefit of ret_out         the population call returning ret_out alone against recording rew (T x B) and reducing it
                                in torch with the same discounting
  4  float32 members            (the default part under --dtype float32) P in {16, 256, 4096} distinct members on B / P envs each,
                                and 64 envs per member with the last shape: the float32 population, the fp64 population on the
                                same rounded weights, and rollout_policy with ONE float32 policy on the same envs (nothing
                                recorded anywhere)

--dtype float32 makes the populations and policies of parts 1 to 3 float32 ones as well.

--per-env-params measures pcg_rollout_policy_pop_unc instead (and with --dtype float32 its float32 kernel): the workload is
bench.py's cstr_unc (the headline's envs with UA and Caf ~ U(+-5 %) sampled per env at reset), P in --members distinct members
on B / P envs each, all routes interleaved in one process:
  new   the population call on the randomised plan
  c     rollout_population with the same members (two inputs fewer) on the headline's envs WITHOUT uncertain parameters
  d     rollout_policy_unc with ONE policy (member 0) on all envs (fp64 only: there is no float32 single-policy form)
        -- these three with nothing recorded, from a copied-back start state --
  eval  evaluate_population(fused_unc=True): reset, the one launch, the per-member scores
  a     P times: reset of an env of B / P envs, rollout_policy_unc with member m (rewards recorded), their sum (fp64 only)
  b     evaluate_population(fused=False): one env.step per step with the population's callable form in torch

--constraints measures pcg_rollout_policy_pop_cons (with --dtype float32 its float32 kernel): the workload is the scenario
cstr_cons_pen_norm under RK4 (N = 60, one affine row family on the temperature, r_penalty), P in --members distinct members on
B / P envs each, all routes interleaved in one process:
  new   the population call with ret / nviol / gmax alone (no sequence recorded)
  c     rollout_population with the same members on cstr_canonical -- the same envs without the rows: what the rows and the
        two statistics cost
  d     rollout_policy_cons with ONE policy (member 0) on all envs, nothing recorded (fp64 only: no float32 single-policy form)
        -- these three from a copied-back start state --
  eval  evaluate_population: reset, the one launch, scores and violation shares per member
  a     P times: reset of an env of B / P envs, rollout_policy_cons with member m (rewards and flags recorded), their sums (fp64 only)
  b     evaluate_population(fused=False): one env.step per step, the statistics formed in torch
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]

SHAPES = {"affine": (), "1x16": (16,), "2x64": (64, 64)}


def member_arrays(spec, hidden, P, seed=17):
    """fixed-seed weights on the normalised boxes (tools/policy_rollout_bench.py's scaling), P members"""
    rng = np.random.default_rng(seed)
    dims = [spec.nobs, *hidden, spec.na]
    Ws = [rng.standard_normal((P, dims[l + 1], dims[l])) / np.sqrt(dims[l]) for l in range(len(dims) - 1)]
    bs = [0.2 * rng.standard_normal((P, dims[l + 1])) for l in range(len(dims) - 1)]
    Ws[-1] *= 0.8
    return Ws, bs


def timed(torch, routes, reps):
    """{name: [ms per call]} of the routes, interleaved, after one warm-up round"""
    times = {k: [] for k in routes}
    for rep in range(reps + 1):
        for k, fn in routes.items():
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            ev0.record()
            fn()
            ev1.record()
            torch.cuda.synchronize()
            if rep:
                times[k].append(ev0.elapsed_time(ev1))
    return times


def fmt(times):
    return "  ".join(f"{k} {[round(t, 3) for t in v]}" for k, v in times.items())


def part1(a, p, torch, VecEnv, PolicyPopulation, MLPPolicy):
    lines = ["# 1. cost of per-wave members: P copies of one policy, ms per episode of B envs (nothing recorded); base = rollout_policy"]
    for name in a.shapes.split(","):
        env = VecEnv(dict(p), n_envs=a.B, seed=1)
        spec, T = env.spec, env.spec.N - 1
        Ws, bs = member_arrays(spec, SHAPES[name], 1)
        pol = MLPPolicy([w[0] for w in Ws], [b[0] for b in bs], activation="tanh", out_map="clip", out_low=-1.0, out_high=1.0, dtype=a.dtype)
        pops = {}
        for G in (1 << 14, 1024, 64):
            P = (a.B + G - 1) // G
            pops[G] = PolicyPopulation([np.broadcast_to(w, (P,) + w.shape[1:]) for w in Ws], [np.broadcast_to(b, (P,) + b.shape[1:]) for b in bs],
                                       activation="tanh", out_map="clip", out_low=-1.0, out_high=1.0, dtype=a.dtype)
            pops[G].handle(env.device)
        x0, o0 = None, None
        env.reset()
        x0, o0 = env.x.clone(), env.obs_soa.clone()

        def restart():
            env.x.copy_(x0), env.obs_soa.copy_(o0)
            env.t = 0

        def base():
            restart()
            env.rollout_policy(pol, T, collect_rew=False, collect_actions=False)

        def with_pop(G):
            def run():
                restart()
                env.rollout_population(pops[G], T, G, collect_returns=False)
            return run

        routes = {"base": base}
        routes.update({f"G={G}": with_pop(G) for G in pops})
        times = timed(torch, routes, a.reps)
        med = {k: statistics.median(v) for k, v in times.items()}
        block = sum(w[0].size + b[0].size for w, b in zip(Ws, bs)) * 8
        lines.append(f"{name:7s} " + "   ".join(f"{k} {med[k]:8.3f} ms ({med[k] / med['base']:.3f} x base)" for k in med)
                     + f"   (both sides copy x / obs back first; unpadded weights per member {block} B)")
        lines.append("        repeats " + fmt(times))
        env.close(), pol.close()
        for q in pops.values():
            q.close()
        del env, pops
        torch.cuda.empty_cache()
    return lines


def part2(a, p, torch, VecEnv, PolicyPopulation, evaluate_population):
    lines = ["# 2. P distinct members, each scored on B / P envs (reset + episode + per-env return), ms: pop = one population call, "
             "seq = P x (reset, rollout_policy, sum) on an env of B / P, step = per-step route with the callable form"]
    for name in a.shapes.split(","):
        for P in (16, 256, 4096):
            G = a.B // P
            if G < 64 or G % 64:
                continue
            big, big2, small = VecEnv(dict(p), n_envs=a.B, seed=1), VecEnv(dict(p), n_envs=a.B, seed=1), VecEnv(dict(p), n_envs=G, seed=1)
            spec, T = big.spec, big.spec.N - 1
            Ws, bs = member_arrays(spec, SHAPES[name], P)
            pop = PolicyPopulation(Ws, bs, activation="tanh", out_map="clip", out_low=-1.0, out_high=1.0, dtype=a.dtype)
            pop.handle(big.device)
            members = [pop.member(m) for m in range(P)]
            for q in members:
                q.handle(big.device)
            keep = {}

            def f_pop():
                keep["pop"] = evaluate_population(big, pop, G, gamma=1.0)["score"]

            def f_seq():
                s = []
                for q in members:
                    small.reset()
                    s.append(small.rollout_policy(q, T, collect_actions=False)[2].sum(dim=0).mean())
                keep["seq"] = torch.stack(s)

            def f_step():
                keep["step"] = evaluate_population(big2, pop, G, gamma=1.0, fused=False)["score"]

            times = timed(torch, {"pop": f_pop, "seq": f_seq, "step": f_step}, a.reps)
            med = {k: statistics.median(v) for k, v in times.items()}
            gap = float((keep["pop"] - keep["step"]).abs().max())
            lines.append(f"{name:7s} P={P:5d} G={G:6d}   pop {med['pop']:9.3f}   seq {med['seq']:9.3f}   step {med['step']:9.3f} ms   "
                         f"seq / pop = {med['seq'] / med['pop']:.2f}   step / pop = {med['step'] / med['pop']:.2f}   "
                         f"{a.B * T / med['pop'] / 1e-3:.3e} env-steps/s pop   max |score pop - step| {gap:.2e}")
            lines.append("        repeats " + fmt(times))
            for e in (big, big2, small):
                e.close()
            pop.close()
            for q in members:
                q.close()
            del big, big2, small, members, pop
            torch.cuda.empty_cache()
    return lines


def part3(a, p, torch, VecEnv, PolicyPopulation):
    lines = ["# 3. benefit of ret_out (1 x 16 members, envs_per_policy 1024, gamma 0.99), ms per episode: ret = ret_out alone, "
             "rew = rew (T x B) recorded and reduced in torch"]
    env = VecEnv(dict(p), n_envs=a.B, seed=1)
    spec, T, G = env.spec, env.spec.N - 1, 1024
    Ws, bs = member_arrays(spec, SHAPES["1x16"], (a.B + G - 1) // G)
    pop = PolicyPopulation(Ws, bs, activation="tanh", out_map="clip", out_low=-1.0, out_high=1.0, dtype=a.dtype)
    pop.handle(env.device)
    env.reset()
    x0, o0 = env.x.clone(), env.obs_soa.clone()
    disc = torch.as_tensor(0.99 ** np.arange(T), device=env.device).unsqueeze(1)
    keep = {}

    def restart():
        env.x.copy_(x0), env.obs_soa.copy_(o0)
        env.t = 0

    def f_ret():
        restart()
        keep["ret"] = env.rollout_population(pop, T, G, gamma=0.99)["ret"]

    def f_rew():
        restart()
        keep["rew"] = (env.rollout_population(pop, T, G, gamma=0.99, collect_rew=True, collect_returns=False)["rew"] * disc).sum(dim=0)

    times = timed(torch, {"ret": f_ret, "rew": f_rew}, a.reps)
    med = {k: statistics.median(v) for k, v in times.items()}
    gap = float((keep["ret"] - keep["rew"]).abs().max() / keep["ret"].abs().max())
    lines.append(f"ret {med['ret']:8.3f}   rew {med['rew']:8.3f} ms   rew / ret = {med['rew'] / med['ret']:.3f}   "
                 f"({8 * T * a.B / 1e6:.0f} MB of rewards not written and not re-read; relative gap of the two returns {gap:.1e})")
    lines.append("        repeats " + fmt(times))
    env.close(), pop.close()
    return lines


def part4(a, p, torch, VecEnv, PolicyPopulation, MLPPolicy):
    lines = ["# 4. float32 members, ms per episode of B envs (nothing recorded): f32 = the float32 population, f64 = the fp64 population "
             "on the same rounded weights, one32 = rollout_policy with ONE float32 policy (member 0) on the same envs"]
    names = a.shapes.split(",")
    cases = [(name, a.B // P) for name in names for P in (16, 256, 4096)] + [(names[-1], 64)]
    for name, G in cases:
        if G < 64 or G % 64:
            continue
        P = (a.B + G - 1) // G
        env = VecEnv(dict(p), n_envs=a.B, seed=1)
        T = env.spec.N - 1
        Ws, bs = member_arrays(env.spec, SHAPES[name], P)
        kw = dict(activation="tanh", out_map="clip", out_low=-1.0, out_high=1.0)
        pop32 = PolicyPopulation(Ws, bs, dtype="float32", **kw)
        pop64 = PolicyPopulation([w.astype(np.float64) for w in pop32.weights], [b.astype(np.float64) for b in pop32.biases], **kw)
        one32 = pop32.member(0)
        for q in (pop32, pop64, one32):
            q.handle(env.device)
        env.reset()
        x0, o0 = env.x.clone(), env.obs_soa.clone()

        def restart():
            env.x.copy_(x0), env.obs_soa.copy_(o0)
            env.t = 0

        def with_pop(q):
            def run():
                restart()
                env.rollout_population(q, T, G, collect_returns=False)
            return run

        def single():
            restart()
            env.rollout_policy(one32, T, collect_rew=False, collect_actions=False)

        times = timed(torch, {"f32": with_pop(pop32), "f64": with_pop(pop64), "one32": single}, a.reps)
        med = {k: statistics.median(v) for k, v in times.items()}
        lines.append(f"{name:7s} P={P:6d} G={G:6d}   f32 {med['f32']:8.3f}   f64 {med['f64']:8.3f}   one32 {med['one32']:8.3f} ms   "
                     f"f64 / f32 = {med['f64'] / med['f32']:.2f}   f32 / one32 = {med['f32'] / med['one32']:.3f}   "
                     f"({med['f32'] / T * 1e3:.1f} / {med['f64'] / T * 1e3:.1f} / {med['one32'] / T * 1e3:.1f} us per step)")
        lines.append("        repeats " + fmt(times))
        env.close()
        for q in (pop32, pop64, one32):
            q.close()
        del env, pop32, pop64, one32
        torch.cuda.empty_cache()
    return lines


def unc_rows(a, bench, torch, VecEnv, PolicyPopulation, evaluate_population):
    p_unc, p_ref = bench.single_workload("cstr_unc")[1], bench.workload_params()
    f64 = a.dtype == "float64"
    lines = ["# --per-env-params: bench.py's cstr_unc (UA, Caf ~ U(+-5 %) per env), ms: new = pcg_rollout_policy_pop_unc, c = rollout_population "
             "without uncertain parameters, d = rollout_policy_unc with ONE policy on all envs (nothing recorded in the three); eval = "
             "evaluate_population(fused_unc=True), a = P x (reset, rollout_policy_unc, sum) on B / P envs, b = per-step route"]
    kw = dict(activation="tanh", out_map="clip", out_low=-1.0, out_high=1.0, dtype=a.dtype)
    for name in a.shapes.split(","):
        for P in [int(v) for v in a.members.split(",")]:
            G = a.B // P
            if G < 64 or G % 64:
                continue
            big, big2, plain, small = (VecEnv(dict(p_unc), n_envs=a.B, seed=1), VecEnv(dict(p_unc), n_envs=a.B, seed=1),
                                       VecEnv(dict(p_ref), n_envs=a.B, seed=1), VecEnv(dict(p_unc), n_envs=G, seed=1))
            spec, T = big.spec, big.spec.N - 1
            assert spec.nunc == 2 and plain.spec.nobs == spec.nobs - 2 and plain.spec.N == spec.N
            pop = PolicyPopulation(*member_arrays(spec, SHAPES[name], P), **kw)
            pop_c = PolicyPopulation(*member_arrays(plain.spec, SHAPES[name], P), **kw)
            members = [pop.member(m) for m in range(P if f64 else 0)]
            for q in [pop, pop_c] + members:
                q.handle(big.device)
            starts = {}
            for e in (big, plain):
                e.reset()
                starts[e] = (e.x.clone(), e.obs_soa.clone())

            def restart(e):
                e.x.copy_(starts[e][0]), e.obs_soa.copy_(starts[e][1])
                e.t = 0

            def f_new():
                restart(big)
                big.rollout_population_unc(pop, T, G, collect_returns=False)

            def f_c():
                restart(plain)
                plain.rollout_population(pop_c, T, G, collect_returns=False)

            def f_d():
                restart(big)
                big.rollout_policy_unc(members[0], T, collect_rew=False, collect_actions=False)

            keep = {}

            def f_eval():
                keep["eval"] = evaluate_population(big, pop, G, gamma=1.0, fused_unc=True)["score"]

            def f_a():
                sc = []
                for q in members:
                    small.reset()
                    sc.append(small.rollout_policy_unc(q, T, collect_actions=False)[2].sum(dim=0).mean())
                keep["a"] = torch.stack(sc)

            def f_b():
                keep["b"] = evaluate_population(big2, pop, G, gamma=1.0, fused=False)["score"]

            routes = {"new": f_new, "c": f_c, "eval": f_eval, "b": f_b}
            if f64:
                routes.update(d=f_d, a=f_a)
            times = timed(torch, routes, a.reps)
            med = {k: statistics.median(v) for k, v in times.items()}
            gap = float((keep["eval"] - keep["b"]).abs().max())
            row = (f"{name:7s} P={P:5d} G={G:6d}   new {med['new']:9.3f} ({med['new'] / T * 1e3:.1f} us per step)   c {med['c']:9.3f}   "
                   f"new / c = {med['new'] / med['c']:.3f}")
            if f64:
                row += f"   d {med['d']:9.3f}   new / d = {med['new'] / med['d']:.3f}"
            row += f"   |   eval {med['eval']:9.3f}   b {med['b']:9.3f}   b / eval = {med['b'] / med['eval']:.2f}"
            if f64:
                row += f"   a {med['a']:9.3f}   a / eval = {med['a'] / med['eval']:.2f}"
            lines.append(row + f"   {a.B * T / med['eval'] / 1e-3:.3e} env-steps/s eval   max |score eval - b| {gap:.2e}")
            lines.append("        repeats " + fmt(times))
            for e in (big, big2, plain, small):
                e.close()
            for q in [pop, pop_c] + members:
                q.close()
            del big, big2, plain, small, members, pop, pop_c, starts
            torch.cuda.empty_cache()
    return lines


def cons_rows(a, torch, VecEnv, PolicyPopulation, evaluate_population):
    import copy

    import scenarios as SC

    p_con = dict(copy.deepcopy(SC.scenarios()["cstr_cons_pen_norm"]["env_params"]), integrator="rk4")
    p_ref = dict(copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"]), integrator="rk4")
    f64 = a.dtype == "float64"
    lines = ["# --constraints: cstr_cons_pen_norm under rk4, ms: new = pcg_rollout_policy_pop_cons (ret / nviol / gmax alone), c = "
             "rollout_population on cstr_canonical (no rows), d = rollout_policy_cons with ONE policy on all envs (nothing recorded); eval = "
             "evaluate_population, a = P x (reset, rollout_policy_cons, sums) on B / P envs, b = evaluate_population(fused=False)"]
    kw = dict(activation="tanh", out_map="clip", out_low=-1.0, out_high=1.0, dtype=a.dtype)
    for name in a.shapes.split(","):
        for P in [int(v) for v in a.members.split(",")]:
            G = a.B // P
            if G < 64 or G % 64:
                continue
            big, big2, plain, small = (VecEnv(dict(p_con), n_envs=a.B, seed=1), VecEnv(dict(p_con), n_envs=a.B, seed=1),
                                       VecEnv(dict(p_ref), n_envs=a.B, seed=1), VecEnv(dict(p_con), n_envs=G, seed=1))
            spec, T = big.spec, big.spec.N - 1
            assert spec.ncon >= 1 and not plain.spec.ncon and plain.spec.nobs == spec.nobs and plain.spec.N == spec.N == 60
            pop = PolicyPopulation(*member_arrays(spec, SHAPES[name], P), **kw)
            members = [pop.member(m) for m in range(P if f64 else 0)]
            for q in [pop] + members:
                q.handle(big.device)
            starts = {}
            for e in (big, plain):
                e.reset()
                starts[e] = (e.x.clone(), e.obs_soa.clone())

            def restart(e):
                e.x.copy_(starts[e][0]), e.obs_soa.copy_(starts[e][1])
                e.t = 0

            def f_new():
                restart(big)
                big.rollout_population_cons(pop, T, G)

            def f_c():
                restart(plain)
                plain.rollout_population(pop, T, G)

            def f_d():
                restart(big)
                big.rollout_policy_cons(members[0], T, collect_rew=False, collect_actions=False, collect_g=False, collect_viol=False)

            keep = {}

            def f_eval():
                keep["eval"] = evaluate_population(big, pop, G, gamma=1.0)

            def f_a():
                sc, vs = [], []
                for q in members:
                    small.reset()
                    o = small.rollout_policy_cons(q, T, collect_actions=False, collect_g=False)
                    sc.append(o["rew"].sum(dim=0).mean()), vs.append(o["viol"].float().mean())
                keep["a"] = (torch.stack(sc), torch.stack(vs))

            def f_b():
                keep["b"] = evaluate_population(big2, pop, G, gamma=1.0, fused=False)

            routes = {"new": f_new, "c": f_c, "eval": f_eval, "b": f_b}
            if f64:
                routes.update(d=f_d, a=f_a)
            times = timed(torch, routes, a.reps)
            med = {k: statistics.median(v) for k, v in times.items()}
            gap = float((keep["eval"]["score"] - keep["b"]["score"]).abs().max())
            vgap = float((keep["eval"]["viol_share"] - keep["b"]["viol_share"]).abs().max())
            row = (f"{name:7s} P={P:5d} G={G:6d}   new {med['new']:9.3f} ({med['new'] / T * 1e3:.1f} us per step)   c {med['c']:9.3f}   "
                   f"new / c = {med['new'] / med['c']:.3f}")
            if f64:
                row += f"   d {med['d']:9.3f}   new / d = {med['new'] / med['d']:.3f}"
            row += f"   |   eval {med['eval']:9.3f}   b {med['b']:9.3f}   b / eval = {med['b'] / med['eval']:.2f}"
            if f64:
                row += f"   a {med['a']:9.3f}   a / eval = {med['a'] / med['eval']:.2f}"
            lines.append(row + f"   {a.B * T / med['eval'] / 1e-3:.3e} env-steps/s eval   max |score eval - b| {gap:.2e}   "
                         f"max |viol_share eval - b| {vgap:.2e}   mean viol_share {float(keep['eval']['viol_share'].mean()):.3f}")
            lines.append("        repeats " + fmt(times))
            for e in (big, big2, plain, small):
                e.close()
            for q in [pop] + members:
                q.close()
            del big, big2, plain, small, members, pop, starts
            torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="affine,1x16,2x64")
    ap.add_argument("--parts", help="default: 1,2,3; under --dtype float32: 4")
    ap.add_argument("--dtype", choices=["float64", "float32"], default="float64")
    ap.add_argument("--per-env-params", action="store_true", help="bench.py's cstr_unc: pcg_rollout_policy_pop_unc against what a caller had")
    ap.add_argument("--constraints", action="store_true", help="cstr_cons_pen_norm: pcg_rollout_policy_pop_cons against what a caller had")
    ap.add_argument("--members", default="16,256,4096", help="--per-env-params / --constraints: the population sizes P")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    import bench
    from pcgym_amd import MLPPolicy, PolicyPopulation, VecEnv, _lib, evaluate_population

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lib = _lib.load()
    lines = [f"# tools/population_rollout_bench.py  B={a.B} reps={a.reps} dtype={a.dtype}  library build {lib.pcg_build_id().decode()} "
             f"({os.path.relpath(_lib.LIB_PATH, ROOT)}, {os.path.getsize(_lib.LIB_PATH)} bytes)  {torch.cuda.get_device_name(0)}",
             "# cstr, RK4 x 1, N = 60: one episode = 59 closed-loop steps; median of the interleaved repeats"]
    p = bench.workload_params()
    parts = (a.parts or ("4" if a.dtype == "float32" else "1,2,3")).split(",")

    def flush():
        text = "\n".join(lines)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")

    if a.constraints:
        parts = []
        lines += cons_rows(a, torch, VecEnv, PolicyPopulation, evaluate_population)
        flush()
    elif a.per_env_params:
        parts = []
        lines += unc_rows(a, bench, torch, VecEnv, PolicyPopulation, evaluate_population)
        flush()
    if "1" in parts:
        lines += part1(a, p, torch, VecEnv, PolicyPopulation, MLPPolicy)
        flush()
    if "2" in parts:
        lines += part2(a, p, torch, VecEnv, PolicyPopulation, evaluate_population)
        flush()
    if "3" in parts:
        lines += part3(a, p, torch, VecEnv, PolicyPopulation)
        flush()
    if "4" in parts:
        lines += part4(a, p, torch, VecEnv, PolicyPopulation, MLPPolicy)
        flush()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
