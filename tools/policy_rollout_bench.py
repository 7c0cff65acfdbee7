#!/usr/bin/env python3
"""Closed-loop rollout with an MLP policy: the fused call (pcg_rollout_policy: the policy evaluated in the rollout kernel)
against the per-step route (collect_rollouts with the same policy as a torch callable: one pcg_step launch and one torch
evaluation per step, obs and a through HBM) -- the reference's policy_eval.rollout loop, policy_evaluation.py:71-130.

    python tools/policy_rollout_bench.py [--B 1048576] [--reps 5] [--shapes affine,1x16,2x64] [--dtype float32] [--out FILE]

Workload: the headline's cstr envs (bench.workload_params: RK4, N = 60, dt = 1 s), both routes through collect_rollouts, so
both produce the reference's x (Nx, N, B) / u (na, N, B) / r (1, N, B) arrays.  The two routes alternate inside one
process (`reps` pairs after one warm-up pair each); times are device-event times of whole episodes, the figure compared is
the median.  The 2 x 64 policy is also reported as a share of the fp64 vector peak (FMAs of the policy alone).
With --constraints the workload is the constraint showcase (scenario cstr_cons_pen_norm under integrator="rk4": two affine rows,
r_penalty): the fused call is pcg_rollout_policy_cons, which also records the rows of every step into g; the per-step route
records them from env.g; a third route, the unconstrained fused call on cstr_canonical under rk4, alternates with them as the
reference for what the rows cost (8 * ncon recorded bytes per env step; the collector does not ask for the flags).
With --per-env-params the workload is bench.py's cstr_unc (the headline's envs with UA and Caf ~ U(+-5 %) sampled per env at
reset) and three routes alternate: a = the fused call (pcg_rollout_policy_unc), b = the per-step route on the same plan
(step_kernel<..., UNC>), c = the existing fused
call on the headline's envs without uncertain parameters (two observation slots fewer).
With --dtype float32 three routes alternate: the float32 fused call (rollout_policy_kernel_f32), the float64 fused call on the
same (float32-rounded) weights, and the per-step route with the float32 callable.
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]

SHAPES = {"affine": (), "1x16": (16,), "2x64": (64, 64)}
FP64_VECTOR_PEAK = 78.6e12  # MI355X, FLOP/s (spec: half the fp32 vector rate)


def make_policy(spec, hidden, seed=17, dtype="float64"):
    """fixed-seed weights on the normalised observation / action boxes: unsaturated units, outputs mostly inside [-1, 1]"""
    from pcgym_amd import MLPPolicy

    rng = np.random.default_rng(seed)
    dims = [spec.nobs, *hidden, spec.na]
    Ws = [rng.standard_normal((dims[l + 1], dims[l])) / np.sqrt(dims[l]) for l in range(len(dims) - 1)]
    bs = [0.2 * rng.standard_normal(dims[l + 1]) for l in range(len(dims) - 1)]
    Ws[-1] *= 0.8
    if dtype == "float32":  # (both dtypes of a comparison hold the same, float32-rounded, weights)
        Ws, bs = [w.astype(np.float32) for w in Ws], [b.astype(np.float32) for b in bs]
        return MLPPolicy(Ws, bs, activation="tanh", out_map="clip", out_low=-1.0, out_high=1.0, dtype="float32")
    return MLPPolicy(Ws, bs, activation="tanh", out_map="clip", out_low=-1.0, out_high=1.0)


def widened(pol):
    """the float64 policy with a float32 policy's weights"""
    from pcgym_amd import MLPPolicy

    return MLPPolicy(pol.weights, pol.biases, activation=pol.activation, out_map=pol.out_map, out_low=pol.out_low, out_high=pol.out_high)


def policy_fmas(pol):
    return sum(int(w.size) for w in pol.weights)


def f32_rows(a, p, VecEnv, collect_rollouts, torch):
    """the float32 comparison: fused32 / fused64 / per_step32 interleaved, us per step"""
    lines = ["# float32 policy: f32 = fused float32 call, f64 = fused float64 call on the same rounded weights (the baseline), "
             "ps32 = per-step route with the float32 callable"]
    for name in a.shapes.split(","):
        envs = {k: VecEnv(dict(p), n_envs=a.B, seed=1) for k in ("f32", "f64", "ps32")}
        spec = envs["f32"].spec
        pol = make_policy(spec, SHAPES[name], dtype="float32")
        pol64 = widened(pol)
        steps = spec.N - 1
        routes = {"f32": lambda: collect_rollouts(envs["f32"], policy=pol), "f64": lambda: collect_rollouts(envs["f64"], policy=pol64),
                  "ps32": lambda: collect_rollouts(envs["ps32"], policy=lambda o: pol(o))}
        times = {k: [] for k in routes}
        gap = float("nan")
        for rep in range(a.reps + 1):  # (round 0 warms every route up)
            u = {}
            for k, fn in routes.items():
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                ev0.record()
                d = fn()
                ev1.record()
                torch.cuda.synchronize()
                if rep:
                    times[k].append(ev0.elapsed_time(ev1))
                if rep == 0 and k != "ps32":
                    u[k] = d["u"][:, 0].clone()  # the first action: the same observation on both routes
                del d
            if rep == 0:
                gap = float((u["f32"] - u["f64"]).abs().max())
        med = {k: statistics.median(v) for k, v in times.items()}
        us = {k: 1e3 * med[k] / steps for k in med}
        verdict = "float32 faster than float64" if med["f32"] < med["f64"] else "FLOAT32 NOT FASTER THAN FLOAT64"
        lines.append(f"{name:7s} f32 {us['f32']:8.2f}  f64 {us['f64']:8.2f}  ps32 {us['ps32']:8.2f} us/step   f64 / f32 = {med['f64'] / med['f32']:.2f}   "
                     f"ps32 / f32 = {med['ps32'] / med['f32']:.2f}   {a.B * steps / med['f32'] / 1e-3:.3e} env-steps/s fused float32   "
                     f"policy FMAs per env step {policy_fmas(pol)}   first action f32 vs f64: max |diff| {gap:.2e}   {verdict}")
        lines.append("        repeats (ms per episode) " + "  ".join(f"{k} {[round(t, 2) for t in times[k]]}" for k in times))
        for e in envs.values():
            e.close()
        pol.close(), pol64.close()
        del envs
        torch.cuda.empty_cache()
    return lines


def unc_rows(a, bench, VecEnv, collect_rollouts, torch):
    """the per-env-parameter comparison: a / b / c interleaved, us per step"""
    p_unc, p_ref = bench.single_workload("cstr_unc")[1], bench.workload_params()
    lines = ["# --per-env-params: bench.py's cstr_unc (UA, Caf ~ U(+-5 %) per env): a = fused (pcg_rollout_policy_unc), b = per-step route on the "
             "same plan, c = fused (pcg_rollout_policy) on the headline's envs without uncertain parameters"]
    for name in a.shapes.split(","):
        envs = {"a": VecEnv(dict(p_unc), n_envs=a.B, seed=1), "b": VecEnv(dict(p_unc), n_envs=a.B, seed=1), "c": VecEnv(dict(p_ref), n_envs=a.B, seed=1)}
        spec, spec_c = envs["a"].spec, envs["c"].spec
        assert spec.nunc == 2 and not spec_c.nunc and (spec_c.nobs + spec.nunc, spec_c.na, spec_c.N) == (spec.nobs, spec.na, spec.N)
        pol, pol_c = make_policy(spec, SHAPES[name]), make_policy(spec_c, SHAPES[name])
        steps = spec.N - 1
        routes = {"a": lambda: collect_rollouts(envs["a"], policy=pol, fused_unc=True), "b": lambda: collect_rollouts(envs["b"], policy=lambda o: pol(o)),
                  "c": lambda: collect_rollouts(envs["c"], policy=pol_c)}
        times = {k: [] for k in routes}
        for rep in range(a.reps + 1):  # (round 0 warms every route up)
            for k, fn in routes.items():
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                ev0.record()
                d = fn()
                ev1.record()
                torch.cuda.synchronize()
                if rep:
                    times[k].append(ev0.elapsed_time(ev1))
                del d
        med = {k: statistics.median(v) for k, v in times.items()}
        us = {k: 1e3 * med[k] / steps for k in med}
        verdict = "fused faster than per-step" if med["a"] < med["b"] else "FUSED NOT FASTER THAN PER-STEP"
        lines.append(f"{name:7s} a {us['a']:8.2f}  b {us['b']:8.2f}  c {us['c']:8.2f} us/step   b / a = {med['b'] / med['a']:.2f}   a / c = {med['a'] / med['c']:.3f}   "
                     f"{a.B * steps / med['a'] / 1e-3:.3e} env-steps/s fused   policy FMAs per env step {policy_fmas(pol)} (c: {policy_fmas(pol_c)})   {verdict}")
        lines.append("        repeats (ms per episode) " + "  ".join(f"{k} {[round(t, 2) for t in times[k]]}" for k in times))
        for e in envs.values():
            e.close()
        pol.close(), pol_c.close()
        del envs
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="affine,1x16,2x64")
    ap.add_argument("--dtype", default="float64", choices=["float64", "float32"])
    ap.add_argument("--constraints", action="store_true", help="the constraint showcase: fused-cons against per-step (and the unconstrained fused call)")
    ap.add_argument("--per-env-params", action="store_true", help="bench.py's cstr_unc: fused-unc against per-step (and the fused call without parameters)")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.constraints and a.dtype != "float64":
        ap.error("--constraints: the constrained kernels take float64 policies")
    if a.per_env_params and (a.dtype != "float64" or a.constraints):
        ap.error("--per-env-params: float64 policies, no constraint rows")
    import torch

    import bench
    from pcgym_amd import VecEnv, _lib, collect_rollouts

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lib = _lib.load()
    lines = [f"# tools/policy_rollout_bench.py  B={a.B} reps={a.reps}  library build {lib.pcg_build_id().decode()} "
             f"({os.path.relpath(_lib.LIB_PATH, ROOT)})  {torch.cuda.get_device_name(0)}",
             "# cstr, RK4 x 1, N = 60: one episode = 59 closed-loop steps; ms per episode, median of the interleaved repeats"]
    p = bench.workload_params()
    p_ref = None
    if a.constraints:
        import copy

        import scenarios as SC

        p = dict(copy.deepcopy(SC.scenarios()["cstr_cons_pen_norm"]["env_params"]), integrator="rk4")
        p_ref = dict(copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"]), integrator="rk4")
        lines[1] = ("# --constraints: cstr_cons_pen_norm, integrator rk4 (fused = pcg_rollout_policy_cons, rows recorded); uncon = the "
                    "unconstrained fused call on cstr_canonical, rk4; ms per episode, median of the interleaved repeats")
    if a.dtype == "float32":
        lines += f32_rows(a, p, VecEnv, collect_rollouts, torch)
    if a.per_env_params:
        lines = lines[:1] + unc_rows(a, bench, VecEnv, collect_rollouts, torch)
    for name in ([] if a.dtype == "float32" or a.per_env_params else a.shapes.split(",")):
        e_f, e_s = VecEnv(dict(p), n_envs=a.B, seed=1), VecEnv(dict(p), n_envs=a.B, seed=1)
        spec = e_f.spec
        pol = make_policy(spec, SHAPES[name])
        steps = spec.N - 1
        routes = {"fused": lambda: collect_rollouts(e_f, policy=pol), "per_step": lambda: collect_rollouts(e_s, policy=lambda o: pol(o))}
        e_u = None
        if p_ref is not None:
            e_u = VecEnv(dict(p_ref), n_envs=a.B, seed=1)
            assert spec.ncon and (e_u.spec.nobs, e_u.spec.na, e_u.spec.N) == (spec.nobs, spec.na, spec.N)
            routes["uncon"] = lambda: collect_rollouts(e_u, policy=pol)
        times = {k: [] for k in routes}
        for rep in range(a.reps + 1):  # (pair 0 warms both routes up)
            for k, fn in routes.items():
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                ev0.record()
                d = fn()
                ev1.record()
                torch.cuda.synchronize()
                if rep:
                    times[k].append(ev0.elapsed_time(ev1))
                if rep == 0 and k == "fused":
                    inside = float(((d["u"] > spec.a_low[0]) & (d["u"] < spec.a_high[0])).double().mean())
                del d
        med = {k: statistics.median(v) for k, v in times.items()}
        us = {k: 1e3 * med[k] / steps for k in med}
        fm = policy_fmas(pol)
        share = 2.0 * fm * a.B * steps / (med["fused"] * 1e-3) / FP64_VECTOR_PEAK
        lines.append(f"{name:7s} fused {med['fused']:9.3f} ms ({us['fused']:8.2f} us/step, {a.B * steps / med['fused'] / 1e-3:.3e} env-steps/s)   "
                     f"per-step {med['per_step']:9.3f} ms ({us['per_step']:8.2f} us/step, {a.B * steps / med['per_step'] / 1e-3:.3e} env-steps/s)   "
                     f"per-step / fused = {med['per_step'] / med['fused']:.2f}   policy FMAs per env step {fm}, "
                     f"= {100 * share:.1f} % of the fp64 vector peak in the fused call   actions inside the box {inside:.2f}")
        lines.append(f"        fused repeats {[round(t, 3) for t in times['fused']]}  per-step repeats {[round(t, 3) for t in times['per_step']]}")
        if e_u is not None:
            extra = 8 * spec.ncon * a.B * steps  # bytes of recorded rows per episode
            lines.append(f"        uncon {med['uncon']:9.3f} ms ({us['uncon']:8.2f} us/step)   fused-cons / uncon = {med['fused'] / med['uncon']:.3f}   "
                         f"fused-cons - uncon = {med['fused'] - med['uncon']:.3f} ms for {extra / 1e6:.1f} MB of rows "
                         f"(ncon = {spec.ncon})   uncon repeats {[round(t, 3) for t in times['uncon']]}")
            e_u.close()
        e_f.close(), e_s.close(), pol.close()
        del e_f, e_s
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
