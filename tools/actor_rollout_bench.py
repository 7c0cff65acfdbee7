#!/usr/bin/env python3
"""On-policy data collection with a stochastic actor-critic: the fused call (pcg_rollout_actor: actor, Gaussian sample,
log-probability and critic evaluated in the rollout kernel) against the per-step route with the same networks, and against
the deterministic fused call (pcg_rollout_policy) with the same actor.

    python tools/actor_rollout_bench.py [--B 1048576] [--reps 5] [--shapes affine,1x16,2x64] [--dtype float32] [--out FILE]

Workload: the headline's cstr envs (bench.workload_params: RK4, N = 60, dt = 1 s).  Four routes alternate inside one process
(`reps` rounds after one warm-up round); times are device-event times of whole episodes (reset included), the figure
compared is the median:
    a   collect_onpolicy(env, ac)                fused, actor + critic of the same hidden shape, GAE included
    b   collect_onpolicy(env, ac, fused=False)   its per-step route: pcg_policy_noise + torch networks + pcg_step per step
    c   collect_rollouts(env, policy=ac.actor)   the deterministic fused call, same actor
    a0  reset + VecEnv.rollout_actor without a critic (samples, log-probabilities, observations, rewards recorded)
The condition: a is not slower than b for any shape (collect_onpolicy takes the fused call wherever the plan qualifies).
With --constraints the workload is the constraint showcase (scenario cstr_cons_pen_norm under integrator="rk4") and three routes
alternate: ac = collect_onpolicy(env, ac, record_cons=True), fused (pcg_rollout_actor_cons: rows and flags of every step
recorded); bc = the same with fused=False, its per-step route; au = collect_onpolicy fused on the unconstrained cstr_canonical
under rk4, the reference for what the 8 * ncon + 1 recorded bytes per env step cost.
With --per-env-params the workload is bench.py's cstr_unc (UA, Caf ~ U(+-5 %) sampled per env at reset) and three routes
alternate: a = collect_onpolicy fused (pcg_rollout_actor_unc), b = the same with fused=False on the same plan, c =
collect_onpolicy fused on the headline's envs without uncertain parameters.
With --dtype float32 three routes alternate instead: a32 = collect_onpolicy fused with float32 networks, a64 = the same with
float64 networks of the same (rounded) weights, b32 = the per-step route of the float32 networks.
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")]

from policy_rollout_bench import SHAPES, make_policy, policy_fmas, widened  # noqa: E402


def make_ac(spec, hidden, critic=True, seed=17, dtype="float64"):
    """policy_rollout_bench's actor, sigma = exp(-1.5) (0.22 of the normalised action half width), a critic of the same shape"""
    from pcgym_amd import GaussianActorCritic, MLPPolicy

    actor = make_policy(spec, hidden, seed, dtype=dtype)
    cr = None
    if critic:
        c = make_policy(spec, hidden, seed + 100, dtype=dtype)
        cr = MLPPolicy(c.weights[:-1] + [c.weights[-1][:1]], c.biases[:-1] + [c.biases[-1][:1]], activation="tanh", out_map="none", dtype=dtype)
    return GaussianActorCritic(actor, np.full(spec.na, -1.5), cr)


def f32_rows(a, p, VecEnv, collect_onpolicy, torch):
    from pcgym_amd import GaussianActorCritic

    lines = ["# float32 networks: a32 = collect_onpolicy fused float32, a64 = fused float64 on the same rounded weights (the baseline), "
             "b32 = per-step route of the float32 networks"]
    for name in a.shapes.split(","):
        envs = {k: VecEnv(dict(p), n_envs=a.B, seed=1) for k in ("a32", "a64", "b32")}
        spec = envs["a32"].spec
        ac = make_ac(spec, SHAPES[name], dtype="float32")
        ac64 = GaussianActorCritic(widened(ac.actor), ac.log_std, widened(ac.critic))
        steps = spec.N - 1
        routes = {"a32": lambda: collect_onpolicy(envs["a32"], ac), "a64": lambda: collect_onpolicy(envs["a64"], ac64),
                  "b32": lambda: collect_onpolicy(envs["b32"], ac, fused=False)}
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
        verdict = "float32 faster than float64" if med["a32"] < med["a64"] else "FLOAT32 NOT FASTER THAN FLOAT64"
        lines.append(f"{name:7s} a32 {us['a32']:8.2f}  a64 {us['a64']:8.2f}  b32 {us['b32']:8.2f} us/step   a64 / a32 = {med['a64'] / med['a32']:.2f}   "
                     f"b32 / a32 = {med['b32'] / med['a32']:.2f}   {a.B * steps / med['a32'] / 1e-3:.3e} env-steps/s fused float32   "
                     f"FMAs per env step: actor {policy_fmas(ac.actor)}, critic {policy_fmas(ac.critic)}   {verdict}")
        lines.append("        repeats (ms per episode) " + "  ".join(f"{k} {[round(t, 2) for t in times[k]]}" for k in times))
        for e in envs.values():
            e.close()
        ac.close(), ac64.close()
        del envs
        torch.cuda.empty_cache()
    return lines


def cons_rows(a, VecEnv, collect_onpolicy, torch):
    import copy

    import scenarios as SC

    p = dict(copy.deepcopy(SC.scenarios()["cstr_cons_pen_norm"]["env_params"]), integrator="rk4")
    p_ref = dict(copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"]), integrator="rk4")
    lines = ["# --constraints: cstr_cons_pen_norm, integrator rk4: ac = collect_onpolicy(record_cons=True) fused (pcg_rollout_actor_cons), "
             "bc = its per-step route, au = collect_onpolicy fused on the unconstrained cstr_canonical, rk4"]
    for name in a.shapes.split(","):
        envs = {"ac": VecEnv(dict(p), n_envs=a.B, seed=1), "bc": VecEnv(dict(p), n_envs=a.B, seed=1), "au": VecEnv(dict(p_ref), n_envs=a.B, seed=1)}
        spec = envs["ac"].spec
        assert spec.ncon and (envs["au"].spec.nobs, envs["au"].spec.na, envs["au"].spec.N) == (spec.nobs, spec.na, spec.N)
        ac = make_ac(spec, SHAPES[name])
        steps = spec.N - 1
        routes = {"ac": lambda: collect_onpolicy(envs["ac"], ac, record_cons=True),
                  "bc": lambda: collect_onpolicy(envs["bc"], ac, record_cons=True, fused=False), "au": lambda: collect_onpolicy(envs["au"], ac)}
        times = {k: [] for k in routes}
        viol = float("nan")
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
                if rep == 0 and k == "ac":
                    viol = float(d["viol"].double().mean())
                del d
        med = {k: statistics.median(v) for k, v in times.items()}
        us = {k: 1e3 * med[k] / steps for k in med}
        extra = (8 * spec.ncon + 1) * a.B * steps
        verdict = "fused not slower than per-step" if med["ac"] <= med["bc"] else "FUSED SLOWER THAN PER-STEP"
        lines.append(f"{name:7s} ac {us['ac']:8.2f}  bc {us['bc']:8.2f}  au {us['au']:8.2f} us/step   bc / ac = {med['bc'] / med['ac']:.2f}   "
                     f"ac / au = {med['ac'] / med['au']:.3f}   ac - au = {med['ac'] - med['au']:.3f} ms per episode for {extra / 1e6:.1f} MB of rows and "
                     f"flags (ncon = {spec.ncon})   {a.B * steps / med['ac'] / 1e-3:.3e} env-steps/s fused   entries violated {viol:.3f}   {verdict}")
        lines.append("        repeats (ms per episode) " + "  ".join(f"{k} {[round(t, 2) for t in times[k]]}" for k in times))
        for e in envs.values():
            e.close()
        ac.close()
        del envs
        torch.cuda.empty_cache()
    return lines


def unc_rows(a, bench, VecEnv, collect_onpolicy, torch):
    p_unc, p_ref = bench.single_workload("cstr_unc")[1], bench.workload_params()
    lines = ["# --per-env-params: bench.py's cstr_unc (UA, Caf ~ U(+-5 %) per env): a = collect_onpolicy fused (pcg_rollout_actor_unc), "
             "b = its per-step route on the same plan, c = collect_onpolicy fused on the headline's envs without uncertain parameters"]
    for name in a.shapes.split(","):
        envs = {"a": VecEnv(dict(p_unc), n_envs=a.B, seed=1), "b": VecEnv(dict(p_unc), n_envs=a.B, seed=1), "c": VecEnv(dict(p_ref), n_envs=a.B, seed=1)}
        spec, spec_c = envs["a"].spec, envs["c"].spec
        assert spec.nunc == 2 and not spec_c.nunc and (spec_c.nobs + spec.nunc, spec_c.na, spec_c.N) == (spec.nobs, spec.na, spec.N)
        ac, ac_c = make_ac(spec, SHAPES[name]), make_ac(spec_c, SHAPES[name])
        steps = spec.N - 1
        routes = {"a": lambda: collect_onpolicy(envs["a"], ac, fused_unc=True), "b": lambda: collect_onpolicy(envs["b"], ac, fused=False),
                  "c": lambda: collect_onpolicy(envs["c"], ac_c)}
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
                     f"{a.B * steps / med['a'] / 1e-3:.3e} env-steps/s fused   FMAs per env step: actor {policy_fmas(ac.actor)}, critic "
                     f"{policy_fmas(ac.critic)}   {verdict}")
        lines.append("        repeats (ms per episode) " + "  ".join(f"{k} {[round(t, 2) for t in times[k]]}" for k in times))
        for e in envs.values():
            e.close()
        ac.close(), ac_c.close()
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
        ap.error("--constraints: the constrained kernels take float64 networks")
    if a.per_env_params and (a.dtype != "float64" or a.constraints):
        ap.error("--per-env-params: float64 networks, no constraint rows")
    import torch

    import bench
    from pcgym_amd import VecEnv, _lib, collect_onpolicy, collect_rollouts

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lib = _lib.load()
    lines = [f"# tools/actor_rollout_bench.py  B={a.B} reps={a.reps}  library build {lib.pcg_build_id().decode()} "
             f"({os.path.relpath(_lib.LIB_PATH, ROOT)})  {torch.cuda.get_device_name(0)}",
             "# cstr, RK4 x 1, N = 60: one episode = 59 closed-loop steps; us per step, median of the interleaved repeats",
             "# a = collect_onpolicy fused (actor + critic), b = its per-step route, c = deterministic pcg_rollout_policy "
             "(same actor), a0 = fused without a critic"]
    p = bench.workload_params()
    if a.dtype == "float32":
        lines += f32_rows(a, p, VecEnv, collect_onpolicy, torch)
    if a.constraints:
        lines = lines[:1] + cons_rows(a, VecEnv, collect_onpolicy, torch)
    if a.per_env_params:
        lines = lines[:1] + unc_rows(a, bench, VecEnv, collect_onpolicy, torch)
    for name in ([] if a.dtype == "float32" or a.constraints or a.per_env_params else a.shapes.split(",")):
        envs = {k: VecEnv(dict(p), n_envs=a.B, seed=1) for k in ("a", "b", "c", "a0")}
        spec = envs["a"].spec
        ac, ac0 = make_ac(spec, SHAPES[name]), make_ac(spec, SHAPES[name], critic=False)
        steps = spec.N - 1

        def no_critic():
            envs["a0"].reset()
            return envs["a0"].rollout_actor(ac0, steps, collect_obs=True, record_next_action=True)

        routes = {"a": lambda: collect_onpolicy(envs["a"], ac), "b": lambda: collect_onpolicy(envs["b"], ac, fused=False),
                  "c": lambda: collect_rollouts(envs["c"], policy=ac.actor), "a0": no_critic}
        times = {k: [] for k in routes}
        clipped = float("nan")
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
                if rep == 0 and k == "a":
                    clipped = float(((d["act"] < -1.0) | (d["act"] > 1.0)).double().mean())
                del d
        med = {k: statistics.median(v) for k, v in times.items()}
        us = {k: 1e3 * med[k] / steps for k in med}
        fm_a, fm_c = policy_fmas(ac.actor), policy_fmas(ac.critic)
        verdict = "fused not slower than per-step" if med["a"] <= med["b"] else "FUSED SLOWER THAN PER-STEP"
        lines.append(f"{name:7s} a {us['a']:8.2f}  b {us['b']:8.2f}  c {us['c']:8.2f}  a0 {us['a0']:8.2f} us/step   "
                     f"a / b = {med['a'] / med['b']:.3f} (b / a = {med['b'] / med['a']:.2f})   a / c = {med['a'] / med['c']:.3f}   "
                     f"a0 / c = {med['a0'] / med['c']:.3f}   {a.B * steps / med['a'] / 1e-3:.3e} env-steps/s fused   "
                     f"FMAs per env step: actor {fm_a}, critic {fm_c}   samples clipped {clipped:.3f}   {verdict}")
        lines.append("        repeats (ms per episode) " + "  ".join(f"{k} {[round(t, 2) for t in times[k]]}" for k in times))
        for e in envs.values():
            e.close()
        ac.close(), ac0.close()
        del envs
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
