#!/usr/bin/env python3
"""Fused closed-loop rollouts on a plan with run-time compiled code: the cstr written out by a user as a custom_model
(PCG_MODEL_USER), whose closed-loop kernels come from the plan's second run-time compiled module, against the per-step route
on the same plan and against the built-in cstr's ahead-of-time kernels.

    python tools/user_closed_loop_bench.py [--B 1048576] [--reps 5] [--shapes affine,1x16,2x64] [--out FILE]
    python tools/user_closed_loop_bench.py --first-call [--reps 3] [--out FILE]     (appends to FILE)

Workload: the headline's cstr envs (bench.workload_params: RK4, N = 60, dt = 1 s).  Per shape and per head (policy:
collect_rollouts; actor-critic: collect_onpolicy) three routes alternate inside one process (`reps` rounds after one warm-up
round, which also builds the closed-loop module); times are device-event times of whole episodes, the figure compared is the
median:
    1  user_fused     the hand-written cstr, ONE launch per episode (the run-time compiled closed-loop kernel)
    2  user_per_step  the same plan, one launch and one torch evaluation of the same networks per step
    3  builtin_fused  the built-in cstr, one launch per episode (the ahead-of-time kernel)

--first-call: what the first closed-loop call of such a plan costs.  Each figure comes from a fresh process with a private
cache directory ($PCG_JIT_CACHE): pcg_plan_create and pcg_plan_prepare_closed_loop cold (hipRTC) and then warm (a second
process finds both code objects on disk).  --create-only times pcg_plan_create alone, for a tree without the function.
"""
import argparse
import copy
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")]

# the reference's cstr (model_classes.py:45-62) written out by a user: CSTR_BY_HAND of tests/test_gpu_user_model.py
CSTR_BY_HAND = {
    "states": ["Ca", "T"], "inputs": ["Tc"], "disturbances": ["Ti", "Caf"],
    "parameters": {"q": 100, "V": 100, "rho": 1000, "C": 0.239, "deltaHr": -5e4, "EA_over_R": 8750, "k0": 7.2e10,
                   "UA": 5e4, "Ti": 350, "Caf": 1},
    "aux": {"rA": "k0*exp(-EA_over_R/T)*Ca"},
    "rhs": ["q/V*(Caf - Ca) - rA", "q/V*(Ti - T) + ((-deltaHr)*rA)*(1/(rho*C)) + UA*(Tc - T)*(1/(rho*C*V))"],
}


def user_params():
    import bench

    p = bench.workload_params()
    p.pop("model")
    p["custom_model"] = copy.deepcopy(CSTR_BY_HAND)
    return p


def first_call_child(create_only):
    """one process: (seconds of pcg_plan_create, seconds of pcg_plan_prepare_closed_loop or nan) of the hand-written cstr"""
    import torch

    from pcgym_amd import _lib
    from pcgym_amd.config import EnvSpec

    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")  # (the context exists before the clock starts)
    torch.cuda.synchronize()
    lib = _lib.load()
    cfg, keep = EnvSpec(user_params()).to_cfg()
    plan = C.c_void_p()
    t0 = time.perf_counter()
    rc = lib.pcg_plan_create(C.byref(plan), C.byref(cfg))
    t1 = time.perf_counter()
    assert rc == 0, rc
    t_prep = float("nan")
    if not create_only:
        rc = lib.pcg_plan_prepare_closed_loop(plan)
        t2 = time.perf_counter()
        assert rc == 0, rc
        t_prep = t2 - t1
        assert lib.pcg_plan_prepare_closed_loop(plan) == 0
    lib.pcg_plan_destroy(plan)
    print(f"FIRST_CALL {t1 - t0:.4f} {t_prep:.4f}")


def first_call(a):
    import torch

    from pcgym_amd import _lib

    lines = [f"# tools/user_closed_loop_bench.py --first-call  library build {_lib.load().pcg_build_id().decode()}  "
             f"{torch.cuda.get_device_name(0)}",
             "# the hand-written cstr, RK4; seconds, one fresh process per figure, a private cache directory per pair; "
             "cold = hipRTC, warm = the code objects on disk"]
    rows = []
    for rep in range(a.reps):
        with tempfile.TemporaryDirectory(prefix="pcg_jit_bench_") as d:
            pair = []
            for state in ("cold", "warm"):
                cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (["--create-only"] if a.create_only else [])
                r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, PCG_JIT_CACHE=os.path.join(d, "jit")),
                                   timeout=900)
                assert r.returncode == 0, r.stderr[-2000:]
                c, p = (float(v) for v in [l for l in r.stdout.splitlines() if l.startswith("FIRST_CALL")][0].split()[1:])
                pair.append((c, p))
            rows.append(pair)
            lines.append(f"pair {rep}: pcg_plan_create cold {pair[0][0]:.3f} warm {pair[1][0]:.3f}   "
                         f"pcg_plan_prepare_closed_loop cold {pair[0][1]:.3f} warm {pair[1][1]:.3f}")
    for i, what in enumerate(("pcg_plan_create", "pcg_plan_prepare_closed_loop")):
        for j, state in enumerate(("cold", "warm")):
            v = [r[j][i] for r in rows]
            lines.append(f"{what} {state}: median {statistics.median(v):.3f} s, range {min(v):.3f} .. {max(v):.3f} over {len(v)} processes")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="affine,1x16,2x64")
    ap.add_argument("--first-call", action="store_true")
    ap.add_argument("--create-only", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return first_call_child(a.create_only)
    import torch

    import bench
    from actor_rollout_bench import make_ac
    from policy_rollout_bench import SHAPES
    from pcgym_amd import VecEnv, _lib, collect_onpolicy, collect_rollouts

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    if a.first_call:
        lines = first_call(a)
    else:
        lib = _lib.load()
        lines = [f"# tools/user_closed_loop_bench.py  B={a.B} reps={a.reps}  library build {lib.pcg_build_id().decode()} "
                 f"({os.path.relpath(_lib.LIB_PATH, ROOT)})  {torch.cuda.get_device_name(0)}",
                 "# cstr, RK4 x 1, N = 60: one episode = 59 closed-loop steps; ms per episode, median of the interleaved repeats",
                 "# 1 = the hand-written cstr (custom_model) fused, 2 = the same plan per step, 3 = the built-in cstr fused"]
        pu, pb = user_params(), bench.workload_params()
        for name in a.shapes.split(","):
            for head in ("policy", "actor"):
                envs = {"1": VecEnv(copy.deepcopy(pu), n_envs=a.B, seed=1), "2": VecEnv(copy.deepcopy(pu), n_envs=a.B, seed=1),
                        "3": VecEnv(copy.deepcopy(pb), n_envs=a.B, seed=1)}
                spec = envs["1"].spec
                assert spec.model.model_id == 17 and envs["3"].spec.model.model_id == 0
                ac = make_ac(spec, SHAPES[name])
                pol = ac.actor
                steps = spec.N - 1
                if head == "policy":
                    routes = {"1": lambda: collect_rollouts(envs["1"], policy=pol),
                              "2": lambda: collect_rollouts(envs["2"], policy=lambda o: pol(o)),
                              "3": lambda: collect_rollouts(envs["3"], policy=pol)}
                else:
                    routes = {"1": lambda: collect_onpolicy(envs["1"], ac, fused=True),
                              "2": lambda: collect_onpolicy(envs["2"], ac, fused=False),
                              "3": lambda: collect_onpolicy(envs["3"], ac, fused=True)}
                times = {k: [] for k in routes}
                for rep in range(a.reps + 1):  # (round 0 warms every route up and builds the closed-loop module)
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
                lines.append(f"{name:7s} {head:6s} 1 user fused {med['1']:9.3f} ms ({1e3 * med['1'] / steps:8.2f} us/step)   "
                             f"2 user per-step {med['2']:9.3f} ms ({1e3 * med['2'] / steps:8.2f} us/step)   "
                             f"3 built-in fused {med['3']:9.3f} ms ({1e3 * med['3'] / steps:8.2f} us/step)   "
                             f"2 / 1 = {med['2'] / med['1']:.2f}   1 / 3 = {med['1'] / med['3']:.2f}   "
                             f"{a.B * steps / med['1'] / 1e-3:.3e} env-steps/s user fused")
                lines.append("        repeats (ms per episode) " + "  ".join(f"{k} {[round(t, 2) for t in times[k]]}" for k in times))
                for e in envs.values():
                    e.close()
                ac.close()
                del envs
                torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.first_call else "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
