#!/usr/bin/env python3
"""The GAE tail of collect_onpolicy: the kernel (pcg_gae, one launch) against the loop of element-wise torch calls it
replaces (rollout.gae fused=False, which stays in the tree), on its own and inside the fused collector.

    python tools/gae_bench.py [--Bs 4096,65536,1048576] [--B 1048576] [--reps 9] [--shapes affine,1x16,2x64] [--out FILE]

Everything alternates inside one process; times are device-event times (a synchronise on both sides), the figure compared is
the median of `reps` interleaved repeats after one warm-up round.

  (i)  gae() alone on cstr-shaped arrays, T = 59 (N = 60), rew (T, B), val (T + 1, B), for every B of --Bs:
         loop    gae(fused=False)                    kernel    gae(fused=True)
         loop_t / kernel_t   the same with a termination mask (10 % of the entries set)
       The kernel's rate is counted against the bytes the estimator needs, 32 B per env step (rew and val in, adv and ret
       out; 33 with the mask), as a share of the HBM peak (8.0 TB/s by specification; 6.29 TB/s is what a float4 copy reaches).
       Results are compared bit for bit before anything is timed.
  (ii) collect_onpolicy(env, ac) on the headline's cstr envs (bench.workload_params: RK4, N = 60), B = --B, fused, for the three
       network shapes in float64 and float32, with the tail on either route (`L`: rollout.gae bound to fused=False for the
       call, what the collector did before the kernel; `K`: as shipped), and the two tails alone on the arrays the collector
       returned.  share = loop alone / L: the part of the fused collector's time that was the torch loop.

Condition: the kernel is not slower than the loop at any shape of (i), and K is not slower than L at any shape of (ii).
"""
import argparse
import functools
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")]

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12  # B/s: specification; measured float4 copy


def timed(torch, routes, reps):
    """{name: [ms]} of the routes called in turn, `reps` rounds after one warm-up round"""
    times = {k: [] for k in routes}
    for rep in range(reps + 1):
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
    return times


def same_bits(torch, a, b):
    return all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(a, b))


def alone_rows(a, torch, gae):
    T = 59
    lines = ["# (i) gae() alone, T = 59: ms per call (median), kernel's bytes = 32 (33 with the mask) x B x T"]
    ok = True
    for B in [int(s) for s in a.Bs.split(",")]:
        g = torch.Generator(device="cuda").manual_seed(B)
        rew = torch.randn((T, B), dtype=torch.float64, device="cuda", generator=g)
        val = torch.randn((T + 1, B), dtype=torch.float64, device="cuda", generator=g)
        term = torch.rand((T, B), device="cuda", generator=g) < 0.1
        assert same_bits(torch, gae(rew, val, fused=True), gae(rew, val, fused=False))
        assert same_bits(torch, gae(rew, val, term=term, fused=True), gae(rew, val, term=term, fused=False))
        routes = {"loop": lambda: gae(rew, val, fused=False), "kernel": lambda: gae(rew, val, fused=True),
                  "loop_t": lambda: gae(rew, val, term=term, fused=False), "kernel_t": lambda: gae(rew, val, term=term, fused=True)}
        times = timed(torch, routes, a.reps)
        med = {k: statistics.median(v) for k, v in times.items()}
        rate, rate_t = 32.0 * B * T / (med["kernel"] * 1e-3), 33.0 * B * T / (med["kernel_t"] * 1e-3)
        good = med["kernel"] <= med["loop"] and med["kernel_t"] <= med["loop_t"]
        ok = ok and good
        lines.append(f"B={B:8d}  loop {med['loop']:8.3f}  kernel {med['kernel']:8.4f}  loop / kernel = {med['loop'] / med['kernel']:7.1f}   "
                     f"loop_t {med['loop_t']:8.3f}  kernel_t {med['kernel_t']:8.4f}  loop_t / kernel_t = {med['loop_t'] / med['kernel_t']:7.1f}   "
                     f"kernel {rate / 1e12:.3f} TB/s = {rate / HBM_SPEC:.3f} of 8.0 TB/s ({rate / HBM_COPY:.3f} of the 6.29 TB/s copy); "
                     f"with mask {rate_t / 1e12:.3f} TB/s = {rate_t / HBM_SPEC:.3f} ({rate_t / HBM_COPY:.3f})   "
                     + ("kernel not slower than the loop" if good else "KERNEL SLOWER THAN THE LOOP"))
        lines.append("        repeats (ms) " + "  ".join(f"{k} {[round(t, 4) for t in times[k]]}" for k in times))
        del rew, val, term
        torch.cuda.empty_cache()
    return lines, ok


def collector_rows(a, torch, gae):
    import bench
    from actor_rollout_bench import make_ac
    from pcgym_amd import VecEnv, collect_onpolicy
    from pcgym_amd import rollout as R
    from policy_rollout_bench import SHAPES

    p = bench.workload_params()
    lines = [f"# (ii) collect_onpolicy fused, cstr RK4 N = 60, B = {a.B}: ms per episode (median); L = tail by the torch loop, K = tail "
             "by the kernel; loop / kernel = the tails alone on the collected arrays; share = loop / L"]
    ok = True

    def with_loop(env, ac):
        R.gae = functools.partial(gae, fused=False)  # the collector as it was: its tail is the torch loop
        try:
            return collect_onpolicy(env, ac)
        finally:
            R.gae = gae

    for dtype in ("float64", "float32"):
        for name in a.shapes.split(","):
            envs = {k: VecEnv(dict(p), n_envs=a.B, seed=1) for k in ("L", "K")}
            spec = envs["L"].spec
            ac = make_ac(spec, SHAPES[name], dtype=dtype)
            steps = spec.N - 1
            d = collect_onpolicy(envs["K"], ac)
            rew, val = d["rew"], d["val"]
            assert same_bits(torch, (d["adv"], d["ret"]), gae(rew, val, fused=False))
            del d
            routes = {"L": lambda: with_loop(envs["L"], ac), "K": lambda: collect_onpolicy(envs["K"], ac),
                      "loop": lambda: gae(rew, val, fused=False), "kernel": lambda: gae(rew, val, fused=True)}
            times = timed(torch, routes, a.reps)
            med = {k: statistics.median(v) for k, v in times.items()}
            good = med["K"] <= med["L"]
            ok = ok and good
            lines.append(f"{dtype} {name:7s} L {med['L']:7.3f}  K {med['K']:7.3f}  L / K = {med['L'] / med['K']:.3f}   loop {med['loop']:7.3f}  "
                         f"kernel {med['kernel']:7.4f}   share of the loop in L = {med['loop'] / med['L']:.3f}   per step: L {1e3 * med['L'] / steps:.2f}  "
                         f"K {1e3 * med['K'] / steps:.2f}  loop {1e3 * med['loop'] / steps:.2f}  kernel {1e3 * med['kernel'] / steps:.3f} us   "
                         f"{a.B * steps / med['K'] / 1e-3:.3e} env-steps/s with the kernel   "
                         + ("K not slower than L" if good else "K SLOWER THAN L"))
            lines.append("        repeats (ms) " + "  ".join(f"{k} {[round(t, 3) for t in times[k]]}" for k in times))
            for e in envs.values():
                e.close()
            ac.close()
            del envs, rew, val
            torch.cuda.empty_cache()
    return lines, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Bs", default="4096,65536,1048576")
    ap.add_argument("--B", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="affine,1x16,2x64")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    from pcgym_amd import _lib, gae

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lib = _lib.load()
    lines = [f"# tools/gae_bench.py  Bs={a.Bs} B={a.B} reps={a.reps}  library build {lib.pcg_build_id().decode()} "
             f"({os.path.relpath(_lib.LIB_PATH, ROOT)})  {torch.cuda.get_device_name(0)}"]
    l1, ok1 = alone_rows(a, torch, gae)
    l2, ok2 = collector_rows(a, torch, gae)
    lines += l1 + l2 + ["# condition (kernel <= loop at every shape of (i), K <= L at every shape of (ii)): " + ("met" if ok1 and ok2 else "NOT MET")]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok1 and ok2 else 1


if __name__ == "__main__":
    sys.exit(main())
