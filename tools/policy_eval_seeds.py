"""Prints the SEEDS table of tests/test_gpu_policy_eval.py: for every plan, activation and hidden shape the first seed of
17, 18, ... under which make_policy's weights meet the test's non-vacuity conditions (_vacuity) with all three output maps.
Host only: EnvSpec, MLPPolicy and the long-double reference, no GPU and no library call.

    python tools/policy_eval_seeds.py            # the table, and what seed 17 would have failed on
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import test_gpu_policy_eval as T  # noqa: E402
from helpers import host_reference  # noqa: E402


def reasons(plan, shape, act, seed):
    out = []
    _, obs = T._inputs(plan)
    for om in T.OUT_MAPS:
        pol = T._network(plan, shape, act, om, seed=seed)
        ref, _, pre = host_reference(pol, obs, 2.0)
        why = T._vacuity(pol, obs, ref)
        if act == "tanh" and pre > T.PRE_MAX:
            why.append(f"pre-activations up to {pre:.1f}")
        out += [f"{om}: {w}" for w in why]
    return out


def main():
    print("SEEDS = {")
    notes = []
    for plan in T.PLANS:
        row = {}
        for act in T.ACTS:
            row[act] = []
            for shape in T.HIDDEN:
                for seed in range(17, 17 + 200):
                    why = reasons(plan, shape, act, seed)
                    if not why:
                        break
                    if seed == 17:
                        notes.append(f"# {plan} {shape} {act}, seed 17: {'; '.join(why)}")
                else:
                    raise SystemExit(f"no seed for {plan} {shape} {act}")
                row[act].append(seed)
        print(f'    "{plan}": {{"tanh": {row["tanh"]},\n' + " " * (8 + len(plan)) + f'"relu": {row["relu"]}}},')
    print("}")
    print("\n".join(notes))


if __name__ == "__main__":
    main()
