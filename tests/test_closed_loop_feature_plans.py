"""CPU: the feature plans of helpers.FEATURE_PLANS mean something as closed-loop test cases -- shown on the oracle alone.

tests/test_gpu_closed_loop_features.py runs the fused closed-loop kernels on plans whose branches the other closed-loop tests
never take: the tracking reward with io->u_prev, the box excess, the crystallisation reward from the observed moments,
disturbance schedules with and without a Gaussian part, dense constraint rows, masked observations, the terminal reward, per-env
parameters next to disturbance slots.  A kernel comparison on such a plan is worth only as much as the branch is really taken:
a tracking term that is zero, a row that never violates, a disturbance slot that never moves would let a wrong kernel pass.
This file runs every case -- plan, integrator, head, network shape: the float64 cases of the GPU file -- closed loop on
OracleEnv for N - 1 steps (B = 578, seed 9, helpers._spread_x0) with the case's network evaluated in numpy and the actor's noise
from the oracle's Philox twin (tests/test_gpu_actor_rollout.py: z_twin), and asserts the conditions under which the GPU case can
fail (conditions()).  No GPU and no library call that touches one: the networks are host objects (MLPPolicy,
GaussianActorCritic; the latter reads its log-probability constant from the built library, pcg_actor_logp_const, host code --
like the other not-gpu tests this file needs build() to have run), and what it imports from tests/test_gpu_actor_rollout.py are
that module's host helpers (make_ac, host_conditioning, z_twin).

The plans' closed loops contract: under one network the envs of a batch reach the same state, bit for bit, within some twenty
steps.  The shares asserted here are therefore carried by the first steps, by the schedules, and (actors) by the per-env noise.

The constants that make a case meet its conditions are chosen here, from the oracle, by deterministic rules, on the plan under
RK4 (the CV8 case takes the RK4 case's choice and is held to the same conditions):
  rows      b_r of a row1 / rows8 plan, committed in ROW_BOUNDS and held here against the rule that gave them: the middle of the widest gap between neighbouring values of row r's linear part, over the
            case's own oracle episode, within 0.02 of its ROW_Q quantile (the median for one row; 0.9 for the eight dense rows,
            whose any-row flag would sit near 1 at the median).  A gap, because envs that have reached the same state share
            one row value: a plain quantile lands ON such a value and makes hundreds of rows exactly zero.
  networks  the first candidate of candidates() under which the case meets conditions(): policies helpers.make_policy with seeds
            17, 18, ... and then the same with the output bias shifted as make_ac shifts it (the output at the mean reset
            observation CENTRES half widths from the middle of the action box); actors
            test_gpu_actor_rollout.make_ac (seed 17) over its clip boxes BOXES and then MORE_BOXES, each also held to
            pick_ac's rule (the oracle's own 1e-15 sensitivity along the episode <= WELL_CONDITIONED, both clip branches at
            the first step).  A plan whose action boxes differ per component has no common clip box: its actor is
            the unbounded one (out_map none, sigma 0.02 half widths: test_gpu_actor_rollout.test_unbounded_actor) over seeds.
            The box plans (the constraint showcase) take feedback_policy instead: the cstr settles between the showcase's two
            rows under every constant coolant temperature but the coldest, so a make_policy network violates the upper row
            on a handful of entries at best; a network that heats the hot reactors and cools the cold ones keeps both rows,
            and both excess branches of the box term, on a real share (>= 1 % each is asserted).
"""
import os

import numpy as np
import pytest

from helpers import (BASE_FEATURE_PLANS, CONS_FEATURE_PLANS, FEATURE_PLANS, SHAPES, UNC_FEATURE_PLANS, EnvSpec, feature_params,
                     make_policy)
from test_gpu_actor_rollout import BOXES, WELL_CONDITIONED, _np_raw, action_box, host_conditioning, make_ac, z_twin

B, SEED, POLICY_SEED = 578, 9, 17
G_TOL = 1e-12  # tests/test_gpu_cons_rollout.py: the row tolerance, relative to |b| + sum |A_i| max(|v_i|, 1)
ROW_Q = {"row1": 0.5, "rows8": 0.9}
N_SEEDS = 4
# clip boxes tried after BOXES (centre in half widths from the middle of the action box, half width in sigmas): the showcase's
# rows are violated below 319 K, which the cstr reaches only with the coolant near the lower end of its box
CENTRES = (-0.6, -0.65, -0.7, -0.75, -0.8, -0.85, -0.9)
MORE_BOXES = [(c, w) for w in (0.2, 0.8) for c in CENTRES]
# the row bounds of the row1 / rows8 plans per head, as _row_bounds gives them on the RK4 plan (test_the_case_is_not_vacuous holds
# the rule against them, so that the plan a GPU case runs does not depend on the machine that chose it)
ROW_BOUNDS = {
    ("cryst_paper_reward_row", "policy"): [10687.861502115093],
    ("cryst_paper_reward_row", "actor"): [14155.621171629471],
    ("cstr_dist_both_rows8", "policy"): [-759.7391024230874, 1010.8308267048781, -804.0577176004631, 581.9872327726061, 322.64769223765904,
                                         -854.904684770534, -986.9466650338118, 958.5472213569217],
    ("cstr_dist_both_rows8", "actor"): [-759.5038671983589, 1011.0724451602666, -804.0916576311461, 581.9897597791926, 322.4532463283917,
                                        -854.9070709092794, -986.5623748099681, 958.6920705180954],
}
THREADS = max(1, min(8, os.cpu_count() or 1))


def cases():
    """(plan, integrator, head, network shape) of every GPU case that runs the float64 kernels"""
    out = [(n, i, h, "1x16") for n in BASE_FEATURE_PLANS for i in ("rk4", "cv8") for h in ("policy", "actor")]
    out += [(n, i, h, "1x16") for n in CONS_FEATURE_PLANS for i in ("rk4", "cv8") for h in ("policy", "actor")]
    out += [(n, "rk4", h, s) for n in UNC_FEATURE_PLANS for h in ("policy", "actor") for s in ("1x16", "affine")]
    return out


def row_scales(spec, x, sp_d, u_abs):
    """|b_r| + sum |A_r,i| max(|v_i|, 1) of every row: test_gpu_cons_rollout._row_scale, row by row"""
    A, b = np.abs(spec.con_A).sum(axis=1), np.abs(np.asarray(spec.con_b, dtype=float))
    top = max(1.0, float(np.max(np.abs(x))), float(np.max(np.abs(sp_d))) if np.size(sp_d) else 0.0, float(u_abs))
    return b + A * top


def u_box(spec, a):
    return max(float(np.max(np.abs(spec.a_low))), float(np.max(np.abs(spec.a_high))), float(np.max(np.abs(a))))


def _rows_A(spec, kind):
    """the coefficients of a row1 / rows8 plan over [x | SP | d | u | model disturbance inputs], each divided by the width of
    its slot's box"""
    nst = spec.nobs - spec.nunc
    width = np.maximum(np.asarray(spec.o_high, dtype=float) - np.asarray(spec.o_low, dtype=float), 1e-6)[:nst]
    a_w = np.maximum(np.asarray(spec.a_high, dtype=float) - np.asarray(spec.a_low, dtype=float), 1e-6)
    if kind == "row1":
        A = np.zeros((1, nst + spec.nu))
        A[0, 0], A[0, nst] = 1.0 / width[0], 0.3 / a_w[0]
        return A
    assert spec.nsp_obs >= 1 and spec.nd >= 2 and spec.ndm == spec.nd
    rng = np.random.default_rng(8)
    ncon = 8
    A = rng.uniform(0.3, 1.0, (ncon, nst + spec.nu)) * rng.choice([-1.0, 1.0], (ncon, nst + spec.nu))
    for r in range(ncon):  # one state per row (alternating), the SP slot, every disturbance slot, the action, every disturbance input
        A[r, (r + 1) % spec.nx] = 0.0
    A[:, :nst] /= width[None, :]
    A[:, nst:nst + spec.na] /= a_w[None, :]
    A[:, nst + spec.na:] /= width[None, spec.nx + spec.nsp_obs:]
    return A


def _row_bounds(g, q):
    """per row the middle of the widest gap between neighbouring distinct values of g (T, ncon, B) among those from its
    (q - 0.02)- to its (q + 0.02)-quantile"""
    b = np.empty(g.shape[1])
    for r in range(g.shape[1]):
        v = np.unique(g[:, r])
        lo, hi = np.quantile(g[:, r], [q - 0.02, q + 0.02])
        w = v[(v >= lo) & (v <= hi)]
        if w.size < 2:
            i = int(np.clip(np.searchsorted(v, lo), 1, v.size - 1))
            w = v[i - 1:i + 1]
        i = int(np.argmax(np.diff(w)))
        b[r] = 0.5 * (w[i] + w[i + 1])
    return b


def host_action(net, head, obs, z):
    """(applied action, sample) of the case's network on `obs` (n_in, B), in numpy"""
    pol = net if head == "policy" else net.actor
    u = _np_raw(pol, obs)
    if head == "actor":
        u = u + net.sigma[:, None] * z
    return (np.clip(u, pol.out_low, pol.out_high) if pol.out_map == "clip" else u), u


def host_episode(spec, net, head, T):
    """the closed loop on the oracle: dict of per-step records (x before the step, the observation the network read, ...)"""
    from oracle import oracle as O

    orc = O.OracleEnv(spec, B, seed=SEED, n_threads=THREADS)
    orc.reset()
    z = z_twin(orc._seed(), 0, B, spec.na, range(T)) if head == "actor" else np.zeros((T, spec.na, B))
    rec = {k: [] for k in ("x", "obs_in", "a", "u", "obs", "rew", "done", "u_prev", "g", "viol", "slots")}
    rec["u_prev0"] = None if orc.u_prev is None else orc.u_prev.copy()
    rec["p_unc"] = None if orc.p_unc is None else orc.p_unc.copy()
    obs = orc.obs.copy()
    for s in range(T):
        a, u = host_action(net, head, obs, z[s])
        rec["x"].append(orc.x.copy()), rec["obs_in"].append(obs), rec["a"].append(a), rec["u"].append(u)
        o, r, d = orc.step(a)
        obs = o.copy()
        rec["obs"].append(obs), rec["rew"].append(r.copy()), rec["done"].append(d.copy()), rec["slots"].append(orc.slots.copy())
        if orc.u_prev is not None:
            rec["u_prev"].append(orc.u_prev.copy())
        if orc.g is not None:
            rec["g"].append(orc.g.copy()), rec["viol"].append(orc.viol.copy())
    rec["x_end"] = orc.x.copy()
    return {k: (np.stack(v) if isinstance(v, list) and v else v) for k, v in rec.items()}


def box_branches(spec, obs, viol):
    """(upper, lower): where the box term of the tracking reward adds its upper / its lower excess, per (step, env) entry of
    the recorded observations (T, Nobs, B) and flags (T, B) -- the kernels' statement: normalised observed state against the
    normalised bounds, `>` the upper one first, else `<` the lower one, while a row is violated"""
    q = int(spec.rew_box_index[0])
    lo, w = float(spec.o_low[q]), float(spec.o_high[q] - spec.o_low[q])
    lon, hin = (float(spec.rew_box_lo[0]) - lo) / w, (float(spec.rew_box_hi[0]) - lo) / w
    on = obs[:, q] if not spec.normalise_o else obs[:, q] * w / 2 + (spec.o_high[q] + spec.o_low[q]) / 2
    xn = (on - lo) / w
    viol = np.asarray(viol).astype(bool)
    return viol & (xn > hin), viol & ~(xn > hin) & (xn < lon)


def conditions(name, spec, net, head, ep):
    """(figures, unmet conditions) of one case on its oracle episode: what makes the GPU case able to fail"""
    kinds = FEATURE_PLANS[name][2]
    T = spec.N - 1
    nx, nso, nd, nunc = spec.nx, spec.nsp_obs, spec.nd, spec.nunc
    figures, unmet = [], []

    def need(ok, what):
        if not ok:
            unmet.append(what)

    # ---- every plan: finite states; the policy's outputs inside the clip box, both branches of the actor's clip ----
    finite = all(np.isfinite(ep[k]).all() for k in ("x", "x_end", "rew", "obs", "a"))
    need(finite, "a state, reward or observation is not finite")
    if not finite:
        return figures, unmet
    pol = net if head == "policy" else net.actor
    inside = float(np.mean((ep["a"] > pol.out_low) & (ep["a"] < pol.out_high)))
    figures.append(f"{inside:.2f} of the actions inside the clip box")
    if head == "policy":
        need(inside >= 0.25, f"only {inside:.2f} of the policy outputs lie strictly inside the clip box")
    elif pol.out_map == "clip":
        need(0.0 < float(np.mean(ep["a"] != ep["u"])) < 1.0, "one branch of the actor's clip never occurs")
    need(np.std(ep["a"]) > 0, "the actions do not vary")
    # ---- tracking plans ----
    if "track" in kinds:
        need(spec.reward_track is not None and spec.reward_track["R"] > 0, "no tracking reward")
        need(np.isnan(ep["u_prev0"]).all(), "step 0 does not take the 'no previous action' branch")
        up, lo = ep["u_prev"], np.asarray(spec.a_low, dtype=float)[None, :, None]
        inv = 1.0 / (np.asarray(spec.a_high, dtype=float) - np.asarray(spec.a_low, dtype=float))[None, :, None]
        un = (up - lo) * inv
        term = spec.reward_track["R"] * np.sum((un[1:] - un[:-1]) ** 2, axis=1)
        share = float(np.mean(term != 0.0))
        figures.append(f"R_du term non-zero on {share:.2f} of the entries from step 1 on")
        need(np.isfinite(up).all() and share >= 0.5, f"the R_du term is non-zero on {share:.2f} of the (env, step) entries only")
        if "R_u" in kinds:
            need(spec.reward_track["R_u"] > 0 and float(np.mean(np.sum(un * un, axis=1) != 0.0)) >= 0.5, "the R_u term is vacuous")
    if "cryst" in kinds:
        need(spec.reward_track["cryst"] and np.std(ep["rew"]) > 0, "no reward from the observed moments")
    # ---- box plans: the term fires while a row is violated and the boxed state is outside its box ----
    if "box" in kinds:
        upper, lower = box_branches(spec, ep["obs"], ep["viol"])
        n, share = upper.size, float(np.mean(upper | lower))
        figures.append(f"box excess on {share:.3f} of the entries ({int(upper.sum())} of {n} upper branch, {int(lower.sum())} lower)")
        need(0.05 <= share <= 0.95, f"the box term fires on {share:.3f} of the entries")
        need(upper.sum() >= 0.01 * n and lower.sum() >= 0.01 * n, "an excess branch of the box term occurs on less than 1 % of the entries")
        per_row = np.mean(ep["g"] > 0, axis=(0, 2))
        need(per_row.min() >= 0.01, f"a row of the showcase is violated on {per_row.min():.4f} of the entries only")
    # ---- constraint rows ----
    if "cons" in kinds:
        g, viol = ep["g"], ep["viol"].astype(bool)
        need(g.shape == (T, spec.ncon, B) and np.array_equal(viol, (g > 0).any(axis=1)), "the flag is not 'any row > 0'")
        any_share = float(np.mean(viol))
        per_row = np.mean(g > 0, axis=(0, 2))
        figures.append(f"rows violated on {per_row.min():.3f} .. {per_row.max():.3f} of the entries, any row {any_share:.3f}")
        need(0.05 <= any_share <= 0.95, f"{any_share:.3f} of the entries violate")
        if "row1" in kinds or "rows8" in kinds:
            need(per_row.min() >= 0.02, f"a row is violated on {per_row.min():.3f} of the entries only")
        if "rows8" in kinds:
            nst = spec.nobs - nunc
            cols = np.abs(spec.con_A) > 0
            need(spec.ncon == 8 and cols[:, :nx].any(axis=1).all() and cols[:, nx:nst].all() and cols[:, nst + nunc:].all(),
                 "a dense row misses a column")
        near = 0
        for s in range(T):
            tol = G_TOL * row_scales(spec, ep["x"][s], ep["slots"][s], u_box(spec, ep["a"][s]))
            near += int(np.sum(np.abs(g[s]) <= tol[:, None]))
        figures.append(f"{near} of {g.size} row entries within the row tolerance of zero")
        need(near <= 0.01 * g.size, f"{near} of {g.size} row entries lie within the row tolerance of zero")
    # ---- disturbance plans ----
    if "dist" in kinds:
        od = ep["obs"][:, nx + nso:nx + nso + nd]
        need(nd >= 1 and np.any(od[1:] != od[:-1], axis=(0, 2)).all(), "a disturbance slot keeps its value through the episode")
        if "gauss" in kinds:
            need(spec.gauss and float(np.std(od, axis=2).min()) > 0, "a step's Gaussian disturbance does not vary over the batch")
        else:
            need(np.all(od == od[:, :, :1]), "the schedule is not shared by the batch")
        if nso:
            osp = ep["obs"][:, nx:nx + nso]
            need(np.any(osp[1:] != osp[:-1], axis=(0, 2)).all(), "the set-point slot keeps its value through the episode")
    # ---- per-env parameters ----
    if "unc" in kinds:
        slots = ep["obs"][:, nx + nso + nd:]
        need(nunc >= 2 and spec.x0_unc is not None and slots.shape[1] == nunc, "fewer than two parameter slots")
        need(float(np.std(slots[0], axis=1).min()) > 0 and np.all(slots == slots[:1]) and float(np.std(ep["p_unc"], axis=1).min()) > 0,
             "the parameter slots do not vary over the batch, or change along the episode")
        if "dist" in kinds:
            need(nd >= 1, "no disturbance slot in front of the parameter slots")
        if "q11" in kinds:
            free = [j for j in range(spec.ndm) if j not in set(int(v) for v in spec.d_slot)]
            need(free and any(int(spec.d_param_index[j]) in set(int(v) for v in spec.unc_index) for j in free),
                 "no uncertain parameter is read by an unconfigured disturbance input")
    # ---- partial observation ----
    if "mask" in kinds:
        masked = [i for i in range(nx) if not spec.obs_mask[i]]
        need(bool(masked), "no masked slot")
        for i in masked:
            need(np.all(ep["obs"][:, i] == 0.0) and np.all(ep["obs_in"][0][i] == 0.0), f"masked slot {i} is not exactly zero")
            need(np.any(pol.weights[0][:, i] != 0.0), f"no first-layer weight on masked slot {i}")
        need(all(np.std(ep["obs"][:, i]) > 0 for i in range(nx) if spec.obs_mask[i]), "an observed slot does not vary")
    # ---- the terminal reward ----
    if "batch" in kinds:
        last = ep["rew"][-1]
        need(spec.reward_batch and np.all(ep["rew"][:-1] == 0.0), "a reward before the last step")
        need(np.all(last != 0.0) and np.std(last) > 0, "the terminal reward is zero or does not vary")
    if "noise" in kinds:
        need(spec.noise and float(spec.noise_pct.max()) > 0, "no observation noise")
    return figures, unmet


def feedback_policy(spec, obs0, shape, seed):
    """make_policy's network turned into a switch on the boxed state of the tracking reward: hidden unit 0 is
    tanh(x_q - the middle of the rows' bounds on x_q) (one unit of the state per unit of pre-activation), the output is the
    middle of the action box + 0.9 half widths of that unit + a tenth of the network's other units -- strictly inside the
    action box, hot reactors heated, cold ones cooled"""
    from pcgym_amd import MLPPolicy

    assert SHAPES[shape] and not spec.normalise_o and not spec.normalise_a
    q = int(spec.rew_box_index[0])
    rows = [r for r in range(spec.ncon) if spec.con_A[r, q] != 0.0]
    thr = float(np.mean([spec.con_b[r] / spec.con_A[r, q] for r in rows]))
    pol = make_policy(spec, obs0, SHAPES[shape], seed=seed)
    Ws, bs = [w.copy() for w in pol.weights], [b.copy() for b in pol.biases]
    lo, hi = np.asarray(spec.a_low, dtype=float), np.asarray(spec.a_high, dtype=float)
    Ws[0][0, :] = 0.0
    Ws[0][0, q], bs[0][0] = 1.0, -thr
    Ws[-1][:, 1:] *= 0.1
    Ws[-1][:, 0], bs[-1] = 0.9 * (hi - lo) / 2, (hi + lo) / 2
    return MLPPolicy(Ws, bs, activation=pol.activation, out_map="clip", out_low=pol.out_low, out_high=pol.out_high)


def candidates(spec, head, name):
    """the networks tried for a case, in order: (seed, out_map or kind, clip-box centre, clip-box half width in sigmas)"""
    if "box" in FEATURE_PLANS[name][2]:
        return [(POLICY_SEED + k, "feedback", None, None) for k in range(N_SEEDS)]
    if head == "policy":
        return ([(POLICY_SEED + k, "clip", None, None) for k in range(N_SEEDS)]
                + [(POLICY_SEED + k, "clip", c, None) for c in CENTRES for k in range(2)])
    lo, hi = action_box(spec)
    if np.all(lo == lo[0]) and np.all(hi == hi[0]):
        return [(POLICY_SEED, "clip", c, w) for c, w in BOXES + MORE_BOXES]
    return [(POLICY_SEED + k, "none", None, None) for k in range(N_SEEDS)]


def build_net(spec, obs0, head, shape, cand):
    seed, out_map, centre, width = cand
    if out_map == "feedback":
        pol = feedback_policy(spec, obs0, shape, seed)
        if head == "policy":
            return pol
        from pcgym_amd import GaussianActorCritic, MLPPolicy

        # (make_ac's sigma and critic; the clip box is the whole action box, which the samples around a mean 0.9 half widths
        # from its middle leave often enough)
        c = make_policy(spec, obs0, SHAPES[shape], seed + 100)
        cr = MLPPolicy(c.weights[:-1] + [c.weights[-1][:1]], c.biases[:-1] + [c.biases[-1][:1]], activation=c.activation, out_map="none")
        lo, hi = action_box(spec)
        return GaussianActorCritic(pol, np.log(0.25 * (hi - lo) / 2), cr)
    if head == "policy":
        pol = make_policy(spec, obs0, SHAPES[shape], seed=seed)
        if centre is None:
            return pol
        # make_ac's shift: the output at the mean reset observation sits `centre` half widths from the middle of the action box
        from pcgym_amd import MLPPolicy

        lo, hi = action_box(spec)
        mu_c = _np_raw(pol, np.mean(obs0, axis=1, keepdims=True))[:, 0]
        bs = [b.copy() for b in pol.biases]
        bs[-1] = bs[-1] + ((lo + hi) / 2 + centre * (hi - lo) / 2 - mu_c)
        return MLPPolicy(pol.weights, bs, activation=pol.activation, out_map=pol.out_map, out_low=pol.out_low, out_high=pol.out_high)
    if out_map == "none":
        return make_ac(spec, obs0, SHAPES[shape], seed=seed, out_map="none", sigma_scale=0.02)
    return make_ac(spec, obs0, SHAPES[shape], seed=seed, centre=centre, box=width)


_CASES = {}


def _with_rows(name, integ, spec0, row_kind, b=None):
    A = _rows_A(spec0, row_kind)
    return EnvSpec(feature_params(name, integ, rows=(A, np.zeros(A.shape[0]) if b is None else b)))


def _episode(name, integ, head, shape, cand):
    """(spec, env_params, net, oracle episode) of the case under candidate `cand`, the row bounds chosen from a pilot episode"""
    from oracle import oracle as O

    kinds = FEATURE_PLANS[name][2]
    row_kind = next((k for k in ROW_Q if k in kinds), None)
    spec0 = EnvSpec(feature_params(name, integ))
    spec = _with_rows(name, integ, spec0, row_kind) if row_kind else spec0
    T = spec.N - 1
    orc = O.OracleEnv(spec, B, seed=SEED)
    orc.reset()
    obs0 = orc.obs.copy()
    net = build_net(spec, obs0, head, shape, cand)
    ep = host_episode(spec, net, head, T)
    if row_kind:
        spec = _with_rows(name, integ, spec0, row_kind, np.array(ROW_BOUNDS[name, head]))
        ep = host_episode(spec, net, head, T)
    return spec, net, ep


def rule_row_bounds(name, head, shape, cand):
    """what the rule gives for ROW_BOUNDS[name, head]: _row_bounds on the RK4 plan's pilot episode, recorded with b = 0 (its
    rows are the linear parts)"""
    from oracle import oracle as O

    row_kind = next(k for k in ROW_Q if k in FEATURE_PLANS[name][2])
    spec = _with_rows(name, "rk4", EnvSpec(feature_params(name, "rk4")), row_kind)
    orc = O.OracleEnv(spec, B, seed=SEED)
    orc.reset()
    net = build_net(spec, orc.obs.copy(), head, shape, cand)
    return _row_bounds(host_episode(spec, net, head, spec.N - 1)["g"], ROW_Q[row_kind])


def row_head(spec, name):
    """the head whose committed row bounds `spec` carries"""
    return next(h for h in ("policy", "actor") if np.array_equal(np.asarray(spec.con_b, dtype=float), np.array(ROW_BOUNDS[name, h])))


def case_params(name, integ, spec):
    """the env_params a VecEnv of the case is made from: those `spec` (feature_case) was made from"""
    row_kind = next((k for k in ROW_Q if k in FEATURE_PLANS[name][2]), None)
    if not row_kind:
        return feature_params(name, integ)
    assert np.array_equal(np.asarray(spec.con_b, dtype=float), np.array(ROW_BOUNDS[name, row_head(spec, name)])), "not the committed row bounds"
    return feature_params(name, integ, rows=(_rows_A(EnvSpec(feature_params(name, integ)), row_kind), np.asarray(spec.con_b, dtype=float)))


def feature_case(name, integ, head, shape="1x16"):
    """(EnvSpec, network, the oracle's episode, the candidate taken) of one case; the networks are host objects until a GPU test
    asks for their device handles.  Cached: the GPU file takes the very objects this file's conditions are asserted on."""
    key = (name, integ, head, shape)
    if key in _CASES:
        return _CASES[key]
    if integ != "rk4":  # (the choice is made on the RK4 plan)
        cand = feature_case(name, "rk4", head, shape)[3]
        _CASES[key] = _episode(name, integ, head, shape, cand) + (cand,)
        return _CASES[key]
    tried = []
    for cand in candidates(EnvSpec(feature_params(name, integ)), head, name):
        spec, net, ep = _episode(name, integ, head, shape, cand)
        unmet = conditions(name, spec, net, head, ep)[1]
        if not unmet and head == "actor":
            amp, clipped0 = host_conditioning(spec, net, B, spec.N - 1, SEED, n_threads=THREADS)
            if amp > WELL_CONDITIONED or (net.actor.out_map == "clip" and not 0.0 < clipped0 < 1.0):
                unmet = [f"the oracle's own 1e-15 sensitivity is {amp:.1e}, {clipped0:.3f} of the first samples clipped"]
        if not unmet:
            _CASES[key] = (spec, net, ep, cand)
            return _CASES[key]
        tried.append((cand, unmet))
        net.close()
    raise AssertionError(f"{key}: no candidate network meets the case's conditions: {tried[:3]} ... {tried[-1:]}")


def _ids(c):
    return "-".join(c)


@pytest.mark.parametrize("case", cases(), ids=_ids)
def test_the_case_is_not_vacuous(case):
    name, integ, head, shape = case
    spec, net, ep, cand = feature_case(*case)
    T = spec.N - 1
    assert spec.integrator == integ and T <= 59 and ep["x"].shape == (T, spec.nx, B)
    figures, unmet = conditions(name, spec, net, head, ep)
    print(f"case {_ids(case)}: network {cand}; " + "; ".join(figures))
    assert not unmet, unmet
    if (name, head) in ROW_BOUNDS and integ == "rk4":
        b = rule_row_bounds(name, head, shape, cand)
        assert np.allclose(b, ROW_BOUNDS[name, head], rtol=1e-9, atol=0), f"the rule gives other row bounds than the committed ones: {list(b)}"
    if head == "actor":
        amp, clipped0 = host_conditioning(spec, net, B, T, SEED, n_threads=THREADS)
        assert amp <= WELL_CONDITIONED, f"the oracle's own 1e-15 sensitivity along the episode is {amp:.1e}"
