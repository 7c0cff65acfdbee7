"""Batched rollout collector + reproducibility metrics.

Counterpart of the reference's ``policy_eval.rollout / get_rollouts``
(src/pcgym/policy_evaluation.py:71-197) and ``reproducibility_metric``
(src/pcgym/evaluation_metrics.py:182-327), for B environments at once and with
every array on the GPU in the reference's axis order:

    r (1, N, B)   r[0, 0] = r_init = 0, r[0, i+1] = reward of step i          (:86, :113-116)
    x (Nx, N, B)  x[:, 0] = reset observation, x[:, i+1] = observation after step i,
                  both de-normalised with observation_space_base                (:88-106)
    u (na, N, B)  physical (de-normalised) actions, column N-1 = the action the policy
                  proposes for the final observation                            (:101-104, 123-127)
    g (n_con, N, 1, B)  constraint rows (cons_info)                             (:118-121, 180-183)

``reps`` of the reference (independent repetitions of one env) is the env axis B here.
Closed loop: ``policy(obs (B, Nobs) tensor) -> (B, na)`` (or ``(na, B)``) tensor, one
kernel launch per step -- or, for a declarative :class:`~pcgym_amd.policy.MLPPolicy` on a plan that qualifies, ONE launch
for the whole episode with the policy evaluated in the kernel (``pcg_rollout_policy``; ``pcg_rollout_policy_cons`` on a plan
with constraint rows, which records the rows of every step).  Open loop (``actions`` given, no constraint rows to record): the fused
``pcg_rollout_strided`` kernel writes straight into these layouts, state in registers.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from . import _lib
from .policy import (fused_actor_cons_ok, fused_actor_ok, fused_actor_unc_ok, fused_cons_ok, fused_policy_ok, fused_pop_cons_ok,
                     fused_pop_ok, fused_pop_unc_ok, fused_unc_ok)


def _torch():
    import torch

    return torch


def _affine(env, low, high, active):
    """de-normalisation (v + 1) * (high - low) / 2 + low as v * half + mid: (half, mid) column tensors, or None"""
    if not active:
        return None
    torch = _torch()
    lo = torch.as_tensor(np.asarray(low, dtype=np.float64), device=env.device)
    hi = torch.as_tensor(np.asarray(high, dtype=np.float64), device=env.device)
    return (hi - lo) / 2, (hi + lo) / 2


def _denorm_(t, hm, dim):
    """in place, one pass over the data: t[..] = t[..] * half + mid with (half, mid) broadcast along `dim`"""
    if hm is None:
        return t
    torch = _torch()
    shp = [1] * t.dim()
    shp[dim] = -1
    half, mid = hm[0].reshape(shp), hm[1].reshape(shp)
    return torch.addcmul(mid, t, half, out=t)


@contextlib.contextmanager
def _recording(env):
    """a per-step loop that binds each step's observation / reward rows to trajectory storage (``env.bind_outputs``): on the
    way out, however the loop ends, the env gets its own storage back, holding its latest outputs"""
    saved = (env.obs_soa, env.rew)
    try:
        yield
    finally:
        last_o, last_r = env.obs_soa, env.rew
        env.bind_outputs(*saved)
        env.obs_soa.copy_(last_o)  # the env keeps its own storage; its latest outputs stay readable there
        env.rew.copy_(last_r)


def collect_rollouts(env, policy=None, actions=None, fused_unc=False):
    """Roll all B envs of a VecEnv through one episode (N-1 steps) and return the reference-shaped dict.

    policy  : callable obs(B,Nobs) -> action (B,na)|(na,B) tensor (closed loop); an ``MLPPolicy`` is evaluated inside
              the fused rollout kernel when the plan qualifies (``fused_policy_ok``: RK4 / CV8, no constraint rows, no
              per-env parameters; user models and reward expressions included -- or ``fused_cons_ok``: a built-in plan
              WITH affine constraint rows, whose rows the kernel of ``pcg_rollout_policy_cons`` records into ``g``) and
              like any other callable otherwise, or
    actions : (N, na, B) tensor of policy outputs (open loop; row N-1 is only recorded in ``u``).
    fused_unc : True takes ``pcg_rollout_policy_unc`` -- the whole episode in one launch -- on a built-in RK4 plan with per-env
              parameters, and raises ValueError unless ``fused_unc_ok(spec, policy)``.  It has to be asked for: by default such a
              plan keeps the per-step loop, whose results the fused kernel matches to rounding and not to the bit (the two
              kernels are compiled separately).

    Recording is zero-copy: each step's kernel writes its observation / reward rows straight into the trajectory
    storage (``VecEnv.bind_outputs``), and the de-normalisation to physical units (policy_evaluation.py:88-106) is one
    in-place pass over the finished arrays.  ``x`` / ``u`` come back in the reference's axis order ``(Nx, N, B)`` as
    views of step-major storage.  (Measured at B = 2^20, N = 60, profiles/r2/collector_probe.txt.)
    """
    torch = _torch()
    s = env.spec
    B, N, dev = env.B, s.N, env.device
    if (policy is None) == (actions is None):
        raise ValueError("give exactly one of policy / actions")
    if env.per_env_t:
        raise ValueError("collect_rollouts needs a lock-stepped VecEnv")
    f64 = torch.float64
    o_hm = _affine(env, s.o_low, s.o_high, s.normalise_o)
    a_hm = _affine(env, s.a_low, s.a_high, s.normalise_a)
    r = torch.empty((1, N, B), dtype=f64, device=dev)
    r[0, 0] = 0.0
    g = torch.zeros((s.ncon, N, 1, B), dtype=f64, device=dev) if s.ncon else None
    obs, _ = env.reset()
    # the fused rollout records observations and rewards, not the constraint rows; per-env parameters roll through the
    # general rollout kernel's UNC form (RK4 / explicit pair, round 4); the 20-state DOPRI5 rollout kernel is slower than stepping (tools/rollout_probe.py)
    # (user models: the run-time compiled module carries its own rollout kernel for the register-only integrators)
    fused_ok = (not s.ncon and (not s.nunc or s.integrator in ("rk4", "dopri5")) and (s.integrator not in ("rodas3", "rodas4", "rodas5", "tsit5") or (s.integrator in ("rodas4", "rodas5") and s.model.name == "multistage_extraction"))
                and (s.user_rhs_src is None or s.integrator in ("rk4", "cv8", "dopri5"))
                # a plan with user expressions runs from its run-time compiled module, which carries a rollout kernel only
                # for the register-only explicit schemes (pcg_abi_jit.hip: jit_kernels): the Rosenbrock pairs step instead
                and not ((s.user_reward_src or s.user_cons_src) and s.integrator in ("rodas3", "rodas4", "rodas5"))
                and (s.integrator in ("rk4", "cv8") or s.nx <= 10))
    if actions is not None:
        actions = actions.to(device=dev, dtype=f64)
        if actions.shape != (N, s.na, B):
            raise ValueError(f"actions must have shape ({N},{s.na},{B})")
    if fused_unc and (policy is None or not fused_unc_ok(s, policy)):  # (closed loop only: `actions` comes without a policy)
        raise ValueError("fused_unc: this plan / policy does not qualify for pcg_rollout_policy_unc (fused_unc_ok; closed loop only)")
    if actions is not None and fused_ok:
        # fused: the kernel writes the observation rows directly into x[:, 1:, :] / r[0, 1:, :]
        x = torch.empty((s.nobs, N, B), dtype=f64, device=dev)
        x[:, 0] = env.obs_soa
        a = actions.contiguous()
        rc = env._lib.pcg_rollout_strided(
            env._plan, env._bufp, 0, N - 1, a.data_ptr(), s.na * B, B,
            x[:, 1:].data_ptr(), B, N * B, r[:, 1:].data_ptr(), B,
            env._episode_seed(), env._stream())
        _lib.check(rc, "pcg_rollout_strided")
        env.t += N - 1
        u = a if a_hm is None else _denorm_(a.clone(), a_hm, 1)  # never scale the caller's tensor in place
        return {"r": r, "x": _denorm_(x, o_hm, 0), "u": u.permute(1, 0, 2)}
    # which fused closed-loop entry point takes this plan and policy, if any: pcg_rollout_policy<kind>
    kind = None
    if policy is not None and fused_policy_ok(s, policy):
        kind = ""
    elif policy is not None and fused_cons_ok(s, policy):
        kind = "_cons"
    elif fused_unc:  # on request: the reset above sampled the parameters; the observation rows carry their slots, as the open loop's do
        kind = "_unc"
    if kind is not None:
        # closed loop in one launch: the kernel evaluates the policy between two steps and writes observations, policy
        # outputs (column N-1: the action proposed for the final observation) and rewards in the reference's axis order;
        # on a plan with constraint rows also every step's rows into g[:, 1:] (g[:, 0]: the first step's pre-step check,
        # pcgym.py:414-420)
        x = torch.empty((s.nobs, N, B), dtype=f64, device=dev)
        u = torch.empty((s.na, N, B), dtype=f64, device=dev)
        x[:, 0] = env.obs_soa
        rows = (g[:, 1:].data_ptr(), B, N * B, None, 0) if kind == "_cons" else ()
        env._buf.d = None
        rc = getattr(env._lib, "pcg_rollout_policy" + kind)(
            env._plan, env._bufp, policy.handle(dev), 0, N - 1, u.data_ptr(), B, N * B,
            x[:, 1:].data_ptr(), B, N * B, r[:, 1:].data_ptr(), B, 1, *rows, env._episode_seed(), env._stream())
        _lib.check(rc, "pcg_rollout_policy" + kind)
        env.t += N - 1
        out = {"r": r, "x": _denorm_(x, o_hm, 0), "u": _denorm_(u, a_hm, 0)}
        if kind == "_cons":
            g[:, 0, 0] = env.g_pre
            out["g"] = g
        return out
    # per-step path: step-major storage, the env's kernels write into it
    xs = torch.empty((N, s.nobs, B), dtype=f64, device=dev)
    us = torch.empty((N, s.na, B), dtype=f64, device=dev)
    xs[0] = env.obs_soa
    rs = r[0]
    with _recording(env):
        for i in range(N - 1):
            a = actions[i] if actions is not None else policy(obs)
            a = env._as_soa(a, s.na, "action")
            us[i] = a
            env.bind_outputs(xs[i + 1], rs[i + 1])
            obs, rew, done, _, info = env.step(a)
            if g is not None:
                if i == 0:
                    g[:, 0, 0] = env.g_pre
                g[:, i + 1, 0] = env.g
        if actions is None:
            us[N - 1] = env._as_soa(policy(obs), s.na, "action")
        else:
            us[N - 1] = actions[N - 1]
    out = {"r": r, "x": _denorm_(xs, o_hm, 1).permute(1, 0, 2), "u": _denorm_(us, a_hm, 1).permute(1, 0, 2)}
    if g is not None:
        out["g"] = g
    return out


def evaluate_population(env, pop, envs_per_policy, gamma=1.0, fused=None, fused_unc=False):
    """Score a :class:`~pcgym_amd.policy.PolicyPopulation` on a VecEnv: reset, one episode (N - 1 steps), env ``e`` driven by
    member ``(env.env_offset + e) // envs_per_policy`` -- the evaluation step of an evolution strategy, a cross-entropy search
    or a comparison of checkpoints under the same disturbances and noise.

    Returns {"ret": (B,) each env's discounted return, "score": (P_local,) the mean of ``ret`` over each member's envs}, for
    the members this env's slice of the global batch touches, in ascending order (the last member may have fewer envs).

    Route: ONE launch (``pcg_rollout_policy_pop``, the returns accumulated in the kernel) when ``fused_pop_ok`` and the env
    offset is a multiple of 64; otherwise -- or with ``fused=False`` -- one ``env.step`` per step with the population's
    callable form and the kernel's recurrence in torch (``J = J + disc * rew; disc = disc * gamma``).  ``fused=True`` raises
    ValueError where the one launch is not possible.  A float32 population takes the same routes: the float32 kernel, or the
    float32 callable per step.

    fused_unc : True takes ``pcg_rollout_policy_pop_unc`` -- one launch as well -- on a built-in RK4 plan with per-env parameters,
    and raises ValueError unless ``fused_pop_unc_ok(spec, pop, envs_per_policy)`` and the env offset is a multiple of 64, or
    together with ``fused=False``.  It has to be asked for: by default such a plan keeps the per-step loop, whose results the
    fused kernel matches to rounding and not to the bit (the two kernels are compiled separately).

    A plan WITH constraint rows takes ONE launch by default as well (``pcg_rollout_policy_pop_cons``, as ``collect_rollouts``
    takes ``pcg_rollout_policy_cons`` by default) when ``fused_pop_cons_ok`` and the env offset is a multiple of 64;
    ``fused=False`` keeps the step loop, ``fused=True`` raises ValueError where the launch is not possible (a constraint
    expression, rows together with per-env parameters, another integrator, slices that are not whole waves).  On such a plan
    BOTH routes return, beside ``ret`` and ``score``: "nviol" (B,) int32, the number of the episode's steps after which a row
    was violated; "gmax" (B,), the largest row value over the steps and rows (from -inf, ``gmax = where(g > gmax, g, gmax)``);
    "viol_share" (P_local,), the mean over each member's envs of ``nviol / T``, sliced as ``score`` is -- what a constrained
    search forms its fitness from (``score - lam * viol_share``; ``examples/policy_search_constrained.py``).  The launch keeps
    the three in registers; the step loop forms them in torch from ``env.viol`` / ``env.g``.  On the launch ``ret`` carries
    the kernel's network arithmetic in place of torch's: the two routes differ through the last bits of the actions alone,
    as on plans without rows.  A plan without rows returns ``ret`` and ``score`` alone."""
    torch = _torch()
    s = env.spec
    B, G, off = env.B, int(envs_per_policy), int(env.env_offset)
    if fused_unc and fused is False:
        raise ValueError("fused_unc=True asks for the one launch that fused=False declines")
    if fused_unc and not (fused_pop_unc_ok(s, pop, G) and off % 64 == 0):
        raise ValueError("fused_unc: this plan / population / slice size does not qualify for pcg_rollout_policy_pop_unc (fused_pop_unc_ok)")
    ok_cons = bool(s.ncon) and fused_pop_cons_ok(s, pop, G) and off % 64 == 0
    if fused and s.ncon and not ok_cons and not fused_unc:
        raise ValueError("this plan / population / slice size does not qualify for pcg_rollout_policy_pop_cons (fused_pop_cons_ok)")
    if env.per_env_t:
        raise ValueError("evaluate_population needs a lock-stepped VecEnv")
    if pop.n_in != s.nobs or pop.n_out != s.na:
        raise ValueError(f"the members map {pop.n_in} -> {pop.n_out}, the env {s.nobs} -> {s.na}")
    if G < 1 or (off + B - 1) // G >= pop.P:
        raise ValueError(f"envs {off} .. {off + B - 1} in slices of {G} need {(off + B - 1) // max(G, 1) + 1} members, the population has {pop.P}")
    if not (0.0 <= float(gamma) <= 1.0):
        raise ValueError(f"gamma must be within [0, 1], not {gamma}")
    ok = fused_pop_ok(s, pop, G) and off % 64 == 0
    if fused and not ok and not ok_cons and not fused_unc:
        raise ValueError("this plan / population / slice size does not qualify for the fused call (fused_pop_ok)")
    T = s.N - 1
    obs, _ = env.reset()
    nviol = gmax = None
    if fused_unc:  # on request: the reset above sampled the parameters
        ret = env.rollout_population_unc(pop, T, G, gamma=gamma)["ret"]
    elif ok and fused is not False:
        ret = env.rollout_population(pop, T, G, gamma=gamma)["ret"]
    elif ok_cons and fused is not False:
        o = env.rollout_population_cons(pop, T, G, gamma=gamma)
        ret, nviol, gmax = o["ret"], o["nviol"], o["gmax"]
    else:
        ret = torch.zeros(B, dtype=torch.float64, device=env.device)
        if s.ncon:
            nviol = torch.zeros(B, dtype=torch.int32, device=env.device)
            gmax = torch.full((B,), -float("inf"), dtype=torch.float64, device=env.device)
        disc = 1.0
        for _ in range(T):
            obs, rew, _, _, _ = env.step(pop(obs, G, off))
            ret = ret + disc * rew
            disc = disc * float(gamma)
            if s.ncon:  # the kernel's two statistics of the post-step rows, with its update of gmax, rows ascending
                nviol += env.viol.to(torch.int32)
                for row in env.g:
                    gmax = torch.where(row > gmax, row, gmax)

    # the mean over each member's envs: member m holds the envs [m G - off, (m + 1) G - off) of this batch
    def per_member(v):
        if off % G == 0 and B % G == 0:
            return v.view(-1, G).mean(dim=1)
        m0, m1 = off // G, (off + B - 1) // G
        bounds = [max(0, m * G - off) for m in range(m0, m1 + 1)] + [B]
        return torch.stack([v[bounds[i]:bounds[i + 1]].mean() for i in range(len(bounds) - 1)])

    out = {"ret": ret, "score": per_member(ret)}
    if s.ncon:
        out.update(nviol=nviol, gmax=gmax, viol_share=per_member(nviol.to(torch.float64) / T))
    return out


def centered_ranks(score):
    """What an evolution strategy weights its noise with (Salimans et al. 2017): the rank of each entry of ``score`` (P,)
    mapped to ``[-0.5, 0.5]`` -- the lowest score gets -0.5, the highest +0.5 -- as a float64 tensor on ``score``'s device.
    Ties are broken by index (a stable sort), so the result is deterministic; a single entry gets 0."""
    torch = _torch()
    score = torch.as_tensor(score)
    if score.dim() != 1 or score.shape[0] < 1:
        raise ValueError(f"centered_ranks takes a non-empty one-dimensional tensor, not {tuple(score.shape)}")
    P = int(score.shape[0])
    order = torch.argsort(score, stable=True)
    ranks = torch.empty(P, dtype=torch.float64, device=score.device)
    ranks[order] = torch.arange(P, dtype=torch.float64, device=score.device)
    if P == 1:
        return ranks
    return ranks / (P - 1) - 0.5


def _gae_fusable(rew, val, term):
    """why these tensors cannot go through ``pcg_gae`` (a string), or None: float64, on one GPU, 2-D, unit stride along B --
    row-sliced or padded views qualify through their row strides"""
    torch = _torch()
    if not rew.is_cuda:
        return "the tensors are not on a GPU"
    if rew.dim() != 2:
        return f"rew has {rew.dim()} dimensions, not 2"
    T, B = rew.shape
    if T < 1 or B < 1:
        return "an empty array"
    for name, t, want in (("rew", rew, torch.float64), ("val", val, torch.float64), ("term", term, (torch.bool, torch.uint8))):
        if t is None:
            continue
        if t.dtype != want and not (isinstance(want, tuple) and t.dtype in want):
            return f"{name} is {t.dtype}"
        if t.device != rew.device:
            return f"{name} is on {t.device}, rew on {rew.device}"
        if B > 1 and t.stride(1) != 1:
            return f"{name} has stride {t.stride(1)} along the env axis"
        if t.shape[0] > 1 and t.stride(0) < B:
            return f"{name} has row stride {t.stride(0)} < B = {B}"
    return None


def gae(rew, val, gamma=0.99, lam=0.95, bootstrap_last=False, term=None, fused=None):
    """Generalised advantage estimation over one episode for all envs at once (Schulman et al. 2016; stable-baselines3's
    ``RolloutBuffer.compute_returns_and_advantage``): rew (T, B), val (T + 1, B) -> (adv (T, B), ret (T, B)).

        delta_t = rew_t + gamma val_{t+1} - val_t;   adv_t = delta_t + gamma lam adv_{t+1};   ret_t = adv_t + val_t

    ``val[T]`` is the value of the observation after the last step.  ``bootstrap_last=False`` treats the episode's end as
    terminal (val[T] does not enter); ``True`` bootstraps from it (a time-limit truncation).

    ``term`` (T, B), bool or uint8: true where the episode of that env ENDED with step t (stable-baselines3's
    ``next_non_terminal`` is its negation).  There the recursion is cut: neither ``val[t+1]`` nor ``adv[t+1]`` enter step t.

    ``fused``: None takes ONE kernel launch (``pcg_gae``) when the tensors are float64, on a GPU, 2-D and have unit stride
    along B, and the loop of element-wise torch calls below otherwise (CPU tensors, other dtypes, more dimensions); False
    always takes the loop; True raises ValueError unless the kernel can take the tensors.  The two return the same bits:
    the kernel performs the loop's operations in the loop's order, each rounded on its own."""
    torch = _torch()
    T = rew.shape[0]
    if val.shape[0] != T + 1 or val.shape[1:] != rew.shape[1:]:
        raise ValueError(f"gae: rew {tuple(rew.shape)} needs val of shape ({T + 1}, ...), not {tuple(val.shape)}")
    if term is not None:
        if term.shape != rew.shape:
            raise ValueError(f"gae: term must have rew's shape {tuple(rew.shape)}, not {tuple(term.shape)}")
        if term.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"gae: term must be bool or uint8, not {term.dtype}")
    why = None if fused is False else _gae_fusable(rew, val, term)
    if fused and why is not None:
        raise ValueError(f"gae(fused=True): {why}")
    if fused is not False and why is None:
        B = rew.shape[1]
        adv = torch.empty((T, B), dtype=rew.dtype, device=rew.device)
        ret = torch.empty((T, B), dtype=rew.dtype, device=rew.device)
        with torch.cuda.device(rew.device):
            rc = _lib.load().pcg_gae(
                B, T, rew.data_ptr(), rew.stride(0), val.data_ptr(), val.stride(0),
                term.data_ptr() if term is not None else None, term.stride(0) if term is not None else 0,
                float(gamma), float(lam), int(bool(bootstrap_last)), adv.data_ptr(), B, ret.data_ptr(), B,
                torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "pcg_gae")
        return adv, ret
    adv = torch.empty_like(rew)
    last = torch.zeros_like(rew[0])
    zero = torch.zeros_like(rew[0])
    for t in range(T - 1, -1, -1):
        end = t == T - 1 and not bootstrap_last
        if term is None or end:
            nxt = zero if end else val[t + 1]
            c = zero if end else last
        else:
            cut = term[t] != 0
            nxt = torch.where(cut, zero, val[t + 1])
            c = torch.where(cut, zero, last)
        delta = rew[t] + gamma * nxt - val[t]
        last = delta + gamma * lam * c
        adv[t] = last
    return adv, adv + val[:T]


def collect_onpolicy(env, ac, gamma=0.99, lam=0.95, bootstrap_last=False, fused=None, record_cons=False, fused_unc=False,
                     terminate_on_violation=False):
    """One episode (N - 1 steps) of all B envs under the stochastic actor-critic ``ac`` (a
    :class:`~pcgym_amd.policy.GaussianActorCritic` with a critic): what an on-policy trainer such as PPO collects.

    Returns a dict of device tensors, step-major, in POLICY space (what the networks read and emit, not physical units):
        obs  (N, Nobs, B)  the policy's inputs, row 0 the reset observation
        act  (N-1, na, B)  the UNMAPPED samples u = mu + sigma z (the env applied out_map(u))
        logp (N-1, B)      log N(u; mu, sigma^2)
        val  (N, B)        critic values of obs; row N-1 is the bootstrap value
        rew  (N-1, B)
        adv, ret (N-1, B)  from :func:`gae` (one more launch, ``pcg_gae``, on either route)

    Route: ONE launch (``pcg_rollout_actor``) when the plan and the networks qualify (``fused_actor_ok``: RK4 / CV8, no
    constraint rows, no per-env parameters, no tanh map; user models and reward expressions included); otherwise -- or with ``fused=False`` -- one
    ``env.step`` per step with the sample formed in torch from ``env.policy_noise``, i.e. from the same random bits.
    ``fused_unc=True`` takes ``pcg_rollout_actor_unc`` -- one launch -- on a built-in RK4 plan with per-env parameters and raises
    ValueError unless ``fused_actor_unc_ok`` (float64 networks; not with ``record_cons`` or ``fused=False``).  It has to be asked
    for: by default, and under ``fused``, such a plan keeps the per-step route, whose results the fused kernel matches to
    rounding and not to the bit.

    ``record_cons=True`` (plans with constraint rows only, ValueError otherwise) adds what a constrained trainer needs -- a
    cost signal, a Lagrangian term, a mask after ``done_on_cons_vio``:
        g     (N-1, ncon, B)  the constraint rows after every step
        g_pre (ncon, B)       the rows of the pre-step check of the first step (pcgym.py:414-420)
        viol  (N-1, B)        bool, any row > 0
    on both routes: ONE launch (``pcg_rollout_actor_cons``) when ``fused_actor_cons_ok`` (a built-in RK4 / CV8 plan with
    affine rows, float64 networks), the per-step loop otherwise or with ``fused=False``; ``fused=True`` then raises only
    when ``fused_actor_cons_ok`` is false.  An env whose ``done`` is set mid-episode keeps stepping on both routes.

    ``terminate_on_violation=True`` (needs ``record_cons=True``, ValueError otherwise) treats a violation as the end of that
    env's episode in the estimator, as every on-policy trainer treats a terminal step: ``viol`` is passed to :func:`gae` as
    ``term``, so ``adv`` / ``ret`` of a violating step see neither the value nor the advantage of what follows.  The env
    still steps on; what follows is recorded and marked by one more entry,
        alive (N-1, B)  bool, no EARLIER step of that env violated (the violating step itself is alive)
    the mask for the trainer's loss.  The default returns today's dict with today's values."""
    torch = _torch()
    s = env.spec
    B, N, dev, f64 = env.B, s.N, env.device, torch.float64
    if env.per_env_t:
        raise ValueError("collect_onpolicy needs a lock-stepped VecEnv")
    if ac.critic is None:
        raise ValueError("collect_onpolicy needs a critic: the advantages are estimated from its values")
    if ac.n_in != s.nobs or ac.n_out != s.na:
        raise ValueError(f"the actor maps {ac.n_in} -> {ac.n_out}, the env {s.nobs} -> {s.na}")
    T = N - 1
    obs = torch.empty((N, s.nobs, B), dtype=f64, device=dev)
    act = torch.empty((T, s.na, B), dtype=f64, device=dev)
    logp = torch.empty((N, B), dtype=f64, device=dev)
    val = torch.empty((N, B), dtype=f64, device=dev)
    rew = torch.empty((T, B), dtype=f64, device=dev)
    o, _ = env.reset()
    obs[0] = env.obs_soa
    if record_cons and not s.ncon:
        raise ValueError("record_cons: this plan has no constraint rows")
    if terminate_on_violation and not record_cons:
        raise ValueError("terminate_on_violation needs record_cons=True: the violation flags are what cuts the recursion")
    # a plan with per-env parameters: pcg_rollout_actor_unc, on request only (the default route of such a plan stays the step loop)
    unc = bool(fused_unc)
    if unc and (record_cons or fused is False or not fused_actor_unc_ok(s, ac)):
        raise ValueError("fused_unc: this plan / actor-critic does not qualify for pcg_rollout_actor_unc (fused_actor_unc_ok)")
    ok = fused_actor_cons_ok(s, ac) if record_cons else (unc or fused_actor_ok(s, ac))
    if fused and not ok:
        raise ValueError("this plan / actor-critic does not qualify for the fused call")
    cons = {}
    if record_cons:
        cons = {"g": torch.empty((T, s.ncon, B), dtype=f64, device=dev), "g_pre": None,
                "viol": torch.empty((T, B), dtype=torch.uint8, device=dev)}
    if ok and fused is not False:
        # (row N-1 of the samples is drawn and dropped: only its value, the bootstrap value, is kept)
        u = torch.empty((N, s.na, B), dtype=f64, device=dev)
        name = "pcg_rollout_actor" + ("_cons" if record_cons else "_unc" if unc else "")
        rows = (cons["g"].data_ptr(), s.ncon * B, B, cons["viol"].data_ptr(), B) if record_cons else ()
        env._buf.d = None
        rc = getattr(env._lib, name)(
            env._plan, env._bufp, ac.actor.handle(dev), ac.critic.handle(dev), ac.sigma.ctypes.data_as(C.POINTER(C.c_double)),
            0, T, None, 0, 0, u.data_ptr(), s.na * B, B, logp.data_ptr(), B, val.data_ptr(), B,
            obs[1:].data_ptr(), s.nobs * B, B, rew.data_ptr(), B, 1, *rows, env._episode_seed(), env._stream())
        _lib.check(rc, name)
        env.t += T
        act = u[:T]
        if record_cons:
            cons["g_pre"] = env.g_pre.clone()
    else:
        z = torch.empty((s.na, B), dtype=f64, device=dev)
        with _recording(env):
            for i in range(T):
                env.policy_noise(i, out=z)
                zt = z.t()
                u = ac.sample(o, zt)
                act[i] = u.t()
                logp[i] = ac.log_prob_z(zt)
                val[i] = ac.value(o)
                env.bind_outputs(obs[i + 1], rew[i])
                o, _, _, _, _ = env.step(ac.action(u))
                if record_cons:
                    if i == 0:
                        cons["g_pre"] = env.g_pre.clone()
                    cons["g"][i] = env.g
                    cons["viol"][i] = env.viol
            val[T] = ac.value(o)
    adv, ret = gae(rew, val, gamma, lam, bootstrap_last, term=cons["viol"] if terminate_on_violation else None)
    out = {"obs": obs, "act": act, "logp": logp[:T], "val": val, "rew": rew, "adv": adv, "ret": ret}
    if record_cons:
        cons["viol"] = cons["viol"].view(torch.bool)
        out.update(cons)
    if terminate_on_violation:  # exclusive cumulative-or over the steps
        alive = torch.ones((T, B), dtype=torch.bool, device=dev)
        alive[1:] = torch.cumsum(cons["viol"][:-1], 0) == 0
        out["alive"] = alive
    return out


class reproducibility_metric:
    """Same constructor / methods / dict shapes as the reference class (evaluation_metrics.py:182-327), computed with
    torch on whatever device the data lives on.  The reductions run along the last axis (the reps / env axis).

    Pinned to the reference's own outputs (tests/golden/metrics_ref.npz, generated by importing evaluation_metrics.py).
    Quirk Q14 (`reference_compat=True`, the default): the reference's MAD subtracts the median WITHOUT keeping the reduced
    axis (evaluation_metrics.py:127-130, "currently only works for the reward component"), so `data - median` follows
    NumPy broadcasting: on (n, N, reps) data it raises unless N == reps (and then subtracts the median of another
    time index), on the constraint component (N, 1, reps) it returns an (N, N) table, 1-D data is reshaped to (n, 1)
    first.  All of that is reproduced, including the ValueError.  `reference_compat=False` gives the median absolute
    deviation about each row's own median, for every shape."""

    def __init__(self, dispersion: str, performance: str, scalarised_weight: float, reference_compat: bool = True):
        if dispersion not in ("std", "mad"):
            raise ValueError("Invalid dispersion metric")
        if performance not in ("mean", "median"):
            raise ValueError("Invalid performance metric")
        self.dispersion, self.performance, self.scalarised_weight = dispersion, performance, scalarised_weight
        self.reference_compat = bool(reference_compat)

    @staticmethod
    def _median(t):
        # np.median averages the two middle values for even counts; torch.median returns the lower one
        torch = _torch()
        return torch.quantile(t, 0.5, dim=-1)

    def _op(self, comp, t):
        return t.amax(dim=0) if comp == "g" else t  # greatest constraint row (evaluation_metrics.py:322-326)

    def _perf(self, t):
        return t.mean(dim=-1) if self.performance == "mean" else self._median(t)

    def _disp(self, t):
        if self.dispersion == "std":
            return t.std(dim=-1, unbiased=False)  # np.std default (ddof = 0)
        if not self.reference_compat:
            return self._median((t - self._median(t).unsqueeze(-1)).abs())
        if t.dim() < 2:  # evaluation_metrics.py:112-114
            t = t.reshape(t.shape[0], 1)
        med = self._median(t)
        try:
            dev = t - med  # NumPy broadcasting of (.., reps) against (..): evaluation_metrics.py:127-130
        except RuntimeError as e:
            raise ValueError(f"operands could not be broadcast together with shapes {tuple(t.shape)} "
                             f"{tuple(med.shape)} (the reference's MAD, evaluation_metrics.py:127-130: quirk Q14; "
                             "reference_compat=False gives the deviation about each row's own median)") from e
        return self._median(dev.abs())

    def _apply(self, fn, data, component):
        out = {k: {} for k in data}
        for pol, d in data.items():
            for comp in (d.keys() if component is None else [component]):
                out[pol][comp] = fn(self._op(comp, _torch().as_tensor(d[comp])))
        return out

    def policy_performance_metric(self, data, component=None):
        return self._apply(self._perf, data, component)

    def policy_dispersion_metric(self, data, component=None):
        return self._apply(self._disp, data, component)

    def scalarised_performance(self, data, component=None):
        p = self.policy_performance_metric(data, component)
        d = self.policy_dispersion_metric(data, component)
        return {k: {c: p[k][c] + self.scalarised_weight * d[k][c] for c in p[k]} for k in p}

    def evaluate(self, policy_evaluator, component=None):
        data = getattr(policy_evaluator, "data", None)
        if data is None:
            data = policy_evaluator.get_rollouts()
        return self.scalarised_performance(data, component)
