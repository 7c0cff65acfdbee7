"""Recorded step graphs skip the stores of wave-uniform rows the node before them left unchanged (pcg_graph_create,
StepArgs::held): the observation's set-point / disturbance slot rows and the done bytes of the lean pipelined kernel.

Every comparison is bitwise (torch.equal) against a twin VecEnv stepped eagerly with step(), which stores every row in
every step.  The graph env's observation is filled with NaN and its done bytes with 0xFF before each replay, so a row
that no node of the replay stored cannot pass.  StepGraph.held is held against counts worked out here from the spec's
schedules with numpy -- node j >= 1 holds the slot rows iff the normalised slot values of steps t0 + j and t0 + j - 1
are equal, and the done bytes iff the two steps' flags are -- not by calling the library's rule."""
import copy

import numpy as np
import pytest

import scenarios as SC

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU test selected but no GPU visible"
    return torch


def _params(name):
    """the scenario's configuration; cstr forced to RK4 (its default is the adaptive pair), four_tank on its default CV8"""
    p = copy.deepcopy(SC.scenarios()[name]["env_params"])
    if p.get("model") == "cstr":
        p["integrator"] = "rk4"
    return p


def _actions(spec, T, B, seed):
    rng = np.random.default_rng(seed)
    if spec.normalise_a:
        return rng.uniform(-1, 1, (T, spec.na, B))
    return rng.uniform(spec.a_low[None, :, None], spec.a_high[None, :, None], (T, spec.na, B))


def _slot_values(s, t):
    """the set-point and disturbance slots of the observation step t -> t + 1 writes (pcgym.py:394,438: SP[t], D[t + 1],
    clamped to the last column), normalised like the observation"""
    v = np.array([s.sp[k, min(t, s.N - 1)] for k in range(s.nsp_obs)] +
                 [s.d_sched[k, min(t + 1, s.N - 1)] for k in range(s.nd)], dtype=np.float64)
    if s.normalise_o:
        lo, hi = s.o_low[s.nx:s.nx + v.size], s.o_high[s.nx:s.nx + v.size]
        v = 2.0 * (v - lo) / (hi - lo) - 1.0
    return v


def _expected_held(s, t0, T):
    slot = sum(bool(np.array_equal(_slot_values(s, t0 + j), _slot_values(s, t0 + j - 1))) for j in range(1, T))
    done = sum((t0 + j + 1 == s.N - 1) == (t0 + j == s.N - 1) for j in range(1, T))
    return slot, done


def _poison(env):
    env.obs_soa.fill_(float("nan"))
    env.done.fill_(0xFF)


def _assert_same(ref, env, what):
    torch = _torch()
    assert ref.t == env.t, what
    for k in ("x", "obs_soa", "rew", "done", "status"):
        a, b = getattr(ref, k), getattr(env, k)
        if a.dtype.is_floating_point:
            # the bit patterns: an env that random actions drive to a non-finite state (a four_tank level below zero)
            # carries the same NaN in both, which an equality of values would call different
            a, b = a.view(torch.int64), b.view(torch.int64)
        assert torch.equal(a, b), (what, k)


def _run(p, B, t0, T, with_reset, seed=0):
    """Twin check of one graph, replayed twice with the buffers poisoned before each replay; returns (held, spec).
    with_reset: the graph resets and runs T steps from t = 0, so the second replay is a second episode.  Otherwise both
    envs are brought to t0 eagerly before each replay."""
    torch = _torch()
    from pcgym_amd import VecEnv

    ref = VecEnv(copy.deepcopy(p), n_envs=B, seed=3)
    env = VecEnv(copy.deepcopy(p), n_envs=B, seed=3)
    s = env.spec
    acts = torch.tensor(_actions(s, t0 + T, B, seed), device=env.device)
    g = None
    try:
        for rep in range(2):
            ref.reset()
            if not with_reset:
                env.reset()
                for i in range(t0):
                    ref.step(acts[i])
                    env.step(acts[i])
            if g is None:
                g = env.capture_steps([acts[t0 + j] for j in range(T)], with_reset=with_reset)
            for j in range(T):
                ref.step(acts[t0 + j])
            _poison(env)
            g.replay()
            torch.cuda.synchronize()
            _assert_same(ref, env, (B, t0, T, with_reset, rep))
        return g.held, s
    finally:
        if g is not None:
            g.destroy()
        ref.close()
        env.close()


def _b_second_iteration():
    """just past what one resident grid of the pipelined kernel covers at two envs per lane (five workgroups per CU, 512
    envs each), with a ragged tail: the persistent loop runs a second, partial iteration"""
    torch = _torch()
    return torch.cuda.get_device_properties(0).multi_processor_count * 5 * 512 + 1026


# cstr_canonical: N = 60, the set-point steps at t = 20 and t = 40, done flips at t = 58
@pytest.mark.parametrize("B", [2, 510, 777, 4096, "grid+1026"])
def test_graph_across_set_point_change(B):
    """B = 2: one lane; 510: partial tile; 777: odd, one env per lane; 4096: several workgroups; the last one: a second,
    partial iteration of the persistent loop"""
    if B == "grid+1026":
        B = _b_second_iteration()
    t0, T = 17, 6
    held, s = _run(_params("cstr_canonical"), B, t0, T, False)
    assert held == _expected_held(s, t0, T)
    assert 0 < held[0] < T - 1  # some nodes hold the slot rows, the node of the change does not
    assert held[1] == T - 1     # done stays 0: every node but the first holds it


@pytest.mark.parametrize("B", [777, 4096])
def test_graph_with_last_step(B):
    t0, T = 50, 9  # t = 50 .. 58
    held, s = _run(_params("cstr_canonical"), B, t0, T, False, seed=1)
    assert t0 + T == s.N - 1
    assert held == _expected_held(s, t0, T)
    assert held[1] == T - 2  # neither node 0 nor the last one, where done flips to 1


@pytest.mark.parametrize("B", [510, 4096])
def test_graph_with_reset_whole_episode(B):
    p = _params("cstr_canonical")
    T = p["N"] - 1
    held, s = _run(p, B, 0, T, True, seed=2)
    assert held == _expected_held(s, 0, T)
    assert held == (T - 1 - 2, T - 2)  # two set-point changes; node 0 and the last step store done


@pytest.mark.parametrize("B", [1024, 999])
def test_four_tank_two_set_point_slots(B):
    """the CV8 pipelined kernel, two set-point slots that step together mid-episode: a whole episode with its reset"""
    p = _params("four_tank_canonical")
    T = p["N"] - 1
    held, s = _run(p, B, 0, T, True, seed=4)
    assert s.integrator == "cv8" and s.nsp_obs == 2
    assert held == _expected_held(s, 0, T)
    assert 0 < held[0] < T - 1 and held[1] == T - 2
    # ... and steps only, across the change
    t0, T = 27, 6
    held, s = _run(p, B, t0, T, False, seed=5)
    assert held == _expected_held(s, t0, T)
    assert 0 < held[0] < T - 1 and held[1] == T - 1


def test_scheduled_disturbance_slot():
    """cstr_dist_Ti: a scheduled inlet temperature that steps at columns 15 and 45, no Gaussian part and no per-env values
    -- a lean plan whose observation carries a disturbance slot (LeanStep::od).  That it takes the lean pipelined kernel
    shows in held itself: no other route holds anything."""
    p = _params("cstr_dist_Ti")
    t0, T = 10, 8  # the slot shows D[t + 1]: it changes in step t = 14
    held, s = _run(p, 1026, t0, T, False, seed=6)
    assert s.nd == 1 and not s.gauss
    assert held[1] == T - 1  # precondition: the lean route (done held in every node but the first)
    assert held == _expected_held(s, t0, T)
    assert held[0] == T - 2
    # a graph over both kinds of change (set-point at t = 20, disturbance in step t = 44) and the last step
    T = p["N"] - 1
    held, s = _run(p, 1026, 0, T, True, seed=7)
    assert held == _expected_held(s, 0, T)
    assert held == (T - 1 - 4, T - 2)


def test_switch_turns_holding_off(monkeypatch):
    """PCG_NO_HELD_ROWS, read when the plan is created: nothing is held, results are the same"""
    monkeypatch.setenv("PCG_NO_HELD_ROWS", "1")
    held, _ = _run(_params("cstr_canonical"), 4096, 17, 6, False)
    assert held == (0, 0)
    p = _params("cstr_canonical")
    held, _ = _run(p, 510, 0, p["N"] - 1, True, seed=2)
    assert held == (0, 0)


def test_other_routes_hold_nothing():
    """observation noise and a Gaussian disturbance: the plan leaves the lean route, every node stores everything"""
    torch = _torch()
    from pcgym_amd import VecEnv

    p = _params("cstr_dist_Ti")
    p.update(noise=True, noise_percentage=0.01, gaussian_disturbances={"Ti": 2.0})
    B = 1000
    ref = VecEnv(copy.deepcopy(p), n_envs=B, seed=5)
    env = VecEnv(copy.deepcopy(p), n_envs=B, seed=5)
    T = env.N - 1
    acts = torch.tensor(_actions(env.spec, T, B, 2), device=env.device)
    g = env.capture_steps([acts[i] for i in range(T)], with_reset=True)
    assert g.held == (0, 0)
    for ep in range(2):
        ref.reset()
        for i in range(T):
            ref.step(acts[i])
        _poison(env)
        g.replay()
        _assert_same(ref, env, ep)
    g.destroy()
    ref.close()
    env.close()
