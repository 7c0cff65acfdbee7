"""Recorded step graphs run a run of consecutive lean pipelined RK4 steps as ONE chained launch (pcg_graph_create,
step_chain_kernel): a tile's state stays in registers from the run's first step to its last, every step still stores its
observation, reward and done bytes, the state goes back once.

The twin method is that of test_gpu_graph_held_rows.py: every comparison is bitwise against a twin VecEnv stepped eagerly
with step(); the graph env's observation and reward are filled with NaN and its done bytes with 0xFF before each replay,
and each graph is replayed twice.  StepGraph.chained is held against what the rule gives, worked out here from T and the
plan's route: a lean RK4 graph of T >= 2 steps without per-step disturbances is one chain of T steps, anything else none.
StepGraph.held against the numpy rule of the held-rows test: a chained step counts like any other recorded step.

The kernel fetches its actions in groups of D steps, D a compile-time constant of the library chosen among {1, 2, 4, 8}: the
run lengths below are the union of {1, 2, D - 1, D, D + 1, 2 D + 1} over those four values, so the group boundaries of
whichever D the library was built with are covered."""
import copy

import numpy as np
import pytest

import helpers as H
import scenarios as SC
from test_gpu_graph_held_rows import _actions, _assert_same, _expected_held

pytestmark = pytest.mark.gpu

RUN_LENGTHS = sorted({T for D in (1, 2, 4, 8) for T in (1, 2, D - 1, D, D + 1, 2 * D + 1) if T >= 1})


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU test selected but no GPU visible"
    return torch


def _params(name, **over):
    """cstr forced to RK4 (its default is the adaptive pair); four_tank on its default CV8 unless `over` says otherwise"""
    p = copy.deepcopy(SC.scenarios()[name]["env_params"])
    if p.get("model") == "cstr":
        p["integrator"] = "rk4"
    p.update(over)
    return p


def _bench_actions(spec, T, B, seed):
    """as bench.py draws them: the full box, except four_tank's pump voltages in its upper 3/4 (no tank drains)"""
    rng = np.random.default_rng(seed)
    lo = -0.5 if spec.model.name == "four_tank" else -1.0
    a = rng.uniform(lo, 1.0, (T, spec.na, B))
    if not spec.normalise_a:
        al, ah = spec.a_low[None, :, None], spec.a_high[None, :, None]
        a = al + (a + 1) / 2 * (ah - al)
    return a


def _poison(env):
    env.obs_soa.fill_(float("nan"))
    env.rew.fill_(float("nan"))
    env.done.fill_(0xFF)


def _chain_rule(T, lean_rk4=True):
    """(launches, steps) of a graph of T plain steps"""
    return (1, T) if lean_rk4 and T >= 2 else (0, 0)


def _run(p, B, t0, T, with_reset, seed=0, act_list=None, stream=False, reseed=False):
    """Twin check of one graph, replayed twice with the buffers poisoned before each replay; returns (held, chained, spec).
    with_reset: the graph resets and runs T steps from t = 0, so the second replay is a second episode.  Otherwise both
    envs are brought to t0 eagerly before each replay.  act_list(acts) -> the T recorded action tensors (default: the
    rows acts[t0 + j] of one allocation); stream: replay on a stream of its own; reseed: pcg_graph_set_seed between the
    two replays."""
    torch = _torch()
    from pcgym_amd import VecEnv, _lib

    ref = VecEnv(copy.deepcopy(p), n_envs=B, seed=3)
    env = VecEnv(copy.deepcopy(p), n_envs=B, seed=3)
    s = env.spec
    acts = torch.tensor(_actions(s, t0 + T, B, seed), device=env.device)
    rec = [acts[t0 + j] for j in range(T)] if act_list is None else act_list(acts[t0:])
    side = torch.cuda.Stream() if stream else None
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
                g = env.capture_steps(rec, with_reset=with_reset)
            elif reseed:
                _lib.check(env._lib.pcg_graph_set_seed(g._g, 12345 + rep), "pcg_graph_set_seed")
            for j in range(T):
                ref.step(rec[j])
            _poison(env)
            if side is not None:
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    g.replay()
                torch.cuda.current_stream().wait_stream(side)
            else:
                g.replay()
            torch.cuda.synchronize()
            _assert_same(ref, env, (B, t0, T, with_reset, rep))
        return g.held, g.chained, s
    finally:
        if g is not None:
            g.destroy()
        ref.close()
        env.close()


# cstr_canonical: N = 60, the set-point steps at t = 20 and t = 40, done flips at t = 58
@pytest.mark.parametrize("T", RUN_LENGTHS)
@pytest.mark.parametrize("B", [2, 510, 777, 4096])
def test_chain_lengths_across_set_point_change(B, T):
    """B = 2: one lane; 510: partial tile; 777: odd, one env per lane; 4096: several workgroups.  From t0 = 17: runs of
    four steps and more cross the set-point change at t = 20."""
    t0 = 17
    held, chained, s = _run(_params("cstr_canonical"), B, t0, T, False, seed=T)
    assert chained == _chain_rule(T)
    assert held == _expected_held(s, t0, T)
    assert held[1] == T - 1  # done stays 0: every step but the first holds it


@pytest.mark.parametrize("B", [777, 4096])
def test_chain_ends_on_the_last_step(B):
    t0, T = 50, 9  # t = 50 .. 58: done flips in the chain's last step
    held, chained, s = _run(_params("cstr_canonical"), B, t0, T, False, seed=1)
    assert t0 + T == s.N - 1
    assert chained == (1, T)
    assert held == _expected_held(s, t0, T)
    assert held[1] == T - 2


@pytest.mark.parametrize("B", [510, 4096])
def test_whole_episode_with_reset(B):
    p = _params("cstr_canonical")
    T = p["N"] - 1
    held, chained, s = _run(p, B, 0, T, True, seed=2)
    assert chained == (1, T)
    assert held == _expected_held(s, 0, T)
    assert held == (T - 1 - 2, T - 2)  # two set-point changes; step 0 and the last step store done


@pytest.mark.parametrize("B", [1024, 999])
def test_four_tank_rk4(B):
    """four states, two set-point slots that step together mid-episode: a whole episode with its reset, then steps only,
    across the change"""
    p = _params("four_tank_canonical", integrator="rk4")
    T = p["N"] - 1
    held, chained, s = _run(p, B, 0, T, True, seed=4)
    assert s.integrator == "rk4" and s.nsp_obs == 2
    assert chained == (1, T)
    assert held == _expected_held(s, 0, T)
    assert 0 < held[0] < T - 1 and held[1] == T - 2
    t0, T = 27, 6
    held, chained, s = _run(p, B, t0, T, False, seed=5)
    assert chained == (1, T)
    assert held == _expected_held(s, t0, T)
    assert 0 < held[0] < T - 1 and held[1] == T - 1


@pytest.mark.parametrize("name,over", [("cstr_canonical", {}), ("four_tank_canonical", {"integrator": "rk4"})])
@pytest.mark.parametrize("B", [777, 1026])  # odd: one env per lane; even: two
def test_chained_replay_vs_oracle(name, over, B):
    """x / obs / rew of a chained replay against the oracle stepped with the same actions, at the bar of
    test_gpu_parity.test_batched_step_vs_oracle for these plans (1e-12 on the state, 10 x on the observation, 100 x on the
    reward, 12 steps from the reset state)"""
    torch = _torch()
    from oracle import oracle as O
    from pcgym_amd import VecEnv

    T, tol = 12, 1e-12
    env = VecEnv(_params(name, **over), n_envs=B, seed=5)
    s = env.spec
    assert s.integrator == "rk4"
    orc = O.OracleEnv(s, B, seed=5)
    acts = _bench_actions(s, T, B, 3)
    dev = torch.tensor(acts, device=env.device)
    g = env.capture_steps([dev[i] for i in range(T)], with_reset=True)
    try:
        assert g.chained == (1, T)
        _poison(env)
        og, rg, dg = g.replay()
        torch.cuda.synchronize()
        orc.reset()
        for i in range(T):
            oc, rc, dc = orc.step(acts[i])
        assert np.isfinite(orc.x).all()
        xs = np.maximum(np.abs(orc.x), 1e-6 * np.max(np.abs(orc.x), axis=1, keepdims=True))
        ex = np.max(np.abs(env.x.cpu().numpy() - orc.x) / xs)
        eo = np.max(np.abs(og.cpu().numpy().T - oc) / np.maximum(np.abs(oc), 1e-3))
        er = np.max(np.abs(rg.cpu().numpy() - rc) / np.maximum(np.abs(rc), 1.0))
        print(f"{name} B={B}: x {ex:.2e} obs {eo:.2e} rew {er:.2e}")
        assert ex <= tol and eo <= 10 * tol and er <= max(100 * tol, 1e-10), (ex, eo, er)
        assert np.array_equal(dg.cpu().numpy().astype(np.uint8), dc)
        assert not env.status.any()
    finally:
        g.destroy()
        env.close()


# ---- fall-backs: every step a launch of its own, same results ----------------------------------------------------------
def test_switch_turns_chaining_off(monkeypatch):
    """PCG_NO_CHAIN, read when the plan is created"""
    monkeypatch.setenv("PCG_NO_CHAIN", "1")
    held, chained, s = _run(_params("cstr_canonical"), 4096, 17, 6, False)
    assert chained == (0, 0)
    assert held == _expected_held(s, 17, 6)


def test_four_tank_default_scheme_is_not_chained():
    p = _params("four_tank_canonical")
    held, chained, s = _run(p, 1024, 27, 6, False, seed=5)
    assert s.integrator == "cv8"
    assert chained == (0, 0)
    assert held == _expected_held(s, 27, 6)


def test_other_routes_are_not_chained():
    """observation noise: the plan leaves the lean route, every step is recorded as the launch it was"""
    p = _params("cstr_canonical", noise=True, noise_percentage=0.01)
    held, chained, _ = _run(p, 1000, 17, 6, False)
    assert chained == (0, 0) and held == (0, 0)


def test_one_step_is_not_a_chain():
    held, chained, _ = _run(_params("cstr_canonical"), 4096, 17, 1, False)
    assert chained == (0, 0) and held == (0, 0)


# ---- where the actions live --------------------------------------------------------------------------------------------
def test_repeated_and_separate_action_tensors():
    p = _params("cstr_canonical")
    # three tensors of their own, recorded round-robin
    held, chained, _ = _run(p, 4096, 17, 7, False, seed=6,
                            act_list=lambda a: [t for _ in range(3) for t in [a[0].clone(), a[1].clone(), a[2].clone()]][:7])
    assert chained == (1, 7)
    # the same tensor in every step
    held, chained, _ = _run(p, 510, 17, 5, False, seed=7, act_list=lambda a: [a[0]] * 5)
    assert chained == (1, 5)


def test_one_misaligned_action_row_takes_one_env_per_lane():
    """even B, every buffer 16-byte aligned but ONE recorded action tensor, which sits 8 bytes off: the whole run takes the
    one-env-per-lane instantiation (the eager twin takes it for that step alone), same bytes"""
    torch = _torch()
    from pcgym_amd import _lib

    B, T = 4096, 6

    def rec(a):
        flat = torch.empty(a[3].numel() + 1, dtype=torch.float64, device=a.device)
        off = flat[1:].view_as(a[3])
        off.copy_(a[3])
        assert off.data_ptr() % 16 == 8 and off.is_contiguous()
        assert all(a[j].data_ptr() % 16 == 0 for j in range(T))
        return [a[0], a[1], a[2], off, a[4], a[5]]

    lib = _lib.load()
    held, chained, _ = _run(_params("cstr_canonical"), B, 17, T, False, seed=8, act_list=rec)
    assert chained == (1, T)
    if lib.pcg_coverage_names(None, 0, 0) >= 0:  # the launch record is on (the GPU suite's conftest turns it on)
        names = [n for n in H._launch_names(lib) if "17step_chain_kernelI" in n]
        assert names and all(n.endswith("ELi1EEEvNS_8StepArgsE") for n in names), names


def test_set_seed_on_a_chained_graph():
    held, chained, _ = _run(_params("cstr_canonical"), 4096, 17, 6, False, seed=9, reseed=True)
    assert chained == (1, 6)
    p = _params("cstr_canonical")
    held, chained, _ = _run(p, 510, 0, p["N"] - 1, True, seed=10, reseed=True)
    assert chained == (1, p["N"] - 1)


def test_replay_on_a_side_stream():
    held, chained, _ = _run(_params("cstr_canonical"), 4096, 17, 9, False, seed=11, stream=True)
    assert chained == (1, 9)


def test_bytes_per_env_step_follows_what_the_replays_move():
    """VecEnv.bytes_per_env_step is pcg_plan_bytes_per_env_step's formula (cstr: 73) until a graph is replayed, then the mean
    over the env's steps of what their launches move.  A chained cstr step reads its action (8) and writes two observation
    rows and the reward (24); the slot row (8) and the done byte (1) unless held; the state (16 + 16) once per chain."""
    torch = _torch()
    from pcgym_amd import VecEnv

    B, t0, T = 4096, 17, 6  # the set-point changes at t = 20: five steps hold done, four the slot row
    env = VecEnv(_params("cstr_canonical"), n_envs=B, seed=3)
    try:
        acts = torch.tensor(_actions(env.spec, t0 + T, B, 0), device=env.device)
        assert env.bytes_per_env_step == 73
        env.reset()
        for i in range(t0):
            env.step(acts[i])
        assert env.bytes_per_env_step == 73
        g = env.capture_steps([acts[t0 + j] for j in range(T)])
        assert g.chained == (1, T) and g.held == (4, 5)
        want = T * (8 + 24) + 8 * (T - 4) + (T - 5) + 32
        assert g.bytes_per_env == want == T * 73 - 8 * 4 - 5 - 32 * (T - 1)
        g.replay()
        torch.cuda.synchronize()
        assert env.bytes_per_env_step == round((73 * t0 + want) / (t0 + T))
        g.destroy()
    finally:
        env.close()
