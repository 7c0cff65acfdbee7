"""The fused closed-loop rollout of a POPULATION of MLP policies on plans WITH per-env model parameters
(pcg_rollout_policy_pop_unc, pcg_rollout_pop_unc.hpp): every slice of `envs_per_policy` consecutive envs driven by its own member,
every env integrating with its own parameters, one launch; float64 and float32 members.

Shapes are the population tests': B = 200, T = 6, G = 64 -- three full waves and a wave of 8 lanes, four members.  Plans are
test_gpu_unc_rollout's (_params: the model's first two non-zero parameters +-3 % per env, every env its own initial state
+-2 %), tolerances the project's own for per-env parameters (helpers._tols, _rew_close, worst_rel).

The step is compiled in these kernels on its own (the compiler's default contraction), so equal bits are asked only where the
SAME kernel runs twice -- copies of a member against the mixed population, one call against chunks, shards against the whole,
eager against a replayed graph -- and every comparison with another kernel (the oracle, rollout_policy_unc, the per-step route)
uses the tolerances.

   1. every instantiation   each key x dtype against the oracle, teacher-forced, three one-step calls;
   2. the networks          every recorded action against its OWN member on the host, on the kernel's own observation;
   3. members               four copies of member m give, on slice m, the mixed population's bits;
   4. rollout_policy_unc    slice by slice with pop.member(m), to rounding (fp64);
   5. chunks and returns    one call equals chunked calls bitwise; ret is the stated recurrence over each chunk's rewards;
   6. shards                env offsets 0 and 128 against the one env of 200;
   7. update_ / set_flat_   rewriting member 2 changes slice 2's bits and no other;
   8. public path           evaluate_population(fused_unc=True) against the per-step route, teacher-forced;
   9. refusals              the statuses in the documented order, nothing launched, nothing written;
  10. stream capture        one call inside torch.cuda.graph, replayed twice, equal to the eager call.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import scenarios as SC
from helpers import (LD, MODEL_KEYS, PRE_MAX, _final_equal, _launch_names, _launched, _make, _perm_hidden, _rew_close, _tols, _torch,
                     host_reference, make_policy, sweep_params, tanh_k, worst_rel)
from test_gpu_pop_rollout import _returns
from test_gpu_unc_rollout import KEYS, SEED, _envs, _params

pytestmark = pytest.mark.gpu

B, T, G = 200, 6, 64  # three full waves and a wave of 8 lanes: four members
DTYPES = ("float64", "float32")
# (mangled names: the template argument list follows the name, which tells the fp64 kernel from its _f32 twin)
KERNEL = {"float64": "rollout_pop_unc_policy_kernelI", "float32": "rollout_pop_unc_policy_kernel_f32I"}
KW = dict(collect_obs=True, collect_rew=True, collect_actions=True, record_next_action=True)
NAMES = ("a", "obs", "rew", "ret")


def _as_dtype(mem, dtype):
    from test_gpu_policy_f32 import to32

    return [to32(q) for q in mem] if dtype == "float32" else list(mem)


def _members(spec, obs0, dtype, hidden=(16,), P=4, seed=17):
    """members that really differ: make_policy with seeds seed + m, of `dtype`"""
    return _as_dtype([make_policy(spec, obs0, hidden, seed=seed + m) for m in range(P)], dtype)


def _pop(mem):
    from pcgym_amd import PolicyPopulation

    return PolicyPopulation.from_policies(mem)


def _slices(g, nb=B):
    return [slice(m * g, min(nb, (m + 1) * g)) for m in range((nb + g - 1) // g)]


def _equal(a, b, what, sl=slice(None)):
    torch = _torch()
    for n in NAMES:
        assert torch.equal(a[n][..., sl], b[n][..., sl]), f"{what}: {n}"


# ---- 1. every instantiation against the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", KEYS)
def test_every_instantiation_against_the_oracle(key, dtype):
    torch = _torch()
    from oracle import oracle as O

    tol = _tols(key)
    (env,) = _envs(_params(key), 1, B)
    spec = env.spec
    assert spec.nunc >= 1 and not spec.ncon and spec.integrator == "rk4" and spec.x0_unc is not None
    orc = O.OracleEnv(spec, B, seed=SEED)
    orc.reset()
    p_unc = env.p_unc.cpu().numpy().copy()
    assert np.allclose(p_unc, orc.p_unc, rtol=1e-14, atol=0) and np.std(orc.p_unc, axis=1).min() > 0
    assert np.allclose(env.x.cpu().numpy(), orc.x, rtol=1e-14, atol=0)
    obs0_t = env.obs_soa.clone()
    obs0 = obs0_t.cpu().numpy().copy()
    lo = spec.nobs - spec.nunc
    assert np.std(obs0[lo:], axis=1).min() > 0, "the parameter slots of the reset observation do not vary"
    pop = _pop(_members(spec, obs0, dtype))
    assert pop.P == 4 and pop.dtype == dtype and pop.validate() == 0
    env._lib.pcg_coverage_names(None, 0, 1)
    for c in range(3):
        x_before = env.x.cpu().numpy().copy()
        out = env.rollout_population_unc(pop, 1, G, gamma=0.99, collect_obs=True, collect_rew=True, collect_actions=True)
        torch.cuda.synchronize()
        a = out["a"][0].cpu().numpy()
        assert np.isfinite(a).all()
        orc.x[:] = x_before  # teacher-forced: common start state, the recorded action
        oc, rc, _ = orc.step(a)
        ex = worst_rel(env.x.cpu().numpy(), orc.x)
        o_np, r_np = out["obs"][0].cpu().numpy(), out["rew"][0].cpu().numpy()
        eo = float(np.max(np.abs(o_np - oc) - tol["o_rtol"] * np.abs(oc)))
        print(f"case {key}-{dtype} call {c}: state {ex:.3e} (bar {tol['x1']:.0e}), observation excess over rtol {eo:.3e} "
              f"(atol {tol['o_atol']:.0e}), reward max |diff| {np.max(np.abs(r_np - rc)):.3e} of max |r| {np.max(np.abs(rc)):.3e}")
        assert ex <= tol["x1"], f"call {c}: state {ex:.3e} from the oracle"
        assert np.allclose(o_np, oc, rtol=tol["o_rtol"], atol=tol["o_atol"]), f"call {c}: observation"
        assert _rew_close(r_np, rc), f"call {c}: reward"
        assert torch.equal(out["obs"][0, lo:], obs0_t[lo:]), f"call {c}: the recorded parameter slots are not the reset observation's"
        assert torch.equal(env.obs_soa, out["obs"][0]) and torch.equal(env.rew, out["rew"][0]) and env.t == c + 1
        assert torch.equal(out["ret"], out["rew"][0])  # (one step: J = 0 + 1 * rew)
    names = _launch_names(env._lib)
    assert any(KERNEL[dtype] in n for n in names), f"rollout_population_unc of a {dtype} population launched {names}"
    assert not any(KERNEL["float32" if dtype == "float64" else "float64"] in n for n in names)
    assert torch.equal(env.p_unc.cpu(), torch.as_tensor(p_unc)), "the call wrote io->p_unc"
    assert not env.status.any()
    env.close(), pop.close()


# ---- 2. the networks ------------------------------------------------------------------------------------------------------------
def _with_slot(pol, obs0, slot):
    """`pol` with ONE large first-layer weight of its first hidden unit on `slot`, and that unit reaching the output (the idea of
    test_gpu_unc_rollout._slot_policy): a dropped slot shows in the output"""
    from pcgym_amd import MLPPolicy

    Ws, bs = [w.copy() for w in pol.weights], [b.copy() for b in pol.biases]
    values = obs0[slot]
    spread = float(np.max(values) - np.min(values))
    assert spread > 0
    w = 4.0 / spread  # the slot alone moves the unit's pre-activation by 4 across the batch
    Ws[0][0, slot] = w
    for j in range(Ws[0].shape[1]):
        if j != slot:
            Ws[0][0, j] = 0.0  # (its ONLY large weight: nothing else moves the unit)
    bs[0][0] = -w * float(np.mean(values))
    Ws[1][:, 0] = np.where(Ws[1][:, 0] >= 0, 1.0, -1.0) * max(float(np.max(np.abs(Ws[1]))), 0.1)
    return MLPPolicy(Ws, bs, activation=pol.activation, out_map=pol.out_map, out_low=pol.out_low, out_high=pol.out_high)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hidden", [(16,), (13, 7)], ids=["1x16", "13x7"])
def test_every_action_is_its_own_members(hidden, dtype):
    """members 0 and 3: make_policy; member 1: a first unit that reads the LAST parameter slot alone; member 2: hidden units in
    another order (_perm_hidden); widths 13 x 7 are no multiple of any unroll block"""
    torch = _torch()
    (env,) = _envs(_params("cstr"), 1, B)
    spec = env.spec
    obs0 = env.obs_soa.cpu().numpy().copy()
    slot = spec.nobs - 1
    assert spec.nunc >= 2 and slot >= spec.nobs - spec.nunc
    base = [make_policy(spec, obs0, hidden, seed=17 + m) for m in range(4)]
    mem = _as_dtype([base[0], _with_slot(base[1], obs0, slot), _perm_hidden(base[2], 5), base[3]], dtype)
    pop = _pop(mem)
    if dtype == "float32":
        from test_gpu_policy_f32 import is_f32, tanh32_k
        from test_policy_f32 import bound32 as reference

        k = tanh32_k()
    else:
        reference, k = host_reference, tanh_k()
    # a condition on the INPUTS: without the slot member 1's reference moves by far more than its bound
    sl1 = _slices(G)[1]
    ref0, bound0, _ = reference(mem[1], obs0[:, sl1], k + 1.0)
    dropped = obs0[:, sl1].copy()
    dropped[slot] = 0.0
    gap = np.abs((reference(mem[1], dropped, k + 1.0)[0] - ref0).astype(np.float64))
    assert np.mean(gap > 100 * np.max(bound0)) > 0.25, f"the slot moves the output of {np.mean(gap > 100 * np.max(bound0)):.2f} of slice 1 only"
    out = env.rollout_population_unc(pop, T, G, **KW)
    torch.cuda.synchronize()
    assert _launched(env._lib, KERNEL[dtype])
    a_np, o_np = out["a"].cpu().numpy(), out["obs"].cpu().numpy()
    assert a_np.shape == (T + 1, spec.na, B) and np.isfinite(a_np).all() and np.isfinite(o_np).all()
    if dtype == "float32":
        assert is_f32(a_np), "a recorded output of a float32 member is not a float32 value"
    pre, worst = 0.0, 0.0
    for m, sl in enumerate(_slices(G)):
        for s in range(T + 1):  # (row T: the member on the observation after the last step, recorded and not applied)
            o_in = obs0[:, sl] if s == 0 else o_np[s - 1][:, sl]
            ref, bound, pm = reference(mem[m], o_in, k + 1.0)
            pre = max(pre, pm)
            diff = np.abs(a_np[s][:, sl].astype(LD) - ref).astype(np.float64)
            worst = max(worst, float(np.max(diff / np.maximum(bound, 1e-300))))
            assert np.all(diff <= bound), f"member {m} step {s}: policy output off by {np.max(diff):.3e} (bound {np.max(bound):.3e})"
    print(f"networks {hidden}-{dtype}: worst {worst:.3f} x the running bound, pre-activations up to {pre:.1f}")
    assert pre <= PRE_MAX
    assert torch.equal(env.obs_soa, out["obs"][T - 1])  # row T was evaluated on io->obs as the call leaves it
    assert np.any((a_np > pop.out_low) & (a_np < pop.out_high)), "every output sits on the clip box"
    # slice 1 is member 1's, not member 0's
    ref_other = reference(mem[0], obs0[:, sl1], k + 1.0)[0]
    assert np.any(np.abs(a_np[0][:, sl1].astype(LD) - ref_other).astype(np.float64) > 100 * np.max(bound0))
    env.close(), pop.close()


# ---- 3. a population is its members, bitwise within the kernel --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g", [64, 128])
def test_a_population_is_its_members(g, dtype):
    torch = _torch()
    sls = _slices(g)
    envs = _envs(_params("cstr"), 1 + len(sls), B)
    spec = envs[0].spec
    mem = _members(spec, envs[0].obs_soa.cpu().numpy(), dtype)
    pop = _pop(mem)
    mixed = envs[0].rollout_population_unc(pop, T, g, gamma=0.99, **KW)
    assert _launched(envs[0]._lib, KERNEL[dtype])
    for m, sl in enumerate(sls):
        same = _pop([mem[m]] * 4)
        got = envs[1 + m].rollout_population_unc(same, T, g, gamma=0.99, **KW)
        torch.cuda.synchronize()
        _equal(got, mixed, f"four copies of member {m}, G = {g}", sl)
        assert torch.equal(envs[1 + m].x[..., sl], envs[0].x[..., sl]) and torch.equal(envs[1 + m].obs_soa[..., sl], envs[0].obs_soa[..., sl])
        if m == 0:  # (the members really differ: slice 1 is not what member 0 does there)
            assert not torch.equal(got["a"][..., sls[1]], mixed["a"][..., sls[1]])
        same.close()
    for e in envs:
        e.close()
    pop.close()


# ---- 4. against rollout_policy_unc with pop.member(m), to rounding ----------------------------------------------------------------
@pytest.mark.parametrize("key", ["cstr", "multistage_extraction^1.5"])
def test_against_rollout_policy_unc_member_by_member(key):
    torch = _torch()
    tol = _tols(key)
    sls = _slices(G)
    envs = _envs(_params(key), 1 + len(sls), B)
    spec = envs[0].spec
    pop = _pop(_members(spec, envs[0].obs_soa.cpu().numpy(), "float64"))
    got = envs[0].rollout_population_unc(pop, T, G, **KW)
    torch.cuda.synchronize()
    for m, sl in enumerate(sls):
        one = pop.member(m)
        a, o, r = envs[1 + m].rollout_policy_unc(one, T, collect_obs=True, record_next_action=True)
        torch.cuda.synchronize()
        eo = max(worst_rel(got["obs"][s][:, sl].cpu().numpy(), o[s][:, sl].cpu().numpy()) for s in range(T))
        ea = worst_rel(got["a"].permute(1, 0, 2)[..., sl].reshape(spec.na, -1).cpu().numpy(), a.permute(1, 0, 2)[..., sl].reshape(spec.na, -1).cpu().numpy())
        dr = float((got["rew"][:, sl] - r[:, sl]).abs().max())
        bits = bool(torch.equal(got["obs"][..., sl], o[..., sl]))
        print(f"case {key} member {m}: observation {eo:.3e}, action {ea:.3e} from rollout_policy_unc (bar {tol['xT']:.0e}), reward max |diff| "
              f"{dr:.3e}; equal bits: {bits}")
        assert eo <= tol["xT"], f"member {m}: observation {eo:.3e} from rollout_policy_unc"
        assert _rew_close(got["rew"][:, sl].cpu().numpy(), r[:, sl].cpu().numpy()), f"member {m}: reward"
        assert worst_rel(envs[0].x[:, sl].cpu().numpy(), envs[1 + m].x[:, sl].cpu().numpy()) <= tol["xT"]
        one.close()
    assert _launched(envs[0]._lib, KERNEL["float64"]) and _launched(envs[0]._lib, "rollout_unc_policy_kernel")
    for e in envs:
        e.close()
    pop.close()


# ---- 5. one call equals chunked calls; the returns -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("gamma", [1.0, 0.99])
def test_one_call_equals_chunked_calls_and_the_returns(gamma, dtype):
    torch = _torch()
    ea, eb, ec, er = _envs(_params("cstr"), 4, B)
    spec = ea.spec
    obs0 = ea.obs_soa.clone()
    pop = _pop(_members(spec, obs0.cpu().numpy(), dtype))
    one = ea.rollout_population_unc(pop, T, G, gamma=gamma, **KW)
    torch.cuda.synchronize()
    assert float(one["rew"].std()) > 0 and bool(torch.isfinite(one["ret"]).all()) and not ea.status.any()
    assert torch.equal(one["ret"], _returns(one["rew"], gamma)), f"ret is not the recurrence over the recorded rewards (gamma = {gamma})"
    if gamma != 1.0:
        assert not torch.equal(one["ret"], _returns(one["rew"], 1.0))
    for env, chunks in ((eb, (1, 2, 3)), (ec, (3, 3))):
        parts, done = [], 0
        for n in chunks:
            assert env.t == done
            parts.append(env.rollout_population_unc(pop, n, G, gamma=gamma, **dict(KW, record_next_action=(done + n == T))))
            torch.cuda.synchronize()
            # each chunk returns the return of its own steps, discounted from its first
            assert torch.equal(parts[-1]["ret"], _returns(one["rew"][done:done + n], gamma)), f"chunks {chunks}: ret of the chunk at {done}"
            done += n
        for k in ("a", "obs", "rew"):
            assert torch.equal(torch.cat([q[k] for q in parts]), one[k]), f"chunks {chunks}: {k}"
        _final_equal(env, ea)
    # nothing else recorded: the same returns
    only = er.rollout_population_unc(pop, T, G, gamma=gamma)
    torch.cuda.synchronize()
    assert only["a"] is None and only["obs"] is None and only["rew"] is None
    assert torch.equal(only["ret"], one["ret"]) and torch.equal(er.x, ea.x)
    # the parameter slots of every recorded row are the reset observation's, bit for bit
    lo = spec.nobs - spec.nunc
    for s in range(T):
        assert torch.equal(one["obs"][s, lo:], obs0[lo:]), f"step {s}: the recorded parameter slots"
    assert _launched(ea._lib, KERNEL[dtype])
    for e in (ea, eb, ec, er):
        e.close()
    pop.close()


# ---- 6. shards -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_shards_split_members_and_parameters_by_the_global_env_index(dtype):
    torch = _torch()
    p = _params("cstr")
    whole = _make(p, B, seed=SEED)
    parts = [_make(p, nb, seed=SEED, env_offset=off) for off, nb in ((0, 128), (128, B - 128))]
    for e in [whole] + parts:
        e.reset()
    assert torch.equal(torch.cat([e.x for e in parts], dim=1), whole.x) and torch.equal(torch.cat([e.p_unc for e in parts], dim=1), whole.p_unc)
    assert float(whole.p_unc.std(dim=1).min()) > 0
    pop = _pop(_members(whole.spec, whole.obs_soa.cpu().numpy(), dtype))
    w = whole.rollout_population_unc(pop, T, G, gamma=0.99, **KW)
    ps = [e.rollout_population_unc(pop, T, G, gamma=0.99, **KW) for e in parts]
    torch.cuda.synchronize()
    for n in NAMES:
        assert torch.equal(torch.cat([q[n] for q in ps], dim=-1), w[n]), n
    assert torch.equal(torch.cat([e.x for e in parts], dim=1), whole.x)
    assert torch.equal(torch.cat([e.obs_soa for e in parts], dim=1), whole.obs_soa)
    # the second shard is driven by members 2 and 3: not what members 0 and 1 do on the same envs
    alone = _make(p, B - 128, seed=SEED, env_offset=128)
    alone.reset()
    alone._lib.pcg_plan_set_env_offset(alone._plan, 0)  # (members 0 and 1; the reset above drew the shard's own states and parameters)
    other = alone.rollout_population_unc(pop, 1, G, collect_actions=True)
    torch.cuda.synchronize()
    assert not torch.equal(other["a"][0], ps[1]["a"][0])
    for e in [whole, alone] + parts:
        e.close()
    pop.close()


# ---- 7. update_ / set_flat_ ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_rewriting_one_member_changes_its_slice_and_no_other(dtype):
    torch = _torch()
    envs = _envs(_params("cstr"), 4, B)
    spec = envs[0].spec
    obs0 = envs[0].obs_soa.cpu().numpy()
    mem = _members(spec, obs0, dtype)
    pop = _pop(mem)
    before = envs[0].rollout_population_unc(pop, T, G, gamma=0.99, **KW)
    h = pop.handle(envs[0].device)
    theta2 = pop.flat(first=2, count=1).clone()  # (member 2 as it is now, on the device)
    (new,) = _as_dtype([make_policy(spec, obs0, (16,), seed=99)], dtype)
    pop.update_([w[None] for w in new.weights], [b[None] for b in new.biases], first=2)
    assert pop.handle(envs[0].device) is h  # the same device object, rewritten
    after = envs[1].rollout_population_unc(pop, T, G, gamma=0.99, **KW)
    fresh = _pop(mem[:2] + [new] + mem[3:])
    want = envs[2].rollout_population_unc(fresh, T, G, gamma=0.99, **KW)
    torch.cuda.synchronize()
    two = _slices(G)[2]
    keep = torch.ones(B, dtype=torch.bool, device=envs[0].device)
    keep[two] = False
    _equal(after, want, "after update_ against a fresh population")
    for n in NAMES:
        assert not torch.equal(after[n][..., two], before[n][..., two]), f"{n}: slice 2 did not change"
        assert torch.equal(after[n][..., keep], before[n][..., keep]), f"{n}: another slice's bits changed"
    # set_flat_ writes member 2 back on the device: every bit of the first run returns
    pop.set_flat_(theta2, first=2)
    back = envs[3].rollout_population_unc(pop, T, G, gamma=0.99, **KW)
    torch.cuda.synchronize()
    _equal(back, before, "after set_flat_ of the old member 2")
    for n in NAMES:
        assert not torch.equal(back[n][..., two], after[n][..., two]), f"{n}: set_flat_ did not change slice 2"
    for e in envs:
        e.close()
    pop.close(), fresh.close()


# ---- 8. the public path ------------------------------------------------------------------------------------------------------------
class _Replay:
    """the callable form of a population that replays recorded actions: what evaluate_population's per-step route calls"""

    def __init__(self, pop, a_seq):
        self.n_in, self.n_out, self.P, self.a_seq, self.calls = pop.n_in, pop.n_out, pop.P, a_seq, 0

    def __call__(self, obs, envs_per_policy, env_offset=0):
        self.calls += 1
        return self.a_seq[self.calls - 1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_evaluate_population_takes_the_fused_call(dtype):
    torch = _torch()
    from pcgym_amd import evaluate_population
    from test_gpu_actor_rollout import make_ac

    Bn = 256
    ef, es, er = _envs(_params("cstr"), 3, Bn)  # (evaluate_population resets again: the envs stay in the same RNG epoch)
    spec = ef.spec
    N, tol = spec.N, _tols("cstr")
    obs0 = ef.obs_soa.cpu().numpy()
    # (make_ac's actor: its mean at the mean reset observation is the middle of the action box, which keeps every reactor of
    # this episode away from thermal runaway -- a state that is not finite compares with nothing: test_gpu_unc_rollout.py)
    acs = [make_ac(spec, obs0, (16,), seed=23 + m, sigma_scale=0.1) for m in range(4)]
    pop = _pop(_as_dtype([ac.actor for ac in acs], dtype))
    ef._lib.pcg_coverage_names(None, 0, 1)
    fused = evaluate_population(ef, pop, G, gamma=0.99, fused_unc=True)
    torch.cuda.synchronize()
    names = _launch_names(ef._lib)
    assert any(KERNEL[dtype] in n for n in names), f"evaluate_population(fused_unc=True) launched {names}"
    assert ef.t == N - 1 and fused["ret"].shape == (Bn,) and fused["score"].shape == (Bn // G,)
    assert bool(torch.isfinite(fused["ret"]).all()) and not ef.status.any()
    assert torch.equal(fused["score"], fused["ret"].view(-1, G).mean(dim=1)) and float(fused["score"].std()) > 0
    # the per-step route, teacher-forced: torch and the kernel round the networks differently, so the callable replays the
    # policy outputs the same kernel records (the networks themselves: test_every_action_is_its_own_members)
    er.reset()
    rec = er.rollout_population_unc(pop, N - 1, G, gamma=0.99, collect_actions=True)
    torch.cuda.synchronize()
    assert torch.equal(rec["ret"], fused["ret"])
    replay = _Replay(pop, rec["a"])
    es._lib.pcg_coverage_names(None, 0, 1)
    ref = evaluate_population(es, replay, G, gamma=0.99, fused=False)
    torch.cuda.synchronize()
    assert replay.calls == N - 1 and not any("rollout_pop" in n for n in _launch_names(es._lib))
    d = worst_rel(fused["ret"][None].cpu().numpy(), ref["ret"][None].cpu().numpy())
    ds = worst_rel(fused["score"][None].cpu().numpy(), ref["score"][None].cpu().numpy())
    print(f"evaluate_population {dtype} B={Bn} G={G} N={N}: ret {d:.3e}, score {ds:.3e} from the per-step route (bar {tol['xT']:.0e})")
    assert d <= tol["xT"] and ds <= tol["xT"]
    assert worst_rel(ef.x.cpu().numpy(), es.x.cpu().numpy()) <= tol["xT"]
    # what is refused: the slice size, the two switches against each other; the default route on such a plan steps
    for kw in (dict(envs_per_policy=96, fused_unc=True), dict(envs_per_policy=G, fused_unc=True, fused=False), dict(envs_per_policy=G, fused=True)):
        with pytest.raises(ValueError):
            evaluate_population(er, pop, kw.pop("envs_per_policy"), **kw)
    for e in (ef, es, er):
        e.close()
    pop.close()
    for ac in acs:
        ac.close()


# ---- 9. refusals, in the documented order -----------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_write_nothing():
    torch = _torch()
    from pcgym_amd import _abi as abi
    from pcgym_amd.models import get_model

    Bn, Tn = 256, 2
    OK, UNS, DIM, VAL, NUL, PLAN = abi.PCG_OK, abi.PCG_E_UNSUPPORTED, abi.PCG_E_DIM, abi.PCG_E_VALUE, abi.PCG_E_NULL, abi.PCG_E_PLAN

    class Case:
        def __init__(self, p, members=4, **kw):
            self.env = env = _make(p, Bn, seed=2, **kw)
            env.reset()
            s = self.spec = env.spec
            self.pop = self.population(members)
            shapes = {"a": (Tn + 1, s.na, Bn), "obs": (Tn, s.nobs, Bn), "rew": (Tn, Bn), "ret": (Bn,)}
            # guard cells around every output: one row more on either side, which no call may touch
            self.guard = {n: torch.full((3,) + shp, -7.0, dtype=torch.float64, device=env.device) for n, shp in shapes.items()}
            self.bufs = {n: g[1] for n, g in self.guard.items()}
            self.x0, self.o0 = env.x.clone(), env.obs_soa.clone()
            self.pu = env.p_unc.clone() if env.p_unc is not None else None
            torch.cuda.synchronize()
            env._lib.pcg_coverage_names(None, 0, 1)

        def population(self, members, n_in=None, dtype="float64"):
            from pcgym_amd import MLPPolicy

            s, rng = self.spec, np.random.default_rng(3)
            n_in = s.nobs if n_in is None else n_in
            return _pop([MLPPolicy([rng.standard_normal((16, n_in)) / 4, rng.standard_normal((s.na, 16)) / 4], [np.zeros(16), np.zeros(s.na)],
                                   dtype=dtype) for _ in range(members)])

        def call(self, pop=None, g=64, gamma=0.99, T=Tn, buf=None, fn="pcg_rollout_policy_pop_unc", handle=False):
            env, s, b = self.env, self.spec, self.bufs
            h = pop if handle else (pop or self.pop).handle(env.device)
            rc = getattr(env._lib, fn)(env._plan, env._bufp if buf is None else C.byref(buf), h, g, 0, T, b["a"].data_ptr(),
                                       s.na * Bn, Bn, b["obs"].data_ptr(), s.nobs * Bn, Bn, b["rew"].data_ptr(), Bn, 1,
                                       gamma, b["ret"].data_ptr(), 1, None)
            torch.cuda.synchronize()
            return rc

        def refused(self, what, want, **kw):
            rc = self.call(**kw)
            assert rc == want, f"{what}: status {rc}, not {want}"
            names = _launch_names(self.env._lib, reset=True)
            assert not names, f"{what}: a refused call launched or compiled {names}"
            assert torch.equal(self.env.x, self.x0) and torch.equal(self.env.obs_soa, self.o0), f"{what}: a refused call wrote the env"
            assert self.pu is None or torch.equal(self.env.p_unc, self.pu), f"{what}: a refused call wrote io->p_unc"
            assert all(bool((g == -7.0).all()) for g in self.guard.values()), f"{what}: a refused call wrote an output buffer or a guard cell"

        def close(self):
            self.env.close(), self.pop.close()

    unc = _params("cstr")
    ok = Case(unc)
    assert ok.spec.nunc >= 1
    # ---- positive control: the valid call runs, writes every buffer and no guard cell, and is seen by the launch record ----
    for dtype in DTYPES:
        q = ok.population(4, dtype=dtype)
        assert ok.call(pop=q) == OK
        assert any(KERNEL[dtype] in n for n in _launch_names(ok.env._lib, reset=True)), f"the valid {dtype} call launched nothing"
        assert not torch.equal(ok.env.x, ok.x0) and all(bool((b != -7.0).all()) for b in ok.bufs.values())
        assert all(bool((g[0] == -7.0).all()) and bool((g[2] == -7.0).all()) for g in ok.guard.values()), "the valid call wrote a guard cell"
        assert torch.equal(ok.env.p_unc, ok.pu)
        ok.env.x.copy_(ok.x0), ok.env.obs_soa.copy_(ok.o0)
        for b in ok.bufs.values():
            b.fill_(-7.0)
        torch.cuda.synchronize()
        q.close()

    # ---- 1. plan, buffers and handle ----
    ok.refused("a null population", NUL, pop=None, handle=True)
    ok.refused("what is not a population", PLAN, pop=C.cast(C.create_string_buffer(512), C.c_void_p), handle=True)
    # ---- 2. the plans: PCG_E_UNSUPPORTED, before the sizes and the slices ----
    plain = copy.deepcopy(SC.scenarios()["cstr_canonical"]["env_params"])
    plain.update(integrator="rk4")
    both = copy.deepcopy(SC.scenarios()["cstr_cons_pen_norm"]["env_params"])
    both.update(integrator="rk4", uncertainty_percentages={"q": 0.03}, distribution="uniform",
                uncertainty_bounds={"low": np.array([90.0]), "high": np.array([110.0])})
    cv8 = dict(plain, integrator="cv8")  # (cv8 refuses per-env parameters when the plan is made: such a plan has none)
    dopri = copy.deepcopy(unc)
    dopri.update(integrator="dopri5", rtol=1e-6, atol=1e-8)
    affine = next(k for k in MODEL_KEYS if get_model(k.partition("^")[0]).affine_builder is not None)
    plans = {"no parameters": (plain, {}), "rows": (both, {}), "cv8": (cv8, {}), "dopri5": (dopri, {}), "per-env counters": (unc, dict(per_env_t=True)),
             "an affine registry model": (sweep_params(affine, "rk4", "lean"), {})}
    cases = {n: Case(p, **kw) for n, (p, kw) in plans.items()}
    assert not cases["no parameters"].spec.nunc and cases["rows"].spec.nunc and cases["rows"].spec.ncon and cases["dopri5"].spec.nunc
    for n, c in cases.items():
        c.refused(n, UNS)
        c.refused(n + ", members of another size", UNS, pop=c.population(4, n_in=c.spec.nobs + 1))  # the plan before the sizes
        c.refused(n + ", envs_per_policy = 96", UNS, g=96)                                          # the plan before the slices
    # ---- 3. the members' sizes, before the slices ----
    wrong = ok.population(4, n_in=ok.spec.nobs - ok.spec.nunc)  # (the observation without its parameter slots)
    ok.refused("members that forget the parameter slots", DIM, pop=wrong)
    ok.refused("members of another size and envs_per_policy = 96", DIM, pop=wrong, g=96)
    # ---- 4. the slices and gamma, before the buffers ----
    nop = abi.pcg_buffers.from_buffer_copy(ok.env._buf)
    nop.p_unc = None
    ok.refused("envs_per_policy = 96", VAL, g=96)
    ok.refused("envs_per_policy = 0", VAL, g=0)
    shifted = Case(unc, env_offset=32, members=5)
    shifted.refused("env offset 32", VAL)
    small = ok.population(3)
    ok.refused("three members for four slices", DIM, pop=small)
    ok.refused("gamma = 1.5", VAL, gamma=1.5)
    ok.refused("gamma = nan", VAL, gamma=float("nan"))
    ok.refused("gamma = 1.5 and io->p_unc == NULL", VAL, gamma=1.5, buf=nop)
    ok.refused("three members and io->p_unc == NULL", DIM, pop=small, buf=nop)
    # ---- 5. closed_loop_launch's checks ----
    ok.refused("T = 0", VAL, T=0)
    ok.refused("T = 0 and io->p_unc == NULL", VAL, T=0, buf=nop)
    ok.refused("io->p_unc == NULL", NUL, buf=nop)
    nor = abi.pcg_buffers.from_buffer_copy(ok.env._buf)
    nor.rew = None
    ok.refused("io->rew == NULL", NUL, buf=nor)
    # ---- pcg_rollout_policy_pop keeps refusing the plan ----
    ok.refused("pcg_rollout_policy_pop on the parameter plan", UNS, fn="pcg_rollout_policy_pop")
    for dtype in DTYPES:
        q = ok.population(4, dtype=dtype)
        ok.refused(f"pcg_rollout_policy_pop on the parameter plan, {dtype}", UNS, fn="pcg_rollout_policy_pop", pop=q)
        q.close()
    for c in [ok, shifted] + list(cases.values()):
        c.close()
    small.close(), wrong.close()


# ---- 10. stream capture --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_stream_capture_replays_the_eager_call(dtype):
    torch = _torch()
    (env,) = _envs(_params("cstr"), 1, B)
    spec = env.spec
    pop = _pop(_members(spec, env.obs_soa.cpu().numpy(), dtype, seed=29))
    h = pop.handle(env.device)
    x0, o0, pu = env.x.clone(), env.obs_soa.clone(), env.p_unc.clone()
    f64, dev = torch.float64, env.device
    a_seq = torch.zeros((T + 1, spec.na, B), dtype=f64, device=dev)
    o_seq = torch.zeros((T, spec.nobs, B), dtype=f64, device=dev)
    r_seq = torch.zeros((T, B), dtype=f64, device=dev)
    ret = torch.zeros(B, dtype=f64, device=dev)
    seed = env._episode_seed()

    def call(stream):
        return env._lib.pcg_rollout_policy_pop_unc(env._plan, env._bufp, h, G, 0, T, a_seq.data_ptr(), spec.na * B, B, o_seq.data_ptr(),
                                                   spec.nobs * B, B, r_seq.data_ptr(), B, 1, 0.99, ret.data_ptr(), seed, stream)

    assert call(torch.cuda.current_stream(dev).cuda_stream) == 0
    torch.cuda.synchronize()
    assert _launched(env._lib, KERNEL[dtype])
    outs = (a_seq, o_seq, r_seq, ret, env.x, env.obs_soa, env.rew, env.done)
    eager = [t.clone() for t in outs]
    assert float(a_seq.std()) > 0 and torch.equal(ret, _returns(r_seq, 0.99))
    gr = torch.cuda.CUDAGraph()
    env.x.copy_(x0), env.obs_soa.copy_(o0)
    torch.cuda.synchronize()
    with torch.cuda.graph(gr):  # (one call: a single branch)
        rc = call(torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    for rep in range(2):
        for t in (a_seq, o_seq, r_seq, ret):
            t.fill_(-3.0)
        env.x.copy_(x0), env.obs_soa.copy_(o0)  # re-seed the state
        gr.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, eager):
            assert torch.equal(got, want), f"replay {rep} differs from the eager call"
    assert torch.equal(env.p_unc, pu)
    env.close(), pop.close()
