"""The fused closed-loop rollout of a POPULATION of MLP policies (pcg_rollout_policy_pop, pcg_rollout_pop.hpp): every slice of
`envs_per_policy` consecutive envs driven by its own member, one launch.

  every instantiation  each model x {RK4, CV8}: test_gpu_policy_rollout's three teacher-forced checks, group by group -- the
                       recorded actions against the member evaluated on the host in np.longdouble inside its running bound,
                       the recorded actions replayed through the open-loop rollout BITWISE, one call per step bitwise the one
                       call and every step against the oracle;
  members              a population is its members: P copies of one policy give rollout_policy's bits, distinct members give,
                       slice by slice, the bits of rollout_policy with that member on the full batch;
  returns              ret_out against the stated recurrence in torch, bit for bit; with nothing else recorded; per chunk;
  shards               two envs with env offsets against the one env that holds both;
  update               update_ of one member changes that member's group and no other bit;
  public path          evaluate_population fused against the step loop with the callable form;
  refusals             every refused call returns its status, launches nothing and writes nothing;
  stream capture       one call inside torch.cuda.graph, replayed twice, equal to the eager call.
"""
import copy

import numpy as np
import pytest

import scenarios as SC
from helpers import (CASE_KEYS, LD, PRE_MAX, SHAPES, UNSUPPORTED_PLANS, _case_params, _launch_names, _launched, _make, _perm_hidden,
                     _spread_x0, _torch, host_reference, make_policy, tanh_k)

pytestmark = pytest.mark.gpu

B, T, G = 200, 6, 64  # three full waves and a wave of 8 lanes: four members


def _population(spec, obs0, hidden, P, seed=17):
    """members that really differ: make_policy with seeds seed + m"""
    from pcgym_amd import PolicyPopulation

    mem = [make_policy(spec, obs0, hidden, seed=seed + m) for m in range(P)]
    return PolicyPopulation.from_policies(mem), mem


# Where the members' outputs sit in the action box, for the comparison with the oracle: (centre in half widths from the middle
# of the box, scale of the output layer).  (0, 1) is make_policy's own output layer; the others move it into a part of the box.
# A case takes the first entry under which the ORACLE itself is well conditioned along the case's closed loop (test_gpu_actor_
# rollout's rule and bar: a 1e-15 perturbation of a step's start state grows at most 100-fold, so that round-off stays two
# orders below the 1e-12 bar) -- chosen on the host from the oracle alone, before any kernel runs.  An explicit step whose
# stages leave the model's physical range amplifies round-off by many orders of magnitude; no two correct implementations
# agree to 1e-12 there (the biofilm reactor under cv8 over most of its action box).
REMAPS = [(0.0, 1.0), (-0.5, 0.25), (0.5, 0.25), (-0.9, 0.1), (0.9, 0.1)]


def _remapped(spec, pol, centre, scale):
    from pcgym_amd import MLPPolicy
    from test_gpu_actor_rollout import action_box

    if (centre, scale) == (0.0, 1.0):
        return pol
    lo, hi = action_box(spec)
    mid, half = (hi + lo) / 2, (hi - lo) / 2
    Ws, bs = [w.copy() for w in pol.weights], [b.copy() for b in pol.biases]
    Ws[-1], bs[-1] = scale * Ws[-1], mid + centre * half + scale * (bs[-1] - mid)
    return MLPPolicy(Ws, bs, activation=pol.activation, out_map=pol.out_map, out_low=pol.out_low, out_high=pol.out_high)


def _oracle_conditioning(spec, mem, g, Bn, Tn, env_seed):
    """host_conditioning (test_gpu_actor_rollout) for a population of deterministic members: the oracle's own sensitivity along
    the closed loop in which slice m is driven by mem[m], evaluated in fp64 numpy"""
    from oracle import oracle as O
    from test_gpu_actor_rollout import _np_raw

    o1, o2 = (O.OracleEnv(spec, Bn, seed=env_seed) for _ in range(2))
    o1.reset(), o2.reset()
    rng = np.random.default_rng(0)
    obs, worst = o1.obs.copy(), 0.0
    for s in range(Tn):
        a = np.concatenate([np.clip(_np_raw(q, obs[:, m * g:(m + 1) * g]), q.out_low, q.out_high) for m, q in enumerate(mem)], axis=1)
        o2.x[:] = o1.x * (1 + 1e-15 * rng.standard_normal(o1.x.shape))
        obs = o1.step(a)[0].copy()
        o2.step(a)
        if not (np.isfinite(o1.x).all() and np.isfinite(o2.x).all()):
            return float("inf")
        worst = max(worst, float(np.max(np.abs(o1.x - o2.x) / np.maximum(np.abs(o1.x), 1.0))))
    return worst


def _pick_members(spec, obs0, hidden, P, g, Bn, Tn, env_seed, seed=17):
    """make_policy with seeds seed + m, output layers placed by the first entry of REMAPS the oracle is well conditioned under"""
    from test_gpu_actor_rollout import WELL_CONDITIONED

    tried = []
    for centre, scale in REMAPS:
        mem = [_remapped(spec, make_policy(spec, obs0, hidden, seed=seed + m), centre, scale) for m in range(P)]
        amp = _oracle_conditioning(spec, mem, g, Bn, Tn, env_seed)
        tried.append((centre, scale, amp))
        if amp <= WELL_CONDITIONED:
            return mem, (centre, scale, amp)
    raise AssertionError(f"the oracle is well conditioned under no entry of REMAPS: {tried}")


def _plan(scen, integ, **over):
    p = copy.deepcopy(SC.scenarios()[scen]["env_params"])
    p.update(integrator=integ, **over)
    return p


@pytest.mark.parametrize("integ", ["rk4", "cv8"])
@pytest.mark.parametrize("key", CASE_KEYS)
def test_population_rollout(key, integ):
    torch = _torch()
    from oracle import oracle as O

    p = _spread_x0(_case_params(key, integ))
    e_one, e_chain = (_make(p, B, seed=9) for _ in range(2))
    e_open = _make(p, B, seed=9, variant=1)  # PCG_OPT_VARIANT 1: the general kernels
    spec = e_one.spec
    assert spec.integrator == integ and not spec.ncon and not spec.nunc and spec.x0_unc is not None
    for e in (e_one, e_chain, e_open):
        e.reset()
    obs0 = e_one.obs_soa.cpu().numpy().copy()
    x0 = e_one.x.cpu().numpy().copy()
    P = (B + G - 1) // G
    from pcgym_amd import PolicyPopulation

    mem, (centre, scale, amp) = _pick_members(spec, obs0, SHAPES["1x16"], P, G, B, T, env_seed=9)
    print(f"case {key}-{integ}: output layers at {centre:+.2f} half widths x {scale:.2f}, oracle amplification of 1e-15: {amp:.2e}")
    pop = PolicyPopulation.from_policies(mem)
    assert P == 4 and pop.validate() == 0
    k = tanh_k()
    e_one._lib.pcg_coverage_names(None, 0, 1)

    # ---- the fused closed loop: one call ----
    out = e_one.rollout_population(pop, T, G, gamma=0.99, collect_obs=True, collect_rew=True, collect_actions=True, record_next_action=True)
    torch.cuda.synchronize()
    assert _launched(e_one._lib, "rollout_pop_policy_kernel"), "rollout_population did not launch the population kernel"
    a_seq, obs_seq, rew_seq = out["a"], out["obs"], out["rew"]
    a_np, o_np = a_seq.cpu().numpy(), obs_seq.cpu().numpy()
    assert a_np.shape == (T + 1, spec.na, B) and o_np.shape == (T, spec.nobs, B) and out["ret"].shape == (B,)
    assert np.isfinite(a_np).all() and np.isfinite(o_np).all() and not e_one.status.any()
    assert torch.equal(e_one.obs_soa, obs_seq[T - 1]) and torch.equal(e_one.rew, rew_seq[T - 1])  # io-> hold the last step
    assert e_one.t == T

    # ---- 1. action check, per group: recorded a[s] against member m on the host, on the kernel's own obs[s-1] ----
    pre = 0.0
    for m in range(P):
        sl = slice(m * G, min(B, (m + 1) * G))
        for s in range(T + 1):
            o_in = obs0[:, sl] if s == 0 else o_np[s - 1][:, sl]
            ref, bound, pm = host_reference(mem[m], o_in, k + 1.0)
            pre = max(pre, pm)
            diff = np.abs(a_np[s][:, sl].astype(LD) - ref).astype(np.float64)
            assert np.all(diff <= bound), (f"member {m} step {s}: policy output off by {np.max(diff):.3e}, "
                                           f"{np.max(diff / np.maximum(bound, 1e-300)):.2f} x the running bound ({np.max(bound):.3e})")
    assert pre <= PRE_MAX, f"pre-activations up to {pre:.1f}: outside the grid the tanh error was measured on"
    assert np.std(a_np) > 0
    # the groups are driven by different members: group 1's first actions are not member 0's on group 1's observations
    o1 = torch.as_tensor(obs0[:, G:2 * G].T.copy())
    assert not np.array_equal(a_np[..., :G], a_np[..., G:2 * G])
    assert not np.array_equal(mem[0](o1).numpy().T, a_np[0][:, G:2 * G])

    # ---- 2. dynamics check: the recorded actions through the open-loop rollout, general kernel: bitwise ----
    assert np.array_equal(e_open.x.cpu().numpy(), x0)
    oq, rq = e_open.rollout(a_seq[:T].contiguous(), collect_obs=True, collect_rew=True)
    torch.cuda.synchronize()
    assert torch.equal(oq, obs_seq), "observations differ from the open-loop replay of the recorded actions"
    assert torch.equal(rq, rew_seq), "rewards differ from the open-loop replay"
    assert torch.equal(e_open.x, e_one.x), "final state differs from the open-loop replay"
    assert torch.equal(e_open.done, e_one.done) and torch.equal(e_open.status, e_one.status)
    if spec.a_delta:
        assert torch.equal(e_open.a_save_t, e_one.a_save_t)

    # ---- 3. oracle check: one call per step == the one call, bitwise; every step against the oracle, every lane ----
    orc = O.OracleEnv(spec, B, seed=9)
    orc.reset()
    assert np.allclose(orc.x, x0, rtol=1e-14, atol=0)
    for s in range(T):
        x_before = e_chain.x.cpu().numpy().copy()
        c1 = e_chain.rollout_population(pop, 1, G, collect_obs=True, collect_rew=True, collect_actions=True, record_next_action=(s == T - 1))
        torch.cuda.synchronize()
        assert torch.equal(c1["a"][0], a_seq[s]) and torch.equal(c1["obs"][0], obs_seq[s]) and torch.equal(c1["rew"][0], rew_seq[s]), f"chained call {s}"
        assert torch.equal(c1["ret"], rew_seq[s])  # (one step: J = 0 + 1 * rew)
        if s == T - 1:
            assert torch.equal(c1["a"][1], a_seq[T])
        orc.x[:] = x_before  # teacher-forced: common start state, the recorded action
        oc, rc, dc = orc.step(a_np[s])
        xg = e_chain.x.cpu().numpy()
        assert np.isfinite(orc.x).all()
        err = float(np.max(np.abs(xg - orc.x) / np.maximum(np.abs(orc.x), 1.0)))
        assert err <= 1e-12, f"step {s}: state {err:.3e} from the oracle (relative to max(|x|, 1))"
        assert np.array_equal(e_chain.done.cpu().numpy(), dc)
        if not spec.noise:  # (with noise the observation carries the noise twin's fp32 variates: compared through x and the reward)
            assert np.allclose(c1["obs"][0].cpu().numpy(), oc, rtol=1e-10, atol=1e-11)
        assert np.allclose(c1["rew"][0].cpu().numpy(), rc, rtol=1e-9, atol=1e-10 * (1 + np.max(np.abs(rc))))
    assert torch.equal(e_chain.x, e_one.x)
    for e in (e_one, e_chain, e_open):
        e.close()
    pop.close()


@pytest.mark.parametrize("g", [64, 128])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("scen,integ", [("cstr_canonical", "rk4"), ("four_tank_canonical", "cv8")])
def test_a_population_is_its_members(scen, integ, shape, g):
    """both kernels execute the same policy_eval (explicit FMAs) and the same env_step: bits, not tolerances"""
    torch = _torch()
    from pcgym_amd import PolicyPopulation

    p = _spread_x0(_plan(scen, integ))
    P = (B + g - 1) // g
    envs = [_make(p, B, seed=9) for _ in range(3 + P)]
    for e in envs:
        e.reset()
    spec = envs[0].spec
    obs0 = envs[0].obs_soa.cpu().numpy().copy()
    pop, mem = _population(spec, obs0, SHAPES[shape], P)
    kw = dict(collect_obs=True, collect_rew=True, collect_actions=True, record_next_action=True)

    # P copies of one policy: rollout_policy's bits
    same = PolicyPopulation.from_policies([mem[0]] * P)
    got = envs[0].rollout_population(same, T, g, **kw)
    a, o, r = envs[1].rollout_policy(mem[0], T, **kw)
    torch.cuda.synchronize()
    assert torch.equal(got["a"], a) and torch.equal(got["obs"], o) and torch.equal(got["rew"], r)
    assert torch.equal(envs[0].x, envs[1].x) and torch.equal(envs[0].obs_soa, envs[1].obs_soa) and torch.equal(envs[0].done, envs[1].done)

    # distinct members: group m's slice is rollout_policy with member(m) on an identical full-batch env
    got = envs[2].rollout_population(pop, T, g, **kw)
    for m in range(P):
        sl = slice(m * g, min(B, (m + 1) * g))
        em = envs[3 + m]
        a, o, r = em.rollout_policy(pop.member(m), T, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got["a"][..., sl], a[..., sl]), f"member {m}: actions"
        assert torch.equal(got["obs"][..., sl], o[..., sl]) and torch.equal(got["rew"][..., sl], r[..., sl]), f"member {m}"
        assert torch.equal(envs[2].x[..., sl], em.x[..., sl]), f"member {m}: final state"
        if m == 0:
            a_first = a
    # (the members really differ: group 1 is not what member 0 does on group 1's envs)
    assert not torch.equal(got["a"][..., g:2 * g], a_first[..., g:2 * g])
    for e in envs:
        e.close()
    pop.close(), same.close()


def _returns(rew, gamma):
    """the kernel's recurrence in torch: every operation rounded on its own"""
    torch = _torch()
    J, disc = torch.zeros_like(rew[0]), 1.0
    for s in range(rew.shape[0]):
        J = J + disc * rew[s]
        disc = disc * gamma
    return J


@pytest.mark.parametrize("gamma", [1.0, 0.99])
def test_returns(gamma):
    torch = _torch()
    p = _spread_x0(_plan("cstr_canonical", "rk4"))
    e_all, e_ret, e_chunk = (_make(p, B, seed=9) for _ in range(3))
    for e in (e_all, e_ret, e_chunk):
        e.reset()
    pop, _ = _population(e_all.spec, e_all.obs_soa.cpu().numpy(), SHAPES["1x16"], 4)
    full = e_all.rollout_population(pop, T, G, gamma=gamma, collect_obs=True, collect_rew=True, collect_actions=True)
    want = _returns(full["rew"], gamma)
    torch.cuda.synchronize()
    assert float(full["rew"].std()) > 0 and bool(torch.isfinite(full["ret"]).all())
    assert torch.equal(full["ret"], want), f"ret is not the recurrence over the recorded rewards (gamma = {gamma})"
    if gamma != 1.0:
        assert not torch.equal(full["ret"], _returns(full["rew"], 1.0))
    # nothing else recorded: the same returns
    only = e_ret.rollout_population(pop, T, G, gamma=gamma)
    torch.cuda.synchronize()
    assert only["a"] is None and only["obs"] is None and only["rew"] is None
    assert torch.equal(only["ret"], full["ret"]) and torch.equal(e_ret.x, e_all.x)
    # two chunks of 3, the second at t0 = 3: each returns the return of its own steps, discounted from its first
    for c in range(2):
        ch = e_chunk.rollout_population(pop, 3, G, gamma=gamma, collect_rew=True)
        torch.cuda.synchronize()
        assert torch.equal(ch["rew"], full["rew"][3 * c:3 * c + 3]), f"chunk {c}"
        assert torch.equal(ch["ret"], _returns(full["rew"][3 * c:3 * c + 3], gamma)), f"chunk {c}"
    assert e_chunk.t == T and torch.equal(e_chunk.x, e_all.x)
    for e in (e_all, e_ret, e_chunk):
        e.close()
    pop.close()


def test_shards_split_a_population_by_the_global_env_index():
    torch = _torch()
    p = _spread_x0(_plan("cstr_canonical", "rk4", noise=True, noise_percentage=0.002))
    whole = _make(p, 256, seed=9)
    parts = [_make(p, 128, seed=9, env_offset=off) for off in (0, 128)]
    for e in [whole] + parts:
        e.reset()
    assert torch.equal(torch.cat([e.x for e in parts], dim=1), whole.x)
    pop, _ = _population(whole.spec, whole.obs_soa.cpu().numpy(), SHAPES["1x16"], 4)
    kw = dict(gamma=0.99, collect_obs=True, collect_rew=True, collect_actions=True, record_next_action=True)
    w = whole.rollout_population(pop, T, G, **kw)
    ps = [e.rollout_population(pop, T, G, **kw) for e in parts]
    torch.cuda.synchronize()
    for n in ("a", "obs", "rew", "ret"):
        assert torch.equal(torch.cat([q[n] for q in ps], dim=-1), w[n]), n
    assert torch.equal(torch.cat([e.x for e in parts], dim=1), whole.x)
    assert torch.equal(torch.cat([e.obs_soa for e in parts], dim=1), whole.obs_soa)
    # the second shard is driven by members 2 and 3: not what members 0 and 1 do on the same envs
    alone = _make(p, 128, seed=9, env_offset=128)
    alone.reset()
    alone._lib.pcg_plan_set_env_offset(alone._plan, 0)  # (members 0 and 1; the reset above drew the shard's own states)
    other = alone.rollout_population(pop, 1, G, collect_actions=True)
    torch.cuda.synchronize()
    assert not torch.equal(other["a"][0], ps[1]["a"][0])
    for e in [whole, alone] + parts:
        e.close()
    pop.close()


def test_update_rewrites_one_member_and_no_other():
    torch = _torch()
    from pcgym_amd import PolicyPopulation

    p = _spread_x0(_plan("cstr_canonical", "rk4"))
    envs = [_make(p, B, seed=9) for _ in range(3)]
    for e in envs:
        e.reset()
    spec = envs[0].spec
    obs0 = envs[0].obs_soa.cpu().numpy()
    pop, mem = _population(spec, obs0, SHAPES["1x16"], 4)
    kw = dict(collect_obs=True, collect_rew=True, collect_actions=True)
    before = envs[0].rollout_population(pop, T, G, **kw)
    h = pop.handle(envs[0].device)
    new = make_policy(spec, obs0, SHAPES["1x16"], seed=99)
    pop.update_([w[None] for w in new.weights], [b[None] for b in new.biases], first=2)
    assert pop.handle(envs[0].device) is h  # the same device object, rewritten
    after = envs[1].rollout_population(pop, T, G, **kw)
    fresh = PolicyPopulation.from_policies(mem[:2] + [new] + mem[3:])
    want = envs[2].rollout_population(fresh, T, G, **kw)
    torch.cuda.synchronize()
    two = slice(2 * G, 3 * G)
    for n in ("a", "obs", "rew", "ret"):
        assert torch.equal(after[n], want[n]), n
        assert not torch.equal(after[n][..., two], before[n][..., two]), f"{n}: group 2 did not change"
        keep = torch.ones(B, dtype=torch.bool, device=after[n].device)
        keep[two] = False
        assert torch.equal(after[n][..., keep], before[n][..., keep]), f"{n}: another group's bits changed"
    for e in envs:
        e.close()
    pop.close(), fresh.close()


def test_evaluate_population_takes_the_fused_call():
    torch = _torch()
    from pcgym_amd import PolicyPopulation, evaluate_population

    Bn, g = 1024, 256
    p = _spread_x0(_plan("cstr_canonical", "rk4"), 0.01)  # (T0 <= 334 K, below the ignition branch)
    envs = [_make(p, Bn, seed=4) for _ in range(3)]
    for e in envs:
        e.reset()  # (evaluate_population resets again: the three envs stay in the same RNG epoch)
    spec = envs[0].spec
    pop, mem = _population(spec, envs[0].obs_soa.cpu().numpy(), SHAPES["1x16"], Bn // g, seed=23)
    pop2 = PolicyPopulation.from_policies([_perm_hidden(q, 5) for q in mem])
    envs[0]._lib.pcg_coverage_names(None, 0, 1)
    fused = evaluate_population(envs[0], pop, g, gamma=0.99)
    torch.cuda.synchronize()
    assert _launched(envs[0]._lib, "rollout_pop_policy_kernel"), "evaluate_population did not take the fused call"
    envs[1]._lib.pcg_coverage_names(None, 0, 1)
    ref = evaluate_population(envs[1], pop, g, gamma=0.99, fused=False)
    ref2 = evaluate_population(envs[2], pop2, g, gamma=0.99, fused=False)
    torch.cuda.synchronize()
    assert not _launched(envs[1]._lib, "rollout_pop_policy_kernel")
    assert fused["ret"].shape == (Bn,) and fused["score"].shape == (Bn // g,) and bool(torch.isfinite(fused["ret"]).all())
    assert torch.equal(fused["score"], fused["ret"].view(-1, g).mean(dim=1)) and float(fused["score"].std()) > 0

    def dist(a, b):
        return max(float((a[k] - b[k]).abs().max()) / max(1.0, float(b[k].abs().max())) for k in ("ret", "score"))

    spread, d = dist(ref2, ref), dist(fused, ref)
    print(f"evaluate_population B={Bn} G={g} N={spec.N}: per-step spread under hidden-unit permutation {spread:.3e}, fused vs per-step {d:.3e}")
    assert spread > 0, "the permuted run is bitwise the reference run: the spread measures nothing"
    assert d <= 8 * spread + 1e-13, f"fused result {d:.3e} from the per-step path; two per-step runs differ by {spread:.3e}"
    with pytest.raises(ValueError):
        evaluate_population(envs[0], pop, 96, fused=True)
    with pytest.raises(ValueError):
        evaluate_population(envs[0], pop, 128)  # eight slices, four members
    for e in envs:
        e.close()
    pop.close(), pop2.close()


def test_refusals_launch_nothing_and_write_nothing():
    torch = _torch()
    from pcgym_amd import _abi as abi
    from test_policy_jit_plans import _chemostat

    Bn, Tn = 256, 2

    class Case:
        def __init__(self, p, members=4, **kw):
            self.env = env = _make(p, Bn, seed=2, **kw)
            env.reset()
            s = self.spec = env.spec
            self.pop, _ = _population(s, env.obs_soa.cpu().numpy(), (16,), members, seed=3)
            shapes = {"a": (Tn + 1, s.na, Bn), "obs": (Tn, s.nobs, Bn), "rew": (Tn, Bn), "ret": (Bn,)}
            self.bufs = {n: torch.full(shp, -7.0, dtype=torch.float64, device=env.device) for n, shp in shapes.items()}
            self.x0, self.o0 = env.x.clone(), env.obs_soa.clone()
            torch.cuda.synchronize()
            env._lib.pcg_coverage_names(None, 0, 1)

        def call(self, pop=None, g=64, gamma=0.99, T=Tn):
            env, s, b = self.env, self.spec, self.bufs
            rc = env._lib.pcg_rollout_policy_pop(env._plan, env._bufp, (pop or self.pop).handle(env.device), g, 0, T, b["a"].data_ptr(),
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
            assert all(bool((b == -7.0).all()) for b in self.bufs.values()), f"{what}: a refused call wrote an output buffer"

        def close(self):
            self.env.close(), self.pop.close()

    base = _plan("cstr_canonical", "rk4")
    ok = Case(base)
    # ---- positive control: the valid call runs, writes every buffer, and is seen by the launch record ----
    assert ok.call() == abi.PCG_OK
    assert _launched(ok.env._lib, "rollout_pop_policy_kernel"), "the valid call launched nothing"
    assert not torch.equal(ok.env.x, ok.x0) and all(bool((b != -7.0).all()) for b in ok.bufs.values())
    ok.env.x.copy_(ok.x0), ok.env.obs_soa.copy_(ok.o0)
    for b in ok.bufs.values():
        b.fill_(-7.0)
    torch.cuda.synchronize()
    ok.env._lib.pcg_coverage_names(None, 0, 1)

    # ---- the population's own refusals ----
    ok.refused("envs_per_policy = 96", abi.PCG_E_VALUE, g=96)
    ok.refused("envs_per_policy = 0", abi.PCG_E_VALUE, g=0)
    ok.refused("gamma = 1.5", abi.PCG_E_VALUE, gamma=1.5)
    ok.refused("gamma = nan", abi.PCG_E_VALUE, gamma=float("nan"))
    small, _ = _population(ok.spec, ok.o0.cpu().numpy(), (16,), 3, seed=3)
    ok.refused("three members for four slices", abi.PCG_E_DIM, pop=small)
    wrong, _ = _population(type("S", (), dict(nobs=ok.spec.nobs + 1, na=ok.spec.na, normalise_o=True, normalise_a=True))(),
                           np.zeros((ok.spec.nobs + 1, 2)), (16,), 4, seed=3)
    ok.refused("members of another input size", abi.PCG_E_DIM, pop=wrong)
    ok.refused("members of another size and envs_per_policy = 96", abi.PCG_E_DIM, pop=wrong, g=96)  # sizes before slices
    ok.refused("T = 0", abi.PCG_E_VALUE, T=0)
    shifted = Case(base, env_offset=32, members=5)
    shifted.refused("env_offset = 32", abi.PCG_E_VALUE)

    # ---- the plans the kernel does not take ----
    cases = {n: Case(_plan(scen, over.get("integrator", "rk4"), **{k_: v for k_, v in over.items() if k_ != "integrator"}))
             for n, (scen, over) in UNSUPPORTED_PLANS.items() if n != "rodas5"}
    assert cases["constraints"].spec.ncon > 0 and cases["per_env_parameters"].spec.nunc > 0
    cases["dopri5"] = Case(_plan("cstr_canonical", "dopri5"))
    cases["per_env_t"] = Case(base, per_env_t=True)
    cases["chemostat"] = Case(_chemostat(integrator="rk4"))
    assert cases["chemostat"].spec.user_rhs_src is not None
    for n, c in cases.items():
        c.refused(n, abi.PCG_E_UNSUPPORTED)
        c.refused(n + " with envs_per_policy = 96", abi.PCG_E_UNSUPPORTED, g=96)  # the plan before the slices
    for c in [ok, shifted] + list(cases.values()):
        c.close()
    small.close(), wrong.close()


def test_stream_capture_replays_the_eager_call():
    torch = _torch()
    Bn, Tn, g = 8192, 12, 1024
    p = _plan("cstr_canonical", "rk4", noise=True, noise_percentage=0.002)
    env = _make(p, Bn, seed=6)
    spec = env.spec
    env.reset()
    pop, _ = _population(spec, env.obs_soa.cpu().numpy(), (16,), Bn // g, seed=29)
    h = pop.handle(env.device)
    x0, o0 = env.x.clone(), env.obs_soa.clone()
    f64, dev = torch.float64, env.device
    a_seq = torch.zeros((Tn + 1, spec.na, Bn), dtype=f64, device=dev)
    o_seq = torch.zeros((Tn, spec.nobs, Bn), dtype=f64, device=dev)
    r_seq = torch.zeros((Tn, Bn), dtype=f64, device=dev)
    ret = torch.zeros(Bn, dtype=f64, device=dev)
    seed = env._episode_seed()

    def call(stream):
        return env._lib.pcg_rollout_policy_pop(env._plan, env._bufp, h, g, 0, Tn, a_seq.data_ptr(), spec.na * Bn, Bn, o_seq.data_ptr(),
                                               spec.nobs * Bn, Bn, r_seq.data_ptr(), Bn, 1, 0.99, ret.data_ptr(), seed, stream)

    assert call(torch.cuda.current_stream(dev).cuda_stream) == 0
    torch.cuda.synchronize()
    outs = (a_seq, o_seq, r_seq, ret, env.x, env.obs_soa, env.rew, env.done)
    eager = [t.clone() for t in outs]
    assert float(a_seq.std()) > 0 and torch.equal(ret, _returns(r_seq, 0.99))
    gr = torch.cuda.CUDAGraph()
    env.x.copy_(x0), env.obs_soa.copy_(o0)
    torch.cuda.synchronize()
    with torch.cuda.graph(gr):
        rc = call(torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    for rep in range(2):
        for t in (a_seq, o_seq, r_seq, ret):
            t.fill_(-3.0)
        env.x.copy_(x0), env.obs_soa.copy_(o0)
        gr.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, eager):
            assert torch.equal(got, want), f"replay {rep} differs from the eager call"
    env.close(), pop.close()
