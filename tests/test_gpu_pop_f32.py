"""GPU: a FLOAT32 policy population (pcg_policy_pop_create_f32) through every layer: rollout_pop_policy_kernel_f32
(pcg_rollout_pop.hpp), the float32 search kernels (pcg_pop_search.hpp), PolicyPopulation(dtype="float32"), evaluate_population.
The env arithmetic is fp64 and unchanged; each member's network is evaluated in float32 (pcg_rollout_policy_f32.hpp's
specification), and a parameter written on the device is stored with one round-to-nearest conversion.

Shapes are the fp64 population tests': B = 200, T = 6, G = 64 -- three full waves and one of 8 lanes, four members.

  1. every instantiation   each key of CASE_KEYS x {rk4, cv8}, four distinct 1 x 16 float32 members placed by
                           test_gpu_pop_rollout._pick_members' conditioning rule: every recorded action a float32 value inside
                           test_policy_f32.bound32 of its member's np.longdouble reference on the kernel's own observation; the
                           recorded actions through the open-loop general kernel BITWISE; one call per step bitwise the one
                           call; every step within 1e-12 of the oracle; a quarter of the actions strictly inside the clip box;
  2. members               P copies of one float32 policy give rollout_policy's float32 bits; distinct members give, slice by
                           slice, the bits of rollout_policy with member(m) -- ragged widths, both activations, every map;
  3. returns               ret against the stated recurrence in torch, bit for bit; with nothing else recorded; per chunk;
  4. shards                two envs with env offsets 0 and 128 against the one env of 200;
  5. update_               rewriting member 2 changes group 2's bits and no other; equal to a fresh population;
  6. weights on the device flat / set_flat_ / sample_ / noise_dot against numpy built from the oracle's Philox and Box-Muller,
                           bitwise; sample_ = float32 of the fp64 population's; a rollout after every device-side write equals
                           the rollout of a fresh population built from flat() (header, padding and the interleaved map intact);
  7. public path           evaluate_population fused against the per-step route with the float32 callable;
  8. refusals              the statuses, in the fp64 population's order, nothing launched, nothing written;
  9. stream capture        one call inside torch.cuda.graph, replayed twice, equal to the eager call.

Measured figures are printed and, when PCG_RECORD_DIR names a directory, appended to pop_f32_test.txt there.
"""
import numpy as np
import pytest

from helpers import (CASE_KEYS, LD, PRE_MAX, SHAPES, UNSUPPORTED_PLANS, _case_params, _launch_names, _launched, _make, _perm_hidden,
                     _spread_x0, _torch, make_policy)
from helpers import _record as _record_to
from pcgym_amd import _abi as abi
from test_gpu_policy_f32 import ULP32, is_f32, tanh32_k, to32
from test_gpu_pop_rollout import REMAPS, _pick_members, _plan, _returns
from test_gpu_pop_search import SEED, _host_flat, _np, _pop, noise_dot_ref, same_bits, z_ref
from test_policy_f32 import bound32

pytestmark = pytest.mark.gpu

B, T, G = 200, 6, 64  # three full waves and a wave of 8 lanes: four members
KERNEL = "rollout_pop_policy_kernel_f32"
KW = dict(collect_obs=True, collect_rew=True, collect_actions=True, record_next_action=True)


def _record(line):
    _record_to("pop_f32_test.txt", line)


def _population32(spec, obs0, hidden, P, seed=17, **kw):
    """float32 members that really differ: make_policy with seeds seed + m, rounded to float32"""
    from pcgym_amd import PolicyPopulation

    mem = [to32(make_policy(spec, obs0, hidden, seed=seed + m, **kw)) for m in range(P)]
    return PolicyPopulation.from_policies(mem), mem


def _r32(a):
    """round to nearest float32, widened back: what a float32 population stores of a float64 value"""
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ---- 1. every instantiation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integ", ["rk4", "cv8"])
@pytest.mark.parametrize("key", CASE_KEYS)
def test_population_rollout_f32(key, integ):
    torch = _torch()
    from oracle import oracle as O
    from pcgym_amd import PolicyPopulation

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
    # (the conditioning rule is the oracle's own, evaluated on the host on the float64 networks before any kernel runs)
    mem64, (centre, scale, amp) = _pick_members(spec, obs0, SHAPES["1x16"], P, G, B, T, env_seed=9)
    assert (centre, scale) in REMAPS
    mem = [to32(q) for q in mem64]
    pop = PolicyPopulation.from_policies(mem)
    assert P == 4 and pop.dtype == "float32" and pop.validate() == 0
    k = tanh32_k()
    e_one._lib.pcg_coverage_names(None, 0, 1)

    # ---- the fused closed loop: one call ----
    out = e_one.rollout_population(pop, T, G, gamma=0.99, **KW)
    torch.cuda.synchronize()
    names = _launch_names(e_one._lib)
    assert any(KERNEL in n for n in names), f"rollout_population of a float32 population launched {names}"
    assert e_one._lib.pcg_policy_pop_dtype(pop.handle(e_one.device)) == abi.PCG_POL_F32
    a_seq, obs_seq, rew_seq = out["a"], out["obs"], out["rew"]
    a_np, o_np = a_seq.cpu().numpy(), obs_seq.cpu().numpy()
    assert a_np.shape == (T + 1, spec.na, B) and o_np.shape == (T, spec.nobs, B) and out["ret"].shape == (B,)
    assert np.isfinite(a_np).all() and np.isfinite(o_np).all() and not e_one.status.any()
    assert torch.equal(e_one.obs_soa, obs_seq[T - 1]) and torch.equal(e_one.rew, rew_seq[T - 1])  # io-> hold the last step
    assert e_one.t == T
    assert torch.equal(out["ret"], _returns(rew_seq, 0.99))

    # ---- action check, per group: a float32 value inside the float32 bound of member m on the kernel's own obs[s-1] ----
    assert is_f32(a_np), "a recorded output of a float32 member is not a float32 value"
    worst, pre = 0.0, 0.0
    for m in range(P):
        sl = slice(m * G, min(B, (m + 1) * G))
        for s in range(T + 1):
            o_in = obs0[:, sl] if s == 0 else o_np[s - 1][:, sl]
            ref, bound, pm = bound32(mem[m], o_in, k + 1.0)
            pre = max(pre, pm)
            diff = np.abs(a_np[s][:, sl].astype(LD) - ref).astype(np.float64)
            frac = float(np.max(diff / np.maximum(bound, 1e-300)))
            assert np.all(diff <= bound), (f"member {m} step {s}: policy output off by {np.max(diff):.3e}, {frac:.2f} x "
                                           f"the float32 running bound ({np.max(bound):.3e})")
            worst = max(worst, frac)
    assert pre <= PRE_MAX, f"pre-activations up to {pre:.1f}: outside the grid the tanhf error was measured on"
    inside = float(np.mean((a_np > pop.out_low) & (a_np < pop.out_high)))
    print(f"case {key}-{integ}: output layers at {centre:+.2f} half widths x {scale:.2f} (oracle amplification {amp:.2e}), "
          f"{inside:.2f} of the actions inside the box, worst {worst:.3f} x the float32 bound")
    assert inside >= 0.25, f"only {inside:.2f} of the recorded actions lie strictly inside the clip box"
    assert np.std(a_np) > 0
    # the groups are driven by different members: group 1's first actions are not member 0's on group 1's observations
    o1 = torch.as_tensor(obs0[:, G:2 * G].T.copy())
    assert not np.array_equal(mem[0](o1).numpy().T, a_np[0][:, G:2 * G])

    # ---- dynamics check: the recorded actions through the open-loop rollout, general kernel: bitwise ----
    assert np.array_equal(e_open.x.cpu().numpy(), x0)
    oq, rq = e_open.rollout(a_seq[:T].contiguous(), collect_obs=True, collect_rew=True)
    torch.cuda.synchronize()
    assert torch.equal(oq, obs_seq), "observations differ from the open-loop replay of the recorded actions"
    assert torch.equal(rq, rew_seq), "rewards differ from the open-loop replay"
    assert torch.equal(e_open.x, e_one.x), "final state differs from the open-loop replay"
    assert torch.equal(e_open.done, e_one.done) and torch.equal(e_open.status, e_one.status)
    if spec.a_delta:
        assert torch.equal(e_open.a_save_t, e_one.a_save_t)

    # ---- oracle check: one call per step == the one call, bitwise; every step against the oracle, every lane ----
    orc = O.OracleEnv(spec, B, seed=9)
    orc.reset()
    assert np.allclose(orc.x, x0, rtol=1e-14, atol=0)
    worst_x = 0.0
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
        worst_x = max(worst_x, err)
        assert np.array_equal(e_chain.done.cpu().numpy(), dc)
        if not spec.noise:  # (with noise the observation carries the noise twin's fp32 variates: compared through x and the reward)
            assert np.allclose(c1["obs"][0].cpu().numpy(), oc, rtol=1e-10, atol=1e-11)
        assert np.allclose(c1["rew"][0].cpu().numpy(), rc, rtol=1e-9, atol=1e-10 * (1 + np.max(np.abs(rc))))
    assert torch.equal(e_chain.x, e_one.x)
    _record(f"population {key}-{integ}: output error <= {worst:.3f} x float32 bound (tanhf {k:.3f} ulp), |pre-activation| <= {pre:.2f}, "
            f"{inside:.2f} of the actions inside the box, state vs oracle {worst_x:.2e}")
    for e in (e_one, e_chain, e_open):
        e.close()
    pop.close()


# ---- 2. a population is its members -------------------------------------------------------------------------------------------
# (the two ragged shapes put an odd unit count in every role: the interleaved pair's second half is padding)
MEMBER_SHAPES = dict(SHAPES, **{"5": (5,), "7x3": (7, 3)})


@pytest.mark.parametrize("shape", list(MEMBER_SHAPES))
@pytest.mark.parametrize("integ", ["rk4", "cv8"])
def test_a_float32_population_is_its_members(integ, shape):
    """both kernels execute the same policy_raw_f32 + policy_map_f32 and the same env_step: bits, not tolerances"""
    torch = _torch()
    from pcgym_amd import PolicyPopulation

    p = _spread_x0(_plan("cstr_canonical", integ))
    P = (B + G - 1) // G
    for act in ("tanh", "relu"):
        for out_map in ("clip", "none", "tanh"):
            tag = f"{integ}-{shape}-{act}-{out_map}"
            envs = [_make(p, B, seed=9) for _ in range(3 + P)]
            for e in envs:
                e.reset()
            spec = envs[0].spec
            obs0 = envs[0].obs_soa.cpu().numpy().copy()
            pop, mem = _population32(spec, obs0, MEMBER_SHAPES[shape], P, activation=act, out_map=out_map)
            assert pop.dtype == "float32" and (pop.activation, pop.out_map) == (act, out_map)

            # P copies of one float32 policy: rollout_policy's float32 bits
            same = PolicyPopulation.from_policies([mem[0]] * P)
            envs[0]._lib.pcg_coverage_names(None, 0, 1)
            got = envs[0].rollout_population(same, T, G, **KW)
            a, o, r = envs[1].rollout_policy(mem[0], T, **KW)
            torch.cuda.synchronize()
            assert _launched(envs[0]._lib, KERNEL) and _launched(envs[0]._lib, "rollout_policy_kernel_f32"), tag
            assert bool(torch.isfinite(a).all()) and float(a.std()) > 0, tag
            assert torch.equal(got["a"], a) and torch.equal(got["obs"], o) and torch.equal(got["rew"], r), tag
            assert torch.equal(envs[0].x, envs[1].x) and torch.equal(envs[0].obs_soa, envs[1].obs_soa) and torch.equal(envs[0].done, envs[1].done), tag

            # distinct members: group m's slice is rollout_policy with member(m) on an identical full-batch env
            got = envs[2].rollout_population(pop, T, G, **KW)
            for m in range(P):
                sl = slice(m * G, min(B, (m + 1) * G))
                em = envs[3 + m]
                qm = pop.member(m)
                assert qm.dtype == "float32"
                a, o, r = em.rollout_policy(qm, T, **KW)
                torch.cuda.synchronize()
                assert torch.equal(got["a"][..., sl], a[..., sl]), f"{tag} member {m}: actions"
                assert torch.equal(got["obs"][..., sl], o[..., sl]) and torch.equal(got["rew"][..., sl], r[..., sl]), f"{tag} member {m}"
                assert torch.equal(envs[2].x[..., sl], em.x[..., sl]), f"{tag} member {m}: final state"
                qm.close()
                if m == 0:
                    a_first = a
            # (the members really differ: group 1 is not what member 0 does on group 1's envs)
            assert not torch.equal(got["a"][..., G:2 * G], a_first[..., G:2 * G]), tag
            for e in envs:
                e.close()
            pop.close(), same.close()


# ---- 3. returns ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [1.0, 0.99])
def test_returns_f32(gamma):
    torch = _torch()
    p = _spread_x0(_plan("cstr_canonical", "rk4"))
    e_all, e_ret, e_chunk = (_make(p, B, seed=9) for _ in range(3))
    for e in (e_all, e_ret, e_chunk):
        e.reset()
    pop, _ = _population32(e_all.spec, e_all.obs_soa.cpu().numpy(), SHAPES["1x16"], 4)
    e_all._lib.pcg_coverage_names(None, 0, 1)
    full = e_all.rollout_population(pop, T, G, gamma=gamma, collect_obs=True, collect_rew=True, collect_actions=True)
    want = _returns(full["rew"], gamma)
    torch.cuda.synchronize()
    assert _launched(e_all._lib, KERNEL)
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


# ---- 4. shards ----------------------------------------------------------------------------------------------------------------
def test_shards_split_a_float32_population_by_the_global_env_index():
    torch = _torch()
    p = _spread_x0(_plan("cstr_canonical", "rk4", noise=True, noise_percentage=0.002))
    whole = _make(p, B, seed=9)
    parts = [_make(p, n, seed=9, env_offset=off) for off, n in ((0, 128), (128, B - 128))]
    for e in [whole] + parts:
        e.reset()
    assert torch.equal(torch.cat([e.x for e in parts], dim=1), whole.x)
    pop, _ = _population32(whole.spec, whole.obs_soa.cpu().numpy(), SHAPES["1x16"], 4)
    w = whole.rollout_population(pop, T, G, gamma=0.99, **KW)
    ps = [e.rollout_population(pop, T, G, gamma=0.99, **KW) for e in parts]
    torch.cuda.synchronize()
    for n in ("a", "obs", "rew", "ret"):
        assert torch.equal(torch.cat([q[n] for q in ps], dim=-1), w[n]), n
    assert torch.equal(torch.cat([e.x for e in parts], dim=1), whole.x)
    assert torch.equal(torch.cat([e.obs_soa for e in parts], dim=1), whole.obs_soa)
    # the second shard is driven by members 2 and 3: not what members 0 and 1 do on the same envs
    alone = _make(p, B - 128, seed=9, env_offset=128)
    alone.reset()
    alone._lib.pcg_plan_set_env_offset(alone._plan, 0)  # (members 0 and 1; the reset above drew the shard's own states)
    other = alone.rollout_population(pop, 1, G, collect_actions=True)
    torch.cuda.synchronize()
    assert not torch.equal(other["a"][0], ps[1]["a"][0])
    for e in [whole, alone] + parts:
        e.close()
    pop.close()


# ---- 5. update_ ---------------------------------------------------------------------------------------------------------------
def test_update_rewrites_one_float32_member_and_no_other():
    torch = _torch()
    from pcgym_amd import PolicyPopulation

    p = _spread_x0(_plan("cstr_canonical", "rk4"))
    envs = [_make(p, B, seed=9) for _ in range(3)]
    for e in envs:
        e.reset()
    spec = envs[0].spec
    obs0 = envs[0].obs_soa.cpu().numpy()
    pop, mem = _population32(spec, obs0, SHAPES["1x16"], 4)
    kw = dict(collect_obs=True, collect_rew=True, collect_actions=True)
    before = envs[0].rollout_population(pop, T, G, **kw)
    h = pop.handle(envs[0].device)
    new = make_policy(spec, obs0, SHAPES["1x16"], seed=99)  # (float64 arrays: update_ rounds first)
    bad = [w[None].copy() for w in new.weights]
    bad[0][0, 3, 0] = 1e39
    with pytest.raises(ValueError, match="overflows float32"):
        pop.update_(bad, [b[None] for b in new.biases], first=2)
    pop.update_([w[None] for w in new.weights], [b[None] for b in new.biases], first=2)
    assert pop.handle(envs[0].device) is h and pop.dtype == "float32"  # the same device object, rewritten
    after = envs[1].rollout_population(pop, T, G, **kw)
    fresh = PolicyPopulation.from_policies(mem[:2] + [to32(new)] + mem[3:])
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


# ---- 6. weights on the device -------------------------------------------------------------------------------------------------
P6 = 6  # antithetic pairs and a sub-range both exist
SEARCH_CASES = [("cstr_canonical", "rk4", (5, 3)), ("four_tank_canonical", "cv8", (5, 3)), ("cstr_canonical", "rk4", (64, 64))]


class _Search:
    """P6 x G envs of one plan, and rollouts of a float32 population on fresh envs of it"""

    def __init__(self, scen, integ, hidden):
        self.p = _spread_x0(_plan(scen, integ))
        probe = _make(self.p, P6 * G, seed=3)
        self.spec, self.dev = probe.spec, probe.device
        probe.close()
        self.dims = [self.spec.nobs] + list(hidden) + [self.spec.na]

    def pop(self, seed=5, dtype="float32"):
        q = _pop(self.dims, P6, seed=seed, out_low=-1.0, out_high=1.0, dtype=dtype)
        q.handle(self.dev)
        return q

    def roll(self, pop):
        torch = _torch()
        env = _make(self.p, P6 * G, seed=3)
        env.reset()
        env._lib.pcg_coverage_names(None, 0, 1)
        out = env.rollout_population(pop, 5, G, gamma=0.99, collect_actions=True)
        torch.cuda.synchronize()
        assert _launched(env._lib, KERNEL if pop.dtype == "float32" else "rollout_pop_policy_kernelI")
        res = {n: out[n].clone() for n in ("a", "ret")}
        res["x"] = env.x.clone()
        env.close()
        return res

    def fresh_from(self, theta):
        """a float32 population created on the host from flat parameter rows (float32 values)"""
        from pcgym_amd import PolicyPopulation

        proto = _pop(self.dims, P6, seed=1, dtype="float32")
        lay = proto.flat_layout()
        proto.close()
        Ws = [theta[:, a:b].reshape((P6,) + shape) for name, l, a, b, shape in lay if name == "W"]
        bs = [theta[:, a:b].reshape((P6,) + shape) for name, l, a, b, shape in lay if name == "b"]
        q = PolicyPopulation(Ws, bs, out_low=-1.0, out_high=1.0, dtype="float32")
        assert same_bits(_host_flat(q).astype(np.float64), theta)  # (float32 values: the rounding changed nothing)
        return q

    def written_rolls_like_fresh(self, pop, what):
        """the written population against a fresh one built from flat()'s values: header, padding and the interleaved map"""
        torch = _torch()
        theta = _np(pop.flat())
        assert np.isfinite(theta).all() and is_f32(theta), what
        fresh = self.fresh_from(theta)
        got, want = self.roll(pop), self.roll(fresh)
        for n in ("a", "ret", "x"):
            assert torch.equal(got[n].view(torch.int64), want[n].view(torch.int64)), f"{what}: {n} of the written population is not the fresh one's"
        a0 = got["a"][0, 0].view(P6, G)
        assert float(a0.std()) > 0 and len(torch.unique(a0, dim=0)) > 2, what  # the members really differ
        fresh.close()
        return got


def _mean_std6(n, seed=8):
    rng = np.random.default_rng(seed)
    return 0.3 * rng.standard_normal(n), np.where(np.arange(n) == n // 2, 0.0, 0.4)  # (one parameter held fixed)


@pytest.mark.parametrize("scen,integ,hidden", SEARCH_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_flat_and_set_flat_of_a_float32_population(scen, integ, hidden):
    torch = _torch()
    S = _Search(scen, integ, hidden)
    pop = S.pop()
    n = pop.n_params
    host = _host_flat(pop)
    assert host.dtype == np.float32
    from pcgym_amd import _lib

    h = pop.handle(S.dev)
    assert _lib.load().pcg_policy_pop_dtype(h) == abi.PCG_POL_F32 and _lib.load().pcg_policy_pop_nparams(h) == n
    assert same_bits(_np(pop.flat()), host.astype(np.float64))  # get_flat against the host packing, widened exactly
    # random fp64 theta with full mantissas (from the oracle's variates): stored rounded to nearest, handed back widened
    z = z_ref(np.arange(P6), n, SEED, 11, False)
    theta = z * 0.3 + 0.01
    assert not is_f32(theta)
    pop.set_flat_(torch.as_tensor(theta, device=S.dev))
    got = _np(pop.flat())
    assert same_bits(got, _r32(theta))
    rows = _np(pop.flat(members=[5, 0, 0, -1, 6]))
    assert same_bits(rows[:3], _r32(theta)[[5, 0, 0]]) and np.isnan(rows[3:]).all() and rows.shape == (5, n)
    assert same_bits(_np(pop.flat()), _r32(theta))  # (the bad indices disturbed nothing)
    S.written_rolls_like_fresh(pop, "set_flat_")
    # a sub-range from a strided view; the other members keep their bits
    wide = torch.full((2, n + 3), -9.0, dtype=torch.float64, device=S.dev)
    wide[:, :n] = torch.as_tensor(theta[:2] * 0.5, device=S.dev)
    pop.set_flat_(wide[:, :n], first=3)
    want = _r32(theta)
    want[3:5] = _r32(theta[:2] * 0.5)
    assert same_bits(_np(pop.flat()), want)
    # the host mirror: float32 arrays holding the device values exactly
    assert pop._stale.all()
    m4 = pop.member(4)
    assert m4.dtype == "float32" and not pop._stale.any() and all(w.dtype == np.float32 for w in pop.weights + pop.biases)
    assert same_bits(_host_flat(pop).astype(np.float64), want)
    m4.close(), pop.close()


@pytest.mark.parametrize("anti", [False, True], ids=["plain", "antithetic"])
@pytest.mark.parametrize("scen,integ,hidden", SEARCH_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_sample_of_a_float32_population(scen, integ, hidden, anti):
    torch = _torch()
    S = _Search(scen, integ, hidden)
    pop, pop64 = S.pop(), S.pop(dtype="float64")
    n = pop.n_params
    mean, std = _mean_std6(n)
    for gen in (0, 3):
        pop.sample_(mean, std, SEED, generation=gen, antithetic=anti)
        got = _np(pop.flat())
        z = z_ref(np.arange(P6), n, SEED, gen, anti)
        assert same_bits(got, _r32(mean + std * z)), (gen, anti)
        # ... which is float32 of what the fp64 population holds under the same arguments
        pop64.sample_(mean, std, SEED, generation=gen, antithetic=anti)
        wide = _np(pop64.flat())
        assert same_bits(wide, mean + std * z) and same_bits(got, _r32(wide)) and not same_bits(got, wide)
        if anti:  # (rounding to nearest is odd: the negated noise of a pair survives it exactly at mean = 0)
            pop.sample_(np.zeros(n), std, SEED, generation=gen, antithetic=True)
            zz = _np(pop.flat())
            assert np.array_equal(zz[1::2], -zz[0::2]) and float(np.abs(zz).max()) > 0
            pop.sample_(mean, std, SEED, generation=gen, antithetic=anti)
        res = S.written_rolls_like_fresh(pop, f"sample_ generation {gen}")
    # after sample_, member(i) comes back float32 and rolls like its group
    assert pop._stale.all()
    for i in (1, P6 - 1):
        q = pop.member(i)
        assert q.dtype == "float32" and all(w.dtype == np.float32 for w in q.weights + q.biases)
        flat_i = np.concatenate([np.concatenate([w.ravel(), b]) for w, b in zip(q.weights, q.biases)]).astype(np.float64)
        assert same_bits(flat_i, got[i])
        env = _make(S.p, P6 * G, seed=3)
        env.reset()
        a, _, _ = env.rollout_policy(q, 5, collect_rew=False)
        torch.cuda.synchronize()
        sl = slice(i * G, (i + 1) * G)
        assert torch.equal(a[..., sl], res["a"][..., sl]) and torch.equal(env.x[..., sl], res["x"][..., sl]), f"member {i}"
        env.close(), q.close()
    # a sub-range: members 0, 1 and 5 bitwise untouched
    before = _np(pop.flat())
    pop.sample_(mean, std, SEED + 1, generation=1, antithetic=anti, first=2, count=3)
    part = _np(pop.flat())
    assert same_bits(part[2:5], _r32(mean + std * z_ref([2, 3, 4], n, SEED + 1, 1, anti))) and not np.array_equal(part[2:5], before[2:5])
    assert same_bits(part[[0, 1, 5]], before[[0, 1, 5]])
    S.written_rolls_like_fresh(pop, "sample_ of a sub-range")
    # an overflow is stored as an infinity of its sign, in exactly that parameter, and not inspected
    big = mean.copy()
    big[0], big[1] = 1e39, -1e39
    pop.sample_(big, std, SEED, generation=0, antithetic=anti, first=1, count=1)
    ov = _np(pop.flat())
    assert ov[1, 0] == np.inf and ov[1, 1] == -np.inf and np.isfinite(ov[1, 2:]).all() and same_bits(ov[[0, 2, 3, 4, 5]], part[[0, 2, 3, 4, 5]])
    pop.close(), pop64.close()


@pytest.mark.parametrize("anti", [False, True], ids=["plain", "antithetic"])
def test_noise_dot_does_not_depend_on_the_storage(anti):
    S = _Search("cstr_canonical", "rk4", (5, 3))
    pop, pop64 = S.pop(), S.pop(dtype="float64")
    n = pop.n_params
    rng = np.random.default_rng(4)
    for first, count in ((0, P6), (2, 3)):
        w = rng.standard_normal(count)
        got = _np(pop.noise_dot(w, SEED, generation=9, antithetic=anti, first=first))
        wide = _np(pop64.noise_dot(w, SEED, generation=9, antithetic=anti, first=first))
        assert same_bits(got, wide)
        assert same_bits(got, noise_dot_ref(w, z_ref(first + np.arange(count), n, SEED, 9, anti)))
    assert same_bits(_np(pop.flat()), _host_flat(pop).astype(np.float64))  # noise_dot writes no member
    pop.close(), pop64.close()


# ---- 7. the public path -------------------------------------------------------------------------------------------------------
def test_evaluate_population_takes_the_float32_fused_call():
    """The bar is test_gpu_policy_f32's for its collectors: the fused result within 8 x the spread of two per-step float32 runs
    that differ only in the order of the hidden units, plus 8 float32 ulps -- of the action scale (the actions are normalised:
    1), carried through the return in the same relative measure (distances relative to max(1, largest |ret|))."""
    torch = _torch()
    from pcgym_amd import PolicyPopulation, evaluate_population

    Bn, g = 1024, 256
    p = _spread_x0(_plan("cstr_canonical", "rk4"), 0.01)  # (T0 <= 334 K, below the ignition branch)
    envs = [_make(p, Bn, seed=4) for _ in range(3)]
    for e in envs:
        e.reset()  # (evaluate_population resets again: the three envs stay in the same RNG epoch)
    spec = envs[0].spec
    pop, mem = _population32(spec, envs[0].obs_soa.cpu().numpy(), SHAPES["1x16"], Bn // g, seed=23)
    pop2 = PolicyPopulation.from_policies([to32(_perm_hidden(q, 5)) for q in mem])
    assert pop2.dtype == "float32"
    envs[0]._lib.pcg_coverage_names(None, 0, 1)
    fused = evaluate_population(envs[0], pop, g, gamma=0.99)
    torch.cuda.synchronize()
    assert _launched(envs[0]._lib, KERNEL), "evaluate_population did not take the float32 fused call"
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
    _record(f"evaluate_population float32 B={Bn} G={g} N={spec.N}: per-step spread under hidden-unit permutation {spread:.3e}, "
            f"fused vs per-step {d:.3e} ({d / max(spread, 1e-300):.2f} x)")
    assert spread > 0, "the permuted run is bitwise the reference run: the spread measures nothing"
    assert d <= 8 * spread + 8 * ULP32, f"fused result {d:.3e} from the per-step path; two per-step runs differ by {spread:.3e}"
    with pytest.raises(ValueError):
        evaluate_population(envs[0], pop, 96, fused=True)  # (fused_pop_ok is False)
    with pytest.raises(ValueError):
        evaluate_population(envs[0], pop, 128)  # eight slices, four members
    for e in envs:
        e.close()
    pop.close(), pop2.close()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_of_a_float32_population_launch_nothing_and_write_nothing():
    torch = _torch()
    from pcgym_amd import PolicyPopulation
    from test_policy_jit_plans import _chemostat

    Bn, Tn = 256, 2

    def both(spec, obs0, members, n_in=None):
        """(float32 population, the fp64 population of the same rounded weights)"""
        s = spec if n_in is None else type("S", (), dict(nobs=n_in, na=spec.na, normalise_o=True, normalise_a=True))()
        o = obs0 if n_in is None else np.zeros((n_in, 2))
        p32, mem = _population32(s, o, (16,), members, seed=3)
        return p32, PolicyPopulation([w.astype(np.float64) for w in p32.weights], [b.astype(np.float64) for b in p32.biases],
                                     activation=p32.activation, out_map=p32.out_map, out_low=p32.out_low, out_high=p32.out_high)

    class Case:
        def __init__(self, p, members=4, **kw):
            self.env = env = _make(p, Bn, seed=2, **kw)
            env.reset()
            s = self.spec = env.spec
            self.pop, self.pop64 = both(s, env.obs_soa.cpu().numpy(), members)
            shapes = {"a": (Tn + 1, s.na, Bn), "obs": (Tn, s.nobs, Bn), "rew": (Tn, Bn), "ret": (Bn,)}
            self.bufs = {n: torch.full(shp, -7.0, dtype=torch.float64, device=env.device) for n, shp in shapes.items()}
            self.x0, self.o0 = env.x.clone(), env.obs_soa.clone()
            lib, dev = env._lib, env.device
            assert lib.pcg_policy_pop_dtype(self.pop.handle(dev)) == abi.PCG_POL_F32 and lib.pcg_policy_pop_dtype(self.pop64.handle(dev)) == abi.PCG_POL_F64
            torch.cuda.synchronize()
            lib.pcg_coverage_names(None, 0, 1)

        def call(self, pop=None, g=64, gamma=0.99, T=Tn):
            env, s, b = self.env, self.spec, self.bufs
            rc = env._lib.pcg_rollout_policy_pop(env._plan, env._bufp, (pop or self.pop).handle(env.device), g, 0, T, b["a"].data_ptr(),
                                                 s.na * Bn, Bn, b["obs"].data_ptr(), s.nobs * Bn, Bn, b["rew"].data_ptr(), Bn, 1,
                                                 gamma, b["ret"].data_ptr(), 1, None)
            torch.cuda.synchronize()
            return rc

        def refused(self, what, want, pops=None, **kw):
            for kind, pop in zip(("float32", "float64"), pops or (self.pop, self.pop64)):  # the same status, in the same order, for both kinds
                rc = self.call(pop=pop, **kw)
                assert rc == want, f"{what} ({kind} population): status {rc}, not {want}"
                names = _launch_names(self.env._lib, reset=True)
                assert not names, f"{what} ({kind}): a refused call launched or compiled {names}"
                assert torch.equal(self.env.x, self.x0) and torch.equal(self.env.obs_soa, self.o0), f"{what} ({kind}): a refused call wrote the env"
                assert all(bool((b == -7.0).all()) for b in self.bufs.values()), f"{what} ({kind}): a refused call wrote an output buffer"

        def close(self):
            self.env.close(), self.pop.close(), self.pop64.close()

    base = _plan("cstr_canonical", "rk4")
    ok = Case(base)
    lib = ok.env._lib
    assert lib.pcg_policy_pop_dtype(None) == abi.PCG_E_NULL
    pol = ok.pop.member(0)
    assert lib.pcg_policy_pop_dtype(pol.handle(ok.env.device)) == abi.PCG_E_PLAN  # (a single policy is not a population)
    pol.close()
    # ---- positive control: the valid call runs the float32 kernel, writes every buffer, and is seen by the launch record ----
    assert ok.call() == abi.PCG_OK
    assert _launched(lib, KERNEL), "the valid call launched nothing"
    assert not torch.equal(ok.env.x, ok.x0) and all(bool((b != -7.0).all()) for b in ok.bufs.values())
    ok.env.x.copy_(ok.x0), ok.env.obs_soa.copy_(ok.o0)
    for b in ok.bufs.values():
        b.fill_(-7.0)
    torch.cuda.synchronize()
    lib.pcg_coverage_names(None, 0, 1)

    # ---- the population's own refusals ----
    ok.refused("envs_per_policy = 96", abi.PCG_E_VALUE, g=96)
    ok.refused("gamma = 1.5", abi.PCG_E_VALUE, gamma=1.5)
    small = both(ok.spec, ok.o0.cpu().numpy(), 3)
    ok.refused("three members for four slices", abi.PCG_E_DIM, pops=small)
    wrong = both(ok.spec, None, 4, n_in=ok.spec.nobs + 1)
    ok.refused("members of another input size", abi.PCG_E_DIM, pops=wrong)
    ok.refused("members of another size and envs_per_policy = 96", abi.PCG_E_DIM, pops=wrong, g=96)  # sizes before slices
    ok.refused("three members and envs_per_policy = 96", abi.PCG_E_VALUE, pops=small, g=96)  # slices before the member count
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
    for q in small + wrong:
        q.close()


# ---- 9. stream capture --------------------------------------------------------------------------------------------------------
def test_stream_capture_replays_the_eager_float32_call():
    torch = _torch()
    p = _spread_x0(_plan("cstr_canonical", "rk4", noise=True, noise_percentage=0.002))
    env = _make(p, B, seed=6)
    spec = env.spec
    env.reset()
    pop, _ = _population32(spec, env.obs_soa.cpu().numpy(), (16,), 4, seed=29)
    h = pop.handle(env.device)
    x0, o0 = env.x.clone(), env.obs_soa.clone()
    f64, dev = torch.float64, env.device
    a_seq = torch.zeros((T + 1, spec.na, B), dtype=f64, device=dev)
    o_seq = torch.zeros((T, spec.nobs, B), dtype=f64, device=dev)
    r_seq = torch.zeros((T, B), dtype=f64, device=dev)
    ret = torch.zeros(B, dtype=f64, device=dev)
    seed = env._episode_seed()

    def call(stream):
        return env._lib.pcg_rollout_policy_pop(env._plan, env._bufp, h, G, 0, T, a_seq.data_ptr(), spec.na * B, B, o_seq.data_ptr(),
                                               spec.nobs * B, B, r_seq.data_ptr(), B, 1, 0.99, ret.data_ptr(), seed, stream)

    env._lib.pcg_coverage_names(None, 0, 1)
    assert call(torch.cuda.current_stream(dev).cuda_stream) == 0
    torch.cuda.synchronize()
    assert _launched(env._lib, KERNEL)
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
