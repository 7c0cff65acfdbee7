"""The order in which the six fused closed-loop entry points refuse bad arguments (pcg_abi_policy.hip: closed_loop_open, the head's
own function, closed_loop_launch -- read top to bottom):

   1  plan and buffers (fill_args)                          PLAN / NULL / DIM
   2  policy handle null                                    NULL
   3  policy handle magic / device                          PLAN
   4  a plan the kind does not carry                        UNSUPPORTED   (cons / unc: a float32 actor or policy too)
   5  no kernel in the table                                UNSUPPORTED
   6  policy sizes                                          DIM
   7  actor: critic magic / device, then (cons / unc) a float32 critic, then its sizes, then its map
                                                            PLAN, UNSUPPORTED, DIM, VALUE
   8  actor: tanh-mapped actor                              UNSUPPORTED
   9  actor: sigma null, then not finite / positive         NULL, VALUE
  10  step range                                            VALUE
  11  B == 0                                                OK, nothing launched
  12  null x / obs / rew / done, a_save, u_prev, (unc) p_unc    NULL
  13  observation component stride, then the head's sequences   DIM
  14  cons: row / flag strides, the overlap rule            DIM
  15  base: actor and critic of two dtypes, then float32 on a run-time compiled plan    UNSUPPORTED
  16  run-time compiled plans: capture status, module build, launch

For every entry point: one valid call as the positive control, then for every pair of ADJACENT stages it has one call that
carries both defects and must return the earlier stage's status -- and the later defect alone, which must return another
status (otherwise the pair shows nothing).  Pairs that cannot be told apart are left out, each with its reason:

   2 | 3    one handle is either null or junk
   4 | 5    the same status; and pcg_plan_create refuses every plan that would reach stage 5 alone (per-env parameters on a
            model without kernels for them)
   7        a junk critic handle has no dtype, size or map: only dtype | size and size | map can be combined
   9        one sigma is either null or holds values; 9 | 10 return VALUE both with a bad value, so the null sigma is held
            against stage 10 and the bad value against stage 12
  12, 13    every clause of either stage returns one status
  13 | 14   DIM both: stage 14 is held against stage 12 instead
  15        UNSUPPORTED both; 15 | 16 too (a capture in progress)

Every call but the positive controls is refused by host validation: nothing is launched, env.x, env.obs_soa, env.p_unc and
every pre-filled output buffer stay as they were.  B = 64, T = 2, cstr plans under RK4; the plans are made once.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import scenarios as SC
from helpers import _launch_names, _make, _torch, make_policy
from test_gpu_unc_rollout import _params as _unc_plan

pytestmark = pytest.mark.gpu

B, T = 64, 2
FILL, FILL_U8 = -7.0, 7
GOOD = "good"
KINDS = {"base": "", "cons": "_cons", "unc": "_unc"}


def _closed_loop_launches(lib):
    return [n for n in _launch_names(lib) if "rollout_" in n and ("policy_kernel" in n or "actor_kernel" in n)]


class Plan:
    """one env after its reset, pre-filled output buffers of its sizes, and the networks of its sizes: good ones and one per defect"""

    def __init__(self, params):
        torch = _torch()
        from pcgym_amd import MLPPolicy

        self.env = env = _make(params, B, seed=2)
        env.reset()
        s = self.spec = env.spec
        dev = env.device
        shapes = {"a": (T + 1, s.na, B), "u": (T + 1, s.na, B), "logp": (T + 1, B), "val": (T + 1, B), "obs": (T, s.nobs, B),
                  "rew": (T, B), "g": (T, max(s.ncon, 1), B)}
        self.bufs = {n: torch.full(shp, FILL, dtype=torch.float64, device=dev) for n, shp in shapes.items()}
        self.bufs["viol"] = torch.full((T, B), FILL_U8, dtype=torch.uint8, device=dev)
        self.kept = {"x": env.x, "obs_soa": env.obs_soa}
        if env.p_unc is not None:
            self.kept["p_unc"] = env.p_unc
        self.saved = {n: t.clone() for n, t in self.kept.items()}
        obs0 = env.obs_soa.cpu().numpy()
        pol = make_policy(s, obs0, (16,), seed=3)
        c = make_policy(s, obs0, (16,), seed=103)
        cw, cb = c.weights[:-1] + [c.weights[-1][:1]], c.biases[:-1] + [c.biases[-1][:1]]
        c.close()
        big = s.nobs + 5  # (an input size that no plan here has)
        self.nets = {
            "pol": pol,
            "cr": MLPPolicy(cw, cb, out_map="none"),
            "pol32": MLPPolicy(pol.weights, pol.biases, out_map=pol.out_map, out_low=pol.out_low, out_high=pol.out_high, dtype="float32"),
            "cr32": MLPPolicy(cw, cb, out_map="none", dtype="float32"),
            "wrong": MLPPolicy([np.zeros((s.na, big))], [np.zeros(s.na)]),
            "wrong32": MLPPolicy([np.zeros((s.na, big))], [np.zeros(s.na)], dtype="float32"),
            "wrong_cr": MLPPolicy([np.zeros((1, big))], [np.zeros(1)], out_map="none"),
            "wrong_cr32": MLPPolicy([np.zeros((1, big))], [np.zeros(1)], out_map="none", dtype="float32"),
            "wrong_clip_cr": MLPPolicy([np.zeros((1, big))], [np.zeros(1)], out_map="clip"),
            "clip_cr": MLPPolicy(cw, cb, out_map="clip"),
            "tanh": MLPPolicy(pol.weights, pol.biases, out_map="tanh"),
        }

    def handle(self, net, good):
        net = good if net is GOOD else net
        net = self.nets[net] if isinstance(net, str) else net
        return net.handle(self.env.device) if hasattr(net, "handle") else net  # (None and a junk pointer pass as they are)

    def restore(self):
        for n, t in self.kept.items():
            t.copy_(self.saved[n])
        for n, b in self.bufs.items():
            b.fill_(FILL_U8 if n == "viol" else FILL)
        _torch().cuda.synchronize()
        self.env._lib.pcg_coverage_names(None, 0, 1)

    def untouched(self, what):
        assert not _closed_loop_launches(self.env._lib), f"{what}: a refused call launched a closed-loop kernel"
        for n, t in self.kept.items():
            assert _torch().equal(t, self.saved[n]), f"{what}: a refused call wrote env.{n}"
        for n, b in self.bufs.items():
            assert bool((b == (FILL_U8 if n == "viol" else FILL)).all()), f"{what}: a refused call wrote the {n} buffer"

    def close(self):
        self.env.close()
        for q in self.nets.values():
            q.close()


@pytest.fixture(scope="module")
def plans():
    sc = SC.scenarios()
    params = {"base": copy.deepcopy(sc["cstr_canonical"]["env_params"]), "cons": copy.deepcopy(sc["cstr_cons_pen_norm"]["env_params"]),
              "unc": _unc_plan("cstr"),
              # a plan with run-time compiled code: the cstr with a reward expression (tests/test_gpu_closed_loop_jit.py)
              "jit": copy.deepcopy(sc["cstr_expr_reward_q3"]["env_params"])}
    for k in ("constraints", "done_on_cons_vio", "r_penalty"):
        params["jit"].pop(k, None)
    for p in params.values():
        p.update(integrator="rk4")
    out = {k: Plan(p) for k, p in params.items()}
    s = {k: q.spec for k, q in out.items()}
    assert not s["base"].ncon and not s["base"].nunc and s["base"].user_reward_src is None
    assert s["cons"].ncon > 0 and not s["cons"].nunc and s["unc"].nunc > 0 and not s["unc"].ncon
    assert s["jit"].user_reward_src and not s["jit"].ncon and not s["jit"].nunc
    assert all(not q.a_delta for q in s.values())  # (stage 12's a_save / u_prev clauses: not on these plans)
    yield out
    for q in out.values():
        q.close()


def _call(kind, head, plan, pol=GOOD, critic=GOOD, sigma=0.25, T=T, a_cs=B, g_cs=B, io=None):
    """one call of the entry point on `plan`; `io`: fields of a copy of the env's buffer struct to overwrite"""
    from pcgym_amd import _abi as abi

    env, s, b = plan.env, plan.spec, plan.bufs
    bufp = env._bufp
    if io:
        buf = abi.pcg_buffers.from_buffer_copy(env._buf)
        for field, value in io.items():
            setattr(buf, field, value)
        bufp = C.byref(buf)
    args = [env._plan, bufp, plan.handle(pol, "pol")]
    if head == "actor":
        args += [plan.handle(critic, "cr"), None if sigma is None else (C.c_double * s.na)(*[sigma] * s.na)]
    args += [0, T, b["a"].data_ptr(), s.na * B, a_cs]
    if head == "actor":
        args += [b["u"].data_ptr(), s.na * B, B, b["logp"].data_ptr(), B, b["val"].data_ptr(), B]
    args += [b["obs"].data_ptr(), s.nobs * B, B, b["rew"].data_ptr(), B, 1]
    if kind == "cons":
        args += [b["g"].data_ptr(), max(s.ncon, 1) * B, g_cs, b["viol"].data_ptr(), B]
    rc = getattr(env._lib, f"pcg_rollout_{head}{KINDS[kind]}")(*args, 1, None)
    _torch().cuda.synchronize()
    return rc


@pytest.mark.parametrize("head", ["policy", "actor"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_the_earlier_stage_decides(plans, kind, head):
    torch = _torch()
    from pcgym_amd import _abi as abi

    OK, UNS, DIM, VAL, NUL, PLAN = abi.PCG_OK, abi.PCG_E_UNSUPPORTED, abi.PCG_E_DIM, abi.PCG_E_VALUE, abi.PCG_E_NULL, abi.PCG_E_PLAN
    own, other, jit = plans[kind], plans["cons" if kind == "base" else "base"], plans["jit"]  # `other`: a plan the kind does not carry
    actor = head == "actor"
    junk = C.cast(C.create_string_buffer(512), C.c_void_p)

    def one(what, want, plan=own, **kw):
        rc = _call(kind, head, plan, **kw)
        assert rc == want, f"{kind} {head}, {what}: status {rc}, not {want}"
        plan.untouched(f"{kind} {head}, {what}")

    def pair(what, want, both, want_later, later):
        """both defects -> the earlier stage's status; the later stage's defect alone -> its own, which is another"""
        assert want != want_later
        one(what, want, **both)
        one(what + " (the later defect alone)", want_later, **later)

    for q in (own, other, jit):
        q.restore()

    # ---- positive control: the valid call runs this entry's kernels and writes every buffer ----
    assert _call(kind, head, own) == OK
    family = f"rollout_{'' if kind == 'base' else kind + '_'}{head}_kernel"
    names = _closed_loop_launches(own.env._lib)
    assert names and all(family in n for n in names), (family, names)
    assert not torch.equal(own.env.x, own.saved["x"]) and not torch.equal(own.env.obs_soa, own.saved["obs_soa"])
    if kind == "unc":
        assert torch.equal(own.env.p_unc, own.saved["p_unc"])  # (read, never written)
    written = {"a", "obs", "rew"} | ({"u", "logp", "val"} if actor else set()) | ({"g", "viol"} if kind == "cons" else set())
    for n, b in own.bufs.items():
        fill = FILL_U8 if n == "viol" else FILL
        assert bool((b != fill).all()) if n in written else bool((b == fill).all()), f"the valid call and the {n} buffer"
    own.restore()

    # ---- adjacent stages (the docstring's numbers) ----
    no_rew, short = {"rew": None}, B - 1
    pair("1 | 2: negative batch size, no policy", DIM, dict(io={"B": -1}, pol=None), NUL, dict(pol=None))
    pair("3 | 4: junk policy handle on a plan of another kind", PLAN, dict(plan=other, pol=junk), UNS, dict(plan=other))
    pair("4 | 6: wrong-size policy on a plan of another kind", UNS, dict(plan=other, pol="wrong"), DIM, dict(pol="wrong"))
    if kind != "base":
        pair("4 | 6: float32 policy of the wrong size", UNS, dict(pol="wrong32"), DIM, dict(pol="wrong"))
    if not actor:
        pair("6 | 10: wrong-size policy, T = 0", DIM, dict(pol="wrong", T=0), VAL, dict(T=0))
    else:
        pair("6 | 7: wrong-size actor, junk critic handle", DIM, dict(pol="wrong", critic=junk), PLAN, dict(critic=junk))
        if kind != "base":
            # the one line in which the three actor forms differ: a float32 critic is refused before its sizes are looked at
            one("7: float32 critic, float64 actor", UNS, critic="cr32")
            pair("7: float32 critic of the wrong size", UNS, dict(critic="wrong_cr32"), DIM, dict(critic="wrong_cr"))
        else:
            # (the base form takes float32 networks: the critic's sizes are looked at, its dtype after every other check)
            pair("7 | 15: float32 critic of the wrong size, float64 actor", DIM, dict(critic="wrong_cr32"), UNS, dict(critic="cr32"))
        pair("7: clip-mapped critic of the wrong size", DIM, dict(critic="wrong_clip_cr"), VAL, dict(critic="clip_cr"))
        pair("7 | 8: clip-mapped critic, tanh-mapped actor", VAL, dict(critic="clip_cr", pol="tanh"), UNS, dict(pol="tanh"))
        pair("8 | 9: tanh-mapped actor, no sigma", UNS, dict(pol="tanh", sigma=None), NUL, dict(sigma=None))
        pair("9 | 10: no sigma, T = 0", NUL, dict(sigma=None, T=0), VAL, dict(T=0))
        pair("9 | 12: negative sigma, io->rew null", VAL, dict(sigma=-0.25, io=no_rew), NUL, dict(io=no_rew))
    pair("10 | 11: T = 0, empty batch", VAL, dict(T=0, io={"B": 0}), OK, dict(io={"B": 0}))
    pair("10 | 12: T = 0, io->rew null", VAL, dict(T=0, io=no_rew), NUL, dict(io=no_rew))
    one("11 | 12: empty batch, io->rew null", OK, io={"B": 0, "rew": None})
    pair("12 | 13: io->rew null, action component stride B - 1", NUL, dict(io=no_rew, a_cs=short), DIM, dict(a_cs=short))
    if kind == "unc":
        pair("12 | 13: io->p_unc null, action component stride B - 1", NUL, dict(io={"p_unc": None}, a_cs=short), DIM, dict(a_cs=short))
    if kind == "cons":
        pair("12 | 14: io->rew null, row component stride B - 1", NUL, dict(io=no_rew, g_cs=short), DIM, dict(g_cs=short))
    if kind == "base":
        if actor:
            pair("13 | 15: action component stride B - 1, actor and critic of two dtypes", DIM, dict(a_cs=short, critic="cr32"),
                 UNS, dict(critic="cr32"))
        f32 = dict(plan=jit, pol="pol32", critic="cr32")
        pair("13 | 15: action component stride B - 1, float32 on a run-time compiled plan", DIM, dict(a_cs=short, **f32), UNS, f32)
