// pcg_lean.hpp -- the lean, lock-stepped hot path (BASELINE configs[1]): env_step_lean, the tile I/O layer its kernels
// and the feature-masked sibling (pcg_step_feat.hpp) share, and the three kernels step_kernel_stream, step_kernel_pipe
// and rollout_kernel_lean.  Included by pcg_kernels.hpp, which defines what this header builds on (StepArgs, DevConst,
// LeanStep, the Philox draws, action_map, RhsFn).
//
// Streaming variant for the lean, lock-stepped hot path:
//   * persistent grid (all workgroups resident), grid-stride over tiles of 256*EPL envs;
//   * EPL = 2 environments per lane -> every global access is 16 B per lane (dwordx4),
//     1 KiB contiguous per wave-instruction, and the two envs give the VALU two
//     independent dependency chains through exp/div;
//   * the loads of tile i+1 are issued before tile i is integrated, so each wave has HBM
//     reads in flight while it computes, and waves drift out of phase instead of
//     alternating chip-wide "all load / all compute / all store" rounds.
// Preconditions (checked on the host): no per-env t, no extras, no a_delta, no per-env d,
// B % EPL == 0 and 16-byte aligned rows when EPL == 2.
#pragma once

namespace pcg {

// ---------------------------------------------------------------------------
// Lean env step for W envs per lane (Pack<W>): the hot path of BASELINE configs[1].
// Same statements as env_step with everything the lean plan cannot contain removed (a_delta,
// per-env / Gaussian disturbances, noise, constraints, terminal reward); the lock-stepped batch makes
// the SP / disturbance slots, `done` and all schedule values wave-uniform scalars.
// ---------------------------------------------------------------------------
template <int NX, int W>
PCG_DEV Pack<W> pick(const Pack<W> (&v)[NX], int idx) {
  Pack<W> r(0.0);
#pragma unroll
  for (int i = 0; i < NX; ++i)
#pragma unroll
    for (int j = 0; j < W; ++j) r.v[j] = (i == idx) ? v[i].v[j] : r.v[j];
  return r;
}

// One set-point's term of the reward, r + (-(dd dd)) r_scale with dd = x[idx] - spn, for a wave-uniform idx within [0, NX)
// (build_devconst refuses any other): the row is chosen by scalar branches, one arm taken and the last one without a test,
// where pick() spends 2 W selects per state on the vector unit.  No arm writes r ahead of its branch.
template <int NX, int W, int I = 0>
PCG_DEV void reward_row(const Pack<W> (&x)[NX], int idx, double spn, double r_scale, Pack<W>& r) {
  if (I == NX - 1 || idx == I) {
    const Pack<W> dd = x[I] - spn;
    r = r + (-(dd * dd)) * r_scale;
    asm volatile("");  // keep it a (scalar) branch
  } else {
    if constexpr (I + 1 < NX) reward_row<NX, W, I + 1>(x, idx, spn, r_scale, r);
  }
}

template <class M, int W>
struct LeanOut {
  Pack<W> ox[M::NX];
  Pack<W> rew;
  bool done;                // wave-uniform
};

// INTEG: PCG_INT_RK4 (the lean kernels' scheme) or PCG_INT_CV8.  (A guarded scheme with the adaptive fallback inside this
// kernel was built and measured: 41.3 us against 37 us in the general kernel on the canonical cstr loop -- the fallback's
// registers leave one env per lane at four waves per SIMD -- and 26 % slower when half the batch escalates, because a
// 256-thread workgroup then waits for its slowest env.)
// Round 4: the kernel's time follows its vector-instruction count (profiles/r4/headline_bisect.txt: +8 % instructions,
// +9 % time), so everything wave-uniform is gone from the vector unit -- the SP / disturbance slots of step t come
// finished from the host (LeanStep, scalar loads), h/2 and h/6 too, and the normalised-action branch is a scalar branch
// instead of both values and a select.
// Round 23 took what was left of it (profiles/r23/lean_trim.txt): the set-point's state row is chosen by a scalar branch, the
// action box's half width comes from the host, and the action map is a function of its own, lean_input, so that the chained
// kernel can apply it where the action rows land.  step_chain_kernel<cstr,2> executes 324.8 vector instructions per wave
// and step (SQ_INSTS_VALU; 344.8 before), 306 of them in the RK4 stage loop.  PCG_LEAN_TRIM (bits, for the A/B builds of
// that profile) switches each back: 1 the reward row, 2 the action map, 4 step_chain_kernel's action hand-over, 8 the
// uniform store flags.
#ifndef PCG_LEAN_TRIM
#define PCG_LEAN_TRIM 15
#endif

// physical action u[0..NA) of the lean step (pcgym.py:371-375): DevConst::a_mode says how, one scalar branch
template <class M, int W>
PCG_DEV void lean_input(CDevConst& c, const Pack<W> (&a_in)[M::NA], Pack<W> (&u)[M::NA]) {
#pragma clang fp contract(off)
  constexpr int NA = M::NA;
  const int na = M::DYNAMIC ? c.na : NA;
#if PCG_LEAN_TRIM & 2
  int32_t mode = c.a_mode;
  asm volatile("" : "+s"(mode));  // one scalar register, and every arm writes u itself: scalar branches, no copy ahead of them
  if (mode == PCG_AMAP_FOLDED) {
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
      for (int j = 0; j < W; ++j) u[i].v[j] = (i < na) ? (a_in[i].v[j] + 1.0) * c.a_w[i] + c.a_lo[i] : 0.0;
    asm volatile("");  // keep it a (scalar) branch
  } else if (mode == PCG_AMAP_EXACT) {
#else
  if (c.flags & PCG_F_NORMALISE_A) {
#endif
#pragma unroll
    for (int i = 0; i < NA; ++i) u[i] = (i < na) ? action_map(a_in[i], c.a_lo[i], c.a_hi[i], true, false) : Pack<W>(0.0);
    asm volatile("");  // keep it a (scalar) branch
  } else {
#pragma unroll
    for (int i = 0; i < NA; ++i) u[i] = (i < na) ? a_in[i] : Pack<W>(0.0);
    asm volatile("");
  }
}

// the step from the physical action on
template <class M, int W, int INTEG = PCG_INT_RK4>
PCG_DEV void env_step_lean_u(const StepArgs& A, CDevConst& c, const PCG_CONSTANT LeanStep& L, int t,
                             const Pack<W> (&ua)[M::NA], Pack<W> (&x)[M::NX], LeanOut<M, W>& out) {
  constexpr int NX = M::NX, NA = M::NA, NDM = M::NDM;
  using R = Pack<W>;
  const int nx = M::DYNAMIC ? c.nx : NX;
  const int N = c.N, nsp = c.nsp;
  typename M::CKP& kp = model_kp<M>(c);
  // the action and the held disturbance inputs (pcgym.py:386-404)
  R u[NA + NDM];
#pragma unroll
  for (int i = 0; i < NA; ++i) u[i] = ua[i];
#pragma unroll
  for (int j = 0; j < NDM; ++j) u[NA + j] = R(L.ud[j]);
  // integrate over [0,dt] with the input held (integrator.py:163-182)
  const typename M::template HoldT<R> hold = M::template hold<R>(kp, u);
  const RhsFn<M, R> f{kp, hold};
  if constexpr (INTEG == PCG_INT_CV8) {
    cv8<NX>(f, x, c.h, c.substeps);
  } else {
    rk4<NX>(f, x, c.h, c.h2, c.h6, c.substeps);
  }
  // reward against SP[t_new] (pcgym.py:535-558)
  R r(0.0);
#pragma unroll
  for (int k = 0; k < PCG_MAX_NSP; ++k)
    if (k < nsp) {
#if PCG_LEAN_TRIM & 1
      int32_t idx = c.sp_index[k];
      asm volatile("" : "+s"(idx));
      reward_row<NX, W>(x, idx, L.spn[k], c.r_scale[k], r);
#else
      const R dd = pick<NX, W>(x, c.sp_index[k]) - L.spn[k];
      r = r + (-(dd * dd)) * c.r_scale[k];
#endif
    }
  out.rew = r;
  out.done = (t + 1 == N - 1);  // pcgym.py:448-449
#pragma unroll
  for (int i = 0; i < NX; ++i)
    if (i < nx) out.ox[i] = (x[i] - c.omap[i].lo) * c.omap[i].sc + c.omap[i].off;
}

template <class M, int W, int INTEG = PCG_INT_RK4>
PCG_DEV void env_step_lean(const StepArgs& A, CDevConst& c, const PCG_CONSTANT LeanStep& L, int t,
                           const Pack<W> (&a_in)[M::NA], Pack<W> (&x)[M::NX], LeanOut<M, W>& out) {
  Pack<W> ua[M::NA];
  lean_input<M, W>(c, a_in, ua);
  env_step_lean_u<M, W, INTEG>(A, c, L, t, ua, x, out);
}

template <int EPL>
struct Vec;
template <>
struct Vec<1> {
  using T = double;
  PCG_DEV static double get(const T& v, int) { return v; }
  PCG_DEV static T make(const double (&s)[1]) { return s[0]; }
  // streaming store: the data is not re-read by this kernel (obs / reward go to the policy)
  PCG_DEV static void store_nt(double* p, const double (&s)[1]) { __builtin_nontemporal_store(s[0], p); }
  PCG_DEV static T load_nt(const double* p) { return __builtin_nontemporal_load(p); }
};
template <>
struct Vec<2> {
  using T = double2;
  typedef double d2 __attribute__((ext_vector_type(2)));
  PCG_DEV static double get(const T& v, int j) { return j ? v.y : v.x; }
  PCG_DEV static T make(const double (&s)[2]) { return make_double2(s[0], s[1]); }
  PCG_DEV static void store_nt(double* p, const double (&s)[2]) {
    __builtin_nontemporal_store(d2{s[0], s[1]}, reinterpret_cast<d2*>(p));
  }
  PCG_DEV static T load_nt(const double* p) {
    const d2 v = __builtin_nontemporal_load(reinterpret_cast<const d2*>(p));
    return make_double2(v.x, v.y);
  }
};

PCG_DEV void land(double& v) { asm volatile("" : "+v"(v)); }
PCG_DEV void land(double2& v) {
  asm volatile("" : "+v"(v.x));
  asm volatile("" : "+v"(v.y));
}

// ---------------------------------------------------------------------------
// Tile I/O of the lean kernels: where a lane's EPL consecutive envs sit within a row, the
// row stores of an observation, the flag bytes, the unpacking of loaded rows and the per-env health check.
// ---------------------------------------------------------------------------
// Rows are addressed as (uniform row base) + (32-bit byte offset of the lane): the row bases stay in scalar registers and the
// lane's offset is ONE vector register for every row (the 64-bit per-row addresses of rounds 1-3 were two dozen vector
// instructions per tile).  Callers guarantee B < 2^28.
template <class T>
PCG_DEV T* row_at(double* base, uint32_t off8) {
  return reinterpret_cast<T*>(reinterpret_cast<char*>(base) + off8);
}
template <class T>
PCG_DEV const T* row_at(const double* base, uint32_t off8) {
  return reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + off8);
}
// the two ways a lane finds its envs in a row: that byte offset (step_kernel_pipe, step_kernel_stream), or a 64-bit env index
struct LaneOff8 {
  uint32_t off8;
  PCG_DEV double* operator()(double* row) const { return row_at<double>(row, off8); }
};
struct LaneIdx {
  int64_t e0;
  PCG_DEV double* operator()(double* row) const { return row + e0; }
};

// the EPL values of a lane into one row (16 bytes when EPL == 2), non-temporal on request
template <int EPL>
PCG_DEV void put(double* p, const double (&v)[EPL], bool nt) {
  // A flag that is not a constant goes through a scalar register first, so that each store tests a word of its own.  One
  // boolean shared by the stores of a tile lives as a lane mask, and the branches between them had the compiler rebuild its
  // negation on the vector unit (v_cndmask_b32 0, 1 + v_cmp_ne_u32, six pairs in step_chain_kernel<cstr,2>).
#if PCG_LEAN_TRIM & 8
  if (!__builtin_constant_p(nt)) {
    int32_t w = nt;
    asm volatile("" : "+s"(w));
    nt = w != 0;
  }
#endif
  if (nt) Vec<EPL>::store_nt(p, v);
  else *reinterpret_cast<typename Vec<EPL>::T*>(p) = Vec<EPL>::make(v);
}
// ... one wave-uniform value for all of them: it arrives as a scalar, never through a per-lane array
template <int EPL>
PCG_DEV void put_uniform(double* p, double s, bool nt) {
  double tmp[EPL];
#pragma unroll
  for (int j = 0; j < EPL; ++j) tmp[j] = s;
  put<EPL>(p, tmp, nt);
}

// rows [component][env] of one destination: row base, row stride in doubles, non-temporal stores
struct Rows {
  double* base;
  size_t stride;
  bool nt;
};
// The rows of one observation, in the order every kernel of the family writes them: ox[0..nx), then the set-point slots
// osp[0..nso) and the disturbance slots od[0..nd), which are wave-uniform (LeanStep in constant memory, or scalars of the
// caller).  put_state_rows: the same with the state row xs[i] going back in place ahead of each ox[i]; `hold` (wave-uniform)
// leaves the slot rows as they are -- they already hold these values (StepArgs::held bit 0).
template <class M, int EPL, class Lane, class SP, class D>
PCG_DEV void put_slot_rows(const Rows obs, const Lane at, int nx, int nso, int nd, const SP& osp, const D& od) {
#pragma unroll
  for (int k = 0; k < PCG_MAX_NSP; ++k)
    if (k < nso) put_uniform<EPL>(at(obs.base + (size_t)(nx + k) * obs.stride), osp[k], obs.nt);
#pragma unroll
  for (int k = 0; k < M::NDM; ++k)
    if (k < nd) put_uniform<EPL>(at(obs.base + (size_t)(nx + nso + k) * obs.stride), od[k], obs.nt);
}
template <class M, int EPL, class Lane, class SP, class D>
PCG_DEV void put_obs_rows(const Rows obs, const Lane at, int nx, int nso, int nd, const Pack<EPL> (&ox)[M::NX], const SP& osp,
                          const D& od) {
#pragma unroll
  for (int i = 0; i < M::NX; ++i)
    if (i < nx) put<EPL>(at(obs.base + (size_t)i * obs.stride), ox[i].v, obs.nt);
  put_slot_rows<M, EPL>(obs, at, nx, nso, nd, osp, od);
}
// ... with `hold` as in put_state_rows (step_chain_kernel: every step of a chain but its last)
template <class M, int EPL, class Lane, class SP, class D>
PCG_DEV void put_obs_rows(const Rows obs, const Lane at, int nx, int nso, int nd, const Pack<EPL> (&ox)[M::NX], const SP& osp,
                          const D& od, bool hold) {
#pragma unroll
  for (int i = 0; i < M::NX; ++i)
    if (i < nx) put<EPL>(at(obs.base + (size_t)i * obs.stride), ox[i].v, obs.nt);
  if (!hold) {
    put_slot_rows<M, EPL>(obs, at, nx, nso, nd, osp, od);
    asm volatile("");  // keep it a (scalar) branch
  }
}
template <class M, int EPL, class Lane, class SP, class D>
PCG_DEV void put_state_rows(const Rows x, const Rows obs, const Lane at, int nx, int nso, int nd, const Pack<EPL> (&xs)[M::NX],
                            const Pack<EPL> (&ox)[M::NX], const SP& osp, const D& od, bool hold = false) {
#pragma unroll
  for (int i = 0; i < M::NX; ++i)
    if (i < nx) {
      put<EPL>(at(x.base + (size_t)i * x.stride), xs[i].v, x.nt);
      put<EPL>(at(obs.base + (size_t)i * obs.stride), ox[i].v, obs.nt);
    }
  if (!hold) {
    put_slot_rows<M, EPL>(obs, at, nx, nso, nd, osp, od);
    asm volatile("");  // keep it a (scalar) branch
  }
}

// the wave-uniform done flag of the lane's envs, EPL == 2 as one 2-byte store
template <int EPL>
PCG_DEV void put_done(uint8_t* p, bool done) {
  if (EPL == 2) *reinterpret_cast<uint16_t*>(p) = done ? (uint16_t)0x0101u : (uint16_t)0;
  else p[0] = done ? 1 : 0;
}

// loaded rows -> Pack<EPL> values, zero beyond the plan's n components
template <int N, int EPL>
PCG_DEV void unpack(const typename Vec<EPL>::T (&src)[N], int n, Pack<EPL> (&dst)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < EPL; ++j) dst[i].v[j] = (i < n) ? Vec<EPL>::get(src[i], j) : 0.0;
}

// per-env health: a fixed step cannot fail in the integrator, only leave a non-finite state
template <int NX, int W>
PCG_DEV bool nonfinite(const Pack<W> (&x)[NX], int j) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < NX; ++i) ok = ok && (__builtin_fabs(x[i].v[j]) < __builtin_inf());
  return !ok;
}
// ... into the sticky status bytes of the lane's envs e0, e0 + 1, ..: only failures are written
template <int NX, int W, class E>
PCG_DEV void flag_nonfinite(uint8_t* status, E e0, const Pack<W> (&x)[NX]) {
#pragma unroll
  for (int j = 0; j < W; ++j)
    if (nonfinite<NX, W>(x, j)) status[e0 + j] = PCG_ST_NONFINITE;
}

// stores of one lean tile: the state back in place, observation / reward (non-temporal on request), done flags.
// HOLD (step_kernel_pipe without the reset path): StepArgs::held names wave-uniform rows that the previous node of a step
// graph left with these very bytes and that are not stored again -- bit 0 the observation's slot rows, bit 1 the done flags.
// The word passes through an empty asm here, in the tile loop: its two tests then stay in the loop and the kernel carries
// ONE scalar register for them.  Hoisted, each outcome is a scalar pair of its own, and the headline kernel, one register
// short of the scalar file as it is, spilled four of them into a new vector register (58 -> 59).
template <class M, int EPL, bool HOLD = false>
PCG_DEV void store_lean(const StepArgs& A, CDevConst& c, const PCG_CONSTANT LeanStep& L, uint32_t e0,
                        const Pack<EPL> (&xs)[M::NX], const LeanOut<M, EPL>& out, bool nt) {
  const size_t B = (size_t)A.B;
  const int nx = M::DYNAMIC ? c.nx : M::NX;
  const LaneOff8 at{e0 * 8u};
  int32_t held = HOLD ? A.held : 0;
  if (HOLD) asm volatile("" : "+s"(held));
  put_state_rows<M, EPL>(Rows{A.x, B, (A.nt_stores & 2) != 0}, Rows{A.obs, B, nt}, at, nx, c.nsp_obs, c.nd, xs, out.ox,
                         L.osp, L.od, (held & 1) != 0);
  put<EPL>(at(A.rew), out.rew.v, nt);
  if (!(held & 2)) {
    put_done<EPL>(A.done + e0, out.done);
    asm volatile("");  // keep it a (scalar) branch
  }
}

// initial state of one env (pcgym.py:284-288, apply_uncertainties :255-261) and its observation rows: the draws of
// reset_env, kept in registers so that the caller can merge them into a vector store
template <class M>
PCG_DEV void reset_vals(const StepArgs& A, CDevConst& c, int nx, uint64_t env_id, uint64_t seed, double (&xv)[M::NX],
                        double (&ov)[M::NX]) {
#pragma unroll
  for (int i = 0; i < M::NX; ++i) {
    double v = (i < nx) ? c.x0[i] : 0.0;
    if (i < nx && c.has_x0_unc && c.x0_unc[i] != 0.0) {
      const double pct = c.x0_unc[i];
      if (c.flags & PCG_F_X0_NORMAL) {
        double z0, z1;
        rng_normal2(seed, env_id, 0u, RNG_RESET + (uint32_t)(i >> 1), z0, z1);
        v = c.x0[i] + pct * c.x0[i] * ((i & 1) ? z1 : z0);
      } else {
        double u0, u1;
        rng_uniform2(seed, env_id, 0u, RNG_RESET + (uint32_t)(i >> 1), u0, u1);
        v = c.x0[i] * (1 + pct * (2.0 * ((i & 1) ? u1 : u0) - 1.0));
      }
    }
    xv[i] = v;
    ov[i] = (v - c.omap[i].lo) * c.omap[i].sc + c.omap[i].off;
  }
}

// reset of the EPL consecutive envs of one lean lane (lock-stepped batch, no per-env parameters / a_delta: those
// configurations never reach the lean kernels): the draws of reset_vals, stored 16 bytes per lane and row
template <class M, int EPL>
PCG_DEV void reset_lean(const StepArgs& A, CDevConst& c, int64_t e0, uint64_t seed, bool nt) {
  constexpr int NX = M::NX, ND = M::NDM > 0 ? M::NDM : 1;
  const int nx = M::DYNAMIC ? c.nx : NX;
  Pack<EPL> xs[NX], ox[NX];
#pragma unroll
  for (int j = 0; j < EPL; ++j) {
    double xv[NX], ov[NX];
    reset_vals<M>(A, c, nx, (uint64_t)(A.env_offset + e0 + j), seed, xv, ov);
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      xs[i].v[j] = xv[i];
      ox[i].v[j] = ov[i];
    }
  }
  // the SP / disturbance slots of a reset observation (pcgym.py:291-298, quirk Q6: disturbances[k][0]): wave-uniform
  const int nso = c.nsp_obs, nd = c.nd;
  double osp[PCG_MAX_NSP], od[ND];
#pragma unroll
  for (int k = 0; k < PCG_MAX_NSP; ++k)
    if (k < nso) osp[k] = (c.x0[nx + k] - c.omap[nx + k].lo) * c.omap[nx + k].sc + c.omap[nx + k].off;
#pragma unroll
  for (int k = 0; k < M::NDM; ++k)
    if (k < nd) {
      const int q = nx + nso + k;
      od[k] = (A.sched[(size_t)(c.nsp + k) * c.N] - c.omap[q].lo) * c.omap[q].sc + c.omap[q].off;
    }
  const size_t B = (size_t)A.B;
  put_state_rows<M, EPL>(Rows{A.x, B, false}, Rows{A.obs, B, nt}, LaneIdx{e0}, nx, nso, nd, xs, ox, osp, od);
}

template <class M, int INTEG, int EPL, int UNR>
__global__ __launch_bounds__(BLOCK, (PCG_LEAN_WPE > wpe(M::NX, INTEG, false) ? PCG_LEAN_WPE : wpe(M::NX, INTEG, false)))
void step_kernel_stream(const StepArgs A) {
  static_assert(INTEG == PCG_INT_RK4, "only <M, PCG_INT_RK4, {1, 2}, 1> is instantiated (make_kernels: k.stream)");
  // One workgroup = UNR sub-tiles of 256*EPL envs.  All UNR sub-tiles' inputs are requested up front
  // (UNR * (NX+NA) loads in flight per lane), then the sub-tiles are integrated and stored one after
  // the other: the memory system works on sub-tile u+1.. while the VALU integrates sub-tile u, and
  // results leave as soon as each sub-tile is done instead of in one burst per wave.
  CDevConst& c = *A.C;
  constexpr int NX = M::NX, NA = M::NA;
  using V = typename Vec<EPL>::T;
  const int64_t B = A.B;
  const int nx = M::DYNAMIC ? c.nx : NX;
  const int na = M::DYNAMIC ? c.na : NA;
  const int t = A.t_scalar;
  const bool nt = (A.nt_stores & 1) != 0;
  constexpr int64_t SUB = (int64_t)BLOCK * EPL;  // envs per sub-tile
  const int64_t tile = SUB * UNR;
  const int64_t ntile = (B + tile - 1) / tile;
  for (int64_t it = blockIdx.x; it < ntile; it += gridDim.x) {
    V xv[UNR][NX], av[UNR][NA];
    bool live[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int64_t e0 = it * tile + u * SUB + (int64_t)threadIdx.x * EPL;
      live[u] = e0 < B;
      if (live[u]) {
#pragma unroll
        for (int i = 0; i < NX; ++i)
          if (i < nx) xv[u][i] = *reinterpret_cast<const V*>(A.x + (size_t)i * B + e0);
#pragma unroll
        for (int i = 0; i < NA; ++i)
          if (i < na) av[u][i] = *reinterpret_cast<const V*>(A.a + (size_t)i * B + e0);
      }
    }
    // Land ALL inputs here, while only loads are outstanding.  gfx9-class hardware counts loads and
    // stores in one counter (vmcnt) and lets the two kinds complete out of order, so once a store is
    // pending the compiler can only wait with vmcnt(0) -- i.e. every later "wait for my input" would
    // also wait for the previous sub-tile's stores to be acknowledged (microseconds under load).
    // Passing the loaded registers through an empty asm makes this the single wait of the tile:
    // after it, the sub-tiles are integrated and stored back-to-back and no store is ever waited for.
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
#pragma unroll
      for (int i = 0; i < NX; ++i) land(xv[u][i]);
#pragma unroll
      for (int i = 0; i < NA; ++i) land(av[u][i]);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int64_t e0 = it * tile + u * SUB + (int64_t)threadIdx.x * EPL;
      if (!live[u]) continue;
      // W = EPL envs advance together through one instruction stream (independent chains -> ILP)
      Pack<EPL> xs[NX], as[NA];
      unpack<NX, EPL>(xv[u], nx, xs);
      unpack<NA, EPL>(av[u], na, as);
      LeanOut<M, EPL> out;
      env_step_lean<M, EPL>(A, c, A.lean[min(t, c.N - 1)], t, as, xs, out);
      store_lean<M, EPL>(A, c, A.lean[min(t, c.N - 1)], (uint32_t)e0, xs, out, nt);
    }
  }
}

// ---------------------------------------------------------------------------
// Software-pipelined persistent variant of the lean kernel (PCG_OPT_VARIANT 4): each wave walks
// over its tiles and always has the NEXT tile's inputs in flight while it integrates the current one.
//   loop:  land(cur)            -- the only wait: cur's loads (issued one iteration ago) + previous stores
//          issue loads(next)
//          integrate(cur)       -- no memory operation inside the lean step
//          issue stores(cur)    -- never waited for explicitly
// The `land` placement matters: loads and stores share one in-order-per-kind counter (vmcnt), so the
// compiler can only wait with vmcnt(0) once stores are pending; waiting BEFORE the prefetch is issued
// keeps the prefetch out of that wait.
// ---------------------------------------------------------------------------
// AR: the instantiation launched for the LAST step of a lock-stepped episode with same-launch auto-reset
// (pcg_step_autoreset).  It is a separate instantiation because the inlined reset path (Philox draws for the x0 /
// parameter uncertainty) raises the register count of the whole kernel from 75 to 118 (6 -> 4 waves per SIMD);
// the other N-2 steps of the episode run the lean one.
template <class M, int EPL, bool AR = false, int INTEG = PCG_INT_RK4>
__global__ __launch_bounds__(BLOCK, INTEG == PCG_INT_RK4 ? PCG_LEAN_WPE : 4) void step_kernel_pipe(const StepArgs A) {
  CDevConst& c = *A.C;
  constexpr int NX = M::NX, NA = M::NA;
  using V = typename Vec<EPL>::T;
  const uint32_t B = (uint32_t)A.B;  // < 2^28 (step_impl): 32-bit env indices and byte offsets, row bases in scalar registers
  const size_t Bs = (size_t)A.B;
  const int nx = M::DYNAMIC ? c.nx : NX;
  const int na = M::DYNAMIC ? c.na : NA;
  const int t = A.t_scalar;
  const PCG_CONSTANT LeanStep& L = A.lean[min(t, c.N - 1)];
  const bool nt = (A.nt_stores & 1) != 0;
  const bool ntl = (A.nt_stores & 4) != 0;
  constexpr uint32_t TILE = (uint32_t)BLOCK * EPL;
  const uint32_t ntile = (B + TILE - 1) / TILE;
  uint32_t it = blockIdx.x;
  if (it >= ntile) return;
  V xv[NX], av[NA];
  uint32_t e0 = it * TILE + threadIdx.x * EPL;
  bool live = e0 < B;
  auto load = [&](uint32_t ee, V (&xd)[NX], V (&ad)[NA]) {
    const uint32_t o8 = ee * 8u;
    if (ntl) {
#pragma unroll
      for (int i = 0; i < NX; ++i)
        if (i < nx) xd[i] = Vec<EPL>::load_nt(row_at<double>(A.x + (size_t)i * Bs, o8));
#pragma unroll
      for (int i = 0; i < NA; ++i)
        if (i < na) ad[i] = Vec<EPL>::load_nt(row_at<double>(A.a + (size_t)i * Bs, o8));
    } else {
#pragma unroll
      for (int i = 0; i < NX; ++i)
        if (i < nx) xd[i] = *row_at<V>(A.x + (size_t)i * Bs, o8);
#pragma unroll
      for (int i = 0; i < NA; ++i)
        if (i < na) ad[i] = *row_at<V>(A.a + (size_t)i * Bs, o8);
    }
  };
#ifdef PCG_TIMELINE  // measurement build (tools/timeline_probe.py): per-wave stamps of the 100 MHz wall clock into A.g
  int tl_it = 0;
#define PCG_TL(k)                                                                                              \
  if ((threadIdx.x & 63) == 0 && A.g)                                                                          \
  reinterpret_cast<unsigned long long*>(A.g)[((size_t)(blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + tl_it) * 8 + (k)] = \
      wall_clock64()
#else
#define PCG_TL(k)
#endif
  PCG_TL(0);
  if (live) load(e0, xv, av);
  for (;;) {
#pragma unroll
    for (int i = 0; i < NX; ++i) land(xv[i]);
#pragma unroll
    for (int i = 0; i < NA; ++i) land(av[i]);
    PCG_TL(1);
    const uint32_t itn = it + gridDim.x;
    const uint32_t e1 = itn * TILE + threadIdx.x * EPL;
    const bool live_n = (itn < ntile) && (e1 < B);
    V xn[NX], an[NA];
    asm volatile("" ::: "memory");
    if (live_n) load(e1, xn, an);
    asm volatile("" ::: "memory");
    if (live) {
      Pack<EPL> xs[NX], as[NA];
      unpack<NX, EPL>(xv, nx, xs);
      unpack<NA, EPL>(av, na, as);
      LeanOut<M, EPL> out;
      env_step_lean<M, EPL, INTEG>(A, c, L, t, as, xs, out);
      PCG_TL(2);
      if (A.status) flag_nonfinite<NX, EPL>(A.status, e0, xs);
      if (AR && A.auto_reset && out.done) {
        // last step of a lock-stepped episode with same-launch auto-reset: reward / done of the finished step,
        // then the new episode's state and observation instead of the terminal ones (pcg_step_autoreset)
        put<EPL>(A.rew + e0, out.rew.v, nt);
        put_done<EPL>(A.done + e0, true);
        reset_lean<M, EPL>(A, c, (int64_t)e0, A.reset_seed, nt);
      } else {
        store_lean<M, EPL, !AR>(A, c, L, e0, xs, out, nt);  // (the auto-reset instantiation stores everything)
      }
    }
    PCG_TL(3);
#ifdef PCG_TIMELINE
    if (itn >= ntile) {
      __builtin_amdgcn_s_waitcnt(0);  // all stores of this wave acknowledged
      PCG_TL(4);
    }
    tl_it = 1;
#endif
    if (itn >= ntile) break;
    it = itn;
    e0 = e1;
    live = live_n;
#pragma unroll
    for (int i = 0; i < NX; ++i) xv[i] = xn[i];
#pragma unroll
    for (int i = 0; i < NA; ++i) av[i] = an[i];
  }
}

// ---------------------------------------------------------------------------
// A run of consecutive step_kernel_pipe nodes of a recorded step graph as ONE launch (pcg_graph_create): A.T steps from
// t = A.t_scalar on one tile of BLOCK * EPL envs per workgroup, the state in registers from the first load to the last
// store.  Tile i of step j + 1 depends on tile i of step j alone, and nothing outside the graph can touch the buffers
// between two of its nodes: the launch boundary was a grid-wide barrier, and the state's round trip through memory a pass,
// that the result does not need.  Every step still stores what its holding node stored, in that order -- observation rows,
// the slot rows and done bytes unless held (ChainStep::held), the reward -- through the same env_step_lean call, so the
// bytes are step_kernel_pipe's.  The state goes back once, after the last step; the sticky status byte is written once,
// at the end (a non-finite state is absorbing, as in rollout_kernel_lean).  No workgroup waits for another one.
//
// Actions arrive in groups of PCG_CHAIN_D steps: the next group's rows are requested before the current group is
// integrated, and ONE land() per group waits for them.  Loads and stores share the vmcnt counter, so that wait also meets
// the stores of the group's last step -- once per PCG_CHAIN_D steps, where rollout_kernel_lean's per-step land() meets every
// step's.  (D, waves per SIMD asked of the register allocator) by measurement: profiles/r21/graph_chain.txt.
// ---------------------------------------------------------------------------
#ifndef PCG_CHAIN_D
#define PCG_CHAIN_D 2
#endif
// waves per SIMD asked of the register allocator: the most at which the kernel stays out of scratch at that D
// (nx = 2: cstr, nx = 4: four_tank; PCG_CHAIN_WPE overrides, for the measurement builds)
constexpr int chain_wpe(int nx, int epl) {
#ifdef PCG_CHAIN_WPE
  return PCG_CHAIN_WPE;
#else
  return nx <= 2 ? (epl == 1 ? 7 : 6) : (epl == 1 ? 5 : 4);
#endif
}
template <class M, int EPL>
__global__ __launch_bounds__(BLOCK, chain_wpe(M::NX, EPL)) void step_chain_kernel(const StepArgs A) {
  CDevConst& c = *A.C;
  constexpr int NX = M::NX, NA = M::NA, D = PCG_CHAIN_D;
  using V = typename Vec<EPL>::T;
  const uint32_t B = (uint32_t)A.B;  // < 2^28 (pcg_graph_create), as in step_kernel_pipe
  const size_t Bs = (size_t)A.B;
  const int nx = M::DYNAMIC ? c.nx : NX;
  const int na = M::DYNAMIC ? c.na : NA;
  const int n = A.T;
  const PCG_CONSTANT ChainStep* const cs = A.chain;
  const bool nt = (A.nt_stores & 1) != 0;
  const bool ntl = (A.nt_stores & 4) != 0;
  const uint32_t e0 = (blockIdx.x * (uint32_t)BLOCK + threadIdx.x) * EPL;
  if (e0 >= B) return;
  const uint32_t o8 = e0 * 8u;
  const LaneOff8 at{o8};
  V xv[NX], an[D][NA] = {};
  // the action rows of steps s0 .. s0 + D - 1 (those the chain has)
  auto fetch = [&](int s0) {
#pragma unroll
    for (int d = 0; d < D; ++d)
      if (s0 + d < n) {
        const double* const a = cs[s0 + d].a;
#pragma unroll
        for (int i = 0; i < NA; ++i)
          if (i < na) an[d][i] = ntl ? Vec<EPL>::load_nt(row_at<double>(a + (size_t)i * Bs, o8)) : *row_at<V>(a + (size_t)i * Bs, o8);
      }
  };
#pragma unroll
  for (int i = 0; i < NX; ++i)
    if (i < nx) xv[i] = ntl ? Vec<EPL>::load_nt(row_at<double>(A.x + (size_t)i * Bs, o8)) : *row_at<V>(A.x + (size_t)i * Bs, o8);
  fetch(0);
#pragma unroll
  for (int i = 0; i < NX; ++i) land(xv[i]);
  Pack<EPL> xs[NX];
  unpack<NX, EPL>(xv, nx, xs);
  const Rows obs{A.obs, Bs, nt};
  for (int s0 = 0; s0 < n; s0 += D) {
    // The group's rows are consumed where they landed: the action map runs here, ahead of the next group's fetch, and its
    // results are the registers the D steps hold.  (Unpacked rows held across the fetch instead are a copy of every row
    // out of the registers the fetch is about to overwrite, and one back on the path without a fetch.)
#if PCG_LEAN_TRIM & 4
    Pack<EPL> ua[D][NA];
#pragma unroll
    for (int d = 0; d < D; ++d) {
#pragma unroll
      for (int i = 0; i < NA; ++i) land(an[d][i]);
      Pack<EPL> as[NA];
      unpack<NA, EPL>(an[d], na, as);
      lean_input<M, EPL>(c, as, ua[d]);
    }
#else
    Pack<EPL> as[D][NA];
#pragma unroll
    for (int d = 0; d < D; ++d) {
#pragma unroll
      for (int i = 0; i < NA; ++i) land(an[d][i]);
      unpack<NA, EPL>(an[d], na, as[d]);
    }
#endif
    asm volatile("" ::: "memory");
    if (s0 + D < n) fetch(s0 + D);
    asm volatile("" ::: "memory");
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int s = s0 + d;
      if (s < n) {
        const int t = A.t_scalar + s;
        const PCG_CONSTANT LeanStep& L = A.lean[min(t, c.N - 1)];
        int32_t held = cs[s].held;
        asm volatile("" : "+s"(held));  // (its two tests stay scalar branches, as in store_lean)
        LeanOut<M, EPL> out;
#if PCG_LEAN_TRIM & 4
        env_step_lean_u<M, EPL>(A, c, L, t, ua[d], xs, out);
#else
        env_step_lean<M, EPL>(A, c, L, t, as[d], xs, out);
#endif
        if (s + 1 < n) {
          put_obs_rows<M, EPL>(obs, at, nx, c.nsp_obs, c.nd, out.ox, L.osp, L.od, (held & 1) != 0);
        } else {  // the last step: the state goes back in place, row by row ahead of its observation row
          if (A.status) flag_nonfinite<NX, EPL>(A.status, e0, xs);
          put_state_rows<M, EPL>(Rows{A.x, Bs, (A.nt_stores & 2) != 0}, obs, at, nx, c.nsp_obs, c.nd, xs, out.ox, L.osp, L.od,
                                 (held & 1) != 0);
        }
        put<EPL>(at(A.rew), out.rew.v, nt);
        if (!(held & 2)) {
          put_done<EPL>(A.done + e0, out.done);
          asm volatile("");  // keep it a (scalar) branch
        }
      }
    }
  }
}

// Lean fused rollout: T lock-stepped env steps, W envs per lane, state in registers throughout;
// per step only the action row(s) are read and reward (+ observation rows, if requested) written.
template <class M, int EPL>
__global__ __launch_bounds__(BLOCK) void rollout_kernel_lean(const StepArgs A) {
  CDevConst& c = *A.C;
  constexpr int NX = M::NX, NA = M::NA;
  using V = typename Vec<EPL>::T;
  const int64_t B = A.B;
  const int nx = M::DYNAMIC ? c.nx : NX;
  const int na = M::DYNAMIC ? c.na : NA;
  const int nso = c.nsp_obs;
  const int64_t e0 = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * EPL;
  if (e0 >= B) return;
  V xv[NX], an[NA];
#pragma unroll
  for (int i = 0; i < NX; ++i)
    if (i < nx) xv[i] = *reinterpret_cast<const V*>(A.x + (size_t)i * B + e0);
  Pack<EPL> xs[NX];
  unpack<NX, EPL>(xv, nx, xs);
#pragma unroll
  for (int i = 0; i < NA; ++i)
    if (i < na) an[i] = *reinterpret_cast<const V*>(A.a_seq + (size_t)i * A.a_cs + e0);
  LeanOut<M, EPL> out;
  for (int s = 0; s < A.T; ++s) {
    Pack<EPL> as[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) land(an[i]);
    unpack<NA, EPL>(an, na, as);
    asm volatile("" ::: "memory");
    if (s + 1 < A.T) {  // next step's action in flight during this step's integration
      const double* nxt = A.a_seq + (size_t)(s + 1) * A.a_ss;
#pragma unroll
      for (int i = 0; i < NA; ++i)
        if (i < na) an[i] = *reinterpret_cast<const V*>(nxt + (size_t)i * A.a_cs + e0);
    }
    asm volatile("" ::: "memory");
    const PCG_CONSTANT LeanStep& L = A.lean[min(A.t_scalar + s, c.N - 1)];
    env_step_lean<M, EPL>(A, c, L, A.t_scalar + s, as, xs, out);
    if (A.rew_seq) put<EPL>(A.rew_seq + (size_t)s * A.r_ss + e0, out.rew.v, true);
    if (A.obs_seq)
      put_obs_rows<M, EPL>(Rows{A.obs_seq + (size_t)s * A.o_ss + e0, (size_t)A.o_cs, true}, LaneIdx{0}, nx, nso, c.nd, out.ox,
                           L.osp, L.od);
  }
  // a non-finite state is absorbing: one check at the end covers the T steps (sticky byte)
  if (A.status) flag_nonfinite<NX, EPL>(A.status, e0, xs);
  // final state and the last step's outputs into the regular per-step buffers
  const PCG_CONSTANT LeanStep& L = A.lean[min(A.t_scalar + A.T - 1, c.N - 1)];
  put_state_rows<M, EPL>(Rows{A.x, (size_t)B, false}, Rows{A.obs, (size_t)B, false}, LaneIdx{e0}, nx, nso, c.nd, xs, out.ox,
                         L.osp, L.od);
  put<EPL>(A.rew + e0, out.rew.v, false);
  put_done<EPL>(A.done + e0, out.done);
}

}  // namespace pcg
