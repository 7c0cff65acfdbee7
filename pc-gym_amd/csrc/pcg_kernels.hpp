// pcg_kernels.hpp -- device code shared by every translation unit of libpcgym_hip.so: the fused
// environment-step / rollout / test-hook kernel templates and make_kernels<ID>() (the table of
// instantiations for one model).  pcg_inst_*.hip instantiate groups of models so that the library
// builds in parallel; pcg_abi.hip and its pcg_abi_*.hip siblings hold the C ABI, the host dispatch and the reset kernel.
//
//
// Execution model
//   * one wavefront lane = one environment; 256-thread workgroups; grid = ceil(B/256)
//     (B = 2^20 -> 4096 workgroups = 16 per CU, 2 per CU per XCD round).
//   * all per-env arrays are SoA  field[component][B]  in HBM: lane i of a wave reads
//     address base + 8*i  -> every load/store instruction of a wave touches 512
//     contiguous bytes.  Each byte of state/action/obs crosses HBM exactly once per step.
//   * env state, the RK work vectors and the held inputs live in VGPRs; everything that
//     is identical for all envs of a plan (model constants, folded affine maps, bounds,
//     constraint rows) is one DevConst block in device memory read with wave-uniform
//     addresses, i.e. through the scalar cache into SGPRs -- no VGPR or LDS cost.
//   * time-indexed tables (set-point / disturbance schedules) are read with the scalar
//     unit when the batch is lock-stepped, and are staged in LDS when every env carries
//     its own step counter (per-lane table lookups after masked auto-reset).
//   * DOPRI5 stage vectors: VGPRs, or LDS [stage][component][lane] (PCG_OPT_LDS_STAGES).
//   * no MFMA: the env step has no dense contraction; the one dense contraction of a closed loop, the policy of
//     pcg_rollout_policy.hpp, is small enough for scalar-operand FMAs (measured: DESIGN.md section 3).
//
// Reference path restated: make_env.step / reset (src/pcgym/pcgym.py:263-500),
// integration_engine (src/pcgym/integrator.py:65-107,163-182), model RHS
// (src/pcgym/model_classes.py) -- see pcg_models.hpp for per-model line ranges.
#pragma once
#ifndef __HIPCC_RTC__  // built in under hipRTC
#include <hip/hip_runtime.h>
#endif

#ifndef __HIPCC_RTC__  // host-side headers: not available (and not needed) under hipRTC
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>
#endif

#include "../../include/pcgym_hip.h"
#include "pcg_integrators.hpp"
#include "pcg_models.hpp"

#ifndef PCG_LEAN_WPE
#define PCG_LEAN_WPE 1  // min waves per SIMD requested from the register allocator for the lean kernels
#endif

namespace pcg {

constexpr int BLOCK = 256;      // threads per workgroup (4 waves, one per SIMD)
constexpr int BLOCK_LDS = 64;   // LDS-staged DOPRI5: 6*NX*8 B of stage storage per lane
// Adaptive (DOPRI5) kernels run one wave per workgroup: lanes take different numbers of steps, a 4-wave workgroup
// holds its CU slots until its slowest wave ends, and single-wave workgroups let the dispatcher refill per wave.
// Rosenbrock integrators with the dense per-lane LU in LDS: Rodas3 always, Rodas4 unless the model brings its own
// structured linear algebra (M::ROS_STRUCTURED -> registers only, launched like the explicit adaptive pair)
constexpr bool ros_dense(int integ, bool structured) {
  return integ == PCG_INT_RODAS3 || (is_ros_pair(integ) && !structured);
}
// the fixed-step schemes the lean pipelined kernel is instantiated for: index into Kernels::pipe (-1: none)
constexpr int lean_scheme(int integ) { return integ == PCG_INT_RK4 ? 0 : integ == PCG_INT_CV8 ? 1 : -1; }
constexpr int tb(bool lds_stages, int integ, int nx = 0, bool structured = false) {
  return ros_dense(integ, structured) ? ros_threads(nx)
         : (lds_stages || integ == PCG_INT_DOPRI5 || is_ros_pair(integ) || integ == PCG_INT_TSIT5) ? BLOCK_LDS : BLOCK;
}
// doubles of dynamic LDS the integrator itself needs per workgroup (the schedules follow them)
constexpr size_t integ_lds_doubles(int nx, int integ, bool lds_stages, bool structured = false) {
  return ros_dense(integ, structured) ? ros_lds_doubles(nx) : lds_stages ? (size_t)6 * nx * BLOCK_LDS : 0;
}
// Minimum waves per SIMD asked of the register allocator.  DOPRI5 with <= 10 states needs ~280 registers
// when left alone (1 wave/SIMD, latency-bound: measured 14k cycles per attempted step against ~3.6k of
// issue); capping it at 256 costs a few spills and doubles the resident waves.
constexpr int wpe(int nx, int integ, bool lds_stages, bool structured = false) {
  return (((integ == PCG_INT_DOPRI5 || integ == PCG_INT_TSIT5) && !lds_stages && nx <= 10) ||
          (is_ros_pair(integ) && structured && nx <= 10)) ? 2 : 1;
}
constexpr int KNU = PCG_MAX_NA + PCG_MAX_NDM;                      // kernel-side u width
constexpr int CON_W = PCG_MAX_NX + PCG_MAX_NSP + PCG_MAX_NDM + KNU; // padded constraint row

// Everything wave-uniform about a plan.  Read only through uniform addresses (scalar loads).
// Layout matters: the fields the lean step kernel touches are packed at the front and the affine
// maps are interleaved per row, so the compiler can fetch them with a few wide s_load_dwordx8/x16
// instead of ~50 separate 8-byte scalar loads (the scalar cache is shared by several CUs and every
// wave of the grid replays this prologue).
struct OMap {
  double lo, sc, off;      // obs = (o - lo) * sc + off          (pcgym.py:483-498; mask -> sc=off=0)
};
// DevConst::a_mode, how env_step_lean maps its action: not at all (normalise_a off), (a + 1) * a_w + a_lo with the half
// width from the host, or through action_map() where that fold would not be exact (amap_fold, below).
enum { PCG_AMAP_NONE = 0, PCG_AMAP_FOLDED = 1, PCG_AMAP_EXACT = 2 };
// With p = a + 1, d = hi - lo and w = d 0.5:  fl(fl(p d) 0.5) == fl(p w) bit for bit, because a scaling by a power of two
// commutes with rounding as long as nothing on the way is subnormal or overflows.  A non-zero p = fl(a + 1) is at least
// 2^-53 in magnitude, so with d finite and |w| >= 2^-969 (or d == 0) p d 0.5 is normal for every action; an infinite or NaN
// p gives the same infinity or NaN both ways.  What remains is overflow: |p d| >= 2^1024 is infinite in action_map() and
// may be finite here -- actions beyond 2^1023 / |d|, past anything a normalised policy emits.
// Where the rule fails (w subnormal: it may have lost d's last bit, and the product is rounded twice in one form and once
// in the other; d infinite) the plan keeps action_map().
inline bool amap_fold(double lo, double hi, double* w) {
  const double d = hi - lo, h = d * 0.5;
  *w = h;
  return __builtin_fabs(d) < __builtin_inf() && (d == 0.0 || __builtin_fabs(h) >= 0x1p-969);
}
struct DevConst {
  double dt, h, rtol, atol;
  double dt_edge, h_floor;            // dt (1 - 1e-14) and 1e-13 dt of the DOPRI5 loop, folded on the host
  double h2, h6;                      // 0.5 h and h / 6.0 of rk4(), folded on the host (there is no scalar fp unit: a
                                      // wave-uniform division in the kernel is eleven VALU instructions per tile)
  uint32_t flags;
  int32_t nx, na, ndm, nd, nsp, nsp_obs, ncon, nrew, N, substeps, max_steps, nobs, has_x0_unc, nunc;
  int32_t sp_index[PCG_MAX_NSP], d_slot[PCG_MAX_NDM];
  int32_t a_mode;                     // env_step_lean's action map (PCG_AMAP_*, above); sits in what was padding
  double kp[16];                      // model KP (pcg_models.hpp) of the five built-in models
  double a_lo[PCG_MAX_NA], a_hi[PCG_MAX_NA];  // a_space: action_map() (pcgym.py:372-379)
  double a_w[PCG_MAX_NA];             // (a_hi - a_lo) * 0.5, folded on the host (build_devconst; PCG_AMAP_FOLDED only)
  double r_scale[PCG_MAX_NX];
  double d_default[PCG_MAX_NDM];
  OMap omap[PCG_MAX_NOBS];
  // ---- cold: a_delta, noise, reset, Gaussian disturbances, batch reward, constraints, affine model ----
  double a_act_lo[PCG_MAX_NA], a_act_hi[PCG_MAX_NA], a_0[PCG_MAX_NA];
  double noise_pct[PCG_MAX_NX];
  double x0[PCG_MAX_NX + PCG_MAX_NSP];
  double x0_unc[PCG_MAX_NX];
  double d_sigma[PCG_MAX_NDM], d_lo[PCG_MAX_NDM], d_hi[PCG_MAX_NDM];
  int32_t rew_index[PCG_MAX_NX];
  // constraint rows over [x(PCG_MAX_NX) | sp(PCG_MAX_NSP) | d(PCG_MAX_NDM) | u(KNU)], compat folded in
  double con_A[PCG_MAX_NCON][CON_W];
  double con_b[PCG_MAX_NCON];
  double kp_big[136];                 // KP of the affine custom model (A 8x8 | B 8x4 | c 8)
  // per-env parameter uncertainty (pcgym.py:212-253, 301-310): raw parameter vector + which entries vary
  double raw[32];
  double unc_pct[PCG_MAX_NUNC];
  int32_t unc_index[PCG_MAX_NUNC];
  int32_t emp_off[PCG_MAX_NUNC + 1];  // PCG_F_UNC_EMPIRICAL: sample tables live behind the schedules in `sched`
  // PCG_F_REWARD_TRACK: normalised tracking + action-increment reward (pc-gym_paper custom_reward family)
  double trk_lo[PCG_MAX_NSP], trk_inv[PCG_MAX_NSP];  // o_space low and 1/(high-low) of each SP state
  double act_lo[PCG_MAX_NA], act_inv[PCG_MAX_NA];    // a_space low and 1/(high-low)
  double R_du, R_u;
  int32_t nbox, box_index[PCG_MAX_RBOX];
  double box_lo[PCG_MAX_RBOX], box_inv[PCG_MAX_RBOX];    // o_space low and 1/(high-low) of each boxed state
  double box_lon[PCG_MAX_RBOX], box_hin[PCG_MAX_RBOX];   // box bounds, normalised
  // user constraint expressions (run-time compiled): quirk Q3 as an affine map of the state / input vector they see
  double q3_mul[PCG_MAX_NOBS], q3_add[PCG_MAX_NOBS], q3u_mul[KNU], q3u_add[KNU];
  // PCG_INT_RODAS4 end-point error control: ep_c = ep_frac log2(e) (0 when off), largest tolerance exponent
  double ep_c;
  int32_t ep_kmax;
  // ... heavy envs (M::coop_key >= coop_thr) take SEULEX-8 instead of the pair (pcg_seulex.hpp); 0 = off
  double coop_thr;
};

using CDevConst = const PCG_CONSTANT DevConst;

// Wave-uniform values of one lock-stepped step t -> t + 1 (lean plans), folded on the host at plan creation
// (pcg_abi_cfg.hip: lean_table): what env_step_lean() used to compute on the vector unit once per tile.
struct LeanStep {
  double osp[PCG_MAX_NSP];  // observation SP slots, normalised: SP[k][min(t, N-1)]                (quirk Q5)
  double spn[PCG_MAX_NSP];  // reward set-points SP[k][min(t+1, N-1)]
  double od[PCG_MAX_NDM];   // observation disturbance slots, normalised: D[k][min(t+1, N-1)]    (quirk Q6)
  double ud[PCG_MAX_NDM];   // model disturbance inputs held over the step (defaults, overridden by the configured ones)
};

// One step of a chained launch (step_chain_kernel, pcg_lean.hpp): its action rows and its StepArgs::held word.  A device
// table owned by the step graph that records the launch (pcg_graph_create); wave-uniform, read with scalar loads.
struct ChainStep {
  const double* a;
  int32_t held;
};

struct StepArgs {
  CDevConst* C;                      // constant address space: uniform reads -> s_load
  const PCG_CONSTANT double* sched;   // [nsp + nd][N]
  const PCG_CONSTANT LeanStep* lean;  // [N] (lock-stepped lean kernels)
  double* x;
  const double* a;
  const double* d;
  int32_t* t;
  double* a_save;
  double* obs;
  double* rew;
  uint8_t* done;
  uint8_t* viol;
  double* g;
  double* g_pre;
  int32_t* nsteps;
  double* p_unc;        // [nunc][B] per-env uncertain parameters
  double* u_prev;       // [na][B] previous physical action (PCG_F_REWARD_TRACK)
  uint8_t* status;      // [B] per-env health of the step (PCG_ST_*), or null
  const uint8_t* mask;  // reset only
  int64_t B;
  int64_t env_offset;
  uint64_t seed;
  int32_t t_scalar;
  int32_t sched_in_lds;  // per-env-t kernels: schedules staged in LDS
  int32_t nt_stores;     // stream kernels: non-temporal stores for obs / reward
  int32_t q_tile;        // work-queue kernel: slots of the LDS tile | QT_* flags (below); flat rollout: its step cadence
  int32_t auto_reset;    // per-env-t kernels: reset the envs that finished in this step (pcg_step_autoreset)
  uint64_t reset_seed;   // RNG key of those resets
  // rollout: the T steps from t_scalar, their actions one sequence ...
  // ... or, for the chained launch of a recorded step graph (step_chain_kernel), one table entry per step.  The two share
  // the slot: StepArgs keeps its size and every field its offset, so every other kernel -- those that take a second
  // by-value argument behind StepArgs included -- keeps its kernarg layout and its code.
  union {
    const double* a_seq;
    const PCG_CONSTANT ChainStep* chain;  // [T]
  };
  double* obs_seq;
  double* rew_seq;
  // element strides of the sequences: (step, component); the env index is always unit-stride
  int64_t a_ss, a_cs, o_ss, o_cs, r_ss;
  int32_t T;
  float q_w;             // work-queue kernel: weight of ln(scaled |f(x0)|) in the sort key (the transient's share)
  int32_t q_prio;        // work-queue kernel: waves holding one of the q_prio heaviest envs of their tile raise their issue
                         // priority (0 = off); workgroups of the upper half of the grid start their heaviest envs two waves on
  int32_t fixup;         // guarded plans in two launches (pcg_abi_step.hip): 1 = the general kernel leaves an env the guard does not
                         // trust untouched and marks it (done[e] = PCG_DONE_PENDING), the work-queue kernel then integrates
                         // exactly the marked envs with the adaptive pair and finishes their step
  int32_t held;          // step_kernel_pipe inside a recorded step graph (pcg_graph_create), 0 everywhere else: bit 0 = the
                         // observation's set-point / disturbance slot rows already hold this step's values, bit 1 = the
                         // done bytes do (the previous node stored the same bytes): those stores are skipped
  // barrier-free rollout of a guarded plan in two passes (pcg_rollout_flat.hpp): plan-owned work space
  int32_t* flat_q;       // [4] counters: [1] length of the hand-over list, [2] head of the second pass's queue
  int32_t* flat_hot;     // [B] the envs the first pass handed over (in the order they tripped)
  int32_t* flat_tstar;   // [B] the step at which an env left the first pass
};

// The q_tile word of a work-queue launch: tile slots in the low bits, then how the tile is laid out in LDS and how many
// waves of a workgroup take part in the cooperative phase (written by pcg_abi_step.hip, read by pcg_step_queue.hpp)
constexpr int32_t QT_SLOTS = 0xFFFF;      // slots of the tile
constexpr int32_t QT_XLDS = 0x20000;      // the tile's state lives in LDS
constexpr int32_t QT_LEAN = 0x40000;      // the lean LDS layout (QTile): what lets the state fit
constexpr int QT_COOPW_SHIFT = 27;        // 4 bits: waves in the cooperative phase of a Rosenbrock tile (0 = all)

// ---------------------------------------------------------------------------
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11).  RNG contract:
//   key = (seed_lo, seed_hi); ctr = (env_lo, env_hi, t, purpose + pair index)
//   uniform draws: one block -> two 53-bit uniforms;  normal draws: one block -> four fp32 Box-Muller variates (v2).
// ---------------------------------------------------------------------------
constexpr uint32_t RNG_NOISE = 0x100u, RNG_DIST = 0x200u, RNG_RESET = 0x300u;

__host__ __device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

PCG_DEV void rng_uniform2(uint64_t seed, uint64_t env, uint32_t t, uint32_t stream, double& u0, double& u1) {
  uint32_t o[4];
  philox4x32_10((uint32_t)env, (uint32_t)(env >> 32), t, stream, (uint32_t)seed, (uint32_t)(seed >> 32), o);
  u0 = (double)(((uint64_t)(o[0] >> 5) << 26) | (uint64_t)(o[1] >> 6)) * (1.0 / 9007199254740992.0);
  u1 = (double)(((uint64_t)(o[2] >> 5) << 26) | (uint64_t)(o[3] >> 6)) * (1.0 / 9007199254740992.0);
}

// Box-Muller in fp32, as an explicit sequence of IEEE-754 single-precision operations (no contraction, fmaf where
// written, correctly rounded divide and square root) -- DESIGN.md "RNG", contract v2.  Every operation is exactly
// specified, so the oracle's C twin (fmaf / sqrtf / rintf) produces the SAME BITS, and the variate costs ~65 fp32
// instructions for two normals instead of ~100 fp64 ones at half the issue rate (the fp64 log / sqrt / sincospi of
// round 1 made observation noise cost more VALU time than the whole RK4 step: profiles/r1/exploration.md).  A 24-bit
// uniform and variates within 2.0e-7 of r (3.4 units of 2^-24 r, measured against a long double Box-Muller on the same
// uniforms; tests/test_rng_accuracy.py holds 6 units) are far beyond what a noise sample needs (the reference draws
// np.random.normal).
//   u0 = odd 24-bit integer * 2^-24 in (0,1),  u1 = 24-bit integer * 2^-24 in [0,1)
//   ln u0 = e ln2 + 2 atanh(s), s = (m-1)/(m+1), m in [sqrt(1/2), sqrt(2));   r = sqrt(-2 ln u0)
//   angle 2 pi u1 by quarter turns, Taylor polynomials on [-pi/4, pi/4];   z0 = r cos, z1 = r sin
PCG_DEV void box_muller_f32(uint32_t w0, uint32_t w1, float& z0, float& z1) {
#pragma clang fp contract(off)
  const float u0 = (float)(((w0 >> 9) << 1) | 1u) * 0x1p-24f;
  const float u1 = (float)(w1 >> 8) * 0x1p-24f;
  float m = __builtin_amdgcn_frexp_mantf(u0);  // [0.5, 1)
  int e = __builtin_amdgcn_frexp_expf(u0);
  const bool lo = m < 0.70710678f;
  m = lo ? m + m : m;
  e = lo ? e - 1 : e;
  const float s = (m - 1.0f) / (m + 1.0f);
  const float q = s * s;
  float p = 0.22222222f;
  p = __builtin_fmaf(p, q, 0.28571429f);
  p = __builtin_fmaf(p, q, 0.4f);
  p = __builtin_fmaf(p, q, 0.66666667f);
  const float lm = __builtin_fmaf(s * q, p, s + s);
  const float fe = (float)e;
  const float ln = __builtin_fmaf(fe, 0.693359375f, __builtin_fmaf(fe, -2.12194440e-4f, lm));
  const float r = __builtin_sqrtf(__builtin_fmaxf(-2.0f * ln, 0.0f));
  const float x = u1 + u1;  // [0, 2)
  const float n = __builtin_rintf(x + x);  // quarter-turn index 0..4
  const float a = __builtin_fmaf(n, -0.5f, x) * 3.14159274f;  // [-pi/4, pi/4]
  const float a2 = a * a;
  float ps = 2.7557319e-6f;
  ps = __builtin_fmaf(ps, a2, -1.9841270e-4f);
  ps = __builtin_fmaf(ps, a2, 8.3333333e-3f);
  ps = __builtin_fmaf(ps, a2, -0.16666667f);
  const float sy = __builtin_fmaf(a * a2, ps, a);
  float pc = 2.4801587e-5f;
  pc = __builtin_fmaf(pc, a2, -1.3888889e-3f);
  pc = __builtin_fmaf(pc, a2, 4.1666667e-2f);
  pc = __builtin_fmaf(pc, a2, -0.5f);
  const float cy = __builtin_fmaf(a2, pc, 1.0f);
  const int qd = (int)n & 3;
  const float ss = (qd & 1) ? cy : sy, cc = (qd & 1) ? sy : cy;
  z1 = r * ((qd & 2) ? -ss : ss);
  z0 = r * (((qd + 1) & 2) ? -cc : cc);
}

// `stream` = purpose + pair index p (p = variate index / 2): pair p lives in Philox block (purpose + p/2), words
// (0,1) for even p and (2,3) for odd p -- one block serves four normal variates.
PCG_DEV void rng_normal2(uint64_t seed, uint64_t env, uint32_t t, uint32_t stream, double& z0, double& z1) {
  const uint32_t pair = stream & 0xFFu, purpose = stream & ~0xFFu;
  uint32_t o[4];
  philox4x32_10((uint32_t)env, (uint32_t)(env >> 32), t, purpose + (pair >> 1), (uint32_t)seed, (uint32_t)(seed >> 32), o);
  float f0, f1;
  box_muller_f32((pair & 1u) ? o[2] : o[0], (pair & 1u) ? o[3] : o[1], f0, f1);
  z0 = (double)f0;
  z1 = (double)f1;
}

// value at runtime index `idx` of a register array, without dynamic register indexing
template <int N>
PCG_DEV double pick(const double (&v)[N], int idx) {
  double r = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) r = (i == idx) ? v[i] : r;
  return r;
}

// reset of ONE env (pcgym.py:263-349): initial state with optional x0 / parameter uncertainty (Philox keyed by
// `seed`), first observation, a_delta accumulator, step counter.  Shared by reset_kernel and by the fused
// "step, then reset what finished" path of step_kernel (pcg_step_autoreset).
PCG_DEV void reset_env(const StepArgs& A, CDevConst& c, int64_t e, uint64_t seed) {
  const int64_t B = A.B;
  const int nx = c.nx, nsp = c.nsp_obs, nd = c.nd;
  const uint64_t env_id = (uint64_t)(A.env_offset + e);
  for (int i = 0; i < nx; ++i) {
    double v = c.x0[i];
    if (c.has_x0_unc && c.x0_unc[i] != 0.0) {  // apply_uncertainties, pcgym.py:255-261
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
    A.x[(size_t)i * B + e] = v;
    A.obs[(size_t)i * B + e] = (v - c.omap[i].lo) * c.omap[i].sc + c.omap[i].off;
  }
  for (int k = 0; k < nsp; ++k)
    A.obs[(size_t)(nx + k) * B + e] = (c.x0[nx + k] - c.omap[nx + k].lo) * c.omap[nx + k].sc + c.omap[nx + k].off;
  for (int k = 0; k < nd; ++k) {  // disturbances[k][0] (pcgym.py:291-298, quirk Q6)
    const int j = nx + nsp + k;
    A.obs[(size_t)j * B + e] = (A.sched[(size_t)(c.nsp + k) * c.N] - c.omap[j].lo) * c.omap[j].sc + c.omap[j].off;
  }
  // uncertain model parameters (pcgym.py:301-310): sampled per env, appended to the observation
  for (int j = 0; j < c.nunc; ++j) {
    const double orig = c.raw[c.unc_index[j]], pct = c.unc_pct[j];
    const int ri = nx + j;  // RNG index after the x0 draws
    double v;
    if (c.flags & PCG_F_UNC_EMPIRICAL) {  // np.random.choice(samples), pcgym.py:311-316
      double u0, u1;
      rng_uniform2(seed, env_id, 0u, RNG_RESET + (uint32_t)(ri >> 1), u0, u1);
      const int len = c.emp_off[j + 1] - c.emp_off[j];
      int idx = (int)(((ri & 1) ? u1 : u0) * (double)len);
      idx = idx < len - 1 ? idx : len - 1;
      v = A.sched[(size_t)(c.nsp + c.nd) * c.N + c.emp_off[j] + idx];
    } else if (c.flags & PCG_F_X0_NORMAL) {
      double z0, z1;
      rng_normal2(seed, env_id, 0u, RNG_RESET + (uint32_t)(ri >> 1), z0, z1);
      v = orig + pct * orig * ((ri & 1) ? z1 : z0);
    } else {
      double u0, u1;
      rng_uniform2(seed, env_id, 0u, RNG_RESET + (uint32_t)(ri >> 1), u0, u1);
      v = orig * (1 + pct * (2.0 * ((ri & 1) ? u1 : u0) - 1.0));
    }
    A.p_unc[(size_t)j * B + e] = v;
    const int q = nx + nsp + nd + j;
    A.obs[(size_t)q * B + e] = (v - c.omap[q].lo) * c.omap[q].sc + c.omap[q].off;
  }
  if ((c.flags & PCG_F_A_DELTA) && A.a_save)
    for (int i = 0; i < c.na; ++i) A.a_save[(size_t)i * B + e] = c.a_0[i];
  if (A.t) A.t[e] = 0;
}

template <class M, class R = double, class K = typename M::CKP>
struct RhsFn {
  const K& kp;
  const typename M::template HoldT<R>& hold;
  PCG_DEV void operator()(const R (&x)[M::NX], R (&dx)[M::NX]) const { M::rhs(kp, hold, x, dx); }
};

// where a model's constants live: the 16-double block, or the 136-double one (affine custom model, user models)
template <class M, class = void>
struct kp_is_big : tt::false_type {};
template <class M>
struct kp_is_big<M, tt::void_t<decltype(M::KP_BIG)>> : tt::true_type {};
template <class M>
PCG_DEV typename M::CKP& model_kp(CDevConst& c) {
  return *(typename M::CKP*)((M::DYNAMIC || kp_is_big<M>::value) ? c.kp_big : c.kp);
}

#ifdef PCG_USER_NCON
// user constraint expressions, defined by the run-time compiled translation unit (pcgym_hip.h: user_cons_src)
__device__ void pcg_user_constraints(const double* x, const double* u, double* g);
#endif
#ifdef PCG_USER_REWARD
__device__ double pcg_user_reward(const double* o, const double* x, const double* u, const double* sp, int violated,
                                  int t, int N);
#endif

// the reference's state vector [x | SP slots | disturbances] as the user expressions index it
template <class M>
PCG_DEV void state_vector(CDevConst& c, const double (&x)[M::NX], const double (&spv)[PCG_MAX_NSP],
                          const double (&dv)[PCG_MAX_NDM], double (&s)[PCG_MAX_NOBS]) {
  const int nx = M::DYNAMIC ? c.nx : M::NX, nso = c.nsp_obs, nd = c.nd;
#pragma unroll
  for (int i = 0; i < PCG_MAX_NOBS; ++i) s[i] = 0.0;
#pragma unroll
  for (int i = 0; i < M::NX; ++i)
    if (i < nx) s[i] = x[i];
  for (int k = 0; k < nso; ++k) s[nx + k] = spv[k];
  for (int k = 0; k < nd; ++k) s[nx + nso + k] = dv[k];
}

// constraint rows g = A.[x|sp|d|u] - b  (affine form of the reference's callable, pcgym.py:560-577);
// writes rows to gout (if non-null) and returns "any row > 0".
template <class M>
PCG_DEV bool constraint_rows(CDevConst& c, const double (&x)[M::NX], const double (&spv)[PCG_MAX_NSP],
                             const double (&dv)[PCG_MAX_NDM], const double (&u)[M::NA + M::NDM], double* gout,
                             int64_t B, int64_t e) {
  bool violated = false;
#ifdef PCG_USER_NCON
  {  // the callable form: g = user(x, u) on the (quirk Q3: re-"de-normalised") state / input vectors
    double s[PCG_MAX_NOBS], uu[KNU], g[PCG_USER_NCON];
    state_vector<M>(c, x, spv, dv, s);
    for (int i = 0; i < c.nobs; ++i) s[i] = s[i] * c.q3_mul[i] + c.q3_add[i];
#pragma unroll
    for (int j = 0; j < KNU; ++j) uu[j] = (j < M::NA + M::NDM) ? u[j < M::NA + M::NDM ? j : 0] * c.q3u_mul[j] + c.q3u_add[j] : 0.0;
    pcg_user_constraints(s, uu, g);
#pragma unroll
    for (int r = 0; r < PCG_USER_NCON; ++r) {
      if (gout) gout[(size_t)r * B + e] = g[r];
      violated |= (g[r] > 0.0);
    }
    return violated;
  }
#endif
  for (int r = 0; r < c.ncon; ++r) {
    const PCG_CONSTANT double* row = c.con_A[r];
    double g = -c.con_b[r];
#pragma unroll
    for (int i = 0; i < M::NX; ++i) g += row[i] * x[i];
#pragma unroll
    for (int k = 0; k < PCG_MAX_NSP; ++k) g += row[PCG_MAX_NX + k] * spv[k];
#pragma unroll
    for (int k = 0; k < PCG_MAX_NDM; ++k) g += row[PCG_MAX_NX + PCG_MAX_NSP + k] * dv[k];
#pragma unroll
    for (int j = 0; j < M::NA; ++j) g += row[PCG_MAX_NX + PCG_MAX_NSP + PCG_MAX_NDM + j] * u[j];
#pragma unroll
    for (int j = 0; j < M::NDM; ++j)
      g += row[PCG_MAX_NX + PCG_MAX_NSP + PCG_MAX_NDM + PCG_MAX_NA + j] * u[M::NA + j];
    if (gout) gout[(size_t)r * B + e] = g;
    violated |= (g > 0.0);
  }
  return violated;
}

// schedule lookup: lock-stepped -> uniform scalar load; per-env t -> LDS table (or global)
template <bool PER_ENV_T>
PCG_DEV double sched_at(const PCG_CONSTANT double* sched_g, const double* sched_l, bool in_lds, int row, int N, int idx) {
  if (PER_ENV_T && in_lds) return sched_l[row * N + idx];
  return sched_g[(size_t)row * N + idx];
}

// per-env results of one step, kept in registers so the caller chooses the store width
template <class M>
struct EnvOut {
  double ox[M::NX];          // observation rows of the physical states
  double osp[PCG_MAX_NSP];   // SP slots
  double od[PCG_MAX_NDM];    // disturbance slots
  double ounc[PCG_MAX_NUNC]; // uncertain-parameter slots
  double rew;
  bool done, viol;
  uint8_t status;            // PCG_ST_*
};

// ---------------------------------------------------------------------------
// One env step for the lane's environment.  Statement order follows
// make_env.step (pcgym.py:350-500).  `x` is the lane's physical state (in/out);
// everything the hot path writes comes back in `out` (registers).  Only the rare
// side outputs (a_save, constraint rows, DOPRI5 step counts) are stored here.
// ---------------------------------------------------------------------------
// integrate one env over [0,dt] with model constants `kp` of any storage class (scalar constants of the
// plan, or a per-lane struct when parameters are uncertain)
// A lane whose adaptive integration gave up (step budget exhausted / step-size underflow) stopped at some t < dt:
// its state is poisoned with NaN so that the failure can never pass for a result (the reference's CVODES raises).
template <int NX>
PCG_DEV void poison_if_failed(int status, double (&x)[NX]) {
  if (status != PCG_ST_OK) {
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = __builtin_nan("");
  }
}
// PCG_ST_NONFINITE when a step that did not fail in the integrator still left a non-finite state
template <int NX>
PCG_DEV int finite_status(int status, const double (&x)[NX], int nx) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < NX; ++i) ok = ok && (i >= nx || __builtin_fabs(x[i]) < __builtin_inf());
  return (status == PCG_ST_OK && !ok) ? PCG_ST_NONFINITE : status;
}

constexpr int PCG_ST_PENDING = 64;        // internal: a guarded env left to the fix-up launch (never reaches a status buffer)
constexpr unsigned char PCG_DONE_PENDING = 2;  // its mark in the `done` buffer between the two launches (overwritten by the second)
// Guarded fixed-step plans on one env (PCG_INT_RK4G, PCG_INT_T5G): the fixed-step scheme under the model's guard; an env
// that is not trusted (guard tripped; PCG_INT_T5G: or the embedded error estimate too large) is re-integrated from its start
// state by the adaptive pair at the plan's tolerance.  Returns the pair's status (PCG_ST_OK for trusted envs).
template <class M, int INTEG, class K, class F>
PCG_DEV int guarded_env(const F& f, const K& kp, const typename M::Hold& hold, double (&x)[M::NX], CDevConst& c, int nx,
                        int& nacc, int& nrej, bool defer = false) {
  constexpr int NX = M::NX;
  int status = PCG_ST_OK;
  if constexpr (has_guard<M>::value) {
    double x0[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x0[i] = x[i];
    int gc;
    if constexpr (INTEG == PCG_INT_T5G) {
      int g1[1];
      t5_guarded<M, K, double>(kp, hold, x, c.h, c.substeps, g1);
      gc = g1[0];
    } else {
      gc = rk4_guarded<M>(f, kp, hold, x, c.h, c.substeps);
    }
    if (gc != 0) {  // the fixed step is not trusted for this env: the adaptive pair, from the start state
#pragma unroll
      for (int i = 0; i < NX; ++i) x[i] = x0[i];
      if (defer) return PCG_ST_PENDING;  // two-launch form: the work-queue kernel picks this env up (same pair, same tolerance)
      RegStages<NX> Kst;
      // at the PLAN's tolerance, whatever tripped (round 3 ran contracting states at 1e-7 whatever the user had asked for)
      status = dopri5<NX>(f, Kst, x, nx, c.dt, c.rtol, c.atol, c.max_steps, nacc, nrej);
      poison_if_failed<NX>(status, x);
    }
  } else {
    status = PCG_ST_NONFINITE;  // (not reachable: plans of models without a guard are refused at creation)
  }
  return status;
}

template <class M, int INTEG, bool LDS_STAGES, class K>
PCG_DEV int integrate_env(const StepArgs& A, CDevConst& c, const K& kp, const double (&u)[M::NA + M::NDM],
                          double (&x)[M::NX], double* stage_l, int64_t e, int nx) {
  constexpr int NX = M::NX;
  const typename M::Hold hold = M::hold(kp, u);
  const RhsFn<M, double, K> f{kp, hold};
  int status = PCG_ST_OK;
  if (INTEG == PCG_INT_RK4) {
    rk4<NX>(f, x, c.h, c.h2, c.h6, c.substeps);
  } else if (INTEG == PCG_INT_RODAS3) {
    int nacc = 0, nrej = 0;
    const RosLds<NX> Lm(stage_l);
    status = rodas3<NX>(f, Lm, x, nx, c.dt, c.rtol, c.atol, c.max_steps, nacc, nrej);
    if (A.nsteps) {
      A.nsteps[e] = nacc;
      A.nsteps[A.B + e] = nrej;
    }
    poison_if_failed<NX>(status, x);
  } else if (INTEG == PCG_INT_CV8) {
    cv8<NX>(f, x, c.h, c.substeps);
  } else if (INTEG == PCG_INT_RK4G || INTEG == PCG_INT_T5G) {
    int nacc = 0, nrej = 0;
    status = guarded_env<M, INTEG>(f, kp, hold, x, c, nx, nacc, nrej, A.fixup != 0);
    if (status == PCG_ST_PENDING) return status;
    if (A.nsteps) {
      A.nsteps[e] = nacc;
      A.nsteps[A.B + e] = nrej;
    }
  } else if (INTEG == PCG_INT_TSIT5) {
    int nacc = 0, nrej = 0;
    status = tsit5<NX>(f, x, nx, c.dt, c.rtol, c.atol, c.max_steps, nacc, nrej);
    if (A.nsteps) {
      A.nsteps[e] = nacc;
      A.nsteps[A.B + e] = nrej;
    }
    poison_if_failed<NX>(status, x);
  } else if (is_ros_pair(INTEG)) {
    int nacc = 0, nrej = 0;
    const EpWeights<M, K> ep{kp, u, c.ep_c, c.ep_kmax};
    if constexpr (ros_structured<M>::value) {
      if (!seulex8_if_heavy<M>(kp, hold, u, f, ep, x, nx, c.dt, c.rtol, c.atol, c.max_steps, c.coop_thr, nacc, nrej, status)) {
        const RosStructured<M, K> ls{kp, hold, {}};
        status = ros_pair<INTEG, NX>(f, ls, ep, x, nx, c.dt, c.rtol, c.atol, c.max_steps, nacc, nrej);
      }
    } else {
      const RosLds<NX> Lm(stage_l);
      const RosDense<NX, RhsFn<M, double, K>> ls{f, Lm, nx, c.rtol, c.atol};
      status = ros_pair<INTEG, NX>(f, ls, ep, x, nx, c.dt, c.rtol, c.atol, c.max_steps, nacc, nrej);
    }
    if (A.nsteps) {
      A.nsteps[e] = nacc;
      A.nsteps[A.B + e] = nrej;
    }
    poison_if_failed<NX>(status, x);
  } else {
    int nacc = 0, nrej = 0;
    if (LDS_STAGES) {
      LdsStages<NX, BLOCK_LDS> Kst{stage_l + threadIdx.x};
      status = dopri5<NX>(f, Kst, x, nx, c.dt, c.rtol, c.atol, c.max_steps, nacc, nrej);
    } else {
      RegStages<NX> Kst;
      status = dopri5<NX>(f, Kst, x, nx, c.dt, c.rtol, c.atol, c.max_steps, nacc, nrej);
    }
    if (A.nsteps) {
      A.nsteps[e] = nacc;
      A.nsteps[A.B + e] = nrej;
    }
    poison_if_failed<NX>(status, x);
  }
  return finite_status<NX>(status, x, nx);
}

// Action map of make_env.step (pcgym.py:371-379) for one action component, in the reference's own operation order and
// without compiler contraction: (a + 1) (high - low) / 2 + low, applied twice under quirk Q1 (a_delta with
// reference_compat).  Every kernel -- classic, work-queue, streaming, feature-masked, fused rollout -- goes through
// this one function, so the held input is the same bits everywhere, and the same bits as the oracle's.  (Round 1
// folded the map into one FMA per action; the two extra flops are invisible next to an RK step, and a last-bit
// difference of the input is what the stability-limited adaptive case cannot tolerate: tests/helpers.py.)
PCG_DEV double action_map(double a, double lo, double hi, bool norm, bool twice) {
#pragma clang fp contract(off)
  double av = a;
  if (norm) av = (av + 1.0) * (hi - lo) * 0.5 + lo;
  if (twice) av = (av + 1.0) * (hi - lo) * 0.5 + lo;
  return av;
}
template <int W>
PCG_DEV Pack<W> action_map(const Pack<W>& a, double lo, double hi, bool norm, bool twice) {
  Pack<W> r;
#pragma unroll
  for (int j = 0; j < W; ++j) r.v[j] = action_map(a.v[j], lo, hi, norm, twice);
  return r;
}

// What the pre-integration half of a step hands to the post-integration half (registers in the classic kernel,
// partly LDS in the work-queue kernel): the held input vector, the disturbance slots, the t == 0 verdict.
template <class M>
struct EnvPre {
  double u[M::NA + M::NDM];   // physical action | model disturbance inputs, held over [0,dt]
  double dv[PCG_MAX_NDM];     // configured disturbance values (observation slots, constraint rows)
  bool done_pre;              // pre-step constraint check at t == 0 said "done"
};

// ---- first half of make_env.step (pcgym.py:371-420): action map, disturbance injection, pre-step check ----
template <class M, bool PER_ENV_T, bool EXTRAS>
PCG_DEV void env_pre(const StepArgs& A, CDevConst& c, const double* sched_l, int64_t e, int t,
                     const double (&a_in)[M::NA], const double (&x)[M::NX], EnvPre<M>& pre) {
#pragma clang fp contract(off)
  constexpr int NX = M::NX, NA = M::NA, NDM = M::NDM;
  const int64_t B = A.B;
  const uint32_t flags = c.flags;
  const int nx = M::DYNAMIC ? c.nx : NX;
  const int na = M::DYNAMIC ? c.na : NA;
  const int N = c.N, nsp = c.nsp, nso = c.nsp_obs, nd = c.nd;
  const int tn = min(t + 1, N - 1);  // schedule index clamp (the reference would IndexError)
  const uint64_t env_id = (uint64_t)(A.env_offset + e);
  double (&u)[NA + NDM] = pre.u;
  double (&dv)[PCG_MAX_NDM] = pre.dv;
  // ---- action map (pcgym.py:371-383): action_map(), bit-identical to the oracle's held input ----
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    double av = 0.0;
    if (i < na) {
      av = action_map(a_in[i], c.a_lo[i], c.a_hi[i], (flags & PCG_F_NORMALISE_A) != 0,
                      (flags & PCG_F_A_DELTA) && (flags & PCG_F_REF_COMPAT));
      if (EXTRAS && (flags & PCG_F_A_DELTA)) {
        av = A.a_save[(size_t)i * B + e] + av;  // Q2: the unclipped sum drives the plant
        A.a_save[(size_t)i * B + e] = fmin(fmax(av, c.a_act_lo[i]), c.a_act_hi[i]);
      }
    }
    u[i] = av;
  }
  // ---- disturbance injection (pcgym.py:386-412) ----
#pragma unroll
  for (int k = 0; k < PCG_MAX_NDM; ++k) dv[k] = 0.0;
#pragma unroll
  for (int j = 0; j < NDM; ++j) u[NA + j] = c.d_default[j];
  if (NDM > 0 && nd > 0) {
#pragma unroll
    for (int k = 0; k < (NDM > 0 ? NDM : 1); ++k) {
      if (k < nd) {
        double v = (EXTRAS && A.d) ? A.d[(size_t)k * B + e] : sched_at<PER_ENV_T>(A.sched, sched_l, A.sched_in_lds, nsp + k, N, tn);
        if (EXTRAS && (flags & PCG_F_GAUSS_DIST)) {
          double z0, z1;
          rng_normal2(A.seed, env_id, (uint32_t)t, RNG_DIST + (uint32_t)(k >> 1), z0, z1);
          v += c.d_sigma[k] * ((k & 1) ? z1 : z0);
          v = fmin(fmax(v, c.d_lo[k]), c.d_hi[k]);
        }
        dv[k] = v;
        const int slot = c.d_slot[k];
#pragma unroll
        for (int j = 0; j < NDM; ++j) u[NA + j] = (j == slot) ? v : u[NA + j];
      }
    }
  }
  // ---- pre-step constraint check at t == 0 (pcgym.py:414-420) ----
  pre.done_pre = false;
  if (EXTRAS && c.ncon > 0 && t == 0) {
    double sp0[PCG_MAX_NSP];
#pragma unroll
    for (int k = 0; k < PCG_MAX_NSP; ++k) sp0[k] = (k < nso) ? c.x0[(M::DYNAMIC ? nx : NX) + k] : 0.0;
    const bool v = constraint_rows<M>(c, x, sp0, dv, u, A.g_pre, B, e);
    pre.done_pre = v && (flags & PCG_F_DONE_ON_CONS);
  }
}
// The three accumulating terms of the declarative tracking reward as exactly specified operation sequences (no contraction),
// shared by every kernel that states the reward: env_post and env_step_feat (pcg_step_feat.hpp; until r26 a third statement,
// env_post_cons).  Under the compiler's default contraction each restatement of `cost += a * b` became an FMA or a
// multiply and an add kernel by kernel: rollout_cons_actor_kernel<cstr, RK4> and the feature-masked step kernel gave tracking
// rewards that differ in the last bit, where pcg_rollout_cons.hpp promises the per-step route's bits.  The order is the
// oracle's (pcg_oracle.c: one `cost +=` per term).  What these take as arguments -- the normalisations (v - lo) * inv, a
// subtraction followed by a multiplication -- has nothing to fuse; the rest of each restatement is not covered by this.
PCG_DEV double track_sp_cost(double cost, double xn, double sn, double r_scale) {
#pragma clang fp contract(off)
  const double d = xn - sn;
  return cost + (d * d) * r_scale;
}
PCG_DEV double track_act_cost(double cost, double R_du, double R_u, double un, double upn) {
#pragma clang fp contract(off)
  const double d = un - upn;
  cost = cost + R_du * (d * d);
  return cost + R_u * (un * un);
}
PCG_DEV double track_box_cost(double cost, double xn, double lon, double hin) {
#pragma clang fp contract(off)
  if (xn > hin) return cost + (xn - hin) * (xn - hin);
  if (xn < lon) return cost + (lon - xn) * (lon - xn);
  return cost;
}

// ---- second half of make_env.step (pcgym.py:432-498): SP slot, constraints, done, reward, observation ----
// `x` is the integrated state, `status` what the integrator reported for this env.  `Rows` says where the post-step constraint
// rows come from: StepRows, the rows as pcg_step sums and stores them (constraint_rows into A.g where the plan has any), or a
// type whose static rows<M>(c, x, spv, dv, u, row_args...) -> "any row > 0" sums and stores them itself (ConsRows,
// pcg_rollout_cons.hpp).  Its operands travel as trailing arguments, scalars by value: gathered in one struct (by value or by
// reference alike), or as a pack of forwarding references, the constrained cstr kernels came out with register moves in
// another order than with env_post restated (profiles/r26/cons_step_refactor.txt).
struct StepRows {};
template <class M, bool PER_ENV_T, bool EXTRAS, bool UNC = false, class Rows = StepRows, class... RowArgs>
PCG_DEV void env_post(const StepArgs& A, CDevConst& c, const double* sched_l, int64_t e, int t, const EnvPre<M>& pre,
                      const double (&x)[M::NX], int status, EnvOut<M>& out, RowArgs... row_args) {
  constexpr int NX = M::NX, NA = M::NA;
  const int64_t B = A.B;
  const uint32_t flags = c.flags;
  const int nx = M::DYNAMIC ? c.nx : NX;
  const int na = M::DYNAMIC ? c.na : NA;
  const int N = c.N, nsp = c.nsp, nso = c.nsp_obs, nd = c.nd;
  const int tn = min(t + 1, N - 1);
  const int tc = min(t, N - 1);
  const uint64_t env_id = (uint64_t)(A.env_offset + e);
  const double (&u)[NA + M::NDM] = pre.u;
  const double (&dv)[PCG_MAX_NDM] = pre.dv;
  bool done = pre.done_pre;
  out.status = (uint8_t)status;
  // ---- SP slot uses SP[t_old] (pcgym.py:432-438, quirk Q5); t += 1 ----
  double spv[PCG_MAX_NSP] = {0.0, 0.0, 0.0, 0.0};
  double spn[PCG_MAX_NSP] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < PCG_MAX_NSP; ++k)
    if (k < nsp) {
      spv[k] = sched_at<PER_ENV_T>(A.sched, sched_l, A.sched_in_lds, k, N, tc);
      spn[k] = sched_at<PER_ENV_T>(A.sched, sched_l, A.sched_in_lds, k, N, tn);
    }
  const int t_new = t + 1;
  // ---- post-step constraints (pcgym.py:443-446) ----
  bool violated = false;
  if constexpr (tt::is_same<Rows, StepRows>::value) {
    if (EXTRAS && c.ncon > 0) {
      violated = constraint_rows<M>(c, x, spv, dv, u, A.g, B, e);
      done |= violated && (flags & PCG_F_DONE_ON_CONS);
    }
  } else {
    violated = Rows::template rows<M>(c, x, spv, dv, u, row_args...);
    done |= violated && (flags & PCG_F_DONE_ON_CONS);
  }
  done |= (t_new == N - 1);  // pcgym.py:448-449
  out.done = done;
  out.viol = violated;
  // ---- reward on the noise-free state (pcgym.py:470-482) ----
  double r = 0.0;
  if (EXTRAS && (flags & PCG_F_REWARD_BATCH)) {  // pcgym.py:502-532
    if (t_new == N - 1) {
      for (int k = 0; k < c.nrew; ++k) {
        const double v = pick<NX>(x, c.rew_index[k]) * c.r_scale[k];
        r = (flags & PCG_F_MAXIMISE) ? r + v : r - v;
      }
      if ((flags & PCG_F_R_PENALTY) && violated) r -= 1000.0;
    }
  } else {  // pcgym.py:535-558
#pragma unroll
    for (int k = 0; k < PCG_MAX_NSP; ++k)
      if (k < nsp) {
        const double dd = pick<NX>(x, c.sp_index[k]) - spn[k];
        r += (-(dd * dd)) * c.r_scale[k];
        if ((flags & PCG_F_R_PENALTY) && violated) r -= 1000.0;  // Q4: once per SP key
      }
  }
  out.rew = r;
  // ---- observation: noise (pcgym.py:452-466), normalise (:483-489), mask (:495-498) ----
  double zn[NX];
  if (EXTRAS && (flags & PCG_F_NOISE)) {
#pragma unroll
    for (int i = 0; i < NX; i += 2) {
      double z0, z1;
      rng_normal2(A.seed, env_id, (uint32_t)t, RNG_NOISE + (uint32_t)(i >> 1), z0, z1);
      zn[i] = z0;
      if (i + 1 < NX) zn[i + 1] = z1;
    }
  }
  double on[NX];  // physical observation of the states, noise included (what custom_reward receives, pcgym.py:470-471)
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    on[i] = 0.0;
    if (i < nx) {
      double o = x[i];
      if (EXTRAS && (flags & PCG_F_NOISE)) o += zn[i] * x[i] * c.noise_pct[i];
      on[i] = o;
      out.ox[i] = (o - c.omap[i].lo) * c.omap[i].sc + c.omap[i].off;
    }
  }
  if (EXTRAS && (flags & PCG_F_REWARD_TRACK)) {
    // declarative form of the paper's custom_reward family (custom_reward.py:3-39; constraint_showcase/
    // custom_reward.py:6-69): normalised squared tracking error at SP[t_new], squared normalised action increment
    // (and level), squared normalised box excess while a constraint row is violated
    double cost = 0.0;
#pragma unroll
    for (int k = 0; k < PCG_MAX_NSP; ++k)
      if (k < nsp) {
        double xv = pick<NX>(on, c.sp_index[k]);
        if constexpr (tt::is_same<M, Model<PCG_MODEL_CRYST>>::value) {
          if (flags & PCG_F_REWARD_CRYST) {  // cryst_train.py:24-25: CV and Ln from the observed moments
            if (c.sp_index[k] == 5) xv = sqrt(on[2] * on[0] / (on[1] * on[1]) - 1.0);
            if (c.sp_index[k] == 6) xv = on[1] / on[0];
          }
        }
        const double xn = (xv - c.trk_lo[k]) * c.trk_inv[k];
        const double sn = (spn[k] - c.trk_lo[k]) * c.trk_inv[k];
        cost = track_sp_cost(cost, xn, sn, c.r_scale[k]);
      }
#pragma unroll
    for (int j = 0; j < NA; ++j)
      if (j < na) {
        const double up0 = A.u_prev[(size_t)j * B + e];
        const double up = (up0 == up0) ? up0 : u[j];  // NaN: no previous action yet (hasattr branch, :7-8)
        const double un = (u[j] - c.act_lo[j]) * c.act_inv[j];
        const double upn = (up - c.act_lo[j]) * c.act_inv[j];
        cost = track_act_cost(cost, c.R_du, c.R_u, un, upn);
        A.u_prev[(size_t)j * B + e] = u[j];
      }
    if (violated)
      for (int q = 0; q < c.nbox; ++q) {
        const double xn = (pick<NX>(on, c.box_index[q]) - c.box_lo[q]) * c.box_inv[q];
        cost = track_box_cost(cost, xn, c.box_lon[q], c.box_hin[q]);
      }
    out.rew = -cost;
  }
#ifdef PCG_USER_REWARD
  {  // the callable form of custom_reward(self, obs, uk, violated) (pcgym.py:470-471): obs = the noisy physical vector
    double of[PCG_MAX_NOBS], xf[PCG_MAX_NOBS], uu[KNU];
    state_vector<M>(c, on, spv, dv, of);
    state_vector<M>(c, x, spv, dv, xf);
#pragma unroll
    for (int j = 0; j < KNU; ++j) uu[j] = (j < NA + M::NDM) ? u[j < NA + M::NDM ? j : 0] : 0.0;
    out.rew = pcg_user_reward(of, xf, uu, spn, violated ? 1 : 0, t_new, N);
  }
#endif
#pragma unroll
  for (int k = 0; k < PCG_MAX_NSP; ++k)
    if (k < nso) out.osp[k] = (spv[k] - c.omap[nx + k].lo) * c.omap[nx + k].sc + c.omap[nx + k].off;
#pragma unroll
  for (int k = 0; k < PCG_MAX_NDM; ++k)
    if (k < nd) out.od[k] = (dv[k] - c.omap[nx + nso + k].lo) * c.omap[nx + nso + k].sc + c.omap[nx + nso + k].off;
  if constexpr (UNC) {
    // static indices into the register array (a run-time trip count would put ounc[] -- and with it the lane's
    // rebuilt parameter block -- into scratch memory: measured 31.0 -> see profiles/r2/unc_probe.txt)
#pragma unroll
    for (int j = 0; j < PCG_MAX_NUNC; ++j) {
      if (j < c.nunc) {
        const int q = nx + nso + nd + j;
        out.ounc[j] = (A.p_unc[(size_t)j * B + e] - c.omap[q].lo) * c.omap[q].sc + c.omap[q].off;
      }
    }
  }
}


// ---------------------------------------------------------------------------
// One env step for the lane's environment: env_pre -> integrate over [0,dt] -> env_post.  Statement order follows
// make_env.step (pcgym.py:350-500).  `x` is the lane's physical state (in/out); everything the hot path writes
// comes back in `out` (registers).  Only the rare side outputs (a_save, constraint rows, DOPRI5 step counts) are
// stored on the way.
// ---------------------------------------------------------------------------
template <class M, int INTEG, bool PER_ENV_T, bool LDS_STAGES, bool EXTRAS, bool UNC = false>
PCG_DEV void env_step(const StepArgs& A, CDevConst& c, const double* sched_l, double* stage_l, int64_t e,
                      int t, const double (&a_in)[M::NA], double (&x)[M::NX], EnvOut<M>& out) {
  constexpr int NX = M::NX, NA = M::NA, NDM = M::NDM;
  const int64_t B = A.B;
  const int nx = M::DYNAMIC ? c.nx : NX;
  typename M::CKP& kp = model_kp<M>(c);
  EnvPre<M> pre;
  env_pre<M, PER_ENV_T, EXTRAS>(A, c, sched_l, e, t, a_in, x, pre);
  // ---- integrate over [0, dt], u held (pcgym.py:423-429, integrator.py:90-107,163-182) ----
  int status;
  if constexpr (UNC && !M::DYNAMIC) {
    // per-env uncertain parameters (sampled at reset, pcgym.py:301-310): rebuild the folded model constants
    // for this lane from the raw parameter vector with the env's values substituted
    constexpr int NR = M::NRAW;
    double raw[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) raw[i] = c.raw[i];
#pragma unroll
    for (int j = 0; j < PCG_MAX_NUNC; ++j) {
      if (j < c.nunc) {
        const double v = A.p_unc[(size_t)j * B + e];
        const int idx = c.unc_index[j];
#pragma unroll
        for (int i = 0; i < NR; ++i) raw[i] = (i == idx) ? v : raw[i];
      }
    }
    typename M::KP kpl;
    double dd[PCG_MAX_NDM] = {0.0, 0.0, 0.0, 0.0};
    M::prep(raw, NX, NA, reinterpret_cast<double*>(&kpl), dd);
    // unconfigured disturbance inputs take the env's own (possibly uncertain) model parameters (pcgym.py:400-404);
    // configured ones keep their schedule value (quirk Q11: layout [x | SP | d | unc] in reset and step)
#pragma unroll
    for (int j = 0; j < NDM; ++j) {
      bool configured = false;
#pragma unroll
      for (int k = 0; k < NDM; ++k) configured = configured || (k < c.nd && c.ndm != 0 && c.d_slot[k] == j);
      if (!configured) pre.u[NA + j] = dd[j];
    }
    status = integrate_env<M, INTEG, LDS_STAGES>(A, c, kpl, pre.u, x, stage_l, e, nx);
  } else {
    status = integrate_env<M, INTEG, LDS_STAGES>(A, c, kp, pre.u, x, stage_l, e, nx);
  }
  if constexpr (INTEG == PCG_INT_RK4G || INTEG == PCG_INT_T5G) {
    if (status == PCG_ST_PENDING) {  // nothing of this env's step has been stored: the fix-up launch redoes it from x_t
      out.status = PCG_ST_PENDING;
      return;
    }
  }
  env_post<M, PER_ENV_T, EXTRAS, UNC>(A, c, sched_l, e, t, pre, x, status, out);
}

// scalar (8 B per lane) store of one env's outputs; obs_base = &obs[0][e] of the destination
template <class M, bool UNC = false>
PCG_DEV void store_obs(const StepArgs& A, CDevConst& c, const EnvOut<M>& out, double* obs_base, int64_t B) {
  // B here is the component stride of the destination
  const int nx = M::DYNAMIC ? c.nx : M::NX;
  const int nso = c.nsp_obs, nd = c.nd;
#pragma unroll
  for (int i = 0; i < M::NX; ++i)
    if (i < nx) obs_base[(size_t)i * B] = out.ox[i];
#pragma unroll
  for (int k = 0; k < PCG_MAX_NSP; ++k)
    if (k < nso) obs_base[(size_t)(nx + k) * B] = out.osp[k];
#pragma unroll
  for (int k = 0; k < PCG_MAX_NDM; ++k)
    if (k < nd) obs_base[(size_t)(nx + nso + k) * B] = out.od[k];
  if constexpr (UNC)
#pragma unroll
    for (int j = 0; j < PCG_MAX_NUNC; ++j)
      if (j < c.nunc) obs_base[(size_t)(nx + nso + nd + j) * B] = out.ounc[j];
}

template <class M, bool UNC = false>
PCG_DEV void store_out(const StepArgs& A, CDevConst& c, int64_t e, const EnvOut<M>& out, double* obs_base) {
  // observation and reward are write-once streams: non-temporal stores keep them out of the L2 working set
  // (measured on the lean path: 20.1 -> 18.7 us per launch)
  const int64_t B = A.B;
  const int nx = M::DYNAMIC ? c.nx : M::NX;
  const int nso = c.nsp_obs, nd = c.nd;
#pragma unroll
  for (int i = 0; i < M::NX; ++i)
    if (i < nx) __builtin_nontemporal_store(out.ox[i], obs_base + (size_t)i * B);
#pragma unroll
  for (int k = 0; k < PCG_MAX_NSP; ++k)
    if (k < nso) __builtin_nontemporal_store(out.osp[k], obs_base + (size_t)(nx + k) * B);
#pragma unroll
  for (int k = 0; k < PCG_MAX_NDM; ++k)
    if (k < nd) __builtin_nontemporal_store(out.od[k], obs_base + (size_t)(nx + nso + k) * B);
  if constexpr (UNC)
#pragma unroll
    for (int j = 0; j < PCG_MAX_NUNC; ++j)
      if (j < c.nunc) __builtin_nontemporal_store(out.ounc[j], obs_base + (size_t)(nx + nso + nd + j) * B);
  __builtin_nontemporal_store(out.rew, A.rew + e);
  A.done[e] = out.done ? 1 : 0;
  if (A.viol) A.viol[e] = out.viol ? 1 : 0;
  if (A.status && out.status != PCG_ST_OK) A.status[e] = out.status;  // sticky: only failures are written
}

// cooperative copy of the schedules into LDS (per-env-t kernels)
PCG_DEV void stage_schedules(const StepArgs& A, CDevConst& c, double* sched_l) {
  if (A.sched_in_lds) {
    const int n = (c.nsp + c.nd) * c.N;
    for (int i = threadIdx.x; i < n; i += blockDim.x) sched_l[i] = A.sched[i];
    __syncthreads();
  }
}

template <class M, int INTEG, bool PER_ENV_T, bool LDS_STAGES, bool EXTRAS, bool UNC = false>
__global__ __launch_bounds__(tb(LDS_STAGES, INTEG, M::NX, ros_structured<M>::value),
                             wpe(M::NX, INTEG, LDS_STAGES, ros_structured<M>::value)) void step_kernel(const StepArgs A) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  CDevConst& c = *A.C;
  constexpr int NX = M::NX, NA = M::NA;
  double* stage_l = lds;
  double* sched_l = lds + integ_lds_doubles(NX, INTEG, LDS_STAGES, ros_structured<M>::value);
  if (PER_ENV_T) stage_schedules(A, c, sched_l);
  const int64_t e = (int64_t)blockIdx.x * tb(LDS_STAGES, INTEG, M::NX, ros_structured<M>::value) + threadIdx.x;
  if (e >= A.B) return;
  const int64_t B = A.B;
  const int nx = M::DYNAMIC ? c.nx : NX;
  const int na = M::DYNAMIC ? c.na : NA;
  const int t = PER_ENV_T ? A.t[e] : A.t_scalar;
  double x[NX], a[NA];
#pragma unroll
  for (int i = 0; i < NX; ++i) x[i] = (i < nx) ? A.x[(size_t)i * B + e] : 0.0;
#pragma unroll
  for (int i = 0; i < NA; ++i) a[i] = (i < na) ? A.a[(size_t)i * B + e] : 0.0;
  EnvOut<M> out;
  env_step<M, INTEG, PER_ENV_T, LDS_STAGES, EXTRAS, UNC>(A, c, sched_l, stage_l, e, t, a, x, out);
  if constexpr (INTEG == PCG_INT_RK4G || INTEG == PCG_INT_T5G) {
    if (out.status == PCG_ST_PENDING) {
      A.done[e] = PCG_DONE_PENDING;
      return;
    }
  }
  if (A.auto_reset && out.done) {
    // gymnasium "same-step" auto-reset in the same launch: reward / done / viol of the finished step are kept,
    // state, observation, step counter (and a_delta accumulator, per-env parameters) are those of the new episode
    __builtin_nontemporal_store(out.rew, A.rew + e);
    A.done[e] = 1;
    if (A.viol) A.viol[e] = out.viol ? 1 : 0;
    if (A.status && out.status != PCG_ST_OK) A.status[e] = out.status;  // sticky: only failures are written
    reset_env(A, c, e, A.reset_seed);
    return;
  }
#pragma unroll
  for (int i = 0; i < NX; ++i)
    if (i < nx) A.x[(size_t)i * B + e] = x[i];
  store_out<M, UNC>(A, c, e, out, A.obs + e);
  if (PER_ENV_T) A.t[e] = t + 1;
}

// Open-loop fused rollout: T env steps with x in registers ("next" row f-1).
// UNC: per-env uncertain parameters (p_unc, sampled by the reset that precedes the episode: pcgym.py:300-316), as in
// step_kernel<..., UNC>.
template <class M, int INTEG, bool LDS_STAGES, bool UNC = false>
__global__ __launch_bounds__(tb(LDS_STAGES, INTEG)) void rollout_kernel(const StepArgs A) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  CDevConst& c = *A.C;
  constexpr int NX = M::NX, NA = M::NA;
  const int64_t e = (int64_t)blockIdx.x * tb(LDS_STAGES, INTEG) + threadIdx.x;
  if (e >= A.B) return;
  const int64_t B = A.B;
  const int nx = M::DYNAMIC ? c.nx : NX;
  const int na = M::DYNAMIC ? c.na : NA;
  const int nobs = c.nobs;
  double x[NX], a[NA];
#pragma unroll
  for (int i = 0; i < NX; ++i) x[i] = (i < nx) ? A.x[(size_t)i * B + e] : 0.0;
  for (int s = 0; s < A.T; ++s) {
    const double* as = A.a_seq + (size_t)s * A.a_ss;
#pragma unroll
    for (int i = 0; i < NA; ++i) a[i] = (i < na) ? as[(size_t)i * A.a_cs + e] : 0.0;
    const bool last = (s == A.T - 1);
    EnvOut<M> out;
    env_step<M, INTEG, false, LDS_STAGES, true, UNC>(A, c, lds, lds, e, A.t_scalar + s, a, x, out);
    if constexpr (INTEG == PCG_INT_RK4G || INTEG == PCG_INT_T5G) {
      // first pass of the barrier-free rollout (A.fixup: pcg_rollout_flat.hpp): the guard did not trust this step -- nothing
      // of it has been stored and x is the step's start state again; the env leaves this pass here, with the step it stopped at
      if (out.status == PCG_ST_PENDING) {
        A.flat_tstar[e] = s;
        A.flat_hot[atomicAdd(A.flat_q + 1, 1)] = (int32_t)e;
        break;
      }
    }
    if (A.rew_seq) A.rew_seq[(size_t)s * A.r_ss + e] = out.rew;
    if (A.obs_seq) store_obs<M, UNC>(A, c, out, A.obs_seq + (size_t)s * A.o_ss + e, A.o_cs);
    if (last || !A.obs_seq) store_out<M, UNC>(A, c, e, out, A.obs + e);  // io->obs/rew/done hold the last step
  }
#pragma unroll
  for (int i = 0; i < NX; ++i)
    if (i < nx) A.x[(size_t)i * B + e] = x[i];
}

// test hooks ------------------------------------------------------------------
template <class M>
__global__ __launch_bounds__(BLOCK) void rhs_kernel(CDevConst* C, int64_t B, int nu_rows, const double* xg,
                                                    const double* ug, double* dxg) {
  CDevConst& c = *C;
  constexpr int NX = M::NX, NA = M::NA, NDM = M::NDM;
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= B) return;
  const int nx = M::DYNAMIC ? c.nx : NX;
  const int na = M::DYNAMIC ? c.na : NA;
  double x[NX], dx[NX], u[NA + NDM];
#pragma unroll
  for (int i = 0; i < NX; ++i) x[i] = (i < nx) ? xg[(size_t)i * B + e] : 0.0;
#pragma unroll
  for (int i = 0; i < NA; ++i) u[i] = (i < na) ? ug[(size_t)i * B + e] : 0.0;
#pragma unroll
  for (int j = 0; j < NDM; ++j) u[NA + j] = (na + j < nu_rows) ? ug[(size_t)(na + j) * B + e] : c.d_default[j];
  typename M::CKP& kp = model_kp<M>(c);
  const typename M::Hold hold = M::hold(kp, u);
  M::rhs(kp, hold, x, dx);
#pragma unroll
  for (int i = 0; i < NX; ++i)
    if (i < nx) dxg[(size_t)i * B + e] = dx[i];
}

template <class M, int INTEG, bool LDS_STAGES>
__global__ __launch_bounds__(tb(LDS_STAGES, INTEG, M::NX, ros_structured<M>::value)) void integrate_kernel(CDevConst* C, int64_t B, int nu_rows,
                                                                          double* xg, const double* ug, int32_t* nsteps) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  CDevConst& c = *C;
  constexpr int NX = M::NX, NA = M::NA, NDM = M::NDM;
  const int64_t e = (int64_t)blockIdx.x * tb(LDS_STAGES, INTEG, NX, ros_structured<M>::value) + threadIdx.x;
  if (e >= B) return;
  const int nx = M::DYNAMIC ? c.nx : NX;
  const int na = M::DYNAMIC ? c.na : NA;
  double x[NX], u[NA + NDM];
#pragma unroll
  for (int i = 0; i < NX; ++i) x[i] = (i < nx) ? xg[(size_t)i * B + e] : 0.0;
#pragma unroll
  for (int i = 0; i < NA; ++i) u[i] = (i < na) ? ug[(size_t)i * B + e] : 0.0;
#pragma unroll
  for (int j = 0; j < NDM; ++j) u[NA + j] = (na + j < nu_rows) ? ug[(size_t)(na + j) * B + e] : c.d_default[j];
  typename M::CKP& kp = model_kp<M>(c);
  const typename M::Hold hold = M::hold(kp, u);
  const RhsFn<M> f{kp, hold};
  if (INTEG == PCG_INT_RK4) {
    rk4<NX>(f, x, c.h, c.h2, c.h6, c.substeps);
  } else if (INTEG == PCG_INT_RODAS3) {
    int nacc = 0, nrej = 0;
    const RosLds<NX> Lm(lds);
    const int status = rodas3<NX>(f, Lm, x, nx, c.dt, c.rtol, c.atol, c.max_steps, nacc, nrej);
    poison_if_failed<NX>(status, x);
    if (nsteps) {
      nsteps[e] = nacc;
      nsteps[B + e] = nrej;
    }
  } else if (INTEG == PCG_INT_CV8) {
    cv8<NX>(f, x, c.h, c.substeps);
  } else if (INTEG == PCG_INT_RK4G || INTEG == PCG_INT_T5G) {
    int nacc = 0, nrej = 0;
    guarded_env<M, INTEG>(f, kp, hold, x, c, nx, nacc, nrej);
    if (nsteps) {
      nsteps[e] = nacc;
      nsteps[B + e] = nrej;
    }
  } else if (INTEG == PCG_INT_TSIT5) {
    int nacc = 0, nrej = 0;
    const int status = tsit5<NX>(f, x, nx, c.dt, c.rtol, c.atol, c.max_steps, nacc, nrej);
    poison_if_failed<NX>(status, x);
    if (nsteps) {
      nsteps[e] = nacc;
      nsteps[B + e] = nrej;
    }
  } else if (is_ros_pair(INTEG)) {
    int nacc = 0, nrej = 0, status;
    const EpWeights<M, typename M::CKP> ep{kp, u, c.ep_c, c.ep_kmax};
    if constexpr (ros_structured<M>::value) {
      if (!seulex8_if_heavy<M>(kp, hold, u, f, ep, x, nx, c.dt, c.rtol, c.atol, c.max_steps, c.coop_thr, nacc, nrej, status)) {
        const RosStructured<M, typename M::CKP> ls{kp, hold, {}};
        status = ros_pair<INTEG, NX>(f, ls, ep, x, nx, c.dt, c.rtol, c.atol, c.max_steps, nacc, nrej);
      }
    } else {
      const RosLds<NX> Lm(lds);
      const RosDense<NX, RhsFn<M>> ls{f, Lm, nx, c.rtol, c.atol};
      status = ros_pair<INTEG, NX>(f, ls, ep, x, nx, c.dt, c.rtol, c.atol, c.max_steps, nacc, nrej);
    }
    poison_if_failed<NX>(status, x);
    if (nsteps) {
      nsteps[e] = nacc;
      nsteps[B + e] = nrej;
    }
  } else {
    int nacc = 0, nrej = 0, status;
    if (LDS_STAGES) {
      LdsStages<NX, BLOCK_LDS> K{lds + threadIdx.x};
      status = dopri5<NX>(f, K, x, nx, c.dt, c.rtol, c.atol, c.max_steps, nacc, nrej);
    } else {
      RegStages<NX> K;
      status = dopri5<NX>(f, K, x, nx, c.dt, c.rtol, c.atol, c.max_steps, nacc, nrej);
    }
    poison_if_failed<NX>(status, x);
    if (nsteps) {
      nsteps[e] = nacc;
      nsteps[B + e] = nrej;
    }
  }
#pragma unroll
  for (int i = 0; i < NX; ++i)
    if (i < nx) xg[(size_t)i * B + e] = x[i];
}

}  // namespace pcg
#include "pcg_lean.hpp"
#include "pcg_step_queue.hpp"
#include "pcg_rollout_flat.hpp"
// (also under hipRTC: a plan's second run-time compiled module instantiates the two closed-loop kernels, pcg_abi_jit.hip jit_closed_loop)
#include "pcg_rollout_policy.hpp"
#include "pcg_rollout_actor.hpp"
#ifndef __HIPCC_RTC__
// (ahead-of-time only: a plan's run-time compiled closed-loop module carries the fp64 kernels alone)
#include "pcg_rollout_policy_f32.hpp"
// (... nor the kernels of the plans with constraint rows: such a plan with run-time compiled code steps)
#include "pcg_rollout_cons.hpp"
// (... nor those of the plans with per-env parameters, which refuse run-time compiled code at creation)
#include "pcg_rollout_unc.hpp"
// (... nor the population forms of the fp64 and float32 policy kernels, which refuse run-time compiled plans)
#include "pcg_rollout_pop.hpp"
// (... nor the population forms on plans with per-env parameters)
#include "pcg_rollout_pop_unc.hpp"
// (... nor the population forms on plans with constraint rows)
#include "pcg_rollout_pop_cons.hpp"
#endif
namespace pcg {

using StepFn = void (*)(const StepArgs);
using PolFn = void (*)(const StepArgs, const PolicyArgs);
using ActFn = void (*)(const StepArgs, const ActorArgs);
#ifndef __HIPCC_RTC__
using PolConsFn = void (*)(const StepArgs, const PolicyArgs, const ConsArgs);
using ActConsFn = void (*)(const StepArgs, const ActorArgs, const ConsArgs);
using PopFn = void (*)(const StepArgs, const PopArgs);
using PopConsFn = void (*)(const StepArgs, const PopConsArgs, const ConsArgs);
#endif

#ifndef __HIPCC_RTC__
// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
using RhsKFn = void (*)(CDevConst*, int64_t, int, const double*, const double*, double*);
using IntKFn = void (*)(CDevConst*, int64_t, int, double*, const double*, int32_t*);

// one instantiation of the feature-masked small-model kernel (pcg_step_feat.hpp): serves every launch whose
// needs are a subset of `mask`
struct FeatEntry {
  unsigned mask;
  StepFn fn;
};
constexpr int MAX_FEAT = 16;
// tables of the two small HBM-bound models, built in their own translation unit (pcg_inst_k.hip)
int feat_fill_cstr(FeatEntry* out, int cap);
int feat_fill_four_tank(FeatEntry* out, int cap);
template <int ID>
inline int feat_fill(FeatEntry*, int) { return 0; }
template <>
inline int feat_fill<PCG_MODEL_CSTR>(FeatEntry* o, int cap) { return feat_fill_cstr(o, cap); }
template <>
inline int feat_fill<PCG_MODEL_FOUR_TANK>(FeatEntry* o, int cap) { return feat_fill_four_tank(o, cap); }

struct Kernels {
  FeatEntry feat[MAX_FEAT];          // feature-masked pipelined kernels, 2 envs per lane (RK4, small models)
  int nfeat;
  StepFn step[PCG_INT_COUNT][2][2][2];  // [integrator][per_env_t][lds_stages][extras]
  StepFn stream[PCG_INT_COUNT][2];      // persistent streaming kernel [integrator][EPL-1] (entries may be null)
  StepFn step_unc[PCG_INT_COUNT][2]; // per-env parameter uncertainty [integrator][per_env_t] (null for affine)
  StepFn queue[2];                   // DOPRI5 with the in-workgroup work queue [per_env_t] (null for affine)
  StepFn queue_fix[2];               // ... the fix-up launch of a guarded plan (models with a guard hook)
  StepFn queue_w[2];                 // ... 512-thread workgroups: both waves of a SIMD on ONE tile (models with a cost key, <= 256 registers)
  StepFn queue_r4[2];                // Rodas4 through the same work queue [per_env_t] (models with structured W only)
  StepFn queue_r4w1[2];              // ... compiled for ONE workgroup per CU (no register spills in the loop)
  StepFn queue_r5[2], queue_r5w1[2]; // the same two for the fifth-order pair (PCG_INT_RODAS5)
  bool ros_structured;               // Rodas4 runs in registers (launch shape of the explicit adaptive pair)
  bool coop;                         // ... and the model has a cooperative rule (cfg.coop_thr, pcg_seulex.hpp)
  bool queue_default;                // route adaptive plans to it unless told otherwise (models with a cost key)
  size_t (*queue_lds)(int);          // LDS bytes of a tile of T slots
  size_t (*queue_lds_x)(int);        // ... with the tile's state parked in LDS as well
  size_t (*queue_lds_x_lean)(int, int);  // ... in the lean layout (tile size, stored input rows: pcg_step_queue.hpp QTile)
  StepFn pipe[2][2];                 // software-pipelined lean kernel [lean_scheme(integrator)][EPL-1] (may be null)
  StepFn pipe_ar[2][2];              // the same with the same-launch auto-reset path compiled in
  StepFn chain[2];                   // a run of RK4 steps of a recorded step graph as one launch [EPL-1] (where pipe[0] exists)
  StepFn roll_lean[2];               // RK4 lean fused rollout [EPL-1] (may be null)
  StepFn rollout[PCG_INT_COUNT][2];  // [integrator][lds_stages]
  StepFn rollout_unc[PCG_INT_COUNT]; // fused rollout with per-env parameters (RK4, DOPRI5; null for affine)
  StepFn roll_hot;                   // second pass of the barrier-free rollout of a PCG_INT_T5G plan (models with a guard)
  PolFn roll_policy[2];              // closed-loop fused rollout with an on-device MLP policy [lean_scheme(integrator)]
  ActFn roll_actor[2];               // ... with a Gaussian actor (sampled action, log-prob) and an optional critic
  PolFn roll_policy_f32[2];          // the same two with the networks evaluated in float32 (pcg_rollout_policy_f32.hpp)
  ActFn roll_actor_f32[2];
  PolConsFn roll_policy_cons[2];     // the fp64 two on plans with constraint rows, recording the rows (pcg_rollout_cons.hpp)
  ActConsFn roll_actor_cons[2];
  PolFn roll_policy_unc;             // the fp64 two on plans with per-env parameters (RK4; null for affine: pcg_rollout_unc.hpp)
  ActFn roll_actor_unc;
  PopFn roll_policy_pop[2];          // roll_policy with one member of a policy population per slice of envs (pcg_rollout_pop.hpp)
  PopFn roll_policy_pop_f32[2];      // ... of a float32 population (pcg_policy_pop_create_f32)
  PopFn roll_policy_pop_unc, roll_policy_pop_unc_f32;  // the population two on plans with per-env parameters (RK4; null for affine: pcg_rollout_pop_unc.hpp)
  PopConsFn roll_policy_pop_cons[2];      // the population two on plans with constraint rows, with the violation statistics
  PopConsFn roll_policy_pop_cons_f32[2];  // (pcg_rollout_pop_cons.hpp)
  RhsKFn rhs;
  IntKFn integ[PCG_INT_COUNT][2];
  int nx, na, ndm, nraw;
  bool dynamic, has_lds_stages;
  void (*prep)(const double*, int, int, double*, double*);
  size_t kp_bytes;
};

template <int ID>
Kernels make_kernels() {
  using M = Model<ID>;
  Kernels k;
  std::memset(&k, 0, sizeof(k));
  k.step[PCG_INT_RK4][0][0][0] = step_kernel<M, PCG_INT_RK4, false, false, false>;
  k.step[PCG_INT_RK4][0][0][1] = step_kernel<M, PCG_INT_RK4, false, false, true>;
  k.step[PCG_INT_RK4][1][0][0] = step_kernel<M, PCG_INT_RK4, true, false, false>;
  k.step[PCG_INT_RK4][1][0][1] = step_kernel<M, PCG_INT_RK4, true, false, true>;
  k.step[PCG_INT_DOPRI5][0][0][0] = step_kernel<M, PCG_INT_DOPRI5, false, false, false>;
  k.step[PCG_INT_DOPRI5][0][0][1] = step_kernel<M, PCG_INT_DOPRI5, false, false, true>;
  k.step[PCG_INT_DOPRI5][1][0][0] = step_kernel<M, PCG_INT_DOPRI5, true, false, false>;
  k.step[PCG_INT_DOPRI5][1][0][1] = step_kernel<M, PCG_INT_DOPRI5, true, false, true>;
  k.rollout[PCG_INT_RK4][0] = rollout_kernel<M, PCG_INT_RK4, false>;
  k.rollout[PCG_INT_DOPRI5][0] = rollout_kernel<M, PCG_INT_DOPRI5, false>;
  k.integ[PCG_INT_RK4][0] = integrate_kernel<M, PCG_INT_RK4, false>;
  k.integ[PCG_INT_DOPRI5][0] = integrate_kernel<M, PCG_INT_DOPRI5, false>;
  // stiff-capable Rosenbrock integrator: general kernel only (one wave per workgroup, per-lane matrices in LDS)
  k.step[PCG_INT_RODAS3][0][0][0] = k.step[PCG_INT_RODAS3][0][0][1] = step_kernel<M, PCG_INT_RODAS3, false, false, true>;
  k.step[PCG_INT_RODAS3][1][0][0] = k.step[PCG_INT_RODAS3][1][0][1] = step_kernel<M, PCG_INT_RODAS3, true, false, true>;
  k.integ[PCG_INT_RODAS3][0] = integrate_kernel<M, PCG_INT_RODAS3, false>;
  // fourth-order Rosenbrock pair: general kernel (dense W in LDS, or the model's structured W in registers), and for
  // the structured models the work-queue kernel
  k.step[PCG_INT_RODAS4][0][0][0] = k.step[PCG_INT_RODAS4][0][0][1] = step_kernel<M, PCG_INT_RODAS4, false, false, true>;
  k.step[PCG_INT_RODAS4][1][0][0] = k.step[PCG_INT_RODAS4][1][0][1] = step_kernel<M, PCG_INT_RODAS4, true, false, true>;
  k.integ[PCG_INT_RODAS4][0] = integrate_kernel<M, PCG_INT_RODAS4, false>;
  // fifth-order Rosenbrock pair: the same set
  k.step[PCG_INT_RODAS5][0][0][0] = k.step[PCG_INT_RODAS5][0][0][1] = step_kernel<M, PCG_INT_RODAS5, false, false, true>;
  k.step[PCG_INT_RODAS5][1][0][0] = k.step[PCG_INT_RODAS5][1][0][1] = step_kernel<M, PCG_INT_RODAS5, true, false, true>;
  k.integ[PCG_INT_RODAS5][0] = integrate_kernel<M, PCG_INT_RODAS5, false>;
  k.ros_structured = ros_structured<M>::value;
  k.coop = ros_structured<M>::value && has_coop<M>::value;
  // guarded RK4 (models with a guard hook): general kernel, integration hook, fused rollout
  if constexpr (has_guard<M>::value) {
    k.step[PCG_INT_RK4G][0][0][0] = k.step[PCG_INT_RK4G][0][0][1] = step_kernel<M, PCG_INT_RK4G, false, false, true>;
    k.step[PCG_INT_RK4G][1][0][0] = k.step[PCG_INT_RK4G][1][0][1] = step_kernel<M, PCG_INT_RK4G, true, false, true>;
    k.integ[PCG_INT_RK4G][0] = k.integ[PCG_INT_RK4G][1] = integrate_kernel<M, PCG_INT_RK4G, false>;
    k.rollout[PCG_INT_RK4G][0] = k.rollout[PCG_INT_RK4G][1] = rollout_kernel<M, PCG_INT_RK4G, false>;
  }
  if constexpr (has_guard<M>::value && !M::DYNAMIC) k.roll_hot = rollout_kernel_hot<M>;
  if constexpr (has_guard<M>::value) {  // guarded fixed-step Tsit5: the same set
    k.step[PCG_INT_T5G][0][0][0] = k.step[PCG_INT_T5G][0][0][1] = step_kernel<M, PCG_INT_T5G, false, false, true>;
    k.step[PCG_INT_T5G][1][0][0] = k.step[PCG_INT_T5G][1][0][1] = step_kernel<M, PCG_INT_T5G, true, false, true>;
    k.integ[PCG_INT_T5G][0] = k.integ[PCG_INT_T5G][1] = integrate_kernel<M, PCG_INT_T5G, false>;
    k.rollout[PCG_INT_T5G][0] = k.rollout[PCG_INT_T5G][1] = rollout_kernel<M, PCG_INT_T5G, false>;
  }
  // fixed-step order-8 method: general kernel, integration hook, fused rollout (launch shape of RK4)
  k.step[PCG_INT_CV8][0][0][0] = k.step[PCG_INT_CV8][0][0][1] = step_kernel<M, PCG_INT_CV8, false, false, true>;
  k.step[PCG_INT_CV8][1][0][0] = k.step[PCG_INT_CV8][1][0][1] = step_kernel<M, PCG_INT_CV8, true, false, true>;
  k.integ[PCG_INT_CV8][0] = k.integ[PCG_INT_CV8][1] = integrate_kernel<M, PCG_INT_CV8, false>;
  k.rollout[PCG_INT_CV8][0] = k.rollout[PCG_INT_CV8][1] = rollout_kernel<M, PCG_INT_CV8, false>;
  // closed-loop fused rollout (pcg_rollout_policy.hpp): the two fixed-step schemes, beside their open-loop kernels
  k.roll_policy[lean_scheme(PCG_INT_RK4)] = rollout_policy_kernel<M, PCG_INT_RK4>;
  k.roll_policy[lean_scheme(PCG_INT_CV8)] = rollout_policy_kernel<M, PCG_INT_CV8>;
  k.roll_policy_pop[lean_scheme(PCG_INT_RK4)] = rollout_pop_policy_kernel<M, PCG_INT_RK4>;
  k.roll_policy_pop[lean_scheme(PCG_INT_CV8)] = rollout_pop_policy_kernel<M, PCG_INT_CV8>;
  k.roll_policy_pop_f32[lean_scheme(PCG_INT_RK4)] = rollout_pop_policy_kernel_f32<M, PCG_INT_RK4>;
  k.roll_policy_pop_f32[lean_scheme(PCG_INT_CV8)] = rollout_pop_policy_kernel_f32<M, PCG_INT_CV8>;
  k.roll_actor[lean_scheme(PCG_INT_RK4)] = rollout_actor_kernel<M, PCG_INT_RK4>;
  k.roll_actor[lean_scheme(PCG_INT_CV8)] = rollout_actor_kernel<M, PCG_INT_CV8>;
  k.roll_policy_f32[lean_scheme(PCG_INT_RK4)] = rollout_policy_kernel_f32<M, PCG_INT_RK4>;
  k.roll_policy_f32[lean_scheme(PCG_INT_CV8)] = rollout_policy_kernel_f32<M, PCG_INT_CV8>;
  k.roll_actor_f32[lean_scheme(PCG_INT_RK4)] = rollout_actor_kernel_f32<M, PCG_INT_RK4>;
  k.roll_actor_f32[lean_scheme(PCG_INT_CV8)] = rollout_actor_kernel_f32<M, PCG_INT_CV8>;
  k.roll_policy_cons[lean_scheme(PCG_INT_RK4)] = rollout_cons_policy_kernel<M, PCG_INT_RK4>;
  k.roll_policy_cons[lean_scheme(PCG_INT_CV8)] = rollout_cons_policy_kernel<M, PCG_INT_CV8>;
  k.roll_policy_pop_cons[lean_scheme(PCG_INT_RK4)] = rollout_pop_cons_policy_kernel<M, PCG_INT_RK4>;
  k.roll_policy_pop_cons[lean_scheme(PCG_INT_CV8)] = rollout_pop_cons_policy_kernel<M, PCG_INT_CV8>;
  k.roll_policy_pop_cons_f32[lean_scheme(PCG_INT_RK4)] = rollout_pop_cons_policy_kernel_f32<M, PCG_INT_RK4>;
  k.roll_policy_pop_cons_f32[lean_scheme(PCG_INT_CV8)] = rollout_pop_cons_policy_kernel_f32<M, PCG_INT_CV8>;
  k.roll_actor_cons[lean_scheme(PCG_INT_RK4)] = rollout_cons_actor_kernel<M, PCG_INT_RK4>;
  k.roll_actor_cons[lean_scheme(PCG_INT_CV8)] = rollout_cons_actor_kernel<M, PCG_INT_CV8>;
  // Tsit5 (the reference's jax method): general kernel, both counter modes, and the integration hook
  k.step[PCG_INT_TSIT5][0][0][0] = k.step[PCG_INT_TSIT5][0][0][1] = step_kernel<M, PCG_INT_TSIT5, false, false, true>;
  k.step[PCG_INT_TSIT5][1][0][0] = k.step[PCG_INT_TSIT5][1][0][1] = step_kernel<M, PCG_INT_TSIT5, true, false, true>;
  k.integ[PCG_INT_TSIT5][0] = k.integ[PCG_INT_TSIT5][1] = integrate_kernel<M, PCG_INT_TSIT5, false>;
  if constexpr (ros_structured<M>::value && !M::DYNAMIC) {
    k.queue_r4[0] = step_kernel_queue<M, false, true, PCG_INT_RODAS4>;
    k.queue_r4[1] = step_kernel_queue<M, true, true, PCG_INT_RODAS4>;
    k.queue_r4w1[0] = step_kernel_queue<M, false, true, PCG_INT_RODAS4, 1>;
    k.queue_r4w1[1] = step_kernel_queue<M, true, true, PCG_INT_RODAS4, 1>;
    // registers only: the fused rollout works as for the explicit pair (64-thread workgroups, no LDS)
    k.rollout[PCG_INT_RODAS4][0] = k.rollout[PCG_INT_RODAS4][1] = rollout_kernel<M, PCG_INT_RODAS4, false>;
    k.queue_r5[0] = step_kernel_queue<M, false, true, PCG_INT_RODAS5>;
    k.queue_r5[1] = step_kernel_queue<M, true, true, PCG_INT_RODAS5>;
    k.queue_r5w1[0] = step_kernel_queue<M, false, true, PCG_INT_RODAS5, 1>;
    k.queue_r5w1[1] = step_kernel_queue<M, true, true, PCG_INT_RODAS5, 1>;
    k.rollout[PCG_INT_RODAS5][0] = k.rollout[PCG_INT_RODAS5][1] = rollout_kernel<M, PCG_INT_RODAS5, false>;
  }
  k.rhs = rhs_kernel<M>;
  if constexpr (!M::DYNAMIC) {
    k.queue[0] = step_kernel_queue<M, false, true>;
    k.queue[1] = step_kernel_queue<M, true, true>;
    k.queue_lds = QLayout<M>::bytes;
    k.queue_lds_x = QLayout<M>::bytes_x;
    k.queue_lds_x_lean = QLayout<M>::bytes_x_lean;
    // Measured (tools/user_model_probe.py, cstr B = 2^20 at 1e-8: ~4 attempts per env step): 90 us through the queue
    // against 38 us for the classic kernel -- sorting, parking and refilling cost more than a cheap env's whole
    // integration.  The queue is the default only where a model declares a cost key, i.e. where the step count is
    // large and predictable from the input (the extraction models: 1.12-1.23x); PCG_OPT_VARIANT 5 routes any model to it.
    k.queue_default = has_cost_key<M>::value;
    if constexpr (has_guard<M>::value) {
      k.queue_fix[0] = step_kernel_queue<M, false, true, PCG_INT_DOPRI5, 0, QBLOCK, true>;
      k.queue_fix[1] = step_kernel_queue<M, true, true, PCG_INT_DOPRI5, 0, QBLOCK, true>;
    }
    // (only where the 256-thread build already runs two waves per SIMD.  The 20-state cascade was tried: at 512 threads its
    // loop is allocated 256 registers with ~10 scratch accesses per attempt, but a second wave buys 9 % of issue rate
    // (3.85 against 4.24 us of SIMD time per attempt) and two envs per lane instead of four cost more: 0.345 against 0.327 ms)
    if constexpr (has_cost_key<M>::value && wpe(M::NX, PCG_INT_DOPRI5, false) >= 2) {
      k.queue_w[0] = step_kernel_queue<M, false, true, PCG_INT_DOPRI5, 0, 2 * QBLOCK>;
      k.queue_w[1] = step_kernel_queue<M, true, true, PCG_INT_DOPRI5, 0, 2 * QBLOCK>;
    }
    k.step_unc[PCG_INT_RK4][0] = step_kernel<M, PCG_INT_RK4, false, false, true, true>;
    k.step_unc[PCG_INT_RK4][1] = step_kernel<M, PCG_INT_RK4, true, false, true, true>;
    k.step_unc[PCG_INT_DOPRI5][0] = step_kernel<M, PCG_INT_DOPRI5, false, false, true, true>;
    k.step_unc[PCG_INT_DOPRI5][1] = step_kernel<M, PCG_INT_DOPRI5, true, false, true, true>;
    k.rollout_unc[PCG_INT_RK4] = rollout_kernel<M, PCG_INT_RK4, false, true>;
    k.rollout_unc[PCG_INT_DOPRI5] = rollout_kernel<M, PCG_INT_DOPRI5, false, true>;
    k.roll_policy_unc = rollout_unc_policy_kernel<M>;
    k.roll_actor_unc = rollout_unc_actor_kernel<M>;
    k.roll_policy_pop_unc = rollout_pop_unc_policy_kernel<M>;
    k.roll_policy_pop_unc_f32 = rollout_pop_unc_policy_kernel_f32<M>;
  }
  if constexpr (M::FULL) {
    // DOPRI5 with the stage vectors in LDS (PCG_OPT_LDS_STAGES)
    k.step[PCG_INT_DOPRI5][0][1][0] = step_kernel<M, PCG_INT_DOPRI5, false, true, false>;
    k.step[PCG_INT_DOPRI5][0][1][1] = step_kernel<M, PCG_INT_DOPRI5, false, true, true>;
    k.step[PCG_INT_DOPRI5][1][1][0] = step_kernel<M, PCG_INT_DOPRI5, true, true, false>;
    k.step[PCG_INT_DOPRI5][1][1][1] = step_kernel<M, PCG_INT_DOPRI5, true, true, true>;
    k.rollout[PCG_INT_DOPRI5][1] = rollout_kernel<M, PCG_INT_DOPRI5, true>;
    k.integ[PCG_INT_DOPRI5][1] = integrate_kernel<M, PCG_INT_DOPRI5, true>;
    // streaming / pipelined lean kernels
    k.roll_lean[0] = rollout_kernel_lean<M, 1>;
    k.stream[PCG_INT_RK4][0] = step_kernel_stream<M, PCG_INT_RK4, 1, 1>;
    // (rounds 1-5 also shipped step_kernel_stream<M, PCG_INT_DOPRI5>: reachable only through the measurement switch
    // PCG_OPT_VARIANT 2, never a default -- adaptive plans take the work queue or the classic kernel -- and launched by no
    // test: removed in round 6 with the kernel-coverage gate, tests/test_zz_kernel_coverage.py)
    // several envs per lane only where the per-env register footprint is
    // small (the HBM-bound models)
    if constexpr (M::NX <= 4) {
      k.roll_lean[1] = rollout_kernel_lean<M, 2>;
      k.pipe[0][0] = step_kernel_pipe<M, 1>;
      k.pipe[0][1] = step_kernel_pipe<M, 2>;
      k.pipe_ar[0][0] = step_kernel_pipe<M, 1, true>;
      k.pipe_ar[0][1] = step_kernel_pipe<M, 2, true>;
      k.chain[0] = step_chain_kernel<M, 1>;
      k.chain[1] = step_chain_kernel<M, 2>;
      // the order-8 scheme keeps more stage vectors alive: two envs per lane only where that fits 128 registers (four
      // waves per SIMD, and room beside the work-queue kernels of a mixed batch) without spilling
      k.pipe[1][0] = step_kernel_pipe<M, 1, false, PCG_INT_CV8>;
      k.pipe_ar[1][0] = step_kernel_pipe<M, 1, true, PCG_INT_CV8>;
      // (measured on four_tank, 4 states: two envs per lane at once spill at 128 registers, one after the other is no
      // faster than one env per lane -- 45.1 against 43.3 us per 2^20-env step -- and writes its spills to HBM)
      if constexpr (M::NX <= 2) {
        k.pipe[1][1] = step_kernel_pipe<M, 2, false, PCG_INT_CV8>;
        k.pipe_ar[1][1] = step_kernel_pipe<M, 2, true, PCG_INT_CV8>;
      }
      k.stream[PCG_INT_RK4][1] = step_kernel_stream<M, PCG_INT_RK4, 2, 1>;
    }
  }
  // where no LDS-stage / RK4 variant exists the plain one is used
  for (int pe = 0; pe < 2; ++pe)
    for (int ex = 0; ex < 2; ++ex) {
      k.step[PCG_INT_RK4][pe][1][ex] = k.step[PCG_INT_RK4][pe][0][ex];
      k.step[PCG_INT_RODAS3][pe][1][ex] = k.step[PCG_INT_RODAS3][pe][0][ex];
      k.step[PCG_INT_RODAS4][pe][1][ex] = k.step[PCG_INT_RODAS4][pe][0][ex];
      k.step[PCG_INT_RODAS5][pe][1][ex] = k.step[PCG_INT_RODAS5][pe][0][ex];
      k.step[PCG_INT_TSIT5][pe][1][ex] = k.step[PCG_INT_TSIT5][pe][0][ex];
      k.step[PCG_INT_RK4G][pe][1][ex] = k.step[PCG_INT_RK4G][pe][0][ex];
      k.step[PCG_INT_T5G][pe][1][ex] = k.step[PCG_INT_T5G][pe][0][ex];
      k.step[PCG_INT_CV8][pe][1][ex] = k.step[PCG_INT_CV8][pe][0][ex];
      if (!k.step[PCG_INT_DOPRI5][pe][1][ex]) k.step[PCG_INT_DOPRI5][pe][1][ex] = k.step[PCG_INT_DOPRI5][pe][0][ex];
    }
  k.rollout[PCG_INT_RK4][1] = k.rollout[PCG_INT_RK4][0];
  if (!k.rollout[PCG_INT_DOPRI5][1]) k.rollout[PCG_INT_DOPRI5][1] = k.rollout[PCG_INT_DOPRI5][0];
  k.integ[PCG_INT_RK4][1] = k.integ[PCG_INT_RK4][0];
  k.integ[PCG_INT_RODAS3][1] = k.integ[PCG_INT_RODAS3][0];
  k.integ[PCG_INT_RODAS4][1] = k.integ[PCG_INT_RODAS4][0];
  k.integ[PCG_INT_RODAS5][1] = k.integ[PCG_INT_RODAS5][0];
  if (!k.integ[PCG_INT_DOPRI5][1]) k.integ[PCG_INT_DOPRI5][1] = k.integ[PCG_INT_DOPRI5][0];
  k.nfeat = feat_fill<ID>(k.feat, MAX_FEAT);
  k.has_lds_stages = M::FULL;
  k.nx = M::NX;
  k.na = M::NA;
  k.ndm = M::NDM;
  k.nraw = M::NRAW;
  k.dynamic = M::DYNAMIC;
  k.prep = M::prep;
  k.kp_bytes = sizeof(typename M::KP);
  return k;
}

#endif  // !__HIPCC_RTC__

}  // namespace pcg
