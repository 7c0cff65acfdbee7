// pcg_gae.hpp -- generalised advantage estimation (Schulman et al. 2016) over one recorded episode, all envs in ONE launch:
// the tail of collect_onpolicy (rollout.py), which was a loop of T steps of eager element-wise torch calls behind a
// collector that is itself one launch.  Interface after stable-baselines3's RolloutBuffer.compute_returns_and_advantage
// (its next_non_terminal is `!cut` here).
//
// One env per lane (two where the host found 16-byte accesses possible: gae_vec2_ok in pcg_abi_policy.hip), backwards in time:
//
//     cut   = term ? term[t] != 0 : false;   the last step is cut as well unless bootstrap_last
//     nxt   = cut ? 0.0 : val[t+1]           c = cut ? 0.0 : carry
//     delta = (rew[t] + gamma * nxt) - val[t]            three roundings
//     carry = delta + gl * c                             two roundings            (gl = gamma * lam, rounded once on the host)
//     adv[t] = carry;  ret[t] = carry + val[t]
//
// Every operation is rounded on its own -- contraction is OFF in this file's arithmetic and the products with zero stay --
// so the result equals the torch loop of rollout.gae(fused=False) bit for bit (NaN payloads aside), on both lane paths.
//
// Memory: 32 B per env step (rew, val in; adv, ret out; val[t+1] is the previous iteration's val[t], kept in registers), 33
// with term.  The recurrence is serial per lane but no address depends on it: the rows of GAE_DEPTH time steps are loaded
// as one group, and the next group is issued BEFORE the current one is consumed (two register sets, alternating, no
// copies), so that a lane has up to 2 * GAE_DEPTH rows in flight -- what carries a small batch, whose few waves cannot hide
// an HBM miss (~900 cycles) per time step by occupancy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pcg {

constexpr int GAE_BLOCK = 256;  // 4 waves, one per SIMD
#ifndef PCG_GAE_DEPTH
#define PCG_GAE_DEPTH 2  // (tools/gae_depth_bench.hip builds the kernel with other depths)
#endif
// time steps per group of loads; two groups alternate.  Depths 2, 4 and 8 (68 / 100 / 201 registers) were timed on two
// boxes (profiles/r17/gae_variants.txt): at B = 2^20 one box has depth 2 ahead by 12 %, the other depth 4 by 4 %, at B = 4096
// and 2^16 they agree to the repeats' spread -- no depth wins beyond the spread between boxes, so the one with the fewest
// registers is kept.
constexpr int GAE_DEPTH = PCG_GAE_DEPTH;

struct GaeArgs {
  int64_t B;
  int32_t T, bootstrap_last, vec2;
  double gamma, gl;
  const double* rew;
  const double* val;
  const uint8_t* term;
  double* adv;
  double* ret;
  int64_t rew_ss, val_ss, term_ss, adv_ss, ret_ss;
};

typedef double gae_d2 __attribute__((ext_vector_type(2)));

template <int EPL>
__device__ __forceinline__ void gae_load(const double* p, double (&v)[EPL]) {
  if constexpr (EPL == 2) {
    const gae_d2 w = *reinterpret_cast<const gae_d2*>(p);
    v[0] = w.x;
    v[1] = w.y;
  } else {
    v[0] = *p;
  }
}
template <int EPL>
__device__ __forceinline__ void gae_store(double* p, const double (&v)[EPL]) {
  if constexpr (EPL == 2) {
    *reinterpret_cast<gae_d2*>(p) = gae_d2{v[0], v[1]};
  } else {
    *p = v[0];
  }
}
// the flag bytes of a lane's EPL envs, one per byte of the word
template <int EPL>
__device__ __forceinline__ uint32_t gae_load_flags(const uint8_t* p) {
  if constexpr (EPL == 2) {
    return *reinterpret_cast<const uint16_t*>(p);
  } else {
    return *p;
  }
}

template <int EPL>
struct GaeGroup {  // the rows of GAE_DEPTH consecutive time steps, newest first
  double rew[GAE_DEPTH][EPL], val[GAE_DEPTH][EPL];
  uint32_t flags[GAE_DEPTH];
};

// rows t_hi, t_hi - 1, .. of the lane's envs (e: the first of them): the first m of them when PARTIAL, otherwise all
// GAE_DEPTH, where a row below 0 reads row 0 instead.  That is the group fetched past the episode's start by the last turn
// of the loop: fetching it without a test keeps the loop free of a branch around loads, at which the compiler would have to
// wait for EVERY load in flight (the wait counter of both paths, merged), i.e. give up the group issued ahead.  Row 0 has
// just been requested by the group before, so the redundant loads are cache hits; they are never consumed.
template <int EPL, bool TERM, bool PARTIAL>
__device__ __forceinline__ void gae_fetch(const GaeArgs& A, int64_t e, int32_t t_hi, int m, GaeGroup<EPL>& g) {
#pragma unroll
  for (int k = 0; k < GAE_DEPTH; ++k) {
    if (!PARTIAL || k < m) {
      const int32_t t = PARTIAL ? t_hi - k : max(t_hi - k, 0);
      gae_load<EPL>(A.rew + (int64_t)t * A.rew_ss + e, g.rew[k]);
      gae_load<EPL>(A.val + (int64_t)t * A.val_ss + e, g.val[k]);
      if constexpr (TERM) g.flags[k] = gae_load_flags<EPL>(A.term + (int64_t)t * A.term_ss + e);
    }
  }
}

// the recurrence over a fetched group; the PARTIAL group is the episode's newest, whose first step is cut when `end_cut`
template <int EPL, bool TERM, bool RET, bool PARTIAL>
__device__ __forceinline__ void gae_consume(const GaeArgs& A, int64_t e, int32_t t_hi, int m, bool end_cut, const GaeGroup<EPL>& g,
                                            double (&carry)[EPL], double (&vnext)[EPL]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < GAE_DEPTH; ++k) {
    if (!PARTIAL || k < m) {
      const int32_t t = t_hi - k;
      double adv[EPL], ret[EPL];
#pragma unroll
      for (int j = 0; j < EPL; ++j) {
        bool cut = PARTIAL && k == 0 && end_cut;
        if constexpr (TERM) cut = cut || ((g.flags[k] >> (8 * j)) & 0xffu) != 0;
        const double nxt = cut ? 0.0 : vnext[j];
        const double c = cut ? 0.0 : carry[j];
        const double gn = A.gamma * nxt;
        const double s = g.rew[k][j] + gn;
        const double delta = s - g.val[k][j];
        const double gc = A.gl * c;
        carry[j] = delta + gc;
        adv[j] = carry[j];
        ret[j] = carry[j] + g.val[k][j];
        vnext[j] = g.val[k][j];
      }
      gae_store<EPL>(A.adv + (int64_t)t * A.adv_ss + e, adv);
      if constexpr (RET) gae_store<EPL>(A.ret + (int64_t)t * A.ret_ss + e, ret);
    }
  }
}

template <int EPL, bool TERM, bool RET>
__device__ __forceinline__ void gae_lane(const GaeArgs& A) {
  const int64_t e = ((int64_t)blockIdx.x * GAE_BLOCK + threadIdx.x) * EPL;
  if (e >= A.B) return;  // (EPL == 2 only with an even B: e + 1 < B)
  double carry[EPL], vnext[EPL];
#pragma unroll
  for (int j = 0; j < EPL; ++j) carry[j] = 0.0;
  GaeGroup<EPL> ga, gb;
  // the newest 1 .. GAE_DEPTH steps form the partial group, so that what is left is whole groups: the loop has no per-row test
  const int m = 1 + (A.T - 1) % GAE_DEPTH;
  int32_t t = A.T - 1;
  gae_load<EPL>(A.val + (int64_t)A.T * A.val_ss + e, vnext);
  gae_fetch<EPL, TERM, true>(A, e, t, m, ga);
  gae_fetch<EPL, TERM, false>(A, e, t - m, 0, gb);
  gae_consume<EPL, TERM, RET, true>(A, e, t, m, !A.bootstrap_last, ga, carry, vnext);
  t -= m;
  while (t >= 0) {
    gae_fetch<EPL, TERM, false>(A, e, t - GAE_DEPTH, 0, ga);
    gae_consume<EPL, TERM, RET, false>(A, e, t, 0, false, gb, carry, vnext);
    t -= GAE_DEPTH;
    if (t < 0) break;
    gae_fetch<EPL, TERM, false>(A, e, t - GAE_DEPTH, 0, gb);
    gae_consume<EPL, TERM, RET, false>(A, e, t, 0, false, ga, carry, vnext);
    t -= GAE_DEPTH;
  }
}

template <int EPL>
__device__ __forceinline__ void gae_lane_pick(const GaeArgs& A) {
  if (A.term) {
    if (A.ret) gae_lane<EPL, true, true>(A);
    else gae_lane<EPL, true, false>(A);
  } else {
    if (A.ret) gae_lane<EPL, false, true>(A);
    else gae_lane<EPL, false, false>(A);
  }
}

// ONE shipped kernel: the lane path and the presence of `term` / `ret` are uniform run-time branches over the eight inlined
// bodies (its register count is the largest body's, two envs per lane with flags).  The coverage gate of
// tests/test_zz_kernel_coverage.py has one name to hold against the oracle; tests/test_gpu_gae.py holds every body against
// the torch loop and numpy bit for bit.
__global__ __launch_bounds__(GAE_BLOCK) void gae_kernel(const GaeArgs A) {
  if (A.vec2) gae_lane_pick<2>(A);
  else gae_lane_pick<1>(A);
}

}  // namespace pcg
