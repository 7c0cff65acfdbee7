// pcg_rollout_policy_f32.hpp -- the closed-loop fused rollouts of pcg_rollout_policy.hpp / pcg_rollout_actor.hpp with the
// NETWORK evaluated in float32 (pcg_policy_create_f32): the env arithmetic stays fp64 throughout, only what happens between
// two env steps changes.  stable-baselines3's MlpPolicy is a float32 module; policy.predict(obs) in the reference is a
// float32 forward pass, and the fp64 tanh is most of what the fp64 evaluator costs.
//
// THE ARITHMETIC IS THE SPECIFICATION:
//   input       in32[i] = (float)obs[i], round to nearest (part of the specification, not an error term);
//   per unit    the sum starts from the unit's bias and takes ONE IEEE float32 FMA per input, inputs ascending
//               (a packed FMA, v_pk_fma_f32, is exactly that in each of its halves);
//   activation  tanhf, or ReLU with NaN -> 0 as in pol_act; a NaN stays a NaN under tanhf;
//   result      the last layer's float32 output, widened to double exactly;
//   deterministic policy (rollout_policy_kernel_f32): PCG_POL_NONE / PCG_POL_CLIP act on the widened value with the
//               float32-rounded box; PCG_POL_TANH is tanhf BEFORE the widening -- so every recorded policy output is exactly
//               a float32 value;
//   actor (rollout_actor_kernel_f32), all in fp64 exactly as in rollout_actor_kernel: mu = the widened raw output,
//               u = fma(sigma, z, mu), a = clip(u) with the rounded box, logp from z, value = the widened critic output.
//
// Weights: one device block per policy behind the PolicyDev header of the fp64 form, offsets counted in FLOATS, read through
// the constant address space with wave-uniform addresses.  Every matrix is zero-padded to the unroll blocks below (padding
// units are exact zeros: tanhf(0) = relu(0) = 0), and the rows of two consecutive OUTPUT units are interleaved:
//     element (r, k) of layer l sits at  offW[l] + ((r / 2) * ld[l] + k) * 2 + (r & 1)
// so that one 64-bit scalar operand holds the weights two units give the same input, and a two-unit float2 accumulator takes
// them with the input broadcast: v_pk_fma_f32.  Biases are plain vectors (a pair of units is contiguous anyway).
// The first hidden layer is 64 registers (128 in fp64); the second is streamed into the output layer as there.
//
// NOT for plans with run-time compiled code (user models, reward expressions): their closed-loop module instantiates the
// fp64 kernels only; pcg_rollout_policy / pcg_rollout_actor refuse a float32 policy there (PCG_E_UNSUPPORTED) and the Python
// collectors step instead.  No LDS, no mutable plan or policy state: capture-safe, usable from several streams.
#pragma once

#include "pcg_policy_layout.hpp"  // POL32_OR

namespace pcg {

typedef float pol_f2 __attribute__((ext_vector_type(2)));

PCG_DEV float pol_act32(float v, int act) {
  if (act == PCG_ACT_TANH) return tanhf(v);
  return v > 0.0f ? v : 0.0f;  // (NaN -> 0, as pol_act)
}

// the pair of weights units (2 p, 2 p + 1) of a layer give input k; W points at the pair's interleaved rows
PCG_DEV pol_f2 pol_w2(const PCG_CONSTANT float* W, int k) {
  return *reinterpret_cast<const PCG_CONSTANT pol_f2*>(W + 2 * k);
}
PCG_DEV pol_f2 pol_fma2(pol_f2 w, float x, pol_f2 acc) {
  const pol_f2 xx = {x, x};
  return __builtin_elementwise_fma(w, xx, acc);
}

// first hidden layer from the observation, POL_HB units (POL_HB / 2 pairs) per trip
template <int NIN>
PCG_DEV void pol32_first(const PCG_CONSTANT PolicyDev& P, const PCG_CONSTANT float* D, const float (&in)[NIN],
                         float (&h)[POL_MAX_W]) {
  const int ld = P.ld[0], n_in = P.n_in, act = P.act;
#pragma unroll
  for (int k = 0; k < POL_MAX_W; ++k) h[k] = 0.0f;
  const int nb = (P.w[0] + POL_HB - 1) / POL_HB;
  for (int jb = 0; jb < nb; ++jb) {
    const PCG_CONSTANT float* W = D + P.offW[0] + (size_t)jb * POL_HB * ld;
    const PCG_CONSTANT float* b = D + P.offb[0] + jb * POL_HB;
    pol_f2 acc[POL_HB / 2];
#pragma unroll
    for (int r = 0; r < POL_HB / 2; ++r) acc[r] = pol_w2(b, r);
#pragma unroll
    for (int ib = 0; ib < NIN / POL_IB; ++ib) {
      if (ib * POL_IB < n_in) {
#pragma unroll
        for (int i = 0; i < POL_IB; ++i)
#pragma unroll
          for (int r = 0; r < POL_HB / 2; ++r) acc[r] = pol_fma2(pol_w2(W + 2 * r * ld, ib * POL_IB + i), in[ib * POL_IB + i], acc[r]);
      }
    }
#pragma unroll
    for (int q = 0; q < POL_MAX_W / POL_HB; ++q) {
      if (jb == q) {  // (uniform: the register array is only ever indexed by constants)
#pragma unroll
        for (int r = 0; r < POL_HB / 2; ++r) {
          h[q * POL_HB + 2 * r] = pol_act32(acc[r].x, act);
          h[q * POL_HB + 2 * r + 1] = pol_act32(acc[r].y, act);
        }
      }
    }
  }
}

// R2 pairs of units of layer `L` from h[0 .. width), from unit j0 (even) on
template <int R2>
PCG_DEV void pol32_rows_from_h(const PCG_CONSTANT PolicyDev& P, const PCG_CONSTANT float* D, int L, int j0, int width,
                               const float (&h)[POL_MAX_W], pol_f2 (&acc)[R2]) {
  const int ld = P.ld[L];
  const PCG_CONSTANT float* W = D + P.offW[L] + (size_t)j0 * ld;
  const PCG_CONSTANT float* b = D + P.offb[L] + j0;
#pragma unroll
  for (int r = 0; r < R2; ++r) acc[r] = pol_w2(b, r);
#pragma unroll
  for (int kb = 0; kb < POL_MAX_W / POL_HB; ++kb) {
    if (kb * POL_HB < width) {
#pragma unroll
      for (int k = 0; k < POL_HB; ++k)
#pragma unroll
        for (int r = 0; r < R2; ++r) acc[r] = pol_fma2(pol_w2(W + 2 * r * ld, kb * POL_HB + k), h[kb * POL_HB + k], acc[r]);
    }
  }
}

// out = the last layer's float32 output BEFORE the output map.  `in`: the fp64 observation vector, rounded to float32 here.
template <int NIN, int NA>
PCG_DEV void policy_raw_f32(const PCG_CONSTANT PolicyDev& P, const double (&in)[NIN], float (&out)[NA]) {
  static_assert(NIN % POL_IB == 0 && NA <= PCG_MAX_NA, "policy_raw_f32: block sizes");
  constexpr int NA2 = (NA + 1) / 2;  // (an odd NA: the last pair's second half is a zero row or a row past n_out, dropped)
  const PCG_CONSTANT float* D = reinterpret_cast<const PCG_CONSTANT float*>(&P + 1);
  const int nh = P.n_hidden;
  float in32[NIN];
#pragma unroll
  for (int i = 0; i < NIN; ++i) in32[i] = (float)in[i];
  pol_f2 o2[NA2];
  if (nh == 0) {
    const int ld = P.ld[0], n_in = P.n_in;
    const PCG_CONSTANT float* W = D + P.offW[0];
    const PCG_CONSTANT float* b = D + P.offb[0];
#pragma unroll
    for (int o = 0; o < NA2; ++o) o2[o] = pol_w2(b, o);
#pragma unroll
    for (int ib = 0; ib < NIN / POL_IB; ++ib) {
      if (ib * POL_IB < n_in) {
#pragma unroll
        for (int i = 0; i < POL_IB; ++i)
#pragma unroll
          for (int o = 0; o < NA2; ++o) o2[o] = pol_fma2(pol_w2(W + 2 * o * ld, ib * POL_IB + i), in32[ib * POL_IB + i], o2[o]);
      }
    }
  } else {
    float h[POL_MAX_W];
    pol32_first<NIN>(P, D, in32, h);
    if (nh == 1) {
      pol32_rows_from_h<NA2>(P, D, 1, 0, P.w[0], h, o2);
    } else {
      // second hidden layer streamed into the output layer: POL_SB units at a time, consumed as soon as they are formed
      const int ld2 = P.ld[2], w0 = P.w[0], act = P.act;
      const PCG_CONSTANT float* W2 = D + P.offW[2];
      const PCG_CONSTANT float* b2 = D + P.offb[2];
#pragma unroll
      for (int o = 0; o < NA2; ++o) o2[o] = pol_w2(b2, o);
      const int nb = (P.w[1] + POL_SB - 1) / POL_SB;
      for (int jb = 0; jb < nb; ++jb) {
        pol_f2 h2[POL_SB / 2];
        pol32_rows_from_h<POL_SB / 2>(P, D, 1, jb * POL_SB, w0, h, h2);
#pragma unroll
        for (int r = 0; r < POL_SB; ++r) {
          const float hv = pol_act32((r & 1) ? h2[r / 2].y : h2[r / 2].x, act);
#pragma unroll
          for (int o = 0; o < NA2; ++o) o2[o] = pol_fma2(pol_w2(W2 + 2 * o * ld2, jb * POL_SB + r), hv, o2[o]);
        }
      }
    }
  }
#pragma unroll
  for (int o = 0; o < NA; ++o) out[o] = (o & 1) ? o2[o / 2].y : o2[o / 2].x;
}

// a = out_map(out) of the deterministic policy: tanhf before the widening, none / clip on the widened value
template <int NA>
PCG_DEV void policy_map_f32(const PCG_CONSTANT PolicyDev& P, const float (&out)[NA], double (&a)[NA]) {
  const int om = P.out_map;
  const double lo = P.out_lo, hi = P.out_hi;
#pragma unroll
  for (int o = 0; o < NA; ++o) {
    double v = (double)(om == PCG_POL_TANH ? tanhf(out[o]) : out[o]);
    if (om == PCG_POL_CLIP) v = v < lo ? lo : (v > hi ? hi : v);  // (a NaN stays a NaN)
    a[o] = v;
  }
}

// rollout_policy_kernel's loop (pcg_rollout_policy.hpp says why it is stated once per kernel) with the float32 evaluator.
// Waves per SIMD asked of the register allocator for the models of up to ten states: measured on the cstr at 2 / 3 / 4,
// tools/policy_rollout_bench.py --dtype float32 (profiles/r13/policy_f32.txt): 291 / 222 / 534 us per step with the 2 x 64
// policy, 57 / 52 / 81 with 1 x 16, 38 / 39 / 37 affine.  Two is kept although three is faster on the cstr: built for three
// waves, the distillation column's CV8 kernel no longer reproduces the open-loop general kernel's env step BITWISE (the
// compiler rounds the step differently under that register budget), and that replay is what ties every closed-loop kernel
// to the oracle-tested open-loop one (tests/test_gpu_policy_f32.py).
#ifndef PCG_POL32_WPE
#define PCG_POL32_WPE 2
#endif
template <class M, int INTEG>
__global__ __launch_bounds__(BLOCK, M::NX <= 10 ? PCG_POL32_WPE : 1) void rollout_policy_kernel_f32(const StepArgs A, const PolicyArgs Q) {
  CDevConst& c = *A.C;
  const PCG_CONSTANT PolicyDev& P = *Q.P;
  constexpr int NX = M::NX, NA = M::NA, NIN = policy_nin<M>();
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= A.B) return;
  const int64_t B = A.B;
  const int nx = M::DYNAMIC ? c.nx : NX;
  const int na = M::DYNAMIC ? c.na : NA;
  const int nobs = c.nobs;
  double x[NX], a[NA], in[NIN];
#pragma unroll
  for (int i = 0; i < NX; ++i) x[i] = (i < nx) ? A.x[(size_t)i * B + e] : 0.0;
#pragma unroll
  for (int i = 0; i < NIN; ++i) in[i] = (i < nobs) ? A.obs[(size_t)i * B + e] : 0.0;
  const int n_eval = A.T + ((Q.record_next && Q.a_out) ? 1 : 0);
  for (int s = 0; s < n_eval; ++s) {
    {
      float raw[NA];
      policy_raw_f32<NIN, NA>(P, in, raw);
      policy_map_f32<NA>(P, raw, a);
    }
    if (Q.a_out) {
      double* ao = Q.a_out + (size_t)s * Q.ao_ss + e;
#pragma unroll
      for (int i = 0; i < NA; ++i)
        if (i < na) ao[(size_t)i * Q.ao_cs] = a[i];
    }
    if (s == A.T) break;  // row T: policy(observation after the last step), recorded and not applied
    const bool last = (s == A.T - 1);
    EnvOut<M> out;
    env_step<M, INTEG, false, false, true>(A, c, nullptr, nullptr, e, A.t_scalar + s, a, x, out);
    if (A.rew_seq) A.rew_seq[(size_t)s * A.r_ss + e] = out.rew;
    if (A.obs_seq) store_obs<M>(A, c, out, A.obs_seq + (size_t)s * A.o_ss + e, A.o_cs);
    if (last) store_out<M>(A, c, e, out, A.obs + e);  // io->obs/rew/done hold the last step
    else if (A.status && out.status != PCG_ST_OK) A.status[e] = out.status;
    policy_input<M, NIN>(c, out, in);
  }
#pragma unroll
  for (int i = 0; i < NX; ++i)
    if (i < nx) A.x[(size_t)i * B + e] = x[i];
}

// rollout_actor_kernel's loop with both networks evaluated in float32; sample, map and log-probability in fp64 as there.
// Waves per SIMD, tools/actor_rollout_bench.py --dtype float32, same file: 753 / 841 / 1325 us per step with 2 x 64 actor and
// critic, 102 / 97 / 161 with 1 x 16, 61 / 67 / 65 affine -- two (the sampling and two networks' worth of live values)
#ifndef PCG_ACT32_WPE
#define PCG_ACT32_WPE 2
#endif
template <class M, int INTEG>
__global__ __launch_bounds__(BLOCK, M::NX <= 10 ? PCG_ACT32_WPE : 1) void rollout_actor_kernel_f32(const StepArgs A, const ActorArgs Q) {
  CDevConst& c = *A.C;
  const PCG_CONSTANT PolicyDev& P = *Q.P;
  constexpr int NX = M::NX, NA = M::NA, NIN = policy_nin<M>();
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= A.B) return;
  const int64_t B = A.B;
  const int nx = M::DYNAMIC ? c.nx : NX;
  const int na = M::DYNAMIC ? c.na : NA;
  const int nobs = c.nobs;
  const uint64_t env_id = (uint64_t)(A.env_offset + e);
  double x[NX], a[NA], in[NIN];
#pragma unroll
  for (int i = 0; i < NX; ++i) x[i] = (i < nx) ? A.x[(size_t)i * B + e] : 0.0;
#pragma unroll
  for (int i = 0; i < NIN; ++i) in[i] = (i < nobs) ? A.obs[(size_t)i * B + e] : 0.0;
  const bool any_out = Q.a_out || Q.u_out || Q.lp_out || Q.v_out;
  const int n_eval = A.T + ((Q.record_next && any_out) ? 1 : 0);
  for (int s = 0; s < n_eval; ++s) {
    double u[NA], z[NA + (NA & 1)];
    {
      float raw[NA];
      policy_raw_f32<NIN, NA>(P, in, raw);  // mu
#pragma unroll
      for (int i = 0; i < NA; ++i) u[i] = (double)raw[i];
    }
#pragma unroll
    for (int i = 0; i < NA; i += 2)
      if (i < na) rng_normal2(A.seed, env_id, (uint32_t)(A.t_scalar + s), RNG_POLICY + (uint32_t)(i >> 1), z[i], z[i + 1]);
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      if (i < na) {
        u[i] = __builtin_fma(Q.sigma[i], z[i], u[i]);
        q = __builtin_fma(z[i], z[i], q);
      }
    }
    policy_map<NA>(P, u, a);  // (none / clip in fp64 on the header's box, which holds the float32-rounded bounds)
    if (Q.a_out) {
      double* ao = Q.a_out + (size_t)s * Q.ao_ss + e;
#pragma unroll
      for (int i = 0; i < NA; ++i)
        if (i < na) ao[(size_t)i * Q.ao_cs] = a[i];
    }
    if (Q.u_out) {
      double* uo = Q.u_out + (size_t)s * Q.uo_ss + e;
#pragma unroll
      for (int i = 0; i < NA; ++i)
        if (i < na) uo[(size_t)i * Q.uo_cs] = u[i];
    }
    if (Q.lp_out) Q.lp_out[(size_t)s * Q.lp_ss + e] = __builtin_fma(-0.5, q, Q.c0);
    if (Q.V && Q.v_out) {  // (uniform)
      float v[1];
      policy_raw_f32<NIN, 1>(*Q.V, in, v);
      Q.v_out[(size_t)s * Q.v_ss + e] = (double)v[0];
    }
    if (s == A.T) break;  // row T: drawn at counter t0 + T, recorded and not applied (its value: the bootstrap value)
    const bool last = (s == A.T - 1);
    EnvOut<M> out;
    env_step<M, INTEG, false, false, true>(A, c, nullptr, nullptr, e, A.t_scalar + s, a, x, out);
    if (A.rew_seq) A.rew_seq[(size_t)s * A.r_ss + e] = out.rew;
    if (A.obs_seq) store_obs<M>(A, c, out, A.obs_seq + (size_t)s * A.o_ss + e, A.o_cs);
    if (last) store_out<M>(A, c, e, out, A.obs + e);  // io->obs/rew/done hold the last step
    else if (A.status && out.status != PCG_ST_OK) A.status[e] = out.status;
    policy_input<M, NIN>(c, out, in);
  }
#pragma unroll
  for (int i = 0; i < NX; ++i)
    if (i < nx) A.x[(size_t)i * B + e] = x[i];
}

}  // namespace pcg
