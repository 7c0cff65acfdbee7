// pcg_rollout_policy.hpp -- closed-loop fused rollout: T env steps with the state in registers AND the policy evaluated in the
// kernel between two steps (pcg_rollout_policy).  The policy is declarative, as the tracking reward is: a small fp64
// multi-layer perceptron (0, 1 or 2 hidden layers of at most 64 units, tanh / relu), the shape stable-baselines3's MlpPolicy
// produces, whose input is the observation the env emitted before the step -- exactly the numbers pcg_step would have
// written to io->obs -- and whose output is what the caller would have put into io->a.
//
// What the reference does per step (policy_evaluation.py:86-128): a = policy.predict(obs); obs, r, done = env.step(a), one env
// at a time in Python.  The per-step route of this library (collect_rollouts with a callable) costs one launch, one torch
// evaluation and one HBM round trip of obs and a per step; here neither obs nor a leaves the lane unless it is recorded.
//
// Arithmetic.  One env per lane, rollout_kernel's loop around env_step<M, INTEG, false, false, true>.  The weights are
// wave-uniform: they sit in one device block behind a PolicyDev header and are read through the constant address space
// with uniform addresses, i.e. by scalar loads into SGPRs, like the plan's DevConst.  Every product is an explicit fp64
// FMA with the weight as its scalar operand; a unit's sum starts from its bias and runs over its inputs in ascending
// order.  Only the first hidden layer (at most 64 doubles) is kept: the second hidden layer is streamed into the output
// layer four units at a time (four independent FMA chains), each unit consumed as soon as its activation is formed.
// The register arrays are indexed with compile-time constants only; the loops over OUTPUT units run at run time (one code
// body whatever the width), the loops over INPUT units are unrolled in blocks that a uniform branch skips past the layer's
// width.  The host pads every matrix with zero rows / columns / biases to those block sizes (pack_policy, pcg_policy_pack.hpp), and
// tanh(0) = relu(0) = 0, so padding units are exact zeros.
// No MFMA: v_mfma_f64_16x16x4_f64 over the wave's 64 envs needs the activations transposed through LDS between layers; the
// measured case for it is the 2 x 64 policy.
#pragma once

#include "pcg_policy_layout.hpp"  // PolicyDev and the block sizes POL_*

namespace pcg {

struct PolicyArgs {
  const PCG_CONSTANT PolicyDev* P;
  double* a_out;           // [T (+1)][na][B] recorded policy outputs, or null
  int64_t ao_ss, ao_cs;    // element strides (step, component)
  int32_t record_next;     // row T = policy(observation after the last step), not applied
};

PCG_DEV double pol_act(double v, int act) {
  if (act == PCG_ACT_TANH) return tanh(v);
  return v > 0.0 ? v : 0.0;  // (NaN -> 0, as torch.relu does not: a non-finite state is reported through `status`)
}

// first hidden layer from the observation: h[j] = act(b[j] + sum_i W[j][i] in[i]), POL_HB units per trip
template <int NIN>
PCG_DEV void pol_first(const PCG_CONSTANT PolicyDev& P, const PCG_CONSTANT double* D, const double (&in)[NIN],
                       double (&h)[POL_MAX_W]) {
  const int ld = P.ld[0], n_in = P.n_in, act = P.act;
#pragma unroll
  for (int k = 0; k < POL_MAX_W; ++k) h[k] = 0.0;
  const int nb = (P.w[0] + POL_HB - 1) / POL_HB;
  for (int jb = 0; jb < nb; ++jb) {
    const PCG_CONSTANT double* W = D + P.offW[0] + (size_t)jb * POL_HB * ld;
    const PCG_CONSTANT double* b = D + P.offb[0] + jb * POL_HB;
    double acc[POL_HB];
#pragma unroll
    for (int r = 0; r < POL_HB; ++r) acc[r] = b[r];
#pragma unroll
    for (int ib = 0; ib < NIN / POL_IB; ++ib) {
      if (ib * POL_IB < n_in) {
#pragma unroll
        for (int i = 0; i < POL_IB; ++i)
#pragma unroll
          for (int r = 0; r < POL_HB; ++r) acc[r] = __builtin_fma(W[r * ld + ib * POL_IB + i], in[ib * POL_IB + i], acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < POL_HB; ++r) acc[r] = pol_act(acc[r], act);
#pragma unroll
    for (int q = 0; q < POL_MAX_W / POL_HB; ++q) {
      if (jb == q) {  // (uniform: the register array is only ever indexed by constants)
#pragma unroll
        for (int r = 0; r < POL_HB; ++r) h[q * POL_HB + r] = acc[r];
      }
    }
  }
}

// R units of layer `L` from h[0 .. width): acc[r] = b[j0 + r] + sum_k W[j0 + r][k] h[k]
template <int R>
PCG_DEV void pol_rows_from_h(const PCG_CONSTANT PolicyDev& P, const PCG_CONSTANT double* D, int L, int j0, int width,
                             const double (&h)[POL_MAX_W], double (&acc)[R]) {
  const int ld = P.ld[L];
  const PCG_CONSTANT double* W = D + P.offW[L] + (size_t)j0 * ld;
  const PCG_CONSTANT double* b = D + P.offb[L] + j0;
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = b[r];
#pragma unroll
  for (int kb = 0; kb < POL_MAX_W / POL_HB; ++kb) {
    if (kb * POL_HB < width) {
#pragma unroll
      for (int k = 0; k < POL_HB; ++k)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = __builtin_fma(W[r * ld + kb * POL_HB + k], h[kb * POL_HB + k], acc[r]);
    }
  }
}

// out = the last layer's output BEFORE the output map (the mean of a Gaussian actor, a critic's value:
// pcg_rollout_actor.hpp).  NIN: a multiple of POL_IB that holds the plan's observation vector (entries past n_in are zero);
// NA: the kernel's output width (rows past n_out are zero: the output matrix is padded to PCG_MAX_NA rows).
template <int NIN, int NA>
PCG_DEV void policy_raw(const PCG_CONSTANT PolicyDev& P, const double (&in)[NIN], double (&out)[NA]) {
  static_assert(NIN % POL_IB == 0 && NA <= PCG_MAX_NA, "policy_raw: block sizes");
  const PCG_CONSTANT double* D = reinterpret_cast<const PCG_CONSTANT double*>(&P + 1);
  const int nh = P.n_hidden;
  if (nh == 0) {
    const int ld = P.ld[0], n_in = P.n_in;
    const PCG_CONSTANT double* W = D + P.offW[0];
    const PCG_CONSTANT double* b = D + P.offb[0];
#pragma unroll
    for (int o = 0; o < NA; ++o) out[o] = b[o];
#pragma unroll
    for (int ib = 0; ib < NIN / POL_IB; ++ib) {
      if (ib * POL_IB < n_in) {
#pragma unroll
        for (int i = 0; i < POL_IB; ++i)
#pragma unroll
          for (int o = 0; o < NA; ++o) out[o] = __builtin_fma(W[o * ld + ib * POL_IB + i], in[ib * POL_IB + i], out[o]);
      }
    }
  } else {
    double h[POL_MAX_W];
    pol_first<NIN>(P, D, in, h);
    if (nh == 1) {
      pol_rows_from_h<NA>(P, D, 1, 0, P.w[0], h, out);
    } else {
      // second hidden layer streamed into the output layer: POL_SB units at a time, consumed as soon as they are formed
      const int ld2 = P.ld[2], w0 = P.w[0], act = P.act;
      const PCG_CONSTANT double* W2 = D + P.offW[2];
      const PCG_CONSTANT double* b2 = D + P.offb[2];
#pragma unroll
      for (int o = 0; o < NA; ++o) out[o] = b2[o];
      const int nb = (P.w[1] + POL_SB - 1) / POL_SB;
      for (int jb = 0; jb < nb; ++jb) {
        double h2[POL_SB];
        pol_rows_from_h<POL_SB>(P, D, 1, jb * POL_SB, w0, h, h2);
#pragma unroll
        for (int r = 0; r < POL_SB; ++r) h2[r] = pol_act(h2[r], act);
#pragma unroll
        for (int r = 0; r < POL_SB; ++r)
#pragma unroll
          for (int o = 0; o < NA; ++o) out[o] = __builtin_fma(W2[o * ld2 + jb * POL_SB + r], h2[r], out[o]);
      }
    }
  }
}

// a = out_map(out): the policy's output map, component by component
template <int NA>
PCG_DEV void policy_map(const PCG_CONSTANT PolicyDev& P, const double (&out)[NA], double (&a)[NA]) {
  const int om = P.out_map;
  const double lo = P.out_lo, hi = P.out_hi;
#pragma unroll
  for (int o = 0; o < NA; ++o) {
    double v = out[o];
    if (om == PCG_POL_CLIP) v = v < lo ? lo : (v > hi ? hi : v);  // (a NaN stays a NaN, as under torch.clamp)
    else if (om == PCG_POL_TANH) v = tanh(v);
    a[o] = v;
  }
}

// a = policy(in) = out_map(raw output)
template <int NIN, int NA>
PCG_DEV void policy_eval(const PCG_CONSTANT PolicyDev& P, const double (&in)[NIN], double (&a)[NA]) {
  double out[NA];
  policy_raw<NIN, NA>(P, in, out);
  policy_map<NA>(P, out, a);
}

// the observation vector of one step in store_obs order [ox | osp | od], zero beyond it
template <class M, int NIN>
PCG_DEV void policy_input(CDevConst& c, const EnvOut<M>& out, double (&in)[NIN]) {
  const int nx = M::DYNAMIC ? c.nx : M::NX;
  const int nso = c.nsp_obs, nd = c.nd;
#pragma unroll
  for (int i = 0; i < NIN; ++i) {
    double v = 0.0;
    if (i < M::NX && i < nx) v = out.ox[i < M::NX ? i : 0];
#pragma unroll
    for (int k = 0; k < PCG_MAX_NSP; ++k)
      if (k < nso && i == nx + k) v = out.osp[k];
#pragma unroll
    for (int k = 0; k < (M::NDM > 0 ? M::NDM : 1); ++k)
      if (k < M::NDM && k < nd && i == nx + nso + k) v = out.od[k];
    in[i] = v;
  }
}

template <class M>
constexpr int policy_nin() {
  return (M::NX + PCG_MAX_NSP + M::NDM + POL_IB - 1) / POL_IB * POL_IB;
}

// Closed-loop fused rollout.  Plans without constraint rows, per-env parameters or user expressions, lock-stepped, RK4 / CV8
// (checked on the host: closed_loop_open, pcg_abi_policy.hip).  Reads io->obs (the observation before step t0), writes what
// pcg_rollout writes plus the recorded policy outputs.
// The loop is stated here and again in rollout_actor_kernel (pcg_rollout_actor.hpp), ON MEASUREMENT.  As one PCG_DEV
// function template that both __global__ functions call, with what happens between two steps as a template argument, it
// returns the same bits but compiles to other code, up to 21 % slower (the affine model's actor kernels; the cstr's 1-2 %);
// even a helper for the record loops alone cost the cstr's actor 2 %.  Moving a kernel's unchanged body into such a function
// is enough to change the code, which is consistent with the by-value kernel arguments being read through references in a
// callee that is optimised before it is inlined.  profiles/r9/closed_loop_refactor.txt, DESIGN.md section 3.6.
// Waves per SIMD asked of the register allocator for the models of up to ten states (the first hidden layer alone is 128
// registers; measured on the cstr, tools/policy_rollout_bench.py: profiles/r7/policy_rollout.txt)
#ifndef PCG_POL_WPE
#define PCG_POL_WPE 2
#endif
template <class M, int INTEG>
__global__ __launch_bounds__(BLOCK, M::NX <= 10 ? PCG_POL_WPE : 1) void rollout_policy_kernel(const StepArgs A, const PolicyArgs Q) {
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
  // (one loop body for the T applied actions and the recorded next one: the policy is inlined once)
  const int n_eval = A.T + ((Q.record_next && Q.a_out) ? 1 : 0);
  for (int s = 0; s < n_eval; ++s) {
    policy_eval<NIN, NA>(P, in, a);
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

}  // namespace pcg
