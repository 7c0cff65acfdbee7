// pcg_rollout_pop_unc.hpp -- closed-loop fused rollout of a POPULATION of MLP policies on plans WITH per-env model parameters
// (pcg_rollout_policy_pop_unc): the search for a controller that holds up over a distribution of plants -- every slice of
// `envs_per_policy` consecutive envs is driven by its own member (pcg_rollout_pop.hpp), and every env of a slice integrates
// with its OWN model parameters, sampled at reset (pcg_rollout_unc.hpp).
//
// rollout_unc_policy_kernel's loop restated -- restated, not shared, for the reason pcg_rollout_policy.hpp gives and
// profiles/r9/closed_loop_refactor.txt measures -- with rollout_pop_policy_kernel's two differences:
//
//   member   m = (env_offset + e) / G, formed once per wave after the e >= B exit and made provably uniform by readfirstlane:
//            the member's block address is a scalar and the weights stay scalar loads (64 | G, 64 | env_offset: the host).
//   returns  ret_out[e] = sum_s gamma^s rew_s:   J = J + disc * r;  disc = disc * gamma   from J = 0, disc = 1, every operation
//            rounded on its own (contraction off for the two statements), disc kept in scalar registers (pop_uniform).
//
// The step is env_step<M, PCG_INT_RK4, false, false, true, UNC = true>; the network reads [ox | osp | od | ounc]
// (policy_input_unc, policy_nin_unc), the recorded rows and the final io->obs carry the parameter slots
// (store_obs / store_out<M, true>).  env_step, policy_eval, policy_input_unc and every kernel that existed before this header
// keep their text.  The step is compiled here on its own, under the compiler's default contraction: an env computes what
// rollout_unc_policy_kernel computes with that member to rounding, not to the bit.
//
// rollout_pop_unc_policy_kernel_f32 is the same loop on a float32 population's blocks (policy_raw_f32 + policy_map_f32): the
// network in float32, the env, J and disc in fp64.  It is the first float32 network on a plan with per-env parameters:
// NIN = policy_nin_unc<M>() is wider than any other float32 kernel's input.
//
// Ahead-of-time only: never part of a plan's run-time compiled closed-loop source (such plans refuse per-env parameters).
// Out of scope: constraint rows, stochastic actors over a population, CV8 and the adaptive integrators.
#pragma once

namespace pcg {

// Waves per SIMD asked for the models of up to ten states: ONE, not the PCG_POL_WPE = 2 of rollout_unc_policy_kernel.  At two
// (256 registers) every instantiation spills -- the cstr's 476 bytes per lane, the member's scalar block address and the
// return's two registers on top of what rollout_unc_policy_kernel already spills (452) -- and at one (512) none does
// (tools/kernel_inventory.py --scratch; profiles/r24/population_unc.txt).
#ifndef PCG_POPUNC_WPE
#define PCG_POPUNC_WPE 1
#endif
template <class M>
__global__ __launch_bounds__(BLOCK, M::NX <= 10 ? PCG_POPUNC_WPE : 1) void rollout_pop_unc_policy_kernel(const StepArgs A, const PopArgs Q) {
  static_assert(!M::DYNAMIC, "per-env parameters: built-in models only");
  CDevConst& c = *A.C;
  constexpr int NX = M::NX, NA = M::NA, NIN = policy_nin_unc<M>();
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= A.B) return;
  // (the same value in every lane of the wave: 64 | G, 64 | env_offset, 64 | BLOCK; m < P <= 2^31 - 1, checked on the host)
  const int m = __builtin_amdgcn_readfirstlane((int)((A.env_offset + e) / Q.G));
  const PCG_CONSTANT PolicyDev& P = *reinterpret_cast<const PCG_CONSTANT PolicyDev*>(Q.blocks + (int64_t)m * Q.stride);
  const int64_t B = A.B;
  const int nobs = c.nobs;
  double x[NX], a[NA], in[NIN];
#pragma unroll
  for (int i = 0; i < NX; ++i) x[i] = A.x[(size_t)i * B + e];
#pragma unroll
  for (int i = 0; i < NIN; ++i) in[i] = (i < nobs) ? A.obs[(size_t)i * B + e] : 0.0;
  double J = 0.0, disc = 1.0;
  // (one loop body for the T applied actions and the recorded next one: the policy is inlined once)
  const int n_eval = A.T + ((Q.record_next && Q.a_out) ? 1 : 0);
  for (int s = 0; s < n_eval; ++s) {
    policy_eval<NIN, NA>(P, in, a);
    if (Q.a_out) {
      double* ao = Q.a_out + (size_t)s * Q.ao_ss + e;
#pragma unroll
      for (int i = 0; i < NA; ++i) ao[(size_t)i * Q.ao_cs] = a[i];
    }
    if (s == A.T) break;  // row T: policy(observation after the last step), recorded and not applied
    const bool last = (s == A.T - 1);
    EnvOut<M> out;
    env_step<M, PCG_INT_RK4, false, false, true, true>(A, c, nullptr, nullptr, e, A.t_scalar + s, a, x, out);
    {
#pragma clang fp contract(off)
      const double dr = disc * out.rew;
      J = J + dr;
      disc = disc * Q.gamma;
    }
    disc = pop_uniform(disc);
    if (A.rew_seq) A.rew_seq[(size_t)s * A.r_ss + e] = out.rew;
    if (A.obs_seq) store_obs<M, true>(A, c, out, A.obs_seq + (size_t)s * A.o_ss + e, A.o_cs);
    if (last) store_out<M, true>(A, c, e, out, A.obs + e);  // io->obs/rew/done hold the last step
    else if (A.status && out.status != PCG_ST_OK) A.status[e] = out.status;
    policy_input_unc<M, NIN>(c, out, in);
  }
  if (Q.ret_out) Q.ret_out[e] = J;
#pragma unroll
  for (int i = 0; i < NX; ++i) A.x[(size_t)i * B + e] = x[i];
}

// The same loop with the member's network evaluated in float32.  Waves per SIMD asked for the models of up to ten states, a
// macro of this kernel's own as in pcg_rollout_pop.hpp: ONE, not PCG_POP32_WPE's two -- with the wider input every
// instantiation spills at two (the cstr's 132 bytes per lane, up to 460) and none does at one.  A register budget is changed
// HERE when an instantiation would otherwise spill.
#ifndef PCG_POPUNC32_WPE
#define PCG_POPUNC32_WPE 1
#endif
template <class M>
__global__ __launch_bounds__(BLOCK, M::NX <= 10 ? PCG_POPUNC32_WPE : 1) void rollout_pop_unc_policy_kernel_f32(const StepArgs A, const PopArgs Q) {
  static_assert(!M::DYNAMIC, "per-env parameters: built-in models only");
  CDevConst& c = *A.C;
  constexpr int NX = M::NX, NA = M::NA, NIN = policy_nin_unc<M>();
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= A.B) return;
  // (the same value in every lane of the wave, as in rollout_pop_unc_policy_kernel)
  const int m = __builtin_amdgcn_readfirstlane((int)((A.env_offset + e) / Q.G));
  const PCG_CONSTANT PolicyDev& P = *reinterpret_cast<const PCG_CONSTANT PolicyDev*>(Q.blocks + (int64_t)m * Q.stride);
  const int64_t B = A.B;
  const int nobs = c.nobs;
  double x[NX], a[NA], in[NIN];
#pragma unroll
  for (int i = 0; i < NX; ++i) x[i] = A.x[(size_t)i * B + e];
#pragma unroll
  for (int i = 0; i < NIN; ++i) in[i] = (i < nobs) ? A.obs[(size_t)i * B + e] : 0.0;
  double J = 0.0, disc = 1.0;
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
      for (int i = 0; i < NA; ++i) ao[(size_t)i * Q.ao_cs] = a[i];
    }
    if (s == A.T) break;  // row T: policy(observation after the last step), recorded and not applied
    const bool last = (s == A.T - 1);
    EnvOut<M> out;
    env_step<M, PCG_INT_RK4, false, false, true, true>(A, c, nullptr, nullptr, e, A.t_scalar + s, a, x, out);
    {
#pragma clang fp contract(off)
      const double dr = disc * out.rew;
      J = J + dr;
      disc = disc * Q.gamma;
    }
    disc = pop_uniform(disc);
    if (A.rew_seq) A.rew_seq[(size_t)s * A.r_ss + e] = out.rew;
    if (A.obs_seq) store_obs<M, true>(A, c, out, A.obs_seq + (size_t)s * A.o_ss + e, A.o_cs);
    if (last) store_out<M, true>(A, c, e, out, A.obs + e);  // io->obs/rew/done hold the last step
    else if (A.status && out.status != PCG_ST_OK) A.status[e] = out.status;
    policy_input_unc<M, NIN>(c, out, in);
  }
  if (Q.ret_out) Q.ret_out[e] = J;
#pragma unroll
  for (int i = 0; i < NX; ++i) A.x[(size_t)i * B + e] = x[i];
}

}  // namespace pcg
