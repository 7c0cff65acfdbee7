// pcg_rollout_pop.hpp -- closed-loop fused rollout of a POPULATION of MLP policies (pcg_rollout_policy_pop): one launch in
// which every slice of `envs_per_policy` consecutive envs (global env indices) is driven by its own member of a
// pcg_policy_pop -- what derivative-free policy search (evolution strategies, CEM, PSO over the weights), the comparison of a
// set of checkpoints under the same disturbances and noise (the reference's policy_eval with its `policies` dict) and
// hyper-parameter sweeps ask for.  Without it a caller with P policies makes P launches of a few workgroups each, or steps
// with a batched matmul in torch.
//
// A population is P device blocks of ONE shape at a fixed byte stride, each exactly what pack_policy (pcg_policy_pack.hpp) writes for
// a pcg_policy: policy_eval (pcg_rollout_policy.hpp) reads a member unchanged.  The kernel is rollout_policy_kernel's loop
// restated -- restated, not shared, for the reason measured in profiles/r9/closed_loop_refactor.txt and given above that
// kernel -- with two differences:
//
//   member   env e is driven by member m = (env_offset + e) / G.  G and env_offset are multiples of 64 (checked on the host),
//            so a wave never spans two members; m is formed once per wave, after the e >= B exit, and made PROVABLY uniform
//            by readfirstlane, so that the member's block address is a scalar and the weights stay scalar loads through the
//            constant address space.  B need not be a multiple of G.
//   returns  ret_out[e] = sum_s gamma^s rew_s of this call's steps, kept in a register so that a search loop neither stores
//            nor re-reads T x B rewards:   J = J + disc * r;  disc = disc * gamma   from J = 0, disc = 1, every operation
//            rounded on its own (contraction off for the two statements, as in pcg_gae.hpp).  That defines the bits.
//
// A float32 population (pcg_policy_pop_create_f32) is P blocks of pack_policy's float32 form, and rollout_pop_policy_kernel_f32
// below is the same loop with pcg_rollout_policy_f32.hpp's evaluator: the network in float32, the env, J and disc in fp64.
//
// Out of scope: stochastic actors over a population and plans with run-time compiled code (whose module does not carry these
// kernels: ahead-of-time only).  Plans with per-env parameters: pcg_rollout_pop_unc.hpp; plans with constraint rows:
// pcg_rollout_pop_cons.hpp.  These two kernels take neither.
#pragma once

namespace pcg {

struct PopArgs {
  const PCG_CONSTANT char* blocks;  // P member blocks (PolicyDev header + packed weights each)
  int64_t stride;                   // bytes from one member's block to the next (a multiple of 8)
  int64_t G;                        // envs per policy (a multiple of 64)
  double* a_out;                    // [T (+1)][na][B] recorded policy outputs, or null
  int64_t ao_ss, ao_cs;             // element strides (step, component)
  int32_t record_next;              // row T = policy(observation after the last step), not applied
  double gamma;
  double* ret_out;                  // [B] discounted return of this call's steps, or null
};

// a double that has the same value in every lane, moved to scalar registers (two readfirstlanes): the discount factor is
// wave-uniform, and as a vector value it would be two more registers alive across the policy and the env step
PCG_DEV double pop_uniform(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32));
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

template <class M, int INTEG>
__global__ __launch_bounds__(BLOCK, M::NX <= 10 ? PCG_POL_WPE : 1) void rollout_pop_policy_kernel(const StepArgs A, const PopArgs Q) {
  CDevConst& c = *A.C;
  constexpr int NX = M::NX, NA = M::NA, NIN = policy_nin<M>();
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= A.B) return;
  // (the same value in every lane of the wave: 64 | G, 64 | env_offset, 64 | BLOCK; m < P <= 2^31 - 1, checked on the host)
  const int m = __builtin_amdgcn_readfirstlane((int)((A.env_offset + e) / Q.G));
  const PCG_CONSTANT PolicyDev& P = *reinterpret_cast<const PCG_CONSTANT PolicyDev*>(Q.blocks + (int64_t)m * Q.stride);
  const int64_t B = A.B;
  const int nx = M::DYNAMIC ? c.nx : NX;
  const int na = M::DYNAMIC ? c.na : NA;
  const int nobs = c.nobs;
  double x[NX], a[NA], in[NIN];
#pragma unroll
  for (int i = 0; i < NX; ++i) x[i] = (i < nx) ? A.x[(size_t)i * B + e] : 0.0;
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
      for (int i = 0; i < NA; ++i)
        if (i < na) ao[(size_t)i * Q.ao_cs] = a[i];
    }
    if (s == A.T) break;  // row T: policy(observation after the last step), recorded and not applied
    const bool last = (s == A.T - 1);
    EnvOut<M> out;
    env_step<M, INTEG, false, false, true>(A, c, nullptr, nullptr, e, A.t_scalar + s, a, x, out);
    {
#pragma clang fp contract(off)
      const double dr = disc * out.rew;
      J = J + dr;
      disc = disc * Q.gamma;
    }
    disc = pop_uniform(disc);
    if (A.rew_seq) A.rew_seq[(size_t)s * A.r_ss + e] = out.rew;
    if (A.obs_seq) store_obs<M>(A, c, out, A.obs_seq + (size_t)s * A.o_ss + e, A.o_cs);
    if (last) store_out<M>(A, c, e, out, A.obs + e);  // io->obs/rew/done hold the last step
    else if (A.status && out.status != PCG_ST_OK) A.status[e] = out.status;
    policy_input<M, NIN>(c, out, in);
  }
  if (Q.ret_out) Q.ret_out[e] = J;
#pragma unroll
  for (int i = 0; i < NX; ++i)
    if (i < nx) A.x[(size_t)i * B + e] = x[i];
}

// The same loop with the member's network evaluated in float32: policy_raw_f32 + policy_map_f32 (pcg_rollout_policy_f32.hpp)
// in place of policy_eval, on a block of pack_policy's float32 form.  A float32 block is half the bytes a wave streams per step.
// Waves per SIMD asked for the models of up to ten states: rollout_policy_kernel_f32's two, for the reason given above that
// kernel -- the bitwise replay of the recorded actions through the open-loop general kernel is the bar
// (tests/test_gpu_pop_f32.py), and a register budget is changed HERE when an instantiation misses it.
#ifndef PCG_POP32_WPE
#define PCG_POP32_WPE PCG_POL32_WPE
#endif
template <class M, int INTEG>
__global__ __launch_bounds__(BLOCK, M::NX <= 10 ? PCG_POP32_WPE : 1) void rollout_pop_policy_kernel_f32(const StepArgs A, const PopArgs Q) {
  CDevConst& c = *A.C;
  constexpr int NX = M::NX, NA = M::NA, NIN = policy_nin<M>();
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= A.B) return;
  // (the same value in every lane of the wave, as in rollout_pop_policy_kernel)
  const int m = __builtin_amdgcn_readfirstlane((int)((A.env_offset + e) / Q.G));
  const PCG_CONSTANT PolicyDev& P = *reinterpret_cast<const PCG_CONSTANT PolicyDev*>(Q.blocks + (int64_t)m * Q.stride);
  const int64_t B = A.B;
  const int nx = M::DYNAMIC ? c.nx : NX;
  const int na = M::DYNAMIC ? c.na : NA;
  const int nobs = c.nobs;
  double x[NX], a[NA], in[NIN];
#pragma unroll
  for (int i = 0; i < NX; ++i) x[i] = (i < nx) ? A.x[(size_t)i * B + e] : 0.0;
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
      for (int i = 0; i < NA; ++i)
        if (i < na) ao[(size_t)i * Q.ao_cs] = a[i];
    }
    if (s == A.T) break;  // row T: policy(observation after the last step), recorded and not applied
    const bool last = (s == A.T - 1);
    EnvOut<M> out;
    env_step<M, INTEG, false, false, true>(A, c, nullptr, nullptr, e, A.t_scalar + s, a, x, out);
    {
#pragma clang fp contract(off)
      const double dr = disc * out.rew;
      J = J + dr;
      disc = disc * Q.gamma;
    }
    disc = pop_uniform(disc);
    if (A.rew_seq) A.rew_seq[(size_t)s * A.r_ss + e] = out.rew;
    if (A.obs_seq) store_obs<M>(A, c, out, A.obs_seq + (size_t)s * A.o_ss + e, A.o_cs);
    if (last) store_out<M>(A, c, e, out, A.obs + e);  // io->obs/rew/done hold the last step
    else if (A.status && out.status != PCG_ST_OK) A.status[e] = out.status;
    policy_input<M, NIN>(c, out, in);
  }
  if (Q.ret_out) Q.ret_out[e] = J;
#pragma unroll
  for (int i = 0; i < NX; ++i)
    if (i < nx) A.x[(size_t)i * B + e] = x[i];
}

}  // namespace pcg
