// pcg_rollout_actor.hpp -- closed-loop fused rollout with a STOCHASTIC actor-critic (pcg_rollout_actor): the data an
// on-policy trainer (PPO) collects, in one launch.  stable-baselines3's MlpPolicy is a Gaussian actor with a
// state-independent log_std plus a separate value network; per step the trainer needs the sampled action, its
// log-probability and the value estimate, and a bootstrap value for the observation after the last step.
//
// rollout_policy_kernel's loop (pcg_rollout_policy.hpp, which also says why it is stated twice), one env per lane, with this
// between two steps:
//   mu    = actor's last-layer output before its output map                       (policy_raw)
//   z_i   = rng_normal2(seed, env_offset + e, t, RNG_POLICY + (i >> 1))           (t = t0 + s, the step's shared counter)
//   u_i   = fma(sigma_i, z_i, mu_i)                                               the sample the trainer's buffer keeps
//   a     = out_map(u)                                                            what the env applies (none / clip)
//   logp  = fma(-0.5, q, c0),  q = 0; for i ascending: q = fma(z_i, z_i, q)       log N(u; mu, sigma^2), the unmapped sample
//   value = critic's output on the same observation                               (policy_raw<NIN, 1>, when a critic is given)
// sigma[na] and c0 = -(sum log sigma_i + na/2 log 2 pi) are formed by the host in fp64 and travel BY VALUE in the kernel
// arguments: they change with every training iteration, and so cost neither a device allocation nor a copy; no division,
// no log and no exp on the device.  (u_i - mu_i) / sigma_i is z_i by construction, which is why logp is stated in z.
// The critic's presence is a wave-uniform run-time branch (the family is not doubled); the two networks are evaluated one
// after the other, so the first-hidden-layer array of the one is dead when the other's is formed: the same registers.
// Plain vector stores, no LDS, no mutable plan or policy state: capture-safe.
#pragma once

namespace pcg {

constexpr uint32_t RNG_POLICY = 0x400u;  // purpose of the policy's exploration noise, beside RNG_NOISE / RNG_DIST / RNG_RESET
constexpr uint32_t RNG_SEARCH = 0x500u;  // purpose of the search noise over a population's weights (pcg_pop_search.hpp)

struct ActorArgs {
  const PCG_CONSTANT PolicyDev* P;   // actor
  const PCG_CONSTANT PolicyDev* V;   // critic (n_out == 1, no output map), or null
  double* a_out;                     // [T (+1)][na][B] applied actions out_map(u), or null
  double* u_out;                     // [T (+1)][na][B] samples u, or null
  double* lp_out;                    // [T (+1)][B] log-probabilities of u, or null
  double* v_out;                     // [T (+1)][B] critic values, or null
  int64_t ao_ss, ao_cs, uo_ss, uo_cs, lp_ss, v_ss;  // element strides (step, component)
  double sigma[PCG_MAX_NA];          // standard deviations (entries past na: 0)
  double c0;                         // -(sum_i log sigma_i + na/2 log 2 pi)
  int32_t record_next;               // row T = the four quantities for the observation after the last step, not applied
};

#ifndef PCG_ACT_WPE
#define PCG_ACT_WPE 2  // waves per SIMD asked for the models of up to ten states, as for rollout_policy_kernel
#endif
template <class M, int INTEG>
__global__ __launch_bounds__(BLOCK, M::NX <= 10 ? PCG_ACT_WPE : 1) void rollout_actor_kernel(const StepArgs A, const ActorArgs Q) {
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
    policy_raw<NIN, NA>(P, in, u);  // mu
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
    policy_map<NA>(P, u, a);
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
      double v[1];
      policy_raw<NIN, 1>(*Q.V, in, v);
      Q.v_out[(size_t)s * Q.v_ss + e] = v[0];
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
