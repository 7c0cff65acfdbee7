// pcg_rollout_unc.hpp -- the closed-loop fused rollouts on plans WITH per-env model parameters (pcg_rollout_policy_unc,
// pcg_rollout_actor_unc): parametric uncertainty sampled at reset (uncertainty_percentages on model parameters, pcgym.py:300-316),
// the reference's domain randomisation.  rollout_policy_kernel's and rollout_actor_kernel's loops (one env per lane, state
// and observation in registers, the networks between two steps, the same Philox keys), with two differences:
//   parameters   the step is env_step<M, PCG_INT_RK4, false, false, true, UNC = true>, as in step_kernel<..., UNC>: every step
//                the lane rebuilds its OWN folded model constants (c.raw with the env's p_unc values substituted, through
//                M::prep) and integrates with them; an unconfigured disturbance input takes the env's own parameter (quirk
//                Q11).  Rebuilding them once per lane in front of the loop, into a register-resident M::KP, was built and
//                measured as well: 3 % faster for affine networks on the cstr, 1-8 % slower with hidden layers, where the
//                constants stay live across the first hidden layer's 128 registers.  It is not kept
//                (profiles/r15/unc_rollout.txt).
//   observation  nunc more slots, [ox | osp | od | ounc]: the networks read them (policy_input_unc, policy_nin_unc), the
//                recorded rows and the final io->obs carry them (store_obs / store_out<M, true>).
// env_step keeps its text, and no kernel that existed before this header changes.  M::prep, the right-hand side and env_post
// are compiled here under the compiler's default contraction, as in every kernel, so this kernel and step_kernel<..., true>
// may differ in the last bits of a step (as rollout_kernel<..., true> and step_kernel<..., true> do).
// The loops are restated and not shared with the other closed-loop kernels for the reason pcg_rollout_policy.hpp gives.
// Launch bounds: those of the twins without per-env parameters (PCG_POL_WPE / PCG_ACT_WPE).  At ONE wave per SIMD the cstr's
// kernels use no scratch and are 1.1-1.5 x slower (profiles/r15/unc_rollout.txt).
//
// Out of scope: float32 networks, plans with per-env parameters AND constraint rows, CV8 (refused with per-env parameters
// at plan creation) and the adaptive integrators, plans with run-time compiled code (which refuse per-env parameters at
// creation beside), and per-env counters.
#pragma once

namespace pcg {

// the network input of a plan with per-env parameters: policy_nin<M>() plus the parameter slots
template <class M>
constexpr int policy_nin_unc() {
  return (M::NX + PCG_MAX_NSP + M::NDM + PCG_MAX_NUNC + POL_IB - 1) / POL_IB * POL_IB;
}

// the observation vector of one step in store_obs<M, true> order [ox | osp | od | ounc], zero beyond it
template <class M, int NIN>
PCG_DEV void policy_input_unc(CDevConst& c, const EnvOut<M>& out, double (&in)[NIN]) {
  const int nx = M::NX;
  const int nso = c.nsp_obs, nd = c.nd, nunc = c.nunc;
#pragma unroll
  for (int i = 0; i < NIN; ++i) {
    double v = 0.0;
    if (i < M::NX) v = out.ox[i < M::NX ? i : 0];
#pragma unroll
    for (int k = 0; k < PCG_MAX_NSP; ++k)
      if (k < nso && i == nx + k) v = out.osp[k];
#pragma unroll
    for (int k = 0; k < (M::NDM > 0 ? M::NDM : 1); ++k)
      if (k < M::NDM && k < nd && i == nx + nso + k) v = out.od[k];
    // (compile-time indices into ounc[], as where env_post fills it: a run-time trip count would put it into scratch)
#pragma unroll
    for (int j = 0; j < PCG_MAX_NUNC; ++j)
      if (j < nunc && i == nx + nso + nd + j) v = out.ounc[j];
    in[i] = v;
  }
}

// rollout_policy_kernel's loop (pcg_rollout_policy.hpp) on a plan with per-env parameters; built-in models, RK4
template <class M>
__global__ __launch_bounds__(BLOCK, M::NX <= 10 ? PCG_POL_WPE : 1) void rollout_unc_policy_kernel(const StepArgs A, const PolicyArgs Q) {
  static_assert(!M::DYNAMIC, "per-env parameters: built-in models only");
  CDevConst& c = *A.C;
  const PCG_CONSTANT PolicyDev& P = *Q.P;
  constexpr int NX = M::NX, NA = M::NA, NIN = policy_nin_unc<M>();
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= A.B) return;
  const int64_t B = A.B;
  const int nobs = c.nobs;
  double x[NX], a[NA], in[NIN];
#pragma unroll
  for (int i = 0; i < NX; ++i) x[i] = A.x[(size_t)i * B + e];
#pragma unroll
  for (int i = 0; i < NIN; ++i) in[i] = (i < nobs) ? A.obs[(size_t)i * B + e] : 0.0;
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
    if (A.rew_seq) A.rew_seq[(size_t)s * A.r_ss + e] = out.rew;
    if (A.obs_seq) store_obs<M, true>(A, c, out, A.obs_seq + (size_t)s * A.o_ss + e, A.o_cs);
    if (last) store_out<M, true>(A, c, e, out, A.obs + e);  // io->obs/rew/done hold the last step
    else if (A.status && out.status != PCG_ST_OK) A.status[e] = out.status;
    policy_input_unc<M, NIN>(c, out, in);
  }
#pragma unroll
  for (int i = 0; i < NX; ++i) A.x[(size_t)i * B + e] = x[i];
}

// rollout_actor_kernel's loop (pcg_rollout_actor.hpp) on a plan with per-env parameters; built-in models, RK4
template <class M>
__global__ __launch_bounds__(BLOCK, M::NX <= 10 ? PCG_ACT_WPE : 1) void rollout_unc_actor_kernel(const StepArgs A, const ActorArgs Q) {
  static_assert(!M::DYNAMIC, "per-env parameters: built-in models only");
  CDevConst& c = *A.C;
  const PCG_CONSTANT PolicyDev& P = *Q.P;
  constexpr int NX = M::NX, NA = M::NA, NIN = policy_nin_unc<M>();
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= A.B) return;
  const int64_t B = A.B;
  const int nobs = c.nobs;
  const uint64_t env_id = (uint64_t)(A.env_offset + e);
  double x[NX], a[NA], in[NIN];
#pragma unroll
  for (int i = 0; i < NX; ++i) x[i] = A.x[(size_t)i * B + e];
#pragma unroll
  for (int i = 0; i < NIN; ++i) in[i] = (i < nobs) ? A.obs[(size_t)i * B + e] : 0.0;
  const bool any_out = Q.a_out || Q.u_out || Q.lp_out || Q.v_out;
  const int n_eval = A.T + ((Q.record_next && any_out) ? 1 : 0);
  for (int s = 0; s < n_eval; ++s) {
    double u[NA], z[NA + (NA & 1)];
    policy_raw<NIN, NA>(P, in, u);  // mu
#pragma unroll
    for (int i = 0; i < NA; i += 2) rng_normal2(A.seed, env_id, (uint32_t)(A.t_scalar + s), RNG_POLICY + (uint32_t)(i >> 1), z[i], z[i + 1]);
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      u[i] = __builtin_fma(Q.sigma[i], z[i], u[i]);
      q = __builtin_fma(z[i], z[i], q);
    }
    policy_map<NA>(P, u, a);
    if (Q.a_out) {
      double* ao = Q.a_out + (size_t)s * Q.ao_ss + e;
#pragma unroll
      for (int i = 0; i < NA; ++i) ao[(size_t)i * Q.ao_cs] = a[i];
    }
    if (Q.u_out) {
      double* uo = Q.u_out + (size_t)s * Q.uo_ss + e;
#pragma unroll
      for (int i = 0; i < NA; ++i) uo[(size_t)i * Q.uo_cs] = u[i];
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
    env_step<M, PCG_INT_RK4, false, false, true, true>(A, c, nullptr, nullptr, e, A.t_scalar + s, a, x, out);
    if (A.rew_seq) A.rew_seq[(size_t)s * A.r_ss + e] = out.rew;
    if (A.obs_seq) store_obs<M, true>(A, c, out, A.obs_seq + (size_t)s * A.o_ss + e, A.o_cs);
    if (last) store_out<M, true>(A, c, e, out, A.obs + e);  // io->obs/rew/done hold the last step
    else if (A.status && out.status != PCG_ST_OK) A.status[e] = out.status;
    policy_input_unc<M, NIN>(c, out, in);
  }
#pragma unroll
  for (int i = 0; i < NX; ++i) A.x[(size_t)i * B + e] = x[i];
}

}  // namespace pcg
