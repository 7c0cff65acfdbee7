// pcg_rollout_pop_cons.hpp -- closed-loop fused rollout of a POPULATION of MLP policies on plans WITH constraint rows
// (pcg_rollout_policy_pop_cons): the evaluation step of a CONSTRAINED derivative-free search -- every slice of
// `envs_per_policy` consecutive envs is driven by its own member (pcg_rollout_pop.hpp), every step's rows and violation flag
// are the per-step route's bits (pcg_rollout_cons.hpp), and beside each env's discounted return the kernel keeps what a
// search needs to penalise or reject a member, so that nobody records T x B flags and reduces them on the host.
//
// rollout_pop_policy_kernel's / rollout_pop_policy_kernel_f32's loop restated -- restated, not shared, for the reason
// pcg_rollout_policy.hpp gives and profiles/r9/closed_loop_refactor.txt measures -- with the constrained env step in place of
// env_step.  Per env, in registers:
//
//   J, disc  ret_out[e] = sum_s gamma^s rew_s:   J = J + disc * r;  disc = disc * gamma   from J = 0, disc = 1, every operation
//            rounded on its own (contraction off for the two statements), disc kept in scalar registers (pop_uniform).
//   nviol    (int32) the number of THIS call's steps whose post-step flag "any row > 0" was set -> nviol_out[e]
//   gmax     (double) the largest post-step row value over this call's steps and rows            -> gmax_out[e]
//            from -inf:   gmax = (g > gmax) ? g : gmax   -- that statement defines the bits, and a NaN row leaves it unchanged.
//
// The pre-step check at counter 0 writes io->g_pre and enters `done` as in pcg_rollout_cons.hpp; it counts in neither nviol
// nor gmax.  An env whose done flag is set mid-episode keeps stepping, as there.  Every output may be null; the rows are
// summed regardless (the flag feeds the penalty, the box excess and `done`).
//
// The step is pcg_rollout_cons.hpp's env_step_cons itself, which shows every post-step row, still in its register, to the
// hook it is given: RowsMax on gmax here, none in the single-policy kernels.  The pre-step check is shown to no hook.  The
// recorded rows, flags, rewards and observations are the per-step route's bits in both summation orders (ConsArgs::order_w,
// picked by the host as for pcg_rollout_policy_cons).
//
// member   m = (env_offset + e) / G, formed once per wave after the e >= B exit and made provably uniform by readfirstlane:
//          the member's block address is a scalar and the weights stay scalar loads (64 | G, 64 | env_offset: the host).
//
// Ahead-of-time only: never part of a plan's run-time compiled closed-loop source (pop_open refuses such plans).
// Out of scope: constraint expressions and user models, rows together with per-env parameters, stochastic actors over a
// population, the adaptive integrators, cutting J at the first violation (a caller masks from viol_seq or penalises through nviol).
#pragma once

namespace pcg {

// PopArgs and the two statistics (PopArgs' layout, then the two pointers)
struct PopConsArgs : PopArgs {
  int32_t* nviol_out;  // [B] steps of this call with a violated row, or null
  double* gmax_out;    // [B] largest row value of this call's steps, or null
};

template <class M, int INTEG>
__global__ __launch_bounds__(BLOCK, M::NX <= 10 ? PCG_POL_WPE : 1) void rollout_pop_cons_policy_kernel(const StepArgs A, const PopConsArgs Q,
                                                                                                      const ConsArgs G) {
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
  double J = 0.0, disc = 1.0, gmax = -__builtin_inf();
  int32_t nviol = 0;
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
    env_step_cons<M, INTEG, RowsMax>(A, c, G, e, A.t_scalar + s, a, x, G.g_seq ? G.g_seq + (size_t)s * G.g_ss + e : nullptr,
                                     (last && G.g_last) ? G.g_last + e : nullptr, out, gmax);
    {
#pragma clang fp contract(off)
      const double dr = disc * out.rew;
      J = J + dr;
      disc = disc * Q.gamma;
    }
    disc = pop_uniform(disc);
    nviol += out.viol ? 1 : 0;
    if (G.viol_seq) G.viol_seq[(size_t)s * G.v_ss + e] = out.viol ? 1 : 0;
    if (A.rew_seq) A.rew_seq[(size_t)s * A.r_ss + e] = out.rew;
    if (A.obs_seq) store_obs<M>(A, c, out, A.obs_seq + (size_t)s * A.o_ss + e, A.o_cs);
    if (last) store_out<M>(A, c, e, out, A.obs + e);  // io->obs/rew/done/viol hold the last step
    else if (A.status && out.status != PCG_ST_OK) A.status[e] = out.status;
    policy_input<M, NIN>(c, out, in);
  }
  if (Q.ret_out) Q.ret_out[e] = J;
  if (Q.nviol_out) Q.nviol_out[e] = nviol;
  if (Q.gmax_out) Q.gmax_out[e] = gmax;
#pragma unroll
  for (int i = 0; i < NX; ++i)
    if (i < nx) A.x[(size_t)i * B + e] = x[i];
}

// The same loop with the member's network evaluated in float32 (policy_raw_f32 + policy_map_f32, pcg_rollout_policy_f32.hpp)
// on a block of pack_policy's float32 form: the network in float32, the env, the rows, J, disc and gmax in fp64.  It is the
// first float32 network on a plan with constraint rows.  Waves per SIMD: rollout_pop_policy_kernel_f32's.
template <class M, int INTEG>
__global__ __launch_bounds__(BLOCK, M::NX <= 10 ? PCG_POP32_WPE : 1) void rollout_pop_cons_policy_kernel_f32(const StepArgs A,
                                                                                                           const PopConsArgs Q,
                                                                                                           const ConsArgs G) {
  CDevConst& c = *A.C;
  constexpr int NX = M::NX, NA = M::NA, NIN = policy_nin<M>();
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= A.B) return;
  // (the same value in every lane of the wave, as in rollout_pop_cons_policy_kernel)
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
  double J = 0.0, disc = 1.0, gmax = -__builtin_inf();
  int32_t nviol = 0;
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
    env_step_cons<M, INTEG, RowsMax>(A, c, G, e, A.t_scalar + s, a, x, G.g_seq ? G.g_seq + (size_t)s * G.g_ss + e : nullptr,
                                     (last && G.g_last) ? G.g_last + e : nullptr, out, gmax);
    {
#pragma clang fp contract(off)
      const double dr = disc * out.rew;
      J = J + dr;
      disc = disc * Q.gamma;
    }
    disc = pop_uniform(disc);
    nviol += out.viol ? 1 : 0;
    if (G.viol_seq) G.viol_seq[(size_t)s * G.v_ss + e] = out.viol ? 1 : 0;
    if (A.rew_seq) A.rew_seq[(size_t)s * A.r_ss + e] = out.rew;
    if (A.obs_seq) store_obs<M>(A, c, out, A.obs_seq + (size_t)s * A.o_ss + e, A.o_cs);
    if (last) store_out<M>(A, c, e, out, A.obs + e);  // io->obs/rew/done/viol hold the last step
    else if (A.status && out.status != PCG_ST_OK) A.status[e] = out.status;
    policy_input<M, NIN>(c, out, in);
  }
  if (Q.ret_out) Q.ret_out[e] = J;
  if (Q.nviol_out) Q.nviol_out[e] = nviol;
  if (Q.gmax_out) Q.gmax_out[e] = gmax;
#pragma unroll
  for (int i = 0; i < NX; ++i)
    if (i < nx) A.x[(size_t)i * B + e] = x[i];
}

}  // namespace pcg
