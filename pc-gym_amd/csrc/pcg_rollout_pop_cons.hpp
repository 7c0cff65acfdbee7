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
// The step: env_step_cons hands its rows to memory alone, and gmax needs them in a register.  So env_step_cons_max /
// env_post_cons_max / cons_rows_max below restate env_step_cons / env_post_cons / cons_rows statement by statement, with the
// one `gmax` update after a row is summed -- pcg_rollout_cons.hpp keeps its text, as every kernel that existed before this
// header does.  The pre-step check is cons_rows itself.  The recorded rows, flags, rewards and observations are the per-step
// route's bits in both summation orders (ConsArgs::order_w, picked by the host as for pcg_rollout_policy_cons).
//
// member   m = (env_offset + e) / G, formed once per wave after the e >= B exit and made provably uniform by readfirstlane:
//          the member's block address is a scalar and the weights stay scalar loads (64 | G, 64 | env_offset: the host).
//
// Ahead-of-time only: never part of a plan's run-time compiled closed-loop source (pop_open refuses such plans).
// Out of scope: constraint expressions and user models, rows together with per-env parameters, stochastic actors over a
// population, the adaptive integrators, cutting J at the first violation (a caller masks from viol_seq or penalises through nviol).
#pragma once

namespace pcg {

// PopArgs' fields and the two statistics.  A struct of its own: the existing kernels take PopArgs and ConsArgs by value, and
// their layout does not move.
struct PopConsArgs {
  const PCG_CONSTANT char* blocks;  // P member blocks (PolicyDev header + packed weights each)
  int64_t stride;                   // bytes from one member's block to the next (a multiple of 8)
  int64_t G;                        // envs per policy (a multiple of 64)
  double* a_out;                    // [T (+1)][na][B] recorded policy outputs, or null
  int64_t ao_ss, ao_cs;             // element strides (step, component)
  int32_t record_next;              // row T = policy(observation after the last step), not applied
  double gamma;
  double* ret_out;                  // [B] discounted return of this call's steps, or null
  int32_t* nviol_out;               // [B] steps of this call with a violated row, or null
  double* gmax_out;                 // [B] largest row value of this call's steps, or null
};

// cons_rows (pcg_rollout_cons.hpp) with the running maximum of the rows
template <class M>
PCG_DEV bool cons_rows_max(CDevConst& c, bool order_w, const double (&x)[M::NX], const double (&spv)[PCG_MAX_NSP],
                           const double (&dv)[PCG_MAX_NDM], const double (&u)[M::NA + M::NDM], double* g0, int64_t s0, double* g1,
                           int64_t s1, double& gmax) {
  bool violated = false;
  for (int r = 0; r < c.ncon; ++r) {
    const PCG_CONSTANT double* row = c.con_A[r];
    double g = -c.con_b[r];
    if (order_w) {  // (uniform) constraint_rows_w: the wave-uniform part of the row first
#pragma unroll
      for (int k = 0; k < PCG_MAX_NSP; ++k) g = g + row[PCG_MAX_NX + k] * spv[k];
#pragma unroll
      for (int k = 0; k < M::NDM; ++k) g = g + row[PCG_MAX_NX + PCG_MAX_NSP + k] * dv[k];
#pragma unroll
      for (int i = 0; i < M::NX; ++i) g = g + row[i] * x[i];
    } else {  // constraint_rows
#pragma unroll
      for (int i = 0; i < M::NX; ++i) g = g + row[i] * x[i];
#pragma unroll
      for (int k = 0; k < PCG_MAX_NSP; ++k) g = g + row[PCG_MAX_NX + k] * spv[k];
#pragma unroll
      for (int k = 0; k < PCG_MAX_NDM; ++k) g = g + row[PCG_MAX_NX + PCG_MAX_NSP + k] * dv[k];
    }
#pragma unroll
    for (int j = 0; j < M::NA; ++j) g = g + row[PCG_MAX_NX + PCG_MAX_NSP + PCG_MAX_NDM + j] * u[j];
#pragma unroll
    for (int j = 0; j < M::NDM; ++j) g = g + row[PCG_MAX_NX + PCG_MAX_NSP + PCG_MAX_NDM + PCG_MAX_NA + j] * u[M::NA + j];
    if (g0) g0[(size_t)r * s0] = g;
    if (g1) g1[(size_t)r * s1] = g;
    violated |= (g > 0.0);
    gmax = (g > gmax) ? g : gmax;
  }
  return violated;
}

// env_post_cons (pcg_rollout_cons.hpp) with the post-step rows from cons_rows_max.  Statement by statement its arithmetic.
template <class M>
PCG_DEV void env_post_cons_max(const StepArgs& A, CDevConst& c, const ConsArgs& G, int64_t e, int t, const EnvPre<M>& pre,
                               const double (&x)[M::NX], int status, double* g0, double* g1, double& gmax, EnvOut<M>& out) {
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
      spv[k] = sched_at<false>(A.sched, nullptr, false, k, N, tc);
      spn[k] = sched_at<false>(A.sched, nullptr, false, k, N, tn);
    }
  const int t_new = t + 1;
  // ---- post-step constraints (pcgym.py:443-446) ----
  const bool violated = cons_rows_max<M>(c, G.order_w != 0, x, spv, dv, u, g0, G.g_cs, g1, B, gmax);
  done |= violated && (flags & PCG_F_DONE_ON_CONS);
  done |= (t_new == N - 1);  // pcgym.py:448-449
  out.done = done;
  out.viol = violated;
  // ---- reward on the noise-free state (pcgym.py:470-482) ----
  double r = 0.0;
  if (flags & PCG_F_REWARD_BATCH) {  // pcgym.py:502-532
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
  if (flags & PCG_F_NOISE) {
#pragma unroll
    for (int i = 0; i < NX; i += 2) {
      double z0, z1;
      rng_normal2(A.seed, env_id, (uint32_t)t, RNG_NOISE + (uint32_t)(i >> 1), z0, z1);
      zn[i] = z0;
      if (i + 1 < NX) zn[i + 1] = z1;
    }
  }
  double on[NX];  // physical observation of the states, noise included
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    on[i] = 0.0;
    if (i < nx) {
      double o = x[i];
      if (flags & PCG_F_NOISE) o += zn[i] * x[i] * c.noise_pct[i];
      on[i] = o;
      out.ox[i] = (o - c.omap[i].lo) * c.omap[i].sc + c.omap[i].off;
    }
  }
  if (flags & PCG_F_REWARD_TRACK) {  // the declarative tracking reward, as in env_post
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
        const double up = (up0 == up0) ? up0 : u[j];  // NaN: no previous action yet
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
#pragma unroll
  for (int k = 0; k < PCG_MAX_NSP; ++k)
    if (k < nso) out.osp[k] = (spv[k] - c.omap[nx + k].lo) * c.omap[nx + k].sc + c.omap[nx + k].off;
#pragma unroll
  for (int k = 0; k < PCG_MAX_NDM; ++k)
    if (k < nd) out.od[k] = (dv[k] - c.omap[nx + nso + k].lo) * c.omap[nx + nso + k].sc + c.omap[nx + nso + k].off;
}

// env_step_cons (pcg_rollout_cons.hpp) with env_post_cons_max: the pre-step check is cons_rows and leaves gmax alone
template <class M, int INTEG>
PCG_DEV void env_step_cons_max(const StepArgs& A, CDevConst& c, const ConsArgs& G, int64_t e, int t, const double (&a_in)[M::NA],
                               double (&x)[M::NX], double* g0, double* g1, double& gmax, EnvOut<M>& out) {
  constexpr int NX = M::NX;
  const int nx = M::DYNAMIC ? c.nx : NX;
  typename M::CKP& kp = model_kp<M>(c);
  EnvPre<M> pre;
  env_pre<M, false, true>(A, c, nullptr, e, t, a_in, x, pre);  // (A.g_pre is null here: its own check stores nothing)
  if (t == 0) {  // ---- pre-step constraint check at t == 0 (pcgym.py:414-420), in the per-step route's order ----
    double sp0[PCG_MAX_NSP];
#pragma unroll
    for (int k = 0; k < PCG_MAX_NSP; ++k) sp0[k] = (k < c.nsp_obs) ? c.x0[(M::DYNAMIC ? nx : NX) + k] : 0.0;
    const bool v = cons_rows<M>(c, G.order_w != 0, x, sp0, pre.dv, pre.u, G.g_pre ? G.g_pre + e : nullptr, A.B, nullptr, 0);
    pre.done_pre = v && (c.flags & PCG_F_DONE_ON_CONS);
  }
  const int status = integrate_env<M, INTEG, false>(A, c, kp, pre.u, x, nullptr, e, nx);
  env_post_cons_max<M>(A, c, G, e, t, pre, x, status, g0, g1, gmax, out);
}

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
    env_step_cons_max<M, INTEG>(A, c, G, e, A.t_scalar + s, a, x, G.g_seq ? G.g_seq + (size_t)s * G.g_ss + e : nullptr,
                                (last && G.g_last) ? G.g_last + e : nullptr, gmax, out);
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
    env_step_cons_max<M, INTEG>(A, c, G, e, A.t_scalar + s, a, x, G.g_seq ? G.g_seq + (size_t)s * G.g_ss + e : nullptr,
                                (last && G.g_last) ? G.g_last + e : nullptr, gmax, out);
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
