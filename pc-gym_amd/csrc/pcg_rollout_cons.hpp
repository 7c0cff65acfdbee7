// pcg_rollout_cons.hpp -- the closed-loop fused rollouts on plans WITH constraint rows, recording the rows
// (pcg_rollout_policy_cons, pcg_rollout_actor_cons).  rollout_policy_kernel's and rollout_actor_kernel's loops (one env per
// lane, state and observation in registers, the networks between two steps, the same Philox keys) with, per step s:
//   rows    the ncon affine rows g = A.[x|sp|d|u] - b after the step      -> g_seq[s * g_ss + r * g_cs + e]
//   flag    "any row > 0"                                                  -> viol_seq[s * v_ss + e] (one byte)
//   last    after the last step io->g / io->viol hold that step's rows and flag, io->done its done flag
//           (PCG_F_DONE_ON_CONS included): what pcg_step leaves
//   pre     at counter 0 the pre-step check of pcgym.py:414-420 writes io->g_pre and enters `done`, as in env_pre
// Either sequence may be null.  The flag feeds the -1000 penalty (PCG_F_R_PENALTY), the box excess of the tracking reward
// and `done`, so the order in which a row is summed is part of the result: cons_rows below states both orders the per-step
// route knows and the host picks the one pcg_step would run on the same buffers -- that of constraint_rows_w
// (pcg_step_feat.hpp: -b, set-point slots, disturbance slots, states ascending, actions, model disturbance inputs) where
// pcg_step takes the feature-masked kernel (RK4 plans of the small models, even 16-byte-aligned batches), that of
// constraint_rows (states first) everywhere else.  The recorded rows and flags are the per-step route's bits either way.
//
// After `done`: an env whose done flag is set mid-episode (PCG_F_DONE_ON_CONS, or the pre-step check) KEEPS STEPPING, exactly
// as the step loops of collect_rollouts / collect_onpolicy do, which never reset single envs of a lock-stepped batch; the
// done flag of a step says nothing about the steps after it.  A caller that wants to mask what follows a violation does it
// from viol_seq.
//
// The step is env_pre -> integrate_env -> env_post<M, false, true>, the per-step route's own second half, with the rows taken
// from cons_rows through env_post's `Rows` parameter (ConsRows below): set-point slot, done, reward, noise and observation
// are stated once, in pcg_kernels.hpp (the terms of the tracking reward are its contraction-free track_*_cost, in env_post and
// env_step_feat alike, which is what makes its bits the per-step route's).  env_pre's own pre-step check runs with a null
// g_pre and its verdict is replaced.  A kernel that needs the rows in a register beside their stores hands env_step_cons a
// hook (RowsMax: pcg_rollout_pop_cons.hpp).  The loops are restated and not shared with the unconstrained kernels for the
// reason pcg_rollout_policy.hpp gives.
//
// Out of scope: constraint expressions and user models (their run-time compiled closed-loop module carries the two
// unconstrained kernels only), float32 networks, per-env parameters, adaptive integrators, and the open-loop pcg_rollout*
// calls, which still keep only the last step's rows.
#pragma once

namespace pcg {

struct ConsArgs {
  double* g_seq;        // [T][ncon][B] recorded rows, or null
  int64_t g_ss, g_cs;   // element strides (step, component)
  uint8_t* viol_seq;    // [T][B] recorded flags, or null
  int64_t v_ss;
  double* g_last;       // io->g: rows of the last step, or null
  double* g_pre;        // io->g_pre: rows of the pre-step check at counter 0, or null
  int32_t order_w;      // sum the rows in constraint_rows_w's order (the per-step route takes the feature-masked kernel)
};

// What a kernel does with each post-step row value beside storing it (cons_rows' `See`): nothing ...
struct RowsUnseen {
  static PCG_DEV void see(double) {}
};
// ... or keeping the largest one.  This statement defines the maximum's bits: a NaN row leaves it unchanged.
// A hook is a type, and what it keeps travels beside it as trailing reference arguments (`seen`), the way cons_rows_max took
// `double& gmax` when it was a copy of cons_rows: with the reference held in a hook object passed by value, fourteen
// population kernels of the large models came out as other code (profiles/r26/cons_step_refactor.txt).
struct RowsMax {
  static PCG_DEV void see(double g, double& m) { m = (g > m) ? g : m; }
};

// constraint rows g = A.[x|sp|d|u] - b of one env in the per-step route's summation order; row r goes to g0[r * s0] and
// g1[r * s1] (each may be null) and to See::see(g, seen...); returns "any row > 0"
template <class M, class See = RowsUnseen, class... Seen>
PCG_DEV bool cons_rows(CDevConst& c, bool order_w, const double (&x)[M::NX], const double (&spv)[PCG_MAX_NSP],
                       const double (&dv)[PCG_MAX_NDM], const double (&u)[M::NA + M::NDM], double* g0, int64_t s0, double* g1,
                       int64_t s1, Seen&... seen) {
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
    See::see(g, seen...);
  }
  return violated;
}

// env_post's `Rows` for these kernels: the post-step rows from cons_rows.  What cons_rows needs beside the step's values comes
// as env_post's trailing arguments (pcg_kernels.hpp says why they are not members of this type).
template <class See>
struct ConsRows {
  template <class M, class... Seen>
  static PCG_DEV bool rows(CDevConst& c, const double (&x)[M::NX], const double (&spv)[PCG_MAX_NSP], const double (&dv)[PCG_MAX_NDM],
                           const double (&u)[M::NA + M::NDM], bool order_w, double* g0, int64_t s0, double* g1, int64_t s1,
                           Seen&... seen) {
    return cons_rows<M, See>(c, order_w, x, spv, dv, u, g0, s0, g1, s1, seen...);
  }
};

// one env step of a constrained plan: env_step<M, INTEG, false, false, true> with cons_rows in both constraint checks.
// g0 / g1: where this step's rows go (the sequence's row s, io->g on the last step), each may be null; `See` is shown the
// post-step rows alone: the pre-step check at counter 0 is no step of the call.
template <class M, int INTEG, class See = RowsUnseen, class... Seen>
PCG_DEV void env_step_cons(const StepArgs& A, CDevConst& c, const ConsArgs& G, int64_t e, int t, const double (&a_in)[M::NA],
                           double (&x)[M::NX], double* g0, double* g1, EnvOut<M>& out, Seen&... seen) {
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
  // (RowArgs spelled out: deduced, the by-value pack would copy what `seen` refers to)
  env_post<M, false, true, false, ConsRows<See>, bool, double*, int64_t, double*, int64_t, Seen&...>(
      A, c, nullptr, e, t, pre, x, status, out, G.order_w != 0, g0, G.g_cs, g1, A.B, seen...);
}

// rollout_policy_kernel's loop (pcg_rollout_policy.hpp) on a plan with constraint rows
template <class M, int INTEG>
__global__ __launch_bounds__(BLOCK, M::NX <= 10 ? PCG_POL_WPE : 1) void rollout_cons_policy_kernel(const StepArgs A, const PolicyArgs Q,
                                                                                                  const ConsArgs G) {
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
    env_step_cons<M, INTEG>(A, c, G, e, A.t_scalar + s, a, x, G.g_seq ? G.g_seq + (size_t)s * G.g_ss + e : nullptr,
                            (last && G.g_last) ? G.g_last + e : nullptr, out);
    if (G.viol_seq) G.viol_seq[(size_t)s * G.v_ss + e] = out.viol ? 1 : 0;
    if (A.rew_seq) A.rew_seq[(size_t)s * A.r_ss + e] = out.rew;
    if (A.obs_seq) store_obs<M>(A, c, out, A.obs_seq + (size_t)s * A.o_ss + e, A.o_cs);
    if (last) store_out<M>(A, c, e, out, A.obs + e);  // io->obs/rew/done/viol hold the last step
    else if (A.status && out.status != PCG_ST_OK) A.status[e] = out.status;
    policy_input<M, NIN>(c, out, in);
  }
#pragma unroll
  for (int i = 0; i < NX; ++i)
    if (i < nx) A.x[(size_t)i * B + e] = x[i];
}

// rollout_actor_kernel's loop (pcg_rollout_actor.hpp) on a plan with constraint rows
template <class M, int INTEG>
__global__ __launch_bounds__(BLOCK, M::NX <= 10 ? PCG_ACT_WPE : 1) void rollout_cons_actor_kernel(const StepArgs A, const ActorArgs Q,
                                                                                                 const ConsArgs G) {
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
    env_step_cons<M, INTEG>(A, c, G, e, A.t_scalar + s, a, x, G.g_seq ? G.g_seq + (size_t)s * G.g_ss + e : nullptr,
                            (last && G.g_last) ? G.g_last + e : nullptr, out);
    if (G.viol_seq) G.viol_seq[(size_t)s * G.v_ss + e] = out.viol ? 1 : 0;
    if (A.rew_seq) A.rew_seq[(size_t)s * A.r_ss + e] = out.rew;
    if (A.obs_seq) store_obs<M>(A, c, out, A.obs_seq + (size_t)s * A.o_ss + e, A.o_cs);
    if (last) store_out<M>(A, c, e, out, A.obs + e);  // io->obs/rew/done/viol hold the last step
    else if (A.status && out.status != PCG_ST_OK) A.status[e] = out.status;
    policy_input<M, NIN>(c, out, in);
  }
#pragma unroll
  for (int i = 0; i < NX; ++i)
    if (i < nx) A.x[(size_t)i * B + e] = x[i];
}

}  // namespace pcg
