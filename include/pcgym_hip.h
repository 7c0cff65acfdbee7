/*
 * pcgym_hip.h -- C ABI of libpcgym_hip.so, the MI355X (gfx950) batched
 * process-control environment engine.
 *
 * This is the drop-in boundary for pc-gym's per-timestep hot path.  In the
 * reference (pc-gym v0.1.8, all Python) that path is
 *
 *     make_env.step            src/pcgym/pcgym.py:350-500
 *       -> integration_engine.casadi_step / jax_step
 *                              src/pcgym/integrator.py:65-107, 163-182
 *       -> model.__call__      src/pcgym/model_classes.py:45-62, 370-412,
 *                                                        790-845, 891-913, 1272-1319
 *     make_env.reset           src/pcgym/pcgym.py:263-349
 *
 * one env per Python object, one CVODES object rebuilt per step.  Here the same
 * arithmetic runs for B environments per launch, one wavefront lane per
 * environment, over caller-owned SoA fp64 buffers  field[component][B].
 *
 * Conventions
 *   - plain C types only; no torch / C++ types cross this boundary.
 *   - every entry point returns an int status: 0 = ok, <0 = PCG_E_* (bad
 *     argument), >0 = a hipError_t.  Nothing throws, nothing calls exit().
 *   - all device buffers are caller-owned (e.g. torch tensors); the library
 *     allocates only the opaque plan (a few KB of device constants, the schedules and
 *     sample tables) and, on request, step-graph objects.
 *   - launches are asynchronous on the hipStream_t passed as `stream`
 *     (NULL = the default stream).  One plan may be driven by one host thread at
 *     a time; distinct plans / streams / devices are independent.
 *   - a plan belongs to the device that was current at pcg_plan_create().
 */
#ifndef PCGYM_HIP_H
#define PCGYM_HIP_H

#ifndef __HIPCC_RTC__
#include <stdint.h>
#else /* hipRTC (run-time compilation of the kernel headers with user expressions) ships no <stdint.h> */
typedef signed char int8_t;
typedef unsigned char uint8_t;
typedef short int16_t;
typedef unsigned short uint16_t;
typedef int int32_t;
typedef unsigned int uint32_t;
typedef long int64_t;
typedef unsigned long uint64_t;
typedef unsigned long uintptr_t;
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define PCG_ABI_VERSION 16

#ifndef PCG_API
#define PCG_API __attribute__((visibility("default")))
#endif

/* capacity limits (compile-time; per-lane state lives in VGPRs) */
#define PCG_MAX_NX 24     /* physical states          */
#define PCG_MAX_NA 5      /* action dims              */
#define PCG_MAX_NDM 4     /* model disturbance inputs */
#define PCG_MAX_NSP 4     /* set-point keys           */
#define PCG_MAX_NCON 8    /* constraint rows          */
#define PCG_MAX_NUNC 8    /* uncertain parameters     */
#define PCG_MAX_PARAMS 128
#define PCG_MAX_NOBS (PCG_MAX_NX + PCG_MAX_NSP + PCG_MAX_NDM + PCG_MAX_NUNC)
#define PCG_MAX_NU (PCG_MAX_NA + PCG_MAX_NDM)
#define PCG_MAX_N 4096    /* episode length (schedule rows staged in LDS) */

/* status codes */
#define PCG_OK 0
#define PCG_E_NULL -1        /* required pointer is NULL                 */
#define PCG_E_MODEL -2       /* unknown model / integrator id            */
#define PCG_E_DIM -3         /* a dimension is out of range / mismatched */
#define PCG_E_VALUE -4       /* invalid scalar (dt<=0, substeps<1, ...)  */
#define PCG_E_PLAN -5        /* plan handle invalid / wrong device       */
#define PCG_E_UNSUPPORTED -6 /* combination not built                    */
#define PCG_E_JIT -7         /* a user expression did not compile (pcg_last_jit_log() has the compiler output) */

/* per-env health of a step, written to pcg_buffers.status (the reference's CVODES raises on an integration
 * failure, integrator.py:90-107; a batched kernel cannot raise per env, so it reports) */
#define PCG_ST_OK 0         /* the step was integrated over the full [0,dt] and the state is finite        */
#define PCG_ST_MAX_STEPS 1  /* DOPRI5: step budget (cfg.max_steps) exhausted before dt; state set to NaN    */
#define PCG_ST_UNDERFLOW 2  /* DOPRI5: step size underflow (blow-up / NaN right-hand side); state NaN      */
#define PCG_ST_NONFINITE 3  /* the integrator finished but the state is not finite (e.g. fixed-step RK4
                               outside its stability region, model_classes.py:1313 division by zero)     */

/* model ids: the reference registry keys (pcgym.py:128-148) that are on the hot path */
enum pcg_model {
  PCG_MODEL_CSTR = 0,          /* model_classes.py:23-62     nx=2  nu=1 (+Ti,Caf)      */
  PCG_MODEL_FOUR_TANK = 1,     /* model_classes.py:864-931   nx=4  nu=2                */
  PCG_MODEL_ME = 2,            /* model_classes.py:346-430   nx=10 nu=2 (+X0,Y6)       */
  PCG_MODEL_ME_REACTIVE = 3,   /* model_classes.py:763-861   nx=20 nu=2                */
  PCG_MODEL_CRYST = 4,         /* model_classes.py:1232-1345 nx=7  nu=1                */
  PCG_MODEL_AFFINE = 5,        /* custom_model whose RHS is affine: dx = A x + B u + c
                                  (pcgym.py:150-153; the reference's only KAT,
                                  tests/environment/test_make_env_custom_model.py:66-86); also carries the
                                  affine registry models hydraulic_tank :128-153, first_order_system :296-343,
                                  nonsmooth_control :509-558 (matrices built on the host) */
  /* "next" row f-2: further registry models (general kernels only, no streaming specialisation) */
  PCG_MODEL_COMPLEX_CSTR = 6,  /* model_classes.py:65-125   nx=4 nu=1 (+Ti,Caf) */
  PCG_MODEL_DISEASE = 7,       /* model_classes.py:156-183  nx=3 nu=1            */
  PCG_MODEL_BATCH = 8,         /* model_classes.py:222-265  nx=4 nu=1            */
  PCG_MODEL_PHOTO = 9,         /* model_classes.py:433-506  nx=3 nu=2 ("photobioreactor") */
  PCG_MODEL_CSTR_SERIES = 10,  /* model_classes.py:611-679  nx=4 nu=4            */
  PCG_MODEL_DISTILLATION = 11, /* model_classes.py:682-760  nx=9 nu=2            */
  PCG_MODEL_POLYMER = 12,      /* model_classes.py:1158-1229 nx=3 nu=4           */
  PCG_MODEL_BIOFILM = 13,      /* model_classes.py:1046-1155 nx=16 nu=5          */
  PCG_MODEL_HEAT_EX = 14,      /* model_classes.py:935-1044 nx=24 nu=4           */
  PCG_MODEL_INV_BATCH = 15,    /* model_classes.py:268-293 nx=4, no inputs (one ignored dummy action) */
  PCG_MODEL_OSCILLATORS = 16,  /* model_classes.py:186-216 nx=20 (N=10), no inputs (dummy action)     */
  PCG_MODEL_USER = 17,         /* custom_model with an arbitrary (non-affine) right-hand side (pcgym.py:150-153,
                                  tests/environment/test_make_env_custom_model.py:7-25): given as C source in
                                  pcg_env_cfg.user_rhs_src and compiled into this plan's kernels with hipRTC;
                                  nx <= PCG_MAX_NX, na <= PCG_MAX_NA, ndm <= PCG_MAX_NDM, n_params <= PCG_MAX_USER_PARAMS */
  PCG_MODEL_COUNT = 18
};
#define PCG_MAX_USER_PARAMS 64

/* integrators replacing integrator.py:90-107 (CVODES) / :65-88 (diffrax Tsit5) */
enum pcg_integrator {
  PCG_INT_RK4 = 0,     /* classical RK4, `substeps` equal sub-steps per env step (zero-order hold on u) */
  PCG_INT_DOPRI5 = 1,  /* adaptive Dormand-Prince 5(4), per-lane step size, rtol/atol
                          (mirrors integrator.py:61 PIDController(rtol=1e-8, atol=1e-8)) */
  PCG_INT_RODAS3 = 2,  /* stiff-capable: adaptive Rodas3 (4-stage linearly implicit Rosenbrock 3(2), L-stable; forward-
                          difference Jacobian, per-lane pivoted LU in LDS), rtol/atol/max_steps as for DOPRI5.  The
                          reference integrates with CVODES BDF (integrator.py:163-182).  Every model (nx <= 24);
                          pcg_step, pcg_step_autoreset, pcg_graph_* and pcg_integrate; pcg_rollout and plans with
                          per-env uncertain parameters return PCG_E_UNSUPPORTED */
  PCG_INT_RODAS4 = 3,  /* stiff-capable, fourth order: adaptive Rodas4 (Hairer & Wanner's RODAS: 6-stage linearly implicit
                          Rosenbrock 4(3) pair, gamma = 1/4, L-stable, stiffly accurate), same controller family as
                          Rodas3 (RMS norm, quantised factor 0.9 E^-1/4 in [0.2, 6]).  Linear algebra: models with a
                          structured analytic Jacobian (the 10-state extraction cascade: block-bidiagonal in both
                          directions) factor and solve W = I/(gamma h) - J in registers (6 reciprocals and ~230 flops per
                          step); every other model uses the forward-difference Jacobian and the per-lane pivoted LU in
                          LDS of Rodas3.  END-POINT ERROR CONTROL (cfg.ep_kmax > 0, models with a contraction-rate
                          hook): an env step only hands x(dt) on, and an error committed at time t is damped by
                          exp(-mu (dt - t)) on its way there, so the local tolerance of an attempted step ending at t'
                          is multiplied by 2^k, k = min(ep_kmax, floor(ep_frac mu log2(e) (dt - t'))) -- exact powers of
                          two, bit-identical in kernel and oracle.  The reference integrates with CVODES BDF
                          (integrator.py:163-182).  pcg_step, pcg_step_autoreset, pcg_graph_*, pcg_integrate;
                          pcg_rollout and per-env uncertain parameters: PCG_E_UNSUPPORTED */
  PCG_INT_TSIT5 = 4,   /* Tsitouras 5(4), FSAL: the method of the reference's jax path (integrator.py:56-61, diffrax.Tsit5 with
                          PIDController(rtol = atol = 1e-8)); controller, norm, initial step and failure semantics of
                          PCG_INT_DOPRI5.  General kernel (both counter modes), pcg_step_autoreset, pcg_graph_*,
                          pcg_integrate; pcg_rollout and per-env uncertain parameters: PCG_E_UNSUPPORTED */
  PCG_INT_RK4G = 5,    /* GUARDED RK4: `substeps` equal RK4 sub-steps, accepted per env only while the model's guard says the
                          fixed step is accurate -- no growing mode (largest growth rate g <= 0) and a resolved fastest
                          rate (rho h <= 1) at every sub-step start and at the end state, finite result; an env that
                          fails the guard is re-integrated from its start state by PCG_INT_DOPRI5 at rtol / atol before
                          pcg_step returns its launches to the stream -- inside the same kernel, or, for batches that fill
                          the chip, by a second launch of the adaptive pair's work-queue kernel over exactly the envs the
                          first one marked (same arithmetic per env, same bits; `done` holds the mark 2 only between the
                          two: a consumer of `done` on ANOTHER stream must order itself behind the whole pcg_step, as for any
                          output; should the second launch fail to start, pcg_step returns its error and the marked envs keep
                          done == 2 with their state, observation and counters of the step not advanced) -- (nsteps reports (0,0) for accepted envs, the pair's counts otherwise).  Models
                          with a guard hook only (cstr: the ignition branch).  The guard is the ONLY test -- RK4 carries no
                          error estimate -- and it is calibrated on the cstr's observation box and action box: an opt-in
                          for that box (the model's default plan is PCG_INT_T5G, which also checks an estimate).  General
                          kernel, pcg_step_autoreset, pcg_graph_*, pcg_integrate, pcg_rollout; not with per-env uncertain
                          parameters */
  PCG_INT_T5G = 6,     /* GUARDED FIXED-STEP TSIT5: `substeps` equal steps of Tsit5's fifth-order solution weights, TRUSTED per
                          env while (i) the model's guard holds at the START and END state of every step (g <= 0, rho h <= 2; the five
                          inner stage states change no decision once the estimate of (ii) is checked)
                          and (ii) the pair's own embedded 5(4) error estimate of every step stays below 4e-7 |x| + 4e-9 (RMS;
                          the seventh stage it needs is the next step's first stage and the end-state guard: no extra
                          evaluation); otherwise PCG_INT_DOPRI5 from the start state at rtol / atol, in one launch or two as
                          PCG_INT_RK4G (same nsteps convention).  Calibrated so that the canonical cstr loop is never
                          escalated and every trusted env of a wide state / input / step-size box lies inside 3 x the
                          reference's CVODES tolerances (1e-6 |x| + 1e-8) of the true solution.  12 + 1 evaluations per
                          canonical cstr step: the default plan of the cstr.  Models with a guard hook only; general kernel,
                          pcg_step_autoreset, pcg_graph_*, pcg_integrate, pcg_rollout; not with per-env uncertain
                          parameters */
  PCG_INT_CV8 = 7,     /* Cooper & Verner's explicit Runge-Kutta method of order 8 (11 stages), `substeps` equal steps per
                          env step: for smooth right-hand sides one step replaces several RK4 steps (four_tank's default
                          plan: 11 evaluations instead of 20 at a smaller error).  Kernels of PCG_INT_RK4: lean pipelined
                          kernel (small models), general kernel, pcg_step_autoreset, pcg_graph_*, pcg_integrate,
                          pcg_rollout; not with per-env uncertain parameters */
  PCG_INT_RODAS5 = 8,  /* stiff-capable, fifth order (ABI 13): adaptive Rodas5 (Di Marzo's coefficient set, the one of Hairer &
                          Wanner's RODAS5 code: 8-stage linearly implicit Rosenbrock 5(4) pair, gamma = 0.19, L-stable, stiffly
                          accurate).  Everything but the tableau and the controller's exponent (quantised factor 0.9 E^-1/5 in
                          [0.2, 6]) is PCG_INT_RODAS4's: linear-algebra policy (structured W in registers / dense W in LDS),
                          error norm, END-POINT ERROR CONTROL (cfg.ep_frac / ep_kmax), cooperative rule (cfg.coop_thr), first
                          step, failure semantics, entry points.  The extraction cascade is accuracy-bound under the fourth-
                          order pair (17.6 attempts per env step for 1e-6 of a 1e-13 solve); this pair reaches the same class in
                          0.6 x the attempts at 8 stages against 6: the default plan of multistage_extraction.  The reference
                          integrates with CVODES BDF, variable order up to 5 (integrator.py:163-182) */
  PCG_INT_COUNT = 9
};

/* cfg.flags */
#define PCG_F_NORMALISE_A 0x0001u   /* pcgym.py:59,372-375                                     */
#define PCG_F_NORMALISE_O 0x0002u   /* pcgym.py:60,483-489                                     */
#define PCG_F_A_DELTA 0x0004u       /* pcgym.py:57,376-383                                     */
#define PCG_F_R_PENALTY 0x0008u     /* pcgym.py:121,556-557 / 529-530                          */
#define PCG_F_DONE_ON_CONS 0x0010u  /* pcgym.py:120,613-614                                    */
#define PCG_F_NOISE 0x0020u         /* pcgym.py:453-466 multiplicative Gaussian obs noise      */
#define PCG_F_REWARD_BATCH 0x0040u  /* terminal reward, pcgym.py:502-532 (else SP reward)      */
#define PCG_F_MAXIMISE 0x0080u      /* batch reward sign, pcgym.py:524-527                     */
#define PCG_F_REF_COMPAT 0x0100u    /* replicate reference quirks Q1 (double action
                                       de-normalisation when normalise_a && a_delta,
                                       pcgym.py:372-379) and Q3 (constraint rows see a
                                       re-"de-normalised" state/input, pcgym.py:597-608)       */
#define PCG_F_GAUSS_DIST 0x0200u    /* extension: d = d_sched + d_sigma*z, z~N(0,1) Philox,
                                       clipped to [d_clip_lo,d_clip_hi] (BASELINE configs[4])  */
#define PCG_F_X0_NORMAL 0x0400u     /* reset-time x0 / parameter uncertainty is normal (else uniform),
                                       pcgym.py:255-261                                        */
#define PCG_F_UNC_EMPIRICAL 0x0800u /* uncertain parameters are drawn uniformly from per-parameter sample
                                       tables (env_params["empirical_distribution"], pcgym.py:311-316:
                                       np.random.choice) instead of value*(1 +- pct)           */
#define PCG_MAX_EMP 65536           /* total empirical samples over all parameters            */
#define PCG_F_REWARD_TRACK 0x1000u  /* declarative form of the custom_reward family every paper script uses
                                       (pc-gym_paper/train_policies/cstr/custom_reward.py:3-39, 4tank_train.py:16-52,
                                       me_train.py:17-53, Biofilm/biofilm_train.py:13-41, constraint_showcase/
                                       custom_reward.py:6-69):  r = -( sum_k r_scale_k ((o_k - SP_k[t]) / (hi_k - lo_k))^2
                                       + sum_j [ R_du (du_j / (a_hi_j - a_lo_j))^2 + R_u ((u_j - a_lo_j) / (a_hi_j - a_lo_j))^2 ]
                                       + [violated] sum_c box_c^2 )  on the (noisy) physical observation o and the
                                       physical action u, with the previous action kept per env in u_prev         */
#define PCG_F_REWARD_CRYST 0x2000u  /* with PCG_F_REWARD_TRACK on the crystallisation model: the tracked CV and Ln are
                                       recomputed from the observed moments, CV = sqrt(mu2 mu0 / mu1^2 - 1), Ln = mu1/mu0
                                       (pc-gym_paper/train_policies/crystalisation/cryst_train.py:17-48)                 */
#define PCG_MAX_RBOX 4              /* state boxes of the constraint-violation term                               */

/*
 * Environment configuration: the numeric content of the reference's
 * env_params dict (pcgym.py:32-253).  All arrays are small HOST arrays, copied
 * at pcg_plan_create(); pointers may be NULL when the matching count is 0.
 *
 * Layout of one env's "state"/observation vector, as in the reference
 * (pcgym.py:160-165,291-298,409-410,432-438):
 *      [ x(0..nx) | SP slot (nsp_obs) | configured disturbances (nd) | uncertain parameters (nunc) ]
 *                                                                   Nobs = nx+nsp_obs+nd+nunc
 *      (reset order of the reference, pcgym.py:291-316; with disturbances AND parameter uncertainty the
 *      reference's step() writes the disturbance slots at a different offset -- quirk Q11: this layout is
 *      kept in step() too, see d_param_index)
 * and of the model input vector (pcgym.py:371,386-404):
 *      uk = [ action (na) | model disturbance inputs (ndm) ]            Nu = na+ndm
 */
typedef struct pcg_env_cfg {
  int32_t model_id;       /* enum pcg_model */
  int32_t integrator_id;  /* enum pcg_integrator */
  int32_t nx;             /* physical states (reference: Nx_oracle)                     */
  int32_t na;             /* action dims (len(a_space.low))                             */
  int32_t ndm;            /* len(model.info()["disturbances"]) if disturbances active, else 0 */
  int32_t nd;             /* configured disturbance keys (reference: Nd), <= ndm         */
  int32_t nsp;            /* len(SP)                                                    */
  int32_t nsp_obs;        /* SP slots present in the state/obs vector: nsp when x0 carries them
                             (len(x0) == nx+nsp, the documented form), 0 when x0 has only the nx
                             physical states -- the reference then silently drops the SP slot
                             (pcgym.py:438 assigns into an empty slice), as in its own KAT      */
  int32_t ncon;           /* constraint rows (reference: n_con)                         */
  int32_t nrew;           /* batch reward: number of reward states                      */
  int32_t nunc;           /* uncertain model parameters sampled per env at reset (pcgym.py:301-310) */
  int32_t N;              /* episode length (reference: N); done when t == N-1          */
  int32_t substeps;       /* RK4 sub-steps per env step (>=1)                           */
  int32_t max_steps;      /* DOPRI5: step budget per env step (accepted+rejected)       */
  uint32_t flags;         /* PCG_F_*                                                    */
  int32_t n_params;
  double dt;              /* tsim / N  (pcgym.py:110)                                   */
  double rtol, atol;      /* DOPRI5 tolerances                                          */

  const double* params;   /* [n_params] model parameters, order = pcg_model_param_names() */
  const double* x0;       /* [nx+nsp_obs] reference x0 incl. SP slots (pcgym.py:108,284) */
  const double* x0_unc;   /* [nx] or NULL: reset-time x0 uncertainty fraction (pcgym.py:285-288) */
  const double* a_low;    /* [na] a_space                                               */
  const double* a_high;   /* [na]                                                       */
  const double* a_act_low;   /* [na] a_space_act (a_delta clip), pcgym.py:383           */
  const double* a_act_high;  /* [na]                                                    */
  const double* a_0;      /* [na] a_delta initial action (pcgym.py:58,320)              */
  const double* o_low;    /* [Nobs] observation_space_base incl. disturbance bounds     */
  const double* o_high;   /* [Nobs]                                                     */
  const uint8_t* obs_mask;/* [nx] or NULL: 1 = observed (partial_observation)           */
  const int32_t* sp_index;/* [nsp] state index of each SP key (pcgym.py:553)            */
  const double* sp;       /* [nsp][N] set-point schedules                               */
  const double* r_scale;  /* [nsp] (SP reward) or [nrew] (batch reward)                 */
  const int32_t* rew_index;  /* [nrew] batch reward state indices                       */
  const int32_t* d_slot;  /* [nd] for each configured key, its index in the model's
                             disturbance list (ascending; pcgym.py:392-398)             */
  const double* d_sched;  /* [nd][N] disturbance schedules (pcgym.py:173,394)           */
  const double* d_default;/* [ndm] model default for unconfigured inputs (pcgym.py:400-404) */
  const double* d_sigma;  /* [nd] PCG_F_GAUSS_DIST                                      */
  const double* d_clip_lo;/* [nd]                                                       */
  const double* d_clip_hi;/* [nd]                                                       */
  const double* con_A;    /* [ncon][Nobs+Nu] affine constraint rows g = A.[state;uk] - b <= 0,
                             the declarative form of the reference's callable g(x,u)
                             (pcgym.py:560-577, docs/guides/constraints.md:35-51)       */
  const double* con_b;    /* [ncon]                                                     */
  const double* noise_pct;/* [nx] per-state noise fraction (pcgym.py:454-466)           */
  const int32_t* unc_index; /* [nunc] index of each uncertain parameter in `params`       */
  const double* unc_pct;  /* [nunc] uncertainty fraction (uniform half-width / normal sigma, pcgym.py:255-261) */
  const double* unc_emp;  /* PCG_F_UNC_EMPIRICAL: concatenated sample tables, parameter j owns
                             unc_emp[unc_emp_off[j] .. unc_emp_off[j+1])                   */
  const int32_t* unc_emp_off; /* [nunc+1], unc_emp_off[0] = 0                              */
  /* PCG_F_REWARD_TRACK */
  double rew_R_du;        /* weight of the squared normalised action increment (R in custom_reward.py:6)     */
  double rew_R_u;         /* weight of the squared normalised action itself (biofilm_train.py:16,39)         */
  int32_t rew_nbox;       /* state boxes penalised while a constraint row is violated (0..PCG_MAX_RBOX)      */
  const int32_t* rew_box_index; /* [rew_nbox] state index                                                     */
  const double* rew_box_lo;     /* [rew_nbox] physical lower bound (constraint_showcase/custom_reward.py:4-5) */
  const double* rew_box_hi;     /* [rew_nbox] physical upper bound                                            */
  /* User expressions: the NON-affine form of the reference's callables (constraints(x,u) pcgym.py:119-125, 560-577;
   * custom_reward(self, obs, uk, violated) pcgym.py:201-205, 470-471), given as C source and compiled into this plan's
   * step kernel with hipRTC at pcg_plan_create() (cached by source hash: in the process and under $PCG_JIT_CACHE).
   *   user_cons_src    statements that fill g[0 .. ncon-1] (double) from  x[] = the reference's state vector
   *                    [x | SP slots | disturbances] (physical units) and u[] = uk [action | disturbance inputs];
   *                    con_A / con_b are ignored when it is given.  Quirk Q3 (state / input "de-normalised" once
   *                    more under PCG_F_REF_COMPAT with normalisation on) is applied to x[] and u[] first, as for rows.
   *   user_reward_src  ONE expression of type double over  o[] = the (noisy) physical observation vector the reference
   *                    hands to custom_reward, x[] = the noise-free state vector, u[] = uk, sp[] = SP_k[t] at the new t,
   *                    violated (0/1), t (new step counter), N.  Replaces the built-in reward.
   * Available in the one-env-per-lane general kernel only (any integrator, lock-stepped or per-env counters) and in
   * pcg_rollout (the run-time compiled module carries its own fused rollout kernel; not for the Rosenbrock integrators,
   * whose matrices live in LDS); not with per-env uncertain parameters or pcg_graph.  Math: exp log sqrt pow fabs fmin
   * fmax sin cos tanh. */
  const char* user_cons_src;
  const char* user_reward_src;
  const char* jit_include_dir;  /* directory holding pcg_kernels.hpp and its siblings (the library's own csrc/)      */
  /* PCG_MODEL_USER: the model's right-hand side (the reference's custom_model.__call__(x, u), pcgym.py:150-153) as C
   * statements that fill dx[0 .. nx-1] (double) from x[] (nx states), u[] (na inputs, then ndm disturbance inputs) and
   * p[] (n_params parameters = cfg.params).  Compiled with hipRTC into this plan's general step kernel (both time
   * modes), pcg_integrate, pcg_rhs and pcg_rollout (the last not for PCG_INT_RODAS3 / PCG_INT_RODAS4 / PCG_INT_RODAS5); any integrator;
   * composes with user_cons_src / user_reward_src.  Not available: per-env uncertain parameters. */
  const char* user_rhs_src;
  /* PCG_INT_RODAS4 / PCG_INT_RODAS5, end-point error control (see enum pcg_integrator): 0 / 0 = classical local error control */
  double ep_frac;         /* fraction of the model's contraction rate credited to the damping (0.5 by default: the cascade
                             is non-normal -- a perturbation travels down the stages before it decays)                 */
  int32_t ep_kmax;        /* largest exponent: tolerances are relaxed by at most 2^ep_kmax (0 = off; the Python side's defaults:
                             10 under PCG_INT_RODAS4, 16 under PCG_INT_RODAS5, whose attempts additionally cap the exponent
                             at 2 bits per remaining step of their size, trunc(2 (dt - t') / h): a Rosenbrock step damps a
                             stiff component by |R(h lambda)| ~ 0.1-0.16 only, whatever exp(h lambda) says)              */
  /* Disturbances TOGETHER with per-env uncertain parameters (pcgym.py:291-316, 386-412; quirk Q11).  The state /
   * observation layout is the reference's reset() order [x | SP | d | unc] in reset AND step (its step() writes the
   * disturbance slots at another offset -- the one place where this engine deliberately does not follow it); a model
   * disturbance input that is NOT configured takes the env's own (possibly uncertain) parameter value, as the
   * reference's `self.model.info()["parameters"][k]` does (pcgym.py:400-404).  d_param_index names that parameter. */
  const int32_t* d_param_index; /* [ndm] or NULL: index in `params` of each model disturbance input                  */
  /* PCG_INT_RODAS4 / PCG_INT_RODAS5 on a model with a cooperative rule (multistage_extraction with eq_exponent == 2): env steps whose
   * predicted cost -- the model's fit of the pair's attempts per env step from the held input and the scaled size of
   * f(x0), in exact arithmetic -- reaches coop_thr are integrated by SEULEX-8 (extrapolated linearly implicit Euler, fixed
   * column of eight, same accuracy class: pcg_seulex.hpp) instead of the pair.  In the work-queue kernel eight lanes share
   * such an env (one row of the extrapolation tableau each), elsewhere one lane runs the eight rows: the same bits either
   * way (the threshold counts attempts of the FOURTH-order pair under either).  A launch is as long as its heaviest env; this is what shortens it (the reference's CVODES integrates a stiff
   * column at a cost that does not depend on its batch-mates, integrator.py:163-182).  0 = off (every env takes the pair);
   * nsteps then counts big steps for the heavy envs.  PCG_E_UNSUPPORTED for other models / integrators when > 0. */
  double coop_thr;
} pcg_env_cfg;

/*
 * Per-call device buffers (caller-owned, SoA, fp64 unless noted).
 * "in/out" buffers are updated in place.
 */
typedef struct pcg_buffers {
  int64_t B;          /* environments in this launch                                            */
  double* x;          /* [nx][B]    in/out  physical state                                      */
  const double* a;    /* [na][B]    in      policy action (normalised if PCG_F_NORMALISE_A)     */
  const double* d;    /* [nd][B]    in|NULL per-env explicit disturbance values for this step;
                                            NULL = use the plan's shared schedule               */
  int32_t* t;         /* [B]        in/out|NULL per-env step counter; NULL = lock-stepped batch,
                                            the scalar `t` argument is used                     */
  double* a_save;     /* [na][B]    in/out|NULL a_delta accumulator (required with PCG_F_A_DELTA) */
  double* obs;        /* [Nobs][B]  out     observation                                         */
  double* rew;        /* [B]        out     reward                                              */
  uint8_t* done;      /* [B]        out     episode finished                                    */
  uint8_t* viol;      /* [B]        out|NULL any constraint row > 0 after the step              */
  double* g;          /* [ncon][B]  out|NULL constraint rows after the step (cons_info[:,t,:])  */
  double* g_pre;      /* [ncon][B]  out|NULL rows of the pre-step check the reference runs when
                                            t==0 (pcgym.py:416-420); untouched for other t      */
  int32_t* nsteps;    /* [2][B]     out|NULL DOPRI5 accepted / rejected step counts             */
  double* u_prev;     /* [na][B]    in/out|NULL previous physical action (required with PCG_F_REWARD_TRACK);
                                            NaN = "no previous action yet" (first step: du = 0, the reference's
                                            hasattr(self, 'u_prev') branch, custom_reward.py:7-8); pcg_reset
                                            leaves it alone, as the reference never clears u_prev              */
  double* p_unc;      /* [nunc][B]  in/out  per-env values of the uncertain parameters: written by
                                            pcg_reset, read by pcg_step (required when nunc > 0)        */
  uint8_t* status;    /* [B]     in/out|NULL per-env health, STICKY: a step that is not PCG_ST_OK writes its
                                            PCG_ST_* code, an OK step leaves the entry alone -- the buffer holds "what
                                            went wrong since the host last cleared it" and costs no traffic while
                                            nothing does.  An env whose adaptive integration fails gets a NaN state
                                            (never a silently wrong one) whether or not this buffer is given      */
} pcg_buffers;

typedef struct pcg_plan pcg_plan; /* opaque */

/* library / ABI version (PCG_ABI_VERSION). */
PCG_API int pcg_version(void);
/* Build id: a digest of the library's sources (csrc: the kernel headers and the .hip units) and of this header at build time (the Makefile's PCG_SRC_HASH;
   "unknown-build" for a build made without it).  Measurements that cannot be taken in-process -- the hardware-counter
   passes under profiles/ -- record it, and bench.py reports their traffic figures only for the build they were taken on. */
PCG_API const char* pcg_build_id(void);

/* human-readable text for a status returned by any entry point (static storage). */
PCG_API const char* pcg_strerror(int status);

/* model metadata = model.info() of the reference (model_classes.py:8-20, 414-430, ...):
 * fills nx, nu (inputs), ndm (disturbance inputs), n_params.  */
PCG_API int pcg_model_info(int model_id, int32_t* nx, int32_t* nu, int32_t* ndm, int32_t* n_params);

/* default parameter vector of a model, in the order the kernels expect
 * (= declaration order of the reference dataclass fields).  out has n_params slots. */
PCG_API int pcg_model_default_params(int model_id, double* out, int32_t n_out);

/* Build a plan: validates cfg, folds the affine maps (action de-normalisation,
 * observation normalisation, compat transforms) and uploads constants and
 * schedules to the current device.  Replaces integration_engine.__init__
 * (integrator.py:19-63) + make_env._setup_* numeric state (pcgym.py:56-253). */
PCG_API int pcg_plan_create(pcg_plan** out, const pcg_env_cfg* cfg);
PCG_API int pcg_plan_destroy(pcg_plan* plan);

/* Algorithmic HBM bytes one env-step moves for this plan and buffer set
 * (SURVEY.md section 8d formula); used by bench.py for the roofline line. */
PCG_API int64_t pcg_plan_bytes_per_env_step(const pcg_plan* plan, const pcg_buffers* io);

/* One fused environment step for B envs: replaces make_env.step (pcgym.py:350-500):
 * action map -> disturbance injection -> ODE integration over [0,dt] -> SP slot ->
 * constraint rows -> done -> observation noise -> reward -> observation normalisation.
 * `t` is the pre-step counter for lock-stepped batches (io->t == NULL).
 * `seed` keys the counter-based RNG (Philox4x32-10 on (seed, env index, t)). */
PCG_API int pcg_step(pcg_plan* plan, const pcg_buffers* io, int32_t t, uint64_t seed, void* stream);

/* Reset (pcgym.py:263-349): x <- x0 (with optional x0 uncertainty), t <- 0,
 * a_save <- a_0, obs <- normalised [x0 | SP slots of x0 | d[:,0]].
 * mask [B] u8 or NULL: only envs with mask!=0 are reset (masked auto-reset).
 * env_offset: global index of env 0 of this shard (keys the RNG; multi-GPU). */
PCG_API int pcg_reset(pcg_plan* plan, const pcg_buffers* io, const uint8_t* mask, uint64_t seed,
              void* stream);

/* Global env index of local env 0 (batch sharded over GPUs); default 0. */
PCG_API int pcg_plan_set_env_offset(pcg_plan* plan, int64_t env_offset);

/* Tuning / sharding options. */
#define PCG_OPT_ENV_OFFSET 1  /* same as pcg_plan_set_env_offset                              */
#define PCG_OPT_LDS_STAGES 2  /* DOPRI5: keep stage vectors k1..k6 in LDS [stage][comp][lane]
                                 (64-thread workgroups) instead of VGPRs; default 0           */
#define PCG_OPT_VARIANT 3     /* step-kernel selection: 0 auto (default), 1 classic one-env-per-lane
                                 grid, 2 streaming persistent kernel 1 env/lane, 3 streaming 2 envs/lane
                                 (16 B per lane accesses), 4 software-pipelined lean kernel; 5 = the in-workgroup
                                 WORK QUEUE for an adaptive plan of any model (by default only models with a cost
                                 key, the extraction columns, go through it): pays when the step counts of a batch
                                 are heavy-tailed -- cstr envs on the ignition branch under PCG_INT_DOPRI5: 572 ->
                                 451 us per 2^20-env step; costs when they are not (canonical cstr loop: 38 -> 90 us).
                                 1-4 are for A/B measurement                                                     */
#define PCG_OPT_STREAM_BLOCKS_PER_CU 4 /* streaming kernel: resident workgroups per CU (0 = occupancy query) */
#define PCG_OPT_NT_STORES 5   /* streaming kernel: non-temporal stores for obs / reward (not re-read by the step) */
PCG_API int pcg_plan_set_option(pcg_plan* plan, int option, int64_t value);

/* Host-only validation of a cfg: the status pcg_plan_create() would return before it
 * touches the device (usable on machines without a GPU). */
PCG_API int pcg_cfg_validate(const pcg_env_cfg* cfg);

/* Test hook: dx = f(x,u) of the plan's model for B envs.
 * x [nx][B], u [Nu][B] (physical units), dx [nx][B]. */
PCG_API int pcg_rhs(pcg_plan* plan, int64_t B, const double* x, const double* u, double* dx, void* stream);

/* Test hook: integrate only.  x [nx][B] in/out, u [Nu][B] physical, held for [0,dt]
 * (zero-order hold, integrator.py:163-182).  nsteps [2][B] or NULL. */
PCG_API int pcg_integrate(pcg_plan* plan, int64_t B, double* x, const double* u, int32_t* nsteps,
                  void* stream);

/* Open-loop fused rollout ("next" row f-1: counterpart of policy_eval.rollout,
 * policy_evaluation.py:71-130): T env steps with the state kept in registers.
 * a_seq [T][na][B]; obs_seq [T][Nobs][B]|NULL; rew_seq [T][B]|NULL; io->obs/rew/done
 * receive the last step.  Lock-stepped only (io->t must be NULL). */
PCG_API int pcg_rollout(pcg_plan* plan, const pcg_buffers* io, int32_t t0, int32_t T, const double* a_seq,
                double* obs_seq, double* rew_seq, uint64_t seed, void* stream);

/* pcg_rollout with explicit element strides (step, component) for the three sequences; the env index is
 * unit-stride.  Lets the collector write straight into the reference's axis order
 * x (Nx, N, reps), u (Nu, N, reps), r (1, N, reps)  (policy_evaluation.py:155-197):
 * obs_comp_stride = N*B, obs_step_stride = B.  Strides must keep rows 16-byte aligned for the 2-env/lane path.
 * PCG_E_DIM for a layout whose rows would overlap: a_comp_stride or obs_comp_stride < B, rew_step_stride < B (T > 1),
 * or observation rows that are neither step-major (obs_step_stride >= (Nobs-1) obs_comp_stride + B) nor
 * component-major (obs_step_stride >= B and obs_comp_stride >= (T-1) obs_step_stride + B).  a_seq is only read:
 * its step stride is free (0 holds one action row for all T steps). */
PCG_API int pcg_rollout_strided(pcg_plan* plan, const pcg_buffers* io, int32_t t0, int32_t T, const double* a_seq,
                                int64_t a_step_stride, int64_t a_comp_stride, double* obs_seq,
                                int64_t obs_step_stride, int64_t obs_comp_stride, double* rew_seq,
                                int64_t rew_step_stride, uint64_t seed, void* stream);

/* Closed-loop fused rollout with an on-device policy (ABI 15).  The policy is DECLARATIVE: a small fp64 multi-layer
 * perceptron, the shape stable-baselines3's MlpPolicy produces (the reference evaluates policy.predict(obs) on the host
 * between two env.step() calls, policy_evaluation.py:86-128):
 *     h1 = act(W[0] obs + b[0]);  h2 = act(W[1] h1 + b[1]);  a = out_map(W[n_hidden] h + b[n_hidden])
 * with 0, 1 or 2 hidden layers; n_hidden == 0 is affine state feedback a = W obs + b. */
#define PCG_ACT_TANH 0
#define PCG_ACT_RELU 1
#define PCG_POL_NONE 0   /* a = the last layer's output                        */
#define PCG_POL_CLIP 1   /* ... clipped to [out_low, out_high]                 */
#define PCG_POL_TANH 2   /* ... squashed by tanh                               */
#define PCG_POL_MAX_WIDTH 64
typedef struct pcg_policy_cfg {
  int32_t n_in, n_out;        /* must equal the plan's Nobs and na                                  */
  int32_t n_hidden;           /* 0, 1 or 2 hidden layers                                            */
  int32_t width[2];           /* 1..PCG_POL_MAX_WIDTH each (entries past n_hidden are ignored)      */
  int32_t activation;         /* PCG_ACT_TANH | PCG_ACT_RELU                                        */
  int32_t out_map;            /* PCG_POL_NONE | PCG_POL_CLIP | PCG_POL_TANH                         */
  double out_low, out_high;   /* PCG_POL_CLIP: out_low <= out_high                                  */
  const double* W[3];         /* host, row-major [n_next][n_prev]; layers 0 .. n_hidden             */
  const double* b[3];         /* host, [n_next]                                                     */
} pcg_policy_cfg;
typedef struct pcg_policy pcg_policy; /* opaque; its weights change only through pcg_policy_update() (ABI 16) */

/* Host-only validation of a policy configuration (usable without a GPU): the status pcg_policy_create() would return
 * before it touches the device.  PCG_E_DIM: n_in outside 1..PCG_MAX_NOBS, n_out outside 1..PCG_MAX_NA, n_hidden outside
 * 0..2, a width outside 1..PCG_POL_MAX_WIDTH; PCG_E_NULL: a missing matrix / bias; PCG_E_VALUE: unknown activation /
 * output map, out_low > out_high (or not finite) under PCG_POL_CLIP, a weight that is not finite. */
PCG_API int pcg_policy_validate(const pcg_policy_cfg* cfg);
/* Copies the weights to the current device (synchronous, a few KB).  A policy belongs to that device. */
PCG_API int pcg_policy_create(pcg_policy** out, const pcg_policy_cfg* cfg);
PCG_API int pcg_policy_destroy(pcg_policy* policy);
/* Re-uploads weights of IDENTICAL shape into the policy's existing device block (ABI 16): a training loop changes the
 * weights every iteration and must not allocate and free device memory each time.  Synchronous, like pcg_policy_create;
 * the caller orders it after the launches that still read the old weights (a rollout on a non-blocking stream has to be
 * synchronised first).  activation, out_map and the clip box may change with the weights.  PCG_E_DIM when n_in, n_out,
 * n_hidden or a width differ from the policy's; the statuses of pcg_policy_validate() for the cfg itself.  On any error
 * the policy is unchanged. */
PCG_API int pcg_policy_update(pcg_policy* policy, const pcg_policy_cfg* cfg);

/* The same policy evaluated in FLOAT32 inside the kernel (additive under ABI 16): stable-baselines3's MlpPolicy is a float32
 * module, and policy.predict(obs) in the reference is a float32 forward pass.  Takes pcg_policy_create()'s cfg; weights,
 * biases, out_low and out_high are rounded to the nearest float32 on upload.  The statuses of pcg_policy_validate(), plus
 * PCG_E_VALUE for a value that is not finite after rounding.  pcg_policy_update() keeps a policy's dtype (and rounds alike).
 * The arithmetic (csrc/pcg_rollout_policy_f32.hpp): in32[i] = (float)obs[i]; per unit one IEEE float32 FMA per input,
 * ascending, from the bias; tanhf / ReLU; the last layer's output widened to double exactly.  pcg_rollout_policy:
 * PCG_POL_NONE / PCG_POL_CLIP act on the widened value with the rounded box, PCG_POL_TANH is tanhf before the widening --
 * every recorded output is a float32 value.  pcg_rollout_actor: mu and value are the widened outputs; u, a, logp are formed
 * in fp64 exactly as for a float64 policy.  The env arithmetic is fp64 whatever the policy's dtype.
 * Both entry points keep their signatures and dispatch on the policy's dtype.  What a float32 policy adds to their
 * statuses, after every other check and with nothing compiled or launched: PCG_E_UNSUPPORTED on a plan with run-time
 * compiled code (PCG_MODEL_USER, user_reward_src: the plan's closed-loop module carries the float64 kernels only -- step
 * such a plan instead), and PCG_E_UNSUPPORTED for an actor and a critic of different dtypes. */
#define PCG_POL_F64 0
#define PCG_POL_F32 1
PCG_API int pcg_policy_create_f32(pcg_policy** out, const pcg_policy_cfg* cfg);
/* PCG_POL_F64 | PCG_POL_F32; PCG_E_NULL / PCG_E_PLAN for what is not a policy. */
PCG_API int pcg_policy_dtype(const pcg_policy* policy);

/* T env steps in ONE launch with the state in registers and the policy evaluated in the kernel between two steps:
 *   - the action of step s is policy(observation the env emitted before step s); for s = 0 that is io->obs as
 *     pcg_reset or the previous call left it.  The observation is exactly what pcg_step would have written (normalised
 *     if the plan normalises, with noise if the plan has noise: Philox keyed (seed, env, t) as everywhere);
 *   - the policy output is what the caller would have put into io->a (policy space, before the action map);
 *     a_seq_out[s] records it; with record_next_action, row T holds policy(observation after the last step), which is
 *     not applied (the last column of `u` in the reference's rollout, policy_evaluation.py:123-127) -- a_seq_out then
 *     has T + 1 rows;
 *   - a_seq_out, obs_seq, rew_seq may each be NULL; layout, strides and 16-byte rules as in pcg_rollout_strided;
 *     io->x / obs / rew / done receive the last step, as in pcg_rollout.  io->a is not read.
 * Lock-stepped plans only (io->t == NULL: PCG_E_UNSUPPORTED otherwise).  PCG_E_DIM when the policy's n_in / n_out are not
 * the plan's Nobs / na.  PCG_E_UNSUPPORTED, before anything is launched: plans with constraint rows (user_cons_src
 * included), per-env parameters, any integrator other than PCG_INT_RK4 / PCG_INT_CV8.
 * A built-in plan's call reads the plan and the policy and writes neither: no lazy allocation, no memset -- safe under
 * stream capture and from several streams at once (on distinct buffers).
 * Plans with run-time compiled code (PCG_MODEL_USER, user_reward_src) run the same kernels from a second run-time compiled
 * module of their own, which pcg_plan_create() does NOT build: the first closed-loop call of the plan (either entry point,
 * after every argument check) or pcg_plan_prepare_closed_loop() builds or loads it -- hipRTC the first time, the caches of
 * the step module afterwards; PCG_E_JIT, with pcg_last_jit_log(), if it does not compile.  Loading a module is not a
 * capturable operation: while `stream` is being captured and the module does not exist yet the call returns
 * PCG_E_UNSUPPORTED and launches nothing -- call pcg_plan_prepare_closed_loop(), or make one eager call, before capturing.
 * Once the module exists the call is as capture-safe as a built-in plan's. */
PCG_API int pcg_rollout_policy(pcg_plan* plan, const pcg_buffers* io, const pcg_policy* policy, int32_t t0, int32_t T,
                               double* a_seq_out, int64_t a_step_stride, int64_t a_comp_stride, double* obs_seq,
                               int64_t obs_step_stride, int64_t obs_comp_stride, double* rew_seq,
                               int64_t rew_step_stride, int32_t record_next_action, uint64_t seed, void* stream);

/* Builds or loads the closed-loop module of a plan with run-time compiled code (see pcg_rollout_policy), on the plan's
 * device, synchronously; idempotent.  PCG_OK and nothing done for a built-in plan, whatever its configuration;
 * PCG_E_UNSUPPORTED for a run-time compiled plan neither closed-loop entry point takes (constraint rows, an integrator
 * other than PCG_INT_RK4 / PCG_INT_CV8); PCG_E_JIT as at pcg_plan_create().  Not inside a stream capture. */
PCG_API int pcg_plan_prepare_closed_loop(pcg_plan* plan);

/* Closed-loop fused rollout with a STOCHASTIC actor-critic (ABI 16): what an on-policy trainer (PPO) collects, in one
 * launch.  The form is stable-baselines3's MlpPolicy: a Gaussian actor with a state-independent standard deviation and a
 * separate value network.  pcg_rollout_policy's loop, with this on the observation before step s (shared counter
 * t = t0 + s):
 *     mu   = actor's last-layer output BEFORE its output map
 *     z_i  = standard normal, Philox keyed (seed, global env index, t, PCG_RNG_POLICY + i / 2): the engine's RNG contract,
 *            so a sharded run (pcg_plan_set_env_offset) draws what the unsharded run draws
 *     u_i  = fma(sigma_i, z_i, mu_i)                            the sample (what PPO's buffer keeps)
 *     a    = out_map(u)                                         the action the env applies (PCG_POL_NONE | PCG_POL_CLIP)
 *     logp = fma(-0.5, q, c0); q = 0, for i ascending: q = fma(z_i, z_i, q)
 *            = log N(u; mu, sigma^2) of the UNMAPPED sample u (stable-baselines3 PPO's meaning: the env clips, the
 *            buffer keeps u), c0 = pcg_actor_logp_const(sigma, na)
 *     value = critic(observation): a second pcg_policy with n_out == 1 and PCG_POL_NONE, or NULL (value_out is then
 *            not written)
 * sigma: HOST array [na], finite and > 0; it and c0 travel by value with the launch (no device allocation, no copy).
 * Recorded rows, each optional (NULL) and strided like a_seq_out of pcg_rollout_policy: a_seq_out [T(+1)][na][B] applied
 * actions, u_seq_out [T(+1)][na][B] samples, logp_out [T(+1)][B], value_out [T(+1)][B].  With record_next_action, row T
 * holds all four for the observation after the last step, drawn at counter t0 + T and not applied; its value entry is the
 * bootstrap value.  obs_seq / rew_seq / io as in pcg_rollout_policy.
 * Statuses, in this order, nothing launched on any of them: those of pcg_rollout_policy for the plan and the actor
 * (PCG_E_UNSUPPORTED plans, PCG_E_DIM actor sizes); critic: PCG_E_PLAN (not a policy / another device), PCG_E_DIM
 * (n_in != Nobs or n_out != 1), PCG_E_VALUE (an output map); PCG_E_UNSUPPORTED for an actor with PCG_POL_TANH (a squashed
 * Gaussian needs the map's Jacobian in logp); PCG_E_NULL sigma == NULL; PCG_E_VALUE a sigma that is not finite and
 * positive; then T / t0 / buffers / strides as in pcg_rollout_policy.
 * Reads the plan and the policies and writes neither: safe under stream capture (a plan with run-time compiled code: once
 * its closed-loop module exists, as for pcg_rollout_policy). */
#define PCG_RNG_POLICY 0x400
PCG_API int pcg_rollout_actor(pcg_plan* plan, const pcg_buffers* io, const pcg_policy* actor, const pcg_policy* critic,
                              const double* sigma, int32_t t0, int32_t T, double* a_seq_out, int64_t a_step_stride,
                              int64_t a_comp_stride, double* u_seq_out, int64_t u_step_stride, int64_t u_comp_stride,
                              double* logp_out, int64_t logp_step_stride, double* value_out, int64_t value_step_stride,
                              double* obs_seq, int64_t obs_step_stride, int64_t obs_comp_stride, double* rew_seq,
                              int64_t rew_step_stride, int32_t record_next_action, uint64_t seed, void* stream);
/* The two closed-loop calls on plans WITH constraint rows, recording the rows (additive under ABI 16; kernels:
 * csrc/pcg_rollout_cons.hpp).  Every argument of pcg_rollout_policy / pcg_rollout_actor up to record_next_action keeps its
 * meaning, the loop, the networks' arithmetic and the Philox keys are theirs.  Added per step s (counter t0 + s):
 *   - g_seq[s * g_step_stride + r * g_comp_stride + e] receives row r of the ncon affine rows g = A.[x|SP|d|u] - b after
 *     the step; viol_seq[s * viol_step_stride + e] the byte "any row > 0".  Either may be NULL.  Step-major
 *     ([T][ncon][B]-like) or component-major ([ncon][T][B]-like, the reference's cons_info order) rows, as obs_seq;
 *   - after the last step io->g and io->viol (where given) hold that step's rows and flag and io->done its done flag,
 *     PCG_F_DONE_ON_CONS included: what pcg_step leaves.  At counter 0 the pre-step check (pcgym.py:414-420) writes
 *     io->g_pre (where given) and enters `done`; a call with t0 > 0 leaves io->g_pre alone;
 *   - the flag feeds the -1000 penalty (r_penalty), the box excess of the declarative tracking reward and `done`.
 * After `done`: an env whose done flag is set mid-episode (done_on_cons_vio) KEEPS STEPPING, exactly as a loop over pcg_step
 * on a lock-stepped batch does, which never resets single envs; mask what follows a violation from viol_seq.
 * Summation order.  g > 0 decides the penalty and `done`, so a row's last bit matters.  The rows are the bits pcg_step
 * leaves in io->g on the same plan and buffers: where pcg_step takes the feature-masked kernel (PCG_INT_RK4 plans of the
 * small models on an even, 16-byte-aligned batch) g = -b, + the SP slots, + the disturbance slots, + the states ascending,
 * + the actions, + the model disturbance inputs; everywhere else the states come first, then SP slots, disturbance slots,
 * actions, model disturbance inputs.  One fused multiply-add per term.
 * Plans: those of pcg_rollout_policy with ncon > 0 and affine rows -- lock-stepped, no per-env parameters, PCG_INT_RK4 /
 * PCG_INT_CV8, built-in.  PCG_E_UNSUPPORTED, before anything is launched: ncon == 0 (use pcg_rollout_policy /
 * pcg_rollout_actor), a plan with run-time compiled code (PCG_MODEL_USER, user_reward_src, user_cons_src: its closed-loop
 * module carries the two unconstrained kernels only), io->t != NULL, nunc > 0, any other integrator, a float32 policy,
 * actor or critic.  Every other status as in pcg_rollout_policy / pcg_rollout_actor and in their order (policy handle,
 * sizes, critic, sigma, T / t0, NULL buffers, strides); PCG_E_DIM besides for g_comp_stride < B, viol_step_stride < B with
 * T > 1, and g_seq rows that are neither step-major nor component-major (pcg_rollout_strided's rule for the observation
 * rows with ncon in place of Nobs).
 * Reads the plan and the policies and writes neither; no allocation, no memset: safe under stream capture.
 * Not here: constraint expressions and user models, float32 networks, per-env parameters, adaptive integrators; the
 * open-loop pcg_rollout / pcg_rollout_strided still keep only the last step's rows. */
PCG_API int pcg_rollout_policy_cons(pcg_plan* plan, const pcg_buffers* io, const pcg_policy* policy, int32_t t0, int32_t T,
                                    double* a_seq_out, int64_t a_step_stride, int64_t a_comp_stride, double* obs_seq,
                                    int64_t obs_step_stride, int64_t obs_comp_stride, double* rew_seq,
                                    int64_t rew_step_stride, int32_t record_next_action, double* g_seq,
                                    int64_t g_step_stride, int64_t g_comp_stride, uint8_t* viol_seq,
                                    int64_t viol_step_stride, uint64_t seed, void* stream);
PCG_API int pcg_rollout_actor_cons(pcg_plan* plan, const pcg_buffers* io, const pcg_policy* actor, const pcg_policy* critic,
                                   const double* sigma, int32_t t0, int32_t T, double* a_seq_out, int64_t a_step_stride,
                                   int64_t a_comp_stride, double* u_seq_out, int64_t u_step_stride, int64_t u_comp_stride,
                                   double* logp_out, int64_t logp_step_stride, double* value_out,
                                   int64_t value_step_stride, double* obs_seq, int64_t obs_step_stride,
                                   int64_t obs_comp_stride, double* rew_seq, int64_t rew_step_stride,
                                   int32_t record_next_action, double* g_seq, int64_t g_step_stride, int64_t g_comp_stride,
                                   uint8_t* viol_seq, int64_t viol_step_stride, uint64_t seed, void* stream);
/* The two closed-loop calls on plans WITH per-env parameters (additive under ABI 16; kernels: csrc/pcg_rollout_unc.hpp):
 * parametric uncertainty sampled at reset (nunc > 0), the reference's domain randomisation.  Argument lists, recorded
 * rows, loop, networks' arithmetic and Philox keys are those of pcg_rollout_policy / pcg_rollout_actor; nothing new is
 * recorded.  Two things differ:
 *   - the observation carries nunc more slots, [x | SP | d | unc]: the networks read them (n_in == Nobs of the plan, the
 *     parameter slots included), and the rows of obs_seq and the final io->obs carry them, as pcg_step writes them;
 *   - io->p_unc [nunc][B] is read and never written: it is whatever the preceding pcg_reset wrote (pcgym.py:300-316), or
 *     what the caller placed there.  The lane's folded model constants are rebuilt from it every step, as pcg_step does:
 *     rebuilding them ONCE per call was built and measured too, is slower as soon as the network has a hidden layer, and
 *     is not kept.  A call of T steps and T calls of one step return the same bits.
 * Against a loop over pcg_step the states agree to rounding, not to the bit: the two kernels are compiled separately and
 * the compiler contracts the model's right-hand side in each on its own (as pcg_rollout and pcg_step differ on such plans).
 * Plans: built-in models, PCG_INT_RK4, lock-stepped, no constraint rows, fp64 networks.  PCG_E_UNSUPPORTED, before anything
 * is launched: nunc == 0 (use pcg_rollout_policy / pcg_rollout_actor), ncon > 0, io->t != NULL, any other integrator
 * (PCG_INT_CV8 refuses per-env parameters at plan creation), a plan with run-time compiled code, a float32 policy, actor or
 * critic, a model without per-env parameter kernels (the affine registry models).  PCG_E_NULL for io->p_unc == NULL, among
 * the NULL buffers.  Every other status as in pcg_rollout_policy / pcg_rollout_actor and in their order (policy handle,
 * sizes, critic, sigma, T / t0, NULL buffers, strides).
 * Reads the plan, the policies and io->p_unc and writes none of them; no allocation, no memset: safe under stream capture.
 * Not here: float32 networks, per-env parameters together with constraint rows, PCG_INT_CV8 and the adaptive integrators,
 * run-time compiled plans, per-env counters. */
PCG_API int pcg_rollout_policy_unc(pcg_plan* plan, const pcg_buffers* io, const pcg_policy* policy, int32_t t0, int32_t T,
                                   double* a_seq_out, int64_t a_step_stride, int64_t a_comp_stride, double* obs_seq,
                                   int64_t obs_step_stride, int64_t obs_comp_stride, double* rew_seq,
                                   int64_t rew_step_stride, int32_t record_next_action, uint64_t seed, void* stream);
PCG_API int pcg_rollout_actor_unc(pcg_plan* plan, const pcg_buffers* io, const pcg_policy* actor, const pcg_policy* critic,
                                  const double* sigma, int32_t t0, int32_t T, double* a_seq_out, int64_t a_step_stride,
                                  int64_t a_comp_stride, double* u_seq_out, int64_t u_step_stride, int64_t u_comp_stride,
                                  double* logp_out, int64_t logp_step_stride, double* value_out, int64_t value_step_stride,
                                  double* obs_seq, int64_t obs_step_stride, int64_t obs_comp_stride, double* rew_seq,
                                  int64_t rew_step_stride, int32_t record_next_action, uint64_t seed, void* stream);
/* Host only: c0 = -(sum_i log sigma_i + na/2 log 2 pi), summed in ascending order in fp64 -- the constant
 * pcg_rollout_actor passes to its kernel.  NaN for a NULL / non-positive / non-finite sigma or na outside 1..PCG_MAX_NA. */
PCG_API double pcg_actor_logp_const(const double* sigma, int32_t na);
/* z_out [na][B] (device): the standard normals pcg_rollout_actor draws at counter t under `seed` -- same keys, same bits --
 * for a caller that samples outside the fused call (one pcg_step per step).  na and the env offset are the plan's. */
PCG_API int pcg_policy_noise(pcg_plan* plan, int64_t B, int32_t t, uint64_t seed, double* z_out, void* stream);

/* Generalised advantage estimation (Schulman et al. 2016) over one recorded episode, all B envs in ONE launch (additive
 * under ABI 16; kernel: csrc/pcg_gae.hpp): what an on-policy trainer forms from the rows pcg_rollout_actor and
 * pcg_rollout_actor_cons record.  The interface is that of stable-baselines3's
 * RolloutBuffer.compute_returns_and_advantage: `term` is its episode-start mask seen from the step before
 * (next_non_terminal = !term[t]), bootstrap_last = 0 its `dones` of the last step, val[T] its `last_values`.
 *   rew [T][B], val [T+1][B] (val[T]: the value of the observation after the last step), term [T][B] bytes or NULL
 *   (non-zero: the episode ended WITH step t -- e.g. viol_seq of pcg_rollout_actor_cons), adv [T][B], ret [T][B] or NULL;
 *   element (t, e) of each array is at t * its step stride + e.  All device memory; outputs must not overlap inputs.
 * Per env, backwards in time, with gl = gamma * lam rounded once on the host:
 *     carry = 0
 *     for t = T-1 .. 0:
 *         cut   = (term && term[t] != 0) || (t == T-1 && !bootstrap_last)
 *         nxt   = cut ? 0.0 : val[t+1];   c = cut ? 0.0 : carry
 *         delta = (rew[t] + gamma * nxt) - val[t]        three operations, each rounded
 *         carry = delta + gl * c                          two operations, each rounded
 *         adv[t] = carry;   ret[t] = carry + val[t]
 * No operation is contracted into a fused multiply-add and the products with zero are carried out, so the result is a
 * fixed rounding sequence: the same bits for every batch size, stride, alignment and launch shape (two envs per lane with
 * 16-byte accesses where B is even and all rows are 16-byte aligned, one env per lane otherwise), and the bits of the
 * same sequence written in any IEEE-754 double arithmetic (NaN payloads aside).  A NaN or infinity stays in its own env.
 * Status, nothing launched on any of them, in this order: PCG_E_NULL for rew, val or adv == NULL; PCG_E_DIM for B < 1 or
 * T < 1; PCG_E_DIM for val_step_stride < B, and while T > 1 for any other step stride < B (term's and ret's only when
 * they are given); PCG_E_VALUE for a gamma or lam that is not finite.
 * There is no plan: the launch goes to `stream` on the caller's current device.  Reads and writes only its arguments; no
 * allocation, no memset: safe under stream capture.  Not here: float32 arrays, advantage normalisation, per-env counters. */
PCG_API int pcg_gae(int64_t B, int32_t T, const double* rew, int64_t rew_step_stride, const double* val, int64_t val_step_stride,
                    const uint8_t* term, int64_t term_step_stride, double gamma, double lam, int32_t bootstrap_last,
                    double* adv, int64_t adv_step_stride, double* ret, int64_t ret_step_stride, void* stream);

/* A POPULATION of policies rolled in one closed-loop launch (additive under ABI 16; kernel: csrc/pcg_rollout_pop.hpp): what
 * derivative-free policy search over network weights, the comparison of a set of checkpoints under the same disturbances
 * and noise (the reference's policy_eval with its `policies` dict) and hyper-parameter sweeps need -- many policies, each
 * on a slice of the batch.
 * pcg_policy_pop holds P policies of IDENTICAL shape: n_in, n_out, n_hidden, widths, activation, output map and clip box
 * are shared, members differ in weights and biases alone, and all are float64 or all float32.  `cfg` is
 * pcg_policy_create()'s with W[l] / b[l] pointing at P consecutive matrices / bias vectors (member-major: member m's layer l
 * starts at W[l] + m rows cols).
 * Storage: one device allocation of P member blocks at a fixed stride, each what pcg_policy_create() writes for one policy.
 * pcg_policy_pop_create: PCG_E_NULL for out / cfg == NULL, PCG_E_DIM for P < 1, then pcg_policy_validate()'s statuses for
 *   the shape and for every member's values -- all before the device is touched.  Copies to the current device
 *   (synchronous); a population belongs to that device.
 * pcg_policy_pop_update: rewrites members [first, first + count) from arrays holding `count` members, into the existing
 *   allocation (nothing is allocated or freed on the device); synchronous and ordered like pcg_policy_update().  The
 *   statuses of create for (cfg, count); PCG_E_DIM for a range outside the population or another shape; PCG_E_VALUE for
 *   another activation, output map or clip box.  On any error the population is unchanged.
 * pcg_policy_pop_size: P (PCG_E_NULL / PCG_E_PLAN for what is not a population).
 * pcg_policy_pop_create_f32: the float32 form -- every member block is what pcg_policy_create_f32() writes for one policy
 *   (the same header, then floats: every value rounded to nearest, the rows of two consecutive units interleaved, the clip box
 *   holding the rounded bounds), back to back at one byte stride that is a multiple of 8.  The statuses of
 *   pcg_policy_pop_create, then PCG_E_VALUE when any member holds a value that is not finite after rounding or a clip bound
 *   overflows: nothing is allocated.  pcg_rollout_policy_pop evaluates such members in float32 (pcg_rollout_policy's
 *   arithmetic for a pcg_policy_create_f32 policy); the env stays fp64.
 *   pcg_policy_pop_update on a float32 population rounds the same way, compares the clip box AFTER rounding and judges every
 *   member of the range before a byte is copied: a member that overflows gives PCG_E_VALUE and the blocks stay as they were.
 * pcg_policy_pop_dtype: PCG_POL_F64 | PCG_POL_F32 (PCG_E_NULL / PCG_E_PLAN for what is not a population). */
typedef struct pcg_policy_pop pcg_policy_pop;
PCG_API int pcg_policy_pop_create(pcg_policy_pop** out, const pcg_policy_cfg* cfg, int32_t P);
PCG_API int pcg_policy_pop_create_f32(pcg_policy_pop** out, const pcg_policy_cfg* cfg, int32_t P);
PCG_API int pcg_policy_pop_dtype(const pcg_policy_pop* pop);
PCG_API int pcg_policy_pop_update(pcg_policy_pop* pop, const pcg_policy_cfg* cfg, int32_t first, int32_t count);
PCG_API int pcg_policy_pop_destroy(pcg_policy_pop* pop);
PCG_API int pcg_policy_pop_size(const pcg_policy_pop* pop);

/* pcg_rollout_policy with one member of `pop` per slice of the batch: env e is driven by member
 *     m = (env_offset + e) / envs_per_policy          (env_offset: pcg_plan_set_env_offset -- the GLOBAL env index, so that
 *                                                      a sharded batch splits a population the way it splits the RNG)
 * and computes, for its env, exactly what pcg_rollout_policy computes with that member as its policy: the same loop, the
 * same policy arithmetic, the same rows in a_seq_out / obs_seq / rew_seq / io (each optional, strided as there).  The kernel is
 * picked by the population's dtype: a float32 population (pcg_policy_pop_create_f32) is refused exactly where a float64 one is.
 * ret_out [B] (device) or NULL: each env's discounted return of THIS call's steps, accumulated in a register,
 *     J = 0; disc = 1;   per step s = 0 .. T-1:   J = J + disc * rew_s;   disc = disc * gamma
 * every operation rounded on its own (no fused multiply-add): a fixed rounding sequence, the bits of the same loop in any
 * IEEE-754 double arithmetic.  A call at t0 > 0 returns the return of its own steps, discounted from its first.
 * Statuses, nothing launched or written on any of them, in this order: those of pcg_rollout_policy for plan, io and the
 * handle (PCG_E_PLAN for what is not a population of the plan's device); PCG_E_UNSUPPORTED for what pcg_rollout_policy
 * refuses (io->t, constraint rows, per-env parameters, integrators other than PCG_INT_RK4 / PCG_INT_CV8) and for a plan
 * with run-time compiled code (PCG_MODEL_USER, user_reward_src: its module does not carry this kernel -- nothing is
 * compiled); PCG_E_DIM for members whose n_in / n_out are not the plan's Nobs / na; PCG_E_VALUE unless envs_per_policy and
 * the plan's env offset are multiples of 64 (envs_per_policy >= 64, offset >= 0: a wave never spans two members);
 * PCG_E_DIM unless (env_offset + B - 1) / envs_per_policy < P (B need not be a multiple of envs_per_policy); PCG_E_VALUE
 * for a gamma that is not finite or outside [0, 1]; then T / t0 / buffers / strides as in pcg_rollout_policy.
 * Reads the plan and the population and writes neither: no lazy allocation, no memset -- safe under stream capture.
 * Not here: stochastic actors over a population; plans with per-env parameters take pcg_rollout_policy_pop_unc and plans
 * with constraint rows pcg_rollout_policy_pop_cons, both below (this call keeps refusing either plan). */
PCG_API int pcg_rollout_policy_pop(pcg_plan* plan, const pcg_buffers* io, const pcg_policy_pop* pop, int64_t envs_per_policy,
                                   int32_t t0, int32_t T, double* a_seq_out, int64_t a_step_stride, int64_t a_comp_stride,
                                   double* obs_seq, int64_t obs_step_stride, int64_t obs_comp_stride, double* rew_seq,
                                   int64_t rew_step_stride, int32_t record_next_action, double gamma, double* ret_out,
                                   uint64_t seed, void* stream);
/* pcg_rollout_policy_pop on plans WITH per-env parameters (additive under ABI 16; kernels: csrc/pcg_rollout_pop_unc.hpp): a
 * population searched or compared over a DISTRIBUTION of plants -- every env of a member's slice integrates with its own
 * model parameters, sampled at reset (nunc > 0, the reference's domain randomisation).  Argument list and meaning, member
 * selection (the global env index), the recurrence of ret_out and the choice of the kernel by the population's dtype are those
 * of pcg_rollout_policy_pop; what per-env parameters change is what pcg_rollout_policy_unc says: the observation carries nunc
 * more slots, [x | SP | d | unc], which the members read (n_in == Nobs of the plan, the parameter slots included) and the
 * rows of obs_seq and the final io->obs carry, and io->p_unc [nunc][B] is read and never written.  A float32 population is
 * evaluated in float32 on that wider input; the env, J and disc stay fp64.
 * Numerical contract: each env computes what pcg_rollout_policy_unc computes with its member as the policy TO ROUNDING, not
 * to the bit -- the two kernels are compiled separately and the compiler contracts the model's right-hand side in each on its
 * own, as said of stepping above.  Against itself the call is bit for bit reproducible: the same bits for the same inputs;
 * a call of T steps and chunked calls over the same steps return the same rows (ret_out: the stated recurrence over each
 * chunk's rewards); a member's slice does not depend on the other members; shards reproduce the whole batch.
 * Statuses, nothing launched or written on any of them, in this order:
 *   1. plan, io and the handle as in pcg_rollout_policy_pop (PCG_E_PLAN for what is not a population of the plan's device);
 *   2. PCG_E_UNSUPPORTED as in pcg_rollout_policy_unc: nunc == 0 (use pcg_rollout_policy_pop), ncon > 0, a plan with
 *      run-time compiled code, io->t != NULL, an integrator other than PCG_INT_RK4, a model without the kernel (the affine
 *      registry models);
 *   3. PCG_E_DIM for members whose n_in / n_out are not the plan's Nobs / na (Nobs counts the parameter slots);
 *   4. the slices and gamma exactly as in pcg_rollout_policy_pop: PCG_E_VALUE unless envs_per_policy and the env offset are
 *      multiples of 64, PCG_E_DIM unless there is a member for every env, PCG_E_VALUE for a gamma outside [0, 1];
 *   5. T / t0, NULL buffers -- io->p_unc == NULL among them, PCG_E_NULL exactly where pcg_rollout_policy_unc gives it -- and
 *      strides.
 * pcg_rollout_policy_pop keeps refusing plans with per-env parameters.
 * Reads the plan, the population and io->p_unc and writes none of them; no allocation, no memset: safe under stream capture.
 * Not here: plans with constraint rows, stochastic actors over a population, paired parameter draws across members,
 * PCG_INT_CV8 and the adaptive integrators. */
PCG_API int pcg_rollout_policy_pop_unc(pcg_plan* plan, const pcg_buffers* io, const pcg_policy_pop* pop, int64_t envs_per_policy,
                                       int32_t t0, int32_t T, double* a_seq_out, int64_t a_step_stride, int64_t a_comp_stride,
                                       double* obs_seq, int64_t obs_step_stride, int64_t obs_comp_stride, double* rew_seq,
                                       int64_t rew_step_stride, int32_t record_next_action, double gamma, double* ret_out,
                                       uint64_t seed, void* stream);
/* pcg_rollout_policy_pop on plans WITH constraint rows (additive under ABI 16; kernels: csrc/pcg_rollout_pop_cons.hpp): the
 * evaluation step of a CONSTRAINED derivative-free search -- "return minus lambda x violations", "reject members that ever
 * violate" -- in one launch.  Member selection (the global env index), the recurrence of ret_out, the choice of the kernel by
 * the population's dtype and every argument up to record_next_action are those of pcg_rollout_policy_pop; g_seq / viol_seq
 * and their strides are those of pcg_rollout_policy_cons (rows [T][ncon][B]-like, step-major or component-major, flag bytes
 * [T][B]-like), and so is what the call leaves in io: io->g / io->viol / io->done / io->obs / io->rew hold the last step,
 * io->g_pre the pre-step check of a call that starts at counter 0 (written by no other call), and an env whose done flag is
 * set mid-episode keeps stepping.  Two statistics are accumulated per env in registers beside the return, over THIS call's
 * steps:
 *     nviol_out [B] int32 (device) or NULL: the number of steps whose post-step flag "any row > 0" was set;
 *     gmax_out  [B] (device) or NULL: the largest post-step row value over the steps and rows, from -inf with
 *         gmax = (g > gmax) ? g : gmax          that statement defines the bits; a NaN row leaves gmax unchanged.
 * The pre-step check at counter 0 counts in neither.  Every output may be NULL; the rows are summed regardless (the flag
 * feeds the penalty, the box excess and `done`).
 * Numerical contract: each env computes what pcg_rollout_policy_cons computes with its member as the policy, bit for bit --
 * recorded actions, observations, rewards, rows, flags and the final io buffers (a float32 population: the member's float32
 * network, which pcg_rollout_policy_cons itself does not take; its rows are the bits of stepping the recorded actions).  The
 * rows are summed in the order pcg_step would use on the same buffers, as there.  nviol_out is the column sum of viol_seq,
 * gmax_out the maximum of g_seq, ret_out the stated recurrence over rew_seq, whether or not those are recorded; chunked calls
 * return the statistics of their own steps.
 * Statuses, nothing launched or written on any of them, in this order:
 *   1. plan, io and the handle as in pcg_rollout_policy_pop (PCG_E_PLAN for what is not a population of the plan's device);
 *   2. PCG_E_UNSUPPORTED for ncon == 0 (use pcg_rollout_policy_pop);
 *   3. PCG_E_UNSUPPORTED for nunc > 0, io->t != NULL, an integrator other than PCG_INT_RK4 / PCG_INT_CV8;
 *   4. PCG_E_UNSUPPORTED for a plan with run-time compiled code (PCG_MODEL_USER, user_reward_src, a constraint expression:
 *      no module carries these kernels -- nothing is compiled);
 *   5. PCG_E_DIM for members whose n_in / n_out are not the plan's Nobs / na;
 *   6. the slices and gamma exactly as in pcg_rollout_policy_pop: PCG_E_VALUE unless envs_per_policy and the env offset are
 *      multiples of 64, PCG_E_DIM unless there is a member for every env, PCG_E_VALUE for a gamma outside [0, 1];
 *   7. T / t0, NULL buffers and strides as in pcg_rollout_policy_cons (PCG_E_DIM for g_comp_stride < B, for
 *      viol_step_stride < B while T > 1, for rows of g_seq that overlap).
 * pcg_rollout_policy_pop keeps refusing plans with constraint rows.
 * Reads the plan and the population and writes neither; no allocation, no memset: safe under stream capture.
 * Not here: constraint expressions and user models, rows together with per-env parameters, stochastic actors over a
 * population, cutting the return at the first violation (mask from viol_seq, or penalise through nviol_out). */
PCG_API int pcg_rollout_policy_pop_cons(pcg_plan* plan, const pcg_buffers* io, const pcg_policy_pop* pop, int64_t envs_per_policy,
                                        int32_t t0, int32_t T, double* a_seq_out, int64_t a_step_stride, int64_t a_comp_stride,
                                        double* obs_seq, int64_t obs_step_stride, int64_t obs_comp_stride, double* rew_seq,
                                        int64_t rew_step_stride, int32_t record_next_action, double* g_seq, int64_t g_step_stride,
                                        int64_t g_comp_stride, uint8_t* viol_seq, int64_t viol_step_stride, double gamma,
                                        double* ret_out, int32_t* nviol_out, double* gmax_out, uint64_t seed, void* stream);

/* The weights of a population written and read ON the device (additive under ABI 16; kernels: csrc/pcg_pop_search.hpp):
 * what surrounds pcg_rollout_policy_pop in a derivative-free search loop -- sampling the members of a diagonal Gaussian,
 * the score-weighted noise sum of an evolution strategy, and flat parameter vectors in and out of the packed blocks --
 * with no weight crossing to the host.
 *
 * Flat parameter order.  Parameter j of a member, 0 <= j < n, runs layer by layer: W[l] row-major (n_next x n_prev)
 * followed by b[l]; n = sum_l rows_l (cols_l + 1) = pcg_policy_pop_nparams().  No entry point below writes a member's
 * header or padding.
 *
 * Search noise (the engine's RNG contract, purpose PCG_RNG_SEARCH; no existing stream uses that word).  For member m (the
 * population's own index: global across shards), parameter j, `generation` g and `seed`:
 *     q = antithetic ? m >> 1 : m
 *     o = philox4x32_10(ctr = (q, j >> 2, g, PCG_RNG_SEARCH), key = (seed_lo, seed_hi))
 *     (z0, z1) = box_muller_f32(o[0], o[1]) -> parameters 4b, 4b + 1       (b = j >> 2)
 *     (z2, z3) = box_muller_f32(o[2], o[3]) -> parameters 4b + 2, 4b + 3
 *     z(m, j)  = (double) of that float, negated (exactly) when antithetic and m is odd
 * Variates past n in the last block are discarded.
 *
 * pcg_policy_pop_sample: members [first, first + count): theta(m, j) = mean[j] + std[j] * z(m, j), product and sum each
 *   rounded on their own (no fused multiply-add), written into the packed blocks in place.  Other members are not touched.
 *   mean, std: device arrays [n].
 * pcg_policy_pop_noise_dot: out[j] = sum over m in [first, first + count) of w[m - first] * z(m, j), in a FIXED order:
 *   chunks of PCG_POP_CHUNK consecutive members counted from `first`; within a chunk acc = 0.0, then acc = acc + (w * z) for
 *   ascending m (two roundings each); partial[c][j] = acc; out[j] = 0.0 + partial[0][j] + partial[1][j] + ... ascending.
 *   w: device [count]; partial: caller-provided device workspace of ceil(count / PCG_POP_CHUNK) * n doubles; out: device
 *   [n].  Two launches, no atomics: the same bits for every launch shape.  The noise is formed again from the keys, never
 *   stored.  The blocks are not read: on a float32 population a member's realised perturbation is
 *   round32(mean + std z) - mean, not std z, while the sum uses the unrounded z -- an evolution strategy's ordinary noise.
 * pcg_policy_pop_get_flat: theta[i * theta_member_stride + j] = parameter j of member (members ? members[i] : first + i),
 *   i < count.  members: device array [count] or NULL, repeats allowed (`first` is not read when it is given); an index
 *   outside [0, P) writes NaN into that row and nothing else -- no fault, no host read.
 * pcg_policy_pop_set_flat: the inverse for the range [first, first + count): the device-to-device form of
 *   pcg_policy_pop_update().
 *
 * Statuses, decided before anything is launched, in this order: PCG_E_NULL for a NULL pop or a NULL required pointer
 * (mean, std; w, partial, out; theta); PCG_E_PLAN for what is not a population, or a population of a device other than the
 * caller's current one; PCG_E_DIM for count < 1, first < 0, first + count > P (with `members`: count < 1 alone), or a member
 * stride < n; PCG_E_VALUE for antithetic not 0 or 1.
 * The CONTENTS of device arrays are not inspected (that would be a host read): a non-finite mean, std or theta gives
 * non-finite weights in exactly those members, where pcg_policy_pop_update() would have refused them.  What
 * pcg_rollout_policy_pop then does with such a member: its outputs are NaN (PCG_POL_CLIP keeps a NaN), so the envs it drives
 * go non-finite -- their states, observations, rewards and ret_out entries are NaN and io->status, where given, reports
 * PCG_ST_NONFINITE.  The envs of every other member are computed as ever; nothing faults.
 * A float32 population (pcg_policy_pop_create_f32) takes the same five calls with the same signatures, fp64 mean / std / theta
 * / w, flat order and keys; only where a parameter lives and how it is stored change.  Parameter (l, r, k) sits at float offset
 * HDR + offW[l] + ((r / 2) ld[l] + k) 2 + (r & 1) of its block and bias (l, r) at HDR + offb[l] + r, HDR the header's size in
 * floats.  _sample forms mean[j] + std[j] * z in fp64 exactly as above and stores it with ONE round-to-nearest conversion: a
 * float32 member is bit for bit (float) of what a float64 population holds under the same seed, generation and antithetic
 * flag.  A value that overflows float32 is stored as +-inf and not inspected: such a member behaves as a non-finite one above.
 * _set_flat stores (float)theta, rounded to nearest; _get_flat returns the stored float widened exactly (NaN rows as above).
 * No allocation, no memset, no synchronisation in any of the five: the launches go to `stream` and are safe under stream
 * capture.  Not here: full-covariance sampling, a device-side generation counter. */
#define PCG_RNG_SEARCH 0x500
#define PCG_POP_CHUNK 64
PCG_API int pcg_policy_pop_nparams(const pcg_policy_pop* pop);
PCG_API int pcg_policy_pop_sample(pcg_policy_pop* pop, int32_t first, int32_t count, const double* mean, const double* std,
                                  int32_t antithetic, uint64_t seed, uint32_t generation, void* stream);
PCG_API int pcg_policy_pop_noise_dot(const pcg_policy_pop* pop, int32_t first, int32_t count, int32_t antithetic, uint64_t seed,
                                     uint32_t generation, const double* w, double* partial, double* out, void* stream);
PCG_API int pcg_policy_pop_get_flat(const pcg_policy_pop* pop, const int32_t* members, int32_t first, int32_t count,
                                    double* theta, int64_t theta_member_stride, void* stream);
PCG_API int pcg_policy_pop_set_flat(pcg_policy_pop* pop, int32_t first, int32_t count, const double* theta,
                                    int64_t theta_member_stride, void* stream);

/* pcg_step followed, in the same launch, by the reset of every env that finished in it (gymnasium "same-step"
 * auto-reset: rew / done / viol are those of the finished step; x, obs, t, a_save and the per-env parameters are
 * those of the new episode, drawn with `reset_seed`).  Equivalent to pcg_step + pcg_reset(mask = io->done,
 * seed = reset_seed) -- the reference has no counterpart (its callers loop "if done: env.reset()",
 * policy_evaluation.py:86-128) -- but one launch instead of two.  With per-env step counters (io->t) `t` is
 * ignored; for a lock-stepped batch `t` is the shared counter and the caller restarts it at 0 after the call
 * that returns done (t == N-2, or a constraint violation with PCG_F_DONE_ON_CONS ends single envs early). */
PCG_API int pcg_step_autoreset(pcg_plan* plan, const pcg_buffers* io, int32_t t, uint64_t seed, uint64_t reset_seed,
                               void* stream);

/* Step graph: T consecutive pcg_step launches (t = t0 .. t0+T-1, optionally preceded by a full pcg_reset)
 * recorded once as a HIP graph and replayed with ONE host call.  This is the on-device form of the
 * reference's per-episode Python loop "for i in range(N-1): env.step(a_i)" (policy_evaluation.py:86-128)
 * for callers that still want every step's obs/rew in the plan's buffers between launches: same results,
 * same buffers, no launch-to-launch gap (measured 15.0 -> 13.6 us per step on the 2^20-env cstr workload).
 * INVARIANT: after every recorded LAUNCH every buffer holds the bytes the pcg_step loop leaves at that point.
 * A launch is one step, except that a run of two or more consecutive steps that would each take the lean pipelined RK4
 * kernel (lock-stepped plans of the small models with none of the extras, no d_steps, B < 2^28, no forced
 * PCG_OPT_VARIANT / PCG_OPT_STREAM_BLOCKS_PER_CU) is recorded as ONE chained launch: every tile of envs keeps its state in
 * registers from the run's first step to its last, and no step waits for the whole batch to finish the one before it.
 * Every step of the run still stores its observation, reward and done bytes, in step order, so after the launch obs / rew
 * / done are the last step's and x is the final state; the states between the run's steps are never in memory (nothing
 * can read the buffers inside a replay).  The sticky status byte is written once per chained launch (a non-finite state
 * stays non-finite).  Two envs per lane only if every a_steps[j] of the run is 16-byte aligned.  The graph owns a small
 * device table of the run's action pointers, allocated before the recording and freed by pcg_graph_destroy.
 * PCG_NO_CHAIN set in the environment when the plan was created: every step is a launch of its own.
 * a_steps [T] device pointers, each [na][B] (entries may repeat); d_steps NULL or [T] pointers, each [nd][B].
 * t0, T, seed and all buffer addresses are baked into the graph; pcg_graph_set_seed() re-keys the RNG of an
 * instantiated graph (new episode, fresh noise) without re-recording.  io->t must be NULL (lock-stepped). */
typedef struct pcg_graph pcg_graph;
PCG_API int pcg_graph_create(pcg_graph** out, pcg_plan* plan, const pcg_buffers* io, const double* const* a_steps,
                             const double* const* d_steps, int32_t t0, int32_t T, uint64_t seed, int with_reset);
PCG_API int pcg_graph_launch(pcg_graph* graph, void* stream);
PCG_API int pcg_graph_set_seed(pcg_graph* graph, uint64_t seed);
PCG_API int pcg_graph_destroy(pcg_graph* graph);
/* Rows that carry nothing new are stored once: a recorded step of the lean pipelined kernel (lock-stepped plans with none
 * of the extras, RK4 / CV8) that directly follows another one skips the observation's set-point / disturbance slot rows
 * when the schedules give both steps bitwise the same values, and the done bytes when both steps set the same flag.  The
 * first recorded step stores everything, so a replay never depends on what the buffers held before it, and after every
 * launch every buffer holds exactly the bytes the pcg_step calls up to there would have left.  *slot_nodes / *done_nodes (either may be
 * NULL): how many recorded steps skip the slot rows / the done bytes; both 0 for graphs of any other kernel and with
 * PCG_NO_HELD_ROWS set in the environment when the plan was created. */
PCG_API int pcg_graph_held(const pcg_graph* graph, int32_t* slot_nodes, int32_t* done_nodes);
/* *launches / *steps (either may be NULL): how many chained launches the graph holds and how many of its recorded steps
 * they cover; both 0 where no run of two chainable steps exists and with PCG_NO_CHAIN.  pcg_graph_held counts a chained
 * step like any other recorded step, and pcg_graph_set_seed re-keys chained launches too. */
PCG_API int pcg_graph_chained(const pcg_graph* graph, int32_t* launches, int32_t* steps);

/* Compiler output of the most recent failed run-time compilation in this process (static storage, "" if none). */
PCG_API const char* pcg_last_jit_log(void);

/* Test hook: the work-queue kernel's tile sort on its own.  words: ntiles x S 32-bit words on the device (distinct
 * within a tile), sorted in place, DESCENDING, one workgroup of `threads` threads per tile.  (S, threads) as the step kernels
 * use them: S in {512, 1024, 2048}, threads in {256, 512}; anything else PCG_E_UNSUPPORTED.  The step results do not depend
 * on the order of a tile -- this is the only way to see that the sort sorts. */
PCG_API int pcg_test_sort_tile(uint32_t* words, int32_t S, int32_t threads, int64_t ntiles, void* stream);

/* Kernel-instantiation coverage (TEST HOOK; active only when PCG_COVERAGE is set in the environment at load time, otherwise
 * returns -1 and records nothing).  Every kernel launch of this library notes the instantiation it launches; this call
 * writes their MANGLED names, newline-separated and NUL-terminated, into buf (at most cap bytes; run-time compiled kernels
 * carry the prefix "jit:"), and returns the size the full list needs.  reset != 0 empties the record afterwards.
 * tests/conftest.py asks after every GPU test; tools/kernel_inventory.py lists what the library carries. (host) */
PCG_API int64_t pcg_coverage_names(char* buf, int64_t cap, int reset);

/* Raw Philox4x32-10 block for KAT tests: ctr[4], key[2] -> out[4]. (host) */
PCG_API void pcg_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* PCGYM_HIP_H */
