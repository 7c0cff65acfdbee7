// pcg_abi_policy.hip -- on-device MLP policies: the policy and population handles (packed by pcg_policy_pack.hpp), a
// population's weights written and read on the device (pcg_pop_search.hpp), the closed-loop fused rollouts with their per-step
// noise hook, and generalised advantage estimation (pcg_gae.hpp).
#include "pcg_host.hpp"
#include "pcg_gae.hpp"
#include "pcg_pop_search.hpp"

#include <algorithm>
#include <initializer_list>

namespace pcg {

// z [na][B] for one (seed, t): the bits rollout_actor_kernel (pcg_rollout_actor.hpp) draws at that counter, for the
// per-step route (pcg_policy_noise)
__global__ __launch_bounds__(BLOCK) void policy_noise_kernel(int64_t B, int32_t na, uint64_t seed, int64_t env_offset, uint32_t t, double* z) {
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= B) return;
#pragma unroll
  for (int i = 0; i < PCG_MAX_NA; i += 2) {
    if (i < na) {
      double z0, z1;
      rng_normal2(seed, (uint64_t)(env_offset + e), t, RNG_POLICY + (uint32_t)(i >> 1), z0, z1);
      z[(size_t)i * B + e] = z0;
      if (i + 1 < na) z[(size_t)(i + 1) * B + e] = z1;
    }
  }
}

static int policy_create(pcg_policy** out, const pcg_policy_cfg* cfg, int dtype) {
  if (!out) return PCG_E_NULL;
  *out = nullptr;
  PCG_TRY(policy_validate(cfg));
  int prc = PCG_OK;
  const std::vector<double> blob = pack_policy(cfg, dtype, &prc);
  PCG_TRY(prc);
  pcg_policy* q = new (std::nothrow) pcg_policy();
  if (!q) return (int)hipErrorOutOfMemory;
  q->dtype = dtype;
  q->shape = PolicyShape::from_cfg(cfg);
  q->out_map = cfg->out_map;
  q->blob_doubles = blob.size();
  hipError_t e = hipGetDevice(&q->device);
  if (e == hipSuccess) e = hipMalloc((void**)&q->dP, sizeof(double) * blob.size());
  if (e == hipSuccess) e = hipMemcpy(q->dP, blob.data(), sizeof(double) * blob.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (q->dP) (void)hipFree(q->dP);
    delete q;
    return (int)e;
  }
  q->magic = POLICY_MAGIC;
  *out = q;
  return PCG_OK;
}

static int pop_create(pcg_policy_pop** out, const pcg_policy_cfg* cfg, int32_t P, int dtype) {
  if (!out) return PCG_E_NULL;
  *out = nullptr;
  PCG_TRY(pop_validate(cfg, P));
  size_t member = 0;
  int prc = PCG_OK;
  const std::vector<double> all = pack_pop(cfg, P, dtype, &member, &prc);
  PCG_TRY(prc);  // (nothing is allocated)
  pcg_policy_pop* q = new (std::nothrow) pcg_policy_pop();
  if (!q) return (int)hipErrorOutOfMemory;
  q->blob_doubles = member;
  q->dtype = dtype;
  q->P = P;
  q->lay = pop_layout(cfg, all.data(), dtype);
  q->shape = PolicyShape::from_cfg(cfg);
  q->act = cfg->activation; q->out_map = cfg->out_map;
  // (the box update holds a new cfg against: a float32 population's is the rounded one, as in its members' headers)
  q->out_lo = dtype == PCG_POL_F32 ? (double)(float)cfg->out_low : cfg->out_low;
  q->out_hi = dtype == PCG_POL_F32 ? (double)(float)cfg->out_high : cfg->out_high;
  hipError_t e = hipGetDevice(&q->device);
  if (e == hipSuccess) e = hipMalloc((void**)&q->dP, sizeof(double) * all.size());
  if (e == hipSuccess) e = hipMemcpy(q->dP, all.data(), sizeof(double) * all.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (q->dP) (void)hipFree(q->dP);
    delete q;
    return (int)e;
  }
  q->magic = POP_MAGIC;
  *out = q;
  return PCG_OK;
}

// ---- the weights of a population written and read on the device (pcg_pop_search.hpp) -------------------------------------
// what all five decide first: a population, of the caller's current device
static int pop_search_open(const pcg_policy_pop* q) {
  if (!pop_ok(q)) return PCG_E_PLAN;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != q->device) return PCG_E_PLAN;
  return PCG_OK;
}
static bool pop_range_ok(const pcg_policy_pop* q, int32_t first, int32_t count) {
  return count >= 1 && first >= 0 && (int64_t)first + count <= q->P;
}
// elements between two members' blocks, in the unit the layout counts in (doubles, or floats for a float32 population)
static int64_t pop_stride(const pcg_policy_pop* q) {
  return (int64_t)q->blob_doubles * (q->dtype == PCG_POL_F32 ? 2 : 1);
}
// grid of the kernels that run blockIdx.x over `lanes` lanes of one row and stride blockIdx.y over `rows` rows
static dim3 pop_grid(int64_t lanes, int64_t rows) {
  return dim3((unsigned)((lanes + POP_BLOCK - 1) / POP_BLOCK), (unsigned)std::min<int64_t>(rows, POP_MAX_GRID_Y));
}

// All six closed-loop entry points (pcg_rollout_policy / pcg_rollout_actor, their _cons and _unc forms) validate through three
// functions, read top to bottom: closed_loop_open up to the policy's size, then the head's own (policy_head; actor_head: critic,
// tanh map, sigma), then closed_loop_launch from the step range on.
// the kind of plan an entry point is for: without constraint rows and per-env parameters, WITH rows (recorded per step), WITH parameters
enum class ClosedLoopKind { base, cons, unc };
struct ClosedLoopRun {  // what every entry point is given beside its networks: step range, the env's recorded sequences, seed
  int32_t t0, T;
  double* obs_seq;
  int64_t obs_ss, obs_cs;  // element strides (step, component)
  double* rew_seq;
  int64_t rew_ss;
  uint64_t seed;
};
struct SeqRec {  // a sequence the head records, with its component stride; null: not recorded
  const double* seq;
  int64_t comp_stride;
};
struct ConsRec {  // what ClosedLoopKind::cons adds: the rows [T][ncon][B]-like and flags [T][B]-like its entry points record
  double* g_seq;
  int64_t g_ss, g_cs;
  uint8_t* viol_seq;
  int64_t v_ss;
};

// whether a closed-loop kernel exists for this run-time compiled plan: the plans the built-in path takes
static bool jit_closed_loop_ok(const pcg_plan* p) {
  return p->hc.ncon <= 0 && p->hc.nunc <= 0 && lean_scheme(p->integrator_id) >= 0;
}

static hipFunction_t jit_head_fn(const pcg_plan* p, const PolicyArgs&) { return p->jit_pol; }
static hipFunction_t jit_head_fn(const pcg_plan* p, const ActorArgs&) { return p->jit_act; }
// (never asked for: pop_open refuses a plan with run-time compiled code, whose module does not carry the population kernels)
static hipFunction_t jit_head_fn(const pcg_plan*, const PopArgs&) { return nullptr; }

// Plan, buffers and policy handle; then which plans the kind's kernels carry and which kernel it is (`actor`: the head); then
// the policy's sizes.  *fn stays null for a plan with run-time compiled code, which has no ahead-of-time kernel:
// closed_loop_launch takes its own module's.
static int closed_loop_open(pcg_plan* p, const pcg_buffers* io, const pcg_policy* q, ClosedLoopKind kind, bool actor, StepArgs* a,
                            const void** fn) {
  PCG_TRY(fill_args(p, io, a));
  if (!q) return PCG_E_NULL;
  if (!policy_ok(q) || q->device != p->device) return PCG_E_PLAN;
  const DevConst& c = p->hc;
  const Kernels& k = kernels(p->kid);
  const int ls = lean_scheme(p->integrator_id);
  const bool jit = p->jit_fn[0] != nullptr, f32 = q->dtype == PCG_POL_F32;
  *fn = nullptr;
  switch (kind) {
    case ClosedLoopKind::base:
      // what the closed-loop kernels do not carry: per-env counters, constraint rows, per-env parameters, and every integrator
      // but the two fixed-step schemes
      if (io->t || c.ncon > 0 || c.nunc > 0 || ls < 0) return PCG_E_UNSUPPORTED;
      if (!jit)
        *fn = actor ? (const void*)(f32 ? k.roll_actor_f32 : k.roll_actor)[ls] : (const void*)(f32 ? k.roll_policy_f32 : k.roll_policy)[ls];
      break;
    case ClosedLoopKind::cons:
      // the plan's side turned round: rows are required, and what these kernels are not built for (a plan with run-time
      // compiled code, a float32 network) is refused here, before the sizes
      if (c.ncon <= 0 || jit || io->t || c.nunc > 0 || ls < 0 || f32) return PCG_E_UNSUPPORTED;
      *fn = actor ? (const void*)k.roll_actor_cons[ls] : (const void*)k.roll_policy_cons[ls];
      break;
    case ClosedLoopKind::unc:
      // likewise: parameters are required; no constraint rows, RK4 alone, and (the null entry) a model with kernels for them
      if (c.nunc <= 0 || c.ncon > 0 || jit || io->t || p->integrator_id != PCG_INT_RK4 || f32) return PCG_E_UNSUPPORTED;
      *fn = actor ? (const void*)k.roll_actor_unc : (const void*)k.roll_policy_unc;
      break;
  }
  if (!*fn && !jit) return PCG_E_UNSUPPORTED;
  if (q->shape.n_in != c.nobs || q->shape.n_out != c.na) return PCG_E_DIM;
  return PCG_OK;
}

// what the base kind, the one that takes float32 networks, refuses after every other check (closed_loop_launch): float32 on
// a plan with run-time compiled code, whose closed-loop module carries the fp64 kernels alone
static int f32_on_jit(const pcg_plan* p, const pcg_policy* q) {
  return q->dtype == PCG_POL_F32 && p->jit_fn[0] ? PCG_E_UNSUPPORTED : PCG_OK;
}

static PolicyArgs policy_head(const pcg_policy* q, double* a_out, int64_t ao_ss, int64_t ao_cs, int32_t record_next) {
  PolicyArgs pa;
  pa.P = (const PCG_CONSTANT PolicyDev*)q->dP;
  pa.a_out = a_out; pa.ao_ss = ao_ss; pa.ao_cs = ao_cs;
  pa.record_next = record_next ? 1 : 0;
  return pa;
}

// The actor's own checks, after closed_loop_open's, and its kernel argument: critic (handle; its dtype for `cons` / `unc`,
// whose kernels are built for fp64 networks; sizes; map), tanh-mapped actor, sigma.  *late: the base kind evaluates both
// networks in one kernel of one dtype -- an actor and a critic of two dtypes are refused, but after every other check.
static int actor_head(const pcg_plan* p, ClosedLoopKind kind, const pcg_policy* q, const pcg_policy* v, const double* sigma,
                      double* a_out, int64_t ao_ss, int64_t ao_cs, double* u_out, int64_t uo_ss, int64_t uo_cs, double* lp_out,
                      int64_t lp_ss, double* v_out, int64_t v_ss, int32_t record_next, ActorArgs* aa, int* late) {
  const DevConst& c = p->hc;
  if (v) {
    if (!policy_ok(v) || v->device != p->device) return PCG_E_PLAN;
    if (kind != ClosedLoopKind::base && v->dtype == PCG_POL_F32) return PCG_E_UNSUPPORTED;
    if (v->shape.n_in != c.nobs || v->shape.n_out != 1) return PCG_E_DIM;
    if (v->out_map != PCG_POL_NONE) return PCG_E_VALUE;
  }
  // a squashed Gaussian's density carries the map's Jacobian: not these calls
  if (q->out_map == PCG_POL_TANH) return PCG_E_UNSUPPORTED;
  if (!sigma) return PCG_E_NULL;
  for (int i = 0; i < c.na; ++i)
    if (!(std::isfinite(sigma[i]) && sigma[i] > 0.0)) return PCG_E_VALUE;
  std::memset(aa, 0, sizeof(*aa));
  aa->P = (const PCG_CONSTANT PolicyDev*)q->dP;
  aa->V = v ? (const PCG_CONSTANT PolicyDev*)v->dP : nullptr;
  aa->a_out = a_out; aa->ao_ss = ao_ss; aa->ao_cs = ao_cs;
  aa->u_out = u_out; aa->uo_ss = uo_ss; aa->uo_cs = uo_cs;
  aa->lp_out = lp_out; aa->lp_ss = lp_ss;
  aa->v_out = v ? v_out : nullptr; aa->v_ss = v_ss;
  for (int i = 0; i < c.na; ++i) aa->sigma[i] = sigma[i];
  aa->c0 = pcg_actor_logp_const(sigma, c.na);
  aa->record_next = record_next ? 1 : 0;
  *late = (v && v->dtype != q->dtype) ? PCG_E_UNSUPPORTED : f32_on_jit(p, q);
  return PCG_OK;
}

// whether pcg_step on these buffers would take the feature-masked kernel (step_impl's routes, for a lock-stepped built-in
// plan with rows and without per-env parameters: io->a is the caller's per-step action row, io->d is not given in a closed loop)
static bool feat_route_of_step(const pcg_plan* p, const pcg_buffers* io) {
  const Kernels& k = kernels(p->kid);
  pcg_buffers b = *io;
  b.a = nullptr; b.d = nullptr;
  return feat_pick(p, k, &b, 0, lds_stages_on(p, k), false) >= 0;
}

// `cons`: what ClosedLoopKind::cons adds (null for the other two) -- the launch then carries a ConsArgs as its third argument;
// `late_status`: what the heads found and the base kind refuses only after every other check (f32_on_jit, actor_head)
template <class HeadArgs>
static int closed_loop_launch(pcg_plan* p, const pcg_buffers* io, StepArgs& a, const void* fn, ClosedLoopKind kind, const ConsRec* cons,
                              const HeadArgs& head, std::initializer_list<SeqRec> head_recs, const ClosedLoopRun& r, int late_status,
                              void* stream) {
  const DevConst& c = p->hc;
  const bool unc = kind == ClosedLoopKind::unc;
  if (r.T < 1 || r.t0 < 0 || (int64_t)r.t0 + (int64_t)r.T > 0x7fffffffLL) return PCG_E_VALUE;
  if (io->B == 0) return PCG_OK;
  if (!io->x || !io->obs || !io->rew || !io->done) return PCG_E_NULL;
  if ((c.flags & PCG_F_A_DELTA) && !io->a_save) return PCG_E_NULL;
  if ((c.flags & PCG_F_REWARD_TRACK) && !io->u_prev) return PCG_E_NULL;
  if (unc && !io->p_unc) return PCG_E_NULL;  // (the entry points for plans with per-env parameters: what the reset wrote)
  if (r.obs_seq && r.obs_cs < io->B) return PCG_E_DIM;
  for (const SeqRec& h : head_recs)
    if (h.seq && h.comp_stride < io->B) return PCG_E_DIM;
  if (kind == ClosedLoopKind::cons) {
    // the rows a rollout WRITES must not overlap: flag rows a full batch apart, constraint rows either step-major or
    // component-major (the reference's axis order) -- pcg_rollout_strided's rule for the observation rows
    const int64_t B = io->B, n = c.ncon;
    if (cons->g_seq && cons->g_cs < B) return PCG_E_DIM;
    if (cons->viol_seq && r.T > 1 && cons->v_ss < B) return PCG_E_DIM;
    if (cons->g_seq) {
      const bool step_major = r.T == 1 || cons->g_ss >= (n - 1) * cons->g_cs + B;
      const bool comp_major = cons->g_ss >= B && (n == 1 || cons->g_cs >= (int64_t)(r.T - 1) * cons->g_ss + B);
      if (!step_major && !comp_major) return PCG_E_DIM;
    }
  }
  // what the float32 form adds, after every other check: networks of two dtypes in one call, float32 on a plan with run-time
  // compiled code -- nothing compiled, nothing launched
  if (late_status != PCG_OK) return late_status;
  a.t_scalar = r.t0; a.seed = r.seed; a.T = r.T;
  a.d = nullptr;  // (the shared schedule: a closed-loop rollout has no per-step explicit disturbance values)
  a.obs_seq = r.obs_seq; a.rew_seq = r.rew_seq;
  a.o_ss = r.obs_ss; a.o_cs = r.obs_cs; a.r_ss = r.rew_ss;
  HeadArgs h = head;
  ConsArgs g;
  void* argv[3] = {&a, &h, &g};  // (a kernel reads as many as it takes: the third is the constrained kernels' alone)
  if (p->jit_fn[0]) {  // the plan's closed-loop module, built at its first use -- which must not be inside a stream capture
    if (!__atomic_load_n(&p->jit_pol, __ATOMIC_ACQUIRE)) {
      hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess) {
        (void)hipGetLastError();
        return PCG_E_UNSUPPORTED;
      }
      if (cap != hipStreamCaptureStatusNone) return PCG_E_UNSUPPORTED;  // (loading a module is not a capturable operation)
      PCG_TRY(jit_prepare_closed_loop(p));
    }
    return (int)hipModuleLaunchKernel(cov_jit(jit_head_fn(p, head)), grid_for(io->B), 1, 1, BLOCK, 1, 1, 0, (hipStream_t)stream,
                                      argv, nullptr);
  }
  if (kind == ClosedLoopKind::cons) {
    g.g_seq = cons->g_seq; g.g_ss = cons->g_ss; g.g_cs = cons->g_cs;
    g.viol_seq = cons->viol_seq; g.v_ss = cons->v_ss;
    // (env_pre's own pre-step check and store_out see no row storage: the kernel writes the rows it summed itself)
    g.g_last = a.g; g.g_pre = a.g_pre;
    a.g = nullptr; a.g_pre = nullptr;
    g.order_w = feat_route_of_step(p, io) ? 1 : 0;
  }
  (void)hipLaunchKernel(cov(fn), dim3(grid_for(io->B)), dim3(BLOCK), argv, 0, (hipStream_t)stream);
  return (int)hipGetLastError();
}
// The three population entry points' sibling of closed_loop_open, with its order of refusals: plan, buffers and handle; which
// plans the kind's kernels carry (the base kind's, without run-time compiled code: the population kernels are ahead-of-time
// only; or, turned round, the unc kind's or the cons kind's) and which kernel it is; the members' sizes; then what is the
// population's own -- the slices (whole waves per member, a member for every env) and gamma.
static int pop_open(pcg_plan* p, const pcg_buffers* io, const pcg_policy_pop* q, ClosedLoopKind kind, int64_t G, double gamma, StepArgs* a,
                    const void** fn) {
  PCG_TRY(fill_args(p, io, a));
  if (!q) return PCG_E_NULL;
  if (!pop_ok(q) || q->device != p->device) return PCG_E_PLAN;
  const DevConst& c = p->hc;
  const Kernels& k = kernels(p->kid);
  const int ls = lean_scheme(p->integrator_id);
  const bool jit = p->jit_fn[0] != nullptr, f32 = q->dtype == PCG_POL_F32;
  *fn = nullptr;
  if (kind == ClosedLoopKind::unc) {
    // parameters are required; no constraint rows, RK4 alone, and (the null entry) a model with kernels for them
    if (c.nunc <= 0 || c.ncon > 0 || jit || io->t || p->integrator_id != PCG_INT_RK4) return PCG_E_UNSUPPORTED;
    *fn = (const void*)(f32 ? k.roll_policy_pop_unc_f32 : k.roll_policy_pop_unc);
  } else if (kind == ClosedLoopKind::cons) {
    // rows are required; then what the kernels are not built for (per-env parameters, per-env counters, another integrator);
    // then run-time compiled code, a constraint expression among it (no closed-loop module carries these kernels)
    if (c.ncon <= 0) return PCG_E_UNSUPPORTED;
    if (c.nunc > 0 || io->t || ls < 0) return PCG_E_UNSUPPORTED;
    if (jit) return PCG_E_UNSUPPORTED;
    *fn = (const void*)(f32 ? k.roll_policy_pop_cons_f32 : k.roll_policy_pop_cons)[ls];
  } else {
    if (io->t || c.ncon > 0 || c.nunc > 0 || ls < 0) return PCG_E_UNSUPPORTED;
    if (jit) return PCG_E_UNSUPPORTED;
    *fn = (const void*)(f32 ? k.roll_policy_pop_f32 : k.roll_policy_pop)[ls];
  }
  if (!*fn) return PCG_E_UNSUPPORTED;
  if (q->shape.n_in != c.nobs || q->shape.n_out != c.na) return PCG_E_DIM;
  if (G < 64 || G % 64 != 0 || p->env_offset < 0 || p->env_offset % 64 != 0) return PCG_E_VALUE;
  if (io->B > 0 && (p->env_offset + io->B - 1) / G >= (int64_t)q->P) return PCG_E_DIM;
  if (!(std::isfinite(gamma) && gamma >= 0.0 && gamma <= 1.0)) return PCG_E_VALUE;
  return PCG_OK;
}

// PopArgs, alone or as PopConsArgs' base
static void pop_head(PopArgs* pa, const pcg_policy_pop* q, int64_t G, double* a_out, int64_t ao_ss, int64_t ao_cs, int32_t record_next,
                     double gamma, double* ret_out) {
  pa->blocks = (const PCG_CONSTANT char*)q->dP;
  pa->stride = (int64_t)(sizeof(double) * q->blob_doubles);
  pa->G = G;
  pa->a_out = a_out; pa->ao_ss = ao_ss; pa->ao_cs = ao_cs;
  pa->record_next = record_next ? 1 : 0;
  pa->gamma = gamma;
  pa->ret_out = ret_out;
}

// the base and unc population entry points: pop_open, the kernel argument, closed_loop_launch of the kind
static int pop_rollout(pcg_plan* p, const pcg_buffers* io, const pcg_policy_pop* q, ClosedLoopKind kind, int64_t G, int32_t t0, int32_t T,
                       double* a_seq_out, int64_t a_step_stride, int64_t a_comp_stride, double* obs_seq, int64_t obs_step_stride,
                       int64_t obs_comp_stride, double* rew_seq, int64_t rew_step_stride, int32_t record_next_action, double gamma,
                       double* ret_out, uint64_t seed, void* stream) {
  StepArgs a;
  const void* fn;
  PCG_TRY(pop_open(p, io, q, kind, G, gamma, &a, &fn));
  PopArgs pa;
  pop_head(&pa, q, G, a_seq_out, a_step_stride, a_comp_stride, record_next_action, gamma, ret_out);
  const ClosedLoopRun run{t0, T, obs_seq, obs_step_stride, obs_comp_stride, rew_seq, rew_step_stride, seed};
  return closed_loop_launch(p, io, a, fn, kind, nullptr, pa, {{a_seq_out, a_comp_stride}}, run, PCG_OK, stream);
}

// two envs per lane with 16-byte accesses (2-byte for the flags): the rule of the lean kernels' tile I/O (step_lean, rollout_lean) --
// an even batch and every row 16-byte aligned, which here, with caller-given strides, asks for even strides as well
static bool gae_vec2_ok(int64_t B, int32_t T, const double* rew, int64_t rew_ss, const double* val, int64_t val_ss, const uint8_t* term,
                        int64_t term_ss, const double* adv, int64_t adv_ss, const double* ret, int64_t ret_ss) {
  const bool rows = T > 1;  // (a single row has no stride to speak of; val has T + 1 rows)
  return B % 2 == 0 && al16(rew) && al16(val) && al16(adv) && al16(ret) && al2(term) && val_ss % 2 == 0 &&
         (!rows || (rew_ss % 2 == 0 && adv_ss % 2 == 0 && (!ret || ret_ss % 2 == 0) && (!term || term_ss % 2 == 0)));
}

}  // namespace pcg

using namespace pcg;

extern "C" {

int pcg_policy_validate(const pcg_policy_cfg* c) { return policy_validate(c); }

int pcg_policy_create(pcg_policy** out, const pcg_policy_cfg* cfg) { return policy_create(out, cfg, PCG_POL_F64); }
int pcg_policy_create_f32(pcg_policy** out, const pcg_policy_cfg* cfg) { return policy_create(out, cfg, PCG_POL_F32); }

int pcg_policy_dtype(const pcg_policy* q) {
  if (!q) return PCG_E_NULL;
  if (!policy_ok(q)) return PCG_E_PLAN;
  return q->dtype;
}

int pcg_policy_update(pcg_policy* q, const pcg_policy_cfg* cfg) {
  if (!q) return PCG_E_NULL;
  if (!policy_ok(q)) return PCG_E_PLAN;
  PCG_TRY(policy_validate(cfg));
  if (!q->shape.matches(cfg)) return PCG_E_DIM;
  int prc = PCG_OK;
  const std::vector<double> blob = pack_policy(cfg, q->dtype, &prc);
  PCG_TRY(prc);
  if (blob.size() != q->blob_doubles) return PCG_E_DIM;  // (cannot happen: the block's size is a function of the shape)
  const int rc = on_device(q->device, [&] { return (int)hipMemcpy(q->dP, blob.data(), sizeof(double) * blob.size(), hipMemcpyHostToDevice); });
  if (rc == PCG_OK) q->out_map = cfg->out_map;
  return rc;
}

int pcg_policy_destroy(pcg_policy* q) {
  if (!q) return PCG_OK;
  if (!policy_ok(q)) return PCG_E_PLAN;
  q->magic = 0;
  const hipError_t e = hipFree(q->dP);
  delete q;
  return (int)e;
}

int pcg_policy_pop_create(pcg_policy_pop** out, const pcg_policy_cfg* cfg, int32_t P) { return pop_create(out, cfg, P, PCG_POL_F64); }
int pcg_policy_pop_create_f32(pcg_policy_pop** out, const pcg_policy_cfg* cfg, int32_t P) { return pop_create(out, cfg, P, PCG_POL_F32); }

int pcg_policy_pop_dtype(const pcg_policy_pop* q) {
  if (!q) return PCG_E_NULL;
  if (!pop_ok(q)) return PCG_E_PLAN;
  return q->dtype;
}

int pcg_policy_pop_update(pcg_policy_pop* q, const pcg_policy_cfg* cfg, int32_t first, int32_t count) {
  if (!q) return PCG_E_NULL;
  if (!pop_ok(q)) return PCG_E_PLAN;
  PCG_TRY(pop_validate(cfg, count));
  if (first < 0 || (int64_t)first + count > q->P) return PCG_E_DIM;
  if (!q->shape.matches(cfg)) return PCG_E_DIM;
  if (cfg->activation != q->act || cfg->out_map != q->out_map) return PCG_E_VALUE;
  const bool f32 = q->dtype == PCG_POL_F32;
  const double lo = f32 ? (double)(float)cfg->out_low : cfg->out_low, hi = f32 ? (double)(float)cfg->out_high : cfg->out_high;
  if (cfg->out_map == PCG_POL_CLIP && (lo != q->out_lo || hi != q->out_hi)) return PCG_E_VALUE;
  size_t member = 0;
  int prc = PCG_OK;
  const std::vector<double> all = pack_pop(cfg, count, q->dtype, &member, &prc);
  PCG_TRY(prc);  // (every member of the range was judged: no byte is copied)
  if (member != q->blob_doubles) return PCG_E_DIM;  // (cannot happen: the block's size is a function of the shape)
  return on_device(q->device, [&] {
    return (int)hipMemcpy(q->dP + (size_t)first * member, all.data(), sizeof(double) * all.size(), hipMemcpyHostToDevice);
  });
}

int pcg_policy_pop_size(const pcg_policy_pop* q) {
  if (!q) return PCG_E_NULL;
  if (!pop_ok(q)) return PCG_E_PLAN;
  return q->P;
}

int pcg_policy_pop_nparams(const pcg_policy_pop* q) {
  if (!q) return PCG_E_NULL;
  if (!pop_ok(q)) return PCG_E_PLAN;
  return q->lay.n;
}

int pcg_policy_pop_sample(pcg_policy_pop* q, int32_t first, int32_t count, const double* mean, const double* std,
                          int32_t antithetic, uint64_t seed, uint32_t generation, void* stream) {
  if (!q || !mean || !std) return PCG_E_NULL;
  PCG_TRY(pop_search_open(q));
  if (!pop_range_ok(q, first, count)) return PCG_E_DIM;
  if (antithetic != 0 && antithetic != 1) return PCG_E_VALUE;
  PopSampleArgs a;
  a.L = q->lay;
  a.blocks = q->dP;
  a.stride = pop_stride(q);
  a.first = first; a.count = count; a.antithetic = antithetic;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.g = generation;
  a.mean = mean; a.std = std;
  if (q->dtype == PCG_POL_F32)
    hipLaunchKernelGGL(cov(pop_sample_kernel_f32), pop_grid((q->lay.n + 3) / 4, count), dim3(POP_BLOCK), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(cov(pop_sample_kernel), pop_grid((q->lay.n + 3) / 4, count), dim3(POP_BLOCK), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int pcg_policy_pop_noise_dot(const pcg_policy_pop* q, int32_t first, int32_t count, int32_t antithetic, uint64_t seed,
                             uint32_t generation, const double* w, double* partial, double* out, void* stream) {
  static_assert(POP_CHUNK == PCG_POP_CHUNK, "chunk of the fixed summation order");
  if (!q || !w || !partial || !out) return PCG_E_NULL;
  PCG_TRY(pop_search_open(q));
  if (!pop_range_ok(q, first, count)) return PCG_E_DIM;
  if (antithetic != 0 && antithetic != 1) return PCG_E_VALUE;
  PopDotArgs a;
  a.n = q->lay.n;
  a.first = first; a.count = count; a.antithetic = antithetic;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.g = generation;
  a.w = w; a.partial = partial; a.out = out;
  const int64_t chunks = ((int64_t)count + POP_CHUNK - 1) / POP_CHUNK;
  hipLaunchKernelGGL(cov(pop_noise_dot_kernel), pop_grid((a.n + 3) / 4, chunks), dim3(POP_BLOCK), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(cov(pop_chunk_sum_kernel), pop_grid(a.n, 1), dim3(POP_BLOCK), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int pcg_policy_pop_get_flat(const pcg_policy_pop* q, const int32_t* members, int32_t first, int32_t count, double* theta,
                            int64_t theta_member_stride, void* stream) {
  if (!q || !theta) return PCG_E_NULL;
  PCG_TRY(pop_search_open(q));
  if (members ? count < 1 : !pop_range_ok(q, first, count)) return PCG_E_DIM;
  if (theta_member_stride < q->lay.n) return PCG_E_DIM;
  PopFlatArgs a;
  a.L = q->lay;
  a.blocks = q->dP;
  a.stride = pop_stride(q);
  a.P = q->P; a.first = members ? 0 : first; a.count = count;
  a.members = members;
  a.theta = theta; a.theta_stride = theta_member_stride;
  if (q->dtype == PCG_POL_F32)
    hipLaunchKernelGGL(cov(pop_get_flat_kernel_f32), pop_grid(a.L.n, count), dim3(POP_BLOCK), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(cov(pop_get_flat_kernel), pop_grid(a.L.n, count), dim3(POP_BLOCK), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int pcg_policy_pop_set_flat(pcg_policy_pop* q, int32_t first, int32_t count, const double* theta, int64_t theta_member_stride,
                            void* stream) {
  if (!q || !theta) return PCG_E_NULL;
  PCG_TRY(pop_search_open(q));
  if (!pop_range_ok(q, first, count)) return PCG_E_DIM;
  if (theta_member_stride < q->lay.n) return PCG_E_DIM;
  PopFlatArgs a;
  a.L = q->lay;
  a.blocks = q->dP;
  a.stride = pop_stride(q);
  a.P = q->P; a.first = first; a.count = count;
  a.members = nullptr;
  a.theta = const_cast<double*>(theta); a.theta_stride = theta_member_stride;
  if (q->dtype == PCG_POL_F32)
    hipLaunchKernelGGL(cov(pop_set_flat_kernel_f32), pop_grid(a.L.n, count), dim3(POP_BLOCK), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(cov(pop_set_flat_kernel), pop_grid(a.L.n, count), dim3(POP_BLOCK), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int pcg_policy_pop_destroy(pcg_policy_pop* q) {
  if (!q) return PCG_OK;
  if (!pop_ok(q)) return PCG_E_PLAN;
  q->magic = 0;
  const hipError_t e = hipFree(q->dP);
  delete q;
  return (int)e;
}

int pcg_rollout_policy(pcg_plan* p, const pcg_buffers* io, const pcg_policy* q, int32_t t0, int32_t T, double* a_seq_out,
                       int64_t a_step_stride, int64_t a_comp_stride, double* obs_seq, int64_t obs_step_stride,
                       int64_t obs_comp_stride, double* rew_seq, int64_t rew_step_stride, int32_t record_next_action,
                       uint64_t seed, void* stream) {
  StepArgs a;
  const void* fn;
  PCG_TRY(closed_loop_open(p, io, q, ClosedLoopKind::base, false, &a, &fn));
  const PolicyArgs pa = policy_head(q, a_seq_out, a_step_stride, a_comp_stride, record_next_action);
  const ClosedLoopRun run{t0, T, obs_seq, obs_step_stride, obs_comp_stride, rew_seq, rew_step_stride, seed};
  return closed_loop_launch(p, io, a, fn, ClosedLoopKind::base, nullptr, pa, {{a_seq_out, a_comp_stride}}, run, f32_on_jit(p, q), stream);
}

int pcg_rollout_policy_cons(pcg_plan* p, const pcg_buffers* io, const pcg_policy* q, int32_t t0, int32_t T, double* a_seq_out,
                            int64_t a_step_stride, int64_t a_comp_stride, double* obs_seq, int64_t obs_step_stride,
                            int64_t obs_comp_stride, double* rew_seq, int64_t rew_step_stride, int32_t record_next_action,
                            double* g_seq, int64_t g_step_stride, int64_t g_comp_stride, uint8_t* viol_seq,
                            int64_t viol_step_stride, uint64_t seed, void* stream) {
  StepArgs a;
  const void* fn;
  PCG_TRY(closed_loop_open(p, io, q, ClosedLoopKind::cons, false, &a, &fn));
  const PolicyArgs pa = policy_head(q, a_seq_out, a_step_stride, a_comp_stride, record_next_action);
  const ClosedLoopRun run{t0, T, obs_seq, obs_step_stride, obs_comp_stride, rew_seq, rew_step_stride, seed};
  const ConsRec rec{g_seq, g_step_stride, g_comp_stride, viol_seq, viol_step_stride};
  return closed_loop_launch(p, io, a, fn, ClosedLoopKind::cons, &rec, pa, {{a_seq_out, a_comp_stride}}, run, f32_on_jit(p, q), stream);
}

int pcg_rollout_policy_unc(pcg_plan* p, const pcg_buffers* io, const pcg_policy* q, int32_t t0, int32_t T, double* a_seq_out,
                           int64_t a_step_stride, int64_t a_comp_stride, double* obs_seq, int64_t obs_step_stride,
                           int64_t obs_comp_stride, double* rew_seq, int64_t rew_step_stride, int32_t record_next_action,
                           uint64_t seed, void* stream) {
  StepArgs a;
  const void* fn;
  PCG_TRY(closed_loop_open(p, io, q, ClosedLoopKind::unc, false, &a, &fn));
  const PolicyArgs pa = policy_head(q, a_seq_out, a_step_stride, a_comp_stride, record_next_action);
  const ClosedLoopRun run{t0, T, obs_seq, obs_step_stride, obs_comp_stride, rew_seq, rew_step_stride, seed};
  return closed_loop_launch(p, io, a, fn, ClosedLoopKind::unc, nullptr, pa, {{a_seq_out, a_comp_stride}}, run, f32_on_jit(p, q), stream);
}

int pcg_rollout_policy_pop(pcg_plan* p, const pcg_buffers* io, const pcg_policy_pop* q, int64_t envs_per_policy, int32_t t0,
                           int32_t T, double* a_seq_out, int64_t a_step_stride, int64_t a_comp_stride, double* obs_seq,
                           int64_t obs_step_stride, int64_t obs_comp_stride, double* rew_seq, int64_t rew_step_stride,
                           int32_t record_next_action, double gamma, double* ret_out, uint64_t seed, void* stream) {
  return pop_rollout(p, io, q, ClosedLoopKind::base, envs_per_policy, t0, T, a_seq_out, a_step_stride, a_comp_stride, obs_seq,
                     obs_step_stride, obs_comp_stride, rew_seq, rew_step_stride, record_next_action, gamma, ret_out, seed, stream);
}

int pcg_rollout_policy_pop_unc(pcg_plan* p, const pcg_buffers* io, const pcg_policy_pop* q, int64_t envs_per_policy, int32_t t0,
                               int32_t T, double* a_seq_out, int64_t a_step_stride, int64_t a_comp_stride, double* obs_seq,
                               int64_t obs_step_stride, int64_t obs_comp_stride, double* rew_seq, int64_t rew_step_stride,
                               int32_t record_next_action, double gamma, double* ret_out, uint64_t seed, void* stream) {
  return pop_rollout(p, io, q, ClosedLoopKind::unc, envs_per_policy, t0, T, a_seq_out, a_step_stride, a_comp_stride, obs_seq,
                     obs_step_stride, obs_comp_stride, rew_seq, rew_step_stride, record_next_action, gamma, ret_out, seed, stream);
}

int pcg_rollout_policy_pop_cons(pcg_plan* p, const pcg_buffers* io, const pcg_policy_pop* q, int64_t envs_per_policy, int32_t t0,
                                int32_t T, double* a_seq_out, int64_t a_step_stride, int64_t a_comp_stride, double* obs_seq,
                                int64_t obs_step_stride, int64_t obs_comp_stride, double* rew_seq, int64_t rew_step_stride,
                                int32_t record_next_action, double* g_seq, int64_t g_step_stride, int64_t g_comp_stride,
                                uint8_t* viol_seq, int64_t viol_step_stride, double gamma, double* ret_out, int32_t* nviol_out,
                                double* gmax_out, uint64_t seed, void* stream) {
  StepArgs a;
  const void* fn;
  PCG_TRY(pop_open(p, io, q, ClosedLoopKind::cons, envs_per_policy, gamma, &a, &fn));
  PopConsArgs pa;
  pop_head(&pa, q, envs_per_policy, a_seq_out, a_step_stride, a_comp_stride, record_next_action, gamma, ret_out);
  pa.nviol_out = nviol_out;
  pa.gmax_out = gmax_out;
  const ClosedLoopRun run{t0, T, obs_seq, obs_step_stride, obs_comp_stride, rew_seq, rew_step_stride, seed};
  const ConsRec rec{g_seq, g_step_stride, g_comp_stride, viol_seq, viol_step_stride};
  return closed_loop_launch(p, io, a, fn, ClosedLoopKind::cons, &rec, pa, {{a_seq_out, a_comp_stride}}, run, PCG_OK, stream);
}

int pcg_plan_prepare_closed_loop(pcg_plan* p) {
  if (!plan_ok(p)) return PCG_E_PLAN;
  if (!p->jit_fn[0]) return PCG_OK;  // a built-in plan's closed-loop kernels are in the library
  if (!jit_closed_loop_ok(p)) return PCG_E_UNSUPPORTED;
  return jit_prepare_closed_loop(p);
}

// ---- ... with a Gaussian actor and an optional critic (pcg_rollout_actor.hpp) -------------------------------------------
// c0 of log N(u; mu, sigma^2) = c0 - q / 2: the one place this constant is formed (GaussianActorCritic.logp_const reads it
// here, so that the host restatement of the kernel's logp holds the kernel's own bits)
double pcg_actor_logp_const(const double* sigma, int32_t na) {
  if (!sigma || na < 1 || na > PCG_MAX_NA) return std::nan("");
  double s = 0.0;
  for (int i = 0; i < na; ++i) {
    if (!(std::isfinite(sigma[i]) && sigma[i] > 0.0)) return std::nan("");
    s += std::log(sigma[i]);
  }
  const double half_log_2pi = 0.91893853320467274178;
  return -(s + (double)na * half_log_2pi);
}

int pcg_rollout_actor(pcg_plan* p, const pcg_buffers* io, const pcg_policy* q, const pcg_policy* v, const double* sigma,
                      int32_t t0, int32_t T, double* a_seq_out, int64_t a_step_stride, int64_t a_comp_stride,
                      double* u_seq_out, int64_t u_step_stride, int64_t u_comp_stride, double* logp_out,
                      int64_t logp_step_stride, double* value_out, int64_t value_step_stride, double* obs_seq,
                      int64_t obs_step_stride, int64_t obs_comp_stride, double* rew_seq, int64_t rew_step_stride,
                      int32_t record_next_action, uint64_t seed, void* stream) {
  StepArgs a;
  const void* fn;
  PCG_TRY(closed_loop_open(p, io, q, ClosedLoopKind::base, true, &a, &fn));
  ActorArgs aa;
  int late;
  PCG_TRY(actor_head(p, ClosedLoopKind::base, q, v, sigma, a_seq_out, a_step_stride, a_comp_stride, u_seq_out, u_step_stride, u_comp_stride,
                     logp_out, logp_step_stride, value_out, value_step_stride, record_next_action, &aa, &late));
  const ClosedLoopRun run{t0, T, obs_seq, obs_step_stride, obs_comp_stride, rew_seq, rew_step_stride, seed};
  return closed_loop_launch(p, io, a, fn, ClosedLoopKind::base, nullptr, aa, {{a_seq_out, a_comp_stride}, {u_seq_out, u_comp_stride}}, run,
                            late, stream);
}

int pcg_rollout_actor_cons(pcg_plan* p, const pcg_buffers* io, const pcg_policy* q, const pcg_policy* v, const double* sigma,
                           int32_t t0, int32_t T, double* a_seq_out, int64_t a_step_stride, int64_t a_comp_stride,
                           double* u_seq_out, int64_t u_step_stride, int64_t u_comp_stride, double* logp_out,
                           int64_t logp_step_stride, double* value_out, int64_t value_step_stride, double* obs_seq,
                           int64_t obs_step_stride, int64_t obs_comp_stride, double* rew_seq, int64_t rew_step_stride,
                           int32_t record_next_action, double* g_seq, int64_t g_step_stride, int64_t g_comp_stride,
                           uint8_t* viol_seq, int64_t viol_step_stride, uint64_t seed, void* stream) {
  StepArgs a;
  const void* fn;
  PCG_TRY(closed_loop_open(p, io, q, ClosedLoopKind::cons, true, &a, &fn));
  ActorArgs aa;
  int late;
  PCG_TRY(actor_head(p, ClosedLoopKind::cons, q, v, sigma, a_seq_out, a_step_stride, a_comp_stride, u_seq_out, u_step_stride, u_comp_stride,
                     logp_out, logp_step_stride, value_out, value_step_stride, record_next_action, &aa, &late));
  const ClosedLoopRun run{t0, T, obs_seq, obs_step_stride, obs_comp_stride, rew_seq, rew_step_stride, seed};
  const ConsRec rec{g_seq, g_step_stride, g_comp_stride, viol_seq, viol_step_stride};
  return closed_loop_launch(p, io, a, fn, ClosedLoopKind::cons, &rec, aa, {{a_seq_out, a_comp_stride}, {u_seq_out, u_comp_stride}}, run,
                            late, stream);
}

int pcg_rollout_actor_unc(pcg_plan* p, const pcg_buffers* io, const pcg_policy* q, const pcg_policy* v, const double* sigma,
                          int32_t t0, int32_t T, double* a_seq_out, int64_t a_step_stride, int64_t a_comp_stride,
                          double* u_seq_out, int64_t u_step_stride, int64_t u_comp_stride, double* logp_out,
                          int64_t logp_step_stride, double* value_out, int64_t value_step_stride, double* obs_seq,
                          int64_t obs_step_stride, int64_t obs_comp_stride, double* rew_seq, int64_t rew_step_stride,
                          int32_t record_next_action, uint64_t seed, void* stream) {
  StepArgs a;
  const void* fn;
  PCG_TRY(closed_loop_open(p, io, q, ClosedLoopKind::unc, true, &a, &fn));
  ActorArgs aa;
  int late;
  PCG_TRY(actor_head(p, ClosedLoopKind::unc, q, v, sigma, a_seq_out, a_step_stride, a_comp_stride, u_seq_out, u_step_stride, u_comp_stride,
                     logp_out, logp_step_stride, value_out, value_step_stride, record_next_action, &aa, &late));
  const ClosedLoopRun run{t0, T, obs_seq, obs_step_stride, obs_comp_stride, rew_seq, rew_step_stride, seed};
  return closed_loop_launch(p, io, a, fn, ClosedLoopKind::unc, nullptr, aa, {{a_seq_out, a_comp_stride}, {u_seq_out, u_comp_stride}}, run,
                            late, stream);
}

int pcg_policy_noise(pcg_plan* p, int64_t B, int32_t t, uint64_t seed, double* z_out, void* stream) {
  if (!plan_ok(p)) return PCG_E_PLAN;
  if (B < 0) return PCG_E_DIM;
  if (t < 0) return PCG_E_VALUE;
  if (B == 0) return PCG_OK;
  if (!z_out) return PCG_E_NULL;
  hipLaunchKernelGGL(cov(policy_noise_kernel), dim3(grid_for(B)), dim3(BLOCK), 0, (hipStream_t)stream, B, (int32_t)p->hc.na, seed,
                     p->env_offset, (uint32_t)t, z_out);
  return (int)hipGetLastError();
}

int pcg_gae(int64_t B, int32_t T, const double* rew, int64_t rew_step_stride, const double* val, int64_t val_step_stride,
            const uint8_t* term, int64_t term_step_stride, double gamma, double lam, int32_t bootstrap_last, double* adv,
            int64_t adv_step_stride, double* ret, int64_t ret_step_stride, void* stream) {
  if (!rew || !val || !adv) return PCG_E_NULL;
  if (B < 1 || T < 1) return PCG_E_DIM;
  if (val_step_stride < B) return PCG_E_DIM;
  if (T > 1 && (rew_step_stride < B || adv_step_stride < B || (term && term_step_stride < B) || (ret && ret_step_stride < B)))
    return PCG_E_DIM;
  if (!std::isfinite(gamma) || !std::isfinite(lam)) return PCG_E_VALUE;
  GaeArgs a;
  a.B = B;
  a.T = T;
  a.bootstrap_last = bootstrap_last != 0;
  a.vec2 = gae_vec2_ok(B, T, rew, rew_step_stride, val, val_step_stride, term, term_step_stride, adv, adv_step_stride, ret, ret_step_stride);
  a.gamma = gamma;
  a.gl = gamma * lam;  // rounded once, here: the torch loop's `gamma * lam * last` is (gamma * lam) * last
  a.rew = rew;
  a.val = val;
  a.term = term;
  a.adv = adv;
  a.ret = ret;
  a.rew_ss = rew_step_stride;
  a.val_ss = val_step_stride;
  a.term_ss = term_step_stride;
  a.adv_ss = adv_step_stride;
  a.ret_ss = ret_step_stride;
  const int64_t lanes = a.vec2 ? B / 2 : B;
  const int64_t grid = (lanes + GAE_BLOCK - 1) / GAE_BLOCK;
  if (grid > INT32_MAX) return PCG_E_DIM;
  hipLaunchKernelGGL(cov(gae_kernel), dim3((unsigned)grid), dim3(GAE_BLOCK), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // extern "C"
