// pcg_abi.hip -- the core of the C ABI of include/pcgym_hip.h: the kernel table, plan objects, version / status / model
// information, the coverage hook, the model-independent reset kernel and the rhs / integrate / validate hooks.  The other
// concerns live in sibling units behind pcg_host.hpp: configuration folding (pcg_abi_cfg.hip), run-time compilation
// (pcg_abi_jit.hip), launch geometry, step routes, open-loop rollouts and step graphs (pcg_abi_step.hip), policies, populations
// and the closed-loop rollouts (pcg_abi_policy.hip).  The kernel templates live in pcg_kernels.hpp; each model's
// instantiations are compiled in a pcg_inst_*.hip unit.
#include "pcg_host.hpp"

#include <algorithm>

namespace pcg {

// reset (pcgym.py:263-349)
__global__ __launch_bounds__(BLOCK) void reset_kernel(const StepArgs A) {
  CDevConst& c = *A.C;
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= A.B) return;
  if (A.mask && !A.mask[e]) return;
  reset_env(A, c, e, A.seed);
}

// one table of kernel instantiations per model, built in the pcg_inst_*.hip units
Kernels kernels_cstr(), kernels_four_tank(), kernels_me(), kernels_me_reactive(), kernels_cryst(), kernels_affine();
Kernels kernels_complex_cstr(), kernels_disease(), kernels_batch(), kernels_photo(), kernels_cstr_series();
Kernels kernels_distillation(), kernels_polymer(), kernels_biofilm(), kernels_heat_ex(), kernels_inv_batch();
Kernels kernels_oscillators(), kernels_me_sq(), kernels_me_reactive_sq();

// PCG_MODEL_USER has no ahead-of-time kernels: every launch of such a plan goes through its run-time compiled module
static Kernels kernels_user_stub() {
  Kernels k;
  std::memset(&k, 0, sizeof(k));
  k.nraw = -1;
  return k;
}

const Kernels& kernels(int id) {
  static const Kernels K[PCG_KID_COUNT] = {
      kernels_cstr(),        kernels_four_tank(),   kernels_me(),      kernels_me_reactive(), kernels_cryst(),
      kernels_affine(),      kernels_complex_cstr(), kernels_disease(), kernels_batch(),       kernels_photo(),
      kernels_cstr_series(), kernels_distillation(), kernels_polymer(), kernels_biofilm(),     kernels_heat_ex(),
      kernels_inv_batch(),   kernels_oscillators(),  kernels_user_stub(), kernels_me_sq(),     kernels_me_reactive_sq()};
  static_assert(PCG_MODEL_USER == 17 && PCG_KID_ME_SQ == 18 && PCG_KID_COUNT == 20, "kernel table order");
  return K[id];
}

// reference default parameters (model_classes.py:24-33, 877-889, 361-367, 777-786, 1260-1270)
static const double DEF_CSTR[] = {100, 100, 1000, 0.239, -5e4, 8750, 7.2e10, 5e4, 350, 1};
static const double DEF_FOUR_TANK[] = {9.81, 0.2, 0.2, 0.00085, 0.00095, 0.0035, 0.0030, 0.0020, 0.0025, 1, 1, 1, 1};
static const double DEF_ME[] = {5, 5, 1, 5, 2, 0.6, 0.05};
static const double DEF_ME_REACTIVE[] = {5.0, 5.0, 1.0, 0.01, 0.1, 2.0, 2.00, 0.00, 2.00, 0.00};
static const double DEF_CRYST[] = {0.923714966, -6754.878558, 0.92229965554, 1.341205945, 48.07514464, -4921.261419,
                                   1.871281405, 0.50523693,   7.271241375,   7.510905767, 2.658};
// model_classes.py:65-87, 156-158, 222-233, 443-453, 619-630, 689-695, 1172-1182
static const double DEF_COMPLEX_CSTR[] = {100, 100, 1000, 0.239, -5e4, 8750, 7.2e10, -3e4, 9000, 1.0e10, 5e4, 350, 1};
static const double DEF_DISEASE[] = {0.3, 0.1};
static const double DEF_BATCH[] = {1.0, 0.5, 5000, 6000, 8.314, -1000, -1500, 1000, 4.0, 100, 1.0};
static const double DEF_PHOTO[] = {0.0572, 0.0, 504.5, 0.00016, 0.281, 23.51, 16.89, 800.0, 178.9, 447.1, 393.1};
static const double DEF_CSTR_SERIES[] = {97.35, 298, 1e-3, 2e-3, 0.461, 0.732, 1.05e3, 3.766, 3.118e5, 46.14, 58.41, 8.3145e-3};
static const double DEF_DISTILLATION[] = {100.0, 1.0, 5.0, 0.2, 2000.0, 2000.0, 2000.0};
static const double DEF_POLYMER[] = {6e10, 4e10, 9e10, 7750, 8500, 8250, 0.5, 1.0, -3e4, 1200.0, 2.0};
// model_classes.py:1062-1073, 949-960, 269-272, 187-189
static const double DEF_BIOFILM[] = {10.0, 15.0, 1.5, 0.5, 1.0, 300, 0.8, 1.0, 0.5, 0.1, 1.5, 0.5};
static const double DEF_HEAT_EX[] = {1, 1, 1, 1, 2, 3, 1, 1, 1, 1, 1, 1};
static const double DEF_INV_BATCH[] = {55.0, 1.0, 2.0, 1.0};
static const double DEF_OSCILLATORS[] = {10, 1.0, 1.0};
static const double* const DEFAULTS[] = {DEF_CSTR,        DEF_FOUR_TANK, DEF_ME,    DEF_ME_REACTIVE, DEF_CRYST,
                                         nullptr,         DEF_COMPLEX_CSTR, DEF_DISEASE, DEF_BATCH, DEF_PHOTO,
                                         DEF_CSTR_SERIES, DEF_DISTILLATION, DEF_POLYMER, DEF_BIOFILM,
                                         DEF_HEAT_EX,     DEF_INV_BATCH,    DEF_OSCILLATORS, nullptr};

std::mutex g_cov_mu;
std::set<const void*> g_cov_fn;
std::set<hipFunction_t> g_cov_jit;

int fill_args(const pcg_plan* p, const pcg_buffers* io, StepArgs* a) {
  if (!plan_ok(p)) return PCG_E_PLAN;
  if (!io) return PCG_E_NULL;
  if (io->B < 0) return PCG_E_DIM;
  std::memset(a, 0, sizeof(*a));
  a->C = (CDevConst*)p->dC; a->sched = (const PCG_CONSTANT double*)p->dsched;
  a->lean = (const PCG_CONSTANT LeanStep*)p->dlean;
  a->x = io->x; a->a = io->a; a->d = io->d; a->t = io->t; a->a_save = io->a_save; a->obs = io->obs;
  a->rew = io->rew; a->done = io->done; a->viol = io->viol; a->g = io->g; a->g_pre = io->g_pre;
  a->nsteps = io->nsteps; a->B = io->B; a->env_offset = p->env_offset;
  a->p_unc = io->p_unc;
  a->u_prev = io->u_prev;
  a->status = io->status;
  return PCG_OK;
}

}  // namespace pcg

using namespace pcg;

extern "C" {

int pcg_version(void) { return PCG_ABI_VERSION; }

int64_t pcg_coverage_names(char* buf, int64_t cap, int reset) {
  std::string out;
  {
    std::lock_guard<std::mutex> g(g_cov_mu);
    for (const void* f : g_cov_fn) {
      const char* n = hipKernelNameRefByPtr(f, nullptr);
      out += n ? n : "?";
      out += '\n';
    }
    for (hipFunction_t f : g_cov_jit) {
      const char* n = hipKernelNameRef(f);
      out += "jit:";
      out += n ? n : "?";
      out += '\n';
    }
    if (reset) {
      g_cov_fn.clear();
      g_cov_jit.clear();
    }
  }
  if (buf && cap > 0) {
    const size_t n = std::min((size_t)cap - 1, out.size());
    std::memcpy(buf, out.data(), n);
    buf[n] = 0;
  }
  return cov_on() ? (int64_t)out.size() + 1 : -1;
}

const char* pcg_build_id(void) { return PCG_SRC_HASH; }

const char* pcg_strerror(int status) {
  switch (status) {
    case PCG_OK: return "ok";
    case PCG_E_NULL: return "required pointer is NULL";
    case PCG_E_MODEL: return "unknown model or integrator id";
    case PCG_E_DIM: return "dimension out of range or inconsistent";
    case PCG_E_VALUE: return "invalid scalar value";
    case PCG_E_PLAN: return "invalid plan handle or wrong device";
    case PCG_E_UNSUPPORTED: return "combination not supported by this build";
    case PCG_E_JIT: return "a user expression did not compile (see pcg_last_jit_log())";
    default: break;
  }
  if (status > 0) return hipGetErrorString((hipError_t)status);
  return "unknown status";
}

int pcg_model_info(int model_id, int32_t* nx, int32_t* nu, int32_t* ndm, int32_t* n_params) {
  if (model_id < 0 || model_id >= PCG_MODEL_COUNT) return PCG_E_MODEL;
  const Kernels& k = kernels(model_id);
  if (nx) *nx = k.nx;
  if (nu) *nu = k.na;
  if (ndm) *ndm = k.ndm;
  if (n_params) *n_params = k.nraw;
  return PCG_OK;
}

int pcg_model_default_params(int model_id, double* out, int32_t n_out) {
  if (model_id < 0 || model_id >= PCG_MODEL_COUNT) return PCG_E_MODEL;
  if (!out) return PCG_E_NULL;
  const Kernels& k = kernels(model_id);
  if (k.nraw < 0 || !DEFAULTS[model_id]) return PCG_E_UNSUPPORTED;
  if (n_out < k.nraw) return PCG_E_DIM;
  for (int i = 0; i < k.nraw; ++i) out[i] = DEFAULTS[model_id][i];
  return PCG_OK;
}

void pcg_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t o[4];
  philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], o);
  for (int i = 0; i < 4; ++i) out[i] = o[i];
}

int pcg_plan_create(pcg_plan** out, const pcg_env_cfg* cfg) {
  if (!out || !cfg) return PCG_E_NULL;
  *out = nullptr;
  pcg_plan* p = new (std::nothrow) pcg_plan();
  if (!p) return (int)hipErrorOutOfMemory;
  int rc = build_devconst(cfg, &p->hc, &p->cfg_nu);
  if (rc != PCG_OK) {
    delete p;
    return rc;
  }
  p->magic = PLAN_MAGIC;
  p->model_id = cfg->model_id;
  p->kid = kernel_id_for(cfg);
  p->integrator_id = cfg->integrator_id;
  p->nt_stores = 1;  // measured: 20.3 -> 18.7 us per launch on the cstr workload (profiles/)
  p->no_fixup = std::getenv("PCG_NO_FIXUP") != nullptr;
  p->no_flat = std::getenv("PCG_NO_FLAT") != nullptr;
  p->q_force_lean = std::getenv("PCG_Q_FORCE_LEAN") != nullptr;
  p->no_held = std::getenv("PCG_NO_HELD_ROWS") != nullptr;
  p->no_chain = std::getenv("PCG_NO_CHAIN") != nullptr;
  p->nx = cfg->nx;  // (every other field starts zeroed)
  hipError_t e = hipGetDevice(&p->device);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&p->num_cus, hipDeviceAttributeMultiprocessorCount, p->device);
  if (e != hipSuccess) { delete p; return (int)e; }
  const int rows = cfg->nsp + cfg->nd;
  const bool emp = (cfg->flags & PCG_F_UNC_EMPIRICAL) && cfg->nunc > 0;
  const size_t n_emp = emp ? (size_t)cfg->unc_emp_off[cfg->nunc] : 0;
  // behind the schedule rows and the sample tables: the per-step table of the lean kernels (LeanStep[N], 128-byte records)
  const size_t lean_off = (((size_t)(rows > 0 ? rows : 1) * cfg->N + n_emp) + 15) & ~(size_t)15;  // in doubles
  const size_t sched_alloc = sizeof(double) * lean_off + sizeof(LeanStep) * (size_t)cfg->N;
  e = hipMalloc((void**)&p->dC, sizeof(DevConst));
  if (e == hipSuccess) e = hipMalloc((void**)&p->dsched, sched_alloc);
  if (e == hipSuccess) {
    p->dlean = reinterpret_cast<LeanStep*>(p->dsched + lean_off);
    p->hlean = lean_table(p->hc, cfg);
    e = hipMemcpy(p->dlean, p->hlean.data(), sizeof(LeanStep) * p->hlean.size(), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) e = hipMemcpy(p->dC, &p->hc, sizeof(DevConst), hipMemcpyHostToDevice);
  if (e == hipSuccess && cfg->nsp)
    e = hipMemcpy(p->dsched, cfg->sp, sizeof(double) * (size_t)cfg->nsp * cfg->N, hipMemcpyHostToDevice);
  if (e == hipSuccess && cfg->nd)
    e = hipMemcpy(p->dsched + (size_t)cfg->nsp * cfg->N, cfg->d_sched, sizeof(double) * (size_t)cfg->nd * cfg->N,
                  hipMemcpyHostToDevice);
  if (e == hipSuccess && n_emp)  // empirical sample tables behind the schedule rows
    e = hipMemcpy(p->dsched + (size_t)rows * cfg->N, cfg->unc_emp, sizeof(double) * n_emp, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)pcg_plan_destroy(p);
    return (int)e;
  }
  if (cfg->user_cons_src || cfg->user_reward_src || cfg->user_rhs_src) {
    JitModule jm;
    rc = jit_kernels(cfg, p->kid, p->device, &jm);
    if (rc != PCG_OK) {
      (void)pcg_plan_destroy(p);
      return rc;
    }
    p->jit_fn[0] = jm.fn[0];
    p->jit_fn[1] = jm.fn[1];
    p->jit_integ = jm.integ;
    p->jit_rhs = jm.rhs;
    p->jit_roll = jm.roll;
    p->jit_src = new (std::nothrow) JitSource{jit_preamble(cfg), cfg->jit_include_dir, p->kid, cfg->integrator_id};
    if (!p->jit_src) {
      (void)pcg_plan_destroy(p);
      return (int)hipErrorOutOfMemory;
    }
    // Rosenbrock pairs keep nx^2 doubles per lane in LDS: past 48 KB per workgroup (nx >= 10) a kernel has to be told.
    // Decided HERE, so that a plan that cannot run says so at creation and not at its first step.
    const int jnx = cfg->model_id == PCG_MODEL_USER ? cfg->nx : kernels(p->kid).nx;
    const size_t need = sizeof(double) * integ_lds_doubles(jnx, cfg->integrator_id, false) + sched_bytes(p->hc);
    if (need > 48 * 1024) {
      hipFunction_t fns[3] = {jm.fn[0], jm.fn[1], jm.integ};
      for (hipFunction_t f : fns) {
        if (!f) continue;
        const hipError_t ae = hipFuncSetAttribute((const void*)f, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                  (int)std::min(need, LDS_MAX));
        if (ae != hipSuccess) {
          (void)hipGetLastError();
          (void)pcg_plan_destroy(p);
          return PCG_E_UNSUPPORTED;
        }
      }
    }
  }
  rc = plan_geometry(p);
  if (rc != PCG_OK) {
    (void)hipGetLastError();
    (void)pcg_plan_destroy(p);
    return rc;
  }
  *out = p;
  return PCG_OK;
}

int pcg_plan_destroy(pcg_plan* p) {
  if (!plan_ok(p)) return PCG_E_PLAN;
  p->magic = 0;
  hipError_t e1 = hipFree(p->dC), e2 = hipFree(p->dsched);
  if (p->flat_ws) (void)hipFree(p->flat_ws);
  delete p->jit_src;
  delete p;
  if (e1 != hipSuccess) return (int)e1;
  if (e2 != hipSuccess) return (int)e2;
  return PCG_OK;
}

int pcg_plan_set_env_offset(pcg_plan* p, int64_t env_offset) {
  if (!plan_ok(p)) return PCG_E_PLAN;
  p->env_offset = env_offset;
  return PCG_OK;
}

int pcg_plan_set_option(pcg_plan* p, int option, int64_t value) {
  if (!plan_ok(p)) return PCG_E_PLAN;
  switch (option) {
    case PCG_OPT_ENV_OFFSET: p->env_offset = value; return PCG_OK;
    case PCG_OPT_LDS_STAGES: p->lds_stages = value ? 1 : 0; return PCG_OK;
    case PCG_OPT_STREAM_BLOCKS_PER_CU: p->stream_bpc = (int)value; return PCG_OK;
    case PCG_OPT_NT_STORES: p->nt_stores = (int)(value & 7); return PCG_OK;  // bit 0 obs / reward, 1 state, 2 loads
    case PCG_OPT_VARIANT:
      if (value < 0 || value > 5) return PCG_E_VALUE;
      p->variant = (int)value;
      return PCG_OK;
    default: return PCG_E_VALUE;
  }
}

int64_t pcg_plan_bytes_per_env_step(const pcg_plan* p, const pcg_buffers* io) {
  if (!plan_ok(p) || !io) return PCG_E_PLAN;
  const DevConst& c = p->hc;
  // read x, read a, write x', write obs, write reward, done (+viol)
  int64_t A = 8 * (int64_t)(c.nx + c.na + c.nx + c.nobs + 1) + 1;
  if (io->viol) A += 1;
  if (io->d) A += 8 * c.nd;
  if (io->g) A += 8 * c.ncon;
  if (io->t) A += 8;
  if ((c.flags & PCG_F_A_DELTA) && io->a_save) A += 16 * c.na;
  if ((c.flags & PCG_F_REWARD_TRACK) && io->u_prev) A += 16 * c.na;
  if (io->nsteps) A += 8;
  A += 16 * c.nunc;  // per-env parameters read + their observation slots written
  return A;
}

int pcg_reset(pcg_plan* p, const pcg_buffers* io, const uint8_t* mask, uint64_t seed, void* stream) {
  StepArgs a;
  int rc = fill_args(p, io, &a);
  if (rc != PCG_OK) return rc;
  if (io->B == 0) return PCG_OK;
  if (!io->x || !io->obs) return PCG_E_NULL;
  if (p->hc.nunc > 0 && !io->p_unc) return PCG_E_NULL;
  a.mask = mask;
  a.seed = seed;
  hipLaunchKernelGGL(cov(reset_kernel), dim3(grid_for(io->B)), dim3(BLOCK), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int pcg_rhs(pcg_plan* p, int64_t B, const double* x, const double* u, double* dx, void* stream) {
  if (!plan_ok(p)) return PCG_E_PLAN;
  if (!x || !u || !dx) return PCG_E_NULL;
  if (B <= 0) return B == 0 ? PCG_OK : PCG_E_DIM;
  if (p->jit_rhs) {  // PCG_MODEL_USER: the run-time compiled hook
    const PCG_CONSTANT DevConst* dc = (CDevConst*)p->dC;
    int nu = p->cfg_nu;
    void* argv[6] = {&dc, &B, &nu, &x, &u, &dx};
    return (int)hipModuleLaunchKernel(cov_jit(p->jit_rhs), grid_for(B), 1, 1, BLOCK, 1, 1, 0, (hipStream_t)stream, argv, nullptr);
  }
  if (p->model_id == PCG_MODEL_USER) return PCG_E_PLAN;
  const Kernels& k = kernels(p->kid);
  hipLaunchKernelGGL(cov(k.rhs), dim3(grid_for(B)), dim3(BLOCK), 0, (hipStream_t)stream, (CDevConst*)p->dC, B, p->cfg_nu, x, u, dx);
  return (int)hipGetLastError();
}

int pcg_integrate(pcg_plan* p, int64_t B, double* x, const double* u, int32_t* nsteps, void* stream) {
  if (!plan_ok(p)) return PCG_E_PLAN;
  if (!x || !u) return PCG_E_NULL;
  if (B <= 0) return B == 0 ? PCG_OK : PCG_E_DIM;
  if (p->jit_integ) {  // PCG_MODEL_USER: the run-time compiled hook
    const int ub = tb(false, p->integrator_id, p->nx);
    const size_t ush = sizeof(double) * integ_lds_doubles(p->nx, p->integrator_id, false);
    const PCG_CONSTANT DevConst* dc = (CDevConst*)p->dC;
    int nu = p->cfg_nu;
    void* argv[6] = {&dc, &B, &nu, &x, &u, &nsteps};
    return (int)hipModuleLaunchKernel(cov_jit(p->jit_integ), grid_for(B, ub), 1, 1, ub, 1, 1, (unsigned)ush, (hipStream_t)stream, argv,
                                      nullptr);
  }
  if (p->model_id == PCG_MODEL_USER) return PCG_E_PLAN;
  const Kernels& k = kernels(p->kid);
  const bool lds_st = lds_stages_on(p, k);
  size_t shmem;
  const int block = classic_shape(p, k, lds_st, &shmem);
  IntKFn fn = k.integ[p->integrator_id][lds_st ? 1 : 0];
  if (!fn) return PCG_E_UNSUPPORTED;
  if (shmem > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  hipLaunchKernelGGL(cov(fn), dim3(grid_for(B, block)), dim3(block), shmem, (hipStream_t)stream, (CDevConst*)p->dC, B, p->cfg_nu, x,
                     u, nsteps);
  return (int)hipGetLastError();
}

// Host-only validation of a cfg (what pcg_plan_create would return before touching the
// device): lets the host logic be tested on machines without a GPU.
int pcg_cfg_validate(const pcg_env_cfg* cfg) {
  DevConst* d = new (std::nothrow) DevConst();
  if (!d) return (int)hipErrorOutOfMemory;
  int rc = build_devconst(cfg, d, nullptr);
  delete d;
  return rc;
}

}  // extern "C"
