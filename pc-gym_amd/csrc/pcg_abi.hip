// pcg_abi.hip -- the C ABI of include/pcgym_hip.h: configuration folding (build_devconst), plan / graph
// objects, host-side kernel dispatch, and the model-independent reset kernel.  The kernel templates
// live in pcg_kernels.hpp; each model's instantiations are compiled in a pcg_inst_*.hip unit.
#include "pcg_kernels.hpp"
#include "pcg_step_feat.hpp"
#include "pcg_gae.hpp"
#include "pcg_pop_search.hpp"

#include <hip/hiprtc.h>
#include <dirent.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <cerrno>
#include <cstdlib>

#include <fstream>
#include <initializer_list>
#include <map>
#include <mutex>
#include <set>
#include <sstream>
#include <string>
#include <type_traits>

namespace pcg {

// reset (pcgym.py:263-349)
__global__ __launch_bounds__(BLOCK) void reset_kernel(const StepArgs A) {
  CDevConst& c = *A.C;
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= A.B) return;
  if (A.mask && !A.mask[e]) return;
  reset_env(A, c, e, A.seed);
}

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

static const Kernels& kernels(int id) {
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

}  // namespace pcg

using namespace pcg;

struct JitSource;  // (with the run-time compilation, below)

struct pcg_plan {
  uint32_t magic;
  int device;
  int model_id, integrator_id;
  int kid;           // kernel-table id: model_id, or the *_SQ specialisation of the extraction models
  int lds_stages;
  int variant;       // PCG_OPT_VARIANT: 0 auto, 1 classic, 2 stream EPL=1, 3 stream EPL=2
  int stream_bpc;    // PCG_OPT_STREAM_BLOCKS_PER_CU: 0 = occupancy query
  int nt_stores;     // PCG_OPT_NT_STORES
  int num_cus;
  // launch geometry of every persistent kernel the plan could take, settled at creation (plan_geometry)
  int stream_occ[2]; // resident workgroups per CU of the stream kernels [EPL-1]
  int pipe_occ[2][2];  // [auto-reset instantiation][EPL-1]
  int feat_occ[MAX_FEAT];  // resident workgroups per CU of the feature-masked kernels
  int q_bpc[2], q_tile[2]; // work-queue kernel [per_env_t]: resident workgroups per CU, tile slots (0 = no queue launch)
  int q_tile1[2];          // the largest tile with ONE workgroup per CU (Rodas4: launches that fit one tile per CU)
  // reference paths the tests select through the environment, read at creation: PCG_NO_FIXUP (guarded plans in one
  // launch), PCG_NO_FLAT (the single-kernel rollout), PCG_Q_FORCE_LEAN (the lean queue layout wherever it fits)
  // ... and PCG_NO_HELD_ROWS: recorded step graphs store every row in every node (pcg_graph_create; A/B)
  // ... and PCG_NO_CHAIN: they record every step as a launch of its own (A/B, and the way back should a chain misbehave)
  bool no_fixup, no_flat, q_force_lean, no_held, no_chain;
  int64_t env_offset;
  DevConst hc;       // host copy
  DevConst* dC;      // device copy
  double* dsched;    // [nsp+nd][N]
  LeanStep* dlean;   // [N] wave-uniform values of each lock-stepped step (inside the dsched allocation)
  std::vector<LeanStep> hlean;  // host copy of that table: pcg_graph_create compares consecutive steps' slot values
  int cfg_nu;        // na + ndm as the caller counts them
  hipFunction_t jit_fn[2];  // run-time compiled general step kernel with user expressions [per_env_t] (or null)
  hipFunction_t jit_integ, jit_rhs;  // PCG_MODEL_USER: the run-time compiled test hooks (pcg_integrate / pcg_rhs)
  hipFunction_t jit_roll;            // run-time compiled fused rollout of a plan with user expressions (or null)
  // the plan's SECOND module, the two closed-loop kernels: null until the first closed-loop call or
  // pcg_plan_prepare_closed_loop builds it from jit_src (written once, under g_jit_mu; read with acquire)
  hipFunction_t jit_pol, jit_act;
  JitSource* jit_src;                // a run-time compiled plan's preamble (null for a built-in plan)
  int nx;                   // states (the kernel table's for built-in models, the cfg's for PCG_MODEL_USER)
  // work space of the barrier-free rollout (pcg_rollout_flat.hpp): 4 counters + 2 x flat_cap indices, allocated at the first
  // rollout that takes that path (and again if a later batch is larger) -- the only plan state a launch still writes
  int32_t* flat_ws;
  int64_t flat_cap;
};
static constexpr uint32_t PLAN_MAGIC = 0x50434731u;  // 'PCG1'

#define HIP_TRY(expr)                          \
  do {                                         \
    hipError_t _e = (expr);                    \
    if (_e != hipSuccess) return (int)_e;      \
  } while (0)
#define PCG_TRY(expr)                          \
  do {                                         \
    const int _rc = (expr);                    \
    if (_rc != PCG_OK) return _rc;             \
  } while (0)

// Kernel-instantiation coverage (test infrastructure; off unless PCG_COVERAGE is set in the environment when the library is
// loaded).  Every launch site passes its kernel through cov(): with coverage on, the host function pointer (or, for a
// run-time compiled module, the hipFunction_t) is noted in a process-wide set.  pcg_coverage_names() turns the set into
// the kernels' mangled names -- the names tools/kernel_inventory.py reads out of this library's code objects -- so that
// the GPU suite can say which of the shipped instantiations it launched, test by test (tests/conftest.py).
static bool cov_on() {
  static const bool on = std::getenv("PCG_COVERAGE") != nullptr;
  return on;
}
static std::mutex g_cov_mu;
static std::set<const void*> g_cov_fn;        // ahead-of-time kernels: host function pointers
static std::set<hipFunction_t> g_cov_jit;     // run-time compiled kernels
template <class F>
static inline F cov(F fn) {
  if (cov_on()) {
    std::lock_guard<std::mutex> g(g_cov_mu);
    g_cov_fn.insert((const void*)fn);
  }
  return fn;
}
static inline hipFunction_t cov_jit(hipFunction_t fn) {
  if (cov_on()) {
    std::lock_guard<std::mutex> g(g_cov_mu);
    g_cov_jit.insert(fn);
  }
  return fn;
}

// Test hook: the work-queue kernel's tile sort on its own (the step results do not depend on the order, so no parity test
// can see a sort that does not sort -- only a slower launch would).
template <int E, int QB>
__global__ __launch_bounds__(QB) void sort_tile_test_kernel(uint32_t* w) {
  __shared__ uint32_t buf[E * QB];
  uint32_t* g = w + (size_t)blockIdx.x * E * QB;
  for (int i = threadIdx.x; i < E * QB; i += QB) buf[i] = g[i];
  __syncthreads();
  sort_tile<E, QB>(buf);
  for (int i = threadIdx.x; i < E * QB; i += QB) g[i] = buf[i];
}
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

#ifndef PCG_SRC_HASH
#define PCG_SRC_HASH "unknown-build"  // the Makefile passes a digest of csrc/*.hpp, csrc/*.hip and include/pcgym_hip.h
#endif
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

int pcg_test_sort_tile(uint32_t* words, int32_t S, int32_t threads, int64_t ntiles, void* stream) {
  if (!words || ntiles <= 0 || ntiles > 0x7fffffff) return PCG_E_VALUE;
  const dim3 g((unsigned)ntiles);
  hipStream_t st = (hipStream_t)stream;
  if (threads == QBLOCK && S == QSORT / 4) hipLaunchKernelGGL(cov((sort_tile_test_kernel<QSORT / 4 / QBLOCK, QBLOCK>)), g, dim3(QBLOCK), 0, st, words);
  else if (threads == QBLOCK && S == QSORT / 2) hipLaunchKernelGGL(cov((sort_tile_test_kernel<QSORT / 2 / QBLOCK, QBLOCK>)), g, dim3(QBLOCK), 0, st, words);
  else if (threads == QBLOCK && S == QSORT) hipLaunchKernelGGL(cov((sort_tile_test_kernel<QSORT / QBLOCK, QBLOCK>)), g, dim3(QBLOCK), 0, st, words);
  else if (threads == 2 * QBLOCK && S == QSORT / 4) hipLaunchKernelGGL(cov((sort_tile_test_kernel<QSORT / 8 / QBLOCK, 2 * QBLOCK>)), g, dim3(2 * QBLOCK), 0, st, words);
  else if (threads == 2 * QBLOCK && S == QSORT / 2) hipLaunchKernelGGL(cov((sort_tile_test_kernel<QSORT / 4 / QBLOCK, 2 * QBLOCK>)), g, dim3(2 * QBLOCK), 0, st, words);
  else if (threads == 2 * QBLOCK && S == QSORT) hipLaunchKernelGGL(cov((sort_tile_test_kernel<QSORT / 2 / QBLOCK, 2 * QBLOCK>)), g, dim3(2 * QBLOCK), 0, st, words);
  else return PCG_E_UNSUPPORTED;
  return (int)hipGetLastError();
}

void pcg_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t o[4];
  philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], o);
  for (int i = 0; i < 4; ++i) out[i] = o[i];
}

// Validates cfg and fills the host DevConst.  No HIP calls: unit-testable without a GPU.
static int kernel_id_for(const pcg_env_cfg* c);
static int build_devconst(const pcg_env_cfg* c, DevConst* d, int* cfg_nu_out) {
  if (!c || !d) return PCG_E_NULL;
  if (c->model_id < 0 || c->model_id >= PCG_MODEL_COUNT) return PCG_E_MODEL;
  if (c->integrator_id < 0 || c->integrator_id >= PCG_INT_COUNT) return PCG_E_MODEL;
  const bool user = c->model_id == PCG_MODEL_USER;
  Kernels ku = kernels(c->model_id);
  if (user) {  // sizes come from the cfg; the right-hand side from cfg.user_rhs_src
    ku.nx = c->nx; ku.na = c->na; ku.ndm = c->ndm; ku.nraw = c->n_params;
  }
  const Kernels& k = ku;
  const int nx = c->nx, na = c->na, ndm = c->ndm, nd = c->nd, nsp = c->nsp, ncon = c->ncon, nrew = c->nrew;
  if (user) {
    if (!c->user_rhs_src) return PCG_E_NULL;
    if (nx < 1 || nx > PCG_MAX_NX || na < 1 || na > PCG_MAX_NA || ndm < 0 || ndm > PCG_MAX_NDM) return PCG_E_DIM;
    if (c->n_params < 0 || c->n_params > PCG_MAX_USER_PARAMS) return PCG_E_DIM;
    if (c->nunc > 0) return PCG_E_UNSUPPORTED;
  } else if (c->user_rhs_src) {
    return PCG_E_UNSUPPORTED;
  }
  if (user) {
  } else if (k.dynamic) {
    if (nx < 1 || nx > k.nx || na < 1 || na > k.na || ndm != 0) return PCG_E_DIM;
    if (c->n_params != nx * nx + nx * na + nx) return PCG_E_DIM;
  } else {
    if (nx != k.nx || na != k.na) return PCG_E_DIM;
    if (ndm != 0 && ndm != k.ndm) return PCG_E_DIM;
    if (c->n_params != k.nraw) return PCG_E_DIM;
    // coupled_oscillators: the ring size is a structural parameter, only the reference default N = 10 is compiled
    if (c->model_id == PCG_MODEL_OSCILLATORS && (!c->params || c->params[0] != 10.0)) return PCG_E_UNSUPPORTED;
  }
  if (nd < 0 || nd > ndm || nsp < 0 || nsp > PCG_MAX_NSP || ncon < 0 || ncon > PCG_MAX_NCON) return PCG_E_DIM;
  const int nso = c->nsp_obs;
  const int nunc = c->nunc;
  if (nunc < 0 || nunc > PCG_MAX_NUNC) return PCG_E_DIM;
  if (nunc > 0 && (k.dynamic || !c->unc_index || !c->unc_pct)) return nunc > 0 && k.dynamic ? PCG_E_UNSUPPORTED : PCG_E_NULL;
  if (nunc > 0 && ndm > 0 && !c->d_param_index) return PCG_E_NULL;  // Q11: which parameter an unconfigured input reads
  if (nso != 0 && nso != nsp) return PCG_E_DIM;
  if (nd > 0 && nso != nsp) return PCG_E_UNSUPPORTED;
  if (nrew < 0 || nrew > PCG_MAX_NX) return PCG_E_DIM;
  if (c->N < 2 || c->N > PCG_MAX_N) return PCG_E_DIM;
  if (!(c->dt > 0.0) || !std::isfinite(c->dt)) return PCG_E_VALUE;
  if (c->integrator_id == PCG_INT_RK4 && c->substeps < 0) return PCG_E_VALUE;  // 0 = no integration (I/O probe)
  if ((c->integrator_id == PCG_INT_RK4G || c->integrator_id == PCG_INT_T5G) &&
      (c->substeps < 1 || !k.step[c->integrator_id][0][0][0] || c->nunc > 0))
    return c->substeps < 1 ? PCG_E_VALUE : PCG_E_UNSUPPORTED;  // models with a guard hook only
  if (c->integrator_id == PCG_INT_CV8 && (c->substeps < 1 || c->nunc > 0)) return c->substeps < 1 ? PCG_E_VALUE : PCG_E_UNSUPPORTED;
  if (c->integrator_id != PCG_INT_RK4 && (!(c->rtol > 0) || !(c->atol >= 0) || c->max_steps < 1))
    return PCG_E_VALUE;
  const int nobs = nx + nso + nd + nunc, cnu = na + ndm;
  if ((!c->params && !(user && c->n_params == 0)) || !c->x0 || !c->a_low || !c->a_high || !c->o_low || !c->o_high) return PCG_E_NULL;
  if (nsp && (!c->sp_index || !c->sp)) return PCG_E_NULL;
  if ((nsp || nrew) && !c->r_scale) return PCG_E_NULL;
  if (nrew && !c->rew_index) return PCG_E_NULL;
  if (nd && (!c->d_slot || !c->d_sched)) return PCG_E_NULL;
  if (ndm && !c->d_default) return PCG_E_NULL;
  if (ncon && !c->user_cons_src && (!c->con_A || !c->con_b)) return PCG_E_NULL;
  if ((c->user_cons_src || c->user_reward_src) && (k.dynamic || c->nunc > 0)) return PCG_E_UNSUPPORTED;
  if ((c->flags & PCG_F_A_DELTA) && (!c->a_act_low || !c->a_act_high || !c->a_0)) return PCG_E_NULL;
  if ((c->flags & PCG_F_NOISE) && !c->noise_pct) return PCG_E_NULL;
  if ((c->flags & PCG_F_GAUSS_DIST) && nd && (!c->d_sigma || !c->d_clip_lo || !c->d_clip_hi)) return PCG_E_NULL;

  std::memset(d, 0, sizeof(*d));
  double ddef[PCG_MAX_NDM] = {0, 0, 0, 0};
  if (user) {
    static_assert(PCG_MAX_USER_PARAMS <= sizeof(d->kp_big) / sizeof(double), "user parameters live in kp_big");
    for (int i = 0; i < c->n_params; ++i) d->kp_big[i] = c->params[i];
  } else {
    k.prep(c->params, nx, na, k.dynamic ? d->kp_big : d->kp, ddef);
  }
  for (int j = 0; j < k.ndm; ++j) d->d_default[j] = ndm ? c->d_default[j] : ddef[j];
  const bool norm_a = c->flags & PCG_F_NORMALISE_A, norm_o = c->flags & PCG_F_NORMALISE_O;
  const bool compat = c->flags & PCG_F_REF_COMPAT;
  for (int i = 0; i < na; ++i) {
    d->a_lo[i] = c->a_low[i];
    d->a_hi[i] = c->a_high[i];
    if (c->flags & PCG_F_A_DELTA) {
      d->a_act_lo[i] = c->a_act_low[i]; d->a_act_hi[i] = c->a_act_high[i]; d->a_0[i] = c->a_0[i];
    }
  }
  for (int i = 0; i < nobs; ++i) {
    const bool masked = (i < nx) && c->obs_mask && !c->obs_mask[i];
    if (masked) {
      d->omap[i] = OMap{0, 0, 0};
    } else if (norm_o) {
      if (!(c->o_high[i] > c->o_low[i])) return PCG_E_VALUE;
      d->omap[i] = OMap{c->o_low[i], 2.0 / (c->o_high[i] - c->o_low[i]), -1.0};
    } else {
      d->omap[i] = OMap{0, 1, 0};
    }
  }
  for (int i = 0; i < nsp; ++i) {
    if (c->sp_index[i] < 0 || c->sp_index[i] >= nx) return PCG_E_DIM;
    d->sp_index[i] = c->sp_index[i];
  }
  for (int i = 0; i < nrew; ++i) {
    if (c->rew_index[i] < 0 || c->rew_index[i] >= nx) return PCG_E_DIM;
    d->rew_index[i] = c->rew_index[i];
  }
  const int nrs = (c->flags & PCG_F_REWARD_BATCH) ? nrew : nsp;
  for (int i = 0; i < nrs; ++i) d->r_scale[i] = c->r_scale[i];
  if (c->flags & PCG_F_REWARD_TRACK) {
    // normalisation of the tracking reward is always by o_space / a_space (custom_reward.py:14-31), whether or
    // not the env normalises its observations / actions
    if ((c->flags & PCG_F_REWARD_BATCH) || nsp == 0) return PCG_E_UNSUPPORTED;
    if ((c->flags & PCG_F_REWARD_CRYST) && c->model_id != PCG_MODEL_CRYST) return PCG_E_UNSUPPORTED;
    if (c->rew_nbox < 0 || c->rew_nbox > PCG_MAX_RBOX) return PCG_E_DIM;
    if (c->rew_nbox > 0 && (!c->rew_box_index || !c->rew_box_lo || !c->rew_box_hi)) return PCG_E_NULL;
    if (nd > 0) return PCG_E_UNSUPPORTED;  // the reference broadcasts uk (Nu + Nd) against a_space (Nu) there
    for (int k = 0; k < nsp; ++k) {
      const int i = c->sp_index[k];
      const double w = c->o_high[i] - c->o_low[i];
      if (!(w != 0.0)) return PCG_E_VALUE;
      d->trk_lo[k] = c->o_low[i];
      d->trk_inv[k] = 1.0 / w;
    }
    for (int j = 0; j < na; ++j) {
      const double w = c->a_high[j] - c->a_low[j];
      if (!(w != 0.0)) return PCG_E_VALUE;
      d->act_lo[j] = c->a_low[j];
      d->act_inv[j] = 1.0 / w;
    }
    d->R_du = c->rew_R_du;
    d->R_u = c->rew_R_u;
    d->nbox = c->rew_nbox;
    for (int q = 0; q < c->rew_nbox; ++q) {
      const int i = c->rew_box_index[q];
      if (i < 0 || i >= nx) return PCG_E_DIM;
      const double w = c->o_high[i] - c->o_low[i];
      if (!(w != 0.0)) return PCG_E_VALUE;
      d->box_index[q] = i;
      d->box_lo[q] = c->o_low[i];
      d->box_inv[q] = 1.0 / w;
      d->box_lon[q] = (c->rew_box_lo[q] - c->o_low[i]) / w;
      d->box_hin[q] = (c->rew_box_hi[q] - c->o_low[i]) / w;
    }
  }
  if (c->flags & PCG_F_NOISE)
    for (int i = 0; i < nx; ++i) d->noise_pct[i] = c->noise_pct[i];
  for (int i = 0; i < nx + nso; ++i) d->x0[i] = c->x0[i];
  d->has_x0_unc = c->x0_unc ? 1 : 0;
  if (c->x0_unc)
    for (int i = 0; i < nx; ++i) d->x0_unc[i] = c->x0_unc[i];
  for (int i = 0; i < nd; ++i) {
    if (c->d_slot[i] < 0 || c->d_slot[i] >= ndm) return PCG_E_DIM;
    d->d_slot[i] = c->d_slot[i];
    if (c->flags & PCG_F_GAUSS_DIST) {
      d->d_sigma[i] = c->d_sigma[i]; d->d_lo[i] = c->d_clip_lo[i]; d->d_hi[i] = c->d_clip_hi[i];
    }
  }
  // constraint rows: cfg layout [state(nobs) | uk(cnu)] -> padded kernel layout; compat Q3 folded:
  //   state' = (s+1)*hs + lo = s*hs + (hs+lo)   (pcgym.py:601-608), input' likewise with a_space (:597-600)
  // the same quirk for user constraint expressions, as an affine map of the vectors they index
  for (int i = 0; i < PCG_MAX_NOBS; ++i) { d->q3_mul[i] = 1.0; d->q3_add[i] = 0.0; }
  for (int j = 0; j < KNU; ++j) { d->q3u_mul[j] = 1.0; d->q3u_add[j] = 0.0; }
  if (compat && norm_o)
    for (int i = 0; i < nobs; ++i) {
      const double hs = (c->o_high[i] - c->o_low[i]) / 2;
      d->q3_mul[i] = hs;
      d->q3_add[i] = hs + c->o_low[i];
    }
  if (compat && norm_a && c->user_cons_src) {
    if (cnu != na && na != 1) return PCG_E_UNSUPPORTED;  // the reference itself raises (broadcast error)
    for (int j = 0; j < cnu; ++j) {
      const int q = (na == 1) ? 0 : j;
      const double hs = (c->a_high[q] - c->a_low[q]) / 2;
      const int col = (j < na) ? j : k.na + (j - na);  // kernel-side u layout [NA | NDM]
      d->q3u_mul[col] = hs;
      d->q3u_add[col] = hs + c->a_low[q];
    }
  }
  for (int r = 0; r < (c->user_cons_src ? 0 : ncon); ++r) {
    const double* row = c->con_A + (size_t)r * (nobs + cnu);
    double b = c->con_b[r];
    for (int i = 0; i < nobs; ++i) {
      double coef = row[i];
      if (compat && norm_o) {
        const double hs = (c->o_high[i] - c->o_low[i]) / 2;
        b -= coef * (hs + c->o_low[i]);
        coef *= hs;
      }
      if (i >= nx + nso + nd) {  // uncertain-parameter slots cannot enter constraint rows
        if (coef != 0.0) return PCG_E_UNSUPPORTED;
        continue;
      }
      const int col = (i < nx) ? i : (i < nx + nso) ? PCG_MAX_NX + (i - nx) : PCG_MAX_NX + PCG_MAX_NSP + (i - nx - nso);
      d->con_A[r][col] = coef;
    }
    for (int j = 0; j < cnu; ++j) {
      double coef = row[nobs + j];
      if (compat && norm_a) {
        if (cnu != na && na != 1) return PCG_E_UNSUPPORTED;  // the reference itself raises (broadcast error)
        const int q = (na == 1) ? 0 : j;
        const double hs = (c->a_high[q] - c->a_low[q]) / 2;
        b -= coef * (hs + c->a_low[q]);
        coef *= hs;
      }
      const int col = PCG_MAX_NX + PCG_MAX_NSP + PCG_MAX_NDM + ((j < na) ? j : PCG_MAX_NA + (j - na));
      d->con_A[r][col] = coef;
    }
    d->con_b[r] = b;
  }
  d->nunc = nunc;
  if (!k.dynamic && !user)
    for (int i = 0; i < k.nraw && i < 32; ++i) d->raw[i] = c->params[i];
  for (int j = 0; j < nunc; ++j) {
    // index == nraw: an INERT entry (sampled at reset and observed, substituted into no model parameter) -- what the
    // reference does with empirical_distribution['x0'] (pcgym.py:311-316); empirical tables only
    const bool inert = (c->flags & PCG_F_UNC_EMPIRICAL) && c->unc_index[j] == k.nraw && k.nraw < 32;
    if ((c->unc_index[j] < 0 || c->unc_index[j] >= k.nraw) && !inert) return PCG_E_DIM;
    d->unc_index[j] = c->unc_index[j];
    d->unc_pct[j] = c->unc_pct[j];
    if (c->flags & PCG_F_UNC_EMPIRICAL) {
      if (!c->unc_emp || !c->unc_emp_off) return PCG_E_NULL;
      if (c->unc_emp_off[0] != 0 || c->unc_emp_off[j + 1] <= c->unc_emp_off[j] || c->unc_emp_off[j + 1] > PCG_MAX_EMP)
        return PCG_E_DIM;
      d->emp_off[j] = c->unc_emp_off[j];
      d->emp_off[j + 1] = c->unc_emp_off[j + 1];
    }
  }
  d->dt = c->dt;
  d->h = c->dt / (c->substeps > 0 ? c->substeps : 1);
  d->h2 = 0.5 * d->h;
  d->h6 = d->h / 6.0;
  d->rtol = c->rtol;
  d->dt_edge = c->dt * (1.0 - 1e-14);
  d->h_floor = 1e-13 * c->dt;
  // end-point error control of the Rosenbrock pairs (PCG_INT_RODAS4 / PCG_INT_RODAS5, pcgym_hip.h): exponent rate = ep_c x the
  // model's contraction rate
  if (is_ros_pair(c->integrator_id)) {
    if (!(c->ep_frac >= 0.0 && c->ep_frac <= 1.0) || c->ep_kmax < 0 || c->ep_kmax > 40) return PCG_E_VALUE;
    if (c->nunc > 0) return PCG_E_UNSUPPORTED;
    d->ep_kmax = c->ep_kmax;
    d->ep_c = c->ep_kmax > 0 ? c->ep_frac * 1.4426950408889634 : 0.0;
  }
  // cooperative rule (pcgym_hip.h: coop_thr): only where the model's kernels carry it
  d->coop_thr = 0.0;
  if (c->coop_thr != 0.0) {
    if (!(c->coop_thr > 0.0) || !std::isfinite(c->coop_thr)) return PCG_E_VALUE;
    if (!is_ros_pair(c->integrator_id) || user || !c->params || !kernels(kernel_id_for(c)).coop) return PCG_E_UNSUPPORTED;
    d->coop_thr = c->coop_thr;
  }
  d->atol = c->atol;
  d->nx = nx; d->na = na; d->ndm = ndm; d->nd = nd; d->nsp = nsp; d->nsp_obs = nso; d->ncon = ncon; d->nrew = nrew;
  d->N = c->N; d->substeps = c->substeps; d->max_steps = c->max_steps; d->nobs = nobs;
  d->flags = c->flags;
  if (cfg_nu_out) *cfg_nu_out = cnu;
  return PCG_OK;
}

// The wave-uniform values of every lock-stepped step t -> t + 1 (LeanStep, pcg_kernels.hpp), computed here once per plan
// with the operations the kernels used to repeat per tile: the observation slots through the folded OMap as one fused
// multiply-add of (v - lo), the schedule indices of pcgym.py:394,438,555 (quirks Q5, Q6) clamped to the last column.
static std::vector<LeanStep> lean_table(const DevConst& d, const pcg_env_cfg* c) {
  const int N = d.N > 0 ? d.N : 1;
  std::vector<LeanStep> tab((size_t)N);
  for (int t = 0; t < N; ++t) {
    LeanStep& L = tab[(size_t)t];
    std::memset(&L, 0, sizeof(L));
    const int tc = t < N - 1 ? t : N - 1, tn = t + 1 < N - 1 ? t + 1 : N - 1;
    for (int k = 0; k < d.nsp && k < PCG_MAX_NSP; ++k) {
      L.spn[k] = c->sp[(size_t)k * N + tn];
      if (k < d.nsp_obs) {
        const OMap& m = d.omap[d.nx + k];
        L.osp[k] = std::fma(c->sp[(size_t)k * N + tc] - m.lo, m.sc, m.off);
      }
    }
    for (int j = 0; j < PCG_MAX_NDM; ++j) L.ud[j] = d.d_default[j];
    for (int k = 0; k < d.nd && k < PCG_MAX_NDM; ++k) {
      const double v = c->d_sched[(size_t)k * N + tn];
      const OMap& m = d.omap[d.nx + d.nsp_obs + k];
      L.od[k] = std::fma(v - m.lo, m.sc, m.off);
      const int slot = d.d_slot[k];
      if (slot >= 0 && slot < PCG_MAX_NDM) L.ud[slot] = v;
    }
  }
  return tab;
}

// eq_exponent == 2 (the reference default) selects the multiply-only instantiation of the extraction models;
// not when the exponent itself is one of the per-env uncertain parameters.
static int kernel_id_for(const pcg_env_cfg* c) {
  int epos = -1, kid = c->model_id;
  if (c->model_id == PCG_MODEL_ME) { epos = 4; kid = PCG_KID_ME_SQ; }
  if (c->model_id == PCG_MODEL_ME_REACTIVE) { epos = 5; kid = PCG_KID_ME_REACTIVE_SQ; }
  if (epos < 0 || c->params[epos] != 2.0) return c->model_id;
  for (int j = 0; j < c->nunc; ++j)
    if (c->unc_index[j] == epos) return c->model_id;
  return kid;
}

// ---- run-time compilation of user source (pcgym_hip.h: user_cons_src / user_reward_src / user_rhs_src) --------------
// The general one-env-per-lane step kernel of the plan's model is instantiated from the library's own headers with the
// user's source spliced in as pcg_user_constraints / pcg_user_reward / pcg_user_rhs, compiled with hipRTC, loaded as
// a module.  A PCG_MODEL_USER plan has no ahead-of-time kernels at all: its module also carries the test hooks.
struct JitModule {
  hipFunction_t fn[2];      // step_kernel [per_env_t]
  hipFunction_t integ, rhs; // PCG_MODEL_USER only
  hipFunction_t roll;       // fused rollout kernel (null for the Rosenbrock integrators: their matrices live in LDS)
};
// what a plan keeps of its configuration to build its closed-loop module later (jit_closed_loop)
struct JitSource {
  std::string preamble, include_dir;
  int kid, integrator_id;
};
static std::mutex g_jit_mu;
static std::string g_jit_log;

static uint64_t fnv1a(const std::string& s) {
  uint64_t h = 1469598103934665603ull;
  for (unsigned char ch : s) h = (h ^ ch) * 1099511628211ull;
  return h;
}

static uint64_t fnv1a_seed(const std::string& s, uint64_t seed) {
  uint64_t h = 1469598103934665603ull ^ seed;
  for (unsigned char ch : s) h = (h ^ ch) * 1099511628211ull;
  return h;
}

// digest of the headers a run-time compilation will see: every *.hpp of the include directory and the ABI header
// next to it (../../include/pcgym_hip.h), by content.  Cached per directory for the life of the process.
static std::string jit_header_digest(const char* inc_dir) {
  static std::map<std::string, std::string> memo;
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  auto it = memo.find(inc_dir);
  if (it != memo.end()) return it->second;
  std::vector<std::string> files;
  if (DIR* d = ::opendir(inc_dir)) {
    while (dirent* e = ::readdir(d)) {
      const std::string n = e->d_name;
      if (n.size() > 4 && n.compare(n.size() - 4, 4, ".hpp") == 0) files.push_back(std::string(inc_dir) + "/" + n);
    }
    ::closedir(d);
  }
  std::sort(files.begin(), files.end());
  files.push_back(std::string(inc_dir) + "/../../include/pcgym_hip.h");
  uint64_t h1 = 0, h2 = 0;
  for (const std::string& f : files) {
    std::ifstream in(f, std::ios::binary);
    const std::string body((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const std::string tag = f.substr(f.find_last_of('/') + 1) + ":" + std::to_string(body.size()) + ":";
    h1 = fnv1a_seed(tag + body, h1);
    h2 = fnv1a_seed(tag + body, h2 ^ 0x9E3779B97F4A7C15ull);
  }
  char hex[40];
  std::snprintf(hex, sizeof(hex), "%016llx%016llx", (unsigned long long)h1, (unsigned long long)h2);
  return memo[inc_dir] = hex;
}

// The disk cache lives in a directory only its owner can write: $PCG_JIT_CACHE, else $XDG_CACHE_HOME/pcgym_amd, else
// ~/.cache/pcgym_amd -- created with mkdir(2), mode 0700, no shell.  A directory (or file) that belongs to somebody
// else, or that group / others can write, is not used: code objects found there would run inside this process.
// Returns "" when there is no usable directory (the in-process cache still works).
static bool jit_path_private(const std::string& p, bool want_dir) {
  struct stat st;
  if (::lstat(p.c_str(), &st) != 0) return false;
  if (want_dir ? !S_ISDIR(st.st_mode) : !S_ISREG(st.st_mode)) return false;
  return st.st_uid == ::geteuid() && (st.st_mode & (S_IWGRP | S_IWOTH)) == 0;
}
static std::string jit_cache_dir() {
  std::string dir;
  if (const char* e = std::getenv("PCG_JIT_CACHE")) dir = e;
  else if (const char* x = std::getenv("XDG_CACHE_HOME")) dir = std::string(x) + "/pcgym_amd";
  else if (const char* h = std::getenv("HOME")) dir = std::string(h) + "/.cache/pcgym_amd";
  if (dir.empty() || dir[0] != '/') return std::string();
  for (size_t i = 1; i <= dir.size(); ++i)  // mkdir -p, without a shell
    if (i == dir.size() || dir[i] == '/') {
      const std::string part = dir.substr(0, i);
      if (::mkdir(part.c_str(), 0700) != 0 && errno != EEXIST) return std::string();
    }
  return jit_path_private(dir, true) ? dir : std::string();
}
// file = "PCGJIT2\n" nfn lowered names (one per line) code size, two 64-bit digests of (names + code) "\n" code
static bool jit_cache_read(const std::string& path, int nfn, std::string* code, std::string* low) {
  if (!jit_path_private(path, false)) return false;
  std::ifstream in(path, std::ios::binary);
  std::string magic, line;
  if (!std::getline(in, magic) || magic != "PCGJIT2") return false;
  std::string all;
  for (int q = 0; q < nfn; ++q) {
    if (!std::getline(in, low[q]) || low[q].empty()) return false;
    all += low[q] + "\n";
  }
  unsigned long long sz = 0, d1 = 0, d2 = 0;
  if (!std::getline(in, line) || std::sscanf(line.c_str(), "%llu %llx %llx", &sz, &d1, &d2) != 3 || sz == 0 || sz > (1ull << 30))
    return false;
  std::string body((size_t)sz, '\0');
  in.read(&body[0], (std::streamsize)sz);
  if ((unsigned long long)in.gcount() != sz) return false;
  all += body;
  if (fnv1a(all) != d1 || fnv1a_seed(all, 0x9E3779B97F4A7C15ull) != d2) return false;  // truncated / corrupted / edited
  *code = std::move(body);
  return true;
}
static void jit_cache_write(const std::string& path, int nfn, const std::string& code, const std::string* low) {
  // several processes (one per GPU) may compile the same source at once: a private temporary, complete and closed
  // before it appears under the final name; a write error never publishes a file
  const std::string tmp = path + "." + std::to_string((long long)getpid()) + ".tmp";
  const int fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW, 0600);
  if (fd < 0) return;
  std::string all;
  for (int q = 0; q < nfn; ++q) all += low[q] + "\n";
  std::string head = "PCGJIT2\n" + all;
  all += code;
  char meta[96];
  std::snprintf(meta, sizeof(meta), "%llu %016llx %016llx\n", (unsigned long long)code.size(), (unsigned long long)fnv1a(all),
                (unsigned long long)fnv1a_seed(all, 0x9E3779B97F4A7C15ull));
  head += meta;
  bool ok = true;
  const std::string* parts[2] = {&head, &code};
  for (const std::string* part : parts) {
    size_t off = 0;
    while (ok && off < part->size()) {
      const ssize_t w = ::write(fd, part->data() + off, part->size() - off);
      if (w <= 0) ok = false;
      else off += (size_t)w;
    }
  }
  ok = (::close(fd) == 0) && ok;
  if (!ok || std::rename(tmp.c_str(), path.c_str()) != 0) ::unlink(tmp.c_str());
}

// What every translation unit of a plan opens with: the user's macros, the kernel headers, the check that they are the ones
// this library was built from, and the user's source as pcg_user_rhs / pcg_user_constraints / pcg_user_reward.  The step
// module (jit_kernels) and the closed-loop module (jit_closed_loop) differ only in what follows it.
static std::string jit_preamble(const pcg_env_cfg* cfg) {
  const bool user = cfg->model_id == PCG_MODEL_USER;
  std::ostringstream src;
  if (user)
    src << "#define PCG_USER_NX " << cfg->nx << "\n#define PCG_USER_NA " << cfg->na << "\n#define PCG_USER_NDM " << cfg->ndm
        << "\n#define PCG_USER_NP " << cfg->n_params << "\n";
  if (cfg->user_cons_src) src << "#define PCG_USER_NCON " << cfg->ncon << "\n";
  if (cfg->user_reward_src) src << "#define PCG_USER_REWARD 1\n";
  src << "#include \"pcg_kernels.hpp\"\n"
      << "static_assert(sizeof(pcg::DevConst) == " << sizeof(DevConst) << " && sizeof(pcg::StepArgs) == " << sizeof(StepArgs)
      << ", \"kernel headers differ from the ones libpcgym_hip.so was built from\");\n"
      << "namespace pcg {\n";
  if (user)
    src << "__device__ void pcg_user_rhs(const double* x, const double* u, const double* p, double* dx) {\n"
        << cfg->user_rhs_src << "\n}\n";
  if (cfg->user_cons_src)
    src << "__device__ void pcg_user_constraints(const double* x, const double* u, double* g) {\n" << cfg->user_cons_src
        << "\n}\n";
  if (cfg->user_reward_src)
    src << "__device__ double pcg_user_reward(const double* o, const double* x, const double* u, const double* sp, "
           "int violated, int t, int N) {\n  return (double)(" << cfg->user_reward_src << ");\n}\n";
  src << "}\n";
  return src.str();
}

constexpr int JIT_MAX_FN = 5;  // kernels of one run-time compiled module
using JitFns = std::array<hipFunction_t, JIT_MAX_FN>;
static std::map<uint64_t, JitFns> g_jit_cache;

// One translation unit -> one module: fns[q] = the kernel names[q] (a name expression of `text`), q < nfn.  Looked up in the
// process (by text, architecture, ABI, header digest, build id and device), then on disk, then compiled with hipRTC.
// The caller holds g_jit_mu.
static int jit_module(const std::string& text, const std::string* names, int nfn, const std::string& inc_dir, int device,
                      JitFns* fns) {
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  std::string arch = prop.gcnArchName;
  arch = arch.substr(0, arch.find(':'));
  // The translation unit only says `#include "pcg_kernels.hpp"`: the CONTENT of the kernel headers it will be compiled
  // against has to be part of the key too (a changed integrator or model with unchanged struct sizes must not find an
  // old code object) -- hash of every header in the include directory + the ABI header + the library's own build id.
  const std::string hdr = jit_header_digest(inc_dir.c_str());
  const std::string ident = text + "|" + arch + "|" + std::to_string(PCG_ABI_VERSION) + "|" + hdr + "|" PCG_SRC_HASH;
  const uint64_t key = fnv1a(ident + "|" + std::to_string(device));
  auto hit = g_jit_cache.find(key);
  if (hit != g_jit_cache.end()) {
    *fns = hit->second;
    return PCG_OK;
  }
  // disk cache: one file per source = lowered kernel names + code object, with a digest of both
  const std::string dir = jit_cache_dir();
  char hex[40];
  std::snprintf(hex, sizeof(hex), "%016llx%016llx", (unsigned long long)fnv1a(ident), (unsigned long long)fnv1a_seed(ident, 0x9E3779B97F4A7C15ull));
  const std::string path = dir.empty() ? std::string() : dir + "/" + hex + ".pco";
  std::string code, low[JIT_MAX_FN];
  bool from_disk = !path.empty() && jit_cache_read(path, nfn, &code, low);
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (code.empty()) {
      hiprtcProgram prog;
      if (hiprtcCreateProgram(&prog, text.c_str(), "pcg_user_step.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) return PCG_E_JIT;
      for (int q = 0; q < nfn; ++q) hiprtcAddNameExpression(prog, names[q].c_str());
      const std::string oarch = "--offload-arch=" + arch, oinc = "-I" + inc_dir;
      const char* opts[] = {oarch.c_str(), "-O3", "-std=c++17", oinc.c_str()};
      const hiprtcResult cr = hiprtcCompileProgram(prog, 4, opts);
      size_t ls = 0;
      hiprtcGetProgramLogSize(prog, &ls);
      g_jit_log.assign(ls, '\0');
      if (ls) hiprtcGetProgramLog(prog, &g_jit_log[0]);
      if (cr != HIPRTC_SUCCESS) {
        hiprtcDestroyProgram(&prog);
        return PCG_E_JIT;
      }
      for (int q = 0; q < nfn; ++q) {
        const char* ln = nullptr;
        if (hiprtcGetLoweredName(prog, names[q].c_str(), &ln) != HIPRTC_SUCCESS || !ln) {
          hiprtcDestroyProgram(&prog);
          return PCG_E_JIT;
        }
        low[q] = ln;
      }
      size_t cs = 0;
      hiprtcGetCodeSize(prog, &cs);
      code.assign(cs, '\0');
      hiprtcGetCode(prog, &code[0]);
      hiprtcDestroyProgram(&prog);
      if (!path.empty()) jit_cache_write(path, nfn, code, low);  // best effort: an unwritable cache is only slower next time
    }
    hipModule_t mod;
    const hipError_t le = hipModuleLoadData(&mod, code.data());
    if (le != hipSuccess) {
      if (from_disk && attempt == 0) {  // a cached object the driver refuses: drop it and compile afresh
        (void)hipGetLastError();
        ::unlink(path.c_str());
        code.clear();
        from_disk = false;
        continue;
      }
      return (int)le;
    }
    JitFns got{};
    for (int q = 0; q < nfn; ++q) HIP_TRY(hipModuleGetFunction(&got[q], mod, low[q].c_str()));
    g_jit_cache[key] = got;
    *fns = got;
    return PCG_OK;
  }
  return PCG_E_JIT;
}

static int jit_kernels(const pcg_env_cfg* cfg, int kid, int device, JitModule* out) {
  if (!cfg->jit_include_dir) return PCG_E_NULL;
  const bool user = cfg->model_id == PCG_MODEL_USER;
  std::ostringstream src;
  src << jit_preamble(cfg);
  const bool roll = cfg->integrator_id != PCG_INT_RODAS3 && !is_ros_pair(cfg->integrator_id);
  const int iroll = user ? 4 : 2;
  const int nfn = iroll + (roll ? 1 : 0);
  std::string names[JIT_MAX_FN];
  for (int pe = 0; pe < 2; ++pe) {
    std::ostringstream nm;
    nm << "pcg::step_kernel<pcg::Model<" << kid << ">, " << cfg->integrator_id << ", " << (pe ? "true" : "false")
       << ", false, true, false>";
    names[pe] = nm.str();
    src << "template __global__ void " << names[pe] << "(const pcg::StepArgs);\n";
  }
  if (user) {
    std::ostringstream ni, nr;
    ni << "pcg::integrate_kernel<pcg::Model<" << kid << ">, " << cfg->integrator_id << ", false>";
    nr << "pcg::rhs_kernel<pcg::Model<" << kid << "> >";
    names[2] = ni.str();
    names[3] = nr.str();
    src << "template __global__ void " << names[2] << "(pcg::CDevConst*, int64_t, int, double*, const double*, int32_t*);\n";
    src << "template __global__ void " << names[3] << "(pcg::CDevConst*, int64_t, int, const double*, const double*, double*);\n";
  }
  if (roll) {  // pcg_rollout for plans with user expressions: T steps with the state in registers
    std::ostringstream nm;
    nm << "pcg::rollout_kernel<pcg::Model<" << kid << ">, " << cfg->integrator_id << ", false>";
    names[iroll] = nm.str();
    src << "template __global__ void " << names[iroll] << "(const pcg::StepArgs);\n";
  }
  JitFns fns;
  std::lock_guard<std::mutex> lk(g_jit_mu);
  PCG_TRY(jit_module(src.str(), names, nfn, cfg->jit_include_dir, device, &fns));
  out->fn[0] = fns[0];
  out->fn[1] = fns[1];
  out->integ = user ? fns[2] : nullptr;
  out->rhs = user ? fns[3] : nullptr;
  out->roll = roll ? fns[iroll] : nullptr;
  return PCG_OK;
}

// The closed-loop module of a run-time compiled plan: rollout_policy_kernel and rollout_actor_kernel of the plan's model and
// integrator behind the plan's own preamble (JitSource, kept from pcg_plan_create).  Built at the plan's first closed-loop
// call or by pcg_plan_prepare_closed_loop, never at creation: a plan that only steps pays nothing for it.  Same caches, same
// lock and same statuses as the step module.
static int jit_closed_loop(const JitSource& js, int device, hipFunction_t* pol, hipFunction_t* act) {
  std::ostringstream src;
  src << js.preamble << "static_assert(sizeof(pcg::PolicyArgs) == " << sizeof(PolicyArgs) << " && sizeof(pcg::ActorArgs) == "
      << sizeof(ActorArgs) << " && sizeof(pcg::PolicyDev) == " << sizeof(PolicyDev)
      << ", \"closed-loop kernel headers differ from the ones libpcgym_hip.so was built from\");\n";
  std::string names[JIT_MAX_FN];
  const char* kern[2] = {"rollout_policy_kernel", "rollout_actor_kernel"};
  const char* args[2] = {"PolicyArgs", "ActorArgs"};
  for (int q = 0; q < 2; ++q) {
    std::ostringstream nm;
    nm << "pcg::" << kern[q] << "<pcg::Model<" << js.kid << ">, " << js.integrator_id << ">";
    names[q] = nm.str();
    src << "template __global__ void " << names[q] << "(const pcg::StepArgs, const pcg::" << args[q] << ");\n";
  }
  JitFns fns;
  PCG_TRY(jit_module(src.str(), names, 2, js.include_dir, device, &fns));
  *pol = fns[0];
  *act = fns[1];
  return PCG_OK;
}

// ---- launch geometry ------------------------------------------------------------------------------------------
// Dynamic LDS one workgroup may ask for, and the budget of the work-queue kernels' workgroups on one CU (2 KB below it)
constexpr size_t LDS_MAX = 160 * 1024;
constexpr size_t LDS_CU = LDS_MAX - 2048;

static bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }
static bool al2(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 1u) == 0; }

// the plan's schedule rows (set points, disturbances), as per-env-t kernels stage them in LDS
static size_t sched_bytes(const DevConst& c) { return sizeof(double) * (size_t)(c.nsp + c.nd) * c.N; }
// ... what a per-env-t launch stages behind `integ` bytes of the integrator's own LDS (0: they stay in HBM)
static size_t sched_in_lds_bytes(const DevConst& c, size_t integ) {
  const size_t sb = sched_bytes(c);
  return sb > 0 && integ + sb <= (integ > 48 * 1024 ? LDS_MAX : 64 * 1024) ? sb : 0;
}

static bool lds_stages_on(const pcg_plan* p, const Kernels& k) {
  return p->lds_stages && p->integrator_id == PCG_INT_DOPRI5 && k.has_lds_stages;
}
// workgroup size of the plan's one-env-per-lane kernels, and the dynamic LDS their integrator needs (*integ_lds)
static int classic_shape(const pcg_plan* p, const Kernels& k, bool lds_st, size_t* integ_lds) {
  const bool user = p->model_id == PCG_MODEL_USER, rstr = !user && k.ros_structured;  // Rodas4 with the model's own W: no LDS
  const int knx = user ? p->nx : k.nx;  // the kernels' compile-time state count
  *integ_lds = sizeof(double) * integ_lds_doubles(knx, p->integrator_id, lds_st, rstr);
  return tb(lds_st, p->integrator_id, knx, rstr);
}

// Resident 256-thread workgroups per CU (= waves per SIMD) of a persistent kernel (left alone if fn is null).
// The occupancy API over-reports by one for some register counts on ROCm 7.2 (MI355X_MICROARCH.md
// "Residency"), and a persistent grid with a non-resident workgroup serialises a whole extra round:
// bound it by the VGPR allocation too.
static int resident_blocks(StepFn fn, int* out) {
  if (!fn) return PCG_OK;
  int nb = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)fn, BLOCK, 0));
  hipFuncAttributes fa;
  HIP_TRY(hipFuncGetAttributes(&fa, (const void*)fn));
  const int alloc = ((fa.numRegs + 7) / 8) * 8;
  const int by_vgpr = alloc > 0 ? 512 / alloc : 8;
  nb = std::min(nb, std::min(by_vgpr, 8));
  *out = nb > 0 ? nb : 1;
  return PCG_OK;
}

// The work-queue kernels [per_env_t] of the plan's integrator: the adaptive pairs' own launch, the guarded plans' fix-up
static const StepFn* queue_table(const Kernels& k, int integ) {
  switch (integ) {
    case PCG_INT_DOPRI5: return k.queue;
    case PCG_INT_RODAS4: return k.queue_r4;
    case PCG_INT_RODAS5: return k.queue_r5;
    case PCG_INT_RK4G:
    case PCG_INT_T5G: return k.queue_fix;
    default: return nullptr;
  }
}
static const StepFn* queue_w1_table(const Kernels& k, int integ) {
  return integ == PCG_INT_RODAS5 ? k.queue_r5w1 : k.queue_r4w1;
}

// Launch geometry of the work-queue kernel [pe] (pcg_step_queue.hpp): resident 256-thread workgroups per CU by the
// register allocation (= waves per SIMD), the largest tile (<= 1024 slots, four per lane) whose LDS fits that many
// workgroups in the CU's budget; sb = the schedule bytes its launches stage behind the tile.
static int queue_geometry(pcg_plan* p, const Kernels& k, int pe, size_t sb) {
  const StepFn* qtab = queue_table(k, p->integrator_id);
  if (!qtab || !qtab[pe]) return PCG_OK;
  const bool ros = is_ros_pair(p->integrator_id);
  hipFuncAttributes fa;
  HIP_TRY(hipFuncGetAttributes(&fa, (const void*)qtab[pe]));
  const int alloc = ((fa.numRegs + 7) / 8) * 8;
  const int bpc = std::max(1, std::min(4, alloc > 0 ? 512 / alloc : 1));
  // tile cap: four envs per lane for the explicit pair (tuned in round 2); the Rosenbrock pair's attempts per env are
  // heavy-tailed (median 17, 1 % above 70, maximum ~100 on BASELINE configs[2]) and want the largest pool
  const int tcap = ros ? QSORT : QSORT / 2;
  int best_t = 0, best_b = 1, t1 = 0;
  for (int b = bpc; b >= 1; --b) {
    int T = tcap;
    while (T >= QBLOCK && k.queue_lds(T) + sb > LDS_CU / b) T -= 64;
    if (T < QBLOCK) continue;
    if (b == 1) t1 = T;
    if (b * T > best_b * best_t) {
      best_t = T;
      best_b = b;
    }
    if (T == tcap && !ros) break;  // the full tile at the highest occupancy that allows it
  }
  p->q_tile[pe] = best_t;
  p->q_bpc[pe] = best_b;
  p->q_tile1[pe] = t1;
  if (best_t > 0) {
    // (the whole CU's LDS: a launch may also park its tile's state there when that fits, see queue_shape)
    const StepFn wide = p->integrator_id == PCG_INT_DOPRI5 ? k.queue_w[pe] : nullptr;
    const StepFn fns[3] = {qtab[pe], ros ? queue_w1_table(k, p->integrator_id)[pe] : nullptr, wide};
    for (StepFn f : fns)
      if (f) HIP_TRY(hipFuncSetAttribute((const void*)f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_CU));
  }
  return PCG_OK;
}

// Every occupancy and work-queue tile the plan could use, from the cfg and the kernel table alone (the PCG_OPT_* options
// set after creation choose among them): no launch queries the device or changes the plan, so a capture never does.
// Plans without ahead-of-time kernels (PCG_MODEL_USER) have nothing to settle.
static int plan_geometry(pcg_plan* p) {
  if (p->model_id == PCG_MODEL_USER) return PCG_OK;
  const Kernels& k = kernels(p->kid);
  const int integ = p->integrator_id, ls = lean_scheme(integ);
  for (int e = 0; e < 2; ++e) {
    PCG_TRY(resident_blocks(k.stream[integ][e], &p->stream_occ[e]));
    if (ls >= 0) {
      PCG_TRY(resident_blocks(k.pipe[ls][e], &p->pipe_occ[0][e]));
      PCG_TRY(resident_blocks(k.pipe_ar[ls][e], &p->pipe_occ[1][e]));
    }
  }
  if (integ == PCG_INT_RK4)
    for (int i = 0; i < k.nfeat; ++i) PCG_TRY(resident_blocks(k.feat[i].fn, &p->feat_occ[i]));
  // (a per-env-t launch stages the schedules behind the tile where a one-env-per-lane kernel of the plan would)
  PCG_TRY(queue_geometry(p, k, 0, 0));
  size_t integ_lds;
  classic_shape(p, k, false, &integ_lds);
  return queue_geometry(p, k, 1, sched_in_lds_bytes(p->hc, integ_lds));
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

const char* pcg_last_jit_log(void) { return g_jit_log.c_str(); }

static bool plan_ok(const pcg_plan* p) { return p && p->magic == PLAN_MAGIC; }

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

static int fill_args(const pcg_plan* p, const pcg_buffers* io, StepArgs* a) {
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

static inline unsigned grid_for(int64_t B, int block = BLOCK) { return (unsigned)((B + block - 1) / block); }

// anything the lean kernels compile out: observation noise, Gaussian or per-env disturbances, a_delta, the terminal "batch"
// reward, the tracking reward, constraints
static bool has_extras(const DevConst& c, const pcg_buffers* io) {
  return (c.flags & (PCG_F_NOISE | PCG_F_GAUSS_DIST | PCG_F_A_DELTA | PCG_F_REWARD_BATCH | PCG_F_REWARD_TRACK)) || c.ncon > 0 ||
         io->d != nullptr;
}

// A route that took the launch: its status
static bool taken(int* rc, int status) {
  *rc = status;
  return true;
}

// Rodas4, launches of at most ~one full tile per CU (measured: 1024 envs per CU 0.361 -> 0.337 ms; 1366 per CU no
// difference; 4096 per CU 1.47 -> 1.71 ms): ONE workgroup per CU on the instantiation that keeps the whole loop in
// registers, every wave alone on its SIMD
// (the fifth-order pair spills more at two waves per SIMD -- 480 B of scratch per lane against 352 -- and takes the shape up to
// the 1366 envs per CU of BASELINE configs[4]'s segment, whose lean tile of 1408 slots still fits the CU's LDS with its
// state: 330 against 337 us per step, HBM traffic 1.06 x the algorithmic bytes against 1.9 x; under the fourth-order pair
// the same shape was 12 % SLOWER than two workgroups per CU, profiles/r5/mixed_lean_layout.txt, mixed_rodas5.txt)
static bool queue_one_per_cu(const pcg_plan* p, const Kernels& k, int64_t B, int pe) {
  const int w1_cap = p->integrator_id == PCG_INT_RODAS5 ? 1500 : 1200;  // envs per CU up to which the shape is taken
  return is_ros_pair(p->integrator_id) && queue_w1_table(k, p->integrator_id)[pe] && p->q_tile1[pe] >= QBLOCK &&
         B <= (int64_t)p->num_cus * w1_cap && B > (int64_t)p->num_cus * QBLOCK;
}

// The explicit pair at two waves per SIMD: ONE 512-thread workgroup per CU on a tile of up to 2048 slots instead of two
// 256-thread workgroups on 1024 each.  The lanes and the envs per lane are the same, the pool is twice as deep, and the
// two waves of a SIMD drain the same queue: with two workgroups a wave whose SIMD-mate's tile ran dry early finished
// alone (per-wave stamps, tools/queue_probe.py: the 10-state cascade's waves ended between 424 and 737 us of a 737 us
// launch).  Taken when every workgroup still gets >= 1.75 envs per lane.
// (The Rosenbrock pair in this shape -- one 512-thread workgroup per CU, both waves of a SIMD on one tile of 1024 -- was
// built and measured in round 5: a wave that shares its SIMD takes 6.8 us per attempt, i.e. 3.4 us per wave-attempt
// against 3.5 alone; 320-323 us per launch against 305-326: declined, profiles/r5/r4wide_sweep.txt.)
static bool queue_wide(const pcg_plan* p, const Kernels& k, int64_t B, int pe, bool fixup) {
  return !is_ros_pair(p->integrator_id) && !fixup && k.queue_w[pe] && B >= (int64_t)p->num_cus * (7 * 2 * QBLOCK / 4);
}

// The shape of one work-queue launch (pcg_step_queue.hpp) from the plan's settled geometry: no HIP calls.
// sb: the schedule bytes the launch stages behind the tile; forced: at any tile fill (fix-up launches are).
struct QueueShape {
  StepFn fn;       // null: not taken (the tiles would be too thin)
  unsigned grid;   // workgroups of `block` threads, `lds` bytes of dynamic LDS each
  int block;
  size_t lds;
  int32_t q_tile;  // slots | QT_* flags
};
static int queue_shape(const pcg_plan* p, const Kernels& k, int64_t B, int pe, size_t sb, bool fixup, bool forced,
                       QueueShape* s) {
  s->fn = nullptr;
  if (p->q_tile[pe] <= 0) return PCG_OK;
  const bool ros = is_ros_pair(p->integrator_id);
  const bool w1 = queue_one_per_cu(p, k, B, pe), wide = queue_wide(p, k, B, pe, fixup);
  const int qb = wide ? 2 * QBLOCK : QBLOCK, bpc = (w1 || wide) ? 1 : p->q_bpc[pe];
  const size_t lds_wg = LDS_CU / bpc;
  int T = w1 ? p->q_tile1[pe] : p->q_tile[pe];
  if (wide) {
    T = QSORT;
    while (T >= qb && k.queue_lds(T) + sb > LDS_CU) T -= 64;
  }
  const int64_t nwg = std::min((int64_t)p->num_cus * bpc, (B + qb - 1) / qb);  // no workgroup with less than one env per lane
  s->grid = (unsigned)nwg; s->block = qb;
  if (fixup) {  // a tile is a compact list of up to T MARKED envs (+ 4 bytes per slot: which env), the state stays in the batch
    T = p->q_tile[pe];
    while (T > qb && k.queue_lds(T) + 4 * (size_t)T + 8 + sb > lds_wg) T -= 64;
    if (T < qb) return PCG_E_UNSUPPORTED;  // (the scan of the fix-up kernel parks QB envs per round: a smaller tile never advances)
    s->fn = k.queue_fix[pe];
    s->lds = k.queue_lds(T) + 4 * (size_t)T + 8 + sb;
    s->q_tile = T;
    return PCG_OK;
  }
  // The queue only pays when its tiles are well filled: with fewer than ~1.75 envs per lane in a sub-tile the
  // re-balancing gain (measured 1.11x at 2.0 on BASELINE configs[2]) no longer covers the bookkeeping (0.99x at
  // 1.33: the ME segment of configs[4]) -- such launches stay on the classic kernel.
  const int64_t per = (B + nwg - 1) / nwg, nsub = (per + T - 1) / T, sub = (per + nsub - 1) / nsub;
  if (sub < (7 * qb) / 4 && !forced) return PCG_OK;
  auto fit = [qb](int64_t n) { return std::max(qb, (int)((n + 63) / 64 * 64)); };  // slots for n envs
  // LDS for the sub-tile this launch actually walks, not for the largest one the plan could (the kernel derives the
  // same number of sub-tiles from the smaller stride); the tile's state goes to LDS too when that still leaves room
  // for the other workgroups of the CU
  T = std::min(T, fit(sub));
  // A workgroup that has its CU to itself and whose tile's state does not fit in LDS walks two half tiles that do, as
  // long as a lane still gets two envs (the 20-state cascade at B = 2^18: 1024 envs per CU, 2 x 512 with 80 KB of state
  // each).  Scattered 8-byte accesses of a state that stays in the batch reach HBM as 32-byte sectors -- a tile's rows
  // do not survive in L2 between a lane's pick-up and its neighbours' -- 592 MB per launch against 114 MB of algorithm;
  // from LDS the launch moves 137 MB (1.21 x) and takes 1.7 % longer (two envs per lane instead of four for the
  // longest-first order; profiles/r4/queue_probe/).
  // (a full tile whose state fits in the LEAN layout -- below -- is preferred to two half tiles)
  const int nu = p->hc.na + p->hc.nd;
  const bool lean_fits = k.queue_lds_x_lean && k.queue_lds_x_lean(T, nu) + sb <= lds_wg;
  if (!lean_fits && bpc == 1 && !wide && k.queue_lds_x(T) + sb > LDS_CU) {
    const int64_t sub2 = (per + 2 * nsub - 1) / (2 * nsub);
    if (sub2 >= 2 * qb && k.queue_lds_x(fit(sub2)) + sb <= LDS_CU) T = fit(sub2);
  }
  // waves of a workgroup that take part in the cooperative phase of a Rodas4 tile (pcg_step_queue.hpp): the heavy envs of
  // a tile are few (1-2 % at the default threshold) and a wave carries eight at a time -- ONE wave with its groups busy
  // where the workgroup has the CU to itself, two where two workgroups share it (me10_ros4 at B = 2^18: all four waves
  // 326.8 us, two 312.9, one 311.6 at threshold 58; profiles/r5/coop_sweep.txt)
  int32_t flags = ros ? (w1 ? 1 : 2) << QT_COOPW_SHIFT : 0;
  s->lds = k.queue_lds(T) + sb;
  if (!p->q_force_lean && k.queue_lds_x(T) + sb <= lds_wg) {
    flags |= QT_XLDS;
    s->lds = k.queue_lds_x(T) + sb;
  } else if (lean_fits && k.queue_lds_x_lean(T, nu) + sb <= lds_wg) {  // (T may have changed)
    // the LEAN tile layout (pcg_step_queue.hpp, QTile; round 5) where it is what lets the state in: no first-step and
    // step-count arrays, only the configured disturbance values of the held input.  configs[4]'s extraction segment
    // (349,524 envs = 683 per workgroup, two workgroups per CU: 98.8 KB each in the full layout, 76.2 in this one) moved
    // 5.1 x its algorithmic bytes with its state in the batch (profiles/r5/pmc.json)
    flags |= QT_XLDS | QT_LEAN;
    s->lds = k.queue_lds_x_lean(T, nu) + sb;
  }
  s->fn = w1 ? queue_w1_table(k, p->integrator_id)[pe] : wide ? k.queue_w[pe] : queue_table(k, p->integrator_id)[pe];
  s->q_tile = T | flags;
  return PCG_OK;
}

// A work-queue launch: the adaptive plans' own (a.fixup = 0), or the second launch of a guarded plan (a.fixup = 1)
static bool launch_queue(const pcg_plan* p, const Kernels& k, StepArgs a, int pe, bool forced, hipStream_t st, int* rc) {
  QueueShape q;
  const int status = queue_shape(p, k, a.B, pe, a.sched_in_lds ? sched_bytes(p->hc) : 0, a.fixup, forced, &q);
  if (status != PCG_OK) return taken(rc, status);
  if (!q.fn) return false;
  const bool ros = is_ros_pair(p->integrator_id);
  a.q_tile = q.q_tile;
  // (Rodas4: the fit of MEImpl::cost_key_ros) sort-key weight 0 / 10 / 20 / 33 -> me10 0.689 / 0.684 / 0.683 / 0.719 ms,
  // configs[4] shard 0.964 / 0.938 / 0.920 / 0.924 ms (profiles/r2/queue_w_sweep.txt)
  a.q_w = ros ? 3.56f : 20.0f;
  // Rodas4 with two workgroups per CU: a wave that carries one of the 128 heaviest envs of its tile raises its issue
  // priority (s_setprio) -- it then runs at the speed of a wave that has its SIMD to itself (2.9 instead of 4.7 us per
  // attempt) while its SIMD-mate fills the gaps; the two workgroups of a CU start their heaviest envs on different
  // SIMDs.  configs[4]'s ME segment (349,524 envs: too many for one tile per CU): 484 -> 430 us; no effect on the
  // explicit pair (profiles/r3/queue_prio_sweep.txt).
  a.q_prio = ros ? 128 : 0;
  hipLaunchKernelGGL(cov(q.fn), dim3(q.grid), dim3(q.block), q.lds, st, a);
  return taken(rc, (int)hipGetLastError());
}

// ---- pcg_step: the routes, tried in this order by step_impl; each says whether it took the launch (*rc: its status) ----
// which of them did, as step_impl reports it (ROUTE_LEAN_PIPE: step_lean's pipelined kernel, not its auto-reset
// instantiation; ROUTE_LEAN: any other kernel of step_lean)
enum StepRoute { ROUTE_NONE = 0, ROUTE_JIT, ROUTE_UNC, ROUTE_QUEUE, ROUTE_LEAN_PIPE, ROUTE_LEAN, ROUTE_FEAT, ROUTE_CLASSIC };

struct StepCall {
  const pcg_plan* p;
  const Kernels& k;
  const pcg_buffers* io;
  StepArgs a;
  int pe;                 // per-env step counters (io->t): 1
  bool lds_st, extras, auto_reset;
  int block;              // workgroup and dynamic LDS of the one-env-per-lane kernels
  size_t shmem;
  hipStream_t st;
  int32_t held;           // StepArgs::held for the pipelined lean kernel, should it take the launch (pcg_graph_create)
  StepRoute route;        // out: the route that took the launch
};

// run-time compiled general kernel with the plan's user expressions
static bool step_jit(StepCall& s, int* rc) {
  if (!s.p->jit_fn[0]) return false;
  if (s.lds_st) return taken(rc, PCG_E_UNSUPPORTED);
  void* argv[1] = {&s.a};
  return taken(rc, (int)hipModuleLaunchKernel(cov_jit(s.p->jit_fn[s.pe]), grid_for(s.io->B, s.block), 1, 1, s.block, 1, 1,
                                              (unsigned)s.shmem, s.st, argv, nullptr));
}

// per-env uncertain parameters: dedicated general kernel
static bool step_unc(StepCall& s, int* rc) {
  if (s.p->hc.nunc <= 0) return false;
  if (!s.io->p_unc) return taken(rc, PCG_E_NULL);
  const StepFn fn = s.k.step_unc[s.p->integrator_id][s.pe];
  if (!fn) return taken(rc, PCG_E_UNSUPPORTED);
  const size_t sh = s.pe ? sched_in_lds_bytes(s.p->hc, 0) : 0;
  if (sh) s.a.sched_in_lds = 1;
  const int ub = tb(false, s.p->integrator_id);
  hipLaunchKernelGGL(cov(fn), dim3(grid_for(s.io->B, ub)), dim3(ub), sh, s.st, s.a);
  return taken(rc, (int)hipGetLastError());
}

// Adaptive plans: the work-queue kernel (lanes that finish early pull the next env from an LDS tile).
// PCG_OPT_VARIANT 1 keeps the classic one-env-per-lane kernel (A/B measurement), PCG_OPT_LDS_STAGES too;
// PCG_OPT_VARIANT 5 takes the queue for any model and any tile fill.
static bool step_queue(StepCall& s, int* rc) {
  const int integ = s.p->integrator_id;
  const bool forced = s.p->variant == 5;
  if ((integ != PCG_INT_DOPRI5 && !is_ros_pair(integ)) || s.lds_st || (s.p->variant != 0 && !forced) ||
      !queue_table(s.k, integ)[s.pe] || !(s.k.queue_default || forced))
    return false;
  return launch_queue(s.p, s.k, s.a, s.pe, forced, s.st, rc);
}

// streaming (persistent, prefetching, 16 B/lane) kernel for the lean lock-stepped path
// Adaptive stepping is left to the one-wave-per-workgroup classic kernel unless a streaming variant is forced:
// lanes take different numbers of steps, and a persistent grid fixes each wave's share of the batch up front,
// whereas the dispatcher hands single-wave workgroups to whichever SIMD slot frees first.
// (the choice on its own, as feat_pick is: also asked by pcg_graph_create, which records a run of the pipelined RK4 kernel's
// steps as one chained launch.  False: the route leaves the launch.  Otherwise *rc is PCG_OK and *o the launch, or an error.)
struct LeanPick {
  StepFn fn;
  int e;          // envs per lane - 1
  bool piped;     // the software-pipelined kernel
  int64_t grid;
};
static bool lean_pick(const StepCall& s, LeanPick* o, int* rc) {
  const pcg_plan* p = s.p; const Kernels& k = s.k; const pcg_buffers* io = s.io;
  const int integ = p->integrator_id, v = p->variant;
  const int ls = lean_scheme(integ);  // fixed-step schemes with a lean pipelined kernel (RK4, CV8)
  const StepFn* const pipe = ls >= 0 ? k.pipe[ls] : nullptr;
  const bool pipe_ok = (v == 0 || v == 4 || v == 5) && pipe && pipe[0];
  const bool stream_ok = ls >= 0 || v == 2 || v == 3;
  // (the lean kernels index envs and row offsets in 32 bits: B < 2^28; larger batches take the classic kernel)
  if (s.pe || s.extras || s.lds_st || io->viol || (io->status && !pipe_ok) || v == 1 || !stream_ok ||
      (s.auto_reset && !pipe_ok) || io->B >= ((int64_t)1 << 28) || !(k.stream[integ][0] || pipe_ok))
    return false;
  const bool epl2_ok = (k.stream[integ][1] || (pipe_ok && pipe[1])) && (io->B % 2 == 0) && al16(io->x) && al16(io->a) &&
                       al16(io->obs) && al16(io->rew) && al2(io->done);
  if (v == 3 && !epl2_ok) return taken(rc, PCG_E_UNSUPPORTED);
  const int e = (v != 2 && epl2_ok) ? 1 : 0;  // envs per lane - 1
  // auto (0): the software-pipelined kernel where it exists (measured best on the cstr workload:
  // 14.9 us vs 15.0 two-sub-tile streaming vs 16.9 plain streaming vs 21 classic, profiles/r1)
  const bool piped = pipe_ok && pipe[e];
  const StepFn fn = piped ? (s.auto_reset ? k.pipe_ar[ls][e] : pipe[e]) : k.stream[integ][e];
  if (!fn) return taken(rc, PCG_E_UNSUPPORTED);  // (a forced streaming variant of a scheme that only has the pipelined kernel)
  const int occ = piped ? p->pipe_occ[s.auto_reset ? 1 : 0][e] : p->stream_occ[e];
  int bpc = occ;
  // HBM-bound lean kernels: five resident workgroups per CU.  More waves per SIMD only lengthen every wave's integration
  // phase (they share the vector unit round-robin), so the grid's stores leave later and in a shorter burst -- measured on
  // the cstr headline, interleaved runs of one box (profiles/r4/headline_bisect.txt): 4 / 5 / 6 / 8 per CU = 13.96 /
  // 12.60 / 13.58 / 15.1 us.  PCG_OPT_STREAM_BLOCKS_PER_CU overrides.
  if (piped && bpc > 5) bpc = 5;
  if (p->stream_bpc > 0 && p->stream_bpc <= occ) bpc = p->stream_bpc;
  const int64_t grid = std::min((int64_t)p->num_cus * bpc, (io->B + BLOCK * (e + 1) - 1) / (BLOCK * (e + 1)));
  *o = LeanPick{fn, e, piped, grid};
  return taken(rc, PCG_OK);
}

static bool step_lean(StepCall& s, int* rc) {
  LeanPick k;
  if (!lean_pick(s, &k, rc)) return false;
  if (*rc != PCG_OK) return true;
  s.a.nt_stores = s.p->nt_stores;
  // rows the previous node of a step graph left with this step's bytes: only the pipelined kernel skips them, and its
  // auto-reset instantiation never does
  if (k.piped && !s.auto_reset) {
    s.a.held = s.held;
    s.route = ROUTE_LEAN_PIPE;
  }
  hipLaunchKernelGGL(cov(k.fn), dim3((unsigned)k.grid), dim3(BLOCK), 0, s.st, s.a);
  return taken(rc, (int)hipGetLastError());
}

// Feature-masked pipelined kernel (pcg_step_feat.hpp): RK4 plans of the small models with anything beyond the
// lean step switched on.  Needs two envs per lane (even B, 16-byte rows); the smallest instantiation whose mask
// covers what this launch uses is taken.  PCG_OPT_VARIANT 1 forces the classic one-env-per-lane kernel (A/B).
// (the choice on its own: the index into k.feat, or -1 -- also asked by the constrained closed-loop rollouts, whose rows are
// summed in the order of the kernel pcg_step would run on the same buffers: feat_route_of_step)
static int feat_pick(const pcg_plan* p, const Kernels& k, const pcg_buffers* io, int pe, bool lds_st, bool auto_reset) {
  const DevConst& c = p->hc;
  if (p->integrator_id != PCG_INT_RK4 || k.nfeat == 0 || lds_st || !(p->variant == 0 || p->variant == 4 || p->variant == 5))
    return -1;
  // observation noise, per-env step counters, per-env / Gaussian disturbances: the classic kernel is the faster one
  // (measured), and a lock-stepped same-launch reset needs every env to end together
  if (pe || io->d || (c.flags & PCG_F_NOISE) || ((c.flags & PCG_F_GAUSS_DIST) && c.nd > 0) ||
      (auto_reset && (c.flags & PCG_F_DONE_ON_CONS) && c.ncon > 0) || (io->B % 2 != 0) || !al16(io->x) || !al16(io->a) ||
      !al16(io->obs) || !al16(io->rew) || !al2(io->done) || !al2(io->viol) || !al2(io->status) || !al16(io->a_save) ||
      !al16(io->u_prev) || !al16(io->g) || !al16(io->g_pre))
    return -1;
  unsigned need = 0;
  if (c.ncon > 0) need |= FT_CONS;
  if (c.flags & PCG_F_A_DELTA) need |= FT_ADELTA;
  if (c.flags & PCG_F_REWARD_TRACK) need |= FT_TRACK;
  if (c.flags & PCG_F_REWARD_BATCH) need |= FT_BATCH;
  if (auto_reset) need |= FT_AR;
  int best = -1;
  for (int i = 0; i < k.nfeat; ++i)
    if ((k.feat[i].mask & need) == need &&
        (best < 0 || __builtin_popcount(k.feat[i].mask) < __builtin_popcount(k.feat[best].mask)))
      best = i;
  return best;
}

static bool step_feat(StepCall& s, int* rc) {
  const pcg_plan* p = s.p; const Kernels& k = s.k; const pcg_buffers* io = s.io;
  const int best = feat_pick(p, k, io, s.pe, s.lds_st, s.auto_reset);
  if (best < 0) return false;
  int bpc = p->feat_occ[best];
  if (p->stream_bpc > 0 && p->stream_bpc < bpc) bpc = p->stream_bpc;
  const int64_t grid = std::min((int64_t)p->num_cus * bpc, (io->B + 2 * BLOCK - 1) / (2 * BLOCK));
  s.a.nt_stores = p->nt_stores;
  hipLaunchKernelGGL(cov(k.feat[best].fn), dim3((unsigned)grid), dim3(BLOCK), 0, s.st, s.a);
  return taken(rc, (int)hipGetLastError());
}

// The classic one-env-per-lane kernel, which takes every launch the routes above leave.
// Guarded plans (PCG_INT_RK4G / PCG_INT_T5G) in TWO launches: the general kernel takes the guarded fixed step of every
// env and only MARKS the ones it does not trust (done[e] = 2, nothing else of their step stored); the work-queue kernel
// of the adaptive pair then integrates exactly the marked envs -- longest first, lanes pulling the next one -- and
// finishes their step.  In one launch the fallback ran inside the wave that met it: with a third of a batch igniting
// every wave waited for its slowest lane (607 us per 2^20-env step on the full x0 box of the cstr against 362 us for the
// adaptive pair through the queue alone).  Same arithmetic per env either way (tests: the oracle's t5g / rk4g twins).
// Costs the calm closed loop one nearly empty launch.  Not with a_delta (env_pre accumulates into a_save: not idempotent).
static int step_classic(StepCall& s) {
  const pcg_plan* p = s.p;
  const int integ = p->integrator_id;
  s.a.fixup = (integ == PCG_INT_RK4G || integ == PCG_INT_T5G) && !s.lds_st && p->variant == 0 && !(p->hc.flags & PCG_F_A_DELTA) &&
              s.io->B >= (int64_t)p->num_cus * QBLOCK && !p->no_fixup && p->q_tile[s.pe] > 0;
  const StepFn fn = s.k.step[integ][s.pe][s.lds_st ? 1 : 0][s.extras ? 1 : 0];
  if (!fn) return PCG_E_UNSUPPORTED;
  if (s.shmem > 48 * 1024)  // (depends on PCG_OPT_LDS_STAGES: set at launch)
    HIP_TRY(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.shmem));
  hipLaunchKernelGGL(cov(fn), dim3(grid_for(s.io->B, s.block)), dim3(s.block), s.shmem, s.st, s.a);
  int rc = (int)hipGetLastError();
  if (rc != PCG_OK || !s.a.fixup) return rc;
  if (!launch_queue(p, s.k, s.a, s.pe, true, s.st, &rc)) return PCG_E_UNSUPPORTED;  // (not reachable: forced)
  return rc;
}

// held: StepArgs::held, honoured by step_lean's pipelined kernel alone (internal: pcg_graph_create); *route: who took the launch
static int step_impl(pcg_plan* p, const pcg_buffers* io, int32_t t, uint64_t seed, void* stream, bool auto_reset,
                     uint64_t reset_seed, int32_t held = 0, StepRoute* route = nullptr) {
  if (route) *route = ROUTE_NONE;
  StepArgs a;
  int rc = fill_args(p, io, &a);
  if (rc != PCG_OK) return rc;
  if (io->B == 0) return PCG_OK;  // empty batch: nothing to do (zero-size buffers may be NULL)
  if (!io->x || !io->a || !io->obs || !io->rew || !io->done) return PCG_E_NULL;
  const DevConst& c = p->hc;
  if ((c.flags & PCG_F_A_DELTA) && !io->a_save) return PCG_E_NULL;
  if ((c.flags & PCG_F_REWARD_TRACK) && !io->u_prev) return PCG_E_NULL;
  const bool per_env_t = io->t != nullptr;
  if (!per_env_t && t < 0) return PCG_E_VALUE;  // the lock-stepped counter indexes the schedules (t past N-1 clamps, t < 0 cannot)
  a.t_scalar = t; a.seed = seed;
  a.auto_reset = auto_reset ? 1 : 0; a.reset_seed = reset_seed;
  const Kernels& k = kernels(p->kid);
  const bool lds_st = lds_stages_on(p, k);
  StepCall s{p, k, io, a, per_env_t ? 1 : 0, lds_st, has_extras(c, io), auto_reset, 0, 0, (hipStream_t)stream, held, ROUTE_NONE};
  s.block = classic_shape(p, k, lds_st, &s.shmem);
  if (per_env_t) {
    const size_t sb = sched_in_lds_bytes(c, s.shmem);
    s.a.sched_in_lds = sb > 0;
    s.shmem += sb;
  }
  static const struct {
    bool (*take)(StepCall&, int*);
    StepRoute route;
  } routes[] = {{step_jit, ROUTE_JIT},
                {step_unc, ROUTE_UNC},
                {step_queue, ROUTE_QUEUE},
                {step_lean, ROUTE_LEAN},  // (or ROUTE_LEAN_PIPE: step_lean says so itself)
                {step_feat, ROUTE_FEAT}};
  for (const auto& r : routes) {
    s.route = r.route;
    if (r.take(s, &rc)) {
      if (route) *route = s.route;
      return rc;
    }
  }
  if (route) *route = ROUTE_CLASSIC;
  return step_classic(s);
}

// Would step_impl hand the plain step t on these buffers to step_lean's pipelined RK4 kernel (ROUTE_LEAN_PIPE), unforced?
// *e: its envs per lane - 1.  Launches nothing, changes nothing (pcg_graph_create: which steps may join a chained launch).
static bool lean_pipe_rk4(const pcg_plan* p, const pcg_buffers* io, int32_t t, int* e) {
  StepArgs a;
  if (fill_args(p, io, &a) != PCG_OK || io->B <= 0 || !io->x || !io->a || !io->obs || !io->rew || !io->done || io->t || t < 0)
    return false;
  // the routes ahead of step_lean: run-time compiled plans and per-env parameters never get there (step_jit, step_unc;
  // step_queue takes adaptive plans only); a forced variant or grid is somebody's measurement of the per-step kernels
  if (p->integrator_id != PCG_INT_RK4 || p->jit_fn[0] || p->hc.nunc > 0 || p->variant != 0 || p->stream_bpc > 0) return false;
  const Kernels& k = kernels(p->kid);
  const bool lds_st = lds_stages_on(p, k);
  const StepCall s{p, k, io, a, 0, lds_st, has_extras(p->hc, io), false, 0, 0, nullptr, 0, ROUTE_NONE};
  LeanPick pick;
  int rc = PCG_OK;
  if (!lean_pick(s, &pick, &rc) || rc != PCG_OK || !pick.piped || !k.chain[pick.e]) return false;
  *e = pick.e;
  return true;
}

// The n steps t .. t + n - 1 of `steps` (device table: action rows and held words) as ONE launch of step_chain_kernel: one
// workgroup per tile, every tile on its own from its first load to its last store.
static int chain_launch(const pcg_plan* p, const pcg_buffers* io, int32_t t, uint64_t seed, int32_t n, const ChainStep* steps, int e,
                        hipStream_t st) {
  StepArgs a;
  PCG_TRY(fill_args(p, io, &a));
  a.t_scalar = t;
  a.seed = seed;
  a.T = n;
  a.chain = (const PCG_CONSTANT ChainStep*)steps;
  a.nt_stores = p->nt_stores;
  const int64_t tile = (int64_t)BLOCK * (e + 1);
  hipLaunchKernelGGL(cov(kernels(p->kid).chain[e]), dim3((unsigned)((io->B + tile - 1) / tile)), dim3(BLOCK), 0, st, a);
  return (int)hipGetLastError();
}

int pcg_step(pcg_plan* p, const pcg_buffers* io, int32_t t, uint64_t seed, void* stream) {
  return step_impl(p, io, t, seed, stream, false, 0);
}

int pcg_step_autoreset(pcg_plan* p, const pcg_buffers* io, int32_t t, uint64_t seed, uint64_t reset_seed, void* stream) {
  if (plan_ok(p) && io && p->hc.nunc > 0 && !io->p_unc) return PCG_E_NULL;
  return step_impl(p, io, t, seed, stream, true, reset_seed);
}

// ---- pcg_rollout: the routes, in the order pcg_rollout_strided tries them ---------------------------------------
// per-env parameters (sampled by the reset before the episode): the general rollout kernel's UNC form
static bool rollout_unc(const pcg_plan* p, const StepArgs& a, hipStream_t st, int* rc) {
  if (p->hc.nunc <= 0) return false;
  const StepFn fn = kernels(p->kid).rollout_unc[p->integrator_id];
  if (!fn) return taken(rc, PCG_E_UNSUPPORTED);  // RK4 and the explicit pair only, as for stepping
  const int ub = tb(false, p->integrator_id);
  hipLaunchKernelGGL(cov(fn), dim3(grid_for(a.B, ub)), dim3(ub), 0, st, a);
  return taken(rc, (int)hipGetLastError());
}

// run-time compiled rollout kernel with the plan's user expressions (general step, one env per lane)
static bool rollout_jit(const pcg_plan* p, StepArgs a, hipStream_t st, int* rc) {
  if (!p->jit_fn[0]) return false;
  void* argv[1] = {&a};
  const int jb = tb(false, p->integrator_id);
  return taken(rc, (int)hipModuleLaunchKernel(cov_jit(p->jit_roll), grid_for(a.B, jb), 1, 1, jb, 1, 1, 0, st, argv, nullptr));
}

// RK4 lean fused rollout, two envs per lane where the rows stay 16-byte aligned
static bool rollout_lean(const pcg_plan* p, const Kernels& k, const StepArgs& a, const pcg_buffers* io, hipStream_t st, int* rc) {
  if (has_extras(p->hc, io) || p->integrator_id != PCG_INT_RK4 || io->viol || p->variant == 1 || !k.roll_lean[0]) return false;
  const bool even = ((a.a_ss | a.a_cs | a.o_ss | a.o_cs | a.r_ss) & 1) == 0;  // 16-byte rows stay 16-byte aligned
  const bool e2 = even && k.roll_lean[1] && (io->B % 2 == 0) && al16(io->x) && al16(a.a_seq) && al16(io->obs) && al16(io->rew) &&
                  (!a.obs_seq || al16(a.obs_seq)) && (!a.rew_seq || al16(a.rew_seq)) && al2(io->done);
  const int epl = e2 ? 2 : 1;
  hipLaunchKernelGGL(cov(k.roll_lean[epl - 1]), dim3(grid_for(io->B, BLOCK * epl)), dim3(BLOCK), 0, st, a);
  return taken(rc, (int)hipGetLastError());
}

// (re)allocates the plan's flat-rollout work space for B envs and clears its counters on the launch stream
static int flat_workspace(pcg_plan* p, int64_t B, hipStream_t st) {
  if (p->flat_cap < B) {
    if (p->flat_ws) HIP_TRY(hipFree(p->flat_ws));
    p->flat_ws = nullptr; p->flat_cap = 0;
    HIP_TRY(hipMalloc((void**)&p->flat_ws, sizeof(int32_t) * (4 + 2 * (size_t)B)));
    p->flat_cap = B;
  }
  HIP_TRY(hipMemsetAsync(p->flat_ws, 0, sizeof(int32_t) * 4, st));
  return PCG_OK;
}

// The guarded default plan of a model with a guard (PCG_INT_T5G), batches of at least one wave per SIMD: the barrier-free
// rollout in two passes (pcg_rollout_flat.hpp).  The first pass is this plan's ordinary fused rollout kernel, told to hand
// an env over at the first step its guard does not trust; the second carries each handed-over env to the end of the rollout
// on a lane of its own.  Same bits as T pcg_step launches.  Not with a_delta (env_pre accumulates), not while the stream is
// being captured into a graph before the work space exists (hipMalloc); PCG_NO_FLAT=1 keeps the single-kernel rollout (A/B).
static bool rollout_flat(pcg_plan* p, const Kernels& k, StepFn first, StepArgs a, bool lds_st, hipStream_t st, int* rc) {
  if (p->integrator_id != PCG_INT_T5G || !k.roll_hot || lds_st || p->variant != 0 || (p->hc.flags & PCG_F_A_DELTA) || a.T < 2 ||
      a.B < (int64_t)p->num_cus * 4 * 64 || a.B >= ((int64_t)1 << 31) || p->no_flat)
    return false;
  const int status = flat_workspace(p, a.B, st);
  if (status != PCG_OK) return taken(rc, status);
  a.flat_q = p->flat_ws;
  a.flat_hot = p->flat_ws + 4;
  a.flat_tstar = p->flat_ws + 4 + p->flat_cap;
  a.fixup = 1;
  const int block = tb(false, PCG_INT_T5G);
  hipLaunchKernelGGL(cov(first), dim3(grid_for(a.B, block)), dim3(block), 0, st, a);
  if (hipError_t e = hipGetLastError()) return taken(rc, (int)e);
  const int wps = 3;  // persistent waves per SIMD of the second pass (measured: profiles/r6/flat_rollout.txt)
  a.q_tile = 2;       // ... and the cadence of its step boundaries (rollout_kernel_hot: `every`)
  hipLaunchKernelGGL(cov(k.roll_hot), dim3((unsigned)(p->num_cus * wps)), dim3(FLAT_BLOCK), 0, st, a);
  return taken(rc, (int)hipGetLastError());
}

int pcg_rollout_strided(pcg_plan* p, const pcg_buffers* io, int32_t t0, int32_t T, const double* a_seq,
                        int64_t a_step_stride, int64_t a_comp_stride, double* obs_seq, int64_t obs_step_stride,
                        int64_t obs_comp_stride, double* rew_seq, int64_t rew_step_stride, uint64_t seed,
                        void* stream) {
  StepArgs a;
  int rc = fill_args(p, io, &a);
  if (rc != PCG_OK) return rc;
  if (io->t) return PCG_E_UNSUPPORTED;  // lock-stepped only
  if (T < 1 || t0 < 0 || (int64_t)t0 + (int64_t)T > 0x7fffffffLL) return PCG_E_VALUE;  // (t0 indexes the per-step tables)
  if (io->B == 0) return PCG_OK;
  if (!io->x || !a_seq || !io->obs || !io->rew || !io->done) return PCG_E_NULL;
  const DevConst& c = p->hc;
  if ((c.flags & PCG_F_A_DELTA) && !io->a_save) return PCG_E_NULL;
  if ((c.flags & PCG_F_REWARD_TRACK) && !io->u_prev) return PCG_E_NULL;
  if (p->jit_fn[0] && !p->jit_roll) return PCG_E_UNSUPPORTED;
  if (c.nunc > 0 && !io->p_unc) return PCG_E_NULL;
  a.t_scalar = t0; a.seed = seed; a.T = T;
  a.a_seq = a_seq; a.obs_seq = obs_seq; a.rew_seq = rew_seq;
  a.a_ss = a_step_stride; a.a_cs = a_comp_stride;
  a.o_ss = obs_step_stride; a.o_cs = obs_comp_stride;
  a.r_ss = rew_step_stride;
  if (a.a_cs < io->B || (obs_seq && a.o_cs < io->B)) return PCG_E_DIM;
  // the rows a rollout WRITES must not overlap (lanes store them without waiting for one another): reward rows a full
  // batch apart, observation rows either step-major ([T][Nobs][B]-like) or component-major (the reference's axis order)
  if (rew_seq && T > 1 && a.r_ss < io->B) return PCG_E_DIM;
  if (obs_seq) {
    const int64_t B = io->B, n = c.nobs;
    const bool step_major = T == 1 || a.o_ss >= (n - 1) * a.o_cs + B;
    const bool comp_major = a.o_ss >= B && (n == 1 || a.o_cs >= (int64_t)(T - 1) * a.o_ss + B);
    if (!step_major && !comp_major) return PCG_E_DIM;
  }
  const hipStream_t st = (hipStream_t)stream;
  const Kernels& k = kernels(p->kid);
  if (rollout_unc(p, a, st, &rc) || rollout_jit(p, a, st, &rc) || rollout_lean(p, k, a, io, st, &rc)) return rc;
  const bool lds_st = lds_stages_on(p, k);
  const StepFn fn = k.rollout[p->integrator_id][lds_st ? 1 : 0];
  if (!fn) return PCG_E_UNSUPPORTED;  // the Rosenbrock integrator steps through pcg_step only
  if (rollout_flat(p, k, fn, a, lds_st, st, &rc)) return rc;
  const int block = tb(lds_st, p->integrator_id);
  const size_t shmem = lds_st ? sizeof(double) * 6 * (size_t)k.nx * BLOCK_LDS : 0;
  if (shmem > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  hipLaunchKernelGGL(cov(fn), dim3(grid_for(io->B, block)), dim3(block), shmem, st, a);
  return (int)hipGetLastError();
}

int pcg_rollout(pcg_plan* p, const pcg_buffers* io, int32_t t0, int32_t T, const double* a_seq, double* obs_seq,
                double* rew_seq, uint64_t seed, void* stream) {
  if (!plan_ok(p)) return PCG_E_PLAN;
  if (!io) return PCG_E_NULL;
  const int64_t B = io->B;
  return pcg_rollout_strided(p, io, t0, T, a_seq, (int64_t)p->hc.na * B, B, obs_seq, (int64_t)p->hc.nobs * B, B, rew_seq,
                             B, seed, stream);
}

// ---- closed-loop fused rollout with an on-device MLP policy (pcg_rollout_policy.hpp) ------------------------------------
struct pcg_policy {
  uint32_t magic;
  int device;
  int n_in, n_out;
  int n_hidden, width[2], out_map;  // the shape pcg_policy_update holds a new cfg against; the map pcg_rollout_actor asks for
  size_t blob_doubles;              // size of the device block
  PolicyDev* dP;  // header + packed weights; rewritten only by pcg_policy_update (same shape, same block)
  int dtype;      // PCG_POL_F64 | PCG_POL_F32: which packing the block holds, hence which kernel family reads it
};
static constexpr uint32_t POLICY_MAGIC = 0x50434750u;  // 'PCGP'

// layer l of a validated cfg: (rows, columns)
static void policy_layer_dims(const pcg_policy_cfg* c, int l, int* rows, int* cols) {
  *cols = l == 0 ? c->n_in : c->width[l - 1];
  *rows = l == c->n_hidden ? c->n_out : c->width[l];
}

int pcg_policy_validate(const pcg_policy_cfg* c) {
  if (!c) return PCG_E_NULL;
  if (c->n_in < 1 || c->n_in > PCG_MAX_NOBS || c->n_out < 1 || c->n_out > PCG_MAX_NA) return PCG_E_DIM;
  if (c->n_hidden < 0 || c->n_hidden > 2) return PCG_E_DIM;
  for (int l = 0; l < c->n_hidden; ++l)
    if (c->width[l] < 1 || c->width[l] > PCG_POL_MAX_WIDTH) return PCG_E_DIM;
  if (c->activation != PCG_ACT_TANH && c->activation != PCG_ACT_RELU) return PCG_E_VALUE;
  if (c->out_map != PCG_POL_NONE && c->out_map != PCG_POL_CLIP && c->out_map != PCG_POL_TANH) return PCG_E_VALUE;
  if (c->out_map == PCG_POL_CLIP && !(std::isfinite(c->out_low) && std::isfinite(c->out_high) && c->out_low <= c->out_high))
    return PCG_E_VALUE;
  for (int l = 0; l <= c->n_hidden; ++l) {
    if (!c->W[l] || !c->b[l]) return PCG_E_NULL;
    int rows, cols;
    policy_layer_dims(c, l, &rows, &cols);
    for (int i = 0; i < rows * cols; ++i)
      if (!std::isfinite(c->W[l][i])) return PCG_E_VALUE;
    for (int i = 0; i < rows; ++i)
      if (!std::isfinite(c->b[l][i])) return PCG_E_VALUE;
  }
  return PCG_OK;
}

// The device block of a policy: header, then every layer's matrix and bias padded with zeros to the block sizes the
// kernel unrolls by (pcg_rollout_policy.hpp) -- rows of a hidden layer to POL_HB (fed by the observation) or POL_SB
// (streamed), rows of the output layer to PCG_MAX_NA, columns to POL_IB (observation) or POL_HB / POL_SB (hidden units).
static std::vector<double> pack_policy(const pcg_policy_cfg* c) {
  static_assert(POL_MAX_W == PCG_POL_MAX_WIDTH && POL_MAX_W % POL_HB == 0 && POL_HB % POL_SB == 0, "policy block sizes");
  auto up = [](int n, int m) { return (n + m - 1) / m * m; };
  PolicyDev h;
  std::memset(&h, 0, sizeof(h));
  h.n_in = c->n_in; h.n_out = c->n_out; h.n_hidden = c->n_hidden; h.act = c->activation; h.out_map = c->out_map;
  h.out_lo = c->out_low; h.out_hi = c->out_high;
  for (int l = 0; l < c->n_hidden; ++l) h.w[l] = c->width[l];
  std::vector<double> data;
  for (int l = 0; l <= c->n_hidden; ++l) {
    int rows, cols;
    policy_layer_dims(c, l, &rows, &cols);
    const bool outl = l == c->n_hidden;
    const int prow = outl ? PCG_MAX_NA : up(rows, l == 0 ? POL_HB : POL_SB);
    const int pcol = l == 0 ? up(cols, POL_IB) : up(cols, l == 1 ? POL_HB : POL_SB);
    h.ld[l] = pcol;
    h.offW[l] = (int32_t)data.size();
    data.resize(data.size() + (size_t)prow * pcol, 0.0);
    for (int r = 0; r < rows; ++r)
      for (int k = 0; k < cols; ++k) data[(size_t)h.offW[l] + (size_t)r * pcol + k] = c->W[l][(size_t)r * cols + k];
    h.offb[l] = (int32_t)data.size();
    data.resize(data.size() + (size_t)prow, 0.0);
    for (int r = 0; r < rows; ++r) data[(size_t)h.offb[l] + r] = c->b[l][r];
  }
  // (one scalar load may fetch up to sixteen words: the block ends in slack, so that no fetch ends outside it)
  std::vector<double> blob(sizeof(PolicyDev) / sizeof(double) + data.size() + 16, 0.0);
  std::memcpy(blob.data(), &h, sizeof(h));
  std::memcpy(blob.data() + sizeof(PolicyDev) / sizeof(double), data.data(), sizeof(double) * data.size());
  return blob;
}

// The float32 form of the device block (pcg_rollout_policy_f32.hpp): the same header, then floats -- every value rounded to
// nearest, the rows of two consecutive units interleaved (element (r, k) at offW + ((r / 2) ld + k) 2 + (r & 1)), rows padded
// to an even count (POL_HB / POL_SB / POL32_OR), columns as in the fp64 form.  The header's clip box holds the rounded
// bounds.  Returned in doubles' worth of storage, so that create / update treat both forms alike.
// PCG_E_VALUE through *rc for a value that is not finite after rounding.
static std::vector<double> pack_policy_f32(const pcg_policy_cfg* c, int* rc) {
  auto up = [](int n, int m) { return (n + m - 1) / m * m; };
  *rc = PCG_OK;
  auto r32 = [&](double v) {
    const float f = (float)v;
    if (!std::isfinite(f)) *rc = PCG_E_VALUE;
    return f;
  };
  PolicyDev h;
  std::memset(&h, 0, sizeof(h));
  h.n_in = c->n_in; h.n_out = c->n_out; h.n_hidden = c->n_hidden; h.act = c->activation; h.out_map = c->out_map;
  h.out_lo = (double)(float)c->out_low; h.out_hi = (double)(float)c->out_high;
  if (c->out_map == PCG_POL_CLIP && !(std::isfinite(h.out_lo) && std::isfinite(h.out_hi))) *rc = PCG_E_VALUE;
  for (int l = 0; l < c->n_hidden; ++l) h.w[l] = c->width[l];
  std::vector<float> data;
  for (int l = 0; l <= c->n_hidden; ++l) {
    int rows, cols;
    policy_layer_dims(c, l, &rows, &cols);
    const bool outl = l == c->n_hidden;
    const int prow = outl ? POL32_OR : up(rows, l == 0 ? POL_HB : POL_SB);
    const int pcol = l == 0 ? up(cols, POL_IB) : up(cols, l == 1 ? POL_HB : POL_SB);
    h.ld[l] = pcol;
    h.offW[l] = (int32_t)data.size();
    data.resize(data.size() + (size_t)prow * pcol, 0.0f);
    for (int r = 0; r < rows; ++r)
      for (int k = 0; k < cols; ++k)
        data[(size_t)h.offW[l] + ((size_t)(r / 2) * pcol + k) * 2 + (r & 1)] = r32(c->W[l][(size_t)r * cols + k]);
    h.offb[l] = (int32_t)data.size();
    data.resize(data.size() + (size_t)prow, 0.0f);
    for (int r = 0; r < rows; ++r) data[(size_t)h.offb[l] + r] = r32(c->b[l][r]);
  }
  // (slack as in the fp64 form: no scalar fetch ends outside the block)
  const size_t words = (data.size() + 32 + 1) / 2;
  std::vector<double> blob(sizeof(PolicyDev) / sizeof(double) + words, 0.0);
  std::memcpy(blob.data(), &h, sizeof(h));
  std::memcpy(blob.data() + sizeof(PolicyDev) / sizeof(double), data.data(), sizeof(float) * data.size());
  return blob;
}

static int policy_create(pcg_policy** out, const pcg_policy_cfg* cfg, int dtype) {
  if (!out) return PCG_E_NULL;
  *out = nullptr;
  PCG_TRY(pcg_policy_validate(cfg));
  int prc = PCG_OK;
  const std::vector<double> blob = dtype == PCG_POL_F32 ? pack_policy_f32(cfg, &prc) : pack_policy(cfg);
  PCG_TRY(prc);
  pcg_policy* q = new (std::nothrow) pcg_policy();
  if (!q) return (int)hipErrorOutOfMemory;
  q->dtype = dtype;
  q->n_in = cfg->n_in; q->n_out = cfg->n_out;
  q->n_hidden = cfg->n_hidden; q->out_map = cfg->out_map;
  for (int l = 0; l < 2; ++l) q->width[l] = l < cfg->n_hidden ? cfg->width[l] : 0;
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

int pcg_policy_create(pcg_policy** out, const pcg_policy_cfg* cfg) { return policy_create(out, cfg, PCG_POL_F64); }
int pcg_policy_create_f32(pcg_policy** out, const pcg_policy_cfg* cfg) { return policy_create(out, cfg, PCG_POL_F32); }

int pcg_policy_dtype(const pcg_policy* q) {
  if (!q) return PCG_E_NULL;
  if (q->magic != POLICY_MAGIC) return PCG_E_PLAN;
  return q->dtype;
}

int pcg_policy_update(pcg_policy* q, const pcg_policy_cfg* cfg) {
  if (!q) return PCG_E_NULL;
  if (q->magic != POLICY_MAGIC) return PCG_E_PLAN;
  PCG_TRY(pcg_policy_validate(cfg));
  if (cfg->n_in != q->n_in || cfg->n_out != q->n_out || cfg->n_hidden != q->n_hidden) return PCG_E_DIM;
  for (int l = 0; l < cfg->n_hidden; ++l)
    if (cfg->width[l] != q->width[l]) return PCG_E_DIM;
  int prc = PCG_OK;
  const std::vector<double> blob = q->dtype == PCG_POL_F32 ? pack_policy_f32(cfg, &prc) : pack_policy(cfg);
  PCG_TRY(prc);
  if (blob.size() != q->blob_doubles) return PCG_E_DIM;  // (cannot happen: the block's size is a function of the shape)
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != q->device) HIP_TRY(hipSetDevice(q->device));
  hipError_t e = hipMemcpy(q->dP, blob.data(), sizeof(double) * blob.size(), hipMemcpyHostToDevice);
  if (dev != q->device) {
    const hipError_t e2 = hipSetDevice(dev);
    if (e == hipSuccess) e = e2;
  }
  if (e == hipSuccess) q->out_map = cfg->out_map;
  return (int)e;
}

int pcg_policy_destroy(pcg_policy* q) {
  if (!q) return PCG_OK;
  if (q->magic != POLICY_MAGIC) return PCG_E_PLAN;
  q->magic = 0;
  const hipError_t e = hipFree(q->dP);
  delete q;
  return (int)e;
}

// ---- a population of policies of one shape (pcg_rollout_pop.hpp) ---------------------------------------------------------
struct pcg_policy_pop {
  uint32_t magic;
  int device;
  int32_t P;
  int n_in, n_out, n_hidden, width[2];  // the shape every member has, and pcg_policy_pop_update holds a new cfg against
  int act, out_map;                     // ... with the activation, the output map and its box: members differ in weights alone
  double out_lo, out_hi;
  size_t blob_doubles;                  // size of ONE member's block (pack_policy's / pack_policy_f32's): the stride between members
  double* dP;                           // P member blocks, one allocation
  int dtype;                            // PCG_POL_F64 | PCG_POL_F32: which packing every block holds (as pcg_policy::dtype)
  PopLayout lay;                        // where the flat parameters of a member live in its block (pcg_pop_search.hpp)
};
static constexpr uint32_t POP_MAGIC = 0x50434751u;  // 'PCGQ'

// the cfg of member m of `count` consecutive ones behind a validated-in-shape cfg (member-major matrices and biases)
static pcg_policy_cfg pop_member_cfg(const pcg_policy_cfg* c, int64_t m) {
  pcg_policy_cfg one = *c;
  for (int l = 0; l <= c->n_hidden; ++l) {
    int rows, cols;
    policy_layer_dims(c, l, &rows, &cols);
    one.W[l] = c->W[l] + (size_t)m * rows * cols;
    one.b[l] = c->b[l] + (size_t)m * rows;
  }
  return one;
}

// The flat parameter order of a member (pcg_pop_search.hpp) against the block pack_policy wrote for it: W[l] row-major, then
// b[l], layer by layer; offsets in elements from the block's start: doubles, or floats for pack_policy_f32's block, whose
// header counts offW / offb in floats.
static PopLayout pop_layout(const pcg_policy_cfg* c, const double* block, int dtype) {
  static_assert(sizeof(PolicyDev) % sizeof(double) == 0, "the weights behind the header are aligned for pair loads");
  PolicyDev h;
  std::memcpy(&h, block, sizeof(h));
  const int HDR = (int)(sizeof(PolicyDev) / (dtype == PCG_POL_F32 ? sizeof(float) : sizeof(double)));
  PopLayout L;
  std::memset(&L, 0, sizeof(L));
  L.f32 = dtype == PCG_POL_F32 ? 1 : 0;
  L.nl = c->n_hidden + 1;
  int n = 0;
  for (int l = 0; l <= c->n_hidden; ++l) {
    int rows, cols;
    policy_layer_dims(c, l, &rows, &cols);
    L.start[l] = n;
    L.rows[l] = rows;
    L.cols[l] = cols;
    L.ld[l] = h.ld[l];
    L.offW[l] = HDR + h.offW[l];
    L.offb[l] = HDR + h.offb[l];
    n += rows * (cols + 1);
  }
  for (int l = c->n_hidden + 1; l < 4; ++l) L.start[l] = n;
  L.n = n;
  return L;
}

// pcg_policy_validate's rules for each of `count` members (the first member's status decides the shape), host only
static int pop_validate(const pcg_policy_cfg* cfg, int64_t count) {
  if (!cfg) return PCG_E_NULL;
  if (count < 1) return PCG_E_DIM;
  PCG_TRY(pcg_policy_validate(cfg));
  for (int64_t m = 1; m < count; ++m) {
    const pcg_policy_cfg one = pop_member_cfg(cfg, m);
    PCG_TRY(pcg_policy_validate(&one));
  }
  return PCG_OK;
}

// the blocks of `count` members, back to back (a block is whole doubles in either form: a byte stride that is a multiple
// of 8).  *rc: PCG_E_VALUE when a member of a float32 population is not finite after rounding -- every member is judged.
static std::vector<double> pack_pop(const pcg_policy_cfg* cfg, int64_t count, int dtype, size_t* member_doubles, int* rc) {
  std::vector<double> all;
  *rc = PCG_OK;
  for (int64_t m = 0; m < count; ++m) {
    const pcg_policy_cfg one = pop_member_cfg(cfg, m);
    int prc = PCG_OK;
    const std::vector<double> blob = dtype == PCG_POL_F32 ? pack_policy_f32(&one, &prc) : pack_policy(&one);
    if (prc != PCG_OK) *rc = prc;
    *member_doubles = blob.size();
    all.insert(all.end(), blob.begin(), blob.end());
  }
  return all;
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
  q->n_in = cfg->n_in; q->n_out = cfg->n_out; q->n_hidden = cfg->n_hidden;
  for (int l = 0; l < 2; ++l) q->width[l] = l < cfg->n_hidden ? cfg->width[l] : 0;
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

int pcg_policy_pop_create(pcg_policy_pop** out, const pcg_policy_cfg* cfg, int32_t P) { return pop_create(out, cfg, P, PCG_POL_F64); }
int pcg_policy_pop_create_f32(pcg_policy_pop** out, const pcg_policy_cfg* cfg, int32_t P) { return pop_create(out, cfg, P, PCG_POL_F32); }

int pcg_policy_pop_dtype(const pcg_policy_pop* q) {
  if (!q) return PCG_E_NULL;
  if (q->magic != POP_MAGIC) return PCG_E_PLAN;
  return q->dtype;
}

int pcg_policy_pop_update(pcg_policy_pop* q, const pcg_policy_cfg* cfg, int32_t first, int32_t count) {
  if (!q) return PCG_E_NULL;
  if (q->magic != POP_MAGIC) return PCG_E_PLAN;
  PCG_TRY(pop_validate(cfg, count));
  if (first < 0 || (int64_t)first + count > q->P) return PCG_E_DIM;
  if (cfg->n_in != q->n_in || cfg->n_out != q->n_out || cfg->n_hidden != q->n_hidden) return PCG_E_DIM;
  for (int l = 0; l < cfg->n_hidden; ++l)
    if (cfg->width[l] != q->width[l]) return PCG_E_DIM;
  if (cfg->activation != q->act || cfg->out_map != q->out_map) return PCG_E_VALUE;
  const bool f32 = q->dtype == PCG_POL_F32;
  const double lo = f32 ? (double)(float)cfg->out_low : cfg->out_low, hi = f32 ? (double)(float)cfg->out_high : cfg->out_high;
  if (cfg->out_map == PCG_POL_CLIP && (lo != q->out_lo || hi != q->out_hi)) return PCG_E_VALUE;
  size_t member = 0;
  int prc = PCG_OK;
  const std::vector<double> all = pack_pop(cfg, count, q->dtype, &member, &prc);
  PCG_TRY(prc);  // (every member of the range was judged: no byte is copied)
  if (member != q->blob_doubles) return PCG_E_DIM;  // (cannot happen: the block's size is a function of the shape)
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != q->device) HIP_TRY(hipSetDevice(q->device));
  hipError_t e = hipMemcpy(q->dP + (size_t)first * member, all.data(), sizeof(double) * all.size(), hipMemcpyHostToDevice);
  if (dev != q->device) {
    const hipError_t e2 = hipSetDevice(dev);
    if (e == hipSuccess) e = e2;
  }
  return (int)e;
}

int pcg_policy_pop_size(const pcg_policy_pop* q) {
  if (!q) return PCG_E_NULL;
  if (q->magic != POP_MAGIC) return PCG_E_PLAN;
  return q->P;
}

// ---- the weights of a population written and read on the device (pcg_pop_search.hpp) -------------------------------------
// what all five decide first: a population, of the caller's current device
static int pop_search_open(const pcg_policy_pop* q) {
  if (q->magic != POP_MAGIC) return PCG_E_PLAN;
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

int pcg_policy_pop_nparams(const pcg_policy_pop* q) {
  if (!q) return PCG_E_NULL;
  if (q->magic != POP_MAGIC) return PCG_E_PLAN;
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
  if (q->magic != POP_MAGIC) return PCG_E_PLAN;
  q->magic = 0;
  const hipError_t e = hipFree(q->dP);
  delete q;
  return (int)e;
}

// All six closed-loop entry points (pcg_rollout_policy / pcg_rollout_actor, their _cons and _unc forms) validate through three
// functions, read top to bottom: closed_loop_open up to the policy's size, then the head's own (policy_head; actor_head: critic,
// tanh map, sigma), then closed_loop_launch from the step range on.  (closed_loop_launch is a template over the head's
// argument type: C++ linkage inside this file's extern "C".)
extern "C++" {
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

// Builds or loads the closed-loop module of a run-time compiled plan; a second call finds it there.
static int jit_prepare_closed_loop(pcg_plan* p) {
  if (__atomic_load_n(&p->jit_pol, __ATOMIC_ACQUIRE)) return PCG_OK;
  std::lock_guard<std::mutex> lk(g_jit_mu);
  if (p->jit_pol) return PCG_OK;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != p->device) HIP_TRY(hipSetDevice(p->device));  // (the module is loaded on the plan's device, as at creation)
  hipFunction_t pol = nullptr, act = nullptr;
  int rc = jit_closed_loop(*p->jit_src, p->device, &pol, &act);
  if (dev != p->device) {
    const hipError_t e = hipSetDevice(dev);
    if (rc == PCG_OK) rc = (int)e;
  }
  PCG_TRY(rc);
  p->jit_act = act;
  __atomic_store_n(&p->jit_pol, pol, __ATOMIC_RELEASE);
  return PCG_OK;
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
  if (q->magic != POLICY_MAGIC || q->device != p->device) return PCG_E_PLAN;
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
  if (q->n_in != c.nobs || q->n_out != c.na) return PCG_E_DIM;
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
    if (v->magic != POLICY_MAGIC || v->device != p->device) return PCG_E_PLAN;
    if (kind != ClosedLoopKind::base && v->dtype == PCG_POL_F32) return PCG_E_UNSUPPORTED;
    if (v->n_in != c.nobs || v->n_out != 1) return PCG_E_DIM;
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
}  // extern "C++"

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

// pcg_rollout_policy_pop's sibling of closed_loop_open, with its order of refusals: plan, buffers and handle; what the base
// kind's kernels do not carry; run-time compiled code (the population kernel is ahead-of-time only); the members' sizes; then
// what is the population's own -- the slices (whole waves per member, a member for every env) and gamma.
static int pop_open(pcg_plan* p, const pcg_buffers* io, const pcg_policy_pop* q, int64_t G, double gamma, StepArgs* a, const void** fn) {
  PCG_TRY(fill_args(p, io, a));
  if (!q) return PCG_E_NULL;
  if (q->magic != POP_MAGIC || q->device != p->device) return PCG_E_PLAN;
  const DevConst& c = p->hc;
  const int ls = lean_scheme(p->integrator_id);
  if (io->t || c.ncon > 0 || c.nunc > 0 || ls < 0) return PCG_E_UNSUPPORTED;
  if (p->jit_fn[0]) return PCG_E_UNSUPPORTED;
  *fn = (const void*)(q->dtype == PCG_POL_F32 ? kernels(p->kid).roll_policy_pop_f32 : kernels(p->kid).roll_policy_pop)[ls];
  if (!*fn) return PCG_E_UNSUPPORTED;
  if (q->n_in != c.nobs || q->n_out != c.na) return PCG_E_DIM;
  if (G < 64 || G % 64 != 0 || p->env_offset < 0 || p->env_offset % 64 != 0) return PCG_E_VALUE;
  if (io->B > 0 && (p->env_offset + io->B - 1) / G >= (int64_t)q->P) return PCG_E_DIM;
  if (!(std::isfinite(gamma) && gamma >= 0.0 && gamma <= 1.0)) return PCG_E_VALUE;
  return PCG_OK;
}

int pcg_rollout_policy_pop(pcg_plan* p, const pcg_buffers* io, const pcg_policy_pop* q, int64_t envs_per_policy, int32_t t0,
                           int32_t T, double* a_seq_out, int64_t a_step_stride, int64_t a_comp_stride, double* obs_seq,
                           int64_t obs_step_stride, int64_t obs_comp_stride, double* rew_seq, int64_t rew_step_stride,
                           int32_t record_next_action, double gamma, double* ret_out, uint64_t seed, void* stream) {
  StepArgs a;
  const void* fn;
  PCG_TRY(pop_open(p, io, q, envs_per_policy, gamma, &a, &fn));
  PopArgs pa;
  pa.blocks = (const PCG_CONSTANT char*)q->dP;
  pa.stride = (int64_t)(sizeof(double) * q->blob_doubles);
  pa.G = envs_per_policy;
  pa.a_out = a_seq_out; pa.ao_ss = a_step_stride; pa.ao_cs = a_comp_stride;
  pa.record_next = record_next_action ? 1 : 0;
  pa.gamma = gamma;
  pa.ret_out = ret_out;
  const ClosedLoopRun run{t0, T, obs_seq, obs_step_stride, obs_comp_stride, rew_seq, rew_step_stride, seed};
  return closed_loop_launch(p, io, a, fn, ClosedLoopKind::base, nullptr, pa, {{a_seq_out, a_comp_stride}}, run, PCG_OK, stream);
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

// two envs per lane with 16-byte accesses (2-byte for the flags): the rule of the lean kernels' tile I/O (step_lean, rollout_lean) --
// an even batch and every row 16-byte aligned, which here, with caller-given strides, asks for even strides as well
static bool gae_vec2_ok(int64_t B, int32_t T, const double* rew, int64_t rew_ss, const double* val, int64_t val_ss, const uint8_t* term,
                        int64_t term_ss, const double* adv, int64_t adv_ss, const double* ret, int64_t ret_ss) {
  const bool rows = T > 1;  // (a single row has no stride to speak of; val has T + 1 rows)
  return B % 2 == 0 && al16(rew) && al16(val) && al16(adv) && al16(ret) && al2(term) && val_ss % 2 == 0 &&
         (!rows || (rew_ss % 2 == 0 && adv_ss % 2 == 0 && (!ret || ret_ss % 2 == 0) && (!term || term_ss % 2 == 0)));
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

// ---- step graph: T pcg_step launches recorded once, replayed with one host call ------------------------------
struct pcg_graph {
  uint32_t magic;
  int device;
  hipGraph_t graph;
  hipGraphExec_t exec;
  int n_nodes;
  int slot_nodes, done_nodes;  // recorded steps that skip the observation's slot rows / the done bytes (pcg_graph_held)
  int chain_launches, chain_steps;  // chained launches and the recorded steps they cover (pcg_graph_chained)
  ChainStep* dchain;           // [T] device table of the chained steps (null without a chain): owned, freed with the graph
};
static constexpr uint32_t GRAPH_MAGIC = 0x50434747u;  // 'PCGG'

// What the step t of a lock-stepped lean plan would store again unchanged if it ran directly after step t - 1 on the same
// buffers (StepArgs::held): bit 0 -- the observation's set-point and disturbance slot rows, bitwise equal in the two steps'
// LeanStep records (memcmp: a NaN schedule value equals itself); bit 1 -- the done bytes, t + 1 == N - 1 in both or neither.
static int32_t held_rows(const pcg_plan* p, int32_t t) {
  const DevConst& c = p->hc;
  if (p->no_held || p->hlean.empty() || t < 1) return 0;
  const int last = (int)p->hlean.size() - 1;
  const LeanStep& L = p->hlean[(size_t)std::min(t, last)];
  const LeanStep& Lp = p->hlean[(size_t)std::min(t - 1, last)];
  const size_t nso = (size_t)std::min(std::max(c.nsp_obs, 0), PCG_MAX_NSP), nd = (size_t)std::min(std::max(c.nd, 0), PCG_MAX_NDM);
  int32_t held = 0;
  if (std::memcmp(L.osp, Lp.osp, sizeof(double) * nso) == 0 && std::memcmp(L.od, Lp.od, sizeof(double) * nd) == 0) held |= 1;
  if ((t + 1 == c.N - 1) == (t == c.N - 1)) held |= 2;
  return held;
}

// Rows that carry nothing new are not stored twice: a node that runs step_lean's pipelined kernel directly after another
// one that did skips the stores of held_rows().  Node 0 of the steps never skips anything, with or without with_reset (the
// reset kernel writes other slot values and no done bytes), so a replay does not depend on what the buffers held before
// it.  INVARIANT: after every recorded LAUNCH every buffer holds exactly the bytes the pcg_step loop leaves at that point --
// replays are bit-identical to T pcg_step calls.
// PCG_NO_HELD_ROWS (read at plan creation) records every store (A/B measurement, tests).
// A launch is one step, except for chains: a maximal run of at least two consecutive steps that would each take step_lean's
// pipelined RK4 kernel unforced (lean_pipe_rk4), without d_steps, is recorded as ONE launch of step_chain_kernel -- a tile's
// state stays in registers from the run's first step to its last, every step still stores its observation, reward and
// (unless held) slot rows and done bytes, the state goes back once.  Two envs per lane only if every step of the run would
// have had them (every a_steps[j] 16-byte aligned).  The held word of each step is held_rows() as before, chained or not,
// so pcg_graph_held counts the same steps.  The steps' action pointers and held words are a device table the graph owns,
// on the device before the capture begins; nothing is allocated or freed on the launch path.  PCG_NO_CHAIN (read at plan
// creation) records one launch per step (A/B measurement, the way back).  n_nodes keeps counting recorded steps (+ reset).
int pcg_graph_create(pcg_graph** out, pcg_plan* p, const pcg_buffers* io, const double* const* a_steps,
                     const double* const* d_steps, int32_t t0, int32_t T, uint64_t seed, int with_reset) {
  if (!out) return PCG_E_NULL;
  *out = nullptr;
  if (!plan_ok(p)) return PCG_E_PLAN;
  if (!io || !a_steps) return PCG_E_NULL;
  if (io->t || p->jit_fn[0]) return PCG_E_UNSUPPORTED;
  if (T <= 0 || t0 < 0 || io->B <= 0) return PCG_E_DIM;
  for (int j = 0; j < T; ++j)
    if (!a_steps[j] || (d_steps && !d_steps[j])) return PCG_E_NULL;
  pcg_buffers b = *io;
  // run[j]: steps in the chained launch that starts at step j (0: step j is a launch of its own, or inside a chain);
  // epl[j]: envs per lane - 1 of the pipelined kernel that would take step j alone, -1 where another kernel would
  std::vector<int> run((size_t)T, 0), epl((size_t)T, -1);
  int chain_launches = 0, chain_steps = 0;
  if (!p->no_chain && !d_steps)
    for (int j = 0; j < T; ++j) {
      b.a = a_steps[j];
      int e1 = 0;
      if (lean_pipe_rk4(p, &b, t0 + j, &e1)) epl[(size_t)j] = e1;
    }
  for (int j = 0; j < T;) {
    int n = 0;
    while (j + n < T && epl[(size_t)(j + n)] >= 0) ++n;
    if (n >= 2) {
      run[(size_t)j] = n;
      ++chain_launches;
      chain_steps += n;
    }
    j += n > 0 ? n : 1;
  }
  // the chained steps' table: filled and on the device BEFORE the capture begins; nothing is allocated on the launch path
  std::vector<ChainStep> hchain((size_t)T, ChainStep{nullptr, 0});
  ChainStep* dchain = nullptr;
  if (chain_launches > 0) {
    // (the route of the step ahead of step j: a chained step is the pipelined kernel's, as is one it would have taken alone)
    for (int j = 0; j < T; ++j) {
      hchain[(size_t)j].a = a_steps[j];
      hchain[(size_t)j].held = (j > 0 && epl[(size_t)(j - 1)] >= 0) ? held_rows(p, t0 + j) : 0;
    }
    HIP_TRY(hipMalloc((void**)&dchain, sizeof(ChainStep) * (size_t)T));
    const hipError_t ec = hipMemcpy(dchain, hchain.data(), sizeof(ChainStep) * (size_t)T, hipMemcpyHostToDevice);
    if (ec != hipSuccess) {
      (void)hipFree(dchain);
      return (int)ec;
    }
  }
  hipStream_t cs;
  hipError_t e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
  if (e == hipSuccess) {
    e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) (void)hipStreamDestroy(cs);
  }
  if (e != hipSuccess) {
    if (dchain) (void)hipFree(dchain);
    return (int)e;
  }
  int rc = PCG_OK;
  hipGraph_t g = nullptr;
  if (with_reset) rc = pcg_reset(p, &b, nullptr, seed, cs);
  int slot_nodes = 0, done_nodes = 0;
  StepRoute prev = ROUTE_NONE;
  for (int j = 0; j < T && rc == PCG_OK;) {
    const int n = run[(size_t)j];
    if (n >= 2) {  // steps j .. j + n - 1 as one launch; two envs per lane where every one of them would have had them
      int e1 = 1;
      for (int i = 0; i < n; ++i) e1 = std::min(e1, epl[(size_t)(j + i)]);
      b.a = a_steps[j];
      b.d = nullptr;
      rc = chain_launch(p, &b, t0 + j, seed, n, dchain + j, e1, cs);
      for (int i = 0; i < n; ++i) {
        slot_nodes += hchain[(size_t)(j + i)].held & 1;
        done_nodes += (hchain[(size_t)(j + i)].held >> 1) & 1;
      }
      prev = ROUTE_LEAN_PIPE;
      j += n;
      continue;
    }
    b.a = a_steps[j];
    b.d = d_steps ? d_steps[j] : nullptr;
    const int32_t held = (j > 0 && prev == ROUTE_LEAN_PIPE) ? held_rows(p, t0 + j) : 0;
    rc = step_impl(p, &b, t0 + j, seed, cs, false, 0, held, &prev);
    if (prev == ROUTE_LEAN_PIPE) {  // (any other route ignores `held`)
      slot_nodes += held & 1;
      done_nodes += (held >> 1) & 1;
    }
    ++j;
  }
  e = hipStreamEndCapture(cs, &g);
  (void)hipStreamDestroy(cs);
  hipGraphExec_t ex = nullptr;
  if (rc == PCG_OK && e == hipSuccess) {
    e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    if (e != hipSuccess) ex = nullptr;
  }
  pcg_graph* q = (rc == PCG_OK && e == hipSuccess) ? new (std::nothrow) pcg_graph() : nullptr;
  if (!q) {
    if (ex) (void)hipGraphExecDestroy(ex);
    if (g) (void)hipGraphDestroy(g);
    if (dchain) (void)hipFree(dchain);
    return rc != PCG_OK ? rc : e != hipSuccess ? (int)e : PCG_E_VALUE;
  }
  q->magic = GRAPH_MAGIC;
  q->device = p->device;
  q->graph = g;
  q->exec = ex;
  q->n_nodes = T + (with_reset ? 1 : 0);
  q->slot_nodes = slot_nodes;
  q->done_nodes = done_nodes;
  q->chain_launches = chain_launches;
  q->chain_steps = chain_steps;
  q->dchain = dchain;
  *out = q;
  return PCG_OK;
}

int pcg_graph_chained(const pcg_graph* q, int32_t* launches, int32_t* steps) {
  if (!q || q->magic != GRAPH_MAGIC) return PCG_E_PLAN;
  if (launches) *launches = q->chain_launches;
  if (steps) *steps = q->chain_steps;
  return PCG_OK;
}

int pcg_graph_held(const pcg_graph* q, int32_t* slot_nodes, int32_t* done_nodes) {
  if (!q || q->magic != GRAPH_MAGIC) return PCG_E_PLAN;
  if (slot_nodes) *slot_nodes = q->slot_nodes;
  if (done_nodes) *done_nodes = q->done_nodes;
  return PCG_OK;
}

int pcg_graph_launch(pcg_graph* q, void* stream) {
  if (!q || q->magic != GRAPH_MAGIC) return PCG_E_PLAN;
  return (int)hipGraphLaunch(q->exec, (hipStream_t)stream);
}

int pcg_graph_set_seed(pcg_graph* q, uint64_t seed) {
  if (!q || q->magic != GRAPH_MAGIC) return PCG_E_PLAN;
  size_t n = 0;
  HIP_TRY(hipGraphGetNodes(q->graph, nullptr, &n));
  std::vector<hipGraphNode_t> nodes(n);
  HIP_TRY(hipGraphGetNodes(q->graph, nodes.data(), &n));
  for (size_t i = 0; i < n; ++i) {
    hipGraphNodeType ty;
    HIP_TRY(hipGraphNodeGetType(nodes[i], &ty));
    if (ty != hipGraphNodeTypeKernel) continue;
    hipKernelNodeParams kp;
    HIP_TRY(hipGraphKernelNodeGetParams(nodes[i], &kp));
    if (!kp.kernelParams || !kp.kernelParams[0]) return PCG_E_UNSUPPORTED;
    // every kernel this library records takes one by-value StepArgs: re-key it in the graph and in the executable
    StepArgs a;
    std::memcpy(&a, kp.kernelParams[0], sizeof(a));
    a.seed = seed;
    void* argv[1] = {&a};
    kp.kernelParams = argv;
    kp.extra = nullptr;
    HIP_TRY(hipGraphKernelNodeSetParams(nodes[i], &kp));
    HIP_TRY(hipGraphExecKernelNodeSetParams(q->exec, nodes[i], &kp));
  }
  return PCG_OK;
}

int pcg_graph_destroy(pcg_graph* q) {
  if (!q) return PCG_OK;
  if (q->magic != GRAPH_MAGIC) return PCG_E_PLAN;
  (void)hipGraphExecDestroy(q->exec);
  (void)hipGraphDestroy(q->graph);
  if (q->dchain) (void)hipFree(q->dchain);
  q->magic = 0;
  delete q;
  return PCG_OK;
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
