// pcg_host.hpp -- what the host units of the C ABI share (pcg_abi.hip and its siblings pcg_abi_cfg.hip, pcg_abi_jit.hip,
// pcg_abi_step.hip, pcg_abi_policy.hip): the four handle structs and their checks, the two status macros, the coverage hook,
// the kernel table, and the declarations of the few functions that cross a unit boundary.  Internal and host only; the
// library is built with hidden visibility, so nothing here is exported.
#pragma once
#ifndef __HIPCC_RTC__

#include "pcg_kernels.hpp"
#include "pcg_policy_pack.hpp"

#include <mutex>
#include <set>
#include <string>

namespace pcg {
// what jit_kernels hands a plan: its first run-time compiled module
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
}  // namespace pcg

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
  int feat_occ[pcg::MAX_FEAT];  // resident workgroups per CU of the feature-masked kernels
  int q_bpc[2], q_tile[2]; // work-queue kernel [per_env_t]: resident workgroups per CU, tile slots (0 = no queue launch)
  int q_tile1[2];          // the largest tile with ONE workgroup per CU (Rodas4: launches that fit one tile per CU)
  // reference paths the tests select through the environment, read at creation: PCG_NO_FIXUP (guarded plans in one
  // launch), PCG_NO_FLAT (the single-kernel rollout), PCG_Q_FORCE_LEAN (the lean queue layout wherever it fits)
  // ... and PCG_NO_HELD_ROWS: recorded step graphs store every row in every node (pcg_graph_create; A/B)
  // ... and PCG_NO_CHAIN: they record every step as a launch of its own (A/B, and the way back should a chain misbehave)
  bool no_fixup, no_flat, q_force_lean, no_held, no_chain;
  int64_t env_offset;
  pcg::DevConst hc;       // host copy
  pcg::DevConst* dC;      // device copy
  double* dsched;    // [nsp+nd][N]
  pcg::LeanStep* dlean;   // [N] wave-uniform values of each lock-stepped step (inside the dsched allocation)
  std::vector<pcg::LeanStep> hlean;  // host copy of that table: pcg_graph_create compares consecutive steps' slot values
  int cfg_nu;        // na + ndm as the caller counts them
  hipFunction_t jit_fn[2];  // run-time compiled general step kernel with user expressions [per_env_t] (or null)
  hipFunction_t jit_integ, jit_rhs;  // PCG_MODEL_USER: the run-time compiled test hooks (pcg_integrate / pcg_rhs)
  hipFunction_t jit_roll;            // run-time compiled fused rollout of a plan with user expressions (or null)
  // the plan's SECOND module, the two closed-loop kernels: null until the first closed-loop call or
  // pcg_plan_prepare_closed_loop builds it from jit_src (written once, under g_jit_mu; read with acquire)
  hipFunction_t jit_pol, jit_act;
  pcg::JitSource* jit_src;                // a run-time compiled plan's preamble (null for a built-in plan)
  int nx;                   // states (the kernel table's for built-in models, the cfg's for PCG_MODEL_USER)
  // work space of the barrier-free rollout (pcg_rollout_flat.hpp): 4 counters + 2 x flat_cap indices, allocated at the first
  // rollout that takes that path (and again if a later batch is larger) -- the only plan state a launch still writes
  int32_t* flat_ws;
  int64_t flat_cap;
};

// closed-loop fused rollout with an on-device MLP policy (pcg_rollout_policy.hpp)
struct pcg_policy {
  uint32_t magic;
  int device;
  pcg::PolicyShape shape;  // what pcg_policy_update holds a new cfg against
  int out_map;             // the map pcg_rollout_actor asks for
  size_t blob_doubles;     // size of the device block
  pcg::PolicyDev* dP;  // header + packed weights; rewritten only by pcg_policy_update (same shape, same block)
  int dtype;      // PCG_POL_F64 | PCG_POL_F32: which packing the block holds, hence which kernel family reads it
};

// a population of policies of one shape (pcg_rollout_pop.hpp)
struct pcg_policy_pop {
  uint32_t magic;
  int device;
  int32_t P;
  pcg::PolicyShape shape;               // the shape every member has, and pcg_policy_pop_update holds a new cfg against
  int act, out_map;                     // ... with the activation, the output map and its box: members differ in weights alone
  double out_lo, out_hi;
  size_t blob_doubles;                  // size of ONE member's block (pack_policy's): the stride between members
  double* dP;                           // P member blocks, one allocation
  int dtype;                            // PCG_POL_F64 | PCG_POL_F32: which packing every block holds (as pcg_policy::dtype)
  pcg::PopLayout lay;                   // where the flat parameters of a member live in its block (pcg_pop_search.hpp)
};

// step graph: T pcg_step launches recorded once, replayed with one host call
struct pcg_graph {
  uint32_t magic;
  int device;
  hipGraph_t graph;
  hipGraphExec_t exec;
  int n_nodes;
  int slot_nodes, done_nodes;  // recorded steps that skip the observation's slot rows / the done bytes (pcg_graph_held)
  int chain_launches, chain_steps;  // chained launches and the recorded steps they cover (pcg_graph_chained)
  pcg::ChainStep* dchain;      // [T] device table of the chained steps (null without a chain): owned, freed with the graph
};

#ifndef PCG_SRC_HASH
#define PCG_SRC_HASH "unknown-build"  // the Makefile passes a digest of csrc/*.hpp, csrc/*.hip and include/pcgym_hip.h
#endif

#define HIP_TRY(expr)                         \
  do {                                         \
    hipError_t _e = (expr);                    \
    if (_e != hipSuccess) return (int)_e;      \
  } while (0)
#define PCG_TRY(expr)                          \
  do {                                         \
    const int _rc = (expr);                    \
    if (_rc != PCG_OK) return _rc;             \
  } while (0)

namespace pcg {

constexpr uint32_t PLAN_MAGIC = 0x50434731u;    // 'PCG1'
constexpr uint32_t POLICY_MAGIC = 0x50434750u;  // 'PCGP'
constexpr uint32_t POP_MAGIC = 0x50434751u;     // 'PCGQ'
constexpr uint32_t GRAPH_MAGIC = 0x50434747u;   // 'PCGG'
inline bool plan_ok(const pcg_plan* p) { return p && p->magic == PLAN_MAGIC; }
inline bool policy_ok(const pcg_policy* q) { return q && q->magic == POLICY_MAGIC; }
inline bool pop_ok(const pcg_policy_pop* q) { return q && q->magic == POP_MAGIC; }
inline bool graph_ok(const pcg_graph* q) { return q && q->magic == GRAPH_MAGIC; }

// Kernel-instantiation coverage (test infrastructure; off unless PCG_COVERAGE is set in the environment when the library is
// loaded).  Every launch site passes its kernel through cov(): with coverage on, the host function pointer (or, for a
// run-time compiled module, the hipFunction_t) is noted in a process-wide set.  pcg_coverage_names() turns the set into
// the kernels' mangled names -- the names tools/kernel_inventory.py reads out of this library's code objects -- so that
// the GPU suite can say which of the shipped instantiations it launched, test by test (tests/conftest.py).
inline bool cov_on() {
  static const bool on = std::getenv("PCG_COVERAGE") != nullptr;
  return on;
}
extern std::mutex g_cov_mu;                   // (the sets and their mutex: defined in pcg_abi.hip)
extern std::set<const void*> g_cov_fn;        // ahead-of-time kernels: host function pointers
extern std::set<hipFunction_t> g_cov_jit;     // run-time compiled kernels
template <class F>
inline F cov(F fn) {
  if (cov_on()) {
    std::lock_guard<std::mutex> g(g_cov_mu);
    g_cov_fn.insert((const void*)fn);
  }
  return fn;
}
inline hipFunction_t cov_jit(hipFunction_t fn) {
  if (cov_on()) {
    std::lock_guard<std::mutex> g(g_cov_mu);
    g_cov_jit.insert(fn);
  }
  return fn;
}

// Runs f() with `device` current: switched to only if another one is, restored afterwards, the first error wins.
template <class F>
inline int on_device(int device, F f) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != device) HIP_TRY(hipSetDevice(device));
  int rc = f();
  if (dev != device) {
    const hipError_t e = hipSetDevice(dev);
    if (rc == PCG_OK) rc = (int)e;
  }
  return rc;
}

inline bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }
inline bool al2(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 1u) == 0; }
inline unsigned grid_for(int64_t B, int block = BLOCK) { return (unsigned)((B + block - 1) / block); }

// Dynamic LDS one workgroup may ask for
constexpr size_t LDS_MAX = 160 * 1024;

// pcg_abi.hip: the one table of kernel instantiations per model (built in the pcg_inst_*.hip units); plan, buffers -> StepArgs
const Kernels& kernels(int id);
int fill_args(const pcg_plan* p, const pcg_buffers* io, StepArgs* a);

// pcg_abi_cfg.hip: cfg folding
int build_devconst(const pcg_env_cfg* c, DevConst* d, int* cfg_nu_out);
std::vector<LeanStep> lean_table(const DevConst& d, const pcg_env_cfg* c);
int kernel_id_for(const pcg_env_cfg* c);

// pcg_abi_jit.hip: run-time compilation
std::string jit_preamble(const pcg_env_cfg* cfg);
int jit_kernels(const pcg_env_cfg* cfg, int kid, int device, JitModule* out);
int jit_prepare_closed_loop(pcg_plan* p);

// pcg_abi_step.hip: launch geometry and the step routes
size_t sched_bytes(const DevConst& c);
bool lds_stages_on(const pcg_plan* p, const Kernels& k);
int classic_shape(const pcg_plan* p, const Kernels& k, bool lds_st, size_t* integ_lds);
int plan_geometry(pcg_plan* p);
int feat_pick(const pcg_plan* p, const Kernels& k, const pcg_buffers* io, int pe, bool lds_st, bool auto_reset);

}  // namespace pcg
#endif  // !__HIPCC_RTC__
