// pcg_abi_jit.hip -- run-time compilation of user source (pcgym_hip.h: user_cons_src / user_reward_src / user_rhs_src).
// The general one-env-per-lane step kernel of the plan's model is instantiated from the library's own headers with the
// user's source spliced in as pcg_user_constraints / pcg_user_reward / pcg_user_rhs, compiled with hipRTC, loaded as
// a module.  A PCG_MODEL_USER plan has no ahead-of-time kernels at all: its module also carries the test hooks.
// Compiled code objects are looked up in the process, then on disk (pcg_jit_cache.hpp), then built with hipRTC.
#include "pcg_host.hpp"
#include "pcg_jit_cache.hpp"

#include <hip/hiprtc.h>

#include <array>
#include <sstream>

namespace pcg {

static std::mutex g_jit_mu;
static std::string g_jit_log;

// What every translation unit of a plan opens with: the user's macros, the kernel headers, the check that they are the ones
// this library was built from, and the user's source as pcg_user_rhs / pcg_user_constraints / pcg_user_reward.  The step
// module (jit_kernels) and the closed-loop module (jit_closed_loop) differ only in what follows it.
std::string jit_preamble(const pcg_env_cfg* cfg) {
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

int jit_kernels(const pcg_env_cfg* cfg, int kid, int device, JitModule* out) {
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

// Builds or loads the closed-loop module of a run-time compiled plan; a second call finds it there.
int jit_prepare_closed_loop(pcg_plan* p) {
  if (__atomic_load_n(&p->jit_pol, __ATOMIC_ACQUIRE)) return PCG_OK;
  std::lock_guard<std::mutex> lk(g_jit_mu);
  if (p->jit_pol) return PCG_OK;
  hipFunction_t pol = nullptr, act = nullptr;
  // (the module is loaded on the plan's device, as at creation)
  PCG_TRY(on_device(p->device, [&] { return jit_closed_loop(*p->jit_src, p->device, &pol, &act); }));
  p->jit_act = act;
  __atomic_store_n(&p->jit_pol, pol, __ATOMIC_RELEASE);
  return PCG_OK;
}

}  // namespace pcg

extern "C" const char* pcg_last_jit_log(void) { return pcg::g_jit_log.c_str(); }
