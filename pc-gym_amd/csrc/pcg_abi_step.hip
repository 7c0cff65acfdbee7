// pcg_abi_step.hip -- everything that launches the plan's own kernels: launch geometry (settled at plan creation), the routes
// of pcg_step, the open-loop fused rollouts, the recorded step graphs, and the work-queue sort's test hook.
#include "pcg_host.hpp"
#include "pcg_step_feat.hpp"

#include <algorithm>

using namespace pcg;

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

namespace pcg {

// ---- launch geometry ------------------------------------------------------------------------------------------
// the budget of the work-queue kernels' workgroups on one CU (2 KB below what one workgroup may ask for)
constexpr size_t LDS_CU = LDS_MAX - 2048;

// the plan's schedule rows (set points, disturbances), as per-env-t kernels stage them in LDS
size_t sched_bytes(const DevConst& c) { return sizeof(double) * (size_t)(c.nsp + c.nd) * c.N; }
// ... what a per-env-t launch stages behind `integ` bytes of the integrator's own LDS (0: they stay in HBM)
static size_t sched_in_lds_bytes(const DevConst& c, size_t integ) {
  const size_t sb = sched_bytes(c);
  return sb > 0 && integ + sb <= (integ > 48 * 1024 ? LDS_MAX : 64 * 1024) ? sb : 0;
}

bool lds_stages_on(const pcg_plan* p, const Kernels& k) {
  return p->lds_stages && p->integrator_id == PCG_INT_DOPRI5 && k.has_lds_stages;
}
// workgroup size of the plan's one-env-per-lane kernels, and the dynamic LDS their integrator needs (*integ_lds)
int classic_shape(const pcg_plan* p, const Kernels& k, bool lds_st, size_t* integ_lds) {
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
int plan_geometry(pcg_plan* p) {
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
int feat_pick(const pcg_plan* p, const Kernels& k, const pcg_buffers* io, int pe, bool lds_st, bool auto_reset) {
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

}  // namespace pcg

extern "C" {

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

int pcg_step(pcg_plan* p, const pcg_buffers* io, int32_t t, uint64_t seed, void* stream) {
  return step_impl(p, io, t, seed, stream, false, 0);
}

int pcg_step_autoreset(pcg_plan* p, const pcg_buffers* io, int32_t t, uint64_t seed, uint64_t reset_seed, void* stream) {
  if (plan_ok(p) && io && p->hc.nunc > 0 && !io->p_unc) return PCG_E_NULL;
  return step_impl(p, io, t, seed, stream, true, reset_seed);
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

// ---- step graph: T pcg_step launches recorded once, replayed with one host call ------------------------------
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
  if (!graph_ok(q)) return PCG_E_PLAN;
  if (launches) *launches = q->chain_launches;
  if (steps) *steps = q->chain_steps;
  return PCG_OK;
}

int pcg_graph_held(const pcg_graph* q, int32_t* slot_nodes, int32_t* done_nodes) {
  if (!graph_ok(q)) return PCG_E_PLAN;
  if (slot_nodes) *slot_nodes = q->slot_nodes;
  if (done_nodes) *done_nodes = q->done_nodes;
  return PCG_OK;
}

int pcg_graph_launch(pcg_graph* q, void* stream) {
  if (!graph_ok(q)) return PCG_E_PLAN;
  return (int)hipGraphLaunch(q->exec, (hipStream_t)stream);
}

int pcg_graph_set_seed(pcg_graph* q, uint64_t seed) {
  if (!graph_ok(q)) return PCG_E_PLAN;
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
  if (!graph_ok(q)) return PCG_E_PLAN;
  (void)hipGraphExecDestroy(q->exec);
  (void)hipGraphDestroy(q->graph);
  if (q->dchain) (void)hipFree(q->dchain);
  q->magic = 0;
  delete q;
  return PCG_OK;
}

}  // extern "C"
