// Stand-alone timing of the GAE kernel (pc-gym_amd/csrc/pcg_gae.hpp) by depth of its load groups and by lane path, without the
// library or torch:
//
//   for d in 2 4 8; do hipcc --offload-arch=gfx950 -O3 -std=c++17 -DPCG_GAE_DEPTH=$d -o gae_depth_$d tools/gae_depth_bench.hip; done
//   ./gae_depth_2; ./gae_depth_4; ./gae_depth_8
//
// T = 59, B in {4096, 2^16, 2^20}, contiguous rows of zeros (the arithmetic does not depend on the data), both lane paths (the
// library takes two envs per lane on such arrays), with and without the flag rows; 20 timed launches after 5, device events,
// median and minimum; the rate is counted against 32 B per env step (33 with flags).  profiles/r17/gae_variants.txt.
#include "../pc-gym_amd/csrc/pcg_gae.hpp"

#include <algorithm>
#include <cstdio>
#include <vector>

#define CK(e)                                                                     \
  do {                                                                            \
    hipError_t _e = (e);                                                          \
    if (_e != hipSuccess) {                                                       \
      printf("HIP error %s at line %d\n", hipGetErrorString(_e), __LINE__);       \
      return 1;                                                                   \
    }                                                                             \
  } while (0)

int main() {
  using namespace pcg;
  const int T = 59;
  const int64_t Bmax = 1 << 20;
  double *rew, *val, *adv, *ret;
  uint8_t* term;
  CK(hipMalloc(&rew, sizeof(double) * T * Bmax));
  CK(hipMalloc(&val, sizeof(double) * (T + 1) * Bmax));
  CK(hipMalloc(&adv, sizeof(double) * T * Bmax));
  CK(hipMalloc(&ret, sizeof(double) * T * Bmax));
  CK(hipMalloc(&term, T * Bmax));
  CK(hipMemset(rew, 0, sizeof(double) * T * Bmax));
  CK(hipMemset(val, 0, sizeof(double) * (T + 1) * Bmax));
  CK(hipMemset(term, 0, T * Bmax));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int64_t B : {(int64_t)4096, (int64_t)65536, Bmax})
    for (int vec2 = 1; vec2 >= 0; --vec2)
      for (int flags = 0; flags < 2; ++flags) {
        GaeArgs a{};
        a.B = B;
        a.T = T;
        a.vec2 = vec2;
        a.gamma = 0.99;
        a.gl = 0.99 * 0.95;
        a.rew = rew;
        a.val = val;
        a.term = flags ? term : nullptr;
        a.adv = adv;
        a.ret = ret;
        a.rew_ss = a.val_ss = a.term_ss = a.adv_ss = a.ret_ss = B;
        const int64_t lanes = vec2 ? B / 2 : B;
        const unsigned grid = (unsigned)((lanes + GAE_BLOCK - 1) / GAE_BLOCK);
        std::vector<float> ms;
        for (int r = 0; r < 25; ++r) {
          CK(hipEventRecord(e0, 0));
          hipLaunchKernelGGL(gae_kernel, dim3(grid), dim3(GAE_BLOCK), 0, 0, a);
          CK(hipEventRecord(e1, 0));
          CK(hipEventSynchronize(e1));
          float t;
          CK(hipEventElapsedTime(&t, e0, e1));
          if (r >= 5) ms.push_back(t);
        }
        CK(hipGetLastError());
        std::sort(ms.begin(), ms.end());
        const double med = ms[ms.size() / 2];
        printf("depth=%d B=%8lld envs_per_lane=%d flags=%d  median %.4f ms  min %.4f  %.3f TB/s\n", GAE_DEPTH, (long long)B, vec2 + 1, flags, med,
               ms[0], (32.0 + flags) * B * T / (med * 1e-3) / 1e12);
      }
  return 0;
}
