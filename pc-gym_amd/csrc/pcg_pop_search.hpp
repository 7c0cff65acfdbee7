// pcg_pop_search.hpp -- the weights of a policy population (pcg_policy_pop, pcg_rollout_pop.hpp) written and read ON the device:
// what surrounds pcg_rollout_policy_pop in a derivative-free search loop (cross-entropy search, evolution strategies), which
// until now drew every member on the host, validated and packed it member by member and sent it with a pageable copy --
// for 4096 members of 2 x 64 about 19 M host normals and 150 MB per generation around a 55 ms evaluation.
//
// Flat parameter order (the contract of all five entry points).  Parameter j of a member, 0 <= j < n, runs layer by layer:
// W[l] row-major (n_next x n_prev), then b[l]; n = sum_l rows_l (cols_l + 1).  Its place in the member's device block is
// pack_policy's (pcg_policy_pack.hpp): header + offW[l] + r ld[l] + k, header + offb[l] + r.  No kernel here writes the header or a
// padding entry: they keep what pcg_policy_pop_create put there (zeros, so that padding units stay exact zeros).
//
// Search noise (RNG contract, purpose RNG_SEARCH = 0x500).  For member m (the population's own index),
// parameter j, generation g:
//     q = antithetic ? m >> 1 : m
//     o = philox4x32_10(ctr = (q, j >> 2, g, RNG_SEARCH), key = (seed_lo, seed_hi))
//     (z0, z1) = box_muller_f32(o[0], o[1]) -> parameters 4b, 4b + 1      (b = j >> 2)
//     (z2, z3) = box_muller_f32(o[2], o[3]) -> parameters 4b + 2, 4b + 3
//     z(m, j)  = (double) of that float, negated (exactly) when antithetic and m is odd
// Variates past n in the last block are discarded.  One Philox block per lane and four parameters: the noise is never stored;
// pcg_policy_pop_noise_dot forms it again from the same keys.
//
// Kernels (all element-wise, no LDS, no atomics):
//   pop_sample_kernel      one lane per (member, block of four parameters): theta = mean[j] + std[j] * z, product and sum
//                          each rounded on their own.  blockIdx.x / threadIdx.x run over the blocks of ONE member, so that
//                          the lanes of a wave store consecutive entries of a matrix row; members are gridDim.y-strided.
//   pop_noise_dot_kernel   one lane per (chunk of POP_CHUNK members, block of four parameters): acc = 0; acc = acc + w z for
//                          ascending m (contraction off).  Only c0 of the counter changes between iterations; the member
//                          index and its weight are wave-uniform (a uniform load).  Under antithetic sampling the two
//                          members of a pair share one Philox block.
//   pop_chunk_sum_kernel   one lane per parameter: out[j] = 0.0 + partial[0][j] + partial[1][j] + ..., ascending.
//   pop_get_flat_kernel /  one lane per (row, parameter); an index outside [0, P) reads as a row of NaN.
//   pop_set_flat_kernel
// The summation order is fixed by the chunk size alone, never by the launch shape: the same bits for every grid.
//
// A float32 population (pcg_policy_pop_create_f32; blocks of pack_policy's float32 form) has siblings of the three kernels that touch
// the blocks: pop_sample_kernel_f32, pop_get_flat_kernel_f32, pop_set_flat_kernel_f32.  Same flat order, same keys, same fp64
// mean / std / theta; a parameter lives at a FLOAT offset, matrices with the rows of two consecutive units interleaved:
//     W (l, r, k) at  HDR + offW[l] + ((r / 2) ld[l] + k) 2 + (r & 1),   b (l, r) at  HDR + offb[l] + r      (HDR in floats)
// and is stored with one round-to-nearest conversion of the fp64 value the fp64 kernel would store (sample: the sum formed
// in fp64 first, so a float32 member is (float) of the fp64 population's under the same keys); get widens exactly.  The
// noise sum does not read the blocks: one kernel serves both kinds.
#pragma once

#include "pcg_policy_layout.hpp"  // PopLayout

namespace pcg {

// (RNG_SEARCH stands beside RNG_POLICY in pcg_rollout_actor.hpp)
constexpr int POP_CHUNK = 64;            // members per partial sum of pcg_policy_pop_noise_dot (PCG_POP_CHUNK)
constexpr int POP_BLOCK = 256;
constexpr int POP_MAX_GRID_Y = 32768;    // rows of the grid; the kernels stride over members / chunks / rows beyond it

// offset (doubles, from the block's start) of flat parameter j, 0 <= j < L.n
__device__ __forceinline__ int pop_param_offset(const PopLayout& L, int j) {
  int l = 0;
  if (L.nl > 1 && j >= L.start[1]) l = 1;
  if (L.nl > 2 && j >= L.start[2]) l = 2;
  const int local = j - L.start[l];
  const int cols = L.cols[l];
  const int nw = L.rows[l] * cols;
  if (local >= nw) return L.offb[l] + (local - nw);
  const int r = local / cols;
  return L.offW[l] + r * L.ld[l] + (local - r * cols);
}

// ... of a float32 population: offset in floats, the float32 form's interleaved rows
__device__ __forceinline__ int pop_param_offset_f32(const PopLayout& L, int j) {
  int l = 0;
  if (L.nl > 1 && j >= L.start[1]) l = 1;
  if (L.nl > 2 && j >= L.start[2]) l = 2;
  const int local = j - L.start[l];
  const int cols = L.cols[l];
  const int nw = L.rows[l] * cols;
  if (local >= nw) return L.offb[l] + (local - nw);
  const int r = local / cols;
  return L.offW[l] + ((r >> 1) * L.ld[l] + (local - r * cols)) * 2 + (r & 1);
}

// the four variates of block b for stream q (the float results of the two Box-Muller pairs)
__device__ __forceinline__ void pop_noise4(uint32_t q, uint32_t b, uint32_t g, uint32_t k0, uint32_t k1, float (&z)[4]) {
  uint32_t o[4];
  philox4x32_10(q, b, g, RNG_SEARCH, k0, k1, o);
  box_muller_f32(o[0], o[1], z[0], z[1]);
  box_muller_f32(o[2], o[3], z[2], z[3]);
}

struct PopSampleArgs {
  PopLayout L;
  double* blocks;   // member 0's block (floats behind it when L.f32)
  int64_t stride;   // elements (doubles, or floats when L.f32) between two members' blocks
  int32_t first, count, antithetic;
  uint32_t k0, k1, g;
  const double* mean;
  const double* std;
};

__global__ __launch_bounds__(POP_BLOCK) void pop_sample_kernel(const PopSampleArgs A) {
  const int b = (int)(blockIdx.x * POP_BLOCK + threadIdx.x);
  const int j0 = 4 * b;
  if (j0 >= A.L.n) return;
  double mu[4], sd[4];
  int off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool in = j0 + i < A.L.n;
    mu[i] = in ? A.mean[j0 + i] : 0.0;
    sd[i] = in ? A.std[j0 + i] : 0.0;
    off[i] = in ? pop_param_offset(A.L, j0 + i) : 0;
  }
  for (int64_t i = blockIdx.y; i < A.count; i += gridDim.y) {
    const uint32_t m = (uint32_t)(A.first + i);
    float z[4];
    pop_noise4(A.antithetic ? m >> 1 : m, (uint32_t)b, A.g, A.k0, A.k1, z);
    const bool neg = A.antithetic && (m & 1u);
    double* blk = A.blocks + (int64_t)m * A.stride;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (j0 + k < A.L.n) {
#pragma clang fp contract(off)
        const double zz = neg ? -(double)z[k] : (double)z[k];
        const double pr = sd[k] * zz;
        blk[off[k]] = mu[k] + pr;
      }
    }
  }
}

// the float32 sibling: the same fp64 sum, stored with one round-to-nearest conversion (an overflow is stored as +-inf)
__global__ __launch_bounds__(POP_BLOCK) void pop_sample_kernel_f32(const PopSampleArgs A) {
  const int b = (int)(blockIdx.x * POP_BLOCK + threadIdx.x);
  const int j0 = 4 * b;
  if (j0 >= A.L.n) return;
  double mu[4], sd[4];
  int off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool in = j0 + i < A.L.n;
    mu[i] = in ? A.mean[j0 + i] : 0.0;
    sd[i] = in ? A.std[j0 + i] : 0.0;
    off[i] = in ? pop_param_offset_f32(A.L, j0 + i) : 0;
  }
  for (int64_t i = blockIdx.y; i < A.count; i += gridDim.y) {
    const uint32_t m = (uint32_t)(A.first + i);
    float z[4];
    pop_noise4(A.antithetic ? m >> 1 : m, (uint32_t)b, A.g, A.k0, A.k1, z);
    const bool neg = A.antithetic && (m & 1u);
    float* blk = reinterpret_cast<float*>(A.blocks) + (int64_t)m * A.stride;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (j0 + k < A.L.n) {
#pragma clang fp contract(off)
        const double zz = neg ? -(double)z[k] : (double)z[k];
        const double pr = sd[k] * zz;
        const double th = mu[k] + pr;
        blk[off[k]] = (float)th;
      }
    }
  }
}

struct PopDotArgs {
  int32_t n;
  int32_t first, count, antithetic;
  uint32_t k0, k1, g;
  const double* w;   // [count]
  double* partial;   // [ceil(count / POP_CHUNK)][n]
  double* out;       // [n]
};

__global__ __launch_bounds__(POP_BLOCK) void pop_noise_dot_kernel(const PopDotArgs A) {
  const int b = (int)(blockIdx.x * POP_BLOCK + threadIdx.x);
  const int j0 = 4 * b;
  if (j0 >= A.n) return;
  const int64_t chunks = ((int64_t)A.count + POP_CHUNK - 1) / POP_CHUNK;
  for (int64_t c = blockIdx.y; c < chunks; c += gridDim.y) {
    const int64_t i0 = c * POP_CHUNK;
    const int len = (int)(A.count - i0 < POP_CHUNK ? A.count - i0 : POP_CHUNK);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t q_have = 0;
    for (int i = 0; i < len; ++i) {
      // (m, q and w are the same in every lane: the branch is uniform and the weight a uniform load)
      const uint32_t m = (uint32_t)(A.first + i0 + i);
      const uint32_t q = A.antithetic ? m >> 1 : m;
      if (i == 0 || q != q_have) {
        pop_noise4(q, (uint32_t)b, A.g, A.k0, A.k1, z);
        q_have = q;
      }
      const double w = A.w[i0 + i];
      const bool neg = A.antithetic && (m & 1u);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma clang fp contract(off)
        const double zz = neg ? -(double)z[k] : (double)z[k];
        const double pr = w * zz;
        acc[k] = acc[k] + pr;
      }
    }
    double* p = A.partial + c * (int64_t)A.n + j0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (j0 + k < A.n) p[k] = acc[k];
  }
}

__global__ __launch_bounds__(POP_BLOCK) void pop_chunk_sum_kernel(const PopDotArgs A) {
  const int j = (int)(blockIdx.x * POP_BLOCK + threadIdx.x);
  if (j >= A.n) return;
  const int64_t chunks = ((int64_t)A.count + POP_CHUNK - 1) / POP_CHUNK;
  double acc = 0.0;
  for (int64_t c = 0; c < chunks; ++c) acc = acc + A.partial[c * (int64_t)A.n + j];
  A.out[j] = acc;
}

struct PopFlatArgs {
  PopLayout L;
  double* blocks;          // (floats behind it when L.f32)
  int64_t stride;          // elements (doubles, or floats when L.f32) between two members' blocks
  int32_t P, first, count;
  const int32_t* members;  // get: [count] member indices (device), or null for first + i
  double* theta;           // [count][theta_stride]
  int64_t theta_stride;
};

__global__ __launch_bounds__(POP_BLOCK) void pop_get_flat_kernel(const PopFlatArgs A) {
  const int j = (int)(blockIdx.x * POP_BLOCK + threadIdx.x);
  if (j >= A.L.n) return;
  const int off = pop_param_offset(A.L, j);
  for (int64_t i = blockIdx.y; i < A.count; i += gridDim.y) {
    const int64_t m = A.members ? (int64_t)A.members[i] : (int64_t)A.first + i;
    const bool ok = m >= 0 && m < A.P;
    A.theta[i * A.theta_stride + j] = ok ? A.blocks[m * A.stride + off] : __builtin_nan("");
  }
}

__global__ __launch_bounds__(POP_BLOCK) void pop_set_flat_kernel(const PopFlatArgs A) {
  const int j = (int)(blockIdx.x * POP_BLOCK + threadIdx.x);
  if (j >= A.L.n) return;
  const int off = pop_param_offset(A.L, j);
  for (int64_t i = blockIdx.y; i < A.count; i += gridDim.y) {
    const int64_t m = (int64_t)A.first + i;  // (inside [0, P): checked on the host)
    A.blocks[m * A.stride + off] = A.theta[i * A.theta_stride + j];
  }
}

// the float32 siblings: the stored float widened exactly / theta rounded to nearest
__global__ __launch_bounds__(POP_BLOCK) void pop_get_flat_kernel_f32(const PopFlatArgs A) {
  const int j = (int)(blockIdx.x * POP_BLOCK + threadIdx.x);
  if (j >= A.L.n) return;
  const int off = pop_param_offset_f32(A.L, j);
  const float* blocks = reinterpret_cast<const float*>(A.blocks);
  for (int64_t i = blockIdx.y; i < A.count; i += gridDim.y) {
    const int64_t m = A.members ? (int64_t)A.members[i] : (int64_t)A.first + i;
    const bool ok = m >= 0 && m < A.P;
    A.theta[i * A.theta_stride + j] = ok ? (double)blocks[m * A.stride + off] : __builtin_nan("");
  }
}

__global__ __launch_bounds__(POP_BLOCK) void pop_set_flat_kernel_f32(const PopFlatArgs A) {
  const int j = (int)(blockIdx.x * POP_BLOCK + threadIdx.x);
  if (j >= A.L.n) return;
  const int off = pop_param_offset_f32(A.L, j);
  float* blocks = reinterpret_cast<float*>(A.blocks);
  for (int64_t i = blockIdx.y; i < A.count; i += gridDim.y) {
    const int64_t m = (int64_t)A.first + i;  // (inside [0, P): checked on the host)
    blocks[m * A.stride + off] = (float)A.theta[i * A.theta_stride + j];
  }
}

}  // namespace pcg
