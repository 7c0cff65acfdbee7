// pcg_policy_pack.hpp -- a policy cfg (include/pcgym_hip.h) into the device block the closed-loop kernels read: validation,
// the shape record of a handle, the packer of both element types, and a population's members and flat layout.  Host only,
// the ABI header, the layout header and the standard library alone -- no HIP -- so that tools/hostcheck/host_code_check.cpp
// holds every index formula against the packed bytes under sanitizers.
#pragma once
#ifndef __HIPCC_RTC__

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "pcg_policy_layout.hpp"

namespace pcg {

// layer l of a validated cfg: (rows, columns)
inline void policy_layer_dims(const pcg_policy_cfg* c, int l, int* rows, int* cols) {
  *cols = l == 0 ? c->n_in : c->width[l - 1];
  *rows = l == c->n_hidden ? c->n_out : c->width[l];
}

// pcg_policy_validate
inline int policy_validate(const pcg_policy_cfg* c) {
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

// The shape a handle's block was packed for: what pcg_policy_update / pcg_policy_pop_update hold a new cfg against (widths
// past n_hidden are zero).
struct PolicyShape {
  int n_in, n_out, n_hidden, width[2];
  static PolicyShape from_cfg(const pcg_policy_cfg* c) {
    return PolicyShape{c->n_in, c->n_out, c->n_hidden, {c->n_hidden > 0 ? c->width[0] : 0, c->n_hidden > 1 ? c->width[1] : 0}};
  }
  bool matches(const pcg_policy_cfg* c) const {
    if (c->n_in != n_in || c->n_out != n_out || c->n_hidden != n_hidden) return false;
    for (int l = 0; l < c->n_hidden; ++l)
      if (c->width[l] != width[l]) return false;
    return true;
  }
};

// What differs between the two forms of a policy's device block: the element type, where element (r, k) of a matrix with
// padded row length ld goes, the padded rows of the output layer, the slack behind the data, the rounding of a stored value.
struct PackF64 {  // pcg_rollout_policy.hpp: doubles, rows plain
  using T = double;
  static constexpr int OUT_ROWS = PCG_MAX_NA;
  static constexpr size_t SLACK = 16;
  static size_t at(int r, int k, int ld) { return (size_t)r * ld + k; }
  static double round(double v) { return v; }
};
struct PackF32 {  // pcg_rollout_policy_f32.hpp: floats rounded to nearest, the rows of two consecutive units interleaved
  using T = float;
  static constexpr int OUT_ROWS = POL32_OR;
  static constexpr size_t SLACK = 32;
  static size_t at(int r, int k, int ld) { return ((size_t)(r / 2) * ld + k) * 2 + (r & 1); }
  static float round(double v) { return (float)v; }
};

// The device block of a policy: header, then every layer's matrix and bias padded with zeros to the block sizes the
// kernels unroll by -- rows of a hidden layer to POL_HB (fed by the observation) or POL_SB (streamed), rows of the output
// layer to F::OUT_ROWS, columns to POL_IB (observation) or POL_HB / POL_SB (hidden units).  The header counts offW / offb in
// elements (doubles or floats) and holds the clip box as stored, i.e. rounded; the block itself is whole doubles in either
// form, so that create / update treat both alike.  PCG_E_VALUE through *rc for a value that is not finite after rounding.
template <class F>
inline std::vector<double> pack_policy_as(const pcg_policy_cfg* c, int* rc) {
  static_assert(POL_MAX_W == PCG_POL_MAX_WIDTH && POL_MAX_W % POL_HB == 0 && POL_HB % POL_SB == 0, "policy block sizes");
  using T = typename F::T;
  auto up = [](int n, int m) { return (n + m - 1) / m * m; };
  auto stored = [&](double v) {
    const T s = F::round(v);
    if (!std::isfinite(s)) *rc = PCG_E_VALUE;
    return s;
  };
  PolicyDev h;
  std::memset(&h, 0, sizeof(h));
  h.n_in = c->n_in; h.n_out = c->n_out; h.n_hidden = c->n_hidden; h.act = c->activation; h.out_map = c->out_map;
  h.out_lo = (double)F::round(c->out_low); h.out_hi = (double)F::round(c->out_high);
  if (c->out_map == PCG_POL_CLIP && !(std::isfinite(h.out_lo) && std::isfinite(h.out_hi))) *rc = PCG_E_VALUE;
  for (int l = 0; l < c->n_hidden; ++l) h.w[l] = c->width[l];
  std::vector<T> data;
  for (int l = 0; l <= c->n_hidden; ++l) {
    int rows, cols;
    policy_layer_dims(c, l, &rows, &cols);
    const bool outl = l == c->n_hidden;
    const int prow = outl ? F::OUT_ROWS : up(rows, l == 0 ? POL_HB : POL_SB);
    const int pcol = l == 0 ? up(cols, POL_IB) : up(cols, l == 1 ? POL_HB : POL_SB);
    h.ld[l] = pcol;
    h.offW[l] = (int32_t)data.size();
    data.resize(data.size() + (size_t)prow * pcol, T(0));
    for (int r = 0; r < rows; ++r)
      for (int k = 0; k < cols; ++k) data[(size_t)h.offW[l] + F::at(r, k, pcol)] = stored(c->W[l][(size_t)r * cols + k]);
    h.offb[l] = (int32_t)data.size();
    data.resize(data.size() + (size_t)prow, T(0));
    for (int r = 0; r < rows; ++r) data[(size_t)h.offb[l] + r] = stored(c->b[l][r]);
  }
  // (one scalar load may fetch up to sixteen words: the block ends in slack, so that no fetch ends outside it)
  const size_t words = (sizeof(T) * (data.size() + F::SLACK) + sizeof(double) - 1) / sizeof(double);
  std::vector<double> blob(sizeof(PolicyDev) / sizeof(double) + words, 0.0);
  std::memcpy(blob.data(), &h, sizeof(h));
  std::memcpy(blob.data() + sizeof(PolicyDev) / sizeof(double), data.data(), sizeof(T) * data.size());
  return blob;
}
inline std::vector<double> pack_policy(const pcg_policy_cfg* c, int dtype, int* rc) {
  *rc = PCG_OK;
  return dtype == PCG_POL_F32 ? pack_policy_as<PackF32>(c, rc) : pack_policy_as<PackF64>(c, rc);
}

// the cfg of member m of `count` consecutive ones behind a validated-in-shape cfg (member-major matrices and biases)
inline pcg_policy_cfg pop_member_cfg(const pcg_policy_cfg* c, int64_t m) {
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
// b[l], layer by layer; offsets in elements from the block's start: doubles, or floats for a float32 block, whose header
// counts offW / offb in floats.
inline PopLayout pop_layout(const pcg_policy_cfg* c, const double* block, int dtype) {
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
inline int pop_validate(const pcg_policy_cfg* cfg, int64_t count) {
  if (!cfg) return PCG_E_NULL;
  if (count < 1) return PCG_E_DIM;
  int rc = policy_validate(cfg);
  for (int64_t m = 1; m < count && rc == PCG_OK; ++m) {
    const pcg_policy_cfg one = pop_member_cfg(cfg, m);
    rc = policy_validate(&one);
  }
  return rc;
}

// the blocks of `count` members, back to back (a block is whole doubles in either form: a byte stride that is a multiple
// of 8).  *rc: PCG_E_VALUE when a member of a float32 population is not finite after rounding -- every member is judged.
inline std::vector<double> pack_pop(const pcg_policy_cfg* cfg, int64_t count, int dtype, size_t* member_doubles, int* rc) {
  std::vector<double> all;
  *rc = PCG_OK;
  for (int64_t m = 0; m < count; ++m) {
    const pcg_policy_cfg one = pop_member_cfg(cfg, m);
    int prc = PCG_OK;
    const std::vector<double> blob = pack_policy(&one, dtype, &prc);
    if (prc != PCG_OK) *rc = prc;
    *member_doubles = blob.size();
    all.insert(all.end(), blob.begin(), blob.end());
  }
  return all;
}

}  // namespace pcg
#endif  // !__HIPCC_RTC__
