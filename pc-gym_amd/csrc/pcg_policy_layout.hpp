// pcg_policy_layout.hpp -- the layout of a policy's device block, as the host packs it (pcg_policy_pack.hpp) and four kernel
// families read it: pcg_rollout_policy.hpp (fp64 networks), pcg_rollout_policy_f32.hpp (float32), pcg_rollout_pop.hpp (one member
// per slice of envs) and pcg_pop_search.hpp (the flat parameters of a population).  Fixed-width integers and doubles only: the
// same text compiles under hipRTC, under hipcc and under a plain host compiler (tools/hostcheck/host_code_check.cpp).
#pragma once

#include "../../include/pcgym_hip.h"

namespace pcg {

constexpr int POL_MAX_W = 64;   // widest hidden layer
constexpr int POL_IB = 4;       // input-side block of the first layer (columns padded to a multiple)
constexpr int POL_HB = 8;       // hidden-side block: rows of a hidden layer fed by the input, columns of a layer fed by h1
constexpr int POL_SB = 4;       // units of the streamed second hidden layer formed together

// Header of a policy's device block; the packed weights follow it (offsets in doubles from the end of the header).
struct PolicyDev {
  int32_t n_in, n_out, n_hidden, act, out_map;
  int32_t w[2];
  int32_t ld[3];      // padded row length of each layer's matrix
  int32_t offW[3], offb[3];
  double out_lo, out_hi;
};
static_assert(sizeof(PolicyDev) % 8 == 0, "the weights behind the header are doubles");

constexpr int POL32_OR = (PCG_MAX_NA + 1) / 2 * 2;  // rows of the output matrix (an even number: units come in pairs)
static_assert(POL_IB % 2 == 0 && POL_HB % 2 == 0 && POL_SB % 2 == 0 && POL32_OR % 2 == 0, "float32 policy: units come in pairs");

// Where the flat parameters of a member live in its device block (offsets in ELEMENTS from the block's first byte, the header
// included -- doubles, or floats for a float32 population): a few words that travel in the kernel arguments.
struct PopLayout {
  int32_t n;         // parameters per member
  int32_t f32;       // element kind: 0 doubles, rows plain; 1 floats, the rows of two consecutive units interleaved
  int32_t nl;        // layers (1..3)
  int32_t start[4];  // flat index of layer l's first parameter; start[nl] = n
  int32_t rows[3], cols[3], ld[3], offW[3], offb[3];
};

}  // namespace pcg
