// The FFN's speech score, one function for the clip path (score_kernel.hip,
// logit_scores_kernel) and the live path (stream_kernel.hip, the scored hop
// kernel): the softmax of C logits read at class `active`,
//   s = 1 / (1 + sum_{j != active} expf(z_j - z_active)),
// and 0 when any logit is inf or NaN.  The same arithmetic in the same order
// wherever a score is made, so a threshold chosen on clips means the same
// thing on a stream.
#pragma once

#include "vad_common.h"

namespace vad {

// A row of C logits, read as one vector: 4-byte aligned is all a row has when
// C is odd, and all a global load needs.
template <int C>
struct __attribute__((packed, aligned(4))) LogitRow {
  float z[C];
};

// Z: anything indexable, z[0] .. z[C - 1]: the row's array, or a float vector
// whose first C lanes are the logits.
template <int C, class Z>
__device__ __forceinline__ float softmax_score(const Z& z, int active) {
  float za = z[0];
#pragma unroll
  for (int j = 1; j < C; ++j) za = j == active ? z[j] : za;
  float sum = 0.f;
  bool finite = true;
#pragma unroll
  for (int j = 0; j < C; ++j) {
    finite &= fabsf(z[j]) < INFINITY;  // false for inf and NaN
    const float e = expf(z[j] - za);
    sum += j == active ? 0.f : e;
  }
  return finite ? 1.0f / (1.0f + sum) : 0.f;
}

}  // namespace vad
