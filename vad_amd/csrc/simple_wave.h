// One wave's share of the energy / ZCR / spectral features (simple_kernel.hip):
// the seven values of one frame whose transform length L is a power of two,
// computed by the 64 lanes of a wave in its own LDS slice.  Called by
// simple_features_wave_kernel (many frames, one row each to global memory)
// and by simple_stream_block_kernel (a stream's frames, rows to LDS): the
// same lane-strided partial sums, butterflies and radix-2 order, so both
// give the same bits.
#pragma once

#include "vad_common.h"

namespace vad {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
// LDS operations are in order within a wave; this keeps the compiler from
// moving them across the point where lanes read each other's stores
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// x: the frame (T = float or int16_t, one exact (double) per sample);
// twc / tws: the W_L^j table in LDS when tw_lds (L <= 4096); re / im: this
// wave's [L] + [L] doubles of LDS; o: the row [3 + n_bands], written by lane 0.
// The caller orders its next use of re / im after this one (wave_lds_sync).
template <typename T>
__device__ __forceinline__ void simple_wave_features(const T* __restrict__ x, int frame_len, int L, int log2L,
                                                     int pad, int band_bins, int n_bands, int tw_lds,
                                                     const double* twc, const double* tws, double* re, double* im,
                                                     int lane, double* o) {
  double e = 0.0, z = 0.0;
  for (int i = lane; i < frame_len; i += 64) {
    const double v = (double)x[i];
    e += v * v;
    if (i + 1 < frame_len) {
      const double w = (double)x[i + 1];
      const double sv = (double)((v > 0.0) - (v < 0.0)), sw = (double)((w > 0.0) - (w < 0.0));
      z += fabs(sw - sv);
    }
  }
  e = wave_sum(e);
  z = wave_sum(z);
  for (int i = lane; i < L; i += 64) {
    const int sidx = i - pad;
    const double v = (sidx >= 0 && sidx < frame_len) ? (double)x[sidx] : 0.0;
    const int r = (int)(__builtin_bitreverse32((unsigned)i) >> (32 - log2L));
    re[r] = v;
    im[r] = 0.0;
  }
  wave_lds_sync();
  for (int len = 2; len <= L; len <<= 1) {  // iterative radix-2 DIT, as the block kernel
    const int half = len >> 1;
    for (int b = lane; b < (L >> 1); b += 64) {
      const int grp = b / half, k = b - grp * half;
      const int i0 = grp * len + k, i1 = i0 + half;
      const int tw = k * (L / len);
      double c, s;
      if (tw_lds) {
        c = twc[tw];
        s = tws[tw];
      } else {
        sincospi(-2.0 * (double)tw / (double)L, &s, &c);
      }
      const double xr = re[i1] * c - im[i1] * s, xi = re[i1] * s + im[i1] * c;
      const double ar = re[i0], ai = im[i0];
      re[i0] = ar + xr;
      im[i0] = ai + xi;
      re[i1] = ar - xr;
      im[i1] = ai - xi;
    }
    wave_lds_sync();
  }
  double mag_sum = 0.0;
  for (int k = lane; k < L; k += 64) {
    const double m = sqrt(re[k] * re[k] + im[k] * im[k]);
    mag_sum += m;
    re[k] = m;
  }
  const double mean = wave_sum(mag_sum) / (double)L;
  double ssd = 0.0;
  for (int k = lane; k < L; k += 64) {
    const double d = re[k] - mean;
    ssd += d * d;
  }
  ssd = wave_sum(ssd);
  for (int b = 0; b < n_bands; ++b) {
    double be = 0.0;
    for (int k = b * band_bins + lane; k < (b + 1) * band_bins; k += 64) be += re[k] * re[k];
    be = wave_sum(be);
    if (lane == 0) o[3 + b] = be / (double)band_bins;
  }
  if (lane == 0) {
    o[0] = e / (double)frame_len;
    o[1] = (z * 0.5) / ((double)frame_len - 1.0) * (double)frame_len;
    o[2] = sqrt(ssd / (double)L);
  }
}

}  // namespace vad
