// What the two hop kernels share: stream_hop_kernel (stream_kernel.hip, the
// FFN) and stream_hop_tree_kernel (stream_tree_kernel.hip, the decision
// tree) run one analyser hop of every stream, one wave per stream.  Here are
// the per-wave LDS layout, the staged tables, the FFT's small helpers and
// the launch rule.  The hop body itself stays in each kernel: one body
// instantiated with a classifier policy kept every register count but not
// the compiler's schedule, and the tree's global walk measured slower
// (profiles/stream_hop_shared/isa.md).
#pragma once

#include "vad_common.h"
#include "features.h"

namespace vad {

// Per-wave LDS scratch (floats): the FFT's ping-pong buffers (the power
// row reuses the first once the transform is done), the log-mel row, two
// rows of 64 (the window's features, 3 mfcc_n <= 48 floats, and the FFN's
// second activation row).
constexpr int kHopZ = 2 * (256 + 32);              // one 256-point complex buffer, padded
// complex element i of a buffer sits at i + i / 8: the Stockham stores of the
// first stages (stride 4 and 16 complex across lanes) spread over the banks
__device__ __forceinline__ int zp(int i) { return i + (i >> 3); }
constexpr int kHopWaveFloats = 2 * kHopZ + kMaxFilters + 64 + 64;
constexpr size_t kHopLdsBytes = 160 * 1024;  // a block's tables + scratch

// Block-shared LDS, staged once per block from the plan (the per-stream
// chain would otherwise wait on one L2 round trip per tap and DCT term):
// twiddles, filter ranges and taps, the DCT rows; the classifier's table
// follows them.
struct HopTables {
  const float2* tw;  // W512^k, k < 256
  const int* f_lo;
  const int* f_len;
  const int* f_off;
  const float* taps;
  const float* dct;  // [c][m], stride vec_row_stride(nf), 16-B aligned
};

__device__ __forceinline__ float2 cmulf(float2 a, float2 w) {
  return make_float2(fmaf(a.x, w.x, -a.y * w.y), fmaf(a.x, w.y, a.y * w.x));
}

// W256^m, 0 <= m < 256, from the W512^k table
__device__ __forceinline__ float2 w256(const float2* __restrict__ tw, int m) {
  const float2 t = tw[2 * (m & 127)];
  return m < 128 ? t : make_float2(-t.x, -t.y);
}

// Launch of a hop kernel pair (K7 for frames up to 7 x 64 samples, K16 up to
// 1024) whose blocks stage `tables` bytes; args are the kernel's arguments.
// Streams per block: at least kHopMinWaves (one wave per SIMD), then spread
// over every CU (each block stages the ~26 KB of tables from L2 once; the
// per-stream chain is LDS-bound, so fewer waves per CU run it faster), up to
// 16 waves when there are more streams than CUs, and as many as the LDS
// holds.  512 streams, A/B on one box: 2 waves per block on 256 CUs
// 11.0-11.3 us per hop, 4 on 128 CUs 10.4, 8 on 64 CUs 10.8
constexpr int kHopMinWaves = 4;
// launches of several hops: the staging amortises over the hops, so one
// stream per block spreads over more CUs (K = 8: 8.2 vs 8.4 us per hop,
// K = 32: 7.4 vs 7.6 with 4 per block)
constexpr int kHopMinWavesK = 1;
// The rule is stream_hop_block_waves (stream_kernel.hip), which the C ABI
// also exports as a query: vad_stream_hop_block_waves.

template <auto K7, auto K16, class... Args>
hipError_t launch_hop_kernels(size_t tables, int len, int64_t n_streams, int n_hops, hipStream_t st,
                              const Args&... args) {
  if (n_streams <= 0 || n_hops <= 0) return hipSuccess;
  const int waves = stream_hop_block_waves(tables, n_streams, n_hops);
  if (waves <= 0) return hipErrorInvalidValue;
  const size_t smem = tables + (size_t)waves * kHopWaveFloats * sizeof(float);
  static std::atomic<unsigned long long> attr_done{0};  // per kernel function: this template's own
  static std::atomic<unsigned long long> attr_done16{0};
  const bool small = len <= 7 * 64;
  const hipError_t e = ensure_dyn_lds(small ? reinterpret_cast<const void*>(K7) : reinterpret_cast<const void*>(K16),
                                      (int)kHopLdsBytes, small ? attr_done : attr_done16);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)((n_streams + waves - 1) / waves));
  if (small)
    hipLaunchKernelGGL(K7, grid, dim3(64 * waves), smem, st, args...);
  else
    hipLaunchKernelGGL(K16, grid, dim3(64 * waves), smem, st, args...);
  return hipGetLastError();
}

}  // namespace vad
