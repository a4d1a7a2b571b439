// The tile-scan chain's shared pieces.  segments_kernel.hip,
// batch_segments_kernel.hip and csv_parse_kernel.hip each scan an array as
//   tile kernel (reduce per tile) -> ONE looping carry workgroup -> tile
//   kernel (apply),
// with no kernel waiting on another workgroup.  Here are the block scan the
// tile kernels and the carry workgroup run, the two carry kernels of the
// label scans (launched by the single-clip and the clip-batch path alike)
// and the host helpers of those two paths.  The tile kernels stay in their
// units, and so does csv_carry_kernel, which writes a line total.  The carry
// loops are written out in each carry kernel: one loop helper under them
// changed the compiled label kernels (profiles/block_scan_shared/isa.md).
#pragma once

#include "vad_common.h"

namespace vad {
namespace {

constexpr int kScanThreads = 256;  // the block every scan here runs in

// tiles of the label scans
constexpr int kSegThreads = kScanThreads;
constexpr int kSegItems = 4;
constexpr int kSegTile = kSegThreads * kSegItems;
static_assert(kSegTile == VAD_SEG_TILE, "the header's tile is the kernels' tile");
constexpr int kCarryPass = kScanThreads;  // tile totals the carry loop scans per pass
static_assert(kCarryPass == VAD_SEG_CARRY_PASS, "the header's pass is the carry kernel's pass");
constexpr int64_t kNone = INT64_MAX;  // "no such window" of a min-scan

struct OpMax {
  __device__ int64_t operator()(int64_t a, int64_t b) const { return a > b ? a : b; }
};
struct OpMin {
  __device__ int64_t operator()(int64_t a, int64_t b) const { return a < b ? a : b; }
};
struct OpSum {
  __device__ int64_t operator()(int64_t a, int64_t b) const { return a + b; }
};

// Exclusive scan over the block's 256 threads in thread order (UP) or in
// reverse thread order (!UP): wave-level __shfl scans, the four wave totals
// through LDS.  Every LDS word read here was written in the same call.
template <bool UP, class Op>
__device__ __forceinline__ int64_t block_excl(int64_t v, Op op, int64_t ident, int64_t* lds, int64_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t t = UP ? __shfl_up(v, d) : __shfl_down(v, d);
    if (UP ? lane >= d : lane + d < 64) v = op(v, t);
  }
  if (lane == (UP ? 63 : 0)) lds[wave] = v;
  __syncthreads();
  int64_t pre = ident, tot = ident;
#pragma unroll
  for (int w = 0; w < kScanThreads / 64; ++w) {
    const int64_t x = lds[w];
    tot = op(tot, x);
    if (UP ? w < wave : w > wave) pre = op(pre, x);
  }
  __syncthreads();  // lds is reused by the next scan
  int64_t ex = UP ? __shfl_up(v, 1) : __shfl_down(v, 1);
  if (lane == (UP ? 0 : 63)) ex = ident;
  *total = tot;
  return op(pre, ex);
}

// Scan of the tile totals of a smoothing stage: carry_prev[t] = max of
// tile_last over tiles < t, carry_next[t] = min of tile_first over tiles > t.
// One workgroup, kCarryPass tiles per pass, any n_tiles.
__global__ __launch_bounds__(kSegThreads) void seg_carry_kernel(const int64_t* tile_last, const int64_t* tile_first,
                                                                int64_t n_tiles, int64_t* carry_prev,
                                                                int64_t* carry_next) {
  __shared__ int64_t lds[kSegThreads / 64];
  int64_t run = -1, tot;
  for (int64_t b = 0; b < n_tiles; b += kCarryPass) {
    const int64_t t = b + threadIdx.x;
    const int64_t ex = block_excl<true>(t < n_tiles ? tile_last[t] : (int64_t)-1, OpMax(), (int64_t)-1, lds, &tot);
    if (t < n_tiles) carry_prev[t] = OpMax()(run, ex);
    run = OpMax()(run, tot);
  }
  run = kNone;
  for (int64_t b = n_tiles > 0 ? (n_tiles - 1) / kCarryPass * kCarryPass : -1; b >= 0; b -= kCarryPass) {
    const int64_t t = b + threadIdx.x;
    const int64_t ex = block_excl<false>(t < n_tiles ? tile_first[t] : kNone, OpMin(), kNone, lds, &tot);
    if (t < n_tiles) carry_next[t] = OpMin()(run, ex);
    run = OpMin()(run, tot);
  }
}

// Scan of per-tile sums (a count, and optionally a second sum): exclusive
// carries per tile and the grand totals into totals[0] (, totals[1]).  One
// workgroup looping, as seg_carry_kernel; n_tiles = 0 writes zero totals.
// BOTH: the caller always has a second sum (the clip-batch path), and the
// pointer is not tested.
template <bool BOTH>
__global__ __launch_bounds__(kSegThreads) void seg_sum_carry_kernel(const int64_t* tile_cnt, const int64_t* tile_sum,
                                                                    int64_t n_tiles, int64_t* carry_cnt,
                                                                    int64_t* carry_sum, int64_t* totals) {
  __shared__ int64_t lds[kSegThreads / 64];
  int64_t run_c = 0, run_s = 0, tot;
  for (int64_t b = 0; b < n_tiles; b += kCarryPass) {
    const int64_t t = b + threadIdx.x;
    const int64_t ec = block_excl<true>(t < n_tiles ? tile_cnt[t] : (int64_t)0, OpSum(), (int64_t)0, lds, &tot);
    if (t < n_tiles) carry_cnt[t] = run_c + ec;
    run_c += tot;
    if (BOTH || tile_sum) {
      const int64_t es = block_excl<true>(t < n_tiles ? tile_sum[t] : (int64_t)0, OpSum(), (int64_t)0, lds, &tot);
      if (t < n_tiles) carry_sum[t] = run_s + es;
      run_s += tot;
    }
  }
  if (threadIdx.x == 0) {
    totals[0] = run_c;
    if (BOTH || tile_sum) totals[1] = run_s;
  }
}

// ---------------------------------------------------------------------------
// Host side of the label scans
// ---------------------------------------------------------------------------
inline int64_t n_tiles_of(int64_t n) { return (n + kSegTile - 1) / kSegTile; }
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// A smoothing stage: neg 0 close(g), neg 1 open(g + 1).
struct Stage {
  int neg;
  int64_t g;
};
inline int add_stage(Stage* stages, int k, int neg, int64_t g, int64_t n) {
  if (g <= 0) return k;  // close(0) and open(m <= 1) change nothing
  stages[k].neg = neg;
  stages[k].g = g < n ? g : n;
  return k + 1;
}

}  // namespace
}  // namespace vad
