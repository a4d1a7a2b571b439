// Smoothed labels and speech segments of a clip batch (include/vad_amd.h,
// "Clip batches"): the stage of segments_kernel.hip over the GLOBAL window
// array of a packed batch, with every clip's label range treated as a whole
// sequence of its own.  Clip k owns the windows [frame0[k], frame0[k] +
// n_rows[k]); a window that belongs to no clip (the junk windows between two
// clips) is never active and never emitted.
//
// Structure: that of segments_kernel.hip, launch for launch -- tile kernel
// (reduce per tile of VAD_SEG_TILE labels) -> one looping carry workgroup ->
// tile kernel (apply), two launches per smoothing stage, then count / carry /
// emit for the rows.  The scans themselves are the global ones (last / next
// window with the predicate, count of run starts, running sum of run
// lengths); the only addition is the clip of a window: a thread finds the
// clip of its first window by binary search in frame0 and walks forward for
// its other three, and every carry it uses is clamped to that clip's range --
// a "last predicate window" before the clip's first window, or a "next" one
// past its last, counts as none, so no gap is closed and no run is measured
// across a clip boundary.  Run sums need no clamping: a run never crosses a
// boundary because the predicate is evaluated per clip (a run ends at its
// clip's last window whatever follows).  One more launch of one looping
// workgroup turns the per-clip values the emit kernel left at every clip's
// first window into clip_rows / clip_row0 / clip_voiced, clips of no windows
// included (they take the next non-empty clip's row offset).
// NO KERNEL WAITS ON ANOTHER WORKGROUP: there is no look-back, flag, atomic or
// grid barrier in this file.  The block scan, the two carry kernels
// (seg_carry_kernel, seg_sum_carry_kernel) and the host helpers are those of
// the single-clip path, from block_scan.h; the tile kernels are this file's
// own, because the clip lookup and the clamping sit inside their bodies.
#include "block_scan.h"

namespace vad {
namespace {

// The clip tables, and the clip of a window.  Whatever the tables hold, a
// range handed out lies inside [0, n]: the kernels then read no label and
// write no output outside their arrays.
struct Clips {
  const int64_t* frame0;
  const int64_t* n_rows;
  int64_t n_clips;
  int64_t n;  // labels

  __device__ void range(int64_t k, int64_t* lo, int64_t* hi) const {
    int64_t a = frame0[k], r = n_rows[k];
    if (a < 0 || a > n) a = n;
    if (r < 0) r = 0;
    *lo = a;
    *hi = r < n - a ? a + r : n;
  }
  // the last clip whose frame0 is <= w (clips of no windows before it are
  // passed over); -1: none
  __device__ int64_t find(int64_t w) const {
    int64_t lo = 0, hi = n_clips - 1, below = -1;
    while (lo <= hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (frame0[mid] <= w) below = mid, lo = mid + 1; else hi = mid - 1;
    }
    return below;
  }
};

// The clips of a thread's kSegItems consecutive windows from `base`: k[j] and
// the clip's range [lo[j], hi[j]); in[j]: window base + j belongs to it.
struct ItemClips {
  int64_t k[kSegItems], lo[kSegItems], hi[kSegItems];
  bool in[kSegItems];
};
__device__ __forceinline__ void item_clips(const Clips& c, int64_t base, ItemClips* ic) {
  int64_t k = base < c.n ? c.find(base) : -1, lo = 0, hi = 0;
  if (k >= 0) c.range(k, &lo, &hi);
#pragma unroll
  for (int j = 0; j < kSegItems; ++j) {
    const int64_t w = base + j;
    if (j > 0 && w < c.n) {
      bool moved = false;
      while (k + 1 < c.n_clips && c.frame0[k + 1] <= w) ++k, moved = true;
      if (moved) c.range(k, &lo, &hi);
    }
    ic->k[j] = k, ic->lo[j] = lo, ic->hi[j] = hi;
    ic->in[j] = k >= 0 && w >= lo && w < hi;
  }
}

// One smoothing stage over a tile, as seg_stage_kernel of segments_kernel.hip
// with p[i] = (window i is in a clip) && ((in[i] == vin) != neg), the carries
// clamped to the clip, and 0 written for the windows of no clip.
struct StageArgs {
  const uint8_t* in;
  uint8_t* out;  // may be null (reduce only)
  Clips clips;
  int vin, neg, apply, ends;
  int64_t g;
  const int64_t* carry_prev;  // per tile: last p window before it (-1: none)
  const int64_t* carry_next;  // per tile: first p window after it (kNone: none)
  int reduce, neg_next;
  int64_t* tile_last;
  int64_t* tile_first;
};

__global__ __launch_bounds__(kSegThreads) void batch_stage_kernel(StageArgs a) {
  __shared__ int64_t lds[kSegThreads / 64];
  const int64_t tile = blockIdx.x;
  const int64_t base = tile * kSegTile + (int64_t)threadIdx.x * kSegItems;
  ItemClips ic;
  item_clips(a.clips, base, &ic);
  bool p[kSegItems], np[kSegItems];
#pragma unroll
  for (int j = 0; j < kSegItems; ++j) np[j] = p[j] = ic.in[j] && ((a.in[base + j] == a.vin) != (a.neg != 0));
  if (a.apply) {
    int64_t mine_last = -1, mine_first = kNone;
#pragma unroll
    for (int j = 0; j < kSegItems; ++j)
      if (p[j]) {
        mine_last = base + j;
        if (mine_first == kNone) mine_first = base + j;
      }
    int64_t tot;
    int64_t prev = block_excl<true>(mine_last, OpMax(), (int64_t)-1, lds, &tot);
    int64_t next = block_excl<false>(mine_first, OpMin(), kNone, lds, &tot);
    prev = OpMax()(prev, a.carry_prev[tile]);
    next = OpMin()(next, a.carry_next[tile]);
    int64_t nx[kSegItems];  // first p window after item j
#pragma unroll
    for (int j = kSegItems - 1; j >= 0; --j) {
      nx[j] = next;
      if (p[j]) next = base + j;
    }
#pragma unroll
    for (int j = 0; j < kSegItems; ++j) {
      if (p[j]) {
        prev = base + j;
      } else if (ic.in[j]) {
        // the run of !p around this window inside its clip: (lo_p, hi_p)
        const bool has_prev = prev >= ic.lo[j], has_next = nx[j] < ic.hi[j];
        const int64_t lo_p = has_prev ? prev : ic.lo[j] - 1, hi_p = has_next ? nx[j] : ic.hi[j];
        np[j] = (has_prev || a.ends) && (has_next || a.ends) && hi_p - lo_p - 1 <= a.g;
      }
    }
  }
  int64_t q_last = -1, q_first = kNone;
#pragma unroll
  for (int j = 0; j < kSegItems; ++j) {
    if (base + j >= a.clips.n) break;
    const bool v = ic.in[j] && (np[j] != (a.neg != 0));
    if (a.out) a.out[base + j] = v ? 1 : 0;
    if (ic.in[j] && (v != (a.neg_next != 0))) {
      q_last = base + j;
      if (q_first == kNone) q_first = base + j;
    }
  }
  if (a.reduce) {
    int64_t last, first;
    block_excl<true>(q_last, OpMax(), (int64_t)-1, lds, &last);
    block_excl<false>(q_first, OpMin(), kNone, lds, &first);
    if (threadIdx.x == 0) {
      a.tile_last[tile] = last;
      a.tile_first[tile] = first;
    }
  }
}

// Segment rows from the final labels d[w] = (w in a clip) && (lab[w] ==
// active).  A run [i0, i1] of clip k in clip-local windows is the row
// (k, S(i0), E(i1), offset), S(i) = (i + 2) * hop, E(i) = min((i + 2) * hop +
// frame_size, len[k]); its number is the count of run starts before it and
// its offset the sum over earlier windows of E at run ends minus S at run
// starts, exactly as seg_rows_kernel.  A window's neighbours count only
// inside its clip.  EMIT 0: the tile's count and sum.  EMIT 1: the rows, the
// packed-buffer rows (frame0[k] * hop + S, frame0[k] * hop + E, offset), and
// at every clip's first window the count and the offset before it.
struct RowsArgs {
  const uint8_t* lab;
  Clips clips;
  const int64_t* len;
  int active, frame_size, hop;
  int64_t* tile_cnt;
  int64_t* tile_sum;
  const int64_t* carry_cnt;
  const int64_t* carry_sum;
  int64_t* rows;    // capacity x 4
  int64_t* packed;  // capacity x 3
  int64_t capacity;
  int64_t* clip_cnt0;  // n_clips: run starts before the clip's first window
  int64_t* clip_off0;  // n_clips: voiced samples before it
};

template <bool EMIT>
__global__ __launch_bounds__(kSegThreads) void batch_rows_kernel(RowsArgs a) {
  __shared__ int64_t lds[kSegThreads / 64];
  const int64_t tile = blockIdx.x;
  const int64_t base = tile * kSegTile + (int64_t)threadIdx.x * kSegItems;
  ItemClips ic;
  item_clips(a.clips, base, &ic);
  bool d[kSegItems], first[kSegItems], last[kSegItems];
  int64_t s[kSegItems], e[kSegItems];
  int64_t cnt = 0, sum = 0;
#pragma unroll
  for (int j = 0; j < kSegItems; ++j) {
    const int64_t w = base + j;
    d[j] = ic.in[j] && a.lab[w] == a.active;
    first[j] = last[j] = false;
    s[j] = e[j] = 0;
    if (!d[j]) continue;
    first[j] = w == ic.lo[j] || a.lab[w - 1] != a.active;
    last[j] = w + 1 == ic.hi[j] || a.lab[w + 1] != a.active;
    s[j] = (w - ic.lo[j] + 2) * a.hop;
    const int64_t len = a.len[ic.k[j]];
    e[j] = s[j] + a.frame_size < len ? s[j] + a.frame_size : len;
    if (first[j]) ++cnt, sum -= s[j];
    if (last[j]) sum += e[j];
  }
  int64_t tot_c, tot_s;
  const int64_t ex_c = block_excl<true>(cnt, OpSum(), (int64_t)0, lds, &tot_c);
  const int64_t ex_s = block_excl<true>(sum, OpSum(), (int64_t)0, lds, &tot_s);
  if (!EMIT) {
    if (threadIdx.x == 0) {
      a.tile_cnt[tile] = tot_c;
      a.tile_sum[tile] = tot_s;
    }
    return;
  }
  int64_t r = a.carry_cnt[tile] + ex_c;    // run starts before this thread's windows
  int64_t off = a.carry_sum[tile] + ex_s;  // samples of the runs ended before them, minus open starts
#pragma unroll
  for (int j = 0; j < kSegItems; ++j) {
    if (ic.in[j] && base + j == ic.lo[j]) {  // no run is open at a clip's first window
      a.clip_cnt0[ic.k[j]] = r;
      a.clip_off0[ic.k[j]] = off;
    }
    if (!d[j]) continue;
    const int64_t origin = ic.lo[j] * a.hop;  // the clip's first sample in the packed buffer
    if (first[j]) {
      if (r < a.capacity) {
        a.rows[4 * r] = ic.k[j];
        a.rows[4 * r + 1] = s[j];
        a.rows[4 * r + 3] = off;
        a.packed[3 * r] = origin + s[j];
        a.packed[3 * r + 2] = off;
      }
      ++r;
      off -= s[j];
    }
    if (last[j]) {
      if (r - 1 < a.capacity) {
        a.rows[4 * (r - 1) + 2] = e[j];
        a.packed[3 * (r - 1) + 1] = origin + e[j];
      }
      off += e[j];
    }
  }
}

// clip_row0 / clip_rows / clip_voiced from the values at the clips' first
// windows: for clip k, nx(k) = the first clip >= k that has windows (a
// backward min-scan over the clips, one workgroup looping); the count before
// clip k is clip_cnt0[nx(k)], or the total when there is none.
__global__ __launch_bounds__(kSegThreads) void batch_clip_finish_kernel(Clips c, const int64_t* clip_cnt0,
                                                                        const int64_t* clip_off0,
                                                                        const int64_t* counts, int64_t* clip_rows,
                                                                        int64_t* clip_row0, int64_t* clip_voiced) {
  __shared__ int64_t lds[kSegThreads / 64];
  int64_t run = kNone, tot;
  for (int64_t b = c.n_clips > 0 ? (c.n_clips - 1) / kCarryPass * kCarryPass : -1; b >= 0; b -= kCarryPass) {
    const int64_t k = b + threadIdx.x;
    int64_t mine = kNone;
    if (k < c.n_clips) {
      int64_t lo, hi;
      c.range(k, &lo, &hi);
      // the clip that find() gives its first window to: the last of equal frame0
      if (hi > lo && c.find(lo) == k) mine = k;
    }
    const int64_t after = OpMin()(run, block_excl<false>(mine, OpMin(), kNone, lds, &tot));  // first such clip > k
    run = OpMin()(run, tot);
    if (k >= c.n_clips) continue;
    const int64_t here = OpMin()(mine, after);
    const int64_t c0 = here == kNone ? counts[0] : clip_cnt0[here], c1 = after == kNone ? counts[0] : clip_cnt0[after];
    const int64_t v0 = here == kNone ? counts[1] : clip_off0[here], v1 = after == kNone ? counts[1] : clip_off0[after];
    clip_row0[k] = c0;
    clip_rows[k] = c1 - c0;
    clip_voiced[k] = v1 - v0;
  }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
// workspace: [labels buffer n] [4 tile arrays of int64] [2 clip arrays of int64]
struct Workspace {
  uint8_t* buf;
  int64_t* tile[4];
  int64_t* clip[2];
};
size_t workspace_bytes(int64_t n, int64_t n_clips) {
  if (n < 0 || n_clips < 0) return 0;
  if (n == 0 && n_clips == 0) return 0;
  return align_up((size_t)n, 256) + align_up(4 * sizeof(int64_t) * (size_t)n_tiles_of(n), 256) +
         2 * sizeof(int64_t) * (size_t)n_clips;
}
Workspace carve(void* ws, int64_t n, int64_t n_clips) {
  Workspace w;
  char* p = static_cast<char*>(ws);
  w.buf = reinterpret_cast<uint8_t*>(p);
  p += align_up((size_t)n, 256);
  const int64_t nt = n_tiles_of(n);
  for (int i = 0; i < 4; ++i) w.tile[i] = reinterpret_cast<int64_t*>(p) + i * nt;
  p += align_up(4 * sizeof(int64_t) * (size_t)nt, 256);
  w.clip[0] = reinterpret_cast<int64_t*>(p);
  w.clip[1] = w.clip[0] + n_clips;
  return w;
}
bool ws_ok(const void* ws, size_t ws_bytes, int64_t n, int64_t n_clips) {
  if (n == 0 && n_clips == 0) return true;
  if (n > (int64_t)1 << 40 || n_clips > (int64_t)1 << 40) return false;  // the tile count is a grid dimension
  return ws && (reinterpret_cast<uintptr_t>(ws) & 15) == 0 && ws_bytes >= workspace_bytes(n, n_clips);
}

// The smoothing stages over `labels` into `buf` (always: the windows of no
// clip must read 0 afterwards, so even no stage is one pass); the result is
// 0 / 1 in buf.
hipError_t run_stages(const uint8_t* labels, const Clips& clips, int active, const Stage* stages, int n_stages,
                      uint8_t* buf, const Workspace& w, hipStream_t st) {
  const int64_t nt = n_tiles_of(clips.n);
  if (clips.n <= 0) return hipSuccess;
  StageArgs a{};
  a.clips = clips;
  a.carry_prev = w.tile[2];
  a.carry_next = w.tile[3];
  a.tile_last = w.tile[0];
  a.tile_first = w.tile[1];
  if (n_stages == 0) {
    a.in = labels, a.out = buf, a.vin = active;
    batch_stage_kernel<<<dim3((unsigned)nt), dim3(kSegThreads), 0, st>>>(a);
    return hipGetLastError();
  }
  // totals of the first stage's predicate over the labels
  a.in = labels, a.out = nullptr, a.vin = active, a.reduce = 1, a.neg_next = stages[0].neg;
  batch_stage_kernel<<<dim3((unsigned)nt), dim3(kSegThreads), 0, st>>>(a);
  for (int s = 0; s < n_stages; ++s) {
    seg_carry_kernel<<<dim3(1), dim3(kSegThreads), 0, st>>>(w.tile[0], w.tile[1], nt, w.tile[2], w.tile[3]);
    a.in = s == 0 ? labels : buf;
    a.vin = s == 0 ? active : 1;
    a.out = buf;
    a.neg = stages[s].neg;
    a.ends = stages[s].neg;  // open: the ends of the clip bound a run
    a.g = stages[s].g;
    a.apply = 1;
    a.reduce = s + 1 < n_stages;
    a.neg_next = a.reduce ? stages[s + 1].neg : 0;
    batch_stage_kernel<<<dim3((unsigned)nt), dim3(kSegThreads), 0, st>>>(a);
  }
  return hipGetLastError();
}

}  // namespace
}  // namespace vad

using namespace vad;

extern "C" {

size_t vad_batch_segments_workspace_bytes(int64_t n_labels, int64_t n_clips) {
  return workspace_bytes(n_labels, n_clips);
}

int vad_batch_label_smooth(const uint8_t* labels, int64_t n, const int64_t* frame0, const int64_t* n_rows,
                           int64_t n_clips, int32_t active, int64_t max_gap, int64_t min_run, uint8_t* out, void* ws,
                           size_t ws_bytes, void* stream) {
  if (n < 0 || n_clips < 0 || max_gap < 0 || min_run < 0 || active < 0 || active > 255) return VAD_EINVAL;
  if (n_clips > 0 && (!frame0 || !n_rows)) return VAD_EINVAL;
  if (n == 0) return VAD_OK;
  if (!labels || !out || overlap(labels, (size_t)n, out, (size_t)n)) return VAD_EINVAL;
  if (!ws_ok(ws, ws_bytes, n, n_clips)) return VAD_EINVAL;
  Stage stages[2];
  int k = add_stage(stages, 0, 0, max_gap, n);
  k = add_stage(stages, k, 1, min_run - 1, n);
  const Clips clips{frame0, n_rows, n_clips, n};
  return (int)run_stages(labels, clips, active, stages, k, out, carve(ws, n, n_clips),
                         static_cast<hipStream_t>(stream));
}

int vad_batch_label_segments(const uint8_t* labels, int64_t n, const int64_t* frame0, const int64_t* n_rows,
                             const int64_t* len, int64_t n_clips, int32_t active, int64_t max_gap, int64_t min_run,
                             int32_t frame_size, int32_t hop, int64_t* clip_segments, int64_t* packed_segments,
                             int64_t capacity, int64_t* counts, int64_t* clip_rows, int64_t* clip_row0,
                             int64_t* clip_voiced, void* ws, size_t ws_bytes, void* stream) {
  if (n < 0 || n_clips < 0 || max_gap < 0 || min_run < 0 || active < 0 || active > 255 || capacity < 0)
    return VAD_EINVAL;
  if (frame_size <= 0 || hop <= 0 || hop > frame_size || !counts) return VAD_EINVAL;
  if (n_clips > 0 && (!frame0 || !n_rows || !len || !clip_rows || !clip_row0 || !clip_voiced)) return VAD_EINVAL;
  if ((n > 0 && !labels) || (capacity > 0 && (!clip_segments || !packed_segments))) return VAD_EINVAL;
  if (capacity > INT64_MAX / 64) return VAD_EINVAL;
  if (overlap(labels, (size_t)n, clip_segments, (size_t)capacity * 32) ||
      overlap(labels, (size_t)n, packed_segments, (size_t)capacity * 24) || overlap(labels, (size_t)n, counts, 16))
    return VAD_EINVAL;
  if (!ws_ok(ws, ws_bytes, n, n_clips)) return VAD_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Workspace w = carve(ws, n, n_clips);
  const Clips clips{frame0, n_rows, n_clips, n};
  Stage stages[3];
  int k = add_stage(stages, 0, 0, max_gap, n);
  k = add_stage(stages, k, 1, min_run - 1, n);
  k = add_stage(stages, k, 0, frame_size / hop - 1, n);  // frames of runs this close overlap or touch
  const hipError_t e = run_stages(labels, clips, active, stages, k, w.buf, w, st);
  if (e != hipSuccess) return (int)e;
  const int64_t nt = n_tiles_of(n);
  RowsArgs a{};
  a.lab = w.buf, a.clips = clips, a.len = len, a.active = 1, a.frame_size = frame_size, a.hop = hop;
  a.tile_cnt = w.tile[0], a.tile_sum = w.tile[1], a.carry_cnt = w.tile[2], a.carry_sum = w.tile[3];
  a.rows = clip_segments, a.packed = packed_segments, a.capacity = capacity;
  a.clip_cnt0 = w.clip[0], a.clip_off0 = w.clip[1];
  if (nt > 0) batch_rows_kernel<false><<<dim3((unsigned)nt), dim3(kSegThreads), 0, st>>>(a);
  seg_sum_carry_kernel<true><<<dim3(1), dim3(kSegThreads), 0, st>>>(w.tile[0], w.tile[1], nt, w.tile[2], w.tile[3], counts);
  if (nt > 0) batch_rows_kernel<true><<<dim3((unsigned)nt), dim3(kSegThreads), 0, st>>>(a);
  if (n_clips > 0)
    batch_clip_finish_kernel<<<dim3(1), dim3(kSegThreads), 0, st>>>(clips, w.clip[0], w.clip[1], counts, clip_rows,
                                                                    clip_row0, clip_voiced);
  return (int)hipGetLastError();
}

}  // extern "C"
