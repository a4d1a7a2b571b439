// Labels -> smoothed labels -> speech segments in samples -> voiced audio
// packed in device memory (include/vad_amd.h, "Speech segments"): the stage
// after the classifiers, what vad.py:52-57,67-72 does on the host with the
// frames the analyser returned as active.
//
// Scan side.  Every quantity is a prefix scan over the labels or its reverse:
//   close(g) / open(m): index of the last / next window with the predicate
//     (forward max-scan, backward min-scan); a run between two such windows
//     is filled when it is short enough;
//   segment rows: count of run starts (the row number) and the running sum of
//     E(run end) - S(run start) (the packed offset), both forward sums;
//   active frames: count of active labels (the output row).
// Each scan is the fixed chain  tile kernel (reduce per tile of VAD_SEG_TILE
// labels) -> carry kernel (scan of the tile totals) -> tile kernel (apply).
// The apply of one smoothing stage also reduces for the next, so a stage
// costs two launches.  NO KERNEL WAITS ON ANOTHER WORKGROUP: a tile kernel
// reads only its own tile, carries written by an EARLIER launch and (segment
// rows) neighbouring labels written by an earlier launch; there is no
// look-back, flag, atomic or grid barrier anywhere in this file.  The carry
// kernel is ONE workgroup that loops over the tile totals kCarryPass at a
// time with a running carry, so any tile count works without recursion.
// The block scan, the carry kernels and the tile constants are in
// block_scan.h, shared with batch_segments_kernel.hip and the CSV line index.
//
// Copy side.  gather_kernel<T, FRAMES>: a persistent grid strides over output
// tiles of 32 KB below the device-side total; per tile the rows of its first
// and last element are found once (binary search in the segment offsets, or a
// division for the fixed-size rows of the active-frames form), and a tile
// inside one row -- every tile but a few for speech-length segments -- is
// copied with 8 independent 16-byte stores per lane and the widest loads the
// source's alignment allows (16, 8, 4 or 2 bytes).  Tiles that straddle rows
// search per 16-byte destination chunk inside [first row, last row].
#include "block_scan.h"

namespace vad {
namespace {

// One smoothing stage over a tile.  p[i] = (in[i] == vin) != neg; a run of
// !p is filled (p set) when its length is <= g and it has a p window on both
// sides (ends: the ends of the sequence count as such).  close(g): neg 0,
// ends 0; open(m): neg 1 (p = inactive), g = m - 1, ends 1.  The value
// written is 1 for an active window: out[i] = newp != neg.  apply 0: newp = p
// (the carries are not read).  reduce: the tile's last / first window with
// the NEXT stage's predicate q = (value == 1) != neg_next, for the carry
// kernel.  in == out is fine: a thread reads its four labels, then writes them.
struct StageArgs {
  const uint8_t* in;
  uint8_t* out;  // may be null (reduce only)
  int64_t n;
  int vin, neg, apply, ends;
  int64_t g;
  const int64_t* carry_prev;  // per tile: last p window before it (-1: none)
  const int64_t* carry_next;  // per tile: first p window after it (kNone: none)
  int reduce, neg_next;
  int64_t* tile_last;
  int64_t* tile_first;
};

__global__ __launch_bounds__(kSegThreads) void seg_stage_kernel(StageArgs a) {
  __shared__ int64_t lds[kSegThreads / 64];
  const int64_t tile = blockIdx.x;
  const int64_t base = tile * kSegTile + (int64_t)threadIdx.x * kSegItems;
  bool p[kSegItems];
#pragma unroll
  for (int j = 0; j < kSegItems; ++j) p[j] = base + j < a.n && ((a.in[base + j] == a.vin) != (a.neg != 0));
  bool np[kSegItems];
#pragma unroll
  for (int j = 0; j < kSegItems; ++j) np[j] = p[j];
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
      } else if (base + j < a.n) {
        const bool left = prev >= 0 || a.ends, right = nx[j] != kNone || a.ends;
        const int64_t hi = nx[j] == kNone ? a.n : nx[j];
        np[j] = left && right && hi - prev - 1 <= a.g;
      }
    }
  }
  int64_t q_last = -1, q_first = kNone;
#pragma unroll
  for (int j = 0; j < kSegItems; ++j) {
    if (base + j >= a.n) break;
    const bool v = np[j] != (a.neg != 0);
    if (a.out) a.out[base + j] = v ? 1 : 0;
    if (v != (a.neg_next != 0)) {
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

// Segment rows from the final labels d[i] = (lab[i] == active).  A run
// [i0, i1] is the row (S(i0), E(i1), offset) with S(i) = (i + 2) * hop and
// E(i) = min((i + 2) * hop + frame_size, n_samples); its number is the count
// of run starts before i0 and its offset the sum over earlier windows of
// E at run ends minus S at run starts.  EMIT 0: the tile's count and sum;
// EMIT 1: the rows, from the carries of seg_sum_carry_kernel -- the start
// window writes (start, offset), the end window writes end, rows >= capacity
// are not written.  lab[i - 1] / lab[i + 1] across a tile edge were written
// by an earlier launch.
struct RowsArgs {
  const uint8_t* lab;
  int64_t n;
  int active, frame_size, hop;
  int64_t n_samples;
  int64_t* tile_cnt;
  int64_t* tile_sum;
  const int64_t* carry_cnt;
  const int64_t* carry_sum;
  int64_t* rows;
  int64_t capacity;
};

template <bool EMIT>
__global__ __launch_bounds__(kSegThreads) void seg_rows_kernel(RowsArgs a) {
  __shared__ int64_t lds[kSegThreads / 64];
  const int64_t tile = blockIdx.x;
  const int64_t base = tile * kSegTile + (int64_t)threadIdx.x * kSegItems;
  bool d[kSegItems + 2];  // d[j + 1] = window base + j
#pragma unroll
  for (int j = -1; j <= kSegItems; ++j) {
    const int64_t i = base + j;
    d[j + 1] = i >= 0 && i < a.n && a.lab[i] == a.active;
  }
  int64_t cnt = 0, sum = 0;
#pragma unroll
  for (int j = 0; j < kSegItems; ++j) {
    if (!d[j + 1]) continue;
    const int64_t s = (base + j + 2) * a.hop;
    if (!d[j]) {
      ++cnt;
      sum -= s;
    }
    if (!d[j + 2]) sum += s + a.frame_size < a.n_samples ? s + a.frame_size : a.n_samples;
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
  int64_t k = a.carry_cnt[tile] + ex_c;    // run starts before this thread's windows
  int64_t off = a.carry_sum[tile] + ex_s;  // samples of the runs ended before them, minus open starts
#pragma unroll
  for (int j = 0; j < kSegItems; ++j) {
    if (!d[j + 1]) continue;
    const int64_t s = (base + j + 2) * a.hop;
    if (!d[j]) {
      if (k < a.capacity) {
        a.rows[3 * k] = s;
        a.rows[3 * k + 2] = off;
      }
      ++k;
      off -= s;
    }
    if (!d[j + 2]) {
      const int64_t e = s + a.frame_size < a.n_samples ? s + a.frame_size : a.n_samples;
      if (k - 1 < a.capacity) a.rows[3 * (k - 1) + 1] = e;
      off += e;
    }
  }
}

// Rank scan of the active labels: EMIT 0 the tile's count, EMIT 1 the
// compacted window list idx[rank] = i (n entries at most, in the workspace).
template <bool EMIT>
__global__ __launch_bounds__(kSegThreads) void seg_rank_kernel(const uint8_t* lab, int64_t n, int active,
                                                               int64_t* tile_cnt, const int64_t* carry_cnt,
                                                               int64_t* idx) {
  __shared__ int64_t lds[kSegThreads / 64];
  const int64_t tile = blockIdx.x;
  const int64_t base = tile * kSegTile + (int64_t)threadIdx.x * kSegItems;
  bool d[kSegItems];
  int64_t cnt = 0;
#pragma unroll
  for (int j = 0; j < kSegItems; ++j) {
    d[j] = base + j < n && lab[base + j] == active;
    cnt += d[j];
  }
  int64_t tot;
  const int64_t ex = block_excl<true>(cnt, OpSum(), (int64_t)0, lds, &tot);
  if (!EMIT) {
    if (threadIdx.x == 0) tile_cnt[tile] = tot;
    return;
  }
  int64_t k = carry_cnt[tile] + ex;
#pragma unroll
  for (int j = 0; j < kSegItems; ++j)
    if (d[j]) idx[k++] = base + j;
}

// ---------------------------------------------------------------------------
// Copy side
// ---------------------------------------------------------------------------
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kGatherThreads = 256;
constexpr int kGatherChunks = 8;  // 16-byte chunks per lane and tile: 32 KB tiles
constexpr int kGatherGrid = 2048;  // 256 CUs x 8 workgroups of 4 waves

// 16 bytes from an address aligned to AB bytes (bits copied, never converted)
template <int AB>
__device__ __forceinline__ u32x4 load16(const char* p) {
  if constexpr (AB == 16) {
    return *reinterpret_cast<const u32x4*>(p);
  } else if constexpr (AB == 8) {
    const u32x2 x = *reinterpret_cast<const u32x2*>(p), y = *reinterpret_cast<const u32x2*>(p + 8);
    return u32x4{x.x, x.y, y.x, y.y};
  } else if constexpr (AB == 4) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    return u32x4{q[0], q[1], q[2], q[3]};
  } else {
    const uint16_t* q = reinterpret_cast<const uint16_t*>(p);
    return u32x4{q[0] | (uint32_t)q[1] << 16, q[2] | (uint32_t)q[3] << 16, q[4] | (uint32_t)q[5] << 16,
                 q[6] | (uint32_t)q[7] << 16};
  }
}

template <int ES>
__device__ __forceinline__ u32x4 load16_any(const char* p) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if ((a & 15) == 0) return load16<16>(p);
  if ((a & 7) == 0) return load16<8>(p);
  if (ES == 4 || (a & 3) == 0) return load16<4>(p);
  return load16<2>(p);
}

// a whole tile inside one row: lane t copies chunks t, t + 256, ...; all the
// loads are issued before the first store
template <int AB>
__device__ __forceinline__ void copy_tile(const char* src, char* dst) {
  u32x4 v[kGatherChunks];
#pragma unroll
  for (int j = 0; j < kGatherChunks; ++j) v[j] = load16<AB>(src + (size_t)(j * kGatherThreads + threadIdx.x) * 16);
#pragma unroll
  for (int j = 0; j < kGatherChunks; ++j)
    *reinterpret_cast<u32x4*>(dst + (size_t)(j * kGatherThreads + threadIdx.x) * 16) = v[j];
}

struct GatherArgs {
  // segments form: rows (start, end, offset), counts[0] = rows found
  const int64_t* rows;
  const int64_t* counts;
  int64_t capacity;
  // active-frames form: row r = frame_size samples from (idx[r] + 2) * hop
  const int64_t* idx;
  const int64_t* count;
  int frame_size, hop;
};

template <bool FRAMES>
struct RowTable {
  const GatherArgs& a;
  int64_t n_rows;
  __device__ int64_t start(int64_t k) const { return FRAMES ? (a.idx[k] + 2) * a.hop : a.rows[3 * k]; }
  __device__ int64_t offset(int64_t k) const { return FRAMES ? k * a.frame_size : a.rows[3 * k + 2]; }
  __device__ int64_t len(int64_t k) const { return FRAMES ? a.frame_size : a.rows[3 * k + 1] - a.rows[3 * k]; }
  // the row of output element e, known to lie in rows [lo, hi]
  __device__ int64_t locate(int64_t e, int64_t lo, int64_t hi) const {
    if (FRAMES) {  // a 32-bit division when e is near row lo (every per-chunk call)
      const uint64_t r = (uint64_t)(e - lo * a.frame_size);
      return lo + (r >> 32 ? (int64_t)(r / (uint32_t)a.frame_size) : (int64_t)((uint32_t)r / (uint32_t)a.frame_size));
    }
    while (lo < hi) {  // the last row whose offset is <= e
      const int64_t mid = lo + (hi - lo + 1) / 2;
      if (a.rows[3 * mid + 2] <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
  }
};

template <typename T, bool FRAMES>
__global__ __launch_bounds__(kGatherThreads) void gather_kernel(const T* audio, int64_t n_samples, GatherArgs a,
                                                                T* out, int64_t out_capacity) {
  constexpr int V = 16 / sizeof(T);
  constexpr int64_t kTileChunks = (int64_t)kGatherThreads * kGatherChunks;
  RowTable<FRAMES> tab{a, 0};
  int64_t total;
  if (FRAMES) {
    tab.n_rows = *a.count < a.capacity ? *a.count : a.capacity;
    total = tab.n_rows * a.frame_size;
  } else {
    tab.n_rows = a.counts[0] < a.capacity ? a.counts[0] : a.capacity;
    total = tab.n_rows > 0 ? tab.offset(tab.n_rows - 1) + tab.len(tab.n_rows - 1) : 0;
  }
  if (total > out_capacity) total = out_capacity;
  if (tab.n_rows <= 0 || total <= 0) return;
  // destination chunks are 16-byte lines of memory: chunk c holds the output
  // elements [c * V - mis, c * V - mis + V)
  const int mis = (int)((reinterpret_cast<uintptr_t>(out) & 15) / sizeof(T));
  const int64_t n_chunks = (total + mis + V - 1) / V;
  for (int64_t c0 = (int64_t)blockIdx.x * kTileChunks; c0 < n_chunks; c0 += (int64_t)gridDim.x * kTileChunks) {
    const int64_t e_lo = c0 * V - mis < 0 ? 0 : c0 * V - mis;
    const int64_t e_end = (c0 + kTileChunks) * V - mis < total ? (c0 + kTileChunks) * V - mis : total;
    const int64_t k_lo = tab.locate(e_lo, 0, tab.n_rows - 1);
    const int64_t k_hi = tab.locate(e_end - 1, k_lo, tab.n_rows - 1);
    if (k_lo == k_hi && c0 * V - mis >= 0 && (c0 + kTileChunks) * V - mis <= total) {
      const int64_t o = tab.offset(k_lo), s = tab.start(k_lo) + (e_lo - o);
      if (e_end <= o + tab.len(k_lo) && s >= 0 && s + kTileChunks * V <= n_samples) {
        const char* src = reinterpret_cast<const char*>(audio + s);
        char* dst = reinterpret_cast<char*>(out + e_lo);
        const uintptr_t al = reinterpret_cast<uintptr_t>(src);
        if ((al & 15) == 0) copy_tile<16>(src, dst);
        else if ((al & 7) == 0) copy_tile<8>(src, dst);
        else if (sizeof(T) == 4 || (al & 3) == 0) copy_tile<4>(src, dst);
        else copy_tile<2>(src, dst);
        continue;
      }
    }
    for (int j = 0; j < kGatherChunks; ++j) {
      const int64_t c = c0 + (int64_t)j * kGatherThreads + threadIdx.x;
      if (c >= n_chunks) break;
      const int64_t e = c * V - mis;
      int64_t ee = e < 0 ? 0 : e;
      const int64_t e_stop = e + V < total ? e + V : total;
      int64_t k = k_lo == k_hi ? k_lo : tab.locate(ee, k_lo, k_hi);
      int64_t o = tab.offset(k), s = tab.start(k), l = tab.len(k);
      if (e >= 0 && e + V <= total && e + V <= o + l) {
        const int64_t si = s + (e - o);
        if (si >= 0 && si + V <= n_samples)
          *reinterpret_cast<u32x4*>(out + e) = load16_any<sizeof(T)>(reinterpret_cast<const char*>(audio + si));
        continue;
      }
      for (; ee < e_stop; ++ee) {  // a chunk across a row boundary or an end of the output
        while (ee >= o + l && k + 1 < tab.n_rows) {
          ++k;
          o = tab.offset(k), s = tab.start(k), l = tab.len(k);
        }
        const int64_t si = s + (ee - o);
        if (si >= 0 && si < n_samples) out[ee] = audio[si];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
// workspace: [labels buffer n] [4 tile arrays of int64] [window list n int64]
struct Workspace {
  uint8_t* buf;
  int64_t* tile[4];
  int64_t* idx;
};
size_t workspace_bytes(int64_t n) {
  if (n <= 0) return 0;
  return align_up((size_t)n, 256) + align_up(4 * sizeof(int64_t) * (size_t)n_tiles_of(n), 256) +
         sizeof(int64_t) * (size_t)n;
}
Workspace carve(void* ws, int64_t n) {
  Workspace w;
  char* p = static_cast<char*>(ws);
  w.buf = reinterpret_cast<uint8_t*>(p);
  p += align_up((size_t)(n > 0 ? n : 0), 256);
  const int64_t nt = n_tiles_of(n > 0 ? n : 0);
  for (int i = 0; i < 4; ++i) w.tile[i] = reinterpret_cast<int64_t*>(p) + i * nt;
  p += align_up(4 * sizeof(int64_t) * (size_t)nt, 256);
  w.idx = reinterpret_cast<int64_t*>(p);
  return w;
}

bool ws_ok(const void* ws, size_t ws_bytes, int64_t n) {
  if (n <= 0) return true;
  if (n > (int64_t)1 << 40) return false;  // the tile count is a grid dimension
  return ws && (reinterpret_cast<uintptr_t>(ws) & 15) == 0 && ws_bytes >= workspace_bytes(n);
}

// The smoothing stages over `labels` into `buf`; returns through `cur` /
// `cur_active` where the result lives: with no effective stage and
// copy == false that is the labels themselves.
hipError_t run_stages(const uint8_t* labels, int64_t n, int active, const Stage* stages, int n_stages, uint8_t* buf,
                      bool copy, const Workspace& w, hipStream_t st, const uint8_t** cur, int* cur_active) {
  const int64_t nt = n_tiles_of(n);
  *cur = labels;
  *cur_active = active;
  if (n <= 0) return hipSuccess;
  StageArgs a{};
  a.n = n;
  a.carry_prev = w.tile[2];
  a.carry_next = w.tile[3];
  a.tile_last = w.tile[0];
  a.tile_first = w.tile[1];
  if (n_stages == 0) {
    if (!copy) return hipSuccess;
    a.in = labels, a.out = buf, a.vin = active;
    seg_stage_kernel<<<dim3((unsigned)nt), dim3(kSegThreads), 0, st>>>(a);
    *cur = buf, *cur_active = 1;
    return hipGetLastError();
  }
  // totals of the first stage's predicate over the labels
  a.in = labels, a.out = nullptr, a.vin = active, a.reduce = 1, a.neg_next = stages[0].neg;
  seg_stage_kernel<<<dim3((unsigned)nt), dim3(kSegThreads), 0, st>>>(a);
  for (int s = 0; s < n_stages; ++s) {
    seg_carry_kernel<<<dim3(1), dim3(kSegThreads), 0, st>>>(w.tile[0], w.tile[1], nt, w.tile[2], w.tile[3]);
    a.in = s == 0 ? labels : buf;
    a.vin = s == 0 ? active : 1;
    a.out = buf;
    a.neg = stages[s].neg;
    a.ends = stages[s].neg;  // open: the sequence ends bound a run
    a.g = stages[s].g;
    a.apply = 1;
    a.reduce = s + 1 < n_stages;
    a.neg_next = a.reduce ? stages[s + 1].neg : 0;
    seg_stage_kernel<<<dim3((unsigned)nt), dim3(kSegThreads), 0, st>>>(a);
  }
  *cur = buf, *cur_active = 1;
  return hipGetLastError();
}

template <typename T>
int gather_segments(const T* audio, int64_t n_samples, const int64_t* segments, const int64_t* counts,
                    int64_t capacity, T* out, int64_t out_capacity, void* stream) {
  if (n_samples < 0 || capacity < 0 || out_capacity < 0 || !counts) return VAD_EINVAL;
  if ((n_samples > 0 && !audio) || (capacity > 0 && !segments) || (out_capacity > 0 && !out)) return VAD_EINVAL;
  if (reinterpret_cast<uintptr_t>(audio) % sizeof(T) || reinterpret_cast<uintptr_t>(out) % sizeof(T))
    return VAD_EINVAL;
  if (overlap(audio, (size_t)n_samples * sizeof(T), out, (size_t)out_capacity * sizeof(T))) return VAD_EINVAL;
  const int64_t bound = out_capacity < n_samples ? out_capacity : n_samples;  // the voiced total is at most either
  if (bound == 0 || capacity == 0) return VAD_OK;
  constexpr int V = 16 / sizeof(T);
  const int64_t tiles = ((bound + V - 1) / V + 1 + kGatherThreads * kGatherChunks - 1) / (kGatherThreads * kGatherChunks);
  GatherArgs a{};
  a.rows = segments, a.counts = counts, a.capacity = capacity;
  gather_kernel<T, false><<<dim3((unsigned)(tiles < kGatherGrid ? tiles : kGatherGrid)), dim3(kGatherThreads), 0,
                            static_cast<hipStream_t>(stream)>>>(audio, n_samples, a, out, out_capacity);
  return (int)hipGetLastError();
}

template <typename T>
int gather_active_frames(const T* audio, int64_t n_samples, const uint8_t* labels, int64_t n, int32_t active,
                         int32_t frame_size, int32_t hop, T* out, int64_t out_capacity_frames, int64_t* count,
                         void* ws, size_t ws_bytes, void* stream) {
  if (n < 0 || n_samples < 0 || out_capacity_frames < 0 || frame_size <= 0 || hop <= 0 || !count) return VAD_EINVAL;
  if (active < 0 || active > 255) return VAD_EINVAL;
  if (n > 0 && (!labels || !audio)) return VAD_EINVAL;
  if (out_capacity_frames > 0 && !out) return VAD_EINVAL;
  if (reinterpret_cast<uintptr_t>(audio) % sizeof(T) || reinterpret_cast<uintptr_t>(out) % sizeof(T))
    return VAD_EINVAL;
  // window n - 1 is frame n + 1: it must end inside the clip
  if (n > 0 && (n_samples < frame_size || n + 1 > (n_samples - frame_size) / hop)) return VAD_EINVAL;
  if (out_capacity_frames > INT64_MAX / frame_size) return VAD_EINVAL;
  if (!ws_ok(ws, ws_bytes, n)) return VAD_EINVAL;
  if (overlap(audio, (size_t)n_samples * sizeof(T), out, (size_t)out_capacity_frames * frame_size * sizeof(T)))
    return VAD_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Workspace w = carve(ws, n);
  const int64_t nt = n_tiles_of(n);
  if (nt > 0)
    seg_rank_kernel<false><<<dim3((unsigned)nt), dim3(kSegThreads), 0, st>>>(labels, n, active, w.tile[0], nullptr,
                                                                               nullptr);
  seg_sum_carry_kernel<false><<<dim3(1), dim3(kSegThreads), 0, st>>>(w.tile[0], nullptr, nt, w.tile[2], nullptr, count);
  const int64_t rows = out_capacity_frames < n ? out_capacity_frames : n;
  if (rows > 0) {
    seg_rank_kernel<true><<<dim3((unsigned)nt), dim3(kSegThreads), 0, st>>>(labels, n, active, nullptr, w.tile[2],
                                                                              w.idx);
    constexpr int V = 16 / sizeof(T);
    const int64_t bound = rows * frame_size;
    const int64_t tiles =
        ((bound + V - 1) / V + 1 + kGatherThreads * kGatherChunks - 1) / (kGatherThreads * kGatherChunks);
    GatherArgs a{};
    a.idx = w.idx, a.count = count, a.capacity = out_capacity_frames, a.frame_size = frame_size, a.hop = hop;
    gather_kernel<T, true><<<dim3((unsigned)(tiles < kGatherGrid ? tiles : kGatherGrid)), dim3(kGatherThreads), 0,
                             st>>>(audio, n_samples, a, out, bound);
  }
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace vad

using namespace vad;

extern "C" {

size_t vad_segments_workspace_bytes(int64_t n_labels) { return workspace_bytes(n_labels); }

int vad_label_smooth(const uint8_t* labels, int64_t n, int32_t active, int64_t max_gap, int64_t min_run,
                     uint8_t* out, void* ws, size_t ws_bytes, void* stream) {
  if (n < 0 || max_gap < 0 || min_run < 0 || active < 0 || active > 255) return VAD_EINVAL;
  if (n == 0) return VAD_OK;
  if (!labels || !out || overlap(labels, (size_t)n, out, (size_t)n)) return VAD_EINVAL;
  if (!ws_ok(ws, ws_bytes, n)) return VAD_EINVAL;
  Stage stages[2];
  int k = add_stage(stages, 0, 0, max_gap, n);
  k = add_stage(stages, k, 1, min_run - 1, n);
  const uint8_t* cur;
  int cur_active;
  return (int)run_stages(labels, n, active, stages, k, out, true, carve(ws, n), static_cast<hipStream_t>(stream),
                         &cur, &cur_active);
}

int vad_label_segments(const uint8_t* labels, int64_t n, int32_t active, int64_t max_gap, int64_t min_run,
                       int32_t frame_size, int32_t hop, int64_t n_samples, int64_t* segments, int64_t capacity,
                       int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
  if (n < 0 || max_gap < 0 || min_run < 0 || active < 0 || active > 255 || capacity < 0 || n_samples < 0)
    return VAD_EINVAL;
  if (frame_size <= 0 || hop <= 0 || hop > frame_size || !counts) return VAD_EINVAL;
  if ((n > 0 && !labels) || (capacity > 0 && !segments)) return VAD_EINVAL;
  const int64_t windows = vad_n_frames(n_samples, frame_size, hop) - 5;
  if (n > (windows > 0 ? windows : 0)) return VAD_EINVAL;
  if (!ws_ok(ws, ws_bytes, n)) return VAD_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Workspace w = carve(ws, n);
  Stage stages[3];
  int k = add_stage(stages, 0, 0, max_gap, n);
  k = add_stage(stages, k, 1, min_run - 1, n);
  k = add_stage(stages, k, 0, frame_size / hop - 1, n);  // frames of runs this close overlap or touch
  RowsArgs a{};
  const hipError_t e = run_stages(labels, n, active, stages, k, w.buf, false, w, st, &a.lab, &a.active);
  if (e != hipSuccess) return (int)e;
  const int64_t nt = n_tiles_of(n);
  a.n = n, a.frame_size = frame_size, a.hop = hop, a.n_samples = n_samples;
  a.tile_cnt = w.tile[0], a.tile_sum = w.tile[1], a.carry_cnt = w.tile[2], a.carry_sum = w.tile[3];
  a.rows = segments, a.capacity = capacity;
  if (nt > 0) seg_rows_kernel<false><<<dim3((unsigned)nt), dim3(kSegThreads), 0, st>>>(a);
  seg_sum_carry_kernel<false><<<dim3(1), dim3(kSegThreads), 0, st>>>(w.tile[0], w.tile[1], nt, w.tile[2], w.tile[3], counts);
  if (nt > 0 && capacity > 0) seg_rows_kernel<true><<<dim3((unsigned)nt), dim3(kSegThreads), 0, st>>>(a);
  return (int)hipGetLastError();
}

int vad_gather_segments_f32(const float* audio, int64_t n_samples, const int64_t* segments, const int64_t* counts,
                            int64_t capacity, float* out, int64_t out_capacity, void* stream) {
  return gather_segments<float>(audio, n_samples, segments, counts, capacity, out, out_capacity, stream);
}
int vad_gather_segments_i16(const int16_t* audio, int64_t n_samples, const int64_t* segments, const int64_t* counts,
                            int64_t capacity, int16_t* out, int64_t out_capacity, void* stream) {
  return gather_segments<int16_t>(audio, n_samples, segments, counts, capacity, out, out_capacity, stream);
}

int vad_gather_active_frames_f32(const float* audio, int64_t n_samples, const uint8_t* labels, int64_t n,
                                 int32_t active, int32_t frame_size, int32_t hop, float* out,
                                 int64_t out_capacity_frames, int64_t* count, void* ws, size_t ws_bytes,
                                 void* stream) {
  return gather_active_frames<float>(audio, n_samples, labels, n, active, frame_size, hop, out, out_capacity_frames,
                                     count, ws, ws_bytes, stream);
}
int vad_gather_active_frames_i16(const int16_t* audio, int64_t n_samples, const uint8_t* labels, int64_t n,
                                 int32_t active, int32_t frame_size, int32_t hop, int16_t* out,
                                 int64_t out_capacity_frames, int64_t* count, void* ws, size_t ws_bytes,
                                 void* stream) {
  return gather_active_frames<int16_t>(audio, n_samples, labels, n, active, frame_size, hop, out,
                                       out_capacity_frames, count, ws, ws_bytes, stream);
}

}  // extern "C"
