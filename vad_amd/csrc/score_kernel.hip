// Speech scores and the decisions made from them (include/vad_amd.h, "Speech
// scores"): the operating point the hard labels of the classifiers lack.
//
//   scores     s[i] in [0, 1], the classifier's estimate that window i is of
//              class `active`: the softmax of the logits the FFN window kernel
//              already writes, or the class fraction of the tree leaf a window
//              ends in (the walks of tree_kernel.hip, ending in one load of
//              node_score[leaf]);
//   decisions  hysteresis (an onset and an offset threshold) and padding
//              (dilation) as uint8 0 / 1 labels, which the segment stage takes
//              with active = 1;
//   scoring    reference labels from speech intervals in samples, and the
//              histogram of scores (or the confusion matrix of labels) per
//              reference class, from which the host draws a ROC.
//
// The two scans are the chain of segments_kernel.hip, from block_scan.h: tile
// kernel (reduce per tile of VAD_SEG_TILE windows) -> the ONE looping carry
// workgroup (seg_carry_kernel) -> tile kernel (apply).  NO KERNEL WAITS ON
// ANOTHER WORKGROUP: a tile kernel reads its own tile and carries written by
// an earlier launch; there is no look-back, flag or grid barrier here, and no
// atomic outside the histogram.  Every workspace word a kernel reads was
// written by an earlier launch of the same call.
//   hysteresis: a window with s >= on or s < off is DECIDED; h[i] is the bit
//     of the last decided window <= i, so the scan is a max over the keys
//     2 * index + bit (-1: undecided);
//   dilation: the last active window <= i and the first >= i, the two scans
//     close() runs.
// The clip-batch forms clamp every carry to the window's clip, in the manner
// of batch_segments_kernel.hip; the clip lookup is restated here (Clips)
// because that unit's tile kernels keep theirs inside their bodies.
#include "block_scan.h"
#include "features.h"
#include "score_dev.h"
#include "tree_walk.h"

namespace vad {
namespace {

int num_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
  }
  return n;
}

// ---------------------------------------------------------------------------
// FFN scores
// ---------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void logit_scores_kernel(const float* __restrict__ logits, int64_t n, int active,
                                                           float* __restrict__ scores) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const LogitRow<C> r = *reinterpret_cast<const LogitRow<C>*>(logits + i * C);
    scores[i] = softmax_score<C>(r.z, active);  // score_dev.h: the hop kernel's function too
  }
}

// ---------------------------------------------------------------------------
// Tree scores: the kernels of tree_kernel.hip with the walk ending in the leaf
// NODE, whose score is then one load.  Same staging, same feature arithmetic
// (features.h), same LDS limit for the compact table.
// ---------------------------------------------------------------------------
constexpr int kTreeWin = 256;
constexpr int kTreeXStride = 3 * kMaxCoefs + 1;
constexpr int kLdsNodes = 3072;  // tree_kernel.hip's: 48 KB of compact nodes

__global__ __launch_bounds__(256) void tree_rows_score_kernel(const TreeNode* __restrict__ nodes, int n_nodes,
                                                              const float* __restrict__ node_score,
                                                              const float* __restrict__ x, int64_t n, int dim,
                                                              float* __restrict__ scores) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    scores[i] = node_score[tree_walk_node(nodes, n_nodes, x + i * dim, 1)];
}

template <int MN, bool LDSN>
__global__ __launch_bounds__(256) void tree_window_score_kernel(const TreeNode* __restrict__ nodes,
                                                                const TreeNodeC* __restrict__ cnodes, int n_nodes,
                                                                const float* __restrict__ node_score,
                                                                const float* __restrict__ mfcc, int64_t n_rows,
                                                                int mfcc_n_rt, int mode, float* __restrict__ scores) {
  constexpr int XS = MN > 0 ? 3 * MN : kTreeXStride;
  constexpr int RS = MN > 0 ? MN : kMaxCoefs;
  __shared__ float rows[(kTreeWin + 4) * RS];
  __shared__ float X[kTreeWin * XS];
  extern __shared__ TreeNodeC cn_s[];
  const int mfcc_n = MN > 0 ? MN : mfcc_n_rt;
  const int tid = threadIdx.x;
  if constexpr (LDSN) {
    for (int i = tid; i < n_nodes; i += 256) cn_s[i] = cnodes[i];
    // (visible after the first chunk's barrier)
  }
  const int64_t n_frames = n_rows + 5;
  const int64_t n_chunks = (n_rows + kTreeWin - 1) / kTreeWin;
  for (int64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
    const int64_t base = ch * kTreeWin;
    const int64_t avail = n_frames - base;
    const int nr = (int)(avail < kTreeWin + 4 ? avail : kTreeWin + 4);
    for (int i = tid; i < nr * mfcc_n; i += 256) {
      const int r = i / mfcc_n, c = i - r * mfcc_n;
      rows[r * RS + c] = mfcc[base * mfcc_n + i];
    }
    __syncthreads();
    const int64_t nwin64 = n_rows - base;
    const int nwin = (int)(nwin64 < kTreeWin ? nwin64 : kTreeWin);
    for (int i = tid; i < nwin * mfcc_n; i += 256) {
      const int w = i / mfcc_n, c = i - w * mfcc_n;
      const float* rw = rows + w * RS + c;
      const Feat3 ft = feature_triple(rw[0], rw[RS], rw[2 * RS], rw[3 * RS], rw[4 * RS], mode);
      float* xw = X + w * XS;
      xw[c] = ft.mn;
      xw[mfcc_n + c] = ft.d1;
      xw[2 * mfcc_n + c] = ft.d2;
    }
    __syncthreads();
    if (tid < nwin) {
      int leaf;
      if constexpr (LDSN) leaf = tree_walk_c_node(cn_s, n_nodes, X + tid * XS);
      else leaf = tree_walk_node(nodes, n_nodes, X + tid * XS, 1);
      scores[base + tid] = node_score[leaf];
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Clips of a batch (the tables of "Clip batches")
// ---------------------------------------------------------------------------
// Whatever the tables hold, a range handed out lies inside [0, n].
struct Clips {
  const int64_t* frame0;
  const int64_t* n_rows;
  int64_t n_clips;
  int64_t n;  // windows

  __device__ void range(int64_t k, int64_t* lo, int64_t* hi) const {
    int64_t a = frame0[k], r = n_rows[k];
    if (a < 0 || a > n) a = n;
    if (r < 0) r = 0;
    *lo = a;
    *hi = r < n - a ? a + r : n;
  }
  // the last clip whose frame0 is <= w; -1: none
  __device__ int64_t find(int64_t w) const {
    int64_t lo = 0, hi = n_clips - 1, below = -1;
    while (lo <= hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (frame0[mid] <= w) below = mid, lo = mid + 1; else hi = mid - 1;
    }
    return below;
  }
};

// The clip ranges [lo[j], hi[j]) of a thread's kSegItems windows from `base`
// (an empty range: the window belongs to no clip) and the clip numbers.
// !BATCH: the one range [0, n).
struct ItemRange {
  int64_t k[kSegItems], lo[kSegItems], hi[kSegItems];
};
template <bool BATCH>
__device__ __forceinline__ void item_ranges(const Clips& c, int64_t base, ItemRange* r) {
  if (!BATCH) {
#pragma unroll
    for (int j = 0; j < kSegItems; ++j) r->k[j] = 0, r->lo[j] = 0, r->hi[j] = c.n;
    return;
  }
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
    const bool in = k >= 0 && w >= lo && w < hi;
    r->k[j] = k, r->lo[j] = in ? lo : 0, r->hi[j] = in ? hi : 0;
  }
}

// ---------------------------------------------------------------------------
// Hysteresis
// ---------------------------------------------------------------------------
struct HystArgs {
  const float* s;
  uint8_t* out;
  Clips clips;  // n = windows; the tables are null for a single clip
  float on, off;
  int64_t* tile_last;          // reduce: the tile's largest key
  int64_t* tile_first;         // reduce: kNone (seg_carry_kernel scans it too)
  const int64_t* carry_prev;   // apply: the largest key before the tile
};

template <bool BATCH, bool APPLY>
__global__ __launch_bounds__(kSegThreads) void score_hyst_kernel(HystArgs a) {
  __shared__ int64_t lds[kSegThreads / 64];
  const int64_t tile = blockIdx.x;
  const int64_t base = tile * kSegTile + (int64_t)threadIdx.x * kSegItems;
  ItemRange r;
  item_ranges<BATCH>(a.clips, base, &r);
  int64_t key[kSegItems], mine = -1;
#pragma unroll
  for (int j = 0; j < kSegItems; ++j) {
    const int64_t w = base + j;
    key[j] = -1;
    if (w >= r.lo[j] && w < r.hi[j]) {
      const float s = a.s[w];
      if (s >= a.on) key[j] = 2 * w + 1;
      else if (!(s >= a.off)) key[j] = 2 * w;  // below off, or NaN
    }
    mine = OpMax()(mine, key[j]);
  }
  int64_t tot;
  int64_t prev = block_excl<true>(mine, OpMax(), (int64_t)-1, lds, &tot);
  if (!APPLY) {
    if (threadIdx.x == 0) {
      a.tile_last[tile] = tot;
      a.tile_first[tile] = kNone;
    }
    return;
  }
  prev = OpMax()(prev, a.carry_prev[tile]);
#pragma unroll
  for (int j = 0; j < kSegItems; ++j) {
    const int64_t w = base + j;
    if (w >= a.clips.n) break;
    prev = OpMax()(prev, key[j]);
    // a key from before the clip's first window is another clip's state
    const bool in = w >= r.lo[j] && w < r.hi[j];
    a.out[w] = in && prev >= 2 * r.lo[j] && (prev & 1) ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------
// Dilation
// ---------------------------------------------------------------------------
struct DilateArgs {
  const uint8_t* in;
  uint8_t* out;
  Clips clips;
  int active;
  int64_t before, after;  // pad_before, pad_after, each cut to n
  int64_t* tile_last;
  int64_t* tile_first;
  const int64_t* carry_prev;
  const int64_t* carry_next;
};

template <bool BATCH, bool APPLY>
__global__ __launch_bounds__(kSegThreads) void score_dilate_kernel(DilateArgs a) {
  __shared__ int64_t lds[kSegThreads / 64];
  const int64_t tile = blockIdx.x;
  const int64_t base = tile * kSegTile + (int64_t)threadIdx.x * kSegItems;
  ItemRange r;
  item_ranges<BATCH>(a.clips, base, &r);
  bool p[kSegItems];
  int64_t mine_last = -1, mine_first = kNone;
#pragma unroll
  for (int j = 0; j < kSegItems; ++j) {
    const int64_t w = base + j;
    p[j] = w >= r.lo[j] && w < r.hi[j] && a.in[w] == a.active;
    if (p[j]) {
      mine_last = w;
      if (mine_first == kNone) mine_first = w;
    }
  }
  int64_t last, first;
  int64_t prev = block_excl<true>(mine_last, OpMax(), (int64_t)-1, lds, &last);
  int64_t next = block_excl<false>(mine_first, OpMin(), kNone, lds, &first);
  if (!APPLY) {
    if (threadIdx.x == 0) {
      a.tile_last[tile] = last;
      a.tile_first[tile] = first;
    }
    return;
  }
  prev = OpMax()(prev, a.carry_prev[tile]);
  next = OpMin()(next, a.carry_next[tile]);
  int64_t nx[kSegItems];  // first active window at or after item j
#pragma unroll
  for (int j = kSegItems - 1; j >= 0; --j) {
    if (p[j]) next = base + j;
    nx[j] = next;
  }
#pragma unroll
  for (int j = 0; j < kSegItems; ++j) {
    const int64_t w = base + j;
    if (w >= a.clips.n) break;
    if (p[j]) prev = w;
    const bool in = w >= r.lo[j] && w < r.hi[j];
    const bool tail = prev >= r.lo[j] && w - prev <= a.after;   // speech ended at most pad_after ago
    const bool head = nx[j] < r.hi[j] && nx[j] - w <= a.before;  // speech starts within pad_before
    a.out[w] = in && (tail || head) ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------
// Reference labels
// ---------------------------------------------------------------------------
// Window i of a clip stands for frame i + 2; it is speech iff its centre
// sample lies in one of the clip's intervals [start, end): one binary search
// for the last interval that starts at or before the centre.  STRIDE 2: rows
// (start, end) of the one clip; STRIDE 3: rows (clip, start, end), clip k's
// the rows [clip_row0[k], clip_row0[k + 1]) (the last clip's end at n_iv).
template <int STRIDE>
__global__ __launch_bounds__(256) void reference_labels_kernel(const int64_t* __restrict__ iv, int64_t n_iv,
                                                               const int64_t* __restrict__ clip_row0, Clips clips,
                                                               int frame_size, int hop, uint8_t* __restrict__ out) {
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < clips.n;
       w += (int64_t)gridDim.x * blockDim.x) {
    int64_t i = w, lo = 0, hi = n_iv;
    bool in = true;
    if (STRIDE == 3) {
      const int64_t k = clips.find(w);
      int64_t c_lo = 0, c_hi = 0;
      if (k >= 0) clips.range(k, &c_lo, &c_hi);
      in = k >= 0 && w >= c_lo && w < c_hi;
      if (in) {
        i = w - c_lo;
        lo = clip_row0[k];
        hi = k + 1 < clips.n_clips ? clip_row0[k + 1] : n_iv;
        lo = lo < 0 ? 0 : lo > n_iv ? n_iv : lo;
        hi = hi < lo ? lo : hi > n_iv ? n_iv : hi;
      }
    }
    uint8_t v = 0;
    if (in) {
      const int64_t centre = (i + 2) * hop + frame_size / 2;
      int64_t found = -1;
      while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (iv[STRIDE * mid + STRIDE - 2] <= centre) found = mid, lo = mid + 1; else hi = mid;
      }
      v = found >= 0 && centre < iv[STRIDE * found + STRIDE - 1];
    }
    out[w] = v;
  }
}

// ---------------------------------------------------------------------------
// Histogram
// ---------------------------------------------------------------------------
constexpr int kHistThreads = 256;
constexpr int kHistMaxBins = VAD_SCORE_MAX_BINS;

__device__ __forceinline__ int score_bin(float s, int bins) {
  const float t = s * (float)bins;  // NaN fails both tests: bin 0
  return t >= (float)bins ? bins - 1 : t > 0.f ? (int)t : 0;
}

// hist[r * bins + b] += windows with ref == r (0 / 1; any other value is not
// counted) and bin b.  T float: b = score_bin; T uint8_t: b = the label, a
// label >= bins not counted.  The workgroup's counts are in LDS (32-bit: a
// workgroup sees fewer than 2^32 windows, the entry bounds n) and reach
// `hist` as 64-bit adds of the nonzero ones.  VEC: four windows per lane and
// load (both arrays aligned for it), the last n % 4 windows one by one.
template <typename T, bool VEC>
__global__ __launch_bounds__(kHistThreads) void score_hist_kernel(const T* __restrict__ x,
                                                                  const uint8_t* __restrict__ ref, int64_t n,
                                                                  int bins, unsigned long long* __restrict__ hist) {
  __shared__ unsigned int h[2 * kHistMaxBins];
  for (int i = threadIdx.x; i < 2 * bins; i += kHistThreads) h[i] = 0;
  __syncthreads();
  auto count = [&](T v, unsigned r) {
    int b;
    if constexpr (sizeof(T) == 4) b = score_bin(v, bins);
    else b = (int)v;
    if (r < 2u && b < bins) atomicAdd(&h[r * bins + b], 1u);
  };
  const int64_t t0 = (int64_t)blockIdx.x * kHistThreads + threadIdx.x, step = (int64_t)gridDim.x * kHistThreads;
  if (VEC) {
    typedef T Tx4 __attribute__((ext_vector_type(4)));
    const int64_t n4 = n / 4;
    for (int64_t q = t0; q < n4; q += step) {
      const Tx4 v = reinterpret_cast<const Tx4*>(x)[q];
      const uint32_t r = reinterpret_cast<const uint32_t*>(ref)[q];
      count(v.x, r & 255u);
      count(v.y, (r >> 8) & 255u);
      count(v.z, (r >> 16) & 255u);
      count(v.w, r >> 24);
    }
    for (int64_t i = n4 * 4 + t0; i < n; i += step) count(x[i], ref[i]);
  } else {
    for (int64_t i = t0; i < n; i += step) count(x[i], ref[i]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * bins; i += kHistThreads)
    if (h[i]) atomicAdd(&hist[i], (unsigned long long)h[i]);
}

template <typename T>
int histogram(const T* x, const uint8_t* ref, int64_t n, int bins, int max_bins, int64_t* hist, void* stream) {
  if (n < 0 || bins <= 0 || bins > max_bins || !hist) return VAD_EINVAL;
  if (n > (int64_t)1 << 38) return VAD_EINVAL;  // 32-bit counts per workgroup
  if (n == 0) return VAD_OK;
  if (!x || !ref || (reinterpret_cast<uintptr_t>(hist) & 7)) return VAD_EINVAL;
  if (overlap(hist, (size_t)2 * bins * 8, x, (size_t)n * sizeof(T)) || overlap(hist, (size_t)2 * bins * 8, ref, (size_t)n))
    return VAD_EINVAL;
  // a multiple of the CU count, and no more workgroups than there is work
  const int cus = num_cus();
  const int64_t want = (n + 4 * kHistThreads - 1) / (4 * kHistThreads);
  int64_t per_cu = (want + cus - 1) / cus;
  if (per_cu > 8) per_cu = 8;
  const dim3 grid((unsigned)(per_cu * cus));
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
  const bool vec = (reinterpret_cast<uintptr_t>(x) % (4 * sizeof(T))) == 0 && (reinterpret_cast<uintptr_t>(ref) & 3) == 0;
  if (vec) score_hist_kernel<T, true><<<grid, dim3(kHistThreads), 0, st>>>(x, ref, n, bins, h);
  else score_hist_kernel<T, false><<<grid, dim3(kHistThreads), 0, st>>>(x, ref, n, bins, h);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// Host side of the scans
// ---------------------------------------------------------------------------
// workspace: 4 tile arrays of int64 (tile last / first, carry prev / next)
size_t workspace_bytes(int64_t n) {
  if (n <= 0) return 0;
  return align_up(4 * sizeof(int64_t) * (size_t)n_tiles_of(n), 256);
}
bool ws_ok(const void* ws, size_t ws_bytes, int64_t n) {
  if (n <= 0) return true;
  if (n > (int64_t)1 << 40) return false;  // the tile count is a grid dimension
  return ws && (reinterpret_cast<uintptr_t>(ws) & 15) == 0 && ws_bytes >= workspace_bytes(n);
}
bool clips_ok(const int64_t* frame0, const int64_t* n_rows, int64_t n_clips) {
  return n_clips >= 0 && (n_clips == 0 || (frame0 && n_rows));
}

template <bool BATCH>
int score_labels(const float* scores, const Clips& clips, float on, float off, uint8_t* out, void* ws, size_t ws_bytes,
                 void* stream) {
  const int64_t n = clips.n;
  if (n < 0 || !(0.f <= off && off <= on && on <= 1.f)) return VAD_EINVAL;  // a NaN threshold fails too
  if (n == 0) return VAD_OK;
  if (!scores || !out || overlap(scores, (size_t)n * 4, out, (size_t)n)) return VAD_EINVAL;
  if (!ws_ok(ws, ws_bytes, n)) return VAD_EINVAL;
  if (overlap(ws, workspace_bytes(n), scores, (size_t)n * 4) || overlap(ws, workspace_bytes(n), out, (size_t)n))
    return VAD_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t nt = n_tiles_of(n);
  int64_t* t = static_cast<int64_t*>(ws);
  HystArgs a{scores, out, clips, on, off, t, t + nt, t + 2 * nt};
  score_hyst_kernel<BATCH, false><<<dim3((unsigned)nt), dim3(kSegThreads), 0, st>>>(a);
  seg_carry_kernel<<<dim3(1), dim3(kSegThreads), 0, st>>>(t, t + nt, nt, t + 2 * nt, t + 3 * nt);
  score_hyst_kernel<BATCH, true><<<dim3((unsigned)nt), dim3(kSegThreads), 0, st>>>(a);
  return (int)hipGetLastError();
}

template <bool BATCH>
int label_dilate(const uint8_t* labels, const Clips& clips, int active, int64_t pad_before, int64_t pad_after,
                 uint8_t* out, void* ws, size_t ws_bytes, void* stream) {
  const int64_t n = clips.n;
  if (n < 0 || pad_before < 0 || pad_after < 0 || active < 0 || active > 255) return VAD_EINVAL;
  if (n == 0) return VAD_OK;
  if (!labels || !out || overlap(labels, (size_t)n, out, (size_t)n)) return VAD_EINVAL;
  if (!ws_ok(ws, ws_bytes, n)) return VAD_EINVAL;
  if (overlap(ws, workspace_bytes(n), labels, (size_t)n) || overlap(ws, workspace_bytes(n), out, (size_t)n))
    return VAD_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t nt = n_tiles_of(n);
  int64_t* t = static_cast<int64_t*>(ws);
  DilateArgs a{labels, out, clips, active, pad_before < n ? pad_before : n, pad_after < n ? pad_after : n,
               t, t + nt, t + 2 * nt, t + 3 * nt};
  score_dilate_kernel<BATCH, false><<<dim3((unsigned)nt), dim3(kSegThreads), 0, st>>>(a);
  seg_carry_kernel<<<dim3(1), dim3(kSegThreads), 0, st>>>(t, t + nt, nt, t + 2 * nt, t + 3 * nt);
  score_dilate_kernel<BATCH, true><<<dim3((unsigned)nt), dim3(kSegThreads), 0, st>>>(a);
  return (int)hipGetLastError();
}

unsigned flat_grid(int64_t n, int per_cu) {
  int64_t blocks = (n + 255) / 256;
  const int64_t cap = (int64_t)per_cu * num_cus();
  return (unsigned)(blocks < cap ? blocks : cap);
}

template <int C>
void launch_logit_scores(const float* logits, int64_t n, int active, float* scores, hipStream_t st) {
  logit_scores_kernel<C><<<dim3(flat_grid(n, 8)), dim3(256), 0, st>>>(logits, n, active, scores);
}

}  // namespace

// The launchers of the tree entries (capi.hip owns the plan).
hipError_t launch_tree_row_scores(const TreeNode* nodes, int n_nodes, const float* node_score, const float* x,
                                  int64_t n, int dim, float* scores, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  tree_rows_score_kernel<<<dim3(flat_grid(n, 8)), dim3(256), 0, st>>>(nodes, n_nodes, node_score, x, n, dim, scores);
  return hipGetLastError();
}

hipError_t launch_tree_window_scores(const TreeNode* nodes, const TreeNodeC* cnodes, int n_nodes,
                                     const float* node_score, const float* mfcc, int64_t n_rows, int mfcc_n, int mode,
                                     float* scores, hipStream_t st) {
  if (n_rows <= 0) return hipSuccess;
  int64_t blocks = (n_rows + kTreeWin - 1) / kTreeWin;
  const int64_t cap = 4 * num_cus();
  if (blocks > cap) blocks = cap;
  const bool lds = cnodes && n_nodes <= kLdsNodes;  // tree_kernel.hip's rule
  const size_t smem = lds ? (size_t)n_nodes * sizeof(TreeNodeC) : 0;
  const dim3 grid((unsigned)blocks), block(256);
  if (mfcc_n == 13 && lds)
    tree_window_score_kernel<13, true><<<grid, block, smem, st>>>(nodes, cnodes, n_nodes, node_score, mfcc, n_rows,
                                                                  mfcc_n, mode, scores);
  else if (mfcc_n == 13)
    tree_window_score_kernel<13, false><<<grid, block, 0, st>>>(nodes, cnodes, n_nodes, node_score, mfcc, n_rows,
                                                                mfcc_n, mode, scores);
  else if (lds)
    tree_window_score_kernel<0, true><<<grid, block, smem, st>>>(nodes, cnodes, n_nodes, node_score, mfcc, n_rows,
                                                                 mfcc_n, mode, scores);
  else
    tree_window_score_kernel<0, false><<<grid, block, 0, st>>>(nodes, cnodes, n_nodes, node_score, mfcc, n_rows,
                                                               mfcc_n, mode, scores);
  return hipGetLastError();
}

}  // namespace vad

using namespace vad;

extern "C" {

int vad_scores_from_logits(const float* logits, int64_t n, int32_t n_classes, int32_t active, float* scores,
                           void* stream) {
  if (n < 0 || n_classes <= 0 || n_classes > VAD_SCORE_MAX_CLASSES || active < 0 || active >= n_classes)
    return VAD_EINVAL;
  if (n > INT64_MAX / 64) return VAD_EINVAL;
  if (n == 0) return VAD_OK;
  if (!logits || !scores || (reinterpret_cast<uintptr_t>(logits) & 3) || (reinterpret_cast<uintptr_t>(scores) & 3))
    return VAD_EINVAL;
  if (overlap(logits, (size_t)n * n_classes * 4, scores, (size_t)n * 4)) return VAD_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (n_classes) {
    case 1: launch_logit_scores<1>(logits, n, active, scores, st); break;
    case 2: launch_logit_scores<2>(logits, n, active, scores, st); break;
    case 3: launch_logit_scores<3>(logits, n, active, scores, st); break;
    case 4: launch_logit_scores<4>(logits, n, active, scores, st); break;
    case 5: launch_logit_scores<5>(logits, n, active, scores, st); break;
    case 6: launch_logit_scores<6>(logits, n, active, scores, st); break;
    case 7: launch_logit_scores<7>(logits, n, active, scores, st); break;
    default: launch_logit_scores<8>(logits, n, active, scores, st); break;
  }
  return (int)hipGetLastError();
}

size_t vad_scores_workspace_bytes(int64_t n) { return workspace_bytes(n); }

int vad_score_labels(const float* scores, int64_t n, float on, float off, uint8_t* out, void* ws, size_t ws_bytes,
                     void* stream) {
  return score_labels<false>(scores, Clips{nullptr, nullptr, 0, n}, on, off, out, ws, ws_bytes, stream);
}

int vad_label_dilate(const uint8_t* labels, int64_t n, int32_t active, int64_t pad_before, int64_t pad_after,
                     uint8_t* out, void* ws, size_t ws_bytes, void* stream) {
  return label_dilate<false>(labels, Clips{nullptr, nullptr, 0, n}, active, pad_before, pad_after, out, ws, ws_bytes,
                             stream);
}

int vad_batch_score_labels(const float* scores, int64_t n, const int64_t* frame0, const int64_t* n_rows,
                           int64_t n_clips, float on, float off, uint8_t* out, void* ws, size_t ws_bytes,
                           void* stream) {
  if (!clips_ok(frame0, n_rows, n_clips)) return VAD_EINVAL;
  return score_labels<true>(scores, Clips{frame0, n_rows, n_clips, n}, on, off, out, ws, ws_bytes, stream);
}

int vad_batch_label_dilate(const uint8_t* labels, int64_t n, const int64_t* frame0, const int64_t* n_rows,
                           int64_t n_clips, int32_t active, int64_t pad_before, int64_t pad_after, uint8_t* out,
                           void* ws, size_t ws_bytes, void* stream) {
  if (!clips_ok(frame0, n_rows, n_clips)) return VAD_EINVAL;
  return label_dilate<true>(labels, Clips{frame0, n_rows, n_clips, n}, active, pad_before, pad_after, out, ws,
                            ws_bytes, stream);
}

int vad_reference_labels(const int64_t* intervals, int64_t n_intervals, int64_t n, int32_t frame_size, int32_t hop,
                         uint8_t* out, void* stream) {
  if (n < 0 || n_intervals < 0 || frame_size <= 0 || hop <= 0) return VAD_EINVAL;
  if (n_intervals > INT64_MAX / 64 || n > INT64_MAX / 4 / hop) return VAD_EINVAL;
  if (n_intervals > 0 && (!intervals || (reinterpret_cast<uintptr_t>(intervals) & 7))) return VAD_EINVAL;
  if (n == 0) return VAD_OK;
  if (!out || overlap(out, (size_t)n, intervals, (size_t)n_intervals * 16)) return VAD_EINVAL;
  reference_labels_kernel<2><<<dim3(flat_grid(n, 8)), dim3(256), 0, static_cast<hipStream_t>(stream)>>>(
      intervals, n_intervals, nullptr, Clips{nullptr, nullptr, 0, n}, frame_size, hop, out);
  return (int)hipGetLastError();
}

int vad_batch_reference_labels(const int64_t* intervals, int64_t n_intervals, const int64_t* clip_row0,
                               const int64_t* frame0, const int64_t* n_rows, int64_t n_clips, int64_t n,
                               int32_t frame_size, int32_t hop, uint8_t* out, void* stream) {
  if (n < 0 || n_intervals < 0 || frame_size <= 0 || hop <= 0 || !clips_ok(frame0, n_rows, n_clips)) return VAD_EINVAL;
  if (n_intervals > INT64_MAX / 64 || n > INT64_MAX / 4 / hop) return VAD_EINVAL;
  if (n_clips > 0 && !clip_row0) return VAD_EINVAL;
  if (n_intervals > 0 && (!intervals || (reinterpret_cast<uintptr_t>(intervals) & 7))) return VAD_EINVAL;
  if (n == 0) return VAD_OK;
  if (!out || overlap(out, (size_t)n, intervals, (size_t)n_intervals * 24)) return VAD_EINVAL;
  reference_labels_kernel<3><<<dim3(flat_grid(n, 8)), dim3(256), 0, static_cast<hipStream_t>(stream)>>>(
      intervals, n_intervals, clip_row0, Clips{frame0, n_rows, n_clips, n}, frame_size, hop, out);
  return (int)hipGetLastError();
}

int vad_score_histogram_f32(const float* scores, const uint8_t* ref, int64_t n, int32_t bins, int64_t* hist,
                            void* stream) {
  if (reinterpret_cast<uintptr_t>(scores) & 3) return VAD_EINVAL;
  return histogram<float>(scores, ref, n, bins, kHistMaxBins, hist, stream);
}

int vad_score_histogram_u8(const uint8_t* labels, const uint8_t* ref, int64_t n, int32_t n_values, int64_t* hist,
                           void* stream) {
  return histogram<uint8_t>(labels, ref, n, n_values, 256, hist, stream);
}

}  // extern "C"
