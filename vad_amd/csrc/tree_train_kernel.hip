// Training the decision tree on the device (the reference fits an sklearn
// DecisionTreeClassifier in learning/decision_classifier_trainer.py:26-30 and
// chooses its parameters with a GridSearchCV over 112 settings in
// learning/cross_validation.py:20-27).
//
// The rule (Gini, best splitter, all features, unweighted rows) is sklearn
// 1.7.2's, made deterministic; DESIGN.md section 4 states it in full.  A node
// with n rows sorted by a feature has a candidate at position p (1 <= p < n)
// when x[p] > x[p-1] (float32, strict) and both sides keep min_samples_leaf
// rows; its score is (sum_k cL[k]^2) / nL + (sum_k cR[k]^2) / nR in IEEE
// double (integer sums exact, two divisions and one addition each rounded
// once); the largest score wins, then the lowest feature, then the lowest p.
//
// All jobs of a call (a job = a set of rows and its three parameters) grow
// level by level.  A segment is one (job, live node).  Per feature the device
// keeps one list of 8-byte entries {float32 value, label << 27 | row}: every
// job's rows sorted by that feature and grouped by live node, jobs in order,
// nodes in level order.  Segments occupy the same positions in every
// feature's list, so whatever depends only on the node (its base class
// counts, its rows' destinations) comes from a scan over the node table and
// is shared by the features.  A level is a fixed chain of launches over
// 2048-entry tiles:
//
//   tt_class_tiles   class counts of every (feature, tile)
//   tt_carry         exclusive scan of those over the tiles of a feature
//   tt_search        running counts -> scores -> per (tile, segment) best
//   tt_decide        one wave per segment: merge the bests, leaf conditions,
//                    threshold, children's class counts
//   tt_scan          one workgroup: exclusive scans over the node table
//   tt_emit          children's nodes, next level's segments
//   tt_mark          goes-left flag per row, from its position in the
//                    winning feature's list (never from comparing values)
//   tt_left_tiles, tt_carry, tt_partition
//                    stable partition of every list into the children's
//                    ranges; rows of leaves drop out
//
// No workgroup waits for another: every hand-over is a kernel boundary.  The
// only global atomics are integer adds (root class counts, splits per job),
// whose sums do not depend on order.  A job's table does not depend on the
// other jobs of the call: scores, winners and thresholds are functions of the
// segment's own rows, and bests are merged by an exact lexicographic maximum.
// The host reads two integers back per level (live segments and rows), which
// size the next level's launches and end the loop.
//
// Nodes are numbered in level order per job here (children adjacent);
// vad_amd/tree_train.py renumbers to sklearn's preorder on the host.
//
// Weighted builds (vad_tree_train_weighted; DESIGN.md section 4, "Integer row
// weights"): a uint8 weight per (job, row) takes the mask's place (weight 0:
// the row is not in the job).  Positions, n_node_samples and the three
// parameters go on counting distinct rows; the class counts, the divisors of
// the score and purity are weighted.  The 8-byte entries have no room for the
// weight, so the kernels that count gather weights[job * n + row], the job
// from the entry's segment.  A tile can hold 2048 * 255 of weight, so the
// packed counters of these builds are 32-bit fields, two per 64-bit word (WW
// words: 1, 2 or 4 for up to 2, 4 or 8 classes).  The unweighted kernels are
// the WW = 0 / WT = false instantiations and compile to what they were.
#include "vad_common.h"

#include <vector>

namespace vad {
namespace {

constexpr int kTT = 256;               // threads per workgroup
constexpr int kTI = 8;                 // entries per thread
constexpr int kTile = kTT * kTI;       // entries per tile
constexpr int kKP = VAD_TREE_TRAIN_MAX_CLASSES;  // class counters are padded to 8
constexpr int kSegLds = kTile / 2 + 2;  // live segments have >= 2 rows: at most this many meet a tile
constexpr unsigned kRowMask = (1u << VAD_TREE_TRAIN_ROW_BITS) - 1;
typedef unsigned long long u64;

struct Rec {  // best candidate of a segment among some tiles and features; score 0: none
  u64 score;  // bits of the non-negative double
  int f;
  int p;
};

struct Segs {  // one level's live segments (begin has n + 1 entries)
  int* begin;
  int* job;
  int* node;
  unsigned* cnt;   // [s][kKP]
  unsigned* base;  // [s][kKP] class counts of all earlier segments
};

struct Jobs {  // device copies of the descriptors and the per-job state
  const int* n;
  const int* off;      // first list position of the job's rows at level 0
  const int* md;
  const int* mss;
  const int* msl;
  const int* cap;
  const int* nodeoff;  // first node of the job in the output tables
  int* first;          // [2][J] segment range of the job, by level parity
  int* end;
  int* nn;             // [2][J] nodes so far
  int* splits;         // splits of this level
  int* ovf;
  unsigned* rootcnt;   // [J][kKP]
};

struct Tables {
  int32_t* feature;
  double* threshold;
  int32_t* left;
  int32_t* right;
  int32_t* leaf;
  uint8_t* nan_left;
  int32_t* n_node_samples;
  int32_t* depth;
  int32_t* value;
  int32_t* n_nodes;
  int32_t* status;
  int K;
};

template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* sh, T& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  T woff = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < kTT / 64; ++i) {
    const T x = sh[i];
    if (i < w) woff += x;
    tot += x;
  }
  __syncthreads();
  total = tot;
  return woff + inc - v;
}

__device__ __forceinline__ void load_items(const uint2* __restrict__ L, int q0, int lim, uint2 (&e)[kTI]) {
  if (q0 + kTI <= lim) {
    const uint4* p = reinterpret_cast<const uint4*>(L + q0);  // lists are 256-B aligned, q0 a multiple of 8
#pragma unroll
    for (int i = 0; i < kTI / 2; ++i) {
      const uint4 v = p[i];
      e[2 * i] = make_uint2(v.x, v.y);
      e[2 * i + 1] = make_uint2(v.z, v.w);
    }
  } else {
#pragma unroll
    for (int j = 0; j < kTI; ++j) e[j] = q0 + j < lim ? L[q0 + j] : make_uint2(0u, 0u);
  }
}

// largest s in [lo, hi] with begin[s] <= q (begin[lo] <= q)
__device__ __forceinline__ int seg_of(const int* begin, int lo, int hi, int q) {
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (begin[mid] <= q) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// first and last segment that meet the tile -> rng[0], rng[1]
__device__ __forceinline__ void tile_seg_range(const int* __restrict__ sbegin, int S, int tile0, int Tl, int* rng) {
  if (threadIdx.x == 0) rng[0] = seg_of(sbegin, 0, S - 1, tile0);
  if (threadIdx.x == 64) rng[1] = seg_of(sbegin, 0, S - 1, min(tile0 + kTile, Tl) - 1);
  __syncthreads();
}

__device__ __forceinline__ bool child_live(int depth, int n, unsigned maxc, int md, int mss, int msl) {
  return depth < md && n >= mss && n >= 2 * msl && (int)maxc < n;
}

// weighted: n counts distinct rows, W is the node's total weight
__device__ __forceinline__ bool child_live_w(int depth, int n, unsigned maxc, unsigned W, int md, int mss, int msl) {
  return depth < md && n >= mss && n >= 2 * msl && maxc < W;
}

// weighted class counters: 32-bit fields, two per word
template <int WW>
__device__ __forceinline__ void add_weight(u64 (&pk)[WW], unsigned lab, unsigned w) {
  const u64 v = (u64)w << (32 * (lab & 1));
#pragma unroll
  for (int i = 0; i < WW; ++i) pk[i] += (lab >> 1) == (unsigned)i ? v : 0ull;
}

// ---- set-up: the lists from the order of all rows and the jobs' masks --------
// (a job's weights serve as its mask: weight > 0)
template <bool APPLY>
__global__ __launch_bounds__(kTT) void tt_filter(const int32_t* __restrict__ order, const uint8_t* __restrict__ mask,
                                                 const float* __restrict__ x, const uint8_t* __restrict__ y, int n,
                                                 int F, int NTn, unsigned* __restrict__ ftile,
                                                 const int* __restrict__ joff, const int* __restrict__ jn,
                                                 uint2* __restrict__ list, int Tp) {
  __shared__ unsigned sh[kTT / 64];
  const int t = blockIdx.x, f = blockIdx.y, j = blockIdx.z;
  const int i0 = t * kTile + threadIdx.x * kTI;
  unsigned r[kTI], m[kTI], c = 0;
#pragma unroll
  for (int k = 0; k < kTI; ++k) {
    r[k] = i0 + k < n ? (unsigned)order[(size_t)f * n + i0 + k] : 0xffffffffu;
    m[k] = r[k] < (unsigned)n && (!mask || mask[(size_t)j * n + r[k]]);
    c += m[k];
  }
  unsigned tot;
  const unsigned ex = block_excl_scan(c, sh, tot);
  unsigned* slot = ftile + ((size_t)j * F + f) * NTn + t;
  if constexpr (!APPLY) {
    if (threadIdx.x == 0) *slot = tot;
  } else {
    unsigned d = *slot + ex;
#pragma unroll
    for (int k = 0; k < kTI; ++k)
      if (m[k]) {
        if (d < (unsigned)jn[j])
          list[(size_t)f * Tp + joff[j] + d] =
              make_uint2(__float_as_uint(x[(size_t)r[k] * F + f]), ((unsigned)(y[r[k]] & 7) << VAD_TREE_TRAIN_ROW_BITS) | r[k]);
        ++d;
      }
  }
}

// in-place exclusive scan over the tiles of each list: data[list][stride][W]
template <int W>
__global__ __launch_bounds__(kTT) void tt_carry(unsigned* __restrict__ data, int nt, int stride) {
  __shared__ unsigned sh[kTT / 64];
  unsigned* d = data + (size_t)blockIdx.x * stride * W;
  const int c = (nt + kTT - 1) / kTT;
  const int a = min(nt, (int)threadIdx.x * c), b = min(nt, a + c);
  unsigned acc[W];
#pragma unroll
  for (int w = 0; w < W; ++w) acc[w] = 0;
  for (int t = a; t < b; ++t)
#pragma unroll
    for (int w = 0; w < W; ++w) acc[w] += d[(size_t)t * W + w];
#pragma unroll
  for (int w = 0; w < W; ++w) {
    unsigned tot;
    acc[w] = block_excl_scan(acc[w], sh, tot);
  }
  for (int t = a; t < b; ++t)
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const unsigned v = d[(size_t)t * W + w];
      d[(size_t)t * W + w] = acc[w];
      acc[w] += v;
    }
}

__global__ __launch_bounds__(kTT) void tt_root_counts(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ y,
                                                      int n, unsigned* __restrict__ rootcnt) {
  __shared__ unsigned c[kKP];
  const int j = blockIdx.y;
  if (threadIdx.x < kKP) c[threadIdx.x] = 0;
  __syncthreads();
  for (int r = blockIdx.x * kTT + threadIdx.x; r < n; r += gridDim.x * kTT)
    if (!mask || mask[(size_t)j * n + r]) atomicAdd(&c[y[r] & 7], 1u);
  __syncthreads();
  if (threadIdx.x < kKP && c[threadIdx.x]) atomicAdd(&rootcnt[j * kKP + threadIdx.x], c[threadIdx.x]);
}

// weighted roots: class counts add the weights; rows[j] counts the rows with
// weight > 0 and wtot[j] their weight in 64 bits (the 32-bit class counts may
// wrap when the total is past the limit: tt_init refuses the job by wtot)
__global__ __launch_bounds__(kTT) void tt_root_counts_w(const uint8_t* __restrict__ wts, const uint8_t* __restrict__ y,
                                                        int n, unsigned* __restrict__ rootcnt, u64* __restrict__ wtot,
                                                        unsigned* __restrict__ rows) {
  __shared__ unsigned c[kKP + 1];
  const int j = blockIdx.y;
  if (threadIdx.x <= kKP) c[threadIdx.x] = 0;
  __syncthreads();
  unsigned mine = 0;
  for (int r = blockIdx.x * kTT + threadIdx.x; r < n; r += gridDim.x * kTT) {
    const unsigned w = wts[(size_t)j * n + r];
    if (w) {
      atomicAdd(&c[y[r] & 7], w);
      ++mine;
    }
  }
  if (mine) atomicAdd(&c[kKP], mine);
  __syncthreads();
  if (threadIdx.x < kKP && c[threadIdx.x]) {
    atomicAdd(&rootcnt[j * kKP + threadIdx.x], c[threadIdx.x]);
    atomicAdd(&wtot[j], (u64)c[threadIdx.x]);
  }
  if (threadIdx.x == kKP && c[kKP]) atomicAdd(&rows[j], c[kKP]);
}

__device__ __forceinline__ void write_leaf_node(const Tables& o, int at, int cap_left, const unsigned* c, int n,
                                                int depth) {
  if (cap_left <= 0) return;
  unsigned best = 0;
  int arg = 0;
  for (int k = 0; k < o.K; ++k) {
    if (c[k] > best) { best = c[k]; arg = k; }
    o.value[(size_t)at * o.K + k] = (int)c[k];
  }
  o.feature[at] = -1;
  o.threshold[at] = -2.0;
  o.left[at] = -1;
  o.right[at] = -1;
  o.leaf[at] = arg;
  o.nan_left[at] = 0;
  o.n_node_samples[at] = n;
  o.depth[at] = depth;
}

// roots: node 0 of every job and the segments of level 0 (one per job)
template <bool WT>
__global__ __launch_bounds__(kTT) void tt_init(Jobs jb, int J, int T, Segs sg, Tables o, const u64* __restrict__ wtot,
                                               const unsigned* __restrict__ rows) {
  const int j = blockIdx.x * kTT + threadIdx.x;
  if (j == 0) sg.begin[J] = T;
  if (j >= J) return;
  unsigned c[kKP], base[kKP], n = 0;
  for (int k = 0; k < kKP; ++k) {
    c[k] = jb.rootcnt[j * kKP + k];
    n += c[k];
    base[k] = 0;
  }
  for (int i = 0; i < j; ++i)
    for (int k = 0; k < kKP; ++k) base[k] += jb.rootcnt[i * kKP + k];
  bool bad;
  int heavy = 0;
  if constexpr (WT) {
    bad = rows[j] != (unsigned)jb.n[j];
    heavy = wtot[j] > (u64)VAD_TREE_TRAIN_MAX_WEIGHT || wtot[j] != (u64)n ? VAD_TREE_TRAIN_BAD_WEIGHT : 0;
  } else {
    bad = n != (unsigned)jb.n[j];
  }
  for (int k = o.K; k < kKP; ++k) bad |= c[k] != 0;  // a label >= n_classes
  o.status[j] = (bad ? VAD_TREE_TRAIN_BAD_ROWS : 0) | heavy;
  write_leaf_node(o, jb.nodeoff[j], jb.cap[j], c, jb.n[j], 0);
  o.n_nodes[j] = 1;
  sg.begin[j] = jb.off[j];
  sg.job[j] = j;
  sg.node[j] = 0;
  for (int k = 0; k < kKP; ++k) {
    sg.cnt[j * kKP + k] = c[k];
    sg.base[j * kKP + k] = base[k];
  }
  jb.first[j] = j;
  jb.end[j] = j + 1;
  jb.nn[j] = 1;
  jb.splits[j] = 0;
  jb.ovf[j] = 0;
}

// ---- split search ------------------------------------------------------------
__device__ __forceinline__ void pack_labels(const uint2 (&e)[kTI], int q0, int Tl, u64 (&pk)[2]) {
  pk[0] = pk[1] = 0;
#pragma unroll
  for (int j = 0; j < kTI; ++j)
    if (q0 + j < Tl) {
      const unsigned lab = (e[j].y >> VAD_TREE_TRAIN_ROW_BITS) & 7;
      pk[lab >> 2] += 1ull << (16 * (lab & 3));
    }
}

__global__ __launch_bounds__(kTT) void tt_class_tiles(const uint2* __restrict__ list, int Tp, int Tl,
                                                      unsigned* __restrict__ tilecnt, int NT) {
  __shared__ u64 sh[kTT / 64];
  const int t = blockIdx.x, f = blockIdx.y;
  const int q0 = t * kTile + threadIdx.x * kTI;
  uint2 e[kTI];
  load_items(list + (size_t)f * Tp, q0, Tl, e);
  u64 pk[2], tot[2];
  pack_labels(e, q0, Tl, pk);
  block_excl_scan(pk[0], sh, tot[0]);
  block_excl_scan(pk[1], sh, tot[1]);
  if (threadIdx.x < kKP)
    tilecnt[((size_t)f * NT + t) * kKP + threadIdx.x] =
        (unsigned)(tot[threadIdx.x >> 2] >> (16 * (threadIdx.x & 3))) & 0xffffu;
}

// the weighted class counts of every (feature, tile): the weight of an entry
// is gathered by (the job of its segment, its row)
template <int WW>
__global__ __launch_bounds__(kTT) void tt_class_tiles_w(const uint2* __restrict__ list, int Tp, int Tl,
                                                        unsigned* __restrict__ tilecnt, int NT,
                                                        const uint8_t* __restrict__ wts, int n,
                                                        const int* __restrict__ sbegin, const int* __restrict__ sjob,
                                                        int S) {
  __shared__ u64 sh[kTT / 64];
  __shared__ int rng[2];
  const int t = blockIdx.x, f = blockIdx.y;
  const int tile0 = t * kTile, q0 = tile0 + threadIdx.x * kTI;
  tile_seg_range(sbegin, S, tile0, Tl, rng);
  uint2 e[kTI];
  load_items(list + (size_t)f * Tp, q0, Tl, e);
  int s = q0 < Tl ? seg_of(sbegin, rng[0], rng[1], q0) : rng[1];
  int send = sbegin[s + 1], job = sjob[s];
  u64 pk[WW], tot[WW];
#pragma unroll
  for (int i = 0; i < WW; ++i) pk[i] = 0;
#pragma unroll
  for (int j = 0; j < kTI; ++j)
    if (q0 + j < Tl) {
      while (q0 + j >= send && s + 1 < S) {
        ++s;
        send = sbegin[s + 1];
        job = sjob[s];
      }
      const unsigned r = e[j].y & kRowMask;
      const unsigned w = r < (unsigned)n ? wts[(size_t)job * n + r] : 0u;
      add_weight<WW>(pk, (e[j].y >> VAD_TREE_TRAIN_ROW_BITS) & 7, w);
    }
#pragma unroll
  for (int i = 0; i < WW; ++i) block_excl_scan(pk[i], sh, tot[i]);
  if (threadIdx.x < kKP) {
    u64 word = 0;
#pragma unroll
    for (int i = 0; i < WW; ++i) word = (int)(threadIdx.x >> 1) == i ? tot[i] : word;
    tilecnt[((size_t)f * NT + t) * kKP + threadIdx.x] = (unsigned)(word >> (32 * (threadIdx.x & 1)));
  }
}

// NW: 64-bit words of packed 16-bit class counters (1: up to 4 classes).
// MASKED: jfmask[job] has bit f set when the job may split on feature f
// (vad_tree_train_features); a feature whose bit is clear in a segment's job
// mask contributes no candidate to that segment, and a feature no segment of
// the tile may use is not searched at all.  !MASKED is the kernel as it was.
// WW > 0: the weighted build (NW is then unused): WW words of 32-bit fields,
// running counts add the gathered weights, the divisors are the weighted
// totals of the two sides; positions and min_samples_leaf stay distinct rows.
template <int NW, bool MASKED, int WW>
__global__ __launch_bounds__(kTT) void tt_search(const uint2* __restrict__ list, int Tp, int Tl, int F, int fc,
                                                 const unsigned* __restrict__ tilecnt, int NT, Segs sg, int S,
                                                 const int* __restrict__ jmsl, const u64* __restrict__ jfmask,
                                                 Rec* __restrict__ segbest, int Smax, Rec* __restrict__ tilefirst,
                                                 const uint8_t* __restrict__ wts, int n) {
  constexpr int KK = WW ? 2 * WW : 4 * NW;
  __shared__ u64 cur_score[kSegLds], best_score[kSegLds], best_key[kSegLds];
  __shared__ unsigned cur_p[kSegLds];
  __shared__ int seg_b[kSegLds + 1];
  __shared__ float lastv[kTT];
  __shared__ u64 sh[kTT / 64];
  __shared__ int rng[2];
  const int tid = threadIdx.x, lane = tid & 63;
  const int t = blockIdx.x, y = blockIdx.y;
  const int tile0 = t * kTile, q0 = tile0 + tid * kTI;
  tile_seg_range(sg.begin, S, tile0, Tl, rng);
  const int sLo = rng[0];
  const int NS = min(rng[1] - sLo + 1, kSegLds);
  for (int i = tid; i < NS; i += kTT) {
    cur_score[i] = 0;
    best_score[i] = 0;
    best_key[i] = 0;
    cur_p[i] = 0xffffffffu;
  }
  for (int i = tid; i <= NS; i += kTT) seg_b[i] = sg.begin[sLo + i];
  u64* seg_fm = nullptr;  // [NS] the segments' feature masks, then their union
  if constexpr (MASKED) {
    __shared__ u64 fm_s[kSegLds + 1];
    seg_fm = fm_s;
    if (tid == 0) fm_s[NS] = 0;
    __syncthreads();
    for (int i = tid; i < NS; i += kTT) {
      const u64 m = jfmask[sg.job[sLo + i]];
      fm_s[i] = m;
      atomicOr(&fm_s[NS], m);
    }
  }
  int* seg_j = nullptr;  // [NS] the segments' jobs (weighted: the row of the weight table)
  if constexpr (WW > 0) {
    __shared__ int sj_s[kSegLds];
    seg_j = sj_s;
    for (int i = tid; i < NS; i += kTT) sj_s[i] = sg.job[sLo + i];
  }
  __syncthreads();

  // the segment of every item (the same in all features); items past the
  // end or past the LDS table take no part
  int sl[kTI];
  {
    int li = q0 < Tl ? seg_of(seg_b, 0, NS - 1, q0) : 0;
#pragma unroll
    for (int j = 0; j < kTI; ++j) {
      while (li + 1 < NS && q0 + j < Tl && q0 + j >= seg_b[li + 1]) ++li;
      sl[j] = li;
    }
  }
  const bool in_table = q0 >= Tl || min(q0 + kTI, Tl) <= seg_b[NS];
  const bool one_seg = sl[0] == sl[kTI - 1];
  const bool wave_one = __all(one_seg && sl[0] == __shfl(sl[0], 0));

  int c_li = -1, c_begin = 0, c_n = 0, c_msl = 0;
  unsigned c_base[KK], c_cnt[KK];
#pragma unroll
  for (int k = 0; k < KK; ++k) c_base[k] = c_cnt[k] = 0;

  const int f_end = min(F, (y + 1) * fc);
  for (int f = y * fc; f < f_end; ++f) {
    if constexpr (MASKED) {
      if (!((seg_fm[NS] >> f) & 1)) continue;  // uniform: no segment of the tile may use f
    }
    const uint2* L = list + (size_t)f * Tp;
    uint2 e[kTI];
    load_items(L, q0, Tl, e);
    unsigned run[KK];
    const unsigned* tc = tilecnt + ((size_t)f * NT + t) * kKP;
    unsigned wv[WW ? kTI : 1];  // weighted: the items' weights
    if constexpr (WW > 0) {
      u64 pw[WW], ex[WW], tot;
#pragma unroll
      for (int i = 0; i < WW; ++i) pw[i] = 0;
#pragma unroll
      for (int j = 0; j < kTI; ++j) {
        const unsigned r = e[j].y & kRowMask;
        wv[j] = q0 + j < Tl && in_table && r < (unsigned)n ? wts[(size_t)seg_j[sl[j]] * n + r] : 0u;
        add_weight<WW>(pw, (e[j].y >> VAD_TREE_TRAIN_ROW_BITS) & 7, wv[j]);
      }
#pragma unroll
      for (int i = 0; i < WW; ++i) ex[i] = block_excl_scan(pw[i], sh, tot);
#pragma unroll
      for (int k = 0; k < KK; ++k) run[k] = tc[k] + (unsigned)(ex[k >> 1] >> (32 * (k & 1)));
    } else {
      u64 pk[2], ex[NW], tot;
      pack_labels(e, q0, Tl, pk);
#pragma unroll
      for (int w = 0; w < NW; ++w) ex[w] = block_excl_scan(pk[w], sh, tot);
#pragma unroll
      for (int k = 0; k < KK; ++k) run[k] = tc[k] + ((unsigned)(ex[k >> 2] >> (16 * (k & 3))) & 0xffffu);
    }
    lastv[tid] = __uint_as_float(e[kTI - 1].x);
    __syncthreads();
    float pv = tid ? lastv[tid - 1] : (q0 > 0 && q0 < Tl ? __uint_as_float(L[q0 - 1].x) : 0.f);

    double sc[kTI];
#pragma unroll
    for (int j = 0; j < kTI; ++j) {
      const int q = q0 + j;
      double score = 0.0;
      if (q < Tl && in_table) {
        const int li = sl[j];
        if (li != c_li) {
          c_li = li;
          c_begin = seg_b[li];
          c_n = seg_b[li + 1] - c_begin;
          const int s = sLo + li;
          c_msl = jmsl[sg.job[s]];
#pragma unroll
          for (int k = 0; k < KK; ++k) {
            c_base[k] = sg.base[(size_t)s * kKP + k];
            c_cnt[k] = sg.cnt[(size_t)s * kKP + k];
          }
        }
        const float v = __uint_as_float(e[j].x);
        const int p = q - c_begin;
        if (p >= 1 && v > pv && p >= c_msl && c_n - p >= c_msl) {
          u64 sL = 0, sR = 0, wL = 0, wR = 0;
#pragma unroll
          for (int k = 0; k < KK; ++k) {
            const u64 a = run[k] - c_base[k];
            const u64 b = c_cnt[k] - a;
            sL += a * a;
            sR += b * b;
            wL += a;
            wR += b;
          }
          if constexpr (WW > 0) score = (double)sL / (double)wL + (double)sR / (double)wR;
          else score = (double)sL / (double)p + (double)sR / (double)(c_n - p);
        }
        const unsigned lab = (e[j].y >> VAD_TREE_TRAIN_ROW_BITS) & 7;
#pragma unroll
        for (int k = 0; k < KK; ++k) {
          if constexpr (WW > 0) run[k] += lab == (unsigned)k ? wv[j] : 0u;
          else run[k] += lab == (unsigned)k;
        }
        pv = v;
      }
      sc[j] = score;
    }

    // the feature's best score per segment (scores are positive doubles:
    // their bit patterns order as integers), then the lowest p that has it
    {
      int rs = sl[0];
      double rm = 0.0;
#pragma unroll
      for (int j = 0; j < kTI; ++j) {
        if (sl[j] != rs) {
          if (rm > 0.0) atomicMax(&cur_score[rs], (u64)__double_as_longlong(rm));
          rs = sl[j];
          rm = 0.0;
        }
        rm = fmax(rm, sc[j]);
      }
      if (wave_one) {
#pragma unroll
        for (int d = 32; d; d >>= 1) rm = fmax(rm, __shfl_xor(rm, d));
        if (lane != 0) rm = 0.0;
      }
      if (rm > 0.0) atomicMax(&cur_score[rs], (u64)__double_as_longlong(rm));
    }
    __syncthreads();
    {
      int rs = sl[0];
      u64 top = cur_score[rs];
      unsigned pm = 0xffffffffu;
#pragma unroll
      for (int j = 0; j < kTI; ++j) {
        if (sl[j] != rs) {
          if (pm != 0xffffffffu) atomicMin(&cur_p[rs], pm);
          rs = sl[j];
          top = cur_score[rs];
          pm = 0xffffffffu;
        }
        if (sc[j] > 0.0 && (u64)__double_as_longlong(sc[j]) == top) pm = min(pm, (unsigned)(q0 + j - seg_b[rs]));
      }
      if (wave_one) {
#pragma unroll
        for (int d = 32; d; d >>= 1) pm = min(pm, (unsigned)__shfl_xor((int)pm, d));
        if (lane != 0) pm = 0xffffffffu;
      }
      if (pm != 0xffffffffu) atomicMin(&cur_p[rs], pm);
    }
    __syncthreads();
    // features come in rising order: only a strictly larger score replaces
    for (int i = tid; i < NS; i += kTT) {
      const u64 cs = cur_score[i];
      bool take = cs > best_score[i];
      if constexpr (MASKED) take = take && ((seg_fm[i] >> f) & 1);
      if (take) {
        best_score[i] = cs;
        best_key[i] = ((u64)(unsigned)f << 32) | cur_p[i];
      }
      cur_score[i] = 0;
      cur_p[i] = 0xffffffffu;
    }
    __syncthreads();
  }

  // a segment that began in an earlier tile reports through the tile's slot
  const bool carried = seg_b[0] < tile0;
  for (int i = tid; i < NS; i += kTT) {
    Rec r;
    r.score = best_score[i];
    r.f = (int)(best_key[i] >> 32);
    r.p = (int)(unsigned)best_key[i];
    if (i == 0 && carried) tilefirst[(size_t)y * NT + t] = r;
    else if (sLo + i < Smax) segbest[(size_t)y * Smax + sLo + i] = r;
  }
  if (tid == 0 && !carried) {
    Rec r;
    r.score = 0;
    r.f = 0;
    r.p = 0;
    tilefirst[(size_t)y * NT + t] = r;
  }
}

// ---- decide: one wave per segment --------------------------------------------
// WT: the weighted build (purity by the total weight, children's class counts weighted)
template <bool WT>
__global__ __launch_bounds__(kTT) void tt_decide(const uint2* __restrict__ list, int Tp, Segs sg, int S, int level,
                                                 Jobs jb, const unsigned* __restrict__ tilecnt, int NT,
                                                 const Rec* __restrict__ segbest, int Smax,
                                                 const Rec* __restrict__ tilefirst, int ny, int* __restrict__ dec,
                                                 int* __restrict__ bf, int* __restrict__ bp,
                                                 unsigned* __restrict__ cl, Tables o,
                                                 const uint8_t* __restrict__ wts, int nrows) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * (kTT / 64) + (threadIdx.x >> 6);
  if (s >= S) return;
  const int begin = sg.begin[s], n = sg.begin[s + 1] - begin, job = sg.job[s];
  const int md = jb.md[job], mss = jb.mss[job], msl = jb.msl[job];
  unsigned cnt[kKP], maxc = 0, W = 0;
#pragma unroll
  for (int k = 0; k < kKP; ++k) {
    cnt[k] = sg.cnt[(size_t)s * kKP + k];
    maxc = max(maxc, cnt[k]);
    W += cnt[k];
  }
  if (lane == 0) dec[s] = 0;
  if constexpr (WT) {
    if (!child_live_w(level, n, maxc, W, md, mss, msl)) return;
  } else {
    if (!child_live(level, n, maxc, md, mss, msl)) return;
  }

  // exact lexicographic maximum of the records: score, then lowest (f, p)
  const int t0 = begin / kTile, nt = (begin + n - 1) / kTile - t0 + 1;
  u64 bs = 0, bk = ~0ull;
  for (int i = lane; i < ny * nt; i += 64) {
    const int y = i / nt, r = i - y * nt;
    const Rec rec = r == 0 ? segbest[(size_t)y * Smax + s] : tilefirst[(size_t)y * NT + t0 + r];
    const u64 key = ((u64)(unsigned)rec.f << 32) | (unsigned)rec.p;
    if (rec.score > bs || (rec.score == bs && rec.score != 0 && key < bk)) {
      bs = rec.score;
      bk = key;
    }
  }
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    const u64 os = __shfl_xor(bs, d), ok = __shfl_xor(bk, d);
    if (os > bs || (os == bs && ok < bk)) {
      bs = os;
      bk = ok;
    }
  }
  if (bs == 0) return;  // no valid candidate: a leaf
  const int f = (int)(bk >> 32), p = (int)(unsigned)bk;
  if (f < 0 || p < 1 || p >= n) return;  // (cannot happen)
  const uint2* L = list + (size_t)f * Tp;
  const int q = begin + p;

  // left class counts: the running counts at q less the segment's base
  const int tq = q / kTile, lo = max(tq * kTile, begin);
  u64 pk[2] = {0, 0}, pw[4] = {0, 0, 0, 0};
  for (int i = lo + lane; i < q; i += 64) {
    const unsigned ey = L[i].y, lab = (ey >> VAD_TREE_TRAIN_ROW_BITS) & 7;
    if constexpr (WT) {
      const unsigned r = ey & kRowMask;
      add_weight<4>(pw, lab, r < (unsigned)nrows ? wts[(size_t)job * nrows + r] : 0u);
    } else {
      pk[lab >> 2] += 1ull << (16 * (lab & 3));
    }
  }
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    if constexpr (WT) {
#pragma unroll
      for (int i = 0; i < 4; ++i) pw[i] += __shfl_xor(pw[i], d);
    } else {
      pk[0] += __shfl_xor(pk[0], d);
      pk[1] += __shfl_xor(pk[1], d);
    }
  }
  unsigned cL[kKP], maxL = 0, maxR = 0, WL = 0;
#pragma unroll
  for (int k = 0; k < kKP; ++k) {
    unsigned v = WT ? (unsigned)(pw[k >> 1] >> (32 * (k & 1))) : (unsigned)(pk[k >> 2] >> (16 * (k & 3))) & 0xffffu;
    if (begin < tq * kTile) v += tilecnt[((size_t)f * NT + tq) * kKP + k] - sg.base[(size_t)s * kKP + k];
    cL[k] = min(v, cnt[k]);
    maxL = max(maxL, cL[k]);
    maxR = max(maxR, cnt[k] - cL[k]);
    WL += cL[k];
  }
  if (lane != 0) return;
  const double x0 = (double)__uint_as_float(L[q - 1].x), x1 = (double)__uint_as_float(L[q].x);
  double thr = x0 / 2.0 + x1 / 2.0;
  if (thr == x1 || thr == INFINITY || thr == -INFINITY) thr = x0;
  const int nL = p, nR = n - p;
  const int at = jb.nodeoff[job] + sg.node[s];
  if (sg.node[s] < jb.cap[job]) {
    o.feature[at] = f;
    o.threshold[at] = thr;
    o.nan_left[at] = nL > nR;
  }
  if constexpr (WT)
    dec[s] = 1 | (child_live_w(level + 1, nL, maxL, WL, md, mss, msl) ? 2 : 0) |
             (child_live_w(level + 1, nR, maxR, W - WL, md, mss, msl) ? 4 : 0);
  else
    dec[s] = 1 | (child_live(level + 1, nL, maxL, md, mss, msl) ? 2 : 0) |
             (child_live(level + 1, nR, maxR, md, mss, msl) ? 4 : 0);
  bf[s] = f;
  bp[s] = p;
#pragma unroll
  for (int k = 0; k < kKP; ++k) cl[(size_t)s * kKP + k] = cL[k];
  atomicAdd(&jb.splits[job], 1);
}

// ---- scans over the node table: one workgroup --------------------------------
// E[v][s], v = 0 splits, 1 next level's segments, 2 rows kept, 3 rows that go
// left, 4.. kept class counts; E[v][S] = the totals.
constexpr int kScanV = 4 + kKP;
__global__ __launch_bounds__(kTT) void tt_scan(Segs sg, int S, Jobs jb, int J, int par, const int* __restrict__ dec,
                                               const int* __restrict__ bp, const unsigned* __restrict__ cl,
                                               unsigned* __restrict__ E, int Estride, int* __restrict__ summary,
                                               int32_t* __restrict__ status) {
  __shared__ unsigned sh[kTT / 64];
  for (int j = threadIdx.x; j < J; j += kTT) {
    const int ov = jb.nn[par * J + j] + 2 * jb.splits[j] > jb.cap[j];
    jb.ovf[j] = ov;
    if (ov) status[j] |= VAD_TREE_TRAIN_OVERFLOW;
  }
  __syncthreads();
  const int c = (S + kTT - 1) / kTT;
  const int a = min(S, (int)threadIdx.x * c), b = min(S, a + c);
  unsigned acc[kScanV];
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 0) {
#pragma unroll
      for (int v = 0; v < kScanV; ++v) acc[v] = 0;
    } else {
#pragma unroll
      for (int v = 0; v < kScanV; ++v) {
        unsigned tot;
        acc[v] = block_excl_scan(acc[v], sh, tot);
        if (threadIdx.x == 0) {
          E[(size_t)v * Estride + S] = tot;
          if (v == 1) summary[0] = (int)tot;
          if (v == 2) summary[1] = (int)tot;
        }
      }
    }
    for (int s = a; s < b; ++s) {
      int d = dec[s];
      if (jb.ovf[sg.job[s]]) d = 0;
      unsigned val[kScanV];
#pragma unroll
      for (int v = 0; v < kScanV; ++v) val[v] = 0;
      if (d & 1) {
        const unsigned n = sg.begin[s + 1] - sg.begin[s], nL = bp[s], lL = (d >> 1) & 1, lR = (d >> 2) & 1;
        val[0] = 1;
        val[1] = lL + lR;
        val[2] = lL * nL + lR * (n - nL);
        val[3] = nL;
#pragma unroll
        for (int k = 0; k < kKP; ++k) {
          const unsigned cLk = cl[(size_t)s * kKP + k];
          val[4 + k] = lL * cLk + lR * (sg.cnt[(size_t)s * kKP + k] - cLk);
        }
      }
#pragma unroll
      for (int v = 0; v < kScanV; ++v) {
        if (pass) E[(size_t)v * Estride + s] = acc[v];
        acc[v] += val[v];
      }
    }
  }
}

// children's nodes and the next level's segments; threads past S: the jobs
__global__ __launch_bounds__(kTT) void tt_emit(Segs sg, int S, int level, Jobs jb, int J, int par,
                                               const int* __restrict__ dec, const int* __restrict__ bp,
                                               const unsigned* __restrict__ cl, const unsigned* __restrict__ E,
                                               int Estride, Segs nx, int Smax, Tables o) {
  const int i = blockIdx.x * kTT + threadIdx.x;
  const unsigned* Esp = E;
  const unsigned* Esg = E + (size_t)Estride;
  const unsigned* Erw = E + (size_t)2 * Estride;
  if (i >= S) {
    const int j = i - S;
    if (j == 0) nx.begin[min((int)Esg[S], Smax)] = (int)Erw[S];
    if (j >= J) return;
    const int f0 = jb.first[par * J + j], e0 = jb.end[par * J + j];
    const int nn = jb.nn[par * J + j] + (jb.ovf[j] ? 0 : 2 * (int)(Esp[e0] - Esp[f0]));
    jb.nn[(par ^ 1) * J + j] = nn;
    jb.first[(par ^ 1) * J + j] = (int)Esg[f0];
    jb.end[(par ^ 1) * J + j] = (int)Esg[e0];
    jb.splits[j] = 0;
    o.n_nodes[j] = nn;
    return;
  }
  const int s = i, d = dec[s];
  if (!(d & 1)) return;
  const int job = sg.job[s], cap = jb.cap[job];
  const int at = jb.nodeoff[job] + sg.node[s];
  if (jb.ovf[job]) {  // the job stops: this node stays the leaf it was created as
    if (sg.node[s] < cap) {
      o.feature[at] = -1;
      o.threshold[at] = -2.0;
      o.nan_left[at] = 0;
    }
    return;
  }
  const int lid = jb.nn[par * J + job] + 2 * (int)(Esp[s] - Esp[jb.first[par * J + job]]);
  if (lid + 1 >= cap || sg.node[s] >= cap) return;  // (the overflow test above covers it)
  const int n = sg.begin[s + 1] - sg.begin[s], nL = bp[s], nR = n - nL;
  unsigned cL[kKP], cR[kKP];
#pragma unroll
  for (int k = 0; k < kKP; ++k) {
    cL[k] = cl[(size_t)s * kKP + k];
    cR[k] = sg.cnt[(size_t)s * kKP + k] - cL[k];
  }
  o.left[at] = lid;
  o.right[at] = lid + 1;
  write_leaf_node(o, jb.nodeoff[job] + lid, cap - lid, cL, nL, level + 1);
  write_leaf_node(o, jb.nodeoff[job] + lid + 1, cap - lid - 1, cR, nR, level + 1);
  int ns = (int)Esg[s], row = (int)Erw[s];
  const unsigned* Ec = E + (size_t)4 * Estride;
  const int lL = (d >> 1) & 1, lR = (d >> 2) & 1;
  if (lL && ns < Smax) {
    nx.begin[ns] = row;
    nx.job[ns] = job;
    nx.node[ns] = lid;
#pragma unroll
    for (int k = 0; k < kKP; ++k) {
      nx.cnt[(size_t)ns * kKP + k] = cL[k];
      nx.base[(size_t)ns * kKP + k] = Ec[(size_t)k * Estride + s];
    }
    ++ns;
    row += nL;
  }
  if (lR && ns < Smax) {
    nx.begin[ns] = row;
    nx.job[ns] = job;
    nx.node[ns] = lid + 1;
#pragma unroll
    for (int k = 0; k < kKP; ++k) {
      nx.cnt[(size_t)ns * kKP + k] = cR[k];
      nx.base[(size_t)ns * kKP + k] = Ec[(size_t)k * Estride + s] + (lL ? cL[k] : 0);
    }
  }
}

// ---- mark and partition ------------------------------------------------------
__global__ __launch_bounds__(kTT) void tt_mark(const uint2* __restrict__ list, int Tp, int Tl, Segs sg, int S,
                                               const int* __restrict__ jovf, const int* __restrict__ dec,
                                               const int* __restrict__ bf, const int* __restrict__ bp, int n,
                                               uint8_t* __restrict__ flags) {
  __shared__ int rng[2];
  const int tile0 = blockIdx.x * kTile;
  tile_seg_range(sg.begin, S, tile0, Tl, rng);
  for (int q = tile0 + threadIdx.x; q < min(tile0 + kTile, Tl); q += kTT) {
    const int s = seg_of(sg.begin, rng[0], rng[1], q);
    const int job = sg.job[s];
    const bool split = (dec[s] & 1) && !jovf[job];
    const uint2 e = list[(size_t)(split ? bf[s] : 0) * Tp + q];
    const unsigned r = e.y & kRowMask;
    if (r < (unsigned)n) flags[(size_t)job * n + r] = split && q - sg.begin[s] < bp[s];
  }
}

template <bool APPLY>
__global__ __launch_bounds__(kTT) void tt_partition(const uint2* __restrict__ list, uint2* __restrict__ next, int Tp,
                                                    int Tl, int Tn, Segs sg, int S, const int* __restrict__ jovf,
                                                    const int* __restrict__ dec, const int* __restrict__ bp,
                                                    const unsigned* __restrict__ E, int Estride, int n,
                                                    const uint8_t* __restrict__ flags, unsigned* __restrict__ ptile,
                                                    int NT) {
  __shared__ unsigned sh[kTT / 64];
  __shared__ int rng[2];
  const int t = blockIdx.x, f = blockIdx.y;
  const int tile0 = t * kTile, q0 = tile0 + threadIdx.x * kTI;
  tile_seg_range(sg.begin, S, tile0, Tl, rng);
  uint2 e[kTI];
  load_items(list + (size_t)f * Tp, q0, Tl, e);
  int s = q0 < Tl ? seg_of(sg.begin, rng[0], rng[1], q0) : rng[1];
  int send = sg.begin[s + 1], job = sg.job[s];
  unsigned fl[kTI], c = 0;
#pragma unroll
  for (int j = 0; j < kTI; ++j) {
    fl[j] = 0;
    if (q0 + j < Tl) {
      while (q0 + j >= send && s + 1 < S) {
        ++s;
        send = sg.begin[s + 1];
        job = sg.job[s];
      }
      const unsigned r = e[j].y & kRowMask;
      fl[j] = r < (unsigned)n ? flags[(size_t)job * n + r] : 0;
      c += fl[j];
    }
  }
  unsigned tot;
  const unsigned ex = block_excl_scan(c, sh, tot);
  unsigned* slot = ptile + (size_t)f * NT + t;
  if constexpr (!APPLY) {
    if (threadIdx.x == 0) *slot = tot;
  } else {
    unsigned lrun = *slot + ex;  // rows before this item, in the whole list, that go left
    s = q0 < Tl ? seg_of(sg.begin, rng[0], rng[1], q0) : rng[1];
    int cs = -1, sbegin = 0, d = 0, p = 0;
    unsigned erow = 0, eleft = 0;
    send = sg.begin[s + 1];
#pragma unroll
    for (int j = 0; j < kTI; ++j) {
      const int q = q0 + j;
      if (q >= Tl) break;
      while (q >= send && s + 1 < S) {
        ++s;
        send = sg.begin[s + 1];
      }
      if (s != cs) {
        cs = s;
        sbegin = sg.begin[s];
        d = jovf[sg.job[s]] ? 0 : dec[s];
        p = bp[s];
        erow = E[(size_t)2 * Estride + s];
        eleft = E[(size_t)3 * Estride + s];
      }
      if (d & 1) {
        const unsigned lbefore = lrun - eleft;  // of this segment
        const int lL = (d >> 1) & 1;
        unsigned dst = 0xffffffffu;
        if (fl[j]) {
          if (lL) dst = erow + lbefore;
        } else if (d & 4) {
          dst = erow + (lL ? (unsigned)p : 0u) + ((unsigned)(q - sbegin) - lbefore);
        }
        if (dst < (unsigned)Tn) next[(size_t)f * Tp + dst] = e[j];
      }
      lrun += fl[j];
    }
  }
}

// ---- host --------------------------------------------------------------------
struct Layout {
  int64_t T = 0, Tp = 0;
  int NT = 0, NTn = 0, Smax = 0, ny = 1, fc = 1;
  size_t list[2], flags, tilecnt, ptile, ftile, segbest, tilefirst, seg[2][5], dec, bf, bp, cl, E, jobi, rootcnt,
      summary, fmask, wtot, wrows, total;
};

inline size_t carve(size_t& at, size_t bytes) {
  const size_t o = at;
  at += (bytes + 255) & ~(size_t)255;
  return o;
}

bool make_layout(int64_t n, int F, int J, const vad_tree_job* jobs, bool weighted, Layout& L) {
  int64_t T = 0, smax = 0;
  for (int j = 0; j < J; ++j) {
    T += jobs[j].n_rows;
    int64_t least = 2;
    if (2 * (int64_t)jobs[j].min_samples_leaf > least) least = 2 * (int64_t)jobs[j].min_samples_leaf;
    if (jobs[j].min_samples_split > least) least = jobs[j].min_samples_split;
    const int64_t m = jobs[j].n_rows / least;
    smax += m > 1 ? m : 1;
  }
  if (T >= (1ll << 31) - 2 * kTile || (int64_t)J * n >= (1ll << 40)) return false;
  L.T = T;
  L.Tp = (T + 31) & ~(int64_t)31;
  L.NT = (int)((T + kTile - 1) / kTile);
  L.NTn = (int)((n + kTile - 1) / kTile);
  L.Smax = (int)smax + 1;
  // feature chunks of the search: enough workgroups to fill the device
  int ny = (2048 + L.NT - 1) / L.NT;
  if (ny > F) ny = F;
  if (ny < 1) ny = 1;
  L.fc = (F + ny - 1) / ny;
  L.ny = (F + L.fc - 1) / L.fc;
  size_t at = 0;
  for (int i = 0; i < 2; ++i) L.list[i] = carve(at, (size_t)F * L.Tp * sizeof(uint2));
  L.flags = carve(at, (size_t)J * n);
  L.tilecnt = carve(at, (size_t)F * L.NT * kKP * 4);
  L.ptile = carve(at, (size_t)F * L.NT * 4);
  L.ftile = carve(at, (size_t)J * F * L.NTn * 4);
  L.segbest = carve(at, (size_t)L.ny * L.Smax * sizeof(Rec));
  L.tilefirst = carve(at, (size_t)L.ny * L.NT * sizeof(Rec));
  for (int i = 0; i < 2; ++i) {
    L.seg[i][0] = carve(at, (size_t)(L.Smax + 1) * 4);
    L.seg[i][1] = carve(at, (size_t)L.Smax * 4);
    L.seg[i][2] = carve(at, (size_t)L.Smax * 4);
    L.seg[i][3] = carve(at, (size_t)L.Smax * kKP * 4);
    L.seg[i][4] = carve(at, (size_t)L.Smax * kKP * 4);
  }
  L.dec = carve(at, (size_t)L.Smax * 4);
  L.bf = carve(at, (size_t)L.Smax * 4);
  L.bp = carve(at, (size_t)L.Smax * 4);
  L.cl = carve(at, (size_t)L.Smax * kKP * 4);
  L.E = carve(at, (size_t)kScanV * (L.Smax + 1) * 4);
  L.jobi = carve(at, (size_t)15 * J * 4);
  L.rootcnt = carve(at, (size_t)J * kKP * 4);
  L.summary = carve(at, 256);
  L.fmask = carve(at, (size_t)J * 8);
  L.wtot = L.wrows = at;
  if (weighted) {  // the roots' total weights and distinct rows
    L.wtot = carve(at, (size_t)J * 8);
    L.wrows = carve(at, (size_t)J * 4);
  }
  L.total = at;
  return true;
}

}  // namespace

size_t tree_train_ws_bytes(int64_t n, int F, int n_jobs, const vad_tree_job* jobs, bool weighted) {
  Layout L;
  return make_layout(n, F, n_jobs, jobs, weighted, L) ? L.total : 0;
}

#define TT_CHECK(e)                         \
  do {                                      \
    const hipError_t e_ = (e);              \
    if (e_ != hipSuccess) return (int)e_;   \
  } while (0)

int tree_train_run(const float* x, const uint8_t* y, int64_t n64, int F, int K, const int32_t* order,
                   const uint8_t* mask, const uint64_t* feature_masks, int J, const vad_tree_job* jobs,
                   const vad_tree_tables& out, void* ws, size_t ws_bytes, int32_t* n_levels, hipStream_t st,
                   bool weighted) {
  // weighted: mask holds the jobs' weights (not NULL)
  Layout L;
  if (!make_layout(n64, F, J, jobs, weighted, L) || ws_bytes < L.total || (weighted && !mask)) return VAD_EINVAL;
  const int n = (int)n64, T = (int)L.T, Tp = (int)L.Tp;
  char* w = (char*)ws;

  // descriptors: n, off, md, mss, msl, cap, nodeoff, then the state arrays
  std::vector<int> h((size_t)7 * J);
  int64_t off = 0, nodeoff = 0;
  int max_depth = 0;
  for (int j = 0; j < J; ++j) {
    h[0 * J + j] = (int)jobs[j].n_rows;
    h[1 * J + j] = (int)off;
    h[2 * J + j] = jobs[j].max_depth;
    h[3 * J + j] = jobs[j].min_samples_split;
    h[4 * J + j] = jobs[j].min_samples_leaf;
    h[5 * J + j] = (int)jobs[j].node_capacity;
    h[6 * J + j] = (int)nodeoff;
    off += jobs[j].n_rows;
    nodeoff += jobs[j].node_capacity;
    if (jobs[j].max_depth > max_depth) max_depth = jobs[j].max_depth;
  }
  int* ji = (int*)(w + L.jobi);
  TT_CHECK(hipMemcpyAsync(ji, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice, st));
  TT_CHECK(hipMemsetAsync(w + L.rootcnt, 0, (size_t)J * kKP * 4, st));
  const u64* jfmask = nullptr;
  if (feature_masks) {
    TT_CHECK(hipMemcpyAsync(w + L.fmask, feature_masks, (size_t)J * 8, hipMemcpyHostToDevice, st));
    jfmask = (const u64*)(w + L.fmask);
  }
  Jobs jb;
  jb.n = ji;
  jb.off = ji + J;
  jb.md = ji + 2 * J;
  jb.mss = ji + 3 * J;
  jb.msl = ji + 4 * J;
  jb.cap = ji + 5 * J;
  jb.nodeoff = ji + 6 * J;
  jb.first = ji + 7 * J;
  jb.end = ji + 9 * J;
  jb.nn = ji + 11 * J;
  jb.splits = ji + 13 * J;
  jb.ovf = ji + 14 * J;
  jb.rootcnt = (unsigned*)(w + L.rootcnt);
  Tables o;
  o.feature = out.feature;
  o.threshold = out.threshold;
  o.left = out.left;
  o.right = out.right;
  o.leaf = out.leaf;
  o.nan_left = out.nan_left;
  o.n_node_samples = out.n_node_samples;
  o.depth = out.depth;
  o.value = out.value;
  o.n_nodes = out.n_nodes;
  o.status = out.status;
  o.K = K;
  Segs sg[2];
  for (int i = 0; i < 2; ++i) {
    sg[i].begin = (int*)(w + L.seg[i][0]);
    sg[i].job = (int*)(w + L.seg[i][1]);
    sg[i].node = (int*)(w + L.seg[i][2]);
    sg[i].cnt = (unsigned*)(w + L.seg[i][3]);
    sg[i].base = (unsigned*)(w + L.seg[i][4]);
  }
  uint2* list[2] = {(uint2*)(w + L.list[0]), (uint2*)(w + L.list[1])};
  uint8_t* flags = (uint8_t*)(w + L.flags);
  unsigned* tilecnt = (unsigned*)(w + L.tilecnt);
  unsigned* ptile = (unsigned*)(w + L.ptile);
  unsigned* ftile = (unsigned*)(w + L.ftile);
  Rec* segbest = (Rec*)(w + L.segbest);
  Rec* tilefirst = (Rec*)(w + L.tilefirst);
  int* dec = (int*)(w + L.dec);
  int* bf = (int*)(w + L.bf);
  int* bp = (int*)(w + L.bp);
  unsigned* cl = (unsigned*)(w + L.cl);
  unsigned* E = (unsigned*)(w + L.E);
  int* summary = (int*)(w + L.summary);
  const int Estride = L.Smax + 1;

  // the lists and the roots
  const dim3 fgrid(L.NTn, F, J);
  hipLaunchKernelGGL(tt_filter<false>, fgrid, dim3(kTT), 0, st, order, mask, x, y, n, F, L.NTn, ftile, jb.off, jb.n,
                     list[0], Tp);
  hipLaunchKernelGGL(tt_carry<1>, dim3(J * F), dim3(kTT), 0, st, ftile, L.NTn, L.NTn);
  hipLaunchKernelGGL(tt_filter<true>, fgrid, dim3(kTT), 0, st, order, mask, x, y, n, F, L.NTn, ftile, jb.off, jb.n,
                     list[0], Tp);
  if (weighted) {
    u64* wtot = (u64*)(w + L.wtot);
    unsigned* wrows = (unsigned*)(w + L.wrows);
    TT_CHECK(hipMemsetAsync(wtot, 0, L.total - L.wtot, st));
    hipLaunchKernelGGL(tt_root_counts_w, dim3(L.NTn < 1024 ? L.NTn : 1024, J), dim3(kTT), 0, st, mask, y, n,
                       jb.rootcnt, wtot, wrows);
    hipLaunchKernelGGL(tt_init<true>, dim3((J + kTT - 1) / kTT), dim3(kTT), 0, st, jb, J, T, sg[0], o, wtot, wrows);
  } else {
    hipLaunchKernelGGL(tt_root_counts, dim3(L.NTn < 1024 ? L.NTn : 1024, J), dim3(kTT), 0, st, mask, y, n, jb.rootcnt);
    hipLaunchKernelGGL(tt_init<false>, dim3((J + kTT - 1) / kTT), dim3(kTT), 0, st, jb, J, T, sg[0], o,
                       (const u64*)nullptr, (const unsigned*)nullptr);
  }
  TT_CHECK(hipGetLastError());

  int S = J, Tl = T, par = 0, cur = 0, level = 0;
  for (; S > 0 && level <= max_depth; ++level) {
    const int NTl = (Tl + kTile - 1) / kTile;
    const dim3 sgrid(NTl, L.ny);
#define TT_SEARCH(NW, MASKED, WW)                                                                                  \
  hipLaunchKernelGGL((tt_search<NW, MASKED, WW>), sgrid, dim3(kTT), 0, st, list[cur], Tp, Tl, F, L.fc, tilecnt, L.NT, \
                     sg[par], S, jb.msl, jfmask, segbest, L.Smax, tilefirst, mask, n)
#define TT_CLASS_W(WW)                                                                                        \
  hipLaunchKernelGGL(tt_class_tiles_w<WW>, dim3(NTl, F), dim3(kTT), 0, st, list[cur], Tp, Tl, tilecnt, L.NT, mask, n, \
                     sg[par].begin, sg[par].job, S)
    if (!weighted) hipLaunchKernelGGL(tt_class_tiles, dim3(NTl, F), dim3(kTT), 0, st, list[cur], Tp, Tl, tilecnt, L.NT);
    else if (K <= 2) TT_CLASS_W(1);
    else if (K <= 4) TT_CLASS_W(2);
    else TT_CLASS_W(4);
    hipLaunchKernelGGL(tt_carry<kKP>, dim3(F), dim3(kTT), 0, st, tilecnt, NTl, L.NT);
    if (!weighted) {
      if (K <= 4 && !jfmask) TT_SEARCH(1, false, 0);
      else if (!jfmask) TT_SEARCH(2, false, 0);
      else if (K <= 4) TT_SEARCH(1, true, 0);
      else TT_SEARCH(2, true, 0);
      hipLaunchKernelGGL(tt_decide<false>, dim3((S + 3) / 4), dim3(kTT), 0, st, list[cur], Tp, sg[par], S, level, jb,
                         tilecnt, L.NT, segbest, L.Smax, tilefirst, L.ny, dec, bf, bp, cl, o, mask, n);
    } else {
      if (K <= 2 && !jfmask) TT_SEARCH(1, false, 1);
      else if (K <= 4 && !jfmask) TT_SEARCH(1, false, 2);
      else if (!jfmask) TT_SEARCH(1, false, 4);
      else if (K <= 2) TT_SEARCH(1, true, 1);
      else if (K <= 4) TT_SEARCH(1, true, 2);
      else TT_SEARCH(1, true, 4);
      hipLaunchKernelGGL(tt_decide<true>, dim3((S + 3) / 4), dim3(kTT), 0, st, list[cur], Tp, sg[par], S, level, jb,
                         tilecnt, L.NT, segbest, L.Smax, tilefirst, L.ny, dec, bf, bp, cl, o, mask, n);
    }
#undef TT_SEARCH
#undef TT_CLASS_W
    hipLaunchKernelGGL(tt_scan, dim3(1), dim3(kTT), 0, st, sg[par], S, jb, J, par, dec, bp, cl, E, Estride, summary,
                       o.status);
    hipLaunchKernelGGL(tt_emit, dim3((S + J + kTT - 1) / kTT), dim3(kTT), 0, st, sg[par], S, level, jb, J, par, dec,
                       bp, cl, E, Estride, sg[par ^ 1], L.Smax, o);
    TT_CHECK(hipGetLastError());
    int next[2] = {0, 0};
    TT_CHECK(hipMemcpyAsync(next, summary, sizeof(next), hipMemcpyDeviceToHost, st));
    TT_CHECK(hipStreamSynchronize(st));
    if (next[0] < 0 || next[0] > L.Smax || next[1] < 0 || next[1] > Tl) return VAD_EINVAL;  // (corrupt inputs)
    if (next[0] > 0) {
      hipLaunchKernelGGL(tt_mark, dim3(NTl), dim3(kTT), 0, st, list[cur], Tp, Tl, sg[par], S, jb.ovf, dec, bf, bp, n,
                         flags);
      hipLaunchKernelGGL(tt_partition<false>, dim3(NTl, F), dim3(kTT), 0, st, list[cur], list[cur ^ 1], Tp, Tl,
                         next[1], sg[par], S, jb.ovf, dec, bp, E, Estride, n, flags, ptile, L.NT);
      hipLaunchKernelGGL(tt_carry<1>, dim3(F), dim3(kTT), 0, st, ptile, NTl, L.NT);
      hipLaunchKernelGGL(tt_partition<true>, dim3(NTl, F), dim3(kTT), 0, st, list[cur], list[cur ^ 1], Tp, Tl, next[1],
                         sg[par], S, jb.ovf, dec, bp, E, Estride, n, flags, ptile, L.NT);
      TT_CHECK(hipGetLastError());
      cur ^= 1;
    }
    S = next[0];
    Tl = next[1];
    par ^= 1;
  }
  if (n_levels) *n_levels = level;
  std::vector<int32_t> status((size_t)J);
  TT_CHECK(hipMemcpyAsync(status.data(), out.status, (size_t)J * 4, hipMemcpyDeviceToHost, st));
  TT_CHECK(hipStreamSynchronize(st));
  int rc = VAD_OK;
  for (int j = 0; j < J; ++j) {
    if (status[j] & (VAD_TREE_TRAIN_BAD_ROWS | VAD_TREE_TRAIN_BAD_WEIGHT)) return VAD_EINVAL;
    if (status[j] & VAD_TREE_TRAIN_OVERFLOW) rc = VAD_ENOMEM;
  }
  return rc;
}

}  // namespace vad
