// Random forest: T decision trees walked per feature row, their leaf class
// shares averaged (sklearn's RandomForestClassifier / ExtraTreesClassifier /
// BaggingClassifier.predict_proba with n_jobs = 1).
//
// Per row: K <= 8 double accumulators start at 0; for t = 0 .. T-1 in order
// acc[k] += proba[leaf_t][k]; then acc[k] /= T.  The score is
// (float)acc[active], the label the first maximum of acc.  Every operation is
// one IEEE double add or divide in a fixed order, so the result is sklearn's
// bit for bit.  The walk rule is tree_walk.h's.
//
// The plan (capi.hip) keeps tree t in the nodes [roots[t], roots[t + 1]) with
// its root first and the child indices RELATIVE to the root, so the walks of
// tree_walk.h run on `nodes + roots[t]` unchanged and a leaf's row of the
// proba table is roots[t] + the node they return.
//
// Window kernel (vad_features_forest): the structure of tree_window_kernel --
// 256 windows per block iteration, their MFCC rows staged in LDS, the
// 3 * mfcc_n features of each window computed ONCE into an LDS row -- and then
// a loop over the trees.  Consecutive trees are staged into one LDS buffer as
// long as they fit (the buffer holds twice the largest tree that fits LDS at
// all, so trees of about equal size go in pairs; it shares its bytes with the
// MFCC rows, which are dead once the features exist), and every thread walks
// the staged trees for its window TWO AT A TIME: a walk is a chain of
// dependent LDS reads (node, then feature), and two trees give a thread two
// independent chains.  The shares are added in tree order whatever the
// pairing.  A tree of more than kLdsNodes nodes is walked from global memory,
// that tree only.  Nothing but labels and scores is written.  No workgroup
// waits on another and there are no atomics.
#include "vad_common.h"
#include "features.h"
#include "tree_walk.h"

#ifndef VAD_FOREST_DUAL
#define VAD_FOREST_DUAL 1  // 0: one tree at a time (the A/B of profiles/forest)
#endif

namespace vad {
namespace {

constexpr int kTreeWin = 256;
constexpr int kTreeXStride = 3 * kMaxCoefs + 1;  // tree_kernel.hip's
constexpr int kLdsNodes = 3072;                  // tree_kernel.hip's: the largest tree staged in LDS
constexpr int kKMax = VAD_FOREST_MAX_CLASSES;

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

// acc[k] += proba[leaf][k]; KT > 0: K known at compile time
template <int KT>
__device__ __forceinline__ void add_shares(double (&acc)[kKMax], const double* __restrict__ proba, int K, int leaf) {
  const double* p = proba + (size_t)leaf * (KT > 0 ? KT : K);
#pragma unroll
  for (int k = 0; k < kKMax; ++k)
    if (k < (KT > 0 ? KT : K)) acc[k] += p[k];
}

// acc /= T, then the score and the first maximum
template <int KT>
__device__ __forceinline__ void finish(double (&acc)[kKMax], int K, int T, int active, int64_t i,
                                       uint8_t* __restrict__ labels, float* __restrict__ scores) {
  const double div = (double)T;
  double best = 0.0, act = 0.0;
  int arg = 0;
#pragma unroll
  for (int k = 0; k < kKMax; ++k)
    if (k < (KT > 0 ? KT : K)) {
      const double v = acc[k] / div;
      if (k == 0 || v > best) { best = v; arg = k; }
      if (k == active) act = v;
    }
  labels[i] = (uint8_t)arg;
  if (scores) scores[i] = (float)act;
}

// Two walks of tree_walk_c_node side by side: trees a and b, the same row.
__device__ __forceinline__ void walk_pair(const TreeNodeC* na, int n_a, const TreeNodeC* nb, int n_b, const float* x,
                                          int* leaf_a, int* leaf_b) {
  int a = 0, b = 0;
  bool da = false, db = false;
  const int bound = n_a > n_b ? n_a : n_b;
  for (int it = 0; it < bound && !(da && db); ++it) {
    const TreeNodeC ca = na[a], cb = nb[b];
    da = ca.feature < 0;
    db = cb.feature < 0;
    const float xa = x[da ? 0 : ca.feature & 0xffff], xb = x[db ? 0 : cb.feature & 0xffff];
    const bool la = xa != xa ? (ca.feature >> 30) != 0 : xa <= ca.thr;
    const bool lb = xb != xb ? (cb.feature >> 30) != 0 : xb <= cb.thr;
    a = da ? a : la ? ca.left : ca.right;
    b = db ? b : lb ? cb.left : cb.right;
  }
  // a malformed table: the root, as tree_walk_c_node
  *leaf_a = da ? a : 0;
  *leaf_b = db ? b : 0;
}

// Feature rows x[i*dim + f] (vad_forest_predict): one thread per row, global walks.
template <int KT>
__global__ __launch_bounds__(256) void forest_rows_kernel(ForestDev f, const float* __restrict__ x, int64_t n, int dim,
                                                          int active, uint8_t* __restrict__ labels,
                                                          float* __restrict__ scores) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double acc[kKMax];
#pragma unroll
    for (int k = 0; k < kKMax; ++k) acc[k] = 0.0;
    for (int t = 0; t < f.T; ++t) {
      const int r = f.roots[t];
      add_shares<KT>(acc, f.proba, f.K, r + tree_walk_node(f.nodes + r, f.roots[t + 1] - r, x + i * dim, 1));
    }
    finish<KT>(acc, f.K, f.T, active, i, labels, scores);
  }
}

// Windows of an MFCC sequence (vad_features_forest), 256 per block iteration.
// Dynamic LDS: X (256 feature rows), then the buffer of buf_nodes compact
// nodes that first holds the chunk's MFCC rows.
template <int MN, int KT>
__global__ __launch_bounds__(256) void forest_window_kernel(ForestDev f, const float* __restrict__ mfcc, int64_t n_rows,
                                                            int mfcc_n_rt, int mode, int active, int buf_nodes,
                                                            uint8_t* __restrict__ labels, float* __restrict__ scores) {
  constexpr int XS = MN > 0 ? 3 * MN : kTreeXStride;
  constexpr int RS = MN > 0 ? MN : kMaxCoefs;
  extern __shared__ __attribute__((aligned(16))) char dyn[];
  float* X = reinterpret_cast<float*>(dyn);
  float* rows = X + kTreeWin * XS;  // (kTreeWin * XS * 4) % 16 == 0
  TreeNodeC* cn_s = reinterpret_cast<TreeNodeC*>(rows);
  const int mfcc_n = MN > 0 ? MN : mfcc_n_rt;
  const int tid = threadIdx.x;
  const int T = f.T;
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
    __syncthreads();  // the features are complete; the rows are dead from here

    const float* xw = X + tid * XS;
    double acc[kKMax];
#pragma unroll
    for (int k = 0; k < kKMax; ++k) acc[k] = 0.0;
    int t = 0;
    while (t < T) {  // uniform: every thread sees the same groups
      const int g0 = f.roots[t];
      int te = t + 1;
      if (f.roots[te] - g0 > buf_nodes || f.roots[te] - g0 > kLdsNodes) {
        // too large for LDS: this tree from global memory
        if (tid < nwin) add_shares<KT>(acc, f.proba, f.K, g0 + tree_walk_node(f.nodes + g0, f.roots[te] - g0, xw, 1));
        t = te;
        continue;
      }
      while (te < T && f.roots[te + 1] - f.roots[te] <= kLdsNodes && f.roots[te + 1] - g0 <= buf_nodes) ++te;
      const int gn = f.roots[te] - g0;
      const uint4* src = reinterpret_cast<const uint4*>(f.cnodes + g0);
      for (int i = tid; i < gn; i += 256) reinterpret_cast<uint4*>(cn_s)[i] = src[i];
      __syncthreads();
      if (tid < nwin) {
        int u = t;
#if VAD_FOREST_DUAL
        for (; u + 1 < te; u += 2) {
          const int ra = f.roots[u], rb = f.roots[u + 1], rc = f.roots[u + 2];
          int la, lb;
          walk_pair(cn_s + (ra - g0), rb - ra, cn_s + (rb - g0), rc - rb, xw, &la, &lb);
          add_shares<KT>(acc, f.proba, f.K, ra + la);
          add_shares<KT>(acc, f.proba, f.K, rb + lb);
        }
#endif
        for (; u < te; ++u) {
          const int r = f.roots[u];
          add_shares<KT>(acc, f.proba, f.K, r + tree_walk_c_node(cn_s + (r - g0), f.roots[u + 1] - r, xw));
        }
      }
      __syncthreads();  // before the next group, or the next chunk's rows, overwrite the buffer
      t = te;
    }
    if (tid < nwin) finish<KT>(acc, f.K, T, active, base + tid, labels, scores);
  }
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

hipError_t launch_forest_rows(const ForestDev& f, const float* x, int64_t n, int dim, int active, uint8_t* labels,
                              float* scores, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  int64_t blocks = (n + 255) / 256;
  const int64_t cap = 8 * num_cus();
  if (blocks > cap) blocks = cap;
  const dim3 grid((unsigned)blocks), block(256);
  if (f.K == 2) forest_rows_kernel<2><<<grid, block, 0, st>>>(f, x, n, dim, active, labels, scores);
  else forest_rows_kernel<0><<<grid, block, 0, st>>>(f, x, n, dim, active, labels, scores);
  return hipGetLastError();
}

// max_lds_tree: the node count of the largest tree of at most kLdsNodes nodes (0: none)
hipError_t launch_forest_windows(const ForestDev& f, int max_lds_tree, const float* mfcc, int64_t n_rows, int mfcc_n,
                                 int mode, int active, uint8_t* labels, float* scores, hipStream_t st) {
  if (n_rows <= 0) return hipSuccess;
  int64_t blocks = (n_rows + kTreeWin - 1) / kTreeWin;
  const int64_t cap = 4 * num_cus();
  if (blocks > cap) blocks = cap;
  const bool m13 = mfcc_n == 13;
  const size_t x_bytes = (size_t)kTreeWin * (m13 ? 39 : kTreeXStride) * sizeof(float);
  const size_t row_bytes = align16((size_t)(kTreeWin + 4) * (m13 ? 13 : kMaxCoefs) * sizeof(float));
  size_t buf = (size_t)(VAD_FOREST_DUAL ? 2 : 1) * (size_t)max_lds_tree * sizeof(TreeNodeC);
  if (buf < row_bytes) buf = row_bytes;
  const int buf_nodes = (int)(buf / sizeof(TreeNodeC));
  const size_t smem = x_bytes + buf;  // <= 50176 + 98304: inside the 160 KB of a CU
  const dim3 grid((unsigned)blocks), block(256);
#define VAD_FOREST_LAUNCH(MN, KT)                                                                                   \
  do {                                                                                                              \
    static std::atomic<unsigned long long> done{0}; /* more than 64 KB of dynamic LDS needs the attribute */        \
    const hipError_t e =                                                                                            \
        ensure_dyn_lds(reinterpret_cast<const void*>(&forest_window_kernel<MN, KT>), 160 * 1024, done);             \
    if (e != hipSuccess) return e;                                                                                  \
    forest_window_kernel<MN, KT><<<grid, block, smem, st>>>(f, mfcc, n_rows, mfcc_n, mode, active, buf_nodes,       \
                                                            labels, scores);                                        \
  } while (0)
  if (m13 && f.K == 2) VAD_FOREST_LAUNCH(13, 2);
  else if (m13) VAD_FOREST_LAUNCH(13, 0);
  else if (f.K == 2) VAD_FOREST_LAUNCH(0, 2);
  else VAD_FOREST_LAUNCH(0, 0);
#undef VAD_FOREST_LAUNCH
  return hipGetLastError();
}

}  // namespace vad
