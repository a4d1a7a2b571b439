// Streaming hops labelled by the decision tree (the classifier vad.py
// deploys, vad.py:17,52): the tree counterparts of stream_kernel.hip's hop
// kernel and of ffn_kernel.hip's ring step.
//
// stream_hop_tree_kernel is stream_hop_kernel with the FFN replaced by a
// wave-uniform walk of the tree.  Its front end -- frame shift, 256-point
// Stockham FFT, real split, mel + log10, lifter x DCT, the ring, the window
// features -- is a copy of that kernel's code, statement for statement; the
// LDS layout, the small helpers and the launch rule are shared
// (stream_hop.h).  One body instantiated by both kernels was built and
// measured: it kept every register count but not the schedule, and the
// global walk came out slower (profiles/stream_hop_shared/isa.md), so the
// copies stay, and
// tests/test_gpu_stream_tree.py::test_front_end_locked_to_ffn_kernel holds
// them together bit for bit (frames, ring and count of a tree batch and an
// FFN batch on the same hops).  Change both or neither.
//
// The walk: a wave has one window per hop, so every lane would take the same
// path; the node index is kept uniform (readfirstlane) and each level is one
// 16-B LDS read of the node (all lanes the same address: a broadcast), one
// LDS read of the feature and the compare of tree_walk_c.  The compact node
// table (TreeNodeC, 16 B = one global_load_lds_dwordx4 lane) is staged by the
// same LDS-DMA as the plan's blob, behind it.  A table that does not fit
// beside one wave's scratch is walked from global memory (TreeNode, double
// threshold, tree_walk's rule) -- see launch_stream_hop_tree for the rule.
#include "vad_common.h"
#include "features.h"
#include "stream_hop.h"
#include "stream_denoise.h"
#include "tree_walk.h"

namespace vad {

// NR, TH: as stream_hop_kernel.  lds_nodes: n_nodes when the compact table is
// staged behind the blob and walked from LDS, 0 for the walk from global.
// The body is stream_hop_tree_body.inc, included by the label-only kernel and
// by the scored one.
template <int NR, class TH>
__global__ __launch_bounds__(1024) void stream_hop_tree_kernel(
    const float* __restrict__ blob, int blob_n, int nf, int n_taps, const TreeNodeC* __restrict__ cnodes,
    const TreeNode* __restrict__ nodes, int n_nodes, int lds_nodes, float* __restrict__ frames, int64_t fstride,
    int len, const TH* __restrict__ hop, int64_t hstride, int hlen, int64_t n_streams, int mfcc_n,
    float* __restrict__ ring, int* __restrict__ count, uint8_t* __restrict__ labels, int n_hops,
    int64_t hop_kstride, int64_t lab_kstride) {
#define VAD_HOP_SCORE 0
#define VAD_HOP_DENOISE 0
#define VAD_HOP_SESSIONS 0
#include "stream_hop_tree_body.inc"
#undef VAD_HOP_SESSIONS
#undef VAD_HOP_DENOISE
#undef VAD_HOP_SCORE
}

template <int NR, class TH>
__global__ __launch_bounds__(1024) void stream_hop_tree_scores_kernel(
    const float* __restrict__ blob, int blob_n, int nf, int n_taps, const TreeNodeC* __restrict__ cnodes,
    const TreeNode* __restrict__ nodes, int n_nodes, int lds_nodes, float* __restrict__ frames, int64_t fstride,
    int len, const TH* __restrict__ hop, int64_t hstride, int hlen, int64_t n_streams, int mfcc_n,
    float* __restrict__ ring, int* __restrict__ count, uint8_t* __restrict__ labels, int n_hops,
    int64_t hop_kstride, int64_t lab_kstride, const float* __restrict__ node_score, float* __restrict__ scores,
    int64_t score_kstride) {
#define VAD_HOP_SCORE 1
#define VAD_HOP_DENOISE 0
#define VAD_HOP_SESSIONS 0
#include "stream_hop_tree_body.inc"
#undef VAD_HOP_SESSIONS
#undef VAD_HOP_DENOISE
#undef VAD_HOP_SCORE
}

// The denoising form (stream_denoise.h): the scored kernel's arguments plus
// the denoise state; `scores`, and with it node_score, may be null.
template <int NR, class TH>
__global__ __launch_bounds__(1024) void stream_hop_tree_denoise_kernel(
    const float* __restrict__ blob, int blob_n, int nf, int n_taps, const TreeNodeC* __restrict__ cnodes,
    const TreeNode* __restrict__ nodes, int n_nodes, int lds_nodes, float* __restrict__ frames, int64_t fstride,
    int len, const TH* __restrict__ hop, int64_t hstride, int hlen, int64_t n_streams, int mfcc_n,
    float* __restrict__ ring, int* __restrict__ count, uint8_t* __restrict__ labels, int n_hops,
    int64_t hop_kstride, int64_t lab_kstride, const float* __restrict__ node_score, float* __restrict__ scores,
    int64_t score_kstride, HopDenoise dn) {
#define VAD_HOP_SCORE 1
#define VAD_HOP_DENOISE 1
#define VAD_HOP_SESSIONS 0
#include "stream_hop_tree_body.inc"
#undef VAD_HOP_SESSIONS
#undef VAD_HOP_DENOISE
#undef VAD_HOP_SCORE
}

// The sessions forms (stream_kernel.hip's stream_hop_sessions_kernel): the
// scored kernel with nullable `scores`, without and with the denoise state,
// plus the per-stream hop counts and restart flags.
template <int NR, class TH>
__global__ __launch_bounds__(1024) void stream_hop_tree_sessions_kernel(
    const float* __restrict__ blob, int blob_n, int nf, int n_taps, const TreeNodeC* __restrict__ cnodes,
    const TreeNode* __restrict__ nodes, int n_nodes, int lds_nodes, float* __restrict__ frames, int64_t fstride,
    int len, const TH* __restrict__ hop, int64_t hstride, int hlen, int64_t n_streams, int mfcc_n,
    float* __restrict__ ring, int* __restrict__ count, uint8_t* __restrict__ labels, int n_hops,
    int64_t hop_kstride, int64_t lab_kstride, const float* __restrict__ node_score, float* __restrict__ scores,
    int64_t score_kstride, const int* __restrict__ hop_counts, uint8_t* __restrict__ restart) {
#define VAD_HOP_SCORE 1
#define VAD_HOP_DENOISE 0
#define VAD_HOP_SESSIONS 1
#include "stream_hop_tree_body.inc"
#undef VAD_HOP_SESSIONS
#undef VAD_HOP_DENOISE
#undef VAD_HOP_SCORE
}

template <int NR, class TH>
__global__ __launch_bounds__(1024) void stream_hop_tree_sessions_denoise_kernel(
    const float* __restrict__ blob, int blob_n, int nf, int n_taps, const TreeNodeC* __restrict__ cnodes,
    const TreeNode* __restrict__ nodes, int n_nodes, int lds_nodes, float* __restrict__ frames, int64_t fstride,
    int len, const TH* __restrict__ hop, int64_t hstride, int hlen, int64_t n_streams, int mfcc_n,
    float* __restrict__ ring, int* __restrict__ count, uint8_t* __restrict__ labels, int n_hops,
    int64_t hop_kstride, int64_t lab_kstride, const float* __restrict__ node_score, float* __restrict__ scores,
    int64_t score_kstride, HopDenoise dn, const int* __restrict__ hop_counts, uint8_t* __restrict__ restart) {
#define VAD_HOP_SCORE 1
#define VAD_HOP_DENOISE 1
#define VAD_HOP_SESSIONS 1
#include "stream_hop_tree_body.inc"
#undef VAD_HOP_SESSIONS
#undef VAD_HOP_DENOISE
#undef VAD_HOP_SCORE
}

// LDS of a launch: the blob, the staged nodes, one scratch per wave.  The
// largest table walked from LDS is the one that fits beside ONE wave's
// scratch; a larger one is walked from global memory.
int64_t stream_tree_max_lds_nodes(int blob_n) {
  const int64_t room = (int64_t)kHopLdsBytes - (int64_t)blob_n * sizeof(float) - (int64_t)kHopWaveFloats * sizeof(float);
  return room > 0 ? room / (int64_t)sizeof(TreeNodeC) : 0;
}

// The nodes a launch stages: the whole table, or none (the global walk).
int stream_tree_lds_nodes(int blob_n, const TreeNodeC* cnodes, int n_nodes, bool force_global) {
  return !force_global && cnodes && n_nodes <= stream_tree_max_lds_nodes(blob_n) ? n_nodes : 0;
}

size_t stream_hop_tree_table_bytes(int blob_n, int lds_nodes) {
  return (size_t)blob_n * sizeof(float) + (size_t)lds_nodes * sizeof(TreeNodeC);
}

template <class TH>
static hipError_t launch_stream_hop_tree_t(const float* blob, int blob_n, int nf, int n_taps, const TreeNodeC* cnodes,
                                           const TreeNode* nodes, int n_nodes, int lds_nodes, float* frames,
                                           int64_t fstride, int len, const void* hop, int64_t hstride, int hlen,
                                           int64_t n_streams, int mfcc_n, float* ring, int* count, uint8_t* labels,
                                           int n_hops, int64_t hop_kstride, int64_t lab_kstride, hipStream_t st) {
  return launch_hop_kernels<&stream_hop_tree_kernel<7, TH>, &stream_hop_tree_kernel<16, TH>>(
      stream_hop_tree_table_bytes(blob_n, lds_nodes), len, n_streams, n_hops, st, blob, blob_n,
      nf, n_taps, cnodes, nodes, n_nodes, lds_nodes, frames, fstride, len, (const TH*)hop, hstride, hlen, n_streams,
      mfcc_n, ring, count, labels, n_hops, hop_kstride, lab_kstride);
}

template <class TH>
static hipError_t launch_stream_hop_tree_scores_t(const float* blob, int blob_n, int nf, int n_taps,
                                                  const TreeNodeC* cnodes, const TreeNode* nodes, int n_nodes,
                                                  int lds_nodes, float* frames, int64_t fstride, int len,
                                                  const void* hop, int64_t hstride, int hlen, int64_t n_streams,
                                                  int mfcc_n, float* ring, int* count, uint8_t* labels, int n_hops,
                                                  int64_t hop_kstride, int64_t lab_kstride, const float* node_score,
                                                  float* scores, int64_t score_kstride, hipStream_t st) {
  return launch_hop_kernels<&stream_hop_tree_scores_kernel<7, TH>, &stream_hop_tree_scores_kernel<16, TH>>(
      stream_hop_tree_table_bytes(blob_n, lds_nodes), len, n_streams, n_hops, st, blob, blob_n,
      nf, n_taps, cnodes, nodes, n_nodes, lds_nodes, frames, fstride, len, (const TH*)hop, hstride, hlen, n_streams,
      mfcc_n, ring, count, labels, n_hops, hop_kstride, lab_kstride, node_score, scores, score_kstride);
}

// hop: fp32 samples (hop_bytes 4) or int16 PCM (2); strides in elements.  The
// table leaves LDS only when it does not fit at one wave per block.
hipError_t launch_stream_hop_tree(const float* blob, int blob_n, int nf, int n_taps, const TreeNodeC* cnodes,
                                  const TreeNode* nodes, int n_nodes, bool force_global, float* frames,
                                  int64_t fstride, int len, const void* hop, int hop_bytes, int64_t hstride, int hlen,
                                  int64_t n_streams, int mfcc_n, float* ring, int* count, uint8_t* labels, int n_hops,
                                  int64_t hop_kstride, int64_t lab_kstride, hipStream_t st) {
  const int lds_nodes = stream_tree_lds_nodes(blob_n, cnodes, n_nodes, force_global);
  const auto launch = hop_bytes == 2 ? launch_stream_hop_tree_t<int16_t> : launch_stream_hop_tree_t<float>;
  return launch(blob, blob_n, nf, n_taps, cnodes, nodes, n_nodes, lds_nodes, frames, fstride, len, hop,
                hstride, hlen, n_streams, mfcc_n, ring, count, labels, n_hops, hop_kstride, lab_kstride, st);
}

// the scored form (the same walk rule): node_score is one class's row of the
// plan's score table, n_nodes floats
hipError_t launch_stream_hop_tree_scores(const float* blob, int blob_n, int nf, int n_taps, const TreeNodeC* cnodes,
                                         const TreeNode* nodes, int n_nodes, bool force_global, float* frames,
                                         int64_t fstride, int len, const void* hop, int hop_bytes, int64_t hstride,
                                         int hlen, int64_t n_streams, int mfcc_n, float* ring, int* count,
                                         uint8_t* labels, int n_hops, int64_t hop_kstride, int64_t lab_kstride,
                                         const float* node_score, float* scores, int64_t score_kstride,
                                         hipStream_t st) {
  const int lds_nodes = stream_tree_lds_nodes(blob_n, cnodes, n_nodes, force_global);
  const auto launch = hop_bytes == 2 ? launch_stream_hop_tree_scores_t<int16_t> : launch_stream_hop_tree_scores_t<float>;
  return launch(blob, blob_n, nf, n_taps, cnodes, nodes, n_nodes, lds_nodes, frames, fstride, len, hop,
                hstride, hlen, n_streams, mfcc_n, ring, count, labels, n_hops, hop_kstride, lab_kstride, node_score,
                scores, score_kstride, st);
}

template <class TH>
static hipError_t launch_stream_hop_tree_denoise_t(const float* blob, int blob_n, int nf, int n_taps,
                                                   const TreeNodeC* cnodes, const TreeNode* nodes, int n_nodes,
                                                   int lds_nodes, float* frames, int64_t fstride, int len,
                                                   const void* hop, int64_t hstride, int hlen, int64_t n_streams,
                                                   int mfcc_n, float* ring, int* count, uint8_t* labels, int n_hops,
                                                   int64_t hop_kstride, int64_t lab_kstride, const float* node_score,
                                                   float* scores, int64_t score_kstride, const HopDenoise& dn,
                                                   hipStream_t st) {
  return launch_hop_kernels<&stream_hop_tree_denoise_kernel<7, TH>, &stream_hop_tree_denoise_kernel<16, TH>>(
      stream_hop_tree_table_bytes(blob_n, lds_nodes), len, n_streams, n_hops, st, blob, blob_n,
      nf, n_taps, cnodes, nodes, n_nodes, lds_nodes, frames, fstride, len, (const TH*)hop, hstride, hlen, n_streams,
      mfcc_n, ring, count, labels, n_hops, hop_kstride, lab_kstride, node_score, scores, score_kstride, dn);
}

// the denoising form (the same walk rule): scores and node_score may be null
hipError_t launch_stream_hop_tree_denoise(const float* blob, int blob_n, int nf, int n_taps, const TreeNodeC* cnodes,
                                          const TreeNode* nodes, int n_nodes, bool force_global, float* frames,
                                          int64_t fstride, int len, const void* hop, int hop_bytes, int64_t hstride,
                                          int hlen, int64_t n_streams, int mfcc_n, float* ring, int* count,
                                          uint8_t* labels, int n_hops, int64_t hop_kstride, int64_t lab_kstride,
                                          const float* node_score, float* scores, int64_t score_kstride,
                                          const HopDenoise& dn, hipStream_t st) {
  const int lds_nodes = stream_tree_lds_nodes(blob_n, cnodes, n_nodes, force_global);
  const auto launch =
      hop_bytes == 2 ? launch_stream_hop_tree_denoise_t<int16_t> : launch_stream_hop_tree_denoise_t<float>;
  return launch(blob, blob_n, nf, n_taps, cnodes, nodes, n_nodes, lds_nodes, frames, fstride, len, hop,
                hstride, hlen, n_streams, mfcc_n, ring, count, labels, n_hops, hop_kstride, lab_kstride, node_score,
                scores, score_kstride, dn, st);
}

template <class TH>
static hipError_t launch_stream_hop_tree_sessions_t(const float* blob, int blob_n, int nf, int n_taps,
                                                    const TreeNodeC* cnodes, const TreeNode* nodes, int n_nodes,
                                                    int lds_nodes, float* frames, int64_t fstride, int len,
                                                    const void* hop, int64_t hstride, int hlen, int64_t n_streams,
                                                    int mfcc_n, float* ring, int* count, uint8_t* labels, int n_hops,
                                                    int64_t hop_kstride, int64_t lab_kstride, const float* node_score,
                                                    float* scores, int64_t score_kstride, const HopDenoise* dn,
                                                    const int* hop_counts, uint8_t* restart, hipStream_t st) {
  const size_t tables = stream_hop_tree_table_bytes(blob_n, lds_nodes);
  if (dn)
    return launch_hop_kernels<&stream_hop_tree_sessions_denoise_kernel<7, TH>,
                              &stream_hop_tree_sessions_denoise_kernel<16, TH>>(
        tables, len, n_streams, n_hops, st, blob, blob_n, nf, n_taps, cnodes, nodes, n_nodes, lds_nodes, frames,
        fstride, len, (const TH*)hop, hstride, hlen, n_streams, mfcc_n, ring, count, labels, n_hops, hop_kstride,
        lab_kstride, node_score, scores, score_kstride, *dn, hop_counts, restart);
  return launch_hop_kernels<&stream_hop_tree_sessions_kernel<7, TH>, &stream_hop_tree_sessions_kernel<16, TH>>(
      tables, len, n_streams, n_hops, st, blob, blob_n, nf, n_taps, cnodes, nodes, n_nodes, lds_nodes, frames, fstride,
      len, (const TH*)hop, hstride, hlen, n_streams, mfcc_n, ring, count, labels, n_hops, hop_kstride, lab_kstride,
      node_score, scores, score_kstride, hop_counts, restart);
}

// the sessions form (the same walk rule): scores and node_score may be null; dn null: no denoising
hipError_t launch_stream_hop_tree_sessions(const float* blob, int blob_n, int nf, int n_taps, const TreeNodeC* cnodes,
                                           const TreeNode* nodes, int n_nodes, bool force_global, float* frames,
                                           int64_t fstride, int len, const void* hop, int hop_bytes, int64_t hstride,
                                           int hlen, int64_t n_streams, int mfcc_n, float* ring, int* count,
                                           uint8_t* labels, int n_hops, int64_t hop_kstride, int64_t lab_kstride,
                                           const float* node_score, float* scores, int64_t score_kstride,
                                           const HopDenoise* dn, const int* hop_counts, uint8_t* restart,
                                           hipStream_t st) {
  const int lds_nodes = stream_tree_lds_nodes(blob_n, cnodes, n_nodes, force_global);
  const auto launch =
      hop_bytes == 2 ? launch_stream_hop_tree_sessions_t<int16_t> : launch_stream_hop_tree_sessions_t<float>;
  return launch(blob, blob_n, nf, n_taps, cnodes, nodes, n_nodes, lds_nodes, frames, fstride, len, hop,
                hstride, hlen, n_streams, mfcc_n, ring, count, labels, n_hops, hop_kstride, lab_kstride, node_score,
                scores, score_kstride, dn, hop_counts, restart, st);
}

// ---------------------------------------------------------------------------
// The three-kernel form's last step with the tree (stream_ffn_kernel's
// counterpart, after the clip MFCC kernel): per stream, the ring's window in
// arrival order -> analyser features -> the tree, if the stream has seen five
// frames; then the new row into the oldest slot and the count advanced with
// stream_ffn_kernel's rule.  64 streams per block: thread (stream, coefficient)
// computes that coefficient's feature triple into the stream's LDS row and
// pushes its element of the new row (it alone reads and writes that ring
// column); after the barrier one thread per stream walks the compact table
// from global memory (tree_walk_c) and advances the count.
// ---------------------------------------------------------------------------
constexpr int kRingStreams = 64;
constexpr int kRingXStride = 3 * kMaxCoefs + 1;  // odd: the walkers' rows spread over the banks

__global__ __launch_bounds__(256) void stream_tree_ring_kernel(const TreeNodeC* __restrict__ cnodes, int n_nodes,
                                                               const float* __restrict__ newrow,
                                                               float* __restrict__ ring, int* __restrict__ count,
                                                               int64_t n_streams, int mfcc_n,
                                                               uint8_t* __restrict__ labels) {
  __shared__ float X[kRingStreams * kRingXStride];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kRingStreams;
  const int64_t left = n_streams - base;
  const int ns = (int)(left < kRingStreams ? left : kRingStreams);
  for (int i = tid; i < ns * mfcc_n; i += 256) {
    const int w = i / mfcc_n, cc = i - w * mfcc_n;
    const int64_t s = base + w;
    const int c = count[s];
    float* rs = ring + s * 5 * mfcc_n + cc;
    if (c >= 5) {
      const Feat3 ft = feature_triple(rs[((c + 0) % 5) * mfcc_n], rs[((c + 1) % 5) * mfcc_n],
                                      rs[((c + 2) % 5) * mfcc_n], rs[((c + 3) % 5) * mfcc_n],
                                      rs[((c + 4) % 5) * mfcc_n], VAD_FEAT_ANALYSER);
      float* xw = X + w * kRingXStride;
      xw[cc] = ft.mn;
      xw[mfcc_n + cc] = ft.d1;
      xw[2 * mfcc_n + cc] = ft.d2;
    }
    rs[(c % 5) * mfcc_n] = newrow[s * mfcc_n + cc];
  }
  __syncthreads();  // the counts are read above, written below
  if (tid < ns) {
    const int64_t s = base + tid;
    const int c = count[s];
    labels[s] = c >= 5 ? (uint8_t)tree_walk_c(cnodes, n_nodes, X + tid * kRingXStride) : (uint8_t)255;
    count[s] = ring_count_next(c);
  }
}

hipError_t launch_stream_tree_ring(const TreeNodeC* cnodes, int n_nodes, const float* newrow, float* ring, int* count,
                                   int64_t n_streams, int mfcc_n, uint8_t* labels, hipStream_t st) {
  if (n_streams <= 0) return hipSuccess;
  const int64_t blocks = (n_streams + kRingStreams - 1) / kRingStreams;
  hipLaunchKernelGGL(stream_tree_ring_kernel, dim3((unsigned)blocks), dim3(256), 0, st, cnodes, n_nodes, newrow, ring,
                     count, n_streams, mfcc_n, labels);
  return hipGetLastError();
}

}  // namespace vad
