// Streaming hops labelled and scored by a random forest: the forest
// counterpart of stream_tree_kernel.hip's hop kernels, one wave per stream.
//
// A stream has one window per hop, so with one tree all 64 lanes would take
// the same path and 63 of them idle through a chain of dependent LDS reads
// (stream_hop_tree_kernel keeps the node index uniform).  With a forest lane
// l walks tree l: T independent chains side by side, in the time of the
// deepest one; trees 64 .. 127 follow in a second pass, and so on.  The
// window's features are the wave's LDS row, read by every lane at its own
// index.
//
// The average is forest_kernel.hip's, operation for operation: K <= 8 double
// sums start at 0, take proba[roots[t] + leaf_t][k] for t = 0 .. T-1 in order,
// and are divided by (double)T; the score is (float) of class `active`, the
// label the first maximum.  Lane t fetches its leaf's K shares (one global
// read per class, all lanes at once) into an LDS row of the wave's dead FFT
// buffers, and lane k < K adds column k in tree order: T adds deep, not T K.
//
// Staging: the compact nodes (ForestDev::cnodes, child indices relative to the
// tree's root) of the longest prefix of WHOLE trees that fits beside the blob
// and kForestStageWaves waves' scratch go behind the MFCC blob by the same
// LDS-DMA loop; lanes whose tree lies past the prefix walk the 24-byte global
// table (double threshold).  tree_walk = global stages nothing.
//
// The front end is stream_hop_tree_body.inc's, statement for statement
// (stream_hop_forest_body.inc); this is a unit of its own so that the twelve
// FFN and tree hop kernels keep their instructions
// (profiles/stream_forest/isa.md).  No atomics, one barrier (the staging's),
// no workgroup waits on another.
#include "vad_common.h"
#include "features.h"
#include "stream_hop.h"
#include "stream_denoise.h"

#ifndef VAD_FOREST_STAGE_WAVES
#define VAD_FOREST_STAGE_WAVES 1  // the staged trees leave room for this many waves' scratch (1: all that fits)
#endif

namespace vad {

#define VAD_HOP_FOREST_ARGS                                                                                          \
  const float* __restrict__ blob, int blob_n, int nf, int n_taps, HopForest fr, float* __restrict__ frames,          \
      int64_t fstride, int len, const TH* __restrict__ hop, int64_t hstride, int hlen, int64_t n_streams,            \
      int mfcc_n, float* __restrict__ ring, int* __restrict__ count, uint8_t* __restrict__ labels, int n_hops,       \
      int64_t hop_kstride, int64_t lab_kstride, float* __restrict__ scores, int64_t score_kstride

// NR, TH: as stream_hop_kernel.  `scores` may be null in every form.
template <int NR, class TH>
__global__ __launch_bounds__(1024) void stream_hop_forest_kernel(VAD_HOP_FOREST_ARGS) {
#define VAD_HOP_DENOISE 0
#define VAD_HOP_SESSIONS 0
#include "stream_hop_forest_body.inc"
#undef VAD_HOP_SESSIONS
#undef VAD_HOP_DENOISE
}

template <int NR, class TH>
__global__ __launch_bounds__(1024) void stream_hop_forest_denoise_kernel(VAD_HOP_FOREST_ARGS, HopDenoise dn) {
#define VAD_HOP_DENOISE 1
#define VAD_HOP_SESSIONS 0
#include "stream_hop_forest_body.inc"
#undef VAD_HOP_SESSIONS
#undef VAD_HOP_DENOISE
}

template <int NR, class TH>
__global__ __launch_bounds__(1024) void stream_hop_forest_sessions_kernel(VAD_HOP_FOREST_ARGS,
                                                                          const int* __restrict__ hop_counts,
                                                                          uint8_t* __restrict__ restart) {
#define VAD_HOP_DENOISE 0
#define VAD_HOP_SESSIONS 1
#include "stream_hop_forest_body.inc"
#undef VAD_HOP_SESSIONS
#undef VAD_HOP_DENOISE
}

template <int NR, class TH>
__global__ __launch_bounds__(1024) void stream_hop_forest_sessions_denoise_kernel(VAD_HOP_FOREST_ARGS, HopDenoise dn,
                                                                                  const int* __restrict__ hop_counts,
                                                                                  uint8_t* __restrict__ restart) {
#define VAD_HOP_DENOISE 1
#define VAD_HOP_SESSIONS 1
#include "stream_hop_forest_body.inc"
#undef VAD_HOP_SESSIONS
#undef VAD_HOP_DENOISE
}

#undef VAD_HOP_FOREST_ARGS

// The leading trees a launch stages: the longest prefix of whole trees whose
// compact nodes fit beside the blob and the scratch of kForestStageWaves
// waves.  roots: T + 1 host entries, the last the node count.
constexpr int kForestStageWaves = VAD_FOREST_STAGE_WAVES;

int stream_forest_lds_trees(int blob_n, const int* roots, int n_trees, bool force_global) {
  if (force_global || !roots) return 0;
  const int64_t room = (int64_t)kHopLdsBytes - (int64_t)blob_n * sizeof(float) -
                       (int64_t)kForestStageWaves * kHopWaveFloats * sizeof(float);
  const int64_t max_nodes = room > 0 ? room / (int64_t)sizeof(TreeNodeC) : 0;
  int t = 0;
  while (t < n_trees && roots[t + 1] <= max_nodes) ++t;
  return t;
}

size_t stream_hop_forest_table_bytes(int blob_n, int lds_nodes) {
  return (size_t)blob_n * sizeof(float) + (size_t)lds_nodes * sizeof(TreeNodeC);
}

template <class TH>
static hipError_t launch_stream_hop_forest_t(const float* blob, int blob_n, int nf, int n_taps, const HopForest& fr,
                                             float* frames, int64_t fstride, int len, const void* hop,
                                             int64_t hstride, int hlen, int64_t n_streams, int mfcc_n, float* ring,
                                             int* count, uint8_t* labels, int n_hops, int64_t hop_kstride,
                                             int64_t lab_kstride, float* scores, int64_t score_kstride,
                                             const HopDenoise* dn, const int* hop_counts, uint8_t* restart,
                                             hipStream_t st) {
  const size_t tables = stream_hop_forest_table_bytes(blob_n, fr.lds_nodes);
#define VAD_FOREST_HOP_LAUNCH(KERNEL, ...)                                                                           \
  launch_hop_kernels<&KERNEL<7, TH>, &KERNEL<16, TH>>(                                                               \
      tables, len, n_streams, n_hops, st, blob, blob_n, nf, n_taps, fr, frames, fstride, len, (const TH*)hop,        \
      hstride, hlen, n_streams, mfcc_n, ring, count, labels, n_hops, hop_kstride, lab_kstride, scores,               \
      score_kstride, ##__VA_ARGS__)
  if (hop_counts && dn) return VAD_FOREST_HOP_LAUNCH(stream_hop_forest_sessions_denoise_kernel, *dn, hop_counts, restart);
  if (hop_counts) return VAD_FOREST_HOP_LAUNCH(stream_hop_forest_sessions_kernel, hop_counts, restart);
  if (dn) return VAD_FOREST_HOP_LAUNCH(stream_hop_forest_denoise_kernel, *dn);
  return VAD_FOREST_HOP_LAUNCH(stream_hop_forest_kernel);
#undef VAD_FOREST_HOP_LAUNCH
}

// hop: fp32 samples (hop_bytes 4) or int16 PCM (2); strides in elements.
// scores null: labels only; dn null: no denoising; hop_counts and restart both
// null: no sessions.
hipError_t launch_stream_hop_forest(const float* blob, int blob_n, int nf, int n_taps, const HopForest& fr,
                                    float* frames, int64_t fstride, int len, const void* hop, int hop_bytes,
                                    int64_t hstride, int hlen, int64_t n_streams, int mfcc_n, float* ring, int* count,
                                    uint8_t* labels, int n_hops, int64_t hop_kstride, int64_t lab_kstride,
                                    float* scores, int64_t score_kstride, const HopDenoise* dn, const int* hop_counts,
                                    uint8_t* restart, hipStream_t st) {
  const auto launch = hop_bytes == 2 ? launch_stream_hop_forest_t<int16_t> : launch_stream_hop_forest_t<float>;
  return launch(blob, blob_n, nf, n_taps, fr, frames, fstride, len, hop, hstride, hlen, n_streams, mfcc_n, ring,
                count, labels, n_hops, hop_kstride, lab_kstride, scores, score_kstride, dn, hop_counts, restart, st);
}

}  // namespace vad
