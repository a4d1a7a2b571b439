// Shared device-side definitions for the MI355X (gfx950) VAD hot path.
//
// Everything here is CDNA4-native: 64-lane waves, LDS-staged exchanges,
// f32 MFMA for the FFN.  No CUDA shims, no dual paths.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/vad_amd.h"

namespace vad {

constexpr int kFftN = 512;          // mfcc.py:61 np.fft.fft(frame, 512)
constexpr int kBins = kFftN / 2;    // bins 0..255 kept (Nyquist dropped)
constexpr int kMaxFilters = VAD_MAX_FILTERS;
constexpr int kMaxCoefs = VAD_MAX_MFCC;
constexpr int kMaxTaps = VAD_MAX_TAPS;
constexpr int kMaxGenericFft = VAD_MAX_FFT_N;  // other FFT lengths: spec_generic.hip

// Device-resident MFCC plan.  Read by every wave through scalar loads
// (the indices are wave-uniform), so it lives in plain global memory.
struct MfccDev {
  int n_filters;
  int mfcc_n;
  int wave_fbeg[16];                 // phase-2 filter range per wave
  int wave_fend[16];
  int f_lo[kMaxFilters];             // first tap bin of filter m
  int f_len[kMaxFilters];            // number of taps (contiguous bins)
  int f_off[kMaxFilters];            // offset of filter m's taps in `taps`
  float taps[kMaxTaps];              // filterbank weights (fp32 of the fp64 bank)
  float dct[kMaxCoefs * kMaxFilters];  // lifter(L) x DCT-II ortho, [c][m]
  float2 tw_a[256];                  // W256^(n2*k1), [n2][k1]
  float2 tw_b[256];                  // W512^k
  float window[kFftN];               // optional analysis window (kSpecWindow plans), 0 past the frame
};

// plan variant of a plan with an analysis window (vad_mfcc_plan_set_window)
constexpr int kSpecWindow = 3;
// the launch-time form of a windowed plan whose filterbank is also the
// compiled 26 / 40-filter bank (capi.hip launch_spec): the reference framing
// then runs the paired-frame kernel with those tables and the window
constexpr int kSpecWindow26 = 5;
constexpr int kSpecWindow40 = 6;


typedef float f32x4 __attribute__((ext_vector_type(4)));

// Device view of an FFN plan (passed by value as a kernel argument).
struct FfnDev {
  int n_layers;
  int dims[VAD_MAX_FFN_LAYERS + 1];
  int n_classes;
  int ks0;                        // K-steps of layer 0 = ceil(in_dim / 4) (16 = generic)
  int tiles[VAD_MAX_FFN_LAYERS];  // 16-row output tiles per layer
  const float* frag;              // [slot][64] per-lane fragments: A operands, then biases
  // split-f16 MFMA weights (ref39 / bl13; null = exact f32 MFMA only):
  // [slot][64 lanes][4 words] of packed f16, slot = ((layer, mt, s), hi | lo)
  const uint32_t* fragh;
  // optional (tests): the fp32 logits of every classified row,
  // logits[row * n_classes + c] (null: labels only)
  float* logits;
  // the Keras weights for the one-wave-per-stream VALU forward of the
  // streaming hop kernel: per layer W_l transposed, row o (output unit o)
  // at woff + o * wstride holding W_l[k][o] for k < din rounded up to 4
  // (wstride = that, or 4 more, so that wstride / 4 is odd: lanes reading
  // their rows as 16-B vectors hit every LDS bank once per 16 lanes), then
  // b_l at boff
  const float* wraw;
  int wraw_n;  // floats in wraw
  int woff[VAD_MAX_FFN_LAYERS];
  int boff[VAD_MAX_FFN_LAYERS];
  int wstride[VAD_MAX_FFN_LAYERS];
  // 1: with analyser inputs (|Mn| <= sqrt(5), or a NaN / inf the kernels
  // handle as they come) every finite layer-1 input is below 32768 in
  // magnitude, so that layer needs no f16-range check (capi.hip, from the
  // layer-0 weights: max_j |b_j| + sqrt(5) sum_k |W[k][j]|)
  int h1_bounded;
};

// Decision-tree node (tree_kernel.hip): internal if feature >= 0 (go left
// iff x[feature] <= threshold, or x[feature] is NaN and nan_left), else a
// leaf of class index `leaf`.
struct TreeNode {
  int feature;
  int left;
  int right;
  short leaf;
  short nan_left;  // a NaN feature goes left (sklearn missing_go_to_left)
  double threshold;
};

// Compact node for the LDS-resident walk: 16 B.  feature >= 0: internal,
// bit 30 = missing_go_to_left, bits 0..15 = feature; feature < 0: leaf of
// class -1 - feature.  thr = the largest float <= threshold, so for a float
// x, x <= thr exactly when (double)x <= threshold (sklearn's comparison).
struct TreeNodeC {
  float thr;
  int feature;
  int left;
  int right;
};

// XCD-balanced tile runs of the persistent MFCC kernel (paired-frame path).
// The 8 XCDs of an MI355X run at their own shader clocks under load (one
// box: 2.04-2.26 GHz), while every workgroup of an equal split does the
// same number of cycles, so the slowest XCD sets the launch time.  `word`
// holds 8 weights (8 bits each, >= 1; 0 = equal split): workgroup b's
// share of the tiles is proportional to the weight of b mod 8 (the XCD
// the dispatcher deals it to; a different placement costs balance, never
// correctness: the runs always partition the tiles exactly).  `stats`
// (host-mapped, may be null): per workgroup (tiles << 40) | s_memrealtime
// ticks, from which the host derives the next launch's weights.
struct MfccBalance {
  unsigned long long word = 0;
  unsigned long long* stats = nullptr;
};
// first tile of workgroup b's run (b = G: n_tiles)
__host__ __device__ inline int64_t balanced_tile(unsigned long long word, int64_t n_tiles, int b, int G) {
  if (word == 0) return (int64_t)b * n_tiles / G;
  int64_t w8 = 0, part = 0;
  for (int x = 0; x < 8; ++x) {
    const int64_t w = (int64_t)((word >> (8 * x)) & 255u);
    w8 += w;
    part += x < (b & 7) ? w : 0;
  }
  int64_t tot = (int64_t)(G >> 3) * w8;
  for (int x = 0; x < (G & 7); ++x) tot += (int64_t)((word >> (8 * x)) & 255u);
  return n_tiles * ((int64_t)(b >> 3) * w8 + part) / tot;
}

// Launchers (defined in the .hip translation units).
size_t mfcc_smem_bytes();
hipError_t launch_mfcc(int mode, const MfccDev* plan, int spec, const float* src, int64_t stride,
                       int len, int64_t n, float* out, hipStream_t st, const MfccBalance& bal = MfccBalance());
hipError_t launch_mfcc_i16(int mode, const MfccDev* plan, int spec, const int16_t* src,
                           int64_t stride, int len, int64_t n, float* out, hipStream_t st,
                           const MfccBalance& bal = MfccBalance());
bool mfcc_ffn_fusable(int spec, const FfnDev& net, int frame_size, int hop, const void* audio, int tin_bytes);
hipError_t launch_mfcc_ffn(const MfccDev* plan, const FfnDev& net, const void* audio, int tin_bytes,
                           int64_t n_frames, int mode, uint8_t* labels, hipStream_t st);
hipError_t launch_ffn(const FfnDev& net, int src, const float* in, int64_t n_rows, int mfcc_n,
                      int mode, uint8_t* labels, hipStream_t st);
hipError_t launch_stream_ffn(const FfnDev& net, const float* newrow, float* ring, int* count,
                             int64_t n_streams, int mfcc_n, uint8_t* labels, hipStream_t st);
hipError_t launch_stream_hop(const float* blob, int blob_n, int nf, int n_taps,
                             const FfnDev& net, float* frames, int64_t fstride, int len,
                             const void* hop, int hop_bytes, int64_t hstride, int hlen, int64_t n_streams,
                             int mfcc_n, float* ring, int* count, uint8_t* labels, int n_hops,
                             int64_t hop_kstride, int64_t lab_kstride, hipStream_t st);
// the scored hop kernel: also scores[k * score_kstride + s], class `active`
hipError_t launch_stream_hop_scores(const float* blob, int blob_n, int nf, int n_taps, const FfnDev& net,
                                    float* frames, int64_t fstride, int len, const void* hop, int hop_bytes,
                                    int64_t hstride, int hlen, int64_t n_streams, int mfcc_n, float* ring, int* count,
                                    uint8_t* labels, int n_hops, int64_t hop_kstride, int64_t lab_kstride, int active,
                                    float* scores, int64_t score_kstride, hipStream_t st);
hipError_t launch_stream_push(float* frames, int64_t fstride, int len, const void* hop, int hop_bytes,
                              int64_t hstride, int hlen, int64_t n_streams, hipStream_t st);
// The hop kernel and the ring step with the decision tree
// (stream_tree_kernel.hip).  stream_tree_max_lds_nodes: the largest table the
// hop kernel walks from LDS beside a blob of blob_n floats; force_global walks
// a smaller one from global memory too.
int64_t stream_tree_max_lds_nodes(int blob_n);
// The hop kernels' launch rule (stream_kernel.hip; launch_hop_kernels in
// stream_hop.h calls it): waves per block of a launch whose blocks stage
// `tables` bytes, on the current device; 0 when the tables leave no room for
// one wave's scratch.  The staged bytes of an FFN launch and of a tree launch
// (stream_tree_lds_nodes: the nodes it stages, 0 for a global walk).
int stream_hop_block_waves(size_t tables, int64_t n_streams, int n_hops);
size_t stream_hop_ffn_table_bytes(int blob_n, const FfnDev& net);
int stream_tree_lds_nodes(int blob_n, const TreeNodeC* cnodes, int n_nodes, bool force_global);
size_t stream_hop_tree_table_bytes(int blob_n, int lds_nodes);
hipError_t launch_stream_hop_tree(const float* blob, int blob_n, int nf, int n_taps, const TreeNodeC* cnodes,
                                  const TreeNode* nodes, int n_nodes, bool force_global, float* frames,
                                  int64_t fstride, int len, const void* hop, int hop_bytes, int64_t hstride, int hlen,
                                  int64_t n_streams, int mfcc_n, float* ring, int* count, uint8_t* labels, int n_hops,
                                  int64_t hop_kstride, int64_t lab_kstride, hipStream_t st);
hipError_t launch_stream_hop_tree_scores(const float* blob, int blob_n, int nf, int n_taps, const TreeNodeC* cnodes,
                                         const TreeNode* nodes, int n_nodes, bool force_global, float* frames,
                                         int64_t fstride, int len, const void* hop, int hop_bytes, int64_t hstride,
                                         int hlen, int64_t n_streams, int mfcc_n, float* ring, int* count,
                                         uint8_t* labels, int n_hops, int64_t hop_kstride, int64_t lab_kstride,
                                         const float* node_score, float* scores, int64_t score_kstride,
                                         hipStream_t st);
hipError_t launch_stream_tree_ring(const TreeNodeC* cnodes, int n_nodes, const float* newrow, float* ring, int* count,
                                   int64_t n_streams, int mfcc_n, uint8_t* labels, hipStream_t st);
// Live spectral subtraction in the hop kernels (stream_denoise.h): the state
// of every stream, contiguous, in the kernels' units |2X|^2; all zero = fresh.
constexpr int kNoiseRows = 5;
struct HopDenoise {
  float* spec;      // (S, 5, 256) power rows of the last five frames, slot = the MFCC ring's
  float* rows;      // (S, 5, 256) noise rows in arrival order, row 0 the oldest
  int* held;        // (S) rows held, 0..5
  float* est;       // (S, 256) the noise estimate in force
  float alpha;      // the low pass's coefficient, in [0, 1)
  int noise_class;  // the label whose windows feed the noise rows
  int update;       // 0: the rows and the estimate are frozen
};
// the denoising hop kernels: the scored forms' arguments (scores, and the
// tree's node_score with it, may be null) plus the state
hipError_t launch_stream_hop_denoise(const float* blob, int blob_n, int nf, int n_taps, const FfnDev& net,
                                     float* frames, int64_t fstride, int len, const void* hop, int hop_bytes,
                                     int64_t hstride, int hlen, int64_t n_streams, int mfcc_n, float* ring, int* count,
                                     uint8_t* labels, int n_hops, int64_t hop_kstride, int64_t lab_kstride, int active,
                                     float* scores, int64_t score_kstride, const HopDenoise& dn, hipStream_t st);
hipError_t launch_stream_hop_tree_denoise(const float* blob, int blob_n, int nf, int n_taps, const TreeNodeC* cnodes,
                                          const TreeNode* nodes, int n_nodes, bool force_global, float* frames,
                                          int64_t fstride, int len, const void* hop, int hop_bytes, int64_t hstride,
                                          int hlen, int64_t n_streams, int mfcc_n, float* ring, int* count,
                                          uint8_t* labels, int n_hops, int64_t hop_kstride, int64_t lab_kstride,
                                          const float* node_score, float* scores, int64_t score_kstride,
                                          const HopDenoise& dn, hipStream_t st);
// The sessions hop kernels: the scored form (scores may be null), dn null for
// no denoising, plus hop_counts (S) int32 -- the hops stream s takes from its
// column of the block, clamped to 0..n_hops -- and restart (S) bytes, consumed
hipError_t launch_stream_hop_sessions(const float* blob, int blob_n, int nf, int n_taps, const FfnDev& net,
                                      float* frames, int64_t fstride, int len, const void* hop, int hop_bytes,
                                      int64_t hstride, int hlen, int64_t n_streams, int mfcc_n, float* ring,
                                      int* count, uint8_t* labels, int n_hops, int64_t hop_kstride,
                                      int64_t lab_kstride, int active, float* scores, int64_t score_kstride,
                                      const HopDenoise* dn, const int* hop_counts, uint8_t* restart, hipStream_t st);
hipError_t launch_stream_hop_tree_sessions(const float* blob, int blob_n, int nf, int n_taps, const TreeNodeC* cnodes,
                                           const TreeNode* nodes, int n_nodes, bool force_global, float* frames,
                                           int64_t fstride, int len, const void* hop, int hop_bytes, int64_t hstride,
                                           int hlen, int64_t n_streams, int mfcc_n, float* ring, int* count,
                                           uint8_t* labels, int n_hops, int64_t hop_kstride, int64_t lab_kstride,
                                           const float* node_score, float* scores, int64_t score_kstride,
                                           const HopDenoise* dn, const int* hop_counts, uint8_t* restart,
                                           hipStream_t st);
// n noise frames per stream, (S, n, len) fp32 / int16 (in_bytes 4 / 2), into
// the noise rows, the count and the estimate
hipError_t launch_stream_noise_load(const float* blob, const void* fr, int in_bytes, int64_t sstride, int64_t fstride,
                                    int len, int n, int64_t n_streams, float* rows, int* held, float* est,
                                    float alpha, hipStream_t st);
hipError_t launch_preemphasis(const float* x, float* y, int64_t n_rows, int64_t row_len, int64_t stride, float a,
                              hipStream_t st);
// Streaming segments (stream_segments_kernel.hip): n_hops hops of every
// stream through the segmenter, or n_hops flush hops (labels == nullptr).
// audio_bytes 0: events only (no hop, history, voiced); 4 / 2: fp32 / int16
// samples, strides in elements.  The C entries have checked everything.
constexpr size_t kSegStreamStateBytes = 128;  // per stream; all zero = a stream before its first hop
struct SegStreamArgs {
  const uint8_t* labels;  // nullptr: flush (inactive windows, no new samples; the state ends)
  int64_t lab_kstride;
  int64_t n_streams;
  int n_hops;
  int active;
  int64_t max_gap, min_run, join, delay;  // join = frame_size / hop - 1; delay = D
  int frame_size, hop;
  void* state;
  int64_t* segments;
  int64_t capacity;
  int64_t* found;
  const void* hop_samples;
  int64_t hstride, hop_kstride;
  void* history;
  int ring;  // history elements per stream, <= 2^30
  void* voiced;
  int32_t* voiced_len;
};
hipError_t launch_stream_segments(const SegStreamArgs& a, int audio_bytes, hipStream_t st);
// The operating-point forms: a.labels is the (n_hops, n_streams) block of
// fp32 scores (is_scores; hysteresis on / off) or of uint8 labels, a.delay
// includes pad_before, and a confirmed run is padded before it is queued.
struct SegOpArgs {
  float on, off;
  int is_scores;
  int64_t pad_before, pad_after;  // windows
};
hipError_t launch_stream_segments_op(const SegStreamArgs& a, const SegOpArgs& op, int audio_bytes, hipStream_t st);
// The sessions forms of a push (never a flush: a.labels is the block): stream
// s takes min(max(hop_counts[s], 0), n_hops) hops; restart[s] != 0 ends its
// session first (flush_rows hops into end_voiced / end_len) and is cleared.
// A kernel argument of its own, so the kernels above keep theirs.
struct SegSessArgs {
  const int32_t* hop_counts;  // S
  uint8_t* restart;           // S
  void* end_voiced;           // flush_rows x S x hop (audio forms)
  int32_t* end_len;           // flush_rows x S
  int32_t* table_session;     // S x capacity: the session ordinal of each row of a.segments
  int flush_rows;
};
hipError_t launch_stream_segments_sessions(const SegStreamArgs& a, const SegOpArgs* op, const SegSessArgs& ss,
                                           int audio_bytes, hipStream_t st);
// any fft_n other than 512 (spec_generic.hip): mode 0 frames -> MFCC,
// 1 frames -> spectra, 2 spectra -> MFCC; tw = exp(-2 pi i m / fft_n), fp64
hipError_t launch_generic(int mode, const MfccDev* plan, const float* src, int64_t stride, int len, int64_t n,
                          int fft_n, const double2* tw, float* out, hipStream_t st);
hipError_t launch_generic_i16(int mode, const MfccDev* plan, const int16_t* src, int64_t stride, int len,
                              int64_t n, int fft_n, const double2* tw, float* out, hipStream_t st);
hipError_t launch_features(const float* mfcc, int64_t n_rows, int mfcc_n, int mode, float* out,
                           hipStream_t st);
hipError_t launch_simple_features(const float* frames, int64_t n_frames, int frame_len,
                                  int64_t frame_stride, int L, int pad, int band_bins, int n_bands,
                                  double* out, hipStream_t st);
// Streams of that analyser (simple_stream_kernel.hip).  The C entries have
// checked every argument.  simple_stream_block_fits: L is one the block
// kernel takes (a power of two <= 4096); in_bytes 4 / 2: fp32 / int16 frames.
// frame_counts / restart / init_left: all three for the sessions kernels, all
// null for the plain ones.
bool simple_stream_block_fits(int L);
hipError_t launch_simple_stream_block(const void* frames, int in_bytes, int64_t block_stride, int64_t stream_stride,
                                      int frame_len, int L, int pad, int band_bins, int64_t n_streams, int n_frames,
                                      int nb, void* state, uint8_t* labels, int64_t lab_stride, double* features_out,
                                      void* voiced, int64_t voiced_stride, int32_t* voiced_len,
                                      const int32_t* frame_counts, uint8_t* restart, int32_t* init_left,
                                      hipStream_t st);
hipError_t launch_simple_stream_state(const double* feats, int64_t n_streams, int n_frames, int nb, void* state,
                                      uint8_t* labels, int64_t lab_stride, const float* frames, int64_t block_stride,
                                      int64_t stream_stride, int frame_len, float* voiced, int64_t voiced_stride,
                                      int32_t* voiced_len, const int32_t* frame_counts, uint8_t* restart,
                                      int32_t* init_left, hipStream_t st);
hipError_t launch_simple_stream_init(const double* feats, int64_t n_streams, int nb, void* state, hipStream_t st);
size_t scale_workspace_bytes();
hipError_t launch_scale_features(float* x, int64_t n_rows, int mfcc_n, double* ws, hipStream_t st);
int64_t format_csv_rows(const float* rows, int64_t n_rows, int n_cols, double label, char* buf,
                        int64_t buf_size);
// Dataset CSV import (csv_parse_kernel.hip).  The C entries have checked
// every argument.
size_t csv_workspace_bytes(int64_t n_bytes);
hipError_t launch_csv_count(const uint8_t* bytes, int64_t n, int64_t* n_lines, void* ws, hipStream_t st);
hipError_t launch_csv_index(const uint8_t* bytes, int64_t n, int64_t skip, int64_t base, int64_t* index,
                            int64_t capacity, const void* ws, hipStream_t st);
hipError_t launch_csv_parse(const uint8_t* bytes, int64_t n_bytes, const int64_t* index, int64_t n_rows, int64_t base,
                            int n_cols, const int32_t* columns, int n_used, bool f64, void* x, uint8_t* y,
                            int32_t* status, hipStream_t st);
hipError_t launch_tree_rows(const TreeNode* nodes, int n_nodes, const float* x, int64_t n, int dim,
                            uint8_t* labels, hipStream_t st);
hipError_t launch_tree_windows(const TreeNode* nodes, const TreeNodeC* cnodes, int n_nodes,
                               const float* mfcc, int64_t n_rows,
                               int mfcc_n, int mode, uint8_t* labels, hipStream_t st);
// The same walks ending in node_score[leaf node] (score_kernel.hip).
hipError_t launch_tree_row_scores(const TreeNode* nodes, int n_nodes, const float* node_score, const float* x,
                                  int64_t n, int dim, float* scores, hipStream_t st);
hipError_t launch_tree_window_scores(const TreeNode* nodes, const TreeNodeC* cnodes, int n_nodes,
                                     const float* node_score, const float* mfcc, int64_t n_rows, int mfcc_n, int mode,
                                     float* scores, hipStream_t st);
// Random forest (forest_kernel.hip): tree t is the nodes [roots[t],
// roots[t + 1]) of both tables, its root first and its child indices relative
// to the root; proba holds K class shares per node (rows of leaves are read).
struct ForestDev {
  const TreeNode* nodes;
  const TreeNodeC* cnodes;
  const int* roots;  // T + 1 entries, the last the node count
  const double* proba;
  int T;
  int K;
};
hipError_t launch_forest_rows(const ForestDev& f, const float* x, int64_t n, int dim, int active, uint8_t* labels,
                              float* scores, hipStream_t st);
hipError_t launch_forest_windows(const ForestDev& f, int max_lds_tree, const float* mfcc, int64_t n_rows, int mfcc_n,
                                 int mode, int active, uint8_t* labels, float* scores, hipStream_t st);
// The hop kernels with a forest (stream_forest_kernel.hip): the forest and
// what a launch does with it.  The leading lds_trees trees -- lds_nodes =
// roots[lds_trees] compact nodes -- are staged behind the blob and walked from
// LDS, the others from the global table.
struct HopForest {
  ForestDev f;
  int lds_trees;
  int lds_nodes;
  int max_tree;  // the node count of the largest tree: the bound of a walk
  int active;    // the class whose share is the score
};
// stream_forest_lds_trees: roots is the HOST copy (T + 1 entries).
int stream_forest_lds_trees(int blob_n, const int* roots, int n_trees, bool force_global);
size_t stream_hop_forest_table_bytes(int blob_n, int lds_nodes);
// scores null: labels only; dn null: no denoising; hop_counts and restart
// both null: no sessions
hipError_t launch_stream_hop_forest(const float* blob, int blob_n, int nf, int n_taps, const HopForest& fr,
                                    float* frames, int64_t fstride, int len, const void* hop, int hop_bytes,
                                    int64_t hstride, int hlen, int64_t n_streams, int mfcc_n, float* ring, int* count,
                                    uint8_t* labels, int n_hops, int64_t hop_kstride, int64_t lab_kstride,
                                    float* scores, int64_t score_kstride, const HopDenoise* dn, const int* hop_counts,
                                    uint8_t* restart, hipStream_t st);
// FFN training (train_kernel.hip).  ffn_train_lds_bytes: LDS of one
// workgroup of the step kernel (train) or of the evaluation kernel; the C
// entries refuse what does not fit in 160 KiB before they launch.
int64_t ffn_train_lds_bytes(int n_layers, const int32_t* dims, int batch, bool train);
hipError_t launch_ffn_train(int n_layers, const int32_t* dims, float* state, int64_t n_models, const float* x,
                            const uint8_t* y, const int32_t* order, int64_t order_stride, int batch, int64_t n_steps,
                            const float* hyper, float* step_loss, hipStream_t st);
hipError_t launch_ffn_eval(int n_layers, const int32_t* dims, const float* state, int64_t n_models, const float* x,
                           const uint8_t* y, int64_t n_rows, int64_t n_chunks, float* loss_sums, int32_t* correct,
                           hipStream_t st);

// Decision-tree training (tree_train_kernel.hip).  The C entries have checked
// every argument; tree_train_ws_bytes is 0 where the sizes do not fit.
// weighted: the sizes of the weighted build (a little more than the unweighted).
size_t tree_train_ws_bytes(int64_t n, int F, int n_jobs, const vad_tree_job* jobs, bool weighted = false);
// feature_masks (host, one word per job; null: every feature): bit f set when
// the job may split on feature f.  weighted: mask holds one uint8 weight per
// (job, row), not null, and the weighted kernels run.
int tree_train_run(const float* x, const uint8_t* y, int64_t n, int F, int K, const int32_t* order,
                   const uint8_t* mask, const uint64_t* feature_masks, int n_jobs, const vad_tree_job* jobs,
                   const vad_tree_tables& out, void* ws, size_t ws_bytes, int32_t* n_levels, hipStream_t st,
                   bool weighted = false);

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per kernel and device
// (`done`: one bit per device ordinal, a static of the launch site).
inline hipError_t ensure_dyn_lds(const void* fn, int bytes, std::atomic<unsigned long long>& done) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  const unsigned long long bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.fetch_or(bit, std::memory_order_acq_rel);
  return e;
}

// Two byte ranges share a byte (an empty range overlaps nothing): the entries'
// check of an output against an input.
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return na && nb && x < y + nb && y < x + na;
}

// log10 of a positive energy: native v_log_f32 (with a pre-scale for tiny
// inputs) times log10(2) -- ~1e-7 relative, far inside the 1e-4 budget.
__device__ __forceinline__ float log10_pos(float e) {
  const bool tiny = e < 0x1p-100f;
  const float x = tiny ? e * 0x1p64f : e;
  const float l2 = __builtin_amdgcn_logf(x);  // log2
  return fmaf(l2, 0.30102999566398120f, tiny ? -19.26591972249479649f : 0.f);
}

// NaN-keeping ReLU (numpy / Keras keep NaN; fmaxf would drop it).
__device__ __forceinline__ float relu_nan(float x) { return x < 0.f ? 0.f : x; }

// Floats per row of a table whose rows lanes read as 16-B vectors: n rounded
// up to 4, plus 4 when that is a multiple of 8 (a stride of 4 x odd floats
// puts 16 consecutive lanes' vectors on distinct LDS banks)
__host__ __device__ constexpr int vec_row_stride(int n) {
  return ((n + 3) & ~3) % 8 == 0 ? ((n + 3) & ~3) + 4 : ((n + 3) & ~3);
}

}  // namespace vad
