// Streaming frame assembly: every stream's frame buffer advances by one hop
// (the oldest `hop` samples drop out, the new ones are appended), i.e. the
// frame that SKLearnAnalyzer.feed_frame (sklearn_analyser.py:46-82) receives
// when vad.py:37-49 cuts the live signal into 25 ms frames every 10 ms.
//
// One wave per stream, in place: the wave loads its whole row into
// registers, then stores it shifted.  Store i (sample t = lane + 64 i) waits
// for its own load, hence for every older load of the wave (vmcnt is in
// order), and a younger load i2 > i reads samples >= 64 i2 + hop > 64 i + 63,
// beyond anything store i writes -- so no sample is overwritten before it is
// read.
#include "vad_common.h"
#include "features.h"
#include "ffn_dev.h"
#include "score_dev.h"
#include "stream_hop.h"
#include "stream_denoise.h"

namespace vad {

// TH: the hop samples' type, float or int16_t (PCM as recorded, vad.py:37;
// the (float) of an int16 is exact, so either type leaves the same frames).
// An int16 row is only 2-byte aligned (odd base, odd strides): one 2-byte
// load per sample, lane-contiguous as the fp32 loads are.
template <int NR, class TH>  // registers per lane: frame_len <= 64 NR
__global__ __launch_bounds__(256) void stream_push_kernel(float* __restrict__ frames, int64_t fstride,
                                                          int len, const TH* __restrict__ hop,
                                                          int64_t hstride, int hlen, int64_t n_streams) {
  const int lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= n_streams) return;
  float* row = frames + s * fstride;
  const TH* h = hop + s * hstride;
  const int keep = len - hlen;
  float v[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int t = lane + 64 * i;
    v[i] = t < keep ? row[t + hlen] : (t < len ? (float)h[t - keep] : 0.f);
  }
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int t = lane + 64 * i;
    if (t < len) row[t] = v[i];
  }
}

template <class TH>
static hipError_t launch_stream_push_t(float* frames, int64_t fstride, int len, const TH* hop, int64_t hstride,
                                       int hlen, int64_t n_streams, hipStream_t st) {
  if (n_streams <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n_streams + 3) / 4));
  if (len <= 64 * 7)
    hipLaunchKernelGGL((stream_push_kernel<7, TH>), grid, dim3(256), 0, st, frames, fstride, len, hop, hstride,
                       hlen, n_streams);
  else
    hipLaunchKernelGGL((stream_push_kernel<16, TH>), grid, dim3(256), 0, st, frames, fstride, len, hop, hstride,
                       hlen, n_streams);
  return hipGetLastError();
}

// hop: fp32 samples (hop_bytes 4) or int16 PCM (2); strides in elements
hipError_t launch_stream_push(float* frames, int64_t fstride, int len, const void* hop, int hop_bytes,
                              int64_t hstride, int hlen, int64_t n_streams, hipStream_t st) {
  if (hop_bytes == 2)
    return launch_stream_push_t(frames, fstride, len, (const int16_t*)hop, hstride, hlen, n_streams, st);
  return launch_stream_push_t(frames, fstride, len, (const float*)hop, hstride, hlen, n_streams, st);
}

// Optional pre-emphasis (not in the reference pipeline, mfcc.py:59-61; the
// python_speech_features convention): y[0] = x[0], y[t] = x[t] - a x[t-1]
// along each row (a whole clip is one row).  Elementwise, 16-B vector loads
// of four samples plus the one before them; out of place.
// y[0] = x[0], y[t] = x[t] - a x[t-1] per row (python_speech_features
// sigproc.preemphasis; an optional stage, not in the reference).  Rows go
// over blockIdx.y (no 64-bit division per element); 16-B aligned rows move
// as float4 (four outputs per lane, the one earlier sample as a scalar load
// that the neighbour lane's vector load has already brought into L1).
template <bool VEC4>
__global__ __launch_bounds__(256) void preemphasis_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          int64_t n_rows, int64_t row_len, int64_t stride,
                                                          float a) {
#pragma clang fp contract(off)  // a rounded product, then the difference: numpy's two roundings
  const int64_t quads = (row_len + 3) / 4;
  for (int64_t r = blockIdx.y; r < n_rows; r += gridDim.y) {
    const float* xr = x + r * stride;
    float* yr = y + r * stride;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads;
         q += (int64_t)gridDim.x * blockDim.x) {
      const int64_t t0 = 4 * q;
      const float prev = t0 > 0 ? xr[t0 - 1] : 0.f;
      if (VEC4 && t0 + 3 < row_len) {
        const float4 v = *reinterpret_cast<const float4*>(xr + t0);
        float4 o;
        o.x = t0 == 0 ? v.x : v.x - a * prev;
        o.y = v.y - a * v.x;
        o.z = v.z - a * v.y;
        o.w = v.w - a * v.z;
        *reinterpret_cast<float4*>(yr + t0) = o;
      } else {
        float p = prev;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int64_t t = t0 + k;
          if (t < row_len) {
            const float v = xr[t];
            yr[t] = t == 0 ? v : v - a * p;
            p = v;
          }
        }
      }
    }
  }
}

hipError_t launch_preemphasis(const float* x, float* y, int64_t n_rows, int64_t row_len, int64_t stride, float a,
                              hipStream_t st) {
  if (n_rows <= 0 || row_len <= 0) return hipSuccess;
  const int64_t quads = (row_len + 3) / 4;
  int64_t bx = (quads + 255) / 256;
  if (bx > 8192) bx = 8192;
  int64_t by = n_rows < 65535 ? n_rows : 65535;
  while (bx * by > 65536 && bx > 1) bx = (bx + 1) / 2;  // about 16M threads in all
  const bool vec4 = (reinterpret_cast<uintptr_t>(x) % 16 == 0) && (reinterpret_cast<uintptr_t>(y) % 16 == 0) &&
                    (n_rows == 1 || stride % 4 == 0);
  if (vec4)
    hipLaunchKernelGGL(preemphasis_kernel<true>, dim3((unsigned)bx, (unsigned)by), dim3(256), 0, st, x, y, n_rows,
                       row_len, stride, a);
  else
    hipLaunchKernelGGL(preemphasis_kernel<false>, dim3((unsigned)bx, (unsigned)by), dim3(256), 0, st, x, y, n_rows,
                       row_len, stride, a);
  return hipGetLastError();
}


// ---------------------------------------------------------------------------
// One analyser hop of every stream in ONE kernel, one wave per stream
// (BASELINE config 5: many small batches, latency first).  The clip kernels
// spread a 64-frame tile over a workgroup; a hop brings one frame per
// stream, so here each wave owns its stream end to end:
//   frame    advance the 400-sample buffer by the hop (as stream_push_kernel)
//   FFT      z[n] = x[2n] + i x[2n+1] (zero past min(len, 512)), 256-point
//            Stockham radix-4 (4 stages through wave-private LDS, lane j
//            one butterfly per stage), then the real-FFT split into
//            |2X[k]|^2, k = 0..255 (the 2^-20 of |X/512|^2 sits in the taps)
//   mel      lane m: filter m's taps, (==0 -> eps), log10 (mfcc.py:72-75)
//   DCT      lane c: lifter x DCT-II ortho row c (mfcc.py:76-78)
//   window   the ring's five rows in arrival order -> analyser features
//            (sklearn_analyser.py:52-69), classified if the stream has seen
//            five frames, then the new row pushed (:71-74)
//   FFN      exact f32 on the VALU, lane o = output unit o, weights as given
//            (ffn_trainer.py:106-116), NaN-keeping ReLU, np.argmax rules.
// Lanes within the wave exchange through LDS only (in order per wave): no
// workgroup barrier anywhere.
// ---------------------------------------------------------------------------
// NR: 64-sample chunks of the frame a lane holds (7: frames up to 448
// samples, the reference's 400; 16: up to 1024) -- the frame and the next
// hop's samples stay in registers across hops, so the bound matters.
// TH: the hop samples' type (float, or int16_t PCM converted by an exact
// (float) where it is loaded -- the two sites that read `hop`; frames, ring
// and counts are fp32 either way, and everything after the load is one code)

template <int NR, class TH>
__global__ __launch_bounds__(1024) void stream_hop_kernel(const float* __restrict__ blob, int blob_n, int nf,
                                                          int n_taps, FfnDev net,
                                                          float* __restrict__ frames, int64_t fstride, int len,
                                                          const TH* __restrict__ hop, int64_t hstride,
                                                          int hlen, int64_t n_streams, int mfcc_n,
                                                          float* __restrict__ ring, int* __restrict__ count,
                                                          uint8_t* __restrict__ labels, int n_hops,
                                                          int64_t hop_kstride, int64_t lab_kstride) {
#define VAD_HOP_SCORE 0
#define VAD_HOP_DENOISE 0
#define VAD_HOP_SESSIONS 0
#include "stream_hop_ffn_body.inc"
#undef VAD_HOP_SESSIONS
#undef VAD_HOP_DENOISE
#undef VAD_HOP_SCORE
}

// The scored form: the same body, plus one fp32 score per (hop, stream).
template <int NR, class TH>
__global__ __launch_bounds__(1024) void stream_hop_scores_kernel(
    const float* __restrict__ blob, int blob_n, int nf, int n_taps, FfnDev net, float* __restrict__ frames,
    int64_t fstride, int len, const TH* __restrict__ hop, int64_t hstride, int hlen, int64_t n_streams, int mfcc_n,
    float* __restrict__ ring, int* __restrict__ count, uint8_t* __restrict__ labels, int n_hops, int64_t hop_kstride,
    int64_t lab_kstride, int active, float* __restrict__ scores, int64_t score_kstride) {
#define VAD_HOP_SCORE 1
#define VAD_HOP_DENOISE 0
#define VAD_HOP_SESSIONS 0
#include "stream_hop_ffn_body.inc"
#undef VAD_HOP_SESSIONS
#undef VAD_HOP_DENOISE
#undef VAD_HOP_SCORE
}

// The denoising form (stream_denoise.h): the scored kernel's arguments plus
// the denoise state; `scores` may be null.
template <int NR, class TH>
__global__ __launch_bounds__(1024) void stream_hop_denoise_kernel(
    const float* __restrict__ blob, int blob_n, int nf, int n_taps, FfnDev net, float* __restrict__ frames,
    int64_t fstride, int len, const TH* __restrict__ hop, int64_t hstride, int hlen, int64_t n_streams, int mfcc_n,
    float* __restrict__ ring, int* __restrict__ count, uint8_t* __restrict__ labels, int n_hops, int64_t hop_kstride,
    int64_t lab_kstride, int active, float* __restrict__ scores, int64_t score_kstride, HopDenoise dn) {
#define VAD_HOP_SCORE 1
#define VAD_HOP_DENOISE 1
#define VAD_HOP_SESSIONS 0
#include "stream_hop_ffn_body.inc"
#undef VAD_HOP_SESSIONS
#undef VAD_HOP_DENOISE
#undef VAD_HOP_SCORE
}

// The sessions forms: the scored kernel (scores may be null), without and
// with the denoise state, plus per stream the hops it takes in this launch
// (hop_counts, clamped to 0..n_hops) and a restart flag the kernel consumes.
// Rows n_s..n_hops-1 of a stream's labels hold VAD_LABEL_NO_HOP, of its scores
// NaN; a stream with no hop and no restart writes nothing else.
template <int NR, class TH>
__global__ __launch_bounds__(1024) void stream_hop_sessions_kernel(
    const float* __restrict__ blob, int blob_n, int nf, int n_taps, FfnDev net, float* __restrict__ frames,
    int64_t fstride, int len, const TH* __restrict__ hop, int64_t hstride, int hlen, int64_t n_streams, int mfcc_n,
    float* __restrict__ ring, int* __restrict__ count, uint8_t* __restrict__ labels, int n_hops, int64_t hop_kstride,
    int64_t lab_kstride, int active, float* __restrict__ scores, int64_t score_kstride,
    const int* __restrict__ hop_counts, uint8_t* __restrict__ restart) {
#define VAD_HOP_SCORE 1
#define VAD_HOP_DENOISE 0
#define VAD_HOP_SESSIONS 1
#include "stream_hop_ffn_body.inc"
#undef VAD_HOP_SESSIONS
#undef VAD_HOP_DENOISE
#undef VAD_HOP_SCORE
}

template <int NR, class TH>
__global__ __launch_bounds__(1024) void stream_hop_sessions_denoise_kernel(
    const float* __restrict__ blob, int blob_n, int nf, int n_taps, FfnDev net, float* __restrict__ frames,
    int64_t fstride, int len, const TH* __restrict__ hop, int64_t hstride, int hlen, int64_t n_streams, int mfcc_n,
    float* __restrict__ ring, int* __restrict__ count, uint8_t* __restrict__ labels, int n_hops, int64_t hop_kstride,
    int64_t lab_kstride, int active, float* __restrict__ scores, int64_t score_kstride, HopDenoise dn,
    const int* __restrict__ hop_counts, uint8_t* __restrict__ restart) {
#define VAD_HOP_SCORE 1
#define VAD_HOP_DENOISE 1
#define VAD_HOP_SESSIONS 1
#include "stream_hop_ffn_body.inc"
#undef VAD_HOP_SESSIONS
#undef VAD_HOP_DENOISE
#undef VAD_HOP_SCORE
}

// The launch rule of every hop kernel (stream_hop.h has its reasons and
// measurements): waves per block, 0 when not even one wave's scratch fits.
int stream_hop_block_waves(size_t tables, int64_t n_streams, int n_hops) {
  if (tables + kHopWaveFloats * sizeof(float) > kHopLdsBytes) return 0;  // before any device call
  static std::atomic<int> n_cu_seen{0};
  int n_cu = n_cu_seen.load(std::memory_order_relaxed);
  if (n_cu == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0)
      n_cu = 256;
    n_cu_seen.store(n_cu, std::memory_order_relaxed);
  }
  int waves = n_hops > 1 ? kHopMinWavesK : kHopMinWaves;
  while (waves < 16 && (int64_t)waves * n_cu < n_streams) waves <<= 1;
  while (waves > 1 && tables + (size_t)waves * kHopWaveFloats * sizeof(float) > kHopLdsBytes) waves >>= 1;
  return waves;
}

size_t stream_hop_ffn_table_bytes(int blob_n, const FfnDev& net) {
  return (size_t)(blob_n + net.wraw_n) * sizeof(float);
}

template <class TH>
static hipError_t launch_stream_hop_sessions_t(const float* blob, int blob_n, int nf, int n_taps, const FfnDev& net,
                                               float* frames, int64_t fstride, int len, const void* hop,
                                               int64_t hstride, int hlen, int64_t n_streams, int mfcc_n, float* ring,
                                               int* count, uint8_t* labels, int n_hops, int64_t hop_kstride,
                                               int64_t lab_kstride, int active, float* scores, int64_t score_kstride,
                                               const HopDenoise* dn, const int* hop_counts, uint8_t* restart,
                                               hipStream_t st) {
  const size_t tables = stream_hop_ffn_table_bytes(blob_n, net);
  if (dn)
    return launch_hop_kernels<&stream_hop_sessions_denoise_kernel<7, TH>, &stream_hop_sessions_denoise_kernel<16, TH>>(
        tables, len, n_streams, n_hops, st, blob, blob_n, nf, n_taps, net, frames, fstride, len, (const TH*)hop, hstride,
        hlen, n_streams, mfcc_n, ring, count, labels, n_hops, hop_kstride, lab_kstride, active, scores, score_kstride,
        *dn, hop_counts, restart);
  return launch_hop_kernels<&stream_hop_sessions_kernel<7, TH>, &stream_hop_sessions_kernel<16, TH>>(
      tables, len, n_streams, n_hops, st, blob, blob_n, nf, n_taps, net, frames, fstride, len, (const TH*)hop, hstride,
      hlen, n_streams, mfcc_n, ring, count, labels, n_hops, hop_kstride, lab_kstride, active, scores, score_kstride,
      hop_counts, restart);
}

template <class TH>
static hipError_t launch_stream_hop_t(const float* blob, int blob_n, int nf, int n_taps, const FfnDev& net,
                                      float* frames, int64_t fstride, int len, const void* hop, int64_t hstride,
                                      int hlen, int64_t n_streams, int mfcc_n, float* ring, int* count,
                                      uint8_t* labels, int n_hops, int64_t hop_kstride, int64_t lab_kstride,
                                      hipStream_t st) {
  return launch_hop_kernels<&stream_hop_kernel<7, TH>, &stream_hop_kernel<16, TH>>(
      stream_hop_ffn_table_bytes(blob_n, net), len, n_streams, n_hops, st, blob, blob_n, nf, n_taps, net,
      frames, fstride, len, (const TH*)hop, hstride, hlen, n_streams, mfcc_n, ring, count, labels, n_hops,
      hop_kstride, lab_kstride);
}

template <class TH>
static hipError_t launch_stream_hop_scores_t(const float* blob, int blob_n, int nf, int n_taps, const FfnDev& net,
                                             float* frames, int64_t fstride, int len, const void* hop,
                                             int64_t hstride, int hlen, int64_t n_streams, int mfcc_n, float* ring,
                                             int* count, uint8_t* labels, int n_hops, int64_t hop_kstride,
                                             int64_t lab_kstride, int active, float* scores, int64_t score_kstride,
                                             hipStream_t st) {
  return launch_hop_kernels<&stream_hop_scores_kernel<7, TH>, &stream_hop_scores_kernel<16, TH>>(
      stream_hop_ffn_table_bytes(blob_n, net), len, n_streams, n_hops, st, blob, blob_n, nf, n_taps, net,
      frames, fstride, len, (const TH*)hop, hstride, hlen, n_streams, mfcc_n, ring, count, labels, n_hops,
      hop_kstride, lab_kstride, active, scores, score_kstride);
}

template <class TH>
static hipError_t launch_stream_hop_denoise_t(const float* blob, int blob_n, int nf, int n_taps, const FfnDev& net,
                                              float* frames, int64_t fstride, int len, const void* hop,
                                              int64_t hstride, int hlen, int64_t n_streams, int mfcc_n, float* ring,
                                              int* count, uint8_t* labels, int n_hops, int64_t hop_kstride,
                                              int64_t lab_kstride, int active, float* scores, int64_t score_kstride,
                                              const HopDenoise& dn, hipStream_t st) {
  return launch_hop_kernels<&stream_hop_denoise_kernel<7, TH>, &stream_hop_denoise_kernel<16, TH>>(
      stream_hop_ffn_table_bytes(blob_n, net), len, n_streams, n_hops, st, blob, blob_n, nf, n_taps, net,
      frames, fstride, len, (const TH*)hop, hstride, hlen, n_streams, mfcc_n, ring, count, labels, n_hops,
      hop_kstride, lab_kstride, active, scores, score_kstride, dn);
}

// hop: fp32 samples (hop_bytes 4) or int16 PCM (2); strides in elements
hipError_t launch_stream_hop(const float* blob, int blob_n, int nf, int n_taps, const FfnDev& net, float* frames,
                             int64_t fstride, int len, const void* hop, int hop_bytes, int64_t hstride, int hlen,
                             int64_t n_streams, int mfcc_n, float* ring, int* count, uint8_t* labels, int n_hops,
                             int64_t hop_kstride, int64_t lab_kstride, hipStream_t st) {
  const auto launch = hop_bytes == 2 ? launch_stream_hop_t<int16_t> : launch_stream_hop_t<float>;
  return launch(blob, blob_n, nf, n_taps, net, frames, fstride, len, hop, hstride, hlen, n_streams, mfcc_n, ring,
                count, labels, n_hops, hop_kstride, lab_kstride, st);
}

// the scored form: scores[k * score_kstride + s] beside labels[k * lab_kstride + s]
hipError_t launch_stream_hop_scores(const float* blob, int blob_n, int nf, int n_taps, const FfnDev& net,
                                    float* frames, int64_t fstride, int len, const void* hop, int hop_bytes,
                                    int64_t hstride, int hlen, int64_t n_streams, int mfcc_n, float* ring, int* count,
                                    uint8_t* labels, int n_hops, int64_t hop_kstride, int64_t lab_kstride, int active,
                                    float* scores, int64_t score_kstride, hipStream_t st) {
  const auto launch = hop_bytes == 2 ? launch_stream_hop_scores_t<int16_t> : launch_stream_hop_scores_t<float>;
  return launch(blob, blob_n, nf, n_taps, net, frames, fstride, len, hop, hstride, hlen, n_streams, mfcc_n, ring,
                count, labels, n_hops, hop_kstride, lab_kstride, active, scores, score_kstride, st);
}

// the denoising form: scores may be null
hipError_t launch_stream_hop_denoise(const float* blob, int blob_n, int nf, int n_taps, const FfnDev& net,
                                     float* frames, int64_t fstride, int len, const void* hop, int hop_bytes,
                                     int64_t hstride, int hlen, int64_t n_streams, int mfcc_n, float* ring, int* count,
                                     uint8_t* labels, int n_hops, int64_t hop_kstride, int64_t lab_kstride, int active,
                                     float* scores, int64_t score_kstride, const HopDenoise& dn, hipStream_t st) {
  const auto launch = hop_bytes == 2 ? launch_stream_hop_denoise_t<int16_t> : launch_stream_hop_denoise_t<float>;
  return launch(blob, blob_n, nf, n_taps, net, frames, fstride, len, hop, hstride, hlen, n_streams, mfcc_n, ring,
                count, labels, n_hops, hop_kstride, lab_kstride, active, scores, score_kstride, dn, st);
}

// the sessions form: scores may be null; dn null: no denoising
hipError_t launch_stream_hop_sessions(const float* blob, int blob_n, int nf, int n_taps, const FfnDev& net,
                                      float* frames, int64_t fstride, int len, const void* hop, int hop_bytes,
                                      int64_t hstride, int hlen, int64_t n_streams, int mfcc_n, float* ring,
                                      int* count, uint8_t* labels, int n_hops, int64_t hop_kstride,
                                      int64_t lab_kstride, int active, float* scores, int64_t score_kstride,
                                      const HopDenoise* dn, const int* hop_counts, uint8_t* restart, hipStream_t st) {
  const auto launch = hop_bytes == 2 ? launch_stream_hop_sessions_t<int16_t> : launch_stream_hop_sessions_t<float>;
  return launch(blob, blob_n, nf, n_taps, net, frames, fstride, len, hop, hstride, hlen, n_streams, mfcc_n, ring,
                count, labels, n_hops, hop_kstride, lab_kstride, active, scores, score_kstride, dn, hop_counts,
                restart, st);
}

// ---------------------------------------------------------------------------
// The noise frames of every stream (load_init_inactive_frames,
// sklearn_analyser.py:40-44): n frames per stream become the n noise rows, in
// the order given, and the estimate is taken from them.  One wave per stream;
// a row is the hop kernels' power spectrum of that frame, bit for bit
// (dn_frame_power).  No barrier: a wave's LDS is its own.
// ---------------------------------------------------------------------------
template <class TH>
__global__ __launch_bounds__(256) void stream_noise_load_kernel(const float* __restrict__ blob,
                                                                const TH* __restrict__ fr, int64_t sstride,
                                                                int64_t fstride, int len, int n, int64_t n_streams,
                                                                float* __restrict__ rows, int* __restrict__ held,
                                                                float* __restrict__ est, float alpha) {
  __shared__ __attribute__((aligned(16))) float sm[4 * 2 * kHopZ];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.x * 4 + wv;
  if (s >= n_streams) return;
  float2* z0 = reinterpret_cast<float2*>(sm + wv * 2 * kHopZ);
  float2* z1 = reinterpret_cast<float2*>(sm + wv * 2 * kHopZ + kHopZ);
  const float2* tw = reinterpret_cast<const float2*>(blob);
  const int used = len < kFftN ? len : kFftN;
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int j = 0; j < n; ++j) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const TH* x = fr + s * sstride + (int64_t)j * fstride;
    float* xs = reinterpret_cast<float*>(z1);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int t = ln + 64 * i;
      xs[2 * zp(t >> 1) + (t & 1)] = t < used ? (float)x[t] : 0.f;
    }
    asm volatile("" ::: "memory");
    dn_frame_power(z0, z1, tw, ln);
    const float4 p = reinterpret_cast<const float4*>(z0)[ln];
    reinterpret_cast<float4*>(rows + (s * kNoiseRows + j) * kBins)[ln] = p;
    sum = j == 0 ? p : make_float4(sum.x + p.x, sum.y + p.y, sum.z + p.z, sum.w + p.w);
    asm volatile("" ::: "memory");
  }
  const float fn = (float)n;
  const float4 m = make_float4(sum.x / fn, sum.y / fn, sum.z / fn, sum.w / fn);
  reinterpret_cast<float4*>(est + s * kBins)[lane] = dn_estimate(m, alpha, lane);
  if (lane == 0) held[s] = n;
}

// fr: (S, n, len) fp32 (in_bytes 4) or int16 (2); strides in elements
hipError_t launch_stream_noise_load(const float* blob, const void* fr, int in_bytes, int64_t sstride, int64_t fstride,
                                    int len, int n, int64_t n_streams, float* rows, int* held, float* est,
                                    float alpha, hipStream_t st) {
  if (n_streams <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n_streams + 3) / 4));
  if (in_bytes == 2)
    hipLaunchKernelGGL(stream_noise_load_kernel<int16_t>, grid, dim3(256), 0, st, blob, (const int16_t*)fr, sstride,
                       fstride, len, n, n_streams, rows, held, est, alpha);
  else
    hipLaunchKernelGGL(stream_noise_load_kernel<float>, grid, dim3(256), 0, st, blob, (const float*)fr, sstride,
                       fstride, len, n, n_streams, rows, held, est, alpha);
  return hipGetLastError();
}

}  // namespace vad
