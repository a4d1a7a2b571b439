// Many live streams of the energy / ZCR / spectral analyser
// (realtime_analysis/simple_analyzer.py: SimpleAnalyser.feed_frame) per
// launch, every stream's state on the device.
//
// Within a block of K frames the features of every (stream, frame) pair do
// not depend on state, and a stream's state machine is serial but small: so
// the feature rows are computed in parallel and each stream's state is then
// stepped K times, in order.
//
//   simple_stream_block_kernel<T>  power-of-two L <= 4096: one workgroup per
//       stream, one frame per wave and round (simple_wave.h, the body of
//       simple_features_wave_kernel), the rows in LDS, one lane stepping the
//       state after each round's barrier.
//   simple_stream_state_kernel     the state steps alone, over feature rows
//       in global memory: the second launch for every other L (after
//       launch_simple_features), and the entry for hand-made rows.
//   simple_stream_init_kernel      load_init_inactive_frames for all streams.
//
// No workgroup waits on another; there are no atomics.
#include "simple_state.h"
#include "simple_wave.h"
#include "vad_common.h"

namespace vad {

constexpr int kStreamBlockLds = 160 * 1024;  // the budget simple_kernel.hip sets itself
constexpr int kStreamBlockMaxWaves = 4;
constexpr int kFeatRow = 8;  // doubles per feature row in LDS (7 used)

// LDS of a block-kernel workgroup of `waves` waves, in doubles.
__host__ __device__ constexpr size_t stream_block_doubles(int L, int waves, int nb) {
  // twiddles, per wave re / im, the noise rows, two rounds of rows, two rounds of voiced slots
  return (size_t)L + (size_t)waves * 2 * L + (size_t)kSimpleNoiseCols * nb + (size_t)2 * waves * kFeatRow +
         (size_t)waves;
}

struct SimpleBlockArgs {
  const void* frames;  // (K, S, frame_len): frames + k * block_stride + s * stream_stride
  int64_t block_stride, stream_stride;
  int frame_len, L, pad, band_bins;
  int n_frames, nb;
  int64_t n_streams;
  void* state;
  uint8_t* labels;  // labels[k * lab_stride + s]
  int64_t lab_stride;
  double* features_out;  // (K, S, 7) or null
  void* voiced;          // (S, voiced_stride) of the input type, or null
  int64_t voiced_stride;
  int32_t* voiced_len;
};

// Dynamic LDS: [L/2] cos, [L/2] sin, per wave [L] re + [L] im, the stream's
// noise rows, rows[2][waves][8], slot[2][waves].  Round r (frames r * waves
// ... ) writes rows[r & 1]; after the round's barrier lane 0 of wave 0 steps
// the state over them while the other waves start round r + 1 in the other
// half, so one barrier per round is enough: rows[r & 1] is written again only
// after barrier r + 1, which wave 0 reaches after it has read them.  slot
// (the place of an active frame in the stream's voiced output, -1 inactive)
// is read one barrier after it is written, in the same two halves.
template <typename T>
__global__ __launch_bounds__(64 * kStreamBlockMaxWaves) void simple_stream_block_kernel(SimpleBlockArgs a) {
  extern __shared__ __attribute__((aligned(16))) double ssm[];
  const int L = a.L, nb = a.nb, K = a.n_frames;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int waves = blockDim.x >> 6;
  double* twc = ssm;
  double* tws = ssm + (L >> 1);
  double* re = ssm + L + (size_t)wave * 2 * L;
  double* im = re + L;
  double* noise = ssm + L + (size_t)waves * 2 * L;
  double* rows = noise + kSimpleNoiseCols * nb;
  int* slot = reinterpret_cast<int*>(rows + 2 * waves * kFeatRow);
  const int64_t s = blockIdx.x;
  double* st = reinterpret_cast<double*>(static_cast<char*>(a.state) + s * simple_state_bytes(nb));
  const T* frames = static_cast<const T*>(a.frames) + s * a.stream_stride;
  T* voiced = a.voiced ? static_cast<T*>(a.voiced) + s * a.voiced_stride : nullptr;
  int log2L = 0;
  while ((1 << log2L) < L) ++log2L;
  for (int j = threadIdx.x; j < (L >> 1); j += blockDim.x)
    sincospi(-2.0 * (double)j / (double)L, &tws[j], &twc[j]);
  for (int j = threadIdx.x; j < kSimpleNoiseCols * nb; j += blockDim.x) noise[j] = st[j];
  SimpleState reg{};
  if (threadIdx.x == 0) simple_state_load(reg, st, nb);
  int n_voiced = 0;
  __syncthreads();
  const int rounds = (K + waves - 1) / waves;
  for (int r = 0; r <= rounds; ++r) {
    const int k = r * waves + wave;
    if (r < rounds && k < K) {
      double* o = rows + ((r & 1) * waves + wave) * kFeatRow;
      simple_wave_features(frames + k * a.block_stride, a.frame_len, L, log2L, a.pad, a.band_bins, 4, 1, twc, tws,
                           re, im, lane, o);
      if (a.features_out && lane == 0) {
        double* fo = a.features_out + ((int64_t)k * a.n_streams + s) * 7;
#pragma unroll
        for (int i = 0; i < 7; ++i) fo[i] = o[i];
      }
      wave_lds_sync();  // the next round overwrites re / im
    }
    __syncthreads();
    // the frames of round r - 1 that were labelled active, packed in order
    const int kp = k - waves;
    if (voiced && r > 0 && kp < K) {
      const int at = slot[((r - 1) & 1) * waves + wave];
      if (at >= 0) {
        const T* x = frames + kp * a.block_stride;
        T* d = voiced + (int64_t)at * a.frame_len;
        for (int i = lane; i < a.frame_len; i += 64) d[i] = x[i];
      }
    }
    if (threadIdx.x == 0 && r < rounds) {
      for (int w = 0; w < waves && r * waves + w < K; ++w) {
        const int lab = simple_state_step(reg, noise, nb, rows + ((r & 1) * waves + w) * kFeatRow);
        a.labels[(int64_t)(r * waves + w) * a.lab_stride + s] = (uint8_t)lab;
        slot[(r & 1) * waves + w] = lab ? n_voiced++ : -1;
      }
    }
  }
  // the last pass of the loop (r == rounds) was the barrier after the last steps
  for (int j = threadIdx.x; j < kSimpleNoiseCols * nb; j += blockDim.x) st[j] = noise[j];
  if (threadIdx.x == 0) {
    simple_state_store(reg, st, nb);
    if (a.voiced_len) a.voiced_len[s] = n_voiced * a.frame_len;
  }
}

// The state steps alone: one wave per stream, lane 0 stepping the rows
// feats[(k * S + s) * 7 ...] in order, the noise rows in the state itself.
// With frames (fp32) the wave also packs the stream's active frames.
__global__ __launch_bounds__(256) void simple_stream_state_kernel(const double* __restrict__ feats, int64_t n_streams,
                                                                  int n_frames, int nb, void* state, uint8_t* labels,
                                                                  int64_t lab_stride, const float* frames,
                                                                  int64_t block_stride, int64_t stream_stride,
                                                                  int frame_len, float* voiced, int64_t voiced_stride,
                                                                  int32_t* voiced_len) {
  const int lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (s >= n_streams) return;
  double* st = reinterpret_cast<double*>(static_cast<char*>(state) + s * simple_state_bytes(nb));
  SimpleState reg{};
  if (lane == 0) simple_state_load(reg, st, nb);
  int n_voiced = 0;
  for (int k = 0; k < n_frames; ++k) {
    int lab = 0;
    if (lane == 0) {
      double f[7];
      const double* row = feats + ((int64_t)k * n_streams + s) * 7;
#pragma unroll
      for (int i = 0; i < 7; ++i) f[i] = row[i];
      lab = simple_state_step(reg, st, nb, f);
      labels[(int64_t)k * lab_stride + s] = (uint8_t)lab;
    }
    if (voiced) {
      lab = __shfl(lab, 0);
      if (lab) {
        const float* x = frames + k * block_stride + s * stream_stride;
        float* d = voiced + s * voiced_stride + (int64_t)n_voiced * frame_len;
        for (int i = lane; i < frame_len; i += 64) d[i] = x[i];
        ++n_voiced;
      }
    }
  }
  if (lane == 0) {
    simple_state_store(reg, st, nb);
    if (voiced_len) voiced_len[s] = n_voiced * frame_len;
  }
}

// load_init_inactive_frames (:120-138) for every stream, one lane each: the
// rows feats[(s * nb + i) * 7 ...] of the init frames fill the noise buffer,
// the thresholds are the plain means; status cleared, silence on.
__global__ __launch_bounds__(256) void simple_stream_init_kernel(const double* __restrict__ feats, int64_t n_streams,
                                                                 int nb, void* state) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_streams) return;
  double* st = reinterpret_cast<double*>(static_cast<char*>(state) + s * simple_state_bytes(nb));
  for (int i = 0; i < nb; ++i) {
    const double* f = feats + (s * nb + i) * 7;
    double* row = st + kSimpleNoiseCols * i;
    row[0] = f[0];
    row[1] = f[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) row[2 + j] = f[3 + j];
  }
  SimpleState reg{};
  simple_noise_means(st, nb, reg.e_th, reg.std_th, reg.b_th);
  reg.silence = 1;
  simple_state_store(reg, st, nb);
}

// Waves of a block-kernel workgroup: up to 4, as many as the LDS holds beside
// the twiddle table, and no more than there are frames.
static int stream_block_waves(int L, int nb, int n_frames) {
  int waves = kStreamBlockMaxWaves;
  while (waves > 1 && stream_block_doubles(L, waves, nb) * sizeof(double) > (size_t)kStreamBlockLds) --waves;
  return n_frames < waves ? n_frames : waves;
}

bool simple_stream_block_fits(int L) { return L >= 2 && L <= 4096 && (L & (L - 1)) == 0; }

template <typename T>
static hipError_t launch_block(const SimpleBlockArgs& a, hipStream_t st) {
  const int waves = stream_block_waves(a.L, a.nb, a.n_frames);
  const size_t smem = stream_block_doubles(a.L, waves, a.nb) * sizeof(double);
  if (smem > (size_t)kStreamBlockLds) return hipErrorInvalidValue;
  static std::atomic<unsigned long long> attr_done{0};
  hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(&simple_stream_block_kernel<T>), kStreamBlockLds,
                                attr_done);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(simple_stream_block_kernel<T>, dim3((unsigned)a.n_streams), dim3(64 * waves), smem, st, a);
  return hipGetLastError();
}

hipError_t launch_simple_stream_block(const void* frames, int in_bytes, int64_t block_stride, int64_t stream_stride,
                                      int frame_len, int L, int pad, int band_bins, int64_t n_streams, int n_frames,
                                      int nb, void* state, uint8_t* labels, int64_t lab_stride, double* features_out,
                                      void* voiced, int64_t voiced_stride, int32_t* voiced_len, hipStream_t st) {
  if (n_streams <= 0 || n_frames <= 0) return hipSuccess;
  if (!simple_stream_block_fits(L) || n_streams > 0x7fffffff) return hipErrorInvalidValue;
  SimpleBlockArgs a{frames, block_stride, stream_stride, frame_len, L,      pad,          band_bins,     n_frames,
                    nb,     n_streams,    state,         labels,    lab_stride, features_out, voiced, voiced_stride,
                    voiced_len};
  return in_bytes == 2 ? launch_block<int16_t>(a, st) : launch_block<float>(a, st);
}

hipError_t launch_simple_stream_state(const double* feats, int64_t n_streams, int n_frames, int nb, void* state,
                                      uint8_t* labels, int64_t lab_stride, const float* frames, int64_t block_stride,
                                      int64_t stream_stride, int frame_len, float* voiced, int64_t voiced_stride,
                                      int32_t* voiced_len, hipStream_t st) {
  if (n_streams <= 0 || n_frames <= 0) return hipSuccess;
  const int64_t blocks = (n_streams + 3) / 4;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(simple_stream_state_kernel, dim3((unsigned)blocks), dim3(256), 0, st, feats, n_streams, n_frames,
                     nb, state, labels, lab_stride, frames, block_stride, stream_stride, frame_len, voiced,
                     voiced_stride, voiced_len);
  return hipGetLastError();
}

hipError_t launch_simple_stream_init(const double* feats, int64_t n_streams, int nb, void* state, hipStream_t st) {
  if (n_streams <= 0) return hipSuccess;
  const int64_t blocks = (n_streams + 255) / 256;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(simple_stream_init_kernel, dim3((unsigned)blocks), dim3(256), 0, st, feats, n_streams, nb, state);
  return hipGetLastError();
}

}  // namespace vad
