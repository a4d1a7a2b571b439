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
//   simple_stream_block_sessions_kernel<T> / simple_stream_state_sessions_kernel
//       the same two bodies built a second time (VAD_SIMPLE_SESSIONS 1): per
//       stream a frame count, a restart flag the kernel consumes and the init
//       frames it still owes, so callers join, leave and stall without a host
//       step and a joining stream's load_init_inactive_frames is its first
//       noise_buf_len frames (simple_state_init_step).
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
#define VAD_SIMPLE_SESSIONS 0
#include "simple_stream_block_body.inc"
#undef VAD_SIMPLE_SESSIONS
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
#define VAD_SIMPLE_SESSIONS 0
#include "simple_stream_state_body.inc"
#undef VAD_SIMPLE_SESSIONS
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

// The sessions forms.  Per stream: frame_counts[s] frames of its column are
// taken (clamped to 0..n_frames), a nonzero restart[s] makes it fresh first
// (record zero, init_left = nb) and is stored back 0, init_left[s] init frames
// are still owed.  Label rows of init frames hold VAD_LABEL_INIT, rows past
// the count VAD_LABEL_NO_HOP; a stream with no frame and no restart writes
// nothing else but voiced_len 0.
struct SimpleSessions {
  const int32_t* frame_counts;
  uint8_t* restart;
  int32_t* init_left;
};

template <typename T>
__global__ __launch_bounds__(64 * kStreamBlockMaxWaves) void simple_stream_block_sessions_kernel(SimpleBlockArgs a,
                                                                                                  SimpleSessions ss) {
#define VAD_SIMPLE_SESSIONS 1
#include "simple_stream_block_body.inc"
#undef VAD_SIMPLE_SESSIONS
}

__global__ __launch_bounds__(256) void simple_stream_state_sessions_kernel(
    const double* __restrict__ feats, int64_t n_streams, int n_frames, int nb, void* state, uint8_t* labels,
    int64_t lab_stride, const float* frames, int64_t block_stride, int64_t stream_stride, int frame_len, float* voiced,
    int64_t voiced_stride, int32_t* voiced_len, SimpleSessions ss) {
#define VAD_SIMPLE_SESSIONS 1
#include "simple_stream_state_body.inc"
#undef VAD_SIMPLE_SESSIONS
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
static hipError_t launch_block(const SimpleBlockArgs& a, const SimpleSessions* ss, hipStream_t st) {
  const int waves = stream_block_waves(a.L, a.nb, a.n_frames);
  const size_t smem = stream_block_doubles(a.L, waves, a.nb) * sizeof(double);
  if (smem > (size_t)kStreamBlockLds) return hipErrorInvalidValue;
  static std::atomic<unsigned long long> attr_done{0}, attr_done_ss{0};
  const void* fn = ss ? reinterpret_cast<const void*>(&simple_stream_block_sessions_kernel<T>)
                      : reinterpret_cast<const void*>(&simple_stream_block_kernel<T>);
  hipError_t e = ensure_dyn_lds(fn, kStreamBlockLds, ss ? attr_done_ss : attr_done);
  if (e != hipSuccess) return e;
  if (ss)
    hipLaunchKernelGGL(simple_stream_block_sessions_kernel<T>, dim3((unsigned)a.n_streams), dim3(64 * waves), smem,
                       st, a, *ss);
  else
    hipLaunchKernelGGL(simple_stream_block_kernel<T>, dim3((unsigned)a.n_streams), dim3(64 * waves), smem, st, a);
  return hipGetLastError();
}

hipError_t launch_simple_stream_block(const void* frames, int in_bytes, int64_t block_stride, int64_t stream_stride,
                                      int frame_len, int L, int pad, int band_bins, int64_t n_streams, int n_frames,
                                      int nb, void* state, uint8_t* labels, int64_t lab_stride, double* features_out,
                                      void* voiced, int64_t voiced_stride, int32_t* voiced_len,
                                      const int32_t* frame_counts, uint8_t* restart, int32_t* init_left,
                                      hipStream_t st) {
  if (n_streams <= 0 || n_frames <= 0) return hipSuccess;
  if (!simple_stream_block_fits(L) || n_streams > 0x7fffffff) return hipErrorInvalidValue;
  SimpleBlockArgs a{frames, block_stride, stream_stride, frame_len, L,      pad,          band_bins,     n_frames,
                    nb,     n_streams,    state,         labels,    lab_stride, features_out, voiced, voiced_stride,
                    voiced_len};
  const SimpleSessions ss{frame_counts, restart, init_left};
  const SimpleSessions* p = frame_counts ? &ss : nullptr;  // all three or none (the C entries have checked)
  return in_bytes == 2 ? launch_block<int16_t>(a, p, st) : launch_block<float>(a, p, st);
}

hipError_t launch_simple_stream_state(const double* feats, int64_t n_streams, int n_frames, int nb, void* state,
                                      uint8_t* labels, int64_t lab_stride, const float* frames, int64_t block_stride,
                                      int64_t stream_stride, int frame_len, float* voiced, int64_t voiced_stride,
                                      int32_t* voiced_len, const int32_t* frame_counts, uint8_t* restart,
                                      int32_t* init_left, hipStream_t st) {
  if (n_streams <= 0 || n_frames <= 0) return hipSuccess;
  const int64_t blocks = (n_streams + 3) / 4;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  if (frame_counts)
    hipLaunchKernelGGL(simple_stream_state_sessions_kernel, dim3((unsigned)blocks), dim3(256), 0, st, feats, n_streams,
                       n_frames, nb, state, labels, lab_stride, frames, block_stride, stream_stride, frame_len, voiced,
                       voiced_stride, voiced_len, SimpleSessions{frame_counts, restart, init_left});
  else
    hipLaunchKernelGGL(simple_stream_state_kernel, dim3((unsigned)blocks), dim3(256), 0, st, feats, n_streams,
                       n_frames, nb, state, labels, lab_stride, frames, block_stride, stream_stride, frame_len, voiced,
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
