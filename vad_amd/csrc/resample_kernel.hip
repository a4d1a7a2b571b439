// Polyphase FIR sample-rate conversion (include/vad_amd.h, "Resampling"):
//   y[m] = sum_j x[j] * h[m * down - j * up + P],  x zero outside the clip,
// with h the 2P+1 taps of the plan.  Written by phase: with q = m * down + P,
// jmax = q / up and r = q % up, the taps output m meets are h[r + i * up] for
// i = 0 .. T-1 (T = ceil((2P+1) / up)), against x[jmax - i].  The plan keeps
// float32(h) as the phase table ph[r][i] = h[r + i * up] (0 past tap 2P), rows
// of Ts = T | 1 floats (an odd stride: lanes on different rows spread over the
// LDS banks).
//
// resample_dot is the ONE dot product: x and the phase row come from LDS, the
// chain is x[jmax] * ph[r][0], then fmaf for i = 1 .. T-1 in that order -- a
// function of (up, down, T) only, so every entry below gives the same bits for
// the same output, whatever the tile, clip table, input type or hop split.
// With h = [1] (up = down = 1) the chain is x * 1.0f: a copy, -0.0 included.
//
// resample_batch_kernel follows ragged_copy_kernel (batch_kernel.hip): a
// persistent grid strides over DESTINATION tiles of kTileOut outputs of the
// packed buffer; per tile the clips of its first and last element are found by
// binary search in `start`, and the clips in between are walked in order.  Per
// clip piece the input span (piece * down / up + T samples, each loaded once,
// int16 converted exactly, zero outside the clip) is staged into LDS and every
// lane computes outputs kThreads apart.  Elements of no clip are written as
// zero; every element of the tile is written once.  No atomics, no workgroup
// waits on another.
//
// resample_stream_kernel: one workgroup per stream stages the stream's history
// (Hn input samples, fp32, in device memory) followed by the K new hops as one
// window and computes the K * hop_out outputs of the block from it; the last
// Hn samples of the window are the next history.
//
// resample_stream_sessions_kernel: the stream kernel for sessions.  Per stream
// it reads hop_counts[s] (n_s = min(max(count, 0), K) hops), a restart flag
// (nonzero: the history and the emitted count become zero, the stream adopts
// rate_index[s] clamped into [0, R-1], and 0 is stored back) and the stream's
// stored rate index, which picks the phase table, T, the history length,
// hop_in, delay and c_off of one of R plans -- uniform over the workgroup.
// The table is staged per stream: the next stream of the workgroup may be at
// another rate.  Rows n_s..K-1 of `out` are not written, and a stream with no
// hop and no restart writes nothing at all.  Each output is the same
// resample_dot chain with the same q, jl, r as resample_stream_kernel.
#include <mutex>
#include <vector>

#include "vad_common.h"

#include <new>

struct vad_resample_plan {
  int up, down, P, T, Ts, delay;
  std::vector<float> table;  // [up][Ts]
  float* dev = nullptr;
  int dev_id = -1;
  std::mutex mu;
};

namespace vad {
namespace {

constexpr int kThreads = 256;
constexpr int kTileOut = VAD_RESAMPLE_TILE;
constexpr int kGrid = 2048;  // 256 CUs x 8 workgroups of 4 waves
constexpr int kSessGrid = 2048;  // workgroups of the sessions stream kernel; more streams are looped over
constexpr int kMaxRates = VAD_RESAMPLE_MAX_RATES;
constexpr int kMaxTable = VAD_RESAMPLE_MAX_TABLE;
constexpr int kMaxSpan = VAD_RESAMPLE_MAX_SPAN;

__device__ __forceinline__ float resample_dot(const float* x_hi, const float* row, int T) {
  float acc = x_hi[0] * row[0];
  for (int i = 1; i < T; ++i) acc = fmaf(x_hi[-i], row[i], acc);
  return acc;
}

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(int16_t v) { return (float)v; }

template <typename TO>
__device__ __forceinline__ TO from_f32(float v);
template <>
__device__ __forceinline__ float from_f32<float>(float v) { return v; }
// rint (ties to even), saturated; NaN -> 0
template <>
__device__ __forceinline__ int16_t from_f32<int16_t>(float v) {
  if (!(v == v)) return 0;
  const float r = rintf(v);
  return (int16_t)(r < -32768.f ? -32768.f : (r > 32767.f ? 32767.f : r));
}

struct Phase {
  const float* table;  // device [up][Ts]
  int up, down, P, T, Ts;
};

__device__ __forceinline__ void stage_table(const Phase& p, float* ph) {
  for (int i = threadIdx.x; i < p.up * p.Ts; i += kThreads) ph[i] = p.table[i];
}

struct BatchArgs {
  Phase p;
  const int64_t* src_ptrs;
  const int64_t* lens;
  const int64_t* start;
  int64_t n_clips;
  void* dst;
  int64_t total;
};

// the last clip in [lo, hi] whose start is <= b; lo - 1 when there is none
__device__ __forceinline__ int64_t locate(const int64_t* start, int64_t b, int64_t lo, int64_t hi) {
  int64_t below = lo - 1;
  while (lo <= hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (start[mid] <= b) below = mid, lo = mid + 1; else hi = mid - 1;
  }
  return below;
}

// outputs of a clip of n input samples, for n <= INT64_MAX / up (the sources
// are device allocations: far below that)
__device__ __forceinline__ int64_t n_out_of(int64_t n, int up, int down) {
  if (n <= 0 || n > INT64_MAX / up - 1) return 0;
  return (n * up + down - 1) / down;
}

template <typename TO>
__device__ __forceinline__ void zero_fill(TO* dst, int64_t lo, int64_t hi) {
  for (int64_t b = lo + threadIdx.x; b < hi; b += kThreads) dst[b] = (TO)0;
}

template <typename TI, typename TO>
__global__ __launch_bounds__(kThreads) void resample_batch_kernel(BatchArgs a) {
  extern __shared__ float lds[];
  const Phase& p = a.p;
  float* ph = lds;
  float* xs = lds + p.up * p.Ts;
  stage_table(p, ph);  // made visible by the barrier before the first dot product
  TO* dst = static_cast<TO*>(a.dst);
  for (int64_t b0 = (int64_t)blockIdx.x * kTileOut; b0 < a.total; b0 += (int64_t)gridDim.x * kTileOut) {
    const int64_t b_end = b0 + kTileOut < a.total ? b0 + kTileOut : a.total;
    const int64_t k_lo = locate(a.start, b0, 0, a.n_clips - 1);
    const int64_t k_hi = locate(a.start, b_end - 1, k_lo < 0 ? 0 : k_lo, a.n_clips - 1);
    int64_t pos = b0;  // everything of the tile below pos is written
    for (int64_t k = k_lo < 0 ? 0 : k_lo; k <= k_hi; ++k) {
      const int64_t sk = a.start[k], n = a.lens[k];
      const int64_t from = sk > pos ? sk : pos;
      if (from >= b_end) break;
      zero_fill(dst, pos, from);
      pos = from;
      if (a.src_ptrs[k] == 0) {  // another launch's clip: its slots are left as they are
        const int64_t nxt = k + 1 < a.n_clips ? a.start[k + 1] : a.total;
        if (nxt > pos) pos = nxt < b_end ? nxt : b_end;
        continue;
      }
      const int64_t n_out = n_out_of(n, p.up, p.down);
      int64_t seg_hi = sk + n_out < b_end ? sk + n_out : b_end;
      if (k + 1 < a.n_clips && a.start[k + 1] < seg_hi) seg_hi = a.start[k + 1];  // cut at the next clip's start
      if (seg_hi <= pos) continue;
      const int cnt = (int)(seg_hi - pos);
      const int64_t q0 = (pos - sk) * p.down + p.P;
      const int64_t jq = q0 / p.up;
      const int r0 = (int)(q0 - jq * p.up);
      const int64_t j_base = jq - (p.T - 1);
      const int span = ((cnt - 1) * p.down + r0) / p.up + p.T;
      const TI* src = reinterpret_cast<const TI*>(static_cast<uintptr_t>(a.src_ptrs[k]));
      __syncthreads();  // the previous piece's dot products have read xs
      for (int s = threadIdx.x; s < span; s += kThreads) {
        const int64_t j = j_base + s;
        xs[s] = j >= 0 && j < n ? to_f32(src[j]) : 0.f;
      }
      __syncthreads();
      for (int e = threadIdx.x; e < cnt; e += kThreads) {
        const int q = r0 + e * p.down;
        const int jl = q / p.up;
        const int r = q - jl * p.up;
        dst[pos + e] = from_f32<TO>(resample_dot(xs + (p.T - 1) + jl, ph + r * p.Ts, p.T));
      }
      pos = seg_hi;
    }
    zero_fill(dst, pos, b_end);
  }
}

struct StreamArgs {
  Phase p;
  const void* in;
  int64_t hop_stride, block_stride;
  int64_t n_streams;
  int n_hops, hop_in, hop_out;
  int Hn, delay, c_off;
  float* hist;       // [S][Hn]
  int32_t* emitted;  // [S], min(outputs emitted, delay)
  void* out;         // (K, S, hop_out)
};

template <typename TI, typename TO>
__global__ __launch_bounds__(kThreads) void resample_stream_kernel(StreamArgs a) {
  extern __shared__ float lds[];
  const Phase& p = a.p;
  float* ph = lds;
  float* w = lds + p.up * p.Ts;
  stage_table(p, ph);
  const TI* in = static_cast<const TI*>(a.in);
  TO* out = static_cast<TO*>(a.out);
  const int n_new = a.n_hops * a.hop_in, n_outs = a.n_hops * a.hop_out;
  for (int64_t s = blockIdx.x; s < a.n_streams; s += gridDim.x) {
    __syncthreads();  // the previous stream's window has been read
    float* hist = a.hist + s * a.Hn;
    for (int i = threadIdx.x; i < a.Hn; i += kThreads) w[i] = hist[i];
    for (int i = threadIdx.x; i < n_new; i += kThreads) {
      const int k = i / a.hop_in, o = i - k * a.hop_in;
      w[a.Hn + i] = to_f32(in[k * a.block_stride + s * a.hop_stride + o]);
    }
    const int em = a.emitted[s];
    __syncthreads();
    for (int e = threadIdx.x; e < n_outs; e += kThreads) {
      const int q = e * p.down + a.c_off;
      const int jl = q / p.up;
      const int r = q - jl * p.up;
      float v = resample_dot(w + (p.T - 1) + jl, ph + r * p.Ts, p.T);
      if (em + e < a.delay) v = 0.f;  // z[n] = 0 for n < d
      const int k = e / a.hop_out, o = e - k * a.hop_out;
      out[((int64_t)k * a.n_streams + s) * a.hop_out + o] = from_f32<TO>(v);
    }
    for (int i = threadIdx.x; i < a.Hn; i += kThreads) hist[i] = w[n_new + i];
    if (threadIdx.x == 0) a.emitted[s] = em + n_outs < a.delay ? em + n_outs : a.delay;
  }
}

struct RateArgs {
  Phase p;
  int hop_in, Hn, delay, c_off;
};

struct SessArgs {
  RateArgs r[kMaxRates];
  int n_rates;
  const void* in;
  int64_t hop_stride, block_stride;
  int64_t n_streams;
  int n_hops, hop_out;
  int Hmax;                    // the longest history of the rates: the stride of hist
  const int32_t* hop_counts;   // [S]
  uint8_t* restart;            // [S], consumed
  const int32_t* rate_index;   // [S], read under a restart flag only
  float* hist;                 // [S][Hmax], the first Hn(rate) of a row in use, the rest zero
  int32_t* emitted;            // [S], min(outputs emitted, delay)
  int32_t* rate;               // [S], the rate index the session runs at
  void* out;                   // (K, S, hop_out)
};

template <typename TI, typename TO>
__global__ __launch_bounds__(kThreads) void resample_stream_sessions_kernel(SessArgs a) {
  extern __shared__ float lds[];
  const TI* in = static_cast<const TI*>(a.in);
  TO* out = static_cast<TO*>(a.out);
  for (int64_t s = blockIdx.x; s < a.n_streams; s += gridDim.x) {
    __syncthreads();  // the previous stream's table and window have been read
    const int c = a.hop_counts[s];
    const int n = __builtin_amdgcn_readfirstlane(c < 0 ? 0 : (c > a.n_hops ? a.n_hops : c));
    const bool fresh = __builtin_amdgcn_readfirstlane((int)a.restart[s]) != 0;
    if (n == 0 && !fresh) continue;  // stalled: nothing is written, the state included
    int ri = a.rate[s];
    if (fresh) ri = a.rate_index[s];
    ri = __builtin_amdgcn_readfirstlane(ri < 0 ? 0 : (ri >= a.n_rates ? a.n_rates - 1 : ri));
    const RateArgs& ra = a.r[ri];
    const Phase& p = ra.p;
    float* ph = lds;
    float* w = lds + p.up * p.Ts;
    stage_table(p, ph);
    const int n_new = n * ra.hop_in, n_outs = n * a.hop_out;
    float* hist = a.hist + s * a.Hmax;
    for (int i = threadIdx.x; i < ra.Hn; i += kThreads) w[i] = fresh ? 0.f : hist[i];
    for (int i = threadIdx.x; i < n_new; i += kThreads) {
      const int k = i / ra.hop_in, o = i - k * ra.hop_in;
      w[ra.Hn + i] = to_f32(in[k * a.block_stride + s * a.hop_stride + o]);
    }
    const int em = fresh ? 0 : a.emitted[s];
    __syncthreads();  // every read of the flag and the state lies before it, every write after it
    for (int e = threadIdx.x; e < n_outs; e += kThreads) {
      const int q = e * p.down + ra.c_off;
      const int jl = q / p.up;
      const int r = q - jl * p.up;
      float v = resample_dot(w + (p.T - 1) + jl, ph + r * p.Ts, p.T);
      if (em + e < ra.delay) v = 0.f;  // z[n] = 0 for n < d, per session
      const int k = e / a.hop_out, o = e - k * a.hop_out;
      out[((int64_t)k * a.n_streams + s) * a.hop_out + o] = from_f32<TO>(v);
    }
    for (int i = threadIdx.x; i < ra.Hn; i += kThreads) hist[i] = w[n_new + i];
    if (fresh)  // what a longer history of the last session left behind
      for (int i = ra.Hn + threadIdx.x; i < a.Hmax; i += kThreads) hist[i] = 0.f;
    if (threadIdx.x == 0) {
      a.emitted[s] = em + n_outs < ra.delay ? em + n_outs : ra.delay;
      if (fresh) a.rate[s] = ri, a.restart[s] = 0;
    }
  }
}

int gcd_i(int a, int b) {
  while (b) { const int t = a % b; a = b; b = t; }
  return a;
}

// the device copy of the phase table, made on first use on the current device
int plan_upload(vad_resample_plan* p) {
  std::lock_guard<std::mutex> lock(p->mu);
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  if (p->dev) return p->dev_id == dev ? VAD_OK : VAD_EINVAL;  // a plan serves one device
  float* d = nullptr;
  e = hipMalloc((void**)&d, p->table.size() * sizeof(float));
  if (e != hipSuccess) return e == hipErrorOutOfMemory ? VAD_ENOMEM : (int)e;
  e = hipMemcpy(d, p->table.data(), p->table.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return (int)e;
  }
  p->dev = d, p->dev_id = dev;
  return VAD_OK;
}

Phase phase_of(const vad_resample_plan* p) { return Phase{p->dev, p->up, p->down, p->P, p->T, p->Ts}; }

// input samples a tile of kTileOut outputs can need
int tile_span(int up, int down, int T) { return (int)(((int64_t)(kTileOut - 1) * down + up - 1) / up) + T; }

template <typename TI, typename TO>
int batch_entry(vad_resample_plan* p, const int64_t* src_ptrs, const int64_t* lens_in, const int64_t* start,
                int64_t n_clips, void* dst, int64_t total, void* stream) {
  if (!p || n_clips < 0 || total < 0 || total > INT64_MAX / 8) return VAD_EINVAL;
  if (n_clips > 0 && (!src_ptrs || !lens_in || !start)) return VAD_EINVAL;
  if (total > 0 && (!dst || reinterpret_cast<uintptr_t>(dst) % 16)) return VAD_EINVAL;
  if (total == 0) return VAD_OK;
  const int rc = plan_upload(p);
  if (rc != VAD_OK) return rc;
  BatchArgs a{phase_of(p), src_ptrs, lens_in, start, n_clips, dst, total};
  const int lds = (p->up * p->Ts + tile_span(p->up, p->down, p->T)) * (int)sizeof(float);
  static std::atomic<unsigned long long> done{0};
  const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(&resample_batch_kernel<TI, TO>),
                                      (kMaxTable + kMaxSpan) * (int)sizeof(float), done);
  if (e != hipSuccess) return (int)e;
  const int64_t tiles = (total + kTileOut - 1) / kTileOut;
  resample_batch_kernel<TI, TO><<<dim3((unsigned)(tiles < kGrid ? tiles : kGrid)), dim3(kThreads), lds,
                                  static_cast<hipStream_t>(stream)>>>(a);
  return (int)hipGetLastError();
}

// history samples per stream: ceil((d * down - P) / up) + T - 1
int history_len(const vad_resample_plan* p) {
  return (p->delay * p->down - p->P + p->up - 1) / p->up + p->T - 1;
}

template <typename TI, typename TO>
int stream_entry(vad_resample_plan* p, const void* in, int64_t hop_stride, int64_t block_stride, int64_t n_streams,
                 int32_t n_hops, int32_t hop_out, void* state, void* out, void* stream) {
  if (!p || n_streams < 0 || n_hops < 0 || hop_out <= 0 || n_streams > INT32_MAX) return VAD_EINVAL;
  if ((int64_t)hop_out * p->down % p->up) return VAD_EINVAL;  // a hop is a whole number of input samples
  const int64_t hop_in = (int64_t)hop_out * p->down / p->up;
  const int Hn = history_len(p);
  if (hop_in <= 0 || (int64_t)n_hops * hop_in + Hn > kMaxSpan || (int64_t)n_hops * hop_out > INT32_MAX / p->down - 1)
    return VAD_EINVAL;
  if (hop_stride < hop_in) return VAD_EINVAL;
  if (n_hops > 1 && !(block_stride > 0 &&
                      (block_stride >= (n_streams - 1) * hop_stride + hop_in ||
                       (block_stride >= hop_in && hop_stride >= (n_hops - 1) * block_stride + hop_in))))
    return VAD_EINVAL;  // the hop-major or stream-major blocks of vad_stream_hops
  if (n_streams == 0 || n_hops == 0) return VAD_OK;
  if (!in || !state || !out) return VAD_EINVAL;
  if (reinterpret_cast<uintptr_t>(in) % sizeof(TI) || reinterpret_cast<uintptr_t>(out) % sizeof(TO) ||
      reinterpret_cast<uintptr_t>(state) % 4)
    return VAD_EINVAL;
  const size_t in_elems = (size_t)((n_hops - 1) * (n_hops > 1 ? block_stride : 0) + (n_streams - 1) * hop_stride + hop_in);
  const size_t out_bytes = (size_t)n_hops * n_streams * hop_out * sizeof(TO);
  const size_t state_bytes = (size_t)n_streams * (Hn + 1) * 4;
  if (overlap(in, in_elems * sizeof(TI), out, out_bytes) || overlap(state, state_bytes, out, out_bytes) ||
      overlap(state, state_bytes, in, in_elems * sizeof(TI)))
    return VAD_EINVAL;
  const int rc = plan_upload(p);
  if (rc != VAD_OK) return rc;
  StreamArgs a{};
  a.p = phase_of(p);
  a.in = in, a.hop_stride = hop_stride, a.block_stride = n_hops > 1 ? block_stride : 0, a.n_streams = n_streams;
  a.n_hops = n_hops, a.hop_in = (int)hop_in, a.hop_out = hop_out;
  const int c0 = p->delay * p->down - p->P, Hc = (c0 + p->up - 1) / p->up;
  a.Hn = Hn, a.delay = p->delay, a.c_off = Hc * p->up - c0;
  a.hist = static_cast<float*>(state);
  a.emitted = reinterpret_cast<int32_t*>(a.hist + n_streams * Hn);
  a.out = out;
  const int lds = (p->up * p->Ts + Hn + n_hops * (int)hop_in) * (int)sizeof(float);
  static std::atomic<unsigned long long> done{0};
  const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(&resample_stream_kernel<TI, TO>),
                                      (kMaxTable + kMaxSpan) * (int)sizeof(float), done);
  if (e != hipSuccess) return (int)e;
  resample_stream_kernel<TI, TO><<<dim3((unsigned)(n_streams < 65536 ? n_streams : 65536)), dim3(kThreads), lds,
                                   static_cast<hipStream_t>(stream)>>>(a);
  return (int)hipGetLastError();
}

// hop_in, history, delay and c_off of a plan for hops of hop_out outputs; false when a hop is no whole
// number of input samples or K hops and the history pass the LDS window
bool rate_args(const vad_resample_plan* p, int32_t n_hops, int32_t hop_out, RateArgs* r) {
  if ((int64_t)hop_out * p->down % p->up) return false;
  const int64_t hop_in = (int64_t)hop_out * p->down / p->up;
  const int Hn = history_len(p);
  if (hop_in <= 0 || (int64_t)n_hops * hop_in + Hn > kMaxSpan || (int64_t)n_hops * hop_out > INT32_MAX / p->down - 1)
    return false;
  const int c0 = p->delay * p->down - p->P, Hc = (c0 + p->up - 1) / p->up;
  r->hop_in = (int)hop_in, r->Hn = Hn, r->delay = p->delay, r->c_off = Hc * p->up - c0;
  return true;
}

template <typename TI, typename TO>
int sessions_entry(vad_resample_plan* const* plans, int32_t n_rates, const void* in, int64_t hop_stride,
                   int64_t block_stride, int64_t n_streams, int32_t n_hops, int32_t hop_out, const int32_t* hop_counts,
                   uint8_t* restart, const int32_t* rate_index, void* state, void* out, void* stream) {
  if (!plans || n_rates < 1 || n_rates > kMaxRates) return VAD_EINVAL;
  if (n_streams < 0 || n_hops < 0 || hop_out <= 0 || n_streams > INT32_MAX) return VAD_EINVAL;
  SessArgs a{};
  int64_t hop_in = 0;  // the widest of the rates: the width of an input row
  int lds = 0;
  for (int i = 0; i < n_rates; ++i) {
    const vad_resample_plan* p = plans[i];
    if (!p || !rate_args(p, n_hops, hop_out, &a.r[i])) return VAD_EINVAL;
    hop_in = a.r[i].hop_in > hop_in ? a.r[i].hop_in : hop_in;
    a.Hmax = a.r[i].Hn > a.Hmax ? a.r[i].Hn : a.Hmax;
    const int need = p->up * p->Ts + a.r[i].Hn + n_hops * a.r[i].hop_in;
    lds = need > lds ? need : lds;
  }
  if (hop_stride < hop_in) return VAD_EINVAL;
  if (n_hops > 1 && !(block_stride > 0 &&
                      (block_stride >= (n_streams - 1) * hop_stride + hop_in ||
                       (block_stride >= hop_in && hop_stride >= (n_hops - 1) * block_stride + hop_in))))
    return VAD_EINVAL;  // the hop-major or stream-major blocks of vad_stream_hops
  if (n_streams == 0 || n_hops == 0) return VAD_OK;
  if (!in || !state || !out || !hop_counts || !restart || !rate_index) return VAD_EINVAL;
  if (reinterpret_cast<uintptr_t>(in) % sizeof(TI) || reinterpret_cast<uintptr_t>(out) % sizeof(TO) ||
      reinterpret_cast<uintptr_t>(state) % 4 || reinterpret_cast<uintptr_t>(hop_counts) % 4 ||
      reinterpret_cast<uintptr_t>(rate_index) % 4)
    return VAD_EINVAL;
  const size_t in_elems = (size_t)((n_hops - 1) * (n_hops > 1 ? block_stride : 0) + (n_streams - 1) * hop_stride + hop_in);
  const void* ptrs[6] = {in, out, state, hop_counts, restart, rate_index};
  const size_t bytes[6] = {in_elems * sizeof(TI), (size_t)n_hops * n_streams * hop_out * sizeof(TO),
                           (size_t)n_streams * (a.Hmax + 2) * 4, (size_t)n_streams * 4, (size_t)n_streams,
                           (size_t)n_streams * 4};
  for (int i = 0; i < 6; ++i)
    for (int j = i + 1; j < 6; ++j)
      if (overlap(ptrs[i], bytes[i], ptrs[j], bytes[j])) return VAD_EINVAL;
  for (int i = 0; i < n_rates; ++i) {
    const int rc = plan_upload(plans[i]);
    if (rc != VAD_OK) return rc;
    a.r[i].p = phase_of(plans[i]);
  }
  a.n_rates = n_rates;
  a.in = in, a.hop_stride = hop_stride, a.block_stride = n_hops > 1 ? block_stride : 0, a.n_streams = n_streams;
  a.n_hops = n_hops, a.hop_out = hop_out;
  a.hop_counts = hop_counts, a.restart = restart, a.rate_index = rate_index;
  a.hist = static_cast<float*>(state);
  a.emitted = reinterpret_cast<int32_t*>(a.hist + n_streams * a.Hmax);
  a.rate = a.emitted + n_streams;
  a.out = out;
  static std::atomic<unsigned long long> done{0};
  const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(&resample_stream_sessions_kernel<TI, TO>),
                                      (kMaxTable + kMaxSpan) * (int)sizeof(float), done);
  if (e != hipSuccess) return (int)e;
  resample_stream_sessions_kernel<TI, TO><<<dim3((unsigned)(n_streams < kSessGrid ? n_streams : kSessGrid)),
                                            dim3(kThreads), lds * (int)sizeof(float),
                                            static_cast<hipStream_t>(stream)>>>(a);
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace vad

using namespace vad;

extern "C" {

int32_t vad_resample_tile_outputs(void) { return kTileOut; }

int vad_resample_plan_create(int32_t up, int32_t down, const float* taps, int32_t n_taps, vad_resample_plan** out) {
  if (!out) return VAD_EINVAL;
  *out = nullptr;
  if (!taps || up <= 0 || down <= 0 || gcd_i(up, down) != 1) return VAD_EINVAL;
  const int64_t mx = up > down ? up : down;
  const int64_t P = mx == 1 ? 0 : 10 * mx;
  if (n_taps != 2 * P + 1) return VAD_EINVAL;
  const int64_t T = (2 * P + up) / up, Ts = T | 1;
  if (up * Ts > kMaxTable) return VAD_EINVAL;  // the phase table's share of LDS
  if (((int64_t)(kTileOut - 1) * down + up - 1) / up + T > kMaxSpan) return VAD_EINVAL;  // the input tile's
  vad_resample_plan* p = new (std::nothrow) vad_resample_plan();
  if (!p) return VAD_ENOMEM;
  p->up = up, p->down = down, p->P = (int)P, p->T = (int)T, p->Ts = (int)Ts;
  p->delay = (int)((P + down - 1) / down);
  p->table.assign((size_t)(up * Ts), 0.f);
  for (int64_t t = 0; t < n_taps; ++t) p->table[(size_t)((t % up) * Ts + t / up)] = taps[t];
  *out = p;
  return VAD_OK;
}

int vad_resample_plan_upload(vad_resample_plan* p) { return p ? plan_upload(p) : VAD_EINVAL; }

int vad_resample_plan_destroy(vad_resample_plan* p) {
  if (!p) return VAD_EINVAL;
  if (p->dev) (void)hipFree(p->dev);
  delete p;
  return VAD_OK;
}

int64_t vad_resample_n_out(const vad_resample_plan* p, int64_t n_in) {
  if (!p || n_in < 0 || n_in > INT64_MAX / p->up - 1) return -1;
  return (n_in * p->up + p->down - 1) / p->down;
}

int32_t vad_resample_delay(const vad_resample_plan* p) { return p ? p->delay : -1; }

size_t vad_resample_stream_state_bytes(const vad_resample_plan* p, int64_t n_streams) {
  if (!p || n_streams <= 0 || n_streams > INT32_MAX) return 0;
  return (size_t)n_streams * (size_t)(history_len(p) + 1) * 4;
}

int32_t vad_resample_sessions_grid(void) { return kSessGrid; }

size_t vad_resample_sessions_state_bytes(vad_resample_plan* const* plans, int32_t n_rates, int64_t n_streams) {
  if (!plans || n_rates < 1 || n_rates > kMaxRates || n_streams <= 0 || n_streams > INT32_MAX) return 0;
  int Hmax = 0;
  for (int i = 0; i < n_rates; ++i) {
    if (!plans[i]) return 0;
    const int Hn = history_len(plans[i]);
    Hmax = Hn > Hmax ? Hn : Hmax;
  }
  return (size_t)n_streams * (size_t)(Hmax + 2) * 4;
}

#define VAD_RESAMPLE_ENTRIES(IN, TI, OUT, TO)                                                                        \
  int vad_resample_batch_##IN##_##OUT(vad_resample_plan* p, const int64_t* src_ptrs, const int64_t* lens_in,        \
                                      const int64_t* start, int64_t n_clips, TO* dst, int64_t total, void* stream) { \
    return batch_entry<TI, TO>(p, src_ptrs, lens_in, start, n_clips, dst, total, stream);                            \
  }                                                                                                                  \
  int vad_resample_stream_##IN##_##OUT(vad_resample_plan* p, const TI* in, int64_t hop_stride, int64_t block_stride, \
                                       int64_t n_streams, int32_t n_hops, int32_t hop_out, void* state, TO* out,     \
                                       void* stream) {                                                               \
    return stream_entry<TI, TO>(p, in, hop_stride, block_stride, n_streams, n_hops, hop_out, state, out, stream);    \
  }                                                                                                                  \
  int vad_resample_stream_sessions_##IN##_##OUT(vad_resample_plan* const* plans, int32_t n_rates, const TI* in,      \
                                                int64_t hop_stride, int64_t block_stride, int64_t n_streams,         \
                                                int32_t n_hops, int32_t hop_out, const int32_t* hop_counts,          \
                                                uint8_t* restart, const int32_t* rate_index, void* state, TO* out,   \
                                                void* stream) {                                                      \
    return sessions_entry<TI, TO>(plans, n_rates, in, hop_stride, block_stride, n_streams, n_hops, hop_out,          \
                                  hop_counts, restart, rate_index, state, out, stream);                              \
  }

VAD_RESAMPLE_ENTRIES(f32, float, f32, float)
VAD_RESAMPLE_ENTRIES(f32, float, i16, int16_t)
VAD_RESAMPLE_ENTRIES(i16, int16_t, f32, float)
VAD_RESAMPLE_ENTRIES(i16, int16_t, i16, int16_t)

}  // extern "C"
