// FFN training on the device (reference learning/ffn_trainer.py:118-154):
// mini-batch Adadelta on softmax cross-entropy, one workgroup per model.
//
// ffn_train_kernel keeps one model's whole state -- parameters and the two
// Adadelta accumulators, 3 x count floats -- in LDS for n_steps consecutive
// steps; HBM is touched for the gathered batch rows only.  Workgroups are
// independent (no atomics, no waiting on another workgroup), so a grid of
// models trains in the time of one as long as every model has a CU.
//
// LDS layout of a workgroup, in floats (train_layout):
//   [params | E[g^2] | E[dx^2]]   3 x count, the global layout unchanged
//   A_0 (x2)  A_1 .. A_{L-1}      A_l = input rows of layer l, [bp][pad16(in_l) + 2]
//   G_0 .. G_{L-1}                G_l = dLoss/d(pre-activation of layer l), [bp][pad16(out_l) + 2]
//   labels (x2)                   [64] int
// bp = batch rounded up to 16.  Rows past the batch and columns past a
// layer's width are zero, so every GEMM runs whole 16x16x4 MFMA tiles; the
// weights stay compact and their out-of-range fragment lanes read as 0.
// A row stride of pad16 + 2 (2 x odd) puts the 32 lanes of a ds_read_b32
// group, 16 rows x 2 k, on 32 distinct banks for the A operands of the
// forward and dA GEMMs.  The dW GEMM reads the same buffers down the rows and
// the compact weights are read at their own stride; both take bank conflicts
// (DESIGN.md 4.9).
//
// One step: forward (L phases), softmax / loss / output gradient (wave 0,
// one lane per row), dA back through the layers (L - 1 phases), then one
// phase of every layer's dW tiles and bias sums, each applying Adadelta to
// its parameters straight from the MFMA accumulators.  All GEMMs are
// v_mfma_f32_16x16x4_f32: a k-ordered f32 fma chain, so together with the
// fixed task -> wave map and the shuffle-tree loss sum a run is
// bit-reproducible and independent of the grid.  Step k + 1's rows and
// labels are fetched into registers while step k computes (row indices one
// step further ahead, so no load waits on another).
//
// Byte budget: 4 x total floats of the layout above <= 160 KiB
// (VAD_EUNSUPPORTED otherwise).  39-64-32-16-3 at batch 64: 62,628 (state)
// + 90,624 (buffers) + 512; 13-64-64-2 at batch 64: 62,232 + 80,896 + 512.
#include <string.h>

#include "vad_common.h"

namespace vad {

constexpr int kTrainThreads = 512;
constexpr int kTrainWaves = kTrainThreads / 64;
constexpr int kTrainLdsBytes = 160 * 1024;
constexpr int kEvalChunkRows = VAD_TRAIN_EVAL_CHUNK_ROWS;

struct TrainDev {
  int n_layers;
  int dims[VAD_MAX_FFN_LAYERS + 1];
  int woff[VAD_MAX_FFN_LAYERS], boff[VAD_MAX_FFN_LAYERS];  // floats into a section
  int count;                                               // parameters of one model
  int bp;                                                  // batch rows rounded up to 16
  int a_off[VAD_MAX_FFN_LAYERS], a_stride[VAD_MAX_FFN_LAYERS];
  int g_off[VAD_MAX_FFN_LAYERS], g_stride[VAD_MAX_FFN_LAYERS];
  int lab_off;
  int total;  // floats of LDS
};

static int pad16(int n) { return (n + 15) & ~15; }

// train: 3 sections, two A_0 buffers, every G_l; eval: parameters only, one
// A_0, the logits buffer G_{L-1}.  Returns the bytes of LDS.
static int64_t train_layout(int n_layers, const int32_t* dims, int batch, bool train, TrainDev& t) {
  memset(&t, 0, sizeof(t));
  t.n_layers = n_layers;
  for (int l = 0; l <= n_layers; ++l) t.dims[l] = dims[l];
  int c = 0;
  for (int l = 0; l < n_layers; ++l) {
    t.woff[l] = c;
    c += dims[l] * dims[l + 1];
    t.boff[l] = c;
    c += dims[l + 1];
  }
  t.count = c;
  t.bp = pad16(batch);
  int off = ((train ? 3 : 1) * c + 3) & ~3;
  for (int l = 0; l < n_layers; ++l) {
    t.a_stride[l] = pad16(dims[l]) + 2;
    t.a_off[l] = off;
    off += t.bp * t.a_stride[l] * (l == 0 && train ? 2 : 1);
  }
  for (int l = 0; l < n_layers; ++l) {
    if (!train && l + 1 < n_layers) continue;
    t.g_stride[l] = pad16(dims[l + 1]) + 2;
    t.g_off[l] = off;
    off += t.bp * t.g_stride[l];
  }
  t.lab_off = off;
  off += 2 * 64;
  t.total = off;
  return (int64_t)off * 4;
}

// Z = A W + b over the 16 x 16 tiles of [bp][pad16(out)], tile -> wave by
// index; ReLU (NaN-keeping) unless `last`.  Columns past `out` are written 0.
__device__ __forceinline__ void dense_forward(const TrainDev& t, const float* P, int l, const float* A, int sa,
                                              float* D, int sd, bool last, int wave, int lane) {
  const int in = t.dims[l], out = t.dims[l + 1];
  const float* W = P + t.woff[l];
  const float* b = P + t.boff[l];
  const int nt_n = (out + 15) >> 4, n_tiles = (t.bp >> 4) * nt_n, ks_n = (in + 3) >> 2;
  const int r16 = lane & 15, q = lane >> 4;
  for (int task = wave; task < n_tiles; task += kTrainWaves) {
    const int mt = task / nt_n, nt = task - mt * nt_n;
    const int col = nt * 16 + r16;
    const bool cok = col < out;
    const float bias = cok ? b[col] : 0.f;
    f32x4 acc = {bias, bias, bias, bias};
    const float* ap = A + (mt * 16 + r16) * sa + q;
    const float* wp = W + q * out + col;
    for (int ks = 0; ks < ks_n; ++ks) {
      const float a = ap[ks * 4];
      const float w = (cok && ks * 4 + q < in) ? wp[ks * 4 * out] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w, acc, 0, 0, 0);
    }
    float* dp = D + (mt * 16 + q * 4) * sd + col;
#pragma unroll
    for (int r = 0; r < 4; ++r) dp[r * sd] = cok ? (last ? acc[r] : relu_nan(acc[r])) : 0.f;
  }
}

// G_{l-1} = (G_l W_l^T) masked by A_l > 0, over the tiles of [bp][pad16(in)].
__device__ __forceinline__ void dense_backward(const TrainDev& t, const float* P, int l, const float* G, int sg,
                                               const float* A, int sa, float* D, int sd, int wave, int lane) {
  const int in = t.dims[l], out = t.dims[l + 1];
  const float* W = P + t.woff[l];
  const int nt_n = (in + 15) >> 4, n_tiles = (t.bp >> 4) * nt_n, ks_n = (out + 3) >> 2;
  const int r16 = lane & 15, q = lane >> 4;
  for (int task = wave; task < n_tiles; task += kTrainWaves) {
    const int mt = task / nt_n, nt = task - mt * nt_n;
    const int col = nt * 16 + r16;
    const bool cok = col < in;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float* gp = G + (mt * 16 + r16) * sg + q;
    const float* wp = W + col * out + q;
    for (int ks = 0; ks < ks_n; ++ks) {
      const float g = gp[ks * 4];
      const float w = (cok && ks * 4 + q < out) ? wp[ks * 4] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(g, w, acc, 0, 0, 0);
    }
    const int row = mt * 16 + q * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) D[(row + r) * sd + col] = (cok && A[(row + r) * sa + col] > 0.f) ? acc[r] : 0.f;
  }
}

// Keras 1 / torch.optim.Adadelta on parameter idx of the LDS state S.
__device__ __forceinline__ void adadelta(float* S, int count, int idx, float g, float lr, float rho, float eps) {
  float a = S[count + idx], d = S[2 * count + idx];
  a = rho * a + (1.f - rho) * (g * g);
  const float u = sqrtf(d + eps) / sqrtf(a + eps) * g;
  d = rho * d + (1.f - rho) * (u * u);
  S[idx] -= lr * u;
  S[count + idx] = a;
  S[2 * count + idx] = d;
}

// Every layer's dW = A_l^T G_l tiles (K = the batch rows) and bias sums, each
// followed by the Adadelta update of its parameters.
__device__ __forceinline__ void update_phase(const TrainDev& t, float* S, const float* lds, int buf, int batch,
                                             float lr, float rho, float eps, int wave, int lane) {
  const int r16 = lane & 15, q = lane >> 4, ks_n = t.bp >> 2;
  int total = 0;
  for (int l = 0; l < t.n_layers; ++l) total += ((t.dims[l] + 15) >> 4) * ((t.dims[l + 1] + 15) >> 4) + 1;
  for (int task = wave; task < total; task += kTrainWaves) {
    int l = 0, loc = task, n_tiles = 0, nt_n = 0;
    for (;; ++l) {
      nt_n = (t.dims[l + 1] + 15) >> 4;
      n_tiles = ((t.dims[l] + 15) >> 4) * nt_n;
      if (loc <= n_tiles) break;
      loc -= n_tiles + 1;
    }
    const int in = t.dims[l], out = t.dims[l + 1];
    const int sa = t.a_stride[l], sg = t.g_stride[l];
    const float* A = lds + t.a_off[l] + (l == 0 ? buf * t.bp * sa : 0);
    const float* G = lds + t.g_off[l];
    if (loc == n_tiles) {  // bias: column sums in row order
      if (lane < out) {
        float s = 0.f;
        for (int r = 0; r < batch; ++r) s += G[r * sg + lane];
        adadelta(S, t.count, t.boff[l] + lane, s, lr, rho, eps);
      }
      continue;
    }
    const int mt = loc / nt_n, nt = loc - mt * nt_n;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float* ap = A + q * sa + mt * 16 + r16;
    const float* gp = G + q * sg + nt * 16 + r16;
    for (int ks = 0; ks < ks_n; ++ks)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[ks * 4 * sa], gp[ks * 4 * sg], acc, 0, 0, 0);
    const int i0 = mt * 16 + q * 4, j = nt * 16 + r16;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (i0 + r < in && j < out) adadelta(S, t.count, t.woff[l] + (i0 + r) * out + j, acc[r], lr, rho, eps);
  }
}

// Max-subtracted softmax of one row's logits z[0..C): p[c] (0 past C), the
// loss -log p[label] as logsumexp - z[label], and the first-max argmax
// (np.argmax: a NaN counts as the maximum).  The label is only compared.
__device__ __forceinline__ void row_softmax(const float* z, int C, int lab, float p[4], float& loss, int& arg) {
  float v[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] = c < C ? z[c] : -INFINITY;
  float m = v[0], best = v[0];
  arg = 0;
#pragma unroll
  for (int c = 1; c < 4; ++c) {
    m = fmaxf(m, v[c]);
    if (c < C && (v[c] > best || (v[c] != v[c] && best == best))) {
      best = v[c];
      arg = c;
    }
  }
  float s = 0.f, zl = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    p[c] = c < C ? expf(v[c] - m) : 0.f;
    s += p[c];
    zl = (c < C && lab == c) ? v[c] : zl;
  }
  const float inv = 1.f / s;
#pragma unroll
  for (int c = 0; c < 4; ++c) p[c] *= inv;
  loss = (m + logf(s)) - zl;
}

// fixed-order sum over the 64 lanes of a wave
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ __launch_bounds__(kTrainThreads) void ffn_train_kernel(
    TrainDev t, float* __restrict__ state, const float* __restrict__ x, const uint8_t* __restrict__ y,
    const int32_t* __restrict__ order, int64_t order_stride, int batch, int64_t n_steps,
    const float* __restrict__ hyper, float* __restrict__ step_loss) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t m = blockIdx.x;
  float* gstate = state + m * 3 * (int64_t)t.count;
  const int32_t* ord = order + m * order_stride;
  const float lr = hyper[m * 3], rho = hyper[m * 3 + 1], eps = hyper[m * 3 + 2];
  const int L = t.n_layers, in0 = t.dims[0], C = t.dims[L];
  const int sa0 = t.a_stride[0];
  int* labs = reinterpret_cast<int*>(lds + t.lab_off);

  for (int i = tid; i < 3 * t.count; i += kTrainThreads) lds[i] = gstate[i];

  // batch fetch: thread -> rows rr, rr + 32, columns c16 + 16 j
  const int c16 = tid & 15, rr = tid >> 4;
  float xv[2][4];
  int lab[2] = {0, 0};
  int64_t idx[2], idx2[2];
  auto fetch_idx = [&](int64_t step, int64_t out[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = rr + 32 * i;
      out[i] = (step < n_steps && r < batch) ? (int64_t)ord[step * batch + r] : 0;
    }
  };
  auto fetch_rows = [&](bool live) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const bool rok = live && rr + 32 * i < batch;
#pragma unroll
      for (int j = 0; j < 4; ++j) xv[i][j] = (rok && c16 + 16 * j < in0) ? x[idx[i] * in0 + c16 + 16 * j] : 0.f;
      lab[i] = (rok && c16 == 0) ? (int)y[idx[i]] : 0;
    }
  };
  auto store_rows = [&](int buf) {
    float* A0 = lds + t.a_off[0] + buf * t.bp * sa0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = rr + 32 * i;
      if (r < t.bp) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (16 * j < sa0 - 2) A0[r * sa0 + c16 + 16 * j] = xv[i][j];
      }
      if (c16 == 0) labs[buf * 64 + r] = lab[i];
    }
  };
  fetch_idx(0, idx);
  fetch_rows(n_steps > 0);
  fetch_idx(1, idx2);
  store_rows(0);
  idx[0] = idx2[0];
  idx[1] = idx2[1];
  __syncthreads();

  for (int64_t k = 0; k < n_steps; ++k) {
    const int buf = (int)(k & 1);
    fetch_rows(k + 1 < n_steps);  // step k + 1's rows, used at the end of this step
    fetch_idx(k + 2, idx2);

    for (int l = 0; l < L; ++l) {
      const float* A = lds + t.a_off[l] + (l == 0 ? buf * t.bp * sa0 : 0);
      const bool last = l + 1 == L;
      float* D = last ? lds + t.g_off[l] : lds + t.a_off[l + 1];
      dense_forward(t, lds, l, A, t.a_stride[l], D, last ? t.g_stride[l] : t.a_stride[l + 1], last, wave, lane);
      __syncthreads();
    }
    if (wave == 0) {  // one lane per row: logits -> (p - onehot) / batch in place
      float loss = 0.f;
      if (lane < t.bp) {
        float* z = lds + t.g_off[L - 1] + lane * t.g_stride[L - 1];
        const bool valid = lane < batch;
        const int lb = labs[buf * 64 + lane];
        float p[4], lo;
        int arg;
        row_softmax(z, C, lb, p, lo, arg);
#pragma unroll
        for (int c = 0; c < 4; ++c) z[c] = (valid && c < C) ? (p[c] - (lb == c ? 1.f : 0.f)) / (float)batch : 0.f;
        loss = valid ? lo : 0.f;
      }
      loss = wave_sum(loss);
      if (lane == 0 && step_loss) step_loss[m * n_steps + k] = loss / (float)batch;
    }
    __syncthreads();
    for (int l = L - 1; l >= 1; --l) {
      dense_backward(t, lds, l, lds + t.g_off[l], t.g_stride[l], lds + t.a_off[l], t.a_stride[l],
                     lds + t.g_off[l - 1], t.g_stride[l - 1], wave, lane);
      __syncthreads();
    }
    update_phase(t, lds, lds, buf, batch, lr, rho, eps, wave, lane);
    store_rows(buf ^ 1);
    idx[0] = idx2[0];
    idx[1] = idx2[1];
    __syncthreads();
  }

  for (int i = tid; i < 3 * t.count; i += kTrainThreads) gstate[i] = lds[i];
}

// model.evaluate_generator (ffn_trainer.py:154): summed loss and correct
// count of one chunk of rows under one model's parameters.
__global__ __launch_bounds__(kTrainThreads) void ffn_eval_kernel(
    TrainDev t, const float* __restrict__ state, const float* __restrict__ x, const uint8_t* __restrict__ y,
    int64_t n_rows, int64_t n_chunks, float* __restrict__ loss_sums, int32_t* __restrict__ correct) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t m = blockIdx.x / n_chunks, chunk = blockIdx.x - m * n_chunks;
  const float* gstate = state + m * 3 * (int64_t)t.count;
  const int L = t.n_layers, in0 = t.dims[0], C = t.dims[L];
  const int sa0 = t.a_stride[0];
  int* labs = reinterpret_cast<int*>(lds + t.lab_off);
  float* A0 = lds + t.a_off[0];
  for (int i = tid; i < t.count; i += kTrainThreads) lds[i] = gstate[i];

  const int64_t row0 = chunk * kEvalChunkRows;
  const int64_t row1 = row0 + kEvalChunkRows < n_rows ? row0 + kEvalChunkRows : n_rows;
  const int c16 = tid & 15, rr = tid >> 4;
  float loss_acc = 0.f;
  int hit = 0;
  for (int64_t base = row0; base < row1; base += 64) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = rr + 32 * i;
      const bool rok = base + r < row1;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (16 * j < sa0 - 2)
          A0[r * sa0 + c16 + 16 * j] = (rok && c16 + 16 * j < in0) ? x[(base + r) * in0 + c16 + 16 * j] : 0.f;
      if (c16 == 0) labs[r] = rok ? (int)y[base + r] : 0;
    }
    __syncthreads();
    for (int l = 0; l < L; ++l) {
      const bool last = l + 1 == L;
      float* D = last ? lds + t.g_off[l] : lds + t.a_off[l + 1];
      dense_forward(t, lds, l, lds + t.a_off[l], t.a_stride[l], D, last ? t.g_stride[l] : t.a_stride[l + 1], last,
                    wave, lane);
      __syncthreads();
    }
    if (wave == 0 && base + lane < row1) {
      const int lb = labs[lane];
      float p[4], lo;
      int arg;
      row_softmax(lds + t.g_off[L - 1] + lane * t.g_stride[L - 1], C, lb, p, lo, arg);
      loss_acc += lo;
      hit += arg == lb ? 1 : 0;
    }
    __syncthreads();
  }
  if (wave == 0) {
    loss_acc = wave_sum(loss_acc);
    hit = wave_sum(hit);
    if (lane == 0) {
      loss_sums[m * n_chunks + chunk] = loss_acc;
      correct[m * n_chunks + chunk] = hit;
    }
  }
}

int64_t ffn_train_lds_bytes(int n_layers, const int32_t* dims, int batch, bool train) {
  TrainDev t;
  return train_layout(n_layers, dims, batch, train, t);
}

hipError_t launch_ffn_train(int n_layers, const int32_t* dims, float* state, int64_t n_models, const float* x,
                            const uint8_t* y, const int32_t* order, int64_t order_stride, int batch, int64_t n_steps,
                            const float* hyper, float* step_loss, hipStream_t st) {
  TrainDev t;
  const int64_t bytes = train_layout(n_layers, dims, batch, true, t);
  if (bytes > kTrainLdsBytes) return hipErrorInvalidValue;
  static std::atomic<unsigned long long> attr_done{0};
  const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(&ffn_train_kernel), kTrainLdsBytes, attr_done);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ffn_train_kernel, dim3((unsigned)n_models), dim3(kTrainThreads), (size_t)bytes, st, t, state, x,
                     y, order, order_stride, batch, n_steps, hyper, step_loss);
  return hipGetLastError();
}

hipError_t launch_ffn_eval(int n_layers, const int32_t* dims, const float* state, int64_t n_models, const float* x,
                           const uint8_t* y, int64_t n_rows, int64_t n_chunks, float* loss_sums, int32_t* correct,
                           hipStream_t st) {
  TrainDev t;
  const int64_t bytes = train_layout(n_layers, dims, 64, false, t);
  if (bytes > kTrainLdsBytes) return hipErrorInvalidValue;
  static std::atomic<unsigned long long> attr_done{0};
  const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(&ffn_eval_kernel), kTrainLdsBytes, attr_done);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ffn_eval_kernel, dim3((unsigned)(n_models * n_chunks)), dim3(kTrainThreads), (size_t)bytes, st,
                     t, state, x, y, n_rows, n_chunks, loss_sums, correct);
  return hipGetLastError();
}

}  // namespace vad
