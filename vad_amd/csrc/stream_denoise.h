// Live spectral noise subtraction in the hop kernels (stream_hop_ffn_body.inc
// and stream_hop_tree_body.inc under VAD_HOP_DENOISE 1), and the kernel that
// loads a stream's noise frames.  The reference computes the subtraction and
// drops it (sklearn_analyser.py:84-101,122-123); here the MFCC is taken from
// the subtracted spectrum.  DESIGN.md section 4 states the semantics.
//
// Per stream, beside frames / ring / count (all fp32 in the kernel's units
// |2X|^2, zero = fresh):
//   spec  (5, 256)  power rows of the last five frames, slot = the MFCC ring's
//   rows  (5, 256)  noise rows in arrival order, row 0 the oldest
//   held  int       rows held, 0..5
//   est   (256)     the noise estimate in force
// Every global access of this state is one 16-B load or store per lane: lane
// l owns bins 4 l .. 4 l + 3 of every row, so a lane only ever reads what it
// wrote itself (or what an earlier launch left), and no fence is needed
// between the hops of one launch.
#pragma once

#include "stream_hop.h"

namespace vad {

// (HopDenoise, the state's pointers and the options, is in vad_common.h.)

// A wave-uniform stream index as the compiler sees one (two scalar registers)
__device__ __forceinline__ int64_t dn_uniform(int64_t s) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)s);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)s >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Steps 2 and 3 of a hop: the raw power row (pw, 256 floats of the wave's
// LDS) goes to the spectrum ring, pw becomes max(p - e, 0) with NaN kept
// (np.where(sub < 0, 0, sub)).  e = 0 leaves every p as it is, bit for bit
// (p is a sum of squares: never -0).
__device__ __forceinline__ void dn_store_subtract(float* pw, int ln, float* spec_row, const float4& e) {
  float4* p4 = reinterpret_cast<float4*>(pw) + ln;
  const float4 p = *p4;
  reinterpret_cast<float4*>(spec_row)[ln] = p;
  float4 d = make_float4(p.x - e.x, p.y - e.y, p.z - e.z, p.w - e.w);
  d.x = d.x < 0.f ? 0.f : d.x;
  d.y = d.y < 0.f ? 0.f : d.y;
  d.z = d.z < 0.f ? 0.f : d.z;
  d.w = d.w < 0.f ? 0.f : d.w;
  *p4 = d;
}

// A stream starting over (the sessions kernels' restart): zeros to the lane's
// own 16 B of the eleven rows -- five of the spectrum ring, five noise rows,
// the estimate.  The lane alone reads these bytes later in the launch, so no
// fence follows.
__device__ __forceinline__ void dn_clear(float* spec, float* rows, float* est, int lane) {
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int j = 0; j < 5; ++j) reinterpret_cast<float4*>(spec + j * kBins)[lane] = z;
#pragma unroll
  for (int j = 0; j < kNoiseRows; ++j) reinterpret_cast<float4*>(rows + j * kBins)[lane] = z;
  reinterpret_cast<float4*>(est)[lane] = z;
}

// The push: the lane's four bins `nw` of a raw power row go behind the rows
// held (the oldest row dropped and the others moved down when five are
// held).  Returns the lane's bins of the mean (((r0 + r1) + r2) + ...) / n in
// arrival order; n (wave-uniform) is advanced.
__device__ __forceinline__ float4 dn_push_mean(float* rows, int& n, const float4& nw, int ln) {
  float4* r4 = reinterpret_cast<float4*>(rows) + ln;  // row j: r4[64 j]
  const bool full = n == kNoiseRows;
  const int kept = full ? kNoiseRows - 1 : n;
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int j = 0; j < kNoiseRows; ++j) {
    if (j <= kept) {
      float4 r = nw;
      if (j < kept) r = r4[64 * (full ? j + 1 : j)];
      if (full || j == kept) r4[64 * j] = r;
      sum = j == 0 ? r : make_float4(sum.x + r.x, sum.y + r.y, sum.z + r.z, sum.w + r.w);
    }
  }
  n = kept + 1;
  const float fn = (float)n;
  return make_float4(sum.x / fn, sum.y / fn, sum.z / fn, sum.w / fn);
}

// The estimate from the mean m (the lane's four bins): the first-order low
// pass over the bins with the reference's wrap at bin 0,
//   e[0] = a m[255] + (1 - a) m[0],  e[i] = a e[i-1] + (1 - a) m[i],
// evaluated as an affine scan across the wave.  Every operation below is one
// fp32 rounding (no contraction) and THIS order is the definition: the host
// model tests/stream_denoise_reference.py::estimate_f32 repeats it operation
// for operation and the kernels equal it bit for bit.
//   b[i]    = (1 - a) m[i]
//   lane l  B_l = ((b0 a + b1) a + b2) a + b3 over its bins (what the lane
//           adds to a zero carry), A_l = (a a)(a a)
//   scan    d = 1, 2, .., 32: lanes l >= d take (A, B) <- (A A', A B' + B)
//           from lane l - d's (A', B') -- Kogge-Stone, inclusive
//   carry   X_l = A_l m[255] + B_l is e[4 l + 3]; lane l starts from X_(l-1),
//           lane 0 from m[255], and runs the recurrence over its four bins
__device__ __forceinline__ float4 dn_estimate(const float4& m, float alpha, int ln) {
#pragma clang fp contract(off)
  const float beta = 1.f - alpha;
  const float b0 = beta * m.x, b1 = beta * m.y, b2 = beta * m.z, b3 = beta * m.w;
  float B = b0;
  B = alpha * B + b1;
  B = alpha * B + b2;
  B = alpha * B + b3;
  const float a2 = alpha * alpha;
  float A = a2 * a2;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float Ap = __shfl_up(A, d, 64), Bp = __shfl_up(B, d, 64);
    if (ln >= d) {
      B = A * Bp + B;
      A = A * Ap;
    }
  }
  const float x0 = __shfl(m.w, 63, 64);
  const float X = A * x0 + B;
  float cin = __shfl_up(X, 1, 64);
  if (ln == 0) cin = x0;
  float4 e;
  e.x = alpha * cin + b0;
  e.y = alpha * e.x + b1;
  e.z = alpha * e.y + b2;
  e.w = alpha * e.z + b3;
  return e;
}

// The hop kernels' power spectrum of one frame, for the load kernel: the
// statements of the hop bodies (Stockham radix-4, real split), the twiddles
// read from the plan's blob in global memory.  xs (the samples, packed as in
// the bodies) sits in z1 on entry; |2X|^2 of bins 0..255 is left in z0 as 256
// floats.  Every product and sum is spelled as in the bodies, so a frame's
// row equals the row a hop stores for it bit for bit.
__device__ __forceinline__ void dn_frame_power(float2* z0, float2* z1, const float2* __restrict__ tw, int ln) {
  float2* src = z1;
  float2* dst = z0;
#pragma unroll
  for (int st = 0; st < 4; ++st) {
    const int ns = 1 << (2 * st);
    const int kk = ln & (ns - 1);
    float2 a0 = src[zp(ln)], a1 = src[zp(ln + 64)], a2 = src[zp(ln + 128)], a3 = src[zp(ln + 192)];
    if (st > 0) {
      const int m = kk * (64 >> (2 * st));
      a1 = cmulf(a1, w256(tw, m));
      a2 = cmulf(a2, w256(tw, 2 * m));
      a3 = cmulf(a3, w256(tw, 3 * m));
    }
    const float2 b0 = make_float2(a0.x + a2.x, a0.y + a2.y), b1 = make_float2(a0.x - a2.x, a0.y - a2.y);
    const float2 b2 = make_float2(a1.x + a3.x, a1.y + a3.y), b3 = make_float2(a1.x - a3.x, a1.y - a3.y);
    const int o = (ln >> (2 * st)) * (4 * ns) + kk;
    dst[zp(o)] = make_float2(b0.x + b2.x, b0.y + b2.y);
    dst[zp(o + ns)] = make_float2(b1.x + b3.y, b1.y - b3.x);
    dst[zp(o + 2 * ns)] = make_float2(b0.x - b2.x, b0.y - b2.y);
    dst[zp(o + 3 * ns)] = make_float2(b1.x - b3.y, b1.y + b3.x);
    float2* t = src;
    src = dst;
    dst = t;
    asm volatile("" ::: "memory");
  }
  float* pw = reinterpret_cast<float*>(dst);
  float pk[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int kb = ln + 64 * q;
    const float2 zk = src[zp(kb)], zn = src[zp((256 - kb) & 255)];
    const float2 S = make_float2(zk.x + zn.x, zk.y - zn.y);
    const float2 D = make_float2(zk.x - zn.x, zk.y + zn.y);
    const float2 Tw = cmulf(D, tw[kb]);
    const float u = S.x + Tw.y, vv = S.y - Tw.x;
    pk[q] = fmaf(u, u, vv * vv);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) pw[ln + 64 * q] = pk[q];
  asm volatile("" ::: "memory");
}

}  // namespace vad
