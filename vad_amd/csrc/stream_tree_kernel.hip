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
#include "tree_walk.h"

namespace vad {

// NR, TH: as stream_hop_kernel.  lds_nodes: n_nodes when the compact table is
// staged behind the blob and walked from LDS, 0 for the walk from global.
template <int NR, class TH>
__global__ __launch_bounds__(1024) void stream_hop_tree_kernel(
    const float* __restrict__ blob, int blob_n, int nf, int n_taps, const TreeNodeC* __restrict__ cnodes,
    const TreeNode* __restrict__ nodes, int n_nodes, int lds_nodes, float* __restrict__ frames, int64_t fstride,
    int len, const TH* __restrict__ hop, int64_t hstride, int hlen, int64_t n_streams, int mfcc_n,
    float* __restrict__ ring, int* __restrict__ count, uint8_t* __restrict__ labels, int n_hops,
    int64_t hop_kstride, int64_t lab_kstride) {
  extern __shared__ __attribute__((aligned(16))) float hsm[];
  const int waves = blockDim.x >> 6;
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  // -- stage the MFCC plan's hop blob, then the compact node table (one node
  // per lane and DMA), by LDS-DMA; then request the stream's state and the
  // FFT's twiddles (registers); then the block's only barrier
  float* base = hsm + waves * kHopWaveFloats;
  {
    const float4* m4 = reinterpret_cast<const float4*>(blob);
    const float4* t4 = reinterpret_cast<const float4*>(cnodes);
    const int nm4 = blob_n >> 2, n4 = nm4 + lds_nodes;
    for (int c0 = wv * 64; c0 < n4; c0 += (int)blockDim.x) {  // wave-uniform chunk base
      const int c = c0 + lane;
      if (c < n4)
        __builtin_amdgcn_global_load_lds(c < nm4 ? (const void*)(m4 + c) : (const void*)(t4 + (c - nm4)),
                                         (__attribute__((address_space(3))) void*)(base + 4 * c0), 16, 0, 0);
    }
  }
  HopTables T;
  T.tw = reinterpret_cast<const float2*>(base);
  const int* ilo = reinterpret_cast<const int*>(base + 2 * 256);
  T.f_lo = ilo;
  T.f_len = ilo + nf;
  T.f_off = ilo + 2 * nf;
  T.taps = base + ((2 * 256 + 3 * nf + 3) & ~3);  // 16-B aligned rows of n_taps (a multiple of 4) in all
  T.dct = T.taps + n_taps;
  const int4* cn = reinterpret_cast<const int4*>(base + blob_n);  // {thr bits, feature, left, right}

  const int64_t s = (int64_t)blockIdx.x * waves + wv;
  const int64_t sc = s < n_streams ? s : 0;
  // -- the stream's state, requested before the barrier so its latency
  // overlaps the staging
  float* row = frames + sc * fstride;
  const int keep = len - hlen;
  float v[NR], hn[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int t = lane + 64 * i;
    v[i] = t < len ? row[t] : 0.f;
    hn[i] = (t >= keep && t < len) ? (float)hop[sc * hstride + (t - keep)] : 0.f;
  }
  int c = count[sc];
  float* rs = ring + sc * 5 * mfcc_n;
  float rv[5];
#pragma unroll
  for (int d = 0; d < 5; ++d) rv[d] = lane < mfcc_n ? rs[d * mfcc_n + lane] : 0.f;
  // this lane's FFT twiddles (stream_hop_kernel: registers in the 7-chunk
  // build, the staged table in the 16-chunk one)
  const float2* tw_g = reinterpret_cast<const float2*>(blob);
  constexpr bool kTwReg = NR <= 7;
  float2 twr[3][3], tws[4];
  if constexpr (kTwReg) {
#pragma unroll
    for (int st = 1; st < 4; ++st) {
      const int ns = 1 << (2 * st);
      const int m = (lane & (ns - 1)) * (64 >> (2 * st));
#pragma unroll
      for (int jj = 1; jj < 4; ++jj) twr[st - 1][jj - 1] = w256(tw_g, jj * m);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) tws[q] = tw_g[lane + 64 * q];
  }
  // the staged tables are complete: LDS-DMA writes count on vmcnt, not
  // lgkmcnt, and a workgroup-scope release fence need not drain vmcnt, so the
  // wait is explicit (vmcnt 0, before the barrier)
  __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt 0, expcnt 7, lgkmcnt 15
  __syncthreads();
  if (s >= n_streams) return;  // wave-uniform; no barrier below
  float* scr = hsm + wv * kHopWaveFloats;
  float2* z0 = reinterpret_cast<float2*>(scr);
  float2* z1 = reinterpret_cast<float2*>(scr + kHopZ);
  float* lmr = scr + 2 * kHopZ;
  float* act_a = lmr + kMaxFilters;
  float* fb = scr;  // the frame shift goes through the FFT buffers (2 kHopZ >= 1024 floats)
  const int used = len < kFftN ? len : kFftN;

  for (int k = 0; k < n_hops; ++k) {
    // the lane index, opaque per hop (stream_hop_kernel: keeps the hop's LDS
    // addresses out of registers across hops)
    int ln = lane;
    asm volatile("" : "+v"(ln));
    // -- frame: shift by the hop through LDS, append the new samples
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int t = ln + 64 * i;
      if (t < len) fb[t] = v[i];
    }
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int t = ln + 64 * i;
      v[i] = t < keep ? fb[t + hlen] : hn[i];
    }
    asm volatile("" ::: "memory");
    if (k + 1 < n_hops) {  // the next hop's samples, in flight during this one
      const TH* hs = hop + (int64_t)(k + 1) * hop_kstride + s * hstride;
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        const int t = ln + 64 * i;
        hn[i] = (t >= keep && t < len) ? (float)hs[t - keep] : 0.f;
      }
    }
    uint8_t* lab_k = labels + (int64_t)k * lab_kstride;
    // samples of the FFT (np.fft.fft(x, 512): zero-pad / truncate, mfcc.py:61)
    float* xs = reinterpret_cast<float*>(z1);
#pragma unroll
    for (int i = 0; i < 8; ++i) {  // all 512 inputs: the zero padding past the frame too
      const int t = ln + 64 * i;  // sample t = component t & 1 of complex t / 2
      xs[2 * zp(t >> 1) + (t & 1)] = (i < NR && t < used) ? v[i < NR ? i : 0] : 0.f;
    }
    asm volatile("" ::: "memory");

    // -- 256-point complex FFT, Stockham radix-4
    float2* src = z1;
    float2* dst = z0;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const int ns = 1 << (2 * st);  // 1, 4, 16, 64
      const int kk = ln & (ns - 1);
      float2 a0 = src[zp(ln)], a1 = src[zp(ln + 64)], a2 = src[zp(ln + 128)], a3 = src[zp(ln + 192)];
      if (st > 0) {  // W_{4 ns}^(j k) = W256^(64 j k / ns)
        const int m = kk * (64 >> (2 * st));
        a1 = cmulf(a1, kTwReg ? twr[st - 1][0] : w256(T.tw, m));
        a2 = cmulf(a2, kTwReg ? twr[st - 1][1] : w256(T.tw, 2 * m));
        a3 = cmulf(a3, kTwReg ? twr[st - 1][2] : w256(T.tw, 3 * m));
      }
      const float2 b0 = make_float2(a0.x + a2.x, a0.y + a2.y), b1 = make_float2(a0.x - a2.x, a0.y - a2.y);
      const float2 b2 = make_float2(a1.x + a3.x, a1.y + a3.y), b3 = make_float2(a1.x - a3.x, a1.y - a3.y);
      const int o = (ln >> (2 * st)) * (4 * ns) + kk;
      dst[zp(o)] = make_float2(b0.x + b2.x, b0.y + b2.y);
      dst[zp(o + ns)] = make_float2(b1.x + b3.y, b1.y - b3.x);      // b1 - i b3
      dst[zp(o + 2 * ns)] = make_float2(b0.x - b2.x, b0.y - b2.y);
      dst[zp(o + 3 * ns)] = make_float2(b1.x - b3.y, b1.y + b3.x);  // b1 + i b3
      float2* t = src;
      src = dst;
      dst = t;
      asm volatile("" ::: "memory");
    }
    // -- real-FFT split: 2X[k] = S - i W512^k D; |2X|^2 into the free buffer
    float* pw = reinterpret_cast<float*>(dst);
    float pk[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int kb = ln + 64 * q;
      const float2 zk = src[zp(kb)], zn = src[zp((256 - kb) & 255)];
      const float2 S = make_float2(zk.x + zn.x, zk.y - zn.y);
      const float2 D = make_float2(zk.x - zn.x, zk.y + zn.y);
      const float2 Tw = cmulf(D, kTwReg ? tws[q] : T.tw[kb]);
      const float u = S.x + Tw.y, vv = S.y - Tw.x;
      pk[q] = fmaf(u, u, vv * vv);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) pw[ln + 64 * q] = pk[q];
    asm volatile("" ::: "memory");
    // -- mel + log10 (ln m), lifter x DCT (ln c)
    if (ln < nf) {
      const int lo4 = T.f_lo[ln], n4 = T.f_len[ln];
      const float4* wt4 = reinterpret_cast<const float4*>(T.taps + T.f_off[ln]);
      const float4* pw4 = reinterpret_cast<const float4*>(pw + lo4);
      float e = 0.f;
#pragma unroll 2
      for (int t = 0; t < n4; t += 4) {
        const float4 w = wt4[t >> 2], q = pw4[t >> 2];
        e = fmaf(w.x, q.x, e);
        e = fmaf(w.y, q.y, e);
        e = fmaf(w.z, q.z, e);
        e = fmaf(w.w, q.w, e);
      }
      lmr[ln] = log10_pos(e == 0.f ? 0x1p-52f : e);  // mfcc.py:74-75
    }
    asm volatile("" ::: "memory");
    float mf = 0.f;
    if (ln < mfcc_n) {
      const float4* d4 = reinterpret_cast<const float4*>(T.dct + ln * vec_row_stride(nf));
      const float4* l4 = reinterpret_cast<const float4*>(lmr);
      int m = 0;
#pragma unroll 4
      for (; m + 4 <= nf; m += 4) {
        const float4 d = d4[m >> 2], l = l4[m >> 2];
        mf = fmaf(d.x, l.x, mf);
        mf = fmaf(d.y, l.y, mf);
        mf = fmaf(d.z, l.z, mf);
        mf = fmaf(d.w, l.w, mf);
      }
      const float* d = T.dct + ln * vec_row_stride(nf);
      for (; m < nf; ++m) mf = fmaf(d[m], lmr[m], mf);
    }
    // -- window of the five previous frames, then push the new row
    const bool have = c >= 5;
    act_a[ln] = 0.f;  // the feature row, zeroed before the store as in stream_hop_kernel
    asm volatile("" ::: "memory");
    if (ln < mfcc_n) {
      if (have) {
        // slot (c + d) % 5, d = 0..4: the ring in arrival order, oldest first
        float r[5];
#pragma unroll
        for (int d = 0; d < 5; ++d) {
          const int q = (c + d) % 5;
          r[d] = q == 0 ? rv[0] : q == 1 ? rv[1] : q == 2 ? rv[2] : q == 3 ? rv[3] : rv[4];
        }
        const Feat3 ft = feature_triple(r[0], r[1], r[2], r[3], r[4], VAD_FEAT_ANALYSER);
        act_a[ln] = ft.mn;
        act_a[mfcc_n + ln] = ft.d1;
        act_a[2 * mfcc_n + ln] = ft.d2;
      }
      const int q = c % 5;  // the push (ring slot of the oldest row)
#pragma unroll
      for (int d = 0; d < 5; ++d) rv[d] = q == d ? mf : rv[d];
    }
    asm volatile("" ::: "memory");
    // -- the tree: one path for the whole wave.  A node's feature index is
    // below the plan's n_features <= 3 mfcc_n (checked by the C entry and by
    // vad_tree_plan_create), its children inside the table; the loop is
    // bounded by n_nodes so that a malformed table cannot spin (tree_walk)
    int label = 255;
    if (have) {
      int node = 0;
      label = 0;
      if (lds_nodes > 0) {
        for (int it = 0; it < n_nodes; ++it) {
          const int4 nd = cn[node];
          const int f = __builtin_amdgcn_readfirstlane(nd.y);
          if (f < 0) {
            label = -1 - f;
            break;
          }
          const float xv = act_a[f & 0xffff];
          const bool left = xv != xv ? (f >> 30) != 0 : xv <= __int_as_float(nd.x);
          node = __builtin_amdgcn_readfirstlane(left ? nd.z : nd.w);
        }
      } else {
        for (int it = 0; it < n_nodes; ++it) {
          const TreeNode nd = nodes[node];
          const int f = __builtin_amdgcn_readfirstlane(nd.feature);
          if (f < 0) {
            label = nd.leaf;
            break;
          }
          const float xv = act_a[f];
          const bool left = xv != xv ? nd.nan_left != 0 : (double)xv <= nd.threshold;
          node = __builtin_amdgcn_readfirstlane(left ? nd.left : nd.right);
        }
      }
    }
    if (ln == 0) lab_k[s] = (uint8_t)label;
    c = ring_count_next(c);
    asm volatile("" ::: "memory");
  }
  // -- the stream's state back: frame, ring, count
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int t = lane + 64 * i;
    if (t < len) row[t] = v[i];
  }
  if (lane < mfcc_n) {
#pragma unroll
    for (int d = 0; d < 5; ++d) rs[d * mfcc_n + lane] = rv[d];
  }
  if (lane == 0) count[s] = c;
}

// LDS of a launch: the blob, the staged nodes, one scratch per wave.  The
// largest table walked from LDS is the one that fits beside ONE wave's
// scratch; a larger one is walked from global memory.
int64_t stream_tree_max_lds_nodes(int blob_n) {
  const int64_t room = (int64_t)kHopLdsBytes - (int64_t)blob_n * sizeof(float) - (int64_t)kHopWaveFloats * sizeof(float);
  return room > 0 ? room / (int64_t)sizeof(TreeNodeC) : 0;
}

template <class TH>
static hipError_t launch_stream_hop_tree_t(const float* blob, int blob_n, int nf, int n_taps, const TreeNodeC* cnodes,
                                           const TreeNode* nodes, int n_nodes, int lds_nodes, float* frames,
                                           int64_t fstride, int len, const void* hop, int64_t hstride, int hlen,
                                           int64_t n_streams, int mfcc_n, float* ring, int* count, uint8_t* labels,
                                           int n_hops, int64_t hop_kstride, int64_t lab_kstride, hipStream_t st) {
  return launch_hop_kernels<&stream_hop_tree_kernel<7, TH>, &stream_hop_tree_kernel<16, TH>>(
      (size_t)blob_n * sizeof(float) + (size_t)lds_nodes * sizeof(TreeNodeC), len, n_streams, n_hops, st, blob, blob_n,
      nf, n_taps, cnodes, nodes, n_nodes, lds_nodes, frames, fstride, len, (const TH*)hop, hstride, hlen, n_streams,
      mfcc_n, ring, count, labels, n_hops, hop_kstride, lab_kstride);
}

// hop: fp32 samples (hop_bytes 4) or int16 PCM (2); strides in elements.  The
// table leaves LDS only when it does not fit at one wave per block.
hipError_t launch_stream_hop_tree(const float* blob, int blob_n, int nf, int n_taps, const TreeNodeC* cnodes,
                                  const TreeNode* nodes, int n_nodes, bool force_global, float* frames,
                                  int64_t fstride, int len, const void* hop, int hop_bytes, int64_t hstride, int hlen,
                                  int64_t n_streams, int mfcc_n, float* ring, int* count, uint8_t* labels, int n_hops,
                                  int64_t hop_kstride, int64_t lab_kstride, hipStream_t st) {
  const bool lds = !force_global && cnodes && n_nodes <= stream_tree_max_lds_nodes(blob_n);
  const auto launch = hop_bytes == 2 ? launch_stream_hop_tree_t<int16_t> : launch_stream_hop_tree_t<float>;
  return launch(blob, blob_n, nf, n_taps, cnodes, nodes, n_nodes, lds ? n_nodes : 0, frames, fstride, len, hop,
                hstride, hlen, n_streams, mfcc_n, ring, count, labels, n_hops, hop_kstride, lab_kstride, st);
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
