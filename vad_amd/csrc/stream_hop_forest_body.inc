// The body of the forest hop kernels (stream_forest_kernel.hip), included once
// per kernel: stream_hop_forest_kernel (VAD_HOP_DENOISE 0, VAD_HOP_SESSIONS 0),
// stream_hop_forest_denoise_kernel, stream_hop_forest_sessions_kernel and
// stream_hop_forest_sessions_denoise_kernel.  Every form writes labels, and
// scores when `scores` is not null.
//
// The front end -- staging, state, frame shift, FFT, real split, mel + log10,
// lifter x DCT, the ring, the window features -- is stream_hop_tree_body.inc's,
// statement for statement (tests/test_gpu_stream_forest.py holds it to the FFN
// kernel's bit for bit: frames, ring and count).  What differs is the table
// behind the blob (the leading fr.lds_nodes compact nodes of the forest: whole
// trees only) and what follows the features: the walk of T trees, lane l tree
// l + 64 p in pass p, and the ordered double average of forest_kernel.hip.
  extern __shared__ __attribute__((aligned(16))) float hsm[];
  const int waves = blockDim.x >> 6;
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  // -- stage the MFCC plan's hop blob, then the staged trees' compact nodes
  // (one node per lane and DMA), by LDS-DMA; then request the stream's state
  // and the FFT's twiddles (registers); then the block's only barrier
  float* base = hsm + waves * kHopWaveFloats;
  {
    const float4* m4 = reinterpret_cast<const float4*>(blob);
    const float4* t4 = reinterpret_cast<const float4*>(fr.f.cnodes);
    const int nm4 = blob_n >> 2, n4 = nm4 + fr.lds_nodes;
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
  // this lane's tree of the first pass: its root (the later passes of a
  // forest of more than 64 trees read theirs per hop)
  const int n_trees = fr.f.T, n_cls = fr.f.K;
  const int root0 = lane < n_trees ? fr.f.roots[lane] : 0;
#if VAD_HOP_DENOISE
  // the denoise state (stream_denoise.h): the estimate in force (the lane's
  // four bins, registers across the hops) and the rows held; the spectrum
  // ring and the noise rows stay in global memory
  const int64_t dn_s = dn_uniform(sc);  // scalar row addresses: the lane's 16 B offset is the only vector part
  float* dn_spec = dn.spec + dn_s * (5 * kBins);
  float* dn_rows = dn.rows + dn_s * (kNoiseRows * kBins);
  float4 dn_e = reinterpret_cast<const float4*>(dn.est + dn_s * kBins)[lane];
  int dn_n = __builtin_amdgcn_readfirstlane(dn.held[sc]);
#endif
#if VAD_HOP_SESSIONS
  // the stream's session for this launch, both wave-uniform (scalar): the
  // hops it takes from its column of the block, min(max(hop_counts[s], 0),
  // n_hops), and whether it starts over first
  int n_s = __builtin_amdgcn_readfirstlane(hop_counts[sc]);
  n_s = n_s < 0 ? 0 : n_s > n_hops ? n_hops : n_s;
  const int restarted = __builtin_amdgcn_readfirstlane((int)restart[sc]);
#endif
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
  // the leaves' class shares of one pass, [tree][class] doubles: 64 x 8 x 8 B
  // = 4 KB of the FFT buffers (4.5 KB), dead between the mel step and the
  // next hop's frame shift
  double* shares = reinterpret_cast<double*>(scr);
  const int used = len < kFftN ? len : kFftN;
#if VAD_HOP_SESSIONS
  if (restarted) {  // what reset() leaves: the registers here, written back below; the flag is consumed
#pragma unroll
    for (int i = 0; i < NR; ++i) v[i] = 0.f;
#pragma unroll
    for (int d = 0; d < 5; ++d) rv[d] = 0.f;
    c = 0;
#if VAD_HOP_DENOISE
    dn_clear(dn_spec, dn_rows, dn.est + dn_s * kBins, lane);  // the lane's own 16 B of the eleven rows
    dn_e = make_float4(0.f, 0.f, 0.f, 0.f);
    dn_n = 0;
#endif
    if (lane == 0) restart[s] = 0;
  }
  if (lane == 0) {  // the rows this stream has no hop in
    for (int k = n_s; k < n_hops; ++k) {
      labels[(int64_t)k * lab_kstride + s] = (uint8_t)VAD_LABEL_NO_HOP;
      if (scores) scores[(int64_t)k * score_kstride + s] = __builtin_nanf("");
    }
  }
  if (n_s == 0 && !restarted) return;  // no hop, no change: nothing is written back
#define VAD_HOP_N n_s
#else
#define VAD_HOP_N n_hops
#endif

  for (int k = 0; k < VAD_HOP_N; ++k) {
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
    if (k + 1 < VAD_HOP_N) {  // the next hop's samples, in flight during this one
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
#if VAD_HOP_DENOISE
    // -- the raw row into the spectrum ring (the MFCC ring's slot), then the
    // noise estimate off the power bins, clamped at zero
    dn_store_subtract(pw, ln, dn_spec + (c % 5) * kBins, dn_e);
    asm volatile("" ::: "memory");
#endif
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
    // -- the forest.  Pass p: lane l walks tree t = l + 64 p, from LDS when the
    // tree is one of the fr.lds_trees staged ones (tree_walk_c_node's rule:
    // float compare against the rounded-down threshold) and from the global
    // table otherwise (tree_walk_node's: double threshold); the choice is the
    // lane's.  A node's feature index is below the forest's n_features <=
    // 3 mfcc_n (checked by the C entry), its children inside its tree
    // (vad_forest_create); the loop is bounded by the largest tree's node
    // count, so a malformed table cannot spin and ends at the tree's root.
    // Then lane t puts its leaf's K shares into the LDS row, and lane k < K
    // adds column k in tree order: K <= 8 double sums, each T adds deep, the
    // additions of forest_kernel.hip in its order.
    int label = 255;
    float score = __builtin_nanf("");
    if (have) {
      double acc = 0.0;
      for (int p0 = 0; p0 < n_trees; p0 += 64) {
        const int t = p0 + ln;
        const bool valid = t < n_trees;
        int root = root0;
        if (p0 > 0) root = valid ? fr.f.roots[t] : 0;
        const bool in_lds = t < fr.lds_trees;
        const int4* tn = cn + root;  // read only by lanes with in_lds: their whole tree is below fr.lds_nodes
        const TreeNode* gn = fr.f.nodes + root;
        int node = 0;
        bool done = !valid;
        for (int it = 0; it < fr.max_tree; ++it) {
          if (__builtin_amdgcn_ballot_w64(!done) == 0) break;  // every lane of the pass at a leaf
          if (!done) {
            if (in_lds) {
              const int4 nd = tn[node];
              if (nd.y < 0) {
                done = true;
              } else {
                const float xv = act_a[nd.y & 0xffff];
                const bool left = xv != xv ? (nd.y >> 30) != 0 : xv <= __int_as_float(nd.x);
                node = left ? nd.z : nd.w;
              }
            } else {
              const TreeNode nd = gn[node];
              if (nd.feature < 0) {
                done = true;
              } else {
                const float xv = act_a[nd.feature];
                const bool left = xv != xv ? nd.nan_left != 0 : (double)xv <= nd.threshold;
                node = left ? nd.left : nd.right;
              }
            }
          }
        }
        const int leaf = done ? node : 0;  // a malformed table: the root, as tree_walk_node
        if (valid) {
          const double* pr = fr.f.proba + (size_t)(root + leaf) * n_cls;
          double* sh = shares + ln * n_cls;
#pragma unroll 2  // two shares in flight: eight would cost sixteen registers the front end has no room for
          for (int q = 0; q < n_cls; ++q) sh[q] = pr[q];
        }
        asm volatile("" ::: "memory");
        const int left_trees = n_trees - p0;
        const int nt = left_trees < 64 ? left_trees : 64;
        if (ln < n_cls) {
          const double* col = shares + ln;
          for (int j = 0; j < nt; ++j) acc += col[j * n_cls];
        }
        asm volatile("" ::: "memory");  // the next pass overwrites the row
      }
      const double mean = acc / (double)n_trees;  // lanes k < K: class k
      const int mlo = __double2loint(mean), mhi = __double2hiint(mean);
      double best = 0.0;
      label = 0;
      for (int q = 0; q < n_cls; ++q) {  // the first maximum, wave-uniform
        const double mq = __hiloint2double(__builtin_amdgcn_readlane(mhi, q), __builtin_amdgcn_readlane(mlo, q));
        if (q == 0 || mq > best) {
          best = mq;
          label = q;
        }
        if (q == fr.active) score = (float)mq;
      }
    }
    if (ln == 0) lab_k[s] = (uint8_t)label;
    if (ln == 0 && scores) scores[(int64_t)k * score_kstride + s] = score;
#if VAD_HOP_DENOISE
    // -- a window of the noise class: the raw row of its middle frame (three
    // hops old, slot (c + 2) % 5 of the spectrum ring) joins the noise rows,
    // and the estimate is taken anew; it holds from the next hop on
    if (have && dn.update && __builtin_amdgcn_readfirstlane((int)label) == dn.noise_class) {
      const float4 mid = reinterpret_cast<const float4*>(dn_spec + ((c + 2) % 5) * kBins)[ln];
      dn_e = dn_estimate(dn_push_mean(dn_rows, dn_n, mid, ln), dn.alpha, ln);
    }
#endif
    c = ring_count_next(c);
    asm volatile("" ::: "memory");
  }
  // -- the stream's state back: frame, ring, count.  The rows' addresses are
  // taken again from the stream index (opaque, so that they are): held over
  // the hops beside the walk's registers they went to scratch
  int64_t se = s;
  asm volatile("" : "+v"(se));
  float* row_e = frames + se * fstride;
  float* rs_e = ring + se * 5 * mfcc_n;
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int t = lane + 64 * i;
    if (t < len) row_e[t] = v[i];
  }
  if (lane < mfcc_n) {
#pragma unroll
    for (int d = 0; d < 5; ++d) rs_e[d * mfcc_n + lane] = rv[d];
  }
  if (lane == 0) count[se] = c;
#if VAD_HOP_DENOISE
  reinterpret_cast<float4*>(dn.est + dn_uniform(se) * kBins)[lane] = dn_e;
  if (lane == 0) dn.held[se] = dn_n;
#endif
#undef VAD_HOP_N
