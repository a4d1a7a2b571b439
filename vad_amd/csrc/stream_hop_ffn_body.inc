// The body of the FFN hop kernels (stream_kernel.hip), included once per
// kernel: stream_hop_kernel with VAD_HOP_SCORE 0 -- the label-only kernel,
// token for token the kernel it was before there were scores, hence its
// instructions (profiles/stream_scores/isa.md; the same body as an inlined
// function template kept every register count but not the schedule) -- and
// stream_hop_scores_kernel with VAD_HOP_SCORE 1, which also writes, per hop,
// the fp32 score of class `active` to scores[k * score_kstride + s]: the
// softmax of score_dev.h on the wave-uniform logits the argmax reads,
// computed and stored by lane 0; NaN for a hop that has no window yet.
// stream_hop_denoise_kernel is the scored form with VAD_HOP_DENOISE 1: the
// noise estimate comes off the power spectrum before the mel bank, and the
// windows of the noise class feed it (stream_denoise.h); its `scores` may be
// null.  With VAD_HOP_DENOISE 0 the text is what it was without it.
// stream_hop_sessions_kernel and stream_hop_sessions_denoise_kernel are the
// scored form (nullable `scores`) with VAD_HOP_SESSIONS 1, with VAD_HOP_DENOISE
// 0 and 1: per stream a hop count for this launch and a restart flag, both
// scalar in the stream's wave (DESIGN.md section 4).  With VAD_HOP_SESSIONS 0
// the text is what it was without it.
  extern __shared__ __attribute__((aligned(16))) float hsm[];
  const int waves = blockDim.x >> 6;
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  // -- stage the plans' tables (the MFCC plan's hop blob, then the FFN
  // weights) by LDS-DMA (global_load_lds_dwordx4: 1 KB per wave-instruction,
  // no registers, all in flight at once), then request the stream's state
  // and the FFT's twiddles (registers), then the block's only barrier.
  // (A/B, 512 streams, profiles/r05/ab/hop_staging_ab.json: 10.26 us per
  // one-hop launch against 10.56 for register staging with LDS twiddles;
  // the barrier moved after the first hop's FFT, so that the staging would
  // overlap it, measured 10.84: the mid-hop barrier costs more than it hides)
  float* base = hsm + waves * kHopWaveFloats;
  {
    const float4* m4 = reinterpret_cast<const float4*>(blob);
    const float4* w4 = reinterpret_cast<const float4*>(net.wraw);
    const int nm4 = blob_n >> 2, n4 = nm4 + (net.wraw_n >> 2);
    for (int c0 = wv * 64; c0 < n4; c0 += (int)blockDim.x) {  // wave-uniform chunk base
      const int c = c0 + lane;
      if (c < n4)
        __builtin_amdgcn_global_load_lds(c < nm4 ? (const void*)(m4 + c) : (const void*)(w4 + (c - nm4)),
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
  const float* wts = base + blob_n;  // the FFN weights (FfnDev::wraw: transposed rows)

  const int64_t s = (int64_t)blockIdx.x * waves + wv;
  const int64_t sc = s < n_streams ? s : 0;
  // -- the stream's state, requested before the barrier so its latency
  // overlaps the staging: the frame as it stands (registers, sample t =
  // lane + 64 i), the first hop's new samples at the positions they take in
  // the advanced frame, the frame count and the MFCC ring
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
#if VAD_HOP_DENOISE
  // the denoise state (stream_denoise.h): the rows held; the spectrum ring,
  // the noise rows and here the estimate too stay in global memory (the 7-chunk
  // build has no four registers left to carry the lane's bins of the estimate
  // across the hops without scratch, as the tree kernel does: each hop reads
  // them again, 16 B per lane that the lane itself or the launch before wrote)
  const int64_t dn_s = dn_uniform(sc);  // scalar row addresses: the lane's 16 B offset is the only vector part
  float* dn_spec = dn.spec + dn_s * (5 * kBins);
  float* dn_rows = dn.rows + dn_s * (kNoiseRows * kBins);
  float4* dn_est = reinterpret_cast<float4*>(dn.est + dn_s * kBins);
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
  // this lane's FFT twiddles (W512^k table = the blob's first 256 complex):
  // stage st's radix-4 butterfly multiplies by W256^(j m), m = (lane mod
  // 4^st) 64 / 4^st, j = 1..3; the real-FFT split by W512^(lane + 64 q)
  // (the 16-chunk build, whose frame registers leave no room for them, reads
  // them from the staged table where it uses them)
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
  // wait is explicit (vmcnt 0, before the barrier; the state and twiddle
  // loads above are needed right after it anyway).  Locked by
  // test_hop_kernel_waits_for_lds_dma_before_barrier (the built ISA).
  __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt 0, expcnt 7, lgkmcnt 15
  __syncthreads();
  if (s >= n_streams) return;  // wave-uniform; no barrier below
  float* scr = hsm + wv * kHopWaveFloats;
  float2* z0 = reinterpret_cast<float2*>(scr);
  float2* z1 = reinterpret_cast<float2*>(scr + kHopZ);
  float* lmr = scr + 2 * kHopZ;
  float* act_a = lmr + kMaxFilters;
  float* act_b = act_a + 64;
  float* fb = scr;  // the frame shift goes through the FFT buffers (2 kHopZ >= 1024 floats)
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

  // K hops of this stream back to back: the same computation per hop as K
  // launches of one hop (state carried in registers), the tables staged once
  for (int k = 0; k < VAD_HOP_N; ++k) {
    // the lane index, opaque per hop: otherwise the compiler hoists every
    // lane-dependent LDS address of the hop out of the loop and runs out of
    // registers holding them
    int ln = lane;
    asm volatile("" : "+v"(ln));
    // -- frame: shift by the hop (through LDS: sample t + hlen belongs to
    // another ln), append the new samples (stream_push_kernel)
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
    // LDS is in order within a wave; these keep the compiler from moving
    // accesses of one phase (other lanes' data, other element types) across
    // the next
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
    // -- real-FFT split: 2X[k] = S - i W512^k D, S = Z[k] + conj(Z[-k]),
    // D = Z[k] - conj(Z[-k]); |2X|^2 into the free buffer
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
    dn_store_subtract(pw, ln, dn_spec + (c % 5) * kBins, dn_est[ln]);
    asm volatile("" ::: "memory");
#endif
    // -- mel + log10 (ln m), lifter x DCT (ln c)
    if (ln < nf) {
      // the filter's 16-B aligned tap row against the power bins from its
      // first bin rounded down to 4: four taps per pair of 16-B reads, one
      // fma chain in bin order (the zero taps around the filter add +0)
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
      // one fma chain in m order; four terms per pair of 16-B reads (the
      // lane's row, the log-mel row broadcast)
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
    act_a[ln] = 0.f;  // feature columns past 3 mfcc_n: zero (the FFN reads them in fours)
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
    {
      // layer 0 reads its inputs in fours: a network narrower than the feature
      // triple (13-64-64-N takes the 13 normalised coefficients) must see zeros,
      // not the delta columns, in the rest of its last block (stored after the
      // features: LDS is in order per wave)
      const int din0 = net.dims[0];
      if (ln >= din0 && ln < ((din0 + 3) & ~3)) act_a[ln] = 0.f;
    }
    asm volatile("" ::: "memory");
    uint8_t label = 255;
    if (have) {
      // -- FFN: exact f32, ln o of each layer
      float* hin = act_a;
      float* hout = act_b;
      const int nl = net.n_layers;
      for (int l = 0; l < nl; ++l) {
        const int din = net.dims[l], dout = net.dims[l + 1];
        // four inputs per step (one ds_read_b128 broadcast), four partial
        // sums; inputs past din are zero and the weight rows past W_l read
        // the next finite values of the block (zero-padded at its end)
        // the lane's transposed row: four weights per 16-B read
        const float4* w4 = reinterpret_cast<const float4*>(wts + net.woff[l] + ln * net.wstride[l]);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        if (ln < dout) {
          const float4* h4 = reinterpret_cast<const float4*>(hin);
#pragma unroll 4
          for (int kq = 0; kq < din; kq += 4) {
            const float4 h = h4[kq >> 2], w = w4[kq >> 2];
            a0 = fmaf(w.x, h.x, a0);
            a1 = fmaf(w.y, h.y, a1);
            a2 = fmaf(w.z, h.z, a2);
            a3 = fmaf(w.w, h.w, a3);
          }
        }
        const float acc = wts[net.boff[l] + (ln < dout ? ln : 0)] + ((a0 + a1) + (a2 + a3));
        hout[ln] = ln < dout ? (l + 1 < nl ? relu_nan(acc) : acc) : 0.f;
        float* t = hin;
        hin = hout;
        hout = t;
        asm volatile("" ::: "memory");
      }
      const f32x4 zl = {hin[0], hin[1 < net.n_classes ? 1 : 0], hin[2 < net.n_classes ? 2 : 0],
                        hin[3 < net.n_classes ? 3 : 0]};
      label = (uint8_t)argmax_classes(zl, net.n_classes);
#if VAD_HOP_SCORE
#if VAD_HOP_DENOISE || VAD_HOP_SESSIONS
      if (ln == 0 && scores) {  // the denoising kernel is the scored form; its scores may be null
#else
      if (ln == 0) {
#endif
        const int nc = net.n_classes;
        scores[(int64_t)k * score_kstride + s] = nc == 2   ? softmax_score<2>(zl, active)
                                                 : nc == 3 ? softmax_score<3>(zl, active)
                                                 : nc == 4 ? softmax_score<4>(zl, active)
                                                           : softmax_score<1>(zl, active);
      }
#if VAD_HOP_DENOISE || VAD_HOP_SESSIONS
    } else if (ln == 0 && scores) {
#else
    } else if (ln == 0) {
#endif
      scores[(int64_t)k * score_kstride + s] = __builtin_nanf("");
#endif
    }
    if (ln == 0) lab_k[s] = label;
#if VAD_HOP_DENOISE
    // -- a window of the noise class: the raw row of its middle frame (three
    // hops old, slot (c + 2) % 5 of the spectrum ring) joins the noise rows,
    // and the estimate is taken anew; it holds from the next hop on
    if (have && dn.update && __builtin_amdgcn_readfirstlane((int)label) == dn.noise_class) {
      const float4 mid = reinterpret_cast<const float4*>(dn_spec + ((c + 2) % 5) * kBins)[ln];
      dn_est[ln] = dn_estimate(dn_push_mean(dn_rows, dn_n, mid, ln), dn.alpha, ln);
    }
#endif
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
#if VAD_HOP_DENOISE
  if (lane == 0) dn.held[s] = dn_n;
#endif
#undef VAD_HOP_N
