// The body of the streaming segment kernels (stream_segments_kernel.hip),
// included once per kernel: stream_segments_kernel with VAD_SEG_OP 0 -- the
// label form, token for token what it was before there was an operating
// point, hence its instructions (profiles/stream_scores/isa.md) -- and
// stream_segments_op_kernel with VAD_SEG_OP 1: scores through the hysteresis
// (SCORES) or labels, a confirmed run padded before it is joined and queued.
#if VAD_SEG_OP
#define SEG_PAD_A +op.pad_after
#define SEG_PAD_B -op.pad_before
#else
#define SEG_PAD_A
#define SEG_PAD_B
#endif
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t s = (int64_t)blockIdx.x * kSegStreamWaves + wv;
  if (s >= a.n_streams) return;  // wave-uniform; there is no barrier below
  SegStreamState* sp = static_cast<SegStreamState*>(a.state) + s;
  SegStreamState st = *sp;
  int64_t found = a.found[s];
  const int H = a.hop, L = a.frame_size, R = a.ring;
  // a state that was never zeroed must not become an address
  if ((uint32_t)st.wpos >= (uint32_t)R) st.wpos = 0;
  if ((uint32_t)st.nq > 4u) st.nq = 0;
  const bool flush = a.labels == nullptr;
  const bool live = st.ended == 0;
  T* ring = AUDIO ? static_cast<T*>(a.history) + s * (int64_t)R : nullptr;
#if VAD_SEG_OP
  // the flush knows the stream's window count N = t - 5: the newest
  // segment's padded end stops at window N - 1 (older ones end before it)
  if (flush && live && st.nq > 0 && st.q[0][1] > st.t - 6) st.q[0][1] = st.t - 6;
#endif

  if (AUDIO && live && !flush) {
    // -- the block's new samples into the history
    int w = st.wpos;
    for (int k = 0; k < a.n_hops; ++k) {
      const T* h = static_cast<const T*>(a.hop_samples) + (int64_t)k * a.hop_kstride + s * a.hstride;
      for (int i = lane; i < H; i += 64) {
        int p = w + i;
        if (p >= R) p -= R;
        ring[p] = h[i];
      }
      w += H;
      if (w >= R) w -= R;
    }
    // the prefixes below may read them: other lanes' stores of this wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  // the prefix of hop t starts L + (D+2)H elements behind that hop's samples
  const int back = (int)(L + (a.delay + 2) * H);  // <= R (checked by the entry)
  const int64_t m1 = a.min_run > 1 ? a.min_run : 1;

  for (int k = 0; k < a.n_hops; ++k) {
    int len = 0;
    if (live) {
      const int64_t t = st.t;
      if (t >= 5) {
        const int64_t n = t - 5;
#if VAD_SEG_OP
        bool act;
        if constexpr (SCORES) {
          if (!flush) {
            const float sc = reinterpret_cast<const float*>(a.labels)[(int64_t)k * a.lab_kstride + s];
            if (sc >= op.on) st.hyst = 1;
            else if (!(sc >= op.off)) st.hyst = 0;  // below off, or NaN
          }
          act = !flush && st.hyst != 0;
        } else {
          act = !flush && a.labels[(int64_t)k * a.lab_kstride + s] == a.active;
        }
#else
        const bool act = !flush && a.labels[(int64_t)k * a.lab_kstride + s] == a.active;
#endif
        if (act) {
          if (!st.cand) {
            st.cand = 1;
            st.conf = 0;
            st.r0 = n;
          }
          st.r1 = n;
          if (st.conf) {
            st.q[0][1] = n SEG_PAD_A;
          } else if (st.r1 - st.r0 + 1 >= m1) {
            st.conf = 1;
            if (st.nq > 0 && st.r0 SEG_PAD_B - st.q[0][1] - 1 <= a.join) {
              st.q[0][1] = n SEG_PAD_A;
            } else {
#pragma unroll
              for (int i = 3; i > 0; --i) {
                st.q[i][0] = st.q[i - 1][0];
                st.q[i][1] = st.q[i - 1][1];
              }
#if VAD_SEG_OP
              st.q[0][0] = st.r0 < op.pad_before ? 0 : st.r0 - op.pad_before;
#else
              st.q[0][0] = st.r0;
#endif
              st.q[0][1] = n SEG_PAD_A;
              if (st.nq < 4) ++st.nq;  // never full (see above); if it were, the oldest would go
            }
          }
        } else if (st.cand && n - st.r1 > a.max_gap) {
          st.cand = 0;
          st.conf = 0;
        }
        const int64_t d = n - a.delay;
        if (d >= 0) {
          int64_t o0 = 0, o1 = -1;  // the oldest queued segment
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (st.nq == i + 1) {
              o0 = st.q[i][0];
              o1 = st.q[i][1];
            }
          if (st.nq > 0 && o1 < d) {  // finished: window o1 + 1 is decided and inactive
            if (found >= 0 && found < a.capacity && lane == 0) {
              int64_t* row = a.segments + (s * a.capacity + found) * 2;
              row[0] = (o0 + 2) * H;
              row[1] = (o1 + 2) * H + L;
            }
            ++found;
            --st.nq;
            o0 = 0, o1 = -1;
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (st.nq == i + 1) {
                o0 = st.q[i][0];
                o1 = st.q[i][1];
              }
          }
          if (st.nq > 0 && o0 <= d && d <= o1) st.e1 = d + 1;
          if (st.e1 > 0) {
            // (e+2)H + L - (d+2)H, clamped to [0, H]
            const int64_t v = (st.e1 - 1 - d) * H + L;
            len = v < 0 ? 0 : (v > H ? H : (int)v);
          }
        }
      }
      if (AUDIO) {
        if (len > 0) {
          int r = st.wpos - back;
          if (r < 0) r += R;
          T* out = static_cast<T*>(a.voiced) + ((int64_t)k * a.n_streams + s) * H;
          for (int i = lane; i < len; i += 64) {
            int p = r + i;
            if (p >= R) p -= R;
            out[i] = ring[p];
          }
        }
        st.wpos += H;
        if (st.wpos >= R) st.wpos -= R;
      }
      st.t = t + 1;
    }
    if (AUDIO && lane == 0) a.voiced_len[(int64_t)k * a.n_streams + s] = len;
  }
  if (flush) st.ended = 1;
  if (lane == 0) {
    *sp = st;
    a.found[s] = found;
  }
#undef SEG_PAD_A
#undef SEG_PAD_B
