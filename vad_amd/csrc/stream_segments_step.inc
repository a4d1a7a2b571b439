// One hop of one stream through the segment machine (the loop body of
// stream_segments_body.inc, which says what the names mean): hop k of a
// block, or flush hop k when `flush` is set.  Included once by the loop over
// hops of every kernel; in the sessions kernels that one loop first runs the
// flush hops that end a restarted stream's session and then the live hops,
// so both are the same state machine.  The includer names the outputs:
// SEG_VOICED / SEG_VLEN the rows the prefix and its length go to, SEG_LEN_ON
// whether the length is stored.
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
#if VAD_SEG_SESSIONS
              ss.table_session[s * a.capacity + found] = st.pad[0];  // the row's session ordinal
#endif
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
          T* out = static_cast<T*>(SEG_VOICED) + ((int64_t)k * a.n_streams + s) * H;
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
    if (SEG_LEN_ON && lane == 0) SEG_VLEN[(int64_t)k * a.n_streams + s] = len;
