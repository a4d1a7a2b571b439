// The body of the streaming segment kernels (stream_segments_kernel.hip),
// included once per kernel: stream_segments_kernel with VAD_SEG_OP 0 -- the
// label form, token for token what it was before there was an operating
// point, hence its instructions (profiles/stream_scores/isa.md) -- and
// stream_segments_op_kernel with VAD_SEG_OP 1: scores through the hysteresis
// (SCORES) or labels, a confirmed run padded before it is joined and queued.
// With VAD_SEG_SESSIONS 1 the two sessions kernels (per-stream hop counts and
// restarts, `ss`); with 0 the expansion is token for token what it was before
// there were sessions (profiles/stream_segments_sessions/isa.md).  The hop
// itself is stream_segments_step.inc, included by each kernel's loop over hops.
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
#if VAD_SEG_SESSIONS
  // -- sessions: the stream's hop count and restart flag, read once, scalar
  int n_s = __builtin_amdgcn_readfirstlane(ss.hop_counts[s]);
  n_s = n_s < 0 ? 0 : (n_s > a.n_hops ? a.n_hops : n_s);
  const bool restart = __builtin_amdgcn_readfirstlane((int)ss.restart[s]) != 0;
  bool live = st.ended == 0;
  const bool ending = restart && live && st.t > 0;  // fresh or flushed: nothing to end
  if (!ending)
    for (int f = lane; f < ss.flush_rows; f += 64) ss.end_len[(int64_t)f * a.n_streams + s] = 0;
  if (!restart && n_s == 0) {  // stalled: every byte of the stream's slices stays
    if (AUDIO)
      for (int k = lane; k < a.n_hops; k += 64) a.voiced_len[(int64_t)k * a.n_streams + s] = 0;
    return;
  }
  T* ring = AUDIO ? static_cast<T*>(a.history) + s * (int64_t)R : nullptr;
  // the prefix of hop t starts L + (D+2)H elements behind that hop's samples
  const int back = (int)(L + (a.delay + 2) * H);  // <= R (checked by the entry)
  const int64_t m1 = a.min_run > 1 ? a.min_run : 1;
  if (restart && lane == 0) ss.restart[s] = 0;  // consumed: a flag set once restarts once
  // One loop over n_end + n_s hops, so that ending a session and the live
  // hops run the same step: first, for a restarted stream with a session to
  // end, this stream's flush -- F hops of inactive windows and no samples,
  // rows and prefixes as vad_stream_segments_flush -- then the block's hops.
  const int n_end = ending ? ss.flush_rows : 0;
#if VAD_SEG_OP
  if (ending && st.nq > 0 && st.q[0][1] > st.t - 6) st.q[0][1] = st.t - 6;
#endif
  // before the first live hop, or after the last flush hop when there is none
  auto begin = [&]() {
    if (restart) {
      // -- become fresh: as zeroed but for the session ordinal, zero carry
      const int32_t ordinal = st.pad[0] + 1;
      st = SegStreamState{};
      st.pad[0] = ordinal;
      live = true;
      if (AUDIO) {
        // the old session's prefix reads are done before its history goes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        for (int i = lane; i < L - H; i += 64) ring[R - (L - H) + i] = T(0);
      }
    }
    if (AUDIO && live) {
      // -- the stream's n_s new rows of samples into the history
      int w = st.wpos;
      for (int k = 0; k < n_s; ++k) {
        const T* h = static_cast<const T*>(a.hop_samples) + (int64_t)k * a.hop_kstride + s * a.hstride;
        for (int i = lane; i < H; i += 64) {
          int p = w + i;
          if (p >= R) p -= R;
          ring[p] = h[i];
        }
        w += H;
        if (w >= R) w -= R;
      }
      // the prefixes below may read them, and a new session its zeroed carry
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
  };
#define SEG_VOICED rows_out
#define SEG_VLEN len_out
#define SEG_LEN_ON len_on
  for (int it = 0; it <= n_end + n_s; ++it) {
    if (it == n_end) begin();
    if (it == n_end + n_s) break;  // begin() has run, hops or not
    const bool flush = it < n_end;
    const int k = flush ? it : it - n_end;
    void* rows_out = flush ? ss.end_voiced : a.voiced;
    int32_t* len_out = flush ? ss.end_len : a.voiced_len;
    const bool len_on = flush || AUDIO;
#include "stream_segments_step.inc"
  }
#undef SEG_VOICED
#undef SEG_VLEN
#undef SEG_LEN_ON
  if (AUDIO)  // rows the stream has no hop in
    for (int k = n_s + lane; k < a.n_hops; k += 64) a.voiced_len[(int64_t)k * a.n_streams + s] = 0;
#else
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

#define SEG_VOICED a.voiced
#define SEG_VLEN a.voiced_len
#define SEG_LEN_ON AUDIO
  for (int k = 0; k < a.n_hops; ++k) {
#include "stream_segments_step.inc"
  }
  if (flush) st.ended = 1;
#undef SEG_VOICED
#undef SEG_VLEN
#undef SEG_LEN_ON
#endif
  if (lane == 0) {
    *sp = st;
    a.found[s] = found;
  }
#undef SEG_PAD_A
#undef SEG_PAD_B
