// Streaming segments (include/vad_amd.h, "Streaming segments"): per stream,
// the label blocks of the hop kernels -> finished speech segments and the
// voiced samples, with the fixed delay D = max_gap + max(min_run, 1) + j + 1
// windows (j = frame_size / hop - 1).  What vad.py:32-59 does in its live
// loop (keep the samples of the active frames), after the smoothing of the
// clip path (segments_kernel.hip), for S streams at once.
//
// One wave per stream, as stream_hop_kernel.  The state machine runs on
// wave-uniform values over the block's n_hops label bytes; the 64 lanes do
// the copies.  No LDS, no atomics, no kernel or workgroup waits on another:
// a stream is owned by one wave, and a wave talks to itself through its own
// slice of the history only.
//
// State machine, window n = t - 5 arriving at hop t (a = label == active):
//   candidate  the run of close(max_gap)(a) still open: [r0, r1], r1 its last
//              active window; it ends when max_gap + 1 inactive windows
//              follow r1, and is dropped then unless confirmed;
//   confirmed  r1 - r0 + 1 >= max(min_run, 1): the run survives open(min_run).
//              At that moment it joins the newest queued segment when the gap
//              between them is <= j (close(j)), else it is queued as a new
//              segment; from then on the newest segment's end follows r1;
//   queue      the segments not yet passed by the decided window d = n - D,
//              newest first.  Two segment starts are at least
//              max(min_run, 1) + max(max_gap, j) + 1 windows apart and
//              D < twice that, so at most three are queued; there is room
//              for four.
//   decide     d = n - D >= 0: the oldest queued segment with end < d is
//              finished (its row is appended: end + 1 = d is decided and
//              inactive); c[d] = d inside the oldest remaining segment;
//              e = the last d with c[d] = 1.
// Every change the machine makes at window n touches windows > n - D only
// (confirmation: >= r0 - j with r0 > n - max_gap - min_run),
// which is why c[d] is read off the queue without looking ahead.
//
// Audio.  Clip position p of a stream lives at history[(p - (L - H)) mod R]
// of its slice of R elements; positions below L - H (the carried samples) at
// the slice's top, zero unless the host put the carry there.  A launch first
// appends the block's n_hops hops, then copies each hop's decided prefix
// [(d+2)H, (d+2)H + len) to its output row: the oldest sample a block reads
// is L + (D+2)H behind its first write and it writes n_hops * H, so nothing
// still needed is overwritten while R >= (D+3)H + L + n_hops * H.  A prefix
// can lie in hops of the same launch; the wave's stores are drained and
// fenced (workgroup scope: one L1 per CU) before its first read.
#include "vad_common.h"

namespace vad {
namespace {

struct SegStreamState {
  int64_t t;         // hops seen
  int64_t e1;        // e + 1 (0: no decided active window yet)
  int64_t r0, r1;    // the candidate run
  int64_t q[4][2];   // queued segments [i0, i1], newest first
  int32_t cand, conf, nq;
  int32_t wpos;      // history index of the next hop's first sample
  int32_t ended;     // flushed: every further row is empty until the state is zeroed
  int32_t pad[3];
};
static_assert(sizeof(SegStreamState) == kSegStreamStateBytes, "the sizing entry's bytes per stream");

constexpr int kSegStreamWaves = 4;

template <class T, bool AUDIO>
__global__ __launch_bounds__(64 * kSegStreamWaves) void stream_segments_kernel(SegStreamArgs a) {
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
        const bool act = !flush && a.labels[(int64_t)k * a.lab_kstride + s] == a.active;
        if (act) {
          if (!st.cand) {
            st.cand = 1;
            st.conf = 0;
            st.r0 = n;
          }
          st.r1 = n;
          if (st.conf) {
            st.q[0][1] = n;
          } else if (st.r1 - st.r0 + 1 >= m1) {
            st.conf = 1;
            if (st.nq > 0 && st.r0 - st.q[0][1] - 1 <= a.join) {
              st.q[0][1] = n;
            } else {
#pragma unroll
              for (int i = 3; i > 0; --i) {
                st.q[i][0] = st.q[i - 1][0];
                st.q[i][1] = st.q[i - 1][1];
              }
              st.q[0][0] = st.r0;
              st.q[0][1] = n;
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
}

template <class T, bool AUDIO>
hipError_t launch_t(const SegStreamArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)((a.n_streams + kSegStreamWaves - 1) / kSegStreamWaves));
  hipLaunchKernelGGL((stream_segments_kernel<T, AUDIO>), grid, dim3(64 * kSegStreamWaves), 0, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_stream_segments(const SegStreamArgs& a, int audio_bytes, hipStream_t st) {
  if (a.n_streams <= 0 || a.n_hops <= 0) return hipSuccess;
  if (audio_bytes == 4) return launch_t<float, true>(a, st);
  if (audio_bytes == 2) return launch_t<int16_t, true>(a, st);
  return launch_t<int16_t, false>(a, st);
}

}  // namespace vad
