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
// Operating point (stream_segments_op_kernel; the clip chain of
// score_kernel.hip, hysteresis -> smooth -> dilate -> segments, one window at
// a time).  The block holds scores or labels.
//   hysteresis  h = 1 at s >= on, 0 at s < off or NaN, else the previous h
//               (0 before the first window); a = h.  One bit of the state.
//   padding     a confirmed run [r0, r1] is queued and joined as
//               [max(r0 - pad_before, 0), r1 + pad_after]: the join test is
//               (r0 - pad_before) - end - 1 <= j against the newest segment's
//               padded end, and that end follows r1 + pad_after.  A flush
//               knows the window count N and stops the newest end at N - 1.
//   delay       D = max_gap + max(min_run, 1) + j + 1 + pad_before.  A run is
//               confirmed at a window n <= r0 + max(min_run, 1) + max_gap - 1
//               and then changes windows >= r0 - pad_before - j (its padded
//               start, or the gap of <= j windows it closes), which is
//               > n - D.  Growing a confirmed run moves an end forward from
//               r1 + pad_after: windows > r1 >= n - max_gap - 1 > n - D, so
//               pad_after adds no delay.  c[d], d = n - D, is therefore final.
//   queue       two queued segments come from runs whose starts are at least
//               max(min_run, 1) + max_gap + 1 apart; after the finished one
//               left, the oldest ends at >= d, so every younger run starts at
//               r0 >= d + pad_before + j + 2 = n - max_gap - max(min_run, 1) + 1
//               and was confirmed, r0 <= n - max(min_run, 1) + 1: max_gap + 1
//               places, less than the spacing, hold one start.  Two queued
//               after a step, three within it; the four places still suffice.
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
//
// Sessions (stream_segments_sessions_kernel, stream_segments_op_sessions_kernel;
// include/vad_amd.h, "Sessions in the streaming segmenter").  The wave reads
// its stream's hop count and restart flag once, makes both scalar, and takes
// n_s = min(max(count, 0), n_hops) hops: a loop bound.  A set flag is cleared
// by lane 0 and, before the hops, (1) ends the running session -- the F flush
// hops of this stream alone, as the first iterations of the one loop that
// also runs the live hops (one expansion of stream_segments_step.inc), rows
// appended, prefixes to end_voiced / end_len -- and (2) makes the state fresh but for the session ordinal in pad[0],
// zeroing the L - H carry positions at the slice's top.  The prefix reads of
// (1) are drained before the stores of (2), and those and the block's hops
// are drained and fenced before the new session's first prefix read, by the
// fence above.  The ring bound is unchanged: the end flush appends no samples
// and runs before the block's hops are written, so it reads what a flush
// entry would read (R >= (D+3)H + L, the bound at n_hops = 0); the new session
// then starts at index 0 and writes n_s * H <= n_hops * H elements, and its
// prefixes start at clip position 2H: in the zeroed carry or in those hops,
// never in what the old session left.  A stream with no hop and no restart
// returns before any store to its state, history, found or table.
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
  int32_t hyst;      // the operating-point forms' hysteresis decision h (one bit; 0 before the first window)
  int32_t pad[2];    // pad[0]: the session ordinal (sessions kernels: restarts consumed so far)
};
static_assert(sizeof(SegStreamState) == kSegStreamStateBytes, "the sizing entry's bytes per stream");

constexpr int kSegStreamWaves = 4;


// The body is stream_segments_body.inc, included by the label kernel and by
// the operating-point kernel (SCORES: the block holds fp32 scores).
template <class T, bool AUDIO>
__global__ __launch_bounds__(64 * kSegStreamWaves) void stream_segments_kernel(SegStreamArgs a) {
#define VAD_SEG_OP 0
#define VAD_SEG_SESSIONS 0
#include "stream_segments_body.inc"
#undef VAD_SEG_SESSIONS
#undef VAD_SEG_OP
}

template <class T, bool AUDIO, bool SCORES>
__global__ __launch_bounds__(64 * kSegStreamWaves) void stream_segments_op_kernel(SegStreamArgs a, SegOpArgs op) {
#define VAD_SEG_OP 1
#define VAD_SEG_SESSIONS 0
#include "stream_segments_body.inc"
#undef VAD_SEG_SESSIONS
#undef VAD_SEG_OP
}

// The sessions forms: the same bodies with per-stream hop counts and restarts.
template <class T, bool AUDIO>
__global__ __launch_bounds__(64 * kSegStreamWaves) void stream_segments_sessions_kernel(SegStreamArgs a,
                                                                                        SegSessArgs ss) {
#define VAD_SEG_OP 0
#define VAD_SEG_SESSIONS 1
#include "stream_segments_body.inc"
#undef VAD_SEG_SESSIONS
#undef VAD_SEG_OP
}

template <class T, bool AUDIO, bool SCORES>
__global__ __launch_bounds__(64 * kSegStreamWaves) void stream_segments_op_sessions_kernel(SegStreamArgs a,
                                                                                           SegOpArgs op,
                                                                                           SegSessArgs ss) {
#define VAD_SEG_OP 1
#define VAD_SEG_SESSIONS 1
#include "stream_segments_body.inc"
#undef VAD_SEG_SESSIONS
#undef VAD_SEG_OP
}

template <class T, bool AUDIO>
hipError_t launch_t(const SegStreamArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)((a.n_streams + kSegStreamWaves - 1) / kSegStreamWaves));
  hipLaunchKernelGGL((stream_segments_kernel<T, AUDIO>), grid, dim3(64 * kSegStreamWaves), 0, st, a);
  return hipGetLastError();
}

template <class T, bool AUDIO>
hipError_t launch_op_t(const SegStreamArgs& a, const SegOpArgs& op, hipStream_t st) {
  const dim3 grid((unsigned)((a.n_streams + kSegStreamWaves - 1) / kSegStreamWaves));
  if (op.is_scores)
    hipLaunchKernelGGL((stream_segments_op_kernel<T, AUDIO, true>), grid, dim3(64 * kSegStreamWaves), 0, st, a, op);
  else
    hipLaunchKernelGGL((stream_segments_op_kernel<T, AUDIO, false>), grid, dim3(64 * kSegStreamWaves), 0, st, a, op);
  return hipGetLastError();
}

template <class T, bool AUDIO>
hipError_t launch_sessions_t(const SegStreamArgs& a, const SegOpArgs* op, const SegSessArgs& ss, hipStream_t st) {
  const dim3 grid((unsigned)((a.n_streams + kSegStreamWaves - 1) / kSegStreamWaves)), block(64 * kSegStreamWaves);
  if (!op)
    hipLaunchKernelGGL((stream_segments_sessions_kernel<T, AUDIO>), grid, block, 0, st, a, ss);
  else if (op->is_scores)
    hipLaunchKernelGGL((stream_segments_op_sessions_kernel<T, AUDIO, true>), grid, block, 0, st, a, *op, ss);
  else
    hipLaunchKernelGGL((stream_segments_op_sessions_kernel<T, AUDIO, false>), grid, block, 0, st, a, *op, ss);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_stream_segments(const SegStreamArgs& a, int audio_bytes, hipStream_t st) {
  if (a.n_streams <= 0 || a.n_hops <= 0) return hipSuccess;
  if (audio_bytes == 4) return launch_t<float, true>(a, st);
  if (audio_bytes == 2) return launch_t<int16_t, true>(a, st);
  return launch_t<int16_t, false>(a, st);
}

// The operating-point forms: a.labels is the block (scores or labels, by
// op.is_scores; nullptr: flush) and a.delay already holds the padded delay.
hipError_t launch_stream_segments_op(const SegStreamArgs& a, const SegOpArgs& op, int audio_bytes, hipStream_t st) {
  if (a.n_streams <= 0 || a.n_hops <= 0) return hipSuccess;
  if (audio_bytes == 4) return launch_op_t<float, true>(a, op, st);
  if (audio_bytes == 2) return launch_op_t<int16_t, true>(a, op, st);
  return launch_op_t<int16_t, false>(a, op, st);
}

// The sessions forms of a push (op == nullptr: the label kernel).
hipError_t launch_stream_segments_sessions(const SegStreamArgs& a, const SegOpArgs* op, const SegSessArgs& ss,
                                           int audio_bytes, hipStream_t st) {
  if (a.n_streams <= 0 || a.n_hops <= 0) return hipSuccess;
  if (audio_bytes == 4) return launch_sessions_t<float, true>(a, op, ss, st);
  if (audio_bytes == 2) return launch_sessions_t<int16_t, true>(a, op, ss, st);
  return launch_sessions_t<int16_t, false>(a, op, ss, st);
}

}  // namespace vad
