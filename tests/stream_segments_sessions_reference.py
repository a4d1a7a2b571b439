"""Host model of the sessions form of the streaming segmenter (include/vad_amd.h,
"Sessions in the streaming segmenter"), and the seeded workloads the CPU and
GPU tests share.

The model is built from the models the plain segmenter is tested with, not
from the kernel: per stream it keeps ONE one-stream model of the running
session -- StreamSegModel (tests/test_stream_segments_cpu.py) for the label
form, OpSegModel below (the same model deciding from the clip chain of
tests/stream_scores_reference.py) for the operating-point forms.  A restart
flag flushes that model, files its rows under the session's ordinal and
starts a new one; a push feeds it the stream's first n_s rows.  The outputs
are the device's: voiced / voiced_len with zero lengths past n_s, end_voiced /
end_len with zero rows where no session ended, rows with their ordinals.
"""
import numpy as np

from stream_scores_reference import delay_pad, final_mask, flush_rows_pad
from test_stream_segments_cpu import StreamSegModel

NO_HOP = 254  # VAD_LABEL_NO_HOP: what the sessions hop kernel leaves in a label row the stream has no hop in


class OpSegModel(StreamSegModel):
    """StreamSegModel with an operating point: the blocks hold scores (`on`
    set) or labels, and window d is decided by the clip chain hysteresis ->
    smooth -> dilate -> close(j) over what has been seen, followed by windows
    that can never be active -- or, once the flush has begun and the window
    count N is known, over exactly the N windows (the padded ends stop at
    N - 1)."""

    def __init__(self, n_streams, L, H, max_gap=0, min_run=0, active=1, dtype=np.float32, fill=0, pad=(0, 0),
                 on=None, off=None):
        super().__init__(n_streams, L, H, max_gap, min_run, active, dtype, fill)
        self.pad, self.on, self.off = pad, on, (on if off is None else off)
        self.D = delay_pad(max_gap, min_run, L, H, pad)
        self.F = flush_rows_pad(max_gap, min_run, L, H, pad)
        self.x = [[] for _ in range(n_streams)]  # the real windows: scores or labels

    def _mask(self, x):
        x = np.array(x, dtype=np.float32 if self.on is not None else np.uint8)
        return final_mask(x, self.L, self.H, self.g, self.m, self.pad, self.on, self.off, self.active)

    def _hop(self, s, label, samples, out_row):
        if self.t >= 5 and label is not None:
            self.x[s].append(label)
        return super()._hop(s, None, samples, out_row)  # self.a only counts the windows, flush windows included

    def _decide(self, s, d):
        x, n = self.x[s], len(self.x[s])
        if len(self.a[s]) > n:  # flushing: N = n
            return int(self._mask(x)[d]) if d < n else 0
        never = [np.nan if self.on is not None else 255] * (self.D + self.pad[1] + 2)
        return int(self._mask(x + never)[d])


class SessionsSegModel:
    """S streams.  push(block (k, S), hops (k, S, H) or None, hop_counts (S,),
    restart (S,)) -> (voiced (k, S, H) or None, voiced_len (k, S), end_voiced
    (F, S, H) or None, end_len (F, S)); elements no prefix covers hold `fill`.
    rows[s]: every (ordinal, start, end) appended so far, in order (found[s] =
    len(rows[s])).  log[s]: per session begun, a dict with its ordinal, the
    block values and samples it consumed and its voiced chunks in order (push
    rows, then end rows) -- what the per-session comparisons read."""

    def __init__(self, n_streams, L, H, max_gap=0, min_run=0, active=1, dtype=np.float32, fill=0, pad=None, on=None,
                 off=None):
        self.S, self.L, self.H, self.dtype, self.fill = n_streams, L, H, dtype, fill
        op = pad is not None or on is not None
        kw = dict(max_gap=max_gap, min_run=min_run, active=active, dtype=dtype, fill=fill)
        if op:
            kw.update(pad=pad or (0, 0), on=on, off=off)
        self._new = lambda: (OpSegModel if op else StreamSegModel)(1, L, H, **kw)
        self.cur = [self._new() for _ in range(n_streams)]
        self.F = self.cur[0].F
        self.ordinal = [0] * n_streams
        self.ended = [False] * n_streams
        self.rows = [[] for _ in range(n_streams)]
        self._taken = [0] * n_streams
        self.log = [[self._session(0)] for _ in range(n_streams)]

    @staticmethod
    def _session(ordinal):
        return dict(ordinal=ordinal, x=[], hops=[], voiced=[], ended=False)

    def _collect(self, s):
        rows = self.cur[s].rows[0]
        self.rows[s] += [(self.ordinal[s],) + r for r in rows[self._taken[s]:]]
        self._taken[s] = len(rows)

    def _chunks(self, s, v, n):
        if v is not None:
            self.log[s][-1]["voiced"] += [v[k, 0, :n[k, 0]].copy() for k in range(len(n))]

    def _end(self, s, audio, end_voiced, end_len):
        """Flush stream s's running model into column s of the end outputs."""
        before = len(self.rows[s])
        v, n = self.cur[s].flush(audio)
        end_len[:, s] = n[:, 0]
        if audio:
            end_voiced[:, s] = v[:, 0]
        self._chunks(s, v, n)
        self._collect(s)
        self.log[s][-1].update(ended=True, end_rows=len(self.rows[s]) - before)  # > 0: cut while a segment was open

    def push(self, block, hops, hop_counts, restart):
        block = np.asarray(block)
        k, audio = block.shape[0], hops is not None
        voiced = np.full((k, self.S, self.H), self.fill, dtype=self.dtype) if audio else None
        vlen = np.zeros((k, self.S), dtype=np.int32)
        end_voiced = np.full((self.F, self.S, self.H), self.fill, dtype=self.dtype) if audio else None
        end_len = np.zeros((self.F, self.S), dtype=np.int32)
        for s in range(self.S):
            n_s = min(max(int(hop_counts[s]), 0), k)
            if restart[s]:
                if not self.ended[s] and self.cur[s].t > 0:
                    self._end(s, audio, end_voiced, end_len)
                self.ordinal[s] += 1
                self.cur[s], self._taken[s], self.ended[s] = self._new(), 0, False
                self.log[s].append(self._session(self.ordinal[s]))
            if self.ended[s] or n_s == 0:
                continue
            v, n = self.cur[s].push(block[:n_s, s:s + 1], hops[:n_s, s:s + 1] if audio else None)
            vlen[:n_s, s] = n[:, 0]
            if audio:
                voiced[:n_s, s] = v[:, 0]
            self._chunks(s, v, n)
            self._collect(s)
            self.log[s][-1]["x"] += block[:n_s, s].tolist()
            if audio:
                self.log[s][-1]["hops"] += [hops[i, s].copy() for i in range(n_s)]
        return voiced, vlen, end_voiced, end_len

    def flush(self, audio=True):
        """The plain flush entry on a sessions state: every live stream ends."""
        voiced = np.full((self.F, self.S, self.H), self.fill, dtype=self.dtype) if audio else None
        vlen = np.zeros((self.F, self.S), dtype=np.int32)
        for s in range(self.S):
            if not self.ended[s]:
                self._end(s, audio, voiced, vlen)
                self.ended[s] = True
        return voiced, vlen

    def table(self, s):
        return np.array([r[1:] for r in self.rows[s]], dtype=np.int64).reshape(-1, 2)

    def table_session(self, s):
        return np.array([r[0] for r in self.rows[s]], dtype=np.int32)

    def sessions(self, s):
        """The sessions of stream s that consumed a hop or were ended."""
        return [g for g in self.log[s] if g["x"] or g["ended"]]


def session_clip(sess, L, H, dtype):
    """A session's equivalent clip: a zero carry, then its hops."""
    parts = [np.zeros(L - H, dtype=dtype)] + [np.asarray(h, dtype=dtype) for h in sess["hops"]]
    return np.concatenate(parts)


# ---------------------------------------------------------------------------
# workloads
# ---------------------------------------------------------------------------
HOPS = 60  # about this many block rows per stream


def schedule(S, K, seed):
    """(B, S) int32 hop counts in -1 .. K + 1 (both clamps are met) and (B, S)
    uint8 restart flags, B = ceil(HOPS / K) blocks.  Random, with these
    planted (S >= 5):
      stream 0  never used (count 0) for the first third, then a restart with
                a full count: a restart on a never-used stream;
      stream 1  stalls for 4 consecutive blocks in the middle, and is restarted
                once with count 0;
      stream 2  restarts every other block with 1 or 2 hops: sessions shorter
                than 5 hops;
      stream 3  full counts, restarted about every 14 hops: whole sessions."""
    rng = np.random.default_rng(seed)
    B = -(-HOPS // K)
    counts = rng.integers(-1, K + 2, size=(B, S)).astype(np.int32)
    restart = (rng.random((B, S)) < 0.08).astype(np.uint8)
    third = B // 3
    counts[:third, 0], restart[:third, 0] = 0, 0
    counts[third, 0], restart[third, 0] = K, 1
    mid = B // 2
    counts[mid:mid + 4, 1], restart[mid:mid + 4, 1] = 0, 0
    counts[mid + 4, 1], restart[mid + 4, 1] = 0, 1
    counts[:, 2] = rng.integers(1, min(K, 2) + 1, size=B)
    restart[:, 2] = np.arange(B) % 2
    counts[:, 3] = K
    restart[:, 3] = (np.arange(B) % max(14 // K, 1) == 0) & (np.arange(B) > 0)
    return counts, restart


def taken(counts, K):
    return np.clip(counts, 0, K)


def block_values(S, K, counts, seed, scores=False, active=1, on=0.6, off=0.4, restart=None):
    """(B, K, S) block values: per stream a walk over the rows it consumes,
    mostly active (runs of mean 6 against gaps of mean 2).  Labels: `active`
    against 0 / 2.  Scores: above `on`, below `off`, the band between them
    (which keeps the last decision) and NaN (inactive).  A row the stream has
    no hop in holds what would count as active if it were read -- the count
    is the definition, not the value found there.  Scores with `restart`
    given: around every restart of stream 3 (full counts) the last score of
    the old session is 1 and the first window of the new one (its sixth hop)
    lies in the band, so a hysteresis bit that leaked across the restart
    would show as an active window."""
    rng = np.random.default_rng(seed + 1)
    B = counts.shape[0]
    x = np.full((B, K, S), 1.0 if scores else active, dtype=np.float32 if scores else np.uint8)
    n = taken(counts, K)
    for s in range(S):
        v, left = 1, 0
        for b in range(B):
            for k in range(n[b, s]):
                if left == 0:
                    v = 1 - v
                    left = int(rng.geometric(1 / 6.0 if v else 1 / 2.0))
                left -= 1
                if scores:
                    u = rng.random()
                    if v:
                        x[b, k, s] = on + (1 - on) * u if u < 0.7 else off + (on - off) * u  # in the band: stays 1
                    else:
                        x[b, k, s] = np.nan if u < 0.2 else off * u * 0.99
                else:
                    x[b, k, s] = active if v else (0 if rng.random() < 0.6 else 2)
    if scores and restart is not None and S > 3:
        for b in np.flatnonzero(restart[:, 3]):
            first = b * K + 5  # the new session's window 0, as a row of stream 3's column
            if b > 0 and first < B * K and not restart[b + 1:first // K + 1, 3].any():
                x[b - 1, K - 1, 3] = 1.0
                x[first // K, first % K, 3] = (on + off) / 2
    return x


def audio_blocks(S, K, B, H, dtype, seed):
    rng = np.random.default_rng(seed + 2)
    if dtype == np.float32:
        a = rng.standard_normal((B, K, S, H)).astype(np.float32)
        bits = a.reshape(-1).view(np.uint32)
        k = rng.integers(0, bits.size, size=max(bits.size // 50, 4))
        bits[k[0::2]] = 0x7FC00001  # a NaN with a payload: bits are copied, never converted
        bits[k[1::2]] = 0x80000000  # -0.0
        return a
    return rng.integers(-32768, 32768, size=(B, K, S, H)).astype(np.int16)


SHAPES = [(5, 1), (5, 3), (9, 1), (9, 3)]  # S = 9: a partial last workgroup of 4 waves
CAPACITY = 3  # of the tables in the tests: some stream finds more rows than that
SESSION_FRAMINGS = [(400, 160), (8, 3), (5, 5), (400, 400)]
SESSION_PARAMS = [(0, 0), (2, 3), (7, 5)]  # of test_stream_segments_cpu.PARAMS
FORMS = {"labels": dict(), "op_labels": dict(pad=(2, 1)), "op_scores": dict(on=0.6, off=0.4)}
DTYPES = [np.float32, np.int16, None]  # None: events only


def shape_for(framing, params, form, dtype):
    """The (S, K) a device-against-model case runs at.  The cases rotate
    through SHAPES, they are not crossed with them: a given (framing, params,
    form, dtype) meets one shape.  Every form and dtype at S = 9 (the partial
    last workgroup) with both K is test_every_form_in_the_partial_workgroup
    of the GPU tests, at one framing and one pair of parameters."""
    i = SESSION_FRAMINGS.index(framing) * 7 + SESSION_PARAMS.index(params) * 3 + list(FORMS).index(form) + \
        DTYPES.index(dtype)
    return SHAPES[i % len(SHAPES)]


def seed_of(S, K):
    """The workload seeds, chosen on the CPU (tests/test_stream_segments_sessions_cpu.py
    asserts that every case the GPU tests rely on occurs at these)."""
    return {(5, 1): 2, (5, 3): 1, (9, 1): 1, (9, 3): 6}[(S, K)]


def run_model(model, x, hops, counts, restart):
    """Every block through the model; the per-block outputs."""
    return [model.push(x[b], None if hops is None else hops[b], counts[b], restart[b]) for b in range(len(x))]
