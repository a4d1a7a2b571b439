"""Models of the streaming segmenter with an operating point (include/vad_amd.h,
"The operating point in the streaming segmenter"): hysteresis on scores and
padding of the smoothed runs, online, against the clip chain.

  clip_chain   the offline answer, from the models the clip path is tested
               with: scores_reference.hysteresis -> test_segments_cpu's
               model_smooth -> scores_reference.dilate -> model_close(j) ->
               model_rows.
  OnlineOp     the online machine, restated window by window in plain NumPy
               over B independent streams (no tiles, no device types, nothing
               of the kernel's layout): per stream the hysteresis bit, the
               candidate run, the queue of padded segments, the decided window
               d = n - D.  Every decision about window d is taken when window
               d + D arrives and never revised: `c` records it, `rows` the
               finished segments, `vlen` each hop's voiced prefix length.

  D = max_gap + max(min_run, 1) + (L // H - 1) + 1 + pad_before
  F = D + 2 + ceil(L / H) flush hops
"""
import numpy as np

from scores_reference import dilate, hysteresis
from test_segments_cpu import model_close, model_rows, model_smooth


def delay_pad(max_gap, min_run, L, H, pad):
    return max_gap + max(min_run, 1) + (L // H - 1) + 1 + pad[0]


def flush_rows_pad(max_gap, min_run, L, H, pad):
    return delay_pad(max_gap, min_run, L, H, pad) + 2 + -(-L // H)


def decisions(x, on=None, off=None, active=1):
    """0 / 1 per window: hysteresis of scores, or label == active."""
    if on is None:
        return (np.asarray(x) == active).astype(np.uint8)
    return hysteresis(x, on, on if off is None else off)


def final_mask(x, L, H, max_gap, min_run, pad, on=None, off=None, active=1):
    b = model_smooth(decisions(x, on, off, active), max_gap, min_run)
    return model_close(dilate(b, 1, pad[0], pad[1]), L // H - 1)


def clip_chain(x, n_samples, L, H, max_gap, min_run, pad, on=None, off=None, active=1):
    """((k, 3) rows (start, end, offset), voiced total) of one clip's windows x."""
    return model_rows(final_mask(x, L, H, max_gap, min_run, pad, on, off, active), n_samples, L, H)


def expected_vlen(mask, n_hops, L, H, D):
    """Hop t's voiced prefix length from a stream's final mask: d = t - 5 - D,
    e the last active window <= d, clamp((e - d) H + L, 0, H)."""
    out = np.zeros(n_hops, dtype=np.int64)
    e = -1
    for t in range(n_hops):
        d = t - 5 - D
        if d < 0:
            continue
        if d < len(mask) and mask[d]:
            e = d
        if e >= 0:
            out[t] = min(max((e - d) * H + L, 0), H)
    return out


class OnlineOp:
    """B streams in lockstep.  run(x, lengths): x (T, B) scores (float32, with
    `on`) or labels (uint8), window w of stream b in row w; stream b has
    lengths[b] windows (hops 0..4 carry no window), is flushed right after its
    last one and fed inactive flush hops from then on.  Afterwards
      c        (decided windows, B) uint8: row d is the decision about window d,
               taken when window d + D arrived
      rows[b]  [(start, end)] in samples, in the order they finished
      vlen     (hops, B) voiced prefix lengths; hop t's prefix starts at
               sample (t - 5 - D + 2) H
      max_queue  the most segments ever queued at once."""

    def __init__(self, B, L, H, max_gap=0, min_run=0, pad=(0, 0), on=None, off=None, active=1):
        self.B, self.L, self.H, self.g, self.m1 = B, L, H, max_gap, max(min_run, 1)
        self.pb, self.pa = pad
        self.on = None if on is None else np.float32(on)
        self.off = None if on is None else np.float32(on if off is None else off)
        self.active, self.j = active, L // H - 1
        self.D = delay_pad(max_gap, min_run, L, H, pad)
        self.F = flush_rows_pad(max_gap, min_run, L, H, pad)
        z = lambda: np.zeros(B, dtype=np.int64)
        self.h, self.cand, self.conf, self.r0, self.r1, self.nq, self.e1 = z(), z(), z(), z(), z(), z(), z()
        self.q = np.zeros((B, 4, 2), dtype=np.int64)
        self._c = []
        self.rows = [[] for _ in range(B)]
        self.max_queue = 0

    def _oldest(self):
        i = np.maximum(self.nq - 1, 0)
        o = self.q[np.arange(self.B), i]
        has = self.nq > 0
        return np.where(has, o[:, 0], 0), np.where(has, o[:, 1], -1)

    def _hop(self, t, x, have):
        """x (B,), have (B,) bool: the stream still gets input at this hop."""
        L, H, D = self.L, self.H, self.D
        out = np.zeros(self.B, dtype=np.int64)
        if t < 5:
            return out
        n = t - 5
        if self.on is not None:
            with np.errstate(invalid="ignore"):
                s = x.astype(np.float32)
                up = have & (s >= self.on)
                down = have & ~up & ~(s >= self.off)  # below off, or NaN
            self.h = np.where(up, 1, np.where(down, 0, self.h))
            act = have & (self.h == 1)
        else:
            act = have & (x == self.active)
        start = act & (self.cand == 0)
        self.cand[start], self.conf[start], self.r0[start] = 1, 0, n
        self.r1[act] = n
        grow = act & (self.conf == 1)
        self.q[grow, 0, 1] = n + self.pa
        newc = act & ~grow & (self.r1 - self.r0 + 1 >= self.m1)
        self.conf[newc] = 1
        join = newc & (self.nq > 0) & (self.r0 - self.pb - self.q[:, 0, 1] - 1 <= self.j)
        self.q[join, 0, 1] = n + self.pa
        push = newc & ~join
        assert not (push & (self.nq >= 4)).any(), "the queue of four overflowed"
        self.q[push, 1:] = self.q[push, :-1]
        self.q[push, 0, 0] = np.maximum(self.r0[push] - self.pb, 0)
        self.q[push, 0, 1] = n + self.pa
        self.nq[push] += 1
        self.max_queue = max(self.max_queue, int(self.nq.max()))
        drop = ~act & (self.cand == 1) & (n - self.r1 > self.g)
        self.cand[drop], self.conf[drop] = 0, 0
        d = n - D
        if d < 0:
            return out
        o0, o1 = self._oldest()
        fin = (self.nq > 0) & (o1 < d)
        for b in np.flatnonzero(fin):
            assert o1[b] == d - 1  # a segment finishes exactly one window after its end
            self.rows[b].append((int(o0[b] + 2) * H, int(o1[b] + 2) * H + L))
        self.nq[fin] -= 1
        o0, o1 = self._oldest()
        inside = (self.nq > 0) & (o0 <= d) & (d <= o1)
        self.e1[inside] = d + 1
        self._c.append(inside.astype(np.uint8))
        v = (self.e1 - 1 - d) * H + L
        return np.where(self.e1 > 0, np.clip(v, 0, H), 0)

    def run(self, x, lengths):
        x = np.asarray(x)
        lengths = np.asarray(lengths, dtype=np.int64)
        hops = int(lengths.max()) + 5 + self.F
        vlen = np.zeros((hops, self.B), dtype=np.int64)
        pad_row = np.zeros(self.B, dtype=x.dtype)
        for t in range(hops):
            # the flush of a stream: its window count N is known, the newest
            # segment's padded end stops at N - 1
            fl = (t == lengths + 5) & (self.nq > 0)
            self.q[fl, 0, 1] = np.minimum(self.q[fl, 0, 1], lengths[fl] - 1)
            w = t - 5
            vlen[t] = self._hop(t, x[w] if 0 <= w < x.shape[0] else pad_row, w < lengths)
        self.vlen = vlen
        self.c = np.stack(self._c) if self._c else np.zeros((0, self.B), np.uint8)
        return self
