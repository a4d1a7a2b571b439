"""Streaming segments (include/vad_amd.h, "Streaming segments"): the online
NumPy model that tests/test_gpu_stream_segments.py compares the kernel with,
pinned here against the offline models of tests/test_segments_cpu.py; the
delay formula by brute force; promptness; and the library's new symbols and
sizing entries (no GPU here).

The model is written from the definitions, not from the kernel's state
machine: per stream it keeps every label and sample seen, and decides window
d = t - 5 - D at hop t by running the offline stages (model_close /
model_smooth) over the labels seen so far -- only over a tail of them, long
enough that the cut cannot reach window d (3 D + 8 windows); the comparison
with model_segments on whole sequences below is what says that it is.

  equivalent clip: L - H carried samples, then every hop; hop t's label is
  window t - 5 (t >= 5; earlier label bytes are ignored).
  D = max_gap + max(min_run, 1) + (L // H - 1) + 1.
  Hop t's output row: the voiced prefix of the slab [(d+2)H, (d+3)H), length
  clamp((e+2)H + L - (d+2)H, 0, H), e the last window <= d of the final mask.
  A segment [i0, i1] is appended at the hop whose d is i1 + 1.
  flush: F = D + 2 + ceil(L / H) more hops of inactive windows, no samples.
"""
import itertools
import os
import re

import numpy as np
import pytest

from test_segments_cpu import model_close, model_rows, model_segments, model_smooth, model_voiced

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FRAMINGS = [(400, 160), (400, 400), (8, 3), (5, 5)]
BLOCKS = [1, 3, 8]
PARAMS = [(0, 0), (0, 1), (3, 0), (2, 3), (7, 5)]


def seg_delay(max_gap, min_run, L, H):
    return max_gap + max(min_run, 1) + (L // H - 1) + 1


def flush_rows(max_gap, min_run, L, H):
    return seg_delay(max_gap, min_run, L, H) + 2 + -(-L // H)


def final_mask(a, max_gap, min_run, L, H):
    """The mask whose runs vad_label_segments turns into rows, of 0/1 windows a."""
    return model_close(model_smooth(a, max_gap, min_run), L // H - 1)


class StreamSegModel:
    """S streams; push(label_block (K, S) uint8, hop_block (K, S, H) or None)
    -> (voiced (K, S, H), voiced_len (K, S) int32) with the elements past each
    prefix left at `fill`; flush() -> the same with F rows.  rows[s]: the
    (start, end) pairs appended so far (all of them: found[s] = len(rows[s]),
    the device writes the first `capacity`)."""

    def __init__(self, n_streams, L, H, max_gap=0, min_run=0, active=1, dtype=np.float32, fill=0, carry=None):
        self.S, self.L, self.H, self.g, self.m, self.active = n_streams, L, H, max_gap, min_run, active
        self.D = seg_delay(max_gap, min_run, L, H)
        self.F = flush_rows(max_gap, min_run, L, H)
        self.dtype, self.fill = dtype, fill
        self.t = 0
        self.a = [[] for _ in range(n_streams)]      # windows seen, 0 / 1
        self.c = [[] for _ in range(n_streams)]      # decided windows of the final mask
        self.e = [-1] * n_streams
        self.rows = [[] for _ in range(n_streams)]
        self.run0 = [None] * n_streams               # start of the decided run still open
        if carry is None:
            carry = np.zeros((n_streams, L - H), dtype=dtype)
        self.clip = [list(np.asarray(carry[s]).tolist()) for s in range(n_streams)]
        self.clip_arr = None

    def _decide(self, s, d):
        """c[d] of stream s from the windows seen so far (inactive ones follow)."""
        a = self.a[s]
        lo = max(0, d - 2 * self.D - 7)
        tail = np.array(a[lo:d + self.D + 1], dtype=np.uint8)
        if d - lo >= len(tail):
            return 0
        return int(final_mask(tail, self.g, self.m, self.L, self.H)[d - lo])

    def _hop(self, s, label, samples, out_row):
        L, H, t = self.L, self.H, self.t
        if t >= 5:
            self.a[s].append(1 if (label is not None and int(label) == self.active) else 0)
        if samples is not None:
            self.clip[s].extend(np.asarray(samples).tolist())
        d = t - 5 - self.D
        if d < 0:
            return 0
        c = self._decide(s, d)
        self.c[s].append(c)
        if c:
            self.e[s] = d
            if self.run0[s] is None:
                self.run0[s] = d
        elif self.run0[s] is not None:
            self.rows[s].append(((self.run0[s] + 2) * H, (d - 1 + 2) * H + L))
            self.run0[s] = None
        e = self.e[s]
        n = 0 if e < 0 else min(max((e + 2) * H + L - (d + 2) * H, 0), H)
        if n and out_row is not None:
            p = (d + 2) * H
            assert p + n <= len(self.clip[s])  # never past the clip's end
            out_row[:n] = np.array(self.clip[s][p:p + n], dtype=self.dtype)
        return n

    def _block(self, K, labels, hops, audio):
        voiced = np.full((K, self.S, self.H), self.fill, dtype=self.dtype) if audio else None
        vlen = np.zeros((K, self.S), dtype=np.int32)
        for k in range(K):
            for s in range(self.S):
                vlen[k, s] = self._hop(s, None if labels is None else labels[k, s],
                                       None if hops is None else hops[k, s], voiced[k, s] if audio else None)
            self.t += 1
        return voiced, vlen

    def push(self, label_block, hop_block=None):
        label_block = np.asarray(label_block)
        return self._block(label_block.shape[0], label_block, hop_block, hop_block is not None)

    def flush(self, audio=True):
        return self._block(self.F, None, None, audio)

    def table(self, s):
        return np.array(self.rows[s], dtype=np.int64).reshape(-1, 2)


# ---------------------------------------------------------------------------
# label families and audio shared with the GPU test
# ---------------------------------------------------------------------------
def geometric_runs(rng, n, mean):
    out = np.zeros(n, dtype=np.uint8)
    pos, v = 0, int(rng.integers(2))
    while pos < n:
        l = int(rng.geometric(1.0 / mean))
        out[pos:pos + l] = v
        pos, v = pos + l, 1 - v
    return out


FAMILIES = ["zeros", "ones", "alternating", "geo2", "geo20", "run_at_end", "gap_at_end"]


def family(name, n, rng):
    """n windows, 1 = active; the inactive windows of the random families are 0 or 2."""
    if name == "zeros":
        return np.zeros(n, dtype=np.uint8)
    if name == "ones":
        return np.ones(n, dtype=np.uint8)
    if name == "alternating":
        return (np.arange(n) % 2).astype(np.uint8)
    a = geometric_runs(rng, n, 20 if name == "geo20" else 2)
    if name in ("run_at_end", "gap_at_end") and n:
        l = int(rng.integers(1, 8))
        a[max(n - l, 0):] = 1 if name == "run_at_end" else 0
        if n - l - 1 >= 0:
            a[n - l - 1] = 0 if name == "run_at_end" else 1
    a[(a == 0) & (rng.random(n) < 0.3)] = 2
    return a


def stream_labels(T, rng, families=FAMILIES, head=255):
    """(T, S) label bytes: rows t < 5 hold `head` (or random bytes for
    head="garbage"), row t >= 5 window t - 5 of each family."""
    n = max(T - 5, 0)
    lab = np.stack([family(f, n, rng) for f in families], axis=1) if n else np.zeros((0, len(families)), np.uint8)
    first = min(T, 5)
    top = rng.integers(0, 256, size=(first, len(families))).astype(np.uint8) if head == "garbage" else \
        np.full((first, len(families)), head, dtype=np.uint8)
    return np.concatenate([top, lab], axis=0)


def stream_audio(T, S, H, dtype, rng):
    if dtype == np.float32:
        a = rng.standard_normal((T, S, H)).astype(np.float32)
        bits = a.reshape(-1).view(np.uint32)
        if bits.size:
            k = rng.integers(0, bits.size, size=max(bits.size // 50, 4))
            bits[k[0::2]] = 0x7FC00001  # a NaN with a payload: bits are copied, never converted
            bits[k[1::2]] = 0x80000000  # -0.0
        return a
    return rng.integers(-32768, 32768, size=(T, S, H)).astype(np.int16)


def equivalent_clip(carry, hops):
    """carry (S, L-H), hops (T, S, H) -> (S, L-H + T*H)."""
    return np.concatenate([carry, np.transpose(hops, (1, 0, 2)).reshape(hops.shape[1], -1)], axis=1)


def run_blocks(model, labels, hops, K):
    """Feed T hops in blocks of K (the last one shorter); the concatenated outputs."""
    voiced, vlen = [], []
    for t0 in range(0, labels.shape[0], K):
        v, n = model.push(labels[t0:t0 + K], None if hops is None else hops[t0:t0 + K])
        voiced.append(v), vlen.append(n)
    return voiced, vlen


def packed(voiced, vlen, s):
    """Stream s's voiced samples: the prefixes of its rows, in order."""
    parts = [v[k, s, :n[k, s]] for v, n in zip(voiced, vlen) for k in range(n.shape[0])]
    return np.concatenate(parts) if parts else np.zeros(0)


def lengths_for(D):
    return [0, 1, 5, 6, 7, 6 + D, 300]


# ---------------------------------------------------------------------------
# the model against the offline models
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", BLOCKS)
@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("framing", FRAMINGS)
def test_model_matches_offline_after_flush(framing, params, K):
    L, H = framing
    g, m = params
    D = seg_delay(g, m, L, H)
    rng = np.random.default_rng(1000 * L + 10 * H + 100 * g + m)
    S = len(FAMILIES)
    for T in lengths_for(D):
        labels = stream_labels(T, rng, head="garbage" if T % 2 else 255)
        dtype = np.int16 if (T + K) % 2 else np.float32
        hops = stream_audio(T, S, H, dtype, rng)
        carry = np.zeros((S, L - H), dtype=dtype)
        model = StreamSegModel(S, L, H, g, m, dtype=dtype)
        voiced, vlen = run_blocks(model, labels, hops, K)
        fv, fn = model.flush()
        assert fv.shape == (flush_rows(g, m, L, H), S, H)
        clip = equivalent_clip(carry, hops)
        assert clip.shape[1] == L - H + T * H
        for s in range(S):
            where = (framing, params, K, T, FAMILIES[s])
            rows, total = model_segments(labels[5:, s], clip.shape[1], L, H, g, m)
            assert np.array_equal(model.table(s), rows[:, :2]), where
            got = packed(voiced + [fv], vlen + [fn], s)
            want = model_voiced(clip[s], rows)
            assert len(got) == total, where
            assert np.array_equal(got.astype(dtype).view(np.uint8), want.view(np.uint8)), where
        # a flushed stream decided everything: nothing more would come
        assert all(r is None for r in model.run0)


def test_model_events_only_gives_the_same_table():
    rng = np.random.default_rng(5)
    labels = stream_labels(120, rng)
    hops = stream_audio(120, len(FAMILIES), 3, np.int16, rng)
    a = StreamSegModel(len(FAMILIES), 8, 3, 2, 3, dtype=np.int16)
    b = StreamSegModel(len(FAMILIES), 8, 3, 2, 3, dtype=np.int16)
    run_blocks(a, labels, hops, 8)
    assert b.push(labels[:64])[0] is None
    run_blocks(b, labels[64:], None, 3)
    a.flush(), b.flush(audio=False)
    for s in range(len(FAMILIES)):
        assert np.array_equal(a.table(s), b.table(s))


def test_model_active_value_and_carry():
    """active = 2, and a primed carry longer than two hops (L > 3 H): its samples can be voiced."""
    rng = np.random.default_rng(6)
    L, H, T = 9, 2, 60
    labels = stream_labels(T, rng, families=["geo2", "geo20", "ones"])
    labels[5:, 2] = 2
    hops = stream_audio(T, 3, H, np.int16, rng)
    carry = rng.integers(-9, 9, size=(3, L - H)).astype(np.int16)
    model = StreamSegModel(3, L, H, 1, 2, active=2, dtype=np.int16, carry=carry)
    voiced, vlen = run_blocks(model, labels, hops, 3)
    fv, fn = model.flush()
    clip = equivalent_clip(carry, hops)
    for s in range(3):
        rows, total = model_segments(labels[5:, s], clip.shape[1], L, H, 1, 2, active=2)
        assert np.array_equal(model.table(s), rows[:, :2])
        assert np.array_equal(packed(voiced + [fv], vlen + [fn], s), model_voiced(clip[s], rows))
    assert model.table(2)[0].tolist() == [2 * H, (T - 6 + 2) * H + L]  # from inside the carry to the clip's end


# ---------------------------------------------------------------------------
# the delay: c[i] does not depend on anything after window i + D
# ---------------------------------------------------------------------------
def test_delay_formula_by_brute_force():
    """Every label string of length 13, max_gap, min_run <= 3, j <= 2: for
    every cut n, the string with everything from window n on made inactive
    (which is what "nothing more is known" means: inactive windows follow
    forever) has the mask of the whole string on every window i <= n - 1 - D.
    If every continuation agrees with that one, they agree with each other."""
    N = 13
    v = np.arange(1 << N)
    bits = ((v[:, None] >> (N - 1 - np.arange(N))[None, :]) & 1).astype(np.uint8)  # window 0 is the top bit
    memo = {}

    def stage(kind, p, row):
        if p == 0 or (kind == "open" and p == 1):
            return row
        key = (kind, p, row.tobytes())
        if key not in memo:
            memo[key] = model_close(row, p) if kind != "open" else model_smooth(row, 0, p)
        return memo[key]

    need = {}
    for g in range(4):
        for m in range(4):
            for j in range(3):
                D = g + max(m, 1) + j + 1
                c = np.stack([stage("close", j, stage("open", m, stage("close", g, row))) for row in bits])
                worst = 0
                for n in range(1, N):
                    cut = (v >> (N - n)) << (N - n)
                    diff = c[cut][:, :n] != c[:, :n]
                    first = np.where(diff.any(axis=1), diff.argmax(axis=1), n)
                    bad = np.flatnonzero(first <= n - 1 - D)
                    assert len(bad) == 0, (g, m, j, n, bits[bad[0]].tolist())
                    worst = max(worst, int((n - first).max()))  # windows after i that c[i] waited for
                need[(g, m, j)] = (worst, D)
    assert all(w <= D for w, D in need.values())


# ---------------------------------------------------------------------------
# promptness
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("params", PARAMS)
def test_rows_come_promptly_and_are_offline_rows(params):
    g, m = params
    L, H = 8, 3
    D = seg_delay(g, m, L, H)
    rng = np.random.default_rng(77 + g + 10 * m)
    T = 200
    labels = stream_labels(T, rng)
    S = labels.shape[1]
    model = StreamSegModel(S, L, H, g, m)
    final = [model_segments(labels[5:, s], L - H + T * H, L, H, g, m)[0][:, :2] for s in range(S)]
    for t0 in range(0, T, 3):
        model.push(labels[t0:t0 + 3])
        last = min(t0 + 3, T) - 1 - 5  # the last window seen
        for s in range(S):
            got = model.table(s)
            rows = final[s]
            assert np.array_equal(got, rows[:len(got)]), (params, t0, s)  # offline rows, in order
            i1 = (rows[:, 1] - L) // H - 2
            assert len(got) >= int((i1 + 1 + D <= last).sum()), (params, t0, s)
    assert sum(len(model.table(s)) for s in range(S)) > 3  # rows did come before any flush


# ---------------------------------------------------------------------------
# the library: symbols, sizing entries, header and symbol map
# ---------------------------------------------------------------------------
SYMBOLS = ["vad_stream_seg_delay", "vad_stream_seg_flush_rows", "vad_stream_seg_state_bytes",
           "vad_stream_seg_history_elems", "vad_stream_segments", "vad_stream_segments_f32",
           "vad_stream_segments_i16", "vad_stream_segments_flush", "vad_stream_segments_flush_f32",
           "vad_stream_segments_flush_i16"]


def test_library_exports_the_streaming_segment_entries():
    from vad_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(REPO, "include", "vad_amd.h")).read()
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\(" % name, header), name
        assert name in integration, name
    for (g, m), (L, H) in itertools.product(PARAMS + [(30, 10)], FRAMINGS + [(400, 100)]):
        D = seg_delay(g, m, L, H)
        assert lib.vad_stream_seg_delay(g, m, L, H) == D
        assert lib.vad_stream_seg_flush_rows(g, m, L, H) == flush_rows(g, m, L, H)
        for S, K in ((1, 1), (65, 8), (512, 32)):
            assert lib.vad_stream_seg_history_elems(S, K, g, m, L, H) >= S * ((D + 3) * H + L + K * H)
    assert lib.vad_stream_seg_state_bytes(0) == 0
    assert lib.vad_stream_seg_state_bytes(3) == 3 * lib.vad_stream_seg_state_bytes(1) > 0
    assert lib.vad_stream_seg_delay(0, 0, 400, 0) == -1 and lib.vad_stream_seg_delay(-1, 0, 400, 160) == -1
    assert lib.vad_stream_seg_delay(0, 0, 160, 400) == -1


def test_python_argument_checks():
    import torch
    from vad_amd.stream_segments import StreamSegmenter
    with pytest.raises(ValueError):
        StreamSegmenter(4, max_gap=-1, device=torch.device("cpu"))
    with pytest.raises(ValueError):
        StreamSegmenter(4, active=255, device=torch.device("cpu"))
    with pytest.raises(ValueError):
        StreamSegmenter(4, capacity=-1, device=torch.device("cpu"))
    with pytest.raises(ValueError):
        StreamSegmenter(4, hops_per_step=0, device=torch.device("cpu"))
    with pytest.raises(TypeError):
        StreamSegmenter(4, audio_dtype=torch.float64, device=torch.device("cpu"))
