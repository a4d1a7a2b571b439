"""The operating point on the live path, without a GPU: the online model of
tests/stream_scores_reference.py against the clip chain -- exhaustively on
short sequences (which is what proves the delay formula: the model decides
window d when window d + D arrives and never looks again), on random score
walks with ties and NaNs -- and the library's sizing entries and refusals,
all of which come before the first device call."""
import itertools
import os
import re

import numpy as np
import pytest

from scores_reference import dilate, hysteresis
from stream_scores_reference import (OnlineOp, clip_chain, delay_pad, expected_vlen, final_mask, flush_rows_pad)
from test_segments_cpu import model_close, model_smooth
from test_stream_segments_cpu import flush_rows, seg_delay

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GAPS, RUNS = [0, 1, 2], [0, 1, 3]
PADS = [(0, 0), (1, 0), (0, 2), (2, 3), (15, 15)]
FRAMINGS = [(400, 160), (64, 16)]  # j = frame_size // hop - 1 = 1 and 3


# ---------------------------------------------------------------------------
# the clip chain over many sequences of one length at once (rows of a 2-D
# array), pinned to the per-sequence models below
# ---------------------------------------------------------------------------
def _prev_next(a):
    n = a.shape[1]
    idx = np.arange(n)[None, :]
    prev = np.maximum.accumulate(np.where(a, idx, -1), axis=1)
    nxt = np.minimum.accumulate(np.where(a, idx, 2 * n)[:, ::-1], axis=1)[:, ::-1]
    return idx, prev, nxt, n


def v_close(a, g):
    idx, prev, nxt, n = _prev_next(a)
    return a | ((prev >= 0) & (nxt < n) & (nxt - prev - 1 <= g))


def v_open(a, m):
    idx, pz, nz, n = _prev_next(~a)  # the zeros around a run
    nz = np.where(nz >= n, n, nz)
    return a & (nz - pz - 1 >= m)


def v_dilate(a, pb, pa):
    idx, prev, nxt, n = _prev_next(a)
    return ((prev >= 0) & (idx - prev <= pa)) | ((nxt < n) & (nxt - idx <= pb))


def v_final(a, j, g, m, pad):
    return v_close(v_dilate(v_open(v_close(a, g), m), *pad), j)


def all_sequences(n):
    v = np.arange(1 << n)
    return ((v[:, None] >> (n - 1 - np.arange(n))[None, :]) & 1).astype(bool).reshape(1 << n, n)


def test_vectorised_chain_is_the_models_chain():
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 12, 40):
        a = rng.random((60, n)) < 0.5
        for g, m, pad, (L, H) in itertools.product(GAPS, RUNS, PADS, FRAMINGS):
            got = v_final(a, L // H - 1, g, m, pad)
            for r in range(0, 60, 7):
                want = final_mask(a[r].astype(np.uint8), L, H, g, m, pad)
                assert np.array_equal(got[r].astype(np.uint8), want), (n, g, m, pad, L, H, r)


# ---------------------------------------------------------------------------
# exhaustive: every 0/1 sequence of length <= 12
# ---------------------------------------------------------------------------
NMAX = 12
SEQS = [all_sequences(n) for n in range(NMAX + 1)]
LENGTHS = np.concatenate([np.full(1 << n, n) for n in range(NMAX + 1)])
X = np.zeros((NMAX, len(LENGTHS)), dtype=np.float32)  # scores 0.0 / 1.0, window w in row w
_o = 0
for _n, _s in enumerate(SEQS):
    X[:_n, _o:_o + len(_s)] = _s.T
    _o += len(_s)


@pytest.mark.parametrize("framing", FRAMINGS)
@pytest.mark.parametrize("pad", PADS)
def test_online_equals_clip_chain_on_every_short_sequence(framing, pad):
    L, H = framing
    B = len(LENGTHS)
    for g, m in itertools.product(GAPS, RUNS):
        D = delay_pad(g, m, L, H, pad)
        model = OnlineOp(B, L, H, g, m, pad, on=0.5, off=0.5).run(X, LENGTHS)
        assert model.max_queue <= 3  # the queue has room for four
        hops = model.vlen.shape[0]
        # the decided mask, taken D windows behind the newest, is the clip chain's
        want = np.zeros((hops, B), dtype=np.uint8)
        o = 0
        for n, s in enumerate(SEQS):
            want[:n, o:o + len(s)] = v_final(s, L // H - 1, g, m, pad).T
            o += len(s)
        nd = model.c.shape[0]
        assert nd == hops - 5 - D and nd > NMAX
        assert np.array_equal(model.c, want[:nd]), (framing, pad, g, m)
        # voiced prefix of every hop: from e, the last active decided window
        idx = np.arange(hops)[:, None]
        e = np.maximum.accumulate(np.where(want == 1, idx, -1), axis=0)
        exp = np.zeros((hops, B), dtype=np.int64)
        d = np.arange(nd)
        ee = e[:nd]
        exp[5 + D:] = np.where(ee >= 0, np.clip((ee - d[:, None]) * H + L, 0, H), 0)
        assert np.array_equal(model.vlen, exp), (framing, pad, g, m)
        # rows and voiced sample ranges of a spread of streams, from the per-sequence models
        for b in range(g + 3 * m, B, 53):
            n = int(LENGTHS[b])
            n_samples = L - H + (n + 5) * H
            rows, total = clip_chain(X[:n, b], n_samples, L, H, g, m, pad, on=0.5, off=0.5)
            assert model.rows[b] == [tuple(r) for r in rows[:, :2].tolist()], (framing, pad, g, m, b)
            assert np.array_equal(model.vlen[:, b], expected_vlen(want[:, b], hops, L, H, D))
            assert int(model.vlen[:, b].sum()) == total
            # the prefixes are the rows' samples, in order: hop t's starts at (t - 5 - D + 2) H
            got = np.concatenate([np.arange((t - 5 - D + 2) * H, (t - 5 - D + 2) * H + model.vlen[t, b])
                                  for t in range(hops)])
            exp_s = np.concatenate([np.arange(r0, r1) for r0, r1, _ in rows.tolist()] or [np.zeros(0, np.int64)])
            assert np.array_equal(got, exp_s), (framing, pad, g, m, b)


# ---------------------------------------------------------------------------
# random score walks with ties and NaNs
# ---------------------------------------------------------------------------
def score_walks(rng, n, B, on, off):
    """(n, B) float32 random walks in [0, 1] with values exactly on, exactly
    off, just below each, and NaNs sprinkled in."""
    s = np.clip(0.5 + np.cumsum(rng.normal(0, 0.12, size=(n, B)), axis=0) % 1.0 - 0.5, 0, 1).astype(np.float32)
    s = np.abs(((s + rng.random((1, B)).astype(np.float32)) % 2.0) - 1.0).astype(np.float32)
    r = rng.random((n, B))
    s[r < 0.06] = np.float32(on)
    s[(r >= 0.06) & (r < 0.12)] = np.float32(off)
    s[(r >= 0.12) & (r < 0.15)] = np.nextafter(np.float32(on), np.float32(-1))
    s[(r >= 0.15) & (r < 0.18)] = np.nextafter(np.float32(off), np.float32(-1)) if off > 0 else np.float32(0)
    s[(r >= 0.18) & (r < 0.22)] = np.nan
    return s


@pytest.mark.parametrize("thr", [(0.6, 0.4), (0.5, 0.5), (1.0, 0.0)])
def test_online_equals_clip_chain_on_random_walks(thr):
    on, off = thr
    rng = np.random.default_rng(int(on * 100) + 7)
    n, B = 300, 6
    for (L, H), (g, m), pad in itertools.product(FRAMINGS, [(0, 0), (2, 3), (1, 1)], PADS):
        s = score_walks(rng, n, B, on, off)
        D = delay_pad(g, m, L, H, pad)
        model = OnlineOp(B, L, H, g, m, pad, on=on, off=off).run(s, np.full(B, n))
        hops = model.vlen.shape[0]
        for b in range(B):
            mask = final_mask(s[:, b], L, H, g, m, pad, on, off)
            assert np.array_equal(model.c[:n, b], mask) and not model.c[n:, b].any(), (thr, L, H, g, m, pad, b)
            rows, total = clip_chain(s[:, b], L - H + (n + 5) * H, L, H, g, m, pad, on, off)
            assert model.rows[b] == [tuple(r) for r in rows[:, :2].tolist()]
            assert np.array_equal(model.vlen[:, b], expected_vlen(mask, hops, L, H, D))
            assert int(model.vlen[:, b].sum()) == total
    # the walks did exercise the chain
    assert hysteresis(s[:, 0], on, off).any() and not hysteresis(s[:, 0], on, off).all()


def test_labels_with_padding_only():
    """on=None: label == active decides, the runs are padded."""
    rng = np.random.default_rng(11)
    n, B = 200, 5
    lab = rng.integers(0, 3, size=(n, B)).astype(np.uint8)
    lab[rng.random((n, B)) < 0.5] = 2
    for pad in PADS[1:]:
        model = OnlineOp(B, 400, 160, 1, 2, pad, active=2).run(lab, np.full(B, n))
        for b in range(B):
            rows, _ = clip_chain(lab[:, b], 240 + (n + 5) * 160, 400, 160, 1, 2, pad, active=2)
            assert model.rows[b] == [tuple(r) for r in rows[:, :2].tolist()], (pad, b)


def test_a_run_at_either_end_is_clamped():
    L, H = 400, 160
    s = np.zeros((20, 1), np.float32)
    s[0:2] = 1.0
    s[18:20] = 1.0
    model = OnlineOp(1, L, H, 0, 0, (4, 6), on=0.5).run(s, np.array([20]))
    assert model.rows[0] == [(2 * H, (1 + 6 + 2) * H + L), ((18 - 4 + 2) * H, (19 + 2) * H + L)]


# ---------------------------------------------------------------------------
# the library: symbols, sizing entries, refusals (no device call is reached)
# ---------------------------------------------------------------------------
SYMBOLS = ["vad_stream_hops_scores", "vad_stream_hops_scores_i16", "vad_stream_hops_tree_scores",
           "vad_stream_hops_tree_scores_i16", "vad_tree_plan_set_scores", "vad_tree_plan_score_classes",
           "vad_stream_seg_delay_pad", "vad_stream_seg_flush_rows_pad", "vad_stream_seg_history_elems_pad",
           "vad_stream_segments_op", "vad_stream_segments_op_f32", "vad_stream_segments_op_i16",
           "vad_stream_segments_op_flush", "vad_stream_segments_op_flush_f32", "vad_stream_segments_op_flush_i16"]


@pytest.fixture(scope="module")
def lib():
    from vad_amd import _lib
    return _lib.lib()


def test_library_exports_the_entries(lib):
    from vad_amd import _lib
    header = open(os.path.join(REPO, "include", "vad_amd.h")).read()
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\(" % name, header), name
        assert name in integration, name


def test_sizing_entries(lib):
    for (g, m), (L, H) in itertools.product([(0, 0), (0, 1), (3, 0), (2, 3), (7, 5)], FRAMINGS + [(8, 3), (5, 5)]):
        # pad (0, 0): the entries without _pad
        assert lib.vad_stream_seg_delay_pad(g, m, L, H, 0, 0) == lib.vad_stream_seg_delay(g, m, L, H) == seg_delay(g, m, L, H)
        assert lib.vad_stream_seg_flush_rows_pad(g, m, L, H, 0, 0) == lib.vad_stream_seg_flush_rows(g, m, L, H) \
            == flush_rows(g, m, L, H)
        for S, K in ((1, 1), (65, 8)):
            assert lib.vad_stream_seg_history_elems_pad(S, K, g, m, L, H, 0, 0) == \
                lib.vad_stream_seg_history_elems(S, K, g, m, L, H)
        for pad in PADS:
            D = delay_pad(g, m, L, H, pad)
            assert lib.vad_stream_seg_delay_pad(g, m, L, H, *pad) == D
            assert lib.vad_stream_seg_flush_rows_pad(g, m, L, H, *pad) == flush_rows_pad(g, m, L, H, pad)
            assert lib.vad_stream_seg_history_elems_pad(3, 8, g, m, L, H, *pad) >= 3 * ((D + 3) * H + L + 8 * H)
    assert lib.vad_stream_seg_delay_pad(0, 0, 400, 160, -1, 0) == -1
    assert lib.vad_stream_seg_delay_pad(0, 0, 400, 160, 0, -1) == -1
    assert lib.vad_stream_seg_delay_pad(0, 0, 400, 160, (1 << 29) + 1, 0) == -1
    assert lib.vad_stream_seg_flush_rows_pad(0, 0, 400, 0, 1, 1) == -1
    assert lib.vad_stream_seg_history_elems_pad(1, 1, 0, 0, 400, 160, 1 << 29, 0) == -1  # past 2^30 per stream
    assert lib.vad_stream_seg_history_elems_pad(-1, 1, 0, 0, 400, 160, 0, 0) == -1


E = -1  # VAD_EINVAL
N = None  # NULL
BLK, ST, SEG, FND = 0x10000, 0x20000, 0x30000, 0x40000
HOP, HIS, VOI, VLN = 0x100000, 0x200000, 0x300000, 0x400000
S, K, L, H = 4, 3, 400, 160
PB, PA = 2, 3
D = 0 + 1 + 1 + 1 + PB
RING = (D + 3 + K) * H + L


def op(lib, fn="vad_stream_segments_op", **kw):
    a = dict(block=BLK, sc=1, bs=S, S=S, K=K, active=1, gap=0, run=0, L=L, H=H, on=0.6, off=0.4, pb=PB, pa=PA,
             state=ST, seg=SEG, cap=8, found=FND, hop=HOP, hs=H, hbs=S * H, hist=HIS, helems=S * RING, voiced=VOI,
             vlen=VLN)
    a.update(kw)
    head = (a["block"], a["sc"], a["bs"], a["S"], a["K"], a["active"], a["gap"], a["run"], a["L"], a["H"], a["on"],
            a["off"], a["pb"], a["pa"], a["state"], a["seg"], a["cap"], a["found"])
    if fn == "vad_stream_segments_op":
        return getattr(lib, fn)(*head, N)
    return getattr(lib, fn)(*head, a["hop"], a["hs"], a["hbs"], a["hist"], a["helems"], a["voiced"], a["vlen"], N)


def op_flush(lib, fn, **kw):
    a = dict(S=S, sc=1, gap=0, run=0, L=L, H=H, on=0.6, off=0.4, pb=PB, pa=PA, state=ST, seg=SEG, cap=8, found=FND,
             hist=HIS, helems=S * RING, voiced=VOI, vlen=VLN)
    a.update(kw)
    head = (a["S"], a["sc"], a["gap"], a["run"], a["L"], a["H"], a["on"], a["off"], a["pb"], a["pa"], a["state"],
            a["seg"], a["cap"], a["found"])
    if fn == "vad_stream_segments_op_flush":
        return getattr(lib, fn)(*head, N)
    return getattr(lib, fn)(*head, a["hist"], a["helems"], a["voiced"], a["vlen"], N)


NAN = float("nan")
OLD = [dict(H=0), dict(H=-160), dict(H=L + 1), dict(L=0), dict(gap=-1), dict(run=-1), dict(cap=-1), dict(S=-1),
       dict(state=N), dict(found=N), dict(seg=N)]
NEW = [dict(on=1.5), dict(on=-0.1, off=-0.2), dict(off=-0.1), dict(on=0.3, off=0.4), dict(on=NAN), dict(off=NAN),
       dict(on=NAN, off=NAN), dict(pb=-1), dict(pa=-1), dict(pb=(1 << 29) + 1), dict(sc=2), dict(sc=-1)]


@pytest.mark.parametrize("fn", ["vad_stream_segments_op", "vad_stream_segments_op_f32", "vad_stream_segments_op_i16"])
def test_op_entries_refuse(lib, fn):
    cases = OLD + NEW + [dict(K=-1), dict(active=255), dict(active=-1), dict(block=N), dict(bs=S - 1), dict(bs=0),
                         dict(block=BLK + 2)]  # a score block is 4-byte aligned
    if fn != "vad_stream_segments_op":
        cases += [dict(hop=N), dict(hist=N), dict(voiced=N), dict(vlen=N), dict(hs=H - 1), dict(hbs=0),
                  dict(hbs=S * H - 1), dict(helems=S * RING - 1), dict(helems=-1),
                  dict(helems=S * ((1 << 30) + 1)),
                  dict(pb=1 << 24, helems=S * (1 << 30)),  # the history would pass 2^30 elements per stream
                  dict(hist=HIS + 1), dict(voiced=VOI + 1), dict(vlen=VLN + 2)]
    for kw in cases:
        assert op(lib, fn, **kw) == E, kw
    for kw in NEW[:-2]:  # the label form checks the same operating point
        assert op(lib, fn, sc=0, **kw) == E, kw
    assert op(lib, fn, S=0) == 0 and op(lib, fn, K=0) == 0
    assert op(lib, fn, S=0, block=N, state=N, seg=N, found=N) == 0  # nothing would be used
    assert op(lib, fn, S=0, on=NAN) == E and op(lib, fn, K=0, pb=-1) == E  # a bad argument stays bad
    assert op(lib, fn, S=0, on=1.0, off=0.0) == 0 and op(lib, fn, S=0, on=0.0, off=0.0) == 0  # the ends are allowed
    if fn != "vad_stream_segments_op":
        # the history a label segmenter would need is too small once there is a pad
        assert op(lib, fn, helems=S * (RING - PB * H)) == E


@pytest.mark.parametrize("fn", ["vad_stream_segments_op_flush", "vad_stream_segments_op_flush_f32",
                                "vad_stream_segments_op_flush_i16"])
def test_op_flush_entries_refuse(lib, fn):
    cases = OLD + NEW
    if fn != "vad_stream_segments_op_flush":
        cases += [dict(hist=N), dict(voiced=N), dict(vlen=N), dict(helems=S * ((D + 3) * H + L) - 1), dict(helems=-1)]
    for kw in cases:
        assert op_flush(lib, fn, **kw) == E, kw
    assert op_flush(lib, fn, S=0) == 0
    assert op_flush(lib, fn, S=0, off=0.7) == E


@pytest.mark.parametrize("name", ["vad_stream_hops_scores", "vad_stream_hops_scores_i16",
                                  "vad_stream_hops_tree_scores", "vad_stream_hops_tree_scores_i16"])
def test_scored_hop_entries_refuse_null_plans(lib, name):
    """Without a device there is no plan to hand over: the null-plan refusals
    (the rest, which read a plan, are in tests/test_gpu_stream_scores.py)."""
    walk = (0,) if "tree" in name else ()
    fn = getattr(lib, name)
    for plan, cls in ((N, N), (0x1000, N), (N, 0x1000)):
        assert fn(plan, cls, 0x2000, L, L, HOP, H, H, S, K, S * H, 0x3000, 0x4000, BLK, S, *walk, 1, 0x5000, S, N) == E
    assert lib.vad_tree_plan_set_scores(N, 0x1000, 2) == E
    assert lib.vad_tree_plan_score_classes(N) == -1


def test_python_argument_checks():
    import torch
    from vad_amd.stream_segments import StreamSegmenter
    cpu = torch.device("cpu")
    for kw in (dict(on=1.5), dict(on=0.4, off=0.6), dict(on=float("nan")), dict(off=0.5), dict(pad=(-1, 0)),
               dict(pad=(0, -1))):
        with pytest.raises(ValueError):
            StreamSegmenter(4, device=cpu, **kw)
    with pytest.raises(TypeError):
        StreamSegmenter(4, device=cpu, pad=3)
    seg = StreamSegmenter(4, device=cpu, max_gap=2, min_run=3, on=0.6, pad=(2, 3))
    assert seg.off == seg.on == 0.6 and seg.delay == 2 + 3 + 1 + 1 + 2
    assert seg.flush_rows == seg.delay + 2 + 3
    plain = StreamSegmenter(4, device=cpu, max_gap=2, min_run=3)
    assert plain.delay == 2 + 3 + 1 + 1 and plain._events_fn == "vad_stream_segments"  # the entries it always called
    assert StreamSegmenter(4, device=cpu, pad=(0, 1)).delay == plain.delay - 2 - 2  # pad_after adds no delay
