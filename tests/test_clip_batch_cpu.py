"""Clip batches (include/vad_amd.h, "Clip batches") without a GPU: the packed
layout's tables against a plain Python loop, the proof obligations of
vad_amd.batch.ClipBatch (every clip's frames and rows inside the global
ranges), the NumPy model of per-clip smoothing / segment rows / voiced audio
(the single-clip model of tests/test_segments_cpu.py called per clip and
concatenated; tests/test_gpu_clip_batch.py uses it), and the C entries'
refusals, which happen before any HIP call (the pointers are never
dereferenced)."""
import numpy as np
import pytest

from test_segments_cpu import model_close, model_rows, model_smooth, model_voiced

LENS_REF = [0, 1, 159, 160, 161, 400, 401, 400 + 5 * 160, 400 + 5 * 160 + 1, 1200, 1201, 1280]
FRAMINGS = [(400, 160), (8, 3), (5, 5)]


def boundary_lens(fs, hop):
    """The boundaries of LENS_REF at another framing: 0, 1, around one hop,
    around one frame, around the first row (6 frames), around a multiple of
    the hop past it."""
    if (fs, hop) == (400, 160):
        return list(LENS_REF)
    m = ((fs + 5 * hop) // hop + 1) * hop
    return [0, 1, hop - 1, hop, hop + 1, fs, fs + 1, fs + 5 * hop, fs + 5 * hop + 1, m - 1, m, m + 1, m + hop]


def loop_tables(lens, fs, hop):
    """The layout by a plain loop (the reference's own framing loop for F)."""
    t = {k: [] for k in ("start", "len", "frame0", "n_frames", "n_rows", "row0")}
    pos = r0 = 0
    for n in lens:
        f, o = 0, 0
        while n - o > fs:  # file_processing.py:99
            f, o = f + 1, o + hop
        assert pos % hop == 0
        t["start"].append(pos), t["len"].append(n), t["frame0"].append(pos // hop)
        t["n_frames"].append(f), t["n_rows"].append(max(f - 5, 0)), t["row0"].append(r0)
        r0 += max(f - 5, 0)
        pos += (n + hop - 1) // hop * hop
    return {k: np.array(v, np.int64) for k, v in t.items()}, pos


def orders(lens):
    rng = np.random.default_rng(len(lens))
    return [list(lens), list(lens)[::-1], [lens[i] for i in rng.permutation(len(lens))], list(lens) + list(lens)]


# ---------------------------------------------------------------------------
# the model: the single-clip model per clip, concatenated
# ---------------------------------------------------------------------------
def batch_model(labels, tables, fs, hop, max_gap=0, min_run=0, active=1):
    """labels: the global window array.  Returns a dict: smooth (global uint8,
    0 outside every clip), rows (k, 4) int64 (clip, start, end, offset),
    packed (k, 3) (start[k] + start, start[k] + end, offset), clip_rows,
    clip_row0, clip_voiced, counts [rows, samples]."""
    labels = np.asarray(labels)
    smooth = np.zeros(len(labels), np.uint8)
    rows, packed, clip_rows, clip_row0, clip_voiced = [], [], [], [], []
    off = 0
    for k, (f0, r, n, s0) in enumerate(zip(tables["frame0"].tolist(), tables["n_rows"].tolist(),
                                           tables["len"].tolist(), tables["start"].tolist())):
        sm = model_smooth(labels[f0:f0 + r], max_gap, min_run, active)
        smooth[f0:f0 + r] = sm
        rk, total = model_rows(model_close(sm, fs // hop - 1), n, fs, hop)
        clip_row0.append(len(rows)), clip_rows.append(len(rk)), clip_voiced.append(total)
        for s, e, o in rk.tolist():
            rows.append((k, s, e, off + o))
            packed.append((s0 + s, s0 + e, off + o))
        off += total
    return {"smooth": smooth, "rows": np.array(rows, np.int64).reshape(-1, 4),
            "packed": np.array(packed, np.int64).reshape(-1, 3), "clip_rows": np.array(clip_rows, np.int64),
            "clip_row0": np.array(clip_row0, np.int64), "clip_voiced": np.array(clip_voiced, np.int64),
            "counts": [len(rows), off]}


def batch_model_voiced(clips, model):
    """The voiced samples of every clip (clips: the host arrays), concatenated."""
    parts = []
    for k, c in enumerate(clips):
        r0, r = int(model["clip_row0"][k]), int(model["clip_rows"][k])
        parts.append(model_voiced(c, model["rows"][r0:r0 + r, 1:]))
    return np.concatenate(parts) if parts else np.zeros(0, np.int16)


def windows_of(lens, fs, hop):
    """Global windows of the packed buffer of these clips (G - 5)."""
    t, total = loop_tables(lens, fs, hop)
    g = (total - fs - 1) // hop + 1 if total > fs else 0
    return t, total, max(g - 5, 0)


def L(s):
    return np.array([int(c) for c in s], dtype=np.uint8)


# ---------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fs,hop", FRAMINGS)
def test_layout_tables_match_a_plain_loop(fs, hop):
    from vad_amd import _lib
    from vad_amd.batch import layout
    lib = _lib.lib()
    for lens in orders(boundary_lens(fs, hop)):
        got, total = layout(lens, fs, hop)
        want, want_total = loop_tables(lens, fs, hop)
        assert total == want_total and total % hop == 0
        for k in want:
            assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (k, fs, hop)
        assert [int(lib.vad_n_frames(n, fs, hop)) for n in lens] == want["n_frames"].tolist()
        # every clip's frames and rows lie inside the global ranges
        g = int(lib.vad_n_frames(total, fs, hop))
        # (a clip with no frames has an empty range, which asks for nothing)
        framed = want["n_frames"] > 0
        assert (want["frame0"] + want["n_frames"])[framed].max() <= g
        has = want["n_rows"] > 0
        assert has.any() and (want["frame0"] + want["n_rows"])[has].max() <= g - 5
        # a clip's frames read its own samples only, and the clips do not overlap
        last = want["start"] + (want["n_frames"] - 1) * hop + fs
        assert (last[want["n_frames"] > 0] < (want["start"] + want["len"])[want["n_frames"] > 0]).all()
        assert (want["start"][1:] >= (want["start"] + want["len"])[:-1]).all()
        # junk frames: the docstring's expression
        slots = -(-want["len"] // hop)
        assert g == total // hop - fs // hop
        assert g - want["n_frames"].sum() == (slots - want["n_frames"]).sum() - fs // hop
        longer = want["len"] > fs
        per_clip = (slots - want["n_frames"])[longer]
        assert ((per_clip == fs // hop) | (per_clip == -(-fs // hop))).all()


def test_the_reference_length_set_hits_every_boundary():
    t, _ = loop_tables(LENS_REF, 400, 160)
    assert t["n_frames"].tolist() == [0, 0, 0, 0, 0, 0, 1, 5, 6, 5, 6, 6]
    assert t["n_rows"].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 1]
    assert t["frame0"].tolist() == [0, 0, 1, 2, 3, 5, 8, 11, 19, 27, 35, 43]


def test_layout_of_no_clips_and_bad_arguments():
    from vad_amd.batch import layout
    t, total = layout([], 400, 160)
    assert total == 0 and all(len(v) == 0 and v.dtype == np.int64 for v in t.values())
    t, total = layout([0, 0], 400, 160)
    assert total == 0 and t["frame0"].tolist() == [0, 0] and t["n_rows"].tolist() == [0, 0]
    with pytest.raises(ValueError):
        layout([10], 160, 400)  # hop > frame_size
    with pytest.raises(ValueError):
        layout([10], 400, 0)
    with pytest.raises(ValueError):
        layout([-1], 400, 160)


def test_python_argument_checks():
    import torch
    from vad_amd.batch import ClipBatch
    from vad_amd.pipeline import VadPipeline
    with pytest.raises(TypeError, match="all int16 or all float32"):
        ClipBatch.from_host([np.zeros(10, np.int16), np.zeros(10, np.float32)])
    with pytest.raises(TypeError, match="int16 or float32"):
        ClipBatch.from_host([np.zeros(10, np.float64)])
    with pytest.raises(TypeError, match="CUDA"):
        ClipBatch.from_device([torch.zeros(10)])
    with pytest.raises(TypeError, match="CUDA"):
        ClipBatch(torch.zeros(10), [10])
    with pytest.raises(TypeError, match="ClipBatch"):
        VadPipeline._check_batch(None, torch.zeros(10))  # before the pipeline's own state is looked at


# ---------------------------------------------------------------------------
# the model, against answers spelled out by hand
# ---------------------------------------------------------------------------
def test_batch_model_keeps_clips_apart():
    # (8, 3): two clips of 6 windows each (11 frames: 8 + 10 * 3 + 1 = 39 samples -> 13 slots)
    lens = [39, 39]
    t, total, n = windows_of(lens, 8, 3)
    assert t["n_rows"].tolist() == [6, 6] and t["frame0"].tolist() == [0, 13] and n == 26 - 2 - 5
    lab = np.zeros(n, np.uint8)
    lab[[4, 5]] = 1      # clip 0 ends active
    lab[[13, 14]] = 1    # clip 1 starts active
    lab[8] = 1           # a junk window: never active
    m = batch_model(lab, t, 8, 3)
    assert m["smooth"].tolist() == L("0000110000000110000")[:n].tolist()
    # two rows, not joined by the frame-overlap close
    assert m["rows"].tolist() == [[0, 18, 29, 0], [1, 6, 17, 11]]
    assert m["packed"].tolist() == [[18, 29, 0], [39 + 6, 39 + 17, 11]]
    assert m["clip_rows"].tolist() == [1, 1] and m["clip_row0"].tolist() == [0, 1]
    assert m["clip_voiced"].tolist() == [11, 11] and m["counts"] == [2, 22]
    # a gap with a clip boundary inside it does not close; inside a clip it does
    m = batch_model(lab, t, 8, 3, max_gap=20)
    assert m["smooth"][:6].tolist() == [0, 0, 0, 0, 1, 1] and m["smooth"][13:19].tolist() == [1, 1, 0, 0, 0, 0]
    # runs of min_run - 1 that meet at the boundary both go
    m = batch_model(lab, t, 8, 3, min_run=3)
    assert not m["smooth"].any() and m["counts"] == [0, 0] and m["rows"].shape == (0, 4)
    audio = [np.arange(39, dtype=np.int16), np.arange(100, 139, dtype=np.int16)]
    v = batch_model_voiced(audio, batch_model(lab, t, 8, 3))
    assert v.tolist() == list(range(18, 29)) + list(range(106, 117))


# ---------------------------------------------------------------------------
# the C ABI refuses bad arguments before any HIP call
# ---------------------------------------------------------------------------
E = -1  # VAD_EINVAL
N = None  # NULL
LAB, OUT, WS = 0x10000, 0x20000, 0x40000
F0, NR, LEN, R0 = 0x100000, 0x110000, 0x120000, 0x130000
SEG, PK, CNT, CR, CR0, CV = 0x200000, 0x210000, 0x220000, 0x230000, 0x240000, 0x250000
BIG = 1 << 30


@pytest.fixture(scope="module")
def lib():
    from vad_amd import _lib
    return _lib.lib()


def test_pack_entries_refuse(lib):
    for fn in (lib.vad_batch_pack_f32, lib.vad_batch_pack_i16):
        # (src_ptrs, lens, start, n_clips, dst, total, stream)
        assert fn(N, LEN, F0, 3, OUT, 1000, N) == E
        assert fn(R0, N, F0, 3, OUT, 1000, N) == E
        assert fn(R0, LEN, N, 3, OUT, 1000, N) == E
        assert fn(R0, LEN, F0, -1, OUT, 1000, N) == E
        assert fn(R0, LEN, F0, 3, OUT, -1, N) == E
        assert fn(R0, LEN, F0, 3, N, 1000, N) == E
        assert fn(R0, LEN, F0, 3, OUT + 2, 1000, N) == E and fn(R0, LEN, F0, 3, OUT + 8, 1000, N) == E
        assert fn(R0, LEN, F0, 3, N, 0, N) == 0 and fn(N, N, N, 0, N, 0, N) == 0  # nothing to write
        assert fn(N, LEN, F0, 3, N, 0, N) == E  # a bad argument stays bad when there is nothing to do


def test_compact_entry_refuses(lib):
    fn = lib.vad_batch_compact_rows
    # (rows, n_rows_in, row_bytes, frame0, n_rows, row0, n_clips, out, n_rows_out, stream)
    assert fn(N, 100, 156, F0, NR, R0, 3, OUT, 50, N) == E
    assert fn(LAB, 100, 156, N, NR, R0, 3, OUT, 50, N) == E
    assert fn(LAB, 100, 156, F0, N, R0, 3, OUT, 50, N) == E
    assert fn(LAB, 100, 156, F0, NR, N, 3, OUT, 50, N) == E
    assert fn(LAB, 100, 156, F0, NR, R0, 3, N, 50, N) == E
    assert fn(LAB, 100, 156, F0, NR, R0, 3, OUT + 4, 50, N) == E
    assert fn(LAB, 100, 0, F0, NR, R0, 3, OUT, 50, N) == E and fn(LAB, 100, -1, F0, NR, R0, 3, OUT, 50, N) == E
    assert fn(LAB, -1, 156, F0, NR, R0, 3, OUT, 50, N) == E and fn(LAB, 100, 156, F0, NR, R0, 3, OUT, -1, N) == E
    assert fn(LAB, 100, 156, F0, NR, R0, -1, OUT, 50, N) == E
    assert fn(LAB, 100, 156, F0, NR, R0, 3, LAB + 16, 50, N) == E  # out overlaps rows
    assert fn(LAB, 100, 156, F0, NR, R0, 3, N, 0, N) == 0 and fn(N, 0, 1, N, N, N, 0, N, 0, N) == 0


def smooth(lib, **kw):
    a = dict(labels=LAB, n=10, f0=F0, nr=NR, nc=2, active=1, gap=0, run=0, out=OUT, ws=WS, wsb=BIG)
    a.update(kw)
    return lib.vad_batch_label_smooth(a["labels"], a["n"], a["f0"], a["nr"], a["nc"], a["active"], a["gap"], a["run"],
                                      a["out"], a["ws"], a["wsb"], N)


def segments(lib, **kw):
    a = dict(labels=LAB, n=10, f0=F0, nr=NR, len=LEN, nc=2, active=1, gap=0, run=0, L=400, H=160, seg=SEG, pk=PK,
             cap=6, cnt=CNT, cr=CR, cr0=CR0, cv=CV, ws=WS, wsb=BIG)
    a.update(kw)
    return lib.vad_batch_label_segments(a["labels"], a["n"], a["f0"], a["nr"], a["len"], a["nc"], a["active"],
                                        a["gap"], a["run"], a["L"], a["H"], a["seg"], a["pk"], a["cap"], a["cnt"],
                                        a["cr"], a["cr0"], a["cv"], a["ws"], a["wsb"], N)


COMMON = [dict(labels=N), dict(f0=N), dict(nr=N), dict(n=-1), dict(nc=-1), dict(gap=-1), dict(run=-1),
          dict(active=-1), dict(active=256), dict(ws=N), dict(wsb=8), dict(ws=WS + 8)]


def test_smooth_entry_refuses(lib):
    for kw in COMMON + [dict(out=N), dict(out=LAB), dict(out=LAB + 5), dict(out=LAB - 5)]:
        assert smooth(lib, **kw) == E, kw
    assert smooth(lib, n=0, labels=N, out=N, ws=N, wsb=0) == 0  # nothing to do, nothing launched
    assert smooth(lib, n=0, f0=N) == E and smooth(lib, n=0, gap=-1) == E  # bad stays bad


def test_segments_entry_refuses(lib):
    for kw in COMMON + [dict(len=N), dict(cr=N), dict(cr0=N), dict(cv=N), dict(cnt=N), dict(seg=N), dict(pk=N),
                        dict(cap=-1), dict(H=0), dict(H=-160), dict(H=401), dict(L=0),
                        dict(seg=LAB), dict(seg=LAB - 8), dict(pk=LAB + 8), dict(cnt=LAB)]:
        assert segments(lib, **kw) == E, kw
    assert segments(lib, cap=0, seg=N, pk=N, wsb=8) == E  # the workspace is needed whatever the capacity


def test_workspace_bytes(lib):
    fn = lib.vad_batch_segments_workspace_bytes
    assert fn(-1, 3) == 0 and fn(10, -1) == 0 and fn(0, 0) == 0
    assert 0 < fn(1000, 1) < fn(1000, 1000) < fn(1000000, 1000) < 32 * 1000000
    assert fn(0, 5) >= 2 * 8 * 5
