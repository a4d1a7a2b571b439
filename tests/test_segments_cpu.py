"""Speech segments from labels: the NumPy model of the semantics (shared with
tests/test_gpu_segments.py), pinned by hand-written cases; the C ABI's
refusals, which happen before any HIP call (no GPU here); and the Python
layer's argument checks.

The model is a plain loop over maximal runs -- deliberately not the prefix
scans the kernels use, so it shares no logic with them.

  a[i] = (labels[i] == active); window i stands for frame i + 2, the samples
  [(i+2)*hop, (i+2)*hop + frame_size).
  close(g): a maximal run of 0 of length <= g with a 1 on both sides -> 1.
  open(m):  a maximal run of 1 of length < m -> 0 (runs at the ends too).
  smooth(max_gap, min_run) = open(min_run)(close(max_gap)(a)).
  segments: close(frame_size // hop - 1) after smooth; run [i0, i1] ->
  [(i0+2)*hop, min((i1+2)*hop + frame_size, n_samples)), with the exclusive
  prefix sum of the lengths as the packed offset.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def runs_of(a):
    """[(start, length, value)] of the maximal runs of a 1-D array."""
    a = np.asarray(a)
    if len(a) == 0:
        return []
    edges = np.flatnonzero(a[1:] != a[:-1]) + 1
    starts = np.concatenate(([0], edges))
    lens = np.concatenate((edges, [len(a)])) - starts
    return list(zip(starts.tolist(), lens.tolist(), a[starts].tolist()))


def model_close(a, g):
    out = np.array(a, dtype=np.uint8)
    n = len(out)
    for s, l, v in runs_of(a):
        if v == 0 and l <= g and s > 0 and s + l < n:
            out[s:s + l] = 1
    return out


def model_open(a, m):
    out = np.array(a, dtype=np.uint8)
    for s, l, v in runs_of(a):
        if v == 1 and l < m:
            out[s:s + l] = 0
    return out


def model_smooth(labels, max_gap=0, min_run=0, active=1):
    a = (np.asarray(labels) == active).astype(np.uint8)
    return model_open(model_close(a, max_gap), min_run)


def model_rows(d, n_samples, frame_size, hop):
    """(k, 3) int64 rows (start, end, offset) of the runs of final labels d,
    and the voiced total."""
    rows, off = [], 0
    for s, l, v in runs_of(d):
        if v == 1:
            start = (s + 2) * hop
            end = min((s + l - 1 + 2) * hop + frame_size, n_samples)
            rows.append((start, end, off))
            off += end - start
    return np.array(rows, dtype=np.int64).reshape(-1, 3), off


def model_segments(labels, n_samples, frame_size=400, hop=160, max_gap=0, min_run=0, active=1):
    d = model_close(model_smooth(labels, max_gap, min_run, active), frame_size // hop - 1)
    return model_rows(d, n_samples, frame_size, hop)


def model_voiced(audio, rows):
    parts = [audio[s:e] for s, e, _ in rows.tolist()]
    return np.concatenate(parts) if parts else audio[:0]


def model_active_frames(audio, labels, frame_size, hop, active=1):
    parts = [audio[(i + 2) * hop:(i + 2) * hop + frame_size] for i in np.flatnonzero(np.asarray(labels) == active)]
    return np.stack(parts) if parts else np.zeros((0, frame_size), dtype=audio.dtype)


def samples_for_windows(n, frame_size, hop):
    """The shortest clip with exactly n windows (n + 5 frames; a frame is
    taken while len - offset > frame_size)."""
    return (n + 4) * hop + frame_size + 1 if n > 0 else 0


# ---------------------------------------------------------------------------
# the model itself, against answers spelled out by hand
# ---------------------------------------------------------------------------
def L(s):
    return np.array([int(c) for c in s], dtype=np.uint8)


def test_model_gap_of_max_gap_closes_and_one_longer_does_not():
    assert model_smooth(L("1100110001"), max_gap=2).tolist() == L("1111110001").tolist()
    assert model_smooth(L("1100110001"), max_gap=3).tolist() == L("1111111111").tolist()
    assert model_smooth(L("1100110001"), max_gap=1).tolist() == L("1100110001").tolist()
    assert model_smooth(L("1100110001"), max_gap=0).tolist() == L("1100110001").tolist()


def test_model_run_shorter_than_min_run_goes():
    assert model_smooth(L("0110111011110"), min_run=3).tolist() == L("0000111011110").tolist()  # 2 goes, 3 stays
    assert model_smooth(L("0110111011110"), min_run=4).tolist() == L("0000000011110").tolist()
    assert model_smooth(L("0110111011110"), min_run=1).tolist() == L("0110111011110").tolist()
    assert model_smooth(L("110001"), min_run=2).tolist() == L("110000").tolist()  # a short run at the end goes
    assert model_smooth(L("111"), min_run=4).tolist() == L("000").tolist()


def test_model_gap_at_either_end_never_closes():
    assert model_smooth(L("0011100"), max_gap=5).tolist() == L("0011100").tolist()
    assert model_smooth(L("0000"), max_gap=9).tolist() == L("0000").tolist()
    assert model_smooth(L("0101"), max_gap=1).tolist() == L("0111").tolist()


def test_model_close_runs_before_open():
    # the one-window gap closes first, so the joined run of 3 survives min_run 3
    assert model_smooth(L("0010100"), max_gap=1, min_run=3).tolist() == L("0011100").tolist()
    assert model_smooth(L("0010100"), max_gap=0, min_run=3).tolist() == L("0000000").tolist()


def test_model_active_value():
    assert model_smooth(np.array([2, 1, 0, 2, 2], dtype=np.uint8), active=2).tolist() == [1, 0, 0, 1, 1]


def test_model_segments_at_reference_framing():
    ns = samples_for_windows(12, 400, 160)
    assert ns == 16 * 160 + 401
    # a one-window gap: frames 3 and 5 overlap (480..880, 800..1200) -> one segment
    rows, total = model_segments(L("010100000000"), ns)
    assert rows.tolist() == [[480, 1200, 0]] and total == 720
    # a two-window gap: frames 3 and 6 (480..880, 960..1360) stay apart
    rows, total = model_segments(L("010010000011"), ns)
    assert rows.tolist() == [[480, 880, 0], [960, 1360, 400], [12 * 160, 13 * 160 + 400, 800]]
    assert total == 800 + 560
    rows, total = model_segments(L("000000000000"), ns)
    assert rows.shape == (0, 3) and total == 0


def test_model_segments_touching_frames_and_clip_end():
    # hop == frame_size: adjacent windows touch and are one run anyway; no extra closing
    rows, total = model_segments(L("1101"), samples_for_windows(4, 5, 5), 5, 5)
    assert rows.tolist() == [[10, 20, 0], [25, 30, 10]] and total == 15
    # (8, 3): 8 // 3 - 1 = 1, a one-window gap merges (frames 6..14 and 12..20 overlap)
    rows, _ = model_segments(L("1010010"), samples_for_windows(7, 8, 3), 8, 3)
    assert rows.tolist() == [[6, 20, 0], [21, 29, 14]]
    # the end is clipped to the clip
    rows, total = model_rows(L("0011"), 17, 8, 3)
    assert rows.tolist() == [[12, 17, 0]] and total == 5


def test_model_voiced_and_frames():
    audio = np.arange(40, dtype=np.int16)
    rows, _ = model_segments(L("1010010"), samples_for_windows(7, 8, 3), 8, 3)
    assert model_voiced(audio, rows).tolist() == list(range(6, 20)) + list(range(21, 29))
    fr = model_active_frames(audio, L("1010010"), 8, 3)
    assert fr.tolist() == [list(range(6, 14)), list(range(12, 20)), list(range(21, 29))]


# ---------------------------------------------------------------------------
# the C ABI refuses bad arguments before any HIP call
# ---------------------------------------------------------------------------
CHILD = r'''
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
from vad_amd import _lib
L = _lib.lib()
N = None  # NULL
P, Q, W = 0x10000, 0x20000, 0x40000  # never dereferenced: every call below is refused first
BIG = 1 << 30
res = {}
def call(tag, name, *args):
    res[tag] = int(getattr(L, name)(*args))
# vad_label_smooth(labels, n, active, max_gap, min_run, out, ws, ws_bytes, stream)
call("smooth null labels", "vad_label_smooth", N, 10, 1, 0, 0, Q, W, BIG, N)
call("smooth null out", "vad_label_smooth", P, 10, 1, 0, 0, N, W, BIG, N)
call("smooth null ws", "vad_label_smooth", P, 10, 1, 0, 0, Q, N, BIG, N)
call("smooth negative n", "vad_label_smooth", P, -1, 1, 0, 0, Q, W, BIG, N)
call("smooth negative max_gap", "vad_label_smooth", P, 10, 1, -1, 0, Q, W, BIG, N)
call("smooth negative min_run", "vad_label_smooth", P, 10, 1, 0, -1, Q, W, BIG, N)
call("smooth active 256", "vad_label_smooth", P, 10, 256, 0, 0, Q, W, BIG, N)
call("smooth out == labels", "vad_label_smooth", P, 10, 1, 0, 0, P, W, BIG, N)
call("smooth out overlaps labels", "vad_label_smooth", P, 10, 1, 0, 0, P + 5, W, BIG, N)
call("smooth short ws", "vad_label_smooth", P, 10, 1, 0, 0, Q, W, 8, N)
# vad_label_segments(labels, n, active, max_gap, min_run, frame_size, hop, n_samples, segments, capacity, counts, ws, ws_bytes, stream)
ns = 14 * 160 + 401  # exactly 10 windows
res["n_frames"] = int(L.vad_n_frames(ns, 400, 160))
call("segments null labels", "vad_label_segments", N, 10, 1, 0, 0, 400, 160, ns, Q, 6, Q + 4096, W, BIG, N)
call("segments null table", "vad_label_segments", P, 10, 1, 0, 0, 400, 160, ns, N, 6, Q + 4096, W, BIG, N)
call("segments null counts", "vad_label_segments", P, 10, 1, 0, 0, 400, 160, ns, Q, 6, N, W, BIG, N)
call("segments null ws", "vad_label_segments", P, 10, 1, 0, 0, 400, 160, ns, Q, 6, Q + 4096, N, BIG, N)
call("segments negative n", "vad_label_segments", P, -1, 1, 0, 0, 400, 160, ns, Q, 6, Q + 4096, W, BIG, N)
call("segments negative capacity", "vad_label_segments", P, 10, 1, 0, 0, 400, 160, ns, Q, -1, Q + 4096, W, BIG, N)
call("segments negative n_samples", "vad_label_segments", P, 0, 1, 0, 0, 400, 160, -5, Q, 6, Q + 4096, W, BIG, N)
call("segments hop 0", "vad_label_segments", P, 10, 1, 0, 0, 400, 0, ns, Q, 6, Q + 4096, W, BIG, N)
call("segments hop negative", "vad_label_segments", P, 10, 1, 0, 0, 400, -160, ns, Q, 6, Q + 4096, W, BIG, N)
call("segments hop > frame_size", "vad_label_segments", P, 10, 1, 0, 0, 400, 401, 1 << 20, Q, 6, Q + 4096, W, BIG, N)
call("segments frame_size 0", "vad_label_segments", P, 10, 1, 0, 0, 0, 160, ns, Q, 6, Q + 4096, W, BIG, N)
call("segments too many labels", "vad_label_segments", P, 11, 1, 0, 0, 400, 160, ns, Q, 6, Q + 4096, W, BIG, N)
call("segments one sample short", "vad_label_segments", P, 10, 1, 0, 0, 400, 160, ns - 1, Q, 6, Q + 4096, W, BIG, N)
call("segments short ws", "vad_label_segments", P, 10, 1, 0, 0, 400, 160, ns, Q, 6, Q + 4096, W, 8, N)
call("segments negative max_gap", "vad_label_segments", P, 10, 1, -1, 0, 400, 160, ns, Q, 6, Q + 4096, W, BIG, N)
# vad_gather_segments_*(audio, n_samples, segments, counts, capacity, out, out_capacity, stream)
A, O = 0x100000, 0x800000
for fn in ("vad_gather_segments_f32", "vad_gather_segments_i16"):
    call(fn + " null audio", fn, N, 1000, Q, Q + 4096, 6, O, 1000, N)
    call(fn + " null table", fn, A, 1000, N, Q + 4096, 6, O, 1000, N)
    call(fn + " null counts", fn, A, 1000, Q, N, 6, O, 1000, N)
    call(fn + " null out", fn, A, 1000, Q, Q + 4096, 6, N, 1000, N)
    call(fn + " negative n_samples", fn, A, -1, Q, Q + 4096, 6, O, 1000, N)
    call(fn + " negative capacity", fn, A, 1000, Q, Q + 4096, -1, O, 1000, N)
    call(fn + " negative out_capacity", fn, A, 1000, Q, Q + 4096, 6, O, -1, N)
    call(fn + " out overlaps audio", fn, A, 1000, Q, Q + 4096, 6, A + 64, 1000, N)
    call(fn + " odd out pointer", fn, A, 1000, Q, Q + 4096, 6, O + 1, 1000, N)
# vad_gather_active_frames_*(audio, n_samples, labels, n, active, frame_size, hop, out, cap_frames, count, ws, ws_bytes, stream)
ns = 11 * 160 + 400  # window 9 is frame 11: it ends exactly at the clip's end
for fn in ("vad_gather_active_frames_f32", "vad_gather_active_frames_i16"):
    call(fn + " null audio", fn, N, ns, P, 10, 1, 400, 160, O, 10, Q, W, BIG, N)
    call(fn + " null labels", fn, A, ns, N, 10, 1, 400, 160, O, 10, Q, W, BIG, N)
    call(fn + " null out", fn, A, ns, P, 10, 1, 400, 160, N, 10, Q, W, BIG, N)
    call(fn + " null count", fn, A, ns, P, 10, 1, 400, 160, O, 10, N, W, BIG, N)
    call(fn + " null ws", fn, A, ns, P, 10, 1, 400, 160, O, 10, Q, N, BIG, N)
    call(fn + " negative n", fn, A, ns, P, -1, 1, 400, 160, O, 10, Q, W, BIG, N)
    call(fn + " negative capacity", fn, A, ns, P, 10, 1, 400, 160, O, -1, Q, W, BIG, N)
    call(fn + " hop 0", fn, A, ns, P, 10, 1, 400, 0, O, 10, Q, W, BIG, N)
    call(fn + " hop negative", fn, A, ns, P, 10, 1, 400, -1, O, 10, Q, W, BIG, N)
    call(fn + " frame_size 0", fn, A, ns, P, 10, 1, 0, 160, O, 10, Q, W, BIG, N)
    call(fn + " too many labels", fn, A, ns - 1, P, 10, 1, 400, 160, O, 10, Q, W, BIG, N)
    call(fn + " short ws", fn, A, ns, P, 10, 1, 400, 160, O, 10, Q, W, 8, N)
neutral = {
    "ws_bytes_negative": int(L.vad_segments_workspace_bytes(-1)),
    "ws_bytes_zero": int(L.vad_segments_workspace_bytes(0)),
    "ws_bytes_1000": int(L.vad_segments_workspace_bytes(1000)),
    "ws_bytes_1M": int(L.vad_segments_workspace_bytes(1000000)),
    "smooth_empty": int(L.vad_label_smooth(N, 0, 1, 3, 3, N, N, 0, N)),
}
print(json.dumps({"calls": res, "neutral": neutral}))
'''


def test_segment_entries_refuse_bad_arguments():
    r = subprocess.run([sys.executable, "-c", CHILD, REPO], capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    out = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    calls = out["calls"]
    assert calls.pop("n_frames") == 15
    assert len(calls) > 60
    bad = {k: v for k, v in calls.items() if v != -1}
    assert not bad, bad  # every refusal is VAD_EINVAL, with no GPU present
    n = out["neutral"]
    assert n["ws_bytes_negative"] == 0 and n["ws_bytes_zero"] == 0
    assert 0 < n["ws_bytes_1000"] < n["ws_bytes_1M"] < 32 * 1000000
    assert n["smooth_empty"] == 0  # nothing to do, nothing launched


def test_header_exports_the_tile_constants():
    import re
    src = open(os.path.join(REPO, "include", "vad_amd.h")).read()
    from vad_amd import segments as S
    assert int(re.search(r"#define VAD_SEG_TILE (\d+)", src).group(1)) == S.SEG_TILE
    assert int(re.search(r"#define VAD_SEG_CARRY_PASS (\d+)", src).group(1)) == S.SEG_CARRY_PASS


# ---------------------------------------------------------------------------
# the Python layer's argument checks (before any device work)
# ---------------------------------------------------------------------------
def test_python_argument_checks():
    import torch
    from vad_amd import segments as S
    lab = torch.zeros(10, dtype=torch.uint8)
    audio = torch.zeros(3000)
    with pytest.raises(TypeError, match="CUDA"):
        S.smooth_labels(lab)
    with pytest.raises(TypeError, match="CUDA"):
        S.label_segments(lab, 3000)
    with pytest.raises(TypeError, match="CUDA"):
        S.active_frames(audio, lab)
    with pytest.raises(TypeError, match="uint8"):
        S.smooth_labels(lab.to(torch.int32))
    with pytest.raises(TypeError, match="uint8"):
        S.label_segments(lab.to(torch.bool), 3000)
    with pytest.raises(TypeError, match="float32 or int16"):
        S.active_frames(audio.double(), lab)
    with pytest.raises(TypeError):
        S.smooth_labels(np.zeros(10, dtype=np.uint8))
    with pytest.raises(TypeError):
        S.voiced_audio(audio, None)
    # aliasing is decided from the address ranges
    buf = torch.zeros(64, dtype=torch.uint8)
    assert S._overlaps(buf[:32], buf[:32]) and S._overlaps(buf[:32], buf[31:40])
    assert not S._overlaps(buf[:32], buf[32:]) and not S._overlaps(buf[:0], buf[:32])
    f = torch.zeros(64)
    assert S._overlaps(f[:16], f[15:20]) and not S._overlaps(f[:16], f[16:])
