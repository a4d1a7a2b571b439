"""Clip batches on the device (vad_amd/batch.py, csrc/batch_kernel.hip,
csrc/batch_segments_kernel.hip).  Every comparison is exact equality: the
values are integers, copied bits, or outputs of the same kernels on the same
frame data.  The yardsticks are the single-clip API run on each clip alone and
the NumPy model of tests/test_clip_batch_cpu.py (the single-clip model of
tests/test_segments_cpu.py per clip, concatenated).

T = VAD_SEG_TILE.  The layouts below put a clip boundary at global window
T - 2: inside a scan tile and within 3 windows of a tile edge."""
import numpy as np
import pytest

from test_clip_batch_cpu import LENS_REF, batch_model, batch_model_voiced, loop_tables
from test_segments_cpu import samples_for_windows

pytestmark = pytest.mark.gpu

T = 1024
PARAMS = [(0, 0), (1, 0), (0, 2), (3, 5), (T + 3, 0), (0, T + 3)]
FRAMINGS = [(400, 160), (400, 400), (8, 3)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from vad_amd import segments as S
    assert S.SEG_TILE == T
    return torch


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def device_sources(torch, clips):
    """Device views of the clips, each at an odd sample offset of one allocation."""
    dt = torch.from_numpy(clips[0][:0]).dtype
    buf = torch.empty(sum(len(c) + 2 for c in clips) + 1, dtype=dt, device="cuda")
    views, pos = [], 1
    for c in clips:
        v = buf[pos:pos + len(c)]
        v.copy_(torch.from_numpy(c))
        views.append(v)
        pos += len(c) + (2 if len(c) % 2 == 0 else 1)
        assert pos % 2 == 1
    return views


# ---------------------------------------------------------------------------
# 1. labels and features
# ---------------------------------------------------------------------------
def label_clip_lens():
    """A clip of T - 2 hop slots first (the next clip starts at global window
    T - 2), the degenerate lengths, 70 frames (across a 64-frame MFCC tile)
    and 1,100 frames."""
    return [(T - 2) * 160] + list(LENS_REF) + [160 * 69 + 401, 0, 160 * 1099 + 401, 401]


@pytest.fixture(scope="module")
def clips_f32():
    from oracle import vad_oracle as O
    return [O.synth_clip(n, seed=200 + i)[:n].astype(np.float32) for i, n in enumerate(label_clip_lens())]


def make_pipe(name, golden):
    from vad_amd.ffn import FFNClassifier, TOPOLOGY_BL13, random_layers
    from vad_amd.pipeline import VadPipeline
    if name == "bl13":
        return VadPipeline(FFNClassifier(random_layers(TOPOLOGY_BL13, seed=3)))
    if name == "tree":
        from sklearn.tree import DecisionTreeClassifier
        gt = golden("tree")
        return VadPipeline(DecisionTreeClassifier(max_depth=6, random_state=0).fit(
            np.nan_to_num(gt["x_test"]), gt["y_test"]))
    w = golden("ffn")
    layers = [(w[f"ref39_W{i}"], w[f"ref39_b{i}"]) for i in range(4)]
    return VadPipeline(FFNClassifier(layers, arith="f32" if name == "ref39_f32" else "split_f16"))


@pytest.mark.parametrize("dtype", ["i16", "f32"])
@pytest.mark.parametrize("clf", ["bl13", "ref39_split", "ref39_f32", "tree"])
def test_labels_and_features_equal_the_single_clip_path(torch_cuda, golden, clips_f32, clf, dtype):
    torch = torch_cuda
    from vad_amd import _lib
    from vad_amd.batch import ClipBatch
    pipe = make_pipe(clf, golden)
    if clf.startswith("ref39"):
        assert pipe.ffn.arith == ("f32" if clf == "ref39_f32" else "split_f16")
    clips = clips_f32 if dtype == "f32" else [c.astype(np.int16) for c in clips_f32]
    lens = [len(c) for c in clips]
    tabs, total = loop_tables(lens, 400, 160)
    assert tabs["frame0"][1] == T - 2 and tabs["n_frames"].max() == 1100 and 70 in tabs["n_frames"].tolist()
    want_packed = np.zeros(total, clips[0].dtype)
    for c, s in zip(clips, tabs["start"].tolist()):
        want_packed[s:s + len(c)] = c
    sources = device_sources(torch, clips)  # what from_device packs: any sample offset, bits copied
    # the yardstick: every clip alone in an allocation of its own, as a caller of the clip path holds it (a
    # source that is not pair-aligned takes the MFCC kernel's generic variant, whose rounding is another)
    alone = [torch.from_numpy(c).cuda() for c in clips]
    want_lab = [pipe.labels(s).cpu().numpy() for s in alone]
    want_feat = {m: [pipe.features(s, mode=m).cpu().numpy() for s in alone]
                 for m in (_lib.FEAT_ANALYSER, _lib.FEAT_OFFLINE)}
    assert [len(w) for w in want_lab] == tabs["n_rows"].tolist()
    for how in ("from_host", "from_device"):
        b = ClipBatch.from_host(clips) if how == "from_host" else ClipBatch.from_device(sources)
        assert b.n_clips == len(clips) and b.total == total and b.n_windows > T
        for name in tabs:
            assert np.array_equal(b.host[name], tabs[name]), name
            assert np.array_equal(getattr(b, "d_" + name).cpu().numpy(), tabs[name]), (how, name)
        # the samples where they belong, the slot tails zero
        assert np.array_equal(bits(b.data.cpu().numpy()), bits(want_packed)), how
        assert b.junk_frames == b.n_frames_global - int(tabs["n_frames"].sum()) and 0 < b.junk_share < 0.05
        lab = pipe.labels_batch(b)
        assert len(lab) == len(clips) and lab.labels.numel() == b.n_windows
        got = [lab[k].cpu().numpy() for k in range(len(clips))]
        for k in range(len(clips)):
            assert got[k].dtype == np.uint8 and np.array_equal(got[k], want_lab[k]), (how, k, lens[k])
        assert np.array_equal(lab.packed().cpu().numpy(), np.concatenate(want_lab))
        if pipe.fusable:
            fl = pipe.labels_batch(b, fused=True)
            assert np.array_equal(fl.labels.cpu().numpy(), lab.labels.cpu().numpy()), how
        for m, want in want_feat.items():
            packed = pipe.features_batch(b, mode=m, packed=True)
            assert tuple(packed.shape) == (int(tabs["n_rows"].sum()), 39) and packed.is_contiguous()
            assert np.array_equal(bits(packed.cpu().numpy()), bits(np.concatenate(want))), (how, m)
            views = pipe.features_batch(b, mode=m)
            for k, v in enumerate(views):
                assert np.array_equal(bits(v.cpu().numpy()), bits(want[k])), (how, m, k)
    assert clf != "bl13" or pipe.fusable  # the fused form was compared for the fusable topology


def test_empty_and_rowless_batches(torch_cuda, golden):
    torch = torch_cuda
    from vad_amd.batch import ClipBatch
    from vad_amd.config import MfccConfig
    from vad_amd.segments import batch_label_segments, batch_smooth_labels
    pipe = make_pipe("bl13", golden)
    for clips in ([], [np.zeros(0, np.int16)], [np.ones(n, np.int16) for n in (0, 1, 400, 1200)]):
        for b in (ClipBatch.from_host(clips), ClipBatch.from_device([torch.from_numpy(c).cuda() for c in clips])):
            assert b.n_clips == len(clips) and b.total_rows == 0
            lab = pipe.labels_batch(b)
            assert lab.labels.numel() == b.n_windows and all(lab[k].numel() == 0 for k in range(b.n_clips))
            assert tuple(pipe.features_batch(b, packed=True).shape) == (0, 39)
            junk = torch.ones(b.n_windows, dtype=torch.uint8, device="cuda")  # caller-made: every junk window "active"
            assert not batch_smooth_labels(junk, b, 2, 2).any()
            seg = batch_label_segments(junk, b)
            assert seg.meta.cpu().tolist() == [0, 0] + [0] * (3 * b.n_clips) and seg.numpy().shape == (0, 3)
            v, offsets = pipe.voiced_batch(b)
            assert v.numel() == 0 and offsets.tolist() == [0] * (b.n_clips + 1)
    with pytest.raises(TypeError):
        ClipBatch.from_device([torch.zeros(5, device="cuda"), torch.zeros(5, dtype=torch.int16, device="cuda")])
    from vad_amd.pipeline import VadPipeline
    pre = VadPipeline(cfg=MfccConfig(preemph=0.97))
    with pytest.raises(ValueError, match="preemph"):
        pre.features_batch(ClipBatch.from_host([np.zeros(2000, np.float32)]))
    with pytest.raises(ValueError, match="framing"):
        pipe.labels_batch(ClipBatch.from_host([np.zeros(100, np.int16)], MfccConfig(frame_size=8, hop=3)))


# ---------------------------------------------------------------------------
# 2. segments on caller-made labels
# ---------------------------------------------------------------------------
def segment_layout(fs, hop):
    """Clip lengths by rows: the first clip ends so that the second starts at
    global window T - 2; clips of no rows between clips with rows."""
    slots_over_rows = 4 + -(-(fs + 1) // hop)  # hop slots of the shortest clip with r > 0 windows, minus r
    rows = [T - 2 - slots_over_rows, 700, 0, 0, 50, 0, 40, 1, 2, 0, 9, 9, 1500, 0, 12, 0]
    rowless = iter([0, 1, fs, fs + 1, hop, 0, fs + 5 * hop, 0])
    lens = [samples_for_windows(r, fs, hop) if r else next(rowless) for r in rows]
    tabs, total = loop_tables(lens, fs, hop)
    assert tabs["n_rows"].tolist() == rows and tabs["frame0"][1] == T - 2
    return lens, tabs, total


def label_families(n, tabs, seed):
    """name -> uint8 global labels (1 = active; inactive 0 or 2 in the random
    ones; the junk windows take whatever the family gives them)."""
    f0, nr = tabs["frame0"].tolist(), tabs["n_rows"].tolist()
    fam = {"zeros": np.zeros(n, np.uint8), "ones": np.ones(n, np.uint8),
           "alternating": (np.arange(n) % 2).astype(np.uint8)}
    ends = np.zeros(n, np.uint8)
    built = np.zeros(n, np.uint8)
    with_rows = [k for k in range(len(f0)) if nr[k] > 0]
    for k in with_rows:
        ends[f0[k]] = ends[f0[k] + nr[k] - 1] = 1  # runs of 1 meet at every boundary
        if nr[k] >= 9:  # runs of 4 = min_run - 1 of (3, 5) at both ends of the clip
            built[f0[k]:f0[k] + 4] = built[f0[k] + nr[k] - 4:f0[k] + nr[k]] = 1
    k_all, k_none = with_rows[3], with_rows[2]
    built[f0[k_all]:f0[k_all] + nr[k_all]] = 1  # a clip that is all active
    built[f0[k_none]:f0[k_none] + nr[k_none]] = 0  # and one that is all inactive
    built[f0[1] - 3:f0[1]] = 1  # junk windows between the first two clips: never active
    fam["ends"], fam["built"] = ends, built
    rng = np.random.default_rng(seed + n)
    for p in (0.02, 0.5, 0.98):
        a = (rng.random(n) < p).astype(np.uint8)
        a[(a == 0) & (rng.random(n) < 0.3)] = 2
        fam[f"iid{p}"] = a
    return fam


def check_segments(seg, model, where):
    k = model["counts"][0]
    meta = seg.meta.cpu().numpy()
    nc = seg.batch.n_clips
    assert meta[:2].tolist() == model["counts"], where
    assert np.array_equal(meta[2:2 + nc], model["clip_rows"]), where
    assert np.array_equal(meta[2 + nc:2 + 2 * nc], model["clip_row0"]), where
    assert np.array_equal(meta[2 + 2 * nc:], model["clip_voiced"]), where
    assert seg.capacity >= k, where
    assert np.array_equal(seg.table[:k].cpu().numpy(), model["rows"]), where
    assert np.array_equal(seg.packed[:k].cpu().numpy(), model["packed"]), where


@pytest.mark.parametrize("fs,hop", FRAMINGS)
def test_segments_stop_at_clip_edges(torch_cuda, fs, hop):
    torch = torch_cuda
    from vad_amd import segments as S
    from vad_amd.batch import ClipBatch
    from vad_amd.config import MfccConfig
    lens, tabs, total = segment_layout(fs, hop)
    rng = np.random.default_rng(fs * 1000 + hop)
    if hop == 160:
        clips = [rng.standard_normal(n).astype(np.float32) for n in lens]
    else:
        clips = [rng.integers(-32768, 32768, size=n).astype(np.int16) for n in lens]
    b = ClipBatch.from_host(clips, MfccConfig(frame_size=fs, hop=hop))
    n = b.n_windows
    assert n > 3 * T and np.array_equal(b.host["n_rows"], tabs["n_rows"])
    ws = S.batch_workspace(b, b.data.device)
    seen_rows = 0
    for name, lab in label_families(n, tabs, 7).items():
        d_lab = torch.from_numpy(lab).cuda()
        for mg, mr in PARAMS:
            where = (name, fs, hop, mg, mr)
            m = batch_model(lab, tabs, fs, hop, mg, mr)
            got = S.batch_smooth_labels(d_lab, b, mg, mr, ws=ws).cpu().numpy()
            assert got.dtype == np.uint8 and np.array_equal(got, m["smooth"]), where
            seg = S.batch_label_segments(d_lab, b, mg, mr, ws=ws)
            check_segments(seg, m, where)
            seen_rows = max(seen_rows, m["counts"][0])
            if (mg, mr) in ((0, 0), (3, 5)):  # the packed-coordinates table, through the existing gather
                out = torch.full((b.total + 7,), 77, dtype=b.data.dtype, device="cuda")
                S.batch_voiced_audio(b, seg, out=out[:b.total])
                want = batch_model_voiced(clips, m)
                got = out.cpu().numpy()
                assert np.array_equal(bits(got[:len(want)]), bits(want)), where
                assert (got[len(want):] == 77).all(), where
            if name == "ends":
                f0, nr = tabs["frame0"], tabs["n_rows"]
                if (mg, mr) == (T + 3, 0):  # gaps <= max_gap with a clip boundary inside: not closed
                    assert m["smooth"][f0[1] - 1] == 0 and m["smooth"][f0[1]] == 1
                    assert m["clip_rows"].tolist() == [(1 if r <= T + 5 else 2) if r else 0 for r in nr.tolist()]
                if (mg, mr) == (0, 2):  # the runs of 1 at both sides of a boundary go
                    assert m["smooth"][f0[0] + nr[0] - 1] == 0 and m["smooth"][f0[1]] == 0
            if name == "ones" and (mg, mr) == (0, 0):  # a clip ends active, the next starts active: two rows
                assert m["counts"][0] == int((tabs["n_rows"] > 0).sum())
            if name == "built" and (mg, mr) == (3, 5):  # runs of min_run - 1 at the clip ends are removed
                assert m["smooth"][tabs["frame0"][1]:tabs["frame0"][1] + 4].tolist() == [0] * 4
    assert seen_rows > 400
    # another active value, and labels from a BatchLabels
    from vad_amd.batch import BatchLabels
    lab = rng.integers(0, 3, size=n).astype(np.uint8)
    seg = S.batch_label_segments(BatchLabels(torch.from_numpy(lab).cuda(), b), b, 2, 3, active=2)
    check_segments(seg, batch_model(lab, tabs, fs, hop, 2, 3, active=2), "active 2")
    rows = seg.numpy()
    assert np.array_equal(rows, batch_model(lab, tabs, fs, hop, 2, 3, active=2)["rows"][:, :3])
    assert np.array_equal(seg.clip(1), rows[rows[:, 0] == 1][:, 1:])
    assert np.array_equal(seg.seconds(16000)[:, 1:], rows[:, 1:] / 16000.0)
    with pytest.raises(ValueError, match="global windows"):
        S.batch_label_segments(torch.zeros(n + 1, dtype=torch.uint8, device="cuda"), b)


@pytest.mark.parametrize("short", ["found - 1", "1", "0"])
def test_segment_capacity(torch_cuda, short):
    torch = torch_cuda
    from vad_amd import _lib, segments as S
    from vad_amd.batch import ClipBatch
    fs, hop = 400, 160
    lens, tabs, total = segment_layout(fs, hop)
    b = ClipBatch.from_host([np.zeros(n, np.int16) for n in lens])
    n, nc = b.n_windows, b.n_clips
    lab = label_families(n, tabs, 9)["iid0.5"]
    m = batch_model(lab, tabs, fs, hop)
    found = m["counts"][0]
    assert found > 100
    cap = {"found - 1": found - 1, "1": 1, "0": 0}[short]
    SENT = -0x0123456789ABCDEF
    table = torch.full((cap + 2, 4), SENT, dtype=torch.int64, device="cuda")
    packed = torch.full((cap + 2, 3), SENT, dtype=torch.int64, device="cuda")
    meta = torch.full((2 + 3 * nc,), SENT, dtype=torch.int64, device="cuda")
    d = torch.from_numpy(lab).cuda()
    ws = S.batch_workspace(b, d.device)
    _lib.check(_lib.lib().vad_batch_label_segments(
        _lib.ptr(d), n, _lib.ptr(b.d_frame0), _lib.ptr(b.d_n_rows), _lib.ptr(b.d_len), nc, 1, 0, 0, fs, hop,
        _lib.ptr(table), _lib.ptr(packed), cap, _lib.ptr(meta[:2]), _lib.ptr(meta[2:2 + nc]),
        _lib.ptr(meta[2 + nc:2 + 2 * nc]), _lib.ptr(meta[2 + 2 * nc:]), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
        "vad_batch_label_segments")
    got = meta.cpu().numpy()
    assert got[:2].tolist() == m["counts"]  # the totals found, not the number written
    assert np.array_equal(got[2:2 + nc], m["clip_rows"]) and np.array_equal(got[2 + 2 * nc:], m["clip_voiced"])
    t, p = table.cpu().numpy(), packed.cpu().numpy()
    assert np.array_equal(t[:cap], m["rows"][:cap]) and np.array_equal(p[:cap], m["packed"][:cap])
    assert (t[cap:] == SENT).all() and (p[cap:] == SENT).all()  # nothing past the capacity is written


# ---------------------------------------------------------------------------
# 3. voiced audio of a batch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["i16", "f32"])
def test_voiced_batch_equals_the_single_clip_path(torch_cuda, golden, clips_f32, dtype):
    torch = torch_cuda
    from vad_amd.batch import ClipBatch
    pipe = make_pipe("ref39_split", golden)
    clips = clips_f32 if dtype == "f32" else [c.astype(np.int16) for c in clips_f32]
    sources = [torch.from_numpy(c).cuda() for c in clips]
    b = ClipBatch.from_device(sources)
    total_voiced = 0
    for active in (0, 1):
        for mg, mr in ((0, 0), (2, 3)):
            want = [pipe.voiced(s, max_gap=mg, min_run=mr, active=active).cpu().numpy() for s in sources]
            v, offsets = pipe.voiced_batch(b, max_gap=mg, min_run=mr, active=active)
            assert v.dtype == sources[0].dtype and offsets.dtype == np.int64
            assert offsets.tolist() == np.concatenate(([0], np.cumsum([len(w) for w in want]))).tolist()
            assert np.array_equal(bits(v.cpu().numpy()), bits(np.concatenate(want))), (active, mg, mr)
            seg = pipe.segments_batch(b, max_gap=mg, min_run=mr, active=active)
            for k, s in enumerate(sources):
                one = pipe.segments(s, max_gap=mg, min_run=mr, active=active).numpy()
                assert np.array_equal(seg.clip(k), one), (active, mg, mr, k)
            total_voiced += v.numel()
    assert total_voiced > 0


# ---------------------------------------------------------------------------
# 4. stale workspaces (the rule of tests/test_gpu_lds_independence.py)
# ---------------------------------------------------------------------------
def test_batch_segments_ignore_stale_workspaces(torch_cuda):
    torch = torch_cuda
    from vad_amd import segments as S
    from vad_amd.batch import ClipBatch
    fs, hop = 400, 160
    lens, tabs, _ = segment_layout(fs, hop)
    small = ClipBatch.from_host([np.zeros(n, np.int16) for n in lens])
    big_lens = [samples_for_windows(r, fs, hop) for r in (3000, 1, 2500, 77)] + lens
    big = ClipBatch.from_host([np.zeros(n, np.int16) for n in big_lens])
    assert big.n_windows > 2 * small.n_windows
    lab = torch.from_numpy(label_families(small.n_windows, tabs, 5)["iid0.5"]).cuda()
    big_lab = torch.ones(big.n_windows, dtype=torch.uint8, device="cuda")
    model = batch_model(lab.cpu().numpy(), tabs, fs, hop, 3, 5)
    assert model["counts"][0] > 50

    def run(ws, larger_first):
        if larger_first:
            S.batch_smooth_labels(big_lab, big, 3, 5, ws=ws)
            S.batch_label_segments(big_lab, big, 3, 5, ws=ws)
        else:
            ws.fill_(0xFF)
        sm = S.batch_smooth_labels(lab, small, 3, 5, ws=ws)
        if not larger_first:
            ws.fill_(0xFF)
        seg = S.batch_label_segments(lab, small, 3, 5, ws=ws)
        k = model["counts"][0]
        return [sm.cpu(), seg.meta.cpu(), seg.table[:k].cpu(), seg.packed[:k].cpu()]

    results = []
    for larger_first in (False, True, False, True):
        ws = S.batch_workspace(big, lab.device)
        ws.fill_(0xFF)
        results.append(run(ws, larger_first))
    check = results[0]
    assert np.array_equal(check[0].numpy(), model["smooth"]) and check[1][:2].tolist() == model["counts"]
    assert np.array_equal(check[2].numpy(), model["rows"])
    for r in results[1:]:
        assert all(torch.equal(a, b) for a, b in zip(r, check))
