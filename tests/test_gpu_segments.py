"""Smoothed labels, speech segments, voiced audio and active frames on the
device (vad_amd/csrc/segments_kernel.hip) against the NumPy model of
tests/test_segments_cpu.py (a plain loop over runs).  Every comparison is
exact equality: these are integers and copied bits.

T = VAD_SEG_TILE labels per scan tile; the tile-total scan covers
VAD_SEG_CARRY_PASS tiles per pass of its one workgroup, so T * PASS + 5 labels
is the smallest size that needs a second pass."""
import ctypes
import os

import numpy as np
import pytest

from test_segments_cpu import (model_active_frames, model_close, model_rows, model_segments, model_smooth,
                               model_voiced, samples_for_windows)

pytestmark = pytest.mark.gpu

T, PASS = 1024, 256
SIZES = [0, 1, 2, 5, T - 1, T, T + 1, 2 * T, 3 * T + 7, T * PASS + 5]
FRAMINGS = [(400, 160), (400, 400), (8, 3), (5, 5)]
SEEDS = [11, 12, 13]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from vad_amd import segments as S
    assert (S.SEG_TILE, S.SEG_CARRY_PASS) == (T, PASS)
    return torch


def params_for(n):
    return [(0, 0), (1, 0), (0, 2), (3, 5), (T + 3, 0), (0, T + 3), (n, n)]


def geometric(rng, n, mean):
    """Alternating runs with geometric lengths; then a run or a gap is laid
    across every tile edge (alternately), so each edge is straddled by both
    kinds over the seeds."""
    out = np.zeros(n, dtype=np.uint8)
    pos, v = 0, int(rng.integers(2))
    while pos < n:
        l = int(rng.geometric(1.0 / mean))
        out[pos:pos + l] = v
        pos, v = pos + l, 1 - v
    first = int(rng.integers(2))
    for k, e in enumerate(range(T, n, T)):
        out[max(e - 3, 0):e + 3] = (k + first) % 2
    return out


def label_families(n, seed):
    """name -> uint8 labels (1 = active; inactive is 0 or 2 in the random ones)."""
    fam = {}
    if seed == "fixed":
        fam["zeros"] = np.zeros(n, dtype=np.uint8)
        fam["ones"] = np.ones(n, dtype=np.uint8)
        fam["alternating"] = (np.arange(n) % 2).astype(np.uint8)
        ends = np.zeros(n, dtype=np.uint8)
        if n:
            ends[0] = ends[-1] = 1
        fam["ends"] = ends
        return fam
    rng = np.random.default_rng(seed * 1000003 + n)
    for p in (0.02, 0.5, 0.98):
        a = (rng.random(n) < p).astype(np.uint8)
        a[(a == 0) & (rng.random(n) < 0.3)] = 2
        fam[f"iid{p}"] = a
    for mean in (3, 300):
        fam[f"geo{mean}"] = geometric(rng, n, mean)
    return fam


@pytest.mark.parametrize("seed", ["fixed"] + SEEDS)
@pytest.mark.parametrize("n", SIZES)
def test_smooth_and_segments_match_model(torch_cuda, n, seed):
    """seed "fixed": the four families without randomness; a number: the five random ones at that seed."""
    torch = torch_cuda
    from vad_amd import segments as S
    ws = S.workspace(n, torch.device("cuda", 0))
    for name, lab in label_families(n, seed).items():
        d_lab = torch.from_numpy(lab).cuda()
        for mg, mr in params_for(n):
            want = model_smooth(lab, mg, mr)
            got = S.smooth_labels(d_lab, mg, mr, ws=ws).cpu().numpy()
            assert got.dtype == np.uint8 and np.array_equal(got, want), (name, n, mg, mr)
            final = {}
            for fs, hop in FRAMINGS:
                g2 = fs // hop - 1
                if g2 not in final:
                    final[g2] = model_close(want, g2)
                ns = samples_for_windows(n, fs, hop)
                rows, total = model_rows(final[g2], ns, fs, hop)
                seg = S.label_segments(d_lab, ns, fs, hop, mg, mr, ws=ws)
                counts = seg.counts.cpu().numpy()
                where = (name, n, mg, mr, fs, hop)
                assert counts.tolist() == [len(rows), total], where
                assert seg.capacity == n // 2 + 1 >= len(rows)
                assert np.array_equal(seg.table[:len(rows)].cpu().numpy(), rows), where
                assert np.array_equal(seg.numpy(), rows[:, :2]), where


def test_model_composition_is_what_the_gpu_test_uses():
    """The cached composition above (smooth, then close, then rows) is the model's segments()."""
    rng = np.random.default_rng(5)
    lab = (rng.random(500) < 0.5).astype(np.uint8)
    for fs, hop in FRAMINGS:
        ns = samples_for_windows(500, fs, hop)
        a, ta = model_segments(lab, ns, fs, hop, 2, 3)
        b, tb = model_rows(model_close(model_smooth(lab, 2, 3), fs // hop - 1), ns, fs, hop)
        assert np.array_equal(a, b) and ta == tb


def test_active_value_unaligned_labels_and_aliasing(torch_cuda):
    torch = torch_cuda
    from vad_amd import segments as S
    rng = np.random.default_rng(3)
    base = rng.integers(0, 3, size=3 * T + 11).astype(np.uint8)
    d = torch.from_numpy(base).cuda()
    for off in (0, 1, 2, 3):  # label pointers of every alignment
        for active in (0, 2):
            lab = base[off:]
            got = S.smooth_labels(d[off:], 2, 3, active=active).cpu().numpy()
            assert np.array_equal(got, model_smooth(lab, 2, 3, active)), (off, active)
            ns = samples_for_windows(len(lab), 8, 3)
            rows, total = model_segments(lab, ns, 8, 3, 2, 3, active)
            seg = S.label_segments(d[off:], ns, 8, 3, 2, 3, active=active)
            assert seg.counts.cpu().tolist() == [len(rows), total]
            assert np.array_equal(seg.table[:len(rows)].cpu().numpy(), rows)
    with pytest.raises(ValueError, match="alias"):
        S.smooth_labels(d, 1, 1, out=d)
    with pytest.raises(ValueError, match="alias"):
        S.smooth_labels(d[:100], 1, 1, out=d[50:150])
    with pytest.raises(ValueError):
        S.label_segments(d, 10 ** 6, 160, 400)  # hop > frame_size
    from vad_amd._lib import VadError
    with pytest.raises(VadError):
        S.label_segments(d, samples_for_windows(len(base), 400, 160) - 1)  # one sample short of the labels


@pytest.mark.parametrize("short", ["found - 1", "0"])
def test_segment_capacity(torch_cuda, short):
    torch = torch_cuda
    from vad_amd import _lib
    rng = np.random.default_rng(21)
    n = 2 * T + 100
    lab = geometric(rng, n, 3)
    ns = samples_for_windows(n, 400, 160)
    rows, total = model_segments(lab, ns)
    found = len(rows)
    assert found > 100
    cap = found - 1 if short == "found - 1" else 0
    SENT = -0x0123456789ABCDEF
    table = torch.full((cap + 2, 3), SENT, dtype=torch.int64, device="cuda")
    counts = torch.full((2,), SENT, dtype=torch.int64, device="cuda")
    d = torch.from_numpy(lab).cuda()
    from vad_amd import segments as S
    ws = S.workspace(n, d.device)
    _lib.check(_lib.lib().vad_label_segments(_lib.ptr(d), n, 1, 0, 0, 400, 160, ns, _lib.ptr(table), cap,
                                             _lib.ptr(counts), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "seg")
    assert counts.cpu().tolist() == [found, total]  # the number found, not the number written
    t = table.cpu().numpy()
    assert np.array_equal(t[:cap], rows[:cap])
    assert (t[cap:] == SENT).all()  # the rows past the capacity are untouched
    # downstream works on the rows that were written
    audio = torch.arange(ns, dtype=torch.float32, device="cuda")
    out = torch.full((ns,), -1.0, device="cuda")
    _lib.check(_lib.lib().vad_gather_segments_f32(_lib.ptr(audio), ns, _lib.ptr(table), _lib.ptr(counts), cap,
                                                  _lib.ptr(out), ns, _lib.stream_ptr()), "gather")
    want = model_voiced(np.arange(ns, dtype=np.float32), rows[:cap])
    got = out.cpu().numpy()
    assert np.array_equal(got[:len(want)], want) and (got[len(want):] == -1.0).all()


def test_sample_indices_are_64_bit(torch_cuda):
    torch = torch_cuda
    from vad_amd import segments as S
    n, hop, fs = 5000, 1 << 20, (1 << 20) + 5
    ns = samples_for_windows(n, fs, hop)
    lab = geometric(np.random.default_rng(8), n, 3)
    lab[-3:] = 1
    rows, total = model_segments(lab, ns, fs, hop)
    assert rows[-1, 0] > 1 << 32 and total > 1 << 31  # starts past 32 bits, offsets past 31
    seg = S.label_segments(torch.from_numpy(lab).cuda(), ns, fs, hop)
    assert seg.counts.cpu().tolist() == [len(rows), total]
    assert np.array_equal(seg.table[:len(rows)].cpu().numpy(), rows)


def make_audio(rng, ns, dtype):
    if dtype == "f32":
        a = rng.standard_normal(ns).astype(np.float32)
        bits = a.view(np.uint32)
        k = rng.integers(0, ns, size=max(ns // 50, 8))
        bits[k[0::4]] = 0x7FC00001  # quiet NaN with a payload
        bits[k[1::4]] = 0xFFA00000  # negative signalling-pattern NaN
        bits[k[2::4]] = 0x80000000  # -0.0
        bits[k[3::4]] = 0x00000001  # the smallest denormal
        return a
    a = rng.integers(-32768, 32768, size=ns).astype(np.int16)
    k = rng.integers(0, ns, size=max(ns // 50, 8))
    a[k[0::2]] = -32768
    a[k[1::2]] = 32767
    return a


def as_bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x.view(np.uint16)


SENT = {"f32": np.float32(-7777.25), "i16": np.int16(-12345)}


def device_view(torch, host, shift):
    """A device copy of `host` whose first element sits `shift` elements past an allocation's start."""
    buf = torch.empty(len(host) + shift, dtype=torch.from_numpy(host[:1]).dtype, device="cuda")
    v = buf[shift:]
    v.copy_(torch.from_numpy(host))
    return v


@pytest.mark.parametrize("dtype", ["f32", "i16"])
@pytest.mark.parametrize("framing,n,mean", [((8, 3), 4000, 3), ((400, 160), 2000, 300)])
def test_voiced_audio(torch_cuda, framing, n, mean, dtype):
    torch = torch_cuda
    from vad_amd import segments as S
    fs, hop = framing
    rng = np.random.default_rng(40 + fs)
    ns = samples_for_windows(n, fs, hop)
    lab = geometric(rng, n, mean)
    lab[T - 150:T + 150] = 1  # at (400, 160): a run that holds whole 32 KB copy tiles of both sample types
    rows, total = model_segments(lab, ns, fs, hop)
    assert 1 < len(rows) and 0 < total < ns
    if framing == (8, 3):  # every alignment of a source start and of a destination offset occurs
        assert set((rows[:, 0] % 8).tolist()) == set(range(8))
        assert set((rows[:, 2] % 8).tolist()) == set(range(8))
    else:
        assert (rows[:, 1] - rows[:, 0]).max() >= 2 * 16384
    audio = make_audio(rng, ns, dtype)
    want = model_voiced(audio, rows)
    assert len(want) == total
    d_lab = torch.from_numpy(lab).cuda()
    seg = S.label_segments(d_lab, ns, fs, hop)
    sent = SENT[dtype]
    # source and destination pointers at every alignment class (2 / 4 / 8 / 16 bytes)
    for a_shift, o_shift in [(0, 0), (1, 0), (2, 0), (4, 0), (0, 1), (3, 2), (0, 4), (5, 7)]:
        d_audio = device_view(torch, audio, a_shift)
        out = device_view(torch, np.full(total + 999, sent, dtype=audio.dtype), o_shift)
        got_out, counts = S.voiced_audio(d_audio, seg, out=out)
        assert got_out is out and counts.cpu().tolist() == [len(rows), total]
        got = out.cpu().numpy()
        assert np.array_equal(as_bits(got[:total]), as_bits(want)), (a_shift, o_shift)
        assert (got[total:] == sent).all(), (a_shift, o_shift)  # the tail is untouched
    d_audio = torch.from_numpy(audio).cuda()
    for cap in (total - 1, total // 2 + 3, 1, 0):  # a short out is filled exactly to its capacity
        buf = device_view(torch, np.full(cap + 64, sent, dtype=audio.dtype), 1)
        S.voiced_audio(d_audio, seg, out=buf[:cap])
        got = buf.cpu().numpy()
        assert np.array_equal(as_bits(got[:cap]), as_bits(want[:cap])), cap
        assert (got[cap:] == sent).all(), cap
    out, counts = S.voiced_audio(d_audio, seg)  # the default: a buffer of the clip's size
    assert out.numel() == ns and np.array_equal(as_bits(out[:total].cpu().numpy()), as_bits(want))
    with pytest.raises(ValueError, match="alias"):
        S.voiced_audio(d_audio, seg, out=d_audio)


@pytest.mark.parametrize("dtype", ["f32", "i16"])
@pytest.mark.parametrize("framing", [(400, 160), (400, 400), (8, 3)])
def test_active_frames(torch_cuda, framing, dtype):
    torch = torch_cuda
    from vad_amd import segments as S
    fs, hop = framing
    n = 2 * T + 77 if fs == 8 else 700
    rng = np.random.default_rng(60 + fs + hop)
    ns = (n + 1) * hop + fs  # the last window's frame ends at the clip's end
    audio = make_audio(rng, ns, dtype)
    sent = SENT[dtype]
    for fam, lab in (("geo3", geometric(rng, n, 3)), ("iid", rng.integers(0, 3, size=n).astype(np.uint8)),
                     ("none", np.zeros(n, dtype=np.uint8))):
        want = model_active_frames(audio, lab, fs, hop)
        k = len(want)
        d_lab = torch.from_numpy(lab).cuda()
        for a_shift, o_shift in [(0, 0), (1, 3), (2, 1)]:
            d_audio = device_view(torch, audio, a_shift)
            out = device_view(torch, np.full((k + 3) * fs, sent, dtype=audio.dtype), o_shift).view(k + 3, fs)
            got_out, count = S.active_frames(d_audio, d_lab, fs, hop, out=out)
            assert count.cpu().tolist() == [k], fam
            got = out.cpu().numpy()
            assert np.array_equal(as_bits(got[:k]), as_bits(want)), (fam, a_shift, o_shift)
            assert (got[k:] == sent).all()
        if k > 1:  # capacity: the count still says what was found, the rows past it are untouched
            d_audio = torch.from_numpy(audio).cuda()
            buf = torch.from_numpy(np.full((k + 1, fs), sent, dtype=audio.dtype)).cuda()
            _, count = S.active_frames(d_audio, d_lab, fs, hop, out=buf[:k - 1])
            assert count.cpu().tolist() == [k]
            got = buf.cpu().numpy()
            assert np.array_equal(as_bits(got[:k - 1]), as_bits(want[:k - 1])) and (got[k - 1:] == sent).all()
    # the default out holds one row per label
    out, count = S.active_frames(torch.from_numpy(audio).cuda(), d_lab, fs, hop)
    assert tuple(out.shape) == (n, fs) and count.cpu().tolist() == [0]
    with pytest.raises(Exception):
        S.active_frames(torch.from_numpy(audio[:-1].copy()).cuda(), d_lab, fs, hop)  # a sample short


@pytest.mark.parametrize("dtype", ["f32", "i16"])
def test_active_frames_of_the_recorder_framing(torch_cuda, dtype):
    """hop == frame_size with every label active: the clip's framed prefix, what vad.py writes."""
    torch = torch_cuda
    from vad_amd import segments as S
    n, fs = 300, 400
    audio = make_audio(np.random.default_rng(70), (n + 2) * fs + 13, dtype)
    lab = torch.ones(n, dtype=torch.uint8, device="cuda")
    out, count = S.active_frames(torch.from_numpy(audio).cuda(), lab, fs, fs)
    assert count.cpu().tolist() == [n]
    assert np.array_equal(as_bits(out.cpu().numpy().reshape(-1)), as_bits(audio[2 * fs:(n + 2) * fs]))


@pytest.mark.parametrize("clf", ["ffn", "tree"])
def test_pipeline_segments_and_voiced(torch_cuda, golden, clf):
    torch = torch_cuda
    from vad_amd.ffn import FFNClassifier
    from vad_amd.pipeline import VadPipeline
    if clf == "ffn":
        w = golden("ffn")
        pipe = VadPipeline(FFNClassifier([(w[f"ref39_W{i}"], w[f"ref39_b{i}"]) for i in range(4)]))
    else:
        from sklearn.tree import DecisionTreeClassifier
        gt = golden("tree")
        pipe = VadPipeline(DecisionTreeClassifier(max_depth=8, random_state=0).fit(
            np.nan_to_num(gt["x_test"]), gt["y_test"]))
    pcm = golden("clip")["clip"]
    for host in (pcm, pcm.astype(np.float32)):
        audio = torch.from_numpy(host).cuda()
        before = pipe.labels(audio).cpu().numpy()
        assert len(before) == 93
        for active in (0, 1):
            for mg, mr in ((0, 0), (2, 3), (10, 4)):
                rows, total = model_segments(before, len(host), 400, 160, mg, mr, active)
                seg = pipe.segments(audio, max_gap=mg, min_run=mr, active=active)
                assert seg.counts.cpu().tolist() == [len(rows), total]
                assert np.array_equal(seg.numpy(), rows[:, :2])
                assert np.array_equal(seg.seconds(16000), rows[:, :2] / 16000.0)
                v = pipe.voiced(audio, max_gap=mg, min_run=mr, active=active)
                assert v.dtype == audio.dtype and v.numel() == total
                assert np.array_equal(as_bits(v.cpu().numpy()), as_bits(model_voiced(host, rows)))
        assert sum(len(model_segments(before, len(host), active=a)[0]) for a in (0, 1)) > 0
        assert np.array_equal(pipe.labels(audio).cpu().numpy(), before)  # labels() itself is unchanged


def test_capture_smooth_segments_gather(torch_cuda):
    """smooth -> segments -> gather captured on one stream (a linear chain of
    kernel nodes), replayed over three label contents in the static buffer."""
    torch = torch_cuda
    from vad_amd import segments as S
    n, fs, hop = 3 * T + 50, 400, 160
    ns = samples_for_windows(n, fs, hop)
    rng = np.random.default_rng(90)
    audio = make_audio(rng, ns, "f32")
    d_audio = torch.from_numpy(audio).cuda()
    static = torch.zeros(n, dtype=torch.uint8, device="cuda")
    smooth = torch.empty(n, dtype=torch.uint8, device="cuda")
    out = torch.empty(ns, device="cuda")
    ws = S.workspace(n, static.device)

    def chain():
        S.smooth_labels(static, 3, 5, out=smooth, ws=ws)
        seg = S.label_segments(static, ns, fs, hop, 3, 5, ws=ws)
        S.voiced_audio(d_audio, seg, out=out)
        return seg

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()  # warm up: code objects loaded before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        seg = chain()
    for i, lab in enumerate((geometric(rng, n, 300), geometric(rng, n, 3), np.zeros(n, dtype=np.uint8))):
        static.copy_(torch.from_numpy(lab))
        out.fill_(-5.0)
        graph.replay()
        torch.cuda.synchronize()
        rows, total = model_segments(lab, ns, fs, hop, 3, 5)
        assert np.array_equal(smooth.cpu().numpy(), model_smooth(lab, 3, 5)), i
        assert seg.counts.cpu().tolist() == [len(rows), total], i
        assert np.array_equal(seg.table[:len(rows)].cpu().numpy(), rows), i
        got = out.cpu().numpy()
        assert np.array_equal(as_bits(got[:total]), as_bits(model_voiced(audio, rows))), i
        assert (got[total:] == -5.0).all(), i


# ---------------------------------------------------------------------------
# stale LDS (as tests/test_gpu_lds_independence.py)
# ---------------------------------------------------------------------------
POISON = (1e30, -1e30, float("nan"))


@pytest.fixture(scope="module")
def poison(torch_cuda):
    torch = torch_cuda
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_host", "liblds_poison.so")
    if not os.path.exists(so):
        pytest.fail("tests/c_host/liblds_poison.so missing: run __graft_entry__.build()")
    helper = ctypes.CDLL(so)
    helper.lds_poison.argtypes = [ctypes.c_float, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    sink = torch.zeros(1, device="cuda")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count

    def fill(v):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert helper.lds_poison(v, ctypes.c_void_p(sink.data_ptr()), 4 * n_cu, st) == 0

    yield fill
    torch.cuda.synchronize()
    assert sink.item() == 0.0  # every poison launch read back its own LDS stores


def test_segment_entries_ignore_stale_lds(torch_cuda, poison):
    torch = torch_cuda
    from vad_amd import segments as S
    n, fs, hop = 5 * T + 9, 400, 160
    ns = samples_for_windows(n, fs, hop)
    rng = np.random.default_rng(95)
    lab = torch.from_numpy(geometric(rng, n, 3)).cuda()
    audio = {d: torch.from_numpy(make_audio(rng, ns, d)).cuda() for d in ("f32", "i16")}

    def run(before):
        """Every entry, each right after before()."""
        before()
        res = [S.smooth_labels(lab, 3, 5)]
        before()
        seg = S.label_segments(lab, ns, fs, hop, 3, 5)
        res += [seg.table[:int(seg.counts[0].item())], seg.counts]
        for d in ("f32", "i16"):
            outs = [torch.zeros(ns, dtype=audio[d].dtype, device="cuda"),
                    torch.zeros((n, fs), dtype=audio[d].dtype, device="cuda")]
            before()
            S.voiced_audio(audio[d], seg, out=outs[0])
            before()
            _, count = S.active_frames(audio[d], lab, fs, hop, out=outs[1])
            res += [o.view(torch.int32 if d == "f32" else torch.int16) for o in outs] + [count]
        return [r.cpu().clone() for r in res]

    want = run(lambda: None)
    assert int(want[2][0]) > 10
    for v in POISON:
        got = run(lambda: poison(v))
        assert all(torch.equal(a, b) for a, b in zip(got, want)), v
