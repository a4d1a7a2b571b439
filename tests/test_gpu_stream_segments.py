"""The streaming segmenter on the device (vad_amd/csrc/stream_segments_kernel.hip,
vad_amd.stream_segments.StreamSegmenter) against the online NumPy model of
tests/test_stream_segments_cpu.py after every block, and against the offline
device entries (label_segments + voiced_audio) on each stream's equivalent
clip after flush.  Every comparison is exact: integers and copied bits.

The equivalent clip of T hops has L - H + T*H samples and T - 5 labels, its
last frame ending exactly at its end; the clip entries count frames with the
reference's strict `>` (vad_n_frames), so they are given the clip with ONE
zero sample appended -- no row reaches it (every end is <= L - H + T*H), so
rows and voiced samples are those of the equivalent clip.

The kernel uses no LDS, so there is no stale-LDS case."""
import functools
import os

import numpy as np
import pytest

from test_stream_segments_cpu import (FAMILIES, FRAMINGS, PARAMS, StreamSegModel, equivalent_clip, packed,
                                      seg_delay, stream_audio, stream_labels)

pytestmark = pytest.mark.gpu

SENT = {np.float32: np.float32(-7777.25), np.int16: np.int16(-12345)}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x.view(np.uint16)


def cfg_of(L, H):
    from vad_amd.config import MfccConfig
    return MfccConfig(frame_size=L, hop=H)


def families_for(S):
    return [FAMILIES[i % len(FAMILIES)] for i in range(S)]


def device_labels(torch, lab):
    """(k, S) labels as rows of a wider buffer: a label_block_stride of S + 3."""
    buf = torch.full((lab.shape[0], lab.shape[1] + 3), 77, dtype=torch.uint8, device="cuda")
    buf[:, :lab.shape[1]].copy_(torch.from_numpy(lab))
    return buf[:, :lab.shape[1]]


def device_hops(torch, hops, layout):
    """(k, S, H) samples, hop-major with padded rows (hop_stride H + 5, one
    element past an allocation's start) or stream-major ((S, k*H) viewed as (k, S, H))."""
    k, S, H = hops.shape
    t = torch.from_numpy(hops)
    if layout == "stream-major":
        buf = torch.empty((S, k * H), dtype=t.dtype, device="cuda")
        v = buf.view(S, k, H).permute(1, 0, 2)
    else:
        buf = torch.empty((k * S * (H + 5) + 1,), dtype=t.dtype, device="cuda")
        v = buf[1:].view(k, S, H + 5)[:, :, :H]
    v.copy_(t)
    assert v.shape == (k, S, H) and v.stride(2) == 1
    return v


def run_device(torch, seg, model, labels, hops, K, dtype, check=True):
    """T hops in blocks of K (the last one shorter) through segmenter and
    model, compared after every block; returns the device's (voiced, len) per
    block, flush included."""
    T, S = labels.shape
    sent = SENT[dtype]
    outs = []
    for b, t0 in enumerate(range(0, T, K)):
        lab, hop = labels[t0:t0 + K], hops[t0:t0 + K]
        k = lab.shape[0]
        seg.voiced.fill_(float(sent) if dtype == np.float32 else int(sent))
        seg.voiced_len.fill_(-1)
        got = seg.push(device_labels(torch, lab), device_hops(torch, hop, ("padded", "stream-major")[b % 2]))
        assert got[0] is seg.voiced and got[1] is seg.voiced_len
        v, n = seg.voiced.cpu().numpy(), seg.voiced_len.cpu().numpy()
        if check:
            mv, mn = model.push(lab, hop)
            assert np.array_equal(n[:k], mn), (b, n[:k].tolist(), mn.tolist())
            assert (n[k:] == -1).all()
            want = np.full(v.shape, sent, dtype=dtype)
            mv_full = np.where(np.arange(seg.cfg.hop)[None, None, :] < mn[:, :, None], mv, sent)
            want[:k] = mv_full
            assert np.array_equal(bits(v), bits(want)), b  # the prefixes, and nothing past them touched
            compare_tables(seg, model, b)
        outs.append((v[:k].copy(), n[:k].copy()))
    seg.flush_voiced.fill_(float(sent) if dtype == np.float32 else int(sent))
    seg.flush_len.fill_(-1)
    fv, fn = seg.flush()
    fv, fn = fv.cpu().numpy(), fn.cpu().numpy()
    if check:
        mv, mn = model.flush()
        assert fv.shape == mv.shape and np.array_equal(fn, mn)
        want = np.where(np.arange(seg.cfg.hop)[None, None, :] < mn[:, :, None], mv, sent)
        assert np.array_equal(bits(fv), bits(want.astype(dtype)))
        compare_tables(seg, model, "flush")
    outs.append((fv, fn))
    return outs


def compare_tables(seg, model, where):
    found = seg.found.cpu().numpy()
    rows = seg.segments()
    for s in range(seg.n):
        want = model.table(s)
        assert found[s] == len(want), (where, s)
        assert np.array_equal(rows[s], want[:seg.capacity]), (where, s)


def compare_offline(torch, seg, outs, labels, carry, hops, g, m, dtype):
    """After flush: label_segments + voiced_audio on each stream's equivalent clip, on the device."""
    from vad_amd import segments as SG
    L, H = seg.cfg.frame_size, seg.cfg.hop
    clip = equivalent_clip(carry, hops)
    rows = seg.segments()
    found = seg.found.cpu().numpy()
    T = labels.shape[0]
    for s in range(seg.n):
        got = packed([o[0] for o in outs], [o[1] for o in outs], s).astype(dtype)
        if T <= 5:
            assert found[s] == 0 and len(got) == 0
            continue
        padded = np.concatenate([clip[s], np.zeros(1, dtype=dtype)])
        d_lab = torch.from_numpy(np.ascontiguousarray(labels[5:, s])).cuda()
        off = SG.label_segments(d_lab, len(padded), L, H, g, m, active=seg.active)
        want_rows = off.numpy()
        assert found[s] == int(off.counts[0].item()), s
        assert np.array_equal(rows[s], want_rows), s
        assert want_rows.size == 0 or want_rows[:, 1].max() <= clip.shape[1]
        out, counts = SG.voiced_audio(torch.from_numpy(padded).cuda(), off)
        total = int(counts[1].item())
        assert len(got) == total, s
        assert np.array_equal(bits(got), bits(out[:total].cpu().numpy())), s


@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("S", [1, 3, 65])
@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("framing", FRAMINGS)
def test_synthetic_labels(torch_cuda, framing, params, S, dtype):
    torch = torch_cuda
    from vad_amd.stream_segments import StreamSegmenter
    (L, H), (g, m) = framing, params
    D = seg_delay(g, m, L, H)
    K = 3
    T = 6 + D + 28  # past the delay, more than one wrap of nothing: the ring is sized for it; not a multiple of K
    T += 1 if T % K == 0 else 0
    rng = np.random.default_rng(L * 7 + H * 3 + g * 100 + m * 10 + S)
    garbage = (g + S) % 2 == 1
    labels = stream_labels(T, rng, families_for(S), head="garbage" if garbage else 255)
    hops = stream_audio(T, S, H, dtype, rng)
    carry = np.zeros((S, L - H), dtype=dtype)
    seg = StreamSegmenter(S, cfg_of(L, H), max_gap=g, min_run=m, hops_per_step=K,
                          audio_dtype=torch.float32 if dtype == np.float32 else torch.int16)
    assert seg.delay == D
    model = StreamSegModel(S, L, H, g, m, dtype=dtype, fill=SENT[dtype])
    outs = run_device(torch, seg, model, labels, hops, K, dtype)
    compare_offline(torch, seg, outs, labels, carry, hops, g, m, dtype)
    # ended: more hops and another flush change nothing and emit nothing
    before = (seg.table.clone(), seg.found.clone())
    seg.push(device_labels(torch, np.ones((K, S), dtype=np.uint8)), device_hops(torch, hops[:K], "padded"))
    assert int(seg.voiced_len.abs().sum().item()) == 0
    seg.flush()
    assert int(seg.flush_len.abs().sum().item()) == 0
    assert torch.equal(seg.table, before[0]) and torch.equal(seg.found, before[1])


@pytest.mark.parametrize("T", [0, 1, 5, 6, 7])
def test_short_streams(torch_cuda, T):
    torch = torch_cuda
    from vad_amd.stream_segments import StreamSegmenter
    L, H, g, m, S = 8, 3, 2, 3, 7
    rng = np.random.default_rng(T)
    labels = stream_labels(T, rng, ["ones"] * S)
    hops = stream_audio(T, S, H, np.int16, rng)
    seg = StreamSegmenter(S, cfg_of(L, H), max_gap=g, min_run=m, hops_per_step=8, audio_dtype=torch.int16)
    model = StreamSegModel(S, L, H, g, m, dtype=np.int16, fill=SENT[np.int16])
    outs = run_device(torch, seg, model, labels, hops, 8, np.int16)
    compare_offline(torch, seg, outs, labels, np.zeros((S, L - H), dtype=np.int16), hops, g, m, np.int16)


def test_long_stream_wraps_the_history_and_reset_restarts(torch_cuda):
    """300 hops: the history ring wraps many times; then reset() and a second, different run."""
    torch = torch_cuda
    from vad_amd.stream_segments import StreamSegmenter
    L, H, g, m, S, K, T = 400, 160, 2, 3, 7, 8, 300
    seg = StreamSegmenter(S, cfg_of(L, H), max_gap=g, min_run=m, hops_per_step=K, audio_dtype=torch.float32)
    assert T * H > 4 * seg.history.shape[1]
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        labels = stream_labels(T, rng)
        hops = stream_audio(T, S, H, np.float32, rng)
        model = StreamSegModel(S, L, H, g, m, dtype=np.float32, fill=SENT[np.float32])
        outs = run_device(torch, seg, model, labels, hops, K, np.float32)
        compare_offline(torch, seg, outs, labels, np.zeros((S, L - H), dtype=np.float32), hops, g, m, np.float32)
        seg.reset()


def test_primed_carry_can_be_voiced(torch_cuda):
    """frame_size > 3 hop: positions [2 hop, L - hop) belong to the carried samples."""
    torch = torch_cuda
    from vad_amd.stream_segments import StreamSegmenter
    L, H, g, m, S, K, T = 9, 2, 1, 2, 3, 3, 40
    rng = np.random.default_rng(9)
    labels = stream_labels(T, rng, ["ones", "geo2", "geo20"])
    labels[labels == 1] = 4
    hops = stream_audio(T, S, H, np.int16, rng)
    carry = rng.integers(1, 99, size=(S, L - H)).astype(np.int16)
    seg = StreamSegmenter(S, cfg_of(L, H), max_gap=g, min_run=m, active=4, hops_per_step=K, audio_dtype=torch.int16)
    seg.prime(torch.from_numpy(carry).cuda())
    model = StreamSegModel(S, L, H, g, m, active=4, dtype=np.int16, fill=SENT[np.int16], carry=carry)
    outs = run_device(torch, seg, model, labels, hops, K, np.int16)
    compare_offline(torch, seg, outs, labels, carry, hops, g, m, np.int16)
    first = packed([o[0] for o in outs], [o[1] for o in outs], 0)[:L - H - 2 * H]
    assert np.array_equal(first, carry[0, 2 * H:])


@pytest.mark.parametrize("short", ["found - 1", "0"])
def test_capacity(torch_cuda, short):
    torch = torch_cuda
    from vad_amd.stream_segments import StreamSegmenter
    L, H, S, K, T = 8, 3, 3, 8, 120
    rng = np.random.default_rng(31)
    labels = stream_labels(T, rng, ["geo2"] * S)
    hops = stream_audio(T, S, H, np.int16, rng)
    model = StreamSegModel(S, L, H, dtype=np.int16, fill=SENT[np.int16])
    for t0 in range(0, T, K):
        model.push(labels[t0:t0 + K], hops[t0:t0 + K])
    model.flush()
    found = [len(model.table(s)) for s in range(S)]
    assert min(found) > 5
    cap = min(found) - 1 if short == "found - 1" else 0
    seg = StreamSegmenter(S, cfg_of(L, H), capacity=cap, hops_per_step=K, audio_dtype=torch.int16)
    GUARD = -0x0123456789ABCDEF
    wide = torch.full((S, cap + 2, 2), GUARD, dtype=torch.int64, device="cuda")  # the table with guard rows behind it
    flat = wide.view(-1)[:S * cap * 2].view(S, cap, 2)
    seg.table = flat
    seg._tables = (seg._tables[0], __import__("ctypes").c_void_p(flat.data_ptr()), cap, seg._tables[3])
    flat.fill_(GUARD)
    fresh = StreamSegModel(S, L, H, dtype=np.int16, fill=SENT[np.int16])
    run_device(torch, seg, fresh, labels, hops, K, np.int16, check=False)
    assert seg.found.cpu().tolist() == found  # the number found, not the number written
    t = flat.cpu().numpy()
    for s in range(S):
        assert np.array_equal(t[s], model.table(s)[:cap]), s
    assert (wide.view(-1)[S * cap * 2:] == GUARD).all()


def test_events_only_entry_matches_the_audio_entry(torch_cuda):
    torch = torch_cuda
    from vad_amd.stream_segments import StreamSegmenter
    L, H, g, m, S, K, T = 400, 160, 3, 2, 7, 8, 96
    rng = np.random.default_rng(41)
    labels = stream_labels(T, rng)
    hops = stream_audio(T, S, H, np.float32, rng)
    a = StreamSegmenter(S, cfg_of(L, H), max_gap=g, min_run=m, hops_per_step=K, audio_dtype=torch.float32)
    b = StreamSegmenter(S, cfg_of(L, H), max_gap=g, min_run=m, hops_per_step=K)
    assert b.history is None and b.voiced is None
    for t0 in range(0, T, K):
        lab = device_labels(torch, labels[t0:t0 + K])
        a.push(lab, device_hops(torch, hops[t0:t0 + K], "padded"))
        assert b.push(lab) is None
        assert torch.equal(a.table, b.table) and torch.equal(a.found, b.found), t0
    a.flush()
    assert b.flush() is None
    assert torch.equal(a.table, b.table) and torch.equal(a.found, b.found)
    assert int(a.found.sum().item()) > 5
    with pytest.raises(ValueError, match="events only"):
        b.push(lab, device_hops(torch, hops[:K], "padded"))


def test_block_size_does_not_matter(torch_cuda):
    torch = torch_cuda
    from vad_amd.stream_segments import StreamSegmenter
    L, H, g, m, S, T = 400, 160, 2, 3, 7, 40
    rng = np.random.default_rng(51)
    labels = stream_labels(T, rng)
    hops = stream_audio(T, S, H, np.int16, rng)
    res = {}
    for K in (8, 1):
        seg = StreamSegmenter(S, cfg_of(L, H), max_gap=g, min_run=m, hops_per_step=K, audio_dtype=torch.int16)
        model = StreamSegModel(S, L, H, g, m, dtype=np.int16, fill=SENT[np.int16])
        outs = run_device(torch, seg, model, labels, hops, K, np.int16, check=False)
        v = np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])
        res[K] = (v, seg.table.cpu().numpy(), seg.found.cpu().numpy())
    for x, y in zip(res[8][0] + res[8][1:], res[1][0] + res[1][1:]):
        assert np.array_equal(x, y)
    assert res[8][2].sum() > 0


# ---------------------------------------------------------------------------
# end to end: StreamBatch -> segmenter, against the clip pipeline
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _clf():
    from vad_amd.ffn import FFNClassifier
    w = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ffn.npz"), allow_pickle=False)
    return FFNClassifier([(w[f"ref39_W{i}"], w[f"ref39_b{i}"]) for i in range(4)], arith="f32")


@functools.lru_cache(maxsize=None)
def _clips(S, T, L=400, H=160):
    from oracle import vad_oracle as O
    n = L - H + T * H
    clips = np.stack([O.synth_clip(n, seed=300 + s)[:n] for s in range(S)]).astype(np.int16)
    hops = np.ascontiguousarray(np.transpose(clips[:, L - H:].reshape(S, T, H), (1, 0, 2)))
    return clips, hops


def test_end_to_end_against_the_clip_pipeline(torch_cuda):
    torch = torch_cuda
    from vad_amd.pipeline import VadPipeline
    from vad_amd.stream import StreamBatch
    S, K, T, L, H, g, m = 8, 4, 120, 400, 160, 2, 3
    clips, hops = _clips(S, T)
    sb = StreamBatch(S, _clf(), hops_per_step=K, input_dtype=torch.int16)
    sb.prime(torch.from_numpy(clips[:, :L - H]).cuda())
    seg = sb.segmenter(max_gap=g, min_run=m)
    assert (seg.n, seg.K, seg.audio_dtype, seg.cfg) == (S, K, torch.int16, sb.cfg)
    labs, outs = [], []
    for t0 in range(0, T, K):
        sb.inputs.copy_(torch.from_numpy(hops[t0:t0 + K]))
        lab = sb.step_block()
        v, n = seg.push(lab, sb.inputs)
        labs.append(lab.cpu().numpy().copy())
        outs.append((v.cpu().numpy().copy(), n.cpu().numpy().copy()))
    fv, fn = seg.flush()
    outs.append((fv.cpu().numpy(), fn.cpu().numpy()))
    labs = np.concatenate(labs)
    rows = seg.segments()
    pipe = VadPipeline(_clf())
    total_rows = 0
    for s in range(S):
        audio = torch.from_numpy(np.concatenate([clips[s], np.zeros(1, dtype=np.int16)])).cuda()
        clip_labels = pipe.labels(audio).cpu().numpy()
        assert np.array_equal(labs[5:, s], clip_labels), s  # both paths give the same labels, or this test fails
        want = pipe.segments(audio, max_gap=g, min_run=m).numpy()
        assert np.array_equal(rows[s], want), s
        voiced = pipe.voiced(audio, max_gap=g, min_run=m).cpu().numpy()
        got = packed([o[0] for o in outs], [o[1] for o in outs], s).astype(np.int16)
        assert np.array_equal(got, voiced), s
        total_rows += len(want)
    assert total_rows > 0


def test_graph_capture_of_hop_block_and_push(torch_cuda):
    """The hop block and the segmenter's push captured as one linear chain on
    one stream, replayed over 10 blocks: the uncaptured run's results."""
    torch = torch_cuda
    from vad_amd.stream import StreamBatch
    S, K, L, H, g, m = 8, 4, 400, 160, 2, 3
    clips, hops = _clips(S, 10 * K)
    d_hops = torch.from_numpy(hops).cuda()
    carry = torch.from_numpy(clips[:, :L - H]).cuda()

    def make():
        sb = StreamBatch(S, _clf(), hops_per_step=K, input_dtype=torch.int16)
        return sb, sb.segmenter(max_gap=g, min_run=m)

    def body(sb, seg):
        sb.step_block()
        seg.push(sb.label_block, sb.inputs)

    def collect(sb, seg, res):
        res.append([x.clone() for x in (sb.label_block, seg.voiced_len, seg.table, seg.found)])
        n = seg.voiced_len.cpu().numpy()
        v = seg.voiced.cpu().numpy()
        res[-1].append(np.where(np.arange(H)[None, None, :] < n[:, :, None], v, 0))

    sb, seg = make()
    sb.prime(carry)
    plain = []
    for b in range(10):
        sb.inputs.copy_(d_hops[b * K:(b + 1) * K])
        body(sb, seg)
        collect(sb, seg, plain)

    sb, seg = make()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body(sb, seg)  # warm up: code objects loaded before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    sb.reset(), seg.reset()
    sb.prime(carry)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body(sb, seg)
    sb.reset(), seg.reset()  # the capture ran nothing; start from the same state anyway
    sb.prime(carry)
    replayed = []
    for b in range(10):
        sb.inputs.copy_(d_hops[b * K:(b + 1) * K])
        graph.replay()
        collect(sb, seg, replayed)
    torch.cuda.synchronize()
    for b, (x, y) in enumerate(zip(plain, replayed)):
        assert all(torch.equal(p, q) for p, q in zip(x[:4], y[:4])), b
        assert np.array_equal(x[4], y[4]), b
    assert int(plain[-1][3].sum().item()) > 0


def test_python_checks(torch_cuda):
    torch = torch_cuda
    from vad_amd.stream_segments import StreamSegmenter
    seg = StreamSegmenter(4, hops_per_step=2, audio_dtype=torch.int16)
    lab = torch.zeros((2, 4), dtype=torch.uint8, device="cuda")
    hop = torch.zeros((2, 4, 160), dtype=torch.int16, device="cuda")
    with pytest.raises(TypeError, match="uint8"):
        seg.push(lab.to(torch.int32), hop)
    with pytest.raises(TypeError, match="CUDA"):
        seg.push(lab.cpu(), hop)
    with pytest.raises(ValueError, match="shape"):
        seg.push(lab[:, :3], hop)
    with pytest.raises(ValueError, match="shape"):
        seg.push(torch.zeros((3, 4), dtype=torch.uint8, device="cuda"), hop)
    with pytest.raises(TypeError, match="int16"):
        seg.push(lab, hop.float())
    with pytest.raises(ValueError, match="shape"):
        seg.push(lab, hop[:, :, :100])
    with pytest.raises(ValueError, match="contiguous"):
        seg.push(lab, torch.zeros((2, 4, 320), dtype=torch.int16, device="cuda")[:, :, ::2])
    one = StreamSegmenter(4, audio_dtype=torch.float32)
    v, n = one.push(lab[0], hop[0].float())  # (S,) and (S, H) for K = 1
    assert tuple(v.shape) == (1, 4, 160) and tuple(n.shape) == (1, 4)
