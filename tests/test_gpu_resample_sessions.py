"""The sessions form of the stream resampler on the device
(resample_stream_sessions_kernel, vad_amd.resample.SessionStreamResampler,
StreamBatch.resampler) against the plain StreamResampler: every comparison is
torch.equal on the bits, every output is pre-filled with a sentinel so that
"not written" is checked too.  The workload is tests/resample_sessions_reference.py's
script; tests/test_resample_sessions_cpu.py asserts, without a GPU, that it
holds the cases these tests are there for."""
import ctypes
import os

import numpy as np
import pytest

import resample_sessions_reference as R

pytestmark = pytest.mark.gpu

S, K, BLOCKS = 6, 3, 12
PAIRS = [("float32", "float32"), ("float32", "int16"), ("int16", "float32"), ("int16", "int16")]
SENT = {"float32": -7777.25, "int16": -12345}
HOP_MAX = max(R.hop_in_of(r) for r in R.RATES)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(t):
    import torch
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(scope="module")
def workload():
    counts, restart, rate = R.script(S, K, BLOCKS)
    return counts, restart, rate, R.audio(BLOCKS, K, S, HOP_MAX), R.session_rows(counts, restart, rate, len(R.RATES), K)


_PLAIN = {}


def plain_rows(torch, rate, idt, odt, hops):
    """The rows a freshly reset one-stream, K = 1 StreamResampler writes for these hops, (n, 160)."""
    from vad_amd import resample as V
    key = (rate, idt, odt)
    if key not in _PLAIN:
        _PLAIN[key] = V.StreamResampler(1, rate, input_dtype=getattr(torch, idt), out_dtype=getattr(torch, odt))
    p = _PLAIN[key]
    p.reset()
    rows = [p.step_block(h.reshape(1, 1, -1)).clone()[0, 0] for h in hops]
    return torch.stack(rows) if rows else p.out.new_zeros((0, p.hop_out))


def make(torch, idt, odt, n=S, k=K, rates=R.RATES):
    from vad_amd import resample as V
    rs = V.SessionStreamResampler(n, rates, hops_per_step=k, input_dtype=getattr(torch, idt),
                                  out_dtype=getattr(torch, odt))
    rs.out.fill_(SENT[odt])
    return rs


@pytest.mark.parametrize("idt,odt", PAIRS)
@pytest.mark.parametrize("rate", [8000, 48000, 44100])
def test_one_rate_full_counts_no_restart_equals_the_plain_kernel(torch_cuda, rate, idt, odt):
    torch = torch_cuda
    from vad_amd import resample as V
    n, blocks = 5, 6
    x = cuda(R.audio(blocks, K, n, R.hop_in_of(rate), seed=rate)).to(getattr(torch, idt))
    rs = make(torch, idt, odt, n=n, rates=[rate])
    rs.restart.zero_()  # no restart at all: the all-zero state is a fresh stream at rates[0]
    plain = V.StreamResampler(n, rate, hops_per_step=K, input_dtype=getattr(torch, idt), out_dtype=getattr(torch, odt))
    words = n * plain.spec.history
    assert rs.state.numel() == words + 2 * n and plain.state.numel() == words + n
    for b in range(blocks):
        want = plain.step_block(x[b])
        got = rs.step_block(x[b])
        assert torch.equal(bits(got), bits(want)), b
        assert torch.equal(rs.state[:words + n], plain.state), b  # the history bytes and the emitted counts
    assert int(rs.stream_rate.abs().sum().item()) == 0 and (rs.out != 0).any()


@pytest.mark.parametrize("idt,odt", PAIRS)
def test_scripted_sessions_with_mixed_rates(torch_cuda, workload, idt, odt):
    """Every stream and session against a plain resampler of the session's rate
    fed the session's hops; the rows past a stream's count keep the sentinel."""
    torch = torch_cuda
    counts, restart, rate, audio, sessions = workload
    x = cuda(audio).to(getattr(torch, idt))
    rs = make(torch, idt, odt)
    outs = []
    for b in range(BLOCKS):
        rs.out.fill_(SENT[odt])
        rs.step_block(x[b], hop_counts=cuda(counts[b]), restart=cuda(restart[b]), rate=cuda(rate[b]))
        assert int(rs.restart.sum().item()) == 0, b  # every flag consumed
        outs.append(rs.out.clone())
    outs = torch.stack(outs)  # (B, K, S, 160)
    n = np.clip(counts, 0, K)
    for b in range(BLOCKS):
        for s in range(S):
            assert (outs[b, n[b, s]:, s] == SENT[odt]).all(), (b, s)
    checked = 0
    for s in range(S):
        for sess in sessions[s]:
            r = R.RATES[sess["rate"]]
            hops = [x[b, k, s, :R.hop_in_of(r)] for b, k in sess["rows"]]
            got = torch.stack([outs[b, k, s] for b, k in sess["rows"]]) if hops else outs.new_zeros((0, 160))
            want = plain_rows(torch, r, idt, odt, hops)
            assert torch.equal(bits(got), bits(want)), (s, sess["start"], r)
            checked += len(hops)
        assert rs.stream_rate[s].item() == sessions[s][-1]["rate"]
    assert checked == int(n.sum()) > 0


def test_a_stalled_stream_keeps_every_byte(torch_cuda, workload):
    torch = torch_cuda
    x = cuda(workload[3])
    rs = make(torch, "int16", "float32")
    idx = cuda(np.array([0, 3, 2, 1, 3, 2], np.int32))
    full = np.full(S, K, np.int32)
    rs.step_block(x[0], hop_counts=cuda(full), rate=idx)  # the flags of a new resampler are set: the rates are adopted
    rs.step_block(x[1])
    stalled = [1, 4]
    c = full.copy()
    c[stalled] = [0, -1]
    before = rs.state.clone(), rs.history.clone(), rs.emitted.clone(), rs.stream_rate.clone()
    rs.out.fill_(SENT["float32"])
    rs.step_block(x[2], hop_counts=cuda(c))
    assert torch.equal(bits(rs.history[stalled]), bits(before[1][stalled]))
    assert torch.equal(rs.emitted[stalled], before[2][stalled]) and torch.equal(rs.stream_rate, before[3])
    assert (rs.history[stalled] != 0).any() and not torch.equal(rs.state, before[0])  # the others moved
    assert (rs.out[:, stalled] == SENT["float32"]).all()
    moved = [s for s in range(S) if s not in stalled]
    assert (rs.out[:, moved] != SENT["float32"]).all()


def test_restart_and_rate_adoption(torch_cuda, workload):
    torch = torch_cuda
    x = cuda(workload[3])
    rs = make(torch, "int16", "float32")
    full, none = cuda(np.full(S, K, np.int32)), cuda(np.zeros(S, np.uint8))
    first = np.array([3, 3, 0, 2, 1, 3], np.int32)
    rs.step_block(x[0], hop_counts=full, rate=cuda(first))
    assert rs.restart.tolist() == [0] * S and rs.stream_rate.tolist() == first.tolist()
    # another rate index without a flag changes nothing
    other = (first + 1) % len(R.RATES)
    rs.step_block(x[1], restart=none, rate=cuda(other.astype(np.int32)))
    assert rs.stream_rate.tolist() == first.tolist()
    for s in range(S):
        r = R.RATES[first[s]]
        want = plain_rows(torch, r, "int16", "float32", [x[b, k, s, :R.hop_in_of(r)] for b in (0, 1) for k in range(K)])
        assert torch.equal(bits(rs.out[:, s]), bits(want[K:])), s
    # a restart with count 0: the state is fresh, the rate adopted, nothing written
    c = np.full(S, K, np.int32)
    c[[0, 5]] = 0
    flags = np.array([1, 0, 0, 0, 0, 1], np.uint8)
    assert (rs.history[[0, 5]] != 0).any() and (rs.emitted[[0, 5]] != 0).all()
    rs.out.fill_(SENT["float32"])
    rs.step_block(x[2], hop_counts=cuda(c), restart=cuda(flags))
    assert rs.restart.tolist() == [0] * S
    assert (rs.out[:, [0, 5]] == SENT["float32"]).all()
    assert int(rs.history[[0, 5]].abs().sum().item()) == 0 and rs.emitted[[0, 5]].tolist() == [0, 0]
    want_rate = first.copy()
    want_rate[[0, 5]] = other[[0, 5]]
    assert rs.stream_rate.tolist() == want_rate.tolist()
    # and the session that follows is a fresh one at the adopted rate
    rs.step_block(x[3], hop_counts=full)
    for s in (0, 5):
        r = R.RATES[want_rate[s]]
        want = plain_rows(torch, r, "int16", "float32", [x[3, k, s, :R.hop_in_of(r)] for k in range(K)])
        assert torch.equal(bits(rs.out[:, s]), bits(want)), s


def test_a_flag_set_once_restarts_once_under_graph_replay(torch_cuda, workload):
    torch = torch_cuda
    x = cuda(workload[3])
    rs = make(torch, "int16", "float32", rates=[48000, 8000])
    rs.rate_index.copy_(cuda(np.array([0, 1, 0, 1, 0, 1], np.int32)))
    rs.capture()
    assert rs.restart.tolist() == [1] * S  # the warm-up consumed the flags; capture put them back
    outs = []
    for b in range(6):
        rs.inputs.copy_(x[b])
        if b == 2:
            rs.restart.copy_(cuda(np.array([0, 1, 1, 0, 0, 0], np.uint8)))  # set once; replays 2 .. 5 follow
        rs.step_block()
        assert rs.restart.tolist() == [0] * S, b
        outs.append(rs.out.clone())
    for s in range(S):
        r = [48000, 8000][s % 2]
        starts = (0, 2) if s in (1, 2) else (0,)
        for i, b0 in enumerate(starts):
            b1 = starts[i + 1] if i + 1 < len(starts) else 6
            hops = [x[b, k, s, :R.hop_in_of(r)] for b in range(b0, b1) for k in range(K)]
            got = torch.cat([outs[b][:, s] for b in range(b0, b1)])
            assert torch.equal(bits(got), bits(plain_rows(torch, r, "int16", "float32", hops))), (s, b0)


def test_counts_and_rate_indices_are_clamped(torch_cuda, workload):
    torch = torch_cuda
    x = cuda(workload[3])
    a, b = make(torch, "int16", "int16"), make(torch, "int16", "int16")
    n_r = len(R.RATES)
    ca, cb = np.array([-1, K + 2, 1, K, -1, K + 2], np.int32), np.array([0, K, 1, K, 0, K], np.int32)
    ia, ib = np.array([-1, n_r, 2, -1, n_r, 1], np.int32), np.array([0, n_r - 1, 2, 0, n_r - 1, 1], np.int32)
    flags = cuda(np.ones(S, np.uint8))
    for blk in range(3):
        for rs, c, i in ((a, ca, ia), (b, cb, ib)):
            rs.out.fill_(SENT["int16"])
            rs.step_block(x[blk], hop_counts=cuda(c), restart=flags if blk != 1 else None, rate=cuda(i))
        assert torch.equal(a.out, b.out) and torch.equal(a.state, b.state), blk
    assert a.stream_rate.tolist() == ib.tolist()
    assert (a.out[:, [0, 4]] == SENT["int16"]).all() and (a.out[:, [1, 3, 5]] != SENT["int16"]).any()


def test_captured_steps_equal_direct_steps(torch_cuda, workload):
    torch = torch_cuda
    counts, restart, rate, audio, _ = workload
    x = cuda(audio).to(torch.float32)
    direct, cap = make(torch, "float32", "int16"), make(torch, "float32", "int16")
    cap.capture()
    assert cap.graph is not None and torch.equal(cap.state, direct.state) and torch.equal(cap.out, direct.out)
    for b in range(BLOCKS):
        for rs in (direct, cap):
            rs.out.fill_(SENT["int16"])
            rs.step_block(x[b], hop_counts=cuda(counts[b]), restart=cuda(restart[b]), rate=cuda(rate[b]))
        assert torch.equal(cap.out, direct.out) and torch.equal(cap.state, direct.state), b
        assert int(cap.restart.sum().item()) == 0


def test_past_the_grid_cap_and_stale_lds(torch_cuda):
    """S = cap + 3 with K = 1: three workgroups take a second stream, two of
    them at another rate than their first and one at the same; whatever LDS
    held before changes nothing."""
    torch = torch_cuda
    from vad_amd import _lib
    cap = int(_lib.lib().vad_resample_sessions_grid())
    n, rates, blocks = cap + 3, [48000, 8000], 3
    idx = np.arange(n, dtype=np.int32) % 2
    idx[cap:] = 1  # streams 0, 1, 2 (rates 0, 1, 0) share their workgroups with cap, cap + 1, cap + 2 (rate 1)
    x = torch.randint(-20000, 20000, (blocks, 1, n, 480), device="cuda", dtype=torch.int32,
                      generator=torch.Generator(device="cuda").manual_seed(5)).to(torch.int16)

    def run():
        rs = make(torch, "int16", "float32", n=n, k=1, rates=rates)
        rs.rate_index.copy_(cuda(idx))
        return torch.stack([rs.step_block(x[b]).clone() for b in range(blocks)]), rs.state.clone()

    want, want_state = run()
    for s in (0, 1, 2, 3, cap - 2, cap - 1, cap, cap + 1, cap + 2):
        r = rates[idx[s]]
        ref = plain_rows(torch, r, "int16", "float32", [x[b, 0, s, :R.hop_in_of(r)] for b in range(blocks)])
        assert torch.equal(bits(want[:, 0, s]), bits(ref)), s
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_host", "liblds_poison.so")
    if not os.path.exists(so):
        pytest.fail("tests/c_host/liblds_poison.so missing: run __graft_entry__.build()")
    helper = ctypes.CDLL(so)
    helper.lds_poison.argtypes = [ctypes.c_float, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    sink = torch.zeros(1, device="cuda")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for v in (1e30, -1e30, float("nan")):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert helper.lds_poison(v, ctypes.c_void_p(sink.data_ptr()), 4 * n_cu, st) == 0
        got, got_state = run()
        assert torch.equal(bits(got), bits(want)) and torch.equal(got_state, want_state), v
    torch.cuda.synchronize()
    assert sink.item() == 0.0


# ---------------------------------------------------------------------------
# end to end: resampler -> sessions batch -> sessions segmenter against the
# plain chain run session by session
# ---------------------------------------------------------------------------
def loud_audio(blocks, k, n, hop, seed=4100):
    """(B, K, S, hop) int16: a noise floor with louder stretches, so that both classes occur."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 300.0, size=(blocks, k, n, hop))
    x = np.where(rng.random((blocks, k, n, 1)) < 0.4, x * 12.0, x)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("bdt", ["float32", "int16"])
def test_end_to_end_in_front_of_a_sessions_batch(torch_cuda, workload, bdt):
    torch = torch_cuda
    from vad_amd import resample as V
    from vad_amd.ffn import FFNClassifier, TOPOLOGY_BL13, random_layers
    from vad_amd.stream import StreamBatch
    counts, restart, rate, _, sessions = workload
    clf = FFNClassifier(random_layers(TOPOLOGY_BL13, seed=3))
    dt = getattr(torch, bdt)
    x = loud_audio(BLOCKS, K, S, HOP_MAX)
    dx = cuda(x)
    sb = StreamBatch(S, clf, sessions=True, hops_per_step=K, input_dtype=dt)
    rs = sb.resampler(R.RATES, input_dtype=torch.int16)
    assert rs.out is sb.inputs and rs.hop_counts is sb.hop_counts and rs.restart is not sb.restart
    # the active class is the commonest label of a dry run, so that both decisions occur
    seen = []
    for b in range(BLOCKS):
        rs.step_block(dx[b], hop_counts=cuda(counts[b]), restart=cuda(restart[b]), rate=cuda(rate[b]))
        seen.append(sb.step_block().cpu().numpy().copy())
    seen = np.concatenate(seen).reshape(-1)
    sb.reset(), rs.reset()
    kw = dict(max_gap=1, min_run=2, capacity=64, active=int(np.bincount(seen[seen < 254]).argmax()))
    seg = sb.segmenter(sessions=True, **kw)
    n = np.clip(counts, 0, K)
    mine = [[dict(labels=[], chunks=[]) for _ in sessions[s]] for s in range(S)]
    cur = [0] * S
    for b in range(BLOCKS):
        rs.step_block(dx[b], hop_counts=cuda(counts[b]), restart=cuda(restart[b]), rate=cuda(rate[b]))
        sb.step_block()
        v, vl, ev, el = seg.push(sb.label_block, sb.inputs)  # the whole loop
        assert int(rs.restart.sum().item()) == 0 and int(sb.restart.sum().item()) == 0 \
            and int(seg.restart.sum().item()) == 0
        lab, v, vl, ev, el = sb.label_block.cpu().numpy(), v.cpu().numpy(), vl.cpu().numpy(), ev.cpu().numpy(), \
            el.cpu().numpy()
        for s in range(S):
            if restart[b, s]:
                mine[s][cur[s]]["chunks"] += [ev[f, s, :el[f, s]] for f in range(len(el))]
                cur[s] += 1
            else:
                assert (el[:, s] == 0).all()
            mine[s][cur[s]]["labels"] += lab[:n[b, s], s].tolist()
            mine[s][cur[s]]["chunks"] += [v[k, s, :vl[k, s]].copy() for k in range(K)]
            assert (lab[n[b, s]:, s] == 254).all() and (vl[n[b, s]:, s] == 0).all()
    fv, fn = seg.flush()
    fv, fn = fv.cpu().numpy(), fn.cpu().numpy()
    got = [dict(g) for g in seg.session_segments()]
    assert int(seg.found.max().item()) <= seg.capacity
    one = StreamBatch(1, clf, input_dtype=dt)
    one_seg = one.segmenter(**kw)
    one_rs = {r: V.StreamResampler(1, r, input_dtype=torch.int16, out=one.inputs) for r in R.RATES}
    n_rows = n_labels = 0
    for s in range(S):
        mine[s][-1]["chunks"] += [fv[f, s, :fn[f, s]] for f in range(len(fn))]
        assert cur[s] == len(sessions[s]) - 1
        for ordinal, (sess, m) in enumerate(zip(sessions[s], mine[s])):
            r = R.RATES[sess["rate"]]
            one.reset(), one_seg.reset(), one_rs[r].reset()
            labels, parts = [], []
            for b, k in sess["rows"]:
                one_rs[r].step_block(dx[b, k, s, :R.hop_in_of(r)].reshape(1, 1, -1))
                labels.append(int(one.step().item()))
                pv, pn = one_seg.push(one.label_block, one.inputs)
                parts.append(pv[0, 0, :int(pn[0, 0].item())].cpu().numpy().copy())
            pv, pn = one_seg.flush()
            pv, pn = pv.cpu().numpy(), pn.cpu().numpy()
            parts += [pv[f, 0, :pn[f, 0]] for f in range(len(pn))]
            where = (bdt, s, ordinal, r, len(sess["rows"]))
            assert m["labels"] == labels, where
            assert np.array_equal(got[s].get(ordinal, np.zeros((0, 2), np.int64)), one_seg.segments()[0]), where
            a = np.concatenate(m["chunks"]) if m["chunks"] else np.zeros(0, x.dtype)
            w = np.concatenate(parts) if parts else np.zeros(0, x.dtype)
            assert a.dtype == w.dtype and np.array_equal(a.view(np.uint8), w.view(np.uint8)), where
            n_rows += len(one_seg.segments()[0])
            n_labels += len(labels)
    print(f"end to end ({bdt} batch): {n_rows} segment rows over {n_labels} hops")
    assert n_rows > 0 and n_labels == int(n.sum())


def test_python_checks(torch_cuda):
    torch = torch_cuda
    from vad_amd import resample as V
    from vad_amd.ffn import FFNClassifier, TOPOLOGY_BL13, random_layers
    from vad_amd.stream import StreamBatch
    clf = FFNClassifier(random_layers(TOPOLOGY_BL13, seed=3))
    with pytest.raises(ValueError, match="sessions=True"):
        StreamBatch(4, clf).resampler([48000])
    with pytest.raises(ValueError, match="three"):
        StreamBatch(4, clf, kernel="three").resampler([48000])
    for bad in ([], list(range(8000, 8900, 100)), [48000, 48000], [11025], [8000.5], [0]):
        with pytest.raises(ValueError):
            V.SessionStreamResampler(4, bad)
    rs = V.SessionStreamResampler(4, [16000, 8000, 44100], hops_per_step=2)
    assert rs.delays == [0, 20, V.ResampleSpec(44100).delay] and rs.hop_ins == [160, 80, 441] and rs.hop_in == 441
    assert tuple(rs.inputs.shape) == (2, 4, 441) and tuple(rs.out.shape) == (2, 4, 160)
    ok = torch.zeros(4, dtype=torch.int32, device="cuda")
    for kw in (dict(hop_counts=ok.long()), dict(hop_counts=ok[:3]), dict(hop_counts=ok.cpu()), dict(rate=ok.long()),
               dict(rate=[0] * 4), dict(restart=ok), dict(x=torch.zeros((2, 4, 160), device="cuda"))):
        with pytest.raises(ValueError, match="must be a CUDA"):
            rs.step_block(**kw)
    # 16 kHz is the copy, with delay 0
    x = torch.randn((2, 4, 441), device="cuda")
    out = rs.step_block(x)
    assert torch.equal(bits(out), bits(x[:, :, :160]))
