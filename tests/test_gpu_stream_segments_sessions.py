"""The sessions form of the streaming segmenter on the device
(stream_segments_sessions_kernel / stream_segments_op_sessions_kernel,
StreamSegmenter(sessions=True), StreamBatch.segmenter(sessions=True)) against
the host model of tests/stream_segments_sessions_reference.py after every
block, against the plain segmenter, and end to end behind a sessions batch.

Every comparison is exact (integers and copied bits), and every output is
pre-filled with a sentinel, so "not written" is checked as well.  The
workloads are those of the reference module; tests/test_stream_segments_sessions_cpu.py
asserts, without a GPU, that they contain the cases these tests are there for.
"""
import numpy as np
import pytest

import stream_segments_sessions_reference as R
from test_gpu_stream_scores import cuda, ffn, torch_cuda, tree_with_scores  # noqa: F401
from test_gpu_stream_sessions import samples

pytestmark = pytest.mark.gpu

SENT = {np.float32: np.float32(-7777.25), np.int16: np.int16(-12345)}
GUARD = -0x0123456789ABCDEF


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x.view(np.uint16) if x.dtype == np.int16 else x


def cfg_of(L, H):
    from vad_amd.config import MfccConfig
    return MfccConfig(frame_size=L, hop=H)


def make(torch, S, K, framing, params, form, dtype, sessions=True, capacity=R.CAPACITY):
    from vad_amd.stream_segments import StreamSegmenter
    dt = None if dtype is None else torch.float32 if dtype == np.float32 else torch.int16
    kw = dict(sessions=True) if sessions else {}
    return StreamSegmenter(S, cfg_of(*framing), max_gap=params[0], min_run=params[1], capacity=capacity,
                           hops_per_step=K, audio_dtype=dt, **R.FORMS[form], **kw)


def workload(S, K, form, dtype, H):
    seed = R.seed_of(S, K)
    counts, restart = R.schedule(S, K, seed)
    x = R.block_values(S, K, counts, seed, scores="on" in R.FORMS[form], restart=restart)
    hops = None if dtype is None else R.audio_blocks(S, K, len(x), H, dtype, seed)
    return counts, restart, x, hops


def fill_outputs(seg, dtype):
    seg.end_len.fill_(-1)
    if dtype is not None:
        sent = float(SENT[dtype]) if dtype == np.float32 else int(SENT[dtype])
        seg.voiced.fill_(sent), seg.end_voiced.fill_(sent), seg.voiced_len.fill_(-1)


def compare_tables(seg, model, where):
    found = seg.found.cpu().numpy()
    table, ordinal = seg.table.cpu().numpy(), seg.table_session.cpu().numpy()
    for s in range(seg.n):
        want, n = model.table(s), min(len(model.rows[s]), seg.capacity)
        assert found[s] == len(want), (where, s)  # the number found, not the number written
        assert np.array_equal(table[s, :n], want[:n]) and (table[s, n:] == GUARD).all(), (where, s)
        assert np.array_equal(ordinal[s, :n], model.table_session(s)[:n]) and (ordinal[s, n:] == -9).all(), (where, s)


def compare_rows(dev, dev_len, want, want_len, H, dtype, where):
    """Lengths equal; the prefixes copied bit for bit and nothing past them touched."""
    dev_len = dev_len.cpu().numpy()
    assert np.array_equal(dev_len, want_len), (where, dev_len.tolist(), want_len.tolist())
    if dtype is not None:
        keep = np.arange(H)[None, None, :] < want_len[:, :, None]
        full = np.where(keep, want, SENT[dtype]).astype(dtype)
        assert np.array_equal(bits(dev.cpu().numpy()), bits(full)), where


def run_against_model(torch, seg, model, counts, restart, x, hops, dtype, where):
    H = seg.cfg.hop
    seg.table.fill_(GUARD), seg.table_session.fill_(-9)
    for b in range(len(x)):
        fill_outputs(seg, dtype)
        got = seg.push(cuda(x[b]), None if hops is None else cuda(hops[b]), hop_counts=cuda(counts[b]),
                       restart=cuda(restart[b]))
        mv, mn, ev, en = model.push(x[b], None if hops is None else hops[b], counts[b], restart[b])
        assert int(seg.restart.sum().item()) == 0, (where, b)  # every flag consumed
        if dtype is None:
            assert got is None
        else:
            assert got[0] is seg.voiced and got[1] is seg.voiced_len and got[2] is seg.end_voiced and got[3] is seg.end_len
            compare_rows(seg.voiced, seg.voiced_len, mv, mn, H, dtype, (where, b, "push"))
        compare_rows(seg.end_voiced, seg.end_len, ev, en, H, dtype, (where, b, "end"))
        compare_tables(seg, model, (where, b))


@pytest.mark.parametrize("form", list(R.FORMS))
@pytest.mark.parametrize("params", R.SESSION_PARAMS)
@pytest.mark.parametrize("framing", R.SESSION_FRAMINGS)
def test_device_against_model_after_every_block(torch_cuda, framing, params, form):
    """fp32, int16 and events only; the (S, K) of each rotates through S in
    {5, 9} (a partial last workgroup of 4 waves) and K in {1, 3}."""
    torch = torch_cuda
    for dtype in R.DTYPES:
        S, K = R.shape_for(framing, params, form, dtype)
        counts, restart, x, hops = workload(S, K, form, dtype, framing[1])
        seg = make(torch, S, K, framing, params, form, dtype)
        model = R.SessionsSegModel(S, *framing, *params, dtype=dtype or np.int16,
                                   fill=SENT[dtype] if dtype else 0, **R.FORMS[form])
        assert seg.flush_rows == model.F
        run_against_model(torch, seg, model, counts, restart, x, hops, dtype, (framing, params, form, dtype, S, K))
        # the plain flush entry ends whatever still runs (the CPU test counts its cases after this flush too)
        if dtype is not None:
            seg.flush_voiced.fill_(float(SENT[dtype]) if dtype == np.float32 else int(SENT[dtype]))
            seg.flush_len.fill_(-1)
        flushed = seg.flush()
        mv, mn = model.flush(audio=dtype is not None)
        if dtype is not None:
            compare_rows(flushed[0], flushed[1], mv, mn, framing[1], dtype, "flush")
        compare_tables(seg, model, "flush")
        assert int(seg.found.max().item()) > seg.capacity  # a table overflowed, and nothing was written past it
        got = seg.session_segments()
        for s in range(S):
            n = min(len(model.rows[s]), seg.capacity)
            flat = [(o, tuple(r)) for o, rows in got[s] for r in rows.tolist()]
            assert flat == [(r[0], r[1:]) for r in model.rows[s][:n]], s
            assert [o for o, _ in got[s]] == sorted({r[0] for r in model.rows[s][:n]}), s


@pytest.mark.parametrize("form", list(R.FORMS))
@pytest.mark.parametrize("K", [1, 3])
def test_every_form_in_the_partial_workgroup(torch_cuda, K, form):
    """S = 9 with both K, crossed with every form and fp32, int16, events only
    (the rotation of the test above does not cross them)."""
    torch = torch_cuda
    S, framing, params = 9, (8, 3), (2, 3)
    for dtype in R.DTYPES:
        counts, restart, x, hops = workload(S, K, form, dtype, framing[1])
        seg = make(torch, S, K, framing, params, form, dtype)
        model = R.SessionsSegModel(S, *framing, *params, dtype=dtype or np.int16,
                                   fill=SENT[dtype] if dtype else 0, **R.FORMS[form])
        run_against_model(torch, seg, model, counts, restart, x, hops, dtype, (form, dtype, S, K))
        assert int(seg.found.sum().item()) > 0


@pytest.mark.parametrize("form", list(R.FORMS))
@pytest.mark.parametrize("S,K", [(5, 3), (9, 1)])
def test_full_counts_and_no_restart_equal_the_plain_segmenter(torch_cuda, S, K, form):
    torch = torch_cuda
    framing, params = (400, 160), (2, 3)
    for dtype in (np.float32, np.int16):
        counts, restart, x, hops = workload(S, K, form, dtype, framing[1])
        a = make(torch, S, K, framing, params, form, dtype, capacity=8)
        b = make(torch, S, K, framing, params, form, dtype, sessions=False, capacity=8)
        for blk in range(len(x)):
            for seg in (a, b):
                seg.voiced.fill_(3), seg.voiced_len.fill_(-1)
            a.end_len.fill_(-1)
            ra = a.push(cuda(x[blk]), cuda(hops[blk]))  # hop_counts as built: K
            rb = b.push(cuda(x[blk]), cuda(hops[blk]))
            for name in ("state", "history", "table", "found", "voiced", "voiced_len"):
                p, q = getattr(a, name), getattr(b, name)
                assert torch.equal(p.view(torch.uint8), q.view(torch.uint8)), (form, dtype, blk, name)
            assert len(ra) == 4 and len(rb) == 2 and int(a.end_len.abs().sum().item()) == 0
        fa, fb = a.flush(), b.flush()  # the same entry for both
        for p, q in ((a.table, b.table), (a.found, b.found), (a.state, b.state), (fa[1], fb[1])):
            assert torch.equal(p.view(torch.uint8), q.view(torch.uint8)), (form, dtype, "flush")
        assert int(a.found.sum().item()) > 0 and int(a.table_session.abs().sum().item()) == 0  # every row in session 0


@pytest.mark.parametrize("form", ["labels", "op_scores"])
def test_a_stalled_stream_keeps_every_byte(torch_cuda, form):
    torch = torch_cuda
    S, K, framing, params, dtype = 9, 3, (8, 3), (2, 3), np.int16
    counts, restart, x, hops = workload(S, K, form, dtype, framing[1])
    seg = make(torch, S, K, framing, params, form, dtype, capacity=16)
    for b in range(8):
        seg.push(cuda(x[b]), cuda(hops[b]), hop_counts=cuda(np.full(S, K, np.int32)))
    stalled = [1, 4, 8]  # the last one in the partial workgroup
    c = np.full(S, K, np.int32)
    c[stalled] = [0, -1, 0]
    names = ("state", "history", "table", "found", "table_session")
    before = {n: getattr(seg, n).clone() for n in names}
    fill_outputs(seg, dtype)
    seg.push(cuda(x[8]), cuda(hops[8]), hop_counts=cuda(c))
    for n in names:
        p, q = getattr(seg, n).view(torch.uint8), before[n].view(torch.uint8)
        assert torch.equal(p[stalled], q[stalled]), n
    assert not torch.equal(seg.state, before["state"])  # the others moved
    n = seg.voiced_len.cpu().numpy()
    assert (n[:, stalled] == 0).all() and int(seg.end_len.abs().sum().item()) == 0
    v = seg.voiced.cpu().numpy()
    assert (v[:, stalled] == SENT[dtype]).all()


@pytest.mark.parametrize("form", ["labels", "op_labels"])
def test_flush_then_a_restart_flag_makes_the_stream_live_again(torch_cuda, form):
    torch = torch_cuda
    S, K, framing, params, dtype = 5, 3, (8, 3), (2, 3), np.float32
    counts, restart, x, hops = workload(S, K, form, dtype, framing[1])
    seg = make(torch, S, K, framing, params, form, dtype, capacity=32)
    model = R.SessionsSegModel(S, *framing, *params, dtype=dtype, fill=SENT[dtype], **R.FORMS[form])
    seg.table.fill_(GUARD), seg.table_session.fill_(-9)
    full, none = np.full(S, K, np.int32), np.zeros(S, np.uint8)
    for b in range(6):
        seg.push(cuda(x[b]), cuda(hops[b]), hop_counts=cuda(full), restart=cuda(none))
        model.push(x[b], hops[b], full, none)
    seg.flush_voiced.fill_(float(SENT[dtype])), seg.flush_len.fill_(-1)
    fv, fn = seg.flush()
    mv, mn = model.flush()
    compare_rows(fv, fn, mv, mn, framing[1], dtype, "flush")
    compare_tables(seg, model, "flush")
    # ended: hops change nothing; then streams 0 and 3 are restarted, the others stay ended
    again = np.array([1, 0, 0, 1, 0], np.uint8)
    for b, flags in ((6, none), (7, again), (8, none), (9, none), (10, none), (11, none)):
        fill_outputs(seg, dtype)
        seg.push(cuda(x[b]), cuda(hops[b]), hop_counts=cuda(full), restart=cuda(flags))
        mv, mn, ev, en = model.push(x[b], hops[b], full, flags)
        compare_rows(seg.voiced, seg.voiced_len, mv, mn, framing[1], dtype, (b, "push"))
        compare_rows(seg.end_voiced, seg.end_len, ev, en, framing[1], dtype, (b, "end"))
        assert (en == 0).all()  # an ended stream has nothing to end
        compare_tables(seg, model, b)
    seg.flush_voiced.fill_(float(SENT[dtype])), seg.flush_len.fill_(-1)
    fv, fn = seg.flush()
    mv, mn = model.flush()
    compare_rows(fv, fn, mv, mn, framing[1], dtype, "second flush")
    compare_tables(seg, model, "second flush")
    assert {r[0] for r in model.rows[0] + model.rows[3]} == {0, 1}  # both sessions of the restarted streams gave rows


def test_a_flag_set_once_restarts_once_under_graph_replay(torch_cuda):
    torch = torch_cuda
    S, K, framing, params, dtype, form = 5, 3, (8, 3), (0, 0), np.int16, "labels"
    counts, restart, x, hops = workload(S, K, form, dtype, framing[1])
    seg = make(torch, S, K, framing, params, form, dtype, capacity=32)
    model = R.SessionsSegModel(S, *framing, *params, dtype=dtype, fill=SENT[dtype])
    lab = torch.zeros((K, S), dtype=torch.uint8, device="cuda")
    hop = torch.zeros((K, S, framing[1]), dtype=torch.int16, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        seg.push(lab, hop)  # warm up: code objects loaded before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    seg.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        seg.push(lab, hop)
    seg.reset()
    seg.table.fill_(GUARD), seg.table_session.fill_(-9)
    full, none = np.full(S, K, np.int32), np.zeros(S, np.uint8)
    flags = np.array([0, 1, 0, 1, 1], np.uint8)
    for b in range(9):
        lab.copy_(cuda(x[b])), hop.copy_(cuda(hops[b]))
        r = flags if b == 5 else none
        if b == 5:
            seg.restart.copy_(cuda(flags))  # set once; replays 5, 6 and 7 follow
        fill_outputs(seg, dtype)
        graph.replay()
        mv, mn, ev, en = model.push(x[b], hops[b], full, r)
        assert int(seg.restart.sum().item()) == 0, b
        compare_rows(seg.voiced, seg.voiced_len, mv, mn, framing[1], dtype, (b, "push"))
        compare_rows(seg.end_voiced, seg.end_len, ev, en, framing[1], dtype, (b, "end"))
        compare_tables(seg, model, b)
    ordinal = seg.state.view(torch.int32)[:, 30].cpu().tolist()  # pad[0] of the 128-byte state
    assert ordinal == flags.tolist()  # one restart each, not three


# ---------------------------------------------------------------------------
# end to end: a sessions batch and its segmenter against a plain batch and a
# plain segmenter run session by session
# ---------------------------------------------------------------------------
def plain_session(torch, sb, seg, hops, block_of):
    """One session through a one-stream plain batch and segmenter: rows, voiced."""
    sb.reset(), seg.reset()
    parts = []
    for h in hops:
        sb.inputs.copy_(cuda(h).view_as(sb.inputs))
        sb.step()
        v, n = seg.push(block_of(sb), sb.inputs)
        parts.append(v[0, 0, :int(n[0, 0].item())].cpu().numpy().copy())
    fv, fn = seg.flush()
    fv, fn = fv.cpu().numpy(), fn.cpu().numpy()
    parts += [fv[f, 0, :fn[f, 0]] for f in range(len(fn))]
    return seg.segments()[0], np.concatenate(parts) if parts else np.zeros(0, np.int16)


@pytest.mark.parametrize("name,scored", [("ffn", False), ("tree", False), ("ffn", True)])
def test_end_to_end_behind_a_sessions_batch(torch_cuda, name, scored):
    torch = torch_cuda
    from vad_amd.stream import StreamBatch
    S, K, H = 5, 3, 160
    clf = tree_with_scores() if name == "tree" else ffn("bl13")
    sb = StreamBatch(S, clf, sessions=True, hops_per_step=K, input_dtype=torch.int16, scores=scored)
    counts, restart = R.schedule(S, K, R.seed_of(S, K))
    x = samples(len(counts), K, S)
    # the operating point comes from a dry run of the workload, so that both decisions occur whatever the
    # classifier makes of these samples: the commonest label is the active one, the median score is `on`
    seen = []
    for b in range(len(counts)):
        sb.inputs.copy_(cuda(x[b]))
        sb.step_block(hop_counts=cuda(counts[b]), restart=cuda(restart[b]))
        seen.append((sb.score_block if scored else sb.label_block).cpu().numpy().copy())
    seen = np.concatenate(seen).reshape(-1)
    sb.reset()
    kw = dict(max_gap=1, min_run=2, capacity=64)
    if scored:
        on = float(np.clip(np.round(np.median(seen[np.isfinite(seen)]), 3), 0.05, 0.95))
        kw.update(on=on, off=on - 0.02, pad=(1, 1))
    else:
        kw.update(active=int(np.bincount(seen[seen < 254]).argmax()))
    seg = sb.segmenter(sessions=True, **kw)
    assert seg.hop_counts is sb.hop_counts and seg.restart is not sb.restart and seg.sessions
    block_of = (lambda b: b.score_block) if scored else (lambda b: b.label_block)
    n = R.taken(counts, K)
    # per stream the sessions: [ordinal, hops, device voiced chunks]
    sessions = [[[0, [], []]] for _ in range(S)]
    for b in range(len(counts)):
        sb.inputs.copy_(cuda(x[b]))
        sb.step_block(hop_counts=cuda(counts[b]), restart=cuda(restart[b]))
        v, vl, ev, el = seg.push(block_of(sb), sb.inputs)  # the whole loop: no count or flag is passed again
        assert int(seg.restart.sum().item()) == 0 and int(sb.restart.sum().item()) == 0
        v, vl, ev, el = v.cpu().numpy(), vl.cpu().numpy(), ev.cpu().numpy(), el.cpu().numpy()
        for s in range(S):
            if restart[b, s]:
                sessions[s][-1][2] += [ev[f, s, :el[f, s]] for f in range(len(el))]
                sessions[s].append([sessions[s][-1][0] + 1, [], []])
            else:
                assert (el[:, s] == 0).all()
            sessions[s][-1][1] += [x[b, k, s] for k in range(n[b, s])]
            sessions[s][-1][2] += [v[k, s, :vl[k, s]].copy() for k in range(K)]
            assert (vl[n[b, s]:, s] == 0).all()
    fv, fn = seg.flush()
    fv, fn = fv.cpu().numpy(), fn.cpu().numpy()
    got = [dict(g) for g in seg.session_segments()]
    assert int(seg.found.max().item()) <= seg.capacity
    one = StreamBatch(1, clf, input_dtype=torch.int16, scores=scored)
    one_seg = one.segmenter(**kw)
    n_rows = n_sessions = 0
    for s in range(S):
        sessions[s][-1][2] += [fv[f, s, :fn[f, s]] for f in range(len(fn))]
        for ordinal, hops, chunks in sessions[s]:
            rows, voiced = plain_session(torch, one, one_seg, hops, block_of)
            where = (name, scored, s, ordinal, len(hops))
            assert np.array_equal(got[s].get(ordinal, np.zeros((0, 2), np.int64)), rows), where
            mine = np.concatenate(chunks) if chunks else np.zeros(0, np.int16)
            assert np.array_equal(mine, voiced), where
            n_rows += len(rows)
            n_sessions += len(rows) > 0
    print(f"end to end ({name}, scores={scored}): {n_rows} rows in {n_sessions} sessions")
    assert n_rows > 0


def test_python_checks(torch_cuda):
    torch = torch_cuda
    from vad_amd.stream import StreamBatch
    from vad_amd.stream_segments import StreamSegmenter
    S, K = 4, 2
    seg = StreamSegmenter(S, hops_per_step=K, audio_dtype=torch.int16, sessions=True)
    lab = torch.zeros((K, S), dtype=torch.uint8, device="cuda")
    hop = torch.zeros((K, S, 160), dtype=torch.int16, device="cuda")
    c, r = torch.ones(S, dtype=torch.int32, device="cuda"), torch.zeros(S, dtype=torch.uint8, device="cuda")
    for kw in (dict(hop_counts=c.long()), dict(hop_counts=c[:3]), dict(hop_counts=c.cpu()), dict(restart=r.int()),
               dict(restart=r[:2]), dict(restart=r.cpu()), dict(hop_counts=[1] * S)):
        with pytest.raises(ValueError, match="must be a CUDA"):
            seg.push(lab, hop, **kw)
    seg.push(lab, hop, hop_counts=c, restart=r)
    assert seg.hop_counts.tolist() == [1] * S
    plain = StreamSegmenter(S, hops_per_step=K, audio_dtype=torch.int16)
    for kw in (dict(hop_counts=c), dict(restart=r)):
        with pytest.raises(ValueError, match="sessions=True"):
            plain.push(lab, hop, **kw)
    with pytest.raises(ValueError, match="sessions=True"):
        StreamBatch(S, ffn("bl13")).segmenter(sessions=True)
    sb = StreamBatch(S, ffn("bl13"), sessions=True)
    with pytest.raises(ValueError, match="one window per label row"):
        sb.segmenter()
    held = sb.segmenter(sessions=True)
    sb.step(torch.zeros((S, 160), device="cuda"), restart=torch.ones(S, dtype=torch.uint8, device="cuda"))
    assert held.restart.tolist() == [1] * S  # handed on; the batch's own flag is consumed by the hop kernel
    del held
    sb.step(torch.zeros((S, 160), device="cuda"), restart=r)  # a dropped segmenter is not held on to
