"""The operating point on the live path, on the device: scores out of the hop
kernels (FFN and tree), and the online segmenter with hysteresis and padding
against the clip chain of vad_amd.scores / vad_amd.segments, bit for bit.

Accuracy of the FFN hop scores (test_ffn_hop_scores, measured on an MI355X and
printed by the test): see profiles/stream_scores/bench.json.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

from oracle import vad_oracle as O

import stream_tree_reference as R
from test_stream_scores_cpu import score_walks
from test_stream_segments_cpu import stream_audio

pytestmark = pytest.mark.gpu

L, H = 400, 160  # the reference's framing; the helpers take another as L=, H=


def framing(L, H):
    from vad_amd.config import MfccConfig
    return MfccConfig(frame_size=L, hop=H)


def is_16_chunk(sb):
    """The launcher's rule: a frame past 7 chunks of 64 samples takes the
    16-chunk build of its hop kernel (launch_hop_kernels)."""
    return sb.cfg.frame_size > 7 * 64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---------------------------------------------------------------------------
# the segmenter
# ---------------------------------------------------------------------------
def clip_chain_device(torch, x, clip, g, m, pad, on, off, active=1, L=L, H=H):
    """Rows and voiced samples of one stream from the clip path's kernels."""
    from vad_amd import scores as SC, segments as SG
    lab = SC.score_labels(cuda(x), on, off) if on is not None else cuda(x)
    act = 1 if on is not None else active
    lab = SC.dilate_labels(SG.smooth_labels(lab, g, m, active=act), pad, active=1)
    padded = np.concatenate([clip, np.zeros(1, clip.dtype)])  # the clip entries count frames with a strict >
    seg = SG.label_segments(lab, len(padded), L, H, 0, 0, active=1)
    out, counts = SG.voiced_audio(cuda(padded), seg)
    total = int(counts[1].item())
    return seg.numpy(), int(seg.counts[0].item()), out[:total].cpu().numpy()


def run_segmenter(torch, seg, block, hops, K):
    outs = []
    for t0 in range(0, block.shape[0], K):
        r = seg.push(cuda(block[t0:t0 + K]), None if hops is None else cuda(hops[t0:t0 + K]))
        if r is not None:  # the static outputs: rows [0, k) are this block's
            k = min(K, block.shape[0] - t0)
            outs.append((r[0][:k].cpu().numpy().copy(), r[1][:k].cpu().numpy().copy()))
    r = seg.flush()
    if r is not None:
        outs.append((r[0].cpu().numpy(), r[1].cpu().numpy()))
    return outs


def packed(outs, s, dtype):
    parts = [v[k, s, :n[k, s]] for v, n in outs for k in range(n.shape[0])]
    return np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)


def scores_for(S, T, on, off, seed):
    """(T, S) float32: rows t < 5 NaN (no window yet), then walks; stream 0
    starts with a run at window 0 and the last stream ends with one at the
    last window, so both clamps of the padding are met."""
    rng = np.random.default_rng(seed)
    x = np.full((T, S), np.nan, np.float32)
    x[5:] = score_walks(rng, T - 5, S, on, off)
    x[5:9, 0] = 1.0
    x[T - 3:, S - 1] = 1.0
    return x


CASES = [  # (on, off), (max_gap, min_run), pad
    ((0.6, 0.4), (2, 3), (2, 3)), ((0.5, 0.5), (0, 0), (1, 0)), ((1.0, 0.0), (1, 1), (0, 2)),
    ((0.6, 0.4), (0, 1), (15, 15)), ((0.6, 0.4), (2, 0), (0, 0))]


@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("S,K", [(1, 1), (5, 3), (9, 8), (5, 8)])
def test_segmenter_equals_clip_chain(torch_cuda, S, K, dtype):
    torch = torch_cuda
    from vad_amd.stream_segments import StreamSegmenter
    T = 64
    nd = np.dtype(dtype)
    rng = np.random.default_rng(S * 10 + K)
    hops = stream_audio(T, S, H, nd.type, rng)
    carry = np.zeros((S, L - H), nd)
    clip = np.concatenate([carry, hops.transpose(1, 0, 2).reshape(S, -1)], axis=1)
    for (on, off), (g, m), pad in CASES:
        x = scores_for(S, T, on, off, seed=S + K + pad[0])
        seg = StreamSegmenter(S, max_gap=g, min_run=m, hops_per_step=K, audio_dtype=getattr(torch, dtype), on=on,
                              off=off, pad=pad)
        assert seg.delay == g + max(m, 1) + (L // H - 1) + 1 + pad[0]
        outs = run_segmenter(torch, seg, x, hops, K)
        rows, found = seg.segments(), seg.found.cpu().numpy()
        n_rows = 0
        for s in range(S):
            want, count, voiced = clip_chain_device(torch, x[5:, s], clip[s], g, m, pad, on, off)
            where = (S, K, dtype, on, off, g, m, pad, s)
            assert found[s] == count, where
            assert np.array_equal(rows[s], want), where
            got = packed(outs, s, nd)
            assert got.shape == voiced.shape and np.array_equal(got.view(np.uint8), voiced.view(np.uint8)), where
            n_rows += len(want)
        assert n_rows > 0
        if pad[0] > 0:
            assert rows[0][0, 0] == 2 * H  # the run at window 0: its padded start stops at window 0
        if pad[1] > 0:
            assert rows[S - 1][-1, 1] == (T - 6 + 2) * H + L  # and the one at the last window at N - 1


@pytest.mark.parametrize("dtype", ["float32", "int16", None])
@pytest.mark.parametrize("S,K", [(5, 3), (9, 8)])
def test_op_kernel_equals_label_kernel_block_by_block(torch_cuda, S, K, dtype):
    """Scores in {0, 1}, on = off = 0.5, no padding: the label segmenter on
    labels = scores >= 0.5, after every block and after the flush."""
    torch = torch_cuda
    from vad_amd.stream_segments import StreamSegmenter
    T = 64
    rng = np.random.default_rng(77 + S)
    x = (rng.random((T, S)) < 0.45).astype(np.float32)
    x[:, 0] = np.arange(T) % 2
    lab = (x >= 0.5).astype(np.uint8)
    dt = None if dtype is None else getattr(torch, dtype)
    hops = None if dtype is None else stream_audio(T, S, H, np.dtype(dtype).type, rng)
    a = StreamSegmenter(S, max_gap=1, min_run=2, hops_per_step=K, audio_dtype=dt, on=0.5)
    b = StreamSegmenter(S, max_gap=1, min_run=2, hops_per_step=K, audio_dtype=dt)
    assert a._events_fn == "vad_stream_segments_op" and b._events_fn == "vad_stream_segments"
    assert a.delay == b.delay and a.flush_rows == b.flush_rows
    for t0 in range(0, T, K):
        h = None if hops is None else cuda(hops[t0:t0 + K])
        ra, rb = a.push(cuda(x[t0:t0 + K]), h), b.push(cuda(lab[t0:t0 + K]), h)
        k = min(K, T - t0)
        assert torch.equal(a.table, b.table) and torch.equal(a.found, b.found), t0
        if hops is not None:
            assert torch.equal(ra[1][:k], rb[1][:k]), t0
            va, vb = ra[0][:k].cpu().numpy(), rb[0][:k].cpu().numpy()
            n = ra[1][:k].cpu().numpy()
            keep = np.arange(H)[None, None, :] < n[:, :, None]
            assert np.array_equal(va[keep].view(np.uint8), vb[keep].view(np.uint8)), t0
    ra, rb = a.flush(), b.flush()
    assert torch.equal(a.table, b.table) and torch.equal(a.found, b.found) and int(a.found.sum()) > 0
    if hops is not None:
        assert torch.equal(ra[1], rb[1])
        n = ra[1].cpu().numpy()
        keep = np.arange(H)[None, None, :] < n[:, :, None]
        assert np.array_equal(ra[0].cpu().numpy()[keep].view(np.uint8), rb[0].cpu().numpy()[keep].view(np.uint8))


def test_labels_with_padding_only(torch_cuda):
    torch = torch_cuda
    from vad_amd.stream_segments import StreamSegmenter
    S, K, T, g, m = 5, 3, 64, 1, 2
    rng = np.random.default_rng(5)
    lab = rng.integers(0, 3, size=(T, S)).astype(np.uint8)
    lab[:5] = 255
    lab[5:8, 0] = 2
    lab[T - 2:, S - 1] = 2
    hops = stream_audio(T, S, H, np.int16, rng)
    clip = np.concatenate([np.zeros((S, L - H), np.int16), hops.transpose(1, 0, 2).reshape(S, -1)], axis=1)
    for pad in ((2, 3), (0, 1), (4, 0)):
        seg = StreamSegmenter(S, max_gap=g, min_run=m, active=2, hops_per_step=K, audio_dtype=torch.int16, pad=pad)
        assert seg._events_fn == "vad_stream_segments_op" and seg.on is None
        outs = run_segmenter(torch, seg, lab, hops, K)
        rows, found = seg.segments(), seg.found.cpu().numpy()
        for s in range(S):
            want, count, voiced = clip_chain_device(torch, lab[5:, s], clip[s], g, m, pad, None, None, active=2)
            assert found[s] == count and np.array_equal(rows[s], want), (pad, s)
            assert np.array_equal(packed(outs, s, np.int16), voiced), (pad, s)
        assert sum(len(r) for r in rows) > 0


# ---------------------------------------------------------------------------
# FFN hop scores
# ---------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def ffn(name, arith="split_f16"):
    from vad_amd.ffn import FFNClassifier, TOPOLOGY_BL13, random_layers
    if name == "bl13":
        return FFNClassifier(random_layers(TOPOLOGY_BL13, seed=3), arith=arith)
    w = np.load(os.path.join(GOLDEN, "ffn.npz"), allow_pickle=False)
    return FFNClassifier([(w[f"ref39_W{i}"], w[f"ref39_b{i}"]) for i in range(4)], arith=arith)


@functools.lru_cache(maxsize=None)
def audio(S, T, seed=1200, L=L, H=H):
    keep = L - H
    clips = np.stack([O.synth_clip(H * T + keep, seed=seed + s)[:H * T + keep] for s in range(S)])
    carry = np.ascontiguousarray(clips[:, :keep])
    hops = np.ascontiguousarray(np.stack([clips[:, keep + H * t: keep + H * (t + 1)] for t in range(T)]))
    return carry.astype(np.float32), hops.astype(np.float32)


def batch(torch, S, clf, carry, **kw):
    from vad_amd.stream import StreamBatch
    sb = StreamBatch(S, clf, **kw)
    sb.prime(cuda(carry))
    return sb


def run_pair(torch, clf, S, K, T, dtype, graph, active, record_seq=False, L=L, H=H, **kw):
    """A scored and an unscored batch on the same hops: labels (T, S), scores
    (T, S), and the state equalities checked after every block."""
    dt = getattr(torch, dtype)
    carry, hops = audio(S, T, L=L, H=H)
    kw["cfg"] = framing(L, H)
    dh = cuda(hops).to(dt)
    a = batch(torch, S, clf, carry, hops_per_step=K, input_dtype=dt, scores=True, active=active, **kw)
    b = batch(torch, S, clf, carry, hops_per_step=K, input_dtype=dt, **kw)
    assert torch.isnan(a.score_block).all()
    if graph:
        a.capture(), b.capture()
        if K == 1:
            assert a.graph_direct  # still one kernel node
    labs, scs, seq = [], [], []
    for t0 in range(0, T, K):
        blk = dh[t0:t0 + K]
        for sb in (a, b):
            if K == 1:
                sb.step(blk[0])
            elif graph:
                sb.inputs.copy_(blk)
                sb.step_block()
            else:
                sb.step_block(blk)
        assert torch.equal(a.label_block, b.label_block), t0
        assert torch.equal(a.frames, b.frames) and torch.equal(a.ring, b.ring) and torch.equal(a.count, b.count), t0
        labs.append(a.label_block.clone()), scs.append(a.score_block.clone())
        if record_seq:
            seq.append(a.ring[:, t0 % 5, :].clone())
    lab, sc = torch.cat(labs).cpu().numpy(), torch.cat(scs).cpu().numpy()
    assert np.array_equal(np.isnan(sc), lab == 255) and (lab[:5] == 255).all() and (lab[5:] != 255).all()
    return lab, sc, (torch.stack(seq, dim=1).contiguous() if record_seq else None), a


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("net,S,K", [("bl13", 5, 8), ("ref39", 9, 3), ("bl13", 1, 1)])
def test_ffn_hop_scores_labels_and_state(torch_cuda, net, S, K, dtype, graph):
    torch = torch_cuda
    clf = ffn(net)
    n_cls = clf.layers[-1][1].shape[0]
    T = 24
    first = None
    for active in range(n_cls):
        lab, sc, _, sb = run_pair(torch, clf, S, K, T, dtype, graph, active)
        ok = ~np.isnan(sc)
        assert (sc[ok] >= 0).all() and (sc[ok] <= 1).all()
        if n_cls == 2:
            assert (sc[ok & (lab == active)] >= 0.5).all() and (sc[ok & (lab != active)] <= 0.5).all()
        first = sc if first is None else first
    if n_cls == 2:  # the two classes' scores sum to one, up to the rounding of each
        assert np.abs(first[5:] + sc[5:] - 1).max() <= 4 * 2.0 ** -24
    sb.reset()
    assert torch.isnan(sb.score_block).all() and (sb.label_block == 255).all()


@pytest.mark.parametrize("net", ["bl13", "ref39"])
def test_ffn_hop_scores_accuracy(torch_cuda, net):
    """Against the float64 forward and softmax of the oracle on the float64
    analyser features of the rows the hop kernel recorded.  Yardstick: the clip
    path's exact-f32 scores on the same rows against the same value.  Bound:
    twice the yardstick (another fp32 summation order) plus 8 * 2^-24 (the
    shared softmax function's own bound in test_ffn_scores)."""
    ffn_scores_accuracy(torch_cuda, net, 9, 40, "float32")


def ffn_scores_accuracy(torch, net, S, T, dtype, L=L, H=H):
    from vad_amd import scores as SC
    from vad_amd.plan import window_logits
    clf, exact = ffn(net), ffn(net, "f32")
    n_cls = clf.layers[-1][1].shape[0]
    worst_hop = worst_clip = 0.0
    for active in range(n_cls):
        lab, sc, seq, sb = run_pair(torch, clf, S, 1, T, dtype, False, active, record_seq=True, L=L, H=H)
        for s in range(S):
            x = O.analyser_features(seq[s].cpu().numpy().astype(np.float64))[:, :clf.layers[0][0].shape[0]]
            _, p = O.ffn_forward(x, clf.layers)
            want = p[:, active]
            _, logits = window_logits(exact.plan, seq[s])
            clip = SC.scores_from_logits(logits, active).cpu().numpy().astype(np.float64)
            got = sc[5:, s].astype(np.float64)
            assert got.shape == want.shape == clip.shape
            worst_hop = max(worst_hop, float(np.abs(got - want).max()))
            worst_clip = max(worst_clip, float(np.abs(clip - want).max()))
    print(f"\n{net}: max |hop score - f64| = {worst_hop:.3e} = {worst_hop * 2 ** 24:.2f} * 2^-24; "
          f"clip exact-f32 yardstick {worst_clip:.3e} = {worst_clip * 2 ** 24:.2f} * 2^-24")
    assert worst_hop <= 2 * worst_clip + 8 * 2.0 ** -24, (net, worst_hop, worst_clip)
    return sb


def test_scored_hop_entries_refuse(torch_cuda):
    """The refusals that read a plan: active outside the classes, a null
    scores, a tree plan without a score table, overlapping score rows."""
    torch = torch_cuda
    from vad_amd import _lib
    lib = _lib.lib()
    S, K = 4, 2
    carry, hops = audio(S, K)
    for clf, name, walk in ((ffn("bl13"), "vad_stream_hops_scores", ()), (tree_with_scores(), "vad_stream_hops_tree_scores", (0,))):
        sb = batch(torch, S, clf, carry, hops_per_step=K, scores=True)
        dh = cuda(hops)

        def call(active=1, scores=_lib.ptr(sb.score_block), stride=S, plan=None):
            return getattr(lib, name)(sb.plan.handle, (plan or clf.plan).handle, _lib.ptr(sb.frames), L, L, _lib.ptr(dh), H, H,
                                      S, K, S * H, _lib.ptr(sb.ring), _lib.ptr(sb.count), _lib.ptr(sb.label_block), S,
                                      *walk, active, scores, stride, _lib.stream_ptr())
        if walk:
            clf.plan_with_scores()
            bare = R.classifier(R.fixture_tree())
            assert lib.vad_tree_plan_score_classes(bare.plan.handle) == 0
            assert call(plan=bare.plan) == -1  # no score table
            assert lib.vad_tree_plan_score_classes(clf.plan.handle) == 2
        for kw in (dict(active=-1), dict(active=2), dict(scores=None), dict(stride=S - 1)):
            assert call(**kw) == -1, (name, kw)
        assert call() == 0
    torch.cuda.synchronize()
    from vad_amd.stream import StreamBatch
    with pytest.raises(ValueError):
        StreamBatch(S, ffn("bl13"), scores=True, kernel="three")
    with pytest.raises(ValueError):
        StreamBatch(S, ffn("bl13"), scores=True, active=2)
    with pytest.raises(ValueError):
        StreamBatch(S, R.classifier(R.fixture_tree()), scores=True)  # no node values to score with
    with pytest.raises(ValueError):
        StreamBatch(S, ffn("bl13")).segmenter(on=0.5)


# ---------------------------------------------------------------------------
# tree hop scores
# ---------------------------------------------------------------------------
def with_counts(table):
    """A TreeClassifier of `table` with class counts per node whose largest
    share is the node's class (a leaf share above one half is its label)."""
    from vad_amd.tree import TreeClassifier
    leaf = np.asarray(table["leaf"])
    n = len(leaf)
    rng = np.random.default_rng(n)
    n_cls = int(leaf.max()) + 1
    value = rng.integers(0, 40, size=(n, n_cls))
    top = value.sum(axis=1) + rng.integers(1, 9, size=n)  # strictly more than all the others together
    value[np.arange(n), np.maximum(leaf, 0)] = top
    return TreeClassifier(*(table[k] for k in R.KEYS), table["n_features"], value=value)


@functools.lru_cache(maxsize=None)
def tree_with_scores():
    return with_counts(R.fixture_tree())


def check_tree_scores(torch, clf, S, K, T, dtype, graph, walk, L=L, H=H):
    from vad_amd import scores as SC
    for active in (0, 1):
        lab, sc, seq, sb = run_pair(torch, clf, S, K, T, dtype, graph, active, record_seq=(K == 1), tree_walk=walk,
                                    L=L, H=H)
        table = clf.score_table(active)
        assert ((sc[5:] > 0.5) == (lab[5:] == active)).all()
        assert np.isin(sc[5:], table).all()
        if seq is not None:
            for s in range(S):
                want = SC.tree_window_scores(clf, seq[s], active=active).cpu().numpy()
                assert np.array_equal(sc[5:, s].view(np.uint32), want.view(np.uint32)), (walk, active, s)
    check_tree_scores.last = sb
    return sc


@pytest.mark.parametrize("walk", ["auto", "global"])
@pytest.mark.parametrize("S,K,dtype,graph", [(5, 1, "float32", False), (9, 1, "int16", True), (1, 1, "float32", True),
                                             (5, 8, "int16", False), (9, 3, "float32", True)])
def test_tree_hop_scores(torch_cuda, S, K, dtype, graph, walk):
    torch = torch_cuda
    T = 24
    sc = check_tree_scores(torch, tree_with_scores(), S, K, T, dtype, graph, walk)
    if K > 1:  # blocks give the one-hop steps' scores
        one = check_tree_scores(torch, tree_with_scores(), S, 1, T, dtype, False, walk)
        assert np.array_equal(sc.view(np.uint32), one.view(np.uint32))


# ---------------------------------------------------------------------------
# the 16-chunk builds of the scored kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("which", ["ffn", "tree"])
@pytest.mark.parametrize("L16,H16", [(512, 160), (1000, 333)])
def test_hop_scores_16_chunk_builds(torch_cuda, L16, H16, which, dtype):
    """Frames past 448 samples (the transform reads the first 512): the
    per-hop comparisons above -- the FFN's scores against the float64 forward
    under test_ffn_hop_scores_accuracy's bound, the tree's against the clip
    kernel's bit for bit, both walks -- in the 16-chunk builds."""
    torch = torch_cuda
    if which == "ffn":
        sb = ffn_scores_accuracy(torch, "bl13", 5, 24, dtype, L=L16, H=H16)
        assert is_16_chunk(sb) and sb._hop_name == "vad_stream_hops_scores" + ("_i16" if dtype == "int16" else "")
    else:
        for walk in ("auto", "global"):
            check_tree_scores(torch, tree_with_scores(), 5, 1, 24, dtype, False, walk, L=L16, H=H16)
            sb = check_tree_scores.last
            assert is_16_chunk(sb) and sb.tree_walk == walk
            assert sb._hop_name == "vad_stream_hops_tree_scores" + ("_i16" if dtype == "int16" else "")


def test_tree_hop_scores_table_past_lds(torch_cuda):
    """A comb one node larger than vad_stream_tree_max_lds_nodes: the global
    walk, the score read at a node index far past the LDS table's size."""
    torch = torch_cuda
    from vad_amd import _lib
    S, T = 5, 16
    carry, hops = audio(S, T)
    probe = batch(torch, S, tree_with_scores(), carry)
    dh = cuda(hops)
    seq = []
    for t in range(T):
        probe.step(dh[t])
        seq.append(probe.ring[:, t % 5, :].clone())
    seq = torch.stack(seq, dim=1)
    X = np.concatenate([O.analyser_features_fast(seq[s].cpu().numpy()) for s in range(S)])
    n_max = _lib.lib().vad_stream_tree_max_lds_nodes(probe.plan.handle)
    table, depth = R.comb_table(n_max + 1, X, list(range(13, 26)))
    clf = with_counts(table)
    check_tree_scores(torch, clf, S, 1, T, "float32", False, "auto")


# ---------------------------------------------------------------------------
# end to end, and stale LDS
# ---------------------------------------------------------------------------
def test_end_to_end_one_graph(torch_cuda):
    torch = torch_cuda
    S, K, T, g, m, pad, on, off = 5, 8, 64, 2, 3, (2, 3), 0.6, 0.4
    carry, hops = audio(S, T, seed=1600)
    c16, h16 = carry.astype(np.int16), hops.astype(np.int16)
    sb = batch(torch, S, ffn("bl13"), c16, hops_per_step=K, input_dtype=torch.int16, scores=True)
    seg = sb.segmenter(on=on, off=off, pad=pad, max_gap=g, min_run=m)
    assert seg.audio_dtype == torch.int16 and seg.active == sb.active and seg.delay == g + m + (L // H - 1) + 1 + pad[0]
    seg.prime(cuda(c16))

    def body():
        sb._block_body()
        seg.push(sb.score_block, sb.inputs)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    saved = [t.clone() for t in (sb.frames, sb.ring, sb.count, seg.state, seg.found, seg.history, seg.table)]
    with torch.cuda.stream(side):
        body()  # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t, v in zip((sb.frames, sb.ring, sb.count, seg.state, seg.found, seg.history, seg.table), saved):
        t.copy_(v)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    scs, outs = [], []
    for t0 in range(0, T, K):
        sb.inputs.copy_(cuda(h16[t0:t0 + K]))
        graph.replay()
        scs.append(sb.score_block.cpu().numpy().copy())
        outs.append((seg.voiced.cpu().numpy().copy(), seg.voiced_len.cpu().numpy().copy()))
    fv, fn = seg.flush()
    outs.append((fv.cpu().numpy(), fn.cpu().numpy()))
    sc = np.concatenate(scs)
    assert np.isnan(sc[:5]).all() and not np.isnan(sc[5:]).any()
    clip = np.concatenate([c16, h16.transpose(1, 0, 2).reshape(S, -1)], axis=1)
    rows, found = seg.segments(), seg.found.cpu().numpy()
    for s in range(S):
        want, count, voiced = clip_chain_device(torch, sc[5:, s], clip[s], g, m, pad, on, off)
        assert found[s] == count and np.array_equal(rows[s], want), s
        assert np.array_equal(packed(outs, s, np.int16), voiced), s


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


@pytest.mark.parametrize("which", ["ffn", "tree_auto", "tree_global"])
def test_scored_hop_kernels_ignore_stale_lds(torch_cuda, poison, which):
    torch = torch_cuda
    S, T = 5, 16
    carry, hops = audio(S, T)
    dh = cuda(hops)
    clf = ffn("ref39") if which == "ffn" else tree_with_scores()
    kw = {} if which == "ffn" else dict(tree_walk=which[5:])

    def run(K, fill):
        sb = batch(torch, S, clf, carry, hops_per_step=K, scores=True, **kw)
        out = []
        for t0 in range(0, T, K):
            if fill is not None:
                poison(fill)
            if K == 1:
                sb.step(dh[t0])
            else:
                sb.step_block(dh[t0:t0 + K])
            out.append((sb.label_block.clone(), sb.score_block.view(torch.int32).clone()))
        return out + [(sb.frames.view(torch.int32).clone(), sb.ring.view(torch.int32).clone())]

    for K in (1, 8):
        want = run(K, None)
        for v in (1e30, -1e30, float("nan")):
            got = run(K, v)
            assert all(torch.equal(a, b) and torch.equal(c, d) for (a, c), (b, d) in zip(got, want)), (which, K, v)
