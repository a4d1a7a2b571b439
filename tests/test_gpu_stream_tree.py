"""The decision tree in the streaming path (stream_tree_kernel.hip,
StreamBatch with a TreeClassifier).

Three references, none of them the code under test:
  the FFN hop kernel, whose front end the tree hop kernel repeats: frames,
    ring and count of a tree batch and an FFN batch on the same hops are
    torch.equal after every block;
  the clip kernel (TreeClassifier.window_labels) on each stream's MFCC
    sequence as the hop kernel computed it (the newest ring row after every
    one-hop step): both run feature_triple, explicit-fma code, so the labels
    are equal exactly, for the LDS walk, the global walk and tables on either
    side of the LDS boundary (the clip kernel's labels are first checked
    against the oracle's walk of the device's own feature rows);
  the fp64 oracle, on every window whose path through the tree stays 1e-3
    (the project's analyser-feature tolerance) away from every threshold.
Every other test is an equivalence between two ways of running the same hops.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

from oracle import vad_oracle as O

import stream_tree_reference as R

pytestmark = pytest.mark.gpu

WALKS = ["auto", "global"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@functools.lru_cache(maxsize=None)
def _ffn():
    from vad_amd.ffn import FFNClassifier
    w = np.load(os.path.join(R.GOLDEN, "ffn.npz"), allow_pickle=False)
    return FFNClassifier([(w[f"ref39_W{i}"], w[f"ref39_b{i}"]) for i in range(4)])


@functools.lru_cache(maxsize=None)
def _tree():
    return R.classifier(R.fixture_tree())


@functools.lru_cache(maxsize=None)
def _audio(S, T, L=400, H=160, seed=1200):
    """carry (S, L-H) and hops (T, S, H) as float32 numpy, integer-valued."""
    keep = L - H
    clips = np.stack([O.synth_clip(H * T + keep, seed=seed + s)[:H * T + keep] for s in range(S)])
    carry = np.ascontiguousarray(clips[:, :keep])
    hops = np.ascontiguousarray(np.stack([clips[:, keep + H * t: keep + H * (t + 1)] for t in range(T)]))
    assert np.array_equal(hops, hops.astype(np.int16).astype(np.float32))
    return carry, hops


def _batch(torch, S, clf, carry, **kw):
    from vad_amd.stream import StreamBatch
    sb = StreamBatch(S, clf, **kw)
    sb.prime(torch.from_numpy(carry).cuda())
    return sb


def _block(sb, blk, K, graph):
    """One block (K, S, H) through sb; the labels (K, S), cloned."""
    if K == 1:
        return sb.step(blk[0]).clone()[None]
    if graph:
        sb.inputs.copy_(blk)
        return sb.step_block().clone()
    return sb.step_block(blk).clone()


def _run(sb, dh, K, graph=False):
    import torch
    if graph:
        sb.capture()
    return torch.cat([_block(sb, dh[b * K:(b + 1) * K], K, graph) for b in range(dh.shape[0] // K)])


def _same_state(a, b):
    import torch
    return torch.equal(a.frames, b.frames) and torch.equal(a.ring, b.ring) and torch.equal(a.count, b.count)


def _hops_for(K):
    return -(-16 // K) * K  # 16 hops, or the next multiple of K


@functools.lru_cache(maxsize=None)
def _serial(S, T, L=400, H=160):
    """One-hop fp32 steps of the fixture tree, LDS walk: labels (T, S), each
    stream's MFCC sequence (S, T, C) as the hop kernel computed it (step t
    writes ring slot t % 5), and the final state.  Computed once per shape,
    never written afterwards."""
    import torch
    from vad_amd.config import MfccConfig
    carry, hops = _audio(S, T, L, H)
    sb = _batch(torch, S, _tree(), carry, cfg=MfccConfig(frame_size=L, hop=H))
    dh = torch.from_numpy(hops).cuda()
    labels, seq = [], []
    for t in range(T):
        labels.append(sb.step(dh[t]).clone())
        seq.append(sb.ring[:, t % 5, :].clone())
    torch.cuda.synchronize()
    return torch.stack(labels), torch.stack(seq, dim=1).contiguous(), (sb.frames.clone(), sb.ring.clone(),
                                                                       sb.count.clone())


def _clip_labels(clf, seq):
    """The clip kernel on every stream's sequence: (T - 5, S) class indices."""
    import torch
    return torch.stack([clf.window_labels(seq[s]) for s in range(seq.shape[0])], dim=1)


# ---------------------------------------------------------------------------
# 1. the front end, locked to the FFN hop kernel
# ---------------------------------------------------------------------------
LOCK = [("hop", S, K) for S in (1, 5, 24) for K in (1, 2, 8)] + [("three", 5, 1), ("three", 5, 2)]


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("kernel,S,K", LOCK)
def test_front_end_locked_to_ffn_kernel(torch_cuda, kernel, S, K, dtype, graph):
    torch = torch_cuda
    dt = getattr(torch, dtype)
    T = _hops_for(K)
    carry, hops = _audio(S, T)
    dh = torch.from_numpy(hops).cuda().to(dt)
    kw = dict(kernel=kernel, hops_per_step=K, input_dtype=dt)
    tree, ffn = _batch(torch, S, _tree(), carry, **kw), _batch(torch, S, _ffn(), carry, **kw)
    assert tree.is_tree and tree.classifier is tree.ffn and not ffn.is_tree
    if graph:
        tree.capture(), ffn.capture()
        if kernel == "hop" and K == 1:
            assert tree.graph_direct  # still a single kernel node
    for b in range(T // K):
        blk = dh[b * K:(b + 1) * K]
        lt, lf = _block(tree, blk, K, graph), _block(ffn, blk, K, graph)
        assert torch.equal(tree.frames, ffn.frames), b
        assert torch.equal(tree.ring, ffn.ring), b
        assert torch.equal(tree.count, ffn.count), b
        assert torch.equal(lt == 255, lf == 255), b
    assert (tree.count > 5).all() and tree.ring.abs().sum().item() > 0


# ---------------------------------------------------------------------------
# 2. the walk, bit for bit against the clip kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("S", [1, 5, 24])
def test_walk_equals_clip_kernel(torch_cuda, S, walk):
    torch = torch_cuda
    T = 16
    carry, hops = _audio(S, T)
    want_lab, seq, state = _serial(S, T)
    sb = _batch(torch, S, _tree(), carry, tree_walk=walk)
    got = _run(sb, torch.from_numpy(hops).cuda(), 1)
    assert (got[:5] == 255).all() and (got[5:] != 255).all()
    clip = _clip_labels(_tree(), seq)
    assert clip.shape == got[5:].shape
    _assert_clip_equals_host_walk(R.fixture_tree(), clip, seq)
    assert torch.equal(got[5:], clip), int((got[5:] != clip).sum())
    assert torch.equal(got, want_lab)  # auto == global
    assert all(torch.equal(x, y) for x, y in zip((sb.frames, sb.ring, sb.count), state))
    if S == 24:
        assert len(torch.unique(clip)) == 2  # both classes reached


def _assert_clip_equals_host_walk(table, clip, seq):
    """The clip kernel's labels (T - 5, S) against the oracle's walk of the
    device's own feature rows, every stream: checked before they judge the
    hop kernel."""
    from vad_amd.plan import window_features
    clip = clip.cpu().numpy().astype(np.int64)
    for s in range(seq.shape[0]):
        want = O.tree_predict(table, window_features(seq[s].contiguous()).cpu().numpy())
        assert np.array_equal(table["classes"][clip[:, s]], want), s


def _features_of(seq):
    """fp64 analyser features of the recorded sequences, all streams' windows
    as rows (comb thresholds are midpoints between them: their last bits do
    not matter)."""
    return np.concatenate([O.analyser_features_fast(seq[s].cpu().numpy()) for s in range(seq.shape[0])])


@pytest.mark.parametrize("extra", [0, 1], ids=["max_lds_nodes", "max_lds_nodes+1"])
def test_walk_at_the_lds_boundary(torch_cuda, extra):
    """A comb of exactly vad_stream_tree_max_lds_nodes nodes (blob + nodes +
    one wave's scratch = 160 KiB or just under: the LDS walk, one wave per
    block) and one of one node more (no launch could hold it in LDS: the
    kernel refuses more than 160 KiB, so a run that succeeds under "auto"
    walked from global memory).  Rows leave the spine all along it, the
    deepest after thousands of levels; labels equal the clip kernel's and
    each other under "auto" and "global"."""
    torch = torch_cuda
    from vad_amd import _lib
    S, T = 5, 16
    carry, hops = _audio(S, T)
    _, seq, state = _serial(S, T)
    X = _features_of(seq)
    probe = _batch(torch, S, _tree(), carry)
    n_max = _lib.lib().vad_stream_tree_max_lds_nodes(probe.plan.handle)
    assert n_max > 3072  # past the clip kernel's own LDS limit too
    table, depth = R.comb_table(n_max + extra, X, list(range(13, 26)))
    assert len(table["feature"]) == n_max + extra
    assert depth.max() > n_max // 4 and len(set(depth.tolist())) > len(X) // 4  # deep, and both directions taken
    clf = R.classifier(table)
    clip = _clip_labels(clf, seq)
    _assert_clip_equals_host_walk(table, clip, seq)
    assert len(torch.unique(clip)) == 2  # leaves alternate class along the spine
    dh = torch.from_numpy(hops).cuda()
    out = {}
    for walk in WALKS:
        for K in (1, 8):
            sb = _batch(torch, S, clf, carry, tree_walk=walk, hops_per_step=K)
            out[walk, K] = _run(sb, dh, K)
            assert all(torch.equal(x, y) for x, y in zip((sb.frames, sb.ring, sb.count), state))
    for got in out.values():
        assert (got[:5] == 255).all()
        assert torch.equal(got[5:], clip), int((got[5:] != clip).sum())


# ---------------------------------------------------------------------------
# 3. equivalences
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("K", [1, 2, 8])
@pytest.mark.parametrize("S", [1, 5, 24])
def test_blocks_dtypes_and_graphs_equal_serial_steps(torch_cuda, S, K, dtype, graph):
    """K-hop launches, int16 input and graph replays against the one-hop fp32
    direct steps: labels and state identical."""
    torch = torch_cuda
    dt = getattr(torch, dtype)
    T = _hops_for(K)
    carry, hops = _audio(S, T)
    want, _, state = _serial(S, T)
    sb = _batch(torch, S, _tree(), carry, hops_per_step=K, input_dtype=dt)
    got = _run(sb, torch.from_numpy(hops).cuda().to(dt), K, graph)
    assert torch.equal(got, want), int((got != want).sum())
    assert all(torch.equal(x, y) for x, y in zip((sb.frames, sb.ring, sb.count), state))


@pytest.mark.parametrize("walk", WALKS)
def test_stream_major_layout(torch_cuda, walk):
    """An (S, K * hop) buffer viewed as (K, S, hop), read in place."""
    torch = torch_cuda
    from vad_amd.stream import hop_rows_disjoint
    S, K, T = 5, 8, 16
    carry, hops = _audio(S, T)
    want, _, state = _serial(S, T)
    per_stream = torch.from_numpy(np.ascontiguousarray(hops.transpose(1, 0, 2).reshape(S, T * 160))).cuda()
    sb = _batch(torch, S, _tree(), carry, hops_per_step=K, tree_walk=walk)
    got = []
    for b in range(T // K):
        blk = per_stream[:, 160 * K * b:160 * K * (b + 1)].contiguous().view(S, K, 160).transpose(0, 1)
        assert blk.stride() == (160, K * 160, 1) and hop_rows_disjoint(S, K, 160, K * 160, 160)
        got.append(sb.step_block(blk).clone())
    assert torch.equal(torch.cat(got), want)
    assert all(torch.equal(x, y) for x, y in zip((sb.frames, sb.ring, sb.count), state))


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_step_host(torch_cuda, graph):
    torch = torch_cuda
    S, K, T = 5, 8, 16
    carry, hops = _audio(S, T)
    want = _serial(S, T)[0].cpu()
    sb = _batch(torch, S, _tree(), carry, hops_per_step=K, input_dtype=torch.int16)
    if graph:
        sb.capture(host_io=True)
    else:
        sb.attach_host_io()
    h16 = torch.from_numpy(hops.astype(np.int16))
    got = []
    for b in range(T // K):
        sb.host_inputs.copy_(h16[b * K:(b + 1) * K])
        lab = sb.step_host()
        torch.cuda.current_stream().synchronize()
        got.append(lab.clone())
    assert torch.equal(torch.cat(got), want)


@pytest.mark.parametrize("kernel,K", [("hop", 2), ("three", 1)])
def test_host_pipeline_equals_serial_step_host(torch_cuda, kernel, K):
    torch = torch_cuda
    S, nb, depth = 5, 8, 2
    T = K * nb
    carry, hops = _audio(S, 16)
    hops_host = torch.from_numpy(hops[:T])
    ser = _batch(torch, S, _tree(), carry, kernel=kernel, hops_per_step=K)
    ser.attach_host_io()
    want = []
    for b in range(nb):
        ser.host_inputs.copy_(hops_host[b * K:(b + 1) * K])
        lab = ser.step_host()
        torch.cuda.current_stream().synchronize()
        want.append(lab.clone())
    sb = _batch(torch, S, _tree(), carry, kernel=kernel, hops_per_step=K)
    pipe = sb.host_pipeline(depth)

    def put(b):
        pipe.host_inputs[b % depth].copy_(hops_host[b * K:(b + 1) * K])
        pipe.submit(b % depth)

    put(0)
    got = []
    for b in range(nb):
        if b + 1 < nb:
            put(b + 1)
        got.append(pipe.wait(b % depth).clone())
        pipe.host_inputs[b % depth].view(torch.uint8).fill_(0x7f)  # a late copy-in would read these
    pipe.drain()
    assert torch.equal(torch.cat(got), torch.cat(want))
    assert _same_state(sb, ser)
    if kernel == "hop":
        assert torch.equal(torch.cat(got), _serial(S, 16)[0].cpu())


def test_odd_geometry_equals_three_kernel_form(torch_cuda):
    """frame_size 1000, hop 333: the 16-chunk build of the hop kernel against
    the three-kernel form (the clip MFCC kernel, then stream_tree_ring_kernel)
    on the same input -- labels, frames and count equal; the two MFCC kernels
    agree to the project's 1e-4 (as the FFN forms do), so the rings are
    compared with that."""
    torch = torch_cuda
    from vad_amd.config import MfccConfig
    S, K, T, L, H = 5, 4, 16, 1000, 333
    cfg = MfccConfig(frame_size=L, hop=H)
    carry, hops = _audio(S, T, L, H, seed=1300)
    dh = torch.from_numpy(hops).cuda()
    three = _batch(torch, S, _tree(), carry, cfg=cfg, kernel="three")
    one = _batch(torch, S, _tree(), carry, cfg=cfg)
    blk = _batch(torch, S, _tree(), carry, cfg=cfg, hops_per_step=K)
    glob = _batch(torch, S, _tree(), carry, cfg=cfg, hops_per_step=K, tree_walk="global", input_dtype=torch.int16)
    lab3, lab1 = _run(three, dh, 1), _run(one, dh, 1)
    assert torch.equal(_run(blk, dh, K), lab1) and _same_state(blk, one)
    assert torch.equal(_run(glob, dh.to(torch.int16), K), lab1) and _same_state(glob, one)
    a, b = one.ring.double().cpu().numpy(), three.ring.double().cpu().numpy()
    rel = np.linalg.norm(a - b, axis=2) / np.maximum(np.linalg.norm(b, axis=2), 1e-30)
    print("hop vs three ring, max relative row error", rel.max())
    assert rel.max() <= 1e-4
    assert torch.equal(one.frames, three.frames) and torch.equal(one.count, three.count)
    print("labels differing, hop vs three:", int((lab1 != lab3).sum()), "of", lab1.numel())
    assert torch.equal(lab1, lab3)
    assert (lab1[:5] == 255).all() and (lab1[5:] <= 1).all()


def test_three_kernel_form_equals_clip_kernel(torch_cuda):
    """stream_tree_ring_kernel against the clip kernel on the sequences it was
    given (the scratch row of every step), 70 streams: more than one block."""
    torch = torch_cuda
    S, T = 70, 12
    carry, hops = _audio(S, T, seed=1500)
    sb = _batch(torch, S, _tree(), carry, kernel="three")
    dh = torch.from_numpy(hops).cuda()
    labels, seq = [], []
    for t in range(T):
        labels.append(sb.step(dh[t]).clone())
        seq.append(sb.scratch.clone())
        assert torch.equal(sb.ring[:, t % 5, :], sb.scratch)
    got = torch.stack(labels)
    assert (got[:5] == 255).all()
    assert torch.equal(got[5:], _clip_labels(_tree(), torch.stack(seq, dim=1).contiguous()))


# ---------------------------------------------------------------------------
# 4. against the fp64 oracle
# ---------------------------------------------------------------------------
def test_against_oracle(torch_cuda):
    """Labels equal the oracle's on every window whose path keeps 1e-3 from
    every threshold it meets; the oracle alone excludes 1 of the 280 windows
    (test_stream_tree_cpu.py), at most 5 % may be."""
    torch = torch_cuda
    tree = R.fixture_tree()
    S, T = 8, 40
    clips = [O.synth_clip(160 * (T - 1) + 401, seed=700 + s) for s in range(S)]
    fb = O.get_mel_filterbanks(300, 8000, 512, 26, 16000)
    sb = _batch(torch, S, _tree(), np.stack([c[:240] for c in clips]))
    got, seq = [], []
    for t in range(T):
        new = np.stack([c[240 + 160 * t: 400 + 160 * t] for c in clips])
        got.append(sb.step(torch.from_numpy(new).cuda()).cpu().numpy().copy())
        seq.append(sb.ring[:, t % 5, :].cpu().numpy().copy())
    got = np.stack(got, axis=1)  # (S, T)
    seq = np.stack(seq, axis=1)  # (S, T, 13)
    assert (got[:, :5] == 255).all()
    got = tree["classes"][got[:, 5:].astype(np.int64)]
    n_ok, counts, bad = 0, np.zeros(2, np.int64), []
    for s, c in enumerate(clips):
        x = O.analyser_features_fast(O.mfcc_batch(c, fb))
        margin, _ = R.path_margin(tree, x)
        want = O.tree_predict(tree, x)
        ok = margin > 1e-3
        n_ok += int(ok.sum())
        counts += np.array([(want == k).sum() for k in tree["classes"]])
        for w in np.nonzero(ok & (got[s] != want))[0]:
            dev = O.analyser_features_fast(seq[s])[w]
            with np.errstate(invalid="ignore"):
                err = np.nanmax(np.abs(dev - x[w]) / np.maximum(1.0, np.abs(x[w])))
            print(f"stream {s} window {w}: device {got[s, w]} oracle {want[w]} margin {margin[w]:.3e} "
                  f"feature error {err:.3e}")
            bad.append((s, int(w)))
    print("windows compared", n_ok, "of", got.size, "oracle labels", counts.tolist())
    assert not bad, bad
    assert n_ok >= 0.95 * got.size
    assert sorted(counts.tolist()) == [133, 147]


# ---------------------------------------------------------------------------
# 5. NaN features and the warm-up
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("nan_left", [1, 0])
def test_nan_follows_the_flag_and_warm_up(torch_cuda, nan_left, walk):
    """Stream 0 is digital silence: every window is constant, every Mn NaN.
    Stream 1 is silence for 7 hops, then noise; stream 2 noise.  The root
    splits on Mn of coefficient 0: left is class 1, right class 0."""
    torch = torch_cuda
    from vad_amd.tree import TreeClassifier
    S, T = 3, 16
    clf = TreeClassifier([0, -1, -1], [0.0, 0.0, 0.0], [1, -1, -1], [2, -1, -1], [0, 1, 0], [nan_left, 0, 0], [0, 1], 39)
    rng = np.random.default_rng(3)
    hops = np.rint(rng.standard_normal((T, S, 160)) * 3000).astype(np.float32)
    hops[:, 0] = 0
    hops[:7, 1] = 0
    dh = torch.from_numpy(hops).cuda()
    sb = _batch(torch, S, clf, np.zeros((S, 240), np.float32), tree_walk=walk)
    for rep in range(2):
        labels, seq = [], []
        for t in range(T):
            labels.append(sb.step(dh[t]).clone())
            seq.append(sb.ring[:, t % 5, :].clone())
        got = torch.stack(labels)
        assert (got[:5] == 255).all(), rep  # the first five hops of every stream, after reset() too
        assert (got[5:, 0] == nan_left).all(), got[5:, 0].tolist()
        assert (got[5:8, 1] == nan_left).all()  # windows of hops 0..6: silence only
        clip = _clip_labels(clf, torch.stack(seq, dim=1).contiguous())
        assert torch.equal(got[5:], clip)
        assert len(torch.unique(got[5:, 2])) == 2  # the finite rule takes both sides
        sb.reset()
        assert (sb.label_block == 255).all()


# ---------------------------------------------------------------------------
# 6. stale LDS
# ---------------------------------------------------------------------------
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


@pytest.mark.parametrize("walk", WALKS)
def test_tree_hop_kernel_ignores_stale_lds(torch_cuda, poison, walk):
    """K = 8, every launch preceded by a kernel that filled every CU's LDS
    with a hostile value: labels and state identical to a clean run."""
    torch = torch_cuda
    S, K, T = 300, 8, 16
    carry, hops = _audio(S, T, seed=1400)
    dh = torch.from_numpy(hops.astype(np.int16)).cuda()
    outs = []
    for v in (None, 1e30, -1e30, float("nan")):
        sb = _batch(torch, S, _tree(), carry, hops_per_step=K, input_dtype=torch.int16, tree_walk=walk)
        labs = []
        for t in range(0, T, K):
            if v is not None:
                poison(v)
            labs.append(sb.step_block(dh[t:t + K]).clone())
        outs.append([torch.cat(labs).cpu(), sb.frames.view(torch.int32).cpu(), sb.ring.view(torch.int32).cpu(),
                     sb.count.cpu()])
    for o in outs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(o, outs[0]))
    assert len(torch.unique(outs[0][0][5:])) == 2


# ---------------------------------------------------------------------------
# 7. segments
# ---------------------------------------------------------------------------
def test_segmenter_on_tree_labels(torch_cuda):
    """sb.segmenter fed the tree batch's label_block and inputs, flushed:
    label_segments / voiced_audio on the same labels and each stream's
    equivalent clip (one zero appended: the clip entries count frames with a
    strict >, test_gpu_stream_segments.py)."""
    torch = torch_cuda
    from vad_amd import segments as SG
    S, K, T, L, H, g, m = 5, 8, 48, 400, 160, 2, 2
    carry, hops = _audio(S, T, seed=1600)
    sb = _batch(torch, S, _tree(), carry.astype(np.int16), hops_per_step=K, input_dtype=torch.int16)
    seg = sb.segmenter(max_gap=g, min_run=m)
    seg.prime(torch.from_numpy(carry.astype(np.int16)).cuda())
    h16 = torch.from_numpy(hops.astype(np.int16))
    labs, outs = [], []
    for t0 in range(0, T, K):
        sb.inputs.copy_(h16[t0:t0 + K])
        lab = sb.step_block()
        v, n = seg.push(lab, sb.inputs)
        labs.append(lab.cpu().numpy().copy())
        outs.append((v.cpu().numpy().copy(), n.cpu().numpy().copy()))
    fv, fn = seg.flush()
    outs.append((fv.cpu().numpy(), fn.cpu().numpy()))
    labs = np.concatenate(labs)
    assert (labs[:5] == 255).all() and (labs[5:] <= 1).all()
    rows, found = seg.segments(), seg.found.cpu().numpy()
    clip = np.concatenate([carry, hops.transpose(1, 0, 2).reshape(S, -1)], axis=1).astype(np.int16)
    total_rows = 0
    for s in range(S):
        padded = np.concatenate([clip[s], np.zeros(1, np.int16)])
        d_lab = torch.from_numpy(np.ascontiguousarray(labs[5:, s])).cuda()
        off = SG.label_segments(d_lab, len(padded), L, H, g, m, active=seg.active)
        want = off.numpy()
        assert found[s] == int(off.counts[0].item()), s
        assert np.array_equal(rows[s], want), s
        out, counts = SG.voiced_audio(torch.from_numpy(padded).cuda(), off)
        total = int(counts[1].item())
        parts = [v[k, s, :n[k, s]] for v, n in outs for k in range(n.shape[0])]
        got = np.concatenate(parts).astype(np.int16) if parts else np.zeros(0, np.int16)
        assert len(got) == total, s
        assert np.array_equal(got, out[:total].cpu().numpy()), s
        total_rows += len(want)
    assert total_rows > 0
