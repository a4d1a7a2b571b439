"""A random forest in the hop kernel (stream_forest_kernel.hip,
ForestStreamBatch).  Every comparison is bit for bit; none of the references
is the code under test:
  the FFN hop kernel for the front end (frames, ring, count);
  the clip forest kernel (ForestClassifier.window_labels / window_scores, itself
    held to sklearn's predict_proba by test_gpu_forest.py) on each stream's
    MFCC sequence as the hop kernel computed it (the newest ring row after
    every one-hop step) for labels and scores;
  the tree hop kernel (StreamBatch with a TreeClassifier) for a one-tree forest;
  the clip chain score_labels -> smooth_labels -> dilate_labels ->
    label_segments for the segmenter.
The rest are equivalences between two ways of running the same hops.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import forest_reference as FR
from oracle import vad_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
L, H = 400, 160


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@functools.lru_cache(maxsize=None)
def _audio(S, T, L=L, H=H, seed=1200):
    """carry (S, L-H) and hops (T, S, H) as float32 numpy, integer-valued."""
    keep = L - H
    clips = np.stack([O.synth_clip(H * T + keep, seed=seed + s)[:H * T + keep] for s in range(S)])
    clips = clips + np.float32(0.0)  # no -0.0 samples: int16 has none, and the state is compared by its bits
    carry = np.ascontiguousarray(clips[:, :keep])
    hops = np.ascontiguousarray(np.stack([clips[:, keep + H * t: keep + H * (t + 1)] for t in range(T)]))
    assert np.array_equal(hops, hops.astype(np.int16).astype(np.float32))
    return carry, hops


@functools.lru_cache(maxsize=None)
def _ffn():
    from vad_amd.ffn import FFNClassifier
    w = np.load(os.path.join(GOLDEN, "ffn.npz"), allow_pickle=False)
    return FFNClassifier([(w[f"ref39_W{i}"], w[f"ref39_b{i}"]) for i in range(4)])


def as_tree(t, F=39, K=2):
    from vad_amd.tree import TreeClassifier
    return TreeClassifier(t["feature"], t["threshold"], t["left"], t["right"], t["leaf"], t["nan_left"], np.arange(K),
                          F, proba=t["proba"])


@functools.lru_cache(maxsize=None)
def random_forest(sizes, K=2, seed=0, F=39):
    from vad_amd.forest import ForestClassifier
    return ForestClassifier.from_trees([as_tree(FR.random_tree(n, F, K, seed + i), F, K) for i, n in enumerate(sizes)])


@functools.lru_cache(maxsize=None)
def golden_forest(name):
    from vad_amd.forest import ForestClassifier
    g = np.load(os.path.join(GOLDEN, "forest.npz"), allow_pickle=False)
    return ForestClassifier(*(g[f"{name}_{k}"] for k in FR.KEYS), g[f"{name}_classes"], 39)


def sizes_between(lo, hi, T, seed):
    """T odd tree sizes in [lo, hi]."""
    return tuple(int(n) | 1 for n in np.random.default_rng(seed).integers(lo, hi, T))


def fbatch(S, forest, carry, **kw):
    from vad_amd.stream import ForestStreamBatch
    sb = ForestStreamBatch(S, forest, **kw)
    sb.prime(cuda(carry))
    return sb


def bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def state(sb):
    return [sb.frames.clone(), sb.ring.clone(), sb.count.clone()]


def same(a, b):
    import torch
    return all(torch.equal(bits(x) if x.dtype == torch.float32 else x, bits(y) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def run(sb, dh, K, graph=False):
    """The hops (T, S, H) through sb in blocks of K: labels and score bits (T, S), cloned."""
    import torch
    if graph:
        sb.capture()
    labs, scs = [], []
    for b in range(dh.shape[0] // K):
        blk = dh[b * K:(b + 1) * K]
        if K == 1:
            sb.step(blk[0])
        elif graph:
            sb.inputs.copy_(blk)
            sb.step_block()
        else:
            sb.step_block(blk)
        labs.append(sb.label_block.clone())
        if sb.scores:
            scs.append(bits(sb.score_block).clone())
    return torch.cat(labs), (torch.cat(scs) if scs else None)


def serial(S, T, forest, active=1, cfg=None, **kw):
    """One-hop direct steps: labels, score bits (T, S), the MFCC sequences (S, T, C)
    the hop kernel computed (step t writes ring slot t % 5), and the final state."""
    import torch
    from vad_amd.config import MfccConfig
    cfg = cfg or MfccConfig()
    carry, hops = _audio(S, T, cfg.frame_size, cfg.hop)
    sb = fbatch(S, forest, carry, cfg=cfg, scores=True, active=active, **kw)
    dh = cuda(hops)
    labs, scs, seq = [], [], []
    for t in range(T):
        sb.step(dh[t])
        labs.append(sb.label_block[0].clone())
        scs.append(bits(sb.score_block[0]).clone())
        seq.append(sb.ring[:, t % 5, :].clone())
    return torch.stack(labs), torch.stack(scs), torch.stack(seq, dim=1).contiguous(), state(sb), sb


def clip_reference(forest, seq, active):
    """The clip forest kernel on every stream's sequence: labels and score bits (T - 5, S)."""
    import torch
    lab = torch.stack([forest.window_labels(seq[s]) for s in range(seq.shape[0])], dim=1)
    sc = torch.stack([bits(forest.window_scores(seq[s], active=active)) for s in range(seq.shape[0])], dim=1)
    return lab, sc


def assert_equals_clip(forest, labs, scs, seq, active):
    import torch
    nan = torch.tensor(float("nan")).view(torch.int32).item()
    assert (labs[:5] == 255).all() and (scs[:5] == nan).all()
    lab, sc = clip_reference(forest, seq, active)
    assert lab.shape == labs[5:].shape
    assert torch.equal(labs[5:], lab), int((labs[5:] != lab).sum())
    assert torch.equal(scs[5:], sc), int((scs[5:] != sc).sum())
    return lab


# ---------------------------------------------------------------------------
# 1. the front end, locked to the FFN hop kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("S,K,L1", [(1, 1, 400), (5, 2, 400), (24, 8, 400), (5, 1, 1024), (5, 8, 1024)])
def test_front_end_locked_to_ffn_kernel(torch_cuda, S, K, L1, dtype, graph):
    torch = torch_cuda
    from vad_amd.config import MfccConfig
    from vad_amd.stream import StreamBatch
    dt = getattr(torch, dtype)
    T = 16
    cfg = MfccConfig(frame_size=L1, hop=H)
    carry, hops = _audio(S, T, L1, H)
    dh = cuda(hops).to(dt)
    kw = dict(cfg=cfg, hops_per_step=K, input_dtype=dt)
    fo = fbatch(S, random_forest((31, 7, 15), seed=3), carry, **kw)
    ffn = StreamBatch(S, _ffn(), **kw)
    ffn.prime(cuda(carry))
    assert fo.is_forest and not fo.is_tree and fo.classifier is fo.ffn
    if graph:
        fo.capture(), ffn.capture()
        if K == 1:
            assert fo.graph_direct  # still a single kernel node
    for b in range(T // K):
        for sb in (fo, ffn):
            if K == 1:
                sb.step(dh[b])
            else:
                sb.inputs.copy_(dh[b * K:(b + 1) * K])
                sb.step_block()
        assert torch.equal(fo.frames, ffn.frames), b
        assert torch.equal(fo.ring, ffn.ring), b
        assert torch.equal(fo.count, ffn.count), b
        assert torch.equal(fo.label_block == 255, ffn.label_block == 255), b
    assert (fo.count > 5).all() and fo.ring.abs().sum().item() > 0


# ---------------------------------------------------------------------------
# 2. labels and scores, bit for bit against the clip forest kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 5, 24])
@pytest.mark.parametrize("name", ["rf", "bag", "rf3"])
def test_golden_forests_equal_clip_kernel(torch_cuda, name, S):
    forest = golden_forest(name)
    for active in range(len(forest.classes_)):
        labs, scs, seq, _, _ = serial(S, 16, forest, active)
        assert_equals_clip(forest, labs, scs, seq, active)


@pytest.mark.parametrize("T_", [1, 2, 3, 63, 64, 65, 130])
def test_tree_counts_at_the_lane_pass_boundary(torch_cuda, T_):
    forest = random_forest(sizes_between(3, 31, T_, seed=T_), seed=100 + T_)
    assert forest.n_trees == T_
    labs, scs, seq, _, sb = serial(5, 16, forest, 1)
    assert sb.lds_trees == T_
    lab = assert_equals_clip(forest, labs, scs, seq, 1)
    if T_ >= 3:
        assert len(torch_cuda.unique(lab)) == 2


@pytest.mark.parametrize("sizes,K", [((31, 1, 201, 7), 2), ((1,), 2), ((1, 1, 1), 3), ((41, 9, 77, 3, 51), 8),
                                     ((15, 3, 9, 27, 1, 5, 31, 11, 7), 8)])
def test_unequal_trees_and_classes(torch_cuda, sizes, K):
    forest = random_forest(sizes, K, seed=21)
    for active in range(K):
        labs, scs, seq, _, _ = serial(5, 16, forest, active)
        assert_equals_clip(forest, labs, scs, seq, active)


# ---------------------------------------------------------------------------
# 3. a forest of one tree is the tree batch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "denoise", "sessions"])
def test_one_tree_forest_equals_tree_batch(torch_cuda, form):
    torch = torch_cuda
    from vad_amd.forest import ForestClassifier
    from vad_amd.stream import StreamBatch
    S, K, T = 5, 4, 16
    tree = as_tree(FR.random_tree(61, 39, 2, seed=8))
    forest = ForestClassifier.from_trees([tree])
    kw = dict(hops_per_step=K, scores=True, active=1, denoise=form == "denoise", sessions=form == "sessions")
    carry, hops = _audio(S, T)
    a = fbatch(S, forest, carry, **kw)
    b = StreamBatch(S, tree, **kw)
    b.prime(cuda(carry))
    dh = cuda(hops)
    cnt = torch.tensor([K, 0, 2, K, 1], dtype=torch.int32, device="cuda")
    for i in range(T // K):
        sess = {}
        if form == "sessions":
            rst = torch.zeros(S, dtype=torch.uint8, device="cuda")
            rst[3] = i == 2
            sess = dict(hop_counts=cnt, restart=rst)
        for sb in (a, b):
            sb.step_block(dh[i * K:(i + 1) * K], **sess)
        assert torch.equal(a.label_block, b.label_block), i
        assert torch.equal(bits(a.score_block), bits(b.score_block)), i
        assert same(state(a), state(b)), i
        if form == "denoise":
            assert same([a._spec, a._noise, a._est, a.noise_count], [b._spec, b._noise, b._est, b.noise_count]), i
    assert len(torch.unique(a.label_block)) >= 2


# ---------------------------------------------------------------------------
# 4. the staging boundary
# ---------------------------------------------------------------------------
def sizes_summing(total, tail=True):
    """Odd tree sizes (31, 63[, 1], big) summing to total, the big tree last (or first)."""
    rest = [31, 63]
    big = total - sum(rest)
    if big % 2 == 0:
        rest.append(1)
        big -= 1
    return tuple(rest + [big]) if tail else tuple([big] + rest)


def test_staging_boundary(torch_cuda):
    torch = torch_cuda
    from vad_amd import _lib
    from vad_amd.plan import MfccPlan
    from vad_amd.config import MfccConfig
    lib = _lib.lib()
    plan = MfccPlan.from_config(MfccConfig())
    n_max = lib.vad_stream_tree_max_lds_nodes(plan.handle)  # the nodes that fit beside the blob and one wave's scratch
    assert n_max > 3072
    S, T = 5, 16
    first_big = n_max + 1 + (n_max % 2)  # odd, past the room
    cases = [(sizes_summing(n_max), lambda n: n), (sizes_summing(n_max + 1), lambda n: n - 1),
             ((first_big, 31, 63), lambda n: 0)]
    carry, hops = _audio(S, T)
    dh = cuda(hops)
    for sizes, want_trees in cases:
        forest = random_forest(sizes, seed=40)
        n = forest.n_trees
        assert lib.vad_stream_forest_lds_trees(plan.handle, forest.plan.handle) == want_trees(n), sizes
        labs, scs, seq, st, sb = serial(S, T, forest, 1)
        assert sb.lds_trees == want_trees(n)
        assert_equals_clip(forest, labs, scs, seq, 1)
        for walk, K in (("global", 1), ("global", 8), ("auto", 8)):
            other = fbatch(S, forest, carry, tree_walk=walk, hops_per_step=K, scores=True, active=1)
            assert other.lds_trees == (0 if walk == "global" else want_trees(n))
            lo, so = run(other, dh, K)
            assert torch.equal(lo, labs) and torch.equal(so, scs), (sizes, walk, K)
            assert same(state(other), st)
    assert lib.vad_stream_hop_forest_table_bytes(plan.handle, forest.plan.handle, 1) == \
        lib.vad_stream_hop_forest_table_bytes(plan.handle, forest.plan.handle, 0)  # nothing staged either way
    whole = random_forest(sizes_summing(n_max), seed=40)
    assert lib.vad_stream_hop_forest_table_bytes(plan.handle, whole.plan.handle, 0) == \
        lib.vad_stream_hop_forest_table_bytes(plan.handle, whole.plan.handle, 1) + 16 * n_max


# ---------------------------------------------------------------------------
# 5. ties and NaN features
# ---------------------------------------------------------------------------
def leaf_tree(share, F=39):
    from vad_amd.tree import TreeClassifier
    return TreeClassifier([-1], [-2.0], [-1], [-1], [int(np.argmax(share))], [0], np.arange(len(share)), F,
                          proba=np.array([share], np.float64))


def test_an_exact_tie_gives_the_first_class(torch_cuda):
    from vad_amd.forest import ForestClassifier
    S, T = 3, 8
    carry, hops = _audio(S, T)
    for shares in ([[1.0, 0.0], [0.0, 1.0]], [[0.0, 1.0], [1.0, 0.0]]):
        forest = ForestClassifier.from_trees([leaf_tree(s) for s in shares])
        sb = fbatch(S, forest, carry, scores=True, active=1)
        labs, scs = run(sb, cuda(hops), 1)
        assert (labs[:5] == 255).all() and labs[5:].cpu().numpy().tolist() == [[0] * S] * (T - 5)
        assert scs[5:].view(torch_cuda.float32).cpu().numpy().tolist() == [[0.5] * S] * (T - 5)


@pytest.mark.parametrize("walk", ["auto", "global"])
@pytest.mark.parametrize("nan_left", [0, 1])
def test_a_constant_window_follows_nan_left(torch_cuda, nan_left, walk):
    """Stream 0 is fed all-zero hops: every window is constant, every Mn NaN."""
    from vad_amd.forest import ForestClassifier
    from vad_amd.tree import TreeClassifier
    stump = TreeClassifier([0, -1, -1], [1e30, -2.0, -2.0], [1, -1, -1], [2, -1, -1], [0, 0, 1], [nan_left, 0, 0],
                           np.arange(2), 39, proba=np.array([[.5, .5], [1., 0.], [0., 1.]]))
    forest = ForestClassifier.from_trees([stump, stump, stump])
    S, T = 2, 12
    rng = np.random.default_rng(3)
    hops = np.rint(rng.standard_normal((T, S, H)) * 3000).astype(np.float32)
    hops[:, 0] = 0
    sb = fbatch(S, forest, np.zeros((S, L - H), np.float32), tree_walk=walk, scores=True, active=1)
    labs, scs = run(sb, cuda(hops), 1)
    got = labs[5:].cpu().numpy()
    assert (got[:, 0] == (0 if nan_left else 1)).all(), got[:, 0]
    assert (got[:, 1] == 0).all()  # every finite Mn is <= 1e30: left, class 0
    assert (scs[5:, 0].view(torch_cuda.float32) == (0.0 if nan_left else 1.0)).all()


# ---------------------------------------------------------------------------
# 6. equivalences
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed_forest():
    return random_forest(sizes_between(3, 61, 20, seed=6), seed=60)


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("S,K", [(1, 2), (5, 8), (24, 4), (24, 1)])
def test_blocks_dtypes_and_graphs_equal_serial_steps(torch_cuda, S, K, dtype, graph):
    torch = torch_cuda
    dt = getattr(torch, dtype)
    T = 16
    forest = _mixed_forest()
    labs, scs, _, st, _ = serial(S, T, forest, 0)
    carry, hops = _audio(S, T)
    sb = fbatch(S, forest, carry, hops_per_step=K, input_dtype=dt, scores=True, active=0)
    lo, so = run(sb, cuda(hops).to(dt), K, graph)
    assert torch.equal(lo, labs) and torch.equal(so, scs)
    assert same(state(sb), st)
    plain = fbatch(S, forest, carry, hops_per_step=K, input_dtype=dt)  # labels alone: a null `scores`
    assert plain.score_block is None
    assert torch.equal(run(plain, cuda(hops).to(dt), K)[0], labs) and same(state(plain), st)


def test_every_block_shape(torch_cuda):
    """block_waves 4 (one hop), 1 (K hops), and 2 and 1 at one hop with tables
    that leave room for two waves' scratch, or one's."""
    torch = torch_cuda
    from vad_amd import _lib
    S, T = 24, 16
    carry, hops = _audio(S, T)
    dh = cuda(hops)
    small = _mixed_forest()
    probe = fbatch(S, small, carry)
    n_max = _lib.lib().vad_stream_tree_max_lds_nodes(probe.plan.handle)
    seen = set()
    for forest, K in ((small, 1), (small, 8), (random_forest(sizes_summing(n_max - 500), seed=41), 1),
                      (random_forest(sizes_summing(n_max), seed=40), 1)):
        labs, scs, seq, st, ser = serial(S, T, forest, 1)
        sb = fbatch(S, forest, carry, hops_per_step=K, scores=True, active=1)
        seen.add(sb.block_waves)
        lo, so = run(sb, dh, K)
        assert torch.equal(lo, labs) and torch.equal(so, scs) and same(state(sb), st)
        assert_equals_clip(forest, labs, scs, seq, 1)
    assert seen == {1, 2, 4}, seen


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


@pytest.mark.parametrize("walk", ["auto", "global"])
def test_forest_hop_kernel_ignores_stale_lds(torch_cuda, poison, walk):
    torch = torch_cuda
    S, K, T = 300, 8, 16
    carry, hops = _audio(S, T, seed=1400)
    dh = cuda(hops.astype(np.int16))
    forest = random_forest(sizes_between(3, 61, 70, seed=9), seed=90)  # two passes
    outs = []
    for v in (None, 1e30, -1e30, float("nan")):
        sb = fbatch(S, forest, carry, hops_per_step=K, input_dtype=torch.int16, tree_walk=walk, scores=True)
        labs = []
        for t in range(0, T, K):
            if v is not None:
                poison(v)
            sb.step_block(dh[t:t + K])
            labs += [sb.label_block.clone(), bits(sb.score_block).clone()]
        outs.append(labs + [bits(x) if x.dtype == torch.float32 else x for x in state(sb)])
    for o in outs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(o, outs[0]))
    assert len(torch.unique(outs[0][2])) == 2  # the second block's labels: both classes


# ---------------------------------------------------------------------------
# 7. sessions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("denoise", [False, True], ids=["plain", "denoise"])
def test_sessions(torch_cuda, denoise):
    torch = torch_cuda
    S, K, T = 5, 4, 16
    forest = _mixed_forest()
    carry, hops = _audio(S, T)
    dh = cuda(hops)
    kw = dict(hops_per_step=K, scores=True, active=1, denoise=denoise)
    nan = torch.tensor(float("nan")).view(torch.int32).item()

    def dn(sb):
        return [sb._spec.clone(), sb._noise.clone(), sb._est.clone(), sb.noise_count.clone()] if denoise else []

    # full counts, no restart: the plain batch, byte for byte
    plain, full = fbatch(S, forest, carry, **kw), fbatch(S, forest, carry, sessions=True, **kw)
    lp, sp = run(plain, dh, K)
    lf, sf = run(full, dh, K)
    assert torch.equal(lp, lf) and torch.equal(sp, sf) and same(state(plain) + dn(plain), state(full) + dn(full))
    # stream 1 stalls in block 1 (count 0), stream 2 takes 3 of block 1's hops, stream 3 restarts at block 2
    sb = fbatch(S, forest, carry, sessions=True, **kw)
    labs, scs = [], []
    for i in range(T // K):
        cnt = torch.full((S,), K, dtype=torch.int32, device="cuda")
        rst = torch.zeros(S, dtype=torch.uint8, device="cuda")
        if i == 1:
            cnt[1], cnt[2] = 0, 3
            before = [t[1].clone() for t in state(sb) + dn(sb)]
        rst[3] = i == 2
        sb.step_block(dh[i * K:(i + 1) * K], hop_counts=cnt, restart=rst)
        assert not sb.restart.any()  # consumed
        labs.append(sb.label_block.clone())
        scs.append(bits(sb.score_block).clone())
        if i == 1:
            assert same(before, [t[1] for t in state(sb) + dn(sb)])  # no hop, no restart: every byte kept
            assert (labs[1][:, 1] == 254).all() and (scs[1][:, 1] == nan).all()
            assert (labs[1][3, 2] == 254) and (scs[1][3, 2] == nan) and (labs[1][:3, 2] != 254).all()
    labs, scs = torch.cat(labs), torch.cat(scs)
    assert torch.equal(labs[:, 0], lp[:, 0]) and torch.equal(scs[:, 0], sp[:, 0])
    # the restarted stream: a fresh batch fed that session's hops
    fresh = fbatch(1, forest, np.zeros((1, L - H), np.float32), **kw)
    fresh.frames.zero_()
    lr, sr = run(fresh, dh[2 * K:, 3:4].contiguous(), K)
    assert torch.equal(labs[2 * K:, 3], lr[:, 0]) and torch.equal(scs[2 * K:, 3], sr[:, 0])
    assert (lr[:5] == 255).all()
    assert same([t[3] for t in state(sb) + dn(sb)], [t[0] for t in state(fresh) + dn(fresh)])


def test_a_replayed_graph_restarts_once(torch_cuda):
    torch = torch_cuda
    S, K, T = 5, 4, 12
    forest = _mixed_forest()
    carry, hops = _audio(S, T)
    dh = cuda(hops)
    g = fbatch(S, forest, carry, sessions=True, hops_per_step=K, scores=True)
    d = fbatch(S, forest, carry, sessions=True, hops_per_step=K, scores=True)
    g.capture()
    for i in range(T // K):
        if i == 1:
            g.restart[2] = 1
            d.restart[2] = 1
        g.inputs.copy_(dh[i * K:(i + 1) * K])
        g.step_block()
        d.step_block(dh[i * K:(i + 1) * K])
        assert not g.restart.any()
        assert torch.equal(g.label_block, d.label_block) and torch.equal(bits(g.score_block), bits(d.score_block))
    # the count runs 0..9 and then steps back by 5: 12 hops leave 7, 8 hops after the one restart 8 (a second
    # restart at the last block would leave 4)
    assert g.count.cpu().tolist() == [7, 7, 8, 7, 7] and same(state(g), state(d))


# ---------------------------------------------------------------------------
# 8. denoise with a multi-tree forest
# ---------------------------------------------------------------------------
def test_denoise_equals_clip_kernel_on_the_denoised_rows(torch_cuda):
    torch = torch_cuda
    S, T = 5, 24
    forest = _mixed_forest()
    out = {}
    for upd in (True, False):
        labs, scs, seq, st, sb = serial(S, T, forest, 1, denoise=True, noise_class=0, noise_update=upd)
        assert_equals_clip(forest, labs, scs, seq, 1)
        out[upd] = (labs, scs, seq, sb)
    labs = out[True][0]
    assert (out[True][3].noise_count > 0).any() and not out[False][3].noise_count.any()
    plain = serial(S, T, forest, 1)[2]
    assert not torch.equal(plain, out[True][2])  # the subtraction is live
    for s in range(S):  # equal until the first noise_class label: its estimate holds from the next hop on
        hit = (labs[:, s] == 0).nonzero()
        n = int(hit[0]) + 1 if len(hit) else T
        assert torch.equal(out[True][0][:n, s], out[False][0][:n, s]), s
        assert torch.equal(out[True][1][:n, s], out[False][1][:n, s]), s
        assert torch.equal(bits(out[True][2][s, :n]), bits(out[False][2][s, :n])), s


# ---------------------------------------------------------------------------
# 9. the segmenter
# ---------------------------------------------------------------------------
def test_segmenter_equals_the_clip_chain(torch_cuda):
    torch = torch_cuda
    from vad_amd import scores as SC, segments as SG
    S, K, T, g, m, pad, on, off = 5, 8, 24, 1, 1, (1, 2), 0.5, 0.45
    forest = _mixed_forest()
    carry, hops = _audio(S, T, seed=1600)
    c16, h16 = carry.astype(np.int16), hops.astype(np.int16)
    sb = fbatch(S, forest, c16, hops_per_step=K, input_dtype=torch.int16, scores=True, active=1)
    seg = sb.segmenter(on=on, off=off, pad=pad, max_gap=g, min_run=m)
    assert seg.active == 1
    seg.prime(cuda(c16))
    scs, outs = [], []
    for t0 in range(0, T, K):
        blk = cuda(h16[t0:t0 + K])
        sb.step_block(blk)
        v, n = seg.push(sb.score_block, blk)
        scs.append(sb.score_block.cpu().numpy().copy())
        outs.append((v.cpu().numpy().copy(), n.cpu().numpy().copy()))
    fv, fn = seg.flush()
    outs.append((fv.cpu().numpy(), fn.cpu().numpy()))
    sc = np.concatenate(scs)
    assert np.isnan(sc[:5]).all() and not np.isnan(sc[5:]).any()
    clip = np.concatenate([c16, h16.transpose(1, 0, 2).reshape(S, -1)], axis=1)
    rows, found = seg.segments(), seg.found.cpu().numpy()
    total = 0
    for s in range(S):
        lab = SC.dilate_labels(SG.smooth_labels(SC.score_labels(cuda(sc[5:, s]), on, off), g, m, active=1), pad, active=1)
        padded = np.concatenate([clip[s], np.zeros(1, np.int16)])  # the clip entries count frames with a strict >
        want = SG.label_segments(lab, len(padded), L, H, 0, 0, active=1)
        assert found[s] == int(want.counts[0].item()), s
        assert np.array_equal(rows[s], want.numpy()), s
        voiced, counts = SG.voiced_audio(cuda(padded), want)
        parts = [v[k, s, :n[k, s]] for v, n in outs for k in range(n.shape[0])]
        got = np.concatenate(parts).astype(np.int16) if parts else np.zeros(0, np.int16)
        assert np.array_equal(got, voiced[:int(counts[1].item())].cpu().numpy()), s
        total += len(rows[s])
    assert total > 0


def test_resampler_and_host_forms_run(torch_cuda):
    """The forms that only route through _hop_call: step_host, host_pipeline and
    resampler(rates) with a forest give the direct steps' labels."""
    torch = torch_cuda
    S, K, T = 5, 4, 16
    forest = _mixed_forest()
    labs, _, _, st, _ = serial(S, T, forest, 1)
    carry, hops = _audio(S, T)
    sb = fbatch(S, forest, carry, hops_per_step=K)
    sb.attach_host_io()
    got = []
    for b in range(T // K):
        sb.host_inputs.copy_(torch.from_numpy(hops[b * K:(b + 1) * K]))
        lab = sb.step_host()
        torch.cuda.current_stream().synchronize()
        got.append(lab.clone())
    assert torch.equal(torch.cat(got), labs.cpu())
    pb = fbatch(S, forest, carry, hops_per_step=K)
    pipe = pb.host_pipeline(2)
    got = []
    for b in range(T // K):
        pipe.host_inputs[b % 2].copy_(torch.from_numpy(hops[b * K:(b + 1) * K]))
        pipe.submit(b % 2)
        got.append(pipe.wait(b % 2).clone())
    pipe.drain()
    assert torch.equal(torch.cat(got), labs.cpu()) and same(state(pb), st)
    rb = fbatch(S, forest, carry, hops_per_step=K, sessions=True)
    rs = rb.resampler([16000])
    assert rs.out.data_ptr() == rb.inputs.data_ptr()
