"""StreamBatch(sessions=True): per-stream hop counts and restarts inside the hop
kernels (vad_stream_hops_sessions and its _i16 / tree forms), against the
plain hop kernels run session by session (tests/stream_sessions_reference.py).
Every comparison is bit for bit."""
import functools

import numpy as np
import pytest

import stream_sessions_reference as R
from test_gpu_stream_scores import L, H, cuda, ffn, torch_cuda, tree_with_scores  # noqa: F401

pytestmark = pytest.mark.gpu

S19, BLOCKS = 19, 12


def bits(t):
    import torch
    return t if t.dtype in (torch.uint8, torch.int32) else t.contiguous().view(torch.int32)


def same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def clf_for(name):
    return tree_with_scores() if name == "tree" else ffn("bl13")  # bl13: 13-64-64-2


@functools.lru_cache(maxsize=None)
def samples(n_blocks, K, S, hop=H, seed=4100):
    """(B, K, S, hop) integer-valued samples (exact as int16 and as fp32): a
    noise floor with louder stretches, so that both classes occur."""
    rng = np.random.default_rng(seed + 17 * K + S)
    x = rng.normal(0.0, 300.0, size=(n_blocks, K, S, hop))
    loud = rng.random((n_blocks, K, S, 1)) < 0.4
    x = np.where(loud, x * 12.0, x)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def make(torch, S, clf, K, dtype, scores, denoise, **kw):
    from vad_amd.stream import StreamBatch
    dn = dict(denoise=True, noise_update=True) if denoise else {}
    return StreamBatch(S, clf, hops_per_step=K, input_dtype=getattr(torch, dtype), scores=scores, **dn, **kw)


@functools.lru_cache(maxsize=None)
def common_class(name, K):
    """The class most windows of the schedule test's samples get from the
    plain kernels without denoising: as noise_class it makes the noise rows
    fill (a stream's first windows do not depend on the noise class)."""
    import torch
    sb = make(torch, S19, clf_for(name), K, "float32", False, False)
    blocks = cuda(samples(BLOCKS, K, S19)).to(torch.float32)
    seen = torch.cat([sb.step_block(blocks[b]).clone().flatten() if K > 1 else sb.step(blocks[b, 0]).clone()
                      for b in range(BLOCKS)])
    return int(torch.bincount(seen[seen != 255].long()).argmax())


def state_names(sb):
    return R.STATE + (R.DN_STATE if sb.denoise else ())


def check_block(sb, exp, b, where):
    import torch
    lab, sc, st = exp.block(b)
    assert torch.equal(sb.label_block, lab), (where, b, "labels")
    if sb.scores:
        assert same(sb.score_block, sc), (where, b, "scores")
    bad = [k for k in state_names(sb) if not same(getattr(sb, k), st[k])]
    assert not bad, (where, b, bad)
    assert not bool(sb.restart.any()), (where, b, "restart not consumed")


def expected(torch, clf, blocks, counts, restart, K, dtype, scores, denoise, **kw):
    return R.Expected(torch, lambda n: make(torch, n, clf, 1, dtype, scores, denoise, **kw), blocks, counts, restart, K)


# ---------------------------------------------------------------------------
# 1. schedules against the plain kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("denoise", [False, True], ids=["plain", "denoise"])
@pytest.mark.parametrize("scores", [False, True], ids=["labels", "scores"])
@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("name", ["bl13", "tree"])
def test_schedules_against_the_plain_kernels(torch_cuda, name, K, dtype, scores, denoise):
    torch = torch_cuda
    clf = clf_for(name)
    counts, restart = R.make_schedule(S19, K, BLOCKS, seed=900 + K)
    blocks = cuda(samples(BLOCKS, K, S19)).to(getattr(torch, dtype))
    kw = dict(noise_class=common_class(name, K)) if denoise else {}
    exp = expected(torch, clf, blocks, counts, restart, K, dtype, scores, denoise, **kw)
    ses = exp.ses
    # the schedule holds what it must: a restart on a count of 0, the warm-up reappearing, clamped counts
    assert restart[5, 3] and counts[5, 3] == 0 and ses.at[8][4][1] == 0 and ses.at[7][4][1] + K >= 7
    assert counts[:, 5].max() > K and counts[:, 5].min() < 0 and len(ses.rows) > S19
    sb = make(torch, S19, clf, K, dtype, scores, denoise, sessions=True, **kw)
    where = (name, K, dtype, scores, denoise)
    seen_255_again = live_restarts = False
    for b in range(BLOCKS):
        c, r = cuda(counts[b]), cuda(restart[b])
        if denoise:  # a restart that meets noise rows and an estimate
            live_restarts |= bool(((sb.noise_count > 0) & sb._est.any(dim=1) & (r != 0)).any())
        if K == 1:
            sb.step(blocks[b, 0], hop_counts=c, restart=r)
        else:
            sb.step_block(blocks[b], hop_counts=c, restart=r)
        check_block(sb, exp, b, where)
        if b >= 8:
            seen_255_again |= bool((sb.label_block[:, 4] == 255).any())
    assert "sessions" in sb._hop_name
    assert seen_255_again and bool((sb.label_block[:, 1] == R.NO_HOP).all())
    assert live_restarts or not denoise


# ---------------------------------------------------------------------------
# 2. full sessions equal a plain batch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("denoise", [False, True], ids=["plain", "denoise"])
@pytest.mark.parametrize("name", ["bl13", "tree"])
@pytest.mark.parametrize("S", [3, 19])
def test_full_sessions_equal_a_plain_batch(torch_cuda, S, name, denoise):
    torch = torch_cuda
    K, clf = 8, clf_for(name)
    blocks = cuda(samples(4, K, S)).to(torch.float32)
    a = make(torch, S, clf, K, "float32", True, denoise, sessions=True)
    b = make(torch, S, clf, K, "float32", True, denoise)
    assert bool((a.hop_counts == K).all()) and not bool(a.restart.any())
    for i in range(blocks.shape[0]):
        a.step_block(blocks[i]), b.step_block(blocks[i])
        assert torch.equal(a.label_block, b.label_block) and same(a.score_block, b.score_block), i
        bad = [k for k in state_names(a) if not same(getattr(a, k), getattr(b, k))]
        assert not bad, (i, bad)
    assert "sessions" in a._hop_name and "sessions" not in b._hop_name
    assert bool((a.label_block != 255).all()) and bool((a.label_block != R.NO_HOP).all())


# ---------------------------------------------------------------------------
# 3. a stalled stream keeps its state
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("bl13", "float32"), ("tree", "int16")])
def test_a_stalled_stream_keeps_its_state(torch_cuda, name, dtype):
    torch = torch_cuda
    S, K = 5, 3
    sb = make(torch, S, clf_for(name), K, dtype, True, True, sessions=True)
    blocks = cuda(samples(2, K, S)).to(getattr(torch, dtype))
    sb.step_block(blocks[0])
    names = state_names(sb)
    for k in names:  # a byte pattern no computation would leave (as fp32 a NaN with a payload)
        getattr(sb, k)[1:2].view(torch.uint8).fill_(0xA5)
    before = {k: getattr(sb, k).clone() for k in names}
    counts = torch.tensor([K, 0, 2, K, 1], dtype=torch.int32, device="cuda")
    sb.step_block(blocks[1], hop_counts=counts)
    for k in names:
        assert same(getattr(sb, k)[1], before[k][1]), k
        assert bool((getattr(sb, k)[1:2].view(torch.uint8) == 0xA5).all()), k
    for k in R.STATE + ("_spec",):  # the others moved on
        assert not same(getattr(sb, k)[0], before[k][0]) and not same(getattr(sb, k)[2], before[k][2]), k
    assert bool((sb.label_block[:, 1] == R.NO_HOP).all()) and bool(torch.isnan(sb.score_block[:, 1]).all())
    assert bool(sb.label_block[2, 2] == R.NO_HOP) and bool((sb.label_block[:2, 2] != R.NO_HOP).all())


# ---------------------------------------------------------------------------
# 4. a restart is consumed once
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,K", [("bl13", 3), ("tree", 1)])
def test_a_restart_is_consumed_once(torch_cuda, name, K):
    torch = torch_cuda
    S, clf = 7, clf_for(name)
    blocks = cuda(samples(5, K, S)).to(torch.float32)
    counts = np.full((5, S), K, np.int32)
    restart = np.zeros((5, S), np.uint8)
    restart[2, 2] = restart[2, 6] = 1  # set once, before the first of three replays
    exp = expected(torch, clf, blocks, counts, restart, K, "float32", True, True)
    sb = make(torch, S, clf, K, "float32", True, True, sessions=True)
    sb.capture()
    for b in range(5):
        sb.inputs.copy_(blocks[b])
        if b == 2:
            sb.restart.copy_(cuda(restart[2]))
        sb.step() if K == 1 else sb.step_block()  # a replay: restart and hop_counts are read in place
        check_block(sb, exp, b, (name, K))
    if K == 1:
        assert sb.graph_direct  # still one kernel node


# ---------------------------------------------------------------------------
# 5. graph and host I/O equal direct calls
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype,denoise", [("bl13", "int16", True), ("tree", "float32", False)])
def test_graph_and_host_io_equal_direct_calls(torch_cuda, name, dtype, denoise):
    torch = torch_cuda
    K, B, clf = 3, 6, clf_for(name)
    counts, restart = R.make_schedule(S19, K, 10, seed=77)
    counts, restart = counts[2:2 + B], restart[2:2 + B]
    blocks = cuda(samples(B, K, S19)).to(getattr(torch, dtype))
    mk = lambda: make(torch, S19, clf, K, dtype, False, denoise, sessions=True)
    direct, graph, ghost, host, piped = mk(), mk(), mk(), mk(), mk()
    graph.capture()
    ghost.capture(host_io=True)
    host.attach_host_io()
    pipe = piped.host_pipeline(depth=2)
    want = []
    for b in range(B):
        direct.step_block(blocks[b], hop_counts=cuda(counts[b]), restart=cuda(restart[b]))
        want.append((direct.label_block.clone(), {k: getattr(direct, k).clone() for k in state_names(direct)}))
    for b in range(B):
        graph.inputs.copy_(blocks[b])
        graph.step_block(hop_counts=cuda(counts[b]), restart=cuda(restart[b]))
        for sb in (ghost, host):
            sb.host_inputs.copy_(blocks[b])
            sb.host_hop_counts.copy_(torch.from_numpy(counts[b]))
            sb.host_restart.copy_(torch.from_numpy(restart[b]))
            got = sb.step_host()
            torch.cuda.synchronize()
            assert torch.equal(got.cuda(), want[b][0]), (b, sb is ghost)
        for sb in (graph, ghost, host):
            assert torch.equal(sb.label_block, want[b][0]), b
            bad = [k for k, v in want[b][1].items() if not same(getattr(sb, k), v)]
            assert not bad and not bool(sb.restart.any()), (b, bad)
    for b in range(B):  # two blocks in flight
        d = b % 2
        if b >= 2:
            assert torch.equal(pipe.wait(d).cuda(), want[b - 2][0]), b
        pipe.host_inputs[d].copy_(blocks[b])
        pipe.host_hop_counts[d].copy_(torch.from_numpy(counts[b]))
        pipe.host_restart[d].copy_(torch.from_numpy(restart[b]))
        pipe.submit(d)
    for b in (B - 2, B - 1):
        assert torch.equal(pipe.wait(b % 2).cuda(), want[b][0]), b
    pipe.drain()
    bad = [k for k, v in want[B - 1][1].items() if not same(getattr(piped, k), v)]
    assert not bad, bad


# ---------------------------------------------------------------------------
# 6. a 16-chunk build
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,denoise", [("bl13", True), ("tree", True), ("bl13", False), ("tree", False)])
def test_a_16_chunk_build(torch_cuda, name, denoise):
    """frame_size 512 > 448: the NR = 16 kernels."""
    torch = torch_cuda
    from vad_amd.config import MfccConfig
    cfg = MfccConfig(frame_size=512)
    S, K, B, clf = 3, 3, 5, clf_for(name)
    counts = np.full((B, S), K, np.int32)
    restart = np.zeros((B, S), np.uint8)
    counts[1, 1], counts[3, 1] = 0, 2  # a stall, a short block
    restart[3, 2] = 1  # a restart after 9 hops
    blocks = cuda(samples(B, K, S, hop=cfg.hop)).to(torch.float32)
    exp = expected(torch, clf, blocks, counts, restart, K, "float32", True, denoise, cfg=cfg)
    sb = make(torch, S, clf, K, "float32", True, denoise, sessions=True, cfg=cfg)
    for b in range(B):
        sb.step_block(blocks[b], hop_counts=cuda(counts[b]), restart=cuda(restart[b]))
        check_block(sb, exp, b, (name, denoise))
