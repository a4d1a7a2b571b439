"""vad_stream_hops_tree(_i16) and vad_stream_step_tree refuse bad arguments
before any HIP call.  Sizes, strides, layouts, the walk selector and null
buffers are refused ahead of the first look into a plan, so those cases run
without a device (the plan and buffer addresses below are never dereferenced);
what depends on a plan's contents (the tree's feature count, a windowed or
generic MFCC plan) needs real plans and is marked gpu: there the label buffer
is pre-filled and must stay unwritten."""
import pytest

E, U = -1, -2  # VAD_EINVAL, VAD_EUNSUPPORTED
N = None
PLAN, TREE, FR, HOP, RING, CNT, LAB = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000
S, K, L, H = 4, 3, 400, 160
HOPS = ["vad_stream_hops_tree", "vad_stream_hops_tree_i16"]


@pytest.fixture(scope="module")
def lib():
    from vad_amd import _lib
    return _lib.lib()


def hops(lib, fn, **kw):
    a = dict(plan=PLAN, tree=TREE, frames=FR, fs=L, L=L, hop=HOP, hs=H, H=H, S=S, K=K, hbs=S * H, ring=RING,
             count=CNT, labels=LAB, lbs=S, walk=0)
    a.update(kw)
    return getattr(lib, fn)(a["plan"], a["tree"], a["frames"], a["fs"], a["L"], a["hop"], a["hs"], a["H"], a["S"],
                            a["K"], a["hbs"], a["ring"], a["count"], a["labels"], a["lbs"], a["walk"], N)


@pytest.mark.parametrize("fn", HOPS)
def test_hop_entries_refuse_without_a_device(lib, fn):
    for kw in [dict(plan=N), dict(tree=N), dict(S=-1), dict(K=-1), dict(L=0), dict(L=-400), dict(L=1025, fs=1025),
               dict(H=0), dict(H=-1), dict(H=L + 1, hs=L + 1), dict(fs=L - 1), dict(fs=0), dict(hs=H - 1), dict(hs=0),
               dict(hs=-H),
               dict(lbs=S - 1), dict(lbs=0), dict(lbs=-S),        # label rows of two hops overlap
               dict(hbs=0), dict(hbs=-S * H),                     # a block repeats or walks backwards
               dict(hbs=S * H - 1),                               # hop-major blocks overlap
               dict(hbs=H, hs=K * H - 1),                         # stream-major rows overlap
               dict(hbs=H - 1, hs=K * H),                         # a stream's hops overlap each other
               dict(walk=2), dict(walk=-1), dict(walk=1 << 20),
               dict(frames=N), dict(hop=N), dict(ring=N), dict(count=N), dict(labels=N)]:
        assert hops(lib, fn, **kw) == E, kw
    # nothing to do: success, no pointer touched
    assert hops(lib, fn, S=0) == 0 and hops(lib, fn, K=0) == 0
    assert hops(lib, fn, S=0, frames=N, hop=N, ring=N, count=N, labels=N) == 0
    assert hops(lib, fn, K=0, frames=N, hop=N, ring=N, count=N, labels=N) == 0
    # a bad argument stays bad when there is nothing to do
    assert hops(lib, fn, S=0, walk=2) == E and hops(lib, fn, K=0, hs=H - 1) == E and hops(lib, fn, S=0, plan=N) == E
    # one hop: the block strides are not used
    assert hops(lib, fn, K=1, S=0, hbs=0, lbs=0) == 0


def test_step_entry_refuses_without_a_device(lib):
    def step(**kw):
        a = dict(plan=PLAN, tree=TREE, frames=FR, fs=L, L=L, S=S, ring=RING, count=CNT, labels=LAB, scratch=HOP)
        a.update(kw)
        return lib.vad_stream_step_tree(a["plan"], a["tree"], a["frames"], a["fs"], a["L"], a["S"], a["ring"],
                                        a["count"], a["labels"], a["scratch"], N)

    for kw in [dict(plan=N), dict(tree=N), dict(S=-1), dict(L=0), dict(fs=-1), dict(frames=N), dict(ring=N),
               dict(count=N), dict(labels=N), dict(scratch=N)]:
        assert step(**kw) == E, kw
    assert step(S=0) == 0 and step(S=0, frames=N, ring=N, count=N, labels=N, scratch=N) == 0


# ---------------------------------------------------------------------------
# with real plans
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _tree(n_features, feature=0):
    from vad_amd.tree import TreeClassifier
    return TreeClassifier([feature, -1, -1], [0.0, 0.0, 0.0], [1, -1, -1], [2, -1, -1], [0, 0, 1], [0, 0, 0], [0, 1],
                          n_features)


class _Bufs:
    def __init__(self, torch, cfg, dtype):
        from vad_amd.plan import MfccPlan
        self.plan = MfccPlan.from_config(cfg)
        self.frames = torch.zeros((S, cfg.frame_size), device="cuda")
        self.hop = torch.ones((K, S, cfg.hop), dtype=dtype, device="cuda")
        self.ring = torch.zeros((S, 5, cfg.n_mfcc), device="cuda")
        self.count = torch.full((S,), 7, dtype=torch.int32, device="cuda")  # past the warm-up: a run would label
        self.labels = torch.full((K, S), 0xAB, dtype=torch.uint8, device="cuda")
        self.scratch = torch.zeros((S, cfg.n_mfcc), device="cuda")
        self.cfg = cfg

    def hops(self, lib, fn, tree, walk=0):
        from vad_amd import _lib
        c = self.cfg
        return getattr(lib, fn)(self.plan.handle, tree.plan.handle, _lib.ptr(self.frames), c.frame_size, c.frame_size,
                                _lib.ptr(self.hop), c.hop, c.hop, S, K, S * c.hop, _lib.ptr(self.ring),
                                _lib.ptr(self.count), _lib.ptr(self.labels), S, walk, _lib.stream_ptr())

    def step(self, lib, tree):
        from vad_amd import _lib
        c = self.cfg
        return lib.vad_stream_step_tree(self.plan.handle, tree.plan.handle, _lib.ptr(self.frames), c.frame_size,
                                        c.frame_size, S, _lib.ptr(self.ring), _lib.ptr(self.count),
                                        _lib.ptr(self.labels[0]), _lib.ptr(self.scratch), _lib.stream_ptr())

    def untouched(self, torch):
        torch.cuda.synchronize()
        return bool((self.labels == 0xAB).all()) and bool((self.count == 7).all())


@pytest.mark.gpu
@pytest.mark.parametrize("fn,dtype", [("vad_stream_hops_tree", "float32"), ("vad_stream_hops_tree_i16", "int16")])
def test_refusals_that_need_a_plan(torch_cuda, lib, fn, dtype):
    torch = torch_cuda
    from vad_amd.config import MfccConfig
    dt = getattr(torch, dtype)
    b = _Bufs(torch, MfccConfig(), dt)
    t39, t40 = _tree(39), _tree(40, feature=39)  # alive until the last launch has run
    # a feature index is an LDS offset: the tree may read 3 * mfcc_n features, not one more
    assert b.hops(lib, fn, t40) == E
    assert b.step(lib, t40) == E
    assert b.hops(lib, fn, t39, walk=2) == E
    assert b.untouched(torch)
    # windowed and generic plans: not the hop kernel's
    w = _Bufs(torch, MfccConfig(window="hamming"), dt)
    assert w.hops(lib, fn, t39) == U and w.hops(lib, fn, t39, walk=1) == U
    g = _Bufs(torch, MfccConfig(fft_n=1024), dt)
    assert g.hops(lib, fn, t39) == U
    assert w.untouched(torch) and g.untouched(torch)
    # ... and they work through the three-kernel step
    for x in (w, g):
        assert x.step(lib, t39) == 0
        torch.cuda.synchronize()
        assert bool((x.labels[0] <= 1).all()) and bool((x.labels[1:] == 0xAB).all()) and bool((x.count == 8).all())
    # the accepted call runs
    assert b.hops(lib, fn, t39) == 0 and b.hops(lib, fn, t39, walk=1) == 0
    torch.cuda.synchronize()
    assert bool((b.labels <= 1).all())


@pytest.mark.gpu
def test_max_lds_nodes(torch_cuda, lib):
    from vad_amd.config import MfccConfig
    from vad_amd.plan import MfccPlan
    p26 = MfccPlan.from_config(MfccConfig())
    p40 = MfccPlan.from_config(MfccConfig(n_filters=40))
    n26, n40 = (lib.vad_stream_tree_max_lds_nodes(p.handle) for p in (p26, p40))
    # 160 KiB less one wave's scratch (1344 floats) and the plan's blob, in 16-B nodes
    assert 8192 < n40 < n26 < (160 * 1024 - 1344 * 4) // 16
    assert lib.vad_stream_tree_max_lds_nodes(None) == -1


@pytest.mark.gpu
def test_stream_batch_refusals(torch_cuda):
    torch = torch_cuda
    from vad_amd.config import MfccConfig
    from vad_amd.stream import StreamBatch
    with pytest.raises(ValueError, match="window"):
        StreamBatch(3, _tree(39), cfg=MfccConfig(window="hamming"), kernel="hop")
    with pytest.raises(ValueError, match="tree_walk"):
        StreamBatch(3, _tree(39), tree_walk="lds")
    with pytest.raises(ValueError, match="features"):
        StreamBatch(3, _tree(40))
    sb = StreamBatch(3, _tree(39), cfg=MfccConfig(window="hamming"), kernel="three")
    assert sb.classifier is sb.ffn and sb.is_tree
    for _ in range(7):
        lab = sb.step(torch.ones((3, 160), device="cuda"))
    assert bool((lab <= 1).all())
