"""The denoising hop entries and vad_stream_noise_load refuse bad arguments
before any HIP call.  Sizes, strides, layouts, alpha, update, a negative
noise_class and the state arrays (null, overlapping) are refused ahead of the
first look into a plan, so those cases run without a device (the plan and
buffer addresses below are never dereferenced).  What reads a plan (the
classifier's classes, a windowed or generic MFCC plan) and StreamBatch's own
ValueErrors that need a classifier are marked gpu."""
import pytest

E, U = -1, -2  # VAD_EINVAL, VAD_EUNSUPPORTED
N = None
PLAN, CLF, FR, HOP, RING, CNT, LAB, SC = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000
SPEC, ROWS, NCNT, EST = 0x100000, 0x200000, 0x300000, 0x400000
S, K, L, H = 4, 3, 400, 160
FFN = ["vad_stream_hops_denoise", "vad_stream_hops_denoise_i16"]
TREE = ["vad_stream_hops_tree_denoise", "vad_stream_hops_tree_denoise_i16"]
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from vad_amd import _lib
    return _lib.lib()


def hops(lib, fn, **kw):
    a = dict(plan=PLAN, clf=CLF, frames=FR, fs=L, L=L, hop=HOP, hs=H, H=H, S=S, K=K, hbs=S * H, ring=RING, count=CNT,
             labels=LAB, lbs=S, walk=0, active=1, scores=N, sbs=S, spec=SPEC, rows=ROWS, ncnt=NCNT, est=EST, alpha=0.9,
             cls=0, update=1)
    a.update(kw)
    walk = (a["walk"],) if "tree" in fn else ()
    return getattr(lib, fn)(a["plan"], a["clf"], a["frames"], a["fs"], a["L"], a["hop"], a["hs"], a["H"], a["S"],
                            a["K"], a["hbs"], a["ring"], a["count"], a["labels"], a["lbs"], *walk, a["active"],
                            a["scores"], a["sbs"], a["spec"], a["rows"], a["ncnt"], a["est"], a["alpha"], a["cls"],
                            a["update"], N)


@pytest.mark.parametrize("fn", FFN + TREE)
def test_hop_entries_refuse_without_a_device(lib, fn):
    spec_bytes, est_bytes = S * 5 * 256 * 4, S * 256 * 4
    cases = [dict(plan=N), dict(clf=N), dict(S=-1), dict(K=-1), dict(L=0), dict(L=1025, fs=1025), dict(H=0),
             dict(H=L + 1, hs=L + 1), dict(fs=L - 1), dict(hs=H - 1),
             dict(lbs=S - 1),                                   # label rows of two hops overlap
             dict(scores=SC, sbs=S - 1),                        # score rows likewise
             dict(hbs=0), dict(hbs=S * H - 1), dict(hbs=H, hs=K * H - 1),
             dict(alpha=1.0), dict(alpha=-0.01), dict(alpha=1.5), dict(alpha=NAN), dict(alpha=float("inf")),
             dict(update=2), dict(update=-1), dict(cls=-1),
             dict(spec=N), dict(rows=N), dict(ncnt=N), dict(est=N),  # a null state
             dict(rows=SPEC), dict(rows=SPEC + spec_bytes - 4), dict(spec=ROWS + 4),  # state arrays that overlap
             dict(est=ROWS + spec_bytes - 4), dict(est=SPEC - est_bytes + 4), dict(ncnt=EST + est_bytes - 4),
             dict(ncnt=ROWS)]
    if "tree" in fn:
        cases += [dict(walk=2), dict(walk=-1)]
    for kw in cases:
        assert hops(lib, fn, **kw) == E, kw
    # a bad argument stays bad when there is nothing to do
    assert hops(lib, fn, S=0, alpha=1.0) == E and hops(lib, fn, K=0, spec=N) == E and hops(lib, fn, S=0, plan=N) == E
    # arrays that touch without overlapping pass these checks: the next refusal is the null frames'
    # (the plans are read in between, so that case is in the gpu test below)


def load(lib, fn, **kw):
    a = dict(plan=PLAN, frames=FR, ss=5 * L, fs=L, L=L, n=5, S=S, rows=ROWS, ncnt=NCNT, est=EST, alpha=0.9)
    a.update(kw)
    return getattr(lib, fn)(a["plan"], a["frames"], a["ss"], a["fs"], a["L"], a["n"], a["S"], a["rows"], a["ncnt"],
                            a["est"], a["alpha"], N)


@pytest.mark.parametrize("fn", ["vad_stream_noise_load", "vad_stream_noise_load_i16"])
def test_load_entry_refuses_without_a_device(lib, fn):
    for kw in [dict(plan=N), dict(S=-1), dict(L=0), dict(L=1025, fs=1025, ss=5 * 1025), dict(n=0), dict(n=6, ss=6 * L),
               dict(n=-1), dict(fs=L - 1), dict(ss=5 * L - 1), dict(ss=0), dict(alpha=1.0), dict(alpha=NAN),
               dict(alpha=-1.0), dict(rows=N), dict(ncnt=N), dict(est=N), dict(est=ROWS), dict(ncnt=ROWS + 8),
               dict(frames=N)]:
        assert load(lib, fn, **kw) == E, kw
    assert load(lib, fn, S=0) == 0 and load(lib, fn, S=0, frames=N) == 0
    assert load(lib, fn, S=0, n=6) == E and load(lib, fn, S=0, rows=N) == E


def test_size_helpers(lib):
    assert lib.vad_stream_spec_ring_floats(7) == 7 * 5 * 256
    assert lib.vad_stream_noise_rows_floats(7) == 7 * 5 * 256
    assert lib.vad_stream_noise_est_floats(7) == 7 * 256
    assert lib.vad_stream_spec_ring_floats(1 << 40) == (1 << 40) * 1280  # 64-bit


# ---------------------------------------------------------------------------
# with real plans
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _tree(n_features=39, leaf=(0, 0, 1)):
    from vad_amd.tree import TreeClassifier
    return TreeClassifier([0, -1, -1], [0.0, 0.0, 0.0], [1, -1, -1], [2, -1, -1], list(leaf), [0, 0, 0],
                          list(range(max(leaf) + 1)), n_features)


def _ffn():
    from vad_amd.ffn import FFNClassifier, TOPOLOGY_BL13, random_layers
    return FFNClassifier(random_layers(TOPOLOGY_BL13, seed=3))


@pytest.mark.gpu
def test_refusals_that_need_a_plan(torch_cuda, lib):
    torch = torch_cuda
    from vad_amd import _lib
    from vad_amd.config import MfccConfig
    from vad_amd.plan import MfccPlan
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    hop, frames, ring, spec, rows, est = z(K, S, H) + 1, z(S, L), z(S, 5, 13), z(S, 5, 256), z(S, 5, 256), z(S, 256)
    count, ncnt = z(S, dtype=torch.int32) + 7, z(S, dtype=torch.int32)
    labels = torch.full((K, S), 0xAB, dtype=torch.uint8, device="cuda")
    bufs = dict(frames=_lib.ptr(frames), hop=_lib.ptr(hop), ring=_lib.ptr(ring), count=_lib.ptr(count),
                labels=_lib.ptr(labels), spec=_lib.ptr(spec), rows=_lib.ptr(rows), ncnt=_lib.ptr(ncnt),
                est=_lib.ptr(est))
    plan = MfccPlan.from_config(MfccConfig())
    ffn, tree, tree3 = _ffn(), _tree(), _tree(leaf=(0, 2, 1))
    n_ffn = ffn.layers[-1][1].shape[0]
    for fn, clf, n_cls in (("vad_stream_hops_denoise", ffn, n_ffn), ("vad_stream_hops_tree_denoise", tree, 2),
                           ("vad_stream_hops_tree_denoise", tree3, 3)):
        call = lambda **kw: hops(lib, fn, **{**bufs, "plan": plan.handle, "clf": clf.plan.handle, **kw})
        assert call(cls=n_cls) == E and call(cls=255) == E  # not a class of the plan
        sc = z(K, S)
        if clf is ffn:
            assert call(scores=_lib.ptr(sc), active=n_cls) == E and call(scores=_lib.ptr(sc), active=-1) == E
        else:
            assert call(scores=_lib.ptr(sc), active=0) == E  # a tree plan without a score table
        assert call(frames=N) == E and call(labels=N) == E
        for cfg in (MfccConfig(window="hamming"), MfccConfig(fft_n=1024)):  # not the hop kernel's FFT of 512
            other = MfccPlan.from_config(cfg)
            assert call(plan=other.handle) == U
        torch.cuda.synchronize()
        assert bool((labels == 0xAB).all()) and bool((count == 7).all()) and not bool(spec.any())
        assert call(cls=n_cls - 1) == 0  # the accepted call runs; its scores are null
        torch.cuda.synchronize()
        assert bool((labels < n_cls).all()) and bool(spec.any())
        labels.fill_(0xAB), count.fill_(7), spec.zero_(), rows.zero_(), est.zero_(), ncnt.zero_()
    fr = z(S, 5, L)
    other = MfccPlan.from_config(MfccConfig(fft_n=1024))
    assert load(lib, "vad_stream_noise_load", plan=other.handle, frames=_lib.ptr(fr), **{k: bufs[k] for k in
                                                                                         ("rows", "ncnt", "est")}) == U
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_stream_batch_refusals(torch_cuda):
    torch = torch_cuda
    from vad_amd.config import MfccConfig
    from vad_amd.stream import StreamBatch
    ffn = _ffn()
    with pytest.raises(ValueError, match="three"):
        StreamBatch(3, ffn, denoise=True, kernel="three")
    for bad in (1.0, -0.1, NAN):
        with pytest.raises(ValueError, match="alpha"):
            StreamBatch(3, ffn, denoise=True, alpha=bad)
    with pytest.raises(ValueError, match="noise_class"):
        StreamBatch(3, ffn, denoise=True, noise_class=ffn.layers[-1][1].shape[0])
    with pytest.raises(ValueError, match="noise_class"):
        StreamBatch(3, _tree(), denoise=True, noise_class=2)
    with pytest.raises(ValueError, match="fft_n"):
        StreamBatch(3, ffn, cfg=MfccConfig(fft_n=1024), denoise=True, kernel="hop")
    plain = StreamBatch(3, ffn)
    for name in ("spec_ring", "noise_rows", "noise_estimate"):
        with pytest.raises(ValueError, match="denoise"):
            getattr(plain, name)
    with pytest.raises(ValueError, match="denoise"):
        plain.load_noise(torch.zeros((3, 5, 400), device="cuda"))
    assert not hasattr(plain, "noise_count") and not hasattr(plain, "_spec")  # nothing more allocated
    sb = StreamBatch(3, ffn, denoise=True)
    for bad in (torch.zeros((3, 6, 400), device="cuda"), torch.zeros((3, 0, 400), device="cuda"),
                torch.zeros((2, 5, 400), device="cuda"), torch.zeros((3, 5, 399), device="cuda"),
                torch.zeros((3, 5, 400), dtype=torch.int16, device="cuda"), torch.zeros((3, 5, 400))):
        with pytest.raises(ValueError, match="frames"):
            sb.load_noise(bad)
