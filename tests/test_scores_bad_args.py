"""The score entries refuse bad arguments with VAD_EINVAL before any HIP call
(no GPU here; the device pointers below are never dereferenced), do nothing,
successfully, for n == 0, and the Python layer raises before it reaches them."""
import ctypes

import numpy as np
import pytest

E = -1  # VAD_EINVAL
N = None  # NULL
A, B, WS, T0, T1, H = 0x100000, 0x800000, 0x1000000, 0x2000000, 0x2100000, 0x3000000
f = ctypes.c_float


@pytest.fixture(scope="module")
def lib():
    from vad_amd import _lib
    return _lib.lib()


def test_workspace_size(lib):
    assert lib.vad_scores_workspace_bytes(0) == 0 and lib.vad_scores_workspace_bytes(-4) == 0
    assert lib.vad_scores_workspace_bytes(1) == 256 and lib.vad_scores_workspace_bytes(1024) == 256
    assert lib.vad_scores_workspace_bytes(8 * 1024 + 1) == 512  # 9 tiles x 4 arrays x 8 bytes, in 256-byte steps


def test_scores_from_logits_refuses(lib):
    def call(**kw):
        a = dict(z=A, n=100, c=2, act=1, s=B)
        a.update(kw)
        return lib.vad_scores_from_logits(a["z"], a["n"], a["c"], a["act"], a["s"], N)

    for kw in (dict(z=N), dict(s=N), dict(n=-1), dict(c=0), dict(c=9), dict(c=-2), dict(act=-1), dict(act=2),
               dict(c=3, act=3), dict(z=A + 2), dict(s=B + 1), dict(s=A), dict(s=A + 4 * 199), dict(n=2 ** 62)):
        assert call(**kw) == E, kw
    assert call(n=0) == 0 and call(n=0, z=N, s=N) == 0
    assert call(n=0, act=2) == E and call(n=0, c=9) == E  # a bad argument stays bad with nothing to do


@pytest.mark.parametrize("batch", [False, True])
def test_score_labels_refuses(lib, batch):
    need = lib.vad_scores_workspace_bytes(5000)

    def call(**kw):
        a = dict(s=A, n=5000, on=0.7, off=0.3, out=B, ws=WS, wsb=need, f0=T0, nr=T1, nc=3)
        a.update(kw)
        if batch:
            return lib.vad_batch_score_labels(a["s"], a["n"], a["f0"], a["nr"], a["nc"], f(a["on"]), f(a["off"]),
                                              a["out"], a["ws"], a["wsb"], N)
        return lib.vad_score_labels(a["s"], a["n"], f(a["on"]), f(a["off"]), a["out"], a["ws"], a["wsb"], N)

    bad = [dict(s=N), dict(out=N), dict(ws=N), dict(n=-1), dict(on=0.3, off=0.7), dict(on=1.5), dict(off=-0.1),
           dict(on=float("nan")), dict(off=float("nan")), dict(on=1.0, off=1.0000001),
           dict(wsb=need - 1), dict(wsb=0), dict(ws=WS + 8),     # short or misaligned workspace
           dict(out=A), dict(out=A + 4 * 5000 - 1),              # out aliases the scores
           dict(ws=A), dict(ws=B), dict(n=2 ** 41)]              # the workspace aliases an array
    if batch:
        bad += [dict(f0=N), dict(nr=N), dict(nc=-1)]
    for kw in bad:
        assert call(**kw) == E, kw
    assert call(n=0) == 0 and call(n=0, s=N, out=N, ws=N, wsb=0) == 0
    assert call(n=0, on=0.2, off=0.4) == E
    if batch:
        assert call(n=0, nc=0, f0=N, nr=N) == 0


@pytest.mark.parametrize("batch", [False, True])
def test_label_dilate_refuses(lib, batch):
    need = lib.vad_scores_workspace_bytes(5000)

    def call(**kw):
        a = dict(lab=A, n=5000, act=1, pb=2, pa=3, out=B, ws=WS, wsb=need, f0=T0, nr=T1, nc=3)
        a.update(kw)
        if batch:
            return lib.vad_batch_label_dilate(a["lab"], a["n"], a["f0"], a["nr"], a["nc"], a["act"], a["pb"],
                                              a["pa"], a["out"], a["ws"], a["wsb"], N)
        return lib.vad_label_dilate(a["lab"], a["n"], a["act"], a["pb"], a["pa"], a["out"], a["ws"], a["wsb"], N)

    bad = [dict(lab=N), dict(out=N), dict(ws=N), dict(n=-1), dict(pb=-1), dict(pa=-1), dict(act=-1), dict(act=256),
           dict(wsb=need - 1), dict(ws=WS + 4), dict(out=A), dict(out=A + 4999), dict(ws=A), dict(ws=B)]
    if batch:
        bad += [dict(f0=N), dict(nr=N), dict(nc=-1)]
    for kw in bad:
        assert call(**kw) == E, kw
    assert call(n=0) == 0 and call(n=0, lab=N, out=N, ws=N, wsb=0) == 0 and call(n=0, pb=-1) == E


def test_reference_labels_refuses(lib):
    def one(**kw):
        a = dict(iv=A, k=4, n=1000, fs=400, hop=160, out=B)
        a.update(kw)
        return lib.vad_reference_labels(a["iv"], a["k"], a["n"], a["fs"], a["hop"], a["out"], N)

    def many(**kw):
        a = dict(iv=A, k=4, r0=H, f0=T0, nr=T1, nc=2, n=1000, fs=400, hop=160, out=B)
        a.update(kw)
        return lib.vad_batch_reference_labels(a["iv"], a["k"], a["r0"], a["f0"], a["nr"], a["nc"], a["n"], a["fs"],
                                              a["hop"], a["out"], N)

    for call in (one, many):
        for kw in (dict(iv=N), dict(out=N), dict(k=-1), dict(n=-1), dict(fs=0), dict(hop=0), dict(hop=-160),
                   dict(iv=A + 4), dict(out=A + 8), dict(n=2 ** 62)):
            assert call(**kw) == E, (call.__name__, kw)
        assert call(n=0) == 0 and call(n=0, out=N) == 0 and call(n=0, hop=0) == E
    assert one(k=0, iv=N, n=0) == 0
    for kw in (dict(r0=N), dict(f0=N), dict(nr=N), dict(nc=-1)):
        assert many(**kw) == E, kw


def test_histograms_refuse(lib):
    def call(fn, **kw):
        a = dict(x=A, ref=B, n=5000, bins=1024, hist=H)
        a.update(kw)
        return getattr(lib, fn)(a["x"], a["ref"], a["n"], a["bins"], a["hist"], N)

    for fn in ("vad_score_histogram_f32", "vad_score_histogram_u8"):
        top = 4096 if fn.endswith("f32") else 256
        for kw in (dict(x=N), dict(ref=N), dict(hist=N), dict(n=-1), dict(bins=0), dict(bins=-1), dict(bins=top + 1),
                   dict(bins=4097), dict(hist=H + 4), dict(hist=A), dict(hist=B), dict(n=2 ** 39)):
            assert call(fn, bins=kw.pop("bins", min(1024, top)), **kw) == E, (fn, kw)
        assert call(fn, n=0, bins=top) == 0 and call(fn, n=0, x=N, ref=N, bins=2) == 0
        assert call(fn, n=0, bins=0) == E and call(fn, n=0, hist=N, bins=2) == E
    assert call("vad_score_histogram_f32", x=A + 2) == E


def test_tree_score_entries_refuse(lib):
    feat = np.array([0, -1, -1], np.int32)
    thr = np.array([0.5, 0, 0], np.float64)
    left, right = np.array([1, -1, -1], np.int32), np.array([2, -1, -1], np.int32)
    leaf, nan_left = np.array([0, 0, 1], np.int32), np.zeros(3, np.uint8)
    h = ctypes.c_void_p()
    rc = lib.vad_tree_plan_create(3, feat.ctypes.data, thr.ctypes.data, left.ctypes.data, right.ctypes.data,
                                  leaf.ctypes.data, nan_left.ctypes.data, 39, ctypes.byref(h))
    if rc != 0:  # the plan's tables are device memory: without a device there is no plan to hand in
        h = None
    for t in ([None] if h is None else [None, h]):
        want_ok = t is not None
        assert lib.vad_tree_predict_scores(t, H, A, 0, B, N) == (0 if want_ok else E)
        assert lib.vad_tree_predict_scores(t, H, A, -1, B, N) == E
        assert lib.vad_features_tree_scores(t, H, A, -1, 13, 0, B, N) == E
        assert lib.vad_features_tree_scores(t, H, A, 100, 0, 0, B, N) == E
        assert lib.vad_features_tree_scores(t, H, A, 100, 17, 0, B, N) == E
        assert lib.vad_features_tree_scores(t, H, A, 100, 13, 2, B, N) == E
        if want_ok:
            assert lib.vad_features_tree_scores(t, H, A, 5, 13, 0, B, N) == 0  # no window: nothing to do
            assert lib.vad_features_tree_scores(t, H, A, 100, 12, 0, B, N) == E  # 39 features need 13 coefficients
            for kw in (dict(ns=N), dict(x=N), dict(s=N), dict(s=A)):
                a = dict(ns=H, x=A, s=B)
                a.update(kw)
                assert lib.vad_tree_predict_scores(t, a["ns"], a["x"], 10, a["s"], N) == E, kw
                assert lib.vad_features_tree_scores(t, a["ns"], a["x"], 100, 13, 0, a["s"], N) == E, kw
    if h is not None:
        assert lib.vad_tree_plan_destroy(h) == 0


def test_python_layer_raises_before_any_launch(monkeypatch):
    """Types, devices, contiguity and ranges are checked on the host: with
    every entry of the unit replaced by one that fails the test, the calls
    below still raise TypeError / ValueError."""
    import torch
    from vad_amd import _lib, scores as S

    class Trap:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was reached")

    monkeypatch.setattr(_lib, "lib", lambda: Trap())
    cpu_f = torch.zeros(8)
    cpu_u = torch.zeros(8, dtype=torch.uint8)
    for call in (lambda: S.score_labels(cpu_f, 0.5), lambda: S.score_labels(np.zeros(8, np.float32), 0.5),
                 lambda: S.score_labels(cpu_u, 0.5), lambda: S.dilate_labels(cpu_u, (1, 1)),
                 lambda: S.dilate_labels(cpu_f, (1, 1)), lambda: S.histogram(cpu_f, cpu_u),
                 lambda: S.confusion(cpu_u, cpu_u), lambda: S.scores_from_logits(torch.zeros(4, 2)),
                 lambda: S.scores_from_logits([[0.0, 1.0]])):
        with pytest.raises(TypeError):
            call()
    for on, off in ((0.3, 0.7), (1.5, None), (-0.1, None), (0.5, -0.2), (float("nan"), None)):
        with pytest.raises(ValueError):
            S._check_thresholds(on, off)
    assert S._check_thresholds(0.6, None) == (0.6, 0.6) and S._check_thresholds(1, 0) == (1.0, 0.0)
    for pad in ((-1, 0), (0, -2)):
        with pytest.raises(ValueError):
            S._check_pad(pad)
    for pad in (3, (1, 2, 3), None):
        with pytest.raises(TypeError):
            S._check_pad(pad)
    for iv in ([[5, 3]], [[0, 10], [5, 20]], [[0.5, 2.0]], [1, 2, 3]):
        with pytest.raises(ValueError):
            S._intervals(iv, 16000)
    with pytest.raises(ValueError):
        S.reference_labels([[0, 10]], -1)
    with pytest.raises(ValueError):
        S.reference_labels([[0, 10]], 5, hop=0)
