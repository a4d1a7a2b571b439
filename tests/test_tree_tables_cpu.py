"""The table builders of tree_tables.py against the oracle's tree_predict
alone: the conditions test_gpu_tree_variants.py relies on hold before a
kernel is involved.  Features are the oracle's, rounded to float32 as the
device stores them."""
import numpy as np
import pytest

from oracle import vad_oracle as O

import tree_tables as T

MODES = ("analyser", "offline")


def features(m, mode):
    x = O.analyser_features_fast(m) if mode == "analyser" else O.offline_features(m).reshape(len(m) - 5, -1)
    return x.astype(np.float32)


def _case(mfcc_n, mode):
    X = features(T.mfcc_like_rows(5 + 1000, mfcc_n, seed=mfcc_n), mode)
    return X, T.variant_tables(X, mfcc_n)


def test_pad_table_leaves_the_walk_unchanged():
    X, (tables, _) = _case(13, "analyser")
    want = O.tree_predict(tables["bushy"], X)
    for n in (len(tables["bushy"]["feature"]), 512, T.LDS_NODES, T.LDS_NODES + 1):
        padded = T.pad_table(tables["bushy"], n)
        assert len(padded["feature"]) == n == len(padded["nan_left"]) == len(padded["leaf"])
        assert np.array_equal(O.tree_predict(padded, X), want)
    one = dict(feature=np.array([-1], np.int32), threshold=np.zeros(1), left=np.array([-1], np.int32),
               right=np.array([-1], np.int32), leaf=np.array([3], np.int32), nan_left=np.zeros(1, np.uint8),
               classes=np.arange(4), n_features=39)
    assert (O.tree_predict(T.pad_table(one, T.LDS_NODES + 1), X) == 3).all()


def test_bushy_table_shape():
    X = features(T.mfcc_like_rows(405, 13, seed=2), "offline")
    for depth in (1, 3, 10):
        t = T.bushy_table(39, depth, X, seed=depth)
        n_int = 2 ** depth - 1
        inner = t["feature"] >= 0
        assert len(inner) == 2 * n_int + 1 and inner.sum() == n_int
        assert t["feature"].max() < 39
        assert np.array_equal(t["nan_left"][inner], np.flatnonzero(inner) % 2)
        assert np.array_equal(t["leaf"][~inner], np.arange(n_int + 1) % 4)
        kids = np.concatenate([t["left"][inner], t["right"][inner]])
        assert np.array_equal(np.sort(kids), np.arange(1, len(inner)))  # every node but the root has one parent
        assert (t["left"][inner] == np.flatnonzero(inner) + 1).all()
    # the root's threshold is its column's median
    t = T.bushy_table(39, 1, X, seed=0)
    col = X[:, t["feature"][0]].astype(np.float64)
    assert t["threshold"][0] == np.median(col)
    assert np.array_equal(O.tree_predict(t, X) == 0, col <= np.median(col))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mfcc_n", T.WIDTHS)
def test_variant_tables_reach_classes_and_nan_nodes(mfcc_n, mode):
    X, (tables, depth) = _case(mfcc_n, mode)
    for name in ("bushy", "bushy_3072", "bushy_3073", "bushy_narrow"):
        t = tables[name]
        lab = O.tree_predict(t, X[:, :t["n_features"]])
        assert len(set(lab.tolist())) >= 3, name
        if mode == "analyser":
            met = T.nan_nodes(t, X)
            assert len({r for r, _ in met}) >= 20, name
            flags = {int(t["nan_left"][n]) for _, n in met}
            assert flags == {0, 1}, name
    assert tables["bushy_narrow"]["n_features"] == T.narrow_features(mfcc_n) < 3 * mfcc_n
    assert np.array_equal(O.tree_predict(tables["bushy_3072"], X), O.tree_predict(tables["bushy"], X))
    for n in (T.LDS_NODES, T.LDS_NODES + 1):
        t, d = tables[f"comb_{n}"], depth[f"comb_{n}"]
        assert len(t["feature"]) == n
        assert len(set(d.tolist())) > len(X) // 4 and d.max() > n // 4
        assert len(set(O.tree_predict(t, X).tolist())) == 2


@pytest.mark.parametrize("name", ["edge", "tie"])
def test_edge_ladder_reaches_its_leaves(name):
    thr = T.EDGE_THRESHOLDS if name == "edge" else T.TIE_THRESHOLDS
    assert len(thr) <= 255 and (np.diff(thr) > 0).all()
    if name == "edge":
        assert len(thr) == 255  # classes up to 255
        for v in (0.0, 5e-324, -5e-324, 1e-50, -1e-50, 1e300, -1e300, -np.inf, float(T.F32.max),
                  float(np.nextafter(float(T.F32.max), np.inf)), float(T.DENORM_MIN), float(T.DENORM_MAX)):
            assert v in thr
    x = T.edge_inputs(thr)
    assert np.isnan(x).sum() == 1 and len(np.unique(x.view(np.uint32))) == len(x)
    for nan_down in (False, True):
        t = T.ladder_table(thr, 0, 1, nan_down=nan_down)
        lab = O.tree_predict(t, x[:, None])
        assert lab[np.isnan(x)][0] == (len(thr) if nan_down else 0)
        fin = ~np.isnan(x)
        reached = set(lab[fin].tolist())
        assert 0 in reached and len(thr) in reached
        print(name, "leaves reached", len(reached), "of", len(thr) + 1)
        assert len(reached) >= 0.9 * (len(thr) + 1)
        # the label names the interval: inputs either side of a threshold never share one
        xv, lv = x[fin].astype(np.float64), lab[fin]
        assert np.array_equal(lv, np.searchsorted(thr, xv, side="left"))
        for k, th in enumerate(thr):
            below, above = lv[xv <= th], lv[xv > th]
            assert (below <= k).all() and (above > k).all()
    if name == "edge":  # the float denormals stand apart from +-0 on either side
        idx = {float(v): int(l) for v, l in zip(x[fin], lab[fin])}
        d = float(T.DENORM_MIN)
        assert idx[-d] < idx[0.0] < idx[d] and idx[0.0] == int(np.searchsorted(thr, 0.0))


def test_round_f32_brackets_the_double():
    thr = T.EDGE_THRESHOLDS
    up, down = T.round_f32(thr, True), T.round_f32(thr, False)
    assert (down.astype(np.float64) <= thr).all() and (up.astype(np.float64) >= thr).all()
    exact = down == up
    assert exact.any() and not exact.all()
    with np.errstate(over="ignore"):
        assert np.array_equal(np.nextafter(down[~exact], np.float32(np.inf)), up[~exact])


def test_mfcc_like_rows_have_flat_windows():
    for n in T.WIDTHS:
        m = T.mfcc_like_rows(1005, n, seed=n, runs=(990,))
        assert m.shape == (1005, n) and m.dtype == np.float32
        assert (m[990:998] == m[990]).all()
        x = features(m, "analyser")
        flat = np.isnan(x[:, 0])
        assert flat.sum() >= 20 and flat[990:994].all()
        assert np.isfinite(x[:, n:2 * n]).all()  # D1: what the combs split on
