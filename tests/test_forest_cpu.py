"""The forest without a GPU: the conversion from sklearn against the fixture
(tests/golden/forest.npz), the numpy restatement of the definition against
sklearn's own predict_proba (bit for bit), save / load, fit_forest's documented
draws, and the arguments the new C entries and fit_many refuse before any HIP
call (the device pointers below are never dereferenced)."""
import ctypes
import os
import sys

import numpy as np
import pytest

import forest_reference as FR

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

E, EUNSUP = -1, -2
N = None
NAMES = ("rf", "bag", "rf3")


def fixture_forest(g, name):
    return {k: g[f"{name}_{k}"] for k in FR.KEYS}


@pytest.mark.parametrize("name", NAMES)
def test_from_sklearn_reproduces_the_fixture(golden, name):
    import gen_forest
    from vad_amd.forest import ForestClassifier
    g = golden("forest")
    clf = gen_forest.fitted(name)
    f = ForestClassifier.from_sklearn(clf)
    want = fixture_forest(g, name)
    for k, v in FR.table(f).items():
        assert v.dtype == want[k].dtype and v.tobytes() == want[k].tobytes(), k
    assert np.array_equal(f.classes_, g[f"{name}_classes"])
    assert f.n_features == 39 and f.n_trees == len(clf.estimators_)
    if name == "bag":  # features mapped back to the columns of the full row
        feats = g["bag_estimators_features"]
        assert np.array_equal(feats, np.stack(clf.estimators_features_))
        for t, est in enumerate(clf.estimators_):
            lo = f.roots[t]
            local = est.tree_.feature
            inner = est.tree_.children_left >= 0
            assert np.array_equal(f.feature[lo:lo + len(local)][inner], feats[t][local[inner]])
        assert len(np.unique(f.feature[f.feature >= 0])) > feats.shape[1]  # more columns than one tree sees


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_sklearn_bit_for_bit(golden, name):
    g = golden("forest")
    f = fixture_forest(g, name)
    x = g[f"{name}_x_test"]
    assert np.isnan(x).any()
    p = FR.predict_proba(f, x)
    want = g[f"{name}_predict_proba"]
    assert p.dtype == want.dtype and p.tobytes() == want.tobytes()
    assert np.array_equal(g[f"{name}_classes"][FR.predict_index(f, x)], g[f"{name}_predict"])


def test_extra_trees_convert(golden):
    from sklearn.ensemble import ExtraTreesClassifier
    import gen_forest
    from vad_amd.forest import ForestClassifier
    x, y = gen_forest.rows(500, 2, seed=3)
    clf = ExtraTreesClassifier(n_estimators=3, max_depth=4, n_jobs=1, random_state=0).fit(x, y)
    f = ForestClassifier.from_sklearn(clf)
    xt = gen_forest.test_rows(2)
    p = FR.predict_proba(FR.table(f), xt)
    assert p.tobytes() == clf.predict_proba(xt).tobytes()
    with pytest.raises(TypeError):
        ForestClassifier.from_sklearn(clf.estimators_[0])


def test_save_load_round_trip(golden, tmp_path):
    from vad_amd.forest import ForestClassifier
    g = golden("forest")
    f = ForestClassifier(*(g[f"rf3_{k}"] for k in FR.KEYS), g["rf3_classes"], 39)
    path = str(tmp_path / "forest.npz")
    f.save(path)
    b = ForestClassifier.load(path)
    for k, v in FR.table(f).items():
        w = getattr(b, k)
        assert w.dtype == v.dtype and w.tobytes() == v.tobytes(), k
    assert np.array_equal(b.classes_, f.classes_) and b.n_features == 39 and b.n_trees == 6
    with np.load(path, allow_pickle=False) as z:  # arrays only
        assert "roots" in z.files


def test_from_trees_checks_and_layout():
    from vad_amd.forest import ForestClassifier
    from vad_amd.tree import TreeClassifier

    def tree(n, K=2, F=5, classes=None):
        t = FR.chain_tree(n, K)
        return TreeClassifier(t["feature"], t["threshold"], t["left"], t["right"], t["leaf"], t["nan_left"],
                              np.arange(K) if classes is None else classes, F, proba=t["proba"])

    f = ForestClassifier.from_trees([tree(5), tree(1), tree(3)])
    assert f.roots.tolist() == [0, 5, 6] and f.roots.dtype == np.int32
    assert f.left.tolist() == [1, -1, 3, -1, -1, -1, 7, -1, -1] and f.right.tolist() == [2, -1, 4, -1, -1, -1, 8, -1, -1]
    assert f.proba.shape == (9, 2) and f.proba.dtype == np.float64
    counts = TreeClassifier([-1], [-2.0], [-1], [-1], [1], [0], np.arange(2), 5, value=np.array([[1, 3]]))
    assert ForestClassifier.from_trees([counts]).proba.tolist() == [[0.25, 0.75]]
    with pytest.raises(ValueError):
        ForestClassifier.from_trees([])
    with pytest.raises(ValueError):
        ForestClassifier.from_trees([tree(3), tree(3, F=6)])
    with pytest.raises(ValueError):
        ForestClassifier.from_trees([tree(3), tree(3, classes=np.array([0, 2]))])
    with pytest.raises(ValueError):
        ForestClassifier.from_trees([TreeClassifier([-1], [-2.0], [-1], [-1], [0], [0], np.arange(2), 5)])


def test_fit_forest_draws_follow_the_recipe():
    from vad_amd.tree_train import forest_draws
    n, F, T = 1000, 39, 4
    draws = forest_draws(n, F, T, max_samples=0.5, max_features=0.5, seed=3)
    rng = np.random.default_rng(3)
    for rows, feats in draws:
        assert np.array_equal(rows, np.sort(rng.choice(n, 500, replace=False)))
        assert np.array_equal(feats, np.sort(rng.choice(F, 19, replace=False)))
    # "sqrt", integer counts, and everything reported as None (the draws are still made)
    rng = np.random.default_rng(0)
    for rows, feats in forest_draws(n, F, 3, max_samples=1.0, max_features="sqrt", seed=0):
        rng.choice(n, n, replace=False)
        assert rows is None and np.array_equal(feats, np.sort(rng.choice(F, 6, replace=False)))
    d = forest_draws(n, F, 2, max_samples=7, max_features=None, seed=1)
    assert all(len(r) == 7 and f is None for r, f in d)
    assert len(forest_draws(n, F, 1, max_features=3)[0][1]) == 3
    for kw in (dict(n_trees=0), dict(max_samples=0.0), dict(max_samples=1001), dict(max_features=40),
               dict(max_features="log2"), dict(max_features=1.5)):
        a = dict(n_trees=2)
        a.update(kw)
        with pytest.raises(ValueError):
            forest_draws(n, F, **a)


def test_fit_many_refuses_bad_features():
    from vad_amd.tree_train import TreeTrainer, feature_mask
    assert feature_mask(None, 5) is None and feature_mask([0, 3], 5) == 9 and feature_mask(np.arange(64), 64) == 2**64 - 1
    x = np.zeros((30, 5), np.float32)
    y = np.arange(30) % 2
    for feats in ([], [5], [-1], [1, 1], [0.5], [[0, 1]]):
        with pytest.raises(ValueError):
            TreeTrainer().fit_many(x, y, [(None, 3, 2, 1, feats)])
    with pytest.raises(ValueError):
        TreeTrainer().fit_many(x, y, [(None, 3, 2)])


# -- the C entries ---------------------------------------------------------------
X, Y, ORD, MASK, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x100000
TAB = [0x1000000 + 0x100000 * i for i in range(11)]


@pytest.fixture(scope="module")
def tt():
    from vad_amd import _lib, tree_train
    return _lib.lib(), tree_train


def test_tree_train_features_refuses(tt):
    lib, mod = tt

    def train(masks, F=5, J=2, **kw):
        jobs = (mod._Job * J)(*[mod._Job(100, 9, 5, 22, 20, 0) for _ in range(J)])
        a = dict(x=X, y=Y, order=ORD, ws=WS, ws_bytes=1 << 40)
        a.update(kw)
        tb = mod._Tables(*TAB)
        fm = None if masks is None else (ctypes.c_uint64 * J)(*masks)
        return lib.vad_tree_train_features(a["x"], a["y"], 100, F, 3, a["order"], MASK, fm, J, jobs, ctypes.byref(tb),
                                           a["ws"], a["ws_bytes"], None, N)

    assert train([1, 0]) == E  # a job with no feature
    assert train([1, 1 << 5]) == E  # only bits at or past n_features
    assert train([1, (1 << 64) - 32]) == E
    assert train([0] * 1, J=1) == E
    assert train([1 << 63, 1 << 62], F=63) == E
    # the checks of vad_tree_train hold with masks and without
    for masks in ([1, 3], None):
        for kw in (dict(x=N), dict(y=N), dict(order=N), dict(ws=N), dict(ws=WS + 8), dict(ws_bytes=1024)):
            assert train(masks, **kw) == E, (masks, kw)
        assert train(masks, F=65) == E and train(masks, F=0) == E


def test_forest_entries_refuse(tt):
    lib = tt[0]
    feat = np.array([0, -1, -1, 1, -1, -1], np.int32)
    thr = np.array([0.5, -2, -2, 0.25, -2, -2], np.float64)
    left = np.array([1, -1, -1, 4, -1, -1], np.int32)
    right = np.array([2, -1, -1, 5, -1, -1], np.int32)
    nl = np.zeros(6, np.uint8)
    roots = np.array([0, 3], np.int32)
    proba = np.full((6, 2), 0.5)

    def create(**kw):
        a = dict(n=6, feature=feat, threshold=thr, left=left, right=right, nan_left=nl, T=2, roots=roots, K=2,
                 proba=proba, F=2, out=True)
        a.update(kw)
        h = ctypes.c_void_p()
        p = {k: (None if a[k] is None else a[k].ctypes.data) for k in
             ("feature", "threshold", "left", "right", "nan_left", "roots", "proba")}
        rc = lib.vad_forest_create(a["n"], p["feature"], p["threshold"], p["left"], p["right"], p["nan_left"], a["T"],
                                   p["roots"], a["K"], p["proba"], a["F"], ctypes.byref(h) if a["out"] else None)
        return rc, h

    bad = [dict(feature=None), dict(threshold=None), dict(left=None), dict(right=None), dict(roots=None),
           dict(proba=None), dict(out=False), dict(n=0), dict(n=-1), dict(F=0), dict(T=0), dict(T=-1), dict(K=0),
           dict(K=9), dict(T=7),
           dict(roots=np.array([0, 6], np.int32)),   # a root outside the table
           dict(roots=np.array([0, -1], np.int32)),
           dict(roots=np.array([1, 3], np.int32)),   # the first tree starts the table
           dict(roots=np.array([0, 0], np.int32)),   # ascending
           dict(roots=np.array([0, 2], np.int32)),   # a child outside its tree
           dict(left=np.array([1, -1, -1, 3, -1, -1], np.int32)),  # a child that is its tree's root
           dict(right=np.array([6, -1, -1, 5, -1, -1], np.int32)),
           dict(feature=np.array([2, -1, -1, 1, -1, -1], np.int32))]  # a feature past the row
    for kw in bad:
        rc, h = create(**kw)
        assert rc == E and not h.value, kw
    assert create(F=65)[0] == EUNSUP
    A, B, C = 0x10000, 0x20000, 0x30000
    assert lib.vad_forest_predict(None, A, 10, 0, B, C, N) == E
    assert lib.vad_features_forest(None, A, 100, 13, 0, 0, B, C, N) == E
    assert lib.vad_forest_destroy(None) == 0
    rc, h = create()
    if rc != 0:  # the plan's tables are device memory: without a device there is no plan to hand in
        return
    try:
        assert lib.vad_forest_predict(h, A, 0, 0, B, C, N) == 0
        assert lib.vad_features_forest(h, A, 5, 13, 0, 0, B, C, N) == 0  # no window: nothing to do
        for args in ((A, -1, 0, B, C), (A, 10, 2, B, C), (A, 10, -1, B, C), (N, 10, 0, B, C), (A, 10, 0, N, C),
                     (A, 10, 0, B, B), (A, 10, 0, A, C), (A, 10, 0, B, A + 8)):
            assert lib.vad_forest_predict(h, *args, N) == E, args
        assert lib.vad_forest_predict(h, A, 0, 2, B, C, N) == E  # active is checked first
        for args in ((A, -1, 13, 0, 0, B, C), (A, 100, 0, 0, 0, B, C), (A, 100, 17, 0, 0, B, C),
                     (A, 100, 13, 2, 0, B, C), (A, 100, 13, 0, 2, B, C), (A, 100, 13, 0, -1, B, C),
                     (N, 100, 13, 0, 0, B, C), (A, 100, 13, 0, 0, N, C), (A, 100, 13, 0, 0, B, B),
                     (A, 100, 13, 0, 0, A + 16, C), (A, 100, 13, 0, 0, B, A)):
            assert lib.vad_features_forest(h, *args, N) == E, args
    finally:
        assert lib.vad_forest_destroy(h) == 0


def test_streams_and_analyser_refuse_a_forest(golden, tmp_path):
    from vad_amd.forest import ForestClassifier
    g = golden("forest")
    f = ForestClassifier(*(g[f"rf_{k}"] for k in FR.KEYS), g["rf_classes"], 39)
    path = str(tmp_path / "forest.npz")
    f.save(path)
    from vad_amd.dist import classify_clip_shard
    from vad_amd.sklearn_analyser import SKLearnAnalyzer
    from vad_amd.stream import StreamBatch
    with pytest.raises(ValueError, match="forest"):
        StreamBatch(4, f)
    with pytest.raises(ValueError, match="forest"):
        SKLearnAnalyzer(path)

    class Pipe:
        ffn = f
    with pytest.raises(ValueError, match="forest"):
        classify_clip_shard(Pipe(), None, None)
