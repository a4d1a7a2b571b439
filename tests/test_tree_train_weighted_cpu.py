"""Weighted tree training without a GPU: the numpy model of the weighted rule
(tests/tree_train_weighted_reference.py) against sklearn's
``fit(X, y, sample_weight=w)`` node by node, the second rule (distinct rows
count for min_samples_leaf), prune, the forest draws, the integer class
weights, the argument checks and the exported symbols."""
import os
import re

import numpy as np
import pytest

import tree_train_reference as R
import tree_train_weighted_reference as W

CONFIGS = ("w13", "w7q", "w5", "w9")
KINDS = ("boot", "class", "both")
STATES = (0, 1, 2, 3)


def _config(g, name):
    K, md, mss, msl = (int(v) for v in g[f"{name}_params"])
    return g[f"{name}_x"], g[f"{name}_y"], K, md, mss, msl


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", CONFIGS)
def test_rule_allows_every_sklearn_node_fixture(golden, name, kind):
    g = golden("tree_train_weighted")
    x, y, K, md, mss, msl = _config(g, name)
    w = g[f"{name}_{kind}_w"]
    assert w.dtype == np.uint8 and w.max() > 1
    if kind != "class":
        assert (w == 0).any()
    ties = 0
    for rs in STATES:
        pre = f"{name}_{kind}_rs{rs}_"
        nodes, splits, t = W.check_tree_nodewise(x, y, w, K, md, mss, msl, g[pre + "left"], g[pre + "right"],
                                                 g[pre + "feature"], g[pre + "threshold"], g[pre + "n_node_samples"],
                                                 g[pre + "missing_go_to_left"], g[pre + "weighted_n_node_samples"],
                                                 g[pre + "value"])
        print(f"{name} {kind} random_state {rs}: {nodes} nodes, {splits} splits, {t} with a tie between features")
        ties += t
    if name == "w7q":
        assert ties > 0  # the fixture does exercise the tie rule


def test_fixture_covers_what_it_should(golden):
    g = golden("tree_train_weighted")
    params = [tuple(int(v) for v in g[f"{n}_params"]) for n in CONFIGS]
    assert {p[0] for p in params} == {2, 3}
    assert {p[3] for p in params} == {1, 5, 20}
    assert min(p[1] for p in params) <= 6
    assert all(len(g[f"{n}_y"]) <= 3000 for n in CONFIGS)


@pytest.mark.parametrize("name", CONFIGS)
def test_rule_allows_every_sklearn_node_live(golden, name):
    tree = pytest.importorskip("sklearn.tree")
    g = golden("tree_train_weighted")
    x, y, K, md, mss, msl = _config(g, name)
    w = g[f"{name}_both_w"]
    t = tree.DecisionTreeClassifier(max_depth=md, min_samples_split=mss, min_samples_leaf=msl,
                                    random_state=0).fit(x, y, sample_weight=w.astype(np.float64)).tree_
    pre = f"{name}_both_rs0_"
    assert np.array_equal(t.feature, g[pre + "feature"])  # the fixture is what this sklearn gives
    W.check_tree_nodewise(x, y, w, K, md, mss, msl, t.children_left, t.children_right, t.feature, t.threshold,
                          t.n_node_samples, t.missing_go_to_left, t.weighted_n_node_samples, t.value[:, 0, :])


@pytest.mark.parametrize("name", ("w7q", "w13"))
def test_model_tree_is_one_sklearn_could_build(golden, name):
    """The model's own weighted tree passes the node-wise check (lowest
    feature, lowest p is one of the allowed choices), is in preorder, keeps
    weighted counts in value and distinct rows in n_node_samples."""
    g = golden("tree_train_weighted")
    x, y, K, md, mss, msl = _config(g, name)
    w = g[f"{name}_both_w"].astype(np.int64)
    t = W.fit(x, y, w, K, md, mss, msl)
    W.check_tree_nodewise(x, y, w, K, md, mss, msl, t["left"], t["right"], t["feature"], t["threshold"],
                          t["n_node_samples"], t["nan_left"])
    inner = t["left"] >= 0
    assert np.array_equal(t["left"][inner], np.flatnonzero(inner) + 1)
    assert t["value"][0].sum() == w.sum() and t["n_node_samples"][0] == (w > 0).sum()
    assert (t["value"].sum(axis=1) > t["n_node_samples"]).any()
    v = t["value"].sum(axis=1)
    assert (v[t["left"][inner]] + v[t["right"][inner]] == v[inner]).all()
    n = t["n_node_samples"]
    assert (n[t["left"][inner]] + n[t["right"][inner]] == n[inner]).all()
    assert (t["leaf"] == t["value"].argmax(axis=1)).all()
    leaves = ~inner
    assert inner.any() and (n[leaves] >= msl).all()


@pytest.mark.parametrize("n,F,K,seed,p", [(900, 7, 3, 11, (25, 10, 5)), (700, 5, 2, 12, (25, 2, 1)),
                                          (1200, 13, 5, 13, (6, 22, 20))])
def test_weights_of_ones_are_the_unweighted_model(n, F, K, seed, p):
    x, y = R.synth(n, F, K, seed)
    a = W.fit(x, y, np.ones(n, np.int64), K, *p)
    assert R.tables_equal(a, R.fit(x, y, K, *p)) is None
    assert R.tables_equal(W.fit(x, y, None, K, *p), a) is None
    # 0 / 1 weights are the rows subset
    keep = np.random.default_rng(seed).random(n) < 0.6
    assert R.tables_equal(W.fit(x, y, keep.astype(np.int64), K, *p), R.fit(x, y, K, *p, rows=np.flatnonzero(keep))) is None


def test_scaling_all_weights_keeps_the_splits():
    x, y = R.synth(800, 7, 3, 21)
    w = W.weights_of("both", y, 3, 5)
    a, b = W.fit(x, y, w, 3, 25, 10, 5), W.fit(x, y, 4 * w, 3, 25, 10, 5)
    for k in ("feature", "left", "right", "leaf", "n_node_samples"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(4 * a["value"], b["value"])


def test_min_samples_leaf_counts_distinct_rows():
    """The second rule: a row of weight 3 is one row for min_samples_leaf (and
    min_samples_split), three rows when it is repeated three times."""
    x = np.array([[0.0], [1.0], [2.0], [3.0]], np.float32)
    y = np.array([0, 0, 1, 1])
    w = np.array([3, 3, 3, 3])
    weighted = W.fit(x, y, w, 2, 5, 2, 3)
    repeated = R.fit(np.repeat(x, w, axis=0), np.repeat(y, w), 2, 5, 2, 3)
    assert len(weighted["feature"]) == 1 and weighted["n_node_samples"][0] == 4
    assert np.array_equal(weighted["value"], [[6, 6]])
    assert len(repeated["feature"]) == 3 and repeated["threshold"][0] == 1.5
    assert np.array_equal(repeated["value"][0], weighted["value"][0])
    # with min_samples_leaf 1 the two agree in everything but the row counts
    a, b = W.fit(x, y, w, 2, 5, 2, 1), R.fit(np.repeat(x, w, axis=0), np.repeat(y, w), 2, 5, 2, 1)
    for k in ("feature", "threshold", "left", "right", "leaf", "value"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["n_node_samples"], [4, 2, 2]) and np.array_equal(b["n_node_samples"], [12, 6, 6])
    tree = pytest.importorskip("sklearn.tree")
    s = tree.DecisionTreeClassifier(max_depth=5, min_samples_leaf=3).fit(x, y, sample_weight=w.astype(float)).tree_
    assert s.node_count == 1 and s.n_node_samples[0] == 4 and s.weighted_n_node_samples[0] == 12.0
    s = tree.DecisionTreeClassifier(max_depth=5, min_samples_leaf=3).fit(np.repeat(x, w, axis=0), np.repeat(y, w)).tree_
    assert s.node_count == 3


def test_a_weight_can_make_an_impure_looking_node_pure_only_by_weight_zero():
    """Purity is max c == W on weighted counts: rows of weight 0 are absent."""
    x = np.arange(6, dtype=np.float32).reshape(-1, 1)
    y = np.array([0, 1, 0, 1, 0, 1])
    t = W.fit(x, y, np.array([2, 0, 5, 0, 1, 0]), 2, 5, 2, 1)
    assert len(t["feature"]) == 1 and np.array_equal(t["value"], [[8, 0]]) and t["n_node_samples"][0] == 3


@pytest.mark.parametrize("md", [3, 10, 25])
@pytest.mark.parametrize("mss", [7, 22])
def test_prune_equals_direct_weighted_fit(md, mss):
    from vad_amd.tree_train import prune_table
    x, y = R.synth(1500, 7, 3, 7)
    w = W.weights_of("both", y, 3, 8)
    big = W.fit(x, y, w, 3, 25, 2, 3)
    assert big["depth"].max() > 10
    assert R.tables_equal(prune_table(big, md, mss), W.fit(x, y, w, 3, md, mss, 3)) is None


def test_forest_draws_bootstrap_sequence():
    from vad_amd.tree_train import forest_draws
    n, F, T = 50, 9, 5
    for ms, m in ((1.0, 50), (0.5, 25), (7, 7)):
        draws = forest_draws(n, F, T, ms, "sqrt", seed=3, bootstrap=True)
        again = forest_draws(n, F, T, ms, "sqrt", seed=3, bootstrap=True)
        rng = np.random.default_rng(3)
        for (c, f), (c2, f2) in zip(draws, again):
            want_c = np.bincount(rng.integers(0, n, m), minlength=n)
            want_f = np.sort(rng.choice(F, 3, replace=False))
            assert c.shape == (n,) and c.sum() == m and np.array_equal(c, want_c) and np.array_equal(f, want_f)
            assert np.array_equal(c, c2) and np.array_equal(f, f2)
    other = forest_draws(n, F, T, 1.0, "sqrt", seed=4, bootstrap=True)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(forest_draws(n, F, T, 1.0, "sqrt", 3, True), other))
    # all features: the feature draw is still made (the sequence does not depend on k) and reported as None
    d = forest_draws(n, F, 2, 1.0, None, seed=3, bootstrap=True)
    rng = np.random.default_rng(3)
    for c, f in d:
        assert np.array_equal(c, np.bincount(rng.integers(0, n, n), minlength=n)) and f is None
        rng.choice(F, F, replace=False)


def test_forest_draws_without_bootstrap_are_unchanged():
    from vad_amd.tree_train import forest_draws
    n, F, T = 40, 10, 4
    for ms, m in ((0.5, 20), (1.0, 40)):
        rng = np.random.default_rng(9)
        for kw in ({}, {"bootstrap": False}):
            got = forest_draws(n, F, T, ms, 0.5, seed=9, **kw)
            rng = np.random.default_rng(9)
            for r, f in got:
                want_r = np.sort(rng.choice(n, m, replace=False))
                want_f = np.sort(rng.choice(F, 5, replace=False))
                assert (r is None and m == n) or np.array_equal(r, want_r)
                assert np.array_equal(f, want_f)
    # pinned values: the sequence of seed 0 as it has always been
    r, f = forest_draws(10, 4, 1, 0.5, 2, seed=0)[0]
    rng = np.random.default_rng(0)
    assert np.array_equal(r, np.sort(rng.choice(10, 5, replace=False)))
    assert np.array_equal(f, np.sort(rng.choice(4, 2, replace=False)))


def test_balanced_integer_weights_values():
    from vad_amd.tree_train import balanced_integer_weights
    y = np.array([0] * 90 + [1] * 30 + [2] * 7)
    assert balanced_integer_weights(y) == {0: 1, 1: 3, 2: 13}             # 90/30 = 3, 90/7 = 12.86
    assert balanced_integer_weights(y, max_weight=8) == {0: 1, 1: 3, 2: 8}
    assert balanced_integer_weights(np.array([5, 5, 7, 7])) == {5: 1, 7: 1}
    big = balanced_integer_weights(np.array([-1] * 1000 + [4]))
    assert big == {-1: 1, 4: 255}                                         # clipped at 255
    assert balanced_integer_weights(np.array([1] * 5 + [0] * 2)) == {0: 2, 1: 1}   # 2.5 rounds to even
    assert all(type(k) is int and type(v) is int for k, v in big.items())
    for bad in (0, 256):
        with pytest.raises(ValueError):
            balanced_integer_weights(y, max_weight=bad)
    # sklearn's "balanced" weights are in the same proportions up to the rounding
    cw = balanced_integer_weights(y)
    bal = len(y) / (3 * np.bincount(y))
    assert np.allclose(np.array([cw[k] for k in (0, 1, 2)]) / cw[0], bal / bal[0], rtol=0.05)


def test_row_weights_product():
    from vad_amd.tree_train import check_job_weights, row_weights
    y = np.array([3, 9, 9, 3, 9])
    classes = np.array([3, 9])
    assert row_weights(y, classes) is None
    assert np.array_equal(row_weights(y, classes, [1, 0, 2, 3, 1], None), [1, 0, 2, 3, 1])
    assert np.array_equal(row_weights(y, classes, None, {3: 2, 9: 5}), [2, 5, 5, 2, 5])
    assert np.array_equal(row_weights(y, classes, np.array([1, 0, 2, 3, 1], np.uint8), {9: 5, 3: 2}), [2, 0, 10, 6, 5])
    got = check_job_weights(np.array([2, 0, 10, 6, 255]), 5)
    assert got.dtype == np.uint8 and np.array_equal(got, [2, 0, 10, 6, 255])


def test_value_errors_before_the_device():
    from vad_amd.tree_train import TreeTrainer
    x, y = R.synth(50, 5, 2, 1)
    tr = TreeTrainer(5, 2, 1)
    ok = np.ones(50, np.int64)
    bad_sw = [ok.astype(np.float64), ok.astype(np.float32) * 0.5, -ok, ok[:-1], np.stack([ok, ok]), 0 * ok,
              ok * 256, ok > 0]
    for sw in bad_sw:
        with pytest.raises(ValueError):
            tr.fit(x, y, sample_weight=sw)
        with pytest.raises(ValueError):
            tr.grid(x, y, [3], [2], [1], [(np.arange(25), np.arange(25, 50))], sample_weight=sw)
    neg = ok.copy()
    neg[7] = -1
    with pytest.raises(ValueError):
        tr.fit(x, y, sample_weight=neg)
    with pytest.raises(ValueError, match="balanced_integer_weights"):
        tr.fit(x, y, class_weight="balanced")
    with pytest.raises(ValueError, match="balanced_integer_weights"):
        tr.fit_forest(x, y, 2, class_weight="balanced")
    for cw in ({0: 1}, {0: 1, 1: 2, 2: 3}, {0: 1, 2: 1}, {0: 1.5, 1: 1}, {0: 2.0, 1: 1}, {0: 0, 1: 1}, {0: -2, 1: 1},
               {0: True, 1: 1}, {0: 256, 1: 1}, [1, 2], 3):
        with pytest.raises(ValueError):
            tr.fit(x, y, class_weight=cw)
        with pytest.raises(ValueError):
            tr.fit_forest(x, y, 2, class_weight=cw)
    with pytest.raises(ValueError):
        tr.fit(x, y, sample_weight=ok * 100, class_weight={0: 3, 1: 1})   # a row above 255
    # a total above 2^26 (rows at most 255 each): refused on the host, nothing is launched
    n = (1 << 26) // 255 + 2
    with pytest.raises(ValueError, match="2\\^26"):
        tr.fit(np.zeros((n, 1), np.float32), np.arange(n) % 2, sample_weight=np.full(n, 255))
    # fit_many jobs
    with pytest.raises(ValueError):
        tr.fit_many(x, y, [([1, 2, 3], 3, 2, 1, None, ok)])               # rows with weights
    for w in (ok.astype(np.float64), -ok, ok[:-1], 0 * ok, ok * 256):
        with pytest.raises(ValueError):
            tr.fit_many(x, y, [(None, 3, 2, 1, None, w)])
    with pytest.raises(ValueError):
        tr.fit_many(x, y, [(None, 3, 2, 1, None, ok, 0)])                 # seven elements
    with pytest.raises(ValueError):
        tr.fit_forest(x, y, 2, bootstrap=True, max_samples=0.0)
    # the class values, not their indices, are the keys
    with pytest.raises(ValueError):
        tr.fit(x, np.array([-3, 8])[y], class_weight={0: 1, 1: 2})


def test_header_and_library_export_the_weighted_entry():
    from vad_amd import _lib
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "include", "vad_amd.h")) as f:
        header = f.read()
    lib = _lib.lib()
    for name in ("vad_tree_train_weighted", "vad_tree_train_weighted_workspace_bytes"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert re.search(r"const uint8_t\* weights", header)
    assert "VAD_TREE_TRAIN_MAX_WEIGHT (1 << 26)" in header
    assert len(_lib.SIGNATURES["vad_tree_train_weighted"][1]) == len(_lib.SIGNATURES["vad_tree_train_features"][1])


def test_weighted_entry_refuses_bad_arguments_before_any_launch():
    """VAD_EINVAL for a NULL required pointer, a job of 0 rows and NULL weights
    with a job that does not take every row: host checks, no device needed."""
    import ctypes

    from vad_amd import _lib
    from vad_amd.tree_train import _Job, _Tables
    lib = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 255) & ~255
    tb = _Tables(*([base] * 11))

    def call(jobs, x=base, y=base, order=base, weights=base, tables=True, ws=base, nbytes=1 << 40, n=100):
        arr = (_Job * len(jobs))(*[_Job(*j) for j in jobs])
        return lib.vad_tree_train_weighted(x, y, n, 4, 2, order, weights, None, len(jobs), arr,
                                           ctypes.byref(tb) if tables else None, ws, nbytes, None, None)

    good = (100, 199, 5, 2, 1, 0)
    for kw in (dict(x=None), dict(y=None), dict(order=None), dict(tables=False), dict(ws=None)):
        assert call([good], **kw) == _lib.VAD_EINVAL, kw
    assert call([(0, 199, 5, 2, 1, 0)]) == _lib.VAD_EINVAL            # a job of 0 rows
    assert call([(101, 199, 5, 2, 1, 0)]) == _lib.VAD_EINVAL          # more rows than there are
    assert call([(60, 199, 5, 2, 1, 0)], weights=None) == _lib.VAD_EINVAL  # all ones, but n_rows != n
    assert call([good], nbytes=64) == _lib.VAD_EINVAL                 # workspace too small
    arr = (_Job * 1)(_Job(*good))
    need = lib.vad_tree_train_weighted_workspace_bytes(100, 4, 2, 1, arr)
    assert need >= lib.vad_tree_train_workspace_bytes(100, 4, 2, 1, arr) > 0
    arr0 = (_Job * 1)(_Job(0, 199, 5, 2, 1, 0))
    assert lib.vad_tree_train_weighted_workspace_bytes(100, 4, 2, 1, arr0) == 0
