"""The score stage on the host: the NumPy models (tests/scores_reference.py)
against brute force, roc / threshold_at on hand-made histograms, and
TreeClassifier.score_table against sklearn's predict_proba."""
import numpy as np
import pytest

import scores_reference as R


def rand_scores(rng, n):
    s = rng.random(n).astype(np.float32)
    s[rng.random(n) < 0.05] = np.nan
    s[rng.random(n) < 0.05] = 0.0
    s[rng.random(n) < 0.05] = 1.0
    return s


@pytest.mark.parametrize("seed", range(6))
def test_hysteresis_model_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(0, 200))
    s = rand_scores(rng, n)
    for on, off in ((0.7, 0.3), (0.5, 0.5), (1.0, 0.0), (0.0, 0.0)):
        want = np.zeros(n, np.uint8)
        for i in range(n):
            for j in range(i, -1, -1):  # the last decided window at or before i
                if s[j] >= np.float32(on):
                    want[i] = 1
                    break
                if not s[j] >= np.float32(off):
                    break
        assert np.array_equal(R.hysteresis(s, on, off), want), (on, off)


@pytest.mark.parametrize("seed", range(6))
def test_dilate_model_against_brute_force(seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(0, 120))
    lab = (rng.random(n) < 0.1).astype(np.uint8) * 3
    for pb, pa in ((0, 0), (1, 0), (0, 1), (2, 5), (n + 5, 0), (0, n + 5)):
        want = np.array([any(lab[j] == 3 for j in range(max(i - pa, 0), min(i + pb, n - 1) + 1)) for i in range(n)],
                        dtype=np.uint8).reshape(n)
        assert np.array_equal(R.dilate(lab, 3, pb, pa), want), (pb, pa)
    assert np.array_equal(R.dilate(lab, 3, 0, 0), (lab == 3).astype(np.uint8))


def test_per_clip_model_keeps_clips_apart():
    lab = np.array([9, 0, 0, 1, 0, 1, 0, 0, 1, 9], np.uint8)  # windows 0 and 9 belong to no clip
    got = R.per_clip(lambda x: R.dilate(x, 1, 1, 2), lab, [1, 4, 7], [3, 0, 2])
    assert got.tolist() == [0, 0, 1, 1, 0, 0, 0, 1, 1, 0]
    s = np.array([.9, .5, .5, .1, .5, .9, .5], np.float32)
    assert R.per_clip(lambda x: R.hysteresis(x, .7, .3), s, [0, 2], [2, 5]).tolist() == [1, 1, 0, 0, 0, 1, 1]


@pytest.mark.parametrize("seed", range(4))
def test_reference_labels_model_against_brute_force(seed):
    rng = np.random.default_rng(200 + seed)
    fs, hop, n = 400, 160, 90
    cuts = np.sort(rng.choice(np.arange(0, (n + 4) * hop), size=8, replace=False))
    iv = cuts.reshape(-1, 2)
    want = np.zeros(n, np.uint8)
    for i in range(n):
        c = (i + 2) * hop + fs // 2
        want[i] = any(s <= c < e for s, e in iv)
    assert np.array_equal(R.reference_labels(iv, n, fs, hop), want)
    assert not R.reference_labels(np.zeros((0, 2), np.int64), n, fs, hop).any()


def test_histogram_model():
    s = np.array([0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), 0.5, np.nan, 0.24999, 0.25, -0.5],
                 np.float32)
    ref = np.array([0, 1, 1, 0, 1, 0, 0, 7], np.uint8)
    assert R.score_bins(s, 4).tolist() == [0, 3, 3, 2, 0, 0, 1, 0]
    h = R.histogram(s, ref, 4)
    assert h.tolist() == [[2, 1, 1, 0], [1, 0, 0, 2]]  # the window with ref 7 is not counted
    assert R.confusion(np.array([0, 1, 1, 2, 5], np.uint8), np.array([0, 0, 1, 1, 1], np.uint8), 3).tolist() == \
        [[1, 1, 0], [0, 1, 1]]


def test_roc_and_threshold_on_hand_made_histograms():
    from vad_amd.scores import roc_from_histogram, threshold_at
    h = np.array([[50, 30, 15, 5], [2, 8, 30, 60]], np.int64)
    roc = roc_from_histogram(h)
    assert roc.thresholds.tolist() == [0, .25, .5, .75, 1]
    assert np.allclose(roc.fpr, [1, .5, .2, .05, 0]) and np.allclose(roc.tpr, [1, .98, .9, .6, 0])
    assert (roc.tpr[0], roc.fpr[0]) == (1, 1) and (roc.tpr[-1], roc.fpr[-1]) == (0, 0)
    assert (np.diff(roc.tpr) <= 0).all() and (np.diff(roc.fpr) <= 0).all()
    for bound, want in ((1.0, 0.0), (0.5, .25), (0.49, .5), (0.2, .5), (0.05, .75), (0.04, 1.0), (0.0, 1.0)):
        t = threshold_at(roc, bound)
        assert t == want, bound
        assert roc.fpr[list(roc.thresholds).index(t)] <= bound
    # random histograms: monotone, the end points, the bound kept and the threshold the lowest that keeps it
    rng = np.random.default_rng(5)
    for bins in (2, 7, 1024):
        h = rng.integers(0, 50, size=(2, bins))
        roc = roc_from_histogram(h)
        assert len(roc.thresholds) == bins + 1
        assert (np.diff(roc.tpr) <= 0).all() and (np.diff(roc.fpr) <= 0).all()
        assert (roc.tpr[0], roc.fpr[0], roc.tpr[-1], roc.fpr[-1]) == (1, 1, 0, 0)
        for bound in (0.0, 0.01, 0.3, 1.0):
            k = list(roc.thresholds).index(threshold_at(roc, bound))
            assert roc.fpr[k] <= bound and (k == 0 or roc.fpr[k - 1] > bound)
    # a class with no windows: its rate is 0 throughout, nothing divides by zero
    roc = roc_from_histogram(np.array([[0, 0], [3, 1]]))
    assert roc.fpr.tolist() == [0, 0, 0] and roc.tpr.tolist() == [1, .25, 0]
    with pytest.raises(ValueError):
        roc_from_histogram(np.zeros((3, 4)))
    with pytest.raises(ValueError):
        threshold_at(roc, 1.5)


def fitted_tree(weighted=False):
    from sklearn.tree import DecisionTreeClassifier
    rng = np.random.default_rng(11)
    x = rng.standard_normal((600, 5)).astype(np.float32)
    y = ((x[:, 0] + 0.5 * x[:, 1] + 0.8 * rng.standard_normal(600)) > 0).astype(np.int64) + (x[:, 2] > 1.2)
    clf = DecisionTreeClassifier(max_depth=6, min_samples_leaf=7, random_state=0)
    clf.fit(x, y, sample_weight=rng.random(600) + 0.1 if weighted else None)
    return clf, x


@pytest.mark.parametrize("weighted", [False, True])
def test_score_table_is_predict_proba(weighted, tmp_path):
    """Bit for bit after the one rounding to float32, for every class, at the
    leaf sklearn itself puts each row in."""
    from vad_amd.tree import TreeClassifier
    clf, x = fitted_tree(weighted)
    tree = TreeClassifier.from_sklearn(clf)
    assert tree.proba is not None and tree.proba.dtype == np.float64
    assert tree.proba.shape == (clf.tree_.node_count, 3)
    leaves = clf.apply(x)
    proba = clf.predict_proba(x)
    for active in range(3):
        table = tree.score_table(active)
        assert table.dtype == np.float32 and table.shape == (clf.tree_.node_count,)
        assert np.array_equal(table[leaves].view(np.uint32), proba[:, active].astype(np.float32).view(np.uint32))
    # the optional key survives save / load; a tree without it loads as before
    p = tmp_path / "t.npz"
    tree.save(p)
    back = TreeClassifier.load(p)
    assert np.array_equal(back.proba, tree.proba) and np.array_equal(back.score_table(1), tree.score_table(1))
    tree.proba = None
    tree.save(p)
    with np.load(p) as z:
        assert "proba" not in z.files
    assert TreeClassifier.load(p).proba is None


def test_score_table_from_counts_and_errors():
    from vad_amd.tree import TreeClassifier
    args = dict(feature=[0, -1, -1], threshold=[0.5, 0, 0], left=[1, -1, -1], right=[2, -1, -1], leaf=[0, 0, 1],
                nan_left=[0, 0, 0], classes=[0, 1], n_features=1)
    tree = TreeClassifier(**args, value=[[5, 3], [4, 0], [0, 0]])  # a zero row: its sum is taken as 1
    assert tree.score_table(1).tolist() == [np.float32(3 / 8), 0.0, 0.0]
    assert tree.score_table(0).tolist() == [np.float32(5 / 8), 1.0, 0.0]
    with pytest.raises(ValueError):
        tree.score_table(2)
    with pytest.raises(ValueError):
        tree.score_table(-1)
    with pytest.raises(ValueError, match="neither"):
        TreeClassifier(**args).score_table(1)
