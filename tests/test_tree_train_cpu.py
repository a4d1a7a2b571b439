"""Tree training without a GPU: the numpy model of the rule
(tests/tree_train_reference.py) against sklearn node by node, prune against
direct fits, kfold, the argument checks and the exported symbols.

sklearn breaks exact score ties between features by its random feature
order, so whole trees differ between random states; every node of every
sklearn tree must still be a choice the rule allows, with the rule's
threshold and missing_go_to_left for that choice bit for bit."""
import os
import re

import numpy as np
import pytest

import tree_train_reference as R

CONFIGS = ("a39", "b13", "c7q", "d5")
STATES = (0, 1, 2, 3)


def check_tree_nodewise(x, y, K, md, mss, msl, left, right, feature, thr, n_node, mgl):
    """Walk an sklearn tree; at every node compare with the rule on the rows
    that reach the node.  Returns (nodes, nodes with a tie between features)."""
    rows = {0: np.arange(len(x))}
    depth = {0: 0}
    ties = 0
    for i in range(len(left)):  # preorder: a parent comes before its children
        r = rows.pop(i)
        n = len(r)
        assert n == n_node[i], (i, n, n_node[i])
        counts = np.bincount(y[r], minlength=K)
        leaf = R.is_leaf(n, counts, depth[i], md, mss, msl)
        sc = None
        if not leaf:
            sc, xs, order = R.scores(x[r], y[r].astype(np.int64), K, msl)
            leaf = sc.max() < 0
        if left[i] < 0:
            assert leaf, f"node {i}: sklearn made a leaf, the rule splits"
            continue
        assert not leaf, f"node {i}: sklearn split, the rule makes a leaf"
        f = int(feature[i])
        goes_left = x[r, f].astype(np.float64) <= thr[i]
        p = int(goes_left.sum())
        assert 1 <= p < n
        m = sc.max()
        assert sc[p - 1, f].tobytes() == m.tobytes(), (i, f, p, sc[p - 1, f], m)
        assert int(np.argmax(sc[:, f] == m)) == p - 1, f"node {i}: not the first maximum of feature {f}"
        ties += int((sc.max(axis=0) == m).sum() > 1)
        t = R.threshold(xs[p - 1, f], xs[p, f])
        assert np.float64(t).tobytes() == np.float64(thr[i]).tobytes(), (i, t, thr[i])
        assert bool(mgl[i]) == (p > n - p), i
        # the rows by position in the sorted list are the rows by the threshold
        assert np.array_equal(np.sort(order[:p, f]), np.flatnonzero(goes_left))
        rows[int(left[i])], rows[int(right[i])] = r[goes_left], r[~goes_left]
        depth[int(left[i])] = depth[int(right[i])] = depth[i] + 1
    return len(left), ties


@pytest.mark.parametrize("name", CONFIGS)
def test_rule_allows_every_sklearn_node_fixture(golden, name):
    g = golden("tree_train")
    x, y = g[f"{name}_x"], g[f"{name}_y"]
    K, md, mss, msl = (int(v) for v in g[f"{name}_params"])
    assert np.unique(x[:, -1]).size == 1 and np.unique(x[:, -2]).size > 1 and np.ptp(x[:, -2]) < 1e-6
    total_ties = 0
    for rs in STATES:
        pre = f"{name}_rs{rs}_"
        nodes, ties = check_tree_nodewise(x, y, K, md, mss, msl, g[pre + "left"], g[pre + "right"], g[pre + "feature"],
                                          g[pre + "threshold"], g[pre + "n_node_samples"],
                                          g[pre + "missing_go_to_left"])
        print(f"{name} random_state {rs}: {nodes} nodes, {ties} with a score tie between features")
        total_ties += ties
    if name in ("c7q", "a39"):
        assert total_ties > 0  # the fixture does exercise the tie rule


@pytest.mark.parametrize("name", CONFIGS)
def test_rule_allows_every_sklearn_node_live(golden, name):
    tree = pytest.importorskip("sklearn.tree")
    g = golden("tree_train")
    x, y = g[f"{name}_x"], g[f"{name}_y"]
    K, md, mss, msl = (int(v) for v in g[f"{name}_params"])
    for rs in (4, 5):
        t = tree.DecisionTreeClassifier(max_depth=md, min_samples_split=mss, min_samples_leaf=msl,
                                        random_state=rs).fit(x, y).tree_
        check_tree_nodewise(x, y, K, md, mss, msl, t.children_left, t.children_right, t.feature, t.threshold,
                            t.n_node_samples, t.missing_go_to_left)


def test_model_tree_is_one_sklearn_could_build(golden):
    """The model's own tree passes the same node-wise check (lowest feature,
    lowest p is one of the allowed choices), is numbered in preorder, and
    classifies its training rows as its leaves say."""
    g = golden("tree_train")
    x, y = g["c7q_x"], g["c7q_y"]
    K, md, mss, msl = (int(v) for v in g["c7q_params"])
    t = R.fit(x, y, K, md, mss, msl)
    check_tree_nodewise(x, y, K, md, mss, msl, t["left"], t["right"], t["feature"], t["threshold"],
                        t["n_node_samples"], t["nan_left"])
    inner = t["left"] >= 0
    assert np.array_equal(t["left"][inner], np.flatnonzero(inner) + 1)
    assert (t["value"].sum(axis=1) == t["n_node_samples"]).all()
    pred = R.walk(t, x)
    leaves = ~inner
    assert (pred == y).sum() == t["value"][leaves].max(axis=1).sum()


def test_near_equal_values_split_with_strict_greater():
    """0.5 + 2^-24 and 0.5 + 2^-23 are distinct float32 values less than 1e-7
    apart: the built sklearn 1.7.2 splits between them, and so does the rule."""
    x = np.repeat(np.array([0.5 + 2.0 ** -24, 0.5 + 2.0 ** -23], np.float32), 30).reshape(-1, 1)
    y = np.repeat([0, 1], 30)
    t = R.fit(x, y, 2, 5, 2, 1)
    assert len(t["feature"]) == 3 and t["feature"][0] == 0
    assert t["threshold"][0] == np.float64(x[0, 0]) / 2 + np.float64(x[-1, 0]) / 2
    tree = pytest.importorskip("sklearn.tree")
    s = tree.DecisionTreeClassifier(min_samples_leaf=1).fit(x, y).tree_
    assert s.node_count == 3 and s.threshold[0] == t["threshold"][0]


@pytest.mark.parametrize("md", [3, 10, 25])
@pytest.mark.parametrize("mss", [7, 22])
def test_prune_equals_direct_fit(md, mss):
    from vad_amd.tree_train import prune_table
    x, y = R.synth(1500, 7, 3, 7)
    big = R.fit(x, y, 3, 25, 2, 3)
    assert big["depth"].max() > 10
    assert R.tables_equal(prune_table(big, md, mss), R.fit(x, y, 3, md, mss, 3)) is None


def test_prune_unequal_children():
    """A root whose left child is a small leaf and whose right child is deep."""
    from vad_amd.tree_train import prune_table
    rng = np.random.default_rng(3)
    x = rng.standard_normal((600, 3)).astype(np.float32)
    y = (x[:, 1] > 0).astype(np.int64) ^ (x[:, 2] > 0.3)
    x[:40, 0] -= 10
    y[:40] = 2
    big = R.fit(x, y, 3, 30, 2, 1)
    assert big["n_node_samples"][big["left"][0]] == 40 and big["left"][big["left"][0]] == -1
    for md, mss in ((1, 2), (2, 2), (4, 50), (30, 41), (30, 2)):
        assert R.tables_equal(prune_table(big, md, mss), R.fit(x, y, 3, md, mss, 1)) is None, (md, mss)


def test_preorder_renumbering():
    """A level-ordered copy of a model table renumbers back to the table."""
    from vad_amd.tree_train import preorder
    x, y = R.synth(800, 5, 2, 9)
    t = R.fit(x, y, 2, 25, 2, 1)
    lvl = np.argsort(t["depth"], kind="stable")  # preorder within a depth = level order
    new = np.empty_like(lvl)
    new[lvl] = np.arange(len(lvl))
    s = {k: v[lvl].copy() for k, v in t.items()}
    for k in ("left", "right"):
        s[k][s[k] >= 0] = new[s[k][s[k] >= 0]]
    inner = s["left"] >= 0
    assert (s["right"][inner] == s["left"][inner] + 1).all()
    assert R.tables_equal(preorder(s), t) is None


@pytest.mark.parametrize("n,k", [(10, 3), (9, 3), (11, 2), (7, 7), (100, 6)])
def test_kfold_blocks(n, k):
    from vad_amd.tree_train import kfold
    folds = kfold(n, k)
    assert len(folds) == k
    assert np.array_equal(np.concatenate([t for _, t in folds]), np.arange(n))
    sizes = [len(t) for _, t in folds]
    assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)
    for tr, te in folds:
        assert np.array_equal(np.sort(np.concatenate([tr, te])), np.arange(n))
    try:
        from sklearn.model_selection import KFold
    except ImportError:
        return
    for (tr, te), (str_, ste) in zip(folds, KFold(k).split(np.zeros(n))):
        assert np.array_equal(tr, str_) and np.array_equal(te, ste)


def test_kfold_refuses():
    from vad_amd.tree_train import kfold
    for n, k in ((5, 1), (3, 4), (0, 2)):
        with pytest.raises(ValueError):
            kfold(n, k)


def test_value_errors_before_the_device():
    from vad_amd.tree_train import TreeTrainer, check_rows
    x, y = R.synth(50, 5, 2, 1)
    tr = TreeTrainer()
    assert (tr.max_depth, tr.min_samples_split, tr.min_samples_leaf) == (25, 22, 20)
    for bad in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[17, 3] = bad
        with pytest.raises(ValueError):
            tr.fit(xb, y)
    with pytest.raises(ValueError):
        tr.fit(x[:, 0], y)                          # not 2-D
    with pytest.raises(ValueError):
        tr.fit(x, y[:-1])                           # rows and labels differ
    with pytest.raises(ValueError):
        tr.fit(x, np.stack([y, y]))
    with pytest.raises(ValueError):
        tr.fit(np.zeros((50, 65), np.float32), y)   # more than 64 features
    with pytest.raises(ValueError):
        tr.fit(np.zeros((50, 0), np.float32), y)
    with pytest.raises(ValueError):
        tr.fit(x, np.arange(50) % 9)                # more than 8 classes
    with pytest.raises(ValueError):
        tr.fit_many(x, y, [([1, 2, 2], 3, 2, 1)])   # a row twice
    with pytest.raises(ValueError):
        tr.fit_many(x, y, [([1, 50], 3, 2, 1)])     # a row outside X
    for kw in (dict(max_depth=0), dict(min_samples_split=1), dict(min_samples_leaf=0)):
        with pytest.raises(ValueError):
            TreeTrainer(**kw)
    xc, yi, classes = check_rows(x.astype(np.float64), np.array([-3, 8])[y])
    assert xc.dtype == np.float32 and np.array_equal(classes, [-3, 8]) and np.array_equal(yi, y)


def test_old_tree_files_load_and_new_ones_round_trip(golden, tmp_path):
    from vad_amd.tree import TreeClassifier
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    old = TreeClassifier.load(os.path.join(repo, "tests", "golden", "tree.npz")) \
        if "n_features" in golden("tree").files else None
    if old is not None:
        assert old.n_node_samples is None and old.depth is None and old.value is None
    x, y = R.synth(300, 5, 2, 2)
    t = R.fit(x, y, 2, 4, 2, 5)
    clf = TreeClassifier(*(t[k] for k in R.KEYS[:6]), np.array([0, 1]), 5, n_node_samples=t["n_node_samples"],
                         depth=t["depth"], value=t["value"])
    clf.save(str(tmp_path / "t.npz"))
    back = TreeClassifier.load(str(tmp_path / "t.npz"))
    for k in R.KEYS:
        assert np.array_equal(getattr(back, k), t[k]), k
    plain = TreeClassifier(*(t[k] for k in R.KEYS[:6]), np.array([0, 1]), 5)
    plain.save(str(tmp_path / "p.npz"))
    with np.load(str(tmp_path / "p.npz")) as z:
        assert "depth" not in z.files
    assert TreeClassifier.load(str(tmp_path / "p.npz")).depth is None


def test_header_and_library_export_the_training_entries():
    from vad_amd import _lib
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "include", "vad_amd.h")) as f:
        header = f.read()
    lib = _lib.lib()
    for name in ("vad_tree_train_workspace_bytes", "vad_tree_train_node_capacity", "vad_tree_train"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.vad_tree_train_node_capacity(1000, 20) == 99
    assert lib.vad_tree_train_node_capacity(1000, 1) == 1999
    assert lib.vad_tree_train_node_capacity(5, 20) == 1
