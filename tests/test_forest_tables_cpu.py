"""The forests of forest_tables.py against the staging model and the numpy
reference alone: the groupings and the conditions test_gpu_forest_variants.py
relies on hold before a kernel is involved.  Features are the oracle's,
rounded to float32 as the device stores them (test_tree_tables_cpu.py)."""
import functools

import numpy as np
import pytest

import forest_reference as FR
import forest_tables as FT
import tree_tables as T
from test_tree_tables_cpu import features

MODES = ("analyser", "offline")
RUNS = tuple(range(20, 300, 40))  # flat windows all along the 300 test windows


@functools.lru_cache(maxsize=None)
def rows_300(mfcc_n, mode):
    return features(T.mfcc_like_rows(5 + 300, mfcc_n, seed=mfcc_n, runs=RUNS), mode)


# ---------------------------------------------------------------------------
# the staging model
# ---------------------------------------------------------------------------
def test_buffer_arithmetic():
    assert FT.MAX_MFCC == 16
    assert FT.row_nodes(13) == 260 * 13 * 4 // 16 == 845
    assert FT.row_nodes(16) == FT.row_nodes(12) == FT.row_nodes(1) == 260 * 16 * 4 // 16 == 1040
    assert FT.buf_nodes([7, 31], 13) == 845 and FT.buf_nodes([7, 31], 16) == 1040
    assert FT.buf_nodes([423, 5000], 13) == 846 and FT.buf_nodes([521], 16) == 1042
    assert FT.buf_nodes([3072, 3073], 13) == 6144 and FT.buf_nodes([3073, 9999], 13) == 845


def test_staging_of_the_older_lists():
    """test_gpu_forest.py's size lists: no group of more than four trees."""
    G = FT.staging_groups
    assert G([31, 1, 201, 7], 13) == [("lds", [0, 1, 2, 3])]
    assert G([15, 3101, 9], 13) == [("lds", [0]), ("global", 1), ("lds", [2])]
    assert G([3071, 3073, 5, 3071], 13) == [("lds", [0]), ("global", 1), ("lds", [2, 3])]
    assert G([41, 9, 77, 3, 51], 13) == [("lds", [0, 1, 2, 3, 4])]
    assert G([1], 16) == [("lds", [0])]


def lds_groups(groups):
    return [g for kind, g in groups if kind == "lds"]


def nodes_in(sizes, group):
    return sum(sizes[t] for t in group)


@pytest.mark.parametrize("mfcc_n", FT.STAGING_WIDTHS)
def test_named_lists_group_as_intended(mfcc_n):
    R = FT.row_nodes(mfcc_n)
    sizes = {name: FT.size_list(name, mfcc_n) for name in FT.NAMES}
    groups = {name: FT.staging_groups(s, mfcc_n) for name, s in sizes.items()}
    for name in FT.NAMES:  # every tree once, in order
        flat = [t for kind, g in groups[name] for t in (g if kind == "lds" else [g])]
        assert flat == list(range(len(sizes[name]))), name

    s, g = sizes["many_small"], groups["many_small"]
    assert len(s) >= 100 and min(s) >= 7 and max(s) <= 31 and sum(s) > R and all(n % 2 for n in s)
    assert FT.buf_nodes(s, mfcc_n) == R and all(kind == "lds" for kind, _ in g) and len(g) >= 3
    counts = [len(x) for x in lds_groups(g)]
    print("many_small", mfcc_n, "trees per group", counts)
    assert any(c % 2 and c >= 3 for c in counts) and any(c % 2 == 0 for c in counts) and max(counts) >= 24
    assert all(nodes_in(s, x) <= R for x in lds_groups(g))

    for name in ("exact_fit", "exact_fit_pairs"):
        s, g = sizes[name], lds_groups(groups[name])
        B = FT.buf_nodes(s, mfcc_n)
        assert B == (R if name == "exact_fit" else 2 * 1001) and len(g) == 3 == len(groups[name])
        assert nodes_in(s, g[0]) == B                       # exactly full
        assert nodes_in(s, g[1]) + s[g[2][0]] == B + 1      # one node too many: the tree starts a group
        assert max(s) <= FT.LDS_NODES

    s, g = sizes["global_mix"], groups["global_mix"]
    assert {3072, 3073}.issubset(s) and max(s) > 3073 and FT.buf_nodes(s, mfcc_n) == 2 * 3072
    kinds = [kind for kind, _ in g]
    assert kinds == ["global", "lds", "global", "lds", "global"]
    assert [x for kind, x in g if kind == "global"] == [0, 4, len(s) - 1]
    sized = [(s[a], s[b]) for a, b in FT.pairs(g)]
    assert (1, 3072) in sized and (3072, 1) in sized
    assert all(len(x) % 2 for x in lds_groups(g))  # each group ends in a single-tree tail

    s, g = sizes["all_global"], groups["all_global"]
    assert len(s) == 2 and min(s) > FT.LDS_NODES and FT.buf_nodes(s, mfcc_n) == R
    assert g == [("global", 0), ("global", 1)]

    s, g = sizes["deep_pairs"], groups["deep_pairs"]
    assert FT.CHAIN == 3071 and FT.buf_nodes(s, mfcc_n) == 2 * 3071
    sized = [(s[a], s[b]) for a, b in FT.pairs(g)]
    assert sized == [(3071, 1), (1, 3071), (3071, 3), (3, 3071)]
    assert all(len(x) == 2 for x in lds_groups(g))

    for name, n in (("one", 1), ("two", 2), ("three", 3)):
        assert len(sizes[name]) == n and groups[name] == [("lds", list(range(n)))]

    for s in (FT.MIXED, FT.CHUNK):
        g = FT.staging_groups(s, mfcc_n)
        assert len(lds_groups(g)) >= 2 and sum(kind == "global" for kind, _ in g) == 1 and len(s) <= 7
    assert len(FT.CHUNK) <= 6
    assert [len(x) for x in lds_groups(FT.staging_groups(FT.MIXED, mfcc_n))] == [3, 3]  # a pair and a tail, twice


# ---------------------------------------------------------------------------
# the builders
# ---------------------------------------------------------------------------
def test_builders_keep_structure_and_sizes():
    X = rows_300(13, "analyser")
    raw = FR.random_tree(63, 39, 3, seed=5)
    fit = FT.fit_tree(raw, X)
    for k in ("feature", "left", "right", "nan_left", "proba"):
        assert np.array_equal(fit[k], raw[k]), k
    root = X[:, raw["feature"][0]].astype(np.float64)
    assert fit["threshold"][0] == np.median(root[~np.isnan(root)])
    padded = FT.pad_tree(fit, 70, 3, seed=1)
    assert len(padded["feature"]) == 70 == len(padded["proba"]) and (padded["feature"][63:] == -1).all()
    assert np.array_equal(padded["proba"][:63], fit["proba"])
    f1, f2 = FT.forest_of([fit], 39, 3), FT.forest_of([padded], 39, 3)
    assert np.array_equal(FR.predict_proba(f1, X), FR.predict_proba(f2, X))
    # a forest's trees keep their own walks: the leaves of tree t are tree t's, moved by its root
    f = FT.build_forest([15, 1, 3072, 31], X, K=2, seed=3)
    assert FT.sizes_of(f) == [15, 1, 3072, 31] and f["roots"].tolist() == [0, 15, 16, 3088]
    lv = FR.leaves(f, X)
    for t in range(4):
        tv = FT.tree_view(f, t)
        alone = FR.leaves(FT.as_forest(tv, f["proba"][:len(tv["feature"])]), X)[0]
        assert np.array_equal(lv[t], alone + f["roots"][t]), t
    chain = FT.spread_chain(FR.chain_tree(FT.CHAIN, 2, 13, seed=0), X)
    spine = chain["threshold"][chain["feature"] >= 0]
    assert len(spine) == 1535 and (np.diff(spine) > 0).all()
    assert X[:, 13].min() < spine[0] and spine[-1] < X[:, 13].max()
    k1 = FT.build_forest([7, 1, 15], X, K=1, seed=2)
    assert k1["proba"].shape == (23, 1) and len(set(k1["proba"][:, 0].tolist())) == 23


# ---------------------------------------------------------------------------
# what makes a wrong kernel visible
# ---------------------------------------------------------------------------
def check_visible(f, X, mode, nan=True):
    sizes = FT.sizes_of(f)
    reached = FT.leaves_per_tree(f, X)
    for t, (n, r) in enumerate(zip(sizes, reached)):
        assert r >= 2 or n == 1, (t, n, r)
    if f["K"] > 1:
        assert len(set(FR.predict_index(f, X).tolist())) >= 2
    assert len(set(FR.scores(f, X, f["K"] - 1).view(np.uint32).tolist())) >= min(len(X), 8) // 2
    if mode == "analyser" and nan:
        assert np.isnan(X).any() and FT.nan_flags_met(f, X) == {0, 1}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mfcc_n", FT.STAGING_WIDTHS)
@pytest.mark.parametrize("name", FT.NAMES)
def test_named_forests_are_visible(name, mfcc_n, mode):
    X = rows_300(mfcc_n, mode)
    assert X.shape == (300, 3 * mfcc_n)
    f = FT.named_forest(name, X)
    assert FT.sizes_of(f) == FT.size_list(name, mfcc_n)
    check_visible(f, X, mode)
    if name == "deep_pairs":
        chains = [t for t, n in enumerate(FT.sizes_of(f)) if n == FT.CHAIN]
        assert len(chains) == 4
        for t in chains:
            d = FT.walk_depths(f, t, X)
            assert (d > 1000).sum() >= 20 and (d < 500).sum() >= 20 and len(set(d.tolist())) > 100, t
        assert {int(f["feature"][f["roots"][t]]) for t in chains} == set(FT.chain_features(mfcc_n))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mfcc_n", T.WIDTHS)
def test_mixed_forest_is_visible(mfcc_n, mode):
    """The forest of the variant matrix, every width and class count."""
    X = features(T.mfcc_like_rows(5 + 1000, mfcc_n, seed=mfcc_n), mode)
    for K in (1, 2, 3, 8) if mfcc_n == 13 else (2, 3):
        f = FT.build_forest(FT.MIXED, X, K, seed=10 * mfcc_n + K)
        assert f["n_features"] == 3 * mfcc_n and f["proba"].shape[1] == K
        check_visible(f, X, mode)
        for W in T.WINDOWS[1:]:  # the shorter inputs are other rows: the trees still split them
            Xw = features(T.mfcc_like_rows(5 + W, mfcc_n, seed=mfcc_n), mode)
            check_visible(f, Xw, mode, nan=False)


def test_tree_scores_restate_score_table():
    v = np.array([[3.0, 1.0], [0.0, 0.0], [0.25, 0.75], [1e-3, 7.0]])
    s = FT.tree_scores(v, 1)
    assert s.dtype == np.float32
    assert s.tolist() == [np.float32(0.25), 0.0, np.float32(0.75), np.float32(7.0 / 7.001)]
    X = rows_300(13, "offline")
    table = T.bushy_table(39, 4, X, seed=1)
    p = FT.table_proba(table, seed=2)
    assert p.shape == (31, 4) and (np.abs(p.sum(axis=1) - 1) > 1e-6).any()
    leaf = FR.leaves(FT.as_forest(table, p), X)[0]
    assert (table["feature"][leaf] < 0).all() and len(set(leaf.tolist())) >= 8
    assert len(set(FT.tree_scores(p, 3)[leaf].tolist())) >= 8
