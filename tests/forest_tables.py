"""Forests and inputs of the forest- and score-variant tests
(test_forest_tables_cpu.py, test_gpu_forest_variants.py): plain NumPy, no
device.

A forest here is forest_reference.py's dict of arrays (feature, threshold,
left, right, leaf, nan_left, roots, proba; child indices absolute) with
n_features and K beside them.  Trees come from forest_reference.random_tree /
chain_tree and tree_tables.pad_table; their thresholds are then fitted to the
feature rows they will be walked with (fit_tree), so that every tree splits
the test windows.  What the GPU tests rely on -- the grouping of every named
size list, windows reaching more than one leaf of every tree, NaN met at nodes
of either flag, deep walks beside one-node trees -- is asserted on the
reference alone in test_forest_tables_cpu.py.

staging_groups() restates how forest_window_kernel (csrc/forest_kernel.hip)
stages a forest.  It only chooses and documents the inputs: no kernel result
is compared with it."""
import os
import re

import numpy as np

import forest_reference as FR
import tree_tables as T

LDS_NODES = T.LDS_NODES  # forest_kernel.hip kLdsNodes: the largest tree staged in LDS
NODE_BYTES = 16          # a compact node (TreeNodeC)
WIN = 256                # windows per block iteration (kTreeWin)


def _max_mfcc():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(here, "include", "vad_amd.h")) as f:
        return int(re.search(r"^#define\s+VAD_MAX_MFCC\s+(\d+)", f.read(), re.M).group(1))


MAX_MFCC = _max_mfcc()


# ---------------------------------------------------------------------------
# the staging rule
# ---------------------------------------------------------------------------
def row_nodes(mfcc_n):
    """R: the bytes of a chunk's MFCC rows (256 + 4 rows of 13 floats at width
    13, of VAD_MAX_MFCC floats at every other width, rounded up to 16 bytes)
    in compact nodes.
      width 13:     260 * 13 * 4 = 13,520 bytes = 845 nodes
      other widths: 260 * 16 * 4 = 16,640 bytes = 1,040 nodes"""
    row_bytes = (WIN + 4) * (13 if mfcc_n == 13 else MAX_MFCC) * 4
    return ((row_bytes + 15) & ~15) // NODE_BYTES


def buf_nodes(sizes, mfcc_n):
    """launch_forest_windows' buffer with VAD_FOREST_DUAL on: max(2 M, R)
    nodes, M the largest tree of at most LDS_NODES nodes (0: none)."""
    M = max([s for s in sizes if s <= LDS_NODES], default=0)
    return max(2 * M, row_nodes(mfcc_n))


def staging_groups(sizes, mfcc_n):
    """The groups forest_window_kernel walks a forest of these tree sizes in:
    ("lds", [tree indices]) for consecutive trees staged together -- walked
    in pairs from the group's first tree, an odd count leaving a single-tree
    tail -- or ("global", t) for a tree of more than LDS_NODES nodes."""
    B = buf_nodes(sizes, mfcc_n)
    groups, t, n = [], 0, len(sizes)
    while t < n:
        if sizes[t] > B or sizes[t] > LDS_NODES:
            groups.append(("global", t))
            t += 1
            continue
        te, total = t + 1, sizes[t]
        while te < n and sizes[te] <= LDS_NODES and total + sizes[te] <= B:
            total += sizes[te]
            te += 1
        groups.append(("lds", list(range(t, te))))
        t = te
    return groups


def pairs(groups):
    """The (a, b) tree pairs walk_pair gets, in order."""
    return [(g[i], g[i + 1]) for kind, g in groups if kind == "lds" for i in range(0, len(g) - 1, 2)]


# ---------------------------------------------------------------------------
# named size lists
# ---------------------------------------------------------------------------
CHAIN = LDS_NODES - 1  # 3071: the deepest tree LDS holds (1,535 internal nodes on one spine)
NAMES = ("many_small", "exact_fit", "exact_fit_pairs", "global_mix", "all_global", "deep_pairs", "one", "two", "three")
STAGING_WIDTHS = (13, 16)


def size_list(name, mfcc_n):
    """Tree sizes of a named forest at width 13 or 16.  A binary tree has an
    odd node count: an even size is the tree of one node less with a leaf no
    node points to appended (tree_tables.pad_table).  The grouping each list
    is meant to produce is asserted in test_forest_tables_cpu.py."""
    assert mfcc_n in STAGING_WIDTHS
    if name == "many_small":
        # 140 trees (141 at width 16: an odd last group) of 7 .. 31 nodes, about 2,700 nodes: M <= 31, so the
        # buffer is R and a group holds dozens
        n = 140 if mfcc_n == 13 else 141
        return (7 + 2 * np.random.default_rng(100 + mfcc_n).integers(0, 13, n)).tolist()
    if name == "exact_fit":
        # the buffer is R (2 M < R); a group of exactly R nodes, then one that a 3-node tree would overfill by one
        if mfcc_n == 13:
            return [401, 401, 43, 401, 401, 41, 3, 9]      # 845 | 843 (+ 3 = 846) | 12
        return [501, 501, 35, 3, 501, 501, 31, 5, 3, 9]    # 1,040 | 1,038 (+ 3 = 1,041) | 12
    if name == "exact_fit_pairs":
        # the buffer is 2 M = 2,002: two largest trees fill it; then 2,000 nodes and a 3-node tree one too many
        return [1001, 1001, 1001, 999, 3, 5]
    if name == "global_mix":
        # M = 3,072, the buffer 6,144: global first, in the middle and last; (1, 3072) and (3072, 1) are pairs
        return [3073, 1, 3072, 15, 4001, 3072, 1, 31, 3073]
    if name == "all_global":
        return [3073, 3501]  # M = 0: the buffer is R, nothing is staged
    if name == "deep_pairs":
        # chains of 3,071 nodes beside one- and three-node trees, either first; the 3,073-node trees end the groups
        return [CHAIN, 1, 3073, 1, CHAIN, 3073, CHAIN, 3, 3073, 3, CHAIN]
    return {"one": [63], "two": [63, 31], "three": [63, 31, 127]}[name]


MIXED = [63, 1, 255, 3073, 31, 3, 127]   # the variant matrix: pairs, a global tree, a tail, a one-node tree
CHUNK = [255, 511, 3073, 127, 511, 63]   # the chunk loop: two LDS groups around a global tree


# ---------------------------------------------------------------------------
# trees and forests
# ---------------------------------------------------------------------------
def fit_tree(tree, X):
    """The tree with every internal node's threshold moved to the median
    (float64, NaN ignored) of its feature over the rows of X that reach the
    node -- the midpoint of two rows' values or a row's own value, a tie; a
    node no finite value reaches takes the column's median (0 for an all-NaN
    column).  Structure, features and flags stay."""
    X = np.asarray(X, np.float32)
    out = dict(tree)
    thr = out["threshold"] = np.array(tree["threshold"], np.float64)
    col = {}
    stack = [(0, np.arange(len(X)))]
    while stack:
        i, rows = stack.pop()
        f = int(tree["feature"][i])
        if f < 0:
            continue
        v = X[rows, f].astype(np.float64)
        med = T._nanmedian(v)
        if med is None:
            if f not in col:
                col[f] = T._nanmedian(X[:, f].astype(np.float64)) or 0.0
            med = col[f]
        thr[i] = med
        with np.errstate(invalid="ignore"):
            go_left = np.where(np.isnan(v), tree["nan_left"][i] != 0, v <= med)
        stack.append((int(tree["right"][i]), rows[~go_left]))
        stack.append((int(tree["left"][i]), rows[go_left]))
    return out


def spread_chain(tree, X):
    """A chain_tree with its rising thresholds spread evenly between the
    smallest and the largest finite value of its feature in X: the rows leave
    the spine all along it."""
    out = dict(tree)
    spine = np.flatnonzero(tree["feature"] >= 0)
    v = np.asarray(X, np.float32)[:, int(tree["feature"][0])].astype(np.float64)
    v = v[np.isfinite(v)]
    thr = out["threshold"] = np.array(tree["threshold"], np.float64)
    thr[spine] = np.linspace(v.min(), v.max(), len(spine) + 2)[1:-1]
    return out


def pad_tree(tree, n_nodes, K, seed):
    """tree_tables.pad_table for a tree with proba rows: unreferenced leaves
    appended up to n_nodes, their shares random."""
    extra = n_nodes - len(tree["feature"])
    out = T.pad_table(dict(tree, classes=np.arange(K)), n_nodes)
    del out["classes"]
    p = np.random.default_rng(seed).random((extra, K))
    out["proba"] = np.concatenate([tree["proba"], p / p.sum(axis=1)[:, None]])
    return out


def build_tree(n_nodes, X, K, seed, chain_feature=None):
    """One tree of exactly n_nodes nodes over the columns of X: a chain on
    chain_feature (spread_chain), else a random tree fitted to X (fit_tree);
    an even n_nodes by padding."""
    F = np.asarray(X).shape[1]
    odd = n_nodes if n_nodes % 2 else n_nodes - 1
    if chain_feature is not None:
        t = spread_chain(FR.chain_tree(odd, K, chain_feature, seed), X)
    else:
        t = fit_tree(FR.random_tree(odd, F, K, seed), X)
    return t if odd == n_nodes else pad_tree(t, n_nodes, K, seed)


def forest_of(trees, n_features, K):
    """The trees one after another, child indices absolute, as the fields of
    vad_amd.forest.ForestClassifier.  K = 1: the shares of a tree always are
    1.0, which no sum could get wrong, so the rows are replaced by arbitrary
    positive values (the kernel and the reference add whatever the table
    holds)."""
    cols = {k: [] for k in ("feature", "threshold", "left", "right", "leaf", "nan_left", "proba")}
    roots, at = [], 0
    for t in trees:
        inner = t["left"] >= 0
        roots.append(at)
        for k in ("feature", "threshold", "leaf", "nan_left", "proba"):
            cols[k].append(t[k])
        cols["left"].append(np.where(inner, t["left"] + at, -1).astype(np.int32))
        cols["right"].append(np.where(inner, t["right"] + at, -1).astype(np.int32))
        at += len(t["feature"])
    f = {k: np.concatenate(v) for k, v in cols.items()}
    if K == 1:
        f["proba"] = np.random.default_rng(at).random((at, 1)) + 0.25
    assert f["proba"].shape == (at, K)
    f.update(roots=np.asarray(roots, np.int32), n_features=int(n_features), K=int(K))
    return f


def sizes_of(f):
    return np.diff(np.append(f["roots"], len(f["feature"]))).tolist()


def chain_features(mfcc_n):
    """What the chains of deep_pairs split on, in turn: D1 of coefficient 0
    (finite in either mode) and Mn of coefficient 0 (NaN in a flat window)."""
    return (mfcc_n, 0)


def build_forest(sizes, X, K=2, seed=0, chains=False):
    """A forest of these tree sizes over the columns of X.  chains: the trees
    of CHAIN nodes are chain trees on chain_features() in turn."""
    X = np.asarray(X, np.float32)
    cf = chain_features(X.shape[1] // 3)
    trees, n_chains = [], 0
    for i, n in enumerate(sizes):
        feature = None
        if chains and n == CHAIN:
            feature = cf[n_chains % len(cf)]
            n_chains += 1
        trees.append(build_tree(n, X, K, seed + i, feature))
    f = forest_of(trees, X.shape[1], K)
    assert sizes_of(f) == list(sizes)
    return f


def named_forest(name, X, K=2):
    mfcc_n = np.asarray(X).shape[1] // 3
    return build_forest(size_list(name, mfcc_n), X, K, seed=1000 * NAMES.index(name) + mfcc_n,
                        chains=name == "deep_pairs")


# ---------------------------------------------------------------------------
# what makes a wrong kernel visible
# ---------------------------------------------------------------------------
def tree_view(f, t):
    """Tree t as tree_tables' single-tree table (child indices relative)."""
    lo = int(f["roots"][t])
    hi = int(f["roots"][t + 1]) if t + 1 < len(f["roots"]) else len(f["feature"])
    inner = f["left"][lo:hi] >= 0
    return dict(feature=f["feature"][lo:hi], threshold=f["threshold"][lo:hi],
                left=np.where(inner, f["left"][lo:hi] - lo, -1), right=np.where(inner, f["right"][lo:hi] - lo, -1),
                leaf=f["leaf"][lo:hi], nan_left=f["nan_left"][lo:hi], classes=np.arange(f["K"]),
                n_features=f["n_features"])


def leaves_per_tree(f, X):
    """How many different leaves the rows of X end in, per tree."""
    return [len(set(row.tolist())) for row in FR.leaves(f, X)]


def nan_flags_met(f, X):
    """The nan_left values of the nodes at which some row of X met a NaN."""
    flags = set()
    for t in range(len(f["roots"])):
        tv = tree_view(f, t)
        flags |= {int(tv["nan_left"][n]) for _, n in T.nan_nodes(tv, X)}
    return flags


def walk_depths(f, t, X):
    """Edges on every row's path through tree t."""
    tv = tree_view(f, t)
    X = np.asarray(X, np.float32)
    node = np.zeros(len(X), np.int64)
    depth = np.zeros(len(X), np.int64)
    rows = np.arange(len(X))
    for _ in range(len(tv["feature"])):
        feat = tv["feature"][node]
        inner = feat >= 0
        if not inner.any():
            break
        v = X[rows, np.maximum(feat, 0)].astype(np.float64)
        with np.errstate(invalid="ignore"):
            left = np.where(np.isnan(v), tv["nan_left"][node] != 0, v <= tv["threshold"][node])
        node = np.where(inner, np.where(left, tv["left"][node], tv["right"][node]), node)
        depth += inner
    return depth


def tree_scores(proba, active):
    """vad_amd.h's definition of a tree's node score (TreeClassifier
    .score_table): the share of class `active` among the node's values,
    value / value.sum() in float64 (a zero sum taken as 1), rounded once to
    float32."""
    v = np.asarray(proba, np.float64)
    norm = v.sum(axis=1)
    norm[norm == 0.0] = 1.0
    return (v[:, active] / norm).astype(np.float32)


def table_proba(table, seed):
    """Node values for a table of tree_tables.py (which has none): random
    positive rows that do not sum to 1, one per node, unreferenced padding
    included."""
    return np.random.default_rng(seed).random((len(table["feature"]), len(table["classes"]))) + 0.05


def as_forest(table, proba):
    """A tree_tables table as a one-tree forest of forest_reference.py."""
    return dict(feature=table["feature"], threshold=table["threshold"], left=table["left"], right=table["right"],
                leaf=table["leaf"], nan_left=table["nan_left"], roots=np.zeros(1, np.int32), proba=proba)
