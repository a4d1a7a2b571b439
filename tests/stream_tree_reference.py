"""Host-side helpers of the tree-in-the-stream tests (test_stream_tree_cpu.py,
test_gpu_stream_tree.py): the fixture tree as the oracle's dict, the margin of
a row's path through a tree, and a synthetic comb table of any node count.

Trees are the oracle's dicts (oracle.vad_oracle.tree_predict): feature (< 0:
leaf), threshold (float64), left, right, leaf (class index), nan_left, classes,
n_features."""
import os

import numpy as np

KEYS = ("feature", "threshold", "left", "right", "leaf", "nan_left", "classes")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture_tree():
    """tests/golden/tree.npz: 977 nodes, 39 features."""
    with np.load(os.path.join(GOLDEN, "tree.npz"), allow_pickle=False) as z:
        t = {k: z[k] for k in KEYS}
        t["n_features"] = int(z["n_features"])
    return t


def classifier(tree):
    from vad_amd.tree import TreeClassifier
    return TreeClassifier(*(tree[k] for k in KEYS), tree["n_features"])


def path_margin(tree, X):
    """Per row of X (n, n_features; compared as float32, as tree_predict
    does): the minimum, over the internal nodes its path visits, of
    |x[feature] - threshold| / max(1, |threshold|) -- how far the features may
    move before the row can take another branch.  A NaN feature follows the
    node's flag whatever its neighbours are: it does not bound the margin.  A
    path of no internal node (a one-leaf tree) has margin inf.  Also returns
    the depth (edges) of each path."""
    X = np.asarray(X, np.float32).reshape(-1, tree["n_features"])
    n = len(X)
    node = np.zeros(n, np.int64)
    rows = np.arange(n)
    margin = np.full(n, np.inf)
    depth = np.zeros(n, np.int64)
    for _ in range(len(tree["feature"])):
        f = tree["feature"][node]
        internal = f >= 0
        if not internal.any():
            break
        v = X[rows, np.maximum(f, 0)].astype(np.float64)
        thr = tree["threshold"][node]
        isnan = np.isnan(v)
        with np.errstate(invalid="ignore"):
            m = np.abs(v - thr) / np.maximum(1.0, np.abs(thr))
            go_left = np.where(isnan, tree["nan_left"][node] != 0, v <= thr)
        m = np.where(isnan | ~internal, np.inf, m)
        margin = np.minimum(margin, m)
        nxt = np.where(go_left, tree["left"][node], tree["right"][node])
        node = np.where(internal, nxt, node)
        depth += internal
    return margin, depth


def comb_table(n_nodes, X, cols):
    """A comb of exactly n_nodes nodes: spine node i (index 2 i) splits on
    feature cols[i % len(cols)]; its left child (2 i + 1) is a leaf of class
    i % 2, its right child the next spine node; the spine ends in a leaf of
    class D % 2 (D = (n_nodes - 1) // 2 spine nodes).  A binary tree has an
    odd number of nodes: an even n_nodes gets one more leaf at the end that no
    node points to.

    Thresholds come from the feature rows X (n, n_features; finite in `cols`)
    so that rows leave the spine all along it: most spine nodes sit below
    every row's value (all go right); at len(X) - 1 evenly spaced "exit" nodes
    the threshold is the midpoint between the smallest and the second smallest
    value still on the spine, so the rows holding the smallest go left there
    and the others go on, with a margin of half that gap on either side.
    Returns (tree dict, exit depth per row of X: the number of edges of its
    path)."""
    X = np.asarray(X, np.float32)
    R, F = X.shape
    D = (n_nodes - 1) // 2
    assert D >= 1 and n_nodes >= 3
    feature = np.full(n_nodes, -1, np.int32)
    threshold = np.zeros(n_nodes, np.float64)
    left = np.full(n_nodes, -1, np.int32)
    right = np.full(n_nodes, -1, np.int32)
    leaf = np.zeros(n_nodes, np.int32)
    spine = 2 * np.arange(D)
    feature[spine] = np.asarray(cols, np.int32)[np.arange(D) % len(cols)]
    left[spine] = spine + 1
    right[spine] = spine + 2
    leaf[spine + 1] = np.arange(D) % 2
    leaf[2 * D] = D % 2
    floor = X.min(axis=0).astype(np.float64) - 1.0
    threshold[spine] = floor[feature[spine]]
    depth = np.full(R, D, np.int64)  # rows that never leave: the spine's end
    remaining = np.arange(R)
    E = min(R - 1, D)
    for j in range(E):
        i = ((j + 1) * D) // (E + 1)
        f = feature[2 * i]
        u = np.unique(X[remaining, f].astype(np.float64))
        if len(u) < 2:
            continue
        thr = 0.5 * (u[0] + u[1])
        threshold[2 * i] = thr
        out = X[remaining, f] <= thr
        depth[remaining[out]] = i + 1
        remaining = remaining[~out]
    tree = dict(feature=feature, threshold=threshold, left=left, right=right, leaf=leaf,
                nan_left=np.zeros(n_nodes, np.uint8), classes=np.array([0, 1]), n_features=F)
    return tree, depth
