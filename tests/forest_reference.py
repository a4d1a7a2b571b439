"""The forest reference of the tests: the definition of vad_amd/forest.py in
numpy.  Per row K double accumulators start at 0; for t = 0 .. T-1 in order
acc += proba[leaf_t]; then acc /= T.  The score is float32(acc[active]), the
label the first maximum.  The walk is sklearn's: float32 feature against the
float64 threshold, a NaN feature following nan_left.

A forest here is a dict of arrays: feature, threshold, left, right, nan_left,
roots, proba (the fields of vad_amd.forest.ForestClassifier)."""
import numpy as np

KEYS = ("feature", "threshold", "left", "right", "leaf", "nan_left", "roots", "proba")


def table(forest):
    return {k: np.asarray(getattr(forest, k)) for k in KEYS}


def leaves(f, X):
    """(T, n) the node every row ends in, per tree."""
    X = np.asarray(X, np.float32)
    out = []
    for r in np.asarray(f["roots"]):
        node = np.full(len(X), int(r), np.int64)
        for _ in range(len(f["feature"])):
            feat = f["feature"][node]
            inner = feat >= 0
            if not inner.any():
                break
            xv = X[np.arange(len(X)), np.maximum(feat, 0)].astype(np.float64)
            left = np.where(np.isnan(xv), f["nan_left"][node] != 0, xv <= f["threshold"][node])
            node = np.where(inner, np.where(left, f["left"][node], f["right"][node]), node)
        out.append(node)
    return np.stack(out)


def predict_proba(f, X):
    lv = leaves(f, X)
    acc = np.zeros((lv.shape[1], f["proba"].shape[1]), np.float64)
    for t in range(lv.shape[0]):
        acc += f["proba"][lv[t]]
    acc /= lv.shape[0]
    return acc


def predict_index(f, X):
    return np.argmax(predict_proba(f, X), axis=1)


def scores(f, X, active=1):
    return predict_proba(f, X)[:, active].astype(np.float32)


def random_tree(n_nodes, F, K=2, seed=0):
    """A random binary tree of exactly n_nodes (odd) nodes in preorder over F
    features, thresholds ~ N(0, 1), random shares per node: the dict of arrays
    TreeClassifier takes, with proba rows."""
    assert n_nodes % 2 == 1
    rng = np.random.default_rng(seed)
    feat = np.full(n_nodes, -1, np.int32)
    thr = np.full(n_nodes, -2.0)
    left = np.full(n_nodes, -1, np.int32)
    right = np.full(n_nodes, -1, np.int32)
    stack = [(0, n_nodes)]
    while stack:
        at, size = stack.pop()
        if size == 1:
            continue
        ls = 1 + 2 * int(rng.integers(0, (size - 1) // 2))  # odd, 1 .. size - 2
        feat[at] = rng.integers(0, F)
        thr[at] = rng.normal()
        left[at], right[at] = at + 1, at + 1 + ls
        stack += [(at + 1, ls), (at + 1 + ls, size - 1 - ls)]
    p = rng.random((n_nodes, K))
    p /= p.sum(axis=1)[:, None]
    return dict(feature=feat, threshold=thr, left=left, right=right, leaf=np.argmax(p, axis=1).astype(np.int32),
                nan_left=rng.integers(0, 2, n_nodes).astype(np.uint8), proba=p)


def chain_tree(n_nodes, K=2, feature=0, seed=0):
    """A synthetic tree of exactly n_nodes (odd) nodes in preorder: a right
    spine of rising thresholds on one feature, every left child a leaf.  As
    the dict of arrays TreeClassifier takes, with proba rows."""
    assert n_nodes % 2 == 1
    m = n_nodes // 2  # internal nodes
    rng = np.random.default_rng(seed)
    feat = np.full(n_nodes, -1, np.int32)
    thr = np.full(n_nodes, -2.0)
    left = np.full(n_nodes, -1, np.int32)
    right = np.full(n_nodes, -1, np.int32)
    cuts = np.linspace(-3.0, 3.0, m) if m else np.zeros(0)
    for i in range(m):  # internal node i at 2 i, its left leaf at 2 i + 1
        feat[2 * i] = feature
        thr[2 * i] = cuts[i]
        left[2 * i] = 2 * i + 1
        right[2 * i] = 2 * i + 2
    p = rng.random((n_nodes, K))
    p /= p.sum(axis=1)[:, None]
    return dict(feature=feat, threshold=thr, left=left, right=right, leaf=np.argmax(p, axis=1).astype(np.int32),
                nan_left=(np.arange(n_nodes) % 3 == 0).astype(np.uint8), proba=p)
