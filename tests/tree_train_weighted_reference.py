"""The weighted tree-training reference of the tests: the rule of DESIGN.md
section 4, "Integer row weights" (sklearn 1.7.2's ``fit(X, y,
sample_weight=w)`` for integer w, ties decided as in the unweighted rule), in
numpy, one node at a time.

A row of weight 0 is not in the job.  n_node_samples, the three parameters, a
candidate's position p and nan_left (p > n - p) count distinct rows; the class
counts are weighted, c[k] = sum of w over the node's rows of class k, W their
total; the score of a candidate is (sum_k cL[k]^2) / WL + (sum_k cR[k]^2) / WR
(integer sums exact, the two divisions and the addition rounded once each in
double); a node is pure when max_k c[k] == W; leaf is the first maximum of the
weighted counts and value holds them.

``fit`` returns the table of ``tree_train_reference.fit`` (preorder); with all
weights 1 it is that table byte for byte."""
import numpy as np

import tree_train_reference as R

KEYS = R.KEYS
threshold = R.threshold
synth = R.synth
tables_equal = R.tables_equal

MAX_TOTAL = 1 << 26


def scores(Xn, yn, wn, K, min_samples_leaf):
    """Per (position p = 1..n-1, feature): the weighted score of the candidate,
    -1 where there is none; the sorted values (n, F); the order."""
    n, F = Xn.shape
    order = np.argsort(Xn, axis=0, kind="stable")
    xs = np.take_along_axis(Xn, order, 0)
    ys = yn[order]
    ws = wn.astype(np.int64)[order]
    cl = np.stack([np.cumsum(np.where(ys == k, ws, 0), axis=0, dtype=np.int64) for k in range(K)], axis=-1)
    tot = cl[-1]
    cL = cl[:-1]
    cR = tot[None] - cL
    p = np.arange(1, n, dtype=np.int64)[:, None]
    valid = (xs[1:] > xs[:-1]) & (p >= min_samples_leaf) & (n - p >= min_samples_leaf)
    sL = (cL * cL).sum(-1).astype(np.float64)  # exact integers below 2^53, then one rounding each
    sR = (cR * cR).sum(-1).astype(np.float64)
    sc = sL / cL.sum(-1).astype(np.float64) + sR / cR.sum(-1).astype(np.float64)
    return np.where(valid, sc, -1.0), xs, order


def counts_of(y, w, K):
    return np.bincount(y, weights=None if w is None else w, minlength=K).astype(np.int64)


def is_leaf(n, counts, depth, max_depth, min_samples_split, min_samples_leaf):
    """n: distinct rows; counts: weighted class counts."""
    return depth >= max_depth or n < min_samples_split or n < 2 * min_samples_leaf or counts.max() == counts.sum()


def best_split(Xn, yn, wn, K, min_samples_leaf):
    """(score, feature, p, threshold, nan_left, order of the feature) or None."""
    n = Xn.shape[0]
    if n < 2:
        return None
    sc, xs, order = scores(Xn, yn, wn, K, min_samples_leaf)
    m = sc.max()
    if m < 0:
        return None
    f = int(np.argmax(sc.max(axis=0) == m))
    p = int(np.argmax(sc[:, f] == m)) + 1
    return m, f, p, threshold(xs[p - 1, f], xs[p, f]), p > n - p, order[:, f]


def fit(X, y, w, K, max_depth, min_samples_split, min_samples_leaf):
    """w: integer weights (n,), 0 leaves a row out (None: all ones)."""
    X = np.ascontiguousarray(X, np.float32)
    y = np.asarray(y).astype(np.int64)
    w = np.ones(len(y), np.int64) if w is None else np.asarray(w).astype(np.int64)
    assert w.shape == y.shape and w.min() >= 0 and 0 < w.sum() <= MAX_TOTAL
    out = {k: [] for k in KEYS}
    stack = [(np.flatnonzero(w > 0), 0, -1, False)]
    while stack:
        r, depth, parent, is_left = stack.pop()
        i = len(out["feature"])
        if parent >= 0:
            out["left" if is_left else "right"][parent] = i
        counts = counts_of(y[r], w[r], K)
        n = len(r)
        split = None
        if not is_leaf(n, counts, depth, max_depth, min_samples_split, min_samples_leaf):
            split = best_split(X[r], y[r], w[r], K, min_samples_leaf)
        out["n_node_samples"].append(n)
        out["depth"].append(depth)
        out["value"].append(counts)
        out["leaf"].append(int(np.argmax(counts)))
        out["left"].append(-1)
        out["right"].append(-1)
        if split is None:
            out["feature"].append(-1)
            out["threshold"].append(-2.0)
            out["nan_left"].append(0)
            continue
        _, f, p, t, nan_left, order = split
        out["feature"].append(f)
        out["threshold"].append(t)
        out["nan_left"].append(int(nan_left))
        stack.append((np.sort(r[order[p:]]), depth + 1, i, False))
        stack.append((np.sort(r[order[:p]]), depth + 1, i, True))
    dt = dict(feature=np.int32, threshold=np.float64, left=np.int32, right=np.int32, leaf=np.int32, nan_left=np.uint8,
              n_node_samples=np.int32, depth=np.int32, value=np.int32)
    return {k: np.asarray(v, dt[k]).reshape((-1, K) if k == "value" else (-1,)) for k, v in out.items()}


def check_tree_nodewise(x, y, w, K, md, mss, msl, left, right, feature, thr, n_node, mgl, weighted_n=None, value=None):
    """Walk an sklearn tree fitted with sample_weight=w; at every node compare
    with the weighted rule on the rows that reach the node: leaf or split,
    n_node_samples (distinct rows), the score of sklearn's choice (the maximum,
    at the first position of its feature that has it), threshold,
    missing_go_to_left, and -- where given -- weighted_n_node_samples and
    ``value`` (sklearn's class fractions) against counts / W bit for bit.
    Returns (nodes, splits, nodes with a score tie between features)."""
    w = np.asarray(w).astype(np.int64)
    y = np.asarray(y).astype(np.int64)
    rows = {0: np.flatnonzero(w > 0)}
    depth = {0: 0}
    ties = splits = 0
    for i in range(len(left)):  # preorder: a parent comes before its children
        r = rows.pop(i)
        n = len(r)
        assert n == n_node[i], (i, n, n_node[i])
        counts = counts_of(y[r], w[r], K)
        W = int(counts.sum())
        if weighted_n is not None:
            assert float(W) == weighted_n[i], (i, W, weighted_n[i])
        if value is not None:
            want = counts.astype(np.float64) / np.float64(W)
            assert want.tobytes() == np.asarray(value[i], np.float64).tobytes(), (i, want, value[i])
        leaf = is_leaf(n, counts, depth[i], md, mss, msl)
        sc = None
        if not leaf:
            sc, xs, order = scores(x[r], y[r], w[r], K, msl)
            leaf = sc.max() < 0
        if left[i] < 0:
            assert leaf, f"node {i}: sklearn made a leaf, the rule splits"
            continue
        assert not leaf, f"node {i}: sklearn split, the rule makes a leaf"
        splits += 1
        f = int(feature[i])
        goes_left = x[r, f].astype(np.float64) <= thr[i]
        p = int(goes_left.sum())
        assert 1 <= p < n
        m = sc.max()
        assert sc[p - 1, f].tobytes() == m.tobytes(), (i, f, p, sc[p - 1, f], m)
        assert int(np.argmax(sc[:, f] == m)) == p - 1, f"node {i}: not the first maximum of feature {f}"
        ties += int((sc.max(axis=0) == m).sum() > 1)
        t = threshold(xs[p - 1, f], xs[p, f])
        assert np.float64(t).tobytes() == np.float64(thr[i]).tobytes(), (i, t, thr[i])
        assert bool(mgl[i]) == (p > n - p), i
        assert np.array_equal(np.sort(order[:p, f]), np.flatnonzero(goes_left))
        rows[int(left[i])], rows[int(right[i])] = r[goes_left], r[~goes_left]
        depth[int(left[i])] = depth[int(right[i])] = depth[i] + 1
    return len(left), splits, ties


# the weight kinds of the fixtures and the GPU tests
def bootstrap_counts(n, seed):
    return np.bincount(np.random.default_rng(seed).integers(0, n, n), minlength=n).astype(np.int64)


def class_integers(y, K, seed):
    return (np.random.default_rng(seed).integers(1, 8, K))[np.asarray(y).astype(np.int64)].astype(np.int64)


def weights_of(kind, y, K, seed):
    n = len(y)
    if kind == "boot":
        return bootstrap_counts(n, seed)
    if kind == "class":
        return class_integers(y, K, seed + 1)
    assert kind == "both"
    return bootstrap_counts(n, seed) * class_integers(y, K, seed + 1)
