"""The tree-training reference of the tests: the rule of DESIGN.md section 4
(sklearn 1.7.2's Gini / best splitter, all features, unweighted rows, ties
decided: lowest feature, then lowest position) in numpy, one node at a time,
and the seeded synthetic rows the tests run on.

``fit`` returns the node table in preorder as a dict of arrays: feature (-1:
leaf), threshold (float64, -2 at a leaf), left, right (-1 at a leaf), leaf
(first maximum of the class counts), nan_left, n_node_samples, depth, value
(n_nodes, K) class counts."""
import numpy as np

KEYS = ("feature", "threshold", "left", "right", "leaf", "nan_left", "n_node_samples", "depth", "value")


def scores(Xn, yn, K, min_samples_leaf):
    """Per (position p = 1..n-1, feature): the score of the candidate, -1 where
    there is none; and the sorted values (n, F)."""
    n, F = Xn.shape
    order = np.argsort(Xn, axis=0, kind="stable")
    xs = np.take_along_axis(Xn, order, 0)
    ys = yn[order]
    cl = np.stack([np.cumsum(ys == k, axis=0, dtype=np.int64) for k in range(K)], axis=-1)  # (n, F, K)
    tot = cl[-1]
    cL = cl[:-1]
    cR = tot[None] - cL
    p = np.arange(1, n, dtype=np.int64)[:, None]
    valid = (xs[1:] > xs[:-1]) & (p >= min_samples_leaf) & (n - p >= min_samples_leaf)
    sL = (cL * cL).sum(-1).astype(np.float64)  # exact integer sums, then one rounding each
    sR = (cR * cR).sum(-1).astype(np.float64)
    sc = sL / p.astype(np.float64) + sR / (n - p).astype(np.float64)
    return np.where(valid, sc, -1.0), xs, order


def threshold(x0, x1):
    """sklearn _splitter.pyx:456-465 on two float32 neighbours, in double."""
    t = np.float64(x0) / 2.0 + np.float64(x1) / 2.0
    if t == np.float64(x1) or np.isinf(t):
        t = np.float64(x0)
    return t


def is_leaf(n, counts, depth, max_depth, min_samples_split, min_samples_leaf):
    return depth >= max_depth or n < min_samples_split or n < 2 * min_samples_leaf or counts.max() == n


def best_split(Xn, yn, K, min_samples_leaf):
    """(score, feature, p, threshold, nan_left, order of the feature) or None."""
    n = Xn.shape[0]
    if n < 2:
        return None
    sc, xs, order = scores(Xn, yn, K, min_samples_leaf)
    m = sc.max()
    if m < 0:
        return None
    f = int(np.argmax(sc.max(axis=0) == m))
    p = int(np.argmax(sc[:, f] == m)) + 1
    return m, f, p, threshold(xs[p - 1, f], xs[p, f]), p > n - p, order[:, f]


def fit(X, y, K, max_depth, min_samples_split, min_samples_leaf, rows=None):
    X = np.ascontiguousarray(X, np.float32)
    y = np.asarray(y).astype(np.int64)
    rows = np.arange(X.shape[0]) if rows is None else np.asarray(rows, np.int64)
    out = {k: [] for k in KEYS}
    stack = [(np.sort(rows), 0, -1, False)]
    while stack:
        r, depth, parent, is_left = stack.pop()
        i = len(out["feature"])
        if parent >= 0:
            out["left" if is_left else "right"][parent] = i
        counts = np.bincount(y[r], minlength=K)
        n = len(r)
        split = None
        if not is_leaf(n, counts, depth, max_depth, min_samples_split, min_samples_leaf):
            split = best_split(X[r], y[r], K, min_samples_leaf)
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


def walk(t, X):
    """Leaf class index of every row, by sklearn's traversal on the host."""
    X = np.asarray(X, np.float32)
    node = np.zeros(len(X), np.int64)
    for _ in range(int(t["depth"].max()) + 1):
        f = t["feature"][node]
        inner = f >= 0
        xv = X[np.arange(len(X)), np.where(inner, f, 0)].astype(np.float64)
        go_left = np.where(np.isnan(xv), t["nan_left"][node] != 0, xv <= t["threshold"][node])
        node = np.where(inner, np.where(go_left, t["left"][node], t["right"][node]), node)
    return t["leaf"][node]


def tables_equal(a, b):
    """Every array bitwise (thresholds as doubles); returns the first key that differs, or None."""
    for k in KEYS:
        x, z = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != z.shape or x.dtype != z.dtype or x.tobytes() != z.tobytes():
            return k
    return None


def synth(n, F, K, seed, spread=1.5):
    """Rows with class centres, plus the columns a splitter can get wrong:
    the last column constant, before it one of 0.5 + j * 2^-24 (neighbouring
    float32 values, j following the label loosely), a two-valued column, a
    copy of column 0 (an exact score tie between two features), a column
    rounded to quarters and a permuted copy of it."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((K, F))
    y = rng.integers(0, K, n).astype(np.uint8)
    x = (centres[y] + spread * rng.standard_normal((n, F))).astype(np.float32)
    if F == 1:
        x[:, 0] = np.round(x[:, 0] * 4) / 4
        return x, y
    if F >= 5:
        x[:, F - 1] = 0.25
        j = (y.astype(np.int64) + rng.integers(0, 3, n)) % 4
        x[:, F - 2] = (0.5 + j * 2.0 ** -24).astype(np.float32)
        x[:, F - 3] = (x[:, F - 3] > 0).astype(np.float32)
        x[:, F - 4] = x[:, 0]
    if F >= 7:
        x[:, 1] = np.round(x[:, 1] * 4) / 4
        x[:, 2] = x[rng.permutation(n), 1]
    return x, y
