"""Node tables and inputs of the tree-variant tests (test_tree_tables_cpu.py,
test_gpu_tree_variants.py, test_gpu_fuzz.py): plain NumPy, no device.

Tables are the oracle's dicts (stream_tree_reference.py): feature (< 0:
leaf), threshold (float64), left, right, leaf (class index), nan_left,
classes, n_features.  Every builder here is checked against
oracle.vad_oracle.tree_predict alone in test_tree_tables_cpu.py, so that what
the GPU tests rely on (classes reached, NaN met at internal nodes, rows
leaving a comb all along it, ladder leaves reached) holds before a kernel is
involved."""
import numpy as np

from stream_tree_reference import classifier, comb_table  # noqa: F401  (re-exported)

LDS_NODES = 3072  # tree_kernel.hip kLdsNodes: the largest table walked from LDS


def _table(feature, threshold, left, right, leaf, nan_left, n_classes, n_features):
    return dict(feature=np.asarray(feature, np.int32), threshold=np.asarray(threshold, np.float64),
                left=np.asarray(left, np.int32), right=np.asarray(right, np.int32),
                leaf=np.asarray(leaf, np.int32), nan_left=np.asarray(nan_left, np.uint8),
                classes=np.arange(n_classes), n_features=int(n_features))


def _nanmedian(v):
    v = v[~np.isnan(v)]
    return float(np.median(v)) if len(v) else None


def bushy_table(n_features, depth, X, seed):
    """A full binary tree of `depth` levels of internal nodes (2^depth - 1 of
    them, 2^depth leaves), numbered in preorder as sklearn numbers its nodes:
    the left child of node i is i + 1, the right child follows the left
    subtree.  Each internal node splits on a random feature below n_features
    at the median (float64: the midpoint of two rows' values, or a row's own
    value -- a tie) of that column of X over the rows that reach the node, NaN
    ignored; a node no finite value reaches takes the column's median (0 for
    an all-NaN column).  nan_left alternates by node index (a left step flips
    it, a right step keeps it), leaf classes cycle over 0..3 from left to
    right."""
    assert 1 <= depth <= 10
    X = np.asarray(X, np.float32)[:, :n_features]
    rng = np.random.default_rng(seed)
    n = 2 ** (depth + 1) - 1
    feature = np.full(n, -1, np.int32)
    threshold = np.zeros(n)
    left = np.full(n, -1, np.int32)
    right = np.full(n, -1, np.int32)
    leaf = np.zeros(n, np.int32)
    nan_left = np.zeros(n, np.uint8)
    col_median = [_nanmedian(X[:, f].astype(np.float64)) or 0.0 for f in range(n_features)]
    n_leaves = 0
    stack = [(0, depth, np.arange(len(X)))]  # node, levels of internal nodes below and including it, rows
    while stack:
        i, h, rows = stack.pop()
        if h == 0:
            leaf[i] = n_leaves % 4
            n_leaves += 1
            continue
        f = feature[i] = rng.integers(0, n_features)
        v = X[rows, f].astype(np.float64)
        med = _nanmedian(v)
        threshold[i] = col_median[f] if med is None else med
        nan_left[i] = i % 2
        with np.errstate(invalid="ignore"):
            go_left = np.where(np.isnan(v), nan_left[i] != 0, v <= threshold[i])
        left[i], right[i] = i + 1, i + 2 ** h
        stack.append((right[i], h - 1, rows[~go_left]))
        stack.append((left[i], h - 1, rows[go_left]))  # popped first: preorder
    return _table(feature, threshold, left, right, leaf, nan_left, 4, n_features)


def pad_table(table, n_nodes):
    """The same tree with leaves that no node points to appended up to n_nodes
    (their classes cycle over the table's, so a walk that strayed into them
    would not be masked by a constant)."""
    n = len(table["feature"])
    extra = n_nodes - n
    assert extra >= 0
    out = dict(table)
    out["feature"] = np.concatenate([table["feature"], np.full(extra, -1, np.int32)]).astype(np.int32)
    out["threshold"] = np.concatenate([table["threshold"], np.zeros(extra)])
    for k in ("left", "right"):
        out[k] = np.concatenate([table[k], np.full(extra, -1, np.int32)]).astype(np.int32)
    out["leaf"] = np.concatenate([table["leaf"], np.arange(extra) % len(table["classes"])]).astype(np.int32)
    out["nan_left"] = np.concatenate([table["nan_left"], np.zeros(extra, np.uint8)]).astype(np.uint8)
    return out


def ladder_table(thresholds, feature, n_features, nan_down=False):
    """A comb over strictly increasing thresholds: spine node i (index 2 i)
    tests x[feature] <= thresholds[i]; its left leaf (2 i + 1) has class i,
    the last right leaf class len(thresholds) -- the label names the interval
    (thresholds[c - 1], thresholds[c]] the value fell into.  At most 255
    thresholds (classes 0..255).  The spine nodes -- the even node indices --
    have nan_left 1, so a NaN leaves at node 0 (class 0); nan_down inverts the
    flags and sends a NaN down the whole spine (the last class)."""
    thr = np.asarray(thresholds, np.float64)
    D = len(thr)
    assert 1 <= D <= 255 and (np.diff(thr) > 0).all()
    n = 2 * D + 1
    spine = 2 * np.arange(D)
    f = np.full(n, -1, np.int32)
    f[spine] = feature
    threshold = np.zeros(n)
    threshold[spine] = thr
    left = np.full(n, -1, np.int32)
    right = np.full(n, -1, np.int32)
    left[spine], right[spine] = spine + 1, spine + 2
    leaf = np.zeros(n, np.int32)
    leaf[spine + 1] = np.arange(D)
    leaf[2 * D] = D
    nan_left = np.zeros(n, np.uint8)
    nan_left[spine] = 0 if nan_down else 1
    return _table(f, threshold, left, right, leaf, nan_left, D + 1, n_features)


# ---------------------------------------------------------------------------
# edge values and thresholds
# ---------------------------------------------------------------------------
F32 = np.finfo(np.float32)
DENORM_MIN = np.float32(1e-45)  # 2^-149
DENORM_MAX = np.nextafter(F32.tiny, np.float32(0))  # the largest float denormal
_POS = [np.float32(0.0), DENORM_MIN, DENORM_MAX, F32.tiny, np.float32(1.0), np.float32(3.0000002), F32.max,
        np.float32(np.inf)]
EDGE_VALUES = np.array([s * v for v in _POS for s in (np.float32(1), np.float32(-1))], np.float32)


def _succ32(v):
    with np.errstate(over="ignore"):  # FLT_MAX -> inf
        return np.nextafter(np.float32(v), np.float32(np.inf))


def _edge_lists():
    """EDGE_THRESHOLDS: each edge value v as a double, the doubles either side
    of it, +-0, the double denormal minimum, +-1e-50 (doubles far below every
    float), +-FLT_MAX with its double neighbours, +-1e300 and -inf -- and
    powers of two across the float range up to 255 entries, so that the
    ladder's classes reach 255.  (+inf is left to SINGLE_THRESHOLDS: as the
    last rung it would leave the last class to NaN alone.)  TIE_THRESHOLDS: the midpoint of each finite v
    and its float successor, where (float)threshold is a tie, with v itself
    and the same powers of two.

    The midpoints stand in a ladder of their own: v < nextafter(v) < midpoint
    < succ(v) leaves two intervals that no float can fall into for every v,
    and one ladder over all of them reaches half of its leaves; apart, the
    first reaches over 90 % and the second all of them
    (test_tree_tables_cpu.py)."""
    fmax = float(F32.max)
    edge, ties = [], []
    for v in EDGE_VALUES:
        d = float(v)
        edge += [d, float(np.nextafter(d, np.inf)), float(np.nextafter(d, -np.inf))]
        if np.isfinite(v):
            ties += [d, 0.5 * d + 0.5 * float(_succ32(v))]
    edge += [0.0, -0.0, 5e-324, -5e-324, 1e-50, -1e-50, 1e300, -1e300, np.inf, -np.inf]
    for s in (1.0, -1.0):
        edge += [s * fmax, s * float(np.nextafter(fmax, np.inf)), s * float(np.nextafter(fmax, -np.inf))]
    edge = np.unique(np.array(edge))  # sorted, equal values (+-0) once
    edge = edge[edge < np.inf]
    ties = np.unique(np.array(ties))
    ties = ties[np.isfinite(ties)]
    k = np.arange(-148.0, 128.0)
    fill = np.concatenate([-(2.0 ** k[::-1]), 2.0 ** k])
    out = []
    for base in (edge, ties):
        cand = fill[~np.isin(fill, base)]
        extra = cand[np.linspace(0, len(cand) - 1, 255 - len(base)).round().astype(int)]  # spread evenly
        out.append(np.unique(np.concatenate([base, extra])))
    assert len(out[0]) == 255 and len(out[1]) <= 255
    return out[0], out[1]


EDGE_THRESHOLDS, TIE_THRESHOLDS = _edge_lists()
# one-rung ladders: what a sorted, deduplicated ladder cannot hold (-0.0 beside 0.0, +inf last)
SINGLE_THRESHOLDS = (0.0, -0.0, 5e-324, -5e-324, np.inf, -np.inf)


def round_f32(t, up):
    """Doubles t rounded to float32 toward +inf (up) or -inf."""
    t = np.asarray(t, np.float64)
    with np.errstate(over="ignore"):
        f = t.astype(np.float32)
        if up:
            return np.where(f.astype(np.float64) < t, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)
        return np.where(f.astype(np.float64) > t, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def edge_inputs(thresholds):
    """Every edge value, every threshold rounded to float32 both ways, and
    NaN: float32, duplicates (by bit pattern) removed."""
    v = np.concatenate([EDGE_VALUES, round_f32(thresholds, True), round_f32(thresholds, False),
                        np.array([np.nan], np.float32)]).astype(np.float32)
    _, first = np.unique(v.view(np.uint32), return_index=True)
    return v[np.sort(first)]


# ---------------------------------------------------------------------------
# MFCC-like rows and the tables of the variant matrix
# ---------------------------------------------------------------------------
def mfcc_like_rows(n_frames, mfcc_n, seed, runs=()):
    """MFCC-like float32 rows of any width (coefficient scales as the
    pipeline's, c0 ~ -100 .. 50) with runs of 8 equal rows -- one per 100
    frames at random places, and one at every index of `runs` -- so that the
    windows inside a run are flat: NaN Mn and D2 in analyser mode; and as many
    runs in which only some of the coefficients stay equal, so that NaN
    windows do not all share one feature pattern (one path through a
    tree)."""
    rng = np.random.default_rng(seed)
    scale = np.array([40.0] + [12.0 / (1 + 0.3 * c) for c in range(1, mfcc_n)], np.float32)
    m = (rng.standard_normal((n_frames, mfcc_n)).astype(np.float32) * scale).astype(np.float32)
    m[:, 0] -= 30.0
    starts = list(rng.integers(0, max(n_frames - 8, 1), size=max(n_frames // 100, 1))) + list(runs)
    for s in starts:
        m[s:s + 8] = m[s]
    for s in rng.integers(0, max(n_frames - 8, 1), size=len(starts)):
        cols = np.flatnonzero(rng.random(mfcc_n) < 0.5)
        m[s:s + 8, cols] = m[s, cols]
    return m


WIDTHS = (13, 1, 12, 16)
WINDOWS = (1, 255, 256, 257, 1000)  # one chunk of 256 minus one, one chunk, plus one, four with a ragged tail
TREES = ("bushy", "bushy_3072", "bushy_3073", "bushy_narrow", "comb_3072", "comb_3073")


def narrow_features(mfcc_n):
    return 2 if mfcc_n == 1 else 2 * mfcc_n + 1


def variant_tables(X, mfcc_n):
    """The tables of one width and mode, built on the feature rows X (the
    1,000-window case): name -> table, and the comb's exit depth per row of X.
    Combs split on the D1 columns, finite whatever the mode."""
    X = np.asarray(X, np.float32)
    assert X.shape[1] == 3 * mfcc_n
    bushy = bushy_table(3 * mfcc_n, 8, X, seed=mfcc_n)
    out = {"bushy": bushy, "bushy_3072": pad_table(bushy, LDS_NODES), "bushy_3073": pad_table(bushy, LDS_NODES + 1),
           "bushy_narrow": bushy_table(narrow_features(mfcc_n), 8, X, seed=100 + mfcc_n)}
    depth = {}
    for n in (LDS_NODES, LDS_NODES + 1):
        out[f"comb_{n}"], depth[f"comb_{n}"] = comb_table(n, X, list(range(mfcc_n, 2 * mfcc_n)))
    return out, depth


def nan_nodes(table, X):
    """Per row of X: the internal nodes at which its walk met a NaN feature,
    as a list of (row, node)."""
    X = np.asarray(X, np.float32)[:, :table["n_features"]]
    node = np.zeros(len(X), np.int64)
    rows = np.arange(len(X))
    met = []
    for _ in range(len(table["feature"])):
        f = table["feature"][node]
        internal = f >= 0
        if not internal.any():
            break
        v = X[rows, np.maximum(f, 0)]
        nan = np.isnan(v) & internal
        met += list(zip(rows[nan].tolist(), node[nan].tolist()))
        go_left = np.where(np.isnan(v), table["nan_left"][node] != 0, v.astype(np.float64) <= table["threshold"][node])
        node = np.where(internal, np.where(go_left, table["left"][node], table["right"][node]), node)
    return met
