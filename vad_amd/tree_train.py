"""Training the decision tree on the device (the reference fits sklearn's
``DecisionTreeClassifier(min_samples_split=22, max_depth=25,
min_samples_leaf=20)`` in learning/decision_classifier_trainer.py:26-30 and
chooses those parameters with a ``GridSearchCV`` over 7 x 4 x 4 settings in
learning/cross_validation.py:20-27).

    tree = TreeTrainer().fit(X, y)                    # a TreeClassifier
    res = TreeTrainer().grid(X, y, [3, 5, 10, 15, 20, 25, 30], [2, 10, 22, 40],
                             [1, 5, 20, 40], kfold(len(X), 3))

The rule is sklearn 1.7.2's (Gini, best splitter, all features), with ties
between features decided: the lowest feature, then the lowest position
(DESIGN.md section 4).  ``fit_many`` grows any number of trees -- each a set
of rows and its three parameters -- in one chain of launches
(csrc/tree_train_kernel.hip); the rows are sorted once per call, by one
``torch.sort``.  The kernels number a tree's nodes level by level; this
module renumbers them to sklearn's preorder on the host.  The split chosen at
a node depends on neither ``max_depth`` nor ``min_samples_split``, so the
tree for smaller values of either is the big tree cut short: ``prune``.
``grid`` therefore trains one tree per (fold, ``min_samples_leaf``) and prunes
for the rest: the reference's 112 x 3 fits are 12 device jobs.

A job may carry a feature subset (a fifth element): the tree then splits on
those columns only, and ``fit_forest`` trains a bagged forest that way -- rows
sampled without replacement and a feature subset per tree, drawn on the host
(``forest_draws``), all trees in one call; it returns a
``vad_amd.forest.ForestClassifier``.

Rows may carry integer weights (a sixth element of a job; ``sample_weight=``
and ``class_weight=`` of ``fit``, ``fit_forest`` and ``grid``): the tree is
sklearn's ``fit(X, y, sample_weight=w)``.  Distinct rows go on counting for
``n_node_samples`` and the three parameters; class counts, scores, purity and
``value`` are weighted.  A row weighs at most 255 and a
job at most 2^26 in all, so that every sum is an exact integer.
``fit_forest(bootstrap=True)`` draws rows WITH replacement, as sklearn's
``RandomForestClassifier`` does: tree t is fitted with the counts of its draw
as weights.  ``balanced_integer_weights`` gives integer class weights in the
proportions of ``class_weight="balanced"``.

There is no CPU path: the trees grow in the HIP kernels or the call raises.
"""
from __future__ import annotations

import ctypes
import time

import numpy as np
import torch

from ._lib import VAD_ENOMEM, VadError, check, lib, stream_ptr
from .tree import TreeClassifier

MAX_FEATURES = 64
MAX_CLASSES = 8
MAX_ROWS = 1 << 27
MAX_ROW_WEIGHT = 255
MAX_TOTAL_WEIGHT = 1 << 26


class _Job(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_int64), ("node_capacity", ctypes.c_int64), ("max_depth", ctypes.c_int32),
                ("min_samples_split", ctypes.c_int32), ("min_samples_leaf", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


_TABLES = (("feature", torch.int32), ("threshold", torch.float64), ("left", torch.int32), ("right", torch.int32),
           ("leaf", torch.int32), ("nan_left", torch.uint8), ("n_node_samples", torch.int32),
           ("depth", torch.int32), ("value", torch.int32), ("n_nodes", torch.int32), ("status", torch.int32))


class _Tables(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k, _ in _TABLES]


def kfold(n, k):
    """sklearn's unshuffled ``KFold(k)``: k consecutive blocks, the first
    ``n % k`` one row longer; [(train_idx, test_idx), ...]."""
    n, k = int(n), int(k)
    if not 2 <= k <= n:
        raise ValueError("kfold: need 2 <= k <= n")
    sizes = np.full(k, n // k, np.int64)
    sizes[:n % k] += 1
    ends = np.cumsum(sizes)
    idx = np.arange(n, dtype=np.int64)
    return [(np.concatenate([idx[:e - s], idx[e:]]), idx[e - s:e]) for s, e in zip(sizes, ends)]


def check_params(max_depth, min_samples_split, min_samples_leaf):
    md, mss, msl = int(max_depth), int(min_samples_split), int(min_samples_leaf)
    if md < 1 or mss < 2 or msl < 1 or max(md, mss, msl) >= 2 ** 31:
        raise ValueError("need max_depth >= 1, min_samples_split >= 2, min_samples_leaf >= 1")
    return md, mss, msl


def check_rows(X, y):
    """Shapes, limits and finiteness (ValueError), before anything touches the
    device.  Returns X (float32, contiguous, as given: numpy or torch), the
    class indices (uint8 numpy) and ``classes_``."""
    if isinstance(X, torch.Tensor):
        Xc = X.detach()
        if Xc.dtype != torch.float32:
            Xc = Xc.to(torch.float32)
        Xc = Xc.contiguous()
    else:
        Xc = np.ascontiguousarray(X, np.float32)
    if Xc.ndim != 2:
        raise ValueError(f"X must be (n_rows, n_features), got {tuple(Xc.shape)}")
    n, F = (int(v) for v in Xc.shape)
    if not 1 <= F <= MAX_FEATURES:
        raise ValueError(f"n_features must be 1..{MAX_FEATURES}, got {F}")
    if not 1 <= n < MAX_ROWS:
        raise ValueError(f"n_rows must be 1..2^27 - 1, got {n}")
    yh = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
    if yh.shape != (n,):
        raise ValueError(f"y must be ({n},), got {yh.shape}")
    finite = bool(torch.isfinite(Xc).all()) if isinstance(Xc, torch.Tensor) else bool(np.isfinite(Xc).all())
    if not finite:
        raise ValueError("X holds NaN or infinity: training rows must be finite")
    classes, idx = np.unique(yh, return_inverse=True)
    if len(classes) > MAX_CLASSES:
        raise ValueError(f"{len(classes)} classes, at most {MAX_CLASSES}")
    return Xc, idx.astype(np.uint8).reshape(n), classes


def check_job_weights(w, n):
    """A job's row weights: an integer array (n,) of 0..255 with at least one
    above 0 and at most 2^26 in all (ValueError); returns it as uint8."""
    w = np.asarray(w.cpu() if isinstance(w, torch.Tensor) else w)
    if w.dtype.kind not in "iu":
        raise ValueError(f"row weights must be integers, got dtype {w.dtype} (float weights are not supported)")
    if w.shape != (int(n),):
        raise ValueError(f"row weights must be ({int(n)},), got {w.shape}")
    if w.size and w.min() < 0:
        raise ValueError("row weights must be >= 0")
    if not (w > 0).any():
        raise ValueError("row weights need at least one row above 0")
    if w.max() > MAX_ROW_WEIGHT:
        raise ValueError(f"a row's weight (sample_weight * class_weight) must be <= {MAX_ROW_WEIGHT}, got {int(w.max())}")
    total = int(w.astype(np.int64).sum())
    if total > MAX_TOTAL_WEIGHT:
        raise ValueError(f"the total weight of a tree's rows must be <= 2^26, got {total}")
    return w.astype(np.uint8)


def row_weights(y, classes, sample_weight=None, class_weight=None):
    """``sample_weight[i] * class_weight[y[i]]`` as int64 (n,), or None when
    both are None.  ``sample_weight``: integers (n,), >= 0; ``class_weight``:
    {class value: positive int} with exactly the keys ``classes``.  Every
    violation is a ValueError; the limits of the product are
    ``check_job_weights``'s."""
    if sample_weight is None and class_weight is None:
        return None
    y = np.asarray(y)
    n = len(y)
    w = np.ones(n, np.int64)
    if sample_weight is not None:
        sw = np.asarray(sample_weight.cpu() if isinstance(sample_weight, torch.Tensor) else sample_weight)
        if sw.dtype.kind not in "iu":
            raise ValueError(f"sample_weight must be integers, got dtype {sw.dtype} (float weights are not supported)")
        if sw.shape != (n,):
            raise ValueError(f"sample_weight must be ({n},), got {sw.shape}")
        if n and sw.min() < 0:
            raise ValueError("sample_weight must be >= 0")
        if not (sw > 0).any():
            raise ValueError("sample_weight needs at least one row above 0")
        if sw.max() > MAX_TOTAL_WEIGHT:
            raise ValueError("sample_weight is past the limits: a row's weight must be <= 255")
        w = sw.astype(np.int64)
    if class_weight is not None:
        if isinstance(class_weight, str):
            raise ValueError(f"class_weight={class_weight!r} is not supported: the weights must be integers; "
                             "balanced_integer_weights(y) gives a dict in the proportions of \"balanced\"")
        if not isinstance(class_weight, dict):
            raise ValueError("class_weight must be a dict {class value: positive int}")
        keys = list(class_weight)
        want = np.asarray(classes).tolist()
        if len(keys) != len(want) or any(k not in keys for k in want):
            raise ValueError(f"class_weight must have exactly the classes {want} as keys, got {keys}")
        cw = np.zeros(len(want), np.int64)
        for i, k in enumerate(want):
            v = class_weight[k]
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or int(v) < 1:
                raise ValueError(f"class_weight[{k!r}] must be a positive integer, got {v!r}")
            if int(v) > MAX_ROW_WEIGHT:
                raise ValueError(f"class_weight[{k!r}] must be <= {MAX_ROW_WEIGHT}, got {v!r}")
            cw[i] = int(v)
        w = w * cw[np.searchsorted(np.asarray(classes), y)]
    return w


def balanced_integer_weights(y, max_weight=255):
    """Integer class weights in the proportions of sklearn's
    ``class_weight="balanced"`` (n / (K * count_k)): {class:
    clip(round(max_count / count_k), 1, max_weight)}, the most frequent class
    at 1 (``round`` to the nearest, halves to even).  Scaling all weights by a
    constant does not change a Gini tree, so only the proportions matter; they
    are met to the rounding."""
    max_weight = int(max_weight)
    if not 1 <= max_weight <= MAX_ROW_WEIGHT:
        raise ValueError(f"max_weight must be 1..{MAX_ROW_WEIGHT}")
    yh = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
    if yh.ndim != 1 or yh.size < 1:
        raise ValueError("y must be a non-empty 1-D array")
    classes, counts = np.unique(yh, return_counts=True)
    top = int(counts.max())
    return {c.item(): int(min(max(round(top / int(k)), 1), max_weight)) for c, k in zip(classes, counts)}


def preorder(t):
    """A level-ordered node table (dict of arrays with ``depth``) renumbered
    node, left subtree, right subtree -- sklearn's depth-first numbering."""
    left, right, depth = t["left"], t["right"], t["depth"]
    m = len(left)
    size = np.ones(m, np.int64)
    inner = left >= 0
    top = int(depth.max()) if m else 0
    for d in range(top - 1, -1, -1):
        i = np.flatnonzero(inner & (depth == d))
        size[i] = 1 + size[left[i]] + size[right[i]]
    new = np.zeros(m, np.int64)
    for d in range(top):
        i = np.flatnonzero(inner & (depth == d))
        new[left[i]] = new[i] + 1
        new[right[i]] = new[i] + 1 + size[left[i]]
    out = {}
    for k, v in t.items():
        a = np.empty_like(v)
        a[new] = v
        out[k] = a
    for k in ("left", "right"):
        a = out[k]
        a[a >= 0] = new[a[a >= 0]].astype(a.dtype)
    return out


_NODE_KEYS = ("feature", "threshold", "left", "right", "leaf", "nan_left", "n_node_samples", "depth", "value")


def _table(tree):
    if tree.n_node_samples is None or tree.depth is None or tree.value is None:
        raise ValueError("the tree carries no n_node_samples / depth / value: it was not trained here")
    return {k: getattr(tree, k) for k in _NODE_KEYS}


def prune_table(t, max_depth, min_samples_split):
    """The preorder table ``t`` cut where ``depth >= max_depth`` or
    ``n_node_samples < min_samples_split``, renumbered in preorder."""
    depth, left, right = t["depth"], t["left"], t["right"]
    cut = (depth >= int(max_depth)) | (t["n_node_samples"] < int(min_samples_split))
    inner = (left >= 0) & ~cut
    keep = np.zeros(len(left), bool)
    keep[0] = True
    for d in range(int(depth.max())):
        i = np.flatnonzero(keep & inner & (depth == d))
        keep[left[i]] = True
        keep[right[i]] = True
    new = np.cumsum(keep) - 1  # dropping whole subtrees keeps the preorder
    out = {k: np.array(v[keep]) for k, v in t.items()}
    leafed = ~inner[keep]
    out["feature"][leafed] = -1
    out["threshold"][leafed] = -2.0
    out["nan_left"][leafed] = 0
    for k in ("left", "right"):
        a = out[k]
        a[leafed] = -1
        a[~leafed] = new[a[~leafed]].astype(a.dtype)
    return out


def prune(tree, max_depth, min_samples_split):
    """The tree that training with a smaller ``max_depth`` and / or a larger
    ``min_samples_split`` (same rows, same ``min_samples_leaf``) gives."""
    t = prune_table(_table(tree), max_depth, min_samples_split)
    return TreeClassifier(*(t[k] for k in _NODE_KEYS[:6]), tree.classes_, tree.n_features,
                          n_node_samples=t["n_node_samples"], depth=t["depth"], value=t["value"])


def feature_mask(features, F):
    """The 64-bit mask of a job's ``features`` (distinct indices into 0..F-1,
    at least one); None for None (all features)."""
    if features is None:
        return None
    f = np.asarray(features.cpu() if isinstance(features, torch.Tensor) else features)
    if f.dtype.kind not in "iu" or f.ndim != 1 or f.size < 1:
        raise ValueError("a job's features must be a 1-D sequence of integer column indices, at least one")
    f = f.astype(np.int64)
    if f.min() < 0 or f.max() >= F or np.unique(f).size != f.size:
        raise ValueError(f"a job's features must be distinct indices into 0..{F - 1}")
    return int(sum(1 << int(i) for i in f))


def forest_draws(n, F, n_trees, max_samples=1.0, max_features="sqrt", seed=0, bootstrap=False):
    """The row and feature subsets ``fit_forest`` trains tree t on, as
    [(rows_t, feats_t), ...] (None: all).  ``rng = np.random.default_rng(seed)``;
    for t = 0 .. n_trees-1 in order
    ``rows_t = np.sort(rng.choice(n, m, replace=False))`` with
    m = max(1, int(max_samples * n)) for a float or the integer itself, then
    ``feats_t = np.sort(rng.choice(F, k, replace=False))`` with k =
    max(1, int(sqrt(F))) for "sqrt", max(1, int(max_features * F)) for a
    float, the integer itself, F for None.  Both draws are always made; a draw
    of everything (m == n, k == F) is then reported as None.

    ``bootstrap=True`` draws the rows WITH replacement instead: in the same
    per-tree order, ``rows_t = np.bincount(rng.integers(0, n, m), minlength=n)``
    -- the (n,) counts of the draw, the tree's row weights, never None -- then
    the feature draw as above."""
    n, F, n_trees = int(n), int(F), int(n_trees)
    if n_trees < 1:
        raise ValueError("n_trees must be >= 1")

    def count(v, total, what):
        if isinstance(v, (float, np.floating)):
            if not 0.0 < v <= 1.0:
                raise ValueError(f"{what} as a fraction must be in (0, 1], got {v}")
            return max(1, int(v * total))
        c = int(v)
        if not 1 <= c <= total:
            raise ValueError(f"{what} must be 1..{total}, got {v}")
        return c

    m = count(max_samples, n, "max_samples")
    if max_features is None:
        k = F
    elif isinstance(max_features, str):
        if max_features != "sqrt":
            raise ValueError('max_features must be "sqrt", a fraction, a count or None')
        k = max(1, int(np.sqrt(F)))
    else:
        k = count(max_features, F, "max_features")
    rng = np.random.default_rng(seed)
    draws = []
    for _ in range(n_trees):
        if bootstrap:
            rows = np.bincount(rng.integers(0, n, m), minlength=n)
        else:
            rows = np.sort(rng.choice(n, m, replace=False))
        feats = np.sort(rng.choice(F, k, replace=False))
        draws.append((rows if bootstrap or m != n else None, None if k == F else feats))
    return draws


class TreeTrainer:
    """Exact Gini trees on the device, the reference's parameters as defaults."""

    def __init__(self, max_depth=25, min_samples_split=22, min_samples_leaf=20):
        self.max_depth, self.min_samples_split, self.min_samples_leaf = check_params(max_depth, min_samples_split,
                                                                                     min_samples_leaf)
        self.last_levels = None  # levels the last call ran (its deepest tree + 1)
        self.last_call_seconds = None  # host clock around the last vad_tree_train (it returns when the stream has run it)

    def fit(self, X, y, sample_weight=None, class_weight=None):
        """The tree of the rows; with ``sample_weight`` (integers (n,), >= 0)
        and / or ``class_weight`` ({class value: positive int}) the tree of
        sklearn's ``fit(X, y, sample_weight=sample_weight * class_weight[y])``."""
        job = (None, self.max_depth, self.min_samples_split, self.min_samples_leaf)
        if sample_weight is None and class_weight is None:
            return self.fit_many(X, y, [job])[0]
        Xc, yi, classes = check_rows(X, y)
        w = check_job_weights(row_weights(classes[yi], classes, sample_weight, class_weight), len(yi))
        tree = self.fit_many(Xc, yi, [job + (None, w)])[0]
        tree.classes_ = classes  # fit_many saw class indices
        return tree

    def fit_many(self, X, y, jobs, node_capacity=None):
        """One tree per job ``(rows, max_depth, min_samples_split,
        min_samples_leaf)`` or ``(rows, max_depth, min_samples_split,
        min_samples_leaf, features)``; ``rows``: indices into X without
        repeats, in any order, or None for all; ``features``: the distinct
        columns the job may split on, or None for all (the tree is the one of
        ``X[:, features]`` with its feature indices mapped back).
        A sixth element ``weights`` (after ``features``, which may be None)
        gives the job integer row weights (n,), 0 for a row that is not in the
        job; ``rows`` must then be None.  Jobs with and without weights mix: a
        job without gets ones on its rows.  A call in which no job has weights
        is the unweighted call.
        ``node_capacity`` (tests): nodes to provide per job instead of the
        bound that always suffices."""
        Xc, yi, classes = check_rows(X, y)
        n, F = (int(v) for v in Xc.shape)
        K = max(2, len(classes))
        if not jobs:
            return []
        params, row_sets, fmasks, weights = [], [], [], []
        for job in jobs:
            if len(job) not in (4, 5, 6):
                raise ValueError("a job is (rows, max_depth, min_samples_split, min_samples_leaf[, features[, weights]])")
            rows, md, mss, msl = job[:4]
            fmasks.append(feature_mask(job[4] if len(job) >= 5 else None, F))
            params.append(check_params(md, mss, msl))
            wj = job[5] if len(job) == 6 else None
            if wj is not None:
                if rows is not None:
                    raise ValueError("a job with weights takes rows=None: a weight of 0 leaves a row out")
                wj = check_job_weights(wj, n)
            weights.append(wj)
            if rows is not None:
                rows = np.asarray(rows.cpu() if isinstance(rows, torch.Tensor) else rows).astype(np.int64).ravel()
                if rows.size < 1 or rows.min() < 0 or rows.max() >= n or np.unique(rows).size != rows.size:
                    raise ValueError("a job's rows must be distinct indices into X, at least one")
            row_sets.append(rows)
        if not torch.cuda.is_available():
            raise RuntimeError("TreeTrainer needs the GPU: there is no CPU path")
        dev = Xc.device if isinstance(Xc, torch.Tensor) and Xc.is_cuda else torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(dev):
            Xd = Xc if isinstance(Xc, torch.Tensor) and Xc.is_cuda else torch.as_tensor(Xc).to(dev)
            yd = torch.from_numpy(yi).to(dev)
            order = torch.sort(Xd.t().contiguous(), dim=1, stable=True).indices.to(torch.int32).contiguous()
            J = len(jobs)
            weighted = any(wj is not None for wj in weights)
            mask = None
            if weighted or any(r is not None for r in row_sets):
                mask = torch.zeros((J, n), dtype=torch.uint8, device=dev)
                for j, r in enumerate(row_sets):
                    if weights[j] is not None:
                        mask[j] = torch.from_numpy(weights[j]).to(dev)
                    elif r is None:
                        mask[j] = 1
                    else:
                        mask[j, torch.from_numpy(r).to(dev)] = 1
            desc = (_Job * J)()
            for j, ((md, mss, msl), r) in enumerate(zip(params, row_sets)):
                nr = n if r is None else int(r.size)
                if weights[j] is not None:
                    nr = int(np.count_nonzero(weights[j]))
                cap = int(lib().vad_tree_train_node_capacity(nr, msl)) if node_capacity is None else int(node_capacity)
                desc[j] = _Job(nr, cap, md, mss, msl, 0)
            total = sum(int(d.node_capacity) for d in desc)
            ws_bytes = lib().vad_tree_train_weighted_workspace_bytes if weighted else lib().vad_tree_train_workspace_bytes
            need = int(ws_bytes(n, F, K, J, desc))
            if need == 0:
                raise ValueError("vad_tree_train refuses these sizes (include/vad_amd.h lists the limits)")
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            out = {k: torch.empty(J if k in ("n_nodes", "status") else total * (K if k == "value" else 1), dtype=dt,
                                  device=dev) for k, dt in _TABLES}
            tb = _Tables(*(out[k].data_ptr() for k, _ in _TABLES))
            levels = ctypes.c_int32(0)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fm = None
            if any(m is not None for m in fmasks):
                fm = (ctypes.c_uint64 * J)(*((1 << F) - 1 if m is None else m for m in fmasks))
            train = lib().vad_tree_train_weighted if weighted else lib().vad_tree_train_features
            rc = train(Xd.data_ptr(), yd.data_ptr(), n, F, K, order.data_ptr(),
                       None if mask is None else mask.data_ptr(), fm, J, desc, ctypes.byref(tb), ws.data_ptr(), need,
                       ctypes.byref(levels), stream_ptr())
            self.last_call_seconds = time.perf_counter() - t0
            if rc == VAD_ENOMEM:
                status = out["status"].cpu().numpy()
                raise VadError(f"vad_tree_train: node storage too small for jobs {np.flatnonzero(status & 1).tolist()}")
            check(rc, "vad_tree_train")
            self.last_levels = int(levels.value)
            host = {k: v.cpu().numpy() for k, v in out.items()}
        host["value"] = host["value"].reshape(total, K)
        trees, at = [], 0
        for j in range(J):
            m = int(host["n_nodes"][j])
            t = preorder({k: host[k][at:at + m] for k in _NODE_KEYS})
            at += int(desc[j].node_capacity)
            trees.append(TreeClassifier(*(t[k] for k in _NODE_KEYS[:6]), classes, F, n_node_samples=t["n_node_samples"],
                                        depth=t["depth"], value=t["value"][:, :max(len(classes), 1)]))
        return trees

    def fit_forest(self, X, y, n_trees, max_samples=1.0, max_features="sqrt", seed=0, bootstrap=False,
                   class_weight=None):
        """A ForestClassifier of ``n_trees`` trees with the trainer's three
        parameters, tree t on the rows and features of ``forest_draws`` (drawn
        on the host; WITHOUT replacement, or with ``bootstrap=True`` WITH, the
        counts of the draw as the tree's row weights), all in one ``fit_many``
        call.  ``class_weight`` ({class value: positive int}) is multiplied
        into every tree's weights."""
        from .forest import ForestClassifier
        Xc, yi, classes = check_rows(X, y)
        n, F = (int(v) for v in Xc.shape)
        cw = row_weights(classes[yi], classes, None, class_weight)
        draws = forest_draws(n, F, n_trees, max_samples, max_features, seed, bootstrap)
        p = (self.max_depth, self.min_samples_split, self.min_samples_leaf)
        jobs = []
        for r, f in draws:
            if not bootstrap and cw is None:
                jobs.append((r,) + p + (f,))
                continue
            if bootstrap:
                w = r.astype(np.int64)
            else:
                w = np.zeros(n, np.int64)
                w[slice(None) if r is None else r] = 1
            jobs.append((None,) + p + (f, check_job_weights(w if cw is None else w * cw, n)))
        trees = self.fit_many(Xc, yi, jobs)
        for t in trees:  # fit_many saw class indices
            t.classes_ = classes
        return ForestClassifier.from_trees(trees)

    def grid(self, X, y, max_depth, min_samples_split, min_samples_leaf, folds, sample_weight=None,
             class_weight=None):
        """Cross-validated accuracy of every (max_depth, min_samples_split,
        min_samples_leaf) over the caller's ``folds`` [(train_idx, test_idx),
        ...] (``kfold`` gives sklearn's).  One device job per (fold,
        min_samples_leaf), at the largest depth and the smallest
        min_samples_split; the other settings are pruned from it.  Returns a
        dict: "params" (list of dicts, in sklearn's ParameterGrid order),
        "mean_test_score", "best_index_", "best_params_", "best_score_" (the
        first maximum, as GridSearchCV ranks).  ``sample_weight`` /
        ``class_weight`` (as in ``fit``) weigh the training rows of every fold;
        the score stays plain accuracy.  Pruning still holds: ``max_depth``
        and ``min_samples_split`` act on distinct rows."""
        mds = [int(v) for v in np.atleast_1d(max_depth)]
        msss = [int(v) for v in np.atleast_1d(min_samples_split)]
        msls = [int(v) for v in np.atleast_1d(min_samples_leaf)]
        folds = [(np.asarray(a, np.int64), np.asarray(b, np.int64)) for a, b in folds]
        if not (mds and msss and msls and folds):
            raise ValueError("grid needs at least one value per parameter and one fold")
        Xc, yi, classes = check_rows(X, y)
        w = row_weights(classes[yi], classes, sample_weight, class_weight)
        if w is None:
            jobs = [(tr, max(mds), min(msss), msl) for tr, _ in folds for msl in msls]
        else:
            jobs = []
            for tr, _ in folds:
                if tr.size < 1 or tr.min() < 0 or tr.max() >= len(yi) or np.unique(tr).size != tr.size:
                    raise ValueError("a fold's training rows must be distinct indices into X, at least one")
                wf = np.zeros(len(yi), np.int64)
                wf[tr] = w[tr]
                wf = check_job_weights(wf, len(yi))
                jobs += [(None, max(mds), min(msss), msl, None, wf) for msl in msls]
        big = self.fit_many(Xc, yi, jobs)
        dev = torch.device("cuda", torch.cuda.current_device())
        Xd = Xc if isinstance(Xc, torch.Tensor) and Xc.is_cuda else torch.as_tensor(Xc).to(dev)
        yd = torch.from_numpy(yi).to(Xd.device)
        # fit_many saw class indices: its classes_ are the indices present
        params = [dict(max_depth=md, min_samples_leaf=msl, min_samples_split=mss)
                  for md in mds for msl in msls for mss in msss]
        score = np.zeros((len(params), len(folds)))
        for fi, (_, test) in enumerate(folds):
            ti = torch.from_numpy(test).to(Xd.device)
            xt, yt = Xd[ti].contiguous(), yd[ti]
            for pi, p in enumerate(params):
                tree = prune(big[fi * len(msls) + msls.index(p["min_samples_leaf"])], p["max_depth"],
                             p["min_samples_split"])
                got = torch.from_numpy(tree.classes_.astype(np.uint8)).to(Xd.device)[tree.predict_device(xt).long()]
                score[pi, fi] = float((got == yt).double().mean())
        mean = score.mean(axis=1)
        best = int(np.argmax(mean))
        return {"params": params, "mean_test_score": mean, "split_test_score": score, "best_index_": best,
                "best_params_": params[best], "best_score_": float(mean[best])}
