"""Random forests on the GPU: T decision trees in one node table, their leaf
class shares averaged by ``csrc/forest_kernel.hip``.

The result is sklearn's ``predict_proba`` / ``predict`` with ``n_jobs=1``
(``RandomForestClassifier``, ``ExtraTreesClassifier``, ``BaggingClassifier``
over decision trees).  Per row, K double accumulators start at 0; for
t = 0 .. T-1 in order ``acc[k] += proba[leaf_t][k]``; then ``acc[k] /= T``.
The score is ``float32(acc[active])``, the label the first maximum of ``acc``
as an index into ``classes_``.  The walk is the tree's (vad_amd.tree): float32
feature, float64 threshold, a NaN feature following ``nan_left``.

    forest = TreeTrainer().fit_forest(X, y, n_trees=16)      # trained here
    forest = ForestClassifier.from_sklearn(fitted_estimator)  # or converted
    VadPipeline(forest).scores(audio)

The table is ``TreeClassifier``'s field layout with the trees one after
another: tree t is the nodes ``roots[t] : roots[t + 1]``, its root first, the
child indices absolute.  ``proba`` is (n_nodes, K) float64, what sklearn's
``predict_proba`` of one tree returns for a row that ends in the node: a
node's ``value`` row divided by its sum in double -- or the row itself where
it already is a row of shares (sklearn >= 1.4 stores fractions and returns
them untouched, and so are they kept here, bit for bit).  Tables are stored as
``.npz`` (arrays only).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .plan import _out, check_out
from .tree import TreeClassifier, _keep_for_stream

MAX_CLASSES = 8
_KEYS = ("feature", "threshold", "left", "right", "leaf", "nan_left", "roots", "proba", "classes")


def node_shares(value):
    """(n_nodes, K) float64 class shares of node values: ``value / value.sum``
    in double (a zero sum taken as 1); rows that already sum to 1 within 1e-9
    are shares as they stand and are returned untouched."""
    v = np.array(value, dtype=np.float64)
    if v.ndim != 2:
        raise ValueError("node values must be (n_nodes, n_classes)")
    norm = v.sum(axis=1)
    norm[norm == 0.0] = 1.0
    if np.all(np.abs(norm - 1.0) <= 1e-9):
        return v
    return v / norm[:, None]


class ForestPlan:
    """Device tables of a forest (include/vad_amd.h vad_forest)."""

    def __init__(self, forest):
        n = forest.feature.shape[0]
        arr = [np.ascontiguousarray(forest.feature, np.int32), np.ascontiguousarray(forest.threshold, np.float64),
               np.ascontiguousarray(forest.left, np.int32), np.ascontiguousarray(forest.right, np.int32),
               np.ascontiguousarray(forest.nan_left, np.uint8)]
        roots = np.ascontiguousarray(forest.roots, np.int32)
        proba = np.ascontiguousarray(forest.proba, np.float64)
        h = ctypes.c_void_p()
        check(lib().vad_forest_create(n, *(a.ctypes.data for a in arr), roots.shape[0], roots.ctypes.data,
                                      proba.shape[1], proba.ctypes.data, forest.n_features, ctypes.byref(h)),
              "vad_forest_create")
        self._h = h
        self._destroy = lib().vad_forest_destroy

    @property
    def handle(self):
        return self._h

    def __del__(self):
        h = getattr(self, "_h", None)
        destroy = getattr(self, "_destroy", None)
        if h is not None and h.value and destroy is not None:
            destroy(h)
            self._h = None


class ForestClassifier:
    """GPU random forest with the sklearn ``predict`` protocol."""

    def __init__(self, feature, threshold, left, right, leaf, nan_left, roots, proba, classes, n_features):
        self.feature = np.asarray(feature, np.int32)
        self.threshold = np.asarray(threshold, np.float64)
        self.left = np.asarray(left, np.int32)
        self.right = np.asarray(right, np.int32)
        self.leaf = np.asarray(leaf, np.int32)
        self.nan_left = np.asarray(nan_left, np.uint8)
        self.roots = np.asarray(roots, np.int32).reshape(-1)
        self.proba = np.asarray(proba, np.float64)
        self.classes_ = np.asarray(classes)
        self.n_features = int(n_features)
        n = self.feature.shape[0]
        if not (self.threshold.shape == self.left.shape == self.right.shape == self.leaf.shape
                == self.nan_left.shape == (n,)) or n < 1:
            raise ValueError("node arrays must have one entry per node, at least one")
        K = len(self.classes_)
        if not 1 <= K <= MAX_CLASSES:
            raise ValueError(f"1 to {MAX_CLASSES} classes, got {K}")
        if self.proba.shape != (n, K):
            raise ValueError(f"proba must be (n_nodes, n_classes) = {(n, K)}, got {self.proba.shape}")
        r = self.roots
        if r.size < 1 or r[0] != 0 or (np.diff(r) <= 0).any() or r[-1] >= n:
            raise ValueError("roots must start at 0, ascend and lie inside the table")
        self._plan = None

    # -- construction ----------------------------------------------------
    @classmethod
    def from_trees(cls, trees):
        """The forest of a list of TreeClassifier (trained here or converted),
        in the list's order: same ``n_features``, same classes."""
        trees = list(trees)
        if not trees:
            raise ValueError("a forest needs at least one tree")
        first = trees[0]
        cols = {k: [] for k in ("feature", "threshold", "left", "right", "leaf", "nan_left", "proba")}
        roots, at = [], 0
        for t in trees:
            if not isinstance(t, TreeClassifier):
                raise TypeError("from_trees takes TreeClassifier objects")
            if t.n_features != first.n_features or not np.array_equal(t.classes_, first.classes_):
                raise ValueError("every tree of a forest must have the same n_features and classes")
            v = t.proba if t.proba is not None else t.value
            if v is None:
                raise ValueError("a tree has neither sklearn's node values (proba) nor class counts (value)")
            if np.asarray(v).shape != (t.feature.shape[0], len(first.classes_)):
                raise ValueError("a tree's node values must be (n_nodes, n_classes)")
            inner = t.left >= 0
            roots.append(at)
            cols["feature"].append(t.feature)
            cols["threshold"].append(t.threshold)
            cols["left"].append(np.where(inner, t.left + at, -1))
            cols["right"].append(np.where(inner, t.right + at, -1))
            cols["leaf"].append(t.leaf)
            cols["nan_left"].append(t.nan_left)
            cols["proba"].append(node_shares(v))
            at += t.feature.shape[0]
        c = {k: np.concatenate(v) for k, v in cols.items()}
        return cls(c["feature"], c["threshold"], c["left"], c["right"], c["leaf"], c["nan_left"], roots, c["proba"],
                   first.classes_, first.n_features)

    @staticmethod
    def looks_like_sklearn_forest(obj):
        est = getattr(obj, "estimators_", None)
        return (est is not None and hasattr(obj, "classes_") and len(est) > 0
                and all(TreeClassifier.looks_like_sklearn_tree(e) for e in est))

    @classmethod
    def from_sklearn(cls, obj):
        """From a fitted RandomForestClassifier, ExtraTreesClassifier or
        BaggingClassifier over DecisionTreeClassifier (single output).  A
        bagged tree's features (``estimators_features_``) are mapped back to
        the columns of the full row, and a tree that saw fewer classes gets
        zero shares for the others, as sklearn adds them."""
        if not cls.looks_like_sklearn_forest(obj):
            raise TypeError("from_sklearn takes a fitted forest or bagging of sklearn decision trees")
        classes = np.asarray(obj.classes_)
        if classes.ndim != 1:
            raise ValueError("multi-output forests are not supported")
        K, F = len(classes), int(obj.n_features_in_)
        feats = getattr(obj, "estimators_features_", None)
        trees = []
        for i, est in enumerate(obj.estimators_):
            t = TreeClassifier.from_sklearn(est)
            if feats is not None:
                cols = np.asarray(feats[i], np.int64)
                t.feature = np.where(t.feature >= 0, cols[np.maximum(t.feature, 0)], -1).astype(np.int32)
            if t.proba.shape[1] != K:  # bagging: est.classes_ are indices into the ensemble's classes
                full = np.zeros((t.proba.shape[0], K))
                full[:, np.asarray(est.classes_).astype(np.int64)] = node_shares(t.proba)
                t.proba = full
                t.leaf = np.argmax(full, axis=1).astype(np.int32)
            t.classes_, t.n_features = classes, F
            trees.append(t)
        return cls.from_trees(trees)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(*(z[k] for k in _KEYS), int(z["n_features"]))

    def save(self, path):
        np.savez(path, feature=self.feature, threshold=self.threshold, left=self.left, right=self.right,
                 leaf=self.leaf, nan_left=self.nan_left, roots=self.roots, proba=self.proba, classes=self.classes_,
                 n_features=np.int64(self.n_features))

    # -- shape -------------------------------------------------------------
    @property
    def n_trees(self):
        return int(self.roots.shape[0])

    @property
    def in_dim(self):
        return self.n_features

    @property
    def plan(self) -> ForestPlan:
        if self._plan is None:
            self._plan = ForestPlan(self)
        return self._plan

    def _active(self, active):
        if not 0 <= int(active) < len(self.classes_):
            raise ValueError(f"active must be a class index below {len(self.classes_)}, got {active}")
        return int(active)

    # -- inference --------------------------------------------------------
    def _rows(self, x, active, labels, scores, stream):
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
            raise TypeError("x must be a CUDA float32 tensor")
        x = x.contiguous().reshape(-1, self.n_features)
        n = x.shape[0]
        labels = _out(labels, (n,), torch.uint8, x.device)
        if scores is not False:
            if scores is None:
                scores = torch.empty((n,), dtype=torch.float32, device=x.device)
            else:
                check_out(scores, (n,), torch.float32, x.device, "out")
        check(lib().vad_forest_predict(self.plan.handle, ptr(x), n, self._active(active), ptr(labels),
                                       ptr(scores) if scores is not False else None, stream_ptr(stream)),
              "vad_forest_predict")
        _keep_for_stream(x, stream)
        return labels, scores

    def predict_device(self, x, out=None, stream=None):
        """Class indices (uint8, device) of device feature rows x (n, n_features) fp32."""
        return self._rows(x, 0, out, False, stream)[0]

    def predict_scores(self, x, active=1, out=None, stream=None):
        """float32(predict_proba(x)[:, active]) of device feature rows (float32, device)."""
        return self._rows(x, active, None, out, stream)[1]

    def predict(self, X):
        """sklearn's predict: class values of feature rows X (n, n_features) or (n_features,)."""
        x = np.asarray(X, dtype=np.float32).reshape(-1, self.n_features)
        idx = self.predict_device(torch.from_numpy(np.ascontiguousarray(x)).cuda())
        return self.classes_[idx.cpu().numpy().astype(np.int64)]

    def _windows(self, mfcc, mode, active, labels, scores, stream):
        if not (isinstance(mfcc, torch.Tensor) and mfcc.is_cuda and mfcc.dtype == torch.float32 and mfcc.dim() == 2):
            raise TypeError("mfcc must be a 2-D CUDA float32 tensor")
        f, c = mfcc.shape
        rows = max(f - 5, 0)
        labels = _out(labels, (rows,), torch.uint8, mfcc.device)
        if scores is not False:
            if scores is None:
                scores = torch.empty((rows,), dtype=torch.float32, device=mfcc.device)
            else:
                check_out(scores, (rows,), torch.float32, mfcc.device, "out")
        m = mfcc.contiguous()  # a temporary copy must outlive the asynchronous kernel
        check(lib().vad_features_forest(self.plan.handle, ptr(m), f, c, int(mode), self._active(active), ptr(labels),
                                        ptr(scores) if scores is not False else None, stream_ptr(stream)),
              "vad_features_forest")
        _keep_for_stream(m, stream)
        return labels, scores

    def window_labels(self, mfcc, mode=_lib.FEAT_ANALYSER, out=None, stream=None):
        """Class indices (uint8, device) of every 5-frame window of an MFCC sequence."""
        return self._windows(mfcc, mode, 0, out, False, stream)[0]

    def window_scores(self, mfcc, mode=_lib.FEAT_ANALYSER, active=1, out=None, stream=None):
        """Scores (float32, device) of every 5-frame window of an MFCC sequence."""
        return self._windows(mfcc, mode, active, None, out, stream)[1]
