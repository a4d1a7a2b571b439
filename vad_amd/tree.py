"""Decision-tree classifier on the GPU (the classifier vad.py deploys:
learning/decision_classifier_trainer.py:26-35, an sklearn
``DecisionTreeClassifier(min_samples_split=22, max_depth=25,
min_samples_leaf=20)`` used through the ``predict`` protocol of
realtime_analysis/sklearn_analyser.py:71).

The tree is a flat node table (feature, threshold, left, right, leaf class)
walked by ``tree_kernel.hip`` with sklearn's rule: left iff
``float32(x[feature]) <= threshold``, a NaN feature following the node's
``missing_go_to_left`` (sklearn >= 1.3).  ``predict`` returns class *values*
(``classes_[index]``), like sklearn.  Tables are stored as ``.npz`` (arrays
only) -- a pickled sklearn estimator can be converted with ``from_sklearn``.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .plan import _out

_KEYS = ("feature", "threshold", "left", "right", "leaf", "nan_left", "classes")
_TRAIN_KEYS = ("n_node_samples", "depth", "value")  # optional: written by a trained tree only
_PROBA_KEYS = ("proba",)  # optional: written by a tree converted from sklearn


class TreePlan:
    """Device node table (include/vad_amd.h vad_tree_plan)."""

    def __init__(self, feature, threshold, left, right, leaf, nan_left, n_features):
        f = np.ascontiguousarray(feature, np.int32)
        t = np.ascontiguousarray(threshold, np.float64)
        lt = np.ascontiguousarray(left, np.int32)
        rt = np.ascontiguousarray(right, np.int32)
        lf = np.ascontiguousarray(leaf, np.int32)
        nl = np.ascontiguousarray(nan_left, np.uint8)
        n = f.shape[0]
        if not (t.shape == lt.shape == rt.shape == lf.shape == nl.shape == (n,)):
            raise ValueError("node arrays must have one entry per node")
        h = ctypes.c_void_p()
        check(lib().vad_tree_plan_create(n, f.ctypes.data, t.ctypes.data, lt.ctypes.data,
                                         rt.ctypes.data, lf.ctypes.data, nl.ctypes.data,
                                         int(n_features), ctypes.byref(h)), "vad_tree_plan_create")
        self._h = h
        self._destroy = lib().vad_tree_plan_destroy
        self.n_features = int(n_features)

    @property
    def handle(self):
        return self._h

    def set_scores(self, table):
        """The plan's score table (vad_tree_plan_set_scores): (n_classes,
        n_nodes) float32, row c the score of class index c per node; the
        scored hop entries read row ``active``."""
        t = np.ascontiguousarray(table, np.float32)
        if t.ndim != 2:
            raise ValueError("the score table must be (n_classes, n_nodes)")
        check(lib().vad_tree_plan_set_scores(self._h, t.ctypes.data, t.shape[0]), "vad_tree_plan_set_scores")
        self.score_classes = int(t.shape[0])

    def __del__(self):
        h = getattr(self, "_h", None)
        destroy = getattr(self, "_destroy", None)  # bound at creation: module globals
        if h is not None and h.value and destroy is not None:  # may be gone at exit
            destroy(h)
            self._h = None


class TreeClassifier:
    """GPU decision tree with the sklearn ``predict`` protocol."""

    def __init__(self, feature, threshold, left, right, leaf, nan_left, classes, n_features,
                 n_node_samples=None, depth=None, value=None, proba=None):
        self.nan_left = np.asarray(nan_left, np.uint8)
        self.feature = np.asarray(feature, np.int32)
        self.threshold = np.asarray(threshold, np.float64)
        self.left = np.asarray(left, np.int32)
        self.right = np.asarray(right, np.int32)
        self.leaf = np.asarray(leaf, np.int32)
        self.classes_ = np.asarray(classes)
        self.n_features = int(n_features)
        # what a trainer knows about its nodes (vad_amd.tree_train; None otherwise):
        # rows, depth and class counts (n_nodes, n_classes) per node
        self.n_node_samples = None if n_node_samples is None else np.asarray(n_node_samples, np.int32)
        self.depth = None if depth is None else np.asarray(depth, np.int32)
        self.value = None if value is None else np.asarray(value, np.int32)
        # sklearn's tree_.value per node, (n_nodes, n_classes) float64 (from_sklearn; None
        # otherwise): class fractions or weighted counts, what predict_proba normalises
        self.proba = None if proba is None else np.asarray(proba, np.float64)
        self._plan = None

    # -- construction ----------------------------------------------------
    @classmethod
    def from_sklearn(cls, clf):
        """From a fitted sklearn DecisionTreeClassifier (single output)."""
        t = clf.tree_
        value = np.asarray(t.value)
        if value.ndim == 3:
            if value.shape[1] != 1:
                raise ValueError("multi-output trees are not supported")
            value = value[:, 0, :]
        leaf = np.argmax(value, axis=1)  # sklearn predict: classes_[argmax(proba)], first max
        feature = np.where(np.asarray(t.children_left) < 0, -1, np.asarray(t.feature))
        nan_left = np.asarray(getattr(t, "missing_go_to_left", np.zeros(t.node_count, np.uint8)))
        return cls(feature, t.threshold, t.children_left, t.children_right, leaf, nan_left,
                   clf.classes_, t.n_features, proba=value)

    @staticmethod
    def looks_like_sklearn_tree(obj):
        t = getattr(obj, "tree_", None)
        return (t is not None and hasattr(obj, "classes_") and hasattr(t, "children_left")
                and hasattr(t, "threshold") and hasattr(t, "feature") and hasattr(t, "value"))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            extra = {k: z[k] for k in _TRAIN_KEYS + _PROBA_KEYS if k in z.files}
            return cls(*(z[k] for k in _KEYS), int(z["n_features"]), **extra)

    def save(self, path):
        np.savez(path, feature=self.feature, threshold=self.threshold, left=self.left,
                 right=self.right, leaf=self.leaf, nan_left=self.nan_left, classes=self.classes_,
                 n_features=np.int64(self.n_features),
                 **{k: getattr(self, k) for k in _TRAIN_KEYS + _PROBA_KEYS if getattr(self, k) is not None})

    @property
    def plan(self) -> TreePlan:
        if self._plan is None:
            self._plan = TreePlan(self.feature, self.threshold, self.left, self.right, self.leaf,
                                  self.nan_left, self.n_features)
        return self._plan

    @property
    def in_dim(self):
        return self.n_features

    # -- scores ------------------------------------------------------------
    def score_table(self, active=1):
        """float32 (n_nodes,): the share of class index ``active`` among a
        node's training rows, by sklearn's predict_proba formula in float64
        (value / value.sum(), a zero sum taken as 1) rounded once to float32.
        From ``proba`` (a tree converted from sklearn) or the integer class
        counts ``value`` (a tree trained here); ValueError with neither."""
        v = self.proba if self.proba is not None else self.value
        if v is None:
            raise ValueError("the tree has neither sklearn's node values (proba) nor class counts (value): "
                             "convert it again with from_sklearn, or train it with vad_amd.tree_train")
        v = np.asarray(v, np.float64)
        if v.ndim != 2 or v.shape[0] != self.feature.shape[0]:
            raise ValueError("node values must be (n_nodes, n_classes)")
        if not 0 <= int(active) < v.shape[1]:
            raise ValueError(f"active must be a class index below {v.shape[1]}, got {active}")
        norm = v.sum(axis=1)
        norm[norm == 0.0] = 1.0
        return np.ascontiguousarray((v[:, int(active)] / norm).astype(np.float32))

    def score_classes(self):
        """Number of classes score_table() knows; ValueError without node values."""
        v = self.proba if self.proba is not None else self.value
        if v is None:
            self.score_table(0)  # raises with the reason
        return int(np.asarray(v).shape[1])

    def plan_with_scores(self):
        """``plan`` with every class's score_table() set on it (once), as the
        scored streaming entries need it."""
        p = self.plan
        if getattr(p, "score_classes", 0) == 0:
            p.set_scores(np.stack([self.score_table(c) for c in range(self.score_classes())]))
        return p

    def window_scores(self, mfcc, mode=_lib.FEAT_ANALYSER, active=1, out=None, stream=None):
        """Scores (float32, device) of every 5-frame window of an MFCC sequence
        (vad_amd.scores.tree_window_scores)."""
        from .scores import tree_window_scores
        return tree_window_scores(self, mfcc, mode, active, out=out, stream=stream)

    # -- inference --------------------------------------------------------
    def predict_device(self, x, out=None, stream=None):
        """Class indices (uint8, device) of device feature rows x (n, n_features) fp32."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
            raise TypeError("x must be a CUDA float32 tensor")
        x = x.contiguous().reshape(-1, self.n_features)  # kept alive until the launch is queued
        n = x.shape[0]
        out = _out(out, (n,), torch.uint8, x.device)
        check(lib().vad_tree_predict(self.plan.handle, ptr(x), n, ptr(out), stream_ptr(stream)),
              "vad_tree_predict")
        _keep_for_stream(x, stream)
        return out

    def predict(self, X):
        """sklearn's predict: class values of feature rows X (n, n_features) or (n_features,)."""
        x = np.asarray(X, dtype=np.float32).reshape(-1, self.n_features)
        idx = self.predict_device(torch.from_numpy(np.ascontiguousarray(x)).cuda())
        return self.classes_[idx.cpu().numpy().astype(np.int64)]

    def window_labels(self, mfcc, mode=_lib.FEAT_ANALYSER, out=None, stream=None):
        """Class indices (uint8, device) of every 5-frame window of an MFCC sequence."""
        if not (isinstance(mfcc, torch.Tensor) and mfcc.is_cuda and mfcc.dtype == torch.float32):
            raise TypeError("mfcc must be a CUDA float32 tensor")
        f, c = mfcc.shape
        rows = max(f - 5, 0)
        out = _out(out, (rows,), torch.uint8, mfcc.device)
        m = mfcc.contiguous()  # a temporary copy must outlive the asynchronous kernel
        check(lib().vad_features_tree(self.plan.handle, ptr(m), f, c, int(mode),
                                      ptr(out), stream_ptr(stream)), "vad_features_tree")
        _keep_for_stream(m, stream)
        return out


def _keep_for_stream(t, stream):
    """A tensor read by a kernel queued on `stream` (not the current stream)
    must not be recycled by the caching allocator for current-stream work
    before that kernel ran."""
    if stream is not None and stream != torch.cuda.current_stream(t.device):
        t.record_stream(stream)
