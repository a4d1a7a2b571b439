"""Speech scores, decisions made from them and their scoring against a
reference, all on the device (include/vad_amd.h, "Speech scores").

The classifiers end in a hard label.  Here a window gets a score in [0, 1]
(VadPipeline.scores: the softmax of the FFN's logits or the class fraction of
the tree's leaf); labels are decided from the scores with an onset and an
offset threshold (score_labels) and padded (dilate_labels), and the segment
stage takes those labels as it takes the classifiers'.  To choose the
thresholds, reference_labels turns the speech intervals of a transcript into
per-window ground truth and roc() draws misses against false alarms from one
histogram of the scores.  No call here synchronises except roc().
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .plan import check_out
from .segments import _check_labels, _overlaps

Roc = namedtuple("Roc", "thresholds tpr fpr")


def _check_scores(scores, name="scores"):
    if not isinstance(scores, torch.Tensor):
        raise TypeError(f"{name} must be a CUDA (HIP) torch tensor")
    if scores.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {scores.dtype}")
    if not scores.is_cuda:
        raise TypeError(f"{name} must be a CUDA (HIP) torch tensor")
    if scores.dim() != 1 or not scores.is_contiguous():
        raise ValueError(f"{name} must be a contiguous 1-D tensor")
    return scores


def _check_thresholds(on, off):
    if off is None:
        off = on
    on, off = float(on), float(off)
    if not 0.0 <= off <= on <= 1.0:  # NaN fails too
        raise ValueError(f"thresholds need 0 <= off <= on <= 1, got on={on}, off={off}")
    return on, off


def _check_pad(pad):
    try:
        before, after = pad
    except (TypeError, ValueError):
        raise TypeError("pad must be a pair (pad_before, pad_after) of windows") from None
    before, after = int(before), int(after)
    if before < 0 or after < 0:
        raise ValueError("pad must be >= 0")
    return before, after


def _out_u8(out, like, n, name):
    if out is None:
        return torch.empty((n,), dtype=torch.uint8, device=like.device)
    check_out(out, (n,), torch.uint8, like.device, "out")
    if _overlaps(out, like):
        raise ValueError(f"out must not alias {name}")
    return out


def workspace(n, device, stream=None):
    """A device workspace for the scans over n windows (vad_scores_workspace_bytes)."""
    need = int(_lib.lib().vad_scores_workspace_bytes(int(n)))
    s = stream if stream is not None else torch.cuda.current_stream(device)
    with torch.cuda.stream(s):
        return torch.empty((max(need, 16),), dtype=torch.uint8, device=device)


def _check_ws(ws, n, device, stream):
    if ws is None:
        return workspace(n, device, stream)
    if not (isinstance(ws, torch.Tensor) and ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous()):
        raise TypeError("ws must be a contiguous uint8 CUDA (HIP) tensor")
    if ws.device != device:
        raise ValueError(f"ws is on {ws.device}, the input on {device}")
    if ws.numel() < int(_lib.lib().vad_scores_workspace_bytes(int(n))):
        raise ValueError("ws is smaller than vad_scores_workspace_bytes(n)")
    return ws


# ----------------------------------------------------------------------------
# Scores
# ----------------------------------------------------------------------------
def scores_from_logits(logits, active=1, out=None, stream=None):
    """s = 1 / (1 + sum_{j != active} expf(z_j - z_active)) of every row of an
    (n, n_classes) float32 device tensor of logits, n_classes <= 8; a row with
    a non-finite logit scores 0."""
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda):
        raise TypeError("logits must be a CUDA (HIP) torch tensor")
    if logits.dtype != torch.float32:
        raise TypeError(f"logits must be float32, got {logits.dtype}")
    if logits.dim() != 2 or not logits.is_contiguous():
        raise ValueError("logits must be a contiguous (n, n_classes) tensor")
    n, c = logits.shape
    if not 1 <= c <= _lib.SCORE_MAX_CLASSES:
        raise ValueError(f"1 to {_lib.SCORE_MAX_CLASSES} classes, got {c}")
    if not 0 <= int(active) < c:
        raise ValueError(f"active must be a class index below {c}, got {active}")
    if out is None:
        out = torch.empty((n,), dtype=torch.float32, device=logits.device)
    else:
        check_out(out, (n,), torch.float32, logits.device, "out")
        if _overlaps(out, logits):
            raise ValueError("out must not alias logits")
    _lib.check(_lib.lib().vad_scores_from_logits(_lib.ptr(logits), n, c, int(active), _lib.ptr(out),
                                                 _lib.stream_ptr(stream)), "vad_scores_from_logits")
    return out


def _node_scores(tree, active, device):
    """The tree's score table on `device` (cached on the classifier)."""
    cache = tree.__dict__.setdefault("_score_tables", {})
    key = (int(active), str(device))
    t = cache.get(key)
    if t is None:
        t = cache[key] = torch.from_numpy(tree.score_table(active)).to(device)
    return t


def tree_window_scores(tree, mfcc, mode=_lib.FEAT_ANALYSER, active=1, out=None, stream=None):
    """Scores of every 5-frame window of an (F, n) MFCC sequence from a
    TreeClassifier: TreeClassifier.window_labels' walk, ending in
    score_table(active)[leaf]."""
    if not (isinstance(mfcc, torch.Tensor) and mfcc.is_cuda and mfcc.dtype == torch.float32 and mfcc.dim() == 2):
        raise TypeError("mfcc must be a 2-D CUDA float32 tensor")
    table = _node_scores(tree, active, mfcc.device)
    f, c = mfcc.shape
    rows = max(f - 5, 0)
    if out is None:
        out = torch.empty((rows,), dtype=torch.float32, device=mfcc.device)
    else:
        check_out(out, (rows,), torch.float32, mfcc.device, "out")
    m = mfcc.contiguous()
    if _overlaps(out, m):
        raise ValueError("out must not alias mfcc")
    _lib.check(_lib.lib().vad_features_tree_scores(tree.plan.handle, _lib.ptr(table), _lib.ptr(m), f, c, int(mode),
                                                   _lib.ptr(out), _lib.stream_ptr(stream)),
               "vad_features_tree_scores")
    _keep(m, stream)
    return out


def tree_predict_scores(tree, x, active=1, out=None, stream=None):
    """Scores of device feature rows x (n, n_features) float32 from a
    TreeClassifier: float32(predict_proba(x)[:, active]) of the sklearn tree
    it was made from."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
        raise TypeError("x must be a CUDA float32 tensor")
    table = _node_scores(tree, active, x.device)
    x = x.contiguous().reshape(-1, tree.n_features)
    n = x.shape[0]
    if out is None:
        out = torch.empty((n,), dtype=torch.float32, device=x.device)
    else:
        check_out(out, (n,), torch.float32, x.device, "out")
        if _overlaps(out, x):
            raise ValueError("out must not alias x")
    _lib.check(_lib.lib().vad_tree_predict_scores(tree.plan.handle, _lib.ptr(table), _lib.ptr(x), n, _lib.ptr(out),
                                                  _lib.stream_ptr(stream)), "vad_tree_predict_scores")
    _keep(x, stream)
    return out


def _keep(t, stream):
    if stream is not None and stream != torch.cuda.current_stream(t.device):
        t.record_stream(stream)


class BatchScores:
    """The scores of a batch: ``scores`` is the global (G - 5,) float32 tensor
    over the packed buffer's windows; ``[k]`` is the view of clip k's
    n_rows[k] scores (as vad_amd.batch.BatchLabels)."""

    def __init__(self, scores, batch):
        self.scores = scores
        self.batch = batch

    def __len__(self):
        return self.batch.n_clips

    def __getitem__(self, k):
        if not -self.batch.n_clips <= k < self.batch.n_clips:
            raise IndexError(k)
        f0 = int(self.batch.host["frame0"][k])
        return self.scores[f0:f0 + int(self.batch.host["n_rows"][k])]


# ----------------------------------------------------------------------------
# Decisions
# ----------------------------------------------------------------------------
def score_labels(scores, on, off=None, out=None, stream=None, ws=None):
    """uint8 0/1 labels by hysteresis: 1 from a window with s >= on until one
    with s < off (or NaN), 0 before the first.  off defaults to on (a plain
    threshold).  0 <= off <= on <= 1."""
    _check_scores(scores)
    on, off = _check_thresholds(on, off)
    n = scores.numel()
    out = _out_u8(out, scores, n, "scores")
    ws = _check_ws(ws, n, scores.device, stream)
    _lib.check(_lib.lib().vad_score_labels(_lib.ptr(scores), n, on, off, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                           _lib.stream_ptr(stream)), "vad_score_labels")
    return out


def dilate_labels(labels, pad=(0, 0), active=1, out=None, stream=None, ws=None):
    """uint8 0/1 labels with every run of labels == active grown by pad[0]
    windows at its start and pad[1] at its end (cut at the array's ends)."""
    _check_labels(labels)
    before, after = _check_pad(pad)
    if not 0 <= int(active) <= 255:
        raise ValueError("active must be a uint8 value")
    n = labels.numel()
    out = _out_u8(out, labels, n, "labels")
    ws = _check_ws(ws, n, labels.device, stream)
    _lib.check(_lib.lib().vad_label_dilate(_lib.ptr(labels), n, int(active), before, after, _lib.ptr(out),
                                           _lib.ptr(ws), ws.numel(), _lib.stream_ptr(stream)), "vad_label_dilate")
    return out


def _batch_tensor(x, batch, attr, check):
    x = getattr(x, attr, x)  # a BatchScores / BatchLabels, or a caller-made tensor
    check(x)
    if x.numel() != batch.n_windows:
        raise ValueError(f"the batch has {batch.n_windows} global windows, the input has {x.numel()}")
    return x


def batch_score_labels(scores, batch, on, off=None, out=None, stream=None, ws=None):
    """score_labels over the global window array of a ClipBatch, every clip a
    sequence of its own (the state is 0 at a clip's first window); 0 for the
    windows of no clip.  scores: a BatchScores or a (batch.n_windows,) tensor."""
    scores = _batch_tensor(scores, batch, "scores", _check_scores)
    on, off = _check_thresholds(on, off)
    n = scores.numel()
    out = _out_u8(out, scores, n, "scores")
    ws = _check_ws(ws, n, scores.device, stream)
    _lib.check(_lib.lib().vad_batch_score_labels(
        _lib.ptr(scores), n, _lib.ptr(batch.d_frame0), _lib.ptr(batch.d_n_rows), batch.n_clips, on, off,
        _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(stream)), "vad_batch_score_labels")
    return out


def batch_dilate_labels(labels, batch, pad=(0, 0), active=1, out=None, stream=None, ws=None):
    """dilate_labels over the global window array of a ClipBatch; padding
    stops at every clip's first and last window."""
    labels = _batch_tensor(labels, batch, "labels", _check_labels)
    before, after = _check_pad(pad)
    if not 0 <= int(active) <= 255:
        raise ValueError("active must be a uint8 value")
    n = labels.numel()
    out = _out_u8(out, labels, n, "labels")
    ws = _check_ws(ws, n, labels.device, stream)
    _lib.check(_lib.lib().vad_batch_label_dilate(
        _lib.ptr(labels), n, _lib.ptr(batch.d_frame0), _lib.ptr(batch.d_n_rows), batch.n_clips, int(active), before,
        after, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(stream)), "vad_batch_label_dilate")
    return out


# ----------------------------------------------------------------------------
# Scoring against a reference
# ----------------------------------------------------------------------------
def _intervals(intervals, rate):
    """(k, 2) int64 [start, end) in samples from an STM transcript path, a
    (starts, ends) pair or a (k, 2) array."""
    if isinstance(intervals, (str, bytes)) or hasattr(intervals, "__fspath__"):
        from .dataset import get_samples_indices
        intervals = get_samples_indices(intervals, rate)
    if isinstance(intervals, tuple) and len(intervals) == 2:
        intervals = np.stack([np.asarray(intervals[0]), np.asarray(intervals[1])], axis=1)
    if isinstance(intervals, torch.Tensor):
        return intervals
    iv = np.asarray(intervals)
    if iv.size == 0:
        iv = iv.reshape(0, 2)
    if iv.ndim != 2 or iv.shape[1] != 2 or iv.dtype.kind not in "iu":
        raise ValueError("intervals must be (k, 2) integers: [start, end) in samples")
    iv = iv.astype(np.int64)
    if (iv[:, 1] < iv[:, 0]).any() or (iv[1:, 0] < iv[:-1, 1]).any():
        raise ValueError("intervals must be ascending and disjoint")
    return iv


def reference_labels(intervals, n, frame_size=400, hop=160, rate=16000, device=None, out=None, stream=None):
    """Per-window ground truth from speech intervals: uint8 (n,), window i is 1
    iff its centre sample (i + 2) * hop + frame_size // 2 lies in an interval.
    intervals: (k, 2) integers [start, end) in samples, ascending and disjoint
    (host array, or an int64 device tensor taken as it is), the (starts, ends)
    of vad_amd.dataset.get_samples_indices, or the path of an STM transcript,
    read at ``rate`` samples per second."""
    if int(n) < 0:
        raise ValueError("n must be >= 0")
    if frame_size <= 0 or hop <= 0:
        raise ValueError("frame_size and hop must be positive")
    iv = _intervals(intervals, rate)
    if isinstance(iv, torch.Tensor):
        if not (iv.is_cuda and iv.dtype == torch.int64 and iv.is_contiguous() and iv.dim() == 2 and iv.shape[1] == 2):
            raise TypeError("device intervals must be a contiguous (k, 2) int64 CUDA (HIP) tensor")
        device = iv.device
    else:
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        iv = torch.from_numpy(np.ascontiguousarray(iv)).to(device)
    if out is None:
        out = torch.empty((int(n),), dtype=torch.uint8, device=device)
    else:
        check_out(out, (int(n),), torch.uint8, device, "out")
    _lib.check(_lib.lib().vad_reference_labels(_lib.ptr(iv), iv.shape[0], int(n), int(frame_size), int(hop),
                                               _lib.ptr(out), _lib.stream_ptr(stream)), "vad_reference_labels")
    _keep(iv, stream)
    return out


def batch_reference_labels(intervals, batch, out=None, stream=None):
    """reference_labels for every clip of a ClipBatch over its global window
    array.  intervals: one entry per clip, each as reference_labels takes it
    on the host (samples of the clip itself).  0 for the windows of no clip."""
    if len(intervals) != batch.n_clips:
        raise ValueError(f"the batch has {batch.n_clips} clips, intervals has {len(intervals)} entries")
    per = [_intervals(iv, None) for iv in intervals]
    if any(isinstance(iv, torch.Tensor) for iv in per):
        raise TypeError("batch intervals are host arrays")
    rows = np.concatenate([np.concatenate([np.full((len(iv), 1), k, np.int64), iv], axis=1)
                           for k, iv in enumerate(per)] + [np.zeros((0, 3), np.int64)])
    row0 = np.concatenate(([0], np.cumsum([len(iv) for iv in per])))[:batch.n_clips].astype(np.int64)
    device = batch.d_frame0.device
    d_rows = torch.from_numpy(np.ascontiguousarray(rows)).to(device)
    d_row0 = torch.from_numpy(row0).to(device)
    n = batch.n_windows
    if out is None:
        out = torch.empty((n,), dtype=torch.uint8, device=device)
    else:
        check_out(out, (n,), torch.uint8, device, "out")
    _lib.check(_lib.lib().vad_batch_reference_labels(
        _lib.ptr(d_rows), d_rows.shape[0], _lib.ptr(d_row0), _lib.ptr(batch.d_frame0), _lib.ptr(batch.d_n_rows),
        batch.n_clips, n, batch.frame_size, batch.hop, _lib.ptr(out), _lib.stream_ptr(stream)),
        "vad_batch_reference_labels")
    _keep(d_rows, stream)
    _keep(d_row0, stream)
    return out


def _check_ref(ref, x):
    _check_labels(ref)
    if ref.numel() != x.numel() or ref.device != x.device:
        raise ValueError("ref must have one entry per window, on the same device")
    return ref


def histogram(scores, ref, bins=1024, stream=None):
    """(2, bins) int64 device tensor: [r, b] = windows with ref == r (0 / 1)
    and b = min(int(s * bins), bins - 1); NaN scores fall in bin 0."""
    _check_scores(scores)
    _check_ref(ref, scores)
    if not 1 <= int(bins) <= _lib.SCORE_MAX_BINS:
        raise ValueError(f"bins must be 1 .. {_lib.SCORE_MAX_BINS}, got {bins}")
    s = stream if stream is not None else torch.cuda.current_stream(scores.device)
    with torch.cuda.stream(s):
        hist = torch.zeros((2, int(bins)), dtype=torch.int64, device=scores.device)
    _lib.check(_lib.lib().vad_score_histogram_f32(_lib.ptr(scores), _lib.ptr(ref), scores.numel(), int(bins),
                                                  _lib.ptr(hist), _lib.stream_ptr(stream)),
               "vad_score_histogram_f32")
    return hist


def confusion(labels, ref, n_values=2, stream=None):
    """(2, n_values) int64 device tensor: [r, v] = windows with ref == r and
    labels == v -- the confusion matrix of hard labels."""
    _check_labels(labels)
    _check_ref(ref, labels)
    if not 1 <= int(n_values) <= 256:
        raise ValueError(f"n_values must be 1 .. 256, got {n_values}")
    s = stream if stream is not None else torch.cuda.current_stream(labels.device)
    with torch.cuda.stream(s):
        hist = torch.zeros((2, int(n_values)), dtype=torch.int64, device=labels.device)
    _lib.check(_lib.lib().vad_score_histogram_u8(_lib.ptr(labels), _lib.ptr(ref), labels.numel(), int(n_values),
                                                 _lib.ptr(hist), _lib.stream_ptr(stream)), "vad_score_histogram_u8")
    return hist


def roc_from_histogram(hist):
    """The ROC of a (2, bins) histogram (host array): thresholds[b] = b / bins,
    the lower edge of bin b, for b = 0 .. bins (bins + 1 points); at threshold
    b / bins every window of a bin >= b is called speech, so
      tpr[b] = sum(hist[1, b:]) / sum(hist[1]),  fpr[b] = sum(hist[0, b:]) / sum(hist[0])
    (reverse cumulative sums): from (1, 1) at threshold 0 down to (0, 0) at
    threshold 1.  A class with no windows has rate 0 throughout."""
    h = np.asarray(hist, dtype=np.int64)
    if h.ndim != 2 or h.shape[0] != 2 or h.shape[1] < 1:
        raise ValueError("hist must be (2, bins)")
    bins = h.shape[1]
    above = np.concatenate([np.cumsum(h[:, ::-1], axis=1)[:, ::-1], np.zeros((2, 1), np.int64)], axis=1)
    tot = np.maximum(above[:, :1], 1)
    rates = above / tot
    return Roc(np.arange(bins + 1, dtype=np.float64) / bins, rates[1], rates[0])


def roc(scores, ref, bins=1024, stream=None):
    """Hit rate against false-alarm rate of the decision s >= threshold, for
    the bins + 1 thresholds b / bins, from one device histogram and ONE copy of
    its 2 * bins int64 to the host (synchronises).  Returns Roc(thresholds,
    tpr, fpr), host float64 arrays (roc_from_histogram)."""
    h = histogram(scores, ref, bins, stream)
    if stream is not None:
        stream.synchronize()
    return roc_from_histogram(h.cpu().numpy())


def threshold_at(roc, max_fpr):
    """The lowest threshold (bin edge) whose false-alarm rate is <= max_fpr:
    the most sensitive operating point within that budget."""
    if not 0.0 <= float(max_fpr) <= 1.0:
        raise ValueError("max_fpr must be in [0, 1]")
    ok = np.flatnonzero(np.asarray(roc.fpr) <= float(max_fpr))
    return float(roc.thresholds[ok[0]])  # fpr ends at 0, so there is always one
