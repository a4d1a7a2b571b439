"""NumPy models of the score stage (include/vad_amd.h, "Speech scores"):
hysteresis, padding (single clip and per clip of a batch), reference labels
and the score histogram.  Plain loops and np.maximum.accumulate over the whole
array; nothing here knows about tiles or carries."""
import numpy as np


def hysteresis(s, on, off):
    """h[-1] = 0; 1 if s >= on, 0 if s < off or NaN, else the previous: the
    decision of the last decided window at or before i."""
    s = np.asarray(s, np.float32)
    n = len(s)
    with np.errstate(invalid="ignore"):
        up = s >= np.float32(on)
        down = ~up & ~(s >= np.float32(off))  # below off, or NaN
    last = np.maximum.accumulate(np.where(up | down, np.arange(n), -1)) if n else np.zeros(0, np.int64)
    return np.where(last >= 0, up[np.maximum(last, 0)], False).astype(np.uint8)


def dilate(labels, active, pad_before, pad_after):
    """out[i] = 1 iff labels[j] == active for a j in [i - pad_after, i + pad_before]."""
    a = np.asarray(labels) == active
    n = len(a)
    if n == 0:
        return np.zeros(0, np.uint8)
    idx = np.arange(n)
    prev = np.maximum.accumulate(np.where(a, idx, -1))                 # last active <= i
    nxt = np.minimum.accumulate(np.where(a, idx, 2 * n)[::-1])[::-1]   # first active >= i
    tail = (prev >= 0) & (idx - prev <= pad_after)
    head = (nxt < n) & (nxt - idx <= pad_before)
    return (tail | head).astype(np.uint8)


def per_clip(fn, x, frame0, n_rows, fill=0):
    """fn over every clip's own range of a global window array; `fill` elsewhere."""
    x = np.asarray(x)
    out = np.full(len(x), fill, np.uint8)
    for f0, r in zip(frame0, n_rows):
        out[f0:f0 + r] = fn(x[f0:f0 + r])
    return out


def reference_labels(intervals, n, frame_size, hop):
    """Window i is 1 iff the centre sample of frame i + 2 lies in a [start, end)."""
    centre = (np.arange(n, dtype=np.int64) + 2) * hop + frame_size // 2
    out = np.zeros(n, np.uint8)
    for s, e in np.asarray(intervals, np.int64).reshape(-1, 2):
        out[(centre >= s) & (centre < e)] = 1
    return out


def score_bins(s, bins):
    """min(int(s * bins), bins - 1) with the product in float32; NaN and negatives -> 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(s, np.float32) * np.float32(bins)
    b = np.zeros(len(t), np.int64)
    ok = t > 0  # False for NaN
    big = ok & (t >= np.float32(bins))
    mid = ok & ~big
    b[mid] = t[mid].astype(np.int64)
    b[big] = bins - 1
    return b


def histogram(s, ref, bins):
    """(2, bins) int64: [r, b] = windows with ref == r (0 / 1) and score bin b."""
    b = score_bins(s, bins)
    ref = np.asarray(ref)
    return np.stack([np.bincount(b[ref == r], minlength=bins) for r in (0, 1)]).astype(np.int64)


def confusion(labels, ref, n_values):
    labels, ref = np.asarray(labels), np.asarray(ref)
    keep = labels < n_values
    return np.stack([np.bincount(labels[keep & (ref == r)], minlength=n_values) for r in (0, 1)]).astype(np.int64)
