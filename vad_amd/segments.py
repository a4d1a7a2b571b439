"""Labels -> smoothed labels -> speech segments in samples -> voiced audio,
all on the device (include/vad_amd.h, "Speech segments").

The reference's application keeps the samples of every frame its analyser
returned as active and writes them out (vad.py:52-57,67-72).  Here the clip
path's per-window labels (VadPipeline.labels) are smoothed (close gaps, drop
short runs), turned into sample ranges and the audio of those ranges -- or of
the active frames themselves, the form vad.py writes -- is packed into one
device buffer.  Window i stands for frame i + 2 (sklearn_analyser.py:19,52,77).
No call here synchronises except Segments.numpy() / .seconds().
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .plan import check_out

SEG_TILE = 1024        # VAD_SEG_TILE
SEG_CARRY_PASS = 256   # VAD_SEG_CARRY_PASS

_AUDIO = {torch.float32: "f32", torch.int16: "i16"}


def _check_labels(labels):
    if not isinstance(labels, torch.Tensor):
        raise TypeError("labels must be a CUDA (HIP) torch tensor")
    if labels.dtype != torch.uint8:
        raise TypeError(f"labels must be uint8, got {labels.dtype}")
    if not labels.is_cuda:
        raise TypeError("labels must be a CUDA (HIP) torch tensor")
    if labels.dim() != 1 or not labels.is_contiguous():
        raise ValueError("labels must be a contiguous 1-D tensor")
    return labels


def _check_audio(audio):
    if not isinstance(audio, torch.Tensor):
        raise TypeError("audio must be a CUDA (HIP) torch tensor")
    if audio.dtype not in _AUDIO:
        raise TypeError(f"audio must be float32 or int16, got {audio.dtype}")
    if not audio.is_cuda:
        raise TypeError("audio must be a CUDA (HIP) torch tensor")
    if audio.dim() != 1 or not audio.is_contiguous():
        raise ValueError("audio must be a contiguous 1-D tensor")
    return audio


def _overlaps(a, b):
    if a.numel() == 0 or b.numel() == 0:
        return False
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def workspace(n, device, stream=None):
    """A device workspace for n labels (vad_segments_workspace_bytes)."""
    need = int(_lib.lib().vad_segments_workspace_bytes(int(n)))
    s = stream if stream is not None else torch.cuda.current_stream(device)
    with torch.cuda.stream(s):
        return torch.empty((max(need, 16),), dtype=torch.uint8, device=device)


def smooth_labels(labels, max_gap=0, min_run=0, active=1, out=None, stream=None, ws=None):
    """uint8 0/1 labels after close(max_gap) (inactive runs of at most max_gap
    windows between two active windows become active), then open(min_run)
    (active runs shorter than min_run windows go, at the ends too).  0 turns a
    stage off."""
    _check_labels(labels)
    n = labels.numel()
    if out is None:
        out = torch.empty((n,), dtype=torch.uint8, device=labels.device)
    else:
        check_out(out, (n,), torch.uint8, labels.device, "out")
        if _overlaps(out, labels):
            raise ValueError("out must not alias labels")
    if ws is None:
        ws = workspace(n, labels.device, stream)
    _lib.check(_lib.lib().vad_label_smooth(_lib.ptr(labels), n, int(active), int(max_gap), int(min_run),
                                           _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(stream)),
               "vad_label_smooth")
    return out


class Segments:
    """The device segment table of one clip: ``table`` (capacity, 3) int64 rows
    (start, end, offset into the packed voiced audio), ``counts`` (2,) int64
    (segments found, voiced samples of all segments found).  Rows past
    min(found, capacity) are not written."""

    def __init__(self, table, counts, n_samples, stream=None):
        self.table = table
        self.counts = counts
        self.n_samples = int(n_samples)
        self.stream = stream  # the stream the table was computed on (None: the current one)

    @property
    def capacity(self):
        return self.table.shape[0]

    def numpy(self):
        """(k, 2) int64 [start, end) in samples -- synchronises."""
        if self.stream is not None:
            self.stream.synchronize()
        found = int(self.counts[0].item())
        k = min(found, self.capacity)
        return self.table[:k, :2].cpu().numpy().astype(np.int64).reshape(k, 2)

    def seconds(self, rate):
        """(k, 2) float [start, end) in seconds at `rate` samples per second -- synchronises."""
        return self.numpy().astype(np.float64) / float(rate)


def label_segments(labels, n_samples, frame_size=400, hop=160, max_gap=0, min_run=0, active=1, capacity=None,
                   stream=None, ws=None):
    """Speech segments of a clip of n_samples samples from its window labels:
    smooth(max_gap, min_run), runs whose frames overlap or touch joined, each
    run [i0, i1] -> samples [(i0+2)*hop, min((i1+2)*hop + frame_size,
    n_samples)).  capacity: rows of the table (default: the worst case,
    n // 2 + 1).  Returns a Segments; nothing synchronises."""
    _check_labels(labels)
    n = labels.numel()
    if not 0 < hop <= frame_size:
        raise ValueError("segments need 0 < hop <= frame_size")
    if capacity is None:
        capacity = n // 2 + 1
    if capacity < 0:
        raise ValueError("capacity must be >= 0")
    s = stream if stream is not None else torch.cuda.current_stream(labels.device)
    with torch.cuda.stream(s):
        table = torch.empty((int(capacity), 3), dtype=torch.int64, device=labels.device)
        counts = torch.empty((2,), dtype=torch.int64, device=labels.device)
    if ws is None:
        ws = workspace(n, labels.device, stream)
    _lib.check(_lib.lib().vad_label_segments(
        _lib.ptr(labels), n, int(active), int(max_gap), int(min_run), int(frame_size), int(hop), int(n_samples),
        _lib.ptr(table), int(capacity), _lib.ptr(counts), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(stream)),
        "vad_label_segments")
    return Segments(table, counts, n_samples, stream)


def voiced_audio(audio, segments, out=None, stream=None):
    """The samples of every segment, packed in order: (out, counts) with
    out[:min(counts[1], len(out))] valid (when the table held every segment
    found).  float32 or int16; bits are copied.  out defaults to a buffer of
    the clip's size; elements past the voiced count are not touched.  No
    synchronisation."""
    _check_audio(audio)
    if not isinstance(segments, Segments):
        raise TypeError("segments must be a Segments (label_segments)")
    if audio.numel() != segments.n_samples:
        raise ValueError(f"the segments are of a clip of {segments.n_samples} samples, audio has {audio.numel()}")
    if out is None:
        s = stream if stream is not None else torch.cuda.current_stream(audio.device)
        with torch.cuda.stream(s):
            out = torch.empty((audio.numel(),), dtype=audio.dtype, device=audio.device)
    else:
        if not (isinstance(out, torch.Tensor) and out.is_cuda):
            raise TypeError("out must be a CUDA (HIP) torch tensor")
        if out.dtype != audio.dtype:
            raise TypeError(f"out must be {audio.dtype}, got {out.dtype}")
        if out.dim() != 1 or not out.is_contiguous() or out.device != audio.device:
            raise ValueError("out must be a contiguous 1-D tensor on the audio's device")
        if _overlaps(out, audio):
            raise ValueError("out must not alias audio")
    fn = "vad_gather_segments_" + _AUDIO[audio.dtype]
    _lib.check(getattr(_lib.lib(), fn)(_lib.ptr(audio), audio.numel(), _lib.ptr(segments.table),
                                       _lib.ptr(segments.counts), segments.capacity, _lib.ptr(out), out.numel(),
                                       _lib.stream_ptr(stream)), fn)
    return out, segments.counts


def active_frames(audio, labels, frame_size=400, hop=160, active=1, out=None, stream=None, ws=None):
    """The frames of the active windows, one after another, overlapping samples
    repeated -- what vad.py:52-57 accumulates: (out, count) with out
    (rows, frame_size), row r = audio[(i_r+2)*hop : (i_r+2)*hop + frame_size]
    for the r-th active window, and count a (1,) int64 device tensor of the
    windows found.  out defaults to one row per label; rows past count are not
    touched.  Any hop > 0.  No synchronisation."""
    _check_audio(audio)
    _check_labels(labels)
    n = labels.numel()
    if frame_size <= 0 or hop <= 0:
        raise ValueError("frame_size and hop must be positive")
    s = stream if stream is not None else torch.cuda.current_stream(audio.device)
    if out is None:
        with torch.cuda.stream(s):
            out = torch.empty((n, frame_size), dtype=audio.dtype, device=audio.device)
    else:
        if not (isinstance(out, torch.Tensor) and out.is_cuda):
            raise TypeError("out must be a CUDA (HIP) torch tensor")
        if out.dtype != audio.dtype:
            raise TypeError(f"out must be {audio.dtype}, got {out.dtype}")
        if out.dim() != 2 or out.shape[1] != frame_size or not out.is_contiguous() or out.device != audio.device:
            raise ValueError("out must be a contiguous (rows, frame_size) tensor on the audio's device")
        if _overlaps(out, audio):
            raise ValueError("out must not alias audio")
    with torch.cuda.stream(s):
        count = torch.empty((1,), dtype=torch.int64, device=audio.device)
    if ws is None:
        ws = workspace(n, labels.device, stream)
    fn = "vad_gather_active_frames_" + _AUDIO[audio.dtype]
    _lib.check(getattr(_lib.lib(), fn)(
        _lib.ptr(audio), audio.numel(), _lib.ptr(labels), n, int(active), int(frame_size), int(hop), _lib.ptr(out),
        out.shape[0], _lib.ptr(count), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(stream)), fn)
    return out, count


# ----------------------------------------------------------------------------
# Clip batches (include/vad_amd.h, "Clip batches"; vad_amd.batch.ClipBatch)
# ----------------------------------------------------------------------------
def batch_workspace(batch, device, stream=None):
    """A device workspace for a batch's windows (vad_batch_segments_workspace_bytes)."""
    need = int(_lib.lib().vad_batch_segments_workspace_bytes(batch.n_windows, batch.n_clips))
    s = stream if stream is not None else torch.cuda.current_stream(device)
    with torch.cuda.stream(s):
        return torch.empty((max(need, 16),), dtype=torch.uint8, device=device)


def _check_batch_labels(labels, batch):
    labels = getattr(labels, "labels", labels)  # a BatchLabels, or a caller-made tensor
    _check_labels(labels)
    if labels.numel() != batch.n_windows:
        raise ValueError(f"the batch has {batch.n_windows} global windows, labels has {labels.numel()}")
    return labels


def batch_smooth_labels(labels, batch, max_gap=0, min_run=0, active=1, out=None, stream=None, ws=None):
    """smooth_labels over the global window array of a ClipBatch, every clip's
    range a sequence of its own: uint8 0/1 per global window, 0 for the
    windows of no clip.  labels: a BatchLabels or a (batch.n_windows,) uint8
    device tensor."""
    labels = _check_batch_labels(labels, batch)
    n = labels.numel()
    if out is None:
        out = torch.empty((n,), dtype=torch.uint8, device=labels.device)
    else:
        check_out(out, (n,), torch.uint8, labels.device, "out")
        if _overlaps(out, labels):
            raise ValueError("out must not alias labels")
    if ws is None:
        ws = batch_workspace(batch, labels.device, stream)
    _lib.check(_lib.lib().vad_batch_label_smooth(
        _lib.ptr(labels), n, _lib.ptr(batch.d_frame0), _lib.ptr(batch.d_n_rows), batch.n_clips, int(active),
        int(max_gap), int(min_run), _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(stream)),
        "vad_batch_label_smooth")
    return out


class BatchSegments:
    """The device segment tables of a batch: ``table`` (capacity, 4) int64
    rows (clip, start, end, offset) in each clip's own samples, ordered by
    clip, then start; ``packed`` (capacity, 3) int64 rows (start, end, offset)
    in samples of the packed buffer, the table vad_gather_segments_* takes;
    ``counts`` (2,) (rows found, voiced samples found); per clip ``clip_rows``,
    ``clip_row0`` (its exclusive prefix) and ``clip_voiced``.  The four small
    tensors are views of one, ``meta``, so one copy brings them to the host.
    Rows past min(found, capacity) are not written."""

    def __init__(self, table, packed, meta, batch, stream=None):
        n = batch.n_clips
        self.table, self.packed, self.meta, self.batch = table, packed, meta, batch
        self.counts = meta[:2]
        self.clip_rows, self.clip_row0, self.clip_voiced = meta[2:2 + n], meta[2 + n:2 + 2 * n], meta[2 + 2 * n:]
        self.stream = stream

    @property
    def capacity(self):
        return self.table.shape[0]

    def _host(self):
        if self.stream is not None:
            self.stream.synchronize()
        meta = self.meta.cpu().numpy()
        k = min(int(meta[0]), self.capacity)
        return meta, self.table[:k].cpu().numpy().astype(np.int64).reshape(k, 4)

    def numpy(self):
        """(k, 3) int64 rows (clip, start, end), samples of the clip -- synchronises."""
        return self._host()[1][:, :3]

    def clip(self, k):
        """(r, 2) int64 [start, end) of clip k's segments -- synchronises."""
        meta, rows = self._host()
        n = self.batch.n_clips
        if not 0 <= k < n:
            raise IndexError(k)
        r0, r = int(meta[2 + n + k]), int(meta[2 + k])
        return rows[r0:r0 + r, 1:3]

    def seconds(self, rate):
        """(k, 3) float64 rows (clip, start, end) with the times in seconds at
        `rate` samples per second -- synchronises."""
        out = self.numpy().astype(np.float64)
        out[:, 1:] /= float(rate)
        return out


def batch_label_segments(labels, batch, max_gap=0, min_run=0, active=1, capacity=None, stream=None, ws=None):
    """label_segments for every clip of a ClipBatch in one launch chain (no
    segment crosses a clip boundary).  labels: a BatchLabels or a
    (batch.n_windows,) uint8 device tensor.  capacity: rows of the tables
    (default: the worst case, sum over the clips of ceil(n_rows / 2)).
    Returns a BatchSegments; nothing synchronises."""
    labels = _check_batch_labels(labels, batch)
    n = labels.numel()
    if capacity is None:
        capacity = int(((batch.host["n_rows"] + 1) // 2).sum())
    if capacity < 0:
        raise ValueError("capacity must be >= 0")
    s = stream if stream is not None else torch.cuda.current_stream(labels.device)
    nc = batch.n_clips
    with torch.cuda.stream(s):
        table = torch.empty((int(capacity), 4), dtype=torch.int64, device=labels.device)
        packed = torch.empty((int(capacity), 3), dtype=torch.int64, device=labels.device)
        meta = torch.empty((2 + 3 * nc,), dtype=torch.int64, device=labels.device)
    if ws is None:
        ws = batch_workspace(batch, labels.device, stream)
    seg = BatchSegments(table, packed, meta, batch, stream)
    _lib.check(_lib.lib().vad_batch_label_segments(
        _lib.ptr(labels), n, _lib.ptr(batch.d_frame0), _lib.ptr(batch.d_n_rows), _lib.ptr(batch.d_len), nc,
        int(active), int(max_gap), int(min_run), batch.frame_size, batch.hop, _lib.ptr(table), _lib.ptr(packed),
        int(capacity), _lib.ptr(seg.counts), _lib.ptr(seg.clip_rows), _lib.ptr(seg.clip_row0),
        _lib.ptr(seg.clip_voiced), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(stream)), "vad_batch_label_segments")
    return seg


def batch_voiced_audio(batch, segments, out=None, stream=None):
    """The samples of every segment of every clip, packed in order, through
    the clip path's gather over the packed buffer: (out, counts) as
    voiced_audio.  Clip k's samples start at the sum of clip_voiced before k.
    No synchronisation."""
    if not isinstance(segments, BatchSegments):
        raise TypeError("segments must be a BatchSegments (batch_label_segments)")
    audio = batch.data
    if out is None:
        s = stream if stream is not None else torch.cuda.current_stream(audio.device)
        with torch.cuda.stream(s):
            out = torch.empty((audio.numel(),), dtype=audio.dtype, device=audio.device)
    else:
        check_out(out, tuple(out.shape), audio.dtype, audio.device, "out")
        if out.dim() != 1:
            raise ValueError("out must be 1-D")
        if _overlaps(out, audio):
            raise ValueError("out must not alias the packed buffer")
    fn = "vad_gather_segments_" + _AUDIO[audio.dtype]
    _lib.check(getattr(_lib.lib(), fn)(_lib.ptr(audio), audio.numel(), _lib.ptr(segments.packed),
                                       _lib.ptr(segments.counts), segments.capacity, _lib.ptr(out), out.numel(),
                                       _lib.stream_ptr(stream)), fn)
    return out, segments.counts
