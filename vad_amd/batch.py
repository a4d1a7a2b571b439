"""Clip batches: many finished clips of different lengths in one device
buffer, so that the clip kernels run once over all of them
(include/vad_amd.h, "Clip batches").

The reference's dataset export takes FILES_PER_STEP files at a time
(dataset_creator.py:58-71), and its application labels one utterance after
another (vad.py:52-72); here a chunk of files, or a queue of utterances, is
one ``ClipBatch`` and ``VadPipeline.labels_batch`` / ``features_batch`` /
``segments_batch`` / ``voiced_batch`` each run one launch chain over it.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .config import MfccConfig
from .plan import n_frames

_DTYPES = {torch.float32: ("f32", np.float32), torch.int16: ("i16", np.int16)}
_TABLES = ("start", "len", "frame0", "n_frames", "n_rows", "row0")


def layout(lens, frame_size, hop):
    """The tables of a batch of clips of ``lens`` samples, as int64 numpy
    arrays, and the packed buffer's size: ``(tables, total)`` with tables a
    dict of start, len, frame0, n_frames, n_rows, row0 (see ClipBatch)."""
    if not 0 < hop <= frame_size:
        raise ValueError("a clip batch needs 0 < hop <= frame_size")
    lens = np.asarray(list(lens), np.int64).reshape(-1)
    if (lens < 0).any():
        raise ValueError("negative clip length")
    slots = -(-lens // hop)
    frame0 = np.concatenate(([0], np.cumsum(slots)))[:-1].astype(np.int64) if len(lens) else lens.copy()
    frames = np.where(lens > frame_size, (lens - frame_size - 1) // hop + 1, 0).astype(np.int64)
    rows = np.maximum(frames - 5, 0)
    row0 = (np.cumsum(rows) - rows).astype(np.int64)
    t = {"start": frame0 * hop, "len": lens, "frame0": frame0, "n_frames": frames, "n_rows": rows, "row0": row0}
    return t, int(slots.sum()) * hop


class ClipBatch:
    """n_clips clips, all int16 or all float32, in one contiguous device
    buffer ``data`` of ``total`` samples.

    Placement.  With L = cfg.frame_size and H = cfg.hop, clip k (len[k]
    samples) starts at sample start[k] = H * frame0[k] and occupies
    ceil(len[k] / H) hop slots: frame0[k+1] = frame0[k] + ceil(len[k] / H),
    total = H * sum_k ceil(len[k] / H).  The unused tail of its last slot is
    zero.

    Global frame grid.  The clip kernels read frame g of a buffer at g * H.
    Frame i of clip k (i < F_k = vad_n_frames(len[k])) is therefore global
    frame frame0[k] + i, and window (row) i of clip k, i < n_rows[k] =
    max(F_k - 5, 0), is global window frame0[k] + i; row0[k] is the exclusive
    prefix of n_rows (rows packed clip after clip).

    Clip ranges lie inside the global ranges.  Frame i of clip k exists when
    i * H + L < len[k].  Its global frame g = frame0[k] + i then has
    g * H + L = start[k] + i * H + L < start[k] + len[k] <= start[k] + H *
    ceil(len[k] / H) <= total, which is the condition for g to be a frame of
    the packed buffer: frame0[k] + F_k <= G = vad_n_frames(total).  The frame
    reads only samples below start[k] + len[k], clip k's own.  Rows: i <
    F_k - 5 gives frame0[k] + i < frame0[k] + F_k - 5 <= G - 5.  The
    constructor asserts both, for the clips that have frames / rows (a clip
    without any has an empty range: its frame0 may lie past G when only such
    clips follow it, and nothing is read or written there).

    Junk frames.  A global frame that is no clip's frame straddles two clips
    (or a clip and its zero tail); its MFCC row, and the rows of the windows
    that use it, are computed and never read.  There are G - sum_k F_k of
    them, G = total / H - floor(L / H) for total > L (else 0): per clip
    ceil(len[k] / H) - F_k, which is floor(L / H) or ceil(L / H) for a clip
    longer than L (2 or 3 at the reference framing) and ceil(len[k] / H) for
    a shorter one, less the floor(L / H) frames the packed buffer's own end
    does not have.  ``junk_frames`` is that number.

    Tables.  ``tables`` is one (6, n_clips) int64 device tensor (start, len,
    frame0, n_frames, n_rows, row0, also as attributes ``d_start`` ...);
    ``host`` holds the same as numpy arrays.
    """

    def __init__(self, data, lens, cfg: MfccConfig = MfccConfig(), _tables=None, _staging=None):
        if not (isinstance(data, torch.Tensor) and data.is_cuda and data.dtype in _DTYPES and data.dim() == 1
                and data.is_contiguous()):
            raise TypeError("data must be a contiguous 1-D float32 or int16 CUDA tensor")
        self.cfg = cfg
        self.frame_size, self.hop = int(cfg.frame_size), int(cfg.hop)
        self.host, self.total = layout(lens, self.frame_size, self.hop)
        if data.numel() != self.total:
            raise ValueError(f"the packed buffer of these clips has {self.total} samples, data has {data.numel()}")
        self.data = data
        self.n_clips = len(self.host["len"])
        self.n_frames_global = n_frames(self.total, self.frame_size, self.hop)
        self.n_windows = max(self.n_frames_global - 5, 0)
        self.total_rows = int(self.host["n_rows"].sum())
        h = self.host
        # the clip ranges lie inside the global ranges (the class docstring has the proof)
        has = h["n_frames"] > 0
        assert not has.any() or (h["frame0"] + h["n_frames"])[has].max() <= self.n_frames_global
        assert self.total_rows == 0 or (h["frame0"] + h["n_rows"])[h["n_rows"] > 0].max() <= self.n_windows
        assert self.total <= self.frame_size or \
            self.n_frames_global == self.total // self.hop - self.frame_size // self.hop
        self.junk_frames = self.n_frames_global - int(h["n_frames"].sum())
        if _tables is None:
            _tables = torch.from_numpy(np.stack([h[t] for t in _TABLES]).reshape(6, self.n_clips)).to(data.device)
        self.tables = _tables
        for i, t in enumerate(_TABLES):
            setattr(self, "d_" + t, self.tables[i])
        self._staging = _staging  # the pinned buffer of from_host, kept until the copy is done

    def __len__(self):
        return self.n_clips

    @property
    def junk_share(self):
        """Junk frames over all global frames (0 for an empty batch)."""
        return self.junk_frames / self.n_frames_global if self.n_frames_global else 0.0

    def clip(self, k):
        """The samples of clip k: a view of ``data``."""
        s = int(self.host["start"][k])
        return self.data[s:s + int(self.host["len"][k])]

    # -- constructors -------------------------------------------------------
    @classmethod
    def from_host(cls, arrays, cfg: MfccConfig = MfccConfig(), device=None):
        """Pack host arrays (numpy, all int16 or all float32) into one pinned
        buffer and make one H2D copy."""
        arrays = [np.asarray(a) for a in arrays]
        kinds = {a.dtype for a in arrays}
        if len(kinds) > 1:
            raise TypeError(f"the clips of a batch are all int16 or all float32, got {sorted(map(str, kinds))}")
        dt = kinds.pop() if kinds else np.dtype(np.float32)
        tdt = {np.dtype(np.int16): torch.int16, np.dtype(np.float32): torch.float32}.get(dt)
        if tdt is None:
            raise TypeError(f"clips must be int16 or float32, got {dt}")
        if any(a.ndim != 1 for a in arrays):
            raise ValueError("every clip is a 1-D array")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        t, total = layout([len(a) for a in arrays], cfg.frame_size, cfg.hop)
        stage = torch.zeros((total,), dtype=tdt, pin_memory=True)
        view = stage.numpy()
        for a, s in zip(arrays, t["start"].tolist()):
            view[s:s + len(a)] = a
        data = torch.empty((total,), dtype=tdt, device=dev)
        data.copy_(stage, non_blocking=True)
        return cls(data, t["len"], cfg, _staging=stage)

    @classmethod
    def from_device(cls, tensors, cfg: MfccConfig = MfccConfig(), stream=None):
        """Pack device tensors (contiguous 1-D, all int16 or all float32, at
        any sample offset of their allocations) with ONE ragged-copy launch
        (vad_batch_pack_*), whatever their number; the tables and the source
        addresses travel in one H2D copy."""
        tensors = list(tensors)
        for x in tensors:
            if not (isinstance(x, torch.Tensor) and x.is_cuda):
                raise TypeError("every clip must be a CUDA (HIP) torch tensor")
            if x.dim() != 1 or not x.is_contiguous():
                raise ValueError("every clip must be a contiguous 1-D tensor")
        kinds = {x.dtype for x in tensors}
        if len(kinds) > 1:
            raise TypeError(f"the clips of a batch are all int16 or all float32, got {sorted(map(str, kinds))}")
        tdt = kinds.pop() if kinds else torch.float32
        if tdt not in _DTYPES:
            raise TypeError(f"clips must be int16 or float32, got {tdt}")
        if len({x.device for x in tensors}) > 1:
            raise ValueError("the clips of a batch lie on one device")
        dev = tensors[0].device if tensors else torch.device("cuda", torch.cuda.current_device())
        t, total = layout([x.numel() for x in tensors], cfg.frame_size, cfg.hop)
        n = len(tensors)
        ptrs = np.array([x.data_ptr() for x in tensors], np.int64).reshape(n)
        host = np.stack([t[name] for name in _TABLES] + [ptrs]).reshape(7, n)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            d = torch.from_numpy(host).to(dev)
            data = torch.empty((total,), dtype=tdt, device=dev)
            fn = "vad_batch_pack_" + _DTYPES[tdt][0]
            _lib.check(getattr(_lib.lib(), fn)(_lib.ptr(d[6]), _lib.ptr(d[1]), _lib.ptr(d[0]), n, _lib.ptr(data),
                                               total, _lib.stream_ptr(s)), fn)
        return cls(data, t["len"], cfg, _tables=d[:6])


class BatchLabels:
    """The labels of a batch: ``labels`` is the global (G - 5,) uint8 tensor
    over the packed buffer's windows; ``[k]`` is the view of clip k's
    n_rows[k] labels.  Nothing is compacted or synchronised."""

    def __init__(self, labels, batch):
        self.labels = labels
        self.batch = batch

    def __len__(self):
        return self.batch.n_clips

    def __getitem__(self, k):
        if not -self.batch.n_clips <= k < self.batch.n_clips:
            raise IndexError(k)
        f0 = int(self.batch.host["frame0"][k])
        return self.labels[f0:f0 + int(self.batch.host["n_rows"][k])]

    def packed(self, stream=None):
        """The labels clip after clip, (sum n_rows,) uint8 (vad_batch_compact_rows)."""
        return compact_rows(self.labels, self.batch, stream=stream)


def compact_rows(rows, batch, stream=None):
    """out[row0[k] + i] = rows[frame0[k] + i]: the per-clip rows of a tensor
    over the batch's global windows (first dimension), clip after clip."""
    if not (isinstance(rows, torch.Tensor) and rows.is_cuda and rows.is_contiguous() and rows.dim() >= 1):
        raise TypeError("rows must be a contiguous CUDA (HIP) torch tensor")
    if rows.shape[0] < batch.n_windows:
        raise ValueError(f"rows has {rows.shape[0]} rows, the batch {batch.n_windows} windows")
    row_bytes = rows.element_size() * int(np.prod(rows.shape[1:], dtype=np.int64))
    s = stream if stream is not None else torch.cuda.current_stream(rows.device)
    with torch.cuda.stream(s):
        out = torch.empty((batch.total_rows,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
    _lib.check(_lib.lib().vad_batch_compact_rows(
        _lib.ptr(rows), rows.shape[0], row_bytes, _lib.ptr(batch.d_frame0), _lib.ptr(batch.d_n_rows),
        _lib.ptr(batch.d_row0), batch.n_clips, _lib.ptr(out), batch.total_rows, _lib.stream_ptr(s)),
        "vad_batch_compact_rows")
    return out
