"""Streaming segments: per stream, the label blocks of a StreamBatch -> finished
speech segments and the voiced samples, on the device, with a fixed delay
(include/vad_amd.h, "Streaming segments"; csrc/stream_segments_kernel.hip).

The live loop of the reference (vad.py:32-59) feeds frames one at a time and
keeps the samples of the active ones.  StreamSegmenter does that for S streams
at once, after the smoothing of the clip path (vad_amd.segments): push() takes
the (K, S) label block the hop kernels wrote and, optionally, the (K, S, hop)
sample block they read; every hop decides one window, ``delay`` windows behind
the newest, appends the segments that ended there to ``table`` / ``found`` and
writes that hop's voiced samples as a prefix of its row of ``voiced``
(``voiced_len`` says how long).  After flush() every stream's rows and voiced
samples equal label_segments / voiced_audio on its equivalent clip (the
carried frame_size - hop samples, then every hop pushed).

Operating point: StreamSegmenter(..., on=, off=, pad=) carries the clip path's
decision chain (vad_amd.scores: score_labels -> smooth_labels -> dilate_labels
-> label_segments) through the live path.  With ``on`` set, push() takes the
(K, S) float32 score block of a StreamBatch built with scores=True and decides
each window by hysteresis (1 at s >= on, 0 at s < off or NaN, else the
previous decision); with pad=(before, after) every smoothed run grows by that
many windows before the segments are cut, which costs ``before`` more windows
of delay and none for ``after``.  After flush() the rows and voiced samples
equal that clip chain on the stream's equivalent clip, bit for bit.

No call synchronises except segments().  One kernel per push: capturable
behind the hop kernel on the same stream.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .config import MfccConfig

_AUDIO = {torch.float32: "f32", torch.int16: "i16"}


class StreamSegmenter:
    """State, history, ``table`` (S, capacity, 2) int64 [start, end) in samples
    of the equivalent clip, ``found`` (S,) int64 (every segment finished; the
    first `capacity` are in the table), and the static outputs ``voiced``
    (K, S, hop) / ``voiced_len`` (K, S) int32 of a push and ``flush_voiced``
    (F, S, hop) / ``flush_len`` (F, S) of a flush.  audio_dtype None: events
    only (no history, no voiced outputs)."""

    def __init__(self, n_streams, cfg: MfccConfig = MfccConfig(), max_gap=0, min_run=0, active=1, capacity=64,
                 hops_per_step=1, audio_dtype=None, device=None, on=None, off=None, pad=(0, 0)):
        S, K, L, H = int(n_streams), int(hops_per_step), int(cfg.frame_size), int(cfg.hop)
        if S < 1:
            raise ValueError("n_streams must be >= 1")
        if K < 1:
            raise ValueError("hops_per_step must be >= 1")
        if not 0 < H <= L:
            raise ValueError("segments need 0 < hop <= frame_size")
        if max_gap < 0 or min_run < 0:
            raise ValueError("max_gap and min_run must be >= 0")
        if not 0 <= int(active) < 255:
            raise ValueError("active must be in [0, 255): 255 is the hop kernels' 'no label yet'")
        if capacity < 0:
            raise ValueError("capacity must be >= 0")
        if audio_dtype is not None and audio_dtype not in _AUDIO:
            raise TypeError(f"audio_dtype must be float32, int16 or None, got {audio_dtype}")
        from .scores import _check_pad, _check_thresholds
        if on is None and off is not None:
            raise ValueError("off needs on")
        self.on, self.off = _check_thresholds(on, off) if on is not None else (None, None)
        self.pad = _check_pad(pad)
        # at the defaults the segmenter calls the label entries it always called
        self._op = on is not None or self.pad != (0, 0)
        lib = _lib.lib()
        self.n, self.K, self.cfg = S, K, cfg
        self.max_gap, self.min_run, self.active, self.capacity = int(max_gap), int(min_run), int(active), int(capacity)
        self.audio_dtype = audio_dtype
        if self._op:
            self._delay = int(lib.vad_stream_seg_delay_pad(self.max_gap, self.min_run, L, H, *self.pad))
            self.flush_rows = int(lib.vad_stream_seg_flush_rows_pad(self.max_gap, self.min_run, L, H, *self.pad))
        else:
            self._delay = int(lib.vad_stream_seg_delay(self.max_gap, self.min_run, L, H))
            self.flush_rows = int(lib.vad_stream_seg_flush_rows(self.max_gap, self.min_run, L, H))
        if self._delay < 0:
            raise ValueError("max_gap / min_run / pad out of range")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.device = dev
        self.state = torch.zeros((S, int(lib.vad_stream_seg_state_bytes(1)) // 8), dtype=torch.int64, device=dev)
        self.table = torch.zeros((S, self.capacity, 2), dtype=torch.int64, device=dev)
        self.found = torch.zeros((S,), dtype=torch.int64, device=dev)
        self._params = (self.max_gap, self.min_run, L, H)
        self._block_dtype = torch.float32 if on is not None else torch.uint8
        if self._op:  # block_is_scores ... and the operating point behind the framing
            self._is_scores = 1 if on is not None else 0
            self._params += (self.on if on is not None else 0.0, self.off if on is not None else 0.0) + self.pad
        self._events_fn = "vad_stream_segments_op" if self._op else "vad_stream_segments"
        self._events_flush_fn = self._events_fn + "_flush"
        self._tables = (_lib.ptr(self.state), _lib.ptr(self.table), self.capacity, _lib.ptr(self.found))
        if audio_dtype is None:
            self.history = self.voiced = self.voiced_len = self.flush_voiced = self.flush_len = None
            return
        if self._op:
            elems = int(lib.vad_stream_seg_history_elems_pad(S, K, self.max_gap, self.min_run, L, H, *self.pad))
        else:
            elems = int(lib.vad_stream_seg_history_elems(S, K, self.max_gap, self.min_run, L, H))
        if elems < 0:
            raise ValueError("the history of one stream would pass 2^30 elements")
        self.history = torch.zeros((S, elems // S), dtype=audio_dtype, device=dev)
        self.voiced = torch.zeros((K, S, H), dtype=audio_dtype, device=dev)
        self.voiced_len = torch.zeros((K, S), dtype=torch.int32, device=dev)
        self.flush_voiced = torch.zeros((self.flush_rows, S, H), dtype=audio_dtype, device=dev)
        self.flush_len = torch.zeros((self.flush_rows, S), dtype=torch.int32, device=dev)
        self._fn = self._events_fn + "_" + _AUDIO[audio_dtype]
        self._flush_fn = self._events_flush_fn + "_" + _AUDIO[audio_dtype]

    @property
    def delay(self):
        """D: hop t decides window t - 5 - D (vad_stream_seg_delay; with an
        operating point vad_stream_seg_delay_pad: pad_before more)."""
        return self._delay

    def reset(self):
        """Every stream back to before its first hop (zero carry)."""
        self.state.zero_()
        self.found.zero_()
        if self.history is not None:
            self.history.zero_()

    def prime(self, carry):
        """The carried frame_size - hop samples of every stream (S, L-H), as
        StreamBatch.prime takes them, before the first push.  They only matter
        when frame_size > 3 * hop (positions in [2 hop, L - hop) can be voiced)."""
        if self.history is None:
            raise ValueError("an events-only segmenter keeps no samples")
        n = self.cfg.frame_size - self.cfg.hop
        if tuple(carry.shape) != (self.n, n):
            raise ValueError(f"carry must have shape {(self.n, n)}")
        if n:
            self.history[:, self.history.shape[1] - n:].copy_(carry)

    def _check_labels(self, lab):
        if not isinstance(lab, torch.Tensor) or not lab.is_cuda:
            raise TypeError("label_block must be a CUDA (HIP) torch tensor")
        if lab.dtype != self._block_dtype:
            what = "the score block must be float32" if self.on is not None else "label_block must be uint8"
            raise TypeError(f"{what}, got {lab.dtype}")
        if lab.dim() == 1 and self.K == 1:
            lab = lab.unsqueeze(0)
        if lab.dim() != 2 or lab.shape[1] != self.n or not 1 <= lab.shape[0] <= self.K:
            raise ValueError(f"label_block must have shape (k <= {self.K}, {self.n})")
        if lab.stride(1) != 1 or lab.device != self.device:
            raise ValueError("label rows must be contiguous and on the segmenter's device")
        return lab

    def _check_hops(self, hop, k):
        if self.history is None:
            raise ValueError("this segmenter was built without audio_dtype: events only")
        if not isinstance(hop, torch.Tensor) or not hop.is_cuda:
            raise TypeError("hop_block must be a CUDA (HIP) torch tensor")
        if hop.dtype != self.audio_dtype:
            raise TypeError(f"hop_block must be {self.audio_dtype}, got {hop.dtype}")
        if hop.dim() == 2 and self.K == 1:
            hop = hop.unsqueeze(0)
        if tuple(hop.shape) != (k, self.n, self.cfg.hop):
            raise ValueError(f"hop_block must have shape {(k, self.n, self.cfg.hop)}")
        if hop.stride(2) != 1 or hop.device != self.device:
            raise ValueError("hop rows must be contiguous and on the segmenter's device")
        return hop

    def push(self, label_block, hop_block=None, stream=None):
        """k <= K hops of every stream: label_block (k, S) uint8 as the hop
        kernels wrote it (strided rows are fine; (S,) for K = 1) -- with ``on``
        set, the (k, S) float32 score block instead -- hop_block
        (k, S, hop) the samples they read, in any layout vad_stream_hops
        reads in place.  Returns (voiced, voiced_len) -- the static outputs,
        rows [0, k) written -- or None without audio."""
        lab = self._check_labels(label_block)
        k = lab.shape[0]
        lib = _lib.lib()
        head = (_lib.ptr(lab),) + ((self._is_scores,) if self._op else ()) + \
            (lab.stride(0) if k > 1 else 0, self.n, k, self.active) + self._params + self._tables
        st = _lib.stream_ptr(stream)
        if hop_block is None:
            _lib.check(getattr(lib, self._events_fn)(*head, st), self._events_fn)
            return None
        hop = self._check_hops(hop_block, k)
        _lib.check(getattr(lib, self._fn)(*head, _lib.ptr(hop), hop.stride(1), hop.stride(0) if k > 1 else 0,
                                          _lib.ptr(self.history), self.history.numel(), _lib.ptr(self.voiced),
                                          _lib.ptr(self.voiced_len), st), self._fn)
        return self.voiced, self.voiced_len

    def flush(self, stream=None):
        """Decide everything: (flush_voiced (F, S, hop), flush_len (F, S)), or
        None for an events-only segmenter.  The streams are then ended: reset()
        (or zero a stream's slices) before pushing again."""
        lib = _lib.lib()
        head = (self.n,) + ((self._is_scores,) if self._op else ()) + self._params + self._tables
        st = _lib.stream_ptr(stream)
        if self.history is None:
            _lib.check(getattr(lib, self._events_flush_fn)(*head, st), self._events_flush_fn)
            return None
        _lib.check(getattr(lib, self._flush_fn)(*head, _lib.ptr(self.history), self.history.numel(),
                                                _lib.ptr(self.flush_voiced), _lib.ptr(self.flush_len), st),
                   self._flush_fn)
        return self.flush_voiced, self.flush_len

    def segments(self):
        """Per stream the (k_s, 2) int64 rows written so far, as numpy arrays -- synchronises."""
        found = self.found.cpu().numpy()
        table = self.table.cpu().numpy()
        return [table[s, :min(int(found[s]), self.capacity)].astype(np.int64).reshape(-1, 2) for s in range(self.n)]
