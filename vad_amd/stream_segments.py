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

Sessions: StreamSegmenter(..., sessions=True) -- or
StreamBatch.segmenter(sessions=True) on a sessions batch -- follows streams
that join, leave and stall inside a push (vad_stream_segments_sessions and its
_f32 / _i16 / _op forms: still one kernel).  Two static tensors are read at
the start of every push: ``hop_counts`` (S,) int32, initially K -- stream s
takes n_s = min(max(hop_counts[s], 0), k) hops from rows 0..n_s-1 of its
column of both blocks, the rows the sessions hop kernel consumed; rows past
n_s are never read and get voiced_len 0 -- and ``restart`` (S,) uint8: nonzero
ends the stream's running session before its hops (that stream's flush: rows
appended, the voiced prefixes in ``end_voiced`` (F, S, hop) / ``end_len``
(F, S), which is zero for every stream that ended nothing), makes the stream
fresh with a zero carry, and the kernel stores 0 back, so a flag set once
restarts once, also under graph replay.  ``table`` / ``found`` keep appending
across sessions; ``table_session`` (S, capacity) int32 holds each row's
session ordinal (restarts consumed so far) and session_segments() groups the
rows by it; sample positions start again at 0 in every session.  Per stream
and session the rows and the voiced prefixes -- push rows, then end rows --
equal a plain one-stream segmenter pushed with the session's hops and flushed,
bit for bit; a stream with no hop and no restart keeps every byte of its
state.  flush() ends every stream as before (and files the rows it appends
under each stream's ordinal); a later restart flag makes a stream live again.  A segmenter from StreamBatch.segmenter(sessions=True)
shares the batch's ``hop_counts`` and is handed the ``restart`` that step /
step_block are given; a caller that writes ``sb.restart`` directly (a replayed
graph) writes ``seg.restart`` too.  Not covered: step_host / HostPipeline (the
caller copies host_restart into ``seg.restart`` itself), a StreamResampler in
front, kernel="three", SimpleStreamBatch.

No call synchronises except segments() and session_segments().  One kernel per
push: capturable behind the hop kernel on the same stream.
"""
from __future__ import annotations

import contextlib

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
    only (no history, no voiced outputs).  sessions=True adds ``hop_counts``
    (S,) int32 (hop_counts=: a tensor to share, a sessions StreamBatch's),
    ``restart`` (S,) uint8, ``end_voiced`` (F, S, hop) / ``end_len`` (F, S)
    int32 and ``table_session`` (S, capacity) int32 (the module docstring)."""

    def __init__(self, n_streams, cfg: MfccConfig = MfccConfig(), max_gap=0, min_run=0, active=1, capacity=64,
                 hops_per_step=1, audio_dtype=None, device=None, on=None, off=None, pad=(0, 0), sessions=False,
                 hop_counts=None):
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
        self.sessions = bool(sessions)
        self.hop_counts = self.restart = self.end_voiced = self.end_len = self.table_session = None
        if hop_counts is not None and not self.sessions:
            raise ValueError("hop_counts: build the segmenter with sessions=True")
        if self.sessions:  # read by the kernel at the start of every push; restart is consumed there
            self._events_fn += "_sessions"
            if hop_counts is None:
                hop_counts = torch.full((S,), K, dtype=torch.int32, device=dev)
            elif not isinstance(hop_counts, torch.Tensor) or hop_counts.shape != (S,) or \
                    hop_counts.dtype != torch.int32 or hop_counts.device != dev or not hop_counts.is_contiguous():
                raise ValueError(f"hop_counts must be a contiguous int32 tensor of shape {(S,)} on the segmenter's "
                                 "device")
            self.hop_counts = hop_counts
            self.restart = torch.zeros((S,), dtype=torch.uint8, device=dev)
            self.end_len = torch.zeros((self.flush_rows, S), dtype=torch.int32, device=dev)
            self.table_session = torch.zeros((S, self.capacity), dtype=torch.int32, device=dev)
            self._rows = torch.arange(self.capacity, device=dev)[None, :]  # flush() files ordinals by row index
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
        if self.sessions:
            self.end_voiced = torch.zeros((self.flush_rows, S, H), dtype=audio_dtype, device=dev)
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
        if self.sessions:
            self.hop_counts.fill_(self.K)
            for t in (self.restart, self.end_len, self.table_session, self.end_voiced):
                if t is not None:
                    t.zero_()

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

    def _set_sessions(self, hop_counts, restart):
        """Check the per-call tensors and copy them into the static ones (as StreamBatch._set_sessions)."""
        if hop_counts is None and restart is None:
            return
        if not self.sessions:
            raise ValueError("hop_counts / restart: build the segmenter with sessions=True")
        for t, dst, name in ((hop_counts, self.hop_counts, "hop_counts"), (restart, self.restart, "restart")):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.shape != dst.shape or t.dtype != dst.dtype:
                raise ValueError(f"{name} must be a CUDA {str(dst.dtype).replace('torch.', '')} tensor of shape "
                                 f"{tuple(dst.shape)}")
        if hop_counts is not None:
            self.hop_counts.copy_(hop_counts)
        if restart is not None:
            self.restart.copy_(restart)

    def push(self, label_block, hop_block=None, hop_counts=None, restart=None, stream=None):
        """k <= K hops of every stream: label_block (k, S) uint8 as the hop
        kernels wrote it (strided rows are fine; (S,) for K = 1) -- with ``on``
        set, the (k, S) float32 score block instead -- hop_block
        (k, S, hop) the samples they read, in any layout vad_stream_hops
        reads in place.  Returns (voiced, voiced_len) -- the static outputs,
        rows [0, k) written -- or None without audio.  A sessions segmenter:
        hop_counts (S,) int32 / restart (S,) uint8 device tensors are copied
        into the static ``hop_counts`` / ``restart`` first (None leaves those
        as written), and the return is (voiced, voiced_len, end_voiced,
        end_len); events only, None (``end_len`` is still written)."""
        lab = self._check_labels(label_block)
        self._set_sessions(hop_counts, restart)
        k = lab.shape[0]
        lib = _lib.lib()
        sess = ()
        if self.sessions:
            sess = (_lib.ptr(self.hop_counts), _lib.ptr(self.restart)) + \
                ((_lib.ptr(self.end_voiced),) if hop_block is not None else ()) + \
                (_lib.ptr(self.end_len), _lib.ptr(self.table_session))
        head = (_lib.ptr(lab),) + ((self._is_scores,) if self._op else ()) + \
            (lab.stride(0) if k > 1 else 0, self.n, k, self.active) + self._params + self._tables
        st = _lib.stream_ptr(stream)
        if hop_block is None:
            _lib.check(getattr(lib, self._events_fn)(*head, *sess, st), self._events_fn)
            return None
        hop = self._check_hops(hop_block, k)
        _lib.check(getattr(lib, self._fn)(*head, _lib.ptr(hop), hop.stride(1), hop.stride(0) if k > 1 else 0,
                                          _lib.ptr(self.history), self.history.numel(), _lib.ptr(self.voiced),
                                          _lib.ptr(self.voiced_len), *sess, st), self._fn)
        if self.sessions:
            return self.voiced, self.voiced_len, self.end_voiced, self.end_len
        return self.voiced, self.voiced_len

    def flush(self, stream=None):
        """Decide everything: (flush_voiced (F, S, hop), flush_len (F, S)), or
        None for an events-only segmenter.  The streams are then ended: reset()
        (or zero a stream's slices) before pushing again; a sessions segmenter
        makes a stream live again with its restart flag.  The flush entries
        know no sessions, so a sessions segmenter files the rows this flush
        appended under each stream's ordinal in ``table_session`` itself: a
        copy of ``found`` before the kernel and three tensor operations after
        it, on the same stream as the kernel (``stream``, a torch stream, or
        the current one), without synchronising; they allocate temporaries of
        (S, capacity) elements, so this is not for a per-hop path."""
        lib = _lib.lib()
        head = (self.n,) + ((self._is_scores,) if self._op else ()) + self._params + self._tables
        st = _lib.stream_ptr(stream)
        before = None
        if self.sessions and self.capacity:
            with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
                before = self.found.clone()
        if self.history is None:
            _lib.check(getattr(lib, self._events_flush_fn)(*head, st), self._events_flush_fn)
        else:
            _lib.check(getattr(lib, self._flush_fn)(*head, _lib.ptr(self.history), self.history.numel(),
                                                    _lib.ptr(self.flush_voiced), _lib.ptr(self.flush_len), st),
                       self._flush_fn)
        if before is not None:
            # the flush entries know no sessions: the rows they appended, [found before, found after), are
            # filed under each stream's ordinal (pad[0] of its state) by tensor ops behind the kernel
            with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
                new = (self._rows >= before[:, None]) & (self._rows < self.found[:, None])
                ordinal = self.state.view(torch.int32)[:, 30:31]
                self.table_session.copy_(torch.where(new, ordinal, self.table_session))
        return None if self.history is None else (self.flush_voiced, self.flush_len)

    def segments(self):
        """Per stream the (k_s, 2) int64 rows written so far, as numpy arrays -- synchronises."""
        found = self.found.cpu().numpy()
        table = self.table.cpu().numpy()
        return [table[s, :min(int(found[s]), self.capacity)].astype(np.int64).reshape(-1, 2) for s in range(self.n)]

    def session_segments(self):
        """Per stream a list of (ordinal, (k, 2) int64 rows) pairs, in the order
        the sessions ran: the rows written so far grouped by ``table_session``
        (sessions without a row are absent) -- synchronises."""
        if not self.sessions:
            raise ValueError("session_segments(): build the segmenter with sessions=True")
        rows = self.segments()
        ordinal = self.table_session.cpu().numpy()
        out = []
        for s in range(self.n):
            o = ordinal[s, :len(rows[s])]
            cuts = np.flatnonzero(np.diff(o)) + 1
            out.append([(int(o[i]), rows[s][i:j]) for i, j in zip(np.r_[0, cuts], np.r_[cuts, len(o)]) if j > i])
        return out
