"""Clip-level (offline / batch) form of the hot path.

Reference call stack: dataset_creator.py -> Pool.map(
process_file) -> split_into_frames (file_processing.py:80-103) -> per-frame
get_mfcc -> 5-frame feature window (file_processing.py:40-70), with the
analyser's classifier applied to every window (sklearn_analyser.py:52-71).
Here a whole clip resident in HBM is framed, transformed and classified by
two HIP kernels (MFCC rows through a workspace) or one fused kernel (MFCC rows
kept on chip); the host only sizes buffers.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .config import MfccConfig
from .ffn import FFNClassifier
from .plan import MfccPlan, check_out, n_frames, preemphasis, window_features


def split_into_frames(data, frame_size, step, transcription_path=None, frame_rate=None):
    """file_processing.py:80-103 -- list of frame views while len - offset >
    size (with the STM segment gathering of :87-94, see vad_amd.dataset)."""
    from .dataset import split_into_frames as _split
    return _split(data, frame_size, step, transcription_path, frame_rate)


class VadPipeline:
    """MFCC plan + FFN for whole clips on one GPU.

    mode: "analyser" (normalised centre MFCC, sklearn_analyser.py:52-69) or
    "offline" (file_processing.py:40-70 features)."""

    def __init__(self, ffn=None, cfg: MfccConfig = MfccConfig(), mode="analyser"):
        """ffn: an FFNClassifier (or its layers), or a TreeClassifier / fitted
        sklearn DecisionTreeClassifier (the classifier vad.py deploys)."""
        from .forest import ForestClassifier
        from .tree import TreeClassifier
        self.cfg = cfg
        self.plan = MfccPlan.from_config(cfg)
        if ffn is not None and TreeClassifier.looks_like_sklearn_tree(ffn):
            ffn = TreeClassifier.from_sklearn(ffn)
        # a ForestClassifier (or a fitted sklearn forest / bagging of trees) runs
        # wherever the tree does on the two-kernel clip path
        if ffn is not None and ForestClassifier.looks_like_sklearn_forest(ffn):
            ffn = ForestClassifier.from_sklearn(ffn)
        if ffn is not None and not isinstance(ffn, (FFNClassifier, TreeClassifier, ForestClassifier)):
            ffn = FFNClassifier(ffn)
        self.ffn = ffn
        self.mode = _lib.FEAT_ANALYSER if mode == "analyser" else _lib.FEAT_OFFLINE
        self._ws = {}  # (device index, stream) -> workspace

    def n_frames(self, n_samples):
        return n_frames(n_samples, self.cfg.frame_size, self.cfg.hop)

    def _staged(self, audio, stream=None):
        """The clip after the optional pre-emphasis (cfg.preemph; off by default)."""
        if self.cfg.preemph is None:
            return audio
        if audio.dtype != torch.float32:
            audio = audio.float()
        return preemphasis(audio, self.cfg.preemph, stream=stream)

    def mfcc(self, audio, out=None, stream=None):
        """(F, n_mfcc) MFCCs of every frame of a device clip."""
        return self.plan.clip_mfcc(self._staged(audio, stream), self.cfg.frame_size, self.cfg.hop, out=out,
                                   stream=stream)

    def features(self, audio, mode=None, stream=None):
        """(F-5, 3*n_mfcc) feature rows of a device clip."""
        m = self.mfcc(audio, stream=stream)
        return window_features(m, self.mode if mode is None else mode, stream=stream)

    def workspace_bytes(self, n_samples):
        """Device bytes of the two-kernel clip path: the (F, n_mfcc) fp32 MFCC rows."""
        return int(_lib.lib().vad_mfcc_ffn_workspace_bytes(
            self.plan.handle, self.ffn.plan.handle, int(n_samples), self.cfg.frame_size, self.cfg.hop))

    @property
    def fusable(self):
        """The fused kernel (no workspace) applies: reference framing, the
        compiled 26-filter bank, a split-f16 FFN topology."""
        return isinstance(self.ffn, FFNClassifier) and bool(_lib.lib().vad_mfcc_ffn_fusable(
            self.plan.handle, self.ffn.plan.handle, self.cfg.frame_size, self.cfg.hop))

    def _workspace(self, need, device, stream):
        """Cached workspace per (device, stream): a buffer is never shared by
        work on two streams or handed to a kernel on another device."""
        s = stream if stream is not None else torch.cuda.current_stream(device)
        key = (device.index, s.cuda_stream)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            with torch.cuda.stream(s):
                ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=device)
            self._ws[key] = ws
        return ws

    def _at_rate(self, audio, rate, stream=None):
        """The clip at cfg.sample_rate: ``audio`` itself when rate is None or
        that rate, else its float32 conversion (vad_amd.resample)."""
        if rate is None or rate == self.cfg.sample_rate:
            return audio
        from .resample import resample_clips
        b = resample_clips([audio], rate, self.cfg, stream=stream)
        return b.data[:int(b.host["len"][0])]

    def _batch_at_rate(self, batch, rate, stream=None):
        """rate None: the ClipBatch as given; else ``batch`` is a sequence of
        clips (device tensors or host arrays) at ``rate`` (one rate or one per
        clip), converted into a ClipBatch at cfg.sample_rate."""
        if rate is None:
            return batch
        from .resample import resample_clips
        return resample_clips(batch, rate, self.cfg, stream=stream)

    def labels(self, audio, out=None, stream=None, fused=False, rate=None):
        """uint8 (F-5,) labels of every window of a device clip; float32
        samples, or int16 PCM as read from a wav file (identical labels).
        rate: the clip's sample rate when it is not cfg.sample_rate; the clip
        is then converted on the device first (None: taken as it is).
        fused=False: MFCC kernel + window kernel through a cached workspace
        (the faster form); fused=True: the single fused kernel, MFCC rows kept
        on chip (vad_mfcc_ffn with no workspace) -- identical labels."""
        if self.ffn is None:
            raise ValueError("pipeline has no FFN")
        if not (isinstance(audio, torch.Tensor) and audio.is_cuda
                and audio.dtype in (torch.float32, torch.int16) and audio.is_contiguous()):
            raise TypeError("audio must be a contiguous float32 or int16 CUDA tensor")
        audio = self._at_rate(audio, rate, stream)
        rows = max(self.n_frames(audio.numel()) - 5, 0)
        if out is None:
            out = torch.empty((rows,), dtype=torch.uint8, device=audio.device)
        else:
            check_out(out, (rows,), torch.uint8, audio.device, "out")
        if not isinstance(self.ffn, FFNClassifier):  # decision tree: MFCC, then windows
            if fused:
                raise ValueError("the fused kernel runs the FFN classifiers only (no decision tree, no forest)")
            return self.ffn.window_labels(self.mfcc(audio, stream=stream), self.mode, out=out,
                                          stream=stream)
        audio = self._staged(audio, stream)
        ws = None if fused else self._workspace(self.workspace_bytes(audio.numel()), audio.device, stream)
        fn = "vad_mfcc_ffn" if audio.dtype == torch.float32 else "vad_mfcc_ffn_i16"
        _lib.check(getattr(_lib.lib(), fn)(
            self.plan.handle, self.ffn.plan.handle, _lib.ptr(audio), audio.numel(),
            self.cfg.frame_size, self.cfg.hop, self.mode, _lib.ptr(out),
            _lib.ptr(ws), 0 if ws is None else ws.numel(), _lib.stream_ptr(stream)), fn)
        return out

    def scores(self, audio, active=1, out=None, stream=None, rate=None):
        """float32 (F-5,) speech scores of every window of a device clip
        (float32 or int16): the classifier's estimate in [0, 1] that the window
        is of class index ``active`` -- the softmax of the FFN's logits, or the
        class fraction of the tree's leaf (vad_amd.scores).  The windows and
        features are those of labels(); rate as there."""
        from .scores import scores_from_logits
        if self.ffn is None:
            raise ValueError("pipeline has no classifier")
        if not (isinstance(audio, torch.Tensor) and audio.is_cuda
                and audio.dtype in (torch.float32, torch.int16) and audio.is_contiguous()):
            raise TypeError("audio must be a contiguous float32 or int16 CUDA tensor")
        audio = self._at_rate(audio, rate, stream)
        mfcc = self.mfcc(audio, stream=stream)
        if not isinstance(self.ffn, FFNClassifier):
            return self.ffn.window_scores(mfcc, self.mode, active, out=out, stream=stream)
        from .plan import window_logits
        _, logits = window_logits(self.ffn.plan, mfcc, self.mode, stream=stream)
        return scores_from_logits(logits, active, out=out, stream=stream)

    def _decided(self, scores_or_labels, on, off, max_gap, min_run, pad, active, stream, batch=None):
        """The operating-point chain: scores -> hysteresis(on, off) (or the
        classifier's labels when on is None) -> close(max_gap) -> open(min_run)
        -> padding; uint8 0 / 1 for the segment stage with active = 1."""
        from . import scores as S
        from . import segments as G
        x = scores_or_labels
        if batch is None:
            lab = S.score_labels(x, on, off, stream=stream) if on is not None else x
            lab = G.smooth_labels(lab, max_gap, min_run, active=1 if on is not None else active, stream=stream)
            return S.dilate_labels(lab, pad, active=1, stream=stream)
        lab = S.batch_score_labels(x, batch, on, off, stream=stream) if on is not None else x
        lab = G.batch_smooth_labels(lab, batch, max_gap, min_run, active=1 if on is not None else active,
                                    stream=stream)
        return S.batch_dilate_labels(lab, batch, pad, active=1, stream=stream)

    def segments(self, audio, max_gap=0, min_run=0, active=1, capacity=None, stream=None, rate=None,
                 on=None, off=None, pad=(0, 0)):
        """Speech segments of a device clip: labels(), then
        vad_amd.segments.label_segments at the pipeline's framing (max_gap /
        min_run in windows).  Returns a Segments; no synchronisation.  With
        ``rate`` the segments are in samples of the converted clip.
        on / off / pad choose an operating point (vad_amd.scores): with ``on``
        the labels are decided from scores() by hysteresis (speech from a
        window with score >= on until one with score < off; off defaults to
        on), smoothed by max_gap / min_run, and every run then grows by
        pad = (before, after) windows.  Left at their defaults, the labels are
        the classifier's and nothing else runs."""
        from .segments import label_segments
        audio = self._at_rate(audio, rate, stream)
        if on is not None or tuple(pad) != (0, 0):
            x = self.scores(audio, active, stream=stream) if on is not None else self.labels(audio, stream=stream)
            lab = self._decided(x, on, off, max_gap, min_run, pad, active, stream)
            return label_segments(lab, audio.numel(), self.cfg.frame_size, self.cfg.hop, active=1,
                                  capacity=capacity, stream=stream)
        labels = self.labels(audio, stream=stream)
        return label_segments(labels, audio.numel(), self.cfg.frame_size, self.cfg.hop, max_gap=max_gap,
                              min_run=min_run, active=active, capacity=capacity, stream=stream)

    def voiced(self, audio, max_gap=0, min_run=0, active=1, stream=None, rate=None, on=None, off=None, pad=(0, 0)):
        """The voiced samples of a device clip (float32 or int16, bits
        copied), packed in order: segments(), then the device gather.  The
        result is trimmed to the voiced count, which lives on the device, so
        this call synchronises once (vad_amd.segments.voiced_audio is the form
        that does not).  With ``rate`` they are samples of the converted clip.
        on / off / pad: as segments()."""
        from .segments import voiced_audio
        audio = self._at_rate(audio, rate, stream)
        seg = self.segments(audio, max_gap=max_gap, min_run=min_run, active=active, stream=stream, on=on, off=off,
                            pad=pad)
        out, counts = voiced_audio(audio, seg, stream=stream)
        if stream is not None:
            stream.synchronize()
        return out[:int(counts[1].item())]

    # -- clip batches (vad_amd.batch.ClipBatch) ------------------------------
    def _check_batch(self, batch):
        from .batch import ClipBatch
        if not isinstance(batch, ClipBatch):
            raise TypeError("batch must be a ClipBatch")
        if (batch.frame_size, batch.hop) != (self.cfg.frame_size, self.cfg.hop):
            raise ValueError(f"the batch is packed for framing {(batch.frame_size, batch.hop)}, the pipeline "
                             f"frames at {(self.cfg.frame_size, self.cfg.hop)}")
        if self.cfg.preemph is not None:
            # pre-emphasis runs along the packed buffer and would carry the last
            # sample of one clip into the first of the next
            raise ValueError("cfg.preemph is not supported for clip batches")
        return batch

    def labels_batch(self, batch, stream=None, fused=False, rate=None):
        """The labels of every clip of a ClipBatch from ONE run of labels()
        over the packed buffer: a BatchLabels whose [k] is the view of clip
        k's labels, equal to labels(clip k).  FFN (both arithmetic modes) or
        decision tree; fused=True where ``fusable``.  No synchronisation.
        rate (here and in the other _batch forms): ``batch`` is then a
        sequence of clips at that rate, or at one rate each, converted into a
        ClipBatch on the device first (vad_amd.resample.resample_clips)."""
        from .batch import BatchLabels
        batch = self._batch_at_rate(batch, rate, stream)
        self._check_batch(batch)
        return BatchLabels(self.labels(batch.data, stream=stream, fused=fused), batch)

    def features_batch(self, batch, mode=None, packed=False, stream=None):
        """The feature rows of every clip of a ClipBatch from one run of
        features() over the packed buffer.  packed=False: a list of per-clip
        views of the global rows; packed=True: one contiguous (sum n_rows,
        3*n_mfcc) tensor, clip after clip (vad_batch_compact_rows)."""
        from .batch import compact_rows
        self._check_batch(batch)
        rows = self.features(batch.data, mode=mode, stream=stream)
        if packed:
            return compact_rows(rows, batch, stream=stream)
        h = batch.host
        return [rows[f0:f0 + r] for f0, r in zip(h["frame0"].tolist(), h["n_rows"].tolist())]

    def scores_batch(self, batch, active=1, stream=None, rate=None):
        """The scores of every clip of a ClipBatch from ONE run of scores()
        over the packed buffer: a BatchScores whose [k] is the view of clip
        k's scores, equal to scores(clip k).  No synchronisation."""
        from .scores import BatchScores
        batch = self._batch_at_rate(batch, rate, stream)
        self._check_batch(batch)
        return BatchScores(self.scores(batch.data, active, stream=stream), batch)

    def segments_batch(self, batch, max_gap=0, min_run=0, active=1, capacity=None, stream=None, rate=None,
                       on=None, off=None, pad=(0, 0)):
        """Speech segments of every clip of a ClipBatch: labels_batch(), then
        vad_amd.segments.batch_label_segments.  Returns a BatchSegments; no
        synchronisation.  on / off / pad: as segments(), every clip a sequence
        of its own."""
        from .segments import batch_label_segments
        batch = self._batch_at_rate(batch, rate, stream)
        if on is not None or tuple(pad) != (0, 0):
            x = (self.scores_batch(batch, active, stream=stream).scores if on is not None
                 else self.labels_batch(batch, stream=stream).labels)
            lab = self._decided(x, on, off, max_gap, min_run, pad, active, stream, batch=batch)
            return batch_label_segments(lab, batch, active=1, capacity=capacity, stream=stream)
        labels = self.labels_batch(batch, stream=stream)
        return batch_label_segments(labels, batch, max_gap=max_gap, min_run=min_run, active=active,
                                    capacity=capacity, stream=stream)

    def voiced_batch(self, batch, max_gap=0, min_run=0, active=1, stream=None, rate=None, on=None, off=None,
                     pad=(0, 0)):
        """The voiced samples of every clip of a ClipBatch, packed clip after
        clip: ``(voiced, offsets)`` with clip k's samples
        voiced[offsets[k]:offsets[k + 1]] (offsets: (n_clips + 1,) int64
        numpy).  Synchronises once, as voiced() does.  on / off / pad: as
        segments()."""
        from .segments import batch_voiced_audio
        batch = self._batch_at_rate(batch, rate, stream)
        seg = self.segments_batch(batch, max_gap=max_gap, min_run=min_run, active=active, stream=stream, on=on,
                                  off=off, pad=pad)
        out, _ = batch_voiced_audio(batch, seg, stream=stream)
        if stream is not None:
            stream.synchronize()
        meta = seg.meta.cpu().numpy()
        offsets = np.concatenate(([0], np.cumsum(meta[2 + 2 * batch.n_clips:]))).astype(np.int64)
        return out[:int(meta[1])], offsets

    def process_clip(self, data):
        """process_file's feature list for an in-memory clip: (F-5, 3, n_mfcc) float64
        (unnormalised, file_processing.py:40-70)."""
        a = torch.from_numpy(np.ascontiguousarray(np.asarray(data).astype(np.float32))).cuda()
        f = window_features(self.mfcc(a), _lib.FEAT_OFFLINE)
        return f.cpu().numpy().astype(np.float64).reshape(len(f), 3, -1)
