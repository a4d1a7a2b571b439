"""Many concurrent analyser streams on one GPU (BASELINE config 5).

Each of S streams behaves like its own ``SKLearnAnalyzer.feed_frame`` loop
(realtime_analysis/sklearn_analyser.py:46-82) fed with the 400-sample frame
that ends at the newest sample, advanced one hop (160 samples = 10 ms) per
step.  Two forms of a step, identical semantics:
  kernel="hop"    ONE HIP kernel, one wave per stream (vad_stream_hop): frame
                  assembly, FFT, mel / log / DCT, window features, FFN (exact
                  f32 on the VALU) -- latency first;
  kernel="three"  frame assembly (shift by one hop, append the new samples,
                  in place), the clip MFCC kernel, the window features + MFMA
                  FFN kernel -- three launches, replayable as one hipGraph.

labels[s] after a step is the class of stream s's window centred three steps
earlier, or 255 during each stream's first five steps (feed_frame returns
None for its first five calls, :48-50).

The classifier is an FFN or the decision tree vad.py deploys (vad.py:17,52):
with a TreeClassifier both forms end in a walk of the tree instead
(vad_stream_hops_tree: the node table staged in LDS, one wave-uniform path
per stream and hop; vad_stream_step_tree), and labels are class indices.

Host I/O (C5's end-to-end rate includes the copies):
attach_host_io() adds pinned host buffers ``host_inputs`` (K, S, hop) and
``host_labels`` (K, S); step_host() runs one step from the first to the
second -- the H2D copy of every stream's new samples, the hop kernel(s), the
D2H copy of the labels (vad.py:32-59's loop body for S streams at once) --
and capture(host_io=True) records exactly that into the graph, replayed
through vad_graph_launch (hipGraphLaunch, no runtime wrapper in between).

Blocks of hops: with hops_per_step=K a step advances every stream by K hops
(step_block), K x 10 ms of audio per stream, whose new samples sit in the
static input block ``inputs`` (K, S, hop) and whose labels land in
``label_block`` (K, S).  kernel="hop" runs the K hops in ONE launch
(vad_stream_hops: the plan tables staged once, the stream state carried in
registers from hop to hop); capture() records one block into a hipGraph that
reads ``inputs`` in place, so a producer that writes the next block there
(e.g. an H2D copy of the audio devices' buffers) replays with no copy at all.

int16 PCM: StreamBatch(..., input_dtype=torch.int16) takes the samples as
they are recorded (vad.py:37, recoder.py:24-25 cast them afterwards):
``inputs`` / ``hop_in`` / ``host_inputs`` are int16, step() / step_block()
read int16 device tensors in place (vad_stream_hops_i16, one 2-byte load per
sample, any element offset and stride), and the H2D copy of a block moves
half the bytes.  The kernels convert with an exact (float) on load; frames,
ring and counts stay fp32, so labels and state equal the fp32 batch's bit
for bit.

Scores: StreamBatch(..., scores=True, active=1) also keeps a static
``score_block`` (K, S) float32 next to ``label_block``: per hop and stream the
classifier's estimate in [0, 1] that the window is of class index ``active``
-- the FFN's softmax (vad_amd.scores.scores_from_logits' function) or the
tree leaf's class share (TreeClassifier.score_table) -- NaN where the label
is 255.  The hop kernel writes it (vad_stream_hops_scores and its _i16 /
tree forms: still one kernel, so a captured one-hop step stays one node) in
step, step_block (both layouts, in place) and graph replay; labels and state
equal those of a batch without scores.  kernel="three" has no scores.  The
host forms (step_host, HostPipeline) copy labels only: the scores stay on the
device, in ``score_block``, valid once the step has run.  segmenter(on=...,
off=..., pad=...) feeds them to the online segmenter.

Noise subtraction: StreamBatch(..., denoise=True, alpha=0.9, noise_class=0,
noise_update=True) makes the reference's dead spectral subtraction live
(sklearn_analyser.py:84-101 computes it, :122-123 drops it): per stream the
hop kernel keeps the power rows of the last five frames (``spec_ring``), up
to five noise rows in arrival order (``noise_rows``, ``noise_count``) and the
noise estimate (``noise_estimate``: the rows' mean, low-passed over the bins
with coefficient ``alpha``); a hop's MFCC row is taken from max(p - e, 0), and
a window labelled ``noise_class`` pushes the raw power row of its middle frame
into the noise rows (noise_update=False freezes them).  load_noise(frames)
is load_init_inactive_frames.  Every form of a hop step works as before
(vad_stream_hops_denoise and its _i16 / tree forms: still one kernel);
kernel="three" has no denoising.  All four are reported in the reference's
units |X/512|^2 (the kernels keep |2X|^2: an exact factor 2^-20).  Not covered:
the clip kernels (the loop is sequential in the frames), SKLearnAnalyzer,
SimpleStreamBatch.

Sessions: StreamBatch(..., sessions=True) lets streams join, leave and stall
inside the hop kernel (vad_stream_hops_sessions and its _i16 / tree forms:
still one kernel).  Two static device tensors are read at the start of every
step: ``hop_counts`` (S,) int32, initially K -- stream s takes n_s =
min(max(hop_counts[s], 0), K) hops from rows 0..n_s-1 of its column of the
input block -- and ``restart`` (S,) uint8, initially 0 -- nonzero: the stream's
state becomes what reset() makes it (with denoise=True its spectrum ring,
noise rows, noise count and estimate too) before its hops, and the kernel
stores 0 back, so a flag set once restarts once, also under graph replay.
Label rows n_s..K-1 of a stream hold LABEL_NO_HOP (254), its score rows NaN; a
stream with no hop and no restart keeps every byte of its state.  With all
counts K and no restart everything equals a batch without sessions, bit for
bit.  step / step_block take ``hop_counts=`` / ``restart=`` (copied into the
static tensors); the host forms copy ``host_hop_counts`` / ``host_restart`` in
before the kernel (the producer clears host_restart itself: the kernel
consumes the device copy only).  Combines with FFN or tree, scores, denoise,
int16 input, hops_per_step 1 or K, capture, step_host and HostPipeline (a
pair per slot).  segmenter(sessions=True) returns the online segmenter's
sessions form (vad_amd.stream_segments): it reads this batch's ``hop_counts``
(both kernels read it, neither writes it) and owns a ``restart`` of its own,
because the hop kernel has cleared the batch's by the time the segmenter
runs; step / step_block copy a ``restart=`` they are given into it as well, so
``sb.step_block(x, hop_counts=c, restart=r); seg.push(sb.label_block,
sb.inputs)`` is the whole loop.  A caller that writes ``sb.restart`` directly
(for a replayed graph) writes ``seg.restart`` too.  resampler(rates) returns
a SessionStreamResampler (vad_amd.resample) in front: callers at 8, 44.1 or
48 kHz, each session at the rate it started with.  It writes ``inputs``,
reads this batch's ``hop_counts`` and owns a third ``restart`` (and a
``rate_index`` read under that flag only), so
``rs.step_block(x, hop_counts=c, restart=r, rate=i); sb.step_block();
seg.push(sb.label_block, sb.inputs)`` is the whole loop with callers at their
own rates, a slot reused by a caller at another rate included.  Not covered:
kernel="three"; segmenter() without sessions=True (the plain online segmenter
counts one window per label row); feeding the segmenter or the resampler from
step_host / HostPipeline (the caller copies ``host_restart`` into
``seg.restart`` itself); the last ``delay`` output samples of a session that
ends behind a resampler (under 1.3 ms).

Blocks in flight: host_pipeline(depth) returns a HostPipeline with `depth`
slots, each with pinned host buffers and a device input / label block of its
own, and three streams (copy-in, compute, copy-out): submit(d) enqueues slot
d's H2D, kernel(s) and D2H, event-ordered, so block k+1's copy-in and block
k-1's copy-out overlap block k's kernel; wait(d) blocks the host on slot d's
D2H only.  All kernels run on the one compute stream in submit order: the
stream state carries exactly as in serial steps.
"""
from __future__ import annotations

import ctypes
import weakref

import torch

from . import _lib
from .config import MfccConfig
from .ffn import FFNClassifier
from .plan import MfccPlan
from .tree import TreeClassifier

_TREE_WALKS = {"auto": _lib.TREE_WALK_AUTO, "global": _lib.TREE_WALK_GLOBAL}
LABEL_NO_HOP = _lib.LABEL_NO_HOP  # VAD_LABEL_NO_HOP: a label row the stream has no hop in (sessions)


def hop_rows_disjoint(n_streams, n_hops, block_stride, hop_stride, hop_len):
    """The layouts vad_stream_hops reads in place (capi.hip
    vad_hop_layout_disjoint): one hop only, or hop rows that neither repeat
    nor overlap, in hop-major order ((K, S, hop) blocks) or stream-major
    order (an (S, K * hop) buffer viewed as (K, S, hop))."""
    if n_hops <= 1:
        return True
    if block_stride <= 0:
        return False
    return (block_stride >= (n_streams - 1) * hop_stride + hop_len
            or (block_stride >= hop_len and hop_stride >= (n_hops - 1) * block_stride + hop_len))


class StreamBatch:
    """S analyser streams with one classifier: an FFNClassifier (or its
    layers), or a decision tree -- a TreeClassifier, or a fitted sklearn
    DecisionTreeClassifier converted by TreeClassifier.from_sklearn, as
    VadPipeline takes them.  ``ffn`` and ``classifier`` both hold it.

    With a tree every form of a step is the FFN batch's (step, step_block in
    either layout, int16 input, kernel="three", capture, step_host,
    host_pipeline, segmenter); the hop kernel is vad_stream_hops_tree, the
    three-kernel form ends in vad_stream_step_tree.  ``label_block`` holds
    class *indices* (uint8) as TreeClassifier.window_labels gives them, 255
    during a stream's first five hops: ``classes_[index]`` is the value
    sklearn's predict returns, and segmenter(active=...) takes the index.
    tree_walk="auto" walks the node table from LDS when it fits
    (vad_stream_tree_max_lds_nodes) and from global memory otherwise;
    "global" always walks from global memory (same labels)."""
    _FOREST = False  # ForestStreamBatch: the classifier is a forest

    def __init__(self, n_streams, ffn, cfg: MfccConfig = MfccConfig(), device=None, kernel="hop",
                 hops_per_step=1, input_dtype=torch.float32, tree_walk="auto", scores=False, active=1,
                 denoise=False, alpha=0.9, noise_class=0, noise_update=True, sessions=False):
        self.sessions = bool(sessions)
        if self.sessions and kernel == "three":
            raise ValueError("sessions live in the one-kernel hop: kernel='three' has none")
        if input_dtype not in (torch.float32, torch.int16):
            raise ValueError("input_dtype must be torch.float32 or torch.int16")
        if tree_walk not in _TREE_WALKS:
            raise ValueError("tree_walk must be 'auto' or 'global'")
        from .forest import ForestClassifier
        self.is_forest = False
        if isinstance(ffn, ForestClassifier) or ForestClassifier.looks_like_sklearn_forest(ffn):
            if not self._FOREST:
                raise ValueError("StreamBatch's hop kernels walk one decision tree: a forest in the stream is a "
                                 "ForestStreamBatch (on clips: VadPipeline)")
            if not isinstance(ffn, ForestClassifier):
                ffn = ForestClassifier.from_sklearn(ffn)
            self.is_forest = True
            if kernel == "three":
                raise ValueError("a forest lives in the one-kernel hop: kernel='three' has none")
            if ffn.n_features > 3 * cfg.n_mfcc:
                raise ValueError(f"the forest reads {ffn.n_features} features; a window has 3 * n_mfcc = "
                                 f"{3 * cfg.n_mfcc}")
            if not 0 <= int(active) < len(ffn.classes_):  # the kernel averages class `active` with or without scores
                raise ValueError(f"active must be a class index below {len(ffn.classes_)}, got {active}")
            if denoise and not 0 <= int(noise_class) < len(ffn.classes_):
                raise ValueError(f"noise_class must be a class index below {len(ffn.classes_)}, got {noise_class}")
        elif self._FOREST:
            raise TypeError("ForestStreamBatch takes a ForestClassifier or a fitted sklearn forest or bagging")
        if not isinstance(ffn, (FFNClassifier, TreeClassifier, ForestClassifier)):
            ffn = TreeClassifier.from_sklearn(ffn) if TreeClassifier.looks_like_sklearn_tree(ffn) \
                else FFNClassifier(ffn)
        self.is_tree = isinstance(ffn, TreeClassifier)
        self.tree_walk = tree_walk
        if self.is_tree and ffn.n_features > 3 * cfg.n_mfcc:
            raise ValueError(f"the tree reads {ffn.n_features} features; a window has 3 * n_mfcc = {3 * cfg.n_mfcc}")
        if cfg.preemph is not None:
            raise ValueError("pre-emphasis is a clip-level stage (VadPipeline); streams take raw frames")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        if kernel not in ("hop", "three"):
            raise ValueError("kernel must be 'hop' or 'three'")
        if kernel == "hop" and cfg.window is not None:
            raise ValueError("the one-kernel hop has no analysis window; use kernel='three'")
        self.scores, self.active = bool(scores), int(active)
        if self.scores:
            if kernel == "three":
                raise ValueError("scores come from the one-kernel hop: kernel='three' has none")
            n_cls = len(ffn.classes_) if self.is_forest else ffn.score_classes() if self.is_tree \
                else int(ffn.layers[-1][1].shape[0])
            if not 0 <= self.active < n_cls:
                raise ValueError(f"active must be a class index below {n_cls}, got {active}")
        self.denoise = bool(denoise)
        if self.denoise:
            if kernel == "three":
                raise ValueError("noise subtraction lives in the one-kernel hop: kernel='three' has none")
            if cfg.fft_n != 512:
                raise ValueError("noise subtraction needs fft_n = 512 (the hop kernel's FFT)")
            self.alpha, self.noise_class, self.noise_update = float(alpha), int(noise_class), bool(noise_update)
            if not 0.0 <= self.alpha < 1.0:  # false for NaN
                raise ValueError(f"alpha must be in [0, 1), got {alpha}")
            n_cls = len(ffn.classes_) if self.is_forest \
                else 1 + max(int(c) for c, f in zip(ffn.leaf, ffn.feature) if f < 0) if self.is_tree \
                else int(ffn.layers[-1][1].shape[0])  # the tree's classes: those of its leaves
            if not 0 <= self.noise_class < n_cls:
                raise ValueError(f"noise_class must be a class index below {n_cls}, got {noise_class}")
        self.cfg, self.ffn, self.n, self.kernel = cfg, ffn, int(n_streams), kernel
        self.classifier = ffn
        self.plan = MfccPlan.from_config(cfg)
        S, L, H, C = self.n, cfg.frame_size, cfg.hop, cfg.n_mfcc
        if not 0 < H <= L:
            raise ValueError("hop must be in (0, frame_size]")
        K = int(hops_per_step)
        if K < 1:
            raise ValueError("hops_per_step must be >= 1")
        self.K = K
        self.input_dtype = input_dtype
        self._i16 = input_dtype == torch.int16
        self._dtype_name = "int16" if self._i16 else "float32"
        self.frames = torch.zeros((S, L), dtype=torch.float32, device=dev)
        # static graph inputs / outputs: K hops of new samples, K label rows
        self.inputs = torch.zeros((K, S, H), dtype=input_dtype, device=dev)
        self.hop_in = self.inputs[0]
        self.ring = torch.zeros((S, 5, C), dtype=torch.float32, device=dev)
        self.count = torch.zeros((S,), dtype=torch.int32, device=dev)
        self.label_block = torch.full((K, S), 255, dtype=torch.uint8, device=dev)
        self.labels = self.label_block[K - 1]
        self.score_block = torch.full((K, S), float("nan"), dtype=torch.float32, device=dev) if self.scores else None
        self.scratch = torch.zeros((S, C), dtype=torch.float32, device=dev)
        if self.denoise:  # the kernels' units |2X|^2; the properties below scale them
            self._spec = torch.zeros((S, 5, 256), dtype=torch.float32, device=dev)
            self._noise = torch.zeros((S, 5, 256), dtype=torch.float32, device=dev)
            self._est = torch.zeros((S, 256), dtype=torch.float32, device=dev)
            self.noise_count = torch.zeros((S,), dtype=torch.int32, device=dev)
        if self.sessions:  # read by the kernel at the start of every step; restart is consumed there
            self.hop_counts = torch.full((S,), K, dtype=torch.int32, device=dev)
            self.restart = torch.zeros((S,), dtype=torch.uint8, device=dev)
        self.graph = None
        self.graph_host_io = False
        self.host_inputs = None
        self.host_labels = None
        self._session_segmenters = weakref.WeakSet()  # segmenter(sessions=True): handed restart= by _set_sessions
        self._session_resamplers = weakref.WeakSet()  # resampler(rates): the same
        self.host_hop_counts = None
        self.host_restart = None

    _UNITS = 2.0 ** -20  # |2X|^2 -> |X/512|^2, exact

    def _need_denoise(self):
        if not self.denoise:
            raise ValueError("build the batch with denoise=True")

    @property
    def spec_ring(self):
        """(S, 5, 256) power rows |X/512|^2 of the last five frames; slot as ``ring``."""
        self._need_denoise()
        return self._spec * self._UNITS

    @property
    def noise_rows(self):
        """(S, 5, 256) noise rows in arrival order; the first noise_count[s] of stream s are held."""
        self._need_denoise()
        return self._noise * self._UNITS

    @property
    def noise_estimate(self):
        """(S, 256) the estimate the next hop subtracts."""
        self._need_denoise()
        return self._est * self._UNITS

    @property
    def block_waves(self):
        """Waves (streams) per block of this batch's hop launches on the
        current device: vad_stream_hop_block_waves, the rule the launcher
        itself applies.  kernel="hop" only."""
        if self.kernel != "hop":
            raise ValueError("block_waves is the one-kernel hop's launch shape: kernel='three' has none")
        lib = _lib.lib()
        if self.is_forest:
            nbytes = lib.vad_stream_hop_forest_table_bytes(self.plan.handle, self.ffn.plan.handle,
                                                           _TREE_WALKS[self.tree_walk])
        elif self.is_tree:
            nbytes = lib.vad_stream_hop_tree_table_bytes(self.plan.handle, self.ffn.plan.handle,
                                                         _TREE_WALKS[self.tree_walk])
        else:
            nbytes = lib.vad_stream_hop_table_bytes(self.plan.handle, self.ffn.plan.handle)
        if nbytes < 0:
            _lib.check(int(nbytes), "vad_stream_hop_table_bytes")
        waves = lib.vad_stream_hop_block_waves(nbytes, self.n, self.K)
        if waves < 0:
            _lib.check(int(waves), "vad_stream_hop_block_waves")
        return int(waves)

    def load_noise(self, frames):
        """frames (S, n, frame_size), n = 1..5, a CUDA tensor of the batch's
        input dtype: their power rows become the noise rows, in order, and
        the estimate is taken from them (load_init_inactive_frames)."""
        self._need_denoise()
        if frames.dim() != 3 or frames.shape[0] != self.n or not 1 <= frames.shape[1] <= 5 \
                or frames.shape[2] != self.cfg.frame_size or frames.dtype != self.input_dtype or not frames.is_cuda:
            raise ValueError(f"frames must be a CUDA {self._dtype_name} tensor of shape "
                             f"({self.n}, 1..5, {self.cfg.frame_size})")
        if frames.stride(2) != 1:
            frames = frames.contiguous()
        name = "vad_stream_noise_load_i16" if self._i16 else "vad_stream_noise_load"
        _lib.check(getattr(_lib.lib(), name)(
            self.plan.handle, ctypes.c_void_p(frames.data_ptr()), frames.stride(0), frames.stride(1),
            self.cfg.frame_size, frames.shape[1], self.n, _lib.ptr(self._noise), _lib.ptr(self.noise_count),
            _lib.ptr(self._est), self.alpha, _lib.stream_ptr()), name)

    def prime(self, carry):
        """Set the last frame_size - hop samples of every stream (S, L-H),
        float32 or int16 (converted exactly: the frames are fp32)."""
        L, H = self.cfg.frame_size, self.cfg.hop
        self.frames[:, H:].copy_(carry)

    def reset(self):
        self.frames.zero_()
        self.ring.zero_()
        self.count.zero_()
        self.label_block.fill_(255)
        if self.scores:
            self.score_block.fill_(float("nan"))
        if self.denoise:
            for t in (self._spec, self._noise, self._est, self.noise_count):
                t.zero_()
        if self.sessions:
            self.hop_counts.fill_(self.K)
            self.restart.zero_()

    def _set_sessions(self, hop_counts, restart):
        """Check the per-call tensors and copy them into the static ones."""
        if hop_counts is None and restart is None:
            return
        if not self.sessions:
            raise ValueError("hop_counts / restart: build the batch with sessions=True")
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
            for seg in self._session_segmenters:  # each consumes a flag of its own
                seg.restart.copy_(restart)
            for rs in self._session_resamplers:
                rs.restart.copy_(restart)

    def _hop_call(self, h, n_hops=1, labels=None, stream=None, sess=None):
        """vad_stream_hops (_i16 for an int16 batch) with the per-batch
        arguments prepared once (the Python side of a launch is a few
        microseconds of ctypes marshalling: per call only the hop block's
        address and strides change).  stream: a hipStream_t pointer, default
        the current stream.  sess: a sessions batch's (hop_counts, restart)
        pointers, default the batch's own tensors."""
        if getattr(self, "_hop_head", None) is None and self.is_forest:
            # one entry for every form: a null `scores`, denoise state or session pair switches that part off
            L = self.cfg.frame_size
            self._hop_name = "vad_stream_hops_forest" + ("_i16" if self._i16 else "")
            self._hop_scores = (self.active, _lib.ptr(self.score_block) if self.scores else None, self.n) + (
                (_lib.ptr(self._spec), _lib.ptr(self._noise), _lib.ptr(self.noise_count), _lib.ptr(self._est),
                 self.alpha, self.noise_class, int(self.noise_update)) if self.denoise
                else (None, None, None, None, 0.0, 0, 0))
            self._hop_sess = (_lib.ptr(self.hop_counts), _lib.ptr(self.restart)) if self.sessions else (None, None)
            self._hop_fn = getattr(_lib.lib(), self._hop_name)
            self._hop_head = (self.plan.handle, self.ffn.plan.handle, _lib.ptr(self.frames), L, L)
            self._hop_mid = (_lib.ptr(self.ring), _lib.ptr(self.count))
            self._hop_walk = (_TREE_WALKS[self.tree_walk],)
            self._hop_labels = {}
        if getattr(self, "_hop_head", None) is None:
            L = self.cfg.frame_size
            self._hop_name = ("vad_stream_hops_tree" if self.is_tree else "vad_stream_hops") + \
                ("_sessions" if self.sessions else "_denoise" if self.denoise else "_scores" if self.scores else "") + \
                ("_i16" if self._i16 else "")
            if self.scores and self.is_tree:
                self.ffn.plan_with_scores()
            # rows [0, n_hops) of score_block, whichever label rows the call writes
            self._hop_scores = (self.active, _lib.ptr(self.score_block), self.n) if self.scores else ()
            if self.denoise:  # the scored entry's arguments (scores may be null), then the state and the options
                self._hop_scores = (self._hop_scores or (0, None, 0)) + (
                    _lib.ptr(self._spec), _lib.ptr(self._noise), _lib.ptr(self.noise_count), _lib.ptr(self._est),
                    self.alpha, self.noise_class, int(self.noise_update))
            elif self.sessions:  # the denoising entry's arguments with a null state: no denoising
                self._hop_scores = (self._hop_scores or (0, None, 0)) + (None, None, None, None, 0.0, 0, 0)
            self._hop_sess = (_lib.ptr(self.hop_counts), _lib.ptr(self.restart)) if self.sessions else ()
            self._hop_fn = getattr(_lib.lib(), self._hop_name)
            self._hop_head = (self.plan.handle, self.ffn.plan.handle, _lib.ptr(self.frames), L, L)
            self._hop_mid = (_lib.ptr(self.ring), _lib.ptr(self.count))
            self._hop_walk = (_TREE_WALKS[self.tree_walk],) if self.is_tree else ()
            self._hop_labels = {}
        lab = self.labels if labels is None else labels
        key = (lab.data_ptr(), n_hops)
        tail = self._hop_labels.get(key)
        if tail is None:
            tail = (ctypes.c_void_p(lab.data_ptr()), lab.stride(0) if lab.dim() == 2 else 0)
            self._hop_labels[key] = tail
        rc = self._hop_fn(*self._hop_head, ctypes.c_void_p(h.data_ptr()), h.stride(-2), self.cfg.hop, self.n,
                          n_hops, h.stride(0) if h.dim() == 3 else 0, *self._hop_mid, *tail, *self._hop_walk,
                          *self._hop_scores, *(self._hop_sess if sess is None else sess),
                          _lib.stream_ptr() if stream is None else stream)
        if rc:
            _lib.check(rc, self._hop_name)

    def _three(self, h, labels, stream=None):
        L, H = self.cfg.frame_size, self.cfg.hop
        lib = _lib.lib()
        st = _lib.stream_ptr() if stream is None else stream
        push = lib.vad_stream_push_hop_i16 if self._i16 else lib.vad_stream_push_hop
        _lib.check(push(_lib.ptr(self.frames), L, L, ctypes.c_void_p(h.data_ptr()), h.stride(0), H, self.n, st),
                   "vad_stream_push_hop_i16" if self._i16 else "vad_stream_push_hop")
        step = lib.vad_stream_step_tree if self.is_tree else lib.vad_stream_step
        _lib.check(step(
            self.plan.handle, self.ffn.plan.handle, _lib.ptr(self.frames), L, L, self.n,
            _lib.ptr(self.ring), _lib.ptr(self.count), ctypes.c_void_p(labels.data_ptr()),
            _lib.ptr(self.scratch), st), "vad_stream_step_tree" if self.is_tree else "vad_stream_step")

    def _body(self, hop=None):
        """One hop (K = 1) from `hop` or the static input."""
        h = self.hop_in if hop is None else hop
        if self.kernel == "hop":
            self._hop_call(h)
        else:
            self._three(h, self.labels)

    def _block_body(self):
        """K hops from the static input block into label_block."""
        if self.kernel == "hop":
            self._hop_call(self.inputs, self.K, self.label_block)
        else:
            for k in range(self.K):
                self._three(self.inputs[k], self.label_block[k])

    def step(self, new_samples=None, hop_counts=None, restart=None):
        """Advance every stream by one hop (new_samples: (S, hop) device
        tensor of the batch's input dtype; None: the hop already written into
        ``hop_in``).  hops_per_step == 1.  A sessions batch: hop_counts (S,)
        int32 / restart (S,) uint8 device tensors are copied into the static
        ``hop_counts`` / ``restart`` first; None leaves those as written."""
        if self.K != 1:
            raise ValueError("this batch advances hops_per_step hops at a time: use step_block")
        self._set_sessions(hop_counts, restart)
        if new_samples is not None and (new_samples.shape != self.hop_in.shape
                                        or new_samples.dtype != self.input_dtype or not new_samples.is_cuda):
            raise ValueError(f"new_samples must be a CUDA {self._dtype_name} tensor of shape "
                             f"{tuple(self.hop_in.shape)}")
        if self.graph is not None and not self.graph_host_io:
            if new_samples is not None:
                self.hop_in.copy_(new_samples)
            self._replay()
        elif self.kernel == "hop" and new_samples is not None and new_samples.stride(1) == 1:
            self._body(new_samples)  # read in place: no copy
        else:
            if new_samples is not None:
                self.hop_in.copy_(new_samples)
            self._body()
        return self.labels

    def step_block(self, new_samples=None, hop_counts=None, restart=None):
        """Advance every stream by K = hops_per_step hops; new_samples: (K, S,
        hop) device tensor of the batch's input dtype, or None when the block was written into ``inputs``
        (the graph's static input: no copy).  Returns label_block (K, S).
        hop_counts / restart: as step (a stream takes min(max(count, 0), K)
        hops; the label rows past them hold LABEL_NO_HOP)."""
        self._set_sessions(hop_counts, restart)
        if new_samples is not None:
            if new_samples.shape != self.inputs.shape or new_samples.dtype != self.input_dtype \
                    or not new_samples.is_cuda:
                raise ValueError(f"new_samples must be a CUDA {self._dtype_name} tensor of shape "
                                 f"{tuple(self.inputs.shape)}")
            if (self.graph is None or self.graph_host_io) and self.kernel == "hop" and new_samples.stride(2) == 1 \
                    and hop_rows_disjoint(self.n, self.K, new_samples.stride(0), new_samples.stride(1), self.cfg.hop):
                self._hop_call(new_samples, self.K, self.label_block)  # read in place
                return self.label_block
            self.inputs.copy_(new_samples)
        if self.graph is not None and not self.graph_host_io:
            self._replay()
        else:
            self._block_body()
        return self.label_block

    def attach_host_io(self):
        """Pinned host buffers for step_host: host_inputs (K, S, hop) of the
        batch's input dtype, host_labels (K, S) uint8; a sessions batch also
        gets host_hop_counts (S,) int32 (K) and host_restart (S,) uint8 (0)."""
        if self.host_inputs is None:
            self.host_inputs = torch.zeros(tuple(self.inputs.shape), dtype=self.input_dtype, pin_memory=True)
            self.host_labels = torch.full(tuple(self.label_block.shape), 255, dtype=torch.uint8,
                                          pin_memory=True)
            if self.sessions:
                self.host_hop_counts = torch.full((self.n,), self.K, dtype=torch.int32, pin_memory=True)
                self.host_restart = torch.zeros((self.n,), dtype=torch.uint8, pin_memory=True)
        return self.host_inputs, self.host_labels

    def _host_body(self):
        self.inputs.copy_(self.host_inputs, non_blocking=True)
        if self.sessions:
            self.hop_counts.copy_(self.host_hop_counts, non_blocking=True)
            self.restart.copy_(self.host_restart, non_blocking=True)
        if self.K == 1:
            self._body()
        else:
            self._block_body()
        self.host_labels.copy_(self.label_block, non_blocking=True)

    def _replay(self):
        _lib.check(self._graph_launch(self._graph_plan, _lib.stream_ptr()), "vad_graph_plan_launch")

    def step_host(self):
        """One step (K hops) from ``host_inputs`` to ``host_labels``: H2D
        copy, the hop kernel(s), D2H copy, all on the current stream (the
        caller synchronises it before reading host_labels).  Replays the
        graph when capture(host_io=True) recorded one.  The copies are
        asynchronous: a producer rewrites host_inputs only once the stream
        has passed the previous step's H2D copy (a stream or event sync, as
        vad.py's loop would do before reading the labels anyway)."""
        if self.host_inputs is None:
            raise ValueError("attach_host_io() (or capture(host_io=True)) first")
        if self.graph is not None and self.graph_host_io:
            self._replay()
        else:
            self._host_body()
        return self.host_labels

    def capture(self, host_io=False):
        """Capture one step (K hops) into a hipGraph (torch.cuda.CUDAGraph);
        step() / step_block() replay it, reading the static ``inputs``.  With
        host_io the graph also holds the H2D copy from ``host_inputs`` and the
        D2H copy to ``host_labels`` (replayed by step_host)."""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        saved = (self.frames.clone(), self.ring.clone(), self.count.clone(), self.label_block.clone())
        saved_scores = self.score_block.clone() if self.scores else None
        dn_state = (self._spec, self._noise, self._est, self.noise_count) if self.denoise else ()
        if self.sessions:  # the warm-up consumes restart flags, and with host_io overwrites both tensors
            dn_state += (self.hop_counts, self.restart)
        dn_saved = [t.clone() for t in dn_state]
        if host_io:
            self.attach_host_io()
            body = self._host_body
        else:
            body = self._body if self.K == 1 else self._block_body
        with torch.cuda.stream(s):
            body()  # warm-up (first launch sets kernel attributes)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.frames.copy_(saved[0]); self.ring.copy_(saved[1])
        self.count.copy_(saved[2]); self.label_block.copy_(saved[3])
        if self.scores:
            self.score_block.copy_(saved_scores)
        for t, v in zip(dn_state, dn_saved):
            t.copy_(v)
        # keep_graph: the captured hipGraph_t stays alive beside its exec, so
        # the replay plan can read its nodes (vad_graph_plan_create: a
        # one-kernel-node graph -- the one-hop step -- is dispatched as its
        # node, whose host cost is a launch's, not hipGraphLaunch's)
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g):
            body()
        g.instantiate()
        self._drop_graph_plan()
        lib = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(lib.vad_graph_plan_create(ctypes.c_void_p(g.raw_cuda_graph()),
                                             ctypes.c_void_p(g.raw_cuda_graph_exec()), ctypes.byref(h)),
                   "vad_graph_plan_create")
        self._graph_plan = h
        self._graph_launch = lib.vad_graph_plan_launch
        self._graph_plan_free = weakref.finalize(self, lib.vad_graph_plan_destroy, h)
        self.graph = g
        self.graph_host_io = bool(host_io)
        return g

    def host_pipeline(self, depth=2):
        """A HostPipeline over this batch: `depth` blocks of K hops in flight
        (H2D, kernel(s), D2H on three streams).  Launches are direct, not a
        graph; use either the pipeline or step()/step_block()/step_host()
        between two synchronisations, not both at once."""
        return HostPipeline(self, depth)

    def segmenter(self, sessions=False, **kw):
        """A StreamSegmenter (vad_amd.stream_segments) matching this batch's
        streams, framing, hops per step and input dtype; kw: max_gap, min_run,
        active, capacity, on, off, pad.  Feed it ``label_block`` and ``inputs``
        (or the blocks step_block read in place) after each step; with ``on``
        (the batch must have scores=True) feed it ``score_block`` instead, and
        ``active`` is the batch's.  A sessions batch takes sessions=True: the
        segmenter's ``hop_counts`` is this batch's tensor, and the ``restart=``
        given to step / step_block is copied into its ``restart`` too (the
        batch holds it weakly)."""
        from .stream_segments import StreamSegmenter
        if self.sessions and not sessions:
            raise ValueError("segmenter() on a sessions batch: the online segmenter counts one window per label "
                             "row, so a row of LABEL_NO_HOP would shift its clock; segmenter(sessions=True) "
                             "follows the per-stream hop counts and restarts")
        if sessions and not self.sessions:
            raise ValueError("segmenter(sessions=True): build the batch with sessions=True")
        if sessions:
            kw.update(sessions=True, hop_counts=self.hop_counts)
        if kw.get("on") is not None:
            if not self.scores:
                raise ValueError("segmenter(on=...) reads score_block: build the batch with scores=True")
            kw.setdefault("active", self.active)
        seg = StreamSegmenter(self.n, self.cfg, hops_per_step=self.K, audio_dtype=self.input_dtype,
                              device=self.frames.device, **kw)
        if sessions:
            self._session_segmenters.add(seg)
        return seg

    def resampler(self, rates, **kw):
        """A SessionStreamResampler (vad_amd.resample) in front of this
        sessions batch: its ``out`` is the batch's ``inputs``, its
        ``hop_counts`` the batch's tensor, and a ``restart=`` given to either's
        step is copied into the batch's, the resampler's and the session
        segmenters' flags (the batch holds the resampler weakly).  kw:
        input_dtype (of the callers' audio; the batch's input dtype is the
        resampler's output)."""
        from .resample import SessionStreamResampler
        if self.kernel == "three":
            raise ValueError("resampler(): sessions live in the one-kernel hop, kernel='three' has none")
        if not self.sessions:
            raise ValueError("resampler(): build the batch with sessions=True (a batch without sessions takes a "
                             "StreamResampler with out=inputs)")
        rs = SessionStreamResampler(self.n, rates, self.cfg, hops_per_step=self.K, out=self.inputs,
                                    hop_counts=self.hop_counts, batch=self, **kw)
        self._session_resamplers.add(rs)
        return rs

    @property
    def graph_direct(self):
        """True when replays dispatch the captured graph's single kernel node."""
        return self.graph is not None and bool(_lib.lib().vad_graph_plan_direct(self._graph_plan))

    def _drop_graph_plan(self):
        fin = getattr(self, "_graph_plan_free", None)
        if fin is not None:
            fin()  # the plan before the graph it points into
        self._graph_plan = None


class ForestStreamBatch(StreamBatch):
    """S analyser streams labelled and scored by a random forest: a
    ForestClassifier, or a fitted sklearn RandomForestClassifier,
    ExtraTreesClassifier or BaggingClassifier over decision trees
    (ForestClassifier.from_sklearn).  StreamBatch's arguments and methods, all
    through the one-kernel hop (vad_stream_hops_forest and its _i16 form; one
    wave per stream, lane l walking tree l): step, step_block in either
    layout, int16 input, capture, step_host, host_pipeline, segmenter
    (sessions=True and on= / off= / pad= included), resampler, scores=True with
    active=, denoise=True with noise_class below len(classes_), load_noise,
    sessions=True, tree_walk, block_waves.  kernel="three" raises ValueError.

    ``label_block`` holds indices into ``classes_`` (255 during a stream's
    first five hops); ``score_block`` holds float32(predict_proba[:, active]):
    what ForestClassifier.window_labels / window_scores give for the stream's
    MFCC rows, and so sklearn's predict_proba of those windows, bit for bit.
    tree_walk="auto" walks the first ``lds_trees`` trees from LDS and the rest
    from global memory; "global" walks every tree from global memory (same
    labels and scores)."""
    _FOREST = True

    @property
    def lds_trees(self):
        """The leading trees a launch stages in LDS (vad_stream_forest_lds_trees); 0 with tree_walk="global"."""
        if self.tree_walk == "global":
            return 0
        n = _lib.lib().vad_stream_forest_lds_trees(self.plan.handle, self.ffn.plan.handle)
        if n < 0:
            _lib.check(int(n), "vad_stream_forest_lds_trees")
        return int(n)


class HostPipeline:
    """`depth` blocks of a StreamBatch in flight between pinned host memory
    and the device (StreamBatch.host_pipeline).

    Slot d has pinned ``host_inputs[d]`` (K, S, hop; the batch's input dtype)
    and ``host_labels[d]`` (K, S; uint8), and a device input block and a device
    label block of its own; over a sessions batch also pinned
    ``host_hop_counts[d]`` / ``host_restart[d]`` and a device pair of its own,
    copied in with the input block (the batch's ``hop_counts`` / ``restart``
    are not read).  submit(d) enqueues
      the H2D copy of host_inputs[d] on the copy-in stream, after slot d's
        previous kernel has finished with the device input block;
      the hop kernel(s) on the compute stream, after that copy and after slot
        d's previous D2H copy has read the device label block;
      the D2H copy into host_labels[d] on the copy-out stream, after the kernel.
    Every submit's kernels go to the one compute stream, in submit order, so
    the streams' state (frames, ring, count) advances exactly as in serial
    steps; a depth of 1 is the serial order.  wait(d) blocks the host until
    slot d's D2H copy has landed and returns host_labels[d]; after it the
    producer may rewrite host_inputs[d].  The batch's own ``inputs`` /
    ``label_block`` / ``labels`` are not touched.
    """

    def __init__(self, batch, depth=2):
        depth = int(depth)
        if depth < 1:
            raise ValueError("depth must be >= 1")
        if batch.graph is not None:
            raise ValueError("a captured batch replays its graph; the pipeline launches directly")
        self.batch, self.depth = batch, depth
        dev = batch.frames.device
        ishape, lshape = tuple(batch.inputs.shape), tuple(batch.label_block.shape)
        self.host_inputs = [torch.zeros(ishape, dtype=batch.input_dtype, pin_memory=True) for _ in range(depth)]
        self.host_labels = [torch.full(lshape, 255, dtype=torch.uint8, pin_memory=True) for _ in range(depth)]
        self._dev_in = [torch.zeros(ishape, dtype=batch.input_dtype, device=dev) for _ in range(depth)]
        self._dev_lab = [torch.full(lshape, 255, dtype=torch.uint8, device=dev) for _ in range(depth)]
        if batch.sessions:  # a pair per slot: slot d + 1's copy-in may run while slot d's kernel reads its own
            S, K = batch.n, batch.K
            self.host_hop_counts = [torch.full((S,), K, dtype=torch.int32, pin_memory=True) for _ in range(depth)]
            self.host_restart = [torch.zeros((S,), dtype=torch.uint8, pin_memory=True) for _ in range(depth)]
            self._dev_cnt = [torch.full((S,), K, dtype=torch.int32, device=dev) for _ in range(depth)]
            self._dev_rst = [torch.zeros((S,), dtype=torch.uint8, device=dev) for _ in range(depth)]
            self._sess = [(_lib.ptr(c), _lib.ptr(r)) for c, r in zip(self._dev_cnt, self._dev_rst)]
        self.copy_in, self.compute, self.copy_out = (torch.cuda.Stream(device=dev) for _ in range(3))
        self._run_ptr = ctypes.c_void_p(self.compute.cuda_stream)
        self._h2d = [torch.cuda.Event() for _ in range(depth)]
        self._ran = [torch.cuda.Event() for _ in range(depth)]
        self._d2h = [torch.cuda.Event() for _ in range(depth)]
        self._busy = [False] * depth
        self._used = [False] * depth
        self._in_flight = 0
        cur = torch.cuda.current_stream(dev)
        for s in (self.copy_in, self.compute, self.copy_out):  # after the fills above
            s.wait_stream(cur)

    def submit(self, d):
        """Enqueue slot d's block (host_inputs[d] -> host_labels[d]); returns
        at once.  A slot submitted and not yet waited raises ValueError."""
        if not 0 <= d < self.depth:
            raise ValueError(f"slot must be in [0, {self.depth})")
        if self._busy[d]:
            raise ValueError(f"slot {d} was submitted and not waited")
        b = self.batch
        cur = torch.cuda.current_stream(b.frames.device)
        if self._in_flight == 0:  # idle: whatever the caller did to the state (prime, reset, steps) comes first
            self.compute.wait_stream(cur)
        used = self._used[d]
        try:
            if used:
                self.copy_in.wait_event(self._ran[d])
            torch.cuda.set_stream(self.copy_in)
            self._dev_in[d].copy_(self.host_inputs[d], non_blocking=True)
            if b.sessions:
                self._dev_cnt[d].copy_(self.host_hop_counts[d], non_blocking=True)
                self._dev_rst[d].copy_(self.host_restart[d], non_blocking=True)
            self._h2d[d].record(self.copy_in)
            self.compute.wait_event(self._h2d[d])
            if used:
                self.compute.wait_event(self._d2h[d])
            if b.kernel == "hop":
                b._hop_call(self._dev_in[d], b.K, self._dev_lab[d], self._run_ptr,
                            self._sess[d] if b.sessions else None)
            else:
                for k in range(b.K):
                    b._three(self._dev_in[d][k], self._dev_lab[d][k], self._run_ptr)
            self._ran[d].record(self.compute)
            self.copy_out.wait_event(self._ran[d])
            torch.cuda.set_stream(self.copy_out)
            self.host_labels[d].copy_(self._dev_lab[d], non_blocking=True)
            self._d2h[d].record(self.copy_out)
        finally:
            torch.cuda.set_stream(cur)
        self._busy[d] = True
        self._used[d] = True
        self._in_flight += 1

    def wait(self, d):
        """Block the host until slot d's labels are in host_labels[d]
        (returned).  Only the slot's D2H event is waited on."""
        if not 0 <= d < self.depth or not self._busy[d]:
            raise ValueError(f"slot {d} has no block in flight")
        self._d2h[d].synchronize()
        self._busy[d] = False
        self._in_flight -= 1
        return self.host_labels[d]

    def drain(self):
        """wait() on every slot in flight; the current stream then sees the
        batch's state as the last kernel left it."""
        for d in range(self.depth):
            if self._busy[d]:
                self.wait(d)
        torch.cuda.current_stream(self.batch.frames.device).wait_stream(self.compute)
