"""Many live ``SimpleAnalyser`` streams on one GPU, state on the device.

Each of S streams behaves like its own ``SimpleAnalyser.feed_frame`` loop
(realtime_analysis/simple_analyzer.py:78-112): per frame the seven features
(stEnergy, ZCR, spectral std, four 1-kHz band energies), the two
classification paths against the adaptive thresholds, the 20-frame status
buffer, the silence state, and the noise buffer with its exponential
threshold updates.  Within a block of K frames the features of every
(stream, frame) pair do not depend on state, so one launch computes all
K x S rows in parallel and then steps each stream's state machine K times
(vad_simple_stream_block_f32 / _i16: one workgroup per stream, the wave body
of vad_simple_features, the rows in LDS).  Frame sizes whose transform
length is not a power of two up to 4096 (401 samples: L = 513) take two
launches, vad_simple_features and the state steps, fp32 input only.

``label_block`` (K, S) uint8 holds 1 (active, feed_frame's True) / 0.  With
``voiced=True`` every block also leaves each stream's active frames packed
in order in ``voiced`` (S, K * frame_size), ``voiced_len`` (S,) samples of it
valid: vad.py:52-57's ``active_frames += np_frame.tobytes()``.

The state layout is include/vad_amd.h's; ``analyser(s)`` / ``from_analysers``
move a stream to and from the single-stream host class.

Sessions (``sessions=True``): callers that join, leave and stall, without a
host step.  Every block reads three static per-stream tensors inside the
kernel (vad_simple_stream_block_sessions_f32 / _i16, and
vad_simple_stream_state_sessions on the two-launch path):

* ``frame_counts`` (S,) int32, initially K: stream s takes
  ``min(max(frame_counts[s], 0), k)`` frames, the first rows of its column of
  the k-frame block.
* ``restart`` (S,) uint8: nonzero makes the stream fresh before its frames of
  this block; the kernel stores 0 back, so a flag set once restarts once,
  also when a captured graph is replayed.
* ``init_left`` (S,) int32: the frames a stream still needs before it is
  initialised.  A fresh stream has an all-zero state record and
  ``init_left = noise_buf_len``; a sessions batch starts with every stream
  fresh and never raises "Analyser not initialized".

A fresh stream's next noise_buf_len frames are its init frames, whichever
blocks they arrive in: vad.py:45-49 per caller, on the device.  Each one's
feature row fills a noise row, and the last does what
``load_init_inactive_frames`` does on those frames (thresholds the plain
means, status cleared, silence on); frames after it in the same block are
classified.  Init frames are labelled ``LABEL_INIT`` (253) and never packed
into ``voiced``; label rows past a stream's count hold ``LABEL_NO_HOP`` (254)
and its ``features`` rows there are not written (the two-launch path computes
every row).  ``voiced_len`` counts the frames labelled 1.  A stream with no
frame and no restart keeps every byte of its state and its ``init_left``; a
restart with no frame leaves the stream fresh.  With every count k, no restart
and every ``init_left`` 0 (after ``load_init_inactive_frames`` or
``from_analysers``, which set it) a sessions batch computes what a plain one
does, bit for bit.
"""
from __future__ import annotations

import ctypes
import weakref

import numpy as np
import torch

from . import _lib
from .simple_analyser import SimpleAnalyser
from .stream import hop_rows_disjoint

STATUS_BITS = SimpleAnalyser.TEMP_BUFFER_SIZE
N_FEATS = 7
LABEL_NO_HOP = _lib.LABEL_NO_HOP  # VAD_LABEL_NO_HOP: a label row the stream has no frame in (sessions)
LABEL_INIT = _lib.LABEL_INIT      # VAD_LABEL_INIT: a label row that holds one of the stream's init frames (sessions)
NOISE_COLS = 6                    # energy, std, band 0..3
_NOISE_FROM_FEAT = [0, 2, 3, 4, 5, 6]  # columns of a feature row kept in a noise row


def state_doubles(noise_buf_len):
    """Doubles per stream of the device state: the noise rows, six
    thresholds, four int32 (status, silence, noise_pointer, frame_number)."""
    return NOISE_COLS * int(noise_buf_len) + 6 + 2


def fft_geometry(frame_rate, frame_size):
    """(fftn, pad, band_bins) of :221-236, as SimpleAnalyser chooses them."""
    frame_size = int(frame_size)
    val = 2
    while val < frame_size:
        val <<= 1
    pad = (val - frame_size) // 2 + (val - frame_size) % 2
    band_bins = int(1000 / ((frame_rate + 0.0) / (val + 0.0)))
    return val, pad, band_bins


def one_kernel_length(L):
    """True when the block kernel takes the transform length L."""
    return 2 <= L <= 4096 and L & (L - 1) == 0


class SimpleStreamBatch:
    """S SimpleAnalyser streams advanced ``frames_per_step`` frames per call.

    ``features=True`` keeps the rows the kernel classified in ``features``
    (K, S, 7) float64 (always kept where the two-launch path needs them).
    ``sessions=True``: per-stream frame counts, restarts and in-kernel
    initialisation (the module docstring has the rules)."""

    def __init__(self, n_streams, frame_rate, frame_size, noise_buf_len, frames_per_step=1,
                 input_dtype=torch.float32, voiced=False, device=None, features=False, sessions=False):
        S, K, nb = int(n_streams), int(frames_per_step), int(noise_buf_len)
        if S < 1:
            raise ValueError("n_streams must be >= 1")
        if K < 1:
            raise ValueError("frames_per_step must be >= 1")
        if not 1 <= nb <= _lib.SIMPLE_MAX_NOISE:
            raise ValueError(f"noise_buf_len must be in 1..{_lib.SIMPLE_MAX_NOISE}")
        if input_dtype not in (torch.float32, torch.int16):
            raise ValueError("input_dtype must be torch.float32 or torch.int16")
        frame_size = int(frame_size)
        if not 2 <= frame_size <= 8192:
            raise ValueError("frame_size must be in 2..8192")
        self.frame_rate, self.frame_size, self.noise_buf_len = frame_rate, frame_size, nb
        self.fftn, self.fft_extended_zeros, self.fftn_for_band = fft_geometry(frame_rate, frame_size)
        self.spectral_bands = 4
        if self.fftn_for_band < 1 or self.fftn < self.spectral_bands * self.fftn_for_band:
            raise Exception("Can't get spectral bands. FFTN is small")
        self.fft_len = frame_size + 2 * self.fft_extended_zeros
        self.one_kernel = one_kernel_length(self.fft_len)
        self._i16 = input_dtype == torch.int16
        if self._i16 and not self.one_kernel:
            raise ValueError(f"int16 input needs a power-of-two transform length <= 4096; frame_size {frame_size} "
                             f"gives {self.fft_len}")
        if K * frame_size > 2 ** 31 - 1:
            raise ValueError("frames_per_step * frame_size must fit in int32")
        self.n, self.K, self.input_dtype = S, K, input_dtype
        self._dtype_name = "int16" if self._i16 else "float32"
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.device = dev
        self.state = torch.zeros((S, state_doubles(nb)), dtype=torch.float64, device=dev)
        self._ints = self.state.view(torch.int32)[:, 2 * (NOISE_COLS * nb + 6):]
        self.inputs = torch.zeros((K, S, frame_size), dtype=input_dtype, device=dev)
        self.label_block = torch.zeros((K, S), dtype=torch.uint8, device=dev)
        self.labels = self.label_block[K - 1]
        self.features = torch.zeros((K, S, N_FEATS), dtype=torch.float64, device=dev) \
            if features or not self.one_kernel else None
        self.voiced = torch.zeros((S, K * frame_size), dtype=input_dtype, device=dev) if voiced else None
        self.voiced_len = torch.zeros((S,), dtype=torch.int32, device=dev) if voiced else None
        self.sessions = bool(sessions)
        self.frame_counts = self.restart = self.init_left = None
        if self.sessions:  # static: a captured graph reads them in place
            self.frame_counts = torch.full((S,), K, dtype=torch.int32, device=dev)
            self.restart = torch.zeros((S,), dtype=torch.uint8, device=dev)
            self.init_left = torch.full((S,), nb, dtype=torch.int32, device=dev)  # every stream fresh
        self.initialized = self.sessions  # each stream of a sessions batch initialises itself
        self.graph = None
        self._fn_name = "vad_simple_stream_block" + ("_sessions" if self.sessions else "") + \
            ("_i16" if self._i16 else "_f32")
        self._fn = None

    # -- state views (read-only: they alias the device state) -------------------
    @property
    def noise_feats(self):
        """(S, noise_buf_len, 6): energy, std, band 0..3 of the noise frames."""
        nb = self.noise_buf_len
        return self.state[:, :NOISE_COLS * nb].view(self.n, nb, NOISE_COLS)

    @property
    def energy_thresh(self):
        return self.state[:, NOISE_COLS * self.noise_buf_len]

    @property
    def spectral_std_thresh(self):
        return self.state[:, NOISE_COLS * self.noise_buf_len + 1]

    @property
    def spectral_energy_bands_thresh(self):
        t = NOISE_COLS * self.noise_buf_len + 2
        return self.state[:, t:t + 4]

    @property
    def silence(self):
        return self._ints[:, 1] != 0

    @property
    def noise_pointer(self):
        return self._ints[:, 2]

    @property
    def frame_number(self):
        return self._ints[:, 3]

    @property
    def temp_buffer(self):
        """(S, 20) bool, oldest entry first (SimpleAnalyser.temp_buffer)."""
        sh = torch.arange(STATUS_BITS - 1, -1, -1, dtype=torch.int32, device=self.state.device)
        return ((self._ints[:, 0:1] >> sh) & 1).bool()

    # -- reference API for S streams -----------------------------------------------
    def _frame_features(self, frames2d):
        x = frames2d.to(torch.float32).contiguous()
        out = torch.empty((x.shape[0], N_FEATS), dtype=torch.float64, device=x.device)
        _lib.check(_lib.lib().vad_simple_features(
            _lib.ptr(x), x.shape[0], self.frame_size, self.frame_size, self.fft_len, self.fft_extended_zeros,
            self.fftn_for_band, self.spectral_bands, _lib.ptr(out), _lib.stream_ptr()), "vad_simple_features")
        return out

    def load_init_inactive_frames(self, frames):
        """:120-138 for every stream: frames (S, noise_buf_len, frame_size) on
        the device, float32 or int16."""
        if frames.dim() != 3 or frames.shape[0] != self.n:
            raise ValueError(f"frames must be (n_streams, noise_buf_len, frame_size) with n_streams = {self.n}")
        if frames.shape[1] != self.noise_buf_len:
            raise Exception("Expected " + str(self.noise_buf_len) + " initial frames. Got " + str(frames.shape[1]))
        self._check_frame_size(frames)
        if not frames.is_cuda:
            raise ValueError("frames must be a CUDA tensor")
        feats = self._frame_features(frames.reshape(-1, self.frame_size))
        _lib.check(_lib.lib().vad_simple_stream_init(_lib.ptr(feats), self.n, self.noise_buf_len, _lib.ptr(self.state),
                                                     _lib.stream_ptr()), "vad_simple_stream_init")
        if self.sessions:
            self.init_left.zero_()
        self.initialized = True

    def reset(self):
        """Back to a batch before load_init_inactive_frames (sessions: every
        stream fresh, the counts K, no restart pending)."""
        self.state.zero_()
        self.label_block.zero_()
        if self.voiced_len is not None:
            self.voiced_len.zero_()
        if self.sessions:
            self.frame_counts.fill_(self.K)
            self.restart.zero_()
            self.init_left.fill_(self.noise_buf_len)
        self.initialized = self.sessions

    def _set_sessions(self, frame_counts, restart):
        """Check the per-call tensors and copy them into the static ones."""
        if frame_counts is None and restart is None:
            return
        if not self.sessions:
            raise ValueError("frame_counts / restart: build the batch with sessions=True")
        for t, dst, name in ((frame_counts, self.frame_counts, "frame_counts"), (restart, self.restart, "restart")):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.shape != dst.shape or t.dtype != dst.dtype:
                raise ValueError(f"{name} must be a CUDA {str(dst.dtype).replace('torch.', '')} tensor of shape "
                                 f"{tuple(dst.shape)}")
        if frame_counts is not None:
            self.frame_counts.copy_(frame_counts)
        if restart is not None:
            self.restart.copy_(restart)

    def _check_frame_size(self, frames):
        if frames.shape[-1] != self.frame_size:
            raise Exception("Wrong frame size. Expected " + str(self.frame_size) + " bytes. Got "
                            + str(frames.shape[-1]))

    def _launch(self, x, k, stream=None):
        """One block of k <= K frames from x (k, S, frame_size), samples contiguous."""
        if self._fn is None:
            self._fn = getattr(_lib.lib(), self._fn_name)
            L = self.frame_size
            self._head = (L, self.fft_len, self.fft_extended_zeros, self.fftn_for_band, self.n)
            self._tail = (self.noise_buf_len, _lib.ptr(self.state), _lib.ptr(self.label_block), self.n,
                          _lib.ptr(self.features), _lib.ptr(self.voiced), self.K * L, _lib.ptr(self.voiced_len))
            if self.sessions:
                self._tail += (_lib.ptr(self.frame_counts), _lib.ptr(self.restart), _lib.ptr(self.init_left))
        rc = self._fn(ctypes.c_void_p(x.data_ptr()), x.stride(0), x.stride(1), *self._head, k, *self._tail,
                      _lib.stream_ptr() if stream is None else stream)
        if rc:
            _lib.check(rc, self._fn_name)

    def _block_body(self):
        self._launch(self.inputs, self.K)

    def step_block(self, frames=None, frame_counts=None, restart=None):
        """Advance every stream by a block of frames: (k, S, frame_size) of the
        batch's input dtype on the device, k <= frames_per_step (a short block
        is the tail of a sequence), or None for the K frames already written
        into ``inputs``.  Returns the static label_block (its first k rows
        for a short block).  sessions: frame_counts (S,) int32 / restart (S,)
        uint8 CUDA tensors are copied into the static ones first; None leaves
        those as written."""
        self._set_sessions(frame_counts, restart)
        if not self.initialized:
            raise Exception("Analyser not initialized")
        k = self.K
        if frames is not None:
            self._check_frame_size(frames)
            if frames.dim() != 3 or frames.shape[1] != self.n or not 1 <= frames.shape[0] <= self.K \
                    or frames.dtype != self.input_dtype or not frames.is_cuda:
                raise ValueError(f"frames must be a CUDA {self._dtype_name} tensor of shape (k, {self.n}, "
                                 f"{self.frame_size}) with 1 <= k <= {self.K}")
            k = frames.shape[0]
            in_place = frames.stride(2) == 1 and (self.n == 1 or frames.stride(1) >= self.frame_size) and \
                hop_rows_disjoint(self.n, k, frames.stride(0), frames.stride(1), self.frame_size)
            if in_place and (self.graph is None or k < self.K):
                self._launch(frames, k)  # read in place: no copy
                return self.label_block if k == self.K else self.label_block[:k]
            self.inputs[:k].copy_(frames)
        if self.graph is not None and k == self.K:
            _lib.check(self._graph_launch(self._graph_plan, _lib.stream_ptr()), "vad_graph_plan_launch")
        else:
            self._launch(self.inputs, k)
        return self.label_block if k == self.K else self.label_block[:k]

    def step(self, frames=None, frame_counts=None, restart=None):
        """One frame of every stream: (S, frame_size), or None for the frame in
        ``inputs[0]``.  frames_per_step == 1.  Returns ``labels`` (S,).
        frame_counts / restart: as for step_block."""
        if self.K != 1:
            raise ValueError("this batch advances frames_per_step frames at a time: use step_block")
        self._set_sessions(frame_counts, restart)
        if frames is not None:
            if not self.initialized:
                raise Exception("Analyser not initialized")
            self._check_frame_size(frames)
            if frames.dim() != 2:
                raise ValueError(f"frames must be ({self.n}, {self.frame_size})")
            frames = frames.unsqueeze(0)
        self.step_block(frames)
        return self.labels

    def capture(self):
        """Capture one block of K frames into a hipGraph that reads the static
        ``inputs``; step() / step_block() replay it."""
        if not self.initialized:
            raise Exception("Analyser not initialized")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        # sessions: the warm-up consumes restart flags and init frames
        keep = [t for t in (self.state, self.label_block, self.features, self.voiced, self.voiced_len,
                            self.frame_counts, self.restart, self.init_left) if t is not None]
        saved = [t.clone() for t in keep]
        with torch.cuda.stream(s):
            self._block_body()  # warm-up (first launch sets kernel attributes)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        for t, v in zip(keep, saved):
            t.copy_(v)
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g):
            self._block_body()
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
        return g

    def _drop_graph_plan(self):
        fin = getattr(self, "_graph_plan_free", None)
        if fin is not None:
            fin()  # the plan before the graph it points into
        self._graph_plan = None

    # -- moving a stream to / from the host class ------------------------------------
    def analyser(self, s):
        """A host SimpleAnalyser loaded with stream s's state."""
        row = self.state[s].cpu()
        d = row.numpy()
        w = row.view(torch.int32).numpy()[2 * (NOISE_COLS * self.noise_buf_len + 6):]
        nb = self.noise_buf_len
        sa = SimpleAnalyser(self.frame_rate, self.frame_size, nb)
        sa._noise_feats[:, _NOISE_FROM_FEAT] = d[:NOISE_COLS * nb].reshape(nb, NOISE_COLS)
        t = NOISE_COLS * nb
        sa.energy_thresh = np.float64(d[t])
        sa.spectral_std_thresh = np.float64(d[t + 1])
        sa.spectral_energy_bands_thresh = d[t + 2:t + 6].copy()
        bits = int(w[0])
        sa.temp_buffer = [bool((bits >> (STATUS_BITS - 1 - j)) & 1) for j in range(STATUS_BITS)]
        sa.silence = bool(w[1])
        sa.noise_pointer = int(w[2])
        sa.frame_number = int(w[3])
        sa.initialized = int(self.init_left[s]) == 0 if self.sessions else self.initialized
        return sa

    @classmethod
    def from_analysers(cls, analysers, frames_per_step=1, input_dtype=torch.float32, voiced=False, device=None,
                       features=False, sessions=False):
        """A batch whose stream s continues analysers[s] (initialised
        SimpleAnalyser objects of one frame rate, frame size and noise_buf_len);
        with sessions=True every stream's init_left is 0."""
        analysers = list(analysers)
        if not analysers:
            raise ValueError("no analysers")
        a0 = analysers[0]
        for a in analysers:
            if (a.frame_rate, a.frame_size, a.noise_buf_len) != (a0.frame_rate, a0.frame_size, a0.noise_buf_len):
                raise ValueError("the analysers differ in frame rate, frame size or noise_buf_len")
            if not a.initialized:
                raise Exception("Analyser not initialized")
        sb = cls(len(analysers), a0.frame_rate, a0.frame_size, a0.noise_buf_len, frames_per_step=frames_per_step,
                 input_dtype=input_dtype, voiced=voiced, device=device, features=features, sessions=sessions)
        sb.state.copy_(torch.from_numpy(pack_state(analysers)))
        if sb.sessions:
            sb.init_left.zero_()
        sb.initialized = True
        return sb


def pack_state(analysers):
    """The device state (S, state_doubles) float64 of host SimpleAnalyser objects."""
    nb = analysers[0].noise_buf_len
    out = np.zeros((len(analysers), state_doubles(nb)), np.float64)
    ints = out.view(np.int32)[:, 2 * (NOISE_COLS * nb + 6):]
    t = NOISE_COLS * nb
    for i, a in enumerate(analysers):
        out[i, :t] = np.asarray(a._noise_feats)[:, _NOISE_FROM_FEAT].reshape(-1)
        out[i, t] = a.energy_thresh
        out[i, t + 1] = a.spectral_std_thresh
        out[i, t + 2:t + 6] = a.spectral_energy_bands_thresh
        buf = [False] * (STATUS_BITS - len(a.temp_buffer)) + list(a.temp_buffer)
        bits = 0
        for st in buf:
            bits = (bits << 1) | int(bool(st))
        ints[i] = (bits, int(a.silence), a.noise_pointer, a.frame_number)
    return out
