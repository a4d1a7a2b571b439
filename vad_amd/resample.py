"""Sample-rate conversion to the front end's rate, on the device
(include/vad_amd.h, "Resampling").

The mel bank, the 400 / 160 framing and every trained classifier assume
``cfg.sample_rate`` (16 kHz).  ``Resampler`` converts finished clips (one, or
a batch written straight into the ``ClipBatch`` layout), ``StreamResampler``
converts live streams hop by hop in front of ``StreamBatch`` /
``SimpleStreamBatch``, ``SessionStreamResampler`` does so in front of a
sessions batch, each stream at the rate its session started with.

Definition.  For rate_in -> rate_out, g = gcd, up = rate_out / g, down =
rate_in / g, P = 10 * max(up, down); ``taps`` are the 2P+1 taps of
scipy.signal.resample_poly's default filter (Kaiser(5.0)-windowed sinc, cutoff
1 / max(up, down), unit DC gain, times up), restated here in numpy; 1 / 1 has
the single tap 1.  For an input x[0..n), zero elsewhere,

    n_out = ceil(n * up / down)
    y[m]  = sum_j x[j] * taps[m * down - j * up + P]

which is resample_poly(x, up, down).  ``resample_model`` is that sum in
float64 numpy; ``StreamModel`` is the hop-by-hop form the stream kernel
implements.
"""
from __future__ import annotations

import ctypes
import math
import weakref

import numpy as np

from .config import MfccConfig

TILE_OUT = 1024     # outputs per destination tile (VAD_RESAMPLE_TILE)
MAX_TABLE = 16384   # floats of the phase table in LDS (VAD_RESAMPLE_MAX_TABLE)
MAX_SPAN = 16384    # floats of the input tile / stream window in LDS (VAD_RESAMPLE_MAX_SPAN)
MAX_RATES = 8       # rates of one SessionStreamResampler (VAD_RESAMPLE_MAX_RATES)
SESSIONS_GRID = 2048  # workgroups of the sessions stream kernel (vad_resample_sessions_grid)


def design_taps(up, down):
    """The float64 taps of resample_poly's default filter for up / down:
    firwin(2P+1, 1 / max(up, down), window=('kaiser', 5.0)) * up."""
    mx = max(up, down)
    if mx == 1:
        return np.ones(1, np.float64)
    half = 10 * mx
    n = 2 * half + 1
    cutoff = 1.0 / mx
    m = np.arange(n) - 0.5 * (n - 1)
    h = cutoff * np.sinc(cutoff * m)
    h = h * np.kaiser(n, 5.0)
    h = h / np.sum(h)
    return h * up


class ResampleSpec:
    """The ratio, filter and sizes of one rate_in -> rate_out conversion (host
    only): ``up``, ``down``, ``half_len`` (P), ``taps`` (float64, 2P+1),
    ``phase_len`` (T), ``delay`` (the stream's d), ``n_out(n)``."""

    def __init__(self, rate_in, rate_out=16000):
        if int(rate_in) != rate_in or int(rate_out) != rate_out or rate_in <= 0 or rate_out <= 0:
            raise ValueError(f"sample rates are positive integers, got {rate_in} -> {rate_out}")
        self.rate_in, self.rate_out = int(rate_in), int(rate_out)
        g = math.gcd(self.rate_in, self.rate_out)
        self.up, self.down = self.rate_out // g, self.rate_in // g
        mx = max(self.up, self.down)
        self.half_len = 0 if mx == 1 else 10 * mx
        self.phase_len = -(-(2 * self.half_len + 1) // self.up)
        self.row_stride = self.phase_len | 1
        self.delay = -(-self.half_len // self.down)
        table = self.up * self.row_stride
        span = -(-((TILE_OUT - 1) * self.down) // self.up) + self.phase_len
        if table > MAX_TABLE or span > MAX_SPAN:
            raise ValueError(
                f"{self.rate_in} -> {self.rate_out} Hz is {self.up} / {self.down}: its phase table ({table} floats) "
                f"and input tile ({span} floats) must fit {MAX_TABLE} and {MAX_SPAN} floats of LDS")
        self.taps = design_taps(self.up, self.down)
        # samples of history a stream keeps: ceil((d * down - P) / up) + T - 1
        self.history = -(-(self.delay * self.down - self.half_len) // self.up) + self.phase_len - 1

    def n_out(self, n):
        n = int(n)
        if n < 0:
            raise ValueError("negative length")
        return -(-n * self.up // self.down)

    def phase_table(self, taps=None):
        """taps as [up][T] (zero past tap 2P): row r holds taps[r + i * up]."""
        h = self.taps if taps is None else np.asarray(taps, np.float64)
        t = np.zeros(self.up * self.phase_len, np.float64)
        idx = np.arange(len(h))
        t[(idx % self.up) * self.phase_len + idx // self.up] = h
        return t.reshape(self.up, self.phase_len)


def _spec(spec_or_rate, rate_out=16000):
    return spec_or_rate if isinstance(spec_or_rate, ResampleSpec) else ResampleSpec(spec_or_rate, rate_out)


def _dots(w, hi, r, ph):
    """sum_i w[hi - i] * ph[r, i], i rising (the device chain's order), float64."""
    acc = w[hi] * ph[r, 0]
    for i in range(1, ph.shape[1]):
        acc = acc + w[hi - i] * ph[r, i]
    return acc


def resample_model(x, rate_in, rate_out=16000, taps=None):
    """y of the module docstring for a 1-D x, in float64 numpy.  rate_in may
    be a ResampleSpec; taps replaces the spec's (e.g. their float32 values)."""
    s = _spec(rate_in, rate_out)
    x = np.asarray(x, np.float64).reshape(-1)
    n, n_out, T = len(x), s.n_out(len(x)), s.phase_len
    if n_out == 0:
        return np.zeros(0, np.float64)
    q = np.arange(n_out, dtype=np.int64) * s.down + s.half_len
    jmax, r = q // s.up, q % s.up
    right = max(int(jmax[-1]) - (n - 1), 0)
    w = np.concatenate([np.zeros(T - 1), x, np.zeros(right)])
    return _dots(w, jmax + (T - 1), r, s.phase_table(taps))


class StreamModel:
    """The stream kernel's arithmetic in float64 numpy, for n_streams streams:
    per stream a history of ``spec.history`` input samples (zero at reset) and
    the count of outputs emitted; ``step(x)`` takes (K, S, hop_in) and returns
    (K, S, hop_out) with z[n] = y[n - d], z[n] = 0 for n < d."""

    def __init__(self, n_streams, rate_in, rate_out=16000, hop_out=160, taps=None):
        s = self.spec = _spec(rate_in, rate_out)
        if hop_out * s.down % s.up:
            raise ValueError("a hop must be a whole number of input samples")
        self.n, self.hop_out, self.hop_in = int(n_streams), int(hop_out), hop_out * s.down // s.up
        self.ph = s.phase_table(taps)
        c0 = s.delay * s.down - s.half_len
        self.c_off = -(-c0 // s.up) * s.up - c0
        self.reset()

    def reset(self):
        self.hist = np.zeros((self.n, self.spec.history), np.float64)
        self.emitted = 0

    def step(self, x):
        s = self.spec
        x = np.asarray(x, np.float64)
        K = x.shape[0]
        assert x.shape == (K, self.n, self.hop_in)
        w = np.concatenate([self.hist, x.transpose(1, 0, 2).reshape(self.n, K * self.hop_in)], axis=1)
        q = np.arange(K * self.hop_out, dtype=np.int64) * s.down + self.c_off
        hi, r = q // s.up + (s.phase_len - 1), q % s.up
        z = np.stack([_dots(w[i], hi, r, self.ph) for i in range(self.n)])
        z[:, :max(s.delay - self.emitted, 0)] = 0.0
        self.emitted += K * self.hop_out
        self.hist = w[:, K * self.hop_in:]
        return z.reshape(self.n, K, self.hop_out).transpose(1, 0, 2)

    def flush(self):
        """The remaining d outputs of every stream, (S, d): zeros are fed."""
        d, out = self.spec.delay, []
        for _ in range(-(-d // self.hop_out)):
            out.append(self.step(np.zeros((1, self.n, self.hop_in)))[0])
        return np.concatenate(out, axis=1)[:, :d] if out else np.zeros((self.n, 0))


def plan_layout(lens_in, rates, cfg: MfccConfig = MfccConfig()):
    """The ClipBatch placement of the resampled clips: ``(tables, total)`` of
    vad_amd.batch.layout over the output lengths (rates: one rate, or one per
    clip)."""
    from .batch import layout
    lens_in = [int(n) for n in lens_in]
    rates = _rates(rates, len(lens_in))
    specs = {r: ResampleSpec(r, cfg.sample_rate) for r in set(rates)}
    return layout([specs[r].n_out(n) for n, r in zip(lens_in, rates)], cfg.frame_size, cfg.hop)


def _rates(rates, n):
    if np.ndim(rates) == 0:
        return [rates] * n
    rates = list(rates)
    if len(rates) != n:
        raise ValueError(f"{n} clips, {len(rates)} rates")
    return rates


# ---------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------
_NAMES = {"float32": "f32", "int16": "i16"}
_PLANS = {}


def _tname(dtype):
    name = _NAMES.get(str(dtype).replace("torch.", ""))
    if name is None:
        raise ValueError(f"samples are int16 or float32, got {dtype}")
    return name


class _Plan:
    """A vad_resample_plan with its table on one device."""

    def __init__(self, spec, device):
        import torch
        from . import _lib
        self.spec, self.device = spec, device
        taps = np.ascontiguousarray(spec.taps.astype(np.float32))
        h = ctypes.c_void_p()
        lib = _lib.lib()
        _lib.check(lib.vad_resample_plan_create(spec.up, spec.down, taps.ctypes.data, len(taps), ctypes.byref(h)),
                   "vad_resample_plan_create")
        self.handle = h
        self._free = weakref.finalize(self, lib.vad_resample_plan_destroy, h)
        with torch.cuda.device(device):
            _lib.check(lib.vad_resample_plan_upload(h), "vad_resample_plan_upload")
        assert lib.vad_resample_delay(h) == spec.delay and lib.vad_resample_tile_outputs() == TILE_OUT


def _plan(spec, device):
    import torch
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (spec.up, spec.down, device.index)
    if key not in _PLANS:
        _PLANS[key] = _Plan(spec, device)
    return _PLANS[key]


def resample_clips(clips, rates, cfg: MfccConfig = MfccConfig(), out_dtype=None, device=None, stream=None):
    """Clips at ``rates`` (one rate, or one per clip) as a ClipBatch at
    cfg.sample_rate, of out_dtype (float32 by default).  clips: all device
    tensors (contiguous 1-D, at any sample offset) or all host arrays, all
    int16 or all float32.  One launch per distinct rate into the one packed
    buffer, whatever the clip count; host arrays travel in one pinned buffer
    and one H2D copy.  No pack step and no synchronisation."""
    import torch
    from . import _lib
    from .batch import _TABLES, ClipBatch
    out_dtype = torch.float32 if out_dtype is None else out_dtype
    oname = _tname(out_dtype)
    clips = list(clips)
    rates = _rates(rates, len(clips))
    specs = {r: ResampleSpec(r, cfg.sample_rate) for r in dict.fromkeys(rates)}
    on_device = [isinstance(c, torch.Tensor) and c.is_cuda for c in clips]
    if any(on_device) and not all(on_device):
        raise ValueError("the clips are all device tensors or all host arrays")
    staging = None
    if clips and not on_device[0]:
        arrays = [np.asarray(c) for c in clips]
        kinds = {a.dtype for a in arrays}
        if len(kinds) > 1:
            raise ValueError(f"the clips of a batch are all int16 or all float32, got {sorted(map(str, kinds))}")
        iname = _tname(arrays[0].dtype)
        if any(a.ndim != 1 for a in arrays):
            raise ValueError("every clip is a 1-D array")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        offs = np.concatenate(([0], np.cumsum([len(a) for a in arrays]))).astype(np.int64)
        tdt = torch.int16 if iname == "i16" else torch.float32
        staging = torch.empty((max(int(offs[-1]), 1),), dtype=tdt, pin_memory=True)
        view = staging.numpy()
        for a, o in zip(arrays, offs[:-1].tolist()):
            view[o:o + len(a)] = a
        lens_in = [len(a) for a in arrays]
    else:
        for x in clips:
            if x.dim() != 1 or not x.is_contiguous():
                raise ValueError("every clip must be a contiguous 1-D tensor")
        kinds = {x.dtype for x in clips}
        if len(kinds) > 1:
            raise ValueError(f"the clips of a batch are all int16 or all float32, got {sorted(map(str, kinds))}")
        iname = _tname(kinds.pop()) if kinds else "f32"
        if len({x.device for x in clips}) > 1:
            raise ValueError("the clips of a batch lie on one device")
        dev = clips[0].device if clips else \
            (torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device))
        lens_in = [x.numel() for x in clips]
    n = len(clips)
    t, total = plan_layout(lens_in, rates, cfg)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        if staging is not None:
            src = torch.empty((staging.numel(),), dtype=staging.dtype, device=dev)
            src.copy_(staging, non_blocking=True)
            esize = src.element_size()
            addr = [src.data_ptr() + int(o) * esize if ln else 0 for o, ln in zip(offs[:-1], lens_in)]
        else:
            src = None
            addr = [x.data_ptr() if x.numel() else 0 for x in clips]
        # one H2D copy: the six batch tables, the input lengths, and per rate
        # the source addresses (0 for the clips of the other rates: left alone)
        rows = [t[name] for name in _TABLES] + [np.asarray(lens_in, np.int64).reshape(n)]
        for r in specs:
            rows.append(np.array([a if rr == r else 0 for a, rr in zip(addr, rates)], np.int64).reshape(n))
        d = torch.from_numpy(np.stack(rows).reshape(len(rows), n)).to(dev)
        data = torch.empty((total,), dtype=out_dtype, device=dev)
        if len(specs) != 1:
            data.zero_()  # no launch, or launches that each leave the other rates' clips alone
        fn = f"vad_resample_batch_{iname}_{oname}"
        for i, spec in enumerate(specs.values()):
            _lib.check(getattr(_lib.lib(), fn)(_plan(spec, dev).handle, _lib.ptr(d[7 + i]), _lib.ptr(d[6]),
                                               _lib.ptr(d[0]), n, _lib.ptr(data), total, _lib.stream_ptr(s)), fn)
    return ClipBatch(data, t["len"], cfg, _tables=d[:6], _staging=staging)


class Resampler:
    """rate_in -> rate_out (16 kHz) for finished clips on the device.

    ``r(x)`` converts one 1-D CUDA int16 / float32 tensor; ``r.batch(tensors,
    cfg)`` converts many into a ClipBatch.  ``up``, ``down``, ``half_len``,
    ``taps``, ``n_out`` and ``delay`` are the ResampleSpec's."""

    def __init__(self, rate_in, rate_out=16000, device=None):
        self.spec = ResampleSpec(rate_in, rate_out)
        self.rate_in, self.rate_out = self.spec.rate_in, self.spec.rate_out
        self.plan = _plan(self.spec, device)
        self.device = self.plan.device
        self._cfg = MfccConfig(sample_rate=self.rate_out)

    up = property(lambda self: self.spec.up)
    down = property(lambda self: self.spec.down)
    half_len = property(lambda self: self.spec.half_len)
    taps = property(lambda self: self.spec.taps)
    delay = property(lambda self: self.spec.delay)

    def n_out(self, n):
        return self.spec.n_out(n)

    def __call__(self, x, out_dtype=None, stream=None):
        import torch
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 1):
            raise TypeError("x must be a 1-D CUDA tensor")
        b = resample_clips([x], self.rate_in, self._cfg, out_dtype, stream=stream)
        return b.data[:self.spec.n_out(x.numel())]

    def batch(self, tensors, cfg: MfccConfig = MfccConfig(), out_dtype=None, stream=None):
        if cfg.sample_rate != self.rate_out:
            raise ValueError(f"this resampler ends at {self.rate_out} Hz, the configuration is at {cfg.sample_rate}")
        return resample_clips(tensors, self.rate_in, cfg, out_dtype, device=self.device, stream=stream)


class StreamResampler:
    """Live streams at rate_in, hop by hop, to cfg.sample_rate: every step
    takes (K, S, hop_in) samples, hop_in = rate_in / 100 at the reference
    framing, and writes (K, S, cfg.hop) into ``out`` -- by default a buffer of
    its own; pass ``StreamBatch.inputs`` (or SimpleStreamBatch's input block
    when its frames are hops) and the hop kernel reads the result in place.
    The output is the clip conversion of the stream's whole input, delayed by
    ``delay`` samples (zeros first); ``flush()`` returns the last ``delay``.
    State (history, counters) lives on the device; a step is one launch, with
    no allocation and no synchronisation, and ``capture()`` records it."""

    def __init__(self, n_streams, rate_in, cfg: MfccConfig = MfccConfig(), hops_per_step=1, input_dtype=None,
                 out=None, out_dtype=None, device=None):
        import torch
        from . import _lib
        if int(rate_in) != rate_in or rate_in <= 0:
            raise ValueError(f"sample rates are positive integers, got {rate_in}")
        if int(rate_in) % 100:
            raise ValueError(f"streams take rates that are multiples of 100 Hz, got {rate_in}")
        self.spec = s = ResampleSpec(rate_in, cfg.sample_rate)
        if cfg.hop * s.down % s.up:
            raise ValueError(f"a hop of {cfg.hop} samples at {cfg.sample_rate} Hz is no whole number of samples "
                             f"at {rate_in} Hz")
        self.cfg, self.n, self.K = cfg, int(n_streams), int(hops_per_step)
        if self.n < 1 or self.K < 1:
            raise ValueError("n_streams and hops_per_step must be >= 1")
        self.hop_out, self.hop_in = int(cfg.hop), cfg.hop * s.down // s.up
        if self.K * self.hop_in + s.history > MAX_SPAN:
            raise ValueError(f"{self.K} hops of {self.hop_in} samples and the history ({s.history}) exceed the "
                             f"{MAX_SPAN}-float window")
        self.delay = s.delay
        self.input_dtype = torch.float32 if input_dtype is None else input_dtype
        iname = _tname(self.input_dtype)
        if out is not None:
            if not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous()
                    and tuple(out.shape) == (self.K, self.n, self.hop_out)):
                raise ValueError(f"out must be a contiguous CUDA tensor of shape {(self.K, self.n, self.hop_out)}")
            if out_dtype is not None and out_dtype != out.dtype:
                raise ValueError("out_dtype differs from out's")
            dev = out.device
        else:
            dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            out = torch.zeros((self.K, self.n, self.hop_out), dtype=out_dtype or torch.float32, device=dev)
        self.out = out
        self.plan = _plan(s, dev)
        lib = _lib.lib()
        self._name = f"vad_resample_stream_{iname}_{_tname(out.dtype)}"
        self._fn = getattr(lib, self._name)
        nbytes = int(lib.vad_resample_stream_state_bytes(self.plan.handle, self.n))
        self.state = torch.zeros((nbytes // 4,), dtype=torch.int32, device=dev)
        self.inputs = torch.zeros((self.K, self.n, self.hop_in), dtype=self.input_dtype, device=dev)
        self.graph = None

    def reset(self):
        self.state.zero_()

    def _launch(self, x, out, stream=None):
        from . import _lib
        rc = self._fn(self.plan.handle, ctypes.c_void_p(x.data_ptr()), x.stride(1), x.stride(0), self.n, x.shape[0],
                      self.hop_out, _lib.ptr(self.state), _lib.ptr(out),
                      _lib.stream_ptr() if stream is None else stream)
        if rc:
            _lib.check(rc, self._name)

    def step_block(self, x=None):
        """K hops of every stream: x (K, S, hop_in) of the input dtype, or
        None for the block already written into ``inputs``.  Returns ``out``.
        A last, shorter block (k < K hops) is taken too and returns out[:k]."""
        from .stream import hop_rows_disjoint
        if x is not None:
            k = x.shape[0] if x.dim() == 3 else 0
            if not 1 <= k <= self.K or tuple(x.shape[1:]) != tuple(self.inputs.shape[1:]) \
                    or x.dtype != self.input_dtype or not x.is_cuda:
                raise ValueError(f"x must be a CUDA {self.input_dtype} tensor of shape {tuple(self.inputs.shape)}")
            in_place = x.stride(2) == 1 and x.stride(1) >= self.hop_in and \
                hop_rows_disjoint(self.n, k, x.stride(0), x.stride(1), self.hop_in)
            if k < self.K or (self.graph is None and in_place):
                if not in_place:
                    x = x.contiguous()
                self._launch(x, self.out[:k])  # read in place
                return self.out[:k]
            self.inputs.copy_(x)
        if self.graph is not None:
            self.graph.replay()
        else:
            self._launch(self.inputs, self.out)
        return self.out

    def capture(self):
        """Capture one step (inputs -> out) into a graph; step_block replays it."""
        import torch
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        saved = (self.state.clone(), self.out.clone())
        with torch.cuda.stream(s):
            self._launch(self.inputs, self.out)  # warm-up (first launch sets kernel attributes)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.state.copy_(saved[0]); self.out.copy_(saved[1])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._launch(self.inputs, self.out)
        self.graph = g
        return g

    def flush(self):
        """The last ``delay`` outputs of every stream, (S, delay) of out's
        dtype: zero hops are fed (directly, not through the graph; ``out`` is
        not touched).  The streams have ended: reset() before new input."""
        import torch
        d = self.delay
        hops = -(-d // self.hop_out)
        got = []
        zeros = torch.zeros_like(self.inputs)
        for _ in range(-(-hops // self.K)):
            o = torch.empty_like(self.out)
            self._launch(zeros, o)
            got.append(o)
        if not got:
            return self.out.new_zeros((self.n, 0))
        z = torch.cat(got).transpose(0, 1).reshape(self.n, -1)
        return z[:, :d].contiguous()


class SessionStreamResampler:
    """The stream resampler for sessions: S slots whose callers join, hang up
    and stall, each session at a rate of its own out of ``rates`` (1 ..
    MAX_RATES distinct rates, multiples of 100 Hz; cfg.sample_rate itself is
    the copy, with delay 0).  One launch converts, per stream, the first
    n_s = min(max(hop_counts[s], 0), K) hops of its column of ``inputs``
    (K, S, hop_in_max) -- the first ``hop_ins[i]`` samples of a row for a
    stream at rates[i] -- into rows 0..n_s-1 of its column of ``out`` (K, S,
    cfg.hop); rows n_s..K-1 are not written.  Static device tensors, read at
    the start of every step:

      hop_counts (S,) int32   shared with the hop kernel when given (neither
                              kernel writes it); K by default
      restart    (S,) uint8   the resampler's own: nonzero makes the stream
                              fresh (zero history, the first ``delays[i]``
                              outputs zero again) at rates[rate_index[s]],
                              and the kernel stores 0 back
      rate_index (S,) int32   read under a flag only, clamped into the rates
      state                   histories padded to the longest, emitted
                              counts, the rate index of every stream

    A stream with no hop and no flag keeps every byte of its state.  A
    session's rows are, bit for bit, those of a freshly reset StreamResampler
    of its rate fed the same hops.  Built by ``StreamBatch.resampler`` it
    writes the batch's ``inputs`` and shares its ``hop_counts``, and
    ``restart=`` reaches batch, resampler and session segmenters alike."""

    def __init__(self, n_streams, rates, cfg: MfccConfig = MfccConfig(), hops_per_step=1, input_dtype=None,
                 out=None, hop_counts=None, out_dtype=None, device=None, batch=None):
        import torch
        from . import _lib
        rates = [rates] if np.ndim(rates) == 0 else list(rates)
        if not 1 <= len(rates) <= MAX_RATES:
            raise ValueError(f"1 to {MAX_RATES} rates, got {len(rates)}")
        for r in rates:
            if int(r) != r or r <= 0:
                raise ValueError(f"sample rates are positive integers, got {r}")
            if int(r) % 100:
                raise ValueError(f"streams take rates that are multiples of 100 Hz, got {r}")
        self.rates = [int(r) for r in rates]
        if len(set(self.rates)) != len(self.rates):
            raise ValueError(f"the rates are distinct, got {self.rates}")
        self.specs = [ResampleSpec(r, cfg.sample_rate) for r in self.rates]
        self.cfg, self.n, self.K = cfg, int(n_streams), int(hops_per_step)
        if self.n < 1 or self.K < 1:
            raise ValueError("n_streams and hops_per_step must be >= 1")
        self.hop_out = int(cfg.hop)
        for s in self.specs:
            if cfg.hop * s.down % s.up:
                raise ValueError(f"a hop of {cfg.hop} samples at {cfg.sample_rate} Hz is no whole number of samples "
                                 f"at {s.rate_in} Hz")
        self.hop_ins = [cfg.hop * s.down // s.up for s in self.specs]
        for s, h in zip(self.specs, self.hop_ins):
            if self.K * h + s.history > MAX_SPAN:
                raise ValueError(f"{self.K} hops of {h} samples and the history ({s.history}) exceed the "
                                 f"{MAX_SPAN}-float window")
        self.hop_in = max(self.hop_ins)
        self.delays = [s.delay for s in self.specs]
        self.input_dtype = torch.float32 if input_dtype is None else input_dtype
        iname = _tname(self.input_dtype)
        if out is not None:
            if not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous()
                    and tuple(out.shape) == (self.K, self.n, self.hop_out)):
                raise ValueError(f"out must be a contiguous CUDA tensor of shape {(self.K, self.n, self.hop_out)}")
            if out_dtype is not None and out_dtype != out.dtype:
                raise ValueError("out_dtype differs from out's")
            dev = out.device
        else:
            dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            out = torch.zeros((self.K, self.n, self.hop_out), dtype=out_dtype or torch.float32, device=dev)
        self.out = out
        if hop_counts is None:
            hop_counts = torch.full((self.n,), self.K, dtype=torch.int32, device=dev)
        elif not (isinstance(hop_counts, torch.Tensor) and hop_counts.is_cuda and hop_counts.is_contiguous()
                  and tuple(hop_counts.shape) == (self.n,) and hop_counts.dtype == torch.int32):
            raise ValueError(f"hop_counts must be a contiguous CUDA int32 tensor of shape ({self.n},)")
        self.hop_counts = hop_counts
        self._batch = batch
        self.plans = [_plan(s, dev) for s in self.specs]
        self._handles = (ctypes.c_void_p * len(self.plans))(*[p.handle.value for p in self.plans])
        lib = _lib.lib()
        assert lib.vad_resample_sessions_grid() == SESSIONS_GRID
        self._name = f"vad_resample_stream_sessions_{iname}_{_tname(out.dtype)}"
        self._fn = getattr(lib, self._name)
        nbytes = int(lib.vad_resample_sessions_state_bytes(self._handles, len(self.plans), self.n))
        self.state = torch.zeros((nbytes // 4,), dtype=torch.int32, device=dev)
        self.inputs = torch.zeros((self.K, self.n, self.hop_in), dtype=self.input_dtype, device=dev)
        self.restart = torch.ones((self.n,), dtype=torch.uint8, device=dev)  # the first step adopts rate_index
        self.rate_index = torch.zeros((self.n,), dtype=torch.int32, device=dev)
        self.graph = None

    @property
    def history(self):
        """(S, longest history) float32 view of the state's histories."""
        import torch
        h = max(s.history for s in self.specs)
        return self.state[:self.n * h].view(torch.float32).view(self.n, h)

    @property
    def emitted(self):
        """(S,) int32: min(outputs emitted by the session, its delay)."""
        return self.state[self.state.numel() - 2 * self.n:self.state.numel() - self.n]

    @property
    def stream_rate(self):
        """(S,) int32: the index in ``rates`` every stream's session runs at."""
        return self.state[self.state.numel() - self.n:]

    def reset(self):
        """Every stream fresh; the next step adopts ``rate_index``."""
        self.state.zero_()
        self.restart.fill_(1)

    def _launch(self, stream=None):
        from . import _lib
        x = self.inputs
        rc = self._fn(self._handles, len(self.plans), _lib.ptr(x), x.stride(1), x.stride(0), self.n, self.K,
                      self.hop_out, _lib.ptr(self.hop_counts), _lib.ptr(self.restart), _lib.ptr(self.rate_index),
                      _lib.ptr(self.state), _lib.ptr(self.out), _lib.stream_ptr() if stream is None else stream)
        if rc:
            _lib.check(rc, self._name)

    def _set(self, t, dst, name):
        import torch
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.shape != dst.shape or t.dtype != dst.dtype:
            raise ValueError(f"{name} must be a CUDA {str(dst.dtype).replace('torch.', '')} tensor of shape "
                             f"{tuple(dst.shape)}")
        dst.copy_(t)

    def step_block(self, x=None, hop_counts=None, restart=None, rate=None):
        """One step.  x (K, S, hop_in) of the input dtype, hop_counts (S,)
        int32, restart (S,) uint8 and rate (S,) int32 -- indices into
        ``rates`` -- are CUDA tensors copied into ``inputs``, ``hop_counts``,
        ``restart`` and ``rate_index``; None leaves those as written.  Behind
        a StreamBatch, hop_counts and restart go through the batch, so the
        hop kernel and the session segmenters see them too.  Returns ``out``."""
        if rate is not None:
            self._set(rate, self.rate_index, "rate")
        if self._batch is not None:
            self._batch._set_sessions(hop_counts, restart)
        else:
            if hop_counts is not None:
                self._set(hop_counts, self.hop_counts, "hop_counts")
            if restart is not None:
                self._set(restart, self.restart, "restart")
        if x is not None:
            self._set(x, self.inputs, "x")
        if self.graph is not None:
            self.graph.replay()
        else:
            self._launch()
        return self.out

    def capture(self):
        """Capture one step into a graph; step_block replays it.  The warm-up
        launch consumes restart flags and advances the streams: state, out
        and flags are put back after it."""
        import torch
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        saved = (self.state.clone(), self.out.clone(), self.restart.clone())
        with torch.cuda.stream(s):
            self._launch()  # warm-up (first launch sets kernel attributes)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.state.copy_(saved[0]); self.out.copy_(saved[1]); self.restart.copy_(saved[2])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._launch()
        self.graph = g
        return g
