"""Offline dataset export, GPU edition of the reference's dataset pipeline
(dataset_creator.py:58-66 -> Pool.map(process_file) -> scale_features ->
write_features).

Same functions and argument conventions as the reference modules:

  dataset/sph.py             ``sph_read`` (class ``Sph``)
  dataset/stm_parser.py      ``stm_parse``, ``get_samples_indices``
  dataset/file_processing.py ``split_into_frames`` (with STM segments),
                             ``process_file``, ``create_table_header``,
                             ``write_features``
  dataset/utils.py           ``scale_features``
  dataset_creator.py:19-73   ``process_files`` (a chunk of files per call:
                             one clip batch, vad_amd.batch)
  dataset/file_processing.py ``load_csv``, ``features_number``
  dataset/file_index.py      ``create_file_index``
  learning/utils.py          ``load_files``
  dataset/__init__.py        ``random_rows_order`` (the order
                             random_features_generator draws rows in)

The MFCC / delta features run on the GPU (one clip per call, the offline
feature rows of ``vad_features_f32``), ``scale_features`` is a device
reduction (``vad_scale_features``), and the CSV text is produced by a native
multithreaded formatter (``vad_format_csv_rows``) that prints values exactly
as numpy prints float32.  ``write_features`` keeps the reference's
``csv.writer`` interface.

The way back, CSV text into the float32 ``X`` / uint8 ``y`` the device
trainers take, is ``read_csv_device``: line index and field parsing are HIP
kernels (``vad_csv_count_lines`` / ``vad_csv_index`` / ``vad_csv_parse``) that
give numpy's values bit for bit; the few rows the device does not decide are
parsed here with ``float()``.
"""
from __future__ import annotations

import csv
import ctypes
import io

import numpy as np
import torch

from . import _lib
from .config import MfccConfig
from .pipeline import VadPipeline

# ----------------------------------------------------------------------------
# dataset/sph.py
# ----------------------------------------------------------------------------


class Sph:
    """sph.py:9-30."""

    def __init__(self, channels, framerate, sample_width, data):
        self._channels = channels
        self._framerate = framerate
        self._sample_width = sample_width
        self._data = data

    @property
    def channels(self):
        return self._channels

    @property
    def framerate(self):
        return self._framerate

    @property
    def sample_width(self):
        return self._sample_width

    @property
    def data(self):
        return self._data


def sph_read(fname):
    """sph.py:33-64: nine header lines (sample_count, sample_n_bytes,
    channel_count, sample_rate taken from lines 3, 4, 5, 7, third field),
    then big-endian samples right after them, stored into int16 (wrapping, as
    the reference's numpy-1 assignment did).  At most sample_count samples;
    a truncated file yields fewer (the rest stay 0)."""
    with open(fname, "rb") as f:
        header = [f.readline(1024) for _ in range(9)]
        samples_num = int(header[2].split(b" ")[2])
        sample_width = int(header[3].split(b" ")[2])
        channels = int(header[4].split(b" ")[2])
        framerate = int(header[6].split(b" ")[2])
        raw = f.read(samples_num * sample_width)
    n = len(raw) // sample_width
    b = np.frombuffer(raw[:n * sample_width], np.uint8).reshape(n, sample_width).astype(np.uint64)
    v = np.zeros(n, np.uint64)
    for j in range(sample_width):  # big-endian: byte j carries bits 8*(w-1-j)
        v |= b[:, j] << np.uint64(8 * (sample_width - 1 - j))
    samples = np.zeros((samples_num,), dtype=np.int16)
    samples[:n] = (v & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16)
    return Sph(channels, framerate, sample_width, samples)


# ----------------------------------------------------------------------------
# dataset/stm_parser.py
# ----------------------------------------------------------------------------
def stm_parse(fname):
    """stm_parser.py:5-19: [starts, ends] float32 of every STM line with >= 7
    space-separated fields whose 7th is not ignore_time_segment_in_scoring."""
    starts, ends = [], []
    with open(fname, "rb") as f:
        for line in iter(lambda: f.readline(1024), b""):
            items = line.split(b" ")
            if len(items) < 7 or items[6].strip() == b"ignore_time_segment_in_scoring":
                continue
            starts.append(np.float32(items[3]))
            ends.append(np.float32(items[4]))
    return [np.array(starts, np.float32), np.array(ends, np.float32)]


def get_samples_indices(fname, samplerate=16384):
    """stm_parser.py:22-26: float32 seconds x rate -> int32 (truncation)."""
    starts, ends = stm_parse(fname)
    return ((starts * samplerate).astype(np.int32, copy=False),
            (ends * samplerate).astype(np.int32, copy=False))


# ----------------------------------------------------------------------------
# dataset/file_processing.py
# ----------------------------------------------------------------------------
def read_audio(fname):
    """file_processing.py:26-35: (sample_rate, samples) of a .wav or .sph."""
    if fname.endswith(".wav"):
        from scipy.io import wavfile
        return wavfile.read(fname)
    if fname.endswith(".sph"):
        s = sph_read(fname)
        return s.framerate, s.data
    raise ValueError("Wrong file format: " + str(fname))


def gather_segments(data, transcription_path, frame_rate):
    """file_processing.py:87-94: concatenation of data[start:end] over the
    transcript's segments (int16, as the reference's new_data)."""
    starts, ends = get_samples_indices(transcription_path, frame_rate)
    parts = [np.asarray(data[s:e]) for s, e in zip(starts, ends)]
    return np.concatenate([np.array([], np.int16)] + parts) if parts else np.array([], np.int16)


def split_into_frames(data, frame_size, step, transcription_path=None, frame_rate=None):
    """file_processing.py:80-103: frames data[o:o+size] while len - o > size,
    after gathering the transcript's segments when a transcript is given."""
    if transcription_path and frame_rate:
        data = gather_segments(data, transcription_path, frame_rate)
    elif transcription_path and frame_rate is None:
        raise Exception('You must specify frame_rate')
    frames, offset = [], 0
    while len(data) - offset > frame_size:
        frames.append(data[offset:offset + frame_size])
        offset += step
    return frames


_PIPES = {}


def _pipeline(frame_size, frame_step, fft_n, n_filters, mfcc_num):
    key = (frame_size, frame_step, fft_n, n_filters, mfcc_num)
    if key not in _PIPES:
        cfg = MfccConfig(frame_size=frame_size, hop=frame_step, fft_n=fft_n,
                         n_filters=n_filters, n_mfcc=mfcc_num)
        _PIPES[key] = VadPipeline(cfg=cfg, mode="offline")
    return _PIPES[key]


def file_features(fname, frame_size=400, frame_step=160, fft_n=512, n_filters=26, mfcc_num=13,
                  transcription_path=None, device_out=False, resample=False):
    """Feature rows of one file as a (F-5, 3*mfcc_num) float32 array (or a
    device tensor): process_file's features without the per-row tuples.
    resample: a file at another rate than the front end's is converted on the
    device (vad_amd.resample) after the transcript's segments were gathered at
    the file's own rate; False takes its samples as they are, as the
    reference does."""
    rate, raw = read_audio(fname)
    if transcription_path:
        raw = gather_segments(raw, transcription_path, rate)
    pipe = _pipeline(frame_size, frame_step, fft_n, n_filters, mfcc_num)
    a = torch.from_numpy(np.ascontiguousarray(np.asarray(raw))).cuda()
    if a.dtype != torch.int16:
        a = a.float()
    if resample and rate != pipe.cfg.sample_rate:
        from .resample import Resampler
        a = Resampler(rate, pipe.cfg.sample_rate)(a)
    feats = _lib_window_features(pipe.mfcc(a), _lib.FEAT_OFFLINE)
    return feats if device_out else feats.cpu().numpy()


def _lib_window_features(mfcc, mode):
    from .plan import window_features
    return window_features(mfcc, mode)


def process_file(args, resample=False):
    """file_processing.py:14-77 with the same argument list
    [fname, frame_size, frame_step, fft_n, mel_filterbank, mfcc_num,
    counter_queue, transcription_path]: the list of (mfcc, delta1, delta2)
    float64 tuples of the file.  mel_filterbank must be the reference
    filterbank of the (low, high, n_filters) configuration (its row count
    selects n_filters); counter_queue may be None.  resample: see
    file_features."""
    fname, frame_size, frame_step, fft_n, fbank, mfcc_num = args[:6]
    counter_queue = args[6] if len(args) > 6 else None
    transcription_path = args[7] if len(args) > 7 else None
    f = file_features(fname, frame_size, frame_step, fft_n, int(np.asarray(fbank).shape[0]),
                      mfcc_num, transcription_path, resample=resample).astype(np.float64)
    c = mfcc_num
    features = [(r[:c], r[c:2 * c], r[2 * c:]) for r in f]
    if counter_queue is not None:
        processed = counter_queue.get() + 1
        if processed % 5 == 0:
            print("Processed " + str(processed) + ' files')
        counter_queue.put(processed)
    return features


def create_table_header(mfcc_len):
    """file_processing.py:106-123."""
    return ([f'MFCC Coef{i + 1}' for i in range(mfcc_len)]
            + [f'First delta{i + 1}' for i in range(mfcc_len)]
            + [f'Second delta{i + 1}' for i in range(mfcc_len)] + ['voiced'])


def write_features(writer, features, label):
    """file_processing.py:126-146: one csv row per window (features, label)."""
    for file_features_ in features:
        rows = [np.concatenate((fr[0], fr[1], fr[2], [label])) for fr in file_features_]
        writer.writerows(rows)


def format_csv_rows(rows, label):
    """CSV text (str) of float32 feature rows (n, 3*C) and one label, exactly
    as write_features + csv.writer print them for float32 values; native,
    multithreaded."""
    x = np.ascontiguousarray(np.asarray(rows, np.float32))
    if x.ndim != 2:
        raise ValueError("rows must be (n, n_cols)")
    n, k = x.shape
    if n == 0:
        return ""
    cap = n * (k * 24 + 48)
    buf = ctypes.create_string_buffer(cap)
    w = _lib.lib().vad_format_csv_rows(x.ctypes.data, n, k, float(label), buf, cap)
    if w < 0:
        raise _lib.VadError("vad_format_csv_rows: buffer too small")
    return buf.raw[:w].decode("ascii")


def write_feature_rows(fobj, rows, label):
    """Fast write_features for one (n, 3*C) array: appends its CSV text."""
    fobj.write(format_csv_rows(rows, label))


# ----------------------------------------------------------------------------
# dataset/utils.py
# ----------------------------------------------------------------------------
_SCALE_WS = {}


def scale_rows_device(rows):
    """scale_features on a device (n, 3*C) fp32 tensor, in place; returns
    (mean[3], std[3]) as float64 numpy arrays."""
    if not (isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dtype == torch.float32
            and rows.is_contiguous() and rows.dim() == 2 and rows.shape[1] % 3 == 0):
        raise TypeError("rows must be a contiguous (n, 3*C) float32 CUDA tensor")
    lib = _lib.lib()
    nb = int(lib.vad_scale_workspace_bytes())
    dev = rows.device
    ws = _SCALE_WS.get(dev)
    if ws is None:
        ws = _SCALE_WS[dev] = torch.zeros((nb // 8,), dtype=torch.float64, device=dev)
    _lib.check(lib.vad_scale_features(_lib.ptr(rows), rows.shape[0], rows.shape[1] // 3,
                                      _lib.ptr(ws), nb, _lib.stream_ptr()), "vad_scale_features")
    st = ws[-6:].cpu().numpy()
    return st[:3].copy(), st[3:].copy()


def scale_features(features):
    """utils.py:5-34: global mean / std per group (mfcc, delta1, delta2) over
    every value of the chunk, then (x - mean) / std.  Accepts the reference
    structure (list of files of lists of (mfcc, d1, d2) tuples, modified in
    place and returned, like the reference) or an (n, 3*C) / (n, 3, C) array
    (a scaled float32 copy is returned).  The statistics run on the GPU."""
    if isinstance(features, np.ndarray) or isinstance(features, torch.Tensor):
        x = torch.as_tensor(np.asarray(features, np.float32) if isinstance(features, np.ndarray)
                            else features).float()
        shape = x.shape
        t = x.reshape(shape[0], -1).contiguous().cuda()
        scale_rows_device(t)
        return t.cpu().numpy().reshape(shape)
    rows = [np.concatenate(fr) for ff in features for fr in ff]
    if not rows:
        return features
    c = len(features[0][0][0]) if features and features[0] else len(rows[0]) // 3
    t = torch.from_numpy(np.asarray(rows, np.float32)).cuda()
    scale_rows_device(t)
    scaled = t.cpu().numpy().astype(np.float64)
    i = 0
    for ff in features:
        for fr in ff:
            for g in range(3):
                fr[g][:] = scaled[i, g * c:(g + 1) * c]
            i += 1
    return features


# ----------------------------------------------------------------------------
# dataset_creator.py:19-73
# ----------------------------------------------------------------------------
FILES_PER_STEP = 30  # config.py:32


def list_audio_files(files, max_files=None):
    """dataset_creator.py:31-40: the .wav / .sph files of every directory of
    ``files`` (a file path stands for itself, if it passes the same filter),
    cut to ``max_files``.  Directory entries are taken in sorted order (the
    reference takes os.listdir's, which is arbitrary)."""
    import os
    todo = []
    for p in files:
        names = [p + '/' + f for f in sorted(os.listdir(p))] if os.path.isdir(p) else [p]
        todo.extend(f for f in names if f.endswith('.wav') or f.endswith('.sph'))
    if max_files is not None and len(todo) > max_files:
        todo = todo[:max_files]
    return todo


def process_files(files, files_type, max_files, out, transcription_dir=None, files_per_step=FILES_PER_STEP,
                  frame_size=400, frame_step=160, fft_n=512, n_filters=26, mfcc_num=13, resample=False):
    """dataset_creator.py:19-73: every .wav / .sph file of the directories (or
    file paths) ``files``, at most ``max_files`` of them, ``files_per_step`` at
    a time: read and decode on the host (with the transcript
    ``transcription_dir/<stem>.stm`` when a directory is given), one
    ``ClipBatch`` and one H2D copy per chunk, the offline feature rows of all
    its files packed clip after clip, ``scale_features`` over the chunk on the
    device, one D2H copy, and the CSV text with label ``files_type`` written
    to ``out`` (a text file object).  Returns the rows written per file.
    resample: a chunk with a file at another rate than the front end's is
    converted on the device into the packed buffer (one launch per distinct
    rate, vad_amd.resample.resample_clips), after the transcript's segments
    were gathered at each file's own rate; False (the default) takes every
    file's samples as they are, as the reference does."""
    from .batch import ClipBatch
    todo = list_audio_files(files, max_files)
    pipe = _pipeline(frame_size, frame_step, fft_n, n_filters, mfcc_num)
    counts = []
    for lo in range(0, len(todo), max(int(files_per_step), 1)):
        clips, rates = [], []
        for path in todo[lo:lo + max(int(files_per_step), 1)]:
            rate, raw = read_audio(path)
            rates.append(int(rate))
            if transcription_dir is not None:
                stem = path.split('/')[-1].split('.')[0]
                raw = gather_segments(raw, transcription_dir + '/' + stem + '.stm', rate)
            clips.append(np.ascontiguousarray(np.asarray(raw)))
        if any(c.dtype != np.int16 for c in clips):  # as file_features: anything but int16 PCM goes in as fp32
            clips = [c.astype(np.float32) for c in clips]
        if resample and any(r != pipe.cfg.sample_rate for r in rates):
            from .resample import resample_clips
            batch = resample_clips(clips, rates, pipe.cfg)
        else:
            batch = ClipBatch.from_host(clips, pipe.cfg)
        rows = pipe.features_batch(batch, mode=_lib.FEAT_OFFLINE, packed=True)
        scale_rows_device(rows)
        out.write(format_csv_rows(rows.cpu().numpy(), files_type))
        counts.extend(batch.host["n_rows"].tolist())
    return counts


# ----------------------------------------------------------------------------
# Reading the CSVs back: dataset/file_processing.py:151-242, file_index.py,
# learning/utils.py, dataset/__init__.py:38-96
# ----------------------------------------------------------------------------
CSV_CHUNK_BYTES = 64 << 20  # pinned staging buffer of read_csv_device
_TORCH_OF = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}


def _csv_source(path_or_bytes):
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        return io.BytesIO(bytes(path_or_bytes))
    return open(path_or_bytes, "rb")


def _after_last_newline(view, n):
    """One past the last '\n' of view[:n]; 0 when there is none."""
    hi = n
    while hi > 0:
        lo = max(0, hi - (1 << 16))
        hit = np.flatnonzero(view[lo:hi] == 10)
        if len(hit):
            return lo + int(hit[-1]) + 1
        hi = lo
    return 0


def _csv_chunks(f, chunk_bytes):
    """Pieces of the file cut after a '\n' (the last one at the end of the
    file), each as a view of one pinned staging buffer, with the piece's
    offset in the file.  A line longer than the buffer grows the buffer."""
    size = max(int(chunk_bytes or CSV_CHUNK_BYTES), 1)
    stage = torch.empty(size, dtype=torch.uint8, pin_memory=True)
    view = stage.numpy()
    filled, base = 0, 0
    while True:
        if filled == len(view):  # no line ends in a full buffer
            bigger = torch.empty(2 * len(view), dtype=torch.uint8, pin_memory=True)
            bigger.numpy()[:filled] = view[:filled]
            stage, view = bigger, bigger.numpy()
        got = f.readinto(memoryview(view)[filled:]) or 0
        filled += got
        eof = got == 0
        if filled == 0:
            return
        cut = filled if eof else _after_last_newline(view, filled)
        if cut == 0:
            continue
        yield stage, view, cut, base
        rest = filled - cut
        if rest:
            view[:rest] = view[cut:filled].copy()
        filled, base = rest, base + cut
        if eof:
            return


def _line_fields(view, start, end):
    line = bytes(memoryview(view)[start:end]).decode("latin-1")
    return line.rstrip("\r\n").split(",")


def read_csv_device(path_or_bytes, offset=1, columns_used=None, dtype=torch.float32, device=None,
                    chunk_bytes=None, max_rows=None):
    """A dataset CSV (a path, or its bytes) -> ``(X, y, index)`` on the device:
    X (n_rows, n_used) of ``dtype`` (float32 or float64) with exactly the
    values of ``np.asarray(csv row, dtype)``, y uint8 =
    ``int(float(last field))``, index int64 = the byte offset of every data
    line (``create_file_index``).  ``offset`` lines are skipped first;
    ``columns_used`` is a list of column indices (default: all but the last).
    The number of columns is that of the file's first line.

    The file is read through one pinned buffer of ``chunk_bytes`` in pieces
    cut at line ends, so any file size works; ``max_rows`` stops after that
    many data rows.  Rows whose text the device does not decide (more than 19
    significant digits, blanks, ...) are parsed here with ``float()``.
    ValueError, naming the 1-based line: a row with another number of fields
    or longer than 4096 bytes, a field ``float()`` refuses, a label outside
    0..255.  Columns that are not used are not parsed."""
    if dtype not in (torch.float32, torch.float64):
        raise TypeError("dtype must be torch.float32 or torch.float64")
    dev = torch.device("cuda" if device is None else device)
    lib = _lib.lib()
    cols = None
    if columns_used is not None and len(columns_used):
        cols = (ctypes.c_int32 * len(columns_used))(*[int(c) for c in columns_used])
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    skip_left, n_cols, rows_done = int(offset), None, 0
    Xs, ys, idxs = [], [], []
    with torch.cuda.device(dev), _csv_source(path_or_bytes) as f:
        st = _lib.stream_ptr()
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        for stage, view, cut, base in _csv_chunks(f, chunk_bytes):
            if max_rows is not None and rows_done >= max_rows:
                break
            if n_cols is None:  # the file's first line (the header, when there is one)
                first = bytes(memoryview(view)[:cut]).split(b"\n", 1)[0]
                n_cols = first.count(b",") + 1
                if n_cols < 2:
                    raise ValueError("line 1: a dataset CSV has at least one feature column and a label")
                if cols is not None and not all(0 <= c < n_cols for c in cols):
                    raise ValueError(f"columns_used outside the file's {n_cols} columns")
            d_bytes = torch.empty(cut, dtype=torch.uint8, device=dev)
            d_bytes.copy_(stage[:cut], non_blocking=True)
            nb = int(lib.vad_csv_workspace_bytes(cut))
            ws = torch.empty(nb // 8, dtype=torch.int64, device=dev)
            _lib.check(lib.vad_csv_count_lines(_lib.ptr(d_bytes), cut, _lib.ptr(count), _lib.ptr(ws), nb, st),
                       "vad_csv_count_lines")
            n_lines = int(count.item())  # also: the copy out of the staging buffer is done
            skip = min(skip_left, n_lines)
            skip_left -= skip
            n_rows = n_lines - skip
            if max_rows is not None:
                n_rows = min(n_rows, max_rows - rows_done)
            if n_rows == 0:
                continue
            index = torch.empty(n_rows, dtype=torch.int64, device=dev)
            _lib.check(lib.vad_csv_index(_lib.ptr(d_bytes), cut, skip, base, _lib.ptr(index), n_rows, _lib.ptr(ws),
                                         nb, st), "vad_csv_index")
            n_used = len(cols) if cols is not None else n_cols - 1
            X = torch.empty((n_rows, n_used), dtype=dtype, device=dev)
            y = torch.empty(n_rows, dtype=torch.uint8, device=dev)
            status = torch.empty(n_rows, dtype=torch.int32, device=dev)
            # the text of exactly these rows: the last one ends where the next line starts
            end = cut
            if n_rows < n_lines - skip:
                nxt = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
                _lib.check(lib.vad_csv_index(_lib.ptr(d_bytes), cut, skip, base, _lib.ptr(nxt), n_rows + 1,
                                             _lib.ptr(ws), nb, st), "vad_csv_index")
                end = int(nxt[-1].item()) - base
            _lib.check(lib.vad_csv_parse(_lib.ptr(d_bytes), end, _lib.ptr(index), n_rows, base, n_cols, cols, n_used,
                                         int(dtype == torch.float64), _lib.ptr(X), _lib.ptr(y), _lib.ptr(status),
                                         st), "vad_csv_parse")
            bad = torch.nonzero(status).flatten()
            if bad.numel():
                _patch_rows(view, end, base, index, bad, status, X, y, cols, n_cols, np_dtype,
                            int(offset) + rows_done)
            Xs.append(X)
            ys.append(y)
            idxs.append(index)
            rows_done += n_rows
    if not Xs:
        n_used = len(cols) if cols is not None else max((n_cols or 1) - 1, 0)
        return (torch.empty((0, n_used), dtype=dtype, device=dev), torch.empty(0, dtype=torch.uint8, device=dev),
                torch.empty(0, dtype=torch.int64, device=dev))
    if len(Xs) == 1:
        return Xs[0], ys[0], idxs[0]
    return torch.cat(Xs), torch.cat(ys), torch.cat(idxs)


def _patch_rows(view, end, base, index, bad, status, X, y, cols, n_cols, np_dtype, lines_before):
    """The rows the device flagged, parsed as numpy parses them, from the text
    still in the staging buffer; raises for what numpy refuses."""
    rows = bad.cpu().numpy()
    codes = status[bad].cpu().numpy()
    starts = index[bad].cpu().numpy() - base
    nxt = torch.clamp(bad + 1, max=index.numel() - 1)
    ends = np.where(rows + 1 < index.numel(), index[nxt].cpu().numpy() - base, end)
    used = list(cols) if cols is not None else list(range(n_cols - 1))
    px = np.empty((len(rows), len(used)), np_dtype)
    py = np.empty(len(rows), np.uint8)
    for k, (r, code, a, b) in enumerate(zip(rows, codes, starts, ends)):
        ln = lines_before + int(r) + 1
        fields = _line_fields(view, int(a), int(b))
        if code & _lib.CSV_ROW_MALFORMED:
            if len(fields) != n_cols:
                raise ValueError(f"line {ln}: {len(fields)} fields, expected {n_cols}")
            raise ValueError(f"line {ln}: longer than {_lib.CSV_MAX_LINE} bytes")
        try:
            vals = [float(fields[c]) for c in used]
            label = int(float(fields[-1]))
        except (ValueError, OverflowError) as e:
            raise ValueError(f"line {ln}: {e}") from None
        if not 0 <= label <= 255:
            raise ValueError(f"line {ln}: label {fields[-1]!r} is outside 0..255")
        px[k] = np.asarray(vals, np.float64).astype(np_dtype)
        py[k] = label
    X[bad] = torch.from_numpy(px).to(X.device)
    y[bad] = torch.from_numpy(py).to(y.device)


def load_csv(fname, items_num, columns_used=None, memmap=False, dtype=np.float32):
    """file_processing.py:151-184: the first ``items_num`` data rows after the
    header line as numpy ``features`` (items_num, d) of ``dtype`` and
    ``results`` (items_num, 1) int32.  ValueError when the file has fewer
    rows (the reference's ``reader.next()`` raises there too).  ``memmap`` is
    accepted and unused, as in the reference.  Parsed on the device."""
    tdt = _TORCH_OF.get(np.dtype(dtype))
    if tdt is None:
        raise TypeError("dtype must be float32 or float64")
    X, y, _ = read_csv_device(fname, 1, list(columns_used) if columns_used is not None else None, tdt,
                              max_rows=int(items_num))
    if X.shape[0] < items_num:
        raise ValueError(f"{fname}: {X.shape[0]} data rows, {items_num} asked for")
    return X.cpu().numpy(), y.cpu().numpy().astype(np.int32).reshape(-1, 1)


def load_files(files, features_num, dtype=np.float64):
    """learning/utils.py:5-21: ``load_csv`` of every file, concatenated along
    axis 0 (what the reference plainly meant: its ``np.concatenate`` of a 1-D
    empty array with a 2-D one raises)."""
    parts = [load_csv(f, n, dtype=dtype) for f, n in zip(files, features_num)]
    if not parts:
        return np.empty((0, 0), dtype), np.empty((0, 1), np.int32)
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def create_file_index(path, offset=1):
    """file_index.py:7-23: the byte offset of every line after the first
    ``offset`` lines, uint64; counted and filled on the device."""
    lib = _lib.lib()
    dev = torch.device("cuda")
    out, skip_left = [], int(offset)
    with _csv_source(path) as f:
        st = _lib.stream_ptr()
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        for stage, view, cut, base in _csv_chunks(f, None):
            d_bytes = torch.empty(cut, dtype=torch.uint8, device=dev)
            d_bytes.copy_(stage[:cut], non_blocking=True)
            nb = int(lib.vad_csv_workspace_bytes(cut))
            ws = torch.empty(nb // 8, dtype=torch.int64, device=dev)
            _lib.check(lib.vad_csv_count_lines(_lib.ptr(d_bytes), cut, _lib.ptr(count), _lib.ptr(ws), nb, st),
                       "vad_csv_count_lines")
            n_lines = int(count.item())
            skip = min(skip_left, n_lines)
            skip_left -= skip
            if n_lines == skip:
                continue
            index = torch.empty(n_lines - skip, dtype=torch.int64, device=dev)
            _lib.check(lib.vad_csv_index(_lib.ptr(d_bytes), cut, skip, base, _lib.ptr(index), n_lines - skip,
                                         _lib.ptr(ws), nb, st), "vad_csv_index")
            out.append(index.cpu().numpy().astype(np.uint64))
    return np.concatenate(out) if out else np.asarray([], dtype=np.uint64)


def features_number(path):
    """file_processing.py:231-233: the number of data lines of a dataset CSV
    (the length of its index; the index is computed, not read from an h5py
    file)."""
    return len(create_file_index(path))


def random_rows_order(sizes, total_size=1.0, lines_per_block=8, seed=0):
    """The order in which random_features_generator (dataset/__init__.py:38-96)
    over create_random_file_gen sources (file_processing.py:214-228) visits
    rows, as int32 row numbers into the concatenation of the sources (source
    i's rows start at sum(sizes[:i])), for ``FFNTrainer.steps``.

    Per source ``int(total_size * n_i)`` rows in runs of ``lines_per_block``
    consecutive rows from uniformly drawn starts (the last run is cut to the
    count); the sources are interleaved by drawing each next row from a
    source with probability proportional to the rows it has left, which is a
    uniform shuffle of the sources' labels.  Same distribution, not numpy's
    legacy random stream.  Two reference bugs are not kept: its starts are
    drawn from [0, n_i] inclusive and its runs read past the end of the file;
    here starts lie in [0, n_i - lines_per_block] (0 for a shorter source)."""
    rng = np.random.default_rng(seed)
    lpb = int(lines_per_block)
    if lpb < 1:
        raise ValueError("lines_per_block must be positive")
    seqs, base = [], 0
    for n in sizes:
        n = int(n)
        m = int(total_size * n)
        if m > 0:
            run = min(lpb, n)
            starts = rng.integers(0, n - run + 1, size=-(-m // run))
            seq = (starts[:, None] + np.arange(run)[None, :]).reshape(-1)[:m] + base
        else:
            seq = np.empty(0, np.int64)
        seqs.append(seq)
        base += n
    if base >= 1 << 31:
        raise ValueError("more than 2^31 rows")
    labels = np.repeat(np.arange(len(seqs)), [len(s) for s in seqs])
    rng.shuffle(labels)
    order = np.empty(len(labels), np.int32)
    for i, seq in enumerate(seqs):
        order[labels == i] = seq
    return order
