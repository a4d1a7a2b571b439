"""Host model of the live spectral subtraction of the hop kernels
(vad_amd/csrc/stream_denoise.h).

  estimate_f32   the noise estimate in the kernels' own fp32 order (an affine
                 scan across the 64 lanes, every operation one fp32 rounding):
                 the kernels equal it bit for bit
  estimate_f64   the same estimate from its formulas in float64
  estimate_serial_f32  the serial recurrence in float32, one rounding per
                 operation: the yardstick for the fp32 order's error
  replay         the noise-buffer bookkeeping from a label sequence and the
                 recorded spectra
"""
import numpy as np

BINS = 256
ROWS = 5
MIDDLE = 2  # the window's middle frame: the reference's PROCESSING_FRAME_INDEX

f32 = np.float32


def mean_f32(rows):
    """(((r0 + r1) + r2) + ...) / n in float32, rows in arrival order."""
    rows = np.asarray(rows, f32)
    s = rows[0].copy()
    for r in rows[1:]:
        s = s + r
    return s / f32(len(rows))


def estimate_f32(rows, alpha):
    """The kernels' estimate of `rows` ((n, 256) float32, arrival order; n = 0:
    all zero).  Lane l owns bins 4 l .. 4 l + 3."""
    rows = np.asarray(rows, f32).reshape(-1, BINS)
    if len(rows) == 0:
        return np.zeros(BINS, f32)
    with np.errstate(all="ignore"):
        m = mean_f32(rows)
        a = f32(alpha)
        beta = f32(1) - a
        b = (beta * m).reshape(64, 4)
        B = b[:, 0].copy()
        for j in (1, 2, 3):
            B = a * B + b[:, j]
        a2 = a * a
        A = np.full(64, a2 * a2, f32)
        for d in (1, 2, 4, 8, 16, 32):  # Kogge-Stone, inclusive: lanes l >= d combine with lane l - d
            Bn, An = B.copy(), A.copy()
            Bn[d:] = A[d:] * B[:-d] + B[d:]
            An[d:] = A[d:] * A[:-d]
            A, B = An, Bn
        x0 = m[BINS - 1]  # the reference's wrap: bin 0 takes bin 255 of the mean as its predecessor
        X = A * x0 + B
        prev = np.concatenate([[x0], X[:-1]]).astype(f32)
        e = np.empty((64, 4), f32)
        for j in range(4):
            prev = a * prev + b[:, j]
            e[:, j] = prev
    assert e.dtype == f32
    return e.reshape(BINS)


def estimate_serial_f32(rows, alpha):
    rows = np.asarray(rows, f32).reshape(-1, BINS)
    m = mean_f32(rows)
    a = f32(alpha)
    beta = f32(1) - a
    e = np.empty(BINS, f32)
    prev = m[BINS - 1]
    for i in range(BINS):
        prev = f32(f32(a * prev) + f32(beta * m[i]))
        e[i] = prev
    return e


def estimate_f64(rows, alpha):
    """e[0] = a m[255] + (1 - a) m[0], e[i] = a e[i-1] + (1 - a) m[i], m the
    mean of the rows; alpha as the float32 the kernels receive."""
    rows = np.asarray(rows, np.float64).reshape(-1, BINS)
    if len(rows) == 0:
        return np.zeros(BINS)
    m = rows.sum(axis=0) / len(rows)
    a = float(f32(alpha))
    e = np.empty(BINS)
    prev = m[BINS - 1]
    for i in range(BINS):
        prev = a * prev + (1.0 - a) * m[i]
        e[i] = prev
    return e


class Replay:
    """One stream's noise rows: push(row) appends, dropping the oldest row
    past five; rows() are those held, in arrival order."""

    def __init__(self, rows=()):
        self.held = [np.asarray(r, f32).copy() for r in rows]

    def push(self, row):
        self.held.append(np.asarray(row, f32).copy())
        if len(self.held) > ROWS:
            self.held.pop(0)

    def rows(self):
        return np.stack(self.held) if self.held else np.zeros((0, BINS), f32)


def replay(labels, spectra, noise_class, loaded=(), update=True):
    """The rows held after every hop.  labels: (T,) of one stream (255 = no
    window); spectra: (T, 256), the raw power row of the frame of hop t.  A hop
    whose window is labelled noise_class pushes the row of the window's middle
    frame: the window of hop t holds the frames of hops t-5 .. t-1, so that is
    the frame of hop t - 3.  Returns a list of (n_t, 256) arrays."""
    buf = Replay(loaded)
    out = []
    for t, lab in enumerate(labels):
        if update and lab != 255 and int(lab) == noise_class:
            buf.push(spectra[t - ROWS + MIDDLE])
        out.append(buf.rows())
    return out
