"""The transform lengths, rates and grid shapes of the SimpleAnalyser feature
kernels (vad_amd/csrc/simple_kernel.hip, simple_wave.h and the block and
two-launch paths of simple_stream_kernel.hip), and what the tests of every
length share: the case table with the path each case exists for, a float64
reference of the features with explicit L / pad / band_bins / n_bands, the
frame generators, the comparison, and a NumPy model of the direct kernel's
twiddle scheme (tests/test_simple_lengths_cpu.py measures both against a
long-double DFT; tests/test_gpu_simple_lengths.py runs the kernels).

The kernels choose their path from L = frame_size + 2 * pad:

  power of two    simple_features_wave_kernel, one wave per frame: 4 waves per
                  block up to L = 2048 (144 KB there), 2 at 4096 (the whole
                  160 KB), 1 at 8192 with a sincospi per butterfly and no
                  table; below 64 some lanes have no butterfly
  any other L     simple_features_kernel, 256 threads per frame and a direct
                  DFT whose twiddles are exact every 16th term and rotated in
                  between; L = 8193 takes 128 KB

band_bins = int(1000 / (rate / fftn)) is L / 16 at 16 kHz; the other rates
move the band edges off the multiples of 64 and, at 4 kHz, to the end of the
spectrum.
"""
import numpy as np

from oracle import vad_oracle as O

RTOL = 1e-11   # tests/test_simple_analyser.py::test_gpu_features_match_oracle's

# (frame_rate, frame_size): L, pad -- the path
POW2_CASES = [
    (4000, 4),      # L 4, band_bins 1: log2L = 2, 62 idle lanes, the four bands the whole spectrum
    (16000, 16),    # L 16, band_bins 1: 8 butterflies per stage
    (16000, 64),    # L 64: 32 butterflies, the first length with every lane loading
    (16000, 100),   # L 128, pad 14: the first length with two rows of lanes, padded
    (16000, 1000),  # L 1024, pad 12
    (16000, 1500),  # L 2048, pad 274: 4 waves in 144 KB
    (16000, 2048),  # L 2048, pad 0
    (16000, 3000),  # L 4096, pad 548: 2 waves, the whole 160 KB
    (16000, 4096),  # L 4096, pad 0
    (16000, 8192),  # L 8192, pad 0: 1 wave, no twiddle table
    (16000, 8190),  # L 8192, pad 1
    (16000, 4098),  # L 8192, pad 2047: half the transform is padding
]
ODD_CASES = [
    (4000, 3),      # L 5, pad 1: 251 idle threads
    (16000, 15),    # L 17, pad 1: one exact twiddle and one rotated term past it
    (16000, 255),   # L 257, pad 1: 256 threads, 257 bins
    (16000, 1023),  # L 1025, pad 1
    (16000, 4095),  # L 4097, pad 1
    (16000, 8191),  # L 8193, pad 1: 128 KB
    (16000, 4097),  # L 8193, pad 2048: pad larger than half the frame
]
RATE_CASES = [
    (8000, 400),    # L 512, band_bins 64
    (4000, 400),    # L 512, band_bins 128: the four bands are every bin
    (4000, 401),    # L 513, band_bins 128: one bin outside
    (22050, 400),   # band_bins 23
    (44100, 400),   # band_bins 11
    (48000, 400),   # band_bins 10
    (44100, 8191),  # L 8193, band_bins 185
]
CASES = POW2_CASES + ODD_CASES + RATE_CASES

# (frame_rate, frame_size, noise_buf_len, input dtype): the stream block kernel
# (one launch, power-of-two L <= 4096)
BLOCK_CASES = [
    (16000, 64, 4, "float32"),
    (16000, 1000, 4, "float32"),
    (16000, 1000, 4, "int16"),
    (16000, 2048, 4, "float32"),
    (16000, 2048, 64, "float32"),   # the largest LDS layout that still has 4 waves
    (16000, 3000, 4, "float32"),    # L 4096: one wave
    (16000, 4096, 4, "float32"),
    (16000, 4096, 4, "int16"),
    (8000, 400, 4, "float32"),
    (44100, 400, 4, "float32"),
]
BLOCK_S, BLOCK_K, BLOCK_T = 3, 5, 23   # the tail block is short
# the two-launch path: L 257, 8192 (a power of two past the block kernel), 8193
TWO_LAUNCH_CASES = [(16000, 255, 4, "float32"), (16000, 8192, 4, "float32"), (16000, 8191, 4, "float32")]
TWO_S, TWO_K, TWO_T = 2, 3, 7
SESSIONS_CASE = (16000, 1000, 4)       # L 1024
SESSIONS_S, SESSIONS_K = 3, 5
# frames taken per block and stream: stream 0 every frame (a short last
# block), stream 1 joins two blocks late, stream 2 stalls twice and takes
# ragged counts
SESSIONS_COUNTS = np.array([[5, 0, 5], [5, 0, 2], [5, 5, 0], [5, 5, 3], [5, 4, 5], [5, 5, 0], [3, 5, 5]], np.int32)
SESSIONS_SEED = 6   # sessions_reference() labels 0 and 1 in every stream (asserted where it is used)

# (rate, frame size, noise_buf_len) -> seed (stream s of a case uses seed + s):
# the first for which the float64 reference labels both 0 and 1 in every
# stream, found with stream_seed(); tests/test_simple_lengths_cpu.py asserts
# that property of each.
STREAM_SEEDS = {
    (16000, 64, 4): 3, (16000, 1000, 4): 6, (16000, 2048, 4): 3, (16000, 2048, 64): 3, (16000, 3000, 4): 12,
    (16000, 4096, 4): 0, (8000, 400, 4): 12, (44100, 400, 4): 12,
    (16000, 255, 4): 12, (16000, 8192, 4): 6, (16000, 8191, 4): 12,
}


def geometry(frame_rate, frame_size):
    """(L, pad, band_bins) of a (rate, frame size) pair, from the oracle."""
    fftn, pad, bb = O.simple_fft_layout(frame_size, frame_rate)
    return frame_size + 2 * pad, pad, bb


def is_pow2(L):
    return L >= 2 and L & (L - 1) == 0


def path_of(L):
    """The name of the feature path a length takes (for the error report)."""
    if is_pow2(L):
        return "wave, LDS twiddles" if L <= 4096 else "wave, L = 8192"
    return "direct, L <= 1025" if L <= 1025 else "direct, L >= 4097"


# ---------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------
def ref_features(frame_f32, L, pad, band_bins, n_bands=4):
    """[stEnergy, stZCR * n, std|fft|, n_bands band energies] of one frame in
    float64: oracle.vad_oracle.simple_frame_features with L, pad, band_bins
    and n_bands explicit.  frame_f32: the exact float32 samples."""
    frame = np.asarray(frame_f32, np.float32).astype(np.float64)
    n = len(frame)
    assert L == n + 2 * pad
    if pad > 0:
        x = np.concatenate([np.zeros(pad), frame, np.zeros(pad)])
    else:
        x = frame[0:L]
    X = np.fft.fft(x)
    mag = np.sqrt(np.real(X) ** 2 + np.imag(X) ** 2)
    bands = [O.st_energy(mag[i * band_bins:(i + 1) * band_bins]) for i in range(n_bands)]
    return np.array([O.st_energy(frame), O.st_zcr(frame) * n, np.std(mag)] + bands)


def ref_rows(frames_f32, L, pad, band_bins, n_bands=4):
    return np.array([ref_features(f, L, pad, band_bins, n_bands) for f in frames_f32])


def features_from_mag(frame64, mag, band_bins, n_bands=4):
    """The same seven values from a magnitude spectrum computed elsewhere (a
    long-double DFT, the model of the direct kernel), in mag's precision."""
    n = len(frame64)
    bands = [np.sum(mag[i * band_bins:(i + 1) * band_bins] ** 2) / band_bins for i in range(n_bands)]
    mean = np.sum(mag) / len(mag)
    std = np.sqrt(np.sum((mag - mean) ** 2) / len(mag))
    return np.array([O.st_energy(frame64), O.st_zcr(frame64) * n, std] + bands, mag.dtype)


def padded(frame_f32, L, pad, dtype=np.float64):
    x = np.zeros(L, dtype)
    f = np.asarray(frame_f32, np.float32).astype(dtype)
    x[pad:pad + len(f)] = f
    return x


def longdouble_mag(x):
    """|DFT| of x by the definition, in np.longdouble: one exact-argument
    twiddle exp(-2 pi i (k n mod L) / L) per term, rows of 128 bins at a time;
    only the first L // 2 + 1 bins are summed (x is real)."""
    L = len(x)
    ld = np.longdouble
    x = np.asarray(x, ld)
    ang = -2 * (ld(4) * np.arctan(ld(1))) * np.arange(L).astype(ld) / ld(L)
    wc, ws = np.cos(ang), np.sin(ang)
    n = np.arange(L, dtype=np.int64)
    half = L // 2 + 1
    mag = np.zeros(L, ld)
    for k0 in range(0, half, 128):
        k = np.arange(k0, min(k0 + 128, half), dtype=np.int64)
        idx = (k[:, None] * n[None, :]) % L
        re, im = wc[idx] @ x, ws[idx] @ x
        mag[k] = np.sqrt(re * re + im * im)
    mag[half:] = mag[1:L - half + 1][::-1]
    return mag


def direct_model(x):
    """|DFT| of x as simple_features_kernel sums it, in float64: the twiddle
    of term n exact when n % 16 == 0 and the previous one rotated by
    exp(-2 pi i k / L) otherwise, the terms added in order.  A model of the
    scheme, not of the kernel's arithmetic (no fma, libm's sin / cos for
    sincospi), vectorised over the bins: it shows what the scheme costs in
    accuracy, the kernel itself is measured on the device."""
    L = len(x)
    x = np.asarray(x, np.float64)
    k = np.arange(L, dtype=np.int64)
    ck, sk = np.cos(-2 * np.pi * k / L), np.sin(-2 * np.pi * k / L)
    ar, ai = np.zeros(L), np.zeros(L)
    c, s = np.ones(L), np.zeros(L)
    for n in range(L):
        if n % 16 == 0:
            a = -2 * np.pi * ((k * n) % L) / L
            c, s = np.cos(a), np.sin(a)
        ar += x[n] * c
        ai += x[n] * s
        c, s = c * ck - s * sk, s * ck + c * sk
    return np.sqrt(ar * ar + ai * ai)


def rel_err(got, ref):
    """max |got - ref| / |ref| over the entries with ref != 0 (0 if none)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    nz = ref != 0
    return float(np.max(np.abs(got[nz] - ref[nz]) / np.abs(ref[nz]))) if nz.any() else 0.0


def assert_features(got, ref, what=""):
    """Columns 0 and 1 equal (sums of squared integers and crossing counts are
    exact), the spectral columns within RTOL.  Returns their largest relative
    error."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    assert np.array_equal(got[:, 0], ref[:, 0]), what
    assert np.array_equal(got[:, 1], ref[:, 1]), what
    err = rel_err(got[:, 2:], ref[:, 2:])
    assert np.allclose(got[:, 2:], ref[:, 2:], rtol=RTOL, atol=0), (what, err)
    return err


# ---------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------
def noise_frames(n, frame_size, seed):
    """(n, frame_size) float32: integer-valued noise, sigma 3000, clipped to
    the int16 range.  8192 squares below 2^30 sum exactly in double."""
    rng = np.random.default_rng(seed)
    x = np.clip(np.rint(rng.normal(0, 3000, (n, frame_size))), -32768, 32767)
    return x.astype(np.float32)


def stream_frames(n, frame_size, seed, n_noise, frame_rate=16000, run=(3, 40)):
    """tests/golden/gen_simple.py's stream, restated: n_noise quiet frames,
    then noise (sigma 5) with voiced bursts (harmonics falling as 1 / h^2) and
    loud noise bursts, integer-valued, (n, frame_size) float32 in the int16
    range.  The generator's 150 - 250 Hz fundamental puts 7.5 - 12.5 zero
    crossings into its 400-sample frame at 16 kHz, inside the analyser's
    5 .. 20; here the fundamental is scaled to do the same for any frame size
    and rate, and keeps only the harmonics below half the rate.  run: the
    range of a burst's length in frames (the generator's 3 .. 40 suits its
    hundreds of frames)."""
    rng = np.random.default_rng(seed)
    t = np.arange(frame_size)
    scale = (400.0 / frame_size) * (frame_rate / 16000.0)
    out = []
    state, amp, left = "quiet", 1.0, 0
    for i in range(n):
        if i >= n_noise and left <= 0:
            state = rng.choice(["quiet", "voiced", "loud"], p=[0.45, 0.45, 0.10])
            left = int(rng.integers(run[0], run[1]))
            amp = 10 ** rng.uniform(2.0, 3.7)
        left -= 1
        x = rng.normal(0, 5, frame_size)
        if state == "voiced":
            f0 = rng.uniform(150, 250) * scale
            for h in range(1, 21):
                ph = rng.uniform(0, 0.3)
                if f0 * h < frame_rate / 2:
                    x += amp / h ** 2 * np.sin(2 * np.pi * f0 * h * (t + i * frame_size) / frame_rate + ph)
        elif state == "loud":
            x += rng.normal(0, amp / 4, frame_size)
        out.append(np.clip(np.rint(x), -32768, 32767))
    return np.asarray(out, np.float32)


def streams(frame_rate, frame_size, nb, n_streams, n_frames, seed):
    """init (S, nb, fs) and x (T, S, fs) float32: stream s is
    stream_frames(seed + s), its first nb frames the init frames."""
    fr = [stream_frames(nb + n_frames, frame_size, seed + s, nb, frame_rate, run=(2, 7)) for s in range(n_streams)]
    init = np.stack([f[:nb] for f in fr])
    x = np.stack([f[nb:] for f in fr], axis=1)
    return init, x


def reference_labels(frame_rate, frame_size, nb, init, x):
    """(T, S) labels of the float64 reference: ref_features rows through
    simple_stream_reference.run."""
    import simple_stream_reference as R
    L, pad, bb = geometry(frame_rate, frame_size)
    labs = [R.run(ref_rows(x[:, s], L, pad, bb), ref_rows(init[s], L, pad, bb), nb)[0] for s in range(x.shape[1])]
    return np.stack(labs, axis=1)


def stream_seed(frame_rate, frame_size, nb, n_streams, n_frames, limit=200):
    """The first seed whose streams all get both labels from the reference."""
    for seed in range(0, limit * n_streams, n_streams):
        init, x = streams(frame_rate, frame_size, nb, n_streams, n_frames, seed)
        labs = reference_labels(frame_rate, frame_size, nb, init, x)
        if all(set(labs[:, s].tolist()) == {0, 1} for s in range(n_streams)):
            return seed
    raise AssertionError("no seed gives both labels in every stream")


def sessions_blocks():
    """The sessions case's blocks (K, S, fs) float32, one per row of
    SESSIONS_COUNTS: each holds every stream's next K frames, of which the
    stream takes its count (its first noise_buf_len frames are init frames)."""
    rate, fs, nb = SESSIONS_CASE
    S, K = SESSIONS_S, SESSIONS_K
    n = nb + len(SESSIONS_COUNTS) * K
    fr = [stream_frames(n, fs, SESSIONS_SEED + s, nb, rate, run=(2, 7)) for s in range(S)]
    pos, out = [0] * S, []
    for c in SESSIONS_COUNTS:
        out.append(np.stack([fr[s][pos[s]:pos[s] + K] for s in range(S)], axis=1))
        pos = [p + int(k) for p, k in zip(pos, c)]
    return out


def sessions_reference(blocks):
    """The label blocks (K, S) of the float64 reference over sessions_blocks():
    ref_features rows through simple_stream_sessions_reference."""
    import simple_stream_sessions_reference as RS
    rate, fs, nb = SESSIONS_CASE
    L, pad, bb = geometry(rate, fs)
    ref = RS.RefSessions(SESSIONS_S, nb)
    labs = []
    for blk, c in zip(blocks, SESSIONS_COUNTS):
        rows = ref_rows(blk.reshape(-1, fs), L, pad, bb).reshape(SESSIONS_K, SESSIONS_S, 7)
        labs.append(ref.block(rows, c, [0] * SESSIONS_S)[0])
    return labs


# -- structured frames ---------------------------------------------------------
STRUCTURED_SIZES = [64, 512, 511, 4096, 8192, 8191]   # L 64, 512, 513, 4096, 8192, 8193
AMP = 1000.0


def impulse(n, at, a=AMP):
    x = np.zeros(n, np.float32)
    x[at] = a
    return x


def dc(n, a=AMP):
    return np.full(n, a, np.float32)


def alternating(n, a=AMP):
    x = np.full(n, a, np.float32)
    x[1::2] = -a
    return x


def tone(n, k, a=AMP):
    """a cos(2 pi k i / n) rounded to float32: bin k (and n - k) of an
    n-point transform, everything else at the rounding floor."""
    return (a * np.cos(2 * np.pi * k * np.arange(n) / n)).astype(np.float32)


def crossing_frame(n, seed=7):
    """Noise magnitudes of at least 1 under a sign pattern: a sign change
    exactly at 63|64, 255|256 and n-2|n-1 (the lane-stride and thread-stride
    seams of the kernels' x[i + 1] read) where the frame has them, a 0.0 /
    -0.0 pair at 5, 6 and a lone -0.0 at 20.  Returns the frame and the
    crossing sum / 2 it must give."""
    if n - 1 in (64, 256) or n <= 21:   # the same seam twice (two flips are none), or no room for the zeros
        raise AssertionError("choose another n")
    x = np.abs(noise_frames(1, n, seed)[0]) + 1
    half = 0.0
    for at in (64, 256, n - 1):
        if 20 < at < n:
            x[at:] = -x[at:]
            half += 1.0
    x[5], x[6] = 0.0, -0.0   # +, 0, -0, +: 1 + 0 + 1
    x[20] = -0.0             # +, -0, +: 1 + 1
    half += 2.0
    return x.astype(np.float32), half
