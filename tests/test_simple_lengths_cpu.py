"""What tests/test_gpu_simple_lengths.py stands on, checked without a GPU
(tests/simple_length_cases.py has the case table and the reference):

* the geometry of every frame size 2 .. 8192 and of every table case, as the
  stream module, the class and the oracle compute it, and which lengths the
  one-kernel stream path takes;
* ref_features against the oracle's simple_frame_features, bit for bit;
* the reference's own error against a long-double DFT by the definition: the
  GPU tolerance is rtol 1e-11, the reference has to be 100 times tighter;
* a NumPy model of the direct kernel's twiddle scheme (exact every 16th term,
  rotated in between) against the same long-double DFT: the scheme itself
  costs far less than the tolerance, which is why rtol 1e-11 is kept (the
  kernel's own sincospi and fma arithmetic is measured on the device only);
* the generators: exact float32 / int16 values, exact sums of squares, the
  crossing frame's count at every size used, and stream seeds for which the
  reference gives both labels in every stream, sessions included.
"""
import numpy as np
import pytest

import simple_length_cases as C
from oracle import vad_oracle as O
from vad_amd import simple_stream as SS
from vad_amd.simple_analyser import SimpleAnalyser


def test_geometry_of_every_frame_size():
    pairs = [(16000, fs) for fs in range(2, 8193)] + C.CASES
    for rate, fs in pairs:
        fftn, pad, bb = O.simple_fft_layout(fs, rate)
        assert SS.fft_geometry(rate, fs) == (fftn, pad, bb), (rate, fs)
        L = fs + 2 * pad
        assert L in (fftn, fftn + 1) and L <= 8193, (rate, fs)
        assert L == fftn + (fftn - fs) % 2
        assert 4 * bb <= L
        sa = SimpleAnalyser(rate, fs, 3)   # the class has its own copy of the arithmetic
        assert (sa.fftn, sa.fft_extended_zeros, sa.fftn_for_band) == (fftn, pad, bb), (rate, fs)
        assert sa._fft_len() == L == C.geometry(rate, fs)[0], (rate, fs)
    for L in range(0, 8300):
        assert SS.one_kernel_length(L) == (L in (2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096)), L


def test_case_table_reaches_the_paths_it_names():
    got = {(rate, fs): C.geometry(rate, fs) for rate, fs in C.CASES}
    assert got[(4000, 4)] == (4, 0, 1)
    assert got[(16000, 100)] == (128, 14, 8)
    assert got[(16000, 1000)] == (1024, 12, 64)
    assert got[(16000, 8190)][:2] == (8192, 1) and got[(16000, 4098)][:2] == (8192, 2047)
    assert got[(4000, 3)][:2] == (5, 1) and got[(16000, 15)][:2] == (17, 1) and got[(16000, 255)][:2] == (257, 1)
    assert got[(16000, 8191)][:2] == (8193, 1) and got[(16000, 4097)][:2] == (8193, 2048)
    assert got[(4000, 400)] == (512, 56, 128) and got[(4000, 401)] == (513, 56, 128)   # every bin / one outside
    assert [got[(r, 400)][2] for r in (8000, 22050, 44100, 48000)] == [64, 23, 11, 10]
    assert got[(44100, 8191)] == (8193, 1, 185)
    assert all(C.is_pow2(C.geometry(r, fs)[0]) for r, fs in C.POW2_CASES)
    assert not any(C.is_pow2(C.geometry(r, fs)[0]) for r, fs in C.ODD_CASES)
    assert {C.path_of(C.geometry(r, fs)[0]) for r, fs in C.CASES} == {
        "wave, LDS twiddles", "wave, L = 8192", "direct, L <= 1025", "direct, L >= 4097"}
    for rate, fs, nb, dt in C.BLOCK_CASES:
        assert SS.one_kernel_length(C.geometry(rate, fs)[0])
    assert [C.geometry(r, fs)[0] for r, fs, _, _ in C.TWO_LAUNCH_CASES] == [257, 8192, 8193]
    assert C.geometry(*C.SESSIONS_CASE[:2])[0] == 1024
    assert [C.geometry(16000, fs)[0] for fs in C.STRUCTURED_SIZES] == [64, 512, 513, 4096, 8192, 8193]


@pytest.mark.parametrize("rate,fs", C.CASES)
def test_ref_features_is_the_oracle(rate, fs):
    L, pad, bb = C.geometry(rate, fs)
    for fr in C.noise_frames(2, fs, 100 + fs):
        want = O.simple_frame_features(fr.astype(np.float64), fs, rate)
        assert C.ref_features(fr, L, pad, bb, 4).tobytes() == want.tobytes()


def test_generators_are_exact():
    x = C.noise_frames(3, 8192, 1)
    assert x.dtype == np.float32 and np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 32768
    assert np.array_equal(x.astype(np.int16).astype(np.float32), x)
    assert 2000 < x.std() < 4000
    for row in x:   # the sum of squares is an integer below 2^53, whatever the order
        assert float(np.sum(row.astype(np.float64) ** 2)) == float(sum(int(v) ** 2 for v in row))
    s = C.stream_frames(12, 255, 3, 4, 16000, run=(2, 7))
    assert s.shape == (12, 255) and np.array_equal(s.astype(np.int16).astype(np.float32), s)
    fr, half = C.crossing_frame(512)
    assert np.signbit(fr[6]) and fr[6] == 0 and fr[5] == 0 and not np.signbit(fr[5])
    assert fr[63] > 0 > fr[64] and fr[255] < 0 < fr[256] and fr[510] > 0 > fr[511] and half == 5.0
    assert O.st_zcr(fr.astype(np.float64)) * 511 == half
    for n in C.STRUCTURED_SIZES:    # the analytic count is the oracle's at every size the device test uses
        fr, half = C.crossing_frame(n)
        assert half == (3.0 if n == 64 else 5.0)
        assert np.sum(np.abs(np.diff(np.sign(fr.astype(np.float64))))) / 2 == half, n
        assert O.st_zcr(fr.astype(np.float64)) == half / (n - 1.0), n
        assert C.ref_features(fr, *C.geometry(16000, n))[1] == half / (n - 1.0) * n, n
    for n in (65, 257, 21):
        with pytest.raises(AssertionError, match="choose another n"):
            C.crossing_frame(n)


@pytest.mark.parametrize("fs", [512, 511, 4096, 8191])
def test_reference_error_against_long_double(fs):
    """ref_features (np.fft.fft in double) against the DFT by its definition
    in long double, L = 512, 513, 4096, 8193: at least 100 times tighter than
    the tolerance the kernels are held to."""
    L, pad, bb = C.geometry(16000, fs)
    fr = C.noise_frames(1, fs, 40 + fs)[0]
    mag = C.longdouble_mag(C.padded(fr, L, pad, np.longdouble))
    want = C.features_from_mag(fr.astype(np.longdouble), mag, bb)
    got = C.ref_features(fr, L, pad, bb)
    err = C.rel_err(got[2:], np.asarray(want[2:], np.longdouble).astype(np.float64))
    exact = np.abs((got - want) / want).astype(np.float64).max()
    print(f"L {L}: reference against long double, max relative feature error {exact:.2e}")
    assert exact <= C.RTOL / 100 and err <= C.RTOL / 100
    assert float(want[0]) == got[0] and float(want[1]) == got[1]


@pytest.mark.parametrize("fs", [3, 511, 8191])
def test_direct_twiddle_scheme_model(fs):
    """The direct kernel's scheme (an exact twiddle every 16th term, rotation
    in between) in NumPy, L = 5, 513, 8193: features as close to the
    long-double ones as the tolerance / 100.  A statement about the scheme,
    not about the kernel's sincospi and fma arithmetic, which only the device
    test measures."""
    rate = 4000 if fs == 3 else 16000
    L, pad, bb = C.geometry(rate, fs)
    fr = C.noise_frames(1, fs, 60 + fs)[0]
    x = C.padded(fr, L, pad)
    got = C.features_from_mag(fr.astype(np.float64), C.direct_model(x), bb)
    want = C.features_from_mag(fr.astype(np.longdouble), C.longdouble_mag(x), bb)
    err = np.abs((got - want) / want).astype(np.float64).max()
    print(f"L {L}: direct-scheme model against long double {err:.2e}")
    assert err <= C.RTOL / 100


def test_stream_seeds_give_both_labels():
    """Every stream of every stream case is labelled 0 and 1 by the float64
    reference, so the kernels' state machines are exercised."""
    cases = [(c[:3], C.BLOCK_S, C.BLOCK_T) for c in C.BLOCK_CASES] + \
            [(c[:3], C.TWO_S, C.TWO_T) for c in C.TWO_LAUNCH_CASES]
    assert {c for c, _, _ in cases} == set(C.STREAM_SEEDS)
    for (rate, fs, nb), S, T in dict.fromkeys(cases):
        seed = C.STREAM_SEEDS[(rate, fs, nb)]
        init, x = C.streams(rate, fs, nb, S, T, seed)
        assert init.shape == (S, nb, fs) and x.shape == (T, S, fs)
        labs = C.reference_labels(rate, fs, nb, init, x)
        for s in range(S):
            assert set(labs[:, s].tolist()) == {0, 1}, (rate, fs, nb, s)
    # the sessions case: every stream has init frames, rows without a frame, and both labels
    blocks = C.sessions_blocks()
    assert len(blocks) == len(C.SESSIONS_COUNTS) and blocks[0].shape == (C.SESSIONS_K, C.SESSIONS_S, 1000)
    labs = np.concatenate(C.sessions_reference(blocks))
    for s in range(C.SESSIONS_S):
        assert set(labs[:, s].tolist()) == {0, 1, 253, 254}, s
