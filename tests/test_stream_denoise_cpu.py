"""The host model of the hop kernels' noise estimate and noise-buffer
bookkeeping (tests/stream_denoise_reference.py), without a device.

The estimate's fp32 order (an affine scan across the lanes) is checked
against the float64 formula.  The tolerance is not chosen by hand: the
yardstick is the SERIAL recurrence in float32, one rounding per operation,
against float64 on the same rows; the bound is twice that plus
4 * 2^-24 * max(m) for the other summation order.  Both are printed.
"""
import numpy as np
import pytest

import stream_denoise_reference as D


def rows_for(n, seed, spike):
    rng = np.random.default_rng(seed)
    r = (rng.random((n, D.BINS)) ** 4 * 10.0 ** rng.uniform(0, 9, size=(n, 1))).astype(np.float32)
    if spike:
        r[:, D.BINS - 1] *= np.float32(1e4)  # the wrap: bin 0 must see bin 255
    return r


@pytest.mark.parametrize("alpha", [0.9, 0.5, 0.0, 0.99])
@pytest.mark.parametrize("spike", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_fp32_order_against_float64(n, spike, alpha):
    worst = yard = 0.0
    for seed in range(8):
        r = rows_for(n, 100 * n + seed, spike)
        want = D.estimate_f64(r, alpha)
        got = D.estimate_f32(r, alpha).astype(np.float64)
        serial = D.estimate_serial_f32(r, alpha).astype(np.float64)
        m_max = float(r.astype(np.float64).mean(axis=0).max())
        err, y = np.abs(got - want).max(), np.abs(serial - want).max()
        assert err <= 2 * y + 4 * 2.0 ** -24 * m_max, (n, spike, alpha, seed, err, y, m_max)
        worst, yard = max(worst, err / m_max), max(yard, y / m_max)
    print(f"\nn={n} spike={spike} alpha={alpha}: max |scan - f64| = {worst * 2 ** 24:.2f} * 2^-24 max(m); "
          f"serial fp32 yardstick {yard * 2 ** 24:.2f} * 2^-24 max(m)")
    if spike:  # the wrap, pinned on its own: bin 0 sees bin 255 of the mean (at most ten roundings on the way)
        a = float(np.float32(alpha))
        m = r.astype(np.float64).mean(axis=0)
        assert abs(got[0] - (a * m[255] + (1 - a) * m[0])) <= 10 * 2.0 ** -24 * (m[255] + m[0])
        assert alpha == 0.0 or got[0] > 100 * m[0]


def test_estimate_edge_cases():
    assert not D.estimate_f32(np.zeros((0, D.BINS), np.float32), 0.9).any()
    assert not D.estimate_f64(np.zeros((0, D.BINS)), 0.9).any()
    # a flat spectrum is its own low pass, up to rounding: two roundings of 2^-24 relative per bin, carried on
    # with factor alpha (a geometric sum, 1 / (1 - alpha) = 10), plus the four of the mean and of b
    flat = np.full((3, D.BINS), 7.0, np.float32)
    assert np.abs(D.estimate_f32(flat, 0.9).astype(np.float64) - 7.0).max() <= 7.0 * (2 * 10 + 4) * 2.0 ** -24
    one = rows_for(1, 5, False)
    assert np.array_equal(D.estimate_f32(one, 0.0), one[0])  # alpha 0: the mean itself
    nan = rows_for(2, 6, False)
    nan[1, 100] = np.nan
    e = D.estimate_f32(nan, 0.5)
    # NaN runs on to the last bin; the wrap reads the MEAN's bin 255, which is finite
    assert np.isnan(e[100:]).all() and not np.isnan(e[:100]).any()
    assert np.array_equal(np.isnan(e), np.isnan(D.estimate_serial_f32(nan, 0.5)))


def spectra(T, seed=0):
    return np.random.default_rng(seed).random((T, D.BINS)).astype(np.float32)


def test_replay_fewer_than_five_pushes():
    sp = spectra(12)
    lab = np.array([255] * 5 + [1, 0, 1, 0, 0, 1, 1], np.uint8)
    held = D.replay(lab, sp, noise_class=0)
    assert [len(h) for h in held] == [0] * 6 + [1, 1, 2, 3, 3, 3]
    # hop 6 pushes the frame of hop 3, hop 8 that of hop 5, hop 9 that of hop 6
    assert np.array_equal(held[-1], sp[[3, 5, 6]])


def test_replay_eviction_past_five():
    sp = spectra(16, 1)
    lab = np.array([255] * 5 + [2] * 11, np.uint8)
    loaded = spectra(2, 2)
    held = D.replay(lab, sp, noise_class=2, loaded=loaded)
    assert [len(h) for h in held] == [2] * 5 + [3, 4, 5] + [5] * 8
    assert np.array_equal(held[7], np.concatenate([loaded, sp[[2, 3, 4]]]))
    assert np.array_equal(held[8], np.concatenate([loaded[1:], sp[[2, 3, 4, 5]]]))  # the oldest row left
    assert np.array_equal(held[-1], sp[[8, 9, 10, 11, 12]])


def test_replay_nothing_pushed_without_a_window_or_with_updates_off():
    sp = spectra(8, 3)
    loaded = spectra(3, 4)
    for lab, kw in ((np.full(8, 255, np.uint8), {}), (np.zeros(8, np.uint8), dict(update=False)),
                    (np.ones(8, np.uint8), {})):
        held = D.replay(lab, sp, noise_class=0, loaded=loaded, **kw)
        assert all(np.array_equal(h, loaded) for h in held)
    # class 255 never is a noise class: a stream's first hops push nothing whatever noise_class says
    assert all(len(h) == 0 for h in D.replay(np.full(8, 255, np.uint8), sp, noise_class=255))
