"""Resampling without a GPU (vad_amd/resample.py): the filter is
scipy.signal.resample_poly's default, the float64 model is resample_poly, the
hop-by-hop stream model is the clip model delayed by d, and the Python layer
refuses what the device cannot take."""
import numpy as np
import pytest

import resample_edge_plans as E
from vad_amd import resample as R
from vad_amd.config import MfccConfig

# (rate_in, rate_out) for the ratios 1/3, 2/1, 160/441, 640/441, 1/6, 2/3, 1/1
RATES = [(48000, 16000), (8000, 16000), (44100, 16000), (11025, 16000), (96000, 16000), (24000, 16000),
         (16000, 16000)]
RATIOS = [(1, 3), (2, 1), (160, 441), (640, 441), (1, 6), (2, 3), (1, 1)]
# and every edge plan (tests/resample_edge_plans.py) not among them
EDGE = [r for r in E.EDGE_RATES if (r, 16000) not in RATES]
RATES += [(r, 16000) for r in EDGE]
RATIOS += [E.EDGE_PLANS[r][:2] for r in EDGE]


@pytest.mark.parametrize("rates,ratio", list(zip(RATES, RATIOS)))
def test_taps_and_lengths_are_scipys(rates, ratio):
    from scipy.signal import firwin, resample_poly
    s = R.ResampleSpec(*rates)
    up, down = ratio
    assert (s.up, s.down) == ratio
    mx = max(up, down)
    if mx == 1:
        assert s.half_len == 0 and np.array_equal(s.taps, [1.0])
    else:
        assert s.half_len == 10 * mx and len(s.taps) == 2 * s.half_len + 1
        want = firwin(2 * s.half_len + 1, 1.0 / mx, window=("kaiser", 5.0)) * up
        err = np.abs(s.taps - want).max()
        print(f"{up}/{down}: max |taps - firwin * up| = {err:.3e}")
        assert err <= 1e-15
    assert s.taps.dtype == np.float64
    assert s.phase_len == -(-(2 * s.half_len + 1) // up)
    assert s.delay == -(-s.half_len // down)
    for n in (0, 1, 2, down - 1, down, down + 1, 10007):
        if n == 0:  # resample_poly takes no empty input
            assert s.n_out(0) == 0
        else:
            assert s.n_out(n) == len(resample_poly(np.zeros(n), up, down)), n


@pytest.mark.parametrize("rates", RATES)
def test_model_is_resample_poly(rates):
    from scipy.signal import resample_poly
    s = R.ResampleSpec(*rates)
    rng = np.random.default_rng(s.up * 1000 + s.down)
    n = 2003
    head, tail = np.zeros(n), np.zeros(n)
    head[0], tail[-1] = 1.0, -2.0
    for name, x in (("noise", rng.standard_normal(n) * 3000), ("impulse at 0", head), ("impulse at end", tail),
                    ("constant", np.full(n, 7.5)), ("int16", rng.integers(-32768, 32768, 517).astype(np.int16))):
        got = R.resample_model(x, s)
        want = resample_poly(np.asarray(x).astype(np.float64), s.up, s.down)
        assert got.shape == want.shape and got.dtype == np.float64
        err = np.abs(got - want).max()
        print(f"{s.up}/{s.down} {name}: max err {err:.3e}")
        assert err <= 1e-12 * np.abs(x).max()
    assert R.resample_model(np.zeros(0), s).shape == (0,)
    assert np.array_equal(R.resample_model([3.0], s, taps=s.taps), R.resample_model([3.0], *rates))


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("rate", [48000, 8000, 44100, 32000])
def test_stream_model_is_the_clip_model_delayed(rate, K):
    S, blocks = 2, 3
    s = R.ResampleSpec(rate)
    m = R.StreamModel(S, rate)
    assert m.hop_in == rate // 100 and m.hop_out == 160
    rng = np.random.default_rng(rate + K)
    x = rng.integers(-32768, 32768, (blocks * K, S, m.hop_in)).astype(np.float64)
    z = np.concatenate([m.step(x[b * K:(b + 1) * K]) for b in range(blocks)])
    tail = m.flush()
    d = s.delay
    assert tail.shape == (S, d)
    for i in range(S):
        whole = R.resample_model(x[:, i].reshape(-1), s)
        assert len(whole) == blocks * K * 160
        got = np.concatenate([z[:, i].reshape(-1), tail[i]])
        assert np.array_equal(got[:d], np.zeros(d))
        assert np.array_equal(got[d:], whole)  # exactly: the same sums in the same order
    # the history is as long as the derivation says and no longer than needed
    assert s.history == -(-(d * s.down - s.half_len) // s.up) + s.phase_len - 1


def test_layout_of_the_outputs():
    from vad_amd.batch import layout
    cfg = MfccConfig()
    lens = [0, 1, 48000, 44100, 7, 12345]
    rates = [48000, 8000, 48000, 44100, 11025, 16000]
    t, total = R.plan_layout(lens, rates, cfg)
    outs = [R.ResampleSpec(r).n_out(n) for n, r in zip(lens, rates)]
    assert outs == [0, 2, 16000, 16000, 11, 12345]
    want, wtotal = layout(outs, cfg.frame_size, cfg.hop)
    assert total == wtotal and all(np.array_equal(t[k], want[k]) for k in want)
    one, _ = R.plan_layout(lens, 48000, cfg)
    assert one["len"].tolist() == [R.ResampleSpec(48000).n_out(n) for n in lens]
    with pytest.raises(ValueError):
        R.plan_layout(lens, rates[:-1], cfg)


def test_constants_match_the_header():
    import os
    import re
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(here, "include", "vad_amd.h")).read()
    for name, v in (("TILE", R.TILE_OUT), ("MAX_TABLE", R.MAX_TABLE), ("MAX_SPAN", R.MAX_SPAN)):
        assert int(re.search(rf"#define VAD_RESAMPLE_{name} (\d+)", src).group(1)) == v
    from vad_amd import _lib
    assert _lib.lib().vad_resample_tile_outputs() == R.TILE_OUT


def test_every_required_rate_fits():
    for rate in (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 96000):
        s = R.ResampleSpec(rate)
        assert s.up * s.row_stride <= R.MAX_TABLE and max(s.up, s.down) <= 640
    assert R.ResampleSpec(44100).phase_len == 56 and R.ResampleSpec(11025).phase_len == 21


@pytest.mark.parametrize("rate", E.EDGE_RATES)
def test_edge_plans_are_where_the_tests_expect_them(rate):
    """up, down, T, table, tile span, delay and history of every edge rate: a
    change of the filter design moves these, and the device tests with them."""
    s = R.ResampleSpec(rate)
    assert E.plan_sizes(s) == E.EDGE_PLANS[rate]
    up, down, T, table, span, delay, hist = E.EDGE_PLANS[rate]
    assert table <= R.MAX_TABLE and span <= R.MAX_SPAN
    assert s.row_stride == T | 1 and s.row_stride % 2 == 1
    if rate % 100 == 0:  # a stream's window: the history and K hops
        m = R.StreamModel(1, rate)
        assert m.hop_in == rate // 100 and m.spec.history == hist


def test_edge_plans_reach_the_limits():
    sizes = np.array([E.EDGE_PLANS[r] for r in E.EDGE_RATES])
    assert sizes[:, 3].max() == 16000 and sizes[:, 4].max() == 15646  # of 16384 each
    assert sizes[:, 2].max() == 301 and sizes[:, 6].max() == 300 and sizes[:, 6].min() == 20
    assert {26, 28} <= set(sizes[:, 2].tolist())  # even T, rows padded by one
    assert sorted(sizes[:, 5].tolist())[-2:] == [160, 320]  # delays of one and two whole hops
    # the next plan past either limit is refused (test_value_errors), so these are the last that fit
    assert 640 * (26 | 1) > R.MAX_TABLE and 1023 * 16 + 321 > R.MAX_SPAN


@pytest.mark.parametrize("rate", E.EDGE_RATES)
def test_the_bound_sees_an_off_by_one(rate):
    """The device test accepts |device - model| <= gamma sum |h||x|.  A kernel
    whose jl were one input sample off, or whose phase row r were one off,
    must fall outside it: on more than half of the outputs of every input the
    device test uses, white int16 noise.  Adjacent rows at 16100 and 15975
    are 1/160 and 1/640 of a sample apart, and still every case separates."""
    s = R.ResampleSpec(rate)
    h32 = E.taps32(s)
    worst = 1.0
    for n in E.lengths(s, R.TILE_OUT):
        x = E.clip_input(rate, n)
        want = R.resample_model(x, s, taps=h32)
        assert np.array_equal(E.shifted_model(x, s, h32), want)  # the unshifted form is the model
        if n == 0:
            continue
        bound = E.chain_bound(x, s)
        for kw in (dict(dj=1), dict(dj=-1), dict(dq=1), dict(dq=-1)):
            outside = float((np.abs(E.shifted_model(x, s, h32, **kw) - want) > bound).mean())
            worst = min(worst, outside)
            assert outside > 0.5, (rate, n, kw, outside)
    print(f"{rate} Hz: at least {worst:.4f} of the outputs of a model off by one lie outside the bound")


def test_edge_sessions_script_holds_its_cases():
    """The workload of test_gpu_resample_ratios.py's sessions tests, checked
    here against the float64 sessions model: the cases it is there for occur."""
    import resample_sessions_reference as SR
    rates, K = E.SESSION_RATES, 3
    counts, restart, rate = E.sessions_script()
    B, S = counts.shape
    hn = [R.ResampleSpec(r).history for r in rates]
    assert hn == [300, 20, 20, 120, 20, 60, 20, 40] and len(rates) == R.MAX_RATES
    assert restart[0].all() and set(counts.reshape(-1).tolist()) == set(range(-1, K + 2))
    rows = SR.session_rows(counts, restart, rate, len(rates), K)
    assert [s["rate"] for s in rows[0][1:]] == [0, 1, 0, 1]  # 240000 -> 500 -> 240000 -> 500
    assert [s["rate"] for s in rows[7][1:]] == [7, 0, 7]     # clamped indices
    shorter = sum(hn[b["rate"]] < hn[a["rate"]] and len(a["rows"]) > 0 for s in range(S)
                  for a, b in zip(rows[s][1:], rows[s][2:]))
    assert shorter == 7
    stalls = [(b, s) for b in range(B) for s in range(S) if counts[b, s] <= 0 and not restart[b, s]]
    assert len(stalls) >= 6 and (3, 1) in stalls
    # the model runs it: every session of the model is the clip model of its hops, delayed
    x = SR.audio(B, K, S, 2400, seed=979)
    m = SR.SessionsResampleModel(S, rates, K)
    emitted = []
    for b in range(B):
        out = m.step(x[b], counts[b], restart[b], rate[b])
        assert np.isnan(out[:, 5]).all() == (counts[b, 5] <= 0)
        emitted.append(min(m.model[1].emitted, m.model[1].spec.delay))
    assert emitted[:5] == [160, 0, 160, 160, 320]  # stream 1: restarted inside the delay of 500 Hz
    for s in range(S):
        for sess in m.sessions[s]:
            if not sess["hops"]:
                continue
            spec = R.ResampleSpec(rates[sess["rate"]])
            whole = R.resample_model(np.concatenate(sess["hops"]), spec)
            got = np.concatenate(sess["rows"])
            d = min(spec.delay, len(got))
            assert not got[:d].any() and np.array_equal(got[d:], whole[:len(got) - d]), (s, sess["rate"])


def test_value_errors():
    import torch
    for bad in (0, -8000, 8000.5):
        with pytest.raises(ValueError):
            R.ResampleSpec(bad)
        with pytest.raises(ValueError):
            R.StreamResampler(2, bad)
    with pytest.raises(ValueError):
        R.ResampleSpec(16000, 0)
    with pytest.raises(ValueError, match="LDS"):
        R.ResampleSpec(16001)          # 16000 / 16001: a phase table of 16000 x 21 floats
    with pytest.raises(ValueError, match="LDS"):
        R.Resampler(16001)
    with pytest.raises(ValueError, match="LDS"):
        R.ResampleSpec(16000 * 17)     # 1 / 17: the input tile
    with pytest.raises(ValueError, match="LDS"):
        R.ResampleSpec(256000)         # 1 / 16: 1023 * 16 + 321 = 16,689 floats of input tile, the first too long
    with pytest.raises(ValueError, match="LDS"):
        R.ResampleSpec(20025)          # 640 / 801: T = 26, 640 rows of 27 floats, the first 640-row table too large
    assert R.ResampleSpec(240000).phase_len == 301 and R.ResampleSpec(19975).phase_len == 25  # the last that fit
    with pytest.raises(ValueError):
        R.StreamResampler(1, 240000, hops_per_step=7)  # 7 hops of 2400 samples and 300 of history
    with pytest.raises(ValueError, match="100 Hz"):
        R.StreamResampler(2, 11025)
    with pytest.raises(ValueError):
        R.StreamResampler(2, 48000, hops_per_step=64)  # the window: 64 hops of 480 samples
    with pytest.raises(ValueError, match="all int16 or all float32"):
        R.resample_clips([np.zeros(10, np.int16), np.zeros(10, np.float32)], 48000)
    with pytest.raises(ValueError):
        R.resample_clips([np.zeros(10, np.float64)], 48000)
    with pytest.raises(ValueError):
        R.resample_clips([np.zeros(10, np.int16)], 48000, out_dtype=torch.float64)
    with pytest.raises(ValueError):
        R.resample_clips([np.zeros(10, np.int16)], [48000, 8000])
    with pytest.raises(ValueError):
        R.resample_clips([np.zeros(10, np.int16)], 16001)
