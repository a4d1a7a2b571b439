"""Every ratio class the resampling plan accepts, up to its LDS limits, on the
device (resample_kernel.hip; the rate matrix and its reasons are in
tests/resample_edge_plans.py, the plan sizes pinned by tests/test_resample_cpu.py).

The kernels are not specialised per rate: one index computation q -> jl, r
serves every (up, down, T), so the clip kernel is compared with the float64
model -- pinned to scipy at these very ratios on the CPU -- at every rate, and
the batch, stream, sessions and captured forms with the clip kernel, bit for
bit.  Stale LDS (1e30, NaN) in front of the plans at the span and table limits
must change nothing: a read one float past the staged span or table shows there.

Acceptance rule.  |device - model| <= gamma * sum_j |h_j| |x_j| per output,
gamma = T u / (1 - T u), u = 2^-24, for white int16 noise.  For EVERY rate below
that rule alone was needed: tests/test_resample_cpu.py
(test_the_bound_sees_an_off_by_one) shows that a model with jl one input sample
off, or the phase row r one off, leaves the bound on >= 93 % of the outputs (15
of 16 and 31 of 32 at worst, on short inputs at 16 / 1 and 32 / 1; >= 99.7 % at
every other rate) of every input used here, 16100 Hz (rows 1/160 of a sample apart) and 15975 Hz
(1/640) included; no rate needed the bit-for-bit float32 chain in numpy.

Worst measured |device - model| / bound over all lengths, per rate (MI355X; a
ratio against the derived bound, recorded for the reader, never a threshold):

    rate     up/down    T    err/bound      rate     up/down    T    err/bound
    96000    1/6       121   0.051          15975    640/639    21   0.254
    32000    1/2        41   0.090          19975    640/799    25   0.212
    22050    320/441    28   0.224          192000   1/12      241   0.021
    24000    2/3        31   0.129          240000   1/15      301   0.017
    12000    4/3        21   0.164          1000     16/1       21   0.200
    20000    4/5        26   0.163          500      32/1       21   0.220
    16100    160/161    21   0.220
"""
import ctypes
import os

import numpy as np
import pytest

import resample_edge_plans as E
import resample_sessions_reference as SR

pytestmark = pytest.mark.gpu

STREAM_RATES = [96000, 32000, 24000, 12000, 16100, 1000, 500, 240000]
SESSION_RATES = E.SESSION_RATES
SENT = -7777.25


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(t):
    import torch
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(scope="module")
def poison(torch_cuda):
    """fill(v): every CU's LDS holds v, as test_gpu_resample.py's test_stale_lds_changes_nothing does it."""
    torch = torch_cuda
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_host", "liblds_poison.so")
    if not os.path.exists(so):
        pytest.fail("tests/c_host/liblds_poison.so missing: run __graft_entry__.build()")
    helper = ctypes.CDLL(so)
    helper.lds_poison.argtypes = [ctypes.c_float, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    sink = torch.zeros(1, device="cuda")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count

    def fill(v):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert helper.lds_poison(v, ctypes.c_void_p(sink.data_ptr()), 4 * n_cu, st) == 0

    yield fill
    torch.cuda.synchronize()
    assert sink.item() == 0.0


# -- 3. the clip kernel against the float64 model ------------------------------
@pytest.mark.parametrize("rate", E.EDGE_RATES)
def test_against_the_model(torch_cuda, rate):
    torch = torch_cuda
    from vad_amd import _lib
    from vad_amd import resample as R
    tout = int(_lib.lib().vad_resample_tile_outputs())
    r = R.Resampler(rate)
    s = r.spec
    assert E.plan_sizes(s) == E.EDGE_PLANS[rate]
    h32 = E.taps32(s)
    worst_of_rate = 0.0
    for n in E.lengths(s, tout):
        x = E.clip_input(rate, n)
        want = R.resample_model(x, s, taps=h32)
        bound = E.chain_bound(x, s)
        a = r(torch.from_numpy(x).cuda())
        b = r(torch.from_numpy(x.astype(np.float32)).cuda())
        assert a.dtype == torch.float32 and a.shape == (s.n_out(n),) == want.shape
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))  # int16 input == fp32 input, bit for bit
        err = np.abs(a.cpu().numpy().astype(np.float64) - want)
        worst = float((err / np.maximum(bound, 1e-300)).max()) if n else 0.0
        worst_of_rate = max(worst_of_rate, worst)
        print(f"{rate} Hz n={n}: n_out={len(want)} max err {err.max() if n else 0:.3e}, max err/bound {worst:.3f}")
        assert (err <= bound).all()
    print(f"{rate} Hz ({s.up}/{s.down}, T = {s.phase_len}): worst err/bound {worst_of_rate:.3f}")


# -- 4. batch == single clips, mixed rates == per-rate calls -------------------
def seven_clips(torch, rate):
    """test_gpu_resample.py's: lengths 0 and 1, two clips that share a
    destination tile, every source at an odd int16 offset of its allocation,
    one clip longer than two tiles."""
    from vad_amd import resample as R
    s = R.ResampleSpec(rate)
    lens = [0, 1, 3 * s.down + 1, 700 * s.down // s.up, 2300 * s.down // s.up + 5, 0, 333]
    pool = torch.from_numpy(E.ints(sum(lens) + 16, rate + 7)).cuda()
    clips, o = [], 1
    for n in lens:
        clips.append(pool[o:o + n])
        o += n + n % 2
    assert all(c.data_ptr() % 4 == 2 for c in clips if c.numel())
    return clips


@pytest.mark.parametrize("rate", [240000, 19975, 16100, 500])
def test_batch_equals_single_clips(torch_cuda, rate):
    torch = torch_cuda
    from vad_amd import resample as R
    from vad_amd.config import MfccConfig
    r = R.Resampler(rate)
    clips = seven_clips(torch, rate)
    b = r.batch(clips, MfccConfig())
    t, total = R.plan_layout([c.numel() for c in clips], rate)
    assert b.total == total and all(np.array_equal(b.host[k], t[k]) for k in t)
    want = torch.zeros(total, dtype=torch.float32, device="cuda")
    for k, c in enumerate(clips):
        y = r(c.clone())  # an aligned copy of the clip, alone
        assert y.numel() == t["len"][k]
        want[int(t["start"][k]):int(t["start"][k]) + y.numel()] = y
    assert torch.equal(b.data.view(torch.int32), want.view(torch.int32))  # the clips, and zeros everywhere else
    # clips 1 and 2 share the first tile (at 640 / 799 clip 2 alone runs into the second); clip 4 spans three
    assert int(t["len"][1]) >= 1 and int(t["start"][1]) == 0 < int(t["start"][2]) < R.TILE_OUT
    assert int(t["len"][4]) > 2 * R.TILE_OUT
    hb = R.resample_clips([c.cpu().numpy() for c in clips], rate)
    assert torch.equal(hb.data.view(torch.int32), b.data.view(torch.int32))


def test_mixed_rates_equal_the_per_rate_calls(torch_cuda):
    torch = torch_cuda
    from vad_amd import resample as R
    rates = [240000, 19975, 500, 16100, 15975, 240000, 22050, 192000, 1000, 500, 22050]
    lens = [20000, 1500, 70, 1200, 0, 301, 2000, 13000, 1, 33, 1306]
    assert len(set(rates)) == 8 and set(rates) <= set(E.EDGE_RATES)
    clips = [torch.from_numpy(E.ints(n, 140 + i)).cuda() for i, n in enumerate(lens)]
    b = R.resample_clips(clips, rates)
    t, total = R.plan_layout(lens, rates)
    assert b.total == total and b.data.dtype == torch.float32
    want = torch.zeros(total, dtype=torch.float32, device="cuda")
    for rate in sorted(set(rates)):
        r = R.Resampler(rate)
        for k in [k for k, rr in enumerate(rates) if rr == rate]:
            y = r(clips[k])
            assert y.numel() == t["len"][k]
            want[int(t["start"][k]):int(t["start"][k]) + y.numel()] = y
    assert torch.equal(b.data.view(torch.int32), want.view(torch.int32))
    assert (b.data != 0).any()


# -- 5. streams == the clip delayed by `delay` ---------------------------------
def stream_audio(S, hops, hop_in, seed, dtype):
    return np.random.default_rng(seed).integers(-20000, 20000, (hops, S, hop_in)).astype(dtype)


@pytest.mark.parametrize("rate", STREAM_RATES)
@pytest.mark.parametrize("K,S", [(1, 1), (1, 5), (6, 3)])
def test_stream_equals_the_clip_delayed(torch_cuda, rate, K, S):
    """The blocks of a stream are the clip conversion of its whole input
    behind `delay` zeros, bit for bit; the emitted count is carried from
    launch to launch until the delay has passed, also where that takes whole
    blocks of zeros (1000 Hz: one hop, 500 Hz: two)."""
    torch = torch_cuda
    from vad_amd import resample as R
    spec = R.ResampleSpec(rate)
    d, hop_in, Hn = spec.delay, rate // 100, spec.history
    assert (d, Hn) == E.EDGE_PLANS[rate][5:]
    if K * hop_in + Hn > R.MAX_SPAN:
        with pytest.raises(ValueError, match="window"):
            R.StreamResampler(S, rate, hops_per_step=K, input_dtype=torch.int16)
        return
    hops = 14  # blocks of K = 6: 6, 6 and a last one of 2
    sr = R.StreamResampler(S, rate, hops_per_step=K, input_dtype=torch.int16)
    assert sr.delay == d and sr.hop_in == hop_in and sr.state.numel() == S * (Hn + 1)
    x = stream_audio(S, hops, hop_in, rate + K + S, np.int16)
    dx = torch.from_numpy(x).cuda()
    blocks = []
    for t in range(0, hops, K):
        blocks.append(sr.step_block(dx[t:t + K]).clone())
        done = min(t + K, hops) * 160
        assert sr.state[S * Hn:].tolist() == [min(done, d)] * S, t  # emitted, after every block
    z = torch.cat(blocks)
    tail = sr.flush()
    assert z.shape == (hops, S, 160) and tail.shape == (S, d)
    r = R.Resampler(rate)
    for s in range(S):
        whole = r(torch.from_numpy(np.ascontiguousarray(x[:, s].reshape(-1))).cuda())
        assert whole.numel() == hops * 160
        got = torch.cat([z[:, s].reshape(-1), tail[s]])
        assert (got[:d] == 0).all()
        assert torch.equal(got[d:].view(torch.int32), whole.view(torch.int32))
        if K == 1 and d % 160 == 0:  # 1000 and 500 Hz: whole blocks of zeros first
            first = d // 160
            assert first in (1, 2) and all(int(blocks[i][0, s].abs().sum().item()) == 0 for i in range(first))
            assert torch.equal(blocks[first][0, s].view(torch.int32), whole[:160].view(torch.int32))
            assert (blocks[first][0, s] != 0).any()
    assert (rate in (1000, 500)) == (d % 160 == 0)


def test_the_stream_window_ends_at_the_limit(torch_cuda):
    """240 kHz: six hops of 2400 samples behind 300 of history are 14,700 of
    16,384 floats and run; seven are refused."""
    torch = torch_cuda
    from vad_amd import resample as R
    sr = R.StreamResampler(2, 240000, hops_per_step=6)
    assert 6 * sr.hop_in + sr.spec.history == 14700
    with pytest.raises(ValueError, match="window"):
        R.StreamResampler(2, 240000, hops_per_step=7)
    with pytest.raises(ValueError, match="window"):
        R.SessionStreamResampler(2, [48000, 240000], hops_per_step=7)


def test_captured_stream_with_a_delay_of_two_hops(torch_cuda):
    """500 Hz, K = 1, captured while fresh: the replays carry `emitted`
    through two blocks of zeros exactly as direct steps do."""
    torch = torch_cuda
    from vad_amd import resample as R
    S, blocks = 3, 6
    x = torch.from_numpy(stream_audio(S, blocks, 5, 78, np.float32)).cuda()
    direct = R.StreamResampler(S, 500)
    want, counts = [], []
    for b in range(blocks):
        want.append(direct.step_block(x[b:b + 1]).clone())
        counts.append(direct.state[S * 20:].tolist())
    assert counts == [[min(160 * (b + 1), 320)] * S for b in range(blocks)]
    cap = R.StreamResampler(S, 500)
    cap.capture()
    assert int(cap.state.abs().sum().item()) == 0  # the warm-up launch left no trace
    got = []
    for b in range(blocks):
        cap.inputs.copy_(x[b:b + 1])
        got.append(cap.step_block().clone())
        assert cap.state[S * 20:].tolist() == counts[b], b
    want, got = torch.cat(want), torch.cat(got)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(cap.state, direct.state)
    assert int(want[:2].abs().sum().item()) == 0 and (want[2] != 0).any()


# -- 6. sessions across extreme plans ------------------------------------------
SESS_S, SESS_K, SESS_BLOCKS = 8, 3, 8
HOP_MAX = max(SR.hop_in_of(r) for r in SESSION_RATES)


@pytest.fixture(scope="module")
def sessions_workload():
    counts, restart, rate = E.sessions_script()
    assert counts.shape == (SESS_BLOCKS, SESS_S)
    return (counts, restart, rate, SR.audio(SESS_BLOCKS, SESS_K, SESS_S, HOP_MAX, seed=979),
            SR.session_rows(counts, restart, rate, len(SESSION_RATES), SESS_K))


_PLAIN = {}


def plain_rows(torch, rate, hops):
    """The rows a freshly reset one-stream, K = 1 StreamResampler writes for these hops, (n, 160)."""
    from vad_amd import resample as V
    if rate not in _PLAIN:
        _PLAIN[rate] = V.StreamResampler(1, rate, input_dtype=torch.int16)
    p = _PLAIN[rate]
    p.reset()
    rows = [p.step_block(h.reshape(1, 1, -1)).clone()[0, 0] for h in hops]
    return torch.stack(rows) if rows else p.out.new_zeros((0, p.hop_out))


def make_sessions(torch):
    from vad_amd import resample as V
    rs = V.SessionStreamResampler(SESS_S, SESSION_RATES, hops_per_step=SESS_K, input_dtype=torch.int16)
    assert [s.history for s in rs.specs] == [300, 20, 20, 120, 20, 60, 20, 40] and rs.hop_in == 2400
    assert rs.delays == [10, 320, 10, 10, 160, 10, 20, 10]
    return rs


def test_sessions_across_extreme_plans(torch_cuda, sessions_workload):
    """Every session against a plain resampler of its rate fed its hops, bit
    for bit; after every block, per stream: the emitted count of its session,
    zeros in the history beyond the session's own Hn, every byte of a stalled
    stream's state, the sentinel in the rows past its count."""
    torch = torch_cuda
    counts, restart, rate, audio, sessions = sessions_workload
    x = cuda(audio)
    rs = make_sessions(torch)
    hn = [s.history for s in rs.specs]
    n = np.clip(counts, 0, SESS_K)
    outs = []
    cur = [None] * SESS_S   # the rate index and the hops of every stream's running session
    taken = [0] * SESS_S
    tails_cleared = 0
    for b in range(SESS_BLOCKS):
        before = rs.history.clone(), rs.emitted.clone(), rs.stream_rate.clone()
        rs.out.fill_(SENT)
        rs.step_block(x[b], hop_counts=cuda(counts[b]), restart=cuda(restart[b]), rate=cuda(rate[b]))
        assert int(rs.restart.sum().item()) == 0, b  # every flag consumed
        outs.append(rs.out.clone())
        hist, emitted, running = rs.history.cpu(), rs.emitted.tolist(), rs.stream_rate.tolist()
        for s in range(SESS_S):
            if restart[b, s]:
                cur[s], taken[s] = int(np.clip(rate[b, s], 0, len(SESSION_RATES) - 1)), 0
                if hn[cur[s]] < hn[before[2][s].item()] and (before[0][s, hn[cur[s]]:] != 0).any():
                    tails_cleared += 1  # a longer history left samples where the shorter one has none
            elif n[b, s] == 0:  # stalled: every byte as it was
                assert torch.equal(bits(rs.history[s]), bits(before[0][s])), (b, s)
                assert emitted[s] == before[1][s].item() and running[s] == before[2][s].item(), (b, s)
            taken[s] += int(n[b, s])
            assert running[s] == cur[s], (b, s)
            assert emitted[s] == min(taken[s] * 160, rs.delays[cur[s]]), (b, s)
            assert int(hist[s, hn[cur[s]]:].abs().sum().item()) == 0, (b, s)
            assert (rs.out[n[b, s]:, s] == SENT).all(), (b, s)
    assert tails_cleared >= 3
    outs = torch.stack(outs)  # (B, K, S, 160)
    checked = 0
    for s in range(SESS_S):
        for sess in sessions[s][1:]:  # every stream restarts in block 0: the session before it is empty
            r = SESSION_RATES[sess["rate"]]
            hops = [x[b, k, s, :SR.hop_in_of(r)] for b, k in sess["rows"]]
            got = torch.stack([outs[b, k, s] for b, k in sess["rows"]]) if hops else outs.new_zeros((0, 160))
            assert torch.equal(bits(got), bits(plain_rows(torch, r, hops))), (s, sess["start"], r)
            checked += len(hops)
        assert not sessions[s][0]["rows"]
    assert checked == int(n.sum()) > 0


def test_a_long_delay_session_restarted_mid_delay(torch_cuda, sessions_workload):
    """Stream 1 of the script: 500 Hz (delay 320) takes one hop, is restarted
    with no hop, takes one hop, stalls, and only then passes its delay."""
    torch = torch_cuda
    counts, restart, rate, audio, _ = sessions_workload
    assert rate[:2, 1].tolist() == [1, 1] and restart[:5, 1].tolist() == [1, 1, 0, 0, 0]
    assert counts[:5, 1].tolist() == [1, 0, 1, 0, 3]
    x = cuda(audio)
    rs = make_sessions(torch)
    seen = []
    for b in range(5):
        rs.out.fill_(SENT)
        rs.step_block(x[b], hop_counts=cuda(counts[b]), restart=cuda(restart[b]), rate=cuda(rate[b]))
        seen.append((rs.emitted[1].item(), rs.out[:, 1].clone(), rs.history[1].clone()))
    assert [e for e, _, _ in seen] == [160, 0, 160, 160, 320]
    assert (seen[0][2][:20] != 0).any() and int(seen[1][2].abs().sum().item()) == 0  # the restart cleared the history
    assert int(seen[0][1][0].abs().sum().item()) == 0 and int(seen[2][1][0].abs().sum().item()) == 0  # inside the delay
    assert (seen[1][1] == SENT).all() and (seen[3][1] == SENT).all()
    want = plain_rows(torch, 500, [x[2, 0, 1, :5]] + [x[4, k, 1, :5] for k in range(3)])
    assert torch.equal(bits(seen[4][1]), bits(want[1:])) and (want[2] != 0).any()


# -- 7. stale LDS at the limits ------------------------------------------------
@pytest.mark.parametrize("rate", [240000, 19975])
def test_stale_lds_at_the_span_and_table_limits(torch_cuda, poison, rate):
    """Two full tiles at the plan whose input tile (240 kHz: 15,646 floats) or
    phase table (19,975 Hz: 16,000 floats) all but fills its LDS region."""
    torch = torch_cuda
    from vad_amd import resample as R
    r = R.Resampler(rate)
    s = r.spec
    n = 2 * R.TILE_OUT * s.down // s.up
    assert s.n_out(n) == 2 * R.TILE_OUT
    x = torch.from_numpy(E.ints(n, rate)).cuda()
    want = r(x).clone()
    h32 = E.taps32(s)
    err = np.abs(want.cpu().numpy().astype(np.float64) - R.resample_model(x.cpu().numpy(), s, taps=h32))
    assert (err <= E.chain_bound(x.cpu().numpy(), s)).all()
    for v in (1e30, -1e30, float("nan")):
        poison(v)
        assert torch.equal(r(x).view(torch.int32), want.view(torch.int32)), v


def test_stale_lds_in_front_of_sessions_blocks(torch_cuda, poison, sessions_workload):
    torch = torch_cuda
    counts, restart, rate, audio, _ = sessions_workload
    x = cuda(audio)

    def run(v=None):
        rs = make_sessions(torch)
        got = []
        for b in range(3):
            rs.out.fill_(SENT)
            if v is not None:
                poison(v)
            rs.step_block(x[b], hop_counts=cuda(counts[b]), restart=cuda(restart[b]), rate=cuda(rate[b]))
            got.append(rs.out.clone())
        return torch.stack(got), rs.state.clone()

    want, want_state = run()
    assert (want != SENT).any() and not torch.isnan(want).any()
    for v in (1e30, -1e30, float("nan")):
        got, got_state = run(v)
        assert torch.equal(bits(got), bits(want)) and torch.equal(got_state, want_state), v
