"""Resampling on the device (vad_amd/resample.py, resample_kernel.hip)
against the float64 model run on float32(taps), element by element inside the
fma-chain bound, and the bit-for-bit equalities the one shared dot product
gives: int16 == fp32 input, batch == single clips, mixed rates == per rate,
16 kHz is a copy, int16 output == rint + saturate, streams == clips delayed by
d, graph replay == direct steps, stale LDS changes nothing; then the opt-in
``rate`` / ``resample`` arguments of the pipeline and the dataset export."""
import ctypes
import io
import os
import wave

import numpy as np
import pytest

from oracle import vad_oracle as O

pytestmark = pytest.mark.gpu

RATES = [48000, 8000, 44100, 11025, 16000]
U = 2.0 ** -24


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def ints(n, seed, lo=-32768, hi=32768):
    return np.random.default_rng(seed).integers(lo, hi, n).astype(np.int16)


def lengths(spec, tout):
    """0, 1, T-1 and the input lengths whose n_out is Tout-1, Tout, Tout+1,
    2 Tout+1 (the next reachable n_out where up > down skips one)."""
    ns = [0, 1, spec.phase_len - 1]
    for target in (tout - 1, tout, tout + 1, 2 * tout + 1):
        n = target * spec.down // spec.up
        n += spec.n_out(n) < target
        assert target <= spec.n_out(n) <= target + (spec.up > spec.down)
        ns.append(n)
    return ns


@pytest.mark.parametrize("rate", RATES)
def test_against_the_model(torch_cuda, rate):
    """|device - model| <= gamma * sum_j |h_j| |x_j| for every output, gamma =
    T u / (1 - T u), u = 2^-24: the bound of a T-term fp32 fma chain in any
    order, against the exact sum of the same float32 taps."""
    torch = torch_cuda
    from vad_amd import _lib
    from vad_amd import resample as R
    tout = int(_lib.lib().vad_resample_tile_outputs())
    r = R.Resampler(rate)
    s = r.spec
    h32 = s.taps.astype(np.float32).astype(np.float64)
    gamma = s.phase_len * U / (1 - s.phase_len * U)
    for n in lengths(s, tout):
        x = ints(n, rate + n)
        want = R.resample_model(x, s, taps=h32)
        bound = gamma * R.resample_model(np.abs(x.astype(np.float64)), s, taps=np.abs(h32))
        a = r(torch.from_numpy(x).cuda())
        b = r(torch.from_numpy(x.astype(np.float32)).cuda())
        assert a.dtype == torch.float32 and a.shape == (s.n_out(n),) == want.shape
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))  # int16 input == fp32 input, bit for bit
        err = np.abs(a.cpu().numpy().astype(np.float64) - want)
        worst = float((err / np.maximum(bound, 1e-300)).max()) if n else 0.0
        print(f"{rate} Hz n={n}: n_out={len(want)} max err {err.max() if n else 0:.3e}, max err/bound {worst:.3f}")
        assert (err <= bound).all()


def test_16k_is_a_copy(torch_cuda):
    torch = torch_cuda
    from vad_amd import resample as R
    r = R.Resampler(16000)
    x = np.random.default_rng(5).standard_normal(3001).astype(np.float32)
    x[:6] = [0.0, -0.0, np.inf, -np.inf, 1e-45, -3e38]
    got = r(torch.from_numpy(x).cuda())
    assert np.array_equal(got.cpu().numpy().view(np.int32), x.view(np.int32))
    i = ints(3001, 6)
    assert np.array_equal(r(torch.from_numpy(i).cuda(), out_dtype=torch.int16).cpu().numpy(), i)
    assert np.array_equal(r(torch.from_numpy(i).cuda()).cpu().numpy(), i.astype(np.float32))


@pytest.mark.parametrize("rate", [48000, 44100, 8000])
def test_int16_output_is_rint_and_saturate(torch_cuda, rate):
    torch = torch_cuda
    from vad_amd import resample as R
    r = R.Resampler(rate)
    n = 4000
    x = ints(n, rate).astype(np.float32)
    x[1000:1400] = 32767.0 * 4     # passes +32767
    x[2000:2400] = -32768.0 * 4    # passes -32768
    x[3000] = np.nan
    d = torch.from_numpy(x).cuda()
    f = r(d).cpu().numpy()
    got = r(d, out_dtype=torch.int16).cpu().numpy()
    want = np.where(np.isnan(f), 0.0, np.clip(np.rint(f), -32768, 32767)).astype(np.int16)
    assert (f > 40000).any() and (f < -40000).any() and np.isnan(f).any()
    assert (want == 32767).any() and (want == -32768).any()
    assert np.array_equal(got, want)
    xi = ints(n, rate + 1)
    assert np.array_equal(r(torch.from_numpy(xi).cuda(), out_dtype=torch.int16).cpu().numpy(),
                          np.clip(np.rint(r(torch.from_numpy(xi).cuda()).cpu().numpy()), -32768, 32767)
                          .astype(np.int16))


def seven_clips(torch, rate, dtype=np.int16):
    """Lengths 0 and 1, two clips that share a destination tile, one source at
    an odd int16 offset of its allocation, one longer than two tiles."""
    from vad_amd import resample as R
    s = R.ResampleSpec(rate)
    lens = [0, 1, 3 * s.down + 1, 700 * s.down // s.up, 2300 * s.down // s.up + 5, 0, 333]
    pool = torch.from_numpy(ints(sum(lens) + 16, rate + 7).astype(dtype)).cuda()
    clips, o = [], 1  # every clip starts at an odd sample of the pool
    for n in lens:
        clips.append(pool[o:o + n])
        o += n + n % 2
    assert all(c.data_ptr() % 4 == 2 for c in clips if dtype == np.int16 and c.numel())
    return clips


@pytest.mark.parametrize("rate", [48000, 44100, 8000])
def test_batch_equals_single_clips(torch_cuda, rate):
    torch = torch_cuda
    from vad_amd import resample as R
    from vad_amd.config import MfccConfig
    r = R.Resampler(rate)
    clips = seven_clips(torch, rate)
    b = r.batch(clips, MfccConfig())
    t, total = R.plan_layout([c.numel() for c in clips], rate)
    assert b.total == total and all(np.array_equal(b.host[k], t[k]) for k in t)
    assert torch.equal(b.tables.cpu(), torch.from_numpy(np.stack([t[k] for k in
                                                                  ("start", "len", "frame0", "n_frames", "n_rows",
                                                                   "row0")])))
    want = torch.zeros(total, dtype=torch.float32, device="cuda")
    for k, c in enumerate(clips):
        y = r(c.clone())  # an aligned copy of the clip, alone
        assert y.numel() == t["len"][k]
        want[int(t["start"][k]):int(t["start"][k]) + y.numel()] = y
    assert torch.equal(b.data.view(torch.int32), want.view(torch.int32))  # the clips, and zeros everywhere else
    assert 0 < int(t["start"][2]) < int(t["start"][3]) < R.TILE_OUT       # clips that share a tile
    # host arrays through the pinned staging copy give the same buffer
    hb = R.resample_clips([c.cpu().numpy() for c in clips], rate)
    assert torch.equal(hb.data.view(torch.int32), b.data.view(torch.int32))


def test_mixed_rates_equal_the_per_rate_calls(torch_cuda):
    torch = torch_cuda
    from vad_amd import resample as R
    rates = [48000, 8000, 48000, 16000, 44100, 8000, 44100, 11025]
    lens = [5000, 900, 0, 1234, 4411, 1, 3000, 2000]
    clips = [torch.from_numpy(ints(n, 40 + i)).cuda() for i, n in enumerate(lens)]
    b = R.resample_clips(clips, rates, out_dtype=torch.int16)
    t, total = R.plan_layout(lens, rates)
    assert b.total == total and b.data.dtype == torch.int16
    want = torch.zeros(total, dtype=torch.int16, device="cuda")
    for rate in sorted(set(rates)):
        r = R.Resampler(rate)
        for k in [k for k, rr in enumerate(rates) if rr == rate]:
            y = r(clips[k], out_dtype=torch.int16)
            want[int(t["start"][k]):int(t["start"][k]) + y.numel()] = y
    assert torch.equal(b.data, want)


def test_tables_that_overrun_total_are_cut(torch_cuda):
    """The tables are device memory and their content the caller's contract;
    whatever they hold, nothing is written outside dst[0 .. total)."""
    torch = torch_cuda
    from vad_amd import _lib
    from vad_amd import resample as R
    r = R.Resampler(48000)
    x = torch.from_numpy(ints(9000, 3)).cuda()
    tab = torch.tensor([[x.data_ptr(), x.data_ptr()], [9000, 9000], [0, 1600]], dtype=torch.int64, device="cuda")
    buf = torch.full((4096,), 7.0, device="cuda")
    total = 2000  # the first clip alone has 3000 outputs, the second would end at 4600
    assert _lib.lib().vad_resample_batch_i16_f32(r.plan.handle, _lib.ptr(tab[0]), _lib.ptr(tab[1]), _lib.ptr(tab[2]),
                                                 2, _lib.ptr(buf), total, _lib.stream_ptr()) == 0
    y = r(x)
    assert torch.equal(buf[:1600], y[:1600]) and torch.equal(buf[1600:total], y[:400])
    assert (buf[total:] == 7.0).all()


def stream_audio(S, hops, hop_in, seed, dtype):
    return np.random.default_rng(seed).integers(-20000, 20000, (hops, S, hop_in)).astype(dtype)


@pytest.mark.parametrize("rate", [48000, 8000, 44100])
@pytest.mark.parametrize("K,S", [(1, 1), (1, 5), (8, 1), (8, 5)])
def test_stream_equals_the_clip_delayed(torch_cuda, rate, K, S):
    torch = torch_cuda
    from vad_amd import resample as R
    hops = 12
    sr = R.StreamResampler(S, rate, hops_per_step=K, input_dtype=torch.int16)
    d = sr.delay
    x = stream_audio(S, hops, sr.hop_in, rate + K + S, np.int16)
    dx = torch.from_numpy(x).cuda()
    z = torch.cat([sr.step_block(dx[t:t + K]).clone() for t in range(0, hops, K)])  # the last block of K = 8 is 4 hops
    tail = sr.flush()
    assert z.shape == (hops, S, 160) and tail.shape == (S, d)
    r = R.Resampler(rate)
    for s in range(S):
        whole = r(torch.from_numpy(np.ascontiguousarray(x[:, s].reshape(-1))).cuda())
        assert whole.numel() == hops * 160
        got = torch.cat([z[:, s].reshape(-1), tail[s]])
        assert (got[:d] == 0).all()
        assert torch.equal(got[d:].view(torch.int32), whole.view(torch.int32))
    # stream-major input read in place, fp32 samples, int16 out: the same stream
    sr2 = R.StreamResampler(S, rate, hops_per_step=K, input_dtype=torch.float32, out_dtype=torch.int16)
    per_stream = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2)).astype(np.float32)).cuda()  # (S, hops, hop_in)
    z2 = torch.cat([sr2.step_block(per_stream[:, t:t + K].transpose(0, 1)).clone() for t in range(0, hops, K)])
    f = z.cpu().numpy()
    assert np.array_equal(z2.cpu().numpy(), np.clip(np.rint(f), -32768, 32767).astype(np.int16))


def test_captured_stream_equals_direct_steps(torch_cuda):
    torch = torch_cuda
    from vad_amd import resample as R
    S, K, blocks = 3, 4, 3
    x = torch.from_numpy(stream_audio(S, K * blocks, 441, 77, np.float32)).cuda()
    direct = R.StreamResampler(S, 44100, hops_per_step=K)
    want = torch.cat([direct.step_block(x[b * K:(b + 1) * K]).clone() for b in range(blocks)])
    cap = R.StreamResampler(S, 44100, hops_per_step=K)
    cap.step_block(x[:K])  # state before the capture is kept by it
    cap.capture()
    got = [cap.out.clone()]
    for b in range(1, blocks):
        cap.inputs.copy_(x[b * K:(b + 1) * K])
        got.append(cap.step_block().clone())
    assert torch.equal(torch.cat(got).view(torch.int32), want.view(torch.int32))
    assert torch.equal(cap.state, direct.state)
    cap.reset()
    assert torch.equal(cap.step_block(x[:K]).view(torch.int32), want[:K].view(torch.int32))


def test_stale_lds_changes_nothing(torch_cuda):
    torch = torch_cuda
    from vad_amd import resample as R
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

    clips = seven_clips(torch, 44100)
    r = R.Resampler(44100)
    xs = torch.from_numpy(stream_audio(4, 8, 441, 9, np.int16)).cuda()

    def stream_run():
        sr = R.StreamResampler(4, 44100, hops_per_step=4, input_dtype=torch.int16)
        return torch.cat([sr.step_block(xs[:4]).clone(), sr.step_block(xs[4:]).clone()]), sr.state.clone()

    want_b = r.batch(clips).data.clone()
    want_s, want_state = stream_run()
    for v in (1e30, -1e30, float("nan")):
        fill(v)
        assert torch.equal(r.batch(clips).data.view(torch.int32), want_b.view(torch.int32)), v
        fill(v)
        got_s, got_state = stream_run()
        assert torch.equal(got_s.view(torch.int32), want_s.view(torch.int32)) and torch.equal(got_state, want_state), v
    torch.cuda.synchronize()
    assert sink.item() == 0.0


# -- end to end --------------------------------------------------------------
@pytest.fixture(scope="module")
def clf(golden):
    from vad_amd.ffn import FFNClassifier
    w = golden("ffn")
    return FFNClassifier([(w[f"ref39_W{i}"], w[f"ref39_b{i}"]) for i in range(4)])


def test_pipeline_takes_a_rate(torch_cuda, clf):
    torch = torch_cuda
    from vad_amd import resample as R
    from vad_amd.pipeline import VadPipeline
    pipe = VadPipeline(clf)
    x = torch.from_numpy(O.synth_clip(3 * 48000, seed=61)[:3 * 48000].astype(np.int16)).cuda()
    y = R.Resampler(48000)(x)
    assert y.numel() == 48000
    want = pipe.labels(y)
    assert want.numel() == 293
    assert torch.equal(pipe.labels(x, rate=48000), want)
    assert torch.equal(pipe.labels(y, rate=16000), want) and torch.equal(pipe.labels(y, rate=None), want)
    assert not torch.equal(pipe.labels(x)[:293], want)  # unset: the samples as they are, as before
    seg = pipe.segments(x, rate=48000)
    ref = pipe.segments(y)
    assert np.array_equal(seg.numpy(), ref.numpy()) and torch.equal(seg.counts, ref.counts)
    assert torch.equal(pipe.voiced(x, rate=48000), pipe.voiced(y))
    # _batch forms: clips at their own rates against the single-clip calls
    x8 = torch.from_numpy(O.synth_clip(12000, seed=62)[:12000].astype(np.int16)).cuda()
    lab = pipe.labels_batch([x, x8], rate=[48000, 8000])
    assert torch.equal(lab[0], want) and torch.equal(lab[1], pipe.labels(x8, rate=8000))
    v, offs = pipe.voiced_batch([x, x8], rate=[48000, 8000])
    assert torch.equal(v[offs[0]:offs[1]], pipe.voiced(y))
    sb = pipe.segments_batch([x, x8], rate=[48000, 8000])
    assert sb is not None


def test_stream_resampler_feeds_the_stream_batch(torch_cuda, clf):
    torch = torch_cuda
    from vad_amd import resample as R
    from vad_amd.stream import StreamBatch
    S, K, hops = 4, 8, 40
    x = np.stack([O.synth_clip(hops * 480, seed=70 + s)[:hops * 480] for s in range(S)]).astype(np.int16)  # (S, n)
    blocks = torch.from_numpy(np.ascontiguousarray(x.reshape(S, hops, 480).transpose(1, 0, 2))).cuda()
    sb = StreamBatch(S, clf, hops_per_step=K)
    sr = R.StreamResampler(S, 48000, hops_per_step=K, input_dtype=torch.int16, out=sb.inputs)
    got = []
    for t in range(0, hops, K):
        sr.step_block(blocks[t:t + K])
        got.append(sb.step_block().clone())  # the hop kernel reads the resampler's output in place
    # the reference: the clip conversion of each stream, delayed by d, fed as 16 kHz hops
    r = R.Resampler(48000)
    d = sr.delay
    y = torch.stack([torch.cat([torch.zeros(d, device="cuda"), r(torch.from_numpy(x[s]).cuda())])[:hops * 160]
                     for s in range(S)])
    ref = StreamBatch(S, clf, hops_per_step=K)
    want = [ref.step_block(y.view(S, hops, 160)[:, t:t + K].transpose(0, 1).contiguous()).clone()
            for t in range(0, hops, K)]
    assert torch.equal(torch.cat(got), torch.cat(want))
    assert (torch.cat(got) != 255).any()


def write_wav(path, samples, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(samples, "<i2").tobytes())


def test_process_files_resamples_on_request(torch_cuda, tmp_path):
    torch = torch_cuda
    from scipy.io import wavfile
    from vad_amd import dataset as D
    from vad_amd import resample as R
    raw = [O.synth_clip(n, seed=80 + i)[:n].astype(np.int16) for i, n in enumerate((4000, 2500))]
    src, pre = tmp_path / "src", tmp_path / "pre"
    src.mkdir(), pre.mkdir()
    r = R.Resampler(8000)
    for i, x in enumerate(raw):
        write_wav(src / f"f{i}.wav", x, 8000)
        wavfile.write(str(pre / f"f{i}.wav"), 16000, r(torch.from_numpy(x).cuda()).cpu().numpy())  # float32 wav
    paths = D.list_audio_files([str(src)])
    pre_paths = D.list_audio_files([str(pre)])
    fb = O.get_mel_filterbanks(300, 8000, 512, 26, 16000)

    def text_of(per_file_rows, label):
        rows = torch.from_numpy(np.concatenate(per_file_rows).astype(np.float32)).cuda()
        D.scale_rows_device(rows)
        return D.format_csv_rows(rows.cpu().numpy(), label)

    want_rows = [np.array([np.concatenate(t) for t in D.process_file([p, 400, 160, 512, fb, 13])]).reshape(-1, 39)
                 for p in pre_paths]
    assert [len(w) for w in want_rows] == [43, 24]
    out = io.StringIO()
    assert D.process_files([str(src)], 1, 10, out, resample=True) == [43, 24]
    assert out.getvalue() == text_of(want_rows, 1)
    # process_file resamples the same way
    for p, w in zip(paths, want_rows):
        got = D.process_file([p, 400, 160, 512, fb, 13], resample=True)
        assert np.array_equal(np.array([np.concatenate(t) for t in got]).reshape(-1, 39), w)
    # unset: the text of the unchanged path, which takes the samples as 16 kHz audio
    plain, default = io.StringIO(), io.StringIO()
    counts = D.process_files([str(src)], 1, 10, plain, resample=False)
    assert D.process_files([str(src)], 1, 10, default) == counts == [18, 9]
    same_rows = [np.array([np.concatenate(t) for t in D.process_file([p, 400, 160, 512, fb, 13])]).reshape(-1, 39)
                 for p in paths]
    assert plain.getvalue() == default.getvalue() == text_of(same_rows, 1) != out.getvalue()
