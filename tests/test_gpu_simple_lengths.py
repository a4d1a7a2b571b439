"""The SimpleAnalyser feature kernels at every transform length, rate and grid
shape they accept (tests/simple_length_cases.py has the table, the float64
reference and the generators; tests/test_simple_lengths_cpu.py measures that
reference against a long-double DFT).

a. every table case through SimpleAnalyser.frame_features against the
   reference: energy and crossing count equal, spectral columns rtol 1e-11;
b. shapes only vad_simple_features itself takes: even L that is no power of
   two, pad 0 and pad larger than the frame, other band counts and widths,
   strided and repeated frames;
c. structured frames (zero, impulses, DC, alternating, tones at the band
   edges, signed zeros and sign changes at the seams of the x[i + 1] read);
d. the grid-stride loops of both kernels;
e. stale LDS at the lengths with other LDS layouts;
f. the stream block kernel at other lengths, rates, noise_buf_len and int16;
g. the two-launch stream path at L = 257, 8192 and 8193, and its per-block
   launch loop for a non-contiguous block.

Every test prints the largest relative error of the spectral columns it saw.
"""
import ctypes

import numpy as np
import pytest

import simple_length_cases as C
import simple_stream_reference as R
import simple_stream_sessions_reference as RS
from test_gpu_lds_independence import bits, check, poison, same  # noqa: F401  (poison: a fixture)

pytestmark = pytest.mark.gpu

INIT, NO_HOP = 253, 254


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _report(L, err, what=""):
    print(f"relerr [{C.path_of(L)}] L {L} {what}: {err:.3e}")


def _raw(torch, buf, n, frame_len, stride, L, pad, bb, n_bands):
    """vad_simple_features on a device float32 buffer; rows start as NaN."""
    from vad_amd import _lib
    out = torch.full((n, 3 + n_bands), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().vad_simple_features(_lib.ptr(buf), n, frame_len, stride, L, pad, bb, n_bands,
                                              _lib.ptr(out), _lib.stream_ptr()), "vad_simple_features")
    return out.cpu().numpy()


# ---------------------------------------------------------------------------
# a. every case through the class
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rate,fs", C.CASES)
def test_features_at_every_length(torch_cuda, rate, fs):
    from vad_amd.simple_analyser import SimpleAnalyser
    L, pad, bb = C.geometry(rate, fs)
    n = 3 if L >= 8192 else 5               # no multiple of the 4 or 2 waves of a block
    frames = C.noise_frames(n, fs, 1000 + fs)
    sa = SimpleAnalyser(rate, fs, 3)
    assert (sa._fft_len(), sa.fft_extended_zeros, sa.fftn_for_band) == (L, pad, bb)
    got = sa.frame_features(frames)
    err = C.assert_features(got, C.ref_rows(frames, L, pad, bb), (rate, fs))
    _report(L, err, f"rate {rate} frame {fs}")


# ---------------------------------------------------------------------------
# b. shapes the class cannot make
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("frame_len,pad,bb,n_bands", [
    (400, 100, 37, 4),    # L 600: even, no power of two -> the direct kernel
    (2, 300, 37, 4),      # L 602: two samples in 600 zeros, 254 threads without a sample
    (1000, 0, 62, 4),     # L 1000, pad 0
    (400, 56, 32, 0),     # L 512: no bands, rows of three
    (400, 56, 32, 1),
    (400, 56, 73, 7),     # 7 * 73 = 511 bins of 512
    (400, 56, 37, 4),     # bands that start at 37, 74, 111: no multiple of the lane count
    (401, 56, 37, 4),     # the same in the direct kernel (L 513)
    (401, 56, 73, 7),
])
def test_raw_entry_shapes(torch_cuda, frame_len, pad, bb, n_bands):
    torch = torch_cuda
    L = frame_len + 2 * pad
    frames = C.noise_frames(5, frame_len, 2000 + L + n_bands)
    got = _raw(torch, torch.from_numpy(frames).cuda(), 5, frame_len, frame_len, L, pad, bb, n_bands)
    ref = C.ref_rows(frames, L, pad, bb, n_bands)
    assert got.shape == (5, 3 + n_bands)
    err = C.assert_features(got, ref, (frame_len, pad, bb, n_bands))
    _report(L, err, f"raw frame {frame_len} pad {pad} bands {n_bands} x {bb}")


@pytest.mark.parametrize("fs", [400, 401, 8191])
def test_frame_stride(torch_cuda, fs):
    """frame_stride = frame_len + 13 with NaN in the gaps gives the contiguous
    run's bits; frame_stride = 0 gives the same row n times."""
    torch = torch_cuda
    L, pad, bb = C.geometry(16000, fs)
    n = 5 if fs < 8000 else 3
    frames = C.noise_frames(n, fs, 3000 + fs)
    dense = torch.from_numpy(frames).cuda()
    want = _raw(torch, dense, n, fs, fs, L, pad, bb, 4)
    C.assert_features(want, C.ref_rows(frames, L, pad, bb), fs)
    wide = torch.full((n, fs + 13), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :fs] = dense
    got = _raw(torch, wide, n, fs, fs + 13, L, pad, bb, 4)
    assert np.isfinite(got).all() and got.tobytes() == want.tobytes()
    rep = _raw(torch, dense[1], 3, fs, 0, L, pad, bb, 4)
    assert rep.tobytes() == np.stack([want[1]] * 3).tobytes()


# ---------------------------------------------------------------------------
# c. structured frames
# ---------------------------------------------------------------------------
def _row(got, ref, zero=(), atol_band=0.0, atol_std=0.0, exact_energy=True, what=""):
    """One row against the reference: columns 0, 1 equal, the others rtol
    1e-11 -- but a column that is zero up to roundoff (zero) within atol of 0."""
    assert np.isfinite(got).all(), what
    if exact_energy:
        assert got[0] == ref[0], what
    else:
        assert np.isclose(got[0], ref[0], rtol=C.RTOL, atol=0), what
    assert got[1] == ref[1], what
    err = 0.0
    for c in range(2, 7):
        if c in zero:
            atol = atol_std if c == 2 else atol_band
            assert abs(got[c]) <= atol and abs(ref[c]) <= atol, (what, c, got[c], ref[c], atol)
        else:
            assert np.isclose(got[c], ref[c], rtol=C.RTOL, atol=0), (what, c, got[c], ref[c])
            err = max(err, abs(got[c] - ref[c]) / abs(ref[c]))
    return err


@pytest.mark.parametrize("fs", C.STRUCTURED_SIZES)
def test_structured_frames(torch_cuda, fs):
    from vad_amd.simple_analyser import SimpleAnalyser
    L, pad, bb = C.geometry(16000, fs)
    a, n = C.AMP, fs
    cross, half = C.crossing_frame(n)
    frames = {"zero": np.zeros(n, np.float32), "first": C.impulse(n, 0), "last": C.impulse(n, n - 1),
              "dc": C.dc(n), "alt": C.alternating(n), "cross": cross}
    tones = [bb - 1, bb, 4 * bb - 1, 4 * bb] if pad == 0 else []
    for k in tones:
        frames[f"tone{k}"] = C.tone(n, k)
    names = list(frames)
    got = dict(zip(names, SimpleAnalyser(16000, fs, 3).frame_features(np.stack([frames[k] for k in names]))))
    ref = {k: C.ref_features(frames[k], L, pad, bb) for k in names}
    err = 0.0

    assert np.array_equal(got["zero"], np.zeros(7)) and not np.signbit(got["zero"]).any()

    for k in ("first", "last"):      # |X| = a in every bin: std 0, every band a^2; mean |fft| = a
        err = max(err, _row(got[k], ref[k], zero=(2,), atol_std=C.RTOL * a, what=(fs, k)))
        assert np.allclose(got[k][3:], a * a, rtol=C.RTOL, atol=0)
        assert got[k][0] == a * a / n and got[k][1] == 0.5 / (n - 1.0) * n

    # DC: with pad 0 bin 0 alone, in band 0; padded, a Dirichlet kernel with no zero bin
    band0 = (a * n) ** 2 / bb
    err = max(err, _row(got["dc"], ref["dc"], zero=(4, 5, 6) if pad == 0 else (), atol_band=C.RTOL * band0,
                        what=(fs, "dc")))
    assert got["dc"][1] == 0.0 and got["dc"][0] == a * a
    if pad == 0:
        assert np.isclose(got["dc"][3], band0, rtol=C.RTOL, atol=0)

    # +a, -a: n - 1 crossings; with pad 0 bin L / 2 alone, past the four bands
    # (atol from the energy that bin would give a band)
    err = max(err, _row(got["alt"], ref["alt"], zero=(3, 4, 5, 6) if pad == 0 else (), atol_band=C.RTOL * band0,
                        what=(fs, "alt")))
    assert got["alt"][1] == float(n) and got["alt"][0] == a * a

    err = max(err, _row(got["cross"], ref["cross"], what=(fs, "cross")))
    assert got["cross"][1] == half / (n - 1.0) * n

    # a tone on the last bin of a band and on the first of the next: the energy
    # (a n / 2)^2 / band_bins moves with it; past 4 * band_bins no band has it.
    # The samples are float32 roundings of a cosine: not integers, so the
    # energy column depends on the order of its sum, and the other bins hold a
    # rounding floor of about 1e-15 of the tone's energy.
    e_tone = (a * n / 2) ** 2 / bb
    for k in tones:
        band = k // bb
        zero = tuple(c for c in (3, 4, 5, 6) if c - 3 != band)
        err = max(err, _row(got[f"tone{k}"], ref[f"tone{k}"], zero=zero, atol_band=C.RTOL * e_tone,
                            exact_energy=False, what=(fs, "tone", k)))
        if band < 4:
            assert np.isclose(got[f"tone{k}"][3 + band], e_tone, rtol=1e-6, atol=0)   # float32 samples
    if tones:
        assert [k // bb for k in tones] == [0, 1, 3, 4]
    _report(L, err, "structured")


# ---------------------------------------------------------------------------
# d. grid-stride loops
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fs,n_frames", [
    (16, 2048 * 4 * 2 + 3),    # wave kernel: 2048 blocks of 4 waves, every wave a second frame and three a third
    (15, 4096 * 2 + 3),        # direct kernel: 4096 blocks, every block a second frame and three a third
])
def test_grid_stride_loops(torch_cuda, fs, n_frames):
    from vad_amd.simple_analyser import SimpleAnalyser
    L, pad, bb = C.geometry(16000, fs)
    base = C.noise_frames(64, fs, 4000 + fs)
    pick = np.concatenate([np.arange(64), np.random.default_rng(fs).integers(0, 64, n_frames - 64)])
    sa = SimpleAnalyser(16000, fs, 3)
    small = sa.frame_features(base)
    err = C.assert_features(small, C.ref_rows(base, L, pad, bb), fs)
    big = sa.frame_features(base[pick])
    assert big.shape == (n_frames, 7)
    assert big.tobytes() == small[pick].tobytes()
    _report(L, err, f"{n_frames} frames")


# ---------------------------------------------------------------------------
# e. stale LDS
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fs", [1024, 2048, 4096, 8192, 255, 8191])
def test_features_ignore_stale_lds(torch_cuda, poison, fs):
    from vad_amd.simple_analyser import SimpleAnalyser
    L, pad, bb = C.geometry(16000, fs)
    frames = C.noise_frames(3 if L >= 8192 else 5, fs, 5000 + fs)
    sa = SimpleAnalyser(16000, fs, 3)
    C.assert_features(sa.frame_features(frames), C.ref_rows(frames, L, pad, bb), fs)
    check(poison, f"simple features L={L}", lambda: sa.frame_features(frames))


# ---------------------------------------------------------------------------
# f. / g. streams
# ---------------------------------------------------------------------------
def _stream_case(torch, rate, fs, nb, dtype, S, K, T):
    """A plain batch over a case's streams, in blocks of K with a short tail,
    checked against frame_features, the restatement on the kernel's own rows,
    the float64 reference's labels, a host SimpleAnalyser and the packed
    active frames.  Returns the batch's init tensor, frames and results."""
    from vad_amd import SimpleStreamBatch
    from vad_amd.simple_analyser import SimpleAnalyser
    dt = getattr(torch, dtype)
    L, pad, bb = C.geometry(rate, fs)
    init_np, x_np = C.streams(rate, fs, nb, S, T, C.STREAM_SEEDS[(rate, fs, nb)])
    want_labs = C.reference_labels(rate, fs, nb, init_np, x_np)
    for s in range(S):                                  # the condition the seed was chosen for
        assert set(want_labs[:, s].tolist()) == {0, 1}, s
    init, x = torch.from_numpy(init_np).cuda().to(dt), torch.from_numpy(x_np).cuda().to(dt)
    assert torch.equal(x.float().cpu(), torch.from_numpy(x_np))     # integer-valued: the cast is exact
    sb = SimpleStreamBatch(S, rate, fs, nb, frames_per_step=K, input_dtype=dt, features=True, voiced=True)
    assert sb.fft_len == L and sb.one_kernel == (C.is_pow2(L) and L <= 4096)
    sb.load_init_inactive_frames(init)
    start = sb.state.clone()
    sentinel = 12345
    labs, feats = [], []
    assert T % K != 0
    for t in range(0, T, K):
        blk = x[t:t + K]
        sb.voiced.fill_(sentinel)
        lab = sb.step_block(blk).clone()
        labs.append(lab)
        feats.append(sb.features[:blk.shape[0]].clone())
        v, n = sb.voiced.cpu(), sb.voiced_len.cpu().numpy()
        lab_np = lab.cpu().numpy()
        for s in range(S):
            want = blk[:, s][torch.from_numpy(lab_np[:, s].astype(bool)).cuda()].reshape(-1).cpu()
            assert n[s] == want.numel(), (t, s)
            assert torch.equal(v[s, :n[s]], want), (t, s)
            assert bool((v[s, n[s]:] == sentinel).all()), (t, s)       # nothing past voiced_len is written
    labs = torch.cat(labs).cpu().numpy()
    feats = torch.cat(feats).cpu().numpy()
    state = sb.state.cpu().numpy()
    assert labs.shape == (T, S) and feats.shape == (T, S, 7)
    # features: the class's, bit for bit, and the reference's within the tolerance
    sa = SimpleAnalyser(rate, fs, nb)
    rows = sa.frame_features(x_np.reshape(-1, fs)).reshape(T, S, 7)
    assert feats.tobytes() == rows.tobytes()
    err = C.assert_features(feats.reshape(-1, 7), C.ref_rows(x_np.reshape(-1, fs), L, pad, bb), (rate, fs))
    _report(L, err, f"stream rate {rate} frame {fs} nb {nb} {dtype}")
    for s in range(S):
        # the restatement of the state machine on the kernel's own rows: labels and the packed state
        init_rows = sa.frame_features(init_np[s])
        ref_l, st = R.run(feats[:, s], init_rows, nb)
        assert np.array_equal(labs[:, s], ref_l), s
        assert state[s].tobytes() == st.packed().tobytes(), s
        assert np.array_equal(labs[:, s], want_labs[:, s]), s
        host = SimpleAnalyser(rate, fs, nb)
        host.load_init_inactive_frames(list(init_np[s]))
        assert np.array_equal(np.array(host.classify_frames(list(x_np[:, s])), np.uint8), labs[:, s]), s
    return dict(sb=sb, init=init, x=x, start=start, labs=labs, feats=feats, state=state)


@pytest.mark.parametrize("rate,fs,nb,dtype", C.BLOCK_CASES)
def test_stream_block_kernel_lengths(torch_cuda, rate, fs, nb, dtype):
    run = _stream_case(torch_cuda, rate, fs, nb, dtype, C.BLOCK_S, C.BLOCK_K, C.BLOCK_T)
    assert run["sb"].one_kernel


@pytest.mark.parametrize("rate,fs,nb,dtype", C.TWO_LAUNCH_CASES)
def test_two_launch_path_lengths(torch_cuda, rate, fs, nb, dtype):
    torch = torch_cuda
    from vad_amd import _lib
    run = _stream_case(torch, rate, fs, nb, dtype, C.TWO_S, C.TWO_K, C.TWO_T)
    sb = run["sb"]
    assert sb.one_kernel is False
    if fs != 255:
        return
    # a block whose rows lie further apart than n_streams * stream_stride: one
    # feature launch per block row (capi.hip) in place of one for all
    S, K = C.TWO_S, C.TWO_K
    L, pad, bb = C.geometry(rate, fs)
    out = []
    for gap in (0, 17):
        wide = torch.full((K, S * fs + gap), float("nan"), dtype=torch.float32, device="cuda")
        wide[:, :S * fs] = run["x"][:K].reshape(K, S * fs)
        state = run["start"].clone()
        labels = torch.full((K, S), 0xAB, dtype=torch.uint8, device="cuda")
        feats = torch.full((K, S, 7), float("nan"), dtype=torch.float64, device="cuda")
        voiced = torch.full((S, K * fs), -7.0, dtype=torch.float32, device="cuda")
        vlen = torch.full((S,), -1, dtype=torch.int32, device="cuda")
        rc = _lib.lib().vad_simple_stream_block_f32(
            _lib.ptr(wide), S * fs + gap, fs, fs, L, pad, bb, S, K, nb, _lib.ptr(state), _lib.ptr(labels), S,
            _lib.ptr(feats), _lib.ptr(voiced), K * fs, _lib.ptr(vlen), _lib.stream_ptr())
        _lib.check(rc, "vad_simple_stream_block_f32")
        torch.cuda.synchronize()
        out.append(bits([labels, feats, state, voiced, vlen]))
    assert same(out[0], out[1])
    assert np.array_equal(out[1][0].numpy(), run["labs"][:K])
    assert out[1][1].numpy().view(np.float64).tobytes() == run["feats"][:K].tobytes()


def test_sessions_block_kernel_at_1024(torch_cuda):
    """sessions=True at L = 1024: stream 0 takes every frame, stream 1 joins
    two blocks late, stream 2 stalls twice and takes ragged counts; against
    the sessions restatement on the kernel's own rows and the float64
    reference's labels, which hold 0 and 1 in every stream."""
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    from vad_amd.simple_analyser import SimpleAnalyser
    rate, fs, nb = C.SESSIONS_CASE
    S, K, counts = C.SESSIONS_S, C.SESSIONS_K, C.SESSIONS_COUNTS
    L, pad, bb = C.geometry(rate, fs)
    blocks = C.sessions_blocks()
    want_labs = C.sessions_reference(blocks)
    for s in range(S):   # the condition the seed was chosen for: every stream is initialised, idle, 0 and 1
        assert set(np.concatenate(want_labs)[:, s].tolist()) == {0, 1, INIT, NO_HOP}, s
    sb = SimpleStreamBatch(S, rate, fs, nb, frames_per_step=K, features=True, voiced=True, sessions=True)
    assert sb.one_kernel and sb.fft_len == L
    ref = RS.RefSessions(S, nb)
    sa = SimpleAnalyser(rate, fs, nb)
    seen = [set() for _ in range(S)]
    err = 0.0
    for b, blk_np in enumerate(blocks):
        assert blk_np.shape == (K, S, fs)
        sb.voiced.fill_(-3.0)
        sb.features.fill_(float("nan"))
        before = sb.state.clone()
        lab = sb.step_block(torch.from_numpy(blk_np).cuda(), torch.from_numpy(counts[b]).cuda()).cpu().numpy()
        feats = sb.features.cpu().numpy()
        rows = sa.frame_features(blk_np.reshape(-1, fs)).reshape(K, S, 7)
        for s in range(S):
            n_s = int(counts[b, s])
            assert feats[:n_s, s].tobytes() == rows[:n_s, s].tobytes(), (b, s)
            assert np.isnan(feats[n_s:, s]).all(), (b, s)                            # rows past the count: not written
            if n_s:
                err = max(err, C.assert_features(feats[:n_s, s], C.ref_rows(blk_np[:n_s, s], L, pad, bb), (b, s)))
            else:
                assert torch.equal(sb.state[s], before[s]), (b, s)                   # stalled: every byte kept
        want, voiced = ref.block(np.nan_to_num(feats), counts[b], [0] * S)
        assert np.array_equal(lab, want), b
        assert np.array_equal(lab, want_labs[b]), b          # the float64 reference's labels
        v, n = sb.voiced.cpu().numpy(), sb.voiced_len.cpu().numpy()
        for s in range(S):
            packed = np.concatenate([blk_np[i, s] for i in voiced[s]]) if voiced[s] else np.zeros(0, np.float32)
            assert n[s] == packed.size and np.array_equal(v[s, :n[s]], packed), (b, s)
            assert (v[s, n[s]:] == -3.0).all()
            assert sb.state[s].cpu().numpy().tobytes() == ref.packed(s).tobytes(), (b, s)
            assert int(sb.init_left[s]) == ref.init_left(s)
            seen[s] |= set(lab[:, s].tolist())
    for s in range(S):
        assert seen[s] == {0, 1, INIT, NO_HOP}, s
    _report(L, err, "sessions")
