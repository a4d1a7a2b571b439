"""Live spectral noise subtraction in the hop kernels (StreamBatch(denoise=True),
vad_stream_hops_denoise and its _i16 / tree forms, vad_stream_noise_load)
against the host model of tests/stream_denoise_reference.py and the oracle.

Measured on an MI355X (printed by test_subtracted_rows_against_the_oracle):
  max |denoised row - f64| 4.1e-05 against the plain rows' yardstick 9.9e-06
  (bound 1.9e-04 at max |row| 351); spectrum rows 6.19 * 2^-24 of the row's
  largest bin against 6.16 * 2^-24 for numpy's float32 FFT (bound: twice that).
"""
import functools

import numpy as np
import pytest

from oracle import vad_oracle as O

import stream_denoise_reference as D
from test_gpu_stream_scores import (L, H, audio, batch, clip_chain_device, cuda, ffn, framing, is_16_chunk,  # noqa: F401
                                    packed, poison, torch_cuda, tree_with_scores)

pytestmark = pytest.mark.gpu

UNITS = 2.0 ** -20
STATE = ("frames", "ring", "count", "_spec", "_noise", "_est", "noise_count")


def bits(t):
    import torch
    return t if t.dtype in (torch.uint8, torch.int32) else t.contiguous().view(torch.int32)


def same(a, b):
    import torch
    return torch.equal(bits(a), bits(b))


def state(sb):
    return [getattr(sb, k).clone() for k in STATE]


def same_state(a, b, signed_zero=True):
    """Every state tensor bit for bit.  signed_zero=False compares the frames
    by value: an int16 batch holds +0 where the fp32 batch was fed -0."""
    import torch
    bad = [k for k, x, y in zip(STATE, a, b)
           if not (torch.equal(x, y) if k == "frames" and not signed_zero else same(x, y))]
    assert not bad, bad
    return True


@functools.lru_cache(maxsize=None)
def forced(net, cls, sign):
    """`net` with the last bias of class `cls` at +-1e6: every window with
    finite logits is, or none is, of that class.  (A window of identical rows
    -- digital silence, or frames wholly under the noise floor -- has NaN
    features and logits, and np.argmax's rule labels it 0 whatever the bias.)"""
    from vad_amd.ffn import FFNClassifier
    layers = [(w.copy(), b.copy()) for w, b in ffn(net).layers]
    layers[-1][1][cls] = sign * 1e6
    return FFNClassifier(layers)


def clf_for(name):
    return tree_with_scores() if name == "tree" else ffn(name)


def noise_frames(S, n, seed=77, dtype=np.float32, L=L):
    """n frames per stream of a noise floor: integer-valued Gaussian noise."""
    rng = np.random.default_rng(seed)
    return np.rint(rng.normal(0.0, 300.0, size=(S, n, L))).astype(dtype)


def step(sb, blk, K, graph=False):
    if K == 1:
        sb.step(blk[0])
    elif graph:
        sb.inputs.copy_(blk)
        sb.step_block()
    else:
        sb.step_block(blk)


# ---------------------------------------------------------------------------
# 1. zero noise is the plain hop; 2. silence under a loaded noise floor
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("name,S,K", [("bl13", 5, 8), ("ref39", 9, 3), ("tree", 5, 1), ("tree", 9, 8), ("bl13", 1, 1),
                                      ("tree", 1, 3)])
def test_zero_noise_is_the_plain_hop(torch_cuda, name, S, K, dtype, graph):
    torch = torch_cuda
    T, dt = 24, getattr(torch_cuda, dtype)
    carry, hops = audio(S, T)
    dh = cuda(hops).to(dt)
    clf = clf_for(name)
    for scores in (True, False):
        a = batch(torch, S, clf, carry, hops_per_step=K, input_dtype=dt, scores=scores, denoise=True,
                  noise_update=False)
        b = batch(torch, S, clf, carry, hops_per_step=K, input_dtype=dt, scores=scores)
        if graph:
            a.capture(), b.capture()
            if K == 1:
                assert a.graph_direct  # a one-kernel capture is still dispatched as its node
        for t0 in range(0, T, K):
            for sb in (a, b):
                step(sb, dh[t0:t0 + K], K, graph)
            where = (name, S, K, dtype, graph, scores, t0)
            assert torch.equal(a.label_block, b.label_block), where
            assert same(a.frames, b.frames) and same(a.ring, b.ring) and torch.equal(a.count, b.count), where
            if scores:
                assert same(a.score_block, b.score_block), where
        assert "denoise" in a._hop_name and "denoise" not in b._hop_name
        assert not a._est.any() and not a._noise.any() and not a.noise_count.any() and a._spec.any()
        assert (a.label_block != 255).all()


@pytest.mark.parametrize("name,dtype", [("bl13", "float32"), ("tree", "int16")])
def test_silence_under_a_loaded_noise_floor(torch_cuda, name, dtype):
    """Every bin clamps to 0, so the mel energies take the eps branch: the
    MFCC rows are the plain batch's on the same zero hops, bit for bit."""
    torch = torch_cuda
    S, T, dt = 5, 8, getattr(torch_cuda, dtype)
    a = batch(torch, S, clf_for(name), np.zeros((S, L - H), np.float32), input_dtype=dt, denoise=True,
              noise_update=False)
    b = batch(torch, S, clf_for(name), np.zeros((S, L - H), np.float32), input_dtype=dt)
    a.load_noise(cuda(noise_frames(S, 5)).to(dt))
    assert (a.noise_count == 5).all() and (a.noise_estimate > 0).all()
    zero = torch.zeros((S, H), dtype=dt, device="cuda")
    for t in range(T):
        a.step(zero), b.step(zero)
        assert same(a.ring, b.ring) and torch.equal(a.label_block, b.label_block), t
    assert not a._spec.any() and a.ring.any()


# ---------------------------------------------------------------------------
# 3. bookkeeping, 4. the estimate, and the records 5. reads
# ---------------------------------------------------------------------------
def run_recorded(torch, clf, S, T, noise_class, loaded_n, alpha=0.9, dtype="float32", update=True, L=L, H=H, **kw):
    """K = 1 hops with everything recorded per hop: labels, the raw spectrum
    row of the hop's frame, the estimate in force BEFORE the hop, the frame,
    the new MFCC ring row; the device's rows / count / estimate are checked
    against the host replay and the fp32 model after every hop."""
    dt = getattr(torch, dtype)
    carry, hops = audio(S, T, L=L, H=H)
    dh = cuda(hops).to(dt)
    sb = batch(torch, S, clf, carry, input_dtype=dt, denoise=True, alpha=alpha, noise_class=noise_class,
               noise_update=update, cfg=framing(L, H), **kw)
    loaded = np.zeros((S, 0, D.BINS), np.float32)
    if loaded_n:
        sb.load_noise(cuda(noise_frames(S, loaded_n, L=L)).to(dt))
        loaded = sb._noise[:, :loaded_n].cpu().numpy()
        assert (sb.noise_count == loaded_n).all() and not sb._noise[:, loaded_n:].any()
    rec = dict(lab=[], spec=[], est=[], frame=[], row=[])
    for t in range(T):
        rec["est"].append(sb._est.cpu().numpy())
        sb.step(dh[t])
        rec["lab"].append(sb.labels.cpu().numpy().copy())
        rec["spec"].append(sb._spec[:, t % 5].cpu().numpy())
        rec["frame"].append(sb.frames.cpu().numpy())
        rec["row"].append(sb.ring[:, t % 5].cpu().numpy())
        rec.setdefault("rows", []).append(sb._noise.cpu().numpy())
        rec.setdefault("cnt", []).append(sb.noise_count.cpu().numpy())
        rec.setdefault("est_after", []).append(sb._est.cpu().numpy())
    rec = {k: np.stack(v, axis=1) for k, v in rec.items()}  # (S, T, ...)
    pushes = 0
    for s in range(S):
        held = D.replay(rec["lab"][s], rec["spec"][s], noise_class, loaded=loaded[s], update=update)
        for t in range(T):
            n = len(held[t])
            assert rec["cnt"][s, t] == n, (s, t)
            assert np.array_equal(rec["rows"][s, t, :n].view(np.uint32), held[t].view(np.uint32)), (s, t)
            want = D.estimate_f32(rec["rows"][s, t, :n], alpha)
            assert np.array_equal(rec["est_after"][s, t].view(np.uint32), want.view(np.uint32)), (s, t)
        pushes += int((rec["lab"][s] == noise_class).sum())
    return sb, rec, pushes, loaded


@pytest.mark.parametrize("case", ["always", "never", "real_bl13", "real_tree", "three_class_1", "int16_alpha_half"])
def test_bookkeeping_and_estimate(torch_cuda, case):
    torch = torch_cuda
    S, T = 5, 20
    if case == "always":  # more than five pushes: eviction
        sb, rec, pushes, _ = run_recorded(torch, forced("bl13", 0, +1), S, T, 0, 2)
        assert pushes == S * (T - 5) and (rec["cnt"][:, -1] == 5).all() and (rec["lab"][:, 5:] == 0).all()
        assert np.array_equal(rec["rows"][:, -1], rec["spec"][:, T - 8:T - 3])
    elif case == "never":  # the loaded rows stay untouched (class 0 forced, NaN windows are 0 too: never class 1)
        sb, rec, pushes, loaded = run_recorded(torch, forced("bl13", 0, +1), S, T, 1, 3)
        assert pushes == 0 and np.array_equal(rec["rows"][:, -1, :3], loaded) and (rec["cnt"] == 3).all()
        assert np.array_equal(rec["est_after"][:, -1], rec["est"][:, 0])
    elif case == "real_bl13":
        sb, rec, pushes, _ = run_recorded(torch, ffn("bl13"), 9, 40, 0, 0, scores=True)
        assert 0 < pushes < 9 * 35
    elif case == "real_tree":
        sb, rec, pushes, _ = run_recorded(torch, tree_with_scores(), S, 40, 1, 1)
        assert 0 < pushes < S * 35
    elif case == "three_class_1":
        sb, rec, pushes, _ = run_recorded(torch, forced("ref39", 1, +1), S, T, 1, 0)
        assert S * (T - 5) // 2 < pushes <= S * (T - 5) and (rec["cnt"][:, -1] == 5).all()
    else:
        sb, rec, pushes, _ = run_recorded(torch, forced("bl13", 1, +1), 1, T, 1, 5, alpha=0.5, dtype="int16")
        assert 0 < pushes <= T - 5
    sb.reset()
    assert not any(getattr(sb, k).any() for k in STATE) and (sb.label_block == 255).all()


FRAMINGS_16 = [(512, 160), (1000, 333)]  # frames past 448 samples: the 16-chunk builds


@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("case", ["real_bl13", "real_tree"])
@pytest.mark.parametrize("L16,H16", FRAMINGS_16)
def test_bookkeeping_and_estimate_16_chunk_builds(torch_cuda, L16, H16, case, dtype):
    """run_recorded's checks (rows, count and estimate against the host replay
    and the fp32 model after every hop) in the 16-chunk builds."""
    torch = torch_cuda
    if case == "real_bl13":
        sb, rec, pushes, _ = run_recorded(torch, ffn("bl13"), 9, 40, 0, 0, dtype=dtype, L=L16, H=H16, scores=True)
    else:
        sb, rec, pushes, _ = run_recorded(torch, tree_with_scores(), 5, 40, 1, 1, dtype=dtype, L=L16, H=H16)
    assert pushes > 0 and (rec["cnt"][:, -1] > 0).any()  # noise rows were pushed: there was bookkeeping to check
    assert is_16_chunk(sb) and sb._hop_name == ("vad_stream_hops_tree" if case == "real_tree" else "vad_stream_hops") \
        + "_denoise" + ("_i16" if dtype == "int16" else "")


@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("n", [1, 3, 5])
def test_load_noise(torch_cuda, n, dtype):
    """The loaded rows are the rows a hop stores for the same frames, the
    estimate is the fp32 model's, bit for bit; the properties' units."""
    load_noise_checks(torch_cuda, n, dtype)


@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("L16,H16", FRAMINGS_16)
def test_load_noise_16_chunk_builds(torch_cuda, L16, H16, n, dtype):
    """test_load_noise at frames of 512 and of 1000 samples: the second is
    longer than the 512-point transform, which sees the first 512 samples in
    the load kernel and in the hop kernel alike."""
    assert is_16_chunk(load_noise_checks(torch_cuda, n, dtype, L16, H16))


def load_noise_checks(torch, n, dtype, L=L, H=H):
    S, dt = 9, getattr(torch, dtype)
    fr = noise_frames(S, n, seed=n, L=L)
    kw = dict(input_dtype=dt, denoise=True, noise_update=False, cfg=framing(L, H))
    sb = batch(torch, S, ffn("bl13"), fr[:, 0, H:], **kw)
    sb._noise.fill_(-1.0)
    sb.load_noise(cuda(fr).to(dt))
    rows = sb._noise.cpu().numpy()
    assert (sb.noise_count == n).all() and (rows[:, n:] == -1.0).all()
    for s in range(S):
        want = D.estimate_f32(rows[s, :n], 0.9)
        assert np.array_equal(sb._est[s].cpu().numpy().view(np.uint32), want.view(np.uint32)), s
    assert np.array_equal(sb.noise_estimate.cpu().numpy(), sb._est.cpu().numpy() * np.float32(UNITS))
    assert np.array_equal(sb.noise_rows.cpu().numpy(), rows * np.float32(UNITS))
    # frame 0 again through a hop (the carry is its tail, the hop its last H samples after a shift by H)
    probe = batch(torch, S, ffn("bl13"), fr[:, 0, :L - H], **kw)
    probe.step(cuda(np.ascontiguousarray(fr[:, 0, L - H:])).to(dt))
    assert np.array_equal(probe.frames.cpu().numpy(), fr[:, 0].astype(np.float32))
    assert same(probe._spec[:, 0], sb._noise[:, 0])
    if L > 512:  # and samples past the transform's 512 change nothing
        cut = fr.copy()
        cut[:, :, 512:] = 0
        sb2 = batch(torch, S, ffn("bl13"), fr[:, 0, H:], **kw)
        sb2.load_noise(cuda(cut).to(dt))
        assert same(sb2._noise[:, :n], sb._noise[:, :n]) and same(sb2._est, sb._est)
    return probe


# ---------------------------------------------------------------------------
# 5. the subtracted MFCC rows
# ---------------------------------------------------------------------------
def test_subtracted_rows_against_the_oracle(torch_cuda):
    """Per recorded hop: get_mfcc_from_spec(max(p - e, 0)) in float64 from the
    device's own fp32 p (spectrum ring) and the e in force before the hop,
    against the device's ring row.  Yardstick: the zero-noise batch's rows (the
    plain batch's, bit for bit) against get_mfcc_from_spec(p) of its own
    recorded p.  Bound: twice the yardstick plus 8 * 2^-24 * max|row|."""
    subtracted_rows_checks(torch_cuda)


@pytest.mark.parametrize("L16,H16", FRAMINGS_16)
def test_subtracted_rows_against_the_oracle_16_chunk_builds(torch_cuda, L16, H16):
    """The same comparisons under the same bounds in the 16-chunk build; the
    oracle's spectrum is given the frame as the transform sees it, its first
    512 samples."""
    assert is_16_chunk(subtracted_rows_checks(torch_cuda, L16, H16))


def subtracted_rows_checks(torch, L=L, H=H):
    S, T = 5, 40
    fb = O.get_mel_filterbanks(300, 8000, 512, 26, 16000)
    sb, rec, pushes, _ = run_recorded(torch, ffn("bl13"), S, T, 0, 5, L=L, H=H)
    assert pushes > 0 and (rec["est"] > 0).any()
    p, e = rec["spec"].astype(np.float64) * UNITS, rec["est"].astype(np.float64) * UNITS
    sub = np.maximum(p - e, 0.0)
    assert (sub == 0).any() and (sub > 0).any()  # both sides of the clamp
    want = O.get_mfcc_from_spec(sub.reshape(-1, 256), fb).reshape(S, T, -1)
    err = np.abs(rec["row"].astype(np.float64) - want).max()
    zb, zrec, _, _ = run_recorded(torch, ffn("bl13"), S, T, 0, 0, update=False, L=L, H=H)
    plain = batch(torch, S, ffn("bl13"), audio(S, T, L=L, H=H)[0], cfg=framing(L, H))
    for t in range(T):
        plain.step(cuda(audio(S, T, L=L, H=H)[1][t]))
    assert same(plain.ring, zb.ring)
    zwant = O.get_mfcc_from_spec((zrec["spec"].astype(np.float64) * UNITS).reshape(-1, 256), fb).reshape(S, T, -1)
    yard = np.abs(zrec["row"].astype(np.float64) - zwant).max()
    top = np.abs(want).max()
    print(f"\nmax |denoised row - f64| = {err:.3e}; plain rows' yardstick {yard:.3e}; max |row| {top:.3e}; "
          f"bound {2 * yard + 8 * 2.0 ** -24 * top:.3e}")
    assert err <= 2 * yard + 8 * 2.0 ** -24 * top
    # a recorded spectrum row against the oracle's get_spec_mag of the recorded frame, both against float64.
    # The audio spans eight decades of power, so each row's error is taken relative to the row's largest bin;
    # yardstick: numpy's FFT of the float32 frame (complex64 in NumPy 2, as the oracle notes); margin: two.
    fr = rec["frame"].reshape(-1, L)[:, :512]  # what the 512-point transform sees of a longer frame
    ref = np.abs(np.fft.fft(fr.astype(np.float64), 512)[:, :256] / 512.0) ** 2
    live = ref.max(axis=1) > 0
    npy = np.stack([O.get_spec_mag(f) for f in fr]).astype(np.float64)
    assert O.get_spec_mag(fr[0]).dtype == np.float32
    rel = lambda x: (np.abs(x - ref)[live].max(axis=1) / ref[live].max(axis=1)).max()
    s_err, s_yard = rel(p.reshape(-1, 256)), rel(npy)
    print(f"max over rows of |device spectrum - f64| / max(row) = {s_err:.3e} = {s_err * 2 ** 24:.2f} * 2^-24; "
          f"numpy float32 FFT yardstick {s_yard:.3e} = {s_yard * 2 ** 24:.2f} * 2^-24")
    assert s_err <= 2 * s_yard
    assert np.abs(rec["row"] - zrec["row"]).max() > 0.1  # and the subtraction does something
    return sb


# ---------------------------------------------------------------------------
# 6. one launch of K hops = K launches of one; int16 = fp32; permuted streams
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,S", [("bl13", 5), ("tree", 9), ("ref39", 1)])
def test_block_equals_single_hops(torch_cuda, name, S):
    torch = torch_cuda
    K, T = 8, 32
    clf = clf_for(name)
    carry, hops = audio(S, T)
    fr = noise_frames(S, 2)
    perm = np.roll(np.arange(S), 1)

    def run(k, dtype, order=None, graph=False):
        dt = getattr(torch, dtype)
        o = np.arange(S) if order is None else order
        sb = batch(torch, S, clf, carry[o], hops_per_step=k, input_dtype=dt, scores=True, denoise=True, noise_class=0)
        sb.load_noise(cuda(fr[o]).to(dt))
        if graph:
            sb.capture()
        dh = cuda(hops[:, o]).to(dt)
        out, n_mid = [], 0
        for t0 in range(0, T, k):
            step(sb, dh[t0:t0 + k], k, graph)
            out.append((sb.label_block.clone(), sb.score_block.clone()))
            if k > 1:  # the classifier updates in mid-block: some label but the last of the block is the noise class
                n_mid += int((sb.label_block[:-1] == 0).sum())
        lab = torch.cat([a for a, _ in out])
        sc = torch.cat([b for _, b in out])
        return lab, sc, state(sb), n_mid

    lab1, sc1, st1, _ = run(1, "float32")
    assert (lab1 == 0).any() and (lab1[5:] != 0).any()
    for k, dtype, graph in ((K, "float32", False), (K, "int16", False), (1, "int16", False), (K, "float32", True),
                            (4, "int16", True)):
        lab, sc, st, n_mid = run(k, dtype, graph=graph)
        assert k == 1 or n_mid > 0
        assert torch.equal(lab, lab1) and same(sc, sc1), (k, dtype, graph)
        assert same_state(st, st1, signed_zero=dtype == "float32"), (k, dtype, graph)
    if S > 1:
        labp, scp, stp, _ = run(K, "float32", order=perm)
        assert torch.equal(labp, lab1[:, perm]) and same(scp, sc1[:, perm])
        assert all(same(a, b[perm]) for a, b in zip(stp, st1))


# ---------------------------------------------------------------------------
# 7. tree tables; 8. stale LDS
# ---------------------------------------------------------------------------
def test_tree_walks_agree(torch_cuda):
    torch = torch_cuda
    S, K, T = 5, 3, 24
    carry, hops = audio(S, T)
    dh = cuda(hops)
    outs = []
    for walk in ("auto", "global"):
        sb = batch(torch, S, tree_with_scores(), carry, hops_per_step=K, scores=True, denoise=True, noise_class=0,
                   tree_walk=walk)
        sb.load_noise(cuda(noise_frames(S, 4)))
        labs = []
        for t0 in range(0, T, K):
            sb.step_block(dh[t0:t0 + K])
            labs.append((sb.label_block.clone(), sb.score_block.clone()))
        outs.append((labs, state(sb)))
    (la, sa), (lb, sb_) = outs
    assert all(torch.equal(a, c) and same(b, d) for (a, b), (c, d) in zip(la, lb))
    assert all(same(a, b) for a, b in zip(sa, sb_)) and sa[-1].any()


@pytest.mark.parametrize("which", ["ffn", "tree_auto", "tree_global"])
def test_denoise_kernels_ignore_stale_lds(torch_cuda, poison, which):
    torch = torch_cuda
    S, T = 5, 16
    carry, hops = audio(S, T)
    dh = cuda(hops)
    clf = ffn("ref39") if which == "ffn" else tree_with_scores()
    kw = {} if which == "ffn" else dict(tree_walk=which[5:])
    fr = cuda(noise_frames(S, 3))

    def run(K, fill):
        sb = batch(torch, S, clf, carry, hops_per_step=K, scores=True, denoise=True, noise_class=0, **kw)
        if fill is not None:
            poison(fill)
        sb.load_noise(fr)
        out = []
        for t0 in range(0, T, K):
            if fill is not None:
                poison(fill)
            step(sb, dh[t0:t0 + K], K)
            out.append(bits(sb.label_block).clone())
            out.append(bits(sb.score_block).clone())
        return out + [bits(x) for x in state(sb)]

    for K in (1, 8):
        want = run(K, None)
        for v in (1e30, -1e30, float("nan")):
            got = run(K, v)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (which, K, v)


# ---------------------------------------------------------------------------
# the other forms of a step; 9. end to end in one graph
# ---------------------------------------------------------------------------
def test_host_forms_and_resampler_in_front(torch_cuda):
    """step_host, host_pipeline and a StreamResampler in front give the direct
    steps' labels and state."""
    torch = torch_cuda
    S, K, T = 5, 4, 16
    carry, hops = audio(S, T)
    h16 = hops.astype(np.int16)
    fr = cuda(noise_frames(S, 3, dtype=np.int16))

    def fresh():
        sb = batch(torch, S, ffn("bl13"), carry.astype(np.int16), hops_per_step=K, input_dtype=torch.int16,
                   denoise=True, noise_class=0)
        sb.load_noise(fr)
        return sb

    ref, want = fresh(), []
    for t0 in range(0, T, K):
        want.append(ref.step_block(cuda(h16[t0:t0 + K])).cpu().numpy().copy())
    a = fresh()
    a.attach_host_io()
    for i, t0 in enumerate(range(0, T, K)):
        a.host_inputs.copy_(torch.from_numpy(h16[t0:t0 + K]))
        a.step_host()
        torch.cuda.synchronize()
        assert np.array_equal(a.host_labels.numpy(), want[i])
    b = fresh()
    pipe = b.host_pipeline(2)
    for i, t0 in enumerate(range(0, T, K)):
        pipe.host_inputs[i % 2].copy_(torch.from_numpy(h16[t0:t0 + K]))
        pipe.submit(i % 2)
        assert np.array_equal(pipe.wait(i % 2).numpy(), want[i])
    pipe.drain()
    for sb in (a, b):
        assert all(same(x, y) for x, y in zip(state(sb), state(ref)))
    # a 48 kHz resampler writing the batch's static input block: the hop kernel reads its output in place,
    # and a second batch fed the same 16 kHz blocks as tensors gives the same labels and state
    from vad_amd import resample as R
    x = np.stack([O.synth_clip(T * 480, seed=70 + s)[:T * 480] for s in range(S)]).astype(np.int16)
    blocks = torch.from_numpy(np.ascontiguousarray(x.reshape(S, T, 480).transpose(1, 0, 2))).cuda()
    fresh32 = lambda: batch(torch, S, ffn("bl13"), carry, hops_per_step=K, denoise=True, noise_class=0)
    c, d = fresh32(), fresh32()
    sr = R.StreamResampler(S, 48000, hops_per_step=K, input_dtype=torch.int16, out=c.inputs)
    for t0 in range(0, T, K):
        sr.step_block(blocks[t0:t0 + K])
        got = c.step_block().clone()
        assert torch.equal(got, d.step_block(c.inputs.clone()))
    assert all(same(x, y) for x, y in zip(state(c), state(d))) and c._spec.any()
    assert (c.label_block != 255).all()


def test_end_to_end_one_graph(torch_cuda):
    torch = torch_cuda
    S, K, T, g, m, pad, on, off = 5, 8, 64, 2, 3, (2, 3), 0.6, 0.4
    carry, hops = audio(S, T, seed=1600)
    c16, h16 = carry.astype(np.int16), hops.astype(np.int16)
    sb = batch(torch, S, ffn("bl13"), c16, hops_per_step=K, input_dtype=torch.int16, scores=True, denoise=True,
               noise_class=0)
    sb.load_noise(cuda(noise_frames(S, 5, dtype=np.int16)))
    seg = sb.segmenter(on=on, off=off, pad=pad, max_gap=g, min_run=m)
    seg.prime(cuda(c16))

    def body():
        sb._block_body()
        seg.push(sb.score_block, sb.inputs)

    tensors = [getattr(sb, k) for k in STATE] + [seg.state, seg.found, seg.history, seg.table]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    saved = [t.clone() for t in tensors]
    with torch.cuda.stream(side):
        body()  # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t, v in zip(tensors, saved):
        t.copy_(v)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    scs, outs = [], []
    for t0 in range(0, T, K):
        sb.inputs.copy_(cuda(h16[t0:t0 + K]))
        graph.replay()
        scs.append(sb.score_block.cpu().numpy().copy())
        outs.append((seg.voiced.cpu().numpy().copy(), seg.voiced_len.cpu().numpy().copy()))
    fv, fn = seg.flush()
    outs.append((fv.cpu().numpy(), fn.cpu().numpy()))
    sc = np.concatenate(scs)
    assert np.isnan(sc[:5]).all() and not np.isnan(sc[5:]).any() and sb.noise_count.any()
    clip = np.concatenate([c16, h16.transpose(1, 0, 2).reshape(S, -1)], axis=1)
    rows, found = seg.segments(), seg.found.cpu().numpy()
    for s in range(S):
        want, count, voiced = clip_chain_device(torch, sc[5:, s], clip[s], g, m, pad, on, off)
        assert found[s] == count and np.array_equal(rows[s], want), s
        assert np.array_equal(packed(outs, s, np.int16), voiced), s
