"""SimpleStreamBatch on the device: many SimpleAnalyser streams per launch.

Golden traces of the unmodified reference class (tests/golden/simple.npz),
independence of streams and of the block size, features against
SimpleAnalyser.frame_features bit for bit (the shared wave body), int16
input, strided views, the state kernel alone on hand-made rows, the packed
voiced output, graph replay, moving a stream to and from the host class,
stale LDS, and the reference's exceptions."""
import numpy as np
import pytest

import simple_stream_reference as R
from test_gpu_lds_independence import bits, check, poison, same  # noqa: F401  (poison: a fixture)

pytestmark = pytest.mark.gpu

RATE = 16000
OFFSETS = (0, 60, 150, 290, 420)   # five streams cut from case a's frames
T = 60                             # frames per stream: no multiple of 8 or 20


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _case(golden, case):
    g = golden("simple")
    fs, nb = int(g[f"{case}_meta"][0]), int(g[f"{case}_meta"][1])
    return fs, nb, g[f"{case}_frames"], g[f"{case}_trace"]


def _drive(torch, sb, x, K, before=None):
    """Feed x (T, S, fs) in blocks of K (the tail a short block); returns
    labels (T, S) and, per block, the state after it and the features."""
    labs, states, feats = [], [], []
    for t in range(0, x.shape[0], K):
        blk = x[t:t + K]
        if before is not None:
            before(blk)
        lab = sb.step(blk[0]).unsqueeze(0) if K == 1 else sb.step_block(blk)
        labs.append(lab.clone())
        states.append(sb.state.clone())
        if sb.features is not None:
            feats.append(sb.features[:blk.shape[0]].clone())
    torch.cuda.synchronize()
    return (torch.cat(labs).cpu().numpy(), [s.cpu().numpy() for s in states],
            torch.cat(feats).cpu().numpy() if feats else None)


# ---------------------------------------------------------------------------
# golden traces
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case,K", [("a", 8), ("b", 1), ("b", 7), ("c", 4)])
def test_golden_traces(torch_cuda, golden, case, K):
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    fs, nb, frames, ref = _case(golden, case)
    S = 3
    sb = SimpleStreamBatch(S, RATE, fs, nb, frames_per_step=K)
    assert sb.one_kernel == (case != "c")          # 401 samples: L = 513, the two-launch path
    x = torch.from_numpy(frames.astype(np.float32)).cuda()
    sb.load_init_inactive_frames(x[:nb].unsqueeze(0).expand(S, nb, fs))
    labs, states, _ = _drive(torch, sb, x[nb:].unsqueeze(1).expand(-1, S, fs), K)
    n = len(ref)
    assert labs.shape == (n, S)
    for s in range(S):
        assert np.array_equal(labs[:, s], ref[:, 0])
    ends = [min(t + K, n) - 1 for t in range(0, n, K)]   # the frame each recorded state follows
    assert ends[-1] == n - 1 and (n % K != 0) == ((case, K) == ("b", 7))   # b, 7: the tail is a short block
    for st, e in zip(states, ends):
        w = st.view(np.int32)[:, 2 * (6 * nb + 6):]
        assert np.array_equal(w[:, 1], np.full(S, ref[e, 1]))              # silence
        assert np.array_equal(w[:, 3], np.full(S, e + 1))                  # frame_number
        th = st[:, 6 * nb:6 * nb + 6]
        assert np.allclose(th, np.broadcast_to(ref[e, 2:], (S, 6)), rtol=1e-10, atol=0)
        assert st[0].tobytes() == st[1].tobytes() == st[2].tobytes()      # the three streams identical
    assert bool(sb.silence[0]) == bool(ref[-1, 1]) and int(sb.frame_number[0]) == n


# ---------------------------------------------------------------------------
# independence of streams and of K; the restatement on the kernel's own rows
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def five(torch_cuda, golden):
    """Five streams from case a: init (S, nb, fs) and x (T, S, fs) fp32 on the
    device, and the reference run (K = 8, all streams, with features)."""
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    fs, nb, frames, _ = _case(golden, "a")
    f32 = frames.astype(np.float32)
    init = torch.from_numpy(np.stack([f32[o:o + nb] for o in OFFSETS])).cuda()
    x = torch.from_numpy(np.stack([f32[o + nb:o + nb + T] for o in OFFSETS], axis=1)).cuda()
    sb = SimpleStreamBatch(len(OFFSETS), RATE, fs, nb, frames_per_step=8, features=True)
    sb.load_init_inactive_frames(init)
    labs, states, feats = _drive(torch, sb, x, 8)
    return dict(fs=fs, nb=nb, init=init, x=x, labs=labs, state=states[-1], feats=feats)


@pytest.mark.parametrize("K", [1, 3, 20])
def test_block_size_changes_nothing(torch_cuda, five, K):
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    sb = SimpleStreamBatch(len(OFFSETS), RATE, five["fs"], five["nb"], frames_per_step=K, features=True)
    sb.load_init_inactive_frames(five["init"])
    labs, states, feats = _drive(torch, sb, five["x"], K)
    assert np.array_equal(labs, five["labs"])
    assert states[-1].tobytes() == five["state"].tobytes()
    assert feats.tobytes() == five["feats"].tobytes()


def test_streams_are_independent(torch_cuda, five):
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    for s in range(len(OFFSETS)):
        sb = SimpleStreamBatch(1, RATE, five["fs"], five["nb"], frames_per_step=8)
        sb.load_init_inactive_frames(five["init"][s:s + 1])
        labs, states, _ = _drive(torch, sb, five["x"][:, s:s + 1], 8)
        assert np.array_equal(labs[:, 0], five["labs"][:, s])
        assert states[-1][0].tobytes() == five["state"][s].tobytes()


def test_state_equals_restatement_on_the_kernels_rows(torch_cuda, five):
    from vad_amd.simple_analyser import SimpleAnalyser
    sa = SimpleAnalyser(RATE, five["fs"], five["nb"])
    seen = set()
    for s in range(len(OFFSETS)):
        init_rows = sa.frame_features(five["init"][s].cpu().numpy())
        labs, st = R.run(five["feats"][:, s], init_rows, five["nb"])
        assert np.array_equal(labs, five["labs"][:, s])
        assert st.packed().tobytes() == five["state"][s].tobytes()   # bit for bit: noise_buf_len < 8
        seen |= set(labs.tolist())
    assert seen == {0, 1}


# ---------------------------------------------------------------------------
# features: the shared wave body, int16 input, strided views
# ---------------------------------------------------------------------------
def test_features_equal_frame_features(torch_cuda, five):
    from vad_amd.simple_analyser import SimpleAnalyser
    sa = SimpleAnalyser(RATE, five["fs"], five["nb"])
    want = sa.frame_features(five["x"].reshape(-1, five["fs"]).cpu().numpy()).reshape(T, len(OFFSETS), 7)
    assert five["feats"].tobytes() == want.tobytes()


@pytest.mark.parametrize("view", ["contiguous", "strided"])
def test_int16_equals_fp32(torch_cuda, five, view):
    """int16 frames read in place give the fp32 run's labels, state and
    features; 'strided': rows of a wider buffer at a non-zero, odd offset,
    for both dtypes."""
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    fs, S = five["fs"], len(OFFSETS)
    for dtype in (torch.int16, torch.float32):
        x, init = five["x"].to(dtype), five["init"].to(dtype)
        assert torch.equal(x.float(), five["x"])     # int16 audio: the cast is exact
        if view == "strided":
            wide = torch.zeros((T, S, fs + 25), dtype=dtype, device="cuda")
            wide[:, :, 3:3 + fs] = x
            x = wide[:, :, 3:3 + fs]
            assert x.storage_offset() == 3 and x.stride(1) == fs + 25 and not x.is_contiguous()
        elif dtype == torch.float32:
            continue                                  # the fixture's own run
        sb = SimpleStreamBatch(S, RATE, fs, five["nb"], frames_per_step=8, input_dtype=dtype, features=True)
        sb.load_init_inactive_frames(init)
        before = sb.inputs.clone()
        labs, states, feats = _drive(torch, sb, x, 8)
        assert torch.equal(sb.inputs, before)         # read in place: the static input was not used
        assert np.array_equal(labs, five["labs"])
        assert states[-1].tobytes() == five["state"].tobytes()
        assert feats.tobytes() == five["feats"].tobytes()


# ---------------------------------------------------------------------------
# the state kernel alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 3])
def test_state_kernel_on_edge_rows(torch_cuda, nb):
    torch = torch_cuda
    from vad_amd import _lib
    from vad_amd import simple_stream as SS
    S = 65                                            # a second workgroup and a partial one
    seqs = list(R.edge_sequences().values())
    rows = np.stack([seqs[s % len(seqs)] for s in range(S)], axis=1)      # (K, S, 7)
    K = rows.shape[0]
    lib = _lib.lib()
    state = torch.full((S, SS.state_doubles(nb)), float("nan"), dtype=torch.float64, device="cuda")
    init = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(R.edge_init(nb), (S, nb, 7)))).cuda()
    feats = torch.from_numpy(rows).cuda()
    labels = torch.full((K, S), 0xAB, dtype=torch.uint8, device="cuda")
    _lib.check(lib.vad_simple_stream_init(_lib.ptr(init), S, nb, _lib.ptr(state), _lib.stream_ptr()), "init")
    torch.cuda.synchronize()
    want0 = R.RefStream(nb).init(R.edge_init(nb)).packed()
    assert state.cpu().numpy().tobytes() == np.stack([want0] * S).tobytes()
    # in two calls, so that the state carries from one to the next
    for a, b in ((0, 11), (11, K)):
        _lib.check(lib.vad_simple_stream_state(_lib.ptr(feats[a:b]), S, b - a, nb, _lib.ptr(state),
                                               _lib.ptr(labels[a:b]), S, _lib.stream_ptr()), "state")
    torch.cuda.synchronize()
    got_l, got_s = labels.cpu().numpy(), state.cpu().numpy()
    for s in range(S):
        want_l, st = R.run(rows[:, s], R.edge_init(nb), nb)
        assert np.array_equal(got_l[:, s], want_l), s
        assert got_s[s].tobytes() == st.packed().tobytes(), s


# ---------------------------------------------------------------------------
# voiced
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_voiced_packs_the_active_frames(torch_cuda, five, dtype):
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    dt = getattr(torch, dtype)
    fs, S, K = five["fs"], len(OFFSETS), 8
    x = five["x"].to(dt)
    sb = SimpleStreamBatch(S, RATE, fs, five["nb"], frames_per_step=K, input_dtype=dt, voiced=True)
    sb.load_init_inactive_frames(five["init"].to(dt))
    sentinel = 12345
    lens = set()
    for t in range(0, T, K):
        blk = x[t:t + K]
        sb.voiced.fill_(sentinel)
        lab = sb.step_block(blk).cpu().numpy()
        assert np.array_equal(lab, five["labs"][t:t + K])
        v, n = sb.voiced.cpu(), sb.voiced_len.cpu().numpy()
        for s in range(S):
            want = blk[:, s][torch.from_numpy(lab[:, s].astype(bool))].reshape(-1).cpu()
            assert n[s] == want.numel()
            assert torch.equal(v[s, :n[s]], want)
            assert bool((v[s, n[s]:] == sentinel).all())          # nothing past voiced_len is written
            lens.add((int(n[s]), blk.shape[0]))
    assert (0, K) in lens and (K * fs, K) in lens                 # an all-quiet and an all-active block


def test_voiced_two_launch_path(torch_cuda, golden):
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    fs, nb, frames, ref = _case(golden, "c")
    x = torch.from_numpy(frames.astype(np.float32)).cuda()
    K, S = 4, 2
    sb = SimpleStreamBatch(S, RATE, fs, nb, frames_per_step=K, voiced=True)
    sb.load_init_inactive_frames(x[:nb].unsqueeze(0).expand(S, nb, fs))
    lens = set()
    for t in range(nb + 20, nb + 44, K):      # the trace's frames 20..43: active, then quiet
        if t == nb + 20:
            for u in range(nb, t, K):
                sb.step_block(x[u:u + K].unsqueeze(1).expand(K, S, fs))
        blk = x[t:t + K].unsqueeze(1).expand(K, S, fs)
        sb.voiced.fill_(-7.0)
        lab = sb.step_block(blk).cpu().numpy()
        assert np.array_equal(lab[:, 0], ref[t - nb:t - nb + K, 0])
        v, n = sb.voiced.cpu(), sb.voiced_len.cpu().numpy()
        for s in range(S):
            want = x[t:t + K][torch.from_numpy(lab[:, s].astype(bool)).cuda()].reshape(-1).cpu()
            assert n[s] == want.numel() and torch.equal(v[s, :n[s]], want)
            assert bool((v[s, n[s]:] == -7.0).all())
            lens.add(int(n[s]))
    assert 0 in lens and K * fs in lens


# ---------------------------------------------------------------------------
# graph, moving a stream, stale LDS, exceptions
# ---------------------------------------------------------------------------
def test_graph_replay_equals_direct_blocks(torch_cuda, five):
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    fs, S, K = five["fs"], len(OFFSETS), 4
    x = five["x"][16:28]                       # three blocks, across a silence switch of some stream
    out = []
    for graph in (False, True):
        sb = SimpleStreamBatch(S, RATE, fs, five["nb"], frames_per_step=K, features=True, voiced=True)
        sb.load_init_inactive_frames(five["init"])
        _drive(torch, sb, five["x"][:16], K)
        if graph:
            sb.capture()
        labs = []
        for t in range(0, 12, K):
            if graph:
                sb.inputs.copy_(x[t:t + K])
                labs.append(sb.step_block().clone())
            else:
                labs.append(sb.step_block(x[t:t + K]).clone())
        out.append(bits([torch.stack(labs), sb.state, sb.features, sb.voiced_len]))
    assert same(out[0], out[1])
    assert np.array_equal(out[0][0].reshape(12, S).numpy(), five["labs"][16:28])


def test_moving_a_stream_to_the_host_class_and_back(torch_cuda, five):
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    from vad_amd.simple_stream import pack_state
    fs, S, K = five["fs"], len(OFFSETS), 8
    sb = SimpleStreamBatch(S, RATE, fs, five["nb"], frames_per_step=K)
    sb.load_init_inactive_frames(five["init"])
    _drive(torch, sb, five["x"][:24], K)
    hosts = [sb.analyser(s) for s in range(S)]
    st = sb.state.cpu().numpy()
    assert pack_state(hosts).tobytes() == st.tobytes()
    for s, h in enumerate(hosts):
        assert h.initialized and h.frame_number == 24 and h.silence == bool(sb.silence[s])
        assert h.temp_buffer == sb.temp_buffer[s].cpu().tolist()
        assert h.noise_pointer == int(sb.noise_pointer[s])
        assert h.energy_thresh == float(sb.energy_thresh[s]) and h.spectral_std_thresh == float(sb.spectral_std_thresh[s])
        assert np.array_equal(h.spectral_energy_bands_thresh, sb.spectral_energy_bands_thresh[s].cpu().numpy())
    back = SimpleStreamBatch.from_analysers(hosts, frames_per_step=K)
    assert back.state.cpu().numpy().tobytes() == st.tobytes()
    labs, states, _ = _drive(torch, back, five["x"][24:], K)
    assert np.array_equal(labs, five["labs"][24:])
    assert states[-1].tobytes() == five["state"].tobytes()
    # a stream moved to the host class mid-sequence goes on as the batch does
    for s in (1, 3):
        rest = hosts[s].classify_frames(list(five["x"][24:, s].cpu().numpy()))
        assert np.array_equal(np.array(rest, np.uint8), five["labs"][24:, s])


def test_block_kernel_ignores_stale_lds(torch_cuda, five, poison):
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    fs, S = five["fs"], len(OFFSETS)
    for K, dt in ((8, torch.float32), (20, torch.int16)):
        sb = SimpleStreamBatch(S, RATE, fs, five["nb"], frames_per_step=K, input_dtype=dt, features=True,
                               voiced=True)
        sb.load_init_inactive_frames(five["init"])
        start = sb.state.clone()
        x = five["x"][8:8 + K].to(dt)

        def run():
            sb.state.copy_(start)
            lab = sb.step_block(x)
            return lab.clone(), sb.features.clone(), sb.state.clone(), sb.voiced_len.clone()

        check(poison, f"simple stream block K={K}", run)


def test_exceptions(torch_cuda, five):
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    fs, nb, S = five["fs"], five["nb"], 2
    sb = SimpleStreamBatch(S, RATE, fs, nb)
    with pytest.raises(Exception, match="Analyser not initialized"):
        sb.step(five["x"][0, :S])
    with pytest.raises(Exception, match="Analyser not initialized"):
        sb.step_block()
    with pytest.raises(Exception, match=f"Expected {nb} initial frames. Got {nb - 1}"):
        sb.load_init_inactive_frames(five["init"][:S, :nb - 1])
    sb.load_init_inactive_frames(five["init"][:S])
    with pytest.raises(Exception, match=f"Wrong frame size. Expected {fs} bytes. Got {fs - 1}"):
        sb.step(five["x"][0, :S, :fs - 1])
    assert sb.step(five["x"][0, :S]).shape == (S,)
    sb.reset()
    assert int(sb.frame_number.sum()) == 0
    with pytest.raises(Exception, match="Analyser not initialized"):
        sb.step(five["x"][0, :S])
