"""SimpleStreamBatch(sessions=True) on the device: per-stream frame counts,
restarts the kernel consumes, and load_init_inactive_frames as a joining
stream's first noise_buf_len frames.

Full counts against the plain batch, in-kernel init against the host-driven
one, the golden traces of the unmodified reference class with streams that
join late, a ragged seeded schedule against the NumPy restatement
(tests/simple_stream_sessions_reference.py) and against one-stream plain
batches, stalled streams, graph replay, stale LDS, independence of streams,
and the class's exceptions.  Streams are cut from tests/golden/simple.npz as
tests/test_gpu_simple_stream.py cuts them: case a 400-sample frames, nb 5,
L 512; case b 512 samples, nb 3; case c 401 samples, nb 4, L 513 (the
two-launch path)."""
import numpy as np
import pytest

import simple_stream_sessions_reference as RS
from test_gpu_lds_independence import bits, check, poison, same  # noqa: F401  (poison: a fixture)

pytestmark = pytest.mark.gpu

RATE = 16000
INIT, NO_HOP = 253, 254
CUTS = {"a": ((0, 60, 150, 290, 420), 60), "b": ((0, 50, 120), 40), "c": ((0, 30, 75), 40)}  # offsets, frames
RAGGED_OFFSETS = (0, 60, 130, 200, 270)   # five streams of up to 328 frames from case a's 605
BLOCKS = 40


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _case(golden, case):
    g = golden("simple")
    fs, nb = int(g[f"{case}_meta"][0]), int(g[f"{case}_meta"][1])
    return fs, nb, g[f"{case}_frames"], g[f"{case}_trace"]


@pytest.fixture(scope="module")
def cuts(torch_cuda, golden):
    """case -> fs, nb, init (S, nb, fs) and x (T, S, fs) fp32 on the device."""
    torch = torch_cuda
    out = {}
    for case, (offs, T) in CUTS.items():
        fs, nb, frames, _ = _case(golden, case)
        f32 = frames.astype(np.float32)
        assert offs[-1] + nb + T <= len(f32)
        init = torch.from_numpy(np.stack([f32[o:o + nb] for o in offs])).cuda()
        x = torch.from_numpy(np.stack([f32[o + nb:o + nb + T] for o in offs], axis=1)).cuda()
        out[case] = dict(fs=fs, nb=nb, init=init, x=x, S=len(offs), T=T)
    return out


def _ints(state, nb):
    return state.view(np.int32)[..., 2 * (6 * nb + 6):]


# ---------------------------------------------------------------------------
# 1. full counts, no restart, init_left 0: the plain batch, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_full_counts_equal_the_plain_batch(torch_cuda, cuts, K, dtype):
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    c = cuts["a"]
    dt = getattr(torch, dtype)
    x, init = c["x"].to(dt), c["init"].to(dt)
    assert torch.equal(x.float(), c["x"])                      # integer-valued samples: the cast is exact
    pair = []
    for sessions in (False, True):
        sb = SimpleStreamBatch(c["S"], RATE, c["fs"], c["nb"], frames_per_step=K, input_dtype=dt, features=True,
                               voiced=True, sessions=sessions)
        sb.load_init_inactive_frames(init)
        pair.append(sb)
    plain, sess = pair
    assert sess.initialized and int(sess.init_left.abs().sum()) == 0 and int(sess.frame_counts.min()) == K
    seen = set()
    for t in range(0, c["T"], K):
        blk = x[t:t + K]
        k = blk.shape[0]
        got = []
        for sb in pair:
            sb.voiced.fill_(77)
            lab = sb.step(blk[0]).unsqueeze(0) if K == 1 else sb.step_block(blk)
            got.append(bits([lab, sb.state, sb.features[:k], sb.voiced, sb.voiced_len]))
        assert same(got[0], got[1]), t
        seen |= set(got[1][0].unique().tolist())
        seen.add(("short", k < K))
    assert seen == {0, 1, ("short", False)} | ({("short", True)} if c["T"] % K else set())
    assert int(sess.init_left.abs().sum()) == 0 and int(sess.restart.sum()) == 0
    # from_analysers sets init_left too
    back = SimpleStreamBatch.from_analysers([plain.analyser(s) for s in range(c["S"])], frames_per_step=K,
                                            sessions=True)
    assert back.initialized and int(back.init_left.abs().sum()) == 0
    assert back.state.cpu().numpy().tobytes() == plain.state.cpu().numpy().tobytes()


# ---------------------------------------------------------------------------
# 2. in-kernel init == load_init_inactive_frames
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_in_kernel_init_equals_host_driven_init(torch_cuda, cuts, case, K):
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    c = cuts[case]
    S, nb, T = c["S"], c["nb"], c["T"]
    sess = SimpleStreamBatch(S, RATE, c["fs"], nb, frames_per_step=K, sessions=True)
    assert sess.one_kernel == (case != "c")
    assert sess.initialized and sess.init_left.tolist() == [nb] * S and not bool(sess.state.any())
    plain = SimpleStreamBatch(S, RATE, c["fs"], nb, frames_per_step=K)
    plain.load_init_inactive_frames(c["init"])
    full = torch.cat([c["init"].transpose(0, 1), c["x"]])       # (nb + T, S, fs): init ++ frames
    labs, at = [], 0                                            # at: frames the plain batch has had
    for t in range(0, nb + T, K):
        blk = full[t:t + K]
        lab = sess.step_block(blk).clone()
        labs.append(lab)
        end = t + blk.shape[0] - nb                             # post-init frames the sessions batch has had
        if end <= 0:
            assert int(sess.init_left[0]) == -end and bool((lab == INIT).all())
            continue
        want = plain.step_block(c["x"][at:end]).clone()         # a short block where init ended mid-block
        assert torch.equal(lab[blk.shape[0] - (end - at):], want), t
        assert torch.equal(sess.state, plain.state), t          # after every block, bit for bit
        assert sess.init_left.tolist() == [0] * S
        at = end
    labs = torch.cat(labs).cpu().numpy()
    assert labs.shape == (nb + T, S) and (labs[:nb] == INIT).all() and labs[nb:].max() <= 1
    assert at == T
    if case == "a":
        assert {0, 1} <= set(labs[nb:].ravel().tolist())
    if K == 3 and case == "a":
        assert nb % K == 2        # init ends at row 1 of the second block: classified rows in that same block
    assert all(sess.analyser(s).initialized for s in range(S))


# ---------------------------------------------------------------------------
# 3. the unmodified reference's trace, streams that join late
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case,K", [("a", 8), ("b", 7), ("c", 4)])
def test_golden_trace_with_late_joins(torch_cuda, golden, case, K):
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    fs, nb, frames, ref = _case(golden, case)
    S, n = 3, len(ref)
    total = nb + n
    x = torch.from_numpy(frames.astype(np.float32)).cuda()
    pad = torch.zeros((K * (S + 1), fs), dtype=torch.float32, device="cuda")
    xp = torch.cat([x, pad])
    sb = SimpleStreamBatch(S, RATE, fs, nb, frames_per_step=K, sessions=True)
    n_blocks = (total + K - 1) // K + S - 1
    labs, states = [], []
    for b in range(n_blocks):
        # stream j joins j blocks late: nothing before, then a restart with its first frames
        starts = [max(b - j, 0) * K for j in range(S)]
        blk = torch.stack([xp[st:st + K] for st in starts], dim=1)
        counts = [0 if b < j else max(min(K, total - (b - j) * K), 0) for j in range(S)]
        restart = [1 if b == j else 0 for j in range(S)]
        lab = sb.step_block(blk, torch.tensor(counts, dtype=torch.int32, device="cuda"),
                            torch.tensor(restart, dtype=torch.uint8, device="cuda"))
        labs.append(lab.clone())
        states.append(sb.state.clone())
    assert int(sb.restart.sum()) == 0
    labs = torch.stack(labs).cpu().numpy()                       # (blocks, K, S)
    states = torch.stack(states).cpu().numpy()                   # (blocks, S, doubles)
    for j in range(S):
        col = labs[j:, :, j].reshape(-1)
        assert (labs[:j, :, j] == NO_HOP).all()
        assert (col[:nb] == INIT).all()
        assert np.array_equal(col[nb:total], ref[:, 0].astype(np.uint8))
        assert (col[total:] == NO_HOP).all()
        for b in range(j, n_blocks):
            e = min((b - j + 1) * K, total) - nb - 1             # the trace row this state follows
            if e < 0:
                continue
            st = states[b, j]
            w = _ints(st, nb)
            assert w[1] == ref[e, 1] and w[3] == e + 1, (j, b)
            # test_gpu_simple_stream.py::test_golden_traces' tolerance
            assert np.allclose(st[6 * nb:6 * nb + 6], ref[e, 2:], rtol=1e-10, atol=0), (j, b)


# ---------------------------------------------------------------------------
# 4. / 8. a ragged schedule
# ---------------------------------------------------------------------------
def _schedule(K, nb):
    """counts (BLOCKS, S) and restarts (BLOCKS, S), seeded.  Stream 4 never
    restarts; stream 0 restarts with a count of 0; stream 1 restarts while it
    is still in init, in two consecutive blocks."""
    rng = np.random.RandomState(1234 + K)
    S = len(RAGGED_OFFSETS)
    counts = rng.randint(0, K + 1, size=(BLOCKS, S))
    over = rng.rand(BLOCKS, S)
    counts[over < 0.08] = K + 3                                  # clamped to K
    counts[over > 0.94] = -2                                     # clamped to 0
    restarts = (rng.rand(BLOCKS, S) < 0.1).astype(np.uint8)
    restarts[:, 4] = 0
    restarts[20, 2] = restarts[30, 3] = 1
    restarts[5, 0], counts[5, 0] = 1, 0
    restarts[9:13, 1] = 0
    restarts[10, 1], counts[10, 1] = 1, min(2, nb - 1)           # leaves init_left > 0 ...
    restarts[11, 1], counts[11, 1] = 1, K                        # ... and the next block restarts again
    assert (counts > K).any() and (counts < 0).any() and nb > 2
    return counts, restarts


def _run_schedule(torch, K, c, frames, counts, restarts, streams):
    """A sessions batch of the given streams over the schedule.  Each block
    holds every stream's next K frames; the stream consumes its count of them."""
    from vad_amd import SimpleStreamBatch
    S = len(streams)
    sb = SimpleStreamBatch(S, RATE, c["fs"], c["nb"], frames_per_step=K, features=True, voiced=True, sessions=True)
    pos = [RAGGED_OFFSETS[s] for s in streams]
    out = dict(labs=[], feats=[], voiced=[], taken=[])
    for b in range(BLOCKS):
        blk = torch.stack([frames[p:p + K] for p in pos], dim=1)
        sb.voiced.fill_(-3.0)
        lab = sb.step_block(blk, torch.from_numpy(counts[b, streams].astype(np.int32)).cuda(),
                            torch.from_numpy(np.ascontiguousarray(restarts[b, streams])).cuda())
        n = np.clip(counts[b, streams], 0, K)
        out["taken"].append([(pos[i], int(n[i])) for i in range(S)])
        pos = [p + int(k) for p, k in zip(pos, n)]
        out["labs"].append(lab.clone())
        out["feats"].append(sb.features.clone())
        out["voiced"].append((sb.voiced.clone(), sb.voiced_len.clone()))
    torch.cuda.synchronize()
    out["labs"] = torch.stack(out["labs"]).cpu().numpy()
    out["feats"] = torch.stack(out["feats"]).cpu().numpy()
    out["voiced"] = [(v.cpu().numpy(), n.cpu().numpy()) for v, n in out["voiced"]]
    out["state"] = sb.state.cpu().numpy()
    out["init_left"] = sb.init_left.cpu().numpy()
    out["restart"] = sb.restart.cpu().numpy()
    return out


@pytest.fixture(scope="module", params=[4, 8])
def ragged(request, torch_cuda, golden, cuts):
    torch = torch_cuda
    K = request.param
    c = cuts["a"]
    _, _, frames, _ = _case(golden, "a")
    assert RAGGED_OFFSETS[-1] + BLOCKS * K + K <= len(frames)
    frames = torch.from_numpy(frames.astype(np.float32)).cuda()
    counts, restarts = _schedule(K, c["nb"])
    S = len(RAGGED_OFFSETS)
    run = _run_schedule(torch, K, c, frames, counts, restarts, list(range(S)))
    return dict(K=K, c=c, frames=frames, counts=counts, restarts=restarts, run=run, S=S)


def test_ragged_schedule_equals_the_restatement(ragged):
    K, c, run, S = ragged["K"], ragged["c"], ragged["run"], ragged["S"]
    nb, fs = c["nb"], c["fs"]
    ref = RS.RefSessions(S, nb)
    seen = set()
    for b in range(BLOCKS):
        want, voiced = ref.block(run["feats"][b], ragged["counts"][b], ragged["restarts"][b])
        assert np.array_equal(run["labs"][b], want), b
        v, n = run["voiced"][b]
        for s in range(S):
            assert n[s] == len(voiced[s]) * fs
            seen |= set(want[:, s].tolist())
    assert seen == {0, 1, INIT, NO_HOP}
    for s in range(S):
        assert run["state"][s].tobytes() == ref.packed(s).tobytes(), s       # bit for bit: noise_buf_len < 8
        assert run["init_left"][s] == ref.init_left(s)
    assert not run["restart"].any()
    assert ref.sessions[4] == 0 and min(ref.sessions[:4]) >= 1


def test_ragged_schedule_equals_one_stream_plain_batches(torch_cuda, ragged):
    """Per stream and session: a fresh plain batch loaded with the session's
    first nb frames and fed the rest gives the same labels, voiced samples and
    (for the stream's last session) final state."""
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    K, c, run, S, frames = ragged["K"], ragged["c"], ragged["run"], ragged["S"], ragged["frames"]
    nb, fs = c["nb"], c["fs"]
    compared = 0
    for s in range(S):
        # the stream's sessions: per session the frame positions, labels and voiced samples, in order
        sessions = [dict(pos=[], labs=[], voiced=[])]
        for b in range(BLOCKS):
            if ragged["restarts"][b, s]:
                sessions.append(dict(pos=[], labs=[], voiced=[]))
            p, n = run["taken"][b][s]
            cur = sessions[-1]
            cur["pos"] += list(range(p, p + n))
            cur["labs"] += run["labs"][b, :n, s].tolist()
            assert (run["labs"][b, n:, s] == NO_HOP).all()
            v, vl = run["voiced"][b]
            cur["voiced"].append(v[s, :vl[s]])
            assert (v[s, vl[s]:] == -3.0).all()                  # nothing past voiced_len is written
        for i, se in enumerate(sessions):
            n_init = min(nb, len(se["pos"]))
            assert se["labs"][:n_init] == [INIT] * n_init and INIT not in se["labs"][n_init:]
            if len(se["pos"]) < nb:                              # never initialised: nothing was classified
                assert sum(len(v) for v in se["voiced"]) == 0
                continue
            x = frames[se["pos"]]                                # consecutive frames of the supply
            pb = SimpleStreamBatch(1, RATE, fs, nb, frames_per_step=8, voiced=True)
            pb.load_init_inactive_frames(x[:nb].unsqueeze(0))
            labs, voiced = [], []
            for t in range(nb, len(x), 8):
                lab = pb.step_block(x[t:t + 8].unsqueeze(1))
                labs += lab[:, 0].tolist()
                voiced.append(pb.voiced[0, :int(pb.voiced_len[0])].cpu().numpy())
            assert labs == se["labs"][nb:], (s, i)
            got_v = np.concatenate(se["voiced"]) if se["voiced"] else np.zeros(0, np.float32)
            want_v = np.concatenate(voiced) if voiced else np.zeros(0, np.float32)
            assert got_v.tobytes() == want_v.tobytes(), (s, i)
            if i == len(sessions) - 1:
                assert run["state"][s].tobytes() == pb.state[0].cpu().numpy().tobytes(), s
                assert run["init_left"][s] == 0
            compared += 1
    assert compared >= S


def test_streams_are_independent(torch_cuda, ragged):
    """Any one stream's column equals a one-stream sessions batch on its schedule."""
    torch = torch_cuda
    K, c, run = ragged["K"], ragged["c"], ragged["run"]
    for s in range(ragged["S"]):
        one = _run_schedule(torch, K, c, ragged["frames"], ragged["counts"], ragged["restarts"], [s])
        assert np.array_equal(one["labs"][:, :, 0], run["labs"][:, :, s]), s
        assert one["state"][0].tobytes() == run["state"][s].tobytes(), s
        assert one["init_left"][0] == run["init_left"][s]
        for b in range(BLOCKS):
            n = one["voiced"][b][1][0]
            assert n == run["voiced"][b][1][s]
            assert one["voiced"][b][0][0, :n].tobytes() == run["voiced"][b][0][s, :n].tobytes()
            k = run["taken"][b][s][1]
            assert one["feats"][b, :k, 0].tobytes() == run["feats"][b, :k, s].tobytes()


# ---------------------------------------------------------------------------
# 5. a stalled stream keeps every byte
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "c"])
def test_stalled_stream_keeps_every_byte(torch_cuda, cuts, case):
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    c = cuts[case]
    K, S, nb = 4, 3, c["nb"]
    x = c["x"][:, :S]
    sb = SimpleStreamBatch(S, RATE, c["fs"], nb, frames_per_step=K, features=True, voiced=True, sessions=True)
    one_kernel = sb.one_kernel

    def step(t, counts):
        sb.features.fill_(-99.0)
        sb.voiced_len.fill_(-1)
        lab = sb.step_block(x[t:t + K], torch.tensor(counts, dtype=torch.int32, device="cuda")).cpu().numpy()
        return lab, sb.features.cpu().numpy(), sb.state.cpu().numpy(), sb.init_left.cpu().numpy(), \
            sb.voiced_len.cpu().numpy()

    lab, f, st0, left0, vl = step(0, [nb - 1, 2, 4])
    assert left0.tolist() == [1, nb - 2, max(nb - 4, 0)]
    assert (lab[:nb - 1, 0] == INIT).all() and (lab[nb - 1:, 0] == NO_HOP).all()
    assert st0[0, :6 * (nb - 1)].all() and not st0[0, 6 * (nb - 1):].any()   # mid-init: noise rows so far, zeros
    # mid-init: streams 0 and 1 stall
    lab, f, st1, left1, vl = step(4, [0, 0, 4])
    for s in (0, 1):
        assert st1[s].tobytes() == st0[s].tobytes() and left1[s] == left0[s]
        assert (lab[:, s] == NO_HOP).all() and vl[s] == 0
        if one_kernel:
            assert (f[:, s] == -99.0).all()
    assert (f[:, 2] != -99.0).all() and left1[2] == 0 and st1[2].tobytes() != st0[2].tobytes()
    # all finish their init
    lab, f, st2, left2, vl = step(8, [4, 4, 4])
    assert left2.tolist() == [0, 0, 0] and lab[0, 0] == INIT and lab[1:, 0].max() <= 1
    # after init: stream 0 stalls, stream 2 takes two of the four frames
    lab, f, st3, left3, vl = step(12, [0, 4, 2])
    assert st3[0].tobytes() == st2[0].tobytes() and left3.tolist() == [0, 0, 0]
    assert (lab[:, 0] == NO_HOP).all() and vl[0] == 0
    assert lab[:2, 2].max() <= 1 and (lab[2:, 2] == NO_HOP).all()
    assert vl[2] == int((lab[:2, 2] == 1).sum()) * c["fs"] and vl[1] == int((lab[:, 1] == 1).sum()) * c["fs"]
    assert st3[1].tobytes() != st2[1].tobytes() and st3[2].tobytes() != st2[2].tobytes()
    if one_kernel:
        assert (f[:, 0] == -99.0).all() and (f[2:, 2] == -99.0).all() and (f[:2, 2] != -99.0).all()
    w = _ints(st3, nb)
    assert w[:, 3].tolist() == [3, 2 + 4 + 4 - nb, 4 + 4 + 4 + 2 - nb]       # frame_number: classified frames
    # a restart with no frame: the record zero, init_left nb, the flag consumed
    sb.step_block(x[16:20], torch.tensor([0, 0, 0], dtype=torch.int32, device="cuda"),
                  torch.tensor([0, 1, 0], dtype=torch.uint8, device="cuda"))
    assert not bool(sb.state[1].any()) and sb.init_left.tolist() == [0, nb, 0] and sb.restart.tolist() == [0, 0, 0]
    assert sb.state[0].cpu().numpy().tobytes() == st3[0].tobytes()
    assert not sb.analyser(1).initialized and sb.analyser(0).initialized


# ---------------------------------------------------------------------------
# 6. graph replay
# ---------------------------------------------------------------------------
def test_graph_replay_restarts_once_and_honours_counts(torch_cuda, cuts):
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    c = cuts["a"]
    K, S, nb = 4, c["S"], c["nb"]
    x = c["x"]
    counts = [[4] * S, [4, 0, 2, 4, 3], [4, 4, 4, 1, 0]]
    out = []
    for graph in (False, True):
        sb = SimpleStreamBatch(S, RATE, c["fs"], nb, frames_per_step=K, features=True, voiced=True, sessions=True)
        for t in (0, 4, 8):
            sb.step_block(x[t:t + K])                 # in-kernel init (5 frames), then 7 classified
        assert sb.init_left.tolist() == [0] * S
        sb.restart[2] = 1                             # set once, before the capture
        if graph:
            before = bits([sb.state, sb.init_left, sb.restart, sb.frame_counts])
            sb.capture()                              # the warm-up consumed the flag; capture() put it back
            assert same(bits([sb.state, sb.init_left, sb.restart, sb.frame_counts]), before)
        labs = []
        for i, t in enumerate((12, 16, 20)):
            sb.frame_counts.copy_(torch.tensor(counts[i], dtype=torch.int32, device="cuda"))
            sb.voiced.fill_(5.0)
            if graph:
                sb.inputs.copy_(x[t:t + K])
                labs.append(sb.step_block().clone())
            else:
                labs.append(sb.step_block(x[t:t + K]).clone())
            if i == 0:
                assert int(sb.restart[2]) == 0 and int(sb.init_left[2]) == nb - 4
        out.append(bits([torch.stack(labs), sb.state, sb.features, sb.voiced, sb.voiced_len, sb.init_left,
                         sb.restart]))
        lab = torch.stack(labs).cpu().numpy()
        # stream 2 restarted once: 4 + 2 + 4 frames, nb of them init frames
        got = np.concatenate([lab[0, :, 2], lab[1, :2, 2], lab[2, :, 2]])
        assert (got[:nb] == INIT).all() and got[nb:].max() <= 1 and int(sb.frame_number[2]) == 10 - nb
        assert (lab[1, :, 1] == NO_HOP).all() and (lab[1, 2:, 2] == NO_HOP).all() and (lab[2, 1:, 3] == NO_HOP).all()
        assert sb.frame_number.tolist() == [7 + 12, 7 + 8, 10 - nb, 7 + 9, 7 + 7]
    assert same(out[0], out[1])


# ---------------------------------------------------------------------------
# 7. stale LDS
# ---------------------------------------------------------------------------
def test_sessions_block_kernel_ignores_stale_lds(torch_cuda, cuts, poison):
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    c = cuts["a"]
    S = c["S"]
    for K, dt in ((8, torch.float32), (20, torch.int16)):
        sb = SimpleStreamBatch(S, RATE, c["fs"], c["nb"], frames_per_step=K, input_dtype=dt, features=True,
                               voiced=True, sessions=True)
        sb.step_block(c["x"][:K].to(dt))                             # every stream through its init
        start = sb.state.clone()
        x = c["x"][K:2 * K].to(dt)
        counts = torch.tensor([K, 3, 0, K - 1, K], dtype=torch.int32, device="cuda")
        restart = torch.tensor([0, 0, 0, 1, 1], dtype=torch.uint8, device="cuda")   # restarted: zeros, not the LDS
        left = torch.tensor([0, 0, 0, 0, 0], dtype=torch.int32, device="cuda")

        def run():
            sb.state.copy_(start)
            sb.init_left.copy_(left)
            sb.features.zero_()
            lab = sb.step_block(x, counts, restart)
            return lab.clone(), sb.features.clone(), sb.state.clone(), sb.voiced_len.clone(), sb.init_left.clone()

        check(poison, f"simple stream sessions block K={K}", run)


# ---------------------------------------------------------------------------
# the class's exceptions
# ---------------------------------------------------------------------------
def test_value_errors_and_reset(torch_cuda, cuts):
    torch = torch_cuda
    from vad_amd import SimpleStreamBatch
    from vad_amd import simple_stream as SS
    assert SS.LABEL_INIT == INIT and SS.LABEL_NO_HOP == NO_HOP
    c = cuts["a"]
    S, nb, fs = 2, c["nb"], c["fs"]
    x = c["x"][:, :S]
    cnt = torch.ones(S, dtype=torch.int32, device="cuda")
    rst = torch.zeros(S, dtype=torch.uint8, device="cuda")
    plain = SimpleStreamBatch(S, RATE, fs, nb)
    plain.load_init_inactive_frames(c["init"][:S])
    for kw in (dict(frame_counts=cnt), dict(restart=rst)):
        with pytest.raises(ValueError, match="sessions=True"):
            plain.step_block(x[:1], **kw)
        with pytest.raises(ValueError, match="sessions=True"):
            plain.step(x[0], **kw)
    sb = SimpleStreamBatch(S, RATE, fs, nb, sessions=True)
    assert sb.initialized
    for bad in (cnt.cpu(), cnt.long(), torch.ones(S + 1, dtype=torch.int32, device="cuda"), [1, 1]):
        with pytest.raises(ValueError, match="frame_counts must be a CUDA int32 tensor"):
            sb.step_block(x[:1], frame_counts=bad)
    for bad in (rst.cpu(), rst.bool(), torch.zeros((S, 1), dtype=torch.uint8, device="cuda")):
        with pytest.raises(ValueError, match="restart must be a CUDA uint8 tensor"):
            sb.step(x[0], restart=bad)
    assert sb.init_left.tolist() == [nb, nb]                      # a refused call consumed nothing
    lab = sb.step(x[0], frame_counts=cnt, restart=rst)            # never "Analyser not initialized"
    assert lab.tolist() == [INIT, INIT] and sb.init_left.tolist() == [nb - 1, nb - 1]
    assert not sb.analyser(0).initialized
    sb.frame_counts.fill_(0)
    sb.reset()
    assert sb.initialized and sb.init_left.tolist() == [nb, nb] and sb.frame_counts.tolist() == [1, 1]
    assert not bool(sb.state.any()) and sb.restart.tolist() == [0, 0]
    sb.load_init_inactive_frames(c["init"][:S])                   # still works: all streams, init_left 0
    assert sb.init_left.tolist() == [0, 0] and sb.analyser(1).initialized
    assert torch.equal(sb.state, plain.state)
