"""Every block shape of the hop kernels: 1, 2, 4, 8 and 16 waves per block,
for the FFN and the tree (walked from LDS and from global memory), in every
form -- plain, scores, denoise, sessions, sessions + denoise -- and both input
types, including the tree tables large enough that the LDS cap of the launch
rule halves a multi-wave block.

Streams are independent, so stream s of a batch of thousands, fed pattern
s % 7 of seven distinct inputs, must equal row s % 7 of a seven-stream batch
bit for bit: labels, scores and every state tensor, after every step.  The
seven-row expectation comes from the helpers the forms' own files pin against
the oracle and the host models (tests/test_gpu_stream_scores.py,
test_gpu_stream_denoise.py, test_gpu_stream_sessions.py), one hop per step.
Seven is coprime to every wave count: the pattern never lines up with the wave
index.  Stream counts follow the device's compute units, and every case
asserts through StreamBatch.block_waves (vad_stream_hop_block_waves, the
launcher's own rule) that it ran the shape it was written for.  No tolerance
anywhere."""
import functools

import numpy as np
import pytest

from oracle import vad_oracle as O

import stream_sessions_reference as SR
import stream_tree_reference as TR
from test_gpu_stream_denoise import noise_frames
from test_gpu_stream_scores import H, audio, batch, cuda, ffn, poison, torch_cuda, tree_with_scores, with_counts  # noqa: F401
from test_gpu_stream_sessions import expected, make, same

pytestmark = pytest.mark.gpu

P, HOPS, BLOCKS, LOADED = 7, 12, 10, 2
# Seeds under which the fp64 oracle gives both classifiers both classes, with
# margin, on the seven patterns (bl13: 34 / 5 of the 49 windows of the hops,
# the fixture tree 26 / 20; over the sessions' windows at K = 1 and K = 2
# bl13 8 / 2 and 36 / 3, the tree 5 / 4 and 34 / 7).  Every case asserts it.
AUDIO_SEED, SESSION_SEED = 2100, 6400
STATE, DN_STATE = SR.STATE, SR.DN_STATE
FORMS = {  # the StreamBatch options of a form
    "plain": {},
    "scores": dict(scores=True),
    "denoise": dict(scores=True, denoise=True),
    "sessions": dict(scores=True, sessions=True),
    "sessions_denoise": dict(scores=True, sessions=True, denoise=True),
}
CLASSIFIERS = ("bl13", "tree", "tree_global")
WAVES = (1, 2, 4, 8, 16)


def matrix():
    """Every (classifier, form) pair at every wave count.  1 and 2 waves need
    a launch of several hops (a one-hop launch starts at 4); above that K and
    the input type alternate, so that every form meets both of each."""
    cases = []
    for ci, c in enumerate(CLASSIFIERS):
        for fi, f in enumerate(FORMS):
            p = ci * len(FORMS) + fi
            for j, w in enumerate(WAVES):
                K = 2 if w < 4 or (p + j) % 2 else 1
                dtype = ("float32", "int16")[(j + p // 2) % 2]
                cases.append((c, f, w, K, dtype))
    return cases


MATRIX = matrix()


def n_streams(n_cu, w, K):
    """The smallest stream count that gives w waves per block (15 for one
    wave: two rounds of the patterns and one more): w n_cu / 2 + 1 with blocks
    of hops, 4 waves up to 4 n_cu streams with one-hop launches.  The last
    block holds one live stream and w - 1 waves past n_streams."""
    if w == 1:
        return 2 * P + 1
    if K == 1 and w == 4:
        return n_cu + 1
    return (w // 2) * n_cu + 1


def test_the_matrix_covers_every_shape():
    for c in CLASSIFIERS:
        for f in FORMS:
            assert {w for cc, ff, w, _, _ in MATRIX if (cc, ff) == (c, f)} == set(WAVES), (c, f)
    for f in FORMS:
        assert {K for _, ff, _, K, _ in MATRIX if ff == f} == {1, 2}, f
        assert {d for _, ff, _, _, d in MATRIX if ff == f} == {"float32", "int16"}, f
    assert all(K == 2 for _, _, w, K, _ in MATRIX if w < 4)


# ---------------------------------------------------------------------------
# the seven-row expectations
# ---------------------------------------------------------------------------
def cu_count(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def classifier(key):
    """"bl13", "tree", or ("comb", w): the comb whose table leaves w waves."""
    if key == "bl13":
        return ffn("bl13")
    return tree_with_scores() if key == "tree" else comb(key[1])[0]


def snapshot(sb):
    names = STATE + (DN_STATE if sb.denoise else ())
    return dict(labels=sb.label_block.clone(), scores=sb.score_block.clone() if sb.scores else None,
                state={k: getattr(sb, k).clone() for k in names})


@functools.lru_cache(maxsize=None)
def pattern_run(key, form, dtype, noise_class=0):
    """The P patterns through a P-stream batch without sessions, one hop per
    step: a snapshot per hop (labels and scores (1, P), the state after the
    hop).  Computed once per key, never written afterwards."""
    import torch
    dt = getattr(torch, dtype)
    carry, hops = audio(P, HOPS, seed=AUDIO_SEED)
    kw = dict(FORMS[form])
    if kw.get("denoise"):
        kw.update(noise_class=noise_class, noise_update=True)
    sb = batch(torch, P, classifier(key), carry, input_dtype=dt, **kw)
    assert sb.K == 1
    if sb.denoise:
        sb.load_noise(cuda(noise_frames(P, LOADED)).to(dt))
    dh = cuda(hops).to(dt)
    rec = []
    for t in range(HOPS):
        sb.step(dh[t])
        rec.append(snapshot(sb))
    return rec


def most_common(labels):
    import torch
    return int(torch.bincount(labels.flatten().long()).argmax())


def pattern_run_for(key, form, dtype):
    """pattern_run with a noise class that occurs: the class most patterns get
    at their first window (which no noise class has influenced yet), so that
    hop pushes a noise row."""
    if not FORMS[form].get("denoise"):
        return pattern_run(key, form, dtype)
    return pattern_run(key, form, dtype, most_common(pattern_run(key, form, dtype)[5]["labels"]))


@functools.lru_cache(maxsize=None)
def session_inputs(K, dtype):
    """The schedule of the sessions file for P streams and (BLOCKS, K, P, hop)
    samples cut from the oracle's synthetic clips: the noise floor of that
    file's own samples gives the fixture tree one class only."""
    import torch
    counts, restart = SR.make_schedule(P, K, BLOCKS, seed=300 + K)
    clips = np.stack([O.synth_clip(H * BLOCKS * K, seed=SESSION_SEED + 10 * K + s) for s in range(P)])
    blocks = np.ascontiguousarray(clips.reshape(P, BLOCKS, K, H).transpose(1, 2, 0, 3))
    assert np.array_equal(blocks, blocks.astype(np.int16))
    return counts, restart, cuda(blocks).to(getattr(torch, dtype))


@functools.lru_cache(maxsize=None)
def session_run(key, form, K, dtype, noise_class=0):
    """The sessions file's expectation (the plain kernels, session by session,
    one hop per step) of the P-stream schedule.  Computed once per key."""
    import torch
    counts, restart, blocks = session_inputs(K, dtype)
    denoise = bool(FORMS[form].get("denoise"))
    kw = dict(noise_class=noise_class) if denoise else {}
    return expected(torch, classifier(key), blocks, counts, restart, K, dtype, True, denoise, **kw)


def session_run_for(key, form, K, dtype):
    """session_run and its noise class: as pattern_run_for, the class most
    sessions get at their first window."""
    import torch
    exp = session_run(key, form, K, dtype)
    if not FORMS[form].get("denoise"):
        return exp, None
    first = torch.stack([exp.labels[5][i] for i, r in enumerate(exp.ses.rows) if len(r) > 5])
    noise_class = most_common(first)
    return session_run(key, form, K, dtype, noise_class), noise_class


# ---------------------------------------------------------------------------
# what makes a case worth its time
# ---------------------------------------------------------------------------
def assert_rows_differ(rows):
    """rows[s]: the byte strings of pattern s's labels and state."""
    assert len(rows) == P and len(set(rows)) == P, "two patterns gave the same labels and state"


def assert_pushes(hist, live):
    """hist (T + 1, rows) noise counts before the first hop and after every
    hop, live (T, rows) the hops that are a row's own: some hop pushed a noise
    row, and some push landed below five rows (no eviction)."""
    grew = (hist[1:] > hist[:-1]) & live
    assert grew.any() and (grew & (hist[1:] < 5)).any(), hist.T.tolist()


def check_pattern_run(rec, denoise):
    import torch
    lab = torch.cat([r["labels"] for r in rec]).cpu().numpy()  # (HOPS, P)
    assert (lab[:5] == 255).all() and set(np.unique(lab[5:]).tolist()) == {0, 1}, np.unique(lab).tolist()
    last = rec[-1]["state"]
    assert_rows_differ([lab[:, s].tobytes() + b"".join(last[k][s].cpu().numpy().tobytes() for k in STATE)
                        for s in range(P)])
    if denoise:
        hist = np.stack([np.full(P, LOADED)] + [r["state"]["noise_count"].cpu().numpy() for r in rec])
        assert_pushes(hist, np.ones((HOPS, P), bool))


def check_session_run(exp, counts, restart, K, denoise):
    import torch
    n = SR.clamp(counts, K)
    assert restart.any() and (n == 0).any() and ((restart != 0) & (n == 0)).any()  # a restart on a block of no hops
    assert (counts > K).any() and (counts < 0).any() and (n[:, 1] == 0).all()  # clamped counts, the stalled stream
    T, rows = exp.ses.longest, exp.ses.rows
    lab = torch.stack(exp.labels).cpu().numpy()  # (T, sessions)
    live = np.array([[t < len(r) for r in rows] for t in range(T)])
    assert (lab[:5] == 255).all() and (lab[5:] != 255).all() and set(np.unique(lab[5:][live[5:]]).tolist()) == {0, 1}
    blocks = [exp.block(b) for b in range(BLOCKS)]
    assert_rows_differ([b"".join(lb[:, s].cpu().numpy().tobytes() for lb, _, _ in blocks)
                        + b"".join(blocks[-1][2][k][s].cpu().numpy().tobytes() for k in STATE) for s in range(P)])
    if denoise:
        hist = np.stack([snap["noise_count"].cpu().numpy() for snap in exp.snap])
        assert_pushes(hist, live)
    return blocks


# ---------------------------------------------------------------------------
# the big batch
# ---------------------------------------------------------------------------
def run_case(torch, key, form, S, K, dtype, walk="auto", waves=None, fill=None):
    """S streams, stream s on pattern s % P, compared with the P-row
    expectation after every step.  fill: the poison fixture, launched with each
    hostile value before every launch.  Returns the labels and scores of every
    step and the state after the last."""
    dt = getattr(torch, dtype)
    clf = classifier(key)
    opts = dict(FORMS[form])
    denoise, sessions = bool(opts.get("denoise")), bool(opts.pop("sessions", False))
    if key != "bl13":
        opts["tree_walk"] = walk
    idx = torch.arange(S, device="cuda") % P
    idx_host = np.arange(S) % P
    seen = []

    def foul():
        if fill is not None:
            for v in (1e30, -1e30, float("nan")):
                fill(v)

    def compare(sb, lab, sc, state, where):
        assert torch.equal(sb.label_block, lab[:, idx]), (where, "labels")
        if sb.scores:
            assert same(sb.score_block, sc[:, idx]), (where, "scores")
        bad = [k for k, v in state.items() if not same(getattr(sb, k), v[idx])]
        assert not bad, (where, bad)
        seen.extend([sb.label_block.clone()] + ([sb.score_block.clone()] if sb.scores else []))

    if sessions:
        exp, noise_class = session_run_for(key, form, K, dtype)
        counts, restart, blocks = session_inputs(K, dtype)
        want = check_session_run(exp, counts, restart, K, denoise)
        kw = dict(noise_class=noise_class) if denoise else {}
        if "tree_walk" in opts:
            kw["tree_walk"] = opts["tree_walk"]
        sb = make(torch, S, clf, K, dtype, True, denoise, sessions=True, **kw)
        assert waves is None or sb.block_waves == waves, (sb.block_waves, waves)
        rows = torch.arange(K, device="cuda")[:, None]
        for b in range(BLOCKS):
            c, r = cuda(counts[b])[idx], cuda(restart[b])[idx]
            blk = blocks[b][:, idx]
            foul()
            if K == 1:
                sb.step(blk[0], hop_counts=c, restart=r)
            else:
                sb.step_block(blk, hop_counts=c, restart=r)
            compare(sb, *want[b], (b,))
            assert not bool(sb.restart.any()), (b, "restart not consumed")
            past = rows >= c.clamp(0, K)[None, :]  # rows a stream has no hop in
            assert bool((sb.label_block[past] == SR.NO_HOP).all()) and bool(torch.isnan(sb.score_block[past]).all()), b
        assert "sessions" in sb._hop_name
        return seen + [getattr(sb, k).clone() for k in want[-1][2]]

    rec = pattern_run_for(key, form, dtype)
    check_pattern_run(rec, denoise)
    carry, hops = audio(P, HOPS, seed=AUDIO_SEED)
    if denoise:
        opts.update(noise_class=most_common(rec[5]["labels"]), noise_update=True)
    sb = batch(torch, S, clf, carry[idx_host], hops_per_step=K, input_dtype=dt, **opts)
    assert waves is None or sb.block_waves == waves, (sb.block_waves, waves)
    if denoise:
        foul()
        sb.load_noise(cuda(noise_frames(P, LOADED)).to(dt)[idx])
    dh = cuda(hops).to(dt)[:, idx]
    for t0 in range(0, HOPS, K):
        foul()
        if K == 1:
            sb.step(dh[t0])
        else:
            sb.step_block(dh[t0:t0 + K])
        lab = torch.cat([rec[t0 + k]["labels"] for k in range(K)])
        sc = torch.cat([rec[t0 + k]["scores"] for k in range(K)]) if sb.scores else None
        compare(sb, lab, sc, rec[t0 + K - 1]["state"], (t0,))
    return seen + [getattr(sb, k).clone() for k in rec[-1]["state"]]



# ---------------------------------------------------------------------------
# 1. every (classifier, form) pair at every wave count
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,form,w,K,dtype", MATRIX, ids=["-".join(map(str, c)) for c in MATRIX])
def test_row_equals_pattern(torch_cuda, name, form, w, K, dtype):
    torch = torch_cuda
    key, walk = ("tree", "global") if name == "tree_global" else (name, "auto")
    run_case(torch, key, form, n_streams(cu_count(torch), w, K), K, dtype, walk=walk, waves=w)


# ---------------------------------------------------------------------------
# 2. the LDS cap
# ---------------------------------------------------------------------------
NODE_BYTES = 16  # a node of the table the hop kernel stages (include/vad_amd.h)


@functools.lru_cache(maxsize=None)
def comb(w):
    """The smallest comb (tests/stream_tree_reference.py) whose table caps a
    K = 2 launch of 8 n_cu + 1 streams at w waves per block, found by asking
    the launch rule; thresholds from the patterns' own feature rows.  Returns
    the classifier (with node scores) and its node count."""
    import torch
    from vad_amd import _lib
    from vad_amd.stream import StreamBatch
    lib = _lib.lib()
    probe = StreamBatch(P, tree_with_scores())
    S = 8 * cu_count(torch) + 1
    blob = lib.vad_stream_hop_tree_table_bytes(probe.plan.handle, probe.ffn.plan.handle, _lib.TREE_WALK_GLOBAL)
    n_max = lib.vad_stream_tree_max_lds_nodes(probe.plan.handle)
    assert blob > 0 and lib.vad_stream_hop_block_waves(blob, S, 2) == 16
    n = next(n for n in range(3, n_max + 1) if lib.vad_stream_hop_block_waves(blob + NODE_BYTES * n, S, 2) == w)
    assert lib.vad_stream_hop_block_waves(blob + NODE_BYTES * (n - 1), S, 2) == 2 * w  # one node fewer: not capped to w
    rec = pattern_run("tree", "plain", "float32")
    seq = torch.stack([r["state"]["ring"][:, t % 5] for t, r in enumerate(rec)], dim=1)  # (P, HOPS, C)
    X = np.concatenate([O.analyser_features_fast(seq[s].cpu().numpy()) for s in range(P)])
    table, depth = TR.comb_table(n, X, list(range(13, 26)))
    assert len(table["feature"]) == n and len(set(depth.tolist())) > len(X) // 4
    return with_counts(table), n


@pytest.mark.parametrize("form,dtype", [("plain", "int16"), ("scores", "float32"), ("sessions_denoise", "float32")])
@pytest.mark.parametrize("w", [8, 4, 2])
def test_the_lds_cap_leaves_a_multi_wave_block(torch_cuda, w, form, dtype):
    """8 n_cu + 1 streams in blocks of two hops ask for 16 waves; the comb's
    table leaves room for w.  Rows equal their patterns, and the labels equal
    the global walk's of the same tree (16 waves: nothing staged but the hop
    tables)."""
    torch = torch_cuda
    S = 8 * cu_count(torch) + 1
    clf, n = comb(w)
    assert n > 3
    lds = run_case(torch, ("comb", w), form, S, 2, dtype, walk="auto", waves=w)
    glob = run_case(torch, ("comb", w), form, S, 2, dtype, walk="global", waves=16)
    assert len(lds) == len(glob) and all(same(a, b) for a, b in zip(lds, glob))


# ---------------------------------------------------------------------------
# 3. stale LDS at 16 waves
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,form,K,dtype", [("bl13", "sessions_denoise", 2, "int16"), ("tree", "scores", 1, "float32")])
def test_sixteen_waves_ignore_stale_lds(torch_cuda, poison, name, form, K, dtype):
    """Every launch preceded by three kernels that fill every CU's LDS with
    1e30, -1e30 and NaN: the results are the clean run's."""
    torch = torch_cuda
    S = 8 * cu_count(torch) + 1
    clean = run_case(torch, name, form, S, K, dtype, waves=16)
    fouled = run_case(torch, name, form, S, K, dtype, waves=16, fill=poison)
    assert len(clean) == len(fouled) and all(same(a, b) for a, b in zip(clean, fouled))
