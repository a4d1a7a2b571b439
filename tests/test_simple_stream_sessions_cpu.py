"""The sessions restatement (tests/simple_stream_sessions_reference.py)
against simple_stream_reference itself, on the hand-made edge rows: no
device, nothing of vad_amd."""
import numpy as np

import simple_stream_reference as R
import simple_stream_sessions_reference as RS

NB = 3


def _columns():
    """(K, S, 7): one edge sequence per stream."""
    seqs = list(R.edge_sequences().values())
    return np.stack(seqs, axis=1)


def test_full_counts_equal_the_plain_run():
    rows = _columns()
    K, S = rows.shape[:2]
    for blk in (1, 4, K):
        ref = RS.RefSessions(S, NB)
        for s in range(S):
            ref.load(s, R.edge_init(NB))
        labs = []
        for t in range(0, K, blk):
            lab, voiced = ref.block(rows[t:t + blk], [blk] * S, [0] * S)
            labs.append(lab)
            for s in range(S):
                assert voiced[s] == [i for i in range(lab.shape[0]) if lab[i, s] == 1]
        labs = np.concatenate(labs)
        seen = set()
        for s in range(S):
            want, st = R.run(rows[:, s], R.edge_init(NB), NB)
            assert np.array_equal(labs[:, s], want), s
            assert ref.packed(s).tobytes() == st.packed().tobytes(), s
            assert ref.init_left(s) == 0
            seen |= set(want.tolist())
        assert seen == {0, 1}


def test_in_sequence_init_equals_load():
    """A fresh stream fed init ++ rows equals R.run on them, with nb rows of 253
    in front, whichever blocks the init rows arrive in."""
    rows = _columns()
    K, S = rows.shape[:2]
    full = np.concatenate([np.broadcast_to(R.edge_init(NB)[:, None], (NB, S, 7)), rows])
    for blk in (1, 2, NB, 8):
        labs, _, ref = RS.run([(full[t:t + blk], [blk] * S, [0] * S) for t in range(0, len(full), blk)], S, NB)
        labs = np.concatenate(labs)
        assert (labs[:NB] == RS.INIT).all()
        for s in range(S):
            want, st = R.run(rows[:, s], R.edge_init(NB), NB)
            assert np.array_equal(labs[NB:, s], want)
            assert ref.packed(s).tobytes() == st.packed().tobytes()


def test_restart_mid_sequence_equals_two_runs():
    rows = _columns()
    K, S = rows.shape[:2]
    cut = 13
    init2 = R.edge_init(NB) * 2.0
    first = np.concatenate([np.broadcast_to(R.edge_init(NB)[:, None], (NB, S, 7)), rows[:cut]])
    second = np.concatenate([np.broadcast_to(init2[:, None], (NB, S, 7)), rows[cut:]])
    sched = [(first, [len(first)] * S, [0] * S), (second, [len(second)] * S, [1] * S)]
    labs, _, ref = RS.run(sched, S, NB)
    for s in range(S):
        w1, _ = R.run(rows[:cut, s], R.edge_init(NB), NB)
        w2, st2 = R.run(rows[cut:, s], init2, NB)
        assert np.array_equal(labs[0][NB:, s], w1) and np.array_equal(labs[1][NB:, s], w2)
        assert (labs[0][:NB, s] == RS.INIT).all() and (labs[1][:NB, s] == RS.INIT).all()
        assert ref.packed(s).tobytes() == st2.packed().tobytes()
        assert ref.sessions[s] == 1


def test_init_rules():
    rows = _columns()[:, :2]
    ref = RS.RefSessions(2, NB)
    assert ref.init_left(0) == NB and not ref.packed(0).any()          # fresh: the record all zero
    init = R.edge_init(NB)
    blk = np.stack([init[:2], init[:2]], axis=1)                       # (2, S, 7)
    lab, voiced = ref.block(blk, [2, 0], [0, 0])                       # a count of 0 leaves init_left alone
    assert ref.init_left(0) == NB - 2 and ref.init_left(1) == NB
    assert lab[:, 0].tolist() == [RS.INIT, RS.INIT] and lab[:, 1].tolist() == [RS.NO_HOP, RS.NO_HOP]
    assert voiced == [[], []]
    mid = ref.packed(0)
    assert np.array_equal(mid[:12].reshape(2, 6), init[:2][:, [0, 2, 3, 4, 5, 6]]) and not mid[12:].any()
    # counts above k and below 0 are clamped
    lab, _ = ref.block(blk, [99, -5], [0, 0])
    assert lab[:, 1].tolist() == [RS.NO_HOP, RS.NO_HOP] and ref.init_left(1) == NB
    # stream 0: its third init row, then a classified row, in one block
    assert lab[0, 0] == RS.INIT and lab[1, 0] in (0, 1) and ref.init_left(0) == 0
    want = R.RefStream(NB).init(np.stack([init[0], init[1], init[0]]))
    st = ref.streams[0]
    assert st.frame_number == 1
    # the last init frame: silence on, pointer 0, status cleared, thresholds the plain means
    ref2 = RS.RefSessions(1, NB)
    ref2.block(init[:, None], [NB], [0])
    w = ref2.packed(0).view(np.int32)[2 * (6 * NB + 6):]
    assert w.tolist() == [0, 1, 0, 0]
    assert ref2.packed(0).tobytes() == want.packed().tobytes()          # init rows 0 and 2 are equal
    # a restart with no row: fresh again, and the flag's effect happens once
    ref2.block(init[:1, None], [0], [1])
    assert ref2.init_left(0) == NB and not ref2.packed(0).any() and ref2.sessions[0] == 1
    ref2.block(init[:1, None], [0], [0])
    assert ref2.init_left(0) == NB and rows.shape[1] == 2
