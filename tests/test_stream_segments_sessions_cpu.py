"""Sessions in the streaming segmenter (include/vad_amd.h, "Sessions in the
streaming segmenter"), without a GPU: the host model of
tests/stream_segments_sessions_reference.py pinned, session by session, against
the offline models (model_segments / model_voiced, and the clip chain for the
operating-point forms) on each session's equivalent clip; the workloads the
GPU tests run, checked to contain every case those tests are there for; and
the new symbols with their argument counts in the header and the symbol map.
"""
import os
import re

import numpy as np
import pytest

import stream_segments_sessions_reference as R
from scores_reference import hysteresis
from stream_scores_reference import clip_chain
from test_segments_cpu import model_segments, model_voiced

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_case(framing, params, form, dtype, S, K):
    """The workload of (S, K) through the model, every stream ended by a final flush."""
    (L, H), (g, m) = framing, params
    kw = R.FORMS[form]
    seed = R.seed_of(S, K)
    counts, restart = R.schedule(S, K, seed)
    x = R.block_values(S, K, counts, seed, scores="on" in kw, restart=restart)
    hops = None if dtype is None else R.audio_blocks(S, K, len(x), H, dtype, seed)
    model = R.SessionsSegModel(S, L, H, g, m, dtype=dtype or np.int16, fill=0, **kw)
    outs = R.run_model(model, x, hops, counts, restart)
    model.flush(audio=hops is not None)
    return model, outs, counts, restart


CONFIGS = [(f, p, form) for f in R.SESSION_FRAMINGS for p in R.SESSION_PARAMS for form in R.FORMS]


@pytest.mark.parametrize("framing,params,form", CONFIGS)
def test_every_session_equals_the_offline_models(framing, params, form):
    (L, H), (g, m) = framing, params
    kw = R.FORMS[form]
    for dtype in (np.float32, np.int16):
        S, K = R.shape_for(framing, params, form, dtype)
        model, outs, counts, restart = run_case(framing, params, form, dtype, S, K)
        n_sessions = 0
        for s in range(S):
            rows_of = {}
            for o, a, b in model.rows[s]:
                rows_of.setdefault(o, []).append((a, b))
            ordinals = [g_["ordinal"] for g_ in model.sessions(s)]
            assert ordinals == sorted(set(ordinals)) and set(rows_of) <= set(ordinals)
            for sess in model.sessions(s):
                assert sess["ended"]
                clip = R.session_clip(sess, L, H, dtype)
                T = len(sess["x"])
                assert len(clip) == L - H + T * H
                win = np.array(sess["x"][5:], dtype=np.float32 if "on" in kw else np.uint8)
                if form == "labels":
                    want, total = model_segments(win, len(clip), L, H, g, m)
                else:
                    want, total = clip_chain(win, len(clip), L, H, g, m, kw.get("pad", (0, 0)), kw.get("on"),
                                             kw.get("off"))
                where = (framing, params, form, S, K, s, sess["ordinal"])
                got = np.array(rows_of.get(sess["ordinal"], []), dtype=np.int64).reshape(-1, 2)
                assert np.array_equal(got, want[:, :2]), where
                voiced = np.concatenate(sess["voiced"]) if sess["voiced"] else np.zeros(0, dtype)
                assert len(voiced) == total, where
                assert np.array_equal(voiced.astype(dtype).view(np.uint8), model_voiced(clip, want).view(np.uint8)), where
                n_sessions += 1
        assert n_sessions > S
        # the outputs' shapes and the zeros the device writes
        n = R.taken(counts, K)
        for b, (v, vl, ev, el) in enumerate(outs):
            assert vl.shape == (K, S) and el.shape == (model.F, S)
            for s in range(S):
                assert (vl[n[b, s]:, s] == 0).all()
                if not restart[b, s]:
                    assert (el[:, s] == 0).all()


def test_events_only_model_gives_the_same_rows():
    framing, params = (8, 3), (2, 3)
    for form in R.FORMS:
        a = run_case(framing, params, form, np.int16, 5, 3)[0]
        b = run_case(framing, params, form, None, 5, 3)[0]
        assert a.rows == b.rows and sum(len(r) for r in a.rows) > 0


@pytest.mark.parametrize("S,K", R.SHAPES)
def test_schedules_contain_the_structural_cases(S, K):
    counts, restart = R.schedule(S, K, R.seed_of(S, K))
    n = R.taken(counts, K)
    B = len(counts)
    assert counts.min() == -1 and counts.max() == K + 1  # both clamps
    assert ((restart != 0) & (n == 0)).any()             # a restart with count 0
    assert ((restart != 0) & (n == K)).any()             # a restart with a full count
    used = np.cumsum(n + (restart != 0), axis=0) - (n + (restart != 0))  # hops and flags before block b
    assert ((restart != 0) & (used == 0) & (np.arange(B)[:, None] > 0)).any()  # a restart on a never-used stream
    idle = (n == 0) & (restart == 0)
    stalled = idle[:-2] & idle[1:-1] & idle[2:] & (np.cumsum(n, axis=0)[:-2] > 0)  # after hops, 3 blocks in a row
    assert stalled.any()
    # a session shorter than 5 hops that a restart ends
    model = run_case((8, 3), (0, 0), "labels", None, S, K)[0]
    assert any(0 < len(g["x"]) < 5 and g["ended"] for s in range(S) for g in model.sessions(s))


@pytest.mark.parametrize("framing,params,form", CONFIGS)
def test_workloads_contain_the_label_dependent_cases(framing, params, form):
    """At every (S, K, dtype) the GPU test runs this configuration with."""
    for S, K in sorted({R.shape_for(framing, params, form, d) for d in R.DTYPES}):
        model = run_case(framing, params, form, None, S, K)[0]
        where = (framing, params, form, S, K)
        # a session cut while a segment is open, by a restart (the last session of a stream ends in the flush)
        assert any(g.get("end_rows", 0) > 0 for s in range(S) for g in model.log[s][:-1]), where
        assert len({(s, r[0]) for s in range(S) for r in model.rows[s]}) >= 4, where     # sessions with a segment
        assert max(len(model.rows[s]) for s in range(S)) > R.CAPACITY, where             # rows past the capacity


@pytest.mark.parametrize("S,K", R.SHAPES)
def test_score_workloads_would_show_a_leaked_hysteresis_bit(S, K):
    """A session that a restart ends with the hysteresis decision at 1, followed
    by a session whose first window's score lies in the off..on band: that
    window is inactive in a fresh session and active if the bit leaked."""
    kw = R.FORMS["op_scores"]
    model = run_case((400, 160), (0, 0), "op_scores", None, S, K)[0]
    shown = 0
    for s in range(S):
        log = model.log[s]
        for prev, nxt in zip(log[:-1], log[1:]):
            if len(prev["x"]) > 5 and len(nxt["x"]) > 5 and prev["ended"]:
                h = hysteresis(np.array(prev["x"][5:], np.float32), kw["on"], kw["off"])
                shown += int(h[-1] == 1 and kw["off"] <= nxt["x"][5] < kw["on"])
    assert shown > 0, (S, K)


# ---------------------------------------------------------------------------
# the library: symbols and argument counts
# ---------------------------------------------------------------------------
SYMBOLS = {"vad_stream_segments_sessions": 18, "vad_stream_segments_sessions_f32": 26,
           "vad_stream_segments_sessions_i16": 26, "vad_stream_segments_op_sessions": 23,
           "vad_stream_segments_op_sessions_f32": 31, "vad_stream_segments_op_sessions_i16": 31}


def test_library_exports_the_sessions_entries():
    from vad_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(REPO, "include", "vad_amd.h")).read()
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name, n_args in SYMBOLS.items():
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert decl.group(1).count(",") + 1 == n_args, name
        sibling = name.replace("_sessions", "")
        extra = 4 if name.endswith("sessions") else 5  # end_voiced only with audio
        assert len(_lib.SIGNATURES[sibling][1]) + extra == n_args, name
        for arg in ("hop_counts", "restart", "end_len", "table_session") + (("end_voiced",) if extra == 5 else ()):
            assert re.search(r"\b%s\b" % arg, decl.group(1)), (name, arg)
        assert name in integration, name


def test_python_argument_checks():
    import torch
    from vad_amd.stream_segments import StreamSegmenter
    cpu = torch.device("cpu")
    seg = StreamSegmenter(4, device=cpu, max_gap=2, min_run=3, hops_per_step=3, sessions=True, capacity=5,
                          audio_dtype=torch.int16)
    assert seg.hop_counts.tolist() == [3] * 4 and seg.restart.tolist() == [0] * 4
    assert tuple(seg.end_len.shape) == (seg.flush_rows, 4) and tuple(seg.end_voiced.shape) == (seg.flush_rows, 4, 160)
    assert tuple(seg.table_session.shape) == (4, 5) and seg.table_session.dtype == torch.int32
    assert seg._fn == "vad_stream_segments_sessions_i16" and seg._flush_fn == "vad_stream_segments_flush_i16"
    seg.hop_counts.fill_(1), seg.restart.fill_(1), seg.table_session.fill_(7)
    seg.reset()
    assert seg.hop_counts.tolist() == [3] * 4 and seg.restart.tolist() == [0] * 4 and int(seg.table_session.sum()) == 0
    events = StreamSegmenter(4, device=cpu, sessions=True, on=0.5)
    assert events._events_fn == "vad_stream_segments_op_sessions" and events.end_voiced is None
    assert events.end_len is not None
    shared = torch.zeros(4, dtype=torch.int32)
    assert StreamSegmenter(4, device=cpu, sessions=True, hop_counts=shared).hop_counts is shared
    with pytest.raises(ValueError, match="sessions=True"):
        StreamSegmenter(4, device=cpu, hop_counts=shared)
    with pytest.raises(ValueError, match="hop_counts"):
        StreamSegmenter(4, device=cpu, sessions=True, hop_counts=shared.long())
    with pytest.raises(ValueError, match="hop_counts"):
        StreamSegmenter(4, device=cpu, sessions=True, hop_counts=torch.zeros(5, dtype=torch.int32))
    plain = StreamSegmenter(4, device=cpu)
    assert plain.hop_counts is None and plain.restart is None and not plain.sessions
    with pytest.raises(ValueError, match="sessions=True"):
        plain._set_sessions(shared, None)
    with pytest.raises(ValueError, match="sessions=True"):
        plain.session_segments()
