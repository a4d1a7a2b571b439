"""The host model of the sessions stream resampler (tests/resample_sessions_reference.py)
against vad_amd.resample.StreamModel, without a GPU, and the properties of the
scripted workload that the GPU tests rely on."""
import numpy as np
import pytest

import resample_sessions_reference as R
from vad_amd import resample as V


@pytest.mark.parametrize("rate", [8000, 16000, 44100, 48000])
def test_one_rate_full_counts_no_restart_is_the_stream_model(rate):
    S, K, blocks = 3, 2, 5
    hop_in = R.hop_in_of(rate)
    x = R.audio(blocks, K, S, hop_in, seed=rate).astype(np.float64)
    model = R.SessionsResampleModel(S, [rate], K)
    plain = V.StreamModel(S, rate)
    full, none, idx = np.full(S, K), np.zeros(S, np.uint8), np.zeros(S, np.int32)
    for b in range(blocks):
        got = model.step(x[b], full, none, idx)
        assert np.array_equal(got, plain.step(x[b])), (rate, b)
    assert plain.spec.delay == 0 or (got != 0).any()


def test_a_session_split_over_blocks_equals_its_hops_one_by_one():
    S, K, blocks = 6, 3, 12
    counts, restart, rate = R.script(S, K, blocks)
    hop_max = max(R.hop_in_of(r) for r in R.RATES)
    x = R.audio(blocks, K, S, hop_max).astype(np.float64)
    model = R.SessionsResampleModel(S, R.RATES, K)
    outs = [model.step(x[b], counts[b], restart[b], rate[b]) for b in range(blocks)]
    n = np.clip(counts, 0, K)
    for b in range(blocks):  # rows past the count are not written, the others are
        for s in range(S):
            assert np.isnan(outs[b][n[b, s]:, s]).all() and not np.isnan(outs[b][:n[b, s], s]).any()
    total = 0
    for s in range(S):
        for sess in model.sessions[s]:
            one = V.StreamModel(1, R.RATES[sess["rate"]])
            for hop, row in zip(sess["hops"], sess["rows"]):
                assert len(hop) == one.hop_in
                assert np.array_equal(one.step(hop[None, None, :])[0, 0], row)
            total += len(sess["hops"])
    assert total == int(n.sum())


def test_the_script_holds_the_cases_the_gpu_tests_are_there_for():
    S, K, blocks = 6, 3, 12
    counts, restart, rate = R.script(S, K, blocks)
    assert counts.shape == restart.shape == rate.shape == (blocks, S)
    assert counts.min() == -1 and counts.max() == K + 1          # both clamps
    assert restart[0].all()
    model = R.SessionsResampleModel(S, R.RATES, K)
    hop_max = max(R.hop_in_of(r) for r in R.RATES)
    x = np.zeros((K, S, hop_max))
    for b in range(blocks):
        model.step(x, counts[b], restart[b], rate[b])
    n = np.clip(counts, 0, K)
    for s in range(S):
        used = {sess["rate"] for sess in model.sessions[s][1:] if sess["hops"]}
        assert len(used) >= 2, s                                   # at least two rates, each with hops
        assert ((n[:, s] == 0) & (restart[:, s] == 0)).any(), s    # at least one stall
    assert {sess["rate"] for s in range(S) for sess in model.sessions[s][1:] if sess["hops"]} == {0, 1, 2, 3}
    b = int(np.flatnonzero(restart[1:, 1])[0]) + 1
    assert counts[b, 1] == 0                                       # a restart with count 0
    assert sorted(rate[np.flatnonzero(restart[1:, 2]) + 1, 2].tolist()) == [-1, len(R.RATES)]
    # an index without a flag names another rate than the running one somewhere
    cur, seen = rate[0].copy(), False
    for b in range(1, blocks):
        cur = np.where(restart[b] != 0, np.clip(rate[b], 0, 3), cur)
        seen |= bool(((restart[b] == 0) & (np.clip(rate[b], 0, 3) != cur)).any())
    assert seen


def test_constants_match_the_header_and_the_library():
    import os
    import re
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(here, "include", "vad_amd.h")).read()
    assert int(re.search(r"#define VAD_RESAMPLE_MAX_RATES (\d+)", src).group(1)) == V.MAX_RATES == 8
    from vad_amd import _lib
    assert _lib.lib().vad_resample_sessions_grid() == V.SESSIONS_GRID
    for name in ("vad_resample_sessions_grid", "vad_resample_sessions_state_bytes",
                 *[f"vad_resample_stream_sessions_{i}_{o}" for i in ("f32", "i16") for o in ("f32", "i16")]):
        assert re.search(rf"\b{name}\(", src), name
