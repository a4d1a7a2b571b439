"""The state step of the SimpleAnalyser streams, without a device: the NumPy
restatement (tests/simple_stream_reference.py) against the trace of the
unmodified reference class (tests/golden/simple.npz) and, row by row, against
SimpleAnalyser._step; hand-made rows for every edge of the step; and the
argument rules of SimpleStreamBatch that need no device."""
import numpy as np
import pytest

import simple_stream_reference as R
from oracle import vad_oracle as O
from vad_amd.simple_analyser import SimpleAnalyser

CASES = ["a", "b", "c"]


@pytest.fixture(scope="module")
def case_rows(golden):
    """case -> (noise_buf_len, feature rows of every frame), oracle features, computed once."""
    g = golden("simple")
    out = {}
    for c in CASES:
        fs, nb = int(g[f"{c}_meta"][0]), int(g[f"{c}_meta"][1])
        out[c] = (fs, nb, np.array([O.simple_frame_features(r, fs, 16000) for r in g[f"{c}_frames"]]))
    return out


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_reference_trace(golden, case_rows, case):
    fs, nb, rows = case_rows[case]
    ref = golden("simple")[f"{case}_trace"]
    st = R.RefStream(nb).init(rows[:nb])
    tr = []
    for f in rows[nb:]:
        r = st.step(f)
        tr.append([float(r), float(st.silence), st.energy_thresh, st.std_thresh, *st.bands_thresh])
    tr = np.asarray(tr)
    assert np.array_equal(tr[:, :2], ref[:, :2])
    assert np.allclose(tr[:, 2:], ref[:, 2:], rtol=1e-12, atol=0)


def _host(fs, nb, init_rows, monkeypatch):
    monkeypatch.setattr(SimpleAnalyser, "frame_features", lambda self, frames: np.asarray(init_rows))
    sa = SimpleAnalyser(16000, fs, nb)
    sa.load_init_inactive_frames([np.zeros(fs)] * nb)
    return sa


def _same_state(st, sa):
    assert st.status == list(sa.temp_buffer)
    assert (st.silence, st.noise_pointer, st.frame_number) == (sa.silence, sa.noise_pointer, sa.frame_number)
    got = np.concatenate([[sa.energy_thresh, sa.spectral_std_thresh], sa.spectral_energy_bands_thresh])
    assert st.thresholds().tobytes() == np.asarray(got, np.float64).tobytes()  # bit-equal: noise_buf_len < 8
    assert st.noise.tobytes() == np.ascontiguousarray(sa._noise_feats[:, [0, 2, 3, 4, 5, 6]]).tobytes()


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_host_step_row_by_row(case_rows, monkeypatch, case):
    fs, nb, rows = case_rows[case]
    sa = _host(fs, nb, rows[:nb], monkeypatch)
    st = R.RefStream(nb).init(rows[:nb])
    _same_state(st, sa)
    for f in rows[nb:]:
        assert st.step(f) == sa._step(f)
        _same_state(st, sa)


@pytest.mark.parametrize("nb", [1, 3])
def test_edge_rows_match_host_step(monkeypatch, nb):
    for name, rows in R.edge_sequences().items():
        sa = _host(400, nb, R.edge_init(nb), monkeypatch)
        st = R.RefStream(nb).init(R.edge_init(nb))
        for f in rows:
            assert st.step(f) == sa._step(f), name
            _same_state(st, sa)


def _fresh(nb=3):
    st = R.RefStream(nb).init(R.edge_init(nb))
    assert st.thresholds().tolist() == [10.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    return st


def test_edges_of_the_classification():
    seq = R.edge_sequences()
    want = {"zcr_5": True, "zcr_20": True, "zcr_4.999": False, "zcr_20.001": False,
            "bands_equal": False,   # a feature equal to k * thresh is inactive
            "bands_above": True,    # band 0 and two of the others one ulp above
            "band0_equal": False,   # band 0 decides first
            "energy_equal": False, "std_equal": False, "second_path": True}
    for name, active in want.items():
        assert _fresh().step(seq[name][0]) is active, name


def test_noise_energy_is_truncated():
    st = _fresh(1)
    assert st.step(R.row(**R.QUIET)) is False
    assert st.noise[0, 0] == 7.9                   # stored as it came
    assert st.energy_thresh == 0.75 * 10.0 + 0.25 * 7.0   # counted as 7
    st = _fresh(3)
    st.step(R.row(**R.QUIET))
    assert st.energy_thresh == 0.75 * 10.0 + 0.25 * (27.0 / 3.0)


def test_silence_switches():
    act, quiet = R.row(**R.ACTIVE), R.row(**R.QUIET)
    st = _fresh()
    for i in range(4):
        assert st.step(act) is True and st.silence       # not on the 4th active status
    assert st.step(act) is True and not st.silence       # on the 5th
    for i in range(15):                                  # 20 active statuses in the buffer
        st.step(act)
    assert st.status == [True] * 20 and st.noise_pointer == 0
    th = st.thresholds().copy()
    for i in range(14):
        assert st.step(quiet) is True and not st.silence  # still talking, nothing stored
    assert st.noise_pointer == 0 and np.array_equal(st.thresholds(), th)
    assert st.step(quiet) is True and st.silence          # the 15th: silence, yet returned active ...
    assert st.noise_pointer == 1 and st.noise[0, 0] == 7.9    # ... and stored as noise
    assert not np.array_equal(st.thresholds(), th)
    assert st.step(quiet) is False and st.noise_pointer == 2


@pytest.mark.parametrize("nb", [1, 3])
def test_noise_pointer_wraps(nb):
    st = _fresh(nb)
    seen = []
    for f in R.edge_sequences()["wrap"]:
        assert st.step(f) is False
        seen.append(st.noise_pointer)
    assert seen == [(i + 1) % nb for i in range(len(seen))]
    # the buffer holds the last nb rows, each in its slot
    rows = R.edge_sequences()["wrap"]
    n = len(rows)
    for i in range(n - nb, n):
        assert st.noise[i % nb, 0] == rows[i][0]


def test_packed_state_layout():
    from vad_amd import simple_stream as SS
    st = _fresh(3)
    for f in [R.row(**R.ACTIVE)] * 2 + [R.row(**R.QUIET)]:
        st.step(f)
    p = st.packed()
    assert p.shape == (SS.state_doubles(3),)
    w = p.view(np.int32)[2 * (6 * 3 + 6):]
    assert w.tolist() == [0b110, 1, 1, 3]     # two active statuses, then an inactive one (bit 0 the newest)
    sa = SimpleAnalyser(16000, 400, 3)
    sa.initialized = True
    sa._noise_feats[:, [0, 2, 3, 4, 5, 6]] = st.noise
    sa.energy_thresh, sa.spectral_std_thresh = st.energy_thresh, st.std_thresh
    sa.spectral_energy_bands_thresh = st.bands_thresh.copy()
    sa.temp_buffer, sa.silence, sa.noise_pointer, sa.frame_number = list(st.status), st.silence, 1, 3
    assert SS.pack_state([sa]).tobytes() == p[None].tobytes()


def test_state_size_and_argument_rules():
    import torch
    from vad_amd import SimpleStreamBatch, _lib
    from vad_amd import simple_stream as SS
    lib = _lib.lib()
    for nb in (1, 3, 5, 64):
        assert lib.vad_simple_stream_state_bytes(nb) == 8 * SS.state_doubles(nb) == 48 * nb + 64
    assert lib.vad_simple_stream_state_bytes(0) == 0 and lib.vad_simple_stream_state_bytes(65) == 0
    assert SS.fft_geometry(16000, 400) == (512, 56, 32) and SS.fft_geometry(16000, 401) == (512, 56, 32)
    assert SS.one_kernel_length(512) and SS.one_kernel_length(4096)
    assert not SS.one_kernel_length(513) and not SS.one_kernel_length(8192)
    # refused before anything touches a device
    for kw in [dict(n_streams=0), dict(noise_buf_len=0), dict(noise_buf_len=65), dict(frames_per_step=0),
               dict(input_dtype=torch.float64), dict(frame_size=1), dict(frame_size=8193),
               dict(frame_size=401, input_dtype=torch.int16),    # L = 513: the two-launch path is fp32 only
               dict(frame_size=8192, input_dtype=torch.int16)]:
        a = dict(n_streams=2, frame_rate=16000, frame_size=400, noise_buf_len=5)
        a.update(kw)
        with pytest.raises(ValueError):
            SimpleStreamBatch(**a)
    with pytest.raises(Exception, match="FFTN is small"):
        SimpleStreamBatch(2, 1000, 2, 5)
