"""The sessions entries of the stream resampler refuse bad arguments with
VAD_EINVAL before any HIP call (no GPU here; the device pointers below are
never dereferenced), and do nothing, successfully, for zero streams or zero
hops."""
import ctypes

import numpy as np
import pytest

E = -1  # VAD_EINVAL
N = None  # NULL
INP, STATE, OUT, CNT, RST, IDX = 0x100000, 0x200000, 0x300000, 0x400000, 0x410000, 0x420000
ENTRIES = [f"vad_resample_stream_sessions_{i}_{o}" for i in ("f32", "i16") for o in ("f32", "i16")]


@pytest.fixture(scope="module")
def lib():
    from vad_amd import _lib
    return _lib.lib()


def create(lib, up, down):
    mx = max(up, down)
    buf = np.zeros(1 if mx == 1 else 20 * mx + 1, np.float32)
    h = ctypes.c_void_p()
    assert lib.vad_resample_plan_create(up, down, buf.ctypes.data, len(buf), ctypes.byref(h)) == 0 and h.value
    return h


@pytest.fixture(scope="module")
def plans(lib):
    """48 kHz (1 / 3), 8 kHz (2 / 1), 16 kHz (1 / 1) and 11.025 kHz (640 / 441: 160 outputs are 110.25 samples)."""
    hs = [create(lib, *r) for r in ((1, 3), (2, 1), (1, 1), (640, 441))]
    yield hs
    for h in hs:
        assert lib.vad_resample_plan_destroy(h) == 0


def array(hs):
    return (ctypes.c_void_p * max(len(hs), 1))(*[h.value if h is not None else None for h in hs])


@pytest.mark.parametrize("fn", ENTRIES)
def test_sessions_entries_refuse(lib, plans, fn):
    S, K, HI, HO = 4, 3, 480, 160
    three = array(plans[:3])
    out_size = 2 if fn.endswith("i16") else 4

    def call(**kw):
        a = dict(plans=three, R=3, inp=INP, hs=HI, bs=S * HI, S=S, K=K, ho=HO, cnt=CNT, rst=RST, idx=IDX, state=STATE,
                 out=OUT)
        a.update(kw)
        return getattr(lib, fn)(a["plans"], a["R"], a["inp"], a["hs"], a["bs"], a["S"], a["K"], a["ho"], a["cnt"],
                                a["rst"], a["idx"], a["state"], a["out"], N)

    for kw in (dict(plans=N), dict(plans=array([plans[0], None, plans[2]])),    # null, a null plan in the list
               dict(R=0), dict(R=-1), dict(R=9),                               # n_rates outside 1 .. 8
               dict(plans=array([plans[0], plans[3]]), R=2, hs=480),           # 11.025 kHz: no whole hop
               dict(K=40),                                                     # 40 hops of 480 samples pass the window
               dict(inp=N), dict(state=N), dict(out=N), dict(cnt=N), dict(rst=N), dict(idx=N),
               dict(S=-1), dict(K=-1), dict(ho=0), dict(ho=-160),
               dict(hs=HI - 1), dict(hs=0), dict(hs=-HI),          # a row narrower than the largest hop_in
               dict(bs=0), dict(bs=-S * HI), dict(bs=S * HI - 1),  # hop-major blocks repeat or overlap
               dict(bs=HI, hs=K * HI - 1),                         # stream-major rows overlap
               dict(inp=INP + 1), dict(out=OUT + 1), dict(state=STATE + 2), dict(cnt=CNT + 2), dict(idx=IDX + 1),
               dict(out=INP), dict(state=INP), dict(out=STATE),    # the buffers overlap
               dict(cnt=INP), dict(rst=INP + 5), dict(idx=INP), dict(cnt=OUT), dict(rst=OUT + K * S * HO * out_size - 1),
               dict(idx=OUT), dict(cnt=STATE), dict(rst=STATE + 3), dict(idx=STATE),
               dict(rst=CNT), dict(rst=CNT + 4 * S - 1), dict(idx=CNT), dict(idx=CNT + 4), dict(rst=IDX + 2)):
        assert call(**kw) == E, kw
    # arguments that pass reach the HIP runtime, which is not asked here: what succeeds without it is nothing to do
    assert call(S=0) == 0 and call(K=0) == 0
    assert call(S=0, inp=N, state=N, out=N, cnt=N, rst=N, idx=N) == 0
    # a bad argument stays bad when there is nothing to do
    assert call(S=0, ho=0) == E and call(K=0, hs=HI - 1) == E and call(S=0, R=0) == E and call(K=0, plans=N) == E
    assert call(S=0, plans=array([plans[0], None]), R=2) == E
    # a row is as wide as the largest hop_in: 8 kHz alone takes rows of 80
    assert call(plans=array([plans[1]]), R=1, hs=80, bs=S * 80, S=0) == 0
    assert call(plans=array([plans[1], plans[0]]), R=2, hs=80, bs=S * 80, S=0) == E


def test_state_bytes(lib, plans):
    sb = lib.vad_resample_sessions_state_bytes
    # 1 / 3: history 60; 2 / 1: P = 20, T = 21, d = 20, history = ceil(0 / 2) + 20; 1 / 1: history 0
    assert lib.vad_resample_stream_state_bytes(plans[0], 5) == 5 * 61 * 4
    assert lib.vad_resample_stream_state_bytes(plans[1], 5) == 5 * 21 * 4
    assert lib.vad_resample_stream_state_bytes(plans[2], 5) == 5 * 1 * 4
    # per stream the longest history, the emitted count and the rate index
    assert sb(array(plans[:1]), 1, 5) == 5 * 62 * 4
    assert sb(array(plans[1:2]), 1, 7) == 7 * 22 * 4
    assert sb(array(plans[2:3]), 1, 7) == 7 * 2 * 4
    assert sb(array(plans[:3]), 3, 5) == 5 * 62 * 4
    assert sb(array([plans[2], plans[1], plans[0]]), 3, 1) == 62 * 4
    for bad in ((N, 1, 5), (array(plans[:3]), 0, 5), (array(plans[:3]), 9, 5), (array(plans[:3]), 3, 0),
                (array(plans[:3]), 3, -2), (array([plans[0], None]), 2, 5)):
        assert sb(*bad) == 0, bad
    assert lib.vad_resample_sessions_grid() >= 1
