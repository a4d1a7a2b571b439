"""The streaming-segment entries refuse bad arguments with VAD_EINVAL before
any HIP call (no GPU here; the pointers below are never dereferenced), and do
nothing, successfully, for zero streams or zero hops."""
import pytest

E = -1  # VAD_EINVAL
N = None  # NULL
LAB, ST, SEG, FND = 0x10000, 0x20000, 0x30000, 0x40000
HOP, HIS, VOI, VLN = 0x100000, 0x200000, 0x300000, 0x400000
S, K, L, H = 4, 3, 400, 160
D = 0 + 1 + 1 + 1
RING = (D + 3 + K) * H + L  # elements one stream needs at these parameters


@pytest.fixture(scope="module")
def lib():
    from vad_amd import _lib
    return _lib.lib()


def events(lib, **kw):
    a = dict(labels=LAB, lbs=S, S=S, K=K, active=1, gap=0, run=0, L=L, H=H, state=ST, seg=SEG, cap=8, found=FND)
    a.update(kw)
    return lib.vad_stream_segments(a["labels"], a["lbs"], a["S"], a["K"], a["active"], a["gap"], a["run"], a["L"],
                                   a["H"], a["state"], a["seg"], a["cap"], a["found"], N)


def audio(lib, fn, **kw):
    a = dict(labels=LAB, lbs=S, S=S, K=K, active=1, gap=0, run=0, L=L, H=H, state=ST, seg=SEG, cap=8, found=FND,
             hop=HOP, hs=H, hbs=S * H, hist=HIS, helems=S * RING, voiced=VOI, vlen=VLN)
    a.update(kw)
    return getattr(lib, fn)(a["labels"], a["lbs"], a["S"], a["K"], a["active"], a["gap"], a["run"], a["L"], a["H"],
                            a["state"], a["seg"], a["cap"], a["found"], a["hop"], a["hs"], a["hbs"], a["hist"],
                            a["helems"], a["voiced"], a["vlen"], N)


def flush(lib, fn, **kw):
    a = dict(S=S, gap=0, run=0, L=L, H=H, state=ST, seg=SEG, cap=8, found=FND, hist=HIS, helems=S * RING,
             voiced=VOI, vlen=VLN)
    a.update(kw)
    head = (a["S"], a["gap"], a["run"], a["L"], a["H"], a["state"], a["seg"], a["cap"], a["found"])
    if fn == "vad_stream_segments_flush":
        return getattr(lib, fn)(*head, N)
    return getattr(lib, fn)(*head, a["hist"], a["helems"], a["voiced"], a["vlen"], N)


COMMON = [dict(H=0), dict(H=-160), dict(H=L + 1), dict(L=0), dict(gap=-1), dict(run=-1), dict(cap=-1), dict(S=-1),
          dict(state=N), dict(found=N), dict(seg=N)]


def test_events_entry_refuses(lib):
    for kw in COMMON + [dict(K=-1), dict(active=255), dict(active=256), dict(active=-1), dict(labels=N),
                        dict(lbs=S - 1), dict(lbs=0), dict(lbs=-S)]:
        assert events(lib, **kw) == E, kw
    assert events(lib, S=0) == 0 and events(lib, K=0) == 0
    assert events(lib, S=0, labels=N, state=N, seg=N, found=N) == 0  # nothing would be used
    assert events(lib, K=0, labels=N, state=N, seg=N, found=N) == 0
    # a bad argument stays bad when there is nothing to do
    assert events(lib, S=0, H=0) == E and events(lib, K=0, active=255) == E and events(lib, S=0, cap=-1) == E


@pytest.mark.parametrize("fn", ["vad_stream_segments_f32", "vad_stream_segments_i16"])
def test_audio_entries_refuse(lib, fn):
    for kw in COMMON + [dict(K=-1), dict(active=255), dict(labels=N), dict(lbs=S - 1),
                        dict(hop=N), dict(hist=N), dict(voiced=N), dict(vlen=N),
                        dict(hs=H - 1), dict(hs=0), dict(hs=-H),           # rows of one block overlap
                        dict(hbs=0), dict(hbs=-S * H),                      # a block repeats or walks backwards
                        dict(hbs=S * H - 1),                                # hop-major blocks overlap
                        dict(hbs=H, hs=K * H - 1),                          # stream-major rows overlap
                        dict(helems=S * RING - 1), dict(helems=0), dict(helems=-1),
                        dict(helems=S * ((1 << 30) + 1)),                   # ring indices would pass an int32
                        dict(hist=HIS + 1), dict(voiced=VOI + 1), dict(hop=HOP + 1), dict(vlen=VLN + 2)]:
        assert audio(lib, fn, **kw) == E, kw
    assert audio(lib, fn, S=0) == 0 and audio(lib, fn, K=0) == 0
    assert audio(lib, fn, K=0, hs=H - 1) == E


@pytest.mark.parametrize("fn", ["vad_stream_segments_flush", "vad_stream_segments_flush_f32",
                                "vad_stream_segments_flush_i16"])
def test_flush_entries_refuse(lib, fn):
    cases = list(COMMON)
    if fn != "vad_stream_segments_flush":
        cases += [dict(hist=N), dict(voiced=N), dict(vlen=N), dict(helems=S * ((D + 3) * H + L) - 1), dict(helems=-1)]
    for kw in cases:
        assert flush(lib, fn, **kw) == E, kw
    assert flush(lib, fn, S=0) == 0
    assert flush(lib, fn, S=0, gap=-1) == E


def test_sizing_entries_refuse(lib):
    assert lib.vad_stream_seg_delay(0, 0, 400, 0) == -1
    assert lib.vad_stream_seg_delay(0, -1, 400, 160) == -1
    assert lib.vad_stream_seg_flush_rows(-1, 0, 400, 160) == -1
    assert lib.vad_stream_seg_flush_rows(0, 0, 160, 400) == -1
    assert lib.vad_stream_seg_history_elems(-1, 1, 0, 0, 400, 160) == -1
    assert lib.vad_stream_seg_history_elems(4, -1, 0, 0, 400, 160) == -1
    assert lib.vad_stream_seg_history_elems(4, 1, 0, 0, 400, 401) == -1
    assert lib.vad_stream_seg_history_elems(0, 8, 0, 0, 400, 160) == 0
    assert lib.vad_stream_seg_state_bytes(-5) == 0
