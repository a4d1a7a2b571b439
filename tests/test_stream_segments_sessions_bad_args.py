"""The sessions entries of the streaming segmenter refuse what their siblings
refuse, and a missing or misaligned hop_counts, restart, end_voiced, end_len or
table_session, with VAD_EINVAL before any HIP call (no GPU here; the pointers
below are never dereferenced); and the Python layer's refusals."""
import pytest

E = -1  # VAD_EINVAL
N = None  # NULL
LAB, ST, SEG, FND = 0x10000, 0x20000, 0x30000, 0x40000
HOP, HIS, VOI, VLN = 0x100000, 0x200000, 0x300000, 0x400000
CNT, RST, EVO, ELN, TSE = 0x500000, 0x600000, 0x700000, 0x800000, 0x900000
S, K, L, H = 4, 3, 400, 160
PB = 2
RING = (0 + 1 + 1 + 1 + PB + 3 + K) * H + L  # elements one stream needs with pad_before = PB (enough without)


@pytest.fixture(scope="module")
def lib():
    from vad_amd import _lib
    return _lib.lib()


def call(lib, fn, **kw):
    a = dict(labels=LAB, scores=0, lbs=S, S=S, K=K, active=1, gap=0, run=0, L=L, H=H, on=0.6, off=0.4, pb=PB, pa=1,
             state=ST, seg=SEG, cap=8, found=FND, hop=HOP, hs=H, hbs=S * H, hist=HIS, helems=S * RING, voiced=VOI,
             vlen=VLN, counts=CNT, restart=RST, evoiced=EVO, elen=ELN, tsess=TSE)
    a.update(kw)
    op = "_op_" in fn
    audio = fn.endswith(("_f32", "_i16"))
    args = [a["labels"]] + ([a["scores"]] if op else []) + [a["lbs"], a["S"], a["K"], a["active"], a["gap"], a["run"],
                                                            a["L"], a["H"]]
    args += [a["on"], a["off"], a["pb"], a["pa"]] if op else []
    args += [a["state"], a["seg"], a["cap"], a["found"]]
    args += [a["hop"], a["hs"], a["hbs"], a["hist"], a["helems"], a["voiced"], a["vlen"]] if audio else []
    args += [a["counts"], a["restart"]] + ([a["evoiced"]] if audio else []) + [a["elen"], a["tsess"], N]
    return getattr(lib, fn)(*args)


SIBLING = [dict(H=0), dict(H=-160), dict(H=L + 1), dict(L=0), dict(gap=-1), dict(run=-1), dict(cap=-1), dict(S=-1),
           dict(state=N), dict(found=N), dict(seg=N), dict(K=-1), dict(active=255), dict(active=-1), dict(labels=N),
           dict(lbs=S - 1), dict(state=ST + 4), dict(found=FND + 4)]
SIBLING_AUDIO = [dict(hop=N), dict(hist=N), dict(voiced=N), dict(vlen=N), dict(hs=H - 1), dict(hbs=0),
                 dict(hbs=S * H - 1), dict(helems=S * ((0 + 1 + 1 + 1 + 3 + K) * H + L) - 1), dict(helems=-1),
                 dict(helems=S * ((1 << 30) + 1)), dict(hist=HIS + 1), dict(voiced=VOI + 1), dict(vlen=VLN + 2)]
SIBLING_OP = [dict(on=1.5), dict(off=-0.1), dict(on=0.3, off=0.4), dict(on=float("nan")), dict(pb=-1), dict(pa=-1),
              dict(scores=2), dict(scores=1, labels=LAB + 2)]
SESSIONS = [dict(counts=N), dict(restart=N), dict(elen=N), dict(tsess=N), dict(counts=CNT + 2), dict(elen=ELN + 2),
            dict(tsess=TSE + 1)]
SESSIONS_AUDIO = [dict(evoiced=N), dict(evoiced=EVO + 1)]

ENTRIES = ["vad_stream_segments_sessions", "vad_stream_segments_sessions_f32", "vad_stream_segments_sessions_i16",
           "vad_stream_segments_op_sessions", "vad_stream_segments_op_sessions_f32",
           "vad_stream_segments_op_sessions_i16"]


@pytest.mark.parametrize("fn", ENTRIES)
def test_sessions_entries_refuse(lib, fn):
    audio = fn.endswith(("_f32", "_i16"))
    cases = SIBLING + SESSIONS + (SIBLING_AUDIO + SESSIONS_AUDIO if audio else []) + (SIBLING_OP if "_op_" in fn else [])
    for kw in cases:
        assert call(lib, fn, **kw) == E, (fn, kw)
    # nothing to do: VAD_OK, and nothing would be used
    assert call(lib, fn, S=0) == 0 and call(lib, fn, K=0) == 0
    assert call(lib, fn, S=0, counts=N, restart=N, elen=N, tsess=N, evoiced=N, state=N, found=N, seg=N) == 0
    # a bad argument stays bad when there is nothing to do
    assert call(lib, fn, S=0, H=0) == E and call(lib, fn, K=0, active=255) == E
    # no table, no ordinals: table_session is not used at capacity 0
    assert call(lib, fn, cap=0, seg=N, tsess=N, S=0) == 0


def test_the_sibling_of_each_entry_takes_the_same_arguments(lib):
    """The sessions entry with its five pointers dropped is the sibling's call."""
    from vad_amd import _lib
    for fn in ENTRIES:
        sib = _lib.SIGNATURES[fn.replace("_sessions", "")][1]
        mine = _lib.SIGNATURES[fn][1]
        extra = 5 if fn.endswith(("_f32", "_i16")) else 4
        assert list(mine[:len(sib) - 1]) == list(sib[:-1]) and len(mine) == len(sib) + extra, fn


def test_python_refusals():
    import torch
    from vad_amd.stream_segments import StreamSegmenter
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="sessions=True"):
        StreamSegmenter(4, device=cpu, hop_counts=torch.zeros(4, dtype=torch.int32))
    for bad in (torch.zeros(4, dtype=torch.int64), torch.zeros(3, dtype=torch.int32),
                torch.zeros((4, 2), dtype=torch.int32)[:, 0], [3, 3, 3, 3]):
        with pytest.raises(ValueError, match="hop_counts"):
            StreamSegmenter(4, device=cpu, sessions=True, hop_counts=bad)
    seg = StreamSegmenter(4, device=cpu, sessions=True)
    for kw in (dict(hop_counts=torch.zeros(4, dtype=torch.int32)), dict(restart=torch.zeros(4, dtype=torch.uint8))):
        with pytest.raises(ValueError, match="must be a CUDA"):  # a host tensor
            seg._set_sessions(kw.get("hop_counts"), kw.get("restart"))
    plain = StreamSegmenter(4, device=cpu)
    with pytest.raises(ValueError, match="sessions=True"):
        plain._set_sessions(None, torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="sessions=True"):
        plain.session_segments()
