"""vad_simple_stream_block_sessions_f32 / _i16 and
vad_simple_stream_state_sessions refuse bad arguments before any HIP call,
as their siblings do, so every case runs without a device: the buffer
addresses below are never dereferenced.  And the Python class's ValueErrors
that need no device."""
import os
import re

import pytest

E = -1  # VAD_EINVAL
N = None
FR, STATE, LAB, FEAT, VO, VLEN = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
CNT, RST, LEFT = 0x70000, 0x80001, 0x90000     # restart: bytes, any alignment
S, K, L, NB = 4, 3, 400, 5
BLOCKS = ["vad_simple_stream_block_sessions_f32", "vad_simple_stream_block_sessions_i16"]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from vad_amd import _lib
    return _lib.lib()


def block(lib, fn, **kw):
    a = dict(frames=FR, bs=S * L, ss=L, L=L, fft=512, pad=56, bins=32, S=S, K=K, nb=NB, state=STATE, labels=LAB,
             lbs=S, feats=N, voiced=N, vs=K * L, vlen=N, cnt=CNT, rst=RST, left=LEFT)
    a.update(kw)
    return getattr(lib, fn)(a["frames"], a["bs"], a["ss"], a["L"], a["fft"], a["pad"], a["bins"], a["S"], a["K"],
                            a["nb"], a["state"], a["labels"], a["lbs"], a["feats"], a["voiced"], a["vs"], a["vlen"],
                            a["cnt"], a["rst"], a["left"], N)


SESSION_WORDS = [dict(cnt=N), dict(rst=N), dict(left=N), dict(cnt=N, rst=N, left=N),
                 dict(cnt=CNT + 1), dict(cnt=CNT + 2), dict(left=LEFT + 1), dict(left=LEFT + 2)]


@pytest.mark.parametrize("fn", BLOCKS)
def test_block_entries_refuse(lib, fn):
    # everything the plain entries refuse (tests/test_simple_stream_bad_args.py), with good session words
    for kw in [dict(frames=N), dict(state=N), dict(labels=N),
               dict(S=0), dict(S=-1), dict(K=-1),
               dict(nb=0), dict(nb=-1), dict(nb=65),
               dict(L=1, fft=1, pad=0), dict(L=0, fft=0, pad=0), dict(L=-400),
               dict(L=8193, fft=8193, pad=0, ss=8193, bs=S * 8193, vs=K * 8193),
               dict(L=8191, fft=8195, pad=2, ss=8191, bs=S * 8191),
               dict(fft=511), dict(fft=513), dict(pad=-1, fft=398), dict(pad=57),
               dict(bins=0), dict(bins=-1), dict(bins=129),
               dict(ss=L - 1), dict(ss=0), dict(ss=-L),
               dict(bs=0), dict(bs=-S * L), dict(bs=S * L - 1),
               dict(bs=L, ss=K * L - 1), dict(bs=L - 1, ss=K * L),
               dict(lbs=S - 1), dict(lbs=0), dict(lbs=-S),
               dict(voiced=VO), dict(vlen=VLEN),
               dict(voiced=VO, vlen=VLEN, vs=K * L - 1), dict(voiced=VO, vlen=VLEN, vs=0),
               dict(state=STATE + 4)]:
        assert block(lib, fn, **kw) == E, kw
    # the session words: null, or an int32 array that is not 4-byte aligned
    for kw in SESSION_WORDS:
        assert block(lib, fn, **kw) == E, kw
        assert block(lib, fn, K=0, **kw) == E, kw       # bad stays bad when there is nothing to do
    # nothing to do: success before any launch, so no flag is read or consumed
    assert block(lib, fn, K=0) == 0
    assert block(lib, fn, K=0, feats=FEAT, voiced=VO, vlen=VLEN) == 0
    assert block(lib, fn, K=0, rst=RST + 1) == 0       # restart is bytes: any alignment
    assert block(lib, fn, K=0, nb=0) == E and block(lib, fn, K=0, frames=N) == E and block(lib, fn, K=0, S=0) == E
    assert block(lib, fn, K=0, bs=0, lbs=0) == 0


def test_lengths_the_one_kernel_form_does_not_take(lib):
    odd = dict(L=401, fft=513, pad=56, ss=401, bs=S * 401, vs=K * 401)
    big = dict(L=8192, fft=8192, pad=0, bins=512, ss=8192, bs=S * 8192, vs=K * 8192)
    for geo in (odd, big):
        assert block(lib, BLOCKS[1], feats=FEAT, **geo) == E
        assert block(lib, BLOCKS[1], feats=FEAT, K=0, **geo) == E
        assert block(lib, BLOCKS[0], **geo) == E
        assert block(lib, BLOCKS[0], feats=FEAT, K=0, **geo) == 0
        assert block(lib, BLOCKS[0], feats=FEAT, K=0, cnt=N, **geo) == E


def test_state_entry_refuses(lib):
    def state(**kw):
        a = dict(feats=FEAT, S=S, K=K, nb=NB, state=STATE, labels=LAB, lbs=S, cnt=CNT, rst=RST, left=LEFT)
        a.update(kw)
        return lib.vad_simple_stream_state_sessions(a["feats"], a["S"], a["K"], a["nb"], a["state"], a["labels"],
                                                    a["lbs"], a["cnt"], a["rst"], a["left"], N)

    for kw in [dict(feats=N), dict(state=N), dict(labels=N), dict(S=0), dict(S=-1), dict(K=-1), dict(nb=0),
               dict(nb=65), dict(lbs=S - 1), dict(lbs=0), dict(state=STATE + 4)] + SESSION_WORDS:
        assert state(**kw) == E, kw
    for kw in SESSION_WORDS:
        assert state(K=0, **kw) == E, kw
    assert state(K=0) == 0 and state(K=0, nb=0) == E and state(K=0, feats=N) == E


def test_header_binding_and_docs_agree():
    from vad_amd import _lib
    header = open(os.path.join(REPO, "include", "vad_amd.h")).read()
    m = re.search(r"^#define VAD_LABEL_INIT (\d+)", header, re.M)
    assert m and int(m.group(1)) == 253 == _lib.LABEL_INIT
    assert _lib.LABEL_NO_HOP == 254
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for fn, sib in (("vad_simple_stream_block_sessions_f32", "vad_simple_stream_block_f32"),
                    ("vad_simple_stream_block_sessions_i16", "vad_simple_stream_block_i16"),
                    ("vad_simple_stream_state_sessions", "vad_simple_stream_state")):
        assert fn in _lib.SIGNATURES and fn in integration and re.search(r"\b" + fn + r"\(", header)
        mine, theirs = _lib.SIGNATURES[fn][1], _lib.SIGNATURES[sib][1]
        assert mine[:len(theirs) - 1] == theirs[:-1] and len(mine) == len(theirs) + 3   # ..., three words, stream


def test_python_value_errors_that_need_no_device():
    """sessions= exists, and the constants are the header's.  (The tensor
    checks need CUDA tensors: tests/test_gpu_simple_stream_sessions.py.)"""
    import inspect

    from vad_amd import simple_stream as SS
    assert SS.LABEL_INIT == 253 and SS.LABEL_NO_HOP == 254
    assert inspect.signature(SS.SimpleStreamBatch.__init__).parameters["sessions"].default is False
    assert inspect.signature(SS.SimpleStreamBatch.from_analysers).parameters["sessions"].default is False
    for name in ("step", "step_block"):
        p = inspect.signature(getattr(SS.SimpleStreamBatch, name)).parameters
        assert list(p)[1:] == ["frames", "frame_counts", "restart"]
        assert all(p[k].default is None for k in ("frames", "frame_counts", "restart"))
    # _set_sessions on an object that has no device tensors: the class's checks, in order
    sb = SS.SimpleStreamBatch.__new__(SS.SimpleStreamBatch)
    sb.sessions = False
    sb._set_sessions(None, None)                       # nothing given: nothing to check
    with pytest.raises(ValueError, match="sessions=True"):
        sb._set_sessions(object(), None)
    with pytest.raises(ValueError, match="sessions=True"):
        sb._set_sessions(None, object())
    import torch
    sb.sessions = True
    sb.frame_counts = torch.zeros(4, dtype=torch.int32)
    sb.restart = torch.zeros(4, dtype=torch.uint8)
    for bad in (torch.zeros(4, dtype=torch.int32),     # right dtype and shape, not on the device
                torch.zeros(3, dtype=torch.int32), torch.zeros(4, dtype=torch.int64), [1, 2, 3, 4]):
        with pytest.raises(ValueError, match="frame_counts must be a CUDA int32 tensor of shape \\(4,\\)"):
            sb._set_sessions(bad, None)
    for bad in (torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.bool), torch.zeros((4, 1), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="restart must be a CUDA uint8 tensor of shape \\(4,\\)"):
            sb._set_sessions(None, bad)
