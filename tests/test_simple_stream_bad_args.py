"""vad_simple_stream_init / _block_f32 / _block_i16 / _state refuse bad
arguments before any HIP call, so every case runs without a device: the
buffer addresses below are never dereferenced, and an accepted call would
crash on them."""
import pytest

E = -1  # VAD_EINVAL
N = None
FR, STATE, LAB, FEAT, VO, VLEN = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
S, K, L, NB = 4, 3, 400, 5
BLOCKS = ["vad_simple_stream_block_f32", "vad_simple_stream_block_i16"]


@pytest.fixture(scope="module")
def lib():
    from vad_amd import _lib
    return _lib.lib()


def block(lib, fn, **kw):
    a = dict(frames=FR, bs=S * L, ss=L, L=L, fft=512, pad=56, bins=32, S=S, K=K, nb=NB, state=STATE, labels=LAB,
             lbs=S, feats=N, voiced=N, vs=K * L, vlen=N)
    a.update(kw)
    return getattr(lib, fn)(a["frames"], a["bs"], a["ss"], a["L"], a["fft"], a["pad"], a["bins"], a["S"], a["K"],
                            a["nb"], a["state"], a["labels"], a["lbs"], a["feats"], a["voiced"], a["vs"], a["vlen"],
                            N)


@pytest.mark.parametrize("fn", BLOCKS)
def test_block_entries_refuse(lib, fn):
    for kw in [dict(frames=N), dict(state=N), dict(labels=N),
               dict(S=0), dict(S=-1), dict(K=-1),
               dict(nb=0), dict(nb=-1), dict(nb=65),
               dict(L=1, fft=1, pad=0), dict(L=0, fft=0, pad=0), dict(L=-400),
               dict(L=8193, fft=8193, pad=0, ss=8193, bs=S * 8193, vs=K * 8193),   # frames above the limit
               dict(L=8191, fft=8195, pad=2, ss=8191, bs=S * 8191),                # L above the limit
               dict(fft=511), dict(fft=513), dict(pad=-1, fft=398), dict(pad=57),  # fft_len != frame_len + 2 pad
               dict(bins=0), dict(bins=-1), dict(bins=129),                         # 4 * band_bins > L: "FFTN is small"
               dict(ss=L - 1), dict(ss=0), dict(ss=-L),                             # two streams' frames overlap
               dict(bs=0), dict(bs=-S * L), dict(bs=S * L - 1),                     # two blocks' frames overlap
               dict(bs=L, ss=K * L - 1), dict(bs=L - 1, ss=K * L),                  # stream-major rows overlap
               dict(lbs=S - 1), dict(lbs=0), dict(lbs=-S),                          # label rows overlap
               dict(voiced=VO), dict(vlen=VLEN),                                    # one without the other
               dict(voiced=VO, vlen=VLEN, vs=K * L - 1), dict(voiced=VO, vlen=VLEN, vs=0),
               dict(state=STATE + 4)]:
        assert block(lib, fn, **kw) == E, kw
    # nothing to do: success, nothing written
    assert block(lib, fn, K=0) == 0
    assert block(lib, fn, K=0, feats=FEAT, voiced=VO, vlen=VLEN) == 0
    # a bad argument stays bad when there is nothing to do
    assert block(lib, fn, K=0, nb=0) == E and block(lib, fn, K=0, frames=N) == E and block(lib, fn, K=0, S=0) == E
    assert block(lib, fn, K=0, bins=129) == E and block(lib, fn, K=0, labels=N) == E
    # one frame: the block strides are not used
    assert block(lib, fn, K=0, bs=0, lbs=0) == 0


def test_lengths_the_one_kernel_form_does_not_take(lib):
    odd = dict(L=401, fft=513, pad=56, ss=401, bs=S * 401, vs=K * 401)
    big = dict(L=8192, fft=8192, pad=0, bins=512, ss=8192, bs=S * 8192, vs=K * 8192)
    for geo in (odd, big):
        # int16 input with such a length
        assert block(lib, BLOCKS[1], feats=FEAT, **geo) == E
        assert block(lib, BLOCKS[1], feats=FEAT, K=0, **geo) == E
        # fp32: the two-launch path needs features_out as its workspace
        assert block(lib, BLOCKS[0], **geo) == E
        assert block(lib, BLOCKS[0], feats=FEAT, K=0, **geo) == 0


def test_state_entry_refuses(lib):
    def state(**kw):
        a = dict(feats=FEAT, S=S, K=K, nb=NB, state=STATE, labels=LAB, lbs=S)
        a.update(kw)
        return lib.vad_simple_stream_state(a["feats"], a["S"], a["K"], a["nb"], a["state"], a["labels"], a["lbs"], N)

    for kw in [dict(feats=N), dict(state=N), dict(labels=N), dict(S=0), dict(S=-1), dict(K=-1), dict(nb=0),
               dict(nb=65), dict(lbs=S - 1), dict(lbs=0), dict(state=STATE + 4)]:
        assert state(**kw) == E, kw
    assert state(K=0) == 0 and state(K=0, nb=0) == E and state(K=0, feats=N) == E


def test_init_entry_refuses(lib):
    def init(**kw):
        a = dict(feats=FEAT, S=S, nb=NB, state=STATE)
        a.update(kw)
        return lib.vad_simple_stream_init(a["feats"], a["S"], a["nb"], a["state"], N)

    for kw in [dict(feats=N), dict(state=N), dict(S=0), dict(S=-1), dict(nb=0), dict(nb=65), dict(state=STATE + 4)]:
        assert init(**kw) == E, kw
    assert lib.vad_simple_stream_state_bytes(0) == 0 and lib.vad_simple_stream_state_bytes(65) == 0
    assert lib.vad_simple_stream_state_bytes(5) == 304
