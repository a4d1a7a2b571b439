"""The resampling entries refuse bad arguments with VAD_EINVAL before any HIP
call (no GPU here; the device pointers below are never dereferenced), and do
nothing, successfully, for an empty destination, zero streams or zero hops.

The clip tables of vad_resample_batch_* live in device memory, as those of
vad_batch_pack_* do, so the host cannot compare their content with ``total``:
tables that overrun it are cut at ``total`` by the kernel
(tests/test_gpu_resample.py::test_tables_that_overrun_total_are_cut); what
the host can see of ``total`` (negative, beyond any buffer) is refused here."""
import ctypes

import numpy as np
import pytest

E = -1  # VAD_EINVAL
N = None  # NULL
PTR, LEN, STA, DST, INP, STATE, OUT = 0x10000, 0x20000, 0x30000, 0x40000, 0x100000, 0x200000, 0x300000
BATCH = [f"vad_resample_batch_{i}_{o}" for i in ("f32", "i16") for o in ("f32", "i16")]
STREAM = [f"vad_resample_stream_{i}_{o}" for i in ("f32", "i16") for o in ("f32", "i16")]


@pytest.fixture(scope="module")
def lib():
    from vad_amd import _lib
    return _lib.lib()


def create(lib, up, down, n_taps=None, taps=True, out=True):
    mx = max(up, down)
    want = 1 if mx == 1 else 20 * mx + 1
    n = want if n_taps is None else n_taps
    buf = np.zeros(max(n, 1), np.float32)
    h = ctypes.c_void_p()
    rc = lib.vad_resample_plan_create(up, down, buf.ctypes.data if taps else N, n, ctypes.byref(h) if out else N)
    return rc, h


@pytest.fixture(scope="module")
def plan(lib):
    rc, h = create(lib, 1, 3)
    assert rc == 0 and h.value
    yield h
    assert lib.vad_resample_plan_destroy(h) == 0


def test_plan_create_refuses(lib):
    for kw in (dict(up=0, down=3), dict(up=-1, down=3), dict(up=1, down=0), dict(up=1, down=-3),
               dict(up=2, down=6),                      # not reduced
               dict(up=1, down=3, n_taps=60), dict(up=1, down=3, n_taps=62), dict(up=1, down=3, n_taps=0),
               dict(up=1, down=3, n_taps=-1), dict(up=1, down=1, n_taps=21),   # n_taps != 2P+1
               dict(up=1, down=3, taps=False), dict(up=1, down=3, out=False),  # null
               dict(up=16000, down=16001),              # a phase table over the LDS budget
               dict(up=1000, down=1001), dict(up=781, down=1),
               dict(up=1, down=17)):                    # an input tile over the LDS budget
        rc, h = create(lib, **kw)
        assert rc == E and not h.value, kw
    for up, down in ((1, 3), (2, 1), (160, 441), (640, 441), (1, 6), (2, 3), (1, 1), (3, 1), (1, 2), (320, 441)):
        rc, h = create(lib, up, down)
        assert rc == 0 and h.value, (up, down)
        mx = max(up, down)
        P = 0 if mx == 1 else 10 * mx
        assert lib.vad_resample_delay(h) == -(-P // down)
        for n in (0, 1, down - 1, down, down + 1, 10007):
            assert lib.vad_resample_n_out(h, n) == -(-n * up // down)
        assert lib.vad_resample_n_out(h, -1) == -1 and lib.vad_resample_n_out(h, 2 ** 63 - 1) == -1
        assert lib.vad_resample_plan_destroy(h) == 0
    assert lib.vad_resample_plan_destroy(N) == E and lib.vad_resample_plan_upload(N) == E
    assert lib.vad_resample_n_out(N, 5) == -1 and lib.vad_resample_delay(N) == -1
    assert lib.vad_resample_stream_state_bytes(N, 4) == 0


def test_plan_create_at_the_lds_limits(lib):
    """The last plan that fits and the first that does not, at either limit of
    16,384 floats: the input tile (1023 * down + T for up = 1) and the phase
    table (up * (T | 1))."""
    for up, down, n_taps, delay in ((1, 15, 301, 10),         # 240 kHz: 15,345 + 301 = 15,646 floats of input tile
                                    (640, 799, 15981, 10)):   # 19,975 Hz: T = 25, 640 * 25 = 16,000 floats of table
        rc, h = create(lib, up, down)
        assert rc == 0 and h.value, (up, down)
        assert 20 * max(up, down) + 1 == n_taps and lib.vad_resample_delay(h) == delay
        assert lib.vad_resample_plan_destroy(h) == 0
    for up, down, n_taps in ((1, 16, 321),        # 16,368 + 321 = 16,689 floats of input tile
                             (640, 801, 16021),   # T = 26, rows of 27: 17,280 floats of table
                             (640, 800, 16001)):  # the shortest filter with T = 26 is of no reduced ratio
        assert 20 * max(up, down) + 1 == n_taps
        rc, h = create(lib, up, down)
        assert rc == E and not h.value, (up, down)
    # T = 26 by the tap count alone does not pass as the 640 / 799 plan either
    rc, h = create(lib, 640, 799, n_taps=16001)
    assert rc == E and not h.value


@pytest.mark.parametrize("fn", STREAM)
def test_stream_window_at_the_lds_limit(lib, fn):
    """240 kHz: hops of 2400 samples behind 300 of history; six fit the
    16,384-float window (14,700), seven do not (17,100)."""
    rc, h = create(lib, 1, 15)
    assert rc == 0
    assert lib.vad_resample_stream_state_bytes(h, 3) == 3 * 301 * 4
    for k, want in ((6, 0), (7, E)):  # zero streams: the arguments are checked, nothing is launched
        assert getattr(lib, fn)(h, INP, 2400, 2400, 0, k, 160, STATE, OUT, N) == want, k
    assert getattr(lib, fn)(h, INP, 2400, 4 * 2400, 4, 7, 160, STATE, OUT, N) == E
    assert lib.vad_resample_plan_destroy(h) == 0


@pytest.mark.parametrize("fn", BATCH)
def test_batch_entries_refuse(lib, plan, fn):
    def call(**kw):
        a = dict(plan=plan, ptrs=PTR, lens=LEN, start=STA, n=3, dst=DST, total=4800)
        a.update(kw)
        return getattr(lib, fn)(a["plan"], a["ptrs"], a["lens"], a["start"], a["n"], a["dst"], a["total"], N)

    for kw in (dict(plan=N), dict(ptrs=N), dict(lens=N), dict(start=N), dict(dst=N), dict(n=-1),
               dict(total=-1), dict(total=-160), dict(total=2 ** 62),  # no buffer has that many samples
               dict(dst=DST + 2), dict(dst=DST + 4), dict(dst=DST + 8)):  # dst not 16-byte aligned
        assert call(**kw) == E, kw
    assert call(total=0) == 0 and call(total=0, dst=N, n=0, ptrs=N, lens=N, start=N) == 0
    # a bad argument stays bad when there is nothing to write
    assert call(total=0, n=-1) == E and call(total=0, plan=N) == E and call(total=0, ptrs=N) == E


@pytest.mark.parametrize("fn", STREAM)
def test_stream_entries_refuse(lib, plan, fn):
    S, K, HI, HO = 4, 3, 480, 160

    def call(**kw):
        a = dict(plan=plan, inp=INP, hs=HI, bs=S * HI, S=S, K=K, ho=HO, state=STATE, out=OUT)
        a.update(kw)
        return getattr(lib, fn)(a["plan"], a["inp"], a["hs"], a["bs"], a["S"], a["K"], a["ho"], a["state"], a["out"],
                                N)

    for kw in (dict(plan=N), dict(inp=N), dict(state=N), dict(out=N), dict(S=-1), dict(K=-1), dict(ho=0),
               dict(ho=-160),
               dict(hs=HI - 1), dict(hs=0), dict(hs=-HI),          # rows of one block overlap
               dict(bs=0), dict(bs=-S * HI), dict(bs=S * HI - 1),  # hop-major blocks repeat or overlap
               dict(bs=HI, hs=K * HI - 1),                         # stream-major rows overlap
               dict(K=40),                                         # 40 hops of 480 samples pass the LDS window
               dict(inp=INP + 1), dict(state=STATE + 2), dict(out=OUT + 1),
               dict(out=INP), dict(state=INP), dict(out=STATE)):   # the buffers overlap
        assert call(**kw) == E, kw
    assert call(S=0) == 0 and call(K=0) == 0 and call(S=0, inp=N, state=N, out=N) == 0
    assert call(S=0, ho=0) == E and call(K=0, hs=HI - 1) == E
    assert lib.vad_resample_stream_state_bytes(plan, 0) == 0 and lib.vad_resample_stream_state_bytes(plan, -3) == 0
    # 1 / 3: P = 30, T = 61, d = 10, history = ceil(0 / 1) + 60 samples, and one counter
    assert lib.vad_resample_stream_state_bytes(plan, 5) == 5 * 61 * 4


def test_stream_hop_must_be_whole_input_samples(lib):
    rc, h = create(lib, 640, 441)  # 11025 Hz: 160 outputs are 110.25 input samples
    assert rc == 0
    assert lib.vad_resample_stream_i16_f32(h, INP, 111, 444, 4, 1, 160, STATE, OUT, N) == E
    assert lib.vad_resample_plan_destroy(h) == 0
