"""int16 PCM hop input for the streaming path, and the HostPipeline.

The hop kernels convert an int16 sample with an exact (float) where they load
it and run the same code afterwards, so an int16 batch must leave the labels
and the state (frames, ring, count) of the fp32 batch fed the same values,
bit for bit: every comparison here is torch.equal, no tolerance.  The clips
are oracle.synth_clip's (integer-valued within +-32767: the int16 and fp32
inputs are made from one array).  The pipeline (depth blocks in flight on
three streams) must give the labels and final state of serial single-hop
steps on device inputs.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

from oracle import vad_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@functools.lru_cache(maxsize=None)
def _clf():
    from vad_amd.ffn import FFNClassifier
    w = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ffn.npz"), allow_pickle=False)
    return FFNClassifier([(w[f"ref39_W{i}"], w[f"ref39_b{i}"]) for i in range(4)])


@functools.lru_cache(maxsize=None)
def _audio(S, T, L=400, H=160, seed=1200):
    """carry (S, L-H) and hops (T, S, H) as float32 numpy, integer-valued."""
    keep = L - H
    clips = np.stack([O.synth_clip(H * T + keep, seed=seed + s)[:H * T + keep] for s in range(S)])
    carry = np.ascontiguousarray(clips[:, :keep])
    hops = np.ascontiguousarray(np.stack([clips[:, keep + H * t: keep + H * (t + 1)] for t in range(T)]))
    assert np.array_equal(hops, hops.astype(np.int16).astype(np.float32))
    return carry, hops


@functools.lru_cache(maxsize=None)
def _serial(kernel, S, T):
    """Serial single-hop fp32 device-input steps: labels (T, S), frames, ring,
    count.  Computed once per (kernel, S, T); never written afterwards."""
    import torch
    from vad_amd.stream import StreamBatch
    carry, hops = _audio(S, T)
    ref = StreamBatch(S, _clf(), kernel=kernel)
    ref.prime(torch.from_numpy(carry).cuda())
    dh = torch.from_numpy(hops).cuda()
    want = torch.stack([ref.step(dh[t]).clone() for t in range(T)])
    torch.cuda.synchronize()
    return want, ref.frames.clone(), ref.ring.clone(), ref.count.clone()


def _run(sb, dh, K, graph):
    """All of dh (T, S, H) through sb in blocks of K; the labels (T, S)."""
    import torch
    if graph:
        sb.capture()
    got = []
    for b in range(dh.shape[0] // K):
        blk = dh[b * K:(b + 1) * K]
        if K == 1:
            got.append(sb.step(blk[0]).clone()[None])
        elif graph:
            sb.inputs.copy_(blk)
            got.append(sb.step_block().clone())
        else:
            got.append(sb.step_block(blk).clone())
    return torch.cat(got)


def _assert_same_state(a, b):
    import torch
    assert torch.equal(a.frames, b.frames)
    assert torch.equal(a.ring, b.ring)
    assert torch.equal(a.count, b.count)


CASES = [("hop", 1), ("hop", 2), ("hop", 8), ("three", 1), ("three", 3)]


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("S", [1, 5, 24])
@pytest.mark.parametrize("kernel,K", CASES)
def test_int16_equals_fp32_bitwise(torch_cuda, kernel, K, S, graph):
    """An int16 batch and an fp32 batch on the same values: labels, frames,
    ring and count identical, launched directly and replayed from a graph."""
    torch = torch_cuda
    from vad_amd.stream import StreamBatch
    T = max(6 * K, 16) // K * K
    carry, hops = _audio(S, T)
    out = []
    for dt in (torch.float32, torch.int16):
        sb = StreamBatch(S, _clf(), kernel=kernel, hops_per_step=K, input_dtype=dt)
        assert sb.inputs.dtype == dt and sb.hop_in.dtype == dt and sb.frames.dtype == torch.float32
        sb.prime(torch.from_numpy(carry).cuda().to(dt))
        out.append((sb, _run(sb, torch.from_numpy(hops).cuda().to(dt), K, graph)))
    (f32, lab32), (i16, lab16) = out
    assert torch.equal(lab16, lab32), int((lab16 != lab32).sum())
    _assert_same_state(i16, f32)
    assert (lab32[:5] == 255).all() and (lab32[5:] != 255).all()
    want = _serial(kernel, S, T)
    assert torch.equal(lab16, want[0]) and torch.equal(i16.frames, want[1])


def test_int16_extreme_samples(torch_cuda):
    """-32768 and 32767 in the first and last sample of several hop rows."""
    torch = torch_cuda
    from vad_amd.stream import StreamBatch
    S, K, T = 5, 8, 16
    carry, hops = _audio(S, T)
    h16 = hops.astype(np.int16)
    for t, s in ((0, 0), (3, 4), (7, 2), (8, 1), (15, 4)):
        h16[t, s, 0], h16[t, s, -1] = -32768, 32767
    for t, s in ((1, 3), (9, 0)):
        h16[t, s, 0], h16[t, s, -1] = 32767, -32768
    out = []
    for dt in (torch.float32, torch.int16):
        sb = StreamBatch(S, _clf(), hops_per_step=K, input_dtype=dt)
        sb.prime(torch.from_numpy(carry).cuda())  # a float32 carry for both
        out.append((sb, _run(sb, torch.from_numpy(h16).cuda().to(dt), K, False)))
    (f32, lab32), (i16, lab16) = out
    assert torch.equal(lab16, lab32)
    _assert_same_state(i16, f32)
    assert i16.frames.min().item() == -32768.0 or i16.frames.max().item() == 32767.0


def test_int16_step_checks_dtype(torch_cuda):
    torch = torch_cuda
    from vad_amd.stream import StreamBatch
    sb = StreamBatch(3, _clf(), input_dtype=torch.int16)
    with pytest.raises(ValueError, match="int16"):
        sb.step(torch.zeros((3, 160), device="cuda"))
    sb8 = StreamBatch(3, _clf(), hops_per_step=2, input_dtype=torch.int16)
    with pytest.raises(ValueError, match="int16"):
        sb8.step_block(torch.zeros((2, 3, 160), device="cuda"))
    with pytest.raises(ValueError):
        StreamBatch(3, _clf(), input_dtype=torch.float64)


@pytest.mark.parametrize("frame_size,hop", [(401, 161), (1000, 333)])
def test_int16_odd_geometry(torch_cuda, frame_size, hop):
    """Odd frame and hop lengths (the NR = 7 and the NR = 16 build), the hop
    block a view into a larger int16 buffer at an odd element offset with an
    odd row stride: rows only 2-byte aligned, read in place."""
    torch = torch_cuda
    from vad_amd.config import MfccConfig
    from vad_amd.stream import StreamBatch
    cfg = MfccConfig(frame_size=frame_size, hop=hop)
    S, K, nb = 5, 4, 4
    T = K * nb
    carry, hops = _audio(S, T, frame_size, hop, seed=1300)
    f32 = StreamBatch(S, _clf(), cfg=cfg, hops_per_step=K)
    i16 = StreamBatch(S, _clf(), cfg=cfg, hops_per_step=K, input_dtype=torch.int16)
    f32.prime(torch.from_numpy(carry).cuda())
    i16.prime(torch.from_numpy(carry.astype(np.int16)).cuda())
    rs = hop + 2 if hop % 2 else hop + 3  # odd row stride
    assert rs % 2 == 1
    big = torch.full((7 + K * S * rs + 8,), 12345, dtype=torch.int16, device="cuda")
    view = big[7:7 + K * S * rs].view(K, S, rs)[:, :, :hop]
    assert view.data_ptr() % 4 == 2 and view.stride() == (S * rs, rs, 1)
    dh = torch.from_numpy(hops).cuda()
    for b in range(nb):
        blk = dh[b * K:(b + 1) * K]
        want = f32.step_block(blk).clone()
        view.copy_(blk.to(torch.int16))
        got = i16.step_block(view).clone()  # read in place (disjoint rows, unit sample stride)
        assert torch.equal(got, want), (b, int((got != want).sum()))
    _assert_same_state(i16, f32)
    assert (i16.count > 5).all()
    # one hop from an odd address too (vad_stream_hop_i16's layout)
    one32 = StreamBatch(S, _clf(), cfg=cfg)
    one16 = StreamBatch(S, _clf(), cfg=cfg, input_dtype=torch.int16)
    for t in range(6):
        want = one32.step(dh[t]).clone()
        view[0].copy_(dh[t].to(torch.int16))
        assert torch.equal(one16.step(view[0]), want)
    _assert_same_state(one16, one32)


def test_int16_stream_major_layout(torch_cuda):
    """An (S, K * hop) int16 buffer viewed as (K, S, hop) is read in place
    (StreamBatch and the C ABI, rc 0); an overlapping row stride is refused
    with VAD_EINVAL and nothing runs."""
    torch = torch_cuda
    from vad_amd import _lib
    from vad_amd.stream import StreamBatch, hop_rows_disjoint
    S, K, nb = 5, 4, 4
    T = K * nb
    carry, hops = _audio(S, T)
    want, frames, ring, count = _serial("hop", S, T)
    per_stream = torch.from_numpy(np.ascontiguousarray(hops.transpose(1, 0, 2).reshape(S, T * 160))
                                  .astype(np.int16)).cuda()
    sb = StreamBatch(S, _clf(), hops_per_step=K, input_dtype=torch.int16)
    sb.prime(torch.from_numpy(carry).cuda())
    got = []
    for b in range(nb):
        blk = per_stream[:, 160 * K * b:160 * K * (b + 1)].contiguous().view(S, K, 160).transpose(0, 1)
        assert blk.stride() == (160, K * 160, 1) and hop_rows_disjoint(S, K, 160, K * 160, 160)
        got.append(sb.step_block(blk).clone())
    assert torch.equal(torch.cat(got), want)
    assert torch.equal(sb.frames, frames) and torch.equal(sb.ring, ring) and torch.equal(sb.count, count)
    L = _lib.lib()
    fresh = StreamBatch(S, _clf(), hops_per_step=K, input_dtype=torch.int16)
    ok = per_stream[:, :160 * K].contiguous()
    args = (fresh.plan.handle, fresh.ffn.plan.handle, _lib.ptr(fresh.frames), 400, 400, _lib.ptr(ok))
    tail = (_lib.ptr(fresh.ring), _lib.ptr(fresh.count), _lib.ptr(fresh.label_block), S, _lib.stream_ptr())
    assert L.vad_stream_hops_i16(*args, K * 160 - 1, 160, S, K, 160, *tail) == _lib.VAD_EINVAL
    assert (fresh.count == 0).all()  # nothing ran
    assert L.vad_stream_hops_i16(*args, K * 160, 160, S, K, 160, *tail) == 0
    assert (fresh.count == K).all()
    assert torch.equal(fresh.label_block, want[:K])


def test_int16_against_oracle(torch_cuda):
    """test_stream_hop_narrow_networks' setup fed as int16: labels equal the
    fp64 oracle's wherever its top-2 margin exceeds 1e-3 (more than 95% of
    the windows, a property of the oracle alone)."""
    torch = torch_cuda
    from vad_amd.ffn import FFNClassifier, random_layers
    from vad_amd.stream import StreamBatch
    S, T = 8, 40
    layers = random_layers((13, 64, 64, 2), seed=11)
    clips = [O.synth_clip(160 * (T - 1) + 401, seed=700 + s) for s in range(S)]
    fb = O.get_mel_filterbanks(300, 8000, 512, 26, 16000)
    sb = StreamBatch(S, FFNClassifier(layers), kernel="hop", input_dtype=torch.int16)
    sb.prime(torch.from_numpy(np.stack([c[:240] for c in clips]).astype(np.int16)).cuda())
    got = []
    for t in range(T):
        new = np.stack([c[240 + 160 * t: 400 + 160 * t] for c in clips]).astype(np.int16)
        got.append(sb.step(torch.from_numpy(new).cuda()).cpu().numpy().copy())
    got = np.stack(got, axis=1)[:, 5:]  # (S, T-5)
    n_ok = 0
    for s, c in enumerate(clips):
        x = O.analyser_features_fast(O.mfcc_batch(c, fb))[:, :13]
        ok = O.ffn_margin(x, layers) > 1e-3
        np.testing.assert_array_equal(got[s][ok], O.ffn_labels(x, layers)[ok])
        n_ok += int(ok.sum())
    assert n_ok > 0.95 * got.size


@pytest.mark.parametrize("K,graph", [(1, False), (1, True), (8, False), (8, True)])
def test_int16_host_io(torch_cuda, K, graph):
    """step_host from int16 pinned memory, direct and captured with its
    copies: the host labels equal the device-input fp32 single-hop steps."""
    torch = torch_cuda
    from vad_amd.stream import StreamBatch
    S, nb = 24, 4
    T = K * nb
    carry, hops = _audio(S, 48)
    want = _serial("hop", S, 48)[0][:T].cpu()
    sb = StreamBatch(S, _clf(), hops_per_step=K, input_dtype=torch.int16)
    sb.prime(torch.from_numpy(carry).cuda())
    if graph:
        sb.capture(host_io=True)
    else:
        sb.attach_host_io()
    assert sb.host_inputs.dtype == torch.int16 and sb.host_inputs.is_pinned()
    assert tuple(sb.host_inputs.shape) == (K, S, 160)
    h16 = torch.from_numpy(hops.astype(np.int16))
    got = []
    for b in range(nb):
        sb.host_inputs.copy_(h16[b * K:(b + 1) * K])
        lab = sb.step_host()
        torch.cuda.current_stream().synchronize()
        got.append(lab.clone())
    got = torch.cat(got)
    assert torch.equal(got, want), int((got != want).sum())


def _drive_pipeline(torch, sb, depth, hops_host, K):
    """Keep `depth` blocks in flight: block b + depth - 1 is submitted before
    block b is waited on; a slot's host input is overwritten with 0x7f bytes
    right after its wait, so a copy-in that ran late would read those."""
    pipe = sb.host_pipeline(depth)
    nb = hops_host.shape[0] // K
    assert nb >= 2 * depth + 1

    def put(b):
        d = b % depth
        pipe.host_inputs[d].copy_(hops_host[b * K:(b + 1) * K])
        pipe.submit(d)

    for b in range(min(depth - 1, nb)):
        put(b)
    got = []
    for b in range(nb):
        nxt = b + depth - 1
        if nxt < nb:
            put(nxt)
        d = b % depth
        lab = pipe.wait(d)
        assert lab is pipe.host_labels[d]
        got.append(lab.clone())
        pipe.host_inputs[d].view(torch.uint8).fill_(0x7f)
    pipe.drain()
    return pipe, torch.cat(got)


PIPE_CASES = [("hop", 24, K, depth, dt) for depth in (1, 2, 3) for K in (1, 8) for dt in ("float32", "int16")]
PIPE_CASES += [("hop", 512, 8, 2, "int16"), ("three", 24, 3, 2, "int16"), ("three", 24, 1, 2, "float32")]


@pytest.mark.parametrize("kernel,S,K,depth,dtype", PIPE_CASES)
def test_host_pipeline_equals_serial_steps(torch_cuda, kernel, S, K, depth, dtype):
    torch = torch_cuda
    from vad_amd.stream import HostPipeline, StreamBatch
    dt = getattr(torch, dtype)
    nb = 5 if S == 512 else max(2 * depth + 1, -(-16 // K))  # every slot reused, and at least 16 hops
    T = K * nb
    carry, hops = _audio(S, T)
    want, frames, ring, count = _serial(kernel, S, T)
    sb = StreamBatch(S, _clf(), kernel=kernel, hops_per_step=K, input_dtype=dt)
    sb.prime(torch.from_numpy(carry).cuda())
    hops_host = torch.from_numpy(hops).to(dt)
    pipe, got = _drive_pipeline(torch, sb, depth, hops_host, K)
    assert isinstance(pipe, HostPipeline) and pipe.depth == depth
    for d in range(depth):
        assert pipe.host_inputs[d].dtype == dt and pipe.host_inputs[d].is_pinned()
        assert tuple(pipe.host_inputs[d].shape) == (K, S, 160)
        assert pipe.host_labels[d].dtype == torch.uint8 and pipe.host_labels[d].is_pinned()
        assert tuple(pipe.host_labels[d].shape) == (K, S)
    assert torch.equal(got, want.cpu()), int((got != want.cpu()).sum())
    assert (got[:5] == 255).all() and (got[5:] != 255).all()
    assert torch.equal(sb.frames, frames) and torch.equal(sb.ring, ring) and torch.equal(sb.count, count)


def test_host_pipeline_depth1_equals_step_host(torch_cuda):
    torch = torch_cuda
    from vad_amd.stream import StreamBatch
    S, K, nb = 24, 8, 3
    carry, hops = _audio(S, K * nb)
    h16 = torch.from_numpy(hops.astype(np.int16))
    a = StreamBatch(S, _clf(), hops_per_step=K, input_dtype=torch.int16)
    b = StreamBatch(S, _clf(), hops_per_step=K, input_dtype=torch.int16)
    for sb in (a, b):
        sb.prime(torch.from_numpy(carry).cuda())
    a.attach_host_io()
    pipe = b.host_pipeline(depth=1)
    for i in range(nb):
        a.host_inputs.copy_(h16[i * K:(i + 1) * K])
        la = a.step_host()
        torch.cuda.current_stream().synchronize()
        pipe.host_inputs[0].copy_(h16[i * K:(i + 1) * K])
        pipe.submit(0)
        assert torch.equal(pipe.wait(0), la)
    pipe.drain()
    _assert_same_state(a, b)


def test_host_pipeline_misuse(torch_cuda):
    torch = torch_cuda
    from vad_amd.stream import StreamBatch
    sb = StreamBatch(4, _clf(), hops_per_step=2)
    with pytest.raises(ValueError):
        sb.host_pipeline(depth=0)
    pipe = sb.host_pipeline(depth=2)
    with pytest.raises(ValueError):
        pipe.wait(0)  # nothing in flight
    pipe.submit(0)
    with pytest.raises(ValueError):
        pipe.submit(0)  # submitted and not waited
    pipe.submit(1)
    pipe.wait(0)
    pipe.submit(0)
    pipe.drain()
    assert (sb.count == 6).all()


@pytest.fixture(scope="module")
def poison(torch_cuda):
    torch = torch_cuda
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_host", "liblds_poison.so")
    if not os.path.exists(so):
        pytest.fail("tests/c_host/liblds_poison.so missing: run __graft_entry__.build()")
    helper = ctypes.CDLL(so)
    helper.lds_poison.argtypes = [ctypes.c_float, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    sink = torch.zeros(1, device="cuda")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count

    def fill(v):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert helper.lds_poison(v, ctypes.c_void_p(sink.data_ptr()), 4 * n_cu, st) == 0

    yield fill
    torch.cuda.synchronize()
    assert sink.item() == 0.0  # every poison launch read back its own LDS stores


def test_int16_hop_kernel_ignores_stale_lds(torch_cuda, poison):
    """The int16 hop kernel at K = 8, every launch preceded by a kernel that
    filled every CU's LDS with a hostile value: labels and state identical to
    a clean run, bit for bit."""
    torch = torch_cuda
    from vad_amd.stream import StreamBatch
    S, K, T = 300, 8, 16
    carry, hops = _audio(S, T, seed=1400)
    dh = torch.from_numpy(hops.astype(np.int16)).cuda()
    outs = []
    for v in (None, 1e30, -1e30, float("nan")):
        sb = StreamBatch(S, _clf(), hops_per_step=K, input_dtype=torch.int16)
        sb.prime(torch.from_numpy(carry).cuda())
        labs = []
        for t in range(0, T, K):
            if v is not None:
                poison(v)
            labs.append(sb.step_block(dh[t:t + K]).clone())
        outs.append([torch.cat(labs).cpu(), sb.frames.view(torch.int32).cpu(), sb.ring.view(torch.int32).cpu(),
                     sb.count.cpu()])
    for o in outs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(o, outs[0]))
