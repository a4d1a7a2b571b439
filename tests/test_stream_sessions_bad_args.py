"""The sessions hop entries exist and refuse bad arguments before any HIP call:
a null hop_counts or restart, a partly set denoise state, and what their
denoising siblings refuse ahead of the first look into a plan (the plan and
buffer addresses below are never dereferenced).  StreamBatch's own ValueErrors
that need a batch on a device are marked gpu."""
import os
import re

import pytest

E = -1  # VAD_EINVAL
N = None
PLAN, CLF, FR, HOP, RING, CNT, LAB, SC = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000
SPEC, ROWS, NCNT, EST, HC, RST = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
S, K, L, H = 4, 3, 400, 160
FFN = ["vad_stream_hops_sessions", "vad_stream_hops_sessions_i16"]
TREE = ["vad_stream_hops_tree_sessions", "vad_stream_hops_tree_sessions_i16"]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from vad_amd import _lib
    return _lib.lib()


def hops(lib, fn, **kw):
    a = dict(plan=PLAN, clf=CLF, frames=FR, fs=L, L=L, hop=HOP, hs=H, H=H, S=S, K=K, hbs=S * H, ring=RING, count=CNT,
             labels=LAB, lbs=S, walk=0, active=1, scores=N, sbs=S, spec=SPEC, rows=ROWS, ncnt=NCNT, est=EST, alpha=0.9,
             cls=0, update=1, hc=HC, rst=RST)
    a.update(kw)
    walk = (a["walk"],) if "tree" in fn else ()
    return getattr(lib, fn)(a["plan"], a["clf"], a["frames"], a["fs"], a["L"], a["hop"], a["hs"], a["H"], a["S"],
                            a["K"], a["hbs"], a["ring"], a["count"], a["labels"], a["lbs"], *walk, a["active"],
                            a["scores"], a["sbs"], a["spec"], a["rows"], a["ncnt"], a["est"], a["alpha"], a["cls"],
                            a["update"], a["hc"], a["rst"], N)


NO_DN = dict(spec=N, rows=N, ncnt=N, est=N)


@pytest.mark.parametrize("fn", FFN + TREE)
def test_entries_exist_and_refuse_without_a_device(lib, fn):
    from vad_amd import _lib
    assert fn in _lib.SIGNATURES and getattr(lib, fn) is not None
    cases = [dict(hc=N), dict(rst=N), dict(hc=N, rst=N), dict(hc=N, **NO_DN), dict(rst=N, **NO_DN),
             # a partly set denoise state: any one array missing, any one array alone
             dict(spec=N), dict(rows=N), dict(ncnt=N), dict(est=N),
             dict(rows=N, ncnt=N, est=N), dict(spec=N, ncnt=N, est=N), dict(spec=N, rows=N, est=N),
             dict(spec=N, rows=N, ncnt=N), dict(spec=N, rows=N),
             # what the siblings refuse
             dict(plan=N), dict(clf=N), dict(S=-1), dict(K=-1), dict(L=0), dict(L=1025, fs=1025), dict(H=0),
             dict(H=L + 1, hs=L + 1), dict(fs=L - 1), dict(hs=H - 1), dict(lbs=S - 1), dict(scores=SC, sbs=S - 1),
             dict(hbs=0), dict(hbs=S * H - 1), dict(hbs=H, hs=K * H - 1),
             dict(alpha=1.0), dict(alpha=float("nan")), dict(update=2), dict(cls=-1), dict(rows=SPEC),
             dict(plan=N, **NO_DN), dict(lbs=S - 1, **NO_DN), dict(hbs=0, **NO_DN), dict(K=-1, **NO_DN)]
    if "tree" in fn:
        cases += [dict(walk=2), dict(walk=-1, **NO_DN)]
    for kw in cases:
        assert hops(lib, fn, **kw) == E, kw
    # a bad argument stays bad when there is nothing to do
    assert hops(lib, fn, S=0, hc=N) == E and hops(lib, fn, K=0, rst=N, **NO_DN) == E and hops(lib, fn, S=0, spec=N) == E


def test_no_hop_constant():
    from vad_amd import _lib, stream
    header = open(os.path.join(REPO, "include", "vad_amd.h")).read()
    m = re.search(r"^#define VAD_LABEL_NO_HOP (\d+)", header, re.M)
    assert m and int(m.group(1)) == 254 == stream.LABEL_NO_HOP == _lib.LABEL_NO_HOP
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for fn in FFN + TREE:
        assert re.search(r"\b" + fn + r"\(", header) and fn in integration, fn


def test_three_kernel_form_has_no_sessions():
    from vad_amd.stream import StreamBatch
    with pytest.raises(ValueError, match="three"):  # refused before anything touches a device
        StreamBatch(3, None, sessions=True, kernel="three")


# ---------------------------------------------------------------------------
# with a batch on a device
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_stream_batch_refusals():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from vad_amd.ffn import FFNClassifier, TOPOLOGY_BL13, random_layers
    from vad_amd.stream import StreamBatch
    ffn = FFNClassifier(random_layers(TOPOLOGY_BL13, seed=3))
    with pytest.raises(ValueError, match="three"):
        StreamBatch(3, ffn, sessions=True, kernel="three")
    sb = StreamBatch(3, ffn, sessions=True, hops_per_step=2)
    with pytest.raises(ValueError, match="one window per label row"):
        sb.segmenter()
    cuda = lambda *a, **k: torch.zeros(*a, device="cuda", **k)
    good_c, good_r = cuda(3, dtype=torch.int32), cuda(3, dtype=torch.uint8)
    for bad in (cuda(4, dtype=torch.int32), cuda(3, dtype=torch.int64), cuda(3, 1, dtype=torch.int32),
                torch.zeros(3, dtype=torch.int32), [2, 2, 2]):
        with pytest.raises(ValueError, match="hop_counts"):
            sb.step_block(hop_counts=bad, restart=good_r)
    for bad in (cuda(2, dtype=torch.uint8), cuda(3, dtype=torch.bool), cuda(3, dtype=torch.int32),
                torch.zeros(3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="restart"):
            sb.step_block(hop_counts=good_c, restart=bad)
    one = StreamBatch(3, ffn, sessions=True)
    with pytest.raises(ValueError, match="hop_counts"):
        one.step(hop_counts=cuda(2, dtype=torch.int32))
    # a refused call copies nothing and runs nothing
    torch.cuda.synchronize()
    assert bool((sb.hop_counts == 2).all()) and not bool(sb.restart.any()) and not bool(sb.count.any())
    plain = StreamBatch(3, ffn)
    with pytest.raises(ValueError, match="sessions=True"):
        plain.step(hop_counts=good_c)
    assert not hasattr(plain, "hop_counts") and not hasattr(plain, "restart")  # nothing more allocated
    sb.step_block(hop_counts=good_c + 1, restart=good_r)  # the accepted call runs
    torch.cuda.synchronize()
    assert bool((sb.count == 1).all()) and bool((sb.label_block[1] == 254).all())
