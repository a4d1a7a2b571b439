"""The forest hop entries exist and refuse bad arguments before any HIP call
(the plan, forest and buffer addresses below are never dereferenced), and
ForestStreamBatch refuses what it cannot run before it touches a device.  The
refusals that need a real plan and forest (the feature count, `active` and
`noise_class` against the forest's classes) are marked gpu."""
import os
import re

import numpy as np
import pytest

import forest_reference as FR

E = -1  # VAD_EINVAL
N = None
PLAN, CLF, FR_, HOP, RING, CNT, LAB, SC = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000
SPEC, ROWS, NCNT, EST, HC, RST = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
S, K, L, H = 4, 3, 400, 160
FNS = ["vad_stream_hops_forest", "vad_stream_hops_forest_i16"]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DN = dict(spec=N, rows=N, ncnt=N, est=N)
NO_SESS = dict(hc=N, rst=N)


@pytest.fixture(scope="module")
def lib():
    from vad_amd import _lib
    return _lib.lib()


def hops(lib, fn, **kw):
    a = dict(plan=PLAN, clf=CLF, frames=FR_, fs=L, L=L, hop=HOP, hs=H, H=H, S=S, K=K, hbs=S * H, ring=RING, count=CNT,
             labels=LAB, lbs=S, walk=0, active=1, scores=N, sbs=S, spec=SPEC, rows=ROWS, ncnt=NCNT, est=EST, alpha=0.9,
             cls=0, update=1, hc=HC, rst=RST)
    a.update(kw)
    return getattr(lib, fn)(a["plan"], a["clf"], a["frames"], a["fs"], a["L"], a["hop"], a["hs"], a["H"], a["S"],
                            a["K"], a["hbs"], a["ring"], a["count"], a["labels"], a["lbs"], a["walk"], a["active"],
                            a["scores"], a["sbs"], a["spec"], a["rows"], a["ncnt"], a["est"], a["alpha"], a["cls"],
                            a["update"], a["hc"], a["rst"], N)


@pytest.mark.parametrize("fn", FNS)
def test_entries_exist_and_refuse_without_a_device(lib, fn):
    from vad_amd import _lib
    assert fn in _lib.SIGNATURES and getattr(lib, fn) is not None
    cases = [dict(plan=N), dict(clf=N), dict(S=-1), dict(K=-1), dict(L=0), dict(L=1025, fs=1025), dict(H=0),
             dict(H=L + 1, hs=L + 1), dict(fs=L - 1), dict(hs=H - 1), dict(lbs=S - 1), dict(scores=SC, sbs=S - 1),
             dict(hbs=0), dict(hbs=S * H - 1), dict(hbs=H, hs=K * H - 1), dict(walk=2), dict(walk=-1),
             # hop_counts without restart, or the reverse
             dict(hc=N), dict(rst=N), dict(hc=N, **NO_DN), dict(rst=N, **NO_DN),
             # a partly set denoise state, and its options
             dict(spec=N), dict(rows=N), dict(ncnt=N), dict(est=N), dict(rows=N, ncnt=N, est=N),
             dict(spec=N, rows=N), dict(rows=SPEC), dict(alpha=1.0), dict(alpha=float("nan")), dict(update=2),
             dict(cls=-1),
             # `active` below 0, with scores or without
             dict(active=-1), dict(active=-1, scores=SC), dict(active=-1, **NO_DN, **NO_SESS)]
    dn_keys = set(NO_DN) | {"alpha", "update", "cls"}
    for kw in cases:
        assert hops(lib, fn, **kw) == E, kw
        # the same refusal in the other forms of the entry: without sessions, without denoising (whose own
        # arguments are then not read)
        if not set(NO_SESS) & set(kw):
            assert hops(lib, fn, **{**kw, **NO_SESS}) == E, kw
        if not dn_keys & set(kw):
            assert hops(lib, fn, **{**kw, **NO_DN}) == E, kw
    # a bad argument stays bad when there is nothing to do
    assert hops(lib, fn, S=0, hc=N) == E and hops(lib, fn, K=0, walk=3) == E and hops(lib, fn, S=0, spec=N) == E


def test_queries_refuse_null_handles(lib):
    assert lib.vad_stream_hop_forest_table_bytes(N, CLF, 0) == E
    assert lib.vad_stream_hop_forest_table_bytes(PLAN, N, 0) == E
    assert lib.vad_stream_hop_forest_table_bytes(N, N, 1) == E
    assert lib.vad_stream_forest_lds_trees(N, CLF) == E
    assert lib.vad_stream_forest_lds_trees(PLAN, N) == E


def test_header_and_integration_name_the_entries():
    header = open(os.path.join(REPO, "include", "vad_amd.h")).read()
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for fn in FNS + ["vad_stream_hop_forest_table_bytes", "vad_stream_forest_lds_trees"]:
        assert re.search(r"\b" + fn + r"\(", header) and fn in integration, fn


def small_forest(F=39, K=2):
    from vad_amd.forest import ForestClassifier
    from vad_amd.tree import TreeClassifier
    trees = []
    for i, n in enumerate((7, 1, 15)):
        t = FR.random_tree(n, F, K, seed=i)
        trees.append(TreeClassifier(t["feature"], t["threshold"], t["left"], t["right"], t["leaf"], t["nan_left"],
                                    np.arange(K), F, proba=t["proba"]))
    return ForestClassifier.from_trees(trees)


def test_forest_stream_batch_refuses_before_a_device():
    import vad_amd
    from vad_amd.stream import ForestStreamBatch, StreamBatch
    assert vad_amd.ForestStreamBatch is ForestStreamBatch and issubclass(ForestStreamBatch, StreamBatch)
    forest = small_forest()
    with pytest.raises(ValueError, match="three"):
        ForestStreamBatch(4, forest, kernel="three")
    for active in (-1, 2):
        with pytest.raises(ValueError, match="active"):
            ForestStreamBatch(4, forest, scores=True, active=active)
        with pytest.raises(ValueError, match="active"):
            ForestStreamBatch(4, forest, active=active)
    for cls in (-1, 2):
        with pytest.raises(ValueError, match="noise_class"):
            ForestStreamBatch(4, forest, denoise=True, noise_class=cls)
    with pytest.raises(ValueError, match="features"):
        ForestStreamBatch(4, small_forest(F=40))
    with pytest.raises(ValueError, match="tree_walk"):
        ForestStreamBatch(4, forest, tree_walk="lds")
    with pytest.raises(TypeError):
        ForestStreamBatch(4, object())
    with pytest.raises(ValueError, match="forest"):  # existing behaviour: StreamBatch itself keeps refusing
        StreamBatch(4, forest)


# ---------------------------------------------------------------------------
# with a plan and a forest on a device
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_entries_refuse_with_a_plan_and_a_forest():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from vad_amd import _lib
    from vad_amd.stream import ForestStreamBatch
    lib = _lib.lib()
    sb = ForestStreamBatch(S, small_forest(), hops_per_step=K, scores=True, denoise=True, sessions=True)
    wide = small_forest(F=40).plan  # 40 features: more than 3 * 13
    p = _lib.ptr
    good = dict(plan=sb.plan.handle, clf=sb.ffn.plan.handle, frames=p(sb.frames), hop=p(sb.inputs), ring=p(sb.ring),
                count=p(sb.count), labels=p(sb.label_block), scores=p(sb.score_block), spec=p(sb._spec),
                rows=p(sb._noise), ncnt=p(sb.noise_count), est=p(sb._est), hc=p(sb.hop_counts), rst=p(sb.restart))
    for fn in FNS:
        for kw in (dict(active=2), dict(active=2, scores=N), dict(cls=2), dict(clf=wide.handle),
                   dict(clf=wide.handle, S=0), dict(frames=N), dict(hop=N), dict(ring=N), dict(count=N),
                   dict(labels=N)):
            assert hops(lib, fn, **{**good, **kw}) == E, (fn, kw)
        assert hops(lib, fn, **{**good, "S": 0}) == 0 and hops(lib, fn, **{**good, "K": 0}) == 0
    assert lib.vad_stream_forest_lds_trees(sb.plan.handle, sb.ffn.plan.handle) == 3 == sb.lds_trees
    nb = lib.vad_stream_hop_forest_table_bytes(sb.plan.handle, sb.ffn.plan.handle, 0)
    assert nb == lib.vad_stream_hop_forest_table_bytes(sb.plan.handle, sb.ffn.plan.handle, 1) + 16 * 23
    assert lib.vad_stream_hop_forest_table_bytes(sb.plan.handle, sb.ffn.plan.handle, 2) == E
    torch.cuda.synchronize()
    assert not sb.count.any()  # nothing ran
