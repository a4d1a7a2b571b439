"""The tree-training entries refuse bad arguments before any HIP call (no GPU
here; the pointers below are never dereferenced)."""
import ctypes

import pytest

E, EUNSUP = -1, -2
N = None
X, Y, ORD, MASK, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x100000
TAB = [0x1000000 + 0x100000 * i for i in range(11)]


@pytest.fixture(scope="module")
def tt():
    from vad_amd import _lib, tree_train
    return _lib.lib(), tree_train


def jobs_of(tt, specs):
    arr = (tt[1]._Job * len(specs))()
    for i, s in enumerate(specs):
        d = dict(n_rows=100, node_capacity=9, max_depth=5, min_samples_split=22, min_samples_leaf=20, reserved=0)
        d.update(s)
        arr[i] = tt[1]._Job(**d)
    return arr


def train(tt, specs=({},), tables=None, **kw):
    lib, mod = tt
    a = dict(x=X, y=Y, n=100, F=5, K=3, order=ORD, mask=MASK, J=len(specs), ws=WS, ws_bytes=1 << 40, jobs=True)
    a.update(kw)
    jobs = jobs_of(tt, specs) if a["jobs"] else None
    tb = mod._Tables(*(TAB if tables is None else tables))
    return lib.vad_tree_train(a["x"], a["y"], a["n"], a["F"], a["K"], a["order"], a["mask"], a["J"], jobs,
                              ctypes.byref(tb) if tables != "null" else None, a["ws"], a["ws_bytes"], None, N)


SHAPES = [dict(n=0), dict(n=-1), dict(n=1 << 27), dict(F=0), dict(F=65), dict(K=1), dict(K=9), dict(J=0), dict(J=-1),
          dict(J=4097), dict(jobs=False)]
JOBS = [dict(n_rows=0), dict(n_rows=101), dict(max_depth=0), dict(min_samples_split=1), dict(min_samples_leaf=0),
        dict(reserved=1), dict(node_capacity=0), dict(node_capacity=(1 << 28) + 1), dict(n_rows=-5)]


def test_train_refuses(tt):
    for kw in SHAPES + [dict(x=N), dict(y=N), dict(order=N), dict(ws=N), dict(ws=WS + 8), dict(ws_bytes=0),
                        dict(ws_bytes=1024)]:
        assert train(tt, **kw) == E, kw
    for spec in JOBS:
        assert train(tt, specs=({}, spec)) == E, spec
    for i in range(11):
        tables = list(TAB)
        tables[i] = None
        assert train(tt, tables=tables) == E, i
    tables = list(TAB)
    tables[1] += 4  # thresholds are doubles
    assert train(tt, tables=tables) == E
    # without a mask every job takes every row
    assert train(tt, mask=N, specs=(dict(n_rows=99),)) == E
    # more than 1024 jobs of a single row
    assert train(tt, specs=tuple(dict(n_rows=1, node_capacity=1) for _ in range(1025))) == E
    # all jobs' rows together must stay below 2^31
    big = tuple(dict(n_rows=(1 << 27) - 1, node_capacity=1) for _ in range(17))
    assert train(tt, n=(1 << 27) - 1, specs=big) == EUNSUP


def test_sizing_entries_refuse(tt):
    lib = tt[0]
    assert lib.vad_tree_train_node_capacity(0, 1) == -1
    assert lib.vad_tree_train_node_capacity(10, 0) == -1
    assert lib.vad_tree_train_node_capacity(-1, 5) == -1

    def ws(specs=({},), n=100, F=5, K=3, J=None, jobs=True):
        arr = jobs_of(tt, specs) if jobs else None
        return lib.vad_tree_train_workspace_bytes(n, F, K, len(specs) if J is None else J, arr)

    assert ws() > 0 and ws() % 256 == 0
    assert ws(({}, {})) > ws()
    for kw in SHAPES:
        kw = {k: v for k, v in kw.items()}
        assert ws(**kw) == 0, kw
    for spec in JOBS:
        assert ws(specs=(spec,)) == 0, spec
    assert ws(n=(1 << 27) - 1, specs=tuple(dict(n_rows=(1 << 27) - 1, node_capacity=1) for _ in range(17))) == 0
