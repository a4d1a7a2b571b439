"""TreeTrainer at the grid shapes and edges the other tree-training tests do
not reach, every node table bitwise against the numpy model of the rule
(tests/tree_train_reference.py), thresholds as doubles:

  1  tt_search with several features per workgroup (fc = 2, 3, 4; full and
     partial last chunks), with and without feature masks, against the model
     and against the same job run alone (fc = 1);
  2  scores that tie among the features of a chunk and among chunks;
  3  K = 4 and 5, the two sides of the one-word / two-word class counters,
     and masked jobs at K = 4, 5, 8;
  4  row counts at tile borders;
  5  tiles that meet 1,024 and 1,025 segments (the LDS table holds 1,026);
  6  node capacity at the exact node count and one below it;
  7  +-0, subnormals and +-FLT_MAX neighbours as feature values.

Rows come from tree_train_reference.synth unless a case says otherwise
(tests/tree_train_shape_cases.py builds the others)."""
import ctypes
import functools

import numpy as np
import pytest

import tree_train_reference as R
import tree_train_shape_cases as C

pytestmark = pytest.mark.gpu

TILE = 2048  # restates kTile of csrc/tree_train_kernel.hip
N = 2 * TILE + 37
DEEP = 1000  # a depth the data never reaches


def search_shape(T, F):
    """(NT, ny, fc, features in the last chunk) of tt_search's grid for lists
    of T entries and F features: restates the four lines of make_layout in
    csrc/tree_train_kernel.hip.  The cases assert the shape they are named
    for before they run, so a retuned layout fails here and does not silently
    fall back to one feature per workgroup."""
    NT = -(-T // TILE)
    ny = max(1, min(F, -(-2048 // NT)))
    fc = -(-F // ny)
    ny = -(-F // fc)
    return NT, ny, fc, F - (ny - 1) * fc


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def table(tree):
    return {k: getattr(tree, k) for k in R.KEYS}


def assert_same(got, want, what):
    got = got if isinstance(got, dict) else table(got)
    bad = R.tables_equal(got, want)
    assert bad is None, f"{what}: '{bad}' differs ({len(got['feature'])} nodes, model {len(want['feature'])})"


# ---- 1. feature-chunk grid shapes ----------------------------------------------
# Every job has N rows, so a call of J jobs has lists of T = J * N entries.  The
# jobs are the training rows of fold 0 or 1 of a 3-fold split of M = 6,200 rows
# (6,200 - 2,067 = N rows each); the J jobs of a call are copies of four
# distinct ones in rotating order, so four model fits serve a call.
M = 6200
FOUR = [(0, DEEP, 2, 1), (1, DEEP, 2, 1), (0, DEEP, 2, 20), (1, 3, 22, 20)]  # (fold, md, mss, msl)

#        F,  K,  J,  (NT, ny, fc, features in the last chunk)
SHAPES = [(64, 8, 16, (33, 32, 2, 2)),
          (64, 8, 40, (81, 22, 3, 1)),
          (64, 8, 64, (130, 16, 4, 4)),
          (39, 3, 27, (55, 20, 2, 1))]


@functools.lru_cache(maxsize=None)
def big_rows(F, K):
    return R.synth(M, F, K, 5)


@functools.lru_cache(maxsize=None)
def fold_rows(fold):
    from vad_amd.tree_train import kfold
    r = kfold(M, 3)[fold][0]
    assert len(r) == N
    return r


@functools.lru_cache(maxsize=None)
def four_model(F, K, i, feats=None):
    x, y = big_rows(F, K)
    fold, md, mss, msl = FOUR[i]
    return C.model(x, y, K, md, mss, msl, rows=fold_rows(fold), feats=None if feats is None else np.asarray(feats))


def four_job(i, feats=None):
    fold, md, mss, msl = FOUR[i]
    return (fold_rows(fold), md, mss, msl) + (() if feats is None else (np.asarray(feats),))


_calls = {}


def big_call(F, K, J):
    """The trees of the J-job call, trained once per module run."""
    if (F, K, J) not in _calls:
        from vad_amd.tree_train import TreeTrainer
        x, y = big_rows(F, K)
        _calls[F, K, J] = TreeTrainer().fit_many(x, y, [four_job(j % 4) for j in range(J)])
    return _calls[F, K, J]


@pytest.mark.parametrize("F,K,J,shape", SHAPES)
def test_feature_chunks_equal_the_model(torch_cuda, F, K, J, shape):
    assert search_shape(J * N, F) == shape and shape[2] > 1
    got = big_call(F, K, J)
    assert len(got) == J
    for j, g in enumerate(got):
        assert_same(g, four_model(F, K, j % 4), f"job {j} of {J} (F {F}, K {K}, shape {shape})")
    deep = four_model(F, K, 0)
    assert deep["depth"].max() < DEEP and len(deep["feature"]) > 50


@pytest.mark.parametrize("F,K,J", [(64, 8, 64), (39, 3, 27)])
def test_a_job_alone_equals_itself_among_many(torch_cuda, F, K, J):
    """Alone the job is searched one feature per workgroup, in the large call
    several: the same table for any grid shape."""
    from vad_amd.tree_train import TreeTrainer
    assert search_shape(N, F)[2] == 1 and search_shape(J * N, F)[2] > 1
    x, y = big_rows(F, K)
    among = big_call(F, K, J)
    for i in (1, 2):
        alone = TreeTrainer().fit_many(x, y, [four_job(i)])[0]
        assert_same(alone, four_model(F, K, i), f"job {i} alone")
        for j in range(i, J, 4):
            assert_same(among[j], table(alone), f"job {j} among {J} against job {i} alone")


def feature_subsets(F):
    """Two small subsets and two of F - 1 features.  Column F - 4 is a copy of
    column 0 (synth), so leaving 0 out moves its wins to F - 4."""
    return [(0, 5, F - 2), (1, 4, F - 4), tuple(f for f in range(F) if f != 1), tuple(range(1, F))]


def masked_jobs(F, J):
    """Every second job takes a feature subset, the four in turn (four model
    fits: the deep job of fold 1 with 3 and with F - 1 features, the shallow
    one with the other two)."""
    subs = feature_subsets(F)
    return [(j % 4, subs[(j // 2) % 4] if j % 2 else None) for j in range(J)]


@pytest.mark.parametrize("F,K,J,shape", [SHAPES[0], SHAPES[3]])
def test_masked_feature_chunks_equal_the_model(torch_cuda, F, K, J, shape):
    """Feature subsets under chunking; at K = 8 the two-word masked search."""
    from vad_amd.tree_train import TreeTrainer
    assert search_shape(J * N, F) == shape and shape[2] > 1
    fc = shape[2]
    plan = masked_jobs(F, J)
    assert [s is not None for _, s in plan] == [bool(j % 2) for j in range(J)]
    # next to each other in the lists (the job before, the masked job after):
    # some chunk holds a feature only one of the two may use and another that
    # one of them may use, so the chunk's loop goes on with mixed segments
    everything = set(range(F))
    for j in range(1, J, 2):
        sa = set(plan[j][1])
        for other in (j - 1, j - 2, j + 1):
            if 0 <= other < J:
                sb = everything if plan[other][1] is None else set(plan[other][1])
                assert any(len((sa ^ sb) & set(range(c, c + fc))) >= 1 and len((sa | sb) & set(range(c, c + fc))) >= 2
                           for c in range(0, F, fc)), (j, other)
    assert {len(s) for _, s in plan if s is not None} == {3, F - 1}
    x, y = big_rows(F, K)
    got = TreeTrainer().fit_many(x, y, [four_job(i, s) for i, s in plan])
    for j, ((i, s), g) in enumerate(zip(plan, got)):
        assert_same(g, four_model(F, K, i, s), f"job {j} of {J}, features {s if s is None or len(s) == 3 else 'F - 1'}")
        if s is not None:
            assert set(g.feature[g.feature >= 0].tolist()) <= set(s)
    assert len(four_model(F, K, 1, plan[1][1])["feature"]) > 3


# ---- 2. ties inside and across chunks --------------------------------------------
@functools.lru_cache(maxsize=None)
def tie_case(K):
    x, y, pattern = C.tie_rows(K)
    want = R.fit(x, y, K, DEEP, 2, 1)
    return x, y, pattern, want


@pytest.mark.parametrize("J,fc", [(16, 2), (64, 4)])
@pytest.mark.parametrize("K", [3, 5])
def test_ties_inside_and_across_chunks(torch_cuda, K, J, fc):
    """64 columns that repeat the seven tie columns: every distinct column
    recurs in several chunks and beside its copies in one chunk, and the
    winner is the lowest index of each: 1, 2 or 5."""
    from vad_amd.tree_train import TreeTrainer
    x, y, pattern, want = tie_case(K)
    assert search_shape(J * N, 64)[2] == fc
    assert len(np.unique(y)) == K and x.shape == (N, 64)
    # each of the seven recurs, and some chunk holds two copies of one column
    assert all((pattern[7:] == i).sum() >= 2 for i in range(7))
    assert any(len(set(pattern[c:c + fc])) < fc for c in range(0, 64, fc))
    assert set(want["feature"].tolist()) == {-1, 1, 2, 5} and len(want["feature"]) > 50
    got = TreeTrainer().fit_many(x, y, [(None, DEEP, 2, 1)] * J)
    for j, g in enumerate(got):
        assert set(g.feature.tolist()) <= {-1, 1, 2, 5}, f"job {j}: split features {sorted(set(g.feature.tolist()))}"
        assert_same(g, want, f"job {j} of {J}, K {K}")


# ---- 3. the class-count word border ----------------------------------------------
@functools.lru_cache(maxsize=None)
def rows(F, K, n=N, seed=5):
    return R.synth(n, F, K, seed)


@pytest.mark.parametrize("md,mss,msl", [(DEEP, 2, 1), (3, 22, 20)])
@pytest.mark.parametrize("K", [4, 5])
def test_four_and_five_classes_equal_the_model(torch_cuda, K, md, mss, msl):
    from vad_amd.tree_train import TreeTrainer
    x, y = rows(13, K)
    assert len(np.unique(y)) == K
    want = R.fit(x, y, K, md, mss, msl)
    assert_same(TreeTrainer(md, mss, msl).fit(x, y), want, (K, md, mss, msl))
    if md == DEEP:
        assert want["depth"].max() < DEEP and len(want["feature"]) > 50


@pytest.mark.parametrize("md,mss,msl", [(DEEP, 2, 1), (4, 22, 20)])
@pytest.mark.parametrize("K", [4, 5, 8])
def test_a_feature_subset_at_four_five_and_eight_classes(torch_cuda, K, md, mss, msl):
    """The masked single job of test_gpu_forest_train.py on three tiles."""
    from vad_amd.tree_train import TreeTrainer
    F = 13
    x, y = rows(F, K)
    pick = np.random.default_rng
    for feats in (np.sort(pick(1).choice(F, F // 3, replace=False)), np.sort(pick(2).choice(F, F - 1, replace=False)),
                  [F - 2, 0]):
        got = TreeTrainer().fit_many(x, y, [(None, md, mss, msl, feats)])[0]
        want = C.model(x, y, K, md, mss, msl, feats=np.sort(np.asarray(feats)))
        assert_same(got, want, (K, list(feats)))
        assert set(got.feature[got.feature >= 0].tolist()) <= set(int(f) for f in feats)
        assert len(want["feature"]) > 3


# ---- 4. row counts at tile borders ------------------------------------------------
@pytest.mark.parametrize("md,mss,msl", [(DEEP, 2, 1), (DEEP, 22, 20)])
@pytest.mark.parametrize("n", [2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1])
def test_row_counts_at_tile_borders(torch_cuda, n, md, mss, msl):
    from vad_amd.tree_train import TreeTrainer
    x, y = rows(13, 3, n)
    # with two or three rows a class may be absent: TreeTrainer counts the classes present
    want = C.model_of_present_classes(x, y, md, mss, msl)
    if n >= TILE - 1:
        assert len(np.unique(y)) == 3 and R.tables_equal(want, R.fit(x, y, 3, md, mss, msl)) is None
        assert len(want["feature"]) > 9
    assert_same(TreeTrainer(md, mss, msl).fit(x, y), want, (n, md, mss, msl))


@pytest.mark.parametrize("md,mss,msl", [(DEEP, 2, 1), (DEEP, 22, 20)])
def test_a_job_border_one_entry_past_a_tile_border(torch_cuda, md, mss, msl):
    """Jobs of 2,049 and 2,047 rows: the second begins at entry 2,049 and the
    lists end on a tile border."""
    from vad_amd.tree_train import TreeTrainer
    x, y = rows(13, 3, 2 * TILE)
    sets = [np.arange(TILE + 1), np.arange(TILE + 1, 2 * TILE)]
    got = TreeTrainer().fit_many(x, y, [(r, md, mss, msl) for r in sets])
    for j, (r, g) in enumerate(zip(sets, got)):
        want = R.fit(x, y, 3, md, mss, msl, rows=r)
        assert len(want["feature"]) > 9
        assert_same(g, want, f"job {j} of {len(r)} rows")


# ---- 5. the densest tile ---------------------------------------------------------
def test_tiles_that_meet_1024_and_1025_segments(torch_cuda):
    """2,100 jobs of 3, 2, 2, ... rows in one call.  At level 0 tile 0 meets
    1,024 segments; tile 1 meets 1,025: the first carried in with one row (it
    reports through the tile's slot), the last straddling out."""
    from vad_amd.tree_train import TreeTrainer
    x, y, sets = C.dense_rows(2100)
    assert x.shape == (4201, 2) and [len(r) for r in sets[:3]] == [3, 2, 2]
    meet = C.segments_meeting_tiles(np.array([len(r) for r in sets]))
    assert meet[0] == (1024, 0) and meet[1] == (1025, 1) and len(meet) == 3
    assert meet[1][0] <= TILE // 2 + 2  # restates kSegLds
    want = [R.fit(x, y, 2, DEEP, 2, 1, rows=r) for r in sets]
    split = sum(len(w["feature"]) > 1 for w in want)
    assert 0.4 * len(sets) < split < 0.6 * len(sets)
    got = TreeTrainer().fit_many(x, y, [(r, DEEP, 2, 1) for r in sets])
    assert len(got) == len(sets)
    for j, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, f"job {j} of {len(sets)}")


# ---- 6. capacity at the exact node count ------------------------------------------
def test_node_capacity_at_the_exact_count_and_one_below(torch_cuda):
    from vad_amd import _lib
    from vad_amd._lib import VadError
    from vad_amd.tree_train import _TABLES, _Job, _Tables, TreeTrainer
    torch = torch_cuda
    F, K = 13, 2
    x, y = rows(F, K)
    want = R.fit(x, y, K, DEEP, 2, 1)
    c = len(want["feature"])
    assert c > 50
    got = TreeTrainer().fit_many(x, y, [(None, DEEP, 2, 1)], node_capacity=c)[0]
    assert_same(got, want, f"capacity {c}, the node count")
    with pytest.raises(VadError):
        TreeTrainer().fit_many(x, y, [(None, DEEP, 2, 1)], node_capacity=c - 1)
    # the raw entry one node short: the status, the count and the guard words
    lib = _lib.lib()
    cap, guard = c - 1, 64
    X, Y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    order = torch.sort(X.t().contiguous(), dim=1, stable=True).indices.to(torch.int32).contiguous()
    desc = (_Job * 1)(_Job(N, cap, DEEP, 2, 1, 0))
    need = lib.vad_tree_train_workspace_bytes(N, F, K, 1, desc)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = {}
    for k, dt in _TABLES:
        size = 1 if k in ("n_nodes", "status") else cap * (K if k == "value" else 1)
        out[k] = torch.full((size + guard,), 0x5a if dt == torch.uint8 else -12345, dtype=dt, device="cuda")
    tb = _Tables(*(out[k].data_ptr() for k, _ in _TABLES))
    rc = lib.vad_tree_train(X.data_ptr(), Y.data_ptr(), N, F, K, order.data_ptr(), None, 1, desc, ctypes.byref(tb),
                            ws.data_ptr(), need, None, _lib.stream_ptr())
    assert rc == _lib.VAD_ENOMEM
    assert int(out["status"][0]) & 1 and 1 <= int(out["n_nodes"][0]) <= cap
    for k, dt in _TABLES:
        tail = out[k][-guard:].cpu().numpy()
        assert (tail == (0x5a if dt == torch.uint8 else -12345)).all(), k


# ---- 7. finite float edges ----------------------------------------------------------
@pytest.mark.parametrize("md,mss,msl", [(DEEP, 2, 1), (4, 22, 20)])
def test_signed_zeros_subnormals_and_flt_max(torch_cuda, md, mss, msl):
    """Columns of -0.0 / +0.0 (equal: no candidate), of zeros and 2^-149,
    of k * 2^-149 and of +-FLT_MAX with their neighbours: `v > pv` must keep
    subnormals apart and zeros together, and the threshold is the double sum."""
    from vad_amd.tree_train import TreeTrainer
    x, y = C.edge_rows()
    col = C.EDGE_COLUMNS
    assert x.shape == (N, 17) and np.isfinite(x).all()
    assert set(np.signbit(x[:, col["zeros"]]).tolist()) == {False, True} and not x[:, col["zeros"]].any()
    assert set(x[:, col["zeros_subnormal"]].tolist()) == {0.0, float(C.TINY)}
    assert set(np.signbit(x[x[:, col["zeros_subnormal"]] == 0, col["zeros_subnormal"]]).tolist()) == {False, True}
    assert set((x[:, col["subnormals"]].astype(np.float64) * 2.0 ** 149).tolist()) == set(range(8))
    assert len(set(x[:, col["flt_max"]].tolist())) == 4 and np.abs(x[:, col["flt_max"]]).min() > 3.4e38
    want = R.fit(x, y, 3, md, mss, msl)
    f = want["feature"]
    assert not (f == col["zeros"]).any()
    if md == DEEP:
        for name in ("zeros_subnormal", "subnormals", "flt_max"):
            assert (f == col[name]).any(), f"the model never splits on the {name} column"
        assert (want["threshold"][f == col["zeros_subnormal"]] == 2.0 ** -150).all()
        assert 0.0 in want["threshold"][f == col["flt_max"]].tolist()
    assert_same(TreeTrainer(md, mss, msl).fit(x, y), want, (md, mss, msl))
