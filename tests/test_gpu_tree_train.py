"""TreeTrainer on the device against the numpy model of the rule
(tests/tree_train_reference.py): every array of the node table bitwise,
thresholds as doubles.

Rows: n = 2 tiles + 37 (a tile is 2048 list entries), so that the root spans
three tiles, segments cross tile borders at every level, and deep levels put
many segments into one tile.  The synthetic columns (tree_train_reference.
synth) hold a constant column, one of 0.5 + j * 2^-24, two- and few-valued
columns, a copy of column 0 (an exact score tie between features) and a
permuted copy."""
import ctypes
import functools
import os

import numpy as np
import pytest

import tree_train_reference as R

pytestmark = pytest.mark.gpu

TILE = 2048
N = 2 * TILE + 37
DEEP = 1000  # a depth the data never reaches


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@functools.lru_cache(maxsize=None)
def rows(F, K, seed=5, n=N):
    return R.synth(n, F, K, seed)


@functools.lru_cache(maxsize=None)
def model(F, K, md, mss, msl, seed=5, n=N, sub=None):
    x, y = rows(F, K, seed, n)
    return R.fit(x, y, K, md, mss, msl, rows=None if sub is None else subset(sub, n))


def subset(sub, n=N):
    """A fold's training rows (sub = (fold, k)), or for sub = ("perm", m) m
    rows in arbitrary order."""
    from vad_amd.tree_train import kfold
    if sub[0] == "perm":
        return np.random.default_rng(77).permutation(n)[:sub[1]]
    return kfold(n, sub[1])[sub[0]][0]


def table(tree):
    return {k: getattr(tree, k) for k in R.KEYS}


def assert_same(got, want, what):
    bad = R.tables_equal(table(got) if not isinstance(got, dict) else got, want)
    assert bad is None, f"{what}: '{bad}' differs ({len(got.feature) if not isinstance(got, dict) else ''} nodes, " \
                        f"model {len(want['feature'])})"


PARAMS = [(DEEP, 2, 1), (3, 22, 20), (1, 2, 1), (DEEP, 22, 20)]


@pytest.mark.parametrize("md,mss,msl", PARAMS)
@pytest.mark.parametrize("F,K", [(1, 2), (13, 2), (39, 3), (64, 8)])
def test_table_equals_model(torch_cuda, F, K, md, mss, msl):
    from vad_amd.tree_train import TreeTrainer
    x, y = rows(F, K)
    want = model(F, K, md, mss, msl)
    tr = TreeTrainer(md, mss, msl)
    got = tr.fit(x, y)
    print(f"F {F} K {K} md {md} mss {mss} msl {msl}: {len(want['feature'])} nodes, depth {want['depth'].max()}, "
          f"{tr.last_levels} levels on the device")
    assert_same(got, want, (F, K, md, mss, msl))
    if md == DEEP:
        assert want["depth"].max() < DEEP and len(want["feature"]) > (50 if F > 1 else 3)
    if md == 1:
        assert len(want["feature"]) == 3


def test_ties_take_the_lowest_feature_then_position(torch_cuda):
    """Four identical two-valued columns and a constant one: every score ties
    across features; a column of few values ties across positions."""
    from vad_amd.tree_train import TreeTrainer
    rng = np.random.default_rng(8)
    y = rng.integers(0, 3, N).astype(np.uint8)
    a = ((y == 1) ^ (rng.random(N) < 0.2)).astype(np.float32)
    b = np.round(rng.standard_normal(N) + y).astype(np.float32)
    x = np.stack([np.full(N, 3.0, np.float32), b, a, a, b, a[::-1].copy(), a], axis=1)
    want = R.fit(x, y, 3, DEEP, 2, 1)
    assert set(want["feature"].tolist()) <= {-1, 1, 2, 5}
    assert_same(TreeTrainer(DEEP, 2, 1).fit(x, y), want, "ties")


def test_degenerate_data(torch_cuda):
    from vad_amd.tree_train import TreeTrainer
    x, y = rows(13, 2)
    one = TreeTrainer(DEEP, 2, 1).fit(x, np.full(N, 4))
    assert len(one.feature) == 1 and one.feature[0] == -1 and one.n_node_samples[0] == N
    assert np.array_equal(one.classes_, [4]) and one.value.shape == (1, 1) and one.value[0, 0] == N
    assert np.array_equal(one.predict(x[:7]), np.full(7, 4))
    small = TreeTrainer(5, 22, 1).fit(x[:21], y[:21])  # n < min_samples_split at the root
    assert_same(small, R.fit(x[:21], y[:21], 2, 5, 22, 1), "small")
    assert len(small.feature) == 1
    leafy = TreeTrainer(5, 2, 20).fit(x[:39], y[:39])  # n < 2 * min_samples_leaf
    assert len(leafy.feature) == 1
    sub = ("perm", 1500)
    got = TreeTrainer().fit_many(x, y, [(subset(sub), DEEP, 2, 3)])[0]
    assert_same(got, model(13, 2, DEEP, 2, 3, sub=sub), "subset in arbitrary order")
    # labels that are not 0..K-1 map through classes_
    lab = np.array([-7, 30])[y]
    mapped = TreeTrainer(3, 22, 20).fit(x, lab)
    assert_same(mapped, model(13, 2, 3, 22, 20), "mapped labels")
    assert np.array_equal(mapped.classes_, [-7, 30])


MSLS = (1, 5, 20, 40)


def twelve_jobs():
    return [((f, 3), DEEP, 2, msl) for f in range(3) for msl in MSLS]


@pytest.fixture(scope="module")
def twelve(torch_cuda):
    """Twelve jobs (3 folds x 4 min_samples_leaf) in one call, and the models."""
    from vad_amd.tree_train import TreeTrainer
    x, y = rows(13, 2)
    jobs = twelve_jobs()
    got = TreeTrainer().fit_many(x, y, [(subset(s), md, mss, msl) for s, md, mss, msl in jobs])
    want = [model(13, 2, md, mss, msl, sub=s) for s, md, mss, msl in jobs]
    return got, want


def test_twelve_jobs_equal_the_model(twelve):
    got, want = twelve
    for j, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, f"job {j} of 12")


def test_twelve_jobs_equal_single_calls(torch_cuda, twelve):
    """A job's table does not depend on its company: alone, among 12, among 5
    in another order."""
    from vad_amd.tree_train import TreeTrainer
    x, y = rows(13, 2)
    jobs = twelve_jobs()
    for j in (0, 5, 11):
        s, md, mss, msl = jobs[j]
        alone = TreeTrainer().fit_many(x, y, [(subset(s), md, mss, msl)])[0]
        assert_same(alone, table(twelve[0][j]), f"job {j} alone")
    pick = [7, 2, 9, 0, 4]
    some = TreeTrainer().fit_many(x, y, [(subset(jobs[j][0]),) + jobs[j][1:] for j in pick])
    for g, j in zip(some, pick):
        assert_same(g, table(twelve[0][j]), f"job {j} among 5")


def test_ignores_stale_lds(torch_cuda, twelve):
    """The twelve-job call is bit-identical after every CU's LDS was filled
    with +-1e30 / NaN (loaded as tests/test_gpu_train.py does)."""
    from vad_amd.tree_train import TreeTrainer
    torch = torch_cuda
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_host", "liblds_poison.so")
    if not os.path.exists(so):
        pytest.fail("tests/c_host/liblds_poison.so missing: run __graft_entry__.build()")
    helper = ctypes.CDLL(so)
    helper.lds_poison.argtypes = [ctypes.c_float, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    sink = torch.zeros(1, device="cuda")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    x, y = rows(13, 2)
    X, jobs = torch.from_numpy(x).cuda(), [(subset(s), md, mss, msl) for s, md, mss, msl in twelve_jobs()]
    for v in (1e30, -1e30, float("nan")):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert helper.lds_poison(v, ctypes.c_void_p(sink.data_ptr()), 4 * n_cu, st) == 0
        got = TreeTrainer().fit_many(X, y, jobs)
        for j, g in enumerate(got):
            assert_same(g, table(twelve[0][j]), f"job {j} after LDS {v}")
    torch.cuda.synchronize()
    assert sink.item() == 0.0


def test_predict_and_pipeline(torch_cuda, golden, tmp_path):
    """fit(...).predict(X_train) is the model's tree walked on the host; the
    trained tree labels a clip's windows through VadPipeline / vad_features_tree
    as the TreeClassifier built from the model's arrays does, also after
    save / load."""
    from vad_amd.pipeline import VadPipeline
    from vad_amd.tree import TreeClassifier
    from vad_amd.tree_train import TreeTrainer
    torch = torch_cuda
    x, y = rows(39, 3)
    want = model(39, 3, DEEP, 22, 20)
    clf = TreeTrainer(DEEP, 22, 20).fit(x, y)
    assert np.array_equal(clf.predict(x), R.walk(want, x))
    ref = TreeClassifier(*(want[k] for k in R.KEYS[:6]), np.arange(3), 39)
    clip = torch.from_numpy(np.ascontiguousarray(golden("ffn")["test_clip"][:16000 * 2])).cuda()
    a = VadPipeline(clf).labels(clip)
    b = VadPipeline(ref).labels(clip)
    assert a.numel() > 0 and torch.equal(a, b)
    clf.save(str(tmp_path / "trained.npz"))
    back = TreeClassifier.load(str(tmp_path / "trained.npz"))
    assert_same(back, want, "save / load")
    assert torch.equal(VadPipeline(back).labels(clip), b)


def test_prune_on_device_output_equals_direct_training(torch_cuda):
    from vad_amd.tree_train import TreeTrainer, prune
    x, y = rows(13, 2)
    big = TreeTrainer(DEEP, 2, 5).fit(x, y)
    settings = [(3, 7), (10, 22), (25, 7), (4, 60)]
    direct = TreeTrainer().fit_many(x, y, [(None, md, mss, 5) for md, mss in settings])
    for (md, mss), d in zip(settings, direct):
        assert_same(prune(big, md, mss), table(d), f"prune {md} {mss}")
        assert_same(d, model(13, 2, md, mss, 5), f"direct {md} {mss}")


def test_grid_scores_equal_the_model(torch_cuda):
    """The score table of grid() is the accuracy of the model trained per
    setting and fold on the CPU and walked on the host."""
    from vad_amd.tree_train import TreeTrainer, kfold
    x, y = rows(13, 2)
    mds, msss, msls = [2, 5, DEEP], [2, 40], [5, 20]
    folds = kfold(N, 3)
    res = TreeTrainer().grid(x, y, mds, msss, msls, folds)
    assert len(res["params"]) == 12 and res["split_test_score"].shape == (12, 3)
    want = np.zeros((12, 3))
    for pi, p in enumerate(res["params"]):
        for fi, (tr, te) in enumerate(folds):
            t = R.fit(x, y, 2, p["max_depth"], p["min_samples_split"], p["min_samples_leaf"], rows=tr)
            want[pi, fi] = np.mean(R.walk(t, x[te]) == y[te])
    assert np.array_equal(res["split_test_score"], want)
    assert np.array_equal(res["mean_test_score"], want.mean(axis=1))
    best = int(np.argmax(want.mean(axis=1)))
    assert res["best_index_"] == best and res["best_params_"] == res["params"][best]
    assert res["best_score_"] == want.mean(axis=1)[best]
    assert [tuple(p.values()) for p in res["params"][:3]] == [(2, 5, 2), (2, 5, 40), (2, 20, 2)]


def test_small_node_buffer_is_an_error_not_a_write(torch_cuda):
    """node_capacity 5 for a tree of many nodes: VAD_ENOMEM, the overflow
    status, at most 5 nodes, and the guard words after every table intact."""
    from vad_amd import _lib
    from vad_amd.tree_train import _TABLES, _Job, _Tables, TreeTrainer
    from vad_amd._lib import VadError
    torch = torch_cuda
    x, y = rows(13, 2)
    with pytest.raises(VadError):
        TreeTrainer(DEEP, 2, 1).fit_many(x, y, [(None, DEEP, 2, 1)], node_capacity=5)
    lib = _lib.lib()
    K, cap, guard = 2, 5, 64
    X, Y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    order = torch.sort(X.t().contiguous(), dim=1, stable=True).indices.to(torch.int32).contiguous()
    desc = (_Job * 2)(_Job(N, cap, DEEP, 2, 1, 0), _Job(N, 99, 3, 22, 20, 0))
    need = lib.vad_tree_train_workspace_bytes(N, 13, K, 2, desc)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = {}
    for k, dt in _TABLES:
        size = 2 if k in ("n_nodes", "status") else (cap + 99) * (K if k == "value" else 1)
        fill = 0x5a if dt == torch.uint8 else -12345
        out[k] = torch.full((size + guard,), fill, dtype=dt, device="cuda")
    tb = _Tables(*(out[k].data_ptr() for k, _ in _TABLES))
    rc = lib.vad_tree_train(X.data_ptr(), Y.data_ptr(), N, 13, K, order.data_ptr(), None, 2, desc, ctypes.byref(tb),
                            ws.data_ptr(), need, None, _lib.stream_ptr())
    assert rc == _lib.VAD_ENOMEM
    status = out["status"][:2].cpu().numpy()
    n_nodes = out["n_nodes"][:2].cpu().numpy()
    assert status[0] == 1 and status[1] == 0 and 1 <= n_nodes[0] <= cap
    for k, dt in _TABLES:
        tail = out[k][-guard:].cpu().numpy()
        assert (tail == (0x5a if dt == torch.uint8 else -12345)).all(), k
    # the job beside it is whole: it equals the model (level order -> preorder)
    from vad_amd.tree_train import preorder
    m = int(n_nodes[1])
    t = {k: out[k][cap * (K if k == "value" else 1):].cpu().numpy()[:m * (K if k == "value" else 1)]
         for k in R.KEYS}
    t["value"] = t["value"].reshape(m, K)
    assert_same(preorder(t), model(13, 2, 3, 22, 20), "the job beside the overflowing one")
