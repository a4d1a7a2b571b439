"""Weighted tree training on the device against the numpy model of the
weighted rule (tests/tree_train_weighted_reference.py): every array of the node
table bitwise unless stated.  Weights are bootstrap counts ("boot"), one
integer per class ("class") or their product ("both")."""
import ctypes
import functools

import numpy as np
import pytest

import forest_reference as FR
import tree_train_reference as R
import tree_train_weighted_reference as W

pytestmark = pytest.mark.gpu

TILE = 2048
DEEP = 1000  # a depth the data never reaches
CONFIGS = ("w13", "w7q", "w5", "w9")
KINDS = ("boot", "class", "both")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@functools.lru_cache(maxsize=None)
def rows(n, F, K, seed=5):
    return R.synth(n, F, K, seed)


def model(x, y, w, K, md, mss, msl, feats=None):
    """The weighted model; with feats the model on those columns, indices mapped back."""
    if feats is None:
        return W.fit(x, y, w, K, md, mss, msl)
    feats = np.asarray(feats)
    t = W.fit(x[:, feats], y, w, K, md, mss, msl)
    f = t["feature"]
    t["feature"] = np.where(f >= 0, feats[np.maximum(f, 0)], -1).astype(np.int32)
    return t


def table(tree):
    return {k: getattr(tree, k) for k in R.KEYS}


def assert_same(got, want, what):
    got = got if isinstance(got, dict) else table(got)
    bad = R.tables_equal(got, want)
    assert bad is None, f"{what}: '{bad}' differs ({len(got['feature'])} nodes against {len(want['feature'])})"


def heavy(n, y, K, seed, zeros=0):
    """Weights 1..36 (class integer x 1..5) with ``zeros`` rows at 0."""
    rng = np.random.default_rng(seed)
    w = W.class_integers(y, K, seed) * rng.integers(1, 6, n)
    w[rng.permutation(n)[:zeros]] = 0
    return w


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", CONFIGS)
def test_golden_configurations(torch_cuda, golden, name, kind):
    from vad_amd.tree_train import TreeTrainer
    g = golden("tree_train_weighted")
    x, y = g[f"{name}_x"], g[f"{name}_y"]
    K, md, mss, msl = (int(v) for v in g[f"{name}_params"])
    w = g[f"{name}_{kind}_w"]
    got = TreeTrainer(md, mss, msl).fit(x, y, sample_weight=w)
    want = W.fit(x, y, w, K, md, mss, msl)
    assert_same(got, want, f"{name} {kind}")
    assert got.value[0].sum() == int(w.astype(np.int64).sum()) and got.n_node_samples[0] == np.count_nonzero(w)
    # the root of every sklearn tree of the fixture has this table's counts
    pre = f"{name}_{kind}_rs0_"
    assert (got.value[0] / got.value[0].sum()).tobytes() == g[pre + "value"][0].tobytes()


@pytest.mark.parametrize("live", [2047, 2048, 2049, 4100])
def test_tile_edges(torch_cuda, live):
    """``live`` rows above 0 among live + 300: the lists are exactly ``live`` long."""
    from vad_amd.tree_train import TreeTrainer
    n = live + 300
    x, y = rows(n, 7, 3)
    w = heavy(n, y, 3, live, zeros=300)
    assert np.count_nonzero(w) == live
    got = TreeTrainer(DEEP, 2, 1).fit_many(x, y, [(None, DEEP, 2, 1, None, w), (None, 7, 22, 20, None, w)])
    assert_same(got[0], W.fit(x, y, w, 3, DEEP, 2, 1), f"{live} deep")
    assert_same(got[1], W.fit(x, y, w, 3, 7, 22, 20), f"{live} shallow")
    assert got[0].depth.max() > 8


@pytest.mark.parametrize("live,msl", [(1, 1), (2, 2), (9, 5)])
def test_leaf_roots(torch_cuda, live, msl):
    """1, 2 and 2 * min_samples_leaf - 1 rows above 0: the root is a leaf."""
    from vad_amd.tree_train import TreeTrainer
    n = 600
    x, y = rows(n, 5, 2)
    w = np.zeros(n, np.int64)
    at = np.random.default_rng(live).permutation(n)[:live]
    w[at] = 7 + np.arange(live)
    tr = TreeTrainer(DEEP, 2, msl)
    got = tr.fit_many(x, y, [(None, DEEP, 2, msl, None, w), (None, DEEP, 2, 1, None, heavy(n, y, 2, 3))])
    want = W.fit(x, y, w, 2, DEEP, 2, msl)
    assert len(want["feature"]) == 1
    assert_same(got[0], want, f"{live} rows")
    assert got[0].n_node_samples[0] == live and got[0].value[0].sum() == w.sum()
    assert len(got[1].feature) > 50


@pytest.mark.parametrize("subset", [False, True])
@pytest.mark.parametrize("K", [2, 3, 5])
def test_every_search_build(torch_cuda, K, subset):
    """Up to 2, 4 and 8 classes (one, two and four counter words), each with and without feature masks."""
    from vad_amd.tree_train import TreeTrainer
    n, F = TILE + 500, 13
    x, y = rows(n, F, K)
    w = W.weights_of("both", y, K, 31)
    feats = np.array([0, 3, 4, 9, 10, 12]) if subset else None
    got = TreeTrainer().fit_many(x, y, [(None, DEEP, 4, 2, feats, w)])[0]
    assert_same(got, model(x, y, w, K, DEEP, 4, 2, feats), f"K {K} subset {subset}")
    assert got.depth.max() > 6


def test_mixed_jobs_in_one_call(torch_cuda):
    """An unweighted job, a rows subset, a bootstrap job, a class-weighted job
    on a feature subset and the bootstrap job again: each equals its single
    call and the model; the two bootstrap jobs give identical tables."""
    from vad_amd.tree_train import TreeTrainer
    n, F, K = 2 * TILE + 37, 13, 3
    x, y = rows(n, F, K)
    sub = np.random.default_rng(77).permutation(n)[:1500]
    boot = W.weights_of("boot", y, K, 41)
    cls = W.weights_of("class", y, K, 42)
    feats = np.array([1, 2, 5, 9, 11])
    jobs = [(None, DEEP, 2, 1), (sub, 9, 22, 20), (None, DEEP, 10, 5, None, boot), (None, 12, 2, 3, feats, cls),
            (None, DEEP, 10, 5, None, boot)]
    tr = TreeTrainer()
    got = tr.fit_many(x, y, jobs)
    ones, in_sub = np.ones(n, np.int64), np.zeros(n, np.int64)
    in_sub[sub] = 1
    want = [R.fit(x, y, K, DEEP, 2, 1), R.fit(x, y, K, 9, 22, 20, rows=sub), W.fit(x, y, boot, K, DEEP, 10, 5),
            model(x, y, cls, K, 12, 2, 3, feats), None]
    want[4] = want[2]
    assert_same(want[0], W.fit(x, y, ones, K, DEEP, 2, 1), "model of ones")
    assert_same(want[1], W.fit(x, y, in_sub, K, 9, 22, 20), "model of 0/1")
    for j, (t, m) in enumerate(zip(got, want)):
        assert_same(t, m, f"job {j} in the mixed call")
        assert_same(tr.fit_many(x, y, [jobs[j]])[0], m, f"job {j} alone")
    assert R.tables_equal(table(got[2]), table(got[4])) is None


def test_extremes(torch_cuda):
    """Weights of 255 on some rows, and more than half of the rows at 0."""
    from vad_amd.tree_train import TreeTrainer
    n, F, K = TILE + 700, 7, 2
    x, y = rows(n, F, K)
    rng = np.random.default_rng(8)
    w = rng.integers(1, 4, n)
    w[rng.permutation(n)[:400]] = 255
    w[rng.permutation(n)[:n * 3 // 5]] = 0
    assert (w == 255).sum() > 100 and (w == 0).sum() > n // 2
    got = TreeTrainer(DEEP, 6, 3).fit(x, y, sample_weight=w)
    assert_same(got, W.fit(x, y, w, K, DEEP, 6, 3), "255s and zeros")
    assert got.value[0].sum() == w.sum() > 255 * 100
    allmax = np.full(n, 255)
    assert_same(TreeTrainer(10, 6, 3).fit(x, y, sample_weight=allmax), W.fit(x, y, allmax, K, 10, 6, 3), "all 255")


def _c_run(torch, lib, entry, x, y, K, weights, desc, fmasks=None, ws_fn=None):
    """One call of a C entry on fresh outputs; (rc, {name: bytes}, status)."""
    from vad_amd.tree_train import _TABLES, _Tables
    n, F = x.shape
    J = len(desc)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y.astype(np.uint8)).cuda()
    order = torch.sort(xd.t().contiguous(), dim=1, stable=True).indices.to(torch.int32).contiguous()
    need = int((ws_fn or lib.vad_tree_train_workspace_bytes)(n, F, K, J, desc))
    assert need > 0
    total = sum(int(d.node_capacity) for d in desc)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    out = {k: torch.zeros(J if k in ("n_nodes", "status") else total * (K if k == "value" else 1), dtype=dt,
                          device="cuda") for k, dt in _TABLES}
    tb = _Tables(*(out[k].data_ptr() for k, _ in _TABLES))
    wd = None if weights is None else torch.from_numpy(np.ascontiguousarray(weights, np.uint8)).cuda()
    fm = None if fmasks is None else (ctypes.c_uint64 * J)(*fmasks)
    rc = entry(xd.data_ptr(), yd.data_ptr(), n, F, K, order.data_ptr(), None if wd is None else wd.data_ptr(), fm, J,
               desc, ctypes.byref(tb), ws.data_ptr(), need, None, None)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy().tobytes() for k, v in out.items()}, out["status"].cpu().numpy()


@pytest.mark.parametrize("K", [2, 3, 5])
def test_weights_of_ones_equal_the_unweighted_entry_byte_for_byte(torch_cuda, K):
    """The weighted kernels on weights of all ones (and on a 0 / 1 mask) against
    vad_tree_train_features on the same jobs: every output array."""
    torch = torch_cuda
    from vad_amd import _lib
    from vad_amd.tree_train import _Job
    lib = _lib.lib()
    n, F = 2 * TILE + 37, 13
    x, y = rows(n, F, K)
    sub = np.sort(np.random.default_rng(3).choice(n, 900, replace=False))
    mask = np.zeros((2, n), np.uint8)
    mask[0] = 1
    mask[1, sub] = 1
    caps = [int(lib.vad_tree_train_node_capacity(m, 1)) for m in (n, 900)]
    desc = (_Job * 2)(_Job(n, caps[0], DEEP, 2, 1, 0), _Job(900, caps[1], 6, 22, 5, 0))
    for fm in (None, [(1 << F) - 1, 0b1011001101]):
        rc, want, _ = _c_run(torch, lib, lib.vad_tree_train_features, x, y, K, mask, desc, fm)
        assert rc == 0 and int(np.frombuffer(want["n_nodes"], np.int32)[0]) > 50
        rc, got, _ = _c_run(torch, lib, lib.vad_tree_train_weighted, x, y, K, mask, desc, fm,
                            lib.vad_tree_train_weighted_workspace_bytes)
        assert rc == 0
        for k in want:
            assert got[k] == want[k], (K, fm, k)
    # NULL weights: all ones, every job takes every row
    one = (_Job * 1)(_Job(n, caps[0], DEEP, 2, 1, 0))
    rc, want, _ = _c_run(torch, lib, lib.vad_tree_train_features, x, y, K, None, one)
    rc2, got, _ = _c_run(torch, lib, lib.vad_tree_train_weighted, x, y, K, None, one, None,
                         lib.vad_tree_train_weighted_workspace_bytes)
    assert rc == 0 and rc2 == 0 and got == want


def test_unweighted_fit_is_unchanged(torch_cuda):
    from vad_amd.tree_train import TreeTrainer
    n, F, K = 2 * TILE + 37, 13, 3
    x, y = rows(n, F, K)
    tr = TreeTrainer(DEEP, 2, 1)
    assert_same(tr.fit(x, y), R.fit(x, y, K, DEEP, 2, 1), "unweighted fit")
    assert_same(tr.fit(x, y, sample_weight=np.ones(n, np.int64)), R.fit(x, y, K, DEEP, 2, 1), "fit with ones")


def test_min_samples_leaf_counts_distinct_rows_under_heavy_weights(torch_cuda):
    from vad_amd.tree_train import TreeTrainer
    n, F, K = TILE + 900, 7, 3
    x, y = rows(n, F, K)
    w = heavy(n, y, K, 5) * 7
    assert w.max() <= 255
    got = TreeTrainer(DEEP, 22, 20).fit(x, y, sample_weight=w)
    assert_same(got, W.fit(x, y, w, K, DEEP, 22, 20), "min_samples_leaf 20")
    leaves = got.left < 0
    assert leaves.sum() > 20 and got.n_node_samples[leaves].min() >= 20
    assert got.value.sum(axis=1)[leaves].min() > 20 * 7 and got.n_node_samples[leaves].min() < 40
    # the same rows repeated w times split further: weights are not repetition
    small = TreeTrainer(DEEP, 2, 20).fit(x[:300], y[:300], sample_weight=w[:300])
    rep = TreeTrainer(DEEP, 2, 20).fit(np.repeat(x[:300], w[:300], axis=0), np.repeat(y[:300], w[:300]))
    assert len(rep.feature) > len(small.feature)


def test_fit_forest_bootstrap(torch_cuda):
    torch = torch_cuda
    from vad_amd.tree_train import TreeTrainer, forest_draws
    n, F = TILE + 300, 13
    x, y = rows(n, F, 2)
    labels = np.array([3, 8])[y]  # class values that are not indices
    tr = TreeTrainer(8, 10, 3)
    cw = {3: 2, 8: 5}
    for class_weight in (None, cw):
        forest = tr.fit_forest(x, labels, 4, max_features=0.5, seed=3, bootstrap=True, class_weight=class_weight)
        assert forest.n_trees == 4 and np.array_equal(forest.classes_, [3, 8])
        draws = forest_draws(n, F, 4, 1.0, 0.5, 3, bootstrap=True)
        at = np.append(forest.roots, len(forest.feature))
        per_class = np.ones(n, np.int64) if class_weight is None else np.array([2, 5])[y]
        shares = []
        for t, (counts, feats) in enumerate(draws):
            assert counts.sum() == n and (counts == 0).any() and counts.max() > 1
            w = counts * per_class
            single = tr.fit_many(x, labels, [(None, 8, 10, 3, feats, w)])[0]
            m = model(x, y, w, 2, 8, 10, 3, feats)
            assert_same(single, m, f"tree {t} alone")
            for k in ("feature", "threshold", "nan_left"):
                assert np.array_equal(getattr(forest, k)[at[t]:at[t + 1]], m[k]), (t, k)
            shares.append(m)
        # predict_proba: the host average of the trees' value / W, trees in order
        xt, _ = R.synth(300, F, 2, seed=6)
        acc = np.zeros((300, 2))
        for m in shares:
            node = np.zeros(300, np.int64)
            for _ in range(int(m["depth"].max()) + 1):
                f = m["feature"][node]
                inner = f >= 0
                go_left = xt[np.arange(300), np.maximum(f, 0)].astype(np.float64) <= m["threshold"][node]
                node = np.where(inner, np.where(go_left, m["left"][node], m["right"][node]), node)
            v = m["value"][node].astype(np.float64)
            acc += v / v.sum(axis=1, keepdims=True)
        acc /= 4
        ft = FR.table(forest)
        assert np.array_equal(FR.predict_proba(ft, xt), acc)
        assert np.array_equal(forest.predict(xt), np.array([3, 8])[np.argmax(acc, axis=1)])
        got = forest.predict_scores(torch.from_numpy(xt).cuda(), 1).cpu().numpy()
        assert np.array_equal(got.view(np.int32), acc[:, 1].astype(np.float32).view(np.int32))


def test_grid_with_sample_weight(torch_cuda):
    from vad_amd.tree_train import TreeTrainer, kfold
    n, F, K = 900, 7, 2
    x, y = rows(n, F, K)
    sw = W.weights_of("boot", y, K, 9)
    cw = {0: 3, 1: 1}
    w = sw * np.array([3, 1])[y]
    folds = kfold(n, 3)
    mds, msss, msls = [3, 25], [2, 40], [1, 20]
    res = TreeTrainer().grid(x, y, mds, msss, msls, folds, sample_weight=sw, class_weight=cw)
    # the scores are compared as counts of correct test rows: an accuracy is k / 300, and the device's mean of 300
    # doubles may differ from numpy's k / 300 in the last bit (both within 2^-53 of the quotient), so
    # rint(score * 300) == k with |score - k / 300| <= 2^-52 says the same thing exactly
    correct = np.zeros((len(res["params"]), 3), np.int64)
    for pi, p in enumerate(res["params"]):
        for fi, (tr, te) in enumerate(folds):
            assert len(te) == 300
            wf = np.zeros(n, np.int64)
            wf[tr] = w[tr]
            t = W.fit(x, y, wf, K, p["max_depth"], p["min_samples_split"], p["min_samples_leaf"])
            correct[pi, fi] = np.count_nonzero(R.walk(t, x[te]) == y[te])
    got = res["split_test_score"]
    assert np.array_equal(np.rint(got * 300).astype(np.int64), correct)
    assert np.abs(got - correct / 300.0).max() <= 2.0 ** -52
    assert np.array_equal(res["mean_test_score"], got.mean(axis=1))
    totals = correct.sum(axis=1)
    assert totals[res["best_index_"]] == totals.max()
    if (totals == totals.max()).sum() == 1:
        assert res["best_index_"] == int(np.argmax(totals))
    plain = TreeTrainer().grid(x, y, mds, msss, msls, folds)
    assert not np.array_equal(np.rint(plain["split_test_score"] * 300).astype(np.int64), correct)


def test_total_weight_above_the_limit_is_refused(torch_cuda):
    """ValueError on the host before any launch; and the C entry, given such
    weights anyway, refuses the job by its status."""
    torch = torch_cuda
    from vad_amd import _lib
    from vad_amd.tree_train import TreeTrainer, _Job
    lib = _lib.lib()
    n = (1 << 26) // 255 + 2
    x = np.arange(n, dtype=np.float32).reshape(-1, 1) % 97
    y = (np.arange(n) % 2).astype(np.uint8)
    w = np.full(n, 255, np.uint8)
    tr = TreeTrainer(3, 2, 1)
    tr.last_levels = None
    with pytest.raises(ValueError, match="2\\^26"):
        tr.fit(x, y, sample_weight=w)
    assert tr.last_levels is None and tr.last_call_seconds is None  # nothing was launched
    desc = (_Job * 1)(_Job(n, 15, 3, 2, 1, 0))
    rc, _, status = _c_run(torch, lib, lib.vad_tree_train_weighted, x, y, 2, w[None], desc, None,
                           lib.vad_tree_train_weighted_workspace_bytes)
    assert rc == _lib.VAD_EINVAL and status[0] & 4
    w[: n - (1 << 26) // 255] = 0  # two rows fewer: 2^26 - 4 in all, accepted
    desc = (_Job * 1)(_Job(int(np.count_nonzero(w)), 15, 3, 2, 1, 0))
    rc, _, status = _c_run(torch, lib, lib.vad_tree_train_weighted, x, y, 2, w[None], desc, None,
                           lib.vad_tree_train_weighted_workspace_bytes)
    assert rc == 0 and status[0] == 0 and int(w.astype(np.int64).sum()) <= 1 << 26


def test_n_rows_that_disagrees_with_the_weights_is_refused(torch_cuda):
    torch = torch_cuda
    from vad_amd import _lib
    from vad_amd.tree_train import _Job
    lib = _lib.lib()
    n = 700
    x, y = rows(n, 5, 2)
    w = heavy(n, y, 2, 1, zeros=100)
    for claimed in (599, 601):
        desc = (_Job * 1)(_Job(claimed, 2 * n, 5, 2, 1, 0))
        rc, _, status = _c_run(torch, lib, lib.vad_tree_train_weighted, x, y, 2, w[None], desc, None,
                               lib.vad_tree_train_weighted_workspace_bytes)
        assert rc == _lib.VAD_EINVAL and status[0] & 2, claimed


def test_node_capacity_too_small(torch_cuda):
    from vad_amd._lib import VadError
    from vad_amd.tree_train import TreeTrainer
    n = 1500
    x, y = rows(n, 7, 3)
    w = heavy(n, y, 3, 2)
    tr = TreeTrainer(DEEP, 2, 1)
    with pytest.raises(VadError, match="node storage too small"):
        tr.fit_many(x, y, [(None, DEEP, 2, 1, None, w)], node_capacity=9)
    assert 3 <= len(tr.fit_many(x, y, [(None, 3, 2, 1, None, w)], node_capacity=15)[0].feature) <= 15
