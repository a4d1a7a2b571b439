"""Feature subsets per training job (vad_tree_train_features) and fit_forest
against the numpy model of tests/tree_train_reference.py run on the job's
columns, with the feature indices mapped back."""
import ctypes
import functools

import numpy as np
import pytest

import forest_reference as FR
import tree_train_reference as R

pytestmark = pytest.mark.gpu

N = 700
DEEP = 1000


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@functools.lru_cache(maxsize=None)
def rows(F, K, seed=5, n=N):
    return R.synth(n, F, K, seed)


def model(x, y, K, md, mss, msl, rows_=None, feats=None):
    """The reference tree of the job: trained on x[:, feats], features mapped back."""
    if feats is None:
        return R.fit(x, y, K, md, mss, msl, rows=rows_)
    feats = np.asarray(feats)
    t = R.fit(np.ascontiguousarray(x[:, feats]), y, K, md, mss, msl, rows=rows_)
    t["feature"] = np.where(t["feature"] >= 0, feats[np.maximum(t["feature"], 0)], -1).astype(t["feature"].dtype)
    return t


def table(tree):
    return {k: getattr(tree, k) for k in R.KEYS}


def assert_same(got, want, what):
    bad = R.tables_equal(table(got) if not isinstance(got, dict) else got, want)
    assert bad is None, f"{what}: '{bad}' differs"


def some_features(F, k, seed):
    return np.sort(np.random.default_rng(seed).choice(F, k, replace=False))


@pytest.mark.parametrize("md,mss,msl", [(DEEP, 2, 1), (4, 22, 20)])
@pytest.mark.parametrize("F,K", [(5, 2), (5, 3), (39, 2), (39, 3)])
def test_a_feature_subset_equals_the_model_on_those_columns(torch_cuda, F, K, md, mss, msl):
    from vad_amd.tree_train import TreeTrainer
    x, y = rows(F, K)
    for feats in (some_features(F, max(1, F // 3), 1), some_features(F, F - 1, 2), [F - 2, 0][:min(F, 2)]):
        got = TreeTrainer().fit_many(x, y, [(None, md, mss, msl, feats)])[0]
        want = model(x, y, K, md, mss, msl, feats=np.sort(np.asarray(feats)))
        assert_same(got, want, (F, K, list(feats)))
        assert set(got.feature[got.feature >= 0].tolist()) <= set(int(f) for f in feats)
    if md == DEEP:
        assert len(want["feature"]) > 3


def twelve_jobs(n, F):
    rng = np.random.default_rng(13)
    jobs = []
    for j in range(12):
        r = None if j % 4 == 0 else np.sort(rng.choice(n, int(n * (0.4 + 0.05 * (j % 5))), replace=False))
        f = None if j % 3 == 0 else some_features(F, 1 + (5 * j) % (F - 1), 40 + j)
        jobs.append((r, DEEP if j % 2 else 5, 2 + 10 * (j % 3), 1 + 4 * (j % 4), f))
    return jobs


def test_twelve_mixed_jobs_equal_single_calls_and_the_model(torch_cuda):
    from vad_amd.tree_train import TreeTrainer
    x, y = rows(13, 3)
    jobs = twelve_jobs(N, 13)
    together = TreeTrainer().fit_many(x, y, jobs)
    assert len(together) == 12
    for j, (job, got) in enumerate(zip(jobs, together)):
        alone = TreeTrainer().fit_many(x, y, [job])[0]
        assert_same(alone, table(got), f"job {j} alone")
    for j in (1, 2, 7, 11):
        r, md, mss, msl, f = jobs[j]
        assert_same(together[j], model(x, y, 3, md, mss, msl, rows_=r, feats=f), f"job {j} against the model")


def test_a_job_with_only_a_constant_feature_is_a_leaf(torch_cuda):
    from vad_amd.tree_train import TreeTrainer
    x, y = rows(13, 2)
    x = x.copy()
    x[:, 4] = 2.5
    x[:, 9] = -1.0
    leaf, both, other = TreeTrainer(DEEP, 2, 1).fit_many(
        x, y, [(None, DEEP, 2, 1, [4]), (None, DEEP, 2, 1, [4, 9]), (None, DEEP, 2, 1, [4, 6])])
    for t in (leaf, both):
        assert len(t.feature) == 1 and t.feature[0] == -1 and t.n_node_samples[0] == N
        assert t.value[0].tolist() == np.bincount(y, minlength=2).tolist()
    assert len(other.feature) > 1 and set(other.feature[other.feature >= 0].tolist()) == {6}


def test_full_masks_equal_vad_tree_train_byte_for_byte(torch_cuda):
    """The C entry with every bit set, with only the bits below F set and with
    no masks, against vad_tree_train: every output array byte for byte."""
    torch = torch_cuda
    from vad_amd import _lib
    from vad_amd.tree_train import _TABLES, _Job, _Tables
    lib = _lib.lib()
    F, K = 13, 3
    x, y = rows(F, K)
    n = len(x)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y.astype(np.uint8)).cuda()
    order = torch.sort(xd.t().contiguous(), dim=1, stable=True).indices.to(torch.int32).contiguous()
    sub = np.sort(np.random.default_rng(3).choice(n, 400, replace=False))
    mask = torch.zeros((2, n), dtype=torch.uint8, device="cuda")
    mask[0] = 1
    mask[1, torch.from_numpy(sub).cuda()] = 1
    caps = [int(lib.vad_tree_train_node_capacity(m, 1)) for m in (n, 400)]
    desc = (_Job * 2)(_Job(n, caps[0], DEEP, 2, 1, 0), _Job(400, caps[1], 6, 22, 5, 0))
    need = int(lib.vad_tree_train_workspace_bytes(n, F, K, 2, desc))
    total = sum(caps)

    def run(masks, plain=False):
        ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
        out = {k: torch.full((2 if k in ("n_nodes", "status") else total * (K if k == "value" else 1),), 0, dtype=dt,
                             device="cuda") for k, dt in _TABLES}
        tb = _Tables(*(out[k].data_ptr() for k, _ in _TABLES))
        args = [xd.data_ptr(), yd.data_ptr(), n, F, K, order.data_ptr(), mask.data_ptr()]
        tail = [2, desc, ctypes.byref(tb), ws.data_ptr(), need, None, None]
        if plain:
            rc = lib.vad_tree_train(*args, *tail)
        else:
            rc = lib.vad_tree_train_features(*args, None if masks is None else (ctypes.c_uint64 * 2)(*masks), *tail)
        assert rc == 0
        return {k: v.cpu().numpy().tobytes() for k, v in out.items()}

    want = run(None, plain=True)
    assert int(np.frombuffer(want["n_nodes"], np.int32)[0]) > 50
    for masks in (None, [(1 << 64) - 1] * 2, [(1 << F) - 1] * 2, [(1 << F) - 1, (1 << 64) - 1]):
        got = run(masks)
        for k in want:
            assert got[k] == want[k], (masks, k)


def test_fit_forest_equals_its_documented_jobs(torch_cuda):
    from vad_amd.forest import ForestClassifier
    from vad_amd.tree_train import TreeTrainer, forest_draws
    x, y = rows(39, 2)
    labels = np.array([3, 8])[y]  # class values that are not indices
    tr = TreeTrainer(8, 10, 3)
    forest = tr.fit_forest(x, labels, 4, max_samples=0.5, max_features=0.5, seed=3)
    rng = np.random.default_rng(3)
    jobs = []
    for _ in range(4):
        r = np.sort(rng.choice(N, 350, replace=False))
        f = np.sort(rng.choice(39, 19, replace=False))
        jobs.append((r, 8, 10, 3, f))
    for (r, f), job in zip(forest_draws(N, 39, 4, 0.5, 0.5, 3), jobs):
        assert np.array_equal(r, job[0]) and np.array_equal(f, job[4])
    trees = tr.fit_many(x, labels, jobs)
    want = ForestClassifier.from_trees(trees)
    assert forest.n_trees == 4 and np.array_equal(forest.classes_, [3, 8])
    for k, v in FR.table(want).items():
        assert getattr(forest, k).tobytes() == v.tobytes(), k
    at = np.append(forest.roots, len(forest.feature))
    for t, job in enumerate(jobs):  # every tree is the model's
        m = model(x, y, 2, 8, 10, 3, rows_=job[0], feats=job[4])
        for k in ("feature", "threshold", "nan_left"):
            assert np.array_equal(getattr(forest, k)[at[t]:at[t + 1]], m[k]), (t, k)
    f = FR.table(forest)
    xt, _ = R.synth(300, 39, 2, seed=6)
    assert np.array_equal(forest.predict(xt), np.array([3, 8])[FR.predict_index(f, xt)])
    import torch
    got = forest.predict_scores(torch.from_numpy(xt).cuda(), 1).cpu().numpy()
    assert np.array_equal(got.view(np.int32), FR.scores(f, xt, 1).view(np.int32))


def test_forest_training_accuracy_is_reported(torch_cuda):
    """Reported, not asserted: a forest and a single tree on a noisy two-class set."""
    from vad_amd.tree_train import TreeTrainer
    rng = np.random.default_rng(17)
    n = 3000
    y = rng.integers(0, 2, n)
    x = (rng.normal(0.0, 1.0, (n, 39)) + 0.35 * y[:, None] * (np.arange(39) < 10)).astype(np.float32)
    flip = rng.random(n) < 0.1
    y[flip] = 1 - y[flip]
    xt, yt = x[2000:], y[2000:]
    tr = TreeTrainer(25, 22, 20)
    tree = tr.fit(x[:2000], y[:2000])
    forest = tr.fit_forest(x[:2000], y[:2000], 16, max_samples=0.8, seed=1)
    for name, clf in (("tree", tree), ("forest of 16", forest)):
        print(f"{name}: training accuracy {np.mean(clf.predict(x[:2000]) == y[:2000]):.3f}, "
              f"held-out accuracy {np.mean(clf.predict(xt) == yt):.3f}")
    assert forest.n_trees == 16
