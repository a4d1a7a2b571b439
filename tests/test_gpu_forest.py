"""The forest on the device (csrc/forest_kernel.hip) against the definition
restated in numpy (tests/forest_reference.py) and sklearn's own results
(tests/golden/forest.npz): scores bit for bit, labels exactly."""
import ctypes
import os

import numpy as np
import pytest

import forest_reference as FR
from oracle import vad_oracle as O

pytestmark = pytest.mark.gpu

NAMES = ("rf", "bag", "rf3")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def fixture_forest(g, name):
    from vad_amd.forest import ForestClassifier
    return ForestClassifier(*(g[f"{name}_{k}"] for k in FR.KEYS), g[f"{name}_classes"], 39)


def as_tree(t, F, K=2):
    from vad_amd.tree import TreeClassifier
    return TreeClassifier(t["feature"], t["threshold"], t["left"], t["right"], t["leaf"], t["nan_left"], np.arange(K),
                          F, proba=t["proba"])


def random_forest(sizes, F, K=2, seed=0):
    from vad_amd.forest import ForestClassifier
    return ForestClassifier.from_trees([as_tree(FR.random_tree(n, F, K, seed + i), F, K) for i, n in enumerate(sizes)])


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def mfcc_rows(n_rows, mfcc_n, seed):
    """A random MFCC sequence of n_rows windows; from 20 windows on, six equal
    frames (two constant windows: NaN Mn in analyser mode)."""
    m = np.random.default_rng(seed).normal(0.0, 3.0, (n_rows + 5, mfcc_n)).astype(np.float32)
    if n_rows >= 20:
        m[10:16] = m[10]
    return m


def check_windows(torch, forest, m, mode, active=1):
    """window_labels / window_scores against the reference run on the rows of
    the existing feature path."""
    from vad_amd.plan import window_features
    md = torch.from_numpy(m).cuda()
    x = window_features(md, mode).cpu().numpy()
    f = FR.table(forest)
    lab = forest.window_labels(md, mode).cpu().numpy()
    sc = forest.window_scores(md, mode, active).cpu().numpy()
    assert lab.shape == sc.shape == (len(m) - 5,)
    assert np.array_equal(lab, FR.predict_index(f, x))
    assert np.array_equal(bits(sc), bits(FR.scores(f, x, active)))
    return x


@pytest.mark.parametrize("name", NAMES)
def test_rows_equal_sklearn(torch_cuda, golden, name):
    torch = torch_cuda
    g = golden("forest")
    forest = fixture_forest(g, name)
    x = g[f"{name}_x_test"]
    xd = torch.from_numpy(x).cuda()
    proba, want = g[f"{name}_predict_proba"], g[f"{name}_predict"]
    assert np.array_equal(forest.predict(x), want)
    assert np.array_equal(g[f"{name}_classes"][forest.predict_device(xd).cpu().numpy()], want)
    for active in range(proba.shape[1]):
        got = forest.predict_scores(xd, active).cpu().numpy()
        assert np.array_equal(bits(got), bits(proba[:, active].astype(np.float32))), active
    with pytest.raises(ValueError):
        forest.predict_scores(xd, proba.shape[1])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("mfcc_n", [13, 12])
@pytest.mark.parametrize("n_rows", [1, 255, 256, 257, 513])
def test_windows_equal_the_reference(torch_cuda, golden, n_rows, mfcc_n, mode):
    torch = torch_cuda
    if mfcc_n == 13:
        forests = [fixture_forest(golden("forest"), "rf"), fixture_forest(golden("forest"), "rf3")]
    else:
        forests = [random_forest([63, 31, 127], 36, 2, seed=5), random_forest([15, 41], 30, 3, seed=9)]
    for i, forest in enumerate(forests):
        x = check_windows(torch, forest, mfcc_rows(n_rows, mfcc_n, 100 + n_rows), mode, active=i)
        if n_rows >= 20:
            assert np.isnan(x).any() == (mode == 0)


def test_one_tree_equals_the_tree_classifier(torch_cuda, golden):
    torch = torch_cuda
    from vad_amd.forest import ForestClassifier
    from vad_amd.tree import TreeClassifier
    gt = golden("tree")
    # the fixture holds no node values: random ones (rows that do not sum to 1), the larger at the node's class
    p = np.sort(np.random.default_rng(0).random((len(gt["feature"]), 2)), axis=1)
    p[gt["leaf"] == 0] = p[gt["leaf"] == 0][:, ::-1]
    tree = TreeClassifier(*(gt[k] for k in ("feature", "threshold", "left", "right", "leaf", "nan_left")),
                          gt["classes"], 39, proba=p)
    forest = ForestClassifier.from_trees([tree])
    assert forest.n_trees == 1 and len(forest.feature) > 256
    md = torch.from_numpy(mfcc_rows(700, 13, 7)).cuda()
    for mode in (0, 1):
        assert torch.equal(forest.window_labels(md, mode), tree.window_labels(md, mode))
        for active in (0, 1):
            a, b = forest.window_scores(md, mode, active), tree.window_scores(md, mode, active)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    x = torch.from_numpy(np.nan_to_num(gt["x_test"]).astype(np.float32)).cuda()
    assert torch.equal(forest.predict_device(x), tree.predict_device(x))


@pytest.mark.parametrize("sizes,K", [([31, 1, 201, 7], 2), ([1], 2), ([1, 1, 1], 3), ([15, 3101, 9], 2),
                                     ([3071, 3073, 5, 3071], 2), ([41, 9, 77, 3, 51], 8)])
def test_unequal_trees_and_the_global_fallback(torch_cuda, sizes, K):
    """A single-leaf tree, odd tree counts (the pair walk's tail), a tree past
    the LDS limit between two small ones, trees at the limit."""
    torch = torch_cuda
    forest = random_forest(sizes, 39, K, seed=21)
    assert np.diff(np.append(forest.roots, len(forest.feature))).tolist() == sizes
    for mode in (0, 1):
        check_windows(torch, forest, mfcc_rows(300, 13, 3), mode, active=K - 1)
    x = np.random.default_rng(4).normal(0.0, 1.5, (333, 39)).astype(np.float32)
    x[::9, 3] = np.nan
    xd = torch.from_numpy(x).cuda()
    f = FR.table(forest)
    assert np.array_equal(forest.predict_device(xd).cpu().numpy(), FR.predict_index(f, x))
    assert np.array_equal(bits(forest.predict_scores(xd, 0).cpu().numpy()), bits(FR.scores(f, x, 0)))


def leaf_tree(share, F=39):
    from vad_amd.tree import TreeClassifier
    return TreeClassifier([-1], [-2.0], [-1], [-1], [int(np.argmax(share))], [0], np.arange(len(share)), F,
                          proba=np.array([share], np.float64))


def test_an_exact_tie_gives_the_first_class(torch_cuda):
    torch = torch_cuda
    from vad_amd.forest import ForestClassifier
    forest = ForestClassifier.from_trees([leaf_tree([1.0, 0.0]), leaf_tree([0.0, 1.0])])
    md = torch.from_numpy(mfcc_rows(40, 13, 1)).cuda()
    assert forest.window_labels(md).cpu().numpy().tolist() == [0] * 40
    assert forest.window_scores(md, active=1).cpu().numpy().tolist() == [0.5] * 40
    x = torch.zeros((7, 39), device="cuda")
    assert forest.predict_device(x).cpu().numpy().tolist() == [0] * 7
    assert forest.predict_scores(x, 0).cpu().numpy().tolist() == [0.5] * 7
    other = ForestClassifier.from_trees([leaf_tree([0.0, 1.0]), leaf_tree([1.0, 0.0])])
    assert other.window_labels(md).cpu().numpy().tolist() == [0] * 40


@pytest.mark.parametrize("nan_left", [0, 1])
def test_a_constant_window_follows_nan_left(torch_cuda, nan_left):
    torch = torch_cuda
    from vad_amd.forest import ForestClassifier
    from vad_amd.tree import TreeClassifier
    # root on Mn of coefficient 0: NaN in a constant window (analyser mode)
    stump = TreeClassifier([0, -1, -1], [1e30, -2.0, -2.0], [1, -1, -1], [2, -1, -1], [0, 0, 1], [nan_left, 0, 0],
                           np.arange(2), 39, proba=np.array([[.5, .5], [1., 0.], [0., 1.]]))
    forest = ForestClassifier.from_trees([stump, stump, stump])
    m = mfcc_rows(30, 13, 2)
    lab = forest.window_labels(torch.from_numpy(m).cuda(), 0).cpu().numpy()
    want = np.zeros(30, np.uint8)  # every finite Mn is <= 1e30: left, class 0
    want[10:12] = 0 if nan_left else 1
    assert np.array_equal(lab, want)


def test_results_ignore_stale_lds(torch_cuda, golden):
    torch = torch_cuda
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_host", "liblds_poison.so")
    if not os.path.exists(so):
        pytest.fail("tests/c_host/liblds_poison.so missing: run __graft_entry__.build()")
    helper = ctypes.CDLL(so)
    helper.lds_poison.argtypes = [ctypes.c_float, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    sink = torch.zeros(1, device="cuda")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    md = torch.from_numpy(mfcc_rows(3000, 13, 8)).cuda()
    forests = [fixture_forest(golden("forest"), "rf3"), random_forest([15, 3101, 9, 1, 33], 39, 2, seed=2)]
    for forest in forests:
        want = [forest.window_labels(md).clone(), forest.window_scores(md, active=1).view(torch.int32).clone()]
        for v in (1e30, -1e30, float("nan")):
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            assert helper.lds_poison(v, ctypes.c_void_p(sink.data_ptr()), 4 * n_cu, st) == 0
            assert torch.equal(forest.window_labels(md), want[0]), v
            assert helper.lds_poison(v, ctypes.c_void_p(sink.data_ptr()), 4 * n_cu, st) == 0
            assert torch.equal(forest.window_scores(md, active=1).view(torch.int32), want[1]), v
    torch.cuda.synchronize()
    assert sink.item() == 0.0


def test_entries_refuse_with_a_plan(torch_cuda, golden):
    from vad_amd import _lib
    forest = fixture_forest(golden("forest"), "rf")
    lib, h = _lib.lib(), forest.plan.handle
    x = torch_cuda.zeros((10, 39), device="cuda")
    lab = torch_cuda.zeros((10,), dtype=torch_cuda.uint8, device="cuda")
    sc = torch_cuda.zeros((10,), device="cuda")
    X, L, S = x.data_ptr(), lab.data_ptr(), sc.data_ptr()
    assert lib.vad_forest_predict(h, X, 10, 2, L, S, None) == -1
    assert lib.vad_forest_predict(h, X, -1, 0, L, S, None) == -1
    assert lib.vad_forest_predict(h, None, 10, 0, L, S, None) == -1
    assert lib.vad_forest_predict(h, X, 10, 0, None, S, None) == -1
    assert lib.vad_features_forest(h, X, -1, 13, 0, 0, L, S, None) == -1
    assert lib.vad_features_forest(h, X, 15, 13, 0, 2, L, S, None) == -1
    assert lib.vad_features_forest(h, X, 15, 12, 0, 0, L, S, None) == -1  # 39 features need 13 coefficients
    assert lib.vad_features_forest(h, None, 15, 13, 0, 0, L, S, None) == -1
    assert lib.vad_features_forest(h, X, 15, 13, 0, 0, None, S, None) == -1
    assert lib.vad_features_forest(h, X, 15, 13, 0, 0, L, None, None) == 0  # labels alone
    assert lib.vad_forest_predict(h, X, 10, 0, L, None, None) == 0


# -- the pipeline ----------------------------------------------------------------
@pytest.fixture(scope="module")
def clip():
    return O.synth_clip(O.samples_for_frames(1500), seed=77)


def test_pipeline_with_a_forest(torch_cuda, golden, clip):
    torch = torch_cuda
    from vad_amd import scores as S
    from vad_amd.pipeline import VadPipeline
    from vad_amd.segments import label_segments
    forest = fixture_forest(golden("forest"), "rf")
    pipe = VadPipeline(forest)
    audio = torch.from_numpy(clip).cuda()
    f = FR.table(forest)
    x = pipe.features(audio).cpu().numpy()
    lab, sc = pipe.labels(audio), pipe.scores(audio)
    assert np.array_equal(lab.cpu().numpy(), FR.predict_index(f, x))
    assert np.array_equal(bits(sc.cpu().numpy()), bits(FR.scores(f, x, 1)))
    assert np.array_equal(bits(pipe.scores(audio, active=0).cpu().numpy()), bits(FR.scores(f, x, 0)))
    s = sc.cpu().numpy()
    on, off = (float(np.float32(np.quantile(s, p))) for p in (.7, .4))
    want = label_segments(S.dilate_labels(S.score_labels(sc, on, off), (2, 3)), len(clip))
    got = pipe.segments(audio, on=on, off=off, pad=(2, 3))
    assert np.array_equal(got.numpy(), want.numpy()) and len(got.numpy()) > 1
    assert np.array_equal(pipe.segments(audio).numpy(), label_segments(lab, len(clip)).numpy())
    voiced = pipe.voiced(audio, on=on, off=off, pad=(2, 3))
    assert 0 < voiced.numel() < len(clip)
    # a fitted sklearn ensemble is converted on the way in
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import gen_forest
    assert torch.equal(VadPipeline(gen_forest.fitted("rf")).labels(audio), lab)


def test_pipeline_batch_forms_equal_single_clips(torch_cuda, golden, clip):
    torch = torch_cuda
    from vad_amd.batch import ClipBatch
    from vad_amd.pipeline import VadPipeline
    pipe = VadPipeline(fixture_forest(golden("forest"), "rf"))
    lens = [160 * 299 + 401, 160 * 700 + 401, 160 * 40 + 401]
    clips, pos = [], 0
    for n in lens:
        clips.append(clip[pos:pos + n])
        pos += n
    b = ClipBatch.from_host(clips)
    lb, sb = pipe.labels_batch(b), pipe.scores_batch(b)
    s = sb.scores.cpu().numpy()
    on, off = (float(np.float32(np.quantile(s[np.isfinite(s)], p))) for p in (.7, .4))
    kw = dict(on=on, off=off, pad=(2, 3))
    seg = pipe.segments_batch(b, **kw)
    voiced, offsets = pipe.voiced_batch(b, **kw)
    found = 0
    for k, c in enumerate(clips):
        alone = torch.from_numpy(np.ascontiguousarray(c)).cuda()
        assert torch.equal(lb[k], pipe.labels(alone)), k
        assert torch.equal(sb[k].view(torch.int32), pipe.scores(alone).view(torch.int32)), k
        rows = pipe.segments(alone, **kw).numpy()
        assert np.array_equal(seg.clip(k), rows), k
        assert torch.equal(voiced[offsets[k]:offsets[k + 1]], pipe.voiced(alone, **kw)), k
        found += len(rows)
    assert found > 2


def test_refused_combinations_raise(torch_cuda, golden, clip, tmp_path):
    torch = torch_cuda
    from vad_amd.dist import classify_clip_shard, split_clip
    from vad_amd.pipeline import VadPipeline
    from vad_amd.sklearn_analyser import SKLearnAnalyzer
    from vad_amd.stream import StreamBatch
    forest = fixture_forest(golden("forest"), "rf")
    pipe = VadPipeline(forest)
    audio = torch.from_numpy(clip).cuda()
    with pytest.raises(ValueError, match="fused"):
        pipe.labels(audio, fused=True)
    assert not pipe.fusable
    with pytest.raises(ValueError, match="forest"):
        StreamBatch(8, forest)
    path = str(tmp_path / "forest.npz")
    forest.save(path)
    with pytest.raises(ValueError, match="forest"):
        SKLearnAnalyzer(path)
    with pytest.raises(ValueError, match="forest"):
        classify_clip_shard(pipe, audio, split_clip(len(clip), 0, 1))
