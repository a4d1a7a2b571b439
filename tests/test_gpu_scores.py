"""The score stage on the device (vad_amd/csrc/score_kernel.hip) against the
NumPy models of tests/scores_reference.py, the float64 softmax of the FFN
kernel's own logits, sklearn's predict_proba, and the segment stage.

Measured on an MI355X: the largest |score - float64 softmax| is 1.47 * 2^-24
(13-64-64-2) and 1.48 * 2^-24 (39-64-32-16-3) against the bound of 8 * 2^-24;
test_ffn_scores prints it and profiles/scores/bench.json records it."""
import numpy as np
import pytest

import scores_reference as R
from test_segments_cpu import model_smooth, model_voiced, samples_for_windows

pytestmark = pytest.mark.gpu

T = 1024
NS = [0, 1, 5, T - 1, T, T + 1, 2 * T + 3, 256 * T + 7]  # the last crosses a carry pass
THRESHOLDS = [(0.7, 0.3), (0.5, 0.5), (1.0, 0.0), (0.0, 0.0)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from vad_amd import segments as G
    assert G.SEG_TILE == T and G.SEG_CARRY_PASS == 256
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def twice(torch, S, n, run):
    """`run(ws)` twice, the workspace filled with 0xFF before each: nothing a
    kernel reads from it may be left from an earlier call."""
    ws = S.workspace(n, torch.device("cuda"))
    ws.fill_(0xFF)
    a = run(ws).cpu().numpy()
    ws.fill_(0xFF)
    b = run(ws).cpu().numpy()
    assert np.array_equal(a, b)
    return a


def score_families(n, on, off, seed):
    rng = np.random.default_rng(seed)
    mid = np.float32((on + off) / 2)  # undecided where off < on
    fam = {}
    s = rng.random(n).astype(np.float32)
    fam["random"] = s
    s = s.copy()
    s[rng.random(n) < 0.1] = np.nan
    s[rng.random(n) < 0.02] = 0.0
    s[rng.random(n) < 0.02] = 1.0
    fam["nan"] = s
    s = np.full(n, mid, np.float32)
    fam["none_decided"] = s
    s = s.copy()
    s[:1] = 1.0
    fam["only_window_0_decided"] = s
    s = np.full(n, mid, np.float32)
    firsts = np.arange(0, n, T)
    lasts = firsts[1:] - 1
    s[firsts] = np.where(np.arange(len(firsts)) % 2 == 0, 1.0, 0.0)
    s[lasts] = np.where(np.arange(len(lasts)) % 3 == 0, 0.0, 1.0)
    fam["tile_edges"] = s
    s = rng.random(n).astype(np.float32)
    s[rng.random(n) < 0.995] = mid  # long undecided stretches between rare decisions
    fam["sparse"] = s
    return fam


@pytest.mark.parametrize("n", NS)
def test_hysteresis_equals_the_model(torch_cuda, n):
    torch = torch_cuda
    from vad_amd import scores as S
    for t, (on, off) in enumerate(THRESHOLDS):
        for name, s in score_families(n, on, off, seed=n + t).items():
            d = dev(torch, s)
            got = twice(torch, S, n, lambda ws: S.score_labels(d, on, off, ws=ws))
            assert got.dtype == np.uint8 and got.shape == (n,)
            want = R.hysteresis(s, on, off)
            assert np.array_equal(got, want), (n, on, off, name, np.flatnonzero(got != want)[:5])
    if n > 2 * T:  # the carry crossed every tile: window 0's decision holds to the end
        s = score_families(n, 0.7, 0.3, 0)["only_window_0_decided"]
        assert S.score_labels(dev(torch, s), 0.7, 0.3).cpu().numpy().all()


def label_families(n, seed):
    rng = np.random.default_rng(seed)
    fam = {"dense": (rng.random(n) < 0.2).astype(np.uint8) * 2,
           "sparse": (rng.random(n) < 0.0005).astype(np.uint8) * 2,
           "none": np.ones(n, np.uint8)}
    for name, idx in (("first", slice(0, 1)), ("last", slice(max(n - 1, 0), n))):
        a = np.zeros(n, np.uint8)
        a[idx] = 2
        fam[name] = a
    a = np.zeros(n, np.uint8)
    a[np.arange(0, n, T)[1::2]] = 2
    a[(np.arange(0, n, T)[2::2] - 1)] = 2
    fam["tile_edges"] = a
    return fam


@pytest.mark.parametrize("n", NS)
def test_dilation_equals_the_model(torch_cuda, n):
    torch = torch_cuda
    from vad_amd import scores as S
    pads = [0, 1, T, n + 5]
    for name, lab in label_families(n, seed=n).items():
        d = dev(torch, lab)
        for pb in pads:
            for pa in pads:
                if name in ("dense", "none") and (pb, pa) not in ((0, 0), (1, 0), (0, 1), (T, 1), (n + 5, n + 5)):
                    continue
                got = twice(torch, S, n, lambda ws: S.dilate_labels(d, (pb, pa), active=2, ws=ws))
                want = R.dilate(lab, 2, pb, pa)
                assert np.array_equal(got, want), (n, name, pb, pa, np.flatnonzero(got != want)[:5])


def test_out_and_workspace_checks(torch_cuda):
    torch = torch_cuda
    from vad_amd import scores as S
    s = torch.rand(100, device="cuda")
    lab = torch.zeros(100, dtype=torch.uint8, device="cuda")
    buf = torch.zeros(400, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="alias"):
        S.score_labels(buf.view(torch.float32), 0.5, out=buf[:100])
    with pytest.raises(ValueError, match="alias"):
        S.dilate_labels(lab, (1, 1), out=lab)
    with pytest.raises(ValueError):
        S.score_labels(s, 0.5, out=torch.zeros(99, dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        S.score_labels(s, 0.5, out=torch.zeros(100, dtype=torch.int8, device="cuda"))
    with pytest.raises(ValueError):
        S.score_labels(s[::2], 0.5)
    with pytest.raises(ValueError, match="smaller"):
        S.score_labels(torch.rand(5000, device="cuda"), 0.5, ws=torch.zeros(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        S.score_labels(s, 0.3, 0.7)
    with pytest.raises(ValueError):
        S.histogram(s, lab, bins=4097)
    with pytest.raises(ValueError):
        S.histogram(s, lab[:50])
    out = torch.zeros(100, dtype=torch.uint8, device="cuda")
    assert S.score_labels(s, 0.5, out=out) is out


# ---------------------------------------------------------------------------
# batch forms
# ---------------------------------------------------------------------------
CLIP_WINDOWS = [0, 1, 6, 2 * T, 3000, 6]


@pytest.fixture(scope="module")
def zero_batch(torch_cuda):
    from vad_amd.batch import ClipBatch
    clips = [np.zeros(samples_for_windows(w, 400, 160), np.float32) for w in CLIP_WINDOWS]
    b = ClipBatch.from_host(clips)
    assert b.host["n_rows"].tolist() == CLIP_WINDOWS and b.n_windows > sum(CLIP_WINDOWS)  # junk windows between
    return b


def test_batch_forms_equal_the_single_clip_calls(torch_cuda, zero_batch):
    torch = torch_cuda
    from vad_amd import scores as S
    b = zero_batch
    f0s, rows = b.host["frame0"].tolist(), b.host["n_rows"].tolist()
    n = b.n_windows
    rng = np.random.default_rng(7)
    s = rng.random(n).astype(np.float32)
    s[rng.random(n) < 0.05] = np.nan
    # the clip of 6 windows ends active, then undecided; what follows it (junk windows and the next clip's
    # first windows) is undecided too: a leaked carry would call them speech
    k6 = 2
    e6 = f0s[k6] + 6
    s[e6 - 2], s[e6 - 1] = 0.9, 0.5
    s[e6:f0s[k6 + 1] + 40] = 0.5
    lab = (rng.random(n) < 0.01).astype(np.uint8)
    lab[e6 - 1] = 1  # ends active: padding after it stops at the clip's end
    lab[e6:f0s[k6 + 1] + 40] = 0
    lab[f0s[3] + 2 * T - 1] = 1
    ds, dl = dev(torch, s), dev(torch, lab)
    for on, off in THRESHOLDS:
        got = twice(torch, S, n, lambda ws: S.batch_score_labels(ds, b, on, off, ws=ws))
        want = R.per_clip(lambda x: R.hysteresis(x, on, off), s, f0s, rows)
        assert np.array_equal(got, want), (on, off)
        for k, (f0, r) in enumerate(zip(f0s, rows)):
            alone = S.score_labels(ds[f0:f0 + r], on, off).cpu().numpy()
            assert np.array_equal(got[f0:f0 + r], alone), (on, off, k)
    got = S.batch_score_labels(ds, b, 0.7, 0.3).cpu().numpy()
    assert got[e6 - 1] == 1 and not got[e6:f0s[k6 + 1] + 40].any()
    for pad in ((0, 0), (1, 0), (0, 1), (3, 5), (T, T), (n + 5, 0), (0, n + 5)):
        got = twice(torch, S, n, lambda ws: S.batch_dilate_labels(dl, b, pad, ws=ws))
        want = R.per_clip(lambda x: R.dilate(x, 1, *pad), lab, f0s, rows)
        assert np.array_equal(got, want), pad
        for k, (f0, r) in enumerate(zip(f0s, rows)):
            alone = S.dilate_labels(dl[f0:f0 + r], pad).cpu().numpy()
            assert np.array_equal(got[f0:f0 + r], alone), (pad, k)
    got = S.batch_dilate_labels(dl, b, (0, 5)).cpu().numpy()
    assert got[e6 - 1] == 1 and not got[e6:f0s[k6 + 1] + 40].any()
    # a BatchScores / BatchLabels is taken as its tensor
    from vad_amd.batch import BatchLabels
    assert np.array_equal(S.batch_score_labels(S.BatchScores(ds, b), b, 0.5).cpu().numpy(),
                          S.batch_score_labels(ds, b, 0.5).cpu().numpy())
    assert np.array_equal(S.batch_dilate_labels(BatchLabels(dl, b), b, (1, 1)).cpu().numpy(),
                          S.batch_dilate_labels(dl, b, (1, 1)).cpu().numpy())
    with pytest.raises(ValueError):
        S.batch_score_labels(ds[:-1], b, 0.5)


# ---------------------------------------------------------------------------
# FFN scores
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip3000():
    from oracle import vad_oracle as O
    n = 160 * 2999 + 401  # 3,000 frames
    return O.synth_clip(n, seed=41)[:n].astype(np.float32)


def ffn_pipe(name, golden):
    from vad_amd.ffn import FFNClassifier, TOPOLOGY_BL13, random_layers
    from vad_amd.pipeline import VadPipeline
    if name == "bl13":
        return VadPipeline(FFNClassifier(random_layers(TOPOLOGY_BL13, seed=3)))
    w = golden("ffn")
    return VadPipeline(FFNClassifier([(w[f"ref39_W{i}"], w[f"ref39_b{i}"]) for i in range(4)]))


def softmax64(z, active):
    z = z.astype(np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e[:, active] / e.sum(axis=1)


@pytest.mark.parametrize("net", ["bl13", "ref39"])
def test_ffn_scores(torch_cuda, golden, clip3000, net):
    torch = torch_cuda
    from vad_amd import scores as S
    from vad_amd.plan import window_logits
    pipe = ffn_pipe(net, golden)
    audio = dev(torch, clip3000)
    labels, logits = window_logits(pipe.ffn.plan, pipe.mfcc(audio), pipe.mode)
    z = logits.cpu().numpy()
    assert z.shape == (2995, 2 if net == "bl13" else 3)
    fin = np.isfinite(z).all(axis=1)
    assert fin.sum() > 2000
    worst = 0.0
    for active in range(z.shape[1]):
        s = pipe.scores(audio, active=active).cpu().numpy()
        assert s.dtype == np.float32 and s.shape == (2995,)
        assert np.array_equal(s, S.scores_from_logits(logits, active).cpu().numpy())
        assert (s[~fin] == 0).all() and (s >= 0).all() and (s <= 1).all()
        err = np.abs(s[fin].astype(np.float64) - softmax64(z[fin], active)).max()
        worst = max(worst, float(err))
        assert err <= 8 * 2.0 ** -24, (net, active, err)
    print(f"\n{net}: max |score - float64 softmax| = {worst:.3e} = {worst * 2 ** 24:.2f} * 2^-24")
    # int16 PCM: the scores of that clip's own logits
    a16 = dev(torch, clip3000.astype(np.int16))
    _, z16 = window_logits(pipe.ffn.plan, pipe.mfcc(a16), pipe.mode)
    assert np.array_equal(pipe.scores(a16).cpu().numpy(), S.scores_from_logits(z16, 1).cpu().numpy())
    # rows with an injected NaN / inf logit score 0, their neighbours keep their scores
    zz = logits.clone()
    rows = np.flatnonzero(fin)[[0, 7, 500]]
    zz[int(rows[0]), 0] = float("nan")
    zz[int(rows[1]), 1] = float("inf")
    zz[int(rows[2]), z.shape[1] - 1] = float("-inf")
    s0 = S.scores_from_logits(logits, 1).cpu().numpy()
    s1 = S.scores_from_logits(zz, 1).cpu().numpy()
    assert (s1[rows] == 0).all()
    keep = np.ones(len(s0), bool)
    keep[rows] = False
    assert np.array_equal(s0[keep], s1[keep])
    if net == "bl13":
        # the plain threshold at 0.5 is the kernel's argmax wherever the logits differ by 2^-23 or more
        lab = labels.cpu().numpy()
        got = S.score_labels(S.scores_from_logits(logits, 1), 0.5, 0.5).cpu().numpy()
        margin = np.abs(z[:, 1] - z[:, 0])
        sure = fin & (margin >= 2.0 ** -23)
        bad = np.flatnonzero(sure & (got != lab))
        assert bad.size == 0, (f"{bad.size} windows differ; {int((fin & ~sure).sum())} finite windows are below the "
                               f"margin and not compared", bad[:5], z[bad[:5]])
        assert sure.sum() > 2000


def test_scores_from_logits_every_class_count(torch_cuda):
    """1 to 8 classes (odd counts read rows that are only 4-byte aligned), more than one block."""
    torch = torch_cuda
    from vad_amd import scores as S
    rng = np.random.default_rng(3)
    for c in range(1, 9):
        z = (rng.standard_normal((70001, c)) * 4).astype(np.float32)
        z[5] = 80.0  # equal large logits: exp(0), no overflow
        z[6, 0] = -120.0
        d = dev(torch, z)
        for active in {0, c // 2, c - 1}:
            s = S.scores_from_logits(d, active).cpu().numpy()
            err = np.abs(s.astype(np.float64) - softmax64(z, active)).max()
            assert err <= 8 * 2.0 ** -24, (c, active, err)
    with pytest.raises(ValueError):
        S.scores_from_logits(d, 8)
    with pytest.raises(ValueError):
        S.scores_from_logits(torch.zeros((4, 9), device="cuda"), 0)
    assert S.scores_from_logits(torch.zeros((0, 2), device="cuda"), 1).shape == (0,)


# ---------------------------------------------------------------------------
# tree scores
# ---------------------------------------------------------------------------
def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def tree_rows(torch_cuda, clip3000):
    """The device's own feature rows of the clip, both feature modes."""
    from vad_amd import _lib
    from vad_amd.pipeline import VadPipeline
    pipe = VadPipeline()
    audio = dev(torch_cuda, clip3000)
    return {m: pipe.features(audio, mode=m) for m in (_lib.FEAT_ANALYSER, _lib.FEAT_OFFLINE)}


def check_tree(torch, clf, tree, clip, rows, n_classes):
    from vad_amd import _lib, scores as S
    from vad_amd.pipeline import VadPipeline
    audio = dev(torch, clip)
    for mode, name in ((_lib.FEAT_ANALYSER, "analyser"), (_lib.FEAT_OFFLINE, "offline")):
        pipe = VadPipeline(tree, mode=name)
        x = rows[mode]
        xh = x.cpu().numpy()
        proba = clf.predict_proba(xh) if hasattr(clf, "predict_proba") else clf(xh)
        lab = pipe.labels(audio).cpu().numpy()
        for active in range(n_classes):
            want = proba[:, active].astype(np.float32)
            got_w = pipe.scores(audio, active=active).cpu().numpy()
            got_r = S.tree_predict_scores(tree, x, active).cpu().numpy()
            assert got_w.dtype == np.float32 and got_w.shape == (len(xh),)
            assert np.array_equal(bits(got_w), bits(want)), (name, active, np.flatnonzero(got_w != want)[:5])
            assert np.array_equal(bits(got_r), bits(want)), (name, active)
            assert (lab[got_w > 0.5] == active).all()  # a share above one half is the leaf's majority class


def test_tree_scores_lds_table(torch_cuda, golden, clip3000, tree_rows):
    from sklearn.tree import DecisionTreeClassifier
    from vad_amd.tree import TreeClassifier
    gt = golden("tree")
    clf = DecisionTreeClassifier(max_depth=8, min_samples_leaf=5, random_state=0).fit(
        np.nan_to_num(gt["x_test"]), gt["y_test"])
    tree = TreeClassifier.from_sklearn(clf)
    assert tree.feature.shape[0] <= 3072 and len(clf.classes_) >= 2
    check_tree(torch_cuda, clf, tree, clip3000, tree_rows, len(clf.classes_))


def test_tree_scores_global_table(torch_cuda, clip3000, tree_rows):
    """More nodes than the window kernel keeps in LDS (3072): the walk from global memory."""
    from sklearn.tree import DecisionTreeClassifier
    from vad_amd import _lib
    from vad_amd.tree import TreeClassifier
    rng = np.random.default_rng(2)
    x = np.nan_to_num(tree_rows[_lib.FEAT_ANALYSER].cpu().numpy())
    x = np.concatenate([x, x + rng.standard_normal(x.shape).astype(np.float32) * 0.1])
    y = rng.integers(0, 3, len(x))  # labels no split explains: the tree grows to (nearly) one row per leaf
    clf = DecisionTreeClassifier(random_state=0).fit(x, y)
    tree = TreeClassifier.from_sklearn(clf)
    assert tree.feature.shape[0] > 3072
    check_tree(torch_cuda, clf, tree, clip3000, tree_rows, 3)


def test_tree_scores_of_a_trained_tree(torch_cuda, clip3000, tree_rows):
    """A tree from TreeTrainer.fit scores by its integer class counts."""
    from vad_amd import _lib
    from vad_amd.tree_train import TreeTrainer
    x = np.nan_to_num(tree_rows[_lib.FEAT_ANALYSER].cpu().numpy())
    y = (x[:, 0] + 0.3 * np.random.default_rng(4).standard_normal(len(x)) > 0).astype(np.int64)
    tree = TreeTrainer(max_depth=6, min_samples_split=22, min_samples_leaf=20).fit(x, y)
    assert tree.proba is None and tree.value is not None
    v_all = tree.value.astype(np.float64)

    def proba(rows):  # the leaf node of every row by a walk on the host, then its class shares
        leaves = []
        for x in np.asarray(rows, np.float32):
            i = 0
            while tree.feature[i] >= 0:
                v = x[tree.feature[i]]
                left = bool(tree.nan_left[i]) if np.isnan(v) else np.float64(v) <= tree.threshold[i]
                i = tree.left[i] if left else tree.right[i]
            leaves.append(i)
        return (v_all / np.maximum(v_all.sum(axis=1, keepdims=True), 1))[leaves]

    check_tree(torch_cuda, proba, tree, clip3000, tree_rows, 2)


# ---------------------------------------------------------------------------
# reference labels and the histogram
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_reference_labels_and_histogram(torch_cuda, n):
    torch = torch_cuda
    from vad_amd import scores as S
    fs, hop = 400, 160
    rng = np.random.default_rng(n)
    centres = (np.arange(n, dtype=np.int64) + 2) * hop + fs // 2
    # interval ends on window centres and one sample either side of them
    k = min(n // 2, 40)
    pick = np.sort(rng.choice(n, size=2 * k, replace=False)) if k else np.zeros(0, np.int64)
    ends = centres[pick] + rng.integers(-1, 2, size=2 * k)
    iv = ends.reshape(-1, 2)
    for intervals in (iv, iv[:1], np.zeros((0, 2), np.int64), np.array([[0, 2 ** 40]])):
        got = S.reference_labels(intervals, n, fs, hop).cpu().numpy()
        assert np.array_equal(got, R.reference_labels(intervals, n, fs, hop)), (n, len(intervals))
    ref = R.reference_labels(iv, n, fs, hop)
    assert np.array_equal(S.reference_labels((iv[:, 0], iv[:, 1]), n, fs, hop).cpu().numpy(), ref)
    assert np.array_equal(S.reference_labels(dev(torch, iv), n, fs, hop).cpu().numpy(), ref)
    s = rng.random(n).astype(np.float32)
    special = np.array([0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), np.nan, 0.5, 0.25], np.float32)
    where = rng.random(n) < 0.2
    s[where] = rng.choice(special, size=int(where.sum()))
    ds, dr = dev(torch, s), dev(torch, ref)
    for bins in (2, 1024, 4096):
        h = S.histogram(ds, dr, bins).cpu().numpy()
        assert h.dtype == np.int64 and h.shape == (2, bins)
        assert np.array_equal(h, R.histogram(s, ref, bins)), (n, bins)
        assert h.sum(axis=1).tolist() == [int((ref == 0).sum()), int((ref == 1).sum())]
    if n > 1:  # arrays that are not aligned for the four-window loads
        assert np.array_equal(S.histogram(ds[1:], dr[1:], 64).cpu().numpy(), R.histogram(s[1:], ref[1:], 64))
    lab = S.score_labels(ds, 0.5).cpu().numpy()
    c = S.confusion(dev(torch, lab), dr, 2).cpu().numpy()
    assert np.array_equal(c, np.bincount(ref.astype(np.int64) * 2 + lab, minlength=4).reshape(2, 2))
    lab3 = rng.integers(0, 5, n).astype(np.uint8)
    assert np.array_equal(S.confusion(dev(torch, lab3), dr, 4).cpu().numpy(), R.confusion(lab3, ref, 4))
    roc = S.roc(ds, dr, bins=1024)
    want = S.roc_from_histogram(R.histogram(s, ref, 1024))
    assert np.array_equal(roc.tpr, want.tpr) and np.array_equal(roc.fpr, want.fpr)
    assert roc.tpr[-1] == 0 and roc.fpr[-1] == 0 and (np.diff(roc.fpr) <= 0).all()
    t = S.threshold_at(roc, 0.1)
    assert roc.fpr[int(round(t * 1024))] <= 0.1


def test_batch_reference_labels(torch_cuda, zero_batch):
    from vad_amd import scores as S
    b = zero_batch
    rng = np.random.default_rng(9)
    per = []
    for w in CLIP_WINDOWS:
        top = (w + 5) * 160
        k = int(rng.integers(0, 4)) if w > 1 else 0
        per.append(np.sort(rng.choice(top, size=2 * k, replace=False)).reshape(-1, 2))
    per[3] = np.array([[0, 600], [602, 603], [(2 * T + 1) * 160 + 200, 10 ** 9]])  # the first and the last window
    got = S.batch_reference_labels(per, b).cpu().numpy()
    want = np.zeros(b.n_windows, np.uint8)
    for iv, f0, r in zip(per, b.host["frame0"].tolist(), b.host["n_rows"].tolist()):
        want[f0:f0 + r] = R.reference_labels(iv, r, 400, 160)
        assert np.array_equal(got[f0:f0 + r], S.reference_labels(iv, r).cpu().numpy())
    assert np.array_equal(got, want)
    f0 = int(b.host["frame0"][3])
    assert got[f0] == 1 and got[f0 + 1] == 0 and got[f0 + 2 * T - 1] == 1 and got[f0 + 2 * T - 2] == 0


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
NEW_ENTRIES = ["vad_scores_from_logits", "vad_features_tree_scores", "vad_tree_predict_scores",
               "vad_scores_workspace_bytes", "vad_score_labels", "vad_label_dilate", "vad_batch_score_labels",
               "vad_batch_label_dilate", "vad_reference_labels", "vad_batch_reference_labels",
               "vad_score_histogram_f32", "vad_score_histogram_u8"]


def model_chain(s, on, off, max_gap, min_run, pad):
    lab = R.hysteresis(s, on, on if off is None else off)
    return R.dilate(model_smooth(lab, max_gap, min_run), 1, *pad)


def tables_equal(a, b):
    ca, cb = a.counts.cpu().numpy(), b.counts.cpu().numpy()
    return np.array_equal(ca, cb) and np.array_equal(a.numpy(), b.numpy())


@pytest.mark.parametrize("clf", ["bl13", "tree"])
def test_segments_at_an_operating_point(torch_cuda, golden, clip3000, clf, monkeypatch):
    torch = torch_cuda
    from vad_amd import _lib
    from vad_amd.pipeline import VadPipeline
    from vad_amd.segments import label_segments
    if clf == "tree":
        from sklearn.tree import DecisionTreeClassifier
        gt = golden("tree")
        pipe = VadPipeline(DecisionTreeClassifier(max_depth=6, random_state=0).fit(
            np.nan_to_num(gt["x_test"]), gt["y_test"]))
    else:
        pipe = ffn_pipe(clf, golden)
    clip = clip3000[:160 * 1499 + 401]
    audio = dev(torch, clip)
    s = pipe.scores(audio).cpu().numpy()

    def q(p):  # thresholds where this classifier's scores are: its quantile p, as the float32 the entry gets
        return float(np.float32(np.quantile(s[np.isfinite(s)], p)))

    for kw in (dict(on=q(.7), off=q(.3), pad=(2, 3)), dict(on=q(.5)),
               dict(on=q(.6), off=q(.4), max_gap=3, min_run=4, pad=(0, 6)),
               dict(on=q(.9), off=q(.1), pad=(1, 0), max_gap=2)):
        want_lab = model_chain(s, kw["on"], kw.get("off"), kw.get("max_gap", 0), kw.get("min_run", 0),
                               kw.get("pad", (0, 0)))
        want = label_segments(dev(torch, want_lab), len(clip))
        got = pipe.segments(audio, **kw)
        assert tables_equal(got, want), kw
        assert int(got.counts[0]) > 0
        voiced = pipe.voiced(audio, **kw).cpu().numpy()
        rows = np.concatenate([got.numpy(), np.zeros((len(got.numpy()), 1), np.int64)], axis=1)
        assert np.array_equal(voiced, model_voiced(clip, rows)), kw
    # padding alone keeps the classifier's labels
    lab = pipe.labels(audio).cpu().numpy()
    want = label_segments(dev(torch, R.dilate(model_smooth(lab, 2, 0), 1, 1, 4)), len(clip))
    assert tables_equal(pipe.segments(audio, max_gap=2, pad=(1, 4)), want)
    # the defaults take the present path: no entry of the score unit is reached
    before = pipe.segments(audio, max_gap=2, min_run=3)
    v_before = pipe.voiced(audio, max_gap=2, min_run=3)
    handle = _lib.lib()

    def trap(*a, **k):
        raise AssertionError("the default path reached the score unit")

    for name in NEW_ENTRIES:
        monkeypatch.setattr(handle, name, trap)
    after = pipe.segments(audio, max_gap=2, min_run=3)
    assert tables_equal(after, before)
    assert tables_equal(after, label_segments(pipe.labels(audio), len(clip), max_gap=2, min_run=3))
    assert torch.equal(pipe.voiced(audio, max_gap=2, min_run=3), v_before)
    with pytest.raises(AssertionError, match="score unit"):
        pipe.segments(audio, on=0.5)


def test_batch_segments_at_an_operating_point(torch_cuda, golden, clip3000):
    torch = torch_cuda
    from vad_amd.batch import ClipBatch
    pipe = ffn_pipe("bl13", golden)
    lens = [160 * 299 + 401, 0, 401 + 160 * 5, 160 * 1099 + 401, 160 * 40 + 401]
    clips, pos = [], 0
    for n in lens:
        clips.append(clip3000[pos:pos + n])
        pos += n
    b = ClipBatch.from_host(clips)
    sb = pipe.scores_batch(b)
    s = sb.scores.cpu().numpy()
    on, off = (float(np.float32(np.quantile(s[np.isfinite(s)], p))) for p in (.7, .35))
    kw = dict(on=on, off=off, max_gap=2, min_run=2, pad=(2, 3))
    assert len(sb) == len(clips)
    seg = pipe.segments_batch(b, **kw)
    voiced, offsets = pipe.voiced_batch(b, **kw)
    voiced = voiced.cpu().numpy()
    found = 0
    for k, c in enumerate(clips):
        alone = dev(torch, c)
        assert np.array_equal(sb[k].cpu().numpy(), pipe.scores(alone).cpu().numpy()), k
        rows = pipe.segments(alone, **kw).numpy()
        assert np.array_equal(seg.clip(k), rows), k
        found += len(rows)
        assert np.array_equal(voiced[offsets[k]:offsets[k + 1]], pipe.voiced(alone, **kw).cpu().numpy()), k
    assert found > 3 and int(seg.counts[0]) == found
