"""Every variant of the decision tree's window kernel (tree_kernel.hip,
launch_tree_windows) and its table edges against a host walk in double.

The reference is oracle.vad_oracle.tree_predict (float32 feature promoted to
double, compared with the double threshold, NaN following nan_left) on the
device's own feature rows (vad_features_f32, pinned to the fp64 oracle by
test_gpu_features_parity.py).  Every comparison is exact equality of the
labels of all windows.

Which parameters select which instantiation of tree_window_kernel<MN, LDSN>:

  instantiation   mfcc_n        nodes     cases here
  <13, true>      13            <= 3072   bushy, bushy_3072, bushy_narrow, comb_3072 (a); bushy (b);
                                          ladders, width 13 (c); one node, stump (d)
  <13, false>     13            >= 3073   bushy_3073, comb_3073 (a); bushy padded (b);
                                          padded ladders, width 13 (c); padded one node, stump (d)
  <0, true>       1, 12, 16     <= 3072   as <13, true>, widths 1, 12, 16 (a), 16 (b, c, d)
  <0, false>      1, 12, 16     >= 3073   as <13, false>, widths 1, 12, 16 (a), 16 (b, c, d)

  (a) test_variant_matrix, (b) test_grid_stride_loop, (c) test_table_edges /
  test_single_thresholds, (d) test_one_node_tree / test_stump_all_nan; the
  fuzzed widths 1..16, padded or not: test_gpu_fuzz.py
  test_fuzz_tree_windows_any_width.  vad_tree_predict (tree_rows_kernel)
  walks the same tables in (c) and (d).

The tables and inputs come from tree_tables.py; what these tests rely on
(classes reached, NaN met at nodes of either flag, rows leaving the combs all
along them, ladder leaves reached) is asserted on the oracle alone in
test_tree_tables_cpu.py."""
import functools

import numpy as np
import pytest

from oracle import vad_oracle as O

import tree_tables as T

pytestmark = pytest.mark.gpu

MODES = ("analyser", "offline")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _mode(name):
    from vad_amd import _lib
    return _lib.FEAT_ANALYSER if name == "analyser" else _lib.FEAT_OFFLINE


def _features(m, mode):
    """The device's feature rows of device MFCC rows m, as float32 numpy."""
    from vad_amd.plan import window_features
    return window_features(m, _mode(mode)).cpu().numpy()


def _window_labels(table, m, mode):
    """Class values of every window of device MFCC rows m."""
    lab = T.classifier(table).window_labels(m, _mode(mode)).cpu().numpy()
    return table["classes"][lab.astype(np.int64)]


def _reference(table, feats):
    return O.tree_predict(table, feats[:, :table["n_features"]])


def _rows(W, mfcc_n, runs=()):
    import torch
    return torch.from_numpy(T.mfcc_like_rows(5 + W, mfcc_n, seed=mfcc_n, runs=runs)).cuda()


# ---------------------------------------------------------------------------
# a. the four variants, one matrix
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(mfcc_n, mode):
    """Per window count: device MFCC rows and the device's features; and the
    tables, built on the 1,000-window features.  Never written afterwards."""
    rows = {W: _rows(W, mfcc_n) for W in T.WINDOWS}
    feats = {W: _features(m, mode) for W, m in rows.items()}
    tables, depth = T.variant_tables(feats[1000], mfcc_n)
    return rows, feats, tables, depth


@functools.lru_cache(maxsize=None)
def _matrix_labels(mfcc_n, mode, tree):
    rows, _, tables, _ = _inputs(mfcc_n, mode)
    return {W: _window_labels(tables[tree], rows[W], mode) for W in T.WINDOWS}


@pytest.mark.parametrize("tree", T.TREES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mfcc_n", T.WIDTHS)
def test_variant_matrix(torch_cuda, mfcc_n, mode, tree):
    _, feats, tables, depth = _inputs(mfcc_n, mode)
    table = tables[tree]
    assert len(table["feature"]) == (511 if tree in ("bushy", "bushy_narrow") else int(tree.split("_")[1]))
    assert table["n_features"] == (T.narrow_features(mfcc_n) if tree == "bushy_narrow" else 3 * mfcc_n)
    got = _matrix_labels(mfcc_n, mode, tree)
    for W in T.WINDOWS:
        assert feats[W].shape == (W, 3 * mfcc_n)
        want = _reference(table, feats[W])
        assert got[W].shape == want.shape == (W,)
        assert np.array_equal(got[W], want), (W, int((got[W] != want).sum()))
    # what makes the comparison bite, on the device's own features
    if tree.startswith("bushy"):
        assert len(set(got[1000].tolist())) >= 3
        if mode == "analyser":
            met = T.nan_nodes(table, feats[1000])
            assert len({r for r, _ in met}) >= 20 and {int(table["nan_left"][n]) for _, n in met} == {0, 1}
    else:
        d = depth[tree]
        assert len(set(d.tolist())) > 1000 // 4 and d.max() > len(table["feature"]) // 4
        assert len(set(got[1000].tolist())) == 2


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mfcc_n", T.WIDTHS)
def test_bushy_forms_agree(torch_cuda, mfcc_n, mode):
    """The same tree unpadded, padded to 3072 nodes (LDS) and to 3073 (global
    memory): identical labels."""
    a, b, c = (_matrix_labels(mfcc_n, mode, t) for t in ("bushy", "bushy_3072", "bushy_3073"))
    for W in T.WINDOWS:
        assert np.array_equal(a[W], b[W]) and np.array_equal(a[W], c[W]), W


# ---------------------------------------------------------------------------
# b. the grid-stride loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mfcc_n", [13, 16])
def test_grid_stride_loop(torch_cuda, mfcc_n):
    """One window chunk more than the 4 x CUs blocks the launch is capped at,
    and a ragged one after it: the first blocks take a second chunk and reuse
    their LDS rows and features."""
    torch = torch_cuda
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    first = 4 * cus * 256
    W = first + 257
    m = _rows(W, mfcc_n, runs=(first + 100,))
    feats = _features(m, "analyser")
    assert feats.shape == (W, 3 * mfcc_n)
    sample = np.concatenate([feats[:first:16], feats[first:]])
    table = T.bushy_table(3 * mfcc_n, 10, sample, seed=mfcc_n)
    assert len(table["feature"]) == 2047
    want = _reference(table, feats)
    assert len(set(want[first:].tolist())) >= 2 and np.isnan(feats[first:, 0]).any()
    for t in (table, T.pad_table(table, T.LDS_NODES + 1)):
        got = _window_labels(t, m, "analyser")
        assert got.shape == (W,)
        assert np.array_equal(got, want), int((got != want).sum())


# ---------------------------------------------------------------------------
# c. table edges, all three walks
# ---------------------------------------------------------------------------
def _planted(values, mfcc_n, seed):
    """MFCC rows whose column 0 holds `values` at rows 2.., the centre rows of
    windows 0..len(values) - 1: in offline mode feature 0 of window w is
    values[w] itself."""
    import torch
    m = T.mfcc_like_rows(len(values) + 5, mfcc_n, seed=seed)
    m[2:2 + len(values), 0] = values
    return torch.from_numpy(m).cuda()


def _three_walks(table_of, values):
    """table_of(feature, n_features) -> table.  Labels of `values` through
    vad_tree_predict (the tested feature alone, and last of 39 and of 64),
    the LDS window walk and the global window walk (widths 13 and 16, offline
    mode, feature 0): each equal to the oracle's; returns them."""
    rng = np.random.default_rng(len(values))
    one = table_of(0, 1)
    want = O.tree_predict(one, values[:, None])
    for F in (1, 39, 64):
        x = (rng.standard_normal((len(values), F)) * 10).astype(np.float32)
        x[rng.random(x.shape) < 0.05] = np.nan
        x[:, F - 1] = values
        table = table_of(F - 1, F)
        got = T.classifier(table).predict(x)
        assert np.array_equal(O.tree_predict(table, x), want)
        assert np.array_equal(got, want), (F, int((got != want).sum()))
    for mfcc_n in (13, 16):
        m = _planted(values, mfcc_n, seed=mfcc_n)
        feats = _features(m, "offline")
        assert np.array_equal(feats[:, 0].view(np.uint32), values.view(np.uint32))
        table = table_of(0, 3 * mfcc_n)
        assert np.array_equal(_reference(table, feats), want)
        for t in (table, T.pad_table(table, T.LDS_NODES + 1)):
            got = _window_labels(t, m, "offline")
            assert np.array_equal(got, want), (mfcc_n, len(t["feature"]), int((got != want).sum()))
    return want


@pytest.mark.parametrize("nan_down", [False, True], ids=["nan_leaves_at_root", "nan_down_the_spine"])
@pytest.mark.parametrize("name", ["edge", "tie"])
def test_table_edges(torch_cuda, name, nan_down):
    thr = T.EDGE_THRESHOLDS if name == "edge" else T.TIE_THRESHOLDS
    values = T.edge_inputs(thr)
    lab = _three_walks(lambda f, F: T.ladder_table(thr, f, F, nan_down=nan_down), values)
    assert lab[np.isnan(values)][0] == (len(thr) if nan_down else 0)
    fin = ~np.isnan(values)
    assert len(set(lab[fin].tolist())) >= 0.9 * (len(thr) + 1)
    if name == "edge":
        assert len(thr) == 255 and 255 in lab[fin] and 0 in lab[fin]  # the largest class a label holds
        # float denormals and +-0 stand on opposite sides of the thresholds 0.0 and -5e-324 / 5e-324:
        # a compare that flushed denormals would merge them
        at = {float(v): int(c) for v, c in zip(values[fin], lab[fin])}
        d, zero = float(T.DENORM_MIN), int(np.searchsorted(thr, 0.0))
        assert thr[zero] == 0.0 and thr[zero - 1] == -5e-324 and thr[zero + 1] == 5e-324
        assert at[0.0] == zero and lab[fin][np.signbit(values[fin]) & (values[fin] == 0)][0] == zero
        assert at[-d] == int(np.searchsorted(thr, -d)) < zero - 1
        assert at[d] == int(np.searchsorted(thr, d)) > zero + 1


@pytest.mark.parametrize("thr", T.SINGLE_THRESHOLDS, ids=[repr(float(t)) for t in T.SINGLE_THRESHOLDS])
def test_single_thresholds(torch_cuda, thr):
    """One-rung ladders over +-0.0, the double denormals and +-inf, fed +-0,
    the float denormals, +-FLT_MAX, +-inf and NaN."""
    values = np.concatenate([T.EDGE_VALUES, np.array([np.nan], np.float32)])
    d = T.DENORM_MIN
    for nan_down in (False, True):
        lab = _three_walks(lambda f, F: T.ladder_table([thr], f, F, nan_down=nan_down), values)
        at = {(float(v), bool(np.signbit(v))): int(c) for v, c in zip(values, lab) if not np.isnan(v)}
        if np.isfinite(thr):
            assert at[float(d), False] == 1 and at[float(-d), True] == 0
            assert at[0.0, False] == at[0.0, True] == (0 if thr >= -0.0 else 1)
        else:
            assert set(at.values()) == {0} if thr > 0 else (at[-np.inf, True] == 0 and at[float(-T.F32.max), True] == 1)


# ---------------------------------------------------------------------------
# d. degenerate tables
# ---------------------------------------------------------------------------
def _tiny(feature, threshold, left, right, leaf, nan_left, n_features):
    return dict(feature=np.array(feature, np.int32), threshold=np.array(threshold, np.float64),
                left=np.array(left, np.int32), right=np.array(right, np.int32), leaf=np.array(leaf, np.int32),
                nan_left=np.array(nan_left, np.uint8), classes=np.arange(4), n_features=n_features)


@pytest.mark.parametrize("mfcc_n", [13, 16])
def test_one_node_tree(torch_cuda, mfcc_n):
    """The root is a leaf of class 3."""
    W = 300
    one = _tiny([-1], [0.0], [-1], [-1], [3], [0], 3 * mfcc_n)
    m = _rows(W, mfcc_n)
    x = _features(m, "analyser")
    assert (T.classifier(one).predict(x) == 3).all()
    for mode in MODES:
        for t in (one, T.pad_table(one, T.LDS_NODES + 1)):
            got = _window_labels(t, m, mode)
            assert got.shape == (W,) and (got == 3).all()


@pytest.mark.parametrize("nan_left", [0, 1])
@pytest.mark.parametrize("mfcc_n", [13, 16])
def test_stump_all_nan(torch_cuda, mfcc_n, nan_left):
    """A 3-node stump on feature 0 (Mn of coefficient 0) of rows whose
    coefficient 0 is constant: every window's feature 0 is NaN."""
    import torch
    W = 300
    stump = _tiny([0, -1, -1], [0.0, 0.0, 0.0], [1, -1, -1], [2, -1, -1], [0, 1, 2], [nan_left, 0, 0], 3 * mfcc_n)
    rows = T.mfcc_like_rows(5 + W, mfcc_n, seed=7)
    rows[:, 0] = rows[0, 0]
    m = torch.from_numpy(rows).cuda()
    x = _features(m, "analyser")
    assert np.isnan(x[:, 0]).all() and (O.tree_predict(stump, x) == (1 if nan_left else 2)).all()
    assert (T.classifier(stump).predict(x) == (1 if nan_left else 2)).all()
    for t in (stump, T.pad_table(stump, T.LDS_NODES + 1)):
        got = _window_labels(t, m, "analyser")
        assert got.shape == (W,) and (got == (1 if nan_left else 2)).all()
