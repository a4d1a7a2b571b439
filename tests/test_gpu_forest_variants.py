"""Every variant of the forest kernels (forest_kernel.hip) and of the score
kernels at the top of score_kernel.hip, the forest's staging edges and the
loops past the launch caps, against host walks in double.

The forest reference is forest_reference.py (per row K double accumulators,
the trees' shares added in order, one division) on the device's own feature
rows (vad_features_f32, pinned to the fp64 oracle by
test_gpu_features_parity.py): labels equal, scores bit for bit for every
active class.  A tree score is vad_amd.h's class fraction of the leaf
(forest_tables.tree_scores) at the leaf forest_reference.leaves finds for the
tree as a one-tree forest: bit for bit.  Every call writes into buffers 64
elements longer than its result, prefilled with 0xEE (labels) or a NaN of
known payload (scores): nothing past the result may change, and a window the
kernel skipped keeps the fill.

Which parameters select which instantiation, and the cases that run it:

  forest_window_kernel<MN, KT>       mfcc_n      K        cases here
  <13, 2>                            13          2        (a) (b) (c)
  <13, 0>                            13          1, 3, 8  (a); 3 (b) (c)
  <0, 2>                             1, 12, 16   2        (a); 16 (b) (c)
  <0, 0>                             1, 12, 16   3        (a); 16 (b) (c)
  forest_rows_kernel<KT>             -           K
  <2>                                            2        (b) rows, (d)
  <0>                                            3        (b) rows, (d)
  tree_window_score_kernel<MN, LDSN> mfcc_n      nodes
  <13, true>                         13          <= 3072  (e) bushy, bushy_3072, bushy_narrow, comb_3072; chunks
  <13, false>                        13          >= 3073  (e) bushy_3073, comb_3073; chunks, padded
  <0, true>                          1, 12, 16   <= 3072  as <13, true>; chunks at 16
  <0, false>                         1, 12, 16   >= 3073  as <13, false>; chunks at 16
  tree_rows_score_kernel             -           -        (d)
  logit_scores_kernel<C>             -           C 1..8   (d), each C

  (a) test_variant_matrix: a mixed forest (pairs, tails, a global tree, a
      one-node tree) at 1, 255, 256, 257 and 1,000 windows, both modes.
      K = 1 is reached through ForestClassifier, which accepts one class.
  (b) test_staging_edges / test_staging_edges_feature_rows: every named size
      list of forest_tables.py -- dozens of small trees in a buffer of R
      nodes, groups of exactly buf_nodes nodes and one node past it, global
      trees first, between and last, no staged tree at all, 3,071-node chains
      paired with one- and three-node trees in either order, T = 1, 2, 3.
  (c) test_chunk_loop: one chunk more than the 4 x CUs blocks of the window
      launch and a ragged one: the first blocks load a second chunk's MFCC
      rows over the staged trees and stage every group again; once more after
      the LDS of every CU was filled with 1e30, -1e30 and NaN.
  (d) test_flat_grid_*: 257 rows more than the 8 x CUs blocks of 256 the flat
      launches are capped at.
  (e) test_tree_score_variants / test_tree_score_chunk_loop: the tables of
      tree_tables.variant_tables, and the chunk loop of (c).

What these tests rely on -- the grouping of every size list under the staging
rule, windows reaching several leaves of every tree, NaN met at nodes of
either flag, walks of more than 1,000 nodes beside one-node trees -- is
asserted on the references alone in test_forest_tables_cpu.py."""
import ctypes
import functools
import itertools
import os

import numpy as np
import pytest

import forest_reference as FR
import forest_tables as FT
import tree_tables as T
from stream_tree_reference import KEYS as TREE_KEYS

pytestmark = pytest.mark.gpu

MODES = ("analyser", "offline")
GUARD = 64
LABEL_FILL = 0xEE
SCORE_FILL = 0x7FC0BEEF  # a quiet NaN no kernel produces
RUNS = tuple(range(20, 300, 40))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _mode(name):
    from vad_amd import _lib
    return _lib.FEAT_ANALYSER if name == "analyser" else _lib.FEAT_OFFLINE


def _features(m, mode):
    from vad_amd.plan import window_features
    return window_features(m, _mode(mode)).cpu().numpy()


def _rows(W, mfcc_n, runs=()):
    import torch
    return torch.from_numpy(T.mfcc_like_rows(5 + W, mfcc_n, seed=mfcc_n, runs=runs)).cuda()


def _classifier(f):
    from vad_amd.forest import ForestClassifier
    return ForestClassifier(*(f[k] for k in FR.KEYS), np.arange(f["K"]), f["n_features"])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Guarded:
    """An output of n elements inside a buffer GUARD longer, prefilled."""

    def __init__(self, n, kind):
        import torch
        self.n, self.kind = n, kind
        if kind == "labels":
            self.buf = torch.full((n + GUARD,), LABEL_FILL, dtype=torch.uint8, device="cuda")
        else:
            self.buf = torch.full((n + GUARD,), SCORE_FILL, dtype=torch.int32, device="cuda").view(torch.float32)
        self.out = self.buf[:n]

    def result(self, returned):
        """The result as numpy, after checking that the call returned the
        buffer it was given and left the guard alone."""
        assert returned.data_ptr() == self.buf.data_ptr() and tuple(returned.shape) == (self.n,)
        h = self.buf.cpu().numpy()
        if self.kind == "labels":
            assert (h[self.n:] == LABEL_FILL).all(), "labels written past n"
        else:
            assert (h[self.n:].view(np.uint32) == SCORE_FILL).all(), "scores written past n"
        return h[:self.n]


def _same(got, want, what):
    """Exact equality (scores: of the bit patterns), with the count of
    differing elements in the message."""
    if want.dtype == np.float32:
        got, want = bits(got), bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} differ, first at {bad[:5].tolist()}"


def check_windows(forest, f, m, mode, feats, before=None, proba=None):
    """window_labels and window_scores (every active class) of device MFCC
    rows m against the reference on the feature rows feats (proba: its
    result, where a caller has it).  before(): called ahead of every launch."""
    n = len(feats)
    if proba is None:
        proba = FR.predict_proba(f, feats)
    g = Guarded(n, "labels")
    if before:
        before()
    _same(g.result(forest.window_labels(m, _mode(mode), out=g.out)), np.argmax(proba, axis=1).astype(np.uint8),
          f"labels, {mode}")
    for active in range(f["K"]):
        g = Guarded(n, "scores")
        if before:
            before()
        _same(g.result(forest.window_scores(m, _mode(mode), active, out=g.out)), proba[:, active].astype(np.float32),
              f"scores of class {active}, {mode}")
    return proba


def check_rows(forest, f, x):
    """predict_device and predict_scores of host feature rows x."""
    import torch
    xd = torch.from_numpy(x).cuda()
    n = len(x)
    proba = FR.predict_proba(f, x)
    g = Guarded(n, "labels")
    _same(g.result(forest.predict_device(xd, out=g.out)), np.argmax(proba, axis=1).astype(np.uint8), "row labels")
    for active in range(f["K"]):
        g = Guarded(n, "scores")
        _same(g.result(forest.predict_scores(xd, active, out=g.out)), proba[:, active].astype(np.float32),
              f"row scores of class {active}")
    return proba


def with_nans(x, seed):
    """x with one entry in twenty NaN."""
    x = np.array(x, np.float32)
    x[np.random.default_rng(seed).random(x.shape) < 0.05] = np.nan
    return x


# ---------------------------------------------------------------------------
# a. the four window variants, one matrix
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(mfcc_n, mode):
    """Per window count: device MFCC rows and the device's features.  Never
    written afterwards."""
    rows = {W: _rows(W, mfcc_n) for W in T.WINDOWS}
    return rows, {W: _features(m, mode) for W, m in rows.items()}


MATRIX = [(n, K) for n in T.WIDTHS for K in (2, 3)] + [(13, 8), (13, 1)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mfcc_n,K", MATRIX)
def test_variant_matrix(torch_cuda, mfcc_n, K, mode):
    rows, feats = _inputs(mfcc_n, mode)
    f = FT.build_forest(FT.MIXED, feats[1000], K, seed=10 * mfcc_n + K)
    assert f["n_features"] == 3 * mfcc_n and f["proba"].shape[1] == K and FT.sizes_of(f) == FT.MIXED
    forest = _classifier(f)
    for W in T.WINDOWS:
        assert feats[W].shape == (W, 3 * mfcc_n)
        proba = check_windows(forest, f, rows[W], mode, feats[W])
    # what makes the comparison bite, on the device's own features
    assert min(r for r, n in zip(FT.leaves_per_tree(f, feats[1000]), FT.MIXED) if n > 1) >= 2
    assert K == 1 or len(set(np.argmax(proba, axis=1).tolist())) >= 2
    if mode == "analyser":
        assert FT.nan_flags_met(f, feats[1000]) == {0, 1}


# ---------------------------------------------------------------------------
# b. the staging edges
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rows_300(mfcc_n, mode):
    m = _rows(300, mfcc_n, runs=RUNS)
    return m, _features(m, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mfcc_n", FT.STAGING_WIDTHS)
@pytest.mark.parametrize("name", FT.NAMES)
def test_staging_edges(torch_cuda, name, mfcc_n, mode):
    m, feats = _rows_300(mfcc_n, mode)
    assert feats.shape == (300, 3 * mfcc_n)
    for K in (2, 3):
        f = FT.named_forest(name, feats, K)
        assert FT.sizes_of(f) == FT.size_list(name, mfcc_n)
        proba = check_windows(_classifier(f), f, m, mode, feats)
        assert len(set(np.argmax(proba, axis=1).tolist())) >= 2
    assert min(r for r, n in zip(FT.leaves_per_tree(f, feats), FT.sizes_of(f)) if n > 1) >= 2
    if name == "deep_pairs":
        deep = [FT.walk_depths(f, t, feats).max() for t, n in enumerate(FT.sizes_of(f)) if n == FT.CHAIN]
        assert len(deep) == 4 and min(deep) > 1000


@pytest.mark.parametrize("mfcc_n", FT.STAGING_WIDTHS)
@pytest.mark.parametrize("name", FT.NAMES)
def test_staging_edges_feature_rows(torch_cuda, name, mfcc_n):
    """vad_forest_predict on the same forests: the windows' feature rows with
    NaNs planted."""
    _, feats = _rows_300(mfcc_n, "analyser")
    x = with_nans(feats, seed=mfcc_n)
    assert np.isnan(x).sum() > np.isnan(feats).sum() + 100
    for K in (2, 3):
        f = FT.named_forest(name, feats, K)
        proba = check_rows(_classifier(f), f, x)
        assert len(set(np.argmax(proba, axis=1).tolist())) >= 2


# ---------------------------------------------------------------------------
# c. the chunk loop
# ---------------------------------------------------------------------------
def _cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _chunk_inputs(mfcc_n):
    """One chunk more than the window launches' 4 x CUs blocks and a ragged
    one, a constant run in the last: the device rows, the features, and a
    sample of the features (one window in 16 and the last chunks whole) to
    fit trees on.  Never written afterwards."""
    import torch
    first = 4 * _cus(torch) * 256
    W = first + 257
    m = _rows(W, mfcc_n, runs=(first + 100,))
    feats = _features(m, "analyser")
    assert feats.shape == (W, 3 * mfcc_n) and np.isnan(feats[first:, 0]).any()
    return first, m, feats, np.concatenate([feats[:first:16], feats[first:]])


def _poison(torch):
    """The LDS poison helper, as test_gpu_forest.py loads it."""
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_host", "liblds_poison.so")
    if not os.path.exists(so):
        pytest.fail("tests/c_host/liblds_poison.so missing: run __graft_entry__.build()")
    helper = ctypes.CDLL(so)
    helper.lds_poison.argtypes = [ctypes.c_float, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    sink = torch.zeros(1, device="cuda")
    values = itertools.cycle([1e30, -1e30, float("nan")])

    def before():
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert helper.lds_poison(next(values), ctypes.c_void_p(sink.data_ptr()), 4 * _cus(torch), st) == 0

    return before, sink


@pytest.mark.parametrize("mfcc_n,K", [(13, 2), (13, 3), (16, 2), (16, 3)])
def test_chunk_loop(torch_cuda, mfcc_n, K):
    """The first blocks take a second chunk: its MFCC rows overwrite the
    staged trees, and every group is staged again.  Every window is compared;
    a chunk the loop left out keeps the fill."""
    torch = torch_cuda
    first, m, feats, sample = _chunk_inputs(mfcc_n)
    f = FT.build_forest(FT.CHUNK, sample, K, seed=mfcc_n + K)
    groups = FT.staging_groups(FT.sizes_of(f), mfcc_n)
    assert sum(kind == "lds" for kind, _ in groups) >= 2 and sum(kind == "global" for kind, _ in groups) == 1
    forest = _classifier(f)
    proba = check_windows(forest, f, m, "analyser", feats)
    assert len(set(np.argmax(proba[first:], axis=1).tolist())) >= 2
    assert min(FT.leaves_per_tree(f, feats[first:])) >= 2
    # once more with stale LDS: one poison value per launch
    before, sink = _poison(torch)
    check_windows(forest, f, m, "analyser", feats, before=before, proba=proba)
    torch.cuda.synchronize()
    assert sink.item() == 0.0


# ---------------------------------------------------------------------------
# d. the flat grids
# ---------------------------------------------------------------------------
def _flat_n(torch):
    return 8 * _cus(torch) * 256 + 257


@functools.lru_cache(maxsize=None)
def _flat_x(n):
    x = (np.random.default_rng(n).standard_normal((n, 3)) * 1.5).astype(np.float32)
    return with_nans(x, seed=3)


@pytest.mark.parametrize("K", [2, 3])
def test_flat_grid_forest_rows(torch_cuda, K):
    n = _flat_n(torch_cuda)
    x = _flat_x(n)
    f = FT.build_forest([31, 1, 63], x[:4000], K, seed=K)
    assert f["n_features"] == 3
    proba = check_rows(_classifier(f), f, x)
    tail = np.argmax(proba[n - 257:], axis=1)
    assert len(set(tail.tolist())) >= 2 and min(FT.leaves_per_tree(f, x[n - 257:])[::2]) >= 2


def test_flat_grid_tree_rows(torch_cuda):
    import torch
    from vad_amd import scores as S
    from vad_amd.tree import TreeClassifier
    n = _flat_n(torch_cuda)
    x = _flat_x(n)
    t = FT.build_tree(63, x[:4000], 3, seed=9)
    table = dict(t, classes=np.arange(3), n_features=3)
    p = FT.table_proba(table, seed=4)
    tree = TreeClassifier(*(table[k] for k in TREE_KEYS), 3, proba=p)
    leaf = FR.leaves(FT.as_forest(table, p), x)[0]
    assert len(set(leaf[n - 257:].tolist())) >= 8
    xd = torch.from_numpy(x).cuda()
    for active in range(3):
        g = Guarded(n, "scores")
        _same(g.result(S.tree_predict_scores(tree, xd, active, out=g.out)), FT.tree_scores(p, active)[leaf],
              f"tree row scores of class {active}")


def softmax64(z, active):
    z = z.astype(np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e[:, active] / e.sum(axis=1)


@pytest.mark.parametrize("C", range(1, 9))
def test_flat_grid_logit_scores(torch_cuda, C):
    """The float64 softmax and the bound of
    test_gpu_scores.py::test_scores_from_logits_every_class_count."""
    import torch
    from vad_amd import scores as S
    n = _flat_n(torch_cuda)
    z = (np.random.default_rng(C).standard_normal((n, C)) * 4).astype(np.float32)
    d = torch.from_numpy(z).cuda()
    for active in sorted({0, C - 1}):
        g = Guarded(n, "scores")
        s = g.result(S.scores_from_logits(d, active, out=g.out))
        assert (bits(s) != SCORE_FILL).all()
        err = np.abs(s.astype(np.float64) - softmax64(z, active))
        print(f"C = {C}, active {active}: max |score - float64 softmax| = {err.max() * 2 ** 24:.2f} * 2^-24")
        assert err.max() <= 8 * 2.0 ** -24, (C, active, err.max(), int(np.argmax(err)))


# ---------------------------------------------------------------------------
# e. the tree score variants
# ---------------------------------------------------------------------------
def _scored_tree(table, seed):
    from vad_amd.tree import TreeClassifier
    p = FT.table_proba(table, seed)
    return TreeClassifier(*(table[k] for k in TREE_KEYS), table["n_features"], proba=p), p


def check_tree_scores(tree, table, p, m, mode, feats):
    from vad_amd import scores as S
    leaf = FR.leaves(FT.as_forest(table, p), feats)[0]
    assert (table["feature"][leaf] < 0).all()
    for active in (0, p.shape[1] - 1):
        g = Guarded(len(feats), "scores")
        _same(g.result(S.tree_window_scores(tree, m, _mode(mode), active, out=g.out)),
              FT.tree_scores(p, active)[leaf], f"tree scores of class {active}, {len(feats)} windows")
    return leaf


@pytest.mark.parametrize("name", T.TREES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mfcc_n", T.WIDTHS)
def test_tree_score_variants(torch_cuda, mfcc_n, mode, name):
    rows, feats = _inputs(mfcc_n, mode)
    table = _variant_tables(mfcc_n, mode)[name]
    assert len(table["feature"]) == (511 if name in ("bushy", "bushy_narrow") else int(name.split("_")[1]))
    tree, p = _scored_tree(table, seed=len(name) + mfcc_n)
    for W in T.WINDOWS:
        leaf = check_tree_scores(tree, table, p, rows[W], mode, feats[W])
    assert len(set(leaf.tolist())) >= (100 if name.startswith("bushy") else 250)
    assert len(set(bits(FT.tree_scores(p, 0)[leaf]).tolist())) >= (100 if name.startswith("bushy") else 250)


@functools.lru_cache(maxsize=None)
def _variant_tables(mfcc_n, mode):
    return T.variant_tables(_inputs(mfcc_n, mode)[1][1000], mfcc_n)[0]


@pytest.mark.parametrize("mfcc_n", [13, 16])
def test_tree_score_chunk_loop(torch_cuda, mfcc_n):
    """The chunk loop of (c) for an LDS table and the same table padded to
    3,073 nodes (walked from global memory)."""
    first, m, feats, sample = _chunk_inputs(mfcc_n)
    table = T.bushy_table(3 * mfcc_n, 10, sample, seed=mfcc_n)
    assert len(table["feature"]) == 2047
    for t in (table, T.pad_table(table, T.LDS_NODES + 1)):
        tree, p = _scored_tree(t, seed=mfcc_n)
        leaf = check_tree_scores(tree, t, p, m, "analyser", feats)
        assert len(set(leaf[first:].tolist())) >= 100
