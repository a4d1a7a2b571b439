"""The tree in the stream, host side: the test helpers themselves
(stream_tree_reference.py) against the oracle's tree_predict, the new C
symbols, and a refusal that needs no device."""
import numpy as np
import pytest

from oracle import vad_oracle as O

import stream_tree_reference as R

NEW_SYMBOLS = ("vad_stream_hops_tree", "vad_stream_hops_tree_i16", "vad_stream_step_tree",
               "vad_stream_tree_max_lds_nodes")


def _walk_one(tree, x):
    """One row, one node at a time: (class value, margin, depth)."""
    node, margin, depth = 0, np.inf, 0
    while tree["feature"][node] >= 0:
        f, thr = tree["feature"][node], tree["threshold"][node]
        v = np.float64(np.float32(x[f]))
        if np.isnan(v):
            go_left = tree["nan_left"][node] != 0
        else:
            go_left = v <= thr
            margin = min(margin, abs(v - thr) / max(1.0, abs(thr)))
        node = tree["left"][node] if go_left else tree["right"][node]
        depth += 1
    return tree["classes"][tree["leaf"][node]], margin, depth


def test_margin_helper_against_a_plain_walk():
    tree = R.fixture_tree()
    rng = np.random.default_rng(5)
    X = rng.standard_normal((300, 39)).astype(np.float32) * 3
    X[::7, rng.integers(0, 13, 43)] = np.nan
    margin, depth = R.path_margin(tree, X)
    pred = O.tree_predict(tree, X)
    for i in range(0, 300, 3):
        c, m, d = _walk_one(tree, X[i])
        assert c == pred[i] and d == depth[i]
        assert m == margin[i] or (np.isinf(m) and np.isinf(margin[i]))
    assert depth.max() > 5 and len(set(pred.tolist())) == 2


def test_margin_bounds_what_a_perturbation_can_change():
    """Every feature moved by less than the margin (max(1, |thr|) >= 1): the
    same leaf."""
    tree = R.fixture_tree()
    rng = np.random.default_rng(6)
    X = rng.standard_normal((2000, 39)) * 2
    X32 = X.astype(np.float32)
    margin, _ = R.path_margin(tree, X32)
    ok = margin > 1e-3
    assert ok.mean() > 0.5
    for sign in (-1.0, 1.0):
        Y = (X32.astype(np.float64) + sign * 0.9e-3 * rng.uniform(0, 1, X.shape)).astype(np.float32)
        assert np.array_equal(O.tree_predict(tree, Y)[ok], O.tree_predict(tree, X32)[ok])


@pytest.mark.parametrize("n_nodes", [3, 4, 101, 9000, 9001])
def test_comb_table_against_tree_predict(n_nodes):
    rng = np.random.default_rng(n_nodes)
    X = rng.standard_normal((60, 39)).astype(np.float32)
    cols = list(range(13, 26))
    tree, depth = R.comb_table(n_nodes, X, cols)
    assert len(tree["feature"]) == n_nodes and tree["n_features"] == 39
    D = (n_nodes - 1) // 2
    internal = tree["feature"] >= 0
    assert internal.sum() == D
    for a in (tree["left"][internal], tree["right"][internal]):
        assert a.min() >= 1 and a.max() < n_nodes
    assert set(tree["feature"][internal].tolist()) <= set(cols)
    # the comb, evaluated directly: the first spine node whose test holds
    spine = 2 * np.arange(D)
    hit = X[:, tree["feature"][spine]].astype(np.float64) <= tree["threshold"][spine][None, :]
    first = np.where(hit.any(axis=1), hit.argmax(axis=1), D)
    want = first % 2
    assert np.array_equal(O.tree_predict(tree, X), want)
    m, d = R.path_margin(tree, X)
    assert np.array_equal(d, np.where(first < D, first + 1, D)) and np.array_equal(d, depth)
    assert (m > 0).all()  # midpoints: no row sits on a threshold
    if D >= 60:
        assert len(set(d.tolist())) >= 50 and d.max() > D // 2  # rows leave all along the spine
        assert len(set(want.tolist())) == 2


def test_oracle_figures_of_the_streaming_case():
    """The oracle-only figures test_gpu_stream_tree's fp64 comparison rests
    on: 8 clips x 35 windows, 1 of 280 within 1e-3 of a threshold, the labels
    133 / 147."""
    tree = R.fixture_tree()
    S, T = 8, 40
    fb = O.get_mel_filterbanks(300, 8000, 512, 26, 16000)
    n_close, counts = 0, np.zeros(2, np.int64)
    for s in range(S):
        x = O.analyser_features_fast(O.mfcc_batch(O.synth_clip(160 * (T - 1) + 401, seed=700 + s), fb))
        assert x.shape == (T - 5, 39)
        margin, _ = R.path_margin(tree, x)
        n_close += int((margin <= 1e-3).sum())
        lab = O.tree_predict(tree, x)
        counts += np.array([(lab == c).sum() for c in tree["classes"]])
    assert n_close == 1
    assert sorted(counts.tolist()) == [133, 147]


def test_library_exports_the_new_entries():
    from vad_amd import _lib
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.vad_stream_tree_max_lds_nodes(None) == -1


def test_null_plans_are_refused_without_a_device():
    from vad_amd import _lib
    lib = _lib.lib()
    A = 0x10000  # never dereferenced
    for fn in (lib.vad_stream_hops_tree, lib.vad_stream_hops_tree_i16):
        assert fn(None, None, A, 400, 400, A, 160, 160, 4, 1, 0, A, A, A, 0, 0, None) == _lib.VAD_EINVAL
        assert fn(None, A, A, 400, 400, A, 160, 160, 4, 1, 0, A, A, A, 0, 0, None) == _lib.VAD_EINVAL
        assert fn(A, None, A, 400, 400, A, 160, 160, 4, 1, 0, A, A, A, 0, 0, None) == _lib.VAD_EINVAL
    assert lib.vad_stream_step_tree(None, None, A, 400, 400, 4, A, A, A, A, None) == _lib.VAD_EINVAL
    assert lib.vad_stream_step_tree(A, None, A, 400, 400, 4, A, A, A, A, None) == _lib.VAD_EINVAL
