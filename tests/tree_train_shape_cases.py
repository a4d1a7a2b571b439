"""Rows for tests/test_gpu_tree_train_shapes.py, in numpy only: the tie matrix
at 64 columns, the call whose tiles meet as many segments as a tile can, and
the columns of float32 edge values.  The reference stays
tests/tree_train_reference.py; nothing here knows the kernels."""
import numpy as np

import tree_train_reference as R

TILE = 2048  # restates kTile of csrc/tree_train_kernel.hip
N = 2 * TILE + 37

FLT_MAX = np.float32(np.finfo(np.float32).max)
TINY = np.float32(2.0 ** -149)  # the smallest positive subnormal


def model(x, y, K, md, mss, msl, rows=None, feats=None):
    """The reference tree of a job: trained on x[:, feats], features mapped back."""
    if feats is None:
        return R.fit(x, y, K, md, mss, msl, rows=rows)
    feats = np.asarray(feats)
    t = R.fit(np.ascontiguousarray(x[:, feats]), y, K, md, mss, msl, rows=rows)
    t["feature"] = np.where(t["feature"] >= 0, feats[np.maximum(t["feature"], 0)], -1).astype(t["feature"].dtype)
    return t


def model_of_present_classes(x, y, md, mss, msl):
    """The reference tree as TreeTrainer reports it when some class of the
    data set may be missing from y: labels map to indices into the classes
    present, counted in max(2, classes) counters, `value` cut to the classes."""
    classes, idx = np.unique(y, return_inverse=True)
    t = R.fit(x, idx, max(2, len(classes)), md, mss, msl)
    t["value"] = np.ascontiguousarray(t["value"][:, :len(classes)])
    return t


def tie_rows(K, n=N, F=64):
    """The seven columns of test_ties_take_the_lowest_feature_then_position
    (constant, b, a, a, b, a reversed, a), then columns 7..F-1 that repeat
    them in a fixed shuffled pattern: every score ties among the features of a
    chunk and among chunks.  K = 3 as there, or labels over more classes."""
    rng = np.random.default_rng(8)
    y = rng.integers(0, K, n).astype(np.uint8)
    a = ((y == 1) ^ (rng.random(n) < 0.2)).astype(np.float32)
    b = np.round(rng.standard_normal(n) + y).astype(np.float32)
    seven = [np.full(n, 3.0, np.float32), b, a, a, b, a[::-1].copy(), a]
    pattern = np.concatenate([np.arange(7), np.random.default_rng(64).integers(0, 7, F - 7)])
    return np.stack([seven[i] for i in pattern], axis=1), y, pattern


def dense_rows(J=2100):
    """x (n, 2), y and the jobs' rows: job 0 owns rows 0..2, job j >= 1 the next
    two.  Values of four levels and two classes: about half the pairs split."""
    n = 3 + 2 * (J - 1)
    rng = np.random.default_rng(21)
    x = rng.integers(0, 4, (n, 2)).astype(np.float32)
    y = rng.integers(0, 2, n).astype(np.uint8)
    rows = [np.arange(3)] + [np.arange(3 + 2 * (j - 1), 5 + 2 * (j - 1)) for j in range(1, J)]
    return x, y, rows


def segments_meeting_tiles(sizes):
    """Per tile of the level-0 lists (jobs in order, one segment each): how
    many segments meet it, and how many entries its first segment has in it
    when that segment began in the tile before (0: it begins here)."""
    ends = np.cumsum(sizes)
    begins = ends - sizes
    out = []
    for t0 in range(0, int(ends[-1]), TILE):
        meet = np.flatnonzero((begins < t0 + TILE) & (ends > t0))
        first = meet[0]
        out.append((len(meet), int(min(ends[first], t0 + TILE) - t0) if begins[first] < t0 else 0))
    return out


EDGE_COLUMNS = {"zeros": 13, "zeros_subnormal": 14, "subnormals": 15, "flt_max": 16}


def edge_rows(n=N, K=3, seed=5):
    """synth's 13 columns and four of float32 edge values:
    13  -0.0 / +0.0 at random: equal values, no candidate between them;
    14  -0.0 / +0.0, and 2^-149 on most rows of class 1: one candidate;
    15  k * 2^-149, k = 0..7 following the label loosely: all subnormal;
    16  -FLT_MAX, its neighbour towards 0, FLT_MAX's neighbour, FLT_MAX,
        following the label loosely (their midpoints need the double sum)."""
    x13, y = R.synth(n, 13, K, seed)
    rng = np.random.default_rng(seed + 100)
    zero = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    zs = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    zs[(y == 1) ^ (rng.random(n) < 0.15)] = TINY
    k = (2 * y.astype(np.int64) + rng.integers(0, 4, n)) % 8
    sub = (k.astype(np.float64) * 2.0 ** -149).astype(np.float32)
    ends = np.array([-FLT_MAX, np.nextafter(-FLT_MAX, np.float32(0)), np.nextafter(FLT_MAX, np.float32(0)), FLT_MAX],
                    np.float32)
    big = ends[(y.astype(np.int64) + rng.integers(0, 3, n)) % 4]
    x = np.concatenate([x13, np.stack([zero, zs, sub, big], axis=1)], axis=1)
    return np.ascontiguousarray(x, np.float32), y
