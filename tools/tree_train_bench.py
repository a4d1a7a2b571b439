"""Time of the device tree trainer: 1 M rows x 39 features x 3 classes at the
reference's parameters (max_depth 25, min_samples_split 22, min_samples_leaf 20).

    python tools/tree_train_bench.py [--rows 1000000] [--reps 3] [--out profiles/tree_train/bench.json]

Recorded: milliseconds per fit (host clock around vad_tree_train, which
returns when the stream has run it; the sort of the rows and the whole
TreeTrainer.fit next to it), per level, and bytes per second against two
counts of a level's list traffic for full lists: the 24 bytes per (row,
feature) a level needs at the least (search read, partition read and write)
and the 40 the kernels move (both scans read their lists twice).  Rows of
leaves drop out of the lists, so both rates are upper bounds on what was
moved.  Then the 12-job call of a 3-fold x 4 min_samples_leaf grid against
the same 12 jobs one call each, and sklearn's fit of the same rows on the
host (one thread) as the stand-in for the reference.  No target is set.
Without a GPU the tool fails; it has no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

F, K = 39, 3
PARAMS = (25, 22, 20)


def synth(n, seed=0):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((K, F))
    y = rng.integers(0, K, n).astype(np.uint8)
    return (centres[y] + 1.5 * rng.standard_normal((n, F))).astype(np.float32), y


def timed(fn, reps):
    fn()  # warm-up: this shape, code objects loaded
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tree_train", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tree_train_bench needs the GPU: nothing is timed without one")
    from vad_amd.tree_train import TreeTrainer, kfold
    n = args.rows
    x, y = synth(n)
    X = torch.from_numpy(x).cuda()
    tr = TreeTrainer(*PARAMS)
    calls = []

    def one():
        t = tr.fit(X, y)
        calls.append(tr.last_call_seconds * 1e3)
        return t

    fit_ms, tree = timed(one, args.reps)
    call_ms = float(np.median(calls[1:]))
    levels = tr.last_levels
    sort_ms, _ = timed(lambda: torch.sort(X.t().contiguous(), dim=1, stable=True), args.reps)
    res = {"rows": n, "features": F, "classes": K, "params": list(PARAMS), "device": torch.cuda.get_device_name(0),
           "timing": "host clock around calls that end in a device synchronise; medians of --reps after a warm-up",
           "nodes": int(len(tree.feature)), "levels": levels,
           "fit_ms": float(np.median(fit_ms)), "fit_ms_min_max": [min(fit_ms), max(fit_ms)],
           "vad_tree_train_ms": call_ms, "vad_tree_train_ms_all": calls[1:], "sort_ms": float(np.median(sort_ms)),
           "ms_per_level": call_ms / levels}
    for name, b in (("least_24B", 24), ("moved_40B", 40)):
        res[f"bytes_per_level_full_lists_{name}"] = b * n * F
        res[f"bytes_per_s_upper_bound_{name}"] = b * n * F * levels / (call_ms * 1e-3)
    print(res, flush=True)

    folds = kfold(n, 3)
    jobs = [(trn, 30, 2, msl) for trn, _ in folds for msl in (1, 5, 20, 40)]
    many = []

    def grid_call():
        t = tr.fit_many(X, y, jobs)
        many.append(tr.last_call_seconds * 1e3)
        return t

    timed(grid_call, 1)
    single = []
    for j in jobs:
        tr.fit_many(X, y, [j])
        single.append(tr.last_call_seconds * 1e3)
    res["grid12"] = {"jobs": "3 folds x min_samples_leaf 1, 5, 20, 40; max_depth 30, min_samples_split 2",
                     "one_call_ms": many[-1], "twelve_calls_ms": float(sum(single)), "each_ms": single}
    print(res["grid12"], flush=True)

    if not args.no_sklearn:
        try:
            from sklearn.tree import DecisionTreeClassifier
            t0 = time.perf_counter()
            sk = DecisionTreeClassifier(max_depth=PARAMS[0], min_samples_split=PARAMS[1], min_samples_leaf=PARAMS[2],
                                        random_state=0).fit(x, y)
            res["sklearn_fit_ms"] = (time.perf_counter() - t0) * 1e3
            res["sklearn_nodes"] = int(sk.tree_.node_count)
            res["sklearn_note"] = "DecisionTreeClassifier.fit on the CPU of the GPU host, one thread; a stand-in for the reference"
        except ImportError:
            res["sklearn_fit_ms"] = None
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
