"""Times of the forest: the window kernel against T launches of the single-tree
window score kernel, and training with feature subsets against plain training.

    python tools/forest_bench.py --out run1.json            # one process, one set of numbers
    python tools/forest_bench.py --collect run1.json run2.json run3.json --out profiles/forest/bench.json

Window kernel (2^20 windows of 13 MFCCs, T = 4 and 16 random trees of 1001
nodes): ``forest_us`` is one vad_features_forest launch (labels and scores);
``trees_sum_us`` is what the library offered before it -- T launches of
TreeClassifier.window_scores on the same rows into T arrays, and the torch adds
and the division that average them; ``single_tree_us`` is one of those
launches.  Device events around ``--reps`` repetitions after a warm-up.

Training (1 M rows x 39 features x 3 classes, max_depth 25, min_samples_split
22, min_samples_leaf 20: the configuration of profiles/tree_train/bench.json):
``train_null_masks_ms`` is vad_tree_train for one tree on all features (the host
clock around the call, which returns when the stream has run it);
``fit_forest16_ms`` the same clock around the one call that trains 16 trees
on "sqrt" feature subsets, and ``fit_forest16_total_ms`` the whole fit_forest.

``--lib PATH`` times another build of the library (an A/B variant, or the
parent commit's, which has no forest entries: ``--parent`` then skips them and
routes training through vad_tree_train).  ``--collect`` writes the medians and
the min / max of the runs it is given.  Without a GPU the tool fails.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NEW = ("vad_tree_train_features", "vad_forest_create", "vad_forest_destroy", "vad_forest_predict",
       "vad_features_forest")
N_WIN = 1 << 20
TREE_NODES = 1001
F, K = 39, 3
PARAMS = (25, 22, 20)


def random_tree(n_nodes, n_features, seed):
    rng = np.random.default_rng(seed)
    feat = np.full(n_nodes, -1, np.int32)
    thr = np.full(n_nodes, -2.0)
    left = np.full(n_nodes, -1, np.int32)
    right = np.full(n_nodes, -1, np.int32)
    stack = [(0, n_nodes)]
    while stack:
        at, size = stack.pop()
        if size == 1:
            continue
        half = (size - 1) // 2  # balanced within a quarter: depths a trained tree of this size has
        ls = 1 + 2 * int(rng.integers(half // 4, half - half // 4 + (half < 2)))
        ls = min(max(ls, 1), size - 2)
        feat[at] = rng.integers(0, n_features)
        thr[at] = rng.normal()
        left[at], right[at] = at + 1, at + 1 + ls
        stack += [(at + 1, ls), (at + 1 + ls, size - 1 - ls)]
    p = rng.random((n_nodes, 2))
    p /= p.sum(axis=1)[:, None]
    return dict(feature=feat, threshold=thr, left=left, right=right, leaf=np.argmax(p, axis=1),
                nan_left=np.zeros(n_nodes, np.uint8), proba=p)


def events_us(torch, fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def run(args):
    if args.lib:
        os.environ["VAD_AMD_LIB"] = os.path.abspath(args.lib)
    import torch
    if not torch.cuda.is_available():
        sys.exit("forest_bench needs the GPU: nothing is timed without one")
    from vad_amd import _lib
    if args.parent:
        for k in NEW:
            _lib.SIGNATURES.pop(k)
        h = _lib.lib()
        h.vad_tree_train_features = lambda *a: h.vad_tree_train(*a[:7], *a[8:])
    from vad_amd.tree import TreeClassifier
    from vad_amd.tree_train import TreeTrainer
    res = {"device": torch.cuda.get_device_name(0), "lib": args.lib or "default", "windows": N_WIN,
           "tree_nodes": TREE_NODES, "reps": args.reps}
    mfcc = torch.randn((N_WIN + 5, 13), device="cuda", generator=torch.Generator("cuda").manual_seed(1)) * 3.0
    for T in (4, 16):
        trees = [TreeClassifier(*(t[k] for k in ("feature", "threshold", "left", "right", "leaf", "nan_left")),
                                np.arange(2), 39, proba=t["proba"])
                 for t in (random_tree(TREE_NODES, 39, 100 + i) for i in range(T))]
        outs = [torch.empty(N_WIN, device="cuda") for _ in range(T)]
        avg = torch.empty(N_WIN, device="cuda")

        def trees_sum():
            for t, o in zip(trees, outs):
                t.window_scores(mfcc, 0, 1, out=o)
            torch.add(outs[0], outs[1], out=avg)
            for o in outs[2:]:
                avg.add_(o)
            avg.div_(T)

        r = {"trees_sum_us": events_us(torch, trees_sum, args.reps),
             "single_tree_us": events_us(torch, lambda: trees[0].window_scores(mfcc, 0, 1, out=outs[0]), args.reps)}
        if not args.parent:
            from vad_amd.forest import ForestClassifier
            forest = ForestClassifier.from_trees(trees)
            lab = torch.empty(N_WIN, dtype=torch.uint8, device="cuda")
            sc = torch.empty(N_WIN, device="cuda")
            r["forest_us"] = events_us(torch, lambda: forest._windows(mfcc, 0, 1, lab, sc, None), args.reps)
            r["ratio_trees_sum_over_forest"] = r["trees_sum_us"] / r["forest_us"]
            trees_sum()
            torch.cuda.synchronize()
            r["max_abs_difference_to_float_average"] = float((avg - sc).abs().max())
        res[f"T{T}"] = r
        print(T, r, flush=True)
    if not args.no_train:
        rng = np.random.default_rng(0)
        centres = rng.standard_normal((K, F))
        y = rng.integers(0, K, args.rows).astype(np.uint8)
        x = (centres[y] + 1.5 * rng.standard_normal((args.rows, F))).astype(np.float32)
        X = torch.from_numpy(x).cuda()
        tr = TreeTrainer(*PARAMS)
        calls = []
        for _ in range(args.train_reps + 1):
            tr.fit(X, y)
            calls.append(tr.last_call_seconds * 1e3)
        res["rows"] = args.rows
        res["train_null_masks_ms"] = float(np.median(calls[1:]))
        res["train_null_masks_ms_all"] = calls[1:]
        if not args.parent:
            tot, call = [], []
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                forest = tr.fit_forest(X, y, 16, max_samples=1.0, max_features="sqrt", seed=0)
                tot.append((time.perf_counter() - t0) * 1e3)
                call.append(tr.last_call_seconds * 1e3)
            res["fit_forest16_ms"] = call[-1]
            res["fit_forest16_total_ms"] = tot[-1]
            res["fit_forest16_nodes"] = int(len(forest.feature))
            res["fit_forest16_levels"] = tr.last_levels
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def collect(args):
    runs = [json.load(open(p)) for p in args.collect]

    def fold(vals):
        if isinstance(vals[0], dict):
            return {k: fold([v[k] for v in vals]) for k in vals[0]}
        if isinstance(vals[0], (int, float)) and not isinstance(vals[0], bool) and len(set(vals)) > 1:
            return {"median": float(np.median(vals)), "min": min(vals), "max": max(vals)}
        return vals[0]

    out = fold(runs)
    out["processes"] = len(runs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--lib")
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--train-reps", type=int, default=3)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--collect", nargs="+")
    args = ap.parse_args()
    collect(args) if args.collect else run(args)


if __name__ == "__main__":
    main()
