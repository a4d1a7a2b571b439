"""Time of the device tree trainer with integer row weights: 1 M rows x 39
features x 3 classes at the reference's parameters (max_depth 25,
min_samples_split 22, min_samples_leaf 20).

One process measures every case once (each the median of --reps calls after a
warm-up, host clock around the C call, which returns when the stream has run
it) and writes a JSON file:

    python tools/tree_train_weights_bench.py --out /tmp/p1.json
    python tools/tree_train_weights_bench.py --lib /path/to/parent/libvad_amd.so --out /tmp/b1.json

With --lib the process loads that library (the parent commit's, built
separately) and measures the unweighted case only: the baseline for
"unchanged".  Three processes of each are then merged, median and min-max over
the processes:

    python tools/tree_train_weights_bench.py --merge /tmp/p1.json /tmp/p2.json /tmp/p3.json \
        --baseline /tmp/b1.json /tmp/b2.json /tmp/b3.json --out profiles/tree_train_weights/bench.json

Cases: "unweighted" (the existing entry), "ones" (the weighted kernels on
weights of all 1: the cost of the gather and of the wider counters),
"bootstrap" (counts of n draws with replacement), "class" (one integer per
class), "forest16" / "forest16_bootstrap" (fit_forest, 16 trees,
max_samples 1.0, sqrt features).  No target is set.  Without a GPU the tool
fails; it has no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

F, K = 39, 3
PARAMS = (25, 22, 20)
WEIGHTED_ENTRIES = ("vad_tree_train_weighted", "vad_tree_train_weighted_workspace_bytes")


def synth(n, seed=0):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((K, F))
    y = rng.integers(0, K, n).astype(np.uint8)
    return (centres[y] + 1.5 * rng.standard_normal((n, F))).astype(np.float32), y


def merge(paths, baseline, out):
    def fold(files):
        runs = [json.load(open(p)) for p in files]
        cases = {}
        for name in runs[0]["cases"]:
            v = [r["cases"][name]["call_ms"] for r in runs]
            cases[name] = {"call_ms_median": float(np.median(v)), "call_ms_min_max": [min(v), max(v)],
                           "call_ms_per_process": v, "nodes": runs[0]["cases"][name]["nodes"],
                           "levels": runs[0]["cases"][name]["levels"]}
        head = {k: runs[0][k] for k in ("rows", "features", "classes", "params", "device", "reps")}
        return head, cases

    head, cases = fold(paths)
    res = dict(head)
    res["timing"] = ("host clock around the C call, which returns when the stream has run it; per process the median "
                     "of reps calls after a warm-up; here the median and min-max over the processes")
    res["processes"] = len(paths)
    res["cases"] = cases
    if baseline:
        _, b = fold(baseline)
        res["parent_library"] = b
    u = cases["unweighted"]["call_ms_median"]
    res["ratios_of_medians"] = {k: cases[k]["call_ms_median"] / u for k in cases if k in ("ones", "bootstrap", "class")}
    if "forest16" in cases:
        res["ratios_of_medians"]["forest16_bootstrap / forest16"] = (cases["forest16_bootstrap"]["call_ms_median"]
                                                                    / cases["forest16"]["call_ms_median"])
    if baseline:
        res["ratios_of_medians"]["unweighted / parent_library"] = u / res["parent_library"]["unweighted"]["call_ms_median"]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trees", type=int, default=16)
    ap.add_argument("--lib", default=None, help="another build of the library: the unweighted case only")
    ap.add_argument("--merge", nargs="+", default=None)
    ap.add_argument("--baseline", nargs="+", default=None)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.baseline, args.out)
    if args.lib:
        os.environ["VAD_AMD_LIB"] = os.path.abspath(args.lib)
    import torch
    if not torch.cuda.is_available():
        sys.exit("tree_train_weights_bench needs the GPU: nothing is timed without one")
    from vad_amd import _lib
    if args.lib:  # an older build does not export the weighted entries
        for name in WEIGHTED_ENTRIES:
            _lib.SIGNATURES.pop(name, None)
    from vad_amd.tree_train import TreeTrainer
    n = args.rows
    x, y = synth(n)
    X = torch.from_numpy(x).cuda()
    tr = TreeTrainer(*PARAMS)
    rng = np.random.default_rng(1)
    boot = np.bincount(rng.integers(0, n, n), minlength=n)
    cls = np.array([1, 3, 7])[y]
    job = (None,) + PARAMS
    res = {"rows": n, "features": F, "classes": K, "params": list(PARAMS), "device": torch.cuda.get_device_name(0),
           "reps": args.reps, "library": _lib.LIB_PATH if args.lib else "this build", "cases": {}}

    def case(name, fn):
        calls = []
        out = None
        for _ in range(args.reps + 1):  # the first is the warm-up
            out = fn()
            calls.append(tr.last_call_seconds * 1e3)
        nodes = int(len(out.feature))
        res["cases"][name] = {"call_ms": float(np.median(calls[1:])), "call_ms_all": calls[1:], "nodes": nodes,
                              "levels": tr.last_levels}
        print(name, res["cases"][name], flush=True)

    case("unweighted", lambda: tr.fit_many(X, y, [job])[0])
    if not args.lib:
        case("ones", lambda: tr.fit_many(X, y, [job + (None, np.ones(n, np.int64))])[0])
        case("bootstrap", lambda: tr.fit_many(X, y, [job + (None, boot)])[0])
        case("class", lambda: tr.fit_many(X, y, [job + (None, cls)])[0])
        case("forest16", lambda: tr.fit_forest(X, y, args.trees, max_samples=1.0, seed=1))
        case("forest16_bootstrap", lambda: tr.fit_forest(X, y, args.trees, max_samples=1.0, seed=1, bootstrap=True))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
