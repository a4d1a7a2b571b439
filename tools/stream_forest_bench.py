"""Times of the forest in the hop kernel: a ForestStreamBatch step against the
tree hop step and against what a user could do before it.

    python tools/stream_forest_bench.py --out run1.json            # one process, one set of numbers
    python tools/stream_forest_bench.py --collect run1.json run2.json run3.json --out profiles/stream_forest/bench.json

512 streams, one hop per step (K = 1) and eight (K = 8), each a captured graph
replayed ``--reps`` times between two device events after a warm-up; times are
microseconds per STEP (K hops).  Random trees (tools/forest_bench.py's):
T = 4 and 16 trees of 501 nodes, which stage whole, and 16 of 1001 nodes, of
which a prefix is staged and the rest walked from global memory.

  ``forest_us``        ForestStreamBatch(scores=True).
  ``tree_us``          StreamBatch(scores=True) with the first tree alone.
  ``trees_sum_us``     before this kernel: T tree batches on the same hops (each
                       repeats the whole front end) in one graph, plus the torch
                       adds and the divide that average their score blocks.
  ``ffn_us``           the FFN hop step (ref39 topology, random weights).
  ``lds_trees``, ``block_waves``   what the launch staged and its shape.

``--lib PATH`` times another build of the library: a staging-cap variant
(``python -m vad_amd.build --variant w2 -DVAD_FOREST_STAGE_WAVES=2``: the staged
trees leave room for two waves' scratch; 4 likewise), or the parent commit's,
which has no forest entries -- ``--parent`` then times the tree and FFN steps
only.  ``--collect`` writes the medians and the min / max of the runs it is
given.  Without a GPU the tool fails.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

NEW = ("vad_stream_hops_forest", "vad_stream_hops_forest_i16", "vad_stream_hop_forest_table_bytes",
       "vad_stream_forest_lds_trees")
S = 512
CASES = (("T4_n501", 4, 501), ("T16_n501", 16, 501), ("T16_n1001", 16, 1001))


def replay_us(torch, batches, reps, extra=None):
    """One graph holding a step of every batch (and `extra`), replayed."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())

    def body():
        for b in batches:
            b._body() if b.K == 1 else b._block_body()
        if extra:
            extra()

    with torch.cuda.stream(side):
        body()  # the first launch sets kernel attributes
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    for _ in range(10):
        g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def run(args):
    if args.lib:
        os.environ["VAD_AMD_LIB"] = os.path.abspath(args.lib)
    import torch
    if not torch.cuda.is_available():
        sys.exit("stream_forest_bench needs the GPU: nothing is timed without one")
    from vad_amd import _lib
    if args.parent:
        for k in NEW:
            _lib.SIGNATURES.pop(k)
    from forest_bench import random_tree
    from vad_amd.ffn import FFNClassifier, TOPOLOGY_REF39, random_layers
    from vad_amd.stream import StreamBatch
    from vad_amd.tree import TreeClassifier
    res = {"device": torch.cuda.get_device_name(0), "lib": args.lib or "default", "streams": S, "reps": args.reps}
    gen = torch.Generator("cuda").manual_seed(1)

    def fill(b):
        b.inputs.copy_((torch.randn(b.inputs.shape, device="cuda", generator=gen) * 3000).round())
        return b

    for K in (1, 8):
        r = {"ffn_us": replay_us(torch, [fill(StreamBatch(S, FFNClassifier(random_layers(TOPOLOGY_REF39, seed=3)),
                                                          hops_per_step=K, scores=True))], args.reps)}
        for name, T, n in CASES:
            trees = [TreeClassifier(*(t[k] for k in ("feature", "threshold", "left", "right", "leaf", "nan_left")),
                                    np.arange(2), 39, proba=t["proba"])
                     for t in (random_tree(n, 39, 100 + i) for i in range(T))]
            c = {"tree_us": replay_us(torch, [fill(StreamBatch(S, trees[0], hops_per_step=K, scores=True))],
                                      args.reps)}
            if not args.parent:
                from vad_amd.forest import ForestClassifier
                from vad_amd.stream import ForestStreamBatch
                fb = fill(ForestStreamBatch(S, ForestClassifier.from_trees(trees), hops_per_step=K, scores=True))
                c["forest_us"] = replay_us(torch, [fb], args.reps)
                c["lds_trees"], c["block_waves"] = fb.lds_trees, fb.block_waves
                if not args.no_sum:
                    tb = [fill(StreamBatch(S, t, hops_per_step=K, scores=True)) for t in trees]
                    avg = torch.empty_like(tb[0].score_block)

                    def average():
                        torch.add(tb[0].score_block, tb[1].score_block, out=avg)
                        for b in tb[2:]:
                            avg.add_(b.score_block)
                        avg.div_(T)

                    c["trees_sum_us"] = replay_us(torch, tb, args.reps, average)
                    c["ratio_trees_sum_over_forest"] = c["trees_sum_us"] / c["forest_us"]
                c["ratio_forest_over_tree"] = c["forest_us"] / c["tree_us"]
            r[name] = c
            print(K, name, c, flush=True)
        res[f"K{K}"] = r
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
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--no-sum", action="store_true")
    ap.add_argument("--collect", nargs="+")
    args = ap.parse_args()
    collect(args) if args.collect else run(args)


if __name__ == "__main__":
    main()
