"""Time of the hop kernel with the decision tree next to the FFN hop kernel.

    python tools/stream_tree_bench.py [--out profiles/stream_tree/bench.json]

S = 512 streams, K = 1 and K = 8 hops per launch, fp32 samples, one process.
Every classifier is timed in two ways, interleaved over `--repeats` rounds so
that clock drift hits all of them alike, medians reported:
  graph   the captured step replayed `--replays` times on its static input
          block (K = 8: eight different hops, replayed; K = 1: one hop
          replayed, so every window is constant and its Mn features are NaN --
          the fixture tree then walks its NaN path only; the combs below do
          not depend on the audio);
  direct  vad_stream_hops(_tree) launched from Python on a pool of 16
          different blocks read in place (fresh audio; host-bound when the
          kernel is shorter than a launch).
Classifiers:
  ffn            the FFN hop kernel with ref39: the yardstick, the code
                 bench.py's C5 measures
  tree           tests/golden/tree.npz (977 nodes), LDS walk and global walk
  leaf           a one-node table: the kernel with no walk at all
  comb23         a 47-node comb every window walks to depth 23 (the fixture
                 tree's depth): comb23 - leaf = 23 levels, from LDS and from L2
  comb23@max     the same 23 levels in a table of vad_stream_tree_max_lds_nodes
                 nodes (LDS: the block stages all of it, one wave per block)
  comb23@max+1   ... and of one node more (walked from global memory): the step
                 at the boundary
"""
import argparse
import datetime
import json
import os
import socket
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import vad_oracle as O  # noqa: E402
from vad_amd import _lib  # noqa: E402
from vad_amd.ffn import FFNClassifier  # noqa: E402
from vad_amd.stream import StreamBatch  # noqa: E402
from vad_amd.tree import TreeClassifier  # noqa: E402

POOL = 16


def comb(n_nodes, depth):
    """n_nodes nodes, spine node i at 2 i splitting on a first-difference
    feature (13 + i % 13: finite whatever the audio), left child a leaf, right
    child the next spine node; thresholds send every row right until spine
    node depth - 1, which sends every row left: `depth` levels for every
    window.  An even n_nodes gets one unreferenced leaf at the end."""
    D = (n_nodes - 1) // 2
    assert 1 <= depth <= D
    feature = np.full(n_nodes, -1, np.int32)
    thr = np.zeros(n_nodes)
    left = np.full(n_nodes, -1, np.int32)
    right = np.full(n_nodes, -1, np.int32)
    leaf = np.zeros(n_nodes, np.int32)
    sp = 2 * np.arange(D)
    feature[sp] = 13 + np.arange(D) % 13
    left[sp], right[sp] = sp + 1, sp + 2
    thr[sp] = -1e30
    thr[2 * (depth - 1)] = 1e30
    leaf[sp + 1] = np.arange(D) % 2
    return TreeClassifier(feature, thr, left, right, leaf, np.zeros(n_nodes, np.uint8), [0, 1], 39)


def timed_graph(sb, replays, warm):
    for _ in range(warm):
        sb._replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        sb._replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / replays  # us per launch


def timed_direct(sb, pool, replays, warm):
    call = (lambda i: sb._hop_call(pool[i % POOL][0])) if sb.K == 1 else \
        (lambda i: sb._hop_call(pool[i % POOL], sb.K, sb.label_block))
    for i in range(warm):
        call(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(replays):
        call(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / replays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--replays", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stream_tree", "bench.json"))
    args = ap.parse_args()
    S = args.streams
    w = np.load(os.path.join(REPO, "tests", "golden", "ffn.npz"), allow_pickle=False)
    ffn = FFNClassifier([(w[f"ref39_W{i}"], w[f"ref39_b{i}"]) for i in range(4)])
    fixture = TreeClassifier.load(os.path.join(REPO, "tests", "golden", "tree.npz"))
    probe = StreamBatch(1, fixture)
    n_max = int(_lib.lib().vad_stream_tree_max_lds_nodes(probe.plan.handle))
    leaf = TreeClassifier([-1], [0.0], [-1], [-1], [0], [0], [0, 1], 39)
    cases = [("ffn", ffn, "auto"), ("tree_lds", fixture, "auto"), ("tree_global", fixture, "global"),
             ("leaf_lds", leaf, "auto"), ("leaf_global", leaf, "global"),
             ("comb23_lds", comb(47, 23), "auto"), ("comb23_global", comb(47, 23), "global"),
             ("comb23_at_max_lds", comb(n_max, 23), "auto"), ("comb23_at_max_plus_1", comb(n_max + 1, 23), "auto"),
             ("comb23_at_max_forced_global", comb(n_max, 23), "global")]
    res = {"streams": S, "replays": args.replays, "warmup": args.warmup, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "box": socket.gethostname(),
           "date": datetime.date.today().isoformat(), "max_lds_nodes": n_max,
           "fixture_tree_nodes": int(len(fixture.feature)), "us_per_launch": {}}
    for K in (1, 8):
        # fresh audio: POOL blocks of K hops cut from one synthetic clip per stream
        n = 160 * K * POOL
        clips = np.stack([O.synth_clip(n, seed=4000 + s)[:n] for s in range(S)])
        pool = torch.from_numpy(np.ascontiguousarray(clips.reshape(S, POOL, K, 160).transpose(1, 2, 0, 3))).cuda()
        batches = {}
        for name, clf, walk in cases:
            sb = StreamBatch(S, clf, hops_per_step=K, tree_walk=walk)
            sb.inputs.copy_(pool[0])
            for i in range(POOL):  # past every stream's warm-up
                sb._hop_call(pool[i][0]) if K == 1 else sb._hop_call(pool[i], K, sb.label_block)
            sb.capture()
            batches[name] = sb
        runs = {(name, mode): [] for name in batches for mode in ("graph", "direct")}
        for _ in range(args.repeats):
            for name, sb in batches.items():
                runs[name, "graph"].append(timed_graph(sb, args.replays, args.warmup))
                runs[name, "direct"].append(timed_direct(sb, pool, args.replays, args.warmup))
        out = {}
        for mode in ("graph", "direct"):
            med = {name: float(np.median(runs[name, mode])) for name in batches}
            out[mode] = {
                "median": med,
                "runs": {name: runs[name, mode] for name in batches},
                "per_hop_median": {k: v / K for k, v in med.items()},
                "tree_lds_over_ffn": med["tree_lds"] / med["ffn"],
                "tree_global_over_ffn": med["tree_global"] / med["ffn"],
                "walk_23_levels_lds_us_per_hop": (med["comb23_lds"] - med["leaf_lds"]) / K,
                "walk_23_levels_global_us_per_hop": (med["comb23_global"] - med["leaf_global"]) / K,
                "boundary_step_us_per_launch": med["comb23_at_max_plus_1"] - med["comb23_at_max_lds"],
            }
        res["us_per_launch"][f"K={K}"] = out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: {m: {"ffn": v[m]["median"]["ffn"], "tree_lds": v[m]["median"]["tree_lds"],
                              "ratio": v[m]["tree_lds_over_ffn"],
                              "lds23": v[m]["walk_23_levels_lds_us_per_hop"],
                              "global23": v[m]["walk_23_levels_global_us_per_hop"],
                              "boundary": v[m]["boundary_step_us_per_launch"]} for m in v}
                      for k, v in res["us_per_launch"].items()}))


if __name__ == "__main__":
    main()
