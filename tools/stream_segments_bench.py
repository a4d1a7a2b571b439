"""Time of the streaming segmenter next to the hop kernel it follows.

    python tools/stream_segments_bench.py [--out profiles/stream_segments/bench.json]

S = 512 streams, K = 8 hops per block, int16 and fp32 samples.  Two graphs
per dtype, captured in the same process on the same buffers: the hop block
alone (vad_stream_hops) and the hop block + StreamSegmenter.push.  Each is
replayed `--replays` times after a warm-up, between two events; the labels
are forced half active (the segmenter reads a label block of its own, filled
once, so its copy work does not depend on what the random-weight FFN says).
The yardstick is the hop block's own time in this run.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from vad_amd.ffn import FFNClassifier  # noqa: E402
from vad_amd.stream import StreamBatch  # noqa: E402


def timed(graph, replays, warm):
    for _ in range(warm):
        graph.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / replays  # us per block


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--hops", type=int, default=8)
    ap.add_argument("--replays", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stream_segments", "bench.json"))
    args = ap.parse_args()
    S, K = args.streams, args.hops
    w = np.load(os.path.join(REPO, "tests", "golden", "ffn.npz"), allow_pickle=False)
    clf = FFNClassifier([(w[f"ref39_W{i}"], w[f"ref39_b{i}"]) for i in range(4)])
    rng = np.random.default_rng(0)
    res = {"streams": S, "hops_per_block": K, "replays": args.replays, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "cases": {}}
    for name, dt in (("int16", torch.int16), ("float32", torch.float32)):
        sb = StreamBatch(S, clf, hops_per_step=K, input_dtype=dt)
        pcm = rng.integers(-3000, 3000, size=(K, S, sb.cfg.hop))
        sb.inputs.copy_(torch.from_numpy(pcm.astype(np.int16 if dt == torch.int16 else np.float32)))
        seg = sb.segmenter(max_gap=2, min_run=3)
        # half-active labels in runs of 8 windows, per stream shifted: every block ends and starts segments
        t = np.arange(K)[:, None] + np.arange(S)[None, :]
        half = torch.from_numpy(((t // 4) % 2).astype(np.uint8)).cuda()
        g_hop = capture(lambda: sb.step_block())
        g_both = capture(lambda: (sb.step_block(), seg.push(half, sb.inputs)))
        g_seg = capture(lambda: seg.push(half, sb.inputs))
        g_evt = capture(lambda: seg.push(half))
        runs = {"hop_block": [], "hop_block_plus_segmenter": [], "segmenter_alone": [], "segmenter_events_only": []}
        for _ in range(args.repeats):  # interleaved, so drift hits every form alike
            runs["hop_block"].append(timed(g_hop, args.replays, args.warmup))
            runs["hop_block_plus_segmenter"].append(timed(g_both, args.replays, args.warmup))
            runs["segmenter_alone"].append(timed(g_seg, args.replays, args.warmup))
            runs["segmenter_events_only"].append(timed(g_evt, args.replays, args.warmup))
        med = {k: float(np.median(v)) for k, v in runs.items()}
        added = med["hop_block_plus_segmenter"] - med["hop_block"]
        res["cases"][name] = {
            "us_per_block_median": med, "us_per_block_runs": runs,
            "added_us_per_block": added, "added_over_hop_block": added / med["hop_block"],
            "hop_us_per_hop": med["hop_block"] / K,
            "voiced_fraction_of_rows": float((seg.voiced_len > 0).float().mean().item()),
        }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: {"hop_block_us": v["us_per_block_median"]["hop_block"], "added_us": v["added_us_per_block"],
                          "ratio": v["added_over_hop_block"]} for k, v in res["cases"].items()}))


if __name__ == "__main__":
    main()
