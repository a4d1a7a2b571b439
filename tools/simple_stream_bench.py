"""Time of SimpleStreamBatch next to the single-stream SimpleAnalyser.

    python tools/simple_stream_bench.py [--out profiles/simple_stream/bench.json]

S = 512 streams of 400-sample frames (L = 512), noise_buf_len 5, K = 1 and
K = 8 frames per launch, fp32 and int16 samples, one process.  Every batch is
timed in two ways, interleaved over `--repeats` rounds so that clock drift
hits all of them alike; medians and every run are reported, in us per
launch and per frame-step (one frame of every stream):
  direct  step_block on a pool of 16 different blocks read in place;
  graph   the captured block replayed on its static input.
Beside them:
  features  one vad_simple_features launch over the same K x S frames: the
            design's expectation is a block of about this plus a launch floor;
  host      the figure to beat: S SimpleAnalyser objects, each running
            classify_frames on its K frames (per object an H2D copy, a
            launch, a D2H copy and the state machine in Python), timed with
            a host clock over `--host-blocks` blocks.
"""
import argparse
import datetime
import json
import os
import socket
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import vad_oracle as O  # noqa: E402
from vad_amd import _lib  # noqa: E402
from vad_amd.simple_analyser import SimpleAnalyser  # noqa: E402
from vad_amd.simple_stream import SimpleStreamBatch  # noqa: E402

POOL = 16
RATE, FS, NB = 16000, 400, 5


def events(fn, n, warm):
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n  # us per call


def stats(runs, K):
    med = float(np.median(runs))
    return {"median_us_per_launch": med, "min": float(min(runs)), "max": float(max(runs)), "runs": runs,
            "median_us_per_frame_step": med / K}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--replays", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-blocks", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "simple_stream", "bench.json"))
    args = ap.parse_args()
    S = args.streams
    res = {"streams": S, "frame_size": FS, "noise_buf_len": NB, "replays": args.replays, "warmup": args.warmup,
           "repeats": args.repeats, "host_blocks": args.host_blocks, "device": torch.cuda.get_device_name(0),
           "box": socket.gethostname(), "date": datetime.date.today().isoformat(), "cases": {}}
    lib = _lib.lib()
    for K in (1, 8):
        n = FS * (NB + K * POOL)
        clips = np.stack([O.synth_clip(n, seed=7000 + s)[:n] for s in range(S)])
        init = torch.from_numpy(np.ascontiguousarray(clips[:, :FS * NB].reshape(S, NB, FS))).cuda()
        pool_np = np.ascontiguousarray(clips[:, FS * NB:].reshape(S, POOL, K, FS).transpose(1, 2, 0, 3))
        pool = {torch.float32: torch.from_numpy(pool_np).cuda()}
        pool[torch.int16] = pool[torch.float32].to(torch.int16)
        batches = {}
        for name, dt in (("f32", torch.float32), ("i16", torch.int16)):
            sb = SimpleStreamBatch(S, RATE, FS, NB, frames_per_step=K, input_dtype=dt)
            sb.load_init_inactive_frames(init)
            sb.inputs.copy_(pool[dt][0])
            sb.step_block(pool[dt][0])
            sb.capture()
            batches[name] = (sb, pool[dt])
        flat = pool[torch.float32].reshape(POOL, K * S, FS)
        feat_out = torch.empty((K * S, 7), dtype=torch.float64, device="cuda")

        def features(i):
            _lib.check(lib.vad_simple_features(_lib.ptr(flat[i % POOL]), K * S, FS, FS, 512, 56, 32, 4,
                                               _lib.ptr(feat_out), _lib.stream_ptr()), "vad_simple_features")

        runs = {(name, mode): [] for name in batches for mode in ("direct", "graph")}
        runs["features", "direct"] = []
        for _ in range(args.repeats):
            for name, (sb, p) in batches.items():
                runs[name, "direct"].append(events(lambda i: sb._launch(p[i % POOL], K), args.replays, args.warmup))
                runs[name, "graph"].append(events(
                    lambda i: sb._graph_launch(sb._graph_plan, _lib.stream_ptr()), args.replays, args.warmup))
            runs["features", "direct"].append(events(features, args.replays, args.warmup))
        # the parent's way: one object per stream
        hosts = []
        init_np = init.cpu().numpy()
        for s in range(S):
            sa = SimpleAnalyser(RATE, FS, NB)
            sa.load_init_inactive_frames(list(init_np[s]))
            hosts.append(sa)
        host_runs = []
        for r in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in range(args.host_blocks):
                blk = pool_np[(r * args.host_blocks + b) % POOL]
                for s in range(S):
                    hosts[s].classify_frames(list(blk[:, s]))
            torch.cuda.synchronize()
            host_runs.append((time.perf_counter() - t0) * 1e6 / args.host_blocks)
        out = {f"{name}_{mode}": stats(v, K) for (name, mode), v in runs.items()}
        out["host_objects"] = stats(host_runs, K)
        for k in ("f32_direct", "f32_graph", "i16_direct", "i16_graph"):
            out[k]["host_over_this"] = out["host_objects"]["median_us_per_launch"] / out[k]["median_us_per_launch"]
            out[k]["this_over_features_launch"] = out[k]["median_us_per_launch"] / \
                out["features_direct"]["median_us_per_launch"]
        res["cases"][f"K={K}"] = out
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: {c: round(v[c]["median_us_per_frame_step"], 2) for c in v} for k, v in res["cases"].items()}))


if __name__ == "__main__":
    main()
