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

    python tools/simple_stream_bench.py --sessions --parent-lib PATH \
        [--out profiles/simple_stream_sessions/bench.json]

The sessions kernels next to the plain ones, as replayed graphs, same shapes.
PATH is libvad_amd.so built from the parent commit (the plain kernels as they
were).  Each of `--processes` rounds starts one fresh process per line, so
every line is timed under the same conditions (a process that has captured
only its own graphs); medians over the processes are reported with min-max,
every line also as a ratio to the parent's plain kernel:
  parent_plain     the plain kernel through the parent's library
  plain            the plain kernel through this build
  sessions_full    the sessions kernel, every count K, init_left 0
  sessions_ragged  counts uniform in 0..K (seeded), the streams initialised
  sessions_restart every stream restarting in every block; the kernel
                   consumes the flags, so this graph has a second node, the
                   one-kernel fill that sets them again
"""
import argparse
import datetime
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import vad_oracle as O  # noqa: E402
from vad_amd import _lib  # noqa: E402

if "--sessions-child=parent_plain" in sys.argv:  # the parent commit's library has no sessions entries to bind
    for _name in [n for n in _lib.SIGNATURES if n.startswith("vad_simple_stream_") and "_sessions" in n]:
        del _lib.SIGNATURES[_name]

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


SESSION_LINES = ("parent_plain", "plain", "sessions_full", "sessions_ragged", "sessions_restart")


def sessions_child(line, args):
    """One process of the sessions comparison: graph-replay time of one line,
    K = 1 and 8, fp32 and int16, in us per launch, as one JSON line on stdout."""
    S, out = args.streams, {}
    for K in (1, 8):
        n = FS * (NB + K)
        clips = np.stack([O.synth_clip(n, seed=7000 + s)[:n] for s in range(S)])
        init = torch.from_numpy(np.ascontiguousarray(clips[:, :FS * NB].reshape(S, NB, FS))).cuda()
        blk = torch.from_numpy(np.ascontiguousarray(clips[:, FS * NB:].reshape(S, K, FS).transpose(1, 0, 2))).cuda()
        ragged = torch.from_numpy(np.random.RandomState(11).randint(0, K + 1, size=S).astype(np.int32)).cuda()
        counts = ragged if line == "sessions_ragged" else None
        batches = []
        for name, dt in (("f32", torch.float32), ("i16", torch.int16)):
            kw = dict(sessions=True) if line.startswith("sessions") else {}
            sb = SimpleStreamBatch(S, RATE, FS, NB, frames_per_step=K, input_dtype=dt, **kw)
            sb.load_init_inactive_frames(init)
            sb.inputs.copy_(blk.to(dt))
            if counts is not None:
                sb.frame_counts.copy_(counts)
            if line == "sessions_restart":
                body = sb._block_body

                def with_flags(sb=sb, body=body):
                    sb.restart.fill_(1)
                    body()
                sb._block_body = with_flags
            sb.capture()
            batches.append((f"K={K}/{name}/{line}", sb))
        runs = {key: [] for key, _ in batches}
        for _ in range(args.repeats):  # interleaved, so that clock drift hits both dtypes alike
            for key, sb in batches:
                runs[key].append(events(lambda i: sb._graph_launch(sb._graph_plan, _lib.stream_ptr()), args.replays,
                                        args.warmup))
        for key, v in runs.items():
            out[key] = float(np.median(v))
    print("SESSIONS_CHILD " + json.dumps(out), flush=True)


def sessions_main(args):
    """A fresh process per line and round, one at a time; this process never opens the GPU."""
    per = {}
    for p in range(args.processes):
        for which in SESSION_LINES:
            env = dict(os.environ)
            if which == "parent_plain":
                env["VAD_AMD_LIB"] = os.path.abspath(args.parent_lib)
            else:
                env.pop("VAD_AMD_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), f"--sessions-child={which}", "--streams",
                   str(args.streams), "--replays", str(args.replays), "--warmup", str(args.warmup), "--repeats",
                   str(args.repeats)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"child {which} failed with {r.returncode}")  # nothing more is started
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("SESSIONS_CHILD ")][-1]
            for key, v in json.loads(line[len("SESSIONS_CHILD "):]).items():
                per.setdefault(key, []).append(v)
    res = {"streams": args.streams, "frame_size": FS, "noise_buf_len": NB, "replays": args.replays,
           "warmup": args.warmup, "repeats_per_process": args.repeats, "processes": args.processes,
           "box": socket.gethostname(), "date": datetime.date.today().isoformat(), "mode": "graph replay",
           "unit": "us per launch", "lines": {}}
    for key, v in sorted(per.items()):
        K, name, _ = key.split("/")
        base = float(np.median(per[f"{K}/{name}/parent_plain"]))
        res["lines"][key] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "processes": v,
                             "over_parent_plain": float(np.median(v)) / base}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: [round(v["median"], 2), round(v["min"], 2), round(v["max"], 2),
                          round(v["over_parent_plain"], 3)] for k, v in res["lines"].items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", action="store_true", help="the sessions kernels next to the plain ones")
    ap.add_argument("--sessions-child", choices=SESSION_LINES, help=argparse.SUPPRESS)
    ap.add_argument("--parent-lib", help="libvad_amd.so built from the parent commit (--sessions)")
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--replays", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-blocks", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.sessions_child:
        return sessions_child(args.sessions_child, args)
    if args.sessions:
        if not args.parent_lib or not os.path.exists(args.parent_lib):
            ap.error("--sessions needs --parent-lib, a libvad_amd.so built from the parent commit")
        args.out = args.out or os.path.join(REPO, "profiles", "simple_stream_sessions", "bench.json")
        return sessions_main(args)
    args.out = args.out or os.path.join(REPO, "profiles", "simple_stream", "bench.json")
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
