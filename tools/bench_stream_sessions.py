"""Sessions in the hop kernels, timed: 512 streams, K = 8 and K = 1, FFN and
tree, graph replays, device events on warm clocks, medians over fresh
processes.

    python tools/bench_stream_sessions.py [--out profiles/stream_sessions/bench.json] [--procs 3] [--reps 11]
                                          [--parent-lib libvad_amd_parent.so]

Every figure is measured in a child process of its own (--child), which warms
the device for about half a second per entry, then takes the median of --reps
event-timed runs of 50 replays each; the parent process reports the median
over --procs children and their spread (min, max).  Nothing here is gated.
Per classifier (the golden 39-input FFN; the 977-node tree fixture, LDS walk)
and K, microseconds per replayed step:
  (a) the mechanism
  scored_us            StreamBatch(scores=True): the sibling kernel of this build
  parent_plain_us, parent_scored_us, parent_frozen_us
                       with --parent-lib: the plain, scored and denoising
                       (rows frozen) steps launched through the parent commit's
                       library on this build's plans and buffers
  full_us              sessions, scores=True, every count K, no restart
  frozen_us, full_frozen_us
                       denoise=True with the noise rows frozen: without and with sessions
  (b) idle streams
  uniform_us           counts drawn uniformly from 0..K (mean K / 2)
  half_idle_us         every other stream at count 0, the others at K
  (c) restarts: the flag is consumed, so a fill of ``restart`` precedes every replay
  fill0_us, restart_us             sessions: a fill with 0 (no restart) and with 1
                                   (every stream restarts in every block)
  fill0_denoise_us, restart_denoise_us   the same with denoise=True, noise loaded and rows frozen
A run without a GPU fails: nothing here falls back.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

S, CALLS = 512, 50


def child(reps, parent_lib):
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    from vad_amd import _lib
    from vad_amd.ffn import FFNClassifier
    from vad_amd.stream import StreamBatch
    from vad_amd.tree import TreeClassifier

    def events_us(fn):
        out = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e3 / CALLS)
        return statistics.median(out)

    def timed(fn, seconds=0.5):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            fn()
            torch.cuda.synchronize()
        return events_us(fn)

    w = np.load(os.path.join(REPO, "tests", "golden", "ffn.npz"), allow_pickle=False)
    ffn = FFNClassifier([(w[f"ref39_W{i}"], w[f"ref39_b{i}"]) for i in range(4)])
    tree = TreeClassifier.load(os.path.join(REPO, "tests", "golden", "tree.npz"))
    tree.proba = np.random.default_rng(0).random((tree.feature.shape[0], len(tree.classes_)))  # a score table
    old = ctypes.CDLL(parent_lib) if parent_lib else None
    g = torch.Generator(device="cuda").manual_seed(1)
    noise = (torch.randn((S, 5, 400), device="cuda", generator=g) * 300).round()
    frozen = dict(denoise=True, noise_update=False)
    res = {}
    for name, clf in (("ffn", ffn), ("tree", tree)):
        for K in (8, 1):
            block = (torch.randn((K, S, 160), device="cuda", generator=g) * 3000).round()
            uniform = torch.randint(0, K + 1, (S,), device="cuda", generator=g, dtype=torch.int32)
            half = (torch.arange(S, device="cuda", dtype=torch.int32) % 2) * K
            r = {}

            def run(key, counts=None, fill=None, parent=False, **kw):
                sb = StreamBatch(S, clf, hops_per_step=K, **kw)
                if parent:
                    sb._hop_call(sb.inputs, K, sb.label_block)  # binds the entry and its arguments
                    fn = getattr(old, sb._hop_name)
                    fn.restype, fn.argtypes = _lib.SIGNATURES[sb._hop_name]
                    sb._hop_fn = fn
                if kw.get("denoise"):
                    sb.load_noise(noise)
                sb.inputs.copy_(block)
                if counts is not None:
                    sb.hop_counts.copy_(counts)
                sb.capture()
                step = sb.step if K == 1 else sb.step_block
                if fill is None:
                    r[key] = timed(step)
                else:
                    r[key] = timed(lambda: (sb.restart.fill_(fill), step()))
                    assert not bool(sb.restart.any())  # consumed
                return sb

            run("scored_us", scores=True)
            if old is not None:
                run("parent_plain_us", parent=True)
                run("parent_scored_us", parent=True, scores=True)
                run("parent_frozen_us", parent=True, scores=True, **frozen)
            sb = run("full_us", scores=True, sessions=True)
            assert bool((sb.label_block < 254).all())
            run("frozen_us", scores=True, **frozen)
            run("full_frozen_us", scores=True, sessions=True, **frozen)
            sb = run("uniform_us", counts=uniform, scores=True, sessions=True)
            assert bool((sb.label_block[K - 1][uniform < K] == 254).all())
            run("half_idle_us", counts=half, scores=True, sessions=True)
            run("fill0_us", fill=0, scores=True, sessions=True)
            sb = run("restart_us", fill=1, scores=True, sessions=True)
            assert bool((sb.count == min(K, 5)).all() if K <= 5 else (sb.count >= 5).all())
            run("fill0_denoise_us", fill=0, scores=True, sessions=True, **frozen)
            sb = run("restart_denoise_us", fill=1, scores=True, sessions=True, **frozen)
            assert not bool(sb.noise_count.any()) and not bool(sb._noise.any())  # the loaded rows were cleared
            base = r.get("parent_scored_us", r["scored_us"])
            r["full_added_us"] = r["full_us"] - base
            r["full_frozen_added_us"] = r["full_frozen_us"] - r.get("parent_frozen_us", r["frozen_us"])
            r["restart_added_us"] = r["restart_us"] - r["fill0_us"]
            r["restart_denoise_added_us"] = r["restart_denoise_us"] - r["fill0_denoise_us"]
            res[f"{name}_K{K}_graph"] = r
    print("RESULT " + json.dumps(res), flush=True)


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stream_sessions", "bench.json"))
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.reps, args.parent_lib)
    runs = []
    for _ in range(args.procs):  # one process at a time, each with a device context of its own
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)]
        if args.parent_lib:
            cmd += ["--parent-lib", os.path.abspath(args.parent_lib)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"a child ended with status {p.returncode}")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        runs.append(json.loads(line[7:]))
        print(line, flush=True)
    import torch
    out = {"device": torch.cuda.get_device_name(0), "streams": S, "procs": args.procs, "reps": args.reps,
           "calls_per_rep": CALLS, "parent_library": bool(args.parent_lib)}
    for key in runs[0]:
        out[key] = {f: spread([r[key][f] for r in runs]) for f in runs[0][key]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
