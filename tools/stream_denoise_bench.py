"""Live spectral subtraction in the hop kernels, timed: 512 streams, one hop and
blocks of 8, direct launches and graph replays, device events on warm clocks,
medians over fresh processes.

    python tools/stream_denoise_bench.py [--out profiles/stream_denoise/bench.json] [--procs 3] [--reps 11]
                                         [--parent-lib libvad_amd_parent.so]

Every figure is measured in a child process of its own (--child), which warms
the device for about half a second per entry, then takes the median of --reps
event-timed runs of 50 calls each; the parent process reports the median over
--procs children and their spread (min, max).  Nothing here is gated.
Per classifier (the golden 39-input FFN; the 977-node tree fixture, LDS walk)
and per form (K = 1 / K = 8, direct / graph), microseconds per step:
  plain_us          StreamBatch without denoising
  parent_plain_us   with --parent-lib: the same step launched through the
                    parent commit's library (its vad_stream_hops(_tree) on this
                    build's plans and buffers) -- the figure the denoising
                    step is compared against
  frozen_us         denoise=True, five noise frames loaded, noise_update=False:
                    the store of the spectrum row and the subtraction
  update_us         the worst case: a classifier that labels every window
                    noise_class, so every hop of every stream pushes a row and
                    takes the estimate anew
and load_noise_us: load_noise of five frames per stream alone.
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
    layers = [(w[f"ref39_W{i}"], w[f"ref39_b{i}"]) for i in range(4)]
    ffn = FFNClassifier(layers)
    always = [(a.copy(), b.copy()) for a, b in layers]
    always[-1][1][0] = 1e6  # every window is class 0
    ffn_always = FFNClassifier(always)
    tree = TreeClassifier.load(os.path.join(REPO, "tests", "golden", "tree.npz"))
    leaf0 = TreeClassifier.load(os.path.join(REPO, "tests", "golden", "tree.npz"))
    leaf0.leaf = np.zeros_like(leaf0.leaf)  # the same walk, every leaf class 0
    old = ctypes.CDLL(parent_lib) if parent_lib else None
    g = torch.Generator(device="cuda").manual_seed(1)
    noise = (torch.randn((S, 5, 400), device="cuda", generator=g) * 300).round()
    res = {}
    for name, clf, clf_always in (("ffn", ffn, ffn_always), ("tree", tree, leaf0)):
        for K in (1, 8):
            block = (torch.randn((K, S, 160), device="cuda", generator=g) * 3000).round()
            for graph in (False, True):
                r = {}
                for key, c, kw in (("plain_us", clf, {}), ("parent_plain_us", clf, {}),
                                   ("frozen_us", clf, dict(denoise=True, noise_update=False)),
                                   ("update_us", clf_always, dict(denoise=True, noise_class=0))):
                    if key == "parent_plain_us" and old is None:
                        continue
                    sb = StreamBatch(S, c, hops_per_step=K, **kw)
                    if key == "parent_plain_us":
                        sb._hop_call(sb.inputs, K, sb.label_block)  # binds the entry and its arguments
                        fn = getattr(old, sb._hop_name)
                        fn.restype, fn.argtypes = _lib.SIGNATURES[sb._hop_name]
                        sb._hop_fn = fn
                    if kw:
                        sb.load_noise(noise)
                    sb.inputs.copy_(block)
                    if graph:
                        sb.capture()
                    r[key] = timed(sb.step if K == 1 else sb.step_block)
                    if key == "update_us":
                        assert (sb.label_block == 0).all() and (sb.noise_count == 5).all()
                base = r.get("parent_plain_us", r["plain_us"])
                r["frozen_added_us"] = r["frozen_us"] - base
                r["update_added_us"] = r["update_us"] - base
                res[f"{name}_K{K}_{'graph' if graph else 'direct'}"] = r
    sb = StreamBatch(S, ffn, denoise=True)
    res["load_noise"] = {"load_noise_us": timed(lambda: sb.load_noise(noise))}
    print("RESULT " + json.dumps(res), flush=True)


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stream_denoise", "bench.json"))
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
