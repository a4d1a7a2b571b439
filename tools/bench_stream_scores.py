"""The operating point on the live path, timed: 512 streams x 8 hops per block,
device events on warm clocks, medians over fresh processes.

    python tools/bench_stream_scores.py [--out profiles/stream_scores/bench.json] [--procs 3] [--reps 11]
                                        [--parent-lib libvad_amd_parent.so]

Every figure is measured in a child process of its own (--child), which warms
the device for about half a second per entry, then takes the median of --reps
event-timed runs of 50 calls each; the parent process reports the median over
--procs children and their spread (min, max).  Nothing here is gated.
  hop_block   one replayed hop block (StreamBatch.capture, step_block) with
              and without scores, FFN (the golden 39-input network) and tree
              (the 977-node fixture, LDS walk).  With --parent-lib the
              label-only block is also launched through the parent commit's
              library in the same process: its vad_stream_hops(_tree) on this
              build's plans and buffers (the label entries' kernels are the
              parent's instruction for instruction, profiles/stream_scores/isa.md).
  segmenter   one push of a (8, 512) block: the label entry against the _op
              entry on scores 0.0 / 1.0 of the same decisions with on / off =
              0.6 / 0.4, without padding and with pad = (2, 3); fp32 and int16
              audio, max_gap 2, min_run 3.
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

S, K, CALLS = 512, 8, 50


def child(reps, parent_lib):
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    from vad_amd import _lib
    from vad_amd.ffn import FFNClassifier
    from vad_amd.stream import StreamBatch
    from vad_amd.stream_segments import StreamSegmenter
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
    tree.proba = np.random.default_rng(0).random((tree.feature.shape[0], len(tree.classes_)))
    old = ctypes.CDLL(parent_lib) if parent_lib else None
    g = torch.Generator(device="cuda").manual_seed(1)
    block = (torch.randn((K, S, 160), device="cuda", generator=g) * 3000).round()
    res = {}
    for name, clf in (("ffn", ffn), ("tree", tree)):
        r = {}
        for key, kw in (("labels_us", {}), ("scores_us", dict(scores=True)), ("parent_labels_us", {})):
            if key == "parent_labels_us" and old is None:
                continue
            sb = StreamBatch(S, clf, hops_per_step=K, **kw)
            if key == "parent_labels_us":
                sb._hop_call(sb.inputs, K, sb.label_block)  # binds the entry and its arguments
                fn = getattr(old, sb._hop_name)
                fn.restype, fn.argtypes = _lib.SIGNATURES[sb._hop_name]
                sb._hop_fn = fn
            sb.inputs.copy_(block)
            sb.capture()
            r[key] = timed(sb.step_block)
            if kw:
                assert not torch.isnan(sb.score_block).any()
        r["scores_added_us"] = r["scores_us"] - r["labels_us"]
        res["hop_block_" + name] = r
    # the same decisions for every form: speech runs of about 20 hops, as 0 / 1
    # labels and as scores 0.0 / 1.0 (a push of one block, repeated)
    lab = ((torch.arange(K, device="cuda")[:, None] + 7 * torch.arange(S, device="cuda")[None, :]) % 40 < 20)
    lab = lab.to(torch.uint8).contiguous()
    sc = lab.float().contiguous()
    for name, dt in (("f32", torch.float32), ("i16", torch.int16)):
        hops = block.to(dt)
        kw = dict(max_gap=2, min_run=3, hops_per_step=K, audio_dtype=dt)
        a = StreamSegmenter(S, **kw)
        b = StreamSegmenter(S, on=0.6, off=0.4, **kw)
        c = StreamSegmenter(S, on=0.6, off=0.4, pad=(2, 3), **kw)
        r = {"label_push_us": timed(lambda: a.push(lab, hops)), "op_push_nopad_us": timed(lambda: b.push(sc, hops)),
             "op_push_us": timed(lambda: c.push(sc, hops))}
        r["op_added_us"] = r["op_push_us"] - r["label_push_us"]
        res["segmenter_" + name] = r
    print("RESULT " + json.dumps(res), flush=True)


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stream_scores", "bench.json"))
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
    out = {"device": torch.cuda.get_device_name(0), "streams": S, "hops_per_block": K, "procs": args.procs,
           "reps": args.reps, "calls_per_rep": CALLS, "parent_library": bool(args.parent_lib)}
    for key in runs[0]:
        out[key] = {f: spread([r[key][f] for r in runs]) for f in runs[0][key]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
