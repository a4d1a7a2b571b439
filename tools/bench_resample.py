"""The resampling kernels, timed with device events on warm clocks; medians
over fresh processes.

    python tools/bench_resample.py [--out profiles/resample/bench.json] [--procs 3] [--reps 11]

Every figure is measured in a child process of its own run (--child), which
warms the device for about half a second, then takes the median of --reps
event-timed calls; the parent reports the median over --procs children and
their spread (min, max).
  clip    one clip of 160M outputs (1M frames' worth): 48 kHz int16 -> fp32 and
          44.1 kHz fp32 -> fp32; microseconds, algorithmic bytes (in + out),
          and the time of a plain torch device copy that moves the same bytes
          (half of them read, half written) on the same box
  batch   256 int16 clips of 3 s at 48 kHz: one resample_clips launch against
          the loop of single-clip calls (host clock, ended by a synchronise)
  stream  512 streams x K = 8 hops, 48 kHz int16: the launch alone, and as a
          node of one replayed graph in front of the StreamBatch hop block,
          against that block's graph alone
A run without a GPU fails: nothing here falls back.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def child(reps):
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    from vad_amd import resample as R
    from vad_amd.ffn import FFNClassifier
    from vad_amd.stream import StreamBatch

    def events_us(fn, n=reps):
        out = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e3)
        return statistics.median(out)

    def host_us(fn, n=reps):
        out = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e6)
        return statistics.median(out)

    def warm(fn, seconds=0.5):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            fn()
            torch.cuda.synchronize()

    res = {}
    n_out = 160 * 1000 * 1000
    for name, rate, dt in (("clip_48k_i16_f32", 48000, torch.int16), ("clip_44k1_f32_f32", 44100, torch.float32)):
        r = R.Resampler(rate)
        n_in = n_out * r.down // r.up
        x = torch.randint(-3000, 3000, (n_in,), device="cuda", dtype=torch.int32).to(dt)
        nbytes = n_in * x.element_size() + n_out * 4
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        warm(lambda: r(x))
        us = events_us(lambda: r(x))
        warm(lambda: dst.copy_(src))
        cp = events_us(lambda: dst.copy_(src))
        res[name] = {"us": us, "bytes": nbytes, "GBps": nbytes / us / 1e3, "copy_us": cp,
                     "copy_GBps": nbytes / cp / 1e3, "share_of_copy": cp / us}
        del x, src, dst
    r = R.Resampler(48000)
    pool = torch.randint(-3000, 3000, (256 * 144000,), device="cuda", dtype=torch.int32).to(torch.int16)
    clips = [pool[i * 144000:(i + 1) * 144000] for i in range(256)]
    warm(lambda: r.batch(clips))
    res["batch_256x3s"] = {"batch_us": host_us(lambda: r.batch(clips)), "loop_us": host_us(lambda: [r(c) for c in clips])}
    res["batch_256x3s"]["speedup"] = res["batch_256x3s"]["loop_us"] / res["batch_256x3s"]["batch_us"]
    del pool, clips
    S, K = 512, 8
    g = np.load(os.path.join(REPO, "tests", "golden", "ffn.npz"), allow_pickle=False)
    sb = StreamBatch(S, FFNClassifier([(g[f"ref39_W{i}"], g[f"ref39_b{i}"]) for i in range(4)]), hops_per_step=K)
    sr = R.StreamResampler(S, 48000, hops_per_step=K, input_dtype=torch.int16, out=sb.inputs)
    sr.inputs.copy_(torch.randint(-3000, 3000, tuple(sr.inputs.shape), device="cuda", dtype=torch.int32))
    warm(lambda: sr.step_block())
    alone = events_us(lambda: sr.step_block(), 51)

    def graph_of(body):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            body()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            body()
        return gr

    hop = graph_of(sb._block_body)
    both = graph_of(lambda: (sr._launch(sr.inputs, sr.out), sb._block_body()))
    warm(hop.replay)
    hop_us = events_us(hop.replay, 51)
    warm(both.replay)
    both_us = events_us(both.replay, 51)
    res["stream_512x8"] = {"alone_us": alone, "hop_block_graph_us": hop_us, "resample_and_hop_block_graph_us": both_us,
                           "added_us": both_us - hop_us}
    print("RESULT " + json.dumps(res), flush=True)


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resample", "bench.json"))
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.reps)
    runs = []
    for _ in range(args.procs):  # one process at a time, each with a device context of its own
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)],
                           capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"a child ended with status {p.returncode}")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        runs.append(json.loads(line[7:]))
        print(line, flush=True)
    import torch
    out = {"device": torch.cuda.get_device_name(0), "procs": args.procs, "reps": args.reps}
    for key in runs[0]:
        out[key] = {f: spread([r[key][f] for r in runs]) for f in runs[0][key]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
