"""The sessions stream resampler, timed with device events on warm clocks;
medians over fresh processes.

    python tools/bench_resample_sessions.py [--out profiles/resample_sessions/bench.json]
        [--procs 3] [--reps 51] [--parent-lib vad_amd/lib/libvad_amd_parent.so]

512 streams x K = 8 hops, int16 callers into the fp32 input block of a
StreamBatch, every step a replayed graph.  Each figure is measured in a child
process of its own run (--child) under a time limit of its own, one child
after the other, and the first that fails ends the run; the parent reports the
median over --procs children and their spread (min, max).
  plain_48k         the plain stream kernel at 48 kHz (through --parent-lib too
                    when given: the parent commit's library, built with
                    `python -m vad_amd.build` in a checkout of it)
  one_rate_full     the sessions kernel, 48 kHz alone, all counts K
  three_rates       8 / 44.1 / 48 kHz mixed over the streams, all counts K
  counts_uniform    the three rates, counts uniform in 0 .. K
  hop_block         the sessions hop block's graph alone, with the sessions
                    resampler in front, and what that adds
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
S, K = 512, 8


def child(reps, parent_lib):
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    from vad_amd import _lib
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

    def warm(fn, seconds=0.5):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            fn()
            torch.cuda.synchronize()

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

    def timed(gr):
        warm(gr.replay)
        return events_us(gr.replay)

    gen = torch.Generator(device="cuda").manual_seed(1)
    audio = torch.randint(-3000, 3000, (K, S, 480), device="cuda", dtype=torch.int32, generator=gen).to(torch.int16)
    res = {}
    plain = R.StreamResampler(S, 48000, hops_per_step=K, input_dtype=torch.int16)
    plain.inputs.copy_(audio)
    graphs = {"plain_48k": graph_of(lambda: plain._launch(plain.inputs, plain.out))}
    if parent_lib:  # the same launch through the parent commit's library, loaded beside this one
        old = ctypes.CDLL(parent_lib, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
        for name in ("vad_resample_plan_create", "vad_resample_plan_upload", "vad_resample_stream_i16_f32"):
            getattr(old, name).argtypes = _lib.SIGNATURES[name][1]
        taps = np.ascontiguousarray(plain.spec.taps.astype(np.float32))
        h = ctypes.c_void_p()
        assert old.vad_resample_plan_create(plain.spec.up, plain.spec.down, taps.ctypes.data, len(taps),
                                            ctypes.byref(h)) == 0
        assert old.vad_resample_plan_upload(h) == 0
        state, out = torch.zeros_like(plain.state), torch.zeros_like(plain.out)

        def parent_launch():
            x = plain.inputs
            assert old.vad_resample_stream_i16_f32(h, _lib.ptr(x), x.stride(1), x.stride(0), S, K, 160,
                                                   _lib.ptr(state), _lib.ptr(out), _lib.stream_ptr()) == 0

        graphs["plain_48k_parent_lib"] = graph_of(parent_launch)

    def sessions(rates, uniform_counts):
        rs = R.SessionStreamResampler(S, rates, hops_per_step=K, input_dtype=torch.int16)
        rs.inputs.copy_(audio[:, :, :rs.hop_in])
        rs.rate_index.copy_(torch.arange(S, device="cuda", dtype=torch.int32) % len(rates))
        if uniform_counts:
            rs.hop_counts.copy_(torch.randint(0, K + 1, (S,), device="cuda", dtype=torch.int32, generator=gen))
        rs._launch()  # the flags of a new resampler are set: every stream adopts its rate here
        return rs

    one = sessions([48000], False)
    three = sessions([8000, 44100, 48000], False)
    ragged = sessions([8000, 44100, 48000], True)
    graphs["one_rate_full"] = graph_of(one._launch)
    graphs["three_rates"] = graph_of(three._launch)
    graphs["counts_uniform"] = graph_of(ragged._launch)
    for _ in range(2):  # the cases alternate: each is timed twice, the figures are the means of the two
        for name, gr in graphs.items():
            res.setdefault(name, []).append(timed(gr))
    res = {name: {"us": sum(v) / len(v)} for name, v in res.items()}
    if parent_lib:
        got = torch.zeros_like(plain.out)
        plain.reset(), state.zero_()
        graphs["plain_48k"].replay(), got.copy_(plain.out), graphs["plain_48k_parent_lib"].replay()
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), out.view(torch.int32)), "the two libraries' plain kernels differ"
    g = np.load(os.path.join(REPO, "tests", "golden", "ffn.npz"), allow_pickle=False)
    sb = StreamBatch(S, FFNClassifier([(g[f"ref39_W{i}"], g[f"ref39_b{i}"]) for i in range(4)]), hops_per_step=K,
                     sessions=True)
    rs = sb.resampler([48000], input_dtype=torch.int16)
    rs.inputs.copy_(audio)
    hop = graph_of(sb._block_body)
    both = graph_of(lambda: (rs._launch(), sb._block_body()))
    hop_us, both_us = [], []
    for _ in range(2):
        hop_us.append(timed(hop)), both_us.append(timed(both))
    hop_us, both_us = sum(hop_us) / 2, sum(both_us) / 2
    res["hop_block"] = {"hop_block_graph_us": hop_us, "resample_and_hop_block_graph_us": both_us,
                        "added_us": both_us - hop_us}
    print("RESULT " + json.dumps(res), flush=True)


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resample_sessions", "bench.json"))
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=51)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.reps, args.parent_lib)
    if args.parent_lib and not os.path.exists(args.parent_lib):
        raise SystemExit(f"{args.parent_lib} not found")
    runs = []
    for _ in range(args.procs):  # one process at a time under its own limit; the first that fails ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)]
        if args.parent_lib:
            cmd += ["--parent-lib", os.path.abspath(args.parent_lib)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"a child ended with status {p.returncode}")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        runs.append(json.loads(line[7:]))
        print(line, flush=True)
    import torch
    out = {"device": torch.cuda.get_device_name(0), "streams": S, "hops": K, "procs": args.procs, "reps": args.reps}
    for key in runs[0]:
        out[key] = {f: spread([r[key][f] for r in runs]) for f in runs[0][key]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
