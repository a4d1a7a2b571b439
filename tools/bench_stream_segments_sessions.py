"""The sessions form of the online segmenter, timed: 512 streams, K = 8 and
K = 1, the golden FFN, fp32 samples; the hop step and the segmenter's push
captured as one graph (hop kernel, then push) and replayed, device events on
warm clocks, medians over fresh processes.

    python tools/bench_stream_segments_sessions.py [--out profiles/stream_segments_sessions/bench.json]
                                                   [--procs 3] [--reps 11] [--parent-lib libvad_amd_parent.so]

Every figure is measured in a child process of its own (--child), which warms
the device for about half a second per entry, then takes the median of --reps
event-timed runs of 50 replays each; the parent process reports the median
over --procs children and their spread (min, max).  Nothing here is gated.
Per K, microseconds per replayed block:
  hop_us               the plain hop graph alone (StreamBatch, no segmenter)
  plain_us             plain hop + plain push (StreamBatch.segmenter())
  parent_hop_us, parent_plain_us
                       with --parent-lib: the same two graphs with both kernels
                       launched through the parent commit's library on this
                       build's plans and buffers
  sess_hop_us          the sessions hop graph alone, every count K
  full_us              sessions hop + sessions push, every count K, no restart
  events_us, plain_events_us
                       the same two pushes without audio (events only)
  uniform_us           counts drawn uniformly from 0..K
  fill0_us, restart_us the flag is consumed, so fills of both ``restart`` tensors
                       precede every replay: with 0 (no restart) and with 1
                       (every stream restarts in every block: F flush hops and
                       up to F voiced rows per stream, the end flush's worst case)
and the differences: push_us = plain_us - hop_us, sess_push_us = full_us -
sess_hop_us, full_added_us = sess_push_us - push_us (the parent's push when
--parent-lib is given), restart_added_us = restart_us - fill0_us.
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
SEG = dict(max_gap=2, min_run=3)


class ParentLib:
    """vad_amd._lib as the segmenter sees it, with the segment entries it
    launches taken from the parent commit's library."""

    class Entries:
        def __init__(self, real, old):
            self._real, self._old = real, old

        def __getattr__(self, name):
            if not name.startswith("vad_stream_segments"):
                return getattr(self._real.lib(), name)
            fn = getattr(self._old, name)
            fn.restype, fn.argtypes = self._real.SIGNATURES[name]
            return fn

    def __init__(self, real, old):
        self._real, self._entries = real, ParentLib.Entries(real, old)

    def __getattr__(self, name):
        return getattr(self._real, name)

    def lib(self):
        return self._entries


def child(reps, parent_lib):
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    from vad_amd import _lib, stream_segments
    from vad_amd.ffn import FFNClassifier
    from vad_amd.stream import StreamBatch

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
    old = ctypes.CDLL(parent_lib) if parent_lib else None
    shim = ParentLib(_lib, old)
    g = torch.Generator(device="cuda").manual_seed(1)
    res = {}
    for K in (8, 1):
        # a noise floor with louder stretches, so that both classes occur and segments begin and end
        block = torch.randn((K, S, 160), device="cuda", generator=g) * 300
        block = torch.where(torch.rand((K, S, 1), device="cuda", generator=g) < 0.4, block * 12, block).round()
        uniform = torch.randint(0, K + 1, (S,), device="cuda", generator=g, dtype=torch.int32)
        r = {}

        def run(key, push=True, audio=True, counts=None, fill=None, parent=False, **kw):
            sb = StreamBatch(S, ffn, hops_per_step=K, **kw)
            if parent:
                sb._hop_call(sb.inputs, K, sb.label_block)  # binds the entry and its arguments
                fn = getattr(old, sb._hop_name)
                fn.restype, fn.argtypes = _lib.SIGNATURES[sb._hop_name]
                sb._hop_fn = fn
            seg = sb.segmenter(sessions=sb.sessions, **SEG) if push else None
            sb.inputs.copy_(block)
            if counts is not None:
                sb.hop_counts.copy_(counts)
            step = sb.step if K == 1 else sb.step_block
            stream_segments._lib = shim if parent else _lib

            def body():
                step()
                if seg is not None:
                    seg.push(sb.label_block, sb.inputs if audio else None)

            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                body()  # warm up: code objects loaded before the capture
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            sb.reset()
            if seg is not None:
                seg.reset()
            if counts is not None:  # both resets refill the shared tensor with K
                sb.hop_counts.copy_(counts)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                body()
            stream_segments._lib = _lib
            if fill is None:
                r[key] = timed(graph.replay)
            else:
                r[key] = timed(lambda: (sb.restart.fill_(fill), seg.restart.fill_(fill), graph.replay()))
                assert not bool(sb.restart.any()) and not bool(seg.restart.any())  # consumed
            return sb, seg

        run("hop_us", push=False)
        run("plain_us")
        run("plain_events_us", audio=False)
        if old is not None:
            run("parent_hop_us", push=False, parent=True)
            run("parent_plain_us", parent=True)
        run("sess_hop_us", push=False, sessions=True)
        sb, seg = run("full_us", sessions=True)
        assert not bool(seg.end_len.any())
        run("events_us", audio=False, sessions=True)
        sb, seg = run("uniform_us", counts=uniform, sessions=True)
        assert bool((seg.voiced_len[K - 1][uniform < K] == 0).all())
        run("fill0_us", fill=0, sessions=True)
        sb, seg = run("restart_us", fill=1, sessions=True)
        assert int(seg.state.view(torch.int32)[:, 30].min()) > CALLS  # every replay restarted every stream
        r["push_us"] = r["plain_us"] - r["hop_us"]
        if old is not None:
            r["parent_push_us"] = r["parent_plain_us"] - r["parent_hop_us"]
        r["sess_push_us"] = r["full_us"] - r["sess_hop_us"]
        r["full_added_us"] = r["sess_push_us"] - r.get("parent_push_us", r["push_us"])
        r["restart_added_us"] = r["restart_us"] - r["fill0_us"]
        res[f"ffn_K{K}_graph"] = r
    print("RESULT " + json.dumps(res), flush=True)


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stream_segments_sessions", "bench.json"))
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
           "calls_per_rep": CALLS, "segmenter": SEG, "parent_library": bool(args.parent_lib)}
    for key in runs[0]:
        out[key] = {f: spread([r[key][f] for r in runs]) for f in runs[0][key]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
