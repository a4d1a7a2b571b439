"""C5 end to end with host I/O: serial steps against blocks in flight, fp32
against int16 PCM input.

S = 512 streams, frame 400 / hop 160, the 13-64-64-2 random net of bench.py's
C5 lines, K hops per block for K in {1, 8}.  Per K four variants, every block
from pinned host samples to labels in pinned host memory:
  serial_f32     StreamBatch.step_host, fp32 input (the baseline: the code
                 path bench.py's e2e_host_io_direct lines time)
  serial_i16     step_host, int16 input (half the H2D bytes)
  pipelined_f32  HostPipeline, depth 2, fp32
  pipelined_i16  HostPipeline, depth 2, int16
Every variant is warmed, then the variants run alternately for `--rounds`
rounds in this one process; a timed window is a host-clock interval of at
least `--window` seconds that ends in a device synchronise, and gives one
us-per-hop figure; the median and min-max over the rounds are reported.
latency_us_p50 is the host-clock time from a block's submit (step_host /
submit) until its labels are in host memory (stream synchronise / wait), the
pipelined variants measured in steady state with `depth` blocks in flight (so
a block's latency includes its wait behind the block before it).

    python tools/c5_host_io.py [--out FILE.json] [--depth D]

--depth changes the pipelined variants' blocks in flight (default 2, the
recorded configuration; the JSON says which).

Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vad_amd import ffn as ffn_mod  # noqa: E402
from vad_amd.stream import StreamBatch  # noqa: E402

S, HOP, CARRY = 512, 160, 240
DEPTH = 2  # blocks in flight of the pipelined variants (--depth)


class Variant:
    def __init__(self, name, clf, K, dtype, pipelined):
        self.name, self.K, self.pipelined = name, K, pipelined
        self.sb = StreamBatch(S, clf, kernel="hop", hops_per_step=K, input_dtype=dtype)
        g = torch.Generator().manual_seed(500)
        pcm = (torch.randn((S, CARRY + 8 * K * HOP), generator=g) * 1000).round().clamp(-32768, 32767)
        self.sb.prime(pcm[:, :CARRY].cuda())
        block = pcm[:, CARRY:CARRY + K * HOP].reshape(S, K, HOP).transpose(0, 1).contiguous().to(dtype)
        if pipelined:
            self.pipe = self.sb.host_pipeline(DEPTH)
            for d in range(DEPTH):
                self.pipe.host_inputs[d].copy_(block)
        else:
            self.sb.attach_host_io()
            self.sb.host_inputs.copy_(block)
        self.h2d_bytes = K * S * HOP * (2 if dtype == torch.int16 else 4)
        self.n = 64

    def run(self, n, lat=None):
        """n blocks back to back, then a synchronise; the seconds it took.
        lat: a list that receives each block's submit-to-labels seconds."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if self.pipelined:
            p, t_sub = self.pipe, [0.0] * n
            for b in range(n + DEPTH - 1):
                if b < n:
                    t_sub[b] = time.perf_counter()
                    p.submit(b % DEPTH)
                w = b - (DEPTH - 1)
                if w >= 0:
                    p.wait(w % DEPTH)
                    if lat is not None:
                        lat.append(time.perf_counter() - t_sub[w])
        elif lat is None:
            for _ in range(n):
                self.sb.step_host()
        else:
            cur = torch.cuda.current_stream()
            for _ in range(n):
                t1 = time.perf_counter()
                self.sb.step_host()
                cur.synchronize()
                lat.append(time.perf_counter() - t1)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def window(self, seconds):
        """One timed window of at least `seconds`: us per hop."""
        while True:
            dt = self.run(self.n)
            if dt >= seconds:
                return dt / (self.n * self.K) * 1e6
            self.n = int(self.n * max(1.25, 1.2 * seconds / max(dt, 1e-6))) + 1


def main():
    global DEPTH
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--depth", type=int, default=DEPTH)
    a = ap.parse_args()
    if a.rounds < 5 or a.window < 0.2 or a.depth < 1:
        sys.exit("at least 5 rounds of at least 0.2 s, depth >= 1")
    DEPTH = a.depth
    if not torch.cuda.is_available():
        sys.exit("c5_host_io.py needs the GPU (no fallback)")
    clf = ffn_mod.FFNClassifier(ffn_mod.random_layers(ffn_mod.TOPOLOGY_BL13, seed=3))
    res = {"streams": S, "frame": 400, "hop": HOP, "net": list(ffn_mod.TOPOLOGY_BL13), "depth": DEPTH,
           "rounds": a.rounds, "window_s": a.window, "device": torch.cuda.get_device_name(0), "results": {}}
    for K in (1, 8):
        vs = [Variant("serial_f32", clf, K, torch.float32, False),
              Variant("serial_i16", clf, K, torch.int16, False),
              Variant("pipelined_f32", clf, K, torch.float32, True),
              Variant("pipelined_i16", clf, K, torch.int16, True)]
        for v in vs:  # warm: first launches, allocator, and the window's block count
            v.run(200)
            v.window(a.window)
        us = {v.name: [] for v in vs}
        for _ in range(a.rounds):  # alternately
            for v in vs:
                us[v.name].append(v.window(a.window))
        for v in vs:
            lat = []
            v.run(400, lat)
            x = np.asarray(us[v.name])
            res["results"][f"K{K}_{v.name}"] = {
                "hops_per_block": K, "us_per_hop_median": float(np.median(x)), "us_per_hop_min": float(x.min()),
                "us_per_hop_max": float(x.max()), "us_per_hop_rounds": [float(t) for t in x],
                "stream_frames_per_s_median": S / (float(np.median(x)) * 1e-6),
                "latency_us_p50": float(np.median(np.asarray(lat[len(lat) // 4:])) * 1e6),
                "h2d_bytes_per_block": v.h2d_bytes, "d2h_bytes_per_block": K * S, "blocks_per_window": v.n}
        del vs
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
