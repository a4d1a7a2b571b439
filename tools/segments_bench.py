"""Timing of the segment stage at the 1M-frame clip size.

For an fp32 and an int16 clip of 1,000,000 frames and synthetic labels at
voiced shares 0.1 / 0.5 / 0.9 (geometric runs, mean 300 active windows, like
speech) and the all-voiced case, three things are timed with device events,
interleaved round by round in one process:

  scan    vad_label_segments (smooth 20 / 10, join, rows, counters)
  gather  vad_gather_segments_* of the rows into a packed buffer
  copy    a plain device-to-device Tensor.copy_ of the same number of bytes

and, for the all-voiced case, the gather from a source that is only 4 / 2
bytes aligned relative to the destination (the clip shifted by one sample).
Every figure is the median over the rounds of (window time / iterations).
The gather's bytes are voiced bytes read plus voiced bytes written.

    python tools/segments_bench.py --out profiles/segments/segments_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # bytes / s, the MI355X specification


def speech_like_labels(n, share, seed, mean_run=300):
    if share >= 1.0:
        return np.ones(n, dtype=np.uint8)
    rng = np.random.default_rng(seed)
    mean_gap = mean_run * (1.0 - share) / share
    out = np.zeros(n, dtype=np.uint8)
    pos, v = 0, 0
    while pos < n:
        l = int(rng.geometric(1.0 / (mean_run if v else mean_gap)))
        out[pos:pos + l] = v
        pos, v = pos + l, 1 - v
    return out


def make_ops(S, lab, seg, total, clip, shifted, out, ns, fs, hop, ws):
    ops = {
        "scan": lambda: S.label_segments(lab, ns, fs, hop, 20, 10, ws=ws, capacity=seg.capacity),
        "gather": lambda: S.voiced_audio(clip, seg, out=out),
        "copy": lambda: out[:total].copy_(clip[:total]),
    }
    if shifted is not None:
        ops["gather_shifted_source"] = lambda: S.voiced_audio(shifted, seg, out=out)
    return ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "segments", "segments_bench.json"))
    args = ap.parse_args()

    import torch
    from vad_amd import segments as S
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no fallback"
    dev = torch.device("cuda", 0)
    fs, hop = 400, 160
    ns = (args.frames - 1) * hop + fs + 1
    n = args.frames - 5
    ws = S.workspace(n, dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3 / args.iters

    cases = []
    for dtype, name in ((torch.float32, "f32"), (torch.int16, "i16")):
        g = torch.Generator(device="cuda").manual_seed(1)
        # one spare sample in front: clip[1:] is the clip at the narrowest relative alignment
        store = torch.empty(ns + 1, dtype=dtype, device=dev)
        if dtype == torch.float32:
            store.normal_(generator=g)
        else:
            store.copy_(torch.randint(-32768, 32768, (ns + 1,), device=dev, generator=g).to(torch.int16))
        clip, shifted = store[:ns], store[1:]
        out = torch.empty(ns, dtype=dtype, device=dev)
        for share in (0.1, 0.5, 0.9, 1.0):
            lab = torch.from_numpy(speech_like_labels(n, share, seed=int(share * 100))).to(dev)
            seg = S.label_segments(lab, ns, fs, hop, 20, 10, ws=ws)
            found, total = (int(x) for x in seg.counts.cpu().tolist())
            ops = make_ops(S, lab, seg, total, clip, shifted if share >= 1.0 else None, out, ns, fs, hop, ws)
            for fn in ops.values():  # warm up every shape
                fn()
            # the gather moved what the model of the rows says (first and last row)
            rows = seg.table[:found].cpu().numpy()
            S.voiced_audio(clip, seg, out=out)
            for s, e, o in (rows[0], rows[-1]):
                assert torch.equal(out[o:o + e - s], clip[s:e])
            cases.append(dict(dtype=name, share=share, segments=found, voiced_samples=total, ops=ops,
                              times={k: [] for k in ops}, bytes=2 * total * clip.element_size()))
        for _ in range(args.rounds):  # interleaved: every op of every case once per round
            for c in cases:
                if c["dtype"] != name:
                    continue
                for k, fn in c["ops"].items():
                    c["times"][k].append(timed(fn))
        del store, out
        for c in cases:
            c.pop("ops", None)
        torch.cuda.empty_cache()

    result = dict(tool="tools/segments_bench.py", device=torch.cuda.get_device_name(0), frames=args.frames,
                  n_samples=ns, n_labels=n, frame_size=fs, hop=hop, max_gap=20, min_run=10, rounds=args.rounds,
                  iters_per_window=args.iters, hbm_peak_bytes_per_s=HBM_PEAK, cases=[])
    for c in cases:
        med = {k: statistics.median(v) for k, v in c["times"].items()}
        row = dict(dtype=c["dtype"], voiced_share=c["share"], segments=c["segments"],
                   voiced_samples=c["voiced_samples"], bytes_read_plus_written=c["bytes"],
                   median_s=med, min_s={k: min(v) for k, v in c["times"].items()},
                   max_s={k: max(v) for k, v in c["times"].items()},
                   gather_over_copy=med["gather"] / med["copy"],
                   gather_bytes_per_s=c["bytes"] / med["gather"], copy_bytes_per_s=c["bytes"] / med["copy"],
                   gather_share_of_hbm_peak=c["bytes"] / med["gather"] / HBM_PEAK)
        if "gather_shifted_source" in med:
            row["gather_shifted_source_over_copy"] = med["gather_shifted_source"] / med["copy"]
        result["cases"].append(row)
        print(f"{row['dtype']} share {row['voiced_share']}: {row['segments']} segments, scan "
              f"{med['scan'] * 1e6:.1f} us, gather {med['gather'] * 1e6:.1f} us, copy {med['copy'] * 1e6:.1f} us, "
              f"gather/copy {row['gather_over_copy']:.3f}, {row['gather_bytes_per_s'] / 1e12:.2f} TB/s "
              f"({100 * row['gather_share_of_hbm_peak']:.0f}% of 8 TB/s)"
              + (f", shifted source/copy {row['gather_shifted_source_over_copy']:.3f}"
                 if "gather_shifted_source_over_copy" in row else ""), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
