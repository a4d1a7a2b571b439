"""Clip batches against the per-clip loop they replace, on the same build.

    python tools/clip_batch_bench.py [--out profiles/clip_batch/bench.json] [--reps 7]

Workload: 30, 256 and 2,048 int16 clips of 1 s, 3 s and 10 s at 16 kHz, resident
on the device.  Timed, host clock around work that ends in a device
synchronise, median of --reps after a warm-up of every shape:
  loop     for every clip: pipe.segments(clip)  (pipe.labels + label_segments)
  batch    pipe.segments_batch(batch)           (labels_batch + batch_label_segments)
  pack     ClipBatch.from_device(clips)         (tables H2D + one ragged-copy launch)
and, for the dataset layer, process_files over 30 synthetic wav files of 3 s
against the loop of file_features -> torch.cat -> scale_rows_device ->
format_csv_rows.  The junk-frame share of every batch is recorded.  A run
without a GPU fails: nothing here falls back.
"""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time
import wave

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

RATE = 16000


def timed(fn, reps):
    """Median and spread of fn() in milliseconds, each call ended by a synchronise."""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "clip_batch", "bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--clips", type=int, nargs="*", default=[30, 256, 2048])
    ap.add_argument("--seconds", type=int, nargs="*", default=[1, 3, 10])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    from vad_amd import dataset as D
    from vad_amd.batch import ClipBatch
    from vad_amd.ffn import FFNClassifier
    from vad_amd.pipeline import VadPipeline

    g = np.load(os.path.join(REPO, "tests", "golden", "ffn.npz"), allow_pickle=False)
    pipe = VadPipeline(FFNClassifier([(g[f"ref39_W{i}"], g[f"ref39_b{i}"]) for i in range(4)]))
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rate": RATE, "segments": [], "dataset": None}
    gen = torch.Generator(device="cuda").manual_seed(1)
    for secs in args.seconds:
        for n in args.clips:
            ns = secs * RATE
            pool = torch.randint(-3000, 3000, (n * ns,), generator=gen, device="cuda", dtype=torch.int32).to(torch.int16)
            clips = [pool[i * ns:(i + 1) * ns] for i in range(n)]
            batch = ClipBatch.from_device(clips)

            def loop():
                return [pipe.segments(c, max_gap=3, min_run=5) for c in clips]

            def one():
                return pipe.segments_batch(batch, max_gap=3, min_run=5)

            ref, got = loop(), one()  # warm-up of both shapes, and the results agree
            torch.cuda.synchronize()
            rows = sum(int(s.counts[0].item()) for s in ref[:30])
            assert int(got.clip_row0[min(30, n) - 1].item() + got.clip_rows[min(30, n) - 1].item()) == rows
            r = {"clips": n, "seconds": secs, "junk_frame_share": batch.junk_share,
                 "global_frames": batch.n_frames_global,
                 "loop": timed(loop, args.reps), "batch": timed(one, args.reps),
                 "pack": timed(lambda: ClipBatch.from_device(clips), args.reps)}
            r["speedup_batch_over_loop"] = r["loop"]["median_ms"] / r["batch"]["median_ms"]
            r["speedup_with_pack"] = r["loop"]["median_ms"] / (r["batch"]["median_ms"] + r["pack"]["median_ms"])
            print(json.dumps(r), flush=True)
            res["segments"].append(r)
            del pool, clips, batch, ref, got
    # the dataset layer: 30 wav files of 3 s
    with tempfile.TemporaryDirectory() as d:
        rng = np.random.default_rng(2)
        for i in range(30):
            with wave.open(os.path.join(d, f"f{i:02d}.wav"), "wb") as w:
                w.setnchannels(1), w.setsampwidth(2), w.setframerate(RATE)
                w.writeframes(rng.integers(-3000, 3000, 3 * RATE).astype("<i2").tobytes())
        paths = D.list_audio_files([d])

        def per_file():
            rows = torch.cat([D.file_features(p, device_out=True) for p in paths])
            D.scale_rows_device(rows)
            return D.format_csv_rows(rows.cpu().numpy(), 1)

        def chunk():
            out = io.StringIO()
            D.process_files([d], 1, 30, out)
            return out.getvalue()

        def device_part():  # process_files without reading files and printing text
            clips = [np.ascontiguousarray(D.read_audio(p)[1]) for p in paths]
            return clips

        assert per_file() == chunk()
        host_clips = device_part()

        def batch_device_only():
            b = ClipBatch.from_host(host_clips)
            rows = pipe.features_batch(b, mode=1, packed=True)
            D.scale_rows_device(rows)
            return rows.cpu()

        def loop_device_only():
            rows = torch.cat([D._lib_window_features(pipe.mfcc(torch.from_numpy(c).cuda()), 1) for c in host_clips])
            D.scale_rows_device(rows)
            return rows.cpu()

        batch_device_only(), loop_device_only()
        res["dataset"] = {"files": 30, "seconds": 3,
                          "file_features_loop": timed(per_file, args.reps), "process_files": timed(chunk, args.reps),
                          "loop_without_read_and_text": timed(loop_device_only, args.reps),
                          "batch_without_read_and_text": timed(batch_device_only, args.reps)}
        print(json.dumps(res["dataset"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
