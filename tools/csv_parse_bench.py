"""Dataset CSV import: device chain against the copy that feeds it and against
the host parsers.

Two texts of `--rows` x 40 columns (39 features and a label, "\\r\\n" lines):
  float32   what vad_amd.dataset.format_csv_rows writes (numpy's float32 text)
  repr64    repr(float64) fields, what the reference's csv.writer wrote
Each text is `--unique` generated rows repeated to `--rows` (the parser's work
per row does not depend on whether a row occurred before).  Per text:
  device_ms       count + index + parse (vad_csv_count_lines, the count read
                  back, vad_csv_index, vad_csv_parse) on text already on the
                  device, device events, median of `--reps`
  h2d_ms          the pinned host -> device copy of the same bytes
  end_to_end_ms   read_csv_device(file) -> X, y, host clock ending in a
                  synchronise, file in the page cache
  loadtxt_ms / per_line_ms   np.loadtxt and the reference-shaped loop
                  (csv.reader + np.asarray(line, float32) per line) on the
                  first `--host-rows` rows, scaled to `--rows`
  host_flag_share fields the device left to the host / all fields

    python tools/csv_parse_bench.py [--out profiles/csv_parse/bench.json]

Needs the GPU: there is no fallback.
"""
import argparse
import csv
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vad_amd import _lib  # noqa: E402
from vad_amd.dataset import format_csv_rows, read_csv_device  # noqa: E402


def make_text(kind, unique, rows, seed):
    x = np.random.default_rng(seed).standard_normal((unique, 39))
    if kind == "float32":
        block = format_csv_rows(x.astype(np.float32), 1)
    else:
        block = "".join(",".join(repr(float(v)) for v in r) + ",1.0\r\n" for r in x)
    return (block * -(-rows // unique)).encode("ascii"), block


def device_chain(d, n_cols):
    lib, st = _lib.lib(), _lib.stream_ptr()
    n = d.numel()
    nb = int(lib.vad_csv_workspace_bytes(n))
    ws = torch.empty(nb // 8, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    _lib.check(lib.vad_csv_count_lines(_lib.ptr(d), n, _lib.ptr(count), _lib.ptr(ws), nb, st), "count")
    rows = int(count.item())
    index = torch.empty(rows, dtype=torch.int64, device="cuda")
    X = torch.empty((rows, n_cols - 1), dtype=torch.float32, device="cuda")
    y = torch.empty(rows, dtype=torch.uint8, device="cuda")
    status = torch.empty(rows, dtype=torch.int32, device="cuda")
    _lib.check(lib.vad_csv_index(_lib.ptr(d), n, 0, 0, _lib.ptr(index), rows, _lib.ptr(ws), nb, st), "index")
    _lib.check(lib.vad_csv_parse(_lib.ptr(d), n, _lib.ptr(index), rows, 0, n_cols, None, n_cols - 1, 0, _lib.ptr(X),
                                 _lib.ptr(y), _lib.ptr(status), st), "parse")
    return X, y, status


def timed_events(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--unique", type=int, default=20_000)
    ap.add_argument("--host-rows", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "csv_parse", "bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "csv_parse_bench needs the GPU"
    result = {"rows": args.rows, "cols": 40, "unique_rows": args.unique, "reps": args.reps,
              "device": torch.cuda.get_device_name(0), "texts": {}}
    for kind in ("float32", "repr64"):
        data, block = make_text(kind, args.unique, args.rows, seed=7)
        data = data[:_nth_line_end(data, args.rows)]
        pinned = torch.empty(len(data), dtype=torch.uint8, pin_memory=True)
        pinned.numpy()[:] = np.frombuffer(data, np.uint8)
        d = torch.empty(len(data), dtype=torch.uint8, device="cuda")
        h2d = timed_events(lambda: d.copy_(pinned, non_blocking=True), args.reps + 2)[2:]
        device_chain(d, 40)  # warm-up: code objects, allocator
        dev = timed_events(lambda: device_chain(d, 40), args.reps)
        X, y, status = device_chain(d, 40)
        assert X.shape[0] == args.rows
        flagged_rows = int((status != 0).sum())
        with tempfile.NamedTemporaryFile(suffix=".csv") as f:
            f.write(data)
            f.flush()
            e2e = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                Xe, ye, _ = read_csv_device(f.name, 0)
                torch.cuda.synchronize()
                e2e.append((time.perf_counter() - t0) * 1e3)
        assert Xe.shape == X.shape
        host_text = "".join(block.splitlines(True)[:args.host_rows])
        scale = args.rows / args.host_rows
        t0 = time.perf_counter()
        lt = np.loadtxt(io.StringIO(host_text), delimiter=",", dtype=np.float32)
        t1 = time.perf_counter()
        per = [np.asarray(line, dtype=np.float32) for line in csv.reader(io.StringIO(host_text, newline=""))]
        t2 = time.perf_counter()
        assert np.array_equal(lt[:, :-1], X[:args.host_rows].cpu().numpy(), equal_nan=True)
        assert np.array_equal(np.stack(per)[:, :-1], X[:args.host_rows].cpu().numpy(), equal_nan=True)
        result["texts"][kind] = {
            "bytes": len(data),
            "device_ms": statistics.median(dev), "device_ms_min_max": [min(dev), max(dev)],
            "h2d_ms": statistics.median(h2d), "h2d_gb_per_s": len(data) / statistics.median(h2d) / 1e6,
            "device_gb_per_s": len(data) / statistics.median(dev) / 1e6,
            "end_to_end_ms": statistics.median(e2e), "end_to_end_ms_all": e2e,
            "loadtxt_ms_scaled": (t1 - t0) * 1e3 * scale, "per_line_ms_scaled": (t2 - t1) * 1e3 * scale,
            "host_rows_timed": args.host_rows,
            "host_flagged_rows": flagged_rows,
            # a flagged row has at least one flagged field: an upper bound on the fields' share
            "host_flag_share_rows": flagged_rows / args.rows,
            "device_not_slower_than_h2d": statistics.median(dev) <= statistics.median(h2d),
        }
        print(kind, json.dumps(result["texts"][kind]), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


def _nth_line_end(data, n):
    pos = -1
    view = np.frombuffer(data, np.uint8)
    ends = np.flatnonzero(view == 10)
    pos = int(ends[n - 1]) + 1
    return pos


if __name__ == "__main__":
    main()
