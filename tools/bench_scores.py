"""The score stage on 1M windows, timed with device events on warm clocks;
medians over fresh processes.

    python tools/bench_scores.py [--out profiles/scores/bench.json] [--procs 3] [--reps 11]

Every figure is measured in a child process of its own run (--child), which
warms the device for about half a second per entry, then takes the median of
--reps event-timed calls; the parent reports the median over --procs children
and their spread (min, max).  Nothing here is gated: these are first numbers.
  entries   every new entry alone on N = 2^20 windows, microseconds
  copies    the two elementwise kernels (scores from logits, reference
            labels) and the two histograms against a plain torch device copy
            that moves the same bytes (half read, half written) on the same box
  chain     VadPipeline.segments(on, off, pad, max_gap, min_run) against
            VadPipeline.segments(max_gap, min_run) with the arguments at
            their defaults -- the parent commit's path, line for line -- on
            the same 1M-window clip in the same process
  error     the largest |score - float64 softmax of the kernel's own logits|
            over the two FFN topologies on a 3,000-frame synthetic clip
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

N = 1 << 20


def child(reps):
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    from oracle import vad_oracle as O
    from vad_amd import scores as S
    from vad_amd.batch import ClipBatch
    from vad_amd.ffn import FFNClassifier, TOPOLOGY_BL13, random_layers
    from vad_amd.pipeline import VadPipeline
    from vad_amd.plan import window_logits
    from vad_amd.tree import TreeClassifier

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

    def timed(fn):
        warm(fn)
        return events_us(fn)

    def against_copy(fn, nbytes):
        src = torch.empty(max(nbytes // 2, 1), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        us, cp = timed(fn), timed(lambda: dst.copy_(src))
        return {"us": us, "bytes": nbytes, "GBps": nbytes / us / 1e3, "copy_us": cp, "share_of_copy": cp / us}

    res = {}
    g = torch.Generator(device="cuda").manual_seed(1)
    logits = torch.randn((N, 2), device="cuda", generator=g) * 3
    scores = torch.empty(N, device="cuda")
    res["scores_from_logits"] = against_copy(lambda: S.scores_from_logits(logits, 1, out=scores), 12 * N)
    iv = np.arange(0, (N + 5) * 160, 16000, dtype=np.int64)[:2 * ((N + 5) // 200)].reshape(-1, 2)  # 1 s on, 1 s off
    d_iv = torch.from_numpy(iv).cuda()
    ref = torch.empty(N, dtype=torch.uint8, device="cuda")
    res["reference_labels"] = against_copy(lambda: S.reference_labels(d_iv, N, out=ref), N)
    res["histogram_1024"] = against_copy(lambda: S.histogram(scores, ref, 1024), 5 * N)
    res["histogram_2"] = against_copy(lambda: S.histogram(scores, ref, 2), 5 * N)
    ws = S.workspace(N, scores.device)
    lab, out = torch.empty(N, dtype=torch.uint8, device="cuda"), torch.empty(N, dtype=torch.uint8, device="cuda")
    res["confusion"] = against_copy(lambda: S.confusion(lab, ref, 2), 2 * N)
    res["score_labels"] = {"us": timed(lambda: S.score_labels(scores, 0.7, 0.3, out=lab, ws=ws))}
    res["dilate_labels"] = {"us": timed(lambda: S.dilate_labels(lab, (2, 3), out=out, ws=ws))}
    # a batch of 64 clips of 2^14 windows: the same 1M windows, per clip
    w = N // 64
    b = ClipBatch.from_host([np.zeros((w + 4) * 160 + 401, np.int16)] * 64)
    bs = torch.rand(b.n_windows, device="cuda", generator=g)
    bws = S.workspace(b.n_windows, bs.device)
    bl, bo = (torch.empty(b.n_windows, dtype=torch.uint8, device="cuda") for _ in range(2))
    res["batch_score_labels"] = {"us": timed(lambda: S.batch_score_labels(bs, b, 0.7, 0.3, out=bl, ws=bws))}
    res["batch_dilate_labels"] = {"us": timed(lambda: S.batch_dilate_labels(bl, b, (2, 3), out=bo, ws=bws))}
    del b, bs, bl, bo
    # the fixture tree (977 nodes, walked from LDS) with made-up leaf shares
    tree = TreeClassifier.load(os.path.join(REPO, "tests", "golden", "tree.npz"))
    tree.proba = np.random.default_rng(0).random((tree.feature.shape[0], len(tree.classes_)))
    mfcc = torch.randn((N + 5, 13), device="cuda", generator=g)
    x = torch.randn((N, 39), device="cuda", generator=g)
    ts = torch.empty(N, device="cuda")
    tl = torch.empty(N, dtype=torch.uint8, device="cuda")
    res["tree_window_scores"] = {"us": timed(lambda: S.tree_window_scores(tree, mfcc, out=ts)),
                                 "labels_us": timed(lambda: tree.window_labels(mfcc, out=tl))}
    res["tree_predict_scores"] = {"us": timed(lambda: S.tree_predict_scores(tree, x, out=ts)),
                                  "labels_us": timed(lambda: tree.predict_device(x, out=tl))}
    del mfcc, x
    # the chain on one clip of N windows
    pipe = VadPipeline(FFNClassifier(random_layers(TOPOLOGY_BL13, seed=3)))
    audio = torch.randint(-3000, 3000, ((N + 4) * 160 + 401,), device="cuda", dtype=torch.int32).float()
    assert pipe.n_frames(audio.numel()) - 5 == N
    s = pipe.scores(audio)
    fin = s[torch.isfinite(s)]
    on, off = float(torch.quantile(fin[:1 << 20].double(), 0.7)), float(torch.quantile(fin[:1 << 20].double(), 0.3))
    on, off = float(np.float32(on)), float(np.float32(off))
    res["chain"] = {
        "labels_us": timed(lambda: pipe.labels(audio)),
        "scores_us": timed(lambda: pipe.scores(audio)),
        "segments_default_us": timed(lambda: pipe.segments(audio, max_gap=3, min_run=4)),
        "segments_on_off_pad_us": timed(lambda: pipe.segments(audio, max_gap=3, min_run=4, on=on, off=off,
                                                              pad=(2, 3)))}
    res["chain"]["added_us"] = res["chain"]["segments_on_off_pad_us"] - res["chain"]["segments_default_us"]
    del audio
    # the softmax error the GPU test bounds by 8 * 2^-24
    w39 = np.load(os.path.join(REPO, "tests", "golden", "ffn.npz"), allow_pickle=False)
    nets = {"bl13": pipe, "ref39": VadPipeline(FFNClassifier([(w39[f"ref39_W{i}"], w39[f"ref39_b{i}"])
                                                              for i in range(4)]))}
    n = 160 * 2999 + 401
    clip = torch.from_numpy(O.synth_clip(n, seed=41)[:n].astype(np.float32)).cuda()
    err = {}
    for name, p in nets.items():
        _, z = window_logits(p.ffn.plan, p.mfcc(clip), p.mode)
        zh = z.cpu().numpy().astype(np.float64)
        ok = np.isfinite(zh).all(axis=1)
        e = np.exp(zh[ok] - zh[ok].max(axis=1, keepdims=True))
        worst = 0.0
        for a in range(zh.shape[1]):
            got = S.scores_from_logits(z, a).cpu().numpy().astype(np.float64)[ok]
            worst = max(worst, float(np.abs(got - e[:, a] / e.sum(axis=1)).max()))
        err[name + "_max_abs_err"] = worst
        err[name + "_in_units_of_2^-24"] = worst * 2 ** 24
    res["ffn_softmax_error"] = err
    print("RESULT " + json.dumps(res), flush=True)


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scores", "bench.json"))
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.reps)
    runs = []
    for _ in range(args.procs):  # one process at a time, each with a device context of its own
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)],
                           capture_output=True, text=True, timeout=400)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"a child ended with status {p.returncode}")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        runs.append(json.loads(line[7:]))
        print(line, flush=True)
    import torch
    out = {"device": torch.cuda.get_device_name(0), "windows": N, "procs": args.procs, "reps": args.reps}
    for key in runs[0]:
        out[key] = {f: spread([r[key][f] for r in runs]) for f in runs[0][key]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
