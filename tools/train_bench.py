"""Step time of the device trainer: 39-64-32-16-3, batch 32, Adadelta.

    python tools/train_bench.py [--steps 8192] [--reps 5] [--out profiles/train/bench.json]

For 1, 64, 256 and 512 models per launch: microseconds per step (device
events around launches of --steps steps, after a warm-up launch of the same
shape; the median of --reps windows, with the spread), and the same per
model.  Next to it the same steps in torch float32 on the CPU, 16 threads --
a stand-in for the reference's Keras train_on_batch loop, which no machine
here runs.  No target is set: the numbers, and the ratio of the 256-model
launch to the 1-model launch (1 = models train side by side for free), are
recorded as measured.  Without a GPU the tool fails; it has no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

DIMS = (39, 64, 32, 16, 3)
BATCH = 32


def synth(n, seed=0):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((DIMS[-1], DIMS[0]))
    y = rng.integers(0, DIMS[-1], n).astype(np.uint8)
    return (centres[y] + 1.5 * rng.standard_normal((n, DIMS[0]))).astype(np.float32), y


def gpu_times(n_models, steps, reps, X, Y):
    from vad_amd.train import FFNTrainer
    tr = FFNTrainer(DIMS, n_models=n_models, batch_size=BATCH)
    g = torch.Generator().manual_seed(n_models)
    order = torch.randint(0, X.shape[0], (n_models, steps * BATCH), generator=g, dtype=torch.int32).cuda()
    tr.steps(X, Y, order, return_loss=False)  # warm-up: this shape, code objects loaded
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tr.steps(X, Y, order, return_loss=False)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / steps)
    return out


def cpu_time(steps, x, y):
    import torch.nn.functional as F
    torch.set_num_threads(16)
    from vad_amd.train import glorot_layers
    params = []
    for w, b in glorot_layers(DIMS, np.random.default_rng(0)):
        params += [torch.tensor(w, requires_grad=True), torch.tensor(b, requires_grad=True)]
    opt = torch.optim.Adadelta(params, lr=1.0, rho=0.95, eps=1e-8)
    xt, yt = torch.from_numpy(x), torch.from_numpy(y.astype(np.int64))
    order = torch.randint(0, len(x), (steps + 16, BATCH))

    def run(rows):
        for idx in rows:
            h = xt[idx]
            for i in range(0, 8, 2):
                h = h @ params[i] + params[i + 1]
                if i < 6:
                    h = torch.relu(h)
            loss = F.cross_entropy(h, yt[idx])
            opt.zero_grad()
            loss.backward()
            opt.step()

    run(order[:16])
    t0 = time.perf_counter()
    run(order[16:])
    return (time.perf_counter() - t0) * 1e6 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-steps", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "train", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("train_bench needs the GPU: nothing is timed without one")
    x, y = synth(65536)
    X, Y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    res = {"dims": list(DIMS), "batch": BATCH, "steps_per_window": args.steps, "windows": args.reps,
           "device": torch.cuda.get_device_name(0), "timing": "device events around the launches of one window",
           "gpu": {}}
    for n in (1, 64, 256, 512):
        t = gpu_times(n, args.steps, args.reps, X, Y)
        res["gpu"][str(n)] = {"us_per_step": float(np.median(t)), "min": min(t), "max": max(t),
                              "us_per_model_step": float(np.median(t)) / n}
        print(n, res["gpu"][str(n)], flush=True)
    res["ratio_256_to_1"] = res["gpu"]["256"]["us_per_step"] / res["gpu"]["1"]["us_per_step"]
    res["ratio_512_to_256"] = res["gpu"]["512"]["us_per_step"] / res["gpu"]["256"]["us_per_step"]
    res["cpu_torch_fp32_16_threads_us_per_step"] = cpu_time(args.cpu_steps, x, y)
    res["cpu_note"] = ("torch float32 autograd + torch.optim.Adadelta, one model, on the CPU of the GPU host; "
                       "a stand-in for the Keras loop, not a measurement of it")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
