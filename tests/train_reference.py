"""The training reference of the trainer tests: torch on the CPU -- the same
forward, F.cross_entropy, autograd and torch.optim.Adadelta(lr, rho, eps) --
in float64 (the reference) or float32 (the yardstick: its deviation from the
float64 run is what a correct fp32 implementation may differ by), and the
seeded synthetic data both run on."""
import numpy as np
import torch
import torch.nn.functional as F


def synth_rows(n, in_dim, classes, seed):
    """Class centres N(0,1) per feature; rows centre[y] + 1.5 N(0,1)."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((classes, in_dim))
    y = rng.integers(0, classes, n).astype(np.uint8)
    x = centres[y] + 1.5 * rng.standard_normal((n, in_dim))
    return x.astype(np.float32), y


def pack(tensors):
    return np.concatenate([t.detach().numpy().astype(np.float64).ravel() for t in tensors])


def torch_train(layers, x, y, order, batch, lr, rho, eps, dtype):
    """Train from ``layers`` over the batches of ``order``; returns the state
    block [params | square_avg | acc_delta] (float64 numpy, W0 b0 W1 b1 ...
    per section) and the per-step losses."""
    params = []
    for w, b in layers:
        params += [torch.tensor(w, dtype=dtype, requires_grad=True), torch.tensor(b, dtype=dtype, requires_grad=True)]
    opt = torch.optim.Adadelta(params, lr=float(lr), rho=float(rho), eps=float(eps))
    xt = torch.tensor(x, dtype=dtype)
    yt = torch.tensor(y.astype(np.int64))
    order = np.asarray(order).reshape(-1, batch)
    losses = []
    for idx in order:
        h = xt[idx]
        for i in range(0, len(params), 2):
            h = h @ params[i] + params[i + 1]
            if i + 2 < len(params):
                h = torch.relu(h)
        loss = F.cross_entropy(h, yt[idx])
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    state = np.concatenate([pack(params), pack([opt.state[p]["square_avg"] for p in params]),
                            pack([opt.state[p]["acc_delta"] for p in params])])
    return state, np.array(losses)


def layers_of(state, dims):
    out, o = [], 0
    for a, b in zip(dims[:-1], dims[1:]):
        w = state[o:o + a * b].reshape(a, b)
        o += a * b
        out.append((w, state[o:o + b]))
        o += b
    return out


def forward(x, layers, dtype):
    """(loss per row given y is applied by the caller) logits in ``dtype``."""
    h = np.asarray(x, dtype)
    for i, (w, b) in enumerate(layers):
        h = h @ np.asarray(w, dtype) + np.asarray(b, dtype)
        if i + 1 < len(layers):
            h = np.where(h < 0, dtype(0), h)
    return h


def row_losses(z, y):
    z = z - z.max(axis=1, keepdims=True)
    lse = np.log(np.exp(z).sum(axis=1))
    return lse - z[np.arange(len(y)), y]
