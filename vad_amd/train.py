"""Training the FFN on the device (reference learning/ffn_trainer.py:118-154).

The reference compiles its Keras model with ``optimizer='adadelta'`` and
``loss='categorical_crossentropy'`` and calls ``train_on_batch`` on batches
of 32 feature rows.  One such model is a serial chain of tiny steps; a grid
of them (seeds, folds, optimiser settings: learning/cross_validation.py) is
not.  ``FFNTrainer`` trains ``n_models`` models at once, one workgroup per
model, each model's parameters and Adadelta accumulators resident in LDS for
all the steps of a launch (csrc/train_kernel.hip).

    tr = FFNTrainer(TOPOLOGY_REF39, n_models=64, seed=0)
    hist = tr.fit(X, y, epochs=3, val=(Xv, yv))       # device tensors
    tr.save("ffn.npz", tr.best("val_acc"))            # FFNClassifier.load reads it

There is no CPU path: the steps run in the HIP kernel or raise.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, stream_ptr
from .ffn import TOPOLOGY_REF39, FFNClassifier, save_layers

MAX_STEPS_PER_LAUNCH = 4096  # no single kernel runs long on a shared device


def param_count(dims):
    """Parameters of one model (ValueError for shapes the kernels do not take)."""
    d = (ctypes.c_int32 * len(dims))(*[int(v) for v in dims])
    n = int(lib().vad_ffn_train_param_count(len(dims) - 1, d))
    if n < 0:
        raise ValueError(f"unsupported topology {tuple(dims)}: 1..4 layers, dims 1..64, classes <= 4")
    return n


def glorot_layers(dims, rng):
    """Keras 1 Dense defaults: glorot_uniform weights, zero biases."""
    out = []
    for a, b in zip(dims[:-1], dims[1:]):
        lim = np.sqrt(6.0 / (a + b))
        out.append((rng.uniform(-lim, lim, (a, b)).astype(np.float32), np.zeros(b, np.float32)))
    return out


def pack_layers(layers):
    """[(W, b), ...] -> one section of a state block: W0 row-major, b0, W1, ..."""
    return np.concatenate([np.asarray(v, np.float32).ravel() for w, b in layers for v in (w, b)])


def unpack_layers(section, dims):
    out, o = [], 0
    for a, b in zip(dims[:-1], dims[1:]):
        w = np.array(section[o:o + a * b], np.float32).reshape(a, b)
        o += a * b
        out.append((w, np.array(section[o:o + b], np.float32)))
        o += b
    return out


def _per_model(v, n, name, ok, rule):
    a = np.asarray(v, np.float64)
    if a.ndim == 0:
        a = np.full(n, float(a))
    if a.shape != (n,):
        raise ValueError(f"{name} must be a scalar or {n} values, got shape {a.shape}")
    if not np.all(np.isfinite(a)) or not np.all(ok(a)):
        raise ValueError(f"{name} must be {rule}")
    return a.astype(np.float32)


def fold_orders(n_rows, k, n_models=None, epochs=1, batch_size=32, seed=0, device="cpu"):
    """Training orders and held-out rows of a k-fold run.

    Model m trains on every row outside fold ``m % k`` (folds: a seeded
    permutation of the rows cut into k nearly equal parts).  Returns
    ``(order, held_out)``: ``order`` (n_models, n_steps * batch_size) int32 for
    ``FFNTrainer.steps`` -- per epoch a fresh permutation of the model's
    training rows, cut to whole batches; every model runs the same number of
    steps, that of the smallest training set -- and ``held_out``, per model
    the int64 row indices of its fold.
    """
    n_rows, k, epochs, batch_size = int(n_rows), int(k), int(epochs), int(batch_size)
    n_models = k if n_models is None else int(n_models)
    if k < 2 or k > n_rows or n_models < 1 or epochs < 1 or not 1 <= batch_size <= 64:
        raise ValueError("fold_orders: need 2 <= k <= n_rows, n_models >= 1, epochs >= 1, 1 <= batch_size <= 64")
    rng = np.random.default_rng((int(seed), 0x666F6C64))
    folds = np.array_split(rng.permutation(n_rows), k)
    steps = (n_rows - max(len(f) for f in folds)) // batch_size
    if steps < 1:
        raise ValueError("fold_orders: a training set is smaller than one batch")
    order = np.empty((n_models, epochs * steps * batch_size), np.int32)
    held = []
    for m in range(n_models):
        train = np.concatenate([f for i, f in enumerate(folds) if i != m % k])
        for e in range(epochs):
            order[m, e * steps * batch_size:(e + 1) * steps * batch_size] = rng.permutation(train)[:steps * batch_size]
        held.append(torch.from_numpy(np.sort(folds[m % k]).astype(np.int64)).to(device))
    return torch.from_numpy(order).to(device), held


class FFNTrainer:
    """``n_models`` FFNs of one topology trained side by side with Adadelta."""

    def __init__(self, dims=TOPOLOGY_REF39, n_models=1, seed=0, lr=1.0, rho=0.95, eps=1e-8, batch_size=32,
                 layers=None):
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) < 2:
            raise ValueError("dims needs an input and an output size")
        self.count = param_count(self.dims)
        self.n_models = int(n_models)
        if self.n_models < 1:
            raise ValueError("n_models must be >= 1")
        self.batch_size = int(batch_size)
        if not 1 <= self.batch_size <= 64:
            raise ValueError("batch_size must be 1..64")
        self.hyper = np.stack([
            _per_model(lr, self.n_models, "lr", lambda a: a > 0, "> 0"),
            _per_model(rho, self.n_models, "rho", lambda a: (a >= 0) & (a < 1), "in [0, 1)"),
            _per_model(eps, self.n_models, "eps", lambda a: a > 0, "> 0")], axis=1)
        self.seed = int(seed)
        state = np.zeros((self.n_models, 3 * self.count), np.float32)
        if layers is not None:
            shapes = [(np.shape(w), np.shape(b)) for w, b in layers]
            want = [((a, b), (b,)) for a, b in zip(self.dims[:-1], self.dims[1:])]
            if shapes != want:
                raise ValueError(f"layers do not have the shapes of dims {self.dims}")
            state[:, :self.count] = pack_layers(layers)
        else:
            for m in range(self.n_models):
                state[m, :self.count] = pack_layers(glorot_layers(self.dims, np.random.default_rng((self.seed, m))))
        self._host = state    # the state until the first device call, then stale
        self._state = None    # (n_models, 3 * count) float32 on the device
        self._hyper_dev = None
        self._gen = torch.Generator().manual_seed(self.seed)
        self._labels_ok = None
        self.history = []
        self.last_step_loss = None  # (n_models, steps) losses of the last fit epoch, on the device
        self._dims_c = (ctypes.c_int32 * len(self.dims))(*self.dims)

    # ---- state ----------------------------------------------------------
    def state(self):
        """(n_models, 3 * count) float32 numpy copy: [params | E[g^2] | E[dx^2]]."""
        return self._host.copy() if self._state is None else self._state.cpu().numpy()

    def layers(self, m=0):
        """Model m's [(W, b), ...] as float32 numpy (Keras layout)."""
        m = self._model_index(m)
        row = self._host[m] if self._state is None else self._state[m, :self.count].cpu().numpy()
        return unpack_layers(row[:self.count], self.dims)

    def classifier(self, m=0):
        return FFNClassifier(self.layers(m))

    def save(self, path, m=0):
        """Model m's weights in ffn.save_layers' format (FFNClassifier.load)."""
        save_layers(path, self.layers(m))

    def best(self, metric="val_acc"):
        """Index of the best model of the last ``fit`` epoch: lowest "loss" /
        "val_loss", highest "val_acc"."""
        if metric not in ("loss", "val_loss", "val_acc"):
            raise ValueError("metric must be 'loss', 'val_loss' or 'val_acc'")
        if not self.history or metric not in self.history[-1]:
            raise ValueError(f"no '{metric}' recorded: run fit" + (" with val=" if metric != "loss" else ""))
        v = np.asarray(self.history[-1][metric])
        return int(np.argmax(v) if metric == "val_acc" else np.argmin(v))

    def _model_index(self, m):
        m = int(m)
        if not 0 <= m < self.n_models:
            raise IndexError(f"model {m} of {self.n_models}")
        return m

    def _to_device(self, dev):
        if self._state is None:
            self._state = torch.from_numpy(self._host).to(dev)
            self._hyper_dev = torch.from_numpy(self.hyper).to(dev)
        elif self._state.device != dev:
            raise ValueError(f"the trainer's state is on {self._state.device}, the data on {dev}")

    # ---- argument checks (values first: they hold on any device) ---------
    def _check_rows(self, X, y):
        if not isinstance(X, torch.Tensor) or not isinstance(y, torch.Tensor):
            raise TypeError("X and y must be torch tensors")
        if X.dtype != torch.float32:
            raise TypeError(f"X must be float32, got {X.dtype}")
        if y.dtype != torch.uint8:
            raise TypeError(f"y must be uint8 class indices, got {y.dtype}")
        if X.ndim != 2 or X.shape[1] != self.dims[0]:
            raise ValueError(f"X must be (n_rows, {self.dims[0]}), got {tuple(X.shape)}")
        if y.ndim != 1 or y.shape[0] != X.shape[0]:
            raise ValueError(f"y must be ({X.shape[0]},), got {tuple(y.shape)}")
        if not X.is_contiguous() or not y.is_contiguous():
            raise ValueError("X and y must be contiguous")
        key = (y.data_ptr(), y.shape[0], y._version)
        if self._labels_ok != key:  # once per label tensor, on its device
            if y.numel() and int(y.max()) >= self.dims[-1]:
                raise ValueError(f"labels must be < {self.dims[-1]} classes")
            self._labels_ok = key

    @staticmethod
    def _check_device(X, y):
        if not X.is_cuda or y.device != X.device:
            raise TypeError("X and y must be CUDA (HIP) tensors on one device")

    # ---- training -------------------------------------------------------
    def steps(self, X, y, order, return_loss=True):
        """Run mini-batch steps: ``order`` holds the row indices of consecutive
        batches, (n_steps * batch_size,) for all models or (n_models, n_steps *
        batch_size) per model, int32 on the device.  Returns the per-step losses
        (n_models, n_steps) float32 on the device, or None."""
        if not isinstance(order, torch.Tensor):
            raise TypeError("order must be a torch tensor")
        if order.dtype != torch.int32:
            raise TypeError(f"order must be int32, got {order.dtype}")
        shared = order.ndim == 1
        if order.ndim not in (1, 2) or (not shared and order.shape[0] != self.n_models):
            raise ValueError(f"order must be (n,) or ({self.n_models}, n), got {tuple(order.shape)}")
        total = order.shape[-1]
        if total % self.batch_size:
            raise ValueError(f"order holds {total} indices, not a multiple of batch_size {self.batch_size}")
        if not order.is_contiguous():
            raise ValueError("order must be contiguous")
        if isinstance(X, torch.Tensor) and X.ndim == 2 and total:
            lo, hi = torch.aminmax(order)
            if int(lo) < 0 or int(hi) >= X.shape[0]:
                raise ValueError(f"order indices must lie in [0, {X.shape[0]})")
        self._check_rows(X, y)
        self._check_device(X, y)
        if order.device != X.device:
            raise TypeError("order must be on the device of X")
        self._to_device(X.device)
        n_steps = total // self.batch_size
        loss = torch.empty((self.n_models, n_steps), dtype=torch.float32, device=X.device) if return_loss else None
        if n_steps == 0:
            return loss
        with torch.cuda.device(X.device):
            st = stream_ptr()
            for s0 in range(0, n_steps, MAX_STEPS_PER_LAUNCH):
                ns = min(MAX_STEPS_PER_LAUNCH, n_steps - s0)
                part = (loss if ns == n_steps else
                        torch.empty((self.n_models, ns), dtype=torch.float32, device=X.device)) if return_loss else None
                check(lib().vad_ffn_train_steps(
                    len(self.dims) - 1, self._dims_c, self._state.data_ptr(), self.n_models, X.data_ptr(),
                    y.data_ptr(), X.shape[0], order.data_ptr() + 4 * s0 * self.batch_size,
                    0 if shared else total, self.batch_size, ns, self._hyper_dev.data_ptr(),
                    None if part is None else part.data_ptr(), st), "vad_ffn_train_steps")
                if part is not None and part is not loss:
                    loss[:, s0:s0 + ns] = part
        return loss

    def fit(self, X, y, epochs=1, shuffle=True, val=None):
        """``epochs`` passes over the rows in batches of ``batch_size`` (the rows
        that do not fill a last batch are dropped, as get_batches_num's integer
        division does), every model in its own seeded random order per epoch
        (``shuffle=False``: all in row order).  Returns, per epoch, a dict of
        float64 arrays over the models: "loss" (mean training loss of the epoch)
        and, with ``val=(Xv, yv)``, "val_loss" and "val_acc"."""
        self._check_rows(X, y)
        n = X.shape[0]
        nb = n // self.batch_size
        if nb < 1:
            raise ValueError(f"{n} rows do not fill one batch of {self.batch_size}")
        self._check_device(X, y)
        used = nb * self.batch_size
        out = []
        for _ in range(int(epochs)):
            if shuffle:
                order = torch.stack([torch.randperm(n, generator=self._gen)[:used] for _ in range(self.n_models)])
            else:
                order = torch.arange(used)
            loss = self.steps(X, y, order.to(torch.int32).to(X.device))
            self.last_step_loss = loss
            rec = {"loss": loss.double().mean(dim=1).cpu().numpy()}
            if val is not None:
                rec["val_loss"], rec["val_acc"] = self.evaluate(*val)
            out.append(rec)
            self.history.append(rec)
        return out

    def evaluate(self, X, y):
        """(loss, accuracy) float64 arrays over the models (evaluate_generator)."""
        self._check_rows(X, y)
        n = X.shape[0]
        if n == 0:
            raise ValueError("evaluate needs at least one row")
        self._check_device(X, y)
        self._to_device(X.device)
        nc = int(lib().vad_ffn_train_eval_chunks(n))
        sums = torch.empty((self.n_models, nc), dtype=torch.float32, device=X.device)
        hits = torch.empty((self.n_models, nc), dtype=torch.int32, device=X.device)
        with torch.cuda.device(X.device):
            check(lib().vad_ffn_train_eval(len(self.dims) - 1, self._dims_c, self._state.data_ptr(), self.n_models,
                                           X.data_ptr(), y.data_ptr(), n, sums.data_ptr(), hits.data_ptr(),
                                           stream_ptr()), "vad_ffn_train_eval")
        return (sums.double().sum(dim=1).cpu().numpy() / n, hits.long().sum(dim=1).cpu().numpy() / float(n))
