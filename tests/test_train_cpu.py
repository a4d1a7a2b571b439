"""The trainer without a GPU: the four C entries exist everywhere they must,
their argument checks answer before any HIP call, and the Python side's
initialisation, state layout and argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vad_ffn_train_param_count", "vad_ffn_train_steps", "vad_ffn_train_eval_chunks", "vad_ffn_train_eval")
REF39 = (39, 64, 32, 16, 3)
BL13 = (13, 64, 64, 2)


def dims_c(dims):
    return (ctypes.c_int32 * len(dims))(*dims)


def test_symbols_exported_declared_and_mapped():
    from vad_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(REPO, "include", "vad_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
        assert re.search(r"\b" + s + r"\s*\(", header), s
        assert re.search(r"\b" + s + r"\b", doc), s


def test_param_count():
    from vad_amd import _lib
    f = _lib.lib().vad_ffn_train_param_count
    assert f(4, dims_c(REF39)) == 5219
    assert f(3, dims_c(BL13)) == 5186
    assert f(1, dims_c((7, 3))) == 24
    assert f(4, None) == -1
    assert f(0, dims_c((7,))) == -1
    assert f(5, dims_c((8, 8, 8, 8, 8, 2))) == -1
    assert f(2, dims_c((65, 8, 2))) == -1
    assert f(2, dims_c((8, 65, 2))) == -1
    assert f(2, dims_c((8, 8, 5))) == -1
    assert f(2, dims_c((8, 0, 2))) == -1
    assert f(2, dims_c((-1, 8, 2))) == -1


def test_eval_chunks():
    from vad_amd import _lib
    f = _lib.lib().vad_ffn_train_eval_chunks
    assert f(0) == 0
    assert f(1) == 1
    assert f(-1) == -1
    prev = 0
    for n in list(range(0, 5000, 97)) + [10 ** 6, 10 ** 9, 2 ** 40]:
        c = f(n)
        assert c >= prev and c * 1024 >= n > (c - 1) * 1024 or n == 0
        prev = c


def test_c_entries_reject_invalid_arguments():
    """Every VAD_EINVAL case, answered with no GPU present (any non-null
    pointer will do: nothing is dereferenced)."""
    from vad_amd import _lib
    lib = _lib.lib()
    E, OK = _lib.VAD_EINVAL, _lib.VAD_OK
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    d = dims_c(REF39)

    def steps(n_layers=4, dims=d, state=p, n_models=1, x=p, y=p, n_rows=10, order=p, stride=0, batch=32, n_steps=1,
              hyper=p, loss=p):
        return lib.vad_ffn_train_steps(n_layers, dims, state, n_models, x, y, n_rows, order, stride, batch, n_steps,
                                       hyper, loss, None)

    for kw in (dict(state=None), dict(x=None), dict(y=None), dict(order=None), dict(hyper=None), dict(dims=None),
               dict(n_models=-1), dict(n_rows=-1), dict(n_rows=0), dict(n_steps=-1), dict(stride=-1),
               dict(stride=31), dict(n_steps=2, stride=63), dict(batch=0), dict(batch=65), dict(batch=-3),
               dict(n_layers=0), dict(n_layers=5), dict(dims=dims_c((65, 64, 32, 16, 3))),
               dict(dims=dims_c((39, 64, 32, 16, 5))), dict(dims=dims_c((39, 0, 32, 16, 3)))):
        assert steps(**kw) == E, kw
    assert steps(n_models=0) == OK and steps(n_steps=0) == OK  # nothing to do, nothing launched

    def ev(n_layers=4, dims=d, state=p, n_models=1, x=p, y=p, n_rows=10, sums=p, hits=p):
        return lib.vad_ffn_train_eval(n_layers, dims, state, n_models, x, y, n_rows, sums, hits, None)

    for kw in (dict(state=None), dict(x=None), dict(y=None), dict(sums=None), dict(hits=None), dict(dims=None),
               dict(n_models=-1), dict(n_rows=-1), dict(n_layers=0), dict(n_layers=5),
               dict(dims=dims_c((39, 64, 32, 16, 5)))):
        assert ev(**kw) == E, kw
    assert ev(n_rows=0) == OK and ev(n_models=0) == OK


def test_unsupported_lds_budget():
    """A topology whose state and activations pass 160 KiB of LDS is refused
    (before any HIP call); both shipped topologies fit at every batch."""
    from vad_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = dims_c((64, 64, 64, 64, 4))
    assert lib.vad_ffn_train_steps(4, big, p, 1, p, p, 10, p, 0, 64, 1, p, p, None) == _lib.VAD_EUNSUPPORTED


def test_glorot_init_seeds_and_biases():
    from vad_amd.train import FFNTrainer
    tr = FFNTrainer(REF39, n_models=3, seed=5)
    assert tr.count == 5219
    seen = []
    for m in range(3):
        lay = tr.layers(m)
        assert [w.shape for w, _ in lay] == [(39, 64), (64, 32), (32, 16), (16, 3)]
        for (w, b), (a, o) in zip(lay, zip(REF39[:-1], REF39[1:])):
            lim = np.sqrt(6.0 / (a + o))
            assert w.dtype == np.float32 and b.dtype == np.float32
            assert np.abs(w).max() <= lim and np.abs(w).max() > 0.8 * lim
            assert abs(w.mean()) < 0.1 * lim
            assert not b.any()
        seen.append(lay[0][0])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    again = FFNTrainer(REF39, n_models=3, seed=5)
    np.testing.assert_array_equal(again.state(), tr.state())
    assert not np.array_equal(FFNTrainer(REF39, n_models=1, seed=6).state()[0], tr.state()[0])
    st = tr.state()
    assert st.shape == (3, 3 * 5219) and not st[:, 5219:].any()  # fresh accumulators


def test_state_layout_roundtrip():
    from vad_amd.ffn import random_layers
    from vad_amd.train import FFNTrainer, pack_layers, unpack_layers
    lay = random_layers(BL13, seed=2)
    tr = FFNTrainer(BL13, n_models=2, layers=lay)
    st = tr.state()
    o = 0
    for w, b in lay:  # W0 row-major, b0, W1, b1, ...
        np.testing.assert_array_equal(st[1, o:o + w.size], w.ravel())
        o += w.size
        np.testing.assert_array_equal(st[1, o:o + b.size], b)
        o += b.size
    assert o == tr.count == 5186
    for m in range(2):
        for (w, b), (w2, b2) in zip(lay, tr.layers(m)):
            np.testing.assert_array_equal(w, w2)
            np.testing.assert_array_equal(b, b2)
    back = unpack_layers(pack_layers(lay), BL13)
    assert all(np.array_equal(w, w2) and np.array_equal(b, b2) for (w, b), (w2, b2) in zip(lay, back))
    with pytest.raises(ValueError):
        FFNTrainer(REF39, layers=lay)


def test_constructor_rejects_bad_hyper_parameters():
    from vad_amd.train import FFNTrainer
    for kw in (dict(lr=0.0), dict(lr=-1.0), dict(lr=float("nan")), dict(rho=1.0), dict(rho=-0.1), dict(eps=0.0),
               dict(eps=float("inf")), dict(lr=[1.0, 2.0]), dict(batch_size=0), dict(batch_size=65),
               dict(n_models=0), dict(dims=(65, 3)), dict(dims=(8, 5)), dict(dims=(8,))):
        with pytest.raises(ValueError):
            FFNTrainer(**{"dims": (5, 7, 3), "n_models": 3, **kw})
    tr = FFNTrainer((5, 7, 3), n_models=2, lr=[1.0, 0.5], rho=0.9, eps=1e-6)
    np.testing.assert_array_equal(tr.hyper, np.array([[1.0, 0.9, 1e-6], [0.5, 0.9, 1e-6]], np.float32))


def test_python_argument_checks_on_cpu_tensors():
    from vad_amd.train import FFNTrainer
    tr = FFNTrainer((5, 7, 3), n_models=2, batch_size=4)
    X = torch.zeros((16, 5))
    y = torch.zeros(16, dtype=torch.uint8)
    order = torch.arange(16, dtype=torch.int32)
    with pytest.raises(TypeError):  # the right tensors, on the CPU
        tr.steps(X, y, order)
    with pytest.raises(TypeError):
        tr.evaluate(X, y)
    with pytest.raises(TypeError):
        tr.fit(X, y)
    with pytest.raises(TypeError):
        tr.steps(X.double(), y, order)
    with pytest.raises(TypeError):
        tr.steps(X, y.long(), order)
    with pytest.raises(TypeError):
        tr.steps(X, y, order.long())
    with pytest.raises(TypeError):
        tr.steps(X.numpy(), y, order)
    with pytest.raises(ValueError):  # labels >= classes
        tr.steps(X, torch.full((16,), 3, dtype=torch.uint8), order)
    with pytest.raises(ValueError):  # index out of range
        tr.steps(X, y, torch.full((16,), 16, dtype=torch.int32))
    with pytest.raises(ValueError):
        tr.steps(X, y, torch.full((16,), -1, dtype=torch.int32))
    with pytest.raises(ValueError):  # not whole batches
        tr.steps(X, y, order[:6])
    with pytest.raises(ValueError):  # per-model order for another model count
        tr.steps(X, y, order.reshape(1, 16).repeat(3, 1))
    with pytest.raises(ValueError):
        tr.steps(torch.zeros((16, 6)), y, order)
    with pytest.raises(ValueError):
        tr.steps(X, y[:15], order)
    with pytest.raises(ValueError):
        tr.fit(X[:3], y[:3])
    with pytest.raises(ValueError):
        tr.best("val_acc")
    with pytest.raises(IndexError):
        tr.layers(2)


def test_fold_orders():
    from vad_amd.train import fold_orders
    order, held = fold_orders(1000, 5, n_models=10, epochs=2, batch_size=32, seed=3)
    steps = (1000 - 200) // 32
    assert order.shape == (10, 2 * steps * 32) and order.dtype == torch.int32 and len(held) == 10
    assert sorted(torch.cat(held[:5]).tolist()) == list(range(1000))  # the folds partition the rows
    for m in range(10):
        assert torch.equal(held[m], held[m % 5])
        h = set(held[m].tolist())
        o = order[m].tolist()
        assert not h & set(o) and 0 <= min(o) and max(o) < 1000
        for e in range(2):  # a permutation per epoch: no row twice
            ep = o[e * steps * 32:(e + 1) * steps * 32]
            assert len(set(ep)) == len(ep)
    again, _ = fold_orders(1000, 5, n_models=10, epochs=2, batch_size=32, seed=3)
    assert torch.equal(order, again)
    with pytest.raises(ValueError):
        fold_orders(10, 1)
    with pytest.raises(ValueError):
        fold_orders(40, 2, batch_size=32)
