"""FFNTrainer on the device against torch on the CPU (tests/train_reference.py).

Reference: the same steps in float64.  Yardstick: the same torch code in
float32; e32 = its max-abs deviation from the float64 run, per section of the
state (parameters, E[g^2], E[dx^2]) over the models of a case.  The kernel's
fp32 arithmetic sums in another order, so it may differ from the reference by
a small multiple of what torch's own fp32 does: C = 4.

Measured on an MI355X: the worst ratio error / e32 over all the parity cases
is 1.56 (E[g^2] and E[dx^2] of 13-64-64-2 at batch 20); parameters reach
1.28 (39-64-32-16-3, batch 64), step losses 1.44 (the 512-step case).
"""
import ctypes
import os

import numpy as np
import pytest

from oracle import vad_oracle as O
import train_reference as R

pytestmark = pytest.mark.gpu

C = 4.0
REF39 = (39, 64, 32, 16, 3)
BL13 = (13, 64, 64, 2)
HYPER = dict(lr=[1.0, 0.5, 2.0], rho=[0.95, 0.9, 0.99], eps=[1e-8, 1e-6, 1e-7])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def dev(torch, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def run_case(torch, dims, batch, n_steps, n_rows=600, seed=11):
    """3 models (own seeds and hyper-parameters, own orders) for n_steps on
    the device and in torch float64 / float32.  Returns the worst ratios."""
    from vad_amd.train import FFNTrainer
    x, y = R.synth_rows(n_rows, dims[0], dims[-1], seed)
    rng = np.random.default_rng(seed + 1)
    order = np.stack([np.concatenate([rng.permutation(n_rows) for _ in range(-(-n_steps * batch // n_rows))])
                      [:n_steps * batch] for _ in range(3)]).astype(np.int32)
    tr = FFNTrainer(dims, n_models=3, seed=seed, batch_size=batch, **HYPER)
    start = [tr.layers(m) for m in range(3)]
    loss = tr.steps(dev(torch, x), dev(torch, y), dev(torch, order)).cpu().numpy().astype(np.float64)
    got = tr.state().astype(np.float64)
    n = tr.count
    e32 = np.zeros(3)
    err = np.zeros(3)
    e32_loss = err_loss = 0.0
    for m in range(3):
        lr, rho, eps = (float(v) for v in tr.hyper[m])
        s64, l64 = R.torch_train(start[m], x, y, order[m], batch, lr, rho, eps, torch.float64)
        s32, l32 = R.torch_train(start[m], x, y, order[m], batch, lr, rho, eps, torch.float32)
        for s in range(3):
            sec = slice(s * n, (s + 1) * n)
            e32[s] = max(e32[s], np.abs(s32[sec] - s64[sec]).max())
            err[s] = max(err[s], np.abs(got[m, sec] - s64[sec]).max())
        e32_loss = max(e32_loss, np.abs(l32 - l64).max())
        err_loss = max(err_loss, np.abs(loss[m] - l64).max())
    ratios = list(err / e32) + [err_loss / e32_loss]
    print(f"train parity {dims} batch {batch} steps {n_steps}: e32 {e32} err {err} "
          f"loss e32 {e32_loss:.3g} err {err_loss:.3g} ratios {np.round(ratios, 3)}")
    return ratios


@pytest.mark.parametrize("batch", [32, 20, 64])
@pytest.mark.parametrize("dims", [REF39, BL13, (5, 7, 3), (7, 3)])
def test_parity_64_steps(torch_cuda, dims, batch):
    """Parameters, both accumulators and every step's loss within C x the
    float32 torch run's own error of the float64 reference."""
    ratios = run_case(torch_cuda, dims, batch, 64)
    assert max(ratios) <= C, ratios


def test_parity_512_steps(torch_cuda):
    ratios = run_case(torch_cuda, REF39, 32, 512, n_rows=2000)
    assert max(ratios) <= C, ratios


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _train(torch, n_models, at, x, y, order, n_steps=64, split=None, shared=False, lr=1.0, before=None):
    """Model `at` of n_models: the layers of seed 3, the given lr, its own
    order; the others run other rates and orders.  Returns its state, losses."""
    from vad_amd.train import FFNTrainer, glorot_layers
    lay = glorot_layers(REF39, np.random.default_rng(3))
    lrs = [0.3 + 0.01 * i for i in range(n_models)]
    lrs[at] = lr
    tr = FFNTrainer(REF39, n_models=n_models, lr=lrs, layers=lay)
    if shared:
        od = dev(torch, order)
    else:
        rng = np.random.default_rng(99)
        full = rng.integers(0, len(x), (n_models, order.size)).astype(np.int32)
        full[at] = order
        od = dev(torch, full)
    X, Y = dev(torch, x), dev(torch, y)
    losses = []
    for part in (split or [n_steps]):
        if before is not None:
            before()
        o = od[..., :part * 32].contiguous()
        od = od[..., part * 32:]
        losses.append(tr.steps(X, Y, o)[at].cpu().numpy())
    return tr.state()[at], np.concatenate(losses)


@pytest.fixture(scope="module")
def iso_data():
    x, y = R.synth_rows(700, 39, 3, 21)
    order = np.random.default_rng(22).permutation(64 * 32 * 2)[:64 * 32].astype(np.int32) % 700
    return x, y, order


def test_isolation_and_determinism(torch_cuda, iso_data):
    """A model's result does not depend on its launch: alone, one of 5, one of
    300 (more workgroups than CUs), run twice, in two calls of 32 steps."""
    x, y, order = iso_data
    want, wloss = _train(torch_cuda, 1, 0, x, y, order)
    assert np.isfinite(want).all() and wloss[-1] < wloss[0]
    for n_models, at in ((1, 0), (5, 3), (300, 299), (300, 7)):
        got, gloss = _train(torch_cuda, n_models, at, x, y, order)
        assert np.array_equal(_bits(got), _bits(want)), (n_models, at)
        assert np.array_equal(_bits(gloss), _bits(wloss)), (n_models, at)
    got, gloss = _train(torch_cuda, 5, 3, x, y, order, split=[32, 32])
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(gloss), _bits(wloss))


def test_shared_order_equals_repeated_order(torch_cuda, iso_data):
    from vad_amd.train import FFNTrainer
    torch = torch_cuda
    x, y, order = iso_data
    X, Y = dev(torch, x), dev(torch, y)
    a = FFNTrainer(REF39, n_models=4, seed=8, lr=[1.0, 0.5, 2.0, 1.0])
    b = FFNTrainer(REF39, n_models=4, seed=8, lr=[1.0, 0.5, 2.0, 1.0])
    la = a.steps(X, Y, dev(torch, order))
    lb = b.steps(X, Y, dev(torch, np.tile(order, (4, 1))))
    assert np.array_equal(_bits(a.state()), _bits(b.state()))
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32))
    assert not np.array_equal(a.state()[0], a.state()[1])


def test_ignores_stale_lds(torch_cuda, iso_data):
    """The 64-step run is bit-identical after every CU's LDS was filled with
    +-1e30 / NaN (loaded as tests/test_gpu_lds_independence.py does)."""
    torch = torch_cuda
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_host", "liblds_poison.so")
    if not os.path.exists(so):
        pytest.fail("tests/c_host/liblds_poison.so missing: run __graft_entry__.build()")
    helper = ctypes.CDLL(so)
    helper.lds_poison.argtypes = [ctypes.c_float, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    sink = torch.zeros(1, device="cuda")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    x, y, order = iso_data
    want, wloss = _train(torch, 5, 3, x, y, order, split=[32, 32])
    for v in (1e30, -1e30, float("nan")):
        def fill():
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            assert helper.lds_poison(v, ctypes.c_void_p(sink.data_ptr()), 4 * n_cu, st) == 0
        got, gloss = _train(torch, 5, 3, x, y, order, split=[32, 32], before=fill)
        assert np.array_equal(_bits(got), _bits(want)), v
        assert np.array_equal(_bits(gloss), _bits(wloss)), v
    torch.cuda.synchronize()
    assert sink.item() == 0.0


@pytest.mark.parametrize("n_rows", [1000, 1])
def test_evaluate(torch_cuda, n_rows):
    """Loss within C x the float32 forward's error (plus the spacing of the
    fp32 result itself) of a float64 forward; the correct count exact over the
    rows whose float64 logit margin exceeds 0.05, the others free."""
    from vad_amd.train import FFNTrainer
    torch = torch_cuda
    x, y = R.synth_rows(1500, 39, 3, 31)
    tr = FFNTrainer(REF39, n_models=3, seed=4)
    tr.steps(dev(torch, x), dev(torch, y), dev(torch, np.arange(32 * 16, dtype=np.int32)), return_loss=False)
    xe, ye = x[400:400 + n_rows], y[400:400 + n_rows]
    loss, acc = tr.evaluate(dev(torch, xe), dev(torch, ye))
    assert loss.shape == acc.shape == (3,)
    for m in range(3):
        lay = tr.layers(m)
        z64 = R.forward(xe, lay, np.float64)
        l64 = R.row_losses(z64, ye).mean()
        l32 = R.row_losses(R.forward(xe, lay, np.float32), ye).astype(np.float64).mean()
        tol = C * abs(l32 - l64) + 2 * float(np.spacing(np.float32(l64)))
        print(f"evaluate rows {n_rows} model {m}: loss {loss[m]:.9g} f64 {l64:.9g} f32 err {abs(l32 - l64):.3g} "
              f"err {abs(loss[m] - l64):.3g} tol {tol:.3g}")
        assert abs(loss[m] - l64) <= tol
        s = np.sort(z64, axis=1)
        sure = s[:, -1] - s[:, -2] > 0.05
        hit = z64.argmax(axis=1) == ye
        correct = int(round(acc[m] * n_rows))
        assert (hit & sure).sum() <= correct <= (hit & sure).sum() + (~sure).sum()
        assert sure.mean() > 0.8 or n_rows == 1


def test_end_to_end(torch_cuda, golden, tmp_path):
    """fit on 512 x 32 rows; the trained model classifies as the float64-trained
    reference model does, and drops into the pipeline through its .npz."""
    from vad_amd.ffn import FFNClassifier
    from vad_amd.pipeline import VadPipeline
    from vad_amd.train import FFNTrainer
    torch = torch_cuda
    n = 512 * 32
    x, y = R.synth_rows(n + 2000, 39, 3, 41)
    tr = FFNTrainer(REF39, n_models=2, seed=6)
    start = tr.layers(1)
    hist = tr.fit(dev(torch, x[:n]), dev(torch, y[:n]), epochs=1, shuffle=False,
                  val=(dev(torch, x[n:]), dev(torch, y[n:])))
    steps = tr.last_step_loss.cpu().numpy()
    assert steps.shape == (2, 512)
    print(f"end to end: first loss {steps[:, 0]}, last 8 mean {steps[:, -8:].mean(axis=1)}, epoch {hist}")
    assert (steps[:, -8:].mean(axis=1) < 0.5 * steps[:, 0]).all()
    assert np.allclose(hist[0]["loss"], steps.astype(np.float64).mean(axis=1))
    assert (hist[0]["val_acc"] > 0.9).all() and tr.best("val_acc") in (0, 1)
    lr, rho, eps = (float(v) for v in tr.hyper[1])
    s64, _ = R.torch_train(start, x, y, np.arange(n), 32, lr, rho, eps, torch.float64)
    ref = R.layers_of(s64, REF39)
    z = R.forward(x[n:], ref, np.float64)
    s = np.sort(z, axis=1)
    sure = s[:, -1] - s[:, -2] > 0.05
    assert sure.mean() > 0.9
    got = tr.classifier(1).predict(x[n:])
    assert np.array_equal(got[sure], z.argmax(axis=1)[sure])
    p = tmp_path / "trained.npz"
    tr.save(str(p), 1)
    clf = FFNClassifier.load(str(p))
    for (w, b), (w2, b2) in zip(clf.layers, tr.layers(1)):
        assert np.array_equal(w, w2) and np.array_equal(b, b2)
    g = golden("ffn")
    clip = torch.from_numpy(np.ascontiguousarray(g["test_clip"][:16000 * 2])).cuda()
    labels = VadPipeline(clf).labels(clip)
    assert labels.numel() > 0 and int(labels.max()) < 3
