"""read_csv_device / the vad_csv_* entries against numpy on the same text:
``np.asarray(csv.reader rows, dtype)`` compared by bit pattern (nan as nan),
and a Python create_file_index for the line index."""
import csv
import ctypes
import io
import os

import numpy as np
import pytest

import csv_parse_reference as R

pytestmark = pytest.mark.gpu

T = 4096  # VAD_CSV_TILE
MAX_LINE = 4096


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def golden_text(golden):
    return bytes(golden("dataset")["csv_text"]).decode("ascii")


def py_index(data, offset):
    """dataset/file_index.py:7-23 on bytes."""
    index, pos = [], 0
    for k, line in enumerate(io.BytesIO(data)):
        if k >= offset:
            index.append(pos)
        pos += len(line)
    return np.asarray(index, dtype=np.uint64)


def oracle(text, offset, cols, dtype):
    rows = list(csv.reader(io.StringIO(text, newline="")))[offset:]
    if not rows:
        return None, np.zeros(0, np.uint8)
    full = np.asarray(rows, dtype=dtype)
    y = np.asarray([int(float(r[-1])) for r in rows]).astype(np.uint8)
    return (full[:, cols] if cols is not None else full[:, :-1]), y


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def check_text(torch, text, offset=0, cols=None, **kw):
    from vad_amd.dataset import read_csv_device
    data = text.encode("ascii")
    for tdt, ndt in ((torch.float32, np.float32), (torch.float64, np.float64)):
        X, y, index = read_csv_device(data, offset, cols, tdt, **kw)
        wx, wy = oracle(text, offset, cols, ndt)
        assert X.dtype == tdt and y.dtype == torch.uint8 and index.dtype == torch.int64
        assert np.array_equal(index.cpu().numpy().astype(np.uint64), py_index(data, offset))
        assert np.array_equal(y.cpu().numpy(), wy)
        if wx is None:
            assert X.shape[0] == 0
        else:
            assert same_bits(X.cpu().numpy(), wx)
    return X, y, index


def test_golden_text(torch_cuda, golden_text):
    X, _, _ = check_text(torch_cuda, golden_text)
    assert tuple(X.shape) == (273, 39)
    header = ",".join(f"c{i}" for i in range(40)) + "\r\n"
    check_text(torch_cuda, header + golden_text, offset=1)
    check_text(torch_cuda, header + golden_text, offset=1, cols=[38, 0, 5])


def padded_line(total, body, term):
    """A line of exactly ``total`` bytes, terminator included: ``body`` behind leading zeros."""
    k = total - len(body) - len(term)
    assert 0 <= k and total - len(term) <= MAX_LINE
    return "0" * k + body + term


@pytest.mark.parametrize("term,first,second", [
    ("\n", T, "2.5,0"),            # '\n' is the last byte of tile 0
    ("\n", T + 1, "2.5,0"),        # '\n' is the first byte of tile 1
    ("\r\n", T + 1, "2.5,0"),      # "\r\n" straddles the boundary
    ("\r\n", T, "2.5,0"),
    ("\r\n", T - 2, "123.456,1"),  # the second line crosses the boundary inside its first field
    ("\r\n", T - 4, "1.5e-3,1"),   # ... inside the exponent: "1.5e" | "-3"
    ("\n", T - 4, "1.5e-3,1"),
])
def test_tile_edges(torch_cuda, term, first, second):
    text = padded_line(first, "1.25,1", term) + second + term + "7.5,3" + term
    assert text[first - 1] == "\n"
    check_text(torch_cuda, text)


@pytest.mark.parametrize("total", [T - 1, T, T + 1])
@pytest.mark.parametrize("tail", ["\r\n", ""])
def test_text_of_a_tile_more_or_less(torch_cuda, total, tail):
    rest = "2.5,0" + tail
    text = padded_line(total - len(rest), "1.25,1", "\r\n") + rest
    assert len(text) == total
    check_text(torch_cuda, text)


def test_more_tiles_than_one_carry_pass(torch_cuda, golden_text):
    text = golden_text * 6
    assert len(text) > 256 * T
    check_text(torch_cuda, text)
    check_text(torch_cuda, text, offset=300)


def test_row_counts(torch_cuda):
    from vad_amd.dataset import read_csv_device
    torch = torch_cuda
    X, y, index = check_text(torch, "a,b,c\r\n", offset=1)
    assert tuple(X.shape) == (0, 2) and y.numel() == 0 and index.numel() == 0
    X, y, index = read_csv_device(b"", 1)
    assert X.shape[0] == 0 and y.numel() == 0 and index.numel() == 0
    check_text(torch, "a,b\r\n1.5,1", offset=1)
    check_text(torch, "1.5,1")
    check_text(torch, "a,b\n" + "".join(f"{i}.5,{i % 2}\n" for i in range(10)), offset=1)
    for n in (63, 64, 65):
        check_text(torch, "".join(f"{i}.25,-{i}e-3,{i % 3}\r\n" for i in range(n)))
    check_text(torch, "a,b\r\n1,1\r\n2,0\r\n", offset=5)  # more lines skipped than there are


@pytest.mark.parametrize("n_cols", [2, 40, 64, 65, 66, 130])
def test_field_counts(torch_cuda, n_cols):
    rng = np.random.default_rng(n_cols)
    vals = rng.standard_normal((7, n_cols - 1))
    text = "".join(",".join(repr(float(v)) for v in row) + f",{k % 2}\r\n" for k, row in enumerate(vals))
    check_text(torch_cuda, text)
    if n_cols >= 40:
        check_text(torch_cuda, text, cols=[38, 0, 5])
        check_text(torch_cuda, text, cols=list(range(n_cols - 1, -1, -1)))


def raw_parse(torch, data, n_cols, f64=False):
    """The three C entries on a device copy of ``data``: X, y, row_status."""
    from vad_amd import _lib
    lib = _lib.lib()
    d = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    nb = int(lib.vad_csv_workspace_bytes(len(data)))
    ws = torch.empty(nb // 8, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = _lib.stream_ptr()
    _lib.check(lib.vad_csv_count_lines(_lib.ptr(d), len(data), _lib.ptr(count), _lib.ptr(ws), nb, st), "count")
    n = int(count.item())
    index = torch.empty(n, dtype=torch.int64, device="cuda")
    _lib.check(lib.vad_csv_index(_lib.ptr(d), len(data), 0, 0, _lib.ptr(index), n, _lib.ptr(ws), nb, st), "index")
    X = torch.zeros((n, n_cols - 1), dtype=torch.float64 if f64 else torch.float32, device="cuda")
    y = torch.zeros(n, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.vad_csv_parse(_lib.ptr(d), len(data), _lib.ptr(index), n, 0, n_cols, None, n_cols - 1, int(f64),
                                 _lib.ptr(X), _lib.ptr(y), _lib.ptr(status), st), "parse")
    return X.cpu().numpy(), y.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("which", ["edge", "float32", "double"])
def test_field_sets_and_host_flags(torch_cuda, which):
    """One field per row: the device decides exactly the fields the
    restatement decides, to the same bits, and flagged rows come back patched."""
    fields = {"edge": R.EDGE, "float32": R.random_float32_fields, "double": R.random_double_fields}[which]
    fields = fields if isinstance(fields, list) else fields(4000)
    text = "".join(f + ",1\r\n" for f in fields)
    X, y, status = raw_parse(torch_cuda, text.encode("ascii"), 2, f64=True)
    want = [R.parse_field(f) for f in fields]
    host = np.asarray([w == R.HOST for w in want])
    assert np.array_equal(status != 0, host) and np.all(status[host] == 1)
    assert int(host.sum()) == sum(w == R.HOST for w in want)
    got = X[:, 0].view(np.uint64)
    for f, w, g, h in zip(fields, want, got, host):
        assert h or int(g) == w, (f, hex(int(g)), w)
    assert np.all(y == 1)
    check_text(torch_cuda, text)


@pytest.mark.parametrize("bad,line", [
    ("1.5,2.5\r\n", 3),                       # a short row
    ("1.5,2.5,3.5,1\r\n", 3),                 # a long row
    ("\r\n", 3),                              # an empty line in the middle
    ("0" * (MAX_LINE + 1) + "1.5,2.5,1\r\n", 3),  # over the length limit
    ("1.2.3,2.5,1\r\n", 3),
    ("1.5,abc,1\r\n", 3),
    ("1.5,2.5,256\r\n", 3),
    ("1.5,2.5,-1\r\n", 3),
    ("1.5,2.5,nan\r\n", 3),
])
def test_malformed_input_raises(torch_cuda, bad, line):
    from vad_amd.dataset import read_csv_device
    text = "a,b,c\r\n0.5,0.25,0\r\n" + bad + "0.75,1e3,1\r\n"
    for chunk in (None, 16):
        with pytest.raises(ValueError, match=rf"line {line}\b"):
            read_csv_device(text.encode("ascii"), 1, chunk_bytes=chunk)
    ok, _, _ = read_csv_device(b"a,b,c\r\n0.5,0.25,0\r\n0.75,1e3,1\r\n", 1)
    assert tuple(ok.shape) == (2, 2)


def test_independent_of_stale_lds(torch_cuda, golden_text):
    torch = torch_cuda
    from vad_amd.dataset import read_csv_device
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_host", "liblds_poison.so")
    if not os.path.exists(so):
        pytest.fail("tests/c_host/liblds_poison.so missing: run __graft_entry__.build()")
    helper = ctypes.CDLL(so)
    helper.lds_poison.argtypes = [ctypes.c_float, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    sink = torch.zeros(1, device="cuda")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    data = (golden_text + "1.5,2.5\r\n").encode("ascii")  # its last row is malformed: read the entries' raw outputs
    want = raw_parse(torch, data, 40)
    for v in (1e30, -1e30, float("nan")):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert helper.lds_poison(v, ctypes.c_void_p(sink.data_ptr()), 4 * n_cu, stream) == 0
        got = raw_parse(torch, data, 40)
        assert same_bits(got[0][:-1], want[0][:-1]) and np.array_equal(got[1][:-1], want[1][:-1])
        assert np.array_equal(got[2], want[2]) and got[2][-1] == 2
    assert sink.item() == 0.0
    good = golden_text.encode("ascii")
    a = read_csv_device(good, 0)
    assert helper.lds_poison(1e30, ctypes.c_void_p(sink.data_ptr()), 4 * n_cu,
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    b = read_csv_device(good, 0)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def random_float32_rows(n, k, seed):
    b = np.random.default_rng(seed).integers(0, 1 << 32, n * k, dtype=np.uint64).astype(np.uint32)
    x = b.view(np.float32).copy()
    x[np.isnan(x)] = np.float32("nan")  # the text says "nan": one payload
    return x.reshape(n, k)


def test_round_trip_of_the_formatter(torch_cuda):
    from vad_amd.dataset import format_csv_rows, read_csv_device
    rows = random_float32_rows(2000, 39, seed=11)
    text = format_csv_rows(rows, 1)
    X, y, _ = read_csv_device(text.encode("ascii"), 0)
    assert same_bits(X.cpu().numpy(), rows)
    assert np.array_equal(X.cpu().numpy().view(np.uint32)[~np.isnan(rows)], rows.view(np.uint32)[~np.isnan(rows)])
    assert bool((y == 1).all())


def test_chunked_read_equals_one_chunk(torch_cuda, golden_text, tmp_path):
    torch = torch_cuda
    from vad_amd.dataset import create_file_index, features_number, load_csv, load_files, read_csv_device
    text = "h," * 39 + "h\r\n" + golden_text
    data = text.encode("ascii")
    one = read_csv_device(data, 1)
    for chunk in (1000, 4097, 100):  # 100: shorter than a line, the buffer grows
        parts = read_csv_device(data, 1, chunk_bytes=chunk)
        assert all(torch.equal(p, q) for p, q in zip(one, parts))
    path = tmp_path / "voiced.csv"
    path.write_bytes(data)
    from_file = read_csv_device(str(path), 1, chunk_bytes=5000)
    assert all(torch.equal(p, q) for p, q in zip(one, from_file))
    assert np.array_equal(create_file_index(str(path)), py_index(data, 1))
    assert create_file_index(str(path)).dtype == np.uint64 and features_number(str(path)) == 273
    wx, wy = oracle(text, 1, None, np.float32)
    f, r = load_csv(str(path), 100)
    assert f.dtype == np.float32 and r.dtype == np.int32 and r.shape == (100, 1)
    assert same_bits(f, wx[:100]) and np.array_equal(r[:, 0], wy[:100])
    f, r = load_csv(str(path), 7, columns_used=[3, 1], dtype=np.float64)
    assert same_bits(f, oracle(text, 1, [3, 1], np.float64)[0][:7])
    with pytest.raises(ValueError):
        load_csv(str(path), 274)
    f, r = load_files([str(path), str(path)], [5, 9])
    w64 = oracle(text, 1, None, np.float64)[0]
    assert f.dtype == np.float64 and same_bits(f, np.concatenate([w64[:5], w64[:9]])) and r.shape == (14, 1)


def test_end_to_end_into_the_trainers(torch_cuda):
    """Text -> read_csv_device -> FFNTrainer.steps with a random_rows_order
    and TreeTrainer.fit: the same as from host-parsed arrays."""
    torch = torch_cuda
    from vad_amd.dataset import format_csv_rows, random_rows_order, read_csv_device
    from vad_amd.train import FFNTrainer
    from vad_amd.tree_train import TreeTrainer
    rng = np.random.default_rng(21)
    n = 600
    labels = rng.integers(0, 2, n)
    rows = (rng.standard_normal((n, 39)) + labels[:, None] * 0.7).astype(np.float32)
    text = "".join(format_csv_rows(rows[i:i + 1], int(labels[i])) for i in range(n))
    X, y, _ = read_csv_device(text.encode("ascii"), 0)
    hx, hy = oracle(text, 0, None, np.float32)
    assert same_bits(hx, rows) and np.array_equal(hy, labels)
    Xh, yh = torch.from_numpy(hx).cuda(), torch.from_numpy(hy).cuda()
    order = random_rows_order([400, 200], 0.8, 8, seed=2)
    order = torch.from_numpy(order[:len(order) // 32 * 32].copy()).cuda()
    states = []
    for a, b in ((X, y), (Xh, yh)):
        tr = FFNTrainer(n_models=2, seed=3)
        loss = tr.steps(a, b, order)
        states.append((tr.state(), loss.cpu().numpy()))
    assert np.array_equal(states[0][0].view(np.uint32), states[1][0].view(np.uint32))
    assert np.array_equal(states[0][1].view(np.uint32), states[1][1].view(np.uint32))
    trees = [TreeTrainer(max_depth=6).fit(a, b) for a, b in ((X, y), (Xh, yh))]
    for k in ("feature", "threshold", "left", "right", "leaf", "n_node_samples"):
        assert np.array_equal(getattr(trees[0], k), getattr(trees[1], k)), k
    assert len(trees[0].feature) > 1
