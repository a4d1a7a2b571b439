"""The CSV import entries refuse bad arguments before any HIP call (no GPU
here; the pointers below are never dereferenced)."""
import ctypes

import pytest

E = -1
N = None
BYTES, IDX, X, Y, ST, WS, CNT = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x100000, 0x60000


@pytest.fixture(scope="module")
def lib():
    from vad_amd import _lib
    return _lib.lib()


def cols_of(c):
    return None if c is None else (ctypes.c_int32 * len(c))(*c)


def test_workspace_bytes(lib):
    assert lib.vad_csv_workspace_bytes(-1) == 0
    assert lib.vad_csv_workspace_bytes(0) > 0
    assert lib.vad_csv_workspace_bytes(1 << 30) >= 2 * 8 * ((1 << 30) // 4096)
    assert lib.vad_csv_workspace_bytes(1 << 20) % 256 == 0


def test_count_lines_refuses(lib):
    def call(bytes_=BYTES, n=1000, out=CNT, ws=WS, ws_bytes=1 << 30):
        return lib.vad_csv_count_lines(bytes_, n, out, ws, ws_bytes, N)

    for kw in (dict(bytes_=N), dict(n=-1), dict(out=N), dict(out=CNT + 4), dict(ws=N), dict(ws=WS + 4),
               dict(ws_bytes=0), dict(ws_bytes=lib.vad_csv_workspace_bytes(1000) - 1), dict(n=(1 << 42) + 1)):
        assert call(**kw) == E, kw


def test_index_refuses(lib):
    def call(bytes_=BYTES, n=1000, skip=1, base=0, index=IDX, cap=10, ws=WS, ws_bytes=1 << 30):
        return lib.vad_csv_index(bytes_, n, skip, base, index, cap, ws, ws_bytes, N)

    for kw in (dict(bytes_=N), dict(n=-1), dict(skip=-1), dict(base=-1), dict(index=N), dict(index=IDX + 4),
               dict(cap=-1), dict(ws=N), dict(ws_bytes=0), dict(ws_bytes=lib.vad_csv_workspace_bytes(1000) - 1)):
        assert call(**kw) == E, kw


def test_parse_refuses(lib):
    def call(bytes_=BYTES, n=1000, index=IDX, rows=10, base=0, n_cols=40, cols=None, n_used=39, f64=0, x=X, y=Y,
             st=ST):
        return lib.vad_csv_parse(bytes_, n, index, rows, base, n_cols, cols_of(cols), n_used, f64, x, y, st, N)

    for kw in (dict(bytes_=N), dict(n=-1), dict(n=0), dict(index=N), dict(index=IDX + 4), dict(rows=-1),
               dict(base=-1), dict(n_cols=1), dict(n_cols=0), dict(n_cols=2049), dict(n_used=38), dict(n_used=0),
               dict(cols=[0, 40], n_used=2), dict(cols=[-1], n_used=1), dict(cols=[0] * 1025, n_used=1025),
               dict(x=N), dict(y=N), dict(st=N), dict(x=X + 2), dict(x=X + 4, f64=1), dict(st=ST + 2)):
        assert call(**kw) == E, kw
