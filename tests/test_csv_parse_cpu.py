"""The CSV parser's algorithm, proven on the host before any GPU run: the
generated powers-of-five table, the Python restatement of the device parser
(tests/csv_parse_reference.py) against float(), the share of fields it leaves
to the host, and random_rows_order."""
import os

import numpy as np
import pytest

import csv_parse_reference as R
from vad_amd import gen_pow5 as G

HERE = os.path.dirname(os.path.abspath(__file__))


def test_table_is_big_integer_powers_of_five():
    t = G.table()
    assert len(t) == G.Q_MAX - G.Q_MIN + 1
    for q, v in zip(range(G.Q_MIN, G.Q_MAX + 1), t):
        assert 1 << 127 <= v < 1 << 128
        e = (q * G.LOG2_5_Q16) >> 16  # floor(log2(5^q))
        s = 127 - e
        # v = floor(5^q * 2^s), stated without division: v <= 5^q 2^s < v + 1
        num, den = (5 ** q, 1) if q >= 0 else (1, 5 ** -q)
        num, den = (num << s, den) if s >= 0 else (num, den << -s)
        assert v * den <= num < (v + 1) * den, q
        assert (v * den == num) == (0 <= q <= G.Q_EXACT_MAX), q
    assert 10 ** G.MAX_DIGITS < 1 << 64 and 5 ** G.SMALL_MAX < 1 << 64
    assert float(10 ** G.FAST_MAX_EXP) == 10 ** G.FAST_MAX_EXP


def test_committed_header_is_what_the_generator_prints():
    with open(G.OUT) as f:
        assert f.read() == G.render()


def check_against_float(fields):
    """Bit equality with float() wherever the restatement decides; returns
    the reasons of the fields it leaves to the host."""
    reasons = []
    for f in fields:
        got, why = R.parse_field_ex(f)
        if got == R.HOST:
            reasons.append(why)
            continue
        want = float(f)
        if want != want:
            assert got == R.NAN_BITS, f
        else:
            assert got == R.bits_of(want), (f, hex(got), hex(R.bits_of(want)))
    return reasons


def golden_fields(golden):
    text = bytes(golden("dataset")["csv_text"]).decode("ascii")
    return [x for line in text.splitlines() for x in line.split(",")]


def test_restatement_equals_float_on_golden_text(golden):
    fields = golden_fields(golden)
    assert len(fields) == 273 * 40
    assert len(check_against_float(fields)) * 1000 <= len(fields)


def test_restatement_equals_float_on_random_doubles():
    fields = R.random_double_fields()
    reasons = check_against_float(fields)
    assert R.DIGITS not in reasons and R.GRAMMAR not in reasons
    assert len(reasons) * 1000 <= len(fields)


def test_restatement_equals_float_on_float32_text():
    fields = R.random_float32_fields()
    assert check_against_float(fields) == []


def test_restatement_on_the_edge_list():
    for f in R.EDGE:
        got, why = R.parse_field_ex(f)
        try:
            want = float(f)
        except ValueError:
            assert got == R.HOST and why == R.GRAMMAR, f
            continue
        if got == R.HOST:
            continue
        assert got == (R.NAN_BITS if want != want else R.bits_of(want)), f
    decided = {f: R.parse_field(f) != R.HOST for f in R.EDGE}
    mids = R.float32_midpoint_fields()
    assert [decided[m] for m in mids] == [False, False, False, True, True]  # 25 digits: host; 19: device
    for f in ("1e22", "1e23", "9007199254740993", "8.98846567431158e307", "4.9e-324", "2.4703282292062327e-324",
              "1e-400", "1e400", "+1.5", "1.", ".5", "1E-5", "0.000000000000000000001234", "00012.50", "-0.0", "NaN",
              "-inf", "Infinity", "1274361900000000.0", "3801906481570168.5"):
        assert decided[f], f
    for f in (" 1.5", "2.5 ", "-nan", "1_0"):
        assert not decided[f], f
    # numpy's contract is the rounded double, cast once: the 19-digit text just above the float32 midpoint
    # rounds to the midpoint as a double, and the cast's tie goes to the even neighbour, 1.0
    for m in mids[3:]:
        assert np.float32(R.double_of(R.parse_field(m))) == np.asarray([m], dtype=np.float32)[0] == np.float32(1)
    assert R.parse_field("-0.0") == R.SIGN


def test_formatter_output_never_goes_to_the_host():
    from vad_amd.dataset import format_csv_rows
    b = np.random.default_rng(5).integers(0, 1 << 32, 39 * 500, dtype=np.uint64).astype(np.uint32)
    b[:7] = [0, 0x80000000, 0x7F7FFFFF, 0x7FC00000, 0x7F800000, 0xFF800000, 1]
    rows = b.view(np.float32).reshape(500, 39)
    text = format_csv_rows(rows, 1)
    fields = [x for line in text.splitlines() for x in line.split(",")]
    assert len(fields) == 500 * 40
    assert check_against_float(fields) == []


def test_more_than_19_digits_all_go_to_the_host():
    fields = ["%.25e" % R.double_of(R.bits_of(float(f))) for f in R.random_double_fields(1000, seed=9)]
    assert all(R.parse_field_ex(f) == (R.HOST, R.DIGITS) for f in fields)


def test_random_rows_order():
    from vad_amd.dataset import random_rows_order
    sizes, lpb = [1000, 333, 5, 64], 8
    order = random_rows_order(sizes, 0.5, lpb, seed=4)
    assert order.dtype == np.int32
    bases = np.concatenate([[0], np.cumsum(sizes)])
    assert len(order) == sum(int(0.5 * n) for n in sizes)
    for i, n in enumerate(sizes):
        mine = order[(order >= bases[i]) & (order < bases[i + 1])] - bases[i]
        m, run = int(0.5 * n), min(lpb, n)
        assert len(mine) == m
        blocks = [mine[k:k + run] for k in range(0, m, run)]  # a source's rows keep their order
        for blk in blocks:
            assert np.array_equal(blk, blk[0] + np.arange(len(blk)))
            assert 0 <= blk[0] <= n - run
    assert order.min() >= 0 and order.max() < bases[-1]
    assert np.array_equal(order, random_rows_order(sizes, 0.5, lpb, seed=4))
    assert not np.array_equal(order, random_rows_order(sizes, 0.5, lpb, seed=5))
    # interleaved: the first source does not come out in one piece
    first = np.flatnonzero(order < bases[1])
    assert first[-1] - first[0] + 1 > len(first)
    assert len(random_rows_order([10, 20], 1.0, 8, seed=0)) == 30
    assert len(random_rows_order([], 1.0)) == 0
