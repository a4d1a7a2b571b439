"""Pure-Python restatement of the CSV field parser of
vad_amd/csrc/csv_parse_kernel.hip: the same grammar, the same 19-digit cap,
the same generated table of 128-bit powers of five and the same "host" rules,
in integer arithmetic on 64-bit words (masked Python ints).

parse_field(text) returns the IEEE-754 bits of the double the device stores
(the float32 output is one cast of it), or HOST where the device sets the
row's host flag and leaves the field to ``float()``.
"""
import struct

from vad_amd import gen_pow5 as G

HOST = "host"
M64 = (1 << 64) - 1
TABLE = G.table()
INF_BITS = 0x7FF0000000000000
NAN_BITS = 0x7FF8000000000000
SIGN = 1 << 63
EXP_CAP = 100000  # exponent digits saturate here (far past any double)

# why a field went to the host
DIGITS, AMBIGUOUS, GRAMMAR = "digits", "ambiguous", "grammar"


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def double_of(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def round_pack(m54, sticky, e2):
    """m54: 54 leading bits (2^53 <= m54 < 2^54) of a value in
    [2^e2, 2^(e2+1)); sticky: anything nonzero below them.  Round to nearest
    even into a double's bits (subnormals, zero and infinity included)."""
    normal = e2 >= -1022
    d = 1 if normal else -1021 - e2  # bits dropped from m54
    if d >= 64:
        return 0
    kept = m54 >> d
    rnd = (m54 >> (d - 1)) & 1
    st = sticky or (m54 & ((1 << (d - 1)) - 1)) != 0
    if rnd and (st or kept & 1):
        kept += 1
    bits = (((e2 + 1022) << 52) if normal else 0) + kept
    return INF_BITS if bits >= INF_BITS else bits


def to_double(w, q):
    """Bits of the double nearest w * 10^q (0 <= w < 10^19), or AMBIGUOUS."""
    if w == 0 or q < G.Q_MIN:
        return 0
    if q > G.Q_MAX:
        return INF_BITS
    if w < 1 << 53 and -G.FAST_MAX_EXP <= q <= G.FAST_MAX_EXP:
        # both operands exact doubles: one IEEE operation, correctly rounded
        return bits_of(float(w) * float(10 ** q) if q >= 0 else float(w) / float(10 ** -q))
    lz = 64 - w.bit_length()
    wn = (w << lz) & M64
    t = TABLE[q - G.Q_MIN]
    thi, tlo = t >> 64, t & M64
    exact = 0 <= q <= G.Q_EXACT_MAX
    x = wn * thi
    xh, xl = x >> 64, x & M64
    if tlo == 0:  # exact, and the product is (xh, xl, 0)
        h, m, lo = xh, xl, 0
        sticky = None
    elif not exact and (xh & 0x1FF) != 0x1FF:
        # the true product lies in (L, L + wn) with L = wn * T: the words
        # below xh add less than 2^64 at xl's weight, a carry of at most one
        # into xh, which cannot reach the bits above the low nine
        h, m, lo = xh, 0, 0
        sticky = True
    else:
        y = wn * tlo
        m = xl + (y >> 64)
        h = (xh + (m >> 64)) & M64
        m &= M64
        lo = y & M64
        sticky = None
        if not exact:
            lo2 = lo + wn
            m2 = m + (lo2 >> 64)
            h2 = h + (m2 >> 64)
            up, up2 = h >> 63, h2 >> 63
            if up != up2 or h >> (9 + up) != h2 >> (9 + up2):
                # L and L + wn round differently.  The one case with a rule:
                # 5^-q divides w, so w * 10^q = (w / 5^-q) * 2^q is a dyadic
                # number ("1274361900000000.0"): one rounding of the integer
                # quotient, then an exact scaling
                if -G.SMALL_MAX <= q < 0 and w % 5 ** -q == 0:
                    return bits_of(float(w // 5 ** -q) * 2.0 ** q)
                return AMBIGUOUS
            sticky = True
    up = h >> 63
    m54 = h >> (9 + up)
    if sticky is None:
        sticky = (h & ((1 << (9 + up)) - 1)) != 0 or m != 0 or lo != 0
    e2 = 63 + up + ((q * G.LOG2_5_Q16) >> 16) + q - lz
    return round_pack(m54, sticky, e2)


def _lower(c):
    return c | 0x20


def parse_field_ex(text):
    """(bits, None) or (HOST, reason)."""
    s = text.encode("ascii", "replace") if isinstance(text, str) else bytes(text)
    n, i = len(s), 0
    if n == 0:
        return HOST, GRAMMAR
    neg = signed = False
    if s[0] in b"+-":
        neg, signed, i = s[0] == 0x2D, True, 1
    sign = SIGN if neg else 0
    rest = bytes(_lower(c) for c in s[i:])
    if rest[:1] in (b"n", b"i"):
        if rest == b"nan" and not signed:
            return NAN_BITS, None
        if rest in (b"inf", b"infinity"):
            return INF_BITS | sign, None
        return HOST, GRAMMAR
    w = nd = frac = 0
    seen_digit = seen_point = False
    while i < n:
        c = s[i]
        if 0x30 <= c <= 0x39:
            seen_digit = True
            if w != 0 or c != 0x30:
                if nd < G.MAX_DIGITS:
                    w = w * 10 + (c - 0x30)
                nd += 1
            if seen_point:
                frac += 1
        elif c == 0x2E and not seen_point:
            seen_point = True
        else:
            break
        i += 1
    if not seen_digit:
        return HOST, GRAMMAR
    e = 0
    if i < n and _lower(s[i]) == 0x65:
        i += 1
        eneg = False
        if i < n and s[i] in b"+-":
            eneg = s[i] == 0x2D
            i += 1
        if i >= n or not 0x30 <= s[i] <= 0x39:
            return HOST, GRAMMAR
        while i < n and 0x30 <= s[i] <= 0x39:
            e = min(e * 10 + (s[i] - 0x30), EXP_CAP)
            i += 1
        if eneg:
            e = -e
    if i != n:
        return HOST, GRAMMAR
    if nd > G.MAX_DIGITS:
        return HOST, DIGITS
    r = to_double(w, e - frac)
    if r == AMBIGUOUS:
        return HOST, AMBIGUOUS
    return r | sign, None


def parse_field(text):
    return parse_field_ex(text)[0]


# ---------------------------------------------------------------------------
# The field sets the CPU and GPU tests share
# ---------------------------------------------------------------------------
def float32_midpoint_fields():
    """The midpoint of the float32 neighbours 1 and 1 + 2^-23 has exactly 25
    significant digits; that text +- one unit of its last digit, and its
    19-digit truncation and the next 19-digit number (below / above it)."""
    from decimal import ROUND_FLOOR, Decimal, getcontext
    getcontext().prec = 60
    mid = Decimal(1) + Decimal(2) ** -24
    u25, u19 = Decimal(10) ** -24, Decimal(10) ** -18
    lo19 = mid.quantize(u19, rounding=ROUND_FLOOR)
    return [str(mid - u25), str(mid), str(mid + u25), str(lo19), str(lo19 + u19)]


EDGE = ["1e22", "1e23", "9007199254740993", "8.98846567431158e307", "4.9e-324", "2.4703282292062327e-324",
        "1e-400", "1e400"] + float32_midpoint_fields() + [
        "+1.5", "1.", ".5", "1E-5", "0.000000000000000000001234", "00012.50", "-0.0", "NaN", "-inf", "Infinity",
        # past the issue's list: the largest double and the first overflow, the smallest normal and the largest
        # subnormal, dyadic values behind 17 digits, blanks, a signed nan
        "1.7976931348623157e308", "1.7976931348623159e308", "2.2250738585072014e-308", "2.2250738585072011e-308",
        "1274361900000000.0", "3801906481570168.5", "9007199254740995e-1", " 1.5", "2.5 ", "-nan", "+inf", "inf",
        "1_0", "0e999999999999", "1e-99999999999"]


def random_double_fields(n=20000, seed=1):
    """repr of doubles of random bit patterns: the whole exponent range."""
    import random
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        x = double_of(rng.getrandbits(64))
        if x == x:
            out.append(repr(x))
    return out


def random_float32_fields(n=20000, seed=2):
    """str(np.float32) of random bit patterns, with subnormals, +-0, +-max,
    nan and +-inf among them."""
    import numpy as np
    b = np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    b[:12] = [0, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7FC00000, 0x7F800000, 0xFF800000, 1, 0x80000001, 0x007FFFFF,
              0x00800000, 0x00400000]
    b[12:512] &= 0x807FFFFF  # subnormals
    return [str(x) for x in b.view(np.float32)]
