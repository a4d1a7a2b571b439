"""The edge plans of the resampler (vad_amd.resample.ResampleSpec) and what the
tests of every ratio class share: the rate matrix with the plan sizes it was
chosen for, the inputs, the fma-chain acceptance bound, and two deliberately
wrong models that the bound has to reject (tests/test_resample_cpu.py asserts
that it does; tests/test_gpu_resample_ratios.py relies on it).

Why these rates (all to 16 kHz; table = up * (T | 1) floats of LDS, span = the
input floats one tile of 1024 outputs can need, both limited to 16,384):

  96000, 32000, 22050   headline rates no device test ran; 22050 has an even T
                        (28) padded to rows of 29
  24000, 12000, 20000   small up and down on both sides of 1; 20000 has T = 26
  16100, 15975          down / up just above and just below 1: jl advances by
                        0, 1 or 2 per output and r walks every phase row
  19975                 the table limit: 640 rows of 25, 16,000 floats
  192000, 240000        large down: T = 241 / 301, span 12,517 / 15,646
  1000, 500             large up, tiny inputs; stream delay of exactly one and
                        two hops of 160 outputs
"""
import numpy as np

from vad_amd import resample as R

EDGE_RATES = [96000, 32000, 22050, 24000, 12000, 20000, 16100, 15975, 19975, 192000, 240000, 1000, 500]

# rate: (up, down, T, table floats, tile span floats, stream delay, stream history Hn)
EDGE_PLANS = {
    96000: (1, 6, 121, 121, 6259, 10, 120),
    32000: (1, 2, 41, 41, 2087, 10, 40),
    22050: (320, 441, 28, 9280, 1438, 10, 27),
    24000: (2, 3, 31, 62, 1566, 10, 30),
    12000: (4, 3, 21, 84, 789, 14, 21),
    20000: (4, 5, 26, 108, 1305, 10, 25),
    16100: (160, 161, 21, 3360, 1051, 10, 20),
    15975: (640, 639, 21, 13440, 1043, 11, 21),
    19975: (640, 799, 25, 16000, 1303, 10, 24),
    192000: (1, 12, 241, 241, 12517, 10, 240),
    240000: (1, 15, 301, 301, 15646, 10, 300),
    1000: (16, 1, 21, 336, 85, 160, 20),
    500: (32, 1, 21, 672, 53, 320, 20),
}

U = 2.0 ** -24  # unit roundoff of float32


# the rates of the sessions test, histories 300, 20, 20, 120, 20, 60, 20, 40
SESSION_RATES = [240000, 500, 16100, 96000, 1000, 48000, 8000, 32000]


def sessions_script():
    """The sessions workload over SESSION_RATES: (B, S) = (8, 8) int32 hop
    counts for K = 3, uint8 restart flags and int32 rate indices (read under a
    flag only: the others name some other rate and must change nothing).

      stream 0  240000 -> 500 -> 240000 -> 500: history 300 -> 20 and back
      stream 1  500 Hz (delay 320): one hop, a restart with no hop, one hop, a
                stall, then past the delay; then 1000 Hz, then 240000
      stream 2  16100 throughout, counts 0 .. K and both clamps (-1, K + 1)
      stream 3  96000 -> 1000 -> 96000, a stall at 1000 Hz
      stream 4  1000 -> 240000 -> 16100
      stream 5  48000 -> 8000 -> 32000
      stream 6  starts with no hop, stalls twice, 8000 -> 96000 -> 8000
      stream 7  restart indices 9, -1 and 8, clamped to 32000, 240000, 32000
    """
    counts = np.array([[3, 2, 3, 1, 3, 0, 3, 2],
                       [1, 0, 1, 0, 3, 1, 2, 3],
                       [3, 0, 1, 2, 3, 3, -1, 4],
                       [3, 3, 2, 3, 0, 3, 3, 1],
                       [2, 1, 3, 3, 3, 3, 0, 3],
                       [3, 3, 3, 2, 3, 0, 3, 3],
                       [0, 3, 0, -1, 3, 3, 2, 1],
                       [3, 3, 3, 3, 3, 3, 3, 3]], np.int32).T.copy()
    starts = [{0: 0, 2: 1, 4: 0, 6: 1}, {0: 1, 1: 1, 5: 4, 7: 0}, {0: 2}, {0: 3, 3: 4, 5: 3}, {0: 4, 2: 0, 5: 2},
              {0: 5, 3: 6, 6: 7}, {0: 6, 4: 3, 6: 6}, {0: 9, 4: -1, 6: 8}]
    B, S = counts.shape
    restart = np.zeros((B, S), np.uint8)
    rate = (np.arange(B)[:, None] * 3 + np.arange(S)[None, :] + 1).astype(np.int32) % len(SESSION_RATES)
    for s, when in enumerate(starts):
        for b, i in when.items():
            restart[b, s], rate[b, s] = 1, i
    return counts, restart, rate


def plan_sizes(spec):
    """The EDGE_PLANS row of a ResampleSpec, from the spec's own fields."""
    table = spec.up * spec.row_stride
    span = -(-((R.TILE_OUT - 1) * spec.down) // spec.up) + spec.phase_len
    return spec.up, spec.down, spec.phase_len, table, span, spec.delay, spec.history


def ints(n, seed, lo=-32768, hi=32768):
    """White int16 noise over the full range (tests/test_gpu_resample.py's)."""
    return np.random.default_rng(seed).integers(lo, hi, n).astype(np.int16)


def lengths(spec, tout):
    """Input lengths 0, 1, T-1 and, for n_out = tout-1, tout, tout+1 and
    2 tout+1, the longest input with no more outputs than that and the shortest
    with no fewer: the same input where the count is reachable, its two
    neighbours where up > down steps over it (at 16 / 1 only multiples of 16
    are)."""
    ns = [0, 1, spec.phase_len - 1]
    step = -(-spec.up // spec.down)
    for target in (tout - 1, tout, tout + 1, 2 * tout + 1):
        lo = target * spec.down // spec.up   # the longest input with n_out <= target
        hi = lo + (spec.n_out(lo) < target)  # the shortest with n_out >= target
        assert target - step < spec.n_out(lo) <= target <= spec.n_out(hi) < target + step
        ns += [lo, hi]
    return list(dict.fromkeys(ns))


def clip_input(rate, n):
    return ints(n, rate + n)


def taps32(spec):
    """The taps the device holds: float32(taps), as float64."""
    return spec.taps.astype(np.float32).astype(np.float64)


def chain_bound(x, spec):
    """gamma * sum_j |h_j| |x_j| per output, gamma = T u / (1 - T u): the
    error bound of a T-term float32 fma chain in any order against the exact
    sum of the same float32 taps."""
    gamma = spec.phase_len * U / (1 - spec.phase_len * U)
    return gamma * R.resample_model(np.abs(np.asarray(x, np.float64)), spec, taps=np.abs(taps32(spec)))


def shifted_model(x, spec, taps, dj=0, dq=0):
    """resample_model's sum with the index computation q -> jl, r wrong by one:

      dj = +-1  the newest input sample of every output is x[jmax +- 1]: jl off
                by one input sample;
      dq = +-1  the taps are h[r +- 1 + i * up]: the phase row off by one (from
                row up-1 onwards into row 0 one tap later, which is what the
                next row of a contiguous table would be).  With up = 1 there
                is one row, and this is the shift by one input sample again.

    dj = dq = 0 is resample_model itself, to the bit."""
    x = np.asarray(x, np.float64).reshape(-1)
    n, n_out, T = len(x), spec.n_out(len(x)), spec.phase_len
    if n_out == 0:
        return np.zeros(0, np.float64)
    q = np.arange(n_out, dtype=np.int64) * spec.down + spec.half_len + dq
    jmax, r = q // spec.up + dj, q % spec.up
    w = np.concatenate([np.zeros(T + 1), x, np.zeros(max(int(jmax[-1]) - (n - 1), 0))])
    h = np.concatenate([np.asarray(taps, np.float64), np.zeros(spec.up * (T + 1) - len(taps))])
    return R._dots(w, jmax + (T + 1), r, h.reshape(T + 1, spec.up).T)
