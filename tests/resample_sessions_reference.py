"""Host model of the sessions form of the stream resampler (include/vad_amd.h,
"Sessions through the stream resampler"; vad_amd.resample.SessionStreamResampler)
in float64 numpy, and the scripted workload the GPU tests run.

The model keeps one ``vad_amd.resample.StreamModel`` (one stream) per stream
and session: a restart flag drops the stream's model and builds a new one at
the rate ``rate_index`` names, clamped; a step feeds it the stream's first
n_s = min(max(count, 0), K) hops of the block, one block of n_s hops.  Rows
n_s .. K-1 of the output are NaN: "not written".
"""
import numpy as np

from vad_amd.resample import StreamModel

RATES = [8000, 16000, 44100, 48000]
HOP_OUT = 160


def hop_in_of(rate):
    return rate // 100


class SessionsResampleModel:
    def __init__(self, n_streams, rates, K, hop_out=HOP_OUT, taps=None):
        self.n, self.rates, self.K, self.hop_out = int(n_streams), list(rates), int(K), int(hop_out)
        self.taps = taps or {}
        self.rate = [0] * self.n          # the stored rate index: all-zero state is rate 0
        self.model = [self._fresh(0) for _ in range(self.n)]
        self.sessions = [[dict(rate=0, hops=[], rows=[])] for _ in range(self.n)]

    def _fresh(self, i):
        return StreamModel(1, self.rates[i], hop_out=self.hop_out, taps=self.taps.get(self.rates[i]))

    def step(self, x, counts, restart, rate_index):
        """x (K, S, hop_in_max); returns (K, S, hop_out) float64, NaN where nothing is written."""
        out = np.full((self.K, self.n, self.hop_out), np.nan)
        for s in range(self.n):
            n = int(min(max(int(counts[s]), 0), self.K))
            if restart[s]:
                self.rate[s] = int(min(max(int(rate_index[s]), 0), len(self.rates) - 1))
                self.model[s] = self._fresh(self.rate[s])
                self.sessions[s].append(dict(rate=self.rate[s], hops=[], rows=[]))
            if n == 0:
                continue
            m = self.model[s]
            hops = np.asarray(x[:n, s, :m.hop_in], np.float64)
            out[:n, s] = m.step(hops[:, None, :])[:, 0]
            self.sessions[s][-1]["hops"] += list(hops)
            self.sessions[s][-1]["rows"] += list(out[:n, s])
        return out


def script(S=6, K=3, blocks=12, seed=4, n_rates=4):
    """The workload of the GPU tests; the seed was chosen on the CPU
    (tests/test_resample_sessions_cpu.py asserts that every case named here
    occurs at it).  (B, S) int32 counts in -1 .. K + 1 (both clamps occur), (B, S) uint8
    restart flags, (B, S) int32 rate indices.  Every stream starts a session in
    block 0, restarts at a rate other than its last at least once, and stalls
    (count <= 0, no flag) at least once; a rate index is drawn afresh in every
    block, so most of those without a flag name another rate than the running
    one and must change nothing.  Stream 1 is restarted once with count 0;
    stream 2's restart indices are -1 and n_rates (clamped)."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(-1, K + 2, size=(blocks, S)).astype(np.int32)
    restart = np.zeros((blocks, S), np.uint8)
    rate = rng.integers(0, n_rates, size=(blocks, S)).astype(np.int32)
    cur = np.zeros(S, np.int64)
    for s in range(S):
        when = sorted({0, *rng.choice(np.arange(2, blocks), size=2, replace=False).tolist()})
        for b in when:
            restart[b, s] = 1
            if b == 0:
                cur[s] = rate[b, s]
                continue
            rate[b, s] = (cur[s] + 1 + rng.integers(0, n_rates - 1)) % n_rates  # another rate than the last
            cur[s] = rate[b, s]
        stall = int(rng.choice([b for b in range(1, blocks) if not restart[b, s]]))
        counts[stall, s] = int(rng.integers(-1, 1))
    b = int(np.flatnonzero(restart[1:, 1])[0]) + 1
    counts[b, 1] = 0
    for b, v in zip(np.flatnonzero(restart[1:, 2]) + 1, (-1, n_rates)):
        rate[b, 2] = v
    return counts, restart, rate


def session_rows(counts, restart, rate, n_rates, K):
    """Per stream its sessions in order, as dicts: ``rate`` (the clamped
    index), ``start`` (the block of the restart, -1 for the session a fresh
    state begins with) and ``rows``, the (block, k) pairs of the hops it took."""
    B, S = counts.shape
    out = [[dict(rate=0, start=-1, rows=[])] for _ in range(S)]
    for b in range(B):
        for s in range(S):
            if restart[b, s]:
                out[s].append(dict(rate=int(np.clip(rate[b, s], 0, n_rates - 1)), start=b, rows=[]))
            out[s][-1]["rows"] += [(b, k) for k in range(int(np.clip(counts[b, s], 0, K)))]
    return out


def audio(blocks, K, S, hop_in, seed=977):
    """(B, K, S, hop_in) integer-valued samples, exact as int16 and as fp32."""
    rng = np.random.default_rng(seed)
    return rng.integers(-20000, 20000, size=(blocks, K, S, hop_in)).astype(np.int16)
