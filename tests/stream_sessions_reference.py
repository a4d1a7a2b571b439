"""What a sessions StreamBatch must compute, from the plain hop kernels.

A schedule gives, per block and stream, a hop count and a restart bit
(StreamBatch(sessions=True): vad_amd/stream.py).  Stream s's hops, in order,
are split at its restarts into *sessions*; every session starts from a fresh
state, so it is one row of a plain ``StreamBatch(n_sessions, ...,
hops_per_step=1)`` -- a batch WITHOUT sessions, the kernels that were there
before -- fed that session's hops one step at a time (rows padded with zero
hops to the longest session; a row's values past its own end are not used).
Labels, scores and the state after each step are recorded per row and mapped
back to (block, row, stream).  Nothing here calls the sessions kernels.
"""
import numpy as np

NO_HOP = 254  # VAD_LABEL_NO_HOP, spelled out: the expected value does not come from the code under test
STATE = ("frames", "ring", "count")
DN_STATE = ("_spec", "_noise", "_est", "noise_count")


def make_schedule(S, K, n_blocks, seed):
    """counts (B, S) int32 as given to the kernel (unclamped) and restart
    (B, S) uint8.  S >= 7, n_blocks >= 10.  Forced streams:
      0  always K hops, never restarts
      1  never a hop, never restarts
      2  restarts in block 0
      3  restarts in a block in which its count is 0 (block 5), hops before it
      4  K hops per block and one restart in block 8: it has seen >= 7 hops
         (8 K), so the five warm-up rows of 255 reappear
      5  counts above K and below 0 (clamped), no restart
    the rest: counts uniform in 0..K, a restart with probability 0.15."""
    assert S >= 7 and n_blocks >= 10
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, K + 1, size=(n_blocks, S)).astype(np.int32)
    restart = (rng.random((n_blocks, S)) < 0.15).astype(np.uint8)
    counts[:, 0], restart[:, 0] = K, 0
    counts[:, 1], restart[:, 1] = 0, 0
    restart[0, 2] = 1
    counts[:5, 3], counts[5, 3], restart[5, 3] = K, 0, 1
    counts[:, 4], restart[:, 4] = K, 0
    restart[8, 4] = 1
    counts[:, 5] = np.where(np.arange(n_blocks) % 3 == 0, K + 3, np.where(np.arange(n_blocks) % 3 == 1, -2, K))
    restart[:, 5] = 0
    return counts, restart


def clamp(counts, K):
    return np.clip(counts, 0, K)


class Sessions:
    """The sessions of a schedule.  rows[i] is session i's list of (block,
    hop row, stream); at[b][s] = (session, hops the session has had before
    block b, hops in block b) AFTER block b's restart bit was applied."""

    def __init__(self, counts, restart, K):
        B, S = counts.shape
        n = clamp(counts, K)
        self.K, self.B, self.S = K, B, S
        self.rows, self.at = [], [[None] * S for _ in range(B)]
        for s in range(S):
            cur = None
            for b in range(B):
                if cur is None or restart[b, s]:
                    self.rows.append([])
                    cur = len(self.rows) - 1
                self.at[b][s] = (cur, len(self.rows[cur]), int(n[b, s]))
                self.rows[cur] += [(b, k, s) for k in range(int(n[b, s]))]
        self.longest = max(len(r) for r in self.rows)


class Expected:
    """Runs the plain batch and answers, for block b: label_block (K, S),
    score_block (K, S) or None, and the state tensors (S, ...) after it.

    make_plain(n_rows) builds the plain batch (hops_per_step=1, the options of
    the batch under test, no sessions); blocks: (B, K, S, hop) device tensor
    of its input dtype."""

    def __init__(self, torch, make_plain, blocks, counts, restart, K):
        self.torch = torch
        ses = self.ses = Sessions(counts, restart, K)
        R, T = len(ses.rows), ses.longest
        sb = make_plain(R)
        assert sb.K == 1 and not getattr(sb, "sessions", False)
        self.names = STATE + (DN_STATE if sb.denoise else ())
        H = blocks.shape[-1]
        feed = torch.zeros((max(T, 1), R, H), dtype=blocks.dtype, device=blocks.device)
        for i, row in enumerate(ses.rows):
            for t, (b, k, s) in enumerate(row):
                feed[t, i] = blocks[b, k, s]
        # snap[h]: every row's state after h hops (h = 0: a fresh stream)
        snap = [{k: getattr(sb, k).clone() for k in self.names}]
        assert not any(bool(v.any()) for v in snap[0].values())
        labels, scores = [], []
        for t in range(T):
            sb.step(feed[t])
            labels.append(sb.label_block[0].clone())
            if sb.scores:
                scores.append(sb.score_block[0].clone())
            snap.append({k: getattr(sb, k).clone() for k in self.names})
        self.snap, self.labels, self.scores = snap, labels, (scores if sb.scores else None)

    def block(self, b):
        torch, ses = self.torch, self.ses
        K, S = ses.K, ses.S
        dev = self.snap[0]["count"].device
        lab = torch.full((K, S), NO_HOP, dtype=torch.uint8, device=dev)
        sc = None if self.scores is None else torch.full((K, S), float("nan"), dtype=torch.float32, device=dev)
        state = {k: torch.empty((S,) + tuple(v.shape[1:]), dtype=v.dtype, device=dev)
                 for k, v in self.snap[0].items()}
        for s in range(S):
            i, h0, n = ses.at[b][s]
            for k in range(n):
                lab[k, s] = self.labels[h0 + k][i]
                if sc is not None:
                    sc[k, s] = self.scores[h0 + k][i]
            for name in self.names:
                state[name][s] = self.snap[h0 + n][name][i]
        return lab, sc, state
