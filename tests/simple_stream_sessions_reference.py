"""NumPy restatement of SimpleStreamBatch(sessions=True) over feature rows:
one simple_stream_reference.RefStream per stream and session, driven over a
schedule of (rows, counts, restarts).  A helper for the sessions tests: it
calls nothing of vad_amd.

The rules (vad_amd/simple_stream.py's docstring), spelled out here so that the
expected values do not come from the code under test:
  * stream s takes n_s = min(max(counts[s], 0), k) rows of its column of a
    k-row block, rows 0..n_s-1; label rows n_s..k-1 hold 254;
  * a nonzero restart makes the stream fresh before those rows: its record
    all zero, init_left = noise_buf_len;
  * a fresh stream's next noise_buf_len rows, whichever blocks they come in,
    are its init rows, labelled 253; with the last one the stream is
    RefStream(nb).init(those rows); the rows after it are stepped;
  * voiced: the block's row indices labelled 1, in order;
  * no row and no restart: nothing of the stream changes.
"""
import numpy as np

from simple_stream_reference import RefStream

INIT = 253    # VAD_LABEL_INIT
NO_HOP = 254  # VAD_LABEL_NO_HOP


class RefSessions:
    def __init__(self, n_streams, noise_buf_len):
        self.n, self.nb = int(n_streams), int(noise_buf_len)
        self.streams = [None] * self.n               # the RefStream of an initialised stream
        self.init_rows = [[] for _ in range(self.n)]  # the init rows a fresh stream has so far
        self.sessions = [0] * self.n                  # restarts seen, per stream

    def init_left(self, s):
        return 0 if self.streams[s] is not None else self.nb - len(self.init_rows[s])

    def load(self, s, init_rows):
        """load_init_inactive_frames for stream s."""
        self.streams[s] = RefStream(self.nb).init(init_rows)
        self.init_rows[s] = []

    def packed(self, s):
        """Stream s's device record: of a stream still in init, its noise rows
        so far and zeros."""
        if self.streams[s] is not None:
            return self.streams[s].packed()
        out = np.zeros(6 * self.nb + 8, np.float64)
        for i, r in enumerate(self.init_rows[s]):
            out[6 * i:6 * i + 6] = np.asarray(r, np.float64)[[0, 2, 3, 4, 5, 6]]
        return out

    def block(self, rows, counts, restarts):
        """rows (k, S, 7); returns labels (k, S) uint8 and per stream the list
        of the block's row indices labelled 1."""
        rows = np.asarray(rows, np.float64)
        k = rows.shape[0]
        labels = np.full((k, self.n), NO_HOP, np.uint8)
        voiced = [[] for _ in range(self.n)]
        for s in range(self.n):
            if restarts[s]:
                self.streams[s], self.init_rows[s] = None, []
                self.sessions[s] += 1
            n_s = min(max(int(counts[s]), 0), k)
            for i in range(n_s):
                if self.streams[s] is None:
                    self.init_rows[s].append(rows[i, s].copy())
                    labels[i, s] = INIT
                    if len(self.init_rows[s]) == self.nb:
                        self.load(s, np.stack(self.init_rows[s]))
                else:
                    labels[i, s] = int(self.streams[s].step(rows[i, s]))
                    if labels[i, s] == 1:
                        voiced[s].append(i)
        return labels, voiced


def run(schedule, n_streams, noise_buf_len):
    """schedule: (rows, counts, restarts) per block.  Returns the label blocks,
    the voiced index lists per block, and the RefSessions after the last."""
    ref = RefSessions(n_streams, noise_buf_len)
    labs, voiced = [], []
    for rows, counts, restarts in schedule:
        lab, v = ref.block(rows, counts, restarts)
        labs.append(lab)
        voiced.append(v)
    return labs, voiced, ref
