"""NumPy restatement of the SimpleAnalyser state step over feature rows,
written from realtime_analysis/simple_analyzer.py:78-112 (feed_frame),
:144-164 (_classify_frame and its four tests), :245-256 (_add_inactive_frame)
and the threshold updates :261-327.  A helper for the simple-stream tests:
it calls nothing of vad_amd.

A row is [stEnergy, zcr * n, std|fft|, band 0..3].  The noise buffer keeps
[energy, std, band 0..3] of its frames (what the reference recomputes from
the stored frames on every update).
"""
import numpy as np

STATUS = 20
ACTIVE_RUN = 5
INACTIVE_RUN = 15
P = 0.25


class RefStream:
    def __init__(self, noise_buf_len):
        self.nb = int(noise_buf_len)
        self.noise = np.zeros((self.nb, 6), np.float64)
        self.energy_thresh = np.float64(0.0)
        self.std_thresh = np.float64(0.0)
        self.bands_thresh = np.zeros(4, np.float64)
        self.status = [False] * STATUS          # oldest first
        self.silence = True
        self.noise_pointer = 0
        self.frame_number = 0

    # -- the three means (:269-314, :362-384) -------------------------------------
    def _energy_mean(self):
        # energies stored in a uint32 array (:309): truncated toward zero;
        # integer sums below 2^53, so the order is free
        return np.float64(int(sum(int(e) for e in self.noise[:, 0]))) / np.float64(self.nb)

    def _std_mean(self):
        s = np.float64(self.noise[0, 1])
        for i in range(1, self.nb):
            s = s + self.noise[i, 1]
        return s / np.float64(self.nb)

    def _bands_mean(self):
        s = self.noise[0, 2:].copy()
        for i in range(1, self.nb):
            s = s + self.noise[i, 2:]
        return s / np.float64(self.nb)

    def init(self, rows):
        """load_init_inactive_frames (:120-138) from the init frames' rows."""
        rows = np.asarray(rows, np.float64)
        assert rows.shape == (self.nb, 7)
        self.noise[:] = rows[:, [0, 2, 3, 4, 5, 6]]
        self.energy_thresh = self._energy_mean()
        self.bands_thresh = self._bands_mean()
        self.std_thresh = self._std_mean()
        self.status = [False] * STATUS
        self.silence = True
        self.noise_pointer = 0
        self.frame_number = 0
        return self

    def _classify(self, f):
        zcr = 20 >= f[1] >= 5
        spec = False
        if f[3] > self.bands_thresh[0] * 3.0:
            spec = sum(1 for i in range(1, 4) if f[3 + i] > self.bands_thresh[i] * 3.0) >= 2
        if spec and zcr:
            return True
        return bool(zcr and f[0] > 2.0 * self.energy_thresh and f[2] > self.std_thresh * 2.0)

    def _add_inactive(self, f):
        self.noise[self.noise_pointer] = [f[0], f[2], f[3], f[4], f[5], f[6]]
        self.energy_thresh = (1 - P) * self.energy_thresh + P * self._energy_mean()
        self.bands_thresh = (1 - P) * self.bands_thresh + P * self._bands_mean()
        self.std_thresh = (1 - P) * self.std_thresh + P * self._std_mean()
        self.noise_pointer = 0 if self.noise_pointer == self.nb - 1 else self.noise_pointer + 1

    def step(self, f):
        f = np.asarray(f, np.float64)
        self.frame_number += 1
        status = self._classify(f)
        self.status = self.status[1:] + [status]
        active = sum(self.status)
        if status:
            if self.silence and active >= ACTIVE_RUN:
                self.silence = False
            return True
        if self.silence:
            self._add_inactive(f)
            return False
        if STATUS - active >= INACTIVE_RUN:
            self._add_inactive(f)
            self.silence = True
        return True

    def thresholds(self):
        return np.concatenate([[self.energy_thresh, self.std_thresh], self.bands_thresh])

    def packed(self):
        """The device state of this stream as 8-byte words (include/vad_amd.h)."""
        out = np.zeros(6 * self.nb + 8, np.float64)
        out[:6 * self.nb] = self.noise.reshape(-1)
        out[6 * self.nb:6 * self.nb + 6] = self.thresholds()
        bits = 0
        for s in self.status:
            bits = (bits << 1) | int(s)
        out.view(np.int32)[2 * (6 * self.nb + 6):] = (bits, int(self.silence), self.noise_pointer, self.frame_number)
        return out


def run(rows, init_rows, noise_buf_len):
    """(labels, RefStream) after init on init_rows and one step per row."""
    st = RefStream(noise_buf_len).init(init_rows)
    return np.array([st.step(r) for r in rows], np.uint8), st


# Hand-made rows for the edges of the step, over init rows whose thresholds
# are easy: energy 10 (7.9 and friends truncate), std 1, bands 1.
def edge_init(nb):
    rows = np.zeros((nb, 7), np.float64)
    rows[:, 0] = 10.0
    rows[:, 1] = 10.0
    rows[:, 2] = 1.0
    rows[:, 3:] = 1.0
    return rows


def row(energy=0.0, zcr=10.0, std=0.0, bands=(0.0, 0.0, 0.0, 0.0)):
    return np.array([energy, zcr, std, *bands], np.float64)


ACTIVE = dict(energy=1e6, std=1e6, bands=(1e6, 1e6, 1e6, 1e6))
QUIET = dict(energy=7.9, zcr=0.0, std=0.5, bands=(0.5, 0.25, 0.125, 0.75))


def edge_sequences():
    """name -> rows, all of one length (padded with quiet rows): the edges of
    the step over edge_init thresholds (energy 10, std 1, bands 1)."""
    act, quiet = row(**ACTIVE), row(**QUIET)
    up = float(np.nextafter(3.0, 4.0))
    seqs = {
        "zcr_5": [row(zcr=5.0, **ACTIVE)],
        "zcr_20": [row(zcr=20.0, **ACTIVE)],
        "zcr_4.999": [row(zcr=4.999, **ACTIVE)],
        "zcr_20.001": [row(zcr=20.001, **ACTIVE)],
        "bands_equal": [row(energy=0.0, std=0.0, bands=(3.0, 3.0, 3.0, 3.0))],
        "bands_above": [row(energy=0.0, std=0.0, bands=(up, up, 0.0, up))],
        "band0_equal": [row(energy=0.0, std=0.0, bands=(3.0, up, up, up))],
        "energy_equal": [row(energy=20.0, std=1e6)],
        "std_equal": [row(energy=1e6, std=2.0)],
        "second_path": [row(energy=float(np.nextafter(20.0, 21.0)), std=float(np.nextafter(2.0, 3.0)))],
        "truncation": [quiet],
        "silence_off": [act] * 6,
        "silence_on": [act] * 20 + [quiet] * 17,
        "wrap": [row(energy=float(i) + 0.9, zcr=0.0, std=0.5 + i / 16, bands=(0.5, 0.25 * i, 0.125, 0.75))
                 for i in range(9)],
    }
    n = max(len(v) for v in seqs.values())
    return {k: np.array(v + [quiet] * (n - len(v))) for k, v in seqs.items()}
