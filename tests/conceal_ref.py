"""The loss concealment's law (include/conan_hip.h, conan_conceal_cfg) restated in numpy with Python integers, as a per-sample loop:
the lag search on the s16 view in int64, the template, the level of a run, the cross-fade back into received audio.  dec / enc are
tests/sample_format_ref.py's; the fused multiply-add is tests/bypass_ref.py's.  Everything is exact: the tests compare bits.

A Concealer keeps the state between calls, so the same class gives the whole-signal form (one call) and the streaming form (one call
per row, packets counted from the start of each row)."""
import numpy as np

from tests import sample_format_ref as SF
from tests.bypass_ref import fma32

F32, F64 = np.float32, np.float64
FULL = 1 << 20
MAX_LAG, MAX_WINDOW = 1024, 1024
FIELDS = ("packet", "lag_min", "lag_max", "window", "hold", "fall", "fade")


def defaults(rate):
    """The documented defaults for a rate."""
    r = int(rate)
    return dict(packet=r // 50, lag_min=r // 400, lag_max=r * 15 // 1000, window=r // 50, hold=r // 100, fall=r // 20, fade=r // 200)


def level(k, hold, fall):
    if k < hold:
        return FULL
    if k < hold + fall:
        return ((hold + fall - k) << 20) // fall
    return 0


def gain(l):
    return F32(F64(int(l)) / F64(FULL))


def search(y_hist, lag_min, lag_max, window):
    """The lag of a run that starts behind y_hist (its last window + lag_max values are read)."""
    q = SF.quantize(np.asarray(y_hist, dtype=F32)[-(window + lag_max):])      # int64
    n = len(q)
    a = q[n - window:]
    best, best_d = None, None
    for p in range(lag_min, lag_max + 1):
        d = a - q[n - window - p:n - p]
        dd = int(np.sum(d * d))
        if best is None or dd < best_d:
            best, best_d = p, dd
    return best


class Concealer:
    def __init__(self, fmt="f32", **cfg):
        for f in FIELDS:
            setattr(self, f, int(cfg[f]))
        assert self.packet >= 1 and 1 <= self.lag_min <= self.lag_max <= MAX_LAG and 1 <= self.window <= MAX_WINDOW
        assert self.hold >= 0 and self.fall >= 1 and 0 <= self.fade <= 1024
        self.fmt = fmt
        self.restart()

    def restart(self):
        self.mode, self.p, self.k, self.j = 0, 0, 0, 0
        self.T = np.zeros(0, dtype=F32)
        self.hist = np.zeros(self.window + self.lag_max, dtype=F32)      # y[t - H .. t - 1]

    def copy_state_from(self, other):
        self.mode, self.p, self.k, self.j = other.mode, other.p, other.k, other.j
        self.T, self.hist = other.T.copy(), other.hist.copy()

    def _put(self, out, y, b, t, v):
        code = SF.encode(np.asarray([v], dtype=F32), self.fmt)
        out[t] = code[0]
        y[b] = SF.decode(code, self.fmt)[0]

    def apply(self, row, lost):
        """row: [n] codes of self.fmt; lost: the flags of its packets, counted from the row's start -> (the repaired row, a bool mask
        of the samples that were written)."""
        row = np.asarray(row)
        n, H = len(row), len(self.hist)
        out, written = row.copy(), np.zeros(n, dtype=bool)
        y = np.concatenate([self.hist, np.zeros(n, dtype=F32)])
        dec = SF.decode(row, self.fmt)
        for t in range(n):
            b = H + t
            if lost[t // self.packet]:
                if self.mode != 1:
                    self.p = search(y[:b], self.lag_min, self.lag_max, self.window)
                    self.T = y[b - self.p:b].copy()
                    self.k, self.mode = 0, 1
                v = F32(self.T[self.k % self.p] * gain(level(self.k, self.hold, self.fall)))
                self._put(out, y, b, t, v)
                written[t] = True
                self.k += 1
                continue
            x = dec[t]
            if self.mode == 1:
                self.j = 0
                self.mode = 2 if self.fade > 0 else 0
            if self.mode == 2:
                l_in = ((self.j + 1) << 20) // (self.fade + 1)
                s = F32(self.T[self.k % self.p] * gain(level(self.k, self.hold, self.fall)))
                xin = F32(x * gain(l_in))
                v = fma32(np.asarray([s], dtype=F32), np.asarray([gain(FULL - l_in)], dtype=F32), np.asarray([xin], dtype=F32))[0]
                self._put(out, y, b, t, v)
                written[t] = True
                self.k += 1
                self.j += 1
                if self.j == self.fade:
                    self.mode = 0
            else:
                y[b] = x
        self.hist = y[len(y) - H:].copy()
        return out, written


def conceal(row, lost, fmt="f32", **cfg):
    """The law on a whole signal from the zero state -> the repaired row."""
    return Concealer(fmt, **cfg).apply(row, lost)[0]


def conceal_chunked(row, lost, cuts, fmt="f32", **cfg):
    """The same signal cut into rows at `cuts` (ascending sample positions); the flags of each row are those of its own packets."""
    c = Concealer(fmt, **cfg)
    out, lo = [], 0
    for hi in list(cuts) + [len(row)]:
        assert lo % c.packet == 0, "a cut off a packet boundary shifts the packets of the rows behind it"
        out.append(c.apply(row[lo:hi], lost[lo // c.packet:])[0])
        lo = hi
    return np.concatenate(out)
