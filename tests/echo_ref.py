"""The echo canceller's law (include/conan_hip.h, conan_echo_cfg) restated in numpy with int64 integers: the block-NLMS filter, the
guard, the Geigel detector with its hang-over, the idle test and the weight update.  Every sum is an exact integer (the header
states the bounds), so nothing here has a tolerance and the result does not depend on how a signal is cut into calls.  dec / enc are
tests/sample_format_ref.py's.

A Canceller keeps the state between calls, so the same class gives the whole-signal form (one call) and the streaming form (one
call per row); record() / from_record() are the state record of conan_streams_echo_state, byte for byte."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from tests import sample_format_ref as SF

F32, I64 = np.float32, np.int64
BLOCK, MAX_TAPS, MAX_DELAY, MAX_SHIFT = 64, 2048, 4096, 12
HIST = 6208      # far samples a record keeps: >= MAX_TAPS + BLOCK - 1 + MAX_DELAY, a multiple of 4
WMAX = (1 << 31) - 1
FIELDS = ("taps", "delay", "mu_shift", "dt_num", "dt_den", "hang", "reg", "far_min")
STATE_BYTES = 64 + 4 * MAX_TAPS + 4 * BLOCK + 2 * HIST


def defaults(rate):
    """The documented defaults for a rate."""
    r = int(rate)
    taps = min(MAX_TAPS, max(BLOCK, (r * 64 // 1000 + 32) // 64 * 64))
    return dict(taps=taps, delay=0, mu_shift=4, dt_num=1, dt_den=2, hang=(r // 20 + BLOCK - 1) // BLOCK, reg=taps * 4096, far_min=taps * 1024)


def q16(x):
    """The 16-bit view of f32 values; a non-finite value counts as 0."""
    x = np.asarray(x, dtype=F32)
    return SF.quantize(np.where(np.isfinite(x), x, F32(0)))


def trunc_div(a, b):
    """C's int64 division (toward zero) of an array by a positive integer."""
    return np.abs(a) // I64(b) * np.sign(a)


class Canceller:
    def __init__(self, fmt="f32", **cfg):
        self.fmt = fmt
        self.configure(**cfg)
        self.restart()

    def configure(self, **cfg):
        """The fields as the setter takes them; a live change keeps the state: the weights that still exist stay, the rest is zero."""
        for f in FIELDS:
            setattr(self, f, int(cfg[f]))
        assert self.taps % BLOCK == 0 and BLOCK <= self.taps <= MAX_TAPS and 0 <= self.delay <= MAX_DELAY and 0 <= self.mu_shift <= MAX_SHIFT
        assert self.dt_num >= 0 and self.dt_den >= 0 and self.hang >= 0 and self.reg >= 1 and self.far_min >= 0
        if hasattr(self, "w"):
            w = np.zeros(self.taps, dtype=I64)
            m = min(self.taps, len(self.w))
            w[:m] = self.w[:m]
            self.w = w

    def restart(self):
        self.w = np.zeros(self.taps, dtype=I64)
        self.hist = np.zeros(HIST, dtype=I64)      # x[pos - HIST .. pos - 1]
        self.e = []                                # the pending block's e
        self.D = self.E = self.dmax = 0
        self.pos, self.shift, self.hcnt = 0, self.mu_shift, 0
        self.adapted = self.frozen = self.trips = 0

    def record(self):
        head = np.array([self.pos], dtype="<i8").tobytes() + np.array([self.shift, self.hcnt], dtype="<i4").tobytes()
        head += np.array([self.adapted, self.frozen, self.trips, self.D, self.E], dtype="<i8").tobytes() + np.array([self.dmax, 0], dtype="<i4").tobytes()
        w = np.zeros(MAX_TAPS, dtype="<i4")
        w[:self.taps] = self.w
        e = np.zeros(BLOCK, dtype="<i4")
        e[:len(self.e)] = self.e
        out = head + w.tobytes() + e.tobytes() + self.hist.astype("<i2").tobytes()
        assert len(out) == STATE_BYTES
        return np.frombuffer(out, dtype=np.uint8).copy()

    def from_record(self, rec):
        """The state becomes the record's (a seed); the fields stay."""
        b = np.asarray(rec, dtype=np.uint8).tobytes()
        self.pos = int(np.frombuffer(b, "<i8", 1, 0)[0])
        self.shift, self.hcnt = (int(v) for v in np.frombuffer(b, "<i4", 2, 8))
        self.adapted, self.frozen, self.trips, self.D, self.E = (int(v) for v in np.frombuffer(b, "<i8", 5, 16))
        self.dmax = int(np.frombuffer(b, "<i4", 1, 56)[0])
        self.w = np.frombuffer(b, "<i4", MAX_TAPS, 64)[:self.taps].astype(I64)
        self.e = [int(v) for v in np.frombuffer(b, "<i4", BLOCK, 64 + 4 * MAX_TAPS)[:self.pos % BLOCK]]
        self.hist = np.frombuffer(b, "<i2", HIST, 64 + 4 * MAX_TAPS + 4 * BLOCK).astype(I64)

    def _block_end(self, xs, b1):
        """The end of the block whose last sample is row position b1 - 1; xs[HIST + u] = x[u] in row positions.  -> (adapted, frozen)"""
        L = self.taps
        e = np.asarray(self.e, dtype=I64)
        D, E, dmax = self.D, self.E, self.dmax
        self.e, self.D, self.E, self.dmax = [], 0, 0, 0
        if E > 4 * D + 4096:      # the guard: nothing else happens in this block
            self.w[:] = 0
            self.shift = min(self.shift + 1, MAX_SHIFT)
            self.trips += 1
            return 0, 0
        top = HIST + b1 - 1 - self.delay                      # x'[b1 - 1]
        win = xs[top - (L + BLOCK - 2):top + 1]               # x'[b0 - L + 1 .. b1 - 1]
        xmax = int(np.max(np.abs(win)))
        P = int(np.sum(win[BLOCK - 1:] ** 2))                 # x'[b1 - L .. b1 - 1]
        cond = self.dt_den > 0 and dmax * self.dt_den > xmax * self.dt_num
        frz = cond or self.hcnt > 0
        if cond:
            self.hcnt = self.hang
        elif self.hcnt > 0:
            self.hcnt -= 1
        if frz:
            self.frozen += 1
            return 0, 1
        if P < self.far_min:
            return 0, 0
        G = (sliding_window_view(win, BLOCK) @ e)[::-1]       # row j holds x'[b0 - L + 1 + j + i]: tap k = L - 1 - j
        step = trunc_div(G * I64(1 << (24 - self.shift)), P + self.reg)
        self.w = np.clip(self.w + step, -WMAX, WMAX)
        self.adapted += 1
        return 1, 0

    def apply(self, row, far):
        """row, far: [n] codes of self.fmt -> (the cancelled row, a bool mask of the samples that were written, the call's stats
        [sum d^2, sum e^2, blocks adapted, blocks frozen])."""
        row = np.asarray(row)
        n, L = len(row), self.taps
        out, written = row.copy(), np.zeros(n, dtype=bool)
        m = SF.decode(row, self.fmt)
        m = np.where(np.isfinite(m), m, F32(0)).astype(F32)
        d = SF.quantize(m)
        xs = np.concatenate([self.hist, q16(SF.decode(np.asarray(far), self.fmt))])
        stats = [0, 0, 0, 0]
        t = 0
        while t < n:
            ph = self.pos % BLOCK
            ln = min(n - t, BLOCK - ph)
            top = HIST + t - self.delay                                            # x'[t]
            win = sliding_window_view(xs[top - L + 1:top + ln], L)                # row i: x'[t + i - L + 1 .. t + i]
            S = win @ self.w[::-1]
            y = np.clip((S + (1 << 23)) >> 24, -32768, 32767)
            e = d[t:t + ln] - y
            nz = np.nonzero(y)[0]
            if len(nz):
                v = (m[t + nz] - y[nz].astype(F32) * F32(2.0 ** -15)).astype(F32)      # one f32 subtraction; the product is exact
                out[t + nz] = SF.encode(v, self.fmt)
                written[t + nz] = True
            self.e += [int(v) for v in e]
            dd, ee = int(np.sum(d[t:t + ln] ** 2)), int(np.sum(e ** 2))
            self.D += dd
            self.E += ee
            self.dmax = max(self.dmax, int(np.max(np.abs(d[t:t + ln]))))
            stats[0] += dd
            stats[1] += ee
            self.pos += ln
            t += ln
            if self.pos % BLOCK == 0:
                a, f = self._block_end(xs, t)
                stats[2] += a
                stats[3] += f
        self.hist = xs[len(xs) - HIST:].copy()
        return out, written, stats


def cancel(row, far, fmt="f32", **cfg):
    """The law on a whole signal from the zero state -> (the cancelled row, the stats, the canceller)."""
    c = Canceller(fmt, **cfg)
    out, _, stats = c.apply(row, far)
    return out, stats, c


def cancel_chunked(row, far, cuts, fmt="f32", **cfg):
    """The same signal cut into calls at `cuts` (ascending sample positions) -> (the row, the summed stats, the canceller)."""
    c = Canceller(fmt, **cfg)
    out, total, lo = [], [0, 0, 0, 0], 0
    for hi in list(cuts) + [len(row)]:
        o, _, st = c.apply(row[lo:hi], far[lo:hi])
        out.append(o)
        total = [a + b for a, b in zip(total, st)]
        lo = hi
    return np.concatenate(out), total, c


def erle_db(D, E):
    """10 log10(sum d^2 / sum e^2)."""
    return 10.0 * np.log10(max(float(D), 1e-30) / max(float(E), 1e-30))
