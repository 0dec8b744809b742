"""The echo-delay estimator's law (include/conan_hip.h, conan_echo_delay_cfg) restated in numpy with Python / int64 integers: ternary
signs of the canceller's 16-bit views, a leaky cross-correlation over n_lags lags, and at every frame end the peak test, the
confirmation counter and the leak.  Every sum is an exact integer and the leak and the decision happen only at fixed multiples of
FRAME, so nothing here has a tolerance and the result does not depend on how a signal is cut into calls.  dec is
tests/sample_format_ref.py's, q16 tests/echo_ref.py's.

An Estimator keeps the state between calls, so the same class gives the whole-signal form (one call) and the streaming form (one
call per row); record() / from_record() are the state record of conan_streams_echo_delay_state, byte for byte.  follow() is the
host rule the engine applies between calls (conan_amd._lib.echo_delay_follow)."""
import numpy as np

from tests import sample_format_ref as SF
from tests.echo_ref import MAX_DELAY, q16

I64 = np.int64
FRAME, MAX_LAGS = 1024, 6144
AGE_MAX = (1 << 31) - 1
FIELDS = ("n_lags", "thr", "leak", "ratio", "min_peak", "hold", "tol")
REPORT = ("est", "age", "cand", "run", "last_pk", "last_s")
STATE_BYTES = 64 + 4 * MAX_LAGS + MAX_LAGS


def defaults(rate):
    """The documented defaults for a rate.  Choices, not measurements."""
    r = int(rate)
    n_lags = min(MAX_LAGS, max(64, (r * 384 // 1000 + 32) // 64 * 64))
    return dict(n_lags=n_lags, thr=16, leak=5, ratio=10, min_peak=1024, hold=4, tol=r * 2 // 1000)


def sgn(v, thr):
    """The ternary sign of 16-bit values."""
    v = np.asarray(v, dtype=I64)
    return (v >= thr).astype(I64) - (v <= -thr).astype(I64)


class Estimator:
    def __init__(self, fmt="f32", **cfg):
        self.fmt = fmt
        self.configure(**cfg)
        self.restart()

    def configure(self, **cfg):
        """The fields as the setter takes them; a live change keeps the state: A[l] stays for l below both n_lags, the rest is zero."""
        for f in FIELDS:
            setattr(self, f, int(cfg[f]))
        assert self.n_lags % 64 == 0 and 64 <= self.n_lags <= MAX_LAGS and 1 <= self.thr <= 32767 and 1 <= self.leak <= 8
        assert self.ratio >= 1 and self.min_peak >= 1 and self.hold >= 1 and self.tol >= 0
        if hasattr(self, "A"):
            self.A[self.n_lags:] = 0

    def restart(self):
        self.A = np.zeros(MAX_LAGS, dtype=I64)        # zeros from n_lags on, always
        self.hist = np.zeros(MAX_LAGS, dtype=I64)     # sgn(x[pos - MAX_LAGS .. pos - 1]); the law reads the last MAX_LAGS - 1
        self.pos = self.age = self.run = self.frames = self.last_pk = self.last_s = 0
        self.est = self.cand = -1

    def report(self):
        return [int(getattr(self, f)) for f in REPORT]

    def record(self):
        head = np.array([self.pos], dtype="<i8").tobytes() + np.array([self.est, self.age, self.cand, self.run], dtype="<i4").tobytes()
        head += np.array([self.frames, self.last_pk, self.last_s], dtype="<i8").tobytes() + bytes(16)
        h = self.hist.astype("i1")
        h[0] = 0      # (the record keeps the last MAX_LAGS - 1 values behind one zero byte)
        out = head + self.A.astype("<i4").tobytes() + h.tobytes()
        assert len(out) == STATE_BYTES
        return np.frombuffer(out, dtype=np.uint8).copy()

    def from_record(self, rec):
        """The state becomes the record's (a seed); the fields stay."""
        b = np.asarray(rec, dtype=np.uint8).tobytes()
        self.pos = int(np.frombuffer(b, "<i8", 1, 0)[0])
        self.est, self.age, self.cand, self.run = (int(v) for v in np.frombuffer(b, "<i4", 4, 8))
        self.frames, self.last_pk, self.last_s = (int(v) for v in np.frombuffer(b, "<i8", 3, 24))
        self.A = np.frombuffer(b, "<i4", MAX_LAGS, 64).astype(I64)
        self.A[self.n_lags:] = 0
        self.hist = np.frombuffer(b, "i1", MAX_LAGS, 64 + 4 * MAX_LAGS).astype(I64)

    def _frame_end(self):
        n = self.n_lags
        a = np.abs(self.A[:n])
        p = int(np.argmax(a))      # the smallest l that maximises a
        pk, s = int(a[p]), int(np.sum(a))
        ok = pk >= self.min_peak and pk * n > self.ratio * s      # Python integers: no width to overflow
        if ok and self.cand >= 0 and abs(p - self.cand) <= self.tol:
            self.run += 1
        elif ok:
            self.run = 1
        else:
            self.run = 0
        self.cand = p if ok else -1
        if self.run >= self.hold:
            self.est, self.age = p, 0
        elif self.est >= 0:
            self.age = min(self.age + 1, AGE_MAX)
        self.frames += 1
        self.last_pk, self.last_s = pk, s
        self.A[:n] -= self.A[:n] >> self.leak      # arithmetic: floors

    def apply(self, mic, far):
        """mic, far: [n] codes of self.fmt (both are only read) -> (the report after each frame end of this call [frames, 6], the
        report after the call)."""
        n, L = len(mic), self.n_lags
        sd = sgn(q16(SF.decode(np.asarray(mic), self.fmt)), self.thr)
        xs = np.concatenate([self.hist, sgn(q16(SF.decode(np.asarray(far), self.fmt)), self.thr)])
        track, t = [], 0
        while t < n:
            ln = min(n - t, FRAME - self.pos % FRAME)
            seg = sd[t:t + ln]
            if np.any(seg):
                win = xs[MAX_LAGS + t - (L - 1):MAX_LAGS + t + ln]      # x[t - L + 1 .. t + ln - 1]
                # c[k] = sum over i of win[k + i] * seg[i] = the sum for lag L - 1 - k; float64 holds these integers (<= 1024) exactly
                c = np.correlate(win.astype(np.float64), seg.astype(np.float64), "valid")
                self.A[:L] += np.rint(c[::-1]).astype(I64)
            self.pos += ln
            t += ln
            if self.pos % FRAME == 0:
                self._frame_end()
                track.append(self.report())
        self.hist = xs[len(xs) - MAX_LAGS:].copy()
        return np.asarray(track, dtype=I64).reshape(-1, 6), self.report()


def estimate(mic, far, fmt="f32", **cfg):
    """The law on a whole signal from the zero state -> (track [frames, 6], report, the estimator)."""
    e = Estimator(fmt, **cfg)
    track, rep = e.apply(mic, far)
    return track, rep, e


def estimate_chunked(mic, far, cuts, fmt="f32", **cfg):
    """The same signal cut into calls at `cuts` (ascending sample positions) -> (track, report, the estimator)."""
    e = Estimator(fmt, **cfg)
    tracks, lo, rep = [], 0, e.report()
    for hi in list(cuts) + [len(mic)]:
        tr, rep = e.apply(mic[lo:hi], far[lo:hi])
        tracks.append(tr)
        lo = hi
    return np.concatenate(tracks), rep, e


def follow(est, age, in_force, lead, hyst, max_age):
    """The host rule between calls: the canceller's new bulk delay, or None to leave it."""
    if est < 0 or age > max_age:
        return None
    target = min(max(est - lead, 0), MAX_DELAY)
    return target if abs(target - in_force) > hyst else None
