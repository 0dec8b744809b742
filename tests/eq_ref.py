"""The equaliser's law (include/conan_hip.h, conan_eq_cfg) restated in float64 scalars: the sections, the segment grid, the pending
tail, the non-finite rule and the list of live changes.  Python floats are IEEE doubles and Python never fuses a product into a sum,
so every operation below is the single rounded one the law names and the library's bits can be compared with `==`.  Also the state
record's bytes and a numpy restatement of the design formulas (which are not part of the bit-exact law)."""
import math
import struct

import numpy as np

SEG = 128
MAX_SECTIONS = 4
MAX_COEF = 65536.0
MAX_CALL = 15 * SEG
KINDS = ("lowpass", "highpass", "bandpass", "notch", "peak", "lowshelf", "highshelf", "dcblock", "deemphasis")


def step(c, s0, s1, x):
    """One step of section c = (b0, b1, b2, a1, a2) from state (s0, s1) -> (y, s0', s1')."""
    b0, b1, b2, a1, a2 = c
    y = b0 * x + s0
    n0 = (b1 * x - a1 * y) + s1
    n1 = b2 * x - a2 * y
    return y, n0, n1


def transition(c):
    """The 2x2 transition matrix of SEG zero inputs, row-major (M00, M01, M10, M11): the step applied to the two unit states."""
    cols = []
    for s0, s1 in ((1.0, 0.0), (0.0, 1.0)):
        for _ in range(SEG):
            _, s0, s1 = step(c, s0, s1, 0.0)
        cols.append((s0, s1))
    return (cols[0][0], cols[1][0], cols[0][1], cols[1][1])


def sanitize(x):
    """The f32 samples as the law reads them: a non-finite sample counts as 0."""
    x = np.asarray(x, dtype=np.float32)
    return np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float32)


def stable(c):
    return abs(c[4]) < 1.0 and abs(c[3]) < 1.0 + c[4]


class Stream:
    """One row's filter: push(samples) emits every sample it is given, whatever the cut."""

    def __init__(self, sections, origin=0):
        self.origin = self.pos = int(origin)
        self.carry = [(0.0, 0.0)] * MAX_SECTIONS
        self.tail = []
        self._set(sections)

    def _set(self, sections):
        self.sections = [tuple(float(v) for v in c) for c in sections]
        assert 1 <= len(self.sections) <= MAX_SECTIONS
        self.M = [transition(c) for c in self.sections]

    def push(self, x, f64=False):
        """len(x) samples -> their outputs, float32 (f64=True: the last section's float64 outputs before the rounding)."""
        new = [float(v) for v in sanitize(x)]
        t = len(self.tail)
        raw = self.tail + new
        buf = list(raw)
        total = len(buf)
        nseg, rem = divmod(total, SEG)
        for k, c in enumerate(self.sections):
            M = self.M[k]
            c0, c1 = self.carry[k]
            starts = []
            for j in range(nseg):      # the zero-state run of each complete segment, and the scan
                e0 = e1 = 0.0
                for v in buf[j * SEG:(j + 1) * SEG]:
                    _, e0, e1 = step(c, e0, e1, v)
                starts.append((c0, c1))
                c0, c1 = (M[0] * c0 + M[1] * c1) + e0, (M[2] * c0 + M[3] * c1) + e1
            starts.append((c0, c1))
            self.carry[k] = (c0, c1)
            for j in range(nseg + (1 if rem else 0)):      # every sample by the direct recursion from its segment's start state
                s0, s1 = starts[j]
                for i in range(j * SEG, min((j + 1) * SEG, total)):
                    buf[i], s0, s1 = step(c, s0, s1, buf[i])
        self.tail = raw[nseg * SEG:]
        self.pos += len(new)
        out = np.asarray(buf[t:], dtype=np.float64)
        return out if f64 else out.astype(np.float32)

    def change(self, sections):
        """A live change at the current position: the pending tail is closed with the OLD coefficients (the carries advance over it by
        the direct recursion through the cascade), the origin moves here, section k keeps its two state words for k below both
        section counts and new sections start at zero."""
        buf = list(self.tail)
        for k, c in enumerate(self.sections):
            s0, s1 = self.carry[k]
            for i in range(len(buf)):
                buf[i], s0, s1 = step(c, s0, s1, buf[i])
            self.carry[k] = (s0, s1)
        keep = min(len(self.sections), len(sections))
        self.carry = self.carry[:keep] + [(0.0, 0.0)] * (MAX_SECTIONS - keep)
        self.tail = []
        self.origin = self.pos
        self._set(sections)

    def state_bytes(self):
        """conan_eq_state as the library reports it: zeros behind the last section's carries and behind the tail's entries."""
        carry = [v for k in range(MAX_SECTIONS) for v in (self.carry[k] if k < len(self.sections) else (0.0, 0.0))]
        tail = list(self.tail) + [0.0] * (SEG - len(self.tail))
        return struct.pack("<qq8d%df" % SEG, self.origin, self.pos, *carry, *tail)


STATE_BYTES = 16 + 8 * 2 * MAX_SECTIONS + 4 * SEG


def run(x, sections, cuts=None, changes=(), origin=0, f64=False):
    """x through the cascade.  cuts: the call lengths, cycled (None: one call); changes: [(position, sections)] - a change takes effect
    in front of the sample at that position (positions count from `origin`) -> (y, the Stream behind the last sample)."""
    x = np.asarray(x, dtype=np.float32)
    s = Stream(sections, origin)
    pending = sorted(((int(p), sec) for p, sec in changes), key=lambda t: t[0])
    out, i, k = [], 0, 0
    while i < len(x) or (pending and pending[0][0] <= s.pos):
        while pending and pending[0][0] <= s.pos:
            s.change(pending.pop(0)[1])
        if i >= len(x):
            break
        m = len(x) - i if cuts is None else min(int(cuts[k % len(cuts)]), len(x) - i)
        if pending:
            m = min(m, pending[0][0] - s.pos)
        out.append(s.push(x[i:i + m], f64))
        i += m
        k += 1
    y = np.concatenate(out) if out else np.zeros(0, dtype=np.float64 if f64 else np.float32)
    return y, s


def direct(x, sections):
    """The plain recursion over the whole signal, no segments: float64.  Not the law - the yardstick for what the segmenting costs."""
    buf = [float(v) for v in sanitize(x)]
    for c in sections:
        s0 = s1 = 0.0
        for i in range(len(buf)):
            buf[i], s0, s1 = step(c, s0, s1, buf[i])
    return np.asarray(buf, dtype=np.float64)


def cookbook(kind, rate, f0, q=math.sqrt(0.5), gain_db=0.0):
    """The Audio EQ Cookbook's section (and the two first-order ones) in numpy float64 -> (b0, b1, b2, a1, a2) / a0."""
    w0 = np.float64(2.0 * np.pi) * (np.float64(f0) / np.float64(rate))
    cw, sw = np.cos(w0), np.sin(w0)
    alpha = sw / (2.0 * np.float64(q))
    A = np.power(np.float64(10.0), np.float64(gain_db) / 40.0)
    one = np.float64(1.0)
    if kind == "lowpass":
        b, a = ((one - cw) / 2, one - cw, (one - cw) / 2), (one + alpha, -2 * cw, one - alpha)
    elif kind == "highpass":
        b, a = ((one + cw) / 2, -(one + cw), (one + cw) / 2), (one + alpha, -2 * cw, one - alpha)
    elif kind == "bandpass":
        b, a = (alpha, 0.0, -alpha), (one + alpha, -2 * cw, one - alpha)
    elif kind == "notch":
        b, a = (one, -2 * cw, one), (one + alpha, -2 * cw, one - alpha)
    elif kind == "peak":
        b, a = (one + alpha * A, -2 * cw, one - alpha * A), (one + alpha / A, -2 * cw, one - alpha / A)
    elif kind == "lowshelf":
        r = 2 * np.sqrt(A) * alpha
        b = (A * ((A + 1) - (A - 1) * cw + r), 2 * A * ((A - 1) - (A + 1) * cw), A * ((A + 1) - (A - 1) * cw - r))
        a = ((A + 1) + (A - 1) * cw + r, -2 * ((A - 1) + (A + 1) * cw), (A + 1) + (A - 1) * cw - r)
    elif kind == "highshelf":
        r = 2 * np.sqrt(A) * alpha
        b = (A * ((A + 1) + (A - 1) * cw + r), -2 * A * ((A - 1) + (A + 1) * cw), A * ((A + 1) + (A - 1) * cw - r))
        a = ((A + 1) - (A - 1) * cw + r, 2 * ((A - 1) - (A + 1) * cw), (A + 1) - (A - 1) * cw - r)
    elif kind == "dcblock":
        R = np.exp(-w0)
        g = (one + R) / 2
        b, a = (g, -g, 0.0), (one, -R, 0.0)
    elif kind == "deemphasis":
        p = np.exp(-w0)
        b, a = (one - p, 0.0, 0.0), (one, -p, 0.0)
    else:
        raise ValueError(kind)
    return tuple(float(np.float64(v) / a[0]) for v in (b[0], b[1], b[2], a[1], a[2]))


def response(sections, f, rate):
    """|H(e^{jw})| of the cascade at f Hz."""
    z = np.exp(-1j * 2.0 * np.pi * f / rate)
    h = 1.0 + 0.0j
    for b0, b1, b2, a1, a2 in sections:
        h *= (b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z)
    return abs(h)


# the issue's cascade at 16 kHz: high-pass 80 Hz, notch 50 Hz Q 30, peak +6 dB at 2.5 kHz, low-pass 3.4 kHz - a choice, not a preset
# anybody has listened to
def cascade4(rate=16000.0):
    return [cookbook("highpass", rate, 80.0), cookbook("notch", rate, 50.0, 30.0), cookbook("peak", rate, 2500.0, 1.0, 6.0),
            cookbook("lowpass", rate, 3400.0)]


def signal(n, seed=0, rate=16000.0):
    """Noise-like speech stand-in with a 0.2 DC offset and 50 Hz hum, float32."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    x = 0.2 + 0.1 * np.sin(2 * np.pi * 50.0 * t) + 0.3 * np.sin(2 * np.pi * 440.0 * t + 0.3) + 0.1 * rng.standard_normal(n)
    return x.astype(np.float32)
