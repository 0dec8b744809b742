"""The drift resampler's law (include/conan_hip.h, conan_resample_drift) restated in numpy: step, schedule, positions, length and
readiness in Python integers; the f32 sum with bypass_ref.fma32.  The f32 table T [1025][2W] is an argument: the tests hand over the
library's (conan_resample_drift_table), so the last bit of libm stays out of the bit comparisons; kernel64 / table64 evaluate the same
kernel in float64 for the table's own check and for the exact-position quality measurement."""
import math

import numpy as np

from tests.bypass_ref import fma32

F32, F64 = np.float32, np.float64
SOURCE, SINK = 0, 1
PHASES, FRAC_BITS = 1024, 22
MAX_PPB = 2000000
G = 10 ** 9
KAISER_BEST_BETA = 14.769656459379492


def ppb_of(ppm):
    return int(round(float(ppm) * 1000))


def step(in_rate, out_rate, side, ppb):
    assert side in (SOURCE, SINK) and abs(int(ppb)) <= MAX_PPB
    if side == SOURCE:
        return ((int(in_rate) * (G + int(ppb))) << 32) // (int(out_rate) * G)
    return ((int(in_rate) * G) << 32) // (int(out_rate) * (G + int(ppb)))


def width(in_rate, out_rate, lpw=6, rolloff=0.99):
    """(W, base / in_rate); rolloff is the library's f32."""
    base = float(min(in_rate, out_rate)) * float(F32(rolloff))
    return int(math.ceil(lpw * float(in_rate) / base)), base / in_rate


def segments(in_rate, out_rate, side, schedule):
    """schedule [(at, ppb)] -> [(at, pos of output at, step)]: output at[k] is the first one at step k."""
    assert schedule[0][0] == 0
    out = []
    for k, (at, ppb) in enumerate(schedule):
        st = step(in_rate, out_rate, side, ppb)
        if k == 0:
            out.append((0, 0, st))
        else:
            pa, pp, ps = out[-1]
            assert at > pa
            out.append((int(at), pp + (int(at) - 1 - pa) * ps + st, st))
    return out


def length(in_rate, out_rate, side, schedule, samples):
    """Outputs j with pos_j >> 32 < samples."""
    seg = segments(in_rate, out_rate, side, schedule)
    end = int(samples) << 32
    for k, (at, pos, st) in enumerate(seg):
        if pos >= end:
            return at
        cnt = (end - pos + st - 1) // st
        if k + 1 == len(seg) or cnt < seg[k + 1][0] - at:
            return at + cnt
    return 0


def ready(in_rate, out_rate, side, schedule, received, W):
    """Outputs j with n_j + W < received: the stream's ready count once `received` inputs have arrived."""
    return length(in_rate, out_rate, side, schedule, max(0, int(received) - W))


def positions(in_rate, out_rate, side, schedule, count):
    """pos_j, j < count, as a list of Python ints (by the recurrence, not the closed form)."""
    steps = {int(at): step(in_rate, out_rate, side, ppb) for at, ppb in schedule}
    pos, cur, out = 0, steps[0], []
    for j in range(count):
        cur = steps.get(j, cur)
        if j:
            pos += cur
        out.append(pos)
    return out


def bessel_i0(x):
    s, term, h = 1.0, 1.0, 0.25 * x * x
    for k in range(1, 500):
        term *= h / (float(k) * k)
        s += term
        if term < s * 1e-17:
            break
    return s


def kernel64(d, in_rate, out_rate, lpw=6, rolloff=0.99, window="hann", beta=None):
    """The configuration's kernel in float64 at tap distances d (input samples from the output's position, any real values)."""
    W, scale = width(in_rate, out_rate, lpw, rolloff)
    t = np.asarray(d, dtype=F64) * scale
    inside = np.abs(t) < lpw
    ts = np.where(inside, t, 0.0)
    if window == "hann":
        win = np.cos(ts * math.pi / lpw / 2) ** 2
    else:
        b = KAISER_BEST_BETA if beta is None or beta <= 0 else float(F32(beta))
        u = ts / lpw
        arg = b * np.sqrt(1.0 - u * u)
        win = np.array([bessel_i0(float(a)) for a in arg.ravel()]).reshape(arg.shape) / bessel_i0(b)
    m = np.rint(ts)
    r = ts - m
    sn = np.where(np.fmod(m, 2.0) != 0.0, -np.sin(math.pi * r), np.sin(math.pi * r))
    sinc = np.where(ts == 0, 1.0, sn / np.where(ts == 0, 1.0, math.pi * ts))
    return np.where(inside, sinc * (win * scale), 0.0)


def table64(in_rate, out_rate, lpw=6, rolloff=0.99, window="hann", beta=None):
    """T [1025][2W] in float64 (the law rounds it once to f32)."""
    W, _ = width(in_rate, out_rate, lpw, rolloff)
    k = np.arange(2 * W, dtype=F64)[None, :] - (W - 1)
    p = np.arange(PHASES + 1, dtype=F64)[:, None] / PHASES
    return kernel64(k - p, in_rate, out_rate, lpw, rolloff, window, beta)


def resample(x, table, pos, lo=0, received=None):
    """The law's sum: x [..., N] f32 (input index lo onward; zero outside [0, received or lo + N)), table f32 [1025][2W], pos a list of
    positions -> [..., len(pos)] f32."""
    x = np.asarray(x, dtype=F32)
    table = np.asarray(table, dtype=F32)
    L = table.shape[1]
    W = L // 2
    N = x.shape[-1]
    end = lo + N if received is None else received
    pos = [int(v) for v in pos]
    n = np.array([v >> 32 for v in pos], dtype=np.int64)
    f = np.array([v & 0xffffffff for v in pos], dtype=np.int64)
    p = f >> FRAC_BITS
    mu = ((f & ((1 << FRAC_BITS) - 1)).astype(F64) * 2.0 ** -FRAC_BITS).astype(F32)
    D = (table[1:] - table[:-1]).astype(F32)
    acc = np.zeros(x.shape[:-1] + (len(pos),), dtype=F32)
    for k in range(L):
        h = fma32(mu, D[p, k], table[p, k])
        i = n - W + 1 + k
        ok = (i >= 0) & (i < end) & (i - lo >= 0) & (i - lo < N)
        xi = np.where(ok, x[..., np.clip(i - lo, 0, N - 1)], F32(0))
        acc = fma32(np.broadcast_to(h, acc.shape), xi, acc)
    return acc


def whole(x, table, in_rate, out_rate, side, schedule):
    """conan_resample_drift of whole signals x [..., N]."""
    n = length(in_rate, out_rate, side, schedule, np.asarray(x).shape[-1])
    return resample(x, table, positions(in_rate, out_rate, side, schedule, n))


def exact64(x, pos, in_rate, out_rate, **filt):
    """The same kernel at the exact positions, no table, all float64: x [N] -> [len(pos)]."""
    x = np.asarray(x, dtype=F64)
    W, _ = width(in_rate, out_rate, filt.get("lpw", 6), filt.get("rolloff", 0.99))
    n = np.array([int(v) >> 32 for v in pos], dtype=np.int64)
    fr = np.array([(int(v) & 0xffffffff) for v in pos], dtype=F64) * 2.0 ** -32
    acc = np.zeros(len(pos), dtype=F64)
    for k in range(2 * W):
        i = n - W + 1 + k
        ok = (i >= 0) & (i < x.shape[0])
        acc += kernel64((k - W + 1) - fr, in_rate, out_rate, **filt) * np.where(ok, x[np.clip(i, 0, x.shape[0] - 1)], 0.0)
    return acc
