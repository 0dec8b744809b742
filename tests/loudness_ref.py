"""numpy restatement of the loudness arithmetic that include/conan_hip.h defines (conan_loudness_cfg): BS.1770 K-weighting, gating
blocks, the two gates, the gain and the peak division, as pyloudnorm's Meter / normalize.loudness and the reference's
librosa_wav2spec(loud_norm=True) compute them.  numpy only; the recursion is a plain float64 loop (scipy.signal.lfilter's direct
form II transposed).  tests/test_loudness_cpu.py holds it to facts from outside this project."""
import math

import numpy as np

T_G, STEP = 0.4, 0.25
ABS_GATE = -70.0


def k_weighting(fs):
    """((b, a) of the high shelf, (b, a) of the high pass) at rate fs, each normalised by its a0 (float64 lists of 3)."""
    fs = float(fs)
    G, Q, fc = 4.0, 1.0 / math.sqrt(2.0), 1500.0
    A = 10.0 ** (G / 40.0)
    w0 = 2.0 * math.pi * (fc / fs)
    alpha = math.sin(w0) / (2.0 * Q)
    c, r = math.cos(w0), 2.0 * math.sqrt(A) * alpha
    b = [A * ((A + 1) + (A - 1) * c + r), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - r)]
    a = [(A + 1) - (A - 1) * c + r, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - r]
    shelf = ([v / a[0] for v in b], [v / a[0] for v in a])
    Q, fc = 0.5, 38.0
    w0 = 2.0 * math.pi * (fc / fs)
    alpha = math.sin(w0) / (2.0 * Q)
    c = math.cos(w0)
    b = [(1 + c) / 2, -(1 + c), (1 + c) / 2]
    a = [1 + alpha, -2 * c, 1 - alpha]
    hp = ([v / a[0] for v in b], [v / a[0] for v in a])
    return shelf, hp


def biquad(b, a, x):
    """Direct form II transposed from a zero state, float64: y = b0 x + z0; z0 = b1 x - a1 y + z1; z1 = b2 x - a2 y."""
    b0, b1, b2 = b
    _, a1, a2 = a
    y = np.empty(len(x), dtype=np.float64)
    z0 = z1 = 0.0
    for i, v in enumerate(np.asarray(x, dtype=np.float64).tolist()):
        o = b0 * v + z0
        z0 = b1 * v - a1 * o + z1
        z1 = b2 * v - a2 * o
        y[i] = o
    return y


def k_filter(x, fs):
    shelf, hp = k_weighting(fs)
    return biquad(*hp, biquad(*shelf, x))


def block_edges(samples, fs):
    """[(start, end)] of the gating blocks, ends truncated at the signal's end as a Python slice truncates."""
    fs = float(fs)
    T = samples / fs
    n = int(round((T - T_G) / (T_G * STEP)) + 1)
    return [(min(int(T_G * (j * STEP) * fs), samples), min(int(T_G * (j * STEP + 1) * fs), samples)) for j in range(n)]


def measure(x, fs):
    """-> dict(L, z [blocks], l [blocks], gamma_r, kept: bool [blocks]) of one float32 signal."""
    x = np.asarray(x, dtype=np.float32)
    if len(x) < T_G * fs:
        raise ValueError("signal shorter than one gating block")
    y = k_filter(x, fs)
    z = np.array([np.sum(np.square(y[lo:hi])) / (T_G * float(fs)) for lo, hi in block_edges(len(x), fs)], dtype=np.float64)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
    first = l >= ABS_GATE
    if not first.any():
        return dict(L=-np.inf, z=z, l=l, gamma_r=np.nan, kept=np.zeros(len(z), dtype=bool))
    gamma_r = -0.691 + 10.0 * np.log10(np.mean(z[first])) - 10.0
    kept = (l > gamma_r) & (l > ABS_GATE)
    L = -0.691 + 10.0 * np.log10(np.mean(z[kept])) if kept.any() else -np.inf
    return dict(L=float(L), z=z, l=l, gamma_r=float(gamma_r), kept=kept)


def loudness(x, fs):
    return measure(x, fs)["L"]


def normalize(x, fs, target=-22.0, peak_limit=True):
    """-> (y float32, stats [LUFS, gain applied, peak before limiting, blocks kept]); a signal without a loudness is returned unchanged."""
    x = np.asarray(x, dtype=np.float32)
    m = measure(x, fs)
    peak = float(np.abs(x).max()) if len(x) else 0.0
    if m["L"] == -np.inf:
        return x.copy(), np.array([-np.inf, 1.0, peak, 0.0])
    gain = 10.0 ** ((float(target) - m["L"]) / 20.0)
    y = gain * x.astype(np.float64)
    p = gain * peak
    applied = gain
    if peak_limit and p > 1.0:
        y = y / p
        applied = gain / p
    return y.astype(np.float32), np.array([m["L"], applied, p, float(m["kept"].sum())])
