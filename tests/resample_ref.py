"""Float64 restatement of the library's resampler (include/conan_hip.h, conan_resample_cfg): torchaudio.functional.resample's
windowed sinc, taps with |t| >= lowpass_filter_width dropped, each phase's taps contiguous.  The configuration's rolloff and beta
are f32 fields, so they are rounded to f32 here as the library sees them."""
import math

import numpy as np

KAISER_BETA = 14.769656459379492
PRESETS = {"hann": (6, 0.99, "hann", None), "kaiser_best": (64, 0.9475937167399596, "kaiser", None)}


def reduce(in_rate, out_rate):
    g = math.gcd(in_rate, out_rate)
    return in_rate // g, out_rate // g


def length(in_rate, out_rate, samples):
    orig, new = reduce(in_rate, out_rate)
    return -(-new * samples // orig)


def _window(t, lpw, window, beta):
    if window == "hann":
        return np.cos(t * math.pi / lpw / 2) ** 2
    b = float(np.float32(beta)) if beta else KAISER_BETA
    return np.i0(b * np.sqrt(np.maximum(0.0, 1 - (t / lpw) ** 2))) / np.i0(b)


def filt(in_rate, out_rate, lpw=6, rolloff=0.99, window="hann", beta=None):
    """-> (orig, new, w, phases): phases[p] = (klo, taps float64 [cnt]); output p + new*q reads inputs q*orig - w + klo + k."""
    orig, new = reduce(in_rate, out_rate)
    base = min(orig, new) * float(np.float32(rolloff))
    w = math.ceil(lpw * orig / base)
    k = np.arange(-w, w + orig)
    phases = []
    for p in range(new):
        t = (-p / new + k / orig) * base
        keep = np.abs(t) < lpw
        idx = np.nonzero(keep)[0]
        assert len(idx) and idx[-1] - idx[0] + 1 == len(idx)
        tt = t[keep]
        win = _window(tt, lpw, window, beta)
        x = tt * math.pi
        with np.errstate(invalid="ignore", divide="ignore"):
            sinc = np.where(x == 0, 1.0, np.sin(x) / np.where(x == 0, 1.0, x))
        phases.append((int(idx[0]), sinc * (win * (base / orig))))
    return orig, new, w, phases


def resample(x, in_rate, out_rate, lpw=6, rolloff=0.99, window="hann", beta=None, block=2048):
    """x [n, N] -> (y float64 [n, nout], abs_sum [n, nout] = sum_k |h_k x_k|, K [nout] = taps of each output's phase)."""
    x = np.asarray(x, dtype=np.float64)
    n, N = x.shape
    orig, new, w, phases = filt(in_rate, out_rate, lpw, rolloff, window, beta)
    nout = length(in_rate, out_rate, N)
    y, s = np.zeros((n, nout)), np.zeros((n, nout))
    K = np.zeros(nout, dtype=np.int64)
    for p, (klo, h) in enumerate(phases):
        js = np.arange(p, nout, new)
        K[js] = len(h)
        for b in range(0, len(js), block):
            j = js[b:b + block]
            i = (j // new)[:, None] * orig - w + klo + np.arange(len(h))[None, :]
            ok = (i >= 0) & (i < N)
            xi = np.where(ok[None], x[:, np.clip(i, 0, N - 1)], 0.0)
            y[:, j] = (xi * h[None, None]).sum(-1)
            s[:, j] = np.abs(xi * h[None, None]).sum(-1)
    return y, s, K


def bound(abs_sum, K):
    """Rigorous bound of an f32 FMA chain of K terms with f32-rounded taps against the float64 sum: (gamma_K + 2u) sum |h x|."""
    u = 2.0 ** -24
    gamma = K * u / (1 - K * u)
    return (gamma + 2 * u) * abs_sum
