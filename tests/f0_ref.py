"""The source-pitch tracker's law (include/conan_hip.h, conan_f0_cfg) restated in float64 numpy: YIN on the mel front-end's centred
frames.  `track` is the reference the GPU tests hold conan_f0 to; `judge` also reports, per frame, the smallest margin of every
comparison the law made, so that a test can show that no decision of a test signal sits on a knife's edge.

The cfg fields are float32 in the C struct: thresholds and frequencies are rounded to float32 first, as the library receives them."""
import numpy as np

def lags(sr, fmin, fmax):
    """(tmin, tmax) = (floor(sr / fmax), ceil(sr / fmin)) with the float32 cfg values."""
    fmin, fmax = float(np.float32(fmin)), float(np.float32(fmax))
    return int(np.floor(sr / fmax)), int(np.ceil(sr / fmin))


def judge(x, hop=320, N=1024, fmin=50.0, fmax=900.0, threshold=0.15, floor_db=-60.0):
    """x: one signal (float32 samples are taken as they are) -> dict of per-frame arrays:
    v (float32 log2 Hz, 0 where unvoiced), uv (0 | 1), lag (the picked lag after the walk, -1 without one), f0 (float64 Hz, 0 where
    unvoiced), off (the parabola's offset: the period is lag + off), margin (the smallest distance of any comparison the frame's
    decision made from equality)."""
    sr = 50.0 * hop
    x = np.asarray(x, np.float64).reshape(-1)
    thr = float(np.float32(threshold))
    gate = 10.0 ** (float(np.float32(floor_db)) / 10.0)
    tmin, tmax = lags(sr, fmin, fmax)
    if tmin < 2 or tmax > N // 2 or not float(np.float32(fmin)) < float(np.float32(fmax)):
        raise ValueError("f0_ref: tmin < 2, tmax > N / 2 or fmin >= fmax")
    W = N - tmax - 1
    F = 1 + len(x) // hop
    xp = np.concatenate([np.zeros(N // 2), x, np.zeros(N + hop)])
    v = np.zeros(F, np.float32)
    uv = np.ones(F, np.int32)
    lag = np.full(F, -1, np.int32)
    f0 = np.zeros(F)
    offs = np.zeros(F)
    margin = np.full(F, np.inf)
    for f in range(F):
        fr = xp[f * hop: f * hop + N]
        a = fr[:W]
        power = float(np.dot(a, a)) / W
        d = np.zeros(tmax + 2)
        for t in range(1, tmax + 2):
            e = a - fr[t:t + W]
            d[t] = np.dot(e, e)
        cs = np.cumsum(d[1:])
        dn = np.ones(tmax + 2)
        tt = np.arange(1, tmax + 2, dtype=np.float64)
        nz = cs > 0
        dn[1:][nz] = d[1:][nz] * tt[nz] / cs[nz]
        m = abs(power - gate) / gate                      # the gate, relative to its level
        gated = power < gate
        pick = -1
        t = tmin
        while t <= tmax:
            m = min(m, abs(dn[t] - thr))                  # every threshold test up to and including the first that passes
            if dn[t] < thr:
                pick = t
                break
            t += 1
        if pick >= 0:
            while pick + 1 <= tmax:
                m = min(m, abs(dn[pick + 1] - dn[pick]))  # the walk's comparisons, the one that stops it included
                if not dn[pick + 1] < dn[pick]:
                    break
                pick += 1
        if pick >= 0 and not gated:
            a0, b0, c0 = dn[pick - 1], dn[pick], dn[pick + 1]
            den = a0 - 2.0 * b0 + c0
            m = min(m, abs(den))                          # the denominator's sign
            off = 0.5 * (a0 - c0) / den if den > 0 else 0.0
            off = min(max(off, -1.0), 1.0)
            f0[f] = sr / (pick + off)
            offs[f] = off
            v[f] = np.float32(np.log2(f0[f]))
            uv[f] = 0
            lag[f] = pick
        margin[f] = m
    return dict(v=v, uv=uv, lag=lag, f0=f0, off=offs, margin=margin)


def track(x, **kw):
    """-> (v float32 [frames] log2 Hz, uv int32 [frames]) of one signal."""
    r = judge(x, **kw)
    return r["v"], r["uv"]


def lag_of(v, uv, sr=16000.0):
    """The integer lag nearest to a contour value (the pick within the interpolation's +-1), -1 where unvoiced."""
    v = np.asarray(v, np.float64)
    out = np.full(v.shape, -1, np.int64)
    ok = np.asarray(uv) == 0
    out[ok] = np.rint(sr / np.exp2(v[ok])).astype(np.int64)
    return out


# ---- the test signals (16 kHz).  The GPU tests and the CPU margin test draw from the same functions.

def harmonic(f, N, sr=16000, nh=6, amp=0.2, seed=0, noise=1e-3):
    """nh harmonics of f with 1 / k amplitudes and a little noise, float32 [N]."""
    t = np.arange(N) / float(sr)
    rng = np.random.default_rng(seed)
    h = sum(amp / k * np.sin(2 * np.pi * k * f * t) for k in range(1, nh + 1) if k * f < 0.45 * sr)
    return (h + noise * rng.standard_normal(N)).astype(np.float32)


def glide(N, f_lo=110.0, ratio=3.0, sr=16000, seed=0, gap=None, burst=None):
    """A six-harmonic glide from f_lo to f_lo * ratio over one second, with an optional silent gap and noise burst (sample ranges)."""
    t = np.arange(N) / float(sr)
    rng = np.random.default_rng(seed)
    ph = 2 * np.pi * np.cumsum(f_lo * ratio ** t) / sr
    h = sum(0.2 / k * np.sin(k * ph) for k in range(1, 7))
    if gap:
        h[gap[0]:gap[1]] = 0
    if burst:
        h[burst[0]:burst[1]] = 0.2 * rng.standard_normal(burst[1] - burst[0])
    return (h + 1e-3 * rng.standard_normal(N)).astype(np.float32)


def sig(B, N, rate, seed):
    """tests/wav_helpers._sig on the host: speech-band tones plus noise, float32 [B, N]."""
    rng = np.random.default_rng(seed)
    t = np.arange(N) / float(rate)
    w = [0.3 * np.sin(2 * np.pi * (150 + 70 * i) * t) + 0.1 * np.sin(2 * np.pi * 2300 * t) + 0.05 * rng.standard_normal(N) for i in range(B)]
    return np.stack(w).astype(np.float32)


def gpu_signals():
    """name -> (signal float32 [N], kwargs of judge): every whole signal tests/test_gpu_f0.py compares with this reference."""
    out = {}
    s = sig(2, 8000, 16000, 11)
    out["sig0"], out["sig1"] = (s[0], {}), (s[1], {})
    out["glide"] = (glide(8000, gap=(2500, 3500), burst=(5500, 6500)), {})
    out["h220"] = (harmonic(220.0, 8000, seed=2), {})
    out["short300"] = (harmonic(180.0, 300, seed=3), {})
    lim = sig(1, 8000, 16000, 12)[0]
    out["limits"] = (lim, dict(fmin=31.25, fmax=8000.0))              # tmax = N / 2 = 512, tmin = 2: the setter's limits
    out["n512"] = (harmonic(300.0, 4000, seed=4), dict(N=512, fmin=70.0))   # tmax = 229 <= 256
    return out
