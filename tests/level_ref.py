"""numpy restatement of the streaming leveller's law that include/conan_hip.h defines (conan_level_cfg), built on
tests/loudness_ref.py's K-weighting: the causal meter over complete gating blocks, the update instants every U samples, the two
gates over the window, the gain with its caps and peak limit, the ramps.  numpy only; float64 throughout, one rounding to float32 at
the end.  tests/test_level_cpu.py holds it to loudness_ref.loudness on the prefixes."""
import numpy as np

from tests import loudness_ref as LR

FS, U = 16000, 1280      # the shipped configuration: hop 320 * 50, segment 4 * hop 320


def blocks(n, fs=FS):
    """[(lo_j, hi_j)] of the complete gating blocks of an n-sample stream, evaluated in double in the header's order."""
    fs = float(fs)
    out, j = [], 0
    while True:
        lo, hi = int(LR.T_G * (j * LR.STEP) * fs), int(LR.T_G * (j * LR.STEP + 1) * fs)
        if hi > n:
            return out
        out.append((lo, hi))
        j += 1


def gate(z, l):
    """conan_loud_norm's two gates over the window's blocks -> (L, distance of the nearest l_j to a gate)."""
    if len(z) == 0:
        return -np.inf, np.inf
    margin = float(np.min(np.abs(l - LR.ABS_GATE)))
    first = l >= LR.ABS_GATE
    if not first.any():
        return -np.inf, margin
    rel = -0.691 + 10.0 * np.log10(np.mean(z[first])) - 10.0
    margin = min(margin, float(np.min(np.abs(l - rel))))
    kept = (l > rel) & (l > LR.ABS_GATE)
    if not kept.any():
        return -np.inf, margin
    return float(-0.691 + 10.0 * np.log10(np.mean(z[kept]))), margin


def level(x, fs=FS, u=U, target=-22.0, max_boost_db=20.0, max_cut_db=40.0, initial_gain_db=0.0, window_blocks=4096, peak_limit=True,
          clip=False, yk=None):
    """yk: LR.k_filter(x, fs) where the caller has it already.  -> dict(y float32 [N], trace float64 [K, 2] rows (L_k, G_k),
    peaks [K] P_k, counts [K] J_k, hi [K] the end of block J_k - 1 (0 without one), margin: the smallest distance of any window
    block's l_j to either gate over all instants)."""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    target, boost, cut = (float(np.float32(v)) for v in (target, max_boost_db, max_cut_db))
    yk = LR.k_filter(x, fs) if yk is None else yk
    bl = blocks(n, fs)
    z = np.array([np.sum(np.square(yk[lo:hi])) / (LR.T_G * float(fs)) for lo, hi in bl], dtype=np.float64)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
    ax = np.abs(x.astype(np.float64))
    K = -(-n // u)
    y = np.empty(n, dtype=np.float32)
    trace, peaks, counts, his = np.empty((K, 2)), np.empty(K), np.empty(K, dtype=np.int64), np.empty(K, dtype=np.int64)
    g_prev = 10.0 ** (float(np.float32(initial_gain_db)) / 20.0)
    margin = np.inf
    for k in range(K):
        uk = k * u
        J = sum(1 for _, hi in bl if hi <= uk)
        w0 = max(0, J - int(window_blocks))
        L, m = gate(z[w0:J], l[w0:J])
        margin = min(margin, m)
        P = float(ax[:uk].max()) if uk else 0.0
        G = g_prev if L == -np.inf else 10.0 ** (min(max(target - L, -cut), boost) / 20.0)
        if peak_limit and G * P > 1.0:
            G = 1.0 / P
        cnt = min(u, n - uk)
        g = g_prev + (G - g_prev) * (np.arange(1, cnt + 1, dtype=np.float64) / float(u))
        yy = (x[uk:uk + cnt].astype(np.float64) * g).astype(np.float32)
        y[uk:uk + cnt] = np.clip(yy, -1.0, 1.0) if clip else yy
        trace[k], peaks[k], counts[k], his[k] = (L, G), P, J, (bl[J - 1][1] if J else 0)
        g_prev = G
    return dict(y=y, trace=trace, peaks=peaks, counts=counts, hi=his, margin=float(margin))


def sig(n, seed):
    """The dynamic test signal: blocks under the absolute gate, a first reading that asks for more than the boost cap, a 0.9 spike
    that makes the peak limit pull the gain to 1.11, a quiet stretch the relative gate drops once the loud part arrives."""
    t = np.arange(n) / 16000.0
    rng = np.random.RandomState(seed)
    base = 0.3 * np.sin(2 * np.pi * 220 * t) + 0.1 * np.sin(2 * np.pi * 2300 * t) + 0.05 * rng.randn(n)
    env = np.where(t < 0.35, 1e-5, np.where(t < 1.2, 0.02, np.where(t < 1.5, 1e-5, 0.6)))
    x = base * env
    x[int(0.9 * 16000)] = 0.9
    return x.astype(np.float32)


CASES = [(n, seed) for seed in (1, 2, 3) for n in (2 * 16000 + 5, 3 * 16000 + 777)]
