"""Register matching restated (include/conan_hip.h, conan_register_cfg): the causal log-f0 mean transform of a tracked contour, with
Python integers for the state and np.float64 / np.float32 scalars for every rounded step, so each line is one IEEE operation.

match():          the law as a sequential loop over the frames.
match_blocked():  the same law the way a machine with many lanes walks it: the frames in tiles, inclusive prefix sums of (counted, q)
                  inside a tile, the tiles' totals carried along afterwards.  The sums are exact integers, so the two must agree bit for
                  bit whatever the tile width - tests/test_register_ref_cpu.py checks that.
Both take v, uv [T] float32 and return (v' [T] float32, (n, S) after the row)."""
import numpy as np

UNIT = 4194304      # 2^22
F64, F32 = np.float64, np.float32


def quantise(v):
    """q = llrint((double)v * 2^22) -> Python int (np.rint ties to even, as llrint in the default rounding mode)."""
    return int(np.rint(F64(F32(v)) * F64(UNIT)))


def prior_seed(value, frames=50):
    """The prior as a seed: `frames` voiced frames at `value` (log2 Hz)."""
    return int(frames), int(frames) * quantise(value)


def counted(v, uv):
    v, uv = F32(v), F32(uv)
    return bool(uv == 0 and np.isfinite(v) and abs(v) <= F32(64.0))


def shift(n, S, target, max_shift):
    """d of the law for the state (n, S), n >= 1: f64."""
    mu = F64(S) / (F64(n) * F64(UNIT))
    d = F64(F32(target)) - mu
    lim = F64(F32(max_shift))
    return np.minimum(np.maximum(d, -lim), lim)


def match(v, uv, target, max_shift=2.0, seed=(0, 0)):
    v = np.asarray(v, dtype=np.float32)
    uv = np.asarray(uv, dtype=np.float32)
    out = v.copy()
    n, S = int(seed[0]), int(seed[1])
    for j in range(v.shape[0]):
        if not counted(v[j], uv[j]):
            continue
        n += 1
        S += quantise(v[j])
        out[j] = F32(F64(v[j]) + shift(n, S, target, max_shift))
    return out, (n, S)


def match_blocked(v, uv, target, max_shift=2.0, seed=(0, 0), tile=256):
    v = np.asarray(v, dtype=np.float32)
    uv = np.asarray(uv, dtype=np.float32)
    out = v.copy()
    cn, cS = int(seed[0]), int(seed[1])
    for base in range(0, v.shape[0], tile):
        idx = range(base, min(base + tile, v.shape[0]))
        flags = [counted(v[j], uv[j]) for j in idx]
        ks = [1 if f else 0 for f in flags]
        qs = [quantise(v[j]) if f else 0 for j, f in zip(idx, flags)]
        # inclusive prefix sums inside the tile (Hillis-Steele, the shape of a lane scan)
        d = 1
        while d < len(ks):
            ks = [k + (ks[i - d] if i >= d else 0) for i, k in enumerate(ks)]
            qs = [q + (qs[i - d] if i >= d else 0) for i, q in enumerate(qs)]
            d *= 2
        # the carry is added afterwards
        for i, j in enumerate(idx):
            if flags[i]:
                out[j] = F32(F64(v[j]) + shift(cn + ks[i], cS + qs[i], target, max_shift))
        if ks:
            cn, cS = cn + ks[-1], cS + qs[-1]
    return out, (cn, cS)


def mean(state):
    """Mean log2 Hz of a state, None without a counted frame."""
    n, S = state
    return S / (n * float(UNIT)) if n else None
