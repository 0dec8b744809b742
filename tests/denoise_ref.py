"""The noise suppressor's law (include/conan_hip.h, conan_denoise_cfg) restated in numpy with int64: the Q10 level of a log-mel
value, the start, the SNR under the floor as it was, the 1-2-1 average across bins, the slew across time, the output and the floor's
update.  Integers and single correctly rounded IEEE operations: the tests compare bits.  `seen` counts every branch taken."""
import collections
import struct

import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64
BINS = 256
STATE_BYTES = 16 + 8 * BINS
FIELDS = ("bias", "knee", "slope", "depth", "close_step", "open_step", "rise", "fall_shift", "floor_min", "smooth", "out_floor")
BRANCHES = ("start", "floor_fall", "floor_rise", "floor_min", "d_zero", "depth", "close", "open", "keep", "out_floor")
seen = collections.Counter()


def fields(c):
    """The law's parameters of a cfg: a dict of FIELDS, or any object with those attributes (an _lib.DenoiseCfg)."""
    get = (lambda k: c[k]) if isinstance(c, dict) else (lambda k: getattr(c, k))
    p = {k: int(get(k)) for k in FIELDS[:-1]}
    p["out_floor"] = F32(get("out_floor"))
    return p


def level(v):
    """L of f32 values: rint(fmin(fmax((double)v, -1024), 1024) * 1024), ties to even; a NaN reads as -1024."""
    with np.errstate(invalid="ignore"):
        return np.rint(np.fmin(np.fmax(np.asarray(v, F32).astype(F64), F64(-1024.0)), F64(1024.0)) * F64(1024.0)).astype(I64)


def denoise(mel, cfg, state=None):
    """mel [T, nm] float32 -> (y [T, nm] float32, state).  state: None (before the first frame) or the dict a call returned:
    frames, bins, floor [nm], att [nm]; a state whose bins is not nm counts as None, as the library's records do."""
    p = fields(cfg)
    x = np.ascontiguousarray(np.asarray(mel, F32))
    T, nm = x.shape
    assert 1 <= nm <= BINS
    y = x.copy()
    fresh = state is None or int(state["bins"]) != nm
    N = np.zeros(nm, I64) if fresh else np.asarray(state["floor"], I64).copy()
    A = np.zeros(nm, I64) if fresh else np.asarray(state["att"], I64).copy()
    frames = 0 if fresh else int(state["frames"])
    lo, hi = np.maximum(np.arange(nm) - 1, 0), np.minimum(np.arange(nm) + 1, nm - 1)
    for f in range(T):
        L = level(x[f])
        if fresh:
            N, A, fresh = np.maximum(L, p["floor_min"]), np.zeros(nm, I64), False
            seen["start"] += 1
        snr = L - (N + p["bias"])
        d = np.maximum(p["knee"] - snr, 0)
        raw = (d * I64(p["slope"])) >> 8
        a = np.minimum(raw, p["depth"])
        seen["d_zero"] += int((d == 0).sum())
        seen["depth"] += int((raw > p["depth"]).sum())
        a2 = (a[lo] + 2 * a + a[hi] + 2) >> 2 if p["smooth"] else a
        closing = a2 > A
        An = np.where(closing, np.minimum(A + p["close_step"], a2), np.maximum(A - p["open_step"], a2))
        seen["close"] += int((closing & (A + p["close_step"] < a2)).sum())
        seen["open"] += int((~closing & (A - p["open_step"] > a2)).sum())
        out = ((L - An).astype(F64) * F64(0.0009765625)).astype(F32)
        seen["out_floor"] += int(((An != 0) & (out < p["out_floor"])).sum())
        out = np.fmax(out, p["out_floor"])
        keep = An == 0
        seen["keep"] += int(keep.sum())
        y[f] = np.where(keep, x[f], out)
        y[f].view(np.uint32)[keep] = x[f].view(np.uint32)[keep]      # (the bits, whatever they are)
        falls = L < N
        Nn = np.where(falls, N - ((N - L + (1 << p["fall_shift"]) - 1) >> p["fall_shift"]), np.minimum(L, N + p["rise"]))
        seen["floor_fall"] += int(falls.sum())
        seen["floor_rise"] += int((~falls).sum())
        seen["floor_min"] += int((Nn < p["floor_min"]).sum())
        N, A = np.maximum(Nn, p["floor_min"]), An
        frames += 1
    if fresh:
        return y, dict(frames=0, bins=0, floor=np.zeros(nm, I64), att=np.zeros(nm, I64))
    return y, dict(frames=frames, bins=nm, floor=N, att=A)


def state_bytes(state):
    """The conan_denoise_state record of a state: int64 frames, int32 bins, reserved, floor[256], att[256]; entries past bins are 0."""
    fl, at = np.zeros(BINS, np.int32), np.zeros(BINS, np.int32)
    n = int(state["bins"])
    fl[:n], at[:n] = np.asarray(state["floor"])[:n], np.asarray(state["att"])[:n]
    return struct.pack("<qii", int(state["frames"]), n, 0) + fl.tobytes() + at.tobytes()


def state_from(raw):
    """The state of a conan_denoise_state record (bytes)."""
    frames, bins, _ = struct.unpack("<qii", raw[:16])
    words = np.frombuffer(raw[16:STATE_BYTES], np.int32).astype(I64)
    return dict(frames=frames, bins=bins, floor=words[:bins].copy(), att=words[BINS:BINS + bins].copy())
