"""The signalling tones' law (include/conan_hip.h, conan_tone_cfg) restated in numpy with Python integers: the table, the s16 value
of a sample, the 17 integer sums of a 20 ms frame over the absolute sample index, the frame digit, the debounce with its level and
sound, and the regeneration - one f32 product and one f32 fused multiply-add per sample.  Everything is exact: the tests compare
bits.  No constant here is read from the library."""
import numpy as np

from tests.bypass_ref import fma32, interp

F32, F64 = np.float32, np.float64
FULL = 1 << 20
HOP_MAX = 512
FREQS = (697, 770, 852, 941, 1209, 1336, 1477, 1633)      # rows 0 .. 3, columns 0 .. 3
KEYS = "123A456B789C*0#D"                                  # d = 4 * row + column
STOP = 1 << 30


def table(M):
    """W[m] = rint(2^14 cos(2 pi m / M)), int16."""
    return np.rint(16384.0 * np.cos(2.0 * np.pi * np.arange(M, dtype=F64) / F64(M))).astype(np.int16)


def cfg(hop=320, **kw):
    """The law's parameters with the Python layer's defaults; thr = (A hop / 8)^2 for A = 327.68, -40 dBFS per tone."""
    c = dict(thr=int(round((327.68 * hop / 8.0) ** 2)), twist_fwd_q8=643, twist_rev_q8=1615, sel=8, share_q8=128, on_frames=2, off_frames=2,
             min_frames=3, step=FULL, gain=0.125)
    c.update(kw)
    return c


def seed():
    return dict(cand=-1, run=0, cur=-1, miss=0, held=0, sound=-1, level=0, events=0, frames=0)


def quantise(x):
    """q = clamp(rint(x * 32768), -32768, 32767) in f32, ties to even."""
    v = np.rint(np.asarray(x, dtype=F32) * F32(32768.0))
    return np.fmin(np.fmax(v, F32(-32768.0)), F32(32767.0)).astype(np.int64)


def frame_sums(q, j0, W):
    """(E, [C], [S]) as Python integers of the frame q [hop] (int64) whose first sample has utterance index j0."""
    M = len(W)
    j = int(j0) % M + np.arange(len(q), dtype=np.int64)      # ((F j) mod M depends on j mod M only)
    w = W.astype(np.int64)
    E = int(np.sum(q * q))
    C, S = [], []
    for F in FREQS:
        ic = (F * j) % M
        C.append(int(np.sum(q * w[ic])))
        S.append(int(np.sum(q * w[(ic - M // 4) % M])))
    return E, C, S


def powers(C, S):
    return [(c >> 16) ** 2 + (s >> 16) ** 2 for c, s in zip(C, S)]      # (Python's >> is arithmetic)


def frame_digit(E, C, S, c, hop):
    P = powers(C, S)
    r = max(range(4), key=lambda i: (P[i], -i))
    k = max(range(4), key=lambda i: (P[4 + i], -i))
    Pr, Pc = P[r], P[4 + k]
    ok = Pr >= c["thr"] and Pc >= c["thr"]
    ok = ok and Pc * 256 <= Pr * c["twist_fwd_q8"] and Pr * 256 <= Pc * c["twist_rev_q8"]
    ok = ok and all(P[i] * c["sel"] <= Pr for i in range(4) if i != r) and all(P[4 + i] * c["sel"] <= Pc for i in range(4) if i != k)
    ok = ok and (Pr + Pc) * 32 * 256 >= c["share_q8"] * hop * E
    return 4 * r + k if ok else -1


def share(E, C, S, hop):
    """The pair's share of the frame's energy in 0 .. 1 (a float, for the tests' reports only)."""
    P = powers(C, S)
    return (max(P[:4]) + max(P[4:])) * 32.0 / (hop * E) if E else 0.0


def step(s, d, c):
    """One frame of the debounce on the state dict s (in place) with frame digit d."""
    if d >= 0 and d == s["cand"]:
        s["run"] = min(s["run"] + 1, STOP)
    elif d >= 0:
        s["cand"], s["run"] = d, 1
    else:
        s["cand"], s["run"] = -1, 0
    if s["cur"] >= 0:
        s["held"] = min(s["held"] + 1, STOP)
        s["miss"] = 0 if d == s["cur"] else s["miss"] + 1
        if s["miss"] >= c["off_frames"] and s["held"] >= c["min_frames"]:
            s["cur"], s["miss"], s["held"] = -1, 0, 0
    if s["cur"] < 0 and s["run"] >= c["on_frames"]:
        s["cur"], s["held"], s["miss"] = s["cand"], 0, 0
        s["events"] += 1
    target = FULL if s["cur"] >= 0 else 0
    s["level"] += max(-c["step"], min(c["step"], target - s["level"]))
    if s["cur"] >= 0:
        s["sound"] = s["cur"]
    elif s["level"] == 0:
        s["sound"] = -1
    s["frames"] += 1


def detect(x, c=None, hop=320, state=None, W=None, raw=False):
    """The detector over x [N] (f32, 50 * hop Hz) from `state` (default: the seed), whose `frames` is the first frame's index ->
    (digit, sound, level) int32 [ceil(N / hop)] and the state after; raw=True: also the frame digits d."""
    c = cfg(hop) if c is None else c
    W = table(50 * hop) if W is None else W
    s = dict(seed() if state is None else state)
    q = quantise(x)
    n = (len(q) + hop - 1) // hop
    q = np.concatenate([q, np.zeros(n * hop - len(q), dtype=np.int64)])
    dg, sd, lv, ds = (np.empty(n, dtype=np.int32) for _ in range(4))
    for f in range(n):
        E, C, S = frame_sums(q[f * hop:(f + 1) * hop], s["frames"] * hop, W)
        d = frame_digit(E, C, S, c, hop)
        step(s, d, c)
        dg[f], sd[f], lv[f], ds[f] = s["cur"], s["sound"], s["level"], d
    return (dg, sd, lv, s, ds) if raw else (dg, sd, lv, s)


def events(digit):
    """[(key, first frame, frames)] of a row of per-frame digits."""
    out, prev, start = [], -1, 0
    for f, d in enumerate(list(digit) + [-1]):
        d = int(d)
        if d != prev:
            if prev >= 0:
                out.append((KEYS[prev], start, f - start))
            prev, start = d, f
    return out


def fill(y, sound, level, gain=0.125, hop=320, pos0=0, start_level=0, start_sound=-1, W=None):
    """The regeneration on y [N] f32 with sound[f], level[f] after frame f; sample s is utterance sample pos0 + s."""
    y = np.asarray(y, dtype=F32)
    N, M = y.shape[-1], 50 * hop
    W = table(M) if W is None else W
    sound = np.asarray(sound, dtype=np.int64)
    l = interp(level, start_level, N, hop)
    s = np.arange(N, dtype=np.int64)
    f = s // hop
    prev = np.where(f > 0, sound[np.maximum(f - 1, 0)], np.int64(start_sound))
    g = np.where(sound[f] >= 0, sound[f], prev)
    gc = np.maximum(g, 0)
    fr, fc = np.array(FREQS[:4], dtype=np.int64)[gc // 4], np.array(FREQS[4:], dtype=np.int64)[gc % 4]
    j = int(pos0) % M + s                                      # ((F j) mod M depends on j mod M only)
    ir, ic = (fr * j - M // 4) % M, (fc * j - M // 4) % M
    w = np.where(g >= 0, W.astype(np.int64)[ir] + W.astype(np.int64)[ic], 0)
    kf = F32(gain) * F32(2.0 ** -14)
    syn = (w.astype(F32) * kf).astype(F32)
    full = hop << 20
    g_t = (l.astype(F64) / F64(full)).astype(F32)
    g_y = ((full - l).astype(F64) / F64(full)).astype(F32)
    return np.where(l == 0, y, fma32(syn, g_t, (y * g_y).astype(F32))).astype(F32)


def pair(key, n, amp_db=(-6.0, -6.0), hop=320, start=0, offset=0.0, phase=(0.3, 1.1)):
    """n samples of the key's tone pair (f64): per tone the level in dBFS (full scale = 1.0), a relative frequency offset, phases."""
    d = KEYS.index(key)
    M = 50 * hop
    t = (np.arange(n, dtype=F64) + start) / M
    lo, hi = FREQS[d // 4] * (1.0 + offset), FREQS[4 + d % 4] * (1.0 + offset)
    return 10.0 ** (amp_db[0] / 20.0) * np.sin(2 * np.pi * lo * t + phase[0]) + 10.0 ** (amp_db[1] / 20.0) * np.sin(2 * np.pi * hi * t + phase[1])
