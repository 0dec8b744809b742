"""Source activity restated (include/conan_hip.h, conan_activity_cfg): the causal voice-activity detector and the gate's gain law, with
Python integers for the state's integers and np.float64 / np.float32 for every rounded step, so each line is one IEEE operation.

params():   the fields of a cfg (conan_amd._lib.ActivityCfg or anything shaped like it) as Python numbers: the f32 fields as the
            f64 of the f32, exactly what the kernel reads.
powers():   P of frames [f0, f0 + count) of a signal, by the law's fixed order: 64 partial sums over k = j (mod 64) ascending,
            multiply (exact in f64) then add, then the fold by 32, 16, 8, 4, 2, 1, then / N.
detect():   the recursion over a list of powers from a state; returns flags, levels, the state after and the branch counts.
run():      powers + detect over a whole signal, or over frames [f0, f0 + count) of it from a carried state (the streamed form).
gain() / gate():  the gain law on the vocoder's samples."""
import numpy as np

FULL = 1 << 20
F64, F32 = np.float64, np.float32
FLOATS = ("open_abs", "close_abs", "open_ratio", "close_ratio", "rise_active", "rise_idle", "floor_min")
INTS = ("hold_frames", "up_step", "down_step", "closed_level")
STATE = ("active", "hang", "level", "floor", "frames", "active_frames")


def params(cfg):
    p = {k: F64(F32(getattr(cfg, k))) for k in FLOATS}
    p.update({k: int(getattr(cfg, k)) for k in INTS})
    return p


def seed_state(cfg):
    s = cfg.seed
    return dict(active=int(s.active), hang=int(s.hang), level=int(s.level), floor=F64(s.floor), frames=int(s.frames), active_frames=int(s.active_frames))


def n_frames(samples, hop):
    return 1 + samples // hop


def frames_of(s, f0, count, N, hop):
    """[count, N] f64: x[k] = s[f * hop - N / 2 + k], zeros outside the signal."""
    s = np.asarray(s, dtype=np.float32)
    idx = (np.arange(f0, f0 + count, dtype=np.int64)[:, None] * hop - N // 2) + np.arange(N, dtype=np.int64)[None, :]
    ok = (idx >= 0) & (idx < s.shape[0])
    return np.where(ok, s[np.clip(idx, 0, max(s.shape[0] - 1, 0))].astype(F64), F64(0.0))


def powers(s, N, hop, f0=0, count=None):
    count = n_frames(len(s), hop) - f0 if count is None else count
    x = frames_of(s, f0, count, N, hop).reshape(count, N // 64, 64)
    p = np.zeros((count, 64), dtype=F64)
    for i in range(N // 64):
        sq = x[:, i, :] * x[:, i, :]      # exact: the square of an f32 fits an f64
        p = sq + p
    for d in (32, 16, 8, 4, 2, 1):
        p[:, :d] = p[:, :d] + p[:, d:2 * d]
    return p[:, 0] / F64(N)


def detect(P, prm, state):
    """-> (act [F] int32, level [F] int32, state after, counts).  counts: openings, closings, hangover frames, floor clamps, and the
    openings decided by the ratio (nf * open_ratio above open_abs)."""
    st = dict(state)
    nf = F64(st["floor"])
    act_out, lvl_out = np.zeros(len(P), dtype=np.int32), np.zeros(len(P), dtype=np.int32)
    counts = dict(openings=0, closings=0, hangover=0, clamps=0, ratio_openings=0)
    for j, Pj in enumerate(P):
        Pj = F64(Pj)
        t_open, t_close = nf * prm["open_ratio"], nf * prm["close_ratio"]
        open_ = np.fmax(prm["open_abs"], t_open)
        close = np.fmax(prm["close_abs"], t_close)
        raw = bool(Pj > (close if st["active"] else open_))
        if raw:
            act = 1
            st["hang"] = prm["hold_frames"]
        elif st["hang"] > 0:
            act = 1
            st["hang"] -= 1
            counts["hangover"] += 1
        else:
            act = 0
        if act and not st["active"]:
            counts["openings"] += 1
            counts["ratio_openings"] += int(t_open > prm["open_abs"])
        if st["active"] and not act:
            counts["closings"] += 1
        rise = nf * (prm["rise_active"] if act else prm["rise_idle"])
        low = np.fmin(Pj, rise)
        counts["clamps"] += int(low < prm["floor_min"])
        nf = np.fmax(low, prm["floor_min"])
        st["level"] = min(st["level"] + prm["up_step"], FULL) if act else max(st["level"] - prm["down_step"], prm["closed_level"])
        st["active"] = act
        st["frames"] += 1
        st["active_frames"] += act
        act_out[j], lvl_out[j] = act, st["level"]
    st["floor"] = nf
    return act_out, lvl_out, st, counts


def run(s, cfg, N=1024, hop=320, state=None, f0=0, count=None):
    """The law over frames [f0, f0 + count) of signal s (default: all of them) from `state` (default: the cfg's seed)."""
    P = powers(s, N, hop, f0, count)
    act, lvl, st, counts = detect(P, params(cfg), seed_state(cfg) if state is None else state)
    return dict(act=act, level=lvl, power=P, state=st, counts=counts)


def gain(lvl_prev, lvl_next, hop):
    """[hop] f32: g of the samples of one frame."""
    g = np.empty(hop, dtype=F32)
    den = F64(hop << 20)
    for k in range(hop):
        l = int(lvl_prev) * (hop - 1 - k) + int(lvl_next) * (k + 1)
        g[k] = F32(F64(l) / den)
    return g


def gains(levels, start, samples, hop):
    """[samples] f32 for a signal whose frame f ends at level levels[f]; start = the level before frame 0."""
    levels = np.asarray(levels, dtype=np.int64)
    s = np.arange(samples, dtype=np.int64)
    f, k = s // hop, s % hop
    prev = np.where(f > 0, levels[np.maximum(f - 1, 0)], np.int64(start))
    l = prev * (hop - 1 - k) + levels[f] * (k + 1)      # exact int64
    return (l.astype(F64) / F64(hop << 20)).astype(F32)


def gate(x, levels, start, hop):
    x = np.asarray(x, dtype=np.float32)
    return (x * gains(levels, start, x.shape[-1], hop)).astype(F32)


def burst_signal(noise=1e-3, seconds=5.0, sr=16000, seed=0):
    """Noise of rms `noise` with six-harmonic bursts at 0.30-0.80 s, 1.30-1.42 s and 2.0-3.2 s and digital silence at 3.6-3.9 s."""
    rng = np.random.default_rng(seed)
    n = int(seconds * sr)
    t = np.arange(n) / sr
    x = noise * rng.standard_normal(n)
    for a, b, f in ((0.30, 0.80, 140.0), (1.30, 1.42, 210.0), (2.0, 3.2, 120.0)):
        m = (t >= a) & (t < b)
        for h in range(1, 7):
            x[m] += (0.2 / h) * np.sin(2 * np.pi * f * h * t[m])
    x[(t >= 3.6) & (t < 3.9)] = 0.0
    return x.astype(np.float32)
