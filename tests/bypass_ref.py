"""The source bypass's law (include/conan_hip.h, conan_bypass_cfg) restated in numpy with Python integers: the slew of the wet and dry
levels per emitted frame, the fill by the closed part of the activity gate, the linear interpolation of a level inside a frame and
the mix - one f32 product and one f32 fused multiply-add per sample.  Everything is exact: the tests compare bits.

numpy has no fused multiply-add.  fma32 forms x * g exactly in f64 (two 24-bit significands), adds t with the rounding error in hand
(TwoSum) and rounds the f64 sum to odd before it is rounded to f32: a sum rounded to odd at 53 bits and then to nearest at 24 bits
is the exact sum rounded to nearest once."""
import numpy as np

F32, F64 = np.float32, np.float64
FULL = 1 << 20


def slew(v, target, step):
    d = int(target) - int(v)
    return int(v) + max(-int(step), min(int(step), d))


def fill(dry, gate, fill_gate):
    """The effective dry level of a frame that ends at gate level `gate` (FULL: open)."""
    return (int(dry) * (FULL - int(gate))) >> 20 if fill_gate else int(dry)


def seed_state(wet, dry, fill_gate=False, gate_before=FULL):
    """The state a restart begins from: the seed levels, and the fill formula on seed_dry with the gate's level before the chunk."""
    return dict(wet=int(wet), dry=int(dry), dry_eff=fill(dry, gate_before, fill_gate))


def levels(state, wet_target, dry_target, step, frames, fill_gate=False, gate=None):
    """The slew over `frames` frames from state (wet, dry, dry_eff) -> (wet [frames], dry_eff [frames], state after).  gate: the
    frame-end gate levels [frames] (None: no gate, which counts as open)."""
    st = dict(state)
    w, d = np.empty(frames, dtype=np.int32), np.empty(frames, dtype=np.int32)
    for f in range(frames):
        st["wet"] = slew(st["wet"], wet_target, step)
        st["dry"] = slew(st["dry"], dry_target, step)
        st["dry_eff"] = fill(st["dry"], FULL if gate is None else gate[f], fill_gate)
        w[f], d[f] = st["wet"], st["dry_eff"]
    return w, d, st


def interp(lv, start, samples, hop):
    """[samples] int64: l of every sample of a signal whose frame f ends at level lv[f]; start = the level before frame 0."""
    lv = np.asarray(lv, dtype=np.int64)
    s = np.arange(samples, dtype=np.int64)
    f, k = s // hop, s % hop
    prev = np.where(f > 0, lv[np.maximum(f - 1, 0)], np.int64(start))
    return prev * (hop - 1 - k) + lv[f] * (k + 1)


def gain(l, hop):
    return (l.astype(F64) / F64(hop << 20)).astype(F32)


def fma32(x, g, t):
    """fmaf(x, g, t) of f32 arrays, correctly rounded."""
    p = x.astype(F64) * g.astype(F64)      # exact
    t = t.astype(F64)
    s = p + t
    bb = s - p
    err = (p - (s - bb)) + (t - bb)        # exact: s + err = p + t
    even = (s.view(np.uint64) & np.uint64(1)) == 0
    fix = (err != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def mix(y, x, wet_lv, dry_lv, start_wet, start_dry, hop):
    """The mix of y (the vocoder's samples behind the gate) and x (the source samples), both [samples] f32."""
    y, x = np.asarray(y, dtype=F32), np.asarray(x, dtype=F32)
    n = y.shape[-1]
    lw, ld = interp(wet_lv, start_wet, n, hop), interp(dry_lv, start_dry, n, hop)
    t = (y * gain(lw, hop)).astype(F32)
    return np.where(ld == 0, t, fma32(x, gain(ld, hop), t)).astype(F32)
