"""The comfort noise's law (include/conan_hip.h, conan_comfort_cfg) restated in numpy with Python integers: the quantised frame
power, the tracker per emitted frame, the amplitude of a level, the white source (a 64-bit hash of the seed and the utterance sample
index), the colouring taps and the fill against the gate's ramp - one f32 product for the amplitude, one for the noise sample and one
f32 fused multiply-add per sample.  Everything is exact: the tests compare bits."""
import struct

import numpy as np

from tests.bypass_ref import fma32, interp

F32, F64 = np.float32, np.float64
FULL = 1 << 20
M64 = (1 << 64) - 1
GOLDEN, MUL1, MUL2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
TAPS = ((1,), (1, 2, 1), (1, 2, 3, 2, 1))
LEVEL_MIN = -16384


def clamp(v, lo, hi):
    return max(int(lo), min(int(hi), int(v)))


def lq(P):
    """The quantised power of a frame: the biased exponent and the top 8 mantissa bits of the double."""
    bits = struct.unpack("<Q", struct.pack("<d", float(P)))[0]
    return int(bits >> 44) - (1023 << 8)


def hash64(seed, j):
    """The law's 64-bit word of sample j (a Python integer, negative for the taps before sample 0)."""
    z = (int(seed) + ((int(j) + 1) & M64) * GOLDEN) & M64
    z ^= z >> 30
    z = (z * MUL1) & M64
    z ^= z >> 27
    z = (z * MUL2) & M64
    z ^= z >> 31
    return z


def white1(seed, j):
    z = hash64(seed, j)
    return int(z & 0xFFFF) + int((z >> 16) & 0xFFFF) - 65535


def white(seed, j0, count):
    """w(j) for j = j0 .. j0 + count - 1 -> int64 [count].  uint64 arithmetic wraps, as the law's."""
    with np.errstate(over="ignore"):
        j = (np.arange(count, dtype=np.int64) + np.int64((int(j0) + 1 + (1 << 63)) % (1 << 64) - (1 << 63))).astype(np.uint64)
        z = np.uint64(int(seed) & M64) + j * np.uint64(GOLDEN)
        z ^= z >> np.uint64(30)
        z *= np.uint64(MUL1)
        z ^= z >> np.uint64(27)
        z *= np.uint64(MUL2)
        z ^= z >> np.uint64(31)
    return (z & np.uint64(0xFFFF)).astype(np.int64) + ((z >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64) - 65535


def coloured(seed, j0, count, colour):
    """v(j) = sum_i c[i] * w(j - i) for j = j0 .. j0 + count - 1 -> int64 [count]."""
    c = TAPS[colour]
    w = white(seed, int(j0) - (len(c) - 1), count + len(c) - 1)
    return sum(int(ci) * w[len(c) - 1 - i:len(c) - 1 - i + count] for i, ci in enumerate(c))


def norm(colour):
    """The helper's norm: the f32 of 1 / (rms of w * sqrt(sum c^2)); w is the sum of two uniform 16-bit words."""
    return F32(1.0 / (np.sqrt((65536.0 ** 2 - 1.0) / 6.0) * np.sqrt(float(sum(c * c for c in TAPS[colour])))))


def amplitude(L):
    """a of a level L <= 0: the octave in floor(L / 512), a linear piece inside it.  Exact in f32."""
    e = int(L) // 512
    r = int(L) - 512 * e
    return F32(np.ldexp(F64(512 + r), e - 9))


def amplitudes(levels, nrm):
    lv = np.asarray(levels, dtype=np.int64)
    e = lv // 512
    a = np.ldexp((512 + (lv - 512 * e)).astype(F64), (e - 9).astype(np.int64)).astype(F32)      # exact
    return (a * F32(nrm)).astype(F32)


def track(state, cfg, act, power):
    """The tracker over the frames of act / power from state dict(level, idle_frames) -> (levels int32 [frames], state after).
    cfg: anything with the fields of conan_comfort_cfg (mode 1 | 2)."""
    st = dict(level=int(state["level"]), idle_frames=int(state["idle_frames"]))
    out = np.empty(len(act), dtype=np.int32)
    for f in range(len(act)):
        if cfg.mode == 1:
            st["level"] = clamp(cfg.level, cfg.l_min, cfg.l_max)
        elif int(act[f]) == 0:
            target = clamp(lq(power[f]) + cfg.offset, cfg.l_min, cfg.l_max)
            st["level"] += clamp(target - st["level"], -cfg.down_step, cfg.up_step)
            st["idle_frames"] += 1
        out[f] = st["level"]
    return out, st


def fill(y, gate_lv, comfort_lv, start_gate, hop, seed, colour, nrm, pos0=0):
    """The fill of y [samples] f32 (the sample behind the gate and the mix), whose sample s is sample pos0 + s of the white source and
    belongs to frame s // hop of the levels."""
    y = np.asarray(y, dtype=F32)
    n = y.shape[-1]
    l = interp(gate_lv, start_gate, n, hop)
    lc = (np.int64(hop) << np.int64(20)) - l
    gc = (lc.astype(F64) / F64(hop << 20)).astype(F32)
    A = amplitudes(comfort_lv, nrm)[np.arange(n) // hop]
    v = coloured(seed, pos0, n, colour)
    t = (v.astype(F32) * A).astype(F32)
    return np.where(lc == 0, y, fma32(t, gc, y)).astype(F32)
