"""The output watermark's two laws (include/conan_hip.h, conan_watermark_cfg) restated in numpy with Python integers: the chip
sequence from the comfort noise's 64-bit hash, the 24-block word, the embedder under a causal peak envelope - one f32 product for the
envelope's decay, one for the amplitude, one f32 add per sample - and the integer detector: pre-whitening, chip correlation at every
block offset, block weights, the offset's score and the soft bits, then the host's decision.  Everything is exact: the tests compare
bits."""
import numpy as np

from tests.comfort_ref import GOLDEN, M64, MUL1, MUL2, hash64

F32, F64 = np.float32, np.float64
CHIP, BLK, SUB, W = 4, 2048, 64, 24
NCHIP = BLK // CHIP
MARKER = (1, 0, 1, 1, 0, 1, 0, 1)
DECAY = F32(0.875)
GAIN, FLOOR = 0.1, 0.0
R_BOUND = 31 * 32768 * 4 * NCHIP      # |R| <= this < 2^31: int32 accumulation is exact
THRESHOLD = 11.5                      # the library's default (midway between the two measured groups)
STATE_BYTES = 16


def chip(key, m):
    """+1 if bit 63 of hash64(key, m) is set, else -1."""
    return 1 if hash64(key, m) >> 63 else -1


def chips(key):
    """chip(key, m) for m = 0 .. 511 -> int64 [512].  uint64 arithmetic wraps, as the law's."""
    with np.errstate(over="ignore"):
        z = np.uint64(int(key) & M64) + (np.arange(NCHIP, dtype=np.uint64) + np.uint64(1)) * np.uint64(GOLDEN)
        z ^= z >> np.uint64(30)
        z *= np.uint64(MUL1)
        z ^= z >> np.uint64(27)
        z *= np.uint64(MUL2)
        z ^= z >> np.uint64(31)
    return np.where(z >> np.uint64(63), 1, -1).astype(np.int64)


def word(id_):
    """The 24 signs of a word: the marker, then the 16 bits of id, MSB first."""
    bits = list(MARKER) + [(int(id_) >> (15 - i)) & 1 for i in range(16)]
    return np.array([1 if b else -1 for b in bits], dtype=np.int64)


def signs(key, id_, pos, count):
    """s(j) for j = pos .. pos + count - 1 -> int64 [count]."""
    j = np.arange(count, dtype=np.int64) + np.int64(pos)
    return chips(key)[(j % BLK) // CHIP] * word(id_)[(j // BLK) % W]


def embed(y, key, id_, gain=GAIN, floor=FLOOR, state=None):
    """The mark on y [samples] f32 from state dict(pos, env) (None: the start) -> (marked f32 [samples], state after).  A last
    sub-block may be short."""
    y = np.asarray(y, dtype=F32)
    n = y.shape[0]
    pos, env = (0, F32(0.0)) if state is None else (int(state["pos"]), F32(state["env"]))
    gain, floor = F32(gain), F32(floor)
    nsub = (n + SUB - 1) // SUB
    pad = np.zeros(nsub * SUB, dtype=F32)
    pad[:n] = np.abs(y)
    p = pad.reshape(nsub, SUB).max(axis=1) if nsub else np.zeros(0, dtype=F32)
    a = np.empty(nsub, dtype=F32)
    for b in range(nsub):
        env = max(F32(p[b]), F32(env * DECAY))
        a[b] = max(F32(env * gain), floor)
    s = signs(key, id_, pos, n).astype(F32)
    out = (y + s * np.repeat(a, SUB)[:n]).astype(F32)
    return out, dict(pos=pos + n, env=F32(env))


def state_bytes(state):
    return np.array([state["pos"]], dtype=np.int64).tobytes() + np.array([state["env"], 0.0], dtype=F32).tobytes()


def state_from(raw):
    raw = bytes(raw)
    return dict(pos=int(np.frombuffer(raw[:8], dtype=np.int64)[0]), env=F32(np.frombuffer(raw[8:12], dtype=F32)[0]))


def blocks(n):
    return max(0, int(n) // BLK - 1)


def bit_length(v):
    return max(1, int(v).bit_length())


def detect(q, key):
    """The device half on the 16-bit view q [n] (integers) -> dict(S int64 [BLK], soft int64 [K], R int64 [K, BLK] before the weights,
    offset, blocks, peak)."""
    q = np.asarray(q, dtype=np.int64)
    n = q.shape[0]
    K = blocks(n)
    out = dict(S=np.zeros(BLK, dtype=np.int64), soft=np.zeros(K, dtype=np.int64), R=np.zeros((K, BLK), dtype=np.int64), offset=0, blocks=K, peak=0)
    if K == 0:
        return out
    d = 16 * q - 15 * np.concatenate([[0], q[:-1]])
    u = d[:-3] + d[1:-2] + d[2:-1] + d[3:]
    c = chips(key).astype(F64)
    Rn = np.zeros((K, BLK), dtype=np.int64)
    for k in range(K):
        w = u[k * BLK:k * BLK + BLK + CHIP * (NCHIP - 1)].astype(F64)      # every partial sum is an integer under 2^31: exact in f64
        win = np.lib.stride_tricks.as_strided(w, shape=(BLK, NCHIP), strides=(w.strides[0], CHIP * w.strides[0]))
        R = (win @ c).astype(np.int64)
        out["R"][k] = R
        nk = bit_length(int(np.abs(d[k * BLK:(k + 2) * BLK]).sum()))
        Rn[k] = np.sign(R) * ((np.abs(R) << 12) >> nk)
    S = np.abs(Rn).sum(axis=0)
    o = int(np.argmax(S))      # the lowest index on ties
    out.update(S=S, soft=Rn[:, o].copy(), offset=o, peak=int(S[o]))
    return out


def decide(S, soft, offset, nblocks, threshold=THRESHOLD):
    """The host half -> dict(present, z, id, offset, rotation, marker_score, blocks)."""
    if nblocks == 0:
        return dict(present=0, z=0.0, id=0, offset=0, rotation=0, marker_score=0, blocks=0)
    tot = 0.0
    for v in S:
        tot += float(int(v))
    mean = tot / BLK
    var = 0.0
    for v in S:
        e = float(int(v)) - mean
        var += e * e
    std = float(np.sqrt(F64(var / BLK)))
    z = (float(int(S[offset])) - mean) / std if std > 0.0 else 0.0
    best = None
    mk = word(0)[:8]
    for r in range(W):
        acc = [0] * W
        for k in range(nblocks):
            acc[(k + r) % W] += int(soft[k])
        score = sum(int(mk[i]) * acc[i] for i in range(8))
        if best is None or score > best[0]:
            best = (score, r, acc)
    score, r, acc = best
    id_ = 0
    for i in range(16):
        id_ = (id_ << 1) | (1 if acc[8 + i] > 0 else 0)
    return dict(present=int(z >= threshold), z=z, id=id_, offset=int(offset), rotation=r, marker_score=score, blocks=int(nblocks))


def detect_decide(q, key, threshold=THRESHOLD):
    d = detect(q, key)
    return dict(decide(d["S"], d["soft"], d["offset"], d["blocks"], threshold), S=d["S"], soft=d["soft"], R=d["R"], peak=d["peak"])
