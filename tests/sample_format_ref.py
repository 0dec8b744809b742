"""The sample formats of include/conan_hip.h (CONAN_SAMPLE_S16 / _ULAW / _ALAW) restated in numpy from the header's text: exact
decoding of 16-bit PCM and ITU-T G.711 codes to floats, and encoding of finite floats through s = clamp(rint(x * 32768)), ties to
even.  Written from the rules, not from the library: the CPU test holds it to the pinned facts and to audioop, the GPU tests hold
the library to it."""
import numpy as np

FORMATS = ("s16", "ulaw", "alaw")
DTYPES = {"f32": np.float32, "s16": np.int16, "ulaw": np.uint8, "alaw": np.uint8}
BYTES = {"f32": 4, "s16": 2, "ulaw": 1, "alaw": 1}
ULAW_STEPS = (0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF)
ALAW_STEPS = (0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF)
# float -> s16 at ties and at the ends of the range: (k + 0.5) / 32768 for even and odd k of both signs, +-1, +-1.5, +-0, 2^-20
TIES = np.array([(k + 0.5) / 32768 for k in (0, 1, 2, 3, 100, 101, 32766, 32767, -1, -2, -3, -4, -101, -102, -32768, -32769)]
                + [1.0, -1.0, 1.5, -1.5, 0.0, -0.0, 2.0 ** -20, -2.0 ** -20], dtype=np.float32)


def decode_int(codes, fmt):
    """Codes -> the 16-bit integers v with x = v / 32768 (int64)."""
    c = np.asarray(codes)
    if fmt == "s16":
        return c.astype(np.int64)
    b = c.astype(np.int64) & 0xFF
    if fmt == "ulaw":
        u = ~b & 0xFF
        t = (((u & 15) << 3) + 0x84) << ((u >> 4) & 7)
        return np.where(u & 0x80, 0x84 - t, t - 0x84)
    assert fmt == "alaw", fmt
    a = b ^ 0x55
    m, e = a & 15, (a >> 4) & 7
    t = np.where(e == 0, (m << 4) + 8, ((m << 4) + 0x108) << np.maximum(e - 1, 0))
    return np.where(a & 0x80, t, -t)


def decode(codes, fmt):
    """Codes -> float32, exactly."""
    if fmt == "f32":
        return np.asarray(codes, dtype=np.float32)
    return (decode_int(codes, fmt).astype(np.float64) / 32768.0).astype(np.float32)


def quantize(x):
    """s = clamp(rint(x * 32768), -32768, 32767) of finite float32 x, ties to even (int64).  x * 32768 is exact in float64."""
    s = np.rint(np.asarray(x, dtype=np.float32).astype(np.float64) * 32768.0)      # np.rint rounds half to even
    return np.clip(s, -32768, 32767).astype(np.int64)


def encode_int(s, fmt):
    """16-bit integers s -> codes of fmt (int64 in, the format's dtype out)."""
    s = np.asarray(s, dtype=np.int64)
    if fmt == "s16":
        return s.astype(np.int16)
    if fmt == "ulaw":
        p = s >> 2
        neg = p < 0
        p = np.minimum(np.where(neg, -p, p), 8159) + 0x21
        seg = sum((t < p).astype(np.int64) for t in ULAW_STEPS)
        u = np.where(seg >= 8, 0x7F, (seg << 4) | ((p >> (seg + 1)) & 15))
        return (u ^ np.where(neg, 0x7F, 0xFF)).astype(np.uint8)
    assert fmt == "alaw", fmt
    p = s >> 3
    neg = p < 0
    p = np.where(neg, -p - 1, p)
    seg = sum((t < p).astype(np.int64) for t in ALAW_STEPS)
    a = np.where(seg >= 8, 0x7F, (seg << 4) | (np.where(seg < 2, p >> 1, p >> seg) & 15))
    return (a ^ np.where(neg, 0x55, 0xD5)).astype(np.uint8)


def encode(x, fmt):
    """Finite float32 x -> codes of fmt."""
    if fmt == "f32":
        return np.asarray(x, dtype=np.float32)
    return encode_int(quantize(x), fmt)


def convert(x, src, dst):
    return encode(decode(x, src), dst)
