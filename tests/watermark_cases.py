"""The cases the watermark's CPU and GPU tests share: the two 4 s test signals, the three channels of the robustness matrix and the
adversarial rows of the correlation's bound.  The CPU test runs the matrix through the references (tests/resample_ref.py,
tests/sample_format_ref.py); the GPU test hands in the library's own resampler and codecs."""
import numpy as np

from tests import resample_ref as rs
from tests import sample_format_ref as sf
from tests import watermark_ref as wm

KEY, ID, CROP = 0x0123456789ABCDEF, 0xBEEF, 777
OFFSET = (wm.BLK - CROP) % wm.BLK      # where a block of the cropped row begins
SECONDS, RATE = 4, 16000
KINDS = ("marked", "unmarked", "wrongkey")
CHANNELS = ("s16", "ulaw16", "ulaw8")


def tones(N=SECONDS * RATE, seed=5):
    """wav_helpers._sig's speech-band tones plus noise (row 0), restated in numpy: that module needs a GPU to import."""
    rng = np.random.default_rng(seed)
    t = np.arange(N) / float(RATE)
    return (0.3 * np.sin(2 * np.pi * 150 * t) + 0.1 * np.sin(2 * np.pi * 2300 * t) + 0.05 * rng.standard_normal(N)).astype(np.float32)


def ar_noise(N=SECONDS * RATE, seed=9):
    """An AR(2) noise (a resonance near 1.2 kHz) under a 3 Hz amplitude modulation, plus a 140 Hz tone: coloured, and far from
    stationary - the envelope moves through 20 dB."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(N)
    x = np.zeros(N)
    for j in range(2, N):
        x[j] = 1.6 * x[j - 1] - 0.8 * x[j - 2] + e[j]
    x /= np.abs(x).max()
    t = np.arange(N) / float(RATE)
    am = 0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * t)
    return (0.5 * am * x + 0.1 * np.sin(2 * np.pi * 140 * t)).astype(np.float32)


SIGNALS = (("tones", tones), ("ar", ar_noise))


def ref_channels(y):
    """channel -> (format, the row as it arrives at the detector), through the references."""
    down = rs.resample(y[None], RATE, RATE // 2)[0][0].astype(np.float32)
    back = rs.resample(sf.decode(sf.encode(down, "ulaw"), "ulaw")[None], RATE // 2, RATE)[0][0].astype(np.float32)
    return dict(s16=("s16", sf.encode(y, "s16")), ulaw16=("ulaw", sf.encode(y, "ulaw")), ulaw8=("f32", back))


def view(fmt, row):
    """The detector's 16-bit view of a row."""
    return sf.quantize(row) if fmt == "f32" else sf.decode_int(row, fmt)


def rows(embed=None):
    """(signal, kind) -> the cropped f32 row in front of the channels.  embed(x, key): the embedder (default: the reference's)."""
    embed = embed or (lambda x, key: wm.embed(x, key, ID)[0])
    out = {}
    for name, make in SIGNALS:
        x = make()
        out[name, "marked"] = embed(x, KEY)[CROP:]
        out[name, "unmarked"] = x[CROP:]
        out[name, "wrongkey"] = embed(x, KEY ^ 1)[CROP:]
    return out


def matrix(detect, channels=ref_channels, embed=None):
    """(signal, kind, channel) -> detect(signal, kind, channel, format, row, q)."""
    res = {}
    for (name, kind), y in rows(embed).items():
        for ch, (fmt, row) in channels(y).items():
            res[name, kind, ch] = detect(name, kind, ch, fmt, row, view(fmt, row))
    return res


def adversarial(name, key, n):
    """The rows of the bound: q_j = 32767 s(j), and -32768 / 32767 alternating."""
    if name == "chips":
        return 32767 * wm.signs(key, ID, 0, n)
    assert name == "alternating", name
    return np.where(np.arange(n) % 2 == 0, -32768, 32767).astype(np.int64)
