"""Float64 restatement of the mel front-end (conan_wav2mel and the streaming kernels of conan_amd/csrc/frontend.hip) and a derived
per-element bound on |kernel - reference|, for tests/test_frontend_ref_cpu.py and tests/test_gpu_frontend_f64.py.

The specification is librosa_wav2spec (framing 0) / the torch.stft front-end of the earlier loop (framing 1), see oracle/frontend.py.
Two of its steps are float32 BY SPECIFICATION and are float32 here: the stored window and the window x sample product (librosa and
torch multiply in the input dtype), and the filterbank weights (librosa.filters.mel(dtype=float32)).  Everything else - the DFT, the
magnitude, the filterbank sum, the logarithm - is float64 here, and the kernels' deviation from it is what `bound` bounds.  Unlike
oracle/frontend.py (np.fft.rfft on float32 frames: a float32 FFT under numpy 2) this reference is better than the kernels it judges.

Plain numpy; nothing here imports the package or the oracle."""
import functools

import numpy as np

U32 = 2.0 ** -24          # unit roundoff of float32
U64 = 2.0 ** -53          # unit roundoff of float64 (2 U64 = 2^-52)
DENORM32 = 2.0 ** -149    # smallest float32 denormal

# ulp error of the device's logf / log10f.  The HIP math API documentation (the table of maximum ulp errors of the single-precision
# device functions) is not part of the ROCm installation these tests were written against, so the figure is OpenCL's full-profile
# one: log <= 3 ulp, log10 <= 3 ulp (OpenCL C specification, "Relative error as ULPs").  Plus 2: the result's own rounding to float32
# against the unrounded float64 reference (counted as a whole ulp) and a binade edge between reference and result (the ulp of the
# reference may be half the ulp of the result).
LOG_ULP = 3
K_LOG = LOG_ULP + 2

DEFAULT = dict(fft_size=1024, hop_size=320, win_length=1024, num_mels=80, sample_rate=16000, fmin=80, fmax=7600, eps=1e-6,
               mel_vmin=-6.0, mel_vmax=1.5, framing=0, natural_log=False, mag_eps=0.0)


def config(fft_size=1024, hop_size=320, win_length=1024, num_mels=80, sample_rate=16000, fmin=80, fmax=7600, **kw):
    """Context.wav2mel's keywords for (fft, hop, win, mels, rate, fmin, fmax) and anything else by name."""
    p = dict(DEFAULT, fft_size=fft_size, hop_size=hop_size, win_length=win_length, num_mels=num_mels, sample_rate=sample_rate, fmin=fmin, fmax=fmax)
    assert set(kw) <= set(DEFAULT), kw
    p.update(kw)
    return p


def window(n_fft, win_length):
    """Periodic Hann of win_length, centred in the FFT frame (librosa.util.pad_center: lp = (n_fft - win_length) // 2), stored as f32."""
    i = np.arange(win_length, dtype=np.float64)
    w = np.zeros(n_fft, np.float32)
    lp = (n_fft - win_length) // 2
    w[lp:lp + win_length] = (0.5 - 0.5 * np.cos(2.0 * np.pi * i / win_length)).astype(np.float32)
    return w


def _hz_to_mel(f):
    f = np.asarray(f, np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-30) / 1000.0) / (np.log(6.4) / 27.0), f * 3.0 / 200.0)


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), m * 200.0 / 3.0)


@functools.lru_cache(maxsize=None)
def filterbank(sample_rate, n_fft, n_mels, fmin, fmax):
    """librosa.filters.mel(htk=False, norm='slaney', dtype=float32): triangles computed in f64, rounded to f32, scaled by the f32 area
    norm in f32.  fmin / fmax < 0: 0 / Nyquist.  -> [n_mels, n_fft // 2 + 1] float32 (read-only)."""
    fmin = 0.0 if fmin < 0 else float(fmin)
    fmax = sample_rate / 2.0 if fmax < 0 else float(fmax)
    nb = n_fft // 2 + 1
    freqs = np.linspace(0.0, sample_rate / 2.0, nb)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fb = np.zeros((n_mels, nb), np.float32)
    for m in range(n_mels):
        rise = (freqs - edges[m]) / (edges[m + 1] - edges[m])
        fall = (edges[m + 2] - freqs) / (edges[m + 2] - edges[m + 1])
        fb[m] = np.maximum(0.0, np.minimum(rise, fall)).astype(np.float32)
        fb[m] *= np.float32(2.0 / (edges[m + 2] - edges[m]))
    fb.setflags(write=False)
    return fb


def nonempty(fb):
    """Filters with at least one non-zero weight (the others see no FFT bin: their output is the floor)."""
    return (fb != 0).any(axis=1)


def n_frames(p, samples):
    """conan_mel_frames."""
    if p["framing"] == 0:
        return 1 + samples // p["hop_size"]
    padded = samples + 2 * ((p["fft_size"] - p["hop_size"]) // 2)
    return 0 if padded < p["fft_size"] else (padded - p["fft_size"]) // p["hop_size"] + 1


def frames_f32(wav, p, win=None):
    """The windowed frames [frames, n_fft] float32: framing 0 pads n_fft // 2 zeros per side (center=True, pad_mode='constant'),
    framing 1 reflect-pads (n_fft - hop) // 2 per side and frames from the padded signal's first sample (center=False)."""
    x = np.asarray(wav, np.float32)
    assert x.ndim == 1
    N, hop = p["fft_size"], p["hop_size"]
    if p["framing"] == 0:
        y = np.concatenate([np.zeros(N // 2, np.float32), x, np.zeros(N // 2, np.float32)])
    else:
        pad = (N - hop) // 2
        assert pad < len(x)
        y = np.pad(x, (pad, pad), mode="reflect")
    F = n_frames(p, len(x))
    idx = hop * np.arange(F)[:, None] + np.arange(N)[None, :]
    w = window(N, p["win_length"]) if win is None else win
    fr = y[idx] * w[None, :]
    assert fr.dtype == np.float32
    return fr


def _log(p, c):
    return np.log(c) if p["natural_log"] else np.log10(c)


def clip(p, v):
    return np.clip(v, np.float64(np.float32(p["mel_vmin"])), np.float64(np.float32(p["mel_vmax"])))


def magnitudes(fr, p):
    """rfft on float64 frames (a float64 FFT), sqrt(re^2 + im^2 + f32(mag_eps)) -> [frames, n_fft // 2 + 1] float64."""
    spec = np.fft.rfft(fr.astype(np.float64), axis=1)
    assert spec.dtype == np.complex128
    return np.sqrt(spec.real ** 2 + spec.imag ** 2 + np.float64(np.float32(p["mag_eps"])))


def mel_sums(fr, p, fb=None):
    """Float64 from the f32 frames on: magnitudes(), then the f32 filterbank summed in f64.
    -> s [frames, n_mels] float64, the filterbank sums before floor and log."""
    mag = magnitudes(fr, p)
    fb = filterbank(p["sample_rate"], p["fft_size"], p["num_mels"], p["fmin"], p["fmax"]) if fb is None else fb
    return mag @ fb.astype(np.float64).T


def reference(wav, p):
    """-> dict(mel: the unrounded float64 log-mel [frames, n_mels] clipped as configured, raw: the same unclipped,
    s: the filterbank sums, abs_sum: sum_t |x_t w_t| per frame, fb_sum: sum_b fb[m, b], nonempty: filters with a bin)."""
    fr = frames_f32(wav, p)
    fb = filterbank(p["sample_rate"], p["fft_size"], p["num_mels"], p["fmin"], p["fmax"])
    s = mel_sums(fr, p, fb)
    raw = _log(p, np.maximum(np.float64(np.float32(p["eps"])), s))
    return dict(mel=clip(p, raw), raw=raw, s=s, abs_sum=np.abs(fr.astype(np.float64)).sum(1), fb_sum=fb.astype(np.float64).sum(1),
                nonempty=nonempty(fb))


def bound(ref, p, K=K_LOG):
    """Per-element bound on |kernel - reference| in log units, [frames, n_mels].

    rel = 2 * 2^-24 + (N + 2) * 2^-52 * sum_t |x_t w_t| * sum_b fb[m, b] / max(eps, s):
      - 2 * 2^-24: the two f32 roundings of the kernels, |X| (relative, per bin, so relative on the non-negative filterbank sum) and
        the filterbank sum itself;
      - the second term: an N-term f64 FMA chain with twiddles rounded to f64 is off by at most gamma_N + u <= (N + 2) 2^-53 of
        sum_t |x_t w_t| per component; both components and the square root stay within twice that, (N + 2) 2^-52, on |X| of every bin,
        so the filterbank sum is off by at most that times sum_b fb[m, b], relative to max(eps, s) after the floor (max is 1-Lipschitz).
    A relative error rel becomes rel (ln) or rel / ln 10 (log10) in log units; the device logarithm and the f32 result add
    K ulp32(|reference|) (K_LOG above), plus one float32 denormal.  max and clip are monotone and 1-Lipschitz, so the bound holds for
    the clipped values too: compare clipped with clipped."""
    N = p["fft_size"]
    eps = np.float64(np.float32(p["eps"]))
    rel = 2 * U32 + (N + 2) * 2 * U64 * ref["abs_sum"][:, None] * ref["fb_sum"][None, :] / np.maximum(eps, ref["s"])
    scale = 1.0 if p["natural_log"] else 1.0 / np.log(10.0)
    ulp = np.spacing(np.abs(ref["mel"]).astype(np.float32)).astype(np.float64)
    return rel * scale + K * ulp + DENORM32


# ---- the inputs of the GPU tests (amplitudes below 1; the same three signals serve every test)
SIGNALS = ("broadband", "tone", "silence")


def signal(kind, samples, sample_rate, seed=0):
    """broadband: a decaying 220 Hz sine + a sine at 0.19 x sample_rate + 0.02 x Gaussian noise; tone: 440 Hz at 0.9 (its quiet bins
    lie 6 decades down: where f32 accumulation shows); silence.  -> [samples] float32"""
    t = np.arange(samples) / float(sample_rate)
    if kind == "broadband":
        rng = np.random.default_rng(1000 + seed)
        x = 0.5 * np.sin(2 * np.pi * 220.0 * t + 0.7) * np.exp(-t) + 0.1 * np.sin(2 * np.pi * 0.19 * sample_rate * t + 0.3) + 0.02 * rng.standard_normal(samples)
    elif kind == "tone":
        x = 0.9 * np.sin(2 * np.pi * 440.0 * t)
    elif kind == "silence":
        x = np.zeros(samples)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


# (fft, hop, win, mels, rate, fmin, fmax) of the whole-signal test, centred framing
CENTRED = (
    (1024, 320, 1024, 80, 16000, 80, 7600),        # the default
    (64, 320, 64, 80, 16000, -1, -1),              # n_fft < hop, 0 .. Nyquist, 32 filters without a bin
    (128, 320, 128, 80, 16000, 80, 7600),
    (256, 80, 200, 40, 8000, 0, 4000),
    (512, 128, 399, 128, 16000, 20, 8000),         # odd n_fft - win_length
    (2048, 320, 2048, 80, 16000, 80, 7600),
    (2048, 512, 1201, 512, 48000, 0, 24000),       # 512 mels, odd n_fft - win_length
)
NO_CLIP = dict(mel_vmin=-1e30, mel_vmax=1e30)
# variants on top: the default clip on the default and one other configuration; natural log with mag_eps on one
VARIANTS = (
    (CENTRED[0], {}),
    (CENTRED[4], {}),
    (CENTRED[3], dict(NO_CLIP, natural_log=True, mag_eps=1e-9, eps=1e-5)),
)
# (fft, hop, win) of framing 1 (reflect padding, center=False); 80 mels, 16 kHz, 80 .. Nyquist, ln, mag_eps 1e-9, floor 1e-5 as in the
# earlier loop's front-end
REFLECT = ((1024, 320, 1024), (1024, 321, 1024), (512, 128, 400), (2048, 512, 2048))


def centred_cases():
    """-> [(id, config)] of the whole-signal test's centred configurations."""
    out = [("-".join(str(v) for v in c), config(*c, **NO_CLIP)) for c in CENTRED]
    out += [("-".join(str(v) for v in c) + ("-ln" if kw.get("natural_log") else "-clip"), config(*c, **kw)) for c, kw in VARIANTS]
    return out


def reflect_cases():
    return [("reflect-%d-%d-%d" % c, config(c[0], c[1], c[2], 80, 16000, 80, -1, framing=1, natural_log=True, mag_eps=1e-9, eps=1e-5, **NO_CLIP))
            for c in REFLECT]


def lengths(p):
    """Signal lengths of a configuration: 1, hop - 1, n_fft / 2 - 1, exactly k hop, 3 rate / 10 + 57 (centred); pad + 1, pad + hop and
    one long length (reflect)."""
    N, hop, rate = p["fft_size"], p["hop_size"], p["sample_rate"]
    if p["framing"] == 0:
        return sorted({1, max(1, hop - 1), N // 2 - 1, 3 * hop, 3 * rate // 10 + 57})
    pad = (N - hop) // 2
    return [pad + 1, pad + hop, 3 * rate // 10 + 57]


# ---- the streaming tests: fft_size x {the full window, an odd shorter one} at the vocoder's hop and the Emformer's width
STREAM_FFT = (64, 128, 256, 512, 2048)
ODD_WIN = {64: 51, 128: 101, 256: 201, 512: 399, 2048: 1201}       # n_fft - win_length odd
STREAM_LENGTHS = (700, 1280, 3840, 5453, 2881)                     # 700, L, 3 L, 4 L + 333, 9 hop + 1 (hop 320, L = 4 hop)
STREAM_DIRECT = 5453                                               # the length whose first row is also held to the reference directly


def stream_cfgs(n_fft):
    """Two configurations per size: the full window and an odd shorter one.  64 runs 0 .. Nyquist (fmin = fmax = -1), 2048's short
    window runs ln with mag_eps, 512's short window runs the default clip; the others run with clipping off."""
    full = dict(fft_size=n_fft, win_length=n_fft, **NO_CLIP)
    short = dict(fft_size=n_fft, win_length=ODD_WIN[n_fft], **NO_CLIP)
    if n_fft == 64:
        full.update(fmin=-1, fmax=-1)
    if n_fft == 512:
        short = dict(fft_size=n_fft, win_length=ODD_WIN[n_fft])
    if n_fft == 2048:
        short.update(natural_log=True, mag_eps=1e-9, eps=1e-5)
    return full, short


def stream_seed(k, j):
    """Seed of the first (broadband) row of configuration k's utterance j in the common-position test."""
    return 10 * k + j


def ragged_seed(k, i):
    return 90 + 10 * k + i


def ragged_length(n_fft, k, i):
    """Length of slot i's utterance under configuration k in the ragged test: the slots of a call differ."""
    return STREAM_LENGTHS[(i + 2 * k + n_fft // 64) % len(STREAM_LENGTHS)]


def stream_direct_cases():
    """-> [(config, samples, seed)]: the broadband utterances the streaming tests hold to the reference directly."""
    out = []
    for n_fft in STREAM_FFT:
        for k, mel in enumerate(stream_cfgs(n_fft)):
            out.append((config(**mel), STREAM_DIRECT, stream_seed(k, STREAM_LENGTHS.index(STREAM_DIRECT))))
            out.append((config(**mel), ragged_length(n_fft, k, 0), ragged_seed(k, 0)))
    return out


@functools.lru_cache(maxsize=None)
def _case(key, samples, kind):
    p = dict(key)
    return reference(signal(kind, samples, p["sample_rate"]), p)


def case(p, samples, kind):
    """reference() of one configuration, length and signal, computed once per process (shared, read-only by convention)."""
    return _case(tuple(sorted(p.items())), samples, kind)
