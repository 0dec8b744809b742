"""tests/frontend_ref.py pinned, and its bound shown to have teeth (CPU only):
  - the float64 reference agrees with oracle/frontend.py at the defaults (both framings) to the tolerances tests/test_oracle_frontend.py
    uses for its own pins, and with that file's explicit-DFT construction at a non-default configuration;
  - a numpy emulation of the kernels' arithmetic (f32 products, f64 sums, f32 |X|, f64 filterbank sum rounded to f32, f32 log) stays
    inside frontend_ref.bound on every configuration, length and signal of tests/test_gpu_frontend_f64.py;
  - three mutants of that emulation break it: the DFT accumulated in f32, the window placed at lp + 1, each triangle's last non-zero
    bin dropped;
  - on the broadband signal with clipping off no element of a non-empty filter sits on the eps floor (else the GPU test would compare
    floor with floor)."""
import functools

import numpy as np
import pytest

from oracle import frontend as ofe
from tests import frontend_ref as fr

CENTRED = fr.centred_cases()
REFLECT = fr.reflect_cases()
ALL = CENTRED + REFLECT
IDS = [c[0] for c in ALL]


@functools.lru_cache(maxsize=None)
def _twiddles(N):
    """(cos, sin)(2 pi ((t b) mod N) / N) as the kernels read them from their f64 table: [N, N / 2 + 1] each."""
    tb = np.outer(np.arange(N), np.arange(N // 2 + 1)) % N
    tab_c, tab_s = np.cos(2.0 * np.pi * np.arange(N) / N), np.sin(2.0 * np.pi * np.arange(N) / N)
    return tab_c[tb], tab_s[tb]


def emulate(wav, p, dft="f64", win=None, fb=None):
    """The kernels' arithmetic (stft_frames_kernel -> dft_mag_kernel -> mel_log_kernel) in numpy -> [frames, n_mels] float32.
    dft='f32': the mutant that accumulates the DFT sums in f32, term after term as the kernel's chain does.  win / fb: a mutant's
    window / filterbank."""
    x = fr.frames_f32(wav, p, win)
    C, S = _twiddles(p["fft_size"])
    if dft == "f64":
        re, im = x.astype(np.float64) @ C, x.astype(np.float64) @ S
    else:
        C32, S32 = C.astype(np.float32), S.astype(np.float32)
        re, im = np.zeros((x.shape[0], C.shape[1]), np.float32), np.zeros((x.shape[0], C.shape[1]), np.float32)
        for t in range(p["fft_size"]):
            re += x[:, t, None] * C32[t][None, :]
            im += x[:, t, None] * S32[t][None, :]
        assert re.dtype == np.float32
        re, im = re.astype(np.float64), im.astype(np.float64)
    mag = np.sqrt(re * re + im * im + np.float64(np.float32(p["mag_eps"]))).astype(np.float32)
    fb = fr.filterbank(p["sample_rate"], p["fft_size"], p["num_mels"], p["fmin"], p["fmax"]) if fb is None else fb
    s = (mag.astype(np.float64) @ fb.astype(np.float64).T).astype(np.float32)
    c = np.maximum(np.float32(p["eps"]), s)
    v = np.log(c) if p["natural_log"] else np.log10(c)
    assert v.dtype == np.float32
    return np.clip(v, np.float32(p["mel_vmin"]), np.float32(p["mel_vmax"]))


def _ratio(got, ref, p, K=fr.K_LOG):
    return np.abs(got.astype(np.float64) - ref["mel"]) / fr.bound(ref, p, K)


# ---- the reference is the oracle's front-end, in float64
def _oracle_signal(seed=3, dur=1.3, extra=57):
    rng = np.random.default_rng(seed)
    t = np.arange(int(dur * 16000) + extra) / 16000
    return (0.5 * np.sin(2 * np.pi * 220 * t) * np.exp(-t) + 0.1 * np.sin(2 * np.pi * 3100 * t) + 0.02 * rng.standard_normal(t.shape)).astype(np.float32)


def test_reference_agrees_with_the_oracle_at_the_defaults():
    """oracle/frontend.py::wav2mel (a float32 FFT) to 1e-5 on broadband signals and 1e-3 on the pure tone (its bins 6 decades down
    carry the oracle's complex64 rounding), torch_mel_spectrogram to 2e-4: the tolerances of tests/test_oracle_frontend.py's pins."""
    p = fr.config()
    tone = (0.9 * np.sin(2 * np.pi * 440 * np.arange(9000) / 16000)).astype(np.float32)
    for wav, tol in ((_oracle_signal(), 1e-5), (_oracle_signal(5, 0.4, 0), 1e-5), (tone, 1e-3)):
        ref, want = fr.reference(wav, p)["mel"], ofe.wav2mel(wav)
        assert ref.shape == want.shape and ref.dtype == np.float64
        assert np.abs(ref - want).max() < tol, np.abs(ref - want).max()
    q = fr.config(fmax=-1, framing=1, natural_log=True, mag_eps=1e-9, eps=1e-5, **fr.NO_CLIP)
    for wav in (_oracle_signal(), _oracle_signal(5, 0.4, 0)):
        ref, want = fr.reference(wav, q)["mel"], ofe.torch_mel_spectrogram(wav).T
        assert ref.shape == want.shape == (len(wav) // 320, 80)
        assert np.abs(ref - want).max() < 2e-4, np.abs(ref - want).max()


def test_reference_agrees_with_explicit_dft_sums_off_the_defaults():
    """The construction of tests/test_oracle_frontend.py::test_stft_matches_explicit_dft_sums (zero-padded frames, the window from
    its formula, a dense float64 DFT matrix) at n_fft 256, hop 80, and with a shorter, odd window placed by pad_center."""
    x = _oracle_signal(0, 0.1, 0)
    for n_fft, hop, wl in ((256, 80, 256), (256, 80, 199)):
        p = fr.config(n_fft, hop, wl, 40, 8000, 0, 4000)
        mag = fr.magnitudes(fr.frames_f32(x, p), p)
        assert mag.shape == (1 + len(x) // hop, n_fft // 2 + 1)
        k = np.arange(n_fft)
        lp = (n_fft - wl) // 2
        win = np.where((k >= lp) & (k < lp + wl), 0.5 - 0.5 * np.cos(2 * np.pi * (k - lp) / wl), 0.0)
        y = np.concatenate([np.zeros(n_fft // 2), x.astype(np.float64), np.zeros(n_fft // 2)])
        dft = np.exp(-2j * np.pi * np.outer(np.arange(n_fft // 2 + 1), k) / n_fft)
        for f in (0, 1, 7, mag.shape[0] - 1):
            want = np.abs(dft @ (y[f * hop:f * hop + n_fft] * win))
            np.testing.assert_allclose(mag[f], want, rtol=1e-4, atol=1e-4)
    assert np.array_equal(fr.filterbank(16000, 1024, 80, 80, 7600), ofe.mel_filterbank(16000, 1024, 80, 80, 7600))


def test_shapes_follow_conan_mel_frames():
    for _, p in ALL:
        for n in fr.lengths(p):
            ref = fr.case(p, n, "silence")
            assert ref["mel"].shape == (fr.n_frames(p, n), p["num_mels"]) and ref["mel"].shape[0] >= 1, (p, n)


# ---- the emulation stays inside the bound on every input of the GPU test
@pytest.mark.parametrize("name,p", ALL, ids=IDS)
def test_emulation_within_bound(name, p):
    worst = 0.0
    for n in fr.lengths(p):
        for kind in fr.SIGNALS:
            ref = fr.case(p, n, kind)
            r = _ratio(emulate(fr.signal(kind, n, p["sample_rate"]), p), ref, p)
            assert r.max() <= 1.0, (name, n, kind, r.max())
            worst = max(worst, r.max())
    print(f"emulation {name}: worst error / bound = {worst:.3f}")


def test_emulation_within_bound_on_the_streamed_utterances():
    """The utterances tests/test_gpu_frontend_f64.py's streaming tests hold to the reference directly; none sits on the floor either."""
    for p, n, seed in fr.stream_direct_cases():
        wav = fr.signal("broadband", n, p["sample_rate"], seed)
        ref = fr.reference(wav, p)
        r = _ratio(emulate(wav, p), ref, p)
        assert r.max() <= 1.0, (p, n, seed, r.max())
        assert (ref["s"][:, ref["nonempty"]] > np.float64(np.float32(p["eps"]))).all(), (p, n, seed)


# ---- mutants: each must break the bound
def _long(p):
    return fr.lengths(p)[-1]


@pytest.mark.parametrize("name,p", [c for c in CENTRED if c[1]["fft_size"] <= 1024], ids=[c[0] for c in CENTRED if c[1]["fft_size"] <= 1024])
def test_mutant_f32_dft_breaks_the_bound(name, p):
    """The pure tone: its quiet bins lie 6 decades below the peak, where an f32 chain's rounding (relative to the frame's sum of
    magnitudes) shows.  Between the 64- and 1024-point configurations."""
    n = _long(p)
    r = _ratio(emulate(fr.signal("tone", n, p["sample_rate"]), p, dft="f32"), fr.case(p, n, "tone"), p)
    print(f"f32 DFT {name}: worst error / bound = {r.max():.2f}")
    assert r.max() > 1.0, (name, r.max())


@pytest.mark.parametrize("name,p", [c for c in ALL if c[1]["win_length"] < c[1]["fft_size"]], ids=[c[0] for c in ALL if c[1]["win_length"] < c[1]["fft_size"]])
def test_mutant_window_offset_breaks_the_bound(name, p):
    """pad_center off by one sample: wherever win_length < fft_size, more than 90 % of the elements of non-empty filters leave the bound."""
    n = _long(p)
    ref = fr.case(p, n, "broadband")
    win = np.roll(fr.window(p["fft_size"], p["win_length"]), 1)
    assert win[0] == 0.0
    r = _ratio(emulate(fr.signal("broadband", n, p["sample_rate"]), p, win=win), ref, p)[:, ref["nonempty"]]
    print(f"window offset {name}: worst error / bound = {r.max():.3g}, share outside = {(r > 1).mean():.4f}")
    assert r.max() > 1.0 and (r > 1.0).mean() >= 0.9, (name, r.max(), (r > 1.0).mean())


@pytest.mark.parametrize("name,p", ALL, ids=IDS)
def test_mutant_dropped_last_bin_breaks_the_bound(name, p):
    """Each triangle loses its last non-zero bin (a bin range one short): at fft_size >= 256 more than 90 % of the elements of non-empty
    filters leave the bound; below, the bound still breaks."""
    n = _long(p)
    ref = fr.case(p, n, "broadband")
    fb = fr.filterbank(p["sample_rate"], p["fft_size"], p["num_mels"], p["fmin"], p["fmax"]).copy()
    for m in np.nonzero(ref["nonempty"])[0]:
        fb[m, np.nonzero(fb[m])[0][-1]] = 0.0
    r = _ratio(emulate(fr.signal("broadband", n, p["sample_rate"]), p, fb=fb), ref, p)[:, ref["nonempty"]]
    print(f"dropped bin {name}: worst error / bound = {r.max():.3g}, share outside = {(r > 1).mean():.4f}")
    assert r.max() > 1.0, (name, r.max())
    if p["fft_size"] >= 256:
        assert (r > 1.0).mean() >= 0.9, (name, (r > 1.0).mean())


# ---- coverage: the broadband signal keeps every non-empty filter off the floor
@pytest.mark.parametrize("name,p", ALL, ids=IDS)
def test_broadband_never_sits_on_the_floor(name, p):
    eps = np.float64(np.float32(p["eps"]))
    for n in fr.lengths(p):
        ref = fr.case(p, n, "broadband")
        assert ref["nonempty"].any()
        s = ref["s"][:, ref["nonempty"]]
        assert (s > eps).all(), (name, n, s.min(), int((s <= eps).sum()))
        sil = fr.case(p, n, "silence")
        if p["mag_eps"] == 0.0:
            assert (sil["s"] == 0.0).all()


def test_empty_filters_of_the_64_point_configuration():
    """32 of the 80 filters of (64, ., ., 80, 16000, 0, Nyquist) see no FFT bin."""
    fb = fr.filterbank(16000, 64, 80, -1, -1)
    assert int((~fr.nonempty(fb)).sum()) == 32
