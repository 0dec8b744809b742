"""The source-pitch tracker's reference (tests/f0_ref.py, the law of include/conan_hip.h, conan_f0_cfg) on its own: it reads what a
pitch tracker should read, and every decision it makes on the signals of tests/test_gpu_f0.py has room to spare, so the GPU
comparison leaves no frame out."""
import numpy as np
import pytest

from tests import f0_ref as R

SR = 16000


@pytest.mark.parametrize("f", [80.0, 150.0, 440.0, 850.0])
def test_harmonic_tones_read_within_half_a_percent(f):
    r = R.judge(R.harmonic(f, 8000))
    inner = slice(2, -2)      # (the first and last frames are half zero padding)
    assert (r["uv"][inner] == 0).all()
    assert np.abs(r["f0"][inner] / f - 1).max() < 0.005
    assert np.array_equal(r["v"][inner], np.log2(r["f0"][inner]).astype(np.float32))
    assert (np.abs(R.lag_of(r["v"], r["uv"]) - r["lag"])[r["uv"] == 0] <= 1).all()


def test_glide_follows_the_frame_centre_and_leaves_gap_and_burst_unvoiced():
    N = SR
    r = R.judge(R.glide(N, gap=(4000, 6000), burst=(10000, 12000)))
    true = 110.0 * 3.0 ** (np.arange(len(r["uv"])) * 320 / SR)
    v = r["uv"] == 0
    assert v.sum() >= 30
    assert np.abs(r["f0"][v] / true[v] - 1).max() < 0.017
    centre = np.arange(len(v)) * 320
    for lo, hi in ((4000, 6000), (10000, 12000)):
        inside = (centre - 512 >= lo) & (centre + 512 <= hi)      # frames wholly inside the gap / the burst
        assert inside.any() and not v[inside].any()


def test_silence_and_noise_are_unvoiced():
    assert (R.judge(np.zeros(6400, np.float32))["uv"] == 1).all()
    noise = (0.1 * np.random.default_rng(0).standard_normal(6400)).astype(np.float32)
    r = R.judge(noise)
    assert (r["uv"] == 1).all() and (r["v"] == 0).all()


def test_speech_band_test_signals_are_mostly_voiced():
    for x in R.sig(4, SR, SR, 5):
        r = R.judge(x)
        assert len(r["uv"]) == 51 and (r["uv"] == 0).sum() >= 48


def test_an_utterance_shorter_than_one_frame():
    for n in (1, 17, 319):
        r = R.judge(R.harmonic(200.0, n))
        assert len(r["uv"]) == 1
    r = R.judge(R.harmonic(200.0, 700))
    assert len(r["uv"]) == 3


def test_limits_are_refused():
    x = np.zeros(4000, np.float32)
    for kw in (dict(fmax=8001.0), dict(fmin=31.0), dict(fmin=500.0, fmax=500.0), dict(N=512, fmin=50.0)):
        with pytest.raises(ValueError):
            R.judge(x, **kw)
    R.judge(x, fmin=31.25, fmax=8000.0)


def test_every_decision_on_the_gpu_tests_signals_has_margin():
    """Every comparison the law makes - threshold tests, the walk, the gate, the denominator's sign - on every frame of every signal
    tests/test_gpu_f0.py compares with this reference is at least 1e-6 away from equality: the GPU's f64 sums in another order
    (relative differences of 1e-13) cannot turn one, and the cap on frames left out of the GPU comparison is zero."""
    for name, (x, kw) in R.gpu_signals().items():
        r = R.judge(x, **kw)
        assert r["margin"].min() >= 1e-6, (name, r["margin"].min(), int(r["margin"].argmin()))
