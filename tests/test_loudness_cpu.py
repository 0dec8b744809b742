"""tests/loudness_ref.py - the numpy restatement of the loudness arithmetic in include/conan_hip.h - held to facts that do not come
from this project: the BS.1770 coefficient table, the standard's 997 Hz conformance sine, linearity, pyloudnorm's block edges and
scipy's lfilter.  No GPU."""
import numpy as np
import pytest

from tests import loudness_ref as LR


def test_48k_coefficients_against_the_bs1770_table():
    (sb, sa), (hb, ha) = LR.k_weighting(48000)
    assert sa[0] == 1.0 and ha[0] == 1.0
    dev_b = np.abs(np.array(sb) - [1.53512485958697, -2.69169618940638, 1.19839281085285]).max()
    dev_sa = np.abs(np.array(sa[1:]) - [-1.69065929318241, 0.73248077421585]).max()
    dev_ha = np.abs(np.array(ha[1:]) - [-1.99004745483398, 0.99007225036621]).max()
    print("deviation from the table: shelf b %.3g, shelf a %.3g, high-pass a %.3g; high-pass b factor %.6f" % (dev_b, dev_sa, dev_ha, hb[0]))
    assert dev_b <= 2e-4 and dev_sa <= 1e-4 and dev_ha <= 1e-4
    # the high-pass numerator is [1, -2, 1] times one factor (the table's is 1: pyloudnorm's known deviation)
    assert hb[1] == -2.0 * hb[0] and hb[2] == hb[0] and abs(hb[0] - 0.99504) < 1e-5


@pytest.mark.parametrize("fs", [48000, 16000])
def test_997hz_full_scale_sine_reads_minus_3_01(fs):
    x = np.sin(2 * np.pi * 997.0 * np.arange(3 * fs) / fs).astype(np.float32)
    L = LR.loudness(x, fs)
    print("997 Hz sine at %d Hz: %.4f LUFS" % (fs, L))
    assert abs(L - (-3.01)) <= 0.1


def test_scaling_moves_the_loudness_by_20_log10_k():
    rng = np.random.default_rng(5)
    x = (0.1 * rng.standard_normal(16000)).astype(np.float32)
    L = LR.loudness(x, 16000)
    for k in (0.5, 0.25, 4.0):          # powers of two: the scaled float32 samples are exact
        assert abs(LR.loudness((k * x).astype(np.float32), 16000) - (L + 20 * np.log10(k))) <= 1e-9


def test_block_edges():
    assert LR.block_edges(6400, 16000) == [(0, 6400)]
    assert LR.block_edges(7300, 16000) == [(0, 6400), (1600, 7300)]
    assert [lo for lo, _ in LR.block_edges(11025, 11025)][:5] == [0, 1102, 2205, 3307, 4410]
    with pytest.raises(ValueError):
        LR.measure(np.zeros(6399, np.float32), 16000)


def test_normalize_rules():
    rng = np.random.default_rng(6)
    x = (0.05 * rng.standard_normal(16000)).astype(np.float32)
    y, st = LR.normalize(x, 16000)
    assert abs(LR.loudness(y, 16000) - (-22.0)) < 1e-5 and st[3] >= 1
    z, zs = LR.normalize(np.zeros(8000, np.float32), 16000)
    assert not z.any() and zs[0] == -np.inf and zs[1] == 1.0 and zs[3] == 0
    s = (1e-3 * rng.standard_normal(32000)).astype(np.float32)
    s[::4000] = 1.0
    y, st = LR.normalize(s, 16000)
    assert st[2] > 1 and abs(np.abs(y).max() - 1.0) <= 2 ** -23
    y, st2 = LR.normalize(s, 16000, peak_limit=False)
    assert abs(np.abs(y).max() - st2[2]) <= 1e-6 * st2[2] and st2[1] > st[1]


def test_loop_equals_scipy_lfilter():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(7)
    x = rng.standard_normal(4000).astype(np.float32)
    for fs in (8000, 16000, 48000):
        shelf, hp = LR.k_weighting(fs)
        ref = signal.lfilter(hp[0], hp[1], signal.lfilter(shelf[0], shelf[1], x.astype(np.float64)))
        got = LR.k_filter(x, fs)
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
