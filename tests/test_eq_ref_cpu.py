"""The equaliser's reference (tests/eq_ref.py) alone: the law's cut independence, its distance from scipy.signal.sosfilt, the design
formulas against the library's host-only helper, physical checks of the designed sections, and the state record's size."""
import numpy as np
import pytest

from conan_amd import _lib
from tests import eq_ref as R

RATE = 16000.0
N = 16077
CUTS = [1280, 1280, 333, 1, 127, 128, 129, 1000]


@pytest.fixture(scope="module")
def whole():
    x = R.signal(N, seed=1)
    y, s = R.run(x, R.cascade4(), f64=True)
    return x, y, s


def test_cut_independence(whole):
    x, y, s = whole
    z, t = R.run(x, R.cascade4(), cuts=CUTS, f64=True)
    assert np.array_equal(y.view(np.uint64), z.view(np.uint64))
    assert t.state_bytes() == s.state_bytes() and len(s.state_bytes()) == R.STATE_BYTES
    one, _ = R.run(x[:700], R.cascade4(), cuts=[1], f64=True)
    assert np.array_equal(one.view(np.uint64), y[:700].view(np.uint64))


def test_live_change_is_cut_independent_and_continuous():
    x = R.signal(3000, seed=2)
    alt = [R.cookbook("peak", RATE, 1800.0, 1.5, 4.0)]
    a, _ = R.run(x, R.cascade4(), changes=[(1301, alt)], f64=True)
    b, _ = R.run(x, R.cascade4(), cuts=CUTS, changes=[(1301, alt)], f64=True)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert np.array_equal(a[:1301], R.run(x[:1301], R.cascade4(), f64=True)[0])
    # no click: section 0 keeps its state, so the step across the change is of the size of the steps around it
    steps = np.abs(np.diff(a))
    assert steps[1300] < 4.0 * steps[1200:1400].mean() + 1e-3


def test_against_sosfilt(whole):
    signal = pytest.importorskip("scipy.signal")
    x, y, _ = whole
    sos = np.asarray([[c[0], c[1], c[2], 1.0, c[3], c[4]] for c in R.cascade4()])
    want = signal.sosfilt(sos, x.astype(np.float64))
    own = np.abs(y - R.direct(x, R.cascade4())).max()      # what the segmenting itself costs
    diff = np.abs(y - want).max()
    print("segmented vs direct %.3g, vs sosfilt %.3g, peak %.3g" % (own, diff, np.abs(want).max()))
    assert own > 0.0 and diff <= 64.0 * own
    a, b = y.astype(np.float32), want.astype(np.float32)
    bad = np.flatnonzero(a != b)
    print("f32 samples that differ: %d of %d" % (bad.size, N))
    assert bad.size <= N // 1000
    assert (np.abs(a[bad].view(np.int32).astype(np.int64) - b[bad].view(np.int32).astype(np.int64)) == 1).all()


DESIGNS = [(k, f, q, g) for k in R.KINDS for f, q, g in ((80.0, 0.7071, 0.0), (50.0, 30.0, -12.0), (2500.0, 1.0, 6.0), (3400.0, 0.5, 12.0), (7900.0, 2.0, -3.0))]


@pytest.mark.parametrize("rate", [16000.0, 8000.0, 48000.0])
def test_design_matches_the_restatement(rate):
    for kind, f, q, g in DESIGNS:
        if f >= rate / 2:
            continue
        got, want = _lib.eq_section(kind, rate, f, q, g), R.cookbook(kind, rate, f, q, g)
        for c, w in zip(got, want):
            assert abs(c - w) <= 64.0 * 2.0 ** -52 * max(1.0, abs(w)), (kind, rate, f, q, g, c, w)
        assert R.stable(got), (kind, f, q, g)
        if kind in ("dcblock", "deemphasis"):
            assert got[2] == 0.0 and got[4] == 0.0


def test_design_refusals():
    for args in (("lowpass", 16000.0, 0.0), ("lowpass", 16000.0, 8000.0), ("lowpass", 16000.0, -5.0), ("peak", 16000.0, 100.0, 0.0),
                 ("peak", 16000.0, 100.0, -1.0), ("peak", 16000.0, float("nan")), ("peak", 16000.0, 100.0, 1.0, float("inf")),
                 ("notch", float("inf"), 100.0), ("highshelf", 16000.0, 100.0, 1.0, 61.0)):
        with pytest.raises(_lib.ConanError) as e:
            _lib.eq_section(*args)
        assert e.value.code == _lib.ERR_INVALID, args
    with pytest.raises(ValueError):
        _lib.eq_section("brickwall", 16000.0, 100.0)


def test_physical_checks():
    hp = [R.cookbook("highpass", RATE, 80.0)]
    y, _ = R.run(np.full(8000, 0.2, dtype=np.float32), hp, f64=True)      # half a second
    assert np.abs(y[-1]) < 1e-4
    pk = [R.cookbook("peak", RATE, 2500.0, 1.0, 6.0)]
    assert abs(20.0 * np.log10(R.response(pk, 2500.0, RATE)) - 6.0) < 0.01
    t = np.arange(16000) / RATE
    tone = np.sin(2 * np.pi * 2500.0 * t).astype(np.float32)
    y, _ = R.run(tone, pk, f64=True)
    gain = 20.0 * np.log10(np.sqrt(np.mean(y[8000:] ** 2)) / np.sqrt(np.mean(tone[8000:].astype(np.float64) ** 2)))
    assert abs(gain - 6.0) < 0.01, gain
    nt = [R.cookbook("notch", RATE, 50.0, 30.0)]
    hum = np.sin(2 * np.pi * 50.0 * np.arange(32000) / RATE).astype(np.float32)
    y, _ = R.run(hum, nt, f64=True)
    left = 20.0 * np.log10(np.sqrt(np.mean(y[24000:] ** 2)) / np.sqrt(0.5))
    assert left < -40.0, left


def test_state_record_size():
    assert R.STATE_BYTES == int(_lib.lib().conan_eq_state_bytes()) == 592
    assert len(R.Stream(R.cascade4()).state_bytes()) == R.STATE_BYTES
    assert R.SEG == _lib.EQ_SEG and R.MAX_SECTIONS == _lib.EQ_MAX_SECTIONS and R.MAX_COEF == _lib.EQ_MAX_COEF
