"""tests/comfort_ref.py against known answers and against the properties the law was chosen for: the hash, the quantised power, the
amplitude of a level, the level of the coloured noise, how well a quantised power gives the amplitude back, and the tracker."""
import types

import numpy as np
import pytest

from tests import comfort_ref as R


def test_hash_known_answers():
    assert R.hash64(0, 0) == 0xE220A8397B1DCDAF
    assert R.hash64(0, 1) == 0x6E789E6AA1B965F4
    # the vector form is the scalar one, also before sample 0 and past 2^33
    for seed, j0 in ((0, 0), (7, -4), (0xFFFFFFFFFFFFFFFF, 2 ** 33 + 5), (123456789, -1)):
        got = R.white(seed, j0, 9)
        assert [int(v) for v in got] == [R.white1(seed, j0 + k) for k in range(9)], (seed, j0)
        assert int(np.abs(got).max()) <= 65535
    # a coloured sample is its taps on the white ones
    for colour, taps in enumerate(R.TAPS):
        v = R.coloured(5, 10, 6, colour)
        assert [int(x) for x in v] == [sum(c * R.white1(5, 10 + k - i) for i, c in enumerate(taps)) for k in range(6)]


def test_quantised_power_and_amplitude():
    assert R.lq(1.0) == 0 and R.lq(0.5) == -256 and R.lq(0.0) == -261888
    assert R.lq(0.25) == -512 and R.lq(5e-324) == -261888
    assert R.amplitude(0) == 1.0 and R.amplitude(-512) == 0.5 and R.amplitude(-10240) == 2.0 ** -20
    assert R.amplitude(-256) == 0.75 and R.amplitude(-1) == np.float32(1023.0 / 1024.0)      # the linear piece inside an octave
    lv = np.arange(R.LEVEL_MIN, 1)
    a = R.amplitudes(lv, 1.0)
    assert all(a[i] == R.amplitude(int(lv[i])) for i in range(0, lv.size, 97))
    assert bool((np.diff(a.astype(np.float64)) > 0).all())      # strictly rising in L


@pytest.mark.parametrize("colour", [0, 1, 2])
def test_noise_rms_is_one_at_level_zero(colour):
    v = R.coloured(7, 0, 160000, colour).astype(np.float64) * float(R.norm(colour))
    db = 20.0 * np.log10(np.sqrt(np.mean(v * v)))
    print("colour", colour, "rms dB", db)
    assert abs(db) < 0.1


def test_amplitude_of_a_quantised_power():
    P = np.logspace(-9, -1, 20001)
    err = np.array([20.0 * np.log10(float(R.amplitude(R.lq(p))) / np.sqrt(p)) for p in P])
    print("a(Lq(P)) / sqrt(P), dB:", err.min(), err.max())
    assert -0.05 <= err.min() and err.max() <= 0.55


def _cfg(**kw):
    base = dict(mode=2, level=-5000, offset=0, l_min=-8000, l_max=-2000, up_step=20, down_step=170)
    return types.SimpleNamespace(**dict(base, **kw))


def test_tracker():
    idle = dict(level=-5000, idle_frames=0)
    # a step up is limited by up_step, a step down by down_step
    lv, st = R.track(idle, _cfg(), [0] * 5, [2.0 ** -10] * 5)      # Lq = -2560
    assert list(lv) == [-4980, -4960, -4940, -4920, -4900] and st == dict(level=-4900, idle_frames=5)
    lv, st = R.track(idle, _cfg(), [0] * 4, [2.0 ** -28] * 4)      # Lq = -7168
    assert list(lv) == [-5170, -5340, -5510, -5680] and st["idle_frames"] == 4
    # it arrives exactly, with the offset
    lv, _ = R.track(dict(level=-2570, idle_frames=0), _cfg(offset=-30), [0] * 3, [2.0 ** -10] * 3)
    assert list(lv) == [-2590, -2590, -2590]
    # the level holds over active frames, which are not counted
    lv, st = R.track(idle, _cfg(), [1, 1, 0, 1], [1.0, 1.0, 2.0 ** -10, 1.0])
    assert list(lv) == [-5000, -5000, -4980, -4980] and st["idle_frames"] == 1
    # the clamps: a silent frame aims at l_min, a loud one at l_max
    lv, _ = R.track(dict(level=-7900, idle_frames=0), _cfg(), [0, 0], [0.0, 0.0])
    assert list(lv) == [-8000, -8000]
    lv, _ = R.track(dict(level=-2010, idle_frames=0), _cfg(), [0, 0], [1.0, 1.0])
    assert list(lv) == [-2000, -2000]
    # fixed mode gives the fixed level, clamped, on every frame
    lv, st = R.track(idle, _cfg(mode=1, level=-3000), [0, 1, 0], [0.0] * 3)
    assert list(lv) == [-3000] * 3 and st == dict(level=-3000, idle_frames=0)
    lv, _ = R.track(idle, _cfg(mode=1, level=-100), [1], [0.0])
    assert list(lv) == [-2000]


def test_fill_keeps_an_open_gate_and_fills_a_closed_one():
    hop, F = 8, 6
    rng = np.random.default_rng(0)
    y = rng.standard_normal(F * hop).astype(np.float32)
    nrm = R.norm(1)
    out = R.fill(y, [R.FULL] * F, [-2000] * F, R.FULL, hop, 9, 1, nrm)
    assert np.array_equal(out.view(np.uint32), y.view(np.uint32))
    gate = [R.FULL, 0, 0, 0, R.FULL, R.FULL]
    out = R.fill(np.zeros(F * hop, np.float32), gate, [-2000] * F, R.FULL, hop, 9, 1, nrm)
    assert not out[:hop].any() and not out[5 * hop:].any() and out[5 * hop - 1] == 0 and out[5 * hop - 2] != 0     # open frames, and the last sample of an opening ramp
    v = R.coloured(9, 0, F * hop, 1)
    A = np.float32(R.amplitude(-2000) * nrm)
    want = (v[2 * hop:4 * hop].astype(np.float32) * A).astype(np.float32)      # a closed gate: gc = 1, out = t
    assert np.array_equal(out[2 * hop:4 * hop], want)
    # a position: the noise of sample s at pos0 is that of sample pos0 + s
    a = R.fill(np.zeros(2 * hop, np.float32), [0, 0], [-2000] * 2, 0, hop, 9, 2, nrm, pos0=2 ** 33 + 5)
    assert a[3] == np.float32(np.float32(R.coloured(9, 2 ** 33 + 8, 1, 2)[0]) * A)
