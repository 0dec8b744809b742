"""Properties of the bypass law as tests/bypass_ref.py states it (no GPU): what the header promises of the mix follows from the law."""
from fractions import Fraction

import numpy as np

from tests import bypass_ref as B

HOP = 320
FULL = B.FULL


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _sig(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n).astype(np.float32), (0.3 * rng.standard_normal(n)).astype(np.float32)


def test_fma32_is_correctly_rounded():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(4000).astype(np.float32)
    g = rng.random(4000).astype(np.float32)
    t = (rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 2, 4000)).astype(np.float32)
    # cases built to sit next to a rounding boundary of f32: t = a tie of the product's neighbourhood
    x[:8] = np.float32(1.0) + np.float32(2.0 ** -23) * np.arange(8, dtype=np.float32)
    g[:8] = np.float32(1.0) - np.float32(2.0 ** -24)
    t[:8] = np.float32(2.0 ** -25)
    got = B.fma32(x, g, t)
    for i in range(x.shape[0]):
        exact = Fraction(float(x[i])) * Fraction(float(g[i])) + Fraction(float(t[i]))
        r = np.float32(float(exact))      # float(Fraction) rounds once to f64; check the f32 candidates around it exactly
        cands = [np.nextafter(r, np.float32(-np.inf)), r, np.nextafter(r, np.float32(np.inf))]
        best = min(cands, key=lambda c: (abs(Fraction(float(c)) - exact), int(np.float32(c).view(np.uint32)) & 1))
        assert got[i] == best, (i, x[i], g[i], t[i])


def test_full_wet_keeps_the_bits_and_full_dry_gives_the_source():
    y, x = _sig(5 * HOP + 77, 1)
    y[3], x[5], y[5] = -0.0, -0.0, 1.0
    F = 6
    full, zero = np.full(F, FULL, dtype=np.int32), np.zeros(F, dtype=np.int32)
    assert np.array_equal(_bits(B.mix(y, x, full, zero, FULL, 0, HOP)), _bits(y))
    out = B.mix(y, x, zero, full, 0, FULL, HOP)
    assert np.array_equal(out, x)      # in value: y * 0 is a zero of either sign, and x + (-0) keeps x but 0 + -0 = +0
    assert _bits(out)[5] == 0 and _bits(x)[5] == 0x80000000      # the one place the bits differ: +0 + -0 = +0


def test_a_sequence_cut_at_any_frame_boundary_gives_the_same_samples():
    F = 9
    y, x = _sig(F * HOP, 2)
    gate = np.array([FULL, FULL, 700000, 300000, 0, 0, 400000, FULL, FULL], dtype=np.int32)
    for fill in (False, True):
        st0 = B.seed_state(FULL, 0, fill, gate_before=FULL)
        w, d, _ = B.levels(st0, 200000, 900000, 150000, F, fill, gate)
        whole = B.mix(y, x, w, d, st0["wet"], st0["dry_eff"], HOP)
        for cut in range(1, F):
            w1, d1, st1 = B.levels(st0, 200000, 900000, 150000, cut, fill, gate[:cut])
            w2, d2, _ = B.levels(st1, 200000, 900000, 150000, F - cut, fill, gate[cut:])
            assert np.array_equal(np.concatenate([w1, w2]), w) and np.array_equal(np.concatenate([d1, d2]), d)
            a = B.mix(y[:cut * HOP], x[:cut * HOP], w1, d1, st0["wet"], st0["dry_eff"], HOP)
            b = B.mix(y[cut * HOP:], x[cut * HOP:], w2, d2, st1["wet"], st1["dry_eff"], HOP)
            assert np.array_equal(_bits(np.concatenate([a, b])), _bits(whole)), (fill, cut)


def test_the_fill_is_zero_under_an_open_gate_and_dry_under_a_closed_one():
    st0 = B.seed_state(FULL, 123456, True, gate_before=FULL)
    assert st0["dry_eff"] == 0
    _, d, _ = B.levels(st0, FULL, 123456, FULL, 4, True, np.full(4, FULL))
    assert not d.any()
    _, d, _ = B.levels(st0, FULL, 123456, FULL, 4, True, np.zeros(4, dtype=np.int64))
    assert (d == 123456).all()
    _, d, _ = B.levels(st0, FULL, 123456, FULL, 4, False, np.zeros(4, dtype=np.int64))
    assert (d == 123456).all()
    _, d, _ = B.levels(st0, FULL, FULL, FULL, 1, True, [FULL // 4])
    assert d[0] == 3 * FULL // 4
    # an absent gate counts as open: nothing is filled
    _, d, _ = B.levels(st0, FULL, 123456, FULL, 3, True, None)
    assert not d.any()
    # with the gate open all the way, a filling slot at full wet keeps the vocoder's bits
    y, x = _sig(3 * HOP, 3)
    w, d, _ = B.levels(st0, FULL, 123456, FULL, 3, True, np.full(3, FULL))
    assert np.array_equal(_bits(B.mix(y, x, w, d, st0["wet"], st0["dry_eff"], HOP)), _bits(y))


def test_the_slew_reaches_its_target_in_ceil_delta_over_step_frames():
    for start, target, step in ((0, FULL, FULL // 2), (FULL, 0, FULL // 3), (100, 100, 7), (5, FULL - 3, 99999), (FULL, 17, 1 << 19), (0, 1, FULL)):
        need = -(-abs(target - start) // step)
        w, _, st = B.levels(dict(wet=start, dry=0, dry_eff=0), target, 0, step, need + 2)
        assert all(w[f] != target for f in range(need - 1)) and (need == 0 or w[need - 1] == target) and st["wet"] == target
        assert all(abs(int(b) - int(a)) <= step for a, b in zip([start] + list(w), w))
        assert (np.diff(np.concatenate([[start], w])) * np.sign(target - start) >= 0).all()      # monotonic, no overshoot
