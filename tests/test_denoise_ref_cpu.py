"""The noise suppressor's numpy reference (tests/denoise_ref.py) against itself and against a scalar restatement of the law in Python
integers: cutting a row into pieces through the state, the fixed point on a constant mel, the bins that must keep their bits, the
cross-bin edges at one and two bins, NaN and out-of-range values, and the branch counters."""
import math
import struct

import numpy as np
import pytest

from conan_amd import _lib
from tests import denoise_ref as R

F32 = np.float32
DEFAULT = R.fields(_lib.denoise_cfg())
# every clamp governs: a floor_min above the quiet frames, a shallow depth, small steps, an out_floor above the attenuated values
CLAMPS = dict(bias=200, knee=900, slope=1024, depth=700, close_step=150, open_step=120, rise=40, fall_shift=2, floor_min=-4500, smooth=1, out_floor=-4.25)
PLAIN = dict(DEFAULT, smooth=0, fall_shift=0)


def noisy(T, nm, seed):
    """Bursts over a noise floor, with pauses well under it: values in the mel's range [-6, 1.5]."""
    rng = np.random.default_rng(seed)
    x = -4.0 + 0.3 * rng.standard_normal((T, nm))
    x[T // 4:T // 2, nm // 3:] += 3.0 * rng.random((T // 2 - T // 4, nm - nm // 3))
    x[T // 2:T // 2 + max(T // 8, 1)] = -5.9
    return np.clip(x, -6.0, 1.5).astype(F32)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_state(a, b):
    return R.state_bytes(a) == R.state_bytes(b)


def scalar(mel, p, state=None):
    """The law once more, one bin at a time in Python integers (the struct module rounds the output to f32)."""
    T, nm = mel.shape
    f32 = lambda v: struct.unpack("<f", struct.pack("<f", v))[0]      # noqa: E731
    N, A = (None, None) if state is None else (list(state[0]), list(state[1]))
    y = mel.copy()
    for f in range(T):
        L = []
        for b in range(nm):
            v = float(mel[f, b])
            v = -1024.0 if math.isnan(v) else min(max(v, -1024.0), 1024.0)
            t = v * 1024.0
            r = math.floor(t)
            L.append(r + (1 if t - r > 0.5 or (t - r == 0.5 and r % 2) else 0))
        if N is None:
            N, A = [max(l, p["floor_min"]) for l in L], [0] * nm
        a = [min((max(p["knee"] - (L[b] - (N[b] + p["bias"])), 0) * p["slope"]) >> 8, p["depth"]) for b in range(nm)]
        if p["smooth"]:
            a = [(a[max(b - 1, 0)] + 2 * a[b] + a[min(b + 1, nm - 1)] + 2) >> 2 for b in range(nm)]
        for b in range(nm):
            A[b] = min(A[b] + p["close_step"], a[b]) if a[b] > A[b] else max(A[b] - p["open_step"], a[b])
            if A[b]:
                y[f, b] = max(f32((L[b] - A[b]) * 0.0009765625), float(p["out_floor"]))
            if L[b] < N[b]:
                n = N[b] - ((N[b] - L[b] + (1 << p["fall_shift"]) - 1) >> p["fall_shift"])
            else:
                n = min(L[b], N[b] + p["rise"])
            N[b] = max(n, p["floor_min"])
    return y, (N, A)


@pytest.mark.parametrize("cfg", [DEFAULT, PLAIN, CLAMPS], ids=["default", "plain", "clamps"])
def test_pieces_equal_the_whole_for_every_cut(cfg):
    x = noisy(40, 7, 1)
    y, st = R.denoise(x, cfg)
    for cut in range(41):
        y0, s0 = R.denoise(x[:cut], cfg)
        y1, s1 = R.denoise(x[cut:], cfg, s0)
        assert np.array_equal(bits(np.concatenate([y0, y1])), bits(y)), cut
        assert same_state(s1, st), cut
    # three pieces, and the state through its record
    y0, s0 = R.denoise(x[:13], cfg)
    y1, s1 = R.denoise(x[13:14], cfg, R.state_from(R.state_bytes(s0)))
    y2, s2 = R.denoise(x[14:], cfg, R.state_from(R.state_bytes(s1)))
    assert np.array_equal(bits(np.concatenate([y0, y1, y2])), bits(y)) and same_state(s2, st)
    assert len(R.state_bytes(st)) == R.STATE_BYTES == 2064


@pytest.mark.parametrize("cfg", [DEFAULT, PLAIN, CLAMPS, dict(DEFAULT, close_step=1000000), dict(DEFAULT, close_step=7)], ids=str)
@pytest.mark.parametrize("value", [-3.3, 0.5])
def test_a_constant_mel_converges_to_its_fixed_point(cfg, value):
    p = R.fields(cfg)
    want = min(((p["knee"] + p["bias"]) * p["slope"]) >> 8, p["depth"])
    need = -(-want // p["close_step"])
    x = np.full((need + 5, 5), value, F32)
    L = int(R.level(F32(value)))
    for T in range(1, need + 6):
        _, st = R.denoise(x[:T], p)
        assert (st["floor"] == L).all()
        assert (st["att"] == min(T * p["close_step"], want)).all()
        if T >= need:
            assert (st["att"] == want).all()


@pytest.mark.parametrize("cfg", [DEFAULT, CLAMPS], ids=["default", "clamps"])
def test_a_bin_well_over_the_floor_keeps_its_bits(cfg):
    p = R.fields(cfg)
    x = noisy(60, 11, 2)
    x[30, 5] = -0.0
    x[31:36, 2:9] = 1.25
    state, kept = None, 0
    for f in range(x.shape[0]):
        y, after = R.denoise(x[f:f + 1], p, state)
        if state is not None:
            snr = R.level(x[f]) - (state["floor"] + p["bias"])
            ok = snr >= p["knee"]
            ok = ok & np.concatenate([ok[:1], ok[:-1]]) & np.concatenate([ok[1:], ok[-1:]]) & (state["att"] <= p["open_step"])
            assert np.array_equal(bits(y[0])[ok], bits(x[f])[ok]), f
            assert (after["att"][ok] == 0).all()
            kept += int(ok.sum())
        state = after
    assert kept > 0      # (the property was exercised)


@pytest.mark.parametrize("cfg", [DEFAULT, PLAIN, CLAMPS], ids=["default", "plain", "clamps"])
@pytest.mark.parametrize("nm", [1, 2, 3, 9])
def test_the_scalar_restatement_agrees_and_the_edges_hold(cfg, nm):
    p = R.fields(cfg)
    x = noisy(48, nm, 3 + nm)
    y, st = R.denoise(x, p)
    ys, (N, A) = scalar(x, p)
    assert np.array_equal(bits(y), bits(ys))
    assert list(st["floor"]) == N and list(st["att"]) == A
    if nm == 1:      # (a + 2a + a + 2) >> 2 = a: the average of a lone bin is the bin
        y0, s0 = R.denoise(x, dict(p, smooth=0))
        assert np.array_equal(bits(y), bits(y0)) and same_state(st, s0)
    if nm == 2 and p["smooth"]:      # a2[0] = (3 a[0] + a[1] + 2) >> 2: each edge counts itself twice more
        one = np.array([[-4.0, -4.0], [-5.0, -4.0]], F32)
        _, s = R.denoise(one, dict(p, close_step=1 << 20, open_step=1 << 20, rise=0, floor_min=-(1 << 20)))
        a = [min(((p["knee"] + p["bias"] + d) * p["slope"]) >> 8, p["depth"]) for d in (1024, 0)]
        assert list(s["att"]) == [(3 * a[0] + a[1] + 2) >> 2, (a[0] + 3 * a[1] + 2) >> 2]


def test_nan_and_out_of_range_values():
    full = 1 << 20
    vals = np.array([np.nan, 2000.0, -2000.0, np.inf, -np.inf, 1024.0, -1024.0, 0.00048828125, 0.00146484375, -0.00048828125], F32)
    assert list(R.level(vals)) == [-full, full, -full, full, -full, full, -full, 0, 2, 0]      # ties to even
    weird = np.array([[0x7FC00123, 0xFFC00001, 0x7F800000, 0x80000000, 0x00000001]], np.uint32).view(F32)
    # a gate that never closes keeps every bin's bits, NaN payloads included
    y, st = R.denoise(np.repeat(weird, 3, 0), dict(DEFAULT, slope=0))
    assert np.array_equal(bits(y), bits(np.repeat(weird, 3, 0)))
    assert int(st["floor"][0]) == DEFAULT["floor_min"] and int(st["floor"][2]) == full      # (a NaN starts the floor at floor_min)
    # a NaN under an established floor is an empty bin: it is attenuated down to out_floor
    x = np.full((4, 3), -2.0, F32)
    x[2, 1] = np.nan
    y, _ = R.denoise(x, DEFAULT)
    assert bits(y[2])[1] == bits(np.array([DEFAULT["out_floor"]], F32))[0]
    assert not np.isnan(y).any()


def test_every_branch_is_taken():
    R.seen.clear()
    for cfg in (DEFAULT, PLAIN, CLAMPS):
        R.denoise(noisy(80, 9, 5), cfg)
    missing = [b for b in R.BRANCHES if R.seen[b] < 1]
    assert not missing, (missing, dict(R.seen))
