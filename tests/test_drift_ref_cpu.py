"""The drift resampler's reference (tests/drift_ref.py) and the library's host-only helpers: the table against a float64 evaluation
of the kernel, the exact length against Python integers, the schedule's cut independence, the identity case, and the distance of
the interpolated table from the exact-position kernel."""
import numpy as np
import pytest

from conan_amd import _lib
from tests import drift_ref as R

KAISER16 = dict(lowpass_filter_width=16, resampling_method="sinc_interp_kaiser")
TABLES = [
    ("hann-16k-16k", 16000, 16000, {}, {}),
    ("hann-8k-16k", 8000, 16000, {}, {}),
    ("kaiser16-16k-16k", 16000, 16000, KAISER16, dict(lpw=16, window="kaiser")),
    ("kaiser16-8k-16k", 8000, 16000, KAISER16, dict(lpw=16, window="kaiser")),
    ("kaiser16-48k-16k", 48000, 16000, KAISER16, dict(lpw=16, window="kaiser")),
]


@pytest.mark.parametrize("name,fin,fout,kw,rk", TABLES, ids=[t[0] for t in TABLES])
def test_table_against_float64(name, fin, fout, kw, rk):
    tab = _lib.resample_drift_table(fin, fout, **kw)
    W, _ = R.width(fin, fout, rk.get("lpw", 6), 0.99)
    assert tab.shape == (R.PHASES + 1, 2 * W) and tab.dtype == np.float32
    want = R.table64(fin, fout, **rk)
    w32 = want.astype(np.float32)
    err = np.abs(tab.astype(np.float64) - want)
    ulp = np.spacing(np.abs(w32)).astype(np.float64)
    print("%s: W %d, %d of %d entries differ from the rounded float64 value, worst %.3g ulp" %
          (name, W, int((tab != w32).sum()), tab.size, float((err / ulp).max())))
    assert (err <= ulp).all()


def test_table_rows_shift_by_one_input():
    tab = _lib.resample_drift_table(16000, 16000)
    # phase 1024 of input n is phase 0 of input n + 1: T[1024][k] = T[0][k - 1]
    assert np.array_equal(tab[R.PHASES, 1:], tab[0, :-1])
    assert tab[R.PHASES, 0] == 0.0 or abs(tab[R.PHASES, 0]) < 1e-6


def test_table_refusals():
    with pytest.raises(_lib.ConanError):      # 2W = 2 * ceil(128 * 48000 / (16000 * 0.99)) > 512
        _lib.resample_drift_table(48000, 16000, lowpass_filter_width=128)
    cfg = _lib.resample_cfg(16000, 16000)
    small = np.empty(8, dtype=np.float32)
    assert _lib.lib().conan_resample_drift_table(_lib.C.byref(cfg), None, small.ctypes.data, 8) < 0


LENGTHS = [(fin, fout, side, ppb, N)
           for fin, fout in ((16000, 16000), (8000, 16000), (48000, 16000), (16000, 8000), (16000, 48000), (44100, 16000))
           for side in (R.SOURCE, R.SINK)
           for ppb in (0, 300000, -150000, 2000000, -2000000)
           for N in (1, 699, 700, 1 << 20, 1 << 40)]


def test_length_against_integers():
    lib, C = _lib.lib(), _lib.C
    for fin, fout, side, ppb, N in LENGTHS:
        cfg = _lib.resample_cfg(fin, fout)
        at, pb = np.zeros(1, dtype=np.int64), np.array([ppb], dtype=np.int32)
        got = lib.conan_resample_drift_length(C.byref(cfg), side, N, at.ctypes.data, pb.ctypes.data, 1)
        want = R.length(fin, fout, side, [(0, ppb)], N)
        assert got == want, (fin, fout, side, ppb, N, got, want)
        # the definition itself: the last output lies inside the signal, the next one does not
        st = R.step(fin, fout, side, ppb)
        assert ((want - 1) * st) >> 32 < N <= (want * st) >> 32


def test_length_of_schedules():
    lib, C = _lib.lib(), _lib.C
    cfg = _lib.resample_cfg(8000, 16000)
    sched = [(0, 300000), (257, -2000000), (1000, 2000000), (1 << 35, 0)]
    at = np.array([a for a, _ in sched], dtype=np.int64)
    pb = np.array([p for _, p in sched], dtype=np.int32)
    for side in (R.SOURCE, R.SINK):
        for N in (1, 100, 128, 129, 499, 500, 501, 700, 1 << 34, (1 << 34) + 12345, 1 << 40):
            for n_seg in (1, 2, 3, 4):
                got = lib.conan_resample_drift_length(C.byref(cfg), side, N, at.ctypes.data, pb.ctypes.data, n_seg)
                assert got == R.length(8000, 16000, side, sched[:n_seg], N), (side, N, n_seg)
    # the closed form is the recurrence
    n = R.length(8000, 16000, R.SOURCE, sched[:3], 700)
    pos = R.positions(8000, 16000, R.SOURCE, sched[:3], n + 1)
    assert pos[n - 1] >> 32 < 700 <= pos[n] >> 32
    seg = R.segments(8000, 16000, R.SOURCE, sched[:3])
    assert [pos[a] for a, _, _ in seg] == [p for _, p, _ in seg]
    # refusals: at[0] != 0, a descending schedule, a ppb out of range, a side that is none, too many segments
    bad_at = np.array([1, 5], dtype=np.int64)
    assert lib.conan_resample_drift_length(C.byref(cfg), 0, 700, bad_at.ctypes.data, pb.ctypes.data, 2) == -1
    desc = np.array([0, 5, 5], dtype=np.int64)
    assert lib.conan_resample_drift_length(C.byref(cfg), 0, 700, desc.ctypes.data, pb.ctypes.data, 3) == -1
    big = np.array([2000001], dtype=np.int32)
    assert lib.conan_resample_drift_length(C.byref(cfg), 0, 700, at.ctypes.data, big.ctypes.data, 1) == -1
    assert lib.conan_resample_drift_length(C.byref(cfg), 2, 700, at.ctypes.data, pb.ctypes.data, 1) == -1
    assert lib.conan_resample_drift_length(C.byref(cfg), 0, 700, at.ctypes.data, pb.ctypes.data, _lib.DRIFT_MAX_SEGMENTS + 1) == -1


def test_schedule_split_anywhere_equals_unsplit():
    """A segment cut in two with the same ppb changes no position, no length and no ready count."""
    sched = [(0, 300000), (400, -150000)]
    whole = R.positions(48000, 16000, R.SOURCE, sched, 900)
    for cut in (1, 2, 255, 256, 257, 399, 401, 899):
        split = sorted(set(sched + [(cut, 300000 if cut < 400 else -150000)]))
        assert R.positions(48000, 16000, R.SOURCE, split, 900) == whole, cut
        for N in (10, 700, 2000, 2700):
            assert R.length(48000, 16000, R.SOURCE, split, N) == R.length(48000, 16000, R.SOURCE, sched, N)
            assert R.ready(48000, 16000, R.SOURCE, split, N, 19) == R.ready(48000, 16000, R.SOURCE, sched, N, 19)
    # and the sum over a stream cut into calls is the whole signal's: outputs computed from a window of the input equal the whole's
    x = np.random.default_rng(3).standard_normal(700).astype(np.float32)
    tab = _lib.resample_drift_table(48000, 16000)
    W = tab.shape[1] // 2
    n = R.length(48000, 16000, R.SOURCE, sched, 700)
    pos = R.positions(48000, 16000, R.SOURCE, sched, n)
    y = R.resample(x, tab, pos)
    lo_out, hi_out = 100, 180
    lo_in = (pos[lo_out] >> 32) - W + 1
    hi_in = (pos[hi_out - 1] >> 32) + W + 1
    part = R.resample(x[lo_in:hi_in], tab, pos[lo_out:hi_out], lo=lo_in, received=700)
    assert np.array_equal(part.view(np.uint32), y[lo_out:hi_out].view(np.uint32))


def test_unit_impulse_is_the_identity():
    tab = _lib.resample_drift_table(16000, 16000, rolloff=1.0)
    W = tab.shape[1] // 2
    assert W == 6 and np.count_nonzero(tab[0]) == 1 and tab[0, W - 1] == 1.0
    x = np.random.default_rng(4).standard_normal((2, 700)).astype(np.float32)
    x[0, :3] = (0.0, 1e-30, -1e-40)
    for side in (R.SOURCE, R.SINK):
        assert R.step(16000, 16000, side, 0) == 1 << 32
        y = R.whole(x, tab, 16000, 16000, side, [(0, 0)])
        assert y.shape == x.shape and np.array_equal(y.view(np.uint32), x.view(np.uint32))


# What drift_ref measures in the case below: the largest distance, over the interior outputs, of the law's f32 result from the
# float64 exact-position evaluation.  The test asserts 4 x this value; the margin covers other phases and frequencies.
MEASURED_TABLE_ERROR = 9.3e-8


def test_table_form_against_exact_positions():
    """A 1 kHz sine of amplitude 0.5 at +300 ppm, hann 16k -> 16k: the law (f32 table of 1024 phases, linear interpolation, f32 FMA
    chain) against the same kernel evaluated in float64 at the exact positions, without a table; interior samples only.  Printed
    beside it: what the linear interpolation alone costs (the table law in float64), and the hann filter's own distance from the
    ideal sine, three orders above both."""
    fin = fout = 16000
    N = 4000
    x = (0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(N) / fin)).astype(np.float32)
    x64 = x.astype(np.float64)
    tab = _lib.resample_drift_table(fin, fout)
    W = tab.shape[1] // 2
    sched = [(0, R.ppb_of(300.0))]
    n = R.length(fin, fout, R.SOURCE, sched, N)
    pos = R.positions(fin, fout, R.SOURCE, sched, n)
    interior = slice(2 * W, n - 2 * W)
    exact = R.exact64(x64, pos, fin, fout)[interior]
    got = R.resample(x, tab, pos).astype(np.float64)[interior]
    err = np.abs(got - exact).max()
    t64 = R.table64(fin, fout)
    nn = np.array([p >> 32 for p in pos])
    f = np.array([p & 0xffffffff for p in pos])
    ph, mu = f >> 22, (f & 0x3fffff) * 2.0 ** -22
    lin = np.zeros(n)
    for k in range(2 * W):
        i = nn - W + 1 + k
        ok = (i >= 0) & (i < N)
        lin += (t64[ph, k] + mu * (t64[ph + 1, k] - t64[ph, k])) * np.where(ok, x64[np.clip(i, 0, N - 1)], 0.0)
    ideal = 0.5 * np.sin(2 * np.pi * 1000.0 * (np.array(pos, dtype=np.float64) * 2.0 ** -32) / fin)[interior]
    print("table law vs exact kernel: f32 %.3g (float64 interpolation alone %.3g); the hann filter vs the ideal sine %.3g" %
          (err, np.abs(lin[interior] - exact).max(), np.abs(exact - ideal).max()))
    assert err <= 4.0 * MEASURED_TABLE_ERROR
