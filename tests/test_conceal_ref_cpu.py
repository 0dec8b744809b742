"""tests/conceal_ref.py, the numpy restatement of the loss concealment's law (include/conan_hip.h, conan_conceal_cfg), held to the
facts the law pins: the lag of an integer-valued periodic signal is its period and a held run continues it exactly, an all-zero
history gives lag_min and zeros, a long run ends in zeros, fade = 0 goes straight back to idle, received samples outside a fade are
never written, and cutting a signal into rows on packet boundaries changes nothing."""
import numpy as np
import pytest

from tests import conceal_ref as R
from tests import sample_format_ref as SF

TINY = dict(packet=16, lag_min=4, lag_max=24, window=32, hold=8, fall=16, fade=8)


def periodic(n, period, seed=0):
    """An integer-valued (k / 32768, exact in every format's decoder domain) periodic signal whose fundamental period is `period`."""
    rng = np.random.default_rng(seed)
    while True:
        cell = rng.integers(-12000, 12000, size=period)
        if all(np.any(cell != np.roll(cell, d)) for d in range(1, period)):      # no shorter period
            break
    return (np.tile(cell, n // period + 1)[:n].astype(np.float64) / 32768.0).astype(np.float32)


def flags(n, packet, lost_packets):
    f = np.zeros((n + packet - 1) // packet, dtype=np.int32)
    f[list(lost_packets)] = 1
    return f


def test_defaults():
    assert R.defaults(48000) == dict(packet=960, lag_min=120, lag_max=720, window=960, hold=480, fall=2400, fade=240)
    assert R.defaults(8000) == dict(packet=160, lag_min=20, lag_max=120, window=160, hold=80, fall=400, fade=40)
    d = R.defaults(48000)
    assert d["lag_max"] <= R.MAX_LAG and d["window"] <= R.MAX_WINDOW and d["fade"] <= 1024


def test_level_and_gain():
    assert [R.level(k, 2, 4) for k in range(8)] == [R.FULL, R.FULL, R.FULL, (3 << 20) // 4, (2 << 20) // 4, (1 << 20) // 4, 0, 0]
    assert R.level(0, 0, 3) == R.FULL and R.level(1, 0, 3) == (2 << 20) // 3      # floor
    assert R.gain(R.FULL) == np.float32(1) and R.gain(0) == np.float32(0) and R.gain(1) == np.float32(2.0 ** -20)


@pytest.mark.parametrize("period", [4, 7, 13, 24])
def test_the_search_returns_the_period_and_a_held_run_continues_the_signal(period):
    cfg = dict(TINY, hold=16)
    n = 128
    x = periodic(n, period, period)
    lost = flags(n, cfg["packet"], [4])      # samples 64 .. 79: window + lag_max = 56 received samples in front
    c = R.Concealer("f32", **cfg)
    y, written = c.apply(x, lost)
    assert c.p == period
    assert np.array_equal(y[64:80].view(np.uint32), x[64:80].view(np.uint32))      # k < hold: the original exactly
    assert written[64:80].all() and not written[:64].any()
    assert np.array_equal(y[:64].view(np.uint32), x[:64].view(np.uint32))


def test_an_all_zero_history_gives_lag_min_and_zeros():
    c = R.Concealer("f32", **TINY)
    x = np.full(64, 0.25, dtype=np.float32)
    y, _ = c.apply(x, flags(64, 16, [0, 1]))      # a loss at position 0
    assert c.p == TINY["lag_min"] and not y[:32].any()
    for fmt in SF.FORMATS:
        c = R.Concealer(fmt, **TINY)
        y, _ = c.apply(SF.encode(x, fmt), flags(64, 16, [0]))
        # (every sample is the format's code of zero; A-law has no zero: its code of 0 decodes to 8 / 32768)
        assert c.p == TINY["lag_min"] and np.array_equal(y[:16], np.repeat(SF.encode(np.zeros(1, np.float32), fmt), 16))


def test_a_run_beyond_hold_and_fall_ends_in_zeros():
    n = 160
    x = periodic(n, 9)
    y = R.conceal(x, flags(n, 16, [4, 5, 6, 7, 8, 9]), **TINY)      # a run of 96 > hold + fall = 24
    assert y[64:64 + 8].any() and not y[64 + 24:160].any()
    k = np.arange(8, 24)
    assert np.all(np.abs(y[64 + 8:64 + 24]) <= np.abs(np.tile(x[64 - 9:64], 11)[k]))      # the fall never raises a sample


def test_fade_zero_switches_straight_to_idle():
    n = 128
    x = periodic(n, 11)
    c = R.Concealer("f32", **dict(TINY, fade=0))
    y, written = c.apply(x, flags(n, 16, [4]))
    assert c.mode == 0 and not written[80:].any() and np.array_equal(y[80:], x[80:])
    c = R.Concealer("f32", **TINY)
    y, written = c.apply(x, flags(n, 16, [4]))
    assert written[80:88].all() and not written[88:].any() and c.mode == 0 and c.j == TINY["fade"]


def test_a_loss_inside_a_fade_is_a_new_run():
    cfg = dict(TINY, packet=4)
    n = 128
    x = periodic(n, 10)
    lost = flags(n, 4, [16, 18])      # 64 .. 67 lost, 68 .. 71 fade (4 of 8), 72 .. 75 lost again
    c = R.Concealer("f32", **cfg)
    y, written = c.apply(x, lost)
    assert written[64:76].all() and written[76:84].all() and not written[84:].any()
    one = R.Concealer("f32", **cfg)
    one.apply(x[:72], lost)
    assert one.mode == 2 and one.j == 4


@pytest.mark.parametrize("fmt", ["f32", "s16", "ulaw", "alaw"])
def test_chunked_application_equals_whole_signal_application(fmt):
    n = 400
    rng = np.random.default_rng(5)
    x = SF.encode((periodic(n, 17, 3) + rng.integers(-300, 300, size=n).astype(np.float32) / 32768).astype(np.float32), fmt)
    lost = flags(n, 16, [0, 5, 6, 7, 8, 9, 12, 14, 20, 24])
    whole = R.conceal(x, lost, fmt, **TINY)
    for cuts in ([128, 256], [16, 32, 48, 96, 112, 208, 384], [80, 144, 224]):      # through runs, through fades, a short last row
        assert np.array_equal(R.conceal_chunked(x, lost, cuts, fmt, **TINY), whole), cuts
    assert whole.dtype == x.dtype and not np.array_equal(whole, x)
