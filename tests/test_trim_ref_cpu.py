"""The trimming law (tests/trim_ref.py) against what it restates: the reference's centred float moving average followed by np.round, and
scipy.ndimage.binary_dilation with a structure of ones - over random flags for every smoothing width 1 .. 19 and every dilation width
1 .. 39.  The same checks must reject the two near misses: a tie rule of >= and the mirrored window for even dilation widths."""
import numpy as np
import pytest

from conan_amd import _lib
from tests import activity_ref as A
from tests import trim_ref as R

WIDTHS, DILATIONS = range(1, 20), range(1, 40)


def _flag_rows():
    rng = np.random.default_rng(5)
    rows = [np.zeros(1, np.int32), np.ones(1, np.int32), np.zeros(50, np.int32), np.ones(50, np.int32)]
    rows.append((np.arange(60) % 2).astype(np.int32))      # every even window inside it is exactly half active
    rows.append((np.arange(101) == 50).astype(np.int32))      # one frame alone: the dilation's window shows as it is
    for F in (2, 3, 7, 40, 41, 257):
        for density in (0.1, 0.5, 0.9):
            rows.append((rng.random(F) < density).astype(np.int32))
    return rows


def _moving_average_round(flags, w):
    """The float form: zero padding of (w - 1) // 2 in front and w // 2 behind, the mean of every window of w, np.round (ties to even)."""
    padded = np.concatenate((np.zeros((w - 1) // 2), np.asarray(flags, dtype=float), np.zeros(w // 2)))
    means = np.array([padded[i:i + w].sum() / w for i in range(len(flags))])
    return np.round(means).astype(bool)


def _smooth_tie_up(act, w):
    a = (np.asarray(act) != 0).astype(np.int64)
    return (2 * R._window_sums(a, (w - 1) // 2, w // 2) >= w).astype(np.int32)


def _dilate_mirrored(m1, max_silence):
    s = max_silence + 1
    return (R._window_sums((np.asarray(m1) != 0).astype(np.int64), s // 2, s - 1 - s // 2) > 0).astype(np.int32)


def test_smoothing_is_the_float_moving_average_rounded_to_even():
    rows = _flag_rows()
    tie_caught = set()
    for w in WIDTHS:
        for flags in rows:
            want = _moving_average_round(flags, w)
            assert np.array_equal(R.smooth(flags, w).astype(bool), want), (w, flags)
            if not np.array_equal(_smooth_tie_up(flags, w).astype(bool), want):
                tie_caught.add(w)
    # a window that is exactly half active exists for even w only: the flipped rule is caught at every one of them
    assert tie_caught == {w for w in WIDTHS if w % 2 == 0}


def test_dilation_is_scipys_binary_dilation():
    ndimage = pytest.importorskip("scipy.ndimage")
    rows = _flag_rows()
    mirrored_caught = set()
    for s in DILATIONS:
        for flags in rows:
            want = ndimage.binary_dilation(flags.astype(bool), np.ones(s))
            assert np.array_equal(R.dilate(flags, s - 1).astype(bool), want), (s, flags)
            if not np.array_equal(_dilate_mirrored(flags, s - 1).astype(bool), want):
                mirrored_caught.add(s)
    # scipy's origin is off-centre for even widths: the mirrored window is caught at every one of them, and is the same for odd ones
    assert mirrored_caught == {s for s in DILATIONS if s % 2 == 0}


def test_plan_offsets_and_the_copy():
    hop = 4
    wav = np.arange(1, 24, dtype=np.float32)      # 23 samples: 6 frames, the last owns 3
    act = np.array([0, 1, 1, 0, 0, 1], np.int32)
    out, m2, off, out_len = R.trim(wav, act, hop, w=1, max_silence=0)
    assert list(R.counts(23, hop)) == [4, 4, 4, 4, 4, 3]
    assert list(m2) == [0, 1, 1, 0, 0, 1] and list(off) == [-1, 0, 4, -1, -1, 8] and out_len == 11
    assert list(out) == [5, 6, 7, 8, 9, 10, 11, 12, 21, 22, 23] + [0] * 12
    # s = 2 reaches one frame ahead and none back (scipy's origin); the pause of two frames is kept whole from max_silence = 2 on
    assert list(R.plan(act, 23, hop, 1, 1)[0]) == [1, 1, 1, 0, 1, 1]
    assert list(R.plan(act, 23, hop, 1, 2)[0]) == [1, 1, 1, 1, 1, 1]
    # len % hop == 0: the last frame owns nothing, kept or not
    out, m2, off, out_len = R.trim(wav[:20], np.ones(6, np.int32), hop, w=1, max_silence=0)
    assert list(off) == [0, 4, 8, 12, 16, 20] and out_len == 20 and np.array_equal(out, wav[:20])
    # payloads survive the copy
    odd = np.array([0x7fc00001, 0xffc12345, 0x80000000, 0x00000001, 0x7f800000], np.uint32).view(np.float32)
    out = R.trim(odd, np.ones(2, np.int32), 4, 1, 0)[0]
    assert np.array_equal(out.view(np.uint32), odd.view(np.uint32))


def test_burst_signal_counts():
    """activity_ref.burst_signal() with the default detector and the default widths: 251 frames, 130 active, 175 kept."""
    x = A.burst_signal()
    act, out, m2, off, out_len = R.run(x, _lib.activity_cfg())
    assert act.shape[0] == m2.shape[0] == R.n_frames(x.shape[0], 320) == 251
    assert int(act.sum()) == 130
    assert int(m2.sum()) == 175
    kept = np.flatnonzero(m2)
    assert 0 < kept[0] and kept[-1] < 250      # the kept frames lie strictly inside the signal
    assert out_len == 175 * 320 and not out[out_len:].any()
    # the dilation only adds frames, and every stretch it adds is a pause of at most 18 frames or a margin of at most 9
    m1 = R.smooth(act, R.SMOOTH)
    assert not (m1 & ~m2).any()
    assert _lib.trim_cfg().smooth_frames == R.SMOOTH and _lib.trim_cfg().max_silence_frames == R.MAX_SILENCE
