"""Silence trimming restated (include/conan_hip.h, conan_trim_cfg): the offline half of source activity, with Python / numpy integers
only, so the GPU and this file agree bit for bit.

n_frames():  F = 1 + len // hop, the detector's frame count.
smooth():    rule 2: S[f] = sum of act[j], j in [f - (w - 1) // 2, f + w // 2], zeros outside; m1[f] = 2 * S[f] > w.
dilate():    rule 3: s = max_silence + 1; m2[f] = OR of m1[j], j in [f - (s - 1 - s // 2), f + s // 2], clipped.
counts():    cnt[f]: frame f owns samples f * hop .. min((f + 1) * hop, len) - 1.
plan():      rules 2 - 4 on a row's flags -> (m2 int32 [F], off int64 [F]: off[f] or -1 for a dropped frame, out_len).
trim():      plan + the bit copy of the kept frames' samples -> (out [len] with zeros from out_len on, m2, off, out_len).
run():       the detector's flags (activity_ref.run, from the cfg's seed) and trim() on them."""
import numpy as np

from tests import activity_ref

SMOOTH, MAX_SILENCE = 12, 18


def n_frames(length, hop):
    return 1 + length // hop


def _window_sums(a, left, right):
    """sum of a[j] over j in [f - left, f + right] clipped to 0 .. F-1, for every f: differences of one prefix sum (int64)."""
    F = a.shape[0]
    pre = np.concatenate(([0], np.cumsum(a, dtype=np.int64)))
    f = np.arange(F, dtype=np.int64)
    lo, hi = np.maximum(f - left, 0), np.minimum(f + right, F - 1)
    return pre[hi + 1] - pre[lo]


def smooth(act, w):
    a = (np.asarray(act) != 0).astype(np.int64)
    return (2 * _window_sums(a, (w - 1) // 2, w // 2) > w).astype(np.int32)


def dilate(m1, max_silence):
    s = max_silence + 1
    m = (np.asarray(m1) != 0).astype(np.int64)
    return (_window_sums(m, s - 1 - s // 2, s // 2) > 0).astype(np.int32)


def counts(length, hop):
    f = np.arange(n_frames(length, hop), dtype=np.int64)
    return np.minimum((f + 1) * hop, length) - f * hop


def plan(act, length, hop, w=SMOOTH, max_silence=MAX_SILENCE):
    F = n_frames(length, hop)
    act = np.asarray(act)[:F]
    assert act.shape[0] == F, "one flag per frame"
    m2 = dilate(smooth(act, w), max_silence)
    kept = counts(length, hop) * m2
    ends = np.cumsum(kept, dtype=np.int64)
    off = np.where(m2 != 0, ends - kept, np.int64(-1)).astype(np.int64)
    return m2, off, int(ends[-1])


def trim(wav, act, hop, w=SMOOTH, max_silence=MAX_SILENCE):
    """wav: f32 [len] (copied through a uint32 view: NaN payloads and -0.0 survive)."""
    bits = np.ascontiguousarray(np.asarray(wav, dtype=np.float32)).view(np.uint32)
    length = bits.shape[0]
    m2, off, out_len = plan(act, length, hop, w, max_silence)
    out = np.zeros(length, dtype=np.uint32)
    cnt = counts(length, hop)
    for f in np.flatnonzero(m2):
        out[off[f]:off[f] + cnt[f]] = bits[f * hop:f * hop + cnt[f]]
    return out.view(np.float32), m2, off, out_len


def run(wav, cfg, N=1024, hop=320, w=SMOOTH, max_silence=MAX_SILENCE):
    """The detector form: activity_ref's flags for the row from the cfg's seed, then trim()."""
    act = activity_ref.run(wav, cfg, N=N, hop=hop)["act"]
    return (act,) + trim(wav, act, hop, w, max_silence)
