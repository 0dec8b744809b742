"""The source-activity law's reference against itself, without a GPU (tests/activity_ref.py; include/conan_hip.h, conan_activity_cfg):
the streamed form equals the whole-signal form however the frames are cut, the fixed-order power sum is as accurate as its depth
promises, an open gate is the identity, and the test signals take every branch of the law."""
import math

import numpy as np

from conan_amd import _lib
from tests import activity_ref as A

HOP, N = 320, 1024


def _cfg2():
    return _lib.activity_cfg(open_db=-70.0, close_db=-75.0, floor_db=-38.0)


def test_any_cut_into_pieces_equals_the_whole_signal():
    x = A.burst_signal()
    rng = np.random.default_rng(7)
    for cfg in (_lib.activity_cfg(), _cfg2(), _lib.activity_cfg(hold_frames=0, up_step=A.FULL // 3, down_step=A.FULL // 7 + 1, closed_level=1 << 16)):
        whole = A.run(x, cfg, N, HOP)
        F = A.n_frames(len(x), HOP)
        assert len(whole["act"]) == F == 251
        cuts = [0] + sorted(rng.choice(np.arange(1, F), size=36, replace=False).tolist()) + [F]      # 37 pieces
        state, acts, lvls = None, [], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            r = A.run(x, cfg, N, HOP, state=state, f0=a, count=b - a)
            state = r["state"]
            acts.append(r["act"]); lvls.append(r["level"])
        assert np.array_equal(np.concatenate(acts), whole["act"]) and np.array_equal(np.concatenate(lvls), whole["level"])
        assert state == whole["state"] and state["frames"] == F and state["active_frames"] == int(whole["act"].sum())


def test_the_fixed_order_power_sum_is_within_its_depth_of_the_exact_sum():
    """Each of the 64 partial sums adds N / 64 terms and the fold adds 6 levels: a relative error of at most (N / 64 + 6) * 2^-53 for a
    sum of non-negative terms.  Measured here at N = 1024: 2.3e-16."""
    x = A.burst_signal()
    worst = 0.0
    for n_fft in (64, 256, 1024, 2048):
        P = A.powers(x, n_fft, HOP)
        fr = A.frames_of(x, 0, len(P), n_fft, HOP)
        bound = (n_fft // 64 + 6) * 2.0 ** -53
        for f in range(0, len(P), 7):
            exact = math.fsum(float(v) * float(v) for v in fr[f]) / n_fft
            if exact > 0.0:
                err = abs(float(P[f]) - exact) / exact
                assert err <= bound, (n_fft, f, err, bound)
                worst = max(worst, err) if n_fft == 1024 else worst
            else:
                assert P[f] == 0.0
    print("largest relative error at N = 1024:", worst)


def test_an_open_gate_is_the_identity_and_the_gain_is_the_law():
    assert np.array_equal(A.gain(A.FULL, A.FULL, HOP), np.ones(HOP, dtype=np.float32))
    for hop in (1, 7, 256, 320):
        assert (A.gain(A.FULL, A.FULL, hop) == np.float32(1.0)).all()
        g = A.gain(0, A.FULL, hop)
        assert g[-1] == np.float32(1.0) and (np.diff(g) >= 0).all() and g[0] == np.float32(np.float64(1 << 20) / np.float64(hop << 20))
    rng = np.random.default_rng(1)
    x = rng.standard_normal(5 * HOP + 17).astype(np.float32)
    lv = np.full(6, A.FULL)
    assert np.array_equal(A.gate(x, lv, A.FULL, HOP).view(np.uint32), x.view(np.uint32))      # the audio keeps its bits
    lv = np.array([0, A.FULL // 2, A.FULL, A.FULL, 12345, 0])
    y = A.gate(x, lv, 777, HOP)
    want = np.concatenate([x[f * HOP:(f + 1) * HOP] * A.gain(777 if f == 0 else lv[f - 1], lv[f], HOP)[:len(x[f * HOP:(f + 1) * HOP])] for f in range(6)])
    assert np.array_equal(y.view(np.uint32), want.astype(np.float32).view(np.uint32))


def test_the_signals_take_every_branch():
    r = A.run(A.burst_signal(), _lib.activity_cfg(), N, HOP)
    print("default cfg:", r["counts"])
    c = r["counts"]
    assert c["openings"] >= 1 and c["closings"] >= 1 and c["hangover"] >= 1 and c["clamps"] >= 1
    assert 0 < r["act"].sum() < len(r["act"])
    assert r["level"].min() == 0 and r["level"].max() == A.FULL and len(set(r["level"].tolist())) > 2      # the release ramp is visible
    r2 = A.run(A.burst_signal(noise=1e-2), _cfg2(), N, HOP)
    print("ratio-governed cfg:", r2["counts"])
    assert r2["counts"]["ratio_openings"] >= 1 and r2["counts"]["openings"] >= r2["counts"]["ratio_openings"]
    # digital silence: the power is exactly zero there and the floor sits at its minimum
    P = r["power"]
    assert (P[185:190] == 0.0).all()


def test_the_helper_reads_decibels_once_into_f32():
    c = _lib.activity_cfg()
    p = A.params(c)
    assert p["open_abs"] == np.float64(np.float32(10.0 ** -5.0)) and p["close_abs"] == np.float64(np.float32(10.0 ** -5.5))
    assert p["open_ratio"] == np.float64(np.float32(10.0 ** 0.9)) and p["close_ratio"] == np.float64(np.float32(10.0 ** 0.6))
    assert p["floor_min"] == np.float64(np.float32(1e-7)) and A.seed_state(c)["floor"] == np.float64(np.float32(1e-6))
    assert (p["hold_frames"], p["up_step"], p["down_step"], p["closed_level"]) == (10, 1 << 20, 209716, 0)      # attack in one frame, release in five
    assert 5 * p["down_step"] >= A.FULL > 4 * p["down_step"]
