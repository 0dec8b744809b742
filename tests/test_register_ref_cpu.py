"""The register-matching law (tests/register_ref.py) against itself, without a GPU: its two restatements agree bit for bit, the prior
seed gives the closed form (target - v_s) * n / (50 + n), the clamp holds, uncounted frames pass, a cut run continues from its state."""
import numpy as np
import pytest

from tests import register_ref as G


def contour(T, seed, unvoiced=0.3, odd=True):
    """A random contour [T]: voiced values in the tracker's range, unvoiced frames (v = 0, uv = 1) and - odd - a few frames no
    tracker writes: NaN, infinities, |v| > 64, a voiced flag that is not 0."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(5.0, 10.0, T).astype(np.float32)
    uv = (rng.random(T) < unvoiced).astype(np.float32)
    v[uv > 0] = 0.0
    if odd and T >= 8:
        k = rng.choice(T, size=min(6, T // 2), replace=False)
        v[k[0]] = np.nan; uv[k[0]] = 0
        v[k[1]] = np.inf; uv[k[1]] = 0
        v[k[2]] = 64.5; uv[k[2]] = 0
        v[k[3]] = -100.0; uv[k[3]] = 0
        uv[k[4]] = 0.5
        if len(k) > 5:
            v[k[5]] = 64.0; uv[k[5]] = 0      # the edge of the counted range: counted
    return v, uv


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("T", [0, 1, 3, 63, 64, 65, 255, 256, 257, 1000])
def test_the_two_restatements_agree_bit_for_bit(T):
    v, uv = contour(T, 100 + T)
    for kw in (dict(target=8.0), dict(target=6.5, seed=G.prior_seed(6.5)), dict(target=11.0, max_shift=0.25, seed=(7, 7 * G.quantise(5.5)))):
        a, sa = G.match(v, uv, **kw)
        for tile in (256, 64, 7):
            b, sb = G.match_blocked(v, uv, tile=tile, **kw)
            assert same(a, b) and sa == sb, (T, kw, tile)


def test_quantisation_is_exact_in_the_trackers_range():
    rng = np.random.default_rng(1)
    v = rng.uniform(3.96, 13.97, 4000).astype(np.float32)
    for x in v:
        q = G.quantise(x)
        assert np.float64(q) / np.float64(G.UNIT) == np.float64(x)
        assert abs(q) <= 2 ** 28


def test_steady_source_with_the_prior_seed_follows_the_closed_form():
    target, vs, N = np.float32(7.75), np.float32(6.3125), 400
    v = np.full(N, vs, dtype=np.float32)
    out, (n, S) = G.match(v, np.zeros(N, dtype=np.float32), target, max_shift=4.0, seed=G.prior_seed(target))
    assert (n, S) == (50 + N, 50 * G.quantise(target) + N * G.quantise(vs))
    k = np.arange(1, N + 1, dtype=np.float64)
    want = np.float64(vs) + (np.float64(target) - np.float64(vs)) * k / (50.0 + k)
    step = np.spacing(np.abs(out))      # one f32 step of v'
    assert (np.abs(out.astype(np.float64) - want) <= step).all()
    assert out[0] > vs and (np.diff(out) >= 0).all() and out[-1] < target      # the shift starts near 0 and converges towards the target


def test_the_clamp_holds():
    v, uv = contour(300, 5, odd=False)
    for lim in (0.0, 0.125, 1.0):
        out, _ = G.match(v, uv, target=12.0, max_shift=lim)
        voiced = uv == 0
        d = out[voiced].astype(np.float64) - v[voiced].astype(np.float64)
        assert (np.abs(d) <= lim + np.spacing(out[voiced]).astype(np.float64)).all()
        if lim == 0.0:
            assert same(out, v)
        else:
            assert np.abs(d - lim).min() <= 1e-6      # ... and the clamp is reached: the target is octaves away


def test_uncounted_frames_pass_unchanged_and_leave_the_state_alone():
    v = np.array([0.0, np.nan, np.inf, -np.inf, 64.5, -65.0, 7.0, 7.0], dtype=np.float32)
    uv = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.5], dtype=np.float32)
    seed = (3, 3 * G.quantise(6.0))
    for fn in (G.match, G.match_blocked):
        out, state = fn(v, uv, target=9.0, seed=seed)
        assert same(out, v) and state == seed
    # and between counted frames they change nothing: the counted frames' results are those of the contour without them
    v2 = np.array([7.0, np.nan, 7.5, 0.0, 8.0], dtype=np.float32)
    u2 = np.array([0.0, 0.0, 0.0, 1.0, 0.0], dtype=np.float32)
    a, sa = G.match(v2, u2, target=9.0, seed=seed)
    b, sb = G.match(v2[[0, 2, 4]], u2[[0, 2, 4]], target=9.0, seed=seed)
    assert same(a[[0, 2, 4]], b) and sa == sb and same(a[[1, 3]], v2[[1, 3]])


@pytest.mark.parametrize("cut", [0, 1, 17, 128, 299, 300])
def test_a_cut_run_continued_from_its_state_equals_the_uncut_run(cut):
    v, uv = contour(300, 9)
    kw = dict(target=8.25, max_shift=1.5)
    whole, state = G.match(v, uv, seed=G.prior_seed(8.25), **kw)
    a, mid = G.match(v[:cut], uv[:cut], seed=G.prior_seed(8.25), **kw)
    b, end = G.match_blocked(v[cut:], uv[cut:], seed=mid, **kw)
    assert same(np.concatenate([a, b]), whole) and end == state
