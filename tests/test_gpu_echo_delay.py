"""The echo-delay estimator on the GPU (conan_streams_set_echo_delay, conan_streams_echo_delay, conan_streams_echo_delay_state,
conan_echo_delay; include/conan_hip.h, conan_echo_delay_cfg), bit for bit against tests/echo_delay_ref.py: the whole-signal form over
the lag counts, formats and thresholds; the streaming form in every cut and through the wav-in step; the rows it reads keep their
bytes; the state records byte for byte; a live change of n_lags, the hand-over and the restart; a stream-set that never enables the
feature keeps its memory and its launches; and the engine with the follow rule end to end.  Nothing here has a tolerance: the law is
integer arithmetic.

The shapes are the smallest that reach every path: rows of one sample, one short of a frame, one frame, one tile and a sample, and two
tiles and a rest (so a row crosses eight frame ends); one wave of lags, a lag count that leaves lanes idle, and the full range."""
import functools

import numpy as np
import pytest
import torch

from conan_amd import _lib
from conan_amd.engine import StreamingVoiceConversionEngine
from tests import echo_delay_cases as EC
from tests import echo_delay_ref as R
from tests import echo_ref as CR
from tests import sample_format_ref as SF
from tests.test_gpu_echo import _pack, _unpack
from tests.test_gpu_f0 import _launches, _ref
from tests.test_gpu_pitch import full  # noqa: F401  (module fixture: the small synthetic full model)

pytestmark = pytest.mark.gpu

MAX_SLOTS = 4
FMTS = ("f32", "s16", "ulaw", "alaw")
ROW_BYTES = 64      # one table row of the kernel (streams.h: four tables of max_slots rows)
LENGTHS = (1, 1023, 1024, 4097, 9000)
BASE = dict(n_lags=320, thr=16, leak=3, ratio=4, min_peak=8, hold=2, tol=2)


def _codes(v, fmt):
    """16-bit integer values -> the codes of fmt (exact in f32 and s16; G.711 rounds them to its own grid)."""
    return SF.encode((np.asarray(v, dtype=np.float64) / 32768.0).astype(np.float32), fmt)


@functools.lru_cache(maxsize=None)
def _rows(fmt, n_lags, thr):
    """Five (mic, far) rows of LENGTHS, as 16-bit values before the format:
    0: one sample, mic = thr, far = -thr;
    1: small values around the threshold, with +-thr, +-(thr - 1) and -32768 sprinkled in, the mic an echo 20 samples late;
    2: an all-zero far row;
    3: louder noise, the mic an echo 37 samples late (f32: with NaN and +-Inf in both rows);
    4: a far impulse train of period 16, which divides every lag count, and a mic train 5 samples late that starts once every lag has
       its far sample: A is EQUAL at lags 5, 21, 37, ... and the lowest must win."""
    rng = np.random.default_rng(1000 + n_lags + thr)
    special = np.array([thr, -thr, thr - 1, -(thr - 1), -32768, 32767, 0])
    rows = [(np.array([thr]), np.array([-thr]))]
    far = rng.integers(-3 * thr, 3 * thr + 1, LENGTHS[1])
    far[rng.integers(0, len(far), 200)] = special[rng.integers(0, len(special), 200)]
    mic = np.roll(far, 20)
    mic[:20] = 0
    mic[rng.integers(0, len(mic), 100)] = special[rng.integers(0, len(special), 100)]
    rows.append((mic, far))
    rows.append((rng.integers(-3000, 3000, LENGTHS[2]), np.zeros(LENGTHS[2], dtype=np.int64)))
    far = rng.integers(-3000, 3000, LENGTHS[3])
    mic = np.roll(far, 37) // 2 + rng.integers(-40, 40, LENGTHS[3])
    rows.append((mic, far))
    t = np.arange(LENGTHS[4])
    rows.append((np.where(((t - 5) % 16 == 0) & (t >= n_lags), 9000, 0), np.where(t % 16 == 0, 9000, 0)))
    out = [(_codes(m, fmt), _codes(f, fmt)) for m, f in rows]
    if fmt == "f32":
        m, f = out[3]
        m[[3, 1500, 4096]] = [np.nan, np.inf, -np.inf]
        f[[7, 1500, 2047]] = [-np.inf, np.nan, np.inf]
    return out


def _padded(rows, N):
    out = np.zeros((len(rows), N), dtype=rows[0].dtype)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return torch.from_numpy(out).cuda()


# ------------------------------------------------------------------------------------------------------------------ 1. whole signals

@pytest.mark.parametrize("thr", [1, 16])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("n_lags", [64, 320, 6144])
def test_whole_signal_against_the_law(full, n_lags, fmt, thr):
    cfg = dict(BASE, n_lags=n_lags, thr=thr)
    rows = _rows(fmt, n_lags, thr)
    N = max(LENGTHS)
    mic, far = _padded([m for m, _ in rows], N), _padded([f for _, f in rows], N)
    before = mic.clone(), far.clone()
    track, report = full.echo_delay(mic, far, _lib.echo_delay_cfg(**cfg), fmt, lengths=list(LENGTHS))
    track, report = track.cpu().numpy(), report.cpu().numpy()
    assert track.shape == (5, N // 1024, 6)
    confirmed = 0
    for i, (m, f) in enumerate(rows):
        tr, rep, e = R.estimate(m, f, fmt, **cfg)
        k = len(m) // 1024
        assert np.array_equal(track[i, :k], tr) and not track[i, k:].any(), (i, track[i, :k], tr)
        assert [int(v) for v in report[i]] == rep, (i, report[i], rep)
        confirmed += rep[0] >= 0
    if fmt == "alaw" and thr <= 8:      # A-law has no zero: its silence is +-8, which a threshold this low reads as signal everywhere
        assert rep[4] > 0
    else:      # the ties: every lag 5 + 16 j holds the same sum, the lowest wins and is confirmed; the echo of row 3 is found too
        assert rep[0] == 5 and rep[4] > 0 and len({int(v) for v in e.A[5:n_lags:16]}) == 1
        assert confirmed == 2
    assert torch.equal(mic.view(torch.uint8), before[0].view(torch.uint8)) and torch.equal(far.view(torch.uint8), before[1].view(torch.uint8))


def test_the_defaults_of_a_rate_a_dict_and_one_row(full):
    far = EC.white(3, 1024 * 14 + 5)
    mic = EC.echo(far, EC.path(103), 1000)
    tr, rep, _ = R.estimate(mic, far, **R.defaults(16000))
    assert 0 <= rep[0] - 1000 < EC.PATH_TAPS
    for cfg in (16000, dict(R.defaults(16000))):
        track, report = full.echo_delay(torch.from_numpy(mic).cuda(), torch.from_numpy(far).cuda(), cfg)
        assert np.array_equal(track[0].cpu().numpy(), tr) and [int(v) for v in report[0].cpu()] == rep


# ------------------------------------------------------------------------------------------------------------------ 2. streaming

N_STREAM = 3 * 3840
CUTS = (0, 1, 63, 1280, 2049, 3840)


@functools.lru_cache(maxsize=None)
def _stream_signal(fmt, seed):
    rng = np.random.default_rng(50 + seed)
    far = rng.integers(-3000, 3000, N_STREAM)
    mic = np.roll(far, 100 + seed) // 2 + rng.integers(-40, 40, N_STREAM)
    return _codes(mic, fmt), _codes(far, fmt)


@pytest.fixture(scope="module")
def st(full):
    s = full.streams(MAX_SLOTS, 4, 64)
    s.set_input_format([1], "s16")
    s.set_input_format([2], "ulaw")
    yield s
    s.close()


def _fresh(st, slots, cfg):
    """The slots enabled from off: their states restart."""
    st.set_echo_delay(slots, None)
    st.set_echo_delay(slots, _lib.echo_delay_cfg(**cfg))


def _rec(st, slot):
    return st.echo_delay_state([slot])[0].cpu().numpy()


def _call(st, slots, mics, fars, samples=None):
    """One streaming call -> the report rows; the buffers the kernel read must keep every byte."""
    ld = max(1, max((max(m.nbytes, 4) + 3) // 4 + 1 for m in mics))
    buf, fbuf = _pack(mics, ld), _pack(fars, ld)
    b0, f0 = buf.clone(), fbuf.clone()
    rep = torch.full((len(slots), 6), -7, dtype=torch.int64, device="cuda")
    assert st.echo_delay(slots, buf, [len(m) for m in mics] if samples is None else samples, fbuf, rep) is rep
    assert torch.equal(buf, b0) and torch.equal(fbuf, f0)
    return rep.cpu().numpy()


@pytest.mark.parametrize("shift", [0, 1, 2])
def test_cuts_equal_the_whole_signal(st, shift):
    """Slots 0 (f32) and 1 (s16) take their signals in calls of CUTS samples, each at its own place in the sequence, so they stand at
    different positions in every call; slot 2 (mu-law) has no estimator and reports zeros; slot 3 has one and passes rows without
    samples."""
    cfgs = [dict(BASE), dict(BASE, n_lags=6144, thr=1)]
    _fresh(st, [0], cfgs[0])
    _fresh(st, [1], cfgs[1])
    _fresh(st, [3], BASE)
    st.set_echo_delay([2], None)
    assert st.echo_delay_cfg([0, 1, 2, 3]) == [cfgs[0], cfgs[1], None, BASE]
    sig = [_stream_signal("f32", 0), _stream_signal("s16", 1), _stream_signal("ulaw", 2)]
    pos = [0, 0, 0]
    k = 0
    last = np.zeros((2, 6), dtype=np.int64)
    while min(pos[:2]) < N_STREAM:
        take = [min(CUTS[(k + shift * (i + 1)) % len(CUTS)], N_STREAM - pos[i]) for i in range(3)]
        mics = [sig[i][0][pos[i]:pos[i] + take[i]] for i in range(3)] + [sig[0][0][:5]]
        fars = [sig[i][1][pos[i]:pos[i] + take[i]] for i in range(3)] + [sig[0][1][:5]]
        rep = _call(st, [0, 1, 2, 3], mics, fars, samples=take + [0])
        for i in range(2):
            if take[i]:
                last[i] = rep[i]
            else:
                assert not rep[i].any()      # a row without samples reports zeros
        assert not rep[2].any() and not rep[3].any()
        pos = [p + t for p, t in zip(pos, take)]
        k += 1
    for i, fmt in enumerate(("f32", "s16")):
        m, f = sig[i]
        tr, rep, e = R.estimate(m, f, fmt, **cfgs[i])
        assert rep[0] >= 0 and [int(v) for v in last[i]] == rep, (i, last[i], rep)
        assert np.array_equal(_rec(st, i), e.record()), i      # the record byte for byte: header, A, history
        # ... which is what conan_echo_delay gives for the concatenation
        track, report = st.ctx.echo_delay(torch.from_numpy(m).cuda(), torch.from_numpy(f).cuda(), dict(cfgs[i]), fmt)
        assert np.array_equal(track[0].cpu().numpy(), tr) and [int(v) for v in report[0].cpu()] == rep
    assert np.array_equal(_rec(st, 3), R.Estimator("f32", **BASE).record())      # rows without samples left slot 3 about to restart
    with pytest.raises(_lib.ConanError) as err:
        st.echo_delay_state([2])
    assert err.value.code == _lib.ERR_STATE


def test_no_row_means_no_launch_and_one_call_is_one_launch(st):
    _fresh(st, [0], BASE)
    m, f = _stream_signal("f32", 0)
    t, tf = torch.from_numpy(m[None, :2049].copy()).cuda(), torch.from_numpy(f[None, :2049].copy()).cuda()
    (_, launches) = _launches(st, lambda: st.echo_delay([0], t, 0, tf))
    assert "echo_delay_kernel" not in launches
    (_, launches) = _launches(st, lambda: st.echo_delay([0], t, 2049, tf))
    assert launches == {"echo_delay_kernel": 1}
    assert np.array_equal(_rec(st, 0), R.estimate(m[:2049], f[:2049], **BASE)[2].record())


def test_a_live_change_of_n_lags_the_hand_over_and_the_restart(full, st):
    cfg = dict(BASE, n_lags=1024)
    _fresh(st, [1], cfg)      # (s16)
    fresh = R.Estimator("s16", **cfg).record()
    assert int(st.lib.conan_echo_delay_state_bytes()) == R.STATE_BYTES
    assert np.array_equal(_rec(st, 1), fresh)      # a slot about to restart reports the restart state: zeros, est = cand = -1
    ref = R.Estimator("s16", **cfg)
    m, f = _stream_signal("s16", 1)
    lo = 0
    for n_lags, hi in ((1024, 1500), (320, 3000), (2048, 5200)):
        cfg = dict(cfg, n_lags=n_lags)
        st.set_echo_delay([1], _lib.echo_delay_cfg(**cfg))      # (no seed: an enabled slot keeps its state)
        before = ref.A.copy()
        ref.configure(**cfg)
        assert st.echo_delay_cfg([1]) == [cfg]
        got = _rec(st, 1)      # A[l] stays for l below both values, the rest is zero - already in the record the setter leaves
        assert np.array_equal(got, ref.record()) and np.array_equal(ref.A[:min(n_lags, 320)], before[:min(n_lags, 320)]) and not ref.A[n_lags:].any()
        rep = _call(st, [1], [m[lo:hi]], [f[lo:hi]])
        assert [int(v) for v in rep[0]] == ref.apply(m[lo:hi], f[lo:hi])[1]
        assert np.array_equal(_rec(st, 1), ref.record())
        lo = hi
    assert ref.A[320:2048].any() and ref.pos % 1024      # (the record travels with an open frame)
    # the hand-over: the record seeds a slot of another stream-set, which continues bit for bit (the seed's row stride is wider)
    other = full.streams(2, 4, 64)
    other.set_input_format([0], "s16")
    seed = torch.zeros(2, R.STATE_BYTES + 64, dtype=torch.uint8, device="cuda")
    seed[1, :R.STATE_BYTES] = st.echo_delay_state([1])[0]
    other.set_echo_delay([0], _lib.echo_delay_cfg(**cfg), seed=seed[1:])
    assert torch.equal(other.echo_delay_state([0])[0], seed[1, :R.STATE_BYTES])
    rep = _call(other, [0], [m[lo:9000]], [f[lo:9000]])
    assert [int(v) for v in rep[0]] == ref.apply(m[lo:9000], f[lo:9000])[1] and np.array_equal(other.echo_delay_state([0])[0].cpu().numpy(), ref.record())
    # a seed from a slot with more lags: the record the new slot reports holds zeros in A[n_lags ..] at once
    small = dict(cfg, n_lags=320)
    other.set_echo_delay([1], _lib.echo_delay_cfg(**small), seed=other.echo_delay_state([0]))
    ref.configure(**small)
    assert not ref.A[320:].any() and ref.A[:320].any() and np.array_equal(other.echo_delay_state([1])[0].cpu().numpy(), ref.record())
    other.close()
    # a reset of the front-end restarts the state (the setting stays); a reset of the models alone does not
    was = _rec(st, 1)
    st.reset([1], which=7)
    assert np.array_equal(_rec(st, 1), was)
    st.reset([1], which=8)
    assert np.array_equal(_rec(st, 1), R.Estimator("s16", **cfg).record()) and st.echo_delay_cfg([1]) == [cfg]
    rep = _call(st, [1], [m[:3000]], [f[:3000]])
    assert [int(v) for v in rep[0]] == R.estimate(m[:3000], f[:3000], "s16", **cfg)[1]


def test_refused_calls_change_nothing(st):
    _fresh(st, [0], BASE)
    m, f = _stream_signal("f32", 0)
    t, tf = torch.from_numpy(m[None, :100].copy()).cuda(), torch.from_numpy(f[None, :100].copy()).cuda()
    bad_cfg = _lib.echo_delay_cfg(**BASE)
    bad_cfg.n_lags = 6208
    for bad in (lambda: st.echo_delay([0], t, 101, tf),               # more samples than the row stride holds
                lambda: st.echo_delay([0], t, 100, torch.zeros(1, 99, device="cuda")),      # ... than the far row's stride holds
                lambda: st.echo_delay([0, 0], t.repeat(2, 1), 100, tf.repeat(2, 1)),
                lambda: st.echo_delay([0], t, -1, tf),
                lambda: st.set_echo_delay([0], bad_cfg),
                lambda: st.set_echo_delay([MAX_SLOTS], _lib.echo_delay_cfg(**BASE))):
        with pytest.raises(_lib.ConanError) as e:
            bad()
        assert e.value.code == _lib.ERR_INVALID
    assert np.array_equal(_rec(st, 0), R.Estimator("f32", **BASE).record()) and st.echo_delay_cfg([0]) == [BASE]


# ------------------------------------------------------------------------------------------------------------------ 3. the wav-in steps

def _calls(s, slots, wav, far, L=1280):
    """The wav-in ragged steps over wav [n, N] with the far end of the whole signal -> (the concatenated wav rows, the canceller's
    summed stats, the estimator's last reports, calls that took samples)."""
    n, N = wav.shape
    outs, took = [[] for _ in slots], 0
    stats, last = np.zeros((n, 4), dtype=np.int64), np.zeros((n, 6), dtype=np.int64)
    last_pos = (N - 1) // L * L
    pieces = [(p, p + L, False) for p in range(0, last_pos, L)] + [(last_pos, N, True)]
    while True:
        sd = torch.zeros(n, 4, dtype=torch.int64, device="cuda")
        rp = torch.zeros(n, 6, dtype=torch.int64, device="cuda")
        if pieces:
            lo, hi, fin = pieces.pop(0)
            rows = torch.zeros(n, L, device="cuda")
            rows[:, :hi - lo] = wav[:, lo:hi]
            frows = torch.zeros(n, L, device="cuda")
            frows[:, :hi - lo] = far[:, lo:hi]
            emit, _, _, w = s.step_wav_ragged(slots, rows, [hi - lo] * n, [fin] * n, far=frows, echo_stats=sd, echo_delay_report=rp)
            took += 1
            stats += sd.cpu().numpy()
            last = rp.cpu().numpy()
        else:
            emit, _, _, w = s.step_wav_ragged(slots, None, [0] * n, [True] * n)
            if not any(emit):
                break
        for i, e in enumerate(emit):
            if e:
                outs[i].append(w[i, :e * 320].clone())
    return [torch.cat(o) for o in outs], stats, last, took


def test_the_wav_in_step_in_every_cut(full):
    """step_wav_ragged(far=...) in calls of CUTS samples: the slots take their input through the drift resampler at 48 kHz, which
    admits any count up to two chunks, so rows are wider than seg * hop.  Slot 0 (f32) and slot 1 (s16, with a canceller behind
    the estimator) take the sequence from different places and so stand at different positions; slot 2 has no estimator; slot 3 has
    one and only rows without samples.  Report and state are conan_echo_delay's of the concatenation."""
    slots = [0, 1, 2, 3]
    s = full.streams(MAX_SLOTS, 4, 64)
    s.reset(slots, which=15)
    s.set_reference(slots, _ref(4))
    s.set_input_format([1], "s16")
    s.set_input_drift(slots, [0.0] * 4, rate=48000)
    cfgs = [dict(BASE), dict(BASE, n_lags=6144, thr=1)]
    s.set_echo_delay([0], _lib.echo_delay_cfg(**cfgs[0]))
    s.set_echo_delay([1], _lib.echo_delay_cfg(**cfgs[1]))
    s.set_echo_delay([3], _lib.echo_delay_cfg(**BASE))
    s.set_echo([1], True, taps=128, mu_shift=1)
    sig = [_stream_signal("f32", 0), _stream_signal("s16", 1), _stream_signal("f32", 2)]
    pos, k = [0, 0, 0], 0
    last = np.zeros((2, 6), dtype=np.int64)
    sizes = set()
    while min(pos[:2]) < N_STREAM:
        take = [min(CUTS[(k + 2 * i) % len(CUTS)], N_STREAM - pos[i]) for i in range(3)]
        sizes.update(take[:2])
        rows = [torch.from_numpy(sig[i][0][pos[i]:pos[i] + take[i]].copy()).cuda() for i in range(3)] + [torch.zeros(0, device="cuda")]
        fars = [torch.from_numpy(sig[i][1][pos[i]:pos[i] + take[i]].copy()).cuda() for i in range(3)] + [torch.zeros(0, device="cuda")]
        rp = torch.full((4, 6), -7, dtype=torch.int64, device="cuda")
        if any(take):
            s.step_wav_ragged(slots, rows, take + [0], [False] * 4, far=fars, echo_delay_report=rp)
            rp = rp.cpu().numpy()
            for i in range(2):
                if take[i]:
                    last[i] = rp[i]
                else:
                    assert not rp[i].any()      # a row without samples beside live rows reports zeros
            assert not rp[2].any() and not rp[3].any()
        pos = [p + t for p, t in zip(pos, take)]
        k += 1
    assert sizes >= set(CUTS)
    for i, fmt in enumerate(("f32", "s16")):
        m, f = sig[i]
        tr, rep, e = R.estimate(m, f, fmt, **cfgs[i])
        assert rep[0] >= 0 and [int(v) for v in last[i]] == rep, (i, last[i], rep)
        assert np.array_equal(_rec(s, i), e.record()), i
        track, report = full.echo_delay(torch.from_numpy(m).cuda(), torch.from_numpy(f).cuda(), dict(cfgs[i]), fmt)
        assert np.array_equal(track[0].cpu().numpy(), tr) and [int(v) for v in report[0].cpu()] == rep
    assert np.array_equal(_rec(s, 3), R.Estimator("f32", **BASE).record())      # still about to restart
    with pytest.raises(_lib.ConanError) as err:
        s.echo_delay_state([2])
    assert err.value.code == _lib.ERR_STATE
    s.close()


def test_memory_launches_and_the_canceller_behind_it(full):
    """a: canceller and estimator; b: canceller only - the parent's launches; c: an estimator and no canceller.  The estimator changes
    neither the canceller's result nor any launch of the step."""
    slots = [0, 1, 2]
    N = 5 * 1280 + 500
    rng = np.random.default_rng(3)
    far = torch.from_numpy((0.1 * rng.standard_normal((3, N))).astype(np.float32)).cuda()
    wav = (0.5 * torch.roll(far, 300, 1) + torch.from_numpy((0.01 * rng.standard_normal((3, N))).astype(np.float32)).cuda()).contiguous()
    a, b, c = (full.streams(MAX_SLOTS, 4, 64) for _ in range(3))
    never = b.state_bytes
    a.set_echo_delay([3], None)      # turning off what was never on: nothing is allocated
    assert a.state_bytes == never
    ecfg = dict(CR.defaults(16000), mu_shift=1)
    for s in (a, b):
        s.set_echo([1], True, mu_shift=1)
    with_echo = b.state_bytes
    cfg = dict(R.defaults(16000), min_peak=256, hold=2)
    for s in (a, c):
        s.set_echo_delay([1, 2], True, min_peak=256, hold=2)      # the model rate's defaults
    assert a.state_bytes == with_echo + MAX_SLOTS * R.STATE_BYTES + 4 * MAX_SLOTS * ROW_BYTES and a.echo_delay_cfg([0, 1]) == [None, cfg]
    assert b.state_bytes == with_echo and c.state_bytes == never + MAX_SLOTS * R.STATE_BYTES + 4 * MAX_SLOTS * ROW_BYTES
    for s in (a, b, c):
        s.reset(slots, which=15)
        s.set_reference(slots, _ref(3))
    (wa, sa, ra, took), la = _launches(a, lambda: _calls(a, slots, wav, far))
    (wb, sb, rb, _), lb = _launches(b, lambda: _calls(b, slots, wav, far))
    (wc, sc, rc, _), lc = _launches(c, lambda: _calls(c, slots, wav, far))      # (a far end without a canceller is allowed)
    assert "echo_delay_kernel" not in lb and not rb.any()
    assert all(torch.equal(x, y) for x, y in zip(wa, wb)) and np.array_equal(sa, sb) and sa[1].any()
    # one launch per call that took samples, in front of the step, and the step's own launches are the ones it ran before
    assert la.pop("echo_delay_kernel") == took and la == lb, (la, lb)
    assert lc.pop("echo_delay_kernel") == took and "echo_kernel" not in lc and not sc.any()
    lb.pop("echo_kernel")
    assert lc == lb
    # the reports are the law's on the rows as they came (slot 1's before the canceller rewrote them)
    for i in (1, 2):
        want = R.estimate(wav[i].cpu().numpy(), far[i].cpu().numpy(), **cfg)[1]
        assert want[0] >= 300 and [int(v) for v in ra[i]] == want == [int(v) for v in rc[i]], (i, ra[i], want)
    assert not ra[0].any()
    for s in (a, b, c):
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 4. the engine

def test_engine_follows_the_estimate_call_by_call(full):
    """The composed case of tests/test_echo_delay_ref_cpu.py through open_slots(echo=..., echo_delay=True) and feed(far=...): slot 0
    hears the path at bulk delay 3000, slot 1 an independent mic.  The canceller's stats of every call and the delay in force during
    it are the numpy references', exactly; the rule is applied at the head of the next feed, and by echo_delays() where that is
    called."""
    calls = 30
    mic, far = EC.composed_signals()
    other = EC.white(77, len(mic), 0.05)
    eng = StreamingVoiceConversionEngine(full, 2, max_ref_frames=64)
    eng.open_slots([0, 1], _ref(2), echo=dict(taps=EC.COMPOSED["taps"]), echo_delay=True)
    assert eng.st.echo_delay_cfg([0, 1]) == [R.defaults(16000)] * 2 and eng.echo_delays() == [(-1, 0, 0)] * 2
    want = [EC.composed_run(m, far, True, calls) for m in (mic, other)]
    L = EC.COMPOSED["call"]
    src = torch.from_numpy(np.stack([mic, other])).cuda()
    tfar = torch.from_numpy(np.stack([far, far])).cuda()
    for i in range(calls):
        sd = torch.zeros(2, 4, dtype=torch.int64, device="cuda")
        eng.feed(src[:, i * L:(i + 1) * L], pipelined=bool(i % 2), far=tfar[:, i * L:(i + 1) * L], echo_stats=sd)
        # the rule ran at the head of this feed on the report of the call before: the delay in force during call i is the one the
        # reference holds after call i - 1 (the setting is read on the host; nothing is applied here)
        in_force = [c["delay"] for c in eng.st.echo_cfg([0, 1])]
        got = eng.echo_delays() if i in (14, calls - 1) else None      # (reads this call's report and applies the rule now)
        for k in range(2):
            stats, delays, reports = want[k]
            assert [int(v) for v in sd[k].cpu()] == [int(v) for v in stats[i]], (i, k)
            assert in_force[k] == (delays[i - 1] if i else 0), (i, k, in_force[k])
            if got is not None:
                assert got[k] == (int(reports[i][0]), int(reports[i][1]), delays[i]), (i, k, got[k])
    eng.st.join()
    assert want[0][1][-1] == 2873 and set(want[1][1]) == {0}      # (slot 0 moved onto the path; slot 1 never confirmed anything)
    assert torch.equal(src, torch.from_numpy(np.stack([mic, other])).cuda())      # (the engine works in a copy of each chunk)
