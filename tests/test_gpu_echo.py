"""Echo cancellation on the GPU (conan_streams_set_echo, conan_streams_echo, conan_streams_echo_state, conan_echo; include/conan_hip.h,
conan_echo_cfg), bit for bit against tests/echo_ref.py: the whole-signal form, the streaming form in every cut, in all four sample
formats; rows of other slots and rows without samples keep their bytes; the state records byte for byte; every branch of a block's
end; a live change of taps; the hand-over; a stream-set that never enables the feature keeps its memory and its launches; and the
engine end to end.  Nothing here has a tolerance: the law is integer arithmetic and one f32 subtraction.

The shapes are the smallest that reach every path: rows one sample short of a block, one block, one over, and five blocks and a
rest; the shortest and the longest filter; no delay, one sample and the longest delay (with one row long enough for the delayed far
end to arrive); calls of 1, 63, 64, 65 and 127 samples."""
import functools

import numpy as np
import pytest
import torch

from conan_amd import _lib
from conan_amd.engine import StreamingVoiceConversionEngine
from tests import echo_ref as R
from tests import sample_format_ref as SF
from tests.test_gpu_f0 import _launches, _ref
from tests.test_gpu_pitch import full  # noqa: F401  (module fixture: the small synthetic full model)

pytestmark = pytest.mark.gpu

MAX_SLOTS = 6
FMTS = ("f32", "s16", "ulaw", "alaw")
STATE_BYTES = R.STATE_BYTES
ROW_BYTES = 80      # one table row of the kernel (streams.h: four tables of max_slots rows)
PAD = 0xAB
BASE = dict(taps=128, delay=5, mu_shift=1, dt_num=1, dt_den=2, hang=2, reg=128 * 64, far_min=1000)


@functools.lru_cache(maxsize=None)
def _signal(fmt, n, seed=0, delay=0):
    """(mic codes, far codes) of fmt: a white far end and its echo through a short path behind `delay` samples, plus a little noise."""
    rng = np.random.default_rng(100 + seed)
    far = rng.standard_normal(n) * 0.2
    h = rng.standard_normal(24) * np.exp(-np.arange(24) / 6.0) * 0.08      # (quiet enough for the Geigel test to pass it)
    echo = np.convolve(np.concatenate([np.zeros(delay), far]), h)[:n]
    mic = echo + rng.standard_normal(n) * 0.002
    return SF.encode(mic.astype(np.float32), fmt), SF.encode(far.astype(np.float32), fmt)


def _same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    return got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def _pack(rows, ld):
    """Rows (numpy, each in its own format's dtype) packed from the start of rows ld * 4 bytes apart; the bytes behind them are PAD."""
    buf = np.full((len(rows), ld * 4), PAD, dtype=np.uint8)
    for i, r in enumerate(rows):
        buf[i, :r.nbytes] = r.view(np.uint8)
    return torch.from_numpy(buf).cuda()


def _unpack(buf, rows):
    raw = buf.cpu().numpy()
    for i, r in enumerate(rows):
        assert (raw[i, r.nbytes:] == PAD).all(), "bytes behind a row's samples were written"
    return [raw[i, :r.nbytes].view(r.dtype).copy() for i, r in enumerate(rows)]


@pytest.fixture(scope="module")
def st(full):
    s = full.streams(MAX_SLOTS, 4, 64)
    for slot, fmt in enumerate(FMTS):
        if fmt != "f32":
            s.set_input_format([slot], fmt)
    yield s
    s.close()


def _fresh(st, slots, cfg):
    """The slots enabled from off: their states restart."""
    st.set_echo(slots, None)
    st.set_echo(slots, _lib.echo_cfg(**cfg))


def _cancel(st, slot, mic, far, stats=False):
    """One streaming call on one slot -> the row (and the stats)."""
    ld = max(1, (max(mic.nbytes, 4) + 3) // 4 + 1)
    buf, fbuf = _pack([mic], ld), _pack([far], ld)
    sd = torch.full((1, 4), -1, dtype=torch.int64, device="cuda") if stats else None
    st.echo([slot], buf, len(mic), fbuf, sd)
    out = _unpack(buf, [mic])[0]
    return (out, [int(v) for v in sd[0].cpu()]) if stats else out


def _rec(st, slot):
    return st.echo_state([slot])[0].cpu().numpy()


def _seed(st, slot, ref):
    """The reference's state becomes the slot's."""
    st.set_echo([slot], _lib.echo_cfg(**{f: getattr(ref, f) for f in R.FIELDS}), seed=torch.from_numpy(ref.record()[None].copy()).cuda())


# ------------------------------------------------------------------------------------------------------------------ 1. whole signals

LENGTHS = (63, 64, 65, 64 * 5 + 17)


@pytest.mark.parametrize("delay", [0, 1, 4096])
@pytest.mark.parametrize("taps", [64, 2048])
@pytest.mark.parametrize("fmt", FMTS)
def test_whole_signal_against_the_law(full, fmt, taps, delay):
    lengths = list(LENGTHS) + [delay + 64 * 3 + 5]      # (the last row is long enough for the delayed far end to arrive)
    N = max(lengths)
    # (behind the longest delay x' is zero for 4096 samples, which the Geigel test reads as double talk with hang-over: off there)
    cfg = dict(BASE, taps=taps, delay=delay, reg=taps * 64, dt_den=0 if delay == 4096 else 2)
    sig = [_signal(fmt, N, seed=i, delay=delay) for i in range(len(lengths))]
    mic = torch.from_numpy(np.stack([m for m, _ in sig])).cuda()
    far = torch.from_numpy(np.stack([f for _, f in sig])).cuda()
    got, stats = full.echo(mic, far, _lib.echo_cfg(**cfg), fmt, lengths=lengths, stats=True)
    stats = stats.cpu().numpy()
    changed = 0
    for i, (n, (m, f)) in enumerate(zip(lengths, sig)):
        want, st_want, c = R.cancel(m[:n], f[:n], fmt, **cfg)
        assert _same(got[i, :n], want) and _same(got[i, n:], m[n:]), (i, n)      # (the samples behind a row's length keep their bytes)
        assert [int(v) for v in stats[i]] == st_want, (i, n)
        changed += int(np.any(want != m[:n]))
    assert changed >= 1      # (rows shorter than two blocks cannot change: the first block's weights are zero)
    assert _same(mic, np.stack([m for m, _ in sig]))      # (the caller's tensor keeps its samples)


def test_the_defaults_of_a_rate_a_dict_and_one_row(full):
    m, f = _signal("f32", 64 * 20 + 3, seed=9)
    want, _, c = R.cancel(m, f, "f32", **R.defaults(16000))
    assert c.adapted > 0
    assert _same(full.echo(torch.from_numpy(m).cuda(), torch.from_numpy(f).cuda(), 16000), want)
    assert _same(full.echo(torch.from_numpy(m).cuda(), torch.from_numpy(f).cuda(), dict(R.defaults(16000))), want)


# ------------------------------------------------------------------------------------------------------------------ 2. streaming

N_STREAM = 64 * 3 + 17


@functools.lru_cache(maxsize=None)
def _want_stream(fmt):
    m, f = _signal(fmt, N_STREAM, seed=3, delay=BASE["delay"])
    out, stats, c = R.cancel(m, f, fmt, **BASE)
    assert c.adapted >= 2 and np.any(out != m)
    return out, stats, c.record()


@pytest.mark.parametrize("step", [1, 63, 64, 65, 127])
def test_cuts_equal_the_whole_signal_in_every_format_in_one_call(st, step):
    """Slots 0 .. 3 (f32, s16, mu-law, A-law) cancel their signals call by call in the same launches; slot 4 has no canceller and keeps
    its bytes; slot 5 has one and passes rows without samples."""
    _fresh(st, [0, 1, 2, 3, 5], BASE)
    st.set_echo([4], None)
    assert st.echo_cfg([0, 4, 5]) == [BASE, None, BASE]
    sig = [_signal(fmt, N_STREAM, seed=3, delay=BASE["delay"]) for fmt in FMTS]
    other = _signal("f32", N_STREAM, seed=4)
    outs = [[] for _ in range(6)]
    total = np.zeros((6, 4), dtype=np.int64)
    ld = step + 1      # (f32 rows fill `step` of the step + 1 words: a stride that is not the row's length)
    for lo in range(0, N_STREAM, step):
        hi = min(lo + step, N_STREAM)
        rows = [m[lo:hi] for m, _ in sig] + [other[0][lo:hi]] * 2
        fars = [f[lo:hi] for _, f in sig] + [other[1][lo:hi]] * 2
        buf, fbuf = _pack(rows, ld), _pack(fars, ld)
        sd = torch.full((6, 4), -1, dtype=torch.int64, device="cuda")
        assert st.echo(list(range(6)), buf, [hi - lo] * 5 + [0], fbuf, sd) is buf
        total += sd.cpu().numpy()
        for i, r in enumerate(_unpack(buf, rows)):
            outs[i].append(r)
    for i, fmt in enumerate(FMTS):
        want, stats, rec = _want_stream(fmt)
        assert _same(np.concatenate(outs[i]), want), fmt
        assert [int(v) for v in total[i]] == stats, fmt
        assert np.array_equal(_rec(st, i), rec), fmt      # the record byte for byte: weights, pending e, counters, history
        # ... which is what conan_echo gives for the whole signal
        m, f = sig[i]
        assert _same(st.ctx.echo(torch.from_numpy(m).cuda(), torch.from_numpy(f).cuda(), dict(BASE), fmt), want), fmt
    assert _same(np.concatenate(outs[4]), other[0]) and _same(np.concatenate(outs[5]), other[0])
    assert not total[4].any() and not total[5].any()      # skipped rows report zeros
    fresh = R.Canceller("f32", **BASE)
    assert np.array_equal(_rec(st, 5), fresh.record())      # rows without samples left slot 5 about to restart


def test_a_float32_tensor_is_cancelled_in_place_and_no_row_means_no_launch(st):
    _fresh(st, [0], BASE)
    m, f = _signal("f32", N_STREAM, seed=3, delay=BASE["delay"])
    t = torch.from_numpy(m[None].copy()).cuda()
    (_, launches) = _launches(st, lambda: st.echo([0], t, 0, torch.from_numpy(f[None].copy()).cuda()))
    assert "echo_kernel" not in launches and _same(t[0], m)
    (got, launches) = _launches(st, lambda: st.echo([0], t, len(m), torch.from_numpy(f[None].copy()).cuda()))
    assert got is t and launches.get("echo_kernel") == 1
    assert _same(t[0], _want_stream("f32")[0])


# ------------------------------------------------------------------------------------------------------------------ 3. the branches

def _both(st, slot, ref, mic, far):
    """The same call on the slot and on the reference: rows, stats and records must agree."""
    got, stats = _cancel(st, slot, mic, far, stats=True)
    want, _, st_want = ref.apply(mic, far)
    assert _same(got, want) and stats == st_want
    assert np.array_equal(_rec(st, slot), ref.record())


def test_guard_trip_from_seeded_large_weights(st):
    cfg = dict(BASE, dt_den=0)
    ref = R.Canceller("f32", **cfg)
    ref.w[:] = np.random.default_rng(1).integers(-2 ** 28, 2 ** 28, ref.taps)
    _seed(st, 0, ref)
    assert np.array_equal(_rec(st, 0), ref.record())
    m, f = _signal("f32", 64 * 3 + 10, seed=5, delay=cfg["delay"])
    _both(st, 0, ref, m, f)
    assert ref.trips == 1 and ref.shift == cfg["mu_shift"] + 1 and ref.adapted >= 1      # block 0 trips and clears w; the next ones adapt
    ref.shift, ref.w[:] = R.MAX_SHIFT, 2 ** 28      # the back-off stops at CONAN_ECHO_MAX_SHIFT
    _seed(st, 0, ref)
    _both(st, 0, ref, m[:64], f[:64])
    assert ref.trips == 2 and ref.shift == R.MAX_SHIFT and not ref.w.any()


def test_a_frozen_block_and_its_hang_over(st):
    cfg = dict(BASE, hang=2)
    _fresh(st, [1], cfg)      # (s16)
    ref = R.Canceller("s16", **cfg)
    n = 64 * 7
    m, f = _signal("s16", n, seed=6, delay=cfg["delay"])
    m = m.copy()
    m[64 + 10] = 30000      # a near-end peak in block 1: dmax * 2 > xmax
    _both(st, 1, ref, m, f)
    # block 0 adapts, block 1 is frozen by the condition, blocks 2 and 3 by the hang-over, block 4 on adapt again
    assert (ref.adapted, ref.frozen, ref.hcnt) == (4, 3, 0)


def test_an_idle_far_end_does_not_adapt(st):
    cfg = dict(BASE, dt_den=0, far_min=128 * 100)
    _fresh(st, [0], cfg)
    ref = R.Canceller("f32", **cfg)
    m, f = _signal("f32", 64 * 6, seed=7, delay=cfg["delay"])
    f = f.copy()
    f[:64 * 3] = (f[:64 * 3] * np.float32(2.0 ** -12)).astype(np.float32)      # a far end of a few LSB: P < far_min
    _both(st, 0, ref, m[:64 * 3], f[:64 * 3])
    assert ref.adapted == 0 and not ref.w.any()
    _both(st, 0, ref, m[64 * 3:], f[64 * 3:])
    assert ref.adapted >= 2      # (block 3's window still holds the quiet samples; from block 5 on P counts loud ones only)


def test_a_weight_at_the_clamp(st):
    cfg = dict(taps=64, delay=0, mu_shift=0, dt_num=1, dt_den=0, hang=0, reg=1, far_min=0)
    _fresh(st, [0], cfg)
    ref = R.Canceller("f32", **cfg)
    sign = np.random.default_rng(8).integers(0, 2, 64 * 3) * 2 - 1
    f = (sign / 32768.0).astype(np.float32)      # a far end of one LSB
    m = (sign * 0.6).astype(np.float32)          # ... and a mic that follows it: one update's step is beyond 2^31
    _both(st, 0, ref, m, f)
    assert ref.adapted >= 1 and np.any(np.abs(ref.w) == R.WMAX)


def test_a_live_change_of_taps_keeps_the_weights_that_still_exist(st):
    cfg = dict(BASE, taps=256, reg=256 * 64)
    _fresh(st, [2], cfg)      # (mu-law)
    ref = R.Canceller("ulaw", **cfg)
    m, f = _signal("ulaw", 64 * 8 + 9, seed=8, delay=cfg["delay"])
    _both(st, 2, ref, m[:330], f[:330])
    assert ref.w[128:].any()
    for taps, lo, hi in ((128, 330, 430), (256, 430, len(m))):
        cfg = dict(cfg, taps=taps)
        st.set_echo([2], _lib.echo_cfg(**cfg))      # (no seed: an enabled slot keeps its state)
        ref.configure(**cfg)
        assert st.echo_cfg([2]) == [cfg]
        _both(st, 2, ref, m[lo:hi], f[lo:hi])


def test_hand_over_state_query_and_reset(st):
    a, b = 0, 5
    _fresh(st, [a], BASE)
    st.set_echo([b], None)
    assert int(st.lib.conan_echo_state_bytes()) == STATE_BYTES
    fresh = R.Canceller("f32", **BASE).record()
    assert np.array_equal(_rec(st, a), fresh)      # a slot about to restart reports the restart state: zeros, shift = mu_shift
    with pytest.raises(_lib.ConanError) as e:
        st.echo_state([b])
    assert e.value.code == _lib.ERR_STATE
    m, f = _signal("f32", N_STREAM, seed=3, delay=BASE["delay"])
    want, _, rec = _want_stream("f32")
    got = [_cancel(st, a, m[:83], f[:83])]      # (the call ends inside a block: pending e travel with the record)
    # the hand-over: the record seeds another slot, which continues bit for bit (two rows: the seed's row stride is wider than a record)
    seed = torch.zeros(2, STATE_BYTES + 64, dtype=torch.uint8, device="cuda")
    seed[1, :STATE_BYTES] = st.echo_state([a])[0]
    st.set_echo([b], _lib.echo_cfg(**BASE), seed=seed[1:])
    assert torch.equal(st.echo_state([b])[0], seed[1, :STATE_BYTES])
    got.append(_cancel(st, b, m[83:150], f[83:150]))
    # ... and back, through a setter call that changes nothing else: an enabled slot keeps its state without a seed
    st.set_echo([a], _lib.echo_cfg(**BASE), seed=st.echo_state([b]))
    st.set_echo([a], _lib.echo_cfg(**BASE))
    got.append(_cancel(st, a, m[150:], f[150:]))
    assert _same(np.concatenate(got), want) and np.array_equal(_rec(st, a), rec)
    # a reset of the front-end restarts the state (the setting stays); a reset of the models alone does not
    st.reset([a], which=7)
    assert np.array_equal(_rec(st, a), rec)
    st.reset([a], which=8)
    assert np.array_equal(_rec(st, a), fresh) and st.echo_cfg([a]) == [BASE]
    assert _same(_cancel(st, a, m, f), want)
    st.set_echo([b], None)


def test_refused_calls_change_nothing(st):
    _fresh(st, [0], BASE)
    m, f = _signal("f32", N_STREAM, seed=3, delay=BASE["delay"])
    t, tf = torch.from_numpy(m[None].copy()).cuda(), torch.from_numpy(f[None].copy()).cuda()
    for bad in (lambda: st.echo([0], t, len(m) + 1, tf),               # more samples than the row stride holds
                lambda: st.echo([0], t, len(m), torch.zeros(1, len(m) - 1, device="cuda")),      # ... than the far row's stride holds
                lambda: st.echo([0, 0], t.repeat(2, 1), len(m), tf.repeat(2, 1)),
                lambda: st.echo([0], t, -1, tf),
                lambda: st.set_echo([0], _lib.echo_cfg(**dict(BASE, taps=2112))),
                lambda: st.set_echo([MAX_SLOTS], _lib.echo_cfg(**BASE))):
        with pytest.raises(_lib.ConanError) as e:
            bad()
        assert e.value.code == _lib.ERR_INVALID
    assert _same(t[0], m) and np.array_equal(_rec(st, 0), R.Canceller("f32", **BASE).record()) and st.echo_cfg([0]) == [BASE]
    st.echo([0], t, len(m), tf)
    assert _same(t[0], _want_stream("f32")[0])


# ------------------------------------------------------------------------------------------------------------------ 4. memory and launches

def _calls(s, slots, wav, far=None):
    """infer_wav's calls over wav [n, N] with the far end of the whole signal -> (the concatenated wav, calls that took samples)."""
    L, outs, took = 4 * 320, [], 0
    n, N = wav.shape
    last = (N - 1) // L * L
    pieces = [(p, p + L, False) for p in range(0, last, L)] + [(last, N, True)]
    while True:
        if pieces:
            lo, hi, fin = pieces.pop(0)
            e, _, _, w = s.step_wav(slots, wav[:, lo:hi].clone(), final=fin, far=None if far is None else far[:, lo:hi])
            took += 1
        else:
            e, _, _, w = s.step_wav(slots, wav[:, :0], final=True)
            if e == 0:
                break
        if e:
            outs.append(w.clone())
    return torch.cat(outs, 1), took


def test_a_stream_set_that_never_enables_it_keeps_its_memory_and_its_launches(full):
    slots = [0, 1, 2]
    N = 2 * 1280 + 500
    rng = np.random.default_rng(3)
    far = torch.from_numpy((0.1 * rng.standard_normal((3, N))).astype(np.float32)).cuda()
    wav = (0.5 * torch.roll(far, 3, 1) + torch.from_numpy((0.01 * rng.standard_normal((3, N))).astype(np.float32)).cuda()).contiguous()
    a, b = full.streams(MAX_SLOTS, 4, 64), full.streams(MAX_SLOTS, 4, 64)
    never = b.state_bytes
    assert a.state_bytes == never
    a.set_echo([4], None)      # turning off what was never on: nothing is allocated
    assert a.state_bytes == never
    a.set_echo([1], True, mu_shift=1)      # the model rate's defaults
    assert a.state_bytes == never + MAX_SLOTS * STATE_BYTES + 4 * MAX_SLOTS * ROW_BYTES
    cfg = dict(R.defaults(16000), mu_shift=1)
    assert a.echo_cfg([1]) == [cfg]
    for s in (a, b):
        s.reset(slots, which=15)
        s.set_reference(slots, _ref(3))
    (wa, took), la = _launches(a, lambda: _calls(a, slots, wav, far))
    (wb, _), lb = _launches(b, lambda: _calls(b, slots, wav, far))      # (the far end of a stream-set without the feature cancels nothing)
    b.reset(slots, which=15)
    b.set_reference(slots, _ref(3))
    (wc, _), lc = _launches(b, lambda: _calls(b, slots, wav))
    assert torch.equal(wb, wc) and lb == lc and "echo_kernel" not in lb
    # the slots without the feature keep their bits; the cancelled one is the run over the cancelled signal
    assert torch.equal(wa[0], wb[0]) and torch.equal(wa[2], wb[2]) and not torch.equal(wa[1], wb[1])
    fixed = wav.clone()
    fixed[1] = full.echo(wav[1], far[1], dict(cfg))
    assert not torch.equal(fixed[1], wav[1])
    b.reset(slots, which=15)
    b.set_reference(slots, _ref(3))
    assert torch.equal(_calls(b, slots, fixed)[0], wa)
    # one launch per call that took samples, in front of the step, and the step's own launches are the ones it ran before
    assert la.pop("echo_kernel") == took and la == lb, (la, lb)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------------------------ 5. the engine

@pytest.mark.parametrize("form", ["f32", "s16", "in_8k"])
def test_engine_infer_wav_equals_the_cancelled_signal(full, form):
    n = 2
    rate = 8000 if form == "in_8k" else 16000
    N = 2 * (rate // 50) * 4 + 3 * (rate // 50) + 7
    rng = np.random.default_rng(9)
    far = (0.1 * rng.standard_normal((n, N))).astype(np.float32)
    mic = (0.5 * np.roll(far, 2, 1) + 0.05 * np.sin(2 * np.pi * 180.0 * np.arange(N) / rate)).astype(np.float32)
    fmt = "s16" if form == "s16" else "f32"
    src, far = torch.from_numpy(SF.encode(mic, fmt)).cuda(), torch.from_numpy(SF.encode(far, fmt)).cuda()
    kw = dict(in_format=None if fmt == "f32" else fmt, in_rate=None if rate == 16000 else rate)
    cfg = dict(R.defaults(rate), mu_shift=1, dt_den=0)
    eng = StreamingVoiceConversionEngine(full, n, max_ref_frames=64)
    fixed = full.echo(src, far, dict(cfg), fmt)
    assert not torch.equal(fixed, src)
    want = eng.infer_wav(fixed, _ref(n), pipelined=False, **kw)
    before = src.clone()
    for pipelined, echo in ((False, dict(cfg)), (True, _lib.echo_cfg(**cfg))):
        got = eng.infer_wav(src, _ref(n), pipelined=pipelined, echo=echo, far=far, **kw)
        torch.cuda.synchronize()
        assert all(torch.equal(g, w) for g, w in zip(got, want)), (form, pipelined)
    assert torch.equal(src, before)      # (the engine cancels in a copy of each chunk)
    # the slots keep the setting; without a far end nothing is cancelled
    assert eng.st.echo_cfg(eng.slots) == [cfg] * n
    plain = eng.infer_wav(src, _ref(n), pipelined=False, echo=True, **kw)
    off = eng.infer_wav(src, _ref(n), pipelined=False, **kw)
    assert all(torch.equal(g, w) for g, w in zip(plain, off)) and eng.st.echo_cfg(eng.slots) == [None] * n


def test_engine_staggered_utterances(full):
    L = 1280
    rng = np.random.default_rng(4)
    lens = [2 * L + 400, L + 900, 3 * L]
    fars = [torch.from_numpy((0.1 * rng.standard_normal(N)).astype(np.float32)).cuda() for N in lens]
    srcs = [(0.5 * torch.roll(f, 1) + 0.01 * torch.sin(torch.arange(len(f), device="cuda") * 0.07)).contiguous() for f in fars]
    cfg = dict(R.defaults(16000), mu_shift=1, dt_den=0)
    eng = StreamingVoiceConversionEngine(full, 2, max_ref_frames=64)
    fixed = [full.echo(srcs[0], fars[0], dict(cfg)), srcs[1], full.echo(srcs[2], fars[2], dict(cfg))]
    assert not torch.equal(fixed[0], srcs[0])
    want = eng.infer_wav_staggered(fixed, [0, 1, 2], _ref(3), pipelined=False)
    got = eng.infer_wav_staggered(srcs, [0, 1, 2], _ref(3), pipelined=False, echo=[dict(cfg), None, dict(cfg)], far=[fars[0], None, fars[2]])
    for u in range(3):
        assert all(torch.equal(g, w) for g, w in zip(got[u], want[u])), u
