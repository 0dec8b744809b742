"""Clock-drift compensation on the GPU (conan_resample_drift, conan_streams_set_input_drift / _set_output_drift): every comparison
is bit for bit against tests/drift_ref.py, which takes the library's own table (conan_resample_drift_table), so the sums alone are
under test; the streams are held to the whole-signal entry point under the schedule their own counters report."""
import numpy as np
import pytest
import torch

from conan_amd import _lib
from conan_amd.engine import StreamingVoiceConversionEngine
from tests import drift_ref as R
from tests.wav_helpers import HOP, L, SENTINEL, _equal, _mel, _profiled, _ref, _sig, _voc_run, ctx  # noqa: F401  (ctx: module fixture)

pytestmark = pytest.mark.gpu

SIDES = {"source": R.SOURCE, "sink": R.SINK}
N_IN = 700          # 16k -> 16k: three tiles of 256 outputs, the last partial; 8k -> 16k: six; 48k -> 16k: one
RATES = [(16000, 16000), (8000, 16000), (48000, 16000), (16000, 8000), (16000, 48000)]
KAISER16 = dict(lowpass_filter_width=16, resampling_method="sinc_interp_kaiser")

_tables = {}


def _table(fin, fout, **kw):
    key = (fin, fout, tuple(sorted(kw.items())))
    if key not in _tables:
        _tables[key] = _lib.resample_drift_table(fin, fout, **kw)
    return _tables[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(ctx, x, fin, fout, side, sched_ppb, **kw):
    """ctx.resample_drift under the schedule [(at, ppb)] against the reference; returns the output count."""
    drift = [(a, p / 1000.0) for a, p in sched_ppb]
    assert [_lib.drift_ppb(p) for _, p in drift] == [p for _, p in sched_ppb]
    y = ctx.resample_drift(x, fin, fout, drift, side=side, **kw).cpu().numpy()
    want = R.whole(x.cpu().numpy(), _table(fin, fout, **kw), fin, fout, SIDES[side], sched_ppb)
    assert y.shape == want.shape, (y.shape, want.shape)
    bad = np.flatnonzero((_bits(y) != _bits(want)).any(axis=0))
    assert bad.size == 0, (fin, fout, side, sched_ppb, bad[:8], y[:, bad[:4]], want[:, bad[:4]])
    return y.shape[-1]


@pytest.mark.parametrize("side", ["source", "sink"])
@pytest.mark.parametrize("rates", RATES, ids=lambda r: "%d-%d" % r)
def test_whole_signal_constant_drift(ctx, rates, side):
    """2 rows x 700 inputs at ppb 0, +300 000, -150 000 and the law's limits +-2 000 000; the first and last W outputs (taps outside the signal) are in the
    comparison, and the counts are the closed form's."""
    fin, fout = rates
    x = _sig(2, N_IN, fin, 11)
    for ppb in (0, 300000, -150000, 2000000, -2000000):
        n = _check(ctx, x, fin, fout, side, [(0, ppb)])
        assert n == R.length(fin, fout, SIDES[side], [(0, ppb)], N_IN)
        assert n == _lib.resample_drift_length(fin, fout, N_IN, ppb / 1000.0, side=side)


@pytest.mark.parametrize("side", ["source", "sink"])
@pytest.mark.parametrize("rates", RATES[:3], ids=lambda r: "%d-%d" % r)
def test_whole_signal_schedules(ctx, rates, side):
    """Three segments whose change points lie 1, 255, 256 and 257 outputs into a tile (tile 1 where the signal has one)."""
    fin, fout = rates
    x = _sig(2, N_IN, fin, 12)
    nout = R.length(fin, fout, SIDES[side], [(0, 2000000 if side == "sink" else -2000000)], N_IN)
    t = 256 if nout > 2 * 256 else 0
    for a, b in ((1, 255), (255, 256), (256, 257), (1, 257)):
        sched = [(0, 300000), (t + a, -2000000), (t + b, 2000000)]
        if t + b >= nout:       # (48k -> 16k has one tile of 233 outputs: keep the points inside it)
            sched = [(0, 300000), (a if a < nout else 2, -2000000), (nout - 3, 2000000)]
        _check(ctx, x, fin, fout, side, sched)


def test_whole_signal_kaiser_and_shapes(ctx):
    """A wider filter (2W = 98 taps at 48k -> 16k), one row, a 1-D input, and a signal shorter than the filter."""
    x = _sig(1, 2000, 48000, 13)
    _check(ctx, x, 48000, 16000, "source", [(0, 300000), (300, -150000)], **KAISER16)
    _check(ctx, _sig(1, N_IN, 8000, 14), 8000, 16000, "sink", [(0, -150000)], **KAISER16)
    short = _sig(3, 5, 16000, 15)
    _check(ctx, short, 16000, 16000, "source", [(0, 2000000)])
    y = ctx.resample_drift(x[0], 48000, 16000, 300.0)
    assert y.dim() == 1 and y.shape[0] == _lib.resample_drift_length(48000, 16000, 2000, 300.0)


def test_identity(ctx):
    """rolloff = 1, ppb = 0, equal rates: the taps are a unit impulse and the output is the input, bit for bit."""
    x = _sig(2, 1000, 16000, 16)
    for side in ("source", "sink"):
        y = ctx.resample_drift(x, 16000, 16000, 0.0, side=side, rolloff=1.0)
        assert y.shape == x.shape and np.array_equal(_bits(y.cpu().numpy()), _bits(x.cpu().numpy()))
    # and the default filter is one: ppb = 0 at equal rates is filtered, not copied
    assert not torch.equal(ctx.resample_drift(x, 16000, 16000, 0.0), x)


def test_refusals(ctx):
    x = _sig(1, N_IN, 48000, 17)
    with pytest.raises(ValueError):
        ctx.resample_drift(x, 48000, 16000, 2000.5)                                   # |ppb| > 2 000 000
    with pytest.raises(ValueError):
        ctx.resample_drift(x, 48000, 16000, [(1, 0.0)])                               # a schedule starts at output 0
    with pytest.raises(ValueError):
        ctx.resample_drift(x, 48000, 16000, 0.0, side="both")
    with pytest.raises(ValueError):
        ctx.resample_drift(x, 48000, 16000, 0.0, lowpass_filter_width=128)            # 2W > 512
    cfg = _lib.resample_cfg(48000, 16000)
    at, ppb = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32)
    y = torch.empty(1, 300, device="cuda")
    rc = ctx.lib.conan_resample_drift(ctx.h, _lib.C.byref(cfg), 0, _lib.C.c_void_p(x.data_ptr()), 1, N_IN, at.ctypes.data, ppb.ctypes.data, 1,
                                      _lib.C.c_void_p(y.data_ptr()), 100, None, None)    # y_ld below the output length
    assert rc == _lib.ERR_INVALID


# ---- streams: the input side
def _engine(ctx, n=1):
    eng = StreamingVoiceConversionEngine(ctx, n, max_ref_frames=64)
    eng.start_wav(_ref(n))
    return eng


def _source(ctx, rate, N, fmt, seed):
    """A source row in the slot's input format [1, N] and its decoded floats."""
    x = _sig(1, N, rate, seed)
    if fmt == "f32":
        return x, x
    raw = ctx.convert_samples(x, "f32", fmt)
    return raw, ctx.convert_samples(raw, fmt, "f32")


def _drive_input(eng, src, sizes, changes, s_in):
    """One slot fed `sizes` samples per call (then the rest with final, then drain calls); changes: call index -> ppm set before
    that call.  -> (the schedule in output indices from input_drift(), frames the front-end emitted, step outputs)."""
    st = eng.st
    sched = [(0, st.input_drift([0])[0][0])]
    frames, outs, pos, k = [], [], 0, 0
    N = src.shape[1]
    while True:
        if k in changes:
            ppm, _, out = st.input_drift([0])[0]
            st.set_input_drift([0], changes[k])
            if out == sched[-1][0]:
                sched[-1] = (out, changes[k])
            else:
                sched.append((out, changes[k]))
        final = k >= len(sizes)
        m = (N - pos) if final else sizes[k]
        assert pos + m <= N and m <= 2 * s_in
        before = st.input_drift([0])[0][2]
        e, c, mel, w = st.step_wav([0], src[:, pos:pos + m], final=final)
        pos += m
        k += 1
        if e:
            frames.append(st.wav_chunk(1)[:, :e].clone())
            outs.append((w.clone(), mel.clone(), c[:, :e].clone()))
        elif final and m == 0 and st.input_drift([0])[0][2] == before:      # a drain call that handed nothing over and emitted nothing
            break
        assert k < len(sizes) + 40
    torch.cuda.synchronize()
    return sched, torch.cat(frames, 1), [torch.cat(t, 1) for t in zip(*outs)]


STREAM_IN = [(16000, "f32", 6), (8000, "ulaw", 6), (48000, "s16", 9)]


@pytest.mark.parametrize("rate,fmt,calls", STREAM_IN, ids=lambda v: str(v))
def test_stream_input_equals_whole_signal(ctx, rate, fmt, calls):
    """One slot fed s_in - 1, s_in and s_in + 1 samples in an irregular pattern, a 0-sample call and one of 2 * s_in; the drift
    changes before three of the calls, once while output is owed (behind the 2 * s_in call).  At 48 kHz nine calls take the input
    index past the history ring's 32768."""
    s_in = L * rate // 16000
    sizes = [s_in + 1, s_in - 1, 2 * s_in, 0, s_in, s_in + 1, s_in - 1, s_in, s_in + 1][:calls]
    N = sum(sizes) + s_in // 2 + 3
    raw, x = _source(ctx, rate, N, fmt, 21)
    eng = _engine(ctx)
    if fmt != "f32":
        eng.st.set_input_format([0], fmt)
    eng.st.set_input_drift([0], 300.0, rate=rate)
    sched, frames, got = _drive_input(eng, raw, sizes, {1: -150.0, 3: 2000.0, 5: -2000.0}, s_in)
    assert len(sched) == 4 and sched[2][0] > sched[1][0]
    ppm, n_in, n_out = eng.st.input_drift([0])[0]
    assert n_in == N and ppm == -2000.0
    if calls == 9:
        assert N > 32768
    res = ctx.resample_drift(x, rate, 16000, sched)
    assert n_out == res.shape[1] == R.length(rate, 16000, R.SOURCE, [(a, _lib.drift_ppb(p)) for a, p in sched], N)
    # the whole-signal kernel is the reference's (tests above); here once more on this signal, against numpy
    want = R.whole(x.cpu().numpy(), _table(rate, 16000), rate, 16000, R.SOURCE, [(a, _lib.drift_ppb(p)) for a, p in sched])
    assert np.array_equal(_bits(res.cpu().numpy()), _bits(want))
    mel = ctx.wav2mel(res)
    assert frames.shape[1] == 1 + res.shape[1] // HOP and torch.equal(frames, mel[:, :frames.shape[1]])
    ref = StreamingVoiceConversionEngine(ctx, 1, max_ref_frames=64)
    w, m, c = ref.infer(mel, _ref(1), pipelined=False)
    torch.cuda.synchronize()
    assert _equal(got, (w, m, c))


# ---- streams: the output side
STREAM_OUT = [(8000, "ulaw"), (16000, "f32"), (48000, "f32")]


@pytest.mark.parametrize("rate,fmt", STREAM_OUT, ids=lambda v: str(v))
def test_stream_output_equals_whole_signal(ctx, rate, fmt):
    """Vocoder steps of 4, 1 and 3 frames plus flush_output against ctx.resample_drift(side='sink') of the model-rate audio, with
    a drift change between steps; output_pending is the flush count."""
    T = 19
    mel = _mel(1, T, 5)
    plain = StreamingVoiceConversionEngine(ctx, 1, max_ref_frames=64)
    plain.st.reset([0])
    rows, _ = _voc_run(plain.st, [0], mel, [4, 1, 3])
    model_wav = torch.cat([r[0] for r in rows])[None]
    eng = StreamingVoiceConversionEngine(ctx, 1, max_ref_frames=64)
    st = eng.st
    st.reset([0])
    st.set_output_drift([0], 2000.0, rate=rate)
    if fmt != "f32":
        st.set_output_format([0], fmt)
    ld = 4 * HOP * rate // 16000 + 16
    st.set_output_ld(ld)
    sched, pieces, pos, k = [(0, 2000.0)], [], 0, 0
    sizes = [4, 1, 3]
    while pos < T:
        f = min(sizes[k % 3], T - pos)
        if k in (2, 4):
            new = -2000.0 if k == 2 else 300.0
            st.set_output_drift([0], new)
            sched.append((st.output_drift([0])[0][2], new))
        buf = torch.full((1, ld), SENTINEL, device="cuda")
        got = st.hifigan_step([0], mel[:, pos:pos + f], out=buf)
        cnt = st.output_samples()
        pieces.append(got[0].clone() if isinstance(got, (list, tuple)) else got[0, :cnt[0]].clone())
        assert pieces[-1].shape[0] == cnt[0]
        pos, k = pos + f, k + 1
    pend = st.output_pending([0])
    tail = st.flush_output([0])
    assert tail[0].shape[0] == pend[0] and st.output_pending([0]) == [0]
    torch.cuda.synchronize()
    want = ctx.resample_drift(model_wav, 16000, rate, sched, side="sink")
    ppm, n_in, n_out = st.output_drift([0])[0]
    assert (ppm, n_in, n_out) == (300.0, T * HOP, want.shape[1])
    ref = R.whole(model_wav.cpu().numpy(), _table(16000, rate), 16000, rate, R.SINK, [(a, _lib.drift_ppb(p)) for a, p in sched])
    assert np.array_equal(_bits(want.cpu().numpy()), _bits(ref))
    if fmt != "f32":
        want = ctx.convert_samples(want, "f32", fmt)
    out = torch.cat(pieces + [tail[0]])
    assert out.dtype == want.dtype and torch.equal(out, want[0])


# ---- a ragged call mixing a drift row with a rational-rate row, a format-only row and a plain row
def _mixed_run(ctx, with_drift):
    eng = StreamingVoiceConversionEngine(ctx, 4, max_ref_frames=64, flags=_lib.STREAMS_FIXED_PLAN)      # (one launch plan whatever the rows of a step)
    slots = [0, 1, 2, 3] if with_drift else [1, 2, 3]
    eng.open_slots(slots, _ref(4)[slots], in_rate=([None] if with_drift else []) + [48000, None, None])      # (each slot its own reference in both runs)
    eng.st.set_input_format([2], "s16")
    if with_drift:
        eng.st.set_input_drift([0], -2000.0, rate=8000)
    srcs = {0: _sig(1, 4 * 640 + 7, 8000, 31)[0], 1: _sig(1, 4 * 3840, 48000, 32)[0],
            2: ctx.convert_samples(_sig(1, 4 * L, 16000, 33), "f32", "s16")[0], 3: _sig(1, 4 * L, 16000, 34)[0]}
    step = {0: [641, 639, 1280, 7], 1: [3840] * 4, 2: [L] * 4, 3: [L] * 4}
    pos = {s: 0 for s in slots}
    outs = {s: [] for s in slots}
    names = []      # per call: the resampler launches
    for k in range(6):
        fin = k >= 4
        sm = [0 if fin else step[s][k] for s in slots]
        rows = [srcs[s][pos[s]:pos[s] + m] for s, m in zip(slots, sm)]
        res, ks = _profiled(eng.st, lambda: eng.feed_ragged(slots, rows, sm, [fin] * len(slots)))
        names.append(ks.get("resample_stream_kernel", 0))
        for s, m, (w, mel, c) in zip(slots, sm, res):
            pos[s] += m
            outs[s].append((w.clone(), mel.clone(), c.clone()))
    torch.cuda.synchronize()
    return {s: [torch.cat(t) for t in zip(*outs[s])] for s in slots}, names


def test_mixed_ragged_call(ctx):
    with_d, names_d = _mixed_run(ctx, True)
    without, names = _mixed_run(ctx, False)
    for s in (1, 2, 3):
        for k, (a, b) in enumerate(zip(with_d[s], without[s])):
            assert a.shape == b.shape and torch.equal(a, b), (s, ("wav", "mel", "codes")[k], a.shape, b.shape)
    assert with_d[0][1].shape[0] > 0
    # no new launch: the drift row rides in the one resampler launch a call with samples makes anyway; a drain call launches at
    # most once, for output some slot is still owed (a rational row's remainder, the drift slot's backlog behind its 2 * s_in call)
    assert names[:4] == names_d[:4] == [1, 1, 1, 1] and all(c in (0, 1) for c in names[4:] + names_d[4:])


def test_set_without_drift_launches_as_before(ctx):
    """A stream-set that never asks allocates nothing and launches exactly what it launched before: the kernels of a plain run
    are those of a run whose other engine has a drift slot, and the state size is the plain one."""
    a = StreamingVoiceConversionEngine(ctx, 2, max_ref_frames=64)
    b = StreamingVoiceConversionEngine(ctx, 2, max_ref_frames=64)
    bytes0 = a.st.state_bytes
    src = _sig(2, 3 * L + 11, 16000, 5)
    wa, ka = _profiled(a.st, lambda: a.infer_wav(src, _ref(2), pipelined=False))
    assert "resample_stream_kernel" not in ka and "resample_out_kernel" not in ka and a.st.state_bytes == bytes0
    wb, kb = _profiled(b.st, lambda: b.infer_wav(src, _ref(2), pipelined=False, drift=0.0, rolloff=1.0, out_filter=dict(rolloff=1.0)))
    assert kb.get("resample_stream_kernel", 0) > 0 and kb.get("resample_out_kernel", 0) > 0
    assert set(kb) - set(ka) == {"resample_stream_kernel", "resample_out_kernel"}
    # the identity case end to end: rolloff = 1, drift 0 at the model rate on both sides hands every sample through unchanged,
    # W samples later on each side - the utterance's results are the plain run's
    assert _equal(wb, wa)


# ---- refusals change nothing
def test_stream_refusals_change_nothing(ctx):
    rate, s_in = 8000, 640
    src = _sig(1, 5 * s_in + 11, rate, 41)
    sizes = [s_in, s_in + 1, s_in - 1, s_in]

    def run(hook):
        eng = _engine(ctx, 2)
        eng.slots = [0]
        eng.st.set_input_drift([0], 300.0, rate=rate)
        pos, outs = 0, []
        for k in range(8):
            hook(eng, k)
            fin = k >= len(sizes)
            m = (src.shape[1] - pos) if fin else sizes[k]
            e, c, mel, w = eng.st.step_wav([0], src[:, pos:pos + m], final=fin)
            pos += m
            if e:
                outs.append((w.clone(), mel.clone(), c[:, :e].clone()))
        torch.cuda.synchronize()
        return [torch.cat(t, 1) for t in zip(*outs)], eng.st.input_drift([0])[0]

    def hook(eng, k):
        st = eng.st
        if k != 2:
            return
        before = st.input_drift([0])[0]
        with pytest.raises(_lib.ConanError) as e:      # a live change on a slot without drift
            st.set_input_drift([0, 1], 10.0)
        assert e.value.code == _lib.ERR_STATE
        with pytest.raises(_lib.ConanError) as e:      # configure mid-utterance
            st.set_input_drift([0], 10.0, rate=rate)
        assert e.value.code == _lib.ERR_STATE
        with pytest.raises(_lib.ConanError) as e:      # 2W > 512
            st.set_input_drift([1], 10.0, rate=48000, lowpass_filter_width=128)
        assert e.value.code == _lib.ERR_INVALID
        with pytest.raises(_lib.ConanError) as e:      # an over-long call
            st.step_wav([0], _sig(1, 2 * s_in + 1, rate, 1))
        assert e.value.code == _lib.ERR_INVALID
        with pytest.raises(_lib.ConanError) as e:      # slot snapshots
            st.export_slots([0])
        assert e.value.code == _lib.ERR_UNSUPPORTED
        assert st.input_drift([0])[0] == before
        with pytest.raises(_lib.ConanError):
            st.input_drift([1])

    clean, end_clean = run(lambda eng, k: None)
    got, end = run(hook)
    assert end == end_clean and _equal(got, clean)


def test_step_wav_unequal_ppb_refused(ctx):
    eng = _engine(ctx, 2)
    eng.st.set_input_drift([0, 1], [100.0, 100.5], rate=8000)
    with pytest.raises(_lib.ConanError) as e:
        eng.st.step_wav([0, 1], _sig(2, 640, 8000, 1))
    assert e.value.code == _lib.ERR_INVALID
    assert [d[1:] for d in eng.st.input_drift([0, 1])] == [(0, 0), (0, 0)]
    eng.st.set_input_drift([1], 100.0)
    e, *_ = eng.st.step_wav([0, 1], _sig(2, 640, 8000, 1))
    assert [d[1] for d in eng.st.input_drift([0, 1])] == [640, 640]


def test_reset_keeps_drift_and_restarts_position(ctx):
    eng = _engine(ctx)
    eng.st.set_input_drift([0], 2000.0, rate=8000)
    x = _sig(1, 640, 8000, 3)
    eng.st.step_wav([0], x)
    first = eng.st.input_drift([0])[0]
    eng.st.reset([0], which=7 | 8)
    assert eng.st.input_drift([0])[0] == (2000.0, 0, 0)
    eng.st.step_wav([0], x)
    assert eng.st.input_drift([0])[0] == first
    eng.st.reset([0], which=7 | 8)
    eng.st.set_input_rate([0], 8000)               # a rate setter at an utterance start removes the drift resampler
    with pytest.raises(_lib.ConanError):
        eng.st.input_drift([0])
