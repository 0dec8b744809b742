"""Signalling tones on the GPU (conan_tones, conan_tone_fill, conan_tone_table, conan_streams_set_tones, conan_step_wav_tones;
include/conan_hip.h, conan_tone_cfg): the whole-signal forms against tests/tone_ref.py, the streaming form against the library's own
whole-signal form, and the feature against itself - neighbours keep their bits and launches, the placement behind every other in-place
stage, the setter, restarts, the hand-over, refused calls - and the promise to the user: the regenerated tones are detectable behind
8 kHz mu-law.  Every comparison but the last is bit for bit: the law is integer sums and single correctly rounded IEEE operations."""
import ctypes as C

import numpy as np
import pytest
import torch

from conan_amd import _lib
from conan_amd.engine import StreamingVoiceConversionEngine
from conan_amd.runtime import Context, _ptr, _stream
from tests import activity_ref as A
from tests import pitch_ref as P
from tests import tone_ref as R
from tests.test_gpu_f0 import _launches, _open, _ragged, _ref, _run
from tests.test_gpu_pitch import full  # noqa: F401  (module fixture: the small synthetic full model)
from tests.test_tone_cpu import BAD, put

pytestmark = pytest.mark.gpu

HOP, SEG = 320, 4
L = SEG * HOP
MAX_SLOTS = 6
SLOTS = [1, 4]
FULL = R.FULL
W = R.table(50 * HOP)
KW = dict(hold_frames=1, attack_frames=2, release_frames=3)      # the activity tests' detector


def _u32(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.uint32)


def _speech(N, seed):
    return A.burst_signal(noise=1e-3, seed=seed)[3000:3000 + N].astype(np.float64)


def _keyed(N, seed, keys, db=-12.0, on=5, off=4, first=3):
    """Speech-like audio of N samples with the keys' tone pairs in it: `on` frames each, `off` frames apart, from frame `first` on,
    not aligned with the frames."""
    x = _speech(N, seed)
    pos = first * HOP + 37 * (seed % 7)
    for k in keys:
        if pos + on * HOP > N:      # (a key that does not fit is left out)
            break
        x[pos:pos + on * HOP] = R.pair(k, on * HOP, (db, db - 2.0), start=pos)
        pos += (on + off) * HOP
    return x.astype(np.float32)


def _padded(x):
    """x [n, N] -> [n, (1 + N // hop) * hop]: the source as the detector sees it, zeros beyond the samples received."""
    n, N = x.shape
    out = torch.zeros(n, (1 + N // HOP) * HOP, dtype=x.dtype, device=x.device)
    out[:, :N] = x
    return out


def _ref_rows(x, c=None, state=None):
    return R.detect(x, R.cfg(HOP) if c is None else c, HOP, state=state, W=W)


def _state_dict(s):
    return {k: int(v) for k, v in s.items()}


# ------------------------------------------------------------------------------------------------------------------ 1. table, detector

def test_table_equals_numpy(full):
    assert np.array_equal(full.tone_table(), W) and full.tone_table().dtype == np.int16
    assert np.array_equal(full.tone_table(8000), R.table(8000))
    for rate in (16001, 50 * 514, 50 * 3, 0):      # not 50 * hop; hop beyond 512; a rate that is no multiple of 4; nothing
        with pytest.raises(_lib.ConanError) as e:
            full.tone_table(rate)
        assert e.value.code == _lib.ERR_UNSUPPORTED, rate


def _tones_raw(full, x, lens, c, out_ld, seed=None):
    """conan_tones with an output stride of the caller's choosing and sentinels in the outputs."""
    n = x.shape[0]
    outs = [torch.full((n, out_ld), 77, dtype=torch.int32, device="cuda") for _ in range(3)]
    st = torch.zeros(n, 48, dtype=torch.uint8, device="cuda")
    sm = np.ascontiguousarray(np.asarray(lens, dtype=np.int64))
    frames = np.zeros(n, dtype=np.int64)
    _lib.check(full.lib.conan_tones(full.h, HOP, C.byref(c), _ptr(x), x.stride(0), n, sm.ctypes.data_as(C.c_void_p), _ptr(seed), _ptr(outs[0]), _ptr(outs[1]),
                                    _ptr(outs[2]), out_ld, _ptr(st), frames.ctypes.data_as(C.c_void_p), _stream()))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], st, frames


@pytest.mark.parametrize("N", [320, 321, 1280, 1281, 5 * 1280 + 37])
def test_whole_signal_detector_against_the_law(full, N):
    keys = "5" if N < 2000 else "5#"
    x = np.stack([_keyed(5 * 1280 + 37, 3 + i, keys, first=0 if N < 2000 else 2, on=4, off=3)[:N] for i in range(3)])
    x[2] *= 3.0      # (clipping: the s16 clamp)
    xd = torch.from_numpy(x).cuda()
    c = _lib.tone_cfg(ramp_ms=60.0)
    rc = R.cfg(HOP, step=c.step)
    dg, sd, lv, (states, rows) = full.tones(xd, cfg=c, return_state=True)
    F = -(-N // HOP)
    assert dg.shape == (3, F)
    for i in range(3):
        rd, rs, rl, rst = _ref_rows(x[i], rc)
        assert np.array_equal(dg[i].cpu().numpy(), rd) and np.array_equal(sd[i].cpu().numpy(), rs) and np.array_equal(lv[i].cpu().numpy(), rl), (N, i)
        assert states[i] == rst, (N, i)
        assert bytes(rows[i].cpu().numpy()) == bytes(_lib.tone_cfg(seed=rst).seed)      # the state's bytes, reserved word included
    if N >= 1280:
        assert any(len(R.events(dg[i].cpu().numpy())) for i in range(3))      # (the rows do hold digits)


def test_rows_of_different_lengths_and_seeds_in_one_call(full):
    lens = [5 * 1280 + 37, 640, 0, 321]
    x = np.stack([_keyed(5 * 1280 + 37, 11 + i, "9D", first=1) for i in range(4)])
    xw = torch.zeros(4, x.shape[1] + 5, device="cuda")      # (a row stride wider than the samples)
    xv = xw[:, :x.shape[1]]
    xv.copy_(torch.from_numpy(x))
    c = _lib.tone_cfg()
    seeds = [R.seed(), dict(R.seed(), cand=14, run=1, frames=3), R.seed(), dict(R.seed(), cur=8, sound=8, level=FULL, held=1, frames=4, events=1)]
    sd_rows = torch.from_numpy(np.frombuffer(b"".join(bytes(_lib.tone_cfg(seed=s).seed) for s in seeds), dtype=np.uint8).reshape(4, 48).copy()).cuda()
    F = -(-lens[0] // HOP)
    outs, st, frames = _tones_raw(full, xv, lens, c, F + 3, seed=sd_rows)
    assert list(frames) == [-(-n // HOP) for n in lens]
    for i, n in enumerate(lens):
        f = int(frames[i])
        want = _ref_rows(x[i, :n], state=seeds[i])
        for k in range(3):
            assert np.array_equal(outs[k][i, :f], want[k]), (i, k)
            assert (outs[k][i, f:] == 77).all(), (i, k)      # nothing behind a row's frames
        assert bytes(st[i].cpu().numpy()) == bytes(_lib.tone_cfg(seed=want[3]).seed), i


def test_any_cut_through_the_state_equals_the_whole_signal(full):
    x = np.stack([_keyed(20 * HOP, 5 + i, "27", first=1 + i, on=5 + i, off=2) for i in range(2)])
    xd = torch.from_numpy(x).cuda()
    c = _lib.tone_cfg(ramp_ms=80.0)
    whole = full.tones(xd, cfg=c, return_state=True)
    assert all(len(R.events(whole[0][i].cpu().numpy())) == 2 for i in range(2))
    for cuts in ((4, 1, 7, 8), (1,) * 20, (19, 1)):
        seed, parts, pos = None, [], 0
        for n in cuts:
            dg, sd, lv, (_, seed) = full.tones(xd[:, pos * HOP:(pos + n) * HOP].contiguous(), cfg=c, seed=seed, return_state=True)
            parts.append((dg, sd, lv))
            pos += n
        for k in range(3):
            assert torch.equal(torch.cat([p[k] for p in parts], 1), whole[k]), (cuts, k)
        assert torch.equal(seed, whole[3][1]), cuts


# ------------------------------------------------------------------------------------------------------------------ 2. the fill

@pytest.mark.parametrize("N", [1, 319, 321, 7 * 320 + 5])
def test_fill_against_the_law(full, N):
    rng = np.random.default_rng(N)
    F = -(-N // HOP)
    base_s = np.array([-1, 5, 5, -1, -1, 9, 14, 14], dtype=np.int32)
    base_l = np.array([0, FULL // 3, FULL, FULL // 2, 0, FULL, FULL, 1], dtype=np.int32)
    sound = np.stack([np.resize(base_s, F), np.full(F, -1, np.int32), np.resize(np.roll(base_s, 3), F)])
    level = np.stack([np.resize(base_l, F), np.zeros(F, np.int32), np.resize(np.roll(base_l, 3), F)])
    y = rng.standard_normal((3, N)).astype(np.float32)
    pos0 = [0, 5 * HOP, 123456789 * HOP]
    starts = [(0, -1), (FULL, 3), (FULL // 7, 12)]
    yd, sdv, lvd = torch.from_numpy(y).cuda(), torch.from_numpy(sound).cuda(), torch.from_numpy(level).cuda()
    for sl, ss in starts:
        want = np.stack([R.fill(y[i], sound[i], level[i], 0.125, HOP, pos0[i], sl, ss, W) for i in range(3)])
        got = full.tone_fill(yd, sdv, lvd, start=(sl, ss), pos0=pos0)
        assert np.array_equal(_u32(got), _u32(want)), (N, sl, ss)
        if (sl, ss) == (0, -1):
            assert np.array_equal(_u32(got[1]), _u32(y[1]))      # a row without a sound keeps its bits
        z = yd.clone()
        assert full.tone_fill(z, sdv, lvd, start=(sl, ss), pos0=pos0, out=z) is z      # in place
        assert np.array_equal(_u32(z), _u32(want))
        # rows at unaligned addresses and an odd stride: the single-word path
        yw, ow = torch.zeros(3, N + 5, device="cuda"), torch.zeros(3, N + 6, device="cuda")
        yv, ov = yw[:, 1:N + 1], ow[:, 2:N + 2]
        yv.copy_(yd)
        lw = torch.zeros(3, F + 3, dtype=torch.int32, device="cuda")
        sv, lv = lw.clone()[:, :F], lw[:, :F]
        sv.copy_(sdv); lv.copy_(lvd)
        assert full.tone_fill(yv, sv, lv, start=(sl, ss), pos0=pos0, out=ov) is ov
        assert np.array_equal(_u32(ov.contiguous()), _u32(want)), (N, "views")
        assert not ow[:, :2].any() and not ow[:, N + 2:].any()      # nothing outside the rows was written
        assert full.tone_fill(yv, sv, lv, start=(sl, ss), pos0=pos0, out=yv) is yv
        assert np.array_equal(_u32(yv.contiguous()), _u32(want))
    other = full.tone_fill(yd, sdv, lvd, start=(FULL, 3), pos0=pos0, gain=0.25)
    assert not torch.equal(other[0], got[0])


# ------------------------------------------------------------------------------------------------------------------ 3. streaming

def _run_tones(st, slots, wav, pipelined=False, on_call=None, first_call=0, rows=True):
    """infer_wav's calls from call `first_call` on -> (codes, mel, wav, digit, sound, level) over the emitted chunks (the tone rows
    per emitting call where rows=True: the hook joins, so a pipelined run that is to stay pipelined passes rows=False)."""
    n, N = wav.shape
    last = (N - 1) // L * L
    calls = ([(p, p + L, False) for p in range(0, last, L)] + [(last, N, True)])[first_call:]
    step = st.step_wav_async if pipelined else st.step_wav
    outs, k = [], first_call
    while True:
        if on_call:
            on_call(k)
        if calls:
            a, b, fin = calls.pop(0)
            e, c, m, w = step(slots, wav[:, a:b], final=fin)
        else:
            e, c, m, w = step(slots, wav[:, :0], final=True)
            if e == 0:
                break
        k += 1
        if e:
            row = [c[:, :e], m, w]
            if rows:
                dg, sd, lv = st.step_wav_tones()
                assert not dg[:, e:].any() and not sd[:, e:].any() and not lv[:, e:].any()      # entries past the emitted frames are zero
                row += [dg[:, :e].clone(), sd[:, :e].clone(), lv[:, :e].clone()]
            outs.append(row)
    st.join()
    torch.cuda.synchronize()
    return [torch.cat([o[i] for o in outs], 1).clone() for i in range(len(outs[0]))]


def _four(N=9 * L + 10):
    """Four rows of speech-like audio; rows 1 and 3 (slots 1 and 4 of [0, 1, 2, 4]) carry different digit strings."""
    return torch.from_numpy(np.stack([_speech(N, 40).astype(np.float32), _keyed(N, 41, "159"), _speech(N, 42).astype(np.float32), _keyed(N, 43, "#0", on=7, first=5)])).cuda()


def _expect(full, w_off, x, c):
    """The library's own whole-signal form: the rows of x's padded form, and w_off through conan_tone_fill."""
    dg, sd, lv = full.tones(_padded(x), cfg=c)
    return dg, sd, lv, full.tone_fill(w_off, sd, lv, cfg=c)


def test_streaming_equals_the_whole_signal_form(full):
    slots = [0, 1, 2, 4]
    wav = _four()
    c = _lib.tone_cfg(ramp_ms=60.0)
    plain = _open(full, slots)
    c0, m0, w0 = _run_tones(plain, slots, wav, rows=False)
    plain.close()
    dg, sd, lv, want = _expect(full, w0[[1, 3]], wav[[1, 3]], c)
    ev = _lib.tone_events(dg.cpu().numpy())
    assert ["".join(k for k, _, _ in e) for e in ev] == ["159", "#0"]
    assert not torch.equal(want, w0[[1, 3]])
    st = _open(full, slots)
    st.set_tones(SLOTS, cfg=c)
    for pipelined, rows in ((False, True), (True, True), (True, False)):
        out = _run_tones(st, slots, wav, pipelined=pipelined, rows=rows)
        assert torch.equal(out[0], c0) and torch.equal(out[1], m0), (pipelined, rows)      # the feature touches no model input
        assert np.array_equal(_u32(out[2][[0, 2]]), _u32(w0[[0, 2]])), (pipelined, rows)      # the other slots keep their bits
        assert np.array_equal(_u32(out[2][[1, 3]]), _u32(want)), (pipelined, rows)
        if rows:
            for got, exp in zip(out[3:], (dg, sd, lv)):
                assert torch.equal(got[[1, 3]], exp) and not got[[0, 2]].any(), (pipelined,)
        assert [s["events"] for s in st.tone_state(SLOTS)] == [3, 2]
        st.reset(slots, which=15)
        st.set_reference(slots, _ref(4))
    st.close()


def _ragged_rows(st, slots, wavs, starts):
    """test_gpu_f0's _ragged (blocking, no contour) with the tone rows read behind every call -> its result, and per utterance
    (digit, sound, level) over its emitted frames, the calls' rows joined."""
    log = []
    step = st.step_wav_ragged

    def logged(live_slots, rows, samples, final):
        out = step(live_slots, rows, samples, final)
        log.append((list(live_slots), list(out[0]), [t.clone() for t in st.step_wav_tones()]))
        return out

    st.step_wav_ragged = logged
    try:
        outs = _ragged(st, slots, wavs, starts, contour=False)
    finally:
        del st.step_wav_ragged      # (the instance attribute: the method is the class's again)
    rows = {s: [] for s in slots}
    for live, emit, (dg, sd, lv) in log:
        assert dg.shape == sd.shape == lv.shape == (len(live), SEG)
        for r, (s, e) in enumerate(zip(live, emit)):
            assert not dg[r, e:].any() and not sd[r, e:].any() and not lv[r, e:].any()      # entries past the emitted frames are zero
            rows[s].append((dg[r, :e], sd[r, :e], lv[r, :e]))
    return outs, [[torch.cat([c[k] for c in rows[s]]) for k in range(3)] for s in slots]


def test_ragged_calls_equal_the_whole_signal_form(full):
    slots, starts = [1, 0, 4], [0, 1, 3]
    wavs = [torch.from_numpy(_keyed(4 * L + 333, 50, "37", first=2, on=4, off=3)).cuda(), torch.from_numpy(_speech(3 * L, 51).astype(np.float32)).cuda(),
            torch.from_numpy(_keyed(3 * L + 1, 52, "C", first=1, on=6)).cuda()]
    c = _lib.tone_cfg()
    plain = _open(full, slots)
    want, lp = _launches(plain, lambda: _ragged(plain, slots, wavs, starts, contour=False))
    plain.close()
    st = _open(full, slots)
    st.set_tones([1, 4], cfg=c)
    (got, rows), lg = _launches(st, lambda: _ragged_rows(st, slots, wavs, starts))
    assert all(torch.equal(got[1][i], want[1][i]) for i in range(3))
    assert not any(r.any() for r in rows[1])      # the slot without the feature reads zeros
    for u in (0, 2):
        assert torch.equal(got[u][0], want[u][0]) and torch.equal(got[u][1], want[u][1])
        dg, sd, lv, w = _expect(full, want[u][2][None], wavs[u][None], c)
        assert len(_lib.tone_events(dg[0].cpu().numpy())) == (2 if u == 0 else 1)
        for k, exp in enumerate((dg, sd, lv)):      # the calls' rows, joined: conan_tones of the slot's whole input
            assert torch.equal(rows[u][k], exp[0]), (u, k)
        assert np.array_equal(_u32(got[u][2]), _u32(w[0])), u
    assert lg.pop("tone_kernel") >= 1 and lg.pop("tone_fill_kernel") >= 1 and lg == lp, (lg, lp)
    st.close()


@pytest.mark.parametrize("pipelined", [False, True])
def test_mu_law_at_8_khz_in_and_out(full, pipelined):
    n, N8 = 2, (7 * L + 200) // 2
    x16 = np.stack([_keyed(2 * N8, 60, "48", db=-9.0), _keyed(2 * N8, 61, "*", db=-9.0, on=8)])
    src = full.convert_samples(full.resample(torch.from_numpy(x16).cuda(), 16000, 8000), "f32", "ulaw")
    N8 = src.shape[1]
    prepared = full.resample(full.convert_samples(src, "ulaw", "f32"), 8000, 16000)
    eng = StreamingVoiceConversionEngine(full, n, max_ref_frames=64)
    w_off, m_off, _ = eng.infer_wav(src, _ref(n), pipelined=pipelined, in_rate=8000, in_format="ulaw")
    c = _lib.tone_cfg()
    dg, sd, lv, filled = _expect(full, w_off, prepared, c)
    assert ["".join(k for k, _, _ in e) for e in _lib.tone_events(dg.cpu().numpy())] == ["48", "*"]
    want = full.convert_samples(full.resample(filled, 16000, 8000), "f32", "ulaw")      # (the steps plus the flush)
    w_on, m_on, _ = eng.infer_wav(src, _ref(n), pipelined=pipelined, in_rate=8000, in_format="ulaw", out_rate=8000, out_format="ulaw", tones=True)
    torch.cuda.synchronize()
    assert torch.equal(m_on, m_off) and w_on.dtype == torch.uint8 and w_on.shape == want.shape
    assert torch.equal(w_on, want)
    plain = eng.infer_wav(src, _ref(n), pipelined=pipelined, in_rate=8000, in_format="ulaw", out_rate=8000, out_format="ulaw", tones=None)[0]
    assert not torch.equal(plain, w_on)
    # the same utterance call by call (infer_wav's calls) with chunk_tones behind each: the rows are conan_tones of the decoded,
    # resampled input, and reading them between pipelined calls changes no audio
    eng.start_wav(_ref(n), in_rate=8000, out_rate=8000, in_format="ulaw", out_format="ulaw", tones=True)
    L8 = eng._in_len(8000)
    calls = [src[:, p:p + L8] for p in range(0, (N8 - 1) // L8 * L8, L8)] + [src[:, (N8 - 1) // L8 * L8:]]
    rows, wavs = [], []
    while True:
        drain = not calls
        piece = src[:, :0] if drain else calls.pop(0)
        w, m, _ = eng.feed(piece, final=not calls, pipelined=pipelined)
        e = m.shape[1]
        if drain and e == 0:
            break
        if e:
            got = eng.chunk_tones()
            assert all(not r[:, e:].any() for r in got)
            rows.append([r[:, :e].clone() for r in got])
            wavs.append(w.clone())
    for k, exp in enumerate((dg, sd, lv)):
        assert torch.equal(torch.cat([r[k] for r in rows], 1), exp), k
    assert torch.equal(torch.cat(wavs + [torch.stack(eng.finish())], 1), want)
    eng.st.close()


def test_engine_entry_points(full):
    """The engine's surface beyond infer_wav(tones=True): tones= with one value per utterance on infer_wav_staggered (which hands them
    to open_slots slot by slot), tones= with one value per slot on open_slots, engine.set_tones between calls, engine.chunk_tones."""
    wavs = [torch.from_numpy(_keyed(3 * L + 50, 95, "2", first=2, on=5)).cuda(), torch.from_numpy(_keyed(2 * L + 9, 96, "8", first=1)).cuda(),
            torch.from_numpy(_keyed(3 * L, 97, "D", first=2, on=6)).cuda()]
    starts, ref = [0, 1, 1], _ref(3)
    eng = StreamingVoiceConversionEngine(full, 3, max_ref_frames=64)
    plain = eng.infer_wav_staggered(wavs, starts, ref)
    assert eng.st.tones(eng.slots) == [None] * 3
    got = eng.infer_wav_staggered(wavs, starts, ref, tones=[dict(ramp_ms=60.0), None, dict(regenerate=False)])
    torch.cuda.synchronize()
    kw = eng.st.tones(eng.staggered_slots)
    assert kw[0]["regenerate"] is True and kw[1] is None and kw[2]["regenerate"] is False
    for u in range(3):
        assert torch.equal(got[u][1], plain[u][1]) and torch.equal(got[u][2], plain[u][2]), u
    dg, _, _, want = _expect(full, plain[0][0][None], wavs[0][None], _lib.tone_cfg(ramp_ms=60.0))
    assert _lib.tone_events(dg[0].cpu()) == _lib.tone_events(dg.cpu().numpy())[0] and [k for k, _, _ in _lib.tone_events(dg[0].cpu())] == ["2"]
    assert np.array_equal(_u32(got[0][0]), _u32(want[0])) and not torch.equal(got[0][0], plain[0][0])
    for u in (1, 2):      # no feature, and a detector alone: the audio keeps its bits
        assert np.array_equal(_u32(got[u][0]), _u32(plain[u][0])), u
    # open_slots with one value per slot, a live engine.set_tones before the call that emits the first chunk, chunk_tones per call
    slots = [0, 2]
    x = torch.stack([wavs[0][:3 * L], wavs[2][:3 * L]])
    eng.open_slots(slots, _ref(2), tones=[None, True])
    now = eng.st.tones(slots)
    assert now[0] is None and now[1]["regenerate"] is True
    rows = []
    for k in range(3):
        if k == 1:
            eng.set_tones([0], regenerate=False)
        res = eng.feed_ragged(slots, x[:, k * L:(k + 1) * L], [L, L], [0, 0])
        e = res[0][1].shape[0]
        assert e == res[1][1].shape[0] == (SEG if k else 0)
        if e:
            rows.append([r[:, :e].clone() for r in eng.chunk_tones()])
    exp = full.tones(x[:, :2 * L].contiguous())
    for k in range(3):
        assert torch.equal(torch.cat([r[k] for r in rows], 1), exp[k]), k
    assert [[key for key, _, _ in ev] for ev in _lib.tone_events(exp[0].cpu())] == [["2"], ["D"]]
    assert eng.st.tones(slots)[0]["regenerate"] is False
    eng.st.close()


# ------------------------------------------------------------------------------------------------------------------ 4. neighbours

def test_neighbours_keep_their_bits_and_launches(full):
    slots = [0, 1, 2, 4]
    wav = _four(3 * L + 77)
    a, b, d = _open(full, slots), _open(full, slots), _open(full, slots)
    bytes_never = b.state_bytes
    a.set_tones([1], regenerate=False)
    a.set_tones([4])
    d.set_tones([1], regenerate=False)
    state = MAX_SLOTS * C.sizeof(_lib.ToneState) + 8 * MAX_SLOTS * (3 * SEG + 2) * 4 + 8 * MAX_SLOTS * 168
    assert a.state_bytes == bytes_never + state      # the state, the staging sets and the row tables, from the first enabling call on
    b.set_tones(slots, None)                         # turning off what was never on allocates nothing
    assert b.state_bytes == bytes_never and b.tones(slots) == [None] * 4
    ((ca, ma, wa, _, _), emits), la = _launches(a, lambda: _run(a, slots, wav, contour=False))
    ((cb, mb, wb, _, _), _), lb = _launches(b, lambda: _run(b, slots, wav, contour=False))
    ((_, _, wd, _, _), _), ld = _launches(d, lambda: _run(d, slots, wav, contour=False))
    assert torch.equal(ca, cb) and torch.equal(ma, mb)
    for i in (0, 1, 2):
        assert np.array_equal(_u32(wa[i]), _u32(wb[i])), i      # rows without the feature and the mode-1 row keep their bits
    assert not torch.equal(wa[3], wb[3]) and np.array_equal(_u32(wd), _u32(wb))
    # a stream-set that never enabled it runs the launches it ran before; a mode-1 slot adds the detector launch per emitting call and
    # no fill; a mode-2 slot adds one of each
    assert "tone_kernel" not in lb and "tone_fill_kernel" not in lb
    assert ld.pop("tone_kernel") == len(emits) and ld == lb, (ld, lb)
    assert la.pop("tone_kernel") == len(emits) and la.pop("tone_fill_kernel") == len(emits) and la == lb, (la, lb)
    a.set_tones(slots, None)
    assert a.tones(slots) == [None] * 4
    a.reset(slots, which=15)
    a.set_reference(slots, _ref(4))
    ((_, m2, w2, _, _), _), l2 = _launches(a, lambda: _run(a, slots, wav, contour=False))
    assert l2 == lb and torch.equal(m2, mb) and torch.equal(w2, wb)
    a.close(); b.close(); d.close()


# ------------------------------------------------------------------------------------------------------------------ 5. placement

def test_placement_behind_every_other_in_place_stage(full):
    slots = SLOTS
    wav = _four()[[1, 3]]
    c = _lib.tone_cfg(ramp_ms=40.0)

    def run(tones):
        st = _open(full, slots)
        st.set_activity(slots, **KW)
        st.set_bypass(slots, wet=0.8, dry=0.2, fill_gate=True)
        st.set_comfort(slots)
        st.set_output_level(slots)
        st.set_watermark(slots, key=99, id=7)
        if tones:
            st.set_tones(slots, cfg=c)
        out = _run_tones(st, slots, wav, rows=tones)
        mark = st.watermark_state(slots).cpu().numpy().copy()
        st.close()
        return out, mark

    off, mark_off = run(False)
    on, mark_on = run(True)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    dg, sd, lv, want = _expect(full, off[2], wav, c)
    assert torch.equal(on[3], dg) and torch.equal(on[4], sd) and torch.equal(on[5], lv)
    assert np.array_equal(_u32(on[2]), _u32(want)) and not torch.equal(on[2], off[2])      # the order holds: the fill is the last stage
    assert np.array_equal(mark_on, mark_off)      # the mark's state advanced as it did before


# ------------------------------------------------------------------------------------------------------------------ 6. setter, hand-over, errors

def test_setter_between_pipelined_steps_and_restarts(full):
    slots = SLOTS
    wav = _four()[[1, 3]]
    c = _lib.tone_cfg()
    plain = _open(full, slots)
    _, _, w0 = _run_tones(plain, slots, wav, rows=False)
    plain.close()
    st = _open(full, slots)
    k_on = 3      # the setter joins the pipelined calls before it and is in force from chunk k_on - 1 on: frames (k_on - 1) * SEG ...

    def on_call(k):
        if k == k_on:
            st.set_tones(slots, cfg=c)

    _, _, w1, dg1, sd1, lv1 = _run_tones(st, slots, wav, pipelined=True, on_call=on_call)
    f0 = (k_on - 1) * SEG
    x_pad = _padded(wav)
    seed = torch.from_numpy(np.frombuffer(bytes(_lib.tone_cfg(seed=dict(R.seed(), frames=f0)).seed) * 2, dtype=np.uint8).reshape(2, 48).copy()).cuda()
    dg, sd, lv = full.tones(x_pad[:, f0 * HOP:].contiguous(), cfg=c, seed=seed)      # (a stream's j is the utterance's: the row starts at frame f0)
    tail = full.tone_fill(w0[:, f0 * HOP:].contiguous(), sd, lv, cfg=c, pos0=f0 * HOP)
    assert not dg1[:, :f0].any() and torch.equal(dg1[:, f0:], dg) and torch.equal(sd1[:, f0:], sd) and torch.equal(lv1[:, f0:], lv)
    assert np.array_equal(_u32(w1[:, :f0 * HOP]), _u32(w0[:, :f0 * HOP]))
    diff = (w1[:, f0 * HOP:] != tail).nonzero()
    assert diff.numel() == 0, (diff[0].tolist(), diff.shape[0])
    assert len(_lib.tone_events(dg[0].cpu().numpy())) >= 2
    # a reset with the front-end restarts from the seed; one without keeps the state; the setting survives both
    after = st.tone_state(slots)
    assert after[0]["events"] >= 2
    st.reset(slots, which=7)
    assert st.tone_state(slots) == after
    st.reset(slots, which=15)
    st.set_reference(slots, _ref(2))
    assert st.tone_state(slots) == [R.seed()] * 2 and st.tones(slots) == [_lib.tone_keywords(c)] * 2
    out = _run_tones(st, slots, wav)
    dgw, sdw, lvw, want = _expect(full, w0, wav, c)
    assert torch.equal(out[3], dgw) and np.array_equal(_u32(out[2]), _u32(want))
    # reseed = 0 on an enabled slot keeps the state, reseed = 1 restarts, and so does enabling a slot that was off
    done = st.tone_state(slots)
    st.set_tones([1], regenerate=False)
    assert st.tone_state([1]) == [done[0]] and st.tones([1])[0]["regenerate"] is False
    st.set_tones([1], reseed=True)
    assert st.tone_state(slots) == [R.seed(), done[1]]
    st.set_tones([4], None)
    st.set_tones([4])
    assert st.tone_state(slots) == [R.seed()] * 2
    st.close()


def test_hand_over_continues_bit_for_bit_mid_digit(full):
    slots, dst = SLOTS, [3, 0]
    wav = torch.from_numpy(np.stack([_keyed(7 * L + 123, 70, "6", first=9, on=9), _keyed(7 * L + 123, 71, "B", first=8, on=10)])).cuda()
    c = _lib.tone_cfg(ramp_ms=200.0)      # ten frames: the cut falls inside the ramp and inside the digit
    kw = {k: v for k, v in _lib.tone_keywords(c).items() if k != "seed"}
    a = _open(full, slots)
    a.set_tones(slots, cfg=c)
    whole = _run_tones(a, slots, wav)
    a.reset(slots, which=15)
    a.set_reference(slots, _ref(2))
    cut = 4      # calls before the export: chunks 0 .. 2 are out
    b = full.streams(MAX_SLOTS, 4, 64)
    lid, nbytes = b.layout_id, b.snapshot_bytes
    assert (a.layout_id, a.snapshot_bytes) == (lid, nbytes)      # the feature changes neither
    for k in range(cut):
        a.step_wav(slots, wav[:, k * L:(k + 1) * L])
    states = a.tone_state(slots)
    assert all(s["cur"] >= 0 and 0 < s["level"] < FULL for s in states), states      # mid-digit, mid-ramp
    snap = a.export_slots(slots)
    b.import_slots(dst, snap)
    assert b.tones(dst) == [None, None]      # a snapshot carries neither the setting nor the state
    for d, s in zip(dst, states):
        b.set_tones([d], seed=s, reseed=True, **kw)
    assert (b.layout_id, b.snapshot_bytes) == (lid, nbytes)
    rest = _run_tones(b, dst, wav, first_call=cut)
    done = (cut - 1) * SEG
    assert torch.equal(rest[0], whole[0][:, done:]) and torch.equal(rest[1], whole[1][:, done:])
    assert np.array_equal(_u32(rest[2]), _u32(whole[2][:, done * HOP:]))
    for k in (3, 4, 5):
        assert torch.equal(rest[k], whole[k][:, done:]), k
    a.close(); b.close()


def test_refused_calls_change_nothing(full):
    slots = [0, 2]
    st = _open(full, slots)
    with pytest.raises(_lib.ConanError) as e:      # the state query on a stream-set that never enabled the feature
        st.tone_state([0])
    assert e.value.code == _lib.ERR_STATE
    st.set_tones([0], ramp_ms=100.0)
    before = st.tones(range(MAX_SLOTS))
    assert before[0] is not None and before[1:] == [None] * (MAX_SLOTS - 1)
    x = torch.zeros(1, 700, device="cuda")
    for field, value in BAD:
        c = _lib.tone_cfg()
        put(c, field, value)
        with pytest.raises(_lib.ConanError) as e:
            st.set_tones([0, 2, 3], cfg=c)
        assert e.value.code == _lib.ERR_INVALID, (field, value)
        with pytest.raises(_lib.ConanError) as e:
            full.tones(x, cfg=c)
        assert e.value.code == _lib.ERR_INVALID, (field, value)
    off = _lib.tone_cfg()
    off.mode = 0      # (the setter's "off" is no setting of a whole-signal call)
    with pytest.raises(_lib.ConanError) as e:
        full.tones(x, cfg=off)
    assert e.value.code == _lib.ERR_INVALID
    for bad_slots in ([2, 2], [1, MAX_SLOTS], [-1]):
        with pytest.raises(_lib.ConanError) as e:
            st.set_tones(bad_slots)
        assert e.value.code == _lib.ERR_INVALID
    assert st.tones(range(MAX_SLOTS)) == before
    with pytest.raises(_lib.ConanError) as e:      # a slot without the feature in the state query
        st.tone_state([0, 2])
    assert e.value.code == _lib.ERR_STATE
    with pytest.raises(_lib.ConanError) as e:      # no wav-in call yet
        st.step_wav_tones()
    assert e.value.code == _lib.ERR_STATE
    z = torch.zeros(1, 2, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.ConanError) as e:      # 700 samples are 3 frames
        full.tone_fill(x, z, z)
    assert e.value.code == _lib.ERR_INVALID
    for hop in (513, 3):      # beyond the table's range; a rate that is no multiple of 4
        with pytest.raises(_lib.ConanError) as e:
            full.tones(x, hop_size=hop)
        assert e.value.code == _lib.ERR_UNSUPPORTED, hop
    # The ring.  A chunk is emitted at most (seg + right context - 1) * hop + fft_size / 2 + seg * hop samples behind the samples
    # received - 3840 at fft_size 2048, the largest the front-end takes - and the ring holds 4096: the chunk's samples [pos * hop, ...)
    # are always still there, so the refusal the bypass shares (CONAN_ERR_UNSUPPORTED before anything changes) cannot be provoked
    # through the public calls (the header and DESIGN.md §4.24 say so).  What can be checked is that the largest front-end is served,
    # and served right.
    big = dict(fft_size=2048, win_length=2048)
    wav = torch.from_numpy(np.stack([_keyed(6 * L, 80, "3", first=4, on=8), _speech(6 * L, 81).astype(np.float32)])).cuda()
    rows = []
    for k in range(6):
        e_, _, _, _ = st.step_wav(slots, wav[:, k * L:(k + 1) * L], mel=big)
        if e_:
            rows.append(st.step_wav_tones()[0][:1, :e_].clone())
    got = torch.cat(rows, 1)
    dg, _, _ = full.tones(wav[:1], ramp_ms=100.0)
    assert got.shape[1] >= 2 * SEG and torch.equal(got, dg[:, :got.shape[1]]) and len(_lib.tone_events(got[0].cpu().numpy())) == 1
    st.close()
    # a stream-set without the streaming front-end
    hp, sd_np, _ = P.model()
    ctx = Context(hp, None, 0, emformer=False, conan=True, hifigan=False)
    ctx.load_state_dict("conan", sd_np)
    ctx.finalize()
    dec = ctx.streams(2, 4, 64)
    with pytest.raises(_lib.ConanError) as e:
        dec.set_tones([0])
    assert e.value.code == _lib.ERR_STATE
    dec.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ 7. end to end

def test_regenerated_tones_are_detectable_behind_the_codec(full):
    """The user-visible promise, against the law's thresholds and not bit for bit: the emitted 8 kHz mu-law audio of a digit string,
    decoded and resampled by the library, reports the same keys."""
    keys = "1590#"
    N = (3 + 10 * len(keys) + 4) * HOP + 100
    x16 = _keyed(N, 90, keys, db=-15.0, on=6, off=4)[None]
    eng = StreamingVoiceConversionEngine(full, 1, max_ref_frames=64)
    w, _, _ = eng.infer_wav(torch.from_numpy(x16).cuda(), _ref(1), out_rate=8000, out_format="ulaw", tones=True)
    torch.cuda.synchronize()
    eng.st.close()
    back = full.resample(full.convert_samples(w, "ulaw", "f32"), 8000, 16000)
    dg, _, _ = full.tones(back)
    src, _, _ = full.tones(torch.from_numpy(x16).cuda())
    ev_out, ev_src = _lib.tone_events(dg[0].cpu().numpy()), _lib.tone_events(src[0].cpu().numpy())
    assert "".join(k for k, _, _ in ev_src) == keys
    assert "".join(k for k, _, _ in ev_out) == keys, (ev_out, ev_src)
