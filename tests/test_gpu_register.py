"""Register matching on the GPU (conan_f0_register, conan_streams_set_pitch_register, conan_streams_pitch_register[_state];
include/conan_hip.h, conan_register_cfg): the kernel against tests/register_ref.py, the streamed contour against the whole-signal one,
the matched chunk steps against the hand-composed path, and against themselves - neighbours keep their bits and launches, pipelined
equals blocking, live changes, the hand-over, the voice bank, errors.

Every comparison of contours and states is bit for bit: the law's sums are exact integers and each of its other steps is one correctly
rounded IEEE operation (include/conan_hip.h), so no tolerance is involved.  The one bound in this file is on the decoder's
f0_denorm_pred tap (test_the_decoder_hears_the_shift), which passes the contour through exp2f; it is worked out there."""
import ctypes as C

import numpy as np
import pytest
import torch

from conan_amd import _lib
from conan_amd.engine import StreamingVoiceConversionEngine
from conan_amd.runtime import Context, VoiceBank
from tests import f0_ref as R
from tests import pitch_ref as P
from tests import register_ref as G
from tests.test_gpu_f0 import HOP, L, MAX_SLOTS, SEG, _launches, _open, _ragged, _ref, _run, _run_from
from tests.test_gpu_pitch import full  # noqa: F401  (module fixture: the small synthetic full model)

pytestmark = pytest.mark.gpu

ROW_LENGTHS = [0, 1, 3, 63, 64, 65, 255, 256, 257, 1000]      # the wave and tile edges of the scan (64 lanes, tiles of 256 frames)
STEP_LENGTHS = [3 * L, 3 * L + 1, 2 * L + 319, 2 * L + 320, 700]


def _tones(N, seed=0):
    """Two voiced sources [2, N] at 16 kHz: a glide from 110 Hz up and a steady 220 Hz tone."""
    return torch.from_numpy(np.stack([R.glide(N, seed=seed), R.harmonic(220.0, N, seed=seed + 1)])).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """Equal bit for bit (NaN payloads included)."""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _kw(cfg):
    """set_pitch_register / f0_register keywords -> register_ref.match's."""
    target = cfg["target"]
    if cfg.get("seed") is not None:
        seed = tuple(cfg["seed"])
    else:
        seed = G.prior_seed(target if cfg.get("prior") is None else cfg["prior"], cfg.get("prior_frames", 50))
    return dict(target=target, max_shift=cfg.get("max_shift", 2.0), seed=seed)


def _states(st, slots):
    return [(r["count"], r["sum"]) for r in st.pitch_register(slots)]


# ------------------------------------------------------------------------------------------------------------------ 1. the law

def _contours():
    """[10, 1000] rows of ROW_LENGTHS frames: voiced runs and unvoiced stretches; the row of 255 all unvoiced; the row of 257 voiced
    only in its last frame; NaN, infinities and out-of-range v in the rows of 65, 256 and 1000."""
    rng = np.random.default_rng(7)
    n, ld = len(ROW_LENGTHS), max(ROW_LENGTHS)
    v = np.zeros((n, ld), dtype=np.float32)
    uv = np.ones((n, ld), dtype=np.float32)
    for i, T in enumerate(ROW_LENGTHS):
        run = np.cumsum(rng.random(T) < 0.08) % 3 != 2      # runs: two voiced for one unvoiced
        x = (7.0 + 1.5 * np.sin(np.arange(T) / 17.0 + i) + 0.05 * rng.standard_normal(T)).astype(np.float32)
        v[i, :T] = np.where(run, x, 0.0)
        uv[i, :T] = np.where(run, 0.0, 1.0)
        if T == 255:
            v[i, :T], uv[i, :T] = 0.0, 1.0
        if T == 257:
            v[i, :T], uv[i, :T] = 0.0, 1.0
            v[i, T - 1], uv[i, T - 1] = 6.5, 0.0
        if T in (65, 256, 1000):
            k = rng.choice(T, size=8, replace=False)
            for j, bad in zip(k, (np.nan, np.inf, -np.inf, 64.5, -70.0, 1e30, 64.0, -64.0)):      # (the last two are counted: |v| <= 64)
                v[i, j], uv[i, j] = bad, 0.0
    return v, uv


LAW_CFGS = [dict(target=8.0, prior_frames=0), dict(target=6.25, prior=7.5, prior_frames=50), dict(target=11.5, max_shift=0.25, seed=(3, 3 * G.quantise(5.0)))]


@pytest.mark.parametrize("cfg", LAW_CFGS, ids=["zero_seed", "seeded", "clamped"])
def test_the_law_against_the_reference(full, cfg):
    v, uv = _contours()
    tv, tu = torch.from_numpy(v).cuda(), torch.from_numpy(uv).cuda()
    out, state = full.f0_register(tv, tu, lengths=ROW_LENGTHS, **cfg)
    out, state = out.cpu().numpy(), state.cpu().tolist()
    clamped = voiced_frames = 0
    for i, T in enumerate(ROW_LENGTHS):
        want, ws = G.match(v[i, :T], uv[i, :T], **_kw(cfg))
        assert np.array_equal(out[i, :T].view(np.uint32), want.view(np.uint32)), (i, T)
        assert tuple(state[i]) == ws, (i, T)
        voiced = (uv[i, :T] == 0) & np.isfinite(v[i, :T]) & (np.abs(v[i, :T]) <= 64)
        clamped += int((np.abs(want[voiced].astype(np.float64) - v[i, :T][voiced]) >= cfg.get("max_shift", 2.0) - 1e-5).sum())
        voiced_frames += int(voiced.sum())
    # the clamped cfg clamps (nearly) every counted frame, the others do not live on the clamp
    assert clamped >= 0.9 * voiced_frames if "max_shift" in cfg else clamped < 0.5 * voiced_frames, (clamped, voiced_frames)
    assert tuple(state[ROW_LENGTHS.index(255)]) == _kw(cfg)["seed"]      # no counted frame: the seed comes back
    # the measure-only form and the in-place form give the same state; in place, frames past a row's length are left alone
    none, s2 = full.f0_register(tv, tu, lengths=ROW_LENGTHS, target=None, seed=_kw(cfg)["seed"])
    assert none is None and torch.equal(s2.cpu(), torch.tensor(state))
    buf, s3 = tv.clone(), torch.empty(len(ROW_LENGTHS), 2, dtype=torch.int64, device="cuda")
    c = _lib.register_cfg(**cfg)
    lens = np.asarray(ROW_LENGTHS, dtype=np.int32)
    _lib.check(full.lib.conan_f0_register(full.h, C.byref(c), C.c_void_p(buf.data_ptr()), C.c_void_p(tu.data_ptr()), len(ROW_LENGTHS),
                                          lens.ctypes.data_as(C.c_void_p), buf.shape[1], C.c_void_p(buf.data_ptr()), C.c_void_p(s3.data_ptr()), None))
    torch.cuda.synchronize()
    assert torch.equal(s3.cpu(), torch.tensor(state))
    got = buf.cpu().numpy()
    for i, T in enumerate(ROW_LENGTHS):
        assert np.array_equal(got[i, :T].view(np.uint32), out[i, :T].view(np.uint32)) and np.array_equal(got[i, T:].view(np.uint32), v[i, T:].view(np.uint32)), i
    # a row does not depend on what it shares a launch with
    solo, s4 = full.f0_register(tv[9:10], tu[9:10], **cfg)
    assert _same(solo[0], torch.from_numpy(out[9]).cuda()) and s4.cpu().tolist()[0] == state[9]


# ------------------------------------------------------------------------------------------------------------------ 2. streaming = whole signal

REG2 = [dict(target=8.5), dict(target=6.0, prior=7.0, prior_frames=20, max_shift=0.75)]


@pytest.mark.parametrize("N", STEP_LENGTHS)
def test_streamed_contour_equals_conan_f0_register(full, N):
    wav = _tones(N)
    eng = StreamingVoiceConversionEngine(full, 2, max_ref_frames=64)
    w, m, c = eng.infer_wav(wav, _ref(2), pipelined=False, follow=True, register=REG2)
    torch.cuda.synchronize()
    whole = [full.f0_register(*full.f0(wav[i:i + 1]), **REG2[i]) for i in range(2)]
    assert _states(eng.st, eng.slots) == [tuple(s.cpu().tolist()[0]) for _, s in whole]
    assert [(r["target"], r["max_shift"]) for r in eng.st.pitch_register(eng.slots)] == [(8.5, 2.0), (6.0, 0.75)]
    # the same calls by hand, with the contour hook behind each: the start of the utterance restarts the estimates from their seeds
    eng.start_wav(_ref(2), follow=True, register=REG2)
    (c2, m2, w2, f0, uv), emits = _run(eng.st, eng.slots, wav)
    assert sum(emits) == 1 + N // HOP
    assert _same(f0, torch.cat([o for o, _ in whole])) and _same(uv, full.f0(wav)[1]), N
    assert torch.equal(c, c2) and torch.equal(m, m2) and torch.equal(w, w2)
    raw = full.f0(wav)[0]
    assert N < L or (int((uv == 0).sum()) >= f0.numel() // 2 and not torch.equal(f0, raw))      # (voiced contours, and matching moves them)
    assert _states(eng.st, eng.slots) == [tuple(s.cpu().tolist()[0]) for _, s in whole]
    eng.st.close()


def test_staggered_utterances_and_a_reused_slot(full):
    """Three utterances on two slots: the third takes a slot the first has left, whose reset restarts the estimate from the seed."""
    Ns = (4 * L + 333, 7 * L, 3 * L + 1)
    wavs = [torch.from_numpy(x).cuda() for x in (R.glide(Ns[0], seed=3), R.harmonic(180.0, Ns[1], seed=4), R.harmonic(300.0, Ns[2], seed=5))]
    regs = [dict(target=8.0), dict(target=6.5, prior_frames=10), dict(target=9.0, max_shift=1.0)]
    eng = StreamingVoiceConversionEngine(full, 2, max_ref_frames=64)
    log = {0: [], 1: []}
    feed = eng.feed_ragged

    def spy(slots, *a, **kw):      # the contour hook behind every call, per slot over its emitted frames
        res = feed(slots, *a, **kw)
        f0, uv = eng.st.step_wav_contour()
        for r, slot in enumerate(slots):
            e = res[r][1].shape[0]
            if e:
                log[slot].append((f0[r, :e].clone(), uv[r, :e].clone()))
        return res

    eng.feed_ragged = spy
    outs = eng.infer_wav_staggered(wavs, [0, 1, 2], _ref(3), pipelined=False, follow=True, register=regs)
    torch.cuda.synchronize()
    assert eng.staggered_slots == [0, 1, 0]      # utterance 2 waited for slot 0
    want = [full.f0_register(*full.f0(x[None]), **r) for x, r in zip(wavs, regs)]
    got = {slot: torch.cat([f for f, _ in rows]) for slot, rows in log.items()}
    assert _same(got[0], torch.cat([want[0][0][0], want[2][0][0]])) and _same(got[1], want[1][0][0])
    assert [o[1].shape[0] for o in outs] == [1 + n // HOP for n in Ns]
    assert _states(eng.st, [0, 1]) == [tuple(want[2][1].cpu().tolist()[0]), tuple(want[1][1].cpu().tolist()[0])]
    eng.st.close()


# ------------------------------------------------------------------------------------------------------------------ 3. pipelined = blocking

REG4 = [dict(target=8.25), None, dict(target=6.5, max_shift=0.5), dict(target=7.0, prior_frames=0)]
FOLLOW4 = [True, True, True, None]      # (the last slot has the register on and following off: nothing happens to it)


def _open_reg(full, slots, follow, regs, **kw):
    st = _open(full, slots, follow=follow, **kw)
    for slot, r in zip(slots, regs):
        if r is not None:
            st.set_pitch_register([slot], **r)
    return st


def test_pipelined_equals_blocking(full):
    slots = [2, 5, 0, 3]
    wav = torch.cat([_tones(13 * L + 77, seed=8), _tones(13 * L + 77, seed=9)])
    st = _open_reg(full, slots, FOLLOW4, REG4)
    (cb, mb, wb, f0b, uvb), eb = _run(st, slots, wav)
    sb = st.pitch_register(slots)
    assert len(eb) >= 13
    st.reset(slots, which=15)
    st.set_reference(slots, _ref(4))
    sampled = {}

    def on_call(k):      # before every third call: the contour of call k - 1, which emitted chunk k - 2 (the hook joins; the calls between stay back to back)
        if 3 <= k <= 12 and k % 3 == 0:
            sampled[k - 2] = tuple(t.clone() for t in st.step_wav_contour())

    (cp, mp, wp, _, _), ep = _run(st, slots, wav, pipelined=True, on_call=on_call)
    assert ep == eb and torch.equal(cp, cb) and torch.equal(mp, mb) and torch.equal(wp, wb)
    assert sorted(sampled) == [1, 4, 7, 10]
    for chunk, (f0p, uvp) in sampled.items():
        fr = slice(chunk * SEG, (chunk + 1) * SEG)
        assert _same(f0p, f0b[:, fr]) and _same(uvp, uvb[:, fr]), chunk
    assert st.pitch_register(slots) == sb and sb[1] is None and sb[0]["count"] > 50      # ... and the estimates
    st.close()


def test_pipelined_ragged_equals_blocking(full):
    slots, starts = [5, 0, 2, 4], [0, 2, 5, 1]
    Ns = (13 * L + 5, 12 * L, 9 * L + 400, 10 * L + 1)
    wavs = [torch.from_numpy(R.harmonic(150.0 + 40 * i, n, seed=80 + i)).cuda() for i, n in enumerate(Ns)]
    outs, states = [], []
    for pipelined in (False, True):
        st = _open_reg(full, slots, FOLLOW4, REG4)
        outs.append(_ragged(st, slots, wavs, starts, pipelined=pipelined, contour=not pipelined))
        states.append(st.pitch_register(slots))
        st.close()
    for u in range(4):
        for i in range(3):
            assert torch.equal(outs[0][u][i], outs[1][u][i]), (u, i)
    assert states[0] == states[1]
    for u in (0, 2):      # the blocking run's contours are the whole-signal ones
        want, s = full.f0_register(*full.f0(wavs[u][None]), **REG4[u])
        assert _same(outs[0][u][3], want[0]) and (states[0][u]["count"], states[0][u]["sum"]) == tuple(s.cpu().tolist()[0])


# ------------------------------------------------------------------------------------------------------------------ 4. into the decoder

def test_matched_steps_equal_the_hand_composed_path(full):
    """wav2mel chunk -> emformer_step -> decoder_step(f0=, uv=) fed conan_f0_register's contour -> hifigan_step, on a stream-set that
    never heard of following or registers, against the wav-in steps of slots with both."""
    slots = [4, 1]
    wav = _tones(3 * L + 500, seed=12)
    st = _open_reg(full, slots, [True, True], REG2)
    (c, m, w, f0, uv), _ = _run(st, slots, wav)
    st.close()
    raw, ruv = full.f0(wav)
    matched = torch.cat([full.f0_register(raw[i:i + 1], ruv[i:i + 1], **REG2[i])[0] for i in range(2)])
    assert _same(f0, matched) and not torch.equal(matched, raw)
    tw = _open(full, slots)
    cs, ms, ws = [], [], []
    for pos, emit, chunk in StreamingVoiceConversionEngine.chunks(tw, full.wav2mel(wav)):      # (chunks reads .seg and .rc only)
        _, _, codes = tw.emformer_step(slots, chunk, want_out=False, want_logits=False)
        mel = tw.decoder_step(slots, codes[:, :emit], f0=matched[:, pos:pos + emit], uv=ruv[:, pos:pos + emit])
        ws.append(tw.hifigan_step(slots, mel))
        cs.append(codes[:, :emit]); ms.append(mel)
    torch.cuda.synchronize()
    assert torch.equal(c, torch.cat(cs, 1)) and torch.equal(m, torch.cat(ms, 1)) and torch.equal(w, torch.cat(ws, 1))
    tw.close()


def test_the_decoder_hears_the_shift(full):
    """With the target two octaves above a steady source and a seed count of 0 the estimate is the source's own value from the first
    voiced frame on, so every voiced frame is moved by target - v exactly (the law).  The decoder's f0_denorm_pred tap is
    fminf(fmaxf(exp2f(v), 50), 900) (include/conan_hip.h, conan_pitch_cfg): 110 Hz against 440 Hz here, inside the clamp.  The taps are
    compared as log2 of their ratio in f64: each tap is one exp2f, which is within 1 ulp of f32 (2^-23 relative, 1.7e-7 octave), so the
    ratio's log2 is within 3.5e-7 octave of the shift; the bound is 2^-20 = 9.5e-7 octave, under three such steps.  Measured on the
    MI355X: 7.9e-8 octave."""
    slots = [4, 1]
    wav = torch.from_numpy(np.stack([R.harmonic(110.0, 3 * L, seed=1), R.harmonic(111.0, 3 * L, seed=2)])).cuda()
    raw, ruv = full.f0(wav)
    raw, ruv = raw[:, 3:3 + SEG].contiguous(), ruv[:, 3:3 + SEG].contiguous()
    assert not ruv.any()
    target = float(raw[0, 0]) + 2.0
    matched, _ = full.f0_register(raw, ruv, target=target, prior_frames=0, max_shift=4.0)
    for i in range(2):
        want, _ = G.match(raw[i].cpu().numpy(), ruv[i].cpu().numpy(), target=target, max_shift=4.0, seed=(0, 0))
        assert np.array_equal(matched[i].cpu().numpy().view(np.uint32), want.view(np.uint32))
    codes = (torch.arange(2 * SEG, device="cuda", dtype=torch.int32).reshape(2, SEG) * 7) % 50
    taps = []
    for contour in (raw, matched):
        st = _open(full, slots)
        st.reset(slots, which=2)
        taps.append(st.decoder_step(slots, codes, taps=True, f0=contour, uv=ruv)[1]["f0_denorm_pred"].double().cpu())
        st.close()
    heard = torch.log2(taps[1] / taps[0])
    law = matched.double().cpu() - raw.double().cpu()
    print("largest |log2(tap ratio) - shift| (octaves):", float((heard - law).abs().max()))
    assert (taps[1] > 3.9 * taps[0]).all() and float(taps[1].max()) < 900.0
    assert float((heard - law).abs().max()) <= 2.0 ** -20


# ------------------------------------------------------------------------------------------------------------------ 5. neighbours

def test_neighbours_keep_their_bits_and_launches(full):
    slots = [0, 1, 2, 3, 4, 5]
    follow = [True, True, None, True, True, None]
    regs = [dict(target=8.5), None, None, dict(target=6.0, max_shift=1.0), None, dict(target=9.0)]      # slot 5: register on, following off
    wav = torch.cat([_tones(3 * L + 77, seed=20 + i) for i in range(3)])
    plain = _open(full, slots)
    b = _open(full, slots, follow=follow)
    a = _open_reg(full, slots, follow, regs)
    assert b.state_bytes == plain.state_bytes + 4 * 2 * MAX_SLOTS * SEG * 4      # following alone: what it always counted
    assert a.state_bytes == b.state_bytes + 16 * MAX_SLOTS + 4 * 64 * MAX_SLOTS      # the state, and four row tables of 64-byte rows
    b.set_pitch_register(slots, cfg=None)      # turning it off where it never was on: nothing is allocated
    assert b.state_bytes == plain.state_bytes + 4 * 2 * MAX_SLOTS * SEG * 4 and b.pitch_register(slots) == [None] * 6
    plain.close()
    ((ca, ma, wa, _, _), emits), la = _launches(a, lambda: _run(a, slots, wav, contour=False))
    ((cb, mb, wb, _, _), _), lb = _launches(b, lambda: _run(b, slots, wav, contour=False))
    assert torch.equal(ca, cb)
    for i in (1, 2, 4, 5):
        assert torch.equal(ma[i], mb[i]) and torch.equal(wa[i], wb[i]), i
    for i in (0, 3):
        assert not torch.equal(ma[i], mb[i]), i
    # one more launch per call that emits, and nothing else; a stream-set that never enabled the register runs no such kernel
    assert "f0_register_kernel" not in lb
    assert la.pop("f0_register_kernel") == len(emits)
    assert la == lb, (la, lb)
    # the register off again: the launches and bits of the stream-set that never had it
    a.set_pitch_register(slots, cfg=None)
    a.reset(slots, which=15)
    a.set_reference(slots, _ref(6))
    ((_, m2, w2, _, _), _), l2 = _launches(a, lambda: _run(a, slots, wav, contour=False))
    assert l2 == lb and torch.equal(m2, mb) and torch.equal(w2, wb)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------ 6. live changes

def test_live_changes_take_effect_at_the_next_emitted_chunk(full):
    slots = [1, 3]
    wav = _tones(9 * L + 10, seed=30)
    raw, ruv = full.f0(wav)
    first, second = dict(target=8.5, prior_frames=20), dict(target=6.25, max_shift=0.5, prior=7.0, prior_frames=5)
    st = _open_reg(full, slots, [True, True], [first, first])
    seen = {}

    def on_call(k):      # before call k (call k emits chunk k - 1)
        if k == 3:
            before = _states(st, slots)
            st.set_pitch_register(slots, **second)                   # the voice change in the middle of a call
            seen["kept"] = (before, _states(st, slots))
        elif k == 5:
            st.set_pitch_register(slots, reseed=True, **second)
            seen["reseeded"] = _states(st, slots)
        elif k == 7:
            st.set_pitch_register(slots, cfg=None)

    (_, m, _, f0, uv), emits = _run(st, slots, wav, on_call=on_call)
    fr = lambda c0, c1: slice(c0 * SEG, c1 * SEG)      # frames of chunks [c0, c1)
    for i in range(2):
        v, u = raw[i].cpu().numpy(), ruv[i].cpu().numpy()
        a, s1 = G.match(v[fr(0, 2)], u[fr(0, 2)], **_kw(first))
        b, s2 = G.match(v[fr(2, 4)], u[fr(2, 4)], **dict(_kw(second), seed=s1))      # the new target, the estimate kept
        c, _ = G.match(v[fr(4, 6)], u[fr(4, 6)], **_kw(second))                      # restarted from the new seed
        want = np.concatenate([a, b, c, v[6 * SEG:]])                                # off: the followed contour as it is
        assert np.array_equal(f0[i].cpu().numpy().view(np.uint32), want.view(np.uint32)), i
        assert seen["kept"][0][i] == seen["kept"][1][i] == s1 and s1[0] > 20
        assert seen["reseeded"][i] == _kw(second)["seed"]      # pending: the query reports the seed
    assert _same(uv, ruv) and st.pitch_register(slots) == [None, None]
    # the mel heard it: against a stream-set that only ever followed
    fo = _open(full, slots, follow=[True, True])
    (_, mf, _, _, _), _ = _run(fo, slots, wav, contour=False)
    assert not torch.equal(m[:, fr(0, 2)], mf[:, fr(0, 2)])
    st.close(); fo.close()


# ------------------------------------------------------------------------------------------------------------------ 7. the hand-over

def test_a_stream_handed_over_with_its_state_continues_bit_for_bit(full):
    slots, dst = [1, 4], [3, 0]
    wav = _tones(7 * L + 123, seed=40)
    a = _open_reg(full, slots, [True, True], REG2)
    b = full.streams(MAX_SLOTS, 4, 64)
    lid, nbytes = b.layout_id, b.snapshot_bytes      # before any register call
    assert (a.layout_id, a.snapshot_bytes) == (lid, nbytes)
    (cw, mw, ww, f0w, uvw), _ = _run(a, slots, wav)
    a.reset(slots, which=15)      # (the setting persists; the estimates restart from their seeds)
    a.set_reference(slots, _ref(2))
    cut = 4      # calls before the export: chunks 0 .. 2 are out
    for k in range(cut):
        a.step_wav(slots, wav[:, k * L:(k + 1) * L])
    state = _states(a, slots)
    assert all(n > 50 for n, _ in state[:1])
    snap = a.export_slots(slots)
    b.import_slots(dst, snap)
    assert b.pitch_register(dst) == [None, None]      # a snapshot carries neither the setting nor the estimate
    b.set_pitch_follow(dst)
    for slot, cfg, s in zip(dst, REG2, state):
        b.set_pitch_register([slot], **dict(cfg, seed=s, reseed=True))
    assert _states(b, dst) == state
    (c, m, w, f0, uv), _ = _run_from(b, dst, wav, cut)
    done = (cut - 1) * SEG
    assert torch.equal(c, cw[:, done:]) and torch.equal(m, mw[:, done:]) and torch.equal(w, ww[:, done * HOP:])
    assert _same(f0, f0w[:, done:]) and _same(uv, uvw[:, done:])
    assert (a.layout_id, a.snapshot_bytes, b.layout_id, b.snapshot_bytes) == (lid, nbytes, lid, nbytes)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------ 8. the voice bank

def test_voice_bank_registers(full):
    eng = StreamingVoiceConversionEngine(full, 2, max_ref_frames=64)
    bank = VoiceBank(full, 4, 64)
    voices = torch.from_numpy(np.stack([R.harmonic(330.0, 8000, seed=50), R.harmonic(95.0, 8000, seed=51)])).cuda()
    bank.enroll_wav([2, 0], voices, via=eng.st, register=True)
    want = full.register_of(voices)
    assert bank.registers == {2: want[0], 0: want[1]}
    assert abs(want[0] - np.log2(330.0)) < 0.01 and abs(want[1] - np.log2(95.0)) < 0.01
    assert full.register_of(torch.zeros(1, 4000, device="cuda")) == [None]      # silence: no counted frame
    wav = _tones(4 * L + 200, seed=52)
    a = eng.infer_wav(wav, None, pipelined=False, voice=(bank, [2, 0]), follow=True, register="voice")
    got = eng.st.pitch_register(eng.slots)
    b = eng.infer_wav(wav, None, pipelined=False, voice=(bank, [2, 0]), follow=True, register=[want[0], want[1]])
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and eng.st.pitch_register(eng.slots) == got
    assert [r["target"] for r in got] == [float(np.float32(want[0])), float(np.float32(want[1]))]
    plain = eng.infer_wav(wav, None, pipelined=False, voice=(bank, [2, 0]), follow=True)
    assert not torch.equal(plain[1], a[1]) and eng.st.pitch_register(eng.slots) == [None, None]
    # enrolling an id again without the measurement, and removing one, drop the entries
    bank.enroll_wav([2], voices[:1], via=eng.st)
    assert set(bank.registers) == {0}
    bank.remove([0])
    assert bank.registers == {}
    with pytest.raises(ValueError, match="has no register"):
        eng.infer_wav(wav, None, voice=(bank, [2, 0]), follow=True, register="voice")
    bank.close(); eng.st.close()


# ------------------------------------------------------------------------------------------------------------------ 9. errors

def test_errors_change_nothing(full):
    slots = [0, 2]
    st = _open_reg(full, slots, [True, None], [dict(target=7.5), dict(target=8.0, max_shift=1.0)])
    wav = _tones(2 * L, seed=60)
    st.step_wav(slots, wav[:, :L])
    st.step_wav(slots, wav[:, L:])      # one chunk is out: slot 0 has an estimate of its own
    before = st.pitch_register(range(MAX_SLOTS))
    assert before[0]["count"] > 50 and before[2]["count"] == 50 and before[1] is None
    for bad in (dict(target=float("nan"), seed=(0, 0)), dict(target=7.0, max_shift=-1.0), dict(target=7.0, seed=(-1, 0)), dict(target=7.0, seed=(2, 2 ** 30))):
        with pytest.raises(_lib.ConanError) as e:
            st.set_pitch_register([2, 3], **bad)
        assert e.value.code == _lib.ERR_INVALID
    for bad_slots in ([2, 2], [1, MAX_SLOTS], [-1], [0, 3, 0]):      # a bad row: no slot of the call changes
        with pytest.raises(_lib.ConanError) as e:
            st.set_pitch_register(bad_slots, target=9.0, reseed=True)
        assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(ValueError):
        st.set_pitch_register([0])      # no target
    assert st.pitch_register(range(MAX_SLOTS)) == before
    buf = torch.empty(2, 2, dtype=torch.int64, device="cuda")
    one = np.asarray([0, 1], dtype=np.int32)      # slot 1 has no register
    assert st.lib.conan_streams_pitch_register_state(st.h, one.ctypes.data_as(C.c_void_p), 2, C.c_void_p(buf.data_ptr()), None) == _lib.ERR_STATE
    st.close()
    # a stream-set without the streaming front-end
    hp, sd_np, _ = P.model()
    c = Context(hp, None, 0, emformer=False, conan=True, hifigan=False)
    c.load_state_dict("conan", sd_np)
    c.finalize()
    dec = c.streams(2, 4, 64)
    with pytest.raises(_lib.ConanError) as e:
        dec.set_pitch_register([0], target=7.5)
    assert e.value.code == _lib.ERR_STATE
    with pytest.raises(_lib.ConanError) as e:
        dec.pitch_register([0])
    assert e.value.code == _lib.ERR_STATE
    dec.close()
    c.close()
