"""The voice bank on the GPU (conan_voices_*, conan_streams_set_voice[_mix]; include/conan_hip.h): a slot that is given an enrolled
voice in one launch against a second stream-set, created with the same arguments, whose slot ran conan_set_reference with the same
mel - one slot at a time, as enrolment runs one voice per pass.  Equality is torch.equal throughout, except where a test says why not.

Three voices with references of 9 (3 tokens; not a multiple of 4), 32 and 64 frames (the bank's maximum) in a bank of capacity 5;
stream-sets of 6 slots, max_frames 4, max_ref_frames 64 unless a test is about another size."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

from conan_amd import _lib, configs, synth
from conan_amd.engine import StreamingVoiceConversionEngine
from conan_amd.runtime import Context
from tests import pitch_ref as P

pytestmark = pytest.mark.gpu

MAX_SLOTS, FRAMES = 6, 12
LENS = (9, 32, 64)


@pytest.fixture(scope="module")
def ctx():
    hp, sd_np, _ = P.model()
    c = Context(hp, None, 0, emformer=False, conan=True, hifigan=False)
    c.load_state_dict("conan", sd_np)
    c.finalize()
    yield c
    c.close()


@pytest.fixture(scope="module")
def full():
    chp, vhp = configs.conan_hparams(True), configs.hifigan_hparams(True)
    c = Context(chp, vhp, 0)
    c.load_state_dict("emformer", synth.emformer_state_dict(chp, 0))
    c.load_state_dict("conan", synth.conan_state_dict(chp, 0))
    c.load_state_dict("hifigan", synth.hifigan_state_dict(vhp, 0))
    c.finalize()
    yield c
    c.close()


@pytest.fixture(scope="module")
def mels():
    """The voices' reference mels [L, 80] (cuda), and a fourth one (40 frames) for re-enrolment."""
    return [torch.from_numpy(synth.mel(L, 31 + i, 1)[0]).cuda() for i, L in enumerate(LENS + (40,))]


def _enrol(c, mels, via, capacity=5, max_ref=64, ids=(0, 1, 2)):
    """A bank with voice ids[i] = mels[i], enrolled in ONE call (padded rows, one length each)."""
    bank = c.voices(capacity, max_ref)
    width = max(m.shape[0] for m in mels[:len(ids)])
    ref = torch.zeros(len(ids), width, 80, device="cuda")
    for i in range(len(ids)):
        ref[i, :mels[i].shape[0]] = mels[i]
    bank.enroll(list(ids), ref, [mels[i].shape[0] for i in range(len(ids))], via=via)
    return bank


def _codes(n, frames=FRAMES, seed=0):
    return torch.from_numpy(synth.codes(frames, n, seed=7 + seed)).int().cuda()


def _steps(st, slots, codes, taps=False, lo=0, hi=None):
    """Decoder steps of 4 frames over frames [lo, hi) -> mel [n, hi - lo, 80]."""
    out = []
    for p in range(lo, codes.shape[1] if hi is None else hi, 4):
        m = st.decoder_step(slots, codes[:, p:p + 4], taps=taps)
        out.append((m[0] if taps else m).clone())
    return torch.cat(out, 1)


def _same_cache(a, sa, b, sb):
    ia, ca = a.prosody_ids(sa)
    ib, cb = b.prosody_ids(sb)
    return torch.equal(a.style_embed(sa), b.style_embed(sb)) and torch.equal(ia, ib) and torch.equal(ca, cb)


def _partner(c, mels, slots, voices, max_ref=64, **kw):
    """The comparison partner: a fresh stream-set whose slots[i] ran set_reference with mels[voices[i]], one slot at a time."""
    st = c.streams(MAX_SLOTS, 4, max_ref, **kw)
    st.reset(slots)
    for s, v in zip(slots, voices):
        st.set_reference([s], mels[v][None])
    return st


# ------------------------------------------------------------------------------------------------------------------ 1. assign = reference

def test_assign_equals_reference(ctx, mels):
    slots, voices = [5, 0, 3, 2], [2, 0, 1, 0]
    via = ctx.streams(MAX_SLOTS, 4, 64)
    bank = _enrol(ctx, mels, via)
    assert [bank.info(i) and bank.info(i)["ref_frames"] for i in range(5)] == [9, 32, 64, None, None]
    assert [bank.info(i)["tokens"] for i in range(3)] == [3, 8, 16]
    a = ctx.streams(MAX_SLOTS, 4, 64)
    a.reset(slots)
    assert a.voice(slots) == [-1] * 4
    a.profile_begin()
    a.set_voice(slots, bank, voices)
    a.profile_end()
    kernels = a.profile_kernels()
    assert [(k[0], k[3]) for k in kernels] == [("cnk::voice_assign_kernel", 1)], kernels      # one launch, no conv launch
    assert a.voice(slots) == voices and a.voice([1, 4]) == [-1, -1]
    b = _partner(ctx, mels, slots, voices)
    assert _same_cache(a, slots, b, slots)
    assert a.prosody_ids(slots)[1].tolist() == [16, 3, 8, 3]
    codes = _codes(4)
    ma, mb = _steps(a, slots, codes), _steps(b, slots, codes)                   # the persistent launch
    assert torch.equal(ma, mb) and bool(torch.isfinite(ma).all())
    assert not torch.equal(ma[1], ma[2])                                        # (two voices on the same codes would show nothing if equal)
    a.reset(slots, which=2); b.reset(slots, which=2)
    assert torch.equal(_steps(a, slots, codes, taps=True), _steps(b, slots, codes, taps=True))      # the separate launches
    # after set_reference the slot no longer reports a voice
    a.set_reference([slots[0]], mels[1][None])
    assert a.voice(slots) == [-1] + voices[1:]
    for st in (a, b, via):
        st.close()
    bank.close()


# ------------------------------------------------------------------------------------------------------------------ 2. switch mid-utterance

def test_switch_mid_utterance(ctx, mels):
    slots = [4, 1]
    a = ctx.streams(MAX_SLOTS, 4, 64)
    bank = _enrol(ctx, mels, a)                      # (enrolled through the stream-set that then uses the voices)
    codes = _codes(2, 16)
    a.reset(slots)
    a.set_voice(slots, bank, [0, 2])
    first = _steps(a, slots, codes, hi=8)
    a.set_voice(slots, bank, [1, 0])
    second = _steps(a, slots, codes, lo=8)
    b = _partner(ctx, mels, slots, [0, 2])
    assert torch.equal(first, _steps(b, slots, codes, hi=8))
    for s, v in zip(slots, [1, 0]):
        b.set_reference([s], mels[v][None])
    assert torch.equal(second, _steps(b, slots, codes, lo=8))
    # the step taken before the switch is the old voices'; the steps after it are not
    c = _partner(ctx, mels, slots, [0, 2])
    whole = _steps(c, slots, codes)
    assert torch.equal(whole[:, :8], first) and not torch.equal(whole[0, 8:], second[0]) and not torch.equal(whole[1, 8:], second[1])
    for st in (a, b, c):
        st.close()
    bank.close()


# ------------------------------------------------------------------------------------------------------------------ 3. ordering

def test_set_voice_is_ordered_between_pipelined_steps(full, mels):
    """step_async, set_voice (no join by the caller), step_async, join: the first step ran with the old voice, the second with the new
    one - the blocking loop that calls set_reference at the same point gives the same audio."""
    B, slots = 2, [1, 0]
    st = full.streams(B, max_frames=4, max_ref_frames=64)
    bank = _enrol(full, mels, st)
    seg, rc, hop = st.seg, st.rc, full.hop
    src = torch.from_numpy(synth.mel(2 * seg + rc, 5, B)).cuda()
    chunks = [src[:, j * seg:j * seg + seg + rc].contiguous() for j in range(2)]
    old, new = [0, 1], [2, 0]

    st.reset(slots)
    st.set_voice(slots, bank, old)
    outs = []
    for j, ch in enumerate(chunks):
        if j == 1:
            st.set_voice(slots, bank, new)
        w = torch.empty(B, seg * hop, device="cuda")
        st.step_async(slots, ch, w)
        outs.append(w)
    st.join()
    torch.cuda.synchronize()

    p = full.streams(B, max_frames=4, max_ref_frames=64)
    p.reset(slots)
    for s, v in zip(slots, old):
        p.set_reference([s], mels[v][None])
    w0 = p.step(slots, chunks[0])[2].clone()
    stay = p.export_slots(slots)
    for s, v in zip(slots, new):
        p.set_reference([s], mels[v][None])
    w1 = p.step(slots, chunks[1])[2].clone()
    p.import_slots(slots, stay)                       # ... and the second step had the voice not changed
    w1_old = p.step(slots, chunks[1])[2].clone()
    assert torch.equal(outs[0], w0) and torch.equal(outs[1], w1)
    assert not torch.equal(w1, w1_old)
    st.close(); p.close(); bank.close()


# ------------------------------------------------------------------------------------------------------------------ 4. different S_max

def test_bank_and_stream_set_of_different_sizes(ctx, mels):
    via = ctx.streams(MAX_SLOTS, 4, 64)
    bank = _enrol(ctx, mels, via)
    codes = _codes(3)
    # a larger stream-set takes all three
    slots, voices = [1, 4, 2], [0, 1, 2]
    a = ctx.streams(MAX_SLOTS, 4, 128)
    a.reset(slots)
    a.set_voice(slots, bank, voices)
    b = _partner(ctx, mels, slots, voices, max_ref=128)
    assert _same_cache(a, slots, b, slots) and torch.equal(_steps(a, slots, codes), _steps(b, slots, codes))
    a.close(); b.close()
    # a smaller one takes those that fit
    slots, voices = [3, 0], [1, 0]
    a = ctx.streams(MAX_SLOTS, 4, 32)
    a.reset(slots)
    a.set_voice(slots, bank, voices)
    b = _partner(ctx, mels, slots, voices, max_ref=32)
    assert _same_cache(a, slots, b, slots) and torch.equal(_steps(a, slots, codes[:2], hi=4), _steps(b, slots, codes[:2], hi=4))
    # ... and refuses the one that does not, before anything changes - also for the call's other slot
    style = a.style_embed(slots).clone()
    with pytest.raises(_lib.ConanError) as e:
        a.set_voice(slots, bank, [0, 2])
    assert e.value.code == _lib.ERR_SHAPE
    assert a.voice(slots) == voices and torch.equal(a.style_embed(slots), style) and _same_cache(a, slots, b, slots)
    assert torch.equal(_steps(a, slots, codes[:2], lo=4), _steps(b, slots, codes[:2], lo=4))
    # enrolment checks the length against both the bank and `via`
    small = ctx.voices(2, 32)
    for bk, v in ((small, via), (bank, a)):
        with pytest.raises(_lib.ConanError) as e:
            bk.enroll([0], mels[2][None], via=v)
        assert e.value.code == _lib.ERR_INVALID
    assert small.info(0) is None
    for x in (a, b, via, bank, small):
        x.close()


# ------------------------------------------------------------------------------------------------------------------ 5. copy semantics

def test_assignment_is_a_copy(ctx, mels):
    slots = [2, 5]
    a = ctx.streams(MAX_SLOTS, 4, 64)
    bank = _enrol(ctx, mels, a)
    codes = _codes(2)
    a.reset(slots)
    a.set_voice(slots, bank, [0, 1])
    b = _partner(ctx, mels, slots, [0, 1])
    assert torch.equal(_steps(a, slots, codes, hi=4), _steps(b, slots, codes, hi=4))
    bank.enroll([0], mels[3][None], via=a)           # id 0 is another voice now (40 frames: more tokens than the slot's copy holds)
    bank.remove([1])
    assert bank.info(0)["ref_frames"] == 40 and bank.info(1) is None
    assert torch.equal(_steps(a, slots, codes, lo=4, hi=8), _steps(b, slots, codes, lo=4, hi=8))
    bank.close()
    assert _same_cache(a, slots, b, slots) and a.voice(slots) == [0, 1]
    assert torch.equal(_steps(a, slots, codes, lo=8), _steps(b, slots, codes, lo=8))
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------ 6. mix

def test_mix(ctx, mels):
    via = ctx.streams(MAX_SLOTS, 4, 64)
    bank = _enrol(ctx, mels, via)
    a, b = ctx.streams(MAX_SLOTS, 4, 64), ctx.streams(MAX_SLOTS, 4, 64)
    slots = [3, 1]
    a.reset(slots); b.reset(slots)
    # k = 1, weight 1: set_voice's bits
    a.set_voice_mix(slots, bank, [[2], [0]], [[1.0], [1.0]])
    b.set_voice(slots, bank, [2, 0])
    codes = _codes(2)
    assert _same_cache(a, slots, b, slots) and torch.equal(_steps(a, slots, codes, hi=4), _steps(b, slots, codes, hi=4))
    assert a.voice(slots) == [-1, -1] and b.voice(slots) == [2, 0]
    # k = 3: the prosody side of the first voice, the style vector the fp32 fma chain
    w = np.array([0.5, 0.3, 0.2], np.float32)
    b.set_voice([0, 2, 4], bank, [0, 1, 2])
    styles = b.style_embed([0, 2, 4]).cpu().numpy().astype(np.float64)
    a.set_voice(slots[:1], bank, [0])
    assert a.voice(slots[:1]) == [0]
    a.set_voice_mix(slots[:1], bank, [[0, 1, 2]], [w])
    assert a.voice(slots[:1]) == [-1]
    ia, ca = a.prosody_ids(slots[:1])
    ib, cb = b.prosody_ids([0])
    assert torch.equal(ia, ib) and torch.equal(ca, cb) and ca.tolist() == [3]
    got = a.style_embed(slots[:1]).cpu().numpy()[0].astype(np.float64)
    terms = w.astype(np.float64)[:, None] * styles
    bound = 3 * 2.0 ** -24 * np.abs(terms).sum(0)                # k roundings of an fp32 fma chain
    err = np.abs(got - terms.sum(0))
    print("mix: max err %.3g, bound there %.3g, max |style| %.3g" % (err.max(), bound[err.argmax()], np.abs(got).max()))
    assert (err <= bound).all() and np.abs(terms.sum(0) - styles[0]).max() > 1e-3
    # weights must be finite, k in 1 .. 4
    for ids, ws in (([[0, 1]], [[0.5, float("nan")]]), ([[0, 1]], [[float("inf"), 0.5]]), ([[0, 1, 2, 0, 1]], [[0.2] * 5])):
        with pytest.raises(_lib.ConanError) as e:
            a.set_voice_mix(slots[:1], bank, ids, ws)
        assert e.value.code == _lib.ERR_INVALID
    for x in (a, b, via, bank):
        x.close()


# ------------------------------------------------------------------------------------------------------------------ 7. export / import

def test_export_import(ctx, mels):
    via = ctx.streams(MAX_SLOTS, 4, 64)
    bank = _enrol(ctx, mels, via)
    vs = bank.export([0, 2])
    assert len(vs) == 2 and [vs.info(i)["ref_frames"] for i in range(2)] == [9, 64] and [vs.info(i)["tokens"] for i in range(2)] == [3, 16]
    assert vs.info(0)["bytes"] == bank.info(0)["bytes"] < vs.info(1)["bytes"] <= bank.blob_bytes and bank.blob_bytes % 256 == 0
    carried = pickle.loads(pickle.dumps(vs.cpu()))
    assert not carried.blob.is_cuda and carried.meta == vs.meta
    other = ctx.voices(2, 64)
    other.import_voices([1, 0], carried)
    assert other.info(1) == bank.info(0) and other.info(0) == bank.info(2)
    a, b = ctx.streams(MAX_SLOTS, 4, 64), ctx.streams(MAX_SLOTS, 4, 64)
    slots = [0, 5]
    a.reset(slots); b.reset(slots)
    a.set_voice(slots, other, [1, 0])
    b.set_voice(slots, bank, [0, 2])
    codes = _codes(2)
    assert _same_cache(a, slots, b, slots) and torch.equal(_steps(a, slots, codes), _steps(b, slots, codes))
    # ... and both equal the set_reference partner
    p = _partner(ctx, mels, slots, [0, 2])
    assert _same_cache(a, slots, p, slots)
    # exporting what was imported gives the same rows
    again = other.export([1, 0])
    used = [vs.info(i)["bytes"] for i in range(2)]
    assert all(torch.equal(again.blob[i, :used[i]], vs.blob[i, :used[i]]) for i in range(2)) and again.meta == vs.meta
    # a record of another layout id; a voice that does not fit
    M = _lib.VOICE_META_BYTES
    bad = bytearray(carried.select([0]).meta)
    bad[16] ^= 0x01                                   # (the layout id follows the record's four leading words)
    from conan_amd.runtime import VoiceSet
    with pytest.raises(_lib.ConanError) as e:
        other.import_voices([0], VoiceSet(bytes(bad), carried.select([0]).blob))
    assert e.value.code == _lib.ERR_SHAPE and len(bad) == M
    small = ctx.voices(3, 32)
    with pytest.raises(_lib.ConanError) as e:
        small.import_voices([0, 1], carried)
    assert e.value.code == _lib.ERR_SHAPE and small.info(0) is None and small.info(1) is None      # nothing changed
    small.import_voices([2], carried.select([0]))    # the 9-frame voice fits a smaller bank
    a.set_voice(slots[:1], small, [2])
    assert _same_cache(a, slots[:1], p, slots[:1])
    with pytest.raises(_lib.ConanError) as e:
        bank.export([3])
    assert e.value.code == _lib.ERR_STATE
    for x in (a, b, p, via, bank, other, small):
        x.close()


# ------------------------------------------------------------------------------------------------------------------ 8. snapshots

def test_snapshots_carry_the_copy(ctx, mels):
    a, b = ctx.streams(MAX_SLOTS, 4, 64), ctx.streams(MAX_SLOTS, 4, 64)
    bank = _enrol(ctx, mels, a)
    lid, nbytes = b.layout_id, b.snapshot_bytes
    codes = _codes(1)
    a.reset([2])
    a.set_voice([2], bank, [1])
    assert (a.layout_id, a.snapshot_bytes) == (lid, nbytes)      # existing blobs need no new section
    want = _steps(a, [2], codes)
    a.reset([2], which=2)
    _steps(a, [2], codes, hi=4)
    snap = a.export_slots([2])
    assert snap.info(0)["has_ref"]
    b.reset([4])
    b.import_slots([4], snap.cpu().to("cuda"))
    assert b.voice([4]) == [-1] and a.voice([2]) == [1]          # the id stays behind: it names an entry of a bank, not a voice
    assert torch.equal(_steps(b, [4], codes, lo=4), want[:, 4:])
    a.close(); b.close(); bank.close()


# ------------------------------------------------------------------------------------------------------------------ 9. errors

def test_errors(ctx, mels):
    st = ctx.streams(MAX_SLOTS, 4, 64)
    fresh = ctx.voices(5, 64)
    assert all(fresh.info(i) is None for i in range(5))
    info = _lib.VoiceInfo()
    assert st.lib.conan_voices_info(fresh.h, 5, C.byref(info)) == _lib.ERR_INVALID
    bank = _enrol(ctx, mels, st)
    st.reset([0, 1])

    def code(call):
        with pytest.raises(_lib.ConanError) as e:
            call()
        return e.value.code

    assert code(lambda: st.set_voice([0], bank, [3])) == _lib.ERR_STATE           # not enrolled
    assert code(lambda: st.set_voice([0], fresh, [0])) == _lib.ERR_STATE
    assert code(lambda: st.set_voice([0], bank, [5])) == _lib.ERR_INVALID         # = capacity
    assert code(lambda: st.set_voice([0], bank, [-1])) == _lib.ERR_INVALID
    assert code(lambda: st.set_voice([0, 0], bank, [0, 1])) == _lib.ERR_INVALID   # duplicate slots
    assert code(lambda: st.set_voice([6], bank, [0])) == _lib.ERR_INVALID
    assert code(lambda: st.set_voice_mix([0], bank, [[0, 3]], [[0.5, 0.5]])) == _lib.ERR_STATE
    assert code(lambda: bank.enroll([0, 0], torch.stack([mels[1], mels[1]]), via=st)) == _lib.ERR_INVALID
    assert code(lambda: bank.enroll([5], mels[1][None], via=st)) == _lib.ERR_INVALID
    # a bank, or a `via`, of another context
    hp, sd_np, _ = P.model()
    c2 = Context(hp, None, 0, emformer=False, conan=True, hifigan=False)
    c2.load_state_dict("conan", sd_np)
    c2.finalize()
    st2 = c2.streams(2, 4, 64)
    bank2 = _enrol(c2, mels, st2)
    assert code(lambda: st.set_voice([0], bank2, [0])) == _lib.ERR_INVALID
    assert code(lambda: bank.enroll([4], mels[1][None], via=st2)) == _lib.ERR_INVALID
    assert bank.info(4) is None
    # none of the refused calls gave slot 0 a reference
    assert st.voice([0, 1]) == [-1, -1]
    assert code(lambda: st.decoder_step([0], _codes(1)[:, :4])) == _lib.ERR_STATE
    st.set_voice([1], bank, [0])                      # repeated voice ids are fine
    st.set_voice([0, 1], bank, [1, 1])
    assert st.voice([0, 1]) == [1, 1] and torch.equal(st.style_embed([0]), st.style_embed([1]))
    assert bool(torch.isfinite(st.decoder_step([0, 1], _codes(2)[:, :4])).all())
    for x in (st, bank, fresh, st2, bank2):
        x.close()
    c2.close()


# ------------------------------------------------------------------------------------------------------------------ 10. engine

def test_engine(full, mels):
    n = 3
    ea, eb = (StreamingVoiceConversionEngine(full, n, max_ref_frames=64) for _ in range(2))
    bank = _enrol(full, mels, ea.st)
    slots, voices, later = [2, 0, 1], [1, 2, 0], [0, 0, 2]
    L = ea.seg * full.hop
    rng = np.random.default_rng(3)
    t = np.arange(5 * L) / 16000.0
    src = torch.from_numpy(np.stack([0.3 * np.sin(2 * np.pi * (140 + 60 * i) * t) + 0.05 * rng.standard_normal(t.shape[0]) for i in range(n)]).astype(np.float32)).cuda()

    def feed(eng, j):
        res = eng.feed_ragged(slots, src[:, j * L:(j + 1) * L].contiguous(), [L] * n, [0] * n)
        return [tuple(x.clone() for x in r) for r in res]

    ea.open_slots(slots, None, voice=(bank, voices))
    for s, v in zip(slots, voices):
        eb.open_slots([s], mels[v][None])
    assert ea.st.voice(slots) == voices
    emitted = 0
    for j in range(5):
        if j == 3:      # a live change between feeds
            ea.set_voice(slots, bank=bank, ids=later)
            for s, v in zip(slots, later):
                eb.st.set_reference([s], mels[v][None])
        ra, rb = feed(ea, j), feed(eb, j)
        for (wa, ma, ca), (wb, mb, cb) in zip(ra, rb):
            assert torch.equal(wa, wb) and torch.equal(ma, mb) and torch.equal(ca, cb)
            emitted += ma.shape[0]
    assert emitted >= 3 * n * ea.seg
    # a whole utterance: infer with a voice in place of the reference mel (one stream: its style pass is one reference per pass)
    e1 = StreamingVoiceConversionEngine(full, 1, max_ref_frames=64)
    src_mel = torch.from_numpy(synth.mel(2 * ea.seg + 1, 5, 1)).cuda()
    gv = [x.clone() for x in e1.infer(src_mel, None, voice=(bank, [1]))]
    gr = [x.clone() for x in e1.infer(src_mel, mels[1][None])]
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(gv, gr)) and gv[0].shape[1] == src_mel.shape[1] * full.hop
    for x in (ea.st, eb.st, e1.st, bank):
        x.close()


# ------------------------------------------------------------------------------------------------------------------ 11. across configurations

def test_a_voice_enrolled_on_f32_serves_a_limb_stream_set(full, mels):
    """A voice enrolled through an arith='f32' stream-set, assigned to an arith='limb' one, against the limb set's own set_reference
    run.  The bound to hold across configurations is the decoder's (atol 1e-4, rtol 1e-4: tests/test_gpu_pitch.py, test_gpu_round3.py);
    measured on an MI355X the style pass is identical in both forms - the limb forms exist for the vocoder's convolutions only, the
    style pass's run on the f32-input MFMA in either stream-set: max |d style| 0, max |d mel| 0 - so equality is asserted."""
    slots, voices = [4, 1, 2], [0, 1, 2]
    via = full.streams(MAX_SLOTS, 4, 64, arith="f32")
    bank = _enrol(full, mels, via)
    a = full.streams(MAX_SLOTS, 4, 64, arith="limb")
    assert via.arith == "f32" and a.arith == "limb"
    a.reset(slots)
    a.set_voice(slots, bank, voices)
    b = _partner(full, mels, slots, voices, arith="limb")
    codes = _codes(3)
    ma, mb = _steps(a, slots, codes), _steps(b, slots, codes)
    ds = (a.style_embed(slots) - b.style_embed(slots)).abs().max().item()
    print("f32 -> limb: max |d style| %.3g, max |d mel| %.3g" % (ds, (ma - mb).abs().max().item()))
    assert _same_cache(a, slots, b, slots) and torch.equal(ma, mb)
    for x in (a, b, via, bank):
        x.close()
