"""Per-slot pitch control of the decoder step on the GPU (conan_streams_set_pitch / conan_decoder_step_pitch; include/conan_hip.h,
conan_pitch_cfg) against tests/pitch_ref.py - the law in numpy and a decoder built from the oracle's pieces - across the decoder
step's launch forms, and against itself: a slot that does not ask keeps its bits, a change takes effect at the next step through a
cached program, the contour path, the whole path, snapshots.

Tolerances.  uv_pred (the head's raw output) atol 2e-4, rtol 1e-4 and mel atol 1e-4, rtol 1e-4 against the reference: the figures
of the decoder's tests (tests/test_gpu_round3.py, test_gpu_parity.py).  A persistent launch against the separate launches of the same
step: atol 2e-5, rtol 1e-5 (test_decoder_megakernel_equals_the_separate_launches).  Bins are compared on the rows pitch_ref calls
safe (mel-scale value 1e-3 away from a rounding boundary, d0 1e-3 away from the threshold); tests/test_pitch_cpu.py shows with the
reference alone that at most 5 % of every case's rows are not.  The f0 tap on those rows: rtol 1e-3 = ln 2 * (2e-4 + 1e-4 * 10), what
uv_pred's tolerance means for 2^v at |v| <= 10.  The mel reference embeds the GPU's own bins, so a row on a boundary cannot leak into it."""
import ctypes as C

import numpy as np
import pytest
import torch

from conan_amd import _lib, configs, synth
from conan_amd.engine import StreamingVoiceConversionEngine
from conan_amd.runtime import Context, _i32, _ptr, _stream
from tests import pitch_ref as P

pytestmark = pytest.mark.gpu

MAX_SLOTS = 6


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


def _open(ctx, n, dev_plan=None, seed=0):
    """A stream-set of MAX_SLOTS slots with the case's n streams started in SLOT_LISTS[n] -> (streams, slots, codes [n, FRAMES] cuda)."""
    st = ctx.streams(MAX_SLOTS, 4, 64, dev_plan=dev_plan)
    slots = P.SLOT_LISTS[n]
    ref, codes = P.inputs(n, seed)
    st.reset(slots)
    st.set_reference(slots, torch.from_numpy(ref).cuda())
    return st, slots, torch.from_numpy(codes).int().cuda()


def _apply(st, slots, cfgs):
    for slot, cfg in zip(slots, cfgs):
        st.set_pitch([slot], cfg)


def _run(st, slots, codes, T, taps, frames=P.FRAMES, f0=None, uv=None, lo=0):
    """Decoder steps of T frames over frames [lo, frames) -> (mel [n, frames - lo, 80] cpu, dict of the concatenated taps or None)."""
    mels, tps = [], []
    for p in range(lo, frames, T):
        q = slice(p, min(p + T, frames))
        out = st.decoder_step(slots, codes[:, q], taps=taps, f0=None if f0 is None else f0[:, q], uv=None if uv is None else uv[:, q])
        if taps:
            mels.append(out[0].cpu())
            tps.append({k: out[1][k].cpu() for k in ("uv_pred", "f0_denorm_pred", "pitch_bins")})
        else:
            mels.append(out.cpu())
    tp = {k: torch.cat([t[k] for t in tps], 1).numpy() for k in tps[0]} if taps else None
    return torch.cat(mels, 1).numpy(), tp


def _check(n, segments, mel, tp, frames=P.FRAMES, f0=None, uv=None, tag=""):
    """A tapped GPU run against the reference that embeds the GPU's bins."""
    want = P.reference_rows(n, 0, segments, f0=f0, uv=uv, bins=tp["pitch_bins"], frames=frames)
    unsafe = np.stack([w["unsafe"] for w in want])
    print(tag, "unsafe share %.4f" % unsafe.mean(), "max |d uv_pred| %.3g" % max(np.abs(tp["uv_pred"][b] - want[b]["uv_pred"]).max() for b in range(n)),
          "max |d mel| %.3g" % max(np.abs(mel[b] - want[b]["mel_out"]).max() for b in range(n)))
    assert unsafe.mean() <= 0.05, tag
    for b in range(n):
        np.testing.assert_allclose(tp["uv_pred"][b], want[b]["uv_pred"], atol=2e-4, rtol=1e-4, err_msg=str((tag, b)))
        safe = ~want[b]["unsafe"]
        assert np.array_equal(tp["pitch_bins"][b][safe], want[b]["pitch_bins"][safe]), (tag, b)
        np.testing.assert_allclose(tp["f0_denorm_pred"][b][safe], want[b]["f0_denorm_pred"][safe], rtol=1e-3, atol=0, err_msg=str((tag, b)))
        assert tp["pitch_bins"][b].min() >= 1 and tp["pitch_bins"][b].max() <= 255
        np.testing.assert_allclose(mel[b], want[b]["mel_out"], atol=1e-4, rtol=1e-4, err_msg=str((tag, b)))
    return want


# ------------------------------------------------------------------------------------------------------------------ 1. the law per launch form

@pytest.mark.parametrize("name", list(P.LAW_CASES))
def test_law_per_launch_form(ctx, name):
    n, T, cfgs = P.LAW_CASES[name]
    frames = P.FRAMES // T * T
    st, slots, codes = _open(ctx, n)
    assert slots != list(range(n))
    _apply(st, slots, cfgs)
    assert st.pitch(slots) == [P.f32_cfg(c) for c in cfgs]
    mel_t, tp = _run(st, slots, codes, T, True, frames)
    want = _check(n, [(0, cfgs)], mel_t, tp, frames, tag=name)
    if name == "n6_T4_tiles":      # a case in which no cfg moved a bin would show nothing
        base = P.reference_rows(n, 0, [(0, [None] * n)])
        voiced = ~base[1]["uv"]
        assert ((base[1]["pitch_bins"] != want[1]["pitch_bins"]) & voiced).sum() >= voiced.sum() / 4 and voiced.sum() >= 4
    if name != "n1_T4_taps":
        # without taps: the persistent launch (xcd mode at 2 streams, two row tiles at 6; the ragged step keeps separate launches)
        st.reset(slots, which=2)
        mel_m, _ = _run(st, slots, codes, T, False, frames)
        np.testing.assert_allclose(mel_m, mel_t, atol=2e-5, rtol=1e-5)
        sep, _, _ = _open(ctx, n, dev_plan="DEC_MEGA=0")
        _apply(sep, slots, cfgs)
        mel_s, _ = _run(sep, slots, codes, T, False, frames)
        np.testing.assert_allclose(mel_m, mel_s, atol=2e-5, rtol=1e-5)
        sep.close()
    st.close()


# ------------------------------------------------------------------------------------------------------------------ 2. a slot that does not ask

# conan_streams_state_bytes of the parent commit's library for ctx.streams(6, 4, 64) on this context (Conan only, full size), read from
# a run of that library: the table adds 24 bytes per slot and nothing else
PARENT_STATE_BYTES = 110765772


@pytest.mark.parametrize("n", [2, 6])
def test_nothing_changes_for_a_slot_that_does_not_ask(ctx, n):
    cfgs = P.ROW_CFGS[:n]
    a, slots, codes = _open(ctx, n)
    b, _, _ = _open(ctx, n)
    before = a.state_bytes
    _apply(a, slots, cfgs)
    assert a.state_bytes == before == b.state_bytes      # the table came with the stream-set; the setter allocates no stream state
    if PARENT_STATE_BYTES is not None:
        assert before == PARENT_STATE_BYTES + 24 * MAX_SLOTS
    ma = torch.from_numpy(_run(a, slots, codes, 4, False)[0])
    mb = torch.from_numpy(_run(b, slots, codes, 4, False)[0])
    off = [i for i, c in enumerate(cfgs) if c is None]
    on = [i for i, c in enumerate(cfgs) if c is not None]
    assert off and on
    for i in off:
        assert torch.equal(ma[i], mb[i]), i
    assert 1 in on and not torch.equal(ma[1], mb[1])      # (row 1, the +5 semitone slot, has voiced frames: tests/test_pitch_cpu.py)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------ 3. a change at the next step

def _fixed_steps(st, slots, codes, cbuf, mbuf, lo, hi):
    """conan_decoder_step on the SAME code and mel buffers every step (the persistent launch's cached program) -> mel [n, hi - lo, 80] cpu."""
    a, p = _i32(slots)
    out = []
    for q in range(lo, hi, 4):
        cbuf.copy_(codes[:, q:q + 4])
        _lib.check(st.lib.conan_decoder_step(st.h, p, len(a), 4, _ptr(cbuf), _ptr(mbuf), None, None, None, None, _stream()))
        out.append(mbuf.cpu())
    return torch.cat(out, 1).numpy()


def test_a_change_takes_effect_at_the_next_step_through_a_cached_program(ctx):
    n, cut = 6, P.SWITCH_FRAME
    segments = [(0, P.ROW_CFGS), (cut, P.ALT_CFGS)]
    # the tapped run with the switch, against the reference that switches at that frame
    t, slots, codes = _open(ctx, n)
    _apply(t, slots, P.ROW_CFGS)
    m0, tp0 = _run(t, slots, codes, 4, True, cut)
    _apply(t, slots, P.ALT_CFGS)
    m1, tp1 = _run(t, slots, codes, 4, True, lo=cut)
    mel_t = np.concatenate([m0, m1], 1)
    _check(n, segments, mel_t, {k: np.concatenate([tp0[k], tp1[k]], 1) for k in tp0}, tag="switch")
    t.close()
    # the persistent launch on fixed buffers: the program recorded before the change is replayed after it
    st, _, _ = _open(ctx, n)
    cbuf = torch.empty(n, 4, dtype=torch.int32, device="cuda")
    mbuf = torch.empty(n, 4, 80, device="cuda")
    _apply(st, slots, P.ROW_CFGS)
    got0 = _fixed_steps(st, slots, codes, cbuf, mbuf, 0, cut)
    _apply(st, slots, P.ALT_CFGS)
    got1 = _fixed_steps(st, slots, codes, cbuf, mbuf, cut, P.FRAMES)
    np.testing.assert_allclose(np.concatenate([got0, got1], 1), mel_t, atol=2e-5, rtol=1e-5)
    assert np.abs(got1 - _keep_first(ctx, n, codes, cut)).max() > 1e-3      # (the change did change the frames behind it)
    # enabled = 0 again: today's bits from a common reset on
    plain, _, _ = _open(ctx, n)
    want = _fixed_steps(plain, slots, codes, cbuf, mbuf, 0, P.FRAMES)
    _apply(st, slots, [None] * n)
    assert st.pitch(slots) == [None] * n
    st.reset(slots, which=2)
    again = _fixed_steps(st, slots, codes, cbuf, mbuf, 0, P.FRAMES)
    assert np.array_equal(again, want)
    st.close(); plain.close()


def _keep_first(ctx, n, codes, cut):
    """Frames [cut, FRAMES) of the run that keeps ROW_CFGS to the end."""
    st, slots, _ = _open(ctx, n)
    _apply(st, slots, P.ROW_CFGS)
    mel, _ = _run(st, slots, codes, 4, False)
    st.close()
    return mel[:, cut:]


def test_the_setter_joins_pipelined_steps(full):
    """set_pitch between pipelined chunk steps, with steps in flight: the blocking loop with the same change gives the same bits."""
    B, cut, nchunk = 2, 3, 7
    st = full.streams(B, max_frames=4, max_ref_frames=64)
    seg, rc, hop = st.seg, st.rc, full.hop
    slots = [1, 0]
    mel = torch.from_numpy(synth.mel(nchunk * seg + rc, 5, B)).cuda()
    ref = torch.from_numpy(synth.mel(40, 9, B)).cuda()
    chunks = [mel[:, j * seg:j * seg + seg + rc].contiguous() for j in range(nchunk)]

    def run(pipelined, switch):
        st.reset(slots)
        st.set_reference(slots, ref)
        st.set_pitch(slots, None)
        outs = []
        for j, ch in enumerate(chunks):
            if switch and j == cut:
                st.set_pitch([slots[0]], shift_semitones=4.0)      # (no join by the caller)
            if pipelined:
                m, w = torch.empty(B, seg, 80, device="cuda"), torch.empty(B, seg * hop, device="cuda")
                st.step_async(slots, ch, w, mel_out=m)
            else:
                _, m, w = st.step(slots, ch)
            outs.append((m, w))
        st.join()
        torch.cuda.synchronize()
        return torch.cat([o[0] for o in outs], 1).clone(), torch.cat([o[1] for o in outs], 1).clone()

    bm, bw = run(False, True)
    pm, pw = run(True, True)
    assert torch.equal(bm, pm) and torch.equal(bw, pw)
    nm, _ = run(True, False)
    assert torch.equal(nm[:, :cut * seg], pm[:, :cut * seg]) and torch.equal(nm[1], pm[1])      # before the change; the other slot
    assert not torch.equal(nm[0, cut * seg:], pm[0, cut * seg:])
    st.close()


# ------------------------------------------------------------------------------------------------------------------ 4. the caller's contour

@pytest.mark.parametrize("n", [2, 6])
def test_contour(ctx, n):
    f0, uv = P.contour(n)
    f0d, uvd = torch.from_numpy(f0).cuda(), torch.from_numpy(uv).cuda()
    st, slots, codes = _open(ctx, n)
    silent = P.model()[0]["silent_token"]
    assert bool((codes[:, 0] == silent).all()) and (uv[:, 0] == 0).all()
    for tag, cfgs, u, ud in (("contour", [None] * n, uv, uvd), ("contour, uv=None", [None] * n, None, None), ("contour + cfg", P.ROW_CFGS[:n], uv, uvd)):
        _apply(st, slots, cfgs)
        st.reset(slots, which=2)
        mel_t, tp = _run(st, slots, codes, 4, True, f0=f0d, uv=ud)
        _check(n, [(0, cfgs)], mel_t, tp, f0=f0, uv=u, tag="%s n=%d" % (tag, n))
        # the silent-token frame the caller marked voiced stays voiced: no forcing on this path
        assert (tp["f0_denorm_pred"][:, 0] >= 50.0).all() and (tp["pitch_bins"][:, 0] > 1).all()
        if u is None:
            assert (tp["f0_denorm_pred"] >= 50.0).all()
        st.reset(slots, which=2)
        mel_m, _ = _run(st, slots, codes, 4, False, f0=f0d, uv=ud)      # without taps: the persistent launch carries the contour
        np.testing.assert_allclose(mel_m, mel_t, atol=2e-5, rtol=1e-5)
    # a contour of NaN and infinities: every bin in 1 .. 255, a finite mel
    _apply(st, slots, [None, dict(range=4.0, shift_semitones=48.0)] + [None] * (n - 2))
    bad = torch.tensor([float("nan"), float("inf"), float("-inf"), 1e30], device="cuda").repeat(n, P.FRAMES // 4)
    for ud in (None, torch.full((n, P.FRAMES), float("nan"), device="cuda")):
        st.reset(slots, which=2)
        mel_b, tpb = _run(st, slots, codes, 4, True, f0=bad, uv=ud)
        assert tpb["pitch_bins"].min() >= 1 and tpb["pitch_bins"].max() <= 255 and np.isfinite(mel_b).all()
        assert list(tpb["pitch_bins"][0, :4]) == [1, 255, 1, 255]
        st.reset(slots, which=2)
        assert np.isfinite(_run(st, slots, codes, 4, False, f0=bad, uv=ud)[0]).all()
    st.close()


def test_conan_forward_takes_the_contour(ctx):
    from conan_amd.modules.Conan.Conan import Conan
    n = 2
    hp, sd_np, _ = P.model()
    f0, uv = P.contour(n)
    ref, codes = P.inputs(n)
    m = Conan(0, hp)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    kw = dict(content=torch.from_numpy(codes).cuda(), ref=torch.from_numpy(ref).cuda(), global_steps=200000)
    ret = m(f0=torch.from_numpy(f0).cuda(), uv=torch.from_numpy(uv).cuda(), infer=False, **kw)
    tp = {k: ret[k].cpu().numpy() for k in ("uv_pred", "f0_denorm_pred", "pitch_bins")}
    want = _check(n, [(0, [None] * n)], ret["mel_out"].cpu().numpy(), tp, f0=f0, uv=uv, tag="Conan.forward(f0=, uv=, infer=False)")
    # the same mel as the decoder steps of test_contour
    st, slots, cd = _open(ctx, n)
    mel_s, _ = _run(st, slots, cd, 4, True, f0=torch.from_numpy(f0).cuda(), uv=torch.from_numpy(uv).cuda())
    np.testing.assert_allclose(ret["mel_out"].cpu().numpy(), mel_s, atol=1e-4, rtol=1e-4)
    st.close()
    # fdiff as the reference computes it (Conan.py:343-350) from the raw head output
    nonpad = (uv == 0).astype(np.float64)
    fd = (((np.stack([w["uv_pred"][:, 1] for w in want]).astype(np.float64) - f0) ** 2) * nonpad).sum() / nonpad.sum() * hp.get("lambda_f0", 1.0)
    assert abs(float(ret["fdiff"]) - fd) <= 1e-3 * max(1.0, fd)
    # infer=True ignores a contour (Conan.py:174-175); infer=False without one is still not covered
    plain = m(infer=True, **kw)
    same = m(f0=torch.from_numpy(f0).cuda(), uv=torch.from_numpy(uv).cuda(), infer=True, **kw)
    assert torch.equal(plain["mel_out"], same["mel_out"]) and plain["fdiff"] == 0.0
    assert not torch.equal(plain["mel_out"], ret["mel_out"])
    with pytest.raises(NotImplementedError):
        m(infer=False, **kw)


# ------------------------------------------------------------------------------------------------------------------ 5. the whole path

def test_whole_path(full):
    B = 2
    eng = StreamingVoiceConversionEngine(full, B, max_ref_frames=64)
    L = eng.seg * full.hop
    rng = np.random.default_rng(3)
    t = np.arange(4 * L + 333) / 16000.0
    src = torch.from_numpy(np.stack([0.3 * np.sin(2 * np.pi * (140 + 60 * i) * t) + 0.05 * rng.standard_normal(t.shape[0]) for i in range(B)]).astype(np.float32)).cuda()
    ref = torch.from_numpy(synth.mel(40, 3, B)).cuda()
    pitch = {"shift_semitones": -3}
    plain = [x.clone() for x in eng.infer_wav(src, ref, pipelined=False)]
    blocking = [x.clone() for x in eng.infer_wav(src, ref, pipelined=False, pitch=pitch)]
    piped = [x.clone() for x in eng.infer_wav(src, ref, pipelined=True, pitch=pitch)]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(blocking, piped))
    assert torch.equal(plain[2], blocking[2]) and not torch.equal(plain[1], blocking[1]) and not torch.equal(plain[0], blocking[0])
    # the setting persists across a reset: the next utterance on the slots, started without a word about pitch at this level
    eng.st.reset(eng.slots, which=15)
    assert eng.st.pitch(eng.slots) == [P.f32_cfg(dict(shift_semitones=-3.0))] * B
    eng.st.set_reference(eng.slots, ref)
    outs, pos, N = [], 0, src.shape[1]
    last = (N - 1) // L * L
    fin = False
    while True:
        if pos < last:
            w, m, c = eng.feed(src[:, pos:pos + L]); pos += L
        else:
            w, m, c = eng.feed(src[:, pos:] if not fin else src[:, :0], final=True)
            pos, done, fin = N, fin and m.shape[1] == 0, True
            if done:
                break
        if m.shape[1]:
            outs.append((w.clone(), m.clone(), c.clone()))
    again = [torch.cat(x, 1) for x in zip(*outs)]
    assert all(torch.equal(a, b) for a, b in zip(again, blocking))
    # a live change between feeds, then off: the engine's own setter
    eng.set_pitch(shift_semitones=2.0)
    assert eng.st.pitch(eng.slots) == [P.f32_cfg(dict(shift_semitones=2.0))] * B
    eng.set_pitch()
    assert eng.st.pitch(eng.slots) == [None] * B
    assert all(torch.equal(a, b) for a, b in zip(eng.infer_wav(src, ref, pipelined=True), plain))


# ------------------------------------------------------------------------------------------------------------------ 6. snapshots

def test_snapshots_carry_the_cfg(ctx):
    n, cut = 2, 8
    cfg = dict(shift_semitones=-4.0, range=1.5, pivot=7.3, uv_threshold=0.1)
    a, slots, codes = _open(ctx, n)
    b = ctx.streams(MAX_SLOTS, 4, 64)
    # layout id and row size: those of a stream-set of the same shape that never heard of pitch
    lid, nbytes = b.layout_id, b.snapshot_bytes
    assert (a.layout_id, a.snapshot_bytes) == (lid, nbytes)
    a.set_pitch([slots[0]], cfg)
    assert (a.layout_id, a.snapshot_bytes) == (lid, nbytes)
    want, _ = _run(a, slots, codes, 4, False)                 # the uninterrupted run
    a.reset(slots, which=2)
    _run(a, slots, codes, 4, False, cut)
    snap = a.export_slots(slots)
    assert snap.info(0)["pitch"] == P.f32_cfg(cfg) and snap.info(1)["pitch"] is None
    out = _lib.PitchCfg()
    rec = _lib.SlotMeta.from_buffer_copy(snap.meta[:_lib.SLOT_META_BYTES])
    assert _lib.lib().conan_slot_meta_pitch(C.byref(rec), C.byref(out)) == 1
    assert (out.enabled, out.shift_semitones, out.range, out.reserved) == (1, -4.0, 1.5, 0)
    # into other slots of the second stream-set; the destination of the record without a cfg had one: it goes off
    dst = [2, 5]
    b.set_pitch([dst[1]], shift_semitones=7.0)
    b.import_slots(dst, snap.cpu().to("cuda"))
    assert b.pitch(dst) == [P.f32_cfg(cfg), None] and b.pitch_cfgs == {dst[0]: P.f32_cfg(cfg)}
    assert (b.layout_id, b.snapshot_bytes) == (lid, nbytes)
    got, _ = _run(b, dst, codes, 4, False, lo=cut)
    assert np.array_equal(got, want[:, cut:])
    a.close(); b.close()
