"""Source-pitch following on the GPU (conan_f0, conan_streams_set_pitch_follow, conan_step_wav_contour; include/conan_hip.h,
conan_f0_cfg): the tracker against tests/f0_ref.py, the streamed contour against the whole-signal one, the followed chunk steps
against the hand-composed path, and against themselves - neighbours keep their bits, pipelined equals blocking, live changes,
snapshots, errors.

conan_f0 against the reference.  uv and the picked lag are equal on every frame (tests/test_f0_ref_cpu.py shows that every decision
of these signals is at least 1e-6 from equality; the two sides' f64 sums differ by rounding in another order).  |delta log2 f0|:
both sides round an f64 log2 to f32, so they agree or differ by one f32 step of a value in [4, 16), 2^-20 = 9.5e-7 octave; measured on
the MI355X over all signals of f0_ref.gpu_signals(): 0 in every case (F0_MEASURED below) - the two sides landed on the same float on
every voiced frame.  The bound is 16 times the measured figure, never under that one f32 step, which is all the number format
promises, and never looser than 1e-4 octave (a hundredth of the narrowest f0_to_coarse bin)."""
import numpy as np
import pytest
import torch

from conan_amd import _lib
from conan_amd.engine import StreamingVoiceConversionEngine
from conan_amd.runtime import Context
from tests import f0_ref as R
from tests import pitch_ref as P
from tests.conftest import ARITHS
from tests.test_gpu_pitch import full  # noqa: F401  (module fixture: the small synthetic full model)

pytestmark = pytest.mark.gpu

HOP, SEG = 320, 4
L = SEG * HOP
MAX_SLOTS = 6
F0_MEASURED = 0.0            # largest |delta log2 f0| between conan_f0 and f0_ref on the MI355X (octaves)
F0_BOUND = min(1e-4, max(16 * F0_MEASURED, 2.0 ** -20))


def _wav(B, N, seed):
    return torch.from_numpy(R.sig(B, N, 16000, seed)).cuda()


def _ref(B, seed=3):
    from conan_amd import synth
    return torch.from_numpy(synth.mel(40, seed, B)).cuda()


def _open(full, slots, follow=None, pitch=None, arith="auto", dev_plan=None, seed=3):
    st = full.streams(MAX_SLOTS, 4, 64, arith=arith, dev_plan=dev_plan)
    st.reset(slots, which=15)
    st.set_reference(slots, _ref(len(slots), seed))
    for slot, fo in zip(slots, follow or []):
        if fo is not None:
            st.set_pitch_follow([slot], fo)
    for slot, pt in zip(slots, pitch or []):
        if pt is not None:
            st.set_pitch([slot], pt)
    return st


def _run(st, slots, wav, pipelined=False, contour=True, lin=L, on_call=None, mel=None):
    """The calls of infer_wav over wav [n, N] -> (codes, mel, wav, f0, uv) concatenated over the emitted chunks (f0 / uv: the contour
    hook per emitting call, blocking runs only) and the list of emits."""
    n, N = wav.shape
    last = (N - 1) // lin * lin
    calls = [(p, p + lin, False) for p in range(0, last, lin)] + [(last, N, True)]
    outs, emits, k = [], [], 0
    step = st.step_wav_async if pipelined else st.step_wav
    while True:
        if on_call:
            on_call(k)
        if calls:
            a, b, fin = calls.pop(0)
            e, c, m, w = step(slots, wav[:, a:b], final=fin, mel=mel)
        else:
            e, c, m, w = step(slots, wav[:, :0], final=True, mel=mel)
            if e == 0:
                break
        k += 1
        if e:
            f0 = uv = None
            if contour and not pipelined:
                f0, uv = st.step_wav_contour()
                assert not f0[:, e:].any() and not uv[:, e:].any()      # entries past the emitted frames are zero
                f0, uv = f0[:, :e].clone(), uv[:, :e].clone()
            outs.append((c[:, :e], m, w, f0, uv))
            emits.append(e)
    st.join()
    torch.cuda.synchronize()
    cat = [torch.cat([o[i] for o in outs], 1).clone() if outs[0][i] is not None else None for i in range(5)]
    return cat, emits


# ------------------------------------------------------------------------------------------------------------------ 1. the law

def _against_ref(ctx, names, **kw):
    sigs = R.gpu_signals()
    x = np.stack([sigs[k][0] for k in names])
    f0, uv = ctx.f0(torch.from_numpy(x).cuda(), **kw)
    f0, uv = f0.cpu().numpy(), uv.cpu().numpy()
    worst = 0.0
    for i, k in enumerate(names):
        r = R.judge(*[sigs[k][0]], **sigs[k][1])
        assert np.array_equal(uv[i], r["uv"].astype(np.float32)), k
        v = r["uv"] == 0
        assert (f0[i][~v] == 0).all(), k
        period = 16000.0 / np.exp2(f0[i][v].astype(np.float64))
        assert np.array_equal(np.rint(period - r["off"][v]).astype(np.int32), r["lag"][v]), k      # the picked lag
        if v.any():
            worst = max(worst, float(np.abs(f0[i][v].astype(np.float64) - r["v"][v].astype(np.float64)).max()))
    return worst


def test_conan_f0_against_the_reference(full):
    worst = [_against_ref(full, ["sig0", "sig1", "glide", "h220"]),
             _against_ref(full, ["short300"]),
             _against_ref(full, ["limits"], fmin=31.25, fmax=8000.0),
             _against_ref(full, ["n512"], fft_size=512, fmin=70.0)]
    print("max |delta log2 f0| per case (octaves):", worst)
    assert max(worst) <= F0_BOUND, worst
    # rows do not depend on what they share a launch with
    sigs = R.gpu_signals()
    x = torch.from_numpy(np.stack([sigs[k][0] for k in ("sig0", "sig1", "glide", "h220")])).cuda()
    a = full.f0(x)
    b = full.f0(x[2:3])
    assert torch.equal(a[0][2:3], b[0]) and torch.equal(a[1][2:3], b[1])


# ------------------------------------------------------------------------------------------------------------------ 2. streaming = whole signal

@pytest.mark.parametrize("N", [3 * L, 3 * L + 1, 2 * L + 319, 2 * L + 320, 700])
def test_streamed_contour_equals_conan_f0(full, N):
    slots = [4, 1]
    st = _open(full, slots, follow=[True, dict(threshold=0.1)])
    wav = _wav(2, N, 20 + N % 7)
    (_, _, _, f0, uv), emits = _run(st, slots, wav)
    w0, u0 = full.f0(wav[0:1])
    w1, u1 = full.f0(wav[1:2], threshold=0.1)
    assert sum(emits) == 1 + N // HOP
    assert torch.equal(f0, torch.cat([w0, w1])) and torch.equal(uv, torch.cat([u0, u1])), N
    assert N < L or int((uv == 0).sum()) >= f0.numel() // 2      # (a contour of nothing but unvoiced frames would show little)
    st.close()


def _ragged(st, slots, wavs, starts, pipelined=False, contour=True):
    """Utterances wavs[i] in slots[i] from tick starts[i] on, one step_wav_ragged call per tick over the live slots -> per
    utterance (codes, mel, wav, f0, uv) over its emitted frames."""
    U = len(slots)
    pos, fin, done = [0] * U, [False] * U, [False] * U
    outs = [[] for _ in range(U)]
    tick = 0
    step = st.step_wav_ragged_async if pipelined else st.step_wav_ragged
    while not all(done):
        live = [u for u in range(U) if starts[u] <= tick and not done[u]]
        tick += 1
        if not live:
            continue
        rows = torch.zeros(len(live), L, device="cuda")
        samples, final = [], []
        for r, u in enumerate(live):
            N = wavs[u].shape[0]
            last = (N - 1) // L * L
            if pos[u] < last:
                rows[r] = wavs[u][pos[u]:pos[u] + L]; samples.append(L); final.append(False); pos[u] += L
            else:
                k = N - pos[u]
                rows[r, :k] = wavs[u][pos[u]:]; samples.append(k); final.append(True); pos[u] = N
        was_final = [fin[u] for u in live]
        emit, c, m, w = step([slots[u] for u in live], rows, samples, final)
        if contour and not pipelined:
            f0, uv = st.step_wav_contour()
        for r, u in enumerate(live):
            e = emit[r]
            fin[u] = fin[u] or final[r]
            if was_final[r] and e == 0:
                done[u] = True
            if e:
                outs[u].append((c[r, :e], m[r, :e], w[r, :e * HOP], f0[r, :e].clone() if contour and not pipelined else None,
                                uv[r, :e].clone() if contour and not pipelined else None))
    st.join()
    torch.cuda.synchronize()
    return [[torch.cat([o[i] for o in out]).clone() if out[0][i] is not None else None for i in range(5)] for out in outs]


def test_ragged_contour_equals_conan_f0(full):
    slots, starts = [5, 0, 2], [0, 1, 3]
    wavs = [_wav(1, n, 30 + i)[0] for i, n in enumerate((4 * L + 333, 3 * L, 2 * L + 1))]
    st = _open(full, slots, follow=[True, True, True])
    got = _ragged(st, slots, wavs, starts)
    for u, x in enumerate(wavs):
        f0, uv = full.f0(x[None])
        assert torch.equal(got[u][3], f0[0]) and torch.equal(got[u][4], uv[0]), u
    st.close()


@pytest.mark.parametrize("rate", [8000, 48000])
def test_contour_is_of_the_levelled_resampled_samples(full, rate):
    slots = [3, 2]
    st = _open(full, slots, follow=[True, True])
    st.set_input_rate(slots, rate)
    st.set_input_level(slots, target=-26.0)
    lin = L * rate // 16000
    N = 3 * lin + 41
    wav = torch.from_numpy(R.sig(2, N, rate, 41)).cuda()
    (_, _, _, f0, uv), _ = _run(st, slots, wav, lin=lin)
    x = full.level(full.resample(wav, rate, 16000), target=-26.0)
    w, u = full.f0(x)
    assert torch.equal(f0, w) and torch.equal(uv, u)
    st.close()


# ------------------------------------------------------------------------------------------------------------------ 3. the whole path

def _composed(full, slots, wav, pitch, arith, dev_plan, fkw):
    """wav2mel chunk -> emformer_step -> decoder_step(f0=, uv=) fed conan_f0's contour -> hifigan_step, on a stream-set that never
    heard of following."""
    st = _open(full, slots, pitch=pitch, arith=arith, dev_plan=dev_plan)
    whole = full.wav2mel(wav)
    f0, uv = full.f0(wav, **fkw)
    cs, ms, ws = [], [], []
    for pos, emit, chunk in StreamingVoiceConversionEngine.chunks(st, whole):      # (chunks reads .seg and .rc only)
        _, _, codes = st.emformer_step(slots, chunk, want_out=False, want_logits=False)
        m = st.decoder_step(slots, codes[:, :emit], f0=f0[:, pos:pos + emit], uv=uv[:, pos:pos + emit])
        ws.append(st.hifigan_step(slots, m))
        cs.append(codes[:, :emit]); ms.append(m)
    torch.cuda.synchronize()
    out = torch.cat(cs, 1).clone(), torch.cat(ms, 1).clone(), torch.cat(ws, 1).clone()
    st.close()
    return out


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("form", ["single_tile", "multi_tile", "separate"])
def test_followed_steps_equal_the_hand_composed_path(full, arith, form):
    slots = {"single_tile": [4, 1], "multi_tile": [5, 0, 3, 1, 4, 2], "separate": [4, 1]}[form]
    dev_plan = "DEC_MEGA=0" if form == "separate" else None
    n = len(slots)
    wav = _wav(n, 3 * L + 500, 50)
    fkw = dict(threshold=0.2)
    for pitch in (None, dict(shift_semitones=3.0, range=0.5)):
        st = _open(full, slots, follow=[fkw] * n, pitch=[pitch] * n, arith=arith, dev_plan=dev_plan)
        (c, m, w, _, uv), _ = _run(st, slots, wav)
        st.close()
        c0, m0, w0 = _composed(full, slots, wav, [pitch] * n, arith, dev_plan, fkw)
        assert torch.equal(c, c0) and torch.equal(m, m0) and torch.equal(w, w0), (arith, form, pitch)
        assert int((uv == 0).sum()) >= uv.numel() // 2
    # and following changes the mel: the predictor's path of the same stream-set shape
    st = _open(full, slots, arith=arith, dev_plan=dev_plan)
    (_, mp, _, _, _), _ = _run(st, slots, wav, contour=False)
    st.close()
    assert not torch.equal(mp, m0)


# ------------------------------------------------------------------------------------------------------------------ 4. neighbours

def _launches(st, fn):
    st.profile_begin()
    out = fn()
    st.profile_end()
    return out, {k[0]: k[3] for k in st.profile_kernels()}


def test_neighbours_keep_their_bits_and_launches(full):
    slots = [0, 1, 2, 3]
    pt = dict(shift_semitones=-2.0, range=1.5)
    pitch = [None, None, pt, pt]
    wav = _wav(4, 3 * L + 77, 60)
    a = _open(full, slots, follow=[True, None, True, None], pitch=pitch)
    b = _open(full, slots, pitch=pitch)
    bytes_never = b.state_bytes
    assert a.state_bytes == bytes_never + 4 * 2 * MAX_SLOTS * SEG * 4      # the contour sets, from the first enabling call on
    ((ca, ma, wa, f0, uv), emits), la = _launches(a, lambda: _run(a, slots, wav, contour=False))
    ((cb, mb, wb, _, _), _), lb = _launches(b, lambda: _run(b, slots, wav, contour=False))
    assert torch.equal(ca, cb)
    for i in (1, 3):
        assert torch.equal(ma[i], mb[i]) and torch.equal(wa[i], wb[i]), i
    for i in (0, 2):
        assert not torch.equal(ma[i], mb[i]), i
    # one more launch per call that emits, and nothing else; a stream-set that never enabled following runs no tracker
    assert "f0_yin_kernel" not in lb
    assert la.pop("f0_yin_kernel") == len(emits)
    assert la == lb, (la, lb)
    # following off again: the launches of the stream-set that never followed
    a.set_pitch_follow(slots, None)
    assert a.pitch_follow(slots) == [None] * 4
    a.reset(slots, which=15)
    a.set_reference(slots, _ref(4))
    ((_, m2, w2, _, _), _), l2 = _launches(a, lambda: _run(a, slots, wav, contour=False))
    assert l2 == lb and torch.equal(m2, mb) and torch.equal(w2, wb)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------ 5. pipelined = blocking

def test_pipelined_equals_blocking(full):
    slots = [2, 5]
    wav = _wav(2, 13 * L + 77, 70)
    st = _open(full, slots, follow=[True, dict(threshold=0.1)], pitch=[None, dict(shift_semitones=2.0)])
    (cb, mb, wb, _, _), eb = _run(st, slots, wav, contour=False)
    assert len(eb) >= 12
    st.reset(slots, which=15)
    st.set_reference(slots, _ref(2))
    (cp, mp, wp, _, _), ep = _run(st, slots, wav, pipelined=True)
    assert ep == eb and torch.equal(cp, cb) and torch.equal(mp, mb) and torch.equal(wp, wb)
    st.close()


def test_pipelined_ragged_equals_blocking(full):
    slots, starts = [5, 0, 2], [0, 2, 5]
    wavs = [_wav(1, n, 80 + i)[0] for i, n in enumerate((13 * L + 5, 12 * L, 9 * L + 400))]
    outs = []
    for pipelined in (False, True):
        st = _open(full, slots, follow=[True, None, True])
        outs.append(_ragged(st, slots, wavs, starts, pipelined=pipelined, contour=False))
        st.close()
    for u in range(3):
        for i in range(3):
            assert torch.equal(outs[0][u][i], outs[1][u][i]), (u, i)


def test_engine_follow_keyword(full):
    """follow= on the engine: infer_wav blocking and pipelined give the bits of the step_wav loop with the setter called by hand;
    infer_wav_staggered takes one value per utterance; engine.set_pitch_follow turns it off again."""
    B = 2
    wav = _wav(B, 5 * L + 200, 75)
    st = _open(full, [0, 1], follow=[dict(threshold=0.1)] * B)
    (c0, m0, w0, _, _), _ = _run(st, [0, 1], wav, contour=False)
    st.close()
    eng = StreamingVoiceConversionEngine(full, B, max_ref_frames=64)
    for pipelined in (False, True):
        w, m, c = eng.infer_wav(wav, _ref(B), pipelined=pipelined, follow=dict(threshold=0.1))
        torch.cuda.synchronize()
        assert torch.equal(c, c0) and torch.equal(m, m0) and torch.equal(w, w0), pipelined
    assert eng.st.pitch_follow(eng.slots) == [_lib.f0_keywords(_lib.f0_cfg(threshold=0.1))] * B
    outs = eng.infer_wav_staggered([wav[0], wav[1]], [0, 2], _ref(B), pipelined=False, follow=[dict(threshold=0.1), None])
    assert eng.st.pitch_follow(eng.slots) == [_lib.f0_keywords(_lib.f0_cfg(threshold=0.1)), None]
    eng.set_pitch_follow(cfg=None)
    assert eng.st.pitch_follow(eng.slots) == [None] * B
    plain = eng.infer_wav_staggered([wav[0], wav[1]], [0, 2], _ref(B), pipelined=False)
    torch.cuda.synchronize()
    assert not torch.equal(outs[0][1], plain[0][1])                                              # the following utterance
    assert all(torch.equal(x, y) for x, y in zip(outs[1], plain[1]))                             # its neighbour keeps its bits
    eng.st.close()


# ------------------------------------------------------------------------------------------------------------------ 6. live changes

def test_live_changes_take_effect_at_the_next_emitted_chunk(full):
    slots = [1, 3]
    wav = _wav(2, 9 * L + 10, 90)
    w_def = full.f0(wav)
    w_thr = full.f0(wav, threshold=0.02)
    assert not torch.equal(w_def[1], w_thr[1])
    plain = _open(full, slots)
    (_, mp, _, _, _), _ = _run(plain, slots, wav, contour=False)
    plain.close()
    st = _open(full, slots)

    def on_call(k):      # before call k (call k emits chunk k - 1)
        if k == 3:
            st.set_pitch_follow(slots)                       # mid-utterance
        elif k == 5:
            st.set_pitch_follow(slots, None)
        elif k == 7:
            st.set_pitch_follow(slots, threshold=0.02)

    (_, m, _, f0, uv), emits = _run(st, slots, wav, on_call=on_call)
    fr = lambda c0, c1: slice(c0 * SEG, c1 * SEG)      # frames of chunks [c0, c1)
    z = torch.zeros_like(f0)
    assert torch.equal(f0[:, fr(0, 2)], z[:, fr(0, 2)]) and torch.equal(uv[:, fr(0, 2)], z[:, fr(0, 2)])      # rows that do not follow read 0, 0
    assert torch.equal(f0[:, fr(2, 4)], w_def[0][:, fr(2, 4)]) and torch.equal(uv[:, fr(2, 4)], w_def[1][:, fr(2, 4)])
    assert torch.equal(f0[:, fr(4, 6)], z[:, fr(4, 6)])
    assert torch.equal(f0[:, 6 * SEG:], w_thr[0][:, 6 * SEG:]) and torch.equal(uv[:, 6 * SEG:], w_thr[1][:, 6 * SEG:])
    assert torch.equal(m[:, fr(0, 2)], mp[:, fr(0, 2)]) and not torch.equal(m[:, fr(2, 3)], mp[:, fr(2, 3)])
    # a caller contour wins over following: decoder_step(f0=) of a following slot against a stream-set that never followed
    st.set_pitch_follow(slots)
    other = _open(full, slots)
    codes = (torch.arange(8, device="cuda", dtype=torch.int32).reshape(2, 4) * 7) % 50
    cf0 = torch.full((2, 4), 7.7, device="cuda")
    for s_ in (st, other):
        s_.reset(slots, which=2)
    assert torch.equal(st.decoder_step(slots, codes, f0=cf0), other.decoder_step(slots, codes, f0=cf0))
    assert torch.equal(st.decoder_step(slots, codes), other.decoder_step(slots, codes))      # and the mel-in steps keep the predictor's path
    st.close(); other.close()


# ------------------------------------------------------------------------------------------------------------------ 7. snapshots

def test_a_following_stream_continues_bit_for_bit_after_a_snapshot(full):
    slots, dst = [1, 4], [3, 0]
    wav = _wav(2, 7 * L + 123, 100)
    fkw = dict(threshold=0.1)
    a = _open(full, slots, follow=[fkw, fkw])
    (cw, mw, ww, f0w, uvw), emits = _run(a, slots, wav)
    a.reset(slots, which=15)
    a.set_reference(slots, _ref(2))
    cut = 4      # calls before the export: chunks 0 .. 2 are out
    b = full.streams(MAX_SLOTS, 4, 64)
    b.set_pitch_follow([dst[0]], fkw)      # the second destination stays off
    lid, nbytes = b.layout_id, b.snapshot_bytes
    assert (a.layout_id, a.snapshot_bytes) == (lid, nbytes)
    for k in range(cut):
        a.step_wav(slots, wav[:, k * L:(k + 1) * L])
    snap = a.export_slots(slots)
    b.import_slots(dst, snap)
    assert b.pitch_follow(dst) == [_lib.f0_keywords(_lib.f0_cfg(**fkw)), None]      # import leaves the destination's setting alone
    (c, m, w, f0, uv), _ = _run_from(b, dst, wav, cut)
    done = (cut - 1) * SEG
    assert torch.equal(c[0], cw[0, done:]) and torch.equal(m[0], mw[0, done:]) and torch.equal(w[0], ww[0, done * HOP:])
    assert torch.equal(f0[0], f0w[0, done:]) and torch.equal(uv[0], uvw[0, done:])
    # into a slot with following off: the predictor's path (documented), the contour hook reads zeros
    assert not f0[1].any() and not uv[1].any() and not torch.equal(m[1], mw[1, done:])
    a.close(); b.close()


def _run_from(st, slots, wav, first_call):
    """_run's calls from call `first_call` on (the earlier ones were made elsewhere)."""
    n, N = wav.shape
    last = (N - 1) // L * L
    calls = [(p, p + L, False) for p in range(0, last, L)] + [(last, N, True)]
    calls = calls[first_call:]
    outs = []
    while True:
        if calls:
            a, b, fin = calls.pop(0)
            e, c, m, w = st.step_wav(slots, wav[:, a:b], final=fin)
        else:
            e, c, m, w = st.step_wav(slots, wav[:, :0], final=True)
            if e == 0:
                break
        if e:
            f0, uv = st.step_wav_contour()
            outs.append((c[:, :e].clone(), m.clone(), w.clone(), f0[:, :e].clone(), uv[:, :e].clone()))
    torch.cuda.synchronize()
    return [torch.cat([o[i] for o in outs], 1) for i in range(5)], None


# ------------------------------------------------------------------------------------------------------------------ 8. errors

def test_errors_change_nothing(full):
    slots = [0, 2]
    st = _open(full, slots, follow=[True, None])
    before = st.pitch_follow(range(MAX_SLOTS))
    for bad in (dict(fmin=900.0, fmax=100.0), dict(threshold=1.5), dict(fmax=9000.0), dict(fmin=10.0)):
        with pytest.raises(_lib.ConanError) as e:
            st.set_pitch_follow([2, 3], **bad)
        assert e.value.code == _lib.ERR_INVALID
    for bad_slots in ([2, 2], [1, MAX_SLOTS], [-1]):
        with pytest.raises(_lib.ConanError) as e:
            st.set_pitch_follow(bad_slots)
        assert e.value.code == _lib.ERR_INVALID
    assert st.pitch_follow(range(MAX_SLOTS)) == before
    with pytest.raises(_lib.ConanError) as e:      # no wav-in call yet
        st.step_wav_contour()
    assert e.value.code == _lib.ERR_STATE
    # a frame too short for the cfg's lowest pitch: refused by the step, before anything changes
    wav = _wav(2, L, 110)
    with pytest.raises(_lib.ConanError) as e:
        st.step_wav(slots, wav, mel=dict(fft_size=512, win_length=512))
    assert e.value.code == _lib.ERR_INVALID
    # a frame whose chunk has left the audio ring when it is emitted
    big = dict(fft_size=2048, win_length=2048)
    with pytest.raises(_lib.ConanError) as e:
        for k in range(6):
            st.step_wav(slots, _wav(2, L, 111 + k), mel=big)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    st.close()
    # a stream-set without the streaming front-end
    hp, sd_np, _ = P.model()
    c = Context(hp, None, 0, emformer=False, conan=True, hifigan=False)
    c.load_state_dict("conan", sd_np)
    c.finalize()
    dec = c.streams(2, 4, 64)
    with pytest.raises(_lib.ConanError) as e:
        dec.set_pitch_follow([0])
    assert e.value.code == _lib.ERR_STATE
    dec.close()
    c.close()
