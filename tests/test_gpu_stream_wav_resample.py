"""Input sample rates other than the model rate (conan_resample, conan_streams_set_input_rate, conan_step_wav_ragged_ld) on the GPU:
the whole-signal resampler within the rigorous f32 bound of the float64 restatement, streaming input at a rate bit-identical to
infer_wav of the whole signal resampled, one resample_stream_kernel launch per call that needs one (none on stream-sets that never
set a rate), mixed rates in ragged calls, atomic errors, resets, and file input at another rate."""
import ctypes as C
import wave

import numpy as np
import pytest
import torch

from conan_amd import _lib, synth
from conan_amd.engine import StreamingVoiceConversionEngine
from conan_amd.runtime import mel_cfg
from tests import resample_ref
from tests.conftest import ARITHS
from tests.wav_helpers import HOP, L, SEG, _equal, _lin, _ref, _run_manual_at_rate, _sig, _staggered_in_rates, ctx  # noqa: F401  (ctx: module fixture)

pytestmark = pytest.mark.gpu

FIXED = _lib.STREAMS_FIXED_PLAN
RS = "resample_stream_kernel"
PRESET_ARGS = {"hann": (6, 0.99, "hann", None), "kaiser_best": (64, 0.9475937167399596, "kaiser", None)}


# ---- 1. whole signals against float64
WHOLE = [(8000, 16000), (11025, 16000), (22050, 16000), (44100, 16000), (48000, 16000), (96000, 16000), (16000, 48000), (16000, 44100)]


@pytest.mark.parametrize("rates", WHOLE, ids=lambda r: "%d-%d" % r)
@pytest.mark.parametrize("preset", ["hann", "kaiser_best"])
def test_whole_signal_against_float64(ctx, rates, preset):
    r_in, r_out = rates
    orig, _ = resample_ref.reduce(r_in, r_out)
    lengths = sorted({1, max(1, orig - 1), 3 * orig + 7, 1237, 10 * r_in})
    for N in lengths:
        for n in ((1, 8) if N < 10 * r_in else (1,)):
            x = _sig(n, N, r_in, N + n)
            y = ctx.resample(x, r_in, r_out, preset=preset)
            want, abs_sum, K = resample_ref.resample(x.cpu().double().numpy(), r_in, r_out, *PRESET_ARGS[preset])
            assert y.shape == (n, resample_ref.length(r_in, r_out, N))
            err = np.abs(y.cpu().double().numpy() - want)
            bnd = resample_ref.bound(abs_sum, K[None])
            assert (err <= bnd).all(), (rates, preset, N, n, float((err - bnd).max()))


def test_same_rate_is_a_copy(ctx):
    x = _sig(3, 5001, 16000, 1)
    assert torch.equal(ctx.resample(x, 16000, 16000), x)
    assert torch.equal(ctx.resample(x[0], 16000, 16000, preset="kaiser_best"), x[0])


# ---- 2. streaming input at a rate = infer_wav of the whole signal resampled, bit for bit
def _stream_cases():
    out = []
    for rate in (8000, 22050, 44100, 48000):
        for preset in ("hann", "kaiser_best"):
            ariths = ARITHS if (rate, preset) == (48000, "hann") else ARITHS[:1]
            for arith in ariths:
                out.append((rate, preset, arith))
    return out


@pytest.mark.parametrize("rate,preset,arith", _stream_cases())
def test_stream_equals_whole_signal(ctx, rate, preset, arith):
    Li = _lin(rate)
    for B in (1, 4, 64):
        if B == 64 and (rate, preset) != (48000, "hann"):
            continue
        eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64, arith=arith)
        ref = _ref(B)
        lengths = (Li // 2, Li, 2 * Li + 1, 3 * rate + 17) if B < 64 else (Li - 1, 2 * rate + 5)
        for j, N in enumerate(lengths):
            src = _sig(B, N, rate, 40 + j)
            for pipelined in (False, True):
                got = eng.infer_wav(src, ref, pipelined=pipelined, in_rate=rate, preset=preset)
                want = eng.infer_wav(ctx.resample(src, rate, preset=preset), ref, pipelined=pipelined)
                torch.cuda.synchronize()
                assert _equal(got, want), (rate, preset, arith, B, N, pipelined)


def _feed_emits(eng, src, rate=None, preset="hann"):
    """Emit count per call of a blocking feed loop (drain included) and the resample launches per call."""
    eng.start_wav(_ref(src.shape[0]), in_rate=rate, preset=preset)
    Li = _lin(rate or 16000)
    N = src.shape[1]
    last = (N - 1) // Li * Li
    emits, launches, pos, fin = [], [], 0, False
    while True:
        eng.st.profile_begin()
        done = False
        if pos < last:
            e, _, _, _ = eng.st.step_wav(eng.slots, src[:, pos:pos + Li])
            pos += Li
        else:
            e, _, _, _ = eng.st.step_wav(eng.slots, src[:, pos:] if not fin else src[:, :0], final=True)
            pos, done, fin = N, fin and e == 0, True
        eng.st.profile_end()
        launches.append(sum(k[3] for k in eng.st.profile_kernels() if k[0] == RS))
        emits.append(e)
        if done:
            return emits, launches


@pytest.mark.parametrize("rate", [8000, 22050, 44100, 48000])
@pytest.mark.parametrize("preset", ["hann", "kaiser_best"])
def test_emit_schedule_and_launches(ctx, rate, preset):
    """Every call with samples emits what the model-rate run of the resampled signal emits at that call; at most one more drain
    call.  Calls with samples or a remainder make one resample_stream_kernel launch, the others none."""
    eng = StreamingVoiceConversionEngine(ctx, 1, max_ref_frames=64)
    plain = StreamingVoiceConversionEngine(ctx, 1, max_ref_frames=64)
    Li = _lin(rate)
    for j, N in enumerate((Li // 3, Li, 3 * Li - 1, 3 * Li + 1, 5 * rate + 3)):
        src = _sig(1, N, rate, 70 + j)
        e_r, l_r = _feed_emits(eng, src, rate, preset)
        e_m, l_m = _feed_emits(plain, ctx.resample(src, rate, preset=preset))
        n_in = (N - 1) // Li + 1
        assert e_r[:n_in] == e_m[:n_in], (rate, preset, N, e_r, e_m)
        assert len(e_m) <= len(e_r) <= len(e_m) + 1, (e_r, e_m)
        assert sum(e_r) == sum(e_m)
        assert l_m == [0] * len(l_m)
        assert l_r[:n_in] == [1] * n_in
        assert all(x in (0, 1) for x in l_r[n_in:]) and l_r[-1] == 0


def test_set_without_rate_launches_as_before(ctx):
    """A stream-set that never sets a rate makes no resample launch and keeps its state size; its kernels are those of a set that
    sets the model rate (in_rate == out_rate: the model-rate path)."""
    a = StreamingVoiceConversionEngine(ctx, 2, max_ref_frames=64)
    b = StreamingVoiceConversionEngine(ctx, 2, max_ref_frames=64)
    bytes0 = a.st.state_bytes
    src = _sig(2, 3 * L + 11, 16000, 5)

    def kernels(eng, rate):
        eng.st.profile_begin()
        out = eng.infer_wav(src, _ref(2), pipelined=False, in_rate=rate)
        eng.st.profile_end()
        return out, {k[0]: k[3] for k in eng.st.profile_kernels()}

    wa, ka = kernels(a, None)
    wb, kb = kernels(b, 16000)
    assert RS not in ka and RS not in kb
    assert ka == kb and _equal(wa, wb)
    assert a.st.state_bytes == bytes0 and not a.st.input_rate_set
    assert b.st.state_bytes == bytes0 + 2 * 32768 * 4


# ---- 4. ragged calls mixing rates
@pytest.mark.parametrize("pipelined", [False, True])
def test_staggered_mixed_rates_equal_solo(ctx, pipelined):
    U, B = 72, 64
    rates, srcs, starts = _staggered_in_rates(U, 11)
    refs = _ref(U, 5)
    eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64, flags=FIXED)
    outs = eng.infer_wav_staggered(srcs, starts, refs, pipelined=pipelined, in_rates=rates)
    torch.cuda.synchronize()
    used = eng.staggered_slots
    reused = {}
    for u, s in enumerate(used):
        reused.setdefault(s, []).append(rates[u])
    assert any(len(set(v)) > 1 for v in reused.values()), "no slot was reused with another rate"
    solo = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64, flags=FIXED)
    for u in range(U):
        solo.slots = [used[u]]
        w, m, c = solo.infer_wav(srcs[u][None], refs[u][None], pipelined=False, in_rate=rates[u] if rates[u] != 16000 else None)
        torch.cuda.synchronize()
        assert _equal(outs[u], (w[0], m[0], c[0])), (u, rates[u], pipelined)


def test_mixed_rate_call_one_launch(ctx):
    eng = StreamingVoiceConversionEngine(ctx, 3, max_ref_frames=64)
    eng.open_slots([0, 1, 2], _ref(3), in_rate=[48000, 44100, None])
    width = _lin(48000)
    rows = torch.stack([torch.nn.functional.pad(_sig(1, _lin(r), r, 9 + i)[0], (0, width - _lin(r))) for i, r in enumerate((48000, 44100, 16000))])
    eng.st.profile_begin()
    eng.st.step_wav_ragged([0, 1, 2], rows, [_lin(48000), _lin(44100), L], [0, 0, 0])
    eng.st.profile_end()
    ks = {k[0]: k[3] for k in eng.st.profile_kernels()}
    assert ks.get(RS) == 1 and ks.get("mel_stream_ragged_kernel") == 1, ks


# ---- 5. errors leave every slot unchanged; resets
def test_errors_leave_slots_unchanged(ctx):
    rate, B = 48000, 2
    src = _sig(B, 3 * _lin(rate) + 101, rate, 21)
    ref = _ref(B)
    clean = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    clean.start_wav(ref, in_rate=rate)
    want = _run_manual_at_rate(clean, src, rate, "hann")

    eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    eng.start_wav(ref, in_rate=rate)
    lib, h = eng.st.lib, eng.st.h
    slots = (C.c_int32 * B)(*eng.slots)
    mc = mel_cfg()

    def expect(rc, code):
        assert rc == code, (rc, code, lib.conan_last_error())

    def hook(i):
        if i != 1:
            return
        bad_cfgs = [_lib.resample_cfg(44056), _lib.resample_cfg(rate, lowpass_filter_width=0), _lib.resample_cfg(rate, lowpass_filter_width=129),
                    _lib.resample_cfg(rate, rolloff=0.0), _lib.resample_cfg(rate, rolloff=1.5), _lib.resample_cfg(rate, 22050)]
        r = _lib.resample_cfg(rate)
        r.reserved[0] = 3
        for cfg in bad_cfgs + [r]:
            expect(lib.conan_streams_set_input_rate(h, slots, B, C.byref(cfg)), _lib.ERR_INVALID)
        # mid-utterance
        expect(lib.conan_streams_set_input_rate(h, slots, B, C.byref(_lib.resample_cfg(rate))), _lib.ERR_STATE)
        # the old ragged entry with a 48 kHz row
        Li = _lin(rate)
        wav = torch.zeros(B, Li, device="cuda")
        sm, fi, emit = (C.c_int32 * B)(Li, Li), (C.c_int32 * B)(0, 0), (C.c_int32 * B)()
        out = torch.empty(B, L, device="cuda")
        expect(lib.conan_step_wav_ragged(h, slots, B, sm, fi, C.c_void_p(wav.data_ptr()), C.byref(mc), None, None, C.c_void_p(out.data_ptr()),
                                         emit, None), _lib.ERR_INVALID)
        # a non-final call with the wrong sample count
        e = C.c_int32(0)
        expect(lib.conan_step_wav(h, slots, B, L, 0, C.c_void_p(wav.data_ptr()), C.byref(mc), None, None, C.c_void_p(out.data_ptr()),
                                  C.byref(e), None), _lib.ERR_INVALID)

    got = _run_manual_at_rate(eng, src, rate, "hann", hook)
    assert _equal(got, want)


def test_step_wav_mixed_rates_refused(ctx):
    eng = StreamingVoiceConversionEngine(ctx, 2, max_ref_frames=64)
    eng.start_wav(_ref(2))
    eng.st.set_input_rate([0], 48000)
    eng.st.set_input_rate([1], 48000, preset="kaiser_best")
    with pytest.raises(_lib.ConanError) as e:
        eng.st.step_wav([0, 1], _sig(2, _lin(48000), 48000, 1))
    assert e.value.code == _lib.ERR_INVALID
    eng.st.set_input_rate([1], 16000)
    with pytest.raises(_lib.ConanError) as e:
        eng.st.step_wav([0, 1], _sig(2, _lin(48000), 48000, 1))
    assert e.value.code == _lib.ERR_INVALID
    # nothing changed: both slots still take a set_input_rate (start of an utterance)
    eng.st.set_input_rate([0, 1], 44100)


@pytest.mark.parametrize("rate,preset", [(44100, "kaiser_best"), (8000, "hann")])
def test_reset_keeps_rate_and_clears_history(ctx, rate, preset):
    B = 2
    a, b = _sig(B, 2 * _lin(rate) + 77, rate, 31), _sig(B, 3 * _lin(rate) - 5, rate, 32)
    ref = _ref(B)
    eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    eng.start_wav(ref, in_rate=rate, preset=preset)
    _run_manual_at_rate(eng, a, rate, preset)
    eng.start(ref, which=7 | 8)                 # a reset with CONAN_MODEL_FRONTEND, no new set_input_rate
    got = _run_manual_at_rate(eng, b, rate, preset)
    fresh = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    fresh.start_wav(ref, in_rate=rate, preset=preset)
    assert _equal(got, _run_manual_at_rate(fresh, b, rate, preset))


def test_state_bytes(ctx):
    eng = StreamingVoiceConversionEngine(ctx, 5, max_ref_frames=64)
    b0 = eng.st.state_bytes
    eng.start_wav(_ref(5))
    assert eng.st.state_bytes == b0
    with pytest.raises(_lib.ConanError):
        eng.st.set_input_rate([0], 44056)
    assert eng.st.state_bytes == b0
    eng.st.set_input_rate([0], 48000)
    assert eng.st.state_bytes == b0 + 5 * 32768 * 4
    eng.st.set_input_rate([1, 2], 22050, preset="kaiser_best")
    assert eng.st.state_bytes == b0 + 5 * 32768 * 4


# ---- 6. file input at another rate
def test_file_input_resampled(ctx, tmp_path):
    from conan_amd import configs
    from conan_amd.inference.Conan import StreamingVoiceConversion
    from conan_amd.utils.audio import librosa_wav2spec, read_wav
    rng = np.random.default_rng(4)
    n = 44100 * 3 // 4
    x = (0.3 * np.sin(2 * np.pi * 220 * np.arange(n) / 44100) + 0.05 * rng.standard_normal(n)).clip(-1, 1)
    path = str(tmp_path / "src.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(44100)
        f.writeframes((x * 32767).astype("<i2").tobytes())
    samples, sr = read_wav(path)
    assert sr == 44100
    res = ctx.resample(torch.from_numpy(samples), 44100, 16000, preset="kaiser_best").cpu().numpy()
    a = librosa_wav2spec(path, sample_rate=16000, ctx=ctx)
    b = librosa_wav2spec(res, sample_rate=16000, ctx=ctx)
    assert np.array_equal(a["mel"], b["mel"]) and np.array_equal(a["wav"], b["wav"])
    chp, vhp = configs.conan_hparams(True), configs.hifigan_hparams(True)
    sds = {"emformer": synth.emformer_state_dict(chp, 0), "conan": synth.conan_state_dict(chp, 0), "hifigan": synth.hifigan_state_dict(vhp, 0)}
    vc = StreamingVoiceConversion(chp, vhp, sds)
    w1, m1 = vc.infer_once({"src_wav": path, "ref_wav": res})
    w2, m2 = vc.infer_once({"src_wav": vc.ctx.resample(torch.from_numpy(samples), 44100, 16000, preset="kaiser_best").cpu().numpy(), "ref_wav": res})
    assert np.array_equal(w1, w2) and np.array_equal(m1, m2)
