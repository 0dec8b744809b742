"""Streaming waveform input (conan_step_wav / conan_step_wav_async, StreamingVoiceConversionEngine.feed / infer_wav) on the GPU:
frames bit-identical to conan_wav2mel of the whole utterance, steps bit-identical to the mel-in loop fed those frames, the CPU
oracle's front-end + chunk loop within the loop tolerances, resets, argument errors, one mel_stream_kernel launch per call."""
import ctypes as C

import numpy as np
import pytest
import torch

from conan_amd import _lib, configs, synth
from conan_amd.engine import StreamingVoiceConversionEngine
from conan_amd.runtime import Context, mel_cfg
from tests.conftest import ARITHS

pytestmark = pytest.mark.gpu

HOP, SEG = 320, 4
L = SEG * HOP
# N % hop in {0, 1, hop - 1}, shorter than one chunk, exactly one chunk, a multiple of the chunk
LENGTHS = (7 * HOP, 9 * HOP + 1, 11 * HOP - 1, 700, L, 3 * L, 4 * L + 333)


@pytest.fixture(scope="module")
def ctx():
    chp, vhp = configs.conan_hparams(True), configs.hifigan_hparams(True)
    c = Context(chp, vhp, 0)
    c.load_state_dict("emformer", synth.emformer_state_dict(chp, 0))
    c.load_state_dict("conan", synth.conan_state_dict(chp, 0))
    c.load_state_dict("hifigan", synth.hifigan_state_dict(vhp, 0))
    c.finalize()
    assert c.hop == HOP and c.cfg.emf_segment == SEG
    yield c
    c.close()


def _wav(B, N, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(N) / 16000.0
    w = [0.3 * np.sin(2 * np.pi * (150 + 70 * i) * t) + 0.1 * np.sin(2 * np.pi * 2300 * t) + 0.05 * rng.standard_normal(N) for i in range(B)]
    return torch.from_numpy(np.stack(w).astype(np.float32)).cuda()


def _ref(B):
    return torch.from_numpy(synth.mel(40, 3, B)).cuda()


def _calls(N):
    """(samples slice start, stop, final) of the calls infer_wav makes, drain included."""
    last = (N - 1) // L * L
    out = [(p, p + L, False) for p in range(0, last, L)]
    return out + [(last, N, True)]


def _stream_frames(eng, wav, mel=None, pipelined=False):
    """One utterance [B, N] through step_wav (step_wav_async and a join per call when pipelined), drain included, on eng.slots (already
    started) -> (got: (emit, chunk) per emitting call, frames: the emitted rows of those chunks, first_emit, ncalls, fdone,
    with_frames, copy_only): the calls that completed frames / only copied, by the frames-complete rule of the configuration `mel`."""
    B, N = wav.shape
    half = (mel or {}).get("fft_size", 1024) // 2
    step = eng.st.step_wav_async if pipelined else eng.st.step_wav
    got, ncalls, frames = [], 0, []
    calls = _calls(N)
    drained = False
    recv, fdone, with_frames, copy_only = 0, 0, 0, 0
    while not drained:
        if calls:
            a, b, fin = calls.pop(0)
            emit, _, _, _ = step(eng.slots, wav[:, a:b], final=fin, mel=mel)
        else:
            a = b = N
            emit, _, _, _ = step(eng.slots, wav[:, :0], final=True, mel=mel)
            drained = emit == 0
        if pipelined:
            eng.st.join()
        recv += b - a
        fc = 1 + recv // HOP if fin else max(0, (recv - half) // HOP + 1)      # frames complete (half = fft_size / 2)
        with_frames += fc > fdone
        copy_only += fc <= fdone and ((b > a) or emit > 0)
        fdone = max(fdone, fc)
        ncalls += 1
        if ncalls == 1:
            first_emit = emit
        if emit:
            ch = eng.st.wav_chunk(B)
            got.append((emit, ch))
            frames.append(ch[:, :emit])
    return got, frames, first_emit, ncalls, fdone, with_frames, copy_only


@pytest.mark.parametrize("B", [1, 4, 64])
def test_frames_bitwise_equal_wav2mel(ctx, B):
    eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    for j, N in enumerate(LENGTHS if B < 64 else LENGTHS[:4]):
        wav = _wav(B, N, 10 + j)
        whole = ctx.wav2mel(wav)
        want = list(eng.chunks(whole))
        eng.start_wav(_ref(B))
        eng.st.profile_begin()
        got, frames, first_emit, ncalls, fdone, with_frames, copy_only = _stream_frames(eng, wav)
        eng.st.profile_end()
        launches = {k[0]: k[3] for k in eng.st.profile_kernels()}
        assert len(got) == len(want), (N, len(got), len(want))
        for (emit, ch), (_, emit_w, ch_w) in zip(got, want):
            assert emit == emit_w and torch.equal(ch, ch_w), N
        assert torch.equal(torch.cat(frames, 1), whole), N
        # one mel_stream_kernel launch per call that completes frames; drain calls that complete none but emit a chunk launch the
        # copy kernel alone; the drain's empty answer launches nothing
        assert fdone == whole.shape[1] and with_frames >= 1
        assert launches.get("mel_stream_kernel") == with_frames, (N, launches, with_frames)
        assert launches.get("mel_stream_copy_kernel", 0) == copy_only == ncalls - 1 - with_frames, (N, launches, copy_only)
        # the first call emits nothing when more audio follows: one chunk of algorithmic latency
        assert (first_emit == 0) == (N > L), (N, first_emit)
    eng.st.close()


def test_frames_natural_log_and_mag_eps(ctx):
    """conan_mel_cfg.natural_log / mag_eps with centred framing: the streamed frames are conan_wav2mel's with the same
    configuration, bit for bit (ln instead of log10, sqrt(. + mag_eps) magnitudes)."""
    B = 4
    eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    for kw in (dict(natural_log=True, mel_vmin=-13.0, mel_vmax=3.0), dict(natural_log=True, mag_eps=1e-9, mel_vmin=-1e30, mel_vmax=1e30)):
        for j, N in enumerate((3 * L + 1, 11 * HOP - 1)):
            wav = _wav(B, N, 40 + j)
            whole = ctx.wav2mel(wav, **kw)
            assert not torch.equal(whole, ctx.wav2mel(wav))
            eng.start_wav(_ref(B))
            frames, calls, fin = [], _calls(N), False
            while True:
                if calls:
                    a, b, fin = calls.pop(0)
                    emit, _, _, _ = eng.st.step_wav(eng.slots, wav[:, a:b], final=fin, mel=kw)
                else:
                    emit, _, _, _ = eng.st.step_wav(eng.slots, wav[:, :0], final=True, mel=kw)
                    if emit == 0:
                        break
                if emit:
                    frames.append(eng.st.wav_chunk(B)[:, :emit])
            assert torch.equal(torch.cat(frames, 1), whole), (kw, N)
    eng.st.close()


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("B", [1, 4, 64])
def test_infer_wav_bitwise_equal_mel_loop(ctx, arith, B):
    eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64, arith=arith)
    N = 9 * HOP + 1 if B == 64 else 3 * L + 1
    wav, ref = _wav(B, N, B), _ref(B)
    whole = ctx.wav2mel(wav)
    w0, m0, c0 = eng.infer(whole, ref, pipelined=False)
    for pipelined in (False, True):
        w, m, c = eng.infer_wav(wav, ref, pipelined=pipelined)
        torch.cuda.synchronize()
        assert torch.equal(c, c0) and torch.equal(m, m0) and torch.equal(w, w0), (arith, B, pipelined)
    eng.st.close()


def test_infer_wav_fixed_plan_one_slot_of_64(ctx):
    eng = StreamingVoiceConversionEngine(ctx, 64, max_ref_frames=64, flags=_lib.STREAMS_FIXED_PLAN)
    eng.slots = [37]
    wav, ref = _wav(1, 2 * L + HOP - 1, 5), _ref(1)
    w0, m0, c0 = eng.infer(ctx.wav2mel(wav), ref, pipelined=False)
    for pipelined in (False, True):
        w, m, c = eng.infer_wav(wav, ref, pipelined=pipelined)
        torch.cuda.synchronize()
        assert torch.equal(c, c0) and torch.equal(m, m0) and torch.equal(w, w0)
    eng.st.close()


@pytest.mark.parametrize("B", [1, 48])
def test_infer_wav_matches_oracle(ctx, B):
    """Oracle front-end (oracle/frontend.py) then the oracle chunk loop (oracle/loop.py), per stream (all of them at 1 slot, the
    first 4 at 48).  The front-ends agree to 1e-5 (tests/test_gpu_api.py), not bit for bit, so the full oracle chain's codes - argmaxes
    of logits computed from those frames - must agree with the GPU's on >= 95 % of the frames.  The 1e-4 mel / wav tolerance of
    smoke() is then checked for the oracle DECODING THE GPU'S CODES (codes_override), not for the full chain."""
    from oracle import emformer as oemf
    from oracle import frontend as ofe
    from oracle import loop as oloop
    from oracle.common import to_torch_sd
    chp, vhp = configs.conan_hparams(True), configs.hifigan_hparams(True)
    sds = {"emformer": synth.emformer_state_dict(chp, 0), "conan": synth.conan_state_dict(chp, 0), "hifigan": synth.hifigan_state_dict(vhp, 0)}
    tsd = {k: to_torch_sd(v) for k, v in sds.items()}
    eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    N = 2 * L + 517
    wav, ref = _wav(B, N, 21), _ref(B)
    w, m, c = eng.infer_wav(wav, ref)
    torch.cuda.synchronize()
    w, m, c = w.cpu().numpy(), m.cpu().numpy(), c.cpu().numpy()
    cfg = oemf.EmformerCfg(chp)
    wn, rn = wav.cpu().numpy(), ref.cpu().numpy()
    for b in range(B if B == 1 else 4):
        src = ofe.wav2mel(wn[b])
        assert m.shape[1] == src.shape[0]
        _, _, c_ref = oloop.infer_once_stateful(tsd["emformer"], cfg, tsd["conan"], chp, tsd["hifigan"], vhp, src, rn[b])
        assert np.mean(c_ref == c[b]) >= 0.95
        w_ref, m_ref, _ = oloop.infer_once_stateful(tsd["emformer"], cfg, tsd["conan"], chp, tsd["hifigan"], vhp, src, rn[b], codes_override=c[b])
        np.testing.assert_allclose(m[b], m_ref, atol=1e-4, rtol=1e-4)
        np.testing.assert_allclose(w[b], w_ref, atol=1e-4, rtol=0)
    eng.st.close()


def test_reset_frontend_mid_utterance_and_neighbours(ctx):
    B = 4
    ref = _ref(B)
    a_wav, b_wav = _wav(B, 5 * L, 31), _wav(B, 3 * L + 77, 32)
    eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    eng.start_wav(ref)
    for k in range(3):
        eng.feed(a_wav[:, k * L:(k + 1) * L])
    got = eng.infer_wav(b_wav, ref)           # reset with CONAN_MODEL_FRONTEND inside, mid-utterance
    fresh = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    want = fresh.infer_wav(b_wav, ref)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    fresh.st.close()
    eng.st.close()
    # one slot reset while its neighbours go on (fixed plan: a slot's bits do not depend on who steps with it)
    f = _lib.STREAMS_FIXED_PLAN
    full = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64, flags=f)
    want = full.infer_wav(a_wav, ref, pipelined=False)
    split = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64, flags=f)
    split.start_wav(ref)
    outs = []
    nb = [0, 1, 3]
    for k in range(5):
        if k == 2:
            split.st.reset([2], which=15)
        sl = list(range(B)) if k < 2 else nb
        emit, c, m, w = split.st.step_wav(sl, a_wav[sl, k * L:(k + 1) * L])
        outs.append((sl, emit, c, m, w))
        if k >= 2:
            split.st.step_wav([2], b_wav[2:3, (k - 2) * L:(k - 1) * L])
    emit, c, m, w = split.st.step_wav(nb, a_wav[nb, :0], final=True)
    outs.append((nb, emit, c, m, w))
    while True:
        emit, c, m, w = split.st.step_wav(nb, a_wav[nb, :0], final=True)
        if emit == 0:
            break
        outs.append((nb, emit, c, m, w))
    wv = {s: [] for s in nb}
    for sl, emit, c, m, w in outs:
        for i, s in enumerate(sl):
            if s in wv and emit:
                wv[s].append(w[i])
    torch.cuda.synchronize()
    for i in nb:
        assert torch.equal(torch.cat(wv[i]), want[0][i]), i
    full.st.close()
    split.st.close()


def test_step_wav_errors(ctx):
    st = ctx.streams(4, 4, 64)
    lib = _lib.lib()
    slots = (C.c_int32 * 2)(0, 1)
    st.reset([0, 1], which=15)
    st.set_reference([0, 1], _ref(2))
    wav = torch.zeros(2, L, device="cuda")
    out = torch.empty(2, L, device="cuda")
    emit = C.c_int32(0)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(samples, final, mc):
        return lib.conan_step_wav(st.h, slots, 2, samples, final, C.c_void_p(wav.data_ptr()), C.byref(mc), None, None,
                                  C.c_void_p(out.data_ptr()), C.byref(emit), s)

    def err(rc, text):
        assert rc == _lib.ERR_INVALID, rc
        assert text in lib.conan_last_error().decode()

    err(call(L - 1, 0, mel_cfg()), "exactly segment * hop")
    err(call(L, 0, mel_cfg(framing=1)), "framing 0")
    err(call(L, 0, mel_cfg(fft_size=1000)), "power of two")
    err(call(L, 0, _lib.MelCfg(1024, 320, 1024, 80, 16000, 80.0, 7600.0, 1e-6, -6.0, 1.5, 0, 2, 0.0)), "natural_log")
    assert call(L, 0, mel_cfg()) == 0 and emit.value == 0
    assert call(L, 1, mel_cfg()) == 0 and emit.value == SEG
    err(call(L, 1, mel_cfg()), "only samples = 0")
    n = 0
    while True:
        assert call(0, 1, mel_cfg()) == 0
        if emit.value == 0:
            break
        n += 1
    assert n >= 1
    err(call(0, 1, mel_cfg()), "drained")
    # slots at different positions of their utterances
    st.reset([1], which=15)
    err(call(L, 0, mel_cfg()), "same position")
    torch.cuda.synchronize()
    st.close()
