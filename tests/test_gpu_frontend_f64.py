"""The mel front-end on the GPU across its configuration range (fft_size 64 .. 2048, windows shorter than the frame, 40 .. 512 mels,
0 .. Nyquist bands, both framings, ln / mag_eps):
  (a) conan_wav2mel (stft_frames_kernel -> dft_mag_kernel -> mel_log_kernel) within tests/frontend_ref.py's derived bound of its
      float64 reference, element by element;
  (b) the streaming kernels (mel_stream_kernel, mel_stream_copy_kernel, mel_stream_ragged_kernel) bit-identical to conan_wav2mel of the
      whole utterance at every accepted fft_size other than the default's, with their launch counts.
tests/test_frontend_ref_cpu.py pins the reference and shows that an emulation of the kernels' arithmetic stays inside the bound on
these inputs while three mutants of it leave it."""
import numpy as np
import pytest
import torch

from conan_amd import _lib
from conan_amd.engine import StreamingVoiceConversionEngine
from tests import frontend_ref as fr
from tests.test_gpu_stream_wav import HOP, L, _calls, _ref, _stream_frames, ctx  # noqa: F401  (ctx: module fixture)

pytestmark = pytest.mark.gpu

FIXED = _lib.STREAMS_FIXED_PLAN
WHOLE = fr.centred_cases() + fr.reflect_cases()


# ---- (a) the whole-signal path against float64
@pytest.mark.parametrize("name,p", WHOLE, ids=[c[0] for c in WHOLE])
def test_wav2mel_within_bound_of_float64(ctx, name, p):
    """n = 3 (broadband, tone, silence as the rows of one call) and n = 1 (the broadband row alone: the same bits) at every length;
    the shape follows conan_mel_frames; silence gives one value per filter in every frame - the device's log of the floor, the clip's
    lower edge exactly where the default clip is on."""
    worst, bad = 0.0, []
    for n in fr.lengths(p):
        sigs = np.stack([fr.signal(k, n, p["sample_rate"]) for k in fr.SIGNALS])
        got = ctx.wav2mel(torch.from_numpy(sigs).cuda(), **p).cpu().numpy()
        one = ctx.wav2mel(torch.from_numpy(sigs[:1]).cuda(), **p).cpu().numpy()
        assert got.shape == (3, fr.n_frames(p, n), p["num_mels"]) and one.shape == (1,) + got.shape[1:], (name, n, got.shape)
        assert np.array_equal(one[0], got[0]), (name, n)
        for i, kind in enumerate(fr.SIGNALS):
            ref = fr.case(p, n, kind)
            assert np.isfinite(got[i]).all(), (name, n, kind)
            r = np.abs(got[i].astype(np.float64) - ref["mel"]) / fr.bound(ref, p)
            print(f"frontend_f64 {name} n={n} {kind}: error / bound = {r.max():.4f}")
            worst = max(worst, float(r.max()))
            if r.max() > 1.0:
                bad.append((n, kind, float(r.max()), int((r > 1.0).sum())))
        sil = got[2]
        assert (sil == sil[:1]).all(), (name, n)
        if p["mag_eps"] == 0.0:
            assert (sil == sil[0, 0]).all(), (name, n)
            if p["mel_vmin"] > -1e29:
                assert sil[0, 0] == np.float32(p["mel_vmin"]), (name, n, sil[0, 0])
    print(f"frontend_f64 {name}: worst error / bound = {worst:.4f}")
    assert not bad, (name, bad)


def test_reflect_framing_refuses_signals_no_longer_than_the_padding(ctx):
    for _, p in fr.reflect_cases():
        pad = (p["fft_size"] - p["hop_size"]) // 2
        for n in (1, pad):
            with pytest.raises(_lib.ConanError) as e:
                ctx.wav2mel(torch.zeros(1, n, device="cuda"), **p)
            assert e.value.code == _lib.ERR_INVALID, (p, n, e.value)
        assert ctx.wav2mel(torch.zeros(1, pad + 1, device="cuda"), **p).shape[1] == fr.n_frames(p, pad + 1) >= 1


# ---- (b) streaming equals whole signal, bit for bit
STREAM_FFT, LENGTHS, _stream_cfgs = fr.STREAM_FFT, fr.STREAM_LENGTHS, fr.stream_cfgs
assert LENGTHS == (700, L, 3 * L, 4 * L + 333, 9 * HOP + 1)      # 700 < 1024: at fft_size 2048 every frame arrives in the final call


def _rows(B, N, seed):
    """[B, N] cuda: broadband rows (one seed each); with three or more rows the second is the tone and the third silence."""
    x = np.stack([fr.signal("broadband", N, 16000, seed + i) for i in range(B)])
    if B >= 3:
        x[1], x[2] = fr.signal("tone", N, 16000), fr.signal("silence", N, 16000)
    return torch.from_numpy(x).cuda()


def _within_bound(frames, wav, mel):
    """frames [T, 80] (cuda) of one utterance against frontend_ref directly (so this file holds without part (a) having run)."""
    p = fr.config(**mel)
    ref = fr.reference(wav.cpu().numpy(), p)
    r = np.abs(frames.cpu().numpy().astype(np.float64) - ref["mel"]) / fr.bound(ref, p)
    assert frames.shape == ref["mel"].shape and r.max() <= 1.0, (mel, r.max())


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("n_fft", STREAM_FFT)
def test_step_wav_frames_bitwise_equal_wav2mel(ctx, n_fft, B):
    """conan_step_wav at a common position, no source feature enabled: the chunks are those of the whole utterance's conan_wav2mel
    frames, one mel_stream_kernel launch per call that completes frames ((R - N / 2) / hop + 1 frames before the final call),
    mel_stream_copy_kernel in the calls that only copy."""
    eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    for k, mel in enumerate(_stream_cfgs(n_fft)):
        for j, N in enumerate(LENGTHS):
            wav = _rows(B, N, fr.stream_seed(k, j))
            whole = ctx.wav2mel(wav, **mel)
            want = list(eng.chunks(whole))
            eng.start_wav(_ref(B))
            eng.st.profile_begin()
            got, frames, first_emit, ncalls, fdone, with_frames, copy_only = _stream_frames(eng, wav, mel=mel)
            eng.st.profile_end()
            launches = {r[0]: r[3] for r in eng.st.profile_kernels()}
            assert len(got) == len(want), (mel, N, len(got), len(want))
            for (emit, ch), (_, emit_w, ch_w) in zip(got, want):
                assert emit == emit_w and torch.equal(ch, ch_w), (mel, N)
            assert torch.equal(torch.cat(frames, 1), whole), (mel, N)
            assert fdone == whole.shape[1] and with_frames >= 1
            assert launches.get("mel_stream_kernel") == with_frames, (mel, N, launches, with_frames)
            assert launches.get("mel_stream_copy_kernel", 0) == copy_only == ncalls - 1 - with_frames, (mel, N, launches, copy_only)
            assert "mel_stream_ragged_kernel" not in launches, launches
            assert (first_emit == 0) == (N > L), (mel, N, first_emit)
            if n_fft == 2048 and N <= L:
                assert with_frames == 1        # nothing completes before the final call; what follows only copies
            if N == fr.STREAM_DIRECT:
                _within_bound(torch.cat(frames, 1)[0], wav[0], mel)
    eng.st.close()


@pytest.mark.parametrize("n_fft", [64, 2048])
def test_step_wav_async_frames_bitwise_equal_wav2mel(ctx, n_fft):
    """The pipelined step (conan_step_wav_async), read after a join: the same frames."""
    B = 3
    eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    for k, mel in enumerate(_stream_cfgs(n_fft)):
        for j, N in enumerate((700, 4 * L + 333)):
            wav = _rows(B, N, 50 + 10 * k + j)
            whole = ctx.wav2mel(wav, **mel)
            eng.start_wav(_ref(B))
            got, frames, *_ = _stream_frames(eng, wav, mel=mel, pipelined=True)
            torch.cuda.synchronize()
            assert torch.equal(torch.cat(frames, 1), whole), (mel, N)
    eng.st.close()


def test_reset_mid_utterance_at_fft_2048_leaves_the_neighbour(ctx):
    """Slot 1 is reset two calls into an utterance and starts another; slot 0 streams on.  Both give the frames of their whole
    utterances (the reset clears the slot's audio ring and position, nothing of its neighbour's)."""
    def feeder(eng, slot, src, mel, out):
        """One conan_step_wav call of `slot` per next(), the drain included; the emitted rows of each call's chunk go to `out`."""
        N = src.shape[1]
        for a, b, fin in _calls(N) + [(N, N, True)] * (2 + N // L):
            emit, *_ = eng.st.step_wav([slot], src[:, a:b], final=fin, mel=mel)
            if emit:
                out.append(eng.st.wav_chunk(1)[:, :emit])
            elif a == b:
                return
            yield

    for mel in _stream_cfgs(2048):
        eng = StreamingVoiceConversionEngine(ctx, 2, max_ref_frames=64)
        a, x, y = _rows(1, 5 * L, 71), _rows(1, 4 * L, 72), _rows(1, 2 * L + 700, 73)
        eng.start_wav(_ref(2))
        fa, fx, fy = [], [], []
        run_a, run_x, run_y = feeder(eng, 0, a, mel, fa), feeder(eng, 1, x, mel, fx), feeder(eng, 1, y, mel, fy)
        for k in range(16):
            next(run_a, None)
            if k < 2:
                next(run_x)
            else:
                if k == 2:
                    eng.st.reset([1], which=15)
                    eng.st.set_reference([1], _ref(1))
                next(run_y, None)
        torch.cuda.synchronize()
        assert next(run_a, "done") == "done" and next(run_y, "done") == "done"
        assert torch.equal(torch.cat(fa, 1), ctx.wav2mel(a, **mel)), mel
        assert torch.equal(torch.cat(fy, 1), ctx.wav2mel(y, **mel)), mel
        eng.st.close()




# A ragged call's chunk rows are grouped by emit and conan_step_wav_chunk refuses them, and the steps behind the front-end see the frames
# only through the Emformer's codes (an argmax: a frame that is a few per cent off can leave every code as it was).  So the ragged
# kernel's frames are read where it writes them: the slot's mel ring (frame f at f & (LM - 1), longer than any utterance here), out of
# a slot snapshot taken right after the slot's final call, which completes its last frames.  The blob row of a slot that has streamed
# is [core section | audio ring, LA floats | mel ring, LM x 80 floats]; a freshly reset slot's row is the core section alone.
def _mel_ring(ctx, st, slot, core_bytes, T):
    """Frames 0 .. T - 1 of `slot` from its mel ring [T, 80] (cuda)."""
    nm = ctx.cfg.emf_input_dim
    LA = 1 << int(np.ceil(np.log2(2048 + ctx.cfg.emf_segment * ctx.hop)))
    snap = st.export_slots([slot])
    used = snap.info(0)["bytes"]
    ring = snap.blob[0, core_bytes + 4 * LA:used].view(torch.float32)
    LM = ring.numel() // nm
    assert used > core_bytes + 4 * LA and ring.numel() == LM * nm and LM & (LM - 1) == 0 and T <= LM, (used, core_bytes, LA, ring.numel())
    return ring.view(LM, nm)[:T].clone()


def _ragged_run(ctx, eng, utts, starts, refs, mel, core_bytes):
    """Utterance u in slot u from tick starts[u] on, one conan_step_wav_ragged call per tick over the live slots (infer_wav_staggered's
    calls) -> (outs: (wav, mel, codes) per utterance, rings: its frames from the mel ring after its final call, work: per call whether
    it had front-end work)."""
    U = len(utts)
    state, done, tick = {}, set(), 0
    outs, rings, work = [[] for _ in range(U)], [None] * U, []
    while len(done) < U:
        for u in range(U):
            if starts[u] == tick:
                eng.open_slots([u], refs[u][None])
                state[u] = [0, False]
        live = [u for u in sorted(state) if u not in done]
        rows, sm, fi = [], [], []
        for u in live:
            x, (pos, fin) = utts[u], state[u]
            N = x.shape[0]
            last = (N - 1) // L * L
            if pos < last:
                piece, state[u][0] = x[pos:pos + L], pos + L
            elif not fin:
                piece, state[u][0] = x[pos:], N
            else:
                piece = x[:0]
            fi.append(int(pos >= last))
            sm.append(piece.shape[0])
            rows.append(torch.nn.functional.pad(piece, (0, L - piece.shape[0])))
        emit, c, m, w = eng.st.step_wav_ragged(live, torch.stack(rows), sm, fi, mel=mel)
        work.append(any(sm) or any(emit))
        for i, u in enumerate(live):
            e = emit[i]
            if e:
                outs[u].append((w[i, :e * HOP].clone(), m[i, :e].clone(), c[i, :e].clone()))
            elif state[u][1]:
                done.add(u)                            # the drain's empty answer
            if fi[i] and not state[u][1]:              # the final call: every frame of the utterance is in the ring now
                state[u][1] = True
                rings[u] = _mel_ring(ctx, eng.st, u, core_bytes, 1 + utts[u].shape[0] // HOP)
        tick += 1
    return [tuple(torch.cat(t, 0) for t in zip(*o)) for o in outs], rings, work


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("n_fft", STREAM_FFT)
def test_step_wav_ragged_frames_bitwise_equal_wav2mel(ctx, n_fft, B):
    """conan_step_wav_ragged: slot i starts i calls late and the slots' utterances have different lengths (five rows make a workgroup's
    four frames span rows).  Every utterance's frames, read from its slot's mel ring, are conan_wav2mel's of the whole utterance bit for
    bit - the ring read is first shown to give conan_step_wav's frames - and on the fixed-plan stream-set its (wav, mel, codes) are those
    of the mel-in loop fed these frames.  One mel_stream_ragged_kernel launch per call with work, none of conan_step_wav's kernels."""
    eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64, flags=FIXED)
    solo = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64, flags=FIXED)
    solo.slots = [0]
    refs = _ref(B)
    eng.st.reset(eng.slots, which=15)
    core_bytes = eng.st.export_slots([0]).info(0)["bytes"]
    for k, mel in enumerate(_stream_cfgs(n_fft)):
        lens = [fr.ragged_length(n_fft, k, i) for i in range(B)]
        utts = [_rows(1, N, fr.ragged_seed(k, i))[0] for i, N in enumerate(lens)]
        if B >= 3:
            utts[1] = torch.from_numpy(fr.signal("tone", lens[1], 16000)).cuda()
        wholes = [ctx.wav2mel(x[None], **mel)[0] for x in utts]
        # the ring read itself, on frames already known: slot 0 through conan_step_wav up to its final call
        solo.start_wav(refs[:1])
        for a, b, fin in _calls(lens[0]):
            solo.st.step_wav([0], utts[0][None, a:b], final=fin, mel=mel)
        assert torch.equal(_mel_ring(ctx, solo.st, 0, core_bytes, wholes[0].shape[0]), wholes[0]), (mel, lens[0])
        eng.st.profile_begin()
        got, rings, work = _ragged_run(ctx, eng, utts, list(range(B)), refs, mel, core_bytes)
        eng.st.profile_end()
        launches = {r[0]: r[3] for r in eng.st.profile_kernels()}
        assert launches.get("mel_stream_ragged_kernel") == sum(work) >= 1, (mel, launches, work)
        assert "mel_stream_kernel" not in launches and "mel_stream_copy_kernel" not in launches, launches
        for u in range(B):
            assert torch.equal(rings[u], wholes[u]), (mel, u, lens[u])
            w, m, c = solo.infer(wholes[u][None], refs[u][None], pipelined=False)
            torch.cuda.synchronize()
            assert got[u][2].shape[0] == wholes[u].shape[0], (mel, u, lens[u])
            assert torch.equal(got[u][2], c[0]) and torch.equal(got[u][1], m[0]) and torch.equal(got[u][0], w[0]), (mel, u, lens[u])
        _within_bound(rings[0], utts[0], mel)
    eng.st.close()
    solo.st.close()
