"""Ragged waveform-in steps (conan_step_wav_ragged / _async, StreamingVoiceConversionEngine.feed_ragged / infer_wav_staggered) on
the GPU: slots at different positions of their utterances in one call give, per slot, what conan_step_wav gives that slot alone -
bit for bit on fixed-plan stream-sets, within the loop tolerances on auto-plan ones - with one front-end launch per call, one chunk
step per emit group and at most one scatter launch; errors leave every slot where it was."""
import ctypes as C

import numpy as np
import pytest
import torch

from conan_amd import _lib, configs, synth
from conan_amd.engine import StreamingVoiceConversionEngine
from conan_amd.runtime import mel_cfg
from tests.conftest import ARITHS
from tests.test_gpu_stream_wav import HOP, L, LENGTHS, SEG, _calls, _ref, _wav, ctx  # noqa: F401  (ctx: module fixture)
from tests.wav_helpers import _equal

pytestmark = pytest.mark.gpu

FIXED = _lib.STREAMS_FIXED_PLAN
FRONT, SCATTER, EMF = "mel_stream_ragged_kernel", "wav_rows_scatter_kernel", "emformer_fused_kernel"


def _launches(st):
    return {k[0]: k[3] for k in st.profile_kernels()}


def _count(launches, part):
    return sum(v for k, v in launches.items() if part in k)


def _utts(lengths, seed):
    return [_wav(1, N, seed + j)[0] for j, N in enumerate(lengths)]


def _refs(U, seed=3):
    return torch.from_numpy(synth.mel(40, seed, U)).cuda()


def _solo_engine(ctx, arith, B, slot=0):
    """One slot of a fixed-plan set of B slots, for infer_wav of one utterance alone."""
    eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64, arith=arith, flags=FIXED)
    eng.slots = [slot]
    return eng


def _solo(eng, x, ref):
    w, m, c = eng.infer_wav(x[None], ref[None], pipelined=False)
    torch.cuda.synchronize()
    return w[0], m[0], c[0]


# ---- 1. slots at a common position: the ragged step is conan_step_wav
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("B", [1, 4, 64])
def test_common_position_equals_step_wav(ctx, arith, B):
    ea = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64, arith=arith)
    eb = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64, arith=arith)
    ref = _ref(B)
    for j, N in enumerate(LENGTHS if B < 64 else LENGTHS[:3]):
        wav = _wav(B, N, 60 + j)
        for pipelined in (False, True):
            ea.start_wav(ref)
            eb.start_wav(ref)
            if not pipelined:
                eb.st.profile_begin()
            calls, got, want, fronts, scatters = _calls(N), [], [], 0, 0
            while True:
                if calls:
                    a, b, fin = calls.pop(0)
                    piece = wav[:, a:b]
                else:
                    piece, fin = wav[:, :0], True
                step_a = ea.st.step_wav_async if pipelined else ea.st.step_wav
                step_b = eb.st.step_wav_ragged_async if pipelined else eb.st.step_wav_ragged
                e, c, m, w = step_a(ea.slots, piece, final=fin)
                er, cr, mr, wr = step_b(eb.slots, piece, [piece.shape[1]] * B, [fin] * B)
                assert er == [e] * B, (N, e, er)
                want.append((e, c, m, w))
                got.append((er[0], cr, mr, wr))
                fronts += piece.shape[1] > 0 or e > 0         # the drain's empty answer has no front-end work
                scatters += 0 < e < SEG                       # short chunks: rows of [n][e] into rows of [n][seg]
                if piece.shape[1] == 0 and e == 0:
                    break
            if pipelined:
                ea.st.join()
                eb.st.join()
            torch.cuda.synchronize()
            for (e, c, m, w), (er, cr, mr, wr) in zip(want, got):
                assert torch.equal(cr[:, :e], c[:, :e]), (N, pipelined)
                assert torch.equal(mr[:, :e], m) and torch.equal(wr[:, :e * HOP], w), (N, pipelined, e)
            if not pipelined:
                eb.st.profile_end()
                lc = _launches(eb.st)
                # one front-end launch per call that has work, none of conan_step_wav's; the scatter only for short chunks
                assert "mel_stream_kernel" not in lc and "mel_stream_copy_kernel" not in lc, lc
                assert lc.get(FRONT, 0) == fronts == len(want) - 1, (N, lc, fronts)
                assert lc.get(SCATTER, 0) == scatters, (N, lc, scatters)
                assert _count(lc, EMF) == sum(1 for e, *_ in want if e), (N, lc)
    ea.st.close()
    eb.st.close()


# ---- 2. staggered streams equal solo runs bit for bit (fixed plan)
def _schedule(U=64, seed=7):
    rng = np.random.default_rng(seed)
    base = list(LENGTHS) + [HOP, 2 * L - 1, 6 * L + HOP + 1, 5 * HOP, 9 * HOP - 1]
    lengths = [base[j % len(base)] for j in range(U)]
    starts = [int(s) for s in rng.integers(0, 21, U)]
    starts[0], lengths[0] = 0, 700                        # ends at tick 1: its slot is reused by a later start
    starts[1], lengths[1] = 0, 5 * L
    starts[2], lengths[2] = 2, 3 * L                      # starts while slot 0 drains
    starts[3] = starts[4] = 6                             # two starts in one tick
    return lengths, starts


@pytest.mark.parametrize("arith", ARITHS)
def test_staggered_equals_solo_fixed_plan(ctx, arith):
    lengths, starts = _schedule()
    U = len(lengths)
    utts, refs = _utts(lengths, 100), _refs(U)
    eng = StreamingVoiceConversionEngine(ctx, 64, max_ref_frames=64, arith=arith, flags=FIXED)
    blk = eng.infer_wav_staggered(utts, starts, refs, pipelined=False)
    slots_used = list(eng.staggered_slots)
    assert len(set(slots_used)) < U, "no slot was reused"
    pip = eng.infer_wav_staggered(utts, starts, refs, pipelined=True)
    torch.cuda.synchronize()
    eng.st.close()
    for u in range(U):
        assert _equal(pip[u], blk[u]), (u, "pipelined")
    solo = _solo_engine(ctx, arith, 64)
    for u in range(U):
        assert _equal(blk[u], _solo(solo, utts[u], refs[u])), (u, lengths[u], starts[u])
    solo.st.close()


# ---- 3. auto plan: within the loop tolerances; 2 streams against the CPU oracle
def _close(got, want):
    w, m, c = got
    w0, m0, c0 = want
    assert m.shape == m0.shape and w.shape == w0.shape
    agree = (c == c0).float().mean().item()
    assert agree >= 0.95, agree
    if agree == 1.0:
        torch.testing.assert_close(m, m0, atol=1e-4, rtol=1e-4)
        torch.testing.assert_close(w, w0, atol=1e-4, rtol=0)


def test_staggered_auto_plan_and_oracle(ctx):
    from oracle import emformer as oemf
    from oracle import frontend as ofe
    from oracle import loop as oloop
    from oracle.common import to_torch_sd
    lengths = [3 * L + 1, 2 * L + 517, 700, 9 * HOP, 5 * L + 3, 11 * HOP - 1, 4 * L, 2 * L]
    starts = [0, 1, 1, 3, 0, 5, 2, 7]
    U = len(lengths)
    utts, refs = _utts(lengths, 200), _refs(U, 5)
    eng = StreamingVoiceConversionEngine(ctx, 8, max_ref_frames=64)
    got = eng.infer_wav_staggered(utts, starts, refs)
    torch.cuda.synchronize()
    eng.st.close()
    solo = StreamingVoiceConversionEngine(ctx, 1, max_ref_frames=64)
    for u in range(U):
        want = solo.infer_wav(utts[u][None], refs[u][None], pipelined=False)
        torch.cuda.synchronize()
        _close(got[u], tuple(t[0] for t in want))
    solo.st.close()
    chp, vhp = configs.conan_hparams(True), configs.hifigan_hparams(True)
    sds = {"emformer": synth.emformer_state_dict(chp, 0), "conan": synth.conan_state_dict(chp, 0), "hifigan": synth.hifigan_state_dict(vhp, 0)}
    tsd = {k: to_torch_sd(v) for k, v in sds.items()}
    cfg = oemf.EmformerCfg(chp)
    for u in (0, 1):
        w, m, c = (t.cpu().numpy() for t in got[u])
        src = ofe.wav2mel(utts[u].cpu().numpy())
        assert m.shape[0] == src.shape[0]
        rn = refs[u].cpu().numpy()
        _, _, c_ref = oloop.infer_once_stateful(tsd["emformer"], cfg, tsd["conan"], chp, tsd["hifigan"], vhp, src, rn)
        assert np.mean(c_ref == c) >= 0.95
        w_ref, m_ref, _ = oloop.infer_once_stateful(tsd["emformer"], cfg, tsd["conan"], chp, tsd["hifigan"], vhp, src, rn, codes_override=c)
        np.testing.assert_allclose(m, m_ref, atol=1e-4, rtol=1e-4)
        np.testing.assert_allclose(w, w_ref, atol=1e-4, rtol=0)


# ---- 4. one call with emit 0, 4 and short last chunks of 1, 2, 3 frames
def _plan(N):
    """(samples start, stop, final) of every call of one utterance: infer_wav's calls, then drain calls (_run_calls stops at the
    drain's empty answer)."""
    return _calls(N) + [(N, N, True)] * (2 + N // L)


def _run_calls(st, slot, x, calls):
    """One-slot ragged calls up to the drain's empty answer; -> list of (emit, codes, mel, wav) per call."""
    res = []
    for a, b, fin in calls:
        e, c, m, w = st.step_wav_ragged([slot], x[a:b][None], [b - a], [fin])
        e = e[0]
        res.append((e, c[0, :e].clone(), m[0, :e].clone(), w[0, :e * HOP].clone()))
        if a == b and e == 0:
            break
    return res


@pytest.mark.parametrize("arith", ARITHS)
def test_mixed_emit_groups_in_one_call(ctx, arith):
    ref = _ref(1)
    # utterances whose last chunk has 1, 2, 3 frames (T = 1 + N // hop frames), one long one in steady state, one just starting
    lens = {"first": 3 * L, "steady": 5 * L, "d1": 8 * HOP + 5, "d2": 9 * HOP + 7, "d3": 10 * HOP}
    targets = {"first": 0, "steady": SEG, "d1": 1, "d2": 2, "d3": 3}
    utts = {k: _wav(1, N, 300 + j)[0] for j, (k, N) in enumerate(lens.items())}
    # solo per utterance: which call emits the target, and its outputs
    solo_eng = StreamingVoiceConversionEngine(ctx, 8, max_ref_frames=64, arith=arith, flags=FIXED)
    picks = {}
    for k, x in utts.items():
        calls = _plan(lens[k])
        solo_eng.slots = [0]
        solo_eng.open_slots([0], ref)
        res = _run_calls(solo_eng.st, 0, x, calls)
        idx = [j for j, r in enumerate(res) if r[0] == targets[k] and (targets[k] != SEG or j >= 2)]
        assert idx, (k, [r[0] for r in res])
        picks[k] = (calls, idx[0], res[idx[0]])
    torch.cuda.synchronize()
    solo_eng.st.close()
    eng = StreamingVoiceConversionEngine(ctx, 8, max_ref_frames=64, arith=arith, flags=FIXED)
    names = ["d2", "first", "steady", "d3", "d1"]            # call order differs from slot order and from the groups' order
    slot_of = {k: s for k, s in zip(names, [5, 0, 3, 1, 6])}
    for k in names:
        eng.open_slots([slot_of[k]], ref)
        calls, j, _ = picks[k]
        _run_calls(eng.st, slot_of[k], utts[k], calls[:j])
    rows, samples, final = [], [], []
    for k in names:
        calls, j, _ = picks[k]
        a, b, fin = calls[j]
        rows.append(torch.nn.functional.pad(utts[k][a:b], (0, L - (b - a))))
        samples.append(b - a)
        final.append(fin)
    wav_out = torch.full((len(names), L), 7.0, device="cuda")
    eng.st.profile_begin()
    emit, c, m, w = eng.st.step_wav_ragged([slot_of[k] for k in names], torch.stack(rows), samples, final, wav_out=wav_out)
    eng.st.profile_end()
    torch.cuda.synchronize()
    lc = _launches(eng.st)
    assert emit == [targets[k] for k in names], emit
    for i, k in enumerate(names):
        e, c0, m0, w0 = picks[k][2]
        assert emit[i] == e
        assert torch.equal(c[i, :e], c0) and torch.equal(m[i, :e], m0) and torch.equal(w[i, :e * HOP], w0), k
        assert bool((w[i, e * HOP:] == 7.0).all()), k                   # past the row's emit: untouched
    groups = len({e for e in emit if e})
    assert groups == 4
    assert lc.get(FRONT) == 1 and lc.get(SCATTER, 0) <= 1 and _count(lc, EMF) == groups, lc
    eng.st.close()


# ---- 5. a bad entry anywhere leaves every slot where it was
def test_errors_are_atomic(ctx):
    lib = _lib.lib()
    ref = _ref(1)
    x = {s: _wav(1, 4 * L + 100, 400 + s)[0] for s in range(5)}

    def prepare():
        eng = StreamingVoiceConversionEngine(ctx, 8, max_ref_frames=64, flags=FIXED)
        for s in range(5):
            eng.open_slots([s], ref)
        # slot 0: two chunks in; slot 1: fresh; slot 2: after its final call (phase 1); slot 3: drained; slot 4: one chunk in
        _run_calls(eng.st, 0, x[0], [(0, L, False), (L, 2 * L, False)])
        _run_calls(eng.st, 2, x[2], [(0, L, False), (L, L + 700, True)])
        res = _run_calls(eng.st, 3, x[3], [(0, 700, True), (700, 700, True)])
        assert res[-1][0] == 0
        _run_calls(eng.st, 4, x[4], [(0, L, False)])
        return eng

    good_slots, good_samples, good_final = [4, 0, 1, 2], [L, L, L, 0], [0, 0, 0, 1]
    rows = torch.stack([x[4][L:2 * L], x[0][2 * L:3 * L], x[1][:L], torch.zeros(L, device="cuda")])
    bad_calls = [
        ("exactly segment * hop", [4, 0, 1, 2], [L, L, L - 1, 0], [0, 0, 0, 1], mel_cfg()),
        ("only samples = 0", [4, 0, 1, 2], [L, L, L, 5], [0, 0, 0, 1], mel_cfg()),
        ("drained", [4, 0, 1, 3], [L, L, L, 0], [0, 0, 0, 1], mel_cfg()),
        ("duplicate slot", [4, 0, 1, 4], [L, L, L, L], [0, 0, 0, 0], mel_cfg()),
        ("framing 0", good_slots, good_samples, good_final, mel_cfg(framing=1)),
    ]
    eng = prepare()
    out = torch.empty(4, L, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    emit = (C.c_int32 * 4)()
    for text, sl, sm, fi, mc in bad_calls:
        for fn in (lib.conan_step_wav_ragged, lib.conan_step_wav_ragged_async):
            rc = fn(eng.st.h, (C.c_int32 * 4)(*sl), 4, (C.c_int32 * 4)(*sm), (C.c_int32 * 4)(*fi), C.c_void_p(rows.data_ptr()), C.byref(mc),
                    None, None, C.c_void_p(out.data_ptr()), emit, s)
            assert rc == _lib.ERR_INVALID and text in lib.conan_last_error().decode(), (text, rc, lib.conan_last_error())
    mc = mel_cfg()
    args = [(C.c_int32 * 4)(*good_slots), (C.c_int32 * 4)(*good_samples), (C.c_int32 * 4)(*good_final), emit]
    for k in range(4):          # null slots / samples / final / emit_out
        a = list(args)
        a[k] = None
        rc = lib.conan_step_wav_ragged(eng.st.h, a[0], 4, a[1], a[2], C.c_void_p(rows.data_ptr()), C.byref(mc), None, None,
                                       C.c_void_p(out.data_ptr()), a[3], s)
        assert rc == _lib.ERR_INVALID and "null argument" in lib.conan_last_error().decode()
    rc = lib.conan_step_wav_ragged(eng.st.h, args[0], 4, args[1], args[2], None, C.byref(mc), None, None, C.c_void_p(out.data_ptr()), args[3], s)
    assert rc == _lib.ERR_INVALID and "null argument" in lib.conan_last_error().decode()
    got = eng.st.step_wav_ragged(good_slots, rows, good_samples, good_final)
    twin = prepare()
    want = twin.st.step_wav_ragged(good_slots, rows, good_samples, good_final)
    torch.cuda.synchronize()
    assert got[0] == want[0] == [SEG, SEG, 0, 3], got[0]        # slot 2: 1980 samples = 7 frames, the first 4 came with its final call
    for i, e in enumerate(got[0]):
        assert torch.equal(got[1][i, :e], want[1][i, :e]) and torch.equal(got[2][i, :e], want[2][i, :e])
        assert torch.equal(got[3][i, :e * HOP], want[3][i, :e * HOP])
    # conan_step_wav_chunk refuses to copy a ragged call's chunk
    assert lib.conan_step_wav_chunk(eng.st.h, C.c_void_p(out.data_ptr()), s) == _lib.ERR_STATE
    eng.st.close()
    twin.st.close()


# ---- 6. a front-end reset of one slot mid-run restarts that slot only
def test_reset_one_slot_mid_staggered_run(ctx):
    lengths, starts = [5 * L, 4 * L + 11, 6 * L - 1, 3 * L + HOP], [0, 1, 0, 2]
    utts, refs = _utts(lengths, 500), _refs(4, 9)
    base = StreamingVoiceConversionEngine(ctx, 4, max_ref_frames=64, flags=FIXED)
    want = base.infer_wav_staggered(utts, starts, refs, pipelined=False)
    base.st.close()
    other = _wav(1, 3 * L + 5, 501)[0]
    eng = StreamingVoiceConversionEngine(ctx, 4, max_ref_frames=64, flags=FIXED)
    # slot 2 runs utterance 2 for three ticks, is reset at tick 3 and then runs `other`
    srcs = {0: utts[0], 1: utts[1], 2: utts[2], 3: utts[3]}
    state = {}
    outs = {0: [], 1: [], 3: [], "other": []}
    tick = 0
    while True:
        for s in range(4):
            if starts[s] == tick:
                eng.open_slots([s], refs[s][None])
                state[s] = [0, False, False]
        if tick == 3:
            eng.st.reset([2], which=15)
            eng.st.set_reference([2], refs[2][None])
            srcs[2], state[2] = other, [0, False, False]
        live = [s for s in sorted(state) if not state[s][2]]
        if not live:
            break
        rows, sm, fi = [], [], []
        for s in live:
            pos, fin, _ = state[s]
            xx, N = srcs[s], srcs[s].shape[0]
            last = (N - 1) // L * L
            if pos < last:
                piece, state[s][0] = xx[pos:pos + L], pos + L
                fi.append(0)
            elif not fin:
                piece, state[s][0], state[s][1] = xx[pos:], N, True
                fi.append(1)
            else:
                piece = xx[:0]
                fi.append(1)
            sm.append(piece.shape[0])
            rows.append(torch.nn.functional.pad(piece, (0, L - piece.shape[0])))
        res = eng.feed_ragged(live, torch.stack(rows), sm, fi)
        for s, f, (w, m, c) in zip(live, fi, res):
            key = "other" if s == 2 else s
            if m.shape[0]:
                if s != 2 or tick >= 3:
                    outs[key].append((w, m, c))
            elif f and state[s][1]:
                state[s][2] = True
        tick += 1
    torch.cuda.synchronize()
    for s in (0, 1, 3):
        got = tuple(torch.cat(t, 0) for t in zip(*outs[s]))
        assert _equal(got, want[s]), s
    got = tuple(torch.cat(t, 0) for t in zip(*outs["other"]))
    solo = _solo_engine(ctx, "auto", 4, slot=2)
    assert _equal(got, _solo(solo, other, refs[2]))
    solo.st.close()
    eng.st.close()
