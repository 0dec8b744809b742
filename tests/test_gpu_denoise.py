"""Input noise suppression on the GPU (conan_mel_denoise, conan_streams_set_denoise, conan_streams_denoise_state; include/conan_hip.h,
conan_denoise_cfg): the law against tests/denoise_ref.py, the streamed chunks and state against the whole-signal form, the wav-in
steps against themselves - neighbours keep their bits, pipelined equals blocking, live changes, restarts, the hand-over - errors,
and enrolment.  The law is integers and single correctly rounded operations: every comparison is on bit patterns."""
import ctypes as C

import numpy as np
import pytest
import torch

from conan_amd import _lib
from conan_amd.runtime import Context, VoiceBank, _ptr, _stream
from tests import denoise_ref as R
from tests import f0_ref
from tests import pitch_ref as P
from tests.test_denoise_cpu import BAD
from tests.test_denoise_ref_cpu import CLAMPS, DEFAULT, PLAIN, noisy
from tests.test_gpu_f0 import _launches, _open, _ragged, _ref, _run
from tests.test_gpu_pitch import full  # noqa: F401  (module fixture: the small synthetic full model)

pytestmark = pytest.mark.gpu

HOP, SEG = 320, 4
L = SEG * HOP
MAX_SLOTS = 6
STATE = C.sizeof(_lib.DenoiseState)
CFGS = [DEFAULT, PLAIN, CLAMPS]


def _cfg(p, **kw):
    return _lib.denoise_cfg(**dict({k: (float(v) if k == "out_floor" else int(v)) for k, v in p.items()}, **kw))


def _u32(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _wav(B, N, seed):
    """Harmonic signals in white noise: the suppressor has a floor to find and bins to close."""
    g = torch.Generator().manual_seed(seed)
    return (torch.from_numpy(f0_ref.sig(B, N, 16000, seed)) + 0.02 * torch.randn(B, N, generator=g)).float().cuda()


def _on(st, slots, **kw):
    st.set_denoise(slots, **kw)


# ------------------------------------------------------------------------------------------------------------------ 1. the law

def law_input(nm, T, n, seed):
    x = np.stack([noisy(T, nm, seed + i) for i in range(n)])
    if T >= 3:      # values no mel front-end writes: the law still defines them
        odd = np.array([0x7FC00123, 0x7F800000, 0xFF800000, 0x80000000, 0x44FA0000], np.uint32).view(np.float32)
        x[0, T // 2, :min(nm, 5)] = odd[:min(nm, 5)]
    return x


def law_lens(T, n):
    return [T] if n == 1 else [T, T // 2, max(T - 1, 0) if T > 1 else 0]


@pytest.mark.parametrize("nm", [1, 2, 63, 64, 65, 80, 256])
def test_mel_denoise_against_the_reference(full, nm):
    R.seen.clear()
    for T in (1, 2, 3, 50, 257):
        for n in (1, 3):
            lens = law_lens(T, n)
            x = law_input(nm, T, n, 100 * nm + T)
            ld = T * nm + 5      # a row stride wider than the rows
            buf = torch.zeros(n, ld, device="cuda")
            buf[:, :T * nm] = torch.from_numpy(x.reshape(n, -1)).cuda()
            view = torch.as_strided(buf, (n, T, nm), (ld, nm, 1))
            for p in CFGS:
                c = _cfg(p)
                y, st = full.mel_denoise(view, lens=lens, cfg=c, state=True)
                raw = st.cpu().numpy().tobytes()
                for i in range(n):
                    want, ws = R.denoise(x[i, :lens[i]], p)
                    assert np.array_equal(_u32(y[i, :lens[i]]), want.view(np.uint32)), (T, n, i)
                    assert raw[i * STATE:(i + 1) * STATE] == R.state_bytes(ws), (T, n, i)
                # seeded rows: the second half from the first half's state is the whole
                cut = T // 2
                l0, l1 = [min(v, cut) for v in lens], [max(v - cut, 0) for v in lens]
                y0, s0 = full.mel_denoise(view[:, :cut], lens=l0, cfg=c, state=True)
                y1, s1 = full.mel_denoise(view[:, cut:], lens=l1, cfg=c, seed=s0, state=True)
                assert torch.equal(s1, st), (T, n)
                for i in range(n):
                    got = torch.cat([y0[i, :l0[i]], y1[i, :l1[i]]])
                    assert np.array_equal(_u32(got), _u32(y[i, :lens[i]])), (T, n, i)
                # in place, and the frames past a row's length keep their bits
                work = buf.clone()
                wv = torch.as_strided(work, (n, T, nm), (ld, nm, 1))
                out = full.mel_denoise(wv, lens=lens, cfg=c, out=wv)
                assert out is wv
                for i in range(n):
                    assert np.array_equal(_u32(wv[i, :lens[i]]), _u32(y[i, :lens[i]])), (T, n, i)
                    assert np.array_equal(_u32(wv[i, lens[i]:]), _u32(view[i, lens[i]:])), (T, n, i)
                assert np.array_equal(_u32(work[:, T * nm:]), _u32(buf[:, T * nm:]))
                if n == 3:      # a row alone is that row in a batch
                    alone = full.mel_denoise(view[1:2], lens=lens[1:2], cfg=c)
                    assert np.array_equal(_u32(alone[0, :lens[1]]), _u32(y[1, :lens[1]])), T
    missing = [b for b in R.BRANCHES if R.seen[b] < 1]
    assert not missing, (missing, dict(R.seen))


@pytest.mark.parametrize("nm", [65, 80, 256])
def test_seed_records(full, nm):
    """What a seed may hold.  A record before the first frame (the zero record, one of another width) starts every bin of every wave
    from Start, also without the cross-bin step, where the frames have no barrier; a seed in place (state_out = seed) is the seed
    apart; floor and att words outside the law's range are read clamped to it."""
    T = 7
    x = noisy(T, nm, 7 * nm)
    mel = torch.from_numpy(x[None]).cuda()
    lim = 1 << 20
    for p in CFGS:
        c = _cfg(p)
        y, st = full.mel_denoise(mel, cfg=c, state=True)
        other = R.state_bytes(dict(frames=5, bins=nm - 1, floor=np.full(nm - 1, 77), att=np.full(nm - 1, 9)))
        for raw in (bytes(STATE), other):
            seed = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()[None]
            y0, s0 = full.mel_denoise(mel, cfg=c, seed=seed, state=True)
            assert np.array_equal(_u32(y0), _u32(y)) and torch.equal(s0, st)
        # in place: conan_mel_denoise with state_out_dev = seed_dev
        y1, mid = full.mel_denoise(mel[:, :3], cfg=c, state=True)
        want_y, want_s = full.mel_denoise(mel[:, 3:], cfg=c, seed=mid, state=True)
        rec, tail, out = mid.clone(), mel[:, 3:].contiguous(), torch.empty_like(want_y)
        fr = np.array([T - 3], np.int32)
        _lib.check(full.lib.conan_mel_denoise(full.h, C.byref(c), _ptr(tail), 1, fr.ctypes.data_as(C.c_void_p), (T - 3) * nm, nm, _ptr(rec), _ptr(out),
                                              _ptr(rec), _stream()))
        torch.cuda.synchronize()
        assert np.array_equal(_u32(out), _u32(want_y)) and torch.equal(rec, want_s)
        # words outside the range: the record with them clamped
        wild = dict(frames=3, bins=nm, floor=np.resize(np.array([2**31 - 1, -2**31, lim + 1, -lim - 1, 0, 1234]), nm),
                    att=np.resize(np.array([-2**31, 2**31 - 1, -1, lim + 1, 50]), nm))
        tame = dict(wild, floor=np.clip(wild["floor"], -lim, lim), att=np.clip(wild["att"], 0, lim))
        got = [full.mel_denoise(mel, cfg=c, seed=torch.frombuffer(bytearray(R.state_bytes(d)), dtype=torch.uint8).cuda()[None], state=True)
               for d in (wild, tame)]
        assert np.array_equal(_u32(got[0][0]), _u32(got[1][0])) and torch.equal(got[0][1], got[1][1])
        ref, rs = R.denoise(x, p, state=tame)
        assert np.array_equal(_u32(got[1][0][0]), ref.view(np.uint32)) and got[1][1][0].cpu().numpy().tobytes() == R.state_bytes(rs)


# ------------------------------------------------------------------------------------------------------------------ 2. streaming = whole signal

def _calls(st, slots, wav, first_call=0, pipelined=False, on_call=None, chunks=True):
    """The calls of infer_wav over wav [n, N] from call `first_call` on -> (codes, mel, wav) over the emitted chunks and the list of
    the emitted chunks' (emit, [n, seg + rc, nm] chunk) (blocking runs only)."""
    n, N = wav.shape
    last = (N - 1) // L * L
    calls = ([(p, p + L, False) for p in range(0, last, L)] + [(last, N, True)])[first_call:]
    step = st.step_wav_async if pipelined else st.step_wav
    outs, got, k = [], [], first_call
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
            outs.append((c[:, :e], m, w))
            if chunks and not pipelined:
                got.append((e, st.wav_chunk(n).clone()))
    st.join()
    torch.cuda.synchronize()
    return [torch.cat([o[i] for o in outs], 1).clone() for i in range(3)], got


def _want_chunks(D, rows):
    """The chunks of a whole mel D [F, nm]: chunk t holds frames min(t * SEG + r, F - 1), r < rows."""
    F = D.shape[0]
    return [D[torch.clamp(torch.arange(t * SEG, t * SEG + rows), max=F - 1)] for t in range(-(-F // SEG))]


@pytest.mark.parametrize("N", [3 * L, 3 * L + 1, 2 * L + 319, 2 * L + 320, 700])
def test_streamed_chunks_and_state_equal_the_whole_signal(full, N):
    slots = [4, 1]
    rows = SEG + full.cfg.emf_right_context
    st = _open(full, slots)
    cfgs = [_cfg(DEFAULT), _cfg(CLAMPS)]
    for s, c in zip(slots, cfgs):
        _on(st, [s], cfg=c)
    wav = _wav(2, N, 20 + N % 7)
    _, got = _calls(st, slots, wav)
    F = 1 + N // HOP
    assert sum(e for e, _ in got) == F
    mel = full.wav2mel(wav)
    assert mel.shape[1] == F
    states = st.denoise_state(slots)
    plain = _want_chunks(mel[0], rows)
    for i, c in enumerate(cfgs):
        D, ws = full.mel_denoise(mel[i:i + 1], cfg=c, state=True)
        want = _want_chunks(D[0], rows)      # (a short last chunk repeats its last frame)
        assert len(want) == len(got)
        for t, (e, chunk) in enumerate(got):
            assert e == min(SEG, F - t * SEG)
            assert np.array_equal(_u32(chunk[i]), _u32(want[t])), (N, i, t)
        assert torch.equal(states[i:i + 1], ws), (N, i)
        ref, rs = R.denoise(mel[i].cpu().numpy(), R.fields(c))
        assert np.array_equal(_u32(D[0]), ref.view(np.uint32)) and states[i].cpu().numpy().tobytes() == R.state_bytes(rs)
    assert any(not torch.equal(chunk[0], plain[t]) for t, (_, chunk) in enumerate(got))      # (the suppressor did something)
    st.close()


def test_ragged_equals_same_position(full):
    slots, starts = [5, 0, 2], [0, 1, 3]
    wav = _wav(3, 4 * L + 333, 65)
    cfgs = [dict(), None, dict(smooth=False, fall_shift=0)]
    outs = []
    for ragged in (False, True):
        # a fixed plan: a row's arithmetic in decoder and vocoder does not depend on the rows it shares a launch with, so the two
        # layouts can be compared on the model's outputs
        st = full.streams(MAX_SLOTS, 4, 64, flags=_lib.STREAMS_FIXED_PLAN)
        st.reset(slots, which=15)
        st.set_reference(slots, _ref(len(slots)))
        for s, kw in zip(slots, cfgs):
            if kw is not None:
                _on(st, [s], **kw)
        if ragged:
            res = _ragged(st, slots, [wav[u] for u in range(3)], starts, contour=False)
            outs.append([[res[u][i] for u in range(3)] for i in range(3)])
        else:
            (c, m, w, _, _), _ = _run(st, slots, wav, contour=False)
            outs.append([[t[u] for u in range(3)] for t in (c, m, w)])
        outs[-1].append(st.denoise_state([5, 2]))
        st.close()
    for i in range(3):
        for u in range(3):
            assert np.array_equal(_u32(outs[0][i][u]), _u32(outs[1][i][u])), (i, u)
    assert torch.equal(outs[0][3], outs[1][3])


# ------------------------------------------------------------------------------------------------------------------ 3. neighbours

def _calls_with_work(N, rc, n_fft=1024):
    """The calls of _calls over N samples in which a slot completes a frame or emits: the wav-in step's own plan, restated."""
    last = (N - 1) // L * L
    calls = [(L, False)] * (last // L) + [(N - last, True)]
    recv = frames = chunks = count = 0
    while True:
        sm, fin = calls.pop(0) if calls else (0, True)
        recv += sm
        fc = 1 + recv // HOP if fin else ((recv - n_fft // 2) // HOP + 1 if recv >= n_fft // 2 else 0)
        pos = chunks * SEG
        emit = (min(SEG, fc - pos) if pos < fc else 0) if fin else (SEG if pos + SEG + rc <= fc else 0)
        count += fc > frames or emit > 0
        frames, chunks = max(frames, fc), chunks + (emit > 0)
        if fin and not calls and emit == 0:
            return count

def test_neighbours_keep_their_bits_and_launches(full):
    slots = [0, 1, 2, 3]
    wav = _wav(4, 3 * L + 77, 60)
    a, b = _open(full, slots), _open(full, slots)
    bytes_never = b.state_bytes
    assert a.state_bytes == bytes_never
    _on(a, [0])
    _on(a, [2], depth_db=30.0)
    assert a.state_bytes == bytes_never + MAX_SLOTS * STATE + 4 * MAX_SLOTS * 88      # the states and four row tables, from the first enabling call on
    b.set_denoise(slots, None)      # turning off what was never on allocates nothing
    assert b.state_bytes == bytes_never and b.denoise(slots) == [None] * 4
    (oa, ga), la = _launches(a, lambda: _calls(a, slots, wav))
    (ob, gb), lb = _launches(b, lambda: _calls(b, slots, wav))
    for i in (1, 3):      # slots without the feature: chunk, codes, mel and wav keep their bits
        assert all(np.array_equal(_u32(x[i]), _u32(y[i])) for x, y in zip(oa, ob)), i
        assert all(np.array_equal(_u32(ca[i]), _u32(cb[i])) for (_, ca), (_, cb) in zip(ga, gb)), i
    for i in (0, 2):
        assert any(not torch.equal(ca[i], cb[i]) for (_, ca), (_, cb) in zip(ga, gb)), i
    # one more launch per call in which a suppressing slot completes a frame or emits, and nothing else
    assert "denoise_stream_kernel" not in lb
    assert la.pop("denoise_stream_kernel") == _calls_with_work(wav.shape[1], full.cfg.emf_right_context)
    assert la == lb, (la, lb)
    # off again: the launches of the stream-set that never suppressed
    a.set_denoise(slots, None)
    assert a.denoise(slots) == [None] * 4
    a.reset(slots, which=15)
    a.set_reference(slots, _ref(4))
    (o2, _), l2 = _launches(a, lambda: _calls(a, slots, wav))
    assert l2 == lb and all(torch.equal(x, y) for x, y in zip(o2, ob))
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------ 4. pipelined = blocking, live changes, restarts, hand-over

def test_pipelined_equals_blocking(full):
    slots = [2, 5]
    wav = _wav(2, 13 * L + 77, 70)
    st = _open(full, slots)
    _on(st, [2])
    _on(st, [5], cfg=_cfg(CLAMPS))
    (cb, mb, wb, _, _), eb = _run(st, slots, wav, contour=False)
    assert len(eb) >= 12
    state = st.denoise_state(slots)
    st.reset(slots, which=15)
    st.set_reference(slots, _ref(2))
    (cp, mp, wp, _, _), ep = _run(st, slots, wav, pipelined=True, contour=False)
    assert ep == eb and torch.equal(cp, cb) and torch.equal(mp, mb) and torch.equal(wp, wb)
    assert torch.equal(st.denoise_state(slots), state)
    st.close()


def test_setter_between_pipelined_steps(full):
    """The setter with pipelined steps in flight: a parameter change that keeps the state, a reseed, off and on again, each between
    two step_wav_async calls, against the same calls between blocking steps."""
    slots = [4, 0]
    wav = _wav(2, 12 * L + 200, 33)
    c1, c2 = _cfg(DEFAULT), _cfg(CLAMPS)
    runs = []
    for pipelined in (False, True):
        st = _open(full, slots)
        _on(st, slots, cfg=c1)

        def on_call(k):
            if k == 4:
                st.set_denoise([4], cfg=c2)      # the state stays
                st.set_denoise([0], cfg=_cfg(PLAIN, reseed=True))
            elif k == 7:
                st.set_denoise([4], None)
            elif k == 9:
                st.set_denoise([4], cfg=c1)      # off -> on restarts
                st.set_denoise([0], cfg=c2)

        outs, _ = _calls(st, slots, wav, pipelined=pipelined, on_call=on_call)
        runs.append((outs, st.denoise_state(slots), st.denoise(slots)))
        st.close()
    (ob, sb, kb), (op, sp, kp) = runs
    assert all(np.array_equal(_u32(x), _u32(y)) for x, y in zip(ob, op))
    assert torch.equal(sb, sp) and kb == kp == [_lib.denoise_keywords(c1), _lib.denoise_keywords(c2)]
    # the changes took hold: a run that keeps the first setting gives other outputs
    st = _open(full, slots)
    _on(st, slots, cfg=c1)
    fixed, _ = _calls(st, slots, wav, pipelined=True)
    assert not torch.equal(fixed[1], op[1]) and not torch.equal(st.denoise_state(slots), sp)
    st.close()


def test_live_changes_and_restarts(full):
    slots = [1, 3]
    N = 9 * L + 10
    wav = _wav(2, N, 90)
    mel = full.wav2mel(wav)
    rows = SEG + full.cfg.emf_right_context
    c1, c2 = _cfg(DEFAULT), _cfg(CLAMPS)
    zero = torch.zeros(2, STATE, dtype=torch.uint8, device="cuda")
    st = _open(full, slots)
    _on(st, slots, cfg=c1)
    assert torch.equal(st.denoise_state(slots), zero)      # a pending restart reports the zero record
    assert st.denoise([1]) == [_lib.denoise_keywords(c1)]
    mid = {}

    def on_call(k):      # before call k: frames [0, fk) are complete
        if k == 4:
            mid["s"] = st.denoise_state(slots)
            st.set_denoise([1], cfg=c2)                      # reseed = 0: new parameters from the next frame, the state stays
            assert torch.equal(st.denoise_state(slots), mid["s"])
            st.set_denoise([3], cfg=_cfg(CLAMPS, reseed=True))  # reseed = 1: the state restarts at the next frame
            assert torch.equal(st.denoise_state([3]), zero[:1])

    _, got = _calls(st, slots, wav, on_call=on_call)
    fk = (4 * L - 512) // HOP + 1      # frames complete before call 4 (centred frames of 1024 samples)
    assert R.state_from(mid["s"][0].cpu().numpy().tobytes())["frames"] == fk
    D0, s0 = full.mel_denoise(mel[0:1, :fk], cfg=c1, state=True)
    assert torch.equal(s0, mid["s"][0:1])
    D1, e1 = full.mel_denoise(mel[0:1, fk:], cfg=c2, seed=s0, state=True)      # slot 1: the state carried into the new parameters
    D3a = full.mel_denoise(mel[1:2, :fk], cfg=c1)
    D3b, e3 = full.mel_denoise(mel[1:2, fk:], cfg=c2, state=True)               # slot 3: from before the first frame
    for i, D in enumerate((torch.cat([D0, D1], 1)[0], torch.cat([D3a, D3b], 1)[0])):
        for t, want in enumerate(_want_chunks(D, rows)):
            assert np.array_equal(_u32(got[t][1][i]), _u32(want)), (i, t)      # (every frame is suppressed once, when it is computed)
    end = st.denoise_state(slots)
    assert torch.equal(end, torch.cat([e1, e3]))
    # a reset without the front-end keeps the state, one with it restarts; the setting survives both
    st.reset(slots, which=7)
    assert torch.equal(st.denoise_state(slots), end)
    st.reset(slots, which=15)
    st.set_reference(slots, _ref(2))
    assert torch.equal(st.denoise_state(slots), zero) and st.denoise([3]) == [_lib.denoise_keywords(c2)]
    _, again = _calls(st, slots, wav[:, :3 * L + 5])
    whole = full.mel_denoise(full.wav2mel(wav[:, :3 * L + 5]), cfg=c2)
    for i in range(2):
        for t, want in enumerate(_want_chunks(whole[i], rows)):
            assert np.array_equal(_u32(again[t][1][i]), _u32(want)), (i, t)
    # off and on again restarts
    st.set_denoise([1], None)
    st.set_denoise([1], cfg=c1)
    assert torch.equal(st.denoise_state([1]), zero[:1])
    st.close()


def test_hand_over_continues_bit_for_bit(full):
    slots, dst = [1, 4], [3, 0]
    wav = _wav(2, 7 * L + 123, 21)
    kw = dict(rise_db=0.02, close_db=1.0)      # slow laws: the cut falls inside their memory
    a = _open(full, slots)
    _on(a, slots, **kw)
    (cw, mw, ww), gw = _calls(a, slots, wav)
    end = a.denoise_state(slots)
    a.reset(slots, which=15)
    a.set_reference(slots, _ref(2))
    cut = 4      # calls before the export: chunks 0 .. 2 are out
    b = full.streams(MAX_SLOTS, 4, 64)
    lid, nbytes = b.layout_id, b.snapshot_bytes
    assert (a.layout_id, a.snapshot_bytes) == (lid, nbytes)      # the feature changes neither
    for k in range(cut):
        a.step_wav(slots, wav[:, k * L:(k + 1) * L])
    states = a.denoise_state(slots)
    snap = a.export_slots(slots)
    b.import_slots(dst, snap)
    assert b.denoise(dst) == [None, None]      # a snapshot carries neither the setting nor the state
    b.set_denoise(dst, seed=states, reseed=True, **kw)
    assert (b.layout_id, b.snapshot_bytes) == (lid, nbytes)
    assert torch.equal(b.denoise_state(dst), states)
    (c, m, w), g = _calls(b, dst, wav, first_call=cut)
    done = (cut - 1) * SEG
    assert torch.equal(c, cw[:, done:]) and torch.equal(m, mw[:, done:]) and np.array_equal(_u32(w), _u32(ww[:, done * HOP:]))
    assert len(g) == len(gw) - (cut - 1) and all(torch.equal(x[1], y[1]) for x, y in zip(g, gw[cut - 1:]))
    assert torch.equal(b.denoise_state(dst), end) and not torch.equal(end, states)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------ 5. errors

def test_errors_change_nothing(full):
    slots = [0, 2]
    st = _open(full, slots)
    with pytest.raises(_lib.ConanError) as e:      # the state query on a stream-set that never enabled the feature
        st.denoise_state([0])
    assert e.value.code == _lib.ERR_STATE
    st.set_denoise([0], depth_db=12.0)
    st.step_wav(slots, _wav(2, L, 5))
    st.step_wav(slots, _wav(2, L, 6))
    before, bytes_before, state = st.denoise(range(MAX_SLOTS)), st.state_bytes, st.denoise_state([0])
    assert before[0] is not None and before[1:] == [None] * (MAX_SLOTS - 1) and R.state_from(state[0].cpu().numpy().tobytes())["frames"] > 0
    for field, value in BAD:
        c = _lib.denoise_cfg()
        if field == "reserved":
            c.reserved[value] = 1
        else:
            setattr(c, field, value)
        with pytest.raises(_lib.ConanError) as e:
            st.set_denoise([0, 2, 3], cfg=c)
        assert e.value.code == _lib.ERR_INVALID, (field, value)
    for bad_slots in ([2, 2], [1, MAX_SLOTS], [-1]):
        with pytest.raises(_lib.ConanError) as e:
            st.set_denoise(bad_slots)
        assert e.value.code == _lib.ERR_INVALID
    assert st.lib.conan_streams_set_denoise(st.h, None, 1, C.byref(_lib.denoise_cfg()), None, 0, None) == _lib.ERR_INVALID      # a null argument
    assert st.lib.conan_streams_denoise_state(st.h, (C.c_int32 * 1)(0), 1, None, STATE, None) == _lib.ERR_INVALID
    seed = torch.zeros(1, STATE + 8, dtype=torch.uint8, device="cuda")
    assert st.lib.conan_streams_set_denoise(st.h, (C.c_int32 * 1)(0), 1, C.byref(_lib.denoise_cfg()), C.c_void_p(seed.data_ptr() + 4), STATE, None) == _lib.ERR_INVALID
    assert st.lib.conan_streams_set_denoise(st.h, (C.c_int32 * 1)(0), 1, C.byref(_lib.denoise_cfg()), C.c_void_p(seed.data_ptr()), STATE - 8, None) == _lib.ERR_INVALID
    assert st.denoise(range(MAX_SLOTS)) == before and st.state_bytes == bytes_before and torch.equal(st.denoise_state([0]), state)
    with pytest.raises(_lib.ConanError) as e:      # a slot without the feature in the state query
        st.denoise_state([0, 2])
    assert e.value.code == _lib.ERR_STATE
    x = torch.zeros(2, 3, 80, device="cuda")
    with pytest.raises(ValueError):
        full.mel_denoise(x, lens=[3, 4])
    with pytest.raises(_lib.ConanError) as e:
        full.mel_denoise(torch.zeros(1, 2, 257, device="cuda"))
    assert e.value.code == _lib.ERR_INVALID
    st.close()
    # a stream-set without the streaming front-end
    hp, sd_np, _ = P.model()
    ctx = Context(hp, None, 0, emformer=False, conan=True, hifigan=False)
    ctx.load_state_dict("conan", sd_np)
    ctx.finalize()
    dec = ctx.streams(2, 4, 64)
    with pytest.raises(_lib.ConanError) as e:
        dec.set_denoise([0])
    assert e.value.code == _lib.ERR_STATE
    dec.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ 6. enrolment

def test_enroll_wav_denoise(full):
    clips = _wav(2, 5 * L + 40, 44)
    via = full.streams(MAX_SLOTS, 4, 64)
    bank = VoiceBank(full, 4, 64)
    bank.enroll_wav([0, 1], clips, via=via, denoise=True)
    mel = full.wav2mel(clips)
    clean = full.mel_denoise(mel)
    assert not torch.equal(clean, mel)
    bank.enroll([2, 3], clean, via=via)
    sets = bank.export([0, 1]), bank.export([2, 3])
    torch.cuda.synchronize()
    assert torch.equal(sets[0].blob, sets[1].blob)
    bank.enroll_wav([0], clips[:1], via=via, denoise=dict(depth_db=6.0))
    bank.enroll([2], full.mel_denoise(mel[:1], depth_db=6.0), via=via)
    assert torch.equal(bank.export([0]).blob, bank.export([2]).blob) and not torch.equal(bank.export([0]).blob, sets[0].blob[:1])
    bank.close(); via.close()
