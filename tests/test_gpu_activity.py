"""Source activity on the GPU (conan_activity, conan_activity_gate, conan_streams_set_activity, conan_step_wav_activity;
include/conan_hip.h, conan_activity_cfg): the detector and the gate against tests/activity_ref.py, the streamed form against the
whole-signal one, the gate inside the chunk step, and the feature against itself - neighbours keep their bits and launches, pipelined
equals blocking, live changes, the hand-over, errors.  Every comparison is bit for bit: the law is integer operations and single
correctly rounded IEEE operations in a fixed order, so the feature has no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

from conan_amd import _lib
from conan_amd.engine import StreamingVoiceConversionEngine
from conan_amd.runtime import Context
from tests import activity_ref as A
from tests import pitch_ref as P
from tests.test_gpu_f0 import _launches, _open, _ragged, _ref, _run
from tests.test_gpu_pitch import full  # noqa: F401  (module fixture: the small synthetic full model)

pytestmark = pytest.mark.gpu

HOP, SEG = 320, 4
L = SEG * HOP
MAX_SLOTS = 6
FULL = A.FULL
# a detector that opens and closes inside utterances of a few chunks: one frame of hangover, attack in two frames, release in three
KW = dict(hold_frames=1, attack_frames=2, release_frames=3)
KW2 = dict(hold_frames=0, attack_frames=1, release_frames=2, open_db=-45.0, closed_db=-20.0)


def _sig(B, N, seed):
    """Noise of rms 1e-3 with two-harmonic bursts of 3 .. 5 frames every 6 .. 9 frames, other places per row: flags that change inside
    every utterance of the tests below."""
    rng = np.random.default_rng(seed)
    x = 1e-3 * rng.standard_normal((B, N))
    t = np.arange(N) / 16000.0
    for b in range(B):
        p = int(rng.integers(0, 3)) * HOP
        while p < N:
            q = min(N, p + int(rng.integers(3, 6)) * HOP)
            x[b, p:q] += 0.2 * np.sin(2 * np.pi * (130 + 17 * b) * t[p:q]) + 0.1 * np.sin(2 * np.pi * (260 + 34 * b) * t[p:q])
            p = q + int(rng.integers(3, 5)) * HOP
    return x.astype(np.float32)


def _wav(B, N, seed):
    return torch.from_numpy(_sig(B, N, seed)).cuda()


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _same_state(got, ref):
    return all(got[k] == (float(ref[k]) if k == "floor" else int(ref[k])) for k in A.STATE)


def _check_whole(ctx, x, cfg, fft, ref_power=None):
    """Context.activity(power=True) of rows x [n, N] against the reference, bit for bit; -> the reference's counts per row."""
    act, lvl, state, pw = ctx.activity(torch.from_numpy(x).cuda(), cfg=cfg, power=True, fft_size=fft)
    act, lvl, pw = act.cpu().numpy(), lvl.cpu().numpy(), pw.cpu().numpy()
    counts = []
    for i in range(x.shape[0]):
        Pw = A.powers(x[i], fft, HOP) if ref_power is None else ref_power[i]
        a, l, st, cn = A.detect(Pw, A.params(cfg), A.seed_state(cfg))
        assert np.array_equal(_bits(pw[i]), _bits(Pw)), (fft, x.shape, i)
        assert np.array_equal(act[i], a) and np.array_equal(lvl[i], l), (fft, x.shape, i)
        assert _same_state(state[i], st), (state[i], st)
        counts.append(cn)
    return counts


# ------------------------------------------------------------------------------------------------------------------ 1. the law

COUNTS = [1, 319, 320, 321, 63 * 320, 64 * 320 + 7, 255 * 320, 256 * 320, 257 * 320, 1000 * 320 - 1]


def _cfgs():
    return [_lib.activity_cfg(),
            _lib.activity_cfg(open_db=-70.0, close_db=-75.0, floor_db=-38.0),      # the ratio governs
            _lib.activity_cfg(hold_frames=0, up_step=FULL // 3, down_step=FULL // 7 + 1, closed_level=1 << 16)]


@pytest.mark.parametrize("fft", [64, 256, 1024])
def test_the_law_against_the_reference(full, fft):
    base = [np.tile(A.burst_signal(noise=nz, seed=s), 5)[:1000 * 320] for nz, s in ((1e-3, 0), (1e-2, 1))]
    seen = dict(openings=0, closings=0, hangover=0, clamps=0, ratio_openings=0)
    for n in COUNTS:
        powers = [A.powers(b[:n], fft, HOP) for b in base]      # once per (fft, length): the three cfgs share them
        for k, cfg in enumerate(_cfgs()):
            row = 1 if k == 1 else 0
            for cn in _check_whole(full, base[row][None, :n], cfg, fft, [powers[row]]):
                for key in seen:
                    seen[key] += cn[key]
    assert all(v >= 1 for v in seen.values()), seen      # every branch of the law was taken
    # a row run alone equals the same row run in a batch
    n = 64 * 320 + 7
    x = np.stack([base[0][o:o + n] for o in (0, 4321, 30000)])
    cfg = _cfgs()[0]
    _check_whole(full, x, cfg, fft)
    xa = torch.from_numpy(x).cuda()
    a = full.activity(xa, cfg=cfg, power=True, fft_size=fft)
    b = full.activity(xa[1:2], cfg=cfg, power=True, fft_size=fft)
    assert torch.equal(a[0][1:2], b[0]) and torch.equal(a[1][1:2], b[1]) and torch.equal(a[3][1:2], b[3]) and a[2][1] == b[2][0]


# ------------------------------------------------------------------------------------------------------------------ 2. the gate

@pytest.mark.parametrize("N", [5 * HOP + 123, 8 * HOP, 1723, 3])
def test_activity_gate_against_the_gain_law(full, N):
    rng = np.random.default_rng(N)
    F = -(-N // HOP)
    x = rng.standard_normal((3, N)).astype(np.float32)
    lv = rng.integers(0, FULL + 1, size=(3, F + 2)).astype(np.int32)      # (a stride wider than the frames)
    lv[1, :] = FULL
    lv[2, :F // 2] = FULL
    for start in (12345, FULL):
        want = np.stack([A.gate(x[i], lv[i], start, HOP) for i in range(3)])
        xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(lv).cuda()
        y = full.activity_gate(xd, ld, start_level=start)
        assert np.array_equal(y.cpu().numpy().view(np.uint32), want.view(np.uint32)), (N, start)
        z = xd.clone()
        assert full.activity_gate(z, ld, start_level=start, out=z) is z      # out == wav
        assert torch.equal(z, y)
    assert np.array_equal(want[1].view(np.uint32), x[1].view(np.uint32))      # an open gate keeps the samples' bits


# ------------------------------------------------------------------------------------------------------------------ 3. streaming = whole signal

def _log(log):
    return torch.cat([a for a, _ in log], -1), torch.cat([l for _, l in log], -1)


@pytest.mark.parametrize("N", [3 * L, 3 * L + 1, 2 * L + 319, 2 * L + 320, 700])
def test_streamed_flags_equal_the_whole_signal(full, N):
    B = 2
    wav = _wav(B, N, 20 + N % 7)
    eng = StreamingVoiceConversionEngine(full, B, max_ref_frames=64)
    log = []
    eng.infer_wav(wav, _ref(B), pipelined=False, activity=[dict(KW), dict(KW2, gate=False)], activity_log=log)
    act, lvl = _log(log)
    for i, kw in enumerate((dict(KW), dict(KW2, gate=False))):
        a, l, st = full.activity(wav[i:i + 1], **kw)
        assert act.shape[1] == 1 + N // HOP
        assert torch.equal(act[i:i + 1], a) and torch.equal(lvl[i:i + 1], l), (N, i)
        assert eng.st.activity_state([i]) == st
        assert eng.st.activity([i]) == [_lib.activity_keywords(_lib.activity_cfg(**kw))]
    assert N < L or 0 < int(act.sum()) < act.numel()
    eng.st.close()


def test_staggered_flags_equal_the_whole_signal(full):
    eng = StreamingVoiceConversionEngine(full, 3, max_ref_frames=64)
    wavs = [_wav(1, n, 30 + i)[0] for i, n in enumerate((4 * L + 333, 3 * L, 2 * L + 1))]
    for pipelined in (False, True):
        log = []
        eng.infer_wav_staggered(wavs, [0, 1, 3], _ref(3), pipelined=pipelined, activity=[dict(KW), "detect", dict(KW2)], activity_log=log)
        for u, kw in enumerate((dict(KW), dict(gate=False), dict(KW2))):
            a, l, st = full.activity(wavs[u][None], **kw)
            act, lvl = _log(log[u])
            assert torch.equal(act, a[0]) and torch.equal(lvl, l[0]), (pipelined, u)
            assert eng.st.activity_state([eng.staggered_slots[u]]) == st
    eng.st.close()


def test_flags_are_of_the_levelled_resampled_samples(full):
    B, rate = 2, 8000
    lin = L * rate // 16000
    N = 3 * lin + 41
    wav = _wav(B, N, 41)      # (read at 8 kHz: the bursts last twice as long)
    eng = StreamingVoiceConversionEngine(full, B, max_ref_frames=64)
    log = []
    eng.infer_wav(wav, _ref(B), pipelined=False, in_rate=rate, level=dict(target=-26.0), activity=dict(KW), activity_log=log)
    act, lvl = _log(log)
    x = full.level(full.resample(wav, rate, 16000), target=-26.0)
    a, l, st = full.activity(x, **KW)
    assert torch.equal(act, a) and torch.equal(lvl, l)
    assert eng.st.activity_state([0, 1]) == st
    eng.st.close()


# ------------------------------------------------------------------------------------------------------------------ 4. the gate in the step

def _gated(w, lvl, start):
    return np.stack([A.gate(w[i], lvl[i], start[i], HOP) for i in range(w.shape[0])])


@pytest.mark.parametrize("form", ["plain", "out_rate", "s16"])
def test_mode_2_audio_is_the_gain_law_on_mode_1_audio(full, form):
    B = 2
    N = 5 * L + 321      # the final chunk is short: 2 frames
    wav = _wav(B, N, 50)
    kws = [dict(KW), dict(KW2)]
    eng = StreamingVoiceConversionEngine(full, B, max_ref_frames=64)
    log = []
    w1, m1, c1 = eng.infer_wav(wav, _ref(B), pipelined=False, activity=[dict(k, gate=False) for k in kws], activity_log=log)
    torch.cuda.synchronize()
    act, lvl = _log(log)
    assert w1.shape[1] == (1 + N // HOP) * HOP and len(log[-1][0][0]) == 2
    start = [_lib.activity_cfg(**k).seed.level for k in kws]
    want = _gated(w1.cpu().numpy(), lvl.cpu().numpy(), start)
    assert not np.array_equal(want, w1.cpu().numpy())
    if form == "plain":
        for pipelined in (False, True):
            w2, m2, c2 = eng.infer_wav(wav, _ref(B), pipelined=pipelined, activity=kws)
            torch.cuda.synchronize()
            assert torch.equal(m2, m1) and torch.equal(c2, c1)
            assert np.array_equal(w2.cpu().numpy().view(np.uint32), want.view(np.uint32)), pipelined
    elif form == "out_rate":
        w2, _, _ = eng.infer_wav(wav, _ref(B), pipelined=False, out_rate=24000, activity=kws)      # (steps plus the flush)
        torch.cuda.synchronize()
        assert torch.equal(w2, full.resample(torch.from_numpy(want).cuda(), 16000, 24000))
    else:
        w2, _, _ = eng.infer_wav(wav, _ref(B), pipelined=False, out_format="s16", activity=kws)
        torch.cuda.synchronize()
        assert w2.dtype == torch.int16 and torch.equal(w2, full.convert_samples(torch.from_numpy(want).cuda(), "f32", "s16"))
    eng.st.close()


# ------------------------------------------------------------------------------------------------------------------ 5. neighbours

def test_neighbours_keep_their_bits_and_launches(full):
    slots = [0, 1, 2, 3]
    wav = _wav(4, 3 * L + 77, 60)
    a, b, d = _open(full, slots), _open(full, slots), _open(full, slots)
    bytes_never = b.state_bytes
    a.set_activity([0], **KW)
    a.set_activity([2], gate=False, **KW)
    d.set_activity([1, 3], gate=False)
    state = MAX_SLOTS * C.sizeof(_lib.ActivityState) + 8 * MAX_SLOTS * (2 * SEG + 1) * 4 + 8 * MAX_SLOTS * 176
    assert a.state_bytes == bytes_never + state      # the state, the staging sets and the row tables, from the first enabling call on
    ((ca, ma, wa, _, _), emits), la = _launches(a, lambda: _run(a, slots, wav, contour=False))
    ((cb, mb, wb, _, _), _), lb = _launches(b, lambda: _run(b, slots, wav, contour=False))
    ((cd, md, wd, _, _), _), ld = _launches(d, lambda: _run(d, slots, wav, contour=False))
    assert torch.equal(ca, cb) and torch.equal(ma, mb)      # the detector touches no model input
    for i in (1, 2, 3):
        assert torch.equal(wa[i], wb[i]), i      # ungated rows keep their bits, also the detect-only row
    assert not torch.equal(wa[0], wb[0])
    assert torch.equal(wd, wb)
    # a stream-set that never calls the setter runs the launches it ran before; mode 1 adds one per emitting call, mode 2 one more per
    # vocoder step
    assert "activity_kernel" not in lb and "activity_gate_kernel" not in lb
    assert ld.pop("activity_kernel") == len(emits) and ld == lb, (ld, lb)
    assert la.pop("activity_kernel") == len(emits) and la.pop("activity_gate_kernel") == len(emits) and la == lb, (la, lb)
    # off again: the launches of the stream-set that never detected
    a.set_activity(slots, None)
    assert a.activity(slots) == [None] * 4
    a.reset(slots, which=15)
    a.set_reference(slots, _ref(4))
    ((_, m2, w2, _, _), _), l2 = _launches(a, lambda: _run(a, slots, wav, contour=False))
    assert l2 == lb and torch.equal(m2, mb) and torch.equal(w2, wb)
    for s_ in (a, b, d):
        s_.close()


def test_ragged_groups_gate_only_where_a_gated_row_takes_part(full):
    """A ragged call's emit groups are separate vocoder steps: one gate launch per step with a gated row, none for the others."""
    slots, starts = [5, 0, 2], [0, 1, 3]
    wavs = [_wav(1, n, 65 + i)[0] for i, n in enumerate((4 * L + 333, 3 * L, 2 * L + 1))]
    plain = _open(full, slots)
    want = _ragged(plain, slots, wavs, starts, contour=False)
    plain.close()
    st = _open(full, slots)
    st.set_activity([5], **KW)
    st.set_activity([0], gate=False, **KW)
    got, lg = _launches(st, lambda: _ragged(st, slots, wavs, starts, contour=False))
    for u in (1, 2):
        assert all(torch.equal(got[u][i], want[u][i]) for i in range(3)), u
    assert torch.equal(got[0][1], want[0][1]) and not torch.equal(got[0][2], want[0][2])
    a, l, _ = full.activity(wavs[0][None], **KW)
    w = A.gate(want[0][2].cpu().numpy(), l[0].cpu().numpy(), 0, HOP)
    assert np.array_equal(got[0][2].cpu().numpy().view(np.uint32), w.view(np.uint32))
    chunks0 = -(-(1 + wavs[0].shape[0] // HOP) // SEG)      # slot 5's emitting calls: each has one group with the gated row
    assert lg["activity_gate_kernel"] == chunks0
    st.close()


# ------------------------------------------------------------------------------------------------------------------ 6. pipelined = blocking

def test_pipelined_equals_blocking(full):
    slots = [2, 5]
    wav = _wav(2, 13 * L + 77, 70)
    st = _open(full, slots)
    st.set_activity([2], **KW)
    st.set_activity([5], **KW2)
    (cb, mb, wb, _, _), eb = _run(st, slots, wav, contour=False)
    assert len(eb) >= 12
    state = st.activity_state(slots)
    st.reset(slots, which=15)
    st.set_reference(slots, _ref(2))
    (cp, mp, wp, _, _), ep = _run(st, slots, wav, pipelined=True, contour=False)
    assert ep == eb and torch.equal(cp, cb) and torch.equal(mp, mb) and torch.equal(wp, wb)
    assert st.activity_state(slots) == state
    _, lvl, _ = full.activity(wav[0:1], **KW)
    assert 0 < int((lvl < FULL).sum()) < lvl.numel()      # the gate moved
    st.close()


def test_pipelined_ragged_equals_blocking(full):
    slots, starts = [5, 0, 2], [0, 2, 5]
    wavs = [_wav(1, n, 80 + i)[0] for i, n in enumerate((13 * L + 5, 12 * L, 9 * L + 400))]
    outs = []
    for pipelined in (False, True):
        st = _open(full, slots)
        st.set_activity([5, 2], **KW)
        outs.append(_ragged(st, slots, wavs, starts, pipelined=pipelined, contour=False))
        outs[-1].append(st.activity_state([5, 2]))
        st.close()
    assert outs[0][3] == outs[1][3]
    for u in range(3):
        for i in range(3):
            assert torch.equal(outs[0][u][i], outs[1][u][i]), (u, i)


# ------------------------------------------------------------------------------------------------------------------ 7. live changes, restart

def _run_act(st, slots, wav, on_call=None, first_call=0):
    """The blocking calls of infer_wav from call `first_call` on -> (codes, mel, wav, act, level) over the emitted chunks."""
    n, N = wav.shape
    last = (N - 1) // L * L
    calls = ([(p, p + L, False) for p in range(0, last, L)] + [(last, N, True)])[first_call:]
    outs, k = [], first_call
    while True:
        if on_call:
            on_call(k)
        if calls:
            a, b, fin = calls.pop(0)
            e, c, m, w = st.step_wav(slots, wav[:, a:b], final=fin)
        else:
            e, c, m, w = st.step_wav(slots, wav[:, :0], final=True)
            if e == 0:
                break
        k += 1
        if e:
            fl, lv = st.step_wav_activity()
            assert not fl[:, e:].any() and not lv[:, e:].any()      # entries past the emitted frames are zero
            outs.append((c[:, :e].clone(), m.clone(), w.clone(), fl[:, :e].clone(), lv[:, :e].clone()))
    torch.cuda.synchronize()
    return [torch.cat([o[i] for o in outs], 1) for i in range(5)]


def test_live_changes_and_restarts(full):
    slots = [1, 3]
    N = 9 * L + 10
    wav = _wav(2, N, 90)
    x = wav.cpu().numpy()
    c1, c2 = _lib.activity_cfg(**KW), _lib.activity_cfg(open_db=-12.0, close_db=-14.0, **KW)
    st = _open(full, slots)

    def on_call(k):      # before call k (call k emits chunk k - 1)
        if k == 3:
            st.set_activity(slots, **KW)                                      # mid-utterance: from the seed, at chunk 2
            assert st.activity_state(slots) == [_lib.activity_state_dict(c1.seed)] * 2      # a pending restart reports the seed
        elif k == 6:
            st.set_activity(slots, open_db=-12.0, close_db=-14.0, **KW)       # reseed = 0: new thresholds, the state stays

    _, _, _, act, lvl = _run_act(st, slots, wav, on_call=on_call)
    act, lvl = act.cpu().numpy(), lvl.cpu().numpy()
    F = 1 + N // HOP
    changed = False
    for i in range(2):
        assert not act[i, :2 * SEG].any() and not lvl[i, :2 * SEG].any()      # rows without the detector read zero
        r1 = A.run(x[i], c1, f0=2 * SEG, count=3 * SEG)
        r2 = A.run(x[i], c2, state=r1["state"], f0=5 * SEG, count=F - 5 * SEG)
        keep = A.run(x[i], c1, state=r1["state"], f0=5 * SEG, count=F - 5 * SEG)
        assert np.array_equal(act[i, 2 * SEG:5 * SEG], r1["act"]) and np.array_equal(lvl[i, 2 * SEG:5 * SEG], r1["level"]), i
        assert np.array_equal(act[i, 5 * SEG:], r2["act"]) and np.array_equal(lvl[i, 5 * SEG:], r2["level"]), i
        assert _same_state(st.activity_state([slots[i]])[0], r2["state"])
        changed = changed or not np.array_equal(r2["act"], keep["act"])
    assert changed      # (the new thresholds decide otherwise somewhere)
    # a reset with the front-end restarts from the seed (the cfg in force: c2); one without it does not
    before = st.activity_state(slots)
    st.reset(slots, which=7)
    assert st.activity_state(slots) == before
    st.reset(slots, which=15)
    st.set_reference(slots, _ref(2))
    assert st.activity_state(slots) == [_lib.activity_state_dict(c2.seed)] * 2
    _, _, _, act, lvl = _run_act(st, slots, wav)
    a, l, state = full.activity(wav, cfg=c2)
    assert torch.equal(act, a) and torch.equal(lvl, l) and st.activity_state(slots) == state
    # reseed = 1 on an enabled slot restarts too
    st.set_activity([1], reseed=True, **KW)
    assert st.activity_state(slots) == [_lib.activity_state_dict(c1.seed), state[1]]
    st.close()


# ------------------------------------------------------------------------------------------------------------------ 8. the hand-over

def test_hand_over_continues_bit_for_bit(full):
    slots, dst = [1, 4], [3, 0]
    wav = _wav(2, 7 * L + 123, 100)
    a = _open(full, slots)
    a.set_activity(slots, **KW)
    cw, mw, ww, fw, lw = _run_act(a, slots, wav)
    a.reset(slots, which=15)
    a.set_reference(slots, _ref(2))
    cut = 4      # calls before the export: chunks 0 .. 2 are out
    b = full.streams(MAX_SLOTS, 4, 64)
    lid, nbytes = b.layout_id, b.snapshot_bytes
    assert (a.layout_id, a.snapshot_bytes) == (lid, nbytes)      # the feature changes neither
    for k in range(cut):
        a.step_wav(slots, wav[:, k * L:(k + 1) * L])
    states = a.activity_state(slots)
    snap = a.export_slots(slots)
    b.import_slots(dst, snap)
    assert b.activity(dst) == [None, None]      # a snapshot carries neither the setting nor the state
    for d, s in zip(dst, states):
        b.set_activity([d], seed=s, reseed=True, **KW)
    assert (b.layout_id, b.snapshot_bytes) == (lid, nbytes)
    c, m, w, fl, lv = _run_act(b, dst, wav, first_call=cut)
    done = (cut - 1) * SEG
    assert torch.equal(c, cw[:, done:]) and torch.equal(m, mw[:, done:]) and torch.equal(w, ww[:, done * HOP:])
    assert torch.equal(fl, fw[:, done:]) and torch.equal(lv, lw[:, done:])
    assert b.activity_state(dst) == full.activity(wav, **KW)[2]
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------ 9. errors

def test_errors_change_nothing(full):
    slots = [0, 2]
    st = _open(full, slots)
    st.set_activity([0], **KW)
    before = st.activity(range(MAX_SLOTS))
    inf, nan = float("inf"), float("nan")
    bad = [("mode", 3), ("mode", -1), ("reseed", 2), ("open_abs", nan), ("close_abs", -1e-9), ("close_abs", 1.0), ("open_ratio", inf),
           ("close_ratio", -1.0), ("close_ratio", 100.0), ("rise_active", 0.99), ("rise_idle", nan), ("floor_min", 0.0), ("floor_min", 1.0),
           ("hold_frames", -1), ("hold_frames", FULL + 1), ("up_step", 0), ("up_step", FULL + 1), ("down_step", 0), ("down_step", FULL + 1),
           ("closed_level", -1), ("closed_level", FULL), ("reserved", 1)]
    seeds = [("level", FULL + 1), ("level", -1), ("floor", 0.0), ("floor", nan), ("reserved", 7), ("active", 2), ("hang", -1), ("frames", -1),
             ("active_frames", 5)]
    cfgs = []
    for field, value in bad:
        c = _lib.activity_cfg()
        setattr(c, field, value)
        cfgs.append(c)
    for field, value in seeds:
        c = _lib.activity_cfg()
        setattr(c.seed, field, value)
        cfgs.append(c)
    c = _lib.activity_cfg(closed_level=1 << 10)
    c.seed.level = 5      # under closed_level
    cfgs.append(c)
    x = _wav(1, 700, 1)
    for c in cfgs:
        with pytest.raises(_lib.ConanError) as e:
            st.set_activity([2, 3], cfg=c)
        assert e.value.code == _lib.ERR_INVALID
        if c.mode in (1, 2):
            with pytest.raises(_lib.ConanError) as e:
                full.activity(x, cfg=c)
            assert e.value.code == _lib.ERR_INVALID
    for bad_slots in ([2, 2], [1, MAX_SLOTS], [-1]):
        with pytest.raises(_lib.ConanError) as e:
            st.set_activity(bad_slots)
        assert e.value.code == _lib.ERR_INVALID
    assert st.activity(range(MAX_SLOTS)) == before
    with pytest.raises(_lib.ConanError) as e:      # a slot without the feature in the state query
        st.activity_state([0, 2])
    assert e.value.code == _lib.ERR_STATE
    with pytest.raises(_lib.ConanError) as e:      # no wav-in call yet
        st.step_wav_activity()
    assert e.value.code == _lib.ERR_STATE
    with pytest.raises(_lib.ConanError) as e:
        full.activity_gate(x, torch.zeros(1, 2, dtype=torch.int32, device="cuda"))      # 700 samples are 3 frames
    assert e.value.code == _lib.ERR_INVALID
    # a frame whose chunk has left the audio ring when it is emitted: the bound of following
    big = dict(fft_size=2048, win_length=2048)
    with pytest.raises(_lib.ConanError) as e:
        for k in range(6):
            st.step_wav(slots, _wav(2, L, 111 + k), mel=big)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    st.close()
    # a stream-set without the streaming front-end
    hp, sd_np, _ = P.model()
    ctx = Context(hp, None, 0, emformer=False, conan=True, hifigan=False)
    ctx.load_state_dict("conan", sd_np)
    ctx.finalize()
    dec = ctx.streams(2, 4, 64)
    with pytest.raises(_lib.ConanError) as e:
        dec.set_activity([0])
    assert e.value.code == _lib.ERR_STATE
    dec.close()
    ctx.close()
