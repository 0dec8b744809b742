"""Source bypass on the GPU (conan_streams_set_bypass, conan_step_wav_bypass, conan_bypass_mix; include/conan_hip.h,
conan_bypass_cfg): the mix against tests/bypass_ref.py, the alignment of the dry path with the output, the mix inside the chunk step,
and the feature against itself - neighbours keep their bits and launches, pipelined equals blocking, the hand-over, restarts, errors.
Every comparison is bit for bit, except where full dry is compared with the source in value (the law: only the sign of a zero can
differ): the law is integer operations and single correctly rounded IEEE operations in a fixed order."""
import ctypes as C

import numpy as np
import pytest
import torch

from conan_amd import _lib
from conan_amd.engine import StreamingVoiceConversionEngine
from conan_amd.runtime import Context
from tests import activity_ref as A
from tests import bypass_ref as B
from tests import pitch_ref as P
from tests.test_bypass_cpu import BAD
from tests.test_gpu_f0 import _launches, _open, _ragged, _ref, _run
from tests.test_gpu_pitch import full  # noqa: F401  (module fixture: the small synthetic full model)

pytestmark = pytest.mark.gpu

HOP, SEG = 320, 4
L = SEG * HOP
MAX_SLOTS = 6
FULL = B.FULL
KW = dict(hold_frames=1, attack_frames=2, release_frames=3)      # the activity tests' detector: it opens and closes within a few chunks
DRY = dict(wet=0.0, dry=1.0, start=(0, FULL))                    # the source alone, from the first sample on


def _noise(n, N, seed, amp=0.1):
    return torch.from_numpy((amp * np.random.default_rng(seed).standard_normal((n, N))).astype(np.float32)).cuda()


def _bursts(n, seed):
    """Rows cut out of the activity tests' burst signal: the gate moves inside a few chunks."""
    x = A.burst_signal(noise=1e-3, seed=seed)
    return torch.from_numpy(np.stack([x[3000 + 4321 * i:3000 + 4321 * i + 9 * L + 10] for i in range(n)])).cuda()


def _u32(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.uint32)


def _padded(x):
    """x [n, N] -> [n, (1 + N // hop) * hop]: the source as the mix sees it, zeros beyond the samples received."""
    n, N = x.shape
    out = torch.zeros(n, (1 + N // HOP) * HOP, dtype=x.dtype, device=x.device)
    out[:, :N] = x
    return out


def _law(w_off, x_pad, wl, dl, start):
    """The numpy law on a run's unmixed audio w_off [n, T], the padded source and the per-frame levels [n, F]; start: (wet, dry_eff) per row."""
    w_off, x_pad, wl, dl = w_off.cpu().numpy(), x_pad.cpu().numpy(), wl.cpu().numpy(), dl.cpu().numpy()
    return np.stack([B.mix(w_off[i], x_pad[i], wl[i], dl[i], start[i][0], start[i][1], HOP) for i in range(w_off.shape[0])])


# ------------------------------------------------------------------------------------------------------------------ 1. the mix

def _level_rows(F, rng):
    ramp = np.rint(np.linspace(0, FULL, F + 1)[1:]).astype(np.int32)
    step = np.where(np.arange(F) < (F + 1) // 2, FULL // 3, FULL).astype(np.int32)
    wet = np.stack([ramp, np.full(F, FULL, np.int32), np.zeros(F, np.int32), step, rng.integers(0, FULL + 1, F).astype(np.int32)])
    dry = np.stack([ramp[::-1], np.zeros(F, np.int32), np.full(F, FULL, np.int32), FULL - step, rng.integers(0, FULL + 1, F).astype(np.int32)])
    return wet, dry


@pytest.mark.parametrize("N", [1, 319, 320, 321, 63 * 320, 64 * 320 + 7])
def test_bypass_mix_against_the_law(full, N):
    rng = np.random.default_rng(N)
    F = -(-N // HOP)      # (321 and 64 * 320 + 7 end in a partly covered frame)
    wl, dl = _level_rows(F, rng)
    n = wl.shape[0]
    y = rng.standard_normal((n, N)).astype(np.float32)
    x = (0.3 * rng.standard_normal((n, N))).astype(np.float32)
    starts = [(FULL, 0), (0, FULL), (12345, 654321)]
    yd, xd = torch.from_numpy(y).cuda(), torch.from_numpy(x).cuda()
    wld, dld = torch.from_numpy(wl).cuda(), torch.from_numpy(dl).cuda()
    for sw, sd in starts:
        want = np.stack([B.mix(y[i], x[i], wl[i], dl[i], sw, sd, HOP) for i in range(n)])
        got = full.bypass_mix(yd, xd, wld, dld, start=(sw, sd))
        assert np.array_equal(_u32(got), _u32(want)), (N, sw, sd)
        # rows at unaligned addresses and strides: views of wider buffers, each off a 16-byte boundary by another amount
        yw, xw, ow = (torch.zeros(n, N + pad, device="cuda") for pad in (5, 7, 6))
        yv, xv, ov = yw[:, 1:N + 1], xw[:, 3:N + 3], ow[:, 2:N + 2]
        yv.copy_(yd); xv.copy_(xd)
        lw = torch.zeros(n, F + 3, dtype=torch.int32, device="cuda")      # (a level stride wider than the frames)
        lv_w, lv_d = lw[:, :F], lw.clone()[:, :F]
        lv_w.copy_(wld); lv_d.copy_(dld)
        assert full.bypass_mix(yv, xv, lv_w, lv_d, start=(sw, sd), out=ov) is ov
        assert np.array_equal(_u32(ov.contiguous()), _u32(want)), (N, "views")
        assert not ow[:, :2].any() and not ow[:, N + 2:].any()      # nothing outside the rows was written
        z = yd.clone()
        assert full.bypass_mix(z, xd, wld, dld, start=(sw, sd), out=z) is z      # out == wet
        assert np.array_equal(_u32(z), _u32(want))
        assert full.bypass_mix(yv, xv, lv_w, lv_d, start=(sw, sd), out=yv) is yv      # ... also at an unaligned address
        assert np.array_equal(_u32(yv.contiguous()), _u32(want))
    got = full.bypass_mix(yd, xd, wld, dld, start=(FULL, 0))
    assert np.array_equal(_u32(got[1]), _u32(y[1]))              # full wet: the bits of wet
    got = full.bypass_mix(yd, xd, wld, dld, start=(0, FULL))
    assert np.array_equal(got[2].cpu().numpy(), x[2])            # full dry: dry, in value


# ------------------------------------------------------------------------------------------------------------------ 2. alignment

@pytest.mark.parametrize("N", [5 * L + 700, L - 1])
@pytest.mark.parametrize("form", ["plain", "in_8k", "in_48k", "level", "out_rate", "s16"])
def test_full_dry_returns_the_prepared_source(full, form, N):
    n = 2
    eng = StreamingVoiceConversionEngine(full, n, max_ref_frames=64)
    kw, src = {}, _noise(n, N, 7 + N % 5)
    if form in ("in_8k", "in_48k"):
        rate = 8000 if form == "in_8k" else 48000
        src = _noise(n, N * rate // 16000, 11)
        kw = dict(in_rate=rate)
        prepared = full.resample(src, rate, 16000)
    elif form == "level":
        kw = dict(level=dict(target=-26.0))
        prepared = full.level(src, target=-26.0)
    elif form == "s16":
        src = (src * 32767.0).round().clamp(-32768, 32767).to(torch.int16)
        kw = dict(in_format="s16", out_format="s16")
        prepared = full.convert_samples(src, "s16", "f32")
    else:
        if form == "out_rate":
            kw = dict(out_rate=24000)
        prepared = src
    want = _padded(prepared)
    for pipelined in (False, True):
        w, m, _ = eng.infer_wav(src, _ref(n), pipelined=pipelined, bypass=dict(DRY), **kw)
        torch.cuda.synchronize()
        assert m.shape[1] == 1 + prepared.shape[1] // HOP
        if form == "out_rate":
            exp = full.resample(want, 16000, 24000)      # (the steps plus the flush)
        elif form == "s16":
            exp = full.convert_samples(want, "f32", "s16")
        else:
            exp = want
        assert w.shape == exp.shape and w.dtype == exp.dtype, (form, N, w.shape, exp.shape)
        assert bool((w == exp).all()), (form, N, pipelined, int((w != exp).sum()))      # in value: out[j] == src[j], zeros behind
    assert bool((want[:, prepared.shape[1]:] == 0).all()) and bool(want.any())
    eng.st.close()


# ------------------------------------------------------------------------------------------------------------------ 3. the mix in the step

def _run_byp(st, slots, wav, on_call=None, first_call=0, gate_levels=False):
    """The blocking calls of infer_wav from call `first_call` on -> (codes, mel, wav, wet level, dry level[, gate level]) over the
    emitted chunks.  on_call(k) runs before call k (call k emits chunk k - 1)."""
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
            wl, dl = st.step_wav_bypass()
            assert not wl[:, e:].any() and not dl[:, e:].any()      # entries past the emitted frames are zero
            row = [c[:, :e].clone(), m.clone(), w.clone(), wl[:, :e].clone(), dl[:, :e].clone()]
            if gate_levels:
                row.append(st.step_wav_activity()[1][:, :e].clone())
            outs.append(row)
    torch.cuda.synchronize()
    return [torch.cat([o[i] for o in outs], 1) for i in range(len(outs[0]))]


TO_DRY = dict(wet=0.0, dry=1.0, ramp_ms=60.0)       # three frames
TO_WET = dict(wet=1.0, dry=0.25, ramp_ms=100.0)     # five frames: it crosses a chunk boundary


def _toggle(st, slots, fill):
    def on_call(k):
        if k == 3:
            st.set_bypass(slots, fill_gate=fill, **TO_DRY)      # towards dry from chunk 2 on
        elif k == 6:
            st.set_bypass(slots, fill_gate=fill, **TO_WET)      # and back from chunk 5 on
    return on_call


def _ref_levels(F, fill, gate, gate_before):
    """The law's levels of the toggled run: enabled at full wet, TO_DRY from frame 2 * SEG, TO_WET from frame 5 * SEG."""
    st = B.seed_state(FULL, 0, fill, gate_before)
    ws, ds = [], []
    for a, b, kw in ((0, 2 * SEG, dict(wet=1.0, dry=0.0, ramp_ms=40.0)), (2 * SEG, 5 * SEG, TO_DRY), (5 * SEG, F, TO_WET)):
        c = _lib.bypass_cfg(**kw)
        w, d, st = B.levels(st, c.wet_target, c.dry_target, c.step, b - a, fill, None if gate is None else gate[a:b])
        ws.append(w); ds.append(d)
    return np.concatenate(ws), np.concatenate(ds), st


@pytest.mark.parametrize("fill", [False, True])
def test_a_mid_call_toggle_is_the_law_on_the_unmixed_audio(full, fill):
    slots = [1, 3]
    wav = _bursts(2, 5) if fill else _noise(2, 9 * L + 10, 90)
    N = wav.shape[1]
    F = 1 + N // HOP
    x_pad = _padded(wav)
    st = _open(full, slots)
    if fill:
        st.set_activity(slots, **KW)      # mode 2: the unmixed audio is the audio behind the gate
    c0, m0, w0, wl0, dl0, *g0 = _run_byp(st, slots, wav, gate_levels=fill)
    assert c0.shape[1] == F and F >= 9 * SEG and not wl0.any() and not dl0.any()      # without the feature the hook reads zeros
    # enabled at full wet: the bits of the run without the feature
    st.reset(slots, which=15)
    st.set_reference(slots, _ref(2))
    st.set_bypass(slots, fill_gate=fill)
    c1, m1, w1, wl1, dl1 = _run_byp(st, slots, wav)
    assert torch.equal(c1, c0) and torch.equal(m1, m0) and np.array_equal(_u32(w1), _u32(w0))
    assert bool((wl1 == FULL).all()) and not dl1.any()
    # the toggle
    st.reset(slots, which=15)
    st.set_reference(slots, _ref(2))
    c2, m2, w2, wl, dl, *g2 = _run_byp(st, slots, wav, on_call=_toggle(st, slots, fill), gate_levels=fill)
    assert torch.equal(c2, c0) and torch.equal(m2, m0)      # the mix touches no model input
    gate_before = _lib.activity_cfg(**KW).seed.level
    for i in range(2):
        gate = g2[0][i].cpu().numpy() if fill else None
        rw, rd, rst = _ref_levels(F, fill, gate, gate_before)
        assert np.array_equal(wl[i].cpu().numpy(), rw) and np.array_equal(dl[i].cpu().numpy(), rd), i
        assert st.bypass_state([slots[i]]) == [rst]
    if fill:
        assert torch.equal(g2[0], g0[0])
        g = g2[0].cpu().numpy()
        assert 0 < int((g < FULL).sum()) < g.size      # the gate moved ...
        assert int((dl.cpu().numpy()[:, 5 * SEG + 5:] != _lib.bypass_cfg(**TO_WET).dry_target).sum()) > 0      # ... and the fill follows it
    start = [(FULL, 0)] * 2
    want = _law(w0, x_pad, wl, dl, start)
    assert np.array_equal(_u32(w2), _u32(want))
    assert not np.array_equal(_u32(w2), _u32(w0))
    # ... and conan_bypass_mix is the same mix on the whole signals
    got = full.bypass_mix(w0, x_pad, wl, dl, start=start[0])
    assert np.array_equal(_u32(got), _u32(want))
    st.close()


# ------------------------------------------------------------------------------------------------------------------ 4. neighbours

def test_neighbours_keep_their_bits_and_launches(full):
    slots = [0, 1, 2, 3]
    wav = _noise(4, 3 * L + 77, 60)
    a, b = _open(full, slots), _open(full, slots)
    bytes_never = b.state_bytes
    a.set_bypass([0], wet=0.5, dry=0.5)
    a.set_bypass([2], **DRY)
    a.set_bypass([3], wet=1.0, dry=0.5, fill_gate=True)      # a fill without a gate: the absent gate is open, nothing is filled
    state = MAX_SLOTS * C.sizeof(_lib.BypassState) + 8 * MAX_SLOTS * (2 * (SEG + 1) + SEG * HOP) * 4 + 8 * MAX_SLOTS * 80
    assert a.state_bytes == bytes_never + state      # the state, the staging sets and the row tables, from the first enabling call on
    b.set_bypass(slots, None)                         # turning off what was never on allocates nothing
    assert b.state_bytes == bytes_never and b.bypass(slots) == [None] * 4
    ((ca, ma, wa, _, _), emits), la = _launches(a, lambda: _run(a, slots, wav, contour=False))
    ((cb, mb, wb, _, _), _), lb = _launches(b, lambda: _run(b, slots, wav, contour=False))
    assert torch.equal(ca, cb) and torch.equal(ma, mb)
    for i in (1, 3):
        assert np.array_equal(_u32(wa[i]), _u32(wb[i])), i      # a row without the feature keeps its bits, and so does the unfilled one
    assert a.bypass_state([3]) == [dict(wet=FULL, dry=FULL // 2, dry_eff=0)]
    x_pad = _padded(wav)
    assert bool((wa[2] == x_pad[2]).all()) and not torch.equal(wa[0], wb[0])
    h = _lib.bypass_cfg(wet=0.5, dry=0.5)
    F = x_pad.shape[1] // HOP
    want = B.mix(wb[0].cpu().numpy(), x_pad[0].cpu().numpy(), [h.wet_target] * F, [h.dry_target] * F, h.seed_wet, h.seed_dry, HOP)
    assert np.array_equal(_u32(wa[0]), _u32(want))
    # a stream-set that never enabled it runs the launches it ran before; a bypass row adds one stage launch per emitting call and one
    # mix launch per vocoder step of its group
    assert "bypass_stage_kernel" not in lb and "bypass_mix_kernel" not in lb
    assert la.pop("bypass_stage_kernel") == len(emits) and la.pop("bypass_mix_kernel") == len(emits) and la == lb, (la, lb)
    # off again: the launches of the stream-set that never mixed
    a.set_bypass(slots, None)
    assert a.bypass(slots) == [None] * 4
    a.reset(slots, which=15)
    a.set_reference(slots, _ref(4))
    ((_, m2, w2, _, _), _), l2 = _launches(a, lambda: _run(a, slots, wav, contour=False))
    assert l2 == lb and torch.equal(m2, mb) and torch.equal(w2, wb)
    a.close(); b.close()


def test_ragged_groups_mix_only_where_a_bypass_row_takes_part(full):
    """A ragged call's emit groups are separate vocoder steps: one mix launch per step with a bypass row, none for the others."""
    slots, starts = [5, 0, 2], [0, 1, 3]
    wavs = [_noise(1, n, 65 + i)[0] for i, n in enumerate((4 * L + 333, 3 * L, 2 * L + 1))]
    plain = _open(full, slots)
    want, lp = _launches(plain, lambda: _ragged(plain, slots, wavs, starts, contour=False))
    plain.close()
    st = _open(full, slots)
    st.set_bypass([5], wet=0.25, dry=0.75)
    got, lg = _launches(st, lambda: _ragged(st, slots, wavs, starts, contour=False))
    for u in (1, 2):
        assert all(torch.equal(got[u][i], want[u][i]) for i in range(3)), u      # the other utterances keep their bits
    assert torch.equal(got[0][0], want[0][0]) and torch.equal(got[0][1], want[0][1])
    h = _lib.bypass_cfg(wet=0.25, dry=0.75)
    F = 1 + wavs[0].shape[0] // HOP
    w = B.mix(want[0][2].cpu().numpy(), _padded(wavs[0][None])[0].cpu().numpy(), [h.wet_target] * F, [h.dry_target] * F, h.seed_wet, h.seed_dry, HOP)
    assert np.array_equal(_u32(got[0][2]), _u32(w))
    chunks0 = -(-F // SEG)      # slot 5's emitting calls: each has one stage launch and one group with the bypass row
    assert lg.pop("bypass_stage_kernel") == chunks0 and lg.pop("bypass_mix_kernel") == chunks0 and lg == lp, (lg, lp)
    st.close()


# ------------------------------------------------------------------------------------------------------------------ 5. pipelined = blocking

def test_pipelined_equals_blocking(full):
    slots = [2, 5]
    wav = _bursts(2, 9)
    wav = torch.cat([wav, wav[:, :4 * L + 67]], 1)      # 13 chunks and a short one
    st = _open(full, slots)
    st.set_activity([5], **KW)

    def on_call(k):
        if k == 0:
            st.set_bypass([2], reseed=True)
            st.set_bypass([5], wet=1.0, dry=0.5, fill_gate=True, reseed=True)
        _toggle(st, [2], False)(k)

    (cb, mb, wb, _, _), eb = _run(st, slots, wav, contour=False, on_call=on_call)
    assert len(eb) >= 13
    state = st.bypass_state(slots)
    st.reset(slots, which=15)
    st.set_reference(slots, _ref(2))
    (cp, mp, wp, _, _), ep = _run(st, slots, wav, pipelined=True, contour=False, on_call=on_call)
    assert ep == eb and torch.equal(cp, cb) and torch.equal(mp, mb) and np.array_equal(_u32(wp), _u32(wb))
    assert st.bypass_state(slots) == state
    st.set_bypass(slots, None)
    st.reset(slots, which=15)
    st.set_reference(slots, _ref(2))
    (_, _, w0, _, _), _ = _run(st, slots, wav, contour=False)
    assert not torch.equal(w0[0], wb[0]) and not torch.equal(w0[1], wb[1])      # both rows were mixed
    st.close()


def test_staggered_utterances_equal_each_utterance_alone(full):
    fixed = _lib.STREAMS_FIXED_PLAN      # (a fixed plan: a row's arithmetic does not depend on the rows it shares a launch with)
    wavs = [_noise(1, n, 30 + i)[0] for i, n in enumerate((4 * L + 333, 3 * L, 2 * L + 1))]
    byp = [dict(wet=0.5, dry=0.5, start=(FULL, 0), ramp_ms=200.0), None, dict(DRY)]
    refs = _ref(3)
    eng = StreamingVoiceConversionEngine(full, 3, max_ref_frames=64, flags=fixed)
    blk = eng.infer_wav_staggered(wavs, [0, 1, 3], refs, pipelined=False, bypass=byp)
    pip = eng.infer_wav_staggered(wavs, [0, 1, 3], refs, pipelined=True, bypass=byp)
    torch.cuda.synchronize()
    eng.st.close()
    solo = StreamingVoiceConversionEngine(full, 3, max_ref_frames=64, flags=fixed)
    solo.slots = [0]
    for u in range(3):
        w, m, c = solo.infer_wav(wavs[u][None], refs[u][None], pipelined=False, bypass=byp[u])
        torch.cuda.synchronize()
        for got in (blk[u], pip[u]):
            assert torch.equal(got[1], m[0]) and torch.equal(got[2], c[0]) and np.array_equal(_u32(got[0]), _u32(w[0])), u
    assert bool((blk[2][0] == _padded(wavs[2][None])[0]).all())
    solo.st.close()


# ------------------------------------------------------------------------------------------------------------------ 6. the hand-over

def test_hand_over_continues_bit_for_bit(full):
    slots, dst = [1, 4], [3, 0]
    wav = _bursts(2, 21)[:, :7 * L + 123]
    kw = dict(wet=0.2, dry=0.8, ramp_ms=400.0, fill_gate=True)      # twenty frames: the cut falls inside the ramp
    a = _open(full, slots)
    a.set_activity(slots, **KW)
    a.set_bypass(slots, start=(FULL, 0), **kw)
    cw, mw, ww, wlw, dlw = _run_byp(a, slots, wav)
    a.reset(slots, which=15)
    a.set_reference(slots, _ref(2))
    cut = 4      # calls before the export: chunks 0 .. 2 are out
    b = full.streams(MAX_SLOTS, 4, 64)
    lid, nbytes = b.layout_id, b.snapshot_bytes
    assert (a.layout_id, a.snapshot_bytes) == (lid, nbytes)      # the feature changes neither
    for k in range(cut):
        a.step_wav(slots, wav[:, k * L:(k + 1) * L])
    states, acts = a.bypass_state(slots), a.activity_state(slots)
    assert all(0 < s["wet"] < FULL and 0 < s["dry"] < FULL for s in states)      # mid-ramp
    snap = a.export_slots(slots)
    b.import_slots(dst, snap)
    assert b.bypass(dst) == [None, None]      # a snapshot carries neither the setting nor the state
    for d, s, sa in zip(dst, states, acts):
        b.set_activity([d], seed=sa, reseed=True, **KW)
        b.set_bypass([d], start=(s["wet"], s["dry"]), reseed=True, **kw)
    assert (b.layout_id, b.snapshot_bytes) == (lid, nbytes)
    c, m, w, wl, dl = _run_byp(b, dst, wav, first_call=cut)
    done = (cut - 1) * SEG
    assert torch.equal(c, cw[:, done:]) and torch.equal(m, mw[:, done:]) and np.array_equal(_u32(w), _u32(ww[:, done * HOP:]))
    assert torch.equal(wl, wlw[:, done:]) and torch.equal(dl, dlw[:, done:])
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------ 7. restarts, errors

def test_restarts(full):
    slots = [1, 3]
    wav = _noise(2, 3 * L + 10, 95)
    kw = dict(wet=0.0, dry=1.0, ramp_ms=160.0, start=(FULL, 1000))      # eight frames
    c = _lib.bypass_cfg(**kw)
    seed = dict(wet=FULL, dry=1000, dry_eff=1000)
    st = _open(full, slots)
    st.set_bypass(slots, **kw)
    assert st.bypass_state(slots) == [seed] * 2      # a pending restart reports the seed
    F = 1 + wav.shape[1] // HOP
    rw, rd, rst = B.levels(seed, c.wet_target, c.dry_target, c.step, F)
    _, _, _, wl, dl = _run_byp(st, slots, wav)
    assert np.array_equal(wl[0].cpu().numpy(), rw) and np.array_equal(dl[1].cpu().numpy(), rd) and st.bypass_state(slots) == [rst] * 2
    assert rst["wet"] == 0 and rst["dry"] == FULL
    # a reset without the front-end keeps the levels, one with it restarts from the seed; the setting survives both
    st.reset(slots, which=7)
    assert st.bypass_state(slots) == [rst] * 2
    st.reset(slots, which=15)
    st.set_reference(slots, _ref(2))
    assert st.bypass_state(slots) == [seed] * 2 and st.bypass(slots) == [_lib.bypass_keywords(c)] * 2
    _, _, _, wl, dl = _run_byp(st, slots, wav)
    assert np.array_equal(wl[1].cpu().numpy(), rw) and np.array_equal(dl[0].cpu().numpy(), rd)
    # reseed = 0 on an enabled slot keeps the levels, reseed = 1 restarts, and so does enabling a slot that was off
    st.set_bypass([1], wet=1.0, dry=0.0)
    assert st.bypass_state([1]) == [rst]
    st.set_bypass([1], reseed=True, **kw)
    assert st.bypass_state(slots) == [seed, rst]
    st.set_bypass([3], None)
    st.set_bypass([3], **kw)
    assert st.bypass_state(slots) == [seed, seed]
    st.close()


def test_errors_change_nothing(full):
    slots = [0, 2]
    st = _open(full, slots)
    with pytest.raises(_lib.ConanError) as e:      # the state query on a stream-set that never enabled the feature
        st.bypass_state([0])
    assert e.value.code == _lib.ERR_STATE
    st.set_bypass([0], wet=0.5, dry=0.25, ramp_ms=100.0)
    before = st.bypass(range(MAX_SLOTS))
    assert before[0] is not None and before[1:] == [None] * (MAX_SLOTS - 1)
    for field, value in BAD:
        c = _lib.bypass_cfg()
        setattr(c, field, value)
        with pytest.raises(_lib.ConanError) as e:
            st.set_bypass([0, 2, 3], cfg=c)
        assert e.value.code == _lib.ERR_INVALID, (field, value)
    for bad_slots in ([2, 2], [1, MAX_SLOTS], [-1]):
        with pytest.raises(_lib.ConanError) as e:
            st.set_bypass(bad_slots)
        assert e.value.code == _lib.ERR_INVALID
    assert st.bypass(range(MAX_SLOTS)) == before
    with pytest.raises(_lib.ConanError) as e:      # a slot without the feature in the state query
        st.bypass_state([0, 2])
    assert e.value.code == _lib.ERR_STATE
    with pytest.raises(_lib.ConanError) as e:      # no wav-in call yet
        st.step_wav_bypass()
    assert e.value.code == _lib.ERR_STATE
    x = _noise(1, 700, 1)
    with pytest.raises(_lib.ConanError) as e:      # 700 samples are 3 frames
        full.bypass_mix(x, x, torch.zeros(1, 2, dtype=torch.int32, device="cuda"), torch.zeros(1, 2, dtype=torch.int32, device="cuda"))
    assert e.value.code == _lib.ERR_INVALID
    st.close()
    # a stream-set without the streaming front-end
    hp, sd_np, _ = P.model()
    ctx = Context(hp, None, 0, emformer=False, conan=True, hifigan=False)
    ctx.load_state_dict("conan", sd_np)
    ctx.finalize()
    dec = ctx.streams(2, 4, 64)
    with pytest.raises(_lib.ConanError) as e:
        dec.set_bypass([0])
    assert e.value.code == _lib.ERR_STATE
    dec.close()
    ctx.close()
