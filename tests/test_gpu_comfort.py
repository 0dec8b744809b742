"""Comfort noise on the GPU (conan_streams_set_comfort, conan_step_wav_comfort, conan_comfort_track, conan_comfort_fill;
include/conan_hip.h, conan_comfort_cfg): the fill and the tracker against tests/comfort_ref.py, the streamed form against the whole
signals, and the feature against itself - neighbours keep their bits and launches, its place in the output chain, the hand-over,
restarts, errors.  Every comparison is bit for bit: the law is integer operations and single correctly rounded IEEE operations in a
fixed order."""
import ctypes as C

import numpy as np
import pytest
import torch

from conan_amd import _lib, synth
from conan_amd.engine import StreamingVoiceConversionEngine
from conan_amd.runtime import Context
from tests import activity_ref as A
from tests import comfort_ref as R
from tests import pitch_ref as P
from tests.test_comfort_cpu import BAD
from tests.test_gpu_f0 import _launches, _open, _ragged, _ref, _run
from tests.test_gpu_pitch import full  # noqa: F401  (module fixture: the small synthetic full model)

pytestmark = pytest.mark.gpu

HOP, SEG = 320, 4
L = SEG * HOP
MAX_SLOTS = 6
FULL = R.FULL
KW = dict(hold_frames=1, attack_frames=2, release_frames=3)      # the activity tests' detector: it opens and closes within a few chunks
GATE0 = 0                                                        # ... whose gate starts closed


def _u32(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.uint32)


def _seed(slot):
    return 1000 + 17 * slot


def _switched(n, N, seed, noise=1e-3):
    """A tone switched on and off at 3 Hz over line noise, one phase per row: the gate moves every few frames."""
    rng = np.random.default_rng(seed)
    t = np.arange(N) / 16000.0
    rows = []
    for i in range(n):
        on = np.floor((t + 0.05 * i) * 6.0) % 2 == 0
        rows.append(noise * rng.standard_normal(N) + 0.2 * on * np.sin(2 * np.pi * (180.0 + 40.0 * i) * t))
    return torch.from_numpy(np.stack(rows).astype(np.float32)).cuda()


def _law(w_off, gate, cmf, cfgs, seeds, start_gate=GATE0):
    """The numpy law on a run's unfilled audio w_off [n, T] and the per-frame levels [n, F]."""
    w_off, gate, cmf = w_off.cpu().numpy(), gate.cpu().numpy(), cmf.cpu().numpy()
    return np.stack([R.fill(w_off[i], gate[i], cmf[i], start_gate, HOP, seeds[i], cfgs[i].colour, cfgs[i].norm) for i in range(w_off.shape[0])])


# ------------------------------------------------------------------------------------------------------------------ 1. the fill

def _gate_rows(F, rng):
    ramp = np.rint(np.linspace(FULL, 0, F + 1)[1:]).astype(np.int32)
    mixed = np.array(([FULL, FULL, 0, 0, FULL // 3, FULL] * F)[:F], np.int32)      # full frames, closed frames, ramps between them
    return np.stack([mixed, ramp, np.full(F, FULL, np.int32)])


@pytest.mark.parametrize("pos0", [0, 2 ** 33 + 5])
@pytest.mark.parametrize("colour", [0, 1, 2])
def test_comfort_fill_against_the_law(full, colour, pos0):
    N = 5 * HOP + 37      # (a partly covered last frame; 1637 samples are more than one thread's eight and no multiple of them)
    F = -(-N // HOP)
    rng = np.random.default_rng(colour)
    gl = _gate_rows(F, rng)
    n = gl.shape[0]
    cl = rng.integers(-9000, -1500, (n, F)).astype(np.int32)
    y = (0.1 * rng.standard_normal((n, N))).astype(np.float32)
    seeds = [3, 2 ** 64 - 1, 0x123456789ABCDEF]
    cfg = _lib.comfort_cfg(colour=colour, seed=99)
    yd, gld, cld = torch.from_numpy(y).cuda(), torch.from_numpy(gl).cuda(), torch.from_numpy(cl).cuda()
    for sg in (FULL, 0, 54321):
        want = np.stack([R.fill(y[i], gl[i], cl[i], sg, HOP, seeds[i], colour, cfg.norm, pos0) for i in range(n)])
        got = full.comfort_fill(yd, gld, cld, cfg=cfg, seeds=seeds, start=(sg, -3000), pos0=pos0)
        assert np.array_equal(_u32(got), _u32(want)), (colour, pos0, sg)
        # an odd stride and rows off a 16-byte boundary by one float (the single-word path), out of place and in place
        yw, ow = torch.zeros(n, N + 6, device="cuda"), torch.zeros(n, N + 6, device="cuda")
        yv, ov = yw[:, 1:N + 1], ow[:, 1:N + 1]
        yv.copy_(yd)
        lw = torch.zeros(n, F + 3, dtype=torch.int32, device="cuda")      # (a level stride wider than the frames)
        lg, lc = lw[:, :F], lw.clone()[:, :F]
        lg.copy_(gld); lc.copy_(cld)
        assert full.comfort_fill(yv, lg, lc, cfg=cfg, seeds=seeds, start=(sg, 0), pos0=pos0, out=ov) is ov
        assert np.array_equal(_u32(ov.contiguous()), _u32(want)), (colour, pos0, sg, "views")
        assert not ow[:, :1].any() and not ow[:, N + 1:].any()      # nothing outside the rows was written
        assert full.comfort_fill(yv, lg, lc, cfg=cfg, seeds=seeds, start=(sg, 0), pos0=pos0, out=yv) is yv
        assert np.array_equal(_u32(yv.contiguous()), _u32(want))
        z = yd.clone()
        assert full.comfort_fill(z, gld, cld, cfg=cfg, seeds=seeds, start=(sg, 0), pos0=pos0, out=z) is z      # in place, aligned
        assert np.array_equal(_u32(z), _u32(want))
    got = full.comfort_fill(yd, gld, cld, cfg=cfg, seeds=seeds, start=(FULL, 0), pos0=pos0)
    assert got[2].cpu().numpy().tobytes() == y[2].tobytes()      # a row of full levels is its input, byte for byte
    assert not np.array_equal(_u32(got[1]), _u32(y[1]))
    # without seeds every row takes the cfg's
    got = full.comfort_fill(yd[:1], gld[1:2], cld[:1], cfg=cfg, start=(0, 0), pos0=pos0)
    assert np.array_equal(_u32(got[0]), _u32(R.fill(y[0], gl[1], cl[0], 0, HOP, 99, colour, cfg.norm, pos0)))


# ------------------------------------------------------------------------------------------------------------------ 2. the tracker

def _stepped_bursts():
    """Bursts over noise whose floor steps up by 20 dB half way, and a row whose floor steps down."""
    x = A.burst_signal(noise=1e-3, seed=4)
    up, down = x.copy(), x.copy()
    half = x.shape[0] // 2
    rng = np.random.default_rng(8)
    up[half:] += (1e-2 * rng.standard_normal(x.shape[0] - half)).astype(np.float32)
    down[:half] += (1e-2 * rng.standard_normal(half)).astype(np.float32)
    return torch.from_numpy(np.stack([up, down])).cuda()


@pytest.mark.parametrize("follow", [True, False])
def test_comfort_track_against_the_law(full, follow):
    wav = _stepped_bursts()
    act, _, _, pw = full.activity(wav, power=True, state=False, open_db=-30.0, close_db=-35.0)      # (the louder floor, -40 dB, is background)
    cfg = _lib.comfort_cfg(follow=follow, level_db=-47.0, rise_db=0.5)
    got, states = full.comfort_track(act, pw, cfg=cfg, return_state=True)
    a, p = act.cpu().numpy(), pw.cpu().numpy()
    seed = dict(level=cfg.seed_level, idle_frames=0)
    for i in range(2):
        want, st = R.track(seed, cfg, a[i], p[i])
        assert np.array_equal(got[i].cpu().numpy(), want), (follow, i)
        assert states[i] == st
    lv = got.cpu().numpy()
    if follow:
        idle = int((a[0] == 0).sum())
        assert states[0]["idle_frames"] == idle and 0 < idle < a.shape[1]
        mid = a.shape[1] // 2
        assert lv[0, -1] - lv[0, mid - 1] > 1000 and lv[1, mid - 1] - lv[1, mid:].min() > 1000      # the level followed the floor's step (20 dB are 1700 units)
    else:
        assert bool((lv == cfg.level).all()) and states[0]["idle_frames"] == 0
        assert np.array_equal(full.comfort_track(act, None, cfg=cfg).cpu().numpy(), lv)      # fixed mode reads no powers


# ------------------------------------------------------------------------------------------------------------------ 3. streamed = whole

def _run_cmf(st, slots, wav, on_call=None, first_call=0):
    """The blocking calls of infer_wav from call `first_call` on -> (codes, mel, wav, gate level, comfort level) over the emitted chunks."""
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
            cl = st.step_wav_comfort()
            assert not cl[:, e:].any()      # entries past the emitted frames are zero
            outs.append([c[:, :e].clone(), m.clone(), w.clone(), st.step_wav_activity()[1][:, :e].clone(), cl[:, :e].clone()])
    torch.cuda.synchronize()
    return [torch.cat([o[i] for o in outs], 1) for i in range(5)]


def _enable(st, slots, **kw):
    cfgs = []
    for s in slots:
        st.set_comfort([s], seed=_seed(s), **kw)
        cfgs.append(_lib.comfort_cfg(seed=_seed(s), **kw))
    return cfgs


def _whole(full, wav, cfg):
    """The whole-signal chain on the source: conan_activity, then conan_comfort_track on its outputs -> (gate levels, comfort levels)."""
    act, lvl, _, pw = full.activity(wav, power=True, state=False, **KW)
    return lvl, full.comfort_track(act, pw, cfg=cfg)


def test_streamed_equals_whole(full):
    slots = [1, 3, 4]
    wav = _switched(3, 12 * L - 100, 5)
    st = _open(full, slots)
    st.set_activity(slots, **KW)
    c0, m0, w0, g0, cl0 = _run_cmf(st, slots, wav)
    assert not cl0.any()      # without the feature the hook reads zeros
    st.reset(slots, which=15)
    st.set_reference(slots, _ref(3))
    cfgs = _enable(st, slots, rise_db=1.0)
    seeds = [_seed(s) for s in slots]
    c1, m1, w1, g1, cl1 = _run_cmf(st, slots, wav)
    assert torch.equal(c1, c0) and torch.equal(m1, m0) and torch.equal(g1, g0)      # the fill touches no model input
    g = g1.cpu().numpy()
    assert 0 < int((g < FULL).sum()) < g.size and int((g == 0).sum()) > 0      # the gate moved, and closed
    gate_w, cmf_w = _whole(full, wav, cfgs[0])
    assert torch.equal(g1, gate_w) and torch.equal(cl1, cmf_w)
    assert len(np.unique(cl1.cpu().numpy())) > 3      # the level moved
    want = _law(w0, g1, cl1, cfgs, seeds)
    assert np.array_equal(_u32(w1), _u32(want))
    assert not np.array_equal(_u32(w1), _u32(w0))
    got = full.comfort_fill(w0, g1, cl1, cfg=cfgs[0], seeds=seeds, start=(GATE0, cfgs[0].seed_level))
    assert np.array_equal(_u32(got), _u32(want))
    open_ = np.repeat(g[:, 1:] == FULL, HOP, 1) & np.repeat(g[:, :-1] == FULL, HOP, 1)      # frames 1 .. with both levels full
    assert open_.any() and np.array_equal(_u32(w1)[:, HOP:][open_], _u32(w0)[:, HOP:][open_])      # an open gate keeps the bits
    state = st.comfort_state(slots)
    assert [s["level"] for s in state] == [int(v) for v in cl1[:, -1]]
    # pipelined: the audio and the state of the blocking run
    st.reset(slots, which=15)
    st.set_reference(slots, _ref(3))
    (cp, mp, wp, _, _), _ = _run(st, slots, wav, pipelined=True, contour=False)
    assert torch.equal(cp, c0) and torch.equal(mp, m0) and np.array_equal(_u32(wp), _u32(w1))
    assert st.comfort_state(slots) == state
    st.close()


@pytest.mark.parametrize("pipelined", [False, True])
def test_ragged_staggered_equals_whole(full, pipelined):
    slots, starts = [5, 0, 2], [0, 1, 3]
    wavs = [_switched(1, n, 65 + i)[0] for i, n in enumerate((6 * L + 333, 5 * L, 4 * L + 1))]
    plain = _open(full, slots)
    plain.set_activity(slots, **KW)
    off = _ragged(plain, slots, wavs, starts, contour=False)
    plain.close()
    st = _open(full, slots)
    st.set_activity(slots, **KW)
    cfgs = _enable(st, [5, 2], colour=2)
    got = _ragged(st, slots, wavs, starts, pipelined=pipelined, contour=False)
    assert all(torch.equal(got[1][i], off[1][i]) for i in range(3))      # the utterance without the feature keeps its bits
    for u, cfg in ((0, cfgs[0]), (2, cfgs[1])):
        assert torch.equal(got[u][0], off[u][0]) and torch.equal(got[u][1], off[u][1])
        gate, cmf = _whole(full, wavs[u][None], cfg)
        want = R.fill(off[u][2].cpu().numpy(), gate[0].cpu().numpy(), cmf[0].cpu().numpy(), GATE0, HOP, cfg.seed, cfg.colour, cfg.norm)
        assert np.array_equal(_u32(got[u][2]), _u32(want)), u
        assert not torch.equal(got[u][2], off[u][2])
    st.close()


# ------------------------------------------------------------------------------------------------------------------ 4. neighbours

def test_neighbours_keep_their_bits_and_launches(full):
    slots = [0, 1, 2, 3]
    wav = _switched(4, 3 * L + 77, 60)
    a, b = _open(full, slots), _open(full, slots)
    for s_ in (a, b):
        s_.set_activity([0, 1, 2], **KW)
    bytes_never = b.state_bytes
    fixed = dict(follow=False, level_db=-40.0, colour=0)
    cfgs = _enable(a, [0]) + _enable(a, [2], **fixed)
    a.set_comfort([3], seed=5)      # no detector: no frames, never filled
    state = MAX_SLOTS * C.sizeof(_lib.ComfortState) + 8 * MAX_SLOTS * ((SEG + 1) * 4 + SEG * 8) + 8 * MAX_SLOTS * 112
    assert a.state_bytes == bytes_never + state      # the state, the staging sets and the row tables, from the first enabling call on
    b.set_comfort(slots, None)                        # turning off what was never on allocates nothing
    assert b.state_bytes == bytes_never and b.comfort(slots) == [None] * 4
    ((ca, ma, wa, _, _), emits), la = _launches(a, lambda: _run(a, slots, wav, contour=False))
    ((cb, mb, wb, _, _), _), lb = _launches(b, lambda: _run(b, slots, wav, contour=False))
    assert torch.equal(ca, cb) and torch.equal(ma, mb)
    for i in (1, 3):
        assert np.array_equal(_u32(wa[i]), _u32(wb[i])), i      # a row without the feature keeps its bits, and so does the one without a gate
    assert a.comfort_state([3]) == [dict(level=_lib.comfort_cfg().seed_level, idle_frames=0)]
    for i, cfg in ((0, cfgs[0]), (2, cfgs[1])):
        gate, cmf = _whole(full, wav[i:i + 1], cfg)
        want = R.fill(wb[i].cpu().numpy(), gate[0].cpu().numpy(), cmf[0].cpu().numpy(), GATE0, HOP, cfg.seed, cfg.colour, cfg.norm)
        assert np.array_equal(_u32(wa[i]), _u32(want)) and not torch.equal(wa[i], wb[i]), i
    # a stream-set that never enabled it runs the launches it ran before; the feature adds one tracker launch per emitting call and one
    # fill launch per vocoder step with a filled row
    assert "comfort_track_kernel" not in lb and "comfort_fill_kernel" not in lb
    assert la.pop("comfort_track_kernel") == len(emits) and la.pop("comfort_fill_kernel") == len(emits) and la == lb, (la, lb)
    # off again: the launches of the stream-set that never filled
    a.set_comfort(slots, None)
    assert a.comfort(slots) == [None] * 4
    a.reset(slots, which=15)
    a.set_reference(slots, _ref(4))
    ((_, m2, w2, _, _), _), l2 = _launches(a, lambda: _run(a, slots, wav, contour=False))
    assert l2 == lb and torch.equal(m2, mb) and torch.equal(w2, wb)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------ 5. the chain

def test_order_in_the_output_chain(full):
    n = 2
    wav = _switched(n, 5 * L + 700, 31)
    eng = StreamingVoiceConversionEngine(full, n, max_ref_frames=64)
    kw = dict(activity=dict(KW), bypass=dict(wet=1.0, dry=0.5, fill_gate=True), out_level=True)
    cmf = dict(colour=1, offset_db=0.0)
    cfgs = [_lib.comfort_cfg(seed=_lib.comfort_seed(s), **cmf) for s in range(n)]
    for pipelined in (False, True):
        w0, m0, _ = eng.infer_wav(wav, _ref(n), pipelined=pipelined, **kw)      # the model-rate audio behind leveller, gate and mix
        w1, m1, _ = eng.infer_wav(wav, _ref(n), pipelined=pipelined, comfort=cmf, out_rate=8000, out_format="ulaw", **kw)
        torch.cuda.synchronize()
        assert torch.equal(m1, m0)
        gate, lv = _whole(full, wav, cfgs[0])
        filled = torch.from_numpy(_law(w0, gate, lv, cfgs, [c.seed for c in cfgs])).cuda()
        assert not torch.equal(filled, w0)
        exp = full.convert_samples(full.resample(filled, 16000, 8000), "f32", "ulaw")
        assert w1.shape == exp.shape and w1.dtype == exp.dtype and torch.equal(w1, exp), pipelined
    eng.st.close()


# ------------------------------------------------------------------------------------------------------------------ 6. hand-over, restarts

def test_hand_over_continues_bit_for_bit(full):
    slots, dst = [1, 4], [3, 0]
    wav = _switched(2, 7 * L + 123, 21)
    kw = dict(rise_db=1.0, fall_db=1.0, start_db=-40.0)      # a slow fall from a high start: the cut falls inside it
    a = _open(full, slots)
    a.set_activity(slots, **KW)
    _enable(a, slots, **kw)
    cw, mw, ww, gw, clw = _run_cmf(a, slots, wav)
    a.reset(slots, which=15)
    a.set_reference(slots, _ref(2))
    cut = 4      # calls before the export: chunks 0 .. 2 are out
    b = full.streams(MAX_SLOTS, 4, 64)
    lid, nbytes = b.layout_id, b.snapshot_bytes
    assert (a.layout_id, a.snapshot_bytes) == (lid, nbytes)      # the feature changes neither
    for k in range(cut):
        a.step_wav(slots, wav[:, k * L:(k + 1) * L])
    states, acts = a.comfort_state(slots), a.activity_state(slots)
    done = (cut - 1) * SEG
    assert [s["level"] for s in states] == [int(v) for v in clw[:, done - 1]]
    snap = a.export_slots(slots)
    b.import_slots(dst, snap)
    assert b.comfort(dst) == [None, None]      # a snapshot carries neither the setting nor the state
    for d, src, s, sa in zip(dst, slots, states, acts):
        b.set_activity([d], seed=sa, reseed=True, **KW)
        b.set_comfort([d], seed=_seed(src), reseed=True, **dict(kw, start=s["level"]))
    assert (b.layout_id, b.snapshot_bytes) == (lid, nbytes)
    c, m, w, g, cl = _run_cmf(b, dst, wav, first_call=cut)
    assert torch.equal(c, cw[:, done:]) and torch.equal(m, mw[:, done:]) and np.array_equal(_u32(w), _u32(ww[:, done * HOP:]))
    assert torch.equal(g, gw[:, done:]) and torch.equal(cl, clw[:, done:])
    a.close(); b.close()


def test_restarts_and_modes(full):
    slots = [1, 3]
    wav = _switched(2, 4 * L + 10, 95)
    st = _open(full, slots)
    st.set_activity([1], **KW)
    st.set_activity([3], gate=False, **KW)      # mode 1: the slot tracks and is never filled
    cfgs = _enable(st, slots, start_db=-45.0)
    seed = dict(level=cfgs[0].seed_level, idle_frames=0)
    assert st.comfort_state(slots) == [seed] * 2      # a pending restart reports the seed
    assert st.comfort([1]) == [_lib.comfort_keywords(cfgs[0])]
    c1, m1, w1, g1, cl1 = _run_cmf(st, slots, wav)
    _, cmf_w = _whole(full, wav, cfgs[0])
    assert torch.equal(cl1, cmf_w) and cl1[1].any()      # both track
    end = st.comfort_state(slots)
    assert [s["level"] for s in end] == [int(v) for v in cl1[:, -1]] and end[0]["idle_frames"] > 0 and end != [seed] * 2
    # a reset without the front-end keeps the level, one with it restarts level and sequence; the setting survives both
    st.reset(slots, which=7)
    assert st.comfort_state(slots) == end
    st.reset(slots, which=15)
    st.set_reference(slots, _ref(2))
    assert st.comfort_state(slots) == [seed] * 2 and st.comfort([3]) == [_lib.comfort_keywords(cfgs[1])]
    c2, m2, w2, g2, cl2 = _run_cmf(st, slots, wav)
    assert torch.equal(cl2, cl1) and np.array_equal(_u32(w2), _u32(w1))
    # the unfilled run: the gated slot differs from it, the detecting slot is never filled
    st.set_comfort(slots, None)
    st.reset(slots, which=15)
    st.set_reference(slots, _ref(2))
    _, _, w0, _, cl0 = _run_cmf(st, slots, wav)
    assert not cl0.any() and np.array_equal(_u32(w1[1]), _u32(w0[1])) and not np.array_equal(_u32(w1[0]), _u32(w0[0]))
    # enabling a slot that was off restarts it; reseed = 0 on an enabled slot keeps the level, reseed = 1 restarts
    _enable(st, slots, start_db=-45.0)
    assert st.comfort_state(slots) == [seed] * 2
    st.reset(slots, which=15)
    st.set_reference(slots, _ref(2))
    _run_cmf(st, slots, wav[:, :3 * L + 5])
    mid = st.comfort_state(slots)
    assert mid != [seed] * 2
    st.set_comfort([1], seed=_seed(1), start_db=-80.0, colour=2)
    assert st.comfort_state(slots) == mid and st.comfort([1])[0]["colour"] == 2
    st.set_comfort([1], seed=_seed(1), start_db=-80.0, reseed=True)
    assert st.comfort_state(slots) == [dict(level=_lib.comfort_level(-80.0), idle_frames=0), mid[1]]
    st.close()


def test_mel_in_steps_do_not_fill(full):
    slots = [0, 1]
    a, b = _open(full, slots), _open(full, slots)
    a.set_activity(slots, **KW)
    _enable(a, slots)
    chunk = torch.from_numpy(synth.mel(SEG + full.cfg.emf_right_context, 77, 2)).cuda()
    (ca, ma, wa), la = _launches(a, lambda: a.step(slots, chunk))
    (cb, mb, wb), lb = _launches(b, lambda: b.step(slots, chunk))
    torch.cuda.synchronize()
    assert la == lb and "comfort_fill_kernel" not in la and "comfort_track_kernel" not in la
    assert torch.equal(ca, cb) and torch.equal(ma, mb) and np.array_equal(_u32(wa), _u32(wb))
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------ 7. errors

def test_errors_change_nothing(full):
    slots = [0, 2]
    st = _open(full, slots)
    with pytest.raises(_lib.ConanError) as e:      # the state query on a stream-set that never enabled the feature
        st.comfort_state([0])
    assert e.value.code == _lib.ERR_STATE
    st.set_comfort([0], follow=False, level_db=-50.0, seed=11)
    before, bytes_before = st.comfort(range(MAX_SLOTS)), st.state_bytes
    assert before[0] is not None and before[1:] == [None] * (MAX_SLOTS - 1)
    for field, value in BAD:
        c = _lib.comfort_cfg()
        setattr(c, field, value)
        with pytest.raises(_lib.ConanError) as e:
            st.set_comfort([0, 2, 3], cfg=c)
        assert e.value.code == _lib.ERR_INVALID, (field, value)
    for bad_slots in ([2, 2], [1, MAX_SLOTS], [-1]):
        with pytest.raises(_lib.ConanError) as e:
            st.set_comfort(bad_slots)
        assert e.value.code == _lib.ERR_INVALID
    assert st.lib.conan_streams_set_comfort(st.h, None, 1, C.byref(_lib.comfort_cfg()), None) == _lib.ERR_INVALID      # a null argument
    assert st.lib.conan_streams_comfort_state(st.h, (C.c_int32 * 1)(0), 1, None, None) == _lib.ERR_INVALID
    assert st.comfort(range(MAX_SLOTS)) == before and st.state_bytes == bytes_before
    assert st.comfort_state([0]) == [dict(level=_lib.comfort_level(-70.0), idle_frames=0)]
    with pytest.raises(_lib.ConanError) as e:      # a slot without the feature in the state query
        st.comfort_state([0, 2])
    assert e.value.code == _lib.ERR_STATE
    with pytest.raises(_lib.ConanError) as e:      # no wav-in call yet
        st.step_wav_comfort()
    assert e.value.code == _lib.ERR_STATE
    x = torch.zeros(1, 700, device="cuda")
    lv = torch.zeros(1, 2, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.ConanError) as e:      # 700 samples are 3 frames
        full.comfort_fill(x, lv, lv)
    assert e.value.code == _lib.ERR_INVALID
    st.close()
    # a stream-set without the streaming front-end
    hp, sd_np, _ = P.model()
    ctx = Context(hp, None, 0, emformer=False, conan=True, hifigan=False)
    ctx.load_state_dict("conan", sd_np)
    ctx.finalize()
    dec = ctx.streams(2, 4, 64)
    with pytest.raises(_lib.ConanError) as e:
        dec.set_comfort([0])
    assert e.value.code == _lib.ERR_STATE
    dec.close()
    ctx.close()
