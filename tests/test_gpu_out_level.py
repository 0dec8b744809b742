"""Output levelling on the GPU (conan_streams_set_output_level and its queries; include/conan_hip.h): a levelled slot's model-rate
audio equals Context.level (conan_level, the whole-signal yardstick) of the same run's unlevelled audio, bit for bit - wav-in and
mel-in, blocking and pipelined, both arithmetics, ragged groups, across a hand-over; the leveller's place in the output chain; and
the feature against itself - neighbours keep their bits and launches, restarts, errors.  The feature needs no tolerance: every
comparison is of uint32 views.

The fixture's unlevelled vocoder audio (the small synthetic full model on 0.1-amplitude noise) is printed by the first test that
uses it and recorded there: see _base."""
import numpy as np
import pytest
import torch

from conan_amd import _lib, synth
from conan_amd.engine import StreamingVoiceConversionEngine
from tests import bypass_ref as B
from tests.test_gpu_bypass import KW, _bursts, _noise, _padded, _u32
from tests.test_gpu_f0 import _launches, _open, _ragged, _ref, _run
from tests.test_gpu_pitch import full  # noqa: F401  (module fixture: the small synthetic full model)

pytestmark = pytest.mark.gpu

HOP, SEG, FS = 320, 4, 16000
U = SEG * HOP
MAX_SLOTS = 6
N_SRC = 13 * U + 700          # 55 frames: 13 whole vocoder steps and one of 3 frames; 7 gating blocks complete before u_13
CHUNKS = 14
STATE_BYTES = 672 + 2 * (_lib.LEVEL_MAX_BLOCKS + 16) * 8 + 32
ROW_BYTES = 160               # one row of the step's table
SLOTS = [1, 4]


def _blocks_ended(p):
    j = 0
    while int(0.4 * (j * 0.25 + 1.0) * FS) <= p:
        j += 1
    return j


def _yardstick(ctx, w0, **cfg):
    """Context.level of the unlevelled audio with its trace; the condition that makes the comparison mean something is enforced here:
    at least three instants with a finite reading and at least three distinct gains per row."""
    want, trace = ctx.level(w0, return_trace=True, **cfg)
    t = trace.cpu().numpy()
    for i in range(t.shape[0]):
        finite = int(np.isfinite(t[i, :, 0]).sum())
        gains = len(set(t[i, :, 1].tolist()))
        assert finite >= 3 and gains >= 3, (i, finite, gains, t[i])
    assert not np.array_equal(_u32(want), _u32(w0))
    return want, t


_BASE = {}


def _base(ctx, arith="auto"):
    """The unlevelled run, once per arithmetic: the source, the run's (codes, mel, wav) and the target the cases level to - the
    integrated loudness of row 0's unlevelled audio plus 6 dB, under a boost cap of 20 dB.  Measured on MI355X: the fixture's vocoder
    audio reads -25.21 LUFS (row 0) and -25.37 LUFS (row 1) in every arithmetic, far above the absolute gate of -70, so conv_post's weights are left as they are."""
    if arith not in _BASE:
        src = _noise(2, N_SRC, 41)
        st = _open(ctx, SLOTS, arith=arith)
        (c, m, w, _, _), emits = _run(st, SLOTS, src, contour=False)
        st.close()
        assert len(emits) == CHUNKS and w.shape[1] == 55 * HOP
        loud = ctx.loudness(w, FS).cpu().numpy()
        print("unlevelled vocoder audio, LUFS per row (arith %s):" % arith, loud)
        assert np.isfinite(loud).all()      # above the absolute gate
        _BASE[arith] = dict(src=src, c=c, m=m, w=w, target=float(loud[0]) + 6.0)
    return _BASE[arith]


def _cfg(base, **kw):
    return dict(dict(target=base["target"], max_boost_db=20.0), **kw)


VARIANTS = {"default": {}, "window3": dict(window_blocks=3), "clip": dict(clip=True), "nopeak": dict(peak_limit=False)}


# ------------------------------------------------------------------------------------------------ 1. equals the whole-signal form

@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_wav_in_equals_the_whole_signal_form(full, variant, pipelined):
    base = _base(full)
    cfg = _cfg(base, **VARIANTS[variant])
    want, _ = _yardstick(full, base["w"], **cfg)
    st = _open(full, SLOTS)
    st.set_output_level(SLOTS, **cfg)
    assert st.output_levels[1] == _lib.level_keywords(_lib.level_cfg(**cfg))
    (c, m, w, _, _), emits = _run(st, SLOTS, base["src"], pipelined=pipelined, contour=False)
    assert len(emits) == CHUNKS and torch.equal(c, base["c"]) and torch.equal(m, base["m"])      # the leveller touches no model input
    assert np.array_equal(_u32(w), _u32(want)), (variant, pipelined, int((_u32(w) != _u32(want)).sum()))
    st.close()


@pytest.mark.parametrize("arith", ["f32", "limb"])
def test_both_arithmetics_equal_the_whole_signal_form(full, arith):
    base = _base(full, arith)
    cfg = _cfg(base)
    want, _ = _yardstick(full, base["w"], **cfg)
    st = _open(full, SLOTS, arith=arith)
    st.set_output_level(SLOTS, **cfg)
    (c, m, w, _, _), _ = _run(st, SLOTS, base["src"], contour=False)
    assert torch.equal(m, base["m"]) and np.array_equal(_u32(w), _u32(want)), arith
    st.close()


@pytest.mark.parametrize("pipelined", [False, True])
def test_mel_in_equals_the_whole_signal_form(full, pipelined):
    src = torch.from_numpy(synth.mel(55, 9, 2)).cuda()      # 13 chunks of 4 frames and one of 3
    eng = StreamingVoiceConversionEngine(full, 2, max_ref_frames=64)
    w0, m0, _ = eng.infer(src, _ref(2), pipelined=pipelined)
    torch.cuda.synchronize()
    w0 = w0.clone()
    loud = full.loudness(w0, FS).cpu().numpy()
    assert np.isfinite(loud).all(), loud
    cfg = dict(target=float(loud[0]) + 6.0, max_boost_db=20.0)
    want, _ = _yardstick(full, w0, **cfg)
    w1, m1, _ = eng.infer(src, _ref(2), pipelined=pipelined, out_level=cfg)
    torch.cuda.synchronize()
    assert torch.equal(m1, m0) and np.array_equal(_u32(w1), _u32(want))
    w2, _, _ = eng.infer(src, _ref(2), pipelined=pipelined)      # out_level=None turns it off again
    torch.cuda.synchronize()
    assert np.array_equal(_u32(w2), _u32(w0)) and eng.st.output_levels == {}
    eng.st.close()


def test_one_whole_interval(full):
    """1279 source samples: one vocoder step of exactly U samples - the meter reaches its instant, nothing follows."""
    src = _noise(2, 1279, 43)
    st = _open(full, SLOTS)
    (_, _, w0, _, _), emits = _run(st, SLOTS, src, contour=False)
    assert emits == [4] and w0.shape[1] == U
    cfg = dict(target=-20.0, initial_gain_db=-3.0, clip=True)
    want = full.level(w0, **cfg)
    st.reset(SLOTS, which=15)
    st.set_reference(SLOTS, _ref(2))
    st.set_output_level(SLOTS, **cfg)
    assert np.array_equal(st.output_level(SLOTS).cpu().numpy(), np.array([[-np.inf, 10.0 ** (-3.0 / 20.0), 0.0, 0.0]] * 2))
    (_, _, w1, _, _), _ = _run(st, SLOTS, src, contour=False)
    assert np.array_equal(_u32(w1), _u32(want)) and not np.array_equal(_u32(w1), _u32(w0))
    st.close()


def test_stats_against_the_trace(full):
    base = _base(full)
    cfg = _cfg(base)
    src, w0 = base["src"], base["w"]
    st = _open(full, SLOTS)
    st.set_output_level(SLOTS, **cfg)
    calls = [(p, p + U, False) for p in range(0, (N_SRC - 1) // U * U, U)] + [((N_SRC - 1) // U * U, N_SRC, True)]
    chunks, seen = 0, []
    while True:
        if calls:
            a, b, fin = calls.pop(0)
            e, _, _, _ = st.step_wav(SLOTS, src[:, a:b], final=fin)
        else:
            e, _, _, _ = st.step_wav(SLOTS, src[:, :0], final=True)
            if e == 0:
                break
        if not e:
            continue
        chunks += 1
        if chunks in (1, 6, 14):
            done = min(chunks * U, w0.shape[1])      # the audio so far
            _, trace = full.level(w0[:, :done], return_trace=True, **cfg)
            k = (done - 1) // U
            got = st.output_level(SLOTS).cpu().numpy()
            t = trace.cpu().numpy()
            assert t.shape[1] == k + 1
            for i in range(2):
                peak = float(w0[i, :k * U].abs().max()) if k else 0.0
                assert np.array_equal(got[i, :2].view(np.uint64), t[i, k].view(np.uint64)), (chunks, i, got[i], t[i, k])
                assert got[i, 2] == peak and got[i, 3] == _blocks_ended(k * U), (chunks, i, got[i])
            seen.append(chunks)
    assert seen == [1, 6, 14]
    st.close()


# ------------------------------------------------------------------------------------------------ 2. position in the chain

def test_position_in_the_chain(full):
    """Output level, activity mode 2, a 0.5 / 0.5 bypass with fill_gate, a 48 kHz output rate and s16 out on one slot: the output
    plus the flush equals level -> activity_gate -> bypass_mix -> resample -> convert on the unlevelled run's audio."""
    half = B.FULL // 2
    src = _bursts(1, 9)
    src = torch.cat([src, src[:, :4 * U + 690]], 1)
    assert src.shape[1] == N_SRC
    eng = StreamingVoiceConversionEngine(full, 1, max_ref_frames=64)
    w0, m0, _ = eng.infer_wav(src, _ref(1), pipelined=False)
    torch.cuda.synchronize()
    w0 = w0.clone()
    cfg = dict(target=float(full.loudness(w0, FS).cpu().numpy()[0]) + 6.0, max_boost_db=20.0)
    byp = dict(wet=0.5, dry=0.5, fill_gate=True)
    eng.start_wav(_ref(1), activity=dict(KW), bypass=byp, out_rate=48000, out_format="s16", out_level=cfg)
    outs, gl, wl, dl = [], [], [], []
    last = (N_SRC - 1) // U * U
    pos, final = 0, False
    while True:
        if pos < last:
            w, m, _ = eng.feed(src[:, pos:pos + U])
            pos += U
        else:
            w, m, _ = eng.feed(src[:, pos:] if not final else src[:, :0], final=True)
            pos, done, final = N_SRC, final and m.shape[1] == 0, True
            if done:
                break
        if m.shape[1]:
            e = m.shape[1]
            outs.append(w.clone())
            gl.append(eng.chunk_activity()[1][:, :e].clone())
            a, b = eng.chunk_bypass()
            wl.append(a[:, :e].clone()); dl.append(b[:, :e].clone())
    outs.append(torch.stack(eng.finish()))
    torch.cuda.synchronize()
    got = torch.cat(outs, 1)
    gl, wl, dl = torch.cat(gl, 1), torch.cat(wl, 1), torch.cat(dl, 1)
    assert 0 < int((gl < B.FULL).sum()) < gl.numel()      # the gate moved
    gate0 = _lib.activity_cfg(**KW).seed.level
    y = full.level(w0, **cfg)
    assert not np.array_equal(_u32(y), _u32(w0))
    y = full.activity_gate(y, gl, start_level=gate0)
    y = full.bypass_mix(y, _padded(src), wl, dl, start=(half, B.fill(half, gate0, True)))
    y = full.resample(y, FS, 48000)
    y = full.convert_samples(y, "f32", "s16")
    assert got.dtype == y.dtype and got.shape == y.shape and torch.equal(got, y), int((got != y).sum())
    eng.st.close()


# ------------------------------------------------------------------------------------------------ 3. neighbours

def test_neighbours_keep_their_bits_and_launches(full):
    slots = [0, 1, 2, 3]
    wav = _noise(4, 3 * U + 77, 60)
    a, b = _open(full, slots), _open(full, slots)
    bytes_never = b.state_bytes
    lid, snap = b.layout_id, b.snapshot_bytes
    cfg = dict(target=-14.0, initial_gain_db=6.0)
    a.set_output_level([0, 2], **cfg)
    grown = MAX_SLOTS * (STATE_BYTES + 8 * (4 * U + ROW_BYTES))
    assert a.lib.conan_streams_output_level_state_bytes(a.h) == STATE_BYTES
    assert a.state_bytes == bytes_never + grown      # the state, the staging sets and the row tables, from the first enabling call on
    a.set_output_level([3], **cfg)
    a.set_output_level([3], None)
    assert a.state_bytes == bytes_never + grown and (a.layout_id, a.snapshot_bytes) == (lid, snap)
    b.set_output_level(slots, None)                  # turning off what was never on allocates nothing
    assert b.state_bytes == bytes_never and b.output_levels == {}
    ((ca, ma, wa, _, _), emits), la = _launches(a, lambda: _run(a, slots, wav, contour=False))
    ((cb, mb, wb, _, _), _), lb = _launches(b, lambda: _run(b, slots, wav, contour=False))
    assert torch.equal(ca, cb) and torch.equal(ma, mb)
    for i in (1, 3):
        assert np.array_equal(_u32(wa[i]), _u32(wb[i])), i      # a row without the feature keeps its bits
    want = full.level(wb[[0, 2]], **cfg)
    assert np.array_equal(_u32(wa[[0, 2]]), _u32(want)) and not np.array_equal(_u32(want), _u32(wb[[0, 2]]))
    # the launch dictionaries differ exactly by the two kernels, once each per vocoder step
    assert "level_out_apply_kernel" not in lb and "level_out_meter_kernel" not in lb
    assert la.pop("level_out_apply_kernel") == len(emits) and la.pop("level_out_meter_kernel") == len(emits) and la == lb, (la, lb)
    # off again (at the start of the vocoder streams): the launches and bits of the stream-set that never levelled
    a.reset(slots, which=15)
    a.set_reference(slots, _ref(4))
    a.set_output_level(slots, None)
    assert a.output_levels == {}
    ((_, m2, w2, _, _), _), l2 = _launches(a, lambda: _run(a, slots, wav, contour=False))
    assert l2 == lb and torch.equal(m2, mb) and np.array_equal(_u32(w2), _u32(wb))
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 4. ragged groups

def test_ragged_groups_level_only_where_a_levelled_row_takes_part(full):
    slots, starts = [5, 0, 2], [0, 1, 3]
    wavs = [_noise(1, n, 65 + i)[0] for i, n in enumerate((4 * U + 333, 3 * U, 2 * U + 1))]
    plain = _open(full, slots)
    want, lp = _launches(plain, lambda: _ragged(plain, slots, wavs, starts, contour=False))
    plain.close()
    cfg = dict(target=-14.0, initial_gain_db=6.0)
    st = _open(full, slots)
    st.set_output_level([5], **cfg)
    got, lg = _launches(st, lambda: _ragged(st, slots, wavs, starts, contour=False))
    for u in (1, 2):
        assert all(torch.equal(got[u][i], want[u][i]) for i in range(3)), u      # the other utterances keep their bits
    assert torch.equal(got[0][0], want[0][0]) and torch.equal(got[0][1], want[0][1])
    assert np.array_equal(_u32(got[0][2]), _u32(full.level(want[0][2][None], **cfg)[0]))
    chunks0 = -(-(1 + wavs[0].shape[0] // HOP) // SEG)      # slot 5's emit groups: one pair of launches each
    assert lg.pop("level_out_apply_kernel") == chunks0 and lg.pop("level_out_meter_kernel") == chunks0 and lg == lp, (lg, lp)
    st.close()


def test_staggered_utterances_equal_each_utterance_alone(full):
    fixed = _lib.STREAMS_FIXED_PLAN      # (a fixed plan: a row's arithmetic does not depend on the rows it shares a launch with)
    wavs = [_noise(1, n, 30 + i)[0] for i, n in enumerate((4 * U + 333, 3 * U, 2 * U + 1))]
    lv = [dict(target=-14.0, initial_gain_db=6.0), None, True]
    refs = _ref(3)
    eng = StreamingVoiceConversionEngine(full, 3, max_ref_frames=64, flags=fixed)
    blk = eng.infer_wav_staggered(wavs, [0, 1, 3], refs, pipelined=False, out_level=lv)
    pip = eng.infer_wav_staggered(wavs, [0, 1, 3], refs, pipelined=True, out_level=lv)
    torch.cuda.synchronize()
    eng.st.close()
    solo = StreamingVoiceConversionEngine(full, 3, max_ref_frames=64, flags=fixed)
    solo.slots = [0]
    for u in range(3):
        w, m, c = solo.infer_wav(wavs[u][None], refs[u][None], pipelined=False, out_level=lv[u])
        torch.cuda.synchronize()
        for got in (blk[u], pip[u]):
            assert torch.equal(got[1], m[0]) and torch.equal(got[2], c[0]) and np.array_equal(_u32(got[0]), _u32(w[0])), u
    solo.st.close()


# ------------------------------------------------------------------------------------------------ 5. the hand-over

def test_hand_over_continues_bit_for_bit(full):
    base = _base(full)
    cfg = _cfg(base)
    src = base["src"]
    want, t = _yardstick(full, base["w"], **cfg)
    # the cut behind chunk 6 falls where the gain is on the move: the state carries G_5 = G_6 (no block ends between u_5 and u_6), far
    # from the initial gain, and the first ramp that starts from the seeded state (interval 7) moves on to another G_7
    assert t[0, 6, 1] != 1.0 and t[0, 6, 1] != t[0, 7, 1] and t[1, 6, 1] != t[1, 7, 1]
    dst = [3, 0]
    a = _open(full, SLOTS)
    b = full.streams(MAX_SLOTS, 4, 64)
    lid, nbytes = b.layout_id, b.snapshot_bytes
    a.set_output_level(SLOTS, **cfg)
    assert (a.layout_id, a.snapshot_bytes) == (lid, nbytes)      # the feature changes neither
    head = []
    for k in range(7):      # call k emits chunk k - 1: chunks 1 .. 6 are out
        e, _, _, w = a.step_wav(SLOTS, src[:, k * U:(k + 1) * U])
        if e:
            head.append(w.clone())
    assert len(head) == 6
    state = a.output_level_state(SLOTS)
    assert state.shape == (2, STATE_BYTES) and state.dtype == torch.uint8
    stats = a.output_level(SLOTS)
    snap = a.export_slots(SLOTS)
    b.import_slots(dst, snap)
    assert b.output_levels == {}      # a snapshot carries neither the setting nor the state
    with pytest.raises(_lib.ConanError) as e:      # mid-utterance without a seed
        b.set_output_level(dst, **cfg)
    assert e.value.code == _lib.ERR_STATE and b.output_levels == {}
    b.set_output_level(dst, seed=state, **cfg)
    assert torch.equal(b.output_level(dst), stats) and (b.layout_id, b.snapshot_bytes) == (lid, nbytes)
    calls = [(p, p + U, False) for p in range(0, (N_SRC - 1) // U * U, U)] + [((N_SRC - 1) // U * U, N_SRC, True)]
    tail = []
    for p, q, fin in calls[7:]:
        e, _, _, w = b.step_wav(dst, src[:, p:q], final=fin)
        tail.append(w.clone())
    while True:
        e, _, _, w = b.step_wav(dst, src[:, :0], final=True)
        if e == 0:
            break
        tail.append(w.clone())
    torch.cuda.synchronize()
    got = torch.cat(head + tail, 1)
    assert len(tail) == 8 and np.array_equal(_u32(got), _u32(want))
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 6. restarts and errors

def test_restarts_and_errors(full):
    src = _noise(2, 3 * U + 10, 95)
    cfg = dict(target=-14.0, initial_gain_db=6.0)
    st = _open(full, SLOTS)
    with pytest.raises(_lib.ConanError) as e:      # the queries on a stream-set that never enabled the feature
        st.output_level([1])
    assert e.value.code == _lib.ERR_STATE
    st.set_output_level(SLOTS, **cfg)
    (_, _, w1, _, _), _ = _run(st, SLOTS, src, contour=False)
    # a reset with the vocoder restarts the meter and the gain; the setting survives
    st.reset(SLOTS, which=15)
    st.set_reference(SLOTS, _ref(2))
    assert st.output_levels[4] == _lib.level_keywords(_lib.level_cfg(**cfg))
    assert float(st.output_level(SLOTS)[0, 0]) == -np.inf
    (_, _, w2, _, _), _ = _run(st, SLOTS, src, contour=False)
    assert np.array_equal(_u32(w2), _u32(w1))
    # a failed setter call changes nothing: mid-utterance without a seed, bad slots, a bad cfg
    before = dict(st.output_levels)
    for slots, kw, code in ((SLOTS, cfg, _lib.ERR_STATE), ([1, 1], cfg, _lib.ERR_INVALID), ([1, MAX_SLOTS], cfg, _lib.ERR_INVALID),
                            ([1], dict(window_blocks=0), _lib.ERR_INVALID), ([1], dict(max_boost_db=-1.0), _lib.ERR_INVALID)):
        with pytest.raises(_lib.ConanError) as e:
            st.set_output_level(slots, **kw)
        assert e.value.code == code, (slots, kw)
    with pytest.raises(_lib.ConanError) as e:      # removal is bound to the start of the vocoder stream too
        st.set_output_level(SLOTS, None)
    assert e.value.code == _lib.ERR_STATE and st.output_levels == before
    with pytest.raises(_lib.ConanError) as e:      # a slot without the feature in the queries
        st.output_level([1, 2])
    assert e.value.code == _lib.ERR_STATE
    with pytest.raises(_lib.ConanError) as e:
        st.output_level_state([2])
    assert e.value.code == _lib.ERR_STATE
    st.close()


def test_rows_the_split_form_does_not_cover(full):
    """A conan_hifigan_step with frames * hop > U on a levelled slot is refused before anything changes: the next valid steps' bits
    prove it; an unlevelled slot takes the same step."""
    mel = torch.from_numpy(synth.mel(8, 5, 2)).cuda()
    cfg = dict(target=-14.0, initial_gain_db=6.0)
    a = full.streams(MAX_SLOTS, 8, 64)
    a.reset(SLOTS, which=4)
    w0 = torch.cat([a.hifigan_step(SLOTS, mel[:, :4].contiguous()).clone(), a.hifigan_step(SLOTS, mel[:, 4:].contiguous()).clone()], 1)
    a.reset(SLOTS, which=4)
    a.set_output_level([1], **cfg)
    with pytest.raises(_lib.ConanError) as e:
        a.hifigan_step(SLOTS, mel)      # 8 frames: 2 U
    assert e.value.code == _lib.ERR_UNSUPPORTED
    w5 = a.hifigan_step([4], mel[1:]).clone()      # the unlevelled slot may; put it back for the comparison below
    a.reset([4], which=4)
    first = a.hifigan_step(SLOTS, mel[:, :4].contiguous()).clone()
    with pytest.raises(_lib.ConanError) as e:
        a.hifigan_step(SLOTS, mel)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    w1 = torch.cat([first, a.hifigan_step(SLOTS, mel[:, 4:].contiguous()).clone()], 1)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(w1[0]), _u32(full.level(w0[:1], **cfg)[0])) and np.array_equal(_u32(w1[1]), _u32(w0[1]))
    assert w5.shape[1] == 8 * HOP
    # a step at a position that is not a multiple of U
    a.reset([1], which=4)
    a.hifigan_step([1], mel[:1, :3].contiguous())
    with pytest.raises(_lib.ConanError) as e:
        a.hifigan_step([1], mel[:1, 3:6].contiguous())
    assert e.value.code == _lib.ERR_UNSUPPORTED
    a.close()


# ------------------------------------------------------------------------------------------------ 7. the engine

def test_engine_levels_a_quiet_voice(full):
    src = _noise(2, 5 * U + 700, 77)
    eng = StreamingVoiceConversionEngine(full, 2, max_ref_frames=64)
    w0, m0, _ = eng.infer_wav(src, _ref(2))
    torch.cuda.synchronize()
    w0 = w0.clone()
    eng.open_slots(eng.slots, _ref(2), out_level=[dict(target=-40.0), None])      # a target far under the fixture's loudness
    assert list(eng.st.output_levels) == [eng.slots[0]]
    w1, m1, _ = eng.infer_wav(src, _ref(2), out_level=True)
    torch.cuda.synchronize()
    assert sorted(eng.st.output_levels) == sorted(eng.slots)
    assert torch.equal(m1, m0) and np.array_equal(_u32(w1), _u32(full.level(w0))) and not np.array_equal(_u32(w1), _u32(w0))
    eng.st.reset(eng.slots, which=15)
    eng.set_output_level([eng.slots[1]], None)
    eng.st.set_reference(eng.slots, _ref(2))
    (_, _, w2, _, _), _ = _run(eng.st, eng.slots, src, contour=False)
    assert np.array_equal(_u32(w2[0]), _u32(w1[0])) and np.array_equal(_u32(w2[1]), _u32(w0[1]))      # the unlevelled neighbour's bits
    eng.st.close()
