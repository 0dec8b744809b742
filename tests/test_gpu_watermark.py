"""The output watermark on the GPU (conan_watermark_embed / _detect / _decide, conan_streams_set_watermark and its queries;
include/conan_hip.h): the embedder's whole-signal form against tests/watermark_ref.py bit for bit; a marked slot's audio - mel-in and
wav-in, blocking and pipelined - equal to the whole-signal form of the same run's unmarked audio, its neighbours' bits and launches
untouched; the mark's place in the output chain; the setter between pipelined steps, the reset rule, the hand-over, the refused
calls; the detector's integers against the reference bit for bit; and the robustness matrix of tests/watermark_cases.py through the
library's own resampler and codecs.  The feature needs no tolerance but decide's z (1e-12 relative: one f64 sum order, two libms)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conan_amd import _lib, configs, synth
from conan_amd.engine import StreamingVoiceConversionEngine
from conan_amd.runtime import Context, _ptr, _stream
from tests import sample_format_ref as sf
from tests import watermark_cases as cases
from tests import watermark_ref as wm
from tests.test_gpu_bypass import KW, _bursts, _noise, _u32
from tests.test_gpu_f0 import _launches, _open, _ref, _run
from tests.test_gpu_pitch import full  # noqa: F401  (module fixture: the small synthetic full model)

pytestmark = pytest.mark.gpu

HOP, SEG = 320, 4
U = SEG * HOP
MAX_SLOTS = 6
SLOTS = [1, 4]
KEY, ID = cases.KEY, cases.ID
MARK = dict(key=KEY, id=ID)
OTHER = dict(key=KEY ^ 0x55AA, id=0x1234, gain=0.05, floor=0.0005)
ROW_BYTES = 56      # one row of the step's table


def _np(t):
    return t.detach().cpu().numpy()


def _law(w, state=None, lens=None, **cfg):
    """The reference's embedder on rows w [n, N] (numpy or cuda) -> (marked [n, N] float32, the states behind the rows)."""
    w = _np(w) if isinstance(w, torch.Tensor) else np.asarray(w)
    kw = dict(MARK, **cfg)
    out, states = w.copy(), []
    for i in range(w.shape[0]):
        m = w.shape[1] if lens is None else lens[i]
        out[i, :m], s = wm.embed(w[i, :m], kw["key"], kw["id"], kw.get("gain", wm.GAIN), kw.get("floor", wm.FLOOR), state=None if state is None else state[i])
        states.append(s)
    return out, states


def _seed_rows(states):
    return torch.from_numpy(np.frombuffer(b"".join(wm.state_bytes(s) for s in states), dtype=np.uint8).reshape(len(states), 16).copy()).cuda()


def _signal(n, N, seed):
    """Noise with a stretch of digital silence and a loud burst: the envelope rises, holds and decays."""
    x = (0.05 * np.random.default_rng(seed).standard_normal((n, N))).astype(np.float32)
    x[:, N // 5:N // 3] = 0.0
    x[:, N // 2:N // 2 + 40] *= 9.0
    return x


# ------------------------------------------------------------------------------------------------ 1. embed, whole signal

@pytest.mark.parametrize("N", [64, 320, 1280, 1281, 5 * 1280 + 37])
def test_embed_whole_signal_is_the_reference(full, N):
    x = _signal(3, N, N)
    buf = torch.full((3, N + 24), 7.0, device="cuda")      # a sentinel behind every row
    buf[:, :N] = torch.from_numpy(x).cuda()
    view = buf[:, :N]
    want, states = _law(x)
    got, st = full.watermark_embed(view, state=True, **MARK)      # out != x
    assert np.array_equal(_u32(got), _u32(want)) and np.array_equal(_u32(view), _u32(x)) and not np.array_equal(_u32(want), _u32(x))
    assert bytes(_np(st).tobytes()) == b"".join(wm.state_bytes(s) for s in states)
    # rows of different lengths in one call, from seed records, another cfg; the samples behind a row's length come back as they came
    lens = [N, N // 2, min(N, 64)]
    seeds = [dict(pos=7 * 2048 - 64, env=np.float32(0.02)), dict(pos=3, env=np.float32(0.0)), dict(pos=24 * 2048 * 5 + 2047, env=np.float32(0.5))]
    want2, states2 = _law(x, state=seeds, lens=lens, **OTHER)
    got2, st2 = full.watermark_embed(view, lens=lens, seed=_seed_rows(seeds), state=True, **OTHER)
    assert np.array_equal(_u32(got2), _u32(want2)) and bytes(_np(st2).tobytes()) == b"".join(wm.state_bytes(s) for s in states2)
    # in place, with state_out == seed, through the C call
    seed = _seed_rows(seeds)
    c = _lib.watermark_cfg(**OTHER)
    sm = np.asarray(lens, dtype=np.int64)
    _lib.check(full.lib.conan_watermark_embed(full.h, C.byref(c), _ptr(view), 3, sm.ctypes.data_as(C.c_void_p), buf.stride(0), _ptr(seed), _ptr(view), _ptr(seed),
                                              _stream()))
    torch.cuda.synchronize()
    assert np.array_equal(_u32(view), _u32(want2)) and bytes(_np(seed).tobytes()) == bytes(_np(st2).tobytes())
    assert bool((buf[:, N:] == 7.0).all())
    # out=x through the Python layer
    buf[:, :N] = torch.from_numpy(x).cuda()
    assert full.watermark_embed(view, out=view, **MARK) is view
    assert np.array_equal(_u32(view), _u32(want)) and bool((buf[:, N:] == 7.0).all())


def test_embed_any_cut_through_the_state_is_the_whole_signal(full):
    x = torch.from_numpy(_signal(2, 11 * U, 3)).cuda()
    whole = full.watermark_embed(x, **MARK)
    out, seed, pos = [], None, 0
    for frames in [4, 1, 7, 4, 1, 7, 4, 1, 7, 4, 4]:
        y, seed = full.watermark_embed(x[:, pos:pos + frames * HOP], seed=seed, state=True, **MARK)
        out.append(y)
        pos += frames * HOP
    assert pos == x.shape[1] and np.array_equal(_u32(torch.cat(out, 1)), _u32(whole))
    assert np.array_equal(_u32(whole), _u32(_law(x)[0]))


# ------------------------------------------------------------------------------------------------ 2. embed, streaming

def _voc(st, slots, mel, sizes):
    outs, pos, k = [], 0, 0
    while pos < mel.shape[1]:
        f = min(sizes[k % len(sizes)], mel.shape[1] - pos)
        outs.append(st.hifigan_step(slots, mel[:, pos:pos + f].contiguous()).clone())
        pos, k = pos + f, k + 1
    torch.cuda.synchronize()
    return torch.cat(outs, 1), k


def test_blocking_vocoder_steps_equal_the_whole_signal_form(full):
    mel = torch.from_numpy(synth.mel(24, 5, 2)).cuda()
    a, b = full.streams(MAX_SLOTS, 8, 64), full.streams(MAX_SLOTS, 8, 64)
    bytes_never, lid, snap = b.state_bytes, b.layout_id, b.snapshot_bytes
    for st in (a, b):
        st.reset(SLOTS, which=4)
    b.set_watermark(SLOTS, None)      # turning off what was never on allocates nothing
    assert b.state_bytes == bytes_never and b.watermark(SLOTS) == [None, None]
    a.set_watermark([1], **MARK)
    assert a.watermark(SLOTS) == [_lib.watermark_keywords(_lib.watermark_cfg(**MARK)), None]
    assert a.state_bytes == bytes_never + MAX_SLOTS * (16 + 8 * ROW_BYTES) and (a.layout_id, a.snapshot_bytes) == (lid, snap)
    (w1, steps), la = _launches(a, lambda: _voc(a, SLOTS, mel, [4, 1, 7]))
    (w0, _), lb = _launches(b, lambda: _voc(b, SLOTS, mel, [4, 1, 7]))
    assert steps == 6 and w0.shape[1] == 24 * HOP
    want, _ = _law(w0[:1])
    assert np.array_equal(_u32(w1[0]), _u32(want[0])) and not np.array_equal(_u32(w1[0]), _u32(w0[0]))
    assert np.array_equal(_u32(w1[1]), _u32(w0[1]))      # the unmarked slot keeps its bits
    assert np.array_equal(_u32(w1[:1]), _u32(full.watermark_embed(w0[:1], **MARK)))
    assert "watermark_embed_kernel" not in lb
    assert la.pop("watermark_embed_kernel") == steps and la == lb, (la, lb)      # exactly one more launch per marked step
    # a step without a marked row runs the launches of a stream-set that never heard of the feature
    a.reset([4], which=4); b.reset([4], which=4)
    (wa, _), la = _launches(a, lambda: _voc(a, [4], mel[1:], [4]))
    (wb, _), lb = _launches(b, lambda: _voc(b, [4], mel[1:], [4]))
    assert la == lb and np.array_equal(_u32(wa), _u32(wb))
    a.close(); b.close()


def test_pipelined_steps_equal_the_whole_signal_form(full):
    src = _noise(2, 6 * U + 700, 41)
    b = _open(full, SLOTS)
    (c0, m0, w0, _, _), emits = _run(b, SLOTS, src, pipelined=True, contour=False)
    b.reset(SLOTS, which=15)
    b.set_reference(SLOTS, _ref(2))
    ((_, _, wb, _, _), _), lb = _launches(b, lambda: _run(b, SLOTS, src, contour=False))      # (the profile hooks take blocking steps)
    b.close()
    assert np.array_equal(_u32(wb), _u32(w0))
    a = _open(full, SLOTS)
    a.set_watermark([4], **MARK)
    (c1, m1, w1, _, _), _ = _run(a, SLOTS, src, pipelined=True, contour=False)
    assert torch.equal(c1, c0) and torch.equal(m1, m0)      # the mark touches no model input
    assert np.array_equal(_u32(w1[0]), _u32(w0[0])) and np.array_equal(_u32(w1[1]), _u32(_law(w0[1:])[0][0]))
    state = wm.state_from(_np(a.watermark_state([4]))[0].tobytes())
    assert state["pos"] == w0.shape[1] and state["env"] == _law(w0[1:])[1][0]["env"]
    a.reset(SLOTS, which=15)
    a.set_reference(SLOTS, _ref(2))
    ((_, _, wa, _, _), _), la = _launches(a, lambda: _run(a, SLOTS, src, contour=False))
    assert np.array_equal(_u32(wa), _u32(w1))      # blocking and pipelined steps give the same bits, and the reset restarted the state
    assert la.pop("watermark_embed_kernel") == len(emits) and la == lb, (la, lb)
    a.close()
    # mel-in, through the engine: conan_step_async
    mel = torch.from_numpy(synth.mel(23, 9, 2)).cuda()
    eng = StreamingVoiceConversionEngine(full, 2, max_ref_frames=64)
    w0, m0, _ = eng.infer(mel, _ref(2), pipelined=True)
    torch.cuda.synchronize()
    w0 = w0.clone()
    w1, m1, _ = eng.infer(mel, _ref(2), pipelined=True, watermark=[MARK, None])
    torch.cuda.synchronize()
    assert torch.equal(m1, m0) and np.array_equal(_u32(w1[0]), _u32(_law(w0[:1])[0][0])) and np.array_equal(_u32(w1[1]), _u32(w0[1]))
    w2, _, _ = eng.infer(mel, _ref(2), pipelined=True)      # watermark=None turns it off again
    torch.cuda.synchronize()
    assert np.array_equal(_u32(w2), _u32(w0)) and eng.st.watermark(eng.slots) == [None, None]
    eng.st.close()


def test_position_in_the_chain(full):
    """The gate, the comfort fill, an 8 kHz output rate and mu-law on one slot: the bytes equal conan_resample and
    conan_convert_samples of the marked 16 kHz audio - the mark sits behind the fill and in front of the resampler."""
    src = _bursts(1, 9)
    eng = StreamingVoiceConversionEngine(full, 1, max_ref_frames=64)
    w0, _, _ = eng.infer_wav(src, _ref(1), pipelined=False, activity=dict(KW), comfort=True)
    torch.cuda.synchronize()
    w0 = w0.clone()
    plain, _, _ = eng.infer_wav(src, _ref(1), pipelined=False)
    torch.cuda.synchronize()
    assert not np.array_equal(_u32(plain), _u32(w0))      # gate and fill moved the audio
    got, _, _ = eng.infer_wav(src, _ref(1), pipelined=False, activity=dict(KW), comfort=True, watermark=MARK, out_rate=8000, out_format="ulaw")
    torch.cuda.synchronize()
    marked = full.watermark_embed(w0, **MARK)
    assert np.array_equal(_u32(marked), _u32(_law(w0)[0]))
    want = full.convert_samples(full.resample(marked, 16000, 8000), "f32", "ulaw")
    assert got.dtype == torch.uint8 and got.shape == want.shape and torch.equal(got, want), int((got != want).sum())
    assert not torch.equal(want, full.convert_samples(full.resample(w0, 16000, 8000), "f32", "ulaw"))
    eng.st.close()


# ------------------------------------------------------------------------------------------------ 3. the setter

def test_setter_between_pipelined_steps_and_the_reset_rule(full):
    src = _noise(2, 8 * U + 10, 95)
    b = _open(full, SLOTS)
    (_, _, w0, _, _), emits = _run(b, SLOTS, src, pipelined=True, contour=False)
    b.close()
    a = _open(full, SLOTS)
    a.set_watermark(SLOTS, **MARK)
    out_before = []

    def hook(k):      # call k emits chunk k - 1: in front of call 5 four chunks are out
        if k == 5:
            a.set_watermark([1], **OTHER)                   # reseed = 0: key, id, gain and floor change, pos and env stay
            a.set_watermark([4], reseed=True, **OTHER)      # reseed = 1 without a seed: from {0, 0}
            out_before.append(4 * U)
    (_, _, w1, _, _), _ = _run(a, SLOTS, src, pipelined=True, contour=False, on_call=hook)
    cut = out_before[0]
    head, states = _law(w0[:, :cut])
    keep, _ = _law(w0[:1, cut:], state=states[:1], **OTHER)
    fresh, _ = _law(w0[1:, cut:], **OTHER)
    assert np.array_equal(_u32(w1[0]), _u32(np.concatenate([head[0], keep[0]])))
    assert np.array_equal(_u32(w1[1]), _u32(np.concatenate([head[1], fresh[0]])))
    assert not np.array_equal(_u32(keep[0]), _u32(_law(w0[:1, cut:], **OTHER)[0][0]))      # the kept state matters
    # a reset with the vocoder restarts the state and keeps the setting; one without it keeps both
    a.reset(SLOTS, which=15)
    a.set_reference(SLOTS, _ref(2))
    assert a.watermark([1]) == [_lib.watermark_keywords(_lib.watermark_cfg(**OTHER))]
    assert not _np(a.watermark_state(SLOTS)).any()      # about to restart: the zero record
    (_, _, w2, _, _), _ = _run(a, SLOTS, src, contour=False)
    assert np.array_equal(_u32(w2), _u32(_law(w0, **OTHER)[0]))
    before = _np(a.watermark_state(SLOTS)).copy()
    a.reset(SLOTS, which=1 | 2 | 8)
    assert np.array_equal(_np(a.watermark_state(SLOTS)), before) and wm.state_from(before[0].tobytes())["pos"] == w0.shape[1]
    a.close()


def test_hand_over_continues_bit_for_bit(full):
    src = _noise(2, 8 * U + 10, 96)
    b = _open(full, SLOTS)
    (_, _, w0, _, _), _ = _run(b, SLOTS, src, contour=False)
    b.close()
    want, _ = _law(w0)
    dst = [3, 0]
    a = _open(full, SLOTS)
    b = full.streams(MAX_SLOTS, 4, 64)
    lid, nbytes = b.layout_id, b.snapshot_bytes
    a.set_watermark(SLOTS, **MARK)
    head = []
    for k in range(5):
        e, _, _, w = a.step_wav(SLOTS, src[:, k * U:(k + 1) * U])
        if e:
            head.append(w.clone())
    assert len(head) == 4
    state = a.watermark_state(SLOTS)
    assert state.shape == (2, 16) and wm.state_from(_np(state)[0].tobytes())["pos"] == 4 * U
    b.import_slots(dst, a.export_slots(SLOTS))
    assert b.watermark(dst) == [None, None] and (a.layout_id, a.snapshot_bytes, b.layout_id, b.snapshot_bytes) == (lid, nbytes, lid, nbytes)
    b.set_watermark(dst, seed=state, reseed=True, **MARK)
    assert torch.equal(b.watermark_state(dst), state)
    N = src.shape[1]
    calls = [(p, p + U, False) for p in range(0, (N - 1) // U * U, U)] + [((N - 1) // U * U, N, True)]
    tail = []
    for p, q, fin in calls[5:]:
        e, _, _, w = b.step_wav(dst, src[:, p:q], final=fin)
        if e:
            tail.append(w.clone())
    while True:
        e, _, _, w = b.step_wav(dst, src[:, :0], final=True)
        if e == 0:
            break
        tail.append(w.clone())
    torch.cuda.synchronize()
    assert np.array_equal(_u32(torch.cat(head + tail, 1)), _u32(want))
    a.close(); b.close()


def test_refused_calls_change_nothing(full):
    mel = torch.from_numpy(synth.mel(8, 5, 2)).cuda()
    st = full.streams(MAX_SLOTS, 4, 64)
    st.reset(SLOTS, which=4)
    with pytest.raises(_lib.ConanError) as e:      # the query on a stream-set that never enabled the feature
        st.watermark_state([1])
    assert e.value.code == _lib.ERR_STATE
    st.set_watermark([1], **MARK)
    first = st.hifigan_step(SLOTS, mel[:, :4].contiguous()).clone()
    before, state = st.watermark(SLOTS), st.watermark_state([1]).clone()
    bad = _lib.watermark_cfg(**OTHER)
    bad.reserved[3] = 1
    for slots, cfg, kw, code in (([1, 1], True, OTHER, _lib.ERR_INVALID), ([1, MAX_SLOTS], True, OTHER, _lib.ERR_INVALID), ([1], bad, {}, _lib.ERR_INVALID)):
        with pytest.raises(_lib.ConanError) as e:
            st.set_watermark(slots, cfg, **kw)
        assert e.value.code == code, (slots, kw)
    with pytest.raises(_lib.ConanError) as e:      # a seed whose rows are too close
        st.set_watermark(SLOTS, seed=torch.zeros(2, 8, dtype=torch.uint8, device="cuda"), reseed=True, **OTHER)
    assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.ConanError) as e:
        st.watermark_state([1, 4])      # a slot without the feature
    assert e.value.code == _lib.ERR_STATE
    assert st.watermark(SLOTS) == before and torch.equal(st.watermark_state([1]), state)
    rest = st.hifigan_step(SLOTS, mel[:, 4:].contiguous()).clone()
    plain = full.streams(MAX_SLOTS, 4, 64)
    plain.reset(SLOTS, which=4)
    w0 = torch.cat([plain.hifigan_step(SLOTS, mel[:, :4].contiguous()).clone(), plain.hifigan_step(SLOTS, mel[:, 4:].contiguous()).clone()], 1)
    torch.cuda.synchronize()
    w1 = torch.cat([first, rest], 1)
    assert np.array_equal(_u32(w1[0]), _u32(_law(w0[:1])[0][0])) and np.array_equal(_u32(w1[1]), _u32(w0[1]))
    st.close(); plain.close()
    # the whole-prefix vocoder of upsample 'nn': refused before anything changes, as for the output leveller
    vhp = dict(configs.hifigan_hparams(True), upsample="nn")
    nn = Context(None, vhp, 0, emformer=False, conan=False)
    nn.load_state_dict("hifigan", synth.hifigan_state_dict(vhp, 0))
    nn.finalize()
    s = nn.streams(2, 8, 64)
    bytes_never = s.state_bytes
    with pytest.raises(_lib.ConanError) as e:
        s.set_watermark([0], **MARK)
    assert e.value.code == _lib.ERR_UNSUPPORTED and s.state_bytes == bytes_never and s.watermark([0]) == [None]
    s.set_watermark([0], None)      # "off" is always accepted
    s.close(); nn.close()


# ------------------------------------------------------------------------------------------------ 4. detect

def _marked_noise(n, N, seed, amp=0.2):
    x = (amp * np.random.default_rng(seed).standard_normal((n, N))).astype(np.float32)
    return np.stack([wm.embed(r, KEY, ID)[0] for r in x])


def _check_rows(full, rows, fmt, lens=None, key=KEY):
    """The library's detector on rows (numpy, in fmt's dtype) against the reference on the same rows."""
    got = full.watermark_detect(torch.from_numpy(rows).cuda(), key, format=fmt, lens=lens, raw=True)
    assert len(got) == rows.shape[0]
    for i, g in enumerate(got):
        m = rows.shape[1] if lens is None else lens[i]
        r = wm.detect_decide(cases.view(fmt, rows[i, :m]), key)
        assert np.array_equal(g["S"], r["S"]) and np.array_equal(g["soft"], r["soft"]), (fmt, i, m)
        assert (g["offset"], g["blocks"], g["peak"], g["id"], g["rotation"], g["marker_score"]) == \
            (r["offset"], r["blocks"], r["peak"], r["id"], r["rotation"], r["marker_score"]), (fmt, i, m)
        assert abs(g["z"] - r["z"]) <= 1e-12 * abs(r["z"]) and g["present"] == bool(r["present"]), (fmt, i, g["z"], r["z"])
    return got


@pytest.mark.parametrize("fmt", ["f32", "s16", "ulaw", "alaw"])
@pytest.mark.parametrize("n", [4095, 4096, 4097, 3 * 2048 + 5])
def test_detect_is_the_reference(full, n, fmt):
    x = _marked_noise(2, n, n)
    if fmt == "f32":
        x[0, 5:9] = [1.5, -1.5, 2.5 / 32768, -0.5 / 32768]      # beyond the range, and ties
    got = _check_rows(full, sf.encode(x, fmt), fmt)
    assert all(g["blocks"] == wm.blocks(n) for g in got)
    if wm.blocks(n) == 0:
        assert all((g["present"], g["z"], g["id"], g["offset"]) == (False, 0.0, 0, 0) and not g["S"].any() for g in got)


def test_detect_rows_of_different_lengths_in_one_call(full):
    x = _marked_noise(3, 6 * 2048 + 5, 12)
    got = _check_rows(full, sf.encode(x, "s16"), "s16", lens=[6 * 2048 + 5, 4096, 4095])
    assert [g["blocks"] for g in got] == [5, 1, 0]
    _check_rows(full, sf.encode(x, "ulaw"), "ulaw", lens=[4097, 6 * 2048 + 5, 3 * 2048])


@pytest.mark.parametrize("name", ["chips", "alternating"])
def test_detect_on_the_adversarial_rows_of_the_bound(full, name):
    q = cases.adversarial(name, KEY, 3 * wm.BLK)
    rows = np.stack([q, -q - (name == "alternating")]).astype(np.int16)      # (the mirrored alternation: 32767, -32768, ...)
    _check_rows(full, rows, "s16")
    r = wm.detect(rows[0].astype(np.int64), KEY)
    assert int(np.abs(r["R"]).max()) <= wm.R_BOUND < 2 ** 31


# ------------------------------------------------------------------------------------------------ 5. the robustness matrix

def test_robustness_matrix_through_the_library(full):
    def embed(x, key):
        y = _np(full.watermark_embed(torch.from_numpy(x).cuda(), key=key, id=ID))
        assert np.array_equal(_u32(y), _u32(wm.embed(x, key, ID)[0]))
        return y

    def channels(y):
        t = torch.from_numpy(y).cuda()[None]
        code8 = full.convert_samples(full.resample(t, 16000, 8000), "f32", "ulaw")
        back = full.resample(full.convert_samples(code8, "ulaw", "f32"), 8000, 16000)
        return dict(s16=("s16", _np(full.convert_samples(t, "f32", "s16"))[0]), ulaw16=("ulaw", _np(full.convert_samples(t, "f32", "ulaw"))[0]),
                    ulaw8=("f32", _np(back)[0]))

    def detect(name, kind, ch, fmt, row, q):
        g = full.watermark_detect(torch.from_numpy(row).cuda(), KEY, format=fmt, raw=True)[0]
        r = wm.detect_decide(q, KEY)
        assert np.array_equal(g["S"], r["S"]) and np.array_equal(g["soft"], r["soft"]) and (g["offset"], g["blocks"], g["peak"]) == (r["offset"], r["blocks"], r["peak"])
        assert (g["id"], g["rotation"]) == (r["id"], r["rotation"]) and abs(g["z"] - r["z"]) <= 1e-12 * abs(r["z"])
        return g

    res = cases.matrix(detect, channels, embed)
    marked = [r for (name, kind, ch), r in res.items() if kind == "marked"]
    others = [r for (name, kind, ch), r in res.items() if kind != "marked"]
    assert len(marked) == 6 and len(others) == 12
    for (name, kind, ch), r in sorted(res.items()):
        print(f"{name:6s} {kind:9s} {ch:7s} z = {r['z']:6.2f} id = {r['id']:04x} offset = {r['offset']} rotation = {r['rotation']}")
    for r in marked:
        assert r["id"] == ID and min((r["offset"] - cases.OFFSET) % wm.BLK, (cases.OFFSET - r["offset"]) % wm.BLK) <= 1
    lo, hi = max(r["z"] for r in others), min(r["z"] for r in marked)
    assert lo < _lib.WATERMARK_THRESHOLD < hi
    assert all(r["present"] for r in marked) and not any(r["present"] for r in others)
    # rate=: mu-law at 8 kHz goes through the library's decoder and resampler in front of the same detector
    y = cases.rows()["tones", "marked"]
    code8 = full.convert_samples(full.resample(torch.from_numpy(y).cuda()[None], 16000, 8000), "f32", "ulaw")
    a = full.watermark_detect(code8, KEY, format="ulaw", rate=8000, raw=True)[0]
    b = res["tones", "marked", "ulaw8"]
    assert np.array_equal(a["S"], b["S"]) and (a["id"], a["offset"], a["z"], a["present"]) == (b["id"], b["offset"], b["z"], True)
