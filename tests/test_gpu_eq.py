"""The equaliser on the GPU (conan_eq; include/conan_hip.h, conan_eq_cfg) against tests/eq_ref.py, bit for bit: nothing here has a
tolerance.  The law is single rounded f64 operations in a fixed order, so the library's f32 samples and its state records are
compared with the reference's by their bytes."""
import numpy as np
import pytest
import torch

from conan_amd import _lib
from tests import eq_ref as R
from tests.test_gpu_pitch import full  # noqa: F401  (module fixture: the small synthetic full model)

pytestmark = pytest.mark.gpu

LENGTHS = (1, 127, 128, 129, 1280, 1281, 5 * 1280 + 37)
ONE = [R.cookbook("highpass", 16000.0, 80.0)]
FOUR = R.cascade4()
FAST = [(1.0, 0.0, 0.0, -0.64, 0.1024)]      # a double pole at 0.32: the state decays into the f64 denormals within 650 samples


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    g, w = _bits(got.cpu().numpy() if torch.is_tensor(got) else got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, bad[:8], bad.size)


@pytest.fixture(scope="module")
def refs():
    """Per cascade the reference's rows of every length in LENGTHS (one signal each), computed once and left unchanged."""
    out = {}
    for name, sec in (("one", ONE), ("four", FOUR)):
        for N in LENGTHS:
            x = R.signal(N, seed=N)
            y, s = R.run(x, sec, cuts=[R.MAX_CALL])
            out[name, N] = (x, y, s.state_bytes())
    return out


@pytest.mark.parametrize("name", ["one", "four"])
def test_conan_eq_equals_the_reference(full, refs, name):
    """Rows of different lengths under one wider row stride in one call, the state rows, and the same call in place."""
    sec = ONE if name == "one" else FOUR
    ld = max(LENGTHS) + 19
    x = torch.full((len(LENGTHS), ld), 7.0)
    for i, N in enumerate(LENGTHS):
        x[i, :N] = torch.from_numpy(refs[name, N][0])
    xd = x.cuda()
    view = xd[:, :max(LENGTHS)]      # a 2-D view that keeps the wider stride
    y, st = full.eq(view, sections=sec, lengths=LENGTHS, return_state=True)
    torch.cuda.synchronize()
    rows = st.cpu().numpy()
    assert rows.shape == (len(LENGTHS), R.STATE_BYTES)
    for i, N in enumerate(LENGTHS):
        _same(y[i, :N], refs[name, N][1], (name, N))
        assert (y[i, N:].cpu() == 7.0).all()      # the floats behind a row's length come back as they came
        assert rows[i].tobytes() == refs[name, N][2], (name, N)
    z = full.eq(view, sections=sec, lengths=LENGTHS, out=xd)
    torch.cuda.synchronize()
    assert z.data_ptr() == xd.data_ptr()
    for i, N in enumerate(LENGTHS):
        _same(xd[i, :N], refs[name, N][1], (name, N, "in place"))
        assert (xd[i, N:].cpu() == 7.0).all()


def test_a_silent_stretch_keeps_the_denormals(full):
    x = R.signal(6000, seed=5)
    x[1000:5000] = 0.0
    want, _ = R.run(x, FAST + ONE)
    y = full.eq(torch.from_numpy(x).cuda(), sections=FAST + ONE)
    _same(y, want)
    # the state really passes through the denormal range on the way: the fast section's impulse response (n + 1) 0.32^n is about
    # 2^-1043 at n = 640, a segment's start, and a record taken behind it holds denormal words that equal the reference's
    imp = np.concatenate([np.ones(1, np.float32), np.zeros(650, np.float32)])
    dec, sd = R.run(imp, FAST, f64=True)
    assert 0.0 < abs(dec[-1]) < 2.3e-308, dec[-1]
    assert any(0.0 < abs(v) < 2.3e-308 for v in sd.carry[0])
    got = full.eq(torch.from_numpy(imp).cuda(), sections=FAST, return_state=True)[1]
    assert got.cpu().numpy().tobytes() == sd.state_bytes()


def test_a_non_finite_sample_counts_as_zero(full):
    x = R.signal(3000, seed=9)
    x[700], x[701], x[2049] = np.nan, np.inf, -np.inf
    want, s = R.run(x, FOUR)
    assert np.isfinite(want).all()
    y, st = full.eq(torch.from_numpy(x).cuda(), sections=FOUR, return_state=True)
    assert torch.isfinite(y).all()
    _same(y, want)
    assert st.cpu().numpy().tobytes() == s.state_bytes()
    clean = x.copy()
    clean[[700, 701, 2049]] = 0.0
    _same(y, R.run(clean, FOUR)[0])


def test_chained_calls_equal_the_whole_signal(full):
    """The cut independence on the device: calls of 1, 127, 128, 129 ... samples chained through the state record give the whole
    signal's bits and the whole signal's state."""
    N = 4000
    x = R.signal(N, seed=11)
    want, s = R.run(x, FOUR)
    xd = torch.from_numpy(x).cuda()
    cuts, pos, seed, parts = [1280, 333, 1, 127, 128, 129, 1000, 1002], 0, None, []
    for m in cuts:
        cfg = _lib.eq_cfg(FOUR, origin=0, pos=pos)
        y, seed = full.eq(xd[pos:pos + m], cfg=cfg, seed=seed, return_state=True)
        parts.append(y)
        pos += m
    assert pos == N
    _same(torch.cat(parts), want)
    assert seed.cpu().numpy().tobytes() == s.state_bytes()


def test_refusals(full):
    x = torch.zeros(1, 64).cuda()
    bad = [[(1.0, 0.0, 0.0, 0.0, 1.0)], [(1.0, 0.0, 0.0, 2.1, 0.99)], [(float("nan"), 0.0, 0.0, 0.0, 0.0)], [(1e6, 0.0, 0.0, 0.0, 0.0)]]
    for sec in bad:
        with pytest.raises(_lib.ConanError) as e:
            full.eq(x, sections=sec)
        assert e.value.code == _lib.ERR_INVALID
    c = _lib.eq_cfg(ONE)
    c.sections = 5
    with pytest.raises(_lib.ConanError) as e:
        full.eq(x, cfg=c)
    assert e.value.code == _lib.ERR_INVALID
    c = _lib.eq_cfg(ONE, origin=0, pos=5)      # a position behind the origin needs the seed record it continues
    with pytest.raises(_lib.ConanError) as e:
        full.eq(x, cfg=c)
    assert e.value.code == _lib.ERR_INVALID


# ------------------------------------------------------------------------------------------ the stream-set's two stages
from conan_amd import synth  # noqa: E402
from conan_amd.engine import StreamingVoiceConversionEngine  # noqa: E402
from tests.test_gpu_f0 import HOP, L, MAX_SLOTS, SEG, _launches, _ragged, _run, _wav  # noqa: E402

ALT = [R.cookbook("lowshelf", 16000.0, 300.0, 0.7, -6.0), R.cookbook("peak", 16000.0, 1800.0, 1.5, 4.0)]
EQ, EQ_ALT = dict(sections=FOUR), dict(sections=ALT)


def _open(full, slots, seed=3):
    """Slots that share one reference, so that two of them fed the same audio give the same bits."""
    st = full.streams(MAX_SLOTS, 4, 64)
    st.reset(slots, which=15)
    st.set_reference(slots, torch.from_numpy(synth.mel(40, seed, 1)).cuda().repeat(len(slots), 1, 1))
    return st


def _equal(a, b, rows=slice(None)):
    for i in range(3):      # codes, mel, wav
        assert torch.equal(a[i][rows], b[i][rows]), i


@pytest.mark.parametrize("case", ["plain", "level", "rate8k"])
def test_source_side_equals_a_slot_fed_conan_eq(full, case):
    """Slot A has the equaliser and is fed x; slot B has none and is fed conan_eq(x): five chunks and a short final call."""
    N = 5 * L + 300
    x = _wav(1, N, 21)
    if case == "rate8k":
        x8 = _wav(1, N // 2, 22)
        a, b = _open(full, [1]), _open(full, [1])
        a.set_input_rate([1], 8000)
        a.set_input_eq([1], EQ)
        ga, _ = _run(a, [1], x8, contour=False, lin=L // 2)
        gb, _ = _run(b, [1], full.eq(full.resample(x8, 8000, 16000), sections=FOUR), contour=False)
        _equal(ga, gb)
        a.close(); b.close()
        return
    st = _open(full, [1, 4])
    if case == "level":
        st.set_input_level([1, 4], True)
    st.set_input_eq([1], EQ)
    assert st.input_eq([1, 4]) == [dict(_lib.eq_keywords(_lib.eq_cfg(FOUR)), origin=0, pos=0), None]
    got, _ = _run(st, [1, 4], torch.cat([x, full.eq(x, sections=FOUR)]), contour=False)
    for i in range(3):
        assert torch.equal(got[i][0], got[i][1]), (case, i)
    assert st.input_eq([1])[0]["pos"] == N
    st.close()


def test_output_side_equals_conan_eq_of_the_unfiltered_audio(full):
    N = 4 * L + 200
    x = _wav(1, N, 31)
    st = _open(full, [2])
    raw, _ = _run(st, [2], x, contour=False)
    st.reset([2], which=15)
    st.set_reference([2], torch.from_numpy(synth.mel(40, 3, 1)).cuda())
    st.set_output_eq([2], EQ)
    got, _ = _run(st, [2], x, contour=False)
    assert torch.equal(got[0], raw[0]) and torch.equal(got[1], raw[1])
    _same(got[2], full.eq(raw[2], sections=FOUR).cpu().numpy(), "step_wav")
    # with the output leveller behind it: conan_level(conan_eq(raw))
    st.reset([2], which=15)
    st.set_reference([2], torch.from_numpy(synth.mel(40, 3, 1)).cuda())
    st.set_output_level([2], True)
    lev, _ = _run(st, [2], x, contour=False)
    _same(lev[2], full.level(full.eq(raw[2], sections=FOUR)).cpu().numpy(), "levelled")
    st.close()
    # the mel-in steps, and an 8 kHz mu-law output: the encoded bytes
    eng = StreamingVoiceConversionEngine(full, 2, max_ref_frames=64)
    src, ref = torch.from_numpy(synth.mel(19, 5, 2)).cuda(), torch.from_numpy(synth.mel(40, 6, 2)).cuda()
    w0 = eng.infer(src, ref)[0]
    w1 = eng.infer(src, ref, out_eq=[EQ, EQ_ALT])[0]
    _same(w1[0], full.eq(w0[0], sections=FOUR).cpu().numpy(), "mel-in")
    _same(w1[1], full.eq(w0[1], sections=ALT).cpu().numpy(), "mel-in, another cascade")
    w8 = eng.infer(src, ref, out_eq=EQ, out_rate=8000, out_format="ulaw")[0]
    want = full.convert_samples(full.resample(full.eq(w0, sections=FOUR), 16000, 8000), "f32", "ulaw")
    assert torch.equal(w8, want)
    assert torch.equal(eng.infer(src, ref)[0], w0)      # off again: today's bits
    eng.st.close()


def test_ragged_and_pipelined(full):
    """Three slots at different positions with different lengths, two of them filtered with different cascades."""
    slots, starts = [5, 0, 2], [0, 1, 3]
    wavs = [_wav(1, n, 40 + i)[0] for i, n in enumerate((4 * L + 333, 3 * L, 2 * L + 1))]
    fed = [full.eq(wavs[0], sections=FOUR), wavs[1], full.eq(wavs[2], sections=ALT)]

    def run(filtered, pipelined):
        st = _open(full, slots)
        if filtered:
            st.set_input_eq([5], EQ)
            st.set_input_eq([2], EQ_ALT)
            st.set_output_eq([0], EQ_ALT)
        out = _ragged(st, slots, wavs if filtered else fed, starts, pipelined=pipelined, contour=False)
        st.close()
        return out

    a, b, c = run(True, False), run(False, False), run(True, True)
    for u in range(3):
        for i in range(3):
            assert torch.equal(a[u][i], c[u][i]), ("pipelined", u, i)
            if u != 1 or i < 2:
                assert torch.equal(a[u][i], b[u][i]), ("against conan_eq", u, i)
    _same(a[1][2], full.eq(b[1][2], sections=ALT).cpu().numpy(), "the output side of the middle slot")


def _calls(st, slot, x, lin, first=0, until=None, hook=None):
    """step_wav calls of `lin` input samples over x [1, N] from call `first` on (until: stop in front of that call; None: drain) ->
    the emitted (codes, mel, wav) pieces.  hook(k) runs in front of call k."""
    N = x.shape[1]
    last = (N - 1) // lin * lin
    calls = [(p, p + lin, False) for p in range(0, last, lin)] + [(last, N, True)]
    outs, k = [], first
    while until is None or k < until:
        if hook:
            hook(k)
        if k < len(calls):
            p, q, fin = calls[k]
            e, c, m, w = st.step_wav([slot], x[:, p:q], final=fin)
        else:
            e, c, m, w = st.step_wav([slot], x[:, :0], final=True)
            if e == 0:
                break
        k += 1
        if e:
            outs.append((c[:, :e].clone(), m.clone(), w.clone()))
    torch.cuda.synchronize()
    return outs


def _cat(outs):
    return [torch.cat([o[i] for o in outs], 1) for i in range(3)]


def test_live_change_and_enabling_off_the_segment_grid(full):
    """An 8 kHz input: the resampler hands the front-end a count of its own per call, so the change finds a pending tail, which
    must be closed with the OLD coefficients.  The slot without the feature is fed the reference's rows with that change list."""
    N8 = (5 * L + 300) // 2
    x8 = _wav(1, N8, 51)
    x16 = full.resample(x8, 8000, 16000)
    xn = x16[0].cpu().numpy()
    seen = {}

    def run(first, then, key):
        st = _open(full, [1])
        st.set_input_rate([1], 8000)
        if first is not None:
            st.set_input_eq([1], first)

        def hook(k):
            if k == 3:
                before = st.input_eq([1])[0] if first is not None else None
                st.set_input_eq([1], then)
                after = st.input_eq([1])[0]
                seen[key] = after["pos"]
                assert after["origin"] == after["pos"] and (before is None or before["origin"] == 0 and before["pos"] == after["pos"])
        out = _cat(_calls(st, 1, x8, L // 2, hook=hook))
        rec = _lib.EqState.from_buffer_copy(st.input_eq_state([1]).cpu().numpy().tobytes())
        assert (rec.origin, rec.pos) == (seen[key], len(xn))
        st.close()
        return out

    changed, enabled = run(EQ, EQ_ALT, "change"), run(None, EQ_ALT, "enable")
    pos = seen["change"]
    assert pos == seen["enable"] and pos % R.SEG != 0 and 0 < pos < len(xn), pos      # the tail is not empty
    want_change, _ = R.run(xn, FOUR, changes=[(pos, ALT)])
    wrong, _ = R.run(xn, FOUR, changes=[(pos - pos % R.SEG, ALT)])      # what closing no tail would give
    assert not np.array_equal(want_change, wrong)
    want_enable = np.concatenate([xn[:pos], R.run(xn[pos:], ALT, origin=pos)[0]])
    for got, fed in ((changed, want_change), (enabled, want_enable)):
        plain = _open(full, [1])
        _equal(got, _cat(_calls(plain, 1, torch.from_numpy(fed)[None].cuda(), L)))
        plain.close()


def test_output_side_live_change_off_the_segment_grid(full):
    """Vocoder steps of 3, 2, 4 and 1 frames: the change behind the first finds 960 = 7.5 segments, a tail of 64 samples."""
    frames = (3, 2, 4, 1)
    mel = torch.from_numpy(synth.mel(sum(frames), 77, 1)).cuda()

    def run(first, then):
        st = full.streams(MAX_SLOTS, 4, 64)
        st.reset([2], which=15)
        if first is not None:
            st.set_output_eq([2], first)
        out, f = [], 0
        for k, T in enumerate(frames):
            if k == 1 and then is not None:
                st.set_output_eq([2], then)
                assert st.output_eq([2])[0]["origin"] == 3 * HOP == st.output_eq([2])[0]["pos"]
            out.append(st.hifigan_step([2], mel[:, f:f + T]).reshape(1, -1).clone())
            f += T
        torch.cuda.synchronize()
        st.close()
        return torch.cat(out, 1)[0]

    raw = run(None, None).cpu().numpy()
    assert (3 * HOP) % R.SEG == 64
    _same(run(EQ, EQ_ALT), R.run(raw, FOUR, changes=[(3 * HOP, ALT)])[0], "change")
    _same(run(EQ, None), R.run(raw, FOUR)[0], "steps that end off the grid")
    _same(run(None, EQ_ALT), np.concatenate([raw[:3 * HOP], R.run(raw[3 * HOP:], ALT, origin=3 * HOP)[0]]), "enable")


def test_hand_over_off_the_segment_grid(full):
    """Settings and state queried after three calls of an 8 kHz input (a pending tail on the source side), the slot exported, imported
    into another stream-set and both setters seeded: the stream continues bit for bit."""
    N8 = (5 * L + 300) // 2
    x8 = _wav(1, N8, 52)
    a, whole = _open(full, [1]), _open(full, [1])
    for s in (a, whole):
        s.set_input_rate([1], 8000)
        s.set_input_eq([1], EQ)
        s.set_output_eq([1], EQ_ALT)
    want = _cat(_calls(whole, 1, x8, L // 2))
    outs = _calls(a, 1, x8, L // 2, until=3)
    kw = a.input_eq([1])[0]
    assert kw["origin"] == 0 and kw["pos"] % R.SEG != 0, kw
    rows = a.input_eq_state([1])
    assert any(_lib.EqState.from_buffer_copy(rows.cpu().numpy().tobytes()).tail[:kw["pos"] % R.SEG])
    b = full.streams(MAX_SLOTS, 4, 64)
    b.import_slots([3], a.export_slots([1]))
    b.set_input_eq([3], kw, seed=rows)
    b.set_output_eq([3], a.output_eq([1])[0], seed=a.output_eq_state([1]))
    assert b.input_eq([3])[0] == kw
    outs += _calls(b, 3, x8, L // 2, first=3)
    _equal(_cat(outs), want)
    with pytest.raises(_lib.ConanError) as e:      # a seed that is not at the slot's position is refused
        b.set_input_eq([3], dict(kw, pos=kw["pos"] + 1), seed=rows)
    assert e.value.code == _lib.ERR_INVALID
    a.close(); b.close(); whole.close()


def test_engine_keywords(full):
    """eq= / out_eq= through the engine's wav-in entry points, the live setters and VoiceBank.enroll_wav."""
    from conan_amd.runtime import VoiceBank
    x = _wav(2, 3 * L + 100, 61)
    ref = torch.from_numpy(synth.mel(40, 6, 2)).cuda()
    eng = StreamingVoiceConversionEngine(full, 2, max_ref_frames=64)
    fed = torch.stack([full.eq(x[0], sections=FOUR), x[1]])
    w0, m0, c0 = eng.infer_wav(fed, ref)
    w1, m1, c1 = eng.infer_wav(x, ref, eq=[EQ, None], out_eq=[None, EQ_ALT])
    assert torch.equal(c1, c0) and torch.equal(m1, m0) and torch.equal(w1[0], w0[0])
    _same(w1[1], full.eq(w0[1], sections=ALT).cpu().numpy(), "infer_wav(out_eq=)")
    s0 = eng.infer_wav_staggered([fed[0], fed[1]], [0, 2], ref)
    s1 = eng.infer_wav_staggered([x[0], x[1]], [0, 2], ref, eq=[EQ, None], out_eq=[None, EQ_ALT])
    assert torch.equal(s1[0][0], s0[0][0]) and torch.equal(s1[0][1], s0[0][1]) and torch.equal(s1[1][1], s0[1][1])
    _same(s1[1][0], full.eq(s0[1][0], sections=ALT).cpu().numpy(), "infer_wav_staggered(out_eq=)")
    eng.start_wav(ref, eq=EQ)
    assert eng.st.input_eq(eng.slots) == [dict(_lib.eq_keywords(_lib.eq_cfg(FOUR)))] * 2 and eng.st.output_eq(eng.slots) == [None, None]
    eng.feed(x[:, :L])
    eng.set_eq([0], sections=ALT)
    eng.set_out_eq(sections=ALT)
    assert eng.st.input_eq([0])[0] == dict(_lib.eq_keywords(_lib.eq_cfg(ALT)), origin=L, pos=L)
    assert eng.st.output_eq([1])[0]["sections"] == _lib.eq_keywords(_lib.eq_cfg(ALT))["sections"]
    eng.set_eq(cfg=None)
    eng.set_out_eq(cfg=None)
    assert eng.st.input_eq(eng.slots) == [None, None] == eng.st.output_eq(eng.slots)
    with pytest.raises(ValueError):
        eng.start_wav(ref, eq=True)      # there is no default cascade
    eng.open_slots([1], ref[:1], eq=EQ_ALT)
    assert eng.st.input_eq([1])[0]["sections"] == _lib.eq_keywords(_lib.eq_cfg(ALT))["sections"]
    w2 = eng.infer_wav(fed, ref)[0]
    assert torch.equal(w2, w0)      # keywords absent: off again
    eng.st.close()
    via = full.streams(MAX_SLOTS, 4, 64)
    bank = VoiceBank(full, 4, 64)
    bank.enroll_wav([0, 1], x, via=via, eq=EQ)
    bank.enroll([2, 3], full.wav2mel(full.eq(x, sections=FOUR)), via=via)
    assert torch.equal(bank.export([0, 1]).blob, bank.export([2, 3]).blob)
    bank.enroll([3], full.wav2mel(x[1:]), via=via)
    assert not torch.equal(bank.export([1]).blob, bank.export([3]).blob)
    bank.close(); via.close()


def test_neighbours_and_launches(full):
    slots = [0, 1, 2, 3]
    wav = _wav(4, 3 * L + 77, 60)
    a, b = _open(full, slots), _open(full, slots)
    never = b.state_bytes
    a.set_input_eq([0], EQ)
    a.set_output_eq([2], EQ_ALT)
    assert a.state_bytes > never and b.state_bytes == never
    (ga, emits), la = _launches(a, lambda: _run(a, slots, wav, contour=False))
    (gb, _), lb = _launches(b, lambda: _run(b, slots, wav, contour=False))
    for i in (1, 3):      # slots that do not ask keep their bits
        _equal(ga, gb, i)
    assert torch.equal(ga[0][2], gb[0][2]) and torch.equal(ga[1][2], gb[1][2]) and not torch.equal(ga[2][2], gb[2][2])
    assert not torch.equal(ga[1][0], gb[1][0])
    # exactly one more launch per wav-in call with samples and one per vocoder step, and nothing else
    calls_with_samples = 4
    assert "eq_stream_kernel" not in lb
    assert la.pop("eq_stream_kernel") == calls_with_samples + len(emits)
    assert la == lb, (la, lb)
    # off again: the launches and the bits of the stream-set that never asked
    a.set_input_eq(slots, None)
    a.set_output_eq(slots, None)
    assert a.input_eq(slots) == [None] * 4 and a.output_eq(slots) == [None] * 4
    a.reset(slots, which=15)
    a.set_reference(slots, torch.from_numpy(synth.mel(40, 3, 1)).cuda().repeat(4, 1, 1))
    (g2, _), l2 = _launches(a, lambda: _run(a, slots, wav, contour=False))
    assert l2 == lb
    _equal(g2, gb)
    a.close(); b.close()


def test_refused_settings_change_nothing(full):
    from conan_amd import configs
    from conan_amd.runtime import Context
    st = _open(full, [1])
    st.set_input_eq([1], EQ)
    st.set_output_eq([1], EQ)
    before = (st.input_eq([1]), st.output_eq([1]), st.input_eq_state([1]).clone(), st.output_eq_state([1]).clone())
    five = _lib.eq_cfg(ONE)
    five.sections = 5
    for setter in (st.set_input_eq, st.set_output_eq):
        for cfg in (dict(sections=[(1.0, 0.0, 0.0, 0.0, 1.0)]), five):
            with pytest.raises(_lib.ConanError) as e:
                setter([1], cfg)
            assert e.value.code == _lib.ERR_INVALID
    assert (st.input_eq([1]), st.output_eq([1])) == before[:2]
    assert torch.equal(st.input_eq_state([1]), before[2]) and torch.equal(st.output_eq_state([1]), before[3])
    x = _wav(1, 2 * L + 5, 71)
    got, _ = _run(st, [1], x, contour=False)
    ref_st = _open(full, [1])
    ref_st.set_input_eq([1], EQ)
    ref_st.set_output_eq([1], EQ)
    want, _ = _run(ref_st, [1], x, contour=False)
    _equal(got, want)
    st.close(); ref_st.close()
    # the whole-prefix vocoder of upsample 'nn'
    vhp = dict(configs.hifigan_hparams(True), upsample="nn")
    c = Context(None, vhp, 0, emformer=False, conan=False)
    c.load_state_dict("hifigan", synth.hifigan_state_dict(vhp, 0))
    c.finalize()
    s2 = c.streams(2, 8, 64)
    with pytest.raises(_lib.ConanError) as e:
        s2.set_output_eq([0], EQ)
    assert e.value.code == _lib.ERR_UNSUPPORTED and s2.output_eq([0]) == [None]
    s2.close(); c.close()
