"""The streaming input leveller on the GPU (conan_level, conan_streams_set_input_level / _input_level; include/conan_hip.h,
conan_level_cfg) against tests/level_ref.py, the numpy restatement of the law, and against itself: the streaming form in every
stepping mode equals the whole-signal form bit for bit.

Tolerances, those of tests/test_gpu_loudness.py for the same reason - f64 arithmetic on both sides, only pow and log10 differ, by
ulps of a double.  L_k: 2e-5 LU.  G_k: ln(10) / 20 * 2e-5 = 2.4e-6 relative, what 2e-5 LU means for 10^(d / 20).  y: at most 1
float32 ulp - the one rounding to float32 can fall on either side.  The precondition of all three, asserted on the inputs before the
GPU is asked anything: no block within 1e-4 LU of a gate, so a rounding difference cannot flip a block behind a tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conan_amd import _lib
from conan_amd.engine import StreamingVoiceConversionEngine
from tests import level_ref as V
from tests import loudness_ref as LR
from tests.test_gpu_loudness import _ulps
from tests.wav_helpers import _profiled, _ref, _sig, ctx  # noqa: F401  (ctx: module fixture)

pytestmark = pytest.mark.gpu

U, FS = V.U, V.FS
LUFS_TOL = 2e-5
GAIN_RTOL = 2.4e-6
PAD = 37
VARIANTS = {"default": {}, "caps": dict(max_boost_db=6.0), "window5": dict(window_blocks=5), "no_peak_limit": dict(peak_limit=False),
            "clip": dict(clip=True), "boost40_gain-6": dict(max_boost_db=40.0, initial_gain_db=-6.0)}
CFG = dict(target=-22.0, max_boost_db=30.0, max_cut_db=40.0, initial_gain_db=-3.0, window_blocks=30, peak_limit=True, clip=True)


@functools.lru_cache(maxsize=None)
def _cases():
    """[(x, K-weighted x)] of level_ref's six cases, read-only, computed once."""
    out = []
    for n, seed in V.CASES:
        x = V.sig(n, seed)
        yk = LR.k_filter(x, FS)
        x.flags.writeable = False
        yk.flags.writeable = False
        out.append((x, yk))
    return out


@functools.lru_cache(maxsize=None)
def _want(i, variant):
    x, yk = _cases()[i]
    r = V.level(x, yk=yk, **VARIANTS[variant])
    assert r["margin"] >= 1e-4, (i, variant, r["margin"])
    return r


def _pack(rows):
    ld = max(len(x) for x in rows) + PAD
    buf = torch.zeros(len(rows), ld)
    for i, x in enumerate(rows):
        buf[i, :len(x)] = torch.from_numpy(np.array(x))
    return buf.cuda()


def _check(got_y, got_tr, want, tag):
    K = len(want["trace"])
    tr = got_tr[:K].cpu().numpy()
    L, Lw = tr[:, 0], want["trace"][:, 0]
    fin = np.isfinite(Lw)
    print(tag, "max |dL|", np.abs(L[fin] - Lw[fin]).max(), "max rel dG", np.abs(tr[:, 1] / want["trace"][:, 1] - 1).max(), "y ulps", _ulps(got_y, want["y"]))
    assert np.array_equal(np.isfinite(L), fin) and np.array_equal(L[~fin], Lw[~fin]), tag
    assert np.abs(L[fin] - Lw[fin]).max() <= LUFS_TOL, tag
    assert np.abs(tr[:, 1] / want["trace"][:, 1] - 1).max() <= GAIN_RTOL, tag
    assert _ulps(got_y, want["y"]) <= 1, tag


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_level_against_the_restatement(ctx, variant):
    kw = VARIANTS[variant]
    cases = _cases()
    wants = [_want(i, variant) for i in range(len(cases))]
    if variant == "default":      # the signal does what level_ref.sig says: every branch of the law is taken
        w = wants[1]
        assert (w["trace"][:4, 0] == -np.inf).all() and np.isfinite(w["trace"][5:, 0]).all()      # blocks under the absolute gate, then readings
        assert w["trace"][6, 1] == 10.0 and abs(w["trace"][12, 1] - 1 / 0.9) < 1e-6               # the boost cap, then the peak limit
        assert np.abs(w["y"]).max() > 1.0                                                        # the spike passes at the old gain
    if variant == "clip":
        assert all(np.abs(w["y"]).max() == 1.0 for w in wants)
    single = []
    for i, (x, _) in enumerate(cases):      # one row per call
        y, tr = ctx.level(torch.from_numpy(np.array(x)), return_trace=True, **kw)
        _check(y.cpu().numpy(), tr, wants[i], (variant, "row", i))
        single.append((y, tr))
    for grp in ((0, 1, 2), (3, 4, 5)):      # three unequal rows in one call, strides beyond the longest row
        xb = _pack([cases[i][0] for i in grp])
        keep = xb.clone()
        lens = [len(cases[i][0]) for i in grp]
        yb = torch.full_like(xb, 7.0)
        _, tr = ctx.level(xb[:, :max(lens)], lengths=lens, return_trace=True, out=yb, **kw)
        assert torch.equal(xb, keep)
        for r, i in enumerate(grp):
            K = -(-lens[r] // U)
            assert bool((yb[r, lens[r]:] == 7.0).all())                                   # nothing past a row's length
            assert torch.equal(yb[r, :lens[r]], single[i][0])                             # a row does not depend on its batch
            assert torch.equal(tr[r, :K], single[i][1][:K]) and bool(torch.isnan(tr[r, K:]).all())
        _, tr2 = ctx.level(xb[:, :max(lens)], lengths=lens, return_trace=True, out=xb, **kw)      # in place, and a second run
        assert torch.equal(tr2.nan_to_num(9.0), tr.nan_to_num(9.0))
        for r in range(3):
            assert torch.equal(xb[r, :lens[r]], yb[r, :lens[r]]) and torch.equal(xb[r, lens[r]:], keep[r, lens[r]:])


def _dyn(B, N, seed, rate=FS):
    """[B, N] cuda rows at `rate`: level_ref.sig's envelope (quiet, speech level, silence, loud) over wav_helpers' tones, each row at
    its own level."""
    t = np.arange(N) / float(rate)
    env = np.where(t < 0.35, 1e-5, np.where(t < 1.2, 0.02, np.where(t < 1.5, 1e-5, 0.6)))
    x = _sig(B, N, rate, seed).cpu().numpy() * env * (0.5 ** np.arange(B))[:, None]
    if N > int(0.9 * rate):
        x[:, int(0.9 * rate)] = 0.9
    return torch.from_numpy(x.astype(np.float32)).cuda()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _utterance(eng, src, ref, pipelined, **start):
    """infer_wav's loop with the front-end's chunk rows kept (Streams.wav_chunk: the log-mel the step consumed, a continuous function
    of the samples the front-end read - the outputs alone pass through the Emformer's argmax) -> [wav, mel, codes, chunks]."""
    in_rate = start.get("in_rate")
    eng.start_wav(ref, **start)
    B, N = src.shape
    Li = eng._in_len(in_rate)
    last = (N - 1) // Li * Li
    outs, pos, fin = [], 0, False
    while True:
        if pos < last:
            w, m, c = eng.feed(src[:, pos:pos + Li], pipelined=pipelined)
            pos += Li
        else:
            w, m, c = eng.feed(src[:, pos:] if not fin else src[:, :0], final=True, pipelined=pipelined)
            pos, done, fin = N, fin and m.shape[1] == 0, True
            if done:
                break
        if m.shape[1]:
            outs.append((w, m, c, eng.st.wav_chunk(B).clone()))
    eng.st.join()
    return [torch.cat(t, 1) for t in zip(*outs)]


@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("B,arith", [(1, "auto"), (4, "f32"), (4, "limb")])
def test_streaming_equals_the_whole_signal_form(ctx, B, arith, pipelined):
    eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64, arith=arith)
    ref = _ref(B)
    for N in (U // 2, 6 * U, 2 * FS + 5):
        src = _dyn(B, N, 11 + N % 7)
        want = _utterance(eng, ctx.level(src, **CFG), ref, pipelined)
        got = _utterance(eng, src, ref, pipelined, level=CFG)
        assert _same(got, want), (N, B, arith, pipelined)
        assert _same(eng.infer_wav(src, ref, pipelined=pipelined, level=CFG), want[:3])
        if N > FS:
            plain = _utterance(eng, src, ref, pipelined)
            assert not torch.equal(plain[3], got[3])      # (the leveller changed what the front-end read)


@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("rate,fmt,preset", [(48000, None, "hann"), (8000, "ulaw", "kaiser_best")])
def test_streaming_at_an_input_rate_and_format(ctx, rate, fmt, preset, pipelined):
    """The front-end's samples per call vary here (the filter's look-ahead): these are the calls that straddle an update instant."""
    B = 2
    eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    ref = _ref(B)
    x = _dyn(B, 2 * rate + 5 * rate // 16000, 23, rate)
    src = ctx.convert_samples(x, "f32", fmt) if fmt else x
    dec = ctx.convert_samples(src, fmt, "f32") if fmt else x
    model = ctx.resample(dec, rate, preset=preset)
    want = _utterance(eng, ctx.level(model, **CFG), ref, pipelined)
    got = _utterance(eng, src, ref, pipelined, in_rate=rate, in_format=fmt, level=CFG, preset=preset)
    assert _same(got, want)
    _, trace = ctx.level(model, return_trace=True, **CFG)      # the meter's last reading is the whole-signal form's last trace row
    assert torch.equal(eng.st.input_level(eng.slots)[:, :2], trace[:, -1]) and bool(torch.isfinite(trace[:, -1]).all())
    assert _same(eng.infer_wav(src, ref, pipelined=pipelined, in_rate=rate, in_format=fmt, level=CFG, preset=preset), want[:3])
    plain = _utterance(eng, src, ref, pipelined, in_rate=rate, in_format=fmt, preset=preset)
    assert not torch.equal(plain[3], got[3])


@pytest.mark.parametrize("pipelined", [False, True])
def test_ragged_calls_mix_levelled_and_unlevelled_rows(ctx, pipelined):
    # (a fixed plan: the vocoder's launch shapes, and with them the last bits of its audio, otherwise follow a call's slot count)
    eng = StreamingVoiceConversionEngine(ctx, 3, max_ref_frames=64, flags=_lib.STREAMS_FIXED_PLAN)
    rates = [None, 48000, 8000, None, 22050]
    levels = [CFG, None, dict(CFG, clip=False, window_blocks=4096), None, True]
    starts = [0, 0, 2, 3, 5]
    srcs = [_dyn(1, int(1.3 * (r or FS)) + 17 * u, 40 + u, r or FS)[0] for u, r in enumerate(rates)]
    ref = _ref(len(srcs))
    outs = eng.infer_wav_staggered(srcs, starts, ref, pipelined=pipelined, in_rates=rates, level=levels)
    for u in range(len(srcs)):
        solo = eng.infer_wav_staggered([srcs[u]], [0], ref[u:u + 1], pipelined=pipelined, in_rates=[rates[u]], level=[levels[u]])[0]
        assert _same(outs[u], solo), u
    # the meter of a levelled slot that joins two ticks late, beside an unlevelled one: the whole-signal trace, instant by instant
    x = _dyn(2, 8 * U + 77, 61)
    _, trace = ctx.level(x[1:], return_trace=True, **CFG)
    eng.open_slots([0], ref[:1])
    fn = eng.st.step_wav_ragged_async if pipelined else eng.st.step_wav_ragged
    for tick in range(9):
        if tick == 2:
            eng.open_slots([2], ref[1:2], level=CFG)
        live = [0, 2] if tick >= 2 else [0]
        a0, a1 = tick * U, (tick - 2) * U
        rows = torch.zeros(len(live), U, device="cuda")
        n0 = min(U, x.shape[1] - a0)
        rows[0, :n0] = x[0, a0:a0 + n0]
        samples, final = [n0], [n0 < U]
        if tick >= 2:
            rows[1] = x[1, a1:a1 + U]
            samples, final = samples + [U], final + [False]
        fn(live, rows, samples, final)
        if tick >= 2:
            assert torch.equal(eng.st.input_level([2])[0, :2], trace[0, tick - 2]), tick
    assert bool(torch.isfinite(trace[0, :, 0]).any())


def _feed_calls(N):
    """(start, stop, final) of infer_wav's calls over N samples, then the drain calls."""
    last = (N - 1) // U * U
    return [(p, p + U, False) for p in range(0, last, U)] + [(last, N, True)]


def test_input_level_follows_the_trace(ctx):
    st = ctx.streams(2, max_frames=4, max_ref_frames=64)
    slots = [1, 0]
    src = _dyn(2, 2 * FS + 5, 5)
    _, trace = ctx.level(src, return_trace=True, **CFG)
    st.reset(slots, which=15)
    st.set_reference(slots, _ref(2))
    st.set_input_level(slots, CFG)
    got = st.input_level(slots).cpu().numpy()
    g0 = 10.0 ** (-3.0 / 20.0)
    assert np.array_equal(got, np.array([[-np.inf, g0, 0.0, 0.0]] * 2))
    ax = src.abs().double().cpu().numpy()
    for k, (a, b, fin) in enumerate(_feed_calls(src.shape[1])):
        st.step_wav(slots, src[:, a:b], final=fin)
        lv = st.input_level(slots)
        assert torch.equal(lv[:, :2].nan_to_num(neginf=-1e9), trace[:, k].nan_to_num(neginf=-1e9)), k
        lv = lv.cpu().numpy()
        uk = k * U
        assert np.array_equal(lv[:, 2], ax[:, :uk].max(1) if uk else np.zeros(2)), k
        assert (lv[:, 3] == sum(1 for _, hi in V.blocks(uk) if hi <= uk)).all(), k
    st.close()


def test_launch_accounting(ctx):
    """One level_stream_kernel per call that gives a levelled row samples, none on drain calls, none ever - and no resampler launch -
    on a stream-set that never enabled a leveller."""
    src = _dyn(2, 3 * U + 100, 9)
    ref = _ref(2)
    names = {}
    for mode in ("never", "level", "mixed"):
        st = ctx.streams(2, max_frames=4, max_ref_frames=64)
        slots = [0, 1]
        st.reset(slots, which=15)
        st.set_reference(slots, ref)
        if mode == "level":
            st.set_input_level(slots, CFG)
        if mode == "mixed":
            st.set_input_level([1], CFG)
        seen = []
        calls = _feed_calls(src.shape[1])
        for a, b, fin in calls + [(0, 0, True)] * 3:
            if mode == "mixed":
                n = [b - a, b - a]
                (emit, *_), ks = _profiled(st, lambda: st.step_wav_ragged(slots, src[:, a:b] if b > a else src[:, :1], n, [fin, fin]))
                emit = max(emit)
            else:
                (emit, *_), ks = _profiled(st, lambda: st.step_wav(slots, src[:, a:b], final=fin))
            want = 1 if (b > a and mode != "never") else 0
            assert ks.get("level_stream_kernel", 0) == want, (mode, a, b, ks)
            assert ks.get("resample_stream_kernel", 0) == 0, (mode, a, b, ks)      # (no rate, no format: the leveller reads the caller's rows)
            seen.append(ks)
            if b == a and emit == 0:
                break
        names[mode] = seen
        st.close()
    extra = {"level_stream_kernel"}
    assert len(names["never"]) == len(names["level"])
    for a, b in zip(names["never"], names["level"]):      # the unlevelled set's launches are the levelled set's minus the one
        assert not (set(a) & extra) and a == {k: v for k, v in b.items() if k not in extra}


def test_errors_are_atomic_and_a_reset_keeps_the_cfg(ctx):
    eng = StreamingVoiceConversionEngine(ctx, 2, max_ref_frames=64)
    st, lib = eng.st, ctx.lib
    src = _dyn(2, 5 * U + 9, 3)
    ref = _ref(2)
    first = eng.infer_wav(src, ref, pipelined=False, level=CFG)
    # a second utterance on the slots: the reset cleared the meter and kept the cfg
    st.reset(eng.slots, which=15)
    st.set_reference(eng.slots, ref)
    g0 = 10.0 ** (-3.0 / 20.0)
    assert np.array_equal(st.input_level(eng.slots).cpu().numpy(), np.array([[-np.inf, g0, 0.0, 0.0]] * 2))
    outs = []
    for a, b, fin in _feed_calls(src.shape[1]) + [(0, 0, True)] * 4:
        w, m, c = eng.feed(src[:, a:b], final=fin)
        if m.shape[1]:
            outs.append((w, m, c))
        elif b == a:
            break
        if a == U:      # mid-utterance: the setters refuse, nothing changes
            slots = (C.c_int32 * 2)(0, 1)
            other = _lib.level_cfg(target=-30.0)
            assert lib.conan_streams_set_input_level(st.h, slots, 2, C.byref(other)) == _lib.ERR_STATE
            off = _lib.LevelCfg()
            assert lib.conan_streams_set_input_level(st.h, slots, 2, C.byref(off)) == _lib.ERR_STATE
    again = [torch.cat(t, 1) for t in zip(*outs)]
    assert _same(first, again)
    # bad cfgs and slot lists at the start of an utterance: refused before anything changes
    st.reset(eng.slots, which=15)
    st.set_reference(eng.slots, ref)
    two = (C.c_int32 * 2)(0, 1)
    for bad in (dict(window_blocks=0), dict(window_blocks=4097), dict(max_boost_db=-1.0), dict(max_cut_db=float("nan")), dict(target=float("inf")),
                dict(initial_gain_db=float("inf"))):
        assert lib.conan_streams_set_input_level(st.h, two, 2, C.byref(_lib.level_cfg(**bad))) == _lib.ERR_INVALID, bad
    c = _lib.level_cfg()
    c.reserved[2] = 1
    assert lib.conan_streams_set_input_level(st.h, two, 2, C.byref(c)) == _lib.ERR_INVALID
    c = _lib.level_cfg()
    c.clip = 2
    assert lib.conan_streams_set_input_level(st.h, two, 2, C.byref(c)) == _lib.ERR_INVALID
    assert lib.conan_streams_set_input_level(st.h, (C.c_int32 * 2)(0, 7), 2, C.byref(_lib.level_cfg(target=-30.0))) == _lib.ERR_INVALID
    assert lib.conan_streams_set_input_level(st.h, (C.c_int32 * 2)(1, 1), 2, C.byref(_lib.level_cfg(target=-30.0))) == _lib.ERR_INVALID
    # the cfg in force is still CFG on both slots: feeding without touching the level gives the first result again
    outs = []
    for a, b, fin in _feed_calls(src.shape[1]) + [(0, 0, True)] * 4:
        w, m, c = eng.feed(src[:, a:b], final=fin)
        if m.shape[1]:
            outs.append((w, m, c))
        elif b == a:
            break
    assert _same(first, [torch.cat(t, 1) for t in zip(*outs)])
    # a slot without a leveller has no reading
    st.reset(eng.slots, which=15)
    st.set_input_level([1], None)
    out = torch.empty(2, 4, dtype=torch.float64, device="cuda")
    assert lib.conan_streams_input_level(st.h, two, 2, C.c_void_p(out.data_ptr()), None) == _lib.ERR_STATE
    # conan_step_wav's one configuration per call
    st.set_reference(eng.slots, ref)
    with pytest.raises(_lib.ConanError) as e:
        st.step_wav(eng.slots, src[:, :U])
    assert e.value.code == _lib.ERR_INVALID and "input level" in str(e.value)
    # the Python setter: no keywords is the default leveller, only None is off, and input_levels holds every keyword
    st.reset(eng.slots, which=15)
    st.set_input_level([1])
    defaults = dict(target=-22.0, max_boost_db=20.0, max_cut_db=40.0, initial_gain_db=0.0, window_blocks=4096, peak_limit=True, clip=False)
    assert st.input_levels[1] == defaults and st.input_level([1]).cpu().numpy()[0].tolist() == [-np.inf, 1.0, 0.0, 0.0]
    st.set_input_level([1], {"max_boost_db": 6.0}, clip=True)
    assert st.input_levels[1] == dict(defaults, max_boost_db=6.0, clip=True)
    with pytest.raises(ValueError):
        st.set_input_level([1], None, clip=True)
    assert 1 in st.input_levels
    st.set_input_level([1], None)
    assert 1 not in st.input_levels and 0 in st.input_levels


def test_a_levelled_stream_moves_between_slots_and_stream_sets(ctx):
    """Export after 9 calls, import into another slot and into a fresh stream-set, continue: audio and input_level are those of the
    uninterrupted run, bit for bit; the record shows the cfg; a record without a leveller turns a levelled slot's off."""
    src = _dyn(1, 2 * FS + 5, 31)
    ref = _ref(1)
    calls = _feed_calls(src.shape[1]) + [(0, 0, True)] * 8
    cut = 9

    def feed(st, slot, ks, outs, levels):
        for k in ks:
            a, b, fin = calls[k]
            emit, c, m, w = st.step_wav([slot], src[:, a:b], final=fin)
            if emit:
                outs.append((w.clone(), m.clone(), c[:, :emit].clone()))
            levels.append(st.input_level([slot]).clone())
            if b == a and emit == 0:
                break
        return outs, levels

    A = ctx.streams(2, max_frames=4, max_ref_frames=64)
    A.reset([0, 1], which=15)
    A.set_reference([0], ref)
    A.set_input_level([0], CFG)
    whole, whole_lv = feed(A, 0, range(len(calls)), [], [])
    A.reset([0], which=15)
    A.set_reference([0], ref)
    head, head_lv = feed(A, 0, range(cut), [], [])
    snap = A.export_slots([0])
    info = snap.info(0)
    assert info["level"] == dict(CFG, target=-22.0) and A.export_slots([1]).info(0)["level"] is None
    assert info["bytes"] > A.export_slots([1]).info(0)["bytes"]
    B = ctx.streams(2, max_frames=4, max_ref_frames=64)      # a fresh stream-set: the import allocates the leveller's state
    B.reset([0, 1], which=15)
    assert B.layout_id == A.layout_id and B.snapshot_bytes == A.snapshot_bytes
    before = B.state_bytes
    B.import_slots([1], snap)
    assert B.state_bytes - before == 2 * 66464 and B.input_levels == {1: info["level"]}
    A.import_slots([1], snap)                                # another slot of the same set, the source still mid-utterance
    for st, slot in ((A, 1), (B, 1), (A, 0)):
        outs, lv = feed(st, slot, range(cut, len(calls)), list(head), list(head_lv))
        assert _same([torch.cat(t, 1) for t in zip(*outs)], [torch.cat(t, 1) for t in zip(*whole)]), slot
        assert len(lv) == len(whole_lv) and all(torch.equal(x.nan_to_num(neginf=-1e9), y.nan_to_num(neginf=-1e9)) for x, y in zip(lv, whole_lv))
    # a record without a leveller into a levelled slot: off
    B.reset([0, 1], which=15)
    plain = B.export_slots([0])
    B.import_slots([1], plain)
    assert B.input_levels == {}
    with pytest.raises(_lib.ConanError) as e:
        B.input_level([1])
    assert e.value.code == _lib.ERR_STATE
    A.close()
    B.close()


def test_engine_level_true_changes_a_quiet_input_and_leaves_the_neighbour_alone(ctx):
    eng = StreamingVoiceConversionEngine(ctx, 2, max_ref_frames=64)
    ref = _ref(2)
    quiet = 0.02 * _sig(2, 2 * FS, FS, 77)

    def run(levels):
        eng.open_slots(eng.slots, ref, level=levels)
        outs = [[], []]
        for a, b, fin in _feed_calls(quiet.shape[1]) + [(0, 0, True)] * 4:
            res = eng.feed_ragged(eng.slots, quiet[:, a:b] if b > a else quiet[:, :1], [b - a] * 2, [fin] * 2)
            for i, (w, m, c) in enumerate(res):
                if m.shape[0]:
                    outs[i].append((w.clone(), m.clone(), c.clone()))
            if b == a and not any(m.shape[0] for _, m, _ in res):
                break
        return [[torch.cat(t, 0) for t in zip(*o)] for o in outs]

    plain = run(None)
    mixed = run([True, None])
    assert _same(mixed[1], plain[1])                      # the unlevelled neighbour: bit-identical
    lv = eng.st.input_level([0]).cpu().numpy()[0]
    assert np.isfinite(lv[0]) and lv[1] > 2.0             # a quiet line is boosted
    # start_wav / feed, the documented path: what the front-end read (its chunk rows) moves with level=True
    chunks = {}
    for level in (True, None):
        eng.start_wav(ref, level=level)
        for k in range(12):
            _, m, _ = eng.feed(quiet[:, k * U:(k + 1) * U])
        assert m.shape[1] > 0
        chunks[level] = eng.st.wav_chunk(2).clone()
    assert not torch.equal(chunks[True], chunks[None])
    assert eng.st.input_levels == {}
    with pytest.raises(ValueError):
        eng.start_wav(ref, level=[True, None])
