"""Input loss concealment on the GPU (conan_streams_set_conceal, conan_streams_conceal, conan_streams_conceal_state, conan_conceal;
include/conan_hip.h, conan_conceal_cfg), bit for bit against tests/conceal_ref.py: the whole-signal form, the streaming form in
chunks, in all four sample formats and mixed in one call; received samples, rows of other slots, rows without samples and the bytes
behind a row keep their bytes; the state's hand-over, its query and its restart; a stream-set that never enables the feature keeps
its memory and its launches; and the engine end to end.  Nothing here has a tolerance: the law is integer arithmetic and single
correctly rounded f32 operations in a fixed order.

The shapes are the smallest that reach every branch: the tiny configuration on rows of a few hundred samples (chunks of 64), and
the 8 / 16 / 48 kHz defaults on two 80 ms chunks and a short third one.  Every signal loses its first packet (a loss at position 0),
packet 3 and the whole second chunk (a run across a call boundary, an all-lost chunk, a run beyond hold + fall) and its last, partly
filled packet (a loss up to the last sample, in a short final row)."""
import functools

import numpy as np
import pytest
import torch

from conan_amd import _lib
from conan_amd.engine import StreamingVoiceConversionEngine
from tests import conceal_ref as R
from tests import sample_format_ref as SF
from tests.test_gpu_f0 import _launches, _ref
from tests.test_gpu_pitch import full  # noqa: F401  (module fixture: the small synthetic full model)

pytestmark = pytest.mark.gpu

MAX_SLOTS = 6
FMTS = ("f32", "s16", "ulaw", "alaw")
TINY = dict(packet=16, lag_min=4, lag_max=24, window=32, hold=8, fall=16, fade=8)
CFGS = {"tiny": TINY, "tiny4": dict(TINY, packet=4), "8k": R.defaults(8000), "16k": R.defaults(16000), "48k": R.defaults(48000)}
STATE_BYTES = 32 + 4 * 1024 + 4 * 2048
ROW_BYTES = 56      # one table row of the kernel (streams.h: four tables of max_slots rows)
PAD = 0xAB


def _length(name):
    chunk = 4 * CFGS[name]["packet"]
    return 6 * chunk + 5 if name.startswith("tiny") else 2 * chunk + chunk // 2 + 3      # (the last packet is partly filled)


def _flags(name, row):
    cfg = CFGS[name]
    npk = -(-_length(name) // cfg["packet"])
    f = np.zeros(npk, dtype=np.int32)
    f[[0, 3, 4, 5, 6, 7, npk - 1]] = 1
    if name.startswith("tiny"):      # more room: single packets, pairs, and - with packets shorter than the fade - losses inside fades
        f[10:npk - 1] = np.random.default_rng(17 + row).integers(0, 2, npk - 11)
        f[[12, 13, 14]] = (1, 0, 1)
    if row:
        f[1:3] = (1, 0)
    return f


@functools.lru_cache(maxsize=None)
def _signal(name, fmt, row=0):
    """(codes [N] of fmt, flags): a periodic signal with a little noise, the period inside the lag range."""
    cfg, N = CFGS[name], _length(name)
    rng = np.random.default_rng(len(name) + 10 * row)
    period = (cfg["lag_min"] + 2 * cfg["lag_max"]) // 3 + row
    cell = rng.integers(-9000, 9000, size=period)
    x = (np.tile(cell, N // period + 1)[:N] + rng.integers(-200, 200, size=N)).astype(np.float32) / np.float32(32768)
    return SF.encode(x, fmt), _flags(name, row)


@functools.lru_cache(maxsize=None)
def _want(name, fmt, row=0):
    """The law on the whole signal -> (repaired codes, mask of the written samples): computed once, shared by the tests."""
    x, fl = _signal(name, fmt, row)
    out, written = R.Concealer(fmt, **CFGS[name]).apply(x, fl)
    assert written.any() and not written.all() and np.array_equal(out[~written], x[~written])
    return out, written


def _same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    return got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def _pack(rows, ld):
    """Rows (numpy, each in its own format's dtype) packed from the start of rows ld * 4 bytes apart; the bytes behind them are PAD."""
    buf = np.full((len(rows), ld * 4), PAD, dtype=np.uint8)
    for i, r in enumerate(rows):
        buf[i, :r.nbytes] = r.view(np.uint8)
    return torch.from_numpy(buf).cuda()


def _unpack(buf, rows):
    raw = buf.cpu().numpy()
    for i, r in enumerate(rows):
        assert (raw[i, r.nbytes:] == PAD).all(), "bytes behind a row's samples were written"
    return [raw[i, :r.nbytes].view(r.dtype).copy() for i, r in enumerate(rows)]


@pytest.fixture(scope="module")
def st(full):
    s = full.streams(MAX_SLOTS, 4, 64)
    for slot, fmt in enumerate(FMTS):
        if fmt != "f32":
            s.set_input_format([slot], fmt)
    yield s
    s.close()


def _fresh(st, slots, cfg):
    """The slots enabled from off: their states restart."""
    st.set_conceal(slots, None)
    st.set_conceal(slots, _lib.conceal_cfg(**cfg))


# ------------------------------------------------------------------------------------------------------------------ 1. whole signals

@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(CFGS))
def test_whole_signal_against_the_law(full, name, fmt):
    (x0, f0), (x1, f1) = _signal(name, fmt, 0), _signal(name, fmt, 1)
    keep = len(x1) - CFGS[name]["packet"] - 1      # row 1 is repaired over a prefix only: a row of its own length
    x = torch.from_numpy(np.stack([x0, x1])).cuda()
    lost = torch.from_numpy(np.stack([f0, f1])).cuda()
    got = full.conceal(x, lost, _lib.conceal_cfg(**CFGS[name]), fmt, lengths=[len(x0), keep])
    assert _same(got[0], _want(name, fmt, 0)[0])
    want1 = R.conceal(x1[:keep], f1, fmt, **CFGS[name])
    assert _same(got[1, :keep], want1) and _same(got[1, keep:], x1[keep:])
    assert _same(x, np.stack([x0, x1]))      # (the caller's tensor keeps its samples: Context.conceal packs a buffer of its own)
    # bool flags, one row, a 1-D signal
    assert _same(full.conceal(x[0], lost[0] != 0, dict(CFGS[name]), fmt), _want(name, fmt, 0)[0])


def test_the_defaults_of_a_rate(full):
    x, fl = _signal("16k", "f32")
    assert _same(full.conceal(torch.from_numpy(x).cuda(), torch.from_numpy(fl).cuda(), 16000), _want("16k", "f32")[0])


# ------------------------------------------------------------------------------------------------------------------ 2. streaming

@pytest.mark.parametrize("name", ["tiny", "8k", "16k", "48k"])
def test_chunks_equal_the_whole_signal_in_every_format_in_one_call(st, name):
    """Slots 0 .. 3 (f32, s16, mu-law, A-law) repair their signals chunk by chunk in the same calls; slot 4 has no concealment and
    keeps its bytes whatever its flags say; slot 5 has it and passes rows without samples."""
    cfg = CFGS[name]
    chunk = 4 * cfg["packet"]
    N = _length(name)
    _fresh(st, [0, 1, 2, 3, 5], cfg)
    assert st.conceal_cfg([0, 4, 5]) == [cfg, None, cfg]
    sig = [_signal(name, fmt) for fmt in FMTS]
    other = _signal(name, "f32", 1)[0]
    outs = [[] for _ in range(6)]
    for lo in range(0, N, chunk):
        hi = min(lo + chunk, N)
        rows = [x[lo:hi] for x, _ in sig] + [other[lo:hi], other[lo:hi]]
        fl = np.ones((6, 4), dtype=np.int32)
        for i, (_, f) in enumerate(sig):
            part = f[lo // cfg["packet"]:-(-hi // cfg["packet"])]
            fl[i, :len(part)] = part
        buf = _pack(rows, chunk + 1)      # (f32 rows fill chunk of the chunk + 1 words: a stride that is not the row's length)
        assert st.conceal(list(range(6)), buf, [hi - lo] * 5 + [0], torch.from_numpy(fl).cuda()) is buf
        for i, r in enumerate(_unpack(buf, rows)):
            outs[i].append(r)
    for i, fmt in enumerate(FMTS):
        assert _same(np.concatenate(outs[i]), _want(name, fmt)[0]), fmt
    assert _same(np.concatenate(outs[4]), other) and _same(np.concatenate(outs[5]), other)
    # ... which is what conan_conceal gives for the whole signal (f32; the whole-signal test holds the others to the same reference)
    x, f = sig[0]
    assert _same(st.ctx.conceal(torch.from_numpy(x).cuda(), torch.from_numpy(f).cuda(), dict(cfg)), np.concatenate(outs[0]))


def test_a_loss_inside_a_fade_across_short_rows(st):
    """Packets count from the start of each row, so a short row moves them: a row that ends in a lost packet, four received samples
    (half a fade), then a row that begins with a lost packet - the new run's search reads the faded samples."""
    _fresh(st, [0, 1, 2, 3], TINY)
    sig = [_signal("tiny", fmt)[0] for fmt in FMTS]
    cuts = [(0, 64, [0, 0, 0, 1]), (64, 68, [0]), (68, 100, [1, 0]), (100, 103, [0]), (103, 150, [0, 1, 1])]
    refs = [R.Concealer(fmt, **TINY) for fmt in FMTS]
    for lo, hi, fl in cuts:
        rows = [x[lo:hi] for x in sig]
        buf = _pack(rows, 64)
        st.conceal([0, 1, 2, 3], buf, hi - lo, torch.tensor([fl] * 4, dtype=torch.int32).cuda())
        for got, ref, row, fmt in zip(_unpack(buf, rows), refs, rows, FMTS):
            assert _same(got, ref.apply(row, fl)[0]), (fmt, lo)
    assert all(r.mode == 1 and r.k == 31 for r in refs)      # (the last row ends inside a run)


def test_a_float32_tensor_is_repaired_in_place_and_bool_flags_count(st):
    _fresh(st, [0], TINY)
    x, fl = _signal("tiny", "f32")
    t = torch.from_numpy(x[None].copy()).cuda()
    assert st.conceal([0], t, len(x), torch.from_numpy(fl[None] != 0).cuda()) is t
    assert _same(t[0], _want("tiny", "f32")[0])


# ------------------------------------------------------------------------------------------------------------------ 3. the state

def _record(blob):
    raw = blob.cpu().numpy().tobytes()
    head = np.frombuffer(raw[:32], dtype=np.int32)
    k = int(np.frombuffer(raw[16:24], dtype=np.int64)[0])
    T = np.frombuffer(raw[32:32 + 4096], dtype=np.float32)
    hist = np.frombuffer(raw[32 + 4096:], dtype=np.float32)
    return dict(mode=int(head[0]), p=int(head[1]), j=int(head[2]), k=k), T, hist


@pytest.mark.parametrize("fmt", ["f32", "ulaw"])
def test_state_query_hand_over_and_reset(st, fmt):
    a, b = FMTS.index(fmt), 5
    st.set_input_format([b], fmt)
    x, fl = _signal("tiny", fmt)
    want = _want("tiny", fmt)[0]
    _fresh(st, [a], TINY)
    st.set_conceal([b], None)
    assert int(st.lib.conan_conceal_state_bytes()) == STATE_BYTES
    blob = st.conceal_state([a])
    assert blob.shape == (1, STATE_BYTES) and not blob.any()      # a slot about to restart reports the zero state
    with pytest.raises(_lib.ConanError) as e:
        st.conceal_state([b])
    assert e.value.code == _lib.ERR_STATE
    # rows of 80 samples: the first ends inside the run of packets 3 .. 7
    ref = R.Concealer(fmt, **TINY)
    rows = [x[0:80], x[80:240], x[240:]]
    flags = [fl[0:5], fl[5:15], fl[15:]]
    ld = 400

    def repair(slot, row, f):
        buf = _pack([row], ld)
        st.conceal([slot], buf, len(row), torch.from_numpy(f[None].copy()).cuda())
        return _unpack(buf, [row])[0]

    got = [repair(a, rows[0], flags[0])]
    ref.apply(rows[0], flags[0])
    head, T, hist = _record(st.conceal_state([a]))
    assert head == dict(mode=1, p=ref.p, j=ref.j, k=ref.k) and ref.k == 32      # (j: the fade behind packet 0 ran out; a run leaves it alone)
    assert _same(T[:ref.p], ref.T) and _same(hist[-len(ref.hist):], ref.hist)
    # the hand-over: the record seeds another slot, which continues bit for bit (two rows: the seed's row stride is wider than a record)
    seed = torch.zeros(2, STATE_BYTES + 64, dtype=torch.uint8, device="cuda")
    seed[1, :STATE_BYTES] = st.conceal_state([a])[0]
    st.set_conceal([b], _lib.conceal_cfg(**TINY), seed=seed[1:])
    assert torch.equal(st.conceal_state([b])[0], seed[1, :STATE_BYTES])
    got.append(repair(b, rows[1], flags[1]))
    # ... and back, through a setter call that changes nothing else: an enabled slot keeps its state without a seed
    st.set_conceal([a], _lib.conceal_cfg(**TINY), seed=st.conceal_state([b]))
    st.set_conceal([a], _lib.conceal_cfg(**TINY))
    got.append(repair(a, rows[2], flags[2]))
    assert _same(np.concatenate(got), want)
    # a reset of the front-end restarts the state (the setting stays); a reset of the models alone does not
    st.reset([a], which=7)
    assert st.conceal_state([a]).any()
    st.reset([a], which=8)
    assert not st.conceal_state([a]).any() and st.conceal_cfg([a]) == [TINY]
    assert _same(repair(a, x, fl), want)
    st.set_input_format([b], "f32")
    st.set_conceal([b], None)


def test_refused_calls_change_nothing(st):
    _fresh(st, [0], TINY)
    x, fl = _signal("tiny", "f32")
    t = torch.from_numpy(x[None].copy()).cuda()
    lost = torch.from_numpy(fl[None].copy()).cuda()
    for bad in (lambda: st.conceal([0], t, len(x) + 1, lost),               # more samples than the row stride holds
                lambda: st.conceal([0], t, len(x), lost[:, :-1]),           # fewer flags than packets
                lambda: st.conceal([0, 0], t.repeat(2, 1), len(x), lost.repeat(2, 1)),
                lambda: st.conceal([0], t, -1, lost),
                lambda: st.set_conceal([0], _lib.conceal_cfg(**dict(TINY, lag_max=2000))),
                lambda: st.set_conceal([MAX_SLOTS], _lib.conceal_cfg(**TINY))):
        with pytest.raises(_lib.ConanError) as e:
            bad()
        assert e.value.code == _lib.ERR_INVALID
    assert _same(t[0], x) and not st.conceal_state([0]).any() and st.conceal_cfg([0]) == [TINY]
    st.conceal([0], t, len(x), lost)
    assert _same(t[0], _want("tiny", "f32")[0])


def test_a_context_without_the_front_end_is_refused(full):
    from conan_amd import configs, synth
    from conan_amd.runtime import Context
    vhp = configs.hifigan_hparams(True)
    c = Context(None, vhp, 0, emformer=False, conan=False)
    c.load_state_dict("hifigan", synth.hifigan_state_dict(vhp, 0))
    c.finalize()
    s = c.streams(2, 4, 64)
    with pytest.raises(_lib.ConanError) as e:
        s.set_conceal([0], _lib.conceal_cfg(16000))
    assert e.value.code == _lib.ERR_STATE
    s.close()
    c.close()


# ------------------------------------------------------------------------------------------------------------------ 4. memory and launches

def _calls(s, slots, wav, lost=None):
    """infer_wav's calls over wav [n, N] with the flags of the whole signal -> (the concatenated wav, calls that took samples)."""
    L, outs, took = 4 * 320, [], 0
    n, N = wav.shape
    last = (N - 1) // L * L
    pieces = [(p, p + L, False) for p in range(0, last, L)] + [(last, N, True)]
    while True:
        if pieces:
            lo, hi, fin = pieces.pop(0)
            fl = None if lost is None else lost[:, lo // 320:-(-hi // 320)]
            e, _, _, w = s.step_wav(slots, wav[:, lo:hi].clone(), final=fin, lost=fl)
            took += 1
        else:
            e, _, _, w = s.step_wav(slots, wav[:, :0], final=True)
            if e == 0:
                break
        if e:
            outs.append(w.clone())
    return torch.cat(outs, 1), took


def test_a_stream_set_that_never_enables_it_keeps_its_memory_and_its_launches(full):
    slots = [0, 1, 2]
    N = 2 * 1280 + 500
    wav = torch.from_numpy((0.1 * np.random.default_rng(3).standard_normal((3, N))).astype(np.float32)).cuda()
    lost = torch.zeros(3, -(-N // 320), dtype=torch.int32, device="cuda")
    lost[:, [2, 5, 6]] = 1
    a, b = full.streams(MAX_SLOTS, 4, 64), full.streams(MAX_SLOTS, 4, 64)
    never = b.state_bytes
    assert a.state_bytes == never
    a.set_conceal([4], None)      # turning off what was never on: nothing is allocated
    assert a.state_bytes == never
    a.set_conceal([1], True)      # the model rate's defaults
    assert a.state_bytes == never + MAX_SLOTS * STATE_BYTES + 4 * MAX_SLOTS * ROW_BYTES
    assert a.conceal_cfg([1]) == [R.defaults(16000)]
    for s in (a, b):
        s.reset(slots, which=15)
        s.set_reference(slots, _ref(3))
    (wa, took), la = _launches(a, lambda: _calls(a, slots, wav, lost))
    (wb, _), lb = _launches(b, lambda: _calls(b, slots, wav, lost))      # (the flags of a stream-set without the feature repair nothing)
    b.reset(slots, which=15)
    b.set_reference(slots, _ref(3))
    (wc, _), lc = _launches(b, lambda: _calls(b, slots, wav))
    assert torch.equal(wb, wc) and lb == lc and "conceal_kernel" not in lb
    # the slots without the feature keep their bits; the repaired one is the run over the repaired signal
    assert torch.equal(wa[0], wb[0]) and torch.equal(wa[2], wb[2]) and not torch.equal(wa[1], wb[1])
    fixed = wav.clone()
    fixed[1] = full.conceal(wav[1], lost[1], 16000)
    b.reset(slots, which=15)
    b.set_reference(slots, _ref(3))
    assert torch.equal(_calls(b, slots, fixed)[0], wa)
    # one launch per call that took samples, in front of the step, and the step's own launches are the ones it ran before
    assert la.pop("conceal_kernel") == took and la == lb, (la, lb)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------------------------ 5. the engine

@pytest.mark.parametrize("form", ["f32", "s16", "in_8k"])
def test_engine_infer_wav_equals_the_repaired_signal(full, form):
    n = 2
    rate = 8000 if form == "in_8k" else 16000
    pk = rate // 50
    N = 2 * 4 * pk + 3 * pk + 7
    rng = np.random.default_rng(9)
    src = (0.2 * np.sin(2 * np.pi * 180.0 * np.arange(N) / rate) + 0.01 * rng.standard_normal((n, N))).astype(np.float32)
    fmt = "s16" if form == "s16" else "f32"
    src = torch.from_numpy(SF.encode(src, fmt)).cuda()
    lost = torch.zeros(n, -(-N // pk), dtype=torch.int32, device="cuda")
    lost[0, [0, 3, 4, 9, 11]] = 1
    lost[1, [1, 5, 6, 7, 8]] = 1
    kw = dict(in_format=None if fmt == "f32" else fmt, in_rate=None if rate == 16000 else rate)
    eng = StreamingVoiceConversionEngine(full, n, max_ref_frames=64)
    fixed = full.conceal(src, lost, rate, fmt)
    assert not torch.equal(fixed, src)
    want = eng.infer_wav(fixed, _ref(n), pipelined=False, **kw)
    before = src.clone()
    for pipelined, conceal in ((False, True), (True, dict(R.defaults(rate)))):
        got = eng.infer_wav(src, _ref(n), pipelined=pipelined, conceal=conceal, lost=lost, **kw)
        torch.cuda.synchronize()
        assert all(torch.equal(g, w) for g, w in zip(got, want)), (form, pipelined)
    assert torch.equal(src, before)      # (the engine repairs a copy of each chunk)
    # the slots keep the setting; without flags nothing is repaired
    assert eng.st.conceal_cfg(eng.slots) == [R.defaults(rate)] * n
    plain = eng.infer_wav(src, _ref(n), pipelined=False, conceal=True, **kw)
    off = eng.infer_wav(src, _ref(n), pipelined=False, **kw)
    assert all(torch.equal(g, w) for g, w in zip(plain, off)) and eng.st.conceal_cfg(eng.slots) == [None] * n


def test_engine_staggered_utterances(full):
    pk, L = 320, 1280
    rng = np.random.default_rng(4)
    lens = [2 * L + 400, L + 900, 3 * L]
    srcs = [torch.from_numpy((0.1 * rng.standard_normal(N)).astype(np.float32)).cuda() for N in lens]
    losts = [torch.zeros(-(-N // pk), dtype=torch.int32, device="cuda") for N in lens]
    losts[0][[0, 4, 5]] = 1
    losts[2][[2, 3, 4, 5, 6, 7, 11]] = 1
    eng = StreamingVoiceConversionEngine(full, 2, max_ref_frames=64)
    fixed = [srcs[0].clone(), srcs[1], full.conceal(srcs[2], losts[2], 16000)]
    fixed[0] = full.conceal(srcs[0], losts[0], 16000)
    want = eng.infer_wav_staggered(fixed, [0, 1, 2], _ref(3), pipelined=False)
    got = eng.infer_wav_staggered(srcs, [0, 1, 2], _ref(3), pipelined=False, conceal=[True, None, True], lost=[losts[0], None, losts[2]])
    for u in range(3):
        assert all(torch.equal(g, w) for g, w in zip(got[u], want[u])), u
