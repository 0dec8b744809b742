"""Per-slot sample formats (conan_streams_set_input_format / _output_format, conan_convert_samples) on the GPU: the whole-signal
converter against the numpy restatement of the header's rules on every code and every 16-bit value, streaming input in a format
bit-identical to the same engine fed the decoded floats, streaming output in a format byte-identical to conan_convert_samples of the
float engine's rows, the telephony case end to end, launch accounting, atomic errors and persistence across resets.  Every comparison
is exact: decoding is exact, and encoding is one rounding that both sides apply to the same floats."""
import ctypes as C

import numpy as np
import pytest
import torch

from conan_amd import _lib
from conan_amd.engine import StreamingVoiceConversionEngine
from conan_amd.runtime import mel_cfg
from tests import sample_format_ref as sf
from tests.conftest import ARITHS
from tests.test_out_rate_cpu import out_filter, schedule
from tests.wav_helpers import (HOP, L, SEG, SENT, _equal, _lin, _mel, _profiled, _ref, _run_manual, _sig, _voc_run_bytes,  # noqa: F401
                               ctx)  # (ctx: module fixture)

pytestmark = pytest.mark.gpu

FIXED = _lib.STREAMS_FIXED_PLAN
RS, RO = "resample_stream_kernel", "resample_out_kernel"
FORMATS = ("s16", "ulaw", "alaw")
BYTES = sf.BYTES


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _all_codes(fmt):
    return np.arange(-32768, 32768).astype(np.int16) if fmt == "s16" else np.arange(256, dtype=np.uint8)


def _coded(B, N, rate, seed, fmt):
    """A test signal at `rate` as the codes of `fmt` and as the floats they decode to (both by the restatement), on the GPU."""
    codes = sf.encode(_sig(B, N, rate, seed).cpu().numpy(), fmt)
    return _cuda(codes), _cuda(sf.decode(codes, fmt))


# ---- 1. conan_convert_samples, exhaustively
@pytest.mark.parametrize("fmt", FORMATS)
def test_convert_decodes_every_code(ctx, fmt):
    codes = _all_codes(fmt)
    got = ctx.convert_samples(_cuda(codes), fmt, "f32")
    assert got.dtype == torch.float32 and torch.equal(got, _cuda(sf.decode(codes, fmt)))
    # rows: the same codes as [n, N] with N * bytes no multiple of four
    rows = codes[:255 * (len(codes) // 255)].reshape(-1, 255)
    assert torch.equal(ctx.convert_samples(_cuda(rows), fmt, "f32"), _cuda(sf.decode(rows, fmt)))


@pytest.mark.parametrize("fmt", FORMATS)
def test_convert_encodes_every_value_and_the_ties(ctx, fmt):
    x = np.concatenate([np.arange(-32768, 32768).astype(np.float32) / np.float32(32768.0), sf.TIES])
    got = ctx.convert_samples(_cuda(x), "f32", fmt)
    assert got.dtype == _cuda(sf.encode(x[:1], fmt)).dtype and torch.equal(got, _cuda(sf.encode(x, fmt)))
    # values between the 16-bit grid points, and far outside the range
    rng = np.random.default_rng(7)
    y = np.concatenate([rng.uniform(-1.2, 1.2, 50001), rng.standard_normal(9999) * 1e-3, [1e9, -1e9, 3.0e38, -3.0e38]]).astype(np.float32)
    assert torch.equal(ctx.convert_samples(_cuda(y), "f32", fmt), _cuda(sf.encode(y, fmt)))


def test_convert_any_format_to_any(ctx):
    x = _sig(3, 1237, 16000, 5)
    assert torch.equal(ctx.convert_samples(x, "f32", "f32"), x)
    for src in FORMATS:
        codes = _all_codes(src)
        for dst in FORMATS:
            assert torch.equal(ctx.convert_samples(_cuda(codes), src, dst), _cuda(sf.convert(codes, src, dst))), (src, dst)
    with pytest.raises(ValueError):
        ctx.convert_samples(x, "s16", "f32")              # float samples are not int16 codes
    with pytest.raises(ValueError):
        ctx.convert_samples(x, "f32", "s24")


@pytest.mark.parametrize("dst", ("f32",) + FORMATS)
def test_convert_leaves_bytes_past_the_count_untouched(ctx, dst):
    for src in ("f32", "s16", "ulaw"):
        for N in (1, 3, 255, 257, 1281):
            x = _sig(3, N, 16000, N).cpu().numpy()
            xin = x if src == "f32" else sf.encode(x, src)
            want = sf.convert(xin, src, dst)
            ld = (N * BYTES[dst] + 3) // 4 + 3
            out = torch.full((3, ld * 4), SENT, dtype=torch.uint8, device="cuda")
            got = ctx.convert_samples(_cuda(xin), src, dst, out=out)
            torch.cuda.synchronize()
            assert torch.equal(got, _cuda(want)), (src, dst, N)
            assert bool((out[:, N * BYTES[dst]:] == SENT).all()), (src, dst, N)
            assert torch.equal(out[:, :N * BYTES[dst]], _cuda(want).view(torch.uint8).view(3, -1)), (src, dst, N)


# ---- 2. input side: the bytes with the format set = the decoded floats without one
@pytest.mark.parametrize("rate", [None, 8000, 48000])
@pytest.mark.parametrize("fmt", FORMATS)
def test_input_format_equals_decoded_floats(ctx, fmt, rate):
    Li = _lin(rate or 16000)
    for B in (1, 4):
        a = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
        b = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
        ref = _ref(B)
        for j, N in enumerate((Li // 2, 2 * Li + 1)):
            codes, floats = _coded(B, N, rate or 16000, 200 + j, fmt)
            for pipelined in (False, True):
                want = a.infer_wav(floats, ref, pipelined=pipelined, in_rate=rate)
                got = b.infer_wav(codes, ref, pipelined=pipelined, in_rate=rate, in_format=fmt)
                torch.cuda.synchronize()
                assert got[0].dtype == torch.float32 and _equal(got, want), (fmt, rate, B, N, pipelined)
        assert a.st.state_bytes == b.st.state_bytes


@pytest.mark.parametrize("pipelined", [False, True])
def test_staggered_mixed_formats_equal_decoded_floats(ctx, pipelined):
    """Four streams in the same calls: f32 / 16 kHz, s16 / 48 kHz, ulaw / 8 kHz, alaw / 16 kHz.  The comparison engine runs the same
    schedule (same rates, so the same launches) on the decoded floats."""
    fmts, rates = [None, "s16", "ulaw", "alaw"], [None, 48000, 8000, None]
    srcs_b, srcs_a = [], []
    for u, (f, r) in enumerate(zip(fmts, rates)):
        N = 2 * _lin(r or 16000) + 100 * u + 37
        if f is None:
            x = _sig(1, N, r or 16000, 300 + u)
            srcs_b.append(x[0])
            srcs_a.append(x[0])
        else:
            c, x = _coded(1, N, r or 16000, 300 + u, f)
            srcs_b.append(c[0])
            srcs_a.append(x[0])
    refs, starts = _ref(4, 6), [0, 0, 1, 2]
    a = StreamingVoiceConversionEngine(ctx, 4, max_ref_frames=64, flags=FIXED)
    b = StreamingVoiceConversionEngine(ctx, 4, max_ref_frames=64, flags=FIXED)
    want = a.infer_wav_staggered(srcs_a, starts, refs, pipelined=pipelined, in_rates=rates)
    got = b.infer_wav_staggered(srcs_b, starts, refs, pipelined=pipelined, in_rates=rates, in_formats=fmts)
    torch.cuda.synchronize()
    assert a.staggered_slots == b.staggered_slots
    for u in range(4):
        assert _equal(got[u], want[u]), (u, pipelined)


@pytest.mark.parametrize("pipelined", [False, True])
def test_staggered_all_rates_and_formats_equal_solo(ctx, pipelined):
    """Input rates and formats and output rates and formats in the same calls, long enough (9 to 11 input chunks each, five
    utterances on four slots, so one slot is reopened mid-run) that the ragged, input-resampler and output-resampler staging sets
    are all reused several times over.  Each utterance equals its run alone in the slot it was given, bit for bit."""
    ins = [(None, None), ("s16", 48000), ("ulaw", 8000), ("alaw", None), ("s16", 8000)]
    outs_ = [(None, None), ("s16", 48000), ("ulaw", 8000), (None, 8000), ("alaw", None)]
    ifmts, rates = [f for f, _ in ins], [r for _, r in ins]
    ofmts, orates = [f for f, _ in outs_], [r for _, r in outs_]
    srcs = []
    for u, (f, r) in enumerate(ins):
        N = (9 + u % 3) * _lin(r or 16000) + 100 * u + 37
        srcs.append(_sig(1, N, r or 16000, 800 + u)[0] if f is None else _coded(1, N, r or 16000, 800 + u, f)[0][0])
    U, refs, starts = 5, _ref(5, 8), [0, 0, 1, 2, 5]
    eng = StreamingVoiceConversionEngine(ctx, 4, max_ref_frames=64, flags=FIXED)
    outs = eng.infer_wav_staggered(srcs, starts, refs, pipelined=pipelined, in_rates=rates, out_rates=orates, in_formats=ifmts, out_formats=ofmts)
    torch.cuda.synchronize()
    used = eng.staggered_slots
    assert len(set(used)) < U, "no slot was reopened"
    solo = StreamingVoiceConversionEngine(ctx, 4, max_ref_frames=64, flags=FIXED)
    for u in range(U):
        solo.slots = [used[u]]
        w, m, c = solo.infer_wav(srcs[u][None], refs[u][None], pipelined=False, in_rate=rates[u], out_rate=orates[u], in_format=ifmts[u], out_format=ofmts[u])
        torch.cuda.synchronize()
        assert outs[u][0].dtype == sf_dtype(ofmts[u] or "f32")
        assert _equal(outs[u], (w[0], m[0], c[0])), (u, ins[u], outs_[u], pipelined)


# ---- 3. output side: every row = conan_convert_samples of the float engine's row
def _out_cases():
    out = []
    for fmt in FORMATS:
        for rate, preset in ((None, None), (11025, "kaiser_best"), (48000, "hann")):
            for arith in (ARITHS if (fmt, rate) == ("ulaw", 11025) else ARITHS[:1]):
                out.append((fmt, rate, preset, arith))
    return out


@pytest.mark.parametrize("fmt,rate,preset,arith", _out_cases())
def test_output_format_equals_converted_rows(ctx, fmt, rate, preset, arith):
    n, T = 3, 21
    mel = _mel(n, T, 400)
    slots = [2, 0, 1]
    ld = resample_len(rate, 4 * HOP) + 2 if rate else None
    for sizes in ((1,), (1, 2, 3, 4)):
        a = ctx.streams(3, max_frames=4, max_ref_frames=4, arith=arith)
        b = ctx.streams(3, max_frames=4, max_ref_frames=4, arith=arith)
        for st in (a, b):
            st.reset(slots, which=4)
            if rate:
                st.set_output_rate(slots, rate, preset=preset)
                st.set_output_ld(ld)
        bytes0 = b.state_bytes
        b.set_output_format(slots, fmt)
        assert b.state_bytes == bytes0 == a.state_bytes
        rows_a, counts_a = _voc_run_bytes(a, slots, mel, sizes, ld)
        rows_b, counts_b = _voc_run_bytes(b, slots, mel, sizes, ld)
        assert counts_a == counts_b, (fmt, rate, sizes)
        if rate:
            want, tail = schedule(out_filter(rate, preset), [fr * HOP for fr, _ in counts_b])
            assert [c for _, c in counts_b] == [[w] * n for w in want], (fmt, rate, sizes)
            if rate == 11025:
                assert want[0] < want[1] and any(w % 2 for w in want) and any(w % 4 for w in want)      # a short first call, ragged 8-bit tails
        else:
            assert [c for _, c in counts_b] == [[fr * HOP] * n for fr, _ in counts_b]
        for ra, rb in zip(rows_a, rows_b):
            for i in range(n):
                assert rb[i].dtype == sf_dtype(fmt)
                assert torch.equal(rb[i], ctx.convert_samples(ra[i], "f32", fmt)), (fmt, rate, sizes, i)
        assert a.output_pending(slots) == b.output_pending(slots)
        fa, fb = a.flush_output(slots), b.flush_output(slots)
        torch.cuda.synchronize()
        for i in range(n):
            assert fb[i].dtype == sf_dtype(fmt) and fb[i].shape == fa[i].shape
            if rate:
                assert fa[i].shape[0] == tail > 0
                assert torch.equal(fb[i], ctx.convert_samples(fa[i], "f32", fmt)), (fmt, rate, sizes, i)
        a.close()
        b.close()


def resample_len(rate, n):
    from tests import resample_ref
    return resample_ref.length(16000, rate, n)


def sf_dtype(fmt):
    return {"f32": torch.float32, "s16": torch.int16, "ulaw": torch.uint8, "alaw": torch.uint8}[fmt]


def test_flush_into_sentinel_bytes(ctx):
    """conan_streams_flush_output with a row stride wider than the tail: the bytes past each row's count keep the sentinel."""
    slots, mel = [0, 1], _mel(2, 5, 410)
    st = ctx.streams(2, max_frames=4, max_ref_frames=4)
    st.reset(slots, which=4)
    st.set_output_rate(slots, 11025, preset="kaiser_best")
    st.set_output_format([0], "ulaw")
    st.set_output_format([1], "s16")
    st.set_output_ld(1000)
    st.hifigan_step(slots, mel[:, :4])
    st.hifigan_step(slots, mel[:, 4:])
    pend = st.output_pending(slots)
    raw = torch.full((2, 400), SENT, dtype=torch.uint8, device="cuda")
    rows = st.flush_output(slots, out=raw.view(torch.float32))
    torch.cuda.synchronize()
    assert [r.shape[0] for r in rows] == pend and pend[0] == pend[1] > 0
    assert rows[0].dtype == torch.uint8 and rows[1].dtype == torch.int16
    assert bool((raw[0, pend[0]:] == SENT).all()) and bool((raw[1, 2 * pend[1]:] == SENT).all())
    assert not bool((raw[0, :pend[0]] == SENT).all())
    st.close()


# ---- 4. telephony end to end
def test_telephony_ulaw_8k_in_and_out(ctx):
    """64 slots, 8 kHz mu-law in and out, pipelined: the float engine at 8 kHz on the decoded input, its output encoded."""
    B = 64
    N = (3 * L + 5) // 2
    codes, floats = _coded(B, N, 8000, 500, "ulaw")
    ref = _ref(B)
    a = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    b = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    wa, ma, ca = a.infer_wav(floats, ref, pipelined=True, in_rate=8000, out_rate=8000)
    wb, mb, cb = b.infer_wav(codes, ref, pipelined=True, in_rate=8000, out_rate=8000, in_format="ulaw", out_format="ulaw")
    torch.cuda.synchronize()
    assert torch.equal(ma, mb) and torch.equal(ca, cb)
    assert wb.dtype == torch.uint8 and wb.shape == wa.shape
    assert torch.equal(wb, ctx.convert_samples(wa, "f32", "ulaw"))
    assert a.st.state_bytes == b.st.state_bytes


# ---- 5. launch accounting
def _launches_per_call(eng, src, **start):
    """(samples > 0, emit, resample_stream_kernel launches, resample_out_kernel launches) per call of a blocking feed loop, drain included."""
    eng.start_wav(_ref(src.shape[0]), **start)
    Li = _lin(start.get("in_rate") or 16000)
    N = src.shape[1]
    last = (N - 1) // Li * Li
    out, pos, fin = [], 0, False
    while True:
        done = False
        if pos < last:
            piece, pos = src[:, pos:pos + Li], pos + Li
            (e, _, _, _), ks = _profiled(eng.st, lambda: eng.st.step_wav(eng.slots, piece))
        else:
            piece = src[:, pos:] if not fin else src[:, :0]
            (e, _, _, _), ks = _profiled(eng.st, lambda: eng.st.step_wav(eng.slots, piece, final=True))
            pos, done, fin = N, fin and e == 0, True
        out.append((piece.shape[1] > 0, e, ks.get(RS, 0), ks.get(RO, 0)))
        if done:
            return out


def test_launch_accounting(ctx):
    B = 2
    N = 3 * L + 11
    codes, floats = _coded(B, N, 16000, 600, "s16")
    eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    bytes0 = eng.st.state_bytes
    # no format anywhere: no launch of either kernel
    plain = _launches_per_call(eng, floats)
    assert all(c[2] == 0 and c[3] == 0 for c in plain), plain
    # a format and no rate: exactly one of each, per wav-in call with samples and per vocoder step
    both = _launches_per_call(eng, codes, in_format="s16", out_format="s16")
    assert eng.st.state_bytes == bytes0
    assert [c[:2] for c in both] == [c[:2] for c in plain]
    assert [c[2] for c in both] == [int(c[0]) for c in both] and [c[3] for c in both] == [int(c[1] > 0) for c in both], both
    assert sum(c[2] for c in both) == 4 and sum(c[3] for c in both) >= 3
    only_in = _launches_per_call(eng, codes, in_format="s16")
    assert [c[2] for c in only_in] == [c[2] for c in both] and all(c[3] == 0 for c in only_in), only_in
    # "f32" again: the launch counts return to zero
    again = _launches_per_call(eng, floats, in_format="f32", out_format="f32")
    assert again == plain and not eng.st.input_formats and not eng.st.output_formats
    assert eng.st.state_bytes == bytes0
    # a format plus a rate: the launches of the rate alone
    c8, f8 = _coded(B, N // 2, 8000, 601, "alaw")
    r = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    rate_only = _launches_per_call(r, f8, in_rate=8000, out_rate=8000)
    bytes_r = r.st.state_bytes
    rate_fmt = _launches_per_call(r, c8, in_rate=8000, out_rate=8000, in_format="alaw", out_format="alaw")
    assert rate_fmt == rate_only and sum(c[2] for c in rate_only) > 0 and sum(c[3] for c in rate_only) > 0
    assert r.st.state_bytes == bytes_r


# ---- 6. errors and persistence
def test_unknown_format_and_wrong_dtype(ctx):
    eng = StreamingVoiceConversionEngine(ctx, 2, max_ref_frames=64)
    eng.start_wav(_ref(2))
    lib, h = eng.st.lib, eng.st.h
    slots = (C.c_int32 * 2)(0, 1)
    for bad in (-1, 4, 255):
        assert lib.conan_streams_set_input_format(h, slots, 2, bad) == _lib.ERR_INVALID
        assert lib.conan_streams_set_output_format(h, slots, 2, bad) == _lib.ERR_INVALID
    assert lib.conan_streams_set_input_format(h, (C.c_int32 * 2)(0, 2), 2, _lib.SAMPLE_S16) == _lib.ERR_INVALID      # slot out of range
    assert lib.conan_streams_set_output_format(h, (C.c_int32 * 2)(1, 1), 2, _lib.SAMPLE_S16) == _lib.ERR_INVALID     # duplicate slot
    x = torch.zeros(4, device="cuda")
    assert lib.conan_convert_samples(ctx.h, 0, C.c_void_p(x.data_ptr()), 1, 5, C.c_void_p(x.data_ptr()), 1, 1, 1, None) == _lib.ERR_INVALID
    assert lib.conan_convert_samples(ctx.h, 0, C.c_void_p(x.data_ptr()), 1, 1, C.c_void_p(x.data_ptr()), 1, 1, 3, None) == _lib.ERR_INVALID   # 3 floats in a 4-byte row
    with pytest.raises(ValueError):
        eng.st.set_input_format([0], "s24")
    # nothing changed: float rows still step
    codes, floats = _coded(2, L, 16000, 700, "s16")
    eng.st.step_wav([0, 1], floats)
    with pytest.raises(ValueError):
        eng.st.step_wav([0, 1], codes)                 # int16 rows for float32 slots
    eng.st.set_input_format([0, 1], "s16")
    with pytest.raises(ValueError):
        eng.st.step_wav([0, 1], floats)                # float rows for s16 slots
    eng.st.set_input_format([1], "ulaw")
    with pytest.raises(ValueError):
        eng.st.step_wav([0, 1], codes)                 # one dtype for two formats: rows go as a list in the ragged step


def test_input_row_that_does_not_fit_leaves_slots_unchanged(ctx):
    """A 48 kHz s16 row (7680 bytes) does not fit conan_step_wav_ragged's stride of 5120 bytes; the same samples as mu-law do."""
    rate, B = 48000, 2
    Li = _lin(rate)
    codes, _ = _coded(B, 3 * Li + 101, rate, 710, "s16")
    ref = _ref(B)
    clean = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    clean.start_wav(ref, in_rate=rate, in_format="s16")
    want = _run_manual(clean, codes, Li)
    eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    eng.start_wav(ref, in_rate=rate, in_format="s16")
    lib, h = eng.st.lib, eng.st.h
    slots = (C.c_int32 * B)(*eng.slots)
    mc = mel_cfg()

    def hook(i):
        if i != 1:
            return
        wav = torch.zeros(B, Li, device="cuda")
        sm, fi, emit = (C.c_int32 * B)(Li, Li), (C.c_int32 * B)(0, 0), (C.c_int32 * B)()
        out = torch.empty(B, L, device="cuda")
        args = (C.c_void_p(wav.data_ptr()), C.byref(mc), None, None, C.c_void_p(out.data_ptr()), emit, None)
        assert lib.conan_step_wav_ragged(h, slots, B, sm, fi, *args) == _lib.ERR_INVALID, lib.conan_last_error()
        assert b"stride" in lib.conan_last_error()
        # an unaligned wav_dev
        assert lib.conan_step_wav_ragged_ld(h, slots, B, sm, fi, C.c_void_p(wav.data_ptr() + 2), 2 * Li, *args[1:]) == _lib.ERR_INVALID

    got = _run_manual(eng, codes, Li, hook)
    assert _equal(got, want)
    # the same samples as mu-law fit the default stride: 3840 bytes
    u = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    u.open_slots(u.slots, ref, in_rate=rate, in_format="ulaw")
    ucodes, _ = _coded(B, Li, rate, 711, "ulaw")
    emit, _, _, _ = u.st.step_wav_ragged(u.slots, ucodes, [Li, Li], [0, 0])
    assert emit == [0, 0]


def test_output_row_that_does_not_fit_leaves_slots_unchanged(ctx):
    n, T = 2, 12
    slots, mel = [1, 0], _mel(2, 12, 720)
    a = ctx.streams(2, max_frames=4, max_ref_frames=4)
    b = ctx.streams(2, max_frames=4, max_ref_frames=4)
    for st in (a, b):
        st.reset(slots, which=4)
        st.set_output_format(slots, "s16")
    want = [a.hifigan_step(slots, mel[:, p:p + 4]) for p in range(0, T, 4)]
    got = [b.hifigan_step(slots, mel[:, 0:4])]
    b.set_output_ld(4 * HOP // 2 - 1)                    # 1280 s16 samples need 640 four-byte units
    with pytest.raises(_lib.ConanError) as e:
        b.hifigan_step(slots, mel[:, 4:8])
    assert e.value.code == _lib.ERR_INVALID
    b.set_output_ld(4 * HOP // 2)                        # exactly enough
    got.append(b.hifigan_step(slots, mel[:, 4:8]))
    b.set_output_ld(0)
    got.append(b.hifigan_step(slots, mel[:, 8:12]))
    torch.cuda.synchronize()
    for ra, rb in zip(want, got):
        assert all(x.dtype == torch.int16 for x in rb) and _equal(ra, rb)
    # a flush whose stride is too small for the bytes of the tail
    for st in (a, b):
        st.reset(slots, which=4)
        st.set_output_rate(slots, 48000)
        st.set_output_ld(3 * 4 * HOP)
        st.hifigan_step(slots, mel[:, :4])
    pend = b.output_pending(slots)[0]
    buf = torch.empty(2, pend // 2 - 1, device="cuda")
    rc = b.lib.conan_streams_flush_output(b.h, (C.c_int32 * 2)(*slots), 2, C.c_void_p(buf.data_ptr()), buf.shape[1], None)
    assert rc == _lib.ERR_INVALID and b.output_pending(slots) == [pend] * 2
    assert _equal(a.flush_output(slots), b.flush_output(slots))
    a.close()
    b.close()


def test_formats_survive_resets(ctx):
    B = 2
    ca, _ = _coded(B, 2 * L + 77, 16000, 730, "ulaw")
    cb, _ = _coded(B, 3 * L - 5, 16000, 731, "ulaw")
    ref = _ref(B)
    eng = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    eng.start_wav(ref, in_format="ulaw", out_format="alaw")
    _run_manual(eng, ca, L)
    eng.st.reset(eng.slots, which=7)                   # models only
    eng.st.reset(eng.slots, which=_lib.MODEL_FRONTEND)
    eng.st.set_reference(eng.slots, ref)
    got = _run_manual(eng, cb, L)
    fresh = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    fresh.start_wav(ref, in_format="ulaw", out_format="alaw")
    want = _run_manual(fresh, cb, L)
    assert got[0].dtype == torch.uint8 and _equal(got, want)
    # and the floats agree with an engine without formats
    plain = StreamingVoiceConversionEngine(ctx, B, max_ref_frames=64)
    plain.start_wav(ref)
    w, m, c = _run_manual(plain, _cuda(sf.decode(cb.cpu().numpy(), "ulaw")), L)
    assert torch.equal(got[0], ctx.convert_samples(w, "f32", "alaw")) and torch.equal(got[1], m) and torch.equal(got[2], c)
