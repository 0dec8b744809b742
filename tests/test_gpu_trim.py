"""Silence trimming on the GPU (conan_trim_silence; include/conan_hip.h, conan_trim_cfg) against tests/trim_ref.py, the numpy restatement
of the law, and the Python paths that use it (Context.trim_silence, librosa_wav2spec, VoiceBank.enroll_wav, the engine's whole-utterance
calls).  The law is integer sums and a bit copy, so every comparison is exact: np.array_equal on uint32 views of the audio (NaN payloads
included), torch.equal where the library is compared with itself.  Nothing here has a tolerance."""
import ctypes as C
import functools
import wave

import numpy as np
import pytest
import torch

from conan_amd import _lib
from conan_amd.runtime import mel_cfg
from tests import activity_ref as A
from tests import trim_ref as R
from tests.test_gpu_pitch import full  # noqa: F401  (module fixture: the small synthetic full model)

pytestmark = pytest.mark.gpu

HOP, FFT = 320, 1024
PLAN_TILE, GATHER_TILE = 256, 16      # cnk::kTrimThreads (frames per tile of the plan kernel), cnk::kTrimGatherFrames
SENT_F, SENT_I = 7.0, -77             # sentinels of the float and the integer buffers
LENS = (1, 319, 320, 321, 1927, 16000)
WIDTHS = ((1, 0), (2, 1), (7, 0), (8, 12), (12, 18), (64, 1000))


def _tile_lens(T):
    """Row lengths with T - 1, T, T + 1 and 2 T + 3 frames; the remainders differ so that the last frame owns 0, 1, 7 and 319 samples."""
    return [(F - 1) * HOP + r for F, r in ((T - 1, 0), (T, 1), (T + 1, 7), (2 * T + 3, 319))]


ALL_LENS = tuple(LENS) + tuple(_tile_lens(PLAN_TILE)) + tuple(_tile_lens(GATHER_TILE))


@functools.lru_cache(maxsize=None)
def _rows():
    """One row of seeded noise per length of ALL_LENS, read-only, shared by the tests."""
    rng = np.random.default_rng(11)
    out = []
    for n in ALL_LENS:
        x = rng.standard_normal(n).astype(np.float32)
        x.setflags(write=False)
        out.append(x)
    return tuple(out)


def _flags(lens, density, seed):
    rng = np.random.default_rng(seed)
    return [(rng.random(R.n_frames(n, HOP)) < density).astype(np.int32) * (1 + (np.arange(R.n_frames(n, HOP)) % 3)) for n in lens]      # (1, 2, 3: non-zero counts)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _buf(n, ld, misalign):
    """[n, ld] float32 full of sentinels on the GPU; misalign: the base is 4 bytes past a 16-byte boundary."""
    flat = torch.full((n * ld + 4,), SENT_F, device="cuda")
    return flat[1:1 + n * ld].view(n, ld) if misalign else flat[:n * ld].view(n, ld)


def _call(ctx, rows, flags=None, act_cfg=None, w=12, ms=18, ld=None, out_ld=None, plan_only=False, misalign=False, lengths=True, hop=HOP, tc=None,
          out=None, expect=_lib.OK):
    """One conan_trim_silence call over `rows` (f32 numpy rows of unequal length) in sentinel-filled buffers with strides beyond the
    longest row -> dict of everything the call could have written, the input buffer after the call included."""
    n, lens = len(rows), [len(r) for r in rows]
    samples = max(lens)
    ld, out_ld = ld or samples, out_ld or samples
    F = R.n_frames(samples, hop)
    frame_ld, act_ld = F + 3, F + 2
    xb = _buf(n, ld, misalign)
    for i, r in enumerate(rows):
        xb[i, :min(lens[i], ld)] = torch.from_numpy(np.array(r[:ld])).cuda()      # (a stride under the row's length: a call that is refused)
    keep = xb.clone()
    ob = None if plan_only else (_buf(n, out_ld, misalign) if out is None else out)
    ob_before = None if ob is None else ob.clone()
    fb = None
    if flags is not None:
        fb = torch.full((n, act_ld), 1, dtype=torch.int32, device="cuda")      # (flags past a row's frames are active: they must not count)
        for i, f in enumerate(flags):
            fb[i, :len(f)] = torch.from_numpy(np.asarray(f, dtype=np.int32)).cuda()
    mask = torch.full((n, frame_ld), SENT_I, dtype=torch.int32, device="cuda")
    off = torch.full((n, frame_ld), SENT_I, dtype=torch.int64, device="cuda")
    out_len = torch.full((n,), SENT_I, dtype=torch.int64, device="cuda")
    mc = mel_cfg(fft_size=FFT, hop_size=hop, win_length=FFT, sample_rate=50 * hop)
    tc = _lib.trim_cfg(w, ms) if tc is None else tc
    la = np.asarray(lens, dtype=np.int64)
    rc = ctx.lib.conan_trim_silence(ctx.h, C.byref(mc), C.byref(act_cfg) if act_cfg is not None else None, C.byref(tc), C.c_void_p(xb.data_ptr()), ld, n, samples,
                                    la.ctypes.data_as(C.c_void_p) if lengths else None, C.c_void_p(fb.data_ptr()) if fb is not None else None,
                                    act_ld if fb is not None else 0, C.c_void_p(ob.data_ptr()) if ob is not None else None, out_ld,
                                    C.c_void_p(mask.data_ptr()), C.c_void_p(off.data_ptr()), frame_ld, C.c_void_p(out_len.data_ptr()),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == expect, (rc, ctx.lib.conan_last_error())
    torch.cuda.synchronize()
    return dict(x=xb, x_before=keep, out=ob, out_before=ob_before, mask=mask.cpu().numpy(), off=off.cpu().numpy(), out_len=out_len.cpu().numpy(), lens=lens)


def _check(res, rows, flags, w, ms, hop=HOP):
    """Everything a call wrote against the reference, row by row; everything it must not touch against the sentinels."""
    assert torch.equal(res["x"].view(torch.int32), res["x_before"].view(torch.int32))      # the input is read only
    out = _bits(res["out"]) if res["out"] is not None else None
    sent = np.array([SENT_F], np.float32).view(np.uint32)[0]
    for i, r in enumerate(rows):
        n, F = len(r), R.n_frames(len(r), hop)
        ref, m2, off, out_len = R.trim(r, flags[i], hop, w, ms)
        assert np.array_equal(res["mask"][i, :F], m2), i
        assert np.array_equal(res["off"][i, :F], off), i
        assert (res["mask"][i, F:] == SENT_I).all() and (res["off"][i, F:] == SENT_I).all(), i
        assert res["out_len"][i] == out_len, (i, res["out_len"][i], out_len)
        if out is not None:
            assert np.array_equal(out[i, :n], ref.view(np.uint32)), i      # the kept frames' bits, then zeros up to the row's length
            assert (out[i, n:] == sent).all(), i                            # nothing past it
    return res


# ------------------------------------------------------------------------------------------------------------------ 1. caller's flags

@pytest.mark.parametrize("w,ms", WIDTHS)
def test_callers_flags_against_the_reference(full, w, ms):
    rows = list(_rows())
    for k, density in enumerate((0.1, 0.5, 0.9)):
        flags = _flags(ALL_LENS, density, 100 * w + k)
        _check(_call(full, rows, flags=flags, w=w, ms=ms, ld=max(ALL_LENS) + 8, out_ld=max(ALL_LENS) + 4), rows, flags, w, ms)
    # each of the short lengths alone, as `samples` itself (lengths = NULL)
    for i, n in enumerate(LENS[:5]):
        f = _flags([n], 0.5, 7 * w + i)
        _check(_call(full, [rows[i]], flags=f, w=w, ms=ms, lengths=False), [rows[i]], f, w, ms)


def test_hop_that_is_no_multiple_of_four(full):
    """hop 125: the frames start at any word of a 16-byte group, so a kept frame's words move one by one and four words span frames."""
    hop = 125
    rng = np.random.default_rng(3)
    rows = [rng.standard_normal(n).astype(np.float32) for n in (1, 124, 125, 126, 17 * hop + 1, 40 * hop + 77)]
    flags = [(rng.random(R.n_frames(len(r), hop)) < 0.5).astype(np.int32) for r in rows]
    _check(_call(full, rows, flags=flags, w=3, ms=1, hop=hop), rows, flags, 3, 1, hop)
    hop = 2      # more than two frames inside one group of four words
    rows = [rng.standard_normal(n).astype(np.float32) for n in (1, 2, 3, 75)]
    flags = [(rng.random(R.n_frames(len(r), hop)) < 0.5).astype(np.int32) for r in rows]
    _check(_call(full, rows, flags=flags, w=1, ms=0, hop=hop), rows, flags, 1, 0, hop)


# ------------------------------------------------------------------------------------------------------------------ 2. the detector

def test_detector_form(full):
    cfg = _lib.activity_cfg()
    x = A.burst_signal()
    act_ref, out_ref, m2, off, out_len = R.run(x, cfg, N=FFT, hop=HOP)
    kept = np.flatnonzero(m2)
    assert 0 < kept[0] and kept[-1] < len(m2) - 1 and 0 < out_len < len(x)      # the kept frames lie strictly inside the signal
    res = _check(_call(full, [x], act_cfg=cfg), [x], [act_ref], 12, 18)
    assert res["out_len"][0] == out_len
    # rows of their own lengths in one call: each row's flags are conan_activity's for that row alone, and the result is the
    # caller-flag form's on those flags
    rows = [x[:n] for n in (len(x), 30000, 47 * HOP + 5, 1)] + [np.ascontiguousarray(x[20000:70000])]
    flags = []
    for r in rows:
        act = full.activity(torch.from_numpy(r).cuda(), cfg=cfg, fft_size=FFT, hop_size=HOP, state=False)[0]
        flags.append(act.cpu().numpy())
    assert sum(int(f.sum()) for f in flags) > 100
    got = _check(_call(full, rows, act_cfg=cfg, ld=len(x) + 3), rows, flags, 12, 18)
    same = _call(full, rows, flags=flags, ld=len(x) + 3)
    for k in ("mask", "off", "out_len"):
        assert np.array_equal(got[k], same[k]), k
    assert torch.equal(got["out"].view(torch.int32), same["out"].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ 3. the law's corners

def test_all_silent_and_all_active(full):
    rows = [_rows()[ALL_LENS.index(n)] for n in (1927, 16000, _tile_lens(PLAN_TILE)[3])]
    zeros = [np.zeros(R.n_frames(len(r), HOP), np.int32) for r in rows]
    res = _check(_call(full, rows, flags=zeros), rows, zeros, 12, 18)
    assert (res["out_len"] == 0).all() and (res["mask"][:, :7] == 0).all() and (res["off"][:, :7] == -1).all()
    for i, r in enumerate(rows):
        assert not _bits(res["out"])[i, :len(r)].any()
    # digital silence through the detector
    quiet = [np.zeros(5000, np.float32)]
    res = _check(_call(full, quiet, act_cfg=_lib.activity_cfg()), quiet, [np.zeros(16, np.int32)], 12, 18)
    assert res["out_len"][0] == 0
    ones = [np.ones(R.n_frames(len(r), HOP), np.int32) for r in rows]
    res = _check(_call(full, rows, flags=ones), rows, ones, 12, 18)
    for i, r in enumerate(rows):
        F = R.n_frames(len(r), HOP)
        assert np.array_equal(_bits(res["out"])[i, :len(r)], r.view(np.uint32)) and res["out_len"][i] == len(r)
        assert np.array_equal(res["off"][i, :F], np.arange(F) * HOP)


def test_tie_rounds_to_even(full):
    """w = 8: a window with exactly four active frames is dropped, one with five is kept (no dilation: ms = 0)."""
    x = _rows()[ALL_LENS.index(16000)]      # 51 frames
    four, five = np.zeros(51, np.int32), np.zeros(51, np.int32)
    four[[20, 22, 24, 26]] = 1
    five[[20, 22, 23, 24, 26]] = 1
    res = _check(_call(full, [x, x], flags=[four, five], w=8, ms=0), [x, x], [four, five], 8, 0)
    assert res["out_len"][0] == 0 and not res["mask"][0, :51].any()
    assert res["out_len"][1] > 0 and res["mask"][1, :51].any()


@pytest.mark.parametrize("n", [50 * HOP, 50 * HOP + 7])
def test_borders(full, n):
    """Activity in frame 0 only and in frame F - 1 only; the last frame owns nothing (len % hop == 0) or seven samples."""
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    F = R.n_frames(n, HOP)
    first, last = np.zeros(F, np.int32), np.zeros(F, np.int32)
    first[0], last[F - 1] = 1, 1
    for w, ms in ((1, 0), (1, 5), (2, 4), (12, 18)):
        res = _check(_call(full, [x, x], flags=[first, last], w=w, ms=ms), [x, x], [first, last], w, ms)
        if w == 1:
            assert res["mask"][0, 0] == 1 and res["mask"][1, F - 1] == 1
            assert res["off"][0, 0] == 0 and res["out_len"][0] == HOP * (1 + ms // 2)
            back = ms - ms // 2      # frames in front of F - 1 whose window reaches it
            assert res["out_len"][1] == back * HOP + n % HOP


@pytest.mark.parametrize("misalign,ld_extra", [(False, 36), (False, 37), (True, 36), (False, 3)])
def test_payloads_and_strides(full, misalign, ld_extra):
    """NaN payloads, -0.0, infinities and denormals are copied bitwise; strides beyond the rows leave the sentinels alone; an odd
    stride and a base that is not 16-byte aligned take the single-word path."""
    rng = np.random.default_rng(17)
    special = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000], np.uint32)
    lens = (16000, 1927, 5 * HOP + 7, 3)
    rows = []
    for n in lens:
        b = rng.standard_normal(n).astype(np.float32).view(np.uint32).copy()
        pick = rng.random(n) < 0.3
        b[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
        rows.append(b.view(np.float32))
    flags = [(rng.random(R.n_frames(n, HOP)) < 0.6).astype(np.int32) for n in lens]
    _check(_call(full, rows, flags=flags, w=2, ms=1, ld=16000 + ld_extra, out_ld=16000 + ld_extra + (4 if ld_extra % 4 == 0 else 2), misalign=misalign),
           rows, flags, 2, 1)
    if ld_extra == 3:      # an aligned source and a destination that is not, and the other way round
        _check(_call(full, rows, flags=flags, w=2, ms=1, ld=16004, out_ld=16001), rows, flags, 2, 1)
        _check(_call(full, rows, flags=flags, w=2, ms=1, ld=16001, out_ld=16004), rows, flags, 2, 1)


def test_batch_independence(full):
    """65 rows of mixed lengths in one call equal each row run alone."""
    rng = np.random.default_rng(23)
    base = np.tile(A.burst_signal(seed=4), 2)
    lens = [int(v) for v in rng.integers(1, 40000, 65)]
    lens[3], lens[40] = 1, 40000
    rows = [np.ascontiguousarray(base[o:o + n]) for o, n in zip(rng.integers(0, 40000, 65), lens)]
    cfg = _lib.activity_cfg()
    both = _call(full, rows, act_cfg=cfg, ld=40000 + 12)
    flags = [(rng.random(R.n_frames(n, HOP)) < 0.4).astype(np.int32) for n in lens]
    both_f = _check(_call(full, rows, flags=flags, w=3, ms=2), rows, flags, 3, 2)
    assert both["out_len"].max() > 0
    for i in (0, 3, 17, 40, 64):
        for batch, solo in ((both, _call(full, [rows[i]], act_cfg=cfg)), (both_f, _call(full, [rows[i]], flags=[flags[i]], w=3, ms=2))):
            F, n = R.n_frames(lens[i], HOP), lens[i]
            assert np.array_equal(batch["mask"][i, :F], solo["mask"][0, :F]) and np.array_equal(batch["off"][i, :F], solo["off"][0, :F])
            assert batch["out_len"][i] == solo["out_len"][0]
            assert torch.equal(batch["out"][i, :n].view(torch.int32), solo["out"][0, :n].view(torch.int32))
            assert (batch["out"][i, n:] == SENT_F).all()


def test_plan_only_writes_no_audio(full):
    rows = [_rows()[ALL_LENS.index(n)] for n in (16000, 321)]
    flags = _flags([16000, 321], 0.5, 5)
    res = _check(_call(full, rows, flags=flags, plan_only=True), rows, flags, 12, 18)
    assert res["out"] is None and res["out_len"][0] > 0


def test_argument_errors_leave_the_buffers_alone(full):
    rows = [_rows()[ALL_LENS.index(n)] for n in (16000, 1927)]
    flags = _flags([16000, 1927], 0.5, 9)

    def untouched(res):
        assert torch.equal(res["x"].view(torch.int32), res["x_before"].view(torch.int32))
        assert (res["mask"] == SENT_I).all() and (res["off"] == SENT_I).all() and (res["out_len"] == SENT_I).all()
        if res["out"] is not None:
            assert torch.equal(res["out"].view(torch.int32), res["out_before"].view(torch.int32))

    cfg = _lib.activity_cfg()
    untouched(_call(full, rows, flags=flags, act_cfg=cfg, expect=_lib.ERR_INVALID))      # both
    untouched(_call(full, rows, expect=_lib.ERR_INVALID))                                 # neither
    for sm, ms_, res0 in ((0, 18, 0), (65537, 18, 0), (12, -1, 0), (12, 65537, 0), (12, 18, 1)):
        tc = _lib.trim_cfg(sm, ms_)
        tc.reserved[0] = res0
        untouched(_call(full, rows, flags=flags, tc=tc, expect=_lib.ERR_INVALID))
    bad = _lib.activity_cfg()
    bad.up_step = 0
    untouched(_call(full, rows, act_cfg=bad, expect=_lib.ERR_INVALID))
    untouched(_call(full, rows, flags=flags, ld=15999, expect=_lib.ERR_INVALID))
    untouched(_call(full, rows, flags=flags, out_ld=15999, expect=_lib.ERR_INVALID))
    # lengths out of range: the helper passes len(row) per row, so hand it a row longer than `samples` by way of a wrong `samples`
    n, ld = 2, 16000
    xb = _buf(n, ld, False)
    ob = _buf(n, ld, False)
    fb = torch.ones(n, 60, dtype=torch.int32, device="cuda")
    ol = torch.full((n,), SENT_I, dtype=torch.int64, device="cuda")
    mc = mel_cfg(fft_size=FFT, hop_size=HOP, win_length=FFT, sample_rate=50 * HOP)
    tc = _lib.trim_cfg()

    def raw(lens, out):
        la = np.asarray(lens, dtype=np.int64)
        rc = full.lib.conan_trim_silence(full.h, C.byref(mc), None, C.byref(tc), C.c_void_p(xb.data_ptr()), ld, n, 16000, la.ctypes.data_as(C.c_void_p),
                                         C.c_void_p(fb.data_ptr()), 60, C.c_void_p(out), ld, None, None, 0, C.c_void_p(ol.data_ptr()),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc

    for lens in ([16000, 0], [16001, 5], [-1, 5]):
        assert raw(lens, ob.data_ptr()) == _lib.ERR_INVALID and b"lengths" in full.lib.conan_last_error()
    # out overlapping wav: in place, shifted into the first row, starting at the input's last float; ending at its first is fine
    for shift in (0, 4 * 100, 4 * (2 * ld - 1), -4 * 100):
        assert raw([16000, 5], xb.data_ptr() + shift) == _lib.ERR_INVALID and b"overlap" in full.lib.conan_last_error(), shift
    assert (xb == SENT_F).all() and (ob == SENT_F).all() and (ol == SENT_I).all()
    big = _buf(2 * n, ld, False)      # two halves of one allocation, touching: no overlap
    assert full.lib.conan_trim_silence(full.h, C.byref(mc), None, C.byref(tc), C.c_void_p(big.data_ptr()), ld, n, 16000, None, C.c_void_p(fb.data_ptr()), 60,
                                       C.c_void_p(big[n:].data_ptr()), ld, None, None, 0, C.c_void_p(ol.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)) == _lib.OK
    torch.cuda.synchronize()
    assert (ol.cpu().numpy() == 16000).all() and torch.equal(big[n:], big[:n])


# ------------------------------------------------------------------------------------------------------------------ 4. the Python surface

def _speech(seed, seconds=3.0, fs=16000, tail=0.0):
    """Bursts long enough for loud_norm's 0.4 s block, with pauses the default widths cut; tail: seconds of it that are noise only."""
    x = A.burst_signal(seconds=seconds - tail, sr=fs, seed=seed)
    quiet = 1e-3 * np.random.default_rng(seed + 1000).standard_normal(int(tail * fs))
    return np.concatenate([x, quiet.astype(np.float32)])


def test_context_trim_silence(full):
    x = np.stack([_speech(1), 0.5 * _speech(2)])
    xt = torch.from_numpy(x).cuda()
    out, lens, mask, off = full.trim_silence(xt, return_mask=True)
    assert out.shape == (2, int(lens.max())) and lens.dtype == np.int64 and 0 < lens.min() and lens.max() < x.shape[1]
    for i in range(2):
        ref, m2, o, n = R.run(x[i], _lib.activity_cfg(), N=FFT, hop=HOP)[1:]
        assert n == lens[i] and np.array_equal(mask[i].cpu().numpy(), m2) and np.array_equal(off[i].cpu().numpy(), o)
        assert np.array_equal(_bits(out[i]), ref.view(np.uint32)[:out.shape[1]])
    # norm=True is loud_norm(-20 LUFS, peak limit) followed by the trim, and lengths pass through both
    got, gl = full.trim_silence(xt, norm=True, lengths=[48000, 30000], smooth_frames=8, max_silence_frames=6)
    normed = full.loud_norm(xt, 16000, target=-20.0, peak_limit=True, lengths=[48000, 30000])
    want, wl = full.trim_silence(normed, lengths=[48000, 30000], smooth_frames=8, max_silence_frames=6)
    assert np.array_equal(gl, wl) and torch.equal(got, want) and not torch.equal(got, full.trim_silence(xt, lengths=[48000, 30000], smooth_frames=8,
                                                                                                         max_silence_frames=6)[0])
    # the caller's flags, one row, and the keywords of the detector
    act = full.activity(xt[0], state=False)[0]
    a, al = full.trim_silence(xt[0], flags=act)
    b, bl = full.trim_silence(xt[0])
    assert a.dim() == 1 and al == bl == lens[0] and torch.equal(a, b)
    c, cl = full.trim_silence(xt[0], open_db=-10.0, close_db=-12.0)      # a deaf detector
    assert cl == 0 and c.shape == (0,)
    with pytest.raises(ValueError, match="flags"):
        full.trim_silence(xt[0], flags=act, open_db=-10.0)


def test_librosa_wav2spec_trims_a_file(full, tmp_path):
    from conan_amd.utils.audio import librosa_wav2spec, read_wav
    path = str(tmp_path / "clip.wav")
    pcm = np.round(_speech(3) * 32767.0).astype("<i2")
    with wave.open(path, "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
        f.writeframes(pcm.tobytes())
    kw = dict(fft_size=1024, hop_size=320, win_length=1024, num_mels=80, fmin=80, fmax=7600, sample_rate=16000)
    got = librosa_wav2spec(path, trim_long_sil=True, loud_norm=True, ctx=full, **kw)
    x, sr = read_wav(path)
    assert sr == 16000
    kept, n = full.trim_silence(torch.from_numpy(x), norm=True, hop_size=320)
    trimmed = kept[:int(n)].cpu().numpy()
    assert 0 < n < len(x) and np.array_equal(got["wav_orig"], trimmed)
    want = librosa_wav2spec(trimmed, loud_norm=True, ctx=full, **kw)
    assert np.array_equal(got["mel"], want["mel"]) and np.array_equal(got["wav"], want["wav"])
    assert got["mel"].shape[0] == 1 + int(n) // 320 < 1 + len(x) // 320
    with pytest.raises(NotImplementedError, match="trim_long_sil"):
        librosa_wav2spec(x, trim_long_sil=True, ctx=full, **kw)
    with pytest.raises(ValueError, match="multiple of 50"):
        librosa_wav2spec(path, trim_long_sil=True, ctx=full, **dict(kw, sample_rate=22051))


def test_enroll_wav_trim_equals_the_pre_trimmed_rows(full):
    from conan_amd.engine import StreamingVoiceConversionEngine
    from conan_amd.runtime import VoiceBank
    eng = StreamingVoiceConversionEngine(full, 2, max_ref_frames=256)
    bank = VoiceBank(full, 4, 256)
    clips = torch.from_numpy(np.stack([_speech(5), _speech(6, tail=1.0)])).cuda()
    bank.enroll_wav([0, 1], clips, via=eng.st, trim=True)
    rows, kept = full.trim_silence(clips)
    assert kept[0] != kept[1] and kept.max() < clips.shape[1]
    bank.enroll([2, 3], full.wav2mel(rows), [1 + int(k) // HOP for k in kept], via=eng.st)
    a, b = bank.export([0, 1]), bank.export([2, 3])
    torch.cuda.synchronize()
    assert [bank.info(i)["ref_frames"] for i in range(4)] == [1 + int(k) // HOP for k in kept] * 2
    assert torch.equal(a.blob, b.blob)
    bank.enroll_wav([1], clips[:1], via=eng.st, trim=dict(smooth_frames=1, max_silence_frames=0))
    assert bank.info(1)["ref_frames"] < bank.info(0)["ref_frames"]
    with pytest.raises(ValueError, match="no activity"):
        bank.enroll_wav([1], torch.zeros(1, 8000, device="cuda"), via=eng.st, trim=True)
    bank.close(); eng.st.close()


def test_engine_trim_equals_the_trimmed_utterances(full):
    from conan_amd.engine import StreamingVoiceConversionEngine
    from tests.wav_helpers import _ref
    src = torch.from_numpy(np.stack([_speech(7, seconds=2.0), _speech(8, seconds=2.0, tail=1.0)])).cuda()
    ref = _ref(2)
    eng = StreamingVoiceConversionEngine(full, 2, max_ref_frames=64)
    rows, kept = full.trim_silence(src)
    assert 0 < kept.min() and kept.max() < src.shape[1] and kept[0] != kept[1]
    got = eng.infer_wav(src, ref, trim=True)
    want = eng.infer_wav(rows, ref)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and got[1].shape[1] == 1 + int(kept.max()) // HOP
    both = eng.infer_wav(src, ref, trim=dict(smooth_frames=8), loud_norm=True)
    assert all(torch.equal(a, b) for a, b in zip(both, eng.infer_wav(full.loud_norm(full.trim_silence(src, smooth_frames=8)[0], 16000), ref)))
    outs = eng.infer_wav_staggered([src[0], src[1]], [0, 1], ref, trim=True)
    solo = eng.infer_wav_staggered([rows[0, :int(kept[0])], rows[1, :int(kept[1])]], [0, 1], ref)
    assert all(torch.equal(a, b) for o, s in zip(outs, solo) for a, b in zip(o, s))
    assert [o[1].shape[0] for o in outs] == [1 + int(k) // HOP for k in kept]
    with pytest.raises(ValueError, match="float32"):
        eng.infer_wav(src, ref, in_format="s16", trim=True)
    with pytest.raises(ValueError, match="trim"):
        eng.infer_wav(src, ref, trim="yes")
    eng.st.close()
