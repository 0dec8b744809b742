"""conan_loud_norm on the GPU (BS.1770 meter, gain to the target, peak division) against tests/loudness_ref.py, the numpy restatement
of the arithmetic include/conan_hip.h defines, and the Python paths that use it (Context.loud_norm / .loudness, librosa_wav2spec,
StreamingVoiceConversion, the engine's whole-utterance calls).

Tolerances.  LUFS: 2e-5 LU - an error of d dB in the gain shifts every log10-mel value by d / 20, the front-end is held to 1e-5 in
log10 units (tests/test_gpu_api.py), so 2e-5 LU is a tenth of that budget; the segment-parallel recursion differs from the serial one
by 1e-13 in y, so the bound is a ceiling, not a fit.  y: at most 1 float32 ulp from the restatement - only the device's pow and log10
differ from numpy's, by ulps of a double, and the one rounding to float32 can then fall on either side.  The gain in the stats:
ln(10) / 20 * 2e-5 relative, what the LUFS bound allows.  Everything that compares the library with itself is exact."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conan_amd import _lib
from tests import loudness_ref as LR
from tests.wav_helpers import _ref, ctx  # noqa: F401  (ctx: module fixture)

pytestmark = pytest.mark.gpu

RATES = (8000, 11025, 16000, 22050, 44100)
SEG = 128                      # cnk::kLdSeg: samples per lane of the state / energy passes (64 lanes per workgroup: 8192 per tile)
LUFS_TOL = 2e-5
GAIN_RTOL = np.log(10.0) / 20.0 * LUFS_TOL
SENT = 7.0
PAD = 37                       # floats between the longest row's end and the next row


def _lengths(fs):
    """Exactly one gating block; about 5 s (several workgroups, every block-edge pattern of the rate); at 16 kHz the two-block row
    whose second block is truncated and the lengths around a multiple of the segment length that is also a workgroup's tile; at
    8 kHz the lengths around a multiple of the segment length inside a tile."""
    out = [int(0.4 * fs), 5 * fs + 13]
    if fs == 16000:
        out += [7300, 64 * SEG - 1, 64 * SEG, 64 * SEG + 1]
    if fs == 8000:
        out += [26 * SEG - 1, 26 * SEG, 26 * SEG + 1]
    return out


def _bursts(N, fs, seed):
    """Seeded noise bursts with quiet stretches between them: loud, below the absolute gate, below the relative gate, medium, ..."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(N)
    levels, pos, k = (0.1, 2e-6, 0.003, 0.05), 0, 0
    if N <= fs:                                    # a short row is one burst
        return (0.1 * x).astype(np.float32)
    while pos < N:
        d = int(rng.uniform(0.35, 0.8) * fs)
        x[pos:pos + d] *= levels[k % len(levels)]
        pos, k = pos + d, k + 1
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _data():
    """rate -> [(x, y_ref, stats_ref)] with read-only arrays, computed once.  Before the GPU is asked anything the restatement shows
    that both gates drop blocks, that no block lies within 0.01 LU of either gate (a rounding difference cannot flip a block), and
    that no row is skipped."""
    out, abs_dropped, rel_dropped = {}, 0, 0
    for fs in RATES:
        rows = []
        for j, N in enumerate(_lengths(fs)):
            x = _bursts(N, fs, 1000 + fs % 997 + j)
            m = LR.measure(x, fs)
            assert np.isfinite(m["L"]), (fs, N)
            assert np.abs(m["l"] - LR.ABS_GATE).min() > 0.01 and np.abs(m["l"] - m["gamma_r"]).min() > 0.01, (fs, N)
            a, r = int((m["l"] < LR.ABS_GATE).sum()), int(((m["l"] >= LR.ABS_GATE) & (m["l"] <= m["gamma_r"])).sum())
            if N > 4 * fs:
                assert a > 0 and r > 0, (fs, N, a, r)
            abs_dropped, rel_dropped = abs_dropped + a, rel_dropped + r
            y, st = LR.normalize(x, fs)
            for v in (x, y, st):
                v.flags.writeable = False
            rows.append((x, y, st))
        out[fs] = rows
    assert abs_dropped > 0 and rel_dropped > 0
    return out


def _ulps(a, b):
    """Largest distance in float32 ulps between two finite float32 arrays."""
    def key(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(a) - key(b)).max()) if len(a) else 0


def _pack(rows, ld):
    buf = torch.zeros(len(rows), ld)
    for i, x in enumerate(rows):
        buf[i, :len(x)] = torch.from_numpy(np.array(x))
    return buf.cuda()


def _call(ctx, xs, fs, **kw):
    """One conan_loud_norm call over rows of unequal length with strides beyond the longest row -> (x buffer, y buffer, stats)."""
    lens = [len(x) for x in xs]
    ld = max(lens) + PAD
    xb = _pack(xs, ld)
    yb = torch.full((len(xs), ld + 11), SENT, device="cuda")
    y, st = ctx.loud_norm(xb[:, :max(lens)], fs, lengths=lens, return_stats=True, out=yb, **kw)
    torch.cuda.synchronize()
    assert y.data_ptr() == yb.data_ptr()
    return xb, yb, st


@pytest.mark.parametrize("fs", RATES)
def test_unequal_rows_match_the_restatement(ctx, fs):
    rows = _data()[fs]
    xs = [r[0] for r in rows]
    _, yb, st = _call(ctx, xs, fs)
    yb, st = yb.cpu().numpy(), st.cpu().numpy()
    worst_l = worst_u = 0
    for i, (x, y_ref, st_ref) in enumerate(rows):
        N = len(x)
        dl, du = abs(st[i, 0] - st_ref[0]), _ulps(yb[i, :N], y_ref)
        worst_l, worst_u = max(worst_l, dl), max(worst_u, du)
        print("fs %d N %d: LUFS %.6f (ref %.6f, diff %.3g), gain %.6g, blocks %d, y within %d ulp" % (fs, N, st[i, 0], st_ref[0], dl, st[i, 1], st[i, 3], du))
    for i, (x, y_ref, st_ref) in enumerate(rows):
        N = len(x)
        assert abs(st[i, 0] - st_ref[0]) <= LUFS_TOL, (fs, N)
        assert _ulps(yb[i, :N], y_ref) <= 1, (fs, N)
        assert abs(st[i, 1] / st_ref[1] - 1) <= GAIN_RTOL and abs(st[i, 2] / st_ref[2] - 1) <= GAIN_RTOL and st[i, 3] == st_ref[3], (fs, N, st[i], st_ref)
        assert np.all(yb[i, N:] == SENT), (fs, N)              # only the first samples[i] floats of a row are written
    print("fs %d: max LUFS deviation %.3g LU, max y deviation %d ulp" % (fs, worst_l, worst_u))


@pytest.mark.parametrize("fs", RATES)
def test_a_row_does_not_depend_on_its_batch_or_the_run(ctx, fs):
    xs = [r[0] for r in _data()[fs]]
    _, y1, s1 = _call(ctx, xs, fs)
    _, y2, s2 = _call(ctx, xs, fs)
    assert torch.equal(y1, y2) and torch.equal(s1, s2)
    for i in list(range(len(xs)))[::-1]:
        _, ya, sa = _call(ctx, [xs[i]], fs)
        N = len(xs[i])
        assert torch.equal(ya[0, :N], y1[i, :N]) and torch.equal(sa[0], s1[i]), (fs, N)


@pytest.mark.parametrize("fs", RATES)
def test_a_row_one_sample_short_of_a_block_is_refused_before_any_launch(ctx, fs):
    rows = _data()[fs]
    short = rows[0][0][:int(0.4 * fs) - 1]
    with pytest.raises(_lib.ConanError) as e:
        _call(ctx, [short], fs)
    assert e.value.code == _lib.ERR_INVALID
    # inside a batch of valid rows: every row is checked first, nothing is written
    xs = [rows[0][0], short, rows[0][0]]
    ld = len(xs[0]) + PAD
    xb, yb = _pack(xs, ld), torch.full((3, ld), SENT, device="cuda")
    st = torch.full((3, 4), SENT, dtype=torch.float64, device="cuda")
    lens = np.array([len(x) for x in xs], dtype=np.int64)
    cfg = _lib.LoudnessCfg(fs, -22.0, 1, (C.c_int32 * 3)(0, 0, 0))
    rc = ctx.lib.conan_loud_norm(ctx.h, C.byref(cfg), C.c_void_p(xb.data_ptr()), ld, 3, lens.ctypes.data_as(C.c_void_p), C.c_void_p(yb.data_ptr()), ld,
                                 C.c_void_p(st.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == _lib.ERR_INVALID and bool((yb == SENT).all()) and bool((st == SENT).all())


def test_rows_without_a_loudness_are_copied_unchanged(ctx):
    rng = np.random.default_rng(11)
    fs = 16000
    quiet = (1e-5 * rng.standard_normal(2 * fs + 5)).astype(np.float32)
    silent = np.zeros(fs, np.float32)
    loud = np.array(_data()[fs][0][0])
    for x in (quiet, silent):
        assert LR.loudness(x, fs) == -np.inf
    xs = [loud, silent, quiet]
    _, yb, st = _call(ctx, xs, fs)
    yb, st = yb.cpu().numpy(), st.cpu().numpy()
    for i in (1, 2):
        N = len(xs[i])
        assert np.array_equal(yb[i, :N], xs[i]) and np.all(yb[i, N:] == SENT)
        assert st[i, 0] == -np.inf and st[i, 1] == 1.0 and st[i, 3] == 0 and st[i, 2] == np.abs(xs[i]).max()
    assert np.isfinite(st[0, 0]) and _ulps(yb[0, :len(loud)], _data()[fs][0][1]) <= 1
    assert ctx.loudness(torch.from_numpy(silent), fs).item() == -np.inf


def test_peak_limit(ctx):
    """Unit spikes every 4000 samples over 1e-3 noise, 2 s at 16 kHz: the gain to -22 LUFS lifts the spikes above 1."""
    fs = 16000
    rng = np.random.default_rng(12)
    x = (1e-3 * rng.standard_normal(2 * fs)).astype(np.float32)
    x[::4000] = 1.0
    y_on, s_on = LR.normalize(x, fs, peak_limit=True)
    y_off, s_off = LR.normalize(x, fs, peak_limit=False)
    print("peak-limit row: L %.3f, gain %.4f, peak %.4f" % (s_off[0], s_off[1], s_off[2]))
    assert abs(s_off[0] - (-33.4)) < 0.1 and abs(s_off[1] - 3.70) < 0.01 and abs(s_off[2] - 3.71) < 0.01
    g_on, t_on = ctx.loud_norm(torch.from_numpy(x), fs, return_stats=True)
    g_off, t_off = ctx.loud_norm(torch.from_numpy(x), fs, peak_limit=False, return_stats=True)
    g_on, g_off, t_on, t_off = g_on.cpu().numpy(), g_off.cpu().numpy(), t_on.cpu().numpy(), t_off.cpu().numpy()
    assert _ulps(g_on, y_on) <= 1 and _ulps(g_off, y_off) <= 1
    assert _ulps(np.abs(g_on).max(keepdims=True), np.ones(1, np.float32)) <= 1
    assert abs(np.abs(g_off).max() - 3.71) < 0.01
    for got, want in ((t_on, s_on), (t_off, s_off)):
        assert abs(got[0] - want[0]) <= LUFS_TOL and abs(got[1] / want[1] - 1) <= GAIN_RTOL and abs(got[2] / want[2] - 1) <= GAIN_RTOL and got[3] == want[3]
    assert t_on[1] < t_off[1] and t_on[2] == t_off[2]


def test_in_place_and_measure_only_equal_the_full_call(ctx):
    fs = 22050
    xs = [r[0] for r in _data()[fs]]
    xb, yb, st = _call(ctx, xs, fs)
    lens = [len(x) for x in xs]
    keep = xb.clone()
    y2, st2 = ctx.loud_norm(xb[:, :max(lens)], fs, lengths=lens, return_stats=True, out=xb)      # y_dev == x_dev
    torch.cuda.synchronize()
    assert y2.data_ptr() == xb.data_ptr() and torch.equal(st2, st)
    for i, N in enumerate(lens):
        assert torch.equal(xb[i, :N], yb[i, :N]) and torch.equal(xb[i, N:], keep[i, N:])
    got = ctx.loudness(keep[:, :max(lens)], fs, lengths=lens)
    assert got.dtype == torch.float64 and torch.equal(got, st[:, 0])
    assert torch.equal(keep, _pack(xs, max(lens) + PAD))                # a measure-only call writes no audio


def test_python_front_end_honours_loud_norm(ctx):
    from conan_amd import configs, synth
    from conan_amd.inference.Conan import StreamingVoiceConversion
    from conan_amd.utils.audio import librosa_wav2spec
    from oracle import frontend as ofe
    fs = 16000
    x, y_ref, _ = _data()[fs][2]                       # 7300 samples
    kw = dict(fft_size=1024, hop_size=320, win_length=1024, num_mels=80, fmin=80, fmax=7600, sample_rate=fs)
    out = librosa_wav2spec(np.array(x), loud_norm=True, ctx=ctx, **kw)
    ref = ofe.wav2mel(y_ref, mel_vmin=-1e30, mel_vmax=1e30)
    assert out["mel"].shape == ref.shape and np.abs(out["mel"] - ref).max() < 1e-5, np.abs(out["mel"] - ref).max()
    assert np.array_equal(out["wav_orig"], x) and _ulps(out["wav"][:len(x)], y_ref) <= 1
    plain = librosa_wav2spec(np.array(x), ctx=ctx, **kw)
    assert np.array_equal(plain["wav"][:len(x)], x) and np.abs(plain["mel"] - ref).max() > 1e-3      # loud_norm off is unchanged
    with pytest.raises(NotImplementedError, match="trim_long_sil"):
        librosa_wav2spec(np.array(x), trim_long_sil=True, ctx=ctx, **kw)
    chp, vhp = configs.conan_hparams(True), configs.hifigan_hparams(True)
    sds = {"emformer": synth.emformer_state_dict(chp, 0), "conan": synth.conan_state_dict(chp, 0), "hifigan": synth.hifigan_state_dict(vhp, 0)}
    vc = StreamingVoiceConversion(dict(chp, loud_norm=True), vhp, sds)
    mel = vc._wav_to_mel(np.array(x)).cpu().numpy()
    want = np.clip(ref, chp["mel_vmin"], chp["mel_vmax"])
    assert mel.shape == want.shape and np.abs(mel - want).max() < 1e-5, np.abs(mel - want).max()
    wav, m = vc.infer_once({"ref_wav": np.array(x), "src_wav": np.array(x)})
    assert np.isfinite(wav).all() and m.shape[0] == mel.shape[0]


@pytest.mark.parametrize("rate", [None, 8000])
def test_engine_loud_norm_equals_the_pre_normalised_utterance(ctx, rate):
    from conan_amd.engine import StreamingVoiceConversionEngine
    fs = rate or 16000
    x = _data()[fs][0][0]
    src = torch.from_numpy(np.stack([np.array(x), 0.3 * np.array(x)[::-1]])).cuda()
    ref = _ref(2)
    eng = StreamingVoiceConversionEngine(ctx, 2, max_ref_frames=64)
    got = eng.infer_wav(src, ref, in_rate=rate, loud_norm=True)
    want = eng.infer_wav(ctx.loud_norm(src, fs), ref, in_rate=rate)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    outs = eng.infer_wav_staggered([src[0], src[1]], [0, 1], ref, in_rates=[rate, rate], loud_norm=True)
    solo = eng.infer_wav_staggered([ctx.loud_norm(src[0], fs), ctx.loud_norm(src[1], fs)], [0, 1], ref, in_rates=[rate, rate])
    assert all(torch.equal(a, b) for o, s in zip(outs, solo) for a, b in zip(o, s))
    with pytest.raises(ValueError):
        eng.infer_wav(src, ref, in_rate=rate, in_format="s16", loud_norm=True)
