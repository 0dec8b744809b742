"""Silence trimming without a GPU: the C surface (the symbol, the 16-byte cfg and its ctypes mirror, the header as C) and the order of
the checks - every refused argument is refused before a handle is touched, so fake handles are never dereferenced."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conan_amd import _lib


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    return _lib.lib()


def test_symbol_exported():
    _lib_or_skip()
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "conan_trim_silence")
    assert "conan_trim_silence" in _lib.declared_symbols() and "conan_trim_silence" in _lib._PROTOS
    assert raw.conan_abi_version() == 9      # (the feature is detected by symbol: no struct changed)


def test_cfg_mirror_and_helper():
    assert C.sizeof(_lib.TrimCfg) == 16
    c = _lib.trim_cfg()
    assert (c.smooth_frames, c.max_silence_frames, list(c.reserved)) == (12, 18, [0, 0])
    c = _lib.trim_cfg(7, 0)
    assert (c.smooth_frames, c.max_silence_frames) == (7, 0)


def test_header_compiles_as_c_and_matches_the_mirror(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not present")
    inc = os.path.dirname(_lib.HEADER_PATH)
    fields = [f[0] for f in _lib.TrimCfg._fields_]
    protos = tmp_path / "protos.c"
    protos.write_text('#include "conan_hip.h"\n'
                      'int (*a)(conan_ctx*, const conan_mel_cfg*, const conan_activity_cfg*, const conan_trim_cfg*, const float*, int64_t, int, int64_t, '
                      'const int64_t*, const int32_t*, int64_t, float*, int64_t, int32_t*, int64_t*, int64_t, int64_t*, void*) = conan_trim_silence;\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(protos), "-o", str(tmp_path / "protos.o")], check=True)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "conan_hip.h"\n'
                     'int main(void) {\n'
                     '  printf("%d %zu", CONAN_HIP_ABI_VERSION, sizeof(conan_trim_cfg));\n' +
                     "".join('  printf(" %%zu", offsetof(conan_trim_cfg, %s));\n' % f for f in fields) +
                     '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, str(probe), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [9, C.sizeof(_lib.TrimCfg)] + [getattr(_lib.TrimCfg, f).offset for f in fields]
    assert len(_lib._PROTOS["conan_trim_silence"][1]) == 18


def test_null_and_invalid_arguments_are_refused_before_any_gpu_use():
    lib = _lib_or_skip()
    mel_ok = _lib.MelCfg(1024, 320, 1024, 80, 16000, 80.0, 7600.0, 1e-6, -6.0, 1.5, 0, 0, 0.0)
    fake, far = C.c_void_p(1 << 20), C.c_void_p(1 << 30)      # never dereferenced: the checks below come first
    NONE = object()

    def call(ctx=fake, m=mel_ok, ac=NONE, tc=None, wav=fake, ld=1000, n=2, samples=1000, lengths=None, flags=fake, act_ld=4, out=far, out_ld=1000,
             mask=fake, off=fake, frame_ld=4, out_len=fake):
        ac = None if ac is NONE else ac
        tc = _lib.trim_cfg() if tc is None else tc
        lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64)) if lengths is not None else None
        return lib.conan_trim_silence(ctx, C.byref(m) if m is not None else None, C.byref(ac) if ac is not None else None,
                                      C.byref(tc) if tc is not False else None, wav, ld, n, samples,
                                      lens.ctypes.data_as(C.c_void_p) if lens is not None else None, flags, act_ld, out, out_ld, mask, off, frame_ld, out_len,
                                      None)

    for kw in (dict(ctx=None), dict(m=None), dict(tc=False), dict(wav=None)):
        assert call(**kw) == _lib.ERR_INVALID
        assert b"null argument" in lib.conan_last_error()
    # both or neither of the detector's cfg and the caller's flags
    assert call(flags=None) == _lib.ERR_INVALID and b"exactly one" in lib.conan_last_error()
    assert call(ac=_lib.activity_cfg()) == _lib.ERR_INVALID and b"exactly one" in lib.conan_last_error()
    # the detector's cfg is checked as conan_activity checks it, and must be enabled
    bad = _lib.activity_cfg()
    bad.hold_frames = -1
    assert call(ac=bad, flags=None) == _lib.ERR_INVALID and b"hold_frames" in lib.conan_last_error()
    assert call(ac=_lib.ActivityCfg(), flags=None) == _lib.ERR_INVALID and b"mode" in lib.conan_last_error()
    # the frame geometry, as conan_activity reads it
    for field, value in (("fft_size", 1000), ("fft_size", 32), ("fft_size", 4096), ("sample_rate", 22050), ("hop_size", 0)):
        m = _lib.MelCfg(1024, 320, 1024, 80, 16000, 80.0, 7600.0, 1e-6, -6.0, 1.5, 0, 0, 0.0)
        setattr(m, field, value)
        assert call(m=m) == _lib.ERR_INVALID, (field, value)
    # the trim cfg
    for sm, ms, res in ((0, 18, 0), (-1, 18, 0), (65537, 18, 0), (12, -1, 0), (12, 65537, 0), (12, 18, 1)):
        tc = _lib.trim_cfg(sm, ms)
        tc.reserved[1] = res
        assert call(tc=tc) == _lib.ERR_INVALID, (sm, ms, res)
    for sm, ms in ((1, 0), (65536, 65536)):      # the limits themselves pass the cfg check: the next refusal is another one
        assert call(tc=_lib.trim_cfg(sm, ms), n=0) == _lib.ERR_INVALID and b"n must be" in lib.conan_last_error()
    # rows, samples, strides
    for kw in (dict(n=0), dict(n=65536), dict(samples=0), dict(samples=2 ** 30 + 1, ld=2 ** 31, out_ld=2 ** 31), dict(ld=999), dict(out_ld=999),
               dict(act_ld=3), dict(frame_ld=3), dict(ld=2 ** 40 + 1)):
        assert call(**kw) == _lib.ERR_INVALID, kw
    assert call(frame_ld=0, mask=None, off=None, n=0) == _lib.ERR_INVALID and b"n must be" in lib.conan_last_error()      # (frame_ld unused)
    # lengths: each in 1 .. samples; shorter rows need fewer frames of act_ld / frame_ld
    for lens in ([1000, 0], [1001, 5], [-3, 5]):
        assert call(lengths=lens) == _lib.ERR_INVALID and b"lengths" in lib.conan_last_error(), lens
    assert call(lengths=[600, 639], act_ld=2, frame_ld=2, n=70000) == _lib.ERR_INVALID and b"n must be" in lib.conan_last_error()
    assert call(lengths=[600, 640], act_ld=2) == _lib.ERR_INVALID and b"act_ld" in lib.conan_last_error()
    assert call(lengths=[600, 640], frame_ld=2) == _lib.ERR_INVALID and b"frame_ld" in lib.conan_last_error()
    # out overlapping wav, anywhere in either's extent: in place, a row apart, the last float
    for out in (fake, C.c_void_p((1 << 20) + 4 * 1000), C.c_void_p((1 << 20) + 4 * 1999), C.c_void_p((1 << 20) - 4 * 1999)):
        assert call(out=out) == _lib.ERR_INVALID and b"overlap" in lib.conan_last_error(), out


def test_engine_trim_values():
    """trim= of the engine's whole-utterance calls: False / None, True or a dict; anything else is refused before a handle is touched,
    and the streaming entry points do not take the keyword at all."""
    import inspect

    from conan_amd.engine import StreamingVoiceConversionEngine as Engine
    assert Engine._trim_keywords(False) is None and Engine._trim_keywords(None) is None
    assert Engine._trim_keywords(True) == {}
    kw = dict(smooth_frames=8, norm=True)
    got = Engine._trim_keywords(kw)
    assert got == kw and got is not kw
    for bad in ("yes", 1.5, [True], 3):
        with pytest.raises(ValueError, match="trim"):
            Engine._trim_keywords(bad)
    eng = Engine.__new__(Engine)      # no context, no stream-set
    eng.slots = [0, 1]
    with pytest.raises(ValueError, match="trim"):
        eng.infer_wav(None, object(), trim="yes")
    with pytest.raises(ValueError, match="trim"):
        eng.infer_wav_staggered([None, None], [0, 1], object(), trim="yes")
    for name in ("infer_wav", "infer_wav_staggered"):
        assert inspect.signature(getattr(Engine, name)).parameters["trim"].default is False
    for name in ("start_wav", "feed", "feed_ragged", "open_slots"):
        assert "trim" not in inspect.signature(getattr(Engine, name)).parameters, name
