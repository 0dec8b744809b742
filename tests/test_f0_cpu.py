"""Source-pitch following without a GPU: the C surface (symbols, the 24-byte cfg and its ctypes mirror, the header as C), and the
order of the checks - every refused cfg field is refused before a handle is touched, so fake handles are never dereferenced."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conan_amd import _lib

SYMBOLS = ["conan_f0", "conan_streams_set_pitch_follow", "conan_streams_pitch_follow", "conan_step_wav_contour"]


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    return _lib.lib()


def test_symbols_exported():
    _lib_or_skip()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.declared_symbols() and name in _lib._PROTOS
    assert raw.conan_abi_version() == 9      # (the feature is detected by symbol: no struct changed)


def test_cfg_mirror_and_defaults():
    assert C.sizeof(_lib.F0Cfg) == 24
    c = _lib.f0_cfg()
    assert (c.enabled, c.fmin, c.fmax, c.reserved) == (1, 50.0, 900.0, 0)
    assert abs(c.threshold - 0.15) < 1e-7 and c.floor_db == -60.0
    assert _lib.f0_keywords(_lib.f0_cfg(fmin=60, fmax=500, threshold=0.2, floor_db=-50)) == dict(fmin=60.0, fmax=500.0, threshold=C.c_float(0.2).value, floor_db=-50.0)


def test_header_compiles_as_c_and_matches_the_mirror(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not present")
    inc = os.path.dirname(_lib.HEADER_PATH)
    fields = [f[0] for f in _lib.F0Cfg._fields_]
    protos = tmp_path / "protos.c"
    protos.write_text('#include "conan_hip.h"\n'
                      'int (*a)(conan_ctx*, const conan_mel_cfg*, const conan_f0_cfg*, const float*, int, int, float*, float*, int32_t*, void*) = conan_f0;\n'
                      'int (*b)(conan_streams*, const int32_t*, int, const conan_f0_cfg*, void*) = conan_streams_set_pitch_follow;\n'
                      'int (*c)(const conan_streams*, int, conan_f0_cfg*) = conan_streams_pitch_follow;\n'
                      'int (*d)(conan_streams*, float*, float*, void*) = conan_step_wav_contour;\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(protos), "-o", str(tmp_path / "protos.o")], check=True)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "conan_hip.h"\n'
                     'int main(void) {\n'
                     '  printf("%d %zu %zu", CONAN_HIP_ABI_VERSION, sizeof(conan_f0_cfg), sizeof(conan_pitch_cfg));\n' +
                     "".join('  printf(" %%zu", offsetof(conan_f0_cfg, %s));\n' % f for f in fields) +
                     '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, str(probe), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [9, 24, 24] + [getattr(_lib.F0Cfg, f).offset for f in fields]


def _mel(fft=1024, hop=320, rate=16000):
    return _lib.MelCfg(fft, hop, fft, 80, rate, 80.0, 7600.0, 1e-6, -6.0, 1.5, 0, 0, 0.0)


def test_null_and_invalid_arguments_are_refused_before_any_gpu_use():
    lib = _lib_or_skip()
    one = (C.c_int32 * 1)(0)
    ok, mel = _lib.f0_cfg(), _mel()
    fake = C.c_void_p(16)      # never dereferenced: the checks below come first
    frames = C.c_int32(0)

    def f0(ctx=fake, m=mel, c=ok, wav=fake, n=1, samples=1000, o1=fake, o2=fake):
        return lib.conan_f0(ctx, C.byref(m) if m is not None else None, C.byref(c) if c is not None else None, wav, n, samples, o1, o2, C.byref(frames), None)

    for kw in (dict(ctx=None), dict(m=None), dict(c=None), dict(wav=None), dict(o1=None), dict(o2=None)):
        assert f0(**kw) == _lib.ERR_INVALID
        assert b"null argument" in lib.conan_last_error()
    assert lib.conan_streams_set_pitch_follow(None, one, 1, C.byref(ok), None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_pitch_follow(fake, None, 1, C.byref(ok), None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_pitch_follow(fake, one, 1, None, None) == _lib.ERR_INVALID
    assert lib.conan_streams_pitch_follow(None, 0, C.byref(ok)) == _lib.ERR_INVALID      # (host only: no device is touched either way)
    assert lib.conan_streams_pitch_follow(fake, 0, None) == _lib.ERR_INVALID
    assert lib.conan_step_wav_contour(None, fake, fake, None) == _lib.ERR_INVALID
    assert lib.conan_step_wav_contour(fake, None, fake, None) == _lib.ERR_INVALID
    assert lib.conan_step_wav_contour(fake, fake, None, None) == _lib.ERR_INVALID
    # every refused field of the cfg, by both entry points, before the handle is touched
    inf, nan = float("inf"), float("nan")
    bad = [dict(fmin=0.0), dict(fmin=-5.0), dict(fmin=nan), dict(fmax=inf), dict(fmax=nan), dict(fmin=900.0, fmax=900.0), dict(fmin=950.0),
           dict(threshold=0.0), dict(threshold=1.0), dict(threshold=-0.1), dict(threshold=nan), dict(floor_db=nan), dict(floor_db=-inf)]
    cfgs = [_lib.f0_cfg(**kw) for kw in bad]
    for field, value in (("enabled", 2), ("enabled", -1), ("reserved", 7)):
        c = _lib.f0_cfg()
        setattr(c, field, value)
        cfgs.append(c)
    for c in cfgs:
        assert f0(c=c) == _lib.ERR_INVALID, lib.conan_last_error()
        assert lib.conan_streams_set_pitch_follow(fake, one, 1, C.byref(c), None) == _lib.ERR_INVALID
    # the limits that depend on the frame: tmin >= 2, tmax <= fft_size / 2
    assert f0(c=_lib.f0_cfg(fmax=8000.5)) == _lib.ERR_INVALID and b"fmax" in lib.conan_last_error()
    assert f0(c=_lib.f0_cfg(fmin=31.0)) == _lib.ERR_INVALID and b"fmin" in lib.conan_last_error()
    assert f0(c=_lib.f0_cfg(fmin=62.0), m=_mel(fft=512)) == _lib.ERR_INVALID      # tmax = 259 > 256
    # conan_f0's own arguments: an enabled cfg, the frame, the rate, the row and sample counts
    assert f0(c=_lib.F0Cfg()) == _lib.ERR_INVALID and b"enabled" in lib.conan_last_error()
    for m in (_mel(fft=1000), _mel(fft=4096), _mel(fft=32), _mel(hop=0), _mel(rate=22050)):
        assert f0(m=m) == _lib.ERR_INVALID
    assert f0(n=0) == _lib.ERR_INVALID and f0(n=65536) == _lib.ERR_INVALID and f0(samples=0) == _lib.ERR_INVALID
