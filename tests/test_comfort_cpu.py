"""Comfort noise without a GPU: the C surface (symbols, the 56-byte cfg, the 16-byte state and their ctypes mirrors, the header as C),
the order of the checks - every refused argument is refused before a handle is touched, so fake handles are never dereferenced - the
conversions of _lib.comfort_cfg / comfort_dbov and the engine's host logic for comfort=."""
import ctypes as C
import math
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from conan_amd import _lib
from tests import comfort_ref as R

SYMBOLS = ["conan_streams_set_comfort", "conan_streams_comfort", "conan_streams_comfort_state", "conan_step_wav_comfort", "conan_comfort_track",
           "conan_comfort_fill"]
FULL = 1 << 20


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


def test_cfg_mirror_and_conversions():
    assert C.sizeof(_lib.ComfortCfg) == 56 and C.sizeof(_lib.ComfortState) == 16
    assert _lib.COMFORT_LEVEL_MIN == R.LEVEL_MIN and _lib.COMFORT_TAPS == R.TAPS
    assert abs(_lib.COMFORT_UNITS_PER_DB - 85.04) < 0.01
    c = _lib.comfort_cfg()      # follow, 3 dB under the background, -90 .. -30 dBov, +0.25 / -2 dB per frame, colour 1, from -70 dBov
    u = _lib.COMFORT_UNITS_PER_DB
    assert (c.mode, c.reseed, c.offset, c.l_min, c.l_max, c.up_step, c.down_step, c.colour, c.seed_level, c.reserved, c.seed) == \
        (2, 0, round(-3 * u), round(-90 * u), round(-30 * u), round(0.25 * u), round(2 * u), 1, round(-70 * u), 0, 0)
    assert (c.offset, c.l_min, c.l_max, c.up_step, c.down_step, c.seed_level) == (-255, -7654, -2551, 21, 170, -5953)
    assert _lib.COMFORT_LEVEL_MIN <= c.l_min <= c.l_max <= 0
    for colour in (0, 1, 2):
        assert np.float32(_lib.comfort_cfg(colour=colour).norm) == R.norm(colour) == np.float32(_lib.comfort_norm(colour))
    c = _lib.comfort_cfg(follow=False, level_db=-50.0, seed=2 ** 64 - 1, reseed=True)
    assert (c.mode, c.level, c.seed, c.reseed) == (1, round(-50 * u), 2 ** 64 - 1, 1)
    assert _lib.comfort_cfg(rise_db=0.0).up_step == 1      # a step is at least one unit
    c = _lib.comfort_cfg(level=-1, offset=2, l_min=-3, l_max=-2, up_step=5, down_step=6, start=-7, norm=0.5)
    assert (c.level, c.offset, c.l_min, c.l_max, c.up_step, c.down_step, c.seed_level, c.norm) == (-1, 2, -3, -2, 5, 6, -7, 0.5)
    # the reported form gives the same bytes back
    c = _lib.comfort_cfg(follow=False, level_db=-44.0, offset_db=1.5, colour=2, seed=77, start_db=-33.0)
    assert bytes(_lib.comfort_cfg(**_lib.comfort_keywords(c))) == bytes(c)
    assert _lib.comfort_seed(0) != _lib.comfort_seed(1)


def test_dbov():
    assert _lib.comfort_dbov(0) == 0 and _lib.comfort_dbov(_lib.comfort_level(-30.0)) == 30 and _lib.comfort_dbov(_lib.comfort_level(-90.0)) == 90
    assert _lib.comfort_dbov(-16384) == 127 and _lib.comfort_dbov(_lib.comfort_level(-127.0)) == 127      # the byte's range
    assert _lib.comfort_dbov(-5953) == 70
    for L in range(-12000, 1, 333):      # the byte is the level in -dBov, to the nearest dB
        want = -10.0 * math.log10(2.0) * L / 256.0
        assert abs(_lib.comfort_dbov(L) - min(want, 127.0)) <= 0.5 + 1e-9


def test_header_compiles_as_c_and_matches_the_mirror(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not present")
    inc = os.path.dirname(_lib.HEADER_PATH)
    fields = [f[0] for f in _lib.ComfortCfg._fields_]
    sfields = [f[0] for f in _lib.ComfortState._fields_]
    protos = tmp_path / "protos.c"
    protos.write_text('#include "conan_hip.h"\n'
                      'int (*a)(conan_streams*, const int32_t*, int, const conan_comfort_cfg*, void*) = conan_streams_set_comfort;\n'
                      'int (*b)(const conan_streams*, int, conan_comfort_cfg*) = conan_streams_comfort;\n'
                      'int (*c)(conan_streams*, const int32_t*, int, conan_comfort_state*, void*) = conan_streams_comfort_state;\n'
                      'int (*d)(conan_streams*, int32_t*, void*) = conan_step_wav_comfort;\n'
                      'int (*e)(conan_ctx*, const conan_comfort_cfg*, const int32_t*, const double*, int, int64_t, int64_t, int32_t*, conan_comfort_state*, '
                      'void*) = conan_comfort_track;\n'
                      'int (*f)(conan_ctx*, int, const conan_comfort_cfg*, const uint64_t*, const float*, int64_t, int, int64_t, int64_t, const int32_t*, '
                      'const int32_t*, int64_t, int32_t, int32_t, float*, int64_t, void*) = conan_comfort_fill;\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(protos), "-o", str(tmp_path / "protos.o")], check=True)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "conan_hip.h"\n'
                     'int main(void) {\n'
                     '  printf("%d %zu %zu", CONAN_HIP_ABI_VERSION, sizeof(conan_comfort_cfg), sizeof(conan_comfort_state));\n' +
                     "".join('  printf(" %%zu", offsetof(conan_comfort_cfg, %s));\n' % f for f in fields) +
                     "".join('  printf(" %%zu", offsetof(conan_comfort_state, %s));\n' % f for f in sfields) +
                     '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, str(probe), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [9, 56, 16] + [getattr(_lib.ComfortCfg, f).offset for f in fields] + [getattr(_lib.ComfortState, f).offset for f in sfields]


BAD = [("mode", 3), ("mode", -1), ("reseed", 2), ("reseed", -1), ("level", 1), ("level", -16385), ("l_min", 1), ("l_min", -16385), ("l_max", 1),
       ("l_max", -16385), ("seed_level", 1), ("seed_level", -16385), ("l_min", -2000), ("offset", 16385), ("offset", -16385), ("up_step", 0),
       ("up_step", 16385), ("down_step", 0), ("down_step", -3), ("down_step", 16385), ("colour", -1), ("colour", 3), ("norm", 0.0), ("norm", -1.0),
       ("norm", float("inf")), ("norm", float("nan")), ("reserved", 1)]


def bad_cfgs():
    out = []
    for field, value in BAD:
        c = _lib.comfort_cfg()      # (l_max is -2551: l_min = -2000 lies above it)
        setattr(c, field, value)
        out.append(c)
    return out


def test_null_and_invalid_arguments_are_refused_before_any_gpu_use():
    lib = _lib_or_skip()
    one = (C.c_int32 * 1)(0)
    ok = _lib.comfort_cfg()
    off = _lib.ComfortCfg()
    fake = C.c_void_p(16)      # never dereferenced: the checks below come first

    def fill(ctx=fake, hop=320, cfg=ok, wav=fake, ld=1000, n=2, samples=1000, pos0=0, gl=fake, cl=fake, lvld=4, sg=FULL, sc=0, out=C.c_void_p(32), out_ld=1000):
        return lib.conan_comfort_fill(ctx, hop, C.byref(cfg) if cfg is not None else None, None, wav, ld, n, samples, pos0, gl, cl, lvld, sg, sc, out, out_ld, None)

    for kw in (dict(ctx=None), dict(cfg=None), dict(wav=None), dict(gl=None), dict(cl=None), dict(out=None)):
        assert fill(**kw) == _lib.ERR_INVALID
        assert b"null argument" in lib.conan_last_error()
    for kw in (dict(hop=0), dict(hop=4096), dict(n=0), dict(n=65536), dict(samples=0), dict(samples=2 ** 31), dict(ld=999), dict(out_ld=999),
               dict(ld=2 ** 31), dict(lvld=3), dict(sg=-1), dict(sg=FULL + 1), dict(sc=1), dict(sc=-16385), dict(pos0=-1), dict(cfg=off),
               dict(out=fake, out_ld=1001)):      # in place with another stride
        assert fill(**kw) == _lib.ERR_INVALID, kw

    def track(ctx=fake, cfg=ok, act=fake, power=fake, n=2, frames=10, ld=10, out=fake):
        return lib.conan_comfort_track(ctx, C.byref(cfg) if cfg is not None else None, act, power, n, frames, ld, out, None, None)

    for kw in (dict(ctx=None), dict(cfg=None), dict(act=None), dict(power=None), dict(out=None)):      # (ok follows: it needs the powers)
        assert track(**kw) == _lib.ERR_INVALID
        assert b"null argument" in lib.conan_last_error()
    for kw in (dict(n=0), dict(n=65536), dict(frames=0), dict(frames=2 ** 31), dict(ld=9), dict(ld=2 ** 31), dict(cfg=off)):
        assert track(**kw) == _lib.ERR_INVALID, kw
    assert lib.conan_streams_set_comfort(None, one, 1, C.byref(ok), None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_comfort(fake, None, 1, C.byref(ok), None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_comfort(fake, one, 1, None, None) == _lib.ERR_INVALID
    assert lib.conan_streams_comfort(None, 0, C.byref(ok)) == _lib.ERR_INVALID      # (host only: no device is touched either way)
    assert lib.conan_streams_comfort(fake, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_comfort_state(None, one, 1, fake, None) == _lib.ERR_INVALID
    assert lib.conan_streams_comfort_state(fake, None, 1, fake, None) == _lib.ERR_INVALID
    assert lib.conan_streams_comfort_state(fake, one, 1, None, None) == _lib.ERR_INVALID
    assert lib.conan_step_wav_comfort(None, fake, None) == _lib.ERR_INVALID
    assert lib.conan_step_wav_comfort(fake, None, None) == _lib.ERR_INVALID
    # every refused field of the cfg, before the handle is touched
    for c in bad_cfgs():
        assert lib.conan_streams_set_comfort(fake, one, 1, C.byref(c), None) == _lib.ERR_INVALID, lib.conan_last_error()
        assert fill(cfg=c) == _lib.ERR_INVALID and track(cfg=c) == _lib.ERR_INVALID


def _engine(n):
    from conan_amd.engine import StreamingVoiceConversionEngine as Engine
    eng = Engine.__new__(Engine)      # no context, no stream-set: the checks must come before either is touched
    eng.slots = list(range(n))
    return eng


def test_engine_comfort_values():
    from conan_amd.engine import StreamingVoiceConversionEngine as Engine
    got = Engine._values("comfort", [None, True, dict(level_db=-50.0, follow=False), False], 4)
    assert got == [None, {}, dict(level_db=-50.0, follow=False), None]
    assert Engine._values("comfort", dict(colour=2), 2) == [dict(colour=2)] * 2
    eng = _engine(2)
    calls = [lambda **kw: eng.start_wav(kw.pop("ref_mel"), **kw), lambda **kw: eng.open_slots([0, 1], kw.pop("ref_mel"), **kw),
             lambda **kw: eng.infer_wav(None, kw.pop("ref_mel"), **kw), lambda **kw: eng.infer_wav_staggered([None, None], [0, 1], kw.pop("ref_mel"), **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="3 values for 2"):
            call(ref_mel=object(), comfort=[True, True, True])
        with pytest.raises(ValueError, match="comfort: 'pink'"):
            call(ref_mel=object(), comfort="pink")
    # a stream-set that never used it is left alone: no setter call at all
    eng._used = set()
    eng.st = types.SimpleNamespace()      # (any attribute access would raise)
    eng._apply("comfort", eng.slots, [None, None])
    assert "comfort" not in eng._used
    # once used, None turns a slot off and a dict travels as the cfg, with a seed of the slot's own unless one is given
    seen = []
    eng.st = types.SimpleNamespace(set_comfort=lambda slots, cfg=True, **kw: seen.append((list(slots), cfg, kw)))
    eng._apply("comfort", [3, 4, 5], [dict(colour=0), None, dict(seed=9)])
    assert "comfort" in eng._used
    assert seen == [([3], dict(colour=0, seed=_lib.comfort_seed(3)), {}), ([4], None, {}), ([5], dict(seed=9), {})]
    eng.set_comfort([1], follow=False, level_db=-40.0)
    assert seen[-1] == ([1], True, dict(follow=False, level_db=-40.0))
