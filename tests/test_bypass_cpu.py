"""Source bypass without a GPU: the C surface (symbols, the 32-byte cfg, the 16-byte state and their ctypes mirrors, the header as C),
the order of the checks - every refused argument is refused before a handle is touched, so fake handles are never dereferenced - the
conversions of _lib.bypass_cfg and the engine's host logic for bypass=."""
import ctypes as C
import math
import os
import shutil
import subprocess
import types

import pytest

from conan_amd import _lib
from tests import bypass_ref as B

SYMBOLS = ["conan_streams_set_bypass", "conan_streams_bypass", "conan_streams_bypass_state", "conan_step_wav_bypass", "conan_bypass_mix"]
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
    assert C.sizeof(_lib.BypassCfg) == 32 and C.sizeof(_lib.BypassState) == 16
    assert _lib.ACTIVITY_FULL == FULL == B.FULL
    c = _lib.bypass_cfg()      # full wet, no dry, a 40 ms ramp, a restart begins at the targets
    assert (c.enabled, c.reseed, c.wet_target, c.dry_target, c.step, c.fill_gate, c.seed_wet, c.seed_dry) == (1, 0, FULL, 0, FULL // 2, 0, FULL, 0)
    # shares: rint(share * 2^20)
    c = _lib.bypass_cfg(wet=0.25, dry=0.7)
    assert (c.wet_target, c.dry_target, c.seed_wet, c.seed_dry) == (FULL // 4, int(round(0.7 * FULL)), FULL // 4, int(round(0.7 * FULL)))
    assert _lib.bypass_level(0.5 / FULL) == 0 and _lib.bypass_level(1.5 / FULL) == 2      # ties go to the even level
    # decibels, converted once on the host
    c = _lib.bypass_cfg(wet_db=-6.0, dry_db=-20.0)
    assert (c.wet_target, c.dry_target) == (int(round(FULL * 10.0 ** -0.3)), int(round(FULL * 0.1)))
    assert _lib.bypass_cfg(wet_db=0.0).wet_target == FULL
    # ramp_ms -> step = ceil(2^20 / max(1, ramp_ms / 20))
    for ramp, step in ((0.0, FULL), (10.0, FULL), (20.0, FULL), (40.0, FULL // 2), (60.0, math.ceil(FULL / 3)), (100.0, math.ceil(FULL / 5)),
                       (50.0, math.ceil(FULL / 2.5))):
        assert _lib.bypass_cfg(ramp_ms=ramp).step == step, ramp
        assert 1 <= step <= FULL
    assert _lib.bypass_cfg(step=77).step == 77
    c = _lib.bypass_cfg(wet=0.0, dry=1.0, start=(0, FULL), fill_gate=True, reseed=True)
    assert (c.wet_target, c.dry_target, c.seed_wet, c.seed_dry, c.fill_gate, c.reseed) == (0, FULL, 0, FULL, 1, 1)
    # the reported form gives the same bytes back
    c = _lib.bypass_cfg(wet=0.3, dry_db=-12.0, ramp_ms=70.0, fill_gate=True, start=(5, 1 << 19))
    kw = _lib.bypass_keywords(c)
    assert kw["start"] == (5, 1 << 19) and kw["fill_gate"] is True
    assert bytes(_lib.bypass_cfg(**kw)) == bytes(c)


def test_header_compiles_as_c_and_matches_the_mirror(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not present")
    inc = os.path.dirname(_lib.HEADER_PATH)
    fields = [f[0] for f in _lib.BypassCfg._fields_]
    sfields = [f[0] for f in _lib.BypassState._fields_]
    protos = tmp_path / "protos.c"
    protos.write_text('#include "conan_hip.h"\n'
                      'int (*a)(conan_streams*, const int32_t*, int, const conan_bypass_cfg*, void*) = conan_streams_set_bypass;\n'
                      'int (*b)(const conan_streams*, int, conan_bypass_cfg*) = conan_streams_bypass;\n'
                      'int (*c)(conan_streams*, const int32_t*, int, conan_bypass_state*, void*) = conan_streams_bypass_state;\n'
                      'int (*d)(conan_streams*, int32_t*, int32_t*, void*) = conan_step_wav_bypass;\n'
                      'int (*e)(conan_ctx*, int, const float*, int64_t, const float*, int64_t, int, int64_t, const int32_t*, const int32_t*, int64_t, '
                      'int32_t, int32_t, float*, int64_t, void*) = conan_bypass_mix;\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(protos), "-o", str(tmp_path / "protos.o")], check=True)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "conan_hip.h"\n'
                     'int main(void) {\n'
                     '  printf("%d %zu %zu", CONAN_HIP_ABI_VERSION, sizeof(conan_bypass_cfg), sizeof(conan_bypass_state));\n' +
                     "".join('  printf(" %%zu", offsetof(conan_bypass_cfg, %s));\n' % f for f in fields) +
                     "".join('  printf(" %%zu", offsetof(conan_bypass_state, %s));\n' % f for f in sfields) +
                     '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, str(probe), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [9, 32, 16] + [getattr(_lib.BypassCfg, f).offset for f in fields] + [getattr(_lib.BypassState, f).offset for f in sfields]


BAD = [("enabled", 2), ("enabled", -1), ("reseed", 2), ("reseed", -1), ("fill_gate", 2), ("fill_gate", -1), ("wet_target", -1),
       ("wet_target", FULL + 1), ("dry_target", -1), ("dry_target", FULL + 1), ("seed_wet", -1), ("seed_wet", FULL + 1), ("seed_dry", -1),
       ("seed_dry", FULL + 1), ("step", 0), ("step", -5), ("step", FULL + 1)]


def bad_cfgs():
    out = []
    for field, value in BAD:
        c = _lib.bypass_cfg()
        setattr(c, field, value)
        out.append(c)
    return out


def test_null_and_invalid_arguments_are_refused_before_any_gpu_use():
    lib = _lib_or_skip()
    one = (C.c_int32 * 1)(0)
    ok = _lib.bypass_cfg()
    fake = C.c_void_p(16)      # never dereferenced: the checks below come first

    def mix(ctx=fake, hop=320, wet=fake, wet_ld=1000, dry=fake, dry_ld=1000, n=2, samples=1000, wl=fake, dl=fake, lvld=4, sw=FULL, sd=0, out=fake,
            out_ld=1000):
        return lib.conan_bypass_mix(ctx, hop, wet, wet_ld, dry, dry_ld, n, samples, wl, dl, lvld, sw, sd, out, out_ld, None)

    for kw in (dict(ctx=None), dict(wet=None), dict(dry=None), dict(wl=None), dict(dl=None), dict(out=None)):
        assert mix(**kw) == _lib.ERR_INVALID
        assert b"null argument" in lib.conan_last_error()
    for kw in (dict(hop=0), dict(hop=4096), dict(n=0), dict(n=65536), dict(samples=0), dict(samples=2 ** 31), dict(wet_ld=999), dict(dry_ld=999),
               dict(out_ld=999), dict(wet_ld=2 ** 31), dict(lvld=3), dict(sw=-1), dict(sw=FULL + 1), dict(sd=-1), dict(sd=FULL + 1),
               dict(out=fake, wet=fake, out_ld=1001)):      # in place with another stride
        assert mix(**kw) == _lib.ERR_INVALID, kw
    assert lib.conan_streams_set_bypass(None, one, 1, C.byref(ok), None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_bypass(fake, None, 1, C.byref(ok), None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_bypass(fake, one, 1, None, None) == _lib.ERR_INVALID
    assert lib.conan_streams_bypass(None, 0, C.byref(ok)) == _lib.ERR_INVALID      # (host only: no device is touched either way)
    assert lib.conan_streams_bypass(fake, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_bypass_state(None, one, 1, fake, None) == _lib.ERR_INVALID
    assert lib.conan_streams_bypass_state(fake, None, 1, fake, None) == _lib.ERR_INVALID
    assert lib.conan_streams_bypass_state(fake, one, 1, None, None) == _lib.ERR_INVALID
    assert lib.conan_step_wav_bypass(None, fake, fake, None) == _lib.ERR_INVALID
    assert lib.conan_step_wav_bypass(fake, None, fake, None) == _lib.ERR_INVALID
    assert lib.conan_step_wav_bypass(fake, fake, None, None) == _lib.ERR_INVALID
    # every refused field of the cfg, before the handle is touched
    for c in bad_cfgs():
        assert lib.conan_streams_set_bypass(fake, one, 1, C.byref(c), None) == _lib.ERR_INVALID, lib.conan_last_error()


def _engine(n):
    from conan_amd.engine import StreamingVoiceConversionEngine as Engine
    eng = Engine.__new__(Engine)      # no context, no stream-set: the checks must come before either is touched
    eng.slots = list(range(n))
    return eng


def test_engine_bypass_values():
    from conan_amd.engine import StreamingVoiceConversionEngine as Engine
    got = Engine._values("bypass", [None, True, dict(wet=0.5, dry=0.5), False], 4)
    assert got == [None, {}, dict(wet=0.5, dry=0.5), None]
    assert Engine._values("bypass", dict(dry=0.1), 2) == [dict(dry=0.1)] * 2
    eng = _engine(2)
    calls = [lambda **kw: eng.start_wav(kw.pop("ref_mel"), **kw), lambda **kw: eng.open_slots([0, 1], kw.pop("ref_mel"), **kw),
             lambda **kw: eng.infer_wav(None, kw.pop("ref_mel"), **kw), lambda **kw: eng.infer_wav_staggered([None, None], [0, 1], kw.pop("ref_mel"), **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="3 values for 2"):
            call(ref_mel=object(), bypass=[True, True, True])
        with pytest.raises(ValueError, match="bypass: 'dry'"):
            call(ref_mel=object(), bypass="dry")
    # a stream-set that never used it is left alone: no setter call at all
    eng._used = set()
    eng.st = types.SimpleNamespace()      # (any attribute access would raise)
    eng._apply("bypass", eng.slots, [None, None])
    assert "bypass" not in eng._used
    # once used, None turns a slot off and a dict travels as the cfg
    seen = []
    eng.st = types.SimpleNamespace(set_bypass=lambda slots, cfg=True, **kw: seen.append((list(slots), cfg, kw)))
    eng._apply("bypass", eng.slots, [dict(dry=0.2), None])
    assert "bypass" in eng._used and seen == [([0], dict(dry=0.2), {}), ([1], None, {})]
    eng.set_bypass([1], wet=0.0, dry=1.0)
    assert seen[-1] == ([1], True, dict(wet=0.0, dry=1.0))
