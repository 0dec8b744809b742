"""Register matching without a GPU: the C surface (symbols, the 32-byte cfg and its ctypes mirror, the header as C), the order of the
checks - every refused argument is refused before a handle is touched, so fake handles are never dereferenced - and the engine's host
logic for register=."""
import ctypes as C
import os
import shutil
import subprocess
import types

import pytest

from conan_amd import _lib
from tests import register_ref as G

SYMBOLS = ["conan_f0_register", "conan_streams_set_pitch_register", "conan_streams_pitch_register", "conan_streams_pitch_register_state"]


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


def test_cfg_mirror_and_helpers():
    assert C.sizeof(_lib.RegisterCfg) == 32
    c = _lib.register_cfg(7.75)
    assert (c.enabled, c.reseed, c.target, c.max_shift) == (1, 0, 7.75, 2.0)
    assert (c.seed_count, c.seed_sum) == G.prior_seed(7.75) == (50, 50 * 7.75 * 2 ** 22)      # the prior: one second at the target
    c = _lib.register_cfg(7.3, max_shift=1.0, prior=6.1, prior_frames=20, reseed=True)
    assert (c.reseed, c.seed_count, c.seed_sum) == (1,) + G.prior_seed(6.1, 20)
    assert _lib.register_quantise(6.1) == G.quantise(6.1)
    c = _lib.register_cfg(7.0, seed=(123, 123 * 29360128))
    assert (c.seed_count, c.seed_sum) == (123, 123 * 29360128)
    assert _lib.register_keywords(c) == dict(target=7.0, max_shift=2.0, seed=(123, 123 * 29360128))
    back = _lib.register_cfg(**_lib.register_keywords(c))
    assert bytes(back) == bytes(c)
    with pytest.raises(ValueError):
        _lib.register_cfg(None)


def test_header_compiles_as_c_and_matches_the_mirror(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not present")
    inc = os.path.dirname(_lib.HEADER_PATH)
    fields = [f[0] for f in _lib.RegisterCfg._fields_]
    protos = tmp_path / "protos.c"
    protos.write_text('#include "conan_hip.h"\n'
                      'int (*a)(conan_ctx*, const conan_register_cfg*, const float*, const float*, int, const int32_t*, int64_t, float*, int64_t*, void*) = conan_f0_register;\n'
                      'int (*b)(conan_streams*, const int32_t*, int, const conan_register_cfg*, void*) = conan_streams_set_pitch_register;\n'
                      'int (*c)(const conan_streams*, int, conan_register_cfg*) = conan_streams_pitch_register;\n'
                      'int (*d)(conan_streams*, const int32_t*, int, int64_t*, void*) = conan_streams_pitch_register_state;\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(protos), "-o", str(tmp_path / "protos.o")], check=True)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "conan_hip.h"\n'
                     'int main(void) {\n'
                     '  printf("%d %zu", CONAN_HIP_ABI_VERSION, sizeof(conan_register_cfg));\n' +
                     "".join('  printf(" %%zu", offsetof(conan_register_cfg, %s));\n' % f for f in fields) +
                     '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, str(probe), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [9, 32] + [getattr(_lib.RegisterCfg, f).offset for f in fields]


def test_null_and_invalid_arguments_are_refused_before_any_gpu_use():
    lib = _lib_or_skip()
    one = (C.c_int32 * 1)(0)
    frames = (C.c_int32 * 2)(10, 10)
    ok = _lib.register_cfg(7.5)
    fake = C.c_void_p(16)      # never dereferenced: the checks below come first

    def whole(ctx=fake, c=ok, f0=fake, uv=fake, n=2, fr=frames, ld=10, out=fake, state=fake):
        return lib.conan_f0_register(ctx, C.byref(c) if c is not None else None, f0, uv, n, fr, ld, out, state, None)

    for kw in (dict(ctx=None), dict(c=None), dict(f0=None), dict(uv=None), dict(fr=None)):
        assert whole(**kw) == _lib.ERR_INVALID
        assert b"null argument" in lib.conan_last_error()
    assert lib.conan_streams_set_pitch_register(None, one, 1, C.byref(ok), None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_pitch_register(fake, None, 1, C.byref(ok), None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_pitch_register(fake, one, 1, None, None) == _lib.ERR_INVALID
    assert lib.conan_streams_pitch_register(None, 0, C.byref(ok)) == _lib.ERR_INVALID      # (host only: no device is touched either way)
    assert lib.conan_streams_pitch_register(fake, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_pitch_register_state(None, one, 1, fake, None) == _lib.ERR_INVALID
    assert lib.conan_streams_pitch_register_state(fake, None, 1, fake, None) == _lib.ERR_INVALID
    assert lib.conan_streams_pitch_register_state(fake, one, 1, None, None) == _lib.ERR_INVALID
    # every refused field of the cfg, by both entry points, before the handle is touched
    inf, nan = float("inf"), float("nan")
    cfgs = []
    for field, value in (("enabled", 2), ("enabled", -1), ("reseed", 2), ("reseed", -1), ("target", nan), ("target", inf), ("target", -inf),
                         ("max_shift", -0.5), ("max_shift", nan), ("max_shift", inf), ("seed_count", -1), ("seed_count", 2 ** 34 + 1)):
        c = _lib.register_cfg(7.5)
        setattr(c, field, value)
        cfgs.append(c)
    for seed in ((0, 1), (0, -1), (10, 10 * 2 ** 28 + 1), (10, -10 * 2 ** 28 - 1)):      # |seed_sum| <= seed_count * 2^28
        cfgs.append(_lib.register_cfg(7.5, seed=seed))
    for c in cfgs:
        assert whole(c=c) == _lib.ERR_INVALID, lib.conan_last_error()
        assert lib.conan_streams_set_pitch_register(fake, one, 1, C.byref(c), None) == _lib.ERR_INVALID
    # conan_f0_register's own arguments: an enabled cfg, the row count, the stride and the rows' frames
    assert whole(c=_lib.RegisterCfg()) == _lib.ERR_INVALID and b"enabled" in lib.conan_last_error()
    assert whole(n=0) == _lib.ERR_INVALID and whole(n=65536) == _lib.ERR_INVALID and whole(n=-3) == _lib.ERR_INVALID
    assert whole(ld=-1) == _lib.ERR_INVALID and whole(ld=2 ** 31) == _lib.ERR_INVALID
    assert whole(ld=9) == _lib.ERR_INVALID and b"frames" in lib.conan_last_error()      # a row longer than the stride
    assert whole(fr=(C.c_int32 * 2)(3, -1)) == _lib.ERR_INVALID


class _Bank:
    registers = {0: 7.5, 2: 8.25}


def _engine(n):
    from conan_amd.engine import StreamingVoiceConversionEngine as Engine
    eng = Engine.__new__(Engine)      # no context, no stream-set: the checks must come before either is touched
    eng.slots = list(range(n))
    return eng


def test_engine_register_voice_needs_a_voice_with_a_register():
    eng = _engine(2)
    bank = _Bank()
    calls = [lambda **kw: eng.start_wav(kw.pop("ref_mel"), **kw), lambda **kw: eng.open_slots([0, 1], kw.pop("ref_mel"), **kw),
             lambda **kw: eng.infer_wav(None, kw.pop("ref_mel"), **kw), lambda **kw: eng.infer_wav_staggered([None, None], [0, 1], kw.pop("ref_mel"), **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="needs voice="):
            call(ref_mel=object(), follow=True, register="voice")
        with pytest.raises(ValueError, match="voice 1 has no register"):
            call(ref_mel=None, voice=(bank, [0, 1]), follow=True, register="voice")
        with pytest.raises(ValueError, match="voice 1 has no register"):
            call(ref_mel=None, voice=(bank, [0, 1]), follow=True, register=[7.0, "voice"])
        with pytest.raises(ValueError, match="3 values for 2"):
            call(ref_mel=object(), follow=True, register=[7.0, 7.0, 7.0])
        with pytest.raises(ValueError, match="'nearest'"):
            call(ref_mel=object(), follow=True, register="nearest")


def test_engine_register_values():
    from conan_amd.engine import StreamingVoiceConversionEngine as Engine
    bank = _Bank()
    got = Engine._values("register", [None, 7.25, "voice", dict(target=6.0, max_shift=0.5)], 4, voice=(bank, [0, 0, 2, 0]))
    assert got == [None, dict(target=7.25), dict(target=8.25), dict(target=6.0, max_shift=0.5)]
    assert Engine._values("register", False, 2) == [None, None]
    assert Engine._values("register", "voice", 2, voice=(bank, [2, 0])) == [dict(target=8.25), dict(target=7.5)]
    # a stream-set that never used it is left alone: no setter call at all
    eng = _engine(2)
    eng._used = set()
    eng.st = types.SimpleNamespace()      # (any attribute access would raise)
    eng._apply("register", eng.slots, [None, None])
    assert "register" not in eng._used
