"""Echo cancellation without a GPU: the C surface (the six symbols, the 48-byte cfg and its ctypes mirror, the header as C), the order of
the checks - every refused argument is refused before a handle is touched, so fake handles are never dereferenced - the defaults of
_lib.echo_keywords, the feature table's row and the engine's host logic for echo= and far=."""
import ctypes as C
import os
import shutil
import subprocess
import types

import pytest

from conan_amd import _lib
from tests import echo_ref as R

SYMBOLS = ["conan_streams_set_echo", "conan_streams_echo_cfg", "conan_streams_echo", "conan_echo_state_bytes", "conan_streams_echo_state", "conan_echo"]
STATE_BYTES = 64 + 4 * 2048 + 4 * 64 + 2 * 6208      # header, weights, pending e, far history


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    return _lib.lib()


def test_symbols_exported():
    for name in SYMBOLS:
        assert name in _lib.declared_symbols() and name in _lib._PROTOS, name
    _lib_or_skip()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), name
    assert raw.conan_abi_version() == 9      # (the feature is detected by symbol: no struct changed)
    raw.conan_echo_state_bytes.restype = C.c_int64
    assert raw.conan_echo_state_bytes() == STATE_BYTES == R.STATE_BYTES


def test_cfg_mirror_and_defaults():
    assert C.sizeof(_lib.EchoCfg) == 48
    assert (_lib.ECHO_BLOCK, _lib.ECHO_MAX_TAPS, _lib.ECHO_MAX_DELAY, _lib.ECHO_MAX_SHIFT, _lib.ECHO_HISTORY) == (R.BLOCK, R.MAX_TAPS, R.MAX_DELAY, R.MAX_SHIFT, R.HIST)
    assert (R.BLOCK, R.MAX_TAPS, R.MAX_DELAY, R.MAX_SHIFT) == (64, 2048, 4096, 12)
    for rate, taps in ((8000, 512), (16000, 1024), (22050, 1408), (44100, 2048), (48000, 2048)):
        kw = _lib.echo_keywords(rate)
        assert kw == R.defaults(rate) and kw["taps"] == taps
        assert (kw["delay"], kw["mu_shift"], kw["dt_num"], kw["dt_den"], kw["reg"], kw["far_min"]) == (0, 4, 1, 2, taps * 4096, taps * 1024)
        assert (kw["hang"] - 1) * 64 < rate // 20 <= kw["hang"] * 64      # 50 ms in blocks, rounded up
        c = _lib.echo_cfg(rate)
        assert c.enabled == 1 and c.reserved == 0 and _lib.echo_keywords(c) == kw
    c = _lib.echo_cfg(16000, taps=256, delay=17, reg=1 << 40)
    assert (c.taps, c.delay, c.mu_shift, c.dt_num, c.dt_den, c.hang, c.reg, c.far_min) == (256, 17, 4, 1, 2, 13, 1 << 40, 1024 * 1024)
    assert bytes(_lib.echo_cfg(**_lib.echo_keywords(c))) == bytes(c)      # the reported form gives the same bytes back
    with pytest.raises(ValueError, match="unknown"):
        _lib.echo_cfg(16000, step=3)
    with pytest.raises(ValueError, match="without a rate"):
        _lib.echo_cfg(taps=64)


def test_feature_table_row():
    f = _lib.SLOT_FEATURES["echo"]
    assert (f.noun, f.cfg, f.on, f.build, f.keywords) == ("the echo canceller", _lib.EchoCfg, "enabled", _lib.echo_cfg, _lib.echo_keywords)
    assert (f.setter, f.getter, f.seed_state, f.seed_bytes) == ("conan_streams_set_echo", "conan_streams_echo_cfg", "conan_streams_echo_state", "conan_echo_state_bytes")
    assert f.method == "set_echo" and f.state is None and f.last is None and f.meta is None and f.stream and f.release and f.mirror is None
    names = list(_lib.SLOT_FEATURES)
    assert names.index("echo") == names.index("conceal") + 1 == names.index("denoise") - 1      # directly behind the concealment
    v = C.c_void_p
    assert _lib._PROTOS["conan_streams_set_echo"] == (C.c_int, [v, v, C.c_int, v, v, C.c_int64, v])
    assert _lib._PROTOS["conan_streams_echo_cfg"] == (C.c_int, [v, C.c_int, v])
    assert _lib._PROTOS["conan_streams_echo_state"] == (C.c_int, [v, v, C.c_int, v, C.c_int64, v])
    assert _lib._PROTOS["conan_streams_echo"] == (C.c_int, [v, v, C.c_int, v, v, C.c_int64, v, C.c_int64, v, v])
    assert _lib._PROTOS["conan_echo"] == (C.c_int, [v, v, C.c_int, v, C.c_int64, v, C.c_int64, C.c_int, v, v, v])
    assert _lib._PROTOS["conan_echo_state_bytes"] == (C.c_int64, [])


def test_header_compiles_as_c_and_matches_the_mirror(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not present")
    inc = os.path.dirname(_lib.HEADER_PATH)
    fields = [f[0] for f in _lib.EchoCfg._fields_]
    protos = tmp_path / "protos.c"
    protos.write_text('#include "conan_hip.h"\n'
                      'int (*a)(conan_streams*, const int32_t*, int, const conan_echo_cfg*, const void*, int64_t, void*) = conan_streams_set_echo;\n'
                      'int (*b)(const conan_streams*, int, conan_echo_cfg*) = conan_streams_echo_cfg;\n'
                      'int (*c)(conan_streams*, const int32_t*, int, const int32_t*, void*, int64_t, const void*, int64_t, int64_t*, void*) = conan_streams_echo;\n'
                      'int64_t (*d)(void) = conan_echo_state_bytes;\n'
                      'int (*e)(conan_streams*, const int32_t*, int, void*, int64_t, void*) = conan_streams_echo_state;\n'
                      'int (*f)(conan_ctx*, const conan_echo_cfg*, int, void*, int64_t, const void*, int64_t, int, const int64_t*, int64_t*, void*) = conan_echo;\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(protos), "-o", str(tmp_path / "protos.o")], check=True)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "conan_hip.h"\n'
                     'int main(void) {\n'
                     '  printf("%d %zu %d %d %d %d %d", CONAN_HIP_ABI_VERSION, sizeof(conan_echo_cfg), CONAN_ECHO_BLOCK, CONAN_ECHO_MAX_TAPS, CONAN_ECHO_MAX_DELAY,\n'
                     '         CONAN_ECHO_MAX_SHIFT, CONAN_ECHO_HISTORY);\n' +
                     "".join('  printf(" %%zu", offsetof(conan_echo_cfg, %s));\n' % f for f in fields) +
                     '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, str(probe), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [9, 48, 64, 2048, 4096, 12, 6208] + [getattr(_lib.EchoCfg, f).offset for f in fields]


# every bound of the cfg: the issue's cases first
BAD = [("taps", 0), ("taps", 65), ("taps", 2112), ("delay", 4097), ("mu_shift", 13), ("reg", 0),
       ("enabled", 2), ("enabled", -1), ("taps", -64), ("taps", 32), ("delay", -1), ("mu_shift", -1), ("dt_num", -1), ("dt_den", -1), ("hang", -1),
       ("reg", -5), ("reg", (1 << 60) + 1), ("far_min", -1)]


def bad_cfgs():
    out = []
    for field, value in BAD:
        c = _lib.echo_cfg(16000)
        setattr(c, field, value)
        out.append(c)
    return out


def test_null_and_invalid_arguments_are_refused_before_any_gpu_use():
    lib = _lib_or_skip()
    one = (C.c_int32 * 1)(0)
    n64 = (C.c_int64 * 2)(100, 100)
    ok = _lib.echo_cfg(16000)
    off = _lib.EchoCfg()
    fake = C.c_void_p(16)      # never dereferenced: the checks below come first

    def whole(ctx=fake, cfg=ok, fmt=_lib.SAMPLE_F32, x=fake, ld=100, far=fake, far_ld=100, n=2, samples=n64, stats=None):
        return lib.conan_echo(ctx, None if cfg is None else C.byref(cfg), fmt, x, ld, far, far_ld, n, samples, stats, None)

    for kw in (dict(ctx=None), dict(cfg=None), dict(x=None), dict(far=None), dict(samples=None)):
        assert whole(**kw) == _lib.ERR_INVALID
        assert b"null argument" in lib.conan_last_error()
    for kw in (dict(cfg=off), dict(fmt=4), dict(fmt=-1), dict(n=0), dict(n=65536), dict(ld=99), dict(far_ld=99), dict(ld=-1), dict(far_ld=-1),
               dict(x=C.c_void_p(18)), dict(far=C.c_void_p(18)), dict(stats=C.c_void_p(20)), dict(samples=(C.c_int64 * 2)(100, -1)),
               dict(fmt=_lib.SAMPLE_S16, ld=49), dict(samples=(C.c_int64 * 2)(100, 401), ld=400, far_ld=400)):
        assert whole(**kw) == _lib.ERR_INVALID, kw
    for c in bad_cfgs():
        assert whole(cfg=c) == _lib.ERR_INVALID, lib.conan_last_error()
        assert lib.conan_streams_set_echo(fake, one, 1, C.byref(c), None, 0, None) == _lib.ERR_INVALID, lib.conan_last_error()
    assert lib.conan_streams_set_echo(None, one, 1, C.byref(ok), None, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_echo(fake, None, 1, C.byref(ok), None, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_echo(fake, one, 1, None, None, 0, None) == _lib.ERR_INVALID
    # a seed that is misaligned, or whose rows are closer than a record
    assert lib.conan_streams_set_echo(fake, one, 1, C.byref(ok), C.c_void_p(20), STATE_BYTES, None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_echo(fake, one, 1, C.byref(ok), C.c_void_p(64), STATE_BYTES - 8, None) == _lib.ERR_INVALID
    assert lib.conan_streams_echo_cfg(None, 0, C.byref(off)) == _lib.ERR_INVALID      # (host only)
    assert lib.conan_streams_echo_cfg(fake, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_echo(None, one, 1, one, fake, 100, fake, 100, None, None) == _lib.ERR_INVALID
    assert lib.conan_streams_echo(fake, None, 1, one, fake, 100, fake, 100, None, None) == _lib.ERR_INVALID
    assert lib.conan_streams_echo(fake, one, 1, None, fake, 100, fake, 100, None, None) == _lib.ERR_INVALID
    assert lib.conan_streams_echo_state(None, one, 1, fake, STATE_BYTES, None) == _lib.ERR_INVALID
    assert lib.conan_streams_echo_state(fake, None, 1, fake, STATE_BYTES, None) == _lib.ERR_INVALID
    assert lib.conan_streams_echo_state(fake, one, 1, None, STATE_BYTES, None) == _lib.ERR_INVALID
    assert lib.conan_streams_echo_state(fake, one, 1, fake, STATE_BYTES - 8, None) == _lib.ERR_INVALID


def _engine(n):
    from conan_amd.engine import StreamingVoiceConversionEngine as Engine
    eng = Engine.__new__(Engine)      # no context, no stream-set: the checks must come before either is touched
    eng.slots = list(range(n))
    return eng


def test_engine_echo_values():
    from conan_amd.engine import StreamingVoiceConversionEngine as Engine
    cfg = _lib.echo_cfg(8000)
    got = Engine._values("echo", [None, True, dict(taps=128), False, cfg], 5)
    assert got == [None, {}, dict(taps=128), None, cfg]
    eng = _engine(2)
    calls = [lambda **kw: eng.start_wav(kw.pop("ref_mel"), **kw), lambda **kw: eng.open_slots([0, 1], kw.pop("ref_mel"), **kw),
             lambda **kw: eng.infer_wav(None, kw.pop("ref_mel"), **kw), lambda **kw: eng.infer_wav_staggered([None, None], [0, 1], kw.pop("ref_mel"), **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="3 values for 2"):
            call(ref_mel=object(), echo=[True, True, True])
        with pytest.raises(ValueError, match="echo: 'on'"):
            call(ref_mel=object(), echo="on")
    # far= holds the utterance in pieces: not with the paths that hold it whole, and not without echo=
    for call in calls[2:]:
        for kw in (dict(loud_norm=True), dict(trim=True), dict(trim=dict(smooth_frames=3))):
            with pytest.raises(ValueError, match="Context.echo"):
                call(ref_mel=object(), echo=True, far=[object(), object()], **kw)
        with pytest.raises(ValueError, match="needs echo="):
            call(ref_mel=object(), far=[object(), object()])
    # a stream-set that never used it is left alone: no setter call at all
    eng._used = set()
    eng.st = types.SimpleNamespace()      # (any attribute access would raise)
    eng._apply("echo", eng.slots, [None, None], [None, None])
    assert "echo" not in eng._used
    # once used, None turns a slot off, a dict travels as the cfg and True stands for the rate's defaults
    seen = []
    eng.st = types.SimpleNamespace(set_echo=lambda slots, cfg=True, **kw: seen.append((list(slots), cfg, kw)))
    eng._apply("echo", eng.slots, [dict(taps=128), None], [8000, None])
    assert "echo" in eng._used and seen == [([0], dict(taps=128), dict(rate=8000)), ([1], None, dict(rate=None))]
    eng._apply("echo", eng.slots, [{}, cfg], [48000, None])
    assert seen[2:] == [([0], True, dict(rate=48000)), ([1], cfg, dict(rate=None))]
    eng.set_echo([1], mu_shift=6)
    assert seen[-1] == ([1], True, dict(mu_shift=6))
