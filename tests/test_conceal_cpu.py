"""Input loss concealment without a GPU: the C surface (the six symbols, the 32-byte cfg and its ctypes mirror, the header as C), the
order of the checks - every refused argument is refused before a handle is touched, so fake handles are never dereferenced - the
defaults of _lib.conceal_keywords and the engine's host logic for conceal= and lost=."""
import ctypes as C
import os
import shutil
import subprocess
import types

import pytest

from conan_amd import _lib
from tests import conceal_ref as R

SYMBOLS = ["conan_streams_set_conceal", "conan_streams_conceal_cfg", "conan_streams_conceal", "conan_conceal_state_bytes",
           "conan_streams_conceal_state", "conan_conceal"]
STATE_BYTES = 32 + 4 * 1024 + 4 * 2048      # header, template, history


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
    raw.conan_conceal_state_bytes.restype = C.c_int64
    assert raw.conan_conceal_state_bytes() == STATE_BYTES


def test_cfg_mirror_and_defaults():
    assert C.sizeof(_lib.ConcealCfg) == 32
    assert (_lib.CONCEAL_MAX_LAG, _lib.CONCEAL_MAX_WINDOW) == (R.MAX_LAG, R.MAX_WINDOW) == (1024, 1024)
    for rate in (8000, 16000, 22050, 44100, 48000):
        kw = _lib.conceal_keywords(rate)
        assert kw == R.defaults(rate)
        c = _lib.conceal_cfg(rate)
        assert c.enabled == 1 and _lib.conceal_keywords(c) == kw
        assert 1 <= c.lag_min <= c.lag_max <= 1024 and 1 <= c.window <= 1024 and 0 <= c.fade <= 1024
    c = _lib.conceal_cfg(16000, hold=5, fade=0)
    assert (c.packet, c.lag_min, c.lag_max, c.window, c.hold, c.fall, c.fade) == (320, 40, 240, 320, 5, 800, 0)
    assert bytes(_lib.conceal_cfg(**_lib.conceal_keywords(c))) == bytes(c)      # the reported form gives the same bytes back
    with pytest.raises(ValueError, match="unknown"):
        _lib.conceal_cfg(16000, lag=3)
    with pytest.raises(ValueError, match="without a rate"):
        _lib.conceal_cfg(packet=16)


def test_header_compiles_as_c_and_matches_the_mirror(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not present")
    inc = os.path.dirname(_lib.HEADER_PATH)
    fields = [f[0] for f in _lib.ConcealCfg._fields_]
    protos = tmp_path / "protos.c"
    protos.write_text('#include "conan_hip.h"\n'
                      'int (*a)(conan_streams*, const int32_t*, int, const conan_conceal_cfg*, const void*, int64_t, void*) = conan_streams_set_conceal;\n'
                      'int (*b)(const conan_streams*, int, conan_conceal_cfg*) = conan_streams_conceal_cfg;\n'
                      'int (*c)(conan_streams*, const int32_t*, int, const int32_t*, void*, int64_t, const int32_t*, int64_t, void*) = conan_streams_conceal;\n'
                      'int64_t (*d)(void) = conan_conceal_state_bytes;\n'
                      'int (*e)(conan_streams*, const int32_t*, int, void*, int64_t, void*) = conan_streams_conceal_state;\n'
                      'int (*f)(conan_ctx*, const conan_conceal_cfg*, int, void*, int64_t, int, const int64_t*, const int32_t*, int64_t, void*) = conan_conceal;\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(protos), "-o", str(tmp_path / "protos.o")], check=True)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "conan_hip.h"\n'
                     'int main(void) {\n'
                     '  printf("%d %zu %d %d", CONAN_HIP_ABI_VERSION, sizeof(conan_conceal_cfg), CONAN_CONCEAL_MAX_LAG, CONAN_CONCEAL_MAX_WINDOW);\n' +
                     "".join('  printf(" %%zu", offsetof(conan_conceal_cfg, %s));\n' % f for f in fields) +
                     '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, str(probe), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [9, 32, 1024, 1024] + [getattr(_lib.ConcealCfg, f).offset for f in fields]


BAD = [("enabled", 2), ("enabled", -1), ("packet", 0), ("packet", -3), ("lag_min", 0), ("lag_min", -1), ("lag_min", 25), ("lag_max", 1025),
       ("lag_max", 3), ("window", 0), ("window", 1025), ("hold", -1), ("fall", 0), ("fall", -2), ("fade", -1), ("fade", 1025)]


def bad_cfgs():
    out = []
    for field, value in BAD:
        c = _lib.conceal_cfg(packet=16, lag_min=4, lag_max=24, window=32, hold=8, fall=16, fade=8)
        setattr(c, field, value)
        out.append(c)
    return out


def test_null_and_invalid_arguments_are_refused_before_any_gpu_use():
    lib = _lib_or_skip()
    one = (C.c_int32 * 1)(0)
    n64 = (C.c_int64 * 2)(100, 100)
    ok = _lib.conceal_cfg(16000)
    off = _lib.ConcealCfg()
    fake = C.c_void_p(16)      # never dereferenced: the checks below come first

    def whole(ctx=fake, cfg=ok, fmt=_lib.SAMPLE_F32, x=fake, ld=100, n=2, samples=n64, lost=fake, lost_ld=1):
        return lib.conan_conceal(ctx, None if cfg is None else C.byref(cfg), fmt, x, ld, n, samples, lost, lost_ld, None)

    for kw in (dict(ctx=None), dict(cfg=None), dict(x=None), dict(samples=None), dict(lost=None)):
        assert whole(**kw) == _lib.ERR_INVALID
        assert b"null argument" in lib.conan_last_error()
    for kw in (dict(cfg=off), dict(fmt=4), dict(fmt=-1), dict(n=0), dict(n=65536), dict(ld=99), dict(ld=-1), dict(lost_ld=0), dict(x=C.c_void_p(18)),
               dict(samples=(C.c_int64 * 2)(100, -1)), dict(fmt=_lib.SAMPLE_S16, ld=49), dict(samples=(C.c_int64 * 2)(100, 321), ld=400)):
        assert whole(**kw) == _lib.ERR_INVALID, kw
    for c in bad_cfgs():
        assert whole(cfg=c) == _lib.ERR_INVALID, lib.conan_last_error()
        assert lib.conan_streams_set_conceal(fake, one, 1, C.byref(c), None, 0, None) == _lib.ERR_INVALID, lib.conan_last_error()
    assert lib.conan_streams_set_conceal(None, one, 1, C.byref(ok), None, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_conceal(fake, None, 1, C.byref(ok), None, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_conceal(fake, one, 1, None, None, 0, None) == _lib.ERR_INVALID
    # a seed that is misaligned, or whose rows are closer than a record
    assert lib.conan_streams_set_conceal(fake, one, 1, C.byref(ok), C.c_void_p(20), STATE_BYTES, None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_conceal(fake, one, 1, C.byref(ok), C.c_void_p(64), STATE_BYTES - 8, None) == _lib.ERR_INVALID
    assert lib.conan_streams_conceal_cfg(None, 0, C.byref(off)) == _lib.ERR_INVALID      # (host only)
    assert lib.conan_streams_conceal_cfg(fake, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_conceal(None, one, 1, one, fake, 100, fake, 1, None) == _lib.ERR_INVALID
    assert lib.conan_streams_conceal(fake, None, 1, one, fake, 100, fake, 1, None) == _lib.ERR_INVALID
    assert lib.conan_streams_conceal(fake, one, 1, None, fake, 100, fake, 1, None) == _lib.ERR_INVALID
    assert lib.conan_streams_conceal_state(None, one, 1, fake, STATE_BYTES, None) == _lib.ERR_INVALID
    assert lib.conan_streams_conceal_state(fake, None, 1, fake, STATE_BYTES, None) == _lib.ERR_INVALID
    assert lib.conan_streams_conceal_state(fake, one, 1, None, STATE_BYTES, None) == _lib.ERR_INVALID
    assert lib.conan_streams_conceal_state(fake, one, 1, fake, STATE_BYTES - 8, None) == _lib.ERR_INVALID


def _engine(n):
    from conan_amd.engine import StreamingVoiceConversionEngine as Engine
    eng = Engine.__new__(Engine)      # no context, no stream-set: the checks must come before either is touched
    eng.slots = list(range(n))
    return eng


def test_engine_conceal_values():
    from conan_amd.engine import StreamingVoiceConversionEngine as Engine
    cfg = _lib.conceal_cfg(8000)
    got = Engine._values("conceal", [None, True, dict(fade=0), False, cfg], 5)
    assert got == [None, {}, dict(fade=0), None, cfg]
    assert Engine._values("conceal", dict(hold=3), 2) == [dict(hold=3)] * 2
    eng = _engine(2)
    calls = [lambda **kw: eng.start_wav(kw.pop("ref_mel"), **kw), lambda **kw: eng.open_slots([0, 1], kw.pop("ref_mel"), **kw),
             lambda **kw: eng.infer_wav(None, kw.pop("ref_mel"), **kw), lambda **kw: eng.infer_wav_staggered([None, None], [0, 1], kw.pop("ref_mel"), **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="3 values for 2"):
            call(ref_mel=object(), conceal=[True, True, True])
        with pytest.raises(ValueError, match="conceal: 'on'"):
            call(ref_mel=object(), conceal="on")
    # lost= holds the utterance in pieces: not with the paths that hold it whole, and not without conceal=
    for call in calls[2:]:
        for kw in (dict(loud_norm=True), dict(trim=True), dict(trim=dict(smooth_frames=3))):
            with pytest.raises(ValueError, match="Context.conceal"):
                call(ref_mel=object(), conceal=True, lost=[object(), object()], **kw)
        with pytest.raises(ValueError, match="need conceal="):
            call(ref_mel=object(), lost=[object(), object()])
    # a stream-set that never used it is left alone: no setter call at all
    eng._used = set()
    eng.st = types.SimpleNamespace()      # (any attribute access would raise)
    eng._apply("conceal", eng.slots, [None, None], [None, None])
    assert "conceal" not in eng._used
    # once used, None turns a slot off, a dict travels as the cfg and True stands for the rate's defaults
    seen = []
    eng.st = types.SimpleNamespace(set_conceal=lambda slots, cfg=True, **kw: seen.append((list(slots), cfg, kw)))
    eng._apply("conceal", eng.slots, [dict(fade=0), None], [8000, None])
    assert "conceal" in eng._used and seen == [([0], dict(fade=0), dict(rate=8000)), ([1], None, dict(rate=None))]
    eng._apply("conceal", eng.slots, [{}, cfg], [48000, None])
    assert seen[2:] == [([0], True, dict(rate=48000)), ([1], cfg, dict(rate=None))]
    eng.set_conceal([1], hold=0)
    assert seen[-1] == ([1], True, dict(hold=0))
