"""Input noise suppression without a GPU: the C surface (symbols, the 64-byte cfg, the 2064-byte state and their ctypes mirrors, the
header as C), the order of the checks - every refused argument is refused before a handle is touched, so fake handles are never
dereferenced - the conversions of _lib.denoise_cfg, the feature-table row, and the Python layer over the stand-ins of
tests/test_slot_features_cpu.py: what Streams and the engine hand the setter."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conan_amd import _lib
from tests.test_slot_features_cpu import H, STREAM, Seed, _engine, st  # noqa: F401  (st: the Streams over a recording library)

SYMBOLS = ["conan_mel_denoise", "conan_streams_set_denoise", "conan_streams_denoise", "conan_denoise_state_bytes", "conan_streams_denoise_state"]
FULL = 1 << 20
# (field, refused value); ("reserved", i): word i non-zero
BAD = [("enabled", 2), ("enabled", -1), ("reseed", 2), ("reseed", -1), ("bias", -1), ("bias", FULL + 1), ("knee", -1), ("knee", FULL + 1), ("slope", -1),
       ("slope", 65537), ("depth", 0), ("depth", FULL + 1), ("close_step", 0), ("close_step", FULL + 1), ("open_step", 0), ("open_step", -5),
       ("open_step", FULL + 1), ("rise", -1), ("rise", FULL + 1), ("fall_shift", -1), ("fall_shift", 9), ("floor_min", -FULL - 1), ("floor_min", FULL + 1),
       ("smooth", 2), ("smooth", -1), ("out_floor", float("inf")), ("out_floor", float("-inf")), ("out_floor", float("nan")), ("reserved", 0),
       ("reserved", 1), ("reserved", 2)]


def bad_cfgs():
    out = []
    for field, value in BAD:
        c = _lib.denoise_cfg()
        if field == "reserved":
            c.reserved[value] = 1
        else:
            setattr(c, field, value)
        out.append(c)
    return out


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
    raw.conan_denoise_state_bytes.restype = C.c_int64
    assert raw.conan_denoise_state_bytes() == 2064 == C.sizeof(_lib.DenoiseState)


def test_header_compiles_as_c_and_matches_the_mirror(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not present")
    inc = os.path.dirname(_lib.HEADER_PATH)
    fields = [f[0] for f in _lib.DenoiseCfg._fields_]
    sfields = [f[0] for f in _lib.DenoiseState._fields_]
    protos = tmp_path / "protos.c"
    protos.write_text('#include "conan_hip.h"\n'
                      'int (*a)(conan_ctx*, const conan_denoise_cfg*, const float*, int, const int32_t*, int64_t, int, const conan_denoise_state*, float*, '
                      'conan_denoise_state*, void*) = conan_mel_denoise;\n'
                      'int (*b)(conan_streams*, const int32_t*, int, const conan_denoise_cfg*, const void*, int64_t, void*) = conan_streams_set_denoise;\n'
                      'int (*c)(const conan_streams*, int, conan_denoise_cfg*) = conan_streams_denoise;\n'
                      'int64_t (*d)(void) = conan_denoise_state_bytes;\n'
                      'int (*e)(conan_streams*, const int32_t*, int, void*, int64_t, void*) = conan_streams_denoise_state;\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(protos), "-o", str(tmp_path / "protos.o")], check=True)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "conan_hip.h"\n'
                     'int main(void) {\n'
                     '  printf("%d %zu %zu", CONAN_HIP_ABI_VERSION, sizeof(conan_denoise_cfg), sizeof(conan_denoise_state));\n' +
                     "".join('  printf(" %%zu", offsetof(conan_denoise_cfg, %s));\n' % f for f in fields) +
                     "".join('  printf(" %%zu", offsetof(conan_denoise_state, %s));\n' % f for f in sfields) +
                     '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, str(probe), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [9, 64, 2064] + [getattr(_lib.DenoiseCfg, f).offset for f in fields] + [getattr(_lib.DenoiseState, f).offset for f in sfields]
    assert C.sizeof(_lib.DenoiseCfg) == 64 and C.sizeof(_lib.DenoiseState) == 2064 and _lib.ABI_VERSION == 9


def test_feature_table_row_and_protos():
    f = _lib.SLOT_FEATURES["denoise"]
    assert (f.cfg, f.on, f.build, f.keywords) == (_lib.DenoiseCfg, "enabled", _lib.denoise_cfg, _lib.denoise_keywords)
    assert (f.setter, f.getter, f.seed_state, f.seed_bytes) == ("conan_streams_set_denoise", "conan_streams_denoise", "conan_streams_denoise_state",
                                                                "conan_denoise_state_bytes")
    assert f.state is None and f.last is None and f.meta is None and f.mirror is None and f.stream and f.release and f.method == "set_denoise"
    order = list(_lib.SLOT_FEATURES)      # applied with the other source features, in front of the output leveller
    assert order.index("conceal") < order.index("denoise") < order.index("out_level")
    v = C.c_void_p
    assert _lib._PROTOS["conan_streams_set_denoise"] == (C.c_int, [v, v, C.c_int, v, v, C.c_int64, v])
    assert _lib._PROTOS["conan_streams_denoise"] == (C.c_int, [v, C.c_int, v])
    assert _lib._PROTOS["conan_streams_denoise_state"] == (C.c_int, [v, v, C.c_int, v, C.c_int64, v])
    assert _lib._PROTOS["conan_denoise_state_bytes"] == (C.c_int64, [])
    assert _lib._PROTOS["conan_mel_denoise"] == (C.c_int, [v, v, v, C.c_int, v, C.c_int64, C.c_int, v, v, v, v])


def test_cfg_conversions_round_trip():
    c = _lib.denoise_cfg()      # log10: 51.2 steps per dB
    assert (c.enabled, c.reseed, c.bias, c.knee, c.slope, c.depth, c.close_step, c.open_step, c.rise, c.fall_shift, c.floor_min, c.smooth) == \
        (1, 0, round(3 * 51.2), round(6 * 51.2), 512, round(18 * 51.2), round(4.5 * 51.2), round(18 * 51.2), round(0.05 * 51.2), 1, -5120, 1)
    assert (c.bias, c.knee, c.depth, c.close_step, c.rise) == (154, 307, 922, 230, 3) and list(c.reserved) == [0, 0, 0]
    assert np.float32(c.out_floor) == np.float32(-6.0)      # max(mel_vmin, log10(eps)) = max(-6, -6)
    n = _lib.denoise_cfg(natural_log=True, mel_vmin=-20.0, eps=1e-5)      # ln: 1024 steps are 8.686 dB
    u = 1024.0 * math.log(10.0) / 20.0
    assert abs(20.0 / math.log(10.0) - 8.686) < 1e-3
    assert (n.bias, n.knee, n.depth, n.floor_min) == (round(3 * u), round(6 * u), round(18 * u), round(-100 * u))
    assert np.float32(n.out_floor) == np.float32(math.log(1e-5))
    assert _lib.denoise_cfg(mel_vmin=-4.0).out_floor == -4.0 and _lib.denoise_cfg(out_floor=-7.5).out_floor == -7.5
    assert _lib.denoise_cfg(rise_db=0.0).rise == 0 and _lib.denoise_cfg(close_db=0.0).close_step == 1      # a step is at least one unit
    assert _lib.denoise_cfg(depth_db=12.0).open_step == _lib.denoise_cfg(depth_db=12.0).depth == round(12 * 51.2)      # open follows the depth
    assert _lib.denoise_cfg(open_db=2.0).open_step == round(2 * 51.2)
    c = _lib.denoise_cfg(bias=1, knee=2, depth=3, close_step=4, open_step=5, rise=6, floor_min=-7, slope=8, fall_shift=0, smooth=False, reseed=True)
    assert (c.bias, c.knee, c.depth, c.close_step, c.open_step, c.rise, c.floor_min, c.slope, c.fall_shift, c.smooth, c.reseed) == (1, 2, 3, 4, 5, 6, -7, 8, 0, 0, 1)
    # the reported form gives the same bytes back
    for c in (_lib.denoise_cfg(), _lib.denoise_cfg(natural_log=True, knee_db=9.0, smooth=False, out_floor=-11.25, fall_shift=3)):
        assert bytes(_lib.denoise_cfg(**_lib.denoise_keywords(c))) == bytes(c)
    # a field outside its range is refused by the builder, before any call
    for kw in (dict(bias=-1), dict(knee=FULL + 1), dict(slope=65537), dict(depth=0), dict(close_step=0), dict(open_step=FULL + 1), dict(rise=-1),
               dict(fall_shift=9), dict(floor_min=-FULL - 1), dict(out_floor=float("nan")), dict(out_floor=float("inf")), dict(depth_db=1e9)):
        with pytest.raises(ValueError, match="denoise"):
            _lib.denoise_cfg(**kw)


def test_null_and_invalid_arguments_are_refused_before_any_gpu_use():
    lib = _lib_or_skip()
    one = (C.c_int32 * 1)(0)
    ok = _lib.denoise_cfg()
    off = _lib.DenoiseCfg()
    fake = C.c_void_p(16)      # never dereferenced: the checks below come first
    frames = (C.c_int32 * 2)(10, 4)

    def whole(ctx=fake, cfg=ok, mel=fake, n=2, fr=frames, ld=800, nm=80, seed=None, out=fake, state=None):
        return lib.conan_mel_denoise(ctx, C.byref(cfg) if cfg is not None else None, mel, n, fr, ld, nm, seed, out, state, None)

    for kw in (dict(ctx=None), dict(cfg=None), dict(mel=None), dict(fr=None), dict(out=None)):
        assert whole(**kw) == _lib.ERR_INVALID
        assert b"null argument" in lib.conan_last_error()
    for kw in (dict(n=0), dict(n=65536), dict(nm=0), dict(nm=257), dict(ld=799), dict(ld=-1), dict(ld=2 ** 41), dict(fr=(C.c_int32 * 2)(10, -1)), dict(cfg=off),
               dict(seed=C.c_void_p(20)), dict(state=C.c_void_p(12))):
        assert whole(**kw) == _lib.ERR_INVALID, kw
    assert lib.conan_streams_set_denoise(None, one, 1, C.byref(ok), None, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_denoise(fake, None, 1, C.byref(ok), None, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_denoise(fake, one, 1, None, None, 0, None) == _lib.ERR_INVALID
    for seed, ld in ((C.c_void_p(20), 2064), (C.c_void_p(16), 2056), (C.c_void_p(16), 2068)):      # misaligned, rows too close, a stride off 8
        assert lib.conan_streams_set_denoise(fake, one, 1, C.byref(ok), seed, ld, None) == _lib.ERR_INVALID
    assert lib.conan_streams_denoise(None, 0, C.byref(ok)) == _lib.ERR_INVALID      # (host only: no device is touched either way)
    assert lib.conan_streams_denoise(fake, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_denoise_state(None, one, 1, fake, 2064, None) == _lib.ERR_INVALID
    assert lib.conan_streams_denoise_state(fake, None, 1, fake, 2064, None) == _lib.ERR_INVALID
    assert lib.conan_streams_denoise_state(fake, one, 1, None, 2064, None) == _lib.ERR_INVALID
    assert lib.conan_streams_denoise_state(fake, one, 1, fake, 2056, None) == _lib.ERR_INVALID
    # every refused field of the cfg, before the handle is touched
    for c in bad_cfgs():
        assert lib.conan_streams_set_denoise(fake, one, 1, C.byref(c), None, 0, None) == _lib.ERR_INVALID, lib.conan_last_error()
        assert whole(cfg=c) == _lib.ERR_INVALID


# ---- the Python layer over the stand-ins

def _setter_calls(calls):
    return [(name, args) for name, args in calls if name != "_release"]


def test_streams_setter_getter_and_state(st):  # noqa: F811
    want = _lib.denoise_cfg(depth_db=12.0, reseed=True)
    st.set_denoise([3, 1], depth_db=12.0, reseed=True)
    st.set_denoise([2], dict(depth_db=12.0), reseed=True)
    st.set_denoise([4], want)
    st.set_denoise([5], None)
    seed = Seed()
    st.set_denoise([0, 2], seed=seed, reseed=True, depth_db=12.0)
    got = _setter_calls(st.lib.calls)
    assert [c[0] for c in got] == ["conan_streams_set_denoise"] * 5
    assert [c[1][1] for c in got] == [[3, 1], [2], [4], [5], [0, 2]]
    assert [bytes(c[1][3]) for c in got] == [bytes(want)] * 3 + [bytes(_lib.DenoiseCfg())] + [bytes(want)]
    assert [tuple(c[1][4:6]) for c in got[:4]] == [(None, 0)] * 4 and got[4][1][4] is seed and got[4][1][5] == 32
    assert all(c[1][0] is H and c[1][6] is STREAM for c in got)
    assert [name for name, _ in st.lib.calls].count("_release") == 5      # the setter joins pipelined work
    with pytest.raises(ValueError, match="turns the noise suppression off"):
        st.set_denoise([0], None, depth_db=3.0)
    with pytest.raises(ValueError, match="seed must be a cuda uint8"):
        st.set_denoise([0, 2], seed=Seed(cuda=False))
    for kw in (dict(depth=0), dict(bias=-1), dict(fall_shift=9)):      # a refused cfg raises before a call
        n = len(st.lib.calls)
        with pytest.raises(ValueError):
            st.set_denoise([0], **kw)
        assert len(st.lib.calls) == n

    def answer(h, slot, out):
        C.memmove(C.byref(out), C.byref(want if slot == 3 else _lib.DenoiseCfg()), C.sizeof(out))
        return 0
    st.lib.script["conan_streams_denoise"] = answer
    assert st.denoise([3, 1]) == [_lib.denoise_keywords(want), None]
    st.lib.script["conan_denoise_state_bytes"] = lambda: 2064
    rows = st.denoise_state([1, 3])
    assert tuple(rows.shape) == (2, 2064)
    name, args = st.lib.calls[-2]
    assert name == "conan_streams_denoise_state" and args[1] == [1, 3] and args[3] is rows and args[4] == 2064 and args[5] is STREAM


def test_engine_keyword_and_live_setter():
    eng, st = _engine()
    eng.start_wav(object(), denoise=True)
    assert [c for c in st.calls if c[0] == "set_denoise"] == [("set_denoise", dict(slots=[s], cfg={})) for s in (0, 1, 2)]
    eng, st = _engine()
    eng.open_slots([2, 0, 1], object(), denoise=[dict(depth_db=9.0), None, True])
    # (a stream-set that now uses the feature turns a slot given None off)
    assert [c for c in st.calls if c[0] == "set_denoise"] == [("set_denoise", dict(slots=[2], cfg=dict(depth_db=9.0))), ("set_denoise", dict(slots=[0], cfg=None)),
                                                              ("set_denoise", dict(slots=[1], cfg={}))]
    eng, st = _engine()
    eng.start_wav(object())
    eng.open_slots([1], object(), denoise=None)
    assert not [c for c in st.calls if c[0] == "set_denoise"]      # a stream-set that never used it gets no setter call at all
    eng.set_denoise([1], reseed=True, knee_db=4.0)
    eng.set_denoise(cfg=None)
    assert st.calls[-2:] == [("set_denoise", dict(slots=[1], cfg=True, kw=dict(reseed=True, knee_db=4.0))), ("set_denoise", dict(slots=[0, 1, 2], cfg=None))]
    assert "denoise" in eng._used
    # every refused value raises before a call, in every entry point
    for call in (lambda **kw: eng.start_wav(object(), **kw), lambda **kw: eng.open_slots([0, 1, 2], object(), **kw),
                 lambda **kw: eng.infer_wav(None, object(), **kw), lambda **kw: eng.infer_wav_staggered([None] * 3, [0, 1, 2], object(), **kw)):
        n = len(st.calls)
        with pytest.raises(ValueError, match="4 values for 3"):
            call(denoise=[True] * 4)
        with pytest.raises(ValueError, match="denoise: 'strong'"):
            call(denoise="strong")
        with pytest.raises(ValueError, match="denoise: 3"):
            call(denoise=3)
        assert len(st.calls) == n
