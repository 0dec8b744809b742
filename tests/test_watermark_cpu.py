"""The output watermark without a GPU: the C surface (symbols, the 64-byte cfg, the 16-byte state and record, the result and their
ctypes mirrors, the header as C), the order of the checks - every refused argument is refused before a handle is touched, so fake
handles are never dereferenced - the host-only conan_watermark_decide against tests/watermark_ref.py, the feature-table row, and the
Python layer over the stand-ins of tests/test_slot_features_cpu.py: what Streams and the engine hand the setter."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conan_amd import _lib
from tests import watermark_ref as wm
from tests.test_slot_features_cpu import H, STREAM, Seed, _engine, st  # noqa: F401  (st: the Streams over a recording library)

SYMBOLS = ["conan_watermark_embed", "conan_watermark_detect", "conan_watermark_decide", "conan_streams_set_watermark", "conan_streams_watermark",
           "conan_watermark_state_bytes", "conan_streams_watermark_state"]
# (field, refused value); ("reserved", i): word i non-zero
BAD = [("enabled", 2), ("enabled", -1), ("reseed", 2), ("reseed", -1), ("id", -1), ("id", 65536), ("gain", -0.5), ("gain", 1.5), ("gain", float("nan")),
       ("gain", float("inf")), ("floor", -1e-3), ("floor", 2.0), ("floor", float("nan")), ("reserved", 0), ("reserved", 8)]


def bad_cfgs():
    out = []
    for field, value in BAD:
        c = _lib.watermark_cfg(key=5, id=7)
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
    raw.conan_watermark_state_bytes.restype = C.c_int64
    assert raw.conan_watermark_state_bytes() == 16 == C.sizeof(_lib.WatermarkState) == wm.STATE_BYTES


def test_header_compiles_as_c_and_matches_the_mirror(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not present")
    inc = os.path.dirname(_lib.HEADER_PATH)
    structs = (("conan_watermark_cfg", _lib.WatermarkCfg), ("conan_watermark_state", _lib.WatermarkState), ("conan_watermark_hit", _lib.WatermarkHit),
               ("conan_watermark_result", _lib.WatermarkResult))
    protos = tmp_path / "protos.c"
    protos.write_text('#include "conan_hip.h"\n'
                      'int (*a)(conan_ctx*, const conan_watermark_cfg*, const float*, int, const int64_t*, int64_t, const conan_watermark_state*, float*, '
                      'conan_watermark_state*, void*) = conan_watermark_embed;\n'
                      'int (*b)(conan_ctx*, uint64_t, int, const void*, int64_t, int, const int64_t*, int64_t*, int64_t*, int64_t, conan_watermark_hit*, void*) = '
                      'conan_watermark_detect;\n'
                      'int (*c)(const int64_t*, const int64_t*, const conan_watermark_hit*, double, conan_watermark_result*) = conan_watermark_decide;\n'
                      'int (*d)(conan_streams*, const int32_t*, int, const conan_watermark_cfg*, const void*, int64_t, void*) = conan_streams_set_watermark;\n'
                      'int (*e)(const conan_streams*, int, conan_watermark_cfg*) = conan_streams_watermark;\n'
                      'int64_t (*f)(void) = conan_watermark_state_bytes;\n'
                      'int (*g)(conan_streams*, const int32_t*, int, void*, int64_t, void*) = conan_streams_watermark_state;\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(protos), "-o", str(tmp_path / "protos.o")], check=True)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "conan_hip.h"\n'
                     'int main(void) {\n'
                     '  printf("%d %.17g", CONAN_HIP_ABI_VERSION, CONAN_WATERMARK_THRESHOLD);\n' +
                     "".join('  printf(" %%zu", sizeof(%s));\n' % name + "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (name, f[0]) for f in mirror._fields_)
                             for name, mirror in structs) +
                     '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, str(probe), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    want = []
    for _, mirror in structs:
        want += [C.sizeof(mirror)] + [getattr(mirror, f[0]).offset for f in mirror._fields_]
    assert int(out[0]) == 9 == _lib.ABI_VERSION and float(out[1]) == _lib.WATERMARK_THRESHOLD == wm.THRESHOLD
    assert [int(v) for v in out[2:]] == want
    assert [C.sizeof(m) for _, m in structs] == [64, 16, 16, 40]


def test_feature_table_row_and_protos():
    f = _lib.SLOT_FEATURES["watermark"]
    assert (f.cfg, f.on, f.build, f.keywords) == (_lib.WatermarkCfg, "enabled", _lib.watermark_cfg, _lib.watermark_keywords)
    assert (f.setter, f.getter, f.seed_state, f.seed_bytes) == ("conan_streams_set_watermark", "conan_streams_watermark", "conan_streams_watermark_state",
                                                                "conan_watermark_state_bytes")
    assert f.state is None and f.last is None and f.meta is None and f.mirror is None and f.stream and f.release and f.method == "set_watermark"
    assert list(_lib.SLOT_FEATURES)[-1] == "watermark"      # applied last: it is the last stage of the audio's path
    v = C.c_void_p
    assert _lib._PROTOS["conan_streams_set_watermark"] == (C.c_int, [v, v, C.c_int, v, v, C.c_int64, v])
    assert _lib._PROTOS["conan_streams_watermark"] == (C.c_int, [v, C.c_int, v])
    assert _lib._PROTOS["conan_streams_watermark_state"] == (C.c_int, [v, v, C.c_int, v, C.c_int64, v])
    assert _lib._PROTOS["conan_watermark_state_bytes"] == (C.c_int64, [])
    assert _lib._PROTOS["conan_watermark_embed"] == (C.c_int, [v, v, v, C.c_int, v, C.c_int64, v, v, v, v])
    assert _lib._PROTOS["conan_watermark_detect"] == (C.c_int, [v, C.c_uint64, C.c_int, v, C.c_int64, C.c_int, v, v, v, C.c_int64, v, v])
    assert _lib._PROTOS["conan_watermark_decide"] == (C.c_int, [v, v, v, C.c_double, v])


def test_cfg_builder_round_trip_and_ranges():
    c = _lib.watermark_cfg()
    assert (c.enabled, c.reseed, c.key, c.id, list(c.reserved)) == (1, 0, 0, 0, [0] * 9)
    assert np.float32(c.gain) == np.float32(wm.GAIN) and c.floor == wm.FLOOR == 0.0
    c = _lib.watermark_cfg(key=2 ** 64 - 1, id=0xBEEF, gain=0.05, floor=0.001, reseed=True)
    assert (c.key, c.id, c.reseed) == (2 ** 64 - 1, 0xBEEF, 1)
    assert bytes(_lib.watermark_cfg(reseed=True, **_lib.watermark_keywords(c))) == bytes(c)      # the reported form gives the same bytes back
    for kw in (dict(key=-1), dict(key=2 ** 64), dict(id=-1), dict(id=65536), dict(gain=-0.1), dict(gain=1.1), dict(gain=float("nan")), dict(floor=-1e-3),
               dict(floor=float("inf"))):
        with pytest.raises(ValueError, match="watermark"):
            _lib.watermark_cfg(**kw)


def test_null_and_invalid_arguments_are_refused_before_any_gpu_use():
    lib = _lib_or_skip()
    one = (C.c_int32 * 1)(0)
    ok = _lib.watermark_cfg(key=5, id=7)
    off = _lib.WatermarkCfg()
    fake = C.c_void_p(16)      # never dereferenced: the checks below come first
    lens = (C.c_int64 * 2)(640, 64)

    def embed(ctx=fake, cfg=ok, x=fake, n=2, sm=lens, ld=640, seed=None, out=fake, state=None):
        return lib.conan_watermark_embed(ctx, C.byref(cfg) if cfg is not None else None, x, n, sm, ld, seed, out, state, None)

    for kw in (dict(ctx=None), dict(cfg=None), dict(x=None), dict(sm=None), dict(out=None)):
        assert embed(**kw) == _lib.ERR_INVALID
        assert b"null argument" in lib.conan_last_error()
    for kw in (dict(n=0), dict(n=65536), dict(ld=639), dict(ld=-1), dict(ld=2 ** 41), dict(sm=(C.c_int64 * 2)(640, -1)), dict(sm=(C.c_int64 * 2)(2 ** 31, 1), ld=2 ** 32),
               dict(cfg=off), dict(seed=C.c_void_p(20)), dict(state=C.c_void_p(12))):
        assert embed(**kw) == _lib.ERR_INVALID, kw

    def detect(ctx=fake, fmt=0, x=fake, ld=640, n=2, sm=lens, score=fake, soft=fake, soft_ld=4, hit=fake):
        return lib.conan_watermark_detect(ctx, 5, fmt, x, ld, n, sm, score, soft, soft_ld, hit, None)

    for kw in (dict(ctx=None), dict(x=None), dict(sm=None), dict(score=None), dict(soft=None), dict(hit=None), dict(fmt=4), dict(fmt=-1), dict(n=0), dict(n=4097),
               dict(ld=639), dict(x=C.c_void_p(18)), dict(score=C.c_void_p(20)), dict(sm=(C.c_int64 * 2)(-1, 0)), dict(sm=(C.c_int64 * 2)(2 ** 26 + 1, 0), ld=2 ** 27),
               dict(sm=(C.c_int64 * 2)(3 * 2048, 0), ld=3 * 2048, soft_ld=1), dict(fmt=1, ld=160, sm=(C.c_int64 * 2)(321, 0))):
        assert detect(**kw) == _lib.ERR_INVALID, kw
    assert lib.conan_streams_set_watermark(None, one, 1, C.byref(ok), None, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_watermark(fake, None, 1, C.byref(ok), None, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_watermark(fake, one, 1, None, None, 0, None) == _lib.ERR_INVALID
    for seed, ld in ((C.c_void_p(20), 16), (C.c_void_p(16), 8), (C.c_void_p(16), 20)):      # misaligned, rows too close, a stride off 8
        assert lib.conan_streams_set_watermark(fake, one, 1, C.byref(ok), seed, ld, None) == _lib.ERR_INVALID
    assert lib.conan_streams_watermark(None, 0, C.byref(ok)) == _lib.ERR_INVALID      # (host only: no device is touched either way)
    assert lib.conan_streams_watermark(fake, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_watermark_state(None, one, 1, fake, 16, None) == _lib.ERR_INVALID
    assert lib.conan_streams_watermark_state(fake, None, 1, fake, 16, None) == _lib.ERR_INVALID
    assert lib.conan_streams_watermark_state(fake, one, 1, None, 16, None) == _lib.ERR_INVALID
    assert lib.conan_streams_watermark_state(fake, one, 1, fake, 8, None) == _lib.ERR_INVALID
    # every refused field of the cfg, before the handle is touched
    for c in bad_cfgs():
        assert lib.conan_streams_set_watermark(fake, one, 1, C.byref(c), None, 0, None) == _lib.ERR_INVALID, lib.conan_last_error()
        assert embed(cfg=c) == _lib.ERR_INVALID


def _decide(lib, S, soft, offset, blocks, threshold=_lib.WATERMARK_THRESHOLD):
    S, soft = np.ascontiguousarray(S, dtype=np.int64), np.ascontiguousarray(soft, dtype=np.int64)
    hit, out = _lib.WatermarkHit(offset, blocks, int(S[offset]) if blocks else 0), _lib.WatermarkResult()
    assert lib.conan_watermark_decide(S.ctypes.data_as(C.c_void_p), soft.ctypes.data_as(C.c_void_p) if len(soft) else None, C.byref(hit), threshold,
                                      C.byref(out)) == 0, lib.conan_last_error()
    return out


def test_decide_is_the_reference_s():
    lib = _lib_or_skip()
    rng = np.random.default_rng(7)
    w = wm.word(0xBEEF)
    for trial in range(6):
        K = int(rng.integers(1, 70))
        S = rng.integers(0, 40000, wm.BLK)
        o = int(rng.integers(0, wm.BLK))
        S[o] = 40000 + int(rng.integers(0, 400000))
        soft = (rng.integers(-300, 300, K) + 200 * w[(np.arange(K) + trial) % wm.W] * (trial % 2)).astype(np.int64)
        got, want = _decide(lib, S, soft, o, K), wm.decide(S, soft, o, K)
        assert (got.present, got.id, got.offset, got.rotation, got.blocks, got.marker_score) == \
            (want["present"], want["id"], want["offset"], want["rotation"], want["blocks"], want["marker_score"])
        assert abs(got.z - want["z"]) <= 1e-12 * abs(want["z"])
    got = _decide(lib, np.zeros(wm.BLK), np.zeros(0), 0, 0)      # K = 0: nothing is read
    assert (got.present, got.blocks, got.z, got.id) == (0, 0, 0.0, 0)
    assert _decide(lib, np.full(wm.BLK, 9), np.ones(2), 3, 2).z == 0.0
    hit = _lib.WatermarkHit(2048, 1, 0)
    assert lib.conan_watermark_decide(None, None, C.byref(hit), 1.0, C.byref(_lib.WatermarkResult())) == _lib.ERR_INVALID
    assert lib.conan_watermark_decide(None, None, None, 1.0, C.byref(_lib.WatermarkResult())) == _lib.ERR_INVALID


# ---- the Python layer over the stand-ins

def _setter_calls(calls):
    return [(name, args) for name, args in calls if name != "_release"]


def test_streams_setter_getter_and_state(st):  # noqa: F811
    want = _lib.watermark_cfg(key=77, id=0xBEEF, reseed=True)
    st.set_watermark([3, 1], key=77, id=0xBEEF, reseed=True)
    st.set_watermark([2], dict(key=77, id=0xBEEF), reseed=True)
    st.set_watermark([4], want)
    st.set_watermark([5], None)
    seed = Seed()
    st.set_watermark([0, 2], seed=seed, reseed=True, key=77, id=0xBEEF)
    got = _setter_calls(st.lib.calls)
    assert [c[0] for c in got] == ["conan_streams_set_watermark"] * 5
    assert [c[1][1] for c in got] == [[3, 1], [2], [4], [5], [0, 2]]
    assert [bytes(c[1][3]) for c in got] == [bytes(want)] * 3 + [bytes(_lib.WatermarkCfg())] + [bytes(want)]
    assert [tuple(c[1][4:6]) for c in got[:4]] == [(None, 0)] * 4 and got[4][1][4] is seed and got[4][1][5] == 32
    assert all(c[1][0] is H and c[1][6] is STREAM for c in got)
    assert [name for name, _ in st.lib.calls].count("_release") == 5      # the setter joins pipelined work
    with pytest.raises(ValueError, match="turns the watermark off"):
        st.set_watermark([0], None, key=3)
    with pytest.raises(ValueError, match="seed must be a cuda uint8"):
        st.set_watermark([0, 2], seed=Seed(cuda=False))
    for kw in (dict(id=65536), dict(gain=2.0), dict(floor=-1.0), dict(key=-1)):      # a refused cfg raises before a call
        n = len(st.lib.calls)
        with pytest.raises(ValueError):
            st.set_watermark([0], **kw)
        assert len(st.lib.calls) == n

    def answer(h, slot, out):
        C.memmove(C.byref(out), C.byref(want if slot == 3 else _lib.WatermarkCfg()), C.sizeof(out))
        return 0
    st.lib.script["conan_streams_watermark"] = answer
    assert st.watermark([3, 1]) == [_lib.watermark_keywords(want), None]
    st.lib.script["conan_watermark_state_bytes"] = lambda: 16
    rows = st.watermark_state([1, 3])
    assert tuple(rows.shape) == (2, 16)
    name, args = st.lib.calls[-2]
    assert name == "conan_streams_watermark_state" and args[1] == [1, 3] and args[3] is rows and args[4] == 16 and args[5] is STREAM


def test_engine_keyword_and_live_setter():
    mark = dict(key=77, id=0xBEEF)
    eng, st = _engine()
    eng.start(object(), watermark=mark)
    assert [c for c in st.calls if c[0] == "set_watermark"] == [("set_watermark", dict(slots=[s], cfg=mark)) for s in (0, 1, 2)]
    eng, st = _engine()
    eng.start_wav(object(), watermark=True, out_level=True)
    names = [c[0] for c in st.calls]
    assert [c for c in st.calls if c[0] == "set_watermark"] == [("set_watermark", dict(slots=[s], cfg={})) for s in (0, 1, 2)]
    assert max(i for i, m in enumerate(names) if m == "set_output_level") < min(i for i, m in enumerate(names) if m == "set_watermark")
    eng, st = _engine()
    eng.open_slots([2, 0, 1], object(), watermark=[mark, None, True])
    # (a stream-set that now uses the feature turns a slot given None off)
    assert [c for c in st.calls if c[0] == "set_watermark"] == [("set_watermark", dict(slots=[2], cfg=mark)), ("set_watermark", dict(slots=[0], cfg=None)),
                                                                ("set_watermark", dict(slots=[1], cfg={}))]
    assert st.calls[-1][0] == "set_watermark"      # behind every other feature
    eng, st = _engine()
    eng.start_wav(object())
    eng.open_slots([1], object(), watermark=None)
    eng.start(object())
    assert not [c for c in st.calls if c[0] == "set_watermark"]      # a stream-set that never used it gets no setter call at all
    seed = object()
    eng.set_watermark([1], reseed=True, key=9)
    eng.set_watermark([2], mark, seed=seed)
    eng.set_watermark(cfg=None)
    assert st.calls[-3:] == [("set_watermark", dict(slots=[1], cfg=True, seed=None, kw=dict(reseed=True, key=9))),
                             ("set_watermark", dict(slots=[2], cfg=mark, seed=seed)), ("set_watermark", dict(slots=[0, 1, 2], cfg=None, seed=None))]
    assert "watermark" in eng._used
    # every refused value raises before a call, in every entry point
    for call in (lambda **kw: eng.start(object(), **kw), lambda **kw: eng.start_wav(object(), **kw), lambda **kw: eng.open_slots([0, 1, 2], object(), **kw),
                 lambda **kw: eng.infer(None, object(), **kw), lambda **kw: eng.infer_wav(None, object(), **kw),
                 lambda **kw: eng.infer_wav_staggered([None] * 3, [0, 1, 2], object(), **kw)):
        n = len(st.calls)
        with pytest.raises(ValueError, match="4 values for 3"):
            call(watermark=[True] * 4)
        with pytest.raises(ValueError, match="watermark: 'loud'"):
            call(watermark="loud")
        with pytest.raises(ValueError, match="watermark: 3"):
            call(watermark=3)
        assert len(st.calls) == n
