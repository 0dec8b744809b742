"""Source activity without a GPU: the C surface (symbols, the 96-byte cfg, the 40-byte state and their ctypes mirrors, the header as
C), the order of the checks - every refused argument is refused before a handle is touched, so fake handles are never dereferenced -
and the engine's host logic for activity=."""
import ctypes as C
import os
import shutil
import subprocess
import types

import pytest

from conan_amd import _lib
from tests import activity_ref as A

SYMBOLS = ["conan_activity", "conan_activity_gate", "conan_streams_set_activity", "conan_streams_activity", "conan_streams_activity_state",
           "conan_step_wav_activity"]
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


def test_cfg_mirror_and_helpers():
    assert C.sizeof(_lib.ActivityState) == 40 and C.sizeof(_lib.ActivityCfg) == 96
    assert _lib.ACTIVITY_FULL == FULL == A.FULL
    c = _lib.activity_cfg()
    assert (c.mode, c.reseed, c.hold_frames, c.up_step, c.down_step, c.closed_level, c.reserved) == (2, 0, 10, FULL, 209716, 0, 0)
    assert (c.open_abs, c.close_abs) == (_lib.db_power(-50.0), _lib.db_power(-55.0))
    assert (c.open_ratio, c.close_ratio) == (_lib.db_power(9.0), _lib.db_power(6.0))
    assert (c.rise_active, c.rise_idle) == (C.c_float(1.005).value, C.c_float(1.02).value)
    assert c.floor_min == _lib.db_power(-70.0)
    assert _lib.activity_state_dict(c.seed) == dict(active=0, hang=0, level=0, floor=_lib.db_power(-60.0), frames=0, active_frames=0)
    assert _lib.activity_cfg(gate=False).mode == 1
    c = _lib.activity_cfg(closed_db=-20.0, attack_frames=2, release_frames=4, reseed=True)
    cl = round(FULL * 0.1)
    assert (c.closed_level, c.seed.level, c.reseed) == (cl, cl, 1)
    assert 2 * c.up_step >= FULL - cl > c.up_step and 4 * c.down_step >= FULL - cl > 3 * c.down_step
    # the reported form gives the same bytes back, also with a handed-over state as the seed
    seed = dict(active=1, hang=3, level=12345, floor=3.25e-6, frames=1000, active_frames=400)
    c = _lib.activity_cfg(gate=False, open_db=-41.5, hold_frames=3, up_step=FULL // 3, down_step=FULL // 7 + 1, closed_level=1 << 10, seed=seed)
    kw = _lib.activity_keywords(c)
    assert kw["seed"] == seed and kw["gate"] is False
    assert bytes(_lib.activity_cfg(**kw)) == bytes(c)


def test_header_compiles_as_c_and_matches_the_mirror(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not present")
    inc = os.path.dirname(_lib.HEADER_PATH)
    fields = [f[0] for f in _lib.ActivityCfg._fields_]
    sfields = [f[0] for f in _lib.ActivityState._fields_]
    protos = tmp_path / "protos.c"
    protos.write_text('#include "conan_hip.h"\n'
                      'int (*a)(conan_ctx*, const conan_mel_cfg*, const conan_activity_cfg*, const float*, int, int, int32_t*, int32_t*, double*, '
                      'conan_activity_state*, int32_t*, void*) = conan_activity;\n'
                      'int (*b)(conan_ctx*, int, const float*, int, int64_t, int64_t, const int32_t*, int64_t, int32_t, float*, void*) = conan_activity_gate;\n'
                      'int (*c)(conan_streams*, const int32_t*, int, const conan_activity_cfg*, void*) = conan_streams_set_activity;\n'
                      'int (*d)(const conan_streams*, int, conan_activity_cfg*) = conan_streams_activity;\n'
                      'int (*e)(conan_streams*, const int32_t*, int, conan_activity_state*, void*) = conan_streams_activity_state;\n'
                      'int (*f)(conan_streams*, int32_t*, int32_t*, void*) = conan_step_wav_activity;\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(protos), "-o", str(tmp_path / "protos.o")], check=True)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "conan_hip.h"\n'
                     'int main(void) {\n'
                     '  printf("%d %zu %zu %d", CONAN_HIP_ABI_VERSION, sizeof(conan_activity_cfg), sizeof(conan_activity_state), CONAN_ACTIVITY_FULL);\n' +
                     "".join('  printf(" %%zu", offsetof(conan_activity_cfg, %s));\n' % f for f in fields) +
                     "".join('  printf(" %%zu", offsetof(conan_activity_state, %s));\n' % f for f in sfields) +
                     '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, str(probe), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [9, 96, 40, FULL] + [getattr(_lib.ActivityCfg, f).offset for f in fields] + [getattr(_lib.ActivityState, f).offset for f in sfields]


def _bad_cfgs():
    inf, nan = float("inf"), float("nan")
    out = []
    for field, value in (("mode", 3), ("mode", -1), ("reseed", 2), ("reseed", -1), ("open_abs", nan), ("open_abs", inf), ("close_abs", nan),
                         ("close_abs", -1e-9), ("close_abs", 1.0), ("open_ratio", inf), ("open_ratio", nan), ("close_ratio", -1.0),
                         ("close_ratio", 100.0), ("close_ratio", nan), ("rise_active", 0.99), ("rise_active", inf), ("rise_idle", 0.5),
                         ("rise_idle", nan), ("floor_min", 0.0), ("floor_min", -1.0), ("floor_min", nan), ("floor_min", 1.0),
                         ("hold_frames", -1), ("hold_frames", FULL + 1), ("up_step", 0), ("up_step", FULL + 1), ("down_step", 0),
                         ("down_step", FULL + 1), ("closed_level", -1), ("closed_level", FULL), ("reserved", 1)):
        c = _lib.activity_cfg()
        setattr(c, field, value)
        out.append(c)
    for field, value in (("level", FULL + 1), ("level", -1), ("floor", 0.0), ("floor", nan), ("floor", inf), ("reserved", 7), ("active", 2),
                         ("active", -1), ("hang", -1), ("hang", FULL + 1), ("frames", -1), ("active_frames", -1), ("active_frames", 5)):
        c = _lib.activity_cfg()
        setattr(c.seed, field, value)
        out.append(c)
    c = _lib.activity_cfg(closed_level=1 << 10)
    c.seed.level = 5      # under closed_level
    out.append(c)
    return out


def test_null_and_invalid_arguments_are_refused_before_any_gpu_use():
    lib = _lib_or_skip()
    one = (C.c_int32 * 1)(0)
    ok = _lib.activity_cfg()
    mel = _lib.MelCfg(1024, 320, 1024, 80, 16000, 80.0, 7600.0, 1e-6, -6.0, 1.5, 0, 0, 0.0)
    fake = C.c_void_p(16)      # never dereferenced: the checks below come first

    def whole(ctx=fake, m=mel, c=ok, wav=fake, n=2, samples=1000, act=fake, lvl=fake):
        return lib.conan_activity(ctx, C.byref(m) if m is not None else None, C.byref(c) if c is not None else None, wav, n, samples, act, lvl, None, None,
                                  None, None)

    def gate(ctx=fake, hop=320, wav=fake, n=2, samples=1000, ld=1000, lv=fake, lvld=4, start=0, out=fake):
        return lib.conan_activity_gate(ctx, hop, wav, n, samples, ld, lv, lvld, start, out, None)

    for kw in (dict(ctx=None), dict(m=None), dict(c=None), dict(wav=None), dict(act=None), dict(lvl=None)):
        assert whole(**kw) == _lib.ERR_INVALID
        assert b"null argument" in lib.conan_last_error()
    for kw in (dict(ctx=None), dict(wav=None), dict(lv=None), dict(out=None)):
        assert gate(**kw) == _lib.ERR_INVALID
        assert b"null argument" in lib.conan_last_error()
    assert lib.conan_streams_set_activity(None, one, 1, C.byref(ok), None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_activity(fake, None, 1, C.byref(ok), None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_activity(fake, one, 1, None, None) == _lib.ERR_INVALID
    assert lib.conan_streams_activity(None, 0, C.byref(ok)) == _lib.ERR_INVALID      # (host only: no device is touched either way)
    assert lib.conan_streams_activity(fake, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_activity_state(None, one, 1, fake, None) == _lib.ERR_INVALID
    assert lib.conan_streams_activity_state(fake, None, 1, fake, None) == _lib.ERR_INVALID
    assert lib.conan_streams_activity_state(fake, one, 1, None, None) == _lib.ERR_INVALID
    assert lib.conan_step_wav_activity(None, fake, fake, None) == _lib.ERR_INVALID
    assert lib.conan_step_wav_activity(fake, None, fake, None) == _lib.ERR_INVALID
    assert lib.conan_step_wav_activity(fake, fake, None, None) == _lib.ERR_INVALID
    # every refused field of the cfg, by both entry points, before the handle is touched
    for c in _bad_cfgs():
        assert whole(c=c) == _lib.ERR_INVALID, lib.conan_last_error()
        assert lib.conan_streams_set_activity(fake, one, 1, C.byref(c), None) == _lib.ERR_INVALID
    # conan_activity's own arguments: an enabled cfg, the frame geometry, the row count, the samples
    assert whole(c=_lib.ActivityCfg()) == _lib.ERR_INVALID and b"mode" in lib.conan_last_error()
    for bad in (dict(fft_size=1000), dict(fft_size=32), dict(fft_size=4096), dict(sample_rate=22050), dict(hop_size=0)):
        m = _lib.MelCfg(1024, 320, 1024, 80, 16000, 80.0, 7600.0, 1e-6, -6.0, 1.5, 0, 0, 0.0)
        for k, v in bad.items():
            setattr(m, k, v)
        assert whole(m=m) == _lib.ERR_INVALID, bad
    assert whole(n=0) == _lib.ERR_INVALID and whole(n=65536) == _lib.ERR_INVALID and whole(samples=0) == _lib.ERR_INVALID
    # conan_activity_gate's: the hop, the row count, the samples and both strides, the start level
    for kw in (dict(hop=0), dict(hop=4096), dict(n=0), dict(n=65536), dict(samples=0), dict(samples=2 ** 31), dict(ld=999), dict(ld=2 ** 31),
               dict(lvld=3), dict(start=-1), dict(start=FULL + 1)):
        assert gate(**kw) == _lib.ERR_INVALID, kw


def _engine(n):
    from conan_amd.engine import StreamingVoiceConversionEngine as Engine
    eng = Engine.__new__(Engine)      # no context, no stream-set: the checks must come before either is touched
    eng.slots = list(range(n))
    return eng


def test_engine_activity_values():
    from conan_amd.engine import StreamingVoiceConversionEngine as Engine
    got = Engine._values("activity", [None, True, "detect", dict(hold_frames=3, gate=False), False], 5)
    assert got == [None, dict(gate=True), dict(gate=False), dict(hold_frames=3, gate=False), None]
    assert Engine._values("activity", "detect", 2) == [dict(gate=False)] * 2
    eng = _engine(2)
    calls = [lambda **kw: eng.start_wav(kw.pop("ref_mel"), **kw), lambda **kw: eng.open_slots([0, 1], kw.pop("ref_mel"), **kw),
             lambda **kw: eng.infer_wav(None, kw.pop("ref_mel"), **kw), lambda **kw: eng.infer_wav_staggered([None, None], [0, 1], kw.pop("ref_mel"), **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="3 values for 2"):
            call(ref_mel=object(), activity=[True, True, True])
        with pytest.raises(ValueError, match="'gate'"):
            call(ref_mel=object(), activity="gate")
        with pytest.raises(ValueError, match="activity: 2.5"):
            call(ref_mel=object(), activity=2.5)
    # a stream-set that never used it is left alone: no setter call at all
    eng._used = set()
    eng.st = types.SimpleNamespace()      # (any attribute access would raise)
    eng._apply("activity", eng.slots, [None, None])
    assert "activity" not in eng._used
    # once used, None turns a slot off and a dict travels as the cfg
    seen = []
    eng.st = types.SimpleNamespace(set_activity=lambda slots, cfg=True, **kw: seen.append((list(slots), cfg, kw)))
    eng._apply("activity", eng.slots, [dict(gate=False), None])
    assert "activity" in eng._used and seen == [([0], dict(gate=False), {}), ([1], None, {})]
    eng.set_activity([1], hold_frames=2)
    assert seen[-1] == ([1], True, dict(hold_frames=2))
