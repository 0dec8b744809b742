"""The echo-delay estimator without a GPU: the C surface (the six symbols, the 48-byte cfg and its ctypes mirror), the order of the
checks - every refused argument is refused before a handle is touched, so fake handles are never dereferenced - the defaults and
ranges of _lib.echo_delay_cfg, the follow rule on a table of cases, the feature table (which has no row for it) and the engine's
host logic for echo_delay=."""
import ctypes as C
import os
import types

import pytest

from conan_amd import _lib
from tests import echo_delay_ref as R

SYMBOLS = ["conan_streams_set_echo_delay", "conan_streams_echo_delay_cfg", "conan_streams_echo_delay", "conan_echo_delay_state_bytes",
           "conan_streams_echo_delay_state", "conan_echo_delay"]
STATE_BYTES = 64 + 4 * 6144 + 6144      # header, A, the far end's ternary history


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
    raw.conan_echo_delay_state_bytes.restype = C.c_int64
    assert raw.conan_echo_delay_state_bytes() == STATE_BYTES == R.STATE_BYTES


def test_cfg_builder_and_keywords_round_trip():
    assert C.sizeof(_lib.EchoDelayCfg) == 48
    assert (_lib.ECHO_DELAY_FRAME, _lib.ECHO_DELAY_MAX_LAGS) == (R.FRAME, R.MAX_LAGS) == (1024, _lib.ECHO_MAX_DELAY + _lib.ECHO_MAX_TAPS)
    assert _lib.ECHO_DELAY_REPORT == R.REPORT
    for rate, n_lags, tol in ((8000, 3072, 16), (16000, 6144, 32), (22050, 6144, 44), (48000, 6144, 96)):
        kw = _lib.echo_delay_keywords(rate)
        assert kw == R.defaults(rate) == dict(n_lags=n_lags, thr=16, leak=5, ratio=10, min_peak=1024, hold=4, tol=tol)
        c = _lib.echo_delay_cfg(rate)
        assert c.enabled == 1 and list(c.reserved) == [0] * 4 and _lib.echo_delay_keywords(c) == kw
    c = _lib.echo_delay_cfg(8000, n_lags=320, thr=1, hold=2)
    assert (c.n_lags, c.thr, c.leak, c.ratio, c.min_peak, c.hold, c.tol) == (320, 1, 5, 10, 1024, 2, 16)
    assert bytes(_lib.echo_delay_cfg(**_lib.echo_delay_keywords(c))) == bytes(c)      # the reported form gives the same bytes back
    with pytest.raises(ValueError, match="unknown"):
        _lib.echo_delay_cfg(16000, delay=3)
    with pytest.raises(ValueError, match="without a rate"):
        _lib.echo_delay_cfg(n_lags=64)


BAD = [("n_lags", 0), ("n_lags", 32), ("n_lags", 65), ("n_lags", 6208), ("n_lags", -64), ("thr", 0), ("thr", 32768), ("leak", 0), ("leak", 9),
       ("ratio", 0), ("min_peak", 0), ("hold", 0), ("tol", -1)]


def test_range_refusals():
    for field, value in BAD:
        with pytest.raises(ValueError, match=field):
            _lib.echo_delay_cfg(16000, **{field: value})
    lib = _lib_or_skip()
    one = (C.c_int32 * 1)(0)
    n64 = (C.c_int64 * 2)(100, 100)
    ok, off = _lib.echo_delay_cfg(16000), _lib.EchoDelayCfg()
    fake = C.c_void_p(16)      # never dereferenced: the checks below come first

    def whole(ctx=fake, cfg=ok, fmt=_lib.SAMPLE_F32, x=fake, ld=100, far=fake, far_ld=100, n=2, samples=n64, track=None, track_ld=0, report=None):
        return lib.conan_echo_delay(ctx, None if cfg is None else C.byref(cfg), fmt, x, ld, far, far_ld, n, samples, track, track_ld, report, None)

    for kw in (dict(ctx=None), dict(cfg=None), dict(x=None), dict(far=None), dict(samples=None)):
        assert whole(**kw) == _lib.ERR_INVALID
        assert b"null argument" in lib.conan_last_error()
    for kw in (dict(cfg=off), dict(fmt=4), dict(fmt=-1), dict(n=0), dict(n=65536), dict(ld=99), dict(far_ld=99), dict(ld=-1), dict(far_ld=-1),
               dict(x=C.c_void_p(18)), dict(far=C.c_void_p(18)), dict(report=C.c_void_p(20)), dict(track=C.c_void_p(20)), dict(track_ld=-1),
               dict(samples=(C.c_int64 * 2)(100, -1)), dict(fmt=_lib.SAMPLE_S16, ld=49),
               dict(samples=(C.c_int64 * 2)(100, 2048), ld=2048, far_ld=2048, track=C.c_void_p(64), track_ld=11)):      # two frame ends need 12
        assert whole(**kw) == _lib.ERR_INVALID, kw
    for field, value in BAD + [("enabled", 2), ("enabled", -1)]:
        c = _lib.echo_delay_cfg(16000)
        setattr(c, field, value)
        assert whole(cfg=c) == _lib.ERR_INVALID, lib.conan_last_error()
        assert lib.conan_streams_set_echo_delay(fake, one, 1, C.byref(c), None, 0, None) == _lib.ERR_INVALID, lib.conan_last_error()
    assert lib.conan_streams_set_echo_delay(None, one, 1, C.byref(ok), None, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_echo_delay(fake, None, 1, C.byref(ok), None, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_echo_delay(fake, one, 1, None, None, 0, None) == _lib.ERR_INVALID
    # a seed that is misaligned, or whose rows are closer than a record
    assert lib.conan_streams_set_echo_delay(fake, one, 1, C.byref(ok), C.c_void_p(20), STATE_BYTES, None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_echo_delay(fake, one, 1, C.byref(ok), C.c_void_p(64), STATE_BYTES - 8, None) == _lib.ERR_INVALID
    assert lib.conan_streams_echo_delay_cfg(None, 0, C.byref(off)) == _lib.ERR_INVALID      # (host only)
    assert lib.conan_streams_echo_delay_cfg(fake, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_echo_delay(None, one, 1, one, fake, 100, fake, 100, None, None) == _lib.ERR_INVALID
    assert lib.conan_streams_echo_delay(fake, None, 1, one, fake, 100, fake, 100, None, None) == _lib.ERR_INVALID
    assert lib.conan_streams_echo_delay(fake, one, 1, None, fake, 100, fake, 100, None, None) == _lib.ERR_INVALID
    assert lib.conan_streams_echo_delay_state(None, one, 1, fake, STATE_BYTES, None) == _lib.ERR_INVALID
    assert lib.conan_streams_echo_delay_state(fake, None, 1, fake, STATE_BYTES, None) == _lib.ERR_INVALID
    assert lib.conan_streams_echo_delay_state(fake, one, 1, None, STATE_BYTES, None) == _lib.ERR_INVALID
    assert lib.conan_streams_echo_delay_state(fake, one, 1, fake, STATE_BYTES - 8, None) == _lib.ERR_INVALID


# (est, age, in force, lead, hyst, max_age) -> the delay to set, or None
FOLLOW = [((-1, 0, 0, 128, 64, 64), None),            # no estimate
          ((3000, 0, 0, 128, 64, 64), 2872),          # the target lies `lead` in front of the estimate
          ((3000, 64, 0, 128, 64, 64), 2872),         # as old as max_age: still good
          ((3000, 65, 0, 128, 64, 64), None),         # older: the line may have moved
          ((3000, 0, 2872, 128, 64, 64), None),       # already there
          ((3000, 0, 2808, 128, 64, 64), None),       # within hyst
          ((3000, 0, 2807, 128, 64, 64), 2872),       # one beyond
          ((3000, 0, 2937, 128, 64, 64), 2872),
          ((100, 0, 500, 128, 64, 64), 0),            # clamped at 0
          ((100, 0, 64, 128, 64, 64), None),          # ... and within hyst of it
          ((6000, 0, 0, 128, 64, 64), 4096),          # clamped at CONAN_ECHO_MAX_DELAY
          ((6000, 0, 4096, 128, 64, 64), None),
          ((0, 0, 1, 0, 0, 0), 0)]


def test_follow_rule():
    for args, want in FOLLOW:
        assert _lib.echo_delay_follow(*args) == want == R.follow(*args), args
    assert _lib.echo_delay_follow_keywords(16000) == dict(lead=128, hyst=64, max_age=64)
    assert _lib.echo_delay_follow_keywords(8000) == dict(lead=64, hyst=32, max_age=64)


def test_the_feature_table_is_unchanged():
    """The keywords the engine applies from the table are what they were; the estimator is a row of it that the engine applies itself,
    and its prototypes - the table's loop fills four of them - are the ones that were written out before."""
    assert [k for k, f in _lib.SLOT_FEATURES.items() if not f.engine_own] == ["eq", "level", "pitch", "follow", "register", "activity", "bypass", "conceal",
                                                                             "echo", "denoise", "comfort", "tones", "out_eq", "out_level", "watermark"]
    assert [k for k, f in _lib.SLOT_FEATURES.items() if f.engine_own] == ["echo_delay"]
    f = _lib.SLOT_FEATURES["echo_delay"]
    assert (f.cfg, f.on, f.build, f.keywords, f.noun) == (_lib.EchoDelayCfg, "enabled", _lib.echo_delay_cfg, _lib.echo_delay_keywords, "the estimator")
    assert (f.setter, f.getter, f.seed_state, f.seed_bytes) == ("conan_streams_set_echo_delay", "conan_streams_echo_delay_cfg", "conan_streams_echo_delay_state",
                                                                "conan_echo_delay_state_bytes")
    assert f.method == "set_echo_delay" and f.state is None and f.last is None and f.meta is None and f.stream and f.release and f.mirror is None
    v = C.c_void_p
    assert _lib._PROTOS["conan_streams_set_echo_delay"] == (C.c_int, [v, v, C.c_int, v, v, C.c_int64, v])
    assert _lib._PROTOS["conan_streams_echo_delay_cfg"] == (C.c_int, [v, C.c_int, v])
    assert _lib._PROTOS["conan_streams_echo_delay_state"] == (C.c_int, [v, v, C.c_int, v, C.c_int64, v])
    assert _lib._PROTOS["conan_streams_echo_delay"] == (C.c_int, [v, v, C.c_int, v, v, C.c_int64, v, C.c_int64, v, v])
    assert _lib._PROTOS["conan_echo_delay"] == (C.c_int, [v, v, C.c_int, v, C.c_int64, v, C.c_int64, C.c_int, v, v, C.c_int64, v, v])
    assert _lib._PROTOS["conan_echo_delay_state_bytes"] == (C.c_int64, [])


def _engine(n):
    from conan_amd.engine import StreamingVoiceConversionEngine as Engine
    eng = Engine.__new__(Engine)      # no context, no stream-set: the checks must come before either is touched
    eng.slots = list(range(n))
    eng._ed = types.SimpleNamespace(used=False, follow={}, last={}, pending=None)      # (what __init__ sets for the estimator)
    return eng


def test_engine_keyword_checks():
    from conan_amd.engine import StreamingVoiceConversionEngine as Engine
    cfg = _lib.echo_delay_cfg(8000)
    got = Engine._echo_delay_values([None, True, dict(n_lags=128, lead=9), False, cfg], True, 5)
    assert got == [None, {}, dict(n_lags=128, lead=9), None, _lib.echo_delay_keywords(8000)]
    eng = _engine(2)
    calls = [lambda **kw: eng.start_wav(kw.pop("ref_mel"), **kw), lambda **kw: eng.open_slots([0, 1], kw.pop("ref_mel"), **kw),
             lambda **kw: eng.infer_wav(None, kw.pop("ref_mel"), **kw), lambda **kw: eng.infer_wav_staggered([None, None], [0, 1], kw.pop("ref_mel"), **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="needs echo="):
            call(ref_mel=object(), echo_delay=True)
        with pytest.raises(ValueError, match="needs echo="):
            call(ref_mel=object(), echo=[True, None], echo_delay=[True, True])
        with pytest.raises(ValueError, match="3 values for 2"):
            call(ref_mel=object(), echo=True, echo_delay=[True, True, True])
        with pytest.raises(ValueError, match="echo_delay: 'on'"):
            call(ref_mel=object(), echo=True, echo_delay="on")
        with pytest.raises(ValueError, match="unknown fields"):
            call(ref_mel=object(), echo=True, echo_delay=dict(delay=3))
    # a stream-set that never used it is left alone: no setter call at all
    eng.st = types.SimpleNamespace()      # (any attribute access would raise)
    eng._apply_echo_delay(eng.slots, [None, None], [None, None])
    assert not eng._ed.used
    # once used, None turns a slot off; the fields travel as the cfg, the rule's keywords stay with the engine
    seen = []
    eng.st = types.SimpleNamespace(model_rate=16000, set_echo_delay=lambda slots, cfg=True, **kw: seen.append((list(slots), cfg, kw)))
    eng._apply_echo_delay(eng.slots, [dict(n_lags=128, lead=9), None], [8000, None])
    assert eng._ed.used and seen == [([0], dict(n_lags=128), dict(rate=8000)), ([1], None, {})]
    assert eng._ed.follow == {0: dict(lead=9, hyst=32, max_age=64)} and eng._ed.last == {0: (-1, 0)}
    eng._apply_echo_delay(eng.slots, [None, {}], [None, None])
    assert seen[2:] == [([0], None, {}), ([1], True, dict(rate=16000))] and eng._ed.follow == {1: dict(lead=128, hyst=64, max_age=64)}
    # the rule between calls: the report of the last call moves the canceller's delay through set_echo, fields only
    echo = {1: dict(taps=1024, delay=0)}
    eng.st = types.SimpleNamespace(echo_cfg=lambda slots: [echo.get(s) for s in slots], set_echo=lambda slots, cfg: echo.update({slots[0]: cfg}))
    done = types.SimpleNamespace(synchronize=lambda: None)
    host = types.SimpleNamespace(tolist=lambda: [[5, 0, 5, 9, 0, 0], [3000, 0, 3000, 9, 0, 0]])
    eng._ed.pending = ([0, 1], host, done, None)
    assert eng.echo_delays() == [(-1, 0, None), (3000, 0, 2872)] and echo[1] == dict(taps=1024, delay=2872) and eng._ed.pending is None
    eng._ed.pending = ([0, None], host, done, None)      # (a row without samples reports zeros: it is no estimate)
    assert eng.echo_delays([1]) == [(3000, 0, 2872)]
