"""The Python layer of ten per-slot features (input level, pitch, pitch follow, register, activity, bypass, comfort, output level,
concealment, echo delay), characterised without a GPU and without the built library: (a) runtime.Streams over a library stand-in that records every
C call - the symbol, the slot array, the cfg's bytes, the seed rows, the stream argument, the release of pipelined buffers - and (b) the
engine over a Streams stand-in that records every method call, bound through the real method's signature (so a cfg handed over by
position and one handed over by keyword read the same).  The expectations are built from _lib's builders, never from the code under
test.  The block at the end holds the two places where the layer is deliberately more regular than it once was."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest
import torch

from conan_amd import _lib, runtime
from conan_amd.engine import StreamingVoiceConversionEngine as Engine

H = C.c_void_p(0x1234)
STREAM = C.c_void_p(0)


class TPtr(C.c_void_p):
    """What the stand-in library gets for a tensor: the pointer, and the tensor itself in .t"""


def _tptr(t):
    p = TPtr(t.data_ptr() if t is not None else 0)
    p.t = t
    return p


class Lib:
    """Records (symbol, args): a slot array as a list, a byref'd struct as the struct, a tensor as the tensor.  script[symbol] may
    answer a call (fill a struct or a buffer, return a size)."""

    def __init__(self):
        self.calls, self.script = [], {}

    def __getattr__(self, name):
        def fn(*args):
            args = list(args)
            if len(args) > 2 and type(args[1]) is C.c_void_p and isinstance(args[2], int):
                args[1] = np.ctypeslib.as_array(C.cast(args[1], C.POINTER(C.c_int32)), (args[2],)).tolist() if args[2] else []
            args = [a.t if isinstance(a, TPtr) else getattr(a, "_obj", a) for a in args]
            self.calls.append((name, args))
            return self.script[name](*args) if name in self.script else 0
        return fn


@pytest.fixture
def st(monkeypatch):
    monkeypatch.setattr(runtime, "_stream", lambda: STREAM)
    monkeypatch.setattr(runtime, "_ptr", _tptr)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: None)
    s = runtime.Streams.__new__(runtime.Streams)
    s.lib, s.h, s.dev, s._keep = Lib(), H, torch.device("cpu"), []
    s.ctx = types.SimpleNamespace(hop=320)      # (model_rate = 16000)
    s.input_levels, s.output_levels, s.pitch_cfgs, s.echo_delays = {}, {}, {}, set()
    s.input_formats, s.output_formats, s.output_rates, s.input_rate_set = {}, {}, {}, False
    s.seg, s._last_wav_n = 4, 0
    s._release = lambda: s.lib.calls.append(("_release", []))
    return s


class Seed:
    """A stand-in for cuda uint8 [n, 24] seed rows, 32 bytes apart."""

    def __init__(self, n=2, dtype=torch.uint8, dims=2, cuda=True, inner=1):
        self.dtype, self.shape, self.is_cuda, self._dims, self._inner = dtype, (n, 24)[:dims], cuda, dims, inner

    def dim(self):
        return self._dims

    def stride(self, i):
        return (32, self._inner)[i]

    def data_ptr(self):
        return 0x5000


L, P, F0, R, A, B, CF, CC, ED = (_lib.level_cfg, _lib.pitch_cfg, _lib.f0_cfg, _lib.register_cfg, _lib.activity_cfg, _lib.bypass_cfg, _lib.comfort_cfg,
                                 _lib.conceal_cfg, _lib.echo_delay_cfg)
_A_STRUCT, _B_STRUCT, _CF_STRUCT, _CC_STRUCT, _ED_STRUCT = A(hold_frames=3), B(wet=0.25), CF(colour=2), CC(8000, fade=0), ED(8000, leak=3)

# (method, positional arguments after slots, keywords, the struct the C call must carry)
SETTER_CASES = [
    ("set_input_level", (), {}, L()),
    ("set_input_level", (True,), dict(clip=True), L(clip=True)),
    ("set_input_level", (dict(target=-18.0),), {}, L(target=-18.0)),
    ("set_input_level", (dict(target=-18.0, clip=True),), dict(target=-20.0), L(target=-20.0, clip=True)),
    ("set_input_level", (None,), {}, _lib.LevelCfg()),
    ("set_pitch", (), {}, P()),
    ("set_pitch", (dict(shift_semitones=2.0),), {}, P(shift_semitones=2.0)),
    ("set_pitch", (dict(shift_semitones=2.0, range=0.5),), dict(range=0.0), P(shift_semitones=2.0, range=0.0)),
    ("set_pitch", (None,), {}, _lib.PitchCfg()),
    ("set_pitch_follow", (), {}, F0()),
    ("set_pitch_follow", (dict(fmin=60.0),), {}, F0(fmin=60.0)),
    ("set_pitch_follow", (dict(fmin=60.0, fmax=500.0),), dict(fmax=400.0), F0(fmin=60.0, fmax=400.0)),
    ("set_pitch_follow", (None,), {}, _lib.F0Cfg()),
    ("set_pitch_register", (7.0,), {}, R(7.0)),
    ("set_pitch_register", (), dict(target=7.0, max_shift=0.5, prior=6.5, prior_frames=10, reseed=True), R(7.0, 0.5, prior=6.5, prior_frames=10, reseed=True)),
    ("set_pitch_register", (), dict(target=7.0, seed=(5, 12345)), R(7.0, seed=(5, 12345))),
    ("set_pitch_register", (), dict(cfg=dict(target=6.0, max_shift=1.0)), R(6.0, 1.0)),
    ("set_pitch_register", (7.0,), dict(cfg=dict(target=6.0), max_shift=0.5), R(6.0, 0.5)),      # (the dict wins over the explicit keywords)
    ("set_pitch_register", (), dict(cfg=None), _lib.RegisterCfg()),
    ("set_pitch_register", (7.0,), dict(cfg=None, max_shift=0.5), _lib.RegisterCfg()),      # (accepted silently)
    ("set_activity", (), {}, A()),
    ("set_activity", (), dict(gate=False), A(gate=False)),
    ("set_activity", (True,), dict(hold_frames=3), A(hold_frames=3)),
    ("set_activity", (dict(hold_frames=3),), {}, A(hold_frames=3)),
    ("set_activity", (dict(gate=False, hold_frames=3),), dict(hold_frames=5), A(gate=False, hold_frames=5)),
    ("set_activity", (dict(gate=True),), dict(gate=False), A(gate=True)),      # (gate= is the method's default: a dict's entry wins)
    ("set_activity", (_A_STRUCT,), {}, _A_STRUCT),
    ("set_activity", (None,), {}, _lib.ActivityCfg()),
    ("set_activity", (None,), dict(gate=False), _lib.ActivityCfg()),      # (gate= is no keyword of **kw)
    ("set_bypass", (), {}, B()),
    ("set_bypass", (), dict(wet=0.5, dry=0.5, ramp_ms=80.0, fill_gate=True, start=(0, 0), reseed=True), B(0.5, 0.5, 80.0, True, (0, 0), True)),
    ("set_bypass", (), dict(wet_db=-6.0, step=4096), B(wet_db=-6.0, step=4096)),
    ("set_bypass", (dict(wet=0.2, dry=0.8),), {}, B(wet=0.2, dry=0.8)),
    ("set_bypass", (dict(wet=0.2),), dict(wet=0.7, dry=0.3), B(wet=0.2, dry=0.3)),      # (the dict wins over the explicit keywords)
    ("set_bypass", (dict(wet=0.2),), dict(dry_db=-12.0), B(wet=0.2, dry_db=-12.0)),
    ("set_bypass", (_B_STRUCT,), {}, _B_STRUCT),
    ("set_bypass", (None,), {}, _lib.BypassCfg()),
    ("set_bypass", (None,), dict(wet=0.3), _lib.BypassCfg()),      # (accepted silently)
    ("set_bypass", (None,), dict(wet_db=-3.0), _lib.BypassCfg()),      # (accepted silently)
    ("set_comfort", (), {}, CF()),
    ("set_comfort", (dict(colour=2),), {}, CF(colour=2)),
    ("set_comfort", (dict(colour=2, seed=9),), dict(seed=11, follow=False), CF(colour=2, seed=11, follow=False)),
    ("set_comfort", (_CF_STRUCT,), {}, _CF_STRUCT),
    ("set_comfort", (None,), {}, _lib.ComfortCfg()),
    ("set_output_level", (), {}, L()),
    ("set_output_level", (dict(target=-18.0),), {}, L(target=-18.0)),
    ("set_output_level", (dict(target=-18.0, clip=True),), dict(target=-20.0), L(target=-20.0, clip=True)),
    ("set_output_level", (None,), {}, _lib.LevelCfg()),
    ("set_conceal", (), {}, CC(16000)),
    ("set_conceal", (), dict(rate=8000), CC(8000)),
    ("set_conceal", (True,), dict(rate=8000, fade=0), CC(8000, fade=0)),
    ("set_conceal", (dict(fade=0),), {}, CC(16000, fade=0)),
    ("set_conceal", (dict(fade=0, hold=3),), dict(hold=5, rate=48000), CC(48000, fade=0, hold=5)),
    ("set_conceal", (_CC_STRUCT,), {}, _CC_STRUCT),
    ("set_conceal", (None,), {}, _lib.ConcealCfg()),
    ("set_conceal", (None,), dict(rate=8000), _lib.ConcealCfg()),      # (rate= is no keyword of **kw)
    ("set_echo_delay", (), {}, ED(16000)),
    ("set_echo_delay", (), dict(rate=8000), ED(8000)),
    ("set_echo_delay", (True,), dict(rate=8000, leak=3), ED(8000, leak=3)),
    ("set_echo_delay", (dict(leak=3),), {}, ED(16000, leak=3)),
    ("set_echo_delay", (dict(leak=3, hold=3),), dict(hold=5, rate=48000), ED(48000, leak=3, hold=5)),
    ("set_echo_delay", (_ED_STRUCT,), {}, _ED_STRUCT),
    ("set_echo_delay", (_ED_STRUCT,), dict(hold=5), ED(8000, leak=3, hold=5)),      # (keywords over a struct's fields, as over a dict's)
    ("set_echo_delay", (None,), {}, _lib.EchoDelayCfg()),
    ("set_echo_delay", (False,), {}, _lib.EchoDelayCfg()),      # (the engine's "none")
    ("set_echo_delay", (None,), dict(rate=8000), _lib.EchoDelayCfg()),      # (rate= is no keyword of **fields)
    ("set_echo_delay", (8000,), {}, ED(8000)),      # (an integer rate stands for its defaults, as in Context.echo_delay)
]
# method -> (symbol, a stream argument, seed rows and a stride, the release of pipelined buffers, the slot-to-keywords dict and its reporter)
SETTERS = {
    "set_input_level": ("conan_streams_set_input_level", False, False, False, ("input_levels", _lib.level_keywords)),
    "set_pitch": ("conan_streams_set_pitch", True, False, True, ("pitch_cfgs", _lib.pitch_keywords)),
    "set_pitch_follow": ("conan_streams_set_pitch_follow", True, False, True, None),
    "set_pitch_register": ("conan_streams_set_pitch_register", True, False, True, None),
    "set_activity": ("conan_streams_set_activity", True, False, True, None),
    "set_bypass": ("conan_streams_set_bypass", True, False, True, None),
    "set_comfort": ("conan_streams_set_comfort", True, False, True, None),
    "set_output_level": ("conan_streams_set_output_level", True, True, False, ("output_levels", _lib.level_keywords)),
    "set_conceal": ("conan_streams_set_conceal", True, True, True, None),
    "set_echo_delay": ("conan_streams_set_echo_delay", True, True, True, None),
}


def _expect_setter(method, slots, cfg, seed=None):
    symbol, stream, seeded, release, _ = SETTERS[method]
    args = [H, list(slots), len(slots), bytes(cfg)] + ([seed, 32 if seed is not None else 0] if seeded else []) + ([STREAM] if stream else [])
    return [(symbol, args)] + ([("_release", [])] if release else [])


def _seen(calls):
    """The recorded calls with every struct as (its type, its bytes)."""
    return [(name, [bytes(a) if isinstance(a, C.Structure) else a for a in args]) for name, args in calls]


@pytest.mark.parametrize("case", range(len(SETTER_CASES)))
def test_streams_setter_calls(st, case):
    method, args, kw, cfg = SETTER_CASES[case]
    getattr(st, method)([5, 2], *args, **kw)
    assert len(st.lib.calls[0][1]) == 4 + 2 * SETTERS[method][2] + SETTERS[method][1]
    assert type(st.lib.calls[0][1][3]) is type(cfg)
    assert _seen(st.lib.calls) == _expect_setter(method, [5, 2], cfg)
    mirror = SETTERS[method][4]
    on = getattr(cfg, "enabled", 0)
    for name in ("input_levels", "output_levels", "pitch_cfgs"):
        want = {5: mirror[1](cfg), 2: mirror[1](cfg)} if mirror and mirror[0] == name and on else {}
        assert getattr(st, name) == want
    assert st.echo_delays == ({5, 2} if method == "set_echo_delay" and on else set())      # the set _far_stages reads


def test_streams_echo_delays_follow_the_setter(st):
    st.set_echo_delay([1, 2, 3], dict(leak=3))
    st.set_echo_delay([2], True)
    st.set_echo_delay([3, 7], None)
    assert st.echo_delays == {1, 2}
    st.set_echo_delay([1], False)
    assert st.echo_delays == {2}
    st.set_echo_delay(iter([4, 6]))      # (the slots may be any iterable: the set is kept from the list the call was made with)
    assert st.echo_delays == {2, 4, 6} and st.lib.calls[-2][1][1] == [4, 6]
    del st.lib.calls[:]
    with pytest.raises(ValueError, match="^echo_delay: 'on' is neither an _lib.EchoDelayCfg, a dict of its fields, a rate nor True$"):
        st.set_echo_delay([1], "on")
    assert st.lib.calls == [] and st.echo_delays == {2, 4, 6}


def test_streams_setters_keep_their_slot_dicts(st):
    for method, (_, _, _, _, mirror) in SETTERS.items():
        if mirror is None:
            continue
        table = getattr(st, mirror[0])
        getattr(st, method)([1, 2, 3], dict() if method == "set_pitch" else dict(target=-18.0))
        getattr(st, method)([2], True)
        getattr(st, method)([3, 7], None)
        first = _lib.pitch_cfg() if method == "set_pitch" else _lib.level_cfg(target=-18.0)
        second = _lib.pitch_cfg() if method == "set_pitch" else _lib.level_cfg()
        assert table == {1: mirror[1](first), 2: mirror[1](second)}
        assert table[1] is not table[2]
    assert set(st.input_levels) == set(st.output_levels) == set(st.pitch_cfgs) == {1, 2}


@pytest.mark.parametrize("method, noun", [("set_input_level", "the leveller"), ("set_pitch", "the pitch control"), ("set_pitch_follow", "following"),
                                          ("set_activity", "the detector"), ("set_comfort", "the comfort noise"), ("set_output_level", "the leveller"),
                                          ("set_conceal", "the concealment"), ("set_echo_delay", "the estimator")])
def test_streams_setters_off_takes_no_keywords(st, method, noun):
    kw = {"set_input_level": dict(target=-20.0), "set_pitch": dict(range=0.5), "set_pitch_follow": dict(fmin=60.0), "set_activity": dict(hold_frames=2),
          "set_comfort": dict(colour=0), "set_output_level": dict(clip=True), "set_conceal": dict(fade=0), "set_echo_delay": dict(leak=3)}[method]
    with pytest.raises(ValueError) as e:
        getattr(st, method)([0], None, **kw)
    assert str(e.value) == f"{method}: cfg=None turns {noun} off and takes no keywords"
    assert st.lib.calls == []


def test_streams_register_needs_a_target(st):
    with pytest.raises(ValueError, match="target="):
        st.set_pitch_register([0])
    assert st.lib.calls == []


@pytest.mark.parametrize("method, reader", [("set_output_level", "output_level_state"), ("set_conceal", "conceal_state"),
                                            ("set_echo_delay", "echo_delay_state")])
def test_streams_seeded_setters(st, method, reader):
    seed = Seed()
    fields, cfg = {"set_output_level": (dict(target=-18.0), L(target=-18.0)), "set_conceal": (dict(fade=0), CC(16000, fade=0)),
                   "set_echo_delay": (dict(leak=3), ED(16000, leak=3))}[method]
    getattr(st, method)([5, 2], fields, seed=seed)
    assert _seen(st.lib.calls) == _expect_setter(method, [5, 2], cfg, seed)
    del st.lib.calls[:]
    getattr(st, method)([5, 2], None, seed=seed)      # (the library decides what a seed beside "off" means)
    assert _seen(st.lib.calls) == _expect_setter(method, [5, 2], type(cfg)(), seed)
    del st.lib.calls[:]
    for bad in (Seed(dtype=torch.int32), Seed(dims=1), Seed(n=3), Seed(cuda=False), Seed(inner=2)):
        with pytest.raises(ValueError) as e:
            getattr(st, method)([5, 2], seed=bad)
        assert str(e.value) == f"{method}: seed must be a cuda uint8 [n, bytes] tensor, as {reader} returns it"
    assert st.lib.calls == []


def _fill(struct):
    def answer(h, slot, out):
        src = struct if slot == 0 else type(struct)()
        C.memmove(C.addressof(out), bytes(src), C.sizeof(src))
        return 0
    return answer


@pytest.mark.parametrize("method, symbol, struct, report", [
    ("pitch", "conan_streams_pitch", P(shift_semitones=2.0), _lib.pitch_keywords),
    ("pitch_follow", "conan_streams_pitch_follow", F0(fmin=60.0), _lib.f0_keywords),
    ("activity", "conan_streams_activity", A(gate=False, hold_frames=3), _lib.activity_keywords),
    ("bypass", "conan_streams_bypass", B(wet=0.25, dry=0.5), _lib.bypass_keywords),
    ("comfort", "conan_streams_comfort", CF(follow=False, colour=2), _lib.comfort_keywords),
    ("conceal_cfg", "conan_streams_conceal_cfg", CC(8000, fade=0), _lib.conceal_keywords),
    ("echo_delay_cfg", "conan_streams_echo_delay_cfg", ED(8000, leak=3), _lib.echo_delay_keywords)])
def test_streams_cfg_getters(st, method, symbol, struct, report):
    st.lib.script[symbol] = _fill(struct)
    assert getattr(st, method)([0, 6]) == [report(struct), None]
    assert [(name, args[:2], type(args[2])) for name, args in st.lib.calls] == [(symbol, [H, 0], type(struct)), (symbol, [H, 6], type(struct))]


@pytest.mark.parametrize("key, build, fields", [("conceal", _lib.conceal_cfg, dict(fade=0)), ("echo", _lib.echo_cfg, dict(mu_shift=2)),
                                                ("echo_delay", _lib.echo_delay_cfg, dict(leak=3))])
def test_rate_cfg_is_the_builder(key, build, fields):
    """runtime._rate_cfg, the cfg of the whole-signal calls: every form it takes gives the struct of the feature's _lib builder, byte for byte."""
    f = _lib.SLOT_FEATURES[key]
    assert f.build is build
    every = f.keywords(build(8000, **fields))      # every field, so no rate is needed
    struct = build(8000, **fields)
    for form, rate, want in ((True, 8000, build(8000)), (8000, None, build(8000)), (np.int64(48000), None, build(48000)), (8000, 16000, build(8000)),
                             (dict(fields), 8000, build(8000, **fields)), (every, None, build(8000, **fields)), (struct, None, struct), (struct, 16000, struct)):
        got = runtime._rate_cfg(key, form, rate)
        assert type(got) is f.cfg and bytes(got) == bytes(want), (key, form, rate)
    assert runtime._rate_cfg(key, struct) is struct
    with pytest.raises(ValueError) as e:
        runtime._rate_cfg(key, True)
    assert str(e.value) == f"{key}: True stands for a rate's defaults, and no rate is known here"
    for bad in (False, None, 8000.0, "on"):
        with pytest.raises(ValueError, match=f"^{key}: .* is neither an _lib.{f.cfg.__name__}, a dict of its fields, a rate nor True$"):
            runtime._rate_cfg(key, bad)
    with pytest.raises(ValueError, match="without a rate"):
        runtime._rate_cfg(key, dict(fields))      # a dict of some fields and no rate


def _rows(data):
    """A state reader's answer: the rows' bytes into the buffer handed over, whatever its dtype."""
    def answer(h, slots, n, buf, *rest):
        raw = torch.frombuffer(bytearray(b"".join(data[:n])), dtype=torch.uint8)
        buf.view(-1).view(torch.uint8).copy_(raw)
        return 0
    return answer


def test_streams_pitch_register(st):
    st.lib.script["conan_streams_pitch_register"] = _fill(R(7.0, 0.5))
    st.lib.script["conan_streams_pitch_register_state"] = _rows([np.array([4, 4 * 6 * _lib.REGISTER_UNIT], dtype=np.int64).tobytes()])
    got = st.pitch_register([3, 0, 5])
    assert got == [None, dict(target=7.0, max_shift=0.5, count=4, sum=4 * 6 * _lib.REGISTER_UNIT, mean=6.0, shift=0.5), None]
    name, args = st.lib.calls[3]
    assert name == "conan_streams_pitch_register_state" and args[:3] == [H, [0], 1] and args[4] is STREAM and len(args) == 5
    assert args[3].shape == (1, 2) and args[3].dtype == torch.int64
    assert st.lib.calls[4:] == [("_release", [])]


def test_streams_state_readers(st):
    act = [_lib.ActivityState(1, 2, 3, 0, 0.5, 7, 4), _lib.ActivityState(0, 0, 9, 0, 0.25, 8, 1)]
    st.lib.script["conan_streams_activity_state"] = _rows([bytes(s) for s in act])
    assert st.activity_state([4, 1]) == [dict(active=1, hang=2, level=3, floor=0.5, frames=7, active_frames=4),
                                         dict(active=0, hang=0, level=9, floor=0.25, frames=8, active_frames=1)]
    byp = [_lib.BypassState(11, 12, 13, 0), _lib.BypassState(21, 22, 23, 0)]
    st.lib.script["conan_streams_bypass_state"] = _rows([bytes(s) for s in byp])
    assert st.bypass_state([4, 1]) == [dict(wet=11, dry=12, dry_eff=13), dict(wet=21, dry=22, dry_eff=23)]
    com = [_lib.ComfortState(-5000, 0, 17), _lib.ComfortState(-6000, 0, 0)]
    st.lib.script["conan_streams_comfort_state"] = _rows([bytes(s) for s in com])
    assert st.comfort_state([4, 1]) == [dict(level=-5000, idle_frames=17), dict(level=-6000, idle_frames=0)]
    calls = [c for c in st.lib.calls if c[0] != "_release"]
    assert [c[0] for c in st.lib.calls] == ["conan_streams_activity_state", "_release", "conan_streams_bypass_state", "_release",
                                            "conan_streams_comfort_state", "_release"]
    for (name, args), size in zip(calls, (C.sizeof(_lib.ActivityState), 16, 16)):
        assert args[:3] == [H, [4, 1], 2] and args[4] is STREAM and len(args) == 5
        assert args[3].shape[0] == 2 and args[3].numel() * args[3].element_size() == 2 * size
    assert calls[0][1][3].dtype == torch.uint8 and calls[0][1][3].shape == (2, C.sizeof(_lib.ActivityState))
    assert calls[2][1][3].dtype == torch.uint8 and calls[2][1][3].shape == (2, 16)


@pytest.mark.parametrize("method, symbol", [("input_level", "conan_streams_input_level"), ("output_level", "conan_streams_output_level")])
def test_streams_level_rows(st, method, symbol):
    rows = np.arange(8, dtype=np.float64).reshape(2, 4)
    st.lib.script[symbol] = _rows([rows[0].tobytes(), rows[1].tobytes()])
    out = getattr(st, method)([4, 1])
    assert out.dtype == torch.float64 and out.shape == (2, 4) and out.tolist() == rows.tolist()
    (name, args), rel = st.lib.calls
    assert name == symbol and args[:3] == [H, [4, 1], 2] and args[3] is out and args[4] is STREAM and len(args) == 5 and rel == ("_release", [])


@pytest.mark.parametrize("method, symbol, size_symbol, size_args", [
    ("output_level_state", "conan_streams_output_level_state", "conan_streams_output_level_state_bytes", [H]),
    ("conceal_state", "conan_streams_conceal_state", "conan_conceal_state_bytes", []),
    ("echo_delay_state", "conan_streams_echo_delay_state", "conan_echo_delay_state_bytes", [])])
def test_streams_seed_rows(st, method, symbol, size_symbol, size_args):
    st.lib.script[size_symbol] = lambda *a: 24
    st.lib.script[symbol] = _rows([bytes(range(24)), bytes(range(24, 48))])
    out = getattr(st, method)([4, 1])
    assert out.dtype == torch.uint8 and out.shape == (2, 24) and out.flatten().tolist() == list(range(48))
    size, (name, args), rel = st.lib.calls
    assert size == (size_symbol, size_args) and rel == ("_release", [])
    assert name == symbol and args[:3] == [H, [4, 1], 2] and args[3] is out and args[4:] == [24, STREAM]


@pytest.mark.parametrize("method, symbol, k, dtype", [("step_wav_activity", "conan_step_wav_activity", 2, torch.int32),
                                                      ("step_wav_bypass", "conan_step_wav_bypass", 2, torch.int32),
                                                      ("step_wav_comfort", "conan_step_wav_comfort", 1, torch.int32),
                                                      ("step_wav_contour", "conan_step_wav_contour", 2, torch.float32)])
@pytest.mark.parametrize("n", [0, 3])
def test_streams_last_call_rows(st, method, symbol, k, dtype, n):
    st._last_wav_n = n
    out = getattr(st, method)()
    out = (out,) if k == 1 else out
    assert len(out) == k and all(t.shape == (n, st.seg) and t.dtype == dtype for t in out)
    (name, args), rel = st.lib.calls
    assert name == symbol and args[0] is H and args[-1] is STREAM and len(args) == k + 2 and rel == ("_release", [])
    assert all(b.shape == (max(n, 1), st.seg) and b.dtype == dtype for b in args[1:-1])
    assert len({b.data_ptr() for b in args[1:-1]}) == k


class Snapshot:
    """A stand-in for a SlotSnapshot of two streams: the first with a leveller and a pitch control, the second with neither."""
    level, pitch = _lib.level_keywords(_lib.level_cfg(target=-18.0)), _lib.pitch_keywords(_lib.pitch_cfg(range=0.5))

    def __init__(self):
        self.blob = torch.zeros(2, 256, dtype=torch.uint8)
        self.blob.record_stream = lambda s: None
        self.meta = bytes(2 * _lib.SLOT_META_BYTES)

    def __len__(self):
        return 2

    def info(self, i):
        return dict(in_format="f32", out_format="s16" if i == 0 else "f32", in_rate=None, out_rate=8000 if i == 0 else None,
                    level=self.level if i == 0 else None, pitch=self.pitch if i == 0 else None)


def test_import_slots_updates_the_slot_dicts(st):
    st.input_levels, st.pitch_cfgs, st.output_levels = {4: dict(old=1), 9: dict(old=2)}, {4: dict(old=3)}, {4: dict(old=4)}
    st.import_slots([9, 4], Snapshot())
    assert st.input_levels == {9: Snapshot.level} and st.pitch_cfgs == {9: Snapshot.pitch} and st.output_levels == {4: dict(old=4)}
    assert st.output_formats == {9: "s16"} and st.output_rates == {9: 8000}
    assert [c[0] for c in st.lib.calls] == ["conan_streams_import_slots", "_release"]


# ---- (b) the engine over a recording Streams -------------------------------------------------------------------------------------------


class RecStreams:
    """Records (method, the arguments as the real Streams method binds them); the dicts the engine reads are real."""

    def __init__(self):
        self.calls = []
        self.input_levels, self.output_levels, self.pitch_cfgs = {}, {}, {}
        self.input_formats, self.output_formats, self.output_rates = {}, {}, {}
        self.input_rate_set, self.output_ld, self.model_rate = False, 0, 16000

    def __getattr__(self, name):
        sig = inspect.signature(getattr(runtime.Streams, name))

        def method(*args, **kw):
            bound = dict(sig.bind(self, *args, **kw).arguments)
            del bound["self"]
            self.calls.append((name, bound))
        return method


def _engine(n=3):
    st = RecStreams()
    ctx = types.SimpleNamespace(cfg=types.SimpleNamespace(emf_segment=4, emf_right_context=1, voc_upsample=0), hop=320, streams=lambda *a, **kw: st)
    return Engine(ctx, n), st


REF = object()
BANK = types.SimpleNamespace(registers={0: 7.5, 2: 8.25})
CONCEAL = _lib.conceal_cfg(8000)
SINGLE = dict(level=True, pitch=dict(range=0.5), follow=True, register=7.25, activity=True, bypass=True, conceal=True, comfort=True, out_level=True)
LISTS = dict(level=[None, True, dict(target=-18.0)], pitch=[dict(range=0.5), None, True], follow=[True, None, dict(fmin=60.0)],
             register=["voice", 7.25, None], activity=["detect", None, dict(hold_frames=3)], bypass=[None, True, dict(dry=0.2)],
             conceal=[CONCEAL, None, dict(fade=0)], comfort=[dict(seed=9), True, None], out_level=[None, dict(clip=True), True])
NONE = {k: None for k in SINGLE}


def S(slot):
    return _lib.comfort_seed(slot)


def test_engine_start_wav_single_values():
    eng, st = _engine()
    eng.start_wav(REF, in_rate=8000, **SINGLE)
    assert st.calls == [
        ("reset", dict(slots=[0, 1, 2], which=15)),
        ("set_reference", dict(slots=[0, 1, 2], ref_mel=REF, ref_len=None)),
        ("set_pitch", dict(slots=[0], cfg=dict(range=0.5))), ("set_pitch", dict(slots=[1], cfg=dict(range=0.5))),
        ("set_pitch", dict(slots=[2], cfg=dict(range=0.5))),
        ("set_output_level", dict(slots=[0], cfg=True)), ("set_output_level", dict(slots=[1], cfg=True)), ("set_output_level", dict(slots=[2], cfg=True)),
        ("set_input_rate", dict(slots=[0, 1, 2], rate=8000)),
        ("set_input_level", dict(slots=[0], cfg=True)), ("set_input_level", dict(slots=[1], cfg=True)), ("set_input_level", dict(slots=[2], cfg=True)),
        ("set_pitch_follow", dict(slots=[0], cfg=True)), ("set_pitch_follow", dict(slots=[1], cfg=True)), ("set_pitch_follow", dict(slots=[2], cfg=True)),
        ("set_pitch_register", dict(slots=[0], cfg=dict(target=7.25))), ("set_pitch_register", dict(slots=[1], cfg=dict(target=7.25))),
        ("set_pitch_register", dict(slots=[2], cfg=dict(target=7.25))),
        ("set_activity", dict(slots=[0], cfg=dict(gate=True))), ("set_activity", dict(slots=[1], cfg=dict(gate=True))),
        ("set_activity", dict(slots=[2], cfg=dict(gate=True))),
        ("set_bypass", dict(slots=[0], cfg={})), ("set_bypass", dict(slots=[1], cfg={})), ("set_bypass", dict(slots=[2], cfg={})),
        ("set_conceal", dict(slots=[0], cfg=True, rate=8000)), ("set_conceal", dict(slots=[1], cfg=True, rate=8000)),
        ("set_conceal", dict(slots=[2], cfg=True, rate=8000)),
        ("set_comfort", dict(slots=[0], cfg=dict(seed=S(0)))), ("set_comfort", dict(slots=[1], cfg=dict(seed=S(1)))),
        ("set_comfort", dict(slots=[2], cfg=dict(seed=S(2)))),
    ]


def test_engine_start_wav_lists_then_nothing():
    eng, st = _engine()
    lists = dict(LISTS, level=dict(target=-18.0), out_level=dict(clip=True))      # (these two take one value for all slots here)
    eng.start_wav(None, voice=(BANK, [2, 1, 0]), **lists)
    assert st.calls == [
        ("reset", dict(slots=[0, 1, 2], which=15)),
        ("set_voice", dict(slots=[0, 1, 2], bank=BANK, ids=[2, 1, 0])),
        ("set_pitch", dict(slots=[0], cfg=dict(range=0.5))), ("set_pitch", dict(slots=[2], cfg=True)),
        ("set_output_level", dict(slots=[0], cfg=dict(clip=True))), ("set_output_level", dict(slots=[1], cfg=dict(clip=True))),
        ("set_output_level", dict(slots=[2], cfg=dict(clip=True))),
        ("set_input_level", dict(slots=[0], cfg=dict(target=-18.0))), ("set_input_level", dict(slots=[1], cfg=dict(target=-18.0))),
        ("set_input_level", dict(slots=[2], cfg=dict(target=-18.0))),
        ("set_pitch_follow", dict(slots=[0], cfg=True)), ("set_pitch_follow", dict(slots=[1], cfg=None)), ("set_pitch_follow", dict(slots=[2], cfg=dict(fmin=60.0))),
        ("set_pitch_register", dict(slots=[0], cfg=dict(target=8.25))), ("set_pitch_register", dict(slots=[1], cfg=dict(target=7.25))),
        ("set_pitch_register", dict(slots=[2], cfg=None)),
        ("set_activity", dict(slots=[0], cfg=dict(gate=False))), ("set_activity", dict(slots=[1], cfg=None)), ("set_activity", dict(slots=[2], cfg=dict(hold_frames=3))),
        ("set_bypass", dict(slots=[0], cfg=None)), ("set_bypass", dict(slots=[1], cfg={})), ("set_bypass", dict(slots=[2], cfg=dict(dry=0.2))),
        ("set_conceal", dict(slots=[0], cfg=CONCEAL, rate=None)), ("set_conceal", dict(slots=[1], cfg=None, rate=None)),
        ("set_conceal", dict(slots=[2], cfg=dict(fade=0), rate=None)),
        ("set_comfort", dict(slots=[0], cfg=dict(seed=9))), ("set_comfort", dict(slots=[1], cfg=dict(seed=S(1)))), ("set_comfort", dict(slots=[2], cfg=None)),
    ]
    # every keyword absent on the engine that has used each feature: the six features of the stream-set are turned off slot by slot;
    # level, pitch and out_level only in the slots whose Streams dict holds one
    del st.calls[:]
    st.input_levels, st.pitch_cfgs, st.output_levels = {1: {}}, {0: {}, 2: {}}, {2: {}}
    eng.start_wav(REF)
    assert st.calls == [
        ("reset", dict(slots=[0, 1, 2], which=15)),
        ("set_reference", dict(slots=[0, 1, 2], ref_mel=REF, ref_len=None)),
        ("set_pitch", dict(slots=[0], cfg=None)), ("set_pitch", dict(slots=[2], cfg=None)),
        ("set_output_level", dict(slots=[2], cfg=None)),
        ("set_input_level", dict(slots=[1], cfg=None)),
        ("set_pitch_follow", dict(slots=[0], cfg=None)), ("set_pitch_follow", dict(slots=[1], cfg=None)), ("set_pitch_follow", dict(slots=[2], cfg=None)),
        ("set_pitch_register", dict(slots=[0], cfg=None)), ("set_pitch_register", dict(slots=[1], cfg=None)), ("set_pitch_register", dict(slots=[2], cfg=None)),
        ("set_activity", dict(slots=[0], cfg=None)), ("set_activity", dict(slots=[1], cfg=None)), ("set_activity", dict(slots=[2], cfg=None)),
        ("set_bypass", dict(slots=[0], cfg=None)), ("set_bypass", dict(slots=[1], cfg=None)), ("set_bypass", dict(slots=[2], cfg=None)),
        ("set_conceal", dict(slots=[0], cfg=None, rate=None)), ("set_conceal", dict(slots=[1], cfg=None, rate=None)),
        ("set_conceal", dict(slots=[2], cfg=None, rate=None)),
        ("set_comfort", dict(slots=[0], cfg=None)), ("set_comfort", dict(slots=[1], cfg=None)), ("set_comfort", dict(slots=[2], cfg=None)),
    ]


def test_engine_fresh_engine_without_keywords_sets_nothing():
    eng, st = _engine()
    eng.start_wav(REF, **NONE)
    assert st.calls == [("reset", dict(slots=[0, 1, 2], which=15)), ("set_reference", dict(slots=[0, 1, 2], ref_mel=REF, ref_len=None))]
    del st.calls[:]
    eng.open_slots([2, 0], REF, **{k: False for k in NONE})
    assert st.calls == [("reset", dict(slots=[2, 0], which=15)), ("set_reference", dict(slots=[2, 0], ref_mel=REF, ref_len=None))]
    del st.calls[:]
    eng.start(REF)
    assert st.calls == [("reset", dict(slots=[0, 1, 2], which=7)), ("set_reference", dict(slots=[0, 1, 2], ref_mel=REF, ref_len=None))]


def test_engine_open_slots_single_values():
    eng, st = _engine()
    eng.open_slots([2, 0], REF, in_rate=[8000, None], **SINGLE)
    assert st.calls == [
        ("reset", dict(slots=[2, 0], which=15)),
        ("set_reference", dict(slots=[2, 0], ref_mel=REF, ref_len=None)),
        ("set_input_rate", dict(slots=[2], rate=8000)),
        ("set_input_level", dict(slots=[2], cfg=True)), ("set_input_level", dict(slots=[0], cfg=True)),
        ("set_pitch", dict(slots=[2], cfg=dict(range=0.5))), ("set_pitch", dict(slots=[0], cfg=dict(range=0.5))),
        ("set_pitch_follow", dict(slots=[2], cfg=True)), ("set_pitch_follow", dict(slots=[0], cfg=True)),
        ("set_pitch_register", dict(slots=[2], cfg=dict(target=7.25))), ("set_pitch_register", dict(slots=[0], cfg=dict(target=7.25))),
        ("set_activity", dict(slots=[2], cfg=dict(gate=True))), ("set_activity", dict(slots=[0], cfg=dict(gate=True))),
        ("set_bypass", dict(slots=[2], cfg={})), ("set_bypass", dict(slots=[0], cfg={})),
        ("set_conceal", dict(slots=[2], cfg=True, rate=8000)), ("set_conceal", dict(slots=[0], cfg=True, rate=None)),
        ("set_comfort", dict(slots=[2], cfg=dict(seed=S(2)))), ("set_comfort", dict(slots=[0], cfg=dict(seed=S(0)))),
        ("set_output_level", dict(slots=[2], cfg=True)), ("set_output_level", dict(slots=[0], cfg=True)),
    ]


def test_engine_open_slots_lists_then_nothing():
    eng, st = _engine(4)
    eng.open_slots([3, 1, 2], None, voice=(BANK, [2, 1, 0]), **LISTS)
    assert st.calls == [
        ("reset", dict(slots=[3, 1, 2], which=15)),
        ("set_voice", dict(slots=[3, 1, 2], bank=BANK, ids=[2, 1, 0])),
        ("set_input_level", dict(slots=[1], cfg=True)), ("set_input_level", dict(slots=[2], cfg=dict(target=-18.0))),
        ("set_pitch", dict(slots=[3], cfg=dict(range=0.5))), ("set_pitch", dict(slots=[2], cfg=True)),
        ("set_pitch_follow", dict(slots=[3], cfg=True)), ("set_pitch_follow", dict(slots=[1], cfg=None)), ("set_pitch_follow", dict(slots=[2], cfg=dict(fmin=60.0))),
        ("set_pitch_register", dict(slots=[3], cfg=dict(target=8.25))), ("set_pitch_register", dict(slots=[1], cfg=dict(target=7.25))),
        ("set_pitch_register", dict(slots=[2], cfg=None)),
        ("set_activity", dict(slots=[3], cfg=dict(gate=False))), ("set_activity", dict(slots=[1], cfg=None)), ("set_activity", dict(slots=[2], cfg=dict(hold_frames=3))),
        ("set_bypass", dict(slots=[3], cfg=None)), ("set_bypass", dict(slots=[1], cfg={})), ("set_bypass", dict(slots=[2], cfg=dict(dry=0.2))),
        ("set_conceal", dict(slots=[3], cfg=CONCEAL, rate=None)), ("set_conceal", dict(slots=[1], cfg=None, rate=None)),
        ("set_conceal", dict(slots=[2], cfg=dict(fade=0), rate=None)),
        ("set_comfort", dict(slots=[3], cfg=dict(seed=9))), ("set_comfort", dict(slots=[1], cfg=dict(seed=S(1)))), ("set_comfort", dict(slots=[2], cfg=None)),
        ("set_output_level", dict(slots=[1], cfg=dict(clip=True))), ("set_output_level", dict(slots=[2], cfg=True)),
    ]
    del st.calls[:]
    st.input_levels, st.pitch_cfgs, st.output_levels = {1: {}, 0: {}}, {3: {}}, {2: {}, 0: {}}
    eng.open_slots([1, 3], REF)
    assert st.calls == [
        ("reset", dict(slots=[1, 3], which=15)),
        ("set_reference", dict(slots=[1, 3], ref_mel=REF, ref_len=None)),
        ("set_input_level", dict(slots=[1], cfg=None)),
        ("set_pitch", dict(slots=[3], cfg=None)),
        ("set_pitch_follow", dict(slots=[1], cfg=None)), ("set_pitch_follow", dict(slots=[3], cfg=None)),
        ("set_pitch_register", dict(slots=[1], cfg=None)), ("set_pitch_register", dict(slots=[3], cfg=None)),
        ("set_activity", dict(slots=[1], cfg=None)), ("set_activity", dict(slots=[3], cfg=None)),
        ("set_bypass", dict(slots=[1], cfg=None)), ("set_bypass", dict(slots=[3], cfg=None)),
        ("set_conceal", dict(slots=[1], cfg=None, rate=None)), ("set_conceal", dict(slots=[3], cfg=None, rate=None)),
        ("set_comfort", dict(slots=[1], cfg=None)), ("set_comfort", dict(slots=[3], cfg=None)),
    ]


def test_engine_live_setters():
    eng, st = _engine(2)
    seed = object()
    eng.set_activity([1], hold_frames=2)
    eng.set_activity(cfg=None)
    eng.set_bypass([1], wet=0.0, dry=1.0)
    eng.set_comfort(None, dict(colour=0), seed=4)
    eng.set_conceal([0], hold=0, rate=8000)
    eng.set_pitch_follow([0], None)
    eng.set_pitch_register([1], target=7.0, reseed=True)
    eng.set_output_level([0], dict(clip=True), seed=seed, target=-20.0)
    eng.set_pitch([1], range=0.5)
    eng.set_pitch()
    assert st.calls == [
        ("set_activity", dict(slots=[1], cfg=True, kw=dict(hold_frames=2))),
        ("set_activity", dict(slots=[0, 1], cfg=None)),
        ("set_bypass", dict(slots=[1], cfg=True, wet=0.0, dry=1.0)),
        ("set_comfort", dict(slots=[0, 1], cfg=dict(colour=0), kw=dict(seed=4))),
        ("set_conceal", dict(slots=[0], cfg=True, rate=8000, kw=dict(hold=0))),
        ("set_pitch_follow", dict(slots=[0], cfg=None)),
        ("set_pitch_register", dict(slots=[1], target=7.0, reseed=True)),
        ("set_output_level", dict(slots=[0], cfg=dict(clip=True), seed=seed, kw=dict(target=-20.0))),
        ("set_pitch", dict(slots=[1], cfg=dict(range=0.5))),
        ("set_pitch", dict(slots=[0, 1], cfg=None)),
    ]
    # a live setter counts as use: the next utterance without the keyword turns the feature off in every slot
    del st.calls[:]
    eng.start_wav(REF)
    assert [name for name, _ in st.calls[2:]] == [m for m in ("set_pitch_follow", "set_pitch_register", "set_activity", "set_bypass", "set_conceal",
                                                              "set_comfort") for _ in range(2)]
    assert all(args["cfg"] is None for _, args in st.calls[2:])


def _entry_points(eng):
    return [lambda **kw: eng.start_wav(REF, **kw), lambda **kw: eng.open_slots([0, 1], REF, **kw), lambda **kw: eng.infer_wav(None, REF, **kw),
            lambda **kw: eng.infer_wav_staggered([None, None], [0, 1], REF, **kw)]


@pytest.mark.parametrize("keyword, bad, match", [
    ("register", "voices", "register: 'voices'"), ("register", "voice", "needs voice="),
    ("activity", "gate", "'gate'"), ("activity", 2.5, "activity: 2.5"),
    ("bypass", "on", "bypass: 'on'"), ("bypass", 1.5, "bypass: 1.5"),
    ("conceal", "on", "conceal: 'on'"), ("conceal", 8000, "conceal: 8000"),
    ("comfort", "on", "comfort: 'on'"), ("comfort", 1.5, "comfort: 1.5")])
def test_engine_host_checks_come_first(keyword, bad, match):
    eng, st = _engine(2)
    for call in _entry_points(eng):
        with pytest.raises(ValueError, match="3 values for 2"):
            call(**{keyword: [None, None, None]})
        with pytest.raises(ValueError, match=match):
            call(**{keyword: bad})
        with pytest.raises(ValueError, match=match):
            call(**{keyword: [None, bad]})
    assert st.calls == []


def test_engine_register_voice_checks():
    eng, st = _engine(2)
    for call in _entry_points(eng)[:2]:
        with pytest.raises(ValueError, match="not both and not neither"):
            call(register="voice", voice=(BANK, [0, 1]))
    calls = [lambda **kw: eng.start_wav(None, **kw), lambda **kw: eng.open_slots([0, 1], None, **kw), lambda **kw: eng.infer_wav(None, None, **kw),
             lambda **kw: eng.infer_wav_staggered([None, None], [0, 1], None, **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="3 voice ids for 2"):
            call(register="voice", voice=(BANK, [0, 2, 0]))
        with pytest.raises(ValueError, match="voice 1 has no register"):
            call(register=[None, "voice"], voice=(BANK, [0, 1]))
    assert st.calls == []


def test_engine_one_value_for_all_slots():
    eng, st = _engine(2)
    with pytest.raises(ValueError, match="in_format / level: one value for all slots"):
        eng.start_wav(REF, level=[True, True])
    with pytest.raises(ValueError, match="out_level: one value for all slots"):
        eng.start_wav(REF, out_level=[True, True])
    with pytest.raises(ValueError, match="out_level: one value for all slots"):
        eng.start(REF, out_level=[True, True])
    with pytest.raises(ValueError, match="out_level: 3 values for 2 utterances"):
        eng.infer_wav_staggered([None, None], [0, 1], REF, out_level=[True, True, True])
    assert st.calls == []


# ---- the two places where the layer is deliberately more regular than it was ------------------------------------------------------------
# 1. the lengths (and the types) of follow, level, pitch and out_level are checked like the others': a ValueError before anything runs,
#    in every entry point.  2. every setter of Streams takes its Cfg struct as cfg.


@pytest.mark.parametrize("keyword", ["follow", "level", "pitch", "out_level"])
def test_engine_host_checks_of_the_other_four(keyword):
    eng, st = _engine(2)
    calls = _entry_points(eng)
    for call in calls[1:] if keyword in ("level", "out_level") else calls:      # (start_wav takes one level / out_level for all slots)
        with pytest.raises(ValueError, match=f"{keyword}: 3 values for 2"):
            call(**{keyword: [None, None, None]})
    for call in calls:
        with pytest.raises(ValueError, match=f"{keyword}: 2.5"):
            call(**{keyword: 2.5})
    assert st.calls == []


@pytest.mark.parametrize("method, struct", [("set_input_level", L(target=-18.0)), ("set_pitch", P(range=0.5)), ("set_pitch_follow", F0(fmin=60.0)),
                                            ("set_pitch_register", R(7.0, 0.5)), ("set_output_level", L(clip=True))])
def test_streams_setters_take_their_struct(st, method, struct):
    getattr(st, method)([5, 2], cfg=struct)
    assert st.lib.calls[0][1][3] is struct
    assert _seen(st.lib.calls) == _expect_setter(method, [5, 2], struct)
    mirror = SETTERS[method][4]
    if mirror:
        assert getattr(st, mirror[0]) == {5: mirror[1](struct), 2: mirror[1](struct)}
