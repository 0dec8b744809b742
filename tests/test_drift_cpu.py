"""Clock-drift compensation without a GPU: the symbols in the header and the binding, the entry points' argument errors, the ppm ->
ppb rounding and schedule forms, and the engine's drift= keyword over a recording Streams."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conan_amd import _lib
from tests.conftest import REPO
from tests.test_slot_features_cpu import REF, Engine, RecStreams
import types

SYMBOLS = ["conan_resample_drift", "conan_resample_drift_length", "conan_resample_drift_table", "conan_streams_set_input_drift",
           "conan_streams_input_drift", "conan_streams_set_output_drift", "conan_streams_output_drift"]


def test_symbols_in_header_binding_and_library():
    header = open(os.path.join(REPO, "include", "conan_hip.h")).read()
    lib = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib._PROTOS and hasattr(lib, name), name
    for macro, value in (("CONAN_DRIFT_SOURCE", _lib.DRIFT_SOURCE), ("CONAN_DRIFT_SINK", _lib.DRIFT_SINK), ("CONAN_DRIFT_MAX_PPB", _lib.DRIFT_MAX_PPB),
                         ("CONAN_DRIFT_MAX_SEGMENTS", _lib.DRIFT_MAX_SEGMENTS)):
        assert re.search(r"#define %s %d\b" % (macro, value), header), macro
    assert lib.conan_abi_version() == 9      # added within ABI 9: the symbol is the detection


def test_entry_points_refuse_null_arguments():
    lib = _lib.lib()
    ppb = (C.c_int32 * 1)(0)
    slots = (C.c_int32 * 1)(0)
    cfg = _lib.resample_cfg(8000, 16000)
    for fn in (lib.conan_streams_set_input_drift, lib.conan_streams_set_output_drift):
        assert fn(None, slots, 1, C.byref(cfg), ppb) == _lib.ERR_INVALID and b"null argument" in lib.conan_last_error()
    for fn in (lib.conan_streams_input_drift, lib.conan_streams_output_drift):
        assert fn(None, slots, 1, None, None, None) == _lib.ERR_INVALID
    assert lib.conan_resample_drift(None, C.byref(cfg), 0, None, 1, 10, None, None, 1, None, 10, None, None) == _lib.ERR_INVALID
    assert lib.conan_resample_drift_table(None, None, None, 0) == _lib.ERR_INVALID
    at = (C.c_int64 * 1)(0)
    assert lib.conan_resample_drift_length(None, 0, 10, at, ppb, 1) == -1
    assert lib.conan_resample_drift_length(C.byref(cfg), 0, -1, at, ppb, 1) == -1
    assert lib.conan_resample_drift_length(C.byref(cfg), 0, 10, None, ppb, 1) == -1


def test_ppm_to_ppb_rounding():
    assert _lib.drift_ppb(100) == 100000 and _lib.drift_ppb(-150.0) == -150000
    assert _lib.drift_ppb(0.0004) == 0 and _lib.drift_ppb(0.0006) == 1 and _lib.drift_ppb(-0.0006) == -1
    assert _lib.drift_ppb(0.0015) == round(0.0015 * 1000) and _lib.drift_ppb(123.4567) == 123457
    assert _lib.drift_ppb(2000.0) == _lib.DRIFT_MAX_PPB and _lib.drift_ppb(-2000.0) == -_lib.DRIFT_MAX_PPB
    for bad in (2000.001, -2000.001, 1e9):
        with pytest.raises(ValueError):
            _lib.drift_ppb(bad)
    assert _lib.drift_ppb_rows(3.0, 2).tolist() == [3000, 3000] and _lib.drift_ppb_rows([1.0, -2.0], 2).dtype == np.int32
    with pytest.raises(ValueError):
        _lib.drift_ppb_rows([1.0], 2)


def test_schedule_forms():
    at, ppb = _lib.drift_schedule(300.0)
    assert at.tolist() == [0] and ppb.tolist() == [300000] and at.dtype == np.int64 and ppb.dtype == np.int32
    at, ppb = _lib.drift_schedule([(0, 1.0), (257, -2.5), (1000, 0)])
    assert at.tolist() == [0, 257, 1000] and ppb.tolist() == [1000, -2500, 0]
    for bad in ([(1, 0.0)], [(0, 0.0), (5, 1.0), (5, 2.0)], [(0, 0.0), (5, 1.0), (4, 2.0)], [], [(k, 0.0) for k in range(_lib.DRIFT_MAX_SEGMENTS + 1)]):
        with pytest.raises(ValueError):
            _lib.drift_schedule(bad)
    with pytest.raises(ValueError):
        _lib.drift_side("both")
    assert _lib.resample_drift_length(16000, 16000, 1000, 0.0) == 1000 == _lib.resample_drift_length(16000, 16000, 1000, 0.0, side="sink")
    assert _lib.resample_drift_length(16000, 16000, 1000000, 1000.0) < 1000000 < _lib.resample_drift_length(16000, 16000, 1000000, 1000.0, side="sink")


class DriftStreams(RecStreams):
    def __init__(self):
        super().__init__()
        self.input_drifts, self.output_drifts = set(), set()


def _engine(n=3, st=None):
    st = st or DriftStreams()
    ctx = types.SimpleNamespace(cfg=types.SimpleNamespace(emf_segment=4, emf_right_context=1, voc_upsample=0), hop=320, streams=lambda *a, **kw: st)
    return Engine(ctx, n), st


def _drift_calls(st):
    return [(name, b["slots"], b["ppm"], b["rate"]) for name, b in st.calls if name in ("set_input_drift", "set_output_drift")]


def test_engine_keyword_normalisation():
    assert Engine._drift_values(None, 2) == [None, None] and Engine._drift_values(False, 2) == [None, None]
    assert Engine._drift_values(12, 2) == [12.0, 12.0] and Engine._drift_values([None, -3.5], 2) == [None, -3.5]
    for bad in (True, "fast", dict(ppm=1), 2000.5):
        with pytest.raises(ValueError):
            Engine._drift_values(bad, 1)
    with pytest.raises(ValueError):
        Engine._drift_values([1.0], 2)


def test_engine_start_wav_sets_both_sides():
    eng, st = _engine(2)
    eng.start_wav(REF, in_rate=8000, out_rate=48000, drift=120.0)
    calls = _drift_calls(st)
    assert calls == [("set_output_drift", [0], 120.0, 48000), ("set_output_drift", [1], 120.0, 48000),
                     ("set_input_drift", [0], 120.0, 8000), ("set_input_drift", [1], 120.0, 8000)]
    names = [c[0] for c in st.calls]
    assert names.index("set_output_rate") < names.index("set_output_drift") and names.index("set_input_rate") < names.index("set_input_drift")
    with pytest.raises(ValueError):
        eng.start_wav(REF, drift=[1.0, 2.0])      # one value here; open_slots takes one per slot


def test_engine_start_is_output_only_and_none_is_silent():
    eng, st = _engine(2)
    eng.start(REF, drift=-40.0)
    assert _drift_calls(st) == [("set_output_drift", [0], -40.0, 16000), ("set_output_drift", [1], -40.0, 16000)]
    eng2, st2 = _engine(2)
    eng2.start_wav(REF)
    assert _drift_calls(st2) == []


def test_engine_open_slots_per_slot_and_set_drift():
    eng, st = _engine(3)
    eng.open_slots([2, 0], REF, in_rate=[8000, None], drift=[None, 55.0])
    assert _drift_calls(st) == [("set_output_drift", [0], 55.0, 16000), ("set_input_drift", [0], 55.0, 16000)]
    st.input_drifts, st.output_drifts = {0}, {0, 1}
    st.calls.clear()
    eng.set_drift([0, 1], 70.0)
    assert [(n, b["slots"], b["ppm"], b.get("rate")) for n, b in st.calls] == [("set_input_drift", [0], 70.0, None), ("set_output_drift", [0, 1], 70.0, None)]
    with pytest.raises(ValueError):
        eng.set_drift([2], 1.0)                    # a slot without drift
    with pytest.raises(ValueError):
        eng.set_drift([0], 2500.0)
