"""The signalling tones' Python layer without a GPU: the structs against the header's sizes, _lib.tone_cfg against the reference's
defaults, the keywords' round trip, _lib.tone_events, and the feature table's entry."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conan_amd import _lib
from tests import tone_ref as R

# (field, a value outside its range): the setter and the whole-signal calls answer CONAN_ERR_INVALID (tests/test_gpu_tone.py)
BAD = [("mode", 3), ("mode", -1), ("reseed", 2), ("thr", -1), ("thr", (1 << 62) + 1), ("twist_fwd_q8", 255), ("twist_rev_q8", 65536), ("sel", 0),
       ("sel", 65536), ("share_q8", -1), ("share_q8", 257), ("on_frames", 0), ("off_frames", 0), ("off_frames", (1 << 20) + 1), ("min_frames", -1),
       ("step", 0), ("step", (1 << 20) + 1), ("gain", -0.1), ("gain", 0.6), ("gain", float("nan")), ("reserved", 1), ("seed.cur", 16),
       ("seed.cand", -2), ("seed.sound", 16), ("seed.run", -1), ("seed.level", (1 << 20) + 1), ("seed.frames", -1), ("seed.events", (1 << 40) + 1),
       ("seed.reserved", 1)]


def put(c, field, value):
    """c.field = value, for a field of the cfg or ('seed.x') of its seed."""
    obj = c
    *path, name = field.split(".")
    for p in path:
        obj = getattr(obj, p)
    setattr(obj, name, value)


def test_structs_match_the_header():
    assert C.sizeof(_lib.ToneState) == 48 and C.sizeof(_lib.ToneCfg) == 104
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "conan_hip.h")).read()
    assert "conan_tone_state;        /* 48 bytes */" in header and "conan_tone_cfg;          /* 104 bytes */" in header
    for fields, struct in ((_lib.ToneState._fields_, "conan_tone_state"), (_lib.ToneCfg._fields_, "conan_tone_cfg")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n.strip() for decl in body.split(";") for n in re.sub(r"^\s*\w+\s", "", decl.strip()).split(",") if n.strip()]
        assert names == [n for n, *_ in fields], struct
    assert _lib.TONE_HOP_MAX == R.HOP_MAX == int(re.search(r"#define CONAN_TONE_HOP_MAX (\d+)", header).group(1))
    for sym in ("conan_tone_table", "conan_tones", "conan_tone_fill", "conan_streams_set_tones", "conan_streams_tones", "conan_streams_tone_state",
                "conan_step_wav_tones"):
        assert sym in _lib._PROTOS and re.search(r"\bint %s\(" % sym, header), sym


def test_defaults_are_the_reference_s():
    for hop in (320, 160, 480):
        c, r = _lib.tone_cfg(hop=hop), R.cfg(hop)
        assert c.mode == 2 and c.reseed == 0
        assert {k: getattr(c, k) for k in _lib.TONE_FIELDS} == {k: r[k] for k in _lib.TONE_FIELDS}
        assert c.gain == r["gain"] == 0.125
        assert {k: getattr(c.seed, k) for k in _lib.TONE_SEED} == R.seed() == _lib.TONE_SEED
    c = _lib.tone_cfg()
    assert (c.thr, c.twist_fwd_q8, c.twist_rev_q8, c.sel, c.share_q8, c.on_frames, c.off_frames, c.min_frames, c.step) == (171798692, 643, 1615, 8, 128, 2, 2, 3, 1 << 20)
    assert _lib.tone_cfg(regenerate=False).mode == 1 and _lib.tone_cfg(ramp_ms=60.0).step == (1 << 20) // 3 + 1 and _lib.tone_cfg(level_db=-30.0).thr > c.thr
    assert _lib.TONE_KEYS == R.KEYS


def test_keywords_round_trip():
    c = _lib.tone_cfg(regenerate=False, level_db=-33.0, twist_db=(5.0, 9.0), sel=6, share=0.4, on_frames=3, off_frames=4, min_frames=5, ramp_ms=100.0, gain=0.1,
                      seed=dict(R.seed(), cur=5, sound=5, level=77, frames=12, events=3))
    d = _lib.tone_cfg(**_lib.tone_keywords(c))
    assert bytes(c) == bytes(d)
    f = _lib.SLOT_FEATURES["tones"]
    assert (f.cfg, f.on, f.setter, f.getter, f.state, f.rows, f.last) == (_lib.ToneCfg, "mode", "conan_streams_set_tones", "conan_streams_tones",
                                                                           "conan_streams_tone_state", _lib.ToneState, "conan_step_wav_tones")
    names = list(_lib.SLOT_FEATURES)
    assert f.method == "set_tones" and names.index("tones") == names.index("comfort") + 1      # among the wav-in source features, in front of the output's


def test_tone_events():
    row = [-1, 4, 4, 4, -1, -1, 4, 4, 13, 13, -1, 15]
    assert _lib.tone_events(row) == [("4", 1, 3), ("4", 6, 2), ("0", 8, 2), ("D", 11, 1)] == R.events(row)
    assert _lib.tone_events([row, [-1] * 5, []]) == [R.events(row), [], []]
    assert _lib.tone_events([]) == [] and _lib.tone_events([[], row]) == [[], R.events(row)]
    for make in (np.asarray, torch.tensor, lambda r: torch.tensor(r, dtype=torch.int32)):      # one row is one row in every container
        assert _lib.tone_events(make(row)) == R.events(row)
        assert _lib.tone_events(make([row, row[::-1]])) == [R.events(row), R.events(row[::-1])]
    assert "".join(_lib.TONE_KEYS[4 * r + c] for r, c in ((0, 0), (1, 1), (3, 0), (3, 1), (3, 2), (0, 3))) == "15*0#A"


@pytest.mark.parametrize("field,value", BAD)
def test_bad_values_are_representable(field, value):
    c = _lib.tone_cfg()
    put(c, field, value)      # (the struct takes it: the library is what refuses it)
    assert bytes(c) != bytes(_lib.tone_cfg())
