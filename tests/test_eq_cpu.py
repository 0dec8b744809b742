"""The equaliser's library and Python layer without a GPU: the symbols, the header as plain C, the structs, null handles, the feature
table's rows and their order, the keywords' round trip, and the cfgs the library refuses as far as the host check runs without a
device."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conan_amd import _lib
from tests import eq_ref as R

SYMBOLS = ("conan_eq_design", "conan_eq", "conan_eq_state_bytes", "conan_streams_set_input_eq", "conan_streams_input_eq", "conan_streams_input_eq_state",
           "conan_streams_set_output_eq", "conan_streams_output_eq", "conan_streams_output_eq_state")
HP = R.cookbook("highpass", 16000.0, 80.0)
# (what is wrong, a function that makes an enabled cfg wrong): each is CONAN_ERR_INVALID before anything changes
BAD = [("enabled", lambda c: setattr(c, "enabled", 2)), ("no section", lambda c: setattr(c, "sections", 0)),
       ("five sections", lambda c: setattr(c, "sections", 5)), ("nan", lambda c: c.coef[0].__setitem__(1, float("nan"))),
       ("inf", lambda c: c.coef[0].__setitem__(0, float("inf"))), ("too large", lambda c: c.coef[0].__setitem__(0, 2.0 * _lib.EQ_MAX_COEF)),
       ("a2 = 1", lambda c: c.coef[0].__setitem__(4, 1.0)), ("a2 = -1", lambda c: c.coef[0].__setitem__(4, -1.0)),
       ("|a1| = 1 + a2", lambda c: c.coef[0].__setitem__(3, 1.0 + c.coef[0][4])), ("behind the last section", lambda c: c.coef[1].__setitem__(0, 1.0)),
       ("reserved", lambda c: c.reserved.__setitem__(2, 1)), ("origin < 0", lambda c: setattr(c, "origin", -1)),
       ("pos < origin", lambda c: (setattr(c, "origin", 5), setattr(c, "pos", 4)))]


def test_symbols_are_exported_and_declared():
    header = open(_lib.HEADER_PATH).read()
    lib = _lib.lib()
    for sym in SYMBOLS:
        assert sym in _lib._PROTOS and hasattr(lib, sym) and sym in _lib.declared_symbols(), sym
        assert re.search(r"\b(int|int64_t) %s\(" % sym, header), sym
    setter = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
    assert _lib._PROTOS["conan_streams_set_input_eq"] == setter == _lib._PROTOS["conan_streams_set_output_eq"] == _lib._PROTOS["conan_streams_set_watermark"]
    assert _lib._PROTOS["conan_streams_input_eq"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]) == _lib._PROTOS["conan_streams_output_eq"]
    assert _lib._PROTOS["conan_streams_input_eq_state"] == _lib._PROTOS["conan_streams_watermark_state"] == _lib._PROTOS["conan_streams_output_eq_state"]
    assert len(_lib._PROTOS["conan_eq"][1]) == 11 and _lib._PROTOS["conan_eq_state_bytes"] == (C.c_int64, [])


def test_header_is_plain_c_and_the_structs_match(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "conan_hip.h"\n#include <stdio.h>\nint main(void) { printf("%zu %zu %d %d\\n", sizeof(conan_eq_cfg), sizeof(conan_eq_state), '
                   'CONAN_EQ_MAX_SECTIONS, CONAN_EQ_SEG); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(_lib.HEADER_PATH), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(_lib.EqCfg), C.sizeof(_lib.EqState), _lib.EQ_MAX_SECTIONS, _lib.EQ_SEG] == [200, 592, 4, 128]
    header = open(_lib.HEADER_PATH).read()
    for fields, struct in ((_lib.EqCfg._fields_, "conan_eq_cfg"), (_lib.EqState._fields_, "conan_eq_state")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [re.sub(r"\[.*", "", n.strip()) for decl in body.split(";") for n in re.sub(r"^\s*\w+\s", "", decl.strip()).split(",") if n.strip()]
        assert names == [n for n, *_ in fields], struct
    for kind, code in _lib.EQ_KINDS.items():
        assert int(re.search(r"#define CONAN_EQ_%s (\d+)" % kind.upper(), header).group(1)) == code
    assert tuple(_lib.EQ_KINDS) == R.KINDS


def test_null_handles_are_invalid():
    lib = _lib.lib()
    c = _lib.eq_cfg([HP])
    slots = (C.c_int32 * 1)(0)
    assert lib.conan_eq(None, C.byref(c), None, 0, 1, None, None, 0, None, None, None) == _lib.ERR_INVALID
    for name in ("conan_streams_set_input_eq", "conan_streams_set_output_eq"):
        assert getattr(lib, name)(None, slots, 1, C.byref(c), None, 0, None) == _lib.ERR_INVALID
    for name in ("conan_streams_input_eq", "conan_streams_output_eq"):
        assert getattr(lib, name)(None, 0, C.byref(c)) == _lib.ERR_INVALID
    for name in ("conan_streams_input_eq_state", "conan_streams_output_eq_state"):
        assert getattr(lib, name)(None, slots, 1, None, 592, None) == _lib.ERR_INVALID
    assert lib.conan_eq_design(0, 16000.0, 100.0, 1.0, 0.0, None) == _lib.ERR_INVALID


def test_feature_table_rows_and_order():
    names = list(_lib.SLOT_FEATURES)
    assert names.index("eq") == names.index("level") - 1 and names.index("out_eq") == names.index("out_level") - 1
    assert names.index("tones") == names.index("comfort") + 1 and names[-1] == "watermark"
    assert names.index("conceal") < names.index("denoise") < names.index("out_level")
    for key, side in (("eq", "input"), ("out_eq", "output")):
        f = _lib.SLOT_FEATURES[key]
        assert (f.cfg, f.on, f.build, f.keywords) == (_lib.EqCfg, "enabled", _lib.eq_cfg, _lib.eq_keywords)
        assert (f.setter, f.getter, f.seed_state, f.seed_bytes) == ("conan_streams_set_%s_eq" % side, "conan_streams_%s_eq" % side,
                                                                    "conan_streams_%s_eq_state" % side, "conan_eq_state_bytes")
        assert f.method == "set_%s_eq" % side and f.state is None and f.mirror is None and f.stream


def test_keywords_round_trip():
    c = _lib.eq_cfg([HP, dict(kind="notch", f=50.0, q=30.0), dict(kind="peak", f=2500.0, q=1.0, gain_db=6.0)], rate=16000.0, origin=640, pos=1000)
    d = _lib.eq_cfg(**_lib.eq_keywords(c))
    assert bytes(c) == bytes(d) and c.sections == 3 and (c.origin, c.pos) == (640, 1000)
    assert tuple(c.coef[0]) == HP and tuple(c.coef[3]) == (0.0,) * 5
    assert _lib.eq_cfg([HP]).pos == 0
    with pytest.raises(ValueError):
        _lib.eq_cfg([dict(kind="notch", f=50.0)])      # a designed section needs the rate
    with pytest.raises(ValueError):
        _lib.eq_cfg([HP] * 5)
    with pytest.raises(ValueError):
        _lib.eq_cfg()


@pytest.mark.parametrize("what,spoil", BAD, ids=[b[0] for b in BAD])
def test_refused_cfgs_are_refused_by_the_host_check(what, spoil):
    """The cfg check runs before the handle is touched: with every other argument in place but the device, a good cfg gets as far as the
    handle (a null slot list: CONAN_ERR_INVALID too, so the good cfg is told apart by the error's text) and a bad one is named."""
    lib = _lib.lib()
    c = _lib.eq_cfg([HP])
    spoil(c)
    assert bytes(c) != bytes(_lib.eq_cfg([HP]))      # (the struct takes it: the library is what refuses it)
    fake = C.c_void_p(1)      # never dereferenced: the cfg check comes first
    slots = (C.c_int32 * 1)(0)
    for name in ("conan_streams_set_input_eq", "conan_streams_set_output_eq"):
        assert getattr(lib, name)(fake, slots, 1, C.byref(c), None, 0, None) == _lib.ERR_INVALID
        msg = lib.conan_last_error().decode()
        assert name in msg and "null" not in msg, (what, msg)
    assert lib.conan_eq(fake, C.byref(c), fake, 8, 1, slots, fake, 8, None, None, None) == _lib.ERR_INVALID
    assert "conan_eq:" in lib.conan_last_error().decode()


def test_design_is_the_reference_s():
    for kind in R.KINDS:
        got, want = _lib.eq_section(kind, 16000.0, 1000.0, 0.9, 3.0), R.cookbook(kind, 16000.0, 1000.0, 0.9, 3.0)
        assert all(abs(a - b) <= 64.0 * 2.0 ** -52 * max(1.0, abs(b)) for a, b in zip(got, want)), kind
