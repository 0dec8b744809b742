"""Per-slot pitch control (conan_pitch_cfg): the law's restatement, the ABI surface, and the boundary band the GPU tests rest on."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conan_amd import _lib
from oracle import conan as oconan
from tests import pitch_ref as P

SYMBOLS = ["conan_streams_set_pitch", "conan_streams_pitch", "conan_decoder_step_pitch", "conan_slot_meta_pitch"]
SILENT = 57


def _head(seed=0, rows=4000):
    """Synthetic head outputs (d0, d1) and codes: d1 spread over more than the 50 .. 900 Hz range, a few silent tokens."""
    r = np.random.default_rng(seed)
    d0 = r.normal(0, 0.5, rows).astype(np.float32)
    d1 = r.uniform(5.0, 10.5, rows).astype(np.float32)
    codes = r.integers(0, 100, rows)
    codes[::17] = SILENT
    return d0, d1, codes


# ------------------------------------------------------------------------------------------------------------------ the law

def test_disabled_is_the_oracle():
    d0, d1, codes = _head()
    uv = torch.from_numpy((d0 > 0) | (codes == SILENT))
    want = oconan.f0_to_coarse(oconan.denorm_f0(torch.from_numpy(d1.copy()), uv)).numpy()
    for cfg in (None,):
        got = P.law(d0, d1, codes, SILENT, cfg)
        safe = ~got["unsafe"]
        assert safe.mean() > 0.99
        assert np.array_equal(got["bins"][safe], want[safe])
        assert np.array_equal(got["uv"], uv.numpy())
    # an enabled cfg that asks for nothing is the same law
    same = P.law(d0, d1, codes, SILENT, {})
    assert np.array_equal(same["bins"], P.law(d0, d1, codes, SILENT, None)["bins"])


def test_an_octave_doubles_f0_before_the_clamp():
    d0, d1, codes = _head(1)
    v0, _ = P.law_v(d0, d1, codes, SILENT, None)
    v1, _ = P.law_v(d0, d1, codes, SILENT, dict(shift_semitones=12.0))
    np.testing.assert_allclose(np.exp2(v1), 2.0 * np.exp2(v0), rtol=1e-12)
    base, up = P.law(d0, d1, codes, SILENT, None), P.law(d0, d1, codes, SILENT, dict(shift_semitones=12.0))
    inside = (base["f0_voiced"] > 50.0) & (base["f0_voiced"] < 450.0)
    assert inside.sum() > 1000
    np.testing.assert_allclose(up["f0_voiced"][inside], 2.0 * base["f0_voiced"][inside], rtol=1e-12)
    assert (up["f0_voiced"] <= 900.0).all() and (up["f0_voiced"][base["f0_voiced"] >= 450.0] == 900.0).all()


def test_range_zero_is_the_pivots_bin_on_every_voiced_row():
    d0, d1, codes = _head(2)
    got = P.law(d0, d1, codes, SILENT, dict(range=0.0, pivot=7.25))
    pivot_bin = P.law(np.array([-1.0]), np.array([7.25]), np.array([0]), SILENT, None)["bins"][0]
    assert 1 < pivot_bin < 255
    assert (got["bins"][~got["uv"]] == pivot_bin).all() and (got["bins"][got["uv"]] == 1).all()
    assert got["uv"].any() and (~got["uv"]).any()


def test_uv_threshold_at_the_infinities():
    d0, d1, codes = _head(3)
    voiced = P.law(d0, d1, codes, SILENT, dict(uv_threshold=float("inf")))
    assert np.array_equal(voiced["uv"], codes == SILENT)                       # voiced wherever the code is not the silent token
    whisper = P.law(d0, d1, codes, SILENT, dict(uv_threshold=float("-inf")))
    assert whisper["uv"].all() and (whisper["bins"] == 1).all() and (whisper["f0"] == 0).all()


def test_a_contour_of_nan_and_inf_gives_bins_in_range():
    d0, d1, codes = _head(4, 64)
    f0 = np.tile(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 7.5, 0.0, 200.0], np.float32), 8)
    for uv in (None, np.zeros(64, np.float32), np.full(64, np.nan, np.float32)):
        for cfg in (None, dict(range=0.0), dict(range=4.0, shift_semitones=48.0), dict(shift_semitones=-48.0)):
            got = P.law(d0, d1, codes, SILENT, cfg, f0=f0, uv=uv)
            assert got["bins"].min() >= 1 and got["bins"].max() <= 255
            assert not got["uv"].any()                                        # no silent-token forcing with a contour; NaN > 0 is false
    got = P.law(d0, d1, codes, SILENT, None, f0=f0)
    assert list(got["bins"][:5]) == [1, 255, 1, 255, 1]


# ------------------------------------------------------------------------------------------------------------------ the ABI surface

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
    assert raw.conan_abi_version() == 9


def test_header_compiles_as_c_and_matches_the_mirror(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not present")
    inc = os.path.dirname(_lib.HEADER_PATH)
    fields = [f[0] for f in _lib.PitchCfg._fields_]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "conan_hip.h"\nint main(void) {\n  printf("%zu\\n", sizeof(conan_pitch_cfg));\n'
                   + "".join('  printf("%%zu\\n", offsetof(conan_pitch_cfg, %s));\n' % f for f in fields)
                   + '  printf("%zu\\n", sizeof(conan_slot_meta));\n  return 0;\n}\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [C.sizeof(_lib.PitchCfg)] + [getattr(_lib.PitchCfg, f).offset for f in fields] + [_lib.SLOT_META_BYTES]
    assert out[0] == 24


def test_invalid_cfgs_are_refused_before_any_gpu_use():
    lib = _lib_or_skip()
    one = (C.c_int32 * 1)(0)
    ok = _lib.pitch_cfg()
    fake = C.c_void_p(16)      # never dereferenced: the checks below come first
    assert lib.conan_streams_set_pitch(None, one, 1, C.byref(ok), None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_pitch(fake, one, 1, None, None) == _lib.ERR_INVALID
    assert lib.conan_streams_pitch(None, 0, C.byref(ok)) == _lib.ERR_INVALID
    bad = [dict(uv_threshold=float("nan")), dict(shift_semitones=48.5), dict(shift_semitones=-49.0), dict(shift_semitones=float("inf")),
           dict(shift_semitones=float("nan")), dict(range=-0.01), dict(range=4.01), dict(range=float("nan")), dict(pivot=float("inf")),
           dict(pivot=float("nan"))]
    cfgs = [_lib.pitch_cfg(**kw) for kw in bad]
    c = _lib.pitch_cfg()
    c.reserved = 1
    cfgs.append(c)
    for c in cfgs:
        assert lib.conan_streams_set_pitch(fake, one, 1, C.byref(c), None) == _lib.ERR_INVALID, (c.shift_semitones, c.range, c.pivot, c.uv_threshold)
    assert b"reserved" in lib.conan_last_error()


def test_meta_pitch_refuses_what_is_not_a_record():
    lib = _lib_or_skip()
    out = _lib.PitchCfg()
    zero = _lib.SlotMeta()
    assert lib.conan_slot_meta_pitch(None, C.byref(out)) == _lib.ERR_INVALID
    assert lib.conan_slot_meta_pitch(C.byref(zero), None) == _lib.ERR_INVALID
    assert lib.conan_slot_meta_pitch(C.byref(zero), C.byref(out)) == _lib.ERR_INVALID
    assert b"not a slot snapshot record" in lib.conan_last_error()
    rec = bytearray(_lib.SLOT_META_BYTES)      # magic "CNSN", version 1, size 256, flipped bytes where the cfg sits: a wrong checksum
    rec[0:4] = (0x4e534e43).to_bytes(4, "little")
    rec[4:8] = (1).to_bytes(4, "little")
    rec[8:12] = (256).to_bytes(4, "little")
    rec[232:256] = bytes([0xFF] * 24)
    bad = _lib.SlotMeta.from_buffer_copy(bytes(rec))
    assert lib.conan_slot_meta_pitch(C.byref(bad), C.byref(out)) == _lib.ERR_INVALID
    assert b"corrupted" in lib.conan_last_error()


# ------------------------------------------------------------------------------------------------------------------ the decoder restated

def test_decode_frames_pitch_with_nothing_set_is_decode_frames():
    hp, _, sd = P.model()
    ref, codes = P.inputs(2)
    for b in range(2):
        cache = oconan.style_pass(sd, hp, torch.from_numpy(ref[b:b + 1]))
        want = oconan.decode_frames(sd, hp, torch.from_numpy(codes[b:b + 1]), cache, {})
        got = P.decode_frames_pitch(sd, hp, codes[b:b + 1], cache, {})
        for k in ("uv_pred", "f0_denorm_pred", "pitch_bins", "uv", "decoder_inp", "mel_out"):
            assert torch.equal(got[k], want[k]), k
        # an override with the law's own bins changes nothing
        again = P.decode_frames_pitch(sd, hp, codes[b:b + 1], cache, {}, bins_override=got["pitch_bins"])
        assert torch.equal(again["mel_out"], want["mel_out"])


# ------------------------------------------------------------------------------------------------------------------ the boundary band

def _share(rows):
    return float(np.mean(np.concatenate([r["unsafe"] for r in rows])))


def test_boundary_band_of_every_gpu_case():
    """The GPU tests compare bins on the rows outside the band only; here the reference alone shows that this leaves them nearly
    every row (bins are about 1 unit wide and the band is 2e-3: about 0.2 % expected, 5 % allowed)."""
    shares = {}
    for name, (n, T, cfgs) in P.LAW_CASES.items():
        shares[name] = _share(P.reference_rows(n, 0, [(0, cfgs)], frames=P.FRAMES // T * T))
    shares["switch"] = _share(P.reference_rows(6, 0, [(0, P.ROW_CFGS), (P.SWITCH_FRAME, P.ALT_CFGS)]))
    for n in (2, 6):
        f0, uv = P.contour(n)
        shares["contour_n%d" % n] = _share(P.reference_rows(n, 0, [(0, [None] * n)], f0=f0, uv=uv))
        shares["contour_uvnone_n%d" % n] = _share(P.reference_rows(n, 0, [(0, [None] * n)], f0=f0))
        shares["contour_cfg_n%d" % n] = _share(P.reference_rows(n, 0, [(0, P.ROW_CFGS[:n])], f0=f0, uv=uv))
    for name, s in shares.items():
        print("unsafe share %-22s %.4f" % (name, s))
        assert s <= 0.05, (name, s)


def test_one_cfg_moves_the_voiced_bins():
    """A case in which no cfg moved a bin would show nothing: the +5 semitone row differs from its unshifted run on at least a
    quarter of the voiced frames."""
    base = P.reference_rows(6, 0, [(0, [None] * 6)])
    ctl = P.reference_rows(6, 0, [(0, P.ROW_CFGS)])
    voiced = ~base[1]["uv"]
    assert voiced.sum() >= 4
    moved = (base[1]["pitch_bins"] != ctl[1]["pitch_bins"]) & voiced
    assert moved.sum() >= voiced.sum() / 4
