"""CPU checks of the sample formats (conan_streams_set_input_format / _output_format, conan_convert_samples, added within ABI 9):
the numpy restatement of the header's rules (tests/sample_format_ref.py) against the pinned facts of ITU-T G.711 and against
audioop where the interpreter has it, float -> s16 rounding at ties, the exported symbols with null handles, the header's
prototypes against the ctypes binding, and the resource budgets of the kernels that carry the formats."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conan_amd import _lib
from tests import sample_format_ref as sf

NAMES = ("conan_streams_set_input_format", "conan_streams_set_output_format", "conan_convert_samples")
CODES = np.arange(256, dtype=np.uint8)
S16 = np.arange(-32768, 32768, dtype=np.int64)


@pytest.mark.parametrize("fmt,total,peak,worst,sha", [("ulaw", 1532928, 32124, 644, "81d633c9e6972a18"), ("alaw", 1564672, 32256, 512, "38488f6fd710f468")])
def test_pinned_facts(fmt, total, peak, worst, sha):
    v = sf.decode_int(CODES, fmt)
    assert int(np.abs(v).sum()) == total
    assert int(v.max()) == peak and int(v.min()) == -peak
    back = sf.encode_int(v, fmt)
    odd = {0x7F: 0xFF} if fmt == "ulaw" else {}        # mu-law's negative zero comes back as positive zero
    for b in range(256):
        assert int(back[b]) == odd.get(b, b), (fmt, b, int(back[b]))
    table = sf.encode_int(S16, fmt)
    rt = sf.decode_int(table, fmt)
    assert (np.diff(rt) >= 0).all()
    assert int(np.abs(rt - S16).max()) == worst
    assert hashlib.sha256(table.astype(np.uint8).tobytes()).hexdigest().startswith(sha)
    # decoding is exact in float32: at most 16 significant bits
    x = sf.decode(CODES, fmt)
    assert x.dtype == np.float32 and np.array_equal(x.astype(np.float64) * 32768.0, v.astype(np.float64))


def test_against_audioop():
    audioop = pytest.importorskip("audioop")
    pcm = S16.astype("<i2").tobytes()
    assert sf.encode_int(S16, "ulaw").tobytes() == audioop.lin2ulaw(pcm, 2)
    assert sf.encode_int(S16, "alaw").tobytes() == audioop.lin2alaw(pcm, 2)
    assert sf.decode_int(CODES, "ulaw").astype("<i2").tobytes() == audioop.ulaw2lin(CODES.tobytes(), 2)
    assert sf.decode_int(CODES, "alaw").astype("<i2").tobytes() == audioop.alaw2lin(CODES.tobytes(), 2)


def test_s16_rounds_to_nearest_even_and_saturates():
    got = dict(zip([float(t) for t in sf.TIES], sf.quantize(sf.TIES).tolist()))
    for k in (0, 1, 2, 3, 100, 101, 32766, -1, -2, -3, -4, -101, -102):
        want = k if k % 2 == 0 else k + 1              # (k + 0.5) lies between k and k + 1: the even one
        assert got[(k + 0.5) / 32768] == want, (k, got[(k + 0.5) / 32768])
    assert got[32767.5 / 32768] == 32767 and got[-32767.5 / 32768] == -32768 and got[-32768.5 / 32768] == -32768
    assert got[1.0] == 32767 and got[-1.0] == -32768 and got[1.5] == 32767 and got[-1.5] == -32768
    assert got[0.0] == 0 and got[2.0 ** -20] == 0 and got[-2.0 ** -20] == 0
    assert sf.quantize(np.float32(-0.0)) == 0
    # every s16 value is a fixed point, and the tie list is what it claims to be in float32
    assert np.array_equal(sf.quantize(sf.decode(S16, "s16")), S16)
    assert np.array_equal(sf.encode(sf.decode(S16, "s16"), "s16"), S16.astype(np.int16))
    assert all(float(np.float32(t)) == float(t) for t in sf.TIES)


def test_symbols_exported_and_null_handles():
    lib = _lib.lib()
    assert lib.conan_abi_version() == 9
    for name in NAMES:
        assert getattr(lib, name) is not None and name in _lib.declared_symbols() and name in _lib._PROTOS
    slots = (C.c_int32 * 1)(0)
    assert lib.conan_streams_set_input_format(None, slots, 1, _lib.SAMPLE_S16) == _lib.ERR_INVALID
    assert b"null" in lib.conan_last_error()
    assert lib.conan_streams_set_output_format(None, slots, 1, _lib.SAMPLE_ULAW) == _lib.ERR_INVALID
    assert lib.conan_convert_samples(None, 0, None, 1, 1, None, 1, 1, 1, None) == _lib.ERR_INVALID
    assert _lib.sample_format(None) == _lib.SAMPLE_F32 and _lib.sample_format("alaw") == _lib.SAMPLE_ALAW
    with pytest.raises(ValueError):
        _lib.sample_format("s24")


def test_header_constants_and_prototypes(tmp_path):
    if subprocess.run(["which", "gcc"], capture_output=True).returncode:
        pytest.skip("gcc not present")
    inc = os.path.dirname(_lib.HEADER_PATH)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include "conan_hip.h"\n'
                     '#if CONAN_HIP_ABI_VERSION != 9\n#error the sample formats are additive: ABI 9 stays\n#endif\n'
                     'typedef int (*fmt_fn)(conan_streams*, const int32_t*, int, int);\n'
                     'typedef int (*conv_fn)(conan_ctx*, int, const void*, int64_t, int, void*, int64_t, int, int64_t, void*);\n'
                     'fmt_fn a = conan_streams_set_input_format, b = conan_streams_set_output_format; conv_fn c = conan_convert_samples;\n'
                     'int main(void) { printf("%d %d %d %d\\n", CONAN_SAMPLE_F32, CONAN_SAMPLE_S16, CONAN_SAMPLE_ULAW, CONAN_SAMPLE_ALAW); return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(probe), "-o", str(tmp_path / "probe.o")], check=True)
    txt = open(_lib.HEADER_PATH).read()
    for name, val in (("F32", _lib.SAMPLE_F32), ("S16", _lib.SAMPLE_S16), ("ULAW", _lib.SAMPLE_ULAW), ("ALAW", _lib.SAMPLE_ALAW)):
        assert "#define CONAN_SAMPLE_%-4s %d" % (name, val) in txt, name
    P = _lib._PROTOS
    assert P["conan_streams_set_input_format"] == P["conan_streams_set_output_format"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int])
    assert P["conan_convert_samples"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p])
    assert _lib.SAMPLE_BYTES == sf.BYTES and set(_lib.SAMPLE_FORMATS) == set(sf.BYTES)


def test_format_kernel_resources(tmp_path):
    """The kernels that decode and encode keep the resampler kernels' budget: no scratch, no spills, at most 64 VGPRs + AGPRs, LDS
    only dynamic (convert_samples_kernel: none at all)."""
    from tests.test_kernel_resources import _find, _kernels
    ks = _kernels(tmp_path)
    for name in ("resample_stream_kernel", "resample_out_kernel", "convert_samples_kernel"):
        k = _find(ks, name)
        assert k["spill"] == 0 and k["scratch"] == 0 and k["lds"] == 0, (name, k)
        assert k["vgpr"] + k["agpr"] <= 64, (name, k)
        print(name, k)
