"""CPU checks of the ragged waveform-in step (conan_step_wav_ragged / _async, added within ABI 9): the prototypes compile against
the header as plain C and match the ctypes binding, a null handle is CONAN_ERR_INVALID with a message, and the new front-end kernel
keeps mel_stream_kernel's resource budget."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conan_amd import _lib

NAMES = ("conan_step_wav_ragged", "conan_step_wav_ragged_async")


def test_ragged_prototypes_match_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not present")
    inc = os.path.dirname(_lib.HEADER_PATH)
    # -Werror rejects an assignment to a pointer of another function type (compiled only: nothing to link)
    protos = tmp_path / "protos.c"
    protos.write_text('#include "conan_hip.h"\n'
                      'typedef int (*ragged_fn)(conan_streams*, const int32_t*, int, const int32_t*, const int32_t*, const float*,\n'
                      '                         const conan_mel_cfg*, int32_t*, float*, float*, int32_t*, void*);\n'
                      'ragged_fn a = conan_step_wav_ragged, b = conan_step_wav_ragged_async;\n'
                      '#if CONAN_HIP_ABI_VERSION != 9\n#error the ragged step is additive: ABI 9 stays\n#endif\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(protos), "-o", str(tmp_path / "protos.o")], check=True)
    for name in NAMES:
        assert name in _lib.declared_symbols() and name in _lib._PROTOS
        res, args = _lib._PROTOS[name]
        assert res is C.c_int and len(args) == 12
    assert _lib.ABI_VERSION == 9


def test_ragged_null_handle_is_invalid():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.lib()
    assert lib.conan_abi_version() == 9
    emit = (C.c_int32 * 1)(7)
    samples, final = (C.c_int32 * 1)(1280), (C.c_int32 * 1)(0)
    mc = _lib.MelCfg(1024, 320, 1024, 80, 16000, 80.0, 7600.0, 1e-6, -6.0, 1.5, 0, 0, 0.0)
    for name in NAMES:
        rc = getattr(lib, name)(None, None, 1, samples, final, None, C.byref(mc), None, None, None, emit, None)
        assert rc == _lib.ERR_INVALID and b"null argument" in lib.conan_last_error()
        assert emit[0] == 7


def test_mel_stream_ragged_kernel_resources(tmp_path):
    """mel_stream_ragged_kernel runs beside the previous chunk's vocoder like mel_stream_kernel: no scratch, no spills, at most 64
    VGPRs + AGPRs, LDS only dynamic.  Its name must not hide mel_stream_kernel from a substring lookup."""
    from tests.test_kernel_resources import _find, _kernels
    ks = _kernels(tmp_path)
    k = _find(ks, "mel_stream_ragged_kernel")
    assert k["spill"] == 0 and k["scratch"] == 0, k
    assert k["vgpr"] + k["agpr"] <= 64, k
    assert k["lds"] == 0, k
    _find(ks, "mel_stream_kernel")
    _find(ks, "mel_stream_copy_kernel")
    s = _find(ks, "wav_rows_scatter_kernel")
    assert s["spill"] == 0 and s["scratch"] == 0 and s["lds"] == 0, s
