"""CPU checks of the waveform-in step's C-ABI (ABI 9): the header compiled as plain C agrees with the ctypes binding, the
library exports the new entry points, and a null handle is CONAN_ERR_INVALID with a message."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conan_amd import _lib


def test_abi9_header_matches_binding(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not present")
    inc = os.path.dirname(_lib.HEADER_PATH)
    # the values: built, run, and compared with what the ctypes binding declares
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "conan_hip.h"\n'
                     'int main(void) {\n'
                     '  printf("%d %d %zu %zu %zu\\n", CONAN_HIP_ABI_VERSION, CONAN_MODEL_FRONTEND, sizeof(conan_mel_cfg),\n'
                     '         offsetof(conan_mel_cfg, natural_log), offsetof(conan_mel_cfg, mag_eps));\n'
                     '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, str(probe), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [_lib.ABI_VERSION, _lib.MODEL_FRONTEND, C.sizeof(_lib.MelCfg), _lib.MelCfg.natural_log.offset, _lib.MelCfg.mag_eps.offset]
    assert out[:2] == [9, 8]
    # the prototypes: -Werror rejects an assignment to a pointer of another function type (compiled only: nothing to link)
    protos = tmp_path / "protos.c"
    protos.write_text('#include "conan_hip.h"\n'
                      'typedef int (*step_wav_fn)(conan_streams*, const int32_t*, int, int, int, const float*, const conan_mel_cfg*, int32_t*,\n'
                      '                           float*, float*, int32_t*, void*);\n'
                      'step_wav_fn a = conan_step_wav, b = conan_step_wav_async;\n'
                      'int (*c)(conan_streams*, float*, void*) = conan_step_wav_chunk;\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(protos), "-o", str(tmp_path / "protos.o")], check=True)
    for name in ("conan_step_wav", "conan_step_wav_async", "conan_step_wav_chunk"):
        assert name in _lib.declared_symbols() and name in _lib._PROTOS


def test_step_wav_null_handle_is_invalid():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.lib()
    assert lib.conan_abi_version() == 9
    emit = C.c_int32(7)
    mc = _lib.MelCfg(1024, 320, 1024, 80, 16000, 80.0, 7600.0, 1e-6, -6.0, 1.5, 0, 0, 0.0)
    for fn in (lib.conan_step_wav, lib.conan_step_wav_async):
        rc = fn(None, None, 1, 1280, 0, None, C.byref(mc), None, None, None, C.byref(emit), None)
        assert rc == _lib.ERR_INVALID and b"null argument" in lib.conan_last_error()
    assert lib.conan_step_wav_chunk(None, None, None) == _lib.ERR_INVALID


def test_mel_stream_kernel_resources(tmp_path):
    """mel_stream_kernel shares the CUs of the pipelined step's vocoder launches: no scratch, no spills, at most 64 VGPRs (8 waves
    of a 576-thread workgroup per CU fit beside a vocoder block), LDS only dynamic (57 KB at fft_size 1024: 4 frames + twiddles)."""
    from tests.test_kernel_resources import _find, _kernels
    k = _find(_kernels(tmp_path), "mel_stream_kernel")
    assert k["spill"] == 0 and k["scratch"] == 0, k
    assert k["vgpr"] + k["agpr"] <= 64, k
    assert k["lds"] == 0, k
