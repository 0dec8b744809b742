"""CPU checks of the input resampler (conan_resample, conan_streams_set_input_rate, conan_step_wav_ragged_ld, added within ABI 9):
the header compiles as plain C and its struct matches the ctypes binding, the symbols are exported, null handles are
CONAN_ERR_INVALID, conan_resample_length is ceil(new * N / orig) and -1 for refused configurations, the float64 restatement used by
the GPU tests agrees with scipy's upfirdn of the prototype filter, and the two new kernels keep the front-end's resource budget."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conan_amd import _lib
from tests import resample_ref

NAMES = ("conan_resample_length", "conan_resample", "conan_streams_set_input_rate", "conan_step_wav_ragged_ld", "conan_step_wav_ragged_ld_async")
STREAM_RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000)


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    return _lib.lib()


def test_header_struct_and_prototypes(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not present")
    inc = os.path.dirname(_lib.HEADER_PATH)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "conan_hip.h"\n'
                     '#if CONAN_HIP_ABI_VERSION != 9\n#error the resampler is additive: ABI 9 stays\n#endif\n'
                     'typedef int (*ld_fn)(conan_streams*, const int32_t*, int, const int32_t*, const int32_t*, const float*, int64_t,\n'
                     '                     const conan_mel_cfg*, int32_t*, float*, float*, int32_t*, void*);\n'
                     'typedef int (*rs_fn)(conan_ctx*, const conan_resample_cfg*, const float*, int, int64_t, float*, int64_t*, void*);\n'
                     'typedef int (*rate_fn)(conan_streams*, const int32_t*, int, const conan_resample_cfg*);\n'
                     'typedef int64_t (*len_fn)(const conan_resample_cfg*, int64_t);\n'
                     'int main(void) {\n'
                     '  ld_fn a = conan_step_wav_ragged_ld, b = conan_step_wav_ragged_ld_async; rs_fn c = conan_resample;\n'
                     '  rate_fn d = conan_streams_set_input_rate; len_fn e = conan_resample_length;\n'
                     '  (void)a; (void)b; (void)c; (void)d; (void)e;\n'
                     '  printf("%d %d %d %d %d %d %d %d %d %d %d\\n", (int)sizeof(conan_resample_cfg), (int)offsetof(conan_resample_cfg, in_rate),\n'
                     '         (int)offsetof(conan_resample_cfg, out_rate), (int)offsetof(conan_resample_cfg, lowpass_filter_width),\n'
                     '         (int)offsetof(conan_resample_cfg, rolloff), (int)offsetof(conan_resample_cfg, window), (int)offsetof(conan_resample_cfg, beta),\n'
                     '         (int)offsetof(conan_resample_cfg, reserved), CONAN_RESAMPLE_HANN, CONAN_RESAMPLE_KAISER, CONAN_RESAMPLE_MAX_TAPS);\n'
                     '  return 0;\n}\n')
    exe = tmp_path / "probe"
    # -Werror rejects an assignment to a pointer of another function type (compiled only: the symbols are not linked)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(probe), "-o", str(tmp_path / "probe.o")], check=True)
    shim = tmp_path / "shim.c"      # stub definitions, so the probe links and prints the layout
    shim.write_text('#include "conan_hip.h"\n'
                    'int conan_step_wav_ragged_ld(conan_streams* s, const int32_t* a, int n, const int32_t* b, const int32_t* c, const float* d, int64_t e,\n'
                    '  const conan_mel_cfg* f, int32_t* g, float* h, float* i, int32_t* j, void* k) { return 0; }\n'
                    'int conan_step_wav_ragged_ld_async(conan_streams* s, const int32_t* a, int n, const int32_t* b, const int32_t* c, const float* d, int64_t e,\n'
                    '  const conan_mel_cfg* f, int32_t* g, float* h, float* i, int32_t* j, void* k) { return 0; }\n'
                    'int conan_resample(conan_ctx* a, const conan_resample_cfg* b, const float* c, int n, int64_t d, float* e, int64_t* f, void* g) { return 0; }\n'
                    'int conan_streams_set_input_rate(conan_streams* s, const int32_t* a, int n, const conan_resample_cfg* c) { return 0; }\n'
                    'int64_t conan_resample_length(const conan_resample_cfg* c, int64_t n) { return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-I", inc, str(probe), str(shim), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    R = _lib.ResampleCfg
    want = [C.sizeof(R)] + [getattr(R, f).offset for f in ("in_rate", "out_rate", "lowpass_filter_width", "rolloff", "window", "beta", "reserved")]
    assert got[:8] == want
    assert got[8:] == [_lib.RESAMPLE_HANN, _lib.RESAMPLE_KAISER, _lib.RESAMPLE_MAX_TAPS]
    for name in NAMES:
        assert name in _lib.declared_symbols() and name in _lib._PROTOS
    assert len(_lib._PROTOS["conan_step_wav_ragged_ld"][1]) == 13 and _lib._PROTOS["conan_step_wav_ragged_ld"][1][6] is C.c_int64
    assert _lib.ABI_VERSION == 9


def test_symbols_exported_and_null_handles():
    lib = _lib_or_skip()
    assert lib.conan_abi_version() == 9
    for name in NAMES:
        assert getattr(lib, name) is not None
    cfg = _lib.resample_cfg(48000)
    slots = (C.c_int32 * 1)(0)
    assert lib.conan_streams_set_input_rate(None, slots, 1, C.byref(cfg)) == _lib.ERR_INVALID
    assert b"null argument" in lib.conan_last_error()
    assert lib.conan_resample(None, C.byref(cfg), None, 1, 10, None, None, None) == _lib.ERR_INVALID
    emit = (C.c_int32 * 1)(7)
    samples, final = (C.c_int32 * 1)(3840), (C.c_int32 * 1)(0)
    mc = _lib.MelCfg(1024, 320, 1024, 80, 16000, 80.0, 7600.0, 1e-6, -6.0, 1.5, 0, 0, 0.0)
    for name in ("conan_step_wav_ragged_ld", "conan_step_wav_ragged_ld_async"):
        rc = getattr(lib, name)(None, slots, 1, samples, final, None, 3840, C.byref(mc), None, None, None, emit, None)
        assert rc == _lib.ERR_INVALID and b"null argument" in lib.conan_last_error()
        assert emit[0] == 7
    assert lib.conan_resample_length(None, 10) == -1


def test_resample_length():
    lib = _lib_or_skip()
    for r_in, r_out in [(48000, 16000), (44100, 16000), (8000, 16000), (16000, 48000), (16000, 44100), (11025, 16000), (192000, 16000),
                        (22050, 16000), (12345, 16000), (16000, 16000)]:
        g = math.gcd(r_in, r_out)
        orig, new = r_in // g, r_out // g
        for N in (0, 1, orig - 1, orig, orig + 1, 12345, 441000, 10 ** 12):
            for preset in ("hann", "kaiser_best"):
                cfg = _lib.resample_cfg(r_in, r_out, preset=preset)
                assert lib.conan_resample_length(C.byref(cfg), N) == -(-new * N // orig), (r_in, r_out, N)
    ok = _lib.resample_cfg(48000)
    assert lib.conan_resample_length(C.byref(ok), -1) == -1
    bad = [_lib.resample_cfg(7999), _lib.resample_cfg(48000, 192001), _lib.resample_cfg(48000, lowpass_filter_width=0),
           _lib.resample_cfg(48000, lowpass_filter_width=129), _lib.resample_cfg(48000, rolloff=0.0), _lib.resample_cfg(48000, rolloff=1.01),
           _lib.resample_cfg(48000, rolloff=float("nan")), _lib.resample_cfg(48000, rolloff=1e-4)]
    res = _lib.resample_cfg(48000)
    res.reserved[1] = 1
    win = _lib.resample_cfg(48000)
    win.window = 2
    for cfg in bad + [res, win]:
        assert lib.conan_resample_length(C.byref(cfg), 100) == -1


def test_stream_rates_pass_the_80ms_rule():
    """80 ms of input (1280 * in_rate / 16000 samples) is a whole number and a multiple of orig at every documented rate."""
    for r in STREAM_RATES:
        num = 1280 * r
        orig, _ = resample_ref.reduce(r, 16000)
        assert num % 16000 == 0 and (num // 16000) % orig == 0, r
    orig, _ = resample_ref.reduce(44056, 16000)
    assert (1280 * 44056) % 16000 or (1280 * 44056 // 16000) % orig


@pytest.mark.parametrize("r_in,r_out", [(48000, 16000), (44100, 16000), (8000, 16000), (16000, 44100), (22050, 16000)])
@pytest.mark.parametrize("preset", ["hann", "kaiser_best"])
def test_reference_equals_upfirdn(r_in, r_out, preset):
    """The polyphase indexing of the float64 restatement against scipy.signal.upfirdn of the prototype filter h[d + D] =
    H(d) (d = j * orig - i * new), whose output m is output m - D / orig of the resampler."""
    signal = pytest.importorskip("scipy.signal")
    lpw, rolloff, window, beta = resample_ref.PRESETS[preset]
    orig, new = resample_ref.reduce(r_in, r_out)
    base = min(orig, new) * float(np.float32(rolloff))
    Cq = math.ceil(lpw * new / base) + 1
    D = Cq * orig
    d = np.arange(-D, D + 1)
    t = -d * base / (orig * new)
    keep = np.abs(t) < lpw
    x = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(x == 0, 1.0, np.sin(x) / np.where(x == 0, 1.0, x))
    h = np.where(keep, sinc * resample_ref._window(np.clip(t, -lpw, lpw), lpw, window, beta) * (base / orig), 0.0)
    rng = np.random.default_rng(0)
    N = 3 * orig + 17
    sig = rng.standard_normal(N)
    y, _, _ = resample_ref.resample(sig[None], r_in, r_out, lpw, rolloff, window, beta)
    u = signal.upfirdn(h, sig, up=new, down=orig)
    nout = y.shape[1]
    np.testing.assert_allclose(y[0], u[Cq:Cq + nout], rtol=0, atol=1e-12)


def test_resample_kernel_resources(tmp_path):
    """Both resampler kernels run beside the previous chunk's vocoder like mel_stream_ragged_kernel: no scratch, no spills, at most
    64 VGPRs + AGPRs, LDS only dynamic.  Their names hide no existing kernel from a substring lookup."""
    from tests.test_kernel_resources import _find, _kernels
    ks = _kernels(tmp_path)
    for name in ("resample_kernel", "resample_stream_kernel"):
        k = _find(ks, name)
        assert k["spill"] == 0 and k["scratch"] == 0, (name, k)
        assert k["vgpr"] + k["agpr"] <= 64, (name, k)
        assert k["lds"] == 0, (name, k)
    for name in ("mel_stream_kernel", "mel_stream_copy_kernel", "mel_stream_ragged_kernel", "wav_rows_scatter_kernel", "conv_tall_kernel"):
        _find(ks, name)
