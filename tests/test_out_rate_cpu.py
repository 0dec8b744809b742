"""CPU checks of the output resampler (conan_streams_set_output_rate / _set_output_ld / _output_samples / _output_pending /
_flush_output, added within ABI 9): the symbols are exported and null handles are CONAN_ERR_INVALID, the header compiles as plain C
with the prototypes the ctypes binding mirrors, resample_out_kernel keeps the resampler kernels' resource budget, and the delivery
schedule restated from tests/resample_ref.py (what the GPU tests hold conan_streams_output_samples against) agrees with brute force."""
import ctypes as C
import os
import subprocess

import pytest

from conan_amd import _lib
from tests import resample_ref

NAMES = ("conan_streams_set_output_rate", "conan_streams_set_output_ld", "conan_streams_output_samples", "conan_streams_output_pending",
         "conan_streams_flush_output")
MODEL_RATE = 16000
OUT_RATES = (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 96000)
# first step and flush at 4 frames per step, in output samples (the header's latency figures)
LOOKAHEAD = {"hann": {8000: 6, 22050: 8, 44100: 16, 48000: 18, 96000: 36},
             "kaiser_best": {8000: 67, 22050: 93, 44100: 186, 48000: 202, 96000: 405}}


def out_filter(rate, preset):
    return resample_ref.filt(MODEL_RATE, rate, *resample_ref.PRESETS[preset])


def ready(f, total):
    """ch::RsTable::ready restated: the longest prefix of outputs whose last tap is below `total` model-rate samples (and, like the
    whole signal, below its length).  f = resample_ref.filt(...)."""
    orig, new, w, phases = f
    best = -(-new * total // orig)
    for p, (klo, h) in enumerate(phases):
        c = klo + len(h) - 1 - w                     # last tap of output p + new * q = q * orig + c
        q = 0 if total - c <= 0 else -(-(total - c) // orig)
        best = min(best, p + new * q)
    return best


def schedule(f, steps):
    """Samples each step delivers (steps = model-rate samples per step) and what the flush delivers."""
    orig, new, _, _ = f
    total, done, out = 0, 0, []
    for m in steps:
        total += m
        r = max(ready(f, total), done)
        out.append(r - done)
        done = r
    return out, -(-new * total // orig) - done


def test_symbols_exported_and_null_handles():
    lib = _lib.lib()
    assert lib.conan_abi_version() == 9
    for name in NAMES:
        assert getattr(lib, name) is not None and name in _lib.declared_symbols() and name in _lib._PROTOS
    cfg = _lib.resample_cfg(16000, 48000)
    slots, counts = (C.c_int32 * 1)(0), (C.c_int32 * 1)(7)
    assert lib.conan_streams_set_output_rate(None, slots, 1, C.byref(cfg)) == _lib.ERR_INVALID
    assert b"null" in lib.conan_last_error()
    assert lib.conan_streams_set_output_ld(None, 3840) == _lib.ERR_INVALID
    assert lib.conan_streams_output_samples(None, counts, 1) == _lib.ERR_INVALID
    assert lib.conan_streams_output_pending(None, slots, 1, counts) == _lib.ERR_INVALID
    assert lib.conan_streams_flush_output(None, slots, 1, None, 3840, None) == _lib.ERR_INVALID
    assert counts[0] == 7


def test_header_prototypes(tmp_path):
    inc = os.path.dirname(_lib.HEADER_PATH)
    probe = tmp_path / "probe.c"
    probe.write_text('#include "conan_hip.h"\n'
                     '#if CONAN_HIP_ABI_VERSION != 9\n#error the output resampler is additive: ABI 9 stays\n#endif\n'
                     'typedef int (*rate_fn)(conan_streams*, const int32_t*, int, const conan_resample_cfg*);\n'
                     'typedef int (*ld_fn)(conan_streams*, int64_t);\n'
                     'typedef int (*samples_fn)(conan_streams*, int32_t*, int);\n'
                     'typedef int (*pending_fn)(conan_streams*, const int32_t*, int, int32_t*);\n'
                     'typedef int (*flush_fn)(conan_streams*, const int32_t*, int, float*, int64_t, void*);\n'
                     'int main(void) {\n'
                     '  rate_fn a = conan_streams_set_output_rate; ld_fn b = conan_streams_set_output_ld; samples_fn c = conan_streams_output_samples;\n'
                     '  pending_fn d = conan_streams_output_pending; flush_fn e = conan_streams_flush_output;\n'
                     '  (void)a; (void)b; (void)c; (void)d; (void)e;\n'
                     '  return 0;\n}\n')
    # -Werror rejects an assignment to a pointer of another function type (compiled only: the symbols are not linked)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(probe), "-o", str(tmp_path / "probe.o")], check=True)
    P = _lib._PROTOS
    assert P["conan_streams_set_output_rate"] == P["conan_streams_set_input_rate"]
    assert P["conan_streams_set_output_ld"] == (C.c_int, [C.c_void_p, C.c_int64])
    assert P["conan_streams_output_samples"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int])
    assert P["conan_streams_output_pending"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p])
    assert P["conan_streams_flush_output"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p])
    assert _lib.ABI_VERSION == 9


def test_resample_out_kernel_resources(tmp_path):
    """resample_out_kernel sits on the vocoder stream beside resident decoder workgroups: no scratch, no spills, at most 64 VGPRs +
    AGPRs, LDS only dynamic (the tile window).  Its name hides no resampler kernel from a substring lookup."""
    from tests.test_kernel_resources import _find, _kernels
    ks = _kernels(tmp_path)
    k = _find(ks, "resample_out_kernel")
    assert k["spill"] == 0 and k["scratch"] == 0, k
    assert k["vgpr"] + k["agpr"] <= 64, k
    assert k["lds"] == 0, k
    for name in ("resample_kernel", "resample_stream_kernel", "wav_rows_scatter_kernel", "conv_post_kernel"):
        _find(ks, name)


@pytest.mark.parametrize("preset", ["hann", "kaiser_best"])
@pytest.mark.parametrize("rate", OUT_RATES)
def test_schedule_against_brute_force(rate, preset):
    """ready(I) = the number of leading outputs j < length(I) whose last tap q * orig - w + klo + cnt - 1 is below I, counted one by
    one; steps of 320 and 1280 samples; steady steps deliver m * new / orig samples (floor or ceiling when that is no whole number)."""
    f = out_filter(rate, preset)
    orig, new, w, phases = f
    for m in (320, 1280):
        total, done = 0, 0
        for step in range(24):
            total += m
            n_len = -(-new * total // orig)
            j = 0
            while j < n_len:
                q, p = divmod(j, new)
                if q * orig - w + phases[p][0] + len(phases[p][1]) - 1 >= total:
                    break
                j += 1
            assert ready(f, total) == j, (rate, preset, m, step)
            if step >= 1:
                lo = m * new // orig
                assert j - done in (lo, -(-m * new // orig)), (rate, preset, m, step, j - done)
            done = j
        counts, tail = schedule(f, [m] * 24)
        assert sum(counts) + tail == resample_ref.length(MODEL_RATE, rate, 24 * m)
        assert counts[0] + tail == counts[1] or (m * new) % orig       # the first step is short by what the flush delivers
    if rate in LOOKAHEAD[preset]:
        counts, tail = schedule(f, [1280] * 3)
        assert 1280 * new // orig - counts[0] == LOOKAHEAD[preset][rate] == tail, (rate, preset, counts, tail)
    if rate == 11025:
        counts, _ = schedule(f, [320] * 40)
        assert set(counts[1:]) == {220, 221}
