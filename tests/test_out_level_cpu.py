"""The output leveller (conan_streams_set_output_level; include/conan_hip.h) without a GPU: the five symbols are exported, declared
and bound; the header compiles as C99; null handles and bad cfgs are refused before any GPU use; and csrc/level_plan.h, the
leveller's host planning, runs in a stand-alone program under AddressSanitizer and UBSan: the end-of-chunk plan the output
leveller's meter follows agrees with the start-of-chunk plan of conan_level and the input leveller."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conan_amd import _lib

SYMBOLS = ("conan_streams_set_output_level", "conan_streams_output_level_cfg", "conan_streams_output_level",
           "conan_streams_output_level_state_bytes", "conan_streams_output_level_state")
CSRC = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")


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


def test_header_compiles_as_c_and_the_cfg_keeps_its_size(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not present")
    inc = os.path.dirname(_lib.HEADER_PATH)
    protos = tmp_path / "protos.c"
    protos.write_text('#include "conan_hip.h"\n'
                      'int (*a)(conan_streams*, const int32_t*, int, const conan_level_cfg*, const void*, int64_t, void*) = conan_streams_set_output_level;\n'
                      'int (*b)(const conan_streams*, int, conan_level_cfg*) = conan_streams_output_level_cfg;\n'
                      'int (*c)(conan_streams*, const int32_t*, int, double*, void*) = conan_streams_output_level;\n'
                      'int64_t (*d)(const conan_streams*) = conan_streams_output_level_state_bytes;\n'
                      'int (*e)(conan_streams*, const int32_t*, int, void*, int64_t, void*) = conan_streams_output_level_state;\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(protos), "-o", str(tmp_path / "protos.o")], check=True)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include "conan_hip.h"\n'
                     'int main(void) { printf("%zu %d", sizeof(conan_level_cfg), CONAN_HIP_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, str(probe), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["48", "9"] and C.sizeof(_lib.LevelCfg) == 48


def test_null_and_invalid_cfgs_are_refused_before_any_gpu_use():
    lib = _lib_or_skip()
    one = (C.c_int32 * 1)(0)
    ok = _lib.level_cfg()
    out = _lib.LevelCfg()
    fake = C.c_void_p(16)      # never dereferenced: the checks below come first
    assert lib.conan_streams_set_output_level(None, one, 1, C.byref(ok), None, 0, None) == _lib.ERR_INVALID
    assert b"null argument" in lib.conan_last_error()
    assert lib.conan_streams_set_output_level(fake, None, 1, C.byref(ok), None, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_output_level(fake, one, 1, None, None, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_output_level_cfg(None, 0, C.byref(out)) == _lib.ERR_INVALID
    assert lib.conan_streams_output_level_cfg(fake, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_output_level(None, one, 1, fake, None) == _lib.ERR_INVALID
    assert lib.conan_streams_output_level(fake, None, 1, fake, None) == _lib.ERR_INVALID
    assert lib.conan_streams_output_level(fake, one, 1, None, None) == _lib.ERR_INVALID
    assert lib.conan_streams_output_level_state_bytes(None) == _lib.ERR_INVALID
    assert lib.conan_streams_output_level_state(None, one, 1, fake, 1 << 20, None) == _lib.ERR_INVALID
    assert lib.conan_streams_output_level_state(fake, None, 1, fake, 1 << 20, None) == _lib.ERR_INVALID
    assert lib.conan_streams_output_level_state(fake, one, 1, None, 1 << 20, None) == _lib.ERR_INVALID
    # every bad cfg of tests/test_level_cpu.py's list (the handle is never touched: the cfg is checked first)
    bad = [dict(window_blocks=0), dict(window_blocks=_lib.LEVEL_MAX_BLOCKS + 1), dict(max_boost_db=-0.5), dict(max_cut_db=-1.0),
           dict(max_boost_db=float("inf")), dict(max_cut_db=float("nan")), dict(target=float("nan")), dict(initial_gain_db=float("-inf"))]
    cfgs = [_lib.level_cfg(**kw) for kw in bad]
    for field, value in (("enabled", 2), ("peak_limit", 2), ("clip", -1)):
        c = _lib.level_cfg()
        setattr(c, field, value)
        cfgs.append(c)
    c = _lib.level_cfg()
    c.reserved[3] = 5
    cfgs.append(c)
    for c in cfgs:
        assert lib.conan_streams_set_output_level(fake, one, 1, C.byref(c), None, 0, None) == _lib.ERR_INVALID, lib.conan_last_error()


PLAN_PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "level_plan.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static bool same_blocks(const cnk::LvCall& a, const cnk::LvCall& b) {
  if (a.j0 != b.j0 || a.nblk != b.nblk) return false;
  for (int i = 0; i < a.nblk; ++i) if (a.lo[i] != b.lo[i] || a.hi[i] != b.hi[i]) return false;
  return true;
}

int main() {
  const double fs = 16000.0;
  const int U = 1280;
  long long closed = 0;      // blocks closed so far, by the end-of-chunk plans alone
  for (int k = 0; k < 40; ++k) {
    cnk::LvCall e, same, next;
    CHECK(level::plan_end((long long)k * U, U, U, fs, e) == nullptr);
    CHECK(level::plan_call((long long)k * U, U, U, fs, same) == nullptr);          // chunk k by the start-of-chunk plan
    CHECK(level::plan_call((long long)(k + 1) * U, U, U, fs, next) == nullptr);    // chunk k + 1 by the start-of-chunk plan
    CHECK(e.pos0 == (long long)k * U && e.m == U);
    // the instant: at the chunk's end, with the J the next chunk's plan has at its start
    CHECK(e.inst == 1 && e.u == U && next.inst == 1 && next.u == 0 && e.J == next.J);
    CHECK(e.J == (int)level::blocks_ended((long long)(k + 1) * U, fs));
    // the block list over the chunk's segments
    CHECK(same_blocks(e, same));
    CHECK(e.nblk <= cnk::kLvBlocks);
    // the blocks that close: those of the list that end inside the chunk (U is a multiple of 128: all its segments are complete),
    // in index order from the first open one, and after them exactly the blocks the instant counts are closed
    CHECK(e.nblk == 0 || e.j0 == closed);
    for (int i = 0; i < e.nblk; ++i) {
      CHECK(e.lo[i] < U && e.hi[i] > 0);
      CHECK(e.lo[i] == (int)(level::block_lo(e.j0 + i, fs) - (long long)k * U));
      if (e.hi[i] <= U) { CHECK(e.j0 + i == closed); ++closed; }
    }
    CHECK(closed == e.J);
    // ... which is where the next chunk's list of open blocks begins
    CHECK(next.nblk == 0 || next.j0 == closed);
  }
  CHECK(closed > 20);
  {  // a short last chunk: the meter takes its whole segments and reaches no instant
    cnk::LvCall e, same;
    CHECK(level::plan_end(40ll * U, 700, U, fs, e) == nullptr);
    CHECK(level::plan_call(40ll * U, 700, U, fs, same) == nullptr);
    CHECK(e.inst == 0 && e.m == 700 && same_blocks(e, same));
    CHECK(same.inst == 1 && same.u == 0);      // (the start-of-chunk plan has its instant at the chunk's start; the end plan had it in chunk 39)
    for (int i = 0; i < e.nblk; ++i) CHECK(e.lo[i] < 700 / 128 * 128);
    CHECK(level::plan_end(40ll * U, 100, U, fs, e) == nullptr && e.nblk == 0 && e.inst == 0);      // less than a segment
  }
  {  // rows the split form refuses
    cnk::LvCall e;
    CHECK(level::plan_end(5, U, U, fs, e) != nullptr);
    CHECK(level::plan_end(3ll * U + 320, 960, U, fs, e) != nullptr);
    CHECK(level::plan_end(-(long long)U, U, U, fs, e) != nullptr);
    CHECK(level::plan_end(0, U + 1, U, fs, e) != nullptr);
    CHECK(level::plan_end(2ll * U, 2 * U, U, fs, e) != nullptr);
    CHECK(level::plan_end(0, 0, U, fs, e) != nullptr);
    CHECK(level::plan_end(0, 100, 1000, fs, e) != nullptr);      // an interval that is no multiple of 128
    CHECK(level::plan_end(0, U, U, fs, e) == nullptr);
  }
  std::printf("OK\n");
  return 0;
}
"""


def test_end_of_chunk_plan_under_sanitizers(tmp_path):
    """csrc/level_plan.h in a stand-alone program with AddressSanitizer and UBSan.  At fs = 16000, U = 1280, for every chunk k of a
    40-chunk stream and for a short last chunk of 700 samples the end-of-chunk plan agrees with plan_call's: the blocks that close,
    J_{k+1} and the block list over the chunk's segments; unaligned and over-long rows are refused."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not present")
    src = tmp_path / "level_plan.cpp"
    src.write_text(PLAN_PROGRAM)
    exe = tmp_path / "level_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
