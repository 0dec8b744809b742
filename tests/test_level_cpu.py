"""CPU checks of the streaming input leveller (conan_level, conan_streams_set_input_level; include/conan_hip.h, conan_level_cfg):
tests/level_ref.py - the numpy restatement of the law - held to tests/loudness_ref.py on every prefix that ends at a gating block,
the gate margin every tolerance test of tests/test_gpu_level.py rests on, and the ABI surface (symbols, the header as plain C, the
ctypes mirror, configurations refused before any GPU use)."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conan_amd import _lib
from tests import level_ref as V
from tests import loudness_ref as LR

SYMBOLS = ("conan_level", "conan_streams_set_input_level", "conan_streams_input_level", "conan_slot_meta_level")
CSRC = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")


@functools.lru_cache(maxsize=None)
def _runs():
    out = []
    for n, seed in V.CASES:
        x = V.sig(n, seed)
        out.append((x, V.level(x, window_blocks=4096)))
    return out


def test_reading_equals_the_whole_signal_meter_on_every_prefix():
    """With the window at least the block count, L_k is loudness_ref.loudness of the prefix that ends at the last complete block."""
    readings = 0
    for x, r in _runs():
        cache = {}
        for k in range(len(r["trace"])):
            J, hi, L = int(r["counts"][k]), int(r["hi"][k]), r["trace"][k, 0]
            assert J == sum(1 for _, h in V.blocks(len(x)) if h <= k * V.U) and hi <= k * V.U
            if J == 0:
                assert L == -np.inf
                continue
            if hi not in cache:
                cache[hi] = LR.loudness(x[:hi], V.FS)
            want = cache[hi]
            assert (L == want) if want == -np.inf else abs(L - want) <= 1e-9, (k, L, want)
            readings += np.isfinite(want)
    assert readings > 50


def test_gate_margin_of_the_six_cases():
    for (n, seed), (_, r) in zip(V.CASES, _runs()):
        print(n, seed, "gate margin", r["margin"])
        assert r["margin"] >= 1e-4, (n, seed, r["margin"])


def test_the_signal_takes_every_branch_of_the_law():
    x, r = _runs()[1]
    tr = r["trace"]
    assert (tr[:4, 0] == -np.inf).all() and (tr[:4, 1] == 1.0).all()      # nothing above the absolute gate yet: the initial gain stays
    assert tr[5, 0] < -50 and tr[5, 1] == 10.0                            # the first reading asks for more than the +20 dB cap
    assert abs(tr[12, 1] - 1 / 0.9) < 1e-7 and r["peaks"][12] == np.float32(0.9)      # the spike: the peak limit pulls the gain to 1.11
    assert np.abs(r["y"]).max() > 8.0                                     # ... after it passed at the old gain
    wide = V.level(x, window_blocks=4096)["trace"][-1, 0]
    short = V.level(x, window_blocks=5)["trace"][-1, 0]
    assert abs(wide - short) > 0.01                                       # the window matters
    assert tr[-1, 1] < 1.0                                                # the loud part is cut
    # the ramp is continuous: no step larger than the per-sample slope allows
    g = r["y"][20000:21000].astype(np.float64) / x[20000:21000].astype(np.float64)
    assert np.abs(np.diff(g)).max() < 10.0 / V.U


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
    fields = [f[0] for f in _lib.LevelCfg._fields_]
    probe = tmp_path / "probe.c"
    protos = tmp_path / "protos.c"
    protos.write_text('#include "conan_hip.h"\n'
                     'int (*a)(conan_ctx*, const conan_level_cfg*, const float*, int64_t, int, const int64_t*, float*, int64_t, double*, int64_t, void*) = conan_level;\n'
                     'int (*b)(conan_streams*, const int32_t*, int, const conan_level_cfg*) = conan_streams_set_input_level;\n'
                     'int (*c)(conan_streams*, const int32_t*, int, double*, void*) = conan_streams_input_level;\n'
                     'int (*d)(const conan_slot_meta*, conan_level_cfg*) = conan_slot_meta_level;\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(protos), "-o", str(tmp_path / "protos.o")], check=True)
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "conan_hip.h"\n'
                     'int main(void) {\n'
                     '  printf("%d %zu", CONAN_LEVEL_MAX_BLOCKS, sizeof(conan_level_cfg));\n' +
                     "".join('  printf(" %%zu", offsetof(conan_level_cfg, %s));\n' % f for f in fields) +
                     '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, str(probe), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [_lib.LEVEL_MAX_BLOCKS, C.sizeof(_lib.LevelCfg)] + [getattr(_lib.LevelCfg, f).offset for f in fields]
    assert out[:2] == [4096, 48]


def test_null_and_invalid_cfgs_are_refused_before_any_gpu_use():
    lib = _lib_or_skip()
    one = (C.c_int32 * 1)(0)
    n = (C.c_int64 * 1)(1000)
    ok = _lib.level_cfg()
    fake = C.c_void_p(16)      # never dereferenced: the checks below come first
    assert lib.conan_level(None, C.byref(ok), fake, 1000, 1, n, fake, 1000, None, 0, None) == _lib.ERR_INVALID
    assert b"null argument" in lib.conan_last_error()
    assert lib.conan_level(fake, None, fake, 1000, 1, n, fake, 1000, None, 0, None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_input_level(None, one, 1, C.byref(ok)) == _lib.ERR_INVALID
    assert lib.conan_streams_set_input_level(fake, one, 1, None) == _lib.ERR_INVALID
    assert lib.conan_streams_input_level(None, one, 1, fake, None) == _lib.ERR_INVALID
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
    for c in cfgs:      # (the handles are never touched: the cfg is checked first)
        assert lib.conan_level(fake, C.byref(c), fake, 1000, 1, n, fake, 1000, None, 0, None) == _lib.ERR_INVALID
        assert lib.conan_streams_set_input_level(fake, one, 1, C.byref(c)) == _lib.ERR_INVALID
    off = _lib.LevelCfg()
    assert lib.conan_level(fake, C.byref(off), fake, 1000, 1, n, fake, 1000, None, 0, None) == _lib.ERR_INVALID


def test_meta_level_refuses_what_is_not_a_record():
    lib = _lib_or_skip()
    out = _lib.LevelCfg()
    zero = _lib.SlotMeta()
    assert lib.conan_slot_meta_level(None, C.byref(out)) == _lib.ERR_INVALID
    assert lib.conan_slot_meta_level(C.byref(zero), None) == _lib.ERR_INVALID
    assert lib.conan_slot_meta_level(C.byref(zero), C.byref(out)) == _lib.ERR_INVALID
    assert b"not a slot snapshot record" in lib.conan_last_error()
    rec = bytearray(_lib.SLOT_META_BYTES)      # magic "CNSN", version 1, size 256, a wrong checksum
    rec[0:4] = (0x4e534e43).to_bytes(4, "little")
    rec[4:8] = (1).to_bytes(4, "little")
    rec[8:12] = (256).to_bytes(4, "little")
    bad = _lib.SlotMeta.from_buffer_copy(bytes(rec))
    assert lib.conan_slot_meta_level(C.byref(bad), C.byref(out)) == _lib.ERR_INVALID
    assert b"corrupted" in lib.conan_last_error()


LAYOUT_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "snapshot_layout.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

constexpr int kSlots = 3, kCore = 40, kFe = 64, kLevel = 672 + 16 * 24;      // bytes per slot; the level block: a state and two short rings

struct State {
  std::vector<unsigned char> core, fe, level;
  snap::Layout lay;
};

static void build(State& s, bool with_level) {
  s.core.assign(kSlots * kCore, 0); s.fe.assign(kSlots * kFe, 0); s.level.assign(kSlots * kLevel, 0);
  snap::Layout l;
  snap::add_whole(l, s.core.data(), kCore, kCore, snap::SEC_CORE);
  snap::add_whole(l, s.fe.data(), kFe, kFe, snap::SEC_FE, true);
  if (with_level) snap::add_whole(l, s.level.data(), kLevel, kLevel, snap::SEC_LEVEL);
  for (int sec = 1; sec < snap::SEC_COUNT; ++sec) if (l.sec_end[sec] == 0) l.sec_end[sec] = l.sec_end[sec - 1];
  const int32_t cfg[2] = {7, 1};
  snap::finish(l, cfg, 2);
  s.lay = l;
}

template <bool PACK>
static void run(State& s, const snap::CallRow& row, char* blob_row) {
  const int items = s.lay.items(row.used_bytes);
  for (int it = 0; it < items; ++it)
    for (long long off = (long long)it * snap::kItemBytes; off < (long long)(it + 1) * snap::kItemBytes && off < row.used_bytes; off += snap::kCell)
      snap::move_cell<PACK>(s.lay.regions.data(), s.lay.item_first[it], row, blob_row, off);
}

int main() {
  State with, without;
  build(with, true); build(without, false);
  // the section is not part of the id; it is the row's last section and only lengthens rows that carry it
  CHECK(with.lay.id == without.lay.id);
  CHECK(snap::SEC_LEVEL == snap::SEC_COUNT - 1);
  const int fe = (1 << snap::SEC_CORE) | (1 << snap::SEC_FE), lv = fe | (1 << snap::SEC_LEVEL);
  CHECK(with.lay.sec_end[snap::SEC_FE] == without.lay.sec_end[snap::SEC_FE] && with.lay.sec_end[snap::SEC_RS_OUT] == without.lay.sec_end[snap::SEC_RS_OUT]);
  CHECK(with.lay.sec_end[snap::SEC_LEVEL] == with.lay.sec_end[snap::SEC_RS_OUT] + snap::pad_cell(kLevel));
  CHECK(without.lay.sec_end[snap::SEC_LEVEL] == without.lay.sec_end[snap::SEC_RS_OUT]);
  CHECK(snap::used_bytes(with.lay, fe) == snap::used_bytes(without.lay, fe) && snap::used_bytes(with.lay, 1) == without.lay.sec_end[snap::SEC_CORE]);
  CHECK(snap::used_bytes(with.lay, lv) == with.lay.sec_end[snap::SEC_LEVEL] && snap::used_bytes(with.lay, lv) == snap::used_bytes(with.lay, fe) + snap::pad_cell(kLevel));
  CHECK(snap::used_bytes(without.lay, lv) == snap::used_bytes(without.lay, fe));
  CHECK(with.lay.bytes % 256 == 0 && with.lay.bytes >= with.lay.sec_end[snap::SEC_LEVEL]);
  // pack slot 0, unpack into slot 2 of junk-filled state
  for (int i = 0; i < kSlots * kLevel; ++i) with.level[i] = (unsigned char)(1 + i * 7);
  for (int i = 0; i < kSlots * kFe; ++i) with.fe[i] = (unsigned char)(3 + i);
  for (int i = 0; i < kSlots * kCore; ++i) with.core[i] = (unsigned char)(5 + i * 3);
  const long long used = snap::used_bytes(with.lay, lv);
  std::vector<char> blob((size_t)with.lay.bytes + 64, (char)0x5a);
  const snap::CallRow prow = {0, lv, (int)used, 0};
  run<true>(with, prow, blob.data());
  for (size_t i = (size_t)used; i < blob.size(); ++i) CHECK(blob[i] == (char)0x5a);
  State dst; build(dst, true);
  for (auto& v : dst.level) v = 0xee;
  for (auto& v : dst.fe) v = 0xee;
  for (auto& v : dst.core) v = 0xee;
  const snap::CallRow urow = {2, lv, (int)used, 0};
  run<false>(dst, urow, blob.data());
  CHECK(memcmp(dst.level.data() + 2 * kLevel, with.level.data(), kLevel) == 0);
  CHECK(memcmp(dst.fe.data() + 2 * kFe, with.fe.data(), kFe) == 0 && memcmp(dst.core.data() + 2 * kCore, with.core.data(), kCore) == 0);
  for (int i = 0; i < 2 * kLevel; ++i) CHECK(dst.level[i] == 0xee);      // the other slots are untouched
  // a slot without the section: a walk that covers it packs zeros, and an import leaves the destination's block alone
  std::vector<char> absent((size_t)with.lay.bytes, (char)0x5a);
  const snap::CallRow arow = {1, fe, (int)used, 0};
  run<true>(with, arow, absent.data());
  for (long long i = with.lay.sec_end[snap::SEC_RS_OUT]; i < used; ++i) CHECK(absent[(size_t)i] == 0);
  CHECK(memcmp(absent.data(), blob.data(), 16) != 0);      // (slot 1's core, not slot 0's)
  const snap::CallRow brow = {0, fe, (int)used, 0};
  run<false>(dst, brow, absent.data());
  for (int i = 0; i < kLevel; ++i) CHECK(dst.level[i] == 0xee);
  printf("OK\n");
  return 0;
}
"""


def test_level_section_of_the_snapshot_layout_under_sanitizers(tmp_path):
    """csrc/snapshot_layout.h in a stand-alone program with AddressSanitizer and UBSan: a layout with the leveller's whole region and
    one without have the same id; used_bytes and sec_end include the section only when present; the section round-trips through
    pack and unpack; an absent section packs as zeros."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not present")
    src = tmp_path / "level_layout.cpp"
    src.write_text(LAYOUT_PROGRAM)
    exe = tmp_path / "level_layout"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
