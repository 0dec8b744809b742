"""CPU checks of slot snapshots (conan_streams_export_slots / _import_slots, ABI 9): the exported symbols, the header compiled as plain
C against the ctypes mirrors, null handles, the meta record's checks, and csrc/snapshot_layout.h - the blob layout, the layout id and
the cell mover the GPU kernels run - compiled into a stand-alone program with AddressSanitizer and UBSan."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conan_amd import _lib

SYMBOLS = ("conan_streams_layout_id", "conan_streams_snapshot_bytes", "conan_streams_export_slots", "conan_streams_import_slots",
           "conan_slot_meta_info")
CSRC = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    return _lib.lib()


def test_library_exports_snapshot_symbols():
    _lib_or_skip()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.declared_symbols() and name in _lib._PROTOS
    assert raw.conan_abi_version() == 9


def test_header_structs_match_binding(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not present")
    inc = os.path.dirname(_lib.HEADER_PATH)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "conan_hip.h"\n'
                     'int main(void) {\n'
                     '  printf("%d %zu %zu %zu %zu %zu\\n", CONAN_SLOT_META_BYTES, sizeof(conan_slot_meta), sizeof(conan_slot_info),\n'
                     '         offsetof(conan_slot_info, bytes), offsetof(conan_slot_info, in_rate), offsetof(conan_slot_info, out_rate));\n'
                     '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, str(probe), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [_lib.SLOT_META_BYTES, C.sizeof(_lib.SlotMeta), C.sizeof(_lib.SlotInfo), _lib.SlotInfo.bytes.offset,
                   _lib.SlotInfo.in_rate.offset, _lib.SlotInfo.out_rate.offset]
    assert out[:2] == [256, 256]
    protos = tmp_path / "protos.c"
    protos.write_text('#include "conan_hip.h"\n'
                      'uint64_t (*a)(const conan_streams*) = conan_streams_layout_id;\n'
                      'int64_t (*b)(const conan_streams*) = conan_streams_snapshot_bytes;\n'
                      'int (*c)(conan_streams*, const int32_t*, int, void*, int64_t, conan_slot_meta*, void*) = conan_streams_export_slots;\n'
                      'int (*d)(conan_streams*, const int32_t*, int, const void*, int64_t, const conan_slot_meta*, void*) = conan_streams_import_slots;\n'
                      'int (*e)(const conan_slot_meta*, conan_slot_info*) = conan_slot_meta_info;\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(protos), "-o", str(tmp_path / "protos.o")], check=True)


def test_null_handles_are_invalid():
    lib = _lib_or_skip()
    meta = (_lib.SlotMeta * 1)()
    slots = (C.c_int32 * 1)(0)
    assert lib.conan_streams_export_slots(None, slots, 1, None, 0, meta, None) == _lib.ERR_INVALID
    assert b"null argument" in lib.conan_last_error()
    assert lib.conan_streams_import_slots(None, slots, 1, None, 0, meta, None) == _lib.ERR_INVALID
    assert b"null argument" in lib.conan_last_error()
    assert lib.conan_streams_snapshot_bytes(None) == _lib.ERR_INVALID
    assert lib.conan_streams_layout_id(None) == 0
    assert lib.conan_slot_meta_info(None, None) == _lib.ERR_INVALID


def test_meta_info_rejects_what_is_not_a_record():
    lib = _lib_or_skip()
    info = _lib.SlotInfo()
    zero = _lib.SlotMeta()
    assert lib.conan_slot_meta_info(C.byref(zero), C.byref(info)) == _lib.ERR_INVALID
    assert b"not a slot snapshot record" in lib.conan_last_error()
    # the record's first words: magic "CNSN", version, size - a version this library does not read
    rec = bytearray(_lib.SLOT_META_BYTES)
    rec[0:4] = (0x4e534e43).to_bytes(4, "little")
    rec[4:8] = (99).to_bytes(4, "little")
    rec[8:12] = (256).to_bytes(4, "little")
    bad = _lib.SlotMeta.from_buffer_copy(bytes(rec))
    assert lib.conan_slot_meta_info(C.byref(bad), C.byref(info)) == _lib.ERR_INVALID
    assert b"version 99" in lib.conan_last_error()
    # the right version with a wrong checksum
    rec[4:8] = (1).to_bytes(4, "little")
    bad = _lib.SlotMeta.from_buffer_copy(bytes(rec))
    assert lib.conan_slot_meta_info(C.byref(bad), C.byref(info)) == _lib.ERR_INVALID
    assert b"corrupted" in lib.conan_last_error()


LAYOUT_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "snapshot_layout.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

struct RingSpec { int C, rate, hist; };
// widths that are multiples of 4 floats (the vector path), one that is not (the dword path), a ring without history
static const RingSpec kRings[] = {{80, 1, 6}, {256, 8, 15}, {32, 64, 66}, {3, 2, 5}, {16, 1, 0}, {128, 4, 12}};
constexpr int kNR = sizeof(kRings) / sizeof(kRings[0]);
constexpr int kSlots = 3, kOddWords = 9;      // a whole region of 36 bytes: its last cell is padded

struct State {
  std::vector<int> pos;                       // [slots]
  std::vector<std::vector<float>> ring;       // per ring [slots][L][C]
  std::vector<int> L;
  std::vector<uint32_t> odd;                  // [slots][kOddWords]
  std::vector<float> fe;                      // [slots][64]: a section the slots do not use
  snap::Layout lay;
};

static int next_pow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }

static void build(State& s, int frames, const RingSpec* rings = kRings, int cfg0 = 7) {
  s.pos.assign(kSlots, 0); s.ring.clear(); s.L.clear();
  s.odd.assign(kSlots * kOddWords, 0); s.fe.assign(kSlots * 64, 0.f);
  snap::Layout l;
  const int pc = (int)l.regions[snap::add_whole(l, s.pos.data(), 4, 4, snap::SEC_CORE)].blob_off;
  for (int r = 0; r < kNR; ++r) {
    const int L = next_pow2(rings[r].hist + frames * rings[r].rate);
    s.L.push_back(L);
    s.ring.emplace_back((size_t)kSlots * L * rings[r].C, 0.f);
  }
  for (int r = 0; r < kNR; ++r)
    snap::add_ring(l, s.ring[r].data(), (long long)s.L[r] * rings[r].C * 4, rings[r].C, s.L[r], rings[r].rate, rings[r].hist, s.pos.data(), pc, snap::SEC_CORE);
  snap::add_whole(l, s.odd.data(), kOddWords * 4, kOddWords * 4, snap::SEC_CORE);
  snap::add_whole(l, s.fe.data(), 64 * 4, 64 * 4, snap::SEC_FE, true);
  const int32_t cfg[2] = {cfg0, 1};
  snap::finish(l, cfg, 2);
  s.lay = l;
}

static float val(int r, int slot, long long t, int col) { return t < 0 ? 0.f : (float)(1 + r * 1000003 + slot * 7919 + t * 131 + col); }

// what `pos` steps of a stream leave in the rings: logical row t at t & lmask, zeros before the start of the utterance
static void play(State& s, int slot, int pos) {
  s.pos[slot] = pos;
  for (int r = 0; r < kNR; ++r) {
    const int C = kRings[r].C, L = s.L[r];
    const long long end = (long long)pos * kRings[r].rate;
    for (long long t = end - L; t < end; ++t)
      for (int c = 0; c < C; ++c) s.ring[r][((size_t)slot * L + (size_t)(t & (L - 1))) * C + c] = val(r, slot, t, c);
  }
  for (int w = 0; w < kOddWords; ++w) s.odd[slot * kOddWords + w] = 0xabc00000u + slot * 64 + w;
}

template <bool PACK>
static void run(State& s, const snap::CallRow& row, char* blob_row) {      // the kernel's walk over one row
  const int items = s.lay.items(row.used_bytes);
  for (int it = 0; it < items; ++it)
    for (long long off = (long long)it * snap::kItemBytes; off < (long long)(it + 1) * snap::kItemBytes && off < row.used_bytes; off += snap::kCell)
      snap::move_cell<PACK>(s.lay.regions.data(), s.lay.item_first[it], row, blob_row, off);
}

int main() {
  State a, b;
  build(a, 4); build(b, 16);
  // ---- the table: aligned, disjoint, contiguous, summing to the reported size
  long long end = 0;
  for (const snap::Region& r : a.lay.regions) {
    CHECK(r.blob_off % 16 == 0);
    CHECK(r.blob_off == end);                 // disjoint and without holes: every cell belongs to one region
    end = r.blob_off + snap::pad_cell(r.bytes);
  }
  CHECK(a.lay.bytes % 256 == 0 && a.lay.bytes >= end && a.lay.bytes - end < 256);
  CHECK(a.lay.sec_end[snap::SEC_FE] == end && a.lay.sec_end[snap::SEC_CORE] == end - 256);
  CHECK((int)a.lay.item_first.size() == a.lay.items(a.lay.bytes));
  CHECK(a.lay.regions[4].aligned == 0 && a.lay.regions[1].aligned == 1);      // the 3-float ring takes the dword path
  // ---- the id: not the ring length, but every one of C, rate and saved rows, and the caller's words
  CHECK(a.lay.id == b.lay.id && a.lay.bytes == b.lay.bytes);
  CHECK(a.L[1] != b.L[1] && a.L[2] != b.L[2]);
  for (int f = 0; f < 3; ++f) {
    RingSpec alt[kNR];
    for (int r = 0; r < kNR; ++r) alt[r] = kRings[r];
    if (f == 0) alt[2].C += 4; else if (f == 1) alt[2].rate += 1; else alt[2].hist += 1;
    State c; build(c, 4, alt);
    CHECK(c.lay.id != a.lay.id);
  }
  { State c; build(c, 4, kRings, 8); CHECK(c.lay.id != a.lay.id); }
  // ---- ring_row
  CHECK(snap::ring_row(0, 8, 15, 0, 63) == ((-15) & 63) && snap::ring_row(0, 8, 15, 14, 63) == 63 && snap::ring_row(8, 8, 15, 15, 63) == 0);
  // ---- pack from rings of one length, unpack into junk-filled rings of another
  const int positions[] = {0, 1, 2, 16, 64, 1000003};      // no rows yet; below the histories (negative logical rows); exactly at a wrap of the rings; far past many wraps
  for (int dir = 0; dir < 2; ++dir)
    for (int pos : positions) {
      State& src = dir ? b : a; State& dst = dir ? a : b;
      build(src, dir ? 16 : 4); build(dst, dir ? 4 : 16);
      for (int s = 0; s < kSlots; ++s) play(src, s, pos + s);
      const int from = 0, to = 2;
      const long long used = src.lay.sec_end[snap::SEC_CORE];
      std::vector<char> blob((size_t)src.lay.bytes + 64, (char)0x5a);
      const snap::CallRow prow = {from, 1, (int)used, 0};
      run<true>(src, prow, blob.data());
      for (size_t i = (size_t)used; i < blob.size(); ++i) CHECK(blob[i] == (char)0x5a);      // nothing past the used bytes
      std::vector<char> again((size_t)src.lay.bytes + 64, (char)0x33);
      run<true>(src, prow, again.data());
      CHECK(memcmp(blob.data(), again.data(), (size_t)used) == 0);                           // padding included: deterministic
      // the destination: junk everywhere, another stream's position
      for (int r = 0; r < kNR; ++r) for (float& v : dst.ring[r]) v = -777.f;
      for (int s = 0; s < kSlots; ++s) dst.pos[s] = 424242;
      for (uint32_t& w : dst.odd) w = 0xdeadbeefu;
      for (float& v : dst.fe) v = 5.f;
      const snap::CallRow urow = {to, 1, (int)dst.lay.sec_end[snap::SEC_FE], 0};             // the walk covers the unused section: it is cleared
      run<false>(dst, urow, blob.data());
      const int p = pos + from;
      CHECK(dst.pos[to] == p && dst.pos[0] == 424242 && dst.pos[1] == 424242);
      for (int r = 0; r < kNR; ++r) {
        const int C = kRings[r].C, L = dst.L[r], H = kRings[r].hist;
        std::vector<char> written((size_t)L, 0);
        for (int j = 0; j < H; ++j) {
          const long long t = (long long)p * kRings[r].rate - H + j;
          const int row = (int)(t & (L - 1));
          written[row] = 1;
          for (int c = 0; c < C; ++c) CHECK(dst.ring[r][((size_t)to * L + row) * C + c] == val(r, from, t, c));
        }
        for (int row = 0; row < L; ++row)
          if (!written[row]) for (int c = 0; c < C; ++c) CHECK(dst.ring[r][((size_t)to * L + row) * C + c] == -777.f);
        for (int s = 0; s < 2; ++s) for (size_t i = 0; i < (size_t)L * C; ++i) CHECK(dst.ring[r][(size_t)s * L * C + i] == -777.f);
      }
      for (int w = 0; w < kOddWords; ++w) CHECK(dst.odd[to * kOddWords + w] == 0xabc00000u + from * 64 + w);
      for (int w = 0; w < kOddWords; ++w) CHECK(dst.odd[1 * kOddWords + w] == 0xdeadbeefu);
      for (int i = 0; i < 64; ++i) CHECK(dst.fe[to * 64 + i] == 0.f && dst.fe[1 * 64 + i] == 5.f);
    }
  printf("OK\n");
  return 0;
}
"""


def test_layout_pack_unpack_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not present")
    src = tmp_path / "layout_check.cpp"
    src.write_text(LAYOUT_PROGRAM)
    exe = tmp_path / "layout_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
