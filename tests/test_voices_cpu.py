"""CPU checks of the voice bank (conan_voices_*, conan_streams_set_voice[_mix], ABI 9): the exported symbols, the header compiled as
plain C against the ctypes mirrors, null handles, the engine's argument checks, and csrc/voice_layout.h - the row layout and the cell
functions the GPU kernels run - compiled into a stand-alone program with AddressSanitizer and UBSan."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conan_amd import _lib

SYMBOLS = ("conan_voices_create", "conan_voices_destroy", "conan_voices_enroll", "conan_voices_remove", "conan_voices_info",
           "conan_streams_set_voice", "conan_streams_set_voice_mix", "conan_streams_voice", "conan_voices_blob_bytes", "conan_voices_export",
           "conan_voices_import", "conan_voice_meta_info")
CSRC = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    return _lib.lib()


def test_library_exports_voice_symbols():
    _lib_or_skip()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.declared_symbols() and name in _lib._PROTOS
    assert raw.conan_abi_version() == 9 and _lib.ABI_VERSION == 9


def test_header_structs_match_binding(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not present")
    inc = os.path.dirname(_lib.HEADER_PATH)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "conan_hip.h"\n'
                     'int main(void) {\n'
                     '  printf("%d %zu %zu %zu %zu %zu %zu %zu\\n", CONAN_VOICE_META_BYTES, sizeof(conan_voice_meta), sizeof(conan_voice_info),\n'
                     '         offsetof(conan_voice_info, ref_frames), offsetof(conan_voice_info, tokens), offsetof(conan_voice_info, bytes),\n'
                     '         offsetof(conan_voice_info, layout_id), offsetof(conan_voice_meta, opaque));\n'
                     '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, str(probe), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [_lib.VOICE_META_BYTES, C.sizeof(_lib.VoiceMeta), C.sizeof(_lib.VoiceInfo), _lib.VoiceInfo.ref_frames.offset,
                   _lib.VoiceInfo.tokens.offset, _lib.VoiceInfo.bytes.offset, _lib.VoiceInfo.layout_id.offset, _lib.VoiceMeta.opaque.offset]
    assert out[:2] == [256, 256]
    protos = tmp_path / "protos.c"
    protos.write_text('#include "conan_hip.h"\n'
                      'int (*a)(conan_ctx*, int, int, conan_voices**) = conan_voices_create;\n'
                      'int (*b)(conan_voices*) = conan_voices_destroy;\n'
                      'int (*c)(conan_voices*, conan_streams*, const int32_t*, int, const float*, const int32_t*, int, void*) = conan_voices_enroll;\n'
                      'int (*d)(conan_voices*, const int32_t*, int) = conan_voices_remove;\n'
                      'int (*e)(const conan_voices*, int, conan_voice_info*) = conan_voices_info;\n'
                      'int (*f)(conan_streams*, const int32_t*, int, const conan_voices*, const int32_t*, void*) = conan_streams_set_voice;\n'
                      'int (*g)(conan_streams*, const int32_t*, int, const conan_voices*, const int32_t*, const float*, int, void*) = conan_streams_set_voice_mix;\n'
                      'int (*h)(const conan_streams*, int, int32_t*) = conan_streams_voice;\n'
                      'int64_t (*i)(const conan_voices*) = conan_voices_blob_bytes;\n'
                      'int (*j)(conan_voices*, const int32_t*, int, void*, int64_t, conan_voice_meta*, void*) = conan_voices_export;\n'
                      'int (*k)(conan_voices*, const int32_t*, int, const void*, int64_t, const conan_voice_meta*, void*) = conan_voices_import;\n'
                      'int (*l)(const conan_voice_meta*, conan_voice_info*) = conan_voice_meta_info;\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(protos), "-o", str(tmp_path / "protos.o")], check=True)


def test_null_handles_are_invalid():
    lib = _lib_or_skip()
    meta = (_lib.VoiceMeta * 1)()
    info = _lib.VoiceInfo()
    one = (C.c_int32 * 1)(0)
    w = (C.c_float * 1)(1.0)
    out = C.c_void_p()
    vid = C.c_int32(7)
    fake = C.c_void_p(8)      # never dereferenced: the other handle is null
    assert lib.conan_voices_create(None, 4, 64, C.byref(out)) == _lib.ERR_INVALID
    assert b"null argument" in lib.conan_last_error()
    assert lib.conan_voices_enroll(None, fake, one, 1, fake, one, 4, None) == _lib.ERR_INVALID
    assert lib.conan_voices_enroll(fake, None, one, 1, fake, one, 4, None) == _lib.ERR_INVALID
    assert lib.conan_voices_remove(None, one, 1) == _lib.ERR_INVALID
    assert lib.conan_voices_info(None, 0, C.byref(info)) == _lib.ERR_INVALID
    assert lib.conan_streams_set_voice(None, one, 1, fake, one, None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_voice(fake, one, 1, None, one, None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_voice_mix(None, one, 1, fake, one, w, 1, None) == _lib.ERR_INVALID
    assert lib.conan_streams_set_voice_mix(fake, one, 1, None, one, w, 1, None) == _lib.ERR_INVALID
    assert lib.conan_streams_voice(None, 0, C.byref(vid)) == _lib.ERR_INVALID
    assert lib.conan_voices_blob_bytes(None) == _lib.ERR_INVALID
    assert lib.conan_voices_export(None, one, 1, fake, 256, meta, None) == _lib.ERR_INVALID
    assert lib.conan_voices_import(None, one, 1, fake, 256, meta, None) == _lib.ERR_INVALID
    assert lib.conan_voice_meta_info(None, None) == _lib.ERR_INVALID
    assert lib.conan_voice_meta_info(C.byref(meta[0]), C.byref(info)) == _lib.ERR_INVALID      # zeroed: not a record
    assert b"not a voice record" in lib.conan_last_error()


def test_engine_takes_a_reference_or_a_voice_not_both():
    from conan_amd.engine import StreamingVoiceConversionEngine as Engine
    eng = Engine.__new__(Engine)      # no context, no stream-set: the checks must come before either is touched
    bank = object()
    calls = [lambda **kw: eng.start(kw.pop("ref_mel"), **kw), lambda **kw: eng.start_wav(kw.pop("ref_mel"), **kw),
             lambda **kw: eng.open_slots([0], kw.pop("ref_mel"), **kw), lambda **kw: eng.infer(None, kw.pop("ref_mel"), **kw),
             lambda **kw: eng.infer_wav(None, kw.pop("ref_mel"), **kw), lambda **kw: eng.infer_wav_staggered([], [], kw.pop("ref_mel"), **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="not both and not neither"):
            call(ref_mel=object(), voice=(bank, [0]))
        with pytest.raises(ValueError, match="not both and not neither"):
            call(ref_mel=None)
    with pytest.raises(ValueError, match="bank= and ids="):
        eng.set_voice()


LAYOUT_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "voice_layout.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

constexpr int H = 24;      // a multiple of 8 that is no power of two: 6 style cells, 12 cells per K/V row

// a set of caches in exactly sized host arrays (the sanitizer sees every byte past them)
struct Set {
  int n, S;
  std::vector<float> style, kv, kmask; std::vector<int> slen, ids;
  Set(int n_, int S_) : n(n_), S(S_), style((size_t)n_ * H), kv((size_t)n_ * 2 * S_ * 2 * H), kmask((size_t)n_ * S_), slen(n_), ids((size_t)n_ * S_) {}
  voice::Cache cache() { return voice::Cache{style.data(), kv.data(), kmask.data(), slen.data(), ids.data(), S, H}; }
  void junk() {
    for (float& v : style) v = -777.f;
    for (float& v : kv) v = -777.f;
    for (float& v : kmask) v = -777.f;
    for (int& v : slen) v = 424242;
    for (int& v : ids) v = 424242;
  }
};

static float sval(int voice, int c) { return (float)(1 + voice * 1009 + c); }
static float kval(int voice, int l, int r, int c) { return (float)(5 + voice * 100003 + l * 50021 + r * 211 + c); }
static float mval(int voice, int r) { return (voice + r) % 3 == 0 ? -__builtin_inff() : 0.f; }
static int ival(int voice, int r) { return voice * 37 + r * 5 + 1; }

// what the style pass leaves in entry e for a voice of `tokens` tokens; rows past them keep the junk (a bank entry that held a longer voice)
static void enrol(Set& s, int e, int voice, int tokens) {
  for (int c = 0; c < H; ++c) s.style[(size_t)e * H + c] = sval(voice, c);
  for (int l = 0; l < 2; ++l) for (int r = 0; r < tokens; ++r) for (int c = 0; c < 2 * H; ++c) s.kv[(((size_t)e * 2 + l) * s.S + r) * 2 * H + c] = kval(voice, l, r, c);
  for (int r = 0; r < tokens; ++r) { s.kmask[(size_t)e * s.S + r] = mval(voice, r); s.ids[(size_t)e * s.S + r] = ival(voice, r); }
  s.slen[e] = tokens;
}

// entry e holds the voice and, past its tokens, mask 0, ids -1, K/V 0
static int holds(Set& s, int e, int voice, int tokens, float wsum = 1.f) {
  for (int c = 0; c < H; ++c) CHECK(s.style[(size_t)e * H + c] == wsum * sval(voice, c));
  for (int l = 0; l < 2; ++l) for (int r = 0; r < s.S; ++r) for (int c = 0; c < 2 * H; ++c)
    CHECK(s.kv[(((size_t)e * 2 + l) * s.S + r) * 2 * H + c] == (r < tokens ? kval(voice, l, r, c) : 0.f));
  for (int r = 0; r < s.S; ++r) {
    const float m = s.kmask[(size_t)e * s.S + r];
    CHECK(r < tokens ? (m == mval(voice, r)) : (m == 0.f && !__builtin_signbit(m)));
    CHECK(s.ids[(size_t)e * s.S + r] == (r < tokens ? ival(voice, r) : -1));
  }
  CHECK(s.slen[e] == tokens);
  return 0;
}

static int untouched(Set& s, int e) {
  for (int c = 0; c < H; ++c) CHECK(s.style[(size_t)e * H + c] == -777.f);
  for (size_t i = 0; i < (size_t)2 * s.S * 2 * H; ++i) CHECK(s.kv[(size_t)e * 2 * s.S * 2 * H + i] == -777.f);
  for (int r = 0; r < s.S; ++r) CHECK(s.kmask[(size_t)e * s.S + r] == -777.f && s.ids[(size_t)e * s.S + r] == 424242);
  CHECK(s.slen[e] == 424242);
  return 0;
}

// the kernels' walks
static void fill(const voice::Cache& dst, int e, const voice::Src* src, const float* w, int k) {
  for (int item = 0; item < voice::fill_items(dst.S_max, dst.H); ++item)
    for (int lane = 0; lane < voice::kLanes; ++lane) voice::fill_cells(dst, e, src, w, k, item, lane);
}
static void pack(const voice::Cache& bank, int e, int tokens, char* row) {
  for (int item = 0; item < voice::pack_items(bank.H, tokens); ++item)
    for (int lane = 0; lane < voice::kLanes; ++lane) voice::pack_cell(bank, e, tokens, row, (long long)item * voice::kLanes + lane);
}

int main() {
  const int sizes[] = {3, 5, 16, 130};      // S_max: not a multiple of 4 (dword alignment of the mask and the ids), several head items at 130
  // ---- the row: regions in order, each a whole number of cells
  for (int tokens : {1, 3, 16}) {
    const voice::RowOff o = voice::row_off(H, tokens);
    CHECK(o.count == H * 4 && o.ids == o.count + 16 && o.mask == o.ids + (tokens * 4 + 15) / 16 * 16 && o.kv[0] == o.mask + (o.mask - o.ids));
    CHECK(o.kv[1] == o.kv[0] + tokens * 2 * H * 4 && o.bytes == o.kv[1] + tokens * 2 * H * 4 && o.bytes % 16 == 0);
  }
  CHECK(voice::layout_id(256, 2, 80, 128) == voice::layout_id(256, 2, 80, 128));
  CHECK(voice::layout_id(256, 2, 80, 128) != voice::layout_id(128, 2, 80, 128) && voice::layout_id(256, 2, 80, 128) != voice::layout_id(256, 4, 80, 128));
  CHECK(voice::layout_id(256, 2, 80, 128) != voice::layout_id(256, 2, 64, 128) && voice::layout_id(256, 2, 80, 128) != voice::layout_id(256, 2, 80, 64));
  const float one[voice::kMaxMix] = {1.f, 0.f, 0.f, 0.f};
  for (int Sa : sizes) for (int Sb : sizes) for (int tokens : {1, 3, Sa < Sb ? Sa : Sb}) {
    // ---- pack out of a bank of S_max Sa (entry 2 of 3), unpack into entry 1 of a junk-filled bank of S_max Sb
    Set a(3, Sa), b(3, Sb);
    a.junk(); b.junk();
    const int voice_no = Sa * 7 + tokens;
    enrol(a, 2, voice_no, tokens);
    const int bytes = voice::row_off(H, tokens).bytes;
    std::vector<char> row((size_t)bytes), again((size_t)bytes);      // exactly sized: a write past the used bytes is a sanitizer error
    memset(row.data(), 0x5a, row.size()); memset(again.data(), 0x33, again.size());
    pack(a.cache(), 2, tokens, row.data());
    pack(a.cache(), 2, tokens, again.data());
    CHECK(memcmp(row.data(), again.data(), row.size()) == 0);       // padding included: a row is a function of the voice
    CHECK(*reinterpret_cast<int*>(row.data() + H * 4) == tokens);
    voice::Src src[voice::kMaxMix];
    for (int j = 0; j < voice::kMaxMix; ++j) src[j] = voice::src_of_row(row.data(), H, tokens);
    fill(b.cache(), 1, src, one, 1);
    if (holds(b, 1, voice_no, tokens) || untouched(b, 0) || untouched(b, 2)) return 1;
    // ---- and back: the round trip is the identity on the row
    std::vector<char> back((size_t)bytes, (char)0x11);
    pack(b.cache(), 1, tokens, back.data());
    CHECK(memcmp(row.data(), back.data(), row.size()) == 0);
    // ---- assignment: bank entry -> slot of a stream-set of S_max Sb, straight from the bank's arrays
    Set slots(4, Sb);
    slots.junk();
    for (int j = 0; j < voice::kMaxMix; ++j) src[j] = voice::src_of_entry(a.cache(), 2, tokens);
    fill(slots.cache(), 3, src, one, 1);
    if (holds(slots, 3, voice_no, tokens) || untouched(slots, 0) || untouched(slots, 2)) return 1;
  }
  // ---- the mix: prosody of voice[0], style = the fma chain in k order
  {
    Set a(4, 8), slots(2, 8);
    a.junk(); slots.junk();
    enrol(a, 0, 11, 5); enrol(a, 1, 12, 8); enrol(a, 3, 13, 2);
    const int order[3] = {1, 3, 0};
    const float w[voice::kMaxMix] = {0.5f, 0.3f, 0.2f, 0.f};
    voice::Src src[voice::kMaxMix];
    for (int j = 0; j < voice::kMaxMix; ++j) src[j] = voice::src_of_entry(a.cache(), order[j < 3 ? j : 0], 8);
    fill(slots.cache(), 1, src, w, 3);
    for (int c = 0; c < H; ++c) {
      float acc = w[0] * sval(12, c);
      acc = __builtin_fmaf(w[1], sval(13, c), acc);
      acc = __builtin_fmaf(w[2], sval(11, c), acc);
      CHECK(slots.style[(size_t)1 * H + c] == acc);
    }
    for (int c = 0; c < H; ++c) slots.style[(size_t)1 * H + c] = sval(12, c);      // (the rest is voice 12's)
    if (holds(slots, 1, 12, 8) || untouched(slots, 0)) return 1;
  }
  printf("OK\n");
  return 0;
}
"""


def test_voice_layout_pack_unpack_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not present")
    src = tmp_path / "voice_layout_check.cpp"
    src.write_text(LAYOUT_PROGRAM)
    exe = tmp_path / "voice_layout_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
