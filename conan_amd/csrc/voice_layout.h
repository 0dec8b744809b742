// Voice bank (voices.hip): a target voice's style cache as a position-independent row, and the functions that move 16-byte cells
// between rows, bank entries and slots.  No HIP dependency: the kernels of voices.hip and a stand-alone CPU program compile the same
// code.
//
// A style cache is what the reference-mel side of Conan.forward leaves behind: the style vector [H], the cross-attention K/V rows of
// the prosody tokens [2 layers][S_max][2H], their key mask [S_max], the token count and the VQ ids [S_max].  A stream-set holds one per
// slot and a bank one per entry (`Cache`: the same five arrays, indexed by slot or by voice id, each with its own S_max).
//
// A row holds one voice, sized by its token count alone - style, count, ids, mask, then the K/V rows of its tokens per layer, each
// region padded to a 16-byte cell (`row_off`) - so it moves between banks of any capacity and any S_max that holds the voice.
//
// `fill_cells` writes a whole destination entry from a source voice (a bank entry or a row): the voice's tokens, and past them what
// conan_set_reference leaves in a freshly created slot - mask 0, ids -1, K/V 0 - so an entry is a function of the voice alone.
#pragma once
#include <cstdint>

#include "snapshot_layout.h"

#define VOICE_HD SNAP_HD

namespace voice {

using snap::Vec16;
using snap::pad_cell;

constexpr int kCell = snap::kCell;
constexpr int kLanes = 256;                  // lanes of a work item
constexpr int kKvCells = 2 * kLanes;         // K/V cells of a K/V work item: two per lane, both loaded before either is stored
constexpr int kMaxMix = 4;                   // voices a slot's style vector can blend
constexpr uint32_t kVersion = 1;

// the five arrays of a stream-set's slots or of a bank's entries
struct Cache {
  float* style;      // [index][H]
  float* kv;         // [index][2][S_max][2H]
  float* kmask;      // [index][S_max]
  int* slen;         // [index]
  int* vqids;        // [index][S_max]
  int S_max, H;      // H is a multiple of 8: style and K/V rows are whole cells
};

// one voice where it lies: the K/V rows of a layer are contiguous, 2H floats each
struct Src { const char* style; const char* kv[2]; const char* mask; const char* ids; int tokens; };

// one slot of an assignment: voice[0] gives the prosody side, the style vector blends voice[0 .. k-1] (entries past k repeat voice[0])
struct AssignRow { int slot, tokens; int voice[kMaxMix]; float w[kMaxMix]; int pad_[2]; };
// one entry of an export / import
struct MoveRow { int entry, tokens, pad_[2]; };

// byte offsets of a row's regions
struct RowOff { int count, ids, mask, kv[2], bytes; };

VOICE_HD inline RowOff row_off(int H, int tokens) {
  RowOff o;
  o.count = H * 4;
  o.ids = o.count + kCell;
  o.mask = o.ids + pad_cell(tokens * 4);
  o.kv[0] = o.mask + pad_cell(tokens * 4);
  o.kv[1] = o.kv[0] + tokens * 2 * H * 4;
  o.bytes = o.kv[1] + tokens * 2 * H * 4;
  return o;
}

VOICE_HD inline Src src_of_entry(const Cache& c, int e, int tokens) {
  Src s;
  const long long S = c.S_max, H = c.H;
  s.style = reinterpret_cast<const char*>(c.style + e * H);
  s.kv[0] = reinterpret_cast<const char*>(c.kv + e * 2 * S * 2 * H);
  s.kv[1] = s.kv[0] + S * 2 * H * 4;
  s.mask = reinterpret_cast<const char*>(c.kmask + e * S);
  s.ids = reinterpret_cast<const char*>(c.vqids + e * S);
  s.tokens = tokens;
  return s;
}

VOICE_HD inline Src src_of_row(const char* row, int H, int tokens) {
  const RowOff o = row_off(H, tokens);
  Src s;
  s.style = row; s.kv[0] = row + o.kv[0]; s.kv[1] = row + o.kv[1]; s.mask = row + o.mask; s.ids = row + o.ids; s.tokens = tokens;
  return s;
}

// ---- fill: destination entry <- source voice.  Work items of kLanes lanes: `head_items` head items (the key mask, the ids and the
// count, one dword per lane; item 0 also the style vector, one cell per lane), then the K/V items (kKvCells cells each).
VOICE_HD inline int head_items(int S_max) { return (2 * S_max + 1 + kLanes - 1) / kLanes; }
VOICE_HD inline int kv_items(int S_max, int H) { return (S_max * H + kKvCells - 1) / kKvCells; }      // 2 layers x S_max rows x H / 2 cells
VOICE_HD inline int fill_items(int S_max, int H) { return head_items(S_max) + kv_items(S_max, H); }

VOICE_HD inline float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
VOICE_HD inline uint32_t as_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// Lane `lane` of work item `item` of entry `e`.  src[0] gives the prosody side; the style vector is the fp32 chain
// w[0] * style_0, then fmaf(w[j], style_j, .) for j = 1 .. k-1 (k = 1, w = 1: a copy).  Every load is unconditional at a clamped
// address - the condition applies to the value - so the loads of a lane leave together; src[j] for j >= k must be readable too (the
// caller repeats src[0]).
VOICE_HD inline void fill_cells(const Cache& dst, int e, const Src* src, const float* w, int k, int item, int lane) {
  const int S = dst.S_max, H = dst.H, tokens = src[0].tokens;
  const int heads = head_items(S);
  if (item < heads) {
    if (item == 0) {      // the style vector (H / 4 <= 128 cells)
      const int nc = H / 4, c = lane < nc ? lane : nc - 1;
      Vec16 v[kMaxMix];
      for (int j = 0; j < kMaxMix; ++j) v[j] = reinterpret_cast<const Vec16*>(src[j].style)[c];
      Vec16 out;
      for (int q = 0; q < 4; ++q) {
        float acc = w[0] * as_float(v[0].w[q]);
        for (int j = 1; j < kMaxMix; ++j) acc = j < k ? __builtin_fmaf(w[j], as_float(v[j].w[q]), acc) : acc;
        out.w[q] = as_bits(acc);
      }
      if (lane < nc) reinterpret_cast<Vec16*>(dst.style + (long long)e * H)[c] = out;
    }
    const int t = item * kLanes + lane;      // dword t of: mask [S], ids [S], count
    const bool is_ids = t >= S;
    const int u = is_ids ? t - S : t;
    const int uc = u < tokens ? u : tokens - 1;
    const uint32_t got = *reinterpret_cast<const uint32_t*>((is_ids ? src[0].ids : src[0].mask) + (long long)uc * 4);
    uint32_t val = u < tokens ? got : (is_ids ? 0xffffffffu : 0u);
    if (t == 2 * S) val = (uint32_t)tokens;
    if (t < S) reinterpret_cast<uint32_t*>(dst.kmask + (long long)e * S)[u] = val;
    else if (t < 2 * S) reinterpret_cast<uint32_t*>(dst.vqids + (long long)e * S)[u] = val;
    else if (t == 2 * S) reinterpret_cast<uint32_t*>(dst.slen)[e] = val;
    return;
  }
  // K/V: cell c of the entry's [2][S][H / 2] cells
  const int rc = H / 2, total = S * H;
  Vec16 v[2]; int row[2]; long long cell[2];
  for (int p = 0; p < 2; ++p) {
    long long c = (long long)(item - heads) * kKvCells + p * kLanes + lane;
    cell[p] = c;
    if (c >= total) c = total - 1;
    const int l = (int)(c / ((long long)S * rc)), rem = (int)(c - (long long)l * S * rc);
    const int r = rem / rc, col = rem - r * rc;
    row[p] = r;
    const int rs = r < tokens ? r : tokens - 1;
    v[p] = reinterpret_cast<const Vec16*>(l ? src[0].kv[1] : src[0].kv[0])[(long long)rs * rc + col];
  }
  Vec16* out = reinterpret_cast<Vec16*>(dst.kv + (long long)e * 2 * S * 2 * H);
  for (int p = 0; p < 2; ++p) {
    if (row[p] >= tokens) v[p] = Vec16{{0u, 0u, 0u, 0u}};
    if (cell[p] < total) out[cell[p]] = v[p];
  }
}

// ---- pack: row <- bank entry.  One cell per lane: cell `idx` of the row's row_off(H, tokens).bytes / 16.  The padding of the
// count, ids and mask regions is written as zero, so a row is a function of the voice.
VOICE_HD inline int pack_items(int H, int tokens) { return (row_off(H, tokens).bytes / kCell + kLanes - 1) / kLanes; }

VOICE_HD inline void pack_cell(const Cache& bank, int e, int tokens, char* row, long long idx) {
  const RowOff o = row_off(bank.H, tokens);
  const long long off = idx * kCell;
  if (off >= o.bytes) return;
  const Src s = src_of_entry(bank, e, tokens);
  Vec16 v = Vec16{{0u, 0u, 0u, 0u}};
  if (off < o.count) v = *reinterpret_cast<const Vec16*>(s.style + off);
  else if (off < o.ids) v.w[0] = (uint32_t)tokens;
  else if (off < o.kv[0]) {      // ids, then mask: dword by dword (a bank's S_max need not be a multiple of 4)
    const bool m = off >= o.mask;
    const int first = (int)(off - (m ? o.mask : o.ids)) / 4;
    const uint32_t* p = reinterpret_cast<const uint32_t*>(m ? s.mask : s.ids);
    for (int q = 0; q < 4; ++q) if (first + q < tokens) v.w[q] = p[first + q];
  } else {
    const int l = off >= o.kv[1] ? 1 : 0;
    v = *reinterpret_cast<const Vec16*>(s.kv[l] + (off - o.kv[l]));
  }
  *reinterpret_cast<Vec16*>(row + off) = v;
}

// the id a row's record carries: the fields that size a voice and the row structure
inline uint64_t layout_id(int hidden_size, int heads, int num_mels, int nvq) {
  const int32_t w[] = {(int32_t)kVersion, hidden_size, heads, num_mels, nvq, kCell, /* regions, in order: */ 'S', 'C', 'I', 'M', 'K', 'K'};
  return snap::fnv1a(snap::kFnvSeed, w, sizeof(w));
}

}  // namespace voice
