// Slot snapshots (snapshot.hip): the layout of one slot's blob row and the function that moves one 16-byte cell of it.
// No HIP dependency: the kernels of snapshot.hip and a stand-alone CPU program compile the same code.
//
// A blob row is a sequence of regions, each padded to 16 bytes, in the order they were added.  A region is either a ring, saved as
// its history - the `rows` rows a future step can still read, oldest first - or a whole per-slot block.  The row holds no pointers, no
// slot numbers and no ring indices: a ring's rows are addressed by the stream position, which travels in the row itself (a padded
// 16-byte cell per position counter) or in the call row (counters the host keeps).
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define SNAP_HD __host__ __device__
#else
#define SNAP_HD
#endif

namespace snap {

constexpr int kCell = 16;             // bytes every lane moves per access
constexpr int kItemBytes = 8192;      // a work item: 256 lanes x 2 cells
constexpr int kRowAlign = 256;        // snapshot_bytes is a multiple of this

enum Kind : int { KIND_RING = 0, KIND_WHOLE = 1 };
// sections of the row, in this order; the core is always present, the others only for slots that use them.  SEC_LEVEL (the input
// leveller's state, one whole block) came later: its regions are not part of the layout id, so the ids of stream-sets - and the
// blobs written before it existed, which simply end before it - stay what they were.
enum Section : int { SEC_CORE = 0, SEC_FE = 1, SEC_RS_IN = 2, SEC_RS_OUT = 3, SEC_LEVEL = 4, SEC_COUNT = 5 };

struct Region {
  char* base;               // slot 0's block on the device (null: not allocated - only in sections no slot can have yet)
  const int* pos;           // ring: the per-slot position counters on the device (null: the call row's aux position)
  long long slot_stride;    // bytes between slots
  long long blob_off;       // bytes from the start of the row; a multiple of kCell
  int bytes;                // bytes saved: rows * row_bytes (ring) or the block's size (whole)
  int row_bytes;            // ring: bytes of a row
  int lmask;                // ring: rows of the ring - 1
  int rate;                 // ring: rows per position step
  int rows;                 // ring: rows saved (its history)
  int kind, section;
  int pos_cell;             // ring: offset in the row of the cell that holds the exported position (-1: the call row's aux position)
  int aligned;              // every cell is one aligned 16-byte access on the device side too
  int zero_absent;          // import of a row without this section clears the destination block
};

// one slot of an export / import call
struct CallRow { int slot, present, used_bytes, aux; };      // present: bit per section; aux: position of the rings without a device counter

struct alignas(16) Vec16 { uint32_t w[4]; };

// Row of a ring that holds history row j (0 = oldest of `hist` rows) of a stream at position `pos`.  Rows before the start of the
// utterance (negative logical rows) wrap like any other: they hold the zeros that reset put there.
SNAP_HD inline int ring_row(long long pos, int rate, int hist, int j, int lmask) {
  return (int)((pos * rate - hist + j) & (long long)lmask);
}

SNAP_HD inline int pad_cell(int bytes) { return (bytes + kCell - 1) & ~(kCell - 1); }

// device address of byte `o` (a multiple of 4) of region r's saved bytes
SNAP_HD inline char* region_addr(const Region& r, int slot, int o, long long pos) {
  char* p = r.base + (long long)slot * r.slot_stride;
  if (r.kind == KIND_WHOLE) return p + o;
  const int j = o / r.row_bytes, col = o - j * r.row_bytes;
  return p + (long long)ring_row(pos, r.rate, r.rows, j, r.lmask) * r.row_bytes + col;
}

// Moves the cell at byte `off` of a row: PACK state -> blob, else blob -> state.  `first` is a region at or before the cell's.
template <bool PACK>
SNAP_HD inline void move_cell(const Region* regs, int first, const CallRow& row, char* blob_row, long long off) {
  int ri = first;
  while (off >= regs[ri].blob_off + pad_cell(regs[ri].bytes)) ++ri;
  const Region& r = regs[ri];
  const int o = (int)(off - r.blob_off);
  Vec16* cell = reinterpret_cast<Vec16*>(blob_row + off);
  if (!((row.present >> r.section) & 1)) {      // a section this slot does not use (it lies before one it does)
    if (PACK) { *cell = Vec16{{0u, 0u, 0u, 0u}}; return; }
    if (!r.zero_absent) return;
    for (int k = 0; k < 4; ++k)
      if (o + 4 * k < r.bytes) *reinterpret_cast<uint32_t*>(r.base + (long long)row.slot * r.slot_stride + o + 4 * k) = 0u;
    return;
  }
  long long pos = 0;
  if (r.kind == KIND_RING) {
    if (PACK) pos = r.pos ? r.pos[row.slot] : row.aux;
    else pos = r.pos_cell >= 0 ? *reinterpret_cast<const int*>(blob_row + r.pos_cell) : row.aux;
  }
  if (r.aligned) {
    Vec16* dev = reinterpret_cast<Vec16*>(region_addr(r, row.slot, o, pos));
    if (PACK) *cell = *dev; else *dev = *cell;
    return;
  }
  Vec16 v = PACK ? Vec16{{0u, 0u, 0u, 0u}} : *cell;
  for (int k = 0; k < 4; ++k) {
    if (o + 4 * k >= r.bytes) break;      // (the padding of the region's last cell: written as zero, never read back)
    uint32_t* dev = reinterpret_cast<uint32_t*>(region_addr(r, row.slot, o + 4 * k, pos));
    if (PACK) v.w[k] = *dev; else *dev = v.w[k];
  }
  if (PACK) *cell = v;
}

// ---------------------------------------------------------------------------------------------------------------- host side

struct Layout {
  std::vector<Region> regions;
  std::vector<int> item_first;          // per work item of kItemBytes: the region that holds its first cell
  long long bytes = 0;                  // per slot, all sections, a multiple of kRowAlign (after finish)
  long long sec_end[SEC_COUNT] = {};      // end of each section's last region
  uint64_t id = 0;
  int items(long long used_bytes) const { return (int)((used_bytes + kItemBytes - 1) / kItemBytes); }
};

inline uint64_t fnv1a(uint64_t h, const void* data, size_t n) {
  const unsigned char* p = static_cast<const unsigned char*>(data);
  for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}
constexpr uint64_t kFnvSeed = 14695981039346656037ull;

inline int push_region(Layout& l, Region r) {
  r.blob_off = l.bytes;
  const bool unit16 = r.kind == KIND_RING ? (r.row_bytes % kCell == 0) : (r.bytes % kCell == 0);
  r.aligned = (unit16 && r.slot_stride % kCell == 0 && reinterpret_cast<uintptr_t>(r.base) % kCell == 0) ? 1 : 0;
  l.bytes += pad_cell(r.bytes);
  l.sec_end[r.section] = l.bytes;
  l.regions.push_back(r);
  return (int)l.regions.size() - 1;
}

// A ring of L rows of C floats, `rate` rows per position step, whose steps read at most `hist` rows back.  Regions must be added
// section by section, in the order of Section.
inline int add_ring(Layout& l, void* base, long long slot_stride_bytes, int C, int L, int rate, int hist, const int* pos, int pos_cell, int section) {
  Region r; memset(&r, 0, sizeof(r));
  r.base = static_cast<char*>(base); r.pos = pos; r.slot_stride = slot_stride_bytes;
  r.row_bytes = C * 4; r.lmask = L - 1; r.rate = rate; r.rows = hist < L ? hist : L; r.bytes = r.rows * r.row_bytes;
  r.kind = KIND_RING; r.section = section; r.pos_cell = pos_cell;
  return push_region(l, r);
}

inline int add_whole(Layout& l, void* base, long long slot_stride_bytes, int bytes, int section, bool zero_absent = false) {
  Region r; memset(&r, 0, sizeof(r));
  r.base = static_cast<char*>(base); r.slot_stride = slot_stride_bytes; r.bytes = bytes;
  r.kind = KIND_WHOLE; r.section = section; r.pos_cell = -1; r.zero_absent = zero_absent ? 1 : 0;
  return push_region(l, r);
}

// Closes the layout: the work items' prefix table, the row size and the id - a hash over `cfg` (the caller's words: the configuration
// fields that size state, the arithmetic, S_max) and the ordered regions' kind, section, row width, rate and saved rows / bytes.
// Addresses, strides, ring lengths and the regions of SEC_LEVEL are not part of it.
inline void finish(Layout& l, const int32_t* cfg, int ncfg) {
  l.bytes = (l.bytes + kRowAlign - 1) / kRowAlign * kRowAlign;
  l.item_first.clear();
  int ri = 0;
  for (long long off = 0; off < l.bytes; off += kItemBytes) {
    while (ri + 1 < (int)l.regions.size() && off >= l.regions[ri].blob_off + pad_cell(l.regions[ri].bytes)) ++ri;
    l.item_first.push_back(ri);
  }
  uint64_t h = fnv1a(kFnvSeed, cfg, sizeof(int32_t) * (size_t)ncfg);
  for (const Region& r : l.regions) {
    if (r.section == SEC_LEVEL) continue;
    const int32_t w[6] = {r.kind, r.section, r.row_bytes, r.rate, r.rows, r.bytes};
    h = fnv1a(h, w, sizeof(w));
  }
  l.id = h;
}

// bytes of a row that carries the sections of `present` (bit per section; the core always): up to the end of its last section
inline long long used_bytes(const Layout& l, int present) {
  long long u = l.sec_end[SEC_CORE];
  for (int sec = 1; sec < SEC_COUNT; ++sec) if ((present >> sec) & 1) u = l.sec_end[sec];
  return u;
}

}  // namespace snap
