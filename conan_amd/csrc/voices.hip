// Voice bank: enrolled target voices in device memory outside any slot, their assignment to slots in one launch, and their export /
// import as position-independent rows (include/conan_hip.h).  The row layout and the cell functions are voice_layout.h's.
#include <cmath>

#include "streams.h"

namespace cnk {

// Slot rows[y].slot's style cache <- voice rows[y].voice[0] of the bank (style vector: the blend of voice[0 .. k-1]).  Work item x of
// voice::fill_items: 256 lanes, one dword or one or two 16-byte cells each; plain vector loads and stores, no atomics, no waits.  Every
// byte of the slot's cache belongs to exactly one lane.
__global__ __launch_bounds__(256) void voice_assign_kernel(const voice::Cache dst, const voice::Cache bank, const voice::AssignRow* __restrict__ rows, int k) {
  const voice::AssignRow row = rows[blockIdx.y];
  voice::Src src[voice::kMaxMix];
#pragma unroll
  for (int j = 0; j < voice::kMaxMix; ++j) src[j] = voice::src_of_entry(bank, row.voice[j], row.tokens);
  voice::fill_cells(dst, row.slot, src, row.w, k, (int)blockIdx.x, (int)threadIdx.x);
}

// Bank entry rows[y].entry <- row y of the blob (import), by the same walk
__global__ __launch_bounds__(256) void voice_unpack_kernel(const voice::Cache bank, const voice::MoveRow* __restrict__ rows, const char* __restrict__ blob, long long blob_ld) {
  const voice::MoveRow row = rows[blockIdx.y];
  voice::Src src[voice::kMaxMix];
  const float w[voice::kMaxMix] = {1.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < voice::kMaxMix; ++j) src[j] = voice::src_of_row(blob + (long long)blockIdx.y * blob_ld, bank.H, row.tokens);
  voice::fill_cells(bank, row.entry, src, w, 1, (int)blockIdx.x, (int)threadIdx.x);
}

// Row y of the blob <- bank entry rows[y].entry (export): one cell per lane
__global__ __launch_bounds__(256) void voice_pack_kernel(const voice::Cache bank, const voice::MoveRow* __restrict__ rows, char* __restrict__ blob, long long blob_ld) {
  const voice::MoveRow row = rows[blockIdx.y];
  voice::pack_cell(bank, row.entry, row.tokens, blob + (long long)blockIdx.y * blob_ld, (long long)blockIdx.x * voice::kLanes + threadIdx.x);
}

}  // namespace cnk

struct conan_voices {
  conan_ctx* ctx = nullptr;
  int capacity = 0, max_ref = 0;
  voice::Cache cache{};                       // the entries' arrays, indexed by voice id
  std::vector<void*> allocs;
  std::vector<char> enrolled;
  std::vector<int> frames, tokens;            // per enrolled id: reference frames, prosody tokens
  uint64_t layout_id = 0;
  StageSets<std::array<int, 4>> sets;         // export / import call rows
  ~conan_voices() { for (void* p : allocs) (void)hipFree(p); }
};

namespace {

constexpr uint32_t kMagic = 0x43564e43u;      // "CNVC"
constexpr int kHeads = 2;                     // the aligner's heads (decoder.hip)

// the host half of an exported voice (conan_voice_meta.opaque)
struct Meta {
  uint32_t magic, version, size, reserved0;
  uint64_t layout_id; int64_t bytes;
  int32_t frames, tokens, hidden_size, reserved1;
  uint64_t checksum;                          // FNV-1a over the record with this field zero
  unsigned char reserved[CONAN_VOICE_META_BYTES - 56];
};
static_assert(sizeof(Meta) == CONAN_VOICE_META_BYTES && sizeof(conan_voice_meta) == CONAN_VOICE_META_BYTES, "the voice record is 256 bytes");
static_assert(sizeof(voice::AssignRow) == 12 * sizeof(int) && sizeof(voice::MoveRow) == 4 * sizeof(int), "call rows are uploaded as ints");

uint64_t meta_sum(Meta m) { m.checksum = 0; return snap::fnv1a(snap::kFnvSeed, &m, sizeof(m)); }

// (the layout id is compared before the checksum: a record of another model shape is CONAN_ERR_SHAPE, whatever else is wrong with it)
Meta read_meta(const conan_voice_meta* rec, const std::string& where, const uint64_t* bank_id = nullptr) {
  Meta m; memcpy(&m, rec, sizeof(m));
  if (m.magic != kMagic) throw Error(CONAN_ERR_INVALID, where + "not a voice record");
  if (m.version != voice::kVersion || m.size != sizeof(Meta)) throw Error(CONAN_ERR_INVALID, where + "voice record of version " + std::to_string(m.version) + " / " + std::to_string(m.size) + " bytes, this library reads version " + std::to_string(voice::kVersion) + " / " + std::to_string(sizeof(Meta)));
  if (bank_id && m.layout_id != *bank_id) {
    char a[24], b[24];
    snprintf(a, sizeof(a), "%016llx", (unsigned long long)m.layout_id); snprintf(b, sizeof(b), "%016llx", (unsigned long long)*bank_id);
    throw Error(CONAN_ERR_SHAPE, where + "layout id " + a + " of the voice differs from this bank's " + b + " (another model shape)");
  }
  if (m.checksum != meta_sum(m)) throw Error(CONAN_ERR_INVALID, where + "voice record is corrupted (checksum)");
  return m;
}

void check_ids(const conan_voices* v, const int32_t* ids, int n, bool distinct, const char* who) {
  if (n < 1 || (distinct && n > v->capacity)) throw Error(CONAN_ERR_INVALID, std::string(who) + ": voice count out of range");
  std::vector<char> seen(distinct ? v->capacity : 0, 0);
  for (int i = 0; i < n; ++i) {
    if (ids[i] < 0 || ids[i] >= v->capacity) throw Error(CONAN_ERR_INVALID, std::string(who) + ": voice id " + std::to_string(ids[i]) + " out of range (capacity " + std::to_string(v->capacity) + ")");
    if (!distinct) continue;
    if (seen[ids[i]]) throw Error(CONAN_ERR_INVALID, std::string(who) + ": duplicate voice id");
    seen[ids[i]] = 1;
  }
}

void check_blob(const void* blob, int64_t ld, const char* who) {
  if (reinterpret_cast<uintptr_t>(blob) % voice::kCell || ld % voice::kCell || ld < 0)
    throw Error(CONAN_ERR_INVALID, std::string(who) + ": blob_dev and blob_ld_bytes must be multiples of 16");
}

}  // namespace

namespace voices {

void create(conan_ctx* ctx, int capacity, int max_ref_frames, conan_voices** out) {
  if (!ctx || !out) throw Error(CONAN_ERR_INVALID, "null argument");
  if (!ctx->finalized) throw Error(CONAN_ERR_STATE, "conan_ctx_finalize must run before conan_voices_create");
  if (!(ctx->cfg.models & CONAN_MODEL_CONAN)) throw Error(CONAN_ERR_STATE, "context holds no Conan model");
  if (capacity < 1 || capacity > (1 << 20)) throw Error(CONAN_ERR_INVALID, "conan_voices_create: capacity out of range");
  if (max_ref_frames < 4 || max_ref_frames > 2048) throw Error(CONAN_ERR_INVALID, "conan_voices_create: max_ref_frames must be 4 .. 2048");
  HIP_CHECK(hipSetDevice(ctx->device));
  conan_voices* v = new conan_voices();
  try {
    const conan_cfg& c = ctx->cfg;
    v->ctx = ctx; v->capacity = capacity; v->max_ref = max_ref_frames;
    const int H = c.hidden_size, S = (max_ref_frames + 3) / 4;
    auto alloc = [&](size_t words) {
      void* p = nullptr;
      HIP_CHECK(hipMalloc(&p, words * 4));
      v->allocs.push_back(p);
      HIP_CHECK(hipMemset(p, 0, words * 4));
      return p;
    };
    v->cache.S_max = S; v->cache.H = H;
    v->cache.style = (float*)alloc((size_t)capacity * H);
    v->cache.kv = (float*)alloc((size_t)capacity * 2 * S * 2 * H);
    v->cache.kmask = (float*)alloc((size_t)capacity * S);
    v->cache.slen = (int*)alloc((size_t)capacity);
    v->cache.vqids = (int*)alloc((size_t)capacity * S);
    v->enrolled.assign(capacity, 0); v->frames.assign(capacity, 0); v->tokens.assign(capacity, 0);
    v->layout_id = voice::layout_id(H, kHeads, c.num_mels, c.nvq);
  } catch (...) { delete v; throw; }
  *out = v;
}

void destroy(conan_voices* v) {
  if (!v) return;
  (void)hipSetDevice(v->ctx->device);
  (void)hipDeviceSynchronize();      // (assignments and exports in flight read the entries)
  delete v;
}

void enroll(conan_voices* v, conan_streams* via, const int32_t* ids, int n, const float* ref_mel_dev, const int32_t* ref_len, int max_len, void* stream) {
  if (!v || !via || !ids || !ref_mel_dev || !ref_len) throw Error(CONAN_ERR_INVALID, "null argument");
  const char* who = "conan_voices_enroll";
  if (via->ctx != v->ctx) throw Error(CONAN_ERR_INVALID, std::string(who) + ": `via` belongs to another context than the bank");
  check_ids(v, ids, n, true, who);
  for (int i = 0; i < n; ++i)
    if (ref_len[i] <= 0 || ref_len[i] > max_len || ref_len[i] > v->max_ref || ref_len[i] > via->max_ref)
      throw Error(CONAN_ERR_INVALID, std::string(who) + ": reference length " + std::to_string(ref_len[i]) + " out of range (max_len " + std::to_string(max_len) +
                                         ", the bank's max_ref_frames " + std::to_string(v->max_ref) + ", via's " + std::to_string(via->max_ref) + ")");
  HIP_CHECK(hipSetDevice(v->ctx->device)); via->check_fault();
  hipStream_t st = (hipStream_t)stream;
  via->join(st);
  via->style_pass(v->cache, false, ids, n, 1, ref_mel_dev, ref_len, max_len, st);
  for (int i = 0; i < n; ++i) { v->enrolled[ids[i]] = 1; v->frames[ids[i]] = ref_len[i]; v->tokens[ids[i]] = (ref_len[i] + 3) / 4; }
}

void remove(conan_voices* v, const int32_t* ids, int n) {
  if (!v || !ids) throw Error(CONAN_ERR_INVALID, "null argument");
  check_ids(v, ids, n, false, "conan_voices_remove");
  for (int i = 0; i < n; ++i) { v->enrolled[ids[i]] = 0; v->frames[ids[i]] = 0; v->tokens[ids[i]] = 0; }
}

void info(const conan_voices* v, int id, conan_voice_info* out) {
  if (!v || !out) throw Error(CONAN_ERR_INVALID, "null argument");
  if (id < 0 || id >= v->capacity) throw Error(CONAN_ERR_INVALID, "conan_voices_info: voice id out of range");
  memset(out, 0, sizeof(*out));
  out->layout_id = v->layout_id;
  if (!v->enrolled[id]) return;
  out->enrolled = 1; out->ref_frames = v->frames[id]; out->tokens = v->tokens[id];
  out->bytes = voice::row_off(v->cache.H, v->tokens[id]).bytes;
}

void set_voice(conan_streams* s, const int32_t* slots, int n, const conan_voices* v, const int32_t* voice_ids, const float* weights, int k, bool mix, void* stream) {
  if (!s || !slots || !v || !voice_ids || (mix && !weights)) throw Error(CONAN_ERR_INVALID, "null argument");
  const char* who = mix ? "conan_streams_set_voice_mix" : "conan_streams_set_voice";
  if (!(s->ctx->cfg.models & CONAN_MODEL_CONAN)) throw Error(CONAN_ERR_STATE, "context holds no Conan model");
  if (v->ctx != s->ctx) throw Error(CONAN_ERR_INVALID, std::string(who) + ": the bank belongs to another context than the stream-set");
  if (k < 1 || k > voice::kMaxMix) throw Error(CONAN_ERR_INVALID, std::string(who) + ": k must be 1 .. 4");
  wavio::check_slot_list(s, slots, n);
  check_ids(v, voice_ids, n * k, false, who);
  std::vector<voice::AssignRow> rows((size_t)n);
  for (int i = 0; i < n; ++i) {
    voice::AssignRow& r = rows[i];
    memset(&r, 0, sizeof(r));
    for (int j = 0; j < k; ++j) {
      const int id = voice_ids[(size_t)i * k + j];
      if (!v->enrolled[id]) throw Error(CONAN_ERR_STATE, std::string(who) + ": voice " + std::to_string(id) + " is not enrolled");
      const float w = mix ? weights[(size_t)i * k + j] : 1.f;
      if (!std::isfinite(w)) throw Error(CONAN_ERR_INVALID, std::string(who) + ": weights must be finite");
      r.voice[j] = id; r.w[j] = w;
    }
    for (int j = k; j < voice::kMaxMix; ++j) r.voice[j] = r.voice[0];      // (read, never used: voice_layout.h)
    r.slot = slots[i]; r.tokens = v->tokens[r.voice[0]];
    if (r.tokens > s->S_max)
      throw Error(CONAN_ERR_SHAPE, std::string(who) + ": voice " + std::to_string(r.voice[0]) + " has " + std::to_string(r.tokens) + " prosody tokens, the stream-set holds " +
                                       std::to_string(s->S_max) + " (max_ref_frames " + std::to_string(s->max_ref) + ")");
  }
  HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
  hipStream_t st = (hipStream_t)stream;
  s->join(st);
  s->voice_sets.init(s->max_slots, s->allocs);
  using Row = std::array<int, sizeof(voice::AssignRow) / sizeof(int)>;
  const int q = s->voice_sets.begin(reinterpret_cast<const Row*>(rows.data()), n, st);
  const voice::Cache dst = s->style_cache();
  const dim3 grid((unsigned)voice::fill_items(dst.S_max, dst.H), (unsigned)n);
  s->profiled("cnk::voice_assign_kernel", 0.0, st, [&] {
    hipLaunchKernelGGL(cnk::voice_assign_kernel, grid, dim3(voice::kLanes), 0, st, dst, v->cache, reinterpret_cast<const voice::AssignRow*>(s->voice_sets.rows[q]), k);
  });
  s->voice_sets.end(q, st);
  for (int i = 0; i < n; ++i) { s->has_ref[slots[i]] = 1; s->voice_of[slots[i]] = mix ? -1 : voice_ids[i]; }
}

void get_voice(const conan_streams* s, int slot, int32_t* voice_id) {
  if (!s || !voice_id) throw Error(CONAN_ERR_INVALID, "null argument");
  if (slot < 0 || slot >= s->max_slots) throw Error(CONAN_ERR_INVALID, "slot index out of range");
  *voice_id = s->voice_of[slot];
}

int64_t blob_bytes(const conan_voices* v) {
  if (!v) throw Error(CONAN_ERR_INVALID, "null voices");
  const long long b = voice::row_off(v->cache.H, v->cache.S_max).bytes;
  return (b + snap::kRowAlign - 1) / snap::kRowAlign * snap::kRowAlign;
}

void export_voices(conan_voices* v, const int32_t* ids, int n, void* blob_dev, int64_t blob_ld, conan_voice_meta* meta, void* stream) {
  if (!v || !ids || !blob_dev || !meta) throw Error(CONAN_ERR_INVALID, "null argument");
  const char* who = "conan_voices_export";
  check_ids(v, ids, n, false, who);
  check_blob(blob_dev, blob_ld, who);
  std::vector<voice::MoveRow> rows((size_t)n);
  int items = 1;
  for (int i = 0; i < n; ++i) {
    if (!v->enrolled[ids[i]]) throw Error(CONAN_ERR_STATE, std::string(who) + ": voice " + std::to_string(ids[i]) + " is not enrolled");
    rows[i] = voice::MoveRow{ids[i], v->tokens[ids[i]], {0, 0}};
    const int bytes = voice::row_off(v->cache.H, rows[i].tokens).bytes;
    if (bytes > blob_ld) throw Error(CONAN_ERR_SHAPE, std::string(who) + ": voice " + std::to_string(ids[i]) + " needs " + std::to_string(bytes) + " bytes, blob_ld_bytes is " + std::to_string(blob_ld));
    items = std::max(items, voice::pack_items(v->cache.H, rows[i].tokens));
  }
  HIP_CHECK(hipSetDevice(v->ctx->device));
  hipStream_t st = (hipStream_t)stream;
  v->sets.init(v->capacity, v->allocs);
  for (int b0 = 0; b0 < n; b0 += v->capacity) {      // (ids may repeat: a call of more rows than entries goes in several launches)
    const int nb = std::min(v->capacity, n - b0);
    const int q = v->sets.begin(reinterpret_cast<const std::array<int, 4>*>(rows.data() + b0), nb, st);
    hipLaunchKernelGGL(cnk::voice_pack_kernel, dim3((unsigned)items, (unsigned)nb), dim3(voice::kLanes), 0, st, v->cache,
                       reinterpret_cast<const voice::MoveRow*>(v->sets.rows[q]), static_cast<char*>(blob_dev) + (long long)b0 * blob_ld, (long long)blob_ld);
    v->sets.end(q, st);
  }
  for (int i = 0; i < n; ++i) {
    Meta m; memset(&m, 0, sizeof(m));
    m.magic = kMagic; m.version = voice::kVersion; m.size = sizeof(Meta);
    m.layout_id = v->layout_id; m.bytes = voice::row_off(v->cache.H, rows[i].tokens).bytes;
    m.frames = v->frames[ids[i]]; m.tokens = rows[i].tokens; m.hidden_size = v->cache.H;
    m.checksum = meta_sum(m);
    memcpy(&meta[i], &m, sizeof(m));
  }
}

void import_voices(conan_voices* v, const int32_t* ids, int n, const void* blob_dev, int64_t blob_ld, const conan_voice_meta* meta, void* stream) {
  if (!v || !ids || !blob_dev || !meta) throw Error(CONAN_ERR_INVALID, "null argument");
  const char* who = "conan_voices_import";
  check_ids(v, ids, n, true, who);
  check_blob(blob_dev, blob_ld, who);
  std::vector<voice::MoveRow> rows((size_t)n);
  std::vector<Meta> ms((size_t)n);
  for (int i = 0; i < n; ++i) {
    const std::string where = std::string(who) + ": record " + std::to_string(i) + ": ";
    Meta& m = ms[i];
    m = read_meta(&meta[i], where, &v->layout_id);
    if (m.tokens < 1 || m.frames < 1 || m.tokens != (m.frames + 3) / 4 || m.bytes != voice::row_off(v->cache.H, m.tokens).bytes) throw Error(CONAN_ERR_INVALID, where + "inconsistent record");
    if (m.frames > v->max_ref || m.tokens > v->cache.S_max)
      throw Error(CONAN_ERR_SHAPE, where + "the voice has " + std::to_string(m.frames) + " reference frames, the bank holds " + std::to_string(v->max_ref));
    if (m.bytes > blob_ld) throw Error(CONAN_ERR_SHAPE, where + "the voice uses " + std::to_string(m.bytes) + " bytes, blob_ld_bytes is " + std::to_string(blob_ld));
    rows[i] = voice::MoveRow{ids[i], m.tokens, {0, 0}};
  }
  HIP_CHECK(hipSetDevice(v->ctx->device));
  hipStream_t st = (hipStream_t)stream;
  v->sets.init(v->capacity, v->allocs);
  const int q = v->sets.begin(reinterpret_cast<const std::array<int, 4>*>(rows.data()), n, st);
  hipLaunchKernelGGL(cnk::voice_unpack_kernel, dim3((unsigned)voice::fill_items(v->cache.S_max, v->cache.H), (unsigned)n), dim3(voice::kLanes), 0, st, v->cache,
                     reinterpret_cast<const voice::MoveRow*>(v->sets.rows[q]), static_cast<const char*>(blob_dev), (long long)blob_ld);
  v->sets.end(q, st);
  for (int i = 0; i < n; ++i) { v->enrolled[ids[i]] = 1; v->frames[ids[i]] = ms[i].frames; v->tokens[ids[i]] = ms[i].tokens; }
}

void meta_info(const conan_voice_meta* meta, conan_voice_info* out) {
  if (!meta || !out) throw Error(CONAN_ERR_INVALID, "null argument");
  const Meta m = read_meta(meta, "conan_voice_meta_info: ");
  memset(out, 0, sizeof(*out));
  out->enrolled = 1; out->ref_frames = m.frames; out->tokens = m.tokens; out->bytes = m.bytes; out->layout_id = m.layout_id;
}

}  // namespace voices
