// Slot snapshots: export a stream's per-slot state to a position-independent blob row and import it into another slot, stream-set,
// process or device (include/conan_hip.h).  One launch each way; the layout and the cell mover are snapshot_layout.h's.
#include <climits>

#include "streams.h"

namespace cnk {

// Work item w of slot row y: cells [w * kItemBytes / 16, ...) of the row, 256 lanes x 16 bytes per pass.  Plain vector loads and
// stores; no atomics, no waits.  Every cell of the used part belongs to exactly one region (regions are padded to cells), so no two
// lanes touch the same bytes on either side.
template <bool PACK>
__global__ __launch_bounds__(256) void slot_move_kernel(const snap::Region* __restrict__ regs, const int* __restrict__ item_first,
                                                        const snap::CallRow* __restrict__ rows, char* blob, long long blob_ld) {
  const snap::CallRow row = rows[blockIdx.y];
  const long long base = (long long)blockIdx.x * snap::kItemBytes;
  if (base >= row.used_bytes) return;
  const int first = item_first[blockIdx.x];
  char* blob_row = blob + (long long)blockIdx.y * blob_ld;
#pragma unroll
  for (int p = 0; p < snap::kItemBytes / (256 * snap::kCell); ++p) {
    const long long off = base + ((long long)p * 256 + threadIdx.x) * snap::kCell;
    if (off < row.used_bytes) snap::move_cell<PACK>(regs, first, row, blob_row, off);
  }
}

}  // namespace cnk

namespace {

constexpr uint32_t kMagic = 0x4e534e43u;      // "CNSN"
constexpr uint32_t kVersion = 1;

// the host half of a snapshot (conan_slot_meta.opaque)
struct Meta {
  uint32_t magic, version, size, present;
  uint64_t layout_id; int64_t bytes;
  int32_t has_ref, voc_fresh, in_fmt, out_fmt;
  int64_t voc_samples;
  int64_t fe_recv; int32_t fe_frames, fe_chunks, fe_phase, rs_phase;
  int64_t rs_in, rs_out, or_out;
  int32_t or_flushed, has_rs;
  conan_resample_cfg in_cfg, out_cfg;
  uint64_t checksum;                 // FNV-1a over the record with this field zero
  conan_level_cfg lv;                // the input leveller (all zero: none - every record written before it existed)
  conan_pitch_cfg pt;                // the pitch control (all zero: none - every record written before it existed); it fills what was padding
};
static_assert(sizeof(conan_pitch_cfg) == 24 && CONAN_SLOT_META_BYTES - 184 - sizeof(conan_level_cfg) == sizeof(conan_pitch_cfg), "the pitch cfg takes the record's last 24 bytes");
static_assert(sizeof(Meta) == CONAN_SLOT_META_BYTES && sizeof(conan_slot_meta) == CONAN_SLOT_META_BYTES, "the meta record is 256 bytes");

uint64_t meta_sum(Meta m) { m.checksum = 0; return snap::fnv1a(snap::kFnvSeed, &m, sizeof(m)); }

Meta read_meta(const conan_slot_meta* rec, const std::string& where) {
  Meta m; memcpy(&m, rec, sizeof(m));
  if (m.magic != kMagic) throw Error(CONAN_ERR_INVALID, where + "not a slot snapshot record");
  if (m.version != kVersion || m.size != sizeof(Meta)) throw Error(CONAN_ERR_INVALID, where + "snapshot record of version " + std::to_string(m.version) + " / " + std::to_string(m.size) + " bytes, this library reads version " + std::to_string(kVersion) + " / " + std::to_string(sizeof(Meta)));
  if (m.checksum != meta_sum(m)) throw Error(CONAN_ERR_INVALID, where + "snapshot record is corrupted (checksum)");
  return m;
}

std::string hex(uint64_t v) { char b[32]; snprintf(b, sizeof(b), "%016llx", (unsigned long long)v); return b; }

bool has_rate(const conan_resample_cfg& c) { return c.in_rate != c.out_rate; }

void upload_tables(conan_streams* s) {
  conan_streams::Snap& sn = s->snapshot;
  const snap::Layout& l = sn.layout;
  if (!sn.d_regions) {
    sn.d_regions = (snap::Region*)s->stage_alloc(l.regions.size() * sizeof(snap::Region));
    sn.d_item_first = (int*)s->stage_alloc(l.item_first.size() * sizeof(int));
    sn.sets.init(s->max_slots, s->allocs);
  }
  if (sn.built) return;
  // (blocking copies: once per stream-set, and once more when a rate ring is first allocated)
  HIP_CHECK(hipMemcpy(sn.d_regions, l.regions.data(), l.regions.size() * sizeof(snap::Region), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(sn.d_item_first, l.item_first.data(), l.item_first.size() * sizeof(int), hipMemcpyHostToDevice));
  sn.built = true;
}

template <bool PACK>
void launch(conan_streams* s, const std::vector<snap::CallRow>& rows, char* blob, long long blob_ld, hipStream_t st) {
  conan_streams::Snap& sn = s->snapshot;
  s->snapshot_build();
  upload_tables(s);
  long long used = 0;
  for (const snap::CallRow& r : rows) used = std::max<long long>(used, r.used_bytes);
  static_assert(sizeof(snap::CallRow) == sizeof(std::array<int, 4>), "call rows are uploaded as 4 ints");
  const int q = sn.sets.begin(reinterpret_cast<const std::array<int, 4>*>(rows.data()), (int)rows.size(), st);
  const dim3 grid((unsigned)sn.layout.items(used), (unsigned)rows.size());
  hipLaunchKernelGGL(cnk::slot_move_kernel<PACK>, grid, dim3(256), 0, st, sn.d_regions, sn.d_item_first,
                     reinterpret_cast<const snap::CallRow*>(sn.sets.rows[q]), blob, blob_ld);
  sn.sets.end(q, st);
}

int present_of(const conan_streams* s, int slot) {
  int p = 1 << snap::SEC_CORE;
  if (s->wav_in.fe_audio) {
    const conan_streams::FeSlot& f = s->wav_in.fe_slot[slot];
    if (f.recv || f.frames || f.chunks || f.phase) p |= 1 << snap::SEC_FE;
  }
  if (!s->wav_in.rs_slot.empty() && s->wav_in.rs_slot[slot].f) p |= (1 << snap::SEC_RS_IN) | (1 << snap::SEC_FE);
  if (!s->wav_out.or_slot.empty() && s->wav_out.or_slot[slot].f) p |= 1 << snap::SEC_RS_OUT;
  if (s->in_lv.on(slot)) p |= 1 << snap::SEC_LEVEL;
  return p;
}

using snap::used_bytes;

void check_blob(const void* blob, int64_t ld, const char* who) {
  if (reinterpret_cast<uintptr_t>(blob) % snap::kCell || ld % snap::kCell || ld < 0)
    throw Error(CONAN_ERR_INVALID, std::string(who) + ": blob_dev and blob_ld_bytes must be multiples of 16");
}

}  // namespace

// The layout of a slot's row.  Host only: addresses of what is allocated now; the rate rings' sections are part of the layout (and of
// its id) whether or not this stream-set has allocated them yet.
void conan_streams::snapshot_build() {
  Snap& sn = snapshot;
  if (sn.lay_ok && sn.lay_rs == wav_in.rs_ring && sn.lay_or == wav_out.or_ring && sn.lay_lv == in_lv.state) return;
  snap::Layout l;
  const conan_cfg& c = ctx->cfg;
  int* pos_arr[3] = {pos_emf, pos_dec, pos_voc};
  int pos_cell[3];
  for (int k = 0; k < 3; ++k) pos_cell[k] = (int)l.regions[snap::add_whole(l, pos_arr[k], 4, 4, snap::SEC_CORE)].blob_off;
  for (const auto& pr : sn.rings) {
    const Ring& r = pr.first;
    snap::add_ring(l, r.base, r.slot_stride * 4, r.C, r.L, r.rate, r.hist, pos_arr[pr.second], pos_cell[pr.second], snap::SEC_CORE);
  }
  for (const auto& b : emf_state) snap::add_whole(l, b.first, b.second * 4, (int)(b.second * 4), snap::SEC_CORE);      // K / V rings, memory banks
  if (c.models & CONAN_MODEL_CONAN) {
    const int H = c.hidden_size;
    snap::add_whole(l, c_style, (long long)H * 4, H * 4, snap::SEC_CORE);
    snap::add_whole(l, c_kv, (long long)2 * S_max * 2 * H * 4, 2 * S_max * 2 * H * 4, snap::SEC_CORE);
    snap::add_whole(l, c_kmask, (long long)S_max * 4, S_max * 4, snap::SEC_CORE);
    snap::add_whole(l, c_slen, 4, 4, snap::SEC_CORE);
    snap::add_whole(l, c_vqids, (long long)S_max * 4, S_max * 4, snap::SEC_CORE);
  }
  if (wav_in.fe_audio) {
    const int mel_bytes = wav_in.fe_LM * c.emf_input_dim * 4;
    snap::add_whole(l, wav_in.fe_audio, (long long)wav_in.fe_LA * 4, wav_in.fe_LA * 4, snap::SEC_FE, true);
    snap::add_whole(l, wav_in.fe_mel, mel_bytes, mel_bytes, snap::SEC_FE, true);
    snap::add_whole(l, wav_in.rs_ring, (long long)cnk::kRsRing * 4, cnk::kRsRing * 4, snap::SEC_RS_IN);
  }
  if (c.models & CONAN_MODEL_HIFIGAN) {
    // model-rate audio at sample i & (ring length - 1); the position is the host's voc_samples (the call row's aux position)
    const int ring_len = wav_out.or_ring ? wav_out.or_ring_len : ch::next_pow2(CONAN_RESAMPLE_MAX_TAPS + 8 + max_frames * ctx->hop);
    snap::add_ring(l, wav_out.or_ring, (long long)ring_len * 4, 1, ring_len, 1, CONAN_RESAMPLE_MAX_TAPS + 8, nullptr, -1, snap::SEC_RS_OUT);
  }
  if (wav_in.fe_audio) {      // the leveller's block (not part of the id: snapshot_layout.h)
    const long long lv_bytes = (long long)cnk::lv_state_bytes(CONAN_LEVEL_MAX_BLOCKS + cnk::kLvRingPad);
    snap::add_whole(l, in_lv.state, lv_bytes, (int)lv_bytes, snap::SEC_LEVEL);
  }
  for (int sec = 1; sec < snap::SEC_COUNT; ++sec) if (l.sec_end[sec] == 0) l.sec_end[sec] = l.sec_end[sec - 1];
  const int32_t words[] = {(int32_t)kVersion, c.models, c.hidden_size, c.num_mels, c.emf_input_dim, c.emf_layers, c.emf_segment, c.emf_left_context,
                           c.emf_right_context, c.emf_max_memory_size, c.voc_upsample, c.voc_resblock, ctx->hop, rb_limb ? 2 : 1, S_max};
  snap::finish(l, words, (int)(sizeof(words) / sizeof(words[0])));
  sn.layout = std::move(l);
  sn.lay_ok = true; sn.lay_rs = wav_in.rs_ring; sn.lay_or = wav_out.or_ring; sn.lay_lv = in_lv.state;
  sn.built = false;      // (the device tables follow on the next export / import)
}

namespace snapshot {

uint64_t layout_id(conan_streams* s) { s->snapshot_build(); return s->snapshot.layout.id; }
int64_t row_bytes(conan_streams* s) { s->snapshot_build(); return s->snapshot.layout.bytes; }

void export_slots(conan_streams* s, const int32_t* slots, int n, void* blob_dev, int64_t blob_ld, conan_slot_meta* meta, void* stream) {
  if (!s || !slots || !blob_dev || !meta) throw Error(CONAN_ERR_INVALID, "null argument");
  wavio::check_slot_list(s, slots, n);
  check_blob(blob_dev, blob_ld, "conan_streams_export_slots");
  for (int i = 0; i < n; ++i)      // (a drift slot's position is not part of the record)
    if ((!s->wav_in.rs_slot.empty() && s->wav_in.rs_slot[slots[i]].dr.d) || (!s->wav_out.or_slot.empty() && s->wav_out.or_slot[slots[i]].dr.d))
      throw Error(CONAN_ERR_UNSUPPORTED, "conan_streams_export_slots: slot " + std::to_string(slots[i]) + " has a drift resampler (conan_streams_set_input_drift / _set_output_drift): not in slot snapshots");
  s->snapshot_build();
  const snap::Layout& l = s->snapshot.layout;
  std::vector<snap::CallRow> rows(n);
  for (int i = 0; i < n; ++i) {
    const int present = present_of(s, slots[i]);
    const long long used = used_bytes(l, present);
    if (used > blob_ld) throw Error(CONAN_ERR_INVALID, "conan_streams_export_slots: slot " + std::to_string(slots[i]) + " needs " + std::to_string(used) + " bytes, blob_ld_bytes is " + std::to_string(blob_ld));
    rows[i] = snap::CallRow{slots[i], present, (int)used, (int)(s->wav_out.voc_samples[slots[i]] & 0x3fffffff)};
  }
  HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
  hipStream_t st = (hipStream_t)stream;
  s->join(st);
  launch<true>(s, rows, static_cast<char*>(blob_dev), blob_ld, st);
  const int model_rate = 50 * s->ctx->hop;
  const conan_resample_cfg none = {model_rate, model_rate, 6, 0.99f, CONAN_RESAMPLE_HANN, 0.f, {0, 0}};
  for (int i = 0; i < n; ++i) {
    const int slot = slots[i];
    Meta m; memset(&m, 0, sizeof(m));
    m.magic = kMagic; m.version = kVersion; m.size = sizeof(Meta); m.present = (uint32_t)rows[i].present;
    m.layout_id = l.id; m.bytes = rows[i].used_bytes;
    m.has_ref = s->has_ref[slot]; m.voc_fresh = s->voc_fresh[slot]; m.in_fmt = s->wav_in.in_fmt[slot]; m.out_fmt = s->wav_out.out_fmt[slot];
    m.voc_samples = s->wav_out.voc_samples[slot];
    const conan_streams::FeSlot& f = s->wav_in.fe_slot[slot];
    m.fe_recv = f.recv; m.fe_frames = f.frames; m.fe_chunks = f.chunks; m.fe_phase = f.phase;
    m.in_cfg = none; m.out_cfg = none;
    if (!s->wav_in.rs_slot.empty()) {
      const conan_streams::RsSlot& r = s->wav_in.rs_slot[slot];
      m.has_rs = 1; m.rs_in = r.in; m.rs_out = r.out; m.rs_phase = r.phase;
      if (r.f) m.in_cfg = s->snapshot.in_cfg[slot];
    }
    if (!s->wav_out.or_slot.empty()) {
      const conan_streams::OrSlot& o = s->wav_out.or_slot[slot];
      m.or_out = o.out; m.or_flushed = o.flushed;
      if (o.f) m.out_cfg = s->snapshot.out_cfg[slot];
    }
    if (s->in_lv.on(slot)) m.lv = s->in_lv.cfg[slot];
    if (!s->pt_cfg.empty() && s->pt_cfg[slot].enabled) m.pt = s->pt_cfg[slot];
    m.checksum = meta_sum(m);
    memcpy(&meta[i], &m, sizeof(m));
  }
}

void import_slots(conan_streams* s, const int32_t* slots, int n, const void* blob_dev, int64_t blob_ld, const conan_slot_meta* meta, void* stream) {
  if (!s || !slots || !blob_dev || !meta) throw Error(CONAN_ERR_INVALID, "null argument");
  const char* who = "conan_streams_import_slots";
  wavio::check_slot_list(s, slots, n);
  check_blob(blob_dev, blob_ld, who);
  s->snapshot_build();
  const uint64_t id = s->snapshot.layout.id;
  std::vector<Meta> ms(n);
  std::vector<const ch::RsTable*> tin(n, nullptr), tout(n, nullptr);
  bool need_rs_stage = false, need_rs = false, need_or = false, need_lv = false;
  cnk::LvFilter lvf;
  for (int i = 0; i < n; ++i) {
    const std::string where = std::string(who) + ": record " + std::to_string(i) + ": ";
    Meta& m = ms[i];
    m = read_meta(&meta[i], where);
    if (m.layout_id != id)
      throw Error(CONAN_ERR_INVALID, where + "layout id " + hex(m.layout_id) + " of the snapshot differs from this stream-set's " + hex(id) +
                                         " (another configuration, arith, max_ref_frames, or a max_slots across a plan threshold)");
    const int present = (int)m.present;
    if (!(present & 1) || (present >> snap::SEC_COUNT) || m.bytes != used_bytes(s->snapshot.layout, present)) throw Error(CONAN_ERR_INVALID, where + "inconsistent sections");
    if (m.bytes > blob_ld) throw Error(CONAN_ERR_INVALID, where + "the snapshot uses " + std::to_string(m.bytes) + " bytes, blob_ld_bytes is " + std::to_string(blob_ld));
    wavio::check_format(m.in_fmt, who); wavio::check_format(m.out_fmt, who);
    if (has_rate(m.in_cfg)) { tin[i] = wavio::rate_table(s, m.in_cfg, who); need_rs = true; }
    if (has_rate(m.out_cfg)) { tout[i] = wavio::rate_table(s, m.out_cfg, who); need_or = true; }
    if (((present >> snap::SEC_RS_IN) & 1) != (tin[i] != nullptr) || ((present >> snap::SEC_RS_OUT) & 1) != (tout[i] != nullptr)) throw Error(CONAN_ERR_INVALID, where + "inconsistent sections");
    need_rs_stage = need_rs_stage || m.in_fmt != CONAN_SAMPLE_F32 || m.has_rs;
    level::check_cfg(m.lv, who);
    pitch::check_cfg(m.pt, who);
    if (m.pt.enabled && s->pt_cfg.empty()) throw Error(CONAN_ERR_STATE, where + "the stream carries a pitch control and this stream-set has no Conan model");
    if (((present >> snap::SEC_LEVEL) & 1) != (m.lv.enabled != 0)) throw Error(CONAN_ERR_INVALID, where + "inconsistent sections");
    if (m.lv.enabled) {
      if (!s->wav_in.fe_audio) throw Error(CONAN_ERR_STATE, where + "the stream carries an input leveller and this stream-set has no streaming front-end");
      lvf = level::filter(s->ctx, who); need_lv = true;
    }
  }
  HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
  hipStream_t st = (hipStream_t)stream;
  s->join(st);
  // the rate rings, exactly as the setters allocate them
  if (need_rs) s->resample_init(); else if (need_rs_stage && s->wav_in.fe_audio) s->rs_stage_init();
  if (need_or) s->out_ring_init();
  if (need_lv) s->level_init(lvf);      // (the leveller's state, exactly as conan_streams_set_input_level allocates it)
  s->snapshot_build();
  std::vector<snap::CallRow> rows(n);
  std::vector<int32_t> fresh_nn;
  for (int i = 0; i < n; ++i) {
    // (a stream that never took audio: the walk still covers the front-end's section, which clears the destination's rings as a reset would)
    const long long walk = std::max<long long>(ms[i].bytes, s->wav_in.fe_audio ? s->snapshot.layout.sec_end[snap::SEC_FE] : 0);
    rows[i] = snap::CallRow{slots[i], (int)ms[i].present, (int)walk, (int)(ms[i].voc_samples & 0x3fffffff)};
    if (s->ctx->cfg.voc_upsample == 2 && ms[i].voc_fresh) fresh_nn.push_back(slots[i]);
  }
  if (!fresh_nn.empty()) {      // upsample 'nn' relies on untouched ring rows being zero: the reset's own zeroing of the vocoder section
    s->set_slots(fresh_nn.data(), (int)fresh_nn.size(), st);
    for (auto& b : s->voc_state) cnk::launch_zero_slots(b.first, b.second, b.second, s->d_slots, (int)fresh_nn.size(), st);
  }
  launch<false>(s, rows, const_cast<char*>(static_cast<const char*>(blob_dev)), blob_ld, st);
  {      // the destination slots' pitch-control entries (a record without one turns the slot's off)
    std::vector<conan_pitch_cfg> pts((size_t)n);
    for (int i = 0; i < n; ++i) pts[i] = ms[i].pt;
    s->pitch_write(slots, n, pts.data(), st);
  }
  for (int i = 0; i < n; ++i) {
    const int slot = slots[i];
    const Meta& m = ms[i];
    s->has_ref[slot] = (char)m.has_ref; s->voice_of[slot] = -1; s->voc_fresh[slot] = (char)m.voc_fresh; s->wav_out.voc_samples[slot] = m.voc_samples;
    wavio::store_format(s->wav_in.in_fmt, s->wav_in.in_fmt_n, &slot, 1, m.in_fmt);
    wavio::store_format(s->wav_out.out_fmt, s->wav_out.out_fmt_n, &slot, 1, m.out_fmt);
    conan_streams::FeSlot f; f.recv = m.fe_recv; f.frames = m.fe_frames; f.chunks = m.fe_chunks; f.phase = m.fe_phase;
    s->wav_in.fe_slot[slot] = f;
    if (!s->wav_in.rs_slot.empty()) {
      s->wav_in.rs_slot[slot] = conan_streams::RsSlot{tin[i], m.rs_in, m.rs_out, m.rs_phase};
      s->snapshot.in_cfg.resize(s->max_slots, conan_resample_cfg{});
      s->snapshot.in_cfg[slot] = m.in_cfg;
    }
    if (s->in_lv.allocated()) s->in_lv.store(&slot, 1, m.lv);      // (a record without a leveller turns the slot's off)
    if (!s->wav_out.or_slot.empty()) {
      s->wav_out.or_slot[slot] = conan_streams::OrSlot{tout[i], m.or_out, m.or_flushed};
      s->snapshot.out_cfg.resize(s->max_slots, conan_resample_cfg{});
      s->snapshot.out_cfg[slot] = m.out_cfg;
    }
  }
}

void meta_info(const conan_slot_meta* meta, conan_slot_info* out) {
  if (!meta || !out) throw Error(CONAN_ERR_INVALID, "null argument");
  const Meta m = read_meta(meta, "conan_slot_meta_info: ");
  memset(out, 0, sizeof(*out));
  out->layout_id = m.layout_id; out->bytes = m.bytes; out->has_ref = m.has_ref; out->in_format = m.in_fmt; out->out_format = m.out_fmt;
  out->in_rate = m.in_cfg; out->out_rate = m.out_cfg;
}

int meta_level(const conan_slot_meta* meta, conan_level_cfg* out) {
  if (!meta || !out) throw Error(CONAN_ERR_INVALID, "null argument");
  const Meta m = read_meta(meta, "conan_slot_meta_level: ");
  *out = m.lv;
  return m.lv.enabled != 0;
}

int meta_pitch(const conan_slot_meta* meta, conan_pitch_cfg* out) {
  if (!meta || !out) throw Error(CONAN_ERR_INVALID, "null argument");
  const Meta m = read_meta(meta, "conan_slot_meta_pitch: ");
  *out = m.pt;
  return m.pt.enabled != 0;
}

}  // namespace snapshot
