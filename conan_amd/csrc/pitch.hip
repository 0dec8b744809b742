// Per-slot pitch control of the decoder step (include/conan_hip.h, conan_pitch_cfg): the host side.  The law itself is four lines of
// rowops.h (pitch_ctl / pitch_law) inside the two forms of the uv / f0 head; here: the cfg check, the setter and the table writer.
#include <cmath>

#include "streams.h"

namespace pitch {

void check_cfg(const conan_pitch_cfg& c, const char* who) {
  const std::string w = std::string(who) + ": ";
  if (c.enabled != 0 && c.enabled != 1) throw Error(CONAN_ERR_INVALID, w + "conan_pitch_cfg.enabled must be 0 or 1");
  if (!c.enabled) return;      // (the other fields are ignored)
  if (c.reserved != 0) throw Error(CONAN_ERR_INVALID, w + "conan_pitch_cfg.reserved must be 0");
  if (!std::isfinite(c.shift_semitones) || std::fabs(c.shift_semitones) > 48.f) throw Error(CONAN_ERR_INVALID, w + "shift_semitones must be finite and within +-48");
  if (!std::isfinite(c.range) || c.range < 0.f || c.range > 4.f) throw Error(CONAN_ERR_INVALID, w + "range must be in 0 .. 4");
  if (!std::isfinite(c.pivot)) throw Error(CONAN_ERR_INVALID, w + "pivot must be finite (log2 Hz)");
  if (std::isnan(c.uv_threshold)) throw Error(CONAN_ERR_INVALID, w + "uv_threshold must not be NaN (+-inf are allowed)");
}

void set_pitch(conan_streams* s, const int32_t* slots, int n, const conan_pitch_cfg* cfg, void* stream) {
  if (!s || !slots || !cfg) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_streams_set_pitch");      // (before any GPU use)
  if (!(s->ctx->cfg.models & CONAN_MODEL_CONAN)) throw Error(CONAN_ERR_STATE, "context holds no Conan model");
  wavio::check_slot_list(s, slots, n);
  HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
  hipStream_t st = (hipStream_t)stream;
  s->join(st);
  const std::vector<conan_pitch_cfg> cfgs((size_t)n, *cfg);
  s->pitch_write(slots, n, cfgs.data(), st);
}

void get_pitch(const conan_streams* s, int slot, conan_pitch_cfg* out) {
  if (!s || !out) throw Error(CONAN_ERR_INVALID, "null argument");
  if (slot < 0 || slot >= s->max_slots) throw Error(CONAN_ERR_INVALID, "slot index out of range");
  if (s->pt_cfg.empty()) throw Error(CONAN_ERR_STATE, "context holds no Conan model");
  *out = s->pt_cfg[slot];
}

}  // namespace pitch

// cfgs[i] (checked) becomes slot slots[i]'s (checked, distinct): the host copy at once, the device table in the order of `st` - one
// upload of the call's rows and one launch that scatters them, so steps already enqueued on `st` still read the old entries.
void conan_streams::pitch_write(const int32_t* slots, int n, const conan_pitch_cfg* cfgs, hipStream_t st) {
  if (!d_ptab || n <= 0) return;
  static_assert(sizeof(cnk::PitchRow) == 8 * sizeof(int), "rows are uploaded as ints");
  if (!pt_stage) {
    pt_stage = static_cast<cnk::PitchRow*>(stage_alloc((size_t)max_slots * sizeof(cnk::PitchRow)));
    pt_pin.init((size_t)max_slots * 8);
  }
  std::vector<cnk::PitchRow> rows((size_t)n);
  for (int i = 0; i < n; ++i) {
    conan_pitch_cfg c = cfgs[i];
    if (!c.enabled) memset(&c, 0, sizeof(c));
    cnk::PitchRow& r = rows[i];
    memset(&r, 0, sizeof(r));
    r.slot = slots[i];
    r.v.follow = follow.on(slots[i]) ? 1 : 0;      // (conan_streams_set_pitch_follow: the entry's sixth word, whatever the cfg)
    if (c.enabled) {
      r.v.enabled = 1; r.v.shift_oct = (float)((double)c.shift_semitones / 12.0); r.v.range = c.range; r.v.pivot = c.pivot; r.v.thr = c.uv_threshold;
    }
    pt_cfg[slots[i]] = c;
  }
  pt_pin.upload(reinterpret_cast<int*>(pt_stage), reinterpret_cast<const int*>(rows.data()), (size_t)n * 8, st);
  cnk::launch_pitch_table(d_ptab, pt_stage, n, st);
}
