// Comfort noise (include/conan_hip.h, conan_comfort_cfg): the tracker's kernel and the fill's, the whole-signal entry points
// conan_comfort_track / conan_comfort_fill and the host side of conan_streams_set_comfort.  The wav-in steps launch the tracker behind
// the activity detector's launch (and the bypass's stage) on the rows of the call's comfort staging (comfort::WavStage below); the
// vocoder step of a chunk with a filled row launches the fill behind the wet/dry mix and in front of the output resampler
// (streams.hip, hifigan_step).
#include <climits>
#include <cmath>

#include "streams.h"
#include "hash_dev.h"

namespace cnk {

// One thread per row: the recursion over a row's frames is sequential and a few integer operations per frame; a wav-in call has at
// most `segment` frames per row.  Nothing here depends on the launch's other rows.
__global__ __launch_bounds__(kCmfTrackThreads) void comfort_track_kernel(const CmfTrackArgs a) {
  const int i = blockIdx.x * kCmfTrackThreads + threadIdx.x;
  if (i >= a.rows) return;
  const CmfRow r = a.tab[i];
  if (r.mode == 0) return;                 // a row of a slot without the feature (it holds the fill's place in the table)
  CmfState s = r.seed_state;
  if (!r.reseed && r.slot >= 0) s = a.state[r.slot];
  if (r.start_lvl) a.lvl[r.lvl_off - 1] = s.level;
  const int fixed = r.level < r.l_min ? r.l_min : (r.level > r.l_max ? r.l_max : r.level);
  for (int f = 0; f < r.nframes; ++f) {
    if (r.mode == 1) {
      s.level = fixed;
    } else if (a.act[r.in_off + f] == 0) {
      const unsigned long long bits = (unsigned long long)__double_as_longlong(a.power[r.in_off + f]);
      const int t = (int)(bits >> 44) - (1023 << 8) + r.offset;
      const int target = t < r.l_min ? r.l_min : (t > r.l_max ? r.l_max : t);
      const int d = target - s.level;
      s.level += d > r.up_step ? r.up_step : (d < -r.down_step ? -r.down_step : d);
      s.idle_frames += 1;
    }
    a.lvl[r.lvl_off + f] = s.level;
  }
  if (r.slot >= 0) a.state[r.slot] = s;
  if (r.state_row >= 0) a.state_out[r.state_row] = s;
}

// the law's white source: the finaliser of splitmix64 on seed + (j + 1) * golden (hash_dev.h), folded to a triangular value
__device__ __forceinline__ int comfort_white(unsigned long long z) {
  z = hash64_mix(z);
  return (int)(z & 0xFFFFu) + (int)((z >> 16) & 0xFFFFu) - 65535;
}

// Eight consecutive samples per thread, as the gate's four: two 16-byte loads and stores where the thread's samples are whole and
// aligned (always, in a vocoder step whose hop is a multiple of 8), single words at clamped addresses otherwise.  A hash is two 64-bit
// multiplies (the third, (j + 1) * golden, is carried along as an addition) and every sample needs as many hashes as its colour has
// taps: eight samples share them, 8 + 2 * colour hashes for 8 samples.  The gate's integers come first: a thread whose samples all
// have lc == 0 hashes nothing and, in place, neither loads nor stores - a wave covers 512 samples, so inside an open stretch that is
// uniform.  Rows without the feature or without a gate return at once (uniform in the workgroup).
__global__ __launch_bounds__(kCmfFillThreads) void comfort_fill_kernel(const CmfFillArgs a) {
  constexpr int PER = kCmfFillPer;
  const int i = blockIdx.y;
  const CmfRow r = a.tab[i];               // uniform in the workgroup
  if (r.mode == 0 || r.fill != 1) return;
  const float* x = a.x + (long long)i * a.ld;
  float* y = a.y + (long long)i * a.ld_y;
  const int* gl = a.gate_lvl + (long long)i * a.lvl_ld;
  const int* cl = a.cmf_lvl + (long long)i * a.lvl_ld;
  const long long s0 = ((long long)blockIdx.x * kCmfFillThreads + threadIdx.x) * PER;
  if (s0 >= a.samples) return;
  const int start = a.start_in_lvl ? gl[-1] : a.start_gate;
  const int hop = a.hop;
  const long long full = (long long)hop << 20;
  const double den = (double)full;
  // the gate's integer and the comfort level of each sample (samples < 2^31: the one division is a 32-bit one)
  long long lc[PER];
  int lev[PER];
  bool any = false;
  {
    unsigned f = (unsigned)s0 / (unsigned)hop;
    int k = (int)((unsigned)s0 - f * (unsigned)hop);
    const unsigned f_last = (unsigned)(a.samples - 1) / (unsigned)hop;
    int lp = f > 0 ? gl[f - 1] : start, ln = gl[f], lv = cl[f];
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      lc[e] = full - ((long long)lp * (hop - 1 - k) + (long long)ln * (k + 1));
      lev[e] = lv;
      any = any || (lc[e] != 0 && s0 + e < a.samples);
      if (++k == hop && f < f_last) { k = 0; ++f; lp = ln; ln = gl[f]; lv = cl[f]; }      // (past the row's last frame nothing is read: those samples are never stored)
      else if (k == hop) k = hop - 1;
    }
  }
  const bool inplace = x == y;
  if (!any && inplace) return;
  const bool vec = s0 + PER - 1 < a.samples && ((reinterpret_cast<uintptr_t>(x + s0) | reinterpret_cast<uintptr_t>(y + s0)) & 15) == 0;
  float v[PER];
  if (vec) {
    const float4 q0 = *reinterpret_cast<const float4*>(x + s0);
    const float4 q1 = *reinterpret_cast<const float4*>(x + s0 + 4);
    v[0] = q0.x; v[1] = q0.y; v[2] = q0.z; v[3] = q0.w; v[4] = q1.x; v[5] = q1.y; v[6] = q1.z; v[7] = q1.w;
  } else {
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const long long sc = s0 + e < a.samples ? s0 + e : a.samples - 1;      // (clamped: a sample past the row is loaded again, never stored)
      v[e] = x[sc];
    }
  }
  float o[PER];
#pragma unroll
  for (int e = 0; e < PER; ++e) o[e] = v[e];
  if (any) {
    // w(j) for j = j0 - 4 .. j0 + PER - 1, of which a colour reads the last PER + 2 * colour
    const int first = 4 - 2 * r.colour;
    unsigned long long z = r.seed + (unsigned long long)(r.pos0 + s0 - 4 + first + 1) * kHashGolden;
    int w[PER + 4];
#pragma unroll
    for (int t = 0; t < PER + 4; ++t) {
      w[t] = 0;
      if (t >= first) { w[t] = comfort_white(z); z += kHashGolden; }      // (uniform in the workgroup)
    }
    const int c1 = r.colour >= 1 ? 2 : 0, c2 = r.colour == 2 ? 3 : (r.colour == 1 ? 1 : 0), c3 = r.colour == 2 ? 2 : 0, c4 = r.colour == 2 ? 1 : 0;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const int nv = w[e + 4] + c1 * w[e + 3] + c2 * w[e + 2] + c3 * w[e + 1] + c4 * w[e];
      const int L = lev[e];
      const float amp = __fmul_rn(ldexpf((float)(512 + (L & 511)), (L >> 9) - 9), r.norm);      // (L >> 9: the floor division by 512)
      const float t = __fmul_rn((float)nv, amp);
      const float gc = (float)((double)lc[e] / den);
      o[e] = lc[e] == 0 ? v[e] : __fmaf_rn(t, gc, v[e]);
    }
  }
  if (vec) {
    *reinterpret_cast<float4*>(y + s0) = make_float4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<float4*>(y + s0 + 4) = make_float4(o[4], o[5], o[6], o[7]);
  } else {
#pragma unroll
    for (int e = 0; e < PER; ++e) if (s0 + e < a.samples) y[s0 + e] = o[e];
  }
}

void launch_comfort_track(const CmfTrackArgs& a, hipStream_t st) {
  if (a.rows < 1) return;
  hipLaunchKernelGGL(comfort_track_kernel, dim3((a.rows + kCmfTrackThreads - 1) / kCmfTrackThreads), dim3(kCmfTrackThreads), 0, st, a);
}

void launch_comfort_fill(const CmfFillArgs& a, hipStream_t st) {
  if (a.n < 1 || a.samples < 1) return;
  const long long per = (long long)kCmfFillThreads * kCmfFillPer;
  hipLaunchKernelGGL(comfort_fill_kernel, dim3((unsigned)((a.samples + per - 1) / per), a.n), dim3(kCmfFillThreads), 0, st, a);
}

}  // namespace cnk

namespace comfort {

static_assert(sizeof(conan_comfort_state) == sizeof(cnk::CmfState), "the kernels' state is the header's");
static_assert(sizeof(conan_comfort_cfg) == 56, "twelve 32-bit fields and the seed");
constexpr int kLevelMin = -16384, kStepMax = 16384;

void check_cfg(const conan_comfort_cfg& c, const char* who) {
  const std::string w = std::string(who) + ": ";
  auto bad = [&](const char* what) { throw Error(CONAN_ERR_INVALID, w + what); };
  if (c.mode < 0 || c.mode > 2) bad("conan_comfort_cfg.mode must be 0, 1 or 2");
  if (!c.mode) return;      // (the other fields are ignored)
  if (c.reseed != 0 && c.reseed != 1) bad("conan_comfort_cfg.reseed must be 0 or 1");
  const int lv[4] = {c.level, c.l_min, c.l_max, c.seed_level};
  for (int v : lv) if (v < kLevelMin || v > 0) bad("level, l_min, l_max and seed_level must be in -16384 .. 0");
  if (c.l_min > c.l_max) bad("l_min must not exceed l_max");
  if (c.offset < -kStepMax || c.offset > kStepMax) bad("offset must be in -16384 .. 16384");
  if (c.up_step < 1 || c.up_step > kStepMax || c.down_step < 1 || c.down_step > kStepMax) bad("up_step and down_step must be in 1 .. 16384");
  if (c.colour < 0 || c.colour > 2) bad("colour must be 0, 1 or 2");
  if (!std::isfinite(c.norm) || !(c.norm > 0.f)) bad("norm must be finite and > 0");
  if (c.reserved != 0) bad("the reserved word must be 0");
}

cnk::CmfRow row(const conan_comfort_cfg& c) {
  cnk::CmfRow r;
  memset(&r, 0, sizeof(r));
  r.seed = c.seed; r.seed_state.level = c.seed_level;
  r.level = c.level; r.offset = c.offset; r.l_min = c.l_min; r.l_max = c.l_max; r.up_step = c.up_step; r.down_step = c.down_step;
  r.colour = c.colour; r.norm = c.norm;
  r.mode = c.mode; r.reseed = 1; r.slot = -1; r.state_row = -1;
  return r;
}

// the rows of a whole-signal launch -> the context's workspace, through its pinned staging (as conan_activity's)
static const cnk::CmfRow* upload(conan_ctx* ctx, const std::vector<cnk::CmfRow>& rows, hipStream_t st) {
  const size_t table = rows.size() * sizeof(cnk::CmfRow);
  cnk::CmfRow* h = static_cast<cnk::CmfRow*>(ctx->loud_stage.take(table));
  memcpy(h, rows.data(), table);
  char* ws = reinterpret_cast<char*>(ctx->workspace((table + sizeof(float) - 1) / sizeof(float), st));
  HIP_CHECK(hipMemcpyAsync(ws, h, table, hipMemcpyHostToDevice, st));
  ctx->loud_stage.sent(st);
  return reinterpret_cast<const cnk::CmfRow*>(ws);
}

void track(conan_ctx* ctx, const conan_comfort_cfg* cfg, const int32_t* act_dev, const double* power_dev, int n, int64_t frames, int64_t ld,
           int32_t* level_out_dev, conan_comfort_state* state_out_dev, void* stream) {
  if (!ctx || !cfg || !act_dev || !level_out_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_comfort_track");
  if (!cfg->mode) throw Error(CONAN_ERR_INVALID, "conan_comfort_track: cfg.mode must be 1 or 2");
  if (cfg->mode == 2 && !power_dev) throw Error(CONAN_ERR_INVALID, "null argument (power_dev in follow mode)");
  if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, "conan_comfort_track: n must be in 1 .. 65535");
  if (frames < 1 || frames > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_comfort_track: frames must be in 1 .. 2^31 - 1");
  if (ld < frames || ld > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_comfort_track: ld must be in frames .. 2^31 - 1");
  HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  std::vector<cnk::CmfRow> rows((size_t)n, row(*cfg));
  for (int i = 0; i < n; ++i) {
    rows[i].in_off = (long long)i * ld; rows[i].lvl_off = rows[i].in_off; rows[i].nframes = (int)frames; rows[i].state_row = state_out_dev ? i : -1;
  }
  cnk::CmfTrackArgs a;
  memset(&a, 0, sizeof(a));
  a.act = act_dev; a.power = power_dev; a.lvl = level_out_dev; a.state_out = reinterpret_cast<cnk::CmfState*>(state_out_dev);
  a.tab = upload(ctx, rows, st); a.rows = n;
  cnk::launch_comfort_track(a, st);
  HIP_CHECK(hipGetLastError());
}

void fill(conan_ctx* ctx, int hop, const conan_comfort_cfg* cfg, const uint64_t* seeds, const float* wav_dev, int64_t ld, int n, int64_t samples, int64_t pos0,
          const int32_t* gate_lvl_dev, const int32_t* comfort_lvl_dev, int64_t lvl_ld, int32_t start_gate_level, int32_t start_comfort_level, float* out_dev,
          int64_t out_ld, void* stream) {
  if (!ctx || !cfg || !wav_dev || !gate_lvl_dev || !comfort_lvl_dev || !out_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_comfort_fill");
  if (!cfg->mode) throw Error(CONAN_ERR_INVALID, "conan_comfort_fill: cfg.mode must be 1 or 2");
  if (hop < 1 || hop > 2047) throw Error(CONAN_ERR_INVALID, "conan_comfort_fill: hop must be in 1 .. 2047");
  if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, "conan_comfort_fill: n must be in 1 .. 65535");
  if (samples < 1 || samples > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_comfort_fill: samples must be in 1 .. 2^31 - 1");
  if (ld < samples || ld > INT_MAX || out_ld < samples || out_ld > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_comfort_fill: ld and out_ld must be in samples .. 2^31 - 1");
  if (out_dev == wav_dev && out_ld != ld) throw Error(CONAN_ERR_INVALID, "conan_comfort_fill: in place (out_dev = wav_dev) out_ld must be ld");
  if (pos0 < 0 || pos0 > (int64_t)1 << 62) throw Error(CONAN_ERR_INVALID, "conan_comfort_fill: pos0 must be in 0 .. 2^62");
  if (lvl_ld < (samples + hop - 1) / hop || lvl_ld > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_comfort_fill: lvl_ld must cover ceil(samples / hop) frames");
  if (start_gate_level < 0 || start_gate_level > cnk::kActFull) throw Error(CONAN_ERR_INVALID, "conan_comfort_fill: start_gate_level must be in 0 .. 2^20");
  if (start_comfort_level < kLevelMin || start_comfort_level > 0) throw Error(CONAN_ERR_INVALID, "conan_comfort_fill: start_comfort_level must be in -16384 .. 0");
  HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  std::vector<cnk::CmfRow> rows((size_t)n, row(*cfg));
  for (int i = 0; i < n; ++i) {
    rows[i].mode = 1; rows[i].fill = 1; rows[i].pos0 = pos0;
    if (seeds) rows[i].seed = seeds[i];
  }
  cnk::CmfFillArgs a;
  memset(&a, 0, sizeof(a));
  a.x = wav_dev; a.y = out_dev; a.gate_lvl = gate_lvl_dev; a.cmf_lvl = comfort_lvl_dev; a.tab = upload(ctx, rows, st);
  a.ld = ld; a.ld_y = out_ld; a.lvl_ld = lvl_ld; a.samples = samples; a.n = n; a.hop = hop; a.start_gate = start_gate_level; a.start_in_lvl = 0;
  cnk::launch_comfort_fill(a, st);
  HIP_CHECK(hipGetLastError());
}

void set_comfort(conan_streams* s, const int32_t* slots, int n, const conan_comfort_cfg* cfg, void* stream) {
  if (!s || !slots || !cfg) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_streams_set_comfort");      // (before the handle is touched, before any GPU use)
  if (!wavio::begin_setter(s, slots, n, cfg->mode != 0, s->cmf.allocated(), "conan_streams_set_comfort", stream)) return;
  s->comfort_init();
  s->cmf.store_restarting(slots, n, *cfg);      // the restart travels in the slot's next tracker row
}

// rows without frames: a pending slot's row starts from the seed and names no slot, any other reads its state (and writes it back as it is)
void state(conan_streams* s, const int32_t* slots, int n, conan_comfort_state* state_dev, void* stream) {
  if (!s || !slots || !state_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  wavio::check_slot_list(s, slots, n);
  const std::vector<cnk::CmfRow> rows = s->cmf.state_rows<cnk::CmfRow>(slots, n, row, "conan_streams_comfort_state", " has no comfort noise (conan_streams_set_comfort)");
  hipStream_t st = s->enter(stream);
  const int q = s->cmf.sets.begin(rows.data(), n, st);
  cnk::CmfTrackArgs a;
  memset(&a, 0, sizeof(a));
  a.lvl = s->cmf.levels[q];      // (no frames, start_lvl = 0: nothing is read or written there)
  a.state = s->cmf.state; a.state_out = reinterpret_cast<cnk::CmfState*>(state_dev); a.tab = s->cmf.sets.rows[q]; a.rows = n;
  cnk::launch_comfort_track(a, st);
  HIP_CHECK(hipGetLastError());
  s->cmf.sets.end(q, st);      // (only the set's table was taken: the staging beside it still holds what its last wav-in call wrote)
}

// the levels the last wav-in call produced, in call order: rows of `seg`, zeros where a row had no comfort noise or did not emit
void last_call(conan_streams* s, int32_t* level_dev, void* stream) {
  if (!s || !level_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  hipStream_t st = wavio::begin_last_call(s, "conan_step_wav_comfort", stream);
  const int seg = s->ctx->cfg.emf_segment, n = s->wav_in.fe_last_n;
  copy_last_rows(s->cmf.last, level_dev, n, seg, s->cmf.levels, seg + 1, 1, st);
}

void WavStage::plan(const conan_streams* s, const WavCall& c) {
  if (s->cmf.n_on < 1 || gate_stage->rows.empty()) return;      // (no detector row in the call: no frames here)
  bool any = false;
  for (int i = 0; i < c.n; ++i) any = any || (s->cmf.on(c.slots[i]) && s->act.on(c.slots[i]) && c.pl[i].emit > 0);
  if (!any) return;
  fill.assign(c.groups.size(), 0);
  rows = c.table_rows<cnk::CmfRow>([&](int g, int i, int at, cnk::CmfRow& r) {
    const int slot = c.slots[i];
    if (!s->cmf.on(slot) || !s->act.on(slot)) return false;
    const FePlan& p = c.pl[i];
    r = row(s->cmf.cfg[slot]);
    // (the detector's table has the same rows in the same order: its flags and powers of chunk row `at` are this row's)
    r.pos0 = (long long)p.pos * c.hop; r.in_off = (long long)at * c.seg; r.lvl_off = (long long)at * (c.seg + 1) + 1;
    r.nframes = p.emit; r.slot = slot; r.reseed = s->cmf.pending[slot]; r.start_lvl = 1;
    r.fill = s->act.cfg[slot].mode == 2 ? 1 : 0;      // (a slot that is not gated counts as open: it tracks and is never filled)
    follows = follows || r.mode == 2;
    last.push_back({i, 0, at, p.emit});
    if (r.fill) fill[g] = 1;
    return true;
  });
}

double* WavStage::take(conan_streams* s, hipStream_t cst) {
  if (rows.empty()) return nullptr;
  q = s->cmf.sets.begin(rows.data(), (int)rows.size(), cst);
  for (LastRow& r : last) r.set = q;
  return follows ? s->cmf.powers[q] : nullptr;
}

// the tracker, behind the detector (and the bypass's stage): the call's flags and powers are in the activity set and in this one
void WavStage::enqueue(conan_streams* s, const WavCall& c, hipStream_t, FrontWork& front, std::vector<conan_streams::OutPlan>& ops) {
  if (rows.empty()) return;
  cnk::CmfTrackArgs a;
  memset(&a, 0, sizeof(a));
  a.act = s->act.flags[gate_stage->q]; a.power = follows ? s->cmf.powers[q] : nullptr; a.lvl = s->cmf.levels[q]; a.state = s->cmf.state;
  a.tab = s->cmf.sets.rows[q]; a.rows = (int)rows.size();
  front.at[kFrComfort] = [s, a](hipStream_t st) { s->profiled("comfort_track_kernel", 0.0, st, [&] { cnk::launch_comfort_track(a, st); }); };
  c.each_group([&](int g, int off) {
    if (!fill[g]) return;
    const size_t lvl = (size_t)off * (c.seg + 1) + 1;
    ops[g].fill = {s->cmf.sets.rows[q] + off, s->cmf.levels[q] + lvl, s->act.levels[gate_stage->q] + lvl, c.seg + 1};
  });
}

void WavStage::commit(conan_streams* s, hipStream_t, hipStream_t last_st) {
  if (!rows.empty()) s->cmf.sets.end(q, last_st);      // (behind the call's last vocoder step: the fill is the last reader of table and levels)
  for (const cnk::CmfRow& r : rows) if (r.slot >= 0) s->cmf.pending[r.slot] = 0;      // (the rows carried the restarts)
  s->cmf.last = std::move(last);
}

}  // namespace comfort

void conan_streams::comfort_init() {
  if (cmf.state) return;
  const int seg = ctx->cfg.emf_segment;
  cmf.state = reinterpret_cast<cnk::CmfState*>(alloc((size_t)max_slots * sizeof(cnk::CmfState) / sizeof(float)));      // zeroed (counted by state_bytes)
  for (int q = 0; q < kActSets; ++q) {
    cmf.levels[q] = reinterpret_cast<int*>(alloc((size_t)max_slots * (seg + 1)));
    cmf.powers[q] = reinterpret_cast<double*>(alloc((size_t)max_slots * seg * 2));
  }
  cmf.sets.init(max_slots, allocs);
  state_bytes += (int64_t)kActSets * max_slots * sizeof(cnk::CmfRow);
  cmf.assign(max_slots);
}
