// Source bypass (include/conan_hip.h, conan_bypass_cfg): the stage kernel and the mix kernel, the whole-signal entry point
// conan_bypass_mix and the host side of conan_streams_set_bypass.  The wav-in steps launch the stage kernel behind their front-end
// launch (and the activity detector's) on the rows of the call's bypass staging (byp::WavStage below); the vocoder step of a chunk with a bypass
// row launches the mix between the activity gate and the output resampler (streams.hip, hifigan_step).
#include <climits>

#include "streams.h"

namespace cnk {

// One row per workgroup.  Thread 0 runs the slew over the row's <= seg frames (a few integer operations per frame) while the whole
// workgroup copies the chunk's samples: four per lane with one 16-byte load and store where hop is a multiple of 4 - a chunk starts
// at a multiple of hop and the ring's length is a power of two >= 4, so such a group neither straddles the wrap nor is misaligned -
// and single words otherwise.  Every load is unconditional at a masked address, which is always inside the slot's ring; the zeros at
// and beyond `valid` are selected after it.
__global__ __launch_bounds__(kBypStageThreads) void bypass_stage_kernel(const BypStageArgs a) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= a.rows) return;
  const BypRow r = a.tab[blockIdx.x];      // uniform in the workgroup
  if (r.mode == 0) return;                 // a row of a slot without the feature (it holds the mix's place in the table)
  const int hop = a.hop;
  if (tid == 0) {
    const long long lo = (long long)blockIdx.x * (a.seg + 1);
    const int* gl = r.fill == 1 ? a.gate_lvl + lo : nullptr;      // (fill = 2: no gate, which counts as open - nothing is filled)
    BypState s = r.seed;
    if (!r.reseed && r.slot >= 0) s = a.state[r.slot];
    else if (r.fill) s.dry_eff = gl ? (int)(((long long)s.dry * (kActFull - gl[0])) >> 20) : 0;
    a.wet_lvl[lo] = s.wet; a.dry_lvl[lo] = s.dry_eff;
    for (int f = 0; f < r.nframes; ++f) {
      const int dw = r.wet_target - s.wet, dd = r.dry_target - s.dry;
      s.wet += dw > r.step ? r.step : (dw < -r.step ? -r.step : dw);
      s.dry += dd > r.step ? r.step : (dd < -r.step ? -r.step : dd);
      s.dry_eff = gl ? (int)(((long long)s.dry * (kActFull - gl[1 + f])) >> 20) : (r.fill ? 0 : s.dry);
      a.wet_lvl[lo + 1 + f] = s.wet; a.dry_lvl[lo + 1 + f] = s.dry_eff;
    }
    if (r.slot >= 0) a.state[r.slot] = s;
    if (r.state_row >= 0) a.state_out[r.state_row] = s;
  }
  const int count = r.nframes * hop;
  if (count < 1) return;
  const float* src = a.src + r.src_off;
  float* dst = a.dry + (long long)blockIdx.x * a.seg * hop;
  if ((hop & 3) == 0) {
    for (int j = tid * 4; j < count; j += kBypStageThreads * 4) {
      const long long sj = r.s_first + j;
      float4 q = *reinterpret_cast<const float4*>(src + (sj & (long long)r.mask));
      q.x = sj < r.valid ? q.x : 0.f; q.y = sj + 1 < r.valid ? q.y : 0.f; q.z = sj + 2 < r.valid ? q.z : 0.f; q.w = sj + 3 < r.valid ? q.w : 0.f;
      *reinterpret_cast<float4*>(dst + j) = q;
    }
  } else {
    for (int j = tid; j < count; j += kBypStageThreads) {
      const long long sj = r.s_first + j;
      const float v = src[sj & (long long)r.mask];
      dst[j] = sj < r.valid ? v : 0.f;
    }
  }
}

// Four consecutive samples per thread, as the gate: one 16-byte load of each input and one 16-byte store where the thread's samples
// are whole and aligned (always, in a vocoder step), single words otherwise.  Both inputs are loaded before either is used, the single
// words at clamped addresses.  The gains are the law's: an integer interpolation of the frame's two levels and one f64 division each,
// then one f32 product and - where the dry level is not zero - one f32 fused multiply-add.
__global__ __launch_bounds__(kBypMixThreads) void bypass_mix_kernel(const BypMixArgs a) {
  const int i = blockIdx.y;
  if (a.tab && a.tab[i].mode == 0) return;      // uniform: the row does not mix and keeps its bits
  const float* y = a.wet + (long long)i * a.wet_ld;
  const float* x = a.dry + (long long)i * a.dry_ld;
  float* o = a.out + (long long)i * a.out_ld;
  const int* lw = a.wet_lvl + (long long)i * a.lvl_ld;
  const int* ld = a.dry_lvl + (long long)i * a.lvl_ld;
  const long long s0 = ((long long)blockIdx.x * kBypMixThreads + threadIdx.x) * 4;
  if (s0 >= a.samples) return;
  const int start_w = a.start_in_lvl ? lw[-1] : a.start_wet, start_d = a.start_in_lvl ? ld[-1] : a.start_dry;
  const int hop = a.hop;
  const double den = (double)((long long)hop << 20);
  const bool vec = s0 + 3 < a.samples &&
                   ((reinterpret_cast<uintptr_t>(y + s0) | reinterpret_cast<uintptr_t>(x + s0) | reinterpret_cast<uintptr_t>(o + s0)) & 15) == 0;
  float vy[4], vx[4];
  if (vec) {
    const float4 qy = *reinterpret_cast<const float4*>(y + s0);
    const float4 qx = *reinterpret_cast<const float4*>(x + s0);
    vy[0] = qy.x; vy[1] = qy.y; vy[2] = qy.z; vy[3] = qy.w;
    vx[0] = qx.x; vx[1] = qx.y; vx[2] = qx.z; vx[3] = qx.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long sc = s0 + e < a.samples ? s0 + e : a.samples - 1;      // (clamped: a sample past the row is loaded again, never stored)
      vy[e] = y[sc]; vx[e] = x[sc];
    }
  }
  float r[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long long sx = s0 + e < a.samples ? s0 + e : a.samples - 1;        // (clamped: the levels of a sample past the row are never read)
    const long long f = sx / hop;
    const int k = (int)(sx - f * hop);
    const int wp = f > 0 ? lw[f - 1] : start_w, wn = lw[f];
    const int dp = f > 0 ? ld[f - 1] : start_d, dn = ld[f];
    const long long l_w = (long long)wp * (hop - 1 - k) + (long long)wn * (k + 1);
    const long long l_d = (long long)dp * (hop - 1 - k) + (long long)dn * (k + 1);
    const float g_w = (float)((double)l_w / den), g_d = (float)((double)l_d / den);
    const float t = __fmul_rn(vy[e], g_w);
    r[e] = l_d == 0 ? t : __fmaf_rn(vx[e], g_d, t);
  }
  if (vec) {
    *reinterpret_cast<float4*>(o + s0) = make_float4(r[0], r[1], r[2], r[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) if (s0 + e < a.samples) o[s0 + e] = r[e];
  }
}

void launch_bypass_stage(const BypStageArgs& a, hipStream_t st) {
  if (a.rows < 1) return;
  hipLaunchKernelGGL(bypass_stage_kernel, dim3(a.rows), dim3(kBypStageThreads), 0, st, a);
}

void launch_bypass_mix(const BypMixArgs& a, hipStream_t st) {
  if (a.n < 1 || a.samples < 1) return;
  const long long per = (long long)kBypMixThreads * 4;
  hipLaunchKernelGGL(bypass_mix_kernel, dim3((unsigned)((a.samples + per - 1) / per), a.n), dim3(kBypMixThreads), 0, st, a);
}

}  // namespace cnk

namespace byp {

static_assert(sizeof(conan_bypass_state) == sizeof(cnk::BypState), "the kernels' state is the header's");
static_assert(sizeof(conan_bypass_cfg) == 32, "eight int32 fields");

void check_cfg(const conan_bypass_cfg& c, const char* who) {
  const std::string w = std::string(who) + ": ";
  auto bad = [&](const char* what) { throw Error(CONAN_ERR_INVALID, w + what); };
  if (c.enabled != 0 && c.enabled != 1) bad("conan_bypass_cfg.enabled must be 0 or 1");
  if (!c.enabled) return;      // (the other fields are ignored)
  if (c.reseed != 0 && c.reseed != 1) bad("conan_bypass_cfg.reseed must be 0 or 1");
  if (c.fill_gate != 0 && c.fill_gate != 1) bad("conan_bypass_cfg.fill_gate must be 0 or 1");
  const int lv[4] = {c.wet_target, c.dry_target, c.seed_wet, c.seed_dry};
  for (int v : lv) if (v < 0 || v > cnk::kActFull) bad("wet_target, dry_target, seed_wet and seed_dry must be in 0 .. 2^20");
  if (c.step < 1 || c.step > cnk::kActFull) bad("step must be in 1 .. 2^20");
}

cnk::BypRow row(const conan_bypass_cfg& c) {
  cnk::BypRow r;
  memset(&r, 0, sizeof(r));
  r.seed.wet = c.seed_wet; r.seed.dry = c.seed_dry; r.seed.dry_eff = c.seed_dry;
  r.wet_target = c.wet_target; r.dry_target = c.dry_target; r.step = c.step; r.fill = c.fill_gate;
  r.mode = 1; r.mask = -1; r.reseed = 1; r.slot = -1; r.state_row = -1;
  return r;
}

void mix(conan_ctx* ctx, int hop, const float* wet_dev, int64_t wet_ld, const float* dry_dev, int64_t dry_ld, int n, int64_t samples, const int32_t* wet_lvl_dev,
         const int32_t* dry_lvl_dev, int64_t lvl_ld, int32_t start_wet, int32_t start_dry, float* out_dev, int64_t out_ld, void* stream) {
  if (!ctx || !wet_dev || !dry_dev || !wet_lvl_dev || !dry_lvl_dev || !out_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  if (hop < 1 || hop > 2047) throw Error(CONAN_ERR_INVALID, "conan_bypass_mix: hop must be in 1 .. 2047");
  if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, "conan_bypass_mix: n must be in 1 .. 65535");
  if (samples < 1 || samples > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_bypass_mix: samples must be in 1 .. 2^31 - 1");
  const int64_t lds[3] = {wet_ld, dry_ld, out_ld};
  for (int64_t ld : lds) if (ld < samples || ld > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_bypass_mix: wet_ld, dry_ld and out_ld must be in samples .. 2^31 - 1");
  if (out_dev == wet_dev && out_ld != wet_ld) throw Error(CONAN_ERR_INVALID, "conan_bypass_mix: in place (out_dev = wet_dev) out_ld must be wet_ld");
  if (lvl_ld < (samples + hop - 1) / hop || lvl_ld > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_bypass_mix: lvl_ld must cover ceil(samples / hop) frames");
  if (start_wet < 0 || start_wet > cnk::kActFull || start_dry < 0 || start_dry > cnk::kActFull)
    throw Error(CONAN_ERR_INVALID, "conan_bypass_mix: start_wet and start_dry must be in 0 .. 2^20");
  HIP_CHECK(hipSetDevice(ctx->device));
  cnk::BypMixArgs a;
  memset(&a, 0, sizeof(a));
  a.wet = wet_dev; a.dry = dry_dev; a.out = out_dev; a.wet_lvl = wet_lvl_dev; a.dry_lvl = dry_lvl_dev; a.tab = nullptr;
  a.wet_ld = wet_ld; a.dry_ld = dry_ld; a.out_ld = out_ld; a.lvl_ld = lvl_ld; a.samples = samples;
  a.n = n; a.hop = hop; a.start_wet = start_wet; a.start_dry = start_dry; a.start_in_lvl = 0;
  cnk::launch_bypass_mix(a, (hipStream_t)stream);
  HIP_CHECK(hipGetLastError());
}

void set_bypass(conan_streams* s, const int32_t* slots, int n, const conan_bypass_cfg* cfg, void* stream) {
  if (!s || !slots || !cfg) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_streams_set_bypass");      // (before the handle is touched, before any GPU use)
  if (!wavio::begin_setter(s, slots, n, cfg->enabled != 0, s->byp.allocated(), "conan_streams_set_bypass", stream)) return;
  s->bypass_init();
  s->byp.store_restarting(slots, n, *cfg);      // the restart travels in the slot's next stage row
}

// rows without frames: a pending slot's row starts from the seed and names no slot, any other reads its state (and writes it back as it is)
void state(conan_streams* s, const int32_t* slots, int n, conan_bypass_state* state_dev, void* stream) {
  if (!s || !slots || !state_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  wavio::check_slot_list(s, slots, n);
  std::vector<cnk::BypRow> rows = s->byp.state_rows<cnk::BypRow>(slots, n, row, "conan_streams_bypass_state", " has no bypass (conan_streams_set_bypass)");
  for (cnk::BypRow& r : rows) r.fill = 0;
  hipStream_t st = s->enter(stream);
  const int q = s->byp.sets.begin(rows.data(), n, st);
  cnk::BypStageArgs a;
  memset(&a, 0, sizeof(a));
  // (no frames: no sample is copied; word 0 of the set's level rows is written, which nothing reads before the set's next call writes it)
  a.src = s->wav_in.fe_audio; a.dry = s->byp.dry[q]; a.wet_lvl = s->byp.wet_lvl[q]; a.dry_lvl = s->byp.dry_lvl[q];
  a.state = s->byp.state; a.state_out = reinterpret_cast<cnk::BypState*>(state_dev); a.tab = s->byp.sets.rows[q]; a.rows = n;
  a.seg = s->ctx->cfg.emf_segment; a.hop = s->ctx->hop;
  cnk::launch_bypass_stage(a, st);
  HIP_CHECK(hipGetLastError());
  s->byp.sets.end(q, st);
}

// the levels the last wav-in call produced, in call order: rows of `seg`, zeros where a row had no bypass or did not emit
void last_call(conan_streams* s, int32_t* wet_lvl_dev, int32_t* dry_lvl_dev, void* stream) {
  if (!s || !wet_lvl_dev || !dry_lvl_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  hipStream_t st = wavio::begin_last_call(s, "conan_step_wav_bypass", stream);
  const int seg = s->ctx->cfg.emf_segment, n = s->wav_in.fe_last_n;
  copy_last_rows(s->byp.last, wet_lvl_dev, n, seg, s->byp.wet_lvl, seg + 1, 1, st);
  copy_last_rows(s->byp.last, dry_lvl_dev, n, seg, s->byp.dry_lvl, seg + 1, 1, st);
}

void WavStage::plan(const conan_streams* s, const WavCall& c) {
  if (s->byp.n_on < 1) return;
  bool any = false;
  for (int i = 0; i < c.n; ++i) {
    const FePlan& p = c.pl[i];
    if (!s->byp.on(c.slots[i]) || p.emit < 1) continue;
    if (p.R - (long long)p.pos * c.hop > s->wav_in.fe_LA)
      throw Error(CONAN_ERR_UNSUPPORTED, c.who + ": slot " + std::to_string(c.slots[i]) + " mixes its source: the chunk's samples have left the audio ring");
    any = true;
  }
  if (!any) return;
  mix.assign(c.groups.size(), 0);
  rows = c.table_rows<cnk::BypRow>([&](int g, int i, int at, cnk::BypRow& r) {
    const int slot = c.slots[i];
    if (!s->byp.on(slot)) return false;
    const FePlan& p = c.pl[i];
    r = row(s->byp.cfg[slot]);
    r.src_off = (long long)slot * s->wav_in.fe_LA; r.valid = p.R; r.mask = s->wav_in.fe_LA - 1; r.s_first = (long long)p.pos * c.hop;
    r.nframes = p.emit; r.slot = slot; r.reseed = s->byp.pending[slot];
    // (the fill reads the gate's levels of this call: the activity table has the same rows in the same order; a slot that
    // is not in activity mode 2 has no gate, which counts as open)
    if (r.fill) r.fill = s->act.on(slot) && s->act.cfg[slot].mode == 2 ? 1 : 2;
    fill = fill || r.fill == 1;
    last.push_back({i, 0, at, p.emit});
    mix[g] = 1;
    return true;
  });
}

// the stage kernel, behind the detector: the slew, and the chunk's source samples out of the audio rings into the set's dry staging
void WavStage::enqueue(conan_streams* s, const WavCall& c, hipStream_t cst, FrontWork& front, std::vector<conan_streams::OutPlan>& ops) {
  if (rows.empty()) return;
  q = s->byp.sets.begin(rows.data(), (int)rows.size(), cst);
  for (LastRow& r : last) r.set = q;
  cnk::BypStageArgs a;
  memset(&a, 0, sizeof(a));
  a.src = s->wav_in.fe_audio; a.dry = s->byp.dry[q]; a.wet_lvl = s->byp.wet_lvl[q]; a.dry_lvl = s->byp.dry_lvl[q];
  a.gate_lvl = fill ? s->act.levels[gate_stage->q] : nullptr; a.state = s->byp.state;
  a.tab = s->byp.sets.rows[q]; a.rows = (int)rows.size(); a.seg = c.seg; a.hop = c.hop;
  front.at[kFrBypass] = [s, a](hipStream_t st) { s->profiled("bypass_stage_kernel", 0.0, st, [&] { cnk::launch_bypass_stage(a, st); }); };
  c.each_group([&](int g, int off) {
    if (!mix[g]) return;
    const size_t lvl = (size_t)off * (c.seg + 1) + 1;
    ops[g].mix = {s->byp.sets.rows[q] + off, s->byp.wet_lvl[q] + lvl, s->byp.dry_lvl[q] + lvl, s->byp.dry[q] + (size_t)off * c.seg * c.hop,
                  c.seg + 1, (long long)c.seg * c.hop};
  });
}

void WavStage::commit(conan_streams* s, hipStream_t, hipStream_t last_st) {
  if (!rows.empty()) s->byp.sets.end(q, last_st);      // (behind the call's last vocoder step: the mix is the last reader of table, levels and samples)
  for (const cnk::BypRow& r : rows) if (r.slot >= 0) s->byp.pending[r.slot] = 0;      // (the rows carried the restarts)
  s->byp.last = std::move(last);
}

}  // namespace byp

void conan_streams::bypass_init() {
  if (byp.state) return;
  const int seg = ctx->cfg.emf_segment;
  byp.state = reinterpret_cast<cnk::BypState*>(alloc((size_t)max_slots * sizeof(cnk::BypState) / sizeof(float)));      // zeroed (counted by state_bytes)
  for (int q = 0; q < kActSets; ++q) {
    byp.wet_lvl[q] = reinterpret_cast<int*>(alloc((size_t)max_slots * (seg + 1)));
    byp.dry_lvl[q] = reinterpret_cast<int*>(alloc((size_t)max_slots * (seg + 1)));
    byp.dry[q] = alloc((size_t)max_slots * seg * ctx->hop);
  }
  byp.sets.init(max_slots, allocs);
  state_bytes += (int64_t)kActSets * max_slots * sizeof(cnk::BypRow);
  byp.assign(max_slots);
}
