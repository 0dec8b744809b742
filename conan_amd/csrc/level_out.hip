// Output leveller (include/conan_hip.h, conan_streams_set_output_level): conan_level_cfg's law on a slot's own vocoder audio, between
// conv_post and the activity gate.  The law's gains G_{k-1}, G_k of the interval [u_k, u_k + U) depend only on samples before u_k, and
// a levelled row of a vocoder step is such an interval (or its beginning), so the work is split: level_out_apply_kernel, on the
// step's critical path, only reads two gains and writes the ramp; level_out_meter_kernel, behind the step's last launch, runs the
// meter (level_dev.h's lv_meter, the input leveller's and conan_level's) over the samples the apply staged and leaves the gains of
// the next interval.  hifigan_step (streams.hip) launches both; out_plan (wavio.hip) builds and checks the rows before anything changes.
#include <climits>

#include "streams.h"
#include "level_dev.h"

namespace cnk {

// Grid (ceil(samples / 1024), rows); four consecutive samples per lane, one 16-byte load and two 16-byte stores where the lane's
// samples are whole and aligned, single words at clamped addresses otherwise (a sample past the row is loaded again, never stored).
// The gains are loaded from the slot's state whether the row is fresh or not - the state is always there - and the fresh row's
// initial gain is selected behind the load.  No LDS, no scratch, no atomics.
__global__ __launch_bounds__(kOlApplyThreads) void level_out_apply_kernel(const LevelOutApplyArgs a) {
  const int i = blockIdx.y;
  const OlRow& r = a.tab[i];      // uniform in the workgroup
  if (!r.on) return;              // the row keeps its bits
  const int s0 = ((int)blockIdx.x * kOlApplyThreads + (int)threadIdx.x) * 4;
  if (s0 >= a.samples) return;
  float* x = a.x + (long long)i * a.ld;
  float* z = a.stage + (long long)i * a.stage_ld;
  const LvState* S = reinterpret_cast<const LvState*>(a.state + (long long)r.slot * a.state_stride);
  const bool fresh = r.c.pos0 == 0;
  const double sm = S->Gm, sc = S->Gc;
  const double gm = fresh ? r.cfg.g_init : sm, gc = fresh ? r.cfg.g_init : sc;
  const double U = (double)a.U;
  const int clip = r.cfg.clip;
  const bool vec = s0 + 3 < a.samples && ((reinterpret_cast<uintptr_t>(x + s0) | reinterpret_cast<uintptr_t>(z + s0)) & 15) == 0;
  float v[4];
  if (vec) {
    const float4 q = *reinterpret_cast<const float4*>(x + s0);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = x[s0 + e < a.samples ? s0 + e : a.samples - 1];
  }
  float y[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) y[e] = lv_ramp(gm, gc, s0 + e + 1, U, v[e], clip);      // (the row starts at u_k: sample t is the interval's (t + 1)-th)
  if (vec) {
    *reinterpret_cast<float4*>(z + s0) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(x + s0) = make_float4(y[0], y[1], y[2], y[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) if (s0 + e < a.samples) { z[s0 + e] = v[e]; x[s0 + e] = y[e]; }
  }
}

// One workgroup per step row.  Before the meter runs, thread 0 keeps the stats of the instant the row's ramp ended at (the latest one
// so far; at position 0 the start's) as prev: the meter of a whole row overwrites them with the next instant's.
__global__ __launch_bounds__(kLvThreads) void level_out_meter_kernel(const LevelOutMeterArgs a) {
  __shared__ LvShared sh;
  const OlRow& R = a.tab[blockIdx.x];
  if (!R.on) return;
  char* base = a.state + (long long)R.slot * a.state_stride;
  LvState* S = reinterpret_cast<LvState*>(base);
  double* zr = reinterpret_cast<double*>(base + sizeof(LvState));
  double* prev = zr + 2 * (size_t)a.zcap;
  if (threadIdx.x == 0 && R.c.inst) {
    const bool fresh = R.c.pos0 == 0;
    prev[0] = fresh ? -INFINITY : S->stat[0]; prev[1] = fresh ? R.cfg.g_init : S->stat[1];
    prev[2] = fresh ? 0.0 : S->stat[2]; prev[3] = fresh ? 0.0 : S->stat[3];
  }
  lv_meter(a.f, R.cfg, S, zr, zr + a.zcap, a.zcap, R.c, a.stage + (long long)blockIdx.x * a.stage_ld, sh);
}

// conan_streams_output_level: {L_k, G_k, P_k, J_k} of the instant the rows' latest ramps ended at
__global__ __launch_bounds__(64) void level_out_stats_kernel(const LevelOutStatsArgs a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n) return;
  const OlRow& R = a.tab[i];
  const char* base = a.state + (long long)R.slot * a.state_stride;
  const LvState* S = reinterpret_cast<const LvState*>(base);
  const double* prev = reinterpret_cast<const double*>(base + sizeof(LvState)) + 2 * (size_t)a.zcap;
  const double* src = R.prev ? prev : S->stat;
  double* o = a.out + (size_t)i * 4;
  if (R.c.pos0 == 0) { o[0] = -INFINITY; o[1] = R.cfg.g_init; o[2] = 0.0; o[3] = 0.0; }
  else { o[0] = src[0]; o[1] = src[1]; o[2] = src[2]; o[3] = src[3]; }
}

void launch_level_out_apply(const LevelOutApplyArgs& a, hipStream_t st) {
  if (a.n < 1 || a.samples < 1) return;
  const int per = kOlApplyThreads * 4;
  hipLaunchKernelGGL(level_out_apply_kernel, dim3((unsigned)((a.samples + per - 1) / per), (unsigned)a.n), dim3(kOlApplyThreads), 0, st, a);
}

void launch_level_out_meter(const LevelOutMeterArgs& a, hipStream_t st) {
  if (a.n < 1) return;
  hipLaunchKernelGGL(level_out_meter_kernel, dim3((unsigned)a.n), dim3(kLvThreads), 0, st, a);
}

void launch_level_out_stats(const LevelOutStatsArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(level_out_stats_kernel, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, st, a);
}

}  // namespace cnk

namespace olv {

constexpr int kZcap = CONAN_LEVEL_MAX_BLOCKS + cnk::kLvRingPad;

std::vector<cnk::OlRow> step_rows(const conan_streams* s, const int32_t* slots, int n, int frames, const std::string& who) {
  std::vector<cnk::OlRow> rows;
  if (s->out_lv.n_on < 1 || frames < 1) return rows;
  bool any = false;
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] >= s->max_slots) throw Error(CONAN_ERR_INVALID, "slot index out of range");
    any = any || s->out_lv.on(slots[i]);
  }
  if (!any) return rows;
  const int hop = s->ctx->hop, U = s->out_lv.filter.U;
  rows.resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    cnk::OlRow& r = rows[i];
    memset(&r, 0, sizeof(r));
    r.slot = slots[i]; r.state_row = -1;
    if (!s->out_lv.on(slots[i])) continue;
    const std::string where = who + ": slot " + std::to_string(slots[i]) + " levels its output (conan_streams_set_output_level): ";
    if (s->ctx->cfg.voc_upsample == 2) throw Error(CONAN_ERR_UNSUPPORTED, where + "upsample 'nn' runs whole prefixes, not update intervals");
    const long long m = (long long)frames * hop;
    if (m > U) throw Error(CONAN_ERR_UNSUPPORTED, where + "a levelled row carries 1 .. segment * hop samples");
    if (const char* why = level::plan_end(s->wav_out.voc_samples[slots[i]], (int)m, U, 50.0 * hop, r.c)) throw Error(CONAN_ERR_UNSUPPORTED, where + why);
    r.cfg = level::kernel_cfg(s->out_lv.cfg[slots[i]]);
    r.on = 1;
  }
  return rows;
}

int64_t state_bytes(const conan_streams* s) {
  if (!s) throw Error(CONAN_ERR_INVALID, "null streams");
  return (int64_t)cnk::ol_state_bytes(kZcap);
}

void set_level(conan_streams* s, const int32_t* slots, int n, const conan_level_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream) {
  if (!s || !slots || !cfg) throw Error(CONAN_ERR_INVALID, "null argument");
  level::check_cfg(*cfg, "conan_streams_set_output_level");      // (before the handle is touched, before any GPU use)
  if (!(s->ctx->cfg.models & CONAN_MODEL_HIFIGAN)) throw Error(CONAN_ERR_STATE, "conan_streams_set_output_level: context holds no HiFi-GAN model");
  wavio::check_slot_list(s, slots, n);
  const int64_t bytes = (int64_t)cnk::ol_state_bytes(kZcap);
  if (seed_dev && (seed_ld < bytes || ((uintptr_t)seed_dev & 7) || (seed_ld & 7)))
    throw Error(CONAN_ERR_INVALID, "conan_streams_set_output_level: seed rows are conan_streams_output_level_state_bytes bytes, 8-byte aligned, seed_ld apart");
  cnk::LvFilter f;
  if (cfg->enabled) f = level::filter(s->ctx, "conan_streams_set_output_level");
  for (int i = 0; i < n && !seed_dev; ++i)
    if (s->wav_out.voc_samples[slots[i]] != 0)
      throw Error(CONAN_ERR_STATE, "conan_streams_set_output_level: slot " + std::to_string(slots[i]) +
                                       " is not at the start of its vocoder stream (reset it with CONAN_MODEL_HIFIGAN first, or seed it)");
  if (!cfg->enabled && !s->out_lv.allocated()) return;      // a stream-set that never levelled: nothing to allocate, nothing to write
  hipStream_t st = s->enter(stream);      // (rows of pipelined steps in flight were built from the old setting, and their meters write the state)
  if (cfg->enabled) s->out_level_init(f);
  s->out_lv.store(slots, n, *cfg);
  for (int i = 0; i < n && cfg->enabled && seed_dev; ++i)
    HIP_CHECK(hipMemcpyAsync(s->out_lv.state + (size_t)slots[i] * s->out_lv.stride, static_cast<const char*>(seed_dev) + (size_t)i * seed_ld, (size_t)bytes,
                             hipMemcpyDeviceToDevice, st));
}

void stats(conan_streams* s, const int32_t* slots, int n, double* stats_dev, void* stream) {
  if (!s || !slots || !stats_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  wavio::check_slot_list(s, slots, n);
  std::vector<cnk::OlRow> rows((size_t)n);
  for (int i = 0; i < n; ++i) {
    if (!s->out_lv.on(slots[i])) throw Error(CONAN_ERR_STATE, "conan_streams_output_level: slot " + std::to_string(slots[i]) + " has no leveller (conan_streams_set_output_level)");
    memset(&rows[i], 0, sizeof(cnk::OlRow));
    const long long pos = s->wav_out.voc_samples[slots[i]];
    rows[i].cfg = level::kernel_cfg(s->out_lv.cfg[slots[i]]);
    // after a whole row the meter has already formed the NEXT instant's stats: the reading is the one it kept as prev
    rows[i].c.pos0 = pos; rows[i].slot = slots[i]; rows[i].on = 1; rows[i].prev = pos % s->out_lv.filter.U == 0; rows[i].state_row = i;
  }
  hipStream_t st = s->enter(stream);
  const int q = s->out_lv.sets.begin(rows.data(), n, st);
  cnk::LevelOutStatsArgs a;
  a.state = s->out_lv.state; a.state_stride = s->out_lv.stride; a.zcap = kZcap; a.tab = s->out_lv.sets.rows[q]; a.n = n; a.out = stats_dev;
  cnk::launch_level_out_stats(a, st);
  HIP_CHECK(hipGetLastError());
  s->out_lv.sets.end(q, st);
}

void state(conan_streams* s, const int32_t* slots, int n, void* state_dev, int64_t ld, void* stream) {
  if (!s || !slots || !state_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  wavio::check_slot_list(s, slots, n);
  const int64_t bytes = (int64_t)cnk::ol_state_bytes(kZcap);
  if (ld < bytes || ((uintptr_t)state_dev & 7) || (ld & 7))
    throw Error(CONAN_ERR_INVALID, "conan_streams_output_level_state: rows are conan_streams_output_level_state_bytes bytes, 8-byte aligned, ld apart");
  for (int i = 0; i < n; ++i)
    if (!s->out_lv.on(slots[i])) throw Error(CONAN_ERR_STATE, "conan_streams_output_level_state: slot " + std::to_string(slots[i]) + " has no leveller (conan_streams_set_output_level)");
  hipStream_t st = s->enter(stream);
  for (int i = 0; i < n; ++i)
    HIP_CHECK(hipMemcpyAsync(static_cast<char*>(state_dev) + (size_t)i * ld, s->out_lv.state + (size_t)slots[i] * s->out_lv.stride, (size_t)bytes,
                             hipMemcpyDeviceToDevice, st));
}

}  // namespace olv

void conan_streams::out_level_init(const cnk::LvFilter& f) {
  if (out_lv.state) return;
  out_lv.filter = f;
  out_lv.stride = (long long)cnk::ol_state_bytes(olv::kZcap);
  out_lv.state = reinterpret_cast<char*>(alloc((size_t)max_slots * out_lv.stride / sizeof(float)));      // zeroed (counted by state_bytes)
  for (int q = 0; q < kActSets; ++q) out_lv.stage[q] = alloc((size_t)max_slots * f.U);
  out_lv.sets.init(max_slots, allocs);
  state_bytes += (int64_t)kActSets * max_slots * sizeof(cnk::OlRow);
  out_lv.assign(max_slots);
}
