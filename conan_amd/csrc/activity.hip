// Source activity (include/conan_hip.h, conan_activity_cfg): the detector's kernel and the gate's, the whole-signal entry points
// conan_activity / conan_activity_gate and the host side of conan_streams_set_activity.  The wav-in steps launch the detector behind
// their front-end launch on the rows of the call's activity staging (act::WavStage below); the vocoder step of a chunk with a gated row launches
// the gate between conv_post and the output resampler (streams.hip, hifigan_step).
#include <climits>
#include <cmath>

#include "streams.h"

namespace cnk {

// The law's power of U frames of one row at once, by one wave: lane j holds the partial sums p_j of the U frames (x[j], x[j + 64], ...
// in ascending order: consecutive lanes read consecutive samples).  The loads of four steps of the U frames are issued together -
// one load in flight per wave is what a dependent fma chain would otherwise wait for - and the sums then take the steps in the law's
// order.  A step past the frame's end adds x = 0 to a non-negative sum, which leaves its bits alone; every load is unconditional at a
// clamped address and the zero padding is selected after it.  Lane 0 returns with the law's fold.
template <int U>
__device__ __forceinline__ void frame_powers(const float* __restrict__ src, const ActRow& r, const long long last, const long long (&s0)[U], const int N,
                                             const int lane, double (&p)[U]) {
#pragma unroll
  for (int u = 0; u < U; ++u) p[u] = 0.0;
  for (int k0 = 0; k0 < N; k0 += 256) {
    float v[4][U];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long si = s0[u] + k0 + e * 64 + lane;
        const long long sc = si < 0 ? 0 : (si > last ? last : si);
        v[e][u] = src[sc & (long long)r.mask];
      }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long si = s0[u] + k0 + e * 64 + lane;
        const double x = k0 + e * 64 + lane < N && si >= 0 && si < r.valid ? (double)v[e][u] : 0.0;
        p[u] = fma(x, x, p[u]);
      }
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
    for (int d = 32; d >= 1; d >>= 1) p[u] = p[u] + __shfl_down(p[u], d);
}

// One row per workgroup, the row's frames in tiles of the workgroup's size (kActThreads lanes for whole signals, kActStreamThreads
// for the rows of a wav-in call: a workgroup of 16 waves at this kernel's 126 VGPRs needs a CU with every SIMD's register file free,
// which a pipelined call's front-end would wait for while the vocoder fills the device).  The power sums are the parallel part: a wave per frame - four
// frames per wave at a time where the tile has that many, so that a whole signal's row keeps 16 loads per lane in flight
// (frame_powers).  The recursion over the tile's frames is sequential and belongs to thread 0, which keeps the state in registers
// from tile to tile; the tile's flags and levels go out through LDS so that the stores are consecutive over the lanes.  Nothing here
// depends on the tile width, the wave count or the launch's other rows.
__global__ __launch_bounds__(kActThreads) void activity_kernel(const ActArgs a) {
  __shared__ double pw_s[kActThreads];
  __shared__ int act_s[kActThreads];
  __shared__ int lvl_s[kActThreads];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = blockDim.x, W = T >> 6;    // tile width, waves
  if ((int)blockIdx.x >= a.rows) return;
  const ActRow r = a.tab[blockIdx.x];      // uniform in the workgroup
  if (r.mode == 0) return;                 // a row of a slot without the feature (it holds the gate's place in the table)
  ActState s = r.seed;
  if (tid == 0) {
    if (!r.reseed && r.slot >= 0) s = a.state[r.slot];
    if (r.start_lvl) a.lvl[r.lvl_off - 1] = s.level;
  }
  const int N = a.n_fft, hop = a.hop;
  const long long last = r.valid > 0 ? r.valid - 1 : 0;
  const float* src = a.src + r.src_off;
  const double inv_n = 1.0 / (double)N;      // (N is a power of two: the product is the quotient, exactly)
  for (int base = 0; base < r.nframes; base += T) {
    const int nt = r.nframes - base < T ? r.nframes - base : T;
    int j = wave;
    for (; j + 3 * W < nt; j += 4 * W) {      // frames j, j + W, j + 2 W, j + 3 W of the tile
      long long s0[4];
      double p[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) s0[u] = (long long)(r.f_first + base + j + u * W) * hop - N / 2;
      frame_powers<4>(src, r, last, s0, N, lane, p);
#pragma unroll
      for (int u = 0; u < 4; ++u) if (lane == 0) pw_s[j + u * W] = p[u] * inv_n;
    }
    for (; j < nt; j += W) {
      const long long s0[1] = {(long long)(r.f_first + base + j) * hop - N / 2};
      double p[1];
      frame_powers<1>(src, r, last, s0, N, lane, p);
      if (lane == 0) pw_s[j] = p[0] * inv_n;
    }
    __syncthreads();
    if (tid == 0) {
      for (int j = 0; j < nt; ++j) {
        const double P = pw_s[j];
        const double open = fmax(r.open_abs, s.floor * r.open_ratio), close = fmax(r.close_abs, s.floor * r.close_ratio);
        const bool raw = P > (s.active ? close : open);
        int act = 0;
        if (raw) { act = 1; s.hang = r.hold; }
        else if (s.hang > 0) { act = 1; s.hang -= 1; }
        s.floor = fmax(fmin(P, s.floor * (act ? r.rise_active : r.rise_idle)), r.floor_min);
        const int up = s.level + r.up_step, down = s.level - r.down_step;
        s.level = act ? (up < kActFull ? up : kActFull) : (down > r.closed_level ? down : r.closed_level);
        s.active = act; s.frames += 1; s.active_frames += act;
        act_s[j] = act; lvl_s[j] = s.level;
      }
    }
    __syncthreads();
    if (tid < nt) {
      a.act[r.out_off + base + tid] = act_s[tid];
      a.lvl[r.lvl_off + base + tid] = lvl_s[tid];
      if (a.power) a.power[r.out_off + base + tid] = pw_s[tid];
    }
    __syncthreads();      // (the next tile writes the LDS rows again)
  }
  if (tid == 0) {
    if (r.slot >= 0) a.state[r.slot] = s;
    if (r.state_row >= 0) a.state_out[r.state_row] = s;
  }
}

// Four consecutive samples per thread: one 16-byte load and store where the thread's samples are whole and aligned (always, in a
// vocoder step: a row is emit * hop samples of staging or of the caller's buffer), single words otherwise (the tail of a whole signal,
// an odd stride).  The gain is the law's: an integer interpolation of the frame's two levels, one f64 division, one f32 product.
__global__ __launch_bounds__(kActGateThreads) void activity_gate_kernel(const ActGateArgs a) {
  const int i = blockIdx.y;
  if (a.tab && a.tab[i].mode != 2) return;      // uniform: the row is not gated and keeps its bits
  const float* x = a.x + (long long)i * a.ld;
  float* y = a.y + (long long)i * a.ld_y;
  const int* lv = a.lvl + (long long)i * a.lvl_ld;
  const long long s0 = ((long long)blockIdx.x * kActGateThreads + threadIdx.x) * 4;
  if (s0 >= a.samples) return;
  const int start = a.start_in_lvl ? lv[-1] : a.start;
  const int hop = a.hop;
  const double den = (double)((long long)hop << 20);
  const bool vec = s0 + 3 < a.samples && ((reinterpret_cast<uintptr_t>(x + s0) | reinterpret_cast<uintptr_t>(y + s0)) & 15) == 0;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (vec) {
    const float4 q = *reinterpret_cast<const float4*>(x + s0);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) if (s0 + e < a.samples) v[e] = x[s0 + e];
  }
  float o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long long sx = s0 + e < a.samples ? s0 + e : a.samples - 1;      // (clamped: the levels of a sample past the row are never read)
    const long long f = sx / hop;
    const int k = (int)(sx - f * hop);
    const int lp = f > 0 ? lv[f - 1] : start, ln = lv[f];
    const long long l = (long long)lp * (hop - 1 - k) + (long long)ln * (k + 1);
    const float g = (float)((double)l / den);
    o[e] = __fmul_rn(v[e], g);
  }
  if (vec) {
    *reinterpret_cast<float4*>(y + s0) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) if (s0 + e < a.samples) y[s0 + e] = o[e];
  }
}

void launch_activity(const ActArgs& a, hipStream_t st) {
  if (a.rows < 1) return;
  hipLaunchKernelGGL(activity_kernel, dim3(a.rows), dim3(a.long_rows ? kActThreads : kActStreamThreads), 0, st, a);
}

void launch_activity_gate(const ActGateArgs& a, hipStream_t st) {
  if (a.n < 1 || a.samples < 1) return;
  const long long per = (long long)kActGateThreads * 4;
  hipLaunchKernelGGL(activity_gate_kernel, dim3((unsigned)((a.samples + per - 1) / per), a.n), dim3(kActGateThreads), 0, st, a);
}

}  // namespace cnk

namespace act {

static_assert(sizeof(conan_activity_state) == sizeof(cnk::ActState), "the kernels' state is the header's");
static_assert(CONAN_ACTIVITY_FULL == cnk::kActFull, "2^20");

void check_cfg(const conan_activity_cfg& c, const char* who) {
  const std::string w = std::string(who) + ": ";
  auto bad = [&](const char* what) { throw Error(CONAN_ERR_INVALID, w + what); };
  if (c.mode < 0 || c.mode > 2) bad("conan_activity_cfg.mode must be 0, 1 or 2");
  if (!c.mode) return;      // (the other fields are ignored)
  if (c.reseed != 0 && c.reseed != 1) bad("conan_activity_cfg.reseed must be 0 or 1");
  const float fl[7] = {c.open_abs, c.close_abs, c.open_ratio, c.close_ratio, c.rise_active, c.rise_idle, c.floor_min};
  for (float v : fl) if (!std::isfinite(v)) bad("every threshold, ratio and rise must be finite");
  if (!(c.close_abs >= 0.f) || !(c.close_abs <= c.open_abs)) bad("0 <= close_abs <= open_abs");
  if (!(c.close_ratio >= 0.f) || !(c.close_ratio <= c.open_ratio)) bad("0 <= close_ratio <= open_ratio");
  if (!(c.rise_active >= 1.f) || !(c.rise_idle >= 1.f)) bad("rise_active and rise_idle must be >= 1");
  if (!(c.floor_min > 0.f)) bad("floor_min must be > 0");
  if (c.hold_frames < 0 || c.hold_frames > cnk::kActFull) bad("hold_frames must be in 0 .. 2^20");
  if (c.up_step < 1 || c.up_step > cnk::kActFull || c.down_step < 1 || c.down_step > cnk::kActFull) bad("up_step and down_step must be in 1 .. 2^20");
  if (c.closed_level < 0 || c.closed_level > cnk::kActFull - 1) bad("closed_level must be in 0 .. 2^20 - 1");
  if (c.reserved != 0 || c.seed.reserved != 0) bad("the reserved words must be 0");
  if (c.seed.level < c.closed_level || c.seed.level > cnk::kActFull) bad("seed.level must be in closed_level .. 2^20");
  if (!std::isfinite(c.seed.floor) || !(c.seed.floor >= (double)c.floor_min)) bad("seed.floor must be finite and >= floor_min");
  if (c.seed.active != 0 && c.seed.active != 1) bad("seed.active must be 0 or 1");
  if (c.seed.hang < 0 || c.seed.hang > cnk::kActFull) bad("seed.hang must be in 0 .. 2^20");
  if (c.seed.frames < 0 || c.seed.active_frames < 0 || c.seed.active_frames > c.seed.frames) bad("seed counters: 0 <= active_frames <= frames");
}

cnk::ActRow row(const conan_activity_cfg& c) {
  cnk::ActRow r;
  memset(&r, 0, sizeof(r));
  r.open_abs = (double)c.open_abs; r.close_abs = (double)c.close_abs; r.open_ratio = (double)c.open_ratio; r.close_ratio = (double)c.close_ratio;
  r.rise_active = (double)c.rise_active; r.rise_idle = (double)c.rise_idle; r.floor_min = (double)c.floor_min;
  memcpy(&r.seed, &c.seed, sizeof(r.seed));
  r.hold = c.hold_frames; r.up_step = c.up_step; r.down_step = c.down_step; r.closed_level = c.closed_level;
  r.mode = c.mode; r.mask = -1; r.reseed = 1; r.slot = -1; r.state_row = -1;
  return r;
}

void check_mel(const conan_mel_cfg& m, const char* who) {
  const std::string w = std::string(who) + ": ";
  if (m.fft_size < 64 || (m.fft_size & (m.fft_size - 1)) || m.fft_size > 2048) throw Error(CONAN_ERR_INVALID, w + "fft_size must be a power of two in [64, 2048]");
  if (m.hop_size < 1 || m.hop_size > 2047) throw Error(CONAN_ERR_INVALID, w + "hop_size must be in 1 .. 2047");
  if (m.sample_rate != 50 * m.hop_size) throw Error(CONAN_ERR_INVALID, w + "sample_rate must be 50 * hop_size (20 ms frames)");
}

void whole(conan_ctx* ctx, const conan_mel_cfg* mel, const conan_activity_cfg* cfg, const float* wav_dev, int n, int samples, int32_t* act_out_dev,
           int32_t* level_out_dev, double* power_out_dev, conan_activity_state* state_out_dev, int32_t* frames_out, void* stream) {
  if (!ctx || !mel || !cfg || !wav_dev || !act_out_dev || !level_out_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  check_mel(*mel, "conan_activity");
  check_cfg(*cfg, "conan_activity");
  if (!cfg->mode) throw Error(CONAN_ERR_INVALID, "conan_activity: cfg.mode must be 1 or 2");
  if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, "conan_activity: n must be in 1 .. 65535");
  if (samples < 1) throw Error(CONAN_ERR_INVALID, "conan_activity: an utterance needs at least one sample");
  const int frames = 1 + samples / mel->hop_size;
  if (frames_out) *frames_out = frames;
  HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t table = (size_t)n * sizeof(cnk::ActRow);
  cnk::ActRow* h = static_cast<cnk::ActRow*>(ctx->loud_stage.take(table));
  const cnk::ActRow proto = row(*cfg);
  for (int i = 0; i < n; ++i) {
    h[i] = proto;
    h[i].src_off = (long long)i * samples; h[i].valid = samples; h[i].out_off = (long long)i * frames; h[i].lvl_off = h[i].out_off;
    h[i].nframes = frames; h[i].state_row = state_out_dev ? i : -1;
  }
  char* ws = reinterpret_cast<char*>(ctx->workspace((table + sizeof(float) - 1) / sizeof(float), st));
  HIP_CHECK(hipMemcpyAsync(ws, h, table, hipMemcpyHostToDevice, st));
  ctx->loud_stage.sent(st);
  cnk::ActArgs a;
  memset(&a, 0, sizeof(a));
  a.src = wav_dev; a.act = act_out_dev; a.lvl = level_out_dev; a.power = power_out_dev;
  a.state_out = reinterpret_cast<cnk::ActState*>(state_out_dev);
  a.tab = reinterpret_cast<const cnk::ActRow*>(ws); a.rows = n; a.n_fft = mel->fft_size; a.hop = mel->hop_size;
  a.long_rows = frames > 4 * (cnk::kActStreamThreads / 64);
  cnk::launch_activity(a, st);
  HIP_CHECK(hipGetLastError());
}

void gate(conan_ctx* ctx, int hop, const float* wav_dev, int n, int64_t samples, int64_t ld, const int32_t* level_dev, int64_t level_ld, int32_t start_level,
          float* out_dev, void* stream) {
  if (!ctx || !wav_dev || !level_dev || !out_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  if (hop < 1 || hop > 2047) throw Error(CONAN_ERR_INVALID, "conan_activity_gate: hop must be in 1 .. 2047");
  if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, "conan_activity_gate: n must be in 1 .. 65535");
  if (samples < 1 || samples > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_activity_gate: samples must be in 1 .. 2^31 - 1");
  if (ld < samples || ld > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_activity_gate: ld must be in samples .. 2^31 - 1");
  if (level_ld < (samples + hop - 1) / hop || level_ld > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_activity_gate: level_ld must cover ceil(samples / hop) frames");
  if (start_level < 0 || start_level > cnk::kActFull) throw Error(CONAN_ERR_INVALID, "conan_activity_gate: start_level must be in 0 .. 2^20");
  HIP_CHECK(hipSetDevice(ctx->device));
  cnk::ActGateArgs a;
  memset(&a, 0, sizeof(a));
  a.x = wav_dev; a.y = out_dev; a.lvl = level_dev; a.tab = nullptr; a.ld = ld; a.ld_y = ld; a.lvl_ld = level_ld; a.samples = samples;
  a.n = n; a.hop = hop; a.start = start_level; a.start_in_lvl = 0;
  cnk::launch_activity_gate(a, (hipStream_t)stream);
  HIP_CHECK(hipGetLastError());
}

void set_activity(conan_streams* s, const int32_t* slots, int n, const conan_activity_cfg* cfg, void* stream) {
  if (!s || !slots || !cfg) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_streams_set_activity");      // (before the handle is touched, before any GPU use)
  if (!wavio::begin_setter(s, slots, n, cfg->mode != 0, s->act.allocated(), "conan_streams_set_activity", stream)) return;
  s->activity_init();
  s->act.store_restarting(slots, n, *cfg);      // the restart travels in the slot's next detector row
}

// rows without frames: a pending slot's row starts from the seed and names no slot, any other reads its state (and writes it back as it is)
void state(conan_streams* s, const int32_t* slots, int n, conan_activity_state* state_dev, void* stream) {
  if (!s || !slots || !state_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  wavio::check_slot_list(s, slots, n);
  const std::vector<cnk::ActRow> rows = s->act.state_rows<cnk::ActRow>(slots, n, row, "conan_streams_activity_state", " has no activity detector (conan_streams_set_activity)");
  hipStream_t st = s->enter(stream);
  const int q = s->act.sets.begin(rows.data(), n, st);
  cnk::ActArgs a;
  memset(&a, 0, sizeof(a));
  a.src = s->wav_in.fe_audio; a.act = s->act.flags[q]; a.lvl = s->act.levels[q];      // (no frames: nothing is read or written there)
  a.state = s->act.state; a.state_out = reinterpret_cast<cnk::ActState*>(state_dev); a.tab = s->act.sets.rows[q]; a.rows = n;
  a.n_fft = 64; a.hop = s->ctx->hop;
  cnk::launch_activity(a, st);
  HIP_CHECK(hipGetLastError());
  s->act.sets.end(q, st);      // (only the set's table was taken: the staging beside it still holds what its last wav-in call wrote)
}

// the flags and levels the last wav-in call produced, in call order: rows of `seg`, zeros where a row had no detector or did not emit
void last_call(conan_streams* s, int32_t* act_dev, int32_t* level_dev, void* stream) {
  if (!s || !act_dev || !level_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  hipStream_t st = wavio::begin_last_call(s, "conan_step_wav_activity", stream);
  const int seg = s->ctx->cfg.emf_segment, n = s->wav_in.fe_last_n;
  copy_last_rows(s->act.last, act_dev, n, seg, s->act.flags, seg, 0, st);
  copy_last_rows(s->act.last, level_dev, n, seg, s->act.levels, seg + 1, 1, st);
}

void WavStage::plan(const conan_streams* s, const WavCall& c) {
  if (s->act.n_on < 1) return;
  bool any = false;
  for (int i = 0; i < c.n; ++i) {
    if (!s->act.on(c.slots[i])) continue;
    if (c.mel.sample_rate != 50 * c.hop) throw Error(CONAN_ERR_INVALID, c.who + ": slot " + std::to_string(c.slots[i]) + " detects source activity: conan_mel_cfg.sample_rate must be 50 * hop_size");
    const FePlan& p = c.pl[i];
    if (p.emit < 1) continue;
    if (p.R - std::max(0ll, (long long)p.pos * c.hop - c.N / 2) > s->wav_in.fe_LA)
      throw Error(CONAN_ERR_UNSUPPORTED, c.who + ": slot " + std::to_string(c.slots[i]) + " detects source activity: the chunk's frames have left the audio ring at this fft_size");
    any = true;
  }
  if (!any) return;
  gate.assign(c.groups.size(), 0);
  rows = c.table_rows<cnk::ActRow>([&](int g, int i, int at, cnk::ActRow& r) {
    const int slot = c.slots[i];
    if (!s->act.on(slot)) return false;
    const FePlan& p = c.pl[i];
    r = row(s->act.cfg[slot]);
    r.src_off = (long long)slot * s->wav_in.fe_LA; r.valid = p.R; r.mask = s->wav_in.fe_LA - 1;
    r.f_first = p.pos; r.nframes = p.emit; r.slot = slot; r.reseed = s->act.pending[slot]; r.start_lvl = 1;
    last.push_back({i, 0, at, p.emit});
    if (r.mode == 2) gate[g] = 1;
    return true;
  });
  for (size_t at = 0; at < rows.size(); ++at) { rows[at].out_off = (long long)at * c.seg; rows[at].lvl_off = (long long)at * (c.seg + 1) + 1; }
}

// the detector, behind the front-end launch (and the tracker's and the register's): the call's samples are in the audio rings
void WavStage::enqueue(conan_streams* s, const WavCall& c, hipStream_t cst, FrontWork& front, std::vector<conan_streams::OutPlan>& ops) {
  if (rows.empty()) return;
  q = s->act.sets.begin(rows.data(), (int)rows.size(), cst);
  for (LastRow& r : last) r.set = q;
  cnk::ActArgs a;
  memset(&a, 0, sizeof(a));
  a.src = s->wav_in.fe_audio; a.act = s->act.flags[q]; a.lvl = s->act.levels[q]; a.state = s->act.state;
  a.power = power;      // (comfort.hip: a following row of the call reads the frame powers; null otherwise)
  a.tab = s->act.sets.rows[q]; a.rows = (int)rows.size(); a.n_fft = c.N; a.hop = c.hop;
  front.at[kFrActivity] = [s, a](hipStream_t st) { s->profiled("activity_kernel", 0.0, st, [&] { cnk::launch_activity(a, st); }); };
  c.each_group([&](int g, int off) {
    if (gate[g]) ops[g].gate = {s->act.sets.rows[q] + off, s->act.levels[q] + (size_t)off * (c.seg + 1) + 1, c.seg + 1};
  });
}

void WavStage::commit(conan_streams* s, hipStream_t, hipStream_t last_st) {
  if (!rows.empty()) s->act.sets.end(q, last_st);      // (behind the call's last vocoder step: the gate is the last reader of table and levels)
  for (const cnk::ActRow& r : rows) if (r.slot >= 0) s->act.pending[r.slot] = 0;      // (the rows carried the restarts)
  s->act.last = std::move(last);
}

}  // namespace act

void conan_streams::activity_init() {
  if (act.state) return;
  const int seg = ctx->cfg.emf_segment;
  act.state = reinterpret_cast<cnk::ActState*>(alloc((size_t)max_slots * sizeof(cnk::ActState) / sizeof(float)));      // zeroed (counted by state_bytes)
  for (int q = 0; q < kActSets; ++q) {
    act.flags[q] = reinterpret_cast<int*>(alloc((size_t)max_slots * seg));
    act.levels[q] = reinterpret_cast<int*>(alloc((size_t)max_slots * (seg + 1)));
  }
  act.sets.init(max_slots, allocs);
  state_bytes += (int64_t)kActSets * max_slots * sizeof(cnk::ActRow);
  act.assign(max_slots);
}
