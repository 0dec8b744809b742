// Streaming leveller (conan_level, conan_streams_set_input_level): the causal BS.1770 leveller that include/conan_hip.h defines
// (conan_level_cfg).  The plan is in kernels.h (LvState, LvCall); lv_chunk is the one routine that level_stream_kernel (a wav-in
// call's rows) and level_signal_kernel (whole signals, one update interval at a time) both call, so the two agree bit for bit.
// The host side of the streaming form follows the kernels (the setter, the query and level::WavStage, the leveller's part of a wav-in
// call); conan_ctx_level below is conan_level's body.
#include <climits>
#include <cmath>

#include "level_dev.h"
#include "streams.h"

namespace cnk {

// One chunk of one stream: c.m samples at x (position c.pos0 on) -> y (may be x): the meter (level_dev.h), then the ramps.  Called by
// every thread of a kLvThreads workgroup with the same arguments; c lives in LDS or in the kernel's arguments.
__device__ void lv_chunk(const LvFilter& f, const LvCfg& cfg, LvState* S, double* zr, double* lr, int zcap, const LvCall& c, const float* x, float* y,
                         LvShared& sh) {
  lv_meter(f, cfg, S, zr, lr, zcap, c, x, sh);
  // 5. the ramps: g_t = G_{k-1} + (G_k - G_{k-1}) * ((t - u_k + 1) / U), two roundings; y = f32(f64(x) * g_t), one rounding
  const int tail = (int)(c.pos0 & (kLdSeg - 1));
  const int off = (int)(c.pos0 % f.U);      // samples of the interval that came before this chunk
  const double U = (double)f.U;
  for (int t = threadIdx.x; t < c.m; t += kLvThreads) {
    const bool after = c.inst && t >= c.u;
    const double gm = after ? sh.g[2] : sh.g[0], gc = after ? sh.g[3] : sh.g[1];
    const int i = tail + t;
    y[t] = lv_ramp(gm, gc, after ? t - c.u + 1 : off + t + 1, U, sh.buf[(i >> 7) * kLdStride + (i & (kLdSeg - 1))], cfg.clip);
  }
  __syncthreads();
}

__global__ __launch_bounds__(kLvThreads) void level_stream_kernel(const LevelStreamArgs a) {
  __shared__ LvShared sh;
  const LvRow& R = a.rows[blockIdx.x];
  if (R.copy) {      // (the whole workgroup: an unlevelled row on its way to the staging the front-end reads)
    const float* x = a.x + (size_t)R.row * a.x_ld;
    float* y = a.y + (size_t)R.row * a.y_ld;
    for (int t = threadIdx.x; t < R.c.m; t += kLvThreads) y[t] = x[t];
    return;
  }
  char* base = a.state + (size_t)R.slot * a.state_stride;
  LvState* S = reinterpret_cast<LvState*>(base);
  double* zr = reinterpret_cast<double*>(base + sizeof(LvState));
  lv_chunk(a.f, R.cfg, S, zr, zr + a.zcap, a.zcap, R.c, a.x + (size_t)R.row * a.x_ld, a.y + (size_t)R.row * a.y_ld, sh);
}

// conan_streams_input_level: {L_k, G_k, P_k, J_k} of the rows' latest instants
__global__ __launch_bounds__(64) void level_stats_kernel(const LevelStatsArgs a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n) return;
  const LvRow& R = a.rows[i];
  const LvState* S = reinterpret_cast<const LvState*>(a.state + (size_t)R.slot * a.state_stride);
  double* o = a.out + (size_t)i * 4;
  if (R.fresh) { o[0] = -INFINITY; o[1] = R.cfg.g_init; o[2] = 0.0; o[3] = 0.0; }
  else { o[0] = S->stat[0]; o[1] = S->stat[1]; o[2] = S->stat[2]; o[3] = S->stat[3]; }
}

// Whole signals: the row's update intervals in order, each one chunk with its instant at the chunk's start.
__global__ __launch_bounds__(kLvThreads) void level_signal_kernel(const LevelSignalArgs a) {
  __shared__ LvShared sh;
  __shared__ LvCall c;
  const LvSigRow R = a.rows[blockIdx.x];
  char* base = a.state + (size_t)blockIdx.x * a.state_stride;
  LvState* S = reinterpret_cast<LvState*>(base);
  double* zr = reinterpret_cast<double*>(base + sizeof(LvState));
  const int* blk = a.blocks + (size_t)R.blk0 * 2;
  const float* x = a.x + (size_t)blockIdx.x * a.x_ld;
  float* y = a.y + (size_t)blockIdx.x * a.y_ld;
  const int U = a.f.U;
  int J = 0;      // thread 0's: the blocks complete at the instant p, which is also the first block that ends behind the chunk's start
  for (long long p = 0, k = 0; p < R.samples; p += U, ++k) {
    if (threadIdx.x == 0) {
      const int m = (int)min((long long)U, R.samples - p), span = m / kLdSeg * kLdSeg;      // (U is a multiple of kLdSeg: no pending tail at p)
      while (J < R.nblocks && blk[2 * J + 1] <= p) ++J;
      int nb = 0;
      while (nb < kLvBlocks && J + nb < R.nblocks && blk[2 * (J + nb)] < p + span) {
        c.lo[nb] = (int)(blk[2 * (J + nb)] - p); c.hi[nb] = (int)(blk[2 * (J + nb) + 1] - p);
        ++nb;
      }
      c.pos0 = p; c.m = m; c.inst = 1; c.u = 0; c.J = J; c.j0 = J; c.nblk = nb;
    }
    __syncthreads();
    lv_chunk(a.f, a.cfg, S, zr, zr + a.zcap, a.zcap, c, x + p, y + p, sh);
    if (a.trace && threadIdx.x == 0) {
      double* o = a.trace + ((size_t)blockIdx.x * a.trace_ld + k) * 2;
      o[0] = S->stat[0]; o[1] = S->stat[1];
    }
    __syncthreads();
  }
}

void launch_level_stream(const LevelStreamArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(level_stream_kernel, dim3((unsigned)a.n), dim3(kLvThreads), 0, st, a);
}

void launch_level_stats(const LevelStatsArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(level_stats_kernel, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, st, a);
}

void launch_level_signal(const LevelSignalArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(level_signal_kernel, dim3((unsigned)a.n), dim3(kLvThreads), 0, st, a);
}

}  // namespace cnk

namespace level {

void check_cfg(const conan_level_cfg& c, const char* who) {
  using ch::Error;
  const std::string w(who);
  if (c.enabled != 0 && c.enabled != 1) throw Error(CONAN_ERR_INVALID, w + ": enabled must be 0 or 1");
  if (!c.enabled) return;
  if (!std::isfinite(c.target_lufs)) throw Error(CONAN_ERR_INVALID, w + ": target_lufs must be finite");
  if (!std::isfinite(c.max_boost_db) || !std::isfinite(c.max_cut_db) || c.max_boost_db < 0.f || c.max_cut_db < 0.f)
    throw Error(CONAN_ERR_INVALID, w + ": max_boost_db and max_cut_db must be finite and >= 0");
  if (!std::isfinite(c.initial_gain_db)) throw Error(CONAN_ERR_INVALID, w + ": initial_gain_db must be finite");
  if (c.window_blocks < 1 || c.window_blocks > CONAN_LEVEL_MAX_BLOCKS) throw Error(CONAN_ERR_INVALID, w + ": window_blocks must be in 1 .. CONAN_LEVEL_MAX_BLOCKS");
  if ((c.peak_limit != 0 && c.peak_limit != 1) || (c.clip != 0 && c.clip != 1)) throw Error(CONAN_ERR_INVALID, w + ": peak_limit and clip must be 0 or 1");
  if (c.reserved[0] || c.reserved[1] || c.reserved[2] || c.reserved[3]) throw Error(CONAN_ERR_INVALID, w + ": reserved fields must be 0");
}

cnk::LvCfg kernel_cfg(const conan_level_cfg& c) {
  cnk::LvCfg k;
  memset(&k, 0, sizeof(k));
  k.target = (double)c.target_lufs; k.boost = (double)c.max_boost_db; k.cut = (double)c.max_cut_db;
  k.g_init = std::pow(10.0, (double)c.initial_gain_db / 20.0);
  k.window = c.window_blocks; k.peak_limit = c.peak_limit; k.clip = c.clip;
  return k;
}

// The context's rate and update interval in the kernels' terms; CONAN_ERR_UNSUPPORTED where the segmented plan does not hold.
cnk::LvFilter filter(const conan_ctx* ctx, const char* who) {
  using ch::Error;
  const std::string w(who);
  if (!(ctx->cfg.models & CONAN_MODEL_EMFORMER) || ctx->cfg.emf_segment < 1 || ctx->hop < 1) throw Error(CONAN_ERR_STATE, w + ": the context holds no Emformer model (the update interval is segment * hop)");
  const long long U = (long long)ctx->cfg.emf_segment * ctx->hop;
  const double fs = 50.0 * ctx->hop;
  if (U % cnk::kLdSeg || U > cnk::kLvMaxU) throw Error(CONAN_ERR_UNSUPPORTED, w + ": segment * hop must be a multiple of 128 and at most 1920");
  // at most two block edges inside a segment, at most kLvBlocks blocks over a chunk's segments
  if (fs < 2000.0 || std::ceil((kTg * fs + (double)U + cnk::kLdSeg) / (kTg * kStep * fs)) + 2.0 > (double)cnk::kLvBlocks)
    throw Error(CONAN_ERR_UNSUPPORTED, w + ": the model rate is too low for the segmented meter");
  cnk::LvFilter f;
  memset(&f, 0, sizeof(f));
  conan_k_weighting(fs, f.shelf, f.hp, f.M);
  f.block_len = kTg * fs;
  f.U = (int)U;
  return f;
}

// level_plan.h's plan of the chunk [pos0, pos0 + m); CONAN_ERR_UNSUPPORTED where it cannot be planned
cnk::LvCall plan_call(long long pos0, int m, int U, double fs) {
  cnk::LvCall c;
  if (const char* why = plan_call(pos0, m, U, fs, c)) throw ch::Error(CONAN_ERR_UNSUPPORTED, std::string("input level: ") + why);
  return c;
}

void check_common(const conan_streams* s, const int32_t* slots, int n, const std::string& who) {
  for (int i = 1; i < n && s->in_lv.n_on > 0; ++i) {
    const conan_level_cfg &l0 = s->in_lv.cfg[slots[0]], &l = s->in_lv.cfg[slots[i]];
    if (l.enabled != l0.enabled || (l.enabled && memcmp(&l, &l0, sizeof(l))))
      throw Error(CONAN_ERR_INVALID, who + ": the slots of one call must share one input level configuration (conan_streams_set_input_level)");
  }
}

void set_input_level(conan_streams* s, const int32_t* slots, int n, const conan_level_cfg* cfg) {
  if (!s || !slots || !cfg) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_streams_set_input_level");
  if (!s->wav_in.fe_audio) throw Error(CONAN_ERR_STATE, "conan_streams_set_input_level: the stream-set has no streaming front-end (all three models)");
  wavio::check_slot_list(s, slots, n);
  cnk::LvFilter f;
  if (cfg->enabled) f = filter(s->ctx, "conan_streams_set_input_level");
  wavio::check_utterance_start(s, slots, n, "conan_streams_set_input_level");
  if (!cfg->enabled && !s->in_lv.allocated()) return;      // a stream-set that never had a leveller: nothing to allocate
  if (cfg->enabled) {
    HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
    s->level_init(f);
  }
  s->in_lv.store(slots, n, *cfg);
}

void input_level(conan_streams* s, const int32_t* slots, int n, double* stats_dev, void* stream) {
  if (!s || !slots || !stats_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  wavio::check_slot_list(s, slots, n);
  std::vector<cnk::LvRow> rows((size_t)n);
  for (int i = 0; i < n; ++i) {
    if (!s->in_lv.on(slots[i])) throw Error(CONAN_ERR_STATE, "conan_streams_input_level: slot " + std::to_string(slots[i]) + " has no leveller (conan_streams_set_input_level)");
    memset(&rows[i], 0, sizeof(cnk::LvRow));
    rows[i].cfg = kernel_cfg(s->in_lv.cfg[slots[i]]);
    rows[i].slot = slots[i]; rows[i].row = i; rows[i].fresh = s->wav_in.fe_slot[slots[i]].recv == 0;
  }
  hipStream_t st = s->enter(stream);
  const int q = s->in_lv.sets.begin(rows.data(), n, st);
  cnk::LevelStatsArgs a;
  a.state = s->in_lv.state; a.state_stride = s->in_lv.stride; a.rows = s->in_lv.sets.rows[q]; a.n = n; a.out = stats_dev;
  cnk::launch_level_stats(a, st);
  HIP_CHECK(hipGetLastError());
  s->in_lv.sets.end(q, st);
}

void WavStage::plan(const conan_streams* s, const WavCall& c) {
  bool any = false;
  for (int i = 0; i < c.n && s->in_lv.n_on > 0; ++i) any = any || (s->in_lv.on(c.slots[i]) && c.samples[i] > 0);
  stages = any && !c.rs_launch && !c.pre_staged;
  for (int i = 0; i < c.n && any; ++i) {
    const bool on = s->in_lv.on(c.slots[i]);
    if (c.samples[i] < 1 || (!on && !stages)) continue;
    cnk::LvRow R;
    memset(&R, 0, sizeof(R));
    if (on) {
      R.c = plan_call(s->wav_in.fe_slot[c.slots[i]].recv, c.samples[i], s->in_lv.filter.U, 50.0 * c.hop);
      R.cfg = kernel_cfg(s->in_lv.cfg[c.slots[i]]);
    } else {
      R.c.m = c.samples[i]; R.copy = 1;
    }
    R.slot = c.slots[i]; R.row = i;
    rows.push_back(R);
  }
}

// the leveller, between the resampler's launch (or the caller's rows) and the front-end's, which is the last reader of its rows
void WavStage::enqueue(conan_streams* s, const WavCall& c, hipStream_t cst, FrontWork& front, std::vector<conan_streams::OutPlan>&) {
  if (rows.empty()) return;
  const int q = s->in_lv.sets.begin(rows.data(), (int)rows.size(), cst);
  cnk::LevelStreamArgs a;
  a.y = s->wav_in.rs_wav[c.rs_q]; a.y_ld = c.common ? c.samples[0] : c.seg * c.hop;
  a.x = stages ? c.wav_dev : a.y; a.x_ld = stages ? c.wav_ld : a.y_ld;
  a.state = s->in_lv.state; a.state_stride = s->in_lv.stride; a.zcap = CONAN_LEVEL_MAX_BLOCKS + cnk::kLvRingPad;
  a.rows = s->in_lv.sets.rows[q]; a.n = (int)rows.size(); a.f = s->in_lv.filter;
  front.at[kFrLevel] = [s, a](hipStream_t st) { s->profiled("level_stream_kernel", 0.0, st, [&] { cnk::launch_level_stream(a, st); }); };
  front.at[kFrLevelEnd] = [s, q](hipStream_t st) { s->in_lv.sets.end(q, st); };
}

}  // namespace level

void conan_streams::level_init(const cnk::LvFilter& f) {
  rs_stage_init();
  if (in_lv.state) return;
  in_lv.filter = f;
  in_lv.stride = (long long)cnk::lv_state_bytes(CONAN_LEVEL_MAX_BLOCKS + cnk::kLvRingPad);
  in_lv.state = reinterpret_cast<char*>(alloc((size_t)max_slots * in_lv.stride / sizeof(float)));        // stream state (state_bytes)
  in_lv.sets.init(max_slots, allocs);
  in_lv.assign(max_slots);
}

void conan_ctx_level(conan_ctx* ctx, const conan_level_cfg& c, const float* x, int64_t x_ld, int n, const int64_t* samples, float* y, int64_t y_ld,
                     double* trace, int64_t trace_ld, hipStream_t st) {
  using ch::Error;
  level::check_cfg(c, "conan_level");
  if (!c.enabled) throw Error(CONAN_ERR_INVALID, "conan_level: cfg.enabled must be 1");
  if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, "conan_level: n must be in 1 .. 65535");
  cnk::LevelSignalArgs a;
  memset(&a, 0, sizeof(a));
  a.f = level::filter(ctx, "conan_level");
  a.cfg = level::kernel_cfg(c);
  const double fs = 50.0 * ctx->hop;
  std::vector<cnk::LvSigRow> rows((size_t)n);
  std::vector<int> blocks;
  long long most = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t N = samples[i];
    if (N < 1 || N > (1ll << 30)) throw Error(CONAN_ERR_INVALID, "conan_level: samples must be in 1 .. 2^30");
    if (N > x_ld || N > y_ld) throw Error(CONAN_ERR_INVALID, "conan_level: a row is longer than its stride");
    if (trace && (N + a.f.U - 1) / a.f.U > trace_ld) throw Error(CONAN_ERR_INVALID, "conan_level: trace_ld is smaller than a row's update instants");
    cnk::LvSigRow& R = rows[i];
    memset(&R, 0, sizeof(R));
    R.samples = N; R.blk0 = (long long)(blocks.size() / 2);
    for (long long j = 0; level::block_lo(j, fs) < N; ++j) {      // every block that starts inside the row
      blocks.push_back((int)level::block_lo(j, fs)); blocks.push_back((int)std::min<long long>(level::block_hi(j, fs), INT_MAX));
      ++R.nblocks;
    }
    most = std::max<long long>(most, R.nblocks);
  }
  a.zcap = (int)std::min<long long>(most, c.window_blocks) + cnk::kLvRingPad;
  a.state_stride = (long long)cnk::lv_state_bytes(a.zcap);
  const size_t o_rows = 0, o_blocks = o_rows + rows.size() * sizeof(cnk::LvSigRow), table = (o_blocks + blocks.size() * sizeof(int) + 7) & ~(size_t)7;
  const size_t total = table + (size_t)n * a.state_stride;
  char* ws = reinterpret_cast<char*>(ctx->workspace((total + 3) / 4, st));
  char* h = static_cast<char*>(ctx->loud_stage.take(table));
  memcpy(h + o_rows, rows.data(), rows.size() * sizeof(cnk::LvSigRow));
  memcpy(h + o_blocks, blocks.data(), blocks.size() * sizeof(int));
  HIP_CHECK(hipMemcpyAsync(ws, h, table, hipMemcpyHostToDevice, st));
  ctx->loud_stage.sent(st);
  a.x = x; a.x_ld = x_ld; a.y = y; a.y_ld = y_ld; a.n = n;
  a.rows = reinterpret_cast<const cnk::LvSigRow*>(ws + o_rows); a.blocks = reinterpret_cast<const int*>(ws + o_blocks);
  a.state = ws + table;
  a.trace = trace; a.trace_ld = trace_ld;
  cnk::launch_level_signal(a, st);
  HIP_CHECK(hipGetLastError());
}
