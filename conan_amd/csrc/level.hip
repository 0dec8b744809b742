// Streaming leveller (conan_level, conan_streams_set_input_level): the causal BS.1770 leveller that include/conan_hip.h defines
// (conan_level_cfg).  The plan is in kernels.h (LvState, LvCall); lv_chunk is the one routine that level_stream_kernel (a wav-in
// call's rows) and level_signal_kernel (whole signals, one update interval at a time) both call, so the two agree bit for bit.
// The host side of the streaming form is wavio.hip's; conan_ctx_level below is conan_level's body.
#include <climits>
#include <cmath>

#include "host_common.h"

namespace cnk {

struct LvShared {
  float buf[kLvSegs * kLdStride];      // pending tail + the chunk: segment l at l * kLdStride (the loudness kernels' banking)
  double st[kLvSegs * 4];              // the segments' end states, then (scan) start states
  double part[kLvSegs * kLdSlots];     // per segment: the sums over its bins
  int edge[kLvSegs * 4];               // per segment: the block edges strictly inside it, ascending (INT_MAX: none)
  double rsum[kLvThreads];
  int rcnt[kLvThreads];
  float rpk[2 * kLvThreads];
  double g[4];                         // the ramps: {G_{k-1}, G_k} before the instant, {G_{k-1}, G_k} from it on
};

// sum and count over the workgroup in one fixed order: lane sums, then a binary tree over the lanes
__device__ __forceinline__ void lv_reduce(LvShared& sh, double sum, int cnt, double& tsum, int& tcnt) {
  sh.rsum[threadIdx.x] = sum; sh.rcnt[threadIdx.x] = cnt;
  __syncthreads();
  for (int w = kLvThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { sh.rsum[threadIdx.x] = sh.rsum[threadIdx.x] + sh.rsum[threadIdx.x + w]; sh.rcnt[threadIdx.x] += sh.rcnt[threadIdx.x + w]; }
    __syncthreads();
  }
  tsum = sh.rsum[0]; tcnt = sh.rcnt[0];
  __syncthreads();
}

// l = -0.691 + 10 log10 z with the product and the sum rounded separately: no contraction, so every inlined copy computes the same bits
__device__ __forceinline__ double lv_lufs(double z) { return __dadd_rn(-0.691, __dmul_rn(10.0, log10(z))); }

// One chunk of one stream: c.m samples at x (position c.pos0 on) -> y (may be x).  Called by every thread of a kLvThreads workgroup
// with the same arguments; c lives in LDS or in the kernel's arguments.
__device__ void lv_chunk(const LvFilter& f, const LvCfg& cfg, LvState* S, double* zr, double* lr, int zcap, const LvCall& c, const float* x, float* y,
                         LvShared& sh) {
  const int tid = threadIdx.x;
  if (c.pos0 == 0) {      // the first chunk of an utterance starts the meter and the gain (the rings need no clearing)
    if (tid < 4) S->carry[tid] = 0.0;
    if (tid < kLvBlocks) S->acc[tid] = 0.0;
    if (tid == 0) { S->Gm = cfg.g_init; S->Gc = cfg.g_init; S->peak = 0.0; S->stat[0] = -INFINITY; S->stat[1] = cfg.g_init; S->stat[2] = 0.0; S->stat[3] = 0.0; }
    __syncthreads();
  }
  const int tail = (int)(c.pos0 & (kLdSeg - 1)), total = tail + c.m, nseg = total / kLdSeg, rem = total - nseg * kLdSeg;
  // 1. pending tail + chunk into LDS; the peaks before and from the instant on
  const int split = c.inst ? c.u : c.m;
  float pa = 0.f, pb = 0.f;
  for (int i = tid; i < kLvSegs * kLdSeg; i += kLvThreads) {
    float v = 0.f;
    if (i < tail) v = S->tail[i];
    else if (i < total) {
      v = x[i - tail];
      if (i - tail < split) pa = fmaxf(pa, fabsf(v)); else pb = fmaxf(pb, fabsf(v));
    }
    sh.buf[(i >> 7) * kLdStride + (i & (kLdSeg - 1))] = v;
  }
  sh.rpk[2 * tid] = pa; sh.rpk[2 * tid + 1] = pb;
  __syncthreads();
  for (int w = kLvThreads / 2; w > 0; w >>= 1) {
    if (tid < w) { sh.rpk[2 * tid] = fmaxf(sh.rpk[2 * tid], sh.rpk[2 * (tid + w)]); sh.rpk[2 * tid + 1] = fmaxf(sh.rpk[2 * tid + 1], sh.rpk[2 * (tid + w) + 1]); }
    __syncthreads();
  }
  const double peak_a = (double)sh.rpk[0], peak_b = (double)sh.rpk[1];
  // 2. the complete segments
  if (nseg > 0) {
    const float* w = sh.buf + tid * kLdStride;
    if (tid < nseg) {      // state pass
      double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
      for (int t = 0; t < kLdSeg; ++t) (void)ld_step(f.shelf, f.hp, s, (double)w[t]);
      sh.st[4 * tid] = s[0]; sh.st[4 * tid + 1] = s[1]; sh.st[4 * tid + 2] = s[2]; sh.st[4 * tid + 3] = s[3];
    }
    __syncthreads();
    if (tid == 0) {        // scan from the carried state
      double cs[4] = {S->carry[0], S->carry[1], S->carry[2], S->carry[3]};
      for (int j = 0; j < nseg; ++j) {
        const double e[4] = {sh.st[4 * j], sh.st[4 * j + 1], sh.st[4 * j + 2], sh.st[4 * j + 3]};
        sh.st[4 * j] = cs[0]; sh.st[4 * j + 1] = cs[1]; sh.st[4 * j + 2] = cs[2]; sh.st[4 * j + 3] = cs[3];
        double nx[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) nx[r] = fma(f.M[4 * r + 3], cs[3], fma(f.M[4 * r + 2], cs[2], fma(f.M[4 * r + 1], cs[1], fma(f.M[4 * r], cs[0], e[r]))));
        cs[0] = nx[0]; cs[1] = nx[1]; cs[2] = nx[2]; cs[3] = nx[3];
      }
      S->carry[0] = cs[0]; S->carry[1] = cs[1]; S->carry[2] = cs[2]; S->carry[3] = cs[3];
    }
    __syncthreads();
    if (tid < nseg) {      // energy pass: the segment's bins between the block edges inside it
      const int t0 = tid * kLdSeg;
      int e0 = INT_MAX, e1 = INT_MAX, e2 = INT_MAX;
      for (int b = 0; b < 2 * c.nblk; ++b) {
        const int v = b < c.nblk ? c.lo[b] : c.hi[b - c.nblk];
        if (v <= t0 || v >= t0 + kLdSeg || v == e0 || v == e1 || v == e2) continue;
        if (v < e0) { e2 = e1; e1 = e0; e0 = v; }
        else if (v < e1) { e2 = e1; e1 = v; }
        else if (v < e2) e2 = v;
      }
      sh.edge[4 * tid] = e0; sh.edge[4 * tid + 1] = e1; sh.edge[4 * tid + 2] = e2; sh.edge[4 * tid + 3] = INT_MAX;
      double s[4] = {sh.st[4 * tid], sh.st[4 * tid + 1], sh.st[4 * tid + 2], sh.st[4 * tid + 3]};
      double* part = sh.part + tid * kLdSlots;
      part[1] = 0.0; part[2] = 0.0; part[3] = 0.0;
      int k = 0, next = e0;
      double acc = 0.0;
#pragma unroll 4
      for (int t = 0; t < kLdSeg; ++t) {
        if (t0 + t == next) {      // rare: at most kLdSlots - 1 times per segment
          part[k] = acc;
          ++k; acc = 0.0;
          next = k == 1 ? e1 : (k == 2 ? e2 : INT_MAX);
        }
        const double yv = ld_step(f.shelf, f.hp, s, (double)w[t]);
        acc = fma(yv, yv, acc);
      }
      part[k] = acc;
    }
    __syncthreads();
    if (tid < c.nblk) {    // block tid: the segments in ascending order, each segment's bins inside the block in ascending order
      const int lo = c.lo[tid], hi = c.hi[tid], j = c.j0 + tid;
      double a = S->acc[j % kLvBlocks];
      for (int s = 0; s < nseg; ++s) {
        const int t0 = s * kLdSeg, t1 = t0 + kLdSeg;
        if (hi <= t0 || lo >= t1) continue;
        double p = 0.0; bool any = false;
        int bs = t0;
        for (int k = 0; k < kLdSlots && bs < t1; ++k) {
          const int be = min(sh.edge[4 * s + k], t1);
          if (bs >= lo && be <= hi) { p = any ? p + sh.part[s * kLdSlots + k] : sh.part[s * kLdSlots + k]; any = true; }
          bs = be;
        }
        if (any) a += p;
      }
      if (hi <= nseg * kLdSeg) {      // the block is complete
        const double z = a / f.block_len;
        zr[j % zcap] = z; lr[j % zcap] = lv_lufs(z);
        a = 0.0;
      }
      S->acc[j % kLvBlocks] = a;
    }
  }
  // 3. the new pending tail (every read of the old one is behind the barriers above)
  if (tid < rem) S->tail[tid] = sh.buf[nseg * kLdStride + tid];
  __syncthreads();
  // 4. the update instant: gate the window, form G_k
  if (c.inst) {
    const int first = max(0, c.J - cfg.window), cnt = c.J - first;
    double sum = 0.0; int n = 0;
    for (int i = tid; i < cnt; i += kLvThreads) {
      const int q = (first + i) % zcap;
      if (lr[q] >= -70.0) { sum += zr[q]; ++n; }
    }
    double tsum; int tcnt;
    lv_reduce(sh, sum, n, tsum, tcnt);
    double L = -INFINITY;
    if (tcnt > 0) {
      const double rel = __dadd_rn(lv_lufs(tsum / (double)tcnt), -10.0);
      sum = 0.0; n = 0;
      for (int i = tid; i < cnt; i += kLvThreads) {
        const int q = (first + i) % zcap;
        const double l = lr[q];
        if (l > rel && l > -70.0) { sum += zr[q]; ++n; }
      }
      lv_reduce(sh, sum, n, tsum, tcnt);
      if (tcnt > 0) L = lv_lufs(tsum / (double)tcnt);
    }
    if (tid == 0) {
      const double P = fmax(S->peak, peak_a), Gp = S->Gc;
      double G = Gp;
      if (L != -INFINITY) G = pow(10.0, fmin(fmax(cfg.target - L, -cfg.cut), cfg.boost) / 20.0);
      if (cfg.peak_limit && G * P > 1.0) G = 1.0 / P;
      sh.g[0] = S->Gm; sh.g[1] = Gp; sh.g[2] = Gp; sh.g[3] = G;
      S->Gm = Gp; S->Gc = G;
      S->stat[0] = L; S->stat[1] = G; S->stat[2] = P; S->stat[3] = (double)c.J;
    }
  } else if (tid == 0) {
    sh.g[0] = S->Gm; sh.g[1] = S->Gc; sh.g[2] = sh.g[0]; sh.g[3] = sh.g[1];
  }
  if (tid == 0) S->peak = fmax(S->peak, fmax(peak_a, peak_b));
  __syncthreads();
  // 5. the ramps: g_t = G_{k-1} + (G_k - G_{k-1}) * ((t - u_k + 1) / U), two roundings; y = f32(f64(x) * g_t), one rounding
  const int off = (int)(c.pos0 % f.U);      // samples of the interval that came before this chunk
  const double U = (double)f.U;
  for (int t = tid; t < c.m; t += kLvThreads) {
    const bool after = c.inst && t >= c.u;
    const double gm = after ? sh.g[2] : sh.g[0], gc = after ? sh.g[3] : sh.g[1];
    const double frac = (double)(after ? t - c.u + 1 : off + t + 1) / U;
    const double g = __dadd_rn(gm, __dmul_rn(gc - gm, frac));
    const int i = tail + t;
    float v = (float)__dmul_rn((double)sh.buf[(i >> 7) * kLdStride + (i & (kLdSeg - 1))], g);
    if (cfg.clip) v = fminf(fmaxf(v, -1.f), 1.f);
    y[t] = v;
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

constexpr double kTg = 0.4, kStep = 0.25;      // the meter's gating block length (s) and step (conan_loud_norm's)

long long block_lo(long long j, double fs) { return (long long)(kTg * ((double)j * kStep) * fs); }
long long block_hi(long long j, double fs) { return (long long)(kTg * ((double)j * kStep + 1.0) * fs); }

// J = the number of blocks with hi_j <= p (hi_j never decreases with j)
long long blocks_ended(long long p, double fs) {
  long long j = std::max(0ll, (long long)((double)p / (kTg * kStep * fs)) - 8);
  while (j > 0 && block_hi(j - 1, fs) > p) --j;
  while (block_hi(j, fs) <= p) ++j;
  return j;
}

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

// The chunk [pos0, pos0 + m) of a stream at rate fs with update interval U: its instant and the blocks over its complete segments.
cnk::LvCall plan_call(long long pos0, int m, int U, double fs) {
  cnk::LvCall c;
  memset(&c, 0, sizeof(c));
  c.pos0 = pos0; c.m = m;
  const long long uk = (pos0 + U - 1) / U * U;      // the first instant at or behind pos0
  if (uk < pos0 + m) {
    const long long J = blocks_ended(uk, fs);
    if (J > INT_MAX) throw ch::Error(CONAN_ERR_UNSUPPORTED, "input level: the stream is too long");
    c.inst = 1; c.u = (int)(uk - pos0); c.J = (int)J;
  }
  const long long base = pos0 - (pos0 & (cnk::kLdSeg - 1)), end = base + (pos0 - base + m) / cnk::kLdSeg * cnk::kLdSeg;
  if (end > base) {
    const long long j0 = blocks_ended(base, fs);
    int nb = 0;
    while (block_lo(j0 + nb, fs) < end) {
      if (nb == cnk::kLvBlocks) throw ch::Error(CONAN_ERR_UNSUPPORTED, "input level: too many gating blocks over one call");
      c.lo[nb] = (int)(block_lo(j0 + nb, fs) - base); c.hi[nb] = (int)(block_hi(j0 + nb, fs) - base);
      ++nb;
    }
    if (j0 + nb > INT_MAX) throw ch::Error(CONAN_ERR_UNSUPPORTED, "input level: the stream is too long");
    c.j0 = (int)j0; c.nblk = nb;
  }
  return c;
}

}  // namespace level

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
