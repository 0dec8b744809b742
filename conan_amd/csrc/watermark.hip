// Output watermark (include/conan_hip.h, conan_watermark_cfg): the embedder's kernel, the detector's two, the whole-signal entry
// points conan_watermark_embed / conan_watermark_detect, the host's conan_watermark_decide and the host side of
// conan_streams_set_watermark.  The vocoder step of a marked row launches the embedder behind the comfort fill and in front of the
// output resampler (streams.hip, hifigan_step); out_plan (wavio.hip) builds and checks the rows before anything changes.
#include <climits>
#include <cmath>

#include "streams.h"
#include "hash_dev.h"
#include "sample_dev.h"

namespace cnk {

constexpr int kWmPer = 8, kWmTile = kWmThreads * kWmPer, kWmTileSubs = kWmTile / kWmSub;
static_assert(kWmSub == 8 * kWmPer, "eight lanes own a sub-block");

// One workgroup per row; a row is walked in tiles of 2048 samples, eight consecutive samples per thread: two 16-byte loads and stores
// where the thread's samples are whole and aligned (always, in a vocoder step whose hop is a multiple of 8), single words at clamped
// addresses otherwise (a sample past the row is loaded again, never stored).  The eight lanes of a sub-block reduce its maximum in the
// wave; the envelope's recursion over the tile's sub-blocks is serial, so thread 0 runs it once and hands the amplitudes over through
// LDS.  A thread's eight samples touch at most three chips: three hashes, not eight.  The state record is read once, by every thread,
// in front of an unconditional barrier, and written by thread 0 behind the row's last tile: seed and state_out may be one record.
__global__ __launch_bounds__(kWmThreads) void watermark_embed_kernel(const WmEmbedArgs a) {
  __shared__ float sh_p[kWmTileSubs], sh_a[kWmTileSubs];
  const int i = blockIdx.x, tid = threadIdx.x;
  const WmRow r = a.tab[i];               // uniform in the workgroup
  if (!r.on) return;                      // the row keeps its bits
  const int n = r.samples;
  const float* x = a.x + (long long)i * a.ld;
  float* y = a.y + (long long)i * a.ld_y;
  // (the record is always somewhere: the slot's, the call's seed row, or the table row's own; a restart is selected behind the load)
  const WmState* src = r.slot >= 0 ? a.state + r.slot : (a.seed ? a.seed + i : &a.tab[i].seed);
  WmState s = *src;
  if (r.reseed) s = r.seed;
  __syncthreads();
  float env = s.env;
  const unsigned long long pos = (unsigned long long)s.pos;
  for (int t0 = 0; t0 < n; t0 += kWmTile) {
    const int j0 = t0 + tid * kWmPer;
    const bool vec = j0 + kWmPer - 1 < n && ((reinterpret_cast<uintptr_t>(x + j0) | reinterpret_cast<uintptr_t>(y + j0)) & 15) == 0;
    float v[kWmPer];
    if (vec) {
      const float4 q0 = *reinterpret_cast<const float4*>(x + j0);
      const float4 q1 = *reinterpret_cast<const float4*>(x + j0 + 4);
      v[0] = q0.x; v[1] = q0.y; v[2] = q0.z; v[3] = q0.w; v[4] = q1.x; v[5] = q1.y; v[6] = q1.z; v[7] = q1.w;
    } else {
#pragma unroll
      for (int e = 0; e < kWmPer; ++e) v[e] = x[j0 + e < n ? j0 + e : n - 1];
    }
    float p = 0.f;
#pragma unroll
    for (int e = 0; e < kWmPer; ++e) p = fmaxf(p, j0 + e < n ? fabsf(v[e]) : 0.f);
    p = fmaxf(p, __shfl_xor(p, 1)); p = fmaxf(p, __shfl_xor(p, 2)); p = fmaxf(p, __shfl_xor(p, 4));
    if ((tid & 7) == 0) sh_p[tid >> 3] = p;
    __syncthreads();
    if (tid == 0) {
      const int left = n - t0, nsub = left >= kWmTile ? kWmTileSubs : (left + kWmSub - 1) / kWmSub;
      for (int b = 0; b < nsub; ++b) {
        env = fmaxf(sh_p[b], __fmul_rn(env, 0.875f));
        sh_a[b] = fmaxf(__fmul_rn(env, r.gain), r.floor);
      }
    }
    __syncthreads();
    if (j0 < n) {
      const float amp = sh_a[tid >> 3];
      const unsigned long long P = pos + (unsigned long long)j0;      // the utterance position of the thread's first sample
      const unsigned c0 = (unsigned)(P >> 2);
      bool cb[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) cb[k] = (hash64(r.key, (c0 + k) & (kWmChips - 1)) >> 63) != 0;
      const unsigned w0 = (unsigned)((P >> 11) % kWmWord), w1 = w0 + 1 == kWmWord ? 0 : w0 + 1;
      const bool wb0 = (r.word >> w0) & 1u, wb1 = (r.word >> w1) & 1u;
      const unsigned in_chip = (unsigned)P & 3u, in_blk = (unsigned)P & (kWmBlk - 1);
      float o[kWmPer];
#pragma unroll
      for (int e = 0; e < kWmPer; ++e) {
        const bool c = cb[(in_chip + e) >> 2], w = in_blk + e >= (unsigned)kWmBlk ? wb1 : wb0;
        o[e] = __fadd_rn(v[e], c == w ? amp : -amp);
      }
      if (vec) {
        *reinterpret_cast<float4*>(y + j0) = make_float4(o[0], o[1], o[2], o[3]);
        *reinterpret_cast<float4*>(y + j0 + 4) = make_float4(o[4], o[5], o[6], o[7]);
      } else {
#pragma unroll
        for (int e = 0; e < kWmPer; ++e) if (j0 + e < n) y[j0 + e] = o[e];
      }
    }
  }
  if (tid == 0) {
    WmState out;
    out.pos = (long long)(pos + (unsigned long long)n); out.env = env; out.reserved = 0;
    if (r.slot >= 0) a.state[r.slot] = out;
    if (r.state_row >= 0) a.state_out[r.state_row] = out;
  }
}

// Grid (offset tile, block, row); a row's blocks past its own K return at once (uniform).  Staging: the 16-bit view of the samples
// [k BLK - 1, k BLK + 2 BLK + 3) goes to LDS, one unconditional load_sample per entry at a clamped index (the value of an index
// outside the row is selected behind the load: 0); then every thread forms 16 values of u in registers, adds their |d| to the
// workgroup's sum - at most 4096 * 31 * 32768 < 2^32 - and, behind a barrier, writes u over the view.  The 512 chip signs are eight
// 64-bit ballots, read as scalars.  A thread owns two offsets 256 apart: the lanes of a wave read consecutive words of LDS.
__global__ __launch_bounds__(kWmThreads) void watermark_corr_kernel(const WmDetectArgs a) {
  constexpr int kView = 2 * kWmBlk + 4, kPerThread = 2 * kWmBlk / kWmThreads;
  __shared__ int sh_u[kView + 4];
  __shared__ unsigned long long sh_mask[kWmChips / 64];
  __shared__ unsigned sh_abs;
  const int row = blockIdx.z, k = blockIdx.y, o0 = blockIdx.x * kWmCorrOffsets, tid = threadIdx.x;
  const WmDetRow r = a.tab[row];          // uniform in the workgroup
  if (k >= r.blocks) return;
  const char* x = static_cast<const char*>(a.x) + (long long)row * a.ld * 4;
  const long long n = r.samples, base = (long long)k * kWmBlk;
  if (tid == 0) sh_abs = 0;
#pragma unroll
  for (int h = 0; h < kWmChips / kWmThreads; ++h) {
    const int m = tid + h * kWmThreads;
    const unsigned long long mask = __ballot((hash64(a.key, (unsigned long long)m) >> 63) != 0);
    if ((tid & 63) == 0) sh_mask[m >> 6] = mask;
  }
  for (int t = tid; t < kView; t += kWmThreads) {
    const long long g = base - 1 + t, gc = g < 0 ? 0 : (g > n - 1 ? n - 1 : g);
    const int q = (int)(short)encode_sample(kFmtS16, load_sample(a.fmt, x, gc));      // (a decoded code times 32768 is the code's integer)
    sh_u[t] = g < 0 || g >= n ? 0 : q;
  }
  __syncthreads();
  int u[kPerThread];
  unsigned mine = 0;
#pragma unroll
  for (int e = 0; e < kPerThread; ++e) {
    const int t = tid + e * kWmThreads;      // u[t] and d[t] of the window: q[j] is sh_u[j + 1]
    const int q0 = sh_u[t], q1 = sh_u[t + 1], q2 = sh_u[t + 2], q3 = sh_u[t + 3], q4 = sh_u[t + 4];
    const int d = 16 * q1 - 15 * q0;
    u[e] = 16 * (q1 + q2 + q3 + q4) - 15 * (q0 + q1 + q2 + q3);
    mine += (unsigned)(d < 0 ? -d : d);
  }
#pragma unroll
  for (int sft = 32; sft >= 1; sft >>= 1) mine += __shfl_xor(mine, sft);
  __syncthreads();
  if ((tid & 63) == 0) atomicAdd(&sh_abs, mine);
#pragma unroll
  for (int e = 0; e < kPerThread; ++e) sh_u[tid + e * kWmThreads] = u[e];
  __syncthreads();
  const int oa = o0 + tid, ob = oa + kWmThreads;      // ob + 4 * 511 <= 4091
  int ra = 0, rb = 0;
  for (int w = 0; w < kWmChips / 64; ++w) {
    const unsigned long long mk = sh_mask[w];
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)mk), hi = __builtin_amdgcn_readfirstlane((unsigned)(mk >> 32));
#pragma unroll 8
    for (int b = 0; b < 64; ++b) {
      const int m = w * 64 + b;
      const bool plus = ((b < 32 ? lo >> b : hi >> (b - 32)) & 1u) != 0;
      const int ua = sh_u[oa + 4 * m], ub = sh_u[ob + 4 * m];
      ra += plus ? ua : -ua;
      rb += plus ? ub : -ub;
    }
  }
  const unsigned total = sh_abs;
  const int nk = total ? 32 - __clz((int)total) : 1;      // bit_length, at least 1
  int* out = a.rn + ((long long)row * a.kmax + k) * kWmBlk;
  const long long ma = ra < 0 ? -(long long)ra : (long long)ra, mb = rb < 0 ? -(long long)rb : (long long)rb;
  const int na = (int)((ma << 12) >> nk), nb = (int)((mb << 12) >> nk);
  out[oa] = ra < 0 ? -na : na;
  out[ob] = rb < 0 ? -nb : nb;
}

// One workgroup per row: S[o] over the row's blocks in index order (integers: any order gives the same bits), the argmax with the
// lowest index on ties, the soft bits at it, the record.  A row without blocks reads nothing and reports zeros.
__global__ __launch_bounds__(kWmThreads) void watermark_peak_kernel(const WmDetectArgs a) {
  __shared__ long long sh_v[kWmThreads];
  __shared__ int sh_i[kWmThreads];
  const int row = blockIdx.x, tid = threadIdx.x;
  const WmDetRow r = a.tab[row];
  const int K = r.blocks;
  const int* rn = a.rn + (long long)row * a.kmax * kWmBlk;
  long long best = -1;
  int at = 0;
  for (int e = 0; e < kWmBlk / kWmThreads; ++e) {
    const int o = e * kWmThreads + tid;
    long long S = 0;
    for (int k = 0; k < K; ++k) {
      const int v = rn[(long long)k * kWmBlk + o];
      S += v < 0 ? -v : v;
    }
    a.score[(long long)row * kWmBlk + o] = S;
    if (S > best) { best = S; at = o; }      // (a thread's offsets ascend: the first of equals stays)
  }
  sh_v[tid] = best; sh_i[tid] = at;
  __syncthreads();
  for (int h = kWmThreads / 2; h >= 1; h >>= 1) {
    if (tid < h) {
      const long long v = sh_v[tid + h];
      const int j = sh_i[tid + h];
      if (v > sh_v[tid] || (v == sh_v[tid] && j < sh_i[tid])) { sh_v[tid] = v; sh_i[tid] = j; }
    }
    __syncthreads();
  }
  const int o = sh_i[0];
  for (int k = tid; k < a.kmax; k += kWmThreads) a.soft[(long long)row * a.soft_ld + k] = k < K ? (long long)rn[(long long)k * kWmBlk + o] : 0;
  if (tid == 0) {
    WmHit h;
    h.offset = K ? o : 0; h.blocks = K; h.peak = K ? sh_v[0] : 0;
    a.hit[row] = h;
  }
}

void launch_watermark_embed(const WmEmbedArgs& a, hipStream_t st) {
  if (a.n < 1) return;
  hipLaunchKernelGGL(watermark_embed_kernel, dim3((unsigned)a.n), dim3(kWmThreads), 0, st, a);
}

void launch_watermark_corr(const WmDetectArgs& a, hipStream_t st) {
  if (a.n < 1 || a.kmax < 1) return;
  hipLaunchKernelGGL(watermark_corr_kernel, dim3(kWmBlk / kWmCorrOffsets, (unsigned)a.kmax, (unsigned)a.n), dim3(kWmThreads), 0, st, a);
}

void launch_watermark_peak(const WmDetectArgs& a, hipStream_t st) {
  if (a.n < 1) return;
  hipLaunchKernelGGL(watermark_peak_kernel, dim3((unsigned)a.n), dim3(kWmThreads), 0, st, a);
}

}  // namespace cnk

namespace wmark {

static_assert(sizeof(conan_watermark_cfg) == 64, "two 32-bit fields, the key, three fields and nine reserved words");
static_assert(sizeof(conan_watermark_state) == sizeof(cnk::WmState), "the kernels' state is the header's");
static_assert(sizeof(conan_watermark_hit) == sizeof(cnk::WmHit), "the kernels' record is the header's");
static_assert(sizeof(conan_watermark_result) == 40, "six 32-bit fields, the score and z");
static_assert(31ll * 32768 * 4 * cnk::kWmChips < (1ll << 31), "the correlation fits int32");
static_assert(2ll * cnk::kWmBlk * 31 * 32768 < (1ll << 32), "the window's sum of |d| fits 32 bits");
constexpr int kMarker = 0xB5;      // 1,0,1,1,0,1,0,1, the first block in the top bit
constexpr int64_t kMaxDetectSamples = (int64_t)1 << 26, kMaxDetectWorkspace = (int64_t)1 << 31;

void check_cfg(const conan_watermark_cfg& c, const char* who) {
  const std::string w = std::string(who) + ": ";
  auto bad = [&](const char* what) { throw Error(CONAN_ERR_INVALID, w + what); };
  if (c.enabled != 0 && c.enabled != 1) bad("conan_watermark_cfg.enabled must be 0 or 1");
  if (!c.enabled) return;      // (the other fields are ignored)
  if (c.reseed != 0 && c.reseed != 1) bad("reseed must be 0 or 1");
  if (c.id < 0 || c.id > 65535) bad("id must be in 0 .. 65535");
  if (!std::isfinite(c.gain) || c.gain < 0.f || c.gain > 1.f) bad("gain must be finite and in 0 .. 1");
  if (!std::isfinite(c.floor) || c.floor < 0.f || c.floor > 1.f) bad("floor must be finite and in 0 .. 1");
  for (int v : c.reserved) if (v != 0) bad("the reserved words must be 0");
}

// bit b of the row's word: block b of a word carries +1 (the marker, then the id, MSB first)
static unsigned word_bits(int id) {
  const unsigned w24 = ((unsigned)kMarker << 16) | (unsigned)id;      // block 0 in bit 23
  unsigned out = 0;
  for (int b = 0; b < cnk::kWmWord; ++b) out |= ((w24 >> (cnk::kWmWord - 1 - b)) & 1u) << b;
  return out;
}

cnk::WmRow row(const conan_watermark_cfg& c) {
  cnk::WmRow r;
  memset(&r, 0, sizeof(r));
  r.key = c.key; r.gain = c.gain; r.floor = c.floor; r.word = word_bits(c.id);
  r.on = 1; r.reseed = 1; r.slot = -1; r.state_row = -1;
  return r;
}

std::vector<cnk::WmRow> step_rows(const conan_streams* s, const int32_t* slots, int n, int frames, const std::string& who) {
  std::vector<cnk::WmRow> rows;
  if (s->wm.n_on < 1 || frames < 1) return rows;
  bool any = false;
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] >= s->max_slots) throw Error(CONAN_ERR_INVALID, "slot index out of range");
    any = any || s->wm.on(slots[i]);
  }
  if (!any) return rows;
  if (s->ctx->cfg.voc_upsample == 2) throw Error(CONAN_ERR_UNSUPPORTED, who + ": a slot marks its output (conan_streams_set_watermark): upsample 'nn' runs whole prefixes, not update intervals");
  const long long T = (long long)frames * s->ctx->hop;
  if (T % cnk::kWmSub) throw Error(CONAN_ERR_UNSUPPORTED, who + ": a marked row is a whole number of 64-sample sub-blocks (the hop is not a multiple of 64)");
  rows.resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    cnk::WmRow& r = rows[i];
    memset(&r, 0, sizeof(r));
    r.slot = slots[i]; r.state_row = -1;
    if (!s->wm.on(slots[i])) continue;
    r = row(s->wm.cfg[slots[i]]);
    r.slot = slots[i]; r.reseed = s->wm.pending[slots[i]]; r.samples = (int)T;
  }
  return rows;
}

void embed(conan_ctx* ctx, const conan_watermark_cfg* cfg, const float* x_dev, int n, const int64_t* samples, int64_t ld, const conan_watermark_state* seed_dev,
           float* out_dev, conan_watermark_state* state_out_dev, void* stream) {
  if (!ctx || !cfg || !x_dev || !samples || !out_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_watermark_embed");
  if (!cfg->enabled) throw Error(CONAN_ERR_INVALID, "conan_watermark_embed: cfg.enabled must be 1");
  if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, "conan_watermark_embed: n must be in 1 .. 65535");
  if (ld < 0 || ld > ((int64_t)1 << 40)) throw Error(CONAN_ERR_INVALID, "conan_watermark_embed: ld must be in 0 .. 2^40");
  if (((uintptr_t)seed_dev | (uintptr_t)state_out_dev) & 7) throw Error(CONAN_ERR_INVALID, "conan_watermark_embed: seed_dev and state_out_dev must be 8-byte aligned");
  for (int i = 0; i < n; ++i)
    if (samples[i] < 0 || samples[i] > INT_MAX || samples[i] > ld)
      throw Error(CONAN_ERR_INVALID, "conan_watermark_embed: row " + std::to_string(i) + ": samples must be in 0 .. 2^31 - 1 and fit the row stride ld");
  HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t table = (size_t)n * sizeof(cnk::WmRow);
  cnk::WmRow* h = static_cast<cnk::WmRow*>(ctx->loud_stage.take(table));
  const cnk::WmRow proto = row(*cfg);
  for (int i = 0; i < n; ++i) {
    h[i] = proto;
    h[i].samples = (int)samples[i]; h[i].reseed = seed_dev ? 0 : 1; h[i].state_row = state_out_dev ? i : -1;
  }
  char* ws = reinterpret_cast<char*>(ctx->workspace((table + 3) / sizeof(float), st));
  HIP_CHECK(hipMemcpyAsync(ws, h, table, hipMemcpyHostToDevice, st));
  ctx->loud_stage.sent(st);
  cnk::WmEmbedArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x_dev; a.y = out_dev; a.ld = ld; a.ld_y = ld; a.seed = reinterpret_cast<const cnk::WmState*>(seed_dev);
  a.state_out = reinterpret_cast<cnk::WmState*>(state_out_dev); a.tab = reinterpret_cast<const cnk::WmRow*>(ws); a.n = n;
  cnk::launch_watermark_embed(a, st);
  HIP_CHECK(hipGetLastError());
}

void detect(conan_ctx* ctx, uint64_t key, int format, const void* x_dev, int64_t ld, int n, const int64_t* samples, int64_t* score_dev, int64_t* soft_dev,
            int64_t soft_ld, conan_watermark_hit* hit_dev, void* stream) {
  if (!ctx || !x_dev || !samples || !score_dev || !soft_dev || !hit_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  wavio::check_format(format, "conan_watermark_detect");
  if (n < 1 || n > 4096) throw Error(CONAN_ERR_INVALID, "conan_watermark_detect: n must be in 1 .. 4096");
  if (ld < 0 || ld > ((int64_t)1 << 40)) throw Error(CONAN_ERR_INVALID, "conan_watermark_detect: ld must be in 0 .. 2^40");
  if ((uintptr_t)x_dev & 3) throw Error(CONAN_ERR_INVALID, "conan_watermark_detect: x_dev must be 4-byte aligned");
  if (((uintptr_t)score_dev | (uintptr_t)soft_dev | (uintptr_t)hit_dev) & 7) throw Error(CONAN_ERR_INVALID, "conan_watermark_detect: score_dev, soft_dev and hit_dev must be 8-byte aligned");
  const int bps = wavio::bytes_per_sample(format);
  int kmax = 0;
  for (int i = 0; i < n; ++i) {
    if (samples[i] < 0 || samples[i] > kMaxDetectSamples || samples[i] * bps > ld * 4)
      throw Error(CONAN_ERR_INVALID, "conan_watermark_detect: row " + std::to_string(i) + ": samples must be in 0 .. 2^26 and fit the row stride of ld dwords");
    kmax = std::max(kmax, (int)std::max<int64_t>(0, samples[i] / cnk::kWmBlk - 1));
  }
  if (soft_ld < kmax || soft_ld > ((int64_t)1 << 40)) throw Error(CONAN_ERR_INVALID, "conan_watermark_detect: soft_ld must hold the largest row's blocks");
  const int64_t rn_bytes = (int64_t)n * kmax * cnk::kWmBlk * (int64_t)sizeof(int);
  if (rn_bytes > kMaxDetectWorkspace) throw Error(CONAN_ERR_INVALID, "conan_watermark_detect: rows * blocks * 8 KiB exceeds the 2 GiB workspace of one call: split the call");
  HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t table = ((size_t)n * sizeof(cnk::WmDetRow) + 15) & ~(size_t)15;
  cnk::WmDetRow* h = static_cast<cnk::WmDetRow*>(ctx->loud_stage.take(table));
  for (int i = 0; i < n; ++i) { h[i].samples = samples[i]; h[i].blocks = (int)std::max<int64_t>(0, samples[i] / cnk::kWmBlk - 1); h[i].pad_ = 0; }
  char* ws = reinterpret_cast<char*>(ctx->workspace((table + (size_t)rn_bytes) / sizeof(float), st));
  HIP_CHECK(hipMemcpyAsync(ws, h, (size_t)n * sizeof(cnk::WmDetRow), hipMemcpyHostToDevice, st));
  ctx->loud_stage.sent(st);
  cnk::WmDetectArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x_dev; a.ld = ld; a.tab = reinterpret_cast<const cnk::WmDetRow*>(ws); a.n = n; a.kmax = kmax; a.fmt = format; a.key = key;
  a.rn = reinterpret_cast<int*>(ws + table); a.score = reinterpret_cast<long long*>(score_dev); a.soft = reinterpret_cast<long long*>(soft_dev);
  a.soft_ld = soft_ld; a.hit = reinterpret_cast<cnk::WmHit*>(hit_dev);
  cnk::launch_watermark_corr(a, st);
  cnk::launch_watermark_peak(a, st);
  HIP_CHECK(hipGetLastError());
}

void decide(const int64_t* score, const int64_t* soft, const conan_watermark_hit* hit, double threshold, conan_watermark_result* out) {
  if (!hit || !out) throw Error(CONAN_ERR_INVALID, "null argument");
  memset(out, 0, sizeof(*out));
  if (hit->blocks == 0) return;
  if (!score || !soft) throw Error(CONAN_ERR_INVALID, "null argument");
  if (hit->blocks < 0 || hit->offset < 0 || hit->offset >= cnk::kWmBlk) throw Error(CONAN_ERR_INVALID, "conan_watermark_decide: not a record of conan_watermark_detect");
  if (std::isnan(threshold)) throw Error(CONAN_ERR_INVALID, "conan_watermark_decide: threshold is not a number");
  double tot = 0.0;
  for (int o = 0; o < cnk::kWmBlk; ++o) tot += (double)score[o];
  const double mean = tot / cnk::kWmBlk;
  double var = 0.0;
  for (int o = 0; o < cnk::kWmBlk; ++o) { const double e = (double)score[o] - mean; var += e * e; }
  const double sd = std::sqrt(var / cnk::kWmBlk);
  const double z = sd > 0.0 ? ((double)score[hit->offset] - mean) / sd : 0.0;
  int64_t best = 0, best_acc[cnk::kWmWord] = {};
  int best_r = -1;
  for (int r = 0; r < cnk::kWmWord; ++r) {
    int64_t acc[cnk::kWmWord] = {};
    for (int k = 0; k < hit->blocks; ++k) acc[(k + r) % cnk::kWmWord] += soft[k];
    int64_t sc = 0;
    for (int i = 0; i < 8; ++i) sc += ((kMarker >> (7 - i)) & 1) ? acc[i] : -acc[i];
    if (best_r < 0 || sc > best) { best = sc; best_r = r; memcpy(best_acc, acc, sizeof(acc)); }
  }
  int id = 0;
  for (int i = 0; i < 16; ++i) id = (id << 1) | (best_acc[8 + i] > 0 ? 1 : 0);
  out->present = z >= threshold ? 1 : 0; out->id = id; out->offset = hit->offset; out->rotation = best_r; out->blocks = hit->blocks;
  out->marker_score = best; out->z = z;
}

void set_watermark(conan_streams* s, const int32_t* slots, int n, const conan_watermark_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream) {
  if (!s || !slots || !cfg) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_streams_set_watermark");      // (before the handle is touched, before any GPU use)
  if (seed_dev) conan_streams::Watermark::check_rows("conan_streams_set_", "watermark", "", seed_dev, seed_ld);
  if (!(s->ctx->cfg.models & CONAN_MODEL_HIFIGAN)) throw Error(CONAN_ERR_STATE, "conan_streams_set_watermark: context holds no HiFi-GAN model");
  wavio::check_slot_list(s, slots, n);
  if (cfg->enabled && s->ctx->cfg.voc_upsample == 2)
    throw Error(CONAN_ERR_UNSUPPORTED, "conan_streams_set_watermark: upsample 'nn' runs whole prefixes, not update intervals");
  if (cfg->enabled && s->ctx->hop % cnk::kWmSub) throw Error(CONAN_ERR_UNSUPPORTED, "conan_streams_set_watermark: the hop is not a multiple of 64 samples");
  if (!cfg->enabled && !s->wm.allocated()) return;      // a stream-set that never marked: nothing to allocate, nothing to write
  hipStream_t st = s->enter(stream);      // (rows of pipelined steps in flight were built from the old setting, and they write the state)
  s->watermark_init();
  std::vector<char> restarts((size_t)n);
  for (int i = 0; i < n; ++i) restarts[i] = cfg->enabled && (cfg->reseed != 0 || !s->wm.on(slots[i]));
  s->wm.store_restarting(slots, n, *cfg);      // the restart travels in the slot's next step row ...
  // ... or the seed row becomes the state, now (a slot whose state the call keeps: its seed row is not read)
  if (seed_dev) s->wm.seed(slots, n, seed_dev, seed_ld, st, [&](int i) { return restarts[i] != 0; });
}

void state(conan_streams* s, const int32_t* slots, int n, void* rows_dev, int64_t ld, void* stream) {
  record_state(s, &conan_streams::wm, "watermark", slots, n, rows_dev, ld, stream, fresh_zeros);
}

}  // namespace wmark
