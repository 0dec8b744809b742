// Echo cancellation (include/conan_hip.h, conan_echo_cfg): the kernel, the whole-signal entry point conan_echo and the host side of
// conan_streams_set_echo / conan_streams_echo / conan_streams_echo_state.  The canceller runs on the caller's device rows in front of
// the wav-in step calls, in place and in the slot's input format; no step path reads anything of it.
#include <climits>
#include <cstddef>

#include "streams.h"
#include "sample_dev.h"

namespace cnk {

// One sample of the row becomes enc(v).  Halfword and byte stores: the neighbours in the same dword keep their bytes.
__device__ __forceinline__ void echo_put(int fmt, char* row, long long t, float v) {
  if (fmt == kFmtF32) { reinterpret_cast<float*>(row)[t] = v; return; }
  const unsigned c = encode_sample(fmt, v);
  if (fmt == kFmtS16) reinterpret_cast<unsigned short*>(row)[t] = (unsigned short)c;
  else reinterpret_cast<unsigned char*>(row)[t] = (unsigned char)c;
}

// Eight consecutive halfwords of LDS from a halfword-aligned address as one load, four consecutive weights as another
typedef short echo_short8 __attribute__((ext_vector_type(8), aligned(2)));
typedef int echo_int4 __attribute__((ext_vector_type(4), aligned(16)));
// sum over j < 8 of a[j] * x[7 - j] (the filter: taps ascend as the window descends) / of a[j] * x[j] (the gradient)
__device__ __forceinline__ long long echo_dot8_rev(const int* a, const short* x) {
  const echo_int4 a0 = *reinterpret_cast<const echo_int4*>(a), a1 = *reinterpret_cast<const echo_int4*>(a + 4);
  const echo_short8 v = *reinterpret_cast<const echo_short8*>(x);
  return (long long)a0.x * v[7] + (long long)a0.y * v[6] + (long long)a0.z * v[5] + (long long)a0.w * v[4] +
         (long long)a1.x * v[3] + (long long)a1.y * v[2] + (long long)a1.z * v[1] + (long long)a1.w * v[0];
}
__device__ __forceinline__ long long echo_dot8(const int* a, const short* x) {
  const echo_int4 a0 = *reinterpret_cast<const echo_int4*>(a), a1 = *reinterpret_cast<const echo_int4*>(a + 4);
  const echo_short8 v = *reinterpret_cast<const echo_short8*>(x);
  return (long long)a0.x * v[0] + (long long)a0.y * v[1] + (long long)a0.z * v[2] + (long long)a0.w * v[3] +
         (long long)a1.x * v[4] + (long long)a1.y * v[5] + (long long)a1.z * v[6] + (long long)a1.w * v[7];
}

__device__ __forceinline__ long long echo_wave_sum(long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)((unsigned long long)v >> 32), m);
    v += (long long)(((unsigned long long)hi << 32) | lo);
  }
  return v;
}
__device__ __forceinline__ int echo_wave_max(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m));
  return v;
}

// LDS (about 27 KB): the weights (8 KB), xf = far history | tile of the far end's 16-bit view (16.5 KB; x[tile0 + i] at xf[kEchoHist + i],
// so x'[t - k] of tile sample i is xf[kEchoHist + i - delay - k], never below index 2), the pending block's e, the four waves' partial
// filter sums, and the block's reduced scalars.  Everything that steers the walk - phase, segment bounds, shift, hcnt, the decisions at
// a block's end - is uniform in the workgroup: every lane computes it from the row and from the same LDS words.
//   Filter pass of a segment (the samples of one block that this tile brings, <= 64): lane = (sample tl, wave wv); wave wv sums taps
//   [wv L/4, (wv+1) L/4) eight at a time: the weights are two broadcast 16-byte loads, the window one 16-byte load at a
//   halfword-aligned address (consecutive lanes, consecutive halfwords).  Wave 0 adds the four partials and emits.
//   Block end: P and xmax (one pass over L + 63 halfwords), the decisions, then per lane L/256 taps of the gradient - e[i] is the
//   broadcast address, x' consecutive - each followed by its int64 division.
__global__ __launch_bounds__(kEchoThreads) void echo_kernel(const EchoArgs a) {
  __shared__ __attribute__((aligned(16))) int w[kEchoMaxTaps];
  __shared__ __attribute__((aligned(16))) short xf[kEchoHist + kEchoTile];
  __shared__ __attribute__((aligned(16))) int ep[kEchoBlock];
  __shared__ long long part[4][kEchoBlock];
  __shared__ long long sD, sE;
  __shared__ unsigned long long sP;
  __shared__ int sdmax, sxmax;
  const int tid = threadIdx.x, tl = tid & 63, wv = tid >> 6;
  if ((int)blockIdx.x >= a.rows) return;
  const EchoRow r = a.tab[blockIdx.x];      // uniform in the workgroup
  char* mic = reinterpret_cast<char*>(a.wav) + (long long)r.row * a.wav_ld * 4;
  const char* far = reinterpret_cast<const char*>(a.far) + (long long)r.row * a.far_ld * 4;
  char* rec = r.slot >= 0 ? a.state + (long long)r.slot * kEchoStateBytes : nullptr;
  const int fmt = r.fmt, L = r.taps, delay = r.delay;

  // ---- the state: the restart state, or the slot's record (only values come from it; shift and hcnt are brought into their ranges)
  const bool load = rec && !r.restart;
  int shift = r.mu_shift, hcnt = 0, ph = r.phase;
  long long adapted = 0, frozen = 0, trips = 0;
  EchoHead h = {};
  if (load) {
    h = *reinterpret_cast<const EchoHead*>(rec);
    shift = min(max(h.shift, 0), kEchoMaxShift); hcnt = max(h.hcnt, 0);
    adapted = h.adapted; frozen = h.frozen; trips = h.trips;
  }
  {
    const int* rw = reinterpret_cast<const int*>(rec + sizeof(EchoHead));
    const int* re = rw + kEchoMaxTaps;
    const short* rh = reinterpret_cast<const short*>(re + kEchoBlock);
    for (int i = tid; i < kEchoMaxTaps; i += kEchoThreads) w[i] = (load && i < L) ? rw[i] : 0;
    if (tid < kEchoBlock) ep[tid] = (load && tid < ph) ? re[tid] : 0;
    for (int i = tid; i < kEchoHist; i += kEchoThreads) xf[i] = load ? rh[i] : (short)0;
    if (tid == 0) {
      const bool pend = load && ph > 0;
      sD = pend ? h.D : 0; sE = pend ? h.E : 0; sdmax = pend ? h.dmax : 0; sP = 0; sxmax = 0;
    }
  }
  long long cD = 0, cE = 0, cad = 0, cfr = 0;      // this call's stats (cD, cE: lane 0's)

  for (long long t0 = 0; t0 < r.samples; t0 += kEchoTile) {
    const int n = (int)(r.samples - t0 < kEchoTile ? r.samples - t0 : kEchoTile);
    for (int i = tid; i < n; i += kEchoThreads) xf[kEchoHist + i] = (short)echo_q(echo_finite(load_sample(fmt, far, t0 + i)));
    __syncthreads();

    int pos = 0;
    while (pos < n) {
      // ---- the segment: what this tile brings of the current block
      const int len = min(n - pos, kEchoBlock - ph);
      float m = 0.f;
      if (wv == 0 && tl < len) m = echo_finite(load_sample(fmt, mic, t0 + pos + tl));      // (in flight under the filter's sums)
      long long S = 0;
      if (tl < len) {
        const int base = kEchoHist + pos + tl - delay;      // x'[t - k] = xf[base - k]; base - k >= kEchoHist - kEchoMaxDelay - (kEchoMaxTaps - 1) > 0
        const int k0 = wv * (L >> 2), k1 = k0 + (L >> 2);
#pragma unroll 2      // eight taps per step (L / 4 is a multiple of 16); integer sums have no order to keep
        for (int k = k0; k < k1; k += 8) S += echo_dot8_rev(&w[k], &xf[base - k - 7]);
      }
      part[wv][tl] = S;
      __syncthreads();
      if (wv == 0) {
        long long d2 = 0, e2 = 0;
        int ad = 0;
        if (tl < len) {
          S = part[0][tl] + part[1][tl] + part[2][tl] + part[3][tl];
          long long yl = (S + (1ll << 23)) >> 24;
          yl = yl < -32768 ? -32768 : (yl > 32767 ? 32767 : yl);
          const int yh = (int)yl, d = echo_q(m), e = d - yh;
          ep[ph + tl] = e;
          if (yh != 0) echo_put(fmt, mic, t0 + pos + tl, __fsub_rn(m, (float)yh * (1.f / 32768.f)));
          d2 = (long long)d * d; e2 = (long long)e * e; ad = d < 0 ? -d : d;
        }
        d2 = echo_wave_sum(d2); e2 = echo_wave_sum(e2); ad = echo_wave_max(ad);
        if (tl == 0) { sD += d2; sE += e2; sdmax = max(sdmax, ad); cD += d2; cE += e2; }
      }
      __syncthreads();
      ph += len; pos += len;
      if (ph < kEchoBlock) continue;

      // ---- the end of a block: its last sample is tile sample pos - 1
      const int top = kEchoHist + pos - 1 - delay;      // x'[b1 - 1 - k] = xf[top - k]; top - (L + 62) >= 2
      const long long D = sD, E = sE;
      const int dmax = sdmax;
      if (E > 4 * D + 4096) {      // the guard
        for (int k = tid; k < L; k += kEchoThreads) w[k] = 0;
        shift = min(shift + 1, kEchoMaxShift); ++trips;
      } else {
        unsigned long long p = 0;
        int xm = 0;
        for (int k = tid; k < L + kEchoBlock - 1; k += kEchoThreads) {
          const int v = xf[top - k];
          xm = max(xm, v < 0 ? -v : v);
          if (k < L) p += (unsigned)(v * v);
        }
        p = (unsigned long long)echo_wave_sum((long long)p); xm = echo_wave_max(xm);
        if (tl == 0) { atomicAdd(&sP, p); atomicMax(&sxmax, xm); }
        __syncthreads();
        const long long P = (long long)sP;
        const int xmax = sxmax;
        const bool cond = r.dt_den > 0 && (long long)dmax * r.dt_den > (long long)xmax * r.dt_num;
        const bool frz = cond || hcnt > 0;
        if (cond) hcnt = r.hang; else if (hcnt > 0) --hcnt;
        if (frz) { ++frozen; ++cfr; }
        else if (P >= r.far_min) {
          const long long den = P + r.reg, mul = 1ll << (24 - shift);
          for (int k = tid; k < L; k += kEchoThreads) {
            const int base = top - (kEchoBlock - 1) - k;      // x'[b0 + i - k] = xf[base + i]; base >= 2
            long long G = 0;
#pragma unroll 2
            for (int i = 0; i < kEchoBlock; i += 8) G += echo_dot8(&ep[i], &xf[base + i]);
            long long nw = (long long)w[k] + (G * mul) / den;
            nw = nw < -2147483647ll ? -2147483647ll : (nw > 2147483647ll ? 2147483647ll : nw);
            w[k] = (int)nw;
          }
          ++adapted; ++cad;
        }
      }
      __syncthreads();      // (every lane has read the block's scalars)
      if (tid == 0) { sD = 0; sE = 0; sdmax = 0; sP = 0; sxmax = 0; }
      ph = 0;
      __syncthreads();      // (the next segment's filter reads the new weights; its wave 0 adds to the cleared scalars)
    }

    // ---- the history moves on: the last kEchoHist values, through registers (source and destination overlap when n < kEchoHist)
    constexpr int kPer = (kEchoHist + kEchoThreads - 1) / kEchoThreads;
    short hv[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) { const int i = u * kEchoThreads + tid; hv[u] = i < kEchoHist ? xf[n + i] : (short)0; }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kPer; ++u) { const int i = u * kEchoThreads + tid; if (i < kEchoHist) xf[i] = hv[u]; }
    __syncthreads();
  }

  if (a.stats && tid == 0) {
    long long* o = a.stats + (long long)r.row * 4;
    o[0] = cD; o[1] = cE; o[2] = cad; o[3] = cfr;
  }
  // ---- the state goes back: plain vector stores
  if (rec) {
    if (tid == 0) {
      EchoHead o;
      o.pos = r.pos + r.samples; o.shift = shift; o.hcnt = hcnt; o.adapted = adapted; o.frozen = frozen; o.trips = trips;
      o.D = sD; o.E = sE; o.dmax = sdmax; o.reserved = 0;
      *reinterpret_cast<EchoHead*>(rec) = o;
    }
    int* rw = reinterpret_cast<int*>(rec + sizeof(EchoHead));
    int* re = rw + kEchoMaxTaps;
    short* rh = reinterpret_cast<short*>(re + kEchoBlock);
    for (int i = tid; i < kEchoMaxTaps; i += kEchoThreads) rw[i] = w[i];      // (zeros from L on: never written above)
    if (tid < kEchoBlock) re[tid] = tid < ph ? ep[tid] : 0;
    for (int i = tid; i < kEchoHist; i += kEchoThreads) rh[i] = xf[i];
  }
}

void launch_echo(const EchoArgs& a, hipStream_t st) {
  if (a.rows < 1) return;
  hipLaunchKernelGGL(echo_kernel, dim3(a.rows), dim3(kEchoThreads), 0, st, a);
}

}  // namespace cnk

namespace echo {

static_assert(sizeof(conan_echo_cfg) == 48, "eight int32 and two int64 fields");
static_assert(CONAN_ECHO_BLOCK == cnk::kEchoBlock && CONAN_ECHO_MAX_TAPS == cnk::kEchoMaxTaps && CONAN_ECHO_MAX_DELAY == cnk::kEchoMaxDelay &&
              CONAN_ECHO_MAX_SHIFT == cnk::kEchoMaxShift && CONAN_ECHO_HISTORY == cnk::kEchoHist, "the kernel's limits are the header's");
constexpr int64_t kMaxSamples = 1ll << 40, kMaxStride = 1ll << 40;

void check_cfg(const conan_echo_cfg& c, const char* who) {
  const std::string w = std::string(who) + ": ";
  auto bad = [&](const char* what) { throw Error(CONAN_ERR_INVALID, w + what); };
  if (c.enabled != 0 && c.enabled != 1) bad("conan_echo_cfg.enabled must be 0 or 1");
  if (!c.enabled) return;      // (the other fields are ignored)
  if (c.taps < CONAN_ECHO_BLOCK || c.taps > CONAN_ECHO_MAX_TAPS || c.taps % CONAN_ECHO_BLOCK) bad("taps must be a multiple of 64 in 64 .. CONAN_ECHO_MAX_TAPS");
  if (c.delay < 0 || c.delay > CONAN_ECHO_MAX_DELAY) bad("delay must be in 0 .. CONAN_ECHO_MAX_DELAY");
  if (c.mu_shift < 0 || c.mu_shift > CONAN_ECHO_MAX_SHIFT) bad("mu_shift must be in 0 .. CONAN_ECHO_MAX_SHIFT");
  if (c.dt_num < 0 || c.dt_den < 0) bad("dt_num and dt_den must be >= 0");
  if (c.hang < 0) bad("hang must be >= 0");
  if (c.reg < 1 || c.reg > (1ll << 60)) bad("reg must be in 1 .. 2^60");
  if (c.far_min < 0) bad("far_min must be >= 0");
}

cnk::EchoRow row(const conan_echo_cfg& c) {
  cnk::EchoRow r;
  memset(&r, 0, sizeof(r));
  r.taps = c.taps; r.delay = c.delay; r.mu_shift = c.mu_shift; r.dt_num = c.dt_num; r.dt_den = c.dt_den; r.hang = c.hang; r.reg = c.reg; r.far_min = c.far_min;
  r.slot = -1; r.restart = 1;
  return r;
}

void whole(conan_ctx* ctx, const conan_echo_cfg* cfg, int format, void* x_dev, int64_t ld, const void* far_dev, int64_t far_ld, int n, const int64_t* samples,
           int64_t* stats_dev, void* stream) {
  if (!ctx || !cfg || !x_dev || !far_dev || !samples) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_echo");
  if (!cfg->enabled) throw Error(CONAN_ERR_INVALID, "conan_echo: cfg.enabled must be 1");
  wavio::check_format(format, "conan_echo");
  if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, "conan_echo: n must be in 1 .. 65535");
  if (ld < 0 || ld > kMaxStride || far_ld < 0 || far_ld > kMaxStride) throw Error(CONAN_ERR_INVALID, "conan_echo: ld and far_ld must be in 0 .. 2^40");
  if (((uintptr_t)x_dev & 3) || ((uintptr_t)far_dev & 3)) throw Error(CONAN_ERR_INVALID, "conan_echo: x_dev and far_dev must be 4-byte aligned");
  if ((uintptr_t)stats_dev & 7) throw Error(CONAN_ERR_INVALID, "conan_echo: stats_dev must be 8-byte aligned");
  const int bps = wavio::bytes_per_sample(format);
  for (int i = 0; i < n; ++i) {
    if (samples[i] < 0 || samples[i] > kMaxSamples) throw Error(CONAN_ERR_INVALID, "conan_echo: row " + std::to_string(i) + ": samples must be in 0 .. 2^40");
    if (samples[i] * bps > ld * 4 || samples[i] * bps > far_ld * 4)
      throw Error(CONAN_ERR_INVALID, "conan_echo: row " + std::to_string(i) + " holds more bytes than a row stride (ld, far_ld x 4 bytes)");
  }
  HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t table = (size_t)n * sizeof(cnk::EchoRow);
  cnk::EchoRow* h = static_cast<cnk::EchoRow*>(ctx->loud_stage.take(table));
  const cnk::EchoRow proto = row(*cfg);
  int rows = 0;
  for (int i = 0; i < n; ++i) {
    if (samples[i] < 1) continue;
    h[rows] = proto;
    h[rows].samples = samples[i]; h[rows].row = i; h[rows].fmt = format;
    ++rows;
  }
  if (stats_dev && rows < n) HIP_CHECK(hipMemsetAsync(stats_dev, 0, (size_t)n * 4 * sizeof(int64_t), st));
  if (rows < 1) return;
  char* ws = reinterpret_cast<char*>(ctx->workspace((table + 3) / sizeof(float), st));
  HIP_CHECK(hipMemcpyAsync(ws, h, (size_t)rows * sizeof(cnk::EchoRow), hipMemcpyHostToDevice, st));
  ctx->loud_stage.sent(st);
  cnk::EchoArgs a;
  memset(&a, 0, sizeof(a));
  a.wav = x_dev; a.wav_ld = ld; a.far = far_dev; a.far_ld = far_ld; a.state = nullptr; a.stats = reinterpret_cast<long long*>(stats_dev);
  a.tab = reinterpret_cast<const cnk::EchoRow*>(ws); a.rows = rows;
  cnk::launch_echo(a, st);
  HIP_CHECK(hipGetLastError());
}

static void check_seed(const char* who, const void* p, int64_t ld) {
  if (ld < cnk::kEchoStateBytes || ((uintptr_t)p & 7) || (ld & 7))
    throw Error(CONAN_ERR_INVALID, std::string(who) + ": rows are conan_echo_state_bytes bytes, 8-byte aligned, ld apart");
}

void set_echo(conan_streams* s, const int32_t* slots, int n, const conan_echo_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream) {
  if (!s || !slots || !cfg) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_streams_set_echo");      // (before the handle is touched, before any GPU use)
  if (seed_dev) check_seed("conan_streams_set_echo", seed_dev, seed_ld);
  if (!wavio::begin_setter(s, slots, n, cfg->enabled != 0, s->ec.allocated(), "conan_streams_set_echo", stream)) return;
  hipStream_t st = (hipStream_t)stream;
  s->echo_init();
  // a slot that was off restarts in its next row - or from its seed row, now, which then clears the flag
  s->ec.store(slots, n, *cfg, [&](int i) { s->ec.pending[slots[i]] = 1; });
  if (!cfg->enabled || !seed_dev) return;
  // the host, not the record, tells the kernel where in a block a slot stands: the seeds' positions are read back
  std::vector<long long> pos((size_t)n);
  for (int i = 0; i < n; ++i) {
    const char* src = static_cast<const char*>(seed_dev) + (size_t)i * seed_ld;
    HIP_CHECK(hipMemcpyAsync(s->ec.state + (size_t)slots[i] * cnk::kEchoStateBytes, src, (size_t)cnk::kEchoStateBytes, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(&pos[i], src, sizeof(long long), hipMemcpyDeviceToHost, st));
  }
  HIP_CHECK(hipStreamSynchronize(st));
  for (int i = 0; i < n; ++i) {
    s->ec.pos[slots[i]] = pos[i] < 0 ? 0 : pos[i];      // (a record the kernel cannot have written: any position serves)
    s->ec.pending[slots[i]] = 0;
  }
}

void cancel(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, void* wav_dev, int64_t wav_ld, const void* far_dev, int64_t far_ld,
            int64_t* stats_dev, void* stream) {
  if (!s || !slots || !samples) throw Error(CONAN_ERR_INVALID, "null argument");
  wavio::check_slot_list(s, slots, n);
  if (wav_ld < 0 || wav_ld > kMaxStride || far_ld < 0 || far_ld > kMaxStride) throw Error(CONAN_ERR_INVALID, "conan_streams_echo: wav_ld and far_ld must be in 0 .. 2^40");
  if ((uintptr_t)stats_dev & 7) throw Error(CONAN_ERR_INVALID, "conan_streams_echo: stats_dev must be 8-byte aligned");
  std::vector<cnk::EchoRow> rows;
  for (int i = 0; i < n; ++i) {
    if (samples[i] < 0) throw Error(CONAN_ERR_INVALID, "conan_streams_echo: samples must be >= 0");
    if (!s->ec.on(slots[i]) || samples[i] == 0) continue;      // the row keeps its bytes
    const int fmt = s->wav_in.in_fmt[slots[i]];
    const long long bytes = (long long)samples[i] * wavio::bytes_per_sample(fmt);
    if (bytes > wav_ld * 4 || bytes > far_ld * 4)
      throw Error(CONAN_ERR_INVALID, "conan_streams_echo: slot " + std::to_string(slots[i]) + ": the row holds more bytes than a row stride (wav_ld, far_ld x 4 bytes)");
    cnk::EchoRow r = row(s->ec.cfg[slots[i]]);
    r.restart = s->ec.pending[slots[i]];
    r.pos = r.restart ? 0 : s->ec.pos[slots[i]];
    r.phase = (int)(r.pos % cnk::kEchoBlock);
    r.samples = samples[i]; r.row = i; r.slot = slots[i]; r.fmt = fmt;
    rows.push_back(r);
  }
  hipStream_t st = (hipStream_t)stream;
  if (stats_dev && (int)rows.size() < n && n > 0) {
    HIP_CHECK(hipSetDevice(s->ctx->device));
    HIP_CHECK(hipMemsetAsync(stats_dev, 0, (size_t)n * 4 * sizeof(int64_t), st));
  }
  if (rows.empty()) return;      // no row to cancel: no launch
  if (!wav_dev || !far_dev) throw Error(CONAN_ERR_INVALID, "null argument (wav_dev / far_dev with a row to cancel)");
  if (((uintptr_t)wav_dev & 3) || ((uintptr_t)far_dev & 3)) throw Error(CONAN_ERR_INVALID, "conan_streams_echo: wav_dev and far_dev must be 4-byte aligned");
  HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
  const int q = s->ec.sets.begin(rows.data(), (int)rows.size(), st);
  cnk::EchoArgs a;
  memset(&a, 0, sizeof(a));
  a.wav = wav_dev; a.wav_ld = wav_ld; a.far = far_dev; a.far_ld = far_ld; a.state = s->ec.state; a.stats = reinterpret_cast<long long*>(stats_dev);
  a.tab = s->ec.sets.rows[q]; a.rows = (int)rows.size();
  s->profiled("echo_kernel", 0.0, st, [&] { cnk::launch_echo(a, st); });
  HIP_CHECK(hipGetLastError());
  s->ec.sets.end(q, st);
  for (const cnk::EchoRow& r : rows) { s->ec.pending[r.slot] = 0; s->ec.pos[r.slot] = r.pos + r.samples; }
}

// a slot about to restart reports the restart state; any other its record, in the order of `stream`
void state(conan_streams* s, const int32_t* slots, int n, void* state_dev, int64_t ld, void* stream) {
  if (!s || !slots || !state_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  check_seed("conan_streams_echo_state", state_dev, ld);
  wavio::check_slot_list(s, slots, n);
  for (int i = 0; i < n; ++i)
    if (!s->ec.on(slots[i])) throw Error(CONAN_ERR_STATE, "conan_streams_echo_state: slot " + std::to_string(slots[i]) + " has no echo canceller (conan_streams_set_echo)");
  hipStream_t st = s->enter(stream);
  for (int i = 0; i < n; ++i) {
    char* dst = static_cast<char*>(state_dev) + (size_t)i * ld;
    if (s->ec.pending[slots[i]]) {
      HIP_CHECK(hipMemsetAsync(dst, 0, (size_t)cnk::kEchoStateBytes, st));
      HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(dst + offsetof(cnk::EchoHead, shift)), s->ec.cfg[slots[i]].mu_shift, 1, st));
    } else {
      HIP_CHECK(hipMemcpyAsync(dst, s->ec.state + (size_t)slots[i] * cnk::kEchoStateBytes, (size_t)cnk::kEchoStateBytes, hipMemcpyDeviceToDevice, st));
    }
  }
}

}  // namespace echo

void conan_streams::echo_init() {
  if (ec.state) return;
  ec.state = reinterpret_cast<char*>(alloc((size_t)max_slots * cnk::kEchoStateBytes / sizeof(float)));      // zeroed (counted by state_bytes)
  ec.sets.init(max_slots, allocs);
  state_bytes += (int64_t)kStageSets * max_slots * sizeof(cnk::EchoRow);
  ec.assign(max_slots);
  ec.pos.assign(max_slots, 0);
}
