// Echo cancellation (include/conan_hip.h, conan_echo_cfg): the kernel, the whole-signal entry point conan_echo and the host side of
// conan_streams_set_echo / conan_streams_echo / conan_streams_echo_state.  The canceller runs on the caller's device rows in front of
// the wav-in step calls, in place and in the slot's input format; no step path reads anything of it.
#include <climits>
#include <cstddef>

#include "prestep.h"
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

// The feature's part of the pre-step row call (prestep.h): the second buffer holds the far rows; the report is the call's stats
struct Stage {
  using Cfg = conan_echo_cfg; using Row = cnk::EchoRow; using Args = cnk::EchoArgs;
  struct Call { void* wav; int64_t wav_ld; const void* aux; int64_t aux_ld; int64_t* report; };
  static constexpr const char *kName = "echo", *kWhole = "conan_echo", *kSet = "conan_streams_set_echo", *kCall = "conan_streams_echo";
  static constexpr const char *kAux = "far", *kReportArg = "stats_dev", *kKernel = "echo_kernel";
  static constexpr bool kAuxAudio = true;
  static constexpr int kReport = 4, kBlock = cnk::kEchoBlock;
  static constexpr auto set = &conan_streams::ec;
  static constexpr auto check_cfg = &echo::check_cfg;
  static constexpr auto row = &echo::row;
  static constexpr auto launch = &cnk::launch_echo;
  static const char* check_call(const Call&) { return nullptr; }
  static const char* check_row(const Cfg&, int64_t, const Call&) { return nullptr; }
  static void fill(Args& a, const Call& b) {
    a.wav = b.wav; a.wav_ld = b.wav_ld; a.far = b.aux; a.far_ld = b.aux_ld; a.stats = reinterpret_cast<long long*>(b.report);
  }
};

void whole(conan_ctx* ctx, const conan_echo_cfg* cfg, int format, void* x_dev, int64_t ld, const void* far_dev, int64_t far_ld, int n, const int64_t* samples,
           int64_t* stats_dev, void* stream) {
  prestep::whole<Stage>(ctx, cfg, format, {x_dev, ld, far_dev, far_ld, stats_dev}, n, samples, stream);
}

void set_echo(conan_streams* s, const int32_t* slots, int n, const conan_echo_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream) {
  if (!prestep::begin_set<Stage>(s, slots, n, cfg, seed_dev, seed_ld, stream)) return;
  hipStream_t st = (hipStream_t)stream;
  s->echo_init();
  // a slot that was off restarts in its next row - or from its seed row, now, which then clears the flag
  s->ec.store(slots, n, *cfg, [&](int i) { s->ec.pending[slots[i]] = 1; });
  if (!cfg->enabled || !seed_dev) return;
  s->ec.seed(slots, n, seed_dev, seed_ld, st, [](int) { return true; });
  prestep::read_seed_pos<Stage>(s, slots, n, seed_dev, seed_ld, st);
}

void cancel(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, void* wav_dev, int64_t wav_ld, const void* far_dev, int64_t far_ld,
            int64_t* stats_dev, void* stream) {
  prestep::call<Stage>(s, slots, n, samples, {wav_dev, wav_ld, far_dev, far_ld, stats_dev}, stream);
}

// the restart state: zeros, and the slot's step size
void state(conan_streams* s, const int32_t* slots, int n, void* state_dev, int64_t ld, void* stream) {
  record_state(s, &conan_streams::ec, "echo", slots, n, state_dev, ld, stream, [&](int slot, char* dst, hipStream_t st) {
    HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(dst + offsetof(cnk::EchoHead, shift)), s->ec.cfg[slot].mu_shift, 1, st));
  });
}

}  // namespace echo
