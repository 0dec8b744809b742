// Input loss concealment (include/conan_hip.h, conan_conceal_cfg): the kernel, the whole-signal entry point conan_conceal and the host
// side of conan_streams_set_conceal / conan_streams_conceal / conan_streams_conceal_state.  The repair runs on the caller's device rows
// in front of the wav-in step calls, in place and in the slot's input format; no step path reads anything of it.
#include <climits>

#include "prestep.h"
#include "sample_dev.h"

namespace cnk {

constexpr long long kConcFull = 1ll << 20;

// g = (float)((double)l / 2^20): the quotient is exact in f64, so this is one rounding
__device__ __forceinline__ float conc_gain(long long l) { return (float)((double)l * (1.0 / 1048576.0)); }
// the level of sample k of a run
__device__ __forceinline__ long long conc_level(long long k, long long hold, long long fall) {
  return k < hold ? kConcFull : (k < hold + fall ? ((hold + fall - k) << 20) / fall : 0ll);
}
__device__ __forceinline__ short conc_q(float v) { return (short)encode_sample(kFmtS16, v); }      // the library's f32 -> s16 value

// One sample of the row becomes enc(v); returns dec(enc(v)).  Halfword and byte stores: the received neighbours in the same dword keep
// their bytes, and are never written.
__device__ __forceinline__ float conc_put(int fmt, char* row, long long t, float v) {
  if (fmt == kFmtF32) { reinterpret_cast<float*>(row)[t] = v; return v; }
  const unsigned c = encode_sample(fmt, v);
  if (fmt == kFmtS16) reinterpret_cast<unsigned short*>(row)[t] = (unsigned short)c;
  else reinterpret_cast<unsigned char*>(row)[t] = (unsigned char)c;
  return decode_sample(fmt, c, c);
}

__device__ __forceinline__ unsigned long long conc_min_xor(unsigned long long v, int m) {
  const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
  const unsigned long long o = ((unsigned long long)hi << 32) | lo;
  return o < v ? o : v;
}

// LDS: y = history | tile of the decoded repaired signal (24 KB), q = its s16 view (12 KB: consecutive lags read consecutive
// halfwords, two lanes per bank word, and the newer operand is one broadcast address), the template (4 KB), the tile's packet flags
// (4 KB).  Everything that steers the walk - the state's header, the segment bounds - is uniform in the workgroup: every thread
// computes it from the same LDS words.  Inside a segment the work is one thread per lag or per sample.
__global__ __launch_bounds__(kConcThreads) void conceal_kernel(const ConcArgs a) {
  __shared__ float y[kConcHist + kConcTile];
  __shared__ short q[kConcHist + kConcTile];
  __shared__ float T[kConcMaxLag];
  __shared__ unsigned char fl[kConcTile + 8];
  __shared__ unsigned long long best;
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= a.rows) return;
  const ConcRow r = a.tab[blockIdx.x];      // uniform in the workgroup
  char* row = reinterpret_cast<char*>(a.wav) + (long long)r.row * a.wav_ld * 4;
  const int* lost = a.lost + (long long)r.row * a.lost_ld;
  char* rec = r.slot >= 0 ? a.state + (long long)r.slot * kConcStateBytes : nullptr;
  const int fmt = r.fmt;
  const long long hold = r.hold, fall = r.fall;

  // ---- the state: zeros, or the slot's record (a record that is not one the kernel can have written counts as zeros in its header)
  int mode = 0, p = 0, j = 0;
  long long k = 0;
  const bool load = rec && !r.restart;
  if (load) {
    const ConcHead h = *reinterpret_cast<const ConcHead*>(rec);
    const bool ok = h.mode >= 0 && h.mode <= 2 && h.p >= 0 && h.p <= kConcMaxLag && h.j >= 0 && h.k >= 0 && (h.mode == 0 || h.p >= 1);
    if (ok) { mode = h.mode; p = h.p; j = h.j; k = h.k; }
  }
  if (load) {      // (uniform)
    const float* rt = reinterpret_cast<const float*>(rec + sizeof(ConcHead));
    const float* rh = rt + kConcMaxLag;
    for (int i = tid; i < kConcMaxLag; i += kConcThreads) T[i] = rt[i];
    for (int i = tid; i < kConcHist; i += kConcThreads) { const float v = rh[i]; y[i] = v; q[i] = conc_q(v); }
  } else {
    for (int i = tid; i < kConcMaxLag; i += kConcThreads) T[i] = 0.f;
    for (int i = tid; i < kConcHist; i += kConcThreads) { y[i] = 0.f; q[i] = 0; }
  }

  for (long long t0 = 0; t0 < r.samples; t0 += kConcTile) {
    const int n = (int)(r.samples - t0 < kConcTile ? r.samples - t0 : kConcTile);
    // ---- the tile, decoded (a lost sample's bytes decode to something that is overwritten before anything reads it), and its flags
    for (int i = tid; i < n; i += kConcThreads) {
      const float v = load_sample(fmt, row, t0 + i);
      y[kConcHist + i] = v; q[kConcHist + i] = conc_q(v);
    }
    const long long m0 = t0 / r.packet;
    const int np = (int)((t0 + n - 1) / r.packet - m0) + 1;      // <= kConcTile + 1
    for (int i = tid; i < np; i += kConcThreads) fl[i] = lost[m0 + i] != 0;
    __syncthreads();

    int pos = 0, m = 0;
    while (pos < n) {
      // ---- the segment: the packets from m on with m's flag, cut at the tile's end
      const int f = fl[m];
      int m1 = m + 1;
      while (m1 < np && fl[m1] == f) ++m1;
      const long long e = (m0 + m1) * r.packet - t0;
      const int end = e < n ? (int)e : n;
      const int b = kConcHist + pos, len = end - pos;
      if (f) {
        if (mode != 1) {
          // ---- a run starts: the lag search on the s16 view, one lag per thread, then the argmin with ties to the smaller lag
          if (tid == 0) best = ~0ull;
          __syncthreads();
          unsigned long long key = ~0ull;
          for (int lag = r.lag_min + tid; lag <= r.lag_max; lag += kConcThreads) {
            unsigned long long D = 0;
#pragma unroll 8      // the loads of 8 terms issue together; integer sums have no order to keep
            for (int i = 1; i <= r.window; ++i) {
              const int d = (int)q[b - i] - (int)q[b - i - lag];      // (b - window - lag_max >= 0: the history covers it)
              const unsigned ud = (unsigned)(d < 0 ? -d : d);
              D += ud * ud;                                           // (65535^2 < 2^32; the sum < 2^42)
            }
            const unsigned long long c = (D << 11) | (unsigned)lag;
            key = c < key ? c : key;
          }
#pragma unroll
          for (int s = 32; s >= 1; s >>= 1) key = conc_min_xor(key, s);
          if ((tid & 63) == 0) atomicMin(&best, key);
          __syncthreads();
          p = (int)(best & 2047u);
          for (int i = tid; i < p; i += kConcThreads) T[i] = y[b - p + i];
          k = 0; mode = 1;
          __syncthreads();
        }
        // ---- synthesis: one thread per sample
        const int k0 = (int)(k % p);
        for (int i = tid; i < len; i += kConcThreads) {
          const float v = __fmul_rn(T[(k0 + i) % p], conc_gain(conc_level(k + i, hold, fall)));
          const float yv = conc_put(fmt, row, t0 + pos + i, v);
          y[b + i] = yv; q[b + i] = conc_q(yv);
        }
        k += len;
      } else {
        if (mode == 1) { j = 0; mode = r.fade > 0 ? 2 : 0; }
        if (mode == 2) {
          // ---- the cross-fade back into received audio: one thread per sample; what lies behind it keeps its bytes
          const int left = r.fade - j, nf = left < len ? (left > 0 ? left : 0) : len;
          const int k0 = (int)(k % p);
          for (int i = tid; i < nf; i += kConcThreads) {
            const long long l_in = ((long long)(j + i + 1) << 20) / (r.fade + 1);
            const float s = __fmul_rn(T[(k0 + i) % p], conc_gain(conc_level(k + i, hold, fall)));
            const float v = __fmaf_rn(s, conc_gain(kConcFull - l_in), __fmul_rn(y[b + i], conc_gain(l_in)));
            const float yv = conc_put(fmt, row, t0 + pos + i, v);
            y[b + i] = yv; q[b + i] = conc_q(yv);
          }
          j += nf; k += nf;
          if (j >= r.fade) mode = 0;
        }
      }
      __syncthreads();      // (the next segment's search and template read what this one wrote)
      pos = end; m = m1;
    }

    // ---- the history moves on: the last kConcHist values, through registers (source and destination overlap when n < kConcHist)
    float hv[kConcHist / kConcThreads];
    short hq[kConcHist / kConcThreads];
#pragma unroll
    for (int u = 0; u < kConcHist / kConcThreads; ++u) { hv[u] = y[n + u * kConcThreads + tid]; hq[u] = q[n + u * kConcThreads + tid]; }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kConcHist / kConcThreads; ++u) { y[u * kConcThreads + tid] = hv[u]; q[u * kConcThreads + tid] = hq[u]; }
    __syncthreads();
  }

  // ---- the state goes back: plain vector stores
  if (rec) {
    if (tid == 0) {
      ConcHead h;
      h.mode = mode; h.p = p; h.j = j; h.reserved0 = 0; h.k = k; h.reserved1 = 0;
      *reinterpret_cast<ConcHead*>(rec) = h;
    }
    float* rt = reinterpret_cast<float*>(rec + sizeof(ConcHead));
    float* rh = rt + kConcMaxLag;
    for (int i = tid; i < kConcMaxLag; i += kConcThreads) rt[i] = T[i];
    for (int i = tid; i < kConcHist; i += kConcThreads) rh[i] = y[i];
  }
}

void launch_conceal(const ConcArgs& a, hipStream_t st) {
  if (a.rows < 1) return;
  hipLaunchKernelGGL(conceal_kernel, dim3(a.rows), dim3(kConcThreads), 0, st, a);
}

}  // namespace cnk

namespace conc {

static_assert(sizeof(conan_conceal_cfg) == 32, "eight int32 fields");
static_assert(CONAN_CONCEAL_MAX_LAG == cnk::kConcMaxLag && CONAN_CONCEAL_MAX_WINDOW == cnk::kConcMaxWindow, "the kernel's limits are the header's");

void check_cfg(const conan_conceal_cfg& c, const char* who) {
  const std::string w = std::string(who) + ": ";
  auto bad = [&](const char* what) { throw Error(CONAN_ERR_INVALID, w + what); };
  if (c.enabled != 0 && c.enabled != 1) bad("conan_conceal_cfg.enabled must be 0 or 1");
  if (!c.enabled) return;      // (the other fields are ignored)
  if (c.packet < 1) bad("packet must be >= 1");
  if (c.lag_min < 1 || c.lag_min > c.lag_max || c.lag_max > CONAN_CONCEAL_MAX_LAG) bad("1 <= lag_min <= lag_max <= CONAN_CONCEAL_MAX_LAG must hold");
  if (c.window < 1 || c.window > CONAN_CONCEAL_MAX_WINDOW) bad("window must be in 1 .. CONAN_CONCEAL_MAX_WINDOW");
  if (c.hold < 0) bad("hold must be >= 0");
  if (c.fall < 1) bad("fall must be >= 1");
  if (c.fade < 0 || c.fade > 1024) bad("fade must be in 0 .. 1024");
}

cnk::ConcRow row(const conan_conceal_cfg& c) {
  cnk::ConcRow r;
  memset(&r, 0, sizeof(r));
  r.packet = c.packet; r.lag_min = c.lag_min; r.lag_max = c.lag_max; r.window = c.window; r.hold = c.hold; r.fall = c.fall; r.fade = c.fade;
  r.slot = -1; r.restart = 1;
  return r;
}

static int64_t packets(int64_t samples, int packet) { return (samples + packet - 1) / packet; }

// The feature's part of the pre-step row call (prestep.h): the second buffer holds the caller's packet flags, one int per packet
struct Stage {
  using Cfg = conan_conceal_cfg; using Row = cnk::ConcRow; using Args = cnk::ConcArgs;
  struct Call { void* wav; int64_t wav_ld; const int32_t* aux; int64_t aux_ld; };
  static constexpr const char *kName = "conceal", *kWhole = "conan_conceal", *kSet = "conan_streams_set_conceal", *kCall = "conan_streams_conceal";
  static constexpr const char *kAux = "lost", *kKernel = "conceal_kernel";
  static constexpr bool kAuxAudio = false;
  static constexpr int kReport = 0, kBlock = 0;
  static constexpr auto set = &conan_streams::conc;
  static constexpr auto check_cfg = &conc::check_cfg;
  static constexpr auto row = &conc::row;
  static constexpr auto launch = &cnk::launch_conceal;
  static const char* check_call(const Call&) { return nullptr; }
  static const char* check_row(const Cfg& c, int64_t samples, const Call& b) {
    return packets(samples, c.packet) > b.aux_ld ? "lost_ld must cover ceil(samples / packet) flags" : nullptr;
  }
  static void fill(Args& a, const Call& b) { a.wav = b.wav; a.wav_ld = b.wav_ld; a.lost = b.aux; a.lost_ld = b.aux_ld; }
};

void whole(conan_ctx* ctx, const conan_conceal_cfg* cfg, int format, void* x_dev, int64_t ld, int n, const int64_t* samples, const int32_t* lost_dev,
           int64_t lost_ld, void* stream) {
  prestep::whole<Stage>(ctx, cfg, format, {x_dev, ld, lost_dev, lost_ld}, n, samples, stream);
}

void set_conceal(conan_streams* s, const int32_t* slots, int n, const conan_conceal_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream) {
  if (!prestep::begin_set<Stage>(s, slots, n, cfg, seed_dev, seed_ld, stream)) return;
  s->conceal_init();
  // a slot that was off restarts from zeros in its next repair row - or from its seed row, now, which then clears the flag
  s->conc.store(slots, n, *cfg, [&](int i) { s->conc.pending[slots[i]] = 1; });
  if (cfg->enabled && seed_dev) s->conc.seed(slots, n, seed_dev, seed_ld, (hipStream_t)stream, [](int) { return true; });
}

void repair(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, void* wav_dev, int64_t wav_ld, const int32_t* lost_dev, int64_t lost_ld,
            void* stream) {
  prestep::call<Stage>(s, slots, n, samples, {wav_dev, wav_ld, lost_dev, lost_ld}, stream);
}

void state(conan_streams* s, const int32_t* slots, int n, void* state_dev, int64_t ld, void* stream) {
  record_state(s, &conan_streams::conc, "conceal", slots, n, state_dev, ld, stream, fresh_zeros);
}

}  // namespace conc
