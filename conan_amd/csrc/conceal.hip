// Input loss concealment (include/conan_hip.h, conan_conceal_cfg): the kernel, the whole-signal entry point conan_conceal and the host
// side of conan_streams_set_conceal / conan_streams_conceal / conan_streams_conceal_state.  The repair runs on the caller's device rows
// in front of the wav-in step calls, in place and in the slot's input format; no step path reads anything of it.
#include <climits>

#include "streams.h"
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
constexpr int64_t kMaxSamples = 1ll << 40, kMaxStride = 1ll << 40;

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

void whole(conan_ctx* ctx, const conan_conceal_cfg* cfg, int format, void* x_dev, int64_t ld, int n, const int64_t* samples, const int32_t* lost_dev,
           int64_t lost_ld, void* stream) {
  if (!ctx || !cfg || !x_dev || !samples || !lost_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_conceal");
  if (!cfg->enabled) throw Error(CONAN_ERR_INVALID, "conan_conceal: cfg.enabled must be 1");
  wavio::check_format(format, "conan_conceal");
  if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, "conan_conceal: n must be in 1 .. 65535");
  if (ld < 0 || ld > kMaxStride || lost_ld < 0 || lost_ld > kMaxStride) throw Error(CONAN_ERR_INVALID, "conan_conceal: ld and lost_ld must be in 0 .. 2^40");
  if ((uintptr_t)x_dev & 3) throw Error(CONAN_ERR_INVALID, "conan_conceal: x_dev must be 4-byte aligned");
  const int bps = wavio::bytes_per_sample(format);
  for (int i = 0; i < n; ++i) {
    if (samples[i] < 0 || samples[i] > kMaxSamples) throw Error(CONAN_ERR_INVALID, "conan_conceal: row " + std::to_string(i) + ": samples must be in 0 .. 2^40");
    if (samples[i] * bps > ld * 4) throw Error(CONAN_ERR_INVALID, "conan_conceal: row " + std::to_string(i) + " holds more bytes than the row stride (ld x 4 bytes)");
    if (packets(samples[i], cfg->packet) > lost_ld) throw Error(CONAN_ERR_INVALID, "conan_conceal: lost_ld must cover ceil(samples / packet) flags of every row");
  }
  HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t table = (size_t)n * sizeof(cnk::ConcRow);
  cnk::ConcRow* h = static_cast<cnk::ConcRow*>(ctx->loud_stage.take(table));
  const cnk::ConcRow proto = row(*cfg);
  int rows = 0;
  for (int i = 0; i < n; ++i) {
    if (samples[i] < 1) continue;
    h[rows] = proto;
    h[rows].samples = samples[i]; h[rows].row = i; h[rows].fmt = format;
    ++rows;
  }
  if (rows < 1) return;
  char* ws = reinterpret_cast<char*>(ctx->workspace((table + 3) / sizeof(float), st));
  HIP_CHECK(hipMemcpyAsync(ws, h, (size_t)rows * sizeof(cnk::ConcRow), hipMemcpyHostToDevice, st));
  ctx->loud_stage.sent(st);
  cnk::ConcArgs a;
  memset(&a, 0, sizeof(a));
  a.wav = x_dev; a.wav_ld = ld; a.lost = lost_dev; a.lost_ld = lost_ld; a.state = nullptr;
  a.tab = reinterpret_cast<const cnk::ConcRow*>(ws); a.rows = rows;
  cnk::launch_conceal(a, st);
  HIP_CHECK(hipGetLastError());
}

static void check_seed(const char* who, const void* p, int64_t ld) {
  if (ld < cnk::kConcStateBytes || ((uintptr_t)p & 7) || (ld & 7))
    throw Error(CONAN_ERR_INVALID, std::string(who) + ": rows are conan_conceal_state_bytes bytes, 8-byte aligned, ld apart");
}

void set_conceal(conan_streams* s, const int32_t* slots, int n, const conan_conceal_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream) {
  if (!s || !slots || !cfg) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_streams_set_conceal");      // (before the handle is touched, before any GPU use)
  if (seed_dev) check_seed("conan_streams_set_conceal", seed_dev, seed_ld);
  if (!wavio::begin_setter(s, slots, n, cfg->enabled != 0, s->conc.allocated(), "conan_streams_set_conceal", stream)) return;
  hipStream_t st = (hipStream_t)stream;
  s->conceal_init();
  // a slot that was off restarts from zeros in its next repair row - or from its seed row, now, which then clears the flag
  s->conc.store(slots, n, *cfg, [&](int i) { s->conc.pending[slots[i]] = 1; });
  for (int i = 0; i < n && cfg->enabled && seed_dev; ++i) {
    HIP_CHECK(hipMemcpyAsync(s->conc.state + (size_t)slots[i] * cnk::kConcStateBytes, static_cast<const char*>(seed_dev) + (size_t)i * seed_ld,
                             (size_t)cnk::kConcStateBytes, hipMemcpyDeviceToDevice, st));
    s->conc.pending[slots[i]] = 0;
  }
}

void repair(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, void* wav_dev, int64_t wav_ld, const int32_t* lost_dev, int64_t lost_ld,
            void* stream) {
  if (!s || !slots || !samples) throw Error(CONAN_ERR_INVALID, "null argument");
  wavio::check_slot_list(s, slots, n);
  if (wav_ld < 0 || wav_ld > kMaxStride || lost_ld < 0 || lost_ld > kMaxStride) throw Error(CONAN_ERR_INVALID, "conan_streams_conceal: wav_ld and lost_ld must be in 0 .. 2^40");
  std::vector<cnk::ConcRow> rows;
  for (int i = 0; i < n; ++i) {
    if (samples[i] < 0) throw Error(CONAN_ERR_INVALID, "conan_streams_conceal: samples must be >= 0");
    if (!s->conc.on(slots[i]) || samples[i] == 0) continue;      // the row keeps its bytes
    const conan_conceal_cfg& c = s->conc.cfg[slots[i]];
    const int fmt = s->wav_in.in_fmt[slots[i]];
    const std::string where = "conan_streams_conceal: slot " + std::to_string(slots[i]) + ": ";
    if ((long long)samples[i] * wavio::bytes_per_sample(fmt) > wav_ld * 4) throw Error(CONAN_ERR_INVALID, where + "the row holds more bytes than the row stride of wav_dev (wav_ld x 4 bytes)");
    if (packets(samples[i], c.packet) > lost_ld) throw Error(CONAN_ERR_INVALID, where + "lost_ld must cover ceil(samples / packet) flags");
    cnk::ConcRow r = row(c);
    r.samples = samples[i]; r.row = i; r.slot = slots[i]; r.restart = s->conc.pending[slots[i]]; r.fmt = fmt;
    rows.push_back(r);
  }
  if (rows.empty()) return;      // no row to repair: no launch
  if (!wav_dev || !lost_dev) throw Error(CONAN_ERR_INVALID, "null argument (wav_dev / lost_dev with a row to repair)");
  if ((uintptr_t)wav_dev & 3) throw Error(CONAN_ERR_INVALID, "conan_streams_conceal: wav_dev must be 4-byte aligned");
  HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
  hipStream_t st = (hipStream_t)stream;
  const int q = s->conc.sets.begin(rows.data(), (int)rows.size(), st);
  cnk::ConcArgs a;
  memset(&a, 0, sizeof(a));
  a.wav = wav_dev; a.wav_ld = wav_ld; a.lost = lost_dev; a.lost_ld = lost_ld; a.state = s->conc.state;
  a.tab = s->conc.sets.rows[q]; a.rows = (int)rows.size();
  s->profiled("conceal_kernel", 0.0, st, [&] { cnk::launch_conceal(a, st); });
  HIP_CHECK(hipGetLastError());
  s->conc.sets.end(q, st);
  for (const cnk::ConcRow& r : rows) s->conc.pending[r.slot] = 0;
}

// a slot about to restart reports the zero state; any other its record, in the order of `stream`
void state(conan_streams* s, const int32_t* slots, int n, void* state_dev, int64_t ld, void* stream) {
  if (!s || !slots || !state_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  check_seed("conan_streams_conceal_state", state_dev, ld);
  wavio::check_slot_list(s, slots, n);
  for (int i = 0; i < n; ++i)
    if (!s->conc.on(slots[i])) throw Error(CONAN_ERR_STATE, "conan_streams_conceal_state: slot " + std::to_string(slots[i]) + " has no concealment (conan_streams_set_conceal)");
  hipStream_t st = s->enter(stream);
  for (int i = 0; i < n; ++i) {
    char* dst = static_cast<char*>(state_dev) + (size_t)i * ld;
    if (s->conc.pending[slots[i]]) HIP_CHECK(hipMemsetAsync(dst, 0, (size_t)cnk::kConcStateBytes, st));
    else HIP_CHECK(hipMemcpyAsync(dst, s->conc.state + (size_t)slots[i] * cnk::kConcStateBytes, (size_t)cnk::kConcStateBytes, hipMemcpyDeviceToDevice, st));
  }
}

}  // namespace conc

void conan_streams::conceal_init() {
  if (conc.state) return;
  conc.state = reinterpret_cast<char*>(alloc((size_t)max_slots * cnk::kConcStateBytes / sizeof(float)));      // zeroed (counted by state_bytes)
  conc.sets.init(max_slots, allocs);
  state_bytes += (int64_t)kStageSets * max_slots * sizeof(cnk::ConcRow);
  conc.assign(max_slots);
}
