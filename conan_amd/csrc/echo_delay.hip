// Echo delay (include/conan_hip.h, conan_echo_delay_cfg): the kernel, the whole-signal entry point conan_echo_delay and the host side of
// conan_streams_set_echo_delay / conan_streams_echo_delay / conan_streams_echo_delay_state.  The estimator reads the caller's mic and far
// rows in front of the canceller and writes only its own state and report; no step path reads anything of it.
#include <climits>
#include <cstddef>

#include "prestep.h"
#include "sample_dev.h"

namespace cnk {

// LDS (about 3.6 KB): the far end's ternary signs as two bit planes (>= thr, <= -thr) - bit u of xp / xn is the sample at tile
// position u - kEdMaxLags, so the first kEdHistWords words are the history and one spare word ends the buffer (the upper half of
// the last funnel shift) - and the mic's two planes of the tile.
constexpr int kEdHistWords = kEdMaxLags / 32, kEdMicWords = kEdTile / 32, kEdFarWords = kEdHistWords + kEdMicWords + 1;

// bits sh .. sh + 31 of the word pair (lo, hi)
__device__ __forceinline__ unsigned ed_funnel(unsigned lo, unsigned hi, int sh) { return (unsigned)((((unsigned long long)hi << 32) | lo) >> sh); }

__device__ __forceinline__ long long ed_wave_sum(long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)((unsigned long long)v >> 32), m);
    v += (long long)(((unsigned long long)hi << 32) | lo);
  }
  return v;
}

// Lane i owns lags i + 256 k, k < n_lags / 256 (rounded up; a lane whose lag is n_lags or more works on and adds nothing): their A
// stay in registers over the row.  Everything that steers the walk - phase, segment bounds, the decisions at a frame end - is uniform
// in the workgroup: every lane computes it from the row and from the same LDS words.
//   Segment (the samples of one frame that this tile brings): per lag and per 32-sample word of the mic planes, masked to the
//   segment, the far window at bit offset (word's first sample) - lag is one funnel shift of two neighbouring words per plane; the
//   word's contribution is popc(dp & xp) + popc(dn & xn) - popc(dp & xn) - popc(dn & xp).
//   Frame end: per lane the first maximum of |A| over its lags and their sum, wave reductions (the lower lag wins a tie), one LDS
//   exchange across the four waves, the decisions, the leak.
__global__ __launch_bounds__(kEdThreads) void echo_delay_kernel(const EdArgs a) {
  __shared__ unsigned xp[kEdFarWords], xn[kEdFarWords], dp[kEdMicWords], dn[kEdMicWords];
  __shared__ int spk[4], sp[4];
  __shared__ long long ss[4];
  const int tid = threadIdx.x, tl = tid & 63, wv = tid >> 6;
  if ((int)blockIdx.x >= a.rows) return;
  const EdRow r = a.tab[blockIdx.x];      // uniform in the workgroup
  const char* mic = reinterpret_cast<const char*>(a.wav) + (long long)r.row * a.wav_ld * 4;
  const char* far = reinterpret_cast<const char*>(a.far) + (long long)r.row * a.far_ld * 4;
  char* rec = r.slot >= 0 ? a.state + (long long)r.slot * kEdStateBytes : nullptr;
  const int fmt = r.fmt, thr = r.thr, nl = r.n_lags;

  // ---- the state: the restart state, or the slot's record (only values come from it)
  const bool load = rec && !r.restart;
  int est = -1, cand = -1, age = 0, run = 0, ph = r.phase;
  long long frames = 0, last_pk = 0, last_s = 0;
  if (load) {
    const EdHead h = *reinterpret_cast<const EdHead*>(rec);
    est = h.est; age = h.age; cand = h.cand; run = h.run; frames = h.frames; last_pk = h.last_pk; last_s = h.last_s;
  }
  int A[kEdPerLane];
  {
    const int* rA = reinterpret_cast<const int*>(rec + sizeof(EdHead));
#pragma unroll
    for (int k = 0; k < kEdPerLane; ++k) { const int l = tid + k * kEdThreads; A[k] = (load && l < nl) ? rA[l] : 0; }
    if (tid < kEdHistWords) {      // 32 history bytes become one word of each plane
      unsigned P = 0, N = 0;
      if (load) {
        const unsigned* rh = reinterpret_cast<const unsigned*>(rec + sizeof(EdHead) + kEdMaxLags * 4) + tid * 8;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const unsigned wd = rh[q];
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const int v = (int)(signed char)(wd >> (8 * b));
            P |= (unsigned)(v > 0) << (4 * q + b); N |= (unsigned)(v < 0) << (4 * q + b);
          }
        }
        if (tid == 0) { P &= ~1u; N &= ~1u; }      // (the record's first byte is no sample)
      }
      xp[tid] = P; xn[tid] = N;
    }
    if (tid == 0) { xp[kEdFarWords - 1] = 0; xn[kEdFarWords - 1] = 0; }
  }
  long long fi = 0;      // frame ends of this row so far

  for (long long t0 = 0; t0 < r.samples; t0 += kEdTile) {
    const int n = (int)(r.samples - t0 < kEdTile ? r.samples - t0 : kEdTile);
    // ---- the tile's planes: a wave's 64 samples are two words of each; the loads are unconditional, their index clamped
    for (int base = 0; base < n; base += kEdThreads) {
      const int i = base + tid;
      const long long ti = t0 + (i < n ? i : n - 1);
      const int xv = echo_q(echo_finite(load_sample(fmt, far, ti))), dv = echo_q(echo_finite(load_sample(fmt, mic, ti)));
      const bool in = i < n;
      const unsigned long long bxp = __ballot(in && xv >= thr), bxn = __ballot(in && xv <= -thr);
      const unsigned long long bdp = __ballot(in && dv >= thr), bdn = __ballot(in && dv <= -thr);
      if (tl == 0) {
        const int w = (base >> 5) + 2 * wv;      // < kEdMicWords
        xp[kEdHistWords + w] = (unsigned)bxp; xp[kEdHistWords + w + 1] = (unsigned)(bxp >> 32);
        xn[kEdHistWords + w] = (unsigned)bxn; xn[kEdHistWords + w + 1] = (unsigned)(bxn >> 32);
        dp[w] = (unsigned)bdp; dp[w + 1] = (unsigned)(bdp >> 32);
        dn[w] = (unsigned)bdn; dn[w + 1] = (unsigned)(bdn >> 32);
      }
    }
    __syncthreads();

    int pos = 0;
    while (pos < n) {
      // ---- the segment [pos, pos + len): what this tile brings of the current frame
      const int len = min(n - pos, kEdFrame - ph);
      const int last = pos + len - 1, w0 = pos >> 5, w1 = last >> 5;
      const unsigned m0 = 0xFFFFFFFFu << (pos & 31), m1 = 0xFFFFFFFFu >> (31 - (last & 31));
#pragma unroll
      for (int k = 0; k < kEdPerLane; ++k) {
        if (k * kEdThreads >= nl) continue;      // (uniform)
        const int l = tid + k * kEdThreads;      // <= kEdMaxLags - 1
        const int o = kEdMaxLags + w0 * 32 - l;      // >= 1: the far bit of sample w0 * 32 at this lag
        const int sh = o & 31;
        int wi = o >> 5;      // wi + 1 + (w1 - w0) <= kEdFarWords - 1
        unsigned lop = xp[wi], lon = xn[wi];
        int c = 0;
        for (int w = w0; w <= w1; ++w) {
          ++wi;
          const unsigned hp = xp[wi], hn = xn[wi];
          const unsigned fp = ed_funnel(lop, hp, sh), fn = ed_funnel(lon, hn, sh);
          const unsigned m = (w == w0 ? m0 : 0xFFFFFFFFu) & (w == w1 ? m1 : 0xFFFFFFFFu);
          const unsigned P = dp[w] & m, N = dn[w] & m;
          c += __popc(P & fp) + __popc(N & fn) - __popc(P & fn) - __popc(N & fp);
          lop = hp; lon = hn;
        }
        if (l < nl) A[k] += c;
      }
      ph += len; pos += len;
      if (ph < kEdFrame) continue;

      // ---- the end of a frame
      ph = 0;
      int pk = -1, p = kEdMaxLags;
      long long s = 0;
#pragma unroll
      for (int k = 0; k < kEdPerLane; ++k) {
        const int l = tid + k * kEdThreads;
        if (l < nl) {
          const int av = A[k] < 0 ? -A[k] : A[k];
          s += av;
          if (av > pk) { pk = av; p = l; }
        }
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const int opk = __shfl_xor(pk, m), op = __shfl_xor(p, m);
        if (opk > pk || (opk == pk && op < p)) { pk = opk; p = op; }
      }
      s = ed_wave_sum(s);
      if (tl == 0) { spk[wv] = pk; sp[wv] = p; ss[wv] = s; }
      __syncthreads();
      pk = spk[0]; p = sp[0]; s = ss[0];
#pragma unroll
      for (int v = 1; v < 4; ++v) {
        const int opk = spk[v], op = sp[v];
        if (opk > pk || (opk == pk && op < p)) { pk = opk; p = op; }
        s += ss[v];
      }
      __syncthreads();      // (every lane has read the exchange words before the next frame end writes them)
      const bool ok = pk >= r.min_peak && (long long)pk * nl > (long long)r.ratio * s;
      const int dist = p > cand ? p - cand : cand - p;
      if (ok && cand >= 0 && dist <= r.tol) ++run;
      else run = ok ? 1 : 0;
      cand = ok ? p : -1;
      if (run >= r.hold) { est = p; age = 0; }
      else if (est >= 0) age = age < INT_MAX ? age + 1 : age;
      ++frames; last_pk = pk; last_s = s;
      if (a.track && tid == 0) {
        long long* o = a.track + (long long)r.row * a.track_ld + fi * 6;
        o[0] = est; o[1] = age; o[2] = cand; o[3] = run; o[4] = last_pk; o[5] = last_s;
      }
      ++fi;
#pragma unroll
      for (int k = 0; k < kEdPerLane; ++k) A[k] -= A[k] >> r.leak;      // (a lag from n_lags on holds 0 and keeps it)
    }

    // ---- the history moves on: bits [n, n + kEdMaxLags) become bits [0, kEdMaxLags), through registers
    unsigned hp = 0, hn = 0;
    if (tid < kEdHistWords) {
      const int o = n + 32 * tid, wi = o >> 5, sh = o & 31;      // wi + 1 <= kEdFarWords - 1
      hp = ed_funnel(xp[wi], xp[wi + 1], sh); hn = ed_funnel(xn[wi], xn[wi + 1], sh);
    }
    __syncthreads();
    if (tid < kEdHistWords) { xp[tid] = hp; xn[tid] = hn; }
    __syncthreads();
  }

  if (a.report && tid == 0) {
    long long* o = a.report + (long long)r.row * 6;
    o[0] = est; o[1] = age; o[2] = cand; o[3] = run; o[4] = last_pk; o[5] = last_s;
  }
  // ---- the state goes back: plain vector stores
  if (rec) {
    if (tid == 0) {
      EdHead o;
      o.pos = r.pos + r.samples; o.est = est; o.age = age; o.cand = cand; o.run = run; o.frames = frames; o.last_pk = last_pk; o.last_s = last_s;
      o.reserved[0] = 0; o.reserved[1] = 0;
      *reinterpret_cast<EdHead*>(rec) = o;
    }
    int* wA = reinterpret_cast<int*>(rec + sizeof(EdHead));
#pragma unroll
    for (int k = 0; k < kEdPerLane; ++k) wA[tid + k * kEdThreads] = A[k];      // (zeros from n_lags on)
    unsigned* wh = reinterpret_cast<unsigned*>(rec + sizeof(EdHead) + kEdMaxLags * 4);
    for (int j = tid; j < kEdMaxLags / 4; j += kEdThreads) {      // four history bytes per store
      unsigned P = (xp[j >> 3] >> ((j & 7) * 4)) & 15u, N = (xn[j >> 3] >> ((j & 7) * 4)) & 15u;
      if (j == 0) { P &= ~1u; N &= ~1u; }
      unsigned wd = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) wd |= (unsigned)(((int)((P >> b) & 1u) - (int)((N >> b) & 1u)) & 0xFF) << (8 * b);
      wh[j] = wd;
    }
  }
}

void launch_echo_delay(const EdArgs& a, hipStream_t st) {
  if (a.rows < 1) return;
  hipLaunchKernelGGL(echo_delay_kernel, dim3(a.rows), dim3(kEdThreads), 0, st, a);
}

}  // namespace cnk

namespace echo_delay {

static_assert(sizeof(conan_echo_delay_cfg) == 48, "twelve int32 fields");
static_assert(CONAN_ECHO_DELAY_FRAME == cnk::kEdFrame && CONAN_ECHO_DELAY_MAX_LAGS == cnk::kEdMaxLags, "the kernel's limits are the header's");

void check_cfg(const conan_echo_delay_cfg& c, const char* who) {
  const std::string w = std::string(who) + ": ";
  auto bad = [&](const char* what) { throw Error(CONAN_ERR_INVALID, w + what); };
  if (c.enabled != 0 && c.enabled != 1) bad("conan_echo_delay_cfg.enabled must be 0 or 1");
  if (!c.enabled) return;      // (the other fields are ignored)
  if (c.n_lags < 64 || c.n_lags > CONAN_ECHO_DELAY_MAX_LAGS || c.n_lags % 64) bad("n_lags must be a multiple of 64 in 64 .. CONAN_ECHO_DELAY_MAX_LAGS");
  if (c.thr < 1 || c.thr > 32767) bad("thr must be in 1 .. 32767");
  if (c.leak < 1 || c.leak > 8) bad("leak must be in 1 .. 8");
  if (c.ratio < 1) bad("ratio must be >= 1");
  if (c.min_peak < 1) bad("min_peak must be >= 1");
  if (c.hold < 1) bad("hold must be >= 1");
  if (c.tol < 0) bad("tol must be >= 0");
}

cnk::EdRow row(const conan_echo_delay_cfg& c) {
  cnk::EdRow r;
  memset(&r, 0, sizeof(r));
  r.n_lags = c.n_lags; r.thr = c.thr; r.leak = c.leak; r.ratio = c.ratio; r.min_peak = c.min_peak; r.hold = c.hold; r.tol = c.tol;
  r.slot = -1; r.restart = 1;
  return r;
}

// The feature's part of the pre-step row call (prestep.h): the second buffer holds the far rows; the whole-signal call also has a
// track of 6 int64 per frame end and row
struct Stage {
  using Cfg = conan_echo_delay_cfg; using Row = cnk::EdRow; using Args = cnk::EdArgs;
  struct Call { const void* wav; int64_t wav_ld; const void* aux; int64_t aux_ld; int64_t* report; int64_t* track; int64_t track_ld; };
  static constexpr const char *kName = "echo_delay", *kWhole = "conan_echo_delay", *kSet = "conan_streams_set_echo_delay", *kCall = "conan_streams_echo_delay";
  static constexpr const char *kAux = "far", *kReportArg = "report_dev", *kKernel = "echo_delay_kernel";
  static constexpr bool kAuxAudio = true;
  static constexpr int kReport = 6, kBlock = cnk::kEdFrame;
  static constexpr auto set = &conan_streams::ed;
  static constexpr auto check_cfg = &echo_delay::check_cfg;
  static constexpr auto row = &echo_delay::row;
  static constexpr auto launch = &cnk::launch_echo_delay;
  static const char* check_call(const Call& b) {
    if (!prestep::stride_ok(b.track_ld)) return "track_ld must be in 0 .. 2^40";
    return ((uintptr_t)b.track & 7) ? "track_dev must be 8-byte aligned" : nullptr;
  }
  static const char* check_row(const Cfg&, int64_t samples, const Call& b) {
    return b.track && samples / CONAN_ECHO_DELAY_FRAME * 6 > b.track_ld ? "the row ends more frames than track_ld holds (6 int64 per frame)" : nullptr;
  }
  static void fill(Args& a, const Call& b) {
    a.wav = b.wav; a.wav_ld = b.wav_ld; a.far = b.aux; a.far_ld = b.aux_ld; a.report = reinterpret_cast<long long*>(b.report);
    a.track = reinterpret_cast<long long*>(b.track); a.track_ld = b.track_ld;
  }
};

void whole(conan_ctx* ctx, const conan_echo_delay_cfg* cfg, int format, const void* mic_dev, int64_t ld, const void* far_dev, int64_t far_ld, int n,
           const int64_t* samples, int64_t* track_dev, int64_t track_ld, int64_t* report_dev, void* stream) {
  prestep::whole<Stage>(ctx, cfg, format, {mic_dev, ld, far_dev, far_ld, report_dev, track_dev, track_ld}, n, samples, stream);
}

// zeros in A[from, to) of a slot's record: the kernel keeps a lag from n_lags on at 0 and relies on finding it so
static void zero_lags(conan_streams* s, int slot, int from, int to, hipStream_t st) {
  if (from < to) HIP_CHECK(hipMemsetAsync(s->ed.record(slot) + sizeof(cnk::EdHead) + (size_t)from * 4, 0, (size_t)(to - from) * 4, st));
}

void set_echo_delay(conan_streams* s, const int32_t* slots, int n, const conan_echo_delay_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream) {
  if (!prestep::begin_set<Stage>(s, slots, n, cfg, seed_dev, seed_ld, stream)) return;
  hipStream_t st = (hipStream_t)stream;
  s->echo_delay_init();
  // a live slot whose n_lags shrinks (a seed or a restart replaces its record anyway)
  for (int i = 0; i < n && cfg->enabled && !seed_dev; ++i)
    if (s->ed.on(slots[i]) && !s->ed.pending[slots[i]]) zero_lags(s, slots[i], cfg->n_lags, s->ed.cfg[slots[i]].n_lags, st);
  // a slot that was off restarts in its next row - or from its seed row, now, which then clears the flag
  s->ed.store(slots, n, *cfg, [&](int i) { s->ed.pending[slots[i]] = 1; });
  if (!cfg->enabled || !seed_dev) return;
  s->ed.seed(slots, n, seed_dev, seed_ld, st, [](int) { return true; });
  for (int i = 0; i < n; ++i) zero_lags(s, slots[i], cfg->n_lags, cnk::kEdMaxLags, st);      // (a seed from a slot with more lags)
  prestep::read_seed_pos<Stage>(s, slots, n, seed_dev, seed_ld, st);
}

void estimate(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, const void* wav_dev, int64_t wav_ld, const void* far_dev, int64_t far_ld,
              int64_t* report_dev, void* stream) {
  prestep::call<Stage>(s, slots, n, samples, {wav_dev, wav_ld, far_dev, far_ld, report_dev, nullptr, 0}, stream);
}

// the restart state: zeros, and no estimate and no candidate
void state(conan_streams* s, const int32_t* slots, int n, void* state_dev, int64_t ld, void* stream) {
  record_state(s, &conan_streams::ed, "echo_delay", slots, n, state_dev, ld, stream, [](int, char* dst, hipStream_t st) {
    HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(dst + offsetof(cnk::EdHead, est)), -1, 1, st));
    HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(dst + offsetof(cnk::EdHead, cand)), -1, 1, st));
  });
}

}  // namespace echo_delay
