// Signalling tones (include/conan_hip.h, conan_tone_cfg): the DTMF detector's kernel and the regeneration's, the whole-signal entry
// points conan_tones / conan_tone_fill and the host side of conan_streams_set_tones.  The wav-in steps launch the detector behind
// their front-end launch, beside the activity detector's, on the rows of the call's tone staging (tone::WavStage below); the vocoder
// step of a chunk with a mode-2 row launches the fill behind the watermark, as the last in-place stage in front of the output
// resampler (streams.hip, hifigan_step).
#include <climits>
#include <cmath>

#include "streams.h"

namespace cnk {

// rows 0 .. 3, columns 0 .. 3 (Hz)
__device__ __forceinline__ int tone_hz(int i) {
  return i == 0 ? 697 : i == 1 ? 770 : i == 2 ? 852 : i == 3 ? 941 : i == 4 ? 1209 : i == 5 ? 1336 : i == 6 ? 1477 : 1633;
}

// the law's frame digit from the frame's 17 sums: E, then (C, S) of the eight frequencies
__device__ __forceinline__ int tone_digit(const long long* sm, const ToneRow& r, const int hop) {
  const long long E = sm[0];
  long long P[kToneFreqs];
#pragma unroll
  for (int i = 0; i < kToneFreqs; ++i) {
    const long long c = sm[1 + 2 * i] >> 16, s = sm[2 + 2 * i] >> 16;
    P[i] = c * c + s * s;
  }
  int ri = 0, ci = 0;
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    if (P[i] > P[ri]) ri = i;
    if (P[4 + i] > P[4 + ci]) ci = i;
  }
  const long long Pr = P[ri], Pc = P[4 + ci];
  bool ok = Pr >= r.thr && Pc >= r.thr;
  ok = ok && Pc * 256 <= Pr * r.twist_fwd && Pr * 256 <= Pc * r.twist_rev;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ok = ok && (i == ri || P[i] * r.sel <= Pr);
    ok = ok && (i == ci || P[4 + i] * r.sel <= Pc);
  }
  ok = ok && (Pr + Pc) * (32 * 256) >= (long long)r.share * hop * E;
  return ok ? 4 * ri + ci : -1;
}

// the law's debounce, level and sound for one frame with digit d
__device__ __forceinline__ void tone_frame(ToneState& s, const ToneRow& r, const int d) {
  constexpr int kStop = 1 << 30;
  if (d >= 0 && d == s.cand) s.run += s.run < kStop;
  else if (d >= 0) { s.cand = d; s.run = 1; }
  else { s.cand = -1; s.run = 0; }
  if (s.cur >= 0) {
    s.held += s.held < kStop;
    s.miss = d == s.cur ? 0 : s.miss + 1;
    if (s.miss >= r.off_frames && s.held >= r.min_frames) { s.cur = -1; s.miss = 0; s.held = 0; }
  }
  if (s.cur < 0 && s.run >= r.on_frames) { s.cur = s.cand; s.events += 1; s.held = 0; s.miss = 0; }
  const int dl = (s.cur >= 0 ? kToneFull : 0) - s.level;
  s.level += dl > r.step ? r.step : (dl < -r.step ? -r.step : dl);
  if (s.cur >= 0) s.sound = s.cur;
  else if (s.level == 0) s.sound = -1;
  s.frames += 1;
}

// One row per workgroup (kActStreamThreads lanes for the rows of a wav-in call, so that the launch does not wait for a whole CU beside
// the vocoder; kActThreads for whole signals), the table staged once in LDS (2 M bytes: 32 KB at 16 kHz).  A wave works on one frame:
// its lanes take consecutive samples - every load unconditional at a clamped, masked address, the zero padding selected after it
//  - and each lane accumulates the 17 int64 partial sums, its eight table phases carried along as additions modulo M.
// Integer sums are associative: the shuffle reduction's order is no part of the law.  The recursion over a tile's frames belongs to
// thread 0, which keeps the state in registers from tile to tile; the tile's rows go out through LDS so that the stores are
// consecutive over the lanes.  Nothing here depends on the tile width, the wave count or the launch's other rows.
__global__ __launch_bounds__(kActThreads) void tone_kernel(const ToneArgs a) {
  extern __shared__ long long tone_lds[];
  long long* sums = tone_lds;                                        // [kToneTile][kToneSums]
  int* dg_s = reinterpret_cast<int*>(sums + kToneTile * kToneSums);  // [kToneTile] each
  int* sd_s = dg_s + kToneTile;
  int* lv_s = sd_s + kToneTile;
  short* W = reinterpret_cast<short*>(lv_s + kToneTile);             // [M]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = blockDim.x, NW = T >> 6;
  if ((int)blockIdx.x >= a.rows) return;
  const ToneRow r = a.tab[blockIdx.x];     // uniform in the workgroup
  if (r.mode == 0) return;                 // a row of a slot without the feature (it holds the fill's place in the table)
  const int hop = a.hop, M = a.M;
  ToneState s = r.seed;
  if (a.seed) s = a.seed[blockIdx.x];      // (a whole-signal row: uniform, every thread reads its first frame index there)
  const long long f_first = r.f_first >= 0 ? r.f_first : s.frames;
  if (tid == 0) {
    if (!r.reseed && r.slot >= 0) s = a.state[r.slot];
    if (r.start_lvl) { a.sound[r.lvl_off - 1] = s.sound; a.level[r.lvl_off - 1] = s.level; }
  }
  if (r.nframes > 0) {
    for (int i = tid; i < M / 2; i += T) reinterpret_cast<int*>(W)[i] = reinterpret_cast<const int*>(a.table)[i];      // (M is a multiple of 4)
    __syncthreads();
  }
  const long long last = r.valid > 0 ? r.valid - 1 : 0;
  const float* src = a.src + r.src_off;
  const unsigned uM = (unsigned)M, quarter = uM / 4;
  for (int base = 0; base < r.nframes; base += kToneTile) {
    const int nt = r.nframes - base < kToneTile ? r.nframes - base : kToneTile;
    for (int j = wave; j < nt; j += NW) {
      const long long j0 = (f_first + base + j) * hop;      // the frame's first utterance sample: the phase, and in a stream the ring's index
      const long long a0 = r.f_first >= 0 ? j0 : (long long)(base + j) * hop;      // (a whole-signal row's samples count from the row's start)
      const unsigned jm = (unsigned)((j0 + lane) % M);
      unsigned ph[kToneFreqs], st[kToneFreqs];
#pragma unroll
      for (int i = 0; i < kToneFreqs; ++i) {
        const unsigned fm = (unsigned)tone_hz(i) % uM;      // (fm * jm < M^2 < 2^32)
        ph[i] = fm * jm % uM;
        st[i] = fm * 64u % uM;
      }
      long long acc[kToneSums];
#pragma unroll
      for (int i = 0; i < kToneSums; ++i) acc[i] = 0;
      for (int k0 = 0; k0 < hop; k0 += 64) {
        const int k = k0 + lane;
        const long long sj = a0 + k;
        const long long sc = sj > last ? last : sj;
        const float v = src[sc & (long long)r.mask];
        const float x = k < hop && sj < r.valid ? v : 0.f;
        const int q = (int)fminf(fmaxf(rintf(x * 32768.f), -32768.f), 32767.f);      // (encode_sample(kFmtS16, x)'s integer)
        acc[0] += (long long)(q * q);
#pragma unroll
        for (int i = 0; i < kToneFreqs; ++i) {
          const unsigned pc = ph[i], ps = pc >= quarter ? pc - quarter : pc + uM - quarter;
          acc[1 + 2 * i] += (long long)(q * (int)W[pc]);      // (|q W| <= 2^29)
          acc[2 + 2 * i] += (long long)(q * (int)W[ps]);
          const unsigned nx = pc + st[i];
          ph[i] = nx >= uM ? nx - uM : nx;
        }
      }
#pragma unroll
      for (int i = 0; i < kToneSums; ++i) {
        long long v = acc[i];
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
        if (lane == 0) sums[j * kToneSums + i] = v;
      }
    }
    __syncthreads();
    if (tid == 0) {
      for (int j = 0; j < nt; ++j) {
        tone_frame(s, r, tone_digit(sums + j * kToneSums, r, hop));
        dg_s[j] = s.cur; sd_s[j] = s.sound; lv_s[j] = s.level;
      }
    }
    __syncthreads();
    if (tid < nt) {
      a.digit[r.out_off + base + tid] = dg_s[tid];
      a.sound[r.lvl_off + base + tid] = sd_s[tid];
      a.level[r.lvl_off + base + tid] = lv_s[tid];
    }
    __syncthreads();      // (the next tile writes the LDS rows again)
  }
  if (tid == 0) {
    if (r.slot >= 0) a.state[r.slot] = s;
    if (r.state_row >= 0) a.state_out[r.state_row] = s;
  }
}

// Four consecutive samples per thread, as the gate: one 16-byte load and store where the thread's samples are whole and aligned
// (always, in a vocoder step), single words otherwise (the tail of a whole signal, an odd stride).  The levels come first: a thread
// whose samples all have l == 0 neither loads nor stores in place, so a row outside a digit costs its level reads only.  The pair's
// two table entries come from global memory (the table is 2 M bytes and stays in L2); the gains are the law's: an integer
// interpolation, one f64 division each, one f32 product and one fused multiply-add.  Rows that do not regenerate return at once
// (uniform in the workgroup).
__global__ __launch_bounds__(kToneFillThreads) void tone_fill_kernel(const ToneFillArgs a) {
  const int i = blockIdx.y;
  const ToneRow r = a.tab[i];              // uniform in the workgroup
  if (r.mode != 2) return;
  const float* x = a.x + (long long)i * a.ld;
  float* y = a.y + (long long)i * a.ld_y;
  const int* sd = a.sound + (long long)i * a.lvl_ld;
  const int* lv = a.level + (long long)i * a.lvl_ld;
  const long long s0 = ((long long)blockIdx.x * kToneFillThreads + threadIdx.x) * 4;
  if (s0 >= a.samples) return;
  const int start_l = a.start_in_lvl ? lv[-1] : a.start_level, start_s = a.start_in_lvl ? sd[-1] : a.start_sound;
  const int hop = a.hop;
  const long long full = (long long)hop << 20;
  const double den = (double)full;
  long long l[4];
  int g[4];
  bool any = false;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long long sx = s0 + e < a.samples ? s0 + e : a.samples - 1;      // (clamped: the rows of a sample past the row are never read)
    const long long f = sx / hop;
    const int k = (int)(sx - f * hop);
    const int lp = f > 0 ? lv[f - 1] : start_l, ln = lv[f];
    const int sn = sd[f], sp = f > 0 ? sd[f - 1] : start_s;
    l[e] = (long long)lp * (hop - 1 - k) + (long long)ln * (k + 1);
    g[e] = sn >= 0 ? sn : sp;
    any = any || (l[e] != 0 && s0 + e < a.samples);
  }
  const bool inplace = x == y;
  if (!any && inplace) return;
  const bool vec = s0 + 3 < a.samples && ((reinterpret_cast<uintptr_t>(x + s0) | reinterpret_cast<uintptr_t>(y + s0)) & 15) == 0;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (vec) {
    const float4 q = *reinterpret_cast<const float4*>(x + s0);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long sc = s0 + e < a.samples ? s0 + e : a.samples - 1;      // (clamped: a sample past the row is loaded again, never stored)
      v[e] = x[sc];
    }
  }
  float o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = v[e];
  if (any) {
    const unsigned uM = (unsigned)a.M, quarter = uM / 4;
    const unsigned jm0 = (unsigned)((r.pos0 + s0) % a.M);
    const float kf = r.gain * (1.f / 16384.f);      // (exact: a power of two)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (l[e] == 0) continue;
      const unsigned jm = jm0 + e >= uM ? jm0 + e - uM : jm0 + e;
      int w = 0;      // (a frame with a level and no pair sounds nothing)
      if (g[e] >= 0) {
        const unsigned fr = (unsigned)tone_hz((g[e] >> 2) & 3) % uM, fc = (unsigned)tone_hz(4 + (g[e] & 3)) % uM;
        const unsigned pr = fr * jm % uM, pc = fc * jm % uM;
        w = (int)a.table[pr >= quarter ? pr - quarter : pr + uM - quarter] + (int)a.table[pc >= quarter ? pc - quarter : pc + uM - quarter];
      }
      const float syn = __fmul_rn((float)w, kf);
      const float g_t = (float)((double)l[e] / den), g_y = (float)((double)(full - l[e]) / den);
      o[e] = __fmaf_rn(syn, g_t, __fmul_rn(v[e], g_y));
    }
  }
  if (vec) {
    *reinterpret_cast<float4*>(y + s0) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) if (s0 + e < a.samples) y[s0 + e] = o[e];
  }
}

static size_t tone_lds_bytes(int M) { return (size_t)kToneTile * kToneSums * sizeof(long long) + 3 * kToneTile * sizeof(int) + (size_t)M * sizeof(short); }

void launch_tone(const ToneArgs& a, hipStream_t st) {
  if (a.rows < 1) return;
  hipLaunchKernelGGL(tone_kernel, dim3(a.rows), dim3(a.long_rows ? kActThreads : kActStreamThreads), tone_lds_bytes(a.M), st, a);
}

void launch_tone_fill(const ToneFillArgs& a, hipStream_t st) {
  if (a.n < 1 || a.samples < 1) return;
  const long long per = (long long)kToneFillThreads * 4;
  hipLaunchKernelGGL(tone_fill_kernel, dim3((unsigned)((a.samples + per - 1) / per), a.n), dim3(kToneFillThreads), 0, st, a);
}

}  // namespace cnk

namespace tone {

static_assert(sizeof(conan_tone_state) == sizeof(cnk::ToneState), "the kernels' state is the header's");
static_assert(sizeof(conan_tone_cfg) == 104, "two flags, thr, eight int32 fields, gain, a reserved word and the seed");
static_assert(CONAN_TONE_FULL == cnk::kToneFull && CONAN_TONE_HOP_MAX == cnk::kToneHopMax, "the header's constants");
static_assert((size_t)cnk::kToneTile * cnk::kToneSums * 8 + 3 * cnk::kToneTile * 4 + 2 * 50 * cnk::kToneHopMax <= 65536, "the table and a tile's staging fit 64 KB of LDS");
constexpr int kCount = 1 << 30;
constexpr long long kPosMax = 1ll << 40;

void check_cfg(const conan_tone_cfg& c, const char* who) {
  const std::string w = std::string(who) + ": ";
  auto bad = [&](const char* what) { throw Error(CONAN_ERR_INVALID, w + what); };
  if (c.mode < 0 || c.mode > 2) bad("conan_tone_cfg.mode must be 0, 1 or 2");
  if (!c.mode) return;      // (the other fields are ignored)
  if (c.reseed != 0 && c.reseed != 1) bad("conan_tone_cfg.reseed must be 0 or 1");
  if (c.thr < 0 || c.thr > (1ll << 62)) bad("thr must be in 0 .. 2^62");
  if (c.twist_fwd_q8 < 256 || c.twist_fwd_q8 > 65535 || c.twist_rev_q8 < 256 || c.twist_rev_q8 > 65535) bad("twist_fwd_q8 and twist_rev_q8 must be in 256 .. 65535");
  if (c.sel < 1 || c.sel > 65535) bad("sel must be in 1 .. 65535");
  if (c.share_q8 < 0 || c.share_q8 > 256) bad("share_q8 must be in 0 .. 256");
  if (c.on_frames < 1 || c.on_frames > cnk::kToneFull || c.off_frames < 1 || c.off_frames > cnk::kToneFull) bad("on_frames and off_frames must be in 1 .. 2^20");
  if (c.min_frames < 0 || c.min_frames > cnk::kToneFull) bad("min_frames must be in 0 .. 2^20");
  if (c.step < 1 || c.step > cnk::kToneFull) bad("step must be in 1 .. 2^20");
  if (!std::isfinite(c.gain) || !(c.gain >= 0.f) || !(c.gain <= 0.5f)) bad("gain must be in 0 .. 0.5");
  if (c.reserved != 0 || c.seed.reserved != 0) bad("the reserved words must be 0");
  const conan_tone_state& s = c.seed;
  if (s.cand < -1 || s.cand > 15 || s.cur < -1 || s.cur > 15 || s.sound < -1 || s.sound > 15) bad("seed.cand, seed.cur and seed.sound must be in -1 .. 15");
  if (s.run < 0 || s.run > kCount || s.miss < 0 || s.miss > kCount || s.held < 0 || s.held > kCount) bad("seed.run, seed.miss and seed.held must be in 0 .. 2^30");
  if (s.level < 0 || s.level > cnk::kToneFull) bad("seed.level must be in 0 .. 2^20");
  if (s.events < 0 || s.events > kPosMax || s.frames < 0 || s.frames > kPosMax) bad("seed.events and seed.frames must be in 0 .. 2^40");
}

void check_rate(int hop, const char* who) {
  if (hop < 2 || hop > cnk::kToneHopMax || (50 * hop) % 4 != 0)
    throw Error(CONAN_ERR_UNSUPPORTED, std::string(who) + ": the tone table needs a hop in 2 .. 512 and a sample rate (50 * hop) that is a multiple of 4");
}

std::vector<short> host_table(int M) {
  std::vector<short> t((size_t)M);
  const double w = 2.0 * 3.14159265358979323846 / (double)M;
  for (int m = 0; m < M; ++m) t[m] = (short)std::rint(16384.0 * std::cos(w * (double)m));
  return t;
}

void table_out(int sample_rate, int16_t* out) {
  if (!out) throw Error(CONAN_ERR_INVALID, "null argument");
  if (sample_rate < 1 || sample_rate % 50 != 0) throw Error(CONAN_ERR_UNSUPPORTED, "conan_tone_table: sample_rate must be 50 * hop");
  check_rate(sample_rate / 50, "conan_tone_table");
  const std::vector<short> t = host_table(sample_rate);
  memcpy(out, t.data(), t.size() * sizeof(short));
}

const short* table(conan_ctx* ctx, int M) {
  const std::string key = "tone_table/" + std::to_string(M);
  if (float* p = ctx->vec_or_null(key)) return reinterpret_cast<const short*>(p);
  const std::vector<short> t = host_table(M);
  float* d = ctx->dev_alloc(((size_t)M * sizeof(short) + sizeof(float) - 1) / sizeof(float), false);
  HIP_CHECK(hipMemcpy(d, t.data(), t.size() * sizeof(short), hipMemcpyHostToDevice));
  ctx->vecs[key] = d;
  return reinterpret_cast<const short*>(d);
}

cnk::ToneRow row(const conan_tone_cfg& c) {
  cnk::ToneRow r;
  memset(&r, 0, sizeof(r));
  memcpy(&r.seed, &c.seed, sizeof(r.seed));
  r.thr = c.thr; r.twist_fwd = c.twist_fwd_q8; r.twist_rev = c.twist_rev_q8; r.sel = c.sel; r.share = c.share_q8;
  r.on_frames = c.on_frames; r.off_frames = c.off_frames; r.min_frames = c.min_frames; r.step = c.step; r.gain = c.gain;
  r.mode = c.mode; r.mask = -1; r.reseed = 1; r.slot = -1; r.state_row = -1; r.f_first = -1;
  return r;
}

// the rows of a whole-signal launch -> the context's workspace, through its pinned staging (as conan_activity's)
static const cnk::ToneRow* upload(conan_ctx* ctx, const std::vector<cnk::ToneRow>& rows, hipStream_t st) {
  const size_t bytes = rows.size() * sizeof(cnk::ToneRow);
  cnk::ToneRow* h = static_cast<cnk::ToneRow*>(ctx->loud_stage.take(bytes));
  memcpy(h, rows.data(), bytes);
  char* ws = reinterpret_cast<char*>(ctx->workspace((bytes + sizeof(float) - 1) / sizeof(float), st));
  HIP_CHECK(hipMemcpyAsync(ws, h, bytes, hipMemcpyHostToDevice, st));
  ctx->loud_stage.sent(st);
  return reinterpret_cast<const cnk::ToneRow*>(ws);
}

void whole(conan_ctx* ctx, int hop, const conan_tone_cfg* cfg, const float* wav_dev, int64_t ld, int n, const int64_t* samples, const conan_tone_state* seed_dev,
           int32_t* digit_dev, int32_t* sound_dev, int32_t* level_dev, int64_t out_ld, conan_tone_state* state_out_dev, int64_t* frames_out, void* stream) {
  if (!ctx || !cfg || !wav_dev || !samples || !digit_dev || !sound_dev || !level_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_tones");
  if (!cfg->mode) throw Error(CONAN_ERR_INVALID, "conan_tones: cfg.mode must be 1 or 2");
  check_rate(hop, "conan_tones");
  if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, "conan_tones: n must be in 1 .. 65535");
  if (ld < 1 || ld > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_tones: ld must be in 1 .. 2^31 - 1");
  if (out_ld < 1 || out_ld > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_tones: out_ld must be in 1 .. 2^31 - 1");
  int64_t longest = 0;
  for (int i = 0; i < n; ++i) {
    if (samples[i] < 0 || samples[i] > ld) throw Error(CONAN_ERR_INVALID, "conan_tones: samples[i] must be in 0 .. ld");
    longest = std::max(longest, (samples[i] + hop - 1) / hop);
  }
  if (out_ld < longest) throw Error(CONAN_ERR_INVALID, "conan_tones: out_ld must cover ceil(samples[i] / hop) frames");
  HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  std::vector<cnk::ToneRow> rows((size_t)n, row(*cfg));
  for (int i = 0; i < n; ++i) {
    const int64_t frames = (samples[i] + hop - 1) / hop;
    if (frames_out) frames_out[i] = frames;
    rows[i].src_off = (long long)i * ld; rows[i].valid = samples[i]; rows[i].out_off = (long long)i * out_ld; rows[i].lvl_off = rows[i].out_off;
    rows[i].nframes = (int)frames; rows[i].state_row = state_out_dev ? i : -1;
  }
  cnk::ToneArgs a;
  memset(&a, 0, sizeof(a));
  a.src = wav_dev; a.table = table(ctx, 50 * hop); a.digit = digit_dev; a.sound = sound_dev; a.level = level_dev;
  a.seed = reinterpret_cast<const cnk::ToneState*>(seed_dev); a.state_out = reinterpret_cast<cnk::ToneState*>(state_out_dev);
  a.tab = upload(ctx, rows, st); a.rows = n; a.hop = hop; a.M = 50 * hop;
  a.long_rows = longest > 4 * (cnk::kActStreamThreads / 64);
  cnk::launch_tone(a, st);
  HIP_CHECK(hipGetLastError());
}

void fill(conan_ctx* ctx, int hop, const conan_tone_cfg* cfg, const float* wav_dev, int64_t ld, int n, int64_t samples, const int64_t* pos0, const int32_t* sound_dev,
          const int32_t* level_dev, int64_t lvl_ld, int32_t start_level, int32_t start_sound, float* out_dev, int64_t out_ld, void* stream) {
  if (!ctx || !cfg || !wav_dev || !sound_dev || !level_dev || !out_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_tone_fill");
  if (!cfg->mode) throw Error(CONAN_ERR_INVALID, "conan_tone_fill: cfg.mode must be 1 or 2");
  check_rate(hop, "conan_tone_fill");
  if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, "conan_tone_fill: n must be in 1 .. 65535");
  if (samples < 1 || samples > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_tone_fill: samples must be in 1 .. 2^31 - 1");
  if (ld < samples || ld > INT_MAX || out_ld < samples || out_ld > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_tone_fill: ld and out_ld must be in samples .. 2^31 - 1");
  if (out_dev == wav_dev && out_ld != ld) throw Error(CONAN_ERR_INVALID, "conan_tone_fill: in place (out_dev = wav_dev) out_ld must be ld");
  if (lvl_ld < (samples + hop - 1) / hop || lvl_ld > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_tone_fill: lvl_ld must cover ceil(samples / hop) frames");
  if (start_level < 0 || start_level > cnk::kToneFull) throw Error(CONAN_ERR_INVALID, "conan_tone_fill: start_level must be in 0 .. 2^20");
  if (start_sound < -1 || start_sound > 15) throw Error(CONAN_ERR_INVALID, "conan_tone_fill: start_sound must be in -1 .. 15");
  for (int i = 0; i < n && pos0; ++i)
    if (pos0[i] < 0 || pos0[i] > (int64_t)1 << 62) throw Error(CONAN_ERR_INVALID, "conan_tone_fill: pos0[i] must be in 0 .. 2^62");
  HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  std::vector<cnk::ToneRow> rows((size_t)n, row(*cfg));
  for (int i = 0; i < n; ++i) { rows[i].mode = 2; rows[i].pos0 = pos0 ? pos0[i] : 0; }
  cnk::ToneFillArgs a;
  memset(&a, 0, sizeof(a));
  a.x = wav_dev; a.y = out_dev; a.sound = sound_dev; a.level = level_dev; a.table = table(ctx, 50 * hop); a.tab = upload(ctx, rows, st);
  a.ld = ld; a.ld_y = out_ld; a.lvl_ld = lvl_ld; a.samples = samples; a.n = n; a.hop = hop; a.M = 50 * hop;
  a.start_level = start_level; a.start_sound = start_sound; a.start_in_lvl = 0;
  cnk::launch_tone_fill(a, st);
  HIP_CHECK(hipGetLastError());
}

void set_tones(conan_streams* s, const int32_t* slots, int n, const conan_tone_cfg* cfg, void* stream) {
  if (!s || !slots || !cfg) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_streams_set_tones");      // (before the handle is touched, before any GPU use)
  if (cfg->mode && s->wav_in.fe_audio) check_rate(s->ctx->hop, "conan_streams_set_tones");      // (without a front-end: begin_setter's CONAN_ERR_STATE)
  if (!wavio::begin_setter(s, slots, n, cfg->mode != 0, s->tn.allocated(), "conan_streams_set_tones", stream)) return;
  s->tones_init();
  s->tn.store_restarting(slots, n, *cfg);      // the restart travels in the slot's next detector row
}

static cnk::ToneArgs stream_args(conan_streams* s, int q, int rows) {
  cnk::ToneArgs a;
  memset(&a, 0, sizeof(a));
  a.src = s->wav_in.fe_audio; a.table = s->tn.table; a.digit = s->tn.digit[q]; a.sound = s->tn.sound[q]; a.level = s->tn.level[q];
  a.state = s->tn.state; a.tab = s->tn.sets.rows[q]; a.rows = rows; a.hop = s->ctx->hop; a.M = 50 * s->ctx->hop;
  return a;
}

// rows without frames: a pending slot's row starts from the seed and names no slot, any other reads its state (and writes it back as it is)
void state(conan_streams* s, const int32_t* slots, int n, conan_tone_state* state_dev, void* stream) {
  if (!s || !slots || !state_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  wavio::check_slot_list(s, slots, n);
  const std::vector<cnk::ToneRow> rows = s->tn.state_rows<cnk::ToneRow>(slots, n, row, "conan_streams_tone_state", " has no tone detector (conan_streams_set_tones)");
  hipStream_t st = s->enter(stream);
  const int q = s->tn.sets.begin(rows.data(), n, st);
  cnk::ToneArgs a = stream_args(s, q, n);      // (no frames, start_lvl = 0: nothing is read or written in the staging)
  a.state_out = reinterpret_cast<cnk::ToneState*>(state_dev);
  cnk::launch_tone(a, st);
  HIP_CHECK(hipGetLastError());
  s->tn.sets.end(q, st);      // (only the set's table was taken: the staging beside it still holds what its last wav-in call wrote)
}

// the rows the last wav-in call produced, in call order: rows of `seg`, zeros where a row had no detector or did not emit
void last_call(conan_streams* s, int32_t* digit_dev, int32_t* sound_dev, int32_t* level_dev, void* stream) {
  if (!s || !digit_dev || !sound_dev || !level_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  hipStream_t st = wavio::begin_last_call(s, "conan_step_wav_tones", stream);
  const int seg = s->ctx->cfg.emf_segment, n = s->wav_in.fe_last_n;
  copy_last_rows(s->tn.last, digit_dev, n, seg, s->tn.digit, seg, 0, st);
  copy_last_rows(s->tn.last, sound_dev, n, seg, s->tn.sound, seg + 1, 1, st);
  copy_last_rows(s->tn.last, level_dev, n, seg, s->tn.level, seg + 1, 1, st);
}

void WavStage::plan(const conan_streams* s, const WavCall& c) {
  if (s->tn.n_on < 1) return;
  bool any = false;
  for (int i = 0; i < c.n; ++i) {
    if (!s->tn.on(c.slots[i])) continue;
    if (c.mel.sample_rate != 50 * c.hop) throw Error(CONAN_ERR_INVALID, c.who + ": slot " + std::to_string(c.slots[i]) + " detects tones: conan_mel_cfg.sample_rate must be 50 * hop_size");
    const FePlan& p = c.pl[i];
    if (p.emit < 1) continue;
    if (p.R - (long long)p.pos * c.hop > s->wav_in.fe_LA)
      throw Error(CONAN_ERR_UNSUPPORTED, c.who + ": slot " + std::to_string(c.slots[i]) + " detects tones: the chunk's samples have left the audio ring");
    any = true;
  }
  if (!any) return;
  fill.assign(c.groups.size(), 0);
  rows = c.table_rows<cnk::ToneRow>([&](int g, int i, int at, cnk::ToneRow& r) {
    const int slot = c.slots[i];
    if (!s->tn.on(slot)) return false;
    const FePlan& p = c.pl[i];
    r = row(s->tn.cfg[slot]);
    r.src_off = (long long)slot * s->wav_in.fe_LA; r.valid = p.R; r.mask = s->wav_in.fe_LA - 1;
    r.f_first = p.pos; r.pos0 = (long long)p.pos * c.hop; r.nframes = p.emit; r.slot = slot; r.reseed = s->tn.pending[slot]; r.start_lvl = 1;
    r.out_off = (long long)at * c.seg; r.lvl_off = (long long)at * (c.seg + 1) + 1;
    last.push_back({i, 0, at, p.emit});
    if (r.mode == 2) fill[g] = 1;
    return true;
  });
}

// the detector, behind the front-end launch, beside the activity detector's: the call's samples are in the audio rings
void WavStage::enqueue(conan_streams* s, const WavCall& c, hipStream_t cst, FrontWork& front, std::vector<conan_streams::OutPlan>& ops) {
  if (rows.empty()) return;
  q = s->tn.sets.begin(rows.data(), (int)rows.size(), cst);
  for (LastRow& r : last) r.set = q;
  const cnk::ToneArgs a = stream_args(s, q, (int)rows.size());
  front.at[kFrTones] = [s, a](hipStream_t st) { s->profiled("tone_kernel", 0.0, st, [&] { cnk::launch_tone(a, st); }); };
  c.each_group([&](int g, int off) {
    if (!fill[g]) return;
    const size_t lvl = (size_t)off * (c.seg + 1) + 1;
    ops[g].tone = {s->tn.sets.rows[q] + off, s->tn.sound[q] + lvl, s->tn.level[q] + lvl, c.seg + 1};
  });
}

void WavStage::commit(conan_streams* s, hipStream_t, hipStream_t last_st) {
  if (!rows.empty()) s->tn.sets.end(q, last_st);      // (behind the call's last vocoder step: the fill is the last reader of table, sounds and levels)
  for (const cnk::ToneRow& r : rows) if (r.slot >= 0) s->tn.pending[r.slot] = 0;      // (the rows carried the restarts)
  s->tn.last = std::move(last);
}

}  // namespace tone

void conan_streams::tones_init() {
  if (tn.state) return;
  const int seg = ctx->cfg.emf_segment;
  tn.table = tone::table(ctx, 50 * ctx->hop);      // (the context's: one copy per rate, whatever the number of stream-sets)
  tn.state = reinterpret_cast<cnk::ToneState*>(alloc((size_t)max_slots * sizeof(cnk::ToneState) / sizeof(float)));      // zeroed (counted by state_bytes)
  for (int q = 0; q < kActSets; ++q) {
    tn.digit[q] = reinterpret_cast<int*>(alloc((size_t)max_slots * seg));
    tn.sound[q] = reinterpret_cast<int*>(alloc((size_t)max_slots * (seg + 1)));
    tn.level[q] = reinterpret_cast<int*>(alloc((size_t)max_slots * (seg + 1)));
  }
  tn.sets.init(max_slots, allocs);
  state_bytes += (int64_t)kActSets * max_slots * sizeof(cnk::ToneRow);
  tn.assign(max_slots);
}
