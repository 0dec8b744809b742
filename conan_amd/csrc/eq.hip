// Equaliser (conan_eq, conan_eq_design): the biquad cascade that include/conan_hip.h defines (conan_eq_cfg).  The plan is in
// kernels.h (EqState, EqCall); eq_chunk (eq_dev.h) is the one routine that holds the section passes, and eq_signal_kernel walks a
// whole row through it chunk by chunk.  The host side follows the kernel: the cfg check, the sections in the kernels' terms (the
// transition matrices), the design helper and conan_eq's body.
#include <climits>
#include <cmath>

#include "eq_dev.h"
#include "streams.h"

// the host's share of the law (the transition matrices) is single rounded operations too
#pragma clang fp contract(off)

namespace cnk {

// Whole signals: the row's chunks of kEqMaxCall samples in order, each through eq_chunk.
__global__ __launch_bounds__(kEqThreads) void eq_signal_kernel(const EqSignalArgs a) {
  __shared__ EqShared sh;
  __shared__ EqCall c;
  const int tid = threadIdx.x;
  const long long N = a.rows[blockIdx.x].samples;
  EqState* S = (a.state_out ? a.state_out : a.work) + blockIdx.x;
  {      // the row's state before its first sample: the seed's record, or zero at the origin
    const unsigned* src = reinterpret_cast<const unsigned*>(a.seed ? a.seed + blockIdx.x : S);
    unsigned* dst = reinterpret_cast<unsigned*>(S);
    constexpr int kWords = (int)(sizeof(EqState) / sizeof(unsigned));
    for (int i = tid; i < kWords; i += kEqThreads) {
      const unsigned v = src[i];
      dst[i] = a.seed ? v : 0u;
    }
    __syncthreads();
    if (tid == 0) { S->origin = a.origin; S->pos = a.pos0; }
    __syncthreads();
  }
  const float* x = a.x + (size_t)blockIdx.x * a.x_ld;
  float* y = a.y + (size_t)blockIdx.x * a.y_ld;
  for (long long p = 0; p < N; p += kEqMaxCall) {
    if (tid == 0) {
      c.origin = a.origin; c.pos0 = a.pos0 + p;
      c.m = (int)min((long long)kEqMaxCall, N - p); c.tail = (int)((c.pos0 - a.origin) & (kEqSeg - 1));
      c.fresh = (!a.seed && p == 0) ? 1 : 0; c.nsec = a.nsec;
    }
    __syncthreads();
    eq_chunk(a.sec, S, c, x + p, y + p, sh);
  }
}

// A wav-in call's rows (source side) or a vocoder step's rows (output side): one workgroup per table row.
__global__ __launch_bounds__(kEqThreads) void eq_stream_kernel(const EqStreamArgs a) {
  __shared__ EqShared sh;
  const EqRow& R = a.rows[blockIdx.x];
  if (!R.on) return;      // (the whole workgroup)
  const float* x = a.x + (size_t)R.row * a.x_ld;
  float* y = a.y + (size_t)R.row * a.y_ld;
  if (R.copy) {
    for (int t = threadIdx.x; t < R.c.m; t += kEqThreads) y[t] = x[t];
    return;
  }
  eq_chunk(a.sec + (size_t)R.slot * kEqMaxSec, a.state + R.slot, R.c, x, y, sh);
}

constexpr int kEqSetThreads = 128;
constexpr int kEqStateWords = (int)(sizeof(EqState) / sizeof(unsigned));

__global__ __launch_bounds__(kEqSetThreads) void eq_set_kernel(const EqSetArgs a) {
  __shared__ double tmp[kEqSeg];
  const int tid = threadIdx.x;
  const EqRow& R = a.rows[blockIdx.x];
  EqState* S = a.state + R.slot;
  EqSec* sec = a.sec + (size_t)R.slot * kEqMaxSec;
  unsigned* words = reinterpret_cast<unsigned*>(S);
  if (R.mode == 2) {
    const unsigned* src = reinterpret_cast<const unsigned*>(a.seed + (size_t)R.row * a.seed_ld);
    for (int i = tid; i < kEqStateWords; i += kEqSetThreads) words[i] = src[i];
  } else if (R.mode == 1) {
    const int tail = R.c.tail;
    if (tid < kEqSeg) tmp[tid] = tid < tail ? (double)S->tail[tid] : 0.0;
    __syncthreads();
    if (tid == 0) {      // rare and short: at most kEqSeg - 1 samples through the old cascade, once per live change
      for (int k = 0; k < kEqMaxSec; ++k) {
        double s0 = S->carry[k][0], s1 = S->carry[k][1];
        if (k < R.c.nsec) {
          const EqSec f = sec[k];
          for (int t = 0; t < tail; ++t) tmp[t] = eq_step(f, s0, s1, tmp[t]);
        }
        const bool keep = k < R.keep;
        S->carry[k][0] = keep ? s0 : 0.0; S->carry[k][1] = keep ? s1 : 0.0;
      }
      S->origin = R.c.pos0; S->pos = R.c.pos0;
    }
    if (tid < kEqSeg) S->tail[tid] = 0.f;      // (its reads are behind the barrier above)
  } else {
    for (int i = tid; i < kEqStateWords; i += kEqSetThreads) words[i] = 0u;
    __syncthreads();
    if (tid == 0) { S->origin = R.c.pos0; S->pos = R.c.pos0; }
  }
  __syncthreads();      // the old sections have been read
  const double* src = reinterpret_cast<const double*>(a.rows + a.n);
  double* dst = reinterpret_cast<double*>(sec);
  for (int i = tid; i < (int)(kEqMaxSec * sizeof(EqSec) / sizeof(double)); i += kEqSetThreads) dst[i] = src[i];
}

__global__ __launch_bounds__(kEqSetThreads) void eq_state_kernel(const EqStateArgs a) {
  const int tid = threadIdx.x;
  const EqRow& R = a.rows[blockIdx.x];
  const unsigned* src = reinterpret_cast<const unsigned*>(a.state + R.slot);
  char* row = a.out + (size_t)R.row * a.ld;
  unsigned* dst = reinterpret_cast<unsigned*>(row);
  for (int i = tid; i < kEqStateWords; i += kEqSetThreads) {
    const unsigned v = src[i];
    dst[i] = R.mode ? v : 0u;
  }
  __syncthreads();
  if (tid == 0 && !R.mode) { EqState* o = reinterpret_cast<EqState*>(row); o->origin = R.c.pos0; o->pos = R.c.pos0; }
}

void launch_eq_signal(const EqSignalArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(eq_signal_kernel, dim3((unsigned)a.n), dim3(kEqThreads), 0, st, a);
}

void launch_eq_stream(const EqStreamArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(eq_stream_kernel, dim3((unsigned)a.n), dim3(kEqThreads), 0, st, a);
}

void launch_eq_set(const EqSetArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(eq_set_kernel, dim3((unsigned)a.n), dim3(kEqSetThreads), 0, st, a);
}

void launch_eq_state(const EqStateArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(eq_state_kernel, dim3((unsigned)a.n), dim3(kEqSetThreads), 0, st, a);
}

}  // namespace cnk

namespace eq {

static_assert(sizeof(conan_eq_cfg) == 200, "two 32-bit fields, origin, pos, twenty doubles and four reserved words");
static_assert(sizeof(conan_eq_state) == sizeof(cnk::EqState), "the kernels' state is the header's");
static_assert(CONAN_EQ_MAX_SECTIONS == cnk::kEqMaxSec && CONAN_EQ_SEG == cnk::kEqSeg, "the header's constants are the kernels'");
constexpr double kPi = 3.14159265358979323846;

void check_cfg(const conan_eq_cfg& c, const char* who) {
  const std::string w = std::string(who) + ": ";
  auto bad = [&](const std::string& what) { throw Error(CONAN_ERR_INVALID, w + what); };
  if (c.enabled != 0 && c.enabled != 1) bad("conan_eq_cfg.enabled must be 0 or 1");
  if (!c.enabled) return;      // (the other fields are ignored)
  if (c.sections < 1 || c.sections > CONAN_EQ_MAX_SECTIONS) bad("sections must be in 1 .. CONAN_EQ_MAX_SECTIONS");
  if (c.origin < 0 || c.pos < c.origin || c.pos > ((int64_t)1 << 62)) bad("origin and pos must satisfy 0 <= origin <= pos <= 2^62");
  for (int k = 0; k < c.sections; ++k) {
    const double* s = c.coef[k];
    for (int i = 0; i < 5; ++i)
      if (!std::isfinite(s[i]) || std::fabs(s[i]) > CONAN_EQ_MAX_COEF) bad("section " + std::to_string(k) + ": every coefficient must be finite and at most CONAN_EQ_MAX_COEF in magnitude");
    if (!(std::fabs(s[4]) < 1.0) || !(std::fabs(s[3]) < 1.0 + s[4])) bad("section " + std::to_string(k) + " is not stable (|a2| < 1 and |a1| < 1 + a2)");
  }
  for (int k = c.sections; k < CONAN_EQ_MAX_SECTIONS; ++k)
    for (int i = 0; i < 5; ++i)
      if (c.coef[k][i] != 0.0) bad("the coefficients behind the last section must be 0");
  for (int v : c.reserved) if (v != 0) bad("the reserved words must be 0");
}

// One step of the law on the host: the same single rounded operations as cnk::eq_step (contraction is off in this file).
static double host_step(const double* s, double& s0, double& s1, double x) {
  const double y = s[0] * x + s0;
  const double p = s[1] * x, q = s[3] * y;
  s0 = (p - q) + s1;
  const double r = s[2] * x, u = s[4] * y;
  s1 = r - u;
  return y;
}

// cfg's sections in the kernels' terms: the coefficients and M, kEqSeg zero inputs applied to the two unit states.
void sections(const conan_eq_cfg& c, cnk::EqSec* out) {
  for (int k = 0; k < cnk::kEqMaxSec; ++k) {
    cnk::EqSec& f = out[k];
    memset(&f, 0, sizeof(f));
    if (k >= c.sections) continue;
    const double* s = c.coef[k];
    f.b0 = s[0]; f.b1 = s[1]; f.b2 = s[2]; f.a1 = s[3]; f.a2 = s[4];
    for (int col = 0; col < 2; ++col) {
      double s0 = col == 0 ? 1.0 : 0.0, s1 = col == 1 ? 1.0 : 0.0;
      for (int t = 0; t < cnk::kEqSeg; ++t) (void)host_step(s, s0, s1, 0.0);
      f.M[col] = s0; f.M[2 + col] = s1;
    }
  }
}

void design(int kind, double rate, double f0, double q, double gain_db, double* out) {
  if (!out) throw Error(CONAN_ERR_INVALID, "null argument");
  if (kind < CONAN_EQ_LOWPASS || kind > CONAN_EQ_DEEMPHASIS) throw Error(CONAN_ERR_INVALID, "conan_eq_design: kind must be one of CONAN_EQ_LOWPASS .. CONAN_EQ_DEEMPHASIS");
  if (!std::isfinite(rate) || !std::isfinite(f0) || !std::isfinite(q) || !std::isfinite(gain_db)) throw Error(CONAN_ERR_INVALID, "conan_eq_design: every argument must be finite");
  if (!(rate > 0.0) || !(f0 > 0.0) || !(f0 < rate / 2.0)) throw Error(CONAN_ERR_INVALID, "conan_eq_design: f0 must lie inside (0, rate / 2)");
  if (!(q > 0.0)) throw Error(CONAN_ERR_INVALID, "conan_eq_design: q must be > 0");
  if (std::fabs(gain_db) > 60.0) throw Error(CONAN_ERR_INVALID, "conan_eq_design: gain_db must be in -60 .. 60");
  const double w0 = 2.0 * kPi * (f0 / rate), cw = std::cos(w0), sw = std::sin(w0), alpha = sw / (2.0 * q);
  const double A = std::pow(10.0, gain_db / 40.0);
  double b0 = 1.0, b1 = 0.0, b2 = 0.0, a0 = 1.0, a1 = 0.0, a2 = 0.0;
  switch (kind) {
    case CONAN_EQ_LOWPASS: b0 = (1.0 - cw) / 2.0; b1 = 1.0 - cw; b2 = (1.0 - cw) / 2.0; a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha; break;
    case CONAN_EQ_HIGHPASS: b0 = (1.0 + cw) / 2.0; b1 = -(1.0 + cw); b2 = (1.0 + cw) / 2.0; a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha; break;
    case CONAN_EQ_BANDPASS: b0 = alpha; b1 = 0.0; b2 = -alpha; a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha; break;
    case CONAN_EQ_NOTCH: b0 = 1.0; b1 = -2.0 * cw; b2 = 1.0; a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha; break;
    case CONAN_EQ_PEAK: b0 = 1.0 + alpha * A; b1 = -2.0 * cw; b2 = 1.0 - alpha * A; a0 = 1.0 + alpha / A; a1 = -2.0 * cw; a2 = 1.0 - alpha / A; break;
    case CONAN_EQ_LOWSHELF: {
      const double r = 2.0 * std::sqrt(A) * alpha;
      b0 = A * ((A + 1.0) - (A - 1.0) * cw + r); b1 = 2.0 * A * ((A - 1.0) - (A + 1.0) * cw); b2 = A * ((A + 1.0) - (A - 1.0) * cw - r);
      a0 = (A + 1.0) + (A - 1.0) * cw + r; a1 = -2.0 * ((A - 1.0) + (A + 1.0) * cw); a2 = (A + 1.0) + (A - 1.0) * cw - r;
      break;
    }
    case CONAN_EQ_HIGHSHELF: {
      const double r = 2.0 * std::sqrt(A) * alpha;
      b0 = A * ((A + 1.0) + (A - 1.0) * cw + r); b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * cw); b2 = A * ((A + 1.0) + (A - 1.0) * cw - r);
      a0 = (A + 1.0) - (A - 1.0) * cw + r; a1 = 2.0 * ((A - 1.0) - (A + 1.0) * cw); a2 = (A + 1.0) - (A - 1.0) * cw - r;
      break;
    }
    case CONAN_EQ_DCBLOCK: {      // first order: y[n] = g (x[n] - x[n-1]) + R y[n-1], R = exp(-w0), g = (1 + R) / 2 (gain 1 at rate / 2)
      const double R = std::exp(-w0), g = (1.0 + R) / 2.0;
      b0 = g; b1 = -g; a1 = -R;
      break;
    }
    default: {                    // CONAN_EQ_DEEMPHASIS, first order: y[n] = (1 - p) x[n] + p y[n-1], p = exp(-w0) (gain 1 at 0 Hz)
      const double p = std::exp(-w0);
      b0 = 1.0 - p; a1 = -p;
      break;
    }
  }
  out[0] = b0 / a0; out[1] = b1 / a0; out[2] = b2 / a0; out[3] = a1 / a0; out[4] = a2 / a0;
}

void whole(conan_ctx* ctx, const conan_eq_cfg* cfg, const float* x_dev, int64_t x_ld, int n, const int64_t* samples, float* y_dev, int64_t y_ld,
           conan_eq_state* state_out_dev, const conan_eq_state* seed_dev, void* stream) {
  if (!ctx || !cfg || !x_dev || !samples || !y_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_eq");
  if (!cfg->enabled) throw Error(CONAN_ERR_INVALID, "conan_eq: cfg.enabled must be 1");
  if (!seed_dev && cfg->pos != cfg->origin) throw Error(CONAN_ERR_INVALID, "conan_eq: without a seed the rows start at the origin (pos must equal origin)");
  if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, "conan_eq: n must be in 1 .. 65535");
  if (x_ld < 0 || y_ld < 0 || x_ld > ((int64_t)1 << 40) || y_ld > ((int64_t)1 << 40)) throw Error(CONAN_ERR_INVALID, "conan_eq: the row strides must be in 0 .. 2^40");
  if (((uintptr_t)seed_dev | (uintptr_t)state_out_dev) & 7) throw Error(CONAN_ERR_INVALID, "conan_eq: seed_dev and state_out_dev must be 8-byte aligned");
  for (int i = 0; i < n; ++i)
    if (samples[i] < 0 || samples[i] > INT_MAX || samples[i] > x_ld || samples[i] > y_ld)
      throw Error(CONAN_ERR_INVALID, "conan_eq: row " + std::to_string(i) + ": samples must be in 0 .. 2^31 - 1 and fit the row strides");
  HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t table = ((size_t)n * sizeof(cnk::EqSigRow) + 15) & ~(size_t)15;
  const size_t total = table + (state_out_dev ? 0 : (size_t)n * sizeof(cnk::EqState));
  cnk::EqSigRow* h = static_cast<cnk::EqSigRow*>(ctx->loud_stage.take(table));
  for (int i = 0; i < n; ++i) h[i].samples = samples[i];
  char* ws = reinterpret_cast<char*>(ctx->workspace((total + 3) / sizeof(float), st));
  HIP_CHECK(hipMemcpyAsync(ws, h, (size_t)n * sizeof(cnk::EqSigRow), hipMemcpyHostToDevice, st));
  ctx->loud_stage.sent(st);
  cnk::EqSignalArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x_dev; a.x_ld = x_ld; a.y = y_dev; a.y_ld = y_ld; a.n = n;
  a.rows = reinterpret_cast<const cnk::EqSigRow*>(ws);
  a.seed = reinterpret_cast<const cnk::EqState*>(seed_dev);
  a.state_out = reinterpret_cast<cnk::EqState*>(state_out_dev);
  a.work = state_out_dev ? nullptr : reinterpret_cast<cnk::EqState*>(ws + table);
  a.origin = cfg->origin; a.pos0 = cfg->pos; a.nsec = cfg->sections;
  sections(*cfg, a.sec);
  cnk::launch_eq_signal(a, st);
  HIP_CHECK(hipGetLastError());
}

// ---- the streaming forms: the two sides share everything but where a slot's position comes from
static const char* setter_name(bool output) { return output ? "conan_streams_set_output_eq" : "conan_streams_set_input_eq"; }
static conan_streams::Eq& side(conan_streams* s, bool output) { return output ? s->out_eq : s->in_eq; }
static const conan_streams::Eq& side(const conan_streams* s, bool output) { return output ? s->out_eq : s->in_eq; }
static long long position(const conan_streams* s, bool output, int slot) {
  return output ? s->wav_out.voc_samples[slot] : s->wav_in.fe_slot[slot].recv;
}

// what a stream-set needs for a side, before the slot list is read; CONAN_ERR_STATE / CONAN_ERR_UNSUPPORTED
static void check_side(const conan_streams* s, bool output, bool enabling, const std::string& who) {
  const conan_cfg& c = s->ctx->cfg;
  if (output) {
    if (!(c.models & CONAN_MODEL_HIFIGAN)) throw Error(CONAN_ERR_STATE, who + ": context holds no HiFi-GAN model");
    if (enabling && c.voc_upsample == 2) throw Error(CONAN_ERR_UNSUPPORTED, who + ": upsample 'nn' runs whole prefixes, not update intervals");
    if (enabling && (long long)s->max_frames * s->ctx->hop > cnk::kEqMaxCall)
      throw Error(CONAN_ERR_UNSUPPORTED, who + ": a vocoder step of max_frames * hop samples exceeds the 1920 samples a row holds");
  } else {
    if (!s->wav_in.fe_audio) throw Error(CONAN_ERR_STATE, who + ": the stream-set has no streaming front-end (all three models)");
    if (enabling && (long long)c.emf_segment * s->ctx->hop > cnk::kEqMaxCall)
      throw Error(CONAN_ERR_UNSUPPORTED, who + ": segment * hop exceeds the 1920 samples a call row holds");
  }
}

static void check_rows(const std::string& who, const void* p, int64_t ld) {
  if (ld < (int64_t)sizeof(cnk::EqState) || ((uintptr_t)p & 7) || (ld & 7))
    throw Error(CONAN_ERR_INVALID, who + ": rows are conan_eq_state_bytes bytes, 8-byte aligned, ld (a multiple of 8) apart");
}

static cnk::EqRow blank_row() {
  cnk::EqRow r;
  memset(&r, 0, sizeof(r));
  return r;
}

void set_eq(conan_streams* s, bool output, const int32_t* slots, int n, const conan_eq_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream) {
  const std::string who = setter_name(output);
  if (!s || !slots || !cfg) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, who.c_str());      // (before the handle is touched, before any GPU use)
  if (seed_dev) check_rows(who, seed_dev, seed_ld);
  check_side(s, output, cfg->enabled != 0, who);
  wavio::check_slot_list(s, slots, n);
  conan_streams::Eq& e = side(s, output);
  for (int i = 0; i < n && cfg->enabled && seed_dev; ++i)
    if (cfg->pos != position(s, output, slots[i]))
      throw Error(CONAN_ERR_INVALID, who + ": slot " + std::to_string(slots[i]) + " is not at the seed's position (cfg.pos)");
  if (!cfg->enabled && !e.allocated()) return;      // a stream-set that never filtered: nothing to allocate, nothing to write
  hipStream_t st = s->enter(stream);      // (rows of pipelined steps in flight were built from the old setting, and they write the state)
  if (!cfg->enabled) { e.store(slots, n, *cfg); return; }
  s->eq_init(e);
  std::vector<cnk::EqRow> rows((size_t)n + cnk::kEqSecRows, blank_row());
  for (int i = 0; i < n; ++i) {
    const int slot = slots[i];
    const long long pos = position(s, output, slot);
    cnk::EqRow& r = rows[i];
    r.slot = slot; r.row = i; r.on = 1; r.c.pos0 = pos; r.c.origin = pos;
    if (seed_dev) { r.mode = 2; e.origin[slot] = cfg->origin; }
    else if (e.on(slot) && !e.pending[slot]) {      // the live change: the tail closes with the old sections, the origin moves here
      r.mode = 1; r.c.origin = e.origin[slot]; r.c.tail = (int)((pos - e.origin[slot]) & (cnk::kEqSeg - 1));
      r.c.nsec = e.cfg[slot].sections; r.keep = std::min(e.cfg[slot].sections, cfg->sections);
      e.origin[slot] = pos;
    } else { r.mode = 0; e.origin[slot] = pos; }
    e.pending[slot] = 0;
  }
  cnk::EqSec sec[cnk::kEqMaxSec];
  sections(*cfg, sec);
  memcpy(static_cast<void*>(&rows[n]), sec, sizeof(sec));
  const int q = e.sets.begin(rows.data(), n + cnk::kEqSecRows, st);
  cnk::EqSetArgs a;
  a.state = e.state; a.sec = e.sec; a.rows = e.sets.rows[q]; a.n = n; a.seed = static_cast<const char*>(seed_dev); a.seed_ld = seed_ld;
  cnk::launch_eq_set(a, st);
  HIP_CHECK(hipGetLastError());
  e.sets.end(q, st);
  conan_eq_cfg stored = *cfg;
  stored.origin = 0; stored.pos = 0;      // (the getter reports them from the slot's own counters)
  e.store(slots, n, stored);
}

void get_eq(const conan_streams* s, bool output, int slot, conan_eq_cfg* cfg_out) {
  if (!s || !cfg_out) throw Error(CONAN_ERR_INVALID, "null argument");
  if (slot < 0 || slot >= s->max_slots) throw Error(CONAN_ERR_INVALID, "slot index out of range");
  if (!output && !s->wav_in.fe_audio) throw Error(CONAN_ERR_STATE, "conan_streams_input_eq: the stream-set has no streaming front-end (all three models)");
  const conan_streams::Eq& e = side(s, output);
  e.get(slot, cfg_out);
  if (!e.on(slot)) return;
  cfg_out->pos = position(s, output, slot);
  cfg_out->origin = e.pending[slot] ? cfg_out->pos : e.origin[slot];
}

// a slot about to restart reports the zero record at its position; any other its record, in the order of `stream`
void state(conan_streams* s, bool output, const int32_t* slots, int n, void* rows_dev, int64_t ld, void* stream) {
  const std::string who = output ? "conan_streams_output_eq_state" : "conan_streams_input_eq_state";
  if (!s || !slots || !rows_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  check_rows(who, rows_dev, ld);
  wavio::check_slot_list(s, slots, n);
  conan_streams::Eq& e = side(s, output);
  std::vector<cnk::EqRow> rows((size_t)n, blank_row());
  for (int i = 0; i < n; ++i) {
    if (!e.on(slots[i])) throw Error(CONAN_ERR_STATE, who + ": slot " + std::to_string(slots[i]) + " has no equaliser (" + setter_name(output) + ")");
    rows[i].slot = slots[i]; rows[i].row = i; rows[i].on = 1; rows[i].mode = e.pending[slots[i]] ? 0 : 1;
    rows[i].c.pos0 = position(s, output, slots[i]); rows[i].c.origin = rows[i].c.pos0;
  }
  hipStream_t st = s->enter(stream);
  const int q = e.sets.begin(rows.data(), n, st);
  cnk::EqStateArgs a;
  a.state = e.state; a.rows = e.sets.rows[q]; a.n = n; a.out = static_cast<char*>(rows_dev); a.ld = ld;
  cnk::launch_eq_state(a, st);
  HIP_CHECK(hipGetLastError());
  e.sets.end(q, st);
}

// one filtered row: m samples from the slot's position on
static void fill_call(const conan_streams::Eq& e, int slot, long long pos, int m, cnk::EqRow& r) {
  const bool fresh = e.pending[slot] != 0;
  const long long origin = fresh ? pos : e.origin[slot];
  r.c.origin = origin; r.c.pos0 = pos; r.c.m = m; r.c.tail = (int)((pos - origin) & (cnk::kEqSeg - 1));
  r.c.fresh = fresh ? 1 : 0; r.c.nsec = e.cfg[slot].sections;
  r.slot = slot; r.on = 1;
}

// the rows carried the restarts: the host's origins follow
static void commit_rows(conan_streams::Eq& e, const std::vector<cnk::EqRow>& rows) {
  for (const cnk::EqRow& r : rows) {
    if (!r.on || r.copy) continue;
    if (r.c.fresh) e.origin[r.slot] = r.c.origin;
    e.pending[r.slot] = 0;
  }
}

std::vector<cnk::EqRow> step_rows(const conan_streams* s, const int32_t* slots, int n, int frames, const std::string& who) {
  std::vector<cnk::EqRow> rows;
  const conan_streams::Eq& e = s->out_eq;
  if (e.n_on < 1 || frames < 1) return rows;
  bool any = false;
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] >= s->max_slots) throw Error(CONAN_ERR_INVALID, "slot index out of range");
    any = any || e.on(slots[i]);
  }
  if (!any) return rows;
  if (s->ctx->cfg.voc_upsample == 2) throw Error(CONAN_ERR_UNSUPPORTED, who + ": a slot filters its output (conan_streams_set_output_eq): upsample 'nn' runs whole prefixes, not update intervals");
  const long long T = (long long)frames * s->ctx->hop;
  if (T > cnk::kEqMaxCall) throw Error(CONAN_ERR_UNSUPPORTED, who + ": a filtered row holds at most 1920 samples");
  rows.assign((size_t)n, blank_row());
  for (int i = 0; i < n; ++i) {
    rows[i].slot = slots[i]; rows[i].row = i;
    if (e.on(slots[i])) fill_call(e, slots[i], s->wav_out.voc_samples[slots[i]], (int)T, rows[i]);
  }
  return rows;
}

int step_begin(conan_streams* s, const std::vector<cnk::EqRow>& rows, hipStream_t st) {
  return s->out_eq.sets.begin(rows.data(), (int)rows.size(), st);
}

void step_launch(conan_streams* s, const std::vector<cnk::EqRow>& rows, int q, float* wav, long long ld, hipStream_t st) {
  conan_streams::Eq& e = s->out_eq;
  cnk::EqStreamArgs a;
  a.x = wav; a.x_ld = ld; a.y = wav; a.y_ld = ld; a.state = e.state; a.sec = e.sec; a.rows = e.sets.rows[q]; a.n = (int)rows.size();
  s->profiled("eq_stream_kernel", 0.0, st, [&] { cnk::launch_eq_stream(a, st); });
  e.sets.end(q, st);
  commit_rows(e, rows);
}

void WavStage::plan(const conan_streams* s, const WavCall& c) {
  const conan_streams::Eq& e = s->in_eq;
  bool any = false;
  for (int i = 0; i < c.n && e.n_on > 0; ++i) any = any || (e.on(c.slots[i]) && c.samples[i] > 0);
  stages = any && !c.rs_launch;
  for (int i = 0; i < c.n && any; ++i) {
    const bool on = e.on(c.slots[i]);
    if (c.samples[i] < 1 || (!on && !stages)) continue;
    if (c.samples[i] > cnk::kEqMaxCall) throw Error(CONAN_ERR_UNSUPPORTED, c.who + ": a filtered call row holds at most 1920 samples");
    cnk::EqRow R = blank_row();
    if (on) fill_call(e, c.slots[i], s->wav_in.fe_slot[c.slots[i]].recv, c.samples[i], R);
    else { R.c.m = c.samples[i]; R.copy = 1; R.slot = c.slots[i]; R.on = 1; }
    R.row = i;
    rows.push_back(R);
  }
}

// the equaliser, between the resampler's launch (or the caller's rows) and the leveller's, on the rows the front-end is about to read
void WavStage::enqueue(conan_streams* s, const WavCall& c, hipStream_t cst, FrontWork& front, std::vector<conan_streams::OutPlan>&) {
  if (rows.empty()) return;
  conan_streams::Eq& e = s->in_eq;
  const int q = e.sets.begin(rows.data(), (int)rows.size(), cst);
  cnk::EqStreamArgs a;
  a.y = s->wav_in.rs_wav[c.rs_q]; a.y_ld = c.common ? c.samples[0] : c.seg * c.hop;
  a.x = stages ? c.wav_dev : a.y; a.x_ld = stages ? c.wav_ld : a.y_ld;
  a.state = e.state; a.sec = e.sec; a.rows = e.sets.rows[q]; a.n = (int)rows.size();
  front.at[kFrEq] = [s, a, q](hipStream_t st) {
    s->profiled("eq_stream_kernel", 0.0, st, [&] { cnk::launch_eq_stream(a, st); });
    s->in_eq.sets.end(q, st);
  };
}

void WavStage::commit(conan_streams* s, hipStream_t, hipStream_t) { commit_rows(s->in_eq, rows); }

}  // namespace eq

void conan_streams::eq_init(Eq& e) {
  if (&e == &in_eq) rs_stage_init();      // (the source side works on the resampler's staging rows)
  if (e.state) return;
  e.state = reinterpret_cast<cnk::EqState*>(alloc((size_t)max_slots * sizeof(cnk::EqState) / sizeof(float)));      // zeroed (counted by state_bytes)
  e.sec = reinterpret_cast<cnk::EqSec*>(alloc((size_t)max_slots * cnk::kEqMaxSec * sizeof(cnk::EqSec) / sizeof(float)));
  e.sets.init(max_slots + cnk::kEqSecRows, allocs);
  state_bytes += (int64_t)kActSets * (max_slots + cnk::kEqSecRows) * sizeof(cnk::EqRow);
  e.assign(max_slots);
  e.origin.assign(max_slots, 0);
}
