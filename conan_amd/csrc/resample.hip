// Polyphase resampler for waveform input at other sample rates: torchaudio.functional.resample's windowed sinc (the reference
// resamples on its input paths: librosa.core.load(sr=...), resampy.resample, torchaudio's Resample), restated in
// include/conan_hip.h (conan_resample_cfg).  Taps are built on the host in double and rounded once to f32; every output is one
// f32 FMA chain over its phase's taps in ascending order (rs_dot), shared by the whole-signal kernel (conan_resample) and the
// streaming kernel (conan_step_wav* with conan_streams_set_input_rate), so the two agree bit for bit whatever their tiles.
#include <climits>
#include <cmath>
#include <cstdio>

#include "host_common.h"
#include "sample_dev.h"

namespace cnk {

// output of phase p: sum over k < cnt of taps[k][p] * win[off + k], ascending k.  The loop runs to the table's L for every lane
// (no divergence); the select keeps the terms past the phase's count out of the sum, and the clamped index keeps the load in the window.
__device__ __forceinline__ float rs_dot(const float* win, int off, int wlen, const float* __restrict__ taps, int nph, int p, int L, int cnt) {
  float acc = 0.f;
#pragma unroll 8      // the loads of 8 taps issue together; the FMA chain keeps its order
  for (int k = 0; k < L; ++k) {
    const float h = taps[(size_t)k * nph + p];
    const float x = win[min(off + k, wlen - 1)];
    const float t = fmaf(h, x, acc);
    acc = k < cnt ? t : acc;
  }
  return acc;
}

// Output j of one row (the caller clamps j into the tile's valid outputs; j0 = the tile's first output): the tile's input window
// [lo, lo + wlen) is the span of its outputs' taps (block min / max through two LDS words), loaded once with fetch(i) (input i,
// zero outside the signal), then one output per thread.  Every thread of the block must call it (barriers).
template <class Fetch>
__device__ __forceinline__ float rs_output(float* lds, long long j0, long long j, const RsFilter& f, int win, const Fetch& fetch) {
  int* red = reinterpret_cast<int*>(lds);
  float* w = lds + 2;
  const long long q0 = j0 / f.nph;
  const long long base = q0 * f.orig - f.w + f.ph[2 * (int)(j0 - q0 * f.nph)];
  const long long q = j / f.nph;
  const int p = (int)(j - q * f.nph);
  const int klo = f.ph[2 * p], cnt = f.ph[2 * p + 1];
  const long long first = q * f.orig - f.w + klo;
  if (threadIdx.x == 0) { red[0] = INT_MAX; red[1] = INT_MIN; }
  __syncthreads();
  atomicMin(&red[0], (int)(first - base));
  atomicMax(&red[1], (int)(first + cnt - 1 - base));
  __syncthreads();
  const long long lo = base + red[0];
  const int wlen = min(red[1] - red[0] + 1, win);
  for (int t = threadIdx.x; t < wlen; t += blockDim.x) w[t] = fetch(lo + t);
  __syncthreads();
  return rs_dot(w, (int)(first - lo), wlen, f.taps, f.nph, p, f.L, cnt);
}

// Drift resampler: the output at 32.32 position (nb << 32) + rel of one row (the caller clamps it into the tile's valid outputs).
// rel_first and rel_last belong to the tile's first and last valid output (block-uniform): positions are monotone, so the tile's
// input window is [n_first - W + 1, n_last + W], loaded once with fetch(i) (input i, zero outside the signal).  The tap loop's trip
// count, 2W, is uniform; its window index is clamped, so every load stays inside the window whatever the position.  Every thread
// of the block must call it (barrier).  Shared by the whole-signal kernel and both stream kernels: one sum, the same bits.
template <class Fetch>
__device__ __forceinline__ float dr_output(float* w, long long nb, unsigned long long rel_first, unsigned long long rel_last, unsigned long long rel, int W,
                                           const float2* __restrict__ tab, int win, const Fetch& fetch) {
  const long long lo = nb + (long long)(rel_first >> 32) - W + 1;
  const int wlen = max(1, min((int)(nb + (long long)(rel_last >> 32) + W - lo) + 1, win));
  for (int t = threadIdx.x; t < wlen; t += blockDim.x) w[t] = fetch(lo + t);
  __syncthreads();
  const unsigned f = (unsigned)rel;
  const int p = (int)(f >> kDrFracBits);
  const float mu = (float)(f & ((1u << kDrFracBits) - 1)) * (1.f / (float)(1 << kDrFracBits));      // exact: 22 bits
  const int off = (int)(nb + (long long)(rel >> 32) - W + 1 - lo);
  float acc = 0.f;
#pragma unroll 8      // the loads of 8 taps issue together; the FMA chain keeps its order
  for (int k = 0; k < 2 * W; ++k) {
    const float2 td = tab[(size_t)k * kDrPhases + p];
    const float h = fmaf(mu, td.y, td.x);
    const float x = w[min(max(off + k, 0), wlen - 1)];
    acc = fmaf(h, x, acc);
  }
  return acc;
}

// A drift row of the stream kernels: output t of the call (t < h) sits at (n0 << 32) + f0 + t * step
struct DrRow { long long n0; unsigned long long step; unsigned f0; int W; const float2* tab; };
template <class Row>
__device__ __forceinline__ DrRow dr_row(const Row& R) {
  DrRow d;
  d.n0 = R.out0; d.step = (unsigned long long)reinterpret_cast<uintptr_t>(R.ph); d.f0 = (unsigned)R.orig; d.W = R.w;
  d.tab = reinterpret_cast<const float2*>(R.taps);
  return d;
}
template <class Fetch>
__device__ __forceinline__ float dr_stream_output(float* lds, const DrRow& d, int tile0, int t, int h, int win, const Fetch& fetch) {
  const int tl = min(tile0 + kRsTile - 1, h - 1), tc = min(t, tl);
  return dr_output(lds, d.n0, d.f0 + (unsigned long long)tile0 * d.step, d.f0 + (unsigned long long)tl * d.step, d.f0 + (unsigned long long)tc * d.step,
                   d.W, d.tab, win, fetch);
}

__global__ __launch_bounds__(kRsTile) void resample_kernel(const ResampleArgs a) {
  extern __shared__ float lds[];
  const long long j0 = (long long)blockIdx.x * kRsTile, jt = j0 + threadIdx.x;
  const bool act = jt < a.nout;
  const float* x = a.x + (size_t)blockIdx.y * a.samples;
  const long long N = a.samples;
  auto fetch = [&](long long i) {
    const float v = x[i < 0 ? 0 : (i >= N ? N - 1 : i)];
    return (i >= 0 && i < N) ? v : 0.f;
  };
  const float y = rs_output(lds, j0, act ? jt : a.nout - 1, a.f, a.win, fetch);
  if (act) a.y[(size_t)blockIdx.y * a.nout + jt] = y;
}

// One launch per wav-in call: row r (blockIdx.y) resamples this call's h outputs of its slot - inputs before in0 from the slot's
// history ring, this call's m inputs from the caller's row, decoded from the row's sample format - into out row r, and appends the m
// decoded inputs to the ring.  The host has checked that the ring positions a call reads ([first tap of its first output, in0)) and
// the ones it writes ([in0, in0 + m)) are disjoint, so the workgroups of a row need no ordering.  Rows without a rate (kRsCopy) are
// decoded into the out row and touch no ring.
__global__ __launch_bounds__(kRsTile) void resample_stream_kernel(const ResampleStreamArgs a) {
  extern __shared__ float lds[];
  const RsRow R = a.rows[blockIdx.y];
  const float* wav = a.wav + blockIdx.y * a.wav_ld;
  const int fmt = R.mode >> kRsFmtShift;
  float* out = a.out + blockIdx.y * a.out_ld;
  const int stride = gridDim.x * kRsTile, t0 = blockIdx.x * kRsTile + threadIdx.x;
  if (R.mode & kRsCopy) {
    for (int t = t0; t < R.m; t += stride) out[t] = load_sample(fmt, wav, t);
    return;
  }
  float* ring = a.ring + (size_t)R.slot * kRsRing;
  if ((int)blockIdx.x * kRsTile < R.h) {          // uniform per block
    const long long j0 = R.out0 + (long long)blockIdx.x * kRsTile, jt = j0 + threadIdx.x;
    const bool act = t0 < R.h;
    const long long end = R.in0 + R.m;
    const int mlast = R.m > 0 ? R.m - 1 : 0;
    auto fetch = [&](long long i) {
      const long long d = i - R.in0;
      const float vw = load_sample(fmt, wav, d < 0 ? 0 : (d > mlast ? mlast : d));
      const float vr = ring[i & (kRsRing - 1)];
      return (i < 0 || i >= end) ? 0.f : (d >= 0 ? vw : vr);
    };
    if (R.mode & kRsDrift) {                      // uniform per block: a drift row (out0 = the first output's input index)
      const float y = dr_stream_output(lds, dr_row(R), (int)blockIdx.x * kRsTile, t0, R.h, a.win + 2, fetch);
      if (act) out[t0] = y;
    } else {
      RsFilter f; f.taps = R.taps; f.ph = R.ph; f.orig = R.orig; f.nph = R.nph; f.w = R.w; f.L = R.L;
      const float y = rs_output(lds, j0, act ? jt : R.out0 + R.h - 1, f, a.win, fetch);
      if (act) out[jt - R.out0] = y;
    }
  }
  for (int t = t0; t < R.m; t += stride) ring[(R.in0 + t) & (kRsRing - 1)] = load_sample(fmt, wav, t);
}

// One launch per vocoder step with an output rate (conan_streams_set_output_rate) or format (conan_streams_set_output_format), behind
// conv_post_kernel: row r (blockIdx.y) resamples its slot's outputs [out0, out0 + h) - model-rate samples before in0 from the slot's
// history ring, the step's m new ones from conv_post's staging row - into row `dst` of the caller's buffer, encoded in the row's
// sample format, and appends the m samples to the ring.  Samples at or past in0 + m read as zero: a flush (m = 0, h = what is left of
// the utterance) pads as the whole-signal kernel does.  The host has checked that the ring positions a launch reads and the ones it
// writes are disjoint.  Rows without a rate are copied (encoded) verbatim.  Stores go through store_sample: whole groups of four lanes.
__global__ __launch_bounds__(kRsTile) void resample_out_kernel(const ResampleOutArgs a) {
  extern __shared__ float lds[];
  const RsOutRow R = a.rows[blockIdx.y];
  const float* wav = a.wav + blockIdx.y * a.wav_ld;
  const int fmt = R.dst >> kOrDstBits;
  float* out = a.out + (R.dst & ((1 << kOrDstBits) - 1)) * a.out_ld;
  const int stride = gridDim.x * kRsTile, t0 = blockIdx.x * kRsTile + threadIdx.x;
  if (!R.taps) {
    const int mlast = R.m > 0 ? R.m - 1 : 0, m4 = (R.m + 3) & ~3;
    for (int t = t0; t < m4; t += stride) store_sample(fmt, out, t, R.m, wav[min(t, mlast)]);
    return;
  }
  const int mask = a.ring_len - 1;
  float* ring = a.ring + (size_t)R.slot * a.ring_len;
  if ((int)blockIdx.x * kRsTile < R.h) {          // uniform per block
    const long long j0 = R.out0 + (long long)blockIdx.x * kRsTile, jt = j0 + threadIdx.x;
    const bool act = t0 < R.h;
    const long long end = R.in0 + R.m;
    const int mlast = R.m > 0 ? R.m - 1 : 0;
    auto fetch = [&](long long i) {
      const long long d = i - R.in0;
      const float vw = wav[d < 0 ? 0 : (d > mlast ? mlast : d)];
      const float vr = ring[i & mask];
      return (i < 0 || i >= end) ? 0.f : (d >= 0 ? vw : vr);
    };
    float y;
    if (R.L == kOrDriftL) {                       // uniform per block: a drift row (out0 = the first output's input index)
      y = dr_stream_output(lds, dr_row(R), (int)blockIdx.x * kRsTile, t0, R.h, a.win + 2, fetch);
    } else {
      RsFilter f; f.taps = R.taps; f.ph = R.ph; f.orig = R.orig; f.nph = R.nph; f.w = R.w; f.L = R.L;
      y = rs_output(lds, j0, act ? jt : R.out0 + R.h - 1, f, a.win, fetch);
    }
    store_sample(fmt, out, t0, R.h, y);           // (every thread of the block: t0 >= h stores nothing)
  }
  for (int t = t0; t < R.m; t += stride) ring[(R.in0 + t) & mask] = wav[t];
}

// position of output j under a whole-signal schedule (every load uniform: the selects keep the last segment that starts at or before j)
__device__ __forceinline__ unsigned long long dr_schedule_pos(const DrSchedule& s, long long j) {
  unsigned long long pos = (unsigned long long)j * s.step[0];
  for (int q = 1; q < s.n; ++q) {
    const unsigned long long c = s.pos[q] + (unsigned long long)(j - s.at[q]) * s.step[q];
    pos = j >= s.at[q] ? c : pos;
  }
  return pos;
}

__global__ __launch_bounds__(kRsTile) void resample_drift_kernel(const ResampleDriftArgs a) {
  extern __shared__ float lds[];
  const long long j0 = (long long)blockIdx.x * kRsTile, jt = j0 + threadIdx.x;
  const long long jl = min(j0 + kRsTile - 1, a.nout - 1);
  const bool act = jt < a.nout;
  const float* x = a.x + (size_t)blockIdx.y * a.samples;
  const long long N = a.samples;
  auto fetch = [&](long long i) {
    const float v = x[i < 0 ? 0 : (i >= N ? N - 1 : i)];
    return (i >= 0 && i < N) ? v : 0.f;
  };
  const float y = dr_output(lds, 0, dr_schedule_pos(a.s, j0), dr_schedule_pos(a.s, jl), dr_schedule_pos(a.s, act ? jt : jl), a.W, a.tab, a.win, fetch);
  if (act) a.y[(size_t)blockIdx.y * a.y_ld + jt] = y;
}

// conan_convert_samples: row r (blockIdx.y), samples [0, samples) in groups of four per lane group, any format to any format.
__global__ __launch_bounds__(kRsTile) void convert_samples_kernel(const ConvertSamplesArgs a) {
  const char* src = reinterpret_cast<const char*>(a.src) + (size_t)blockIdx.y * a.src_ld * 4;
  char* dst = reinterpret_cast<char*>(a.dst) + (size_t)blockIdx.y * a.dst_ld * 4;
  const long long stride = (long long)gridDim.x * kRsTile, n4 = (a.samples + 3) & ~3ll;
  for (long long t = (long long)blockIdx.x * kRsTile + threadIdx.x; t < n4; t += stride)
    store_sample(a.dst_fmt, dst, t, a.samples, load_sample(a.src_fmt, src, min(t, a.samples - 1)));
}

void launch_resample(const ResampleArgs& a, int n, hipStream_t st) {
  const dim3 grid((unsigned)((a.nout + kRsTile - 1) / kRsTile), (unsigned)n);
  hipLaunchKernelGGL(resample_kernel, grid, dim3(kRsTile), (size_t)(a.win + 2) * sizeof(float), st, a);
}

void launch_resample_stream(const ResampleStreamArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(resample_stream_kernel, dim3((unsigned)a.tiles, (unsigned)a.n), dim3(kRsTile), (size_t)(a.win + 2) * sizeof(float), st, a);
}

void launch_resample_out(const ResampleOutArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(resample_out_kernel, dim3((unsigned)a.tiles, (unsigned)a.n), dim3(kRsTile), (size_t)(a.win + 2) * sizeof(float), st, a);
}

void launch_resample_drift(const ResampleDriftArgs& a, int n, hipStream_t st) {
  const dim3 grid((unsigned)((a.nout + kRsTile - 1) / kRsTile), (unsigned)n);
  hipLaunchKernelGGL(resample_drift_kernel, grid, dim3(kRsTile), (size_t)a.win * sizeof(float), st, a);
}

void launch_convert_samples(const ConvertSamplesArgs& a, int n, hipStream_t st) {
  const long long tiles = (a.samples + kRsTile - 1) / kRsTile;
  hipLaunchKernelGGL(convert_samples_kernel, dim3((unsigned)std::min(tiles, 4096ll), (unsigned)n), dim3(kRsTile), 0, st, a);
}

}  // namespace cnk

namespace {

constexpr double kKaiserBeta = 14.769656459379492;

long long gcd_ll(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; }

double bessel_i0(double x) {      // power series: every term positive, converges for the betas in use
  double sum = 1.0, term = 1.0;
  const double h = 0.25 * x * x;
  for (int k = 1; k < 500; ++k) {
    term *= h / ((double)k * k);
    sum += term;
    if (term < sum * 1e-17) break;
  }
  return sum;
}

// The configuration's reduced rates and filter size; CONAN_ERR_INVALID for a configuration the library refuses.
struct RsShape { long long orig, nph; double base, half; int w; };
RsShape rs_shape(const conan_resample_cfg& c) {
  using ch::Error;
  if (c.in_rate < 8000 || c.in_rate > 192000 || c.out_rate < 8000 || c.out_rate > 192000) throw Error(CONAN_ERR_INVALID, "resample: rates must be in 8000 .. 192000 Hz");
  if (c.lowpass_filter_width < 1 || c.lowpass_filter_width > 128) throw Error(CONAN_ERR_INVALID, "resample: lowpass_filter_width must be in 1 .. 128");
  if (!(c.rolloff > 0.f) || !(c.rolloff <= 1.f)) throw Error(CONAN_ERR_INVALID, "resample: rolloff must be in (0, 1]");
  if (c.window != CONAN_RESAMPLE_HANN && c.window != CONAN_RESAMPLE_KAISER) throw Error(CONAN_ERR_INVALID, "resample: window must be CONAN_RESAMPLE_HANN or CONAN_RESAMPLE_KAISER");
  if (c.window == CONAN_RESAMPLE_KAISER && !(c.beta <= 500.f)) throw Error(CONAN_ERR_INVALID, "resample: beta must be <= 500");
  if (c.reserved[0] || c.reserved[1]) throw Error(CONAN_ERR_INVALID, "resample: reserved fields must be 0");
  const long long g = gcd_ll(c.in_rate, c.out_rate);
  RsShape s;
  s.orig = c.in_rate / g; s.nph = c.out_rate / g;
  s.base = (double)std::min(s.orig, s.nph) * (double)c.rolloff;
  s.w = (int)std::ceil(c.lowpass_filter_width * (double)s.orig / s.base);
  s.half = c.lowpass_filter_width * (double)s.orig / s.base;       // a phase's taps span (-half, half) input samples around its centre
  if (2.0 * s.half > CONAN_RESAMPLE_MAX_TAPS - 2) throw Error(CONAN_ERR_INVALID, "resample: more than CONAN_RESAMPLE_MAX_TAPS taps per phase (rolloff too small for these rates)");
  if ((double)s.nph * (2.0 * s.half + 2) > (double)(1 << 24)) throw Error(CONAN_ERR_INVALID, "resample: filter table above 2^24 taps for these rates");
  if ((cnk::kRsTile - 1) * (double)s.orig / s.nph + 2.0 * s.half + 8 > cnk::kRsMaxWindow) throw Error(CONAN_ERR_INVALID, "resample: input window of a tile too large");
  return s;
}

}  // namespace

const ch::RsTable& conan_ctx::resample_table(const conan_resample_cfg& c) {
  const RsShape s = rs_shape(c);
  const double beta = c.window == CONAN_RESAMPLE_KAISER ? (c.beta > 0.f ? (double)c.beta : kKaiserBeta) : 0.0;
  char key[160];
  snprintf(key, sizeof(key), "rs.%d.%d.%d.%.9g.%d.%.17g", c.in_rate, c.out_rate, c.lowpass_filter_width, (double)c.rolloff, c.window, beta);
  auto it = rs_tabs.find(key);
  if (it != rs_tabs.end()) return it->second;
  const int lpw = c.lowpass_filter_width, nph = (int)s.nph, orig = (int)s.orig, w = s.w;
  const double PI = 3.14159265358979323846, scale = s.base / orig, i0b = beta > 0 ? bessel_i0(beta) : 1.0;
  // per phase the contiguous range of taps with |t| < lpw (torchaudio clamps the others to +-lpw, where the window is < 1e-20)
  std::vector<int> ph((size_t)2 * nph);
  std::vector<std::vector<double>> val(nph);
  int L = 0;
  for (int p = 0; p < nph; ++p) {
    const double centre = w + (double)orig * p / nph;
    const long long k0 = std::max(0ll, (long long)std::floor(centre - s.half) - 2), k1 = std::min((long long)2 * w + orig - 1, (long long)std::ceil(centre + s.half) + 2);
    int klo = -1;
    for (long long k = k0; k <= k1; ++k) {
      const double idx = (double)(k - w) / orig;
      double t = (-(double)p / nph + idx) * s.base;          // torchaudio: arange(0, -new, -1) / new + idx, then * base_freq
      if (!(std::fabs(t) < lpw)) continue;
      if (klo < 0) klo = (int)k;
      if ((int)k != klo + (int)val[p].size()) throw ch::Error(CONAN_ERR_INVALID, "resample: non-contiguous taps");
      const double window = beta > 0 ? bessel_i0(beta * std::sqrt(1.0 - (t / lpw) * (t / lpw))) / i0b
                                      : std::pow(std::cos(t * PI / lpw / 2), 2);
      t *= PI;
      const double sinc = t == 0 ? 1.0 : std::sin(t) / t;
      val[p].push_back(sinc * (window * scale));
    }
    if (klo < 0) throw ch::Error(CONAN_ERR_INVALID, "resample: a phase without taps");
    ph[2 * p] = klo; ph[2 * p + 1] = (int)val[p].size();
    L = std::max(L, (int)val[p].size());
  }
  if (L > CONAN_RESAMPLE_MAX_TAPS) throw ch::Error(CONAN_ERR_INVALID, "resample: more than CONAN_RESAMPLE_MAX_TAPS taps per phase");
  std::vector<float> taps((size_t)L * nph, 0.f);
  for (int p = 0; p < nph; ++p)
    for (size_t k = 0; k < val[p].size(); ++k) taps[k * nph + p] = (float)val[p][k];
  ch::RsTable& t = rs_tabs[key];
  float* d_taps = dev_alloc(taps.size(), false);
  HIP_CHECK(hipMemcpy(d_taps, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice));
  int* d_ph = reinterpret_cast<int*>(dev_alloc(ph.size(), false));
  HIP_CHECK(hipMemcpy(d_ph, ph.data(), ph.size() * sizeof(int), hipMemcpyHostToDevice));
  t.f.taps = d_taps; t.f.ph = d_ph; t.f.orig = orig; t.f.nph = nph; t.f.w = w; t.f.L = L;
  t.ph = std::move(ph);
  t.in_rate = c.in_rate; t.out_rate = c.out_rate;
  // a tile's window: the taps of kRsTile consecutive outputs span at most (kRsTile - 1) * orig / new + 2 * half + 2 inputs
  t.win = (int)std::ceil((cnk::kRsTile - 1) * (double)orig / nph + 2.0 * s.half) + 8;
  return t;
}

int64_t conan_resample_length(const conan_resample_cfg* cfg, int64_t samples) {
  if (!cfg || samples < 0) return -1;
  try {
    const RsShape s = rs_shape(*cfg);
    return (int64_t)(((__int128)s.nph * samples + s.orig - 1) / s.orig);
  } catch (...) {
    return -1;
  }
}

void conan_ctx_resample(conan_ctx* ctx, const conan_resample_cfg& c, const float* x, int n, int64_t samples, float* y, int64_t* out_samples, hipStream_t st) {
  using ch::Error;
  if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, "resample: n must be in 1 .. 65535");
  if (samples < 1) throw Error(CONAN_ERR_INVALID, "resample: samples must be >= 1");
  if (c.in_rate == c.out_rate) {
    (void)rs_shape(c);
    HIP_CHECK(hipMemcpyAsync(y, x, (size_t)n * samples * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (out_samples) *out_samples = samples;
    return;
  }
  const ch::RsTable& t = ctx->resample_table(c);
  const long long nout = t.length(samples);
  if ((nout + cnk::kRsTile - 1) / cnk::kRsTile > INT_MAX) throw Error(CONAN_ERR_INVALID, "resample: signal too long");
  cnk::ResampleArgs a;
  a.x = x; a.y = y; a.samples = samples; a.nout = nout; a.f = t.f; a.win = t.win;
  cnk::launch_resample(a, n, st);
  HIP_CHECK(hipGetLastError());
  if (out_samples) *out_samples = nout;
}

// ---- drift resampler (conan_resample_drift*): the law is include/conan_hip.h's.  All position arithmetic is in integers; the host's
// counts come from the closed-form positions, in 128 bits where a product can pass 64.
namespace drift {

using ch::Error;
typedef unsigned __int128 u128;

// W and base / in_rate of a configuration; CONAN_ERR_INVALID for one the drift resampler refuses
static int shape(const conan_resample_cfg& c, double* scale) {
  (void)rs_shape(c);      // the rate, width, rolloff and window limits are conan_resample's
  const double base = (double)std::min(c.in_rate, c.out_rate) * (double)c.rolloff;
  const int W = (int)std::ceil(c.lowpass_filter_width * (double)c.in_rate / base);
  if (2 * W > cnk::kDrMaxTaps) throw Error(CONAN_ERR_INVALID, "resample_drift: more than 512 taps (2W) for these rates and this filter");
  if (scale) *scale = base / c.in_rate;
  return W;
}

static void check_ppb(int side, long long ppb) {
  if (side != CONAN_DRIFT_SOURCE && side != CONAN_DRIFT_SINK) throw Error(CONAN_ERR_INVALID, "resample_drift: side must be CONAN_DRIFT_SOURCE or CONAN_DRIFT_SINK");
  if (ppb < -CONAN_DRIFT_MAX_PPB || ppb > CONAN_DRIFT_MAX_PPB) throw Error(CONAN_ERR_INVALID, "resample_drift: |ppb| must be at most 2 000 000");
}

unsigned long long step(const conan_resample_cfg& c, int side, int ppb) {
  check_ppb(side, ppb);
  const u128 G = 1000000000u;
  const u128 num = side == CONAN_DRIFT_SOURCE ? (u128)c.in_rate * (u128)(1000000000ll + ppb) : (u128)c.in_rate * G;
  const u128 den = side == CONAN_DRIFT_SOURCE ? (u128)c.out_rate * G : (u128)c.out_rate * (u128)(1000000000ll + ppb);
  return (unsigned long long)((num << 32) / den);
}

// LDS floats of a tile's window at the largest step the side can have
int tile_window(const conan_resample_cfg& c, int side) {
  const int W = shape(c, nullptr);
  const unsigned long long smax = step(c, side, side == CONAN_DRIFT_SOURCE ? CONAN_DRIFT_MAX_PPB : -CONAN_DRIFT_MAX_PPB);
  const u128 span = (u128)(cnk::kRsTile - 1) * smax;
  const long long win = (long long)((span + 0xffffffffu) >> 32) + 2 * W + 2;
  if (win > cnk::kRsMaxWindow) throw Error(CONAN_ERR_INVALID, "resample_drift: input window of a tile too large");
  return (int)win;
}

// the schedule's checks; the position of each segment's first output (128 bits: a long signal's positions pass 2^64)
static void positions(const conan_resample_cfg& c, int side, const int64_t* at, const int32_t* ppb, int n_seg, std::vector<u128>& pos,
                      std::vector<unsigned long long>& st) {
  if (!at || !ppb) throw Error(CONAN_ERR_INVALID, "null argument");
  if (n_seg < 1 || n_seg > CONAN_DRIFT_MAX_SEGMENTS) throw Error(CONAN_ERR_INVALID, "resample_drift: n_seg must be in 1 .. CONAN_DRIFT_MAX_SEGMENTS");
  if (at[0] != 0) throw Error(CONAN_ERR_INVALID, "resample_drift: at[0] must be 0");
  pos.assign(n_seg, 0); st.assign(n_seg, 0);
  for (int k = 0; k < n_seg; ++k) {
    if (k && at[k] <= at[k - 1]) throw Error(CONAN_ERR_INVALID, "resample_drift: at[] must be strictly ascending");
    st[k] = step(c, side, ppb[k]);
    // output at[k] is the first at the new step: one step of segment k past the last output of segment k - 1
    if (k) pos[k] = pos[k - 1] + (u128)(at[k] - 1 - at[k - 1]) * st[k - 1] + st[k];
  }
}

// outputs j with pos_j >> 32 < samples
static long long length(const std::vector<u128>& pos, const std::vector<unsigned long long>& st, const int64_t* at, int64_t samples) {
  const u128 end = (u128)samples << 32;
  const int n_seg = (int)pos.size();
  for (int k = 0; k < n_seg; ++k) {
    if (pos[k] >= end) return at[k];
    const u128 cnt = (end - pos[k] + st[k] - 1) / st[k];      // outputs of an unbounded segment k below `end`
    if (k + 1 == n_seg || cnt < (u128)(at[k + 1] - at[k])) return (long long)(at[k] + (long long)cnt);
  }
  return 0;
}

// T[p][k], p = 0 .. kDrPhases, k = 0 .. 2W - 1, in double, rounded once
static void host_table(const conan_resample_cfg& c, int& W, std::vector<float>& tab) {
  double scale;
  W = shape(c, &scale);
  const int lpw = c.lowpass_filter_width;
  const double beta = c.window == CONAN_RESAMPLE_KAISER ? (c.beta > 0.f ? (double)c.beta : kKaiserBeta) : 0.0;
  const double PI = 3.14159265358979323846, i0b = beta > 0 ? bessel_i0(beta) : 1.0;
  tab.assign((size_t)(cnk::kDrPhases + 1) * 2 * W, 0.f);
  for (int p = 0; p <= cnk::kDrPhases; ++p)
    for (int k = 0; k < 2 * W; ++k) {
      const double t = ((double)(k - W + 1) - (double)p / cnk::kDrPhases) * scale;
      if (!(std::fabs(t) < lpw)) continue;
      const double u = t / lpw;
      const double window = beta > 0 ? bessel_i0(beta * std::sqrt(1.0 - u * u)) / i0b : std::pow(std::cos(t * PI / lpw / 2), 2);
      // sin(pi t) through t's distance r from the nearest integer m: (-1)^m sin(pi r), exactly 0 at an integer t
      const double m = std::nearbyint(t), r = t - m;
      const double sn = std::fmod(m, 2.0) != 0.0 ? -std::sin(PI * r) : std::sin(PI * r);
      const double sinc = t == 0 ? 1.0 : sn / (PI * t);
      tab[(size_t)p * 2 * W + k] = (float)(sinc * (window * scale));
    }
}

}  // namespace drift

const ch::DrTable& conan_ctx::drift_table(const conan_resample_cfg& c) {
  (void)drift::shape(c, nullptr);
  const double beta = c.window == CONAN_RESAMPLE_KAISER ? (c.beta > 0.f ? (double)c.beta : kKaiserBeta) : 0.0;
  char key[160];
  snprintf(key, sizeof(key), "dr.%d.%d.%d.%.9g.%d.%.17g", c.in_rate, c.out_rate, c.lowpass_filter_width, (double)c.rolloff, c.window, beta);
  auto it = dr_tabs.find(key);
  if (it != dr_tabs.end()) return it->second;
  ch::DrTable t;
  drift::host_table(c, t.W, t.host);
  const int L = 2 * t.W, P = cnk::kDrPhases;
  std::vector<float> td((size_t)2 * L * P);
  for (int k = 0; k < L; ++k)
    for (int p = 0; p < P; ++p) {
      const float a = t.host[(size_t)p * L + k], b = t.host[(size_t)(p + 1) * L + k];
      td[2 * ((size_t)k * P + p)] = a;
      td[2 * ((size_t)k * P + p) + 1] = b - a;
    }
  float* d = dev_alloc(td.size(), false);
  HIP_CHECK(hipMemcpy(d, td.data(), td.size() * sizeof(float), hipMemcpyHostToDevice));
  t.dev = reinterpret_cast<const float2*>(d);
  t.in_rate = c.in_rate; t.out_rate = c.out_rate;
  return dr_tabs[key] = std::move(t);
}

int64_t conan_resample_drift_length(const conan_resample_cfg* cfg, int side, int64_t samples, const int64_t* at, const int32_t* ppb, int n_seg) {
  if (!cfg || samples < 0) return -1;
  try {
    (void)drift::shape(*cfg, nullptr);
    std::vector<drift::u128> pos; std::vector<unsigned long long> st;
    drift::positions(*cfg, side, at, ppb, n_seg, pos, st);
    return drift::length(pos, st, at, samples);
  } catch (...) {
    return -1;
  }
}

int64_t conan_ctx_resample_drift_table(const conan_resample_cfg& c, int32_t* W_out, float* table, int64_t cap) {
  int W; std::vector<float> tab;
  drift::host_table(c, W, tab);
  if (W_out) *W_out = W;
  if (table) {
    if (cap < (int64_t)tab.size()) throw ch::Error(CONAN_ERR_INVALID, "conan_resample_drift_table: cap below (1024 + 1) * 2W floats");
    memcpy(table, tab.data(), tab.size() * sizeof(float));
  }
  return (int64_t)tab.size();
}

void conan_ctx_resample_drift(conan_ctx* ctx, const conan_resample_cfg& c, int side, const float* x, int n, int64_t samples, const int64_t* at,
                              const int32_t* ppb, int n_seg, float* y, int64_t y_ld, int64_t* out_samples, hipStream_t st) {
  using ch::Error;
  if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, "resample_drift: n must be in 1 .. 65535");
  if (samples < 1 || samples >= (1ll << 31) - cnk::kDrMaxTaps) throw Error(CONAN_ERR_INVALID, "resample_drift: samples must be in 1 .. 2^31 - 513");
  const int W = drift::shape(c, nullptr);
  const int win = drift::tile_window(c, side);
  std::vector<drift::u128> pos; std::vector<unsigned long long> steps;
  drift::positions(c, side, at, ppb, n_seg, pos, steps);
  const long long nout = drift::length(pos, steps, at, samples);
  if (nout < 1 || (nout + cnk::kRsTile - 1) / cnk::kRsTile > INT_MAX) throw Error(CONAN_ERR_INVALID, "resample_drift: signal too long");
  if (y_ld < nout) throw Error(CONAN_ERR_INVALID, "resample_drift: y_ld below the output length (conan_resample_drift_length)");
  const ch::DrTable& t = ctx->drift_table(c);
  cnk::ResampleDriftArgs a;
  a.x = x; a.y = y; a.samples = samples; a.nout = nout; a.y_ld = y_ld; a.tab = t.dev; a.W = W; a.win = win;
  // segments that start at or past the end produce nothing: the kernel sees the ones below it (their positions fit 64 bits)
  a.s.n = 0;
  for (int k = 0; k < n_seg && at[k] < nout; ++k) {
    a.s.at[k] = at[k]; a.s.pos[k] = (unsigned long long)pos[k]; a.s.step[k] = steps[k];
    a.s.n = k + 1;
  }
  for (int k = a.s.n; k < cnk::kDrMaxSeg; ++k) { a.s.at[k] = 0; a.s.pos[k] = 0; a.s.step[k] = 0; }
  cnk::launch_resample_drift(a, n, st);
  HIP_CHECK(hipGetLastError());
  if (out_samples) *out_samples = nout;
}
