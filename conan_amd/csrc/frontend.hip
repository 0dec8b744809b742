// Mel front-end on the GPU: librosa_wav2spec as called by StreamingVoiceConversion._wav_to_mel
// (utils/audio/__init__.py:37-84, inference/Conan.py:57-70) for waveforms already in device memory:
//   centred, zero-padded frames x periodic Hann -> |rfft| -> Slaney mel filterbank -> log10(max(eps, .)) -> clip.
// The DFT sums and the filterbank products are accumulated in f64 (VALU; 1.1 MMAC per frame, < 0.4 % of the vocoder's
// work per frame): what is left against librosa is librosa's own float32 FFT rounding.
#include <climits>
#include <cmath>

#include "host_common.h"

namespace cnk {

struct FrameArgs { const float* wav; const float* win; float* out; int n, samples, frames, hop, n_fft, framing; };

__global__ __launch_bounds__(256) void stft_frames_kernel(const FrameArgs a) {
  const long long row = blockIdx.x;                       // i * frames + f
  const int i = (int)(row / a.frames), f = (int)(row - (long long)i * a.frames);
  const float* x = a.wav + (long long)i * a.samples;
  if (a.framing == 0) {
    const int s0 = f * a.hop - a.n_fft / 2;               // center=True, pad_mode='constant'
    for (int k = threadIdx.x; k < a.n_fft; k += blockDim.x) {
      const int s = s0 + k;
      a.out[row * a.n_fft + k] = (s >= 0 && s < a.samples) ? x[s] * a.win[k] : 0.f;
    }
  } else {
    // F.pad(y, ((n_fft - hop) / 2,) * 2, mode='reflect') then torch.stft(center=False) (inference/Conan_previous.py:112-116)
    const int s0 = f * a.hop - (a.n_fft - a.hop) / 2;
    for (int k = threadIdx.x; k < a.n_fft; k += blockDim.x) {
      int s = s0 + k;
      if (s < 0) s = -s;
      if (s >= a.samples) s = 2 * (a.samples - 1) - s;
      a.out[row * a.n_fft + k] = x[s] * a.win[k];
    }
  }
}

// |rfft| of the windowed frames: the DFT sums run in f64 (a 1024-term f32 sum loses the bins 5 decades below the frame
// peak, which the log then magnifies; MI355X's f64 vector rate makes the exact sum free at this size: 1 MMAC per frame).
// Block = 256 bins of one frame; the frame and the twiddle table tw[t] = (cos, sin)(2 pi t / N) sit in LDS as f64.
struct DftArgs { const float* fr; const double2* tw; float* mag; int n_fft, nb, cmag; float mag_eps; };

__global__ __launch_bounds__(256) void dft_mag_kernel(const DftArgs a) {
  extern __shared__ __attribute__((aligned(16))) double dsm[];
  double* x = dsm;                                         // [n_fft]
  double2* tw = reinterpret_cast<double2*>(dsm + a.n_fft); // [n_fft]
  const long long row = blockIdx.x;
  for (int t = threadIdx.x; t < a.n_fft; t += blockDim.x) { x[t] = (double)a.fr[row * a.n_fft + t]; tw[t] = a.tw[t]; }
  __syncthreads();
  const int b = blockIdx.y * blockDim.x + threadIdx.x;
  if (b >= a.cmag) return;
  float v = 0.f;
  if (b < a.nb) {
    double re = 0.0, im = 0.0;
    const int mask = a.n_fft - 1;                          // n_fft is a power of two (checked on the host)
    int idx = 0;
    for (int t = 0; t < a.n_fft; ++t) {
      const double2 w = tw[idx];
      re = fma(x[t], w.x, re); im = fma(x[t], w.y, im);
      idx = (idx + b) & mask;
    }
    v = (float)sqrt(re * re + im * im + (double)a.mag_eps);
  }
  a.mag[row * a.cmag + b] = v;
}

// mel = log10(max(eps, filterbank . |X|)) clipped; one thread per (frame, mel bin), f64 sum over the bins of its triangle
struct MelArgs { const float* mag; const float* fb; const int* lo; const int* hi; float* y; long long rows; int nmel, cmag; float eps, vmin, vmax; int natural_log; };

__global__ __launch_bounds__(256) void mel_log_kernel(const MelArgs a) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.rows * a.nmel) return;
  const long long row = e / a.nmel;
  const int m = (int)(e - row * a.nmel);
  const float* mg = a.mag + row * a.cmag;
  const float* w = a.fb + (long long)m * a.cmag;
  double s = 0.0;
  for (int b = a.lo[m]; b < a.hi[m]; ++b) s = fma((double)w[b], (double)mg[b], s);
  const float c = fmaxf(a.eps, (float)s);
  const float v = a.natural_log ? logf(c) : log10f(c);
  a.y[e] = fminf(fmaxf(v, a.vmin), a.vmax);
}

// The two computing parts of mel_stream_ragged_kernel, written as in mel_stream_kernel (dft_mag_kernel's and mel_log_kernel's
// expressions, the same FMA order).  |X| of kMelStreamFrames frames staged in LDS (x [N][F] as f64, tw [N]) into
// mag [F][cmag]: a thread per bin, the f64 FMA chain over t in dft_mag_kernel's order.
__device__ __forceinline__ void mel_dft_mag(const double* x, const double2* tw, float* mag, int N, int nb, int cmag, float mag_eps) {
  constexpr int F = kMelStreamFrames;
  const int mask = N - 1;
  for (int b = threadIdx.x; b < cmag; b += blockDim.x) {
    if (b >= nb) { for (int j = 0; j < F; ++j) mag[j * cmag + b] = 0.f; continue; }
    double re[F], im[F];
    for (int j = 0; j < F; ++j) { re[j] = 0.0; im[j] = 0.0; }
    int idx = 0;
    for (int t = 0; t < N; ++t) {
      const double2 w = tw[idx];
#pragma unroll
      for (int j = 0; j < F; ++j) { const double xv = x[(size_t)t * F + j]; re[j] = fma(xv, w.x, re[j]); im[j] = fma(xv, w.y, im[j]); }
      idx = (idx + b) & mask;
    }
#pragma unroll
    for (int j = 0; j < F; ++j) mag[j * cmag + b] = (float)sqrt(re[j] * re[j] + im[j] * im[j] + (double)mag_eps);
  }
}

// Mel bin mm of one frame's magnitudes mg: mel_log_kernel's f64 filterbank sum, log and clip.
__device__ __forceinline__ float mel_log_value(const float* fb, const int* lo, const int* hi, const float* mg, int mm, int cmag, float eps,
                                               float vmin, float vmax, int natural_log) {
  const float* w = fb + (long long)mm * cmag;
  double s = 0.0;
  for (int b = lo[mm]; b < hi[mm]; ++b) s = fma((double)w[b], (double)mg[b], s);
  const float c = fmaxf(eps, (float)s);
  return fminf(fmaxf(natural_log ? logf(c) : log10f(c), vmin), vmax);
}

// The part of a call's front-end that computes nothing, for slot i: the chunk rows that earlier calls computed, from the mel ring,
// and this call's samples appended to the audio ring.  Neither touches a ring position that the frame computation of the same call
// reads or writes (the host checks the ring spans), so it runs beside it in any order.
__device__ inline void mel_stream_copy(const MelStreamArgs& a, int i) {
  const int slot = a.slots[i];
  const float* mr = a.mring + (long long)slot * a.LM * a.nm;
  for (int e = threadIdx.x; e < a.rows * a.nm; e += blockDim.x) {
    const int r = e / a.nm, mm = e - r * a.nm, src = a.pos + min(r, a.real - 1);
    if (src < a.f0) a.chunk[((long long)i * a.rows + r) * a.nm + mm] = mr[(long long)(src & (a.LM - 1)) * a.nm + mm];
  }
  float* ar = a.aring + (long long)slot * a.LA;
  for (int j = threadIdx.x; j < a.m; j += blockDim.x) ar[(a.r_prev + j) & (a.LA - 1)] = a.wav[(long long)i * a.m + j];
}

// Streaming front-end (conan_step_wav): only the frames that became complete in this call, for all active slots in ONE launch,
// written straight into the slot's mel ring and the [n][rows][nm] chunk the step consumes.  Each frame is bit-identical to
// stft_frames_kernel -> dft_mag_kernel -> mel_log_kernel: the same f32 windowed samples, the same f64 FMA chains over t in the
// same order per bin, the same magnitude and filterbank expressions (a frame depends on its own n_fft samples only).
// Tiling: a workgroup takes kMelStreamFrames frames; its threads take bins, each thread all the workgroup's frames of its bin, so a
// twiddle read from LDS (a gather: 16 B per lane) feeds 2 * kMelStreamFrames f64 FMAs and the samples of the frames are LDS
// broadcasts.  64 streams x 4 frames = 64 workgroups: a quarter of the CUs, beside the previous chunk's vocoder.  The same
// workgroups also do the call's copy / append work (mel_stream_copy), so the front-end is one launch per call.
__global__ __launch_bounds__(1024) void mel_stream_kernel(const MelStreamArgs a) {
  constexpr int F = kMelStreamFrames;
  extern __shared__ __attribute__((aligned(16))) double msm[];
  const int N = a.n_fft;
  const int jobs = a.n * a.nnew;
  for (int i = blockIdx.x; i < a.n; i += gridDim.x) mel_stream_copy(a, i);     // the copy / append work of the call, spread over the grid
  double* x = msm;                                                   // [N][F]
  double2* tw = reinterpret_cast<double2*>(msm + (size_t)N * F);     // [N]
  float* mag = reinterpret_cast<float*>(tw + N);                     // [F][cmag]
  const int job0 = blockIdx.x * F;
  for (int e = threadIdx.x; e < N * F; e += blockDim.x) {
    const int j = e / N, k = e - j * N, job = job0 + j;
    float v = 0.f;
    if (job < jobs) {
      const int i = job / a.nnew, f = a.f0 + (job - i * a.nnew);
      const long long smp = (long long)f * a.hop - N / 2 + k;      // center=True, pad_mode='constant'
      if (smp >= 0 && (a.total < 0 || smp < a.total)) {
        const float xs = smp >= a.r_prev ? a.wav[(long long)i * a.m + (smp - a.r_prev)] : a.aring[(long long)a.slots[i] * a.LA + (smp & (a.LA - 1))];
        v = xs * a.win[k];
      }
    }
    x[(size_t)k * F + j] = (double)v;
  }
  for (int t = threadIdx.x; t < N; t += blockDim.x) tw[t] = a.tw[t];
  __syncthreads();
  const int mask = N - 1;
  for (int b = threadIdx.x; b < a.cmag; b += blockDim.x) {
    if (b >= a.nb) { for (int j = 0; j < F; ++j) mag[j * a.cmag + b] = 0.f; continue; }
    double re[F], im[F];
    for (int j = 0; j < F; ++j) { re[j] = 0.0; im[j] = 0.0; }
    int idx = 0;
    for (int t = 0; t < N; ++t) {
      const double2 w = tw[idx];
#pragma unroll
      for (int j = 0; j < F; ++j) { const double xv = x[(size_t)t * F + j]; re[j] = fma(xv, w.x, re[j]); im[j] = fma(xv, w.y, im[j]); }
      idx = (idx + b) & mask;
    }
#pragma unroll
    for (int j = 0; j < F; ++j) mag[j * a.cmag + b] = (float)sqrt(re[j] * re[j] + im[j] * im[j] + (double)a.mag_eps);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < F * a.nm; e += blockDim.x) {
    const int j = e / a.nm, mm = e - j * a.nm, job = job0 + j;
    if (job >= jobs) continue;
    const int i = job / a.nnew, f = a.f0 + (job - i * a.nnew);
    const float* mg = mag + j * a.cmag;
    const float* w = a.fb + (long long)mm * a.cmag;
    double s = 0.0;
    for (int b = a.lo[mm]; b < a.hi[mm]; ++b) s = fma((double)w[b], (double)mg[b], s);
    const float c = fmaxf(a.eps, (float)s);
    const float v = fminf(fmaxf(a.natural_log ? logf(c) : log10f(c), a.vmin), a.vmax);
    a.mring[((long long)a.slots[i] * a.LM + (f & (a.LM - 1))) * a.nm + mm] = v;
    for (int r = 0; r < a.rows; ++r)
      if (a.pos + min(r, a.real - 1) == f) a.chunk[((long long)i * a.rows + r) * a.nm + mm] = v;
  }
}

// Drain calls that complete no frame: the copy / append part alone, one small workgroup per slot (no LDS).
__global__ __launch_bounds__(256) void mel_stream_copy_kernel(const MelStreamArgs a) { mel_stream_copy(a, blockIdx.x); }

void launch_mel_stream(const MelStreamArgs& a, hipStream_t st) {
  const int blocks = (a.n * a.nnew + kMelStreamFrames - 1) / kMelStreamFrames;
  const int threads = std::min(1024, (a.nb + 63) / 64 * 64);
  const size_t lds = mel_stream_lds_bytes(a.n_fft, a.cmag);
  if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)mel_stream_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  hipLaunchKernelGGL(mel_stream_kernel, dim3(blocks), dim3(threads), lds, st, a);
}

void launch_mel_stream_copy(const MelStreamArgs& a, hipStream_t st) {    // only for calls without new frames
  hipLaunchKernelGGL(mel_stream_copy_kernel, dim3(a.n), dim3(256), 0, st, a);
}


// Ragged streaming front-end (conan_step_wav_ragged): every call row i has its own position (tab[i]: kRaggedWords ints), so the
// frame jobs of all rows are numbered by the prefix sums tab[i].kRgJob and a workgroup's kMelStreamFrames frames may belong to
// different rows.  The frames are those of mel_stream_kernel bit for bit (same windowed f32 samples, mel_dft_mag, mel_log_value);
// the chunk rows go to the row block tab[i].kRgChunk, so each emit group's chunk is contiguous.
__device__ __forceinline__ long long ragged_ll(const int* d, int lo) {
  return (long long)(((unsigned long long)(unsigned)d[lo + 1] << 32) | (unsigned)d[lo]);
}

// the call row owning frame job `job`: the last row whose first job is <= job (rows without frames share their successor's prefix)
__device__ __forceinline__ int ragged_row(const MelRaggedArgs& a, int job) {
  int lo = 0, hi = a.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.tab[mid * kRaggedWords + kRgJob] <= job) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// mel_stream_copy for row i of a ragged call: its chunk rows of earlier calls, its samples into its audio ring
__device__ inline void mel_ragged_copy(const MelRaggedArgs& a, int i) {
  const int* d = a.tab + (long long)i * kRaggedWords;
  const int slot = d[kRgSlot], rows = d[kRgRows], real = d[kRgReal], pos = d[kRgPos], f0 = d[kRgF0], m = d[kRgM];
  const float* mr = a.mring + (long long)slot * a.LM * a.nm;
  float* ch = a.chunk + (long long)d[kRgChunk] * rows * a.nm;
  for (int e = threadIdx.x; e < rows * a.nm; e += blockDim.x) {
    const int r = e / a.nm, mm = e - r * a.nm, src = pos + min(r, real - 1);
    if (src < f0) ch[e] = mr[(long long)(src & (a.LM - 1)) * a.nm + mm];
  }
  const long long r_prev = ragged_ll(d, kRgRecvLo);
  float* ar = a.aring + (long long)slot * a.LA;
  const float* w = a.wav + (long long)i * a.wstride;
  for (int j = threadIdx.x; j < m; j += blockDim.x) ar[(r_prev + j) & (a.LA - 1)] = w[j];
}

__global__ __launch_bounds__(1024) void mel_stream_ragged_kernel(const MelRaggedArgs a) {
  constexpr int F = kMelStreamFrames;
  extern __shared__ __attribute__((aligned(16))) double msm[];
  const int N = a.n_fft;
  for (int i = blockIdx.x; i < a.n; i += gridDim.x) mel_ragged_copy(a, i);
  const int job0 = blockIdx.x * F;
  if (job0 >= a.jobs) return;                                        // copy-only workgroups (the whole workgroup leaves)
  double* x = msm;                                                   // [N][F]
  double2* tw = reinterpret_cast<double2*>(msm + (size_t)N * F);     // [N]
  float* mag = reinterpret_cast<float*>(tw + N);                     // [F][cmag]
  int* row_of = reinterpret_cast<int*>(mag + (size_t)F * a.cmag);    // [F] call row of each frame
  // the frame's samples; j, its row and its position are uniform in the workgroup.  The choice between this call's samples and the
  // audio ring is data-dependent per sample: both loads are issued unconditionally at clamped addresses and the value is selected
  // (a load behind that branch would be serialised)
  for (int j = 0; j < F; ++j) {
    const int job = job0 + j;
    if (job >= a.jobs) {
      for (int k = threadIdx.x; k < N; k += blockDim.x) x[(size_t)k * F + j] = 0.0;
      continue;
    }
    const int i = ragged_row(a, job);
    const int* d = a.tab + (long long)i * kRaggedWords;
    const int f = d[kRgF0] + (job - d[kRgJob]), m = d[kRgM];
    const long long r_prev = ragged_ll(d, kRgRecvLo), total = ragged_ll(d, kRgTotalLo);
    const long long end = total < 0 ? LLONG_MAX : total;
    const float* wr = m > 0 ? a.wav + (long long)i * a.wstride : a.aring;     // (no samples: the clamped load reads a valid word)
    const float* ar = a.aring + (long long)d[kRgSlot] * a.LA;
    const long long base = (long long)f * a.hop - N / 2;                     // center=True, pad_mode='constant'
    const long long wlast = m > 0 ? m - 1 : 0;
    if (threadIdx.x == 0) row_of[j] = i;
    for (int k = threadIdx.x; k < N; k += blockDim.x) {
      const long long smp = base + k;
      const float xw = wr[min(max(smp - r_prev, 0ll), wlast)];
      const float xr = ar[smp & (a.LA - 1)];
      const float xs = smp >= r_prev ? xw : xr;
      x[(size_t)k * F + j] = (double)(smp >= 0 && smp < end ? xs * a.win[k] : 0.f);
    }
  }
  for (int t = threadIdx.x; t < N; t += blockDim.x) tw[t] = a.tw[t];
  __syncthreads();
  mel_dft_mag(x, tw, mag, N, a.nb, a.cmag, a.mag_eps);
  __syncthreads();
  for (int e = threadIdx.x; e < F * a.nm; e += blockDim.x) {
    const int j = e / a.nm, mm = e - j * a.nm, job = job0 + j;
    if (job >= a.jobs) continue;
    const int i = row_of[j];
    const int* d = a.tab + (long long)i * kRaggedWords;
    const int f = d[kRgF0] + (job - d[kRgJob]), rows = d[kRgRows], pos = d[kRgPos], real = d[kRgReal];
    const float v = mel_log_value(a.fb, a.lo, a.hi, mag + j * a.cmag, mm, a.cmag, a.eps, a.vmin, a.vmax, a.natural_log);
    a.mring[((long long)d[kRgSlot] * a.LM + (f & (a.LM - 1))) * a.nm + mm] = v;
    float* ch = a.chunk + (long long)d[kRgChunk] * rows * a.nm;
    for (int r = 0; r < rows; ++r)
      if (pos + min(r, real - 1) == f) ch[(long long)r * a.nm + mm] = v;
  }
}

// Rows of the emit groups' staged outputs into the caller's rows (call order); frames past a row's emit stay untouched.
__global__ __launch_bounds__(256) void wav_rows_scatter_kernel(const WavScatterArgs a) {
  const int i = blockIdx.x;
  const int* d = a.tab + (long long)i * kRaggedWords;
  const int e = d[kRgEmit], g = d[kRgGroup], k = d[kRgIndex];
  if (e == 0) return;
  const long long src = (long long)g * a.seg + (long long)k * e;      // the group's compact [rows][e] frames start at g * seg
  if (a.codes) for (int t = threadIdx.x; t < e; t += blockDim.x) a.codes[(long long)i * a.seg + t] = a.codes_src[(long long)(g + k) * a.seg + t];
  if (a.mel) for (int t = threadIdx.x; t < e * a.nm; t += blockDim.x) a.mel[(long long)i * a.seg * a.nm + t] = a.mel_src[src * a.nm + t];
  if (a.wav) for (int t = threadIdx.x; t < e * a.hop; t += blockDim.x) a.wav[(long long)i * a.seg * a.hop + t] = a.wav_src[src * a.hop + t];
}

void launch_mel_ragged(const MelRaggedArgs& a, hipStream_t st) {
  const int threads = std::min(1024, (a.nb + 63) / 64 * 64);
  if (a.jobs == 0) { hipLaunchKernelGGL(mel_stream_ragged_kernel, dim3(a.n), dim3(threads), 0, st, a); return; }
  const int blocks = std::max((a.jobs + kMelStreamFrames - 1) / kMelStreamFrames, std::min(a.n, 64));
  const size_t lds = mel_stream_lds_bytes(a.n_fft, a.cmag) + kMelStreamFrames * sizeof(int);
  if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)mel_stream_ragged_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  hipLaunchKernelGGL(mel_stream_ragged_kernel, dim3(blocks), dim3(threads), lds, st, a);
}

void launch_wav_scatter(const WavScatterArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(wav_rows_scatter_kernel, dim3(a.n), dim3(256), 0, st, a);
}
}  // namespace cnk

namespace {

// librosa.core.convert (htk=False): Slaney's Auditory Toolbox mel scale
double hz_to_mel(double f) {
  const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
  return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
double mel_to_hz(double m) {
  const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
  return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

}  // namespace

int conan_mel_frames(const conan_mel_cfg& m, int samples) {
  if (m.framing == 0) return 1 + samples / m.hop_size;
  const int padded = samples + 2 * ((m.fft_size - m.hop_size) / 2);
  return padded < m.fft_size ? 0 : (padded - m.fft_size) / m.hop_size + 1;
}

// Window, twiddle and filterbank tables of a mel configuration, built and uploaded on first use; returns their key prefix
// in vecs ("<key>.win", ".tw", ".fb", ".range").  Shared by conan_wav2mel and the streaming front-end (streams.hip).
std::string conan_ctx::mel_tables(const conan_mel_cfg& m) {
  const int N = m.fft_size, NB = N / 2 + 1, CM = (NB + 3) & ~3;
  const double fmin = m.fmin < 0 ? 0.0 : m.fmin, fmax = m.fmax < 0 ? m.sample_rate / 2.0 : m.fmax;
  char key[160];
  snprintf(key, sizeof(key), "fe.%d.%d.%d.%d.%g.%g", N, m.win_length, m.num_mels, m.sample_rate, fmin, fmax);
  const std::string k(key);
  if (!vecs.count(k + ".tw")) {
    // periodic Hann (scipy.signal.get_window('hann', win_length, fftbins=True)), centred in the FFT frame (pad_center)
    std::vector<float> win(N, 0.f);
    const int lp = (N - m.win_length) / 2;
    const double PI = 3.14159265358979323846;
    for (int i = 0; i < m.win_length; ++i) win[lp + i] = (float)(0.5 - 0.5 * std::cos(2.0 * PI * i / m.win_length));
    vecs[k + ".win"] = upload(win);
    // twiddles (cos, sin)(2 pi t / N) as f64 pairs (the sign of the sine is irrelevant for |.|)
    std::vector<float> tw((size_t)4 * N);
    for (int t = 0; t < N; ++t) {
      const double c = std::cos(2.0 * PI * t / N), sn = std::sin(2.0 * PI * t / N);
      memcpy(&tw[(size_t)4 * t], &c, 8); memcpy(&tw[(size_t)4 * t + 2], &sn, 8);
    }
    vecs[k + ".tw"] = upload(tw);
    // librosa.filters.mel(htk=False, norm='slaney', dtype=float32), plus each triangle's bin range
    std::vector<double> mel_f(m.num_mels + 2);
    const double m0 = hz_to_mel(fmin), m1 = hz_to_mel(fmax);
    for (int i = 0; i < m.num_mels + 2; ++i) mel_f[i] = mel_to_hz(m0 + (m1 - m0) * i / (m.num_mels + 1));
    std::vector<float> B((size_t)m.num_mels * CM, 0.f), range((size_t)2 * m.num_mels);
    for (int i = 0; i < m.num_mels; ++i) {
      const float enorm = (float)(2.0 / (mel_f[i + 2] - mel_f[i]));
      int lo = NB, hi = 0;
      for (int b = 0; b < NB; ++b) {
        const double f = (m.sample_rate / 2.0) * b / (NB - 1);
        const double lower = (f - mel_f[i]) / (mel_f[i + 1] - mel_f[i]), upper = (mel_f[i + 2] - f) / (mel_f[i + 2] - mel_f[i + 1]);
        float w = (float)std::max(0.0, std::min(lower, upper));
        w *= enorm;
        B[(size_t)i * CM + b] = w;
        if (w != 0.f) { lo = std::min(lo, b); hi = std::max(hi, b + 1); }
      }
      if (hi <= lo) { lo = 0; hi = 0; }
      const int32_t l32 = lo, h32 = hi;
      memcpy(&range[i], &l32, 4); memcpy(&range[(size_t)m.num_mels + i], &h32, 4);
    }
    vecs[k + ".fb"] = upload(B);
    vecs[k + ".range"] = upload(range);
  }
  return k;
}

float* conan_ctx::workspace(size_t floats, hipStream_t st) {
  if (floats > fe_ws_floats) {      // grow: the previous block is released once the stream has drained
    if (fe_ws) {
      HIP_CHECK(hipStreamSynchronize(st));
      for (size_t i = 0; i < allocs.size(); ++i) if (allocs[i] == fe_ws) { allocs.erase(allocs.begin() + i); break; }
      HIP_CHECK(hipFree(fe_ws));
      fe_ws = nullptr; fe_ws_floats = 0;
    }
    fe_ws = dev_alloc(floats, false); fe_ws_floats = floats;
  }
  return fe_ws;
}

void conan_ctx::wav2mel(const conan_mel_cfg& m, const float* wav, int n, int samples, float* mel_out, hipStream_t st) {
  using ch::Error;
  if (m.fft_size < 64 || (m.fft_size & (m.fft_size - 1)) || m.fft_size > 2048 || m.hop_size < 1 || m.win_length < 1 || m.win_length > m.fft_size ||
      m.num_mels < 1 || m.num_mels > 512 || m.sample_rate < 1 || !(m.eps > 0.f))
    throw Error(CONAN_ERR_INVALID, "mel front-end configuration");
  if (n < 1 || samples < 1) throw Error(CONAN_ERR_INVALID, "wav2mel batch / samples");
  if (m.framing < 0 || m.framing > 1 || !(m.mag_eps >= 0.f)) throw Error(CONAN_ERR_INVALID, "mel front-end framing / mag_eps");
  // reflect padding needs pad < samples (torch raises otherwise); frames = (samples + 2 pad - n_fft) / hop + 1
  if (m.framing == 1 && ((m.fft_size - m.hop_size) / 2 >= samples || m.hop_size > m.fft_size)) throw Error(CONAN_ERR_INVALID, "wav2mel: reflect padding longer than the signal");
  const int N = m.fft_size, NB = N / 2 + 1, CM = (NB + 3) & ~3;
  const std::string k = mel_tables(m);
  const int frames = conan_mel_frames(m, samples);
  if (frames < 1) throw Error(CONAN_ERR_INVALID, "wav2mel: signal shorter than one frame");
  const long long rows = (long long)n * frames;
  if (rows > (1ll << 19)) throw Error(CONAN_ERR_INVALID, "wav2mel: more than 2^19 frames in one call");
  // workspace: frames [rows][N] | magnitude [rows][CM]
  const size_t need = (size_t)rows * ((size_t)N + CM);
  float* fr = workspace(need, st); float* mag = fr + (size_t)rows * N;
  { cnk::FrameArgs a{wav, vec(k + ".win"), fr, n, samples, frames, m.hop_size, N, m.framing}; hipLaunchKernelGGL(cnk::stft_frames_kernel, dim3((unsigned)rows), dim3(256), 0, st, a); }
  { cnk::DftArgs a{fr, reinterpret_cast<const double2*>(vec(k + ".tw")), mag, N, NB, CM, m.mag_eps};
    hipLaunchKernelGGL(cnk::dft_mag_kernel, dim3((unsigned)rows, (unsigned)((CM + 255) / 256)), dim3(256), (size_t)N * 24, st, a); }
  { const float* rg = vec(k + ".range");
    cnk::MelArgs a{mag, vec(k + ".fb"), reinterpret_cast<const int*>(rg), reinterpret_cast<const int*>(rg) + m.num_mels, mel_out, rows, m.num_mels, CM, m.eps, m.vmin, m.vmax, m.natural_log};
    const long long total = rows * m.num_mels;
    hipLaunchKernelGGL(cnk::mel_log_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a); }
}
