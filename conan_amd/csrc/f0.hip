// Source-pitch following (include/conan_hip.h, conan_f0_cfg): the YIN tracker's kernel, the whole-signal entry point conan_f0 and the
// host side of conan_streams_set_pitch_follow.  The wav-in steps launch the kernel behind their front-end launch (f0::WavStage
// below); the decoder step reads what it wrote through PitchHeadArgs::trk_f0 / trk_uv (rowops.h, pitch_law).
#include <cmath>

#include "streams.h"

namespace cnk {

constexpr int kF0Threads = 384;      // one lag per thread at the defaults (tmax + 2 = 322 difference sums)
constexpr int kF0Chunk = 8;          // lags per thread in the running sum

// One (row, frame) job per workgroup.  The frame sits in LDS as doubles; thread j takes lags j, j + 384, ...: x[k] is an LDS broadcast
// and x[k + t] is consecutive over the lanes.  Every sum has one order, fixed by (n_fft, tmax) alone - four interleaved partial sums
// over k, then (s0 + s1) + (s2 + s3) - so a frame's bits do not depend on the launch it is part of.
__global__ __launch_bounds__(kF0Threads) void f0_yin_kernel(const F0Args a) {
  __shared__ double x[kF0MaxFft];
  __shared__ double d[kF0MaxFft / 2 + 8];        // d(t), then d'(t), t = 0 .. tmax + 1 (d[0]: the gate's power sum)
  __shared__ double tot[(kF0MaxFft / 2 + 8) / kF0Chunk + 1];
  __shared__ int pick_s;
  const int job = blockIdx.x, tid = threadIdx.x, N = a.n_fft;
  if (job >= a.jobs) return;
  // the job's row: uniform in the workgroup
  F0Row r = a.uni;
  if (a.tab) {
    int i = 0;
    for (int q = 1; q < a.rows; ++q) i = a.tab[q].job0 <= job ? q : i;      // (rows in ascending job order; rows without frames never match last)
    r = a.tab[i];
  } else {
    const int i = job / a.uni.nframes;
    r.src_off = a.uni.src_off * i; r.job0 = a.uni.nframes * i; r.out_off = r.job0;
  }
  const int j = job - r.job0, f = r.f_first + j;
  const int tmin = r.tmin, tmax = r.tmax, W = N - tmax - 1;
  // the frame: loads are unconditional at clamped addresses, the zero padding is selected after them
  const long long base = (long long)f * a.hop - N / 2, last = r.valid > 0 ? r.valid - 1 : 0;
  const float* src = a.src + r.src_off;
  for (int k = tid; k < N; k += kF0Threads) {
    const long long s = base + k;
    const long long sc = s < 0 ? 0 : (s > last ? last : s);
    const float v = src[sc & (long long)r.mask];
    x[k] = s >= 0 && s < r.valid ? (double)v : 0.0;
  }
  if (tid == 0) pick_s = 0x7fffffff;
  __syncthreads();
  // difference function in the difference form; lag 0 compares with nothing: d[0] = sum x[k]^2
  for (int t = tid; t <= tmax + 1; t += kF0Threads) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const double keep = t ? 1.0 : 0.0;
    int k = 0;
    for (; k + 3 < W; k += 4) {
      const double e0 = x[k] - keep * x[k + t], e1 = x[k + 1] - keep * x[k + 1 + t], e2 = x[k + 2] - keep * x[k + 2 + t], e3 = x[k + 3] - keep * x[k + 3 + t];
      s0 = fma(e0, e0, s0); s1 = fma(e1, e1, s1); s2 = fma(e2, e2, s2); s3 = fma(e3, e3, s3);
    }
    for (; k < W; ++k) { const double e = x[k] - keep * x[k + t]; s0 = fma(e, e, s0); }
    d[t] = (s0 + s1) + (s2 + s3);
  }
  __syncthreads();
  // running sum over the lags 1 .. tmax + 1: chunks of kF0Chunk lags, a chunk's start = the earlier chunks' totals added in ascending order
  const int nlag = tmax + 1, nchunk = (nlag + kF0Chunk - 1) / kF0Chunk;
  for (int c = tid; c < nchunk; c += kF0Threads) {
    double s = 0.0;
    for (int u = 0; u < kF0Chunk; ++u) { const int t = 1 + c * kF0Chunk + u; if (t <= nlag) s += d[t]; }
    tot[c] = s;
  }
  __syncthreads();
  const double power = d[0];
  double dn[kF0Chunk];
  for (int c = tid; c < nchunk; c += kF0Threads) {      // (one chunk per thread up to tmax = 3071)
    double run = 0.0;
    for (int q = 0; q < c; ++q) run += tot[q];
    for (int u = 0; u < kF0Chunk; ++u) {
      const int t = 1 + c * kF0Chunk + u;
      double v = 1.0;
      if (t <= nlag) { run += d[t]; v = run > 0.0 ? d[t] * (double)t / run : 1.0; }
      dn[u] = v;
    }
    for (int u = 0; u < kF0Chunk; ++u) { const int t = 1 + c * kF0Chunk + u; if (t <= nlag) d[t] = dn[u]; }      // (a chunk is read and written by its own thread only)
  }
  __syncthreads();
  // the first lag under the threshold: a minimum over lag indices
  for (int t = tmin + tid; t <= tmax; t += kF0Threads)
    if (d[t] < r.thr) atomicMin(&pick_s, t);
  __syncthreads();
  if (tid == 0) {
    int t = pick_s;
    float v = 0.f, uv = 1.f;
    const bool gated = power / (double)W < r.gate;
    if (t <= tmax && !gated) {
      while (t + 1 <= tmax && d[t + 1] < d[t]) ++t;
      const double p0 = d[t - 1], p1 = d[t], p2 = d[t + 1];
      const double den = (p0 - 2.0 * p1) + p2;
      double off = den > 0.0 ? 0.5 * (p0 - p2) / den : 0.0;
      off = off < -1.0 ? -1.0 : (off > 1.0 ? 1.0 : off);
      v = (float)log2(a.sr / ((double)t + off));
      uv = 0.f;
    }
    a.out_f0[r.out_off + j] = v;
    a.out_uv[r.out_off + j] = uv;
  }
}

void launch_f0(const F0Args& a, hipStream_t st) {
  if (a.jobs < 1) return;
  hipLaunchKernelGGL(f0_yin_kernel, dim3(a.jobs), dim3(kF0Threads), 0, st, a);
}

}  // namespace cnk

namespace f0 {

// tmin = floor(sr / fmax), tmax = ceil(sr / fmin) of a checked cfg at the model rate
Lags lags(const conan_f0_cfg& c, double sr) { return Lags{(int)std::floor(sr / (double)c.fmax), (int)std::ceil(sr / (double)c.fmin)}; }

// sr > 0: also the limits that depend on the rate and the frame (tmin >= 2, tmax <= n_fft / 2); the stream setter, which has no frame
// yet, passes the largest one a wav-in step accepts and the step checks its own
void check_cfg(const conan_f0_cfg& c, double sr, int n_fft, const char* who) {
  const std::string w = std::string(who) + ": ";
  if (c.enabled != 0 && c.enabled != 1) throw Error(CONAN_ERR_INVALID, w + "conan_f0_cfg.enabled must be 0 or 1");
  if (!c.enabled) return;      // (the other fields are ignored)
  if (c.reserved != 0) throw Error(CONAN_ERR_INVALID, w + "conan_f0_cfg.reserved must be 0");
  if (!std::isfinite(c.fmin) || !std::isfinite(c.fmax) || !(c.fmin > 0.f) || !(c.fmin < c.fmax)) throw Error(CONAN_ERR_INVALID, w + "fmin and fmax must be finite with 0 < fmin < fmax");
  if (!std::isfinite(c.threshold) || !(c.threshold > 0.f) || !(c.threshold < 1.f)) throw Error(CONAN_ERR_INVALID, w + "threshold must be in (0, 1)");
  if (!std::isfinite(c.floor_db)) throw Error(CONAN_ERR_INVALID, w + "floor_db must be finite");
  if (!(sr > 0.0)) return;
  const Lags l = lags(c, sr);
  if (l.tmin < 2) throw Error(CONAN_ERR_INVALID, w + "fmax is above half the sample rate (floor(sr / fmax) < 2)");
  if (l.tmax > n_fft / 2) throw Error(CONAN_ERR_INVALID, w + "fmin needs lags beyond half the frame (ceil(sr / fmin) > fft_size / 2 = " + std::to_string(n_fft / 2) + ")");
}

cnk::F0Row row(const conan_f0_cfg& c, double sr) {
  cnk::F0Row r;
  memset(&r, 0, sizeof(r));
  const Lags l = lags(c, sr);
  r.tmin = l.tmin; r.tmax = l.tmax; r.thr = (double)c.threshold; r.gate = std::pow(10.0, (double)c.floor_db / 10.0);
  return r;
}

static void check_mel(const conan_mel_cfg& m, const char* who) {
  const std::string w = std::string(who) + ": ";
  if (m.fft_size < 64 || (m.fft_size & (m.fft_size - 1)) || m.fft_size > cnk::kF0MaxFft) throw Error(CONAN_ERR_INVALID, w + "fft_size must be a power of two in [64, 2048]");
  if (m.hop_size < 1) throw Error(CONAN_ERR_INVALID, w + "hop_size must be positive");
  if (m.sample_rate != 50 * m.hop_size) throw Error(CONAN_ERR_INVALID, w + "sample_rate must be 50 * hop_size (20 ms frames)");
}

void whole(conan_ctx* ctx, const conan_mel_cfg* mel, const conan_f0_cfg* cfg, const float* wav_dev, int n, int samples, float* f0_out_dev, float* uv_out_dev,
           int32_t* frames_out, void* stream) {
  if (!ctx || !mel || !cfg || !wav_dev || !f0_out_dev || !uv_out_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  check_mel(*mel, "conan_f0");
  if (!cfg->enabled) throw Error(CONAN_ERR_INVALID, "conan_f0: cfg.enabled must be 1");
  const double sr = 50.0 * mel->hop_size;
  check_cfg(*cfg, sr, mel->fft_size, "conan_f0");
  if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, "conan_f0: n must be in 1 .. 65535");
  if (samples < 1) throw Error(CONAN_ERR_INVALID, "conan_f0: an utterance needs at least one sample");
  const int frames = 1 + samples / mel->hop_size;
  if ((long long)n * frames > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_f0: too many frames in one call");
  if (frames_out) *frames_out = frames;
  HIP_CHECK(hipSetDevice(ctx->device));
  cnk::F0Args a;
  memset(&a, 0, sizeof(a));
  a.src = wav_dev; a.out_f0 = f0_out_dev; a.out_uv = uv_out_dev; a.tab = nullptr; a.rows = n;
  a.uni = row(*cfg, sr);
  a.uni.src_off = samples; a.uni.valid = samples; a.uni.mask = -1; a.uni.f_first = 0; a.uni.nframes = frames;
  a.jobs = n * frames; a.n_fft = mel->fft_size; a.hop = mel->hop_size; a.sr = sr;
  cnk::launch_f0(a, (hipStream_t)stream);
}

void set_follow(conan_streams* s, const int32_t* slots, int n, const conan_f0_cfg* cfg, void* stream) {
  if (!s || !slots || !cfg) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, 0.0, 0, "conan_streams_set_pitch_follow");      // (before the handle is touched, before any GPU use)
  if (!s->wav_in.fe_audio) throw Error(CONAN_ERR_STATE, "conan_streams_set_pitch_follow: the stream-set has no streaming front-end (all three models)");
  check_cfg(*cfg, 50.0 * s->ctx->hop, cnk::kF0MaxFft, "conan_streams_set_pitch_follow");
  wavio::check_slot_list(s, slots, n);
  if (!cfg->enabled && !s->follow.allocated()) return;      // a stream-set that never followed: nothing to allocate, nothing to write
  hipStream_t st = s->enter(stream);
  s->follow_init();
  s->follow.store(slots, n, *cfg);
  std::vector<conan_pitch_cfg> cfgs((size_t)n);
  for (int i = 0; i < n; ++i) cfgs[i] = s->pt_cfg[slots[i]];
  s->pitch_write(slots, n, cfgs.data(), st);      // (the follow flag is the sixth word of the slots' pitch-table entries)
}

// the contour the last wav-in call handed the decoder, in call order: rows of `seg`, zeros where a row did not follow or did not emit
void contour(conan_streams* s, float* f0_dev, float* uv_dev, void* stream) {
  if (!s || !f0_dev || !uv_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  hipStream_t st = wavio::begin_last_call(s, "conan_step_wav_contour", stream);
  const int seg = s->ctx->cfg.emf_segment, n = s->wav_in.fe_last_n;
  copy_last_rows(s->follow.last, f0_dev, n, seg, s->follow.ct_f0, seg, 0, st);
  copy_last_rows(s->follow.last, uv_dev, n, seg, s->follow.ct_uv, seg, 0, st);
}

void WavStage::plan(const conan_streams* s, const WavCall& c) {
  if (s->follow.n_on < 1) return;
  const double sr = 50.0 * c.hop;
  for (int i = 0; i < c.n; ++i) {
    if (!s->follow.on(c.slots[i])) continue;
    if (c.mel.sample_rate != 50 * c.hop) throw Error(CONAN_ERR_INVALID, c.who + ": slot " + std::to_string(c.slots[i]) + " follows the source pitch: conan_mel_cfg.sample_rate must be 50 * hop_size");
    check_cfg(s->follow.cfg[c.slots[i]], sr, c.N, c.who.c_str());
  }
  group.assign(c.groups.size(), 0);
  c.each_chunk_row([&](int g, int, int i, int at) {
    const int slot = c.slots[i];
    if (!s->follow.on(slot)) return;
    const FePlan& p = c.pl[i];
    if (p.R - std::max(0ll, (long long)p.pos * c.hop - c.N / 2) > s->wav_in.fe_LA)
      throw Error(CONAN_ERR_UNSUPPORTED, c.who + ": slot " + std::to_string(slot) + " follows the source pitch: the chunk's frames have left the audio ring at this fft_size");
    cnk::F0Row r = row(s->follow.cfg[slot], sr);
    r.src_off = (long long)slot * s->wav_in.fe_LA; r.valid = p.R; r.mask = s->wav_in.fe_LA - 1;
    r.f_first = p.pos; r.nframes = p.emit; r.job0 = jobs; r.out_off = at * c.seg;
    jobs += p.emit;
    flops += 3.0 * r.nframes * (double)(c.N - r.tmax - 1) * (r.tmax + 2);
    rows.push_back(r);
    last.push_back({i, 0, at, p.emit});
    group[g] = 1;
    if (s->reg.on(slot)) reg_rows.push_back(reg::wav_row(s, slot, r.out_off, p.emit));
  });
}

// the tracker, behind the front-end launch: the call's samples are in the audio rings
void WavStage::enqueue(conan_streams* s, const WavCall& c, hipStream_t cst, FrontWork& front, std::vector<conan_streams::OutPlan>&) {
  if (rows.empty()) return;
  q = s->follow.sets.begin(rows.data(), (int)rows.size(), cst);
  for (LastRow& r : last) r.set = q;
  ct_f0 = s->follow.ct_f0[q]; ct_uv = s->follow.ct_uv[q];
  cnk::F0Args a;
  memset(&a, 0, sizeof(a));
  a.src = s->wav_in.fe_audio; a.out_f0 = s->follow.ct_f0[q]; a.out_uv = s->follow.ct_uv[q];
  a.tab = s->follow.sets.rows[q]; a.rows = (int)rows.size(); a.jobs = jobs; a.n_fft = c.N; a.hop = c.hop; a.sr = 50.0 * c.hop;
  front.at[kFrF0] = [s, a, flops = flops](hipStream_t st) { s->profiled("f0_yin_kernel", flops, st, [&] { cnk::launch_f0(a, st); }); };
  reg::wav_enqueue(s, reg_rows, q, cst, front);
}

void WavStage::commit(conan_streams* s, hipStream_t dec, hipStream_t) {
  if (!rows.empty()) s->follow.sets.end(q, dec);      // (behind the call's last decoder step, the contour's last reader)
  s->follow.last = std::move(last);
  reg::wav_commit(s, reg_rows);
}

}  // namespace f0

void conan_streams::follow_init() {
  if (follow.ct_f0[0]) return;
  const size_t floats = (size_t)max_slots * ctx->cfg.emf_segment;
  for (int q = 0; q < kStageSets; ++q) { follow.ct_f0[q] = alloc(floats); follow.ct_uv[q] = alloc(floats); }      // (counted by state_bytes)
  follow.sets.init(max_slots, allocs);
  follow.assign(max_slots);
}
