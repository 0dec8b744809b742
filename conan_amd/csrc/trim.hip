// Silence trimming (include/conan_hip.h, conan_trim_cfg): the offline half of source activity.  conan_trim_silence runs the detector's
// kernel (activity.hip, unchanged: one table row per signal row with its own length) where the caller brings no flags, then the plan
// kernel - smoothing, dilation and the kept frames' offsets, all differences or prefixes of integer sums - and the gather kernel, which
// moves the kept frames' samples and zero-fills the rest of the row.
#include <climits>
#include <cstdint>

#include "streams.h"

namespace cnk {

constexpr int kTrimWaves = kTrimThreads / 64;

// The inclusive sum of v over the workgroup's lanes 0 .. tid, and the workgroup's total: a wave64 shuffle scan, the waves' totals
// through LDS (register.hip's scan).  Every lane of the workgroup calls it.
__device__ __forceinline__ long long trim_scan(long long v, long long* wave_s, const int lane, const int wave, long long& total) {
  for (int d = 1; d < 64; d <<= 1) {
    const long long v2 = __shfl_up(v, d);
    if (lane >= d) v += v2;
  }
  if (lane == 63) wave_s[wave] = v;
  __syncthreads();
  total = 0;
  for (int w = 0; w < kTrimWaves; ++w) {
    const long long t = wave_s[w];
    if (w < wave) v += t;
    total += t;
  }
  __syncthreads();      // (the next scan writes wave_s again)
  return v;
}

// One row per workgroup; three passes over the row's frames in tiles of kTrimThreads, a lane per frame, each an integer scan with the
// tiles' totals in a register carry.  Pass 1 writes the prefix of the flags (pa[f + 1] = act[0] + .. + act[f]), pass 2 forms S[f] as a
// difference of two of its entries - the window reaches into other tiles, which is why the prefix goes through global memory: the row's
// own workgroup wrote it, and the barrier between the passes makes it visible - and writes the prefix of m1, pass 3 forms m2 the same
// way and scans cnt * m2.  The sums are exact integers, so neither the tile width nor the wave count nor the launch's other rows show
// in a result.  Every load is unconditional at a clamped frame; the tail is selected after it.
__global__ __launch_bounds__(kTrimThreads) void trim_plan_kernel(const TrimArgs a) {
  __shared__ long long wave_s[kTrimWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = blockIdx.x;
  if (row >= a.n) return;
  const long long len = a.lens[row];      // uniform in the workgroup
  const int hop = a.hop;
  const int F = 1 + (int)(len / hop);
  const int* act = a.act + (long long)row * a.act_ld;
  int* pa = a.pa + (long long)row * a.pre_ld;
  int* pb = a.pb + (long long)row * a.pre_ld;
  if (tid == 0) { pa[0] = 0; pb[0] = 0; }
  long long carry = 0, total;
  for (int base = 0; base < F; base += kTrimThreads) {
    const int f = base + tid, fc = f < F ? f : F - 1;
    const int v = act[fc];
    const long long k = trim_scan(f < F && v != 0 ? 1 : 0, wave_s, lane, wave, total);
    if (f < F) pa[f + 1] = (int)(carry + k);
    carry += total;
  }
  __syncthreads();
  const int wl = (a.w - 1) / 2, wr = a.w / 2;
  carry = 0;
  for (int base = 0; base < F; base += kTrimThreads) {
    const int f = base + tid, fc = f < F ? f : F - 1;
    const int lo = fc > wl ? fc - wl : 0, hi = F - 1 - fc > wr ? fc + wr : F - 1;
    const int S = pa[hi + 1] - pa[lo];
    const long long k = trim_scan(f < F && 2ll * S > (long long)a.w ? 1 : 0, wave_s, lane, wave, total);
    if (f < F) pb[f + 1] = (int)(carry + k);
    carry += total;
  }
  __syncthreads();
  const int sl = a.s - 1 - a.s / 2, sr = a.s / 2;
  int* mask = a.mask ? a.mask + (long long)row * a.mask_ld : nullptr;
  long long* off = a.off + (long long)row * a.off_ld;
  carry = 0;
  for (int base = 0; base < F; base += kTrimThreads) {
    const int f = base + tid, fc = f < F ? f : F - 1;
    const int lo = fc > sl ? fc - sl : 0, hi = F - 1 - fc > sr ? fc + sr : F - 1;
    const bool m2 = f < F && pb[hi + 1] - pb[lo] > 0;
    const long long end = (long long)(fc + 1) * hop, start = (long long)fc * hop;
    const long long cnt = m2 ? (end < len ? end : len) - start : 0;
    const long long k = trim_scan(cnt, wave_s, lane, wave, total);
    if (f < F) {
      if (mask) mask[f] = m2 ? 1 : 0;
      off[f] = m2 ? carry + k - cnt : -1;
    }
    carry += total;
  }
  if (tid == 0) a.out_len[row] = carry;
}

// A workgroup per tile of kTrimGatherFrames frames of one row; a lane takes four consecutive source words at a time (words, not floats:
// the move is a bit copy).  Where the row's base is 16-byte aligned the four words are one load, and where they lie in one kept frame
// whose destination is aligned too they are one store - always, when hop, ld and out_ld are multiples of 4 and the bases are aligned,
// since every kept frame in front of a frame is whole and off[f] is then a multiple of hop.  Everything else - an odd stride, the
// row's last words, a hop that is no multiple of 4 - moves as single words.  The loads are unconditional at clamped addresses and the
// words are selected afterwards; only a tile's edge lanes load again behind a branch.  The same lanes zero the destination words
// [out_len, len) of their tile: the moved samples all land under out_len, so no word has two writers.
__global__ __launch_bounds__(kTrimGatherThreads) void trim_gather_kernel(const TrimArgs a) {
  const int row = blockIdx.y, tid = threadIdx.x;
  const long long len = a.lens[row];      // uniform in the workgroup; <= 2^30
  const int hop = a.hop;
  const long long ta = (long long)blockIdx.x * kTrimGatherFrames * hop;
  if (ta >= len) return;
  const long long tb = ta + (long long)kTrimGatherFrames * hop < len ? ta + (long long)kTrimGatherFrames * hop : len;
  const int F = 1 + (int)(len / hop);
  const unsigned* x = reinterpret_cast<const unsigned*>(a.wav) + (long long)row * a.ld;
  unsigned* y = reinterpret_cast<unsigned*>(a.out) + (long long)row * a.out_ld;
  const long long* off = a.off + (long long)row * a.off_ld;
  const long long out_len = a.out_len[row];
  const bool xa = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && len >= 4;      // uniform
  for (long long s0 = ((ta >> 2) + tid) * 4; s0 < tb; s0 += 4ll * kTrimGatherThreads) {
    const bool full = s0 >= ta && s0 + 3 < tb;
    uint4 q = make_uint4(0u, 0u, 0u, 0u);
    if (xa) q = *reinterpret_cast<const uint4*>(x + (full ? s0 : 0));
    unsigned v[4] = {q.x, q.y, q.z, q.w};
    const int f0 = (int)((unsigned)s0 / (unsigned)hop);      // (s0 < len: f0 <= F - 1)
    const int f3r = (int)((unsigned)(s0 + 3) / (unsigned)hop), f3 = f3r < F ? f3r : F - 1;
    const long long o0 = off[f0], o3 = off[f3];
    const int k0 = (int)(s0 - (long long)f0 * hop);
    if (!(xa && full)) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = x[s0 + e < len ? s0 + e : len - 1];
    }
    if (full && f3r == f0 && o0 >= 0 && (reinterpret_cast<uintptr_t>(y + o0 + k0) & 15) == 0) {
      *reinterpret_cast<uint4*>(y + o0 + k0) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long long se = s0 + e;
        if (se >= ta && se < tb) {
          const int fe = (int)((unsigned)se / (unsigned)hop);
          const long long oe = fe == f0 ? o0 : (fe == f3 ? o3 : off[fe]);      // (a third frame only where hop < 3)
          if (oe >= 0) y[oe + (se - (long long)fe * hop)] = v[e];
        }
      }
    }
    if (full && s0 >= out_len && (reinterpret_cast<uintptr_t>(y + s0) & 15) == 0) {
      *reinterpret_cast<uint4*>(y + s0) = make_uint4(0u, 0u, 0u, 0u);
    } else if (s0 + 3 >= out_len) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long long se = s0 + e;
        if (se >= ta && se < tb && se >= out_len) y[se] = 0u;
      }
    }
  }
}

void launch_trim_plan(const TrimArgs& a, hipStream_t st) {
  if (a.n < 1) return;
  hipLaunchKernelGGL(trim_plan_kernel, dim3(a.n), dim3(kTrimThreads), 0, st, a);
}

void launch_trim_gather(const TrimArgs& a, hipStream_t st) {
  if (a.n < 1 || a.tiles < 1 || !a.out) return;
  hipLaunchKernelGGL(trim_gather_kernel, dim3(a.tiles, a.n), dim3(kTrimGatherThreads), 0, st, a);
}

}  // namespace cnk

namespace trim {

constexpr int64_t kMaxSamples = 1ll << 30, kMaxStride = 1ll << 40, kMaxWidth = 65536;

static size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

void check_cfg(const conan_trim_cfg& c, const char* who) {
  const std::string w = std::string(who) + ": ";
  if (c.smooth_frames < 1 || c.smooth_frames > kMaxWidth) throw Error(CONAN_ERR_INVALID, w + "conan_trim_cfg.smooth_frames must be in 1 .. 65536");
  if (c.max_silence_frames < 0 || c.max_silence_frames > kMaxWidth) throw Error(CONAN_ERR_INVALID, w + "conan_trim_cfg.max_silence_frames must be in 0 .. 65536");
  if (c.reserved[0] || c.reserved[1]) throw Error(CONAN_ERR_INVALID, w + "the reserved words must be 0");
}

// The rows of the detector's table for signal rows of their own lengths: row i reads lens[i] samples at i * ld and writes its
// 1 + lens[i] / hop flags and levels at i * frame_ld (host only).
void detector_rows(const conan_activity_cfg& cfg, const int64_t* lens, int n, int hop, int64_t ld, int64_t frame_ld, cnk::ActRow* rows) {
  const cnk::ActRow proto = act::row(cfg);
  for (int i = 0; i < n; ++i) {
    rows[i] = proto;
    rows[i].src_off = (long long)i * ld; rows[i].valid = lens[i]; rows[i].out_off = (long long)i * frame_ld; rows[i].lvl_off = rows[i].out_off;
    rows[i].nframes = 1 + (int)(lens[i] / hop);
  }
}

// Everything conan_trim_silence refuses, before a handle is touched (host only; ctx is compared with null, never read).
void check_args(const conan_ctx* ctx, const conan_mel_cfg* mel, const conan_activity_cfg* act_cfg, const conan_trim_cfg* cfg, const float* wav_dev, int64_t ld,
                int n, int64_t samples, const int64_t* lengths, const int32_t* act_in_dev, int64_t act_ld, const float* out_dev, int64_t out_ld,
                const int32_t* mask_out_dev, const int64_t* offset_out_dev, int64_t frame_ld) {
  const std::string w = "conan_trim_silence: ";
  if (!ctx || !mel || !cfg || !wav_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  if ((act_cfg != nullptr) == (act_in_dev != nullptr)) throw Error(CONAN_ERR_INVALID, w + "exactly one of act_cfg (run the detector) and act_in_dev (the caller's flags) must be given");
  act::check_mel(*mel, "conan_trim_silence");
  if (act_cfg) {
    act::check_cfg(*act_cfg, "conan_trim_silence");
    if (!act_cfg->mode) throw Error(CONAN_ERR_INVALID, w + "act_cfg.mode must be 1 or 2");
  }
  check_cfg(*cfg, "conan_trim_silence");
  if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, w + "n must be in 1 .. 65535");
  if (samples < 1 || samples > kMaxSamples) throw Error(CONAN_ERR_INVALID, w + "samples must be in 1 .. 2^30");
  if (ld < samples || ld > kMaxStride) throw Error(CONAN_ERR_INVALID, w + "ld must be in samples .. 2^40");
  if (out_dev && (out_ld < samples || out_ld > kMaxStride)) throw Error(CONAN_ERR_INVALID, w + "out_ld must be in samples .. 2^40");
  int64_t longest = samples;
  if (lengths) {
    longest = 0;
    for (int i = 0; i < n; ++i) {
      if (lengths[i] < 1 || lengths[i] > samples) throw Error(CONAN_ERR_INVALID, w + "row " + std::to_string(i) + ": lengths must be in 1 .. samples");
      longest = std::max(longest, lengths[i]);
    }
  }
  const int64_t frames = 1 + longest / mel->hop_size;
  if (act_in_dev && (act_ld < frames || act_ld > kMaxStride)) throw Error(CONAN_ERR_INVALID, w + "act_ld must cover the 1 + len / hop frames of every row");
  if ((mask_out_dev || offset_out_dev) && (frame_ld < frames || frame_ld > kMaxStride)) throw Error(CONAN_ERR_INVALID, w + "frame_ld must cover the 1 + len / hop frames of every row");
  if (out_dev) {      // a parallel move towards lower addresses races
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(wav_dev), x1 = x0 + ((uint64_t)(n - 1) * (uint64_t)ld + (uint64_t)samples) * sizeof(float);
    const uintptr_t y0 = reinterpret_cast<uintptr_t>(out_dev), y1 = y0 + ((uint64_t)(n - 1) * (uint64_t)out_ld + (uint64_t)samples) * sizeof(float);
    if (x0 < y1 && y0 < x1) throw Error(CONAN_ERR_INVALID, w + "out_dev must not overlap wav_dev");
  }
}

void whole(conan_ctx* ctx, const conan_mel_cfg* mel, const conan_activity_cfg* act_cfg, const conan_trim_cfg* cfg, const float* wav_dev, int64_t ld, int n,
           int64_t samples, const int64_t* lengths, const int32_t* act_in_dev, int64_t act_ld, float* out_dev, int64_t out_ld, int32_t* mask_out_dev,
           int64_t* offset_out_dev, int64_t frame_ld, int64_t* out_len_dev, void* stream) {
  check_args(ctx, mel, act_cfg, cfg, wav_dev, ld, n, samples, lengths, act_in_dev, act_ld, out_dev, out_ld, mask_out_dev, offset_out_dev, frame_ld);
  const int hop = mel->hop_size;
  HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  // the table (lengths | detector rows) and the scratch arrays behind it, in the context's workspace
  int64_t longest = samples;
  if (lengths) { longest = 0; for (int i = 0; i < n; ++i) longest = std::max(longest, lengths[i]); }
  const size_t frames = (size_t)(1 + longest / hop);
  const size_t o_lens = 0, o_rows = align16(o_lens + (size_t)n * sizeof(int64_t)), table = align16(o_rows + (act_cfg ? (size_t)n * sizeof(cnk::ActRow) : 0));
  const size_t o_act = table, o_lvl = o_act + (act_cfg ? align16((size_t)n * frames * sizeof(int)) : 0),
               o_pa = o_lvl + (act_cfg ? align16((size_t)n * frames * sizeof(int)) : 0), o_pb = o_pa + align16((size_t)n * (frames + 1) * sizeof(int)),
               o_off = o_pb + align16((size_t)n * (frames + 1) * sizeof(int)), o_len = o_off + (offset_out_dev ? 0 : align16((size_t)n * frames * sizeof(int64_t))),
               total = o_len + (out_len_dev ? 0 : align16((size_t)n * sizeof(int64_t)));
  char* ws = reinterpret_cast<char*>(ctx->workspace((total + 3) / 4, st));
  char* h = static_cast<char*>(ctx->loud_stage.take(table));
  int64_t* lens = reinterpret_cast<int64_t*>(h + o_lens);
  for (int i = 0; i < n; ++i) lens[i] = lengths ? lengths[i] : samples;
  if (act_cfg) detector_rows(*act_cfg, lens, n, hop, ld, (int64_t)frames, reinterpret_cast<cnk::ActRow*>(h + o_rows));
  HIP_CHECK(hipMemcpyAsync(ws, h, table, hipMemcpyHostToDevice, st));
  ctx->loud_stage.sent(st);
  if (act_cfg) {
    cnk::ActArgs d;
    memset(&d, 0, sizeof(d));
    d.src = wav_dev; d.act = reinterpret_cast<int*>(ws + o_act); d.lvl = reinterpret_cast<int*>(ws + o_lvl);
    d.tab = reinterpret_cast<const cnk::ActRow*>(ws + o_rows); d.rows = n; d.n_fft = mel->fft_size; d.hop = hop;
    d.long_rows = frames > (size_t)(4 * (cnk::kActStreamThreads / 64));
    cnk::launch_activity(d, st);
    HIP_CHECK(hipGetLastError());
  }
  cnk::TrimArgs a;
  memset(&a, 0, sizeof(a));
  a.wav = wav_dev; a.out = out_dev; a.ld = ld; a.out_ld = out_ld;
  a.act = act_cfg ? reinterpret_cast<const int*>(ws + o_act) : act_in_dev; a.act_ld = act_cfg ? (long long)frames : act_ld;
  a.mask = mask_out_dev; a.mask_ld = frame_ld;
  a.off = offset_out_dev ? reinterpret_cast<long long*>(offset_out_dev) : reinterpret_cast<long long*>(ws + o_off); a.off_ld = offset_out_dev ? frame_ld : (long long)frames;
  a.out_len = out_len_dev ? reinterpret_cast<long long*>(out_len_dev) : reinterpret_cast<long long*>(ws + o_len);
  a.pa = reinterpret_cast<int*>(ws + o_pa); a.pb = reinterpret_cast<int*>(ws + o_pb); a.pre_ld = (long long)frames + 1;
  a.lens = reinterpret_cast<const long long*>(ws + o_lens);
  a.n = n; a.hop = hop; a.w = cfg->smooth_frames; a.s = cfg->max_silence_frames + 1;
  a.tiles = (int)((frames + cnk::kTrimGatherFrames - 1) / cnk::kTrimGatherFrames);
  cnk::launch_trim_plan(a, st);
  HIP_CHECK(hipGetLastError());
  if (out_dev) {
    cnk::launch_trim_gather(a, st);
    HIP_CHECK(hipGetLastError());
  }
}

}  // namespace trim
