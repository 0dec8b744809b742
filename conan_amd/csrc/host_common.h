// Host-side runtime of libconan_hip.so: context (weights), streams (per-slot state), launch plans.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/conan_hip.h"
#include "kernels.h"

namespace ch {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

void hip_check(hipError_t e, const char* what);

struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
  int64_t numel() const { int64_t n = 1; for (auto s : shape) n *= s; return n; }
};

// A conv / linear weight repacked for conv_mfma: [Cout_pad/64][taps][Cin_alloc/4][64][4], zero padded: per group of
// 64 output columns the K rows are 1 KiB apart whatever Cout is (a [K][Cout_pad] layout makes a W tile touch one
// page per row when Cout is large).
struct PackedConv {
  float* w = nullptr;
  float* bias = nullptr;   // [Cout_pad] (zeros when the layer has no bias)
  int Cin = 0, Cin_pad = 0, Cin_alloc = 0, Cout = 0, Cout_pad = 0, k = 1;
  int shuffle_r = 1;
  float* wl = nullptr;     // bf16 limbs for conv_limb.hip (vocoder upsamplers / wide ResBlock convs; bits behind a float pointer)
  float* wf = nullptr;     // fragment-major copy for rowconv.hip (decoder-step layers only), Cout padded to wf_cout_pad
  int wf_cout_pad = 0;
};

struct Ring {
  float* base = nullptr;
  int L = 0, C = 0, rate = 1;
  int hist = 0;             // rows before the step's first that a step may still read (slot snapshots save these)
  long long slot_stride = 0;
  cnk::TRef ref(int off = 0) const {
    cnk::TRef r; r.base = base; r.slot_stride = slot_stride; r.C = C; r.lmask = L - 1; r.rate = rate; r.off = off; r.mode = 0; r.pad_ = 0;
    return r;
  }
  long long floats_per_slot() const { return slot_stride; }
};

struct Lin {   // batch-indexed linear buffer [n][rows][C]
  float* base = nullptr;
  int rows = 0, C = 0;
  cnk::TRef ref(int off = 0) const {
    cnk::TRef r; r.base = base; r.slot_stride = (long long)rows * C; r.C = C; r.lmask = 0; r.rate = 0; r.off = off; r.mode = 1; r.pad_ = 0;
    return r;
  }
};

inline cnk::TRef lin_ref(float* p, int rows, int C, int off = 0) {
  Lin l; l.base = p; l.rows = rows; l.C = C; return l.ref(off);
}
inline cnk::TRef null_ref() { cnk::TRef r; memset(&r, 0, sizeof(r)); r.mode = 1; return r; }

inline int next_pow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

}  // namespace ch

int conan_mel_frames(const conan_mel_cfg& m, int samples);   // frontend.hip: frames conan_wav2mel writes per waveform

// Stream-sets that exist right now on a device (conan_streams_create .. _destroy), over ALL contexts of this process: launches that
// wait inside themselves (Emformer clusters on whole CUs, the decoder's resident groups, the f32 pair kernel) can only be given
// the whole chip when nothing else of the process can overlap them on that device - two contexts on one GPU each counted
// themselves "alone" while the count was per context.  Other PROCESSES on the device are not visible here:
// CONAN_STREAMS_SHARED_DEVICE says so.
inline std::atomic<int>& device_live_streams(int device) {
  static std::atomic<int> counts[64];
  return counts[device & 63];
}

namespace ch {
// One resampler configuration (resample.hip): the device tables and host copies of what the host plans with.
struct RsTable {
  cnk::RsFilter f;
  std::vector<int> ph;                // [nph][2] klo, cnt
  int win = 0;                        // LDS floats of a tile's input window (upper bound)
  int in_rate = 0, out_rate = 0;
  long long first(long long j) const { const long long q = j / f.nph; const int p = (int)(j - q * f.nph); return q * f.orig - f.w + ph[2 * p]; }
  long long last(long long j) const { const long long q = j / f.nph; const int p = (int)(j - q * f.nph); return q * f.orig - f.w + ph[2 * p] + ph[2 * p + 1] - 1; }
  long long length(long long samples) const { return (long long)(((__int128)f.nph * samples + f.orig - 1) / f.orig); }
  // the longest prefix of outputs whose last tap is below `in` (and, like the whole signal, below length(in))
  long long ready(long long in) const {
    long long best = length(in);
    for (int p = 0; p < f.nph; ++p) {
      const long long c = (long long)ph[2 * p] + ph[2 * p + 1] - 1 - f.w;      // last(p + nph * q) = q * orig + c
      const long long q = in - c <= 0 ? 0 : (in - c + f.orig - 1) / f.orig;
      best = std::min(best, p + (long long)f.nph * q);
    }
    return best;
  }
};
// One drift-resampler configuration (resample.hip): the f32 table of the law, [kDrPhases + 1][2W] on the host, and its device form.
struct DrTable {
  std::vector<float> host;
  const float2* dev = nullptr;        // (T, D) at k * kDrPhases + p
  int W = 0, in_rate = 0, out_rate = 0;
};
// A stream slot's place in the drift law: since the last change of ppb, output j >= out0 sits at (n0 << 32) + f0 + (j - out0) * step.
// Output 0 sits at position 0; a change takes effect at the next output, one new step past the last one produced.
struct DriftPos {
  typedef unsigned __int128 u128;
  const DrTable* d = nullptr;         // null: the slot has no drift
  int ppb = 0, win = 0;               // win: LDS floats of a tile's window at the side's largest step
  unsigned long long step = 0;
  long long out0 = 0, n0 = 0; unsigned f0 = 0;
  u128 pos(long long j) const { return (((u128)n0 << 32) | f0) + (u128)(j - out0) * step; }
  // the first output j >= out0 whose input index n_j is at or past `limit`
  long long first_at(long long limit) const {
    const u128 base = pos(out0), end = limit > 0 ? (u128)limit << 32 : 0;
    return end <= base ? out0 : out0 + (long long)((end - base + step - 1) / step);
  }
  // ppb changes in front of output `next` (the slot's next one)
  void retime(int new_ppb, unsigned long long new_step, long long next) {
    if (next > 0) { const u128 p = pos(next - 1) + new_step; n0 = (long long)(p >> 32); f0 = (unsigned)p; out0 = next; }
    ppb = new_ppb; step = new_step;
  }
  void restart() { out0 = 0; n0 = 0; f0 = 0; }
};
// Pinned staging of a whole-signal call's host table (loudness.hip): a buffer is reused only after the copy that read it has
// completed (the wait is on the host, for a copy four calls old).
struct TableStage {
  static constexpr int N = 4;
  void* buf[N] = {}; size_t cap[N] = {}; hipEvent_t ev[N] = {}; int next = 0;
  void* take(size_t bytes) {
    const int q = next;
    if (!ev[q]) HIP_CHECK(hipEventCreateWithFlags(&ev[q], hipEventDisableTiming));
    HIP_CHECK(hipEventSynchronize(ev[q]));
    if (bytes > cap[q]) {
      if (buf[q]) HIP_CHECK(hipHostFree(buf[q]));
      buf[q] = nullptr; cap[q] = 0;
      HIP_CHECK(hipHostMalloc(&buf[q], bytes, hipHostMallocDefault));
      cap[q] = bytes;
    }
    return buf[q];
  }
  void sent(hipStream_t st) { HIP_CHECK(hipEventRecord(ev[next], st)); next = (next + 1) % N; }
  ~TableStage() {
    for (int q = 0; q < N; ++q) { if (ev[q]) (void)hipEventDestroy(ev[q]); if (buf[q]) (void)hipHostFree(buf[q]); }
  }
};
}  // namespace ch

struct conan_ctx {
  int device = 0;
  conan_cfg cfg;
  bool finalized = false;
  std::map<std::string, ch::HostTensor> raw;
  std::map<std::string, ch::PackedConv> convs;
  std::map<std::string, float*> vecs;
  std::map<std::string, float> scalars;
  std::vector<void*> allocs;
  int64_t weight_bytes = 0;
  int hop = 1;
  int num_cu = 256;
  bool has_limb_weights = false;   // finalize packed bf16-limb copies of the vocoder's conv weights (resblock_limb.hip / conv_limb.hip)

  float* dev_alloc(size_t floats, bool zero = true);
  float* upload(const std::vector<float>& v);
  const ch::HostTensor& get(const std::string& key) const;
  bool has(const std::string& key) const { return raw.count(key) != 0; }
  const ch::PackedConv& conv(const std::string& name) const;
  float* vec(const std::string& name) const;
  float* vec_or_null(const std::string& name) const;
  void pack_conv(const std::string& name, const std::vector<float>& W, const float* bias, int Cout, int Cin, int k,
                 int shuffle_r = 1);
  void add_rowconv_weights(const std::string& name, const std::vector<float>& W);   // second, fragment-major copy
  void pack_from_keys(const std::string& name, const std::string& wkey, const std::string& bkey, int shuffle_r = 1);
  void pack_weightnorm(const std::string& name, const std::string& prefix, int shuffle_r = 1, bool rowconv = false);
  void pack_fragments(const std::string& name, const std::string& prefix);   // resblock_fused.hip operand layout
  void fold_weightnorm(const std::string& prefix, std::vector<float>& W, std::vector<float>& bias, int& Cout, int& Cin, int& k) const;
  void upload_vec(const std::string& name, const std::string& key);
  void finalize_hifigan();
  void finalize_conan();
  void finalize_emformer();
  // mel front-end (frontend.hip): tables are built on first use per configuration; one workspace, shared with conan_loud_norm,
  // regrown when a call needs more (the previous block is released once `st` has drained)
  float* fe_ws = nullptr; size_t fe_ws_floats = 0;
  float* workspace(size_t floats, hipStream_t st);
  void wav2mel(const conan_mel_cfg& m, const float* wav, int n, int samples, float* mel_out, hipStream_t st);
  std::string mel_tables(const conan_mel_cfg& m);          // window / twiddle / filterbank tables (vecs key prefix)
  // resampler (resample.hip): taps built on first use per configuration (CONAN_ERR_INVALID for a configuration it refuses)
  std::map<std::string, ch::RsTable> rs_tabs;
  const ch::RsTable& resample_table(const conan_resample_cfg& c);
  std::map<std::string, ch::DrTable> dr_tabs;              // drift resampler: table built on first use per configuration
  const ch::DrTable& drift_table(const conan_resample_cfg& c);
  ch::TableStage loud_stage;                               // conan_loud_norm's per-call table (loudness.hip)
  ~conan_ctx();
};

// conan_resample's body (resample.hip)
void conan_ctx_resample(conan_ctx* ctx, const conan_resample_cfg& c, const float* x, int n, int64_t samples, float* y, int64_t* out_samples, hipStream_t st);
// conan_resample_drift's and conan_resample_drift_table's bodies (resample.hip)
void conan_ctx_resample_drift(conan_ctx* ctx, const conan_resample_cfg& c, int side, const float* x, int n, int64_t samples, const int64_t* at,
                              const int32_t* ppb, int n_seg, float* y, int64_t y_ld, int64_t* out_samples, hipStream_t st);
int64_t conan_ctx_resample_drift_table(const conan_resample_cfg& c, int32_t* W_out, float* table, int64_t cap);
namespace drift {
unsigned long long step(const conan_resample_cfg& c, int side, int ppb);      // the law's step; CONAN_ERR_INVALID for a side or ppb it refuses
int tile_window(const conan_resample_cfg& c, int side);                       // LDS floats of a tile at the side's largest step
}  // namespace drift
// the K-weighting biquads at rate fs and the transition matrix M[16] of kLdSeg zero inputs (loudness.hip; shared with level.hip)
void conan_k_weighting(double fs, cnk::LdBiquad& shelf, cnk::LdBiquad& hp, double* M);
// conan_level's body, and the leveller's host arithmetic that wavio.hip shares (level.hip)
void conan_ctx_level(conan_ctx* ctx, const conan_level_cfg& c, const float* x, int64_t x_ld, int n, const int64_t* samples, float* y, int64_t y_ld,
                     double* trace, int64_t trace_ld, hipStream_t st);
namespace level {
void check_cfg(const conan_level_cfg& c, const char* who);
cnk::LvCfg kernel_cfg(const conan_level_cfg& c);
cnk::LvFilter filter(const conan_ctx* ctx, const char* who);
cnk::LvCall plan_call(long long pos0, int m, int U, double fs);
}  // namespace level
// conan_loud_norm's body (loudness.hip)
void conan_ctx_loud_norm(conan_ctx* ctx, const conan_loudness_cfg& c, const float* x, int64_t x_ld, int n, const int64_t* samples, float* y,
                         int64_t y_ld, double* stats, hipStream_t st);
