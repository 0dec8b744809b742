// Register matching for pitch following (include/conan_hip.h, conan_register_cfg): the kernel that rewrites a tracked contour with the
// causal log-f0 mean transform, the whole-signal entry point conan_f0_register and the host side of conan_streams_set_pitch_register.
// The wav-in steps launch the kernel behind the tracker's launch on the rows of the call's contour staging (reg::wav_enqueue below), so the decoder
// step reads matched values through PitchHeadArgs::trk_f0 / trk_uv.
#include <climits>
#include <cmath>

#include "streams.h"

namespace cnk {

constexpr int kRegWaves = kRegThreads / 64;
constexpr double kRegUnit = 4194304.0;      // 2^22: quantised log2-f0 units per octave

// One row per workgroup; the row's frames in tiles of kRegThreads, a lane per frame.  The state after frame j is the row's start plus
// the inclusive sums of (counted, q) over frames 0 .. j: a wave64 shuffle scan, the waves' totals through LDS, the tiles' totals in a
// register carry.  The sums are int64: exact, so neither the tile width nor the cut of a stream into rows shows in a result.
__global__ __launch_bounds__(kRegThreads) void f0_register_kernel(const RegArgs a) {
  __shared__ long long start_s[2];
  __shared__ long long wave_s[kRegWaves][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if ((int)blockIdx.x >= a.rows) return;
  const RegRow r = a.tab[blockIdx.x];      // uniform in the workgroup
  if (tid == 0) {
    long long n0 = r.seed_n, S0 = r.seed_S;
    if (!r.reseed && r.slot >= 0) { n0 = a.state[2 * (long long)r.slot]; S0 = a.state[2 * (long long)r.slot + 1]; }
    start_s[0] = n0; start_s[1] = S0;
  }
  __syncthreads();
  long long cn = start_s[0], cS = start_s[1];      // the carry: the state before the tile
  const double target = (double)r.target, lim = (double)r.max_shift;
  const float* f0 = a.f0 + r.in_off;
  const float* uv = a.uv + r.in_off;
  for (int base = 0; base < r.nframes; base += kRegThreads) {
    // the lane's frame: loads are unconditional at a clamped address, the tail is selected after them
    const int j = base + tid, jc = j < r.nframes ? j : r.nframes - 1;
    const float v = f0[jc], u = uv[jc];
    const bool in = j < r.nframes;
    const bool counted = in && u == 0.f && isfinite(v) && fabsf(v) <= 64.f;
    long long k = counted ? 1 : 0;
    long long q = counted ? llrint((double)v * kRegUnit) : 0;
    for (int d = 1; d < 64; d <<= 1) {
      const long long k2 = __shfl_up(k, d), q2 = __shfl_up(q, d);
      if (lane >= d) { k += k2; q += q2; }
    }
    if (lane == 63) { wave_s[wave][0] = k; wave_s[wave][1] = q; }
    __syncthreads();
    long long tk = 0, tq = 0;
    for (int w = 0; w < kRegWaves; ++w) {
      const long long wk = wave_s[w][0], wq = wave_s[w][1];
      if (w < wave) { k += wk; q += wq; }
      tk += wk; tq += wq;
    }
    __syncthreads();      // (the next tile writes wave_s again)
    if (in && r.out_off >= 0) {
      float y = v;
      if (counted) {
        const long long n = cn + k, S = cS + q;
        const double mu = (double)S / ((double)n * kRegUnit);
        double d = target - mu;
        d = fmin(fmax(d, -lim), lim);
        y = (float)((double)v + d);
      }
      a.out[r.out_off + j] = y;
    }
    cn += tk; cS += tq;
  }
  if (tid == 0) {
    if (r.slot >= 0) { a.state[2 * (long long)r.slot] = cn; a.state[2 * (long long)r.slot + 1] = cS; }
    if (r.state_row >= 0) { a.state_out[2 * (long long)r.state_row] = cn; a.state_out[2 * (long long)r.state_row + 1] = cS; }
  }
}

void launch_f0_register(const RegArgs& a, hipStream_t st) {
  if (a.rows < 1) return;
  hipLaunchKernelGGL(f0_register_kernel, dim3(a.rows), dim3(kRegThreads), 0, st, a);
}

}  // namespace cnk

namespace reg {

constexpr long long kMaxSeedCount = 1ll << 34, kMaxQ = 1ll << 28;

void check_cfg(const conan_register_cfg& c, const char* who) {
  const std::string w = std::string(who) + ": ";
  if (c.enabled != 0 && c.enabled != 1) throw Error(CONAN_ERR_INVALID, w + "conan_register_cfg.enabled must be 0 or 1");
  if (!c.enabled) return;      // (the other fields are ignored)
  if (c.reseed != 0 && c.reseed != 1) throw Error(CONAN_ERR_INVALID, w + "conan_register_cfg.reseed must be 0 or 1");
  if (!std::isfinite(c.target)) throw Error(CONAN_ERR_INVALID, w + "target must be finite");
  if (!std::isfinite(c.max_shift) || !(c.max_shift >= 0.f)) throw Error(CONAN_ERR_INVALID, w + "max_shift must be finite and >= 0");
  if (c.seed_count < 0 || c.seed_count > kMaxSeedCount) throw Error(CONAN_ERR_INVALID, w + "seed_count must be in 0 .. 2^34");
  const long long bound = c.seed_count * kMaxQ;      // (<= 2^62)
  if (c.seed_sum > bound || c.seed_sum < -bound) throw Error(CONAN_ERR_INVALID, w + "|seed_sum| must not exceed seed_count * 2^28");
}

cnk::RegRow row(const conan_register_cfg& c) {
  cnk::RegRow r;
  memset(&r, 0, sizeof(r));
  r.seed_n = c.seed_count; r.seed_S = c.seed_sum; r.target = c.target; r.max_shift = c.max_shift;
  r.reseed = 1; r.slot = -1; r.state_row = -1; r.out_off = -1;
  return r;
}

void whole(conan_ctx* ctx, const conan_register_cfg* cfg, const float* f0_dev, const float* uv_dev, int n, const int32_t* frames, int64_t ld,
           float* f0_out_dev, int64_t* state_out_dev, void* stream) {
  if (!ctx || !cfg || !f0_dev || !uv_dev || !frames) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_f0_register");
  if (!cfg->enabled) throw Error(CONAN_ERR_INVALID, "conan_f0_register: cfg.enabled must be 1");
  if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, "conan_f0_register: n must be in 1 .. 65535");
  if (ld < 0 || ld > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_f0_register: ld out of range");
  for (int i = 0; i < n; ++i)
    if (frames[i] < 0 || frames[i] > ld) throw Error(CONAN_ERR_INVALID, "conan_f0_register: row " + std::to_string(i) + ": frames must be in 0 .. ld");
  HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t table = (size_t)n * sizeof(cnk::RegRow);
  cnk::RegRow* h = static_cast<cnk::RegRow*>(ctx->loud_stage.take(table));
  const cnk::RegRow proto = row(*cfg);
  for (int i = 0; i < n; ++i) {
    h[i] = proto;
    h[i].in_off = (long long)i * ld; h[i].out_off = f0_out_dev ? (long long)i * ld : -1;
    h[i].nframes = frames[i]; h[i].state_row = state_out_dev ? i : -1;
  }
  char* ws = reinterpret_cast<char*>(ctx->workspace(table / sizeof(float), st));
  HIP_CHECK(hipMemcpyAsync(ws, h, table, hipMemcpyHostToDevice, st));
  ctx->loud_stage.sent(st);
  cnk::RegArgs a;
  memset(&a, 0, sizeof(a));
  a.f0 = f0_dev; a.uv = uv_dev; a.out = f0_out_dev; a.state = nullptr; a.state_out = reinterpret_cast<long long*>(state_out_dev);
  a.tab = reinterpret_cast<const cnk::RegRow*>(ws); a.rows = n;
  cnk::launch_f0_register(a, st);
  HIP_CHECK(hipGetLastError());
}

void set_register(conan_streams* s, const int32_t* slots, int n, const conan_register_cfg* cfg, void* stream) {
  if (!s || !slots || !cfg) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_streams_set_pitch_register");      // (before the handle is touched, before any GPU use)
  if (!wavio::begin_setter(s, slots, n, cfg->enabled != 0, s->reg.allocated(), "conan_streams_set_pitch_register", stream)) return;
  s->register_init();
  s->reg.store_restarting(slots, n, *cfg);      // the restart travels in the slot's next register row
}

// rows without frames: a pending slot's row starts from the seed and names no slot, any other reads its state (and writes it back as it is)
void state(conan_streams* s, const int32_t* slots, int n, int64_t* state_dev, void* stream) {
  if (!s || !slots || !state_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  wavio::check_slot_list(s, slots, n);
  const std::vector<cnk::RegRow> rows = s->reg.state_rows<cnk::RegRow>(slots, n, row, "conan_streams_pitch_register_state", " has no register matching (conan_streams_set_pitch_register)");
  hipStream_t st = s->enter(stream);
  const int q = s->reg.sets.begin(rows.data(), n, st);
  cnk::RegArgs a;
  memset(&a, 0, sizeof(a));
  a.state = s->reg.state; a.state_out = reinterpret_cast<long long*>(state_dev); a.tab = s->reg.sets.rows[q]; a.rows = n;
  cnk::launch_f0_register(a, st);
  HIP_CHECK(hipGetLastError());
  s->reg.sets.end(q, st);
}

cnk::RegRow wav_row(const conan_streams* s, int slot, long long off, int nframes) {
  cnk::RegRow r = row(s->reg.cfg[slot]);
  r.in_off = off; r.out_off = off; r.nframes = nframes; r.slot = slot; r.reseed = s->reg.pending[slot];
  return r;
}

// directly behind the tracker: the decoder stage reads the matched rows
void wav_enqueue(conan_streams* s, const std::vector<cnk::RegRow>& rows, int contour_set, hipStream_t cst, FrontWork& front) {
  if (rows.empty()) return;
  const int q = s->reg.sets.begin(rows.data(), (int)rows.size(), cst);
  cnk::RegArgs a;
  memset(&a, 0, sizeof(a));
  a.f0 = s->follow.ct_f0[contour_set]; a.uv = s->follow.ct_uv[contour_set]; a.out = s->follow.ct_f0[contour_set]; a.state = s->reg.state;
  a.tab = s->reg.sets.rows[q]; a.rows = (int)rows.size();
  front.at[kFrRegister] = [s, a, q](hipStream_t st) {
    s->profiled("f0_register_kernel", 0.0, st, [&] { cnk::launch_f0_register(a, st); });
    s->reg.sets.end(q, st);
  };
}

void wav_commit(conan_streams* s, const std::vector<cnk::RegRow>& rows) {
  for (const cnk::RegRow& r : rows) s->reg.pending[r.slot] = 0;      // (the rows carried the restarts)
}

}  // namespace reg

void conan_streams::register_init() {
  if (reg.state) return;
  reg.state = reinterpret_cast<long long*>(alloc((size_t)max_slots * 4));      // 16 bytes per slot, zeroed (counted by state_bytes)
  reg.sets.init(max_slots, allocs);
  state_bytes += (int64_t)kStageSets * max_slots * sizeof(cnk::RegRow);
  reg.assign(max_slots);
}
