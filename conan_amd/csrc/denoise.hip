// Input noise suppression (include/conan_hip.h, conan_denoise_cfg): the spectral gate's kernels, the whole-signal entry point
// conan_mel_denoise and the host side of conan_streams_set_denoise / conan_streams_denoise / conan_streams_denoise_state.  The wav-in
// steps launch the stream kernel directly behind the mel front-end's launch, on the frames it has just written into the slots' mel
// rings (denoise::WavStage below); nothing else of a step changes.
#include <climits>
#include <cmath>

#include "streams.h"

namespace cnk {

// what lane b carries across a row's frames; fresh: no frame since the restart, the next one applies Start
struct DnLane { int N, A; long long frames; int fresh; };

constexpr int kDnMaxLevel = 1 << 20;      // |L|, |N| and A of the law never pass it

// The record may be the one dn_store rewrites at the end of the same kernel (the stream kernel's state[slot]; the signal kernel's,
// when a caller's seed is its state_out).  The barrier holds every lane's stores behind every lane's loads, so the branch on `bins`
// is uniform in the workgroup whatever the waves' skew; it is unconditional, and so covers a row of no frames and smooth = 0, where
// dn_frames has no barrier.  floor and att are read clamped to the law's range, which a record written here already keeps: the
// int32 arithmetic of dn_frames then cannot overflow whatever words a caller's seed holds.
__device__ __forceinline__ DnLane dn_load(const DnState* st, int nm, int bc) {
  DnLane s;
  s.N = 0; s.A = 0; s.frames = 0; s.fresh = 1;
  if (st && st->bins == nm) {
    const int N = st->floor[bc], A = st->att[bc];
    s.N = N < -kDnMaxLevel ? -kDnMaxLevel : (N > kDnMaxLevel ? kDnMaxLevel : N);
    s.A = A < 0 ? 0 : (A > kDnMaxLevel ? kDnMaxLevel : A);
    s.frames = st->frames; s.fresh = 0;
  }
  __syncthreads();
  return s;
}

// every entry of the record is written: the bins' words by their lanes, zeros behind them
__device__ __forceinline__ void dn_store(DnState* st, const DnLane& s, int nm) {
  const int b = threadIdx.x;
  for (int i = b; i < kDnMaxBins; i += blockDim.x) {
    const bool own = i == b && b < nm && !s.fresh;
    st->floor[i] = own ? s.N : 0;
    st->att[i] = own ? s.A : 0;
  }
  if (b == 0) { st->frames = s.fresh ? 0 : s.frames; st->bins = s.fresh ? 0 : nm; st->reserved = 0; }
}

// The law on `count` frames of one row: frame k at ((first + k) & mask) * nm floats of x, written to the same place of y (y may be
// x: an untouched bin is then not stored).  Lane b owns bin min(b, nm - 1): a lane past the row's bins repeats the last bin's
// arithmetic at the last bin's address and stores nothing, so every load is unconditional and the workgroup's barriers are uniform.
// The neighbours' `a` go through the LDS row frame k & 1: one barrier per frame, because the row a frame writes was last read two
// frames earlier, in front of the barrier between.  The next frame's value is loaded before this frame's arithmetic.
__device__ __forceinline__ void dn_frames(const DnRow& r, int nm, const float* x, float* y, int first, int mask, int count, DnLane& s,
                                          int (*nb)[kDnMaxBins]) {
  const int b = threadIdx.x, bc = b < nm ? b : nm - 1;
  const bool own = b < nm, inplace = x == y;
  const int lo = bc > 0 ? bc - 1 : 0, hi = bc < nm - 1 ? bc + 1 : nm - 1;
  const int fall_add = (1 << r.fall_shift) - 1;
  if (count < 1) return;
  unsigned next = __float_as_uint(x[(long long)(first & mask) * nm + bc]);
  for (int k = 0; k < count; ++k) {
    const long long at = (long long)((first + k) & mask) * nm + bc;
    const unsigned bits = next;
    const int kn = k + 1 < count ? k + 1 : k;      // (clamped: the last frame is loaded again)
    next = __float_as_uint(x[(long long)((first + kn) & mask) * nm + bc]);
    const float v = __uint_as_float(bits);
    const double dv = v != v ? -1024.0 : (double)v;      // fmax(NaN, -1024) = -1024
    const int L = (int)rint(fmin(fmax(dv, -1024.0), 1024.0) * 1024.0);
    if (s.fresh) { s.N = L > r.floor_min ? L : r.floor_min; s.A = 0; s.frames = 0; s.fresh = 0; }
    const int snr = L - (s.N + r.bias);
    const int d = r.knee - snr > 0 ? r.knee - snr : 0;
    const long long prod = ((long long)d * r.slope) >> 8;
    int a = prod < r.depth ? (int)prod : r.depth;
    if (r.smooth) {
      nb[k & 1][b] = a;
      __syncthreads();
      a = (nb[k & 1][lo] + 2 * a + nb[k & 1][hi] + 2) >> 2;
    }
    const int up = s.A + r.close_step < a ? s.A + r.close_step : a, down = s.A - r.open_step > a ? s.A - r.open_step : a;
    s.A = a > s.A ? up : down;
    if (s.A != 0) {
      const float o = fmaxf((float)((double)(L - s.A) * 0.0009765625), r.out_floor);
      if (own) y[at] = o;
    } else if (own && !inplace) {
      y[at] = v;
    }
    int Nn = L < s.N ? s.N - ((s.N - L + fall_add) >> r.fall_shift) : (L < s.N + r.rise ? L : s.N + r.rise);
    s.N = Nn > r.floor_min ? Nn : r.floor_min;
    s.frames = (long long)((unsigned long long)s.frames + 1);      // (a seed's count may be any word)
  }
}

__global__ __launch_bounds__(kDnMaxBins) void denoise_signal_kernel(const DnSignalArgs a) {
  __shared__ int nb[2][kDnMaxBins];
  if ((int)blockIdx.x >= a.rows) return;
  const DnRow r = a.tab[blockIdx.x];      // uniform in the workgroup
  const int nm = a.nm, b = threadIdx.x, bc = b < nm ? b : nm - 1;
  DnLane s = dn_load(a.seed && !r.reseed ? a.seed + r.row : nullptr, nm, bc);
  dn_frames(r, nm, a.x + (long long)r.row * a.ld, a.y + (long long)r.row * a.ld, 0, INT_MAX, r.nnew, s, nb);
  if (r.state_row >= 0) dn_store(a.state_out + r.state_row, s, nm);
}

__global__ __launch_bounds__(kDnMaxBins) void denoise_stream_kernel(const DnStreamArgs a) {
  __shared__ int nb[2][kDnMaxBins];
  if ((int)blockIdx.x >= a.rows) return;
  const DnRow r = a.tab[blockIdx.x];      // uniform in the workgroup
  const int nm = a.nm, b = threadIdx.x, bc = b < nm ? b : nm - 1;
  float* ring = a.mring + (long long)r.slot * a.LM * nm;
  DnLane s = dn_load(r.reseed ? nullptr : a.state + r.slot, nm, bc);
  dn_frames(r, nm, ring, ring, r.f0, a.LM - 1, r.nnew, s, nb);
  dn_store(a.state + r.slot, s, nm);
  // the chunk the step consumes, from the ring: a lane reads back only what it wrote itself (its own bin), so no barrier
  if (b < nm) {
    float* ch = a.chunk + (long long)r.chunk * r.rows * nm;
    for (int q = 0; q < r.rows; ++q) {
      const int src = r.pos + (q < r.real - 1 ? q : r.real - 1);
      ch[(long long)q * nm + b] = ring[(long long)(src & (a.LM - 1)) * nm + b];
    }
  }
}

static unsigned dn_block(int nm) { return 64u * (unsigned)((nm + 63) / 64); }

void launch_denoise_signal(const DnSignalArgs& a, hipStream_t st) {
  if (a.rows < 1) return;
  hipLaunchKernelGGL(denoise_signal_kernel, dim3(a.rows), dim3(dn_block(a.nm)), 0, st, a);
}

void launch_denoise_stream(const DnStreamArgs& a, hipStream_t st) {
  if (a.rows < 1) return;
  hipLaunchKernelGGL(denoise_stream_kernel, dim3(a.rows), dim3(dn_block(a.nm)), 0, st, a);
}

}  // namespace cnk

namespace denoise {

static_assert(sizeof(conan_denoise_cfg) == 64, "sixteen 32-bit fields");
static_assert(sizeof(conan_denoise_state) == sizeof(cnk::DnState), "the kernels' state is the header's");
constexpr int kMax = 1 << 20;

void check_cfg(const conan_denoise_cfg& c, const char* who) {
  const std::string w = std::string(who) + ": ";
  auto bad = [&](const char* what) { throw Error(CONAN_ERR_INVALID, w + what); };
  if (c.enabled != 0 && c.enabled != 1) bad("conan_denoise_cfg.enabled must be 0 or 1");
  if (!c.enabled) return;      // (the other fields are ignored)
  if (c.reseed != 0 && c.reseed != 1) bad("reseed must be 0 or 1");
  if (c.bias < 0 || c.bias > kMax || c.knee < 0 || c.knee > kMax) bad("bias and knee must be in 0 .. 2^20");
  if (c.slope < 0 || c.slope > 65536) bad("slope must be in 0 .. 2^16");
  if (c.depth < 1 || c.depth > kMax) bad("depth must be in 1 .. 2^20");
  if (c.close_step < 1 || c.close_step > kMax || c.open_step < 1 || c.open_step > kMax) bad("close_step and open_step must be in 1 .. 2^20");
  if (c.rise < 0 || c.rise > kMax) bad("rise must be in 0 .. 2^20");
  if (c.fall_shift < 0 || c.fall_shift > 8) bad("fall_shift must be in 0 .. 8");
  if (c.floor_min < -kMax || c.floor_min > kMax) bad("floor_min must be in -2^20 .. 2^20");
  if (c.smooth != 0 && c.smooth != 1) bad("smooth must be 0 or 1");
  if (!std::isfinite(c.out_floor)) bad("out_floor must be finite");
  if (c.reserved[0] != 0 || c.reserved[1] != 0 || c.reserved[2] != 0) bad("the reserved words must be 0");
}

cnk::DnRow row(const conan_denoise_cfg& c) {
  cnk::DnRow r;
  memset(&r, 0, sizeof(r));
  r.bias = c.bias; r.knee = c.knee; r.slope = c.slope; r.depth = c.depth; r.close_step = c.close_step; r.open_step = c.open_step;
  r.rise = c.rise; r.fall_shift = c.fall_shift; r.floor_min = c.floor_min; r.smooth = c.smooth; r.out_floor = c.out_floor;
  r.slot = -1; r.state_row = -1; r.reseed = 1;
  return r;
}

void whole(conan_ctx* ctx, const conan_denoise_cfg* cfg, const float* mel_dev, int n, const int32_t* frames, int64_t ld, int num_mels,
           const conan_denoise_state* seed_dev, float* out_dev, conan_denoise_state* state_out_dev, void* stream) {
  if (!ctx || !cfg || !mel_dev || !frames || !out_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_mel_denoise");
  if (!cfg->enabled) throw Error(CONAN_ERR_INVALID, "conan_mel_denoise: cfg.enabled must be 1");
  if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, "conan_mel_denoise: n must be in 1 .. 65535");
  if (num_mels < 1 || num_mels > cnk::kDnMaxBins) throw Error(CONAN_ERR_INVALID, "conan_mel_denoise: num_mels must be in 1 .. 256");
  if (ld < 0 || ld > ((int64_t)1 << 40)) throw Error(CONAN_ERR_INVALID, "conan_mel_denoise: ld must be in 0 .. 2^40");
  if (((uintptr_t)seed_dev | (uintptr_t)state_out_dev) & 7) throw Error(CONAN_ERR_INVALID, "conan_mel_denoise: seed_dev and state_out_dev must be 8-byte aligned");
  for (int i = 0; i < n; ++i)
    if (frames[i] < 0 || (int64_t)frames[i] * num_mels > ld)
      throw Error(CONAN_ERR_INVALID, "conan_mel_denoise: row " + std::to_string(i) + ": frames must be >= 0 and frames * num_mels floats must fit the row stride ld");
  HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t table = (size_t)n * sizeof(cnk::DnRow);
  cnk::DnRow* h = static_cast<cnk::DnRow*>(ctx->loud_stage.take(table));
  const cnk::DnRow proto = row(*cfg);
  for (int i = 0; i < n; ++i) {
    h[i] = proto;
    h[i].row = i; h[i].nnew = frames[i]; h[i].reseed = seed_dev ? 0 : 1; h[i].state_row = state_out_dev ? i : -1;
  }
  char* ws = reinterpret_cast<char*>(ctx->workspace((table + 3) / sizeof(float), st));
  HIP_CHECK(hipMemcpyAsync(ws, h, table, hipMemcpyHostToDevice, st));
  ctx->loud_stage.sent(st);
  cnk::DnSignalArgs a;
  memset(&a, 0, sizeof(a));
  a.x = mel_dev; a.y = out_dev; a.ld = ld; a.seed = reinterpret_cast<const cnk::DnState*>(seed_dev);
  a.state_out = reinterpret_cast<cnk::DnState*>(state_out_dev); a.tab = reinterpret_cast<const cnk::DnRow*>(ws); a.rows = n; a.nm = num_mels;
  cnk::launch_denoise_signal(a, st);
  HIP_CHECK(hipGetLastError());
}

void set_denoise(conan_streams* s, const int32_t* slots, int n, const conan_denoise_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream) {
  if (!s || !slots || !cfg) throw Error(CONAN_ERR_INVALID, "null argument");
  check_cfg(*cfg, "conan_streams_set_denoise");      // (before the handle is touched, before any GPU use)
  if (seed_dev) conan_streams::Denoise::check_rows("conan_streams_set_", "denoise", "", seed_dev, seed_ld);
  if (cfg->enabled && s->ctx->cfg.emf_input_dim > cnk::kDnMaxBins) throw Error(CONAN_ERR_UNSUPPORTED, "conan_streams_set_denoise: the front-end has more than 256 mel bins");
  if (!wavio::begin_setter(s, slots, n, cfg->enabled != 0, s->dn.allocated(), "conan_streams_set_denoise", stream)) return;
  s->denoise_init();
  std::vector<char> restarts((size_t)n);
  for (int i = 0; i < n; ++i) restarts[i] = cfg->enabled && (cfg->reseed != 0 || !s->dn.on(slots[i]));
  s->dn.store_restarting(slots, n, *cfg);      // the restart travels in the slot's next row ...
  // ... or the seed row becomes the state, now (a slot whose state the call keeps: its seed row is not read)
  if (seed_dev) s->dn.seed(slots, n, seed_dev, seed_ld, (hipStream_t)stream, [&](int i) { return restarts[i] != 0; });
}

void state(conan_streams* s, const int32_t* slots, int n, void* rows_dev, int64_t ld, void* stream) {
  record_state(s, &conan_streams::dn, "denoise", slots, n, rows_dev, ld, stream, fresh_zeros);
}

// One table row per call row whose slot suppresses and either completes a frame or emits: its new frames in the ring, then its chunk
// rows (chunk row = the row's place in the call's emit groups, as fe_chunk's; the call row itself in a same-position call).
void WavStage::plan(const conan_streams* s, const WavCall& c) {
  if (s->dn.n_on < 1) return;
  std::vector<int> chunk(c.n, 0);
  c.each_chunk_row([&](int, int, int i, int at) { chunk[i] = at; });
  const int rows_per_chunk = c.seg + s->ctx->cfg.emf_right_context;
  for (int i = 0; i < c.n; ++i) {
    const int slot = c.slots[i];
    const FePlan& p = c.pl[i];
    if (!s->dn.on(slot) || (p.nnew < 1 && p.emit < 1)) continue;
    cnk::DnRow r = row(s->dn.cfg[slot]);
    r.slot = slot; r.reseed = s->dn.pending[slot]; r.row = i;
    r.f0 = p.f0; r.nnew = p.nnew; r.pos = p.pos; r.rows = p.emit > 0 ? rows_per_chunk : 0; r.real = p.real; r.chunk = chunk[i];
    rows.push_back(r);
  }
}

void WavStage::enqueue(conan_streams* s, const WavCall&, hipStream_t cst, FrontWork& front, std::vector<conan_streams::OutPlan>&) {
  if (rows.empty()) return;
  const int q = s->dn.sets.begin(rows.data(), (int)rows.size(), cst);
  cnk::DnStreamArgs a;
  memset(&a, 0, sizeof(a));
  a.mring = s->wav_in.fe_mel; a.chunk = s->wav_in.fe_chunk; a.state = s->dn.state;
  a.tab = s->dn.sets.rows[q]; a.rows = (int)rows.size(); a.nm = s->ctx->cfg.emf_input_dim; a.LM = s->wav_in.fe_LM;
  front.at[kFrDenoise] = [s, a, q](hipStream_t st) {
    s->profiled("denoise_stream_kernel", 0.0, st, [&] { cnk::launch_denoise_stream(a, st); });
    s->dn.sets.end(q, st);
  };
}

void WavStage::commit(conan_streams* s, hipStream_t, hipStream_t) {
  for (const cnk::DnRow& r : rows) s->dn.pending[r.slot] = 0;      // (the rows carried the restarts)
}

}  // namespace denoise
