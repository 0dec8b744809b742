// Loudness normalisation of whole signals (conan_loud_norm): the reference's loud_norm branch of librosa_wav2spec
// (utils/audio/__init__.py:58-63: pyloudnorm's BS.1770 meter, a gain to the target, a division by the peak above 1), restated in
// include/conan_hip.h (conan_loudness_cfg).  The kernels' plan is in kernels.h (LoudArgs); the host builds, per row, the gating
// blocks' edges in double exactly as the header orders the operations, and everything a kernel needs travels in one table.
#include <climits>
#include <cmath>

#include "host_common.h"

namespace cnk {

// A workgroup's kLdTile contiguous samples of its row, coalesced, into LDS: segment l at l * kLdStride (zero past the row's end: a
// ragged last segment runs on into zeros, which changes nothing that is kept - its end state feeds no segment, |0| raises no peak,
// and the samples past the row's last edge belong to no bin).
__device__ __forceinline__ void ld_load_tile(float* lds, const float* x, long long base, long long samples) {
  const long long left = samples - base;
  const int cnt = left < (long long)kLdTile ? (int)left : kLdTile;
#pragma unroll 16
  for (int i = threadIdx.x; i < kLdTile; i += kLdLanes) {
    const float v = x[base + min(i, cnt - 1)];
    lds[(i >> 7) * kLdStride + (i & (kLdSeg - 1))] = i < cnt ? v : 0.f;
  }
  __syncthreads();
}
static_assert(kLdSeg == 128, "ld_load_tile splits a tile index with >> 7");

// State pass: lane l of workgroup (tile, row) runs segment tile * kLdLanes + l from a zero state and keeps its end state and max |x|.
__global__ __launch_bounds__(kLdLanes) void loud_state_kernel(const LoudArgs a) {
  __shared__ float lds[kLdLanes * kLdStride];
  const LdRow R = a.rows[blockIdx.y];
  const int seg = blockIdx.x * kLdLanes + threadIdx.x;
  if ((int)blockIdx.x * kLdLanes >= R.nseg) return;          // uniform per workgroup
  ld_load_tile(lds, a.x + (size_t)blockIdx.y * a.x_ld, (long long)blockIdx.x * kLdTile, R.samples);
  const float* w = lds + threadIdx.x * kLdStride;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  float pk = 0.f;
#pragma unroll 4
  for (int t = 0; t < kLdSeg; ++t) {
    const float v = w[t];
    pk = fmaxf(pk, fabsf(v));
    (void)ld_step(a.shelf, a.hp, s, (double)v);
  }
  if (seg < R.nseg) {
    double* e = a.state + (size_t)(R.seg0 + seg) * 4;
    e[0] = s[0]; e[1] = s[1]; e[2] = s[2]; e[3] = s[3];
    a.peak[R.seg0 + seg] = pk;
  }
}

// Scan: one workgroup per row.  kLdLanes segments at a time pass through LDS (coalesced loads and stores); lane 0 walks them in
// order, replacing every end state by the segment's start state.
__global__ __launch_bounds__(kLdLanes) void loud_scan_kernel(const LoudArgs a) {
  __shared__ double sh[kLdLanes * 4];
  const LdRow R = a.rows[blockIdx.x];
  double* st = a.state + (size_t)R.seg0 * 4;
  double c[4] = {0.0, 0.0, 0.0, 0.0};
  for (int s0 = 0; s0 < R.nseg; s0 += kLdLanes) {
    const int cnt = min(kLdLanes, R.nseg - s0);
    for (int i = threadIdx.x; i < cnt * 4; i += kLdLanes) sh[i] = st[(size_t)s0 * 4 + i];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll 4
      for (int j = 0; j < cnt; ++j) {
        const double e0 = sh[4 * j], e1 = sh[4 * j + 1], e2 = sh[4 * j + 2], e3 = sh[4 * j + 3];
        sh[4 * j] = c[0]; sh[4 * j + 1] = c[1]; sh[4 * j + 2] = c[2]; sh[4 * j + 3] = c[3];
        double nx[4];
        const double e[4] = {e0, e1, e2, e3};
#pragma unroll
        for (int r = 0; r < 4; ++r) nx[r] = fma(a.M[4 * r + 3], c[3], fma(a.M[4 * r + 2], c[2], fma(a.M[4 * r + 1], c[1], fma(a.M[4 * r], c[0], e[r]))));
        c[0] = nx[0]; c[1] = nx[1]; c[2] = nx[2]; c[3] = nx[3];
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cnt * 4; i += kLdLanes) st[(size_t)s0 * 4 + i] = sh[i];
    __syncthreads();
  }
}

// Energy pass: every segment again, from its true start state; y^2 is summed per bin - slot k of the segment takes its k-th bin, the
// first being the bin that holds the segment's first sample (the samples at or past the row's last edge fill a slot nobody reads).
__global__ __launch_bounds__(kLdLanes) void loud_energy_kernel(const LoudArgs a) {
  __shared__ float lds[kLdLanes * kLdStride];
  const LdRow R = a.rows[blockIdx.y];
  const int seg = blockIdx.x * kLdLanes + threadIdx.x;
  if ((int)blockIdx.x * kLdLanes >= R.nseg) return;          // uniform per workgroup
  ld_load_tile(lds, a.x + (size_t)blockIdx.y * a.x_ld, (long long)blockIdx.x * kLdTile, R.samples);
  const float* w = lds + threadIdx.x * kLdStride;
  const bool live = seg < R.nseg;
  const int* edge = a.edges + R.edge0;
  const int t0 = (live ? seg : R.nseg - 1) * kLdSeg;
  int lo = 0, hi = R.nedges - 1;                              // the last edge at or below t0 (edge[0] = 0)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (edge[mid] <= t0) lo = mid; else hi = mid - 1;
  }
  int b = lo, k = 0;
  int next = b + 1 < R.nedges ? edge[b + 1] : INT_MAX;
  const double* s0 = a.state + (size_t)(R.seg0 + (live ? seg : R.nseg - 1)) * 4;
  double s[4] = {s0[0], s0[1], s0[2], s0[3]};
  double* part = a.part + (size_t)(R.seg0 + (live ? seg : R.nseg - 1)) * kLdSlots;
  double acc = 0.0;
#pragma unroll 4
  for (int t = 0; t < kLdSeg; ++t) {
    if (t0 + t == next) {                                     // rare: at most kLdSlots - 1 times per segment
      if (live && k < kLdSlots) part[k] = acc;
      ++k; ++b; acc = 0.0;
      next = b + 1 < R.nedges ? edge[b + 1] : INT_MAX;
    }
    const double y = ld_step(a.shelf, a.hp, s, (double)w[t]);
    acc = fma(y, y, acc);
  }
  if (live && k < kLdSlots) part[k] = acc;
}

// Gate: one workgroup per row.  Bin sums over the segments in ascending order, block energies over their bins in ascending order,
// the two gates and the sums behind them by one thread in block order, then the gain and the row's stats.
__global__ __launch_bounds__(256) void loud_gate_kernel(const LoudArgs a) {
  __shared__ float red[256];
  const LdRow R = a.rows[blockIdx.x];
  const int* edge = a.edges + R.edge0;
  const int* blk = a.blocks + (size_t)R.blk0 * 2;
  const double* part = a.part + (size_t)R.seg0 * kLdSlots;
  double* binsum = a.binsum + R.edge0;
  double* z = a.z + R.blk0;
  double* l = a.l + R.blk0;
  float pk = 0.f;
  for (int s = threadIdx.x; s < R.nseg; s += 256) pk = fmaxf(pk, a.peak[R.seg0 + s]);
  red[threadIdx.x] = pk;
  for (int b = threadIdx.x; b + 1 < R.nedges; b += 256) {
    const int s_lo = edge[b] / kLdSeg, s_hi = (edge[b + 1] - 1) / kLdSeg;
    int f = b;                                                // the bin that holds s_lo's first sample
    while (edge[f] > s_lo * kLdSeg) --f;
    double sum = part[(size_t)s_lo * kLdSlots + (b - f)];
    for (int s = s_lo + 1; s <= s_hi; ++s) sum += part[(size_t)s * kLdSlots];
    binsum[b] = sum;
  }
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
  for (int j = threadIdx.x; j < R.nblocks; j += 256) {
    double sum = 0.0;
    for (int b = blk[2 * j]; b < blk[2 * j + 1]; ++b) sum += binsum[b];
    const double zj = sum / a.block_len;
    z[j] = zj;
    l[j] = -0.691 + 10.0 * log10(zj);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sum = 0.0; int cnt = 0;
  for (int j = 0; j < R.nblocks; ++j) if (l[j] >= -70.0) { sum += z[j]; ++cnt; }
  double L = -INFINITY; int kept = 0;
  if (cnt > 0) {
    const double rel = -0.691 + 10.0 * log10(sum / cnt) - 10.0;
    sum = 0.0;
    for (int j = 0; j < R.nblocks; ++j) if (l[j] > rel && l[j] > -70.0) { sum += z[j]; ++kept; }
    if (kept > 0) L = -0.691 + 10.0 * log10(sum / kept);
  }
  const double peak = (double)red[0];
  double g = 1.0, div = 0.0, p = peak;
  if (L != -INFINITY) {                                       // a row without a loudness is copied unchanged
    g = pow(10.0, (a.target - L) / 20.0);
    p = g * peak;
    if (a.peak_limit && p > 1.0) div = p;
  }
  a.gain[2 * blockIdx.x] = g; a.gain[2 * blockIdx.x + 1] = div;
  if (a.stats) {
    double* o = a.stats + (size_t)blockIdx.x * 4;
    o[0] = L; o[1] = div > 0.0 ? g / div : g; o[2] = p; o[3] = (double)kept;
  }
}

// Apply: y = f32(f64(x) * gain), divided by the peak where the limit engaged; one rounding.
__global__ __launch_bounds__(256) void loud_apply_kernel(const LoudArgs a) {
  const long long n = a.rows[blockIdx.y].samples;
  const double g = a.gain[2 * blockIdx.y], div = a.gain[2 * blockIdx.y + 1];
  const float* x = a.x + (size_t)blockIdx.y * a.x_ld;
  float* y = a.y + (size_t)blockIdx.y * a.y_ld;
  const long long stride = (long long)gridDim.x * 256;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += stride) {
    const double v = (double)x[t] * g;
    y[t] = (float)(div > 0.0 ? v / div : v);
  }
}

void launch_loud_measure(const LoudArgs& a, hipStream_t st) {
  const dim3 tiles((unsigned)a.tiles, (unsigned)a.n);
  hipLaunchKernelGGL(loud_state_kernel, tiles, dim3(kLdLanes), 0, st, a);
  hipLaunchKernelGGL(loud_scan_kernel, dim3((unsigned)a.n), dim3(kLdLanes), 0, st, a);
  hipLaunchKernelGGL(loud_energy_kernel, tiles, dim3(kLdLanes), 0, st, a);
  hipLaunchKernelGGL(loud_gate_kernel, dim3((unsigned)a.n), dim3(256), 0, st, a);
}

void launch_loud_apply(const LoudArgs& a, long long longest, hipStream_t st) {
  const long long blocks = (longest + 255) / 256;
  hipLaunchKernelGGL(loud_apply_kernel, dim3((unsigned)std::min(blocks, 4096ll), (unsigned)a.n), dim3(256), 0, st, a);
}

}  // namespace cnk

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr double kTg = 0.4, kStep = 0.25;            // gating block length (s) and its step as a fraction of the block

size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

}  // namespace

// The two K-weighting biquads at rate fs, normalised by a0 (include/conan_hip.h), and M, the transition matrix of one segment.
void conan_k_weighting(double fs, cnk::LdBiquad& shelf, cnk::LdBiquad& hp, double* M) {
  {
    const double G = 4.0, Q = 1.0 / std::sqrt(2.0), fc = 1500.0;
    const double A = std::pow(10.0, G / 40.0), w0 = 2.0 * kPi * (fc / fs), alpha = std::sin(w0) / (2.0 * Q), c = std::cos(w0), r = 2.0 * std::sqrt(A) * alpha;
    const double b0 = A * ((A + 1) + (A - 1) * c + r), b1 = -2 * A * ((A - 1) + (A + 1) * c), b2 = A * ((A + 1) + (A - 1) * c - r);
    const double a0 = (A + 1) - (A - 1) * c + r, a1 = 2 * ((A - 1) - (A + 1) * c), a2 = (A + 1) - (A - 1) * c - r;
    shelf = {b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0};
  }
  {
    const double Q = 0.5, fc = 38.0;
    const double w0 = 2.0 * kPi * (fc / fs), alpha = std::sin(w0) / (2.0 * Q), c = std::cos(w0);
    const double b0 = (1 + c) / 2, b1 = -(1 + c), b2 = (1 + c) / 2, a0 = 1 + alpha, a1 = -2 * c, a2 = 1 - alpha;
    hp = {b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0};
  }
  for (int col = 0; col < 4; ++col) {                 // M's columns: kLdSeg zero inputs from each unit state
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    s[col] = 1.0;
    for (int t = 0; t < cnk::kLdSeg; ++t) (void)cnk::ld_step(shelf, hp, s, 0.0);
    for (int r = 0; r < 4; ++r) M[4 * r + col] = s[r];
  }
}

void conan_ctx_loud_norm(conan_ctx* ctx, const conan_loudness_cfg& c, const float* x, int64_t x_ld, int n, const int64_t* samples, float* y,
                         int64_t y_ld, double* stats, hipStream_t st) {
  using ch::Error;
  if (c.sample_rate < 8000 || c.sample_rate > 192000) throw Error(CONAN_ERR_INVALID, "loud_norm: sample_rate must be in 8000 .. 192000 Hz");
  if (!std::isfinite(c.target_lufs)) throw Error(CONAN_ERR_INVALID, "loud_norm: target_lufs must be finite");
  if (c.peak_limit != 0 && c.peak_limit != 1) throw Error(CONAN_ERR_INVALID, "loud_norm: peak_limit must be 0 or 1");
  if (c.reserved[0] || c.reserved[1] || c.reserved[2]) throw Error(CONAN_ERR_INVALID, "loud_norm: reserved fields must be 0");
  if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, "loud_norm: n must be in 1 .. 65535");
  const double fs = (double)c.sample_rate;
  // every row is checked and planned before anything is launched
  std::vector<cnk::LdRow> rows((size_t)n);
  std::vector<int> edges, blocks, lu;
  long long segs = 0, longest = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t N = samples[i];
    if (N < 1 || N > (1ll << 30)) throw Error(CONAN_ERR_INVALID, "loud_norm: samples must be in 1 .. 2^30");
    if (N > x_ld || (y && N > y_ld)) throw Error(CONAN_ERR_INVALID, "loud_norm: a row is longer than its stride");
    if ((double)N < kTg * fs) throw Error(CONAN_ERR_INVALID, "loud_norm: a row is shorter than one gating block (0.4 s)");
    // the gating blocks, in double and in this order (pyloudnorm's meter): a Python slice truncates at the signal's end
    const double T = (double)N / fs;
    const long long nb = (long long)(std::nearbyint((T - kTg) / (kTg * kStep)) + 1.0);
    if (nb < 1 || nb > (1ll << 24)) throw Error(CONAN_ERR_INVALID, "loud_norm: gating block count out of range");
    lu.resize((size_t)nb * 2);
    for (long long j = 0; j < nb; ++j) {
      const long long lo = (long long)(kTg * ((double)j * kStep) * fs), hi = (long long)(kTg * ((double)j * kStep + 1.0) * fs);
      lu[2 * j] = (int)std::min<long long>(lo, N); lu[2 * j + 1] = (int)std::min<long long>(hi, N);
    }
    std::vector<int> e(lu.begin(), lu.end());
    std::sort(e.begin(), e.end());
    e.erase(std::unique(e.begin(), e.end()), e.end());
    if (e.front() != 0) throw Error(CONAN_ERR_INVALID, "loud_norm: the first gating block does not start at sample 0");
    for (size_t k = 0; k + 3 < e.size(); ++k)
      if (e[k + 3] - e[k] < cnk::kLdSeg) throw Error(CONAN_ERR_UNSUPPORTED, "loud_norm: more than three block edges inside one segment");
    cnk::LdRow& R = rows[i];
    memset(&R, 0, sizeof(R));
    R.samples = N; R.seg0 = segs; R.nseg = (int)((N + cnk::kLdSeg - 1) / cnk::kLdSeg);
    R.edge0 = (int)edges.size(); R.nedges = (int)e.size(); R.blk0 = (int)(blocks.size() / 2); R.nblocks = (int)nb;
    for (long long j = 0; j < nb; ++j) {
      blocks.push_back((int)(std::lower_bound(e.begin(), e.end(), lu[2 * j]) - e.begin()));
      blocks.push_back((int)(std::lower_bound(e.begin(), e.end(), lu[2 * j + 1]) - e.begin()));
    }
    edges.insert(edges.end(), e.begin(), e.end());
    segs += R.nseg; longest = std::max<long long>(longest, N);
    if (edges.size() > (size_t)INT_MAX / 2 || blocks.size() > (size_t)INT_MAX / 2) throw Error(CONAN_ERR_INVALID, "loud_norm: too many gating blocks in one call");
  }
  // the table (rows | edges | blocks) and the scratch arrays behind it, in the context's workspace
  const size_t o_rows = 0, o_edges = align8(o_rows + rows.size() * sizeof(cnk::LdRow)), o_blocks = align8(o_edges + edges.size() * sizeof(int)),
               table = align8(o_blocks + blocks.size() * sizeof(int));
  const size_t o_state = table, o_part = o_state + (size_t)segs * 4 * sizeof(double), o_bin = o_part + (size_t)segs * cnk::kLdSlots * sizeof(double),
               o_z = o_bin + align8(edges.size() * sizeof(double)), o_l = o_z + (blocks.size() / 2) * sizeof(double), o_gain = o_l + (blocks.size() / 2) * sizeof(double),
               o_peak = o_gain + (size_t)n * 2 * sizeof(double), total = o_peak + align8((size_t)segs * sizeof(float));
  char* ws = reinterpret_cast<char*>(ctx->workspace((total + 3) / 4, st));
  char* h = static_cast<char*>(ctx->loud_stage.take(table));
  memcpy(h + o_rows, rows.data(), rows.size() * sizeof(cnk::LdRow));
  memcpy(h + o_edges, edges.data(), edges.size() * sizeof(int));
  memcpy(h + o_blocks, blocks.data(), blocks.size() * sizeof(int));
  HIP_CHECK(hipMemcpyAsync(ws, h, table, hipMemcpyHostToDevice, st));
  ctx->loud_stage.sent(st);

  cnk::LoudArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.x_ld = x_ld; a.y = y; a.y_ld = y_ld; a.n = n;
  a.rows = reinterpret_cast<const cnk::LdRow*>(ws + o_rows); a.edges = reinterpret_cast<const int*>(ws + o_edges); a.blocks = reinterpret_cast<const int*>(ws + o_blocks);
  a.state = reinterpret_cast<double*>(ws + o_state); a.part = reinterpret_cast<double*>(ws + o_part); a.binsum = reinterpret_cast<double*>(ws + o_bin);
  a.z = reinterpret_cast<double*>(ws + o_z); a.l = reinterpret_cast<double*>(ws + o_l); a.gain = reinterpret_cast<double*>(ws + o_gain);
  a.peak = reinterpret_cast<float*>(ws + o_peak);
  a.stats = stats;
  conan_k_weighting(fs, a.shelf, a.hp, a.M);
  a.block_len = kTg * fs;
  a.target = (double)c.target_lufs; a.peak_limit = c.peak_limit;
  a.tiles = (int)((longest + cnk::kLdTile - 1) / cnk::kLdTile);
  cnk::launch_loud_measure(a, st);
  HIP_CHECK(hipGetLastError());
  if (y) {
    cnk::launch_loud_apply(a, longest, st);
    HIP_CHECK(hipGetLastError());
  }
}
