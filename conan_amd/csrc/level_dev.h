// The streaming leveller's device routines (include/conan_hip.h, conan_level_cfg), shared by level.hip (level_stream_kernel,
// level_signal_kernel: meter and ramp in one launch) and level_out.hip (level_out_meter_kernel: the meter alone, behind the ramp that
// level_out_apply_kernel wrote).  lv_meter is the one copy of the segment passes, the scan, the block sums, the gating and the gain;
// lv_ramp is the one copy of a sample's gain and product - so every kernel that levels computes conan_level's bits.
#pragma once
#include <climits>
#include <cmath>

#include "kernels.h"

namespace cnk {

struct LvShared {
  float buf[kLvSegs * kLdStride];      // pending tail + the chunk: segment l at l * kLdStride (the loudness kernels' banking)
  double st[kLvSegs * 4];              // the segments' end states, then (scan) start states
  double part[kLvSegs * kLdSlots];     // per segment: the sums over its bins
  int edge[kLvSegs * 4];               // per segment: the block edges strictly inside it, ascending (INT_MAX: none)
  double rsum[kLvThreads];
  int rcnt[kLvThreads];
  float rpk[2 * kLvThreads];
  double g[4];                         // the ramps: {G_{k-1}, G_k} before the instant, {G_{k-1}, G_k} from it on
};

// sum and count over the workgroup in one fixed order: lane sums, then a binary tree over the lanes
__device__ __forceinline__ void lv_reduce(LvShared& sh, double sum, int cnt, double& tsum, int& tcnt) {
  sh.rsum[threadIdx.x] = sum; sh.rcnt[threadIdx.x] = cnt;
  __syncthreads();
  for (int w = kLvThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { sh.rsum[threadIdx.x] = sh.rsum[threadIdx.x] + sh.rsum[threadIdx.x + w]; sh.rcnt[threadIdx.x] += sh.rcnt[threadIdx.x + w]; }
    __syncthreads();
  }
  tsum = sh.rsum[0]; tcnt = sh.rcnt[0];
  __syncthreads();
}

// l = -0.691 + 10 log10 z with the product and the sum rounded separately: no contraction, so every inlined copy computes the same bits
__device__ __forceinline__ double lv_lufs(double z) { return __dadd_rn(-0.691, __dmul_rn(10.0, log10(z))); }

// One sample of a ramp: g = G_{k-1} + (G_k - G_{k-1}) * (n / U) for the n-th sample of the interval (1 .. U), two roundings behind
// the division; y = f32(f64(x) * g), one rounding; then the clip.
__device__ __forceinline__ float lv_ramp(double gm, double gc, int n, double U, float x, int clip) {
  const double frac = (double)n / U;
  const double g = __dadd_rn(gm, __dmul_rn(gc - gm, frac));
  float v = (float)__dmul_rn((double)x, g);
  if (clip) v = fminf(fmaxf(v, -1.f), 1.f);
  return v;
}

// The meter's part of one chunk of one stream: c.m samples at x (position c.pos0 on) into the slot's state, and - c.inst - the gating
// and the gain of the instant at c.pos0 + c.u (0 <= c.u <= c.m: samples before it count towards its peak).  Leaves the chunk in
// sh.buf behind the pending tail and the ramps' gains in sh.g.  Called by every thread of a kLvThreads workgroup with the same
// arguments; c lives in LDS, in global memory or in the kernel's arguments.  Every ring index and the tail count come from c, never
// from the state.
__device__ __forceinline__ void lv_meter(const LvFilter& f, const LvCfg& cfg, LvState* S, double* zr, double* lr, int zcap, const LvCall& c, const float* x,
                                         LvShared& sh) {
  const int tid = threadIdx.x;
  if (c.pos0 == 0) {      // the first chunk of an utterance starts the meter and the gain (the rings need no clearing)
    if (tid < 4) S->carry[tid] = 0.0;
    if (tid < kLvBlocks) S->acc[tid] = 0.0;
    if (tid == 0) { S->Gm = cfg.g_init; S->Gc = cfg.g_init; S->peak = 0.0; S->stat[0] = -INFINITY; S->stat[1] = cfg.g_init; S->stat[2] = 0.0; S->stat[3] = 0.0; }
    __syncthreads();
  }
  const int tail = (int)(c.pos0 & (kLdSeg - 1)), total = tail + c.m, nseg = total / kLdSeg, rem = total - nseg * kLdSeg;
  // 1. pending tail + chunk into LDS; the peaks before and from the instant on
  const int split = c.inst ? c.u : c.m;
  float pa = 0.f, pb = 0.f;
  for (int i = tid; i < kLvSegs * kLdSeg; i += kLvThreads) {
    float v = 0.f;
    if (i < tail) v = S->tail[i];
    else if (i < total) {
      v = x[i - tail];
      if (i - tail < split) pa = fmaxf(pa, fabsf(v)); else pb = fmaxf(pb, fabsf(v));
    }
    sh.buf[(i >> 7) * kLdStride + (i & (kLdSeg - 1))] = v;
  }
  sh.rpk[2 * tid] = pa; sh.rpk[2 * tid + 1] = pb;
  __syncthreads();
  for (int w = kLvThreads / 2; w > 0; w >>= 1) {
    if (tid < w) { sh.rpk[2 * tid] = fmaxf(sh.rpk[2 * tid], sh.rpk[2 * (tid + w)]); sh.rpk[2 * tid + 1] = fmaxf(sh.rpk[2 * tid + 1], sh.rpk[2 * (tid + w) + 1]); }
    __syncthreads();
  }
  const double peak_a = (double)sh.rpk[0], peak_b = (double)sh.rpk[1];
  // 2. the complete segments
  if (nseg > 0) {
    const float* w = sh.buf + tid * kLdStride;
    if (tid < nseg) {      // state pass
      double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
      for (int t = 0; t < kLdSeg; ++t) (void)ld_step(f.shelf, f.hp, s, (double)w[t]);
      sh.st[4 * tid] = s[0]; sh.st[4 * tid + 1] = s[1]; sh.st[4 * tid + 2] = s[2]; sh.st[4 * tid + 3] = s[3];
    }
    __syncthreads();
    if (tid == 0) {        // scan from the carried state
      double cs[4] = {S->carry[0], S->carry[1], S->carry[2], S->carry[3]};
      for (int j = 0; j < nseg; ++j) {
        const double e[4] = {sh.st[4 * j], sh.st[4 * j + 1], sh.st[4 * j + 2], sh.st[4 * j + 3]};
        sh.st[4 * j] = cs[0]; sh.st[4 * j + 1] = cs[1]; sh.st[4 * j + 2] = cs[2]; sh.st[4 * j + 3] = cs[3];
        double nx[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) nx[r] = fma(f.M[4 * r + 3], cs[3], fma(f.M[4 * r + 2], cs[2], fma(f.M[4 * r + 1], cs[1], fma(f.M[4 * r], cs[0], e[r]))));
        cs[0] = nx[0]; cs[1] = nx[1]; cs[2] = nx[2]; cs[3] = nx[3];
      }
      S->carry[0] = cs[0]; S->carry[1] = cs[1]; S->carry[2] = cs[2]; S->carry[3] = cs[3];
    }
    __syncthreads();
    if (tid < nseg) {      // energy pass: the segment's bins between the block edges inside it
      const int t0 = tid * kLdSeg;
      int e0 = INT_MAX, e1 = INT_MAX, e2 = INT_MAX;
      for (int b = 0; b < 2 * c.nblk; ++b) {
        const int v = b < c.nblk ? c.lo[b] : c.hi[b - c.nblk];
        if (v <= t0 || v >= t0 + kLdSeg || v == e0 || v == e1 || v == e2) continue;
        if (v < e0) { e2 = e1; e1 = e0; e0 = v; }
        else if (v < e1) { e2 = e1; e1 = v; }
        else if (v < e2) e2 = v;
      }
      sh.edge[4 * tid] = e0; sh.edge[4 * tid + 1] = e1; sh.edge[4 * tid + 2] = e2; sh.edge[4 * tid + 3] = INT_MAX;
      double s[4] = {sh.st[4 * tid], sh.st[4 * tid + 1], sh.st[4 * tid + 2], sh.st[4 * tid + 3]};
      double* part = sh.part + tid * kLdSlots;
      part[1] = 0.0; part[2] = 0.0; part[3] = 0.0;
      int k = 0, next = e0;
      double acc = 0.0;
#pragma unroll 4
      for (int t = 0; t < kLdSeg; ++t) {
        if (t0 + t == next) {      // rare: at most kLdSlots - 1 times per segment
          part[k] = acc;
          ++k; acc = 0.0;
          next = k == 1 ? e1 : (k == 2 ? e2 : INT_MAX);
        }
        const double yv = ld_step(f.shelf, f.hp, s, (double)w[t]);
        acc = fma(yv, yv, acc);
      }
      part[k] = acc;
    }
    __syncthreads();
    if (tid < c.nblk) {    // block tid: the segments in ascending order, each segment's bins inside the block in ascending order
      const int lo = c.lo[tid], hi = c.hi[tid], j = c.j0 + tid;
      double a = S->acc[j % kLvBlocks];
      for (int s = 0; s < nseg; ++s) {
        const int t0 = s * kLdSeg, t1 = t0 + kLdSeg;
        if (hi <= t0 || lo >= t1) continue;
        double p = 0.0; bool any = false;
        int bs = t0;
        for (int k = 0; k < kLdSlots && bs < t1; ++k) {
          const int be = min(sh.edge[4 * s + k], t1);
          if (bs >= lo && be <= hi) { p = any ? p + sh.part[s * kLdSlots + k] : sh.part[s * kLdSlots + k]; any = true; }
          bs = be;
        }
        if (any) a += p;
      }
      if (hi <= nseg * kLdSeg) {      // the block is complete
        const double z = a / f.block_len;
        zr[j % zcap] = z; lr[j % zcap] = lv_lufs(z);
        a = 0.0;
      }
      S->acc[j % kLvBlocks] = a;
    }
  }
  // 3. the new pending tail (every read of the old one is behind the barriers above)
  if (tid < rem) S->tail[tid] = sh.buf[nseg * kLdStride + tid];
  __syncthreads();
  // 4. the update instant: gate the window, form G_k
  if (c.inst) {
    const int first = max(0, c.J - cfg.window), cnt = c.J - first;
    double sum = 0.0; int n = 0;
    for (int i = tid; i < cnt; i += kLvThreads) {
      const int q = (first + i) % zcap;
      if (lr[q] >= -70.0) { sum += zr[q]; ++n; }
    }
    double tsum; int tcnt;
    lv_reduce(sh, sum, n, tsum, tcnt);
    double L = -INFINITY;
    if (tcnt > 0) {
      const double rel = __dadd_rn(lv_lufs(tsum / (double)tcnt), -10.0);
      sum = 0.0; n = 0;
      for (int i = tid; i < cnt; i += kLvThreads) {
        const int q = (first + i) % zcap;
        const double l = lr[q];
        if (l > rel && l > -70.0) { sum += zr[q]; ++n; }
      }
      lv_reduce(sh, sum, n, tsum, tcnt);
      if (tcnt > 0) L = lv_lufs(tsum / (double)tcnt);
    }
    if (tid == 0) {
      const double P = fmax(S->peak, peak_a), Gp = S->Gc;
      double G = Gp;
      if (L != -INFINITY) G = pow(10.0, fmin(fmax(cfg.target - L, -cfg.cut), cfg.boost) / 20.0);
      if (cfg.peak_limit && G * P > 1.0) G = 1.0 / P;
      sh.g[0] = S->Gm; sh.g[1] = Gp; sh.g[2] = Gp; sh.g[3] = G;
      S->Gm = Gp; S->Gc = G;
      S->stat[0] = L; S->stat[1] = G; S->stat[2] = P; S->stat[3] = (double)c.J;
    }
  } else if (tid == 0) {
    sh.g[0] = S->Gm; sh.g[1] = S->Gc; sh.g[2] = sh.g[0]; sh.g[3] = sh.g[1];
  }
  if (tid == 0) S->peak = fmax(S->peak, fmax(peak_a, peak_b));
  __syncthreads();
}

}  // namespace cnk
