// The equaliser's device routines (include/conan_hip.h, conan_eq_cfg), shared by every kernel that filters: eq_step is the one copy of
// a section's step and eq_chunk the one copy of the section passes, the scan and the pending tail - so every kernel that filters
// computes conan_eq's bits.  Every product and sum is a single rounded f64 operation: eq_step and eq_scan are compiled with
// contraction off (the pragma in their bodies; the __dmul_rn family is plain operators in this toolchain's headers and fuses once it
// is inlined), and tests/eq_ref.py restates the law in Python floats bit for bit.  f64 denormals are kept (the compiler's default
// for f64 on gfx950): a decaying state passes through them.
#pragma once
#include <cfloat>

#include "kernels.h"

namespace cnk {

struct EqShared {
  double buf[kEqSegs * kEqStride];     // pending tail + the chunk, then each section's output: segment l at l * kEqStride
  double st[kEqSegs * 2];              // the segments' zero-state end states, then (scan) their start states; entry nseg: the carry
};

// Transposed direct form II: y = b0 x + s0; s0' = (b1 x - a1 y) + s1; s1' = b2 x - a2 y.
__device__ __forceinline__ double eq_step(const EqSec& f, double& s0, double& s1, double x) {
#pragma clang fp contract(off)
  const double y = f.b0 * x + s0;
  const double p1 = f.b1 * x, q1 = f.a1 * y, p2 = f.b2 * x, q2 = f.a2 * y;
  s0 = (p1 - q1) + s1;
  s1 = p2 - q2;
  return y;
}

// The state at the next segment's start: (M00 c0 + M01 c1) + e0, (M10 c0 + M11 c1) + e1.
__device__ __forceinline__ void eq_scan(const EqSec& f, double& c0, double& c1, double e0, double e1) {
#pragma clang fp contract(off)
  const double m00 = f.M[0] * c0, m01 = f.M[1] * c1, m10 = f.M[2] * c0, m11 = f.M[3] * c1;
  const double n0 = (m00 + m01) + e0, n1 = (m10 + m11) + e1;
  c0 = n0; c1 = n1;
}

// One chunk of one row: c.m samples (1 .. kEqMaxCall) at x, utterance samples c.pos0 on, -> y (may be x) through sec[0 .. c.nsec),
// and the row's state to S.  Called by every thread of a kEqThreads workgroup with the same arguments; c lives in LDS, in global
// memory or in the kernel's arguments.  The tail count and every index come from c, never from the state.
__device__ __forceinline__ void eq_chunk(const EqSec* sec, EqState* S, const EqCall& c, const float* x, float* y, EqShared& sh) {
  const int tid = threadIdx.x;
  const int tail = c.tail, m = c.m, total = tail + m, nseg = total / kEqSeg, rem = total - nseg * kEqSeg;
  // 1. pending tail + chunk into LDS as f64; a non-finite sample counts as 0.  Loads at clamped addresses, then a select.
  for (int i = tid; i < kEqSegs * kEqSeg; i += kEqThreads) {
    const float tv = S->tail[min(i, kEqSeg - 1)];
    const float xv = x[min(max(i - tail, 0), m - 1)];
    float v = i < tail ? tv : (i < total ? xv : 0.f);
    v = fabsf(v) <= FLT_MAX ? v : 0.f;
    sh.buf[(i / kEqSeg) * kEqStride + (i & (kEqSeg - 1))] = (double)v;
  }
  __syncthreads();
  // 2. the new pending tail (every read of the old one is behind the barrier) and the record's positions
  if (tid < kEqSeg) S->tail[tid] = tid < rem ? (float)sh.buf[nseg * kEqStride + tid] : 0.f;
  if (c.fresh && tid < 2 * kEqMaxSec) S->carry[tid >> 1][tid & 1] = 0.0;
  if (tid == 0) { S->origin = c.origin; S->pos = c.pos0 + m; }
  // 3. the sections in order: section k + 1 reads section k's output in place
  double* w = sh.buf + min(tid, kEqSegs - 1) * kEqStride;
  for (int k = 0; k < c.nsec; ++k) {
    const EqSec f = sec[k];
    if (tid < nseg) {      // zero-state pass over the complete segments
      double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
      for (int t = 0; t < kEqSeg; ++t) (void)eq_step(f, s0, s1, w[t]);
      sh.st[2 * tid] = s0; sh.st[2 * tid + 1] = s1;
    }
    __syncthreads();
    if (tid == 0) {        // scan from the carried state: start' = (M00 c0 + M01 c1) + e0, (M10 c0 + M11 c1) + e1
      const double k0 = S->carry[k][0], k1 = S->carry[k][1];
      double c0 = c.fresh ? 0.0 : k0, c1 = c.fresh ? 0.0 : k1;
      for (int j = 0; j < nseg; ++j) {
        const double e0 = sh.st[2 * j], e1 = sh.st[2 * j + 1];
        sh.st[2 * j] = c0; sh.st[2 * j + 1] = c1;
        eq_scan(f, c0, c1, e0, e1);
      }
      sh.st[2 * nseg] = c0; sh.st[2 * nseg + 1] = c1;      // (nseg <= kEqSegs - 1)
      S->carry[k][0] = c0; S->carry[k][1] = c1;
    }
    __syncthreads();
    if (tid < nseg + (rem > 0 ? 1 : 0)) {      // output pass: every segment from its start state, the incomplete one over its samples
      double s0 = sh.st[2 * tid], s1 = sh.st[2 * tid + 1];
      const int len = tid < nseg ? kEqSeg : rem;
#pragma unroll 4
      for (int t = 0; t < len; ++t) w[t] = eq_step(f, s0, s1, w[t]);
    }
    __syncthreads();
  }
  // 4. the new samples, rounded once to f32; stores run over the lanes
  for (int t = tid; t < m; t += kEqThreads) {
    const int i = tail + t;
    y[t] = (float)sh.buf[(i / kEqSeg) * kEqStride + (i & (kEqSeg - 1))];
  }
  __syncthreads();
}

}  // namespace cnk
