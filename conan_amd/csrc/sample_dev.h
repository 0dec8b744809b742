// Device routines of the sample formats (include/conan_hip.h, CONAN_SAMPLE_*), shared by resample.hip (the wav-in and wav-out rows,
// conan_convert_samples), conceal.hip, echo.hip and echo_delay.hip (the repair, the canceller and its delay estimator work on a row in its own format).
#pragma once
#include "kernels.h"

namespace cnk {

// ---- sample formats (include/conan_hip.h, CONAN_SAMPLE_*).  Decoding is exact: every code is an integer of at most 16 bits over 32768.
// decode_sample: the value of the code in the low bits of v (wd: the whole dword, which an f32 sample is).  Integer arithmetic on the
// word; the format only selects among values.  No table in memory.
__device__ __forceinline__ float decode_sample(int fmt, unsigned wd, unsigned v) {
  const int s16 = (int)(short)(v & 0xFFFFu);
  const unsigned u = ~v & 0xFFu;                                         // mu-law
  const int tu = (int)((((u & 15u) << 3) + 0x84u) << ((u >> 4) & 7u));
  const int vu = (u & 0x80u) ? 0x84 - tu : tu - 0x84;
  const unsigned al = (v ^ 0x55u) & 0xFFu;                               // A-law
  const unsigned m = al & 15u, e = (al >> 4) & 7u;
  const int ta = e == 0 ? (int)((m << 4) + 8u) : (int)(((m << 4) + 0x108u) << (e - 1u));
  const int va = (al & 0x80u) ? ta : -ta;
  const int q = fmt == kFmtS16 ? s16 : (fmt == kFmtUlaw ? vu : va);
  return fmt == kFmtF32 ? __uint_as_float(wd) : (float)q * (1.f / 32768.f);
}

// Sample i of a row in format fmt: ONE unconditional dword load - the aligned dword that holds the sample; the row starts on a dword and
// its stride is whole dwords, so the dword lies inside the row - then decode_sample on the loaded word, never a branch around the load.
__device__ __forceinline__ float load_sample(int fmt, const void* row, long long i) {
  const int sh = fmt == kFmtF32 ? 2 : (fmt == kFmtS16 ? 1 : 0);          // log2(bytes per sample)
  const long long b = i << sh;                                           // the sample's first byte in the row
  const unsigned wd = reinterpret_cast<const unsigned*>(row)[b >> 2];
  const unsigned v = wd >> (((unsigned)b & 3u) * 8u);                    // the sample in the low bits
  return decode_sample(fmt, wd, v);
}

// s = clamp(rint(x * 32768), -32768, 32767), ties to even (x * 32768 is exact: a power of two; the clamps come before the
// conversion, so that a product beyond the int range is never converted), then the format's code of s.
__device__ __forceinline__ unsigned encode_sample(int fmt, float x) {
  const int s = (int)fminf(fmaxf(rintf(x * 32768.f), -32768.f), 32767.f);
  if (fmt == kFmtS16) return (unsigned)s & 0xFFFFu;
  if (fmt == kFmtUlaw) {
    int p = s >> 2;
    const bool neg = p < 0;
    p = min(neg ? -p : p, 8159) + 0x21;                                  // 0x21 .. 0x2000
    const int seg = 26 - __clz(p);                                       // thresholds 2^(k + 6) - 1 below p: floor(log2 p) - 5, 0 .. 8
    const unsigned u = seg >= 8 ? 0x7Fu : (unsigned)((seg << 4) | ((p >> (seg + 1)) & 15));
    return u ^ (neg ? 0x7Fu : 0xFFu);
  }
  int p = s >> 3;
  const bool neg = p < 0;
  p = neg ? -p - 1 : p;                                                  // 0 .. 4095
  const int seg = max(27 - __clz(p | 1), 0);                             // thresholds 2^(k + 5) - 1 below p: floor(log2 p) - 4, 0 .. 7
  const unsigned a = (unsigned)((seg << 4) | ((seg < 2 ? p >> 1 : p >> seg) & 15));
  return a ^ (neg ? 0x55u : 0xD5u);
}

// the 16-bit view of a decoded sample, as the echo canceller and its delay estimator read a row; a non-finite value counts as 0
__device__ __forceinline__ float echo_finite(float v) { return fabsf(v) <= 3.402823466e38f ? v : 0.f; }
__device__ __forceinline__ int echo_q(float v) { return (int)(short)encode_sample(kFmtS16, v); }

// Sample i of a row of n samples in format fmt (uniform over the caller's wave).  Every lane of an aligned group of four consecutive
// samples must call it together (lane = i mod 4, also the lanes with i >= n, which store nothing): 16- and 8-bit codes travel to the
// lane that owns the dword and leave as one dword store; the ragged last dword of a row leaves as halfword / byte stores, so that
// no byte past the row's n samples is written.
__device__ __forceinline__ void store_sample(int fmt, void* row, long long i, long long n, float x) {
  if (fmt == kFmtF32) {
    if (i < n) reinterpret_cast<float*>(row)[i] = x;
    return;
  }
  const unsigned c = encode_sample(fmt, x);
  const unsigned c1 = __shfl_down(c, 1), c2 = __shfl_down(c, 2), c3 = __shfl_down(c, 3);
  if (fmt == kFmtS16) {
    if (i & 1) return;
    if (i + 1 < n) reinterpret_cast<unsigned*>(row)[i >> 1] = c | (c1 << 16);
    else if (i < n) reinterpret_cast<unsigned short*>(row)[i] = (unsigned short)c;
    return;
  }
  const long long g = i & ~3ll;
  if (g + 3 < n) {
    if (i == g) reinterpret_cast<unsigned*>(row)[i >> 2] = c | (c1 << 8) | (c2 << 16) | (c3 << 24);
  } else if (i < n) {
    reinterpret_cast<unsigned char*>(row)[i] = (unsigned char)c;
  }
}

}  // namespace cnk
