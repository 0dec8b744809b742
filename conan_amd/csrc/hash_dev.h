// The 64-bit position hash the comfort noise (comfort.hip) and the output watermark (watermark.hip) share: the finaliser of splitmix64
// on seed + (j + 1) * golden.  tests/comfort_ref.py, hash64.
#pragma once

namespace cnk {

constexpr unsigned long long kHashGolden = 0x9E3779B97F4A7C15ull;

// the finaliser alone: a caller that walks consecutive j carries seed + (j + 1) * golden along as an addition
__host__ __device__ __forceinline__ unsigned long long hash64_mix(unsigned long long z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

__host__ __device__ __forceinline__ unsigned long long hash64(unsigned long long seed, unsigned long long j) { return hash64_mix(seed + (j + 1) * kHashGolden); }

}  // namespace cnk
