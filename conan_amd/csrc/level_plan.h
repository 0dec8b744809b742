// The streaming leveller's host planning (include/conan_hip.h, conan_level_cfg): where the meter's gating blocks lie and which of
// them a chunk touches.  Plain C++ with no HIP in it, so a stand-alone program can exercise it (tests/test_out_level_cpu.py);
// kernels.h includes it for the types the kernels read.  plan_call is the input leveller's and conan_level's plan - the update
// instant at the chunk's start or inside it; plan_end is the output leveller's (level_out.hip) - the instant at the chunk's end.
#pragma once
#include <algorithm>
#include <climits>
#include <cstring>

namespace cnk {

constexpr int kLdSeg = 128;                      // samples per segment of the meter (why 128)
constexpr int kLvBlocks = 8;                     // gating blocks that can overlap a chunk's complete segments (the host checks)
struct LvCall {                                  // one chunk
  long long pos0;                                // stream position of the chunk's first sample
  int m;                                         // samples (1 .. U)
  int inst;                                      // 1: an update instant lies in [pos0, pos0 + m) (at most one: m <= U) - or, in
                                                 // plan_end's calls, at pos0 + m
  int u, J;                                      // ... at pos0 + u, with J_k complete blocks
  int j0, nblk;                                  // the blocks that overlap the chunk's complete segments: j0 .. j0 + nblk - 1
  int lo[kLvBlocks], hi[kLvBlocks];              // their edges relative to the first segment's start, pos0 - pos0 % kLdSeg
};

}  // namespace cnk

namespace level {

constexpr double kTg = 0.4, kStep = 0.25;      // the meter's gating block length (s) and step (conan_loud_norm's)

inline long long block_lo(long long j, double fs) { return (long long)(kTg * ((double)j * kStep) * fs); }
inline long long block_hi(long long j, double fs) { return (long long)(kTg * ((double)j * kStep + 1.0) * fs); }

// J = the number of blocks with hi_j <= p (hi_j never decreases with j)
inline long long blocks_ended(long long p, double fs) {
  long long j = std::max(0ll, (long long)((double)p / (kTg * kStep * fs)) - 8);
  while (j > 0 && block_hi(j - 1, fs) > p) --j;
  while (block_hi(j, fs) <= p) ++j;
  return j;
}

// the blocks over the complete segments of [pos0 - pos0 % kLdSeg, pos0 + m); null, or why the chunk cannot be planned
inline const char* plan_blocks(cnk::LvCall& c, double fs) {
  const long long base = c.pos0 - (c.pos0 & (cnk::kLdSeg - 1)), end = base + (c.pos0 - base + c.m) / cnk::kLdSeg * cnk::kLdSeg;
  if (end > base) {
    const long long j0 = blocks_ended(base, fs);
    int nb = 0;
    while (block_lo(j0 + nb, fs) < end) {
      if (nb == cnk::kLvBlocks) return "too many gating blocks over one call";
      c.lo[nb] = (int)(block_lo(j0 + nb, fs) - base); c.hi[nb] = (int)(block_hi(j0 + nb, fs) - base);
      ++nb;
    }
    if (j0 + nb > INT_MAX) return "the stream is too long";
    c.j0 = (int)j0; c.nblk = nb;
  }
  return nullptr;
}

// The chunk [pos0, pos0 + m) of a stream at rate fs with update interval U: its instant and the blocks over its complete segments.
// Returns null, or why the chunk cannot be planned (c is then meaningless).
inline const char* plan_call(long long pos0, int m, int U, double fs, cnk::LvCall& c) {
  memset(&c, 0, sizeof(c));
  c.pos0 = pos0; c.m = m;
  const long long uk = (pos0 + U - 1) / U * U;      // the first instant at or behind pos0
  if (uk < pos0 + m) {
    const long long J = blocks_ended(uk, fs);
    if (J > INT_MAX) return "the stream is too long";
    c.inst = 1; c.u = (int)(uk - pos0); c.J = (int)J;
  }
  return plan_blocks(c, fs);
}

// The output leveller's chunk: [pos0, pos0 + m) with pos0 = u_k a multiple of U and 1 <= m <= U, planned for a meter that runs
// BEHIND the chunk's ramp.  The blocks are plan_call's; the instant is u_{k+1} = pos0 + U at the chunk's end (u = m = U, J = J_{k+1}),
// and a short last chunk (m < U) reaches none.  What this plan closes, gates and lists is what plan_call's start-of-chunk plan of
// chunk k + 1 does after chunk k's blocks: U is a multiple of kLdSeg, so no segment straddles u_{k+1}.
inline const char* plan_end(long long pos0, int m, int U, double fs, cnk::LvCall& c) {
  memset(&c, 0, sizeof(c));
  if (U < cnk::kLdSeg || U % cnk::kLdSeg) return "the update interval must be a multiple of 128";
  if (pos0 < 0 || pos0 % U) return "a levelled row must start at a multiple of segment * hop samples of its vocoder stream";
  if (m < 1 || m > U) return "a levelled row carries 1 .. segment * hop samples";
  c.pos0 = pos0; c.m = m;
  if (m == U) {
    const long long J = blocks_ended(pos0 + U, fs);
    if (J > INT_MAX) return "the stream is too long";
    c.inst = 1; c.u = m; c.J = (int)J;
  }
  return plan_blocks(c, fs);
}

}  // namespace level
