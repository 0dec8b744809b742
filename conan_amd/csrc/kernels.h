// Device-side argument structs and launch wrappers of the conan_hip kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "level_plan.h"
#include "voice_layout.h"

namespace cnk {

#define HIP_CHECK(x) ::ch::hip_check((x), #x)


// A channel-last fp32 activation tensor [slot][row][C].
//  mode 0 (ring):   row(t) = (pos[slot] * rate + off + t) & lmask, slot = slots[i]
//  mode 1 (linear): row(t) = off + t,                          slot = i        (scratch / caller buffers)
struct TRef {
  float* base;
  long long slot_stride;  // floats between consecutive slots
  int C;                  // floats per row
  int lmask;              // ring length - 1 (mode 0)
  int rate;               // rows per frame (mode 0)
  int off;                // constant row offset
  int mode;
  int pad_;
};

// The device slot table (conan_streams::d_slots) holds the n active slots followed by kSlotTablePad copies of the last one: kernels
// whose tiles take several whole slots (conv_limb's ragged last tile) read entries past n without a clamp.
constexpr int kSlotTablePad = 32;

// decoder_mega's developer stamp buffer (CONAN_MEGA_STAMPS), in 8-byte words: [0, 128) per-operator end stamps, [128, 512) four
// stage stamps per operator, [512, 512 + 4 * kMegaMaxOps) the gather's stamps, then one XCC-mask word per group.
constexpr int kMegaMaxOps = 80;
constexpr int kMegaDbgGroupWords = 512 + 4 * kMegaMaxOps;
constexpr int kMegaDbgWords = kMegaDbgGroupWords + 64;

enum Act { ACT_NONE = 0, ACT_LRELU = 1, ACT_RELU = 2, ACT_GELU = 3, ACT_TANH = 4 };

// Bounded cross-workgroup waits.  Three kernels wait for other workgroups of their own launch (decoder_mega: group / grid
// barriers; emformer_fused: cluster exchange; resblock_pair: partner flags and the tile mailbox).  Forward progress rests on
// dispatch-order arguments; should one ever be violated, a waiter must not spin for ever - a hung GPU takes the
// whole box down.  Every such poll loop therefore carries a budget: after kSpinBudgetTicks of the 100 MHz s_memrealtime clock
// (50 ms; a healthy wait is microseconds) the waiter writes a code into the stream-set's guard block and LEAVES the wait (the
// launch then finishes with meaningless results); other waiters see the code and leave too.  The host reads the code through a
// host-mapped word at the next stream-ordered entry point and returns CONAN_ERR_HIP from then on (conan_streams::check_fault).
//   guard[0]     error code, device memory (agent scope): 0 = healthy
//   guard[2..3]  address of the host-mapped word the code is copied to
// The clock is read only every 256th poll iteration, and not at all by waits that end earlier.
// What counts against the budget is the time the waiter spent POLLING, not wall time: s_memrealtime keeps running while a queue's
// waves are descheduled (context-save preemption when several processes oversubscribe the hardware queues, a debugger halt), and a
// waiter restored together with its partner would otherwise see the whole pause as "spent" before the partner had a chance to
// arrive.  Two consecutive clock reads are 256 polls apart (~0.1-0.5 ms); a gap above kSpinGapTicks (1 ms) between them is taken
// for a deschedule and counts as 1 ms only (never as nothing: polls slowed down by a congested memory system must still run the
// budget down, a wait without an end takes the box with it).
constexpr unsigned long long kSpinBudgetTicks = 5000000ull;
constexpr unsigned long long kSpinGapTicks = 100000ull;
enum WaitCode { WAIT_MEGA_BARRIER = 1, WAIT_EMF_CLUSTER = 2, WAIT_PAIR_FLAG = 3, WAIT_PAIR_MAILBOX = 4, WAIT_RETIRED_5 = 5 /* (voc_chain, rounds 4-5: tools/experiments/voc_chain) */, WAIT_MEGA_ELECT = 6, WAIT_MEGA_DECIDED = 7, WAIT_MEGA_FLAGS = 8 };
struct SpinGuard { unsigned long long last = 0, acc = 0; unsigned it = 0; };
#if defined(__HIPCC__)
// true: give up (budget spent, or another wait of this stream-set already failed)
__device__ __forceinline__ bool spin_expired(SpinGuard& g, unsigned* guard, unsigned code) {
  if ((++g.it & 255u) != 0u || guard == nullptr) return false;
  if (__hip_atomic_load(guard, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return true;
  const unsigned long long now = __builtin_amdgcn_s_memrealtime();
  if (g.last != 0) { const unsigned long long d = now - g.last; g.acc += d < kSpinGapTicks ? d : kSpinGapTicks; }
  g.last = now;
  if (g.acc < kSpinBudgetTicks) return false;
  __hip_atomic_store(guard, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  unsigned* host = *reinterpret_cast<unsigned* const*>(guard + 2);
  if (host) __hip_atomic_store(host, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  return true;
}
#endif

// Causal / shifted 1-D convolution as an implicit GEMM on the f32 MFMA:
//   y[i][t][co] = epilogue( sum_{j<ktaps} sum_{ci<Cin} W[j][ci][co] * f(x[i][t + j*dil - pad_left][ci]) )
//   f(v)        = in_act(v)   (LeakyReLU only; the hot layers read tensors their producer stored activated)
//   epilogue(a) = ((out_act((a + bias[co]) * out_scale) + bvec[slot][co]) + res[i][t][co]) * m1[i][t] * m2[i][t]
// and, with shuffle_r > 1, the pixel-shuffled store y[i][t*r + co / Cq][co % Cq] (Cq = Cout / r) for
// weights whose output channels were permuted to j-major at pack time.
struct ConvArgs {
  TRef x;
  TRef y;
  TRef res;
  TRef m1, m2;          // per-row masks (C == 1)
  const float* w;       // packed [ktaps][Cin_pad/4][Cout_pad][4]
  const float* bias;    // [Cout_pad] or nullptr
  const float* bvec;    // per-slot broadcast vector [slot][bvec_stride] or nullptr (indexed by slots[i])
  const int* slots;     // [n]
  const int* pos;       // per-slot frame counters (indexed by slot) or nullptr
  const int* lens;      // per-batch valid output rows (or nullptr: all T rows valid)
  long long bvec_stride;
  int has_res, has_m1, has_m2;
  int Cin, Cin_pad, Cout, Cout_pad;
  int ktaps, dil, pad_left;
  int T;                // output rows per slot
  int n;                // slots in this batch
  int in_act;
  float in_slope;
  int out_act;
  float out_scale, out_slope;
  int shuffle_r;
  int Cin_alloc;        // packed rows per tap (Cin rounded up to 128, zero filled): K-steps may over-read safely
  // optional second output: LeakyReLU(y2_slope) of the stored value, written to a tensor with y's geometry (only the
  // base differs).  The consumer then reads pre-activated rows and its K loop needs no input transform.
  float* y2_base;
  float y2_slope;
  // the weights as bf16 limbs for conv_limb.hip (null: not packed): [Cout_pad16/16 column tiles][Cin/32 channel blocks][ktaps]
  // [3 limbs][64 lanes][8], lane = (packed column ct*16 + (lane & 15), channels cb*32 + 8*(lane >> 4) + e)
  const unsigned short* wl;
#ifdef CK_STAMPS
  unsigned long long* dbg;   // developer build only (tools/conv_bench -DCK_STAMPS): s_memtime stamps of block 1
#endif
};

struct ConvGroup {      // up to 3 independent problems in one launch
  ConvArgs p[3];
  int tile_start[4];    // filled by launch_conv: first tile of the q-th scheduled problem; [3] = total tiles
  int tiles_n[3];       // n-tiles of the q-th scheduled problem
  int order[3];         // q-th scheduled problem -> index into p[] (longest K first)
  // inter-block split-K (latency-bound layers with few tiles): K-steps of a tile are divided over `ksplit` blocks;
  // partial tiles go to `slab` ([tile][slice][TM*TN] floats), `counters` ([tile] ints, zero between launches)
  // elects the last-arriving block as the reducer.
  float* slab;
  int* counters;
  // balanced static schedule (filled by launch_conv for persistent launches): block b runs items
  // assign[b * assign_per + i], i = 0 .. until -1.  nullptr = round-robin over the grid.
  const int* assign;
  int assign_per;
  int ksplit;
  // tiles [0, split_from) are whole work items; only the tiles from split_from on are divided into `ksplit` K slices (the
  // tail of a launch whose tile count is not a multiple of the CU count: 320 tiles on 256 CUs = 256 tiles + 64 x 4
  // quarter tiles - every CU gets 1.25 tiles of work instead of some getting two).  0: every tile is split.
  int split_from;
  // 1: the split-K hand-off is additionally bracketed by agent-scope release / acquire fences (CONAN_FENCED=1, a
  // developer cross-check of the fence-free default: write-through stores, ticket, sc1 loads)
  int fenced;
};

// Tile configurations of conv_mfma (block = 256 threads = 4 waves).
enum ConvCfg { CFG_128x64 = 0, CFG_64x64 = 1, CFG_128x32 = 2, CFG_32x64_K2 = 3, CFG_32x32_K4 = 4, CFG_64x32_K2 = 5,
               CFG_64x64_KS64 = 6, CFG_128x32_KS64 = 7, NUM_CFG };
int conv_cfg_ks(int cfg);          // K-step of the configuration
bool conv_cfg_splitk(int cfg);     // the build carries the inter-block split-K hand-off
const char* conv_cfg_name(int cfg);  // the kernel's name as rocprofv3 prints it
int conv_cfg_tm(int cfg);
int conv_cfg_tn(int cfg);
void launch_conv(const ConvGroup& g, int nprob, int cfg, hipStream_t st, int num_cu = 256);

// A convolution with few rows per slot and a long K (ups.0) as a split-K GEMM in the limb arithmetic (conv_tall.hip): tiles of 128 rows
// of any slots x 128 columns, items = (tile, K slice), the slices' partial tiles summed in slice order by the last arrival.
struct ConvTallArgs {
  ConvArgs p;
  int S, nbps;            // K slices per tile, (tap, 32-channel) blocks per slice (even)
  int mtiles, ntiles;
  float* slab;            // [tile][slice][128 x 128] partial tiles
  int* counters;          // [tile][4 matrix waves] tickets, zero before and after every launch
};
bool conv_tall_supported(const ConvArgs& a);
bool conv_tall_plan(const ConvArgs& a, int num_cu, int plan_n, ConvTallArgs* out, long long slab_floats, int max_counters, int max_T = 32);
void launch_conv_tall(const ConvTallArgs& g, hipStream_t st);

// The same convolution with every fp32 product as six bf16 limb products on the bf16 MFMA (conv_limb.hip); covers the
// subset of ConvArgs that conv_limb_supported() accepts.
struct ConvLimbGroup {
  ConvArgs p[3];        // problems with the same n, T and column count (different taps / dilations / tensors)
  int nprob;
  const int* tiles;     // filled by launch_conv_limb: [items] {problem, m tile, n tile, K slice | slices << 8 | split-tile index << 16}
  const int* assign;    // [grid][assign_per] item indices per block, -1 terminated
  int assign_per;
  int wr_max;           // window rows of the largest problem's tile
  // split-K tail (a single problem whose tile count is not a multiple of the CU count - ups.1: 320 tiles on 256 CUs): the last
  // tiles % CUs tiles are cut into K slices over their channel blocks; partial tiles meet in `slab` ([split tile][slice][TM x TN]),
  // one ticket per (split tile, matrix wave) in `counters` (zero before and after every launch); nullptr: no split
  float* slab; int* counters;
  long long slab_floats; int max_counters;
};
bool conv_limb_supported(const ConvArgs& a);
int conv_limb_shape(const ConvArgs* p, int nprob, int num_cu, int plan_n = 0, bool tail_split = false, int forced = -1);      // tile shape for these problems, -1: none fits (plan_n: conv_limb.hip)
bool launch_conv_limb(const ConvLimbGroup& g, int shape, int num_cu, hipStream_t st);
int conv_limb_tail_slices(const ConvArgs& a, int shape, int num_cu);      // K slices of the split tail this launch would run with (1: none)
const char* conv_limb_name(int shape);

// One ResBlock1 unit (hifigan_causal.py:230-238) as ONE tile pass (resblock_fused.hip):
//   y = c2(leaky_relu(c1(leaky_relu(x)))) + x,  c1: k taps, dilation dil;  c2: k taps, dilation 1, both causal.
struct RBProb {
  const float* w1; const float* w2;   // fragment-major: [C/16 column tiles][k + 1 taps (last zero)][C/16 K groups][64 lanes][4]
  const float* b1; const float* b2;   // [C]
  const unsigned short* w1l; const unsigned short* w2l;   // the same weights as bf16 limbs (resblock_limb.hip):
                                      // [C/16 column tiles][k + 1 taps (last zero)][C/32 K blocks][3 limbs][64 lanes][8]; null: not packed
  TRef x;                             // raw input (c1 operand after LeakyReLU, residual operand as it is)
  TRef y;                             // raw output
  int k, dil;
};
struct RBArgs {
  RBProb p[3];                        // the branches of a stage at one dilation index (inputs / outputs share their ring geometry's mode and rate)
  const int* slots; const int* pos;
  const int* tiles;                   // filled by launch_resblock_fused: [ntiles] {branch, slot index, first row, 0}, most expensive first
                                      // (merge: (slot, row tile)-major, branches 0 .. nprob-1 adjacent)
  int ntiles;
  int* sched;                         // work-queue state owned by the caller: 2 ints, zero before the first launch (re-armed by the kernel);
                                      // one per stream that may have a fused launch in flight
  int nprob, n, T;                    // branches, slots in this batch, output rows per slot
  int tiles_per_slot;
  int order[3];                       // the branches by descending k (stable): the order of the separate-branch tile list (filled by the launcher)
  float slope;
  // merge = 1 (last dilation of a stage, enough row tiles to fill the chip): a workgroup runs the nprob branches of one
  // (slot, row tile) one after the other and stores only leaky_relu(mean of the branch outputs) to `ymean` - the sum
  // (v0 + v1) + v2, the division and the activation are mean_act_kernel's, operation for operation, so the result does
  // not depend on whether a launch was merged; the branches' own outputs (p[].y) are not written.
  int merge;
  TRef ymean;
  unsigned long long* dbg;            // developer builds only (tools/rb_bench -DRB_ABLATE=4): cycle stamps per block
};
bool resblock_fused_supported(int C, int kmax, int span_max);
int resblock_fused_rows(int C, int T, int n, int ksum, int kmax, int num_cu);   // output rows per tile to launch with
bool launch_resblock_fused(const RBArgs& a, int C, int rows, int num_cu, hipStream_t st);
bool resblock_fused_can_merge(int C, int rows);   // a merged-branch build exists for this geometry
const char* resblock_fused_name(int C, int rows, bool merge = false);
const int* resblock_tiles(const RBArgs& a, int ro, int* total_out);      // the cached device tile list of a launch shape (resblock_fused.hip)
// The same tile pass with every fp32 product as six bf16 limb products on the bf16 MFMA (resblock_limb.hip): same arguments
// (RBProb::w1l / w2l), half as tall tiles.
bool resblock_limb_supported(int C, int kmax, int span_max);      // (and at most 256 slots per launch: launch_resblock_limb refuses more)
constexpr int kResblockLimbMaxSlots = 256;
int resblock_limb_rows(int C, int span_max);
bool launch_resblock_limb(const RBArgs& a, int C, int rows, int num_cu, hipStream_t st);
bool resblock_limb_can_merge(int C, int rows);
const char* resblock_limb_name(int C, int rows, bool merge = false);


// One ResBlock1 unit per branch for the wide first stage (C = 256, <= 32 rows per stream and step), a PAIR of workgroups per
// (branch, stream) tile: c1 split over output columns, c2 over input channels, partial sums exchanged at the end of the tile;
// the k-1 rows of xt in front of a tile come from a per-unit history ring (resblock_pair.hip).
struct RPProb {
  const float* w1; const float* w2;   // fragment-major like RBProb: [16 column tiles][k + 1 taps][16 K groups][64 lanes][4]
  const float* b1; const float* b2;   // [256]
  TRef x, y;                          // raw input / raw output
  TRef xh;                            // history of leaky_relu(c1 + b1): a ring with >= k - 1 rows of history, same rate as x
  int k, dil;
};
struct RPArgs {
  RPProb p[3];
  const int* slots; const int* pos;
  const int* tiles; int ntiles;       // filled by launch_resblock_pair
  int* sched;                         // queue state, 2 ints, zero before the first launch (re-armed by the kernel)
  float* xb;                          // exchange buffers, resblock_pair_xb_floats()
  unsigned* xflag; unsigned* mbox; unsigned* xcount;   // [pairs][8] flags, [pairs][4] tile mailboxes, [pairs][2] tile counts: zero at creation
  int nprob, n, T;                    // branches, slots, rows per slot (<= 32)
  float slope;
  unsigned* guard;                    // SpinGuard block of the stream-set (nullptr: unbounded waits)
  int fault;                          // test hook (conan_streams_test_fault): member 1 never posts its partial sums' flags
};
bool resblock_pair_supported(int C, int kmax, int span_max, int T);
size_t resblock_pair_xb_floats(int num_cu);
bool launch_resblock_pair(const RPArgs& a, int num_cu, hipStream_t st);
const char* resblock_pair_name(int T);

// Frame-rate conv / linear of the decoder step with an optional LayerNorm in front (rowconv.hip).
struct RowConvArgs {
  TRef x;               // input rows; with ln: the raw rows of THIS step (earlier rows come from `hist`)
  TRef hist;            // ln only: the layer's ring of normalised rows (read for t < 0, written for t >= 0)
  TRef y, res, m1, m2, lnmask, mask_out;
  const float* w;       // fragment-major: [Cout_pad/16][ktaps + 1][Cin/16][64 lanes][4]
  const float* bias;    // [Cout_pad] or nullptr
  const float* bvec; long long bvec_stride;   // per-slot broadcast vector or nullptr
  const float* gamma; const float* beta; float eps;
  const int* slots; const int* pos;
  int ln, has_res, has_m1, has_m2, has_lnmask, has_mask_out;
  int Cin, Cout, Cout_pad, ktaps, dil, T, n;
  int out_act; float out_scale, out_slope;
  int in_lrelu; float in_slope;   // LeakyReLU applied to the input window (HiFi-GAN resblock convs read raw tensors)
  int wr_max;           // filled by launch_rowconv: window rows of a tile
  int cw;               // filled by launch_rowconv: window channels (0: all of Cin; 1x1 layers wider than 512: chunks of 512)
  // ---- decoder megakernel only (decoder_mega.hip)
  // MOP_FFN: this conv (k = 1, Cout = hidden width, activation applied) is followed IN the workgroup by a second 1x1 conv
  // hidden -> Cout2 whose K range is the member's own hidden columns: member s of the group writes the partial sums
  // part[s][row][Cout2]; bias, residual and everything behind them are applied where the sum is consumed (xp.. below)
  const float* w2;      // second conv, fragment-major [Cout2_pad/16][2][Cout/16][64][4]
  float* part; long long part_stride;      // floats between the members' partial tensors, each [n*T][Cout2]
  int Cout2, Cout2_pad;
  // consumer side: the NEW rows of x are not a tensor but xparts partial tensors: x = ((p0 + p1 + ..) + xbias) + xres
  const float* xp; long long xp_stride; int xparts, xp_ld;
  const float* xbias; TRef xres; int has_xres;
  // ... and, for the decoder's fused conv blocks (LN -> k5 conv -> GELU -> 1x1 partial sums, conv.py:127-264), the rest of the
  // producer's epilogue: x = (((p0 + p1 + ..) + xbias) + xres) * xm1 * xm2; xstore: the summed rows are also stored to `x`
  // (row r by member r % members), where the NEXT fused operator's consumer finds them as its xres
  TRef xm1, xm2; int has_xm1, has_xm2, xstore;
  int hid_overlay;      // MOP_FFN with one 64-column hidden strip per member: the hidden tile overlays the window (read out by then)
};
bool rowconv_supported(int Cin, int ktaps, int dil, int T);
// plan_rows (all three): the row count the kernel variant is chosen for; 0 = the launch's own n * T (rowconv.hip)
struct RowConvTune { bool no_ksplit = false; int wide_min = 1024; };      // developer switches of the variant choice (plan_switches.h: RC_NOKSPLIT, RC_WIDE_MIN)
void launch_rowconv(const RowConvArgs& a, hipStream_t st, int plan_rows = 0, const RowConvTune& tune = {});
const char* rowconv_kernel_name(const RowConvArgs& a, int plan_rows = 0, const RowConvTune& tune = {});   // as rocprofv3 prints it
int rowconv_plan(RowConvArgs& a, int* nbx, int* nby, int* lds_floats, int plan_rows = 0, const RowConvTune& tune = {});   // tile geometry for the decoder megakernel

// LayerNorm over the channel axis of each row:
//   y[i][t][:] = (LN(x[i][t][:] (+ pre[i][t][:])) * gamma + beta) * m1 * m2 (+ post[i][t][:])
// optionally writing mask_out[i][t] = (sum_c |x| > 0).
struct LNArgs {
  TRef x, pre, y, post, m1, m2, mask_out;
  const float* gamma;
  const float* beta;
  const int* slots;
  const int* pos;
  const int* lens;
  int has_pre, has_post, has_m1, has_m2, has_mask_out;
  int T, n, C;
  float eps;
  // decoder megakernel only: x is the sum of xparts partial tensors (+ xbias, + xres) - see RowConvArgs
  const float* xp; long long xp_stride; int xparts, xp_ld;
  const float* xbias; TRef xres; int has_xres;
};
void launch_layernorm(const LNArgs& a, hipStream_t st);

// rows copy / gather helpers
struct CopyArgs {
  TRef x, y;
  const int* slots; const int* pos; const int* lens;
  int T, n, C;
};
void launch_copy_rows(const CopyArgs& a, hipStream_t st);

struct EmbedArgs {       // y[i][t][:] = table[idx[i][t]][:]
  TRef y;
  const float* table; const int* idx;
  const int* slots; const int* pos;
  int T, n, C, vocab;
};
void launch_embed(const EmbedArgs& a, hipStream_t st);

// Emformer attention for one layer (torchaudio _EmformerAttention.infer):
// queries = R+U tokens (+ the summary token when M > 0); keys = valid memory entries (min(M, ceil(past/seg))) | rc(R) |
// cached left context (min(LC, past)) | utt(U); the summary query does not see the memory columns; then the U new
// utterance keys/values are appended to the per-slot rings.
struct EmfAttnArgs {
  const float* q;      // [n][R+U(+1)][D]  (emb_to_query output, unscaled; last row = summary query when M > 0)
  const float* kv;     // [n][M+R+U][2D]   (emb_to_key_value output; rows [0,M) = memory bank entries, right-aligned)
  float* out;          // [n][R+U(+1)][D]
  float* kring; float* vring;   // [slot][LR][D]
  long long ring_slot_stride;
  const int* slots; const int* past;   // past[slot]
  int n, R, U, D, H, LC, lmask;
  float scaling;
  int M, seg;          // memory bank size (0: none) and segment length
};
void launch_emf_attn(const EmfAttnArgs& a, hipStream_t st);

// Memory-bank bookkeeping of one Emformer layer (torchaudio _EmformerLayer._unpack_state / _pack_state, memory_op):
//   ln[i][M+R+U]   = mean over the U utterance rows of ln (the summary token)
//   ln[i][0..M)    = the bank's last min(M, ceil(past/seg)) entries, right-aligned, zeros before them
//   bank[slot]    <- append mems_in[i]   (entry of segment number ceil(past/seg); ring of MB >= M+1 rows)
struct EmfMemArgs {
  float* ln;            // [n][M+R+U+1][D]
  float* bank;          // [slot][MB][D]
  const float* mems_in; // [n][D]
  const int* slots; const int* past;
  int n, R, U, D, M, MB, seg;
};
void launch_emf_mem_prep(const EmfMemArgs& a, hipStream_t st);
// out[i][:] = mean over rows [row0, row0+U) of x[i] ([n][rows][D])
void launch_emf_seg_mean(const float* x, float* out, int n, int rows, int row0, int U, int D, hipStream_t st);
// out[i][:] = tanh_on_mem ? tanh(x[i][row][:]) : clamp(x[i][row][:], -10, 10)
void launch_emf_mem_out(const float* x, float* out, int n, int rows, int row, int D, int tanh_on_mem, hipStream_t st);

// Whole streaming Emformer step in one launch (emformer_fused.hip): all layers + projection + arg-max.
constexpr int EMF_MAX_LAYERS = 12;
struct EmfLayerW {
  // fragment-major weights (ctx.hip finalize_emformer): 1 KiB per (16-column tile, 16-row k-group) MFMA B operand
  const float *wqkv, *wo, *w1, *w2;
  // [bq D | bkv 2D | bo D | b2 D | ln_in g,b | ln_ff g,b | ln_out g,b | b1 F]: one contiguous block per layer
  const float* params;
};
struct EmfFusedArgs {
  EmfLayerW layers[EMF_MAX_LAYERS];
  float* kring[EMF_MAX_LAYERS]; float* vring[EMF_MAX_LAYERS];          // [slot][LR][D]
  long long ring_slot_stride;
  const float* chunk;      // [n][U+R][D]  (utterance rows first, then the right context)
  float* out;              // optional [n][U][D]
  float* logits;           // optional [n][U][K]
  int* codes;              // optional [n][U]
  const float* wp; const float* bp;    // output projection, fragment-major (nullptr when output_dim == input_dim)
  const int* slots; int* past;         // past[slot] is advanced by U at the end of the launch
  int n, L, R, U, D, H, LC, lmask, F, K;
#ifdef EF_STAMPS
  unsigned long long* dbg;
#endif
  unsigned magic_per_g;   // ceil(2^32 / (max(LC,1) * D/4)): exact e / per_g for the prefetch units
  float scaling;
  // cluster mode (cs = 2, 4, 8): cs workgroups share one group of streams, each runs 1/cs of the feed-forward hidden
  // units and the partial sums meet in `xch` once per layer.  Workspace sizes: emformer_cluster_ws().
  int cs;
  float* xch;             // [cluster][2][EMF_MAX_CHUNKS][16][D] the feed-forward's per-chunk partial sums (layer parity double buffer)
  unsigned* xflag;        // [cluster][EMF_MAX_LAYERS][EMF_MAX_CLUSTER] "partial of this launch is written" (= epoch + 1)
  unsigned* xepoch;       // [cluster] launches this cluster has taken part in
  int fenced;             // 1: release / acquire fences around the exchange as well (CONAN_FENCED=1 cross-check)
  unsigned* guard;        // SpinGuard block of the stream-set (nullptr: unbounded waits)
  unsigned fault;         // test hook (conan_streams_test_fault): the cluster waits for a flag value nobody writes
  // memory bank (max_memory_size = M > 0): per layer the PROJECTED key / value rows of the last memory inputs, rings of MB >= M + 1
  // (power of two) entries per slot; entry of segment number j in row j % MB
  int M, MB, tanh_on_mem;
  float* bank_k[EMF_MAX_LAYERS]; float* bank_v[EMF_MAX_LAYERS];
  long long bank_slot_stride;
};
constexpr int EMF_MAX_CLUSTER = 8;
constexpr int EMF_MAX_CHUNKS = 16;      // hidden chunks of 256 columns per layer (ffn_dim <= 4096)
// floats of xch / words of xflag+xepoch for up to `max_groups` stream groups
inline size_t emformer_cluster_xch_floats(int max_groups, int D) { return (size_t)max_groups * 2 * EMF_MAX_CHUNKS * 16 * D; }
inline size_t emformer_cluster_flag_words(int max_groups) { return (size_t)max_groups * (EMF_MAX_LAYERS * EMF_MAX_CLUSTER + 1); }
int emformer_fused_streams_per_block(const EmfFusedArgs& a);
bool emformer_fused_supported(const EmfFusedArgs& a);
void launch_emformer_fused(const EmfFusedArgs& a, hipStream_t st);

// Cross attention of the prosody aligner (nn.MultiheadAttention, 2 heads) against cached K/V.
struct XAttnArgs {
  TRef q;              // [i][t][E]   already scaled by 1/sqrt(dh)
  TRef out;            // [i][t][E]
  const float* kv;     // [slot][S_max][2E]  (K | V)
  long long kv_slot_stride;
  const float* kmask;  // [slot][S_max] 0 or -inf
  const int* slen;     // [slot]
  float* attn_avg;     // optional [i][t][S_max] head-averaged weights
  const int* slots; const int* pos;
  int T, n, E, H, S_max;
};
void launch_xattn(const XAttnArgs& a, hipStream_t st);

// A slot's entry of the pitch-control table (include/conan_hip.h, conan_pitch_cfg, as the kernels read it): shift_oct is the host's
// (float)((double)shift_semitones / 12.0); a disabled slot's entry is all zero (thr = 0: the model's own threshold).
// follow (conan_streams_set_pitch_follow): 1 = v / uv of the slot come from the step's tracked contour where the step has one (f0.hip).
struct PitchSlot { int enabled; float shift_oct, range, pivot, thr; int follow; };
static_assert(sizeof(PitchSlot) == 24, "24 bytes per slot");
// uv/f0 head: LN(128) -> Linear(128->2) -> uv/f0 -> pitch control -> coarse bin -> decoder_inp = pitch_inp + pitch_embed[bin]
struct PitchHeadArgs {
  TRef h;              // [i][t][Cp]
  TRef pitch_inp;      // [i][t][E]
  TRef dec_inp;        // [i][t][E]
  const float* gamma; const float* beta; const float* w; const float* b;   // w [2][Cp]
  const float* pitch_embed;     // [300][E]
  const int* codes;             // [n][T]
  float* uv_pred; float* f0; int* bins;   // optional taps, [n][T][2], [n][T], [n][T]
  const int* slots; const int* pos;
  int T, n, Cp, E, silent_token;
  int trk_ld;                   // row stride of the tracked contour (the segment)
  const PitchSlot* ptab;        // [max_slots] per-slot pitch control, indexed by slot (conan_streams_set_pitch); never null
  const float* f0_in; const float* uv_in;   // optional caller contour [n][T] (log2 Hz; > 0: unvoiced), conan_decoder_step_pitch
  // optional tracked contour of a wav-in step (source-pitch following, f0.hip): library staging [n][trk_ld], row i = the step's row i;
  // read by the rows whose slot follows (PitchSlot::follow) in a step without a caller contour
  const float* trk_f0; const float* trk_uv;
};
void launch_pitch_head(const PitchHeadArgs& a, hipStream_t st);
// table[rows[i].slot] = rows[i].v for i < n (conan_streams_set_pitch, snapshot import); slots checked by the host
struct PitchRow { int slot; PitchSlot v; int pad_; };
static_assert(sizeof(PitchRow) == 32, "uploaded as 8 ints");
void launch_pitch_table(PitchSlot* table, const PitchRow* rows, int n, hipStream_t st);

// Source-pitch tracker (f0.hip; include/conan_hip.h, conan_f0_cfg): one workgroup per (row, frame) job.  A row reads `src` at
// src_off + (s & mask) for sample s of its signal (mask = -1: a plain row; LA - 1: a slot's audio ring), samples outside [0, valid) are
// zero; its frames f_first .. f_first + nframes - 1 are jobs job0 .. and go to out_f0 / out_uv [out_off + j].
struct F0Row { long long src_off, valid; double thr, gate; int mask, f_first, nframes, job0, out_off, tmin, tmax, pad_; };
static_assert(sizeof(F0Row) == 64, "uploaded as 16 ints");
struct F0Args {
  const float* src; float* out_f0; float* out_uv;
  const F0Row* tab; int rows;      // tab == nullptr: `rows` rows shaped like `uni`, row r at src_off * r, job0 = out_off = nframes * r
  F0Row uni;
  int jobs, n_fft, hop; double sr;
};
constexpr int kF0MaxFft = 2048;
void launch_f0(const F0Args& a, hipStream_t st);

// Register matching (register.hip; include/conan_hip.h, conan_register_cfg): one workgroup per row.  A row reads its nframes frames at
// f0 / uv [in_off + j] and starts from state[slot] (reseed = 0 and slot >= 0) or from its seed; it writes the matched values to
// out[out_off + j] (out_off < 0: none), the state after the row to state[slot] (slot >= 0) and to state_out[state_row] (state_row >= 0).
struct RegRow { long long seed_n, seed_S, in_off, out_off; int nframes, slot, reseed, state_row; float target, max_shift; int pad_[2]; };
static_assert(sizeof(RegRow) == 64, "uploaded as 16 ints");
struct RegArgs {
  const float* f0; const float* uv; float* out;
  long long* state;          // [max_slots][2] = (n, S), indexed by slot; may be null when no row names a slot
  long long* state_out;      // [rows][2]; may be null when no row has a state_row
  const RegRow* tab; int rows;
};
constexpr int kRegThreads = 256;
void launch_f0_register(const RegArgs& a, hipStream_t st);

// Source activity (activity.hip; include/conan_hip.h, conan_activity_cfg): one workgroup per row.  A row reads `src` at
// src_off + (s & mask) for sample s of its signal (mask = -1: a plain row; LA - 1: a slot's audio ring), samples outside [0, valid) are
// zero.  It runs the detector over its frames f_first .. f_first + nframes - 1 from state[slot] (reseed = 0 and slot >= 0) or from its
// seed, writes flags to act[out_off + j], levels to lvl[lvl_off + j] and - start_lvl = 1 - the level before the row's first frame to
// lvl[lvl_off - 1], powers to power[out_off + j] (where the launch has a power buffer), and the state after the row to state[slot]
// (slot >= 0) and state_out[state_row] (state_row >= 0).  mode = 0: a row of a slot without the feature, which shares the table so
// that the gate finds row i of a vocoder step at entry i: the detector leaves it alone and the gate skips it; mode 2: gated.
struct ActState { int active, hang, level, reserved; double floor; long long frames, active_frames; };
static_assert(sizeof(ActState) == 40, "conan_activity_state");
struct ActRow {
  long long src_off, valid, out_off, lvl_off;
  double open_abs, close_abs, open_ratio, close_ratio, rise_active, rise_idle, floor_min;
  ActState seed;
  int mask, f_first, nframes, slot, reseed, state_row, mode, start_lvl;
  int hold, up_step, down_step, closed_level;
};
static_assert(sizeof(ActRow) == 176, "uploaded as 44 ints");
struct ActArgs {
  const float* src; int* act; int* lvl; double* power;      // power may be null
  ActState* state;          // [max_slots], indexed by slot; may be null when no row names a slot
  ActState* state_out;      // [rows]; may be null when no row has a state_row
  const ActRow* tab; int rows, n_fft, hop;
  int long_rows;            // 1: rows of many frames (a whole signal): workgroups of kActThreads; 0: of kActStreamThreads
};
constexpr int kActThreads = 1024, kActStreamThreads = 256, kActFull = 1 << 20;
void launch_activity(const ActArgs& a, hipStream_t st);
// The gate: row i of the launch is x + i * ld -> y + i * ld_y (y may equal x), `samples` samples; its levels are lvl[i * lvl_ld + f] after
// frame f, and before frame 0 start (start_in_lvl = 0) or lvl[i * lvl_ld - 1] (start_in_lvl = 1: the detector's staging rows).
// tab != nullptr: row i is gated only where tab[i].mode == 2, every other row is skipped (not multiplied by 1).
struct ActGateArgs {
  const float* x; float* y; const int* lvl; const ActRow* tab;
  long long ld, ld_y, lvl_ld, samples;
  int n, hop, start, start_in_lvl;
};
constexpr int kActGateThreads = 256;
void launch_activity_gate(const ActGateArgs& a, hipStream_t st);

// Source bypass (bypass.hip; include/conan_hip.h, conan_bypass_cfg).  bypass_stage_kernel: one workgroup per row.  A row with mode 1
// runs the slew over its nframes <= seg frames from state[slot] (reseed = 0 and slot >= 0) or from its seed, writes the wet and
// effective dry levels to wet_lvl / dry_lvl [row][seg + 1] (word 0: the level before the chunk), the state after the row to
// state[slot] (slot >= 0) and state_out[state_row] (state_row >= 0), and copies nframes * hop samples - sample s_first + j of the
// slot's signal from src[src_off + ((s_first + j) & mask)], zero at and beyond `valid` - to dry[row][seg * hop].  fill = 0: the
// effective dry level of a frame is the dry level; 1: it is scaled by the closed part of gate_lvl[row][1 + f] (the activity staging of
// the same call, whose rows are in the same order); 2: the slot fills but has no gate, which counts as open - the effective level is
// 0.  mode = 0: a row of a slot without the feature, which holds its
// place in the table so that the mix finds row i of a vocoder step at entry i.
struct BypState { int wet, dry, dry_eff, reserved; };
static_assert(sizeof(BypState) == 16, "conan_bypass_state");
struct BypRow {
  long long src_off, valid, s_first;
  BypState seed;
  int mask, nframes, slot, reseed, state_row, mode;
  int wet_target, dry_target, step, fill;
};
static_assert(sizeof(BypRow) == 80, "uploaded as 20 ints");
struct BypStageArgs {
  const float* src; float* dry; int* wet_lvl; int* dry_lvl;
  const int* gate_lvl;      // [rows][seg + 1]; null when no row has fill = 1
  BypState* state;          // [max_slots], indexed by slot; may be null when no row names a slot
  BypState* state_out;      // [rows]; may be null when no row has a state_row
  const BypRow* tab; int rows, seg, hop;
};
constexpr int kBypStageThreads = 256;
void launch_bypass_stage(const BypStageArgs& a, hipStream_t st);
// The mix: row i of the launch is wet + i * wet_ld and dry + i * dry_ld -> out + i * out_ld (out may equal wet), `samples` samples; its
// levels are wet_lvl / dry_lvl [i * lvl_ld + f] after frame f, and before frame 0 start_wet / start_dry (start_in_lvl = 0) or the
// words at [i * lvl_ld - 1] (start_in_lvl = 1: the stage kernel's rows).  tab != nullptr: rows with tab[i].mode == 0 are skipped.
struct BypMixArgs {
  const float* wet; const float* dry; float* out; const int* wet_lvl; const int* dry_lvl; const BypRow* tab;
  long long wet_ld, dry_ld, out_ld, lvl_ld, samples;
  int n, hop, start_wet, start_dry, start_in_lvl;
};
constexpr int kBypMixThreads = 256;
void launch_bypass_mix(const BypMixArgs& a, hipStream_t st);

// Comfort noise (comfort.hip; include/conan_hip.h, conan_comfort_cfg).  comfort_track_kernel: one thread per row.  A row runs the
// tracker over its nframes frames - the detector's flags act[in_off + f] and, in follow mode, powers power[in_off + f] - from
// state[slot] (reseed = 0 and slot >= 0) or from its seed, writes the frame-end levels to lvl[lvl_off + f] and - start_lvl = 1 - the
// level before the row's first frame to lvl[lvl_off - 1], and the state after the row to state[slot] (slot >= 0) and
// state_out[state_row] (state_row >= 0).  mode = 0: a row of a slot without the feature (or without a detector), which holds its
// place in the table so that the fill finds row i of a vocoder step at entry i.  fill = 1: the slot's output is gated (activity
// mode 2) and the vocoder step fills the row; any other row is skipped there.  pos0: the utterance sample index of the row's first
// sample in the fill (the front-end's frame position * hop).
struct CmfState { int level, reserved; long long idle_frames; };
static_assert(sizeof(CmfState) == 16, "conan_comfort_state");
struct CmfRow {
  unsigned long long seed;
  long long pos0, in_off, lvl_off;
  CmfState seed_state;
  int nframes, slot, reseed, state_row, mode, start_lvl;
  int level, offset, l_min, l_max, up_step, down_step;
  int colour, fill;
  float norm;
  int pad_;
};
static_assert(sizeof(CmfRow) == 112, "uploaded as 28 ints");
struct CmfTrackArgs {
  const int* act; const double* power;      // power may be null when no row follows
  int* lvl;
  CmfState* state;          // [max_slots], indexed by slot; may be null when no row names a slot
  CmfState* state_out;      // [rows]; may be null when no row has a state_row
  const CmfRow* tab; int rows;
};
constexpr int kCmfTrackThreads = 64;
void launch_comfort_track(const CmfTrackArgs& a, hipStream_t st);
// The fill: row i of the launch is x + i * ld -> y + i * ld_y (y may equal x), `samples` samples, sample s being sample tab[i].pos0 + s
// of the white source; its gate levels are gate_lvl[i * lvl_ld + f] after frame f and before frame 0 start_gate (start_in_lvl = 0) or
// gate_lvl[i * lvl_ld - 1] (start_in_lvl = 1: the detector's staging rows); its comfort levels cmf_lvl[i * lvl_ld + f].  Rows with
// tab[i].mode == 0 or fill != 1 are skipped and keep their bits.
struct CmfFillArgs {
  const float* x; float* y; const int* gate_lvl; const int* cmf_lvl; const CmfRow* tab;
  long long ld, ld_y, lvl_ld, samples;
  int n, hop, start_gate, start_in_lvl;
};
constexpr int kCmfFillThreads = 256, kCmfFillPer = 8;
void launch_comfort_fill(const CmfFillArgs& a, hipStream_t st);

// Input loss concealment (conceal.hip; include/conan_hip.h, conan_conceal_cfg).  conceal_kernel: one workgroup per table row, which
// repairs `samples` samples of row `row` of the caller's buffer (wav + row * wav_ld dwords, in format fmt) in place from the flags
// lost[row * lost_ld + m], packet m = samples [m * packet, (m + 1) * packet) of the row.  The state - header, template, the last
// kConcHist values of the decoded repaired signal - is read from state[slot] (restart = 0 and slot >= 0) or starts as zeros, and is
// written back to state[slot] (slot >= 0).  A row is walked in tiles of kConcTile samples, so a whole signal (slot = -1,
// restart = 1) and a chunk take the same path.
constexpr int kConcMaxLag = 1024, kConcMaxWindow = 1024;      // CONAN_CONCEAL_MAX_LAG / _MAX_WINDOW
constexpr int kConcHist = kConcMaxLag + kConcMaxWindow;       // history values kept: the lag search reads the last window + lag_max of them
constexpr int kConcTile = 4096, kConcThreads = 1024;
struct ConcHead { int mode, p, j, reserved0; long long k, reserved1; };      // the first 32 bytes of a state record
static_assert(sizeof(ConcHead) == 32, "the header's record");
constexpr long long kConcStateBytes = (long long)sizeof(ConcHead) + (kConcMaxLag + kConcHist) * (long long)sizeof(float);
struct ConcRow {
  long long samples;
  int row, slot, restart, fmt;
  int packet, lag_min, lag_max, window, hold, fall, fade, pad_;
};
static_assert(sizeof(ConcRow) == 56, "uploaded as 14 ints");
struct ConcArgs {
  void* wav; long long wav_ld;            // the caller's rows, stride in dwords
  const int* lost; long long lost_ld;     // the caller's flags, stride in ints
  char* state;                            // [max_slots][kConcStateBytes]; may be null when no row names a slot
  const ConcRow* tab; int rows;
};
void launch_conceal(const ConcArgs& a, hipStream_t st);

// Echo cancellation (echo.hip; include/conan_hip.h, conan_echo_cfg).  echo_kernel: one workgroup of kEchoThreads lanes per table row,
// which cancels `samples` samples of row `row` of the caller's buffer (wav + row * wav_ld dwords, in format fmt) in place from the far
// row (far + row * far_ld dwords, same format).  The state - header, weights, the pending block's e, the last kEchoHist far samples -
// is read from state[slot] (restart = 0 and slot >= 0) or starts as the restart state, and is written back to state[slot] (slot >= 0).
// Every index the kernel forms comes from the row: taps, delay and phase (= pos mod 64, the pending block's fill) are the host's; of
// the record only values are read.  A row is walked in tiles of kEchoTile samples and, inside, block by block, so a whole signal
// (slot = -1, restart = 1) and a chunk take the same path.
constexpr int kEchoBlock = 64, kEchoMaxTaps = 2048, kEchoMaxDelay = 4096, kEchoMaxShift = 12;      // CONAN_ECHO_*
constexpr int kEchoHist = 6208;                                                                    // CONAN_ECHO_HISTORY
constexpr int kEchoTile = 2048, kEchoThreads = 256;
static_assert(kEchoHist >= kEchoMaxTaps + kEchoBlock - 1 + kEchoMaxDelay && kEchoHist % 4 == 0, "the window of the oldest tap of a block's first sample");
struct EchoHead { long long pos; int shift, hcnt; long long adapted, frozen, trips, D, E; int dmax, reserved; };      // the first 64 bytes of a record
static_assert(sizeof(EchoHead) == 64, "the header's record");
constexpr long long kEchoStateBytes = (long long)sizeof(EchoHead) + (kEchoMaxTaps + kEchoBlock) * 4ll + kEchoHist * 2ll;
struct EchoRow {
  long long samples, pos, reg, far_min;      // pos: the slot's position at the row's first sample
  int row, slot, restart, fmt;
  int taps, delay, phase, mu_shift;
  int dt_num, dt_den, hang, pad_;
};
static_assert(sizeof(EchoRow) == 80, "uploaded as 20 ints");
struct EchoArgs {
  void* wav; long long wav_ld;              // the caller's rows, stride in dwords
  const void* far; long long far_ld;        // the far rows, stride in dwords
  char* state;                              // [max_slots][kEchoStateBytes]; may be null when no row names a slot
  long long* stats;                         // [call rows][4] or null
  const EchoRow* tab; int rows;
};
void launch_echo(const EchoArgs& a, hipStream_t st);

// Echo delay (echo_delay.hip; include/conan_hip.h, conan_echo_delay_cfg).  echo_delay_kernel: one workgroup of kEdThreads lanes per
// table row, which reads `samples` samples of row `row` of the mic buffer (wav + row * wav_ld dwords, in format fmt) and of the far
// buffer and writes neither.  The state - header, A[kEdMaxLags], the far end's last ternary values - is read from state[slot]
// (restart = 0 and slot >= 0) or starts as the restart state, and is written back to state[slot] (slot >= 0).  Every index the kernel
// forms comes from the row: n_lags and phase (= pos mod kEdFrame) are the host's; of the record only values are read.  A row is
// walked in tiles of kEdTile samples and, inside, segment by segment up to the next frame end, so a whole signal (slot = -1,
// restart = 1) and a chunk take the same path.  track (may be null): [call rows] of track_ld int64, six per frame end of the row.
constexpr int kEdFrame = 1024, kEdMaxLags = 6144, kEdTile = 4096, kEdThreads = 256;      // CONAN_ECHO_DELAY_*
constexpr int kEdPerLane = kEdMaxLags / kEdThreads;
static_assert(kEdMaxLags == kEchoMaxDelay + kEchoMaxTaps && kEdMaxLags % kEdThreads == 0 && kEdTile % kEdThreads == 0, "lane i owns lags i + 256 k");
struct EdHead { long long pos; int est, age, cand, run; long long frames, last_pk, last_s; long long reserved[2]; };      // the first 64 bytes of a record
static_assert(sizeof(EdHead) == 64, "the header's record");
constexpr long long kEdStateBytes = (long long)sizeof(EdHead) + kEdMaxLags * 4ll + kEdMaxLags;
struct EdRow {
  long long samples, pos;      // pos: the slot's position at the row's first sample
  int row, slot, restart, fmt;
  int n_lags, phase, thr, leak;
  int ratio, min_peak, hold, tol;
};
static_assert(sizeof(EdRow) == 64, "uploaded as 16 ints");
struct EdArgs {
  const void* wav; long long wav_ld;        // the mic rows, stride in dwords
  const void* far; long long far_ld;        // the far rows, stride in dwords
  char* state;                              // [max_slots][kEdStateBytes]; may be null when no row names a slot
  long long* report;                        // [call rows][6] or null
  long long* track; long long track_ld;     // [call rows][track_ld] or null
  const EdRow* tab; int rows;
};
void launch_echo_delay(const EdArgs& a, hipStream_t st);

// Input noise suppression (denoise.hip; include/conan_hip.h, conan_denoise_cfg): the spectral gate on log-mel frames of nm bins.  One
// workgroup of 64 * ceil(nm / 64) lanes per table row; lane b keeps the floor and the attenuation of bin b in registers across the
// row's frames.  DnState is the published conan_denoise_state; a record whose `bins` is not nm is the state before the first frame.
//   denoise_signal_kernel: row i of x [n][.][nm] (stride ld floats), nnew frames from frame 0, into y (may be x); the state starts
//     from seed[row] (seed given and reseed = 0) or before the first frame and goes to state_out[state_row] (state_row >= 0).
//   denoise_stream_kernel: the frames [f0, f0 + nnew) of slot's mel ring in place (frame f at f & (LM - 1)), from state[slot]
//     (reseed = 0) or before the first frame, written back to state[slot]; then chunk row r < rows of block `chunk` of fe_chunk <-
//     ring frame pos + min(r, real - 1).
//   Both read the record once, in front of a barrier, and write one behind it: seed may be state_out.  floor and att of a record are
//   read clamped to -2^20 .. 2^20 and 0 .. 2^20, the range the law keeps them in.
constexpr int kDnMaxBins = 256;
struct DnState { long long frames; int bins, reserved; int floor[kDnMaxBins], att[kDnMaxBins]; };
static_assert(sizeof(DnState) == 2064, "conan_denoise_state");
struct DnRow {
  int bias, knee, slope, depth, close_step, open_step, rise, fall_shift, floor_min, smooth;
  float out_floor;
  int slot, state_row, reseed;
  int row, f0, nnew, pos, rows, real, chunk, pad_;
};
static_assert(sizeof(DnRow) == 88, "uploaded as 22 ints");
struct DnSignalArgs {
  const float* x; float* y; long long ld;
  const DnState* seed; DnState* state_out;
  const DnRow* tab; int rows, nm;
};
struct DnStreamArgs {
  float* mring; float* chunk; DnState* state;
  const DnRow* tab; int rows, nm, LM, pad_;
};
void launch_denoise_signal(const DnSignalArgs& a, hipStream_t st);
void launch_denoise_stream(const DnStreamArgs& a, hipStream_t st);

// Silence trimming (trim.hip; include/conan_hip.h, conan_trim_cfg).  Row i has lens[i] samples at wav + i * ld and F = 1 + lens[i] / hop
// frames; its flags are act[i * act_ld + f] (any non-zero counts as 1).  The plan kernel (one workgroup per row) writes the row's two
// prefix arrays pa / pb [i * pre_ld + 0 .. F] (scratch: the prefixes of act and of m1), the kept-frame mask m2 to mask[i * mask_ld + f]
// (mask may be null), off[f] - or -1 for a dropped frame - to off[i * off_ld + f] and the row's out_len to out_len[i].  The gather
// kernel (grid: tiles of kTrimGatherFrames frames x rows) reads off / out_len and moves the kept frames' samples to out + i * out_ld,
// then zero-fills [out_len, lens[i]).
struct TrimArgs {
  const float* wav; float* out; const int* act; int* mask; long long* off; long long* out_len; int* pa; int* pb; const long long* lens;
  long long ld, out_ld, act_ld, mask_ld, off_ld, pre_ld;
  int n, hop, w, s, tiles, pad_;
};
constexpr int kTrimThreads = 256, kTrimGatherThreads = 256, kTrimGatherFrames = 16;
void launch_trim_plan(const TrimArgs& a, hipStream_t st);
void launch_trim_gather(const TrimArgs& a, hipStream_t st);

// y = leaky_relu((x0 + x1 + x2) / nsrc): the MRF mean of HifiGanGenerator.forward (hifigan_causal.py:324-331) with the
// following LeakyReLU, materialised once so that the consuming conv runs the single-source direct-to-LDS path.
struct MeanActArgs { TRef x[3]; TRef y; const int* slots; const int* pos; int nsrc, T, n, C; float slope; };
void launch_mean_act(const MeanActArgs& a, hipStream_t st);
// conv_post (CausalConv1d(C -> 1, k) + tanh, hifigan_causal.py:331-333) as a VALU dot-product kernel: N = 1 would
// waste 31/32 of an MFMA tile.  x[0] is the already activated input ring (nsrc = 1); w is [k][C]; optional pre-tanh tap.
// xmean.base != nullptr: x[0 .. nsrc) are the RAW outputs of the last stage's branches (nsrc may be 1: a single-branch
// vocoder still needs its LeakyReLU in front of conv_post) and the kernel forms leaky_relu(mean) itself (the same
// operations in the same order as mean_act_kernel), so the stage's own mean_act launch disappears; rows of earlier steps
// (the k - 1 rows of left context) come from `xmean`, the activated-mean ring, to which the kernel also appends the rows
// it formed - the ring stays valid whichever way a step produced it (merged fused launch, or here).
// adv_pos != nullptr: the last workgroup to finish advances the per-slot frame counters by adv_delta (the step's
// launch_advance folded in; adv_ticket is a zeroed int the kernel leaves zeroed).
struct ConvPostArgs { TRef x[3]; TRef xmean; int nsrc; float slope; const float* w; float bias; float* wav; float* pre; const int* slots; const int* pos; int T, n, C, k;
                      int* adv_pos; int adv_delta; int* adv_ticket; };
void launch_conv_post(const ConvPostArgs& a, hipStream_t st);

// The decoder step as ONE persistent launch (decoder_mega.hip): a list of row-wise operators (rowops.h) walked by every
// workgroup, tiles of an operator dealt round-robin over the grid, a grid barrier between dependent operators.
enum MegaOpType { MOP_RC111 = 0, MOP_RC114 = 1, MOP_ROWLIN = 2, MOP_LN = 3, MOP_XATTN = 4, MOP_PITCH = 5, MOP_EMBED = 6, MOP_COPY32 = 7, MOP_ADVANCE = 8, MOP_FFN = 9 };
struct MegaCopy { unsigned* dst; const unsigned* src; long long n; };          // n 32-bit words (plain accesses: inputs of the launch -> outputs read after it)
struct MegaAdvance { int* pos; const int* slots; int n, delta; };              // pos[slots[q]] += delta (the step's last operator)
struct MegaOp {
  int type, nbx, nby;
  int barrier;            // 1: the operators after this one read what it wrote - grid barrier behind it
  float f0, f1;           // pitch head: mel_min, mel_max - mel_min
  int pad_[2];
  union U { RowConvArgs rc; LNArgs ln; XAttnArgs xa; PitchHeadArgs ph; EmbedArgs em; MegaCopy cp; MegaAdvance adv; } u;
};
int decoder_mega_lds_floats(const MegaOp& op, int rc_lds_floats);
int decoder_mega_blocks_per_cu(int lds_bytes, bool wide_regs);
// prog: device copy of nops operators.  njobs 16-row tiles are dealt over `groups` groups of `group_size` workgroups; kw4: the
// step is one tile and its strips are 16 columns with the K loop split over a workgroup's waves.  gbar: one zero-initialised
// counter per group, 16 words apart; bar: the grid barrier's counter, counts for ever - bar_base is its value before this
// launch (the host adds groups * group_size per launch).
struct MegaLaunch {
  const MegaOp* prog; int nops, njobs, groups, group_size, kw4, lds_bytes;
  const int* slots; const int* pos; int n, T;
  unsigned* gbar; unsigned* bar; unsigned bar_base; unsigned long long* dbg;
  unsigned* guard;        // SpinGuard block of the stream-set (nullptr: unbounded waits)
  int wide_regs;          // 1: the 128-register build (bf16-limb stream-sets), 0: the 80-register build
  // xcd mode (a single row tile in the step): one workgroup per CU is launched, those on workgroup 0's XCD form the one group
  int xcd; unsigned* xs; unsigned xseq, xdec_base;
};
void launch_decoder_mega(const MegaLaunch& m, hipStream_t st);

struct ArgmaxArgs { const float* x; int* idx; int rows, C; };
void launch_argmax(const ArgmaxArgs& a, hipStream_t st);

void launch_advance(int* pos, const int* slots, int n, int delta, hipStream_t st);
void launch_fill_int(int* p, const int* slots, int n, int value, hipStream_t st);
void launch_copy_int_rows(int* dst, const int* src, int n, int T, int S, hipStream_t st);
void launch_profile_mark(hipStream_t st);
void launch_scatter_int(int* dst, const int* slots, const int* src, int n, hipStream_t st);
void launch_scatter_ids(int* dst, const int* slots, const int* src, const int* lens, int n, int S_max, int src_ld, hipStream_t st);   // dst[slot][s] = s < lens[i] ? src[i][s] : -1 (rows of dst S_max, of src src_ld ints)
void launch_gather_ids(int* dst, int* cnt, const int* src, const int* slen, const int* slots, int n, int S_max, hipStream_t st);
void launch_scatter_rows(float* dst, const float* src, const int* slots, int n, int C, hipStream_t st);   // dst[slots[i]][:] = src[i][:]
void launch_zero_slots(float* base, long long slot_stride, long long count, const int* slots, int n, hipStream_t st);
// streaming mel front-end (frontend.hip, conan_step_wav): the frames [f0, f0 + nnew) of each of the n slots plus the chunk rows
// row r <- frame pos + min(r, real - 1), r < rows (rows = 0: no chunk in this call)
constexpr int kMelStreamFrames = 4;     // frames per workgroup
struct MelStreamArgs {
  const float* wav;          // [n][m] this call's samples
  float* aring;              // [slot][LA] audio ring: sample s at s & (LA - 1)
  float* mring;              // [slot][LM][nm] mel ring: frame f at f & (LM - 1)
  float* chunk;              // [n][rows][nm]
  const int* slots;
  const float* win; const double2* tw; const float* fb; const int* lo; const int* hi;
  long long r_prev, total;   // samples received before this call; utterance length once final (-1 before)
  int m, n, f0, nnew, pos, rows, real;
  int LA, LM, nm, n_fft, hop, nb, cmag;
  float eps, vmin, vmax, mag_eps;
  int natural_log;           // 0: log10, 1: ln (as mel_log_kernel)
};
inline size_t mel_stream_lds_bytes(int n_fft, int cmag) { return (size_t)n_fft * kMelStreamFrames * 8 + (size_t)n_fft * 16 + (size_t)kMelStreamFrames * cmag * 4; }
void launch_mel_stream(const MelStreamArgs& a, hipStream_t st);        // nnew > 0: the new frames, the old chunk rows, the samples
void launch_mel_stream_copy(const MelStreamArgs& a, hipStream_t st);   // nnew = 0: old chunk rows from the mel ring, samples into the audio ring
// ragged streaming front-end (conan_step_wav_ragged): slots at different positions of their utterances.  The per-slot fields
// live in a device table of kRaggedWords ints per call row (uploaded through PinRing); the shared fields stay in the arguments.
enum RaggedField {
  kRgSlot, kRgRecvLo, kRgRecvHi, kRgTotalLo, kRgTotalHi,   // slot; samples received before this call; utterance length (-1: not final)
  kRgM, kRgF0, kRgNnew, kRgPos, kRgRows, kRgReal,          // samples of this call; frames [f0, f0 + nnew); chunk rows pos + min(r, real - 1)
  kRgChunk,                                                // destination chunk row block (rows = 0: no chunk)
  kRgJob,                                                  // prefix sum of nnew: this row's first frame job
  kRgGroup, kRgIndex, kRgEmit,                             // scatter: the emit group's first staging row, the row's index in it, frames emitted
  kRaggedWords = 16
};
struct MelRaggedArgs {
  const float* wav;          // [n][wstride] this call's samples, row i: tab[i].m used
  float* aring; float* mring; float* chunk;
  const int* tab;            // [n][kRaggedWords]
  const float* win; const double2* tw; const float* fb; const int* lo; const int* hi;
  int n, jobs, wstride;
  int LA, LM, nm, n_fft, hop, nb, cmag;
  float eps, vmin, vmax, mag_eps;
  int natural_log;
};
void launch_mel_ragged(const MelRaggedArgs& a, hipStream_t st);         // one launch per call (jobs may be 0: copy / append only)
// rows of the emit groups' staged outputs into call order: row i <- row kRgIndex of the group staged at row kRgGroup, its first kRgEmit frames
struct WavScatterArgs {
  const int* tab; int n, seg, nm, hop;
  const int* codes_src; const float* mel_src; const float* wav_src;     // staging: group-compact rows ([k][emit][.]) at group offsets
  int* codes; float* mel; float* wav;                                    // caller's [n][seg], [n][seg][nm], [n][seg * hop]; each may be null (wav: resample_out_kernel places the audio rows)
};
void launch_wav_scatter(const WavScatterArgs& a, hipStream_t st);

// ---- polyphase resampler (resample.hip): torchaudio's windowed sinc (include/conan_hip.h, conan_resample_cfg).  Output j = p + nph * q
// of a row is rs_dot over the inputs [first, first + cnt) with first = q * orig - w + klo[p]; a workgroup takes kRsTile outputs of one
// row and stages their input window in LDS.
constexpr int kRsTile = 256;
constexpr int kRsRing = 32768;        // streaming input history per slot (floats; input sample i at i & (kRsRing - 1))
constexpr int kRsMaxWindow = 16384;   // LDS floats of a tile's input window (a configuration that needs more is refused)
struct RsFilter {
  const float* taps;                  // [L][nph]: tap k' of phase p at k' * nph + p (zero past the phase's count)
  const int* ph;                      // [nph][2]: klo (first tap, relative to q * orig - w), cnt
  int orig, nph, w, L;
};
// Sample formats of the caller's rows (include/conan_hip.h, CONAN_SAMPLE_*): f32, s16, G.711 mu-law, G.711 A-law.  A row of a format
// other than f32 is packed from the row's first byte; row strides stay in 4-byte units, so every row starts on a dword.
constexpr int kFmtF32 = 0, kFmtS16 = 1, kFmtUlaw = 2, kFmtAlaw = 3;
constexpr int kRsCopy = 1, kRsFmtShift = 8;      // RsRow::mode: bit 0 = the row has no rate, bits 8.. = the format of the caller's row
// A drift row (conan_streams_set_input_drift / _output_drift; RsRow::mode bit 1, RsOutRow::L == kOrDriftL) reuses the rational fields:
// taps = the drift table (float2), ph = the step (its 64 bits in the pointer), out0 = the input index n of the call's first output,
// orig = that output's 32-bit fraction, w = W; output t of the call sits at (out0 << 32) + orig + t * step.
constexpr int kRsDrift = 2, kOrDriftL = -1;
constexpr int kOrDstBits = 24;                   // RsOutRow::dst: the row index in the low 24 bits, the format of the caller's row above
struct RsRow {                        // one call row of resample_stream_kernel (16 ints, uploaded through PinRing)
  long long in0, out0;                // input samples received before this call; model-rate samples handed over before it
  const float* taps; const int* ph;
  int slot, m, h, orig, nph, w, L, mode;   // m input samples this call, h outputs; mode: kRsCopy (no rate: h = m samples, decoded) | format << kRsFmtShift
};
static_assert(sizeof(RsRow) == 16 * sizeof(int), "RsRow is uploaded as 16 ints");
struct ResampleArgs { const float* x; float* y; long long samples, nout; RsFilter f; int win; };
void launch_resample(const ResampleArgs& a, int n, hipStream_t st);            // whole signals: x [n][samples] -> y [n][nout]
struct ResampleStreamArgs {
  const float* wav; long long wav_ld;   // this call's input, row r at r * wav_ld dwords in its slot's format (never null: a dummy when no row has samples)
  float* ring;                          // [max_slots][kRsRing]
  float* out; long long out_ld;         // model-rate rows for the front-end
  const RsRow* rows; int n, tiles, win;
};
void launch_resample_stream(const ResampleStreamArgs& a, hipStream_t st);
// Output side (conan_streams_set_output_rate): one call row of resample_out_kernel.  The roles of ring and row are the input side's:
// the slot's older model-rate samples come from its history ring, the vocoder step's m new ones from staging row r; outputs
// [out0, out0 + h) go to row `dst` of the caller's buffer.  taps == nullptr: the slot has no rate, its m samples are copied verbatim.
struct RsOutRow {
  long long in0, out0;                // model-rate samples produced before this step; output samples delivered before it
  const float* taps; const int* ph;
  int slot, m, h, orig, nph, w, L, dst;   // dst: row | format << kOrDstBits
};
static_assert(sizeof(RsOutRow) == 16 * sizeof(int), "RsOutRow is uploaded as 16 ints");
struct ResampleOutArgs {
  const float* wav; long long wav_ld;   // conv_post's model-rate rows (staging), row r at r * wav_ld (a flush: m = 0 everywhere, never null)
  float* ring; int ring_len;            // [max_slots][ring_len] (a power of two; model-rate sample i at i & (ring_len - 1))
  float* out; long long out_ld;         // the caller's wav_out_dev at the stride in force (dwords), each row in its slot's format
  const RsOutRow* rows; int n, tiles, win;
};
void launch_resample_out(const ResampleOutArgs& a, hipStream_t st);
// Drift resampler (conan_resample_drift; the law is include/conan_hip.h's): output j sits at the 32.32 fixed-point input position pos_j;
// its 2W taps are row p = frac >> 22 of a table of kDrPhases + 1 phases, interpolated towards row p + 1 by the low 22 bits.  The device
// table holds (T[p][k], T[p + 1][k] - T[p][k]) as one float2 at k * kDrPhases + p (phase-fastest).  A workgroup takes kRsTile outputs of
// one row; positions are monotone, so the tile's window is [n_first - W + 1, n_last + W].
constexpr int kDrPhases = 1024, kDrFracBits = 22;
constexpr int kDrMaxTaps = 512;       // 2W at most
constexpr int kDrMaxSeg = 32;         // segments of a whole-signal schedule (passed by value)
struct DrSchedule {                   // segment q: outputs [at[q], at[q + 1]) at pos[q] + (j - at[q]) * step[q]
  long long at[kDrMaxSeg];
  unsigned long long pos[kDrMaxSeg], step[kDrMaxSeg];
  int n;
};
struct ResampleDriftArgs {
  const float* x; float* y; long long samples, nout, y_ld;     // x [n][samples] -> y rows at y_ld floats
  const float2* tab; int W, win;                               // win: LDS floats of a tile's window (upper bound)
  DrSchedule s;
};
void launch_resample_drift(const ResampleDriftArgs& a, int n, hipStream_t st);
// Whole signals from one sample format to another through the float rule (conan_convert_samples): n rows of `samples`, strides in dwords.
struct ConvertSamplesArgs { const void* src; void* dst; long long src_ld, dst_ld, samples; int src_fmt, dst_fmt; };
void launch_convert_samples(const ConvertSamplesArgs& a, int n, hipStream_t st);

// ---- loudness meter and gain (loudness.hip): BS.1770 K-weighting and gating as include/conan_hip.h states them (conan_loudness_cfg).
// The K-weighting recursion is serial in time and linear, so a row is cut into segments of kLdSeg samples, one lane each: loud_state_kernel
// runs every segment from a zero state, loud_scan_kernel turns the segments' end states into their true start states
// (in[s + 1] = M in[s] + end[s], M = the transition matrix of one whole segment), loud_energy_kernel re-runs every segment from its start
// state and sums y^2 into the bins between consecutive block edges, loud_gate_kernel (one workgroup per row) sums the bins over the
// segments and the blocks over their bins, gates, and writes the row's gain, loud_apply_kernel scales.  All filter and energy arithmetic
// is f64; every sum has one order, fixed by the row alone.
// (kLdSeg = 128, the samples per segment, is level_plan.h's: the host planning shares it)
constexpr int kLdLanes = 64;                     // segments per workgroup of the state / energy passes: one wave
constexpr int kLdStride = kLdSeg + 1;            // LDS floats between two lanes' segments: lane l, step t reads bank (l + t) mod 32
constexpr int kLdTile = kLdSeg * kLdLanes;       // samples per workgroup
constexpr int kLdSlots = 4;                      // bins a segment can touch: at most 3 edges inside a segment (the host checks)
struct LdBiquad { double b0, b1, b2, a1, a2; };  // normalised by a0; direct form II transposed
struct LdRow {                                   // one call row (12 ints, uploaded with the edge and block tables)
  long long samples, seg0;                       // seg0: the row's first segment in the state / partial-sum arrays
  int nseg, edge0, nedges, blk0, nblocks, pad_[3];   // edge0 / blk0: the row's first entry in the edge / block tables
};
static_assert(sizeof(LdRow) == 12 * sizeof(int), "LdRow is uploaded as 12 ints");
struct LoudArgs {
  const float* x; long long x_ld;
  float* y; long long y_ld;                      // y may be null (measure only) or x
  const LdRow* rows; int n;
  const int* edges;                              // per row: the sorted distinct block starts and ends; bin b = [edge[b], edge[b + 1])
  const int* blocks;                             // per row and block: first bin, end bin
  double* state;                                 // [segments][4]: end states, then (scan) start states
  double* part;                                  // [segments][kLdSlots]: slot k = the sum over the segment's k-th bin
  float* peak;                                   // [segments]: max |x|
  double* binsum;                                // [edges]
  double* z; double* l;                          // [blocks]: block energies and loudnesses
  double* gain;                                  // [n][2]: gain, divisor (0: none)
  double* stats;                                 // caller's [n][4] or null
  LdBiquad shelf, hp;
  double M[16];                                  // row-major transition matrix of kLdSeg zero inputs
  double block_len;                              // T_g * fs
  double target; int peak_limit;
  int tiles;                                     // the longest row's workgroups in the state / energy passes
};
void launch_loud_measure(const LoudArgs& a, hipStream_t st);      // state, scan, energy, gate
void launch_loud_apply(const LoudArgs& a, long long longest, hipStream_t st);
// one step of the cascade (shelf, then high pass) on state s[4]; shared by the kernels and the host (M)
__host__ __device__ inline double ld_step(const LdBiquad& f, const LdBiquad& g, double* s, double x) {
  const double u = fma(f.b0, x, s[0]);
  s[0] = fma(-f.a1, u, fma(f.b1, x, s[1]));
  s[1] = fma(-f.a2, u, f.b2 * x);
  const double y = fma(g.b0, u, s[2]);
  s[2] = fma(-g.a1, y, fma(g.b1, u, s[3]));
  s[3] = fma(-g.a2, y, g.b2 * u);
  return y;
}

// ---- streaming leveller (level.hip): the causal BS.1770 leveller of include/conan_hip.h (conan_level_cfg).  A slot's stream is cut
// into the meter's kLdSeg-sample segments, aligned to position 0.  A chunk (the samples of one wav-in call, or one update interval
// of a whole signal; at most U = segment * hop samples) is appended to the slot's pending tail; the complete segments run one lane
// each - state pass from a zero state, scan from the slot's carried state, energy pass into per-segment bin partials - and are
// added, in ascending segment order, to the accumulators of the gating blocks they overlap; a block whose end the segments reached
// goes to the slot's ring of block energies.  At an update instant the window is gated by the whole workgroup and the new gain
// formed; then the ramps are applied.  One workgroup per row; lv_chunk (level.hip) is the one routine both kernels call.
constexpr int kLvThreads = 256;
constexpr int kLvSegs = 16;                      // LDS segments of a chunk: pending tail + U samples, U <= kLvMaxU
constexpr int kLvMaxU = (kLvSegs - 1) * kLdSeg;  // 1920
constexpr int kLvRingPad = 16;                   // blocks a ring holds beyond the window (blocks closed after the instant's J_k)
struct LvState {                                 // per slot / row, followed by z[zcap] and l[zcap] (doubles)
  double carry[4];                               // filter state at the start of the first incomplete segment
  double acc[kLvBlocks];                         // energies of the open blocks, block j at j % kLvBlocks
  double Gm, Gc, peak;                           // G_{k-1}, G_k of the latest instant k; max |x| of every sample so far
  double stat[4];                                // {L_k, G_k, P_k, J_k} of the latest instant
  float tail[kLdSeg];                            // pending raw samples: the first (position % kLdSeg) entries
  double pad_;                                   // (a multiple of 16 bytes: slot snapshots move the block in 16-byte cells)
};
static_assert(sizeof(LvState) == 20 * 8 + kLdSeg * 4 && sizeof(LvState) % 16 == 0, "LvState is sized in include/conan_hip.h");
constexpr size_t lv_state_bytes(int zcap) { return sizeof(LvState) + (size_t)zcap * 16; }
struct LvCfg {                                   // conan_level_cfg in the kernels' terms
  double target, boost, cut, g_init;
  int window, peak_limit, clip, pad_;
};
// (LvCall, one chunk's plan, and kLvBlocks are level_plan.h's)
struct LvRow {                                   // one call row of level_stream_kernel (uploaded through PinRing)
  LvCall c;
  LvCfg cfg;
  int slot, row, fresh, copy;                    // row: the call row whose samples these are; fresh: conan_streams_input_level before any sample;
                                                 // copy: an unlevelled row of a call whose staging the kernel writes - c.m samples, x -> y as they are
};
static_assert(sizeof(LvRow) % sizeof(int) == 0 && sizeof(LvCall) == 24 * sizeof(int), "LvRow is uploaded as ints");
struct LvFilter { LdBiquad shelf, hp; double M[16]; double block_len; int U; };
struct LevelStreamArgs {
  const float* x; long long x_ld;                // the call's model-rate rows
  float* y; long long y_ld;                      // the rows the front-end reads (may be x)
  char* state; long long state_stride; int zcap; // [max_slots] LvState + rings
  const LvRow* rows; int n;                      // the levelled rows with samples (and, where x is not y, the call's other rows as copy rows)
  LvFilter f;
};
void launch_level_stream(const LevelStreamArgs& a, hipStream_t st);
struct LevelStatsArgs { const char* state; long long state_stride; const LvRow* rows; int n; double* out; };
void launch_level_stats(const LevelStatsArgs& a, hipStream_t st);
struct LvSigRow { long long samples, blk0; int nblocks, pad_; };      // blk0: the row's first entry of the block table
struct LevelSignalArgs {
  const float* x; long long x_ld;
  float* y; long long y_ld;
  char* state; long long state_stride; int zcap; // [n] scratch states
  const LvSigRow* rows; int n;
  const int* blocks;                             // per row and block: lo, hi (every block that starts inside the row)
  double* trace; long long trace_ld;             // [n][trace_ld][2] or null
  LvCfg cfg;
  LvFilter f;
};
void launch_level_signal(const LevelSignalArgs& a, hipStream_t st);

// ---- output leveller (level_out.hip; conan_streams_set_output_level): the same law on the slot's own vocoder audio, split in two.
// A vocoder step's row is [u_k, u_k + m) with m <= U, and G_{k-1}, G_k depend only on samples before u_k: level_out_apply_kernel (on
// the step's critical path, shaped like bypass_mix_kernel) reads the two gains from the slot's LvState - or, at position 0, the cfg's
// initial gain - and writes the ramp in place, leaving the unlevelled samples in a staging row; level_out_meter_kernel (one
// workgroup per row, behind the step's last launch) runs lv_meter on the staged samples with the instant at the chunk's end
// (level::plan_end) and leaves {G_k, G_{k+1}} and the stats for the next step's apply.  Row i of a step is entry i of the table; on = 0:
// a row of a slot without the feature, which both kernels leave at once.  A slot's state is LvState, its two rings of zcap doubles,
// then prev[4]: the stats of the instant before the latest one (the reading after a whole chunk k is instant k's, not k + 1's).
struct OlRow {
  LvCall c;
  LvCfg cfg;
  int slot, on, prev, state_row;                 // prev / state_row: the stats query's (1: read prev[4]; fresh: c.pos0 == 0, c.m == 0)
};
static_assert(sizeof(OlRow) == 160, "OlRow is uploaded as 40 ints, and sized in include/conan_hip.h");
constexpr size_t ol_state_bytes(int zcap) { return lv_state_bytes(zcap) + 4 * sizeof(double); }
struct LevelOutApplyArgs {
  float* x; long long ld;                        // the step's rows, levelled in place
  float* stage; long long stage_ld;              // the unlevelled samples, for the meter
  const char* state; long long state_stride;
  const OlRow* tab; int n, samples, U;
};
constexpr int kOlApplyThreads = 256;
void launch_level_out_apply(const LevelOutApplyArgs& a, hipStream_t st);
struct LevelOutMeterArgs {
  const float* stage; long long stage_ld;
  char* state; long long state_stride; int zcap;
  const OlRow* tab; int n;
  LvFilter f;
};
void launch_level_out_meter(const LevelOutMeterArgs& a, hipStream_t st);
struct LevelOutStatsArgs { const char* state; long long state_stride; int zcap; const OlRow* tab; int n; double* out; };
void launch_level_out_stats(const LevelOutStatsArgs& a, hipStream_t st);

// ---- output watermark (watermark.hip; include/conan_hip.h, conan_watermark_cfg): a keyed +-1 chip sequence under a causal peak
// envelope, added to a slot's vocoder audio behind the comfort fill and in front of the output resampler, and its integer detector.
//   watermark_embed_kernel: one workgroup per table row, in place on row i of x (or into y); the row's state comes from state[slot]
//     (a step row), from seed[i] or from the row's own seed record, and goes back to state[slot] / state_out[state_row].  A row with
//     on = 0 holds a step row's place and returns at once.
//   watermark_corr_kernel: grid (offset tile, block, row): the pre-whitened window of block k in LDS, the chip correlation at
//     kWmCorrOffsets offsets in int32 (|R| < 2^31: conan_hip.h), the block weight, Rn -> the workspace [row][kmax][kWmBlk] (int32:
//     |Rn| < 2^12, because |R| is at most the window's sum of |d|, which is under 2^n_k).
//   watermark_peak_kernel: one workgroup per row: S[o] over the blocks in index order, the argmax (lowest index on ties), soft, the record.
constexpr int kWmChip = 4, kWmBlk = 2048, kWmSub = 64, kWmWord = 24, kWmChips = kWmBlk / kWmChip;
constexpr int kWmThreads = 256, kWmCorrOffsets = 512;
struct WmState { long long pos; float env; int reserved; };
static_assert(sizeof(WmState) == 16, "conan_watermark_state");
struct WmRow {
  unsigned long long key;
  WmState seed;                                  // what a restarting row starts from
  float gain, floor;
  unsigned word;                                 // bit b: block b of a word carries +1
  int on, reseed, slot;                          // slot -1: a whole-signal row
  int samples, state_row;                        // the row's length; state_row: the entry of state_out (-1: none)
};
static_assert(sizeof(WmRow) == 56, "uploaded as 14 ints");
struct WmEmbedArgs {
  const float* x; float* y; long long ld, ld_y;
  WmState* state;                                // [max_slots], or null
  const WmState* seed; WmState* state_out;       // per row of a whole-signal call, each may be null
  const WmRow* tab; int n, pad_;
};
void launch_watermark_embed(const WmEmbedArgs& a, hipStream_t st);
struct WmHit { int offset, blocks; long long peak; };
static_assert(sizeof(WmHit) == 16, "conan_watermark_hit");
struct WmDetRow { long long samples; int blocks, pad_; };
struct WmDetectArgs {
  const void* x; long long ld;                   // rows of `fmt` samples, ld dwords apart
  const WmDetRow* tab; int n, kmax, fmt, pad_;
  unsigned long long key;
  int* rn;                                       // workspace [n][kmax][kWmBlk]
  long long* score; long long* soft; long long soft_ld; WmHit* hit;
};
void launch_watermark_corr(const WmDetectArgs& a, hipStream_t st);
void launch_watermark_peak(const WmDetectArgs& a, hipStream_t st);

// ---- signalling tones (tone.hip; include/conan_hip.h, conan_tone_cfg): the DTMF detector of a row's source frames and the
// regeneration of a confirmed digit on the vocoder's audio.
//   tone_kernel: one workgroup per table row, the table W in LDS.  A row runs the law over its nframes frames - samples
//     src[src_off + (j & mask)] for j < valid, zero beyond, frame f_first + k (f_first < 0: the state's `frames`) - from state[slot]
//     (reseed = 0 and slot >= 0) or from its seed record (seed[row] of a whole-signal call where given), writes digit[out_off + k],
//     sound[lvl_off + k], level[lvl_off + k] and - start_lvl = 1 - the sound and level before the row's first frame to word
//     lvl_off - 1, and the state after the row to state[slot] / state_out[state_row].  mode = 0: a row of a slot without the feature,
//     which holds its place in the table so that the fill finds row i of a vocoder step at entry i.
//   tone_fill_kernel: row i of the launch is x + i * ld -> y + i * ld_y (y may equal x), `samples` samples, sample s being utterance
//     sample tab[i].pos0 + s; sound[i * lvl_ld + f] and level[i * lvl_ld + f] after frame f, and before frame 0 start_sound /
//     start_level (start_in_lvl = 0) or word -1 of the rows (start_in_lvl = 1: the detector's staging rows).  Rows with
//     tab[i].mode != 2 are skipped and keep their bits.
constexpr int kToneFreqs = 8, kToneSums = 2 * kToneFreqs + 1, kToneTile = 64, kToneFull = 1 << 20, kToneHopMax = 512;
struct ToneState { int cand, run, cur, miss, held, sound, level, reserved; long long events, frames; };
static_assert(sizeof(ToneState) == 48, "conan_tone_state");
struct ToneRow {
  long long src_off, valid, out_off, lvl_off, f_first, thr, pos0;
  ToneState seed;
  int mask, nframes, slot, reseed, state_row, mode, start_lvl;
  int twist_fwd, twist_rev, sel, share, on_frames, off_frames, min_frames, step;
  float gain;
};
static_assert(sizeof(ToneRow) == 168, "uploaded as 42 ints");
struct ToneArgs {
  const float* src; const short* table;
  int* digit; int* sound; int* level;
  ToneState* state;             // [max_slots], indexed by slot; may be null when no row names a slot
  const ToneState* seed;        // [rows] of a whole-signal call; may be null
  ToneState* state_out;         // [rows]; may be null when no row has a state_row
  const ToneRow* tab; int rows, hop, M;
  int long_rows;                // 1: rows of many frames (a whole signal): workgroups of kActThreads; 0: of kActStreamThreads
};
void launch_tone(const ToneArgs& a, hipStream_t st);
struct ToneFillArgs {
  const float* x; float* y; const int* sound; const int* level; const short* table; const ToneRow* tab;
  long long ld, ld_y, lvl_ld, samples;
  int n, hop, M, start_level, start_sound, start_in_lvl;
};
constexpr int kToneFillThreads = 256;
void launch_tone_fill(const ToneFillArgs& a, hipStream_t st);

// ---- equaliser (eq.hip, eq_dev.h; include/conan_hip.h, conan_eq_cfg): a cascade of up to kEqMaxSec biquad sections in f64, every
// product and sum rounded on its own.  A row's stream is cut into segments of kEqSeg samples from its origin; eq_chunk (eq_dev.h) is
// the one copy of the section passes: per section a zero-state pass over the chunk's complete segments (one lane each), a scan with
// the section's transition matrix from the carried state, and an output pass from every segment's start state that overwrites the
// LDS buffer for the next section.  An incomplete last segment is emitted from its start state and its inputs stay in the state's
// tail; the call that completes it runs it again and emits the new samples only.  One workgroup of kEqThreads per row.
constexpr int kEqSeg = 128;                      // samples per segment: a constant of the law (tests/eq_ref.py, SEG)
constexpr int kEqStride = kEqSeg + 1;            // LDS doubles between two lanes' segments: lane l, step t on bank pair (l + t) mod 32
constexpr int kEqSegs = 16;                      // LDS segments of a chunk: pending tail + the call's samples
constexpr int kEqMaxCall = (kEqSegs - 1) * kEqSeg;      // 1920: the samples one chunk takes
constexpr int kEqMaxSec = 4;
constexpr int kEqThreads = 256;
struct EqSec { double b0, b1, b2, a1, a2; double M[4]; };      // M: row-major 2x2 transition matrix of kEqSeg zero inputs
struct EqState {                                 // conan_eq_state
  long long origin, pos;                         // the grid's first sample; the samples filtered so far (both utterance indices)
  double carry[kEqMaxSec][2];                    // per section: the state at the start of the segment that holds `pos`
  float tail[kEqSeg];                            // that segment's inputs so far (behind the non-finite rule): (pos - origin) % kEqSeg entries, zeros behind
};
static_assert(sizeof(EqState) == 16 + 64 + 4 * kEqSeg && sizeof(EqState) % 16 == 0, "EqState is sized in include/conan_hip.h");
struct EqCall {                                  // one chunk's plan, built by the host (or by the whole-signal kernel's lane 0): never read from the state
  long long origin, pos0;                        // the chunk's first sample is utterance sample pos0
  int m, tail;                                   // new samples (0 .. kEqMaxCall); pending samples in front of them ((pos0 - origin) % kEqSeg)
  int fresh, nsec;                               // fresh: the carries count as zero (tail is 0 then)
};
struct EqSigRow { long long samples; };
struct EqSignalArgs {
  const float* x; long long x_ld;
  float* y; long long y_ld;                      // may be x
  const EqSigRow* rows; int n;
  const EqState* seed;                           // [n]; may be null: every row starts from zero at origin
  EqState* state_out;                            // [n]; may be null (then the rows' states live in `work`)
  EqState* work;                                 // [n] scratch states when state_out is null
  long long origin, pos0;                        // of every row
  int nsec;
  EqSec sec[kEqMaxSec];
};
void launch_eq_signal(const EqSignalArgs& a, hipStream_t st);
// The streaming forms (conan_streams_set_input_eq / _output_eq): a slot's state is state[slot] and its sections sec[slot * kEqMaxSec + k],
// both written by eq_set_kernel in stream order.
//   eq_stream_kernel: one workgroup per table row; row R filters R.c.m samples x + R.row * x_ld -> y + R.row * y_ld (y may be x) through
//     eq_chunk; on = 0: a row that holds its place; copy = 1: an unfiltered row on its way to the staging the front-end reads.
//   eq_set_kernel: one workgroup per listed slot.  mode 0: the zero state at c.pos0; mode 1, the live change: the c.tail pending samples
//     are closed with the OLD sections (the carries advance over them by the direct recursion through the c.nsec old sections), the
//     origin moves to c.pos0, the first `keep` sections keep their carries and the others start at zero; mode 2: seed row R.row
//     becomes the state.  Then the new sections - the kEqMaxSec EqSec records behind the table's n rows - become the slot's.
//   eq_state_kernel: row R -> out + R.row * ld bytes: the slot's record, or (mode 0: a slot about to restart) the zero record at c.pos0.
struct EqRow {                                   // uploaded through PinRing
  EqCall c;
  int slot, row, on, copy;
  int mode, keep, pad_[2];
};
static_assert(sizeof(EqRow) == 64 && sizeof(EqCall) == 32, "EqRow is uploaded as 16 ints");
constexpr int kEqSecRows = (int)((kEqMaxSec * sizeof(EqSec) + sizeof(EqRow) - 1) / sizeof(EqRow));      // table rows the setter's sections take
struct EqStreamArgs {
  const float* x; long long x_ld;
  float* y; long long y_ld;
  EqState* state; const EqSec* sec;
  const EqRow* rows; int n;
};
void launch_eq_stream(const EqStreamArgs& a, hipStream_t st);
struct EqSetArgs { EqState* state; EqSec* sec; const EqRow* rows; int n; const char* seed; long long seed_ld; };
void launch_eq_set(const EqSetArgs& a, hipStream_t st);
struct EqStateArgs { const EqState* state; const EqRow* rows; int n; char* out; long long ld; };
void launch_eq_state(const EqStateArgs& a, hipStream_t st);

// ---- style pass (per utterance) helpers
struct RowMaskArgs { TRef x; TRef m; const int* lens; int T, n, C; int mode; };  // mode 0: sum|x|>0, 1: x[0]!=0
void launch_rowmask(const RowMaskArgs& a, hipStream_t st);
struct WNGateArgs { TRef xin; TRef acts; const int* lens; int T, n, H; };          // tanh(a[:H])*sigmoid(a[H:])
void launch_wn_gate(const WNGateArgs& a, hipStream_t st);
struct WNUpdateArgs { TRef rs; TRef x; TRef out; TRef m; const int* lens; int T, n, H; int last; int first; };
void launch_wn_update(const WNUpdateArgs& a, hipStream_t st);
struct PoolArgs { TRef x; TRef m; TRef y; const int* lens; int T, n, C, group; };  // y = mean over groups of x*m
void launch_group_pool(const PoolArgs& a, hipStream_t st);
struct VQArgs {       // dots[i][s][M] = x.e ; picks argmin of (e2 + x2) - 2*dot, writes z = x + (q - x) and [z | posemb]
  TRef x; TRef dots; TRef cat;
  const float* emb; const float* e2; const float* postable;
  int* ids;            // [i][S_max]
  const int* lens; int S, n, E, M, S_max;
};
void launch_vq(const VQArgs& a, hipStream_t st);
struct KMaskArgs { TRef tok; float* kmask; long long kmask_stride; const int* slots; const int* lens; int S, n, S_max; };
void launch_kmask(const KMaskArgs& a, hipStream_t st);
struct MeanArgs { TRef x; TRef m; float* out; long long out_stride; const int* slots; const int* lens; int T, n, C; };
void launch_masked_mean(const MeanArgs& a, hipStream_t st);
struct ScaleMaskArgs { TRef x; TRef m; const int* lens; int T, n, C; };           // x *= m (in place)
void launch_mul_mask(const ScaleMaskArgs& a, hipStream_t st);

// ---- voice bank (voices.hip; the cell functions are voice_layout.h's).  Grid (work items, call rows), 256 lanes.
__global__ void voice_assign_kernel(const voice::Cache dst, const voice::Cache bank, const voice::AssignRow* __restrict__ rows, int k);      // voice::fill_items(dst) items
__global__ void voice_unpack_kernel(const voice::Cache bank, const voice::MoveRow* __restrict__ rows, const char* __restrict__ blob, long long blob_ld);
__global__ void voice_pack_kernel(const voice::Cache bank, const voice::MoveRow* __restrict__ rows, char* __restrict__ blob, long long blob_ld);      // voice::pack_items items

}  // namespace cnk
