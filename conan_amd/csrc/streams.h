// conan_streams: per-slot streaming state and launch plans (see streams.hip, decoder.hip, style.hip).
#pragma once
#include <array>
#include <functional>

#include "host_common.h"
#include "plan_switches.h"
#include "snapshot_layout.h"
#include "voice_layout.h"

using ch::Error;
using ch::Lin;
using ch::PackedConv;
using ch::Ring;
using cnk::ConvArgs;
using cnk::ConvGroup;
using cnk::TRef;

constexpr int kMaxBranches = 3;
static_assert(plan::kMaxUps == CONAN_MAX_UPS, "plan_switches.h: one UPS_CFG entry per upsampler");
constexpr int PADR = 16;   // zero rows before/after a reference utterance in the style-pass buffers (k31 -> 15)

struct VocStage {
  Ring up;                                  // ups[i] output (pixel shuffled), also residual source
  Ring upa;                                 // leaky_relu(up): c1 operand
  Ring xs;                                  // leaky_relu(mean of the branches): input of ups[i+1] / conv_post
  std::vector<std::vector<Ring>> xt, xo;    // [branch][dilation]; xt is stored activated
  std::vector<std::vector<Ring>> xa;        // leaky_relu(xo) for the outputs that feed another c1
  int C = 0, rate = 1;
  bool fused = false;                       // ResBlock1 units run as one tile pass each (resblock_fused.hip): no xt / activated twins
  bool pair = false;                        // ... by pairs of workgroups (resblock_pair.hip: the wide first stage); xh = history of activated xt per unit
  std::vector<std::vector<Ring>> xh;
};

// Small host tables (slot lists, reference lengths) go to the device through a ring of pinned staging buffers: an
// asynchronous copy from pageable memory may still be reading the host buffer after the call returns, and the callers'
// vectors do not live that long.  A buffer is reused only after the copy that read it has completed (event).
struct PinRing {
  static constexpr int N = 8;
  int* buf = nullptr;
  size_t cap = 0;            // ints per buffer
  hipEvent_t ev[N] = {};
  int next = 0, cur = 0;
  void init(size_t ints) {
    cap = ints;
    HIP_CHECK(hipHostMalloc((void**)&buf, cap * N * sizeof(int), hipHostMallocDefault));
    for (int i = 0; i < N; ++i) HIP_CHECK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
  }
  // copy `n` ints to `dst` (device) on `st`
  void upload(int* dst, const int* src, size_t n, hipStream_t st) {
    if (n > cap) throw ch::Error(CONAN_ERR_INVALID, "host table larger than the staging buffer");
    cur = next; next = (next + 1) % N;
    HIP_CHECK(hipEventSynchronize(ev[cur]));          // never recorded / long complete in the steady state
    memcpy(buf + (size_t)cur * cap, src, n * sizeof(int));
    HIP_CHECK(hipMemcpyAsync(dst, buf + (size_t)cur * cap, n * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipEventRecord(ev[cur], st));
  }
  ~PinRing() {
    for (int i = 0; i < N; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]);
    if (buf) (void)hipHostFree(buf);
  }
};

// Per-call row tables of the waveform I/O kernels (wavio.hip): kStageSets device tables used round robin, set q reused only after the
// last reader of the call that used it has completed (event).  begin() takes the next set on `st` - wait for its event, upload the
// call's rows through the pinned ring - and returns q; the caller enqueues the kernels that read the table and calls end(q, their
// stream).  Staging buffers a call needs sit beside the tables in the owner, indexed by the same q.  Not stream state (state_bytes).
constexpr int kStageSets = 4;
// The activity sets (activity.hip) are read last by the gate on the VOCODER stream of a pipelined call, and begin() makes the next
// call's front-end wait for that.  A pipelined Emformer runs up to 2 * NP steps ahead of the vocoder (it waits for the decoder of step
// t - NP, which waited for the vocoder of step t - 2 NP): with 2 * NP sets the wait asks for nothing the hand-off rings do not already
// ask for.  With kStageSets sets it released the Emformer of step t exactly as the vocoder of step t - 3 began its wide first
// stage, whose workgroup pairs stall on CUs an Emformer workgroup holds (ev_wide below): measured +0.13 ms per 64-stream step
// against +0.025 ms with 2 * NP sets.
constexpr int kActSets = 8;
using RgRow = std::array<int, cnk::kRaggedWords>;      // one call row of mel_stream_ragged_kernel / wav_rows_scatter_kernel
template <typename Row, int kSets = kStageSets>
struct StageSets {
  static_assert(sizeof(Row) % sizeof(int) == 0, "rows are uploaded as ints");
  Row* rows[kSets] = {};
  hipEvent_t ev[kSets] = {};
  PinRing pin;
  long long calls = 0;
  StageSets() = default;
  StageSets(const StageSets&) = delete;
  StageSets& operator=(const StageSets&) = delete;
  void init(int max_rows, std::vector<void*>& allocs) {      // (the tables are freed with the owner's allocations)
    if (pin.buf) return;
    for (int q = 0; q < kSets; ++q) {
      HIP_CHECK(hipMalloc((void**)&rows[q], (size_t)max_rows * sizeof(Row)));
      allocs.push_back(rows[q]);
      if (!ev[q]) HIP_CHECK(hipEventCreateWithFlags(&ev[q], hipEventDisableTiming));
    }
    pin.init((size_t)max_rows * sizeof(Row) / sizeof(int));
  }
  int begin(const Row* host_rows, int n, hipStream_t st) {
    const int q = (int)(calls++ % kSets);
    HIP_CHECK(hipStreamWaitEvent(st, ev[q], 0));
    pin.upload(reinterpret_cast<int*>(rows[q]), reinterpret_cast<const int*>(host_rows), (size_t)n * sizeof(Row) / sizeof(int), st);
    return q;
  }
  void end(int q, hipStream_t st) { HIP_CHECK(hipEventRecord(ev[q], st)); }
  ~StageSets() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

// ---- the per-slot source features (level.hip, f0.hip, register.hip, activity.hip, bypass.hip, conceal.hip, echo.hip, echo_delay.hip, denoise.hip, level_out.hip) share one
// slot-setting type.  cfg: per slot the configuration as set (zeros: off; `reseed` kept 0), which persists across resets; n_on: slots
// with the feature on (On: the cfg field that says so).  Empty until the feature's first enabling call (assign(), from its *_init()
// beside the device state and row tables).  pending: the slot's state restarts in its next kernel row, which clears the flag - a host
// flag, no launch; restart() sets it (a reset with CONAN_MODEL_FRONTEND), and when a setter call does is each feature's own rule.
template <typename Cfg, int32_t Cfg::*On = &Cfg::enabled>
struct SlotSetting {
  std::vector<Cfg> cfg;
  std::vector<char> pending;
  int n_on = 0;
  bool allocated() const { return !cfg.empty(); }
  bool on(int slot) const { return n_on > 0 && cfg[slot].*On != 0; }
  void assign(int max_slots) { cfg.assign(max_slots, Cfg{}); pending.assign(max_slots, 0); }
  // c (zeros where it turns the feature off) -> the listed slots; went_on(i) for each list entry whose slot was off and is on now
  template <typename F>
  void store(const int32_t* slots, int n, const Cfg& c, F&& went_on) {
    Cfg v = c;
    if (!(c.*On)) memset(&v, 0, sizeof(v));
    for (int i = 0; i < n; ++i) {
      Cfg& o = cfg[slots[i]];
      const bool was = o.*On != 0;
      n_on += (v.*On != 0) - was;
      o = v;
      if (v.*On && !was) went_on(i);
    }
  }
  void store(const int32_t* slots, int n, const Cfg& c) { store(slots, n, c, [](int) {}); }
  // the rule of a cfg with a `reseed` field: a reseeding call and an off-to-on change restart the slot
  void store_restarting(const int32_t* slots, int n, Cfg c) {
    const bool reseed = c.*On && c.reseed != 0;
    c.reseed = 0;
    store(slots, n, c, [&](int i) { pending[slots[i]] = 1; });
    for (int i = 0; i < n && reseed; ++i) pending[slots[i]] = 1;
  }
  void restart(const int32_t* slots, int n) { for (int i = 0; i < n && allocated(); ++i) pending[slots[i]] = 1; }
  // the zero-frame rows of a state query (make: the feature's row(), which starts from the seed and names no slot): row i reports to
  // state_row i; a slot that is not pending reads its state (and writes it back as it is).  missing: the error's text behind the slot
  template <typename Row, typename Make>
  std::vector<Row> state_rows(const int32_t* slots, int n, Make make, const char* who, const char* missing) const {
    std::vector<Row> rows((size_t)n);
    for (int i = 0; i < n; ++i) {
      if (!on(slots[i])) throw Error(CONAN_ERR_STATE, std::string(who) + ": slot " + std::to_string(slots[i]) + missing);
      rows[i] = make(cfg[slots[i]]);
      rows[i].state_row = i;
      if (!pending[slots[i]]) { rows[i].slot = slots[i]; rows[i].reseed = 0; }
    }
    return rows;
  }
  void get(int slot, Cfg* out) const {
    if (allocated()) *out = cfg[slot];
    else memset(out, 0, sizeof(*out));
  }
};
// A SlotSetting whose per-slot state is an opaque device record of kBytes that the setter takes back as seed rows and a state query
// hands out (conceal.hip, echo.hip, echo_delay.hip, denoise.hip, watermark.hip; `name`: the feature's in conan_streams_set_<name>,
// conan_streams_<name>_state and conan_<name>_state_bytes).  With it go the row tables of the feature's launches; conan_streams::
// records_init() allocates both and record_state() (below) is the state query.
template <typename Cfg, typename RowT, typename Rec, int kSetsN = kStageSets, size_t kBytes = sizeof(Rec)>
struct RecordSetting : SlotSetting<Cfg> {
  using Row = RowT;
  static constexpr size_t kRecBytes = kBytes;
  static constexpr int kSets = kSetsN;
  Rec* state = nullptr;      // [max_slots] records; stream state
  StageSets<Row, kSets> sets;
  char* record(int slot) const { return reinterpret_cast<char*>(state) + (size_t)slot * kBytes; }
  // seed rows and state rows: at least a record apart, pointer and stride 8-byte aligned
  // (the entry point's name in three parts - "conan_streams_set_", name, "" - so that a call that passes builds no string)
  static void check_rows(const char* who_head, const char* name, const char* who_tail, const void* p, int64_t ld) {
    if (ld < (int64_t)kBytes || ((uintptr_t)p & 7) || (ld & 7))
      throw Error(CONAN_ERR_INVALID, std::string(who_head) + name + who_tail + ": rows are conan_" + name + "_state_bytes bytes, 8-byte aligned, ld apart");
  }
  // seed row i becomes the record of slots[i], now, and the slot restarts no more - for the list entries that take(i) names
  template <typename Take>
  void seed(const int32_t* slots, int n, const void* seed_dev, int64_t seed_ld, hipStream_t st, Take&& take) {
    for (int i = 0; i < n; ++i) {
      if (!take(i)) continue;
      HIP_CHECK(hipMemcpyAsync(record(slots[i]), static_cast<const char*>(seed_dev) + (size_t)i * seed_ld, kBytes, hipMemcpyDeviceToDevice, st));
      this->pending[slots[i]] = 0;
    }
  }
};
// A row of a feature's most recent wav-in call, for the conan_step_wav_* hooks: call row, the staging set, the chunk row there, frames
struct LastRow { int row, set, src, emit; };

struct conan_streams {
  conan_ctx* ctx = nullptr;
  std::atomic<int>* live = nullptr;            // this device's count of live stream-sets (device_live_streams)
  // developer / test switches of the launch plan (plan_switches.h), resolved once by conan_streams_create_opts from conan_streams_opts.dev_plan
  const plan::PlanSwitches sw;
  explicit conan_streams(const plan::PlanSwitches& p) : sw(p) {}
  // CONAN_STREAMS_FIXED_PLAN: every plan choice from max_slots, never from the step's active slot count
  bool fixed_plan = false;
  // (the per-utterance style pass of a fixed-plan stream-set runs one slot at a time: its plan follows the slot's own reference length)
  bool in_style_pass = false;
  int plan_n(int n) const { return (fixed_plan && !in_style_pass) ? max_slots : n; }
  bool pipe_idle = false;                      // set by conan_step_async: no earlier pipelined step of this stream-set is still in flight
  bool shared_device = false;                  // CONAN_STREAMS_SHARED_DEVICE: other processes drive this GPU too - never take whole-chip launch shapes
  int max_slots = 0, max_frames = 0, max_ref = 0, S_max = 0;
  std::vector<void*> allocs;
  int64_t state_bytes = 0;
  std::vector<std::pair<float*, long long>> voc_state, dec_state, emf_state;  // (base, floats per slot) to zero on reset

  int* d_slots = nullptr;   // [max_slots]
  int* d_ident = nullptr;   // identity 0..max_slots-1
  int* d_zero = nullptr;    // zeros (pos array for batch-indexed style pass)
  int* d_lens = nullptr;    // [max_slots] per-batch lengths (style pass)
  int* d_lens2 = nullptr;
  int* d_codes = nullptr;   // [max_slots][max_frames] codes scratch for the fused step
  // inter-block split-K workspaces (partial tiles + ticket counters), one per stream that can have conv launches in
  // flight (ws_index): the caller's stream / pipelined decoder, the pipelined vocoder, the pipelined Emformer
  // (conan_step_async runs the three concurrently, and all split K at small batch sizes)
  float* sk_slab[3] = {nullptr, nullptr, nullptr};
  int* sk_counters[3] = {nullptr, nullptr, nullptr};
  bool rb_limb = false;         // bf16-limb form of the vocoder's matrix kernels where it exists (conan_streams_opts.arith, resolved at creation)
  bool arith_auto = true;       // the caller left the choice to the library (conan_streams_opts.arith == AUTO)
  int* cp_ticket[3] = {nullptr, nullptr, nullptr};   // conv_post's last-workgroup ticket, per internal stream
  int* rb_sched[2] = {nullptr, nullptr};   // work-queue counters of the fused resblock launches, per stream like the split-K workspaces
  // resblock_pair workspaces (per stream like rb_sched): exchange buffers, and one block of zero-initialised words:
  // [pairs][8] flags | [pairs][4] mailboxes | [pairs][2] tile counts | 2 queue words
  float* rp_xb[2] = {nullptr, nullptr};
  unsigned* rp_words[2] = {nullptr, nullptr};
  long long sk_slab_floats = 0;
  int sk_max_tiles = 0;
  std::vector<int> h_slots;
  std::vector<int> slot_seen;   // duplicate detection: generation stamp per slot
  int slot_gen = 0;
  PinRing pin;
  int* pos_emf = nullptr; int* pos_dec = nullptr; int* pos_voc = nullptr;
  // bounded cross-workgroup waits (kernels.h, SpinGuard): guard block in device memory + the host-mapped word a waiter that gave
  // up copies its code to; check_fault() turns a non-zero word into CONAN_ERR_HIP at every stream-ordered entry point, for good
  unsigned* d_guard = nullptr;
  unsigned* h_guard = nullptr;
  int test_fault = 0;           // conan_streams_test_fault: the next launch of that kind waits for an arrival that never comes
  void check_fault() const {
    if (!h_guard) return;
    const unsigned code = *(volatile const unsigned*)h_guard;
    if (code == 0) return;
    static const char* what[] = {"?", "decoder_mega_kernel group / grid barrier", "emformer_fused_kernel cluster exchange", "resblock_pair_kernel partner flag", "resblock_pair_kernel tile mailbox",
                                 "(retired)", "decoder_mega_kernel xcd election", "decoder_mega_kernel xcd roll call", "decoder_mega_kernel xcd flag barrier"};
    throw ch::Error(CONAN_ERR_HIP, std::string("a cross-workgroup wait gave up after its 50 ms budget (") + what[code < 9 ? code : 0] +
                                       "): results since then are invalid and this stream-set is unusable - destroy it and create a new one");
  }

  // --- waveform input (wavio.hip).  Streaming front-end (conan_step_wav): per slot an audio ring (sample s at s & (fe_LA - 1)) and a
  // ring of computed log-mel frames (frame f at f & (fe_LM - 1)); fe_chunk = the [n][seg + rc][num_mels] chunk the step consumes.  Host
  // side, per slot: samples received, frames computed, chunks emitted, phase (0 open, 1 the final call has come, 2 drained)
  struct FeSlot { long long recv = 0; int frames = 0, chunks = 0, phase = 0; };
  // (dr: the slot's drift resampler, conan_streams_set_input_drift - it replaces f, and a rate setter removes it)
  struct RsSlot { const ch::RsTable* f = nullptr; long long in = 0, out = 0; int phase = 0; ch::DriftPos dr; int s_in = 0; bool rated() const { return f || dr.d; } };
  struct WavIn {
    float* fe_audio = nullptr; float* fe_mel = nullptr; float* fe_chunk = nullptr;
    int fe_LA = 0, fe_LM = 0, fe_last_n = 0;
    std::vector<FeSlot> fe_slot;
    // conan_step_wav_ragged: per call a [n][kRaggedWords] row table (set q of rg_sets) and, when the emit groups' outputs need
    // reordering, staging for them beside it; the set's event follows the last reader of the call.  Allocated on the first ragged
    // call; not stream state (state_bytes).
    StageSets<RgRow> rg_sets;
    int* rg_codes[kStageSets] = {}; float* rg_mel[kStageSets] = {}; float* rg_wav[kStageSets] = {};
    bool fe_last_ragged = false;      // the last wav-in call was ragged: fe_chunk holds its rows grouped by emit (conan_step_wav_chunk refuses)
    // input resampler (conan_streams_set_input_rate): per slot the filter (null: input at the model rate), input samples received,
    // model-rate samples handed to the front-end, phase (1: the input's final call has come).  The history ring ([max_slots][kRsRing],
    // stream state) and per call a row table (set q of rs_sets) and model-rate staging beside it (the set's event follows the
    // front-end launch that read it) are allocated by the first conan_streams_set_input_rate.
    std::vector<RsSlot> rs_slot;
    float* rs_ring = nullptr;
    StageSets<cnk::RsRow> rs_sets;
    float* rs_wav[kStageSets] = {};
    // sample formats of the caller's rows (conan_streams_set_input_format; cnk::kFmt*), per slot; they persist across resets.  A slot
    // with a format and no rate takes the copy rows of resample_stream_kernel.  in_fmt_n: slots whose format is not f32 (0: every
    // launch is today's).
    std::vector<unsigned char> in_fmt;
    int in_fmt_n = 0;
  } wav_in;
  // --- the per-slot source features: each a SlotSetting (above) with its device state, its per-call row tables (set q of `sets`) and
  // the staging beside them, allocated by the first enabling call (*_init()).  What differs:
  // input leveller (conan_streams_set_input_level; level.hip).  state: [max_slots] of `stride` bytes (cnk::LvState and the two block
  // rings; stream state).  The kernel works in place on the resampler's staging rows (wav_in.rs_wav), so such a stream-set has those
  // too.  Rows: the levelled call rows with samples (and copy rows, see level::WavStage).  Event: behind the front-end launch.
  struct InLevel : SlotSetting<conan_level_cfg> {
    char* state = nullptr; long long stride = 0;
    StageSets<cnk::LvRow> sets;
    cnk::LvFilter filter;
  } in_lv;
  void level_init(const cnk::LvFilter& f);
  // source-pitch following (conan_streams_set_pitch_follow; f0.hip).  The tracker keeps no state: a wav-in call that emits a chunk
  // tracks the chunk's frames from the slot's audio ring.  Rows: one per following call row that emits; beside the table the contour
  // the call's decoder steps read, ct_f0 / ct_uv [q][chunk row][seg] (chunk row = the row's place in the call's emit groups, as
  // fe_chunk; stream state).  Event: behind the last decoder step of the call, so the contour of a pipelined call outlives the
  // front-ends of the calls behind it.  last: conan_step_wav_contour.
  struct Follow : SlotSetting<conan_f0_cfg> {
    float* ct_f0[kStageSets] = {}; float* ct_uv[kStageSets] = {};
    StageSets<cnk::F0Row> sets;
    std::vector<LastRow> last;
  } follow;
  void follow_init();
  // register matching (conan_streams_set_pitch_register; register.hip).  state: [max_slots][2] = (n, S), read and written by the rows
  // of f0_register_kernel in the order of the front-end launches; pending restarts it from the cfg's seed.  Rows: one per following
  // row whose slot has the register on; it rewrites its place in the contour.  Event: behind the kernel's launch.
  struct Register : SlotSetting<conan_register_cfg> {
    long long* state = nullptr;
    StageSets<cnk::RegRow> sets;
  } reg;
  void register_init();
  // source activity (conan_streams_set_activity; activity.hip; on: mode != 0).  state: [max_slots], read and written by the rows of
  // activity_kernel in the order of the front-end launches; pending restarts it from the cfg's seed.  Rows: one per emitting call row
  // in chunk-row order, mode 0 for a slot without the feature; beside the table the flags [q][chunk row][seg] and the levels
  // [q][chunk row][seg + 1] (word 0: the level before the chunk) on their way from the front-end stage to the vocoder stage of the
  // same call, whose gate reads table and levels.  Event: on the stream of the call's last vocoder step, behind the gate launch, so
  // under pipelining a set outlives the front-ends of the calls behind it (kActSets sets, not kStageSets: see there).
  // last: conan_step_wav_activity.
  struct Activity : SlotSetting<conan_activity_cfg, &conan_activity_cfg::mode> {
    cnk::ActState* state = nullptr;
    int* flags[kActSets] = {}; int* levels[kActSets] = {};
    StageSets<cnk::ActRow, kActSets> sets;
    std::vector<LastRow> last;
  } act;
  void activity_init();
  // source bypass (conan_streams_set_bypass; bypass.hip).  state: [max_slots], read and written by the rows of bypass_stage_kernel in
  // the order of the front-end launches; pending restarts it from the cfg's seed.  Rows: as the activity table's; beside the table
  // the wet and effective dry levels [q][chunk row][seg + 1] (word 0: the level before the chunk) and the dry samples
  // [q][chunk row][seg * hop] on their way to the vocoder stage of the same call.  The samples are staged, not read from the audio
  // ring by the mix: under pipelining the vocoder runs several calls behind the front-end that overwrites the ring.  Event: behind
  // the call's last vocoder step; kActSets sets for the reason given there.  last: conan_step_wav_bypass.
  struct Bypass : SlotSetting<conan_bypass_cfg> {
    cnk::BypState* state = nullptr;
    int* wet_lvl[kActSets] = {}; int* dry_lvl[kActSets] = {}; float* dry[kActSets] = {};
    StageSets<cnk::BypRow, kActSets> sets;
    std::vector<LastRow> last;
  } byp;
  void bypass_init();
  // comfort noise (conan_streams_set_comfort; comfort.hip; on: mode != 0).  state: [max_slots], read and written by the rows of
  // comfort_track_kernel in the order of the front-end launches; pending restarts it from the cfg's seed_level.  Rows: as the activity
  // table's (a slot without a detector holds its place only); beside the table the frame-end levels [q][chunk row][seg + 1] (word 0: the
  // level before the chunk) on their way to the vocoder stage of the same call, whose fill reads table, levels and the activity set's
  // gate levels, and the powers [q][chunk row][seg] the detector of a call with a following row stages for the tracker.  Event: behind
  // the call's last vocoder step; kActSets sets for the reason given there.  last: conan_step_wav_comfort.
  struct Comfort : SlotSetting<conan_comfort_cfg, &conan_comfort_cfg::mode> {
    cnk::CmfState* state = nullptr;
    int* levels[kActSets] = {}; double* powers[kActSets] = {};
    StageSets<cnk::CmfRow, kActSets> sets;
    std::vector<LastRow> last;
  } cmf;
  void comfort_init();
  // signalling tones (conan_streams_set_tones; tone.hip; on: mode != 0).  state: [max_slots], read and written by the rows of
  // tone_kernel in the order of the front-end launches; pending restarts it from the cfg's seed.  Rows: as the activity table's;
  // beside the table the frame digits [q][chunk row][seg] and the sounds and levels [q][chunk row][seg + 1] (word 0: the value
  // before the chunk) on their way to the vocoder stage of the same call, whose fill reads table, sounds and levels.  Event: behind
  // the call's last vocoder step; kActSets sets for the reason given there.  last: conan_step_wav_tones.
  struct Tones : SlotSetting<conan_tone_cfg, &conan_tone_cfg::mode> {
    cnk::ToneState* state = nullptr;
    const short* table = nullptr;
    int* digit[kActSets] = {}; int* sound[kActSets] = {}; int* level[kActSets] = {};
    StageSets<cnk::ToneRow, kActSets> sets;
    std::vector<LastRow> last;
  } tn;
  void tones_init();
  // The shared *_init() of a RecordSetting, behind the feature's first enabling call: the zeroed records and the row tables, both
  // stream state (kSets is spelt out where it is called: the tables' count is part of what state_bytes reports); false: done before
  template <int kSets, typename R>
  bool records_init(R& r) {
    static_assert(kSets == R::kSets, "the feature's own number of row tables");
    if (r.state) return false;
    r.state = reinterpret_cast<decltype(r.state)>(alloc((size_t)max_slots * R::kRecBytes / sizeof(float)));
    r.sets.init(max_slots, allocs);
    state_bytes += (int64_t)kSets * max_slots * sizeof(typename R::Row);
    r.assign(max_slots);
    return true;
  }
  // --- the pre-step row features (prestep.h): each a RecordSetting whose kernel works on the caller's device rows in front of the
  // wav-in step calls, in the order of the caller's stream; no step path reads any of it.  pending restarts the record in the slot's
  // next row (set when a slot that was off is enabled without a seed; a seed clears it).  Rows: per call; event: behind the kernel's
  // launch.  What differs:
  // input loss concealment (conan_streams_set_conceal; conceal.hip): restarts from zeros, keeps no position.
  struct Conceal : RecordSetting<conan_conceal_cfg, cnk::ConcRow, char, kStageSets, cnk::kConcStateBytes> {} conc;
  void conceal_init() { records_init<kStageSets>(conc); }
  // echo cancellation (conan_streams_set_echo; echo.hip).  pos: per slot the samples cancelled since its restart as the host counts
  // them (a seed's is read back): the kernel takes the pending block's fill from the call row, never from the record.
  struct Echo : RecordSetting<conan_echo_cfg, cnk::EchoRow, char, kStageSets, cnk::kEchoStateBytes> {
    std::vector<long long> pos;
  } ec;
  void echo_init() { if (records_init<kStageSets>(ec)) ec.pos.assign(max_slots, 0); }
  // echo delay (conan_streams_set_echo_delay; echo_delay.hip).  pos: as the canceller's, for the pending frame's fill.
  struct EchoDelay : RecordSetting<conan_echo_delay_cfg, cnk::EdRow, char, kStageSets, cnk::kEdStateBytes> {
    std::vector<long long> pos;
  } ed;
  void echo_delay_init() { if (records_init<kStageSets>(ed)) ed.pos.assign(max_slots, 0); }
  // input noise suppression (conan_streams_set_denoise; denoise.hip).  state: [max_slots] records of conan_denoise_state, read and
  // written by the rows of denoise_stream_kernel in the order of the front-end launches; pending restarts it before the slot's next
  // frame (a seed row becomes the state at once and clears the flag).  Rows: one per suppressing call row that completes a frame or
  // emits.  Event: behind the kernel's launch, in the front-end work.
  struct Denoise : RecordSetting<conan_denoise_cfg, cnk::DnRow, cnk::DnState> {} dn;
  void denoise_init() { records_init<kStageSets>(dn); }
  // a reset with CONAN_MODEL_FRONTEND: the settings stay; the states restart in the slots' next rows (host flags: no launch)
  void restart_features(const int32_t* slots, int n) { reg.restart(slots, n); act.restart(slots, n); byp.restart(slots, n); cmf.restart(slots, n); conc.restart(slots, n); ec.restart(slots, n); ed.restart(slots, n); dn.restart(slots, n); tn.restart(slots, n); in_eq.restart(slots, n); }
  void ragged_init();
  void resample_init();        // staging, row tables and the history ring (conan_streams_set_input_rate)
  void rs_stage_init();        // staging and row tables only (conan_streams_set_input_format: no stream state)
  // --- waveform output (wavio.hip).  Output resampler (conan_streams_set_output_rate): per slot the filter (null: audio leaves at the
  // model rate), output samples delivered, whether conan_streams_flush_output has ended the utterance.  voc_samples = model-rate
  // samples the slot's vocoder has produced since its last reset with CONAN_MODEL_HIFIGAN (kept from creation on: pos_voc is device
  // memory).  The history ring ([max_slots][or_ring_len], stream state) is allocated by the first conan_streams_set_output_rate with a
  // real rate; conv_post's staging rows and the row table (set q of or_sets; the set's event follows the resample_out_kernel launch
  // that read it) by the first vocoder step that needs them.
  // (dr: the slot's drift resampler, conan_streams_set_output_drift - it replaces f, and a rate setter removes it)
  struct OrSlot { const ch::RsTable* f = nullptr; long long out = 0; int flushed = 0; ch::DriftPos dr; int out_rate = 0; bool rated() const { return f || dr.d; } };
  struct WavOut {
    std::vector<OrSlot> or_slot;
    std::vector<long long> voc_samples;
    float* or_ring = nullptr; int or_ring_len = 0;
    StageSets<cnk::RsOutRow> or_sets;
    float* or_wav[kStageSets] = {};
    long long out_ld = 0;                     // conan_streams_set_output_ld (0: each entry point's own stride)
    std::vector<int32_t> out_counts;          // conan_streams_output_samples: per row of the most recent step call
    // sample formats of the caller's rows (conan_streams_set_output_format), as wav_in.in_fmt; the copy rows are resample_out_kernel's
    std::vector<unsigned char> out_fmt;
    int out_fmt_n = 0;
  } wav_out;
  // output leveller (conan_streams_set_output_level; level_out.hip), a SlotSetting as the source features.  state: [max_slots] of `stride` bytes on the device (cnk::LvState, the two block rings, the previous
  // instant's stats), written by level_out_meter_kernel and read by the next step's level_out_apply_kernel in stream order.  The
  // restart of a reset with CONAN_MODEL_HIFIGAN needs no flag of its own: it returns voc_samples to 0, and a row at position 0
  // starts meter and gain in both kernels.  Per vocoder step with a levelled row a row table (set q of `sets`: one row per step row,
  // on = 0 for a slot without the feature) and beside it the staging rows [q][step row][U] in which the apply leaves the unlevelled
  // samples for the meter - staged, not read from the step's rows, because the meter runs behind the apply, the gate and the mix,
  // which all work in place.  The set's event is recorded behind the meter launch.  Allocated by the first enabling call; state,
  // staging and row tables count as stream state.
  struct OutLevel : SlotSetting<conan_level_cfg> {
    char* state = nullptr; long long stride = 0;
    float* stage[kActSets] = {};
    StageSets<cnk::OlRow, kActSets> sets;
    cnk::LvFilter filter;
  } out_lv;
  void out_level_init(const cnk::LvFilter& f);
  // output watermark (conan_streams_set_watermark; watermark.hip), a SlotSetting as the others.  state: [max_slots] records of
  // conan_watermark_state, read and written by the rows of watermark_embed_kernel in the order of the vocoder steps; pending restarts
  // it from zeros in the slot's next step row (set when a slot that was off is enabled, by reseed = 1 without a seed and by a reset
  // with CONAN_MODEL_HIFIGAN; a seed row becomes the state at once and clears the flag).  Per vocoder step with a marked row a row
  // table (set q of `sets`: one row per step row, on = 0 for a slot without the feature); the set's event is recorded behind the
  // embed launch.  Allocated by the first enabling call; state and row tables count as stream state.
  struct Watermark : RecordSetting<conan_watermark_cfg, cnk::WmRow, cnk::WmState, kActSets> {} wm;
  void watermark_init() { records_init<kActSets>(wm); }
  // equaliser (conan_streams_set_input_eq / conan_streams_set_output_eq; eq.hip), a SlotSetting on each side.  state: [max_slots]
  // records of conan_eq_state; sec: [max_slots][kEqMaxSec] sections with their transition matrices, written by the setter's launch in
  // stream order; origin: per slot the grid's first sample as the host knows it (the kernels take every index from the call rows).
  // pending restarts the state in the slot's next row, at that row's position (a reset with CONAN_MODEL_FRONTEND / CONAN_MODEL_HIFIGAN).
  // Source side: position = fe_slot.recv, rows: the filtered call rows with samples (and copy rows, see eq::WavStage), event behind the
  // launch.  Output side: position = voc_samples, one row per step row (on = 0: a slot without the feature), event behind the launch.
  // Allocated by a side's first enabling call; state, sections and row tables count as stream state.
  struct Eq : SlotSetting<conan_eq_cfg> {
    cnk::EqState* state = nullptr;
    cnk::EqSec* sec = nullptr;
    std::vector<long long> origin;
    StageSets<cnk::EqRow, kActSets> sets;
  } in_eq, out_eq;
  void eq_init(Eq& e);
  void out_stage_init();
  void out_ring_init();        // the output resampler's history ring (conan_streams_set_output_rate with a real rate)
  // --- slot snapshots (snapshot.hip).  rings: every ring of mk_ring in creation order with its position counter (0 pos_emf,
  // 1 pos_dec, 2 pos_voc).  The layout and its device tables are built by the first export / import and rebuilt when a rate ring is
  // first allocated; per call a table of snap::CallRow (set q of snap_sets).  Not stream state (state_bytes).  in_cfg / out_cfg: the
  // rate setters' configurations per slot (in_rate == out_rate: none), which travel with a snapshot.
  struct Snap {
    std::vector<std::pair<Ring, int>> rings;
    snap::Layout layout;
    bool lay_ok = false, built = false;      // the host layout is current; the device tables hold it
    const float* lay_rs = nullptr; const float* lay_or = nullptr;      // the rate rings the layout was built with
    const char* lay_lv = nullptr;                                      // ... and the leveller's state
    snap::Region* d_regions = nullptr; int* d_item_first = nullptr;
    StageSets<std::array<int, 4>> sets;
    std::vector<conan_resample_cfg> in_cfg, out_cfg;
  } snapshot;
  void snapshot_build();
  // One vocoder step's output rows, checked before anything changes (out_plan) and handed to hifigan_step, which commits the slots'
  // counters once its launches are enqueued.  active: the step's audio goes through staging and resample_out_kernel.
  struct OutPlan {
    bool active = false;
    std::vector<cnk::RsOutRow> rows;
    std::vector<int32_t> counts;            // samples per row of this step
    std::vector<int> dst;                   // rows of the call's buffer and of out_counts (empty: 0 .. n-1)
    float* base = nullptr; long long ld = 0;
    int tiles = 1, win = 0;
    double flops = 0;
    // the step's output gate (activity.hip; filled by act::WavStage for a group with a gated row): the group's rows of the call's
    // activity table and of its level staging; hifigan_step launches activity_gate_kernel on the rows conv_post wrote
    struct Gate { const cnk::ActRow* tab = nullptr; const int* lvl = nullptr; int lvl_ld = 0; } gate;
    // the step's wet/dry mix (bypass.hip; filled by byp::WavStage for a group with a bypass row): the group's rows of the call's bypass
    // table, of its level staging and of its dry staging; hifigan_step launches bypass_mix_kernel behind the gate
    struct Mix {
      const cnk::BypRow* tab = nullptr; const int* wet_lvl = nullptr; const int* dry_lvl = nullptr; const float* dry = nullptr;
      int lvl_ld = 0; long long dry_ld = 0;
    } mix;
    // the step's comfort noise (comfort.hip; filled by comfort::WavStage for a group with a filled row): the group's rows of the call's
    // comfort table and level staging and of the activity set's gate levels (one stride: both stagings have rows of seg + 1 words);
    // hifigan_step launches comfort_fill_kernel behind the mix
    struct Fill { const cnk::CmfRow* tab = nullptr; const int* cmf_lvl = nullptr; const int* gate_lvl = nullptr; int lvl_ld = 0; } fill;
    // the step's output levelling (level_out.hip; out_plan's, for a step with a levelled row): one table row per step row;
    // hifigan_step launches level_out_apply_kernel behind conv_post and level_out_meter_kernel behind the step's last launch
    std::vector<cnk::OlRow> lvl_rows;
    // the step's watermark (watermark.hip; out_plan's, for a step with a marked row): one table row per step row; hifigan_step
    // launches watermark_embed_kernel behind the fill and in front of the output resampler
    std::vector<cnk::WmRow> wm_rows;
    // the step's regenerated tones (tone.hip; filled by tone::WavStage for a group with a mode-2 row): the group's rows of the call's
    // tone table and of its sound and level staging; hifigan_step launches tone_fill_kernel behind the watermark, as the last
    // in-place stage in front of the output resampler
    struct Tone { const cnk::ToneRow* tab = nullptr; const int* sound = nullptr; const int* level = nullptr; int lvl_ld = 0; } tone;
    // the step's equaliser (eq.hip; out_plan's, for a step with a filtered row): one table row per step row; hifigan_step launches
    // eq_stream_kernel directly behind conv_post, in front of the output leveller's ramp
    std::vector<cnk::EqRow> eq_rows;
  };
  OutPlan out_plan(const int32_t* slots, int n, int frames, float* wav_out_dev, long long natural_ld, const std::vector<int>* dst, const std::string& who) const;
  // the plan's resample_out_kernel launch behind or_sets.begin() = q, then the set's event; src_ld: stride of the staged rows (a flush: 0)
  void resample_out(const OutPlan& op, int q, long long src_ld, hipStream_t st);
  // --- vocoder
  Ring v_mel, v_pre;
  std::vector<VocStage> v_st;
  // --- emformer
  std::vector<Ring> e_k, e_v;
  std::vector<float*> e_bank;     // memory bank per layer: [slot][e_bank_rows][D] (max_memory_size > 0)
  int e_bank_rows = 0;
  float* e_mems[2] = {nullptr, nullptr};   // memory input / output of a layer, [n][D]
  Lin e_x[2], e_ln, e_q, e_kv, e_att, e_r1, e_ffn, e_h, e_r2, e_logits;
  bool emf_fused = false;
  cnk::EmfFusedArgs emf_fused_args;
  // --- conan decoder
  Ring c_emb, c_pin2, c_lastr;
  std::vector<Ring> c_uvh;      // outputs of the uv predictor's conv layers but the last (each keeps its own left context)
  std::vector<Ring> c_lnrs;     // post-LN rings, one per (block, sub-layer)
  Lin c_pin, c_q, c_att, c_a1, c_a2, c_ff, c_uv5, c_x[2], c_h, c_post, c_mask_blk, c_mask_blk2, c_mask_out, c_mel, c_part, c_part2;
  float* c_style = nullptr;     // [slot][H]
  float* c_kv = nullptr;        // [slot][2 layers][S_max][2H]
  float* c_kmask = nullptr;     // [slot][S_max]
  int* c_slen = nullptr;        // [slot]
  int* c_vqids = nullptr;       // [slot][S_max] VQ indices of the prosody tokens (-1 past the token count)
  std::vector<char> has_ref;    // per slot: conan_set_reference has run for it (or conan_streams_set_voice)
  // voice bank (voices.hip): the id last assigned whole to the slot (conan_streams_voice; -1: none, or overwritten since), and the
  // setter's call rows on their way to the device (allocated by the first call; not stream state)
  std::vector<int> voice_of;
  StageSets<std::array<int, sizeof(voice::AssignRow) / sizeof(int)>> voice_sets;
  voice::Cache style_cache() const { return voice::Cache{c_style, c_kv, c_kmask, c_slen, c_vqids, S_max, ctx->cfg.hidden_size}; }
  // pitch control (pitch.hip; conan_streams_set_pitch): the kernels' table [max_slots], indexed by slot, allocated with the decoder
  // (stream state: 24 bytes per slot, zero = disabled) and the cfgs as set (they persist across resets and travel with a snapshot).
  // pt_stage / pt_pin: the setter's call rows on their way to the device, allocated by the first call; not stream state.
  cnk::PitchSlot* d_ptab = nullptr;
  std::vector<conan_pitch_cfg> pt_cfg;
  cnk::PitchRow* pt_stage = nullptr;
  PinRing pt_pin;
  void pitch_write(const int32_t* slots, int n, const conan_pitch_cfg* cfgs, hipStream_t st);      // cfgs[i] -> slot slots[i], host and device
  std::vector<char> voc_fresh;  // per slot: vocoder state reset and not stepped since (voc_upsample 2 steps need it)
  // --- style pass workspace (batch indexed, max_slots_sp at a time)
  int sp_batch = 0;
  Lin s_mel, s_np, s_wnm, s_x[2], s_ln, s_h, s_blkm, s_wx, s_wout, s_win, s_acts, s_rs, s_ph, s_pm, s_px[2], s_pln, s_phh,
      s_pblk, s_enc, s_dots, s_cat, s_tok, s_kvtmp;
  int* s_ids = nullptr;

  float* alloc(size_t floats) {
    void* p = nullptr;
    if (floats == 0) floats = 4;
    HIP_CHECK(hipMalloc(&p, floats * sizeof(float)));
    HIP_CHECK(hipMemset(p, 0, floats * sizeof(float)));
    allocs.push_back(p);
    state_bytes += (int64_t)floats * 4;
    return (float*)p;
  }
  void* stage_alloc(size_t bytes) { void* p = nullptr; HIP_CHECK(hipMalloc(&p, bytes)); allocs.push_back(p); return p; }   // per-call staging: not stream state
  Ring mk_ring(int C, int rate, int hist, std::vector<std::pair<float*, long long>>* reg) {
    Ring r; r.C = C; r.rate = rate; r.hist = hist;
    r.L = ch::next_pow2(hist + max_frames * rate);
    r.slot_stride = (long long)r.L * C;
    r.base = alloc((size_t)max_slots * r.slot_stride);
    if (reg) reg->push_back({r.base, r.slot_stride});
    if (reg) snapshot.rings.push_back({r, reg == &voc_state ? 2 : (reg == &dec_state ? 1 : 0)});
    return r;
  }
  Lin mk_lin(int rows, int C, int nb = -1) {
    Lin l; l.rows = rows; l.C = C;
    l.base = alloc((size_t)(nb < 0 ? max_slots : nb) * rows * C);
    return l;
  }
  // --- pipelined stepping (conan_step_async): front-end (Emformer + decoder) and vocoder on two internal streams
  hipStream_t st_emf = nullptr, st_front = nullptr, st_voc = nullptr;
  // pipelined steps: recorded on the vocoder stream behind the wide first stage's pair-kernel launches (its workgroups wait for
  // their partners: a CU that an Emformer workgroup holds stalls a whole pair).  Developer switch EMF_HOLD (sw.emf_hold): the Emformer of
  // step t is held back until the vocoder of step t-2 has passed that point.  Measured: with the limb kernels and the pair kernel
  // (CONAN_RB_PAIR=1) the mean step is unchanged and the p95 of the step intervals falls from 1.63 to 1.57 ms; with the exact-f32
  // kernels (1.77 ms steps) it costs 2.6 % (1.815 against 1.769 ms) - off by default.
  hipEvent_t ev_wide[4] = {};
  hipEvent_t mark_wide = nullptr;            // set around hifigan_step by conan_step_async
  bool wide_marked[4] = {false, false, false, false};   // the step at this ring position recorded its ev_wide (it has a pair stage)
  static constexpr int NP = 4;                 // depth of the hand-off rings: a stage may run up to NP steps ahead of its consumer
  hipEvent_t ev_in[NP] = {}, ev_emf[NP] = {}, ev_front[NP] = {}, ev_voc[NP] = {};   // (one input event per ring position: a single
                                               // event re-recorded while its previous record is still pending stalls the pipeline)
  hipEvent_t ev_fence[NP] = {};                // output fences (conan_streams_output_fence)
  hipStream_t fence_stream = nullptr; bool fence_set = false;
  hipEvent_t fence_event = nullptr;            // conan_streams_output_fence_event: wait for this recorded event instead of the stream's tail
  int* codes_hand[NP] = {};                    // code hand-off buffers Emformer -> decoder [max_slots][segment]
  // workspace index of a stream: 0 caller / pipelined decoder, 1 pipelined vocoder, 2 pipelined Emformer
  int ws_index(hipStream_t st) const { return (st_voc && st == st_voc) ? 1 : ((st_emf && st == st_emf) ? 2 : 0); }
  float* mel_hand[NP] = {};                    // mel hand-off buffers decoder -> vocoder [max_slots][max_frames][num_mels]
  long long async_steps = 0;                   // steps enqueued since creation
  std::vector<hipEvent_t> clock_ev;            // conan_step_clock: one timing event per pipelined step, on the vocoder stream
  bool clock_on = false; int clock_n = 0;
  std::vector<hipEvent_t> tl_ev;               // conan_step_timeline: 6 timing events per pipelined step (start / end of each stage on its stream)
  bool tl_on = false; int tl_n = 0;
  void async_init();
  void join(hipStream_t st);                   // make `st` wait for everything enqueued by conan_step_async
  // what a stream-ordered entry point does once its arguments have passed: the device, check_fault(), join -> the stream
  hipStream_t enter(void* stream) { HIP_CHECK(hipSetDevice(ctx->device)); check_fault(); join((hipStream_t)stream); return (hipStream_t)stream; }

  void mega_print_stamps();
  ~conan_streams() {
    if (live) live->fetch_sub(1);
    if (mega_dbg) mega_print_stamps();
    if (st_emf) (void)hipStreamDestroy(st_emf);
    if (st_front) (void)hipStreamDestroy(st_front);
    if (st_voc) (void)hipStreamDestroy(st_voc);
    for (int i = 0; i < NP; ++i) { if (ev_in[i]) (void)hipEventDestroy(ev_in[i]); if (ev_fence[i]) (void)hipEventDestroy(ev_fence[i]); }
    for (int i = 0; i < NP; ++i) { if (ev_wide[i]) (void)hipEventDestroy(ev_wide[i]); if (ev_emf[i]) (void)hipEventDestroy(ev_emf[i]); if (ev_front[i]) (void)hipEventDestroy(ev_front[i]); if (ev_voc[i]) (void)hipEventDestroy(ev_voc[i]); }
    for (void* p : allocs) (void)hipFree(p);
    if (h_guard) (void)hipHostFree(h_guard);
    for (auto& e : prof_ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (auto& e : clock_ev) (void)hipEventDestroy(e);
    for (auto& m : mega_cache) { if (m.copied) (void)hipEventDestroy(m.copied); if (m.pinned) (void)hipHostFree(m.pinned); if (m.dev) (void)hipFree(m.dev); }
    for (auto& e : tl_ev) (void)hipEventDestroy(e);
  }

  void build_vocoder();
  void build_emformer();
  void build_decoder();
  void set_slots(const int32_t* slots, int n, hipStream_t st);
  int pick_cfg(int M, int N, int nprob) const;
  // optional per-launch timing of the conv kernel family (conan_profile_*): HIP events on the launch stream
  bool prof_on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev;
  size_t prof_used = 0;
  double prof_flops = 0.0;
  long long prof_launches = 0;
  struct ProfRec { std::string name; double flops; };
  std::vector<ProfRec> prof_rec;                 // one per recorded launch (same order as prof_ev)
  struct ProfKernel { std::string name; double ms, flops; long long n; };
  std::vector<ProfKernel> prof_kernels;          // filled by conan_profile_end: per template instantiation
  void launch_group(const ConvGroup& g, int nprob, int cfg, hipStream_t st);
  bool launch_rb(const cnk::RBArgs& a, int C, hipStream_t st, const TRef* ymean = nullptr);   // true: the launch stored the branch mean (merged)
  void launch_rp(const cnk::RPArgs& a, hipStream_t st);
  cnk::RowConvTune rc_tune() const { return {sw.rc_noksplit, sw.rc_wide_min}; }
  bool rowconv_ok(const PackedConv& pc, int dil, int T) const { return sw.rowconv && pc.wf && cnk::rowconv_supported(pc.Cin, pc.k, dil, T); }
  cnk::RowConvArgs mk_rc(const PackedConv& pc, const TRef& x, const TRef& y, int n, int T, int dil = 1) const;
  void rowconv(const cnk::RowConvArgs& a, hipStream_t st);
  template <typename F> void profiled(const std::string& name, double flops, hipStream_t st, F&& launch);
  void conv(const ConvArgs& a, hipStream_t st) { ConvGroup g; g.p[0] = a; launch_group(g, 1, pick_cfg(plan_n(a.n) * a.T, a.Cout, 1), st); }
  ConvArgs mk(const PackedConv& pc, const TRef& x, const TRef& y, int n, int T, const int* pos, int dil = 1, int pad_left = -1) const;

  // --- decoder megakernel (decoder_mega.hip): the decoder step's operator list, recorded once per (slot count, frames,
  // buffer set) and replayed as one persistent launch
  struct DecExtra { float* mel_out2 = nullptr; int* codes_dst = nullptr; const int* codes_src = nullptr; int codes_words = 0;
                    const float* f0_in = nullptr; const float* uv_in = nullptr;         // the caller's contour (conan_decoder_step_pitch)
                    const float* trk_f0 = nullptr; const float* trk_uv = nullptr; };    // the tracked contour of a wav-in step (f0.hip)
  struct MegaProgram {
    long long key[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool ok = false;
    int nops = 0, groups = 0, group_size = 0, njobs = 0, kw4 = 0, lds_bytes = 0, barriers = 0, n = 0, T = 0;
    int lds_need = 0;                  // what the operators need (lds_bytes may be padded: xcd mode, blocking steps)
    bool xcd = false;                  // a single row tile: the launch's workgroups on ONE XCD form the group (decoder_mega.hip)
    double flops = 0.0;
    cnk::MegaOp* dev = nullptr;        // device copy (capacity kMegaMaxOps)
    cnk::MegaOp* pinned = nullptr;     // host staging of this entry; reused only after `copied` has fired
    hipEvent_t copied = nullptr;
    long long stamp = 0;               // least-recently-used replacement
  };
  static constexpr int kMegaMaxOps = cnk::kMegaMaxOps, kMegaEntries = 12;
  std::vector<MegaProgram> mega_cache;
  long long mega_clock = 0;
  bool use_mega = true;                          // sw.dec_mega, and no CU-masked front-end stream (sw.front_custride)
  int mega_grid = 128;                           // plan::mega_grid: sw.mega_grid clamped to the CU count
  int mega_ffn_gs = 8;                           // members of a fused feed-forward while a program is recorded (run_mega)
  unsigned* mega_bar = nullptr;                  // the grid barrier's arrival counter (counts for ever); the group counters follow it, 16 words apart
  unsigned mega_bar_count = 0;                   // its value once every launch enqueued so far has finished
  unsigned* mega_x = nullptr;                    // xcd mode: election word, rank counter, "decided" counter, barrier flags (decoder_mega.hip)
  unsigned mega_gseq = 0;                        // multi-tile launches so far (epochs of their groups' flag barriers)
  unsigned mega_xseq = 0, mega_xdec = 0;         // launches in xcd mode so far (24 bits), the decided counter's value once they have all finished
  int opt_flags = 0;                             // conan_streams_opts.flags
  bool mega_single = true;                       // single-tile steps take the persistent launch (xcd mode); CONAN_STREAMS_SEPARATE_SMALL_STEPS: separate launches
  unsigned long long* mega_dbg = nullptr;        // sw.mega_stamps: per-operator clock stamps of the last launch (printed at destruction)
  int mega_dbg_prog = -1;                        // index into mega_cache (the vector may reallocate)
  std::vector<cnk::MegaOp>* mega_rec = nullptr;  // != nullptr: decoder_ops() records its operators instead of launching them
  bool mega_rec_ok = true; int mega_rec_lds = 0; double mega_rec_flops = 0.0;
  void mega_push(cnk::MegaOp& op, int lds_floats);
  bool run_mega(int n, int T, const int32_t* codes, float* mel_out, const DecExtra& ex, hipStream_t st);
  void launch_mega(MegaProgram& e, hipStream_t st);
  void decoder_ops(int n, int frames, const int32_t* codes, float* mel_out, const conan_decoder_taps& taps, hipStream_t st, const DecExtra& ex);
  void op_embed(const cnk::EmbedArgs& a, hipStream_t st);
  void op_ln(const cnk::LNArgs& a, hipStream_t st);
  void op_xattn(const cnk::XAttnArgs& a, hipStream_t st);
  void op_pitch(const cnk::PitchHeadArgs& a, hipStream_t st);
  void op_advance(int* pos, int n, int delta, hipStream_t st);

  void hifigan_step(int n, int frames, const float* mel_dev, float* wav_out_dev, float* pre_tanh, hipStream_t st, const conan_hifigan_taps* taps = nullptr,
                    const OutPlan* op = nullptr);
  void emformer_step(int n, const float* chunk, float* out, float* logits, int32_t* codes, hipStream_t st);
  void decoder_step(int n, int frames, const int32_t* codes, float* mel_out, const conan_decoder_taps& taps, hipStream_t st, const DecExtra* extra = nullptr);
  void set_reference(const int32_t* slots, int n, const float* ref, const int32_t* ref_len, int max_len, hipStream_t st);
  // The style pass behind conan_set_reference, writing entries index[i] of `dst`: this stream-set's own slots (own: the index list goes
  // through set_slots, `batch` references per pass) or a voice bank's entries (conan_voices_enroll: batch 1).
  void style_pass(const voice::Cache& dst, bool own, const int32_t* index, int n, int batch, const float* ref, const int32_t* ref_len, int max_len, hipStream_t st);
  void conv_blocks_noncausal(const std::string& name, int nblocks, int k, int C, Lin* x, Lin& ln, Lin& h, Lin& blkm, const TRef& npm,
                             const int* lens, int n, int T, int& cur, hipStream_t st);
};

// every launch of the matrix kernels goes through here: between conan_profile_begin / _end it is bracketed by HIP
// events on its launch stream and booked under the kernel's name with its algorithmic FLOPs
static_assert(kActSets == 2 * conan_streams::NP, "the activity sets cover the pipeline's depth");
template <typename F>
inline void conan_streams::profiled(const std::string& name, double flops, hipStream_t st, F&& launch) {
  if (!prof_on) { launch(); return; }
  if (prof_used == prof_ev.size()) {
    hipEvent_t a, b;
    HIP_CHECK(hipEventCreate(&a)); HIP_CHECK(hipEventCreate(&b));
    prof_ev.push_back({a, b});
  }
  auto& ev = prof_ev[prof_used++];
  HIP_CHECK(hipEventRecord(ev.first, st));
  launch();
  HIP_CHECK(hipEventRecord(ev.second, st));
  prof_flops += flops;
  prof_launches += 1;
  prof_rec.push_back({name, flops});
}

// ---- the chunk step's stages (api.hip), shared by the mel-in entry points and the wav-in steps (wavio.hip)
void check_chunk_step(const conan_streams* s, const char* who);
// trk_f0 / trk_uv (may be null): the step's tracked contour [n][seg], for its rows whose slot follows (f0.hip)
void step_blocking(conan_streams* s, int n, int emit, const float* mel_chunk_dev, int32_t* codes_dev, float* mel_out_dev, float* wav_out_dev,
                   hipStream_t st, const conan_streams::OutPlan& op, const float* trk_f0 = nullptr, const float* trk_uv = nullptr);
void step_pipelined(conan_streams* s, const int32_t* slots, int n, int emit, const float* mel_chunk_dev, int32_t* codes_dev, float* mel_out_dev,
                    float* wav_out_dev, void* stream, const std::function<void(hipStream_t)>& pre, const conan_streams::OutPlan& op,
                    const float* trk_f0 = nullptr, const float* trk_uv = nullptr);

// ---- the wav-in step and its call stages (wavio.hip: step_wav).  One slot's front-end plan for a call that gives it `samples` (model
// rate) and `final_`.  Centred framing: frame f needs the samples up to f * hop + n_fft / 2 - 1, or the final call: every frame of
// 1 + samples / hop, zero padding past the end.  R = samples received after the call, total = R once final (-1 before); frames [0, fc)
// complete, [f0, f0 + nnew) of them new in this call; chunk t = chunks emitted so far starts at frame pos and is ready once frames
// [pos, pos + seg + rc) are complete or - after the final call - any frame is left (emit frames, rows [0, real) backed by frames: the
// short last chunks of engine.chunks, repeat-last padding).
struct FePlan { long long R, total; int fc, f0, nnew, pos, emit, real; };
// What step_wav has worked out before its features plan their part.  groups: the call rows per emit group, largest emit first; a row's
// place in the groups in this order is its chunk row (as fe_chunk's).  rs_q: the resampler's staging set, once step_wav has taken it.
struct WavCall {
  const int32_t* slots; int n;
  const std::vector<FePlan>& pl;
  const std::vector<std::vector<int>>& groups;
  int seg, hop, N;
  const conan_mel_cfg& mel;
  const std::string& who;
  bool rs_launch; const int32_t* samples;      // the resampler's plan: it launches in this call; per row the samples the front-end gets
  bool common; const float* wav_dev; long long wav_ld;
  int rs_q = 0;
  bool pre_staged = false;      // the equaliser writes the staging in this call: a leveller behind it works in place, as behind a resampler launch
  template <typename F> void each_group(F&& f) const {      // f(g, the group's first chunk row)
    for (int g = 0, off = 0; g < (int)groups.size(); off += (int)groups[g].size(), ++g) f(g, off);
  }
  template <typename F> void each_chunk_row(F&& f) const {      // f(g, k, call row, chunk row): row k of group g
    each_group([&](int g, int off) { for (int k = 0; k < (int)groups[g].size(); ++k) f(g, k, groups[g][k], off + k); });
  }
  // one table row per emitting call row in chunk-row order: fill(g, call row, chunk row, r) writes the row of a slot with the feature
  // (-> true); any other slot gets the row that holds its place (mode 0, slot -1, state_row -1)
  template <typename Row, typename F> std::vector<Row> table_rows(F&& fill) const {
    std::vector<Row> rows;
    each_chunk_row([&](int g, int, int i, int at) {
      Row r;
      if (!fill(g, i, at, r)) { memset(&r, 0, sizeof(r)); r.slot = -1; r.state_row = -1; }
      rows.push_back(r);
    });
    return rows;
  }
};
// The front-end work of a wav-in call: at most one entry per position, run in this order on one stream (the caller's, or as
// step_pipelined's `pre`).  The ...End entries record the events of the sets the mel front-end launch is the last to read.
enum FrontPos { kFrResample, kFrEq, kFrLevel, kFrMel, kFrDenoise, kFrLevelEnd, kFrResampleEnd, kFrF0, kFrRegister, kFrActivity, kFrBypass, kFrComfort, kFrTones, kFrCount };
struct FrontWork {
  std::function<void(hipStream_t)> at[kFrCount];
  void run(hipStream_t st) const { for (const auto& f : at) if (f) f(st); }
};
// Each feature of the wav-in step has a per-call WavStage in its own file (level::, f0:: with reg::'s rows, act::, byp::, comfort::, denoise::), all of one
// shape, called by step_wav in that order:
//   plan      the call's host rows, per-group flags and FLOPs; throws on anything refused.  const with respect to the stream-set and
//             run for every feature before any staging set is taken or any state changes: a refused call leaves everything as it was
//   enqueue   takes the staging set on the caller's stream cst (sets.begin), adds the feature's launch to the front-end work and hands
//             the groups' rows of table and staging to their vocoder steps' OutPlans
//   commit    records the set's event where the front-end work does not (dec / last: the streams of the call's last decoder and vocoder
//             step), clears pending for the rows that carried a restart and stores `last`
// The body of the conan_step_wav_* hooks: zero the caller's [n][seg] rows, then each LastRow's emitted words from the staging of its
// set (src_ld words per chunk row, the first at src_off)
template <typename T>
inline void copy_last_rows(const std::vector<LastRow>& last, T* dst_dev, int n, int seg, T* const* staging, int src_ld, int src_off, hipStream_t st) {
  HIP_CHECK(hipMemsetAsync(dst_dev, 0, (size_t)n * seg * sizeof(T), st));
  for (const LastRow& r : last)
    HIP_CHECK(hipMemcpyAsync(dst_dev + (size_t)r.row * seg, staging[r.set] + (size_t)r.src * src_ld + src_off, (size_t)r.emit * sizeof(T), hipMemcpyDeviceToDevice, st));
}

// ---- waveform I/O host layer (wavio.hip): the bodies of api.hip's wav-in steps, rate / stride / format setters and output queries
namespace wavio {
// What the feature setters share behind their null and cfg checks, in this order: the streaming front-end, the slot list, the early
// return (false) of a call that turns off what the stream-set never had, then enter() (rows in flight were built from the old setting)
bool begin_setter(conan_streams* s, const int32_t* slots, int n, bool enabling, bool allocated, const char* who, void* stream);
// a feature's getter (zeros where the stream-set never enabled it).  front_end_who: the entry point of a feature that needs the
// streaming front-end (null: one that does not)
template <typename Set, typename Cfg>
void get_setting(const conan_streams* s, Set conan_streams::*set, int slot, Cfg* out, const char* front_end_who) {
  if (!s || !out) throw Error(CONAN_ERR_INVALID, "null argument");
  if (slot < 0 || slot >= s->max_slots) throw Error(CONAN_ERR_INVALID, "slot index out of range");
  if (front_end_who && !s->wav_in.fe_audio) throw Error(CONAN_ERR_STATE, std::string(front_end_who) + ": the stream-set has no streaming front-end (all three models)");
  (s->*set).get(slot, out);
}
hipStream_t begin_last_call(conan_streams* s, const char* who, void* stream);      // the conan_step_wav_* hooks: the no-call-yet check, enter()
int bytes_per_sample(int fmt);      // of a CONAN_SAMPLE_* / cnk::kFmt* code
void check_format(int format, const char* who);
void check_slot_list(const conan_streams* s, const int32_t* slots, int n);      // count, range, duplicates
void check_utterance_start(const conan_streams* s, const int32_t* slots, int n, const char* who);
const ch::RsTable* rate_table(conan_streams* s, const conan_resample_cfg& c, const char* who);      // null at the model rate
void store_format(std::vector<unsigned char>& fmt, int& not_f32, const int32_t* slots, int n, int format);
void step_wav(conan_streams* s, const std::string& who, const int32_t* slots, int n, const int32_t* in_samples, const int32_t* in_final, const float* wav_dev,
              long long wav_ld, const conan_mel_cfg* mel, int32_t* codes_dev, float* mel_out_dev, float* wav_out_dev, int32_t* emit_out, void* stream,
              bool pipelined, bool common);
void step_wav_common(conan_streams* s, const int32_t* slots, int n, int samples, int final, const float* wav_dev, const conan_mel_cfg* mel,
                     int32_t* codes_dev, float* mel_out_dev, float* wav_out_dev, int32_t* emit_out, void* stream, bool pipelined);
void step_wav_chunk(conan_streams* s, float* chunk_dev, void* stream);
void set_input_rate(conan_streams* s, const int32_t* slots, int n, const conan_resample_cfg* cfg);
void set_output_rate(conan_streams* s, const int32_t* slots, int n, const conan_resample_cfg* cfg);
void set_drift(conan_streams* s, int side, const int32_t* slots, int n, const conan_resample_cfg* cfg, const int32_t* ppb);      // side: CONAN_DRIFT_*
void get_drift(conan_streams* s, int side, const int32_t* slots, int n, int32_t* ppb_out, int64_t* in_out, int64_t* out_out);
void set_output_ld(conan_streams* s, int64_t ld);
void set_input_format(conan_streams* s, const int32_t* slots, int n, int format);
void set_output_format(conan_streams* s, const int32_t* slots, int n, int format);
int output_samples(conan_streams* s, int32_t* counts, int cap);      // -> rows of the most recent step call
void output_pending(conan_streams* s, const int32_t* slots, int n, int32_t* counts);
void flush_output(conan_streams* s, const int32_t* slots, int n, float* wav_out_dev, int64_t wav_ld, void* stream);
}  // namespace wavio

// The state query of a RecordSetting (conan_streams_<name>_state): a slot about to restart reports the fresh record - zeros, and what
// fresh(slot, dst, st) writes over them - any other its record, in the order of `stream`
template <typename R, typename Fresh>
void record_state(conan_streams* s, R conan_streams::*set, const char* name, const int32_t* slots, int n, void* rows_dev, int64_t ld, void* stream, Fresh&& fresh) {
  if (!s || !slots || !rows_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  R::check_rows("conan_streams_", name, "_state", rows_dev, ld);
  wavio::check_slot_list(s, slots, n);
  R& r = s->*set;
  for (int i = 0; i < n; ++i)
    if (!r.on(slots[i])) throw Error(CONAN_ERR_STATE, std::string("conan_streams_") + name + "_state: slot " + std::to_string(slots[i]) + " has the feature off (conan_streams_set_" + name + ")");
  hipStream_t st = s->enter(stream);
  for (int i = 0; i < n; ++i) {
    char* dst = static_cast<char*>(rows_dev) + (size_t)i * ld;
    if (r.pending[slots[i]]) {
      HIP_CHECK(hipMemsetAsync(dst, 0, R::kRecBytes, st));
      fresh(slots[i], dst, st);
    } else {
      HIP_CHECK(hipMemcpyAsync(dst, r.record(slots[i]), R::kRecBytes, hipMemcpyDeviceToDevice, st));
    }
  }
}
inline void fresh_zeros(int, char*, hipStream_t) {}      // the fresh record of a feature that restarts from zeros

// ---- input leveller (level.hip): the kernel's host side and the bodies of api.hip's entry points
namespace level {
void check_common(const conan_streams* s, const int32_t* slots, int n, const std::string& who);      // conan_step_wav: one configuration per call
void set_input_level(conan_streams* s, const int32_t* slots, int n, const conan_level_cfg* cfg);
void input_level(conan_streams* s, const int32_t* slots, int n, double* stats_dev, void* stream);
// The levelled slots that hand their front-end samples this call.  Behind a resampler launch the kernel works in place on the staged
// rows; in a call without one (stages) it reads the caller's rows and writes the staging itself - step_wav takes the resampler's set
// for it - so the call's unlevelled rows with samples ride along as copy rows and the front-end still finds every row in one place.
struct WavStage {
  std::vector<cnk::LvRow> rows;
  bool stages = false;
  void plan(const conan_streams* s, const WavCall& c);
  void enqueue(conan_streams* s, const WavCall& c, hipStream_t cst, FrontWork& front, std::vector<conan_streams::OutPlan>& ops);
  void commit(conan_streams*, hipStream_t, hipStream_t) {}      // (no host state; the set's event rides in the front-end work)
};
}  // namespace level

// ---- slot snapshots (snapshot.hip): the bodies of api.hip's export / import entry points
namespace snapshot {
uint64_t layout_id(conan_streams* s);
int64_t row_bytes(conan_streams* s);
void export_slots(conan_streams* s, const int32_t* slots, int n, void* blob_dev, int64_t blob_ld, conan_slot_meta* meta, void* stream);
void import_slots(conan_streams* s, const int32_t* slots, int n, const void* blob_dev, int64_t blob_ld, const conan_slot_meta* meta, void* stream);
void meta_info(const conan_slot_meta* meta, conan_slot_info* out);
int meta_level(const conan_slot_meta* meta, conan_level_cfg* out);      // 1: the record carries a leveller
int meta_pitch(const conan_slot_meta* meta, conan_pitch_cfg* out);      // 1: the record carries a pitch control
}  // namespace snapshot

// ---- voice bank (voices.hip): the bodies of api.hip's entry points
namespace voices {
void create(conan_ctx* ctx, int capacity, int max_ref_frames, conan_voices** out);
void destroy(conan_voices* v);
void enroll(conan_voices* v, conan_streams* via, const int32_t* ids, int n, const float* ref_mel_dev, const int32_t* ref_len, int max_len, void* stream);
void remove(conan_voices* v, const int32_t* ids, int n);
void info(const conan_voices* v, int id, conan_voice_info* out);
void set_voice(conan_streams* s, const int32_t* slots, int n, const conan_voices* v, const int32_t* voice_ids, const float* weights, int k, bool mix, void* stream);
void get_voice(const conan_streams* s, int slot, int32_t* voice_id);
int64_t blob_bytes(const conan_voices* v);
void export_voices(conan_voices* v, const int32_t* ids, int n, void* blob_dev, int64_t blob_ld, conan_voice_meta* meta, void* stream);
void import_voices(conan_voices* v, const int32_t* ids, int n, const void* blob_dev, int64_t blob_ld, const conan_voice_meta* meta, void* stream);
void meta_info(const conan_voice_meta* meta, conan_voice_info* out);
}  // namespace voices

// ---- source-pitch following (f0.hip): the tracker's host side and the bodies of api.hip's entry points
namespace f0 {
struct Lags { int tmin, tmax; };
Lags lags(const conan_f0_cfg& c, double sr);
void check_cfg(const conan_f0_cfg& c, double sr, int n_fft, const char* who);      // host only
cnk::F0Row row(const conan_f0_cfg& c, double sr);      // the cfg's fields of a kernel row
void whole(conan_ctx* ctx, const conan_mel_cfg* mel, const conan_f0_cfg* cfg, const float* wav_dev, int n, int samples, float* f0_out_dev, float* uv_out_dev,
           int32_t* frames_out, void* stream);
void set_follow(conan_streams* s, const int32_t* slots, int n, const conan_f0_cfg* cfg, void* stream);
void contour(conan_streams* s, float* f0_dev, float* uv_dev, void* stream);
// The following slots that emit have their chunk's frames tracked, from their audio rings, into the call's contour rows; every such
// row whose slot has the register on also gets a register row (reg::wav_row), launched directly behind the tracker.
struct WavStage {
  std::vector<cnk::F0Row> rows;
  std::vector<cnk::RegRow> reg_rows;
  std::vector<LastRow> last;
  std::vector<char> group;      // per emit group: a row of it follows (empty: none does)
  int jobs = 0, q = 0;
  double flops = 0.0;
  const float* ct_f0 = nullptr; const float* ct_uv = nullptr;      // the call's contour set (enqueue)
  // the contour rows of group g, whose first chunk row is off (null: no row of it follows, and the group's decoder keeps its program)
  const float* trk_f0(int g, int off, int seg) const { return !group.empty() && group[g] ? ct_f0 + (size_t)off * seg : nullptr; }
  const float* trk_uv(int g, int off, int seg) const { return !group.empty() && group[g] ? ct_uv + (size_t)off * seg : nullptr; }
  void plan(const conan_streams* s, const WavCall& c);
  void enqueue(conan_streams* s, const WavCall& c, hipStream_t cst, FrontWork& front, std::vector<conan_streams::OutPlan>& ops);
  void commit(conan_streams* s, hipStream_t dec, hipStream_t last_st);
};
}  // namespace f0

// ---- register matching (register.hip): the kernel's host side and the bodies of api.hip's entry points
namespace reg {
void check_cfg(const conan_register_cfg& c, const char* who);      // host only
cnk::RegRow row(const conan_register_cfg& c);      // the cfg's fields of a kernel row that starts from the seed and names no slot
void whole(conan_ctx* ctx, const conan_register_cfg* cfg, const float* f0_dev, const float* uv_dev, int n, const int32_t* frames, int64_t ld,
           float* f0_out_dev, int64_t* state_out_dev, void* stream);
void set_register(conan_streams* s, const int32_t* slots, int n, const conan_register_cfg* cfg, void* stream);
void state(conan_streams* s, const int32_t* slots, int n, int64_t* state_dev, void* stream);
// the register's part of f0::WavStage: the row that rewrites `nframes` frames at `off` of the call's contour, carrying the slot's
// pending restart; the launch behind the tracker's with its set's event; the restarts the rows carried
cnk::RegRow wav_row(const conan_streams* s, int slot, long long off, int nframes);
void wav_enqueue(conan_streams* s, const std::vector<cnk::RegRow>& rows, int contour_set, hipStream_t cst, FrontWork& front);
void wav_commit(conan_streams* s, const std::vector<cnk::RegRow>& rows);
}  // namespace reg

// ---- source activity (activity.hip): the kernels' host side and the bodies of api.hip's entry points
namespace act {
void check_cfg(const conan_activity_cfg& c, const char* who);      // host only
void check_mel(const conan_mel_cfg& m, const char* who);           // host only: the frame geometry conan_activity accepts
cnk::ActRow row(const conan_activity_cfg& c);      // the cfg's fields of a detector row that starts from the seed and names no slot
void whole(conan_ctx* ctx, const conan_mel_cfg* mel, const conan_activity_cfg* cfg, const float* wav_dev, int n, int samples, int32_t* act_out_dev,
           int32_t* level_out_dev, double* power_out_dev, conan_activity_state* state_out_dev, int32_t* frames_out, void* stream);
void gate(conan_ctx* ctx, int hop, const float* wav_dev, int n, int64_t samples, int64_t ld, const int32_t* level_dev, int64_t level_ld, int32_t start_level,
          float* out_dev, void* stream);
void set_activity(conan_streams* s, const int32_t* slots, int n, const conan_activity_cfg* cfg, void* stream);
void state(conan_streams* s, const int32_t* slots, int n, conan_activity_state* state_dev, void* stream);
void last_call(conan_streams* s, int32_t* act_dev, int32_t* level_dev, void* stream);
// A call in which a slot with the detector emits has one table row per emitting call row (WavCall::table_rows), so that a group's
// gate finds its rows by their place; the groups with a gated row take their rows of the table and of the level staging along.
struct WavStage {
  std::vector<cnk::ActRow> rows;
  std::vector<LastRow> last;
  std::vector<char> gate;       // per emit group: a row of it is gated (empty: no table)
  int q = 0;
  double* power = nullptr;      // the call's power staging (comfort::WavStage::take: a row of the call follows), in the flags' row layout
  void plan(const conan_streams* s, const WavCall& c);
  void enqueue(conan_streams* s, const WavCall& c, hipStream_t cst, FrontWork& front, std::vector<conan_streams::OutPlan>& ops);
  void commit(conan_streams* s, hipStream_t dec, hipStream_t last_st);
};
}  // namespace act

// ---- source bypass (bypass.hip): the kernels' host side and the bodies of api.hip's entry points
namespace byp {
void check_cfg(const conan_bypass_cfg& c, const char* who);      // host only
cnk::BypRow row(const conan_bypass_cfg& c);      // the cfg's fields of a stage row that starts from the seed and names no slot
void mix(conan_ctx* ctx, int hop, const float* wet_dev, int64_t wet_ld, const float* dry_dev, int64_t dry_ld, int n, int64_t samples, const int32_t* wet_lvl_dev,
         const int32_t* dry_lvl_dev, int64_t lvl_ld, int32_t start_wet, int32_t start_dry, float* out_dev, int64_t out_ld, void* stream);
void set_bypass(conan_streams* s, const int32_t* slots, int n, const conan_bypass_cfg* cfg, void* stream);
void state(conan_streams* s, const int32_t* slots, int n, conan_bypass_state* state_dev, void* stream);
void last_call(conan_streams* s, int32_t* wet_lvl_dev, int32_t* dry_lvl_dev, void* stream);
// As the activity table: one row per emitting call row in a call in which a slot with the feature emits; the stage kernel runs
// behind the detector, whose levels of the same call a filling row reads (gate_stage: the call's activity stage, enqueued before);
// the groups with a bypass row take their rows of table, levels and dry samples along.
struct WavStage {
  std::vector<cnk::BypRow> rows;
  std::vector<LastRow> last;
  std::vector<char> mix;        // per emit group: a row of it mixes (empty: no table)
  bool fill = false;            // a row fills from the gate's levels
  int q = 0;
  const act::WavStage* gate_stage = nullptr;
  void plan(const conan_streams* s, const WavCall& c);
  void enqueue(conan_streams* s, const WavCall& c, hipStream_t cst, FrontWork& front, std::vector<conan_streams::OutPlan>& ops);
  void commit(conan_streams* s, hipStream_t dec, hipStream_t last_st);
};
}  // namespace byp

// ---- comfort noise (comfort.hip): the kernels' host side and the bodies of api.hip's entry points
namespace comfort {
void check_cfg(const conan_comfort_cfg& c, const char* who);      // host only
cnk::CmfRow row(const conan_comfort_cfg& c);      // the cfg's fields of a tracker row that starts from the seed and names no slot
void track(conan_ctx* ctx, const conan_comfort_cfg* cfg, const int32_t* act_dev, const double* power_dev, int n, int64_t frames, int64_t ld,
           int32_t* level_out_dev, conan_comfort_state* state_out_dev, void* stream);
void fill(conan_ctx* ctx, int hop, const conan_comfort_cfg* cfg, const uint64_t* seeds, const float* wav_dev, int64_t ld, int n, int64_t samples, int64_t pos0,
          const int32_t* gate_lvl_dev, const int32_t* comfort_lvl_dev, int64_t lvl_ld, int32_t start_gate_level, int32_t start_comfort_level, float* out_dev,
          int64_t out_ld, void* stream);
void set_comfort(conan_streams* s, const int32_t* slots, int n, const conan_comfort_cfg* cfg, void* stream);
void state(conan_streams* s, const int32_t* slots, int n, conan_comfort_state* state_dev, void* stream);
void last_call(conan_streams* s, int32_t* level_dev, void* stream);
// As the activity table, and with its rows: one row per emitting call row in a call in which a slot with the feature and a detector
// emits.  take() runs in front of the detector's enqueue: it takes the staging set and returns the power staging the detector is to
// write (null: no row of the call follows).  The tracker runs behind the detector (gate_stage: the call's activity stage) and the
// bypass's stage; the groups with a filled row take their rows of table, levels and gate levels along.
struct WavStage {
  std::vector<cnk::CmfRow> rows;
  std::vector<LastRow> last;
  std::vector<char> fill;       // per emit group: a row of it is filled (empty: no table)
  bool follows = false;         // a row reads the detector's powers
  int q = 0;
  const act::WavStage* gate_stage = nullptr;
  void plan(const conan_streams* s, const WavCall& c);
  double* take(conan_streams* s, hipStream_t cst);
  void enqueue(conan_streams* s, const WavCall& c, hipStream_t cst, FrontWork& front, std::vector<conan_streams::OutPlan>& ops);
  void commit(conan_streams* s, hipStream_t dec, hipStream_t last_st);
};
}  // namespace comfort

// ---- signalling tones (tone.hip): the kernels' host side and the bodies of api.hip's entry points
namespace tone {
void check_cfg(const conan_tone_cfg& c, const char* who);      // host only
void check_rate(int hop, const char* who);                     // host only: CONAN_ERR_UNSUPPORTED outside the table's range
std::vector<short> host_table(int M);                          // host only
const short* table(conan_ctx* ctx, int M);                     // the context's device copy, built on first use per rate
cnk::ToneRow row(const conan_tone_cfg& c);      // the cfg's fields of a detector row that starts from the seed and names no slot
void table_out(int sample_rate, int16_t* out);
void whole(conan_ctx* ctx, int hop, const conan_tone_cfg* cfg, const float* wav_dev, int64_t ld, int n, const int64_t* samples, const conan_tone_state* seed_dev,
           int32_t* digit_dev, int32_t* sound_dev, int32_t* level_dev, int64_t out_ld, conan_tone_state* state_out_dev, int64_t* frames_out, void* stream);
void fill(conan_ctx* ctx, int hop, const conan_tone_cfg* cfg, const float* wav_dev, int64_t ld, int n, int64_t samples, const int64_t* pos0, const int32_t* sound_dev,
          const int32_t* level_dev, int64_t lvl_ld, int32_t start_level, int32_t start_sound, float* out_dev, int64_t out_ld, void* stream);
void set_tones(conan_streams* s, const int32_t* slots, int n, const conan_tone_cfg* cfg, void* stream);
void state(conan_streams* s, const int32_t* slots, int n, conan_tone_state* state_dev, void* stream);
void last_call(conan_streams* s, int32_t* digit_dev, int32_t* sound_dev, int32_t* level_dev, void* stream);
// As the activity table: one row per emitting call row in a call in which a slot with the feature emits.  The detector runs behind
// the front-end launch; the groups with a mode-2 row take their rows of table, sounds and levels along to their vocoder steps.
struct WavStage {
  std::vector<cnk::ToneRow> rows;
  std::vector<LastRow> last;
  std::vector<char> fill;       // per emit group: a row of it regenerates (empty: no table)
  int q = 0;
  void plan(const conan_streams* s, const WavCall& c);
  void enqueue(conan_streams* s, const WavCall& c, hipStream_t cst, FrontWork& front, std::vector<conan_streams::OutPlan>& ops);
  void commit(conan_streams* s, hipStream_t dec, hipStream_t last_st);
};
}  // namespace tone

// ---- input loss concealment (conceal.hip): the kernel's host side and the bodies of api.hip's entry points
namespace conc {
void check_cfg(const conan_conceal_cfg& c, const char* who);      // host only
cnk::ConcRow row(const conan_conceal_cfg& c);      // the cfg's fields of a row that starts from zeros and names no slot
void whole(conan_ctx* ctx, const conan_conceal_cfg* cfg, int format, void* x_dev, int64_t ld, int n, const int64_t* samples, const int32_t* lost_dev,
           int64_t lost_ld, void* stream);
void set_conceal(conan_streams* s, const int32_t* slots, int n, const conan_conceal_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream);
void repair(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, void* wav_dev, int64_t wav_ld, const int32_t* lost_dev, int64_t lost_ld,
            void* stream);
void state(conan_streams* s, const int32_t* slots, int n, void* state_dev, int64_t ld, void* stream);
}  // namespace conc

// ---- echo cancellation (echo.hip): the kernel's host side and the bodies of api.hip's entry points
namespace echo {
void check_cfg(const conan_echo_cfg& c, const char* who);      // host only
cnk::EchoRow row(const conan_echo_cfg& c);      // the cfg's fields of a row that starts from the restart state and names no slot
void whole(conan_ctx* ctx, const conan_echo_cfg* cfg, int format, void* x_dev, int64_t ld, const void* far_dev, int64_t far_ld, int n, const int64_t* samples,
           int64_t* stats_dev, void* stream);
void set_echo(conan_streams* s, const int32_t* slots, int n, const conan_echo_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream);
void cancel(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, void* wav_dev, int64_t wav_ld, const void* far_dev, int64_t far_ld,
            int64_t* stats_dev, void* stream);
void state(conan_streams* s, const int32_t* slots, int n, void* state_dev, int64_t ld, void* stream);
}  // namespace echo

// ---- echo delay (echo_delay.hip): the kernel's host side and the bodies of api.hip's entry points
namespace echo_delay {
void check_cfg(const conan_echo_delay_cfg& c, const char* who);      // host only
cnk::EdRow row(const conan_echo_delay_cfg& c);      // the cfg's fields of a row that starts from the restart state and names no slot
void whole(conan_ctx* ctx, const conan_echo_delay_cfg* cfg, int format, const void* mic_dev, int64_t ld, const void* far_dev, int64_t far_ld, int n,
           const int64_t* samples, int64_t* track_dev, int64_t track_ld, int64_t* report_dev, void* stream);
void set_echo_delay(conan_streams* s, const int32_t* slots, int n, const conan_echo_delay_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream);
void estimate(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, const void* wav_dev, int64_t wav_ld, const void* far_dev, int64_t far_ld,
              int64_t* report_dev, void* stream);
void state(conan_streams* s, const int32_t* slots, int n, void* state_dev, int64_t ld, void* stream);
}  // namespace echo_delay

// ---- input noise suppression (denoise.hip): the kernels' host side and the bodies of api.hip's entry points
namespace denoise {
void check_cfg(const conan_denoise_cfg& c, const char* who);      // host only
cnk::DnRow row(const conan_denoise_cfg& c);      // the cfg's fields of a row that starts before its first frame and names no slot
void whole(conan_ctx* ctx, const conan_denoise_cfg* cfg, const float* mel_dev, int n, const int32_t* frames, int64_t ld, int num_mels,
           const conan_denoise_state* seed_dev, float* out_dev, conan_denoise_state* state_out_dev, void* stream);
void set_denoise(conan_streams* s, const int32_t* slots, int n, const conan_denoise_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream);
void state(conan_streams* s, const int32_t* slots, int n, void* rows_dev, int64_t ld, void* stream);
// The suppressing slots that complete a frame or emit get one table row each; the launch sits directly behind the mel front-end's
// (kFrDenoise) and records its set's event itself.
struct WavStage {
  std::vector<cnk::DnRow> rows;
  void plan(const conan_streams* s, const WavCall& c);
  void enqueue(conan_streams* s, const WavCall& c, hipStream_t cst, FrontWork& front, std::vector<conan_streams::OutPlan>& ops);
  void commit(conan_streams* s, hipStream_t dec, hipStream_t last_st);
};
}  // namespace denoise

// ---- output leveller (level_out.hip): the kernels' host side and the bodies of api.hip's entry points
namespace olv {
// the table rows of a vocoder step that gives each of `slots` `frames` frames (empty: no levelled slot among them);
// CONAN_ERR_UNSUPPORTED for a levelled row the split form does not cover.  Nothing changes.
std::vector<cnk::OlRow> step_rows(const conan_streams* s, const int32_t* slots, int n, int frames, const std::string& who);
void set_level(conan_streams* s, const int32_t* slots, int n, const conan_level_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream);
void stats(conan_streams* s, const int32_t* slots, int n, double* stats_dev, void* stream);
int64_t state_bytes(const conan_streams* s);
void state(conan_streams* s, const int32_t* slots, int n, void* state_dev, int64_t ld, void* stream);
}  // namespace olv

// ---- output watermark (watermark.hip): the kernels' host side and the bodies of api.hip's entry points
namespace wmark {
void check_cfg(const conan_watermark_cfg& c, const char* who);      // host only
cnk::WmRow row(const conan_watermark_cfg& c);      // the cfg's fields of a row that starts from {0, 0} and names no slot
// the table rows of a vocoder step that gives each of `slots` `frames` frames (empty: no marked slot among them).  Nothing changes.
std::vector<cnk::WmRow> step_rows(const conan_streams* s, const int32_t* slots, int n, int frames, const std::string& who);
void embed(conan_ctx* ctx, const conan_watermark_cfg* cfg, const float* x_dev, int n, const int64_t* samples, int64_t ld, const conan_watermark_state* seed_dev,
           float* out_dev, conan_watermark_state* state_out_dev, void* stream);
void detect(conan_ctx* ctx, uint64_t key, int format, const void* x_dev, int64_t ld, int n, const int64_t* samples, int64_t* score_dev, int64_t* soft_dev,
            int64_t soft_ld, conan_watermark_hit* hit_dev, void* stream);
void decide(const int64_t* score, const int64_t* soft, const conan_watermark_hit* hit, double threshold, conan_watermark_result* out);      // host only
void set_watermark(conan_streams* s, const int32_t* slots, int n, const conan_watermark_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream);
void state(conan_streams* s, const int32_t* slots, int n, void* rows_dev, int64_t ld, void* stream);
}  // namespace wmark

// ---- equaliser (eq.hip): the kernel's host side and the bodies of api.hip's entry points
namespace eq {
void check_cfg(const conan_eq_cfg& c, const char* who);      // host only
void sections(const conan_eq_cfg& c, cnk::EqSec* out);       // host only: out[kEqMaxSec], the coefficients and the transition matrices
void design(int kind, double rate, double f0, double q, double gain_db, double* out);      // host only
void whole(conan_ctx* ctx, const conan_eq_cfg* cfg, const float* x_dev, int64_t x_ld, int n, const int64_t* samples, float* y_dev, int64_t y_ld,
           conan_eq_state* state_out_dev, const conan_eq_state* seed_dev, void* stream);
// the two sides' setters, getters and state queries (output = false: the source side)
void set_eq(conan_streams* s, bool output, const int32_t* slots, int n, const conan_eq_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream);
void get_eq(const conan_streams* s, bool output, int slot, conan_eq_cfg* cfg_out);
void state(conan_streams* s, bool output, const int32_t* slots, int n, void* rows_dev, int64_t ld, void* stream);
// the table rows of a vocoder step that gives each of `slots` `frames` frames (empty: no filtered slot among them).  Nothing changes.
std::vector<cnk::EqRow> step_rows(const conan_streams* s, const int32_t* slots, int n, int frames, const std::string& who);
// hifigan_step's part: the row table travels ahead of the step's kernels (step_begin -> the set q), the launch sits behind conv_post
int step_begin(conan_streams* s, const std::vector<cnk::EqRow>& rows, hipStream_t st);
void step_launch(conan_streams* s, const std::vector<cnk::EqRow>& rows, int q, float* wav, long long ld, hipStream_t st);
// The filtered slots that hand their front-end samples this call, in front of the leveller.  Behind a resampler launch the kernel
// works in place on the staged rows; in a call without one (stages) it reads the caller's rows and writes the staging itself -
// step_wav takes the resampler's set for it - and the call's other rows with samples ride along as copy rows.
struct WavStage {
  std::vector<cnk::EqRow> rows;
  bool stages = false;
  void plan(const conan_streams* s, const WavCall& c);
  void enqueue(conan_streams* s, const WavCall& c, hipStream_t cst, FrontWork& front, std::vector<conan_streams::OutPlan>& ops);
  void commit(conan_streams* s, hipStream_t dec, hipStream_t last_st);
};
}  // namespace eq

// ---- silence trimming (trim.hip): the kernels' host side and the body of api.hip's entry point
namespace trim {
void check_cfg(const conan_trim_cfg& c, const char* who);      // host only
void detector_rows(const conan_activity_cfg& cfg, const int64_t* lens, int n, int hop, int64_t ld, int64_t frame_ld, cnk::ActRow* rows);      // host only
void check_args(const conan_ctx* ctx, const conan_mel_cfg* mel, const conan_activity_cfg* act_cfg, const conan_trim_cfg* cfg, const float* wav_dev, int64_t ld,
                int n, int64_t samples, const int64_t* lengths, const int32_t* act_in_dev, int64_t act_ld, const float* out_dev, int64_t out_ld,
                const int32_t* mask_out_dev, const int64_t* offset_out_dev, int64_t frame_ld);      // host only
void whole(conan_ctx* ctx, const conan_mel_cfg* mel, const conan_activity_cfg* act_cfg, const conan_trim_cfg* cfg, const float* wav_dev, int64_t ld, int n,
           int64_t samples, const int64_t* lengths, const int32_t* act_in_dev, int64_t act_ld, float* out_dev, int64_t out_ld, int32_t* mask_out_dev,
           int64_t* offset_out_dev, int64_t frame_ld, int64_t* out_len_dev, void* stream);
}  // namespace trim

// ---- per-slot pitch control (pitch.hip): the bodies of api.hip's entry points
namespace pitch {
void check_cfg(const conan_pitch_cfg& c, const char* who);      // host only
void set_pitch(conan_streams* s, const int32_t* slots, int n, const conan_pitch_cfg* cfg, void* stream);
void get_pitch(const conan_streams* s, int slot, conan_pitch_cfg* out);
}  // namespace pitch
