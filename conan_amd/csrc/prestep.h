// The pre-step row features (conceal.hip, echo.hip, echo_delay.hip): kernels that work on the caller's device rows in front of a wav-in
// step call, one table row per call row with samples.  Their entry points - the whole-signal call conan_<name>, the setter
// conan_streams_set_<name> with its seed rows, the per-call conan_streams_<name> - have one shape, written here once; a feature's file
// keeps its cfg check, its row, its kernel, its *_init() call and a traits struct F that says what is its own:
//   Cfg, Row, Args        the published cfg, the kernel's table row (samples, row, slot, restart, fmt; with kBlock also pos, phase) and arguments
//   Call                  the entry points' buffers: wav / wav_ld (the rows worked on, stride in dwords), aux / aux_ld (the second
//                         buffer, never null where a row runs) and, with kReport, report - plus whatever only the feature reads
//   kName                 "conceal" of conan_conceal_state_bytes; kWhole, kSet, kCall: the three entry points' names
//   kAux, kReportArg      the second buffer's name in the header ("lost": lost_dev, lost_ld) and the report's ("stats_dev")
//   kKernel               the kernel's name in a profile
//   kAuxAudio             aux holds audio rows as wav does: 4-byte aligned, and a row's bytes fit its stride
//   kReport               int64 words per call row of `report` (0: the feature reports nothing)
//   kBlock                the rows carry the slot's position and phase = pos % kBlock (0: neither)
//   set                   the stream-set's RecordSetting (with kBlock: and its pos)
//   check_cfg, row, launch
//   check_call(c), check_row(cfg, samples, c)      the feature's own checks of the buffers and of a row that runs: null, or what is
//                         wrong as a literal
//   fill(a, c)            the buffers' part of the kernel's arguments
// Every text of a refusal is built where it is thrown (refuse): a call that passes builds no string.
#pragma once
#include "streams.h"

namespace prestep {

constexpr int64_t kMaxSamples = 1ll << 40, kMaxStride = 1ll << 40;
inline bool stride_ok(int64_t ld) { return ld >= 0 && ld <= kMaxStride; }

// CONAN_ERR_INVALID "<entry point>: [<unit> <index>: ]<what>"
[[noreturn]] inline void refuse(const char* who, const std::string& what, const char* unit = nullptr, int index = 0) {
  throw Error(CONAN_ERR_INVALID, std::string(who) + ": " + (unit ? std::string(unit) + " " + std::to_string(index) + ": " : std::string()) + what);
}

template <typename F, typename Call>
inline bool row_fits(long long bytes, const Call& c) { return bytes <= c.wav_ld * 4 && (!F::kAuxAudio || bytes <= c.aux_ld * 4); }
// what both entry points check of the buffers; rows_ld: the rows' stride as the entry point names it ("ld" / "wav_ld")
template <typename F, typename Call>
inline void check_strides(const char* who, const Call& c, const char* rows_ld) {
  if (!stride_ok(c.wav_ld) || !stride_ok(c.aux_ld)) refuse(who, std::string(rows_ld) + " and " + F::kAux + "_ld must be in 0 .. 2^40");
}
template <typename F, typename Call>
inline void check_aligned(const char* who, const Call& c) {
  if (((uintptr_t)c.wav & 3) || (F::kAuxAudio && ((uintptr_t)c.aux & 3)))
    refuse(who, std::string("the rows' buffer") + (F::kAuxAudio ? std::string(" and ") + F::kAux + "_dev" : std::string()) + " must be 4-byte aligned");
}
template <typename F, typename Call>
inline void check_report(const char* who, const Call& c) {
  if constexpr (F::kReport > 0)
    if ((uintptr_t)c.report & 7) refuse(who, std::string(F::kReportArg) + " must be 8-byte aligned");
}
// a call that runs fewer than its n rows reports zeros for the others
template <typename F, typename Call>
inline void zero_report(const Call& c, int n, hipStream_t st) {
  if constexpr (F::kReport > 0)
    if (c.report) HIP_CHECK(hipMemsetAsync(c.report, 0, (size_t)n * F::kReport * sizeof(int64_t), st));
}

// conan_<name>: n whole signals with one cfg, from the restart state; no stream-set, the table goes through the context's workspace
template <typename F>
void whole(conan_ctx* ctx, const typename F::Cfg* cfg, int format, const typename F::Call& c, int n, const int64_t* samples, void* stream) {
  using Row = typename F::Row;
  if (!ctx || !cfg || !c.wav || !c.aux || !samples) throw Error(CONAN_ERR_INVALID, "null argument");
  F::check_cfg(*cfg, F::kWhole);
  if (!cfg->enabled) refuse(F::kWhole, "cfg.enabled must be 1");
  wavio::check_format(format, F::kWhole);
  if (n < 1 || n > 65535) refuse(F::kWhole, "n must be in 1 .. 65535");
  check_strides<F>(F::kWhole, c, "ld");
  check_aligned<F>(F::kWhole, c);
  check_report<F>(F::kWhole, c);
  if (const char* bad = F::check_call(c)) refuse(F::kWhole, bad);
  const int bps = wavio::bytes_per_sample(format);
  for (int i = 0; i < n; ++i) {
    if (samples[i] < 0 || samples[i] > kMaxSamples) refuse(F::kWhole, "samples must be in 0 .. 2^40", "row", i);
    if (!row_fits<F>(samples[i] * bps, c)) refuse(F::kWhole, "the row holds more bytes than a row stride (x 4 bytes)", "row", i);
    if (const char* bad = F::check_row(*cfg, samples[i], c)) refuse(F::kWhole, bad, "row", i);
  }
  HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t table = (size_t)n * sizeof(Row);
  Row* h = static_cast<Row*>(ctx->loud_stage.take(table));
  const Row proto = F::row(*cfg);
  int rows = 0;
  for (int i = 0; i < n; ++i) {
    if (samples[i] < 1) continue;
    h[rows] = proto;
    h[rows].samples = samples[i]; h[rows].row = i; h[rows].fmt = format;
    ++rows;
  }
  if (rows < n) zero_report<F>(c, n, st);
  if (rows < 1) return;
  char* ws = reinterpret_cast<char*>(ctx->workspace((table + 3) / sizeof(float), st));
  HIP_CHECK(hipMemcpyAsync(ws, h, (size_t)rows * sizeof(Row), hipMemcpyHostToDevice, st));
  ctx->loud_stage.sent(st);
  typename F::Args a;
  memset(&a, 0, sizeof(a));
  F::fill(a, c);
  a.state = nullptr; a.tab = reinterpret_cast<const Row*>(ws); a.rows = rows;
  F::launch(a, st);
  HIP_CHECK(hipGetLastError());
}

// conan_streams_set_<name> up to the point where something changes: nulls, the cfg, the seed rows, then what every feature setter
// shares (wavio::begin_setter; false: the call turns off what the stream-set never had).  The caller goes on with its *_init().
template <typename F>
bool begin_set(conan_streams* s, const int32_t* slots, int n, const typename F::Cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream) {
  if (!s || !slots || !cfg) throw Error(CONAN_ERR_INVALID, "null argument");
  F::check_cfg(*cfg, F::kSet);      // (before the handle is touched, before any GPU use)
  if (seed_dev) std::remove_reference_t<decltype(s->*F::set)>::check_rows("conan_streams_set_", F::kName, "", seed_dev, seed_ld);
  return wavio::begin_setter(s, slots, n, cfg->enabled != 0, (s->*F::set).allocated(), F::kSet, stream);
}

// The host, not the record, tells a kBlock kernel where in a block a slot stands: the positions of the seeds a setter has just copied
// are read back (each record's first int64), which takes a synchronisation
template <typename F>
void read_seed_pos(conan_streams* s, const int32_t* slots, int n, const void* seed_dev, int64_t seed_ld, hipStream_t st) {
  std::vector<long long> pos((size_t)n);
  for (int i = 0; i < n; ++i)
    HIP_CHECK(hipMemcpyAsync(&pos[i], static_cast<const char*>(seed_dev) + (size_t)i * seed_ld, sizeof(long long), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  for (int i = 0; i < n; ++i) (s->*F::set).pos[slots[i]] = pos[i] < 0 ? 0 : pos[i];      // (a record the kernel cannot have written: any position serves)
}

// conan_streams_<name>: row i of the buffers belongs to slots[i] and brings samples[i] samples in the slot's input format.  A row whose
// slot has the feature off, or that brings nothing, keeps its bytes; no row to run: no launch.  Nothing changes before the last check.
template <typename F>
void call(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, const typename F::Call& c, void* stream) {
  using Row = typename F::Row;
  if (!s || !slots || !samples) throw Error(CONAN_ERR_INVALID, "null argument");
  wavio::check_slot_list(s, slots, n);
  check_strides<F>(F::kCall, c, "wav_ld");
  check_report<F>(F::kCall, c);
  auto& f = s->*F::set;
  std::vector<Row> rows;
  for (int i = 0; i < n; ++i) {
    const int slot = slots[i];
    if (samples[i] < 0) refuse(F::kCall, "samples must be >= 0");
    if (!f.on(slot) || samples[i] == 0) continue;
    const int fmt = s->wav_in.in_fmt[slot];
    if (!row_fits<F>((long long)samples[i] * wavio::bytes_per_sample(fmt), c)) refuse(F::kCall, "the row holds more bytes than a row stride (x 4 bytes)", "slot", slot);
    if (const char* bad = F::check_row(f.cfg[slot], samples[i], c)) refuse(F::kCall, bad, "slot", slot);
    Row r = F::row(f.cfg[slot]);
    r.samples = samples[i]; r.row = i; r.slot = slot; r.restart = f.pending[slot]; r.fmt = fmt;
    if constexpr (F::kBlock > 0) {
      r.pos = r.restart ? 0 : f.pos[slot];
      r.phase = (int)(r.pos % F::kBlock);
    }
    rows.push_back(r);
  }
  hipStream_t st = (hipStream_t)stream;
  if constexpr (F::kReport > 0)
    if (c.report && (int)rows.size() < n && n > 0) {
      HIP_CHECK(hipSetDevice(s->ctx->device));
      zero_report<F>(c, n, st);
    }
  if (rows.empty()) return;
  if (!c.wav || !c.aux) throw Error(CONAN_ERR_INVALID, std::string("null argument (wav_dev / ") + F::kAux + "_dev with a row to run)");
  check_aligned<F>(F::kCall, c);
  HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
  const int q = f.sets.begin(rows.data(), (int)rows.size(), st);
  typename F::Args a;
  memset(&a, 0, sizeof(a));
  F::fill(a, c);
  a.state = f.state; a.tab = f.sets.rows[q]; a.rows = (int)rows.size();
  s->profiled(F::kKernel, 0.0, st, [&] { F::launch(a, st); });
  HIP_CHECK(hipGetLastError());
  f.sets.end(q, st);
  for (const Row& r : rows) {
    f.pending[r.slot] = 0;
    if constexpr (F::kBlock > 0) f.pos[r.slot] = r.pos + r.samples;
  }
}

}  // namespace prestep
