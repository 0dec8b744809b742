// Host layer of waveform I/O: the wav-in chunk steps (conan_step_wav*), per-slot input / output sample rates and formats, the output
// stride and the output queries.  Host code only: the kernels are resample.hip, frontend.hip and misc_kernels.hip; the extern "C"
// entry points are api.hip's.
#include <climits>

#include "streams.h"

namespace wavio {

int bytes_per_sample(int fmt) { return fmt == cnk::kFmtF32 ? 4 : (fmt == cnk::kFmtS16 ? 2 : 1); }

// the filter fields of a call row (cnk::RsRow, cnk::RsOutRow)
template <typename Row>
static void fill_filter(Row& row, const ch::RsTable& t) {
  row.taps = t.f.taps; row.ph = t.f.ph; row.orig = t.f.orig; row.nph = t.f.nph; row.w = t.f.w; row.L = t.f.L;
}

// the inputs still to be read ([first tap of output `out`, I), up to a rounding step) must fit the history ring
static bool ring_fits(const ch::RsTable& t, long long I, long long out, long long ring_len) { return I - (t.first(out) - 4) <= ring_len; }

// The filter table of a rate setter's configuration; null at the model rate, where the configuration must still be a valid one.
const ch::RsTable* rate_table(conan_streams* s, const conan_resample_cfg& c, const char* who) {
  if (c.in_rate != c.out_rate) return &s->ctx->resample_table(c);
  conan_resample_cfg probe = c;
  if (conan_resample_length(&probe, 0) < 0) throw Error(CONAN_ERR_INVALID, std::string(who) + ": invalid resampler configuration");
  return nullptr;
}

void check_slot_list(const conan_streams* s, const int32_t* slots, int n) {
  if (n < 1 || n > s->max_slots) throw Error(CONAN_ERR_INVALID, "slot count out of range");
  std::vector<char> seen(s->max_slots, 0);
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] >= s->max_slots) throw Error(CONAN_ERR_INVALID, "slot index out of range");
    if (seen[slots[i]]) throw Error(CONAN_ERR_INVALID, "duplicate slot");
    seen[slots[i]] = 1;
  }
}

void check_format(int format, const char* who) {
  if (format != CONAN_SAMPLE_F32 && format != CONAN_SAMPLE_S16 && format != CONAN_SAMPLE_ULAW && format != CONAN_SAMPLE_ALAW)
    throw Error(CONAN_ERR_INVALID, std::string(who) + ": format must be CONAN_SAMPLE_F32, _S16, _ULAW or _ALAW");
}
static_assert(CONAN_SAMPLE_F32 == cnk::kFmtF32 && CONAN_SAMPLE_S16 == cnk::kFmtS16 && CONAN_SAMPLE_ULAW == cnk::kFmtUlaw && CONAN_SAMPLE_ALAW == cnk::kFmtAlaw,
              "the kernels' format codes are the header's");

// a setter of what the front-end's input goes through: every listed slot is at the start of an utterance
void check_utterance_start(const conan_streams* s, const int32_t* slots, int n, const char* who) {
  for (int i = 0; i < n; ++i) {
    const conan_streams::FeSlot& o = s->wav_in.fe_slot[slots[i]];
    const bool rs_fresh = s->wav_in.rs_slot.empty() || (s->wav_in.rs_slot[slots[i]].in == 0 && s->wav_in.rs_slot[slots[i]].phase == 0);
    if (o.recv != 0 || o.phase != 0 || o.frames != 0 || o.chunks != 0 || !rs_fresh)
      throw Error(CONAN_ERR_STATE, std::string(who) + ": slot " + std::to_string(slots[i]) + " is not at the start of an utterance (reset it with CONAN_MODEL_FRONTEND first)");
  }
}

bool begin_setter(conan_streams* s, const int32_t* slots, int n, bool enabling, bool allocated, const char* who, void* stream) {
  if (!s->wav_in.fe_audio) throw Error(CONAN_ERR_STATE, std::string(who) + ": the stream-set has no streaming front-end (all three models)");
  check_slot_list(s, slots, n);
  if (!enabling && !allocated) return false;
  s->enter(stream);
  return true;
}

hipStream_t begin_last_call(conan_streams* s, const char* who, void* stream) {
  if (!s->wav_in.fe_chunk || s->wav_in.fe_last_n == 0) throw Error(CONAN_ERR_STATE, std::string(who) + ": no conan_step_wav call yet");
  return s->enter(stream);
}

// Input resampler of a wav-in call (conan_streams_set_input_rate).  Per call row: the model-rate samples and final flag the front-end
// gets - a row without a rate passes its own; a row with one hands over the longest prefix of outputs whose last tap has arrived (at
// most seg * hop; after the input's final call, what is left, seg * hop at a time, final on the call that delivers the last sample).
// When a row with a rate has input or owed output, or a row with a sample format (conan_streams_set_input_format) has input, one
// resample_stream_kernel launch writes every row's model-rate samples to staging (rows without a rate decoded and copied) and the
// front-end reads them there.  rs_plan checks every row and changes nothing.
struct RsPlan {
  std::vector<int32_t> mm, ff;          // per row: front-end samples and final flag
  std::vector<char> rate;               // per row: the slot has a rate
  std::vector<long long> in_after;      // per row with a rate: input samples received after the call
  std::vector<cnk::RsRow> rows;
  bool launch = false;
  int tiles = 1, win = 0;
  double flops = 0;
};

static RsPlan rs_plan(const conan_streams* s, const int32_t* slots, int n, const int32_t* samples, const int32_t* final_, const float* wav_dev,
                      long long wav_ld, const conan_mel_cfg& m, const char* who) {
  RsPlan P;
  P.mm.assign(samples, samples + n); P.ff.assign(final_, final_ + n); P.rate.assign(n, 0); P.in_after.assign(n, 0);
  if (s->wav_in.rs_slot.empty()) return P;      // (neither a rate nor a format was ever set: the caller's rows go to the front-end as they are)
  const int S = s->ctx->cfg.emf_segment * s->ctx->hop;
  P.rows.resize(n);
  for (int i = 0; i < n; ++i) {
    const conan_streams::RsSlot& r = s->wav_in.rs_slot[slots[i]];
    cnk::RsRow& row = P.rows[i];
    memset(&row, 0, sizeof(row));
    const int fmt = s->wav_in.in_fmt[slots[i]], bps = bytes_per_sample(fmt);
    row.slot = slots[i]; row.mode = cnk::kRsCopy | (fmt << cnk::kRsFmtShift); row.m = samples[i]; row.h = samples[i];
    if (fmt != cnk::kFmtF32 && samples[i] > 0) {
      if ((long long)samples[i] * bps > wav_ld * 4)
        throw Error(CONAN_ERR_INVALID, std::string(who) + ": slot " + std::to_string(slots[i]) + ": the row holds more bytes (" + std::to_string(samples[i]) + " samples of " +
                                           std::to_string(bps) + ") than the row stride of wav_dev (" + std::to_string(wav_ld) + " x 4 bytes)");
      if (!wav_dev) throw Error(CONAN_ERR_INVALID, "null argument (wav_dev with samples > 0)");
      if ((uintptr_t)wav_dev & 3) throw Error(CONAN_ERR_INVALID, std::string(who) + ": wav_dev must be 4-byte aligned");
      if (!r.f) P.launch = true;      // a format alone: the copy rows decode into staging
    }
    if (r.dr.d) {      // a drift slot (conan_streams_set_input_drift): the counts come from the law's closed-form positions
      const ch::DriftPos& D = r.dr;
      auto bad = [&](const std::string& what) {
        throw Error(CONAN_ERR_INVALID, std::string(who) + ": slot " + std::to_string(slots[i]) + " (input at " + std::to_string(D.d->in_rate) + " Hz with drift): " + what);
      };
      const int sm = samples[i], fin = final_[i], W = D.d->W;
      if (fin != 0 && fin != 1) bad("final must be 0 or 1");
      if (m.sample_rate != D.d->out_rate) bad("conan_mel_cfg.sample_rate must be the resampler's out_rate");
      if (r.phase == 1 && (!fin || sm != 0)) bad("after the final call only samples = 0, final = 1 may follow");
      if (sm < 0 || sm > 2 * r.s_in) bad("a call takes 0 .. 2 * segment * hop * in_rate / out_rate samples");
      if ((long long)sm * bps > wav_ld * 4) bad("the row holds more samples than the row stride of wav_dev");
      if (sm > 0 && !wav_dev) throw Error(CONAN_ERR_INVALID, "null argument (wav_dev with samples > 0)");
      const long long I = r.in + sm;
      const long long T = std::max(D.first_at(fin ? I : I - W), r.out);      // outputs that exist (final) or are ready
      const long long J = std::min(T, r.out + S);
      P.ff[i] = fin && J == T;
      const ch::DriftPos::u128 p0 = D.pos(r.out);
      const long long n_first = (long long)(p0 >> 32);
      if (I - std::max(0ll, n_first - W + 1) > cnk::kRsRing)
        throw Error(CONAN_ERR_UNSUPPORTED, std::string(who) + ": slot " + std::to_string(slots[i]) + ": unread input history would leave the resampler's ring (the slot is owed too much output)");
      P.mm[i] = (int)(J - r.out);
      P.rate[i] = 1; P.in_after[i] = I;
      row.taps = reinterpret_cast<const float*>(D.d->dev); row.ph = reinterpret_cast<const int*>((uintptr_t)D.step);
      row.in0 = r.in; row.out0 = n_first; row.orig = (int)(unsigned)p0; row.w = W;
      row.m = sm; row.h = P.mm[i]; row.mode = cnk::kRsDrift | (fmt << cnk::kRsFmtShift);
      P.launch = P.launch || sm > 0 || P.mm[i] > 0;
      P.win = std::max(P.win, D.win);
      P.flops += 8.0 * P.mm[i] * W;
      continue;
    }
    if (!r.f) continue;
    const ch::RsTable& t = *r.f;
    auto bad = [&](const std::string& what) {
      throw Error(CONAN_ERR_INVALID, std::string(who) + ": slot " + std::to_string(slots[i]) + " (input at " + std::to_string(t.in_rate) + " Hz): " + what);
    };
    const int sm = samples[i], fin = final_[i];
    const int s_in = (int)((long long)S * t.in_rate / t.out_rate);
    if (fin != 0 && fin != 1) bad("final must be 0 or 1");
    if (m.sample_rate != t.out_rate) bad("conan_mel_cfg.sample_rate must be the resampler's out_rate");
    if (r.phase == 1 && (!fin || sm != 0)) bad("after the final call only samples = 0, final = 1 may follow");
    if (!fin && sm != s_in) bad("a non-final call takes exactly segment * hop * in_rate / out_rate samples");
    if (fin && (sm < 0 || sm > s_in)) bad("a final call takes 0 .. segment * hop * in_rate / out_rate samples");
    if ((long long)sm * bps > wav_ld * 4) bad("the row holds more samples than the row stride of wav_dev");
    if (sm > 0 && !wav_dev) throw Error(CONAN_ERR_INVALID, "null argument (wav_dev with samples > 0)");
    const long long I = r.in + sm;
    long long J;
    if (fin) {
      const long long T = t.length(I);
      J = std::min(T, r.out + S);
      P.ff[i] = J == T;
    } else {
      J = std::min(std::max(t.ready(I), r.out), r.out + S);
      P.ff[i] = 0;
    }
    if (!ring_fits(t, I, r.out, cnk::kRsRing)) throw Error(CONAN_ERR_UNSUPPORTED, std::string(who) + ": resampler history ring too small for this configuration");
    P.mm[i] = (int)(J - r.out);
    P.rate[i] = 1; P.in_after[i] = I;
    fill_filter(row, t);
    row.in0 = r.in; row.out0 = r.out; row.m = sm; row.h = P.mm[i]; row.mode = fmt << cnk::kRsFmtShift;
    P.launch = P.launch || sm > 0 || P.mm[i] > 0;
    P.win = std::max(P.win, t.win);
    P.flops += 2.0 * P.mm[i] * t.f.L;
  }
  if (P.launch)
    for (int i = 0; i < n; ++i) {
      const cnk::RsRow& row = P.rows[i];
      P.tiles = std::max(P.tiles, (std::max(row.h, row.m) + cnk::kRsTile - 1) / cnk::kRsTile);
    }
  return P;
}

// The launch of the plan whose rows went to set q of rs_sets (begin), first of the call's front-end work
static void rs_enqueue(conan_streams* s, const RsPlan& P, int n, int q, const float* wav_dev, long long wav_ld, long long out_ld, FrontWork& front) {
  cnk::ResampleStreamArgs a;
  a.wav = wav_dev ? wav_dev : s->wav_in.rs_wav[q]; a.wav_ld = wav_dev ? wav_ld : 0;
  a.ring = s->wav_in.rs_ring; a.out = s->wav_in.rs_wav[q]; a.out_ld = out_ld;
  a.rows = s->wav_in.rs_sets.rows[q]; a.n = n; a.tiles = P.tiles; a.win = P.win;
  front.at[kFrResample] = [s, a, flops = P.flops](hipStream_t st) { s->profiled("resample_stream_kernel", flops, st, [&] { cnk::launch_resample_stream(a, st); }); };
}

static void rs_commit(conan_streams* s, const int32_t* slots, int n, const RsPlan& P, const int32_t* final_) {
  for (int i = 0; i < n; ++i) {
    if (!P.rate[i]) continue;
    conan_streams::RsSlot& r = s->wav_in.rs_slot[slots[i]];
    r.in = P.in_after[i]; r.out += P.mm[i];
    if (final_[i]) r.phase = 1;
  }
}

// The conan_mel_cfg of a wav-in call: centred frames at the vocoder's hop into the Emformer's input width.
static void check_mel_stream(const conan_streams* s, const conan_mel_cfg& m, const std::string& who) {
  if (m.framing != 0) throw Error(CONAN_ERR_INVALID, who + ": only framing 0 (centred frames, zero padding) streams");
  if (m.fft_size < 64 || (m.fft_size & (m.fft_size - 1)) || m.fft_size > 2048) throw Error(CONAN_ERR_INVALID, who + ": fft_size must be a power of two in [64, 2048]");
  if (m.hop_size != s->ctx->hop) throw Error(CONAN_ERR_INVALID, who + ": hop_size must be the vocoder's hop (conan_hop_size)");
  if (m.num_mels != s->ctx->cfg.emf_input_dim) throw Error(CONAN_ERR_INVALID, who + ": num_mels must be the Emformer's input width");
  if (m.natural_log != 0 && m.natural_log != 1) throw Error(CONAN_ERR_INVALID, who + ": natural_log must be 0 (log10) or 1 (ln)");
  if (m.win_length < 1 || m.win_length > m.fft_size || m.sample_rate < 1 || !(m.eps > 0.f) || !(m.mag_eps >= 0.f))
    throw Error(CONAN_ERR_INVALID, "mel front-end configuration");
}

// One slot's front-end plan (FePlan, streams.h) for a wav-in call that gives it `samples` (model rate) and `final_`; nothing changes.
static FePlan fe_plan(const conan_streams* s, const conan_streams::FeSlot& o, int samples, int final_, int n_fft, const std::string& who) {
  const int seg = s->ctx->cfg.emf_segment, rc = s->ctx->cfg.emf_right_context, hop = s->ctx->hop, N = n_fft;
  FePlan p;
  p.R = o.recv + samples;
  p.total = final_ ? p.R : -1;
  p.fc = final_ ? (int)(1 + p.R / hop) : (p.R >= N / 2 ? (int)((p.R - N / 2) / hop) + 1 : 0);
  p.f0 = o.frames; p.nnew = std::max(0, p.fc - p.f0); p.pos = o.chunks * seg;
  p.emit = 0; p.real = 0;
  if (final_) {
    if (p.pos < p.fc) { p.emit = std::min(seg, p.fc - p.pos); p.real = p.emit + std::min(rc, p.fc - p.pos - p.emit); }
  } else if (p.pos + seg + rc <= p.fc) {
    p.emit = seg; p.real = seg + rc;
  }
  // ring spans: the samples a new frame reads and the samples appended; the frames a chunk row reads and the frames written
  const long long a_lo = std::min<long long>(o.recv, (long long)p.f0 * hop - N / 2);
  if (p.R - std::max(0ll, a_lo) > s->wav_in.fe_LA || p.fc - std::min(p.pos, p.f0) > s->wav_in.fe_LM)
    throw Error(CONAN_ERR_UNSUPPORTED, who + ": front-end rings too small for this configuration");
  return p;
}

static void fe_commit(conan_streams* s, const int32_t* slots, int n, const std::vector<FePlan>& pl, const int32_t* final_) {
  for (int i = 0; i < n; ++i) {
    conan_streams::FeSlot& o = s->wav_in.fe_slot[slots[i]];
    const FePlan& p = pl[i];
    o.recv = p.R; o.frames = std::max(p.f0, p.fc); o.chunks += p.emit > 0 ? 1 : 0;
    o.phase = final_[i] ? (p.emit > 0 ? 1 : 2) : 0;
  }
}

// Waveform-in chunk steps (conan_step_wav[_async], conan_step_wav_ragged[_ld][_async]).  The host keeps each slot's position in its
// utterance (FeSlot); every slot gets its own plan (fe_plan), and the emitting slots are grouped by emit, each group running one
// mel-in chunk step (blocking or pipelined) on its own slot list.  One front-end launch, in front of the first group's Emformer, does
// the front-end work of every slot of the call: the new frames, the chunk rows of earlier calls from the mel ring, the samples
// appended to the audio ring.
// `common` is conan_step_wav's contract: every slot at the same position with the same input-rate configuration, so the call has at
// most one group, in call order, and the outputs are rows of emit frames ([n][emit]) written in place.  Its front-end is
// mel_stream_kernel on the call's one plan (mel_stream_copy_kernel in calls that complete no frame), the same-position kernel: at 64
// streams a pipelined step is ~10 % slower with the row-table kernel below (1.548 against 1.402 ms per step).
// Otherwise (ragged calls) mel_stream_ragged_kernel is driven by a [n][kRaggedWords] row table and writes each group's chunk
// contiguously into fe_chunk; the outputs are rows of a full chunk ([n][seg]).  A call whose slots all emit a full chunk is one group
// in call order and writes the caller's buffers directly; the groups of any other call write staging (set q of rg_sets) and
// wav_rows_scatter_kernel puts the rows in call order.
// The per-slot source features take part through their WavStage (streams.h): every plan() before anything changes, enqueue() into the
// front-end work in front of the group steps, commit() behind them.
void step_wav(conan_streams* s, const std::string& who, const int32_t* slots, int n, const int32_t* in_samples, const int32_t* in_final, const float* wav_dev,
              long long wav_ld, const conan_mel_cfg* mel, int32_t* codes_dev, float* mel_out_dev, float* wav_out_dev, int32_t* emit_out, void* stream,
              bool pipelined, bool common) {
  if (!s || !slots || !in_samples || !in_final || !mel || !wav_out_dev || !emit_out) throw Error(CONAN_ERR_INVALID, "null argument");
  check_chunk_step(s, who.c_str());
  const conan_mel_cfg& m = *mel;
  check_mel_stream(s, m, who);
  if (n < 1 || n > s->max_slots) throw Error(CONAN_ERR_INVALID, "slot count out of range");
  if (pipelined && s->prof_on) throw Error(CONAN_ERR_STATE, "profiling is not available for pipelined steps");
  const conan_cfg& c = s->ctx->cfg;
  const int seg = c.emf_segment, rc = c.emf_right_context, hop = m.hop_size, N = m.fft_size, rows = seg + rc;
  check_slot_list(s, slots, n);
  if (wav_ld < 0 || wav_ld > INT_MAX) throw Error(CONAN_ERR_INVALID, who + ": wav_ld out of range");
  if (common) {
    const conan_streams::FeSlot& o0 = s->wav_in.fe_slot[slots[0]];
    for (int i = 1; i < n; ++i) {
      const conan_streams::FeSlot& o = s->wav_in.fe_slot[slots[i]];
      if (o.recv != o0.recv || o.frames != o0.frames || o.chunks != o0.chunks || o.phase != o0.phase)
        throw Error(CONAN_ERR_INVALID, who + ": the slots of one call must be at the same position of their utterances");
    }
    for (int i = 1; i < n && !s->wav_in.rs_slot.empty(); ++i) {
      const conan_streams::RsSlot &r0 = s->wav_in.rs_slot[slots[0]], &r = s->wav_in.rs_slot[slots[i]];
      const ch::DriftPos &d0 = r0.dr, &d = r.dr;
      if (d.d != d0.d || (d.d && (d.ppb != d0.ppb || d.out0 != d0.out0 || d.n0 != d0.n0 || d.f0 != d0.f0 || r.in != r0.in || r.out != r0.out || r.phase != r0.phase)))
        throw Error(CONAN_ERR_INVALID, who + ": the slots of one call must share one input drift configuration (conan_streams_set_input_drift), ppb and position");
      if (r.f != r0.f || (r.f && (r.in != r0.in || r.out != r0.out || r.phase != r0.phase)))
        throw Error(CONAN_ERR_INVALID, who + ": the slots of one call must share one input rate configuration (conan_streams_set_input_rate) and position");
    }
    level::check_common(s, slots, n, who);
  }
  // the input resampler's rows first: what each slot's front-end gets this call
  const RsPlan P = rs_plan(s, slots, n, in_samples, in_final, wav_dev, wav_ld, m, who.c_str());
  const int32_t* samples = P.mm.data();
  const int32_t* final_ = P.ff.data();
  // every slot's plan first: nothing changes before all of them have passed
  std::vector<FePlan> pl(n);
  bool run = false;
  for (int i = 0; i < n; ++i) {
    const conan_streams::FeSlot& o = s->wav_in.fe_slot[slots[i]];
    const int sm = samples[i], fin = final_[i];
    auto bad = [&](const char* what) {
      throw Error(CONAN_ERR_INVALID, who + ": slot " + std::to_string(slots[i]) + " (call row " + std::to_string(i) + "): " + what);
    };
    if (fin != 0 && fin != 1) bad("final must be 0 or 1");
    if (o.phase == 2) bad("the utterance has been drained; reset the slot with CONAN_MODEL_FRONTEND first");
    if (o.phase == 1 && (!fin || sm != 0)) bad("after the final call only samples = 0, final = 1 may follow");
    if (!fin && sm != seg * hop && !P.rate[i]) bad("a non-final call takes exactly segment * hop samples per slot");
    if (fin && (sm < 0 || sm > seg * hop)) bad("a final call takes 0 .. segment * hop samples per slot");
    if (sm > wav_ld && !P.rate[i] && !s->wav_in.in_fmt[slots[i]]) bad("the row holds more samples than the row stride of wav_dev");
    if (in_samples[i] > 0 && !wav_dev) throw Error(CONAN_ERR_INVALID, "null argument (wav_dev with samples > 0)");
    if (fin && o.recv + sm < 1) bad("an utterance needs at least one sample");
    pl[i] = fe_plan(s, o, sm, fin, N, who);
    run = run || pl[i].nnew > 0 || sm > 0 || pl[i].emit > 0;
  }
  // emit groups, largest emit first; a group's rows keep call order
  std::vector<std::vector<int>> groups;      // call rows per group
  for (int e = seg; e >= 1; --e) {
    std::vector<int> g;
    for (int i = 0; i < n; ++i) if (pl[i].emit == e) g.push_back(i);
    if (!g.empty()) groups.push_back(std::move(g));
  }
  const bool direct = common || (groups.size() == 1 && (int)groups[0].size() == n && pl[0].emit == seg);
  const bool scatter = !direct && !groups.empty();
  // the groups' output rows (out_plan): a staged call with an output rate among its emitting rows, or any stride set (a group
  // of emit < seg frames then differs from it even at seg * hop), has resample_out_kernel write each group's audio straight to
  // its call-order rows of wav_out_dev (the scatter then places codes and mel only); otherwise no group's plan is active
  bool route = scatter && s->wav_out.out_ld != 0;
  for (int g = 0; scatter && g < (int)groups.size(); ++g)
    for (int i : groups[g]) route = route || (!s->wav_out.or_slot.empty() && s->wav_out.or_slot[slots[i]].rated()) || s->wav_out.out_fmt[slots[i]];
  std::vector<conan_streams::OutPlan> ops;
  std::vector<std::vector<int32_t>> gslots(groups.size());
  for (int g = 0; g < (int)groups.size(); ++g) {
    std::vector<int32_t>& gs = gslots[g];
    for (int i : groups[g]) gs.push_back(slots[i]);
    const int e = pl[groups[g][0]].emit;
    ops.push_back(s->out_plan(gs.data(), (int)gs.size(), e, wav_out_dev, route ? (long long)seg * hop : (long long)e * hop, route ? &groups[g] : nullptr, who));
  }
  // the features' part of the call, each in its own file, in the order of their launches: every plan before anything changes
  WavCall call{slots, n, pl, groups, seg, hop, N, m, who, P.launch, samples, common, wav_dev, wav_ld};
  eq::WavStage equal; level::WavStage lv; f0::WavStage follow; act::WavStage activity; byp::WavStage bypass; comfort::WavStage noise; denoise::WavStage suppress; tone::WavStage tones;
  bypass.gate_stage = &activity; noise.gate_stage = &activity;
  equal.plan(s, call); call.pre_staged = equal.stages;
  lv.plan(s, call); follow.plan(s, call); activity.plan(s, call); bypass.plan(s, call); noise.plan(s, call); suppress.plan(s, call); tones.plan(s, call);
  const int nm_in = m.num_mels, nm = c.num_mels;
  int jobs = 0;
  std::vector<RgRow> tab;
  if (!common) {
    tab.assign(n, RgRow{});
    for (int i = 0; i < n; ++i) {
      const FePlan& p = pl[i];
      int* d = tab[i].data();
      const long long r_prev = s->wav_in.fe_slot[slots[i]].recv;
      d[cnk::kRgSlot] = slots[i];
      d[cnk::kRgRecvLo] = (int)(uint32_t)r_prev; d[cnk::kRgRecvHi] = (int)(r_prev >> 32);
      d[cnk::kRgTotalLo] = (int)(uint32_t)p.total; d[cnk::kRgTotalHi] = (int)(p.total >> 32);
      d[cnk::kRgM] = samples[i]; d[cnk::kRgF0] = p.f0; d[cnk::kRgNnew] = p.nnew; d[cnk::kRgPos] = p.pos;
      d[cnk::kRgRows] = p.emit > 0 ? rows : 0; d[cnk::kRgReal] = p.real; d[cnk::kRgEmit] = p.emit;
      d[cnk::kRgJob] = jobs;
      jobs += p.nnew;
    }
    call.each_chunk_row([&](int, int k, int i, int at) {
      int* d = tab[i].data();
      d[cnk::kRgChunk] = at; d[cnk::kRgGroup] = at - k; d[cnk::kRgIndex] = k;
    });
  }
  HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
  hipStream_t cst = (hipStream_t)stream;
  if (!pipelined || groups.empty()) s->join(cst);
  s->wav_out.out_counts.assign(n, 0);      // (rows that emit no frame; hifigan_step fills the others)
  // a ragged call's row table and staging (set q); the resampler's rows and staging (set rs_q), read by the front-end work
  const std::string k = run ? s->ctx->mel_tables(m) : std::string();      // (may throw: before a staging set is taken)
  const bool staged = P.launch || equal.stages || lv.stages;      // (an equaliser or a leveller alone takes the resampler's set for its staging)
  int q = 0;
  if (!common) {
    s->ragged_init();
    q = s->wav_in.rg_sets.begin(tab.data(), n, cst);
  }
  if (staged) call.rs_q = s->wav_in.rs_sets.begin(P.rows.data(), n, cst);
  const int* rg_tab = reinterpret_cast<const int*>(s->wav_in.rg_sets.rows[q]);
  // the front-end work, in the order of FrontPos (the same-position kernel reads the resampler's rows [n][samples], the ragged one
  // [n][seg * hop])
  FrontWork front;
  if (P.launch) rs_enqueue(s, P, n, call.rs_q, wav_dev, wav_ld, common ? samples[0] : seg * hop, front);
  if (staged) front.at[kFrResampleEnd] = [s, rq = call.rs_q](hipStream_t st) { s->wav_in.rs_sets.end(rq, st); };
  if (run) {
    const float* rg = s->ctx->vec(k + ".range");
    const float* wav = staged ? s->wav_in.rs_wav[call.rs_q] : wav_dev;
    auto fill = [&](auto& a) {      // the fields both front-end kernels share
      a.wav = wav; a.aring = s->wav_in.fe_audio; a.mring = s->wav_in.fe_mel; a.chunk = s->wav_in.fe_chunk; a.n = n;
      a.win = s->ctx->vec(k + ".win"); a.tw = reinterpret_cast<const double2*>(s->ctx->vec(k + ".tw")); a.fb = s->ctx->vec(k + ".fb");
      a.lo = reinterpret_cast<const int*>(rg); a.hi = reinterpret_cast<const int*>(rg) + m.num_mels;
      a.LA = s->wav_in.fe_LA; a.LM = s->wav_in.fe_LM; a.nm = nm_in; a.n_fft = N; a.hop = hop; a.nb = N / 2 + 1; a.cmag = (N / 2 + 1 + 3) & ~3;
      a.eps = m.eps; a.vmin = m.vmin; a.vmax = m.vmax; a.mag_eps = m.mag_eps; a.natural_log = m.natural_log;
    };
    if (common) {
      const FePlan& p = pl[0];
      cnk::MelStreamArgs a;
      fill(a);
      a.slots = s->d_slots; a.r_prev = s->wav_in.fe_slot[slots[0]].recv; a.total = p.total;
      a.m = samples[0]; a.f0 = p.f0; a.nnew = p.nnew; a.pos = p.pos; a.rows = p.emit > 0 ? rows : 0; a.real = p.real;
      const double flops = 4.0 * n * p.nnew * (double)(N / 2 + 1) * N;
      front.at[kFrMel] = [s, a, flops](hipStream_t st) {
        if (a.nnew > 0) s->profiled("mel_stream_kernel", flops, st, [&] { cnk::launch_mel_stream(a, st); });
        else s->profiled("mel_stream_copy_kernel", 0.0, st, [&] { cnk::launch_mel_stream_copy(a, st); });
      };
    } else {
      cnk::MelRaggedArgs a;
      fill(a);
      a.tab = rg_tab; a.jobs = jobs; a.wstride = staged ? seg * hop : (int)wav_ld;
      const double flops = 4.0 * jobs * (double)(N / 2 + 1) * N;
      front.at[kFrMel] = [s, a, flops](hipStream_t st) { s->profiled("mel_stream_ragged_kernel", flops, st, [&] { cnk::launch_mel_ragged(a, st); }); };
    }
  }
  activity.power = noise.take(s, cst);      // (a following comfort row reads the frame powers: the detector stages them in this call)
  equal.enqueue(s, call, cst, front, ops); lv.enqueue(s, call, cst, front, ops); follow.enqueue(s, call, cst, front, ops); activity.enqueue(s, call, cst, front, ops); bypass.enqueue(s, call, cst, front, ops);
  noise.enqueue(s, call, cst, front, ops); suppress.enqueue(s, call, cst, front, ops); tones.enqueue(s, call, cst, front, ops);
  const std::function<void(hipStream_t)> pre = [&front](hipStream_t st) { front.run(st); }, none;
  cnk::WavScatterArgs sc;
  sc.tab = rg_tab; sc.n = n; sc.seg = seg; sc.nm = nm; sc.hop = hop;
  sc.codes_src = s->wav_in.rg_codes[q]; sc.mel_src = s->wav_in.rg_mel[q]; sc.wav_src = s->wav_in.rg_wav[q];
  sc.codes = codes_dev; sc.mel = mel_out_dev; sc.wav = route ? nullptr : wav_out_dev;
  const bool piped = pipelined && !groups.empty();      // (the first group's step_pipelined runs the front-end work)
  if (!piped) {
    if (common) s->set_slots(slots, n, cst);      // (mel_stream_kernel reads the slot table)
    front.run(cst);
  }
  call.each_group([&](int g, int off) {
    const std::vector<int32_t>& gs = gslots[g];
    const int ng = (int)gs.size(), e = pl[groups[g][0]].emit;
    const float* chunk = s->wav_in.fe_chunk + (size_t)off * rows * nm_in;
    int32_t* cd = direct ? codes_dev : s->wav_in.rg_codes[q] + (size_t)off * seg;
    float* md = direct ? mel_out_dev : s->wav_in.rg_mel[q] + (size_t)off * seg * nm;
    float* wd = direct ? wav_out_dev : s->wav_in.rg_wav[q] + (size_t)off * seg * hop;
    const float *tf = follow.trk_f0(g, off, seg), *tu = follow.trk_uv(g, off, seg);
    if (pipelined) {
      step_pipelined(s, gs.data(), ng, e, chunk, cd, md, wd, stream, g == 0 ? pre : none, ops[g], tf, tu);
    } else {
      s->set_slots(gs.data(), ng, cst);
      step_blocking(s, ng, e, chunk, cd, md, wd, cst, ops[g], tf, tu);
    }
  });
  // the streams the call's last launches went to (read behind the group steps: a stream-set's first pipelined step creates them)
  hipStream_t last = piped ? s->st_voc : cst, dec = piped ? s->st_front : cst;
  if (scatter && piped) {
    cnk::launch_wav_scatter(sc, last);
    // join() waits for the last step's vocoder event: it now covers the scatter too
    HIP_CHECK(hipEventRecord(s->ev_voc[(s->async_steps - 1) % conan_streams::NP], s->st_voc));
  } else if (scatter) {
    s->profiled("wav_rows_scatter_kernel", 0.0, cst, [&] { cnk::launch_wav_scatter(sc, cst); });
  }
  if (!common) s->wav_in.rg_sets.end(q, last);
  equal.commit(s, dec, last); lv.commit(s, dec, last); follow.commit(s, dec, last); activity.commit(s, dec, last); bypass.commit(s, dec, last); noise.commit(s, dec, last); suppress.commit(s, dec, last); tones.commit(s, dec, last);
  if (scatter && !route) {      // (each group's step counted its own rows, in group order: back to the call's rows)
    s->wav_out.out_counts.assign(n, 0);
    for (int i = 0; i < n; ++i) s->wav_out.out_counts[i] = pl[i].emit * hop;
  }
  fe_commit(s, slots, n, pl, final_);
  for (int i = 0; i < n; ++i) emit_out[i] = pl[i].emit;
  rs_commit(s, slots, n, P, in_final);
  s->wav_in.fe_last_n = n;
  s->wav_in.fe_last_ragged = !common;
}

// conan_step_wav[_async]: `samples` and `final` for every slot, rows of `samples` samples in wav_dev; *emit_out = the common emit
void step_wav_common(conan_streams* s, const int32_t* slots, int n, int samples, int final, const float* wav_dev, const conan_mel_cfg* mel,
                     int32_t* codes_dev, float* mel_out_dev, float* wav_out_dev, int32_t* emit_out, void* stream, bool pipelined) {
  if (!s || !emit_out) throw Error(CONAN_ERR_INVALID, "null argument");
  *emit_out = 0;
  const size_t rows = std::clamp(n, 1, s->max_slots);      // (step_wav checks n)
  const std::vector<int32_t> sm(rows, samples), fin(rows, final != 0);
  std::vector<int32_t> emit(rows, 0);
  step_wav(s, "conan_step_wav", slots, n, sm.data(), fin.data(), wav_dev, std::max(samples, 0), mel, codes_dev, mel_out_dev, wav_out_dev,
           emit.data(), stream, pipelined, true);
  *emit_out = emit[0];
}

void step_wav_chunk(conan_streams* s, float* chunk_dev, void* stream) {
  if (!s || !chunk_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  if (!s->wav_in.fe_chunk || s->wav_in.fe_last_n == 0) throw Error(CONAN_ERR_STATE, "conan_step_wav_chunk: no conan_step_wav call yet");
  if (s->wav_in.fe_last_ragged) throw Error(CONAN_ERR_STATE, "conan_step_wav_chunk: the last wav-in call was conan_step_wav_ragged, whose chunk rows are grouped by emit");
  s->enter(stream);
  const size_t floats = (size_t)s->wav_in.fe_last_n * (s->ctx->cfg.emf_segment + s->ctx->cfg.emf_right_context) * s->ctx->cfg.emf_input_dim;
  HIP_CHECK(hipMemcpyAsync(chunk_dev, s->wav_in.fe_chunk, floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
}

void set_input_rate(conan_streams* s, const int32_t* slots, int n, const conan_resample_cfg* cfg) {
  if (!s || !slots || !cfg) throw Error(CONAN_ERR_INVALID, "null argument");
  if (!s->wav_in.fe_audio) throw Error(CONAN_ERR_STATE, "conan_streams_set_input_rate: the stream-set has no streaming front-end (all three models)");
  if (n < 1 || n > s->max_slots) throw Error(CONAN_ERR_INVALID, "slot count out of range");
  const int S = s->ctx->cfg.emf_segment * s->ctx->hop, model_rate = 50 * s->ctx->hop;
  const conan_resample_cfg& c = *cfg;
  if (c.out_rate != model_rate)
    throw Error(CONAN_ERR_INVALID, "conan_streams_set_input_rate: out_rate must be the model rate (hop * 50 = " + std::to_string(model_rate) + " Hz)");
  check_slot_list(s, slots, n);
  const ch::RsTable* t = rate_table(s, c, "conan_streams_set_input_rate");
  if (t) {
    const long long num = (long long)S * c.in_rate;
    if (num % c.out_rate || (num / c.out_rate) % t->f.orig)
      throw Error(CONAN_ERR_INVALID, "conan_streams_set_input_rate: segment * hop samples at the model rate must be a whole number of input samples and a multiple of in_rate / gcd(in_rate, out_rate)");
    const long long s_in = num / c.out_rate;
    if (t->length(s_in) - t->ready(s_in) > S) throw Error(CONAN_ERR_INVALID, "conan_streams_set_input_rate: the filter's look-ahead is longer than segment * hop samples");
  }
  check_utterance_start(s, slots, n, "conan_streams_set_input_rate");
  HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
  s->resample_init();
  for (int i = 0; i < n; ++i) s->wav_in.rs_slot[slots[i]] = conan_streams::RsSlot{t, 0, 0, 0};
  s->snapshot.in_cfg.resize(s->max_slots, conan_resample_cfg{});
  for (int i = 0; i < n; ++i) s->snapshot.in_cfg[slots[i]] = c;      // (slot snapshots carry the slot's rate)
}

void set_output_rate(conan_streams* s, const int32_t* slots, int n, const conan_resample_cfg* cfg) {
  if (!s || !slots || !cfg) throw Error(CONAN_ERR_INVALID, "null argument");
  if (!(s->ctx->cfg.models & CONAN_MODEL_HIFIGAN)) throw Error(CONAN_ERR_STATE, "conan_streams_set_output_rate: context holds no HiFi-GAN model");
  check_slot_list(s, slots, n);
  const int model_rate = 50 * s->ctx->hop;
  const conan_resample_cfg& c = *cfg;
  if (c.in_rate != model_rate)
    throw Error(CONAN_ERR_INVALID, "conan_streams_set_output_rate: in_rate must be the model rate (hop * 50 = " + std::to_string(model_rate) + " Hz)");
  HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
  const ch::RsTable* t = rate_table(s, c, "conan_streams_set_output_rate");
  for (int i = 0; i < n; ++i)
    if (s->wav_out.voc_samples[slots[i]] != 0)
      throw Error(CONAN_ERR_STATE, "conan_streams_set_output_rate: slot " + std::to_string(slots[i]) + " is not at the start of its vocoder stream (reset it with CONAN_MODEL_HIFIGAN first)");
  if (!t && s->wav_out.or_slot.empty()) return;      // the model-rate path of a stream-set that never had a rate: nothing to allocate
  s->out_ring_init();
  for (int i = 0; i < n; ++i) s->wav_out.or_slot[slots[i]] = conan_streams::OrSlot{t, 0, 0};
  s->snapshot.out_cfg.resize(s->max_slots, conan_resample_cfg{});
  for (int i = 0; i < n; ++i) s->snapshot.out_cfg[slots[i]] = c;
}

// conan_streams_set_input_drift / _set_output_drift.  cfg: configure (the slots at the start of their utterance / vocoder stream, as for
// the rate setters); null: a live change of ppb, host state only - it takes effect at the slot's next output.
void set_drift(conan_streams* s, int side, const int32_t* slots, int n, const conan_resample_cfg* cfg, const int32_t* ppb) {
  const bool in = side == CONAN_DRIFT_SOURCE;
  const std::string who = in ? "conan_streams_set_input_drift" : "conan_streams_set_output_drift";
  if (!s || !slots || !ppb) throw Error(CONAN_ERR_INVALID, "null argument");
  if (in && !s->wav_in.fe_audio) throw Error(CONAN_ERR_STATE, who + ": the stream-set has no streaming front-end (all three models)");
  if (!in && !(s->ctx->cfg.models & CONAN_MODEL_HIFIGAN)) throw Error(CONAN_ERR_STATE, who + ": context holds no HiFi-GAN model");
  check_slot_list(s, slots, n);
  for (int i = 0; i < n; ++i)
    if (ppb[i] < -CONAN_DRIFT_MAX_PPB || ppb[i] > CONAN_DRIFT_MAX_PPB) throw Error(CONAN_ERR_INVALID, who + ": |ppb| must be at most 2 000 000");
  auto slot_dr = [&](int slot) -> ch::DriftPos* {
    if (in) return s->wav_in.rs_slot.empty() ? nullptr : &s->wav_in.rs_slot[slot].dr;
    return s->wav_out.or_slot.empty() ? nullptr : &s->wav_out.or_slot[slot].dr;
  };
  if (!cfg) {
    for (int i = 0; i < n; ++i) {
      const ch::DriftPos* d = slot_dr(slots[i]);
      if (!d || !d->d) throw Error(CONAN_ERR_STATE, who + ": slot " + std::to_string(slots[i]) + " has no drift resampler (configure it with a cfg first)");
    }
    for (int i = 0; i < n; ++i) {
      ch::DriftPos& d = *slot_dr(slots[i]);
      conan_resample_cfg c{};
      c.in_rate = d.d->in_rate; c.out_rate = d.d->out_rate;
      d.retime(ppb[i], drift::step(c, side, ppb[i]), in ? s->wav_in.rs_slot[slots[i]].out : s->wav_out.or_slot[slots[i]].out);
    }
    return;
  }
  const conan_resample_cfg& c = *cfg;
  const int S = s->ctx->cfg.emf_segment * s->ctx->hop, model_rate = 50 * s->ctx->hop;
  if (in && c.out_rate != model_rate) throw Error(CONAN_ERR_INVALID, who + ": out_rate must be the model rate (hop * 50 = " + std::to_string(model_rate) + " Hz)");
  if (!in && c.in_rate != model_rate) throw Error(CONAN_ERR_INVALID, who + ": in_rate must be the model rate (hop * 50 = " + std::to_string(model_rate) + " Hz)");
  const int win = drift::tile_window(c, side);      // (the configuration's checks; before any GPU use)
  if (in && ((long long)S * c.in_rate) % c.out_rate) throw Error(CONAN_ERR_INVALID, who + ": segment * hop samples at the model rate must be a whole number of input samples");
  if (in) check_utterance_start(s, slots, n, who.c_str());
  for (int i = 0; i < n && !in; ++i)
    if (s->wav_out.voc_samples[slots[i]] != 0)
      throw Error(CONAN_ERR_STATE, who + ": slot " + std::to_string(slots[i]) + " is not at the start of its vocoder stream (reset it with CONAN_MODEL_HIFIGAN first)");
  HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
  const ch::DrTable& t = s->ctx->drift_table(c);
  if (in) s->resample_init(); else s->out_ring_init();
  for (int i = 0; i < n; ++i) {
    ch::DriftPos d;
    d.d = &t; d.win = win; d.ppb = ppb[i]; d.step = drift::step(c, side, ppb[i]);
    if (in) {
      conan_streams::RsSlot& r = s->wav_in.rs_slot[slots[i]];
      r = conan_streams::RsSlot{nullptr, 0, 0, 0};
      r.dr = d; r.s_in = (int)((long long)S * c.in_rate / c.out_rate);
    } else {
      conan_streams::OrSlot& o = s->wav_out.or_slot[slots[i]];
      o = conan_streams::OrSlot{nullptr, 0, 0};
      o.dr = d; o.out_rate = c.out_rate;
    }
  }
  // (slot snapshots refuse a drift slot; its rate record reads "none")
  std::vector<conan_resample_cfg>& rec = in ? s->snapshot.in_cfg : s->snapshot.out_cfg;
  rec.resize(s->max_slots, conan_resample_cfg{});
  for (int i = 0; i < n; ++i) rec[slots[i]] = conan_resample_cfg{};
}

void get_drift(conan_streams* s, int side, const int32_t* slots, int n, int32_t* ppb_out, int64_t* in_out, int64_t* out_out) {
  const bool in = side == CONAN_DRIFT_SOURCE;
  const std::string who = in ? "conan_streams_input_drift" : "conan_streams_output_drift";
  if (!s || !slots) throw Error(CONAN_ERR_INVALID, "null argument");
  check_slot_list(s, slots, n);
  for (int i = 0; i < n; ++i) {
    const bool has = in ? (!s->wav_in.rs_slot.empty() && s->wav_in.rs_slot[slots[i]].dr.d) : (!s->wav_out.or_slot.empty() && s->wav_out.or_slot[slots[i]].dr.d);
    if (!has) throw Error(CONAN_ERR_STATE, who + ": slot " + std::to_string(slots[i]) + " has no drift resampler");
    if (ppb_out) ppb_out[i] = in ? s->wav_in.rs_slot[slots[i]].dr.ppb : s->wav_out.or_slot[slots[i]].dr.ppb;
    if (in_out) in_out[i] = in ? s->wav_in.rs_slot[slots[i]].in : s->wav_out.voc_samples[slots[i]];
    if (out_out) out_out[i] = in ? s->wav_in.rs_slot[slots[i]].out : s->wav_out.or_slot[slots[i]].out;
  }
}

void set_output_ld(conan_streams* s, int64_t ld) {
  if (!s) throw Error(CONAN_ERR_INVALID, "null streams");
  if (ld < 0 || ld > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_streams_set_output_ld: ld out of range");
  s->wav_out.out_ld = ld;
}

void store_format(std::vector<unsigned char>& fmt, int& not_f32, const int32_t* slots, int n, int format) {
  for (int i = 0; i < n; ++i) {
    not_f32 += (format != 0) - (fmt[slots[i]] != 0);
    fmt[slots[i]] = (unsigned char)format;
  }
}

void set_input_format(conan_streams* s, const int32_t* slots, int n, int format) {
  if (!s || !slots) throw Error(CONAN_ERR_INVALID, "null argument");
  if (!s->wav_in.fe_audio) throw Error(CONAN_ERR_STATE, "conan_streams_set_input_format: the stream-set has no streaming front-end (all three models)");
  check_format(format, "conan_streams_set_input_format");
  check_slot_list(s, slots, n);
  if (format != CONAN_SAMPLE_F32) {      // staging rows and row tables only: a format has no stream state
    HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
    s->rs_stage_init();
  }
  store_format(s->wav_in.in_fmt, s->wav_in.in_fmt_n, slots, n, format);
}

void set_output_format(conan_streams* s, const int32_t* slots, int n, int format) {
  if (!s || !slots) throw Error(CONAN_ERR_INVALID, "null argument");
  if (!(s->ctx->cfg.models & CONAN_MODEL_HIFIGAN)) throw Error(CONAN_ERR_STATE, "conan_streams_set_output_format: context holds no HiFi-GAN model");
  check_format(format, "conan_streams_set_output_format");
  check_slot_list(s, slots, n);
  store_format(s->wav_out.out_fmt, s->wav_out.out_fmt_n, slots, n, format);
}

int output_samples(conan_streams* s, int32_t* counts, int cap) {
  if (!s || (!counts && cap > 0) || cap < 0) throw Error(CONAN_ERR_INVALID, "null argument");
  const int rows = (int)s->wav_out.out_counts.size();
  for (int i = 0; i < rows && i < cap; ++i) counts[i] = s->wav_out.out_counts[i];
  return rows;
}

void output_pending(conan_streams* s, const int32_t* slots, int n, int32_t* counts) {
  if (!s || !slots || !counts) throw Error(CONAN_ERR_INVALID, "null argument");
  check_slot_list(s, slots, n);
  const conan_streams::OutPlan P = s->out_plan(slots, n, 0, nullptr, INT_MAX, nullptr, "conan_streams_output_pending");
  for (int i = 0; i < n; ++i) counts[i] = P.counts[i];
}

void flush_output(conan_streams* s, const int32_t* slots, int n, float* wav_out_dev, int64_t wav_ld, void* stream) {
  if (!s || !slots || !wav_out_dev) throw Error(CONAN_ERR_INVALID, "null argument");
  if (wav_ld < 0 || wav_ld > INT_MAX) throw Error(CONAN_ERR_INVALID, "conan_streams_flush_output: wav_ld out of range");
  check_slot_list(s, slots, n);
  const conan_streams::OutPlan P = s->out_plan(slots, n, 0, wav_out_dev, wav_ld, nullptr, "conan_streams_flush_output");
  hipStream_t st = s->enter(stream);
  if (P.active) {
    s->out_stage_init();
    s->resample_out(P, s->wav_out.or_sets.begin(P.rows.data(), n, st), 0, st);
  }
  for (int i = 0; i < n && !s->wav_out.or_slot.empty(); ++i) {
    conan_streams::OrSlot& o = s->wav_out.or_slot[slots[i]];
    if (!o.rated() || s->wav_out.voc_samples[slots[i]] == 0) continue;
    o.out += P.counts[i]; o.flushed = 1;
  }
}

}  // namespace wavio

void conan_streams::resample_init() {
  rs_stage_init();
  if (!wav_in.rs_ring) wav_in.rs_ring = alloc((size_t)max_slots * cnk::kRsRing);        // stream state (state_bytes)
}

void conan_streams::out_ring_init() {
  if (wav_out.or_ring) return;
  // the history holds model-rate audio: the longest span of an accepted filter (CONAN_RESAMPLE_MAX_TAPS) plus the largest step
  wav_out.or_ring_len = ch::next_pow2(CONAN_RESAMPLE_MAX_TAPS + 8 + max_frames * ctx->hop);
  wav_out.or_ring = alloc((size_t)max_slots * wav_out.or_ring_len);        // stream state (state_bytes)
  wav_out.or_slot.assign(max_slots, OrSlot());
}

void conan_streams::rs_stage_init() {
  if (wav_in.rs_wav[0]) return;
  const size_t S = (size_t)ctx->cfg.emf_segment * ctx->hop;
  wav_in.rs_sets.init(max_slots, allocs);
  for (float*& w : wav_in.rs_wav) w = (float*)stage_alloc((size_t)max_slots * S * sizeof(float));
  wav_in.rs_slot.assign(max_slots, RsSlot());
}

void conan_streams::ragged_init() {
  if (wav_in.rg_wav[0]) return;
  const conan_cfg& c = ctx->cfg;
  const size_t seg = c.emf_segment;
  wav_in.rg_sets.init(max_slots, allocs);
  for (int q = 0; q < kStageSets; ++q) {
    wav_in.rg_codes[q] = (int*)stage_alloc((size_t)max_slots * seg * sizeof(int));
    wav_in.rg_mel[q] = (float*)stage_alloc((size_t)max_slots * seg * c.num_mels * sizeof(float));
    wav_in.rg_wav[q] = (float*)stage_alloc((size_t)max_slots * seg * ctx->hop * sizeof(float));
  }
}

void conan_streams::out_stage_init() {
  if (wav_out.or_wav[0]) return;
  const size_t S = (size_t)max_frames * ctx->hop;
  wav_out.or_sets.init(max_slots, allocs);
  for (float*& w : wav_out.or_wav) w = (float*)stage_alloc((size_t)max_slots * S * sizeof(float));
}

// The output rows of one vocoder step that gives each of `slots` `frames` frames (frames = 0: conan_streams_flush_output, the rest of
// the utterance).  Row i goes to row dst[i] (i without a table) of wav_out_dev at the stride in force: conan_streams_set_output_ld, else
// natural_ld.  A slot with a rate receives outputs [delivered, ready(I)) for I = its model-rate samples after the step (a flush:
// up to length(I)), any other slot its frames * hop samples.  Every row is checked and nothing changes.
conan_streams::OutPlan conan_streams::out_plan(const int32_t* slots, int n, int frames, float* wav_out_dev, long long natural_ld, const std::vector<int>* dst,
                                               const std::string& who) const {
  if (n < 1 || n > max_slots) throw Error(CONAN_ERR_INVALID, "slot count out of range");
  OutPlan P;
  const int T = frames * ctx->hop;
  const bool flush = frames == 0;
  P.base = wav_out_dev; P.ld = (wav_out.out_ld && !flush) ? wav_out.out_ld : natural_ld;      // (a flush brings its own stride)
  P.counts.assign(n, T);
  if (dst) P.dst = *dst;
  bool any = false;
  for (int i = 0; i < n && (!wav_out.or_slot.empty() || wav_out.out_fmt_n); ++i) {      // (the mel-in entry points come here before set_slots has seen the list)
    if (slots[i] < 0 || slots[i] >= max_slots) throw Error(CONAN_ERR_INVALID, "slot index out of range");
    any = any || (!wav_out.or_slot.empty() && wav_out.or_slot[slots[i]].rated()) || wav_out.out_fmt[slots[i]];      // (a format alone sends the step through the copy rows)
  }
  if (!flush) P.lvl_rows = olv::step_rows(this, slots, n, frames, who);      // (checked here, before anything changes: CONAN_ERR_UNSUPPORTED rows)
  if (!flush) P.wm_rows = wmark::step_rows(this, slots, n, frames, who);
  if (!flush) P.eq_rows = eq::step_rows(this, slots, n, frames, who);
  P.active = any || dst || P.ld != T;
  if (flush) P.active = false;
  if (!P.active && !flush) return P;
  P.rows.resize(n);
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] >= max_slots) throw Error(CONAN_ERR_INVALID, "slot index out of range");
    cnk::RsOutRow& row = P.rows[i];
    memset(&row, 0, sizeof(row));
    const int fmt = wav_out.out_fmt[slots[i]], bps = wavio::bytes_per_sample(fmt);
    row.slot = slots[i]; row.m = T; row.h = T; row.dst = (dst ? (*dst)[i] : i) | (fmt << cnk::kOrDstBits);
    if (fmt != cnk::kFmtF32 && ((uintptr_t)wav_out_dev & 3)) throw Error(CONAN_ERR_INVALID, who + ": wav_out_dev must be 4-byte aligned");
    if (!wav_out.or_slot.empty() && wav_out.or_slot[slots[i]].dr.d) {      // a drift slot (conan_streams_set_output_drift)
      const OrSlot& o = wav_out.or_slot[slots[i]];
      const ch::DriftPos& D = o.dr;
      const int W = D.d->W;
      const std::string where = who + ": slot " + std::to_string(slots[i]) + " (output at " + std::to_string(o.out_rate) + " Hz with drift): ";
      const long long in0 = wav_out.voc_samples[slots[i]], I = in0 + T;
      long long J = o.out;
      if (flush) { if (!o.flushed) J = std::max(D.first_at(I), o.out); }
      else {
        if (o.flushed) throw Error(CONAN_ERR_STATE, where + "conan_streams_flush_output has ended the utterance; reset the slot with CONAN_MODEL_HIFIGAN first");
        J = std::max(D.first_at(I - W), o.out);
      }
      const ch::DriftPos::u128 p0 = D.pos(o.out);
      const long long n_first = (long long)(p0 >> 32);
      if (I - std::max(0ll, n_first - W + 1) > wav_out.or_ring_len) throw Error(CONAN_ERR_UNSUPPORTED, where + "resampler history ring too small for this configuration");
      if (J - o.out > INT_MAX || (ch::DriftPos::u128)(J - o.out) * D.step >> 62) throw Error(CONAN_ERR_INVALID, where + "too many samples in one call");
      row.taps = reinterpret_cast<const float*>(D.d->dev); row.ph = reinterpret_cast<const int*>((uintptr_t)D.step);
      row.in0 = in0; row.out0 = n_first; row.orig = (int)(unsigned)p0; row.w = W; row.L = cnk::kOrDriftL; row.h = (int)(J - o.out);
      P.active = P.active || row.h > 0;
      P.win = std::max(P.win, D.win);
      P.flops += 8.0 * row.h * W;
    } else if (!wav_out.or_slot.empty() && wav_out.or_slot[slots[i]].f) {
      const OrSlot& o = wav_out.or_slot[slots[i]];
      const ch::RsTable& t = *o.f;
      const std::string where = who + ": slot " + std::to_string(slots[i]) + " (output at " + std::to_string(t.out_rate) + " Hz): ";
      const long long in0 = wav_out.voc_samples[slots[i]], I = in0 + T;
      long long J = o.out;
      if (flush) { if (!o.flushed) J = t.length(I); }
      else {
        if (o.flushed) throw Error(CONAN_ERR_STATE, where + "conan_streams_flush_output has ended the utterance; reset the slot with CONAN_MODEL_HIFIGAN first");
        J = std::max(t.ready(I), o.out);
      }
      if (!wavio::ring_fits(t, I, o.out, wav_out.or_ring_len)) throw Error(CONAN_ERR_UNSUPPORTED, where + "resampler history ring too small for this configuration");
      if (J - o.out > INT_MAX) throw Error(CONAN_ERR_INVALID, where + "too many samples in one call");
      wavio::fill_filter(row, t);
      row.in0 = in0; row.out0 = o.out; row.h = (int)(J - o.out);
      P.active = P.active || row.h > 0;
      P.win = std::max(P.win, t.win);
      P.flops += 2.0 * row.h * t.f.L;
    } else if (flush) {
      row.h = 0;
    }
    P.counts[i] = row.h;
    if ((long long)row.h * bps > P.ld * 4)
      throw Error(CONAN_ERR_INVALID, who + ": slot " + std::to_string(slots[i]) + " (call row " + std::to_string(dst ? (*dst)[i] : i) + ") delivers " + std::to_string(row.h) +
                                         " samples of " + std::to_string(bps) + " bytes, more than the row stride of wav_out_dev in force (" + std::to_string(P.ld) +
                                         " x 4 bytes" + (flush ? "; conan_streams_output_pending)" : "; conan_streams_set_output_ld)"));
    P.tiles = std::max(P.tiles, (std::max(row.h, row.m) + cnk::kRsTile - 1) / cnk::kRsTile);
  }
  return P;
}

void conan_streams::resample_out(const OutPlan& op, int q, long long src_ld, hipStream_t st) {
  cnk::ResampleOutArgs ra;
  ra.wav = wav_out.or_wav[q]; ra.wav_ld = src_ld; ra.ring = wav_out.or_ring; ra.ring_len = wav_out.or_ring_len; ra.out = op.base; ra.out_ld = op.ld;
  ra.rows = wav_out.or_sets.rows[q]; ra.n = (int)op.rows.size(); ra.tiles = op.tiles; ra.win = op.win;
  profiled("resample_out_kernel", op.flops, st, [&] { cnk::launch_resample_out(ra, st); });
  wav_out.or_sets.end(q, st);
}
