// extern "C" surface of libconan_hip.so (include/conan_hip.h).
#include "streams.h"

static thread_local std::string g_err;

template <typename F>
static int guarded(F&& f) {
  try {
    f();
    // kernel launches do not return a status: a launch that the runtime rejected (resources, bad configuration) is
    // reported here instead of being lost - the product path must fail loudly
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) throw ch::Error(CONAN_ERR_HIP, std::string("HIP launch error: ") + hipGetErrorString(le));
    return CONAN_OK;
  } catch (const ch::Error& e) {
    g_err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    g_err = e.what();
    return CONAN_ERR_INVALID;
  }
}

static void validate_cfg(const conan_cfg& c) {
  if (c.abi_version != CONAN_HIP_ABI_VERSION) throw Error(CONAN_ERR_INVALID, "conan_cfg.abi_version mismatch");
  if (c.models & CONAN_MODEL_HIFIGAN) {
    if (c.voc_num_ups < 1 || c.voc_num_ups > CONAN_MAX_UPS) throw Error(CONAN_ERR_INVALID, "voc_num_ups");
    if (c.voc_num_resblocks < 1 || c.voc_num_resblocks > 3) throw Error(CONAN_ERR_UNSUPPORTED, "1..3 resblock branches supported");
    if (c.voc_rb_num_dil < 1 || c.voc_rb_num_dil > CONAN_MAX_DILATIONS) throw Error(CONAN_ERR_INVALID, "voc_rb_num_dil");
    if (c.voc_upsample < 0 || c.voc_upsample > 2) throw Error(CONAN_ERR_UNSUPPORTED, "voc_upsample: 0 (shuffle), 1 (zero) or 2 (nn)");
    for (int i = 0; i < c.voc_num_ups && c.voc_upsample == 2; ++i)     // hifigan_causal.py:70-71
      if (c.voc_up_kernels[i] % 2 || c.voc_up_rates[i] < 2) throw Error(CONAN_ERR_INVALID, "upsample 'nn': kernel sizes must be even, rates >= 2");
    if (c.voc_resblock < 0 || c.voc_resblock > 2) throw Error(CONAN_ERR_UNSUPPORTED, "voc_resblock: 1 or 2");
    int ch_ = c.voc_initial_channel;
    for (int i = 0; i < c.voc_num_ups; ++i) { ch_ /= 2; if (ch_ < 4 || ch_ % 4) throw Error(CONAN_ERR_UNSUPPORTED, "vocoder channel ladder must stay a multiple of 4"); }
    if (c.num_mels % 4) throw Error(CONAN_ERR_UNSUPPORTED, "num_mels must be a multiple of 4");
  }
  if (c.models & CONAN_MODEL_EMFORMER) {
    if (c.emf_input_dim % c.emf_heads || c.emf_input_dim / c.emf_heads > 16) throw Error(CONAN_ERR_UNSUPPORTED, "emformer head_dim must be <= 16");
    if (c.emf_input_dim % 4 || c.emf_input_dim > 512) throw Error(CONAN_ERR_UNSUPPORTED, "emformer input_dim");
    if (c.emf_segment < 1 || c.emf_right_context < 0) throw Error(CONAN_ERR_INVALID, "emformer segment/right context");
    if (c.emf_max_memory_size < 0) throw Error(CONAN_ERR_INVALID, "emf_max_memory_size");
    if (c.emf_max_memory_size > 32) throw Error(CONAN_ERR_UNSUPPORTED, "emf_max_memory_size > 32");
    if (c.emf_max_memory_size + c.emf_right_context + c.emf_left_context + c.emf_segment > 128 || c.emf_heads > 16) throw Error(CONAN_ERR_UNSUPPORTED, "emformer attention supports <= 128 keys, <= 16 heads");
  }
  if (c.models & CONAN_MODEL_CONAN) {
    if (c.hidden_size % 8 || c.hidden_size > 512) throw Error(CONAN_ERR_UNSUPPORTED, "hidden_size must be a multiple of 8 and <= 512");
    if (c.dec_num_blocks < 1 || c.dec_num_blocks > CONAN_MAX_DEC_BLOCKS) throw Error(CONAN_ERR_INVALID, "dec_num_blocks");
    if (c.nvq < 1) throw Error(CONAN_ERR_INVALID, "nvq");
  }
}

// The preconditions of every fused chunk step (conan_step[_async], the wav-in steps): all three models, an upsampler without look-ahead.
void check_chunk_step(const conan_streams* s, const char* who) {
  const int all = CONAN_MODEL_EMFORMER | CONAN_MODEL_CONAN | CONAN_MODEL_HIFIGAN;
  if ((s->ctx->cfg.models & all) != all) throw Error(CONAN_ERR_STATE, std::string(who) + " needs all three models in the context");
  if (s->ctx->cfg.voc_upsample == 2) throw Error(CONAN_ERR_UNSUPPORTED, "fused chunk steps carry vocoder state from chunk to chunk; upsample 'nn' (CausalUpsampleBlock1) looks ahead: "
                                                                      "step the Emformer and decoder per chunk and run conan_hifigan_step over the mel prefix after a reset (inference/Conan.py:147-155)");
}

// The stages of one chunk step on `st` for the slots set_slots has just installed (conan_step, conan_step_wav).
void step_blocking(conan_streams* s, int n, int emit, const float* mel_chunk_dev, int32_t* codes_dev, float* mel_out_dev,
                   float* wav_out_dev, hipStream_t st, const conan_streams::OutPlan& op, const float* trk_f0, const float* trk_uv) {
  const int seg = s->ctx->cfg.emf_segment;
  int* codes_seg = codes_dev ? codes_dev : s->d_codes;
  s->emformer_step(n, mel_chunk_dev, nullptr, nullptr, codes_seg, st);
  const int* codes_emit = codes_seg;
  if (emit != seg && n > 1) {
    int* compact = s->d_codes + (size_t)s->max_slots * s->max_frames;
    cnk::launch_copy_int_rows(compact, codes_seg, n, emit, seg, st);
    codes_emit = compact;
  }
  float* mel = mel_out_dev ? mel_out_dev : s->c_mel.base;
  conan_streams::DecExtra ex;
  ex.trk_f0 = trk_f0; ex.trk_uv = trk_uv;
  { conan_decoder_taps none; memset(&none, 0, sizeof(none)); s->decoder_step(n, emit, codes_emit, mel, none, st, &ex); }
  s->hifigan_step(n, emit, mel, wav_out_dev, nullptr, st, nullptr, &op);
}

// Everything of conan_step_async after its argument checks; `pre` (may be empty) enqueues work on the Emformer stream right
// before the step's Emformer launch, behind the step's input event and slot table.
void step_pipelined(conan_streams* s, const int32_t* slots, int n, int emit, const float* mel_chunk_dev, int32_t* codes_dev, float* mel_out_dev,
                    float* wav_out_dev, void* stream, const std::function<void(hipStream_t)>& pre, const conan_streams::OutPlan& op,
                    const float* trk_f0, const float* trk_uv) {
  const int seg = s->ctx->cfg.emf_segment;
  HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
  s->async_init();
  const long long t = s->async_steps;
  constexpr int NP = conan_streams::NP;
  const int p = (int)(t % NP), pl = (int)((t + NP - 1) % NP);      // hand-off ring positions of this step and of the previous one
  // Three stages on three internal streams: Emformer(t) -> codes, decoder(t) -> mel, vocoder(t) -> audio.  With steps
  // issued back to back the stages work on consecutive chunks at the same time (Emformer of chunk t+2 beside the decoder
  // of t+1 beside the vocoder of t): the decoder's ~50 latency-bound launches no longer queue behind the Emformer's
  // one long launch, and their tail no longer leaves the vocoder stream idle.
  // An EMPTY pipeline (the first step, or every earlier step has completed - e.g. behind the caller's join + synchronize): nothing of
  // this stream-set can overlap this step's Emformer launch, which the decoder and vocoder of the same chunk wait for - it may take
  // the blocking steps' launch shape (one workgroup per CU where the stream-set is alone on the device: 136 instead of 190 us on
  // the first chunk's critical path; the feed-forward's sum does not depend on the cluster size, so the bits are the same).
  s->pipe_idle = t == 0 || (hipEventQuery(s->ev_emf[pl]) == hipSuccess && hipEventQuery(s->ev_front[pl]) == hipSuccess && hipEventQuery(s->ev_voc[pl]) == hipSuccess);
  (void)hipGetLastError();      // (hipErrorNotReady from a query is an answer, not an error)
  // inputs are ready in the caller's stream order
  HIP_CHECK(hipEventRecord(s->ev_in[p], (hipStream_t)stream));
  HIP_CHECK(hipStreamWaitEvent(s->st_emf, s->ev_in[p], 0));
  const bool tl = s->tl_on && s->tl_n < (int)s->tl_ev.size() / 6;
  hipEvent_t* te = tl ? &s->tl_ev[(size_t)s->tl_n * 6] : nullptr;
  // a changed slot list rewrites the table the in-flight decoder / vocoder still read: drain them first
  bool same = (int)s->h_slots.size() == n;
  for (int i = 0; same && i < n; ++i) same = s->h_slots[i] == slots[i];
  if (!same && t >= 1) {
    HIP_CHECK(hipStreamWaitEvent(s->st_emf, s->ev_front[pl], 0));
    HIP_CHECK(hipStreamWaitEvent(s->st_emf, s->ev_voc[pl], 0));
  }
  s->set_slots(slots, n, s->st_emf);
  // the code buffer at this ring position is free once the decoder of step t-NP has read it: the Emformer may run
  // NP steps ahead of the decoder (it is dispatched late - its 129 KB of LDS per block only fit on CUs that a vocoder
  // launch has left - so the decoder must not have to wait for the Emformer of its own chunk)
  if (t >= NP) HIP_CHECK(hipStreamWaitEvent(s->st_emf, s->ev_front[p], 0));
  int* codes_seg = s->codes_hand[p];
  // developer timing switches of `make DEV=1` builds, never of the shipped library (plan_switches.h): SKIP_STAGE bit 0 skips the Emformer
  // launch, bit 1 the decoder's (a skipped stage returns garbage with CONAN_OK); EMF_HOLD keeps the Emformer's workgroups, which need
  // whole CUs for ~0.15 ms, away from the pair kernel's launches (off by default: see streams.h, ev_wide)
  const int skip = s->sw.skip_stage;
  const bool hold = s->sw.emf_hold;
  if (hold && t >= 2 && s->ev_wide[(t + NP - 2) % NP] && s->wide_marked[(t + NP - 2) % NP]) HIP_CHECK(hipStreamWaitEvent(s->st_emf, s->ev_wide[(t + NP - 2) % NP], 0));
  if (pre) pre(s->st_emf);      // conan_step_wav_async: the streaming front-end writes the chunk this step consumes
  if (tl) HIP_CHECK(hipEventRecord(te[0], s->st_emf));
  if (!(skip & 1)) s->emformer_step(n, mel_chunk_dev, nullptr, nullptr, codes_seg, s->st_emf);
  if (tl) HIP_CHECK(hipEventRecord(te[1], s->st_emf));
  HIP_CHECK(hipEventRecord(s->ev_emf[p], s->st_emf));
  HIP_CHECK(hipStreamWaitEvent(s->st_front, s->ev_emf[p], 0));
  // the mel hand-off buffer at this ring position is free once the vocoder of step t-NP has copied it into its ring
  if (t >= NP) HIP_CHECK(hipStreamWaitEvent(s->st_front, s->ev_voc[p], 0));
  if (tl) HIP_CHECK(hipEventRecord(te[2], s->st_front));
  // the caller's copies of the step's codes and mel frames travel with the decoder step (operators of its one launch)
  conan_streams::DecExtra ex;
  if (codes_dev) { ex.codes_dst = codes_dev; ex.codes_src = codes_seg; ex.codes_words = n * seg; }
  ex.mel_out2 = mel_out_dev;
  ex.trk_f0 = trk_f0; ex.trk_uv = trk_uv;
  const int* codes_emit = codes_seg;
  if (emit != seg && n > 1) {
    int* compact = s->d_codes + (size_t)s->max_slots * s->max_frames;
    cnk::launch_copy_int_rows(compact, codes_seg, n, emit, seg, s->st_front);
    codes_emit = compact;
  }
  float* mel = s->mel_hand[p];
  if (!(skip & 2)) { conan_decoder_taps none; memset(&none, 0, sizeof(none)); s->decoder_step(n, emit, codes_emit, mel, none, s->st_front, &ex); }
  if (tl) HIP_CHECK(hipEventRecord(te[3], s->st_front));
  HIP_CHECK(hipEventRecord(s->ev_front[p], s->st_front));
  HIP_CHECK(hipStreamWaitEvent(s->st_voc, s->ev_front[p], 0));
  if (s->fence_set) {      // the caller's output fence: only the stage that writes the audio buffer waits for it
    if (s->fence_event) HIP_CHECK(hipStreamWaitEvent(s->st_voc, s->fence_event, 0));
    else {
      HIP_CHECK(hipEventRecord(s->ev_fence[p], s->fence_stream));
      HIP_CHECK(hipStreamWaitEvent(s->st_voc, s->ev_fence[p], 0));
    }
    s->fence_set = false; s->fence_event = nullptr;
  }
  if (tl) HIP_CHECK(hipEventRecord(te[4], s->st_voc));
  if (!s->ev_wide[p]) HIP_CHECK(hipEventCreateWithFlags(&s->ev_wide[p], hipEventDisableTiming));
  s->mark_wide = s->ev_wide[p];
  s->wide_marked[p] = false;
  s->hifigan_step(n, emit, mel, wav_out_dev, nullptr, s->st_voc, nullptr, &op);
  s->mark_wide = nullptr;
  if (tl) { HIP_CHECK(hipEventRecord(te[5], s->st_voc)); s->tl_n++; }
  HIP_CHECK(hipEventRecord(s->ev_voc[p], s->st_voc));
  if (s->clock_on && s->clock_n < (int)s->clock_ev.size()) HIP_CHECK(hipEventRecord(s->clock_ev[s->clock_n++], s->st_voc));   // step completion stamp
  s->async_steps = t + 1;
}

extern "C" {

const char* conan_last_error(void) { return g_err.c_str(); }
int conan_abi_version(void) { return CONAN_HIP_ABI_VERSION; }

int conan_ctx_create(int device, const conan_cfg* cfg, conan_ctx** out) {
  return guarded([&] {
    if (!cfg || !out) throw Error(CONAN_ERR_INVALID, "null argument");
    validate_cfg(*cfg);
    int ndev = 0;
    HIP_CHECK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) throw Error(CONAN_ERR_HIP, "no such HIP device (libconan_hip has no CPU fallback)");
    HIP_CHECK(hipSetDevice(device));
    conan_ctx* c = new conan_ctx();
    c->device = device;
    c->cfg = *cfg;
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, device));
    c->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    int hop = 1;
    for (int i = 0; i < cfg->voc_num_ups; ++i) hop *= cfg->voc_up_rates[i];
    c->hop = hop;
    *out = c;
  });
}

int conan_ctx_destroy(conan_ctx* ctx) {
  return guarded([&] { delete ctx; });
}

int conan_ctx_load_tensor(conan_ctx* ctx, const char* key, const float* host, const int64_t* shape, int ndim) {
  int known = 1;
  int rc = guarded([&] {
    if (!ctx || !key || !host || ndim < 0 || ndim > 4) throw Error(CONAN_ERR_INVALID, "bad argument");
    if (ctx->finalized) throw Error(CONAN_ERR_STATE, "context already finalized");
    std::string k(key);
    if (k.rfind("emformer.", 0) != 0 && k.rfind("conan.", 0) != 0 && k.rfind("hifigan.", 0) != 0) { known = 0; return; }
    ch::HostTensor t;
    t.shape.assign(shape, shape + ndim);
    int64_t n = t.numel();
    if (n < 0 || n > (int64_t)1 << 31) throw Error(CONAN_ERR_SHAPE, "tensor too large");
    t.data.assign(host, host + n);
    ctx->raw[k] = std::move(t);
  });
  if (rc != CONAN_OK) return rc;
  return known ? 0 : 1;
}

int conan_ctx_finalize(conan_ctx* ctx) {
  return guarded([&] {
    if (!ctx) throw Error(CONAN_ERR_INVALID, "null ctx");
    if (ctx->finalized) return;
    HIP_CHECK(hipSetDevice(ctx->device));
    if (ctx->cfg.models & CONAN_MODEL_HIFIGAN) ctx->finalize_hifigan();
    if (ctx->cfg.models & CONAN_MODEL_EMFORMER) ctx->finalize_emformer();
    if (ctx->cfg.models & CONAN_MODEL_CONAN) ctx->finalize_conan();
    ctx->raw.clear();
    ctx->finalized = true;
  });
}

int conan_streams_create(conan_ctx* ctx, int max_slots, int max_frames, int max_ref_frames, conan_streams** out) {
  return conan_streams_create_opts(ctx, max_slots, max_frames, max_ref_frames, nullptr, out);
}

int conan_streams_arith(const conan_streams* s) {
  if (!s) { g_err = "null streams"; return CONAN_ERR_INVALID; }
  return s->rb_limb ? CONAN_ARITH_LIMB : CONAN_ARITH_F32;
}

int conan_streams_create_opts(conan_ctx* ctx, int max_slots, int max_frames, int max_ref_frames, const conan_streams_opts* opts,
                              conan_streams** out) {
  return guarded([&] {
    if (!ctx || !out) throw Error(CONAN_ERR_INVALID, "null argument");
    int arith = CONAN_ARITH_AUTO, flags = 0;
    if (opts) {
      if (opts->abi_version != CONAN_HIP_ABI_VERSION) throw Error(CONAN_ERR_INVALID, "conan_streams_opts.abi_version mismatch");
      for (int r : opts->reserved) if (r != 0) throw Error(CONAN_ERR_INVALID, "conan_streams_opts.reserved must be 0");
      arith = opts->arith; flags = opts->flags;
      if (opts->reserved0 != 0) throw Error(CONAN_ERR_INVALID, "conan_streams_opts.reserved0 must be 0");
      if (flags & ~(CONAN_STREAMS_FUSED_DECODER_BLOCKS | CONAN_STREAMS_SEPARATE_SMALL_STEPS | CONAN_STREAMS_FIXED_PLAN | CONAN_STREAMS_SHARED_DEVICE)) throw Error(CONAN_ERR_INVALID, "conan_streams_opts.flags: unknown bits");
      if (arith != CONAN_ARITH_AUTO && arith != CONAN_ARITH_F32 && arith != CONAN_ARITH_LIMB) throw Error(CONAN_ERR_INVALID, "conan_streams_opts.arith: 0 (auto), 1 (f32) or 2 (limb)");
    }
    if (!ctx->finalized) throw Error(CONAN_ERR_STATE, "conan_ctx_finalize must run before conan_streams_create");
    if (max_slots < 1 || max_frames < 1) throw Error(CONAN_ERR_INVALID, "max_slots / max_frames");
    HIP_CHECK(hipSetDevice(ctx->device));
    conan_streams* s = new conan_streams(plan::resolve(opts ? opts->dev_plan : nullptr));      // (an unknown switch name: CONAN_ERR_INVALID, nothing allocated)
    const plan::PlanSwitches& sw = s->sw;
    try {
      s->fixed_plan = (flags & CONAN_STREAMS_FIXED_PLAN) != 0; s->shared_device = (flags & CONAN_STREAMS_SHARED_DEVICE) != 0;
      s->ctx = ctx; s->live = &device_live_streams(ctx->device); s->live->fetch_add(1); s->max_slots = max_slots; s->max_frames = std::max(max_frames, ctx->cfg.emf_segment); s->max_ref = std::max(4, max_ref_frames);
      s->d_slots = (int*)s->alloc(max_slots + cnk::kSlotTablePad); s->d_ident = (int*)s->alloc(max_slots + 1); s->d_zero = (int*)s->alloc(max_slots);
      s->d_lens = (int*)s->alloc(max_slots); s->d_lens2 = (int*)s->alloc(max_slots);
      s->d_codes = (int*)s->alloc((size_t)max_slots * s->max_frames * 2);
      s->sk_slab_floats = 8ll << 20; s->sk_max_tiles = 4096;
      for (int w = 0; w < 3; ++w) { s->sk_slab[w] = s->alloc((size_t)s->sk_slab_floats); s->sk_counters[w] = (int*)s->alloc(s->sk_max_tiles); }
      for (int w = 0; w < 2; ++w) s->rb_sched[w] = (int*)s->alloc(4);
      for (int w = 0; w < 3; ++w) s->cp_ticket[w] = (int*)s->alloc(4);
      // fp32 products of the vocoder's matrix kernels as six bf16 limb products (resblock_limb.hip, conv_limb.hip) or on the
      // f32-input MFMA: conan_streams_opts.arith.  AUTO = the limb form wherever the context packed limb weights (ResBlock1
      // vocoders); the developer switch RB_NOLIMB turns AUTO into F32 for A/B runs - it never overrides an explicit request.
      if (arith == CONAN_ARITH_LIMB && !((ctx->cfg.models & CONAN_MODEL_HIFIGAN) && ctx->has_limb_weights))
        throw Error(CONAN_ERR_UNSUPPORTED, "arith = limb: this context holds no bf16-limb weights (no HiFi-GAN model, or a vocoder configuration without limb kernels)");
      s->arith_auto = arith == CONAN_ARITH_AUTO;
      s->rb_limb = arith == CONAN_ARITH_LIMB || (arith == CONAN_ARITH_AUTO && ctx->has_limb_weights && !sw.rb_nolimb);
      // deployment flags (conan_streams_opts.flags)
      s->opt_flags = flags;
      s->mega_single = !(s->opt_flags & CONAN_STREAMS_SEPARATE_SMALL_STEPS);
      // (a CU-masked front-end stream - developer switch - cannot hold the megakernel's grid resident: its barriers would never complete)
      s->use_mega = sw.dec_mega && sw.front_custride < 2;
      s->mega_grid = plan::mega_grid(sw, ctx->num_cu);
      s->mega_bar = reinterpret_cast<unsigned*>(s->alloc(16 * (size_t)(ctx->num_cu + 2)));
      s->mega_x = reinterpret_cast<unsigned*>(s->alloc(256 + 32 * 64));

      {  // guard block of the bounded waits: [0] code, [2..3] device address of the host-mapped copy
        HIP_CHECK(hipHostMalloc((void**)&s->h_guard, 64, hipHostMallocMapped));
        memset(s->h_guard, 0, 64);
        unsigned* hdev = nullptr;
        HIP_CHECK(hipHostGetDevicePointer((void**)&hdev, s->h_guard, 0));
        s->d_guard = reinterpret_cast<unsigned*>(s->alloc(16));
        HIP_CHECK(hipMemcpy(s->d_guard + 2, &hdev, sizeof(hdev), hipMemcpyHostToDevice));
      }
      s->slot_seen.assign(max_slots, 0); s->has_ref.assign(max_slots, 0); s->voice_of.assign(max_slots, -1); s->voc_fresh.assign(max_slots, 1); s->wav_out.voc_samples.assign(max_slots, 0); s->wav_in.in_fmt.assign(max_slots, 0); s->wav_out.out_fmt.assign(max_slots, 0);
      s->pin.init((size_t)max_slots + cnk::kSlotTablePad);
      s->pos_emf = (int*)s->alloc(max_slots); s->pos_dec = (int*)s->alloc(max_slots); s->pos_voc = (int*)s->alloc(max_slots);
      std::vector<int> id(max_slots);
      for (int i = 0; i < max_slots; ++i) id[i] = i;
      HIP_CHECK(hipMemcpy(s->d_ident, id.data(), max_slots * sizeof(int), hipMemcpyHostToDevice));
      s->wav_in.fe_slot.assign(max_slots, conan_streams::FeSlot());
      if ((ctx->cfg.models & 7) == 7) {     // streaming front-end rings, sized for fft_size <= 2048 at the vocoder's hop
        const int seg = ctx->cfg.emf_segment, rc = ctx->cfg.emf_right_context, hop = ctx->hop;
        s->wav_in.fe_LA = ch::next_pow2(2048 + seg * hop);
        s->wav_in.fe_LM = ch::next_pow2(2 * (seg + rc) + seg + 2048 / hop + 4);
        s->wav_in.fe_audio = s->alloc((size_t)max_slots * s->wav_in.fe_LA);
        s->wav_in.fe_mel = s->alloc((size_t)max_slots * s->wav_in.fe_LM * ctx->cfg.emf_input_dim);
        s->wav_in.fe_chunk = s->alloc((size_t)max_slots * (seg + rc) * ctx->cfg.emf_input_dim);
      }
      if (ctx->cfg.models & CONAN_MODEL_HIFIGAN) s->build_vocoder();
      if (ctx->cfg.models & CONAN_MODEL_EMFORMER) s->build_emformer();
      if (ctx->cfg.models & CONAN_MODEL_CONAN) s->build_decoder();
    } catch (...) { delete s; throw; }
    *out = s;
  });
}

int conan_streams_destroy(conan_streams* s) {
  return guarded([&] { if (s) { (void)hipDeviceSynchronize(); delete s; } });
}

int conan_streams_reset(conan_streams* s, const int32_t* slots, int n, int which, void* stream) {
  return guarded([&] {
    if (!s || !slots) throw Error(CONAN_ERR_INVALID, "null argument");
    hipStream_t st = (hipStream_t)stream;
    HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
    s->join((hipStream_t)stream);
    s->set_slots(slots, n, st);
    const int models = s->ctx->cfg.models & which;
    auto zero = [&](std::vector<std::pair<float*, long long>>& v, int* pos) {
      for (auto& b : v) cnk::launch_zero_slots(b.first, b.second, b.second, s->d_slots, n, st);
      cnk::launch_fill_int(pos, s->d_slots, n, 0, st);
    };
    if (models & CONAN_MODEL_HIFIGAN) {
      zero(s->voc_state, s->pos_voc);
      for (int i = 0; i < n; ++i) s->voc_fresh[slots[i]] = 1;
      // the output rate stays; the output resampler restarts (output index 0, inputs before the first are zero: the ring needs no clearing)
      for (int i = 0; i < n; ++i) s->wav_out.voc_samples[slots[i]] = 0;
      s->wm.restart(slots, n);      // the watermark's setting stays; its state restarts in the slots' next step rows
      s->out_eq.restart(slots, n);  // ... and the output equaliser's
      if (!s->wav_out.or_slot.empty())
        for (int i = 0; i < n; ++i) { conan_streams::OrSlot& o = s->wav_out.or_slot[slots[i]]; o.out = 0; o.flushed = 0; o.dr.restart(); }
    }
    if (models & CONAN_MODEL_EMFORMER) zero(s->emf_state, s->pos_emf);
    if (models & CONAN_MODEL_CONAN) zero(s->dec_state, s->pos_dec);
    if ((which & CONAN_MODEL_FRONTEND) && s->wav_in.fe_audio) {
      cnk::launch_zero_slots(s->wav_in.fe_audio, s->wav_in.fe_LA, s->wav_in.fe_LA, s->d_slots, n, st);
      const long long mel_floats = (long long)s->wav_in.fe_LM * s->ctx->cfg.emf_input_dim;
      cnk::launch_zero_slots(s->wav_in.fe_mel, mel_floats, mel_floats, s->d_slots, n, st);
      for (int i = 0; i < n; ++i) s->wav_in.fe_slot[slots[i]] = conan_streams::FeSlot();
      // the input rate stays; the resampler's history restarts (inputs before the first are zero, the ring needs no clearing)
      if (!s->wav_in.rs_slot.empty())
        for (int i = 0; i < n; ++i) { conan_streams::RsSlot& r = s->wav_in.rs_slot[slots[i]]; r.in = 0; r.out = 0; r.phase = 0; r.dr.restart(); }
      // the features' settings stay; their states restart in the slots' next rows
      s->restart_features(slots, n);
    }
  });
}

int conan_set_reference(conan_streams* s, const int32_t* slots, int n, const float* ref_mel_dev, const int32_t* ref_len,
                        int max_len, void* stream) {
  return guarded([&] {
    if (!s || !slots || !ref_mel_dev || !ref_len) throw Error(CONAN_ERR_INVALID, "null argument (the reference raises ValueError when ref is None)");
    if (!(s->ctx->cfg.models & CONAN_MODEL_CONAN)) throw Error(CONAN_ERR_STATE, "context holds no Conan model");
    if (n < 1 || n > s->max_slots) throw Error(CONAN_ERR_INVALID, "slot count out of range");
    HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
    s->join((hipStream_t)stream);
    s->set_reference(slots, n, ref_mel_dev, ref_len, max_len, (hipStream_t)stream);
  });
}

int conan_emformer_step(conan_streams* s, const int32_t* slots, int n, const float* chunk_dev, float* out_dev, float* logits_dev,
                        int32_t* codes_dev, void* stream) {
  return guarded([&] {
    if (!s || !slots || !chunk_dev) throw Error(CONAN_ERR_INVALID, "null argument");
    if (!(s->ctx->cfg.models & CONAN_MODEL_EMFORMER)) throw Error(CONAN_ERR_STATE, "context holds no Emformer model");
    HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
    s->join((hipStream_t)stream);
    s->set_slots(slots, n, (hipStream_t)stream);
    s->emformer_step(n, chunk_dev, out_dev, logits_dev, codes_dev, (hipStream_t)stream);
  });
}

int conan_emformer_head_dim(conan_streams* s, const char* head) {
  int k = 0;
  const int rc = guarded([&] {
    if (!s || !head) throw Error(CONAN_ERR_INVALID, "null argument");
    auto it = s->ctx->convs.find(std::string("emf.head.") + head);
    k = it == s->ctx->convs.end() ? 0 : it->second.Cout;
  });
  return rc < 0 ? rc : k;
}

int conan_emformer_project(conan_streams* s, const char* head, const float* x_dev, int rows, float* y_dev, void* stream) {
  return guarded([&] {
    if (!s || !head || !x_dev || !y_dev) throw Error(CONAN_ERR_INVALID, "null argument");
    if (!(s->ctx->cfg.models & CONAN_MODEL_EMFORMER)) throw Error(CONAN_ERR_STATE, "context holds no Emformer model");
    if (rows <= 0) return;
    const std::string name = std::string("emf.head.") + head;
    if (!s->ctx->convs.count(name)) throw Error(CONAN_ERR_MISSING, std::string("the Emformer checkpoint holds no output head '") + head + "'");
    HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
    hipStream_t st = (hipStream_t)stream;
    s->join(st);
    const ch::PackedConv& pc = s->ctx->conv(name);
    // a Linear is a k = 1 conv over one "slot" of `rows` rows (conv_mfma; no ring, no slot table)
    s->conv(s->mk(pc, ch::lin_ref(const_cast<float*>(x_dev), rows, pc.Cin), ch::lin_ref(y_dev, rows, pc.Cout), 1, rows, nullptr), st);
  });
}

int conan_decoder_step(conan_streams* s, const int32_t* slots, int n, int frames, const int32_t* codes_dev, float* mel_out_dev,
                       float* uv_pred_dev, float* f0_dev, int32_t* bins_dev, float* decoder_inp_dev, void* stream) {
  return guarded([&] {
    if (!s || !slots || !codes_dev || !mel_out_dev) throw Error(CONAN_ERR_INVALID, "null argument");
    if (!(s->ctx->cfg.models & CONAN_MODEL_CONAN)) throw Error(CONAN_ERR_STATE, "context holds no Conan model");
    if (frames < 1 || frames > s->max_frames) throw Error(CONAN_ERR_INVALID, "frames out of range");
    HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
    s->join((hipStream_t)stream);
    s->set_slots(slots, n, (hipStream_t)stream);
    conan_decoder_taps taps; memset(&taps, 0, sizeof(taps));
    taps.uv_pred = uv_pred_dev; taps.f0_denorm_pred = f0_dev; taps.pitch_bins = bins_dev; taps.decoder_inp = decoder_inp_dev;
    s->decoder_step(n, frames, codes_dev, mel_out_dev, taps, (hipStream_t)stream);
  });
}

int conan_decoder_step_taps(conan_streams* s, const int32_t* slots, int n, int frames, const int32_t* codes_dev, float* mel_out_dev,
                            const conan_decoder_taps* taps, void* stream) {
  return guarded([&] {
    if (!s || !slots || !codes_dev || !mel_out_dev) throw Error(CONAN_ERR_INVALID, "null argument");
    if (!(s->ctx->cfg.models & CONAN_MODEL_CONAN)) throw Error(CONAN_ERR_STATE, "context holds no Conan model");
    if (frames < 1 || frames > s->max_frames) throw Error(CONAN_ERR_INVALID, "frames out of range");
    HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
    s->join((hipStream_t)stream);
    s->set_slots(slots, n, (hipStream_t)stream);
    conan_decoder_taps none; memset(&none, 0, sizeof(none));
    s->decoder_step(n, frames, codes_dev, mel_out_dev, taps ? *taps : none, (hipStream_t)stream);
  });
}

int conan_decoder_step_pitch(conan_streams* s, const int32_t* slots, int n, int frames, const int32_t* codes_dev, const float* f0_in_dev,
                             const float* uv_in_dev, float* mel_out_dev, const conan_decoder_taps* taps, void* stream) {
  return guarded([&] {
    if (!s || !slots || !codes_dev || !mel_out_dev) throw Error(CONAN_ERR_INVALID, "null argument");
    if (!(s->ctx->cfg.models & CONAN_MODEL_CONAN)) throw Error(CONAN_ERR_STATE, "context holds no Conan model");
    if (frames < 1 || frames > s->max_frames) throw Error(CONAN_ERR_INVALID, "frames out of range");
    HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
    s->join((hipStream_t)stream);
    s->set_slots(slots, n, (hipStream_t)stream);
    conan_decoder_taps none; memset(&none, 0, sizeof(none));
    conan_streams::DecExtra ex;      // (the contour pointers travel in PitchHeadArgs; a step without taps keeps the persistent launch)
    ex.f0_in = f0_in_dev; ex.uv_in = f0_in_dev ? uv_in_dev : nullptr;
    s->decoder_step(n, frames, codes_dev, mel_out_dev, taps ? *taps : none, (hipStream_t)stream, &ex);
  });
}

int conan_f0(conan_ctx* ctx, const conan_mel_cfg* mel, const conan_f0_cfg* cfg, const float* wav_dev, int n, int samples, float* f0_out_dev,
             float* uv_out_dev, int32_t* frames_out, void* stream) {
  return guarded([&] { f0::whole(ctx, mel, cfg, wav_dev, n, samples, f0_out_dev, uv_out_dev, frames_out, stream); });
}

int conan_streams_set_pitch_follow(conan_streams* s, const int32_t* slots, int n, const conan_f0_cfg* cfg, void* stream) {
  return guarded([&] { f0::set_follow(s, slots, n, cfg, stream); });
}

int conan_streams_pitch_follow(const conan_streams* s, int slot, conan_f0_cfg* out) { return guarded([&] { wavio::get_setting(s, &conan_streams::follow, slot, out, "conan_streams_pitch_follow"); }); }

int conan_step_wav_contour(conan_streams* s, float* f0_dev, float* uv_dev, void* stream) { return guarded([&] { f0::contour(s, f0_dev, uv_dev, stream); }); }

int conan_f0_register(conan_ctx* ctx, const conan_register_cfg* cfg, const float* f0_dev, const float* uv_dev, int n, const int32_t* frames, int64_t ld,
                      float* f0_out_dev, int64_t* state_out_dev, void* stream) {
  return guarded([&] { reg::whole(ctx, cfg, f0_dev, uv_dev, n, frames, ld, f0_out_dev, state_out_dev, stream); });
}

int conan_streams_set_pitch_register(conan_streams* s, const int32_t* slots, int n, const conan_register_cfg* cfg, void* stream) {
  return guarded([&] { reg::set_register(s, slots, n, cfg, stream); });
}

int conan_streams_pitch_register(const conan_streams* s, int slot, conan_register_cfg* cfg_out) { return guarded([&] { wavio::get_setting(s, &conan_streams::reg, slot, cfg_out, "conan_streams_pitch_register"); }); }

int conan_streams_pitch_register_state(conan_streams* s, const int32_t* slots, int n, int64_t* state_dev, void* stream) {
  return guarded([&] { reg::state(s, slots, n, state_dev, stream); });
}

int conan_activity(conan_ctx* ctx, const conan_mel_cfg* mel, const conan_activity_cfg* cfg, const float* wav_dev, int n, int samples, int32_t* act_out_dev,
                   int32_t* level_out_dev, double* power_out_dev, conan_activity_state* state_out_dev, int32_t* frames_out, void* stream) {
  return guarded([&] { act::whole(ctx, mel, cfg, wav_dev, n, samples, act_out_dev, level_out_dev, power_out_dev, state_out_dev, frames_out, stream); });
}

int conan_activity_gate(conan_ctx* ctx, int hop, const float* wav_dev, int n, int64_t samples, int64_t ld, const int32_t* level_dev, int64_t level_ld,
                        int32_t start_level, float* out_dev, void* stream) {
  return guarded([&] { act::gate(ctx, hop, wav_dev, n, samples, ld, level_dev, level_ld, start_level, out_dev, stream); });
}

int conan_streams_set_activity(conan_streams* s, const int32_t* slots, int n, const conan_activity_cfg* cfg, void* stream) {
  return guarded([&] { act::set_activity(s, slots, n, cfg, stream); });
}

int conan_streams_activity(const conan_streams* s, int slot, conan_activity_cfg* cfg_out) { return guarded([&] { wavio::get_setting(s, &conan_streams::act, slot, cfg_out, "conan_streams_activity"); }); }

int conan_streams_activity_state(conan_streams* s, const int32_t* slots, int n, conan_activity_state* state_dev, void* stream) {
  return guarded([&] { act::state(s, slots, n, state_dev, stream); });
}

int conan_step_wav_activity(conan_streams* s, int32_t* act_dev, int32_t* level_dev, void* stream) {
  return guarded([&] { act::last_call(s, act_dev, level_dev, stream); });
}

int conan_streams_set_bypass(conan_streams* s, const int32_t* slots, int n, const conan_bypass_cfg* cfg, void* stream) {
  return guarded([&] { byp::set_bypass(s, slots, n, cfg, stream); });
}

int conan_streams_bypass(const conan_streams* s, int slot, conan_bypass_cfg* cfg_out) { return guarded([&] { wavio::get_setting(s, &conan_streams::byp, slot, cfg_out, "conan_streams_bypass"); }); }

int conan_streams_bypass_state(conan_streams* s, const int32_t* slots, int n, conan_bypass_state* state_dev, void* stream) {
  return guarded([&] { byp::state(s, slots, n, state_dev, stream); });
}

int conan_step_wav_bypass(conan_streams* s, int32_t* wet_lvl_dev, int32_t* dry_lvl_dev, void* stream) {
  return guarded([&] { byp::last_call(s, wet_lvl_dev, dry_lvl_dev, stream); });
}

int conan_streams_set_comfort(conan_streams* s, const int32_t* slots, int n, const conan_comfort_cfg* cfg, void* stream) {
  return guarded([&] { comfort::set_comfort(s, slots, n, cfg, stream); });
}

int conan_streams_comfort(const conan_streams* s, int slot, conan_comfort_cfg* cfg_out) { return guarded([&] { wavio::get_setting(s, &conan_streams::cmf, slot, cfg_out, "conan_streams_comfort"); }); }

int conan_streams_comfort_state(conan_streams* s, const int32_t* slots, int n, conan_comfort_state* state_dev, void* stream) {
  return guarded([&] { comfort::state(s, slots, n, state_dev, stream); });
}

int conan_step_wav_comfort(conan_streams* s, int32_t* level_dev, void* stream) { return guarded([&] { comfort::last_call(s, level_dev, stream); }); }

int conan_comfort_track(conan_ctx* ctx, const conan_comfort_cfg* cfg, const int32_t* act_dev, const double* power_dev, int n, int64_t frames, int64_t ld,
                        int32_t* level_out_dev, conan_comfort_state* state_out_dev, void* stream) {
  return guarded([&] { comfort::track(ctx, cfg, act_dev, power_dev, n, frames, ld, level_out_dev, state_out_dev, stream); });
}

int conan_comfort_fill(conan_ctx* ctx, int hop, const conan_comfort_cfg* cfg, const uint64_t* seeds, const float* wav_dev, int64_t ld, int n, int64_t samples,
                       int64_t pos0, const int32_t* gate_lvl_dev, const int32_t* comfort_lvl_dev, int64_t lvl_ld, int32_t start_gate_level,
                       int32_t start_comfort_level, float* out_dev, int64_t out_ld, void* stream) {
  return guarded([&] {
    comfort::fill(ctx, hop, cfg, seeds, wav_dev, ld, n, samples, pos0, gate_lvl_dev, comfort_lvl_dev, lvl_ld, start_gate_level, start_comfort_level, out_dev, out_ld, stream);
  });
}

int conan_bypass_mix(conan_ctx* ctx, int hop, const float* wet_dev, int64_t wet_ld, const float* dry_dev, int64_t dry_ld, int n, int64_t samples,
                     const int32_t* wet_lvl_dev, const int32_t* dry_lvl_dev, int64_t lvl_ld, int32_t start_wet, int32_t start_dry, float* out_dev,
                     int64_t out_ld, void* stream) {
  return guarded([&] { byp::mix(ctx, hop, wet_dev, wet_ld, dry_dev, dry_ld, n, samples, wet_lvl_dev, dry_lvl_dev, lvl_ld, start_wet, start_dry, out_dev, out_ld, stream); });
}

int conan_trim_silence(conan_ctx* ctx, const conan_mel_cfg* mel, const conan_activity_cfg* act_cfg, const conan_trim_cfg* cfg, const float* wav_dev, int64_t ld,
                       int n, int64_t samples, const int64_t* lengths, const int32_t* act_in_dev, int64_t act_ld, float* out_dev, int64_t out_ld,
                       int32_t* mask_out_dev, int64_t* offset_out_dev, int64_t frame_ld, int64_t* out_len_dev, void* stream) {
  return guarded([&] {
    trim::whole(ctx, mel, act_cfg, cfg, wav_dev, ld, n, samples, lengths, act_in_dev, act_ld, out_dev, out_ld, mask_out_dev, offset_out_dev, frame_ld, out_len_dev,
                stream);
  });
}

int conan_streams_set_pitch(conan_streams* s, const int32_t* slots, int n, const conan_pitch_cfg* cfg, void* stream) {
  return guarded([&] { pitch::set_pitch(s, slots, n, cfg, stream); });
}

int conan_streams_pitch(const conan_streams* s, int slot, conan_pitch_cfg* out) { return guarded([&] { pitch::get_pitch(s, slot, out); }); }

int conan_get_style(conan_streams* s, const int32_t* slots, int n, float* style_dev, int32_t* max_tokens_out, void* stream) {
  return guarded([&] {
    if (!s || !slots || !style_dev) throw Error(CONAN_ERR_INVALID, "null argument");
    if (!(s->ctx->cfg.models & CONAN_MODEL_CONAN)) throw Error(CONAN_ERR_STATE, "context holds no Conan model");
    if (n < 1 || n > s->max_slots) throw Error(CONAN_ERR_INVALID, "slot count out of range");
    for (int i = 0; i < n; ++i) {
      if (slots[i] < 0 || slots[i] >= s->max_slots) throw Error(CONAN_ERR_INVALID, "slot index out of range");
      if (!s->has_ref[slots[i]]) throw Error(CONAN_ERR_STATE, "conan_get_style before conan_set_reference");
    }
    HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
    s->join((hipStream_t)stream);
    const int H = s->ctx->cfg.hidden_size;
    for (int i = 0; i < n; ++i) {
      if (slots[i] < 0 || slots[i] >= s->max_slots) throw Error(CONAN_ERR_INVALID, "slot index out of range");
      HIP_CHECK(hipMemcpyAsync(style_dev + (size_t)i * H, s->c_style + (size_t)slots[i] * H, (size_t)H * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    if (max_tokens_out) *max_tokens_out = s->S_max;
  });
}

int conan_set_style(conan_streams* s, const int32_t* slots, int n, const float* style_dev, void* stream) {
  return guarded([&] {
    if (!s || !slots || !style_dev) throw Error(CONAN_ERR_INVALID, "null argument");
    if (!(s->ctx->cfg.models & CONAN_MODEL_CONAN)) throw Error(CONAN_ERR_STATE, "context holds no Conan model");
    HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
    s->join((hipStream_t)stream);
    s->set_slots(slots, n, (hipStream_t)stream);
    for (int i = 0; i < n; ++i)
      if (!s->has_ref[slots[i]]) throw Error(CONAN_ERR_STATE, "conan_set_style before conan_set_reference (the prosody tokens come from the reference mel)");
    cnk::launch_scatter_rows(s->c_style, style_dev, s->d_slots, n, s->ctx->cfg.hidden_size, (hipStream_t)stream);
    for (int i = 0; i < n; ++i) s->voice_of[slots[i]] = -1;
  });
}

int conan_get_prosody_ids(conan_streams* s, const int32_t* slots, int n, int32_t* ids_dev, int32_t* count_dev, void* stream) {
  return guarded([&] {
    if (!s || !slots || !ids_dev) throw Error(CONAN_ERR_INVALID, "null argument");
    if (!(s->ctx->cfg.models & CONAN_MODEL_CONAN)) throw Error(CONAN_ERR_STATE, "context holds no Conan model");
    HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
    s->join((hipStream_t)stream);
    s->set_slots(slots, n, (hipStream_t)stream);
    for (int i = 0; i < n; ++i)
      if (!s->has_ref[slots[i]]) throw Error(CONAN_ERR_STATE, "conan_get_prosody_ids before conan_set_reference");
    cnk::launch_gather_ids(ids_dev, count_dev, s->c_vqids, s->c_slen, s->d_slots, n, s->S_max, (hipStream_t)stream);
  });
}

int conan_hifigan_step_taps(conan_streams* s, const int32_t* slots, int n, int frames, const float* mel_dev, float* wav_out_dev,
                            float* pre_tanh_dev, const conan_hifigan_taps* taps, void* stream) {
  return guarded([&] {
    if (!s || !slots || !mel_dev || !wav_out_dev) throw Error(CONAN_ERR_INVALID, "null argument");
    if (!(s->ctx->cfg.models & CONAN_MODEL_HIFIGAN)) throw Error(CONAN_ERR_STATE, "context holds no HiFi-GAN model");
    if (frames < 1 || frames > s->max_frames) throw Error(CONAN_ERR_INVALID, "frames out of range");
    HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
    const conan_streams::OutPlan op = s->out_plan(slots, n, frames, wav_out_dev, (long long)frames * s->ctx->hop, nullptr, "conan_hifigan_step_taps");
    s->join((hipStream_t)stream);
    s->set_slots(slots, n, (hipStream_t)stream);
    s->hifigan_step(n, frames, mel_dev, wav_out_dev, pre_tanh_dev, (hipStream_t)stream, taps, &op);
  });
}

int conan_hifigan_step(conan_streams* s, const int32_t* slots, int n, int frames, const float* mel_dev, float* wav_out_dev,
                       float* pre_tanh_dev, void* stream) {
  return guarded([&] {
    if (!s || !slots || !mel_dev || !wav_out_dev) throw Error(CONAN_ERR_INVALID, "null argument");
    if (!(s->ctx->cfg.models & CONAN_MODEL_HIFIGAN)) throw Error(CONAN_ERR_STATE, "context holds no HiFi-GAN model");
    if (frames < 1 || frames > s->max_frames) throw Error(CONAN_ERR_INVALID, "frames out of range");
    HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
    const conan_streams::OutPlan op = s->out_plan(slots, n, frames, wav_out_dev, (long long)frames * s->ctx->hop, nullptr, "conan_hifigan_step");
    s->join((hipStream_t)stream);
    s->set_slots(slots, n, (hipStream_t)stream);
    s->hifigan_step(n, frames, mel_dev, wav_out_dev, pre_tanh_dev, (hipStream_t)stream, nullptr, &op);
  });
}

int conan_step(conan_streams* s, const int32_t* slots, int n, int emit, const float* mel_chunk_dev, int32_t* codes_dev,
               float* mel_out_dev, float* wav_out_dev, void* stream) {
  return guarded([&] {
    if (!s || !slots || !mel_chunk_dev || !wav_out_dev) throw Error(CONAN_ERR_INVALID, "null argument");
    check_chunk_step(s, "conan_step");
    const int seg = s->ctx->cfg.emf_segment;
    if (emit < 1 || emit > seg) throw Error(CONAN_ERR_INVALID, "emit must be in [1, segment]");
    hipStream_t st = (hipStream_t)stream;
    HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
    const conan_streams::OutPlan op = s->out_plan(slots, n, emit, wav_out_dev, (long long)emit * s->ctx->hop, nullptr, "conan_step");
    s->join((hipStream_t)stream);
    s->set_slots(slots, n, st);
    step_blocking(s, n, emit, mel_chunk_dev, codes_dev, mel_out_dev, wav_out_dev, st, op);
  });
}

// Pipelined variant of conan_step.  Within one stream-set the three stages of a chunk are strictly ordered, but the
// front-end of the next chunk depends only on front-end state, so it runs on its own HIP stream while the vocoder of
// this chunk is still busy on another: the ~60 latency-bound front-end launches fill the gaps of the vocoder's large
// kernels instead of adding to the step time.
int conan_step_async(conan_streams* s, const int32_t* slots, int n, int emit, const float* mel_chunk_dev, int32_t* codes_dev,
                     float* mel_out_dev, float* wav_out_dev, void* stream) {
  return guarded([&] {
    if (!s || !slots || !mel_chunk_dev || !wav_out_dev) throw Error(CONAN_ERR_INVALID, "null argument");
    check_chunk_step(s, "conan_step_async");
    const int seg = s->ctx->cfg.emf_segment;
    if (emit < 1 || emit > seg) throw Error(CONAN_ERR_INVALID, "emit must be in [1, segment]");
    if (s->prof_on) throw Error(CONAN_ERR_STATE, "profiling is not available for pipelined steps");
    const conan_streams::OutPlan op = s->out_plan(slots, n, emit, wav_out_dev, (long long)emit * s->ctx->hop, nullptr, "conan_step_async");
    step_pipelined(s, slots, n, emit, mel_chunk_dev, codes_dev, mel_out_dev, wav_out_dev, stream, nullptr, op);
  });
}

int conan_step_wav(conan_streams* s, const int32_t* slots, int n, int samples, int final, const float* wav_dev, const conan_mel_cfg* mel,
                   int32_t* codes_dev, float* mel_out_dev, float* wav_out_dev, int32_t* emit_out, void* stream) {
  return guarded([&] { wavio::step_wav_common(s, slots, n, samples, final, wav_dev, mel, codes_dev, mel_out_dev, wav_out_dev, emit_out, stream, false); });
}

int conan_step_wav_async(conan_streams* s, const int32_t* slots, int n, int samples, int final, const float* wav_dev, const conan_mel_cfg* mel,
                         int32_t* codes_dev, float* mel_out_dev, float* wav_out_dev, int32_t* emit_out, void* stream) {
  return guarded([&] { wavio::step_wav_common(s, slots, n, samples, final, wav_dev, mel, codes_dev, mel_out_dev, wav_out_dev, emit_out, stream, true); });
}

static long long ragged_ld(const conan_streams* s) { return s ? (long long)s->ctx->cfg.emf_segment * s->ctx->hop : 0; }

int conan_step_wav_ragged(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, const int32_t* final, const float* wav_dev,
                          const conan_mel_cfg* mel, int32_t* codes_dev, float* mel_out_dev, float* wav_out_dev, int32_t* emit_out, void* stream) {
  return guarded([&] { wavio::step_wav(s, "conan_step_wav_ragged", slots, n, samples, final, wav_dev, ragged_ld(s), mel, codes_dev, mel_out_dev, wav_out_dev, emit_out, stream, false, false); });
}

int conan_step_wav_ragged_async(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, const int32_t* final, const float* wav_dev,
                                const conan_mel_cfg* mel, int32_t* codes_dev, float* mel_out_dev, float* wav_out_dev, int32_t* emit_out, void* stream) {
  return guarded([&] { wavio::step_wav(s, "conan_step_wav_ragged", slots, n, samples, final, wav_dev, ragged_ld(s), mel, codes_dev, mel_out_dev, wav_out_dev, emit_out, stream, true, false); });
}

int conan_step_wav_ragged_ld(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, const int32_t* final, const float* wav_dev,
                             int64_t wav_ld, const conan_mel_cfg* mel, int32_t* codes_dev, float* mel_out_dev, float* wav_out_dev,
                             int32_t* emit_out, void* stream) {
  return guarded([&] { wavio::step_wav(s, "conan_step_wav_ragged", slots, n, samples, final, wav_dev, wav_ld, mel, codes_dev, mel_out_dev, wav_out_dev, emit_out, stream, false, false); });
}

int conan_step_wav_ragged_ld_async(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, const int32_t* final,
                                   const float* wav_dev, int64_t wav_ld, const conan_mel_cfg* mel, int32_t* codes_dev, float* mel_out_dev,
                                   float* wav_out_dev, int32_t* emit_out, void* stream) {
  return guarded([&] { wavio::step_wav(s, "conan_step_wav_ragged", slots, n, samples, final, wav_dev, wav_ld, mel, codes_dev, mel_out_dev, wav_out_dev, emit_out, stream, true, false); });
}

int conan_resample(conan_ctx* ctx, const conan_resample_cfg* cfg, const float* x_dev, int n, int64_t samples, float* y_dev, int64_t* out_samples,
                   void* stream) {
  return guarded([&] {
    if (!ctx || !cfg || !x_dev || !y_dev) throw Error(CONAN_ERR_INVALID, "null argument");
    HIP_CHECK(hipSetDevice(ctx->device));
    conan_ctx_resample(ctx, *cfg, x_dev, n, samples, y_dev, out_samples, (hipStream_t)stream);
  });
}

int conan_resample_drift(conan_ctx* ctx, const conan_resample_cfg* cfg, int side, const float* x_dev, int n, int64_t samples, const int64_t* at,
                         const int32_t* ppb, int n_seg, float* y_dev, int64_t y_ld, int64_t* out_samples, void* stream) {
  return guarded([&] {
    if (!ctx || !cfg || !x_dev || !y_dev || !at || !ppb) throw Error(CONAN_ERR_INVALID, "null argument");
    HIP_CHECK(hipSetDevice(ctx->device));
    conan_ctx_resample_drift(ctx, *cfg, side, x_dev, n, samples, at, ppb, n_seg, y_dev, y_ld, out_samples, (hipStream_t)stream);
  });
}

int64_t conan_resample_drift_table(const conan_resample_cfg* cfg, int32_t* W, float* table, int64_t cap) {
  try {      // (host only, and no launch to answer for: it also runs where no device is)
    if (!cfg) throw Error(CONAN_ERR_INVALID, "null argument");
    return conan_ctx_resample_drift_table(*cfg, W, table, cap);
  } catch (const ch::Error& e) {
    g_err = e.what();
    return e.code;
  }
}

int conan_loud_norm(conan_ctx* ctx, const conan_loudness_cfg* cfg, const float* x_dev, int64_t x_ld, int n, const int64_t* samples, float* y_dev,
                    int64_t y_ld, double* stats_dev, void* stream) {
  return guarded([&] {
    if (!ctx || !cfg || !x_dev || !samples) throw Error(CONAN_ERR_INVALID, "null argument");
    HIP_CHECK(hipSetDevice(ctx->device));
    conan_ctx_loud_norm(ctx, *cfg, x_dev, x_ld, n, samples, y_dev, y_ld, stats_dev, (hipStream_t)stream);
  });
}

int conan_level(conan_ctx* ctx, const conan_level_cfg* cfg, const float* x_dev, int64_t x_ld, int n, const int64_t* samples, float* y_dev, int64_t y_ld,
                double* trace_dev, int64_t trace_ld, void* stream) {
  return guarded([&] {
    if (!ctx || !cfg || !x_dev || !samples || !y_dev) throw Error(CONAN_ERR_INVALID, "null argument");
    level::check_cfg(*cfg, "conan_level");      // (before any GPU use)
    if (!cfg->enabled) throw Error(CONAN_ERR_INVALID, "conan_level: cfg.enabled must be 1");
    HIP_CHECK(hipSetDevice(ctx->device));
    conan_ctx_level(ctx, *cfg, x_dev, x_ld, n, samples, y_dev, y_ld, trace_dev, trace_ld, (hipStream_t)stream);
  });
}

int conan_streams_set_input_level(conan_streams* s, const int32_t* slots, int n, const conan_level_cfg* cfg) {
  return guarded([&] { level::set_input_level(s, slots, n, cfg); });
}

int conan_streams_input_level(conan_streams* s, const int32_t* slots, int n, double* stats_dev, void* stream) {
  return guarded([&] { level::input_level(s, slots, n, stats_dev, stream); });
}

int conan_streams_set_output_level(conan_streams* s, const int32_t* slots, int n, const conan_level_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream) {
  return guarded([&] { olv::set_level(s, slots, n, cfg, seed_dev, seed_ld, stream); });
}

int conan_streams_output_level_cfg(const conan_streams* s, int slot, conan_level_cfg* cfg_out) { return guarded([&] { wavio::get_setting(s, &conan_streams::out_lv, slot, cfg_out, nullptr); }); }

int conan_streams_output_level(conan_streams* s, const int32_t* slots, int n, double* stats_dev, void* stream) {
  return guarded([&] { olv::stats(s, slots, n, stats_dev, stream); });
}

int64_t conan_streams_output_level_state_bytes(const conan_streams* s) {
  int64_t b = 0;
  const int rc = guarded([&] { b = olv::state_bytes(s); });
  return rc < 0 ? rc : b;
}

int conan_streams_output_level_state(conan_streams* s, const int32_t* slots, int n, void* state_dev, int64_t ld, void* stream) {
  return guarded([&] { olv::state(s, slots, n, state_dev, ld, stream); });
}

int conan_streams_set_conceal(conan_streams* s, const int32_t* slots, int n, const conan_conceal_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream) {
  return guarded([&] { conc::set_conceal(s, slots, n, cfg, seed_dev, seed_ld, stream); });
}

int conan_streams_conceal_cfg(const conan_streams* s, int slot, conan_conceal_cfg* cfg_out) { return guarded([&] { wavio::get_setting(s, &conan_streams::conc, slot, cfg_out, nullptr); }); }

int conan_streams_conceal(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, void* wav_dev, int64_t wav_ld, const int32_t* lost_dev,
                          int64_t lost_ld, void* stream) {
  return guarded([&] { conc::repair(s, slots, n, samples, wav_dev, wav_ld, lost_dev, lost_ld, stream); });
}

int64_t conan_conceal_state_bytes(void) { return (int64_t)cnk::kConcStateBytes; }

int conan_streams_conceal_state(conan_streams* s, const int32_t* slots, int n, void* state_dev, int64_t ld, void* stream) {
  return guarded([&] { conc::state(s, slots, n, state_dev, ld, stream); });
}

int conan_conceal(conan_ctx* ctx, const conan_conceal_cfg* cfg, int format, void* x_dev, int64_t ld, int n, const int64_t* samples, const int32_t* lost_dev,
                  int64_t lost_ld, void* stream) {
  return guarded([&] { conc::whole(ctx, cfg, format, x_dev, ld, n, samples, lost_dev, lost_ld, stream); });
}

// ---- echo cancellation (echo.hip): conan_streams_set_echo, conan_streams_echo_cfg, conan_streams_echo, conan_echo_state_bytes,
// conan_streams_echo_state, conan_echo
int conan_streams_set_echo(conan_streams* s, const int32_t* slots, int n, const conan_echo_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream) {
  return guarded([&] { echo::set_echo(s, slots, n, cfg, seed_dev, seed_ld, stream); });
}

int conan_streams_echo_cfg(const conan_streams* s, int slot, conan_echo_cfg* cfg_out) { return guarded([&] { wavio::get_setting(s, &conan_streams::ec, slot, cfg_out, nullptr); }); }

int conan_streams_echo(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, void* wav_dev, int64_t wav_ld, const void* far_dev,
                       int64_t far_ld, int64_t* stats_dev, void* stream) {
  return guarded([&] { echo::cancel(s, slots, n, samples, wav_dev, wav_ld, far_dev, far_ld, stats_dev, stream); });
}

int64_t conan_echo_state_bytes(void) { return (int64_t)cnk::kEchoStateBytes; }

int conan_streams_echo_state(conan_streams* s, const int32_t* slots, int n, void* state_dev, int64_t ld, void* stream) {
  return guarded([&] { echo::state(s, slots, n, state_dev, ld, stream); });
}

int conan_echo(conan_ctx* ctx, const conan_echo_cfg* cfg, int format, void* x_dev, int64_t ld, const void* far_dev, int64_t far_ld, int n,
               const int64_t* samples, int64_t* stats_dev, void* stream) {
  return guarded([&] { echo::whole(ctx, cfg, format, x_dev, ld, far_dev, far_ld, n, samples, stats_dev, stream); });
}

// ---- echo delay (echo_delay.hip): conan_streams_set_echo_delay, conan_streams_echo_delay_cfg, conan_streams_echo_delay,
// conan_echo_delay_state_bytes, conan_streams_echo_delay_state, conan_echo_delay
int conan_streams_set_echo_delay(conan_streams* s, const int32_t* slots, int n, const conan_echo_delay_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream) {
  return guarded([&] { echo_delay::set_echo_delay(s, slots, n, cfg, seed_dev, seed_ld, stream); });
}

int conan_streams_echo_delay_cfg(const conan_streams* s, int slot, conan_echo_delay_cfg* cfg_out) {
  return guarded([&] { wavio::get_setting(s, &conan_streams::ed, slot, cfg_out, nullptr); });
}

int conan_streams_echo_delay(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, const void* wav_dev, int64_t wav_ld, const void* far_dev,
                             int64_t far_ld, int64_t* report_dev, void* stream) {
  return guarded([&] { echo_delay::estimate(s, slots, n, samples, wav_dev, wav_ld, far_dev, far_ld, report_dev, stream); });
}

int64_t conan_echo_delay_state_bytes(void) { return (int64_t)cnk::kEdStateBytes; }

int conan_streams_echo_delay_state(conan_streams* s, const int32_t* slots, int n, void* state_dev, int64_t ld, void* stream) {
  return guarded([&] { echo_delay::state(s, slots, n, state_dev, ld, stream); });
}

int conan_echo_delay(conan_ctx* ctx, const conan_echo_delay_cfg* cfg, int format, const void* mic_dev, int64_t ld, const void* far_dev, int64_t far_ld, int n,
                     const int64_t* samples, int64_t* track_dev, int64_t track_ld, int64_t* report_dev, void* stream) {
  return guarded([&] { echo_delay::whole(ctx, cfg, format, mic_dev, ld, far_dev, far_ld, n, samples, track_dev, track_ld, report_dev, stream); });
}

// ---- input noise suppression (denoise.hip): conan_mel_denoise, conan_streams_set_denoise, conan_streams_denoise,
// conan_denoise_state_bytes, conan_streams_denoise_state
int conan_mel_denoise(conan_ctx* ctx, const conan_denoise_cfg* cfg, const float* mel_dev, int n, const int32_t* frames, int64_t ld, int num_mels,
                      const conan_denoise_state* seed_dev, float* out_dev, conan_denoise_state* state_out_dev, void* stream) {
  return guarded([&] { denoise::whole(ctx, cfg, mel_dev, n, frames, ld, num_mels, seed_dev, out_dev, state_out_dev, stream); });
}

int conan_streams_set_denoise(conan_streams* s, const int32_t* slots, int n, const conan_denoise_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream) {
  return guarded([&] { denoise::set_denoise(s, slots, n, cfg, seed_dev, seed_ld, stream); });
}

int conan_streams_denoise(const conan_streams* s, int slot, conan_denoise_cfg* cfg_out) { return guarded([&] { wavio::get_setting(s, &conan_streams::dn, slot, cfg_out, "conan_streams_denoise"); }); }

int64_t conan_denoise_state_bytes(void) { return (int64_t)sizeof(cnk::DnState); }

int conan_streams_denoise_state(conan_streams* s, const int32_t* slots, int n, void* rows_dev, int64_t ld, void* stream) {
  return guarded([&] { denoise::state(s, slots, n, rows_dev, ld, stream); });
}

int conan_streams_set_input_rate(conan_streams* s, const int32_t* slots, int n, const conan_resample_cfg* cfg) {
  return guarded([&] { wavio::set_input_rate(s, slots, n, cfg); });
}

int conan_streams_set_input_drift(conan_streams* s, const int32_t* slots, int n, const conan_resample_cfg* cfg, const int32_t* ppb) {
  return guarded([&] { wavio::set_drift(s, CONAN_DRIFT_SOURCE, slots, n, cfg, ppb); });
}

int conan_streams_set_output_drift(conan_streams* s, const int32_t* slots, int n, const conan_resample_cfg* cfg, const int32_t* ppb) {
  return guarded([&] { wavio::set_drift(s, CONAN_DRIFT_SINK, slots, n, cfg, ppb); });
}

int conan_streams_input_drift(conan_streams* s, const int32_t* slots, int n, int32_t* ppb_out, int64_t* in_out, int64_t* out_out) {
  return guarded([&] { wavio::get_drift(s, CONAN_DRIFT_SOURCE, slots, n, ppb_out, in_out, out_out); });
}

int conan_streams_output_drift(conan_streams* s, const int32_t* slots, int n, int32_t* ppb_out, int64_t* in_out, int64_t* out_out) {
  return guarded([&] { wavio::get_drift(s, CONAN_DRIFT_SINK, slots, n, ppb_out, in_out, out_out); });
}

int conan_streams_set_output_rate(conan_streams* s, const int32_t* slots, int n, const conan_resample_cfg* cfg) {
  return guarded([&] { wavio::set_output_rate(s, slots, n, cfg); });
}

int conan_streams_set_output_ld(conan_streams* s, int64_t ld) { return guarded([&] { wavio::set_output_ld(s, ld); }); }

int conan_streams_set_input_format(conan_streams* s, const int32_t* slots, int n, int format) { return guarded([&] { wavio::set_input_format(s, slots, n, format); }); }

int conan_streams_set_output_format(conan_streams* s, const int32_t* slots, int n, int format) { return guarded([&] { wavio::set_output_format(s, slots, n, format); }); }

int conan_convert_samples(conan_ctx* ctx, int src_format, const void* src_dev, int64_t src_ld, int dst_format, void* dst_dev, int64_t dst_ld, int n,
                          int64_t samples, void* stream) {
  return guarded([&] {
    if (!ctx || !src_dev || !dst_dev) throw Error(CONAN_ERR_INVALID, "null argument");
    wavio::check_format(src_format, "conan_convert_samples");
    wavio::check_format(dst_format, "conan_convert_samples");
    if (n < 1 || n > 65535) throw Error(CONAN_ERR_INVALID, "conan_convert_samples: n must be in 1 .. 65535");
    if (samples < 1) throw Error(CONAN_ERR_INVALID, "conan_convert_samples: samples must be >= 1");
    const int64_t lim = INT64_MAX / 8;
    if (src_ld < 0 || dst_ld < 0 || src_ld > lim || dst_ld > lim || samples > lim || samples * wavio::bytes_per_sample(src_format) > src_ld * 4 || samples * wavio::bytes_per_sample(dst_format) > dst_ld * 4)
      throw Error(CONAN_ERR_INVALID, "conan_convert_samples: a row of `samples` samples does not fit its stride (4-byte units)");
    if (((uintptr_t)src_dev | (uintptr_t)dst_dev) & 3) throw Error(CONAN_ERR_INVALID, "conan_convert_samples: src_dev and dst_dev must be 4-byte aligned");
    HIP_CHECK(hipSetDevice(ctx->device));
    cnk::ConvertSamplesArgs a;
    a.src = src_dev; a.dst = dst_dev; a.src_ld = src_ld; a.dst_ld = dst_ld; a.samples = samples; a.src_fmt = src_format; a.dst_fmt = dst_format;
    cnk::launch_convert_samples(a, n, (hipStream_t)stream);
    HIP_CHECK(hipGetLastError());
  });
}

int conan_streams_output_samples(conan_streams* s, int32_t* counts, int cap) {
  int rows = 0;
  const int rc = guarded([&] { rows = wavio::output_samples(s, counts, cap); });
  return rc < 0 ? rc : rows;
}

int conan_streams_output_pending(conan_streams* s, const int32_t* slots, int n, int32_t* counts) { return guarded([&] { wavio::output_pending(s, slots, n, counts); }); }

int conan_streams_flush_output(conan_streams* s, const int32_t* slots, int n, float* wav_out_dev, int64_t wav_ld, void* stream) {
  return guarded([&] { wavio::flush_output(s, slots, n, wav_out_dev, wav_ld, stream); });
}

int conan_step_wav_chunk(conan_streams* s, float* chunk_dev, void* stream) { return guarded([&] { wavio::step_wav_chunk(s, chunk_dev, stream); }); }

int conan_step_clock(conan_streams* s, int capacity) {
  return guarded([&] {
    if (!s || capacity < 0 || capacity > 4096) throw Error(CONAN_ERR_INVALID, "conan_step_clock: capacity in [0, 4096]");
    HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
    while ((int)s->clock_ev.size() < capacity) { hipEvent_t e; HIP_CHECK(hipEventCreate(&e)); s->clock_ev.push_back(e); }
    s->clock_on = capacity > 0; s->clock_n = 0;
  });
}

int conan_step_timeline(conan_streams* s, int capacity) {
  return guarded([&] {
    if (!s || capacity < 0 || capacity > 1024) throw Error(CONAN_ERR_INVALID, "conan_step_timeline: capacity in [0, 1024]");
    HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
    while ((int)s->tl_ev.size() < capacity * 6) { hipEvent_t e; HIP_CHECK(hipEventCreate(&e)); s->tl_ev.push_back(e); }
    s->tl_on = capacity > 0; s->tl_n = 0;
  });
}

int conan_step_timeline_read(conan_streams* s, double* ms_out, int cap_steps) {
  int cnt = 0;
  const int rc = guarded([&] {
    if (!s || (!ms_out && cap_steps > 0)) throw Error(CONAN_ERR_INVALID, "null argument");
    if (s->tl_n < 1) return;
    HIP_CHECK(hipEventSynchronize(s->tl_ev[(size_t)s->tl_n * 6 - 1]));
    HIP_CHECK(hipDeviceSynchronize());
    for (int i = 0; i < s->tl_n && cnt < cap_steps; ++i, ++cnt)
      for (int e = 0; e < 6; ++e) {
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, s->tl_ev[0], s->tl_ev[(size_t)i * 6 + e]));
        ms_out[(size_t)cnt * 6 + e] = ms;
      }
  });
  return rc < 0 ? rc : cnt;
}

int conan_step_clock_read(conan_streams* s, double* ms_out, int cap) {
  int cnt = 0;
  const int rc = guarded([&] {
    if (!s || (!ms_out && cap > 0)) throw Error(CONAN_ERR_INVALID, "null argument");
    if (s->clock_n < 2) return;
    HIP_CHECK(hipEventSynchronize(s->clock_ev[s->clock_n - 1]));
    for (int i = 0; i + 1 < s->clock_n && cnt < cap; ++i) {
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, s->clock_ev[i], s->clock_ev[i + 1]));
      ms_out[cnt++] = ms;
    }
  });
  return rc < 0 ? rc : cnt;
}

int conan_streams_test_fault(conan_streams* s, int kind) {
  return guarded([&] {
    if (!s) throw Error(CONAN_ERR_INVALID, "null streams");
    if (kind < 0 || kind > 3) throw Error(CONAN_ERR_INVALID, "conan_streams_test_fault: kind 0 (off), 1 (decoder megakernel barrier), 2 (Emformer cluster exchange) or 3 (pair kernel flags)");
    s->test_fault = kind;
  });
}

int conan_streams_output_fence(conan_streams* s, void* fence_stream) {
  return guarded([&] {
    if (!s) throw Error(CONAN_ERR_INVALID, "null streams");
    s->fence_stream = (hipStream_t)fence_stream; s->fence_event = nullptr; s->fence_set = true;
  });
}

int conan_streams_output_fence_event(conan_streams* s, void* event) {
  return guarded([&] {
    if (!s || !event) throw Error(CONAN_ERR_INVALID, "null argument");
    s->fence_event = (hipEvent_t)event; s->fence_stream = nullptr; s->fence_set = true;
  });
}

int conan_streams_join(conan_streams* s, void* stream) {
  return guarded([&] {
    if (!s) throw Error(CONAN_ERR_INVALID, "null streams");
    HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
    s->join((hipStream_t)stream);
  });
}

int conan_wav2mel(conan_ctx* ctx, const conan_mel_cfg* cfg, const float* wav_dev, int n, int samples, float* mel_out_dev,
                  int32_t* frames_out, void* stream) {
  return guarded([&] {
    if (!ctx || !cfg || !wav_dev || !mel_out_dev) throw Error(CONAN_ERR_INVALID, "null argument");
    if (!ctx->finalized) throw Error(CONAN_ERR_STATE, "conan_ctx_finalize must run before conan_wav2mel");
    HIP_CHECK(hipSetDevice(ctx->device));
    ctx->wav2mel(*cfg, wav_dev, n, samples, mel_out_dev, (hipStream_t)stream);
    if (frames_out) *frames_out = conan_mel_frames(*cfg, samples);
  });
}

int conan_profile_begin(conan_streams* s) {
  return guarded([&] {
    if (!s) throw Error(CONAN_ERR_INVALID, "null streams");
    s->prof_on = true; s->prof_used = 0; s->prof_flops = 0.0; s->prof_launches = 0; s->prof_rec.clear(); s->prof_kernels.clear();
  });
}

int conan_profile_end(conan_streams* s, double* conv_ms, double* conv_flops, int64_t* conv_launches) {
  return guarded([&] {
    if (!s) throw Error(CONAN_ERR_INVALID, "null streams");
    s->prof_on = false;
    double ms = 0.0;
    for (size_t i = 0; i < s->prof_used; ++i) {
      HIP_CHECK(hipEventSynchronize(s->prof_ev[i].second));
      float t = 0.f;
      HIP_CHECK(hipEventElapsedTime(&t, s->prof_ev[i].first, s->prof_ev[i].second));
      ms += t;
      const auto& r = s->prof_rec[i];
      bool found = false;
      for (auto& k : s->prof_kernels) if (k.name == r.name) { k.ms += t; k.flops += r.flops; k.n += 1; found = true; break; }
      if (!found) s->prof_kernels.push_back({r.name, (double)t, r.flops, 1});
    }
    if (conv_ms) *conv_ms = ms;
    if (conv_flops) *conv_flops = s->prof_flops;
    if (conv_launches) *conv_launches = s->prof_launches;
  });
}

int conan_profile_kernel(conan_streams* s, int index, char* name, int name_cap, double* ms, double* flops, int64_t* launches) {
  int found = 0;
  int rc = guarded([&] {
    if (!s) throw Error(CONAN_ERR_INVALID, "null streams");
    if (index < 0 || index >= (int)s->prof_kernels.size()) return;
    const auto& k = s->prof_kernels[index];
    if (name && name_cap > 0) snprintf(name, name_cap, "%s", k.name.c_str());
    if (ms) *ms = k.ms;
    if (flops) *flops = k.flops;
    if (launches) *launches = k.n;
    found = 1;
  });
  return rc != CONAN_OK ? rc : found;
}

int conan_profile_mark(conan_streams* s, void* stream) {
  return guarded([&] {
    if (!s) throw Error(CONAN_ERR_INVALID, "null streams");
    HIP_CHECK(hipSetDevice(s->ctx->device)); s->check_fault();
    cnk::launch_profile_mark((hipStream_t)stream);
  });
}

// ---- output watermark (watermark.hip): conan_watermark_embed, conan_watermark_detect, conan_watermark_decide,
// conan_streams_set_watermark, conan_streams_watermark, conan_watermark_state_bytes, conan_streams_watermark_state
int conan_watermark_embed(conan_ctx* ctx, const conan_watermark_cfg* cfg, const float* x_dev, int n, const int64_t* samples, int64_t ld,
                          const conan_watermark_state* seed_dev, float* out_dev, conan_watermark_state* state_out_dev, void* stream) {
  return guarded([&] { wmark::embed(ctx, cfg, x_dev, n, samples, ld, seed_dev, out_dev, state_out_dev, stream); });
}

int conan_watermark_detect(conan_ctx* ctx, uint64_t key, int format, const void* x_dev, int64_t ld, int n, const int64_t* samples,
                           int64_t* score_dev, int64_t* soft_dev, int64_t soft_ld, conan_watermark_hit* hit_dev, void* stream) {
  return guarded([&] { wmark::detect(ctx, key, format, x_dev, ld, n, samples, score_dev, soft_dev, soft_ld, hit_dev, stream); });
}

int conan_watermark_decide(const int64_t* score, const int64_t* soft, const conan_watermark_hit* hit, double threshold, conan_watermark_result* out) {
  try {      // (host only, and no launch to answer for: it also runs where no device is)
    wmark::decide(score, soft, hit, threshold, out);
    return CONAN_OK;
  } catch (const ch::Error& e) {
    g_err = e.what();
    return e.code;
  }
}

int conan_streams_set_watermark(conan_streams* s, const int32_t* slots, int n, const conan_watermark_cfg* cfg, const void* seed_dev, int64_t seed_ld,
                                void* stream) {
  return guarded([&] { wmark::set_watermark(s, slots, n, cfg, seed_dev, seed_ld, stream); });
}

int conan_streams_watermark(const conan_streams* s, int slot, conan_watermark_cfg* cfg_out) { return guarded([&] { wavio::get_setting(s, &conan_streams::wm, slot, cfg_out, nullptr); }); }

int64_t conan_watermark_state_bytes(void) { return (int64_t)sizeof(cnk::WmState); }

int conan_streams_watermark_state(conan_streams* s, const int32_t* slots, int n, void* rows_dev, int64_t ld, void* stream) {
  return guarded([&] { wmark::state(s, slots, n, rows_dev, ld, stream); });
}

// ---- signalling tones (tone.hip): conan_tone_table, conan_tones, conan_tone_fill, conan_streams_set_tones, conan_streams_tones,
// conan_streams_tone_state, conan_step_wav_tones
int conan_tone_table(int sample_rate, int16_t* table_out) {
  try {      // (host only, and no launch to answer for: it also runs where no device is)
    tone::table_out(sample_rate, table_out);
    return CONAN_OK;
  } catch (const ch::Error& e) {
    g_err = e.what();
    return e.code;
  }
}

int conan_tones(conan_ctx* ctx, int hop, const conan_tone_cfg* cfg, const float* wav_dev, int64_t ld, int n, const int64_t* samples,
                const conan_tone_state* seed_dev, int32_t* digit_dev, int32_t* sound_dev, int32_t* level_dev, int64_t out_ld,
                conan_tone_state* state_out_dev, int64_t* frames_out, void* stream) {
  return guarded([&] { tone::whole(ctx, hop, cfg, wav_dev, ld, n, samples, seed_dev, digit_dev, sound_dev, level_dev, out_ld, state_out_dev, frames_out, stream); });
}

int conan_tone_fill(conan_ctx* ctx, int hop, const conan_tone_cfg* cfg, const float* wav_dev, int64_t ld, int n, int64_t samples, const int64_t* pos0,
                    const int32_t* sound_dev, const int32_t* level_dev, int64_t lvl_ld, int32_t start_level, int32_t start_sound, float* out_dev,
                    int64_t out_ld, void* stream) {
  return guarded([&] { tone::fill(ctx, hop, cfg, wav_dev, ld, n, samples, pos0, sound_dev, level_dev, lvl_ld, start_level, start_sound, out_dev, out_ld, stream); });
}

int conan_streams_set_tones(conan_streams* s, const int32_t* slots, int n, const conan_tone_cfg* cfg, void* stream) {
  return guarded([&] { tone::set_tones(s, slots, n, cfg, stream); });
}

int conan_streams_tones(const conan_streams* s, int slot, conan_tone_cfg* cfg_out) { return guarded([&] { wavio::get_setting(s, &conan_streams::tn, slot, cfg_out, "conan_streams_tones"); }); }

int conan_streams_tone_state(conan_streams* s, const int32_t* slots, int n, conan_tone_state* state_dev, void* stream) {
  return guarded([&] { tone::state(s, slots, n, state_dev, stream); });
}

int conan_step_wav_tones(conan_streams* s, int32_t* digit_dev, int32_t* sound_dev, int32_t* level_dev, void* stream) {
  return guarded([&] { tone::last_call(s, digit_dev, sound_dev, level_dev, stream); });
}

// ---- equaliser (eq.hip): conan_eq_design, conan_eq, conan_eq_state_bytes, conan_streams_set_input_eq / _set_output_eq and their getters and
// state queries
int conan_eq_design(int kind, double rate, double f0, double q, double gain_db, double out[5]) {
  try {      // (host only, and no launch to answer for: it also runs where no device is)
    eq::design(kind, rate, f0, q, gain_db, out);
    return CONAN_OK;
  } catch (const ch::Error& e) {
    g_err = e.what();
    return e.code;
  }
}

int conan_eq(conan_ctx* ctx, const conan_eq_cfg* cfg, const float* x_dev, int64_t x_ld, int n, const int64_t* samples, float* y_dev, int64_t y_ld,
             conan_eq_state* state_out_dev, const conan_eq_state* seed_dev, void* stream) {
  return guarded([&] { eq::whole(ctx, cfg, x_dev, x_ld, n, samples, y_dev, y_ld, state_out_dev, seed_dev, stream); });
}

int64_t conan_eq_state_bytes(void) { return (int64_t)sizeof(conan_eq_state); }

int conan_streams_set_input_eq(conan_streams* s, const int32_t* slots, int n, const conan_eq_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream) {
  return guarded([&] { eq::set_eq(s, false, slots, n, cfg, seed_dev, seed_ld, stream); });
}

int conan_streams_input_eq(const conan_streams* s, int slot, conan_eq_cfg* cfg_out) { return guarded([&] { eq::get_eq(s, false, slot, cfg_out); }); }

int conan_streams_input_eq_state(conan_streams* s, const int32_t* slots, int n, void* rows_dev, int64_t ld, void* stream) {
  return guarded([&] { eq::state(s, false, slots, n, rows_dev, ld, stream); });
}

int conan_streams_set_output_eq(conan_streams* s, const int32_t* slots, int n, const conan_eq_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream) {
  return guarded([&] { eq::set_eq(s, true, slots, n, cfg, seed_dev, seed_ld, stream); });
}

int conan_streams_output_eq(const conan_streams* s, int slot, conan_eq_cfg* cfg_out) { return guarded([&] { eq::get_eq(s, true, slot, cfg_out); }); }

int conan_streams_output_eq_state(conan_streams* s, const int32_t* slots, int n, void* rows_dev, int64_t ld, void* stream) {
  return guarded([&] { eq::state(s, true, slots, n, rows_dev, ld, stream); });
}

int conan_hop_size(const conan_ctx* ctx) { return ctx ? ctx->hop : 0; }
int64_t conan_ctx_weight_bytes(const conan_ctx* ctx) { return ctx ? ctx->weight_bytes : 0; }
int64_t conan_streams_state_bytes(const conan_streams* s) { return s ? s->state_bytes : 0; }

// ---- slot snapshots (snapshot.hip)
uint64_t conan_streams_layout_id(const conan_streams* s) {
  uint64_t id = 0;
  guarded([&] { if (!s) throw Error(CONAN_ERR_INVALID, "null streams"); id = snapshot::layout_id(const_cast<conan_streams*>(s)); });
  return id;
}
int64_t conan_streams_snapshot_bytes(const conan_streams* s) {
  int64_t b = 0;
  const int rc = guarded([&] { if (!s) throw Error(CONAN_ERR_INVALID, "null streams"); b = snapshot::row_bytes(const_cast<conan_streams*>(s)); });
  return rc < 0 ? rc : b;
}
int conan_streams_export_slots(conan_streams* s, const int32_t* slots, int n, void* blob_dev, int64_t blob_ld_bytes, conan_slot_meta* meta_host, void* stream) {
  return guarded([&] { snapshot::export_slots(s, slots, n, blob_dev, blob_ld_bytes, meta_host, stream); });
}
int conan_streams_import_slots(conan_streams* s, const int32_t* slots, int n, const void* blob_dev, int64_t blob_ld_bytes, const conan_slot_meta* meta_host,
                               void* stream) {
  return guarded([&] { snapshot::import_slots(s, slots, n, blob_dev, blob_ld_bytes, meta_host, stream); });
}
int conan_slot_meta_info(const conan_slot_meta* meta, conan_slot_info* out) { return guarded([&] { snapshot::meta_info(meta, out); }); }

int conan_slot_meta_level(const conan_slot_meta* meta, conan_level_cfg* out) {
  int has = 0;
  const int rc = guarded([&] { has = snapshot::meta_level(meta, out); });
  return rc < 0 ? rc : has;
}

int conan_slot_meta_pitch(const conan_slot_meta* meta, conan_pitch_cfg* out) {
  int has = 0;
  const int rc = guarded([&] { has = snapshot::meta_pitch(meta, out); });
  return rc < 0 ? rc : has;
}

// ---- voice bank (voices.hip)
int conan_voices_create(conan_ctx* ctx, int capacity, int max_ref_frames, conan_voices** out) { return guarded([&] { voices::create(ctx, capacity, max_ref_frames, out); }); }
int conan_voices_destroy(conan_voices* v) { return guarded([&] { voices::destroy(v); }); }
int conan_voices_enroll(conan_voices* v, conan_streams* via, const int32_t* ids, int n, const float* ref_mel_dev, const int32_t* ref_len, int max_len, void* stream) {
  return guarded([&] { voices::enroll(v, via, ids, n, ref_mel_dev, ref_len, max_len, stream); });
}
int conan_voices_remove(conan_voices* v, const int32_t* ids, int n) { return guarded([&] { voices::remove(v, ids, n); }); }
int conan_voices_info(const conan_voices* v, int id, conan_voice_info* out) { return guarded([&] { voices::info(v, id, out); }); }
int conan_streams_set_voice(conan_streams* s, const int32_t* slots, int n, const conan_voices* v, const int32_t* voice_ids, void* stream) {
  return guarded([&] { voices::set_voice(s, slots, n, v, voice_ids, nullptr, 1, false, stream); });
}
int conan_streams_set_voice_mix(conan_streams* s, const int32_t* slots, int n, const conan_voices* v, const int32_t* voice_ids, const float* weights, int k, void* stream) {
  return guarded([&] { voices::set_voice(s, slots, n, v, voice_ids, weights, k, true, stream); });
}
int conan_streams_voice(const conan_streams* s, int slot, int32_t* voice_id) { return guarded([&] { voices::get_voice(s, slot, voice_id); }); }
int64_t conan_voices_blob_bytes(const conan_voices* v) {
  int64_t b = 0;
  const int rc = guarded([&] { b = voices::blob_bytes(v); });
  return rc < 0 ? rc : b;
}
int conan_voices_export(conan_voices* v, const int32_t* ids, int n, void* blob_dev, int64_t blob_ld_bytes, conan_voice_meta* meta_host, void* stream) {
  return guarded([&] { voices::export_voices(v, ids, n, blob_dev, blob_ld_bytes, meta_host, stream); });
}
int conan_voices_import(conan_voices* v, const int32_t* ids, int n, const void* blob_dev, int64_t blob_ld_bytes, const conan_voice_meta* meta_host, void* stream) {
  return guarded([&] { voices::import_voices(v, ids, n, blob_dev, blob_ld_bytes, meta_host, stream); });
}
int conan_voice_meta_info(const conan_voice_meta* meta, conan_voice_info* out) { return guarded([&] { voices::meta_info(meta, out); }); }

}  // extern "C"
