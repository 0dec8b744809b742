/*
 * conan_hip.h -- C-ABI of libconan_hip.so, the MI355X (gfx950) implementation of the
 * chunkwise streaming voice-conversion hot path of User-tian/Conan.
 *
 * The reference has no FFI (it is pure Python/PyTorch); its seams are Python-level.  Each entry
 * point below names the reference interface it replaces.  All tensor pointers marked _dev are
 * DEVICE pointers owned by the caller (e.g. PyTorch-ROCm `tensor.data_ptr()`), fp32 contiguous
 * row-major as documented; the library owns only its handles.  Work is enqueued asynchronously on
 * the hipStream_t passed in (`stream`, as void*; NULL = the default stream).  Functions return 0
 * on success or a negative conan_status and never throw; conan_last_error() is thread-local.
 * One conan_streams handle may be driven by one host thread at a time; distinct handles are
 * independent.
 */
#ifndef CONAN_HIP_H
#define CONAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CONAN_HIP_ABI_VERSION 9

typedef enum conan_status {
  CONAN_OK = 0,
  CONAN_ERR_INVALID = -1,     /* bad argument (the reference raises ValueError / assert)          */
  CONAN_ERR_MISSING = -2,     /* a required state_dict tensor was not loaded (strict load failure) */
  CONAN_ERR_SHAPE = -3,       /* tensor shape does not match the configured architecture          */
  CONAN_ERR_HIP = -4,         /* HIP runtime error                                                */
  CONAN_ERR_STATE = -5,       /* call order violation (e.g. step before finalize/set_reference)    */
  CONAN_ERR_UNSUPPORTED = -6  /* configuration outside the implemented hot path                   */
} conan_status;

#define CONAN_MAX_UPS 8
#define CONAN_MAX_RESBLOCKS 4
#define CONAN_MAX_DILATIONS 4
#define CONAN_MAX_DEC_BLOCKS 16

/* Architecture hyper-parameters: the subset of the reference's `hparams` the hot path reads
 * (utils/commons/hparams.py:25-131; egs/conan_emformer.yaml, egs/hifi_16k320_shuffle.yaml). */
typedef struct conan_cfg {
  int32_t abi_version;            /* must be CONAN_HIP_ABI_VERSION */
  /* Conan (modules/Conan/Conan.py:46-113, modules/tts/fs.py:49-79) */
  int32_t hidden_size;            /* hparams['hidden_size'] (256) */
  int32_t num_mels;               /* audio_num_mel_bins (80) */
  int32_t content_vocab;          /* nn.Embedding(102, H) */
  int32_t content_kernel;         /* hparams['kernel_size'] (3) */
  int32_t dec_kernel;             /* dec_kernel_size (5) */
  int32_t dec_num_blocks;         /* len(dec_dilations) (4) */
  int32_t dec_dilations[CONAN_MAX_DEC_BLOCKS];
  int32_t dec_layers_in_block;    /* layers_in_block (2) */
  int32_t dec_post_kernel;        /* dec_post_net_kernel (3) */
  int32_t predictor_kernel;       /* predictor_kernel (5) */
  int32_t nvq;                    /* nVQ (512) */
  int32_t silent_token;           /* silent_token (57) */
  /* Emformer (modules/Emformer/emformer.py:14-25) */
  int32_t emf_input_dim;          /* 80 */
  int32_t emf_heads;              /* 8 */
  int32_t emf_ffn_dim;            /* 2048 */
  int32_t emf_layers;             /* emformer_layers (6) */
  int32_t emf_segment;            /* chunk_size // 20 (4) */
  int32_t emf_left_context;       /* 50 */
  int32_t emf_right_context;      /* right_context (2) */
  int32_t emf_output_dim;         /* proj out (100) */
  /* HiFi-GAN (modules/vocoder/hifigan/hifigan_causal.py:273-312) */
  int32_t voc_initial_channel;    /* upsample_initial_channel (512) */
  int32_t voc_num_ups;
  int32_t voc_up_rates[CONAN_MAX_UPS];
  int32_t voc_up_kernels[CONAN_MAX_UPS];
  int32_t voc_num_resblocks;      /* len(resblock_kernel_sizes) (3) */
  int32_t voc_rb_kernels[CONAN_MAX_RESBLOCKS];
  int32_t voc_rb_num_dil;
  int32_t voc_rb_dilations[CONAN_MAX_RESBLOCKS][CONAN_MAX_DILATIONS];
  /* which sub-models this context holds (bit 0 Emformer, bit 1 Conan, bit 2 HiFi-GAN) */
  int32_t models;
  /* vocoder config.yaml choices (hifigan_causal.py:287-303); 0 = the shipped egs/hifi_16k320_shuffle.yaml values */
  int32_t voc_upsample;           /* 0: 'shuffle' (CausalUpsampleBlock3), 1: 'zero' (CausalUpsampleBlock2), 2: 'nn' (CausalUpsampleBlock1,
                                     hifigan_causal.py:60-145: looks ahead, so every vocoder step must follow a reset of its slots
                                     and carry the whole utterance or window; CONAN_ERR_STATE otherwise) */
  int32_t voc_resblock;           /* 0 or 1: ResBlock1, 2: ResBlock2 */
  /* torchaudio.models.Emformer(max_memory_size=, tanh_on_mem=): the memory bank.  modules/Emformer/emformer.py:14-22
   * never passes them (0 / false), so shipped checkpoints run without a bank; > 0 enables the summary vector,
   * the per-layer memory ring and the memory tokens in the attention (BASELINE.json north_star "memory-bank update") */
  int32_t emf_max_memory_size;
  int32_t emf_tanh_on_mem;
} conan_cfg;

#define CONAN_MODEL_EMFORMER 1
#define CONAN_MODEL_CONAN 2
#define CONAN_MODEL_HIFIGAN 4
#define CONAN_MODEL_FRONTEND 8   /* conan_streams_reset only (ABI 9): the streaming front-end of conan_step_wav */

typedef struct conan_ctx conan_ctx;          /* per device: packed weights, workspaces */
typedef struct conan_streams conan_streams;  /* per-slot streaming state               */

const char* conan_last_error(void);
int conan_abi_version(void);

/* Replaces model construction: Conan(0, hp) inference/Conan.py:34-38, EmformerDistillModel(hp,
 * output_dim=100) :47-52, HifiGanGenerator(config) tasks/tts/vocoder_infer/hifigan.py:17. */
int conan_ctx_create(int device, const conan_cfg* cfg, conan_ctx** out);
int conan_ctx_destroy(conan_ctx* ctx);

/* Replaces load_ckpt / nn.Module.load_state_dict (utils/commons/ckpt_utils.py:26-66).
 * `key` is "<model>.<state_dict key>" with model in {"emformer","conan","hifigan"}; `host`
 * is a HOST pointer to fp32 data of `shape[0..ndim)`; the data is copied.  Unknown keys are
 * ignored (strict=False behaviour) and reported through the return value 1. */
int conan_ctx_load_tensor(conan_ctx* ctx, const char* key, const float* host, const int64_t* shape, int ndim);

/* Fold weight-norm (w = g*v/||v||, hifigan_causal.py:45), permute pixel-shuffle output channels,
 * repack every weight to the kernels' [tap][Cin/4][Cout][4] layout and upload.  Fails with
 * CONAN_ERR_MISSING naming the first required tensor that was not loaded. */
int conan_ctx_finalize(conan_ctx* ctx);

/* Per-slot state: Emformer K/V rings + past length, Conan conv rings + cached style/prosody,
 * HiFi-GAN conv rings.  max_frames = largest number of mel frames one step may carry;
 * max_ref_frames = longest reference mel conan_set_reference may receive. */
int conan_streams_create(conan_ctx* ctx, int max_slots, int max_frames, int max_ref_frames, conan_streams** out);
int conan_streams_destroy(conan_streams* s);

/* Arithmetic of the vocoder's matrix kernels (HifiGanGenerator's Conv1d products, hifigan_causal.py:191-244, 314-333).  Both
 * forms compute fp32 convolutions with fp32 accumulation and fp32 results; they differ in how an fp32 x fp32 product is formed:
 *   CONAN_ARITH_F32   every product on the f32-input MFMA (v_mfma_f32_*_f32);
 *   CONAN_ARITH_LIMB  every fp32 operand split exactly into three bf16 limbs (x = h + m + l), a product as the six largest of
 *                     the nine limb products on the bf16 MFMA (error of the dropped terms <= 2^-23 |x w|, below the rounding of
 *                     the fp32 accumulation; tests/test_gpu_arith.py holds both forms against float64: measured 0.8-1.1 x the
 *                     f32 kernels' rms error).  The split is exact for |x| >= 2^-109 (the third limb may be a bf16 denormal: the
 *                     bf16 MFMA honours them, measured at 2^-110); smaller operands lose low bits of the third limb, an absolute
 *                     error below 2^-130.
 *   CONAN_ARITH_AUTO  the library's default: LIMB wherever the context holds limb weights and a limb kernel exists for the launch
 *                     (ResBlock1 stages; upsamplers whose tiles fill the chip), F32 elsewhere (ResBlock2, decoder, Emformer).
 * The choice is a property of the stream-set, fixed at creation, reported by conan_streams_arith().  What is and is not invariant:
 * a step is bit-reproducible for a given stream-set, list of active slots and frame count (also pipelined against blocking steps, and
 * after a reset).  WHICH launches of an AUTO stream-set run a limb kernel depends on max_slots (the fused limb passes exist from 4
 * slots on for the C = 128 / 64 stages, always for C = 32; the C = 256 stage's grouped limb convs from 16) and, for the plain convs
 * (ups.2 / ups.3, the C = 256 stage), on whether the step's ACTIVE slots give the launch enough tiles to fill the chip - few active
 * slots in a large stream-set take the f32 kernels there, exactly like the split-K factor of the f32 conv kernel follows the active
 * count.  A stream's audio therefore differs between steps with different active sets by fp32 re-association / the form of a
 * product, within the tolerance every form is held to (tests/test_gpu_configs.py: a stream inside a batch of 64 against the same
 * stream alone, 2e-5; tests/test_gpu_round5.py: both forms against the reference goldens at the plan-switch sizes 3 .. 40).
 * CONAN_STREAMS_FIXED_PLAN (below) removes that dependence: the plan then follows max_slots only. */
typedef enum conan_arith { CONAN_ARITH_AUTO = 0, CONAN_ARITH_F32 = 1, CONAN_ARITH_LIMB = 2 } conan_arith;
/* Deployment choices of a stream-set (conan_streams_opts.flags):
 *   CONAN_STREAMS_FUSED_DECODER_BLOCKS  the decoder's conv blocks [LN -> k5 conv -> GELU] -> [1x1 conv + residual] as ONE operator each
 *                                       of the persistent decoder launch: 2 % less blocking latency at 64 streams, 1.4 % MORE time per
 *                                       pipelined step (every group member reads eight partial tensors) - for latency-bound serving;
 *   CONAN_STREAMS_SEPARATE_SMALL_STEPS  decoder steps of a single row tile (slots x frames <= 16: one to four streams) as ~38
 *                                       separate launches instead of the persistent launch in xcd mode (0.41 against
 *                                       0.28 ms per one-stream step) - an A/B switch, and a way out on parts whose workgroup -> XCD
 *                                       placement gives an XCD fewer than 8 workgroups of a 256-workgroup launch;
 *   (bit 4, CONAN_STREAMS_VOCODER_CHAIN of ABI 7, is retired: the one-launch vocoder step of small stream-sets measured slower
 *   than the launches it replaced at every size and left the library - tools/experiments/voc_chain; the bit is rejected)
 *   CONAN_STREAMS_FIXED_PLAN            (ABI 8) every launch-plan choice - kernel form (limb / f32), tile shape, split-K factor, merged
 *                                       stage tails, the decoder step's single-tile or multi-tile form - is made from max_slots
 *                                       and the step's frame count ONLY, never from the number of slots active in the step: slot k's
 *                                       audio is bit-identical whichever other slots step with it (the reference is batch-1 and
 *                                       deterministic per utterance, inference/Conan.py:109-113; a serving API can promise the
 *                                       same).  Costs throughput only when few slots of a large stream-set are active (the plan is
 *                                       the full set's); at full occupancy the plan IS the default's;
 *   CONAN_STREAMS_SHARED_DEVICE         (ABI 8) other PROCESSES drive this GPU too: never give a launch that waits inside itself
 *                                       (Emformer clusters) the whole chip.  Inside one process the library counts the live stream-sets
 *                                       per device itself (over all contexts) and takes the whole-chip shape only for blocking steps
 *                                       of the only one. */
enum { CONAN_STREAMS_FUSED_DECODER_BLOCKS = 1, CONAN_STREAMS_SEPARATE_SMALL_STEPS = 2, CONAN_STREAMS_FIXED_PLAN = 8, CONAN_STREAMS_SHARED_DEVICE = 16 };
typedef struct conan_streams_opts {
  int32_t abi_version;   /* must be CONAN_HIP_ABI_VERSION */
  int32_t arith;         /* conan_arith */
  int32_t flags;         /* bitwise or of CONAN_STREAMS_* (0: the defaults) */
  int32_t reserved0;     /* must be 0 */
  /* NULL in deployments.  Developer / test switches of the launch plan as "NAME=value;NAME=value" (A/B runs, the cross-checks of
   * tests/test_gpu_round3.py: e.g. "FENCED=1", "EMF_UNFUSED=1", "DEC_MEGA=0"); unknown names are CONAN_ERR_INVALID.  Since ABI 8 the
   * shipped library reads NO environment variable: a process's plan is a function of the arguments it passes, not of its
   * environment (until ABI 7 these were CONAN_* environment variables; `make DEV=1` builds still accept those).  The names, their
   * value rules and defaults are the table in csrc/plan_switches.h (listed in tools/README.md); the text is resolved once, at
   * creation.  Names of switches that are known to be unsafe exist in `make DEV=1` builds only and are unknown names here:
   * MEGA_LAYOUT (a GPU memory fault under "MEGA_LAYOUT=m" is on record and unexplained).  The one runtime knob that stays in the
   * environment is HIP's own GPU_MAX_HW_QUEUES (Multi-GPU). */
  const char* dev_plan;
  int32_t reserved[2];   /* must be 0 */
} conan_streams_opts;
/* conan_streams_create with options (opts == NULL: all defaults, i.e. conan_streams_create). */
int conan_streams_create_opts(conan_ctx* ctx, int max_slots, int max_frames, int max_ref_frames, const conan_streams_opts* opts,
                              conan_streams** out);
/* The arithmetic this stream-set's vocoder launches use where both forms exist: CONAN_ARITH_F32 or CONAN_ARITH_LIMB
 * (AUTO resolved); negative conan_status on a null handle. */
int conan_streams_arith(const conan_streams* s);

/* Start of utterance for the given slots (replaces `state = None` inference/Conan.py:92 and the
 * zero left-padding of every causal conv).  which = bitmask of CONAN_MODEL_*; CONAN_MODEL_FRONTEND clears the slots'
 * conan_step_wav state (no samples seen yet: the zero left-padding of centred framing). */
int conan_streams_reset(conan_streams* s, const int32_t* slots, int n, int which, void* stream);

/* Per-utterance style pass = the reference-mel-only part of Conan.forward
 * (modules/Conan/Conan.py:157-159 encode_spk_embed, :221-245 prosody tokens, K/V of the aligner).
 * ref_mel_dev[n][max_len][num_mels] (rows >= ref_len[i] ignored), ref_len host array. */
int conan_set_reference(conan_streams* s, const int32_t* slots, int n, const float* ref_mel_dev,
                        const int32_t* ref_len, int max_len, void* stream);

/* One streaming step of torchaudio Emformer.infer + proj + argmax
 * (inference/Conan.py:115-124).  chunk_dev[n][seg+rc][D]; out_dev[n][seg][D] (may be NULL);
 * logits_dev[n][seg][K] (may be NULL); codes_dev[n][seg] int32 (may be NULL). */
int conan_emformer_step(conan_streams* s, const int32_t* slots, int n, const float* chunk_dev,
                        float* out_dev, float* logits_dev, int32_t* codes_dev, void* stream);
/* The output heads of EmformerDistillModel applied to features that did NOT just come out of a step
 * (modules/Emformer/emformer.py:25 `proj`, :29-30 `proj1` / `proj2`; used by `inference()` :95-97 on the concatenated
 * per-chunk features): y_dev[rows][K_head] = x_dev[rows][D] @ W_head^T + b_head.  head = "proj", "proj1" or "proj2" as named
 * in the checkpoint.  CONAN_ERR_MISSING when the checkpoint holds no such head. */
int conan_emformer_project(conan_streams* s, const char* head, const float* x_dev, int rows, float* y_dev, void* stream);
/* Output width K_head of that head (nn.Linear(input_dim, K_head).out_features), 0 when the checkpoint has none. */
int conan_emformer_head_dim(conan_streams* s, const char* head);


/* `frames` new content codes per slot -> `frames` mel rows: Conan.forward(infer=True) restricted to
 * the new frames (modules/Conan/Conan.py:140-198 given the cached style pass).
 * codes_dev[n][frames] int32; mel_out_dev[n][frames][num_mels].  Optional taps (may be NULL):
 * uv_pred_dev[n][frames][2], f0_dev[n][frames], bins_dev[n][frames] int32, decoder_inp_dev[n][frames][H]. */
int conan_decoder_step(conan_streams* s, const int32_t* slots, int n, int frames, const int32_t* codes_dev,
                       float* mel_out_dev, float* uv_pred_dev, float* f0_dev, int32_t* bins_dev,
                       float* decoder_inp_dev, void* stream);

/* The remaining entries of the dict Conan.forward returns (modules/Conan/Conan.py:170-198; SURVEY.md §8b seam 3) as
 * optional device outputs of a decoder step; any pointer may be NULL.
 *   content_embed_proj[n][frames][H]   content_proj(content_embedding(content))              (Conan.py:140-142)
 *   attn[l][n][frames][max_tokens]     head-averaged cross-attention weights of ProsodyAligner layer l = 0, 1 over
 *                                      the slot's prosody tokens (prosody_util.py:119-161; the list in ret['attn']);
 *                                      max_tokens = ceil(max_ref_frames / 4) as given to conan_streams_create
 *                                      (conan_get_style reports it), entries past the slot's token count are 0 */
typedef struct conan_decoder_taps {
  float* uv_pred;               /* [n][frames][2] */
  float* f0_denorm_pred;        /* [n][frames] */
  int32_t* pitch_bins;          /* [n][frames] */
  float* decoder_inp;           /* [n][frames][H] */
  float* content_embed_proj;    /* [n][frames][H] */
  float* attn[2];               /* per aligner layer: [n][frames][max_tokens] */
} conan_decoder_taps;
int conan_decoder_step_taps(conan_streams* s, const int32_t* slots, int n, int frames, const int32_t* codes_dev,
                            float* mel_out_dev, const conan_decoder_taps* taps, void* stream);
/* Conan.forward(spk_embed=...) (modules/Conan/Conan.py:146-149): replace the cached global style vector of the slots
 * by a caller-provided one, style_dev[n][H].  The prosody tokens still come from the reference mel
 * (get_prosody(pitch_inp, ref, ...), Conan.py:166), so conan_set_reference must have run for the slots. */
int conan_set_style(conan_streams* s, const int32_t* slots, int n, const float* style_dev, void* stream);
/* VQ code indices of the slots' prosody tokens (VQEmbeddingEMA.encode argmin, prosody_util.py:34-46), cached by
 * conan_set_reference: ids_dev[n][max_tokens] int32 (entries past the slot's token count are -1), count_dev[n] int32
 * (may be NULL). */
int conan_get_prosody_ids(conan_streams* s, const int32_t* slots, int n, int32_t* ids_dev, int32_t* count_dev, void* stream);

/* style_embed of the slots' current reference (encode_spk_embed, Conan.py:200-219, cached by conan_set_reference):
 * style_dev[n][H].  max_tokens_out (may be NULL) receives the attn row width of conan_decoder_taps. */
int conan_get_style(conan_streams* s, const int32_t* slots, int n, float* style_dev, int32_t* max_tokens_out, void* stream);

/* `frames` new mel rows per slot -> frames*hop samples: HifiGanGenerator.forward restricted to the
 * new frames (hifigan_causal.py:314-333).  mel_dev[n][frames][num_mels]; wav_out_dev[n][frames*hop];
 * pre_tanh_dev optional. */
int conan_hifigan_step(conan_streams* s, const int32_t* slots, int n, int frames, const float* mel_dev,
                       float* wav_out_dev, float* pre_tanh_dev, void* stream);

/* conan_hifigan_step with optional taps of the generator's intermediate tensors (the forward hooks a reference
 * maintainer would register on conv_pre / ups[i], hifigan_causal.py:319-322), channel-last; any pointer may be NULL.
 *   conv_pre_act[n][frames][C0]             leaky_relu(conv_pre(mel), 0.1): the tensor ups[0] consumes
 *   ups[i][n][frames*rate_i][C_i]           output of ups[i] after the pixel shuffle (rate_i = prod(up_rates[0..i]))
 *   stage_out[i][n][frames*rate_i][C_i]     the MRF stage's output (see the field) */
typedef struct conan_hifigan_taps {
  float* conv_pre_act;
  float* ups[CONAN_MAX_UPS];
  float* stage_out[CONAN_MAX_UPS];   /* [n][frames*rate_i][C_i]: leaky_relu(mean_j resblocks[i*num_kernels + j](ups[i] output)), the tensor
                                        ups[i+1] / conv_post consumes (hifigan_causal.py:324-331) */
} conan_hifigan_taps;
int conan_hifigan_step_taps(conan_streams* s, const int32_t* slots, int n, int frames, const float* mel_dev,
                            float* wav_out_dev, float* pre_tanh_dev, const conan_hifigan_taps* taps, void* stream);

/* Fused chunk step = one iteration of the loop inference/Conan.py:95-156 for n slots:
 * mel_chunk_dev[n][seg+rc][D] -> codes_dev[n][seg] (int32), mel_out_dev[n][seg][num_mels],
 * wav_out_dev[n][seg*hop].  emit = number of leading frames that are real (<= seg). */
int conan_step(conan_streams* s, const int32_t* slots, int n, int emit, const float* mel_chunk_dev,
               int32_t* codes_dev, float* mel_out_dev, float* wav_out_dev, void* stream);

/* Pipelined conan_step: same arguments, same results bit for bit.  The Emformer + decoder of this call run on an
 * internal HIP stream and the vocoder on a second one, so the front-end of chunk t+1 overlaps the vocoder of chunk t
 * (in the reference the three stages of consecutive chunks are strictly serial, inference/Conan.py:95-156).
 * `stream` is the caller's stream: the inputs are taken as ready in its order at call time.  Outputs are complete in
 * the order of a stream that has passed conan_streams_join(); every buffer handed to a pipelined step must stay valid
 * until then.  All other stream-ordered entry points join pending pipelined work first, so the two styles can be mixed. */
int conan_step_async(conan_streams* s, const int32_t* slots, int n, int emit, const float* mel_chunk_dev,
                     int32_t* codes_dev, float* mel_out_dev, float* wav_out_dev, void* stream);
/* Make `stream` wait (device side, non-blocking for the host) for every step enqueued by conan_step_async. */
int conan_streams_join(conan_streams* s, void* stream);
/* Output fence for the NEXT conan_step_async call: its vocoder stage (the only stage that writes wav_out_dev) first waits,
 * device side, for everything enqueued on `fence_stream` up to now - e.g. the side stream on which a collective still
 * reads the buffer that the next step reuses.  Making the caller's `stream` wait for that instead would hold back the
 * step's Emformer and decoder stages too, which do not touch the buffer, and drain the pipeline (measured: 1.81 -> 2.6 ms
 * per step at 64 streams).  One-shot: cleared by the step that consumes it. */
int conan_streams_output_fence(conan_streams* s, void* fence_stream);
/* The same with an event the caller has ALREADY recorded (hipEvent_t as void*) - e.g. right behind the one collective that read the
 * buffer: the vocoder stage then waits for that collective only, not for whatever else has been enqueued on its stream since (a
 * later gather's join waits for the newest step's audio: fencing on the stream's tail would make step t's vocoder wait for the
 * side stream to have seen step t-1's completion - a cross-stream round trip per fence).  One-shot like the stream form. */
int conan_streams_output_fence_event(conan_streams* s, void* event);

/* Test hook for the bounded device-side waits.  Three kernels wait for other workgroups of their own launch (decoder step:
 * group / grid barriers; Emformer step: cluster exchange; first vocoder stage: partner flags); each such wait carries a 50 ms
 * budget, after which the waiter records a code and leaves, the launch finishes with meaningless results, and every later
 * stream-ordered entry point on the stream-set returns CONAN_ERR_HIP (the stream-set must then be destroyed; the context and
 * the process stay usable).  conan_streams_test_fault(s, kind) makes the NEXT launch of kind 1 (decoder megakernel), 2 (Emformer
 * clusters) or 3 (pair kernel) wait for an arrival that never comes, so that tests can walk that path on a healthy GPU. */
int conan_streams_test_fault(conan_streams* s, int kind);

/* Mel front-end (the step before the hot path): librosa_wav2spec as used by
 * StreamingVoiceConversion._wav_to_mel (utils/audio/__init__.py:37-84, inference/Conan.py:57-70) behind its loud_norm branch
 * (conan_loud_norm below runs that branch; a caller with loud_norm on normalises the waveform first):
 * centred zero-padded STFT (periodic Hann) -> magnitude -> Slaney mel filterbank -> log10(max(eps, .)) -> clip.
 * wav_dev[n][samples] fp32 in [-1, 1]; mel_out_dev[n][frames][num_mels] with frames = 1 + samples / hop_size
 * (*frames_out, may be NULL).  fmin / fmax < 0 mean 0 / Nyquist.  Not re-entrant per context (shared workspace).
 * framing 1 / natural_log 1 / mag_eps 1e-9 select the earlier loop's front-end (inference/Conan_previous.py:100-121:
 * reflect padding of (fft_size - hop_size) / 2 samples per side, torch.stft(center=False), sqrt(re^2 + im^2 + 1e-9),
 * ln(max(eps, .)), frames = samples / hop_size; pass vmin / vmax = -/+ 1e30 for "no clip"). */
typedef struct conan_mel_cfg {
  int32_t fft_size, hop_size, win_length, num_mels, sample_rate;
  float fmin, fmax, eps, vmin, vmax;
  int32_t framing;      /* 0: centred frames, zero padding of fft_size / 2 (librosa.stft, pad_mode='constant');
                           1: reflect padding of (fft_size - hop_size) / 2, frames start at the padded signal's first sample */
  int32_t natural_log;  /* 0: log10, 1: ln */
  float mag_eps;        /* added under the magnitude's square root (0 for librosa's |X|) */
} conan_mel_cfg;
int conan_wav2mel(conan_ctx* ctx, const conan_mel_cfg* cfg, const float* wav_dev, int n, int samples,
                  float* mel_out_dev, int32_t* frames_out, void* stream);

/* Waveform-in chunk step (ABI 9): the whole-utterance front-end of conan_wav2mel (framing 0) computed incrementally per slot, then
 * conan_step / conan_step_async on the chunk.  wav_dev[n][samples] are the slots' next samples; all slots of a call must be at the
 * same position of their utterances (started by a reset with CONAN_MODEL_FRONTEND, then fed the same calls).
 *   - a non-final call passes exactly seg * hop samples per slot (1280 at the shipped config), a final call 0 .. seg * hop;
 *   - a call runs at most ONE chunk step and reports its frame count in *emit_out (host): chunk t runs as soon as its frames
 *     [t * seg, t * seg + seg + rc) are complete - centred frame f needs samples up to f * hop + fft_size / 2 - 1 - so chunk t
 *     comes out of call t + 1 and the first call emits 0: an algorithmic latency of one chunk (80 ms);
 *   - after the final call the caller keeps calling with samples = 0, final = 1 until *emit_out == 0 (one or two more chunks).
 *     The drain frames the whole utterance as conan_wav2mel does (zero padding past the end, 1 + N / hop frames) and pads a
 *     short last chunk by repeating its last frame (StreamingVoiceConversionEngine.chunks, inference/Conan.py:95-110);
 *   - the outputs are those of conan_step fed the same chunk: codes_dev[n][seg], mel_out_dev[n][emit][num_mels] (may be NULL),
 *     wav_out_dev[n][emit * hop]; size them for emit = seg.  Each frame equals conan_wav2mel's bit for bit.
 * mel: framing 0 only (natural_log and mag_eps are honoured as by conan_wav2mel); fft_size a power of two <= 2048;
 * hop_size = conan_hop_size(); num_mels = the Emformer's input width.
 * Anything else, a wrong `samples`, or a call after the drain returned 0 is CONAN_ERR_INVALID. */
int conan_step_wav(conan_streams* s, const int32_t* slots, int n, int samples, int final, const float* wav_dev, const conan_mel_cfg* mel,
                   int32_t* codes_dev, float* mel_out_dev, float* wav_out_dev, int32_t* emit_out, void* stream);
/* Pipelined conan_step_wav: the front-end launch and the step go to the internal streams as in conan_step_async (same ordering
 * rules; wav_dev and the outputs must stay valid until conan_streams_join).  Calls that emit nothing run on `stream`. */
int conan_step_wav_async(conan_streams* s, const int32_t* slots, int n, int samples, int final, const float* wav_dev, const conan_mel_cfg* mel,
                         int32_t* codes_dev, float* mel_out_dev, float* wav_out_dev, int32_t* emit_out, void* stream);
/* Test / debug hook: copy the mel chunk the last conan_step_wav call assembled, chunk_dev[n][seg + rc][num_mels] (joins first).
 * After a conan_step_wav_ragged call it is CONAN_ERR_STATE (that call's chunk rows are grouped by emit, not in call order). */
int conan_step_wav_chunk(conan_streams* s, float* chunk_dev, void* stream);

/* Waveform-in chunk step for slots at DIFFERENT positions of their utterances (streams that started at different times).
 * Added within ABI 9 (no struct changed): a caller detects it by the exported symbol.  Slot i of the call is stepped exactly as a
 * one-slot conan_step_wav(samples[i], final[i]) would step it - same rules (a non-final slot takes seg*hop samples, a final one
 * 0 .. seg*hop; after its final call only samples = 0, final = 1 until it emits 0 frames; a drained slot is an error until a reset
 * with CONAN_MODEL_FRONTEND), same emit_out[i], same bits.  wav_dev [n][seg*hop]: slot i's samples in row i, the first samples[i]
 * used (may be null when every samples[i] is 0).  Outputs in call order with row strides of a full chunk: codes_dev [n][seg]
 * (may be null), mel_out_dev [n][seg][num_mels] (may be null), wav_out_dev [n][seg*hop]; row i holds emit_out[i] frames and
 * everything past them in the row is left untouched.  Every slot is checked before anything changes: an error leaves every slot
 * where it was.  The emitting slots are stepped in one chunk step per distinct emit value (one in the steady state, where the call
 * runs exactly the front-end launch and the mel-in step's launches); calls with several groups, or whose slots do not all emit a
 * full chunk, write the steps' outputs to library staging and copy them into place with one more launch. */
int conan_step_wav_ragged(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, const int32_t* final, const float* wav_dev,
                          const conan_mel_cfg* mel, int32_t* codes_dev, float* mel_out_dev, float* wav_out_dev, int32_t* emit_out, void* stream);
/* Pipelined conan_step_wav_ragged (ordering as conan_step_wav_async; outputs complete after conan_streams_join).  A call whose slot
 * list per emit group differs from the previous step's drains the pipeline first, as conan_step_async does. */
int conan_step_wav_ragged_async(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, const int32_t* final, const float* wav_dev,
                                const conan_mel_cfg* mel, int32_t* codes_dev, float* mel_out_dev, float* wav_out_dev, int32_t* emit_out, void* stream);

/* Input sample rates other than the model rate (added within ABI 9: a caller detects it by the exported symbols).
 * The filter is torchaudio.functional.resample's windowed sinc: with g = gcd(in_rate, out_rate), orig = in_rate / g,
 * new = out_rate / g, base = min(orig, new) * rolloff, w = ceil(lpw * orig / base), output j = p + new * q is
 * sum_k K[p][k] x[q * orig + k - w] (x zero outside the signal) with K[p][k] = sinc(pi t) window(t) base / orig,
 * t = ((k - w) / orig - p / new) * base; taps with |t| >= lpw (clamped by torchaudio, < 1e-20) are dropped.  The taps are
 * computed in double and rounded once to f32; every output is an f32 FMA chain over its phase's taps in ascending order, the
 * same in every entry point, so the streaming and whole-signal paths agree bit for bit.  Presets: hann = lpw 6, rolloff 0.99
 * (torchaudio's defaults); kaiser_best = lpw 64, rolloff 0.9475937167399596, Kaiser beta 14.769656459379492.
 * Accepted: lpw 1 .. 128, rolloff in (0, 1], rates 8000 .. 192000 Hz, reserved = 0, and at most CONAN_RESAMPLE_MAX_TAPS taps per
 * phase and 2^24 in all (a very small rolloff exceeds them). */
#define CONAN_RESAMPLE_HANN 0
#define CONAN_RESAMPLE_KAISER 1
#define CONAN_RESAMPLE_MAX_TAPS 8192
typedef struct conan_resample_cfg {
  int32_t in_rate, out_rate;          /* Hz */
  int32_t lowpass_filter_width;       /* 1..128 */
  float rolloff;                      /* (0, 1] */
  int32_t window;                     /* CONAN_RESAMPLE_HANN | CONAN_RESAMPLE_KAISER */
  float beta;                         /* Kaiser; <= 0 selects 14.769656459379492 */
  int32_t reserved[2];                /* must be 0 */
} conan_resample_cfg;
/* ceil(new * samples / orig) (host only); -1 for an invalid configuration or samples < 0. */
int64_t conan_resample_length(const conan_resample_cfg* cfg, int64_t samples);
/* Whole signals: x_dev[n][samples] -> y_dev[n][conan_resample_length(cfg, samples)] (*out_samples, may be NULL), on `stream`.
 * in_rate == out_rate is a copy. */
int conan_resample(conan_ctx* ctx, const conan_resample_cfg* cfg, const float* x_dev, int n, int64_t samples,
                   float* y_dev, int64_t* out_samples, void* stream);
/* Streaming: slots' input arrives at cfg->in_rate and is resampled on the GPU, in front of the streaming front-end, with a
 * history of its own per slot.  cfg->out_rate must be the model rate, hop * 50 (20 ms frames; 16000 at the shipped config), and
 * the wav-in steps' conan_mel_cfg.sample_rate must equal it.  80 ms of input, seg * hop * in_rate / out_rate samples, must be a
 * whole number and a multiple of orig (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400 and
 * 192000 Hz pass), and the filter's look-ahead (below) at most seg * hop samples.  Every slot must be at the start of an utterance
 * (no sample since its last CONAN_MODEL_FRONTEND reset), else CONAN_ERR_STATE; on any error no slot changes.  The rate persists
 * across CONAN_MODEL_FRONTEND resets, which clear the resampler's history; in_rate == out_rate restores the model-rate path.
 * The first call allocates a history ring of 32768 floats (128 KB) per slot of the stream-set, which conan_streams_state_bytes
 * counts from then on.
 * With a rate set, `samples` of the wav-in steps counts input-rate samples: a non-final call takes exactly
 * seg * hop * in_rate / out_rate (3840 at 48 kHz), a final call 0 .. that.  A call hands the front-end the longest prefix of
 * model-rate samples whose last tap has arrived: the first call is short by the filter's look-ahead (at most 12 samples for hann,
 * 67 for kaiser_best when downsampling, 135 for kaiser_best from 8 kHz, 270 at lpw 128), every later non-final call hands over
 * seg * hop.  The final call hands over at most seg * hop; the rest goes out on the next drain call, and the front-end sees
 * `final` on the call that delivers the last sample - so an utterance can take one more drain call than at the model rate.
 * Look-aheads up to the front-end's slack (fft_size 1024: 448 samples) keep the model-rate emit schedule; longer ones give the
 * same bits with chunks one call later.  conan_step_wav: all slots of a call share one configuration.  One launch per call
 * resamples every slot of the call that has a rate. */
int conan_streams_set_input_rate(conan_streams* s, const int32_t* slots, int n, const conan_resample_cfg* cfg);
/* conan_step_wav_ragged with an explicit row stride of wav_dev (floats), so that one call can mix slots at different rates
 * (wav_ld >= every samples[i]).  conan_step_wav_ragged is this with wav_ld = seg * hop, where a row that needs more samples
 * than that (a non-final slot above the model rate) is CONAN_ERR_INVALID. */
int conan_step_wav_ragged_ld(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, const int32_t* final, const float* wav_dev,
                             int64_t wav_ld, const conan_mel_cfg* mel, int32_t* codes_dev, float* mel_out_dev, float* wav_out_dev,
                             int32_t* emit_out, void* stream);
int conan_step_wav_ragged_ld_async(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, const int32_t* final,
                                   const float* wav_dev, int64_t wav_ld, const conan_mel_cfg* mel, int32_t* codes_dev, float* mel_out_dev,
                                   float* wav_out_dev, int32_t* emit_out, void* stream);

/* Output sample rates other than the model rate (added within ABI 9: a caller detects it by the exported symbols).  The slots'
 * audio leaves at cfg->out_rate, resampled on the GPU behind the vocoder with conan_resample's filter and a history of its own per
 * slot; streamed output plus flush equals conan_resample of the model-rate audio bit for bit.  cfg->in_rate must be the model rate
 * (hop * 50).  Filter fields and limits are conan_resample's.  Every slot must be at the start of its vocoder stream (no frame
 * since its last reset that included CONAN_MODEL_HIFIGAN), else CONAN_ERR_STATE.  On any error no slot changes.  The rate persists
 * across resets.  A reset that includes CONAN_MODEL_HIFIGAN restarts the resampler (output index 0, inputs before the first are
 * zero).  in_rate == out_rate restores the model-rate path for those slots.  The first call with a real rate allocates a history
 * ring per slot (CONAN_RESAMPLE_MAX_TAPS + max_frames * hop floats, rounded up to a power of two), which
 * conan_streams_state_bytes counts from then on.
 * The rate applies to wav_out_dev of every entry point that writes it (conan_hifigan_step[_taps], conan_step[_async],
 * conan_step_wav[_async], conan_step_wav_ragged[_ld][_async]); pre_tanh_dev, the taps, mel_out_dev and codes_dev stay at the model
 * rate.  A step that gives a slot e frames adds e * hop model-rate samples to its total I; the row receives outputs
 * [delivered, ready(I)), the longest prefix of outputs whose last tap has arrived.  So the first step is short by the filter's
 * look-ahead (hann: 6 output samples at 8 kHz, 18 at 48 kHz, 36 at 96 kHz; kaiser_best: 67 / 202 / 405; at most 8.4 ms), every
 * later step delivers e * hop * out_rate / in_rate samples (its floor or ceiling when that is no whole number), and
 * conan_streams_flush_output delivers the tail.  Slots of one call may mix rates, filters and no rate; a slot's samples never
 * depend on the other slots of the call.  One more launch per vocoder step that has a row with a rate. */
int conan_streams_set_output_rate(conan_streams* s, const int32_t* slots, int n, const conan_resample_cfg* cfg);
/* Row stride, in floats, of wav_out_dev in EVERY step entry point from now on.  0 (the default) = each entry point's stride of
 * today (frames * hop, or seg * hop for the ragged wav-in steps).  A call in which some row needs more samples than the stride in
 * force is CONAN_ERR_INVALID before anything changes (the input side's wav_ld rule). */
int conan_streams_set_output_ld(conan_streams* s, int64_t ld);
/* Host only.  Samples written to each row of wav_out_dev by the most recent step call, in call order.  Known when the call
 * returns, also for pipelined calls.  Returns the row count.  Rows without a rate: frames * hop. */
int conan_streams_output_samples(conan_streams* s, int32_t* counts, int cap);
/* Host only.  What conan_streams_flush_output would deliver for these slots now (0 for a slot without a rate). */
int conan_streams_output_pending(conan_streams* s, const int32_t* slots, int n, int32_t* counts);
/* End of utterance.  Row i receives slot i's remaining outputs, up to conan_resample_length(cfg, samples produced), with the
 * taps past the end reading zeros, as the whole-signal kernel pads.  Joins pending pipelined work first, then runs on `stream`.
 * wav_ld below a pending count is CONAN_ERR_INVALID with nothing changed.  A flushed slot refuses further steps with
 * CONAN_ERR_STATE until a reset that includes CONAN_MODEL_HIFIGAN. */
int conan_streams_flush_output(conan_streams* s, const int32_t* slots, int n, float* wav_out_dev, int64_t wav_ld, void* stream);

/* Clock-drift compensation: a resampler whose ratio is in_rate / out_rate corrected by an integer ppb (parts per billion) that may
 * change along the signal (added within ABI 9: a caller detects it by the symbol conan_resample_drift).  ppb describes the far
 * device's clock, ppb > 0 = the device runs fast: on the source side (CONAN_DRIFT_SOURCE, the device samples the input) it delivers
 * in_rate * (1 + ppb * 1e-9) samples per server second; on the sink side (CONAN_DRIFT_SINK, the device plays the output) it consumes
 * out_rate * (1 + ppb * 1e-9).  One number per device serves both directions.  |ppb| <= CONAN_DRIFT_MAX_PPB.
 * The law.  All position arithmetic is in exact integers.
 *   step, in units of 2^-32 input samples per output sample, in 128-bit integers:
 *     source:  step = floor(((in_rate * (10^9 + ppb)) << 32) / (out_rate * 10^9))
 *     sink:    step = floor(((in_rate * 10^9) << 32) / (out_rate * (10^9 + ppb)))
 *   position: output 0 sits at position 0, output j at pos_j = pos_{j-1} + step_j, step_j = the step of the ppb in force at output j
 *     (a change takes effect at the next output).  n = pos >> 32, f = pos & 0xffffffff, p = f >> 22 (1024 phases),
 *     mu = float(f & 0x3fffff) * 2^-22 (exact in f32).
 *   width, from the nominal rates: base = min(in_rate, out_rate) * rolloff, W = ceil(lpw * in_rate / base); 2W taps over the inputs
 *     i = n - W + 1 + k, k = 0 .. 2W - 1.  2W > 512 is CONAN_ERR_INVALID, and so is a tile window,
 *     ceil(255 * step / 2^32) + 2W + 2 at the side's largest step, above 16384.
 *   table T[p][k], p = 0 .. 1024: conan_resample_cfg's kernel at t = ((k - W + 1) - p / 1024) * base / in_rate, that is
 *     sinc(pi t) * window(t / lpw) * base / in_rate (hann: cos(pi t / (2 lpw))^2; kaiser: I0(beta sqrt(1 - (t / lpw)^2)) / I0(beta)),
 *     zero for |t| >= lpw; built in double on the host - sin(pi t) from t's distance to the nearest integer, so an integer t gives an
 *     exact zero - and rounded once to f32.  D[p][k] = T[p + 1][k] - T[p][k], one f32 subtraction.
 *   sum: acc = 0; for k ascending: h = fmaf(mu, D[p][k], T[p][k]); acc = fmaf(h, x[i], acc); x[i] = 0 outside the signal.
 *   existence: in a whole signal of N inputs, output j exists iff n_j < N.
 *   readiness: in a stream, output j is ready once input n_j + W has arrived; after the input's final call (or in a flush) everything
 *     that exists is ready.  The result does not depend on how a stream is cut into calls.
 * Consequences: ppb = 0 is NOT bit-equal to conan_resample (the table is interpolated and every output has 2W taps); the filter runs
 * even at in_rate == out_rate; with rolloff = 1, ppb = 0 and equal rates the taps are a unit impulse and the output equals the input
 * bit for bit (a -0.0 sample leaves as +0.0: the sum starts at +0).  The interpolated table's distance from the exact kernel is
 * measured in DESIGN.md 4.28.
 * Out of scope: estimating the drift (the host's jitter-buffer level is the servo signal), slot snapshots of a drift slot
 * (conan_streams_export_slots returns CONAN_ERR_UNSUPPORTED before anything changes), the watermark detector under drift, Kaiser
 * widths beyond 512 taps. */
#define CONAN_DRIFT_SOURCE 0
#define CONAN_DRIFT_SINK 1
#define CONAN_DRIFT_MAX_PPB 2000000
#define CONAN_DRIFT_MAX_SEGMENTS 32
/* Host only, exact: the outputs of a whole signal of `samples` inputs under the schedule (below); -1 for an invalid configuration,
 * side or schedule, or samples < 0.  samples up to 2^40 and beyond are counted in 128 bits. */
int64_t conan_resample_drift_length(const conan_resample_cfg* cfg, int side, int64_t samples, const int64_t* at, const int32_t* ppb, int n_seg);
/* Host only.  The law's f32 table T, [1025][2W] row-major, into table[cap] (table may be NULL: only the size); *W (may be NULL)
 * receives W.  Returns 1025 * 2W, or a negative conan_status (cap too small: CONAN_ERR_INVALID). */
int64_t conan_resample_drift_table(const conan_resample_cfg* cfg, int32_t* W, float* table, int64_t cap);
/* Whole signals under a piecewise-constant schedule: segment k holds ppb[k] from output at[k] on (host arrays; at[0] = 0, strictly
 * ascending, 1 <= n_seg <= CONAN_DRIFT_MAX_SEGMENTS).  x_dev[n][samples] -> row r of y_dev at r * y_ld floats,
 * conan_resample_drift_length outputs each (*out_samples, may be NULL; y_ld below it is CONAN_ERR_INVALID), on `stream`.
 * 1 <= samples < 2^31 - 512.  One launch. */
int conan_resample_drift(conan_ctx* ctx, const conan_resample_cfg* cfg, int side, const float* x_dev, int n, int64_t samples,
                         const int64_t* at, const int32_t* ppb, int n_seg, float* y_dev, int64_t y_ld, int64_t* out_samples, void* stream);
/* Streams: a drift resampler per slot in place of the rational one, on the input side (conan_step_wav*) and on the output side (every
 * entry point that writes wav_out_dev).  A drift row is a row mode of the resampler launch the call makes anyway: no new launch, and
 * a stream-set that never asks allocates nothing and launches exactly what it launched before.  Rows without drift keep their bits.
 * conan_streams_set_input_drift.  cfg non-null configures the slots with ppb[i] each: cfg->out_rate must be the model rate (hop * 50),
 * in_rate == out_rate is allowed, seg * hop * in_rate / out_rate (s_in, the nominal 80 ms) must be whole, the slots must be at an
 * utterance start (CONAN_ERR_STATE otherwise), as for conan_streams_set_input_rate, whose ring and staging it shares.  cfg == NULL
 * changes only ppb, at any time between calls, host state only; it takes effect at the slot's next output; a slot without a drift
 * resampler is CONAN_ERR_STATE.  On any error no slot changes.  conan_streams_set_input_rate at an utterance start removes the drift
 * resampler.  The setting survives CONAN_MODEL_FRONTEND resets, which put the position back to 0.
 * Call contract of an input-drift slot: a call, final or not, takes 0 .. 2 * s_in samples.  The front-end gets the ready outputs not
 * yet handed over, at most seg * hop; the rest is owed to later calls (a call with 0 samples collects them).  So a call may emit 0
 * frames when the host's servo lags (fewer than seg * hop outputs became ready), and the front-end sees `final` on the call that
 * hands over the last existing output.  Unread history that would leave the 32768-sample ring is CONAN_ERR_UNSUPPORTED before anything
 * changes.  conan_step_wav (same position) wants the same configuration, ppb and position in all of its slots.
 * conan_streams_input_drift: per slot the current ppb, the inputs received and the outputs handed over since the last reset (each
 * array may be NULL) - what a host servo and the tests need to restate the schedule.  A slot without drift is CONAN_ERR_STATE.
 * conan_streams_set_output_drift / conan_streams_output_drift: the same against conan_streams_set_output_rate: cfg->in_rate must be
 * the model rate, the slots at the start of their vocoder stream; inputs = model-rate samples produced, outputs = samples delivered.
 * Every step delivers what is ready (conan_streams_output_samples; a fast sink takes more than frames * hop samples per step, so set
 * conan_streams_set_output_ld), conan_streams_flush_output delivers the tail and conan_streams_output_pending counts it. */
int conan_streams_set_input_drift(conan_streams* s, const int32_t* slots, int n, const conan_resample_cfg* cfg, const int32_t* ppb);
int conan_streams_input_drift(conan_streams* s, const int32_t* slots, int n, int32_t* ppb_out, int64_t* in_out, int64_t* out_out);
int conan_streams_set_output_drift(conan_streams* s, const int32_t* slots, int n, const conan_resample_cfg* cfg, const int32_t* ppb);
int conan_streams_output_drift(conan_streams* s, const int32_t* slots, int n, int32_t* ppb_out, int64_t* in_out, int64_t* out_out);

/* Sample formats of the audio rows (added within ABI 9: a caller detects it by the exported symbols).  wav_dev and wav_out_dev carry
 * [-1, 1] floats by default; a slot can take and deliver 16-bit PCM or G.711 instead, converted on the GPU by the arithmetic below,
 * the same in every entry point. */
#define CONAN_SAMPLE_F32  0   /* 4 bytes, today's behaviour */
#define CONAN_SAMPLE_S16  1   /* 2 bytes, little-endian signed */
#define CONAN_SAMPLE_ULAW 2   /* 1 byte, ITU-T G.711 mu-law */
#define CONAN_SAMPLE_ALAW 3   /* 1 byte, ITU-T G.711 A-law  */
/* Decode.  Decoding is exact; every result is a float with at most 16 significant bits.
 *   S16:  x = v / 32768.0f.
 *   ULAW (byte b):  u = ~b & 0xFF;  t = (((u & 15) << 3) + 0x84) << ((u >> 4) & 7);  v = (u & 0x80) ? 0x84 - t : t - 0x84 (the range
 *         is +-32124);  x = v / 32768.
 *   ALAW (byte b):  a = b ^ 0x55, m = a & 15, e = (a >> 4) & 7;  t = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1);
 *         v = (a & 0x80) ? t : -t (the range is +-32256);  x = v / 32768.
 * Encode.  The input is a finite float x.  First s = clamp(rint(x * 32768), -32768, 32767), rounding to nearest and ties to even.
 *   S16:  store s.
 *   ULAW: p = s >> 2 (arithmetic shift); neg = p < 0; p = neg ? -p : p;  p = min(p, 8159) + 0x21;
 *         seg = number of values in {0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF} that are < p;
 *         u = seg >= 8 ? 0x7F : (seg << 4) | ((p >> (seg + 1)) & 15);  byte = u ^ (neg ? 0x7F : 0xFF).
 *   ALAW: p = s >> 3; neg = p < 0; p = neg ? -p - 1 : p;
 *         seg = number of values in {0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF} that are < p;
 *         a = seg >= 8 ? 0x7F : (seg << 4) | ((seg < 2 ? p >> 1 : p >> seg) & 15);  byte = a ^ (neg ? 0x55 : 0xD5).
 * These are the tables of Python's audioop (ulaw2lin, alaw2lin, lin2ulaw, lin2alaw at width 2) on all 256 codes and all 65536 16-bit
 * values.  encode(decode(b)) == b for every code except mu-law 0x7F (negative zero), which comes back as 0xFF.
 *
 * Input format.  It applies to wav_dev of conan_step_wav[_async] and conan_step_wav_ragged[_ld][_async].  Row i holds samples[i] samples
 * of slot i's format, packed from the start of the row.  Row strides stay in 4-byte units, so existing signatures and every f32 call
 * are unchanged: row i begins i * wav_ld * 4 bytes after wav_dev; the fixed-stride entry points use samples * 4 or seg * hop * 4.
 * wav_dev must be 4-byte aligned.  A row fits when samples[i] * bytes_per_sample <= wav_ld * 4; otherwise the call is
 * CONAN_ERR_INVALID before anything changes (a 48 kHz s16 slot, 7680 bytes, does not fit conan_step_wav_ragged's default stride of
 * 5120 bytes and needs _ld; a 48 kHz mu-law slot, 3840 bytes, fits).  `samples` keeps counting samples.  Slots of one call may mix
 * formats freely, with or without input rates.  A format is stateless: it may be set at any time between calls and takes effect from
 * the next call; it persists across resets; CONAN_SAMPLE_F32 restores today's path.  The decoded float is what the resampler's
 * history ring stores and what the front end sees.  A slot with a format and no rate is decoded by the input resampler's launch
 * (one more launch per wav-in call that has such a row with samples); setting a format allocates no stream state
 * (conan_streams_state_bytes is unchanged). */
int conan_streams_set_input_format(conan_streams* s, const int32_t* slots, int n, int format);
/* Output format.  It applies to wav_out_dev of every entry point that writes it: the list in the conan_streams_set_output_rate
 * comment, plus conan_streams_flush_output.  Packing, stride and alignment follow the input rules: strides come from
 * conan_streams_set_output_ld and the flush's wav_ld, in 4-byte units; a row fits when count * bytes_per_sample <= ld * 4.
 * conan_streams_output_samples and _output_pending keep counting samples.  Bytes of a row past its count are left untouched, at byte
 * granularity.  pre_tanh_dev, the taps, mel_out_dev and codes_dev stay fp32.  Encoding happens after the output resampler, where one
 * is set; a slot with a format and no rate is encoded by the output resampler's launch (one more launch per vocoder step that has
 * such a row). */
int conan_streams_set_output_format(conan_streams* s, const int32_t* slots, int n, int format);
/* Whole signals: n rows of `samples`, any format to any format, going through the float rule above (f32 -> f32 is a copy); row i of
 * src_dev / dst_dev begins i * src_ld * 4 / i * dst_ld * 4 bytes after the pointer (both 4-byte aligned; a row fits as above, bytes of
 * a dst row past `samples` are left untouched).  It is the bit-exact yardstick for both streaming sides, and converts reference clips
 * that arrive as PCM.  An unknown format, a slot out of range or a null handle returns the usual status with nothing changed. */
int conan_convert_samples(conan_ctx* ctx, int src_format, const void* src_dev, int64_t src_ld, int dst_format, void* dst_dev, int64_t dst_ld,
                          int n, int64_t samples, void* stream);

/* Loudness normalisation of whole signals (added within ABI 9: a caller detects it by the exported symbol): the loud_norm branch
 * of the reference's librosa_wav2spec (utils/audio/__init__.py:58-63) - pyloudnorm's BS.1770 meter, a gain to target_lufs, a
 * division by the peak where that exceeds 1.  The arithmetic, which this comment defines (tests/loudness_ref.py restates it in
 * numpy); all filter and energy arithmetic is f64, as scipy.signal.lfilter's on f32 data with f64 coefficients:
 *   K-weighting.  Two biquads at the signal's own rate fs, each normalised by its a0, passband gain 1; for both
 *     w0 = 2 pi fc / fs, alpha = sin(w0) / (2 Q).
 *     High shelf, G = 4.0 dB, Q = 1 / sqrt(2), fc = 1500, A = 10^(G / 40):
 *       b0 = A ((A+1) + (A-1) cos w0 + 2 sqrt(A) alpha)    a0 = (A+1) - (A-1) cos w0 + 2 sqrt(A) alpha
 *       b1 = -2 A ((A-1) + (A+1) cos w0)                   a1 = 2 ((A-1) - (A+1) cos w0)
 *       b2 = A ((A+1) + (A-1) cos w0 - 2 sqrt(A) alpha)    a2 = (A+1) - (A-1) cos w0 - 2 sqrt(A) alpha
 *     High pass, Q = 0.5, fc = 38:  b = [(1 + cos w0) / 2, -(1 + cos w0), (1 + cos w0) / 2],  a = [1 + alpha, -2 cos w0, 1 - alpha].
 *     Shelf first, then high pass, each in direct form II transposed from a zero state:
 *       y = b0 x + z0;  z0 = b1 x - a1 y + z1;  z1 = b2 x - a2 y.
 *   Gating blocks.  T_g = 0.4, step = 0.25, T = samples / fs, numBlocks = int(round((T - T_g) / (T_g * step)) + 1) (round half
 *     to even); block j covers [int(T_g * (j * step) * fs), int(T_g * (j * step + 1) * fs)), truncated at the signal's end, all
 *     evaluated in double in exactly this order on the host.  z_j = sum y^2 / (T_g * fs);  l_j = -0.691 + 10 log10(z_j).
 *   Gating.  Absolute gate: l_j >= -70.  Gamma_r = -0.691 + 10 log10(mean z over those blocks) - 10.  Final set: l_j > Gamma_r and
 *     l_j > -70.  L = -0.691 + 10 log10(mean z over the final set); an empty set gives L = -inf.
 *   Normalise.  gain = 10^((target_lufs - L) / 20);  y = gain * x in double; with peak_limit, if p = gain * max|x| > 1 then
 *     y = y / p; one rounding to f32 at the end.
 * Library rules: a row whose L is -inf (silence, or nothing above the absolute gate) is copied unchanged with gain 1 - the
 * reference's own output there is inf / NaN - and its stats say so (LUFS -inf, 0 blocks); a row shorter than T_g * fs samples is
 * CONAN_ERR_INVALID before any launch (pyloudnorm raises there).
 * Every sum has one order, fixed by the row's length and rate alone: a row's result is bit-identical from run to run and does not
 * depend on the other rows of the call. */
typedef struct conan_loudness_cfg {
  int32_t sample_rate;   /* 8000 .. 192000 */
  float   target_lufs;   /* the reference: -22 */
  int32_t peak_limit;    /* 1: the reference's divide-by-peak above 1; 0: none */
  int32_t reserved[3];   /* must be 0 */
} conan_loudness_cfg;
/* x_dev: n rows of f32, row i at i * x_ld floats, samples[i] (host) of them used (1 .. 2^30 each, n in 1 .. 65535; rows may have
 * different lengths).  y_dev: rows at i * y_ld; only the first samples[i] floats of a row are written; NULL measures only; y_dev may
 * equal x_dev (with y_ld == x_ld).  stats_dev[n][4] (device, may be NULL): the row's LUFS, the gain applied (after the peak
 * division), the peak gain * max|x| before limiting, and the number of blocks in the final gated set.  Stream-ordered on `stream`;
 * the call never waits for the device, except for the stream's earlier work when the workspace has to grow.  Every row is checked
 * before anything is launched.  It uses the context's workspace, like conan_wav2mel: not re-entrant per context. */
int conan_loud_norm(conan_ctx* ctx, const conan_loudness_cfg* cfg, const float* x_dev, int64_t x_ld, int n, const int64_t* samples,
                    float* y_dev, int64_t y_ld, double* stats_dev, void* stream);

/* Live input levelling (added within ABI 9: a caller detects it by the exported symbols): a causal leveller for wav-in slots, the
 * streaming counterpart of conan_loud_norm, whose reading needs the whole utterance.  It runs on the GPU between the input resampler
 * and the streaming front-end, on the model-rate samples the front-end is about to read.  This comment defines it
 * (tests/level_ref.py restates it in numpy).  Per slot: fs = conan_hop_size() * 50, U = segment * hop (the samples of one chunk:
 * 1280 at the shipped configuration), x_t = the model-rate float sample at position t, position 0 being the slot's first sample
 * after a CONAN_MODEL_FRONTEND reset - after format decoding, after the input resampler.
 *   Meter.  conan_loud_norm's K-weighting at fs from a zero state, f64 throughout.  Gating block j covers [lo_j, hi_j),
 *     lo_j = int(0.4 * (j * 0.25) * fs), hi_j = int(0.4 * (j * 0.25 + 1) * fs), both evaluated in double in exactly this order on the
 *     host; z_j = sum y^2 / (0.4 * fs); l_j = -0.691 + 10 log10(z_j).  Only complete blocks count: there is no truncated last block.
 *   Update instants u_k = k * U, k >= 0.  At u_k: J_k = the number of blocks with hi_j <= u_k; the window is blocks
 *     max(0, J_k - window_blocks) .. J_k - 1; L_k = conan_loud_norm's two-gate integrated loudness over the window (absolute gate
 *     l_j >= -70; relative gate 10 LU under the mean z of the blocks that passed; final set: l_j above both, strictly; -inf when the
 *     window or the final set is empty).  P_k = max |x_t| over t < u_k (P_0 = 0).  G_{-1} = 10^(initial_gain_db / 20).
 *     G_k = G_{k-1} if L_k = -inf, else 10^(clamp(target_lufs - L_k, -max_cut_db, +max_boost_db) / 20).  Then, in either case, with
 *     peak_limit: if G_k * P_k > 1 then G_k = 1 / P_k.
 *   Samples.  For t in [u_k, u_{k+1}): g_t = G_{k-1} + (G_k - G_{k-1}) * ((t - u_k + 1) / U) in double (a division, a
 *     multiplication and an addition, each rounded); y_t = (float)((double)x_t * g_t), one rounding; with clip, y_t is then clamped
 *     to [-1, 1].  The front-end, and its audio ring, see y.
 * What follows: G_k depends only on samples before u_k - no look-ahead, no added latency; the gain is continuous and moves over ramps
 * of U samples (80 ms); y is a function of the slot's own sample stream alone - not of how calls cut the stream, of the other slots
 * of a call, or of blocking against pipelined stepping.  The peak limit bounds a ramp's END gain, not every sample of the ramp: a
 * transient louder than anything before it passes at the old gain until the next instant (a 0.9 spike during a +20 dB boost leaves
 * at 9); clip exists for that.  On every prefix that ends at a gating block's end, with window_blocks at least the block
 * count, L_k is conan_loud_norm's reading of that prefix.
 * The order of every sum, fixed by stream positions alone: the stream is cut into 128-sample segments aligned to position 0; a
 * segment's start state is M applied to its predecessor's start state plus the predecessor's end state from zero (conan_loud_norm's
 * scan); inside a segment y^2 is summed in time order (fma) into the bins that the block edges strictly inside the segment cut it
 * into; a block's energy adds, segment by segment in ascending order, the sum of the segment's bins inside the block (ascending);
 * at an instant, lane i of 256 adds the window's blocks i, i + 256, ... oldest first, and the lanes' sums meet in a binary tree
 * (lane i + lane i + w for w = 128, 64, .. 1).
 * Limits: U must be a multiple of 128 and at most 1920, fs at least 2000 Hz, else CONAN_ERR_UNSUPPORTED. */
#define CONAN_LEVEL_MAX_BLOCKS 4096
typedef struct conan_level_cfg {
  int32_t enabled;          /* 0 restores today's path for the slots; the other fields are then ignored */
  float   target_lufs;      /* the reference's loud_norm: -22 */
  float   max_boost_db, max_cut_db;   /* >= 0, finite */
  float   initial_gain_db;  /* finite */
  int32_t window_blocks;    /* 1 .. CONAN_LEVEL_MAX_BLOCKS (100 ms each) */
  int32_t peak_limit, clip; /* 0 | 1 */
  int32_t reserved[4];      /* must be 0 */
} conan_level_cfg;
/* Sets (cfg->enabled = 1) or removes (0) the leveller of `slots`, by conan_streams_set_input_rate's rules: every slot must be at the
 * start of an utterance, else CONAN_ERR_STATE; every slot and the cfg are checked before anything changes.  The setting persists
 * across CONAN_MODEL_FRONTEND resets; a reset clears the meter and returns the gain to initial_gain_db.  It applies to
 * conan_step_wav[_async] and conan_step_wav_ragged[_ld][_async]; the slots of one ragged call may mix levelled and unlevelled rows
 * with any rates and formats, and conan_step_wav's "one configuration per call" rule extends to the level cfg.  A call that gives a
 * levelled slot front-end samples runs one more launch (level_stream_kernel, one workgroup per such row) in front of the front-end
 * launch, on the same stream, so pipelined calls stay pipelined; behind an input resampler's launch it works in place on that
 * launch's staging rows, and in a call without one it reads the caller's rows and writes the staging itself (the call's unlevelled
 * rows ride along as copies), so levelling adds exactly one launch.  A stream-set that never enabled a leveller runs exactly the
 * launches it ran before.  The first enabling call allocates, per slot of the stream-set, the leveller's
 * state - 672 bytes (filter carry, pending samples, open blocks, gains, peak) and two rings of CONAN_LEVEL_MAX_BLOCKS + 16 doubles
 * (block energies and loudnesses): 66464 bytes - which conan_streams_state_bytes counts from then on.  Slot snapshots carry a
 * slot's leveller - its cfg in the record, its state as the row's last section - so a levelled stream exported mid-utterance
 * continues bit for bit elsewhere (conan_streams_import_slots allocates the state exactly as this call would, and a record without
 * a leveller turns the destination slot's off).  conan_streams_snapshot_bytes of every stream-set with a streaming front-end
 * includes that section (66464 bytes, rounded up to 256) whether or not a leveller was ever set - like the rate rings' sections, so
 * that equal stream-sets keep equal row sizes - and is therefore larger than a library without the leveller reports for the same
 * stream-set; a caller that sizes blob rows must ask this library.  conan_slot_info.bytes of a slot without a leveller, the layout id
 * and the blobs themselves are unchanged, and blobs written before the leveller existed still import. */
int conan_streams_set_input_level(conan_streams* s, const int32_t* slots, int n, const conan_level_cfg* cfg);
/* Joins pending pipelined work, then writes per slot {L_k, G_k, P_k, J_k} (stats_dev[n][4], device) on `stream`, for the latest
 * instant k = (recv - 1) / U, recv = the model-rate samples the slot's front-end has received; before any sample
 * {-inf, G_{-1}, 0, 0}.  A slot without a leveller is CONAN_ERR_STATE. */
int conan_streams_input_level(conan_streams* s, const int32_t* slots, int n, double* stats_dev, void* stream);
/* The whole-signal form, and the bit-exact yardstick of the streaming one: the same law at the context's fs and U (a context with
 * an Emformer model) on n rows (1 .. 65535) of samples[i] (host; 1 .. 2^30, rows may differ) f32 samples at i * x_ld; y_dev rows at
 * i * y_ld, only the first samples[i] floats written; y_dev may equal x_dev (with y_ld == x_ld).  trace_dev (may be NULL): row k of
 * [n][trace_ld][2] is (L_k, G_k) for k < ceil(samples[i] / U) <= trace_ld.  cfg->enabled must be 1.  One workgroup walks a row's
 * intervals in order: a yardstick, not a throughput path.  Stream-ordered; it uses the context's workspace like conan_loud_norm. */
int conan_level(conan_ctx* ctx, const conan_level_cfg* cfg, const float* x_dev, int64_t x_ld, int n, const int64_t* samples,
                float* y_dev, int64_t y_ld, double* trace_dev, int64_t trace_ld, void* stream);

/* Measurement hook (replaces the reference's Timer('hifigan') around the vocoder forward,
 * utils/commons/meters.py:21-42, tasks/tts/vocoder_infer/hifigan.py:28): between begin and end every
 * launch of the conv_mfma kernel family is bracketed by HIP events on its launch stream.  end() waits
 * for them and returns the summed kernel time, the algorithmic FLOPs (2*M*N*K of the convolutions,
 * unpadded) and the launch count. */
int conan_profile_begin(conan_streams* s);
int conan_profile_end(conan_streams* s, double* conv_ms, double* conv_flops, int64_t* conv_launches);
/* After conan_profile_end: the same totals per kernel template instantiation (index 0,1,...; returns 1 and fills the
 * outputs, 0 past the last one).  `name` is the kernel name as rocprofv3 prints it. */
int conan_profile_kernel(conan_streams* s, int index, char* name, int name_cap, double* ms, double* flops, int64_t* launches);

/* Enqueue one dispatch of the empty kernel cnk::profile_mark_kernel on `stream`: a marker that tools/summarize_pmc.py
 * uses to keep only the timed steps of a rocprofv3 counter-collection run (bench.py --marks). */
int conan_profile_mark(conan_streams* s, void* stream);
/* Step-time distribution of pipelined steps without touching their schedule: conan_step_clock(s, capacity > 0) makes every
 * following conan_step_async record one timing event on the internal vocoder stream when the step's audio is complete
 * (up to `capacity` steps; 0 switches it off); conan_step_clock_read waits for the last recorded step and writes the
 * intervals between consecutive completions in milliseconds to ms_out[cap], returning their count. */
int conan_step_clock(conan_streams* s, int capacity);
int conan_step_clock_read(conan_streams* s, double* ms_out, int cap);
/* Stage timeline of pipelined steps (developer diagnostics): with capacity > 0 every following conan_step_async records timing
 * events at the start and at the end of its Emformer, decoder and vocoder stage on their internal streams;
 * conan_step_timeline_read writes, per recorded step, the six times in milliseconds since the first step's first event
 * {emf start, emf end, dec start, dec end, voc start, voc end} to ms_out[cap_steps][6] and returns the number of steps. */
int conan_step_timeline(conan_streams* s, int capacity);
int conan_step_timeline_read(conan_streams* s, double* ms_out, int cap_steps);

/* Introspection for tests / INTEGRATION.md. */
int conan_hop_size(const conan_ctx* ctx);             /* prod(upsample_rates) */
int64_t conan_ctx_weight_bytes(const conan_ctx* ctx); /* packed device weight bytes */
int64_t conan_streams_state_bytes(const conan_streams* s);

/* Slot snapshots (added within ABI 9: a caller detects it by the exported symbols).  A stream - everything slot i of a stream-set
 * holds about its utterance - can be exported to a blob row in device memory plus a 256-byte host record, and imported into any slot
 * of a stream-set of the same shape: on another GPU, in another process, later, or into several slots at once (a fork).
 *
 * What travels.  Device state in the blob row: the position counters, every activation ring of the vocoder and the decoder saved as
 * its HISTORY (the rows a future step can still read: row (pos * rate - H + j) & lmask for j = 0 .. H-1, oldest first, H = the left
 * context the ring was sized for; ring sizing L = next_pow2(H + max_frames * rate) is the guarantee that no step reads further back),
 * the Emformer key / value rings and memory bank whole, the style cache (style vector, cross-attention keys / values and mask, token
 * count, prosody ids), and - last, only for slots that use them - the streaming front-end's rings, the input resampler's ring and
 * the output resampler's history.  Host state in the meta record: has_ref, whether the vocoder is freshly reset, the vocoder's
 * sample count, the front-end's and both resamplers' counters and phases, and the slot's configuration that belongs to the stream:
 * both rates with their filters and both sample formats.  The output stride (conan_streams_set_output_ld) is a property of the
 * stream-set and stays behind.  A row holds no pointers, slot numbers or ring indices; it may be copied to the host, to a file or to
 * another device.
 *
 * Layout id.  A 64-bit hash over what decides a slot's state: the conan_cfg fields that size it, the resolved arithmetic, S_max
 * (from max_ref_frames) and the ordered list of state regions with their row width, rate and saved rows.  Ring lengths, and with
 * them max_frames, are not part of it; nor are devices or addresses: stream-sets created with equal arguments on contexts of equal
 * configuration have equal ids in any process.  NOTE: the SET of rings depends on max_slots - the vocoder plan changes at 4, 8 and
 * 16 slots (build_vocoder: fused stages keep no xt / activated twins, the pair stage adds its own history rings) - and on the
 * arithmetic (f32 / limb).  A snapshot therefore moves between stream-sets of the same shape (same context configuration, same
 * arith, same max_ref_frames, max_slots on the same side of those thresholds), not between arbitrary ones; anything else is
 * CONAN_ERR_INVALID naming both ids.
 *
 * conan_streams_snapshot_bytes: bytes of a blob row, an upper bound over all slots (a slot without rates or wav-in uses less:
 * conan_slot_info.bytes), a multiple of 256.
 * conan_streams_export_slots: row i of blob_dev (device memory, 16-byte aligned, rows blob_ld_bytes apart, a multiple of 16 and at
 * least the slot's used bytes) receives slots[i]'s device state, meta_host[i] its host state, complete when the call returns.  Joins
 * pending pipelined work, then runs as ONE launch on `stream`; it never waits for the device (except that the first export or import
 * of a stream-set builds its region table with one blocking copy) and changes nothing in the source.  Deterministic: padding inside
 * the used part is written as zero, bytes past conan_slot_info.bytes are not touched.
 * conan_streams_import_slots: makes slots[i] of `s` the stream of row i / meta_host[i].  Allocates the rate rings exactly as
 * conan_streams_set_input_rate / _output_rate would (conan_streams_state_bytes grows as documented there).  Every slot and every
 * record is checked before anything changes - record magic, version, size and checksum, layout id, bytes <= blob_ld_bytes, slot
 * range, duplicate slots - and on error no slot changes.  One launch on `stream` behind a join.  Rows of the destination rings
 * outside the history keep what they held: no step reads them.  With voc_upsample 'nn', whose steps rely on untouched ring rows
 * being zero, a snapshot of a fresh vocoder slot is restored by the reset's zeroing of the vocoder section first; one of a stepped
 * slot imports, and the next vocoder step refuses as it does today.
 * conan_slot_meta_info: host only, no handle: what a caller may read out of a record; CONAN_ERR_INVALID for a record that is not
 * one (zeroed, wrong version, corrupted). */
#define CONAN_SLOT_META_BYTES 256
typedef struct conan_slot_meta { unsigned char opaque[CONAN_SLOT_META_BYTES]; } conan_slot_meta;
typedef struct conan_slot_info {           /* what a caller may read out of a meta record */
  uint64_t layout_id; int64_t bytes;       /* bytes of the slot's blob row that are used */
  int32_t has_ref, in_format, out_format, reserved;
  conan_resample_cfg in_rate, out_rate;    /* in_rate == out_rate: none set */
} conan_slot_info;
uint64_t conan_streams_layout_id(const conan_streams* s);
int64_t  conan_streams_snapshot_bytes(const conan_streams* s);      /* per slot, upper bound, multiple of 256 */
int conan_streams_export_slots(conan_streams* s, const int32_t* slots, int n, void* blob_dev, int64_t blob_ld_bytes,
                               conan_slot_meta* meta_host, void* stream);
int conan_streams_import_slots(conan_streams* s, const int32_t* slots, int n, const void* blob_dev, int64_t blob_ld_bytes,
                               const conan_slot_meta* meta_host, void* stream);
int conan_slot_meta_info(const conan_slot_meta* meta, conan_slot_info* out);   /* host only, no handle */
/* Host only, no handle (added within ABI 9 with conan_streams_set_input_level): the input leveller a record carries -> 1 and *out
 * = its cfg, or 0 and *out zeroed (enabled = 0) for a record without one - every record written before the leveller existed.
 * CONAN_ERR_INVALID for a record that is not one, as conan_slot_meta_info. */
int conan_slot_meta_level(const conan_slot_meta* meta, conan_level_cfg* out);

/* Per-slot pitch control in the decoder step (added within ABI 9: a caller detects it by the exported symbols; no existing struct
 * changes).  The decoder step ends its pitch head as the reference's add_orig_pitch -> denorm_f0 -> f0_to_coarse -> pitch_embed chain
 * does (modules/Conan/Conan.py:324-351, utils/audio/pitch/utils.py:71-82, :17-28).  A slot can transpose the contour, scale its
 * excursion and move the voicing threshold, and a decoder step can take the caller's normalised contour instead of the predictor's -
 * the reference's Conan.forward(f0=, uv=, infer=False) (Conan.py:174-178).  This comment defines the law (tests/pitch_ref.py restates it
 * in numpy).  Per frame row of slot k, (d0, d1) = the uv / f0 head's output; the uv_pred tap keeps reporting it raw, as ret['uv_pred'].
 *   Source of v and uv.  With a caller contour (conan_decoder_step_pitch, f0_in_dev != NULL): v = f0_in, uv = uv_in > 0 (uv_in_dev
 *     NULL: voiced) - no silent-token forcing, the reference's non-infer branch.  Otherwise v = d1 and
 *     uv = (d0 > thr) || code == silent_token, thr = uv_threshold of an enabled slot, 0 of a disabled one.
 *   Disabled slot (enabled = 0): exactly the arithmetic and the bits of a library without this feature.
 *   Enabled slot, in f32: if range != 1 then v = fmaf(range, v - pivot, pivot); then v = v + shift_oct, with
 *     shift_oct = (float)((double)shift_semitones / 12.0) formed once on the host.
 *   Then, as ever: f0 = fminf(fmaxf(exp2f(v), 50), 900); uv -> f0 = 0; the mel-scale bin of f0_to_coarse;
 *     decoder_inp = pitch_inp + pitch_embed[bin].  The fmaxf / fminf order sends a NaN to 50 Hz: the bin is in 1 .. 255 for every
 *     float input.
 * The taps f0_denorm_pred and pitch_bins report the values after the law. */
typedef struct conan_pitch_cfg {
  int32_t enabled;          /* 0: today's path for the slots, other fields ignored */
  float   shift_semitones;  /* finite, |.| <= 48 */
  float   range;            /* finite, 0 .. 4: scales the contour's excursion around pivot (1: unchanged, 0: monotone) */
  float   pivot;            /* log2 Hz, finite; the contour value that `range` leaves in place */
  float   uv_threshold;     /* frame is unvoiced when d0 > uv_threshold (model: 0; +inf: voiced wherever the code is not the silent
                               token; -inf: all unvoiced); NaN refused */
  int32_t reserved;         /* must be 0 */
} conan_pitch_cfg;          /* 24 bytes */
/* Sets the pitch control of `slots`.  It may be called at any time, also mid-utterance; every slot and the cfg are checked before
 * anything changes.  It joins pending pipelined work, then updates a per-slot device table [max_slots] - indexed by slot, not by call
 * row - in the order of `stream`; the change takes effect from the next step of every entry point that runs a decoder step
 * (conan_decoder_step[_taps / _pitch], conan_step[_async], conan_step_wav[_async], conan_step_wav_ragged[_ld][_async]).  The setting
 * persists across resets.  The table is allocated with the stream-set (24 bytes per slot, part of conan_streams_state_bytes) and
 * initialised to disabled; a stream-set that never calls the setter runs the launches it ran before.  Slot snapshots carry the cfg in
 * the host record: conan_streams_import_slots writes the destination slots' entries (a record without one - every record written
 * before this existed - turns the destination's off); the layout id, blob rows and conan_streams_snapshot_bytes are unchanged. */
int conan_streams_set_pitch(conan_streams* s, const int32_t* slots, int n, const conan_pitch_cfg* cfg, void* stream);
/* Host only: the cfg of `slot` as set (enabled = 0 and zeros for a slot without one). */
int conan_streams_pitch(const conan_streams* s, int slot, conan_pitch_cfg* out);
/* conan_decoder_step_taps with a caller contour: f0_in_dev[n][frames] in log2 Hz (the reference's norm_f0 with pitch_norm 'log'),
 * uv_in_dev[n][frames] (> 0: unvoiced; may be NULL: all voiced) - Conan.forward(content, ref=, f0=, uv=, infer=False).  The slots'
 * pitch control applies on top of the contour.  f0_in_dev == NULL is conan_decoder_step_taps (uv_in_dev is then ignored); taps may be
 * NULL.  The fused chunk steps take no caller contour: they replace the loop of inference/Conan.py, which passes f0=None; the wav-in
 * steps can track the source's own (conan_streams_set_pitch_follow). */
int conan_decoder_step_pitch(conan_streams* s, const int32_t* slots, int n, int frames, const int32_t* codes_dev, const float* f0_in_dev,
                             const float* uv_in_dev, float* mel_out_dev, const conan_decoder_taps* taps, void* stream);
/* Host only, no handle: the pitch control a record carries -> 1 and *out = its cfg, or 0 and *out zeroed for a record without one.
 * CONAN_ERR_INVALID for a record that is not one, as conan_slot_meta_info. */
int conan_slot_meta_pitch(const conan_slot_meta* meta, conan_pitch_cfg* out);

/* Source-pitch following (added within ABI 9: a caller detects it by the exported symbols; no existing struct changes).  A wav-in
 * slot can drive its decoder steps with the f0 / uv contour of its own input - the reference's Conan.forward(f0=, uv=, infer=False)
 * seam fed what the model was trained on, an extractor's contour in which an unvoiced frame has f0 = 0 (utils/audio/pitch_extractors.py,
 * data_gen) - so the converted voice keeps the source speaker's melody.  The reference's extractors are external programs; the tracker
 * is defined here (tests/f0_ref.py restates it in float64 numpy).  It is YIN (de Cheveigne and Kawahara 2002) on the mel front-end's own
 * frames, so frame f of the tracker and frame f of the mel cover the same samples.
 *   Frame.  N = mel.fft_size, hop = mel.hop_size, sr = 50 * hop.  Frame f is x[k] = s[f * hop - N / 2 + k], k = 0 .. N-1, in f64, s = the
 *     model-rate samples (behind the input resampler and the leveller); zeros before the utterance, and past its end once it is final.
 *     No window.  1 + samples / hop frames, as conan_wav2mel framing 0.
 *   Lags and window.  tmin = floor(sr / fmax), tmax = ceil(sr / fmin), W = N - tmax - 1.  tmin < 2, tmax > N / 2 or fmin >= fmax is
 *     CONAN_ERR_INVALID.
 *   Difference function.  d(t) = sum_{k < W} (x[k] - x[k + t])^2 for t = 1 .. tmax + 1, in f64, in this difference form (never as
 *     energies minus a correlation).
 *   Normalisation.  d'(t) = d(t) * t / sum_{j <= t} d(j), and d'(t) = 1 where that sum is 0.
 *   Pick.  The first t in [tmin, tmax] with d'(t) < threshold; then t moves on while t + 1 <= tmax and d'(t + 1) < d'(t).  No such t: the
 *     frame is unvoiced.
 *   Power gate.  sum_{k < W} x[k]^2 / W < 10^(floor_db / 10): the frame is unvoiced.
 *   Interpolation.  a, b, c = d'(t - 1), d'(t), d'(t + 1); off = 0.5 * (a - c) / (a - 2 b + c), clamped to +-1, and 0 where the
 *     denominator is not positive; f0 = sr / (t + off).
 *   Output.  v = (float)log2(f0) with log2 in f64 - the seam's unit - and uv = 0; an unvoiced frame gives v = 0, uv = 1.
 * The order of every sum is fixed by (N, tmax) alone: a frame's bits do not depend on the other frames or rows of a launch, which is
 * why the streaming contour equals conan_f0's of the same samples bit for bit. */
typedef struct conan_f0_cfg {
  int32_t enabled;          /* 0: no following for the slots, other fields ignored */
  float   fmin, fmax;       /* Hz, finite, 0 < fmin < fmax (50 / 900: the range of denorm_f0's clamp) */
  float   threshold;        /* in (0, 1); YIN's absolute threshold (0.15) */
  float   floor_db;         /* finite; frames whose mean power is below 10^(floor_db / 10) are unvoiced (-60) */
  int32_t reserved;         /* must be 0 */
} conan_f0_cfg;             /* 24 bytes */
/* The whole-signal form, and the bit-exact yardstick of the streaming one (the role conan_level plays for the leveller): wav_dev[n][samples]
 * f32 (n in 1 .. 65535, samples >= 1) -> f0_out_dev[n][frames] (log2 Hz, 0 where unvoiced) and uv_out_dev[n][frames] (0 | 1), frames =
 * 1 + samples / hop (*frames_out, may be NULL).  Of mel only fft_size (a power of two in 64 .. 2048), hop_size and sample_rate (which must
 * be 50 * hop_size) are read.  cfg->enabled must be 1.  One launch (cnk::f0_yin_kernel, one workgroup per frame) on `stream`. */
int conan_f0(conan_ctx* ctx, const conan_mel_cfg* mel, const conan_f0_cfg* cfg, const float* wav_dev, int n, int samples, float* f0_out_dev,
             float* uv_out_dev, int32_t* frames_out, void* stream);
/* Sets (cfg->enabled = 1) or removes (0) source-pitch following for `slots`.  It may be called at any time, also mid-utterance; every
 * slot and the cfg are checked before anything changes (the setter has no frame yet: it refuses tmax > 1024, and a wav-in step whose
 * fft_size gives a following slot tmax > fft_size / 2 is CONAN_ERR_INVALID before anything changes).  A stream-set without the streaming
 * front-end is CONAN_ERR_STATE.  It joins pending pipelined work, then writes the slots' follow flag - the sixth word of their
 * pitch-table entries - in the order of `stream`, like conan_streams_set_pitch: the change takes effect from the next emitted chunk.  The
 * setting persists across resets.
 * What a following slot does.  Every conan_step_wav[_async] / conan_step_wav_ragged[_ld][_async] call that emits a chunk for it tracks
 * the chunk's frames from the slot's audio ring - the tracker keeps no state of its own - in ONE more launch per call (f0_yin_kernel,
 * behind the front-end launch on the same stream, so pipelined calls stay pipelined; calls in which no following slot emits run the
 * launches they ran before), and the chunk's decoder step takes v and uv of the slot's rows from that contour: no silent-token
 * forcing, exactly as with a caller contour.  The slot's conan_pitch_cfg (shift, range) then applies on top; its uv_threshold has
 * nothing to act on.  Precedence: a caller contour (conan_decoder_step_pitch) wins over following; conan_decoder_step[_taps] and the
 * mel-in fused steps (conan_step, conan_step_async) take no waveform and run the predictor's path for every slot.  A slot that does
 * not follow keeps its arithmetic and its bits, also in a call mixed with following slots.  The chunk's frames must still be in the
 * audio ring when the chunk is emitted, which holds for fft_size <= 1024 at the shipped configuration; otherwise the call is
 * CONAN_ERR_UNSUPPORTED before anything changes.  conan_mel_cfg.sample_rate of such a call must be 50 * hop.
 * Memory: the first enabling call allocates the contour staging (4 sets of 2 * max_slots * segment floats) and row tables, which
 * conan_streams_state_bytes counts from then on.  A stream-set that never calls the setter runs exactly the launches it ran before.
 * Snapshots: the 256-byte host record is full, so a snapshot does NOT carry the follow setting and conan_streams_import_slots leaves the
 * destination slot's setting alone.  The tracker has no state beyond the audio ring, which snapshots carry: a following stream exported
 * mid-utterance and imported into a slot given the same setting continues bit for bit; imported into a slot with following off it
 * continues on the predictor's path. */
int conan_streams_set_pitch_follow(conan_streams* s, const int32_t* slots, int n, const conan_f0_cfg* cfg, void* stream);
/* Host only: the follow cfg of `slot` as set (enabled = 0 and zeros for a slot without one). */
int conan_streams_pitch_follow(const conan_streams* s, int slot, conan_f0_cfg* out);
/* Test / debug hook in the spirit of conan_step_wav_chunk: the contour the last wav-in call handed the decoder, in call order (joins
 * first): f0_dev[n][seg] (log2 Hz) and uv_dev[n][seg]; row i holds the frames the call emitted for slot i, zeros behind them; rows that
 * do not follow or emitted nothing read v = 0, uv = 0. */
int conan_step_wav_contour(conan_streams* s, float* f0_dev, float* uv_dev, void* stream);

/* Register matching for pitch following (added within ABI 9: a caller detects it by the exported symbols; no existing struct changes).
 * A following slot keeps the source's melody and with it the source's register: a low-pitched speaker converted to a high-pitched
 * voice comes out an octave too low.  The remedy is the log-f0 mean transform of voice conversion - subtract the source's mean log-f0,
 * add the target's - with a causal, streaming estimate of the source's mean.  The law (tests/register_ref.py restates it in numpy with
 * Python integers).  Per slot the state is two 64-bit integers (n, S): the voiced frames counted so far and the sum of their quantised
 * log2-f0.  For every frame of the slot's tracked contour, in stream order, with (v, uv) as the tracker wrote them:
 *   Counted frame.  uv == 0, v finite and |v| <= 64.  Every other frame passes through unchanged and leaves the state alone.
 *   Quantisation.  q = llrint((double)v * 4194304.0) (2^22).  An f32 in [2, 16) has a unit in the last place of at least 2^-22, so q is
 *     exact for every value the tracker can produce (3.96 .. 13.97 at the shipped rate).
 *   Accumulation.  n += 1; S += q, in int64.  With |q| <= 2^28 the sums are exact and associative for any number of frames the library
 *     accepts in one call.
 *   Estimate.  mu = (double)S / ((double)n * 4194304.0), the frame itself included.
 *   Shift.  d = (double)target - mu; d = fmin(fmax(d, -(double)max_shift), (double)max_shift).
 *   Result.  v' = (float)((double)v + d); uv stays 0.
 * Every step is one correctly rounded IEEE operation and the sums are exact integers: the result does not depend on how the frames
 * are cut into calls, how many lanes scan them or which other rows share the launch, and the GPU and the reference agree bit for
 * bit.  That is why the streamed form equals the whole-signal form.
 * The seed is what (n, S) starts from.  As a prior: seed_count = 50, seed_sum = 50 * llrint(target * 2^22) assumes the source sits in
 * the target's register with the weight of one second of voiced speech - the shift starts at 0 and converges as
 * (target - v_src) * n / (50 + n) for a steady source.  As a hand-over: a stream whose (n, S) was queried continues on another slot,
 * stream-set or process bit for bit when those two numbers are given as the seed. */
typedef struct conan_register_cfg {
  int32_t enabled;      /* 0: no matching for the slots, other fields ignored */
  int32_t reseed;       /* 1: the estimate restarts from the seed; 0: it continues (a slot that had none starts from the seed) */
  float   target;       /* log2 Hz, finite: where the slot's mean log-f0 is moved to */
  float   max_shift;    /* octaves, finite, >= 0: clamp of |d| */
  int64_t seed_count;   /* 0 .. 2^34 (the bound keeps the int64 sums from overflowing) */
  int64_t seed_sum;     /* units of 2^-22 octave; |seed_sum| <= seed_count * 2^28 */
} conan_register_cfg;   /* 32 bytes */
/* The whole-signal form, and the bit-exact yardstick of the streaming one: row i of f0_dev / uv_dev [n][ld] holds frames[i] (host,
 * 0 .. ld) frames of a contour as conan_f0 writes it; every row starts from the seed.  f0_out_dev[n][ld] receives the matched contour
 * (may equal f0_dev; NULL: the pure measurement), state_out_dev[n][2] = (n, S) after the row (may be NULL).  The measurement is how a
 * caller obtains a target voice's register: its mean is S / (n * 2^22).  cfg->enabled must be 1, n is 1 .. 65535.  One launch
 * (cnk::f0_register_kernel, one workgroup per row) on `stream`. */
int conan_f0_register(conan_ctx* ctx, const conan_register_cfg* cfg, const float* f0_dev, const float* uv_dev, int n, const int32_t* frames,
                      int64_t ld, float* f0_out_dev, int64_t* state_out_dev, void* stream);
/* Sets (cfg->enabled = 1) or removes (0) register matching for `slots`; every argument is checked before anything changes, a
 * stream-set without the streaming front-end is CONAN_ERR_STATE, and pending pipelined work is joined.  What a slot with the register
 * on AND following on does: in every wav-in call that emits a chunk for it, cnk::f0_register_kernel rewrites the chunk's rows of the
 * call's contour staging directly behind f0_yin_kernel on the same stream - ONE more launch per call in which such a row emits, none
 * otherwise - so the decoder step and conan_step_wav_contour read the matched values and pipelined calls stay pipelined.  A slot with
 * the register on but following off has no contour: nothing happens to it.  The setting persists across resets.
 * The estimate restarts from the seed at the slot's first emitted chunk after a reset that includes CONAN_MODEL_FRONTEND, after a
 * setter call with reseed = 1 and after a setter call that enables a slot that was off.  A setter call with reseed = 0 on an enabled
 * slot changes target / max_shift (and the seed of later restarts) from the next emitted chunk and keeps the estimate: the voice
 * change in the middle of a call.
 * Memory: the first enabling call allocates 16 bytes of state per slot and 4 row tables of 64 bytes per slot, which
 * conan_streams_state_bytes counts from then on.  A stream-set that never calls the setter runs exactly the launches it ran before.
 * Snapshots carry neither the setting nor the estimate (the 256-byte host record is full), as they do not carry the follow setting;
 * conan_streams_layout_id and conan_streams_snapshot_bytes do not change.  The hand-over: conan_streams_pitch_register_state, export,
 * import, conan_streams_set_pitch_follow, then conan_streams_set_pitch_register with seed = the queried pair and reseed = 1. */
int conan_streams_set_pitch_register(conan_streams* s, const int32_t* slots, int n, const conan_register_cfg* cfg, void* stream);
/* Host only: the register cfg of `slot` as set, reseed = 0 (enabled = 0 and zeros for a slot without one). */
int conan_streams_pitch_register(const conan_streams* s, int slot, conan_register_cfg* cfg_out);
/* The estimates of `slots` -> state_dev[n][2] = (n, S), in the order of `stream` behind a join of pipelined work; a slot whose
 * estimate is about to restart reports its seed.  A slot without the register is CONAN_ERR_STATE. */
int conan_streams_pitch_register_state(conan_streams* s, const int32_t* slots, int n, int64_t* state_dev, void* stream);

/* Source activity (added within ABI 9: a caller detects it by the exported symbols; no existing struct or call changes).  On a call leg
 * the source is silent about half the time; in those stretches the front-end, the tracker and the leveller see line noise and the
 * model converts it into the target voice's breath and babble.  The only copy of the model-rate audio - behind the input resampler and
 * the leveller, exactly what the front-end frames - lives in the slot's audio ring on the device, so the detector runs there: a causal
 * per-slot voice-activity detector on the front-end's own frames, per-frame flags the host can read (discontinuous transmission,
 * comfort noise) and an optional click-free gate on the vocoder's audio.  The reference's one silence facility (trim_long_sil) is
 * offline, whole-file and built on an external detector; this is its streaming counterpart, defined here (tests/activity_ref.py
 * restates it in numpy f64 with Python integers).  Every step below is an integer operation or ONE correctly rounded IEEE operation,
 * so the GPU and the reference agree bit for bit and the streamed form equals the whole-signal form bit for bit.
 *   Frame.  N = mel.fft_size (a power of two in 64 .. 2048), hop = mel.hop_size, sample_rate = 50 * hop.  Frame f is
 *     x[k] = (double)s[f * hop - N / 2 + k], k = 0 .. N-1: the tracker's frames (conan_f0_cfg).  s = the model-rate samples behind the
 *     input resampler and the leveller; zeros before the utterance, and past its end once it is final.  No window.  A signal of
 *     `samples` samples has 1 + samples / hop frames.
 *   Power.  64 partial sums: p_j over k = j, j + 64, j + 128, ... in ascending order, each step p = x * x + p rounded once (the square
 *     of an f32 is exact in f64, so a fused multiply-add and multiply-then-add give the same bits).  Then the fold p_j += p_(j+32) for
 *     j < 32, then with 16, 8, 4, 2, 1.  P = p_0 / N.  The order depends on N alone, never on the launch.
 *   Thresholds, with the state's noise floor nf as it was BEFORE this frame and the cfg's floats taken as (double) of the f32:
 *     open = fmax(open_abs, nf * open_ratio), close = fmax(close_abs, nf * close_ratio).
 *   Decision.  raw = P > (active_prev ? close : open).  raw: act = 1, hang = hold_frames.  Else hang > 0: act = 1, hang -= 1.
 *     Else act = 0.
 *   Floor.  nf' = fmax(fmin(P, nf * (act ? rise_active : rise_idle)), floor_min): the floor follows the power down at once and up by at
 *     most the rise per frame.
 *   Gate level, an integer in [closed_level, 2^20].  act: lvl' = min(lvl + up_step, 2^20); else lvl' = max(lvl - down_step, closed_level).
 *   Counters.  frames += 1, active_frames += act (int64).
 *   Gain.  Frame f gates the output samples f * hop + k, k = 0 .. hop-1 (the vocoder's samples of that frame):
 *     l = lvl_prev * (hop - 1 - k) + lvl' * (k + 1), an integer; g = (float)((double)l / (double)(hop << 20)); y = x * g in f32.  The level
 *     moves linearly inside a frame, so the gain has no step (click-free), and with both ends at 2^20 g == 1.0f: open audio keeps its bits.
 * The thresholds and ratios are LINEAR power values: a helper converts decibels to f32 once and the law reads the f32, so no libm
 * function is part of the law.  conan_amd/_lib.py's activity_cfg gives -50 / -55 dBFS absolute, 9 / 6 dB over the floor, rises of 1.02
 * (idle) / 1.005 (active) per frame, a floor minimum of -70 dB, an initial floor of -60 dB, a hold of 10 frames, attack in one frame,
 * release in five and a fully closed gate.  Those defaults are choices, not measurements. */
typedef struct conan_activity_state {
  int32_t active;          /* 0 | 1: the last frame's act */
  int32_t hang;            /* hangover frames left, 0 .. 2^20 */
  int32_t level;           /* gate level after the last frame, closed_level .. 2^20 */
  int32_t reserved;        /* must be 0 */
  double  floor;           /* noise floor nf (linear power) */
  int64_t frames;          /* frames seen */
  int64_t active_frames;   /* ... of them active */
} conan_activity_state;    /* 40 bytes */
typedef struct conan_activity_cfg {
  int32_t mode;            /* 0: off (other fields ignored), 1: detect only, 2: detect and gate the vocoder's audio */
  int32_t reseed;          /* 1: the state restarts from the seed; 0: it continues (a slot that had none starts from the seed) */
  float   open_abs, close_abs;        /* linear power, finite, 0 <= close_abs <= open_abs */
  float   open_ratio, close_ratio;    /* linear power ratios over the floor, finite, 0 <= close_ratio <= open_ratio */
  float   rise_active, rise_idle;     /* finite, >= 1: the floor's largest growth per frame */
  float   floor_min;                  /* finite, > 0 */
  int32_t hold_frames;                /* 0 .. 2^20: hangover */
  int32_t up_step, down_step;         /* 1 .. 2^20: level change per active / inactive frame */
  int32_t closed_level;               /* 0 .. 2^20 - 1: the closed gate's level (0: silence) */
  int32_t reserved;                   /* must be 0 */
  conan_activity_state seed;          /* what the state starts from: active 0 | 1, hang 0 .. 2^20, level in [closed_level, 2^20],
                                         floor finite and >= floor_min, counters >= 0, reserved 0 */
} conan_activity_cfg;      /* 96 bytes */
#define CONAN_ACTIVITY_FULL 1048576   /* 2^20: the open gate's level */
/* The whole-signal form, and the bit-exact yardstick of the streaming one: wav_dev[n][samples] f32 (n in 1 .. 65535, samples >= 1) ->
 * act_out_dev[n][frames] (0 | 1) and level_out_dev[n][frames] (the level after each frame), both int32, frames = 1 + samples / hop
 * (*frames_out, may be NULL); power_out_dev[n][frames] (double, P of each frame; may be NULL); state_out_dev[n] (the state after the
 * row; may be NULL).  Every row starts from the seed.  Of mel only fft_size, hop_size and sample_rate (which must be 50 * hop_size) are
 * read.  cfg->mode must be 1 or 2 (no difference here).  One launch (cnk::activity_kernel, one workgroup per row) on `stream`. */
int conan_activity(conan_ctx* ctx, const conan_mel_cfg* mel, const conan_activity_cfg* cfg, const float* wav_dev, int n, int samples,
                   int32_t* act_out_dev, int32_t* level_out_dev, double* power_out_dev, conan_activity_state* state_out_dev, int32_t* frames_out,
                   void* stream);
/* The gain law on whole signals: row i of wav_dev (n rows of `samples` samples, row stride ld) times the gain of level_dev[i][.] (int32,
 * row stride level_ld >= ceil(samples / hop): the level after each frame, as conan_activity writes it) with start_level (0 .. 2^20) as
 * the level before frame 0 -> out_dev (row stride ld; may equal wav_dev).  A last frame that the samples cover only partly is gated
 * over the part they cover.  One launch (cnk::activity_gate_kernel) on `stream`. */
int conan_activity_gate(conan_ctx* ctx, int hop, const float* wav_dev, int n, int64_t samples, int64_t ld, const int32_t* level_dev, int64_t level_ld,
                        int32_t start_level, float* out_dev, void* stream);
/* Sets (cfg->mode = 1 | 2) or removes (0) the detector for `slots`; every argument is checked before anything changes, a stream-set
 * without the streaming front-end is CONAN_ERR_STATE, and pending pipelined work is joined.  The change takes effect from the next
 * emitted chunk and persists across resets.
 * What a slot with the feature does.  Every conan_step_wav[_async] / conan_step_wav_ragged[_ld][_async] call that emits a chunk for
 * it runs the detector on the chunk's frames [pos, pos + emit) - every emitted frame is backed by an input frame - from the slot's
 * audio ring: ONE more launch per call (cnk::activity_kernel, behind the front-end launch on the same stream, after the tracker's
 * and the register's where present; none in calls in which no such slot emits).  The frames must still be in the audio ring, as for
 * following: otherwise the call is CONAN_ERR_UNSUPPORTED before anything changes (fft_size 2048 at the shipped configuration), and
 * conan_mel_cfg.sample_rate of such a call must be 50 * hop.  In mode 2 the chunk's vocoder step gates the rows conv_post just wrote, in
 * place, in front of the output resampler and the format encoder: ONE more launch (cnk::activity_gate_kernel) per vocoder step in
 * which a gated row takes part - each emit group of a ragged call is such a step - and none otherwise; rows that are not gated are
 * skipped, not multiplied by 1, so they keep their bits.  conan_streams_flush_output sees gated audio.  The mel-in steps
 * (conan_step[_async]) and conan_hifigan_step* take no waveform: they neither detect nor gate.
 * The state restarts from the seed at the slot's first emitted chunk after a reset that includes CONAN_MODEL_FRONTEND, after a
 * setter call with reseed = 1 and after a setter call that enables a slot that was off.  A setter call with reseed = 0 on an enabled
 * slot replaces the parameters (and the seed of later restarts) and keeps the state.
 * Memory: the first enabling call allocates 40 bytes of state per slot, 8 staging sets of (2 * segment + 1) int32 per slot for the
 * flags and levels on their way from the front-end stage to the vocoder stage, and 8 row tables; conan_streams_state_bytes counts them
 * from then on.  A stream-set that never calls the setter allocates nothing and runs exactly the launches it ran before.
 * Snapshots carry neither the setting nor the state (the 256-byte host record is full); conan_streams_layout_id and
 * conan_streams_snapshot_bytes do not change.  The hand-over: conan_streams_activity_state, export, import, then this setter with
 * seed = the queried state and reseed = 1. */
int conan_streams_set_activity(conan_streams* s, const int32_t* slots, int n, const conan_activity_cfg* cfg, void* stream);
/* Host only: the activity cfg of `slot` as set, reseed = 0 (mode = 0 and zeros for a slot without one). */
int conan_streams_activity(const conan_streams* s, int slot, conan_activity_cfg* cfg_out);
/* The states of `slots` -> state_dev[n], in the order of `stream` behind a join of pipelined work; a slot whose state is about to
 * restart reports its seed.  A slot without the feature is CONAN_ERR_STATE. */
int conan_streams_activity_state(conan_streams* s, const int32_t* slots, int n, conan_activity_state* state_dev, void* stream);
/* Hook in the spirit of conan_step_wav_contour: the flags and frame-end levels the last wav-in call produced, in call order (joins
 * first): act_dev[n][seg] and level_dev[n][seg], int32.  Rows without the feature, rows that emitted nothing and positions behind the
 * emitted frames read zero. */
int conan_step_wav_activity(conan_streams* s, int32_t* act_dev, int32_t* level_dev, void* stream);

/* Source bypass (added within ABI 9: a caller detects it by the symbol conan_streams_set_bypass; no existing struct or call changes).
 * A latency-matched dry path and a wet/dry mix per slot: a conversion on/off toggle that neither clicks nor jumps in time, a monitor
 * mix, and the caller's own room tone in place of silence while the activity gate is closed.  Output sample j of a slot's utterance is
 * made from mel frame j / hop, and source sample j - at the model rate, behind format decoding, the input resampler and the leveller;
 * zero at and beyond the samples received - is in the slot's audio ring when that frame's chunk is emitted.  The mix runs in front of
 * the output resampler and the format encoder, so it leaves at the slot's own rate and format, flush included.  The law
 * (tests/bypass_ref.py restates it in numpy with Python integers); levels are integers in 0 .. 2^20 (CONAN_ACTIVITY_FULL):
 *   Slew.  Per emitted frame f each of wet and dry moves towards its target by at most step: v += clamp(target - v, -step, step).
 *   Fill.  dry_eff_f = fill_gate ? (dry_f * (2^20 - gate_f)) >> 20 : dry_f, with gate_f the frame-end level the slot's activity
 *     detector produced for that frame in the same call, and 2^20 where the slot is not in activity mode 2 (an absent gate is open:
 *     nothing is filled).
 *   Gain.  Sample k of frame f takes l = prev * (hop - 1 - k) + next * (k + 1), for the wet levels and for the effective dry levels
 *     separately; the levels before a chunk's first frame are the state's wet and dry_eff.  g = (float)((double)l / (double)(hop << 20)):
 *     the gate's formula.
 *   Mix.  With y the vocoder's sample behind the gate and x the source sample: t = y * g_w (one f32 product);
 *     out = l_d == 0 ? t : fma(x, g_d, t) (one f32 fused multiply-add).  wet = 2^20, dry = 0 gives y bit for bit; wet = 0, dry = 2^20
 *     gives x in value (only the sign of a zero can differ).  Nothing here has a tolerance.
 *   Restart.  The state restarts from the seed - wet = seed_wet, dry = seed_dry, dry_eff = the fill formula on seed_dry and the gate's
 *     level before the chunk - at the slot's first emitted chunk after a reset that includes CONAN_MODEL_FRONTEND, after a setter call
 *     with reseed = 1 and when a slot that was off is enabled.  A setter call with reseed = 0 on an enabled slot replaces the targets,
 *     step and fill_gate and keeps the levels: that call is the toggle. */
typedef struct conan_bypass_cfg {
  int32_t enabled;         /* 0: off (other fields ignored) | 1 */
  int32_t reseed;          /* 0 | 1: the state restarts from the seed */
  int32_t wet_target;      /* 0 .. 2^20 */
  int32_t dry_target;      /* 0 .. 2^20 */
  int32_t step;            /* 1 .. 2^20: levels per 20 ms frame */
  int32_t fill_gate;       /* 0 | 1: the dry level is scaled by the closed part of the slot's activity gate */
  int32_t seed_wet;        /* 0 .. 2^20 */
  int32_t seed_dry;        /* 0 .. 2^20 */
} conan_bypass_cfg;        /* 32 bytes */
typedef struct conan_bypass_state {
  int32_t wet, dry;        /* the levels after the last emitted frame */
  int32_t dry_eff;         /* the effective dry level after that frame */
  int32_t reserved;
} conan_bypass_state;      /* 16 bytes */
/* Sets (cfg->enabled = 1) or removes (0) the bypass for `slots`.  Every argument is checked before anything changes
 * (CONAN_ERR_INVALID: flags not 0 / 1, levels outside 0 .. 2^20, step outside 1 .. 2^20), a stream-set without the streaming
 * front-end is CONAN_ERR_STATE, and pending pipelined work is joined; it may be called at any time, also mid-utterance.  The change
 * takes effect from the next emitted chunk and persists across resets.
 * What a slot with the feature does.  Every conan_step_wav[_async] / conan_step_wav_ragged[_ld][_async] call that emits a chunk for
 * it runs ONE more launch (cnk::bypass_stage_kernel, behind the front-end launch and the activity detector's), which runs the slew
 * over the chunk's frames and copies the chunk's emit * hop source samples from the slot's audio ring into the call's dry staging;
 * the chunk's samples must still be in the ring, otherwise the call is CONAN_ERR_UNSUPPORTED before anything changes.  The chunk's
 * vocoder step mixes the rows conv_post wrote, in place, behind the activity gate and in front of the output resampler and the format
 * encoder: ONE more launch (cnk::bypass_mix_kernel) per vocoder step in which such a row takes part; rows without the feature are
 * skipped and keep their bits.  The mel-in steps (conan_step[_async]) and conan_hifigan_step* take no waveform and do not mix.
 * Memory: the first enabling call allocates 16 bytes of state per slot, 8 staging sets of 2 * (segment + 1) int32 and segment * hop
 * float per slot, and 8 row tables; conan_streams_state_bytes counts them from then on.  A stream-set that never calls the setter
 * allocates nothing and runs exactly the launches it ran before.
 * Snapshots carry neither the setting nor the state (the 256-byte host record is full); conan_streams_layout_id and
 * conan_streams_snapshot_bytes do not change.  The hand-over: conan_streams_bypass_state, export, import, then this setter with
 * seed_wet / seed_dry = the queried wet / dry and reseed = 1 (beside the activity hand-over where fill_gate is in use). */
int conan_streams_set_bypass(conan_streams* s, const int32_t* slots, int n, const conan_bypass_cfg* cfg, void* stream);
/* Host only: the bypass cfg of `slot` as set, reseed = 0 (zeros for a slot without one). */
int conan_streams_bypass(const conan_streams* s, int slot, conan_bypass_cfg* cfg_out);
/* The states of `slots` -> state_dev[n], in the order of `stream` behind a join of pipelined work; a slot whose state is about to
 * restart reports its seed (dry_eff = seed_dry).  A slot without the feature is CONAN_ERR_STATE. */
int conan_streams_bypass_state(conan_streams* s, const int32_t* slots, int n, conan_bypass_state* state_dev, void* stream);
/* The frame-end wet and effective dry levels the last wav-in call produced, in call order (joins first): wet_lvl_dev[n][seg] and
 * dry_lvl_dev[n][seg], int32.  Rows without the feature, rows that emitted nothing and positions behind the emitted frames read zero.
 * CONAN_ERR_STATE before any wav-in call. */
int conan_step_wav_bypass(conan_streams* s, int32_t* wet_lvl_dev, int32_t* dry_lvl_dev, void* stream);
/* The mix on whole signals, and the bit-exact yardstick of the streaming one: row i of wet_dev (n rows in 1 .. 65535 of `samples`
 * samples, row stride wet_ld) and of dry_dev (row stride dry_ld) with the frame-end levels wet_lvl_dev[i][.] and dry_lvl_dev[i][.]
 * (int32, 0 .. 2^20, row stride lvl_ld >= ceil(samples / hop); the dry levels are the EFFECTIVE ones) and start_wet / start_dry as the
 * levels before frame 0 -> out_dev (row stride out_ld; may equal wet_dev with out_ld = wet_ld).  A last frame that the samples cover
 * only partly is mixed over the part they cover.  One launch (cnk::bypass_mix_kernel) on `stream`. */
int conan_bypass_mix(conan_ctx* ctx, int hop, const float* wet_dev, int64_t wet_ld, const float* dry_dev, int64_t dry_ld, int n, int64_t samples,
                     const int32_t* wet_lvl_dev, const int32_t* dry_lvl_dev, int64_t lvl_ld, int32_t start_wet, int32_t start_dry, float* out_dev,
                     int64_t out_ld, void* stream);

/* Comfort noise (added within ABI 9: a caller detects it by the symbol conan_streams_set_comfort; no existing struct or call changes).
 * A synthetic fill for the closed activity gate: noise at the level of the source's background, cross-faded against the gate's ramp so
 * that nothing clicks, in front of the output resampler and the format encoder - and per frame a level the host can send as RFC 3389
 * SID packets while it does not transmit.  Unlike the bypass's fill_gate it passes nothing of the caller's room.  The law
 * (tests/comfort_ref.py restates it in numpy with Python integers) is integer operations and single correctly rounded IEEE
 * operations; no libm function is part of it and nothing has a tolerance:
 *   Levels are integers L in units of 1/256 octave of power relative to full scale: L = 0 is power 1.0, -256 is power 0.5, about 85.04
 *     units are one dB.  Every level of the cfg and of the state lies in -16384 .. 0.
 *   Quantising.  With P the detector's P of the frame (conan_activity_cfg's law; a double >= 0) and bits(P) its raw 64-bit word:
 *     Lq(P) = (int)(bits(P) >> 44) - (1023 << 8), the biased exponent and the top 8 mantissa bits.  Zeros and denormals give about
 *     -261888; the clamp takes them.
 *   Tracker, per emitted frame f, with act_f and P_f of the slot's detector in the same call.  mode 2 (follow) and act_f == 0:
 *     target = clamp(Lq(P_f) + offset, l_min, l_max), L += clamp(target - L, -down_step, up_step), idle_frames += 1; act_f == 1: L
 *     holds.  mode 1 (fixed): L = clamp(level, l_min, l_max) on every frame.  A slot without a detector has no frames here: L holds.
 *   Amplitude of frame f, from the level L after the tracker's step of that frame (L <= 0): e = floor(L / 512), r = L - 512 * e in
 *     0 .. 511, a = ldexpf((float)(512 + r), e - 9), which is exact: the octave in e, a linear piece inside it; A_f = a * norm, one f32
 *     product, with norm the cfg's f32: the amplitude of one unit of v at L = 0.
 *   White source.  j = the utterance sample index f * hop + k, f being the front-end frame index the gate uses, taken as int64 in
 *     two's complement (the taps before sample 0 have j < 0); all arithmetic in uint64:
 *       z = seed + (uint64)(j + 1) * 0x9E3779B97F4A7C15;  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;
 *       z *= 0x94D049BB133111EB;  z ^= z >> 31;  w(j) = (int)(z & 0xFFFF) + (int)((z >> 16) & 0xFFFF) - 65535,
 *     triangular in -65535 .. 65535.  A sample depends on seed and j alone, never on the launch, the call cut or the other rows.
 *   Colour.  v(j) = sum_i c[i] * w(j - i) with the integer taps {1} (colour 0), {1, 2, 1} (1) or {1, 2, 3, 2, 1} (2); |v| <= 9 * 65535,
 *     so (float)v is exact.
 *   Fill.  With l the gate's integer of the sample, lvl_prev * (hop - 1 - k) + lvl' * (k + 1) as in the activity section's gain law,
 *     and y the sample behind the gate and the wet/dry mix: lc = ((int64)hop << 20) - l; gc = (float)((double)lc / (double)(hop << 20));
 *     t = (float)v * A_f (one f32 product); out = lc == 0 ? y : fmaf(t, gc, y).  An open gate keeps y's bits, and so does an absent
 *     one: a slot that is not in activity mode 2 counts as open (the bypass's fill_gate rule).  Where both of a frame's gate levels are
 *     2^20 nothing is hashed.
 *   Restart.  The state restarts from level = seed_level, idle_frames = 0 at the slot's first emitted chunk after a reset that includes
 *     CONAN_MODEL_FRONTEND, after a setter call with reseed = 1 and when a slot that was off is enabled.  A setter call with reseed = 0
 *     on an enabled slot replaces the parameters and keeps L.
 * conan_amd/_lib.py's comfort_cfg takes decibels and forms norm = (float)(1 / (sqrt((65536^2 - 1) / 6) * sqrt(sum c^2))) once on the
 * host (the rms of v is 1 at L = 0); it gives follow mode, an offset of -3 dB, limits of -90 .. -30 dBov, a rise of 0.25 dB and a fall
 * of 2 dB per frame, colour 1 and a seed level of -70 dBov.  Those defaults are choices, not measurements. */
typedef struct conan_comfort_cfg {
  int32_t  mode;           /* 0: off (other fields ignored), 1: fixed level, 2: follow the source's background */
  int32_t  reseed;         /* 0 | 1: the state restarts from seed_level */
  int32_t  level;          /* -16384 .. 0: the fixed mode's level */
  int32_t  offset;         /* -16384 .. 16384: added to the quantised frame power in follow mode */
  int32_t  l_min, l_max;   /* -16384 .. 0, l_min <= l_max */
  int32_t  up_step, down_step;   /* 1 .. 16384: the level's largest rise and fall per 20 ms frame */
  int32_t  colour;         /* 0 .. 2 */
  int32_t  seed_level;     /* -16384 .. 0 */
  float    norm;           /* finite, > 0 */
  int32_t  reserved;       /* must be 0 */
  uint64_t seed;           /* of the white source */
} conan_comfort_cfg;       /* 56 bytes */
typedef struct conan_comfort_state {
  int32_t level;           /* L after the last emitted frame */
  int32_t reserved;
  int64_t idle_frames;     /* inactive frames followed since the restart */
} conan_comfort_state;     /* 16 bytes */
/* Sets (cfg->mode = 1 | 2) or removes (0) the comfort noise for `slots`.  Every argument is checked before anything changes
 * (CONAN_ERR_INVALID: mode not 0 .. 2, reseed not 0 / 1, a level outside -16384 .. 0, l_min > l_max, offset outside -16384 .. 16384, a
 * step outside 1 .. 16384, colour outside 0 .. 2, norm not finite or <= 0, reserved not 0), a stream-set without the streaming
 * front-end is CONAN_ERR_STATE, and pending pipelined work is joined; it may be called at any time, also mid-utterance.  The change
 * takes effect from the next emitted chunk and persists across resets.
 * What a slot with the feature does.  Every conan_step_wav[_async] / conan_step_wav_ragged[_ld][_async] call that emits a chunk for it
 * while it also has an activity detector (conan_streams_set_activity, mode 1 or 2) runs the tracker over the chunk's frames - those
 * the detector saw, whose flags and, for a following slot, powers it reads: ONE more launch per call (cnk::comfort_track_kernel,
 * behind the detector's and the bypass's stage; none in calls in which no such slot emits); the detector of such a call also stages
 * its frame powers, with the same kernel.  There is no ring requirement beyond the detector's.  Where the slot is in activity mode 2
 * the chunk's vocoder step fills the rows conv_post wrote, in place, behind the activity gate and the wet/dry mix and in front of the
 * output resampler and the format encoder: ONE more launch (cnk::comfort_fill_kernel) per vocoder step in which such a row takes part
 * - each emit group of a ragged call is such a step - and none otherwise; rows without the feature or without a gate are skipped and
 * keep their bits.  conan_streams_flush_output and the resampler's ring see filled audio.  The mel-in steps (conan_step[_async]) and
 * conan_hifigan_step* take no waveform: they neither track nor fill.
 * Memory: the first enabling call allocates 16 bytes of state per slot, 8 staging sets of (segment + 1) int32 and segment doubles per
 * slot, and 8 row tables; conan_streams_state_bytes counts them from then on.  A stream-set that never calls the setter allocates
 * nothing and runs exactly the launches it ran before.
 * Snapshots carry neither the setting nor the state (the 256-byte host record is full); conan_streams_layout_id and
 * conan_streams_snapshot_bytes do not change.  The hand-over: conan_streams_comfort_state, export, import, then this setter with
 * seed_level = the queried level and reseed = 1 (beside the activity hand-over).  The noise's position needs nothing: it is the
 * front-end's frame position, which snapshots carry. */
int conan_streams_set_comfort(conan_streams* s, const int32_t* slots, int n, const conan_comfort_cfg* cfg, void* stream);
/* Host only: the comfort cfg of `slot` as set, reseed = 0 (mode = 0 and zeros for a slot without one). */
int conan_streams_comfort(const conan_streams* s, int slot, conan_comfort_cfg* cfg_out);
/* The states of `slots` -> state_dev[n], in the order of `stream` behind a join of pipelined work; a slot whose state is about to
 * restart reports its seed.  A slot without the feature is CONAN_ERR_STATE. */
int conan_streams_comfort_state(conan_streams* s, const int32_t* slots, int n, conan_comfort_state* state_dev, void* stream);
/* The frame-end comfort levels the last wav-in call produced, in call order (joins first): level_dev[n][seg], int32.  Rows without
 * the feature (or without a detector), rows that emitted nothing and positions behind the emitted frames read zero.  CONAN_ERR_STATE
 * before any wav-in call. */
int conan_step_wav_comfort(conan_streams* s, int32_t* level_dev, void* stream);
/* The whole-signal tracker, on conan_activity's outputs: act_dev[n][.] (int32) and power_dev[n][.] (double; may be NULL in fixed
 * mode), `frames` frames per row, row stride ld >= frames -> level_out_dev[n][.] (int32, row stride ld: the level after each frame)
 * and state_out_dev[n] (may be NULL).  Every row starts from seed_level.  cfg->mode must be 1 or 2; n in 1 .. 65535.  One launch
 * (cnk::comfort_track_kernel) on `stream`. */
int conan_comfort_track(conan_ctx* ctx, const conan_comfort_cfg* cfg, const int32_t* act_dev, const double* power_dev, int n, int64_t frames, int64_t ld,
                        int32_t* level_out_dev, conan_comfort_state* state_out_dev, void* stream);
/* The fill on whole signals, and the bit-exact yardstick of the streaming one: row i of wav_dev (n rows in 1 .. 65535 of `samples`
 * samples, row stride ld; sample s of a row is sample pos0 + s of the white source, pos0 >= 0, and frame s / hop of the levels) with the
 * frame-end gate levels gate_lvl_dev[i][.] (int32, 0 .. 2^20) and comfort levels comfort_lvl_dev[i][.] (int32, -16384 .. 0), both of row
 * stride lvl_ld >= ceil(samples / hop), and start_gate_level as the gate level before frame 0 -> out_dev (row stride out_ld; may equal
 * wav_dev with out_ld = ld).  start_comfort_level (-16384 .. 0) is the comfort level before frame 0: it is checked, and the law does
 * not read it, because a frame's amplitude is that of its own frame-end level.  seeds: host, n entries (row i's seed), or NULL: every
 * row takes cfg->seed.  Of cfg, colour, norm and seed are read (mode must be 1 or 2).  A last frame that the samples cover only partly
 * is filled over the part they cover.  One launch (cnk::comfort_fill_kernel) on `stream`. */
int conan_comfort_fill(conan_ctx* ctx, int hop, const conan_comfort_cfg* cfg, const uint64_t* seeds, const float* wav_dev, int64_t ld, int n, int64_t samples,
                       int64_t pos0, const int32_t* gate_lvl_dev, const int32_t* comfort_lvl_dev, int64_t lvl_ld, int32_t start_gate_level,
                       int32_t start_comfort_level, float* out_dev, int64_t out_ld, void* stream);

/* Live output levelling (added within ABI 9: a caller detects it by the symbol conan_streams_set_output_level; no existing struct or
 * call changes).  conan_level_cfg's law, exactly as stated above, on the slot's own vocoder audio, with three substitutions: x_t is
 * the slot's model-rate vocoder sample t as conv_post wrote it, position 0 being the slot's first sample after a reset that
 * includes CONAN_MODEL_HIFIGAN (the position conan_slot_info and snapshots already carry); U = segment * hop and u_k = k * U in that
 * position; y replaces x in place, in front of the activity gate, the wet/dry mix, the output resampler and the encoders - the gate
 * mutes levelled audio, the mix sees a levelled wet beside the already levelled dry, conan_streams_flush_output and the resampler's
 * ring see levelled audio; pre_tanh_dev and the taps are not touched.  What follows, bit for bit: a levelled slot's audio over an
 * utterance is conan_level with the same cfg applied to the audio of the same run without the leveller - however the utterance was
 * cut into calls, blocking or pipelined, whatever the other rows of a call were.
 * Rows.  A levelled row of a vocoder step must start at a multiple of U and carry at most U samples: every chunk of
 * conan_step[_async] and of the wav-in steps does, a short last chunk included.  Any other row - a conan_hifigan_step* with
 * frames * hop > U or at a position that is not a multiple of U, the whole-prefix vocoder of upsample 'nn' - is
 * CONAN_ERR_UNSUPPORTED before anything changes; unlevelled rows of the same call are unaffected.  U and fs carry the limits stated
 * above.  Mel-in steps level too: the feature belongs to the vocoder's output, like the output rate.
 * Launches.  G_k and P_k depend only on samples before u_k, so the work is split: ONE launch (cnk::level_out_apply_kernel: two gains
 * from the slot's state, the ramp, the clip) behind conv_post and ONE (cnk::level_out_meter_kernel: the meter over the step's
 * unlevelled samples, which the apply staged, and the next instant's gain) behind the step's last launch, per vocoder step in which
 * a levelled row takes part - each emit group of a ragged call is such a step - and none otherwise.
 * Setter.  cfg->enabled = 0 removes the leveller.  Every argument is checked before anything changes (the cfg by
 * conan_streams_set_input_level's rules), and pending pipelined work is joined.  With seed_dev == NULL every slot must be at vocoder
 * position 0, else CONAN_ERR_STATE.  With a seed the slot may be anywhere: row i of the seed, at i * seed_ld bytes (8-byte aligned,
 * seed_ld a multiple of 8 and at least conan_streams_output_level_state_bytes), is copied into the slot's state on `stream`; the
 * caller vouches that it was queried from a stream at the same position.  The kernels derive every ring index and tail count from
 * the host's position, never from the blob: a wrong blob gives meaningless gains and no access outside the slot's state.  The
 * setting persists across resets; a reset with CONAN_MODEL_HIFIGAN restarts the meter and the gain (the position returns to 0, which
 * the slot's next rows carry: no launch).  Hand-over: state query, conan_streams_export_slots, import, then this call with the seed.
 * Snapshots carry neither setting nor state: conan_streams_layout_id, conan_streams_snapshot_bytes and conan_slot_info do not change.
 * Memory.  The first enabling call allocates, per slot of the stream-set, the state - conan_streams_output_level_state_bytes = 66496
 * bytes: the input leveller's 66464 (meter state and two rings of CONAN_LEVEL_MAX_BLOCKS + 16 doubles) and the previous instant's
 * four stats - and eight staging sets of U floats and one 160-byte table row each: max_slots * (66496 + 8 * (4 * U + 160)) bytes,
 * which conan_streams_state_bytes counts from then on.  A stream-set that never calls the setter allocates nothing and runs exactly
 * the launches it ran before. */
int conan_streams_set_output_level(conan_streams* s, const int32_t* slots, int n, const conan_level_cfg* cfg, const void* seed_dev, int64_t seed_ld,
                                   void* stream);
/* Host only: the output level cfg of `slot` as set (zeros for a slot without one). */
int conan_streams_output_level_cfg(const conan_streams* s, int slot, conan_level_cfg* cfg_out);
/* Joins pending pipelined work, then writes per slot {L_k, G_k, P_k, J_k} (stats_dev[n][4], device) on `stream` for
 * k = (voc_samples - 1) / U, voc_samples = the slot's vocoder position; before any sample {-inf, G_{-1}, 0, 0}: row k of conan_level's
 * trace on the audio so far.  A slot without the leveller is CONAN_ERR_STATE. */
int conan_streams_output_level(conan_streams* s, const int32_t* slots, int n, double* stats_dev, void* stream);
/* Bytes of one slot's output level state (negative: an error code). */
int64_t conan_streams_output_level_state_bytes(const conan_streams* s);
/* The states of `slots` -> row i at state_dev + i * ld bytes (8-byte aligned, ld a multiple of 8 and at least the state's bytes), on
 * `stream` behind a join of pipelined work.  A slot without the leveller is CONAN_ERR_STATE. */
int conan_streams_output_level_state(conan_streams* s, const int32_t* slots, int n, void* state_dev, int64_t ld, void* stream);

/* Input loss concealment (added within ABI 9: a caller detects it by the symbol conan_streams_set_conceal; no existing struct or call
 * changes).  A server that assembles an 80 ms chunk from 20 ms packets marks the packets that never arrived, and the library fills
 * them from the slot's own recent audio before the chunk is stepped: the repair runs on the caller's device row IN FRONT OF the
 * wav-in step call, in place and in the slot's input format, so decoding, the input resampler, the leveller, the pitch follower, the
 * activity detector and the bypass's dry path all see the repaired row.  No step path changes.
 * The law (tests/conceal_ref.py restates it in numpy with Python integers).  Everything is per slot, at the slot's input rate, in
 * sample positions t = 0, 1, ... counted from the last restart.  y[t] is the decoded repaired signal - what the step call decodes
 * from the row after the repair - and y[t] = 0 for t < 0.  dec and enc are the sample formats' rules (conan_convert_samples: decoding
 * is exact, encoding rounds to nearest even and saturates; the identity for f32).  lost[t] is the flag of the packet that holds t:
 * packet m covers [m * packet, (m + 1) * packet) counted from the start of the row (conan_streams_conceal) or from position 0
 * (conan_conceal); the two agree when every row but the last is a multiple of `packet` long.  A non-zero flag means lost.
 * State: mode (0 idle, 1 run, 2 fade), p, k (samples since the run began), j (fade samples done), a template T[0 .. p-1] and the last
 * window + lag_max values of y.  For t in order:
 *   Lost sample.  If mode != 1 a run starts:
 *     Lag.  With q[i] the f32 -> s16 value of y[i] (clamp(rint(y * 32768))), D(p) = sum over i = 1 .. window of
 *       (q[t-i] - q[t-i-p])^2 in int64; p is the smallest lag in [lag_min, lag_max] with minimal D (an all-zero history gives lag_min).
 *       The difference function and not a normalised correlation: it is exact in integers, so every implementation agrees on p.
 *     Template.  T[i] = y[t-p+i]; k = 0; mode = 1.
 *   Then v = T[k mod p] * g(k), one f32 product; the row's sample becomes enc(v), y[t] = dec(enc(v)), k += 1.
 *     Level.  l(k) = 2^20 for k < hold; floor(((hold + fall - k) << 20) / fall) for hold <= k < hold + fall; 0 beyond.
 *       g = (float)((double)l / 2^20).
 *   Received sample.  x = dec(row[t]).  If mode == 1: j = 0 and mode becomes 2 when fade > 0, else 0.  If mode == 2:
 *     l_in = floor(((j + 1) << 20) / (fade + 1)), l_out = 2^20 - l_in, gains formed as in Level; s = T[k mod p] * g(k), one f32 product;
 *     v = fma(s, g_out, x * g_in), one f32 product and one f32 fused multiply-add; the row's sample becomes enc(v), y[t] = dec(enc(v)),
 *     k += 1, j += 1, and mode = 0 once j == fade.  Otherwise y[t] = x and the row's bytes are NOT written.
 * A loss that begins during a fade is a new run whose lag search reads the faded y.  There is no overlap-add into samples already
 * delivered: the repair adds no latency.  Nothing here has a tolerance, and the result depends only on positions, never on how the
 * signal is cut into calls.  The state restarts (mode = 0, history zero) at the slot's first repair call after a reset that includes
 * CONAN_MODEL_FRONTEND, when a slot that was off is enabled, and from seed_dev when the setter passes one.
 * Defaults for a rate R (conan_amd._lib.conceal_keywords): packet R/50 (20 ms), lag_min R/400 (2.5 ms), lag_max R*15/1000 (15 ms),
 * window R/50 (20 ms), hold R/100 (10 ms), fall R/20 (50 ms), fade R/200 (5 ms); at 48 kHz every one lies within the limits. */
#define CONAN_CONCEAL_MAX_LAG 1024
#define CONAN_CONCEAL_MAX_WINDOW 1024
typedef struct conan_conceal_cfg {
  int32_t enabled;   /* 0: off (other fields ignored) | 1 */
  int32_t packet;    /* samples per loss flag, >= 1 */
  int32_t lag_min;   /* 1 <= lag_min <= lag_max <= CONAN_CONCEAL_MAX_LAG */
  int32_t lag_max;
  int32_t window;    /* 1 .. CONAN_CONCEAL_MAX_WINDOW: samples compared by the lag search */
  int32_t hold;      /* >= 0: samples of a run at full level */
  int32_t fall;      /* >= 1: samples over which the level then falls to zero */
  int32_t fade;      /* 0 .. 1024: samples of cross-fade back into received audio */
} conan_conceal_cfg; /* 32 bytes */
/* Sets (cfg->enabled = 1) or removes (0) the concealment for `slots`.  Every argument is checked before anything changes
 * (CONAN_ERR_INVALID: a field outside its range, a seed that is misaligned or whose rows are too close), a stream-set without the
 * streaming front-end is CONAN_ERR_STATE, and pending pipelined work is joined; it may be called at any time, also mid-utterance, and
 * the setting persists across resets.  A setter call on an enabled slot without a seed replaces the fields and keeps the state.
 * seed_dev (may be null): row i at seed_dev + i * seed_ld bytes is a record as conan_streams_conceal_state writes it, and becomes the
 * state of slots[i] on `stream`.
 * Memory: the first enabling call allocates conan_conceal_state_bytes() per slot and 4 row tables; conan_streams_state_bytes counts
 * them from then on.  A stream-set that never calls the setter allocates nothing and runs exactly the launches it ran before; the step
 * calls of a stream-set that does run exactly the launches they ran before, too.
 * Snapshots carry neither the setting nor the state; conan_streams_layout_id and conan_streams_snapshot_bytes do not change.  The
 * hand-over: conan_streams_conceal_state, export, import, then this setter with the record as seed_dev. */
int conan_streams_set_conceal(conan_streams* s, const int32_t* slots, int n, const conan_conceal_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream);
/* Host only: the concealment cfg of `slot` as set (zeros for a slot without one). */
int conan_streams_conceal_cfg(const conan_streams* s, int slot, conan_conceal_cfg* cfg_out);
/* Repairs row i in place: samples[i] (host, >= 0) samples in the input format of slots[i] at wav_dev + i * wav_ld * 4 bytes (the step
 * calls' row stride), from the int32 flags lost_dev[i * lost_ld + 0 .. ceil(samples[i] / packet) - 1].  ONE launch
 * (cnk::conceal_kernel, one workgroup per repaired row) on `stream`; rows of slots without the feature and rows with samples[i] = 0
 * are skipped and keep their bytes, and a call with no row to repair launches nothing and returns CONAN_OK.  The caller orders it in
 * front of the step call on the same stream, as it orders its own upload of the row. */
int conan_streams_conceal(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, void* wav_dev, int64_t wav_ld, const int32_t* lost_dev,
                          int64_t lost_ld, void* stream);
/* Bytes of one slot's concealment state: a fixed-size, position-independent record - a 32-byte header {int32 mode, p, j, reserved;
 * int64 k, reserved}, the template (CONAN_CONCEAL_MAX_LAG floats, T[0 .. p-1] first) and the last CONAN_CONCEAL_MAX_LAG +
 * CONAN_CONCEAL_MAX_WINDOW values of y, oldest first (the law reads the last window + lag_max of them). */
int64_t conan_conceal_state_bytes(void);
/* The states of `slots` -> row i at state_dev + i * ld bytes (8-byte aligned, ld a multiple of 8 and at least the record's bytes), on
 * `stream` behind a join of pipelined work.  A slot about to restart reports the zero state; a slot without the feature is
 * CONAN_ERR_STATE. */
int conan_streams_conceal_state(conan_streams* s, const int32_t* slots, int n, void* state_dev, int64_t ld, void* stream);
/* The law on whole signals from the zero state, in place, and the bit-exact yardstick of the streaming form: row i (n rows in
 * 1 .. 65535) holds samples[i] (host) samples of `format` (CONAN_SAMPLE_*) at x_dev + i * ld * 4 bytes, its flags are
 * lost_dev[i * lost_ld + .].  cfg->enabled must be 1.  One launch of the same kernel, which walks a row in tiles. */
int conan_conceal(conan_ctx* ctx, const conan_conceal_cfg* cfg, int format, void* x_dev, int64_t ld, int n, const int64_t* samples, const int32_t* lost_dev,
                  int64_t lost_ld, void* stream);

/* Acoustic echo cancellation (added within ABI 9: a caller detects it by the symbol conan_streams_set_echo; no existing struct or call
 * changes).  The far party's audio leaves the caller's loudspeaker and comes back in the caller's microphone; left alone it is converted
 * and sent back, opens the activity gate and is metered as speech.  The canceller is an integer block-NLMS filter per slot: it runs on
 * the caller's device row IN FRONT OF the wav-in step call and behind conan_streams_conceal, in place, in the slot's input format and at
 * its input rate, from a second row that holds what the host sent to this caller's earpiece.  No step path changes.
 * The law (tests/echo_ref.py restates it in numpy with int64 integers).  Everything is per slot; positions t = 0, 1, ... count from the
 * last restart.  dec / enc are the sample formats' rules as in the concealment, q(v) = clamp(rint(v * 32768), -32768, 32767) its 16-bit
 * view.  Mic: m[t] = dec(row[t]) in f32 with a non-finite value counted as 0, d[t] = q(m[t]).  Far end: x[t] = q(dec(far[t])) (a
 * non-finite value counts as 0), x[t] = 0 for t < 0, delayed: x'[t] = x[t - delay].  The far row has the mic row's format, rate and
 * length (conan_resample / conan_convert_samples bring it there).  B = CONAN_ECHO_BLOCK, L = taps, the weights w[k] are int32 in Q24.
 *   Filter, for every t: S = sum over k < L of w[k] * x'[t-k] in int64 (|S| < 2^57); yh = clamp(floor((S + 2^23) / 2^24), -32768,
 *     32767); e[t] = d[t] - yh; the row's sample becomes enc(m[t] - (float)yh * 2^-15) - one f32 subtraction, the second operand is
 *     exact.  A sample with yh = 0 is NOT written and keeps its bytes.  w is constant within a block [jB, (j+1)B), so a sample is
 *     emitted in the call that brings it, whatever the cut: no pending output, no latency.
 *   End of a complete block [b0, b1): D = sum d^2, E = sum e^2 (int64) and dmax = max |d| over the block; P = sum of x'[u]^2 for u in
 *     [b1-L, b1-1]; xmax = max |x'[u]| for u in [b0-L+1, b1-1].  Then, in this order:
 *     1. Guard.  If E > 4 * D + 4096: w = 0, shift = min(shift + 1, CONAN_ECHO_MAX_SHIFT), trips += 1, and NOTHING else happens in this
 *        block (the detector's hcnt keeps its value).
 *     2. Double talk (Geigel).  cond = dt_den > 0 and dmax * dt_den > xmax * dt_num (int64 products).  The block is frozen when cond
 *        holds or hcnt > 0 (its value BEFORE this step).  Then: if cond, hcnt = hang; else if hcnt > 0, hcnt -= 1.  A frozen block
 *        counts frozen += 1 and has no update.
 *     3. Idle far end.  P < far_min: no update.
 *     4. Update.  G[k] = sum over t in the block of e[t] * x'[t-k] (int64, |G| < 2^37); w[k] = clamp(w[k] + (G[k] * 2^(24 - shift)) /
 *        (P + reg), -(2^31 - 1), 2^31 - 1) with C's int64 division (toward zero; |numerator| < 2^61); adapted += 1.
 * shift starts at mu_shift.  All sums are exact integers: every reduction order and every cut into calls gives the same bits.
 * B = 64 and Q24 are choices; no other value was built or timed.
 * The state restarts (all zero, shift = mu_shift) at the slot's first echo call after a reset that includes CONAN_MODEL_FRONTEND and
 * when a slot that was off is enabled; a seed replaces it with the seeded record.
 * Defaults for a rate R (conan_amd._lib.echo_keywords): taps = min(2048, 64 ms rounded to a multiple of 64), delay 0, mu_shift 4,
 * dt 1/2, hang = 50 ms in blocks (rounded up), reg = taps * 4096, far_min = taps * 1024.  Choices, not measurements. */
#define CONAN_ECHO_BLOCK 64
#define CONAN_ECHO_MAX_TAPS 2048
#define CONAN_ECHO_MAX_DELAY 4096
#define CONAN_ECHO_MAX_SHIFT 12
#define CONAN_ECHO_HISTORY 6208 /* far samples a state record keeps: >= MAX_TAPS + BLOCK - 1 + MAX_DELAY */
typedef struct conan_echo_cfg {
  int32_t enabled;   /* 0: off (other fields ignored) | 1 */
  int32_t taps;      /* filter length L: a multiple of 64 in 64 .. CONAN_ECHO_MAX_TAPS */
  int32_t delay;     /* 0 .. CONAN_ECHO_MAX_DELAY: bulk delay of the far end, in samples */
  int32_t mu_shift;  /* 0 .. CONAN_ECHO_MAX_SHIFT: starting value of shift */
  int32_t dt_num;    /* >= 0: Geigel numerator */
  int32_t dt_den;    /* >= 0: Geigel denominator; 0 turns the detector off */
  int32_t hang;      /* >= 0: hang-over, in blocks */
  int32_t reserved;  /* ignored */
  int64_t reg;       /* 1 .. 2^60: regulariser */
  int64_t far_min;   /* >= 0: idle threshold on P */
} conan_echo_cfg; /* 48 bytes */
/* Sets (cfg->enabled = 1) or removes (0) the canceller for `slots`, with conan_streams_set_conceal's semantics point for point: every
 * argument is checked before anything changes (CONAN_ERR_INVALID: a field outside its range, a seed that is misaligned or whose rows are
 * too close), a stream-set without the streaming front-end is CONAN_ERR_STATE, pending pipelined work is joined, and the setting
 * persists across resets.  A setter call on an enabled slot without a seed replaces the fields and keeps the state: a changed `taps`
 * keeps the weights that still exist and zeroes the rest (a record always holds zeros in w[taps ..]), a changed `delay` reads the far
 * history the record already holds, and shift keeps its value.
 * seed_dev (may be null): row i at seed_dev + i * seed_ld bytes is a record as conan_streams_echo_state writes it and becomes the state
 * of slots[i] on `stream`; the call reads each seed's `pos` back (one small copy and a wait on `stream`), because the host, not the
 * record, tells the kernel where in a block a slot stands.
 * Memory: the first enabling call allocates conan_echo_state_bytes() per slot and 4 row tables; conan_streams_state_bytes counts them
 * from then on.  A stream-set that never calls the setter allocates nothing and runs exactly the launches it ran before; the step
 * calls of a stream-set that does run exactly the launches they ran before, too.  Snapshots carry neither the setting nor the state. */
int conan_streams_set_echo(conan_streams* s, const int32_t* slots, int n, const conan_echo_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream);
/* Host only: the echo cfg of `slot` as set (zeros for a slot without one). */
int conan_streams_echo_cfg(const conan_streams* s, int slot, conan_echo_cfg* cfg_out);
/* Cancels row i in place: samples[i] (host, >= 0) samples in the input format of slots[i] at wav_dev + i * wav_ld * 4 bytes (the step
 * calls' row stride), the far end in the same format at far_dev + i * far_ld * 4 bytes.  ONE launch (cnk::echo_kernel, one workgroup
 * per cancelled row) on `stream`; rows of slots without the feature and rows with samples[i] = 0 are skipped and keep their bytes, and
 * a call with no row to cancel launches nothing and returns CONAN_OK.  The caller orders it in front of the step call and behind
 * conan_streams_conceal on the same stream.
 * stats_dev (may be null): int64 [n][4], row i = {sum d^2, sum e^2 over this call's samples, blocks adapted, blocks frozen that
 * completed in this call}; the host forms ERLE = 10 log10(sum d^2 / sum e^2) from them.  A skipped row reports zeros (when a call
 * skips a row, the table is cleared by one memset in front of the launch). */
int conan_streams_echo(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, void* wav_dev, int64_t wav_ld, const void* far_dev,
                       int64_t far_ld, int64_t* stats_dev, void* stream);
/* Bytes of one slot's canceller state: a fixed-size, position-independent record, little endian -
 *   0  int64 pos (samples since the restart; pos mod 64 values of e are pending)    8  int32 shift   12  int32 hcnt
 *  16  int64 adapted, frozen, trips      40  int64 D, E of the pending block        56  int32 dmax   60  int32 reserved (0)
 *  64  int32 w[CONAN_ECHO_MAX_TAPS] (zeros from `taps` on)      then int32 e[CONAN_ECHO_BLOCK] of the pending block (zeros behind them)
 *  then int16 x[CONAN_ECHO_HISTORY]: the last far samples before `pos`, oldest first, UNdelayed (the law reads the last taps + 63 + delay). */
int64_t conan_echo_state_bytes(void);
/* The states of `slots` -> row i at state_dev + i * ld bytes (8-byte aligned, ld a multiple of 8 and at least the record's bytes), on
 * `stream` behind a join of pipelined work.  A slot about to restart reports the restart state (zeros, shift = mu_shift); a slot
 * without the feature is CONAN_ERR_STATE. */
int conan_streams_echo_state(conan_streams* s, const int32_t* slots, int n, void* state_dev, int64_t ld, void* stream);
/* The law on whole signals from the zero state, in place, and the bit-exact yardstick of the streaming form: row i (n rows in
 * 1 .. 65535) holds samples[i] (host) samples of `format` (CONAN_SAMPLE_*) at x_dev + i * ld * 4 bytes, its far end lies at
 * far_dev + i * far_ld * 4 bytes.  cfg->enabled must be 1.  stats_dev as above (may be null).  One launch of the same kernel, which
 * walks a row block by block. */
int conan_echo(conan_ctx* ctx, const conan_echo_cfg* cfg, int format, void* x_dev, int64_t ld, const void* far_dev, int64_t far_ld, int n,
               const int64_t* samples, int64_t* stats_dev, void* stream);

/* Echo delay (added within ABI 9: a caller detects it by the symbol conan_streams_set_echo_delay; no existing struct or call changes).
 * The canceller above cancels what lies inside `taps` samples behind a bulk `delay` the host must supply, and the host cannot know it:
 * it is the round trip through the far device's playout buffer, loudspeaker, room, microphone, the network and the jitter buffer,
 * typically 50 to 300 ms, and it moves during a call.  It can only be measured by comparing the mic row with the far row, and no
 * sample of a slot reaches the host.  The estimator does that per slot on the GPU: it READS the rows in front of the canceller and
 * reports a lag; the host turns the report into the canceller's `delay` (conan_amd._lib.echo_delay_follow is one rule).
 * The law (tests/echo_delay_ref.py restates it in numpy with Python / int64 integers).  Everything is per slot, at the slot's input
 * rate, in positions t = 0, 1, ... since the last restart.  d[t] = q(dec(mic[t])) and x[t] = q(dec(far[t])) are the canceller's 16-bit
 * views (q, dec and the non-finite -> 0 rule as above); x[t] = 0 for t < 0.
 *   Ternary signs: sgn(v) = +1 if v >= thr, -1 if v <= -thr, else 0.  An idle far end, or A-law's 8-LSB silence under a thr above 8,
 *     contributes nothing: there is no separate idle test.
 *   Accumulation, for every t and every lag l in 0 .. n_lags - 1: A[l] += sgn(d[t]) * sgn(x[t - l]).  A is int32, and A[l] = 0 for
 *     l >= n_lags, always (a setter can change n_lags without touching the rest; the rule of w[taps ..] above).
 *   Frame end, W = CONAN_ECHO_DELAY_FRAME: when the sample at position t with (t + 1) mod W == 0 has been added, in this order:
 *     1. a[l] = |A[l]|; p = the smallest l < n_lags that maximises a; pk = a[p]; s = sum of a (int64).
 *     2. ok = pk >= min_peak and pk * n_lags > ratio * s (int64 products).
 *     3. If ok and cand >= 0 and |p - cand| <= tol: run += 1; else if ok: run = 1; else run = 0.  Then cand = ok ? p : -1.
 *     4. If run >= hold: est = p, age = 0; else if est >= 0: age = min(age + 1, 2^31 - 1).
 *     5. frames += 1, last_pk = pk, last_s = s.
 *     6. Leak: A[l] -= A[l] >> leak for l < n_lags (an arithmetic shift: it floors).
 *   The restart value is all zero with est = cand = -1.
 * Bounds: a frame adds at most W to |A[l]| and the leak takes floor(A / 2^leak), so |A| <= (W + 1) * 2^leak (<= 262400 at leak 8: int32
 * with room); with leak <= 8 and n_lags <= 6144, s <= 6144 * 262400 < 2^31.6, so s and both products need int64 (pk * n_lags < 2^31,
 * ratio * s < 2^63).  All sums are exact integers and the leak and the decision happen only at fixed multiples of W: every reduction
 * order and every cut into calls gives the same bits.  W = 1024 and the ternary signs are choices; nothing else was built or timed.
 * The state restarts at the slot's first estimator call after a reset that includes CONAN_MODEL_FRONTEND and when a slot that was off
 * is enabled; a seed replaces it with the seeded record.
 * Defaults for a rate R (conan_amd._lib.echo_delay_keywords): n_lags = min(6144, 384 ms rounded to a multiple of 64), thr 16, leak 5,
 * ratio 10, min_peak 1024, hold 4, tol = 2 ms.  Choices, not measurements (DESIGN.md 4.29 says what the reference measures with them). */
#define CONAN_ECHO_DELAY_FRAME 1024
#define CONAN_ECHO_DELAY_MAX_LAGS 6144 /* CONAN_ECHO_MAX_DELAY + CONAN_ECHO_MAX_TAPS */
typedef struct conan_echo_delay_cfg {
  int32_t enabled;     /* 0: off (other fields ignored) | 1 */
  int32_t n_lags;      /* lags 0 .. n_lags - 1: a multiple of 64 in 64 .. CONAN_ECHO_DELAY_MAX_LAGS */
  int32_t thr;         /* 1 .. 32767: the ternary threshold on the 16-bit view */
  int32_t leak;        /* 1 .. 8: A loses A >> leak at every frame end */
  int32_t ratio;       /* >= 1: the peak must exceed `ratio` times the mean of |A| */
  int32_t min_peak;    /* >= 1: ... and reach this value */
  int32_t hold;        /* >= 1: frames in a row a candidate must stand before it becomes est */
  int32_t tol;         /* >= 0: how far a candidate may move between frames, in samples */
  int32_t reserved[4]; /* ignored */
} conan_echo_delay_cfg; /* 48 bytes */
/* Sets (cfg->enabled = 1) or removes (0) the estimator for `slots`, with conan_streams_set_echo's semantics point for point: every
 * argument is checked before anything changes, a stream-set without the streaming front-end is CONAN_ERR_STATE, pending pipelined work
 * is joined, the setting persists across resets.  A setter call on an enabled slot without a seed replaces the fields and keeps the
 * state: a changed n_lags keeps A[l] for l below both values and zeroes the rest.  seed_dev (may be null): row i at seed_dev + i *
 * seed_ld bytes is a record as conan_streams_echo_delay_state writes it and becomes the state of slots[i] on `stream` (with A[n_lags ..]
 * cleared, should the record come from a slot with more lags); the call reads
 * each seed's `pos` back (one small copy and a wait on `stream`), because the host tells the kernel where in a frame a slot stands.
 * Memory: the first enabling call allocates conan_echo_delay_state_bytes() per slot and 4 row tables; conan_streams_state_bytes counts
 * them from then on.  A stream-set that never calls the setter allocates nothing and runs exactly the launches it ran before; the step
 * calls of one that does run exactly the launches they ran before, too.  Snapshots carry neither the setting nor the state.  The slot
 * needs no canceller. */
int conan_streams_set_echo_delay(conan_streams* s, const int32_t* slots, int n, const conan_echo_delay_cfg* cfg, const void* seed_dev, int64_t seed_ld,
                                 void* stream);
/* Host only: the estimator's cfg of `slot` as set (zeros for a slot without one). */
int conan_streams_echo_delay_cfg(const conan_streams* s, int slot, conan_echo_delay_cfg* cfg_out);
/* Reads row i - samples[i] (host, >= 0) samples in the input format of slots[i] at wav_dev + i * wav_ld * 4 bytes, the far end in the
 * same format at far_dev + i * far_ld * 4 bytes - and writes NEITHER.  ONE launch (cnk::echo_delay_kernel, one workgroup per row) on
 * `stream`; rows of slots without the feature and rows with samples[i] = 0 are skipped, and a call with no row to do launches nothing
 * and returns CONAN_OK.  The caller orders it behind conan_streams_conceal and IN FRONT OF conan_streams_echo on the same stream: the
 * canceller rewrites the mic row.
 * report_dev (may be null): int64 [n][6], row i = {est, age, cand, run, last_pk, last_s} after the call; est is the confirmed lag in
 * samples or -1, age the frames since it was last confirmed.  A skipped row reports zeros (when a call skips a row, the table is
 * cleared by one memset in front of the launch). */
int conan_streams_echo_delay(conan_streams* s, const int32_t* slots, int n, const int32_t* samples, const void* wav_dev, int64_t wav_ld, const void* far_dev,
                             int64_t far_ld, int64_t* report_dev, void* stream);
/* Bytes of one slot's estimator state: a fixed-size, position-independent record, little endian -
 *   0  int64 pos (samples since the restart; pos mod 1024 of them lie in the open frame)
 *   8  int32 est   12  int32 age   16  int32 cand   20  int32 run      24  int64 frames, last_pk, last_s      48  16 bytes reserved (0)
 *  64  int32 A[CONAN_ECHO_DELAY_MAX_LAGS] (zeros from n_lags on)
 *  then int8 h[CONAN_ECHO_DELAY_MAX_LAGS]: h[0] = 0, h[1 ..] the far end's last 6143 ternary values before `pos`, oldest first. */
int64_t conan_echo_delay_state_bytes(void);
/* The states of `slots` -> row i at state_dev + i * ld bytes (8-byte aligned, ld a multiple of 8 and at least the record's bytes), on
 * `stream` behind a join of pipelined work.  A slot about to restart reports the restart state; a slot without the feature is
 * CONAN_ERR_STATE. */
int conan_streams_echo_delay_state(conan_streams* s, const int32_t* slots, int n, void* state_dev, int64_t ld, void* stream);
/* The law on whole signals from the zero state, and the bit-exact yardstick of the streaming form: row i (n rows in 1 .. 65535) holds
 * samples[i] (host) samples of `format` (CONAN_SAMPLE_*) at mic_dev + i * ld * 4 bytes, its far end lies at far_dev + i * far_ld * 4
 * bytes.  cfg->enabled must be 1.  track_dev (may be null): int64 rows track_ld apart (in int64), row i holds the report after each of
 * its samples[i] / 1024 frame ends, six values per frame; track_ld must hold them.  report_dev (may be null): as above, after the last
 * sample.  One launch of the same kernel, which walks a row frame by frame. */
int conan_echo_delay(conan_ctx* ctx, const conan_echo_delay_cfg* cfg, int format, const void* mic_dev, int64_t ld, const void* far_dev, int64_t far_ld, int n,
                     const int64_t* samples, int64_t* track_dev, int64_t track_ld, int64_t* report_dev, void* stream);

/* Silence trimming (added within ABI 9: a caller detects it by the exported symbol; no existing struct or call changes).  The offline
 * half of source activity: the reference's trim_long_sil (utils/audio/vad.py, trim_long_silences) cuts the long pauses out of a whole
 * recording - a moving average over an external detector's flags, a dilation that keeps short pauses, a hard cut - and this call does
 * the same on the detector above, for enrolment clips, whole-utterance conversion and recorded calls whose per-frame flags a server
 * already holds.  The law is all integer, so the GPU, numpy (tests/trim_ref.py) and any cut into launches agree bit for bit.
 *   Input.  A row of len f32 samples at the rate conan_activity accepts (sample_rate == 50 * hop).  The row has F = 1 + len / hop frames,
 *     as in the detector.  Frame f owns samples f * hop .. min((f + 1) * hop, len) - 1, the gate's convention: the last frame owns
 *     len % hop samples, possibly none.
 *   1. Flags.  act[f] is 0 or 1: conan_activity's flags for the row from the cfg's seed (the same kernel, the same bits), or flags the
 *     caller supplies (any non-zero counts as 1).
 *   2. Smoothing.  w = smooth_frames.  S[f] = the sum of act[j], j in [f - (w - 1) / 2, f + w / 2] (integer divisions; zeros outside
 *     0 .. F-1).  m1[f] = 2 * S[f] > w.  This is the reference's centred moving average followed by np.round: a window that is exactly
 *     half active rounds to even, that is to 0.
 *   3. Dilation.  s = max_silence_frames + 1.  m2[f] = the OR of m1[j], j in [f - (s - 1 - s / 2), f + s / 2], clipped to 0 .. F-1:
 *     scipy.ndimage.binary_dilation(m1, ones(s)), including its off-centre origin for even s.
 *   4. Compaction.  cnt[f] = the number of samples frame f owns; off[f] = the sum of cnt[j] over j < f with m2[j] set;
 *     out[off[f] + k] = wav[f * hop + k] for every kept frame, as a bit copy (NaN payloads and -0.0 survive); out_len = the sum of
 *     cnt[f] * m2[f]; out[out_len .. len-1] = 0; nothing past len is written.  Cuts are hard, as in the reference: they fall in
 *     stretches the detector called silent.
 * conan_amd/_lib.py's trim_cfg gives smooth_frames = 12 and max_silence_frames = 18: the reference's 8 and 12 windows of 30 ms kept as
 * durations on 20 ms frames.  Those defaults are choices, not measurements.  Both window steps are differences of prefix sums, so
 * their width is free: smooth_frames 1 .. 65536, max_silence_frames 0 .. 65536. */
typedef struct conan_trim_cfg {
  int32_t smooth_frames;        /* w, 1 .. 65536 */
  int32_t max_silence_frames;   /* s - 1, 0 .. 65536: the longest pause (between kept stretches) that is kept whole */
  int32_t reserved[2];          /* must be 0 */
} conan_trim_cfg;          /* 16 bytes */
/* wav_dev: n rows (1 .. 65535) of `samples` samples (1 .. 2^30), row stride ld >= samples; lengths[n] (host; NULL: every row has
 * `samples`) in 1 .. samples.  `mel` is read as conan_activity reads it (fft_size, hop_size, sample_rate == 50 * hop_size).  Exactly one
 * of act_cfg (the detector runs: mode 1 or 2, every row from the seed) and act_in_dev (int32 rows of stride act_ld >= the frames of
 * every row) is given.  out_dev: rows of stride out_ld >= samples, which must not overlap wav_dev's (a parallel move towards lower
 * addresses races: CONAN_ERR_INVALID); NULL: plan only, no audio is written.  mask_out_dev (int32, m2) and offset_out_dev (int64: off[f],
 * or -1 for a dropped frame), rows of stride frame_ld >= the frames of every row, and out_len_dev[n] (int64) may each be NULL.  Every
 * argument is checked before anything is launched.  Asynchronous on `stream`: at most three launches (cnk::activity_kernel when act_cfg
 * is given, cnk::trim_plan_kernel, cnk::trim_gather_kernel when out_dev is given); scratch comes from the context's workspace, which
 * conan_wav2mel, conan_loud_norm and conan_activity share: calls on one context are ordered by the caller. */
int conan_trim_silence(conan_ctx* ctx, const conan_mel_cfg* mel, const conan_activity_cfg* act_cfg, const conan_trim_cfg* cfg,
                       const float* wav_dev, int64_t ld, int n, int64_t samples, const int64_t* lengths, const int32_t* act_in_dev, int64_t act_ld,
                       float* out_dev, int64_t out_ld, int32_t* mask_out_dev, int64_t* offset_out_dev, int64_t frame_ld, int64_t* out_len_dev,
                       void* stream);

/* Voice bank (added within ABI 9: a caller detects it by the exported symbols; no existing struct or call changes).  A bank holds the
 * result of conan_set_reference's style pass for up to `capacity` target voices in device memory, outside any slot: the style vector,
 * both aligner layers' K/V rows of the prosody tokens, their key mask, the token count and the VQ ids.  A server enrols its catalogue
 * once; starting a call, or changing a call's voice mid-utterance, is then conan_streams_set_voice: one upload of the call's rows and
 * one launch (cnk::voice_assign_kernel) instead of a style pass, and no reference mel to upload.
 *
 * conan_voices_create: capacity >= 1 entries for references of up to max_ref_frames (4 .. 2048) frames on ctx's device (a context with
 *   a Conan model, finalized).  conan_voices_destroy waits for the device.  Neither is stream-ordered.
 * conan_voices_enroll: the style pass of ref_mel_dev[n][max_len][num_mels] / ref_len[n] (host), exactly as conan_set_reference runs it,
 *   into entries ids[i] (0 .. capacity-1, distinct) - on the workspace and launch plan of `via`, a stream-set of the bank's context
 *   (else CONAN_ERR_INVALID), ONE voice per pass whatever via's flags, in the order of `stream` behind a join of via's pipelined work.
 *   An entry's bits therefore do not depend on what it was enrolled with, and equal those of conan_set_reference(via, one slot, the
 *   same mel).  ref_len[i] must be 1 .. min(max_len, the bank's max_ref_frames, via's): else CONAN_ERR_INVALID, nothing enqueued.
 *   Enrolling an id again replaces it.  The call uses via's slot table: it must not overlap via's pipelined steps from another thread.
 * conan_voices_remove: host only; the ids become "not enrolled" (an id that is not enrolled is skipped).
 * conan_voices_info: host only; enrolled = 0 for an id that holds no voice.
 * conan_streams_set_voice: slot slots[i] (distinct, as every slot list) gets voice voice_ids[i] (ids may repeat).  Every row is checked
 *   before anything changes: a bank of another context or an id out of range is CONAN_ERR_INVALID, an id that is not enrolled
 *   CONAN_ERR_STATE, a voice with more tokens than the stream-set holds ((max_ref_frames + 3) / 4) CONAN_ERR_SHAPE.  Host bookkeeping
 *   (the slot has a reference; conan_streams_voice) changes at once; the device write runs in the order of `stream` behind a join of
 *   pending pipelined work, like conan_streams_set_pitch: steps already enqueued still run with the old voice, the next step uses the
 *   new one.  The bank's and the stream-set's max_ref_frames may differ.  Rows past the voice's token count are written as
 *   conan_set_reference leaves them in a freshly created slot (mask 0, ids -1, K/V 0): a slot's cache is a function of the voice
 *   alone.  It is a COPY: enrolling the id again, removing it or destroying the bank later (destroy waits for the device) does not
 *   change the slot, and slot snapshots carry it like any other reference.
 * conan_streams_set_voice_mix: as above with the prosody side (K/V, mask, count, ids) of voice_ids[i][0] and the style vector
 *   w[i][0] * style_0, then fmaf(w[i][j], style_j, .) for j = 1 .. k-1 in fp32, in the same launch - Conan.forward(spk_embed=...)
 *   with a blended vector.  1 <= k <= 4; weights (host) must be finite and are not normalised.  k = 1 with weight 1 gives
 *   conan_streams_set_voice's bits.
 * conan_streams_voice: host only; the id last assigned WHOLE to `slot` (conan_streams_set_voice), -1 otherwise: never assigned, or
 *   since then conan_set_reference, conan_set_style, a mix or a snapshot import.  The id is the caller's: the stream-set does not know
 *   whether the bank still holds that voice.
 * Persistence.  conan_voices_export writes entry ids[i] to row i of blob_dev (device, 16-byte aligned, rows blob_ld_bytes apart, a
 *   multiple of 16) and its record to meta_host[i]; one launch on `stream`.  A row is sized by the voice's tokens alone -
 *   style [hidden_size], count, ids [tokens], mask [tokens], then per layer the K/V rows [tokens][2 * hidden_size], each region padded
 *   to 16 bytes, padding zero - and holds no pointers or indices.  conan_voices_blob_bytes: what a row of this bank can need (a
 *   multiple of 256); conan_voice_info.bytes: what a voice uses.  conan_voices_import makes ids[i] the voice of row i; it succeeds
 *   for a bank of another capacity or another max_ref_frames that still holds the voice.  Every record is checked before anything
 *   changes: not a record / corrupted: CONAN_ERR_INVALID; another layout id (a hash over hidden_size, heads, num_mels, nvq and the row
 *   structure) or a voice that does not fit the bank, or the row stride: CONAN_ERR_SHAPE. */
typedef struct conan_voices conan_voices;
#define CONAN_VOICE_META_BYTES 256
typedef struct conan_voice_meta { unsigned char opaque[CONAN_VOICE_META_BYTES]; } conan_voice_meta;
typedef struct conan_voice_info {
  int32_t enrolled, ref_frames, tokens, reserved;
  int64_t bytes;                           /* of an exported row */
  uint64_t layout_id;
} conan_voice_info;
int conan_voices_create(conan_ctx* ctx, int capacity, int max_ref_frames, conan_voices** out);
int conan_voices_destroy(conan_voices* v);
int conan_voices_enroll(conan_voices* v, conan_streams* via, const int32_t* ids, int n, const float* ref_mel_dev, const int32_t* ref_len,
                        int max_len, void* stream);
int conan_voices_remove(conan_voices* v, const int32_t* ids, int n);
int conan_voices_info(const conan_voices* v, int id, conan_voice_info* out);
int conan_streams_set_voice(conan_streams* s, const int32_t* slots, int n, const conan_voices* v, const int32_t* voice_ids, void* stream);
int conan_streams_set_voice_mix(conan_streams* s, const int32_t* slots, int n, const conan_voices* v, const int32_t* voice_ids,
                                const float* weights, int k, void* stream);
int conan_streams_voice(const conan_streams* s, int slot, int32_t* voice_id);
int64_t conan_voices_blob_bytes(const conan_voices* v);
int conan_voices_export(conan_voices* v, const int32_t* ids, int n, void* blob_dev, int64_t blob_ld_bytes, conan_voice_meta* meta_host,
                        void* stream);
int conan_voices_import(conan_voices* v, const int32_t* ids, int n, const void* blob_dev, int64_t blob_ld_bytes,
                        const conan_voice_meta* meta_host, void* stream);
/* Host only, no handle: what a caller may read out of a record (enrolled = 1).  CONAN_ERR_INVALID for what is not one. */
int conan_voice_meta_info(const conan_voice_meta* meta, conan_voice_info* out);

/* Input noise suppression (added within ABI 9: a caller detects it by the symbol conan_streams_set_denoise; no existing struct or call
 * changes).  A causal spectral gate on the log-mel frames of a wav-in slot: the model only ever sees those frames, so the suppressor
 * keeps no STFT of its own, no phase, no overlap-add and no look-ahead.  It rewrites the frames conan_step_wav's front-end has just
 * written into the slot's mel ring, in place, and the chunk the step consumes; the audio ring - and with it the f0 tracker, the
 * activity detector, the dry path and the leveller - and the decoder's mel_out and the vocoder are untouched.
 * The law (tests/denoise_ref.py restates it in numpy with int64).  Levels are integers in Q10 of the mel's log unit: 1024 steps per
 * unit, that is 20 dB per unit for log10 and 8.686 dB per unit for natural_log (conan_amd._lib.denoise_cfg converts once; no libm
 * function is part of the law).  A row has nm = num_mels bins, 1 .. 256, and its frames are taken in order.  State per bin b: the
 * noise floor N[b] and the attenuation A[b]; per row the count `frames`.  For frame f with values v[b]:
 *   Level.   L[b] = (int32) rint(fmin(fmax((double)v[b], -1024.0), 1024.0) * 1024.0), ties to even; through IEEE fmax a NaN reads as
 *            -1024.
 *   Start.   If this is the row's first frame since a restart and no seed was given: N[b] = max(L[b], floor_min), A[b] = 0, before
 *            anything else.
 *   SNR.     With the floor as it was before this frame: snr = L - (N + bias), d = max(knee - snr, 0),
 *            a = min((d * slope) >> 8, depth), the product in int64.
 *   Across bins (smooth = 1).  a2[b] = (a[max(b-1, 0)] + 2 a[b] + a[min(b+1, nm-1)] + 2) >> 2; otherwise a2 = a.
 *   Across time.  A' = a2 > A ? min(A + close_step, a2) : max(A - open_step, a2).
 *   Output.  A' == 0: y = v, the bin keeps its bits whatever they are.  Otherwise
 *            y = fmaxf((float)((double)(L - A') * 0.0009765625), out_floor): one rounding.
 *   Floor.   L < N: N' = N - ((N - L + (1 << fall_shift) - 1) >> fall_shift); otherwise N' = min(L, N + rise); then
 *            N' = max(N', floor_min).
 *   frames += 1.
 * Every operation is an integer one or a single correctly rounded IEEE operation, so the streamed form, the whole-signal form and
 * the numpy reference agree bit for bit however the frames are cut into calls.
 * Defaults (conan_amd._lib.denoise_cfg): bias 3 dB, knee 6 dB, slope 512 (2 dB of attenuation per dB under the knee), depth 18 dB,
 * close 4.5 dB per frame, open = depth (a bin opens within the frame that needs it), rise 0.05 dB per frame, fall_shift 1, floor_min
 * -100 dB, smooth 1, out_floor = max(mel vmin, log(eps)) in f32.  They are choices, not measurements: this repository holds synthetic
 * weights and no speech corpus, so whether they improve real conversions cannot be measured with what it holds. */
typedef struct conan_denoise_cfg {
  int32_t enabled;     /* 0: off (other fields ignored) | 1 */
  int32_t reseed;      /* 0 | 1: the state restarts (setter only) */
  int32_t bias;        /* 0 .. 2^20: the floor is read this much higher */
  int32_t knee;        /* 0 .. 2^20: SNR under which the gate begins to close */
  int32_t slope;       /* Q8, 0 .. 2^16: attenuation per step under the knee */
  int32_t depth;       /* 1 .. 2^20: the largest attenuation */
  int32_t close_step;  /* 1 .. 2^20: per frame */
  int32_t open_step;   /* 1 .. 2^20: per frame */
  int32_t rise;        /* 0 .. 2^20: the floor's rise per frame */
  int32_t fall_shift;  /* 0 .. 8: the floor falls by ceil((N - L) / 2^fall_shift) */
  int32_t floor_min;   /* -2^20 .. 2^20 */
  int32_t smooth;      /* 0 | 1: the 1-2-1 average across bins */
  float out_floor;     /* finite: the smallest value an attenuated bin takes */
  int32_t reserved[3]; /* must be 0 */
} conan_denoise_cfg; /* 64 bytes */
/* Published, so a host can read the noise spectrum.  A record whose `bins` is not the row's num_mels (the zero record among them) is
 * the state before the first frame: the next frame applies Start.  Entries past `bins` are 0.  A seed is a record this library wrote
 * (the zero record among them): of any other, floor[] is read clamped to -2^20 .. 2^20 and att[] to 0 .. 2^20, the ranges the law
 * keeps them in, and `frames` counts modulo 2^64. */
typedef struct conan_denoise_state {
  int64_t frames;
  int32_t bins, reserved;
  int32_t floor[256], att[256];
} conan_denoise_state; /* 2064 bytes */
/* The law on whole rows, and the bit-exact yardstick of the streaming form: row i (n rows in 1 .. 65535) holds frames[i] (host,
 * >= 0) frames of num_mels (1 .. 256) floats at mel_dev + i * ld floats (ld >= frames[i] * num_mels); out_dev has the same shape and
 * may equal mel_dev; an out_dev that overlaps mel_dev in any other way is undefined (rows of one buffer cannot overlap: ld holds
 * every row).  cfg->enabled must be 1; cfg->reseed is ignored.  seed_dev (may be null): conan_denoise_state[n], the state row i
 * starts from; without it every row starts before its first frame.  state_out_dev (may be null): conan_denoise_state[n], the state
 * behind each row's last frame; it may equal seed_dev, and any other overlap of the two is undefined.  ONE launch
 * (cnk::denoise_signal_kernel, one workgroup per row) on `stream`; the row table goes through the context's workspace, which
 * conan_wav2mel, conan_loud_norm and conan_activity share: calls on one context are ordered by the caller.  A caller with mel-in
 * slots streams this call through seed and state. */
int conan_mel_denoise(conan_ctx* ctx, const conan_denoise_cfg* cfg, const float* mel_dev, int n, const int32_t* frames, int64_t ld, int num_mels,
                      const conan_denoise_state* seed_dev, float* out_dev, conan_denoise_state* state_out_dev, void* stream);
/* Sets (cfg->enabled = 1) or removes (0) the suppressor for `slots`.  Every argument is checked before anything changes
 * (CONAN_ERR_INVALID: a field outside its range, a non-zero reserved word, a seed that is misaligned or whose rows are too close;
 * CONAN_ERR_UNSUPPORTED: a front-end of more than 256 mel bins), a stream-set without the streaming front-end is CONAN_ERR_STATE, and
 * pending pipelined work is joined; it may be called at any time, also mid-utterance, and the setting persists across resets.  The
 * state restarts at the slot's next frame after a reset that includes CONAN_MODEL_FRONTEND, after a setter call with reseed = 1 and
 * when a slot that was off is enabled; a setter call with reseed = 0 on an enabled slot changes the parameters from the next frame
 * and keeps the state.  seed_dev (may be null): row i at seed_dev + i * seed_ld bytes is a conan_denoise_state, and is what the state
 * of slots[i] restarts from (on `stream`) in a call that restarts it; in a call that keeps the state it is not read.
 * Launches: one more per wav-in call in which a suppressing slot completes a frame or emits (cnk::denoise_stream_kernel, directly
 * behind the mel front-end's), none otherwise; conan_step_wav_chunk returns the suppressed chunk.
 * Memory: the first enabling call allocates conan_denoise_state_bytes() per slot and 4 row tables; conan_streams_state_bytes counts
 * them from then on.  A stream-set that never calls the setter allocates nothing and runs exactly the launches it ran before.
 * Snapshots: the mel ring, which holds suppressed frames, travels as before; a snapshot carries neither the setting nor the state, and
 * conan_streams_layout_id and conan_streams_snapshot_bytes do not change.  The hand-over: conan_streams_denoise_state, export, import,
 * then this setter with the record as seed_dev and reseed = 1. */
int conan_streams_set_denoise(conan_streams* s, const int32_t* slots, int n, const conan_denoise_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream);
/* Host only: the suppressor's cfg of `slot` as set (zeros for a slot without one; reseed reads 0). */
int conan_streams_denoise(const conan_streams* s, int slot, conan_denoise_cfg* cfg_out);
/* sizeof(conan_denoise_state). */
int64_t conan_denoise_state_bytes(void);
/* The states of `slots` -> row i at rows_dev + i * ld bytes (8-byte aligned, ld a multiple of 8 and at least the record's bytes), on
 * `stream` behind a join of pipelined work.  A slot about to restart reports the zero record; a slot without the feature is
 * CONAN_ERR_STATE. */
int conan_streams_denoise_state(conan_streams* s, const int32_t* slots, int n, void* rows_dev, int64_t ld, void* stream);

/* Output watermark (added within ABI 9: a caller detects it by the symbol conan_streams_set_watermark; no existing struct or call
 * changes).  A keyed mark in the audio a slot emits, which says "synthesised, and by whom": a +-1 chip sequence under a causal peak
 * envelope, added on the GPU at the model rate (16 kHz) in f32 behind the slot's last in-place stage (the comfort fill) and in front of
 * the output resampler and the encoders, and a detector that finds it again in 16-bit audio of any CONAN_SAMPLE_* format.
 * tests/watermark_ref.py restates both laws in numpy with Python integers.
 * Constants.  CHIP = 4 samples per chip; BLK = 2048 samples per block (512 chips, 128 ms); SUB = 64 samples per envelope sub-block;
 *   W = 24 blocks per word (3.07 s).  The word is the marker 1,0,1,1,0,1,0,1 followed by the 16 bits of id, MSB first; bits map to +-1.
 *   chip(key, m), m in 0 .. 511, is +1 if bit 63 of the comfort noise's hash of (key, m) is set, else -1: z = key + (m + 1) *
 *   0x9E3779B97F4A7C15; z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31 (mod 2^64).
 *   The sign of utterance sample j is s(j) = chip(key, (j mod BLK) / CHIP) * word[(j / BLK) mod W].
 * Embed.  State {pos, env}, starting at {0, 0}.  For each sub-block b of a row, in order: p = max |y_j| over the sub-block;
 *   env = fmaxf(p, env * 0.875f) (one f32 product); a = fmaxf(env * gain, floor) (one f32 product); y'_j = y_j + s(pos + j) * a (one
 *   f32 add; the sign is exact).  After the row pos += samples.  A row's last sub-block may be short in the whole-signal form only;
 *   streaming rows are whole hops (a multiple of SUB), so any cut into steps gives the same bits.  There is no clamp: the encoders
 *   clamp, and f32 callers see the sum.  Every operation is a single correctly rounded one in a fixed order.
 *   Defaults (conan_amd._lib.watermark_cfg): gain 0.1, that is -20 dB under the causal peak envelope; floor 0: digital silence stays
 *   digital silence.  They are choices, not measurements: nobody has listened to the result, and this repository holds synthetic
 *   weights and no speech corpus.
 * Detect.  Integers on the 16-bit view q of a 16 kHz row of n samples: q = clamp(rint(x * 32768), -32768, 32767) (ties to even) for
 *   f32, the decoded code otherwise.  d_j = 16 q_j - 15 q_{j-1} (q_{-1} = 0); u_j = d_j + d_{j+1} + d_{j+2} + d_{j+3};
 *   K = max(0, n / BLK - 1) blocks; R[k][o] = sum over m < 512 of chip(key, m) * u[k * BLK + o + 4 m] for o in 0 .. BLK-1.
 *   |u| <= 4 * 31 * 32768, so |R| <= 31 * 32768 * 4 * 512 = 2080374784 < 2^31: int32 accumulation is exact.  The block weight is
 *   n_k = bit_length(sum of |d_j| over j in [k * BLK, (k + 2) * BLK)), at least 1; Rn = sign(R) * ((|R| << 12) >> n_k);
 *   S[o] = sum over k of |Rn[k][o]|; o* = argmax S, the lowest index on ties; soft[k] = Rn[k][o*].
 * Decide (host).  z = (S[o*] - mean S) / std S in f64 (population std; sums sequential in index order; 0 where std is 0).  For each
 *   rotation r in 0 .. W-1 soft is folded into acc[(k + r) mod W] and the marker scored, sum of marker_i * acc[i]; the highest score
 *   wins, the lowest r on ties; id is read from the signs of acc[8 .. 23] (> 0: 1).  present = z >= threshold.
 *   CONAN_WATERMARK_THRESHOLD is about midway between the two groups DESIGN.md 4.23 measured with the reference: marked rows of 4 s
 *   and 8 s through s16, mu-law at 16 kHz and mu-law at 8 kHz gave z = 17.6 .. 22.0, unmarked rows and rows marked with another key
 *   3.0 .. 5.7.
 * Out of scope: clock drift, time-scale changes, and marks cropped to under two blocks.  Audio at another rate comes back to 16 kHz
 * through conan_resample first; the offset search absorbs the filter's delay. */
#define CONAN_WATERMARK_THRESHOLD 11.5
typedef struct conan_watermark_cfg {
  int32_t enabled;     /* 0: off (other fields ignored) | 1 */
  int32_t reseed;      /* 0 | 1: the state restarts (setter only) */
  uint64_t key;
  int32_t id;          /* 0 .. 65535 */
  float gain;          /* finite, 0 .. 1 */
  float floor;         /* finite, 0 .. 1 */
  int32_t reserved[9]; /* must be 0 */
} conan_watermark_cfg; /* 64 bytes */
typedef struct conan_watermark_state {
  int64_t pos;         /* utterance samples marked so far, >= 0 */
  float env;           /* the envelope behind the last sub-block */
  int32_t reserved;
} conan_watermark_state; /* 16 bytes */
typedef struct conan_watermark_hit {
  int32_t offset, blocks;   /* o*, K */
  int64_t peak;             /* S[o*] */
} conan_watermark_hit; /* 16 bytes */
typedef struct conan_watermark_result {
  int32_t present, id, offset, rotation, blocks, reserved;
  int64_t marker_score;
  double z;
} conan_watermark_result; /* 40 bytes */
/* The embedder on whole signals, and the bit-exact yardstick of the streaming form: row i (n rows in 1 .. 65535) holds samples[i]
 * (host, 0 .. 2^31 - 1) floats at x_dev + i * ld floats (ld >= every samples[i]); out_dev has the same shape and may equal x_dev.
 * cfg->enabled must be 1; cfg->reseed is ignored.  seed_dev (may be null): conan_watermark_state[n], the state row i starts from
 * (pos >= 0); without it every row starts at {0, 0}.  state_out_dev (may be null): the state behind each row; it may equal seed_dev.
 * Both 8-byte aligned.  ONE launch (cnk::watermark_embed_kernel, one workgroup per row) on `stream`; the row table goes through the
 * context's workspace, which conan_wav2mel, conan_loud_norm and conan_activity share: calls on one context are ordered by the caller. */
int conan_watermark_embed(conan_ctx* ctx, const conan_watermark_cfg* cfg, const float* x_dev, int n, const int64_t* samples, int64_t ld,
                          const conan_watermark_state* seed_dev, float* out_dev, conan_watermark_state* state_out_dev, void* stream);
/* The detector's device half: row i (n rows in 1 .. 4096) holds samples[i] (host, 0 .. 2^26) samples of `format` at x_dev + i * ld * 4
 * bytes (4-byte aligned; ld dwords hold every row).  score_dev: int64 [n][2048], S; soft_dev: int64 rows soft_ld apart (soft_ld >=
 * the largest K of the call), soft[k] for k < K and 0 from there to the call's largest K; hit_dev: conan_watermark_hit[n]; all three
 * 8-byte aligned.  A row with K = 0 reports zeros.  Two launches on `stream` (cnk::watermark_corr_kernel, none when every K is 0, and
 * cnk::watermark_peak_kernel); Rn goes through the context's workspace as int32 (|Rn| < 2^12, because |R| is at most the window's sum
 * of |d|): 8 KiB per row and block, at most 2 GiB per call (CONAN_ERR_INVALID beyond: split the call); calls on one context are
 * ordered by the caller, as above. */
int conan_watermark_detect(conan_ctx* ctx, uint64_t key, int format, const void* x_dev, int64_t ld, int n, const int64_t* samples,
                           int64_t* score_dev, int64_t* soft_dev, int64_t soft_ld, conan_watermark_hit* hit_dev, void* stream);
/* Host only: the decision from one row's S [2048], soft [blocks] and record.  threshold: CONAN_WATERMARK_THRESHOLD unless the caller
 * has measured its own.  blocks = 0 reports present = 0, blocks = 0 and reads nothing. */
int conan_watermark_decide(const int64_t* score, const int64_t* soft, const conan_watermark_hit* hit, double threshold, conan_watermark_result* out);
/* Sets (cfg->enabled = 1) or removes (0) the mark for `slots`.  Every argument is checked before anything changes (CONAN_ERR_INVALID:
 * a field outside its range, a non-zero reserved word, a seed that is misaligned or whose rows are too close; CONAN_ERR_UNSUPPORTED:
 * the whole-prefix vocoder of upsample 'nn', whose steps are not update intervals - as for the output leveller; CONAN_ERR_STATE: a
 * context without a HiFi-GAN model), and pending pipelined work is joined; it may be called at any time, also mid-utterance, and the
 * setting persists across resets.
 * A marked slot costs one more launch (cnk::watermark_embed_kernel) per vocoder step that carries one, in every step entry point,
 * mel-in ones included: behind the comfort fill and in front of the output resampler.  The output leveller's meter reads its stage as
 * before: unmarked audio.  The state restarts when a slot that was off is enabled, on reseed = 1 (from seed_dev's row where one is
 * given: row i at seed_dev + i * seed_ld bytes, on `stream`) and on a reset that includes CONAN_MODEL_HIFIGAN (from {0, 0}).  A call
 * with reseed = 0 on an enabled slot changes key, id, gain and floor from the next step and keeps pos and env; its seed row is not read.
 * Memory: the first enabling call allocates the states and 8 row tables; conan_streams_state_bytes counts them from then on.  A
 * stream-set that never calls the setter allocates nothing and runs exactly the launches it ran before; a slot that does not ask
 * keeps its bits.  Snapshots carry neither the setting nor the state, and conan_streams_layout_id and conan_streams_snapshot_bytes do
 * not change.  The hand-over: conan_streams_watermark_state, export, import, then this setter with the record as seed_dev and
 * reseed = 1. */
int conan_streams_set_watermark(conan_streams* s, const int32_t* slots, int n, const conan_watermark_cfg* cfg, const void* seed_dev, int64_t seed_ld,
                                void* stream);
/* Host only: the mark's cfg of `slot` as set (zeros for a slot without one; reseed reads 0). */
int conan_streams_watermark(const conan_streams* s, int slot, conan_watermark_cfg* cfg_out);
/* sizeof(conan_watermark_state). */
int64_t conan_watermark_state_bytes(void);
/* The states of `slots` -> row i at rows_dev + i * ld bytes (8-byte aligned, ld a multiple of 8 and at least the record's bytes), on
 * `stream` behind a join of pipelined work.  A slot about to restart reports the zero record; a slot without the feature is
 * CONAN_ERR_STATE. */
int conan_streams_watermark_state(conan_streams* s, const int32_t* slots, int n, void* rows_dev, int64_t ld, void* stream);

/* Signalling tones (added within ABI 9: a caller detects it by the symbol conan_streams_set_tones; no existing struct or call changes).
 * A DTMF key press in a slot's source goes through mel, Emformer, decoder and vocoder like any other sound and leaves as something no
 * DTMF receiver accepts.  A slot with this feature detects the sixteen tone pairs in its own input (mode 1: the host learns the keys
 * and can send them as RFC 4733 events) and - mode 2 - replaces its output, while a digit is confirmed, by a tone pair synthesised
 * from a table: what a media gateway does when it plays out such an event.  Nothing of the source audio reaches the output through
 * this feature.  The law (tests/tone_ref.py restates it in numpy with Python integers) is integer sums - associative, so no order of
 * lanes, waves or tiles is part of it - and for the regeneration single correctly rounded IEEE operations; nothing has a tolerance.
 * With M the model's sample rate and hop = M / 50 (20 ms frames, as conan_activity requires):
 *   Table.  W[m] = rint(2^14 * cos(2 pi m / M)), m = 0 .. M - 1, int16, built once on the host in f64 (conan_tone_table exports it).
 *     M must be a multiple of 4 (a quarter period is M / 4 entries) and hop in 2 .. CONAN_TONE_HOP_MAX = 512, else
 *     CONAN_ERR_UNSUPPORTED: the int64 bounds below hold up to hop = 1024, and the table (2 M bytes) with a workgroup's tile staging
 *     stays inside 64 KB of LDS up to hop = 512, which is the range accepted.  For M = 16000 no 2^14 cos value lies closer than 1e-5
 *     to a half-integer, so every correctly rounded cos gives the same table.
 *   Frame.  Tone frame f of a slot's utterance is source samples [f hop, (f + 1) hop) at the model rate: the audio the activity
 *     detector and the dry path read, behind decoding, the input resampler, concealment and the leveller, in the slot's audio ring;
 *     zero at and beyond the samples received.  q[j] = clamp(rint(x[j] * 32768), -32768, 32767) in f32, ties to even: the library's
 *     s16 value of the sample.
 *   Sums, over the absolute utterance index j of the frame's samples (frames are phase-continuous):  E = sum q^2, and for each of
 *     F = 697, 770, 852, 941 (rows 0 .. 3) and 1209, 1336, 1477, 1633 Hz (columns 0 .. 3):
 *       C = sum q[j] W[(F j) mod M],  S = sum q[j] W[(F j - M / 4) mod M],  c = C >> 16, s = S >> 16 (arithmetic),  P = c^2 + s^2,
 *     all int64.  |C| <= hop 2^29, |c| <= hop 2^13, P <= hop^2 2^27 and E <= hop 2^30 (at hop = 320: |c| <= 2.7e6, P <= 1.5e13).
 *   Frame digit.  r = argmax of the four row P, c = argmax of the four column P, the lowest index on a tie.  d = 4 r + c if all of
 *       P_r >= thr and P_c >= thr;
 *       P_c 256 <= P_r twist_fwd_q8 and P_r 256 <= P_c twist_rev_q8      (twist);
 *       P_o sel <= P_peak for the three others o of each group           (selectivity);
 *       (P_r + P_c) 32 256 >= share_q8 hop E                             (the pair's share of the frame's energy: for a pure pair
 *                                                                         (P_r + P_c) 2^32 = 2^28 (hop / 2) E, so share_q8 / 256 is
 *                                                                         the share in 0 .. 1)
 *     hold, else d = -1.  With twist_*_q8 and sel <= 65535 and share_q8 <= 256 the largest product is P 65535 < hop^2 2^43 <= 2^63 for
 *     hop <= 1024.  There is no second-harmonic test: 2 * 770 Hz sits 63 Hz from 1477 Hz, which a 20 ms rectangular frame cannot
 *     separate.  Keys: d = 0 .. 15 is "123A456B789C*0#D"[d].
 *   Debounce.  State: cand, run, cur, miss, held, sound, level, events, frames.  Per frame, in this order:
 *       run.      d >= 0 and d == cand: run += 1 (it stops at 2^30); d >= 0 otherwise: cand = d, run = 1; d < 0: cand = -1, run = 0.
 *       holding.  cur >= 0: held += 1 (it stops at 2^30); miss = d == cur ? 0 : miss + 1 (misses in a row); if miss >= off_frames and
 *                 held >= min_frames the digit ends: cur = -1, miss = 0, held = 0.
 *       confirm.  cur < 0 and run >= on_frames: cur = cand, events += 1, held = 0, miss = 0 (a run that was waiting while another
 *                 digit held takes over in the frame that digit ends).
 *       digit[f] = cur.   level += clamp((cur >= 0 ? 2^20 : 0) - level, -step, step).
 *       sound.    cur >= 0: sound = cur; otherwise sound = -1 once level == 0.  sound[f] = sound, level[f] = level, frames += 1.
 *     sound[f] = -1 exactly where cur < 0 and level[f] == 0.
 *   Regeneration (mode 2).  Output sample j of the utterance lies in frame f = j / hop at k = j - f hop.  With level[f - 1] and
 *     level[f] the levels before and after frame f: l = level[f - 1] (hop - 1 - k) + level[f] (k + 1), the gate's interpolation.  The
 *     frame's pair is g = sound[f] >= 0 ? sound[f] : sound[f - 1] (a frame that ends at level 0 fades the pair it began with), its
 *     row and column frequencies F_r, F_c.  With y the sample behind every other in-place stage:
 *       syn = (float)(W[(F_r j - M / 4) mod M] + W[(F_c j - M / 4) mod M]) * kf,  kf = gain * 2^-14 (exact scaling: one f32 product);
 *       g_t = (float)((double)l / (double)(hop << 20)),  g_y = (float)((double)((hop << 20) - l) / (double)(hop << 20));
 *       out = l == 0 ? y : fma(syn, g_t, y * g_y)      (one f32 product, one fused multiply-add).
 *     A frame with both levels 0 keeps y's bits; at l = hop << 20 the output is syn in value, whatever finite y is.
 *   Restart.  The state restarts from cfg.seed at the slot's first emitted chunk after a reset that includes CONAN_MODEL_FRONTEND,
 *     after a setter call with reseed = 1 and when a slot that was off is enabled.  A setter call with reseed = 0 on an enabled slot
 *     replaces mode and parameters and keeps the state.  In a stream j is the utterance's sample index (the front-end's frame
 *     position), whatever the state's `frames` says; a whole-signal row starts at frame seed.frames.
 * The defaults of the Python layer (_lib.tone_cfg: -40 dBFS per tone, twist 4 dB / 8 dB, sel 8, share 1/2, 2 frames on, 2 off, 3
 * held, an unramped level, gain 0.125) are choices: talk-off against real speech has not been measured by anyone. */
#define CONAN_TONE_HOP_MAX 512
#define CONAN_TONE_FULL (1 << 20)
typedef struct conan_tone_state {
  int32_t cand, run;       /* the current run of equal frame digits: the digit (-1: none) and its length */
  int32_t cur;             /* the confirmed digit, -1: none */
  int32_t miss, held;      /* while a digit holds: frames in a row that were not it; frames since it was confirmed */
  int32_t sound;           /* the pair the regeneration sounds, -1: none */
  int32_t level;           /* 0 .. 2^20 */
  int32_t reserved;
  int64_t events;          /* digits confirmed */
  int64_t frames;          /* frames seen; a whole-signal row's first frame index */
} conan_tone_state;        /* 48 bytes */
typedef struct conan_tone_cfg {
  int32_t mode;            /* 0: off (other fields ignored) | 1: detect | 2: detect and regenerate */
  int32_t reseed;          /* 0 | 1: the state restarts from the seed */
  int64_t thr;             /* 0 .. 2^62: the least P of a tone */
  int32_t twist_fwd_q8;    /* 256 .. 65535: the column tone may exceed the row tone by this ratio of powers, in 1/256 */
  int32_t twist_rev_q8;    /* 256 .. 65535: the row tone over the column tone */
  int32_t sel;             /* 1 .. 65535 */
  int32_t share_q8;        /* 0 .. 256 */
  int32_t on_frames;       /* 1 .. 2^20 */
  int32_t off_frames;      /* 1 .. 2^20 */
  int32_t min_frames;      /* 0 .. 2^20 */
  int32_t step;            /* 1 .. 2^20: levels per 20 ms frame */
  float gain;              /* 0 .. 0.5: each tone's amplitude (the pair's peak is twice that) */
  int32_t reserved;
  conan_tone_state seed;   /* cand, cur, sound in -1 .. 15; run, miss, held in 0 .. 2^30; level in 0 .. 2^20; events, frames in 0 .. 2^40 */
} conan_tone_cfg;          /* 104 bytes */
/* Host only: the table of `sample_rate` -> table_out[sample_rate] (CONAN_ERR_UNSUPPORTED: a rate that is not 50 * hop with hop in
 * 2 .. 512, or not a multiple of 4). */
int conan_tone_table(int sample_rate, int16_t* table_out);
/* The detector on whole signals, and the bit-exact yardstick of the streaming one: row i of wav_dev (n rows in 1 .. 65535, row stride
 * ld floats) holds samples[i] samples (host array; 0 .. ld) at 50 * hop Hz and has ceil(samples[i] / hop) frames, the last one zero
 * beyond the samples -> digit_dev[i][f], sound_dev[i][f], level_dev[i][f] (int32, row stride out_ld >= the longest row's frames;
 * nothing is written behind a row's frames), the state after the row -> state_out_dev[i] (may be null) and frames_out[i] (host, may
 * be null).  Row i starts from seed_dev[i] (device; null: from cfg->seed), at frame index seed.frames: a signal cut into calls at
 * frame boundaries and chained through the state gives the whole signal's rows.  cfg->mode must be 1 or 2.  One launch
 * (cnk::tone_kernel) on `stream`. */
int conan_tones(conan_ctx* ctx, int hop, const conan_tone_cfg* cfg, const float* wav_dev, int64_t ld, int n, const int64_t* samples,
                const conan_tone_state* seed_dev, int32_t* digit_dev, int32_t* sound_dev, int32_t* level_dev, int64_t out_ld,
                conan_tone_state* state_out_dev, int64_t* frames_out, void* stream);
/* The regeneration on whole signals, and the bit-exact yardstick of the streaming one: row i of wav_dev (n rows in 1 .. 65535 of
 * `samples` samples, row stride ld) with sound_dev[i][f] and level_dev[i][f] after frame f (int32, -1 .. 15 and 0 .. 2^20, row stride
 * lvl_ld >= ceil(samples / hop)) and start_level / start_sound as the values before frame 0 -> out_dev (row stride out_ld; may equal
 * wav_dev with out_ld = ld).  Sample s of row i is utterance sample pos0[i] + s (host array, each in 0 .. 2^62; null: 0); frames
 * count from the row's first sample.  Of cfg only gain is read.  A last frame that the samples cover only partly is filled over the
 * part they cover.  One launch (cnk::tone_fill_kernel) on `stream`. */
int conan_tone_fill(conan_ctx* ctx, int hop, const conan_tone_cfg* cfg, const float* wav_dev, int64_t ld, int n, int64_t samples, const int64_t* pos0,
                    const int32_t* sound_dev, const int32_t* level_dev, int64_t lvl_ld, int32_t start_level, int32_t start_sound, float* out_dev,
                    int64_t out_ld, void* stream);
/* Sets (cfg->mode = 1 | 2) or removes (0) the feature for `slots`.  Every argument is checked before anything changes
 * (CONAN_ERR_INVALID: a field outside its range; CONAN_ERR_UNSUPPORTED: the model's hop or rate outside the table's range), a
 * stream-set without the streaming front-end is CONAN_ERR_STATE, and pending pipelined work is joined; it may be called at any time,
 * also mid-utterance.  The change takes effect from the next emitted chunk and persists across resets.
 * What a slot with the feature does.  Every conan_step_wav[_async] / conan_step_wav_ragged[_ld][_async] call that emits a chunk for
 * it runs ONE more launch (cnk::tone_kernel, behind the front-end launch, beside the activity detector's) over the chunk's frames, read
 * from the slot's audio ring.  The ring requirement is the dry path's: a chunk whose samples had left the ring would make the call
 * CONAN_ERR_UNSUPPORTED before anything changes, but no call reaches that today - a call that is not final takes at most
 * segment * hop samples, so an emitted chunk begins at most (segment + right context - 1) * hop + fft_size / 2 + segment * hop
 * samples behind the samples received, 3840 at the largest front-end accepted, and the ring holds 4096.  The check guards a later
 * change of either figure and is not a condition a caller has to handle.  In mode 2 the chunk's vocoder step regenerates in place on the rows conv_post wrote, behind the gate, the mix, the comfort fill and the
 * watermark, as the last in-place stage in front of the output resampler and the format encoder - the pair leaves clean at the slot's
 * own rate and format, flush included, and the mark's state advances as it did before: ONE more launch (cnk::tone_fill_kernel) per
 * vocoder step in which a mode-2 row takes part; rows of other slots and frames with level 0 at both ends keep their bits.  The
 * mel-in steps (conan_step[_async]) and conan_hifigan_step* take no waveform: they neither detect nor fill.
 * Memory: the first enabling call allocates 48 bytes of state per slot, 8 staging sets of 3 * segment + 2 int32 per slot and 8 row
 * tables; conan_streams_state_bytes counts them from then on (the table belongs to the context: one copy per rate, built on first
 * use).  A stream-set that never calls the setter allocates nothing and runs exactly the launches it ran before.
 * Snapshots carry neither the setting nor the state (the 256-byte host record is full); conan_streams_layout_id and
 * conan_streams_snapshot_bytes do not change.  The hand-over: conan_streams_tone_state, export, import, then this setter with
 * seed = the queried state and reseed = 1. */
int conan_streams_set_tones(conan_streams* s, const int32_t* slots, int n, const conan_tone_cfg* cfg, void* stream);
/* Host only: the tone cfg of `slot` as set, reseed = 0 (mode = 0 and zeros for a slot without one). */
int conan_streams_tones(const conan_streams* s, int slot, conan_tone_cfg* cfg_out);
/* The states of `slots` -> state_dev[n], in the order of `stream` behind a join of pipelined work; a slot whose state is about to
 * restart reports its seed.  A slot without the feature is CONAN_ERR_STATE. */
int conan_streams_tone_state(conan_streams* s, const int32_t* slots, int n, conan_tone_state* state_dev, void* stream);
/* The frame rows the last wav-in call produced, in call order (joins first): digit_dev[n][seg], sound_dev[n][seg] and
 * level_dev[n][seg], int32.  Rows without the feature, rows that emitted nothing and positions behind the emitted frames read zero
 * (a digit row of a slot with the feature reads -1 where no digit holds).  CONAN_ERR_STATE before any wav-in call. */
int conan_step_wav_tones(conan_streams* s, int32_t* digit_dev, int32_t* sound_dev, int32_t* level_dev, void* stream);

/* Equaliser (added within ABI 9: a caller detects it by the symbol conan_eq; no existing struct or call changes).  A cascade of up to
 * CONAN_EQ_MAX_SECTIONS = 4 biquad sections on audio that exists only on the device: a high-pass against DC and rumble, a notch
 * against hum, a tone control, a telephone band - on the source side of a wav-in slot (conan_streams_set_input_eq), on its output
 * (conan_streams_set_output_eq) and on whole signals (conan_eq, the bit-exact yardstick of both).  tests/eq_ref.py restates the law
 * in Python floats (IEEE doubles, never fused), bit for bit.
 *   Coefficients.  A section is five doubles {b0, b1, b2, a1, a2}, normalised by a0, taken as given: how they were designed is not
 *     part of the law.  Each is finite and at most CONAN_EQ_MAX_COEF = 65536 in magnitude (a cookbook section with |gain| <= 60 dB
 *     stays far inside), and each section is stable: |a2| < 1 and |a1| < 1 + a2.
 *   One step.  Transposed direct form II in f64, every product and every sum rounded on its own - no fused multiply-add anywhere:
 *       y = b0 x + s0;   s0' = (b1 x - a1 y) + s1;   s1' = b2 x - a2 y.
 *     Section k + 1 reads section k's f64 output.  The input is the f32 sample widened, a non-finite sample counts as 0 (one bad
 *     sample must not poison a recursive state), and the result is the last section's output rounded once to f32.  There is no
 *     clip: a boost may exceed 1.0.  f64 denormals are kept.
 *   The segment grid.  A row's grid of CONAN_EQ_SEG = 128 samples starts at its origin.  Per section, with c the state at a
 *     segment's start, e the end state of the zero-state run over that segment's true inputs (the section's inputs: the output of
 *     the section in front of it) and M the section's 2x2 transition matrix of 128 zero inputs - built on the host in double by
 *     applying the step to the unit states (1, 0) and (0, 1), which give M's columns - the state at the next segment's start is
 *       c0' = (M00 c0 + M01 c1) + e0,   c1' = (M10 c0 + M11 c1) + e1       (each product and sum rounded on its own).
 *     Every output sample comes from the direct recursion from its segment's start state; the state at the origin is zero.
 *   The pending tail.  An incomplete last segment is emitted from its start state and its inputs (behind the non-finite rule) stay
 *     in the state's tail; when more samples arrive the segment is run again from the same start state and only the new samples
 *     are emitted.  So the output never depends on how a stream was cut into calls, down to cuts of one sample.
 * The state record holds the origin, the position, the per-section carries (the start state of the segment that holds the position;
 * zeros behind the cfg's last section) and the tail ((pos - origin) mod 128 entries, zeros behind them). */
#define CONAN_EQ_MAX_SECTIONS 4
#define CONAN_EQ_SEG 128
#define CONAN_EQ_MAX_COEF 65536.0
typedef struct conan_eq_cfg {
  int32_t enabled;         /* 0: off (other fields ignored) | 1 */
  int32_t sections;        /* 1 .. CONAN_EQ_MAX_SECTIONS */
  int64_t origin;          /* the grid's first sample; with a seed: the origin its record reports.  0 <= origin <= pos <= 2^62 */
  int64_t pos;             /* the position of the first sample filtered: equal to origin without a seed, the seed record's pos with one */
  double coef[CONAN_EQ_MAX_SECTIONS][5];   /* {b0, b1, b2, a1, a2} per section; zeros behind the last one */
  int32_t reserved[4];     /* must be 0 */
} conan_eq_cfg;            /* 200 bytes */
typedef struct conan_eq_state {
  int64_t origin, pos;
  double carry[CONAN_EQ_MAX_SECTIONS][2];
  float tail[CONAN_EQ_SEG];
} conan_eq_state;          /* 592 bytes */
/* sizeof(conan_eq_state). */
int64_t conan_eq_state_bytes(void);
#define CONAN_EQ_LOWPASS 0
#define CONAN_EQ_HIGHPASS 1
#define CONAN_EQ_BANDPASS 2    /* 0 dB peak gain */
#define CONAN_EQ_NOTCH 3
#define CONAN_EQ_PEAK 4
#define CONAN_EQ_LOWSHELF 5
#define CONAN_EQ_HIGHSHELF 6
#define CONAN_EQ_DCBLOCK 7     /* first order (b2 = a2 = 0): g (1 - z^-1) / (1 - R z^-1), R = exp(-2 pi f0 / rate), g = (1 + R) / 2 */
#define CONAN_EQ_DEEMPHASIS 8  /* first order (b2 = a2 = 0): (1 - p) / (1 - p z^-1), p = exp(-2 pi f0 / rate); 50 us is f0 = 3183.1 Hz */
/* Host only, no handle, no GPU: one section {b0, b1, b2, a1, a2} / a0 -> out[5], by the Audio EQ Cookbook's forms (R. Bristow-Johnson)
 * with w0 = 2 pi f0 / rate, alpha = sin w0 / (2 q) and A = 10^(gain_db / 40); gain_db is read by the peak and the shelves, q by
 * every second-order kind.  CONAN_ERR_INVALID: an unknown kind, a non-finite argument, f0 outside (0, rate / 2), q <= 0 (for every
 * kind), |gain_db| > 60.  The design is not part of the bit-exact law: libm decides its last bits. */
int conan_eq_design(int kind, double rate, double f0, double q, double gain_db, double out[5]);
/* The law on whole signals: row i (n rows in 1 .. 65535) holds samples[i] (host, 0 .. 2^31 - 1) floats at x_dev + i * x_ld and is
 * written to y_dev + i * y_ld (strides in floats, each >= every samples[i]); y_dev may equal x_dev with the same stride: in place.
 * cfg->enabled must be 1.  seed_dev (may be null): conan_eq_state[n], the record row i continues from; cfg->origin and cfg->pos then
 * name the origin and position of every seed row (the caller vouches: the library does not read device memory to plan), so a
 * signal cut anywhere and chained through the state gives the whole signal's bits.  Without a seed every row starts from zero at
 * cfg->origin = cfg->pos.  state_out_dev (may be null; may equal seed_dev): the record behind each row.  Both 8-byte aligned.
 * ONE launch (cnk::eq_signal_kernel, one workgroup of 256 lanes per row, chunks of 1920 samples through cnk::eq_chunk) on `stream`;
 * the row table goes through the context's workspace, which conan_wav2mel, conan_loud_norm and conan_activity share: calls on one
 * context are ordered by the caller. */
int conan_eq(conan_ctx* ctx, const conan_eq_cfg* cfg, const float* x_dev, int64_t x_ld, int n, const int64_t* samples, float* y_dev, int64_t y_ld,
             conan_eq_state* state_out_dev, const conan_eq_state* seed_dev, void* stream);
/* Sets (cfg->enabled = 1) or removes (0) the SOURCE-side equaliser for `slots` (wav-in steps only).  Every argument is checked before
 * anything changes (CONAN_ERR_INVALID: a cfg outside the ranges above, a seed that is misaligned or whose rows are too close, a seeded
 * slot that is not at cfg->pos; CONAN_ERR_UNSUPPORTED: segment * hop above 1920 = (16 - 1) * CONAN_EQ_SEG samples, which is what a
 * call row holds; CONAN_ERR_STATE: a stream-set without the streaming front-end), and pending pipelined work is joined; it may be
 * called at any time, also mid-utterance, and the setting persists across resets.
 * What a slot with the feature does.  Every conan_step_wav[_async] / conan_step_wav_ragged[_ld][_async] call that hands it samples
 * runs ONE more launch (cnk::eq_stream_kernel, one workgroup of 256 lanes per row) between the input resampler's launch and the
 * leveller's, on the model-rate rows the front-end is about to read: the audio ring and everything that reads it - the leveller,
 * the mel frames, the follower, the activity and tone detectors, the comfort tracker, the dry path - see the filtered source.  Behind
 * a resampler launch it works in place on the staged rows; in a call without one it reads the caller's rows and writes the
 * resampler's staging set, and the call's other rows ride along as copy rows (as for the leveller, which then works in place behind
 * it).  The slot's position is the model-rate samples its front-end has received.  Slots of one call may carry different cascades.
 * Enabling a slot that was off starts it from the zero state with the origin at its current position.  Changing an enabled slot is
 * the live tone control and does not click: one small launch (cnk::eq_set_kernel) on `stream` closes the pending tail with the OLD
 * coefficients - the carries advance over it by the direct recursion - the origin moves to the current position, section k keeps
 * its two state words for k below both section counts and new sections start at zero (tests/eq_ref.py, Stream.change).  With
 * seed_dev (row i at seed_dev + i * seed_ld bytes, a record queried from a stream at the same position: the caller vouches) the
 * slot continues that stream: cfg->origin names the record's origin and cfg->pos its position, which must be the slot's.  Without
 * a seed cfg->origin and cfg->pos take no part, but the cfg check still holds them to 0 <= origin <= pos (zeros pass).  The state restarts at the slot's next row after a reset that includes
 * CONAN_MODEL_FRONTEND, with the origin at that row's first sample.  enabled = 0 restores the path without the feature.
 * Memory: the first enabling call allocates 592 bytes of state and 288 bytes of sections per slot and 8 row tables;
 * conan_streams_state_bytes counts them from then on.  A stream-set that never calls the setter allocates nothing and runs exactly
 * the launches it ran before; a slot that does not ask keeps its bits.  Snapshots carry neither the setting nor the state, and
 * conan_streams_layout_id and conan_streams_snapshot_bytes do not change.  The hand-over: conan_streams_input_eq (origin, pos) and
 * conan_streams_input_eq_state, export, import, then this setter with the record as seed_dev. */
int conan_streams_set_input_eq(conan_streams* s, const int32_t* slots, int n, const conan_eq_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream);
/* Host only: the cfg of `slot` as set, with origin and pos as they stand now (zeros for a slot without the feature). */
int conan_streams_input_eq(const conan_streams* s, int slot, conan_eq_cfg* cfg_out);
/* The records of `slots` -> row i at rows_dev + i * ld bytes (8-byte aligned, ld a multiple of 8 and at least conan_eq_state_bytes), on
 * `stream` behind a join of pipelined work.  A slot about to restart reports the zero record at its position; a slot without the
 * feature is CONAN_ERR_STATE. */
int conan_streams_input_eq_state(conan_streams* s, const int32_t* slots, int n, void* rows_dev, int64_t ld, void* stream);
/* The OUTPUT-side equaliser: the same setter, getter and state query for the slot's own vocoder audio.  A slot with the feature
 * costs ONE more launch (cnk::eq_stream_kernel) per vocoder step in which it takes part, in every step entry point, the mel-in ones
 * included: in place on the [n][T] rows conv_post wrote, directly behind it and in front of the output leveller's ramp - so a boost
 * does not defeat the level the leveller promises - and of the gate, the mix, the fill, the mark, the output resampler and the
 * encoders.  The slot's position is the model-rate samples its vocoder has produced since its last reset with CONAN_MODEL_HIFIGAN,
 * which is also what restarts the state.  CONAN_ERR_UNSUPPORTED: the whole-prefix vocoder of upsample 'nn' (as for the output
 * leveller), and a stream-set whose max_frames * hop exceeds 1920; CONAN_ERR_STATE: a context without a HiFi-GAN model.  Memory,
 * snapshots and the hand-over are the source side's. */
int conan_streams_set_output_eq(conan_streams* s, const int32_t* slots, int n, const conan_eq_cfg* cfg, const void* seed_dev, int64_t seed_ld, void* stream);
int conan_streams_output_eq(const conan_streams* s, int slot, conan_eq_cfg* cfg_out);
int conan_streams_output_eq_state(conan_streams* s, const int32_t* slots, int n, void* rows_dev, int64_t ld, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CONAN_HIP_H */
