"""ctypes binding of libconan_hip.so (include/conan_hip.h).

There is no CPU fallback: importing symbols works without a GPU (so the CPU test-suite can check
that the library loads and exports every declared symbol), but every compute entry point needs a
MI355X and the library must have been built (`python -c "import __graft_entry__ as g; g.build()"`).
"""
import ctypes as C
import math
import os
import re
import typing

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libconan_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "conan_hip.h")

ABI_VERSION = 9
MAX_UPS, MAX_RESBLOCKS, MAX_DILATIONS, MAX_DEC_BLOCKS = 8, 4, 4, 16
MODEL_EMFORMER, MODEL_CONAN, MODEL_HIFIGAN, MODEL_FRONTEND = 1, 2, 4, 8

ARITH_AUTO, ARITH_F32, ARITH_LIMB = 0, 1, 2
ARITH_NAMES = {"auto": ARITH_AUTO, "f32": ARITH_F32, "limb": ARITH_LIMB}

OK, ERR_INVALID, ERR_MISSING, ERR_SHAPE, ERR_HIP, ERR_STATE, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6


class ConanCfg(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("hidden_size", C.c_int32), ("num_mels", C.c_int32), ("content_vocab", C.c_int32),
        ("content_kernel", C.c_int32), ("dec_kernel", C.c_int32), ("dec_num_blocks", C.c_int32),
        ("dec_dilations", C.c_int32 * MAX_DEC_BLOCKS), ("dec_layers_in_block", C.c_int32),
        ("dec_post_kernel", C.c_int32), ("predictor_kernel", C.c_int32), ("nvq", C.c_int32),
        ("silent_token", C.c_int32),
        ("emf_input_dim", C.c_int32), ("emf_heads", C.c_int32), ("emf_ffn_dim", C.c_int32),
        ("emf_layers", C.c_int32), ("emf_segment", C.c_int32), ("emf_left_context", C.c_int32),
        ("emf_right_context", C.c_int32), ("emf_output_dim", C.c_int32),
        ("voc_initial_channel", C.c_int32), ("voc_num_ups", C.c_int32),
        ("voc_up_rates", C.c_int32 * MAX_UPS), ("voc_up_kernels", C.c_int32 * MAX_UPS),
        ("voc_num_resblocks", C.c_int32), ("voc_rb_kernels", C.c_int32 * MAX_RESBLOCKS),
        ("voc_rb_num_dil", C.c_int32), ("voc_rb_dilations", (C.c_int32 * MAX_DILATIONS) * MAX_RESBLOCKS),
        ("models", C.c_int32), ("voc_upsample", C.c_int32), ("voc_resblock", C.c_int32),
        ("emf_max_memory_size", C.c_int32), ("emf_tanh_on_mem", C.c_int32)]


class StreamsOpts(C.Structure):
    """conan_streams_opts (include/conan_hip.h)."""
    _fields_ = [("abi_version", C.c_int32), ("arith", C.c_int32), ("flags", C.c_int32), ("reserved0", C.c_int32),
                ("dev_plan", C.c_char_p), ("reserved", C.c_int32 * 2)]


# conan_streams_opts.flags (bit 4 - ABI 7's VOCODER_CHAIN - is retired and rejected)
STREAMS_FUSED_DECODER_BLOCKS, STREAMS_SEPARATE_SMALL_STEPS, STREAMS_FIXED_PLAN, STREAMS_SHARED_DEVICE = 1, 2, 8, 16


class ConanError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libconan_hip error {code}: {msg}")
        self.code = code


_PROTOS = {
    "conan_last_error": (C.c_char_p, []),
    "conan_abi_version": (C.c_int, []),
    "conan_ctx_create": (C.c_int, [C.c_int, C.POINTER(ConanCfg), C.POINTER(C.c_void_p)]),
    "conan_ctx_destroy": (C.c_int, [C.c_void_p]),
    "conan_ctx_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "conan_ctx_finalize": (C.c_int, [C.c_void_p]),
    "conan_streams_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "conan_streams_create_opts": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(StreamsOpts), C.POINTER(C.c_void_p)]),
    "conan_streams_arith": (C.c_int, [C.c_void_p]),
    "conan_streams_destroy": (C.c_int, [C.c_void_p]),
    "conan_streams_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "conan_set_reference": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "conan_emformer_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_emformer_head_dim": (C.c_int, [C.c_void_p, C.c_char_p]),
    "conan_emformer_project": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "conan_decoder_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_hifigan_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_hifigan_step_taps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_set_style": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "conan_get_prosody_ids": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_decoder_step_taps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_get_style": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_wav2mel": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_step_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_streams_join": (C.c_int, [C.c_void_p, C.c_void_p]),
    "conan_step_wav": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_step_wav_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_step_wav_chunk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_step_wav_ragged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_step_wav_ragged_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_step_wav_ragged_ld": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_step_wav_ragged_ld_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_resample_length": (C.c_int64, [C.c_void_p, C.c_int64]),
    "conan_resample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_resample_drift_length": (C.c_int64, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]),
    "conan_resample_drift_table": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "conan_resample_drift": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_int64, C.c_void_p, C.c_void_p]),
    "conan_streams_set_input_drift": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "conan_streams_input_drift": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_streams_set_output_drift": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "conan_streams_output_drift": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_loud_norm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "conan_level": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "conan_streams_set_input_rate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "conan_streams_set_output_rate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "conan_streams_set_output_ld": (C.c_int, [C.c_void_p, C.c_int64]),
    "conan_streams_output_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "conan_streams_output_pending": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "conan_streams_flush_output": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "conan_streams_set_input_format": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "conan_streams_set_output_format": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "conan_convert_samples": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p]),
    "conan_streams_output_fence": (C.c_int, [C.c_void_p, C.c_void_p]),
    "conan_streams_output_fence_event": (C.c_int, [C.c_void_p, C.c_void_p]),
    "conan_streams_test_fault": (C.c_int, [C.c_void_p, C.c_int]),
    "conan_profile_mark": (C.c_int, [C.c_void_p, C.c_void_p]),
    "conan_step_clock": (C.c_int, [C.c_void_p, C.c_int]),
    "conan_step_clock_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int]),
    "conan_step_timeline": (C.c_int, [C.c_void_p, C.c_int]),
    "conan_step_timeline_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int]),
    "conan_profile_begin": (C.c_int, [C.c_void_p]),
    "conan_profile_end": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "conan_profile_kernel": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "conan_hop_size": (C.c_int, [C.c_void_p]),
    "conan_ctx_weight_bytes": (C.c_int64, [C.c_void_p]),
    "conan_streams_state_bytes": (C.c_int64, [C.c_void_p]),
    "conan_streams_layout_id": (C.c_uint64, [C.c_void_p]),
    "conan_streams_snapshot_bytes": (C.c_int64, [C.c_void_p]),
    "conan_streams_export_slots": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "conan_streams_import_slots": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "conan_slot_meta_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "conan_slot_meta_level": (C.c_int, [C.c_void_p, C.c_void_p]),
    "conan_decoder_step_pitch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "conan_slot_meta_pitch": (C.c_int, [C.c_void_p, C.c_void_p]),
    "conan_f0": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "conan_step_wav_contour": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_f0_register": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_activity": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.POINTER(C.c_int32), C.c_void_p]),
    "conan_activity_gate": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "conan_step_wav_activity": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_step_wav_bypass": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_bypass_mix": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                   C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "conan_step_wav_comfort": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_comfort_track": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_comfort_fill": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "conan_streams_output_level_state_bytes": (C.c_int64, [C.c_void_p]),
    "conan_streams_conceal": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "conan_conceal_state_bytes": (C.c_int64, []),
    "conan_streams_echo": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "conan_echo_state_bytes": (C.c_int64, []),
    "conan_echo": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_streams_echo_delay": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "conan_echo_delay_state_bytes": (C.c_int64, []),
    "conan_echo_delay": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                   C.c_void_p, C.c_void_p]),
    "conan_denoise_state_bytes": (C.c_int64, []),
    "conan_mel_denoise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_watermark_state_bytes": (C.c_int64, []),
    "conan_watermark_embed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_watermark_detect": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                         C.c_void_p, C.c_void_p]),
    "conan_watermark_decide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]),
    "conan_tone_table": (C.c_int, [C.c_int, C.c_void_p]),
    "conan_tones": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_tone_fill": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                  C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "conan_step_wav_tones": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_eq_design": (C.c_int, [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double)]),
    "conan_eq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_eq_state_bytes": (C.c_int64, []),
    "conan_conceal": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "conan_trim_silence": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "conan_voices_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "conan_voices_destroy": (C.c_int, [C.c_void_p]),
    "conan_voices_enroll": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "conan_voices_remove": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "conan_voices_info": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "conan_streams_set_voice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "conan_streams_set_voice_mix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "conan_streams_voice": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]),
    "conan_voices_blob_bytes": (C.c_int64, [C.c_void_p]),
    "conan_voices_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "conan_voices_import": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "conan_voice_meta_info": (C.c_int, [C.c_void_p, C.c_void_p]),
}

_lib = None


def declared_symbols():
    """Function names declared in include/conan_hip.h."""
    with open(HEADER_PATH) as f:
        txt = f.read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(conan_[a-z_0-9]+)\s*\(", txt)))


def lib():
    """The loaded library.  Fails loudly when it has not been built: no CPU fallback exists."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()').  conan_amd has no CPU fallback.")
        # PyTorch-ROCm bundles its own HIP runtime; load it first so that libconan_hip.so binds to the same
        # libamdhip64 (two runtimes in one process do not see each other's devices / streams).
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOS.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        if l.conan_abi_version() != ABI_VERSION:
            raise ImportError("libconan_hip.so ABI version mismatch; rebuild it")
        _lib = l
    return _lib


def check(rc):
    if rc < 0:
        raise ConanError(rc, lib().conan_last_error().decode("utf-8", "replace"))
    return rc


class MelCfg(C.Structure):
    """conan_mel_cfg (include/conan_hip.h)."""
    _fields_ = [("fft_size", C.c_int32), ("hop_size", C.c_int32), ("win_length", C.c_int32), ("num_mels", C.c_int32),
                ("sample_rate", C.c_int32), ("fmin", C.c_float), ("fmax", C.c_float), ("eps", C.c_float),
                ("vmin", C.c_float), ("vmax", C.c_float), ("framing", C.c_int32), ("natural_log", C.c_int32),
                ("mag_eps", C.c_float)]


# conan_resample_cfg.window
RESAMPLE_HANN, RESAMPLE_KAISER = 0, 1
RESAMPLE_MAX_TAPS = 8192
KAISER_BEST_BETA = 14.769656459379492     # conan_resample_cfg.beta <= 0 selects it (in double; a float beta is rounded to f32)
# named filter presets: torchaudio's defaults, and torchaudio's documented values that mimic resampy's kaiser_best
RESAMPLE_PRESETS = {
    "hann": dict(lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None),
    "kaiser_best": dict(lowpass_filter_width=64, rolloff=0.9475937167399596, resampling_method="sinc_interp_kaiser", beta=None),
}


# conan_resample_drift: the side a drift describes, the law's limits, and the schedule a caller writes in ppm
DRIFT_SOURCE, DRIFT_SINK = 0, 1
DRIFT_SIDES = {"source": DRIFT_SOURCE, "sink": DRIFT_SINK}
DRIFT_MAX_PPB = 2000000
DRIFT_MAX_SEGMENTS = 32
DRIFT_PHASES = 1024


def drift_ppb(ppm):
    """ppm (float) -> the law's integer ppb, round(ppm * 1000); |ppb| <= DRIFT_MAX_PPB."""
    ppb = int(round(float(ppm) * 1000))
    if abs(ppb) > DRIFT_MAX_PPB:
        raise ValueError("drift must be within +-%g ppm, got %r" % (DRIFT_MAX_PPB / 1000.0, ppm))
    return ppb


def drift_ppb_rows(ppm, n):
    """One ppm for all of n slots, or one per slot -> int32 [n] ppb."""
    import numpy as np
    vals = [ppm] * n if isinstance(ppm, (int, float)) else list(ppm)
    if len(vals) != n:
        raise ValueError("%d drift values for %d slots" % (len(vals), n))
    return np.ascontiguousarray([drift_ppb(v) for v in vals], dtype=np.int32)


def drift_side(side):
    if side not in DRIFT_SIDES:
        raise ValueError("side must be one of %s, got %r" % (sorted(DRIFT_SIDES), side))
    return DRIFT_SIDES[side]


def drift_schedule(drift):
    """A ppm float, or a list of (output_index, ppm) -> (at int64 [n_seg], ppb int32 [n_seg]) as conan_resample_drift takes them."""
    import numpy as np
    seq = [(0, drift)] if isinstance(drift, (int, float)) else [(int(a), p) for a, p in drift]
    if not seq or seq[0][0] != 0:
        raise ValueError("a drift schedule starts at output index 0")
    if any(b[0] <= a[0] for a, b in zip(seq, seq[1:])):
        raise ValueError("the output indices of a drift schedule must be strictly ascending")
    if len(seq) > DRIFT_MAX_SEGMENTS:
        raise ValueError("a drift schedule has at most %d segments" % DRIFT_MAX_SEGMENTS)
    return (np.ascontiguousarray([a for a, _ in seq], dtype=np.int64), np.ascontiguousarray([drift_ppb(p) for _, p in seq], dtype=np.int32))


# CONAN_SAMPLE_*: the sample formats of the audio rows (conan_streams_set_input_format / _output_format, conan_convert_samples)
SAMPLE_F32, SAMPLE_S16, SAMPLE_ULAW, SAMPLE_ALAW = 0, 1, 2, 3
SAMPLE_FORMATS = {"f32": SAMPLE_F32, "s16": SAMPLE_S16, "ulaw": SAMPLE_ULAW, "alaw": SAMPLE_ALAW}
SAMPLE_BYTES = {"f32": 4, "s16": 2, "ulaw": 1, "alaw": 1}


def sample_format(fmt):
    """CONAN_SAMPLE_* of 'f32' | 's16' | 'ulaw' | 'alaw' (None: 'f32')."""
    fmt = "f32" if fmt is None else fmt
    if fmt not in SAMPLE_FORMATS:
        raise ValueError("sample format must be one of %s, got %r" % (sorted(SAMPLE_FORMATS), fmt))
    return SAMPLE_FORMATS[fmt]


class ResampleCfg(C.Structure):
    """conan_resample_cfg (include/conan_hip.h)."""
    _fields_ = [("in_rate", C.c_int32), ("out_rate", C.c_int32), ("lowpass_filter_width", C.c_int32), ("rolloff", C.c_float),
                ("window", C.c_int32), ("beta", C.c_float), ("reserved", C.c_int32 * 2)]


def resample_cfg(orig_freq, new_freq=16000, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None,
                 preset=None):
    """conan_resample_cfg with torchaudio.functional.resample's keywords; preset='hann' / 'kaiser_best' replaces the filter keywords."""
    if preset is not None:
        if preset not in RESAMPLE_PRESETS:
            raise ValueError("preset must be one of %s" % sorted(RESAMPLE_PRESETS))
        p = RESAMPLE_PRESETS[preset]
        lowpass_filter_width, rolloff, resampling_method, beta = p["lowpass_filter_width"], p["rolloff"], p["resampling_method"], p["beta"]
    if resampling_method not in ("sinc_interp_hann", "sinc_interp_kaiser"):
        raise ValueError("resampling_method must be 'sinc_interp_hann' or 'sinc_interp_kaiser'")
    window = RESAMPLE_HANN if resampling_method == "sinc_interp_hann" else RESAMPLE_KAISER
    return ResampleCfg(int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff), window,
                       float(beta) if beta is not None else 0.0, (C.c_int32 * 2)(0, 0))


def resample_drift_table(orig_freq, new_freq=16000, **filter):
    """conan_resample_drift_table (host only; needs no device): the drift resampler's f32 table, numpy [1025, 2W]."""
    import numpy as np
    cfg = resample_cfg(orig_freq, new_freq, **filter)
    W = C.c_int32(0)
    count = check(lib().conan_resample_drift_table(C.byref(cfg), C.byref(W), None, 0))
    tab = np.empty(count, dtype=np.float32)
    check(lib().conan_resample_drift_table(C.byref(cfg), C.byref(W), tab.ctypes.data, count))
    return tab.reshape(DRIFT_PHASES + 1, 2 * W.value)


def resample_drift_length(orig_freq, new_freq, samples, drift, side="source", **filter):
    """conan_resample_drift_length (host only, exact): the outputs of `samples` inputs under the schedule (Context.resample_drift's)."""
    cfg = resample_cfg(orig_freq, new_freq, **filter)
    at, ppb = drift_schedule(drift)
    n = lib().conan_resample_drift_length(C.byref(cfg), drift_side(side), int(samples), at.ctypes.data, ppb.ctypes.data, len(at))
    if n < 0:
        raise ValueError("resample_drift_length: the library refuses this configuration or schedule")
    return n


SLOT_META_BYTES = 256


class SlotMeta(C.Structure):
    """conan_slot_meta (include/conan_hip.h): the host half of a slot snapshot, opaque."""
    _fields_ = [("opaque", C.c_ubyte * SLOT_META_BYTES)]


class SlotInfo(C.Structure):
    """conan_slot_info (include/conan_hip.h): what a caller may read out of a conan_slot_meta."""
    _fields_ = [("layout_id", C.c_uint64), ("bytes", C.c_int64), ("has_ref", C.c_int32), ("in_format", C.c_int32),
                ("out_format", C.c_int32), ("reserved", C.c_int32), ("in_rate", ResampleCfg), ("out_rate", ResampleCfg)]


VOICE_META_BYTES = 256
VOICE_MAX_MIX = 4      # voices conan_streams_set_voice_mix blends into one style vector


class VoiceMeta(C.Structure):
    """conan_voice_meta (include/conan_hip.h): the host half of an exported voice, opaque."""
    _fields_ = [("opaque", C.c_ubyte * VOICE_META_BYTES)]


class VoiceInfo(C.Structure):
    """conan_voice_info (include/conan_hip.h): a bank entry, or what a caller may read out of a conan_voice_meta."""
    _fields_ = [("enrolled", C.c_int32), ("ref_frames", C.c_int32), ("tokens", C.c_int32), ("reserved", C.c_int32),
                ("bytes", C.c_int64), ("layout_id", C.c_uint64)]


class LoudnessCfg(C.Structure):
    """conan_loudness_cfg (include/conan_hip.h)."""
    _fields_ = [("sample_rate", C.c_int32), ("target_lufs", C.c_float), ("peak_limit", C.c_int32), ("reserved", C.c_int32 * 3)]


LEVEL_MAX_BLOCKS = 4096


class LevelCfg(C.Structure):
    """conan_level_cfg (include/conan_hip.h)."""
    _fields_ = [("enabled", C.c_int32), ("target_lufs", C.c_float), ("max_boost_db", C.c_float), ("max_cut_db", C.c_float),
                ("initial_gain_db", C.c_float), ("window_blocks", C.c_int32), ("peak_limit", C.c_int32), ("clip", C.c_int32),
                ("reserved", C.c_int32 * 4)]


def level_cfg(target=-22.0, max_boost_db=20.0, max_cut_db=40.0, initial_gain_db=0.0, window_blocks=LEVEL_MAX_BLOCKS, peak_limit=True,
              clip=False):
    """An enabled conan_level_cfg.  The defaults are a choice, not a measurement: the reference's loud_norm target, a boost cap that
    keeps a silent line's noise floor down, a window that is the whole call for anything under 6.8 minutes."""
    return LevelCfg(1, float(target), float(max_boost_db), float(max_cut_db), float(initial_gain_db), int(window_blocks),
                    int(bool(peak_limit)), int(bool(clip)), (C.c_int32 * 4)(0, 0, 0, 0))


def level_keywords(c):
    """level_cfg's keywords of an enabled LevelCfg: the one form Streams.input_levels and SlotSnapshot.info report a leveller in."""
    return dict(target=c.target_lufs, max_boost_db=c.max_boost_db, max_cut_db=c.max_cut_db, initial_gain_db=c.initial_gain_db,
                window_blocks=c.window_blocks, peak_limit=bool(c.peak_limit), clip=bool(c.clip))


class PitchCfg(C.Structure):
    """conan_pitch_cfg (include/conan_hip.h)."""
    _fields_ = [("enabled", C.c_int32), ("shift_semitones", C.c_float), ("range", C.c_float), ("pivot", C.c_float),
                ("uv_threshold", C.c_float), ("reserved", C.c_int32)]


PITCH_PIVOT = 7.5      # log2 Hz (181 Hz): where `range` pivots unless the caller says otherwise


def pitch_cfg(shift_semitones=0.0, range=1.0, pivot=PITCH_PIVOT, uv_threshold=0.0):
    """An enabled conan_pitch_cfg: transpose by shift_semitones, scale the contour's excursion around `pivot` (log2 Hz) by `range`,
    call a frame unvoiced when the head's d0 exceeds uv_threshold.  The defaults change nothing but the code path."""
    return PitchCfg(1, float(shift_semitones), float(range), float(pivot), float(uv_threshold), 0)


def pitch_keywords(c):
    """pitch_cfg's keywords of an enabled PitchCfg: the form Streams.pitch and SlotSnapshot.info report a pitch control in."""
    return dict(shift_semitones=c.shift_semitones, range=c.range, pivot=c.pivot, uv_threshold=c.uv_threshold)


class F0Cfg(C.Structure):
    """conan_f0_cfg (include/conan_hip.h)."""
    _fields_ = [("enabled", C.c_int32), ("fmin", C.c_float), ("fmax", C.c_float), ("threshold", C.c_float), ("floor_db", C.c_float),
                ("reserved", C.c_int32)]


def f0_cfg(fmin=50.0, fmax=900.0, threshold=0.15, floor_db=-60.0):
    """An enabled conan_f0_cfg: the YIN tracker's search range in Hz, its absolute threshold and the power floor under which a frame
    is unvoiced.  The defaults are the range of denorm_f0's clamp and YIN's usual threshold."""
    return F0Cfg(1, float(fmin), float(fmax), float(threshold), float(floor_db), 0)


def f0_keywords(c):
    """f0_cfg's keywords of an enabled F0Cfg: the form Streams.pitch_follow reports a follow setting in."""
    return dict(fmin=c.fmin, fmax=c.fmax, threshold=c.threshold, floor_db=c.floor_db)


class RegisterCfg(C.Structure):
    """conan_register_cfg (include/conan_hip.h)."""
    _fields_ = [("enabled", C.c_int32), ("reseed", C.c_int32), ("target", C.c_float), ("max_shift", C.c_float), ("seed_count", C.c_int64),
                ("seed_sum", C.c_int64)]


REGISTER_UNIT = 4194304      # 2^22: quantised log2-f0 units per octave


def register_quantise(v):
    """q of the law for a log2-Hz value: llrint((double)(float)v * 2^22), a Python int."""
    return int(round(C.c_float(v).value * float(REGISTER_UNIT)))      # (the product is exact in f64; round() ties to even, as llrint)


def register_cfg(target, max_shift=2.0, prior=None, prior_frames=50, seed=None, reseed=False):
    """An enabled conan_register_cfg: move the slot's mean log-f0 to `target` (log2 Hz), by at most max_shift octaves.  The estimate
    starts from seed = (count, sum) where given - a queried state: the hand-over - and else from the prior: prior_frames voiced frames
    at `prior` (log2 Hz; default: the target, so the shift starts at 0)."""
    if target is None:
        raise ValueError("register: target= (log2 Hz) is required")
    if seed is not None:
        count, total = (int(x) for x in seed)
    else:
        count = int(prior_frames)
        total = count * register_quantise(target if prior is None else prior)
    return RegisterCfg(1, int(bool(reseed)), float(target), float(max_shift), count, total)


def register_keywords(c):
    """register_cfg's keywords of an enabled RegisterCfg: the form a register setting is reported in."""
    return dict(target=c.target, max_shift=c.max_shift, seed=(int(c.seed_count), int(c.seed_sum)))


class ActivityState(C.Structure):
    """conan_activity_state (include/conan_hip.h)."""
    _fields_ = [("active", C.c_int32), ("hang", C.c_int32), ("level", C.c_int32), ("reserved", C.c_int32), ("floor", C.c_double),
                ("frames", C.c_int64), ("active_frames", C.c_int64)]


class ActivityCfg(C.Structure):
    """conan_activity_cfg (include/conan_hip.h)."""
    _fields_ = [("mode", C.c_int32), ("reseed", C.c_int32), ("open_abs", C.c_float), ("close_abs", C.c_float), ("open_ratio", C.c_float),
                ("close_ratio", C.c_float), ("rise_active", C.c_float), ("rise_idle", C.c_float), ("floor_min", C.c_float),
                ("hold_frames", C.c_int32), ("up_step", C.c_int32), ("down_step", C.c_int32), ("closed_level", C.c_int32), ("reserved", C.c_int32),
                ("seed", ActivityState)]


ACTIVITY_FULL = 1 << 20      # the open gate's level
ACTIVITY_STATE_FIELDS = ("active", "hang", "level", "floor", "frames", "active_frames")


def db_power(db):
    """A decibel figure as the linear power the law reads: the f32 nearest to 10^(db / 10), as a Python float."""
    return C.c_float(10.0 ** (float(db) / 10.0)).value


def activity_state(state):
    """A dict of ACTIVITY_STATE_FIELDS (what Streams.activity_state returns), or an ActivityState, as an ActivityState."""
    if isinstance(state, ActivityState):
        return state
    return ActivityState(int(state["active"]), int(state["hang"]), int(state["level"]), 0, float(state["floor"]), int(state["frames"]),
                         int(state["active_frames"]))


def activity_state_dict(s):
    return dict(active=int(s.active), hang=int(s.hang), level=int(s.level), floor=float(s.floor), frames=int(s.frames),
                active_frames=int(s.active_frames))


def activity_cfg(gate=True, open_db=-50.0, close_db=-55.0, open_over_db=9.0, close_over_db=6.0, rise_active=1.005, rise_idle=1.02,
                 floor_min_db=-70.0, floor_db=-60.0, hold_frames=10, attack_frames=1, release_frames=5, closed_db=None, open_abs=None,
                 close_abs=None, open_ratio=None, close_ratio=None, floor_min=None, up_step=None, down_step=None, closed_level=None, seed=None,
                 reseed=False):
    """An enabled conan_activity_cfg: detect (gate=False: mode 1) or detect and gate the output (mode 2).  Thresholds in dBFS of the
    frame power (open_db / close_db), in dB over the noise floor (open_over_db / close_over_db); the floor's largest growth per 20 ms
    frame while active / idle; its minimum and its initial value in dB; the hangover in frames; the gate's attack and release in
    frames and its closed level in dB (None: silence).  The defaults are choices, not measurements.  Every decibel figure is
    converted to the f32 linear power the law reads (db_power); the linear keywords (open_abs, close_abs, open_ratio, close_ratio,
    floor_min) and the integer ones (up_step, down_step, closed_level) give a field directly and win over their dB / frame forms.
    seed: the state to start from (a dict as Streams.activity_state returns - the hand-over - or an ActivityState); default: idle,
    the gate closed, the floor at floor_db."""
    cl = int(closed_level) if closed_level is not None else (0 if closed_db is None else int(round(ACTIVITY_FULL * 10.0 ** (float(closed_db) / 20.0))))
    span = ACTIVITY_FULL - cl
    up = int(up_step) if up_step is not None else max(1, -(-span // int(attack_frames)))
    down = int(down_step) if down_step is not None else max(1, -(-span // int(release_frames)))
    fmin = db_power(floor_min_db) if floor_min is None else float(floor_min)
    st = ActivityState(0, 0, cl, 0, max(db_power(floor_db), C.c_float(fmin).value), 0, 0) if seed is None else activity_state(seed)
    return ActivityCfg(2 if gate else 1, int(bool(reseed)),
                       db_power(open_db) if open_abs is None else float(open_abs), db_power(close_db) if close_abs is None else float(close_abs),
                       db_power(open_over_db) if open_ratio is None else float(open_ratio),
                       db_power(close_over_db) if close_ratio is None else float(close_ratio), float(rise_active), float(rise_idle), fmin,
                       int(hold_frames), up, down, cl, 0, st)


def activity_keywords(c):
    """activity_cfg's keywords of an enabled ActivityCfg, in the linear / integer forms that give the same fields back exactly: the form
    Streams.activity reports a setting in."""
    return dict(gate=c.mode == 2, open_abs=c.open_abs, close_abs=c.close_abs, open_ratio=c.open_ratio, close_ratio=c.close_ratio,
                rise_active=c.rise_active, rise_idle=c.rise_idle, floor_min=c.floor_min, hold_frames=c.hold_frames, up_step=c.up_step,
                down_step=c.down_step, closed_level=c.closed_level, seed=activity_state_dict(c.seed))


class TrimCfg(C.Structure):
    """conan_trim_cfg (include/conan_hip.h)."""
    _fields_ = [("smooth_frames", C.c_int32), ("max_silence_frames", C.c_int32), ("reserved", C.c_int32 * 2)]


def trim_cfg(smooth_frames=12, max_silence_frames=18):
    """conan_trim_cfg: the moving average's width and the longest pause that is kept whole, in 20 ms frames.  The defaults are the
    reference's 8 and 12 windows of 30 ms kept as durations; they are choices, not measurements."""
    return TrimCfg(int(smooth_frames), int(max_silence_frames), (C.c_int32 * 2)(0, 0))


class BypassCfg(C.Structure):
    """conan_bypass_cfg (include/conan_hip.h)."""
    _fields_ = [("enabled", C.c_int32), ("reseed", C.c_int32), ("wet_target", C.c_int32), ("dry_target", C.c_int32), ("step", C.c_int32),
                ("fill_gate", C.c_int32), ("seed_wet", C.c_int32), ("seed_dry", C.c_int32)]


class BypassState(C.Structure):
    """conan_bypass_state (include/conan_hip.h)."""
    _fields_ = [("wet", C.c_int32), ("dry", C.c_int32), ("dry_eff", C.c_int32), ("reserved", C.c_int32)]


def bypass_level(share=None, db=None):
    """A linear share (1.0 = full) or a decibel figure (0 dB = full) as the law's integer level: rint(share * 2^20), converted once on
    the host.  Host only."""
    if db is not None:
        share = 10.0 ** (float(db) / 20.0)
    return int(round(float(share) * ACTIVITY_FULL))      # (round half to even: rint)


def bypass_step(ramp_ms):
    """The slew per 20 ms frame of a full-scale ramp of ramp_ms: ceil(2^20 / max(1, ramp_ms / 20))."""
    return int(math.ceil(ACTIVITY_FULL / max(1.0, float(ramp_ms) / 20.0)))


def bypass_cfg(wet=1.0, dry=0.0, ramp_ms=40.0, fill_gate=False, start=None, reseed=False, wet_db=None, dry_db=None, step=None):
    """An enabled conan_bypass_cfg.  wet / dry: the targets as linear shares of the converted and of the source audio (wet_db= / dry_db=
    give them in decibels instead); ramp_ms: the time a full-scale change takes (step= gives the levels per frame directly); fill_gate:
    the dry share is scaled by the closed part of the slot's activity gate (the caller's room tone in pauses); start: the (wet, dry)
    integer levels 0 .. 2^20 a restart begins from (default: the targets, so a fresh slot does not fade in).  The defaults - full wet,
    no dry, a 40 ms ramp - are choices, not measurements."""
    w, d = bypass_level(wet, wet_db), bypass_level(dry, dry_db)
    sw, sd = (w, d) if start is None else (int(start[0]), int(start[1]))
    return BypassCfg(1, int(bool(reseed)), w, d, bypass_step(ramp_ms) if step is None else int(step), int(bool(fill_gate)), sw, sd)


def bypass_keywords(c):
    """bypass_cfg's keywords of an enabled BypassCfg in the integer forms that give the same fields back exactly (wet / dry as shares
    k / 2^20, which rint(share * 2^20) maps back to k): the form Streams.bypass reports a setting in."""
    return dict(wet=c.wet_target / ACTIVITY_FULL, dry=c.dry_target / ACTIVITY_FULL, step=int(c.step), fill_gate=bool(c.fill_gate),
                start=(int(c.seed_wet), int(c.seed_dry)))


class ComfortCfg(C.Structure):
    """conan_comfort_cfg (include/conan_hip.h)."""
    _fields_ = [("mode", C.c_int32), ("reseed", C.c_int32), ("level", C.c_int32), ("offset", C.c_int32), ("l_min", C.c_int32), ("l_max", C.c_int32),
                ("up_step", C.c_int32), ("down_step", C.c_int32), ("colour", C.c_int32), ("seed_level", C.c_int32), ("norm", C.c_float),
                ("reserved", C.c_int32), ("seed", C.c_uint64)]


class ComfortState(C.Structure):
    """conan_comfort_state (include/conan_hip.h)."""
    _fields_ = [("level", C.c_int32), ("reserved", C.c_int32), ("idle_frames", C.c_int64)]


COMFORT_LEVEL_MIN = -16384
COMFORT_UNITS_PER_DB = 256.0 / (10.0 * math.log10(2.0))      # about 85.04: levels are 1/256 octaves of power
COMFORT_TAPS = ((1,), (1, 2, 1), (1, 2, 3, 2, 1))


def comfort_level(db):
    """A decibel figure (dBov: 0 = full scale; or a difference in dB) as the law's integer level, 1/256 octave of power: rint(db *
    85.04), converted once on the host.  Host only."""
    return int(round(float(db) * COMFORT_UNITS_PER_DB))


def comfort_norm(colour):
    """The amplitude of one unit of the coloured noise v at level 0, so that its rms is 1 there: the f32 of 1 / (sqrt((65536^2 - 1) /
    6) * sqrt(sum c^2)) - w is the sum of two uniform 16-bit words less its mean - formed once on the host."""
    return C.c_float(1.0 / (math.sqrt((65536.0 ** 2 - 1.0) / 6.0) * math.sqrt(float(sum(c * c for c in COMFORT_TAPS[int(colour)]))))).value


def comfort_seed(slot):
    """The default seed of a slot's white source: derived from the slot's index, so that two slots do not share a sequence."""
    return 0x636F6D666F727400 + int(slot)


def comfort_cfg(follow=True, level_db=-60.0, offset_db=-3.0, min_db=-90.0, max_db=-30.0, rise_db=0.25, fall_db=2.0, colour=1, start_db=-70.0,
                seed=0, reseed=False, level=None, offset=None, l_min=None, l_max=None, up_step=None, down_step=None, start=None, norm=None):
    """An enabled conan_comfort_cfg: follow the source's background (mode 2) or hold level_db (follow=False: mode 1).  offset_db: added
    to the frame power of an inactive frame; min_db / max_db: the level's limits in dBov; rise_db / fall_db: its largest rise and fall
    per 20 ms frame; colour: 0 white, 1 and 2 low-passed by the taps {1, 2, 1} / {1, 2, 3, 2, 1}; start_db: the level a restart
    begins from; seed: of the white source.  The defaults - follow, 3 dB under the background, -90 .. -30 dBov, a rise of 0.25 dB and
    a fall of 2 dB per frame, colour 1, a start at -70 dBov - are choices, not measurements.  Every decibel figure is converted to
    the law's integer levels once (comfort_level); the integer keywords (level, offset, l_min, l_max, up_step, down_step, start) give
    a field directly and win over their dB forms, and norm= over comfort_norm(colour)."""
    pick = lambda direct, db: comfort_level(db) if direct is None else int(direct)      # noqa: E731
    step = lambda direct, db: max(1, comfort_level(db)) if direct is None else int(direct)      # noqa: E731
    return ComfortCfg(2 if follow else 1, int(bool(reseed)), pick(level, level_db), pick(offset, offset_db), pick(l_min, min_db), pick(l_max, max_db),
                      step(up_step, rise_db), step(down_step, fall_db), int(colour), pick(start, start_db),
                      comfort_norm(colour) if norm is None else float(norm), 0, int(seed) & ((1 << 64) - 1))


def comfort_keywords(c):
    """comfort_cfg's keywords of an enabled ComfortCfg in the integer forms that give the same fields back exactly: the form
    Streams.comfort reports a setting in."""
    return dict(follow=c.mode == 2, level=int(c.level), offset=int(c.offset), l_min=int(c.l_min), l_max=int(c.l_max), up_step=int(c.up_step),
                down_step=int(c.down_step), colour=int(c.colour), start=int(c.seed_level), norm=float(c.norm), seed=int(c.seed))


def comfort_dbov(level):
    """The RFC 3389 noise level byte of a comfort level L (Streams.step_wav_comfort, comfort_state): -dBov, rounded, in 0 .. 127."""
    return max(0, min(127, int(round(-float(level) / COMFORT_UNITS_PER_DB))))


CONCEAL_MAX_LAG, CONCEAL_MAX_WINDOW = 1024, 1024


class ConcealCfg(C.Structure):
    """conan_conceal_cfg (include/conan_hip.h)."""
    _fields_ = [("enabled", C.c_int32), ("packet", C.c_int32), ("lag_min", C.c_int32), ("lag_max", C.c_int32), ("window", C.c_int32),
                ("hold", C.c_int32), ("fall", C.c_int32), ("fade", C.c_int32)]


def conceal_keywords(rate):
    """The documented defaults of the loss concealment for an input rate, or - given an enabled ConcealCfg - its fields: the keywords
    conceal_cfg takes.  20 ms packets, lags of 2.5 .. 15 ms, a 20 ms comparison window, 10 ms at full level, a 50 ms fall, a 5 ms
    cross-fade; at 48 kHz every one lies within the library's limits.  They are choices, not measurements."""
    if isinstance(rate, ConcealCfg):
        return {f: int(getattr(rate, f)) for f, _ in ConcealCfg._fields_[1:]}
    r = int(rate)
    return dict(packet=r // 50, lag_min=r // 400, lag_max=r * 15 // 1000, window=r // 50, hold=r // 100, fall=r // 20, fade=r // 200)


def conceal_cfg(rate=None, **kw):
    """An enabled conan_conceal_cfg: conceal_keywords(rate) with the given fields replaced (rate=None: every field must be given)."""
    base = conceal_keywords(rate) if rate is not None else {}
    f = dict(base, **kw)
    names = [n for n, _ in ConcealCfg._fields_[1:]]
    unknown = sorted(set(f) - set(names))
    if unknown:
        raise ValueError(f"conceal: unknown fields {unknown}")
    missing = [n for n in names if n not in f]
    if missing:
        raise ValueError(f"conceal: without a rate the fields {missing} must be given")
    return ConcealCfg(1, *[int(f[n]) for n in names])


ECHO_BLOCK, ECHO_MAX_TAPS, ECHO_MAX_DELAY, ECHO_MAX_SHIFT, ECHO_HISTORY = 64, 2048, 4096, 12, 6208


class EchoCfg(C.Structure):
    """conan_echo_cfg (include/conan_hip.h)."""
    _fields_ = [("enabled", C.c_int32), ("taps", C.c_int32), ("delay", C.c_int32), ("mu_shift", C.c_int32), ("dt_num", C.c_int32),
                ("dt_den", C.c_int32), ("hang", C.c_int32), ("reserved", C.c_int32), ("reg", C.c_int64), ("far_min", C.c_int64)]


_ECHO_FIELDS = ("taps", "delay", "mu_shift", "dt_num", "dt_den", "hang", "reg", "far_min")


def echo_keywords(rate):
    """The documented defaults of the echo canceller for an input rate, or - given an enabled EchoCfg - its fields: the keywords
    echo_cfg takes.  A 64 ms filter (a multiple of 64 taps, at most 2048), no bulk delay, step shift 4, a Geigel threshold of 1/2
    with 50 ms of hang-over, reg = taps * 4096 and far_min = taps * 1024.  They are choices, not measurements."""
    if isinstance(rate, EchoCfg):
        return {f: int(getattr(rate, f)) for f in _ECHO_FIELDS}
    r = int(rate)
    taps = min(ECHO_MAX_TAPS, max(ECHO_BLOCK, (r * 64 // 1000 + 32) // 64 * 64))
    return dict(taps=taps, delay=0, mu_shift=4, dt_num=1, dt_den=2, hang=(r // 20 + ECHO_BLOCK - 1) // ECHO_BLOCK, reg=taps * 4096, far_min=taps * 1024)


def echo_cfg(rate=None, **kw):
    """An enabled conan_echo_cfg: echo_keywords(rate) with the given fields replaced (rate=None: every field must be given)."""
    base = echo_keywords(rate) if rate is not None else {}
    f = dict(base, **kw)
    unknown = sorted(set(f) - set(_ECHO_FIELDS))
    if unknown:
        raise ValueError(f"echo: unknown fields {unknown}")
    missing = [n for n in _ECHO_FIELDS if n not in f]
    if missing:
        raise ValueError(f"echo: without a rate the fields {missing} must be given")
    c = EchoCfg()
    c.enabled = 1
    for n in _ECHO_FIELDS:
        setattr(c, n, int(f[n]))
    return c


ECHO_DELAY_FRAME, ECHO_DELAY_MAX_LAGS = 1024, 6144
ECHO_DELAY_REPORT = ("est", "age", "cand", "run", "last_pk", "last_s")      # the columns of a report row


class EchoDelayCfg(C.Structure):
    """conan_echo_delay_cfg (include/conan_hip.h)."""
    _fields_ = [("enabled", C.c_int32), ("n_lags", C.c_int32), ("thr", C.c_int32), ("leak", C.c_int32), ("ratio", C.c_int32),
                ("min_peak", C.c_int32), ("hold", C.c_int32), ("tol", C.c_int32), ("reserved", C.c_int32 * 4)]


_ECHO_DELAY_FIELDS = ("n_lags", "thr", "leak", "ratio", "min_peak", "hold", "tol")
_ECHO_DELAY_RANGES = dict(n_lags=(64, ECHO_DELAY_MAX_LAGS), thr=(1, 32767), leak=(1, 8), ratio=(1, 2**31 - 1), min_peak=(1, 2**31 - 1),
                          hold=(1, 2**31 - 1), tol=(0, 2**31 - 1))


def echo_delay_keywords(rate):
    """The documented defaults of the echo-delay estimator for an input rate, or - given an enabled EchoDelayCfg - its fields: the
    keywords echo_delay_cfg takes.  Lags over 384 ms (a multiple of 64, at most 6144), a ternary threshold of 16, leak 5, a peak
    of 10 times the mean and at least 1024, 4 frames to confirm within 2 ms.  They are choices, not measurements."""
    if isinstance(rate, EchoDelayCfg):
        return {f: int(getattr(rate, f)) for f in _ECHO_DELAY_FIELDS}
    r = int(rate)
    n_lags = min(ECHO_DELAY_MAX_LAGS, max(64, (r * 384 // 1000 + 32) // 64 * 64))
    return dict(n_lags=n_lags, thr=16, leak=5, ratio=10, min_peak=1024, hold=4, tol=r * 2 // 1000)


def echo_delay_cfg(rate=None, **kw):
    """An enabled conan_echo_delay_cfg: echo_delay_keywords(rate) with the given fields replaced (rate=None: every field must be
    given).  A field outside the header's range is a ValueError here, before any library call."""
    base = echo_delay_keywords(rate) if rate is not None else {}
    f = dict(base, **kw)
    unknown = sorted(set(f) - set(_ECHO_DELAY_FIELDS))
    if unknown:
        raise ValueError(f"echo_delay: unknown fields {unknown}")
    missing = [n for n in _ECHO_DELAY_FIELDS if n not in f]
    if missing:
        raise ValueError(f"echo_delay: without a rate the fields {missing} must be given")
    c = EchoDelayCfg()
    c.enabled = 1
    for n in _ECHO_DELAY_FIELDS:
        lo, hi = _ECHO_DELAY_RANGES[n]
        if not lo <= int(f[n]) <= hi or (n == "n_lags" and int(f[n]) % 64):
            raise ValueError(f"echo_delay: {n} = {f[n]!r} is outside {lo} .. {hi}" + (" in steps of 64" if n == "n_lags" else ""))
        setattr(c, n, int(f[n]))
    return c


def echo_delay_follow(est, age, in_force, lead, hyst, max_age):
    """The host rule between calls: from an estimator's report (est, age) and the canceller's delay in force, the delay to set, or
    None to leave it.  target = clamp(est - lead, 0, ECHO_MAX_DELAY), so that the filter's first taps lie `lead` samples in front of
    the estimated lag; it is applied when there is an estimate (est >= 0) that is no older than max_age frames and the target is
    more than hyst samples from the delay in force.  Pure: no state, no device."""
    est, age, in_force = int(est), int(age), int(in_force)
    if est < 0 or age > int(max_age):
        return None
    target = min(max(est - int(lead), 0), ECHO_MAX_DELAY)
    return target if abs(target - in_force) > int(hyst) else None


def echo_delay_follow_keywords(rate):
    """The defaults of the engine's follow rule for an input rate: lead 8 ms, hyst 4 ms, max_age 64 frames.  Choices."""
    r = int(rate)
    return dict(lead=r * 8 // 1000, hyst=r * 4 // 1000, max_age=64)


class DenoiseCfg(C.Structure):
    """conan_denoise_cfg (include/conan_hip.h)."""
    _fields_ = [("enabled", C.c_int32), ("reseed", C.c_int32), ("bias", C.c_int32), ("knee", C.c_int32), ("slope", C.c_int32), ("depth", C.c_int32),
                ("close_step", C.c_int32), ("open_step", C.c_int32), ("rise", C.c_int32), ("fall_shift", C.c_int32), ("floor_min", C.c_int32),
                ("smooth", C.c_int32), ("out_floor", C.c_float), ("reserved", C.c_int32 * 3)]


DENOISE_MAX_BINS = 256


class DenoiseState(C.Structure):
    """conan_denoise_state (include/conan_hip.h): a row of Streams.denoise_state / Context.mel_denoise(state=True)."""
    _fields_ = [("frames", C.c_int64), ("bins", C.c_int32), ("reserved", C.c_int32), ("floor", C.c_int32 * DENOISE_MAX_BINS),
                ("att", C.c_int32 * DENOISE_MAX_BINS)]


DENOISE_FULL = 1 << 20
# (field, lowest, highest) of an enabled conan_denoise_cfg's integer fields
DENOISE_RANGES = (("bias", 0, DENOISE_FULL), ("knee", 0, DENOISE_FULL), ("slope", 0, 1 << 16), ("depth", 1, DENOISE_FULL),
                  ("close_step", 1, DENOISE_FULL), ("open_step", 1, DENOISE_FULL), ("rise", 0, DENOISE_FULL), ("fall_shift", 0, 8),
                  ("floor_min", -DENOISE_FULL, DENOISE_FULL), ("smooth", 0, 1))


def denoise_level(db, natural_log=False):
    """A decibel figure as the suppressor's integer level: 1024 steps per unit of the mel's logarithm, which is 20 dB for log10 and
    20 / ln(10) = 8.686 dB for the natural logarithm.  Converted once, on the host."""
    return int(round(float(db) * 1024.0 / (20.0 / math.log(10.0) if natural_log else 20.0)))


def denoise_cfg(natural_log=False, mel_vmin=-6.0, eps=1e-6, bias_db=3.0, knee_db=6.0, slope=512, depth_db=18.0, close_db=4.5, open_db=None,
                rise_db=0.05, fall_shift=1, floor_min_db=-100.0, smooth=True, out_floor=None, reseed=False, bias=None, knee=None, depth=None,
                close_step=None, open_step=None, rise=None, floor_min=None):
    """An enabled conan_denoise_cfg for a mel of the given log base (conan_mel_cfg.natural_log, .vmin, .eps).  bias_db: the floor is
    read this much higher; knee_db: the SNR under which a bin begins to close; slope: Q8 attenuation per step under the knee (512: 2 dB
    per dB); depth_db: the largest attenuation; close_db / open_db: its largest rise and fall per frame (open_db=None: the depth, a bin
    opens within the frame that needs it); rise_db: the floor's rise per frame; fall_shift: the floor falls by ceil(distance /
    2^fall_shift); floor_min_db: the floor's lowest level; smooth: the 1-2-1 average of the attenuation across bins; out_floor: the
    smallest value an attenuated bin takes (None: max(mel_vmin, log(eps)) in f32).  The defaults are choices, not measurements.
    Every decibel figure is converted once (denoise_level); the integer keywords (bias, knee, depth, close_step, open_step, rise,
    floor_min) give a field directly and win over their dB forms.  A field outside its range is a ValueError."""
    pick = lambda direct, db: denoise_level(db, natural_log) if direct is None else int(direct)      # noqa: E731
    step = lambda direct, db: max(1, denoise_level(db, natural_log)) if direct is None else int(direct)      # noqa: E731
    d = step(depth, depth_db)
    if out_floor is None:
        out_floor = max(float(mel_vmin), math.log(float(eps)) if natural_log else math.log10(float(eps)))
    c = DenoiseCfg(1, int(bool(reseed)), pick(bias, bias_db), pick(knee, knee_db), int(slope), d, step(close_step, close_db),
                   d if open_step is None and open_db is None else step(open_step, open_db), pick(rise, rise_db), int(fall_shift),
                   pick(floor_min, floor_min_db), int(bool(smooth)), float(out_floor), (C.c_int32 * 3)(0, 0, 0))
    for name, lo, hi in DENOISE_RANGES:
        if not lo <= getattr(c, name) <= hi:
            raise ValueError(f"denoise: {name} = {getattr(c, name)} is outside {lo} .. {hi}")
    if not math.isfinite(c.out_floor):
        raise ValueError(f"denoise: out_floor = {out_floor!r} is not finite")
    return c


def denoise_keywords(c):
    """denoise_cfg's keywords of an enabled DenoiseCfg in the integer forms that give the same fields back exactly: the form
    Streams.denoise reports a setting in."""
    return dict({name: int(getattr(c, name)) for name, _, _ in DENOISE_RANGES}, smooth=bool(c.smooth), out_floor=float(c.out_floor))


class WatermarkCfg(C.Structure):
    """conan_watermark_cfg (include/conan_hip.h)."""
    _fields_ = [("enabled", C.c_int32), ("reseed", C.c_int32), ("key", C.c_uint64), ("id", C.c_int32), ("gain", C.c_float), ("floor", C.c_float),
                ("reserved", C.c_int32 * 9)]


class WatermarkState(C.Structure):
    """conan_watermark_state (include/conan_hip.h): a row of Streams.watermark_state / Context.watermark_embed(state=True)."""
    _fields_ = [("pos", C.c_int64), ("env", C.c_float), ("reserved", C.c_int32)]


class WatermarkHit(C.Structure):
    """conan_watermark_hit (include/conan_hip.h): the detector's record of a row."""
    _fields_ = [("offset", C.c_int32), ("blocks", C.c_int32), ("peak", C.c_int64)]


class WatermarkResult(C.Structure):
    """conan_watermark_result (include/conan_hip.h): conan_watermark_decide's answer."""
    _fields_ = [("present", C.c_int32), ("id", C.c_int32), ("offset", C.c_int32), ("rotation", C.c_int32), ("blocks", C.c_int32), ("reserved", C.c_int32),
                ("marker_score", C.c_int64), ("z", C.c_double)]


WATERMARK_BLOCK = 2048
WATERMARK_THRESHOLD = 11.5      # CONAN_WATERMARK_THRESHOLD


def watermark_cfg(key=0, id=0, gain=0.1, floor=0.0, reseed=False):
    """An enabled conan_watermark_cfg.  key: the 64-bit key of the chip sequence; id: the 16 bits the mark carries; gain: the mark's
    amplitude under the causal peak envelope (0.1: -20 dB); floor: its smallest amplitude (0: digital silence stays digital silence).
    The defaults are choices, not measurements.  A field outside its range is a ValueError."""
    if not 0 <= int(key) < 1 << 64:
        raise ValueError(f"watermark: key = {key!r} is outside 0 .. 2^64 - 1")
    if not 0 <= int(id) <= 65535:
        raise ValueError(f"watermark: id = {id!r} is outside 0 .. 65535")
    for name, v in (("gain", gain), ("floor", floor)):
        if not (math.isfinite(float(v)) and 0.0 <= float(v) <= 1.0):
            raise ValueError(f"watermark: {name} = {v!r} is outside 0 .. 1")
    return WatermarkCfg(1, int(bool(reseed)), int(key), int(id), float(gain), float(floor), (C.c_int32 * 9)())


def watermark_keywords(c):
    """watermark_cfg's keywords of an enabled WatermarkCfg, which give the same fields back exactly: the form Streams.watermark
    reports a setting in."""
    return dict(key=int(c.key), id=int(c.id), gain=float(c.gain), floor=float(c.floor))


class ToneState(C.Structure):
    """conan_tone_state (include/conan_hip.h)."""
    _fields_ = [("cand", C.c_int32), ("run", C.c_int32), ("cur", C.c_int32), ("miss", C.c_int32), ("held", C.c_int32), ("sound", C.c_int32),
                ("level", C.c_int32), ("reserved", C.c_int32), ("events", C.c_int64), ("frames", C.c_int64)]


class ToneCfg(C.Structure):
    """conan_tone_cfg (include/conan_hip.h)."""
    _fields_ = [("mode", C.c_int32), ("reseed", C.c_int32), ("thr", C.c_int64), ("twist_fwd_q8", C.c_int32), ("twist_rev_q8", C.c_int32), ("sel", C.c_int32),
                ("share_q8", C.c_int32), ("on_frames", C.c_int32), ("off_frames", C.c_int32), ("min_frames", C.c_int32), ("step", C.c_int32),
                ("gain", C.c_float), ("reserved", C.c_int32), ("seed", ToneState)]


TONE_FULL = 1 << 20
TONE_HOP_MAX = 512
TONE_KEYS = "123A456B789C*0#D"      # frame digit d = 4 * row + column
TONE_FIELDS = ("thr", "twist_fwd_q8", "twist_rev_q8", "sel", "share_q8", "on_frames", "off_frames", "min_frames", "step")
TONE_SEED = dict(cand=-1, run=0, cur=-1, miss=0, held=0, sound=-1, level=0, events=0, frames=0)


def tone_cfg(regenerate=True, hop=320, level_db=-40.0, twist_db=(4.0, 8.0), sel=8, share=0.5, on_frames=2, off_frames=2, min_frames=3, ramp_ms=0.0,
             gain=0.125, seed=None, reseed=False, thr=None, twist_fwd_q8=None, twist_rev_q8=None, share_q8=None, step=None):
    """An enabled conan_tone_cfg: detect and regenerate (mode 2) or detect only (regenerate=False: mode 1).  level_db: the least level
    of each tone in dBFS at frames of `hop` samples (thr = (A hop / 8)^2, A = 32768 * 10^(level_db / 20)); twist_db: by how much the
    high tone may exceed the low one, and the low one the high one; sel: a group's peak over each of its other three; share: the
    pair's least share of the frame's energy; on_frames / off_frames / min_frames: the debounce in 20 ms frames; ramp_ms: the time
    the regenerated pair takes to full level, in steps of one frame (0: at once); gain: each regenerated tone's amplitude (0.125:
    -18 dBFS).  seed: a state dict (Streams.tone_state's) a restart begins from.  The integer keywords (thr, twist_fwd_q8,
    twist_rev_q8, share_q8, step) give a field directly and win over their other forms.  The defaults are choices: talk-off against
    real speech has not been measured."""
    if thr is None:
        thr = int(round((32768.0 * 10.0 ** (float(level_db) / 20.0) * int(hop) / 8.0) ** 2))
    q8 = lambda db: int(round(256.0 * 10.0 ** (float(db) / 10.0)))      # noqa: E731
    if step is None:
        step = TONE_FULL if float(ramp_ms) <= 20.0 else max(1, int(math.ceil(TONE_FULL * 20.0 / float(ramp_ms))))      # (the ramp is complete after ramp_ms / 20 frames)
    st = ToneState()
    for name, v in dict(TONE_SEED, **{k: v for k, v in (seed or {}).items() if k != "reserved"}).items():
        setattr(st, name, int(v))
    return ToneCfg(2 if regenerate else 1, int(bool(reseed)), int(thr), q8(twist_db[0]) if twist_fwd_q8 is None else int(twist_fwd_q8),
                   q8(twist_db[1]) if twist_rev_q8 is None else int(twist_rev_q8), int(sel), int(round(256.0 * float(share))) if share_q8 is None else int(share_q8),
                   int(on_frames), int(off_frames), int(min_frames), int(step), float(gain), 0, st)


def tone_keywords(c):
    """tone_cfg's keywords of an enabled ToneCfg in the integer forms that give the same fields back exactly: the form Streams.tones
    reports a setting in."""
    return dict({name: int(getattr(c, name)) for name in TONE_FIELDS}, regenerate=c.mode == 2, gain=float(c.gain),
                seed={name: int(getattr(c.seed, name)) for name in TONE_SEED})


def tone_events(digit_rows):
    """Per row of per-frame digits (Streams.step_wav_tones' / Context.tones', the calls' rows of a slot joined in time; -1: none) the
    key presses [(key, first frame, frames)], keys from '123A456B789C*0#D': what a host sends as RFC 4733 events, 20 ms per frame.
    A digit still held in the last frame is reported with the frames seen so far.  A single row (a 1-D array, tensor or list of
    integers) gives one list, rows (2-D, or a list of rows of their own lengths) a list per row.  Host only: tensors on the CPU."""
    single = len(digit_rows) > 0 and not isinstance(digit_rows[0], (list, tuple)) and getattr(digit_rows[0], "ndim", 0) == 0
    out = []
    for row in ([digit_rows] if single else digit_rows):
        ev, prev, start = [], -1, 0
        for f, d in enumerate([int(v) for v in row] + [-1]):
            if d != prev:
                if prev >= 0:
                    ev.append((TONE_KEYS[prev], start, f - start))
                prev, start = d, f
        out.append(ev)
    return out[0] if single else out


class EqCfg(C.Structure):
    """conan_eq_cfg (include/conan_hip.h)."""
    _fields_ = [("enabled", C.c_int32), ("sections", C.c_int32), ("origin", C.c_int64), ("pos", C.c_int64), ("coef", (C.c_double * 5) * 4),
                ("reserved", C.c_int32 * 4)]


class EqState(C.Structure):
    """conan_eq_state (include/conan_hip.h)."""
    _fields_ = [("origin", C.c_int64), ("pos", C.c_int64), ("carry", (C.c_double * 2) * 4), ("tail", C.c_float * 128)]


EQ_MAX_SECTIONS, EQ_SEG, EQ_MAX_COEF = 4, 128, 65536.0
EQ_KINDS = {"lowpass": 0, "highpass": 1, "bandpass": 2, "notch": 3, "peak": 4, "lowshelf": 5, "highshelf": 6, "dcblock": 7, "deemphasis": 8}


def eq_section(kind, rate, f, q=0.7071067811865476, gain_db=0.0):
    """conan_eq_design, the one implementation of the design formulas: the section {b0, b1, b2, a1, a2} / a0 of `kind` (a key of
    EQ_KINDS) at `rate` Hz with corner or centre f, quality q and - peak and shelves - gain_db, as a tuple of five floats.  Host
    only: no device is needed."""
    if kind not in EQ_KINDS:
        raise ValueError("eq section kind must be one of %s, got %r" % (sorted(EQ_KINDS), kind))
    out = (C.c_double * 5)()
    check(lib().conan_eq_design(EQ_KINDS[kind], float(rate), float(f), float(q), float(gain_db), out))
    return tuple(float(v) for v in out)


def eq_cfg(sections=None, rate=None, origin=0, pos=None):
    """An enabled conan_eq_cfg of 1 .. 4 sections.  A section is a raw 5-tuple (b0, b1, b2, a1, a2), normalised by a0 and taken as
    given, or a dict(kind=, f=, q=, gain_db=) that eq_section designs at `rate` Hz (the rate of the audio the cascade filters: a
    slot's model rate).  origin / pos: the grid's origin and the position of the first sample, for a row that continues a seed
    record (pos defaults to origin: a row that starts from zero).  Any example cascade is a choice: nobody has listened to one."""
    secs = list(sections or ())
    if not 1 <= len(secs) <= EQ_MAX_SECTIONS:
        raise ValueError(f"eq_cfg: 1 .. {EQ_MAX_SECTIONS} sections, got {len(secs)}")
    c = EqCfg()
    c.enabled, c.sections, c.origin, c.pos = 1, len(secs), int(origin), int(origin if pos is None else pos)
    for k, sec in enumerate(secs):
        if isinstance(sec, dict):
            if rate is None:
                raise ValueError("eq_cfg: a section given as a dict needs the rate of the audio it filters")
            sec = eq_section(rate=rate, **sec)
        if len(sec) != 5:
            raise ValueError("eq_cfg: a raw section is (b0, b1, b2, a1, a2)")
        for i, v in enumerate(sec):
            c.coef[k][i] = float(v)
    return c


def eq_keywords(c):
    """eq_cfg's keywords of an enabled EqCfg, the sections as raw 5-tuples: the form that gives the same bytes back."""
    return dict(sections=[tuple(float(c.coef[k][i]) for i in range(5)) for k in range(int(c.sections))], origin=int(c.origin), pos=int(c.pos))


class SlotFeature(typing.NamedTuple):
    """One per-slot feature of a stream-set, as Streams and the engine read it.  A symbol the library does not have is None."""
    keyword: str                  # the engine's keyword (start_wav, open_slots, ...)
    noun: str                     # "cfg=None turns {noun} off and takes no keywords"; None: such a call is accepted
    cfg: type                     # the Cfg struct; zeroed, it is "off"
    on: str                       # the struct's field that says "on": 'enabled' or 'mode'
    build: typing.Callable        # keywords -> an enabled struct
    keywords: typing.Callable     # an enabled struct -> the keywords it is reported in
    setter: str                   # (h, slots, n, cfg [, seed rows, stride] [, stream])
    getter: str = None            # (h, slot, cfg)
    state: str = None             # (h, slots, n, rows, stream)
    rows: object = None           # what `state` fills: a State struct (rows read as dicts) or (dtype, columns) of a numeric tensor
    seed_state: str = None        # (h, slots, n, rows, bytes, stream): opaque rows, which the setter takes back as seed rows with a stride
    seed_bytes: str = None        # the bytes of such a row
    last: str = None              # the rows of the last wav-in call
    meta: str = None              # (slot meta, cfg): the setting in a slot snapshot's host record
    stream: bool = True           # the setter takes a stream (and joins pipelined work: the buffers in flight are released)
    release: bool = True          # ... unless the setter leaves them alone
    mirror: str = None            # the Streams dict slot -> keywords, for the features that keep one
    engine_own: bool = False      # the engine applies it itself, by rules of its own (echo_delay=), not as one of the table's keywords

    @property
    def method(self):
        """The name of Streams' setter."""
        return self.setter[len("conan_streams_"):]


# in the order open_slots applies them (echo_delay: behind them all, by the engine's own rules)
SLOT_FEATURES = {f.keyword: f for f in (
    SlotFeature("eq", "the equaliser", EqCfg, "enabled", eq_cfg, eq_keywords, "conan_streams_set_input_eq", "conan_streams_input_eq",
                seed_state="conan_streams_input_eq_state", seed_bytes="conan_eq_state_bytes"),
    SlotFeature("level", "the leveller", LevelCfg, "enabled", level_cfg, level_keywords, "conan_streams_set_input_level",
                state="conan_streams_input_level", rows=("float64", 4), meta="conan_slot_meta_level", stream=False, release=False,
                mirror="input_levels"),
    SlotFeature("pitch", "the pitch control", PitchCfg, "enabled", pitch_cfg, pitch_keywords, "conan_streams_set_pitch", "conan_streams_pitch",
                meta="conan_slot_meta_pitch", mirror="pitch_cfgs"),
    SlotFeature("follow", "following", F0Cfg, "enabled", f0_cfg, f0_keywords, "conan_streams_set_pitch_follow", "conan_streams_pitch_follow",
                last="conan_step_wav_contour"),
    SlotFeature("register", None, RegisterCfg, "enabled", register_cfg, register_keywords, "conan_streams_set_pitch_register",
                "conan_streams_pitch_register", "conan_streams_pitch_register_state", ("int64", 2)),
    SlotFeature("activity", "the detector", ActivityCfg, "mode", activity_cfg, activity_keywords, "conan_streams_set_activity",
                "conan_streams_activity", "conan_streams_activity_state", ActivityState, last="conan_step_wav_activity"),
    SlotFeature("bypass", None, BypassCfg, "enabled", bypass_cfg, bypass_keywords, "conan_streams_set_bypass", "conan_streams_bypass",
                "conan_streams_bypass_state", BypassState, last="conan_step_wav_bypass"),
    SlotFeature("conceal", "the concealment", ConcealCfg, "enabled", conceal_cfg, conceal_keywords, "conan_streams_set_conceal",
                "conan_streams_conceal_cfg", seed_state="conan_streams_conceal_state", seed_bytes="conan_conceal_state_bytes"),
    SlotFeature("echo", "the echo canceller", EchoCfg, "enabled", echo_cfg, echo_keywords, "conan_streams_set_echo",
                "conan_streams_echo_cfg", seed_state="conan_streams_echo_state", seed_bytes="conan_echo_state_bytes"),
    SlotFeature("denoise", "the noise suppression", DenoiseCfg, "enabled", denoise_cfg, denoise_keywords, "conan_streams_set_denoise",
                "conan_streams_denoise", seed_state="conan_streams_denoise_state", seed_bytes="conan_denoise_state_bytes"),
    SlotFeature("comfort", "the comfort noise", ComfortCfg, "mode", comfort_cfg, comfort_keywords, "conan_streams_set_comfort",
                "conan_streams_comfort", "conan_streams_comfort_state", ComfortState, last="conan_step_wav_comfort"),
    SlotFeature("tones", "the tone detector", ToneCfg, "mode", tone_cfg, tone_keywords, "conan_streams_set_tones", "conan_streams_tones",
                "conan_streams_tone_state", ToneState, last="conan_step_wav_tones"),
    SlotFeature("echo_delay", "the estimator", EchoDelayCfg, "enabled", echo_delay_cfg, echo_delay_keywords, "conan_streams_set_echo_delay",
                "conan_streams_echo_delay_cfg", seed_state="conan_streams_echo_delay_state", seed_bytes="conan_echo_delay_state_bytes",
                engine_own=True),
    SlotFeature("out_eq", "the equaliser", EqCfg, "enabled", eq_cfg, eq_keywords, "conan_streams_set_output_eq", "conan_streams_output_eq",
                seed_state="conan_streams_output_eq_state", seed_bytes="conan_eq_state_bytes"),
    SlotFeature("out_level", "the leveller", LevelCfg, "enabled", level_cfg, level_keywords, "conan_streams_set_output_level",
                "conan_streams_output_level_cfg", "conan_streams_output_level", ("float64", 4), "conan_streams_output_level_state",
                "conan_streams_output_level_state_bytes", release=False, mirror="output_levels"),
    SlotFeature("watermark", "the watermark", WatermarkCfg, "enabled", watermark_cfg, watermark_keywords, "conan_streams_set_watermark",
                "conan_streams_watermark", seed_state="conan_streams_watermark_state", seed_bytes="conan_watermark_state_bytes"),
)}

for _f in SLOT_FEATURES.values():      # the three regular families of _PROTOS: a symbol's shape is stated once, in SlotFeature
    _PROTOS[_f.setter] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_void_p, C.c_int64] * bool(_f.seed_state) + [C.c_void_p] * _f.stream)
    if _f.getter:
        _PROTOS[_f.getter] = (C.c_int, [C.c_void_p, C.c_int, C.c_void_p])
    if _f.state:
        _PROTOS[_f.state] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p])
    if _f.seed_state:
        _PROTOS[_f.seed_state] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p])


class DecoderTaps(C.Structure):
    """conan_decoder_taps (include/conan_hip.h)."""
    _fields_ = [("uv_pred", C.c_void_p), ("f0_denorm_pred", C.c_void_p), ("pitch_bins", C.c_void_p), ("decoder_inp", C.c_void_p),
                ("content_embed_proj", C.c_void_p), ("attn", C.c_void_p * 2)]


class HifiganTaps(C.Structure):
    """conan_hifigan_taps (include/conan_hip.h)."""
    _fields_ = [("conv_pre_act", C.c_void_p), ("ups", C.c_void_p * MAX_UPS), ("stage_out", C.c_void_p * MAX_UPS)]


def make_cfg(conan_hp=None, hifigan_hp=None, emformer=True, conan=True, hifigan=True):
    """conan_cfg from the reference's hparams dicts (utils/commons/hparams.py)."""
    c = ConanCfg()
    c.abi_version = ABI_VERSION
    models = 0
    hp = conan_hp or {}
    if conan_hp is not None and conan:
        models |= MODEL_CONAN
        if hp.get("decoder_type", "conv") != "conv" or hp.get("f0_gen", "orig") != "orig" or not hp.get("style", True):
            raise ConanError(ERR_UNSUPPORTED, "only decoder_type='conv', f0_gen='orig', style=true (egs/conan_emformer.yaml) is on the hot path")
        c.hidden_size = hp["hidden_size"]
        c.content_vocab = 102
        c.content_kernel = hp["kernel_size"]
        c.dec_kernel = hp["dec_kernel_size"]
        dd = list(hp["dec_dilations"])
        c.dec_num_blocks = len(dd)
        for i, d in enumerate(dd):
            c.dec_dilations[i] = d
        c.dec_layers_in_block = hp["layers_in_block"]
        c.dec_post_kernel = hp.get("dec_post_net_kernel", 3)
        c.predictor_kernel = hp["predictor_kernel"]
        c.nvq = hp["nVQ"]
        c.silent_token = hp["silent_token"]
    c.num_mels = (conan_hp or hifigan_hp or {}).get("audio_num_mel_bins", 80)
    if conan_hp is not None and emformer:
        models |= MODEL_EMFORMER
        c.emf_input_dim = 80
        c.emf_heads = 8
        c.emf_ffn_dim = 2048
        c.emf_layers = hp["emformer_layers"]
        c.emf_segment = hp["chunk_size"] // 20
        c.emf_left_context = 50
        c.emf_right_context = hp["right_context"]
        # mode == 'both': the streaming loop projects with proj1 (80 -> 100), inference/Conan.py:117-118
        c.emf_output_dim = 100 if hp.get("mode", None) == "both" else hp.get("emformer_output_dim", 100)
        # not a key of the reference's yaml files (modules/Emformer/emformer.py:14-22 leaves torchaudio's defaults, 0 /
        # False); read when present so that the memory bank can be exercised
        c.emf_max_memory_size = int(hp.get("emformer_max_memory_size", 0))
        c.emf_tanh_on_mem = int(bool(hp.get("emformer_tanh_on_mem", False)))
    if hifigan_hp is not None and hifigan:
        v = hifigan_hp
        up = v.get("upsample", "shuffle")
        if up not in ("shuffle", "zero", "nn"):
            raise ConanError(ERR_UNSUPPORTED, "upsample='%s': 'shuffle', 'zero' or 'nn' (hifigan_causal.py:287-293)" % up)
        c.voc_upsample = {"shuffle": 0, "zero": 1, "nn": 2}[up]
        c.voc_resblock = 1 if str(v.get("resblock", "1")) == "1" else 2
        if len({len(ds) for ds in v["resblock_dilation_sizes"]}) != 1:
            raise ConanError(ERR_UNSUPPORTED, "resblock branches with different numbers of dilations")
        models |= MODEL_HIFIGAN
        c.voc_initial_channel = v.get("upsample_initial_channel", 512)
        c.voc_num_ups = len(v["upsample_rates"])
        for i, (r, k) in enumerate(zip(v["upsample_rates"], v["upsample_kernel_sizes"])):
            c.voc_up_rates[i] = r
            c.voc_up_kernels[i] = k
        c.voc_num_resblocks = len(v["resblock_kernel_sizes"])
        c.voc_rb_num_dil = len(v["resblock_dilation_sizes"][0])
        for b, (k, ds) in enumerate(zip(v["resblock_kernel_sizes"], v["resblock_dilation_sizes"])):
            c.voc_rb_kernels[b] = k
            for j, d in enumerate(ds):
                c.voc_rb_dilations[b][j] = d
    c.models = models
    return c
