"""whisper.tflite_amd — Python host mirror of the reference engine interface over the C ABI.

The product is the native library ``lib/libwhisper-tflite.so`` (hand-written gfx950
kernels behind ``include/wt_capi.h``).  This module only binds it with ctypes so that
tests, ``bench.py`` and ``__graft_entry__.py`` can drive it; it contains no compute and no
fallback: if the library is missing or no MI355X is present, calls fail loudly.

Interface mirrored (reference jerinphilip/whisper.tflite @ v2):
  * ``Engine.transcribe(samples)`` / ``Engine.transcribe(path)``  — whisper.h:159-163
  * ``create_engine(EngineType, model_prefix, vocab_path, multilingual)`` — whisper.h:259-260
  * ``EngineType`` — whisper.h:199-204

The directory is named like the reference's ``whisper.tflite/`` source directory, so it is
not importable with a plain ``import`` statement; load it with
``__graft_entry__.load_package()`` (importlib by path).
"""
from __future__ import annotations

import ctypes
import enum
import os
import types
from ctypes import (POINTER, byref, c_char_p, c_float, c_int, c_int32, c_int64, c_long, c_size_t,
                    c_uint64, c_void_p)

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WT_LIB_PATH") or os.path.join(_HERE, "lib", "libwhisper-tflite.so")  # WT_LIB_PATH: A/B runs of two builds

WT_OK = 0
WT_MAX_IDS = 32
WT_PIPELINE_DEPTH = 24  # include/wt_capi.h
WT_LANGUAGE_AUTO = -1  # option "language": detected per clip
CHUNK_SAMPLES = 480000
STATUS_NAMES = {0: "WT_OK", 1: "WT_ERR_INVALID_ARG", 2: "WT_ERR_IO", 3: "WT_ERR_FORMAT",
                4: "WT_ERR_UNSUPPORTED", 5: "WT_ERR_DEVICE", 6: "WT_ERR_BUFFER"}

# Every symbol include/wt_capi.h and include/wt_debug.h declare.
CAPI_SYMBOLS = [
    "wt_device_alloc", "wt_device_free", "wt_device_upload", "wt_device_download", "wt_device_synchronize",
    "wt_engine_create", "wt_engine_destroy", "wt_last_error", "wt_engine_dims",
    "wt_engine_set_option", "wt_engine_get_option", "wt_engine_set_prompt", "wt_engine_set_context", "wt_engine_set_contexts", "wt_engine_set_suppress", "wt_vocab_default_suppress", "wt_transcribe_pcm", "wt_transcribe_long_pcm", "wt_transcribe_file",
    "wt_logmel_batch", "wt_logmel_batch_dev", "wt_encdec_tokens_batch",
    "wt_encdec_tokens_batch_dev", "wt_transcribe_tokens_batch_dev", "wt_pipeline_submit_dev", "wt_pipeline_submit_pcm_dev", "wt_pipeline_collect",
    "wt_encdec_debug_batch",
    "wt_encdec_tokens_full_batch", "wt_encdec_tokens_full_batch_dev", "wt_transcribe_tokens_full_batch_dev",
    "wt_last_segments", "wt_last_segment_text", "wt_vocab_segments", "wt_vocab_seek_step", "wt_last_windows",
    "wt_transcribe_long_batch", "wt_last_file_text", "wt_last_window_files",
    "wt_vocab_split_words", "wt_vocab_merge_punctuation", "wt_dtw_path",
    "wt_engine_set_alignment_heads", "wt_last_words", "wt_last_word_text",
    "wt_last_scores", "wt_last_token_logprobs", "wt_last_segment_scores", "wt_last_decode_info", "wt_last_best_of",
    "wt_language_count", "wt_detect_language_batch", "wt_detect_language_batch_dev", "wt_detect_language_pcm", "wt_last_languages",
    "wt_engine_set_language_candidates",
    "wt_last_timings", "wt_last_beam_scores", "wt_last_kernel_stats", "wt_decode_text", "wt_language_id", "wt_lang_code", "wt_wav_read_legacy",
    "wt_vocab_info", "wt_filters", "wt_write_synthetic_weights", "wt_write_synthetic_vocab",
    "wt_vocab_open", "wt_vocab_close", "wt_vocab_get_info", "wt_vocab_get_filters", "wt_vocab_size", "wt_vocab_token",
    "wt_vocab_decode", "wt_log_mel_spectrogram", "wt_convert_tflite", "wt_shutdown",
]
DEBUG_SYMBOLS = [
    "wt_dbg_cross_absorbed", "wt_dbg_cross_absorbed_bf16", "wt_dbg_gemm_planes_ln", "wt_dbg_gemm", "wt_dbg_gemm_bench", "wt_dbg_dec_gemm_bench", "wt_dbg_dec_gemm", "wt_dbg_dec_ln_gemm", "wt_dbg_layernorm", "wt_dbg_encoder_attention",
    "wt_dbg_cross_attention", "wt_dbg_self_attention", "wt_dbg_interference", "wt_dbg_concurrency",
    "wt_dbg_gemm_planes", "wt_dbg_set_plane_gemm_mode", "wt_dbg_set_forced_ids", "wt_dbg_dec_gemm_bf16", "wt_dbg_dec_ln_gemm_bf16",
    "wt_dbg_self_attention_bf16", "wt_dbg_cross_attention_bf16", "wt_dbg_encoder_attention_planes", "wt_dbg_gemm_bf16", "wt_dbg_gemm_bf16_ln", "wt_dbg_encoder_attention_bf16",
    "wt_dbg_beam_topk", "wt_dbg_beam_step", "wt_dbg_beam_reorder", "wt_dbg_beam_finalize",
    "wt_dbg_beam_full_step", "wt_dbg_beam_full_finalize",
    "wt_dbg_dec_gemm_ksplit", "wt_dbg_dec_ln_gemm_rows", "wt_dbg_dec_logits", "wt_dbg_select_token",
    "wt_dbg_cross_absorbed_chain", "wt_dbg_absorbed_query_matrix", "wt_dbg_language_head", "wt_dbg_language_head_rows", "wt_dbg_self_attention_long",
    "wt_dbg_self_attention_prefill", "wt_dbg_self_attention_long_gather",
    "wt_dbg_self_attention_long_bf16", "wt_dbg_self_attention_long_gather_bf16", "wt_dbg_self_attention_prefill_bf16",
    "wt_dbg_self_attention_long_ragged", "wt_dbg_self_attention_prefill_ragged", "wt_dbg_dec_ln_gemm_ragged", "wt_dbg_ragged_cap",
    "wt_dbg_timestamp_select", "wt_dbg_token_scores", "wt_dbg_sample_select", "wt_dbg_suppress_logits",
    "wt_dbg_sample_select_group", "wt_dbg_best_of_begin", "wt_dbg_best_of_pick",
    "wt_dbg_frontend_dims", "wt_dbg_frontend_stages", "wt_dbg_log_clipmax", "wt_dbg_mel_normalize", "wt_dbg_mel_transpose",
    "wt_dbg_pcm_to_planes",
    "wt_dbg_gemm_addressed", "wt_dbg_plane_gemm_plan", "wt_dbg_gemm_ln_fused", "wt_dbg_layernorm_planes", "wt_dbg_f32_to_planes", "wt_dbg_encoder_attention_at",
    "wt_dbg_encoder_scales", "wt_dbg_f16_scale_for", "wt_dbg_gemm_planes_scaled",
    "wt_dbg_cross_attention_records", "wt_dbg_cross_attention_records_bf16", "wt_dbg_cross_combine", "wt_dbg_cross_combine_bf16",
    "wt_dbg_self_attention_long_ragged_bf16", "wt_dbg_self_attention_prefill_ragged_bf16", "wt_dbg_align_scores_bf16",
    "wt_dbg_f32_to_bf16",
    "wt_dbg_align_scores", "wt_dbg_align_matrix", "wt_dbg_align_dtw", "wt_dbg_last_alignment", "wt_dbg_set_alignment",
]


class BeamFullArgs(ctypes.Structure):
    """wt_dbg_beam_full_args (include/wt_debug.h)."""
    _SCALARS = ("K", "clips", "c0", "pos", "n_prompt", "V", "ldl", "stride", "cap", "eot", "beg", "max_initial", "timestamps",
                "begin")
    _ARRAYS = (("logits", np.float32), ("ids", np.int64), ("lp", np.float32), ("anc", np.uint8), ("ts_state", np.int32),
               ("n_live", np.int32), ("live_sum", np.float64), ("fin_tok", np.int32), ("fin_lp", np.float32),
               ("fin_sum", np.float64), ("fin_len", np.int32), ("n_fin", np.int32), ("done", np.int32), ("parent", np.int32),
               ("token", np.int64), ("tok_lp", np.float32), ("ids_next", np.int64), ("lp_next", np.float32),
               ("anc_next", np.uint8), ("lse", np.float64), ("part_stats", np.float32), ("part_keys", np.uint64),
               ("out_ids", np.int64), ("out_lp", np.float32), ("out_n", np.int32), ("out_len", np.int32),
               ("out_sum", np.float64))
    _fields_ = [(n, c_int32) for n in _SCALARS] + [(n, c_void_p) for n, _ in _ARRAYS]


def beam_full_state(stride):
    """The per-clip state of a full-length beam chain as decode_beam_full keeps it, before beam_full_begin."""
    return {"ts_state": np.zeros((128, 3), np.int32), "n_live": np.zeros(64, np.int32), "live_sum": np.zeros((64, 8), np.float64),
            "fin_tok": np.zeros((64, 8, stride), np.int32), "fin_lp": np.zeros((64, 8, stride), np.float32),
            "fin_sum": np.zeros((64, 8), np.float64), "fin_len": np.zeros((64, 8), np.int32), "n_fin": np.zeros(64, np.int32),
            "done": np.zeros(64, np.int32)}


class WtError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"{STATUS_NAMES.get(code, code)}: {message}")
        self.code = code


class EngineType(enum.IntEnum):
    Monolith = 0
    EncDec = 1


class Dims(ctypes.Structure):
    _fields_ = [(n, c_int32) for n in (
        "n_mels", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer",
        "n_vocab", "n_text_ctx", "n_text_state", "n_text_head", "n_text_layer")]


class Timings(ctypes.Structure):
    _fields_ = [("logmel_ms", c_float), ("encoder_ms", c_float), ("cross_kv_ms", c_float),
                ("decoder_ms", c_float), ("total_ms", c_float), ("batch", c_int32),
                ("decoder_steps", c_int32)]


class KernelStat(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 48), ("launches", c_int32), ("reserved", c_int32),
                ("ms", ctypes.c_double), ("flops", ctypes.c_double), ("bytes", ctypes.c_double)]


_lib = None


def lib() -> ctypes.CDLL:
    """Loads the native library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `make lib` (or __graft_entry__.build()); "
                "there is no Python/CPU fallback for the engine")
        L = ctypes.CDLL(LIB_PATH)
        fp, ip64, ip32 = POINTER(c_float), POINTER(c_int64), POINTER(c_int32)
        L.wt_engine_create.argtypes = [c_int, c_char_p, c_char_p, c_int, c_int, POINTER(c_void_p)]
        L.wt_engine_destroy.argtypes = [c_void_p]
        L.wt_engine_destroy.restype = None
        L.wt_last_error.argtypes = [c_void_p]
        L.wt_last_error.restype = c_char_p
        L.wt_engine_dims.argtypes = [c_void_p, POINTER(Dims)]
        L.wt_engine_set_option.argtypes = [c_void_p, c_char_p, c_long]
        L.wt_engine_get_option.argtypes = [c_void_p, c_char_p, POINTER(c_long)]
        L.wt_engine_set_prompt.argtypes = [c_void_p, ip64, c_int]
        L.wt_engine_set_context.argtypes = [c_void_p, ip64, c_int]
        L.wt_engine_set_contexts.argtypes = [c_void_p, ip64, ip32, c_int]
        L.wt_engine_set_suppress.argtypes = [c_void_p, ip64, c_int, ip64, c_int]
        L.wt_engine_set_language_candidates.argtypes = [c_void_p, ip32, c_int]
        L.wt_vocab_default_suppress.argtypes = [c_void_p, ip64, c_int, ip32, ip64, c_int, ip32]
        L.wt_dbg_suppress_logits.argtypes = [c_void_p, c_int, c_int, c_int, fp, fp, ip64, c_int, ip64, c_int, c_int]
        L.wt_transcribe_long_batch.argtypes = [c_void_p, POINTER(fp), POINTER(c_size_t), c_int]
        L.wt_last_file_text.argtypes = [c_void_p, c_int, c_char_p, c_size_t, POINTER(c_size_t)]
        L.wt_last_window_files.argtypes = [c_void_p, ip32, c_int]
        L.wt_transcribe_pcm.argtypes = [c_void_p, fp, c_size_t, c_char_p, c_size_t, POINTER(c_size_t)]
        L.wt_transcribe_long_pcm.argtypes = [c_void_p, fp, c_size_t, c_char_p, c_size_t, POINTER(c_size_t)]
        L.wt_transcribe_file.argtypes = [c_void_p, c_char_p, c_char_p, c_size_t, POINTER(c_size_t)]
        L.wt_logmel_batch.argtypes = [c_void_p, fp, c_int, fp]
        L.wt_logmel_batch_dev.argtypes = [c_void_p, c_void_p, c_int, c_void_p]
        L.wt_encdec_tokens_batch.argtypes = [c_void_p, fp, c_int, ip64, ip32]
        L.wt_encdec_tokens_batch_dev.argtypes = [c_void_p, c_void_p, c_int, ip64, ip32]
        L.wt_transcribe_tokens_batch_dev.argtypes = [c_void_p, c_void_p, c_int, ip64, ip32]
        L.wt_pipeline_submit_dev.argtypes = [c_void_p, c_void_p, c_int]
        L.wt_pipeline_submit_pcm_dev.argtypes = [c_void_p, c_void_p, c_int]
        L.wt_pipeline_collect.argtypes = [c_void_p, ip64, ip32]
        L.wt_encdec_debug_batch.argtypes = [c_void_p, fp, c_int, ip64, ip32, fp, fp, c_int]
        L.wt_last_timings.argtypes = [c_void_p, POINTER(Timings)]
        L.wt_last_beam_scores.argtypes = [c_void_p, fp, ip32, c_int]
        L.wt_last_kernel_stats.argtypes = [c_void_p, POINTER(KernelStat), c_int]
        L.wt_decode_text.argtypes = [c_void_p, ip64, c_int, c_int, c_char_p, c_size_t, POINTER(c_size_t)]
        L.wt_language_id.argtypes = [c_char_p]
        L.wt_lang_code.argtypes = [c_int]
        L.wt_lang_code.restype = c_char_p
        L.wt_wav_read_legacy.argtypes = [c_char_p, fp, c_size_t, POINTER(c_size_t)]
        L.wt_vocab_info.argtypes = [c_void_p, ip32]
        L.wt_filters.argtypes = [c_void_p, fp, c_size_t, ip32, ip32]
        L.wt_write_synthetic_weights.argtypes = [c_char_p, c_char_p, c_uint64]
        L.wt_write_synthetic_vocab.argtypes = [c_char_p, c_int]
        L.wt_vocab_open.argtypes = [c_char_p, c_int, POINTER(c_void_p)]
        L.wt_vocab_close.argtypes = [c_void_p]
        L.wt_vocab_close.restype = None
        L.wt_vocab_get_info.argtypes = [c_void_p, ip32]
        L.wt_vocab_get_filters.argtypes = [c_void_p, fp, c_size_t, ip32, ip32]
        L.wt_vocab_size.argtypes = [c_void_p]
        L.wt_vocab_token.argtypes = [c_void_p, c_int, c_char_p, c_size_t, POINTER(c_size_t)]
        L.wt_vocab_decode.argtypes = [c_void_p, ip64, c_int, c_int, c_char_p, c_size_t, POINTER(c_size_t)]
        L.wt_log_mel_spectrogram.argtypes = [fp, c_int, fp, c_int, c_int, c_int, fp, c_size_t, POINTER(c_int)]
        L.wt_convert_tflite.argtypes = [c_char_p, c_char_p]
        L.wt_dbg_gemm.argtypes = [c_void_p, c_int, c_int, c_int, fp, fp, fp, fp, fp, c_int, c_int, fp]
        L.wt_dbg_gemm_planes.argtypes = [c_void_p, c_int, c_int, c_int, fp, fp, fp, fp, fp, c_int, c_int, c_int, c_int, fp,
                                         POINTER(c_float), c_int]
        L.wt_dbg_encoder_attention_planes.argtypes = [c_void_p, c_int, c_int, c_int, fp, c_int, fp, POINTER(c_float)]
        L.wt_dbg_cross_absorbed.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, fp, fp, fp, fp, fp, c_int, POINTER(c_float)]
        L.wt_dbg_cross_absorbed_bf16.argtypes = L.wt_dbg_cross_absorbed.argtypes
        L.wt_dbg_cross_absorbed_chain.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(fp),
                                                  fp, fp, fp, c_int, c_int, c_int, fp, fp]
        L.wt_dbg_absorbed_query_matrix.argtypes = [c_int, c_int, fp, fp, fp, fp, fp]
        L.wt_dbg_gemm_planes_ln.argtypes = [c_void_p, c_int, c_int, fp, fp, fp, fp, fp, c_int, c_int, fp, fp, c_int, fp, fp, fp,
                                            POINTER(c_int)]
        L.wt_dbg_gemm_bf16.argtypes = [c_void_p, c_int, c_int, c_int, fp, fp, fp, fp, fp, c_int, c_int, c_int, c_int, fp,
                                       POINTER(c_float)]
        L.wt_dbg_encoder_attention_bf16.argtypes = [c_void_p, c_int, c_int, c_int, fp, c_int, fp, POINTER(c_float)]
        L.wt_dbg_gemm_bf16_ln.argtypes = [c_void_p, c_int, c_int, c_int, fp, fp, fp, fp, fp, fp, fp, fp, fp, POINTER(c_int)]
        L.wt_dbg_gemm_bench.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_float)]
        L.wt_dbg_dec_gemm_bench.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_float)]
        L.wt_dbg_dec_gemm.argtypes = [c_void_p, c_int, c_int, c_int, c_int, fp, fp, fp, fp, fp, ip64]
        L.wt_dbg_dec_ln_gemm.argtypes = [c_void_p, c_int, c_int, c_int, fp, ip64, c_int, fp, fp,
                                         c_int, c_int, fp, fp, fp, fp, c_int, fp, fp]
        L.wt_dbg_layernorm.argtypes = [c_void_p, c_int, c_int, fp, fp, fp, fp]
        L.wt_device_alloc.argtypes = [c_void_p, ctypes.c_size_t, POINTER(c_void_p)]
        L.wt_device_free.argtypes = [c_void_p, c_void_p]
        L.wt_device_upload.argtypes = [c_void_p, c_void_p, ctypes.c_size_t, c_void_p, ctypes.c_size_t]
        L.wt_device_download.argtypes = [c_void_p, c_void_p, c_void_p, ctypes.c_size_t, ctypes.c_size_t]
        L.wt_device_synchronize.argtypes = [c_void_p]
        L.wt_dbg_set_forced_ids.argtypes = [c_void_p, POINTER(c_int64), c_int]
        L.wt_dbg_dec_gemm_bf16.argtypes = L.wt_dbg_dec_gemm.argtypes
        L.wt_dbg_dec_ln_gemm_bf16.argtypes = L.wt_dbg_dec_ln_gemm.argtypes
        L.wt_dbg_encoder_attention.argtypes = [c_void_p, c_int, c_int, c_int, fp, fp]
        L.wt_dbg_cross_attention.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, fp, fp, fp, fp, fp, fp, fp, fp]
        L.wt_dbg_self_attention.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, fp, fp, fp, fp]
        L.wt_dbg_self_attention_bf16.argtypes = L.wt_dbg_self_attention.argtypes
        L.wt_dbg_cross_attention_bf16.argtypes = L.wt_dbg_cross_attention.argtypes
        L.wt_dbg_cross_attention_records.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, fp, fp, fp, fp, fp, fp, fp,
                                                     c_int, c_int, fp]
        L.wt_dbg_cross_attention_records_bf16.argtypes = L.wt_dbg_cross_attention_records.argtypes
        L.wt_dbg_cross_combine.argtypes = [c_void_p, c_int, c_int, c_int, c_int, fp, fp, fp, fp, c_int, fp]
        L.wt_dbg_cross_combine_bf16.argtypes = L.wt_dbg_cross_combine.argtypes
        u64p = POINTER(c_uint64)
        L.wt_dbg_beam_topk.argtypes = [c_void_p, c_int, c_int, c_int, c_int, fp, fp, fp, u64p]
        L.wt_dbg_beam_step.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int64, fp, ip64, fp, ip32,
                                       fp, ip32, ip32, ip32, ip32, ip64, ip64]
        L.wt_dbg_beam_reorder.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, fp, fp, ip64, ip64, ip32,
                                          ip64]
        L.wt_dbg_beam_finalize.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, ip64, fp, ip32, fp, ip32, ip32, ip32,
                                           ip64, ip32, fp, ip32]
        L.wt_dbg_dec_gemm_ksplit.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, fp, fp, fp, fp, fp, fp]
        L.wt_dbg_dec_ln_gemm_rows.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, fp, fp, ip64, c_int, c_int, fp, fp,
                                              c_int, c_int, fp, fp, fp, fp, c_int, fp, fp]
        L.wt_dbg_dec_logits.argtypes = [c_void_p, c_int, c_int, c_int, c_int, fp, fp, fp, fp, fp, c_int, fp, u64p]
        L.wt_dbg_select_token.argtypes = [c_void_p, c_int, c_int, u64p, ip64, c_int, c_int, ip32, ip32, c_int64, c_int,
                                          c_int]
        L.wt_language_count.argtypes = [c_void_p]
        L.wt_detect_language_batch.argtypes = [c_void_p, fp, c_int, ip32, fp]
        L.wt_detect_language_batch_dev.argtypes = [c_void_p, c_void_p, c_int, ip32, fp]
        L.wt_detect_language_pcm.argtypes = [c_void_p, fp, c_size_t, ip32, fp]
        L.wt_last_languages.argtypes = [c_void_p, ip32, fp, c_int]
        L.wt_dbg_language_head.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, fp, fp, fp, fp, fp, fp, ip32, fp,
                                           ip64, c_int]
        L.wt_dbg_language_head_rows.argtypes = [c_void_p] + [c_int] * 7 + [fp] * 5 + [POINTER(ctypes.c_uint32), ip32, fp, ip32, fp,
                                                                                   ip64, ip64, c_int, c_int, c_int, c_int]
        L.wt_encdec_tokens_full_batch.argtypes = [c_void_p, fp, c_int, ip64, c_int, ip32]
        L.wt_encdec_tokens_full_batch_dev.argtypes = [c_void_p, c_void_p, c_int, ip64, c_int, ip32]
        L.wt_transcribe_tokens_full_batch_dev.argtypes = [c_void_p, c_void_p, c_int, ip64, c_int, ip32]
        L.wt_dbg_self_attention_long.argtypes = [c_void_p, c_int, c_int, c_int, c_int, fp, fp, fp, fp]
        L.wt_dbg_self_attention_prefill.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, fp, fp, fp, fp]
        L.wt_dbg_self_attention_long_bf16.argtypes = L.wt_dbg_self_attention_long.argtypes
        L.wt_dbg_self_attention_prefill_bf16.argtypes = L.wt_dbg_self_attention_prefill.argtypes
        L.wt_dbg_self_attention_long_ragged.argtypes = [c_void_p, c_int, c_int, c_int, c_int, fp, fp, fp, fp, ip32, c_int]
        L.wt_dbg_self_attention_long_ragged_bf16.argtypes = L.wt_dbg_self_attention_long_ragged.argtypes
        L.wt_dbg_beam_full_step.argtypes = [c_void_p, POINTER(BeamFullArgs)]
        L.wt_dbg_beam_full_finalize.argtypes = [c_void_p, POINTER(BeamFullArgs)]
        L.wt_dbg_self_attention_long_gather.argtypes = [c_void_p, c_int, c_int, c_int, c_int, fp, fp, fp, fp, POINTER(ctypes.c_uint8)]
        L.wt_dbg_self_attention_long_gather_bf16.argtypes = L.wt_dbg_self_attention_long_gather.argtypes
        L.wt_dbg_self_attention_prefill_ragged.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, fp, fp, fp, fp, ip32, c_int]
        L.wt_dbg_self_attention_prefill_ragged_bf16.argtypes = L.wt_dbg_self_attention_prefill_ragged.argtypes
        L.wt_dbg_dec_ln_gemm_ragged.argtypes = [c_void_p, c_int, c_int, c_int, ip64, c_int, ip32, fp, fp,
                                                c_int, c_int, fp, fp, fp, fp, c_int, fp, fp]
        L.wt_dbg_ragged_cap.argtypes = [c_void_p, c_int, c_int, c_int, ip32, ip32]
        L.wt_last_segments.argtypes = [c_void_p, c_void_p, c_int]
        L.wt_last_windows.argtypes = [c_void_p, c_void_p, c_int]
        L.wt_vocab_seek_step.argtypes = [c_void_p, ip64, c_int, c_int, c_int, c_void_p, c_int, POINTER(c_int32)]
        L.wt_last_segment_text.argtypes = [c_void_p, c_int, c_char_p, c_size_t, POINTER(c_size_t)]
        L.wt_vocab_segments.argtypes = [c_void_p, ip64, c_int, c_int, c_void_p, c_int]
        L.wt_dbg_timestamp_select.argtypes = [c_void_p, c_int, c_int, fp, ip64, c_int, ip32, c_int, c_int, c_int, c_int,
                                              ip64, POINTER(ctypes.c_double), fp]
        L.wt_dbg_sample_select.argtypes = [c_void_p, c_int, c_int, fp, ip64, c_int, ip32, c_int, c_int, c_int, c_int, c_int,
                                           fp, ctypes.c_uint64, c_int, c_int, c_int, ip64, POINTER(ctypes.c_double), fp, fp]
        dp, u8p = POINTER(ctypes.c_double), POINTER(ctypes.c_uint8)
        L.wt_dbg_sample_select_group.argtypes = [c_void_p, c_int, c_int, c_int, fp, ip64, c_int, c_int, c_int, c_int, c_int,
                                                 c_int, c_int, fp, ctypes.c_uint64, c_int, c_int, c_int, c_int, ip64, dp, fp, fp]
        L.wt_dbg_best_of_begin.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, ip32, ip64, ip32, ip32, dp, ip32, u8p]
        L.wt_dbg_best_of_pick.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, ip64, fp, ip32, dp, ip32, ip64, fp,
                                          ip32, dp, ip32, ip32, dp, ip32]
        L.wt_last_scores.argtypes = [c_void_p, c_void_p, c_int]
        L.wt_last_decode_info.argtypes = [c_void_p, c_void_p, c_int]
        L.wt_last_best_of.argtypes = [c_void_p, ip32, POINTER(ctypes.c_double), ip32, c_int]
        L.wt_last_token_logprobs.argtypes = [c_void_p, fp, c_int, c_int]
        L.wt_last_segment_scores.argtypes = [c_void_p, fp, c_int]
        L.wt_dbg_token_scores.argtypes = [c_void_p, c_int, c_int, fp, ip64, c_int, ip32, c_int, c_int, c_int, c_int, c_int,
                                          ip32, fp, POINTER(ctypes.c_double), ip32, POINTER(ctypes.c_double)]
        u16p, u32p = POINTER(ctypes.c_uint16), POINTER(ctypes.c_uint32)
        L.wt_dbg_frontend_dims.argtypes = [c_void_p, ip32]
        L.wt_dbg_frontend_stages.argtypes = [c_void_p, c_int, fp, c_int, fp, fp, u16p, u16p, fp, fp, fp, u32p, fp, fp, fp]
        L.wt_dbg_log_clipmax.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, fp, fp, u32p, fp]
        L.wt_dbg_mel_normalize.argtypes = [c_void_p, c_int, c_int, c_int, u32p, fp]
        L.wt_dbg_mel_transpose.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, fp, c_void_p]
        L.wt_dbg_pcm_to_planes.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_float, c_float, fp, u16p]
        L.wt_dbg_gemm_addressed.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, fp, c_long, c_int, c_long, c_int, fp, fp,
                                            fp, c_int, c_int, c_void_p, c_long, c_long, c_int, c_long, c_int, fp, c_int, c_int,
                                            c_int, c_int, c_int]
        L.wt_dbg_plane_gemm_plan.argtypes = [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, ip32]
        L.wt_dbg_gemm_ln_fused.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, fp, c_long, c_int, c_long, c_int, fp, fp, fp,
                                           c_int, fp, fp, c_float, c_int, c_int, c_int, c_long, c_int, fp, u16p, fp, u16p, ip32,
                                           ip32]
        L.wt_dbg_layernorm_planes.argtypes = [c_void_p, c_int, c_int, fp, fp, fp, c_float, c_int, c_int, u16p, fp, ip32]
        L.wt_dbg_f32_to_planes.argtypes = [c_void_p, c_int, c_int, fp, fp, c_int, c_int, u16p]
        L.wt_dbg_encoder_attention_at.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, fp, fp, c_void_p]
        L.wt_dbg_encoder_scales.argtypes = [c_void_p, fp, c_int, POINTER(c_int)]
        L.wt_dbg_f16_scale_for.argtypes = [c_float]
        L.wt_dbg_f16_scale_for.restype = c_float
        L.wt_dbg_gemm_planes_scaled.argtypes = [c_void_p, c_int, c_int, c_int, fp, fp, fp, c_int, c_float, c_float, fp, c_int, c_int,
                                                c_int, c_int, c_void_p]
        L.wt_vocab_split_words.argtypes = [c_void_p, ip64, c_int, c_int, ip32, c_int]
        L.wt_vocab_merge_punctuation.argtypes = [c_void_p, ip64, c_int, ip32, c_int, ip32, c_int]
        L.wt_dtw_path.argtypes = [fp, c_int, c_int, ip32, ip32, c_int]
        L.wt_engine_set_alignment_heads.argtypes = [c_void_p, ip32, c_int]
        L.wt_last_words.argtypes = [c_void_p, c_void_p, c_int]
        L.wt_last_word_text.argtypes = [c_void_p, c_int, c_char_p, c_size_t, POINTER(c_size_t)]
        L.wt_dbg_last_alignment.argtypes = [c_void_p, c_int, ip32, ip64, fp, fp, ip32]
        L.wt_dbg_align_scores.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, fp, fp, c_int, ip32, ip32, c_int, ip32,
                                          c_int, c_int, fp, c_int]
        L.wt_dbg_align_scores_bf16.argtypes = L.wt_dbg_align_scores.argtypes
        L.wt_dbg_f32_to_bf16.argtypes = [c_void_p, c_int, c_int, fp, fp]
        L.wt_dbg_set_alignment.argtypes = [c_void_p, c_int, c_int, c_int]
        L.wt_dbg_align_matrix.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, fp, ip32, ip32, fp, fp]
        L.wt_dbg_align_dtw.argtypes = [c_void_p, c_int, c_int, c_int, fp, ip32, ip32, ip32, POINTER(ctypes.c_uint8)]
        _lib = L
    return _lib


PLANE_GEMM_TILES = ("192x128", "192x384", "256x384")
PLANE_GEMM_SCHEDULES = ("in step", "pp", "pp16", "pp16_persist")


def plane_gemm_plan(M, N, K, epi, planes_out=False, ln=False, n_cu=0):
    """What launch_gemm_planes will launch for this shape under the current plane GEMM mode (wt_dbg_plane_gemm_plan, no
    GPU work): SimpleNamespace(tile, schedule, fused, mode, kernel); tile indexes PLANE_GEMM_TILES, schedule
    PLANE_GEMM_SCHEDULES, kernel names both."""
    plan = np.zeros(4, np.int32)
    rc = lib().wt_dbg_plane_gemm_plan(0, M, N, K, epi, int(planes_out), int(ln), int(n_cu), 0, 0, _ip32(plan))
    if rc != WT_OK:
        raise WtError(rc, "wt_dbg_plane_gemm_plan")
    tile, schedule, fused, mode = (int(v) for v in plan)
    return types.SimpleNamespace(tile=tile, schedule=schedule, fused=bool(fused), mode=mode,
                                 kernel=f"{PLANE_GEMM_TILES[tile]} {PLANE_GEMM_SCHEDULES[schedule]}" + (" + LayerNorm" if fused else ""))


def f16_scale_for(bound) -> float:
    """csrc/kernels.h f16_scale_for, the engine's own (wt_dbg_f16_scale_for; no GPU work)."""
    return float(lib().wt_dbg_f16_scale_for(c_float(float(np.float32(bound)))))


def bf16_gemm_plan(M, N, epi, bf16_out=False, ln=False, c_rpb=1 << 30, ldc=None):
    """What launch_gemm_bf16_planes will launch: SimpleNamespace(bn, bm, whole_row, kernel); whole_row = the tile that
    holds whole rows, with the LayerNorm fused."""
    plan = np.zeros(4, np.int32)
    rc = lib().wt_dbg_plane_gemm_plan(1, M, N, 64, epi, int(bf16_out), int(ln), 0, c_rpb, N if ldc is None else ldc, _ip32(plan))
    if rc != WT_OK:
        raise WtError(rc, "wt_dbg_plane_gemm_plan")
    bn, bm, whole = (int(v) for v in plan[:3])
    return types.SimpleNamespace(bn=bn, bm=bm, whole_row=bool(whole), kernel=f"bf16 {bm}x{bn}" + (" + LayerNorm" if whole else ""))


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a: np.ndarray):
    return a.ctypes.data_as(POINTER(c_float)) if a is not None else None


def _ip32(a: np.ndarray):
    if a.dtype != np.int32 or not a.flags.c_contiguous:
        raise ValueError("expected a contiguous int32 array")
    return a.ctypes.data_as(POINTER(c_int32))


def _ip64(a: np.ndarray):
    if a.dtype != np.int64 or not a.flags.c_contiguous:
        raise ValueError("expected a contiguous int64 array")
    return a.ctypes.data_as(POINTER(c_int64))


def write_synthetic_weights(path: str, arch: str = "tiny", seed: int = 0) -> None:
    rc = lib().wt_write_synthetic_weights(path.encode(), arch.encode(), seed)
    if rc != WT_OK:
        raise WtError(rc, lib().wt_last_error(None).decode())


def write_synthetic_vocab(path: str, n_tokens: int = 50257) -> None:
    rc = lib().wt_write_synthetic_vocab(path.encode(), n_tokens)
    if rc != WT_OK:
        raise WtError(rc, lib().wt_last_error(None).decode())


def absorbed_query_matrix(wq, bq, wk):
    """The host fold of the absorbed cross-attention's query projection (no engine, no GPU): wq, wk [d][d], bq [d] ->
    A [heads * d][d] = c0 Wk_h^T Wq_h stacked over the heads and a [heads * d] = c0 Wk_h^T bq_h, c0 = 1/8 log2 e."""
    wq, bq, wk = _f32(wq), _f32(bq), _f32(wk)
    d = wq.shape[0]
    heads = d // 64
    A = np.zeros((heads * d, d), np.float32)
    av = np.zeros(heads * d, np.float32)
    rc = lib().wt_dbg_absorbed_query_matrix(heads, d, _fp(wq), _fp(bq), _fp(wk), _fp(A), _fp(av))
    if rc != WT_OK:
        raise WtError(rc, "absorbed_query_matrix: bad shape")
    return A, av


def language_id(code: str) -> int:
    return lib().wt_language_id(code.encode())


def lang_code(idx: int) -> str:
    return lib().wt_lang_code(idx).decode()


def wav_read_legacy(path: str) -> np.ndarray:
    n = c_size_t(0)
    rc = lib().wt_wav_read_legacy(path.encode(), None, 0, byref(n))
    if rc != WT_OK:
        return np.zeros(0, np.float32)  # the reference returns an empty vector
    out = np.zeros(n.value, np.float32)
    lib().wt_wav_read_legacy(path.encode(), _fp(out), out.size, byref(n))
    return out


# one time-stamped segment (wt_segment): the text ids row[id_begin : id_begin + id_count] of clip
# `clip`, spoken from t0_ms to t1_ms; open = the text ran to the end of the row without a closing timestamp
SEGMENT_DTYPE = np.dtype([(k, np.int32) for k in ("clip", "t0_ms", "t1_ms", "id_begin", "id_count", "open")])


# one clip of a decode with option scores (wt_clip_score)
SCORE_DTYPE = np.dtype([("sum_logprob", np.float32), ("avg_logprob", np.float32), ("no_speech_prob", np.float32),
                        ("n_generated", np.int32), ("skipped", np.int32)])
# one clip of a decode that sampled or ran fall-back (wt_clip_decode)
DECODE_DTYPE = np.dtype([("temperature_milli", np.int32), ("attempts", np.int32), ("needs_fallback", np.int32),
                         ("compression_ratio", np.float32)])


# one window of a seeking transcribe_long (wt_window): where it started in the file, how far the
# next one lies, the context and prompt ids it was decoded behind, the ids kept from it, whether skip_silence blanked it
# and the temperature its kept result was decoded at
WINDOW_DTYPE = np.dtype([("seek_sample", np.int64), ("advance_samples", np.int32), ("n_context", np.int32),
                         ("n_prompt", np.int32), ("n_kept_ids", np.int32), ("skipped", np.int32),
                         ("temperature_milli", np.int32)], align=True)


# one word of a decode with option word_timestamps (wt_word)
WORD_DTYPE = np.dtype([("clip", np.int32), ("segment", np.int32), ("t0_ms", np.int32), ("t1_ms", np.int32),
                       ("id_begin", np.int32), ("id_count", np.int32), ("probability", np.float32)])


def _segments(call):
    n = call(None, 0)
    if n < 0:
        raise WtError(-n, "no timestamp segments: the last synchronous decode ran without timestamps, or bad arguments")
    out = np.zeros(n, SEGMENT_DTYPE)
    if n:
        call(out.ctypes.data_as(c_void_p), n)
    return out


class Vocab:
    """Host-side mirror of the reference's ``Vocab`` + ``Filters`` as ``Reader::read`` fills them
    (whisper.h:44-101, :236-248) and of ``decode`` (whisper.h:252-257).  Needs no GPU."""

    INFO_KEYS = ("n_vocab", "eot", "sot", "translate", "transcribe", "prev", "solm", "not", "beg")

    def __init__(self, vocab_path: str, multilingual: bool = True):
        self._v = c_void_p()
        rc = lib().wt_vocab_open(os.fsencode(vocab_path), int(bool(multilingual)), byref(self._v))
        if rc != WT_OK:
            self._v = c_void_p()
            raise WtError(rc, lib().wt_last_error(None).decode())

    def close(self) -> None:
        if getattr(self, "_v", None) and self._v.value:
            lib().wt_vocab_close(self._v)
            self._v = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        out = (c_int32 * 9)()
        lib().wt_vocab_get_info(self._v, out)
        return dict(zip(self.INFO_KEYS, list(out)))

    def filters(self) -> np.ndarray:
        nm, nf = c_int32(0), c_int32(0)
        total = lib().wt_vocab_get_filters(self._v, None, 0, byref(nm), byref(nf))
        out = np.zeros(total, np.float32)
        lib().wt_vocab_get_filters(self._v, _fp(out), out.size, byref(nm), byref(nf))
        return out.reshape(nm.value, nf.value)

    def size(self) -> int:
        return lib().wt_vocab_size(self._v)

    def token(self, idx: int) -> bytes:
        buf = ctypes.create_string_buffer(512)
        n = c_size_t(0)
        rc = lib().wt_vocab_token(self._v, int(idx), buf, len(buf), byref(n))
        if rc != WT_OK:
            raise WtError(rc, lib().wt_last_error(None).decode())
        return buf.raw[: n.value]

    def decode(self, ids, omit_special_tokens: bool = False) -> bytes:
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        buf = ctypes.create_string_buffer(1 << 16)
        n = c_size_t(0)
        rc = lib().wt_vocab_decode(self._v, ids.ctypes.data_as(POINTER(c_int64)), ids.size, int(omit_special_tokens),
                                   buf, len(buf), byref(n))
        if rc != WT_OK:
            raise WtError(rc, lib().wt_last_error(None).decode())
        return buf.raw[: n.value]

    def segments(self, ids, sample_begin: int = 0) -> np.ndarray:
        """The timestamp segments of one id row whose first sample_begin ids are the prompt (SEGMENT_DTYPE records, clip
        = 0): text between an opening and a closing timestamp id; unclosed text ends at 30 000 ms with open = 1."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        return _segments(lambda out, cap: lib().wt_vocab_segments(self._v, ids.ctypes.data_as(POINTER(c_int64)), ids.size,
                                                                  int(sample_begin), out, cap))

    def seek_step(self, g, win_ticks: int, seg_ticks: int):
        """Whisper's seek rule (wt_vocab_seek_step) on the ids g a window generated before its first
        EOT: (SEGMENT_DTYPE records with clip = 0, times = tick x 20 ms and g[id_begin : id_begin + id_count] the slice,
        timestamps included; advance in ticks)."""
        g = np.ascontiguousarray(g, dtype=np.int64).reshape(-1)
        adv = c_int32(0)
        segs = _segments(lambda out, cap: lib().wt_vocab_seek_step(self._v, g.ctypes.data_as(POINTER(c_int64)), g.size,
                                                                   int(win_ticks), int(seg_ticks), out, cap, byref(adv)))
        return segs, adv.value

    def default_suppress(self):
        """Whisper's default suppression lists from this vocabulary (wt_vocab_default_suppress):
        (ids masked at every generated position, ids masked at the first one), int64, each sorted and unique."""
        ids, first = np.zeros(1024, np.int64), np.zeros(1024, np.int64)
        n, nf = c_int32(0), c_int32(0)
        rc = lib().wt_vocab_default_suppress(self._v, _ip64(ids), ids.size, byref(n), _ip64(first), first.size, byref(nf))
        if rc != WT_OK:
            raise WtError(rc, "default_suppress: more than 1024 ids")
        return ids[: n.value].copy(), first[: nf.value].copy()

    def split_words(self, ids, unicode_only: bool = False) -> np.ndarray:
        """Whisper's split_to_word_tokens (wt_vocab_split_words) on a row of ids, usually a clip's
        text ids and then EOT: the id counts of its words, int32; they add up to len(ids).  unicode_only: the split of the
        languages written without spaces, one word per complete UTF-8 sequence."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        out = np.zeros(max(ids.size, 1), np.int32)
        n = lib().wt_vocab_split_words(self._v, _ip64(ids), ids.size, int(bool(unicode_only)), _ip32(out), out.size)
        if n < 0:
            raise WtError(-n, "split_words: bad arguments")
        return out[:n].copy()

    def merge_punctuation(self, ids, word_len) -> np.ndarray:
        """Whisper's merge_punctuations with its default marks (wt_vocab_merge_punctuation) on the words word_len of a
        row of ids: the id counts of the merged words, int32."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        word_len = np.ascontiguousarray(word_len, dtype=np.int32).reshape(-1)
        out = np.zeros(max(word_len.size, 1), np.int32)
        n = lib().wt_vocab_merge_punctuation(self._v, _ip64(ids), ids.size, _ip32(word_len), word_len.size, _ip32(out),
                                             out.size)
        if n < 0:
            raise WtError(-n, "merge_punctuation: the word counts must be positive and add up to the id count")
        return out[:n].copy()


def dtw_path(cost):
    """Whisper's dynamic time warping in fp32 on the host (wt_dtw_path): cost [N][F] -> (jump int32
    [N], the first frame of the path in each row; path int32 [cells][2], the (row, frame) pairs from (0, 0) on)."""
    cost = _f32(cost)
    N, F = cost.shape
    jump, path = np.zeros(N, np.int32), np.zeros((N + F, 2), np.int32)
    n = lib().wt_dtw_path(_fp(cost), N, F, _ip32(jump), _ip32(path), N + F)
    if n < 0:
        raise WtError(-n, "dtw_path: 1 <= N <= 447 and 1 <= F <= 1500")
    return jump, path[:n].copy()


def log_mel_spectrogram(samples, filters, device_id: int = 0) -> np.ndarray:
    """Mirror of the free function ``whisper::log_mel_spectrogram`` (whisper.h:123): [n_mel][n_samples // 160]."""
    pcm = _f32(samples).reshape(-1)
    f = _f32(filters)
    n_len = c_int(0)
    out = np.zeros((f.shape[0], pcm.size // 160), np.float32)
    rc = lib().wt_log_mel_spectrogram(_fp(pcm), pcm.size, _fp(f), f.shape[0], f.shape[1], device_id, _fp(out),
                                      out.size, byref(n_len))
    if rc != WT_OK:
        raise WtError(rc, lib().wt_last_error(None).decode())
    return out


def convert_tflite(model_prefix: str, out_path: str) -> None:
    rc = lib().wt_convert_tflite(os.fsencode(model_prefix), os.fsencode(out_path))
    if rc != WT_OK:
        raise WtError(rc, lib().wt_last_error(None).decode())


class Engine:
    """Mirror of ``whisper::Engine`` / ``whisper::EncDec`` / ``whisper::Monolith`` (reference whisper.h:159-197)."""

    def __init__(self, model_prefix: str, vocab_path: str, multilingual: bool = True,
                 engine_type: EngineType = EngineType.EncDec, device_id: int = 0):
        self._h = c_void_p()
        rc = lib().wt_engine_create(int(engine_type), model_prefix.encode(), vocab_path.encode(),
                                    int(bool(multilingual)), device_id, byref(self._h))
        if rc != WT_OK:
            self._h = c_void_p()
            raise WtError(rc, lib().wt_last_error(None).decode())
        d = Dims()
        lib().wt_engine_dims(self._h, byref(d))
        self.dims = d

    # -- lifecycle -------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            lib().wt_engine_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        if rc != WT_OK:
            raise WtError(rc, lib().wt_last_error(self._h).decode())

    @property
    def handle(self) -> c_void_p:
        return self._h

    def set_option(self, key: str, value: int) -> None:
        self._check(lib().wt_engine_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key: str) -> int:
        v = c_long(0)
        self._check(lib().wt_engine_get_option(self._h, key.encode(), byref(v)))
        return v.value

    def set_prompt(self, ids) -> None:
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        self._check(lib().wt_engine_set_prompt(self._h, ids.ctypes.data_as(POINTER(c_int64)), ids.size))

    def set_context(self, ids) -> None:
        """Ids fed in front of the prompt behind <|startofprev|> by every full-length decode (Whisper's initial_prompt;
        the engine keeps the last n_text_ctx / 2 - 1, option context_ids); an empty list clears the context."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        self._check(lib().wt_engine_set_context(self._h, ids.ctypes.data_as(POINTER(c_int64)), ids.size))

    def set_contexts(self, contexts) -> None:
        """Per-clip contexts: clip b of every following full-length call is decoded behind contexts[b] (an empty list:
        the prompt alone); the call's batch must equal len(contexts).  One ragged decoder chain.
        An empty list clears; setting either kind of context clears the other (option context_clips)."""
        rows = [np.ascontiguousarray(c, dtype=np.int64).reshape(-1) for c in contexts]
        offsets = np.zeros(len(rows) + 1, np.int32)
        offsets[1:] = np.cumsum([r.size for r in rows])
        flat = np.concatenate(rows) if rows else np.zeros(0, np.int64)
        flat = np.ascontiguousarray(flat, dtype=np.int64)
        self._check(lib().wt_engine_set_contexts(self._h, flat.ctypes.data_as(POINTER(c_int64)),
                                                 offsets.ctypes.data_as(POINTER(c_int32)), len(rows)))

    def set_suppress(self, ids=(), first_ids=()) -> None:
        """Whisper's SuppressTokens / SuppressBlank (wt_engine_set_suppress): every full-length
        decode masks `ids` at every generated position and `first_ids` at the first one, on the device, in front of every
        other decoding rule.  Two empty lists clear (options suppress_ids, suppress_first_ids; suppress_default = 1
        installs Whisper's defaults from the vocabulary)."""
        a = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        f = np.ascontiguousarray(first_ids, dtype=np.int64).reshape(-1)
        self._check(lib().wt_engine_set_suppress(self._h, _ip64(a) if a.size else None, a.size,
                                                 _ip64(f) if f.size else None, f.size))

    def set_language_candidates(self, langs=()) -> None:
        """The languages every detecting path chooses among (wt_engine_set_language_candidates):
        probabilities are normalised over them and exactly 0 elsewhere.  An empty list clears (read-only option
        language_candidates: the number of distinct ids)."""
        a = np.ascontiguousarray(langs, dtype=np.int32).reshape(-1)
        self._check(lib().wt_engine_set_language_candidates(self._h, _ip32(a) if a.size else None, a.size))

    def dbg_suppress_logits(self, logits, ids=(), first_ids=(), first=False, V=None):
        """suppress_logits (k_suppress.hip) on logits [rows][ldl] whose first V columns are the vocabulary (default: all
        of them): the rows with -inf at the listed ids, and at first_ids when `first` is set; padding columns included."""
        logits = _f32(logits)
        rows, ldl = logits.shape
        a = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        f = np.ascontiguousarray(first_ids, dtype=np.int64).reshape(-1)
        out = np.zeros_like(logits)
        self._check(lib().wt_dbg_suppress_logits(self._h, rows, ldl if V is None else int(V), ldl, _fp(logits), _fp(out),
                                                 _ip64(a) if a.size else None, a.size, _ip64(f) if f.size else None, f.size,
                                                 int(bool(first))))
        return out

    # -- shapes ----------------------------------------------------------------------
    @property
    def mel_shape(self):
        return (self.dims.n_mels, 2 * self.dims.n_audio_ctx)

    @property
    def pcm_len(self) -> int:
        return 2 * self.dims.n_audio_ctx * 160

    # -- the reference's two virtuals ------------------------------------------------
    def transcribe(self, samples_or_path) -> str:
        buf = ctypes.create_string_buffer(16384)
        n = c_size_t(0)
        if isinstance(samples_or_path, (str, bytes, os.PathLike)):
            path = os.fsencode(samples_or_path)
            self._check(lib().wt_transcribe_file(self._h, path, buf, len(buf), byref(n)))
        else:
            pcm = _f32(samples_or_path).reshape(-1)
            self._check(lib().wt_transcribe_pcm(self._h, _fp(pcm), pcm.size, buf, len(buf), byref(n)))
        return buf.raw[: n.value].decode("utf-8", errors="replace")

    def transcribe_long(self, samples) -> str:
        """Long audio: consecutive 30 s windows, batched; per-window texts joined with '\\n'.  Option seek = 1: one window
        at a time, each starting at the last closed timestamp of the one before."""
        pcm = _f32(samples).reshape(-1)
        buf = ctypes.create_string_buffer(1 << 20)
        n = c_size_t(0)
        self._check(lib().wt_transcribe_long_pcm(self._h, _fp(pcm), pcm.size, buf, len(buf), byref(n)))
        return buf.raw[: n.value].decode("utf-8", errors="replace")

    def transcribe_long_batch(self, samples_list) -> list:
        """Seeking transcription of several recordings side by side: one window of every file per decoder chain (options
        as for transcribe_long with seek = 1).  Returns the per-file texts, each what transcribe_long
        gives for that file alone; last_windows() lists the windows file by file, last_window_files() is parallel to it."""
        pcms = [_f32(s).reshape(-1) for s in samples_list]
        n = len(pcms)
        ptrs = (POINTER(c_float) * max(n, 1))(*[_fp(p) if p.size else None for p in pcms])
        sizes = (c_size_t * max(n, 1))(*[p.size for p in pcms])
        self._check(lib().wt_transcribe_long_batch(self._h, ptrs, sizes, n))
        texts = []
        for f in range(n):
            ln = c_size_t(0)
            buf = ctypes.create_string_buffer(1 << 20)
            self._check(lib().wt_last_file_text(self._h, f, buf, len(buf), byref(ln)))
            texts.append(buf.raw[: ln.value].decode("utf-8", errors="replace"))
        return texts

    def last_window_files(self) -> np.ndarray:
        """int32 [windows]: the file of every record of last_windows() after transcribe_long_batch."""
        n = lib().wt_last_window_files(self._h, None, 0)
        if n < 0:
            raise WtError(-n, "no window files: the last synchronous decode was not a transcribe_long_batch")
        out = np.zeros(n, np.int32)
        if n:
            lib().wt_last_window_files(self._h, out.ctypes.data_as(POINTER(c_int32)), n)
        return out

    # -- batch entry points ----------------------------------------------------------
    def logmel_batch(self, pcm) -> np.ndarray:
        pcm = _f32(pcm).reshape(-1, self.pcm_len)
        mel = np.empty((pcm.shape[0],) + self.mel_shape, np.float32)
        self._check(lib().wt_logmel_batch(self._h, _fp(pcm), pcm.shape[0], _fp(mel)))
        return mel

    def encdec_tokens_batch(self, mel):
        mel = _f32(mel).reshape((-1,) + self.mel_shape)
        B = mel.shape[0]
        ids = np.zeros((B, WT_MAX_IDS), np.int64)
        n = np.zeros(B, np.int32)
        self._check(lib().wt_encdec_tokens_batch(
            self._h, _fp(mel), B, ids.ctypes.data_as(POINTER(c_int64)), n.ctypes.data_as(POINTER(c_int32))))
        return ids, n

    def encdec_tokens_batch_dev(self, d_mel_ptr: int, batch: int):
        ids = np.zeros((batch, WT_MAX_IDS), np.int64)
        n = np.zeros(batch, np.int32)
        self._check(lib().wt_encdec_tokens_batch_dev(
            self._h, c_void_p(d_mel_ptr), batch, ids.ctypes.data_as(POINTER(c_int64)),
            n.ctypes.data_as(POINTER(c_int32))))
        return ids, n

    def transcribe_tokens_batch_dev(self, d_pcm_ptr: int, batch: int):
        ids = np.zeros((batch, WT_MAX_IDS), np.int64)
        n = np.zeros(batch, np.int32)
        self._check(lib().wt_transcribe_tokens_batch_dev(
            self._h, c_void_p(d_pcm_ptr), batch, ids.ctypes.data_as(POINTER(c_int64)),
            n.ctypes.data_as(POINTER(c_int32))))
        return ids, n

    # -- full-length greedy decoding (option max_positions) ------
    def _full_rows(self, batch, ids_stride):
        stride = self.get_option("max_positions") + 1 if ids_stride is None else int(ids_stride)
        return np.zeros((batch, max(stride, 1)), np.int64), np.zeros(batch, np.int32), stride

    def encdec_tokens_full(self, mel, ids_stride=None):
        """mel [B][n_mels][frames] -> (ids int64 [B][max_positions + 1], n_ids int32 [B]); ids_stride overrides the row
        length handed to the library."""
        mel = _f32(mel).reshape((-1,) + self.mel_shape)
        ids, n, stride = self._full_rows(mel.shape[0], ids_stride)
        self._check(lib().wt_encdec_tokens_full_batch(self._h, _fp(mel), mel.shape[0], _ip64(ids), stride, _ip32(n)))
        return ids, n

    def encdec_tokens_full_dev(self, d_mel_ptr: int, batch: int, ids_stride=None):
        ids, n, stride = self._full_rows(batch, ids_stride)
        self._check(lib().wt_encdec_tokens_full_batch_dev(self._h, c_void_p(d_mel_ptr), batch, _ip64(ids), stride, _ip32(n)))
        return ids, n

    def transcribe_tokens_full_dev(self, d_pcm_ptr: int, batch: int, ids_stride=None):
        ids, n, stride = self._full_rows(batch, ids_stride)
        self._check(lib().wt_transcribe_tokens_full_batch_dev(self._h, c_void_p(d_pcm_ptr), batch, _ip64(ids), stride, _ip32(n)))
        return ids, n

    def pipeline_submit_dev(self, d_mel_ptr: int, batch: int) -> None:
        self._check(lib().wt_pipeline_submit_dev(self._h, c_void_p(d_mel_ptr), batch))
        self._submitted = getattr(self, "_submitted", [])
        self._submitted.append(batch)

    def pipeline_submit_pcm_dev(self, d_pcm_ptr: int, batch: int) -> None:
        self._check(lib().wt_pipeline_submit_pcm_dev(self._h, c_void_p(d_pcm_ptr), batch))
        self._submitted = getattr(self, "_submitted", [])
        self._submitted.append(batch)

    def pipeline_collect(self):
        batch = self._submitted.pop(0)
        ids = np.zeros((batch, WT_MAX_IDS), np.int64)
        n = np.zeros(batch, np.int32)
        self._check(lib().wt_pipeline_collect(
            self._h, ids.ctypes.data_as(POINTER(c_int64)), n.ctypes.data_as(POINTER(c_int32))))
        return ids, n

    def logmel_batch_dev(self, d_pcm_ptr: int, batch: int, d_mel_ptr: int) -> None:
        self._check(lib().wt_logmel_batch_dev(self._h, c_void_p(d_pcm_ptr), batch, c_void_p(d_mel_ptr)))

    def encdec_debug_batch(self, mel, want_enc_out=True, want_logits=True, steps_cap=27):
        mel = _f32(mel).reshape((-1,) + self.mel_shape)
        B = mel.shape[0]
        ids = np.zeros((B, WT_MAX_IDS), np.int64)
        n = np.zeros(B, np.int32)
        enc = np.zeros((B, self.dims.n_audio_ctx, self.dims.n_audio_state), np.float32) if want_enc_out else None
        logits = np.zeros((B, steps_cap, self.dims.n_vocab), np.float32) if want_logits else None
        self._check(lib().wt_encdec_debug_batch(
            self._h, _fp(mel), B, ids.ctypes.data_as(POINTER(c_int64)), n.ctypes.data_as(POINTER(c_int32)),
            _fp(enc) if enc is not None else None, _fp(logits) if logits is not None else None, steps_cap))
        return ids, n, enc, logits

    def timings(self) -> Timings:
        t = Timings()
        self._check(lib().wt_last_timings(self._h, byref(t)))
        return t

    def last_beam_scores(self):
        """Beam search: (sum of log-probabilities float32 [B], generated ids incl. EOT int32 [B]) of the chosen hypothesis
        of every clip of the last synchronous beam call."""
        n = lib().wt_last_beam_scores(self._h, None, None, 0)
        if n < 0:
            raise WtError(-n, "the last synchronous decode was not a beam search")
        sums = np.zeros(n, np.float32)
        lens = np.zeros(n, np.int32)
        lib().wt_last_beam_scores(self._h, _fp(sums), lens.ctypes.data_as(POINTER(c_int32)), n)
        return sums, lens

    # -- timestamp decoding (options timestamps + max_positions) ----
    def last_segments(self, with_text: bool = False, with_scores: bool = False):
        """SEGMENT_DTYPE records of every clip of the last synchronous timestamp decode (after transcribe_long: clip = the
        window's index, times in the file); with_text: (records, [bytes of each segment's text]); with_scores (option
        scores): the mean token log-probability of each segment's text ids, float32, follows as the last element."""
        segs = _segments(lambda out, cap: lib().wt_last_segments(self._h, out, cap))
        out = [segs]
        if with_text:
            texts = []
            for i in range(segs.size):
                buf = ctypes.create_string_buffer(1 << 16)
                n = c_size_t(0)
                self._check(lib().wt_last_segment_text(self._h, i, buf, len(buf), byref(n)))
                texts.append(buf.raw[: n.value])
            out.append(texts)
        if with_scores:
            n = lib().wt_last_segment_scores(self._h, None, 0)
            if n < 0:
                raise WtError(-n, "no segment scores: the last synchronous decode ran without scores or without timestamps")
            sc = np.zeros(n, np.float32)
            lib().wt_last_segment_scores(self._h, _fp(sc), n)
            out.append(sc)
        return out[0] if len(out) == 1 else tuple(out)

    def last_windows(self) -> np.ndarray:
        """WINDOW_DTYPE records, one per window, of the last synchronous decode when that was a transcribe_long with
        seek = 1."""
        n = lib().wt_last_windows(self._h, None, 0)
        if n < 0:
            raise WtError(-n, "no windows: the last synchronous decode was not a seeking transcribe_long")
        out = np.zeros(n, WINDOW_DTYPE)
        if n:
            lib().wt_last_windows(self._h, out.ctypes.data_as(c_void_p), n)
        return out

    # -- decode confidence (options scores + max_positions) ----
    def last_scores(self) -> np.ndarray:
        """SCORE_DTYPE records of every clip of the last synchronous decode with scores = 1 (after transcribe_long: one per
        window): sum_logprob, avg_logprob, no_speech_prob, n_generated, skipped."""
        n = lib().wt_last_scores(self._h, None, 0)
        if n < 0:
            raise WtError(-n, "no scores: the last synchronous decode ran without the option scores")
        out = np.zeros(n, SCORE_DTYPE)
        if n:
            lib().wt_last_scores(self._h, out.ctypes.data_as(c_void_p), n)
        return out

    def last_decode_info(self) -> np.ndarray:
        """DECODE_DTYPE records of every clip of the last synchronous decode that sampled or ran fall-back (options
        temperature, temperature_fallback): temperature_milli, attempts, needs_fallback,
        compression_ratio."""
        n = lib().wt_last_decode_info(self._h, None, 0)
        if n < 0:
            raise WtError(-n, "no decode info: the last synchronous decode neither sampled nor ran fall-back")
        out = np.zeros(n, DECODE_DTYPE)
        if n:
            lib().wt_last_decode_info(self._h, out.ctypes.data_as(c_void_p), n)
        return out

    def last_best_of(self):
        """(picked int32 [clips], sum_logprob float64 [clips][8], n_generated int32 [clips][8]) of the last synchronous
        decode in which some clip was kept from an attempt that ran best_of > 1 samples."""
        n = lib().wt_last_best_of(self._h, None, None, None, 0)
        if n < 0:
            raise WtError(-n, "no best-of record: no clip of the last synchronous decode was kept from an attempt with best_of > 1")
        picked, s, c = np.zeros(n, np.int32), np.zeros((n, 8), np.float64), np.zeros((n, 8), np.int32)
        if n:
            lib().wt_last_best_of(self._h, _ip32(picked), s.ctypes.data_as(POINTER(ctypes.c_double)), _ip32(c), n)
        return picked, s, c

    def last_token_logprobs(self, stride: int) -> np.ndarray:
        """float32 [clips][stride] aligned with the id rows of that decode: 0 for prompt ids and padding."""
        n = lib().wt_last_token_logprobs(self._h, None, 0, 0)
        if n < 0:
            raise WtError(-n, "no scores: the last synchronous decode ran without the option scores")
        out = np.zeros((n, int(stride)), np.float32)
        if out.size:
            lib().wt_last_token_logprobs(self._h, _fp(out), int(stride), n)
        return out

    # -- spoken-language detection ---------------------------
    def language_count(self) -> int:
        """Language tokens of this engine's vocabulary (99 for 51865 entries); WtError when it has none."""
        n = lib().wt_language_count(self._h)
        if n < 0:
            raise WtError(-n, "this engine's vocabulary has no language tokens")
        return n

    def detect_language(self, mel):
        """Encoder + one decoder position + language head: (lang int32 [B], probs float32 [B][language_count()])."""
        mel = _f32(mel).reshape((-1,) + self.mel_shape)
        B = mel.shape[0]
        n_lang = max(lib().wt_language_count(self._h), 1)
        lang = np.zeros(B, np.int32)
        probs = np.zeros((B, n_lang), np.float32)
        self._check(lib().wt_detect_language_batch(self._h, _fp(mel), B, _ip32(lang), _fp(probs)))
        return lang, probs

    def detect_language_dev(self, d_mel_ptr: int, batch: int):
        n_lang = max(lib().wt_language_count(self._h), 1)
        lang = np.zeros(batch, np.int32)
        probs = np.zeros((batch, n_lang), np.float32)
        self._check(lib().wt_detect_language_batch_dev(self._h, c_void_p(d_mel_ptr), batch, _ip32(lang), _fp(probs)))
        return lang, probs

    def detect_language_pcm(self, samples):
        """One clip of PCM (padded or truncated to one window): (lang, probability)."""
        pcm = _f32(samples).reshape(-1)
        lang, prob = c_int32(0), c_float(0)
        self._check(lib().wt_detect_language_pcm(self._h, _fp(pcm), pcm.size, byref(lang), byref(prob)))
        return lang.value, prob.value

    def last_languages(self):
        """After a synchronous decode with language = -1: (lang int32 [B], probability float32 [B]) per clip."""
        n = lib().wt_last_languages(self._h, None, None, 0)
        if n < 0:
            raise WtError(-n, "the last synchronous decode did not detect the language")
        lang = np.zeros(n, np.int32)
        prob = np.zeros(n, np.float32)
        lib().wt_last_languages(self._h, _ip32(lang), _fp(prob), n)
        return lang, prob

    def kernel_stats(self) -> dict:
        arr = (KernelStat * 8)()
        n = lib().wt_last_kernel_stats(self._h, arr, 8)
        return {arr[i].name.decode(): {"launches": arr[i].launches, "ms": arr[i].ms, "flops": arr[i].flops,
                                       "bytes": arr[i].bytes} for i in range(min(n, 8))}

    # -- host helpers ----------------------------------------------------------------
    def decode_bytes(self, ids, omit_special_tokens: bool = False) -> bytes:
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        buf = ctypes.create_string_buffer(16384)
        n = c_size_t(0)
        self._check(lib().wt_decode_text(self._h, ids.ctypes.data_as(POINTER(c_int64)), ids.size,
                                         int(omit_special_tokens), buf, len(buf), byref(n)))
        return buf.raw[: n.value]

    def decode_text(self, ids, omit_special_tokens: bool = False) -> str:
        return self.decode_bytes(ids, omit_special_tokens).decode("utf-8", errors="replace")

    def vocab_info(self) -> dict:
        out = (c_int32 * 9)()
        self._check(lib().wt_vocab_info(self._h, out))
        keys = ("n_vocab", "eot", "sot", "translate", "transcribe", "prev", "solm", "not", "beg")
        return dict(zip(keys, list(out)))

    def filters(self) -> np.ndarray:
        nm, nf = c_int32(0), c_int32(0)
        total = lib().wt_filters(self._h, None, 0, byref(nm), byref(nf))
        out = np.zeros(total, np.float32)
        lib().wt_filters(self._h, _fp(out), out.size, byref(nm), byref(nf))
        return out.reshape(nm.value, nf.value)

    # -- kernel-level taps (include/wt_debug.h) --------------------------------------
    def dbg_gemm(self, A, W, bias=None, R=None, pos=None, epi=0):
        A, W = _f32(A), _f32(W)
        M, K = A.shape
        N = W.shape[0]
        C = np.zeros((M, N), np.float32)
        bias = _f32(bias) if bias is not None else None
        R = _f32(R) if R is not None else None
        pos = _f32(pos) if pos is not None else None
        self._check(lib().wt_dbg_gemm(self._h, M, N, K, _fp(A), _fp(W), _fp(bias), _fp(R), _fp(pos),
                                      pos.shape[0] if pos is not None else 0, epi, _fp(C)))
        return C

    def dbg_gemm_planes(self, A, W, bias=None, R=None, pos=None, epi=1, planes_out=False, iters=0, n_cu=0):
        """The default encoder GEMM (fp16 planes).  Returns C, or (C, ms per launch) when iters > 0."""
        A, W = _f32(A), _f32(W)
        M, K = A.shape
        N = W.shape[0]
        C = np.zeros((M, N), np.float32)
        bias = _f32(bias) if bias is not None else np.zeros(N, np.float32)
        R = _f32(R) if R is not None else None
        pos = _f32(pos) if pos is not None else None
        ms = c_float(0)
        self._check(lib().wt_dbg_gemm_planes(self._h, M, N, K, _fp(A), _fp(W), _fp(bias), _fp(R), _fp(pos),
                                             pos.shape[0] if pos is not None else 0, epi, int(planes_out), iters, _fp(C),
                                             byref(ms), int(n_cu)))
        return (C, ms.value) if iters > 0 else C

    def dbg_gemm_planes_ln(self, A, W, bias, ln_g, ln_b, R=None, pos=None, epi=5, n_cu=0, want_y32=True):
        """The plane GEMM (N = 384) with the LayerNorm of its output rows fused into the epilogue.  Returns
        (C, ln_out, ln_y32, fused)."""
        A, W = _f32(A), _f32(W)
        M, K = A.shape
        assert W.shape[0] == 384
        C = np.zeros((M, 384), np.float32)
        ln = np.zeros((M, 384), np.float32)
        y32 = np.zeros((M, 384), np.float32) if want_y32 else None
        R = _f32(R) if R is not None else None
        pos = _f32(pos) if pos is not None else None
        fused = ctypes.c_int(0)
        self._check(lib().wt_dbg_gemm_planes_ln(self._h, M, K, _fp(A), _fp(W), _fp(_f32(bias)), _fp(R), _fp(pos),
                                                pos.shape[0] if pos is not None else 0, epi, _fp(_f32(ln_g)), _fp(_f32(ln_b)),
                                                int(n_cu), _fp(C), _fp(ln), _fp(y32) if y32 is not None else None, byref(fused)))
        return C, ln, y32, bool(fused.value)

    def dbg_cross_absorbed(self, qp, E, wv, bv, batch, heads, T, chunks, nq, iters=0, bf16=False):
        """Absorbed cross-attention + chunk combine + value projection: qp [nq * batch][heads * d], E [batch][T][d],
        wv [d][d], bv [d] -> [nq * batch][d] (and the average microseconds of the attention launch when iters > 0)"""
        qp, E, wv, bv = _f32(qp), _f32(E), _f32(wv), _f32(bv)
        d = heads * 64
        out = np.zeros((nq * batch, d), np.float32)
        us = c_float(0)
        fn = lib().wt_dbg_cross_absorbed_bf16 if bf16 else lib().wt_dbg_cross_absorbed
        self._check(fn(self._h, batch, heads, T, chunks, nq, _fp(qp), _fp(E), _fp(wv), _fp(bv), _fp(out), iters, byref(us)))
        return (out, us.value) if iters > 0 else out

    def dbg_cross_absorbed_chain(self, qp, E_src, wv, bv, batch, heads, T, chunks, nq, split=None, bf16=False, only=None,
                                 combine_only=False, ws=None, out=None, ws_fill=-7.0, out_fill=-9.0):
        """The absorbed cross-attention as a decoder chain runs it: E_src is a list of 1..4 arrays [clips of the group][T][d]
        (clip b reads E_src[b // split][b % split]), qp [nq * batch][heads * d].  only = (p0, nq) restricts the attention
        to that ONE launch; combine_only skips it (ws then holds hand-made records).  Returns (out [nq * batch + 1][d],
        ws [nq * batch + 1][heads][chunks][d + 4]); both start from the given arrays or the fills, and their last rows
        are guards the kernels must leave alone."""
        d, rows = heads * 64, nq * batch
        wv, bv = _f32(wv), _f32(bv)
        srcs = [_f32(e) for e in (E_src or [])]
        qp = _f32(qp) if qp is not None else None
        ws = np.array(ws, np.float32, order="C") if ws is not None else np.full((rows + 1, heads, chunks, d + 4), ws_fill, np.float32)
        out = np.array(out, np.float32, order="C") if out is not None else np.full((rows + 1, d), out_fill, np.float32)
        assert ws.shape == (rows + 1, heads, chunks, d + 4) and out.shape == (rows + 1, d)
        ptrs = (POINTER(c_float) * max(1, len(srcs)))(*[_fp(e) for e in srcs])
        mode = 2 if combine_only else (1 if only is not None else 0)
        p0, n1 = only if only is not None else (0, 0)
        self._check(lib().wt_dbg_cross_absorbed_chain(
            self._h, int(bf16), batch, heads, T, chunks, nq, batch if split is None else split, len(srcs), ptrs, _fp(qp),
            _fp(wv), _fp(bv), mode, p0, n1, _fp(out), _fp(ws)))
        return out, ws

    def dbg_encoder_attention_planes(self, qkv, batch, T, heads, iters=0):
        qkv = _f32(qkv)
        out = np.zeros((batch * T, heads * 64), np.float32)
        ms = c_float(0)
        self._check(lib().wt_dbg_encoder_attention_planes(self._h, batch, T, heads, _fp(qkv), iters, _fp(out), byref(ms)))
        return (out, ms.value) if iters > 0 else out

    def dbg_gemm_bf16(self, A, W, bias=None, R=None, pos=None, epi=1, bf16_out=False, iters=0):
        """The encoder GEMM of the bf16 storage mode (operands rounded to bf16 on the host side of the tap)."""
        A, W = _f32(A), _f32(W)
        M, K = A.shape
        N = W.shape[0]
        C = np.zeros((M, N), np.float32)
        bias = _f32(bias) if bias is not None else np.zeros(N, np.float32)
        R = _f32(R) if R is not None else None
        pos = _f32(pos) if pos is not None else None
        ms = c_float(0)
        self._check(lib().wt_dbg_gemm_bf16(self._h, M, N, K, _fp(A), _fp(W), _fp(bias), _fp(R), _fp(pos),
                                           pos.shape[0] if pos is not None else 0, epi, int(bf16_out), iters, _fp(C),
                                           byref(ms)))
        return (C, ms.value) if iters > 0 else C

    def dbg_encoder_attention_bf16(self, qkv, batch, T, heads, iters=0):
        qkv = _f32(qkv)
        out = np.zeros((batch * T, heads * 64), np.float32)
        ms = c_float(0)
        self._check(lib().wt_dbg_encoder_attention_bf16(self._h, batch, T, heads, _fp(qkv), iters, _fp(out), byref(ms)))
        return (out, ms.value) if iters > 0 else out

    def dbg_gemm_bench(self, M, N, K, epi=1, variant=0, iters=10) -> float:
        ms = c_float(0)
        self._check(lib().wt_dbg_gemm_bench(self._h, M, N, K, epi, variant, iters, byref(ms)))
        return ms.value

    def device_array(self, a):
        """A copy of the numpy array `a` resident in this engine's HBM (wt_device_alloc + upload): the caller-owned input
        of the *_dev entry points.  Returns a DeviceArray (data_ptr(), download(), free())."""
        return DeviceArray(self, a)

    def device_synchronize(self):
        self._check(lib().wt_device_synchronize(self._h))

    def set_forced_ids(self, ids=None):
        """Teacher forcing (test tap): ids [clips][32] every following decode of that many clips follows instead of its
        own argmax; None switches it off."""
        if ids is None:
            self._check(lib().wt_dbg_set_forced_ids(self._h, None, 0))
            return
        a = np.ascontiguousarray(ids, dtype=np.int64)
        assert a.ndim == 2 and a.shape[1] == 32
        self._check(lib().wt_dbg_set_forced_ids(self._h, a.ctypes.data_as(POINTER(c_int64)), a.shape[0]))

    def dbg_gemm_bf16_ln(self, A, W, bias, R, ln_g, ln_b):
        """x = R + bias + A . W^T (bf16 operands) with the fused LayerNorm: returns (x, LayerNorm plane as float, fp32 LayerNorm, fused)"""
        A, W, bias, R, ln_g, ln_b = (_f32(v) for v in (A, W, bias, R, ln_g, ln_b))
        M, K = A.shape
        N = W.shape[0]
        C = np.zeros((M, N), np.float32)
        ln = np.zeros((M, N), np.float32)
        y32 = np.zeros((M, N), np.float32)
        fused = c_int(0)
        self._check(lib().wt_dbg_gemm_bf16_ln(self._h, M, N, K, _fp(A), _fp(W), _fp(bias), _fp(R), _fp(ln_g), _fp(ln_b), _fp(C), _fp(ln),
                                              _fp(y32), byref(fused)))
        return C, ln, y32, bool(fused.value)

    def dbg_dec_gemm_bench(self, kind, B, N, K, rows=None, iters=200) -> float:
        us = c_float(0)
        self._check(lib().wt_dbg_dec_gemm_bench(self._h, kind, B, N, K, rows or B, iters, byref(us)))
        return us.value

    def dbg_dec_gemm(self, X, W, bias=None, mode=0, R=None, bf16=False):
        """mode 0 bias, 1 bias+gelu, 2 residual (Y = R + bias + X.W^T), 3 logits + argmax.  bf16: the bf16 storage
        mode's instantiation (weights one bf16 plane, activations rounded to bf16 in registers)."""
        X, W = _f32(X), _f32(W)
        B, K = X.shape
        N = W.shape[0]
        bias = _f32(bias) if bias is not None else np.zeros(N, np.float32)
        R = _f32(R) if R is not None else None
        Y = np.zeros((B, N), np.float32)
        am = np.zeros(B, np.int64)
        fn = lib().wt_dbg_dec_gemm_bf16 if bf16 else lib().wt_dbg_dec_gemm
        self._check(fn(self._h, mode, B, N, K, _fp(X), _fp(W), _fp(bias), _fp(R), _fp(Y), am.ctypes.data_as(POINTER(c_int64))))
        return (Y, am) if mode == 3 else Y

    def dbg_dec_ln_gemm(self, W, bias, ln_g, ln_b, xin=None, ids=None, pos=0, tok_emb=None, pos_emb=None,
                        gelu=False, bf16=False):
        W, bias, ln_g, ln_b = _f32(W), _f32(bias), _f32(ln_g), _f32(ln_b)
        N, K = W.shape
        xin = _f32(xin) if xin is not None else None
        ids_a = np.ascontiguousarray(ids, dtype=np.int64) if ids is not None else None
        tok_emb = _f32(tok_emb) if tok_emb is not None else None
        pos_emb = _f32(pos_emb) if pos_emb is not None else None
        B = xin.shape[0] if xin is not None else ids_a.shape[0]
        Y = np.zeros((B, N), np.float32)
        xout = np.zeros((B, K), np.float32)
        fn = lib().wt_dbg_dec_ln_gemm_bf16 if bf16 else lib().wt_dbg_dec_ln_gemm
        self._check(fn(
            self._h, B, N, K, _fp(xin),
            ids_a.ctypes.data_as(POINTER(c_int64)) if ids_a is not None else None, pos, _fp(tok_emb), _fp(pos_emb),
            tok_emb.shape[0] if tok_emb is not None else 0, pos_emb.shape[0] if pos_emb is not None else 0,
            _fp(ln_g), _fp(ln_b), _fp(W), _fp(bias), int(gelu), _fp(Y), _fp(xout)))
        return Y, xout

    def dbg_layernorm(self, x, g, b):
        x, g, b = _f32(x), _f32(g), _f32(b)
        y = np.zeros_like(x)
        self._check(lib().wt_dbg_layernorm(self._h, x.shape[0], x.shape[1], _fp(x), _fp(g), _fp(b), _fp(y)))
        return y

    def dbg_encoder_attention(self, qkv, batch, T, heads):
        qkv = _f32(qkv)
        out = np.zeros((batch * T, heads * 64), np.float32)
        self._check(lib().wt_dbg_encoder_attention(self._h, batch, T, heads, _fp(qkv), _fp(out)))
        return out

    def dbg_cross_attention(self, x, ln_g, ln_b, wq, bq, kc, vc, chunks=2, nq=1, bf16=False):
        """x [nq*B][d] residual rows (row = p * B + b) -> attention output [nq*B][d]; the query projection
        q = LayerNorm(x) . wq^T + bq runs inside the kernel."""
        x, ln_g, ln_b, wq, bq, kc, vc = (_f32(a) for a in (x, ln_g, ln_b, wq, bq, kc, vc))
        B, H, T, _ = kc.shape
        out = np.zeros((nq * B, H * 64), np.float32)
        fn = lib().wt_dbg_cross_attention_bf16 if bf16 else lib().wt_dbg_cross_attention
        self._check(fn(self._h, B, H, T, chunks, nq, _fp(x), _fp(ln_g), _fp(ln_b), _fp(wq), _fp(bq), _fp(kc), _fp(vc), _fp(out)))
        return out

    def dbg_cross_attention_records(self, x, ln_g, ln_b, wq, bq, kc, vc, chunks=2, nq=1, bf16=False, row0=0, n_rows=None,
                                    guard=None, batch=None, heads=None):
        """launch_cross_attention alone: the per-chunk records ws [nq*B][H][chunks][68] (o[64], m, l, pad).  The buffer is
        `guard` as given (default: all 1e30) and ONE launch writes the records of positions row0 .. row0 + n_rows - 1
        (default: all nq).  batch / heads override the counts taken from kc's shape (refusal tests)."""
        x, ln_g, ln_b, wq, bq, kc, vc = (_f32(a) for a in (x, ln_g, ln_b, wq, bq, kc, vc))
        B, H, T, _ = kc.shape
        ws = np.full((max(nq, 1) * B, H, max(chunks, 1), 68), 1e30, np.float32) if guard is None else _f32(guard).copy()
        fn = lib().wt_dbg_cross_attention_records_bf16 if bf16 else lib().wt_dbg_cross_attention_records
        self._check(fn(self._h, B if batch is None else batch, H if heads is None else heads, T, chunks, nq, _fp(x), _fp(ln_g),
                       _fp(ln_b), _fp(wq), _fp(bq), _fp(kc), _fp(vc), row0, nq if n_rows is None else n_rows, _fp(ws)))
        return ws

    def dbg_cross_combine(self, records, W, bias, R, B, bf16=False, guard=None):
        """dec_gemm's kProCombine prologue on given records [M][H][chunks][68]: Y = R + bias + combine(records) . W^T with
        R in place; guard [n][d] = rows behind the M of Y the kernel must not write.  Returns Y [M + n][d]."""
        records, W, bias, R = _f32(records), _f32(W), _f32(bias), _f32(R)
        M, H, chunks, _ = records.shape
        d = H * 64
        guard = np.zeros((0, d), np.float32) if guard is None else _f32(guard)
        Y = np.ascontiguousarray(np.concatenate([np.zeros((M, d), np.float32), guard]))
        fn = lib().wt_dbg_cross_combine_bf16 if bf16 else lib().wt_dbg_cross_combine
        self._check(fn(self._h, M, B, H, chunks, _fp(records), _fp(W), _fp(bias), _fp(R), guard.shape[0], _fp(Y)))
        return Y

    def dbg_self_attention(self, qkv, kcache, vcache, pos, npos=1, bf16=False, batch=None, heads=None):
        """batch / heads override the counts taken from the cache's shape (refusal tests)."""
        qkv, kcache, vcache = _f32(qkv), _f32(kcache).copy(), _f32(vcache).copy()
        B, cap, d = kcache.shape
        out = np.zeros((npos * B if npos > 0 else 0, d), np.float32)
        fn = lib().wt_dbg_self_attention_bf16 if bf16 else lib().wt_dbg_self_attention
        self._check(fn(self._h, B if batch is None else batch, d // 64 if heads is None else heads, cap, pos, npos, _fp(qkv),
                       _fp(kcache), _fp(vcache), _fp(out)))
        return out, kcache, vcache

    def dbg_timestamp_select(self, logits, ids, n_ids, sample_begin, eot, beg, max_initial_timestamp=50):
        """One step of the timestamp rules (k_timestamps.hip) per row: logits [B][V], ids [B][stride] with n_ids [B]
        ids each, the first sample_begin the prompt -> (token int64 [B], L float64 [B], M float32 [B]); L / M are NaN
        where no timestamp / no id below beg is allowed."""
        logits = _f32(logits)
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        n_ids = np.ascontiguousarray(n_ids, dtype=np.int32)
        B, V = logits.shape
        assert ids.shape[0] == B and n_ids.shape == (B,)
        tok, L, M = np.zeros(B, np.int64), np.zeros(B, np.float64), np.zeros(B, np.float32)
        self._check(lib().wt_dbg_timestamp_select(self._h, B, V, _fp(logits), _ip64(ids), ids.shape[1], _ip32(n_ids),
                                                  int(sample_begin), int(eot), int(beg), int(max_initial_timestamp),
                                                  _ip64(tok), L.ctypes.data_as(POINTER(ctypes.c_double)), _fp(M)))
        return tok, L, M

    def set_alignment_heads(self, pairs=()) -> None:
        """The (layer, head) pairs whose cross-attention the word timestamps are read from (wt_engine_set_alignment_heads,
        DESIGN.md section 21); none: the default, every head of the upper half of the decoder layers."""
        a = np.ascontiguousarray(np.asarray(list(pairs), np.int32).reshape(-1, 2))
        self._check(lib().wt_engine_set_alignment_heads(self._h, _ip32(a) if a.size else None, a.shape[0]))

    def last_words(self, with_text: bool = False):
        """The words of the last synchronous decode with option word_timestamps (WORD_DTYPE records, in clip order); with
        with_text also the list of their decoded bytes."""
        n = lib().wt_last_words(self._h, None, 0)
        if n < 0:
            raise WtError(-n, "no words: the last synchronous decode ran without word_timestamps")
        out = np.zeros(n, WORD_DTYPE)
        if n:
            lib().wt_last_words(self._h, out.ctypes.data_as(c_void_p), n)
        if not with_text:
            return out
        texts = []
        for i in range(n):
            buf = ctypes.create_string_buffer(1 << 12)
            ln = c_size_t(0)
            self._check(lib().wt_last_word_text(self._h, i, buf, len(buf), byref(ln)))
            texts.append(buf.raw[: ln.value])
        return out, texts

    def dbg_set_alignment(self, keep=-1, mode=-1, sub=-1) -> None:
        """Handles of the alignment pass (wt_dbg_set_alignment): keep what it forms for dbg_last_alignment, the form of
        align_scores (0 / 1), the most clips per sub-group (0 = by the workspace bound); -1 leaves a setting alone."""
        self._check(lib().wt_dbg_set_alignment(self._h, int(keep), int(mode), int(sub)))

    def dbg_last_alignment(self, clip: int) -> dict:
        """What the alignment pass of the last decode with word_timestamps = 1 behind dbg_set_alignment(keep=1) formed for one clip:
        row [L], W [heads][L][T], C [N][T], jump [N] and the counts n_a, L, N, F, heads, T."""
        dims = np.zeros(6, np.int32)
        self._check(lib().wt_dbg_last_alignment(self._h, int(clip), _ip32(dims), None, None, None, None))
        n_a, L, N, F, heads, T = (int(v) for v in dims)
        row, W = np.zeros(L, np.int64), np.zeros((heads, L, T), np.float32)
        C, jump = np.zeros((N, T), np.float32), np.zeros(N, np.int32)
        self._check(lib().wt_dbg_last_alignment(self._h, int(clip), _ip32(dims), _ip64(row), _fp(W), _fp(C), _ip32(jump)))
        return dict(n_a=n_a, L=L, N=N, F=F, heads=heads, T=T, row=row, W=W, C=C, jump=jump)

    def dbg_align_scores(self, qp, E, head, slot, F, W, pos0=0, mode=1, bf16=False):
        """align_scores (k_align.hip): qp [np][batch][H * d] absorbed queries of one pass, E [batch]
        [T][d] encoder output, head / slot the layer's alignment heads and their places in W's head axis, F [batch]
        valid frames; W [batch][heads_total][L_max][ld] is the output buffer as given (in / out).  Returns the buffer
        with W[b][slot][pos0 + p][t < T] = softmax over t < F[b] of q'_head(p, b) . e_t written into it.  mode: 0 = the
        fused kernel, 1 = frame chunks and the row softmax kernel.  bf16: the bf16 form (option full_bf16_all), E a float32
        array of bf16 values (anything else is rounded to nearest even on the host)."""
        qp, E, W = _f32(qp), _f32(E), _f32(W).copy()
        n_pos, batch, hd = qp.shape
        T, d = E.shape[1], E.shape[2]
        head, slot = np.ascontiguousarray(head, dtype=np.int32), np.ascontiguousarray(slot, dtype=np.int32)
        F = np.ascontiguousarray(F, dtype=np.int32)
        assert E.shape[0] == batch and hd == (d // 64) * d and W.shape[0] == batch and W.ndim == 4
        assert head.shape == slot.shape and F.shape == (batch,)
        fn = lib().wt_dbg_align_scores_bf16 if bf16 else lib().wt_dbg_align_scores
        self._check(fn(self._h, batch, d // 64, T, n_pos, int(pos0), _fp(qp), _fp(E), head.size, _ip32(head), _ip32(slot),
                       W.shape[1], _ip32(F), W.shape[2], W.shape[3], _fp(W), int(mode)))
        return W

    def dbg_f32_to_bf16(self, x, out):
        """launch_f32_to_bf16 (k_misc.hip): x [n] float32 -> a copy of out [n + guard] (float32 holding bf16 values) with
        the first n cells = x rounded to bf16, to nearest even."""
        x, out = _f32(x).ravel(), _f32(out).ravel().copy()
        self._check(lib().wt_dbg_f32_to_bf16(self._h, x.size, out.size - x.size, _fp(x), _fp(out)))
        return out

    def dbg_align_matrix(self, W, L, F, n_a, N_max=None, C=None, stats=None):
        """The two stage kernels of the alignment (k_align.hip): W [clips][heads][L_max][ld]
        attention weights, L [clips] fed positions and F [clips] valid frames -> (C [clips][N_max][ld], the cost of the
        rows n_a .. L[b] - 2; stats [clips][heads][2][ld], mean and 1 / std).  C and stats are in / out: cells the kernels
        do not write keep what the given arrays hold (zeros when None)."""
        W = _f32(W)
        clips, heads, L_max, ld = W.shape
        L, F = np.ascontiguousarray(L, dtype=np.int32), np.ascontiguousarray(F, dtype=np.int32)
        N_max = int(L.max()) - n_a - 1 if N_max is None else int(N_max)
        C = np.zeros((clips, max(N_max, 0), ld), np.float32) if C is None else _f32(C).copy()
        stats = np.zeros((clips, heads, 2, ld), np.float32) if stats is None else _f32(stats).copy()
        assert L.shape == (clips,) and F.shape == (clips,) and C.shape == (clips, N_max, ld) and stats.shape == (clips, heads, 2, ld)
        self._check(lib().wt_dbg_align_matrix(self._h, clips, heads, L_max, ld, int(n_a), N_max, _fp(W), _ip32(L), _ip32(F),
                                              _fp(C), _fp(stats)))
        return C, stats

    def dbg_align_dtw(self, C, N, F, jump=None, trace=None):
        """align_dtw (k_align.hip): C [clips][N_max][ld], N [clips] rows and F [clips] frames per clip -> (jump int32
        [clips][N_max], trace uint8 [clips][N_max][ld]); both in / out as dbg_align_matrix's."""
        C = _f32(C)
        clips, N_max, ld = C.shape
        N, F = np.ascontiguousarray(N, dtype=np.int32), np.ascontiguousarray(F, dtype=np.int32)
        jump = np.zeros((clips, N_max), np.int32) if jump is None else np.ascontiguousarray(jump, dtype=np.int32).copy()
        trace = np.zeros((clips, N_max, ld), np.uint8) if trace is None else np.ascontiguousarray(trace, dtype=np.uint8).copy()
        assert N.shape == (clips,) and F.shape == (clips,) and jump.shape == (clips, N_max) and trace.shape == C.shape
        self._check(lib().wt_dbg_align_dtw(self._h, clips, N_max, ld, _fp(C), _ip32(N), _ip32(F), _ip32(jump),
                                           trace.ctypes.data_as(POINTER(ctypes.c_uint8))))
        return jump, trace

    def dbg_sample_select(self, logits, ids, n_ids, sample_begin, temperature, seed=0, attempt=0, clip_base=0, pos=-1,
                          timestamps=False, eot=0, beg=1, max_initial_timestamp=50):
        """One sampling step (k_sample.hip) per row: arguments as dbg_timestamp_select, plus temperature float32 [B]
        (0 = greedy), the Philox seed, attempt and clip_base, and the position word of the counter (pos < 0: the row's
        n_ids - 1).  timestamps=False: the whole vocabulary is allowed.  Returns (token int64 [B], L float64 [B],
        M float32 [B], key float32 [B] = the winning key z / T + g)."""
        logits = _f32(logits)
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        n_ids = np.ascontiguousarray(n_ids, dtype=np.int32)
        B, V = logits.shape
        temperature = np.ascontiguousarray(np.broadcast_to(np.asarray(temperature, np.float32), (B,)))
        assert ids.shape[0] == B and n_ids.shape == (B,)
        tok, L, M, key = np.zeros(B, np.int64), np.zeros(B, np.float64), np.zeros(B, np.float32), np.zeros(B, np.float32)
        self._check(lib().wt_dbg_sample_select(self._h, B, V, _fp(logits), _ip64(ids), ids.shape[1], _ip32(n_ids),
                                               int(sample_begin), int(bool(timestamps)), int(eot), int(beg),
                                               int(max_initial_timestamp), _fp(temperature), int(seed), int(attempt),
                                               int(clip_base), int(pos), _ip64(tok),
                                               L.ctypes.data_as(POINTER(ctypes.c_double)), _fp(M), _fp(key)))
        return tok, L, M, key

    def dbg_sample_select_group(self, logits, ids, n_ids, sample_begin, temperature, group, seed=0, attempt=0, clip_base=0,
                                row0=0, pos=-1, timestamps=False, eot=0, beg=1, max_initial_timestamp=50):
        """The grouped sampler (k_sample.hip) in ONE launch: the B rows of logits / ids are `group`
        samples of clips = ceil(B / group) clips, row r = sample r // clips of clip r % clips; every row holds n_ids (an
        int) ids; temperature float32 [clips]; row0 = the first clip's entry of the parameter block.  Returns as
        dbg_sample_select."""
        logits = _f32(logits)
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        B, V = logits.shape
        clips = (B + int(group) - 1) // max(int(group), 1)
        temperature = np.ascontiguousarray(np.broadcast_to(np.asarray(temperature, np.float32), (clips,)))
        assert ids.shape[0] == B
        tok, L, M, key = np.zeros(B, np.int64), np.zeros(B, np.float64), np.zeros(B, np.float32), np.zeros(B, np.float32)
        self._check(lib().wt_dbg_sample_select_group(self._h, B, int(group), V, _fp(logits), _ip64(ids), ids.shape[1],
                                                     int(n_ids), int(sample_begin), int(bool(timestamps)), int(eot),
                                                     int(beg), int(max_initial_timestamp), _fp(temperature), int(seed),
                                                     int(attempt), int(clip_base), int(row0), int(pos), _ip64(tok),
                                                     L.ctypes.data_as(POINTER(ctypes.c_double)), _fp(M), _fp(key)))
        return tok, L, M, key

    def dbg_best_of_begin(self, ids, n_prompt, N, cap, frozen=None, fill=0x5a):
        """best_of_begin (k_best_of.hip): ids int64 [N * clips][stride], rows c < clips holding the clips' prompts.  The
        other arrays start filled with the byte `fill`.  Returns (ids, n_ids, finished, sum, count, anc [N * clips][cap])."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).copy()
        R, stride = ids.shape
        clips = R // int(N)
        assert clips * int(N) == R
        n_ids, fin, count = (np.full(R, fill * 0x01010101, np.int32) for _ in range(3))
        s = np.frombuffer(bytes([fill]) * (8 * R), np.float64).copy()
        anc = np.full((R, int(cap)), fill, np.uint8)
        fr = None if frozen is None else np.ascontiguousarray(frozen, dtype=np.int32)
        assert fr is None or fr.shape == (clips,)
        self._check(lib().wt_dbg_best_of_begin(self._h, clips, int(N), int(n_prompt), stride, int(cap),
                                               None if fr is None else _ip32(fr), _ip64(ids), _ip32(n_ids), _ip32(fin),
                                               s.ctypes.data_as(POINTER(ctypes.c_double)), _ip32(count),
                                               anc.ctypes.data_as(POINTER(ctypes.c_uint8))))
        return ids, n_ids, fin, s, count, anc

    def dbg_best_of_pick(self, ids, lp, n_ids, sums, counts, N, c0, out):
        """best_of_pick (k_best_of.hip): ids int64 / lp float32 [N * clips][stride], n_ids / counts int32 and sums float64
        [N * clips], rows r = j * clips + c.  out = dict of the in / out arrays over n_out rows: ids, lp [n_out][stride],
        n, count, picked int32 [n_out], sum float64 [n_out], all_sum float64 / all_count int32 [n_out][8].  Returns the
        dict after the launch (copies)."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        lp = _f32(lp)
        R, stride = ids.shape
        clips = R // int(N)
        assert clips * int(N) == R and lp.shape == ids.shape
        n_ids, counts = np.ascontiguousarray(n_ids, np.int32), np.ascontiguousarray(counts, np.int32)
        sums = np.ascontiguousarray(sums, np.float64)
        kinds = {"ids": np.int64, "lp": np.float32, "n": np.int32, "count": np.int32, "picked": np.int32, "sum": np.float64,
                 "all_sum": np.float64, "all_count": np.int32}
        o = {k: np.ascontiguousarray(out[k], dtype=t).copy() for k, t in kinds.items()}
        n_out = o["n"].shape[0]
        assert o["ids"].shape == (n_out, stride) and o["lp"].shape == (n_out, stride) and o["all_sum"].shape == (n_out, 8)
        dp = POINTER(ctypes.c_double)
        self._check(lib().wt_dbg_best_of_pick(self._h, clips, int(N), int(c0), n_out, stride, _ip64(ids), _fp(lp), _ip32(n_ids),
                                              sums.ctypes.data_as(dp), _ip32(counts), _ip64(o["ids"]), _fp(o["lp"]),
                                              _ip32(o["n"]), o["sum"].ctypes.data_as(dp), _ip32(o["count"]),
                                              _ip32(o["picked"]), o["all_sum"].ctypes.data_as(dp), _ip32(o["all_count"])))
        return o

    def dbg_token_scores(self, logits, ids, n_ids, sample_begin, live=None, sums=None, counts=None, timestamps=False, eot=0,
                         beg=1, max_initial_timestamp=50):
        """The score kernels (k_scores.hip) alone, one step per row: logits [B][V]; row b of ids [B][stride] holds n_ids[b]
        ids, the last of them the id the step chose; live [B] (default all), carried sums float64 [B] and counts int32 [B]
        (default 0).  Returns (lp float32 [B], sums, counts, den float64 [B] = the logsumexp of the allowed set)."""
        logits = _f32(logits)
        ids = np.ascontiguousarray(ids, np.int64)
        n_ids = np.ascontiguousarray(n_ids, np.int32)
        B, V = logits.shape
        live = np.ones(B, np.int32) if live is None else np.ascontiguousarray(live, np.int32)
        sums = np.zeros(B, np.float64) if sums is None else np.array(sums, np.float64)
        counts = np.zeros(B, np.int32) if counts is None else np.array(counts, np.int32)
        lp = np.zeros(B, np.float32)
        den = np.zeros(B, np.float64)
        dp = POINTER(ctypes.c_double)
        self._check(lib().wt_dbg_token_scores(self._h, B, V, _fp(logits), _ip64(ids), ids.shape[1], _ip32(n_ids),
                                              int(sample_begin), int(bool(timestamps)), int(eot), int(beg),
                                              int(max_initial_timestamp), _ip32(live), _fp(lp), sums.ctypes.data_as(dp),
                                              _ip32(counts), den.ctypes.data_as(dp)))
        return lp, sums, counts, den

    def dbg_self_attention_long(self, qkv, kcache, vcache, pos, bf16=False):
        """self_attention_long: one new position against caches [B][cap][d] (cap <= 448); returns (out [B][d], kcache,
        vcache) with row pos appended.  bf16: the bf16 form (option full_bf16) — the caches hold bf16-representable
        values and the appended row comes back rounded."""
        qkv, kcache, vcache = _f32(qkv), _f32(kcache).copy(), _f32(vcache).copy()
        B, cap, d = kcache.shape
        out = np.zeros((B, d), np.float32)
        fn = lib().wt_dbg_self_attention_long_bf16 if bf16 else lib().wt_dbg_self_attention_long
        self._check(fn(self._h, B, d // 64, cap, pos, _fp(qkv), _fp(kcache), _fp(vcache), _fp(out)))
        return out, kcache, vcache

    def dbg_self_attention_prefill(self, qkv, kcache, vcache, pos, npos, bf16=False):
        """self_attention_prefill: npos new positions pos .. pos + npos - 1 against caches [B][cap][d] (cap <= 448,
        npos * B <= 128), qkv [npos * B][3d] with rows p * B + b; returns (out [npos * B][d], kcache, vcache) with those
        rows appended.  bf16: the bf16 form (option full_bf16), caches of bf16-representable values."""
        qkv, kcache, vcache = _f32(qkv), _f32(kcache).copy(), _f32(vcache).copy()
        B, cap, d = kcache.shape
        out = np.zeros((npos * B, d), np.float32)
        fn = lib().wt_dbg_self_attention_prefill_bf16 if bf16 else lib().wt_dbg_self_attention_prefill
        self._check(fn(self._h, B, d // 64, cap, pos, npos, _fp(qkv), _fp(kcache), _fp(vcache), _fp(out)))
        return out, kcache, vcache

    def dbg_self_attention_long_ragged(self, qkv, kcache, vcache, pos, start, P, bf16=False):
        """self_attention_long under a slot count: clip b at position pos - start[b], void outside [0, P).  bf16: the bf16
        form (option full_bf16_all), caches of bf16-representable values."""
        qkv, kcache, vcache = _f32(qkv), _f32(kcache).copy(), _f32(vcache).copy()
        start = np.ascontiguousarray(start, np.int32)
        B, cap, d = kcache.shape
        assert start.shape == (B,)
        out = np.full((B, d), np.nan, np.float32)
        fn = lib().wt_dbg_self_attention_long_ragged_bf16 if bf16 else lib().wt_dbg_self_attention_long_ragged
        self._check(fn(self._h, B, d // 64, cap, pos, _fp(qkv), _fp(kcache), _fp(vcache), _fp(out), _ip32(start), P))
        return out, kcache, vcache

    def dbg_self_attention_long_gather(self, qkv, kcache, vcache, pos, anc, bf16=False):
        """self_attention_long over a shared cache: row r reads key k < pos from cache row min(anc[r][k], rows - 1);
        anc [rows][cap] uint8, rows <= 128.  bf16: the bf16 form (option full_bf16)."""
        qkv, kcache, vcache = _f32(qkv), _f32(kcache).copy(), _f32(vcache).copy()
        anc = np.ascontiguousarray(anc, np.uint8)
        B, cap, d = kcache.shape
        assert anc.shape == (B, cap)
        out = np.full((B, d), np.nan, np.float32)
        fn = lib().wt_dbg_self_attention_long_gather_bf16 if bf16 else lib().wt_dbg_self_attention_long_gather
        self._check(fn(self._h, B, d // 64, cap, pos, _fp(qkv), _fp(kcache), _fp(vcache), _fp(out),
                       anc.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return out, kcache, vcache

    def dbg_self_attention_prefill_ragged(self, qkv, kcache, vcache, pos, npos, start, P, bf16=False):
        """self_attention_prefill under a slot count: query p of clip b at position pos + p - start[b], void outside [0, P).
        bf16: the bf16 form (option full_bf16_all), caches of bf16-representable values."""
        qkv, kcache, vcache = _f32(qkv), _f32(kcache).copy(), _f32(vcache).copy()
        start = np.ascontiguousarray(start, np.int32)
        B, cap, d = kcache.shape
        assert start.shape == (B,)
        out = np.full((npos * B, d), np.nan, np.float32)
        fn = lib().wt_dbg_self_attention_prefill_ragged_bf16 if bf16 else lib().wt_dbg_self_attention_prefill_ragged
        self._check(fn(self._h, B, d // 64, cap, pos, npos, _fp(qkv), _fp(kcache), _fp(vcache), _fp(out), _ip32(start), P))
        return out, kcache, vcache

    def dbg_dec_ln_gemm_ragged(self, W, bias, ln_g, ln_b, ids, pos, pos_start, tok_emb, pos_emb, gelu=False):
        """dbg_dec_ln_gemm's embedding rows with the positional row pos - pos_start[b] (clamped); pos_start None: as it is."""
        W, bias, ln_g, ln_b, tok_emb, pos_emb = _f32(W), _f32(bias), _f32(ln_g), _f32(ln_b), _f32(tok_emb), _f32(pos_emb)
        N, K = W.shape
        ids_a = np.ascontiguousarray(ids, dtype=np.int64)
        B = ids_a.shape[0]
        st = np.ascontiguousarray(pos_start, np.int32) if pos_start is not None else None
        Y = np.zeros((B, N), np.float32)
        xout = np.zeros((B, K), np.float32)
        self._check(lib().wt_dbg_dec_ln_gemm_ragged(
            self._h, B, N, K, _ip64(ids_a), pos, _ip32(st) if st is not None else None, _fp(tok_emb), _fp(pos_emb),
            tok_emb.shape[0], pos_emb.shape[0], _fp(ln_g), _fp(ln_b), _fp(W), _fp(bias), int(gelu), _fp(Y), _fp(xout)))
        return Y, xout

    def dbg_ragged_cap(self, pos, P, start, finished):
        """ragged_cap: returns finished with finished[b] = 1 where pos - start[b] == P - 1."""
        start = np.ascontiguousarray(start, np.int32)
        fin = np.array(finished, np.int32)
        self._check(lib().wt_dbg_ragged_cap(self._h, start.size, pos, P, _ip32(start), _ip32(fin)))
        return fin

    # beam search (k_beam.hip).  The per-clip state is a dict of the engine's arrays (beam_state()), updated in place.
    @staticmethod
    def beam_state(fill=0):
        """live_sum / fin_sum / fin_len [64][8], fin_tok [64][8][32], n_fin / done [64]; every entry = fill."""
        C, S = 64, 8
        return {"live_sum": np.full((C, S), fill, np.float32), "fin_tok": np.full((C, S, 32), fill, np.int32),
                "fin_sum": np.full((C, S), fill, np.float32), "fin_len": np.full((C, S), fill, np.int32),
                "n_fin": np.full(C, fill, np.int32), "done": np.full(C, fill, np.int32)}

    @staticmethod
    def _beam_state_ptrs(st):
        want = Engine.beam_state()
        for k, a in want.items():
            if st[k].dtype != a.dtype or st[k].shape != a.shape or not st[k].flags.c_contiguous:
                raise ValueError(f"beam state {k}: expected a contiguous {a.dtype} array of shape {a.shape}")
        return (_fp(st["live_sum"]), _ip32(st["fin_tok"]), _fp(st["fin_sum"]), _ip32(st["fin_len"]), _ip32(st["n_fin"]),
                _ip32(st["done"]))

    def dbg_beam_topk(self, logits, V, kk):
        """logits [rows][ldl] -> (m [rows][chunks], s [rows][chunks], keys uint64 [rows][chunks][kk])."""
        logits = _f32(logits)
        rows, ldl = logits.shape
        chunks = (V + 4095) // 4096
        m = np.zeros((rows, chunks), np.float32)
        s = np.zeros((rows, chunks), np.float32)
        keys = np.zeros((rows, chunks, kk), np.uint64)
        self._check(lib().wt_dbg_beam_topk(self._h, rows, V, ldl, kk, _fp(logits), _fp(m), _fp(s),
                                           keys.ctypes.data_as(POINTER(c_uint64))))
        return m, s, keys

    def dbg_beam_step(self, K, clips, c0, n_live, pos, n_prompt, eot, logits, ids, state):
        """One step over logits [n_live * clips][V] and id rows [n_live * clips][32]; state updated in place.
        Returns (parent [K * clips], token [K * clips], ids_next [K * clips][32])."""
        logits = _f32(logits)
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        V = logits.shape[1]
        parent = np.zeros(K * clips, np.int32)
        token = np.zeros(K * clips, np.int64)
        ids_next = np.zeros((K * clips, 32), np.int64)
        self._check(lib().wt_dbg_beam_step(self._h, K, clips, c0, n_live, pos, n_prompt, V, eot, _fp(logits), _ip64(ids),
                                           *self._beam_state_ptrs(state), _ip32(parent), _ip64(token), _ip64(ids_next)))
        return parent, token, ids_next

    def _beam_full_args(self, scalars, arrays):
        a = BeamFullArgs()
        for name in BeamFullArgs._SCALARS:
            setattr(a, name, int(scalars.get(name, 0)))
        for name, dt in BeamFullArgs._ARRAYS:
            arr = arrays.get(name)
            if arr is not None:
                assert arr.dtype == dt and arr.flags.c_contiguous, name
                setattr(a, name, arr.ctypes.data)
        return a

    def dbg_beam_full_step(self, state, logits, ids, lp, anc, *, K, clips, pos, n_prompt, cap, eot, beg=0, timestamps=False,
                           max_initial=-1, c0=0, begin=False, want_part=False):
        """One step of decode_beam_full over the live rows' logits [rows][ldl >= V... here ldl = V], ids / lp [rows][cap + 1]
        and anc [rows][cap]; `state` (beam_full_state) is updated in place.  Returns dict(parent, token, tok_lp, ids_next,
        lp_next, anc_next [K * clips][..], lse [rows], and with want_part: part_stats, part_keys)."""
        logits = _f32(logits)
        rows, V = logits.shape
        stride = cap + 1
        R = K * clips
        arrays = dict(state)
        arrays.update(logits=logits, ids=np.ascontiguousarray(ids, np.int64), lp=_f32(lp), anc=np.ascontiguousarray(anc, np.uint8))
        assert arrays["ids"].shape == (rows, stride) and arrays["lp"].shape == (rows, stride) and arrays["anc"].shape == (rows, cap)
        out = {"parent": np.full(R, -1, np.int32), "token": np.full(R, -1, np.int64), "tok_lp": np.full(R, np.nan, np.float32),
               "ids_next": np.full((R, stride), -7, np.int64), "lp_next": np.full((R, stride), -7.0, np.float32),
               "anc_next": np.full((R, cap), 251, np.uint8), "lse": np.full(rows, -7.0, np.float64)}
        if want_part:
            chunks = (V + 4095) // 4096
            out["part_stats"] = np.zeros((rows, chunks, 4), np.float32)
            out["part_keys"] = np.zeros((rows, chunks, 2, K + 1), np.uint64)
        arrays.update(out)
        a = self._beam_full_args(dict(K=K, clips=clips, c0=c0, pos=pos, n_prompt=n_prompt, V=V, ldl=V, stride=stride, cap=cap, eot=eot,
                                      beg=beg, max_initial=max_initial, timestamps=int(bool(timestamps)), begin=int(bool(begin))), arrays)
        self._check(lib().wt_dbg_beam_full_step(self._h, ctypes.byref(a)))
        return out

    def dbg_beam_full_finalize(self, state, ids, lp, *, K, clips, pos, n_prompt, cap, c0=0):
        """beam_full_finalize over the rows after the last advance, ids / lp [K * clips][cap + 1]; `state` updated in place.
        Returns dict(out_ids [64][cap + 1], out_lp, out_n, out_len, out_sum [64])."""
        stride = cap + 1
        arrays = dict(state)
        arrays.update(ids=np.ascontiguousarray(ids, np.int64), lp=_f32(lp))
        assert arrays["ids"].shape == (K * clips, stride) and arrays["lp"].shape == (K * clips, stride)
        out = {"out_ids": np.full((64, stride), -7, np.int64), "out_lp": np.full((64, stride), -7.0, np.float32),
               "out_n": np.full(64, -7, np.int32), "out_len": np.full(64, -7, np.int32), "out_sum": np.full(64, -7.0, np.float64)}
        arrays.update(out)
        a = self._beam_full_args(dict(K=K, clips=clips, c0=c0, pos=pos, n_prompt=n_prompt, V=1, ldl=1, stride=stride, cap=cap), arrays)
        self._check(lib().wt_dbg_beam_full_finalize(self._h, ctypes.byref(a)))
        return out

    def dbg_beam_reorder(self, src_rows, dst_rows, cap, d, slabs, pos, V, kv_src, kv_dst, ids_src, ids_dst, parent, token):
        """kv_dst [slabs * dst_rows + 1][cap][d] and ids_dst [128][32]: returned updated (copies)."""
        kv_src = _f32(kv_src) if slabs > 0 else None
        kv_dst = _f32(kv_dst).copy() if slabs > 0 else None
        ids_src = np.ascontiguousarray(ids_src, dtype=np.int64)
        ids_dst = np.array(ids_dst, dtype=np.int64, order="C")
        parent = np.ascontiguousarray(parent, dtype=np.int32)
        token = np.ascontiguousarray(token, dtype=np.int64)
        self._check(lib().wt_dbg_beam_reorder(self._h, src_rows, dst_rows, cap, d, slabs, pos, V, _fp(kv_src), _fp(kv_dst),
                                              _ip64(ids_src), _ip64(ids_dst), _ip32(parent), _ip64(token)))
        return kv_dst, ids_dst

    def dbg_beam_finalize(self, K, clips, c0, pos, n_prompt, ids, state, out=None):
        """ids [K * clips][32]; state updated in place; out = dict(ids [64][32], n, sum, len [64]) in / out."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        if out is None:
            out = {"ids": np.zeros((64, 32), np.int64), "n": np.zeros(64, np.int32), "sum": np.zeros(64, np.float32),
                   "len": np.zeros(64, np.int32)}
        self._check(lib().wt_dbg_beam_finalize(self._h, K, clips, c0, pos, n_prompt, _ip64(ids), *self._beam_state_ptrs(state),
                                               _ip64(out["ids"]), _ip32(out["n"]), _fp(out["sum"]), _ip32(out["len"])))
        return out

    # the tail of a greedy decoder step (k_decoder.hip, select_token), kernel by kernel
    def dbg_dec_gemm_ksplit(self, X, W, bias, R, B=None, bf16=False):
        """fc2 as the engine runs it with fc2_ksplit = 2 over X [M][K] (M / B positions x B clips): returns (Y, part,
        R as read back) with Y = R + bias + X[:, :K/2] . W[:, :K/2]^T and part = X[:, K/2:] . W[:, K/2:]^T; Y and part
        start as NaN."""
        X, W, bias = _f32(X), _f32(W), _f32(bias)
        R = np.array(R, np.float32, order="C")
        M, K = X.shape
        N = W.shape[0]
        Y = np.full((M, N), np.nan, np.float32)
        part = np.full((M, N), np.nan, np.float32)
        self._check(lib().wt_dbg_dec_gemm_ksplit(self._h, int(bf16), M, B or M, N, K, _fp(X), _fp(W), _fp(bias), _fp(R),
                                                 _fp(Y), _fp(part)))
        return Y, part, R

    def dbg_dec_ln_gemm_rows(self, W, bias, ln_g, ln_b, xin=None, xpart=None, ids=None, pos=0, tok_emb=None, pos_emb=None,
                             B=None, M=None, gelu=False, bf16=False, xout=None):
        """LayerNorm prologue + GEMM over a row source: xin [M][K] (LNMODE 0), xin + xpart (3), or embedding rows from
        ids [B][stride] for M = positions x B rows (2).  xout [M + 1][K] (zeros when not given) is in / out, its last row
        a guard.  Returns (Y [M][N], xout)."""
        W, bias, ln_g, ln_b = _f32(W), _f32(bias), _f32(ln_g), _f32(ln_b)
        N, K = W.shape
        xin = _f32(xin) if xin is not None else None
        xpart = _f32(xpart) if xpart is not None else None
        ids_a = np.ascontiguousarray(ids, dtype=np.int64) if ids is not None else None
        tok_emb = _f32(tok_emb) if tok_emb is not None else None
        pos_emb = _f32(pos_emb) if pos_emb is not None else None
        if ids_a is not None:
            B, stride = ids_a.shape
            M = M or B
        else:
            M, stride = xin.shape[0], 0
            B = B or M
        xout = np.array(xout, np.float32, order="C") if xout is not None else np.zeros((M + 1, K), np.float32)
        assert xout.shape == (M + 1, K)
        Y = np.zeros((M, N), np.float32)
        self._check(lib().wt_dbg_dec_ln_gemm_rows(
            self._h, int(bf16), M, B, N, K, _fp(xin), _fp(xpart), _ip64(ids_a) if ids_a is not None else None, stride, pos,
            _fp(tok_emb), _fp(pos_emb), tok_emb.shape[0] if tok_emb is not None else 0,
            pos_emb.shape[0] if pos_emb is not None else 0, _fp(ln_g), _fp(ln_b), _fp(W), _fp(bias), int(gelu), _fp(Y),
            _fp(xout)))
        return Y, xout

    def dbg_dec_logits(self, xin, ln_g, ln_b, E, xpart=None, blocks=0, bf16=False, want_logits=True,
                       logits_guard=1.0e30, records_guard=0xA5A5A5A5A5A5A5A5):
        """Final LayerNorm of xin [M][K] (+ xpart), logits against E [V][K] and the per-tile argmax records on `blocks`
        resident blocks (0 = 512).  Returns (logits [M + 1][V] or None, records uint64 [M + 1][ceil(V / 32)]); both
        start filled with the guard values, and their last rows must keep them."""
        xin, ln_g, ln_b, E = _f32(xin), _f32(ln_g), _f32(ln_b), _f32(E)
        xpart = _f32(xpart) if xpart is not None else None
        M, K = xin.shape
        V = E.shape[0]
        logits = np.full((M + 1, V), logits_guard, np.float32) if want_logits else None
        records = np.full((M + 1, (V + 31) // 32), records_guard, np.uint64)
        self._check(lib().wt_dbg_dec_logits(self._h, int(bf16), M, V, K, _fp(xin), _fp(xpart), _fp(ln_g), _fp(ln_b), _fp(E),
                                            blocks, _fp(logits), records.ctypes.data_as(POINTER(c_uint64))))
        return logits, records

    def dbg_language_head(self, x, ln_g, ln_b, tok_emb, lang_lo, n_lang, xpart=None, ids=None, forced_lang=-1):
        """language_head over rows x [rows][d] (+ xpart) against tok_emb [n_vocab][d], language rows lang_lo .. lang_lo +
        n_lang - 1.  Returns (probs [rows][n_lang], lang [rows], lang_prob [rows], ids copy or None)."""
        x, ln_g, ln_b, tok_emb = _f32(x), _f32(ln_g), _f32(ln_b), _f32(tok_emb)
        xpart = _f32(xpart) if xpart is not None else None
        rows, d = x.shape
        probs = np.full((rows, n_lang), np.nan, np.float32)
        lang = np.full(rows, -1, np.int32)
        prob = np.full(rows, np.nan, np.float32)
        ids = np.array(ids, np.int64, order="C") if ids is not None else None
        self._check(lib().wt_dbg_language_head(
            self._h, rows, d, tok_emb.shape[0], lang_lo, n_lang, forced_lang, _fp(x), _fp(xpart), _fp(ln_g), _fp(ln_b),
            _fp(tok_emb), _fp(probs), _ip32(lang), _fp(prob), _ip64(ids) if ids is not None else None,
            ids.shape[1] if ids is not None else 0))
        return probs, lang, prob, ids

    def dbg_language_head_rows(self, x, ln_g, ln_b, tok_emb, lang_lo, n_lang, clips, x_rows_per_clip=1, xpart=None, allow=None,
                               hold=None, ids=None, ids2=None, id_pos=1, fan=1):
        """language_head_rows: clip b reads row b * x_rows_per_clip of x [x_rows][d] (+ xpart) and writes lang_lo + lang[b]
        at column id_pos of rows b * fan .. b * fan + fan - 1 of ids (and ids2), both [ids_rows][stride] int64.  allow: four
        uint32 words or None; hold: int32 [clips] or None (a held clip's probs are the detected ones).
        Returns (probs [clips][n_lang], lang [clips], lang_prob [clips], ids copy or None, ids2 copy or None)."""
        x, ln_g, ln_b, tok_emb = _f32(x), _f32(ln_g), _f32(ln_b), _f32(tok_emb)
        xpart = _f32(xpart) if xpart is not None else None
        x_rows, d = x.shape
        probs = np.full((clips, max(n_lang, 1)), np.nan, np.float32)
        lang = np.full(clips, -1, np.int32)
        prob = np.full(clips, np.nan, np.float32)
        allow = np.ascontiguousarray(allow, dtype=np.uint32) if allow is not None else None
        hold = np.ascontiguousarray(hold, dtype=np.int32) if hold is not None else None
        ids = np.array(ids, np.int64, order="C") if ids is not None else None
        ids2 = np.array(ids2, np.int64, order="C") if ids2 is not None else None
        shape = ids.shape if ids is not None else ids2.shape if ids2 is not None else (0, 0)
        self._check(lib().wt_dbg_language_head_rows(
            self._h, clips, x_rows, x_rows_per_clip, d, tok_emb.shape[0], lang_lo, n_lang, _fp(x), _fp(xpart), _fp(ln_g),
            _fp(ln_b), _fp(tok_emb), allow.ctypes.data_as(POINTER(ctypes.c_uint32)) if allow is not None else None,
            _ip32(hold) if hold is not None else None, _fp(probs), _ip32(lang), _fp(prob),
            _ip64(ids) if ids is not None else None, _ip64(ids2) if ids2 is not None else None, shape[0], shape[1], id_pos,
            fan if (ids is not None or ids2 is not None) else 0))
        return probs, lang, prob, ids, ids2

    def dbg_select_token(self, records, ids, pos, n_ids, finished, eot, stop_at_eot=True, keep_ids=False):
        """select_token over records uint64 [B][n_tiles]; ids int64 [B][stride], n_ids / finished int32 [B] are copied
        and returned updated: (ids, n_ids, finished)."""
        records = np.ascontiguousarray(records, dtype=np.uint64)
        B, n_tiles = records.shape
        ids = np.array(ids, np.int64, order="C")
        n_ids = np.array(n_ids, np.int32, order="C")
        finished = np.array(finished, np.int32, order="C")
        self._check(lib().wt_dbg_select_token(self._h, B, n_tiles, records.ctypes.data_as(POINTER(c_uint64)), _ip64(ids),
                                              ids.shape[1], pos, _ip32(n_ids), _ip32(finished), int(eot), int(stop_at_eot),
                                              int(keep_ids)))
        return ids, n_ids, finished


    # --- the log-mel front end, kernel by kernel (include/wt_debug.h) ---

    def dbg_frontend_dims(self) -> dict:
        d = np.zeros(8, np.int32)
        self._check(lib().wt_dbg_frontend_dims(self._h, _ip32(d)))
        return dict(zip(("frames", "samples", "pcm_stride", "pw_ld", "mel_n", "mel_k", "dft_n", "dft_k"), map(int, d)))

    def dbg_frontend_stages(self, pcm, valid_frames=-1) -> dict:
        """Engine::logmel over pcm [batch][samples], every stage: mel, planes ((hi + lo) / scale), hi / lo (float16 views
        of the raw planes), pw, melacc, raw (the log-mel before mel_normalize), words / maxima [batch][4], basis,
        mel_matrix."""
        pcm = _f32(pcm)
        d = self.dbg_frontend_dims()
        B, T0 = pcm.shape[0], d["frames"]
        assert pcm.shape == (B, d["samples"])
        n_mel = self.mel_shape[0]
        r = {
            "mel": np.empty((B, n_mel, T0), np.float32), "planes": np.empty((B, d["pcm_stride"]), np.float32),
            "hi": np.empty((B, d["pcm_stride"]), np.uint16), "lo": np.empty((B, d["pcm_stride"]), np.uint16),
            "pw": np.empty((B * T0, d["pw_ld"]), np.float32), "melacc": np.empty((B * T0, d["mel_n"]), np.float32),
            "raw": np.empty((B, n_mel, T0), np.float32), "words": np.empty((B, 4), np.uint32),
            "maxima": np.empty((B, 4), np.float32), "basis": np.empty((d["dft_n"], d["dft_k"]), np.float32),
            "mel_matrix": np.empty((d["mel_n"], d["mel_k"]), np.float32),
        }
        u16, u32 = POINTER(ctypes.c_uint16), POINTER(ctypes.c_uint32)
        self._check(lib().wt_dbg_frontend_stages(
            self._h, B, _fp(pcm), valid_frames, _fp(r["mel"]), _fp(r["planes"]), r["hi"].ctypes.data_as(u16),
            r["lo"].ctypes.data_as(u16), _fp(r["pw"]), _fp(r["melacc"]), _fp(r["raw"]), r["words"].ctypes.data_as(u32),
            _fp(r["maxima"]), _fp(r["basis"]), _fp(r["mel_matrix"])))
        r["hi"], r["lo"] = r["hi"].view(np.float16), r["lo"].view(np.float16)
        return r

    def dbg_log_clipmax(self, melacc, n_mel, t_valid=-1):
        """log_clipmax over melacc [B][T][ld]: (raw [B][n_mel][T], words uint32 [B][4], maxima float32 [B][4])."""
        melacc = _f32(melacc)
        B, T, ld = melacc.shape
        raw = np.full((B, max(n_mel, 0), T), np.nan, np.float32)
        words, maxima = np.zeros((B, 4), np.uint32), np.zeros((B, 4), np.float32)
        self._check(lib().wt_dbg_log_clipmax(self._h, B, T, n_mel, ld, t_valid, _fp(melacc), _fp(raw),
                                             words.ctypes.data_as(POINTER(ctypes.c_uint32)), _fp(maxima)))
        return raw, words, maxima

    @staticmethod
    def clip_max_words(maxima) -> np.ndarray:
        """floats -> the order-preserving words log_clipmax keeps its partial maxima in; -inf -> 0 (never written)."""
        m = np.ascontiguousarray(maxima, dtype=np.float32)
        u = m.view(np.uint32)
        w = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
        return np.where(np.isneginf(m), np.uint32(0), w).astype(np.uint32)

    def dbg_mel_normalize(self, raw, words):
        """mel_normalize over raw [B][n_mel][T] against words uint32 [B][4]; returns the normalised copy."""
        out = np.array(raw, np.float32, order="C")
        B, n_mel, T = out.shape
        words = np.ascontiguousarray(words, dtype=np.uint32)
        assert words.shape == (B, 4)
        self._check(lib().wt_dbg_mel_normalize(self._h, B, T, n_mel, words.ctypes.data_as(POINTER(ctypes.c_uint32)), _fp(out)))
        return out

    def dbg_mel_transpose(self, mel, out, planes=0, scale=1.0):
        """mel [B][C][T] -> a copy of `out` with the kernel's rows written.  planes 0: out float32 [B][T + 2][C]; 1: out
        float16 [2][B][T + 2][ld] (hi, lo); 2: out uint16 [B][T + 2][ld] (bf16 bits)."""
        mel = _f32(mel)
        B, C, T = mel.shape
        out = np.array(out, order="C")
        want = {0: np.float32, 1: np.float16, 2: np.uint16}[planes]
        lead = (2, B, T + 2) if planes == 1 else (B, T + 2)
        if out.dtype != want or out.shape[:-1] != lead:
            raise ValueError("out has the wrong type or shape")
        self._check(lib().wt_dbg_mel_transpose(self._h, planes, B, C, T, out.shape[-1], scale, _fp(mel),
                                               out.ctypes.data_as(c_void_p)))
        return out

    def dbg_pcm_to_planes(self, pcm, planes, out_stride, scale, limit):
        """pcm [batch][n] -> a copy of planes float16 [2][batch * out_stride + guard] with the clips written."""
        pcm = _f32(pcm)
        batch, n = pcm.shape
        planes = np.array(planes, np.float16, order="C")
        if planes.ndim != 2 or planes.shape[0] != 2:
            raise ValueError("planes must be [2][batch * out_stride + guard]")
        guard = planes.shape[1] - batch * out_stride
        self._check(lib().wt_dbg_pcm_to_planes(self._h, batch, n, out_stride, guard, scale, limit, _fp(pcm),
                                               planes.ctypes.data_as(POINTER(ctypes.c_uint16))))
        return planes

    def dbg_gemm_addressed(self, kind, epi, M, N, K, A, a_rpb, a_bs, lda, W, out, c_off, c_rpb, c_bs, ldc, bias=None, pos=None,
                           pos_period=None, out_scale=None, seg=0, kv=(0, 0, 0), n_cu=0, a_len=None, copy=True):
        """An encoder GEMM under the engine's operand / output addressing (wt_dbg_gemm_addressed).  A is one flat float32
        buffer, W [N][K]; `out` is the flat in / out buffer and its type selects the format: float32 [c_len], float16
        [2][c_len] (hi, lo planes; kind 1) or uint16 [c_len] (bf16 bits; kind 2).  Returns the buffer after the launch (a
        copy of `out`, or `out` itself, written in place, with copy=False).  kv = (kv_batch, kv_heads, kv_dmodel)."""
        A, W = _f32(A).reshape(-1), _f32(W)
        if W.shape != (N, K):
            raise ValueError("W must be [N][K]")
        out = np.array(out, order="C") if copy else out
        if not out.flags.c_contiguous:
            raise ValueError("out must be contiguous")
        if out.dtype == np.float32 and out.ndim == 1:
            fmt, c_len = 0, out.shape[0]
        elif out.dtype == np.float16 and out.ndim == 2 and out.shape[0] == 2:
            fmt, c_len = 1, out.shape[1]
        elif out.dtype == np.uint16 and out.ndim == 1:
            fmt, c_len = 2, out.shape[0]
        else:
            raise ValueError("out must be float32 [c_len], float16 [2][c_len] or uint16 [c_len]")
        bias = _f32(bias) if bias is not None else None
        pos = _f32(pos) if pos is not None else None
        if pos_period is None:
            pos_period = pos.shape[0] if pos is not None else 0
        scales = _f32(out_scale if out_scale is not None else [1.0, 1.0, 1.0])
        if scales.shape != (3,):
            raise ValueError("out_scale holds three values")
        self._check(lib().wt_dbg_gemm_addressed(
            self._h, kind, epi, M, N, K, _fp(A), A.shape[0] if a_len is None else a_len, a_rpb, a_bs, lda, _fp(W), _fp(bias),
            _fp(pos), pos_period, fmt, out.ctypes.data_as(c_void_p), c_len, c_off, c_rpb, c_bs, ldc, _fp(scales), seg,
            kv[0], kv[1], kv[2], int(n_cu)))
        return out

    def dbg_gemm_ln_fused(self, family, epi, M, N, K, A, a_rpb, a_bs, lda, W, bias, C, planes, ln_g, ln_b, ln_scale=64.0, pos=None,
                          pos_period=None, y32=None, n_cu=0, c_rpb=1 << 30, c_bs=0, ldc=None, p_out=None, copy=True):
        """An encoder GEMM with the LayerNorm fused into its epilogue and guard rows behind every output
        (wt_dbg_gemm_ln_fused).  family 0 = fp16 planes, 1 = bf16; A is one flat float32 buffer, W [N][K].  C float32
        [M + guard][N] is in / out (epi 5: the residual, in place); planes float16 [2][M + guard][N] (family 0) or uint16
        [M + guard][N] (family 1) and y32 float32 [M + guard][N] or None are in / out too; guard >= 256 rows.  Returns
        SimpleNamespace(C, planes, y32, p_out, flag, fused) of copies after the launch (copy=False: the given arrays
        themselves, written in place)."""
        A, W = _f32(A).reshape(-1), _f32(W)
        if W.shape != (N, K):
            raise ValueError("W must be [N][K]")

        def own(a, dtype):
            if copy:
                return np.array(a, dtype, order="C")
            if a.dtype != dtype or not a.flags.c_contiguous:
                raise ValueError("copy=False needs contiguous arrays of the tap's types")
            return a
        C = own(C, np.float32)
        rows = C.shape[0]
        planes = own(planes, np.uint16 if family else np.float16)
        shape = (rows, N) if family else (2, rows, N)
        if C.shape != (rows, N) or planes.shape != shape:
            raise ValueError("C must be [M + guard][N], planes [2][M + guard][N] float16 or, bf16, [M + guard][N] uint16")
        if y32 is not None:
            y32 = own(y32, np.float32)
            if y32.shape != (rows, N):
                raise ValueError("y32 must be [M + guard][N]")
        if p_out is not None:
            p_out = own(p_out, planes.dtype)
            if p_out.shape != shape:
                raise ValueError("p_out must be laid out like planes")
        pos = _f32(pos) if pos is not None else None
        if pos_period is None:
            pos_period = pos.shape[0] if pos is not None else 0
        u16p = POINTER(ctypes.c_uint16)
        flag, fused = np.full(1, -1, np.int32), np.full(1, -1, np.int32)
        self._check(lib().wt_dbg_gemm_ln_fused(
            self._h, family, epi, M, N, K, _fp(A), A.shape[0], a_rpb, a_bs, lda, _fp(W), _fp(_f32(bias)), _fp(pos), pos_period,
            _fp(_f32(ln_g)) if ln_g is not None else None, _fp(_f32(ln_b)) if ln_b is not None else None, ln_scale, int(n_cu),
            rows - M, c_rpb, c_bs, N if ldc is None else ldc, _fp(C), planes.ctypes.data_as(u16p), _fp(y32),
            p_out.ctypes.data_as(u16p) if p_out is not None else None, _ip32(flag), _ip32(fused)))
        return types.SimpleNamespace(C=C, planes=planes, y32=y32, p_out=p_out, flag=int(flag[0]), fused=bool(fused[0]))

    def dbg_layernorm_planes(self, x, g, b, scale, planes, y32=None, bf16=False, want_flag=True):
        """launch_layernorm_planes over x [M][d].  planes: float16 [2][M * d + guard] (hi, lo) or, bf16, uint16
        [M * d + guard]; y32: float32 [M * d + guard] or None (the kernel then writes no fp32 copy).  Returns copies
        (planes, y32, flag) with the kernel's cells written; flag is None with want_flag=False."""
        x = _f32(x)
        M, d = x.shape
        planes = np.array(planes, np.uint16 if bf16 else np.float16, order="C")
        if planes.shape[:-1] != (() if bf16 else (2,)):
            raise ValueError("planes must be [2][M * d + guard] float16, or [M * d + guard] uint16 with bf16")
        guard = planes.shape[-1] - M * d
        if y32 is not None:
            y32 = np.array(y32, np.float32, order="C")
            if y32.shape != (M * d + guard,):
                raise ValueError("y32 must be [M * d + guard]")
        flag = np.full(1, -1, np.int32)
        self._check(lib().wt_dbg_layernorm_planes(self._h, M, d, _fp(x), _fp(_f32(g)), _fp(_f32(b)), scale, int(bf16), guard,
                                                  planes.ctypes.data_as(POINTER(ctypes.c_uint16)), _fp(y32),
                                                  _ip32(flag) if want_flag else None))
        return planes, y32, (int(flag[0]) if want_flag else None)

    def dbg_f32_to_planes(self, x, scales, seg, planes):
        """launch_f32_to_planes over x [M][ld] -> a copy of planes float16 [2][M * ld + guard] with the rows written."""
        x = _f32(x)
        M, ld = x.shape
        scales = _f32(scales)
        planes = np.array(planes, np.float16, order="C")
        if planes.ndim != 2 or planes.shape[0] != 2 or scales.shape != (3,):
            raise ValueError("planes must be [2][M * ld + guard], scales [3]")
        self._check(lib().wt_dbg_f32_to_planes(self._h, M, ld, _fp(x), _fp(scales), seg, planes.shape[1] - M * ld,
                                               planes.ctypes.data_as(POINTER(ctypes.c_uint16))))
        return planes

    def dbg_encoder_scales(self) -> np.ndarray:
        """What upload_weights derived per contraction (wt_dbg_encoder_scales): float32 [n][10], conv1, conv2, then per layer
        qkv, attention, out, fc1, fc2, then cross-KV.  GEMM rows: a_scale, w_scale, f16_ok, bound, typical; attention rows:
        q, k, v scales, attn_f16_ok, then (bound, typical) of q, k and v."""
        n = c_int(0)
        self._check(lib().wt_dbg_encoder_scales(self._h, None, 0, ctypes.byref(n)))
        rec = np.zeros((n.value, 10), np.float32)
        self._check(lib().wt_dbg_encoder_scales(self._h, _fp(rec), n.value, ctypes.byref(n)))
        return rec

    def dbg_gemm_planes_scaled(self, A, W, bias, out, a_scale, w_scale, epi=1, out_scale=None, seg=0, n_cu=0):
        """launch_gemm_planes on dense A [M][K], W [N][K] with the caller's scales (wt_dbg_gemm_planes_scaled).  `out` is
        the in / out buffer of M + guard rows and selects the form: float32 [M + guard][N] (epi 5: the residual, in place)
        or float16 [2][M + guard][N], the hi and lo planes of column n times out_scale[n // seg].  Returns the buffer
        after the launch, a copy."""
        A, W, bias = _f32(A), _f32(W), _f32(bias)
        (M, K), N = A.shape, W.shape[0]
        out = np.array(out, order="C")
        if out.dtype == np.float32 and out.ndim == 2 and out.shape[1] == N:
            planes, rows = 0, out.shape[0]
        elif out.dtype == np.float16 and out.ndim == 3 and out.shape[0] == 2 and out.shape[2] == N:
            planes, rows = 1, out.shape[1]
        else:
            raise ValueError("out must be float32 [M + guard][N] or float16 [2][M + guard][N]")
        if W.shape != (N, K) or bias.shape != (N,) or rows < M:
            raise ValueError("W must be [N][K], bias [N], and out at least M rows")
        scales = _f32(out_scale if out_scale is not None else [1.0, 1.0, 1.0])
        if scales.shape != (3,):
            raise ValueError("out_scale holds three values")
        self._check(lib().wt_dbg_gemm_planes_scaled(self._h, M, N, K, _fp(A), _fp(W), _fp(bias), epi, a_scale, w_scale,
                                                    _fp(scales), seg, int(n_cu), planes, rows - M, out.ctypes.data_as(c_void_p)))
        return out

    def dbg_encoder_attention_at(self, kind, qkv, batch, T, heads, out, variant=0, scales=None, guard_rows=None, copy=True):
        """An encoder attention launcher (wt_dbg_encoder_attention_at): kind 0 = launch_encoder_attention with `variant`
        0 or 1, 1 = launch_encoder_attention_planes with scales = (q, k, v, out), 2 = launch_encoder_attention_bf16.
        qkv [batch * T + guard_rows][3 * 64 * heads]; guard_rows defaults to the rows qkv has behind batch * T.  `out` is the
        in / out buffer of rows = batch * T + guard_rows rows: float32 [rows][64 * heads] (kind 0), float16 [2][rows][64 *
        heads] (hi, lo planes; kind 1) or uint16 [rows][64 * heads] (bf16 bits; kind 2).  Returns (raw, values): the buffer
        after the launch (a copy of `out`, or `out` itself, written in place, with copy=False) and what it holds as
        float32 [rows][64 * heads]: (hi + lo) / scales[3] for kind 1, the widened bf16 for kind 2."""
        qkv = _f32(qkv)
        d = 64 * heads
        if guard_rows is None:
            guard_rows = qkv.shape[0] - batch * T
        rows = batch * T + guard_rows
        out = np.array(out, order="C") if copy else out
        want = {0: np.float32, 1: np.float16, 2: np.uint16}.get(kind, out.dtype)
        if out.dtype != want or not out.flags.c_contiguous:
            raise ValueError("out must be contiguous float32 (kind 0), float16 (kind 1) or uint16 (kind 2)")
        if qkv.size < max(rows, 0) * 3 * d or out.size < (2 if kind == 1 else 1) * max(rows, 0) * d:
            raise ValueError("qkv or out is shorter than batch * T + guard_rows rows")
        sc = _f32(scales) if scales is not None else None
        if sc is not None and sc.shape != (4,):
            raise ValueError("scales holds four values: q, k, v, out")
        self._check(lib().wt_dbg_encoder_attention_at(self._h, kind, variant, batch, T, heads, guard_rows, _fp(qkv), _fp(sc),
                                                      out.ctypes.data_as(c_void_p)))
        if kind == 1:
            values = (out[0].astype(np.float32) + out[1].astype(np.float32)) / np.float32(sc[3])
        elif kind == 2:
            values = (out.astype(np.uint32) << 16).view(np.float32)
        else:
            values = out
        return out, values.reshape(rows, d)


class DeviceArray:
    """Device buffer owned by the caller, allocated through the engine's C ABI (no HIP runtime on the Python side)."""

    def __init__(self, eng, a):
        a = np.ascontiguousarray(a)
        self._eng, self.shape, self.dtype, self.nbytes = eng, a.shape, a.dtype, a.nbytes
        p = c_void_p()
        eng._check(lib().wt_device_alloc(eng._h, a.nbytes, byref(p)))
        self._p = p
        eng._check(lib().wt_device_upload(eng._h, p, 0, a.ctypes.data_as(c_void_p), a.nbytes))

    def data_ptr(self) -> int:
        return self._p.value

    def download(self):
        out = np.empty(self.shape, self.dtype)
        self._eng._check(lib().wt_device_download(self._eng._h, out.ctypes.data_as(c_void_p), self._p, 0, self.nbytes))
        return out

    def free(self):
        if self._p:
            self._eng._check(lib().wt_device_free(self._eng._h, self._p))
            self._p = None


def create_engine(engine_type, model_prefix: str, vocab_path: str, multilingual: bool):
    """Mirror of ``whisper::create_engine`` (reference whisper.cpp:778-790): returns None
    (after a message on stderr) for an unknown or unsupported engine type."""
    import sys
    try:
        et = EngineType(int(engine_type))
    except ValueError:
        print("Unknown engine-type", file=sys.stderr)
        return None
    return Engine(model_prefix, vocab_path, multilingual, et)
