"""asr-2pass_amd — MI355X-native Paraformer acoustic-model forward behind the FunASR `Model` seam.

The product is the gfx950 shared library `libpfhip.so` (C ABI in include/pfhip.h, sources in csrc/).
This Python module is only the ctypes binding used by the tests and bench.py, plus `ParaformerHip`,
a thin mirror of the reference's plug-in interface (`funasr::Model`, onnxruntime/include/model.h:13-46;
batched contract onnxruntime/src/paraformer-torch.cpp:301-475) with the same method names and error
behaviour.  There is NO CPU fallback: if the HIP library is missing or a HIP call fails, this raises.
"""
from __future__ import annotations

import ctypes
import json
import os
from typing import List, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PFHIP_LIB: another build of the same library (A/B timing of two builds inside one GPU session; tools/ab_bench.sh)
LIB_PATH = os.environ.get("PFHIP_LIB") or os.path.join(_HERE, "libpfhip.so")

PFHIP_NUM_KCLASS = 8
KCLASS_NAMES = ["gemm", "attention", "layernorm", "fsmn", "fbank", "cif", "head", "other"]

# every symbol include/pfhip.h declares (tests check the built library exports exactly these)
ABI_SYMBOLS = [
    "pfhip_last_error", "pfhip_create", "pfhip_create_from_memory", "pfhip_create_from_files", "pfhip_read_model_files", "pfhip_container_blob",
    "pfhip_container_manifest", "pfhip_container_from_cache", "pfhip_container_free", "pfhip_onnx_summary", "pfhip_vad_create_from_files", "pfhip_punc_create_from_files", "pfhip_create_group", "pfhip_group_size", "pfhip_group_stats", "pfhip_destroy",
    "pfhip_sample_rate", "pfhip_vocab_size", "pfhip_feat_dim", "pfhip_d_model", "pfhip_head_dim",
    "pfhip_offline_forward", "pfhip_offline_enqueue", "pfhip_offline_fetch", "pfhip_offline_forward_resident",
    "pfhip_resample_len", "pfhip_resample", "pfhip_offline_forward_rate",
    "pfhip_set_batching", "pfhip_set_inflight", "pfhip_warm_up", "pfhip_get_inflight", "pfhip_inflight_stats", "pfhip_is_contextual", "pfhip_has_timestamp_head", "pfhip_hotword_embed", "pfhip_set_hotwords",
    "pfhip_offline_forward_hwsets", "pfhip_set_hotword_bank_bytes", "pfhip_set_hotword_merging", "pfhip_hotword_bank_stats",
    "pfhip_offline_forward_nbest", "pfhip_set_nbest", "pfhip_offline_fetch_nbest",
    "pfhip_extract_feats", "pfhip_get_tensor", "pfhip_debug_poke", "pfhip_profile_enable", "pfhip_profile_read",
    "pfhip_stream_create", "pfhip_stream_destroy", "pfhip_stream_reset", "pfhip_stream_forward", "pfhip_stream_last_path", "pfhip_stream_forward_batch", "pfhip_set_stream_batching",
    "pfhip_stream_set_debug", "pfhip_stream_get_tensor",
    "pfhip_vad_create_from_memory", "pfhip_vad_destroy", "pfhip_vad_reset", "pfhip_vad_num_classes", "pfhip_vad_forward",
    "pfhip_vad_forward_sil", "pfhip_vad_stream_create", "pfhip_vad_stream_destroy", "pfhip_vad_stream_reset",
    "pfhip_vad_stream_infer", "pfhip_vad_stream_infer_batch", "pfhip_set_vad_stream_batching", "pfhip_vadseg_create", "pfhip_vadseg_destroy", "pfhip_vadseg_reset", "pfhip_vadseg_feed",
    "pfhip_timestamp_onnx", "pfhip_post_process",
    "pfhip_punc_create_from_memory", "pfhip_punc_destroy", "pfhip_punc_num_classes", "pfhip_punc_infer",
    "pfhip_punc_infer_online", "pfhip_punc_infer_batch", "pfhip_set_punc_batching", "pfhip_punc_add_punc",
    # 16-bit PCM in: the same calls on int16 samples (s means s / 32768), bit-identical to their f32 siblings
    "pfhip_offline_forward_s16", "pfhip_offline_forward_hwsets_s16", "pfhip_offline_forward_rate_s16", "pfhip_offline_enqueue_s16",
    "pfhip_offline_forward_resident_s16", "pfhip_vad_forward_sil_s16", "pfhip_stream_forward_s16", "pfhip_stream_forward_batch_s16",
    "pfhip_vad_stream_infer_s16", "pfhip_vad_stream_infer_batch_s16",
    # VAD: the decibel track on the device, files in company
    "pfhip_vad_forward_sil_energy", "pfhip_vad_forward_sil_energy_s16", "pfhip_vad_forward_sil_batch", "pfhip_vad_forward_sil_batch_s16",
    "pfhip_set_vad_batching", "pfhip_vad_batch_stats", "pfhip_vadseg_feed_energy",
    # streaming: candidates, confidences and fire frames per token; the candidates call on 16-bit PCM
    "pfhip_stream_set_detail", "pfhip_stream_last_detail", "pfhip_offline_forward_nbest_s16",
    # offline: fire frames of the CIF scan per token, and token spans from them
    "pfhip_offline_forward_detail", "pfhip_offline_forward_detail_s16", "pfhip_set_fire_frames", "pfhip_offline_fetch_fire_frames",
    "pfhip_lfr_frame_ms", "pfhip_cif_timestamps",
    # SenseVoiceSmall, offline: CTC head over every frame, collapsed on the device
    "pfhip_is_ctc", "pfhip_svs_lid", "pfhip_svs_forward", "pfhip_svs_forward_s16",
    # SenseVoiceSmall: CTC forced alignment of a token sequence against the last forward's rows
    "pfhip_svs_align",
    # SenseVoiceSmall: the forward with the spans of its greedy tokens in the same call
    "pfhip_svs_forward_spans", "pfhip_svs_forward_spans_s16",
    # SenseVoiceSmall: concurrent callers merged into packed forwards
    "pfhip_svs_set_batching",
    # speech quality: the DNSMOS networks
    "pfhip_mos_create_from_files", "pfhip_mos_create_from_memory", "pfhip_mos_destroy", "pfhip_mos_set_workspace", "pfhip_mos_score",
    "pfhip_mos_score_s16", "pfhip_mos_score_windows", "pfhip_mos_score_windows_s16",
    # SenseVoiceSmall: the forward with the CTC prefix beam search (and hotwords) on the device
    "pfhip_svs_forward_beam", "pfhip_svs_forward_beam_s16",
    # CTC prefix beam search: the hotword context graph (host only)
    "pfhip_ctx_graph_create", "pfhip_ctx_graph_destroy", "pfhip_ctx_graph_vocab", "pfhip_ctx_graph_dump",
    # SenseVoiceSmall: a set of search options per utterance, beam callers in the merge queue, the graphs kept on the device
    "pfhip_svs_forward_beam_sets", "pfhip_svs_forward_beam_sets_s16", "pfhip_svs_set_beam_merging", "pfhip_svs_set_graph_bank_bytes",
    "pfhip_svs_graph_bank_stats",
    # hotwords for any Paraformer: the biased beam search over the head's candidates, behind the forward
    "pfhip_offline_forward_bias", "pfhip_offline_forward_bias_s16",
    # token n-gram language model of the device searches (host only)
    "pfhip_lm_graph_create", "pfhip_lm_graph_create_from_arpa", "pfhip_lm_graph_destroy", "pfhip_lm_graph_vocab", "pfhip_lm_graph_order",
    "pfhip_lm_graph_dump", "pfhip_set_token_lm",
]


def _pcm_buffers(din):
    """The utterances of a call as contiguous arrays of ONE sample format, and whether that format is 16-bit PCM: int16 when every
    array is np.int16 (the *_s16 entry points take them as they are), float32 otherwise (int16 arrays among floats become
    s / 32768, which is what the s16 entry points mean by them)."""
    arrs = [np.asarray(x) for x in din]
    if arrs and all(a.dtype == np.int16 for a in arrs):
        return [np.ascontiguousarray(a) for a in arrs], True
    return [_pcm_f32(a) for a in arrs], False


def _pcm_f32(x):
    x = np.asarray(x)
    if x.dtype == np.int16:
        return np.ascontiguousarray(x.astype(np.float32) / np.float32(32768.0))
    return np.ascontiguousarray(x, dtype=np.float32)


class PfhipError(RuntimeError):
    pass


class _Out(ctypes.Structure):
    _fields_ = [
        ("token_ids", ctypes.POINTER(ctypes.c_int32)),
        ("token_num", ctypes.POINTER(ctypes.c_int32)),
        ("n_fires", ctypes.POINTER(ctypes.c_int32)),
        ("n_frames", ctypes.POINTER(ctypes.c_int32)),
        ("logp", ctypes.POINTER(ctypes.c_float)),
        ("max_tokens", ctypes.c_int32),
        ("us_alphas", ctypes.POINTER(ctypes.c_float)),
        ("us_peaks", ctypes.POINTER(ctypes.c_float)),
        ("us_len", ctypes.POINTER(ctypes.c_int32)),
        ("max_us", ctypes.c_int32),
    ]


class _Nbest(ctypes.Structure):
    _fields_ = [("k", ctypes.c_int32), ("ids", ctypes.POINTER(ctypes.c_int32)), ("logp", ctypes.POINTER(ctypes.c_float))]


class _Detail(ctypes.Structure):
    _fields_ = [("nbest_k", ctypes.c_int32), ("nbest_ids", ctypes.POINTER(ctypes.c_int32)), ("nbest_logp", ctypes.POINTER(ctypes.c_float)),
                ("fire_frame", ctypes.POINTER(ctypes.c_int32))]


class _SvsOut(ctypes.Structure):
    _fields_ = [("ids", ctypes.POINTER(ctypes.c_int32)), ("token_num", ctypes.POINTER(ctypes.c_int32)), ("max_tokens", ctypes.c_int),
                ("tok_frame", ctypes.POINTER(ctypes.c_int32)), ("tok_logp", ctypes.POINTER(ctypes.c_float)),
                ("frame_ids", ctypes.POINTER(ctypes.c_int32)), ("frame_logp", ctypes.POINTER(ctypes.c_float)),
                ("frame_len", ctypes.POINTER(ctypes.c_int32)), ("logp", ctypes.POINTER(ctypes.c_float)), ("logp_cap_floats", ctypes.c_size_t)]


class _SvsAlignOut(ctypes.Structure):
    _fields_ = [("tok_begin", ctypes.POINTER(ctypes.c_int32)), ("tok_end", ctypes.POINTER(ctypes.c_int32)),
                ("tok_logp", ctypes.POINTER(ctypes.c_float)), ("score", ctypes.POINTER(ctypes.c_float)), ("max_tokens", ctypes.c_int)]


class _SvsBeamOpts(ctypes.Structure):
    _fields_ = [("first_beam", ctypes.c_int), ("second_beam", ctypes.c_int), ("nbest", ctypes.c_int), ("graph", ctypes.c_void_p)]


class _SvsBeamOut(ctypes.Structure):
    _fields_ = [("n_hyp", ctypes.POINTER(ctypes.c_int32)), ("ids", ctypes.POINTER(ctypes.c_int32)), ("n_tokens", ctypes.POINTER(ctypes.c_int32)),
                ("score", ctypes.POINTER(ctypes.c_float)), ("ctc_score", ctypes.POINTER(ctypes.c_float)),
                ("ctx_score", ctypes.POINTER(ctypes.c_float)), ("max_tokens", ctypes.c_int)]


class _BiasOpts(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int), ("beam", ctypes.c_int), ("nbest", ctypes.c_int), ("graph", ctypes.c_void_p)]


class _BiasOut(ctypes.Structure):
    _fields_ = [("n_hyp", ctypes.POINTER(ctypes.c_int32)), ("ids", ctypes.POINTER(ctypes.c_int32)), ("n_tokens", ctypes.POINTER(ctypes.c_int32)),
                ("score", ctypes.POINTER(ctypes.c_float)), ("am_score", ctypes.POINTER(ctypes.c_float)),
                ("ctx_score", ctypes.POINTER(ctypes.c_float)), ("max_tokens", ctypes.c_int)]


class _StreamDetail(ctypes.Structure):
    _fields_ = [("k", ctypes.c_int32), ("ids", ctypes.POINTER(ctypes.c_int32)), ("logp", ctypes.POINTER(ctypes.c_float)),
                ("fire_frame", ctypes.POINTER(ctypes.c_int32)), ("cap", ctypes.c_int32)]


class _SlotStats(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("context", ctypes.c_int32), ("forwards", ctypes.c_int64),
                ("calls", ctypes.c_int64), ("utterances", ctypes.c_int64)]


class _HwBankStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in ("hits", "misses", "evictions", "refused", "bytes_in_use", "bytes_capacity", "sets_resident",
                                              "forwards", "per_call_forwards", "sets_in_forwards", "max_sets_in_forward")]


class _GraphBankStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in ("hits", "misses", "evictions", "refused", "bytes_in_use", "bytes_capacity", "graphs_resident")]


class _Profile(ctypes.Structure):
    _fields_ = [
        ("ms", ctypes.c_double * PFHIP_NUM_KCLASS),
        ("launches", ctypes.c_int64 * PFHIP_NUM_KCLASS),
        ("flops", ctypes.c_double * PFHIP_NUM_KCLASS),
        ("bytes", ctypes.c_double * PFHIP_NUM_KCLASS),
    ]


_lib = None


def load_lib() -> ctypes.CDLL:
    """Loads libpfhip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PfhipError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = ctypes.CDLL(LIB_PATH)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.pfhip_last_error.restype = ctypes.c_char_p
    lib.pfhip_create.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ci, ctypes.POINTER(vp)]
    lib.pfhip_create_from_memory.argtypes = [vp, ctypes.c_size_t, ctypes.c_char_p, ci, ctypes.POINTER(vp)]
    lib.pfhip_destroy.argtypes = [vp]
    lib.pfhip_destroy.restype = None
    cs = ctypes.c_char_p
    lib.pfhip_create_from_files.argtypes = [cs, cs, cs, cs, cs, ci, ctypes.POINTER(vp)]
    lib.pfhip_vad_create_from_files.argtypes = [cs, cs, cs, ci, ctypes.POINTER(vp)]
    lib.pfhip_punc_create_from_files.argtypes = [cs, cs, ci, ctypes.POINTER(vp)]
    lib.pfhip_read_model_files.argtypes = [cs, cs, cs, cs, cs, cs, ctypes.POINTER(vp)]
    lib.pfhip_container_blob.argtypes = [vp, ctypes.POINTER(ctypes.c_size_t)]
    lib.pfhip_container_blob.restype = vp
    lib.pfhip_container_manifest.argtypes = [vp]
    lib.pfhip_container_manifest.restype = cs
    lib.pfhip_container_from_cache.argtypes = [vp]
    lib.pfhip_container_free.argtypes = [vp]
    lib.pfhip_container_free.restype = None
    lib.pfhip_onnx_summary.argtypes = [cs, ctypes.c_char_p, ctypes.c_size_t]
    lib.pfhip_create_group.argtypes = [vp, ctypes.c_size_t, ctypes.c_char_p, ctypes.POINTER(ci), ci, ctypes.POINTER(vp)]
    lib.pfhip_group_size.argtypes = [vp]
    lib.pfhip_group_stats.argtypes = [vp, vp, vp, vp, vp, ci]
    for f in ("pfhip_sample_rate", "pfhip_vocab_size", "pfhip_feat_dim", "pfhip_d_model", "pfhip_head_dim"):
        getattr(lib, f).argtypes = [vp]
    lib.pfhip_offline_forward.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ci), ci, vp, ci, ctypes.POINTER(_Out)]
    lib.pfhip_offline_enqueue.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ci), ci, vp]
    lib.pfhip_offline_fetch.argtypes = [vp, ctypes.POINTER(_Out)]
    lib.pfhip_offline_forward_resident.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ci), ci, ctypes.POINTER(_Out)]
    lib.pfhip_resample_len.restype = ctypes.c_int64
    lib.pfhip_resample_len.argtypes = [ci, ci, ctypes.c_int64]
    lib.pfhip_resample.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ci), ci, ci, ctypes.POINTER(vp), ctypes.POINTER(ci),
                                   ctypes.POINTER(ci)]
    lib.pfhip_offline_forward_rate.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ci), ci, ci, vp, ci, ctypes.POINTER(_Out)]
    lib.pfhip_op_resample_table.argtypes = [ci, ci, vp, vp, vp, ctypes.c_size_t, ctypes.POINTER(ci), ctypes.POINTER(ci),
                                            ctypes.POINTER(ci)]
    lib.pfhip_extract_feats.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ci), ci, vp, ctypes.c_size_t, vp]
    lib.pfhip_get_tensor.argtypes = [vp, ctypes.c_char_p, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    lib.pfhip_set_batching.argtypes = [vp, ci, ci]
    lib.pfhip_set_inflight.argtypes = [vp, ci]
    lib.pfhip_get_inflight.argtypes = [vp]
    lib.pfhip_warm_up.argtypes = [vp, ci, ci]
    lib.pfhip_inflight_stats.argtypes = [vp, ctypes.POINTER(_SlotStats), ci, ctypes.POINTER(ci)]
    lib.pfhip_is_contextual.argtypes = [vp]
    lib.pfhip_hotword_embed.argtypes = [vp, vp, vp, ci, vp]
    lib.pfhip_set_hotwords.argtypes = [vp, vp, ci]
    if hasattr(lib, "pfhip_offline_forward_hwsets"):          # (an older build loaded through PFHIP_LIB for A/B timing has none of these)
        lib.pfhip_offline_forward_hwsets.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ci), ci, ctypes.POINTER(vp), ctypes.POINTER(ci), ci,
                                                     ctypes.POINTER(ci), ctypes.POINTER(_Out)]
        lib.pfhip_set_hotword_bank_bytes.argtypes = [vp, ctypes.c_int64]
        lib.pfhip_set_hotword_merging.argtypes = [vp, ci]
        lib.pfhip_hotword_bank_stats.argtypes = [vp, ctypes.POINTER(_HwBankStats)]
    if hasattr(lib, "pfhip_offline_forward_nbest"):
        lib.pfhip_offline_forward_nbest.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ci), ci, ctypes.POINTER(vp), ctypes.POINTER(ci), ci,
                                                    ctypes.POINTER(ci), ctypes.POINTER(_Out), ctypes.POINTER(_Nbest)]
        lib.pfhip_set_nbest.argtypes = [vp, ci]
        lib.pfhip_offline_fetch_nbest.argtypes = [vp, ctypes.POINTER(_Nbest)]
    if hasattr(lib, "pfhip_stream_set_detail"):
        lib.pfhip_offline_forward_nbest_s16.argtypes = lib.pfhip_offline_forward_nbest.argtypes
        lib.pfhip_stream_set_detail.argtypes = [vp, ci, ci]
        lib.pfhip_stream_last_detail.argtypes = [vp, ctypes.POINTER(_StreamDetail), ctypes.POINTER(ci)]
    if hasattr(lib, "pfhip_offline_forward_detail"):
        lib.pfhip_offline_forward_detail.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ci), ci, ci, ctypes.POINTER(vp), ctypes.POINTER(ci),
                                                     ci, ctypes.POINTER(ci), ctypes.POINTER(_Out), ctypes.POINTER(_Detail)]
        lib.pfhip_offline_forward_detail_s16.argtypes = lib.pfhip_offline_forward_detail.argtypes
        lib.pfhip_set_fire_frames.argtypes = [vp, ci]
        lib.pfhip_offline_fetch_fire_frames.argtypes = [vp, vp]
        lib.pfhip_lfr_frame_ms.argtypes = [vp]
        lib.pfhip_cif_timestamps.argtypes = [vp, ci, ci, ci, ctypes.c_float, ctypes.c_float, vp, ci, ctypes.POINTER(ci)]
    if hasattr(lib, "pfhip_offline_forward_bias"):
        lib.pfhip_offline_forward_bias.argtypes = lib.pfhip_offline_forward_detail.argtypes + [ctypes.POINTER(_BiasOpts), ci, ctypes.POINTER(ctypes.c_int32),
                                                                                               ctypes.POINTER(_BiasOut)]
        lib.pfhip_offline_forward_bias_s16.argtypes = lib.pfhip_offline_forward_bias.argtypes
    lib.pfhip_stream_create.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(vp)]
    lib.pfhip_stream_destroy.argtypes = [vp]
    lib.pfhip_stream_destroy.restype = None
    lib.pfhip_stream_reset.argtypes = [vp]
    lib.pfhip_stream_forward.argtypes = [vp, vp, ci, ci, vp, ci, ctypes.POINTER(ci)]
    lib.pfhip_stream_last_path.argtypes = [vp]
    lib.pfhip_stream_forward_batch.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp]
    lib.pfhip_set_stream_batching.argtypes = [vp, ci, ci]
    lib.pfhip_stream_set_debug.argtypes = [vp, ci]
    lib.pfhip_stream_get_tensor.argtypes = [vp, ctypes.c_char_p, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    lib.pfhip_vad_create_from_memory.argtypes = [vp, ctypes.c_size_t, ctypes.c_char_p, ci, ctypes.POINTER(vp)]
    lib.pfhip_vad_destroy.argtypes = [vp]
    lib.pfhip_vad_destroy.restype = None
    lib.pfhip_vad_reset.argtypes = [vp]
    lib.pfhip_vad_num_classes.argtypes = [vp]
    lib.pfhip_vad_forward.argtypes = [vp, vp, ci, ci, vp, ctypes.c_size_t, ctypes.POINTER(ci)]
    lib.pfhip_vad_forward_sil.argtypes = [vp, vp, ci, ci, vp, ctypes.c_size_t, ctypes.POINTER(ci)]
    lib.pfhip_vad_stream_create.argtypes = [vp, ctypes.POINTER(vp)]
    lib.pfhip_vad_stream_destroy.argtypes = [vp]
    lib.pfhip_vad_stream_destroy.restype = None
    lib.pfhip_vad_stream_reset.argtypes = [vp]
    lib.pfhip_vad_stream_infer.argtypes = [vp, vp, ci, ci, vp, ctypes.c_size_t, ctypes.POINTER(ci), vp, ctypes.c_size_t, ctypes.POINTER(ci)]
    lib.pfhip_vad_stream_infer_batch.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.pfhip_set_vad_stream_batching.argtypes = [vp, ci, ci]
    lib.pfhip_vadseg_create.argtypes = [ctypes.POINTER(vp)]
    lib.pfhip_vadseg_destroy.argtypes = [vp]
    lib.pfhip_vadseg_destroy.restype = None
    lib.pfhip_vadseg_reset.argtypes = [vp]
    lib.pfhip_vadseg_feed.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, ci, ctypes.c_float, ci, vp, ci, ctypes.POINTER(ci)]
    lib.pfhip_vadseg_feed_energy.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, ctypes.c_float, ci, vp, ci, ctypes.POINTER(ci)]
    lib.pfhip_vad_forward_sil_energy.argtypes = [vp, vp, ci, ci, vp, ctypes.c_size_t, ctypes.POINTER(ci), vp, ctypes.c_size_t, ctypes.POINTER(ci)]
    lib.pfhip_vad_forward_sil_batch.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    lib.pfhip_set_vad_batching.argtypes = [vp, ci, ci]
    lib.pfhip_vad_batch_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ci)]
    lib.pfhip_timestamp_onnx.argtypes = [vp, vp, ci, ci, ctypes.c_float, ctypes.c_float, vp, ci, ctypes.POINTER(ci)]
    lib.pfhip_punc_create_from_memory.argtypes = [vp, ctypes.c_size_t, ctypes.c_char_p, ci, ctypes.POINTER(vp)]
    lib.pfhip_punc_destroy.argtypes = [vp]
    lib.pfhip_punc_destroy.restype = None
    lib.pfhip_punc_num_classes.argtypes = [vp]
    lib.pfhip_punc_infer.argtypes = [vp, vp, ci, vp, vp]
    lib.pfhip_punc_infer_online.argtypes = [vp, vp, ci, ci, vp, vp]
    lib.pfhip_punc_add_punc.argtypes = [vp, vp, ci, vp, ci, ctypes.POINTER(ci)]
    lib.pfhip_punc_infer_batch.argtypes = [vp, vp, vp, vp, ci, vp]
    lib.pfhip_set_punc_batching.argtypes = [vp, ci, ci]
    lib.pfhip_debug_poke.argtypes = [vp, ctypes.c_char_p, ci]
    if hasattr(lib, "pfhip_svs_forward"):
        lib.pfhip_is_ctc.argtypes = [vp]
        lib.pfhip_svs_lid.argtypes = [ctypes.c_char_p]
        lib.pfhip_svs_forward.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ci), ci, ctypes.POINTER(ctypes.c_int32),
                                          ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_SvsOut)]
        lib.pfhip_svs_forward_s16.argtypes = lib.pfhip_svs_forward.argtypes
    if hasattr(lib, "pfhip_svs_align"):
        lib.pfhip_svs_align.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ci), ci, ctypes.POINTER(_SvsAlignOut)]
    if hasattr(lib, "pfhip_svs_forward_spans"):
        lib.pfhip_svs_forward_spans.argtypes = lib.pfhip_svs_forward.argtypes + [ctypes.POINTER(_SvsAlignOut)]
        lib.pfhip_svs_forward_spans_s16.argtypes = lib.pfhip_svs_forward_spans.argtypes
    if hasattr(lib, "pfhip_svs_set_batching"):
        lib.pfhip_svs_set_batching.argtypes = [vp, ci, ci]
    if hasattr(lib, "pfhip_svs_forward_beam"):
        lib.pfhip_svs_forward_beam.argtypes = lib.pfhip_svs_forward.argtypes + [ctypes.POINTER(_SvsBeamOpts), ctypes.POINTER(_SvsBeamOut)]
        lib.pfhip_svs_forward_beam_s16.argtypes = lib.pfhip_svs_forward_beam.argtypes
    if hasattr(lib, "pfhip_svs_forward_beam_sets"):
        lib.pfhip_svs_forward_beam_sets.argtypes = lib.pfhip_svs_forward.argtypes + [ctypes.POINTER(_SvsBeamOpts), ci,
                                                                                     ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_SvsBeamOut)]
        lib.pfhip_svs_forward_beam_sets_s16.argtypes = lib.pfhip_svs_forward_beam_sets.argtypes
        lib.pfhip_svs_set_beam_merging.argtypes = [vp, ci]
        lib.pfhip_svs_set_graph_bank_bytes.argtypes = [vp, ctypes.c_int64]
        lib.pfhip_svs_graph_bank_stats.argtypes = [vp, ctypes.POINTER(_GraphBankStats)]
    if hasattr(lib, "pfhip_ctx_graph_create"):
        i32p, fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
        lib.pfhip_ctx_graph_create.argtypes = [i32p, ctypes.POINTER(ci), fp, ci, ci, ctypes.POINTER(vp)]
        lib.pfhip_ctx_graph_destroy.argtypes = [vp]
        lib.pfhip_ctx_graph_destroy.restype = None
        lib.pfhip_ctx_graph_vocab.argtypes = [vp]
        lib.pfhip_ctx_graph_dump.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci), i32p, fp, ci, i32p, i32p, fp, ci]
    if hasattr(lib, "pfhip_lm_graph_create"):
        i32p, fp, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
        cf = ctypes.c_float
        lib.pfhip_lm_graph_create.argtypes = [ci, ctypes.POINTER(ci), i32p, dp, dp, ci, cf, cf, cf, ctypes.POINTER(vp)]
        lib.pfhip_lm_graph_create_from_arpa.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ci, cf, cf, cf, ctypes.POINTER(vp),
                                                        ctypes.POINTER(ctypes.c_longlong)]
        lib.pfhip_lm_graph_destroy.argtypes = [vp]
        lib.pfhip_lm_graph_destroy.restype = None
        lib.pfhip_lm_graph_vocab.argtypes = [vp]
        lib.pfhip_lm_graph_order.argtypes = [vp]
        lib.pfhip_lm_graph_dump.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci), fp, i32p, ci,
                                            i32p, fp, i32p, ci, i32p, i32p, fp, ci]
        lib.pfhip_set_token_lm.argtypes = [vp, vp]
    lib.pfhip_profile_enable.argtypes = [vp, ci]
    lib.pfhip_profile_read.argtypes = [vp, ctypes.POINTER(_Profile), ci]
    # 16-bit PCM in: the argument lists of the f32 siblings
    for f in ("pfhip_offline_forward", "pfhip_offline_forward_hwsets", "pfhip_offline_forward_rate", "pfhip_offline_enqueue",
              "pfhip_offline_forward_resident", "pfhip_vad_forward_sil", "pfhip_stream_forward", "pfhip_stream_forward_batch",
              "pfhip_vad_stream_infer", "pfhip_vad_stream_infer_batch", "pfhip_vad_forward_sil_energy", "pfhip_vad_forward_sil_batch"):
        getattr(lib, f + "_s16").argtypes = getattr(lib, f).argtypes
    _lib = lib
    return lib


def _check(lib, st):
    if st != 0:
        e = PfhipError(f"pfhip status {st}: {lib.pfhip_last_error().decode()}")
        e.status = int(st)
        raise e


class ContextGraph:
    """The hotword context graph of the CTC prefix beam search (pfhip_ctx_graph_create, include/pfhip.h): words = token-id
    sequences, weights = one weight per token (a sequence per word, or one number per word for every token of it).  Host only:
    no device is needed.  handle: what ops.ctc_prefix_beam passes on; dump(): the CSR arrays."""

    def __init__(self, words, weights, vocab):
        lib = load_lib()
        words = [[int(t) for t in w] for w in words]
        wts = [[float(x)] * len(w) if np.isscalar(x) else [float(y) for y in x] for w, x in zip(words, weights)]
        if len(wts) != len(words) or any(len(a) != len(b) for a, b in zip(words, wts)):
            raise PfhipError("ContextGraph: one weight per token (or per word) is needed")
        ids = np.asarray([t for w in words for t in w] or [0], np.int32)
        tw = np.asarray([x for w in wts for x in w] or [0], np.float32)
        n = np.asarray([len(w) for w in words] or [0], np.int32)
        h = ctypes.c_void_p()
        st = lib.pfhip_ctx_graph_create(ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                        tw.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(words), int(vocab), ctypes.byref(h))
        if st != 0:
            e = PfhipError(f"pfhip_ctx_graph_create: status {st} (an id outside 1 .. vocab - 1, an empty word or a non-finite weight)")
            e.status = int(st)
            raise e
        self._lib, self.handle, self.vocab = lib, h, int(vocab)

    def dump(self):
        """dict(arc_begin [S + 1], escape [S], arc_label, arc_next, arc_weight [A])."""
        lib = self._lib
        ns, na = ctypes.c_int(), ctypes.c_int()
        st = lib.pfhip_ctx_graph_dump(self.handle, ctypes.byref(ns), ctypes.byref(na), None, None, 0, None, None, None, 0)
        assert st == 0
        S, A = ns.value, na.value
        out = dict(arc_begin=np.zeros(S + 1, np.int32), escape=np.zeros(S, np.float32), arc_label=np.zeros(max(A, 1), np.int32),
                   arc_next=np.zeros(max(A, 1), np.int32), arc_weight=np.zeros(max(A, 1), np.float32))
        i32p, fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
        st = lib.pfhip_ctx_graph_dump(self.handle, ctypes.byref(ns), ctypes.byref(na), out["arc_begin"].ctypes.data_as(i32p),
                                      out["escape"].ctypes.data_as(fp), S, out["arc_label"].ctypes.data_as(i32p),
                                      out["arc_next"].ctypes.data_as(i32p), out["arc_weight"].ctypes.data_as(fp), max(A, 1))
        if st != 0:
            raise PfhipError(f"pfhip_ctx_graph_dump: status {st}")
        for key in ("arc_label", "arc_next", "arc_weight"):
            out[key] = out[key][:A]
        return out

    def close(self):
        if self.handle:
            self._lib.pfhip_ctx_graph_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LmGraph:
    """A token n-gram language model for the device searches and ops.lm_score (pfhip_lm_graph_*, include/pfhip.h states the
    automaton and the weight rule).  Host only: no device is needed.  Labels: 0 .. vocab - 1 token ids, vocab </s>, vocab + 1 <s>,
    vocab + 2 <unk>.  Build with from_ngrams or from_arpa.  handle: what the ops pass on; dump(): the arrays; n_skipped: the n-grams
    from_arpa left out for an unknown word."""

    def __init__(self, handle, vocab, n_skipped=0):
        self._lib, self.handle, self.vocab, self.n_skipped = load_lib(), handle, int(vocab), int(n_skipped)
        self.order = int(self._lib.pfhip_lm_graph_order(handle))

    @classmethod
    def from_ngrams(cls, ngrams, vocab, scale=1.0, token_bonus=0.0, oov_log10=-10.0, order=None):
        """ngrams: a sequence of (labels, log10_prob, log10_backoff) in any sequence; order: the longest length (default: what
        ngrams holds, at least 1)."""
        lib = load_lib()
        ngrams = [(tuple(int(t) for t in lab), float(p), float(b)) for lab, p, b in ngrams]
        order = max([len(g[0]) for g in ngrams] + [1]) if order is None else int(order)
        if any(len(g[0]) < 1 or len(g[0]) > order for g in ngrams):
            raise PfhipError("LmGraph.from_ngrams: an n-gram without labels or longer than the order")
        by_len = [[g for g in ngrams if len(g[0]) == n] for n in range(1, order + 1)]
        flat = [g for part in by_len for g in part]
        n = (ctypes.c_int * max(order, 1))(*[len(part) for part in by_len])
        lab = np.asarray([t for g in flat for t in g[0]] or [0], np.int32)
        p = np.asarray([g[1] for g in flat] or [0.0], np.float64)
        b = np.asarray([g[2] for g in flat] or [0.0], np.float64)
        h = ctypes.c_void_p()
        dp = ctypes.POINTER(ctypes.c_double)
        st = lib.pfhip_lm_graph_create(order, n, lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), p.ctypes.data_as(dp), b.ctypes.data_as(dp),
                                       int(vocab), float(scale), float(token_bonus), float(oov_log10), ctypes.byref(h))
        _check(lib, st)
        return cls(h, vocab)

    @classmethod
    def from_arpa(cls, path, tokens, scale=1.0, token_bonus=0.0, oov_log10=-10.0):
        """path: an ARPA file; tokens: the model's token strings (str or bytes), index = token id."""
        lib = load_lib()
        raw = [t if isinstance(t, bytes) else str(t).encode("utf-8") for t in tokens]
        arr = (ctypes.c_char_p * max(len(raw), 1))(*raw)
        h, skipped = ctypes.c_void_p(), ctypes.c_longlong(0)
        st = lib.pfhip_lm_graph_create_from_arpa(os.fsencode(path), arr, len(raw), float(scale), float(token_bonus), float(oov_log10),
                                                 ctypes.byref(h), ctypes.byref(skipped))
        _check(lib, st)
        return cls(h, len(raw), skipped.value)

    def dump(self):
        """dict(start, has_eos, uni_w / uni_next [vocab + 1], arc_begin [S + 1], backoff_w / backoff_state [S], arc_label / arc_next /
        arc_weight [A])."""
        lib = self._lib
        ci = ctypes.c_int
        ns, na, start, eos = ci(), ci(), ci(), ci()
        st = lib.pfhip_lm_graph_dump(self.handle, ctypes.byref(ns), ctypes.byref(na), ctypes.byref(start), ctypes.byref(eos), None, None, 0,
                                     None, None, None, 0, None, None, None, 0)
        _check(lib, st)
        S, A, U = ns.value, na.value, self.vocab + 1
        out = dict(uni_w=np.zeros(U, np.float32), uni_next=np.zeros(U, np.int32), arc_begin=np.zeros(S + 1, np.int32),
                   backoff_w=np.zeros(S, np.float32), backoff_state=np.zeros(S, np.int32), arc_label=np.zeros(max(A, 1), np.int32),
                   arc_next=np.zeros(max(A, 1), np.int32), arc_weight=np.zeros(max(A, 1), np.float32))
        i32p, fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
        ptr = lambda k: out[k].ctypes.data_as(fp if out[k].dtype == np.float32 else i32p)
        st = lib.pfhip_lm_graph_dump(self.handle, ctypes.byref(ns), ctypes.byref(na), ctypes.byref(start), ctypes.byref(eos), ptr("uni_w"),
                                     ptr("uni_next"), U, ptr("arc_begin"), ptr("backoff_w"), ptr("backoff_state"), S, ptr("arc_label"),
                                     ptr("arc_next"), ptr("arc_weight"), max(A, 1))
        if st != 0:
            raise PfhipError(f"pfhip_lm_graph_dump: status {st}")
        for key in ("arc_label", "arc_next", "arc_weight"):
            out[key] = out[key][:A]
        out["start"], out["has_eos"] = start.value, eos.value
        return out

    def close(self):
        if self.handle:
            self._lib.pfhip_lm_graph_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_model_files(kind, model, second=None, hotword=None, cmvn=None, config=None):
    """The reference's own file contract (com-define.h:52-88) -> (manifest dict, float32 blob, from_cache) through the C++ reader
    in libpfhip.so (pfhip_read_model_files); kind in {"asr", "sensevoice", "vad", "punc"}.  No device needed."""
    lib = load_lib()
    enc = lambda s: None if s is None else str(s).encode()
    h = ctypes.c_void_p()
    _check(lib, lib.pfhip_read_model_files(kind.encode(), enc(model), enc(second), enc(hotword), enc(cmvn), enc(config), ctypes.byref(h)))
    try:
        nbytes = ctypes.c_size_t()
        ptr = lib.pfhip_container_blob(h, ctypes.byref(nbytes))
        blob = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_float)), shape=(nbytes.value // 4,)).copy() if nbytes.value else np.zeros(0, np.float32)
        man = json.loads(lib.pfhip_container_manifest(h).decode())
        return man, blob, bool(lib.pfhip_container_from_cache(h))
    finally:
        lib.pfhip_container_free(h)


def resample_len(fs_in, n, fs_out=16000):
    """pfhip_resample_len: samples that n samples at fs_in become at fs_out (Audio::WavResample, flush); -1 if unsupported."""
    return int(load_lib().pfhip_resample_len(int(fs_in), int(fs_out), int(n)))


def resample_table(fs_in, fs_out=16000):
    """pfhip_op_resample_table (host only): (P, first_index int32 [Q], ntaps int32 [Q], weights float32 [Q, K])."""
    lib = load_lib()
    q, k, p = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    if lib.pfhip_op_resample_table(int(fs_in), int(fs_out), None, None, None, 0, ctypes.byref(q), ctypes.byref(k), ctypes.byref(p)):
        raise PfhipError(f"unsupported rate pair {fs_in} -> {fs_out}")
    first = np.zeros(q.value, np.int32)
    nt = np.zeros(q.value, np.int32)
    w = np.zeros((q.value, k.value), np.float32)
    rc = lib.pfhip_op_resample_table(int(fs_in), int(fs_out), first.ctypes.data, nt.ctypes.data, w.ctypes.data, w.size,
                                     ctypes.byref(q), ctypes.byref(k), ctypes.byref(p))
    if rc:
        raise PfhipError(f"pfhip_op_resample_table: {rc}")
    return p.value, first, nt, w


def onnx_summary(path):
    """pfhip_onnx_summary: what the C++ wire-format walk saw in one .onnx file (dict)."""
    lib = load_lib()
    buf = ctypes.create_string_buffer(1024)
    _check(lib, lib.pfhip_onnx_summary(str(path).encode(), buf, len(buf)))
    return json.loads(buf.value.decode())


class ParaformerHip:
    """Host-side mirror of `funasr::Model` for the offline Paraformer path.

    InitAsr   <-> Paraformer::InitAsr          (onnxruntime/src/paraformer.cpp:21-53)
    Forward   <-> Model::Forward(float** din, int* len, bool input_finished, hw_emb, decoder, batch_in)
                  (model.h:31-32; paraformer.cpp:463-589; paraformer-torch.cpp:301-475)
    GetAsrSampleRate / SetBatchSize / GetBatchSize as in model.h:40-42.
    Token ids -> text (Vocab::Vector2StringV2, vocab.cpp:164) is host string handling outside the
    hot path: Forward joins vocabulary entries when a token list is given, else
    returns space-separated ids.
    """

    def __init__(self):
        self._lib = load_lib()
        self._h = ctypes.c_void_p()
        self._batch_size = 1
        self._vocab: Optional[List[str]] = None
        self.cfg = None

    # -- lifetime ----------------------------------------------------------------------------------
    def InitAsr(self, am_model, am_cmvn=None, am_config=None, token_file=None, thread_num=1, device=0, devices=None,
                second_model=None, hw_model=None):
        """am_model: path prefix of `<prefix>.bin/.json`, a (manifest dict, float32 blob) pair, or — with am_cmvn and am_config —
        the string the reference passes (`<dir>/model.onnx`, `model_quant.onnx`, `model.torchscript`; second_model = the online
        model's `decoder.onnx`, hw_model = `model_eb.onnx`): pfhip_create_from_files reads the reference's own files.
        devices=[0, 1, ...]: one replica per listed device behind this one handle (pfhip_create_group)."""
        if self._h:
            self._lib.pfhip_destroy(self._h)
            self._h = ctypes.c_void_p()
        if isinstance(am_model, str) and am_cmvn and am_config and not os.path.exists(am_model + ".bin"):
            enc = lambda s: None if s is None else str(s).encode()
            _check(self._lib, self._lib.pfhip_create_from_files(enc(am_model), enc(second_model), enc(hw_model), enc(am_cmvn), enc(am_config),
                                                                device, ctypes.byref(self._h)))
            self.cfg = read_model_files("asr", am_model, second_model, hw_model, am_cmvn, am_config)[0]["config"]
        elif isinstance(am_model, (tuple, list)):
            man, blob = am_model
            blob = np.ascontiguousarray(blob, dtype=np.float32)
            if devices is not None:
                devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
                _check(self._lib, self._lib.pfhip_create_group(
                    blob.ctypes.data, blob.nbytes, json.dumps(man).encode(), devs, len(devices), ctypes.byref(self._h)))
            else:
                _check(self._lib, self._lib.pfhip_create_from_memory(
                    blob.ctypes.data, blob.nbytes, json.dumps(man).encode(), device, ctypes.byref(self._h)))
            self.cfg = man["config"]
        else:
            _check(self._lib, self._lib.pfhip_create(
                (am_model + ".bin").encode(), (am_model + ".json").encode(), device, ctypes.byref(self._h)))
            with open(am_model + ".json") as f:
                self.cfg = json.load(f)["config"]
        if token_file:
            with open(token_file) as f:
                self._vocab = json.load(f)
        return self

    def close(self):
        if self._h:
            self._lib.pfhip_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def GetAsrSampleRate(self):
        return self._lib.pfhip_sample_rate(self._h)

    def SetBatchSize(self, n):
        self._batch_size = int(n)

    def GetBatchSize(self):
        return self._batch_size

    def group_stats(self):
        """Per replica of the handle: dict(devices, calls, utterances, open_streams) (pfhip_group_stats)."""
        n = self._lib.pfhip_group_size(self._h)
        dev = np.zeros(n, np.int32); calls = np.zeros(n, np.int64); utts = np.zeros(n, np.int64); streams = np.zeros(n, np.int32)
        _check(self._lib, self._lib.pfhip_group_stats(self._h, dev.ctypes.data, calls.ctypes.data, utts.ctypes.data, streams.ctypes.data, n))
        return dict(devices=dev.tolist(), calls=calls.tolist(), utterances=utts.tolist(), open_streams=streams.tolist())

    def set_stream_batching(self, wait_us, max_streams=128):
        """Merge concurrent ParaformerOnlineHip.Forward callers (one thread per connection) into batched forwards."""
        _check(self._lib, self._lib.pfhip_set_stream_batching(self._h, int(wait_us), int(max_streams)))

    def set_batching(self, wait_us, max_utterances=32):
        """Merge concurrent Forward callers into one packed device batch (pfhip_set_batching)."""
        _check(self._lib, self._lib.pfhip_set_batching(self._h, int(wait_us), int(max_utterances)))

    def set_inflight(self, n):
        """n execution contexts per device over the ONE weight set of this handle (pfhip_set_inflight)."""
        _check(self._lib, self._lib.pfhip_set_inflight(self._h, int(n)))

    def get_inflight(self):
        return self._lib.pfhip_get_inflight(self._h)

    def inflight_stats(self):
        """Per execution slot: dict(device, context, forwards, calls, utterances) (pfhip_inflight_stats)."""
        arr = (_SlotStats * 64)()
        n = ctypes.c_int(0)
        _check(self._lib, self._lib.pfhip_inflight_stats(self._h, arr, 64, ctypes.byref(n)))
        return [dict(device=a.device, context=a.context, forwards=a.forwards, calls=a.calls, utterances=a.utterances)
                for a in arr[:n.value]]

    def set_hotword_merging(self, on=True):
        """Contextual callers join the merge queue of set_batching, each with its own hotword sets (pfhip_set_hotword_merging)."""
        _check(self._lib, self._lib.pfhip_set_hotword_merging(self._h, int(bool(on))))

    def set_hotword_bank_bytes(self, nbytes):
        """Bound of the per-device bank of projected hotword sets (pfhip_set_hotword_bank_bytes); call while nothing is in flight."""
        _check(self._lib, self._lib.pfhip_set_hotword_bank_bytes(self._h, int(nbytes)))

    def hotword_bank_stats(self):
        """dict of the pfhip_hwbank_stats fields: hits, misses, evictions, refused, bytes_in_use, bytes_capacity, sets_resident,
        forwards, per_call_forwards, sets_in_forwards, max_sets_in_forward (pfhip_hotword_bank_stats)."""
        st = _HwBankStats()
        _check(self._lib, self._lib.pfhip_hotword_bank_stats(self._h, ctypes.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in _HwBankStats._fields_}

    def StartUtterance(self):  # paraformer.cpp:297-307: stateless
        pass

    def EndUtterance(self):
        pass

    def Reset(self):
        pass

    @property
    def vocab_size(self):
        return self._lib.pfhip_vocab_size(self._h)

    # -- the hot path --------------------------------------------------------------------------------
    def CompileHotwordEmbedding(self, hotword_ids: Sequence[Sequence[int]]):
        """Paraformer::CompileHotwordEmbedding from the id stage on (paraformer.cpp:629-693): each hotword's token ids are
        truncated / zero-padded to 10, the blank row [1,0,...] is appended, the embedder runs on the GPU and row len-1
        is taken.  (Hotword string -> token ids is host text handling, :601-628.)  Returns [H+1, d] float32; a plain
        model returns one zero row (:594-599)."""
        d = self._lib.pfhip_d_model(self._h)
        if not self._lib.pfhip_is_contextual(self._h):
            return np.zeros((1, d), np.float32)
        rows, lens = [], []
        for ids in hotword_ids:
            ids = list(ids)[:10]
            if not ids:
                continue
            rows.append(ids + [0] * (10 - len(ids)))
            lens.append(len(ids))
        rows.append([1] + [0] * 9)
        lens.append(1)
        mat = np.ascontiguousarray(rows, np.int32)
        ln = np.ascontiguousarray(lens, np.int32)
        out = np.zeros((len(rows), d), np.float32)
        _check(self._lib, self._lib.pfhip_hotword_embed(self._h, mat.ctypes.data, ln.ctypes.data, len(rows), out.ctypes.data))
        return out

    def resample(self, din: Sequence[np.ndarray], sample_rate: int):
        """pfhip_resample: Audio::WavResample of each utterance from sample_rate to the model's rate, on the GPU."""
        B = len(din)
        if B == 0:
            raise PfhipError("empty batch")
        fs_out = self.GetAsrSampleRate()
        bufs = [_pcm_f32(x) for x in din]
        n_out = [resample_len(sample_rate, b.shape[0], fs_out) for b in bufs]
        if min(n_out) < 0:
            raise PfhipError(f"unsupported sample rate {sample_rate}")
        outs = [np.zeros(max(n, 1), np.float32) for n in n_out]
        lens = (ctypes.c_int * B)(*[int(b.shape[0]) for b in bufs])
        ptrs = (ctypes.c_void_p * B)(*[b.ctypes.data if b.shape[0] else None for b in bufs])
        optrs = (ctypes.c_void_p * B)(*[o.ctypes.data for o in outs])
        caps = (ctypes.c_int * B)(*[o.shape[0] for o in outs])
        got = (ctypes.c_int * B)()
        _check(self._lib, self._lib.pfhip_resample(self._h, ptrs, lens, B, int(sample_rate), optrs, caps, got))
        return [o[:got[b]] for b, o in enumerate(outs)]

    def forward_ids(self, din: Sequence[np.ndarray], want_logp=False, max_tokens=None, hw_emb=None, want_timestamps=False,
                    sample_rate=None, hw_sets=None, set_of_utt=None, nbest=None, nbest_fill=0, nbest_s16=False,
                    want_fire_frames=False, fire_fill=-1, bias_sets=None, set_of=None, bias_max_tokens=None):
        """Batched forward.  Returns dict(token_num, n_fires, n_frames, ids=list of int arrays,
        logp=list of [n_fires, V] arrays or None[, us_alphas, us_peaks = lists of [3*T_b] arrays]).
        hw_emb: one hotword set [H, d] for the whole batch.  hw_sets + set_of_utt: a list of sets ([H_k, d] each) and, per
        utterance, the index of the set it attends to (pfhip_offline_forward_hwsets); not together with hw_emb or sample_rate.
        sample_rate: the rate of din when it is not the model's (pfhip_offline_forward_rate resamples on the GPU first).
        nbest=k (1..8): also nbest_ids / nbest_logp [batch, max_tokens, k], the k best columns of every token row and their
        log-probabilities (pfhip_offline_forward_nbest; rows >= n_fires keep nbest_fill); not together with sample_rate.
        nbest_s16: np.int16 utterances go to pfhip_offline_forward_nbest_s16 as they are instead of being converted here.
        want_fire_frames: also fire_frame [batch, max_tokens] int32, the LFR row each token row fired in (n_frames[b] = the tail slot;
        rows >= n_fires keep fire_fill), through pfhip_offline_forward_detail — which takes nbest, hw_sets and sample_rate together.
        bias_sets: the same call plus the hotword-biased beam search over the head's candidates (pfhip_offline_forward_bias; an
        extension that works on any Paraformer): a sequence of (width, beam, nbest, graph) with graph a ContextGraph or None, and
        set_of: per utterance the index of its set, -1 for no search (default: every utterance on set 0).  The result then also holds
        bias=dict(n_hyp [B], ids [B, stride, bias_max_tokens] (-1 where nothing was written), n_tokens, score, am_score, ctx_score
        [B, stride]) with stride the largest nbest among the sets in use, and hyps: per utterance the list of (ids, score, am_score,
        ctx_score).  np.int16 utterances go to the _s16 entry point as they are."""
        B = len(din)
        if B == 0:
            raise PfhipError("empty batch")
        # np.int16 utterances go to the *_s16 entry points as they are (with nbest only where nbest_s16 asks for it: floats otherwise)
        bufs, s16 = _pcm_buffers(din) if nbest is None or nbest_s16 or bias_sets is not None else ([_pcm_f32(x) for x in din], False)
        sfx = "_s16" if s16 else ""
        lens = (ctypes.c_int * B)(*[int(b.shape[0]) for b in bufs])
        ptrs = (ctypes.c_void_p * B)(*[b.ctypes.data if b.shape[0] else None for b in bufs])
        n_model = [int(b.shape[0]) for b in bufs]
        if sample_rate is not None:
            n_model = [resample_len(sample_rate, n, self.GetAsrSampleRate()) for n in n_model]
            if min(n_model) < 0:
                raise PfhipError(f"unsupported sample rate {sample_rate}")
        if max_tokens is None:
            max_tokens = max(1, max(n_model) // 960 + 2)   # <= T+1 fires per utterance
        V = self.vocab_size
        ids = np.zeros((B, max_tokens), np.int32)
        tn = np.zeros(B, np.int32)
        nf = np.zeros(B, np.int32)
        fr = np.zeros(B, np.int32)
        logp = np.zeros((B, max_tokens, V), np.float32) if want_logp else None
        out = _Out()
        out.token_ids = ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out.token_num = tn.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out.n_fires = nf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out.n_frames = fr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out.logp = logp.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if want_logp else None
        out.max_tokens = max_tokens
        if want_timestamps:
            max_us = 3 * max(1, max(n_model) // 960 + 2)
            usa = np.zeros((B, max_us), np.float32)
            usp = np.zeros((B, max_us), np.float32)
            usl = np.zeros(B, np.int32)
            out.us_alphas = usa.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
            out.us_peaks = usp.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
            out.us_len = usl.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
            out.max_us = max_us
        hw = np.ascontiguousarray(hw_emb, dtype=np.float32) if hw_emb is not None else None
        hw_ptr, n_hw = (hw.ctypes.data, int(hw.shape[0])) if hw is not None else (None, 0)
        if want_fire_frames or bias_sets is not None:
            if hw_sets is not None and (hw_emb is not None or set_of_utt is None or len(set_of_utt) != B):
                raise PfhipError("hw_sets needs set_of_utt [batch] and excludes hw_emb")
            k = int(nbest) if nbest is not None else 0
            det = _Detail(k, None, None, None)
            if want_fire_frames:
                fire = np.full((B, max_tokens), fire_fill, np.int32)
                det.fire_frame = fire.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
            if nbest is not None:
                nb_ids = np.full((B, max_tokens, max(k, 1)), nbest_fill, np.int32)
                nb_logp = np.full((B, max_tokens, max(k, 1)), nbest_fill, np.float32)
                det.nbest_ids = nb_ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
                det.nbest_logp = nb_logp.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
            sets = [np.ascontiguousarray(h, dtype=np.float32) for h in hw_sets] if hw_sets is not None else ([hw] if hw is not None else [])
            sptr = (ctypes.c_void_p * max(len(sets), 1))(*[h.ctypes.data if h.size else None for h in sets])
            sn = (ctypes.c_int * max(len(sets), 1))(*[int(h.shape[0]) for h in sets])
            sof = (ctypes.c_int * B)(*[int(j) for j in (set_of_utt if hw_sets is not None else [0] * B)])
            args = [self._h, ptrs, lens, B, int(sample_rate) if sample_rate is not None else 0, sptr, sn, len(sets), sof, ctypes.byref(out)]
            if bias_sets is None:
                _check(self._lib, getattr(self._lib, "pfhip_offline_forward_detail" + sfx)(*args, ctypes.byref(det)))
            else:
                i32p, fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
                bias_sets = list(bias_sets)
                bsets = (_BiasOpts * max(len(bias_sets), 1))(*[_BiasOpts(int(w), int(bm), int(n), g.handle if g is not None else None)
                                                               for w, bm, n, g in bias_sets])
                set_of = [0] * B if set_of is None else [int(j) for j in set_of]
                if len(set_of) != B:
                    raise PfhipError("set_of: one entry per utterance")
                stride = max([int(bias_sets[j][2]) for j in set_of if 0 <= j < len(bias_sets)] + [1])
                bmt = max_tokens if bias_max_tokens is None else int(bias_max_tokens)
                b_nhyp = np.full(B, -7, np.int32)
                b_ids = np.full((B, stride, max(bmt, 1)), -1, np.int32)
                b_ntok = np.full((B, stride), -7, np.int32)
                b_score, b_am, b_ctx = (np.full((B, stride), np.nan, np.float32) for _ in range(3))
                bout = _BiasOut(b_nhyp.ctypes.data_as(i32p), b_ids.ctypes.data_as(i32p), b_ntok.ctypes.data_as(i32p), b_score.ctypes.data_as(fp),
                                b_am.ctypes.data_as(fp), b_ctx.ctypes.data_as(fp), bmt)
                bias = dict(n_hyp=b_nhyp, ids=b_ids, n_tokens=b_ntok, score=b_score, am_score=b_am, ctx_score=b_ctx)
                try:
                    _check(self._lib, getattr(self._lib, "pfhip_offline_forward_bias" + sfx)(
                        *args, ctypes.byref(det) if (nbest is not None or want_fire_frames) else None, bsets, len(bias_sets),
                        (ctypes.c_int32 * B)(*set_of), ctypes.byref(bout)))
                except PfhipError as e:
                    e.bias = bias                    # PFHIP_ERR_CAPACITY: n_hyp, n_tokens and the scores were written all the same
                    raise
        elif nbest is not None:
            if sample_rate is not None or (hw_sets is not None and (hw_emb is not None or set_of_utt is None or len(set_of_utt) != B)):
                raise PfhipError("nbest excludes sample_rate; hw_sets needs set_of_utt [batch] and excludes hw_emb")
            k = int(nbest)
            nb_ids = np.full((B, max_tokens, max(k, 1)), nbest_fill, np.int32)
            nb_logp = np.full((B, max_tokens, max(k, 1)), nbest_fill, np.float32)
            nb = _Nbest(k, nb_ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), nb_logp.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
            sets = [np.ascontiguousarray(h, dtype=np.float32) for h in hw_sets] if hw_sets is not None else ([hw] if hw is not None else [])
            sptr = (ctypes.c_void_p * max(len(sets), 1))(*[h.ctypes.data if h.size else None for h in sets])
            sn = (ctypes.c_int * max(len(sets), 1))(*[int(h.shape[0]) for h in sets])
            sof = (ctypes.c_int * B)(*[int(j) for j in (set_of_utt if hw_sets is not None else [0] * B)])
            _check(self._lib, getattr(self._lib, "pfhip_offline_forward_nbest" + sfx)(self._h, ptrs, lens, B, sptr, sn, len(sets), sof,
                                                                                      ctypes.byref(out), ctypes.byref(nb)))
        elif hw_sets is not None:
            if hw_emb is not None or sample_rate is not None or set_of_utt is None or len(set_of_utt) != B:
                raise PfhipError("hw_sets needs set_of_utt [batch] and excludes hw_emb / sample_rate")
            sets = [np.ascontiguousarray(h, dtype=np.float32) for h in hw_sets]
            sptr = (ctypes.c_void_p * max(len(sets), 1))(*[h.ctypes.data if h.size else None for h in sets])
            sn = (ctypes.c_int * max(len(sets), 1))(*[int(h.shape[0]) for h in sets])
            sof = (ctypes.c_int * B)(*[int(k) for k in set_of_utt])
            _check(self._lib, getattr(self._lib, "pfhip_offline_forward_hwsets" + sfx)(self._h, ptrs, lens, B, sptr, sn, len(sets), sof,
                                                                                       ctypes.byref(out)))
        elif sample_rate is None:
            _check(self._lib, getattr(self._lib, "pfhip_offline_forward" + sfx)(self._h, ptrs, lens, B, hw_ptr, n_hw, ctypes.byref(out)))
        else:
            _check(self._lib, getattr(self._lib, "pfhip_offline_forward_rate" + sfx)(self._h, ptrs, lens, B, int(sample_rate), hw_ptr, n_hw,
                                                                                     ctypes.byref(out)))
        res = dict(token_num=tn, n_fires=nf, n_frames=fr,
                   ids=[ids[b, :min(tn[b], nf[b])].copy() for b in range(B)],
                   logp=[logp[b, :nf[b]].copy() for b in range(B)] if want_logp else None)
        if want_timestamps:
            res["us_alphas"] = [usa[b, :usl[b]].copy() for b in range(B)]
            res["us_peaks"] = [usp[b, :usl[b]].copy() for b in range(B)]
        if nbest is not None:
            res["nbest_ids"], res["nbest_logp"] = nb_ids, nb_logp
        if want_fire_frames:
            res["fire_frame"] = fire
        if bias_sets is not None:
            res["bias"] = bias
            res["hyps"] = [[(b_ids[b, j, :b_ntok[b, j]].copy(), float(b_score[b, j]), float(b_am[b, j]), float(b_ctx[b, j]))
                            for j in range(int(b_nhyp[b]))] for b in range(B)]
        return res

    def set_token_lm(self, lm):
        """pfhip_set_token_lm: lm (an LmGraph, or None to remove it) is walked by every search of this handle's forwards from now
        on; its image is copied to the device, so the LmGraph may be closed afterwards.  The model's share of each hypothesis of
        the last search: beam_lm_score()."""
        _check(self._lib, self._lib.pfhip_set_token_lm(self._h, lm.handle if lm is not None else None))

    def beam_lm_score(self, batch, stride):
        """pfhip_get_tensor "beam_lm_score": [batch, stride] — the language model's share of the scores of this thread's last
        searching forward, laid out as that call's score array."""
        return self.get_tensor("beam_lm_score", int(batch) * int(stride)).reshape(int(batch), int(stride))

    def forward_bias(self, din: Sequence[np.ndarray], bias_sets, set_of=None, **kw):
        """forward_ids(din, bias_sets=bias_sets, set_of=set_of, ...): the forward plus the hotword-biased beam search."""
        return self.forward_ids(din, bias_sets=bias_sets, set_of=set_of, **kw)

    def Forward(self, din, len_=None, input_finished=True, hw_emb=None, decoder_handle=None, batch_in=1):
        """Same contract as Model::Forward: returns batch_in strings; an utterance that yields no
        feature frame gives "" (paraformer.cpp:477-480)."""
        din = list(din)[:batch_in]
        if len_ is not None:
            din = [np.asarray(x)[:n] for x, n in zip(din, len_)]
        r = self.forward_ids(din, hw_emb=hw_emb if self._lib.pfhip_is_contextual(self._h) else None)
        res = []
        for ids in r["ids"]:
            if self._vocab is not None:
                res.append("".join(self._vocab[i] for i in ids))
            else:
                res.append(" ".join(str(int(i)) for i in ids))
        return res

    def extract_feats(self, din: Sequence[np.ndarray]):
        """FbankKaldi + LfrCmvn (paraformer.cpp:309-323, 421-461) on the GPU; list of [T_b, 560]."""
        B = len(din)
        bufs = [_pcm_f32(x) for x in din]
        lens = (ctypes.c_int * B)(*[int(b.shape[0]) for b in bufs])
        ptrs = (ctypes.c_void_p * B)(*[b.ctypes.data if b.shape[0] else None for b in bufs])
        fd = self._lib.pfhip_feat_dim(self._h)
        cap = sum(max(0, (int(b.shape[0]) - 400) // 160 + 1 + 5) // 6 + 1 for b in bufs) * fd
        feats = np.zeros(cap, np.float32)
        nfr = np.zeros(B, np.int32)
        _check(self._lib, self._lib.pfhip_extract_feats(self._h, ptrs, lens, B, feats.ctypes.data, cap, nfr.ctypes.data))
        out, o = [], 0
        for b in range(B):
            out.append(feats[o * fd:(o + int(nfr[b])) * fd].reshape(int(nfr[b]), fd).copy())
            o += int(nfr[b])
        return out

    def get_tensor(self, name: str, cap_floats: int) -> np.ndarray:
        buf = np.zeros(cap_floats, np.float32)
        n = ctypes.c_size_t(0)
        _check(self._lib, self._lib.pfhip_get_tensor(self._h, name.encode(), buf.ctypes.data, cap_floats, ctypes.byref(n)))
        return buf[:n.value]

    # -- device-resident form (bench.py) -------------------------------------------------------------
    def enqueue_device(self, d_pcm_ptr: int, sample_off: np.ndarray, n_samples: np.ndarray, stream: int = 0, s16: bool = False):
        """s16: the device buffer holds int16 samples (pfhip_offline_enqueue_s16; sample_off in samples, any alignment)."""
        B = len(n_samples)
        so = np.ascontiguousarray(sample_off, np.int64)
        ns = np.ascontiguousarray(n_samples, np.int32)
        _check(self._lib, (self._lib.pfhip_offline_enqueue_s16 if s16 else self._lib.pfhip_offline_enqueue)(
            self._h, ctypes.c_void_p(d_pcm_ptr), so.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), B, ctypes.c_void_p(stream) if stream else None))

    def fetch(self, B: int, max_tokens: int):
        ids = np.zeros((B, max_tokens), np.int32)
        tn = np.zeros(B, np.int32)
        nf = np.zeros(B, np.int32)
        fr = np.zeros(B, np.int32)
        out = _Out()
        out.token_ids = ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out.token_num = tn.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out.n_fires = nf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out.n_frames = fr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out.logp = None
        out.max_tokens = max_tokens
        _check(self._lib, self._lib.pfhip_offline_fetch(self._h, ctypes.byref(out)))
        return dict(token_num=tn, n_fires=nf, n_frames=fr, ids=[ids[b, :min(tn[b], nf[b])].copy() for b in range(B)])

    def set_nbest(self, k):
        """pfhip_set_nbest: k candidates per token row for the following enqueue_device calls (0 = off)."""
        _check(self._lib, self._lib.pfhip_set_nbest(self._h, int(k)))

    def fetch_nbest(self, B: int, max_tokens: int, k: int, fill=0):
        """pfhip_offline_fetch_nbest after fetch(B, max_tokens): (nbest_ids, nbest_logp) [B, max_tokens, k]."""
        nb_ids = np.full((B, max_tokens, max(int(k), 1)), fill, np.int32)
        nb_logp = np.full((B, max_tokens, max(int(k), 1)), fill, np.float32)
        nb = _Nbest(int(k), nb_ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), nb_logp.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        _check(self._lib, self._lib.pfhip_offline_fetch_nbest(self._h, ctypes.byref(nb)))
        return nb_ids, nb_logp

    def set_fire_frames(self, on=True):
        """pfhip_set_fire_frames: fire frames for the following enqueue_device / forward_resident calls (False = off)."""
        _check(self._lib, self._lib.pfhip_set_fire_frames(self._h, 1 if on else 0))

    def fetch_fire_frames(self, B: int, max_tokens: int, fill=-1):
        """pfhip_offline_fetch_fire_frames after fetch(B, max_tokens) or forward_resident(..., max_tokens): fire_frame [B, max_tokens]."""
        fire = np.full((B, max_tokens), fill, np.int32)
        _check(self._lib, self._lib.pfhip_offline_fetch_fire_frames(self._h, fire.ctypes.data))
        return fire

    def lfr_frame_ms(self):
        return int(self._lib.pfhip_lfr_frame_ms(self._h))

    def forward_resident(self, d_pcm_ptr: int, sample_off: np.ndarray, n_samples: np.ndarray, max_tokens: int, s16: bool = False):
        """pfhip_offline_forward_resident: PCM already in HBM, routed over the handle's execution contexts like Forward.
        s16: the device buffer holds int16 samples (pfhip_offline_forward_resident_s16)."""
        B = len(n_samples)
        so = np.ascontiguousarray(sample_off, np.int64)
        ns = np.ascontiguousarray(n_samples, np.int32)
        ids = np.zeros((B, max_tokens), np.int32)
        tn = np.zeros(B, np.int32)
        nf = np.zeros(B, np.int32)
        fr = np.zeros(B, np.int32)
        out = _Out()
        out.token_ids = ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out.token_num = tn.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out.n_fires = nf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out.n_frames = fr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out.logp = None
        out.max_tokens = max_tokens
        _check(self._lib, (self._lib.pfhip_offline_forward_resident_s16 if s16 else self._lib.pfhip_offline_forward_resident)(
            self._h, ctypes.c_void_p(d_pcm_ptr), so.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), B, ctypes.byref(out)))
        return dict(token_num=tn, n_fires=nf, n_frames=fr, ids=[ids[b, :min(tn[b], nf[b])].copy() for b in range(B)])

    def debug_poke(self, what, value=0):
        """pfhip_debug_poke: test hooks and read-outs ("range_flag", "range_fallbacks", "blstm_fallbacks", "plane_forwards")."""
        return int(self._lib.pfhip_debug_poke(self._h, what.encode(), int(value)))

    def profile_enable(self, on=True):
        """on: False/0 off, True/1 every kernel class, other int = bit mask of classes (see pfhip.h)."""
        _check(self._lib, self._lib.pfhip_profile_enable(self._h, int(on)))

    def profile_read(self, reset=True):
        p = _Profile()
        _check(self._lib, self._lib.pfhip_profile_read(self._h, ctypes.byref(p), 1 if reset else 0))
        return {KCLASS_NAMES[i]: dict(ms=p.ms[i], launches=p.launches[i], flops=p.flops[i], bytes=p.bytes[i])
                for i in range(PFHIP_NUM_KCLASS)}


FIRE_ROW_MS = 60           # one LFR row: lfr_n (6) frame shifts of 10 ms


class ParaformerOnlineHip:
    """Host-side mirror of `funasr::ParaformerOnline` (onnxruntime/src/paraformer-online.cpp): one object per
    connection, built from the (online) model handle like `ParaformerOnline(Model* offline_handle, chunk_size)`
    (:12-62).  Forward(din, len, input_finished) keeps the reference's name and meaning (:525-601) and returns
    the token ids emitted by the call (the reference returns their text)."""

    def __init__(self, offline_handle: ParaformerHip, chunk_size=(5, 10, 5)):
        self._lib = load_lib()
        self._model = offline_handle          # keeps the model alive
        self._h = ctypes.c_void_p()
        cs = (ctypes.c_int * 3)(*chunk_size)
        _check(self._lib, self._lib.pfhip_stream_create(offline_handle.handle, cs, ctypes.byref(self._h)))

    def close(self):
        if self._h:
            if self._model.handle:            # (a model closed first must not be touched through its stream)
                self._lib.pfhip_stream_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def Reset(self):
        _check(self._lib, self._lib.pfhip_stream_reset(self._h))

    def set_debug(self, on=True):
        _check(self._lib, self._lib.pfhip_stream_set_debug(self._h, 1 if on else 0))

    def set_detail(self, k=0, fires=False):
        """pfhip_stream_set_detail: k = 0..8 candidates per token and, with fires, the row each token fired in, for the following
        calls (an extension; 0 / False = off, the default: the calls then launch what they always launched)."""
        _check(self._lib, self._lib.pfhip_stream_set_detail(self._h, int(k), 1 if fires else 0))
        self._detail = (int(k), bool(fires))

    def last_detail(self, k=None, fires=None, cap=256):
        """The detail of the last Forward / forward_batch call of this stream (pfhip_stream_last_detail), parallel to the ids it
        returned: dict(n, ids [n, k] int32, logp [n, k] float32 descending (exp(logp[:, 0]) = the token's confidence),
        fire_frame [n] int32 or None, fire_ms = fire_frame * lfr_n * 10: the fired row's position to within the 25-ms analysis
        window and the 60-ms row).  k / fires default to what set_detail asked for.  A PfhipError carries .status and, where the
        library reported it, .n_tokens (the count a too small cap needed)."""
        dk, df = getattr(self, "_detail", (0, False))
        k = dk if k is None else int(k)
        fires = df if fires is None else bool(fires)
        ids = np.zeros((max(cap, 1), max(k, 1)), np.int32)
        logp = np.zeros((max(cap, 1), max(k, 1)), np.float32)
        ff = np.zeros(max(cap, 1), np.int32)
        d = _StreamDetail(k, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if k else None,
                          logp.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if k else None,
                          ff.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if fires else None, int(cap))
        n = ctypes.c_int(-1)
        try:
            _check(self._lib, self._lib.pfhip_stream_last_detail(self._h, ctypes.byref(d), ctypes.byref(n)))
        except PfhipError as e:
            e.n_tokens = n.value
            raise
        fire = ff[:n.value].copy() if fires else None
        return dict(n=n.value, ids=ids[:n.value, :k].copy(), logp=logp[:n.value, :k].copy(), fire_frame=fire,
                    fire_ms=None if fire is None else fire * FIRE_ROW_MS)

    def last_path(self):
        """Which branch of ParaformerOnline::Forward the last call took (pfhip_stream_last_path): 2 = the one whose non-empty
        text the reference ends with a blank (paraformer-online.cpp:585-587)."""
        return int(self._lib.pfhip_stream_last_path(self._h))

    def Forward(self, din, len_=None, input_finished=False, cap=256):
        (x,), s16 = _pcm_buffers([din if len_ is None else np.asarray(din)[:len_]])
        ids = np.zeros(max(cap, 1), np.int32)
        n = ctypes.c_int(0)
        _check(self._lib, (self._lib.pfhip_stream_forward_s16 if s16 else self._lib.pfhip_stream_forward)(self._h, x.ctypes.data if x.size else None, int(x.size),
                                                         1 if input_finished else 0, ids.ctypes.data, int(cap), ctypes.byref(n)))
        return [int(v) for v in ids[:n.value]]

    @staticmethod
    def forward_batch(streams, dins, input_finished, caps=None):
        """ParaformerOnline::Forward for many connections of one model in one call (pfhip_stream_forward_batch): the chunk
        windows that are ready are packed into one forward.  Returns one id list per stream.  With `caps` (token-buffer
        capacities per stream) returns (status, id lists, n_tokens) instead of raising: a stream whose buffer is too small
        gets no ids and n_tokens = the count it needed, the others are served."""
        B = len(streams)
        if B == 0:
            return []
        lib = streams[0]._lib
        bufs, s16 = _pcm_buffers(dins)
        hs = (ctypes.c_void_p * B)(*[s._h for s in streams])
        ptrs = (ctypes.c_void_p * B)(*[b.ctypes.data if b.size else None for b in bufs])
        lens = (ctypes.c_int * B)(*[int(b.size) for b in bufs])
        fin = (ctypes.c_int * B)(*[1 if f else 0 for f in input_finished])
        ids = np.zeros((B, 256), np.int32)
        idp = (ctypes.c_void_p * B)(*[ids[i].ctypes.data for i in range(B)])
        ccaps = (ctypes.c_int * B)(*([256] * B if caps is None else [int(c) for c in caps]))
        nt = (ctypes.c_int * B)()
        st = (lib.pfhip_stream_forward_batch_s16 if s16 else lib.pfhip_stream_forward_batch)(hs, B, ptrs, lens, fin, idp, ccaps, nt)
        if caps is not None:
            return st, [[int(v) for v in ids[i, :min(nt[i], ccaps[i])]] for i in range(B)], [int(v) for v in nt]
        _check(lib, st)
        return [[int(v) for v in ids[i, :nt[i]]] for i in range(B)]

    def get_tensor(self, name: str, cap_floats: int) -> np.ndarray:
        buf = np.zeros(max(cap_floats, 1), np.float32)
        n = ctypes.c_size_t(0)
        _check(self._lib, self._lib.pfhip_stream_get_tensor(self._h, name.encode(), buf.ctypes.data, cap_floats, ctypes.byref(n)))
        return buf[:n.value]


def svs_lid(svs_lang):
    """pfhip_svs_lid: lid_map of the reference (sensevoice-small.h:121-129); an unknown string gives 0."""
    return int(load_lib().pfhip_svs_lid(None if svs_lang is None else str(svs_lang).encode()))


class SenseVoiceHip:
    """Host-side mirror of the reference's SenseVoiceSmall (onnxruntime/src/sensevoice-small.cpp) for the offline path, beside
    ParaformerHip: InitAsr on a (manifest, blob) container of kind "sensevoice" or a `<prefix>.bin/.json` pair, then forward() =
    pfhip_svs_forward on a packed batch with per-utterance language and text normalisation.  Model widths and wiring are recalled
    from upstream FunASR.  The text assembly of CTCSearch (:348-375) is host string handling above this."""

    def __init__(self):
        self._lib = load_lib()
        self._h = ctypes.c_void_p()
        self.cfg = None

    def InitAsr(self, am_model, am_cmvn=None, am_config=None, device=0):
        """am_model: a (manifest, blob) pair, the path prefix of `<prefix>.bin/.json`, or — with am_cmvn and am_config — the strings
        the reference passes (`<dir>/model.onnx`, `am.mvn`, `config.yaml`): pfhip_create_from_files reads the reference's own files."""
        self.close()
        if isinstance(am_model, str) and am_cmvn and am_config:
            enc = lambda s: str(s).encode()
            _check(self._lib, self._lib.pfhip_create_from_files(enc(am_model), None, None, enc(am_cmvn), enc(am_config), device,
                                                                ctypes.byref(self._h)))
            self.cfg = read_model_files("sensevoice", am_model, None, None, am_cmvn, am_config)[0]["config"]
        elif isinstance(am_model, (tuple, list)):
            man, blob = am_model
            blob = np.ascontiguousarray(blob, dtype=np.float32)
            _check(self._lib, self._lib.pfhip_create_from_memory(blob.ctypes.data, blob.nbytes, json.dumps(man).encode(), device,
                                                                 ctypes.byref(self._h)))
            self.cfg = man["config"]
        else:
            _check(self._lib, self._lib.pfhip_create((am_model + ".bin").encode(), (am_model + ".json").encode(), device,
                                                     ctypes.byref(self._h)))
            with open(am_model + ".json") as f:
                self.cfg = json.load(f)["config"]
        if not self._lib.pfhip_is_ctc(self._h):
            self.close()
            raise PfhipError("not a SenseVoice container (config.kind != \"sensevoice\"): use ParaformerHip")
        return self

    def close(self):
        if self._h:
            self._lib.pfhip_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def GetAsrSampleRate(self):
        return self._lib.pfhip_sample_rate(self._h)

    def set_inflight(self, n):
        _check(self._lib, self._lib.pfhip_set_inflight(self._h, int(n)))

    def set_batching(self, wait_us, max_utterances=32):
        """Merge concurrent forward() callers into one packed device batch (pfhip_svs_set_batching); wait_us = 0: off."""
        _check(self._lib, self._lib.pfhip_svs_set_batching(self._h, int(wait_us), int(max_utterances)))

    def set_beam_merging(self, on):
        """With set_batching on: forward(beam=...) and forward(beam_sets=...) callers join the merge queue too
        (pfhip_svs_set_beam_merging; off by default: every beam call is a forward of its own)."""
        _check(self._lib, self._lib.pfhip_svs_set_beam_merging(self._h, 1 if on else 0))

    def set_token_lm(self, lm):
        """pfhip_set_token_lm: lm (an LmGraph, or None to remove it) is walked by every search of this handle's forwards from now
        on; its image is copied to the device, so the LmGraph may be closed afterwards.  The model's share of each hypothesis of
        the last search: beam_lm_score()."""
        _check(self._lib, self._lib.pfhip_set_token_lm(self._h, lm.handle if lm is not None else None))

    def beam_lm_score(self, batch, stride):
        """pfhip_get_tensor "beam_lm_score": [batch, stride] — the language model's share of the scores of this thread's last
        searching forward, laid out as that call's score array."""
        return self.get_tensor("beam_lm_score", int(batch) * int(stride)).reshape(int(batch), int(stride))

    def set_graph_bank_bytes(self, nbytes):
        """The bound of the device's bank of context graphs (pfhip_svs_set_graph_bank_bytes); 0 banks nothing."""
        _check(self._lib, self._lib.pfhip_svs_set_graph_bank_bytes(self._h, int(nbytes)))

    def graph_bank_stats(self):
        """dict(hits, misses, evictions, refused, bytes_in_use, bytes_capacity, graphs_resident) (pfhip_svs_graph_bank_stats)."""
        st = _GraphBankStats()
        _check(self._lib, self._lib.pfhip_svs_graph_bank_stats(self._h, ctypes.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in _GraphBankStats._fields_}

    def inflight_stats(self):
        """Per execution slot: dict(device, context, forwards, calls, utterances) (pfhip_inflight_stats)."""
        arr = (_SlotStats * 64)()
        n = ctypes.c_int(0)
        _check(self._lib, self._lib.pfhip_inflight_stats(self._h, arr, 64, ctypes.byref(n)))
        return [dict(device=a.device, context=a.context, forwards=a.forwards, calls=a.calls, utterances=a.utterances)
                for a in arr[:n.value]]

    def warm_up(self, batch, n_samples):
        _check(self._lib, self._lib.pfhip_warm_up(self._h, int(batch), int(n_samples)))

    def rows_of(self, n_samples):
        """Rows of one utterance in the packed sequence: ceil(frames / lfr_n) + 4 prompt rows, or 0 without a frame."""
        frames = 0 if n_samples < 400 else 1 + (n_samples - 400) // 160
        T = -(-frames // int(self.cfg.get("lfr_n", 6)))
        return T + 4 if T > 0 else 0

    def forward(self, din, lang="auto", itn=True, lid=None, textnorm=None, want_logp=False, want_spans=False, max_tokens=None,
                beam=None, nbest=None, graph=None, beam_max_tokens=None, beam_sets=None):
        """One packed forward.  beam_sets = [None | (first_beam, second_beam, nbest, graph), ...], one entry per utterance:
        pfhip_svs_forward_beam_sets — every utterance searched with its own beams and ContextGraph (None: not searched, no
        hypotheses), in one head launch and one search launch; the beam_* results are those of `beam`, the hypothesis stride being
        the largest nbest among the entries.  beam = (first_beam, second_beam): pfhip_svs_forward_beam — the CTC prefix beam search on the device,
        with the hotwords of `graph` (a ContextGraph) — and the result also holds beam_n_hyp [B] and, per utterance, beam_ids (a list
        of token arrays, best first; text tokens only), beam_score / beam_ctc_score / beam_ctx_score (arrays over its hypotheses);
        nbest defaults to second_beam.  want_spans: pfhip_svs_forward_spans — the result also holds span_begin / span_end / span_logp
        (per-utterance arrays over the tokens behind the four tags, as align() returns them) and span_score [B].  lang / itn: a value for all utterances or one per utterance (svs_lang strings, booleans); lid /
        textnorm override them with prompt ids.  Returns dict(token_num [B], ids / tok_frame / tok_logp: per-utterance arrays (the four
        leading tag ids included), frame_len [B], frame_ids / frame_logp: per-utterance arrays over its rows, logp: per-utterance
        [rows, vocab] arrays when want_logp)."""
        bufs, s16 = _pcm_buffers(din)
        B = len(bufs)
        per = lambda v: list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * B
        lid = [svs_lid(x) for x in per(lang)] if lid is None else [int(x) for x in per(lid)]
        textnorm = [14 if x else 15 for x in per(itn)] if textnorm is None else [int(x) for x in per(textnorm)]
        ns = np.array([len(b) for b in bufs], np.int32)
        rows = [self.rows_of(int(n)) for n in ns]
        M, cap = int(sum(rows)), max(rows + [1])
        if max_tokens is not None:
            cap = int(max_tokens)                       # the caller's own bound: PFHIP_ERR_CAPACITY below the longest kept sequence
        V = int(self.cfg["vocab"])
        ptrs = (ctypes.c_void_p * B)(*[b.ctypes.data for b in bufs])
        lid_a, tn_a = np.array(lid, np.int32), np.array(textnorm, np.int32)
        ids = np.full((B, cap), -1, np.int32)
        tok_frame = np.full((B, cap), -1, np.int32)
        tok_logp = np.full((B, cap), np.nan, np.float32)
        token_num = np.zeros(B, np.int32)
        frame_len = np.zeros(B, np.int32)
        frame_ids = np.full(max(M, 1), -1, np.int32)
        frame_logp = np.full(max(M, 1), np.nan, np.float32)
        logp = np.zeros((max(M, 1), V), np.float32) if want_logp else None
        i32p, f32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
        out = _SvsOut(ids.ctypes.data_as(i32p), token_num.ctypes.data_as(i32p), cap, tok_frame.ctypes.data_as(i32p),
                      tok_logp.ctypes.data_as(f32p), frame_ids.ctypes.data_as(i32p), frame_logp.ctypes.data_as(f32p),
                      frame_len.ctypes.data_as(i32p), logp.ctypes.data_as(f32p) if want_logp else None, logp.size if want_logp else 0)
        args = [self._h, ptrs, ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), B, lid_a.ctypes.data_as(i32p), tn_a.ctypes.data_as(i32p),
                ctypes.byref(out)]
        if beam_sets is not None:
            if want_spans or beam is not None:
                raise PfhipError("forward: beam_sets goes without beam and want_spans")
            if len(beam_sets) != B:
                raise PfhipError("forward: beam_sets needs one entry per utterance")
            beam = True                                # the results below are read as for `beam`
            distinct, set_of = [], []
            for e in beam_sets:                        # equal entries (the same graph object) share a set
                key = None if e is None else (int(e[0]), int(e[1]), int(e[2]), e[3])
                if key is not None and key not in distinct:
                    distinct.append(key)
                set_of.append(-1 if key is None else distinct.index(key))
            sets_a = (_SvsBeamOpts * max(len(distinct), 1))(*[_SvsBeamOpts(f, s, n, g.handle if g is not None else None)
                                                              for f, s, n, g in distinct])
            set_of_a = np.array(set_of, np.int32)
            nb = max([k[2] for k in distinct] + [1])
        if beam is not None:
            if want_spans:
                raise PfhipError("forward: beam and want_spans are separate calls (align() the returned ids for spans)")
            if beam_sets is None:
                fbm, sbm = int(beam[0]), int(beam[1])
                nb = sbm if nbest is None else int(nbest)
            bmt = cap if beam_max_tokens is None else int(beam_max_tokens)
            nbq = max(nb, 1)
            b_nhyp = np.full(B, -7, np.int32)
            b_ids = np.full((B, nbq, max(bmt, 1)), -1, np.int32)
            b_ntok = np.full((B, nbq), -7, np.int32)
            b_score, b_ctc, b_ctx = (np.full((B, nbq), np.nan, np.float32) for _ in range(3))
            bout = _SvsBeamOut(b_nhyp.ctypes.data_as(i32p), b_ids.ctypes.data_as(i32p), b_ntok.ctypes.data_as(i32p), b_score.ctypes.data_as(f32p),
                               b_ctc.ctypes.data_as(f32p), b_ctx.ctypes.data_as(f32p), max(bmt, 1) if bmt > 0 else 0)
            if beam_sets is not None:
                fn = self._lib.pfhip_svs_forward_beam_sets_s16 if s16 else self._lib.pfhip_svs_forward_beam_sets
                args += [sets_a, max(len(distinct), 1), set_of_a.ctypes.data_as(i32p), ctypes.byref(bout)]
            else:
                bopts = _SvsBeamOpts(fbm, sbm, nb, graph.handle if graph is not None else None)
                fn = self._lib.pfhip_svs_forward_beam_s16 if s16 else self._lib.pfhip_svs_forward_beam
                args += [ctypes.byref(bopts), ctypes.byref(bout)]
            self.last_beam_n_tokens = b_ntok          # also where the call ends in PFHIP_ERR_CAPACITY: the lengths needed
        elif want_spans:
            sp_begin = np.full((B, cap), -7, np.int32)
            sp_end = np.full((B, cap), -7, np.int32)
            sp_logp = np.full((B, cap), np.nan, np.float32)
            sp_score = np.full(B, np.nan, np.float32)
            sp = _SvsAlignOut(sp_begin.ctypes.data_as(i32p), sp_end.ctypes.data_as(i32p), sp_logp.ctypes.data_as(f32p),
                              sp_score.ctypes.data_as(f32p), cap)
            fn = self._lib.pfhip_svs_forward_spans_s16 if s16 else self._lib.pfhip_svs_forward_spans
            args.append(ctypes.byref(sp))
        else:
            fn = self._lib.pfhip_svs_forward_s16 if s16 else self._lib.pfhip_svs_forward
        try:
            _check(self._lib, fn(*args))
        except PfhipError as e:
            if beam is not None:
                e.beam_n_tokens = b_ntok              # this call's own (last_beam_n_tokens is the handle's last: shared among threads)
            raise
        assert frame_len.tolist() == rows, (frame_len.tolist(), rows)
        offs = np.concatenate([[0], np.cumsum(frame_len)]).astype(np.int64)
        cut = lambda a: [a[offs[b]:offs[b + 1]] for b in range(B)]
        res = dict(token_num=token_num, frame_len=frame_len, ids=[ids[b, :token_num[b]] for b in range(B)],
                   tok_frame=[tok_frame[b, :token_num[b]] for b in range(B)], tok_logp=[tok_logp[b, :token_num[b]] for b in range(B)],
                   frame_ids=cut(frame_ids), frame_logp=cut(frame_logp))
        if want_logp:
            res["logp"] = cut(logp)
        if beam is not None:
            hyp = lambda a, b: a[b, :b_nhyp[b]]
            res.update(beam_n_hyp=b_nhyp, beam_ids=[[b_ids[b, j, :b_ntok[b, j]] for j in range(b_nhyp[b])] for b in range(B)],
                       beam_score=[hyp(b_score, b) for b in range(B)], beam_ctc_score=[hyp(b_ctc, b) for b in range(B)],
                       beam_ctx_score=[hyp(b_ctx, b) for b in range(B)])
        if want_spans:
            nt = [max(int(token_num[b]) - 4, 0) for b in range(B)]
            res.update(span_begin=[sp_begin[b, :nt[b]] for b in range(B)], span_end=[sp_end[b, :nt[b]] for b in range(B)],
                       span_logp=[sp_logp[b, :nt[b]] for b in range(B)], span_score=sp_score)
        return res

    def align(self, tokens, max_tokens=None):
        """pfhip_svs_align: CTC forced alignment of tokens[b] (ids after the four leading tags, e.g. forward()["ids"][b][4:]) against
        the rows of this thread's last forward().  Returns dict(begin, end, logp: per-utterance arrays over its tokens — rows in
        tok_frame's numbering, -1 where the utterance is too short for its tokens —, score: [B], -inf for such an utterance)."""
        toks = [np.ascontiguousarray(t, dtype=np.int32) for t in tokens]
        B = len(toks)
        n = np.array([len(t) for t in toks], np.int32)
        cap = max([int(x) for x in n] + [1]) if max_tokens is None else int(max_tokens)
        begin = np.full((B, max(cap, 1)), -1, np.int32)
        end = np.full((B, max(cap, 1)), -1, np.int32)
        logp = np.full((B, max(cap, 1)), np.nan, np.float32)
        score = np.full(max(B, 1), np.nan, np.float32)
        ptrs = (ctypes.c_void_p * max(B, 1))(*[t.ctypes.data for t in toks])
        i32p, f32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
        out = _SvsAlignOut(begin.ctypes.data_as(i32p), end.ctypes.data_as(i32p), logp.ctypes.data_as(f32p), score.ctypes.data_as(f32p), cap)
        _check(self._lib, self._lib.pfhip_svs_align(self._h, ptrs, n.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), B, ctypes.byref(out)))
        return dict(begin=[begin[b, :n[b]] for b in range(B)], end=[end[b, :n[b]] for b in range(B)],
                    logp=[logp[b, :n[b]] for b in range(B)], score=score[:B])

    def get_tensor(self, name: str, cap_floats: int) -> np.ndarray:
        buf = np.zeros(max(cap_floats, 1), np.float32)
        n = ctypes.c_size_t(0)
        _check(self._lib, self._lib.pfhip_get_tensor(self._h, name.encode(), buf.ctypes.data, cap_floats, ctypes.byref(n)))
        return buf[:n.value]

    def debug_poke(self, what, value=0):
        """pfhip_debug_poke: "ctc_unfused", "ctc_unfused_forwards", "ctc_head_chunks", "range_flag", "range_fallbacks", "plane_forwards",
        "svs_span_cap", "svs_unfused_rows", "svs_forward_calls", "svs_topk_k"."""
        return int(self._lib.pfhip_debug_poke(self._h, what.encode(), int(value)))


class FsmnVadHip:
    """Host-side mirror of `funasr::FsmnVad` up to the frame scores (onnxruntime/src/fsmn-vad.cpp): InitVad,
    Forward(waves, is_final) -> probs [T, classes], InitCache.  The E2EVadModel post-processing state machine
    (e2e-vad.h) that turns scores into segments is host logic above this path."""

    def __init__(self):
        self._lib = load_lib()
        self._h = ctypes.c_void_p()

    def InitVad(self, vad_model, vad_cmvn=None, vad_config=None, thread_num=1, device=0):
        man, blob = vad_model
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        _check(self._lib, self._lib.pfhip_vad_create_from_memory(blob.ctypes.data, blob.nbytes, json.dumps(man).encode(),
                                                                 device, ctypes.byref(self._h)))
        return self

    def close(self):
        if self._h:
            self._lib.pfhip_vad_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def InitCache(self):
        _check(self._lib, self._lib.pfhip_vad_reset(self._h))

    def set_stream_batching(self, wait_us, max_streams):
        """Merge concurrent FsmnVadOnlineHip.Infer callers (one thread per connection) into batched device passes."""
        _check(self._lib, self._lib.pfhip_set_vad_stream_batching(self._h, int(wait_us), int(max_streams)))

    def ForwardSil(self, waves, is_final=False):
        """Frame-wise silence posterior only (what E2EVadModel reads).  np.int16 waves go to pfhip_vad_forward_sil_s16."""
        (x,), s16 = _pcm_buffers([waves])
        cap = max(0, (x.size - 400) // 160 + 1) + 1
        sil = np.zeros(cap, np.float32)
        n = ctypes.c_int(0)
        _check(self._lib, (self._lib.pfhip_vad_forward_sil_s16 if s16 else self._lib.pfhip_vad_forward_sil)(self._h, x.ctypes.data if x.size else None, int(x.size),
                                                          1 if is_final else 0, sil.ctypes.data, cap, ctypes.byref(n)))
        return sil[:n.value]

    def ForwardSilEnergy(self, waves, is_final=False):
        """ForwardSil plus the frame energies (sum of squares of every 25-ms frame) of these samples, computed on the device:
        (sil [T], energy [F]).  Feed both to E2EVadModelHost.feed_energy; np.int16 waves go to the s16 entry point as they are."""
        (x,), s16 = _pcm_buffers([waves])
        cap = max(0, (x.size - 400) // 160 + 1) + 1
        sil, eng = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
        n, ne = ctypes.c_int(0), ctypes.c_int(0)
        fn = self._lib.pfhip_vad_forward_sil_energy_s16 if s16 else self._lib.pfhip_vad_forward_sil_energy
        _check(self._lib, fn(self._h, x.ctypes.data if x.size else None, int(x.size), 1 if is_final else 0, sil.ctypes.data, cap,
                             ctypes.byref(n), eng.ctypes.data, cap, ctypes.byref(ne)))
        return sil[:n.value], eng[:ne.value]

    def ForwardSilBatch(self, files):
        """Several COMPLETE files in one device pass, each scored like ForwardSilEnergy(x, is_final=True) on a fresh object (the
        handle's carried caches are not touched): [(sil, energy), ...].  All np.int16 -> the s16 entry point."""
        xs, s16 = _pcm_buffers(files)
        n = len(xs)
        if n == 0:
            return []
        caps = [max(0, (x.size - 400) // 160 + 1) + 1 for x in xs]
        sil = [np.zeros(c, np.float32) for c in caps]
        eng = [np.zeros(c, np.float32) for c in caps]
        ptrs = lambda arrs: (ctypes.c_void_p * n)(*[a.ctypes.data if a.size else None for a in arrs])
        ns = (ctypes.c_int * n)(*[int(x.size) for x in xs])
        cp = (ctypes.c_size_t * n)(*caps)
        nf, ne = (ctypes.c_int * n)(), (ctypes.c_int * n)()
        fn = self._lib.pfhip_vad_forward_sil_batch_s16 if s16 else self._lib.pfhip_vad_forward_sil_batch
        _check(self._lib, fn(self._h, ptrs(xs), ns, n, ptrs(sil), cp, nf, ptrs(eng), cp, ne))
        return [(sil[i][:nf[i]], eng[i][:ne[i]]) for i in range(n)]

    def set_batching(self, wait_us, max_files=32):
        """Merge concurrent ForwardSilEnergy(is_final=True) callers on a handle without carried state into ForwardSilBatch passes
        (pfhip_set_vad_batching); 0 = off."""
        _check(self._lib, self._lib.pfhip_set_vad_batching(self._h, int(wait_us), int(max_files)))

    def batch_stats(self):
        """Packed passes so far: {"passes", "files", "max_files"}."""
        p, f, m = ctypes.c_longlong(0), ctypes.c_longlong(0), ctypes.c_int(0)
        _check(self._lib, self._lib.pfhip_vad_batch_stats(self._h, ctypes.byref(p), ctypes.byref(f), ctypes.byref(m)))
        return {"passes": p.value, "files": f.value, "max_files": m.value}

    def Forward(self, waves, is_final=False):
        x = _pcm_f32(waves)
        C = self._lib.pfhip_vad_num_classes(self._h)
        cap = (max(0, (x.size - 400) // 160 + 1) + 1) * C
        probs = np.zeros(cap, np.float32)
        n = ctypes.c_int(0)
        _check(self._lib, self._lib.pfhip_vad_forward(self._h, x.ctypes.data if x.size else None, int(x.size),
                                                      1 if is_final else 0, probs.ctypes.data, cap, ctypes.byref(n)))
        return probs[:n.value * C].reshape(n.value, C)


class CTTransformerHip:
    """Host-side mirror of `funasr::CTTransformer` for the forward only (onnxruntime/src/ct-transformer.cpp):
    InitPunc, Infer(input_data) -> punctuation ids.  Tokenisation / sentence re-segmentation (AddPunc) are host
    string logic above this path."""

    def __init__(self):
        self._lib = load_lib()
        self._h = ctypes.c_void_p()

    def InitPunc(self, punc_model, punc_config=None, token_file=None, thread_num=1, device=0):
        if isinstance(punc_model, (str, os.PathLike)):
            # the strings the reference passes (`<dir>/model.onnx` and `<dir>/config.yaml`, offline-stream.cpp:111-117), read in libpfhip.so
            enc = lambda p: None if p is None else os.fspath(p).encode()
            _check(self._lib, self._lib.pfhip_punc_create_from_files(enc(punc_model), enc(punc_config), device, ctypes.byref(self._h)))
            return self
        man, blob = punc_model
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        _check(self._lib, self._lib.pfhip_punc_create_from_memory(blob.ctypes.data, blob.nbytes, json.dumps(man).encode(),
                                                                  device, ctypes.byref(self._h)))
        return self

    def close(self):
        if self._h:
            self._lib.pfhip_punc_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def AddPuncIds(self, input_data):
        """The id-level part of CTTransformer::AddPunc (ct-transformer.cpp:39-155): punctuation id per token (+ one appended
        period when the text does not end a sentence)."""
        ids = np.ascontiguousarray(input_data, dtype=np.int32)
        out = np.zeros(ids.size + 1, np.int32)
        n = ctypes.c_int(0)
        _check(self._lib, self._lib.pfhip_punc_add_punc(self._h, ids.ctypes.data, int(ids.size), out.ctypes.data, int(out.size), ctypes.byref(n)))
        return out[:n.value].copy()

    def Infer(self, input_data, want_logits=False, nCacheSize=None):
        """nCacheSize=None: CTTransformer::Infer; an int: CTTransformerOnline::Infer(input_data, nCacheSize)."""
        ids = np.ascontiguousarray(input_data, dtype=np.int32)
        n = int(ids.size)
        punc = np.zeros(n, np.int32)
        C = self._lib.pfhip_punc_num_classes(self._h)
        logits = np.zeros((n, C), np.float32) if want_logits else None
        lp = logits.ctypes.data if want_logits else None
        if nCacheSize is None:
            _check(self._lib, self._lib.pfhip_punc_infer(self._h, ids.ctypes.data, n, punc.ctypes.data, lp))
        else:
            _check(self._lib, self._lib.pfhip_punc_infer_online(self._h, ids.ctypes.data, n, int(nCacheSize), punc.ctypes.data, lp))
        return (punc, logits) if want_logits else punc

    def InferBatch(self, sequences, nCacheSizes=None):
        """Several Infer calls as one packed device pass (pfhip_punc_infer_batch); nCacheSizes: per sequence, realtime model."""
        seqs = [np.ascontiguousarray(x, dtype=np.int32) for x in sequences]
        B = len(seqs)
        outs = [np.zeros(x.size, np.int32) for x in seqs]
        P = ctypes.c_void_p * B
        pi = P(*[x.ctypes.data for x in seqs])
        po = P(*[x.ctypes.data for x in outs])
        ns = (ctypes.c_int * B)(*[int(x.size) for x in seqs])
        cs = (ctypes.c_int * B)(*[int(c) for c in nCacheSizes]) if nCacheSizes is not None else None
        _check(self._lib, self._lib.pfhip_punc_infer_batch(self._h, pi, ns, cs, B, po))
        return outs

    def set_batching(self, wait_us, max_sequences):
        _check(self._lib, self._lib.pfhip_set_punc_batching(self._h, int(wait_us), int(max_sequences)))


class FsmnVadOnlineHip:
    """`funasr::FsmnVadOnline` (onnxruntime/src/fsmn-vad-online.cpp): one per connection, built on an FsmnVadHip like
    `FsmnVadOnline(FsmnVad*)`.  Infer(waves, input_finished) returns the (start_ms, end_ms) pairs of the online detector
    (-1 = open), as `FsmnVadOnline::Infer` does; InferScores stops before the scorer (scores + the waveform it would get)."""

    def __init__(self, vad: "FsmnVadHip", vad_silence_duration=800, vad_max_len=15000, vad_speech_noise_thres=0.8):
        self._lib = load_lib()
        self._vad = vad
        self._h = ctypes.c_void_p()
        _check(self._lib, self._lib.pfhip_vad_stream_create(vad._h, ctypes.byref(self._h)))
        self._scorer = E2EVadModelHost()
        self.vad_silence_duration_, self.vad_max_len_, self.vad_speech_noise_thres_ = vad_silence_duration, vad_max_len, vad_speech_noise_thres

    def close(self):
        if self._h:
            if self._vad._h:                  # a parent closed first (garbage collection order) took its streams' device state with it
                self._lib.pfhip_vad_stream_destroy(self._h)
            self._h = ctypes.c_void_p()
            self._scorer.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def SetConfig(self, vad_tail_sil, vad_max_len):
        self.vad_silence_duration_, self.vad_max_len_ = vad_tail_sil, vad_max_len

    def InferScores(self, waves, input_finished=False):
        (x,), s16 = _pcm_buffers([waves])
        cap = x.size // 160 + 16
        sil = np.zeros(cap, np.float32)
        wv = np.zeros(x.size + 2048, np.float32)
        nf, nw = ctypes.c_int(0), ctypes.c_int(0)
        _check(self._lib, (self._lib.pfhip_vad_stream_infer_s16 if s16 else self._lib.pfhip_vad_stream_infer)(self._h, x.ctypes.data if x.size else None, int(x.size),
                                                           1 if input_finished else 0, sil.ctypes.data, cap, ctypes.byref(nf),
                                                           wv.ctypes.data, wv.size, ctypes.byref(nw)))
        return sil[:nf.value].copy(), wv[:nw.value].copy()

    @staticmethod
    def InferScoresBatch(streams, waves, input_finished):
        """InferScores of several connections (of one FsmnVadHip) as one device pass; returns [(sil, waveform), ...]."""
        n = len(streams)
        lib = streams[0]._lib
        xs, s16 = _pcm_buffers(waves)
        sils = [np.zeros(x.size // 160 + 16, np.float32) for x in xs]
        wvs = [np.zeros(x.size + 2048, np.float32) for x in xs]
        P = ctypes.c_void_p * n
        h = P(*[s._h.value for s in streams])
        px = P(*[x.ctypes.data if x.size else None for x in xs])
        ns = (ctypes.c_int * n)(*[int(x.size) for x in xs])
        fin = (ctypes.c_int * n)(*[1 if f else 0 for f in input_finished])
        ps = P(*[a.ctypes.data for a in sils])
        caps = (ctypes.c_size_t * n)(*[a.size for a in sils])
        pw = P(*[a.ctypes.data for a in wvs])
        wcaps = (ctypes.c_size_t * n)(*[a.size for a in wvs])
        nf, nw = (ctypes.c_int * n)(), (ctypes.c_int * n)()
        _check(lib, (lib.pfhip_vad_stream_infer_batch_s16 if s16 else lib.pfhip_vad_stream_infer_batch)(h, n, px, ns, fin, ps, caps, nf, pw,
                                                                                                       wcaps, nw))
        return [(sils[i][:nf[i]].copy(), wvs[i][:nw[i]].copy()) for i in range(n)]

    def Infer(self, waves, input_finished=False):
        sil, wv = self.InferScores(waves, input_finished)
        if sil.size == 0:
            return []                                                          # fsmn-vad-online.cpp:140-146
        return self._scorer(sil, wv, input_finished, True, self.vad_silence_duration_, self.vad_max_len_,
                            self.vad_speech_noise_thres_, 16000)

    def Reset(self):
        _check(self._lib, self._lib.pfhip_vad_stream_reset(self._h))


class E2EVadModelHost:
    """ctypes handle on the host-side end-point detector (csrc/host/vad_segmenter.cpp), call-compatible with
    `funasr::E2EVadModel::operator()` (onnxruntime/src/e2e-vad.h:303-362) except that it takes the class-0 score
    column instead of the whole score matrix."""

    def __init__(self):
        self._lib = load_lib()
        self._h = ctypes.c_void_p()
        _check(self._lib, self._lib.pfhip_vadseg_create(ctypes.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.pfhip_vadseg_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __call__(self, score_sil, waveform, is_final=False, online=False, max_end_sil=800, max_single_segment_time=15000,
                 speech_noise_thres=0.8, sample_rate=16000):
        sc = np.ascontiguousarray(score_sil, dtype=np.float32)
        wv = np.ascontiguousarray(waveform, dtype=np.float32)
        cap = sc.size + 8
        segs = np.zeros((cap, 2), np.int32)
        n = ctypes.c_int(0)
        _check(self._lib, self._lib.pfhip_vadseg_feed(self._h, sc.ctypes.data if sc.size else None, int(sc.size),
                                                      wv.ctypes.data if wv.size else None, int(wv.size), int(is_final),
                                                      int(online), int(max_end_sil), int(max_single_segment_time),
                                                      float(speech_noise_thres), int(sample_rate), segs.ctypes.data, cap,
                                                      ctypes.byref(n)))
        return [[int(a), int(b)] for a, b in segs[:n.value]]

    def feed_energy(self, score_sil, energy, n_samples, is_final=False, online=False, max_end_sil=800, max_single_segment_time=15000,
                    speech_noise_thres=0.8, sample_rate=16000):
        """The same call with the frame energies of the n_samples new samples (FsmnVadHip.ForwardSilEnergy, ops.frame_energy) in
        place of the waveform (pfhip_vadseg_feed_energy): same segments, no samples on the host."""
        sc = np.ascontiguousarray(score_sil, dtype=np.float32)
        en = np.ascontiguousarray(energy, dtype=np.float32)
        cap = sc.size + 8
        segs = np.zeros((cap, 2), np.int32)
        n = ctypes.c_int(0)
        _check(self._lib, self._lib.pfhip_vadseg_feed_energy(self._h, sc.ctypes.data if sc.size else None, int(sc.size),
                                                             en.ctypes.data if en.size else None, int(en.size), int(n_samples),
                                                             int(is_final), int(online), int(max_end_sil), int(max_single_segment_time),
                                                             float(speech_noise_thres), int(sample_rate), segs.ctypes.data, cap,
                                                             ctypes.byref(n)))
        return [[int(a), int(b)] for a, b in segs[:n.value]]


def timestamp_onnx(us_alphas, us_cif_peak, n_chars, begin_time=0.0, total_offset=-1.5):
    """`funasr::TimestampOnnx` (onnxruntime/src/util.cpp:838-963) through the C ABI: [(begin_s, end_s, is_sil)]."""
    lib = load_lib()
    a = np.ascontiguousarray(us_alphas, dtype=np.float32).copy()
    p = np.ascontiguousarray(us_cif_peak, dtype=np.float32)
    cap = 2 * (n_chars + 4) + 8
    spans = np.zeros((cap, 3), np.float32)
    n = ctypes.c_int(0)
    _check(lib, lib.pfhip_timestamp_onnx(a.ctypes.data, p.ctypes.data, int(p.size), int(n_chars), float(begin_time),
                                         float(total_offset), spans.ctypes.data, cap, ctypes.byref(n)))
    return [(float(s[0]), float(s[1]), bool(s[2])) for s in spans[:n.value]]


def cif_timestamps(fire_frame, n_chars, n_frames, frame_ms=60.0, begin_time=0.0, cap=None):
    """pfhip_cif_timestamps: token spans from the fire frames of the CIF scan (an extension: the reference stamps only through its
    timestamp head): [(begin_s, end_s, is_sil)].  cap: room for that many spans (default: enough)."""
    lib = load_lib()
    f = np.ascontiguousarray(fire_frame, dtype=np.int32)
    cap = 2 * max(int(n_chars), 0) + 2 if cap is None else int(cap)
    spans = np.zeros((max(cap, 1), 3), np.float32)
    n = ctypes.c_int(0)
    rc = lib.pfhip_cif_timestamps(f.ctypes.data if f.size else None, int(f.size), int(n_chars), int(n_frames), float(frame_ms),
                                  float(begin_time), spans.ctypes.data, cap, ctypes.byref(n))
    if rc == 5:      # PFHIP_ERR_CAPACITY: the count it needed travels with the error
        err = PfhipError(f"pfhip status {rc}: {lib.pfhip_last_error().decode()}")
        err.status, err.needed = rc, n.value
        raise err
    _check(lib, rc)
    return [(float(s[0]), float(s[1]), bool(s[2])) for s in spans[:n.value]]


def __getattr__(name):
    # DnsMosHip (dnsmos.py) runs on the operator bindings, which import torch: loaded on first use
    if name == "DnsMosHip":
        from .dnsmos import DnsMosHip
        return DnsMosHip
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
