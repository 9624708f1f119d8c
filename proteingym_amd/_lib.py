"""ctypes binding of libpgmi.so (include/pgmi.h).  No torch import here: the GPU path is
Python -> ctypes -> C ABI -> HIP kernels.  There is no CPU fallback: if the library is missing
or no GPU is visible the calls raise."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libpgmi.so")

ABI_VERSION = 7
ARCH_ESM1B, ARCH_ESM2, ARCH_TRANCEPTION = 1, 2, 3
ARCH_PROGEN2 = 5
ARCH_GPT = 6
ARCH_ESMC = 7
ARCH_SAPROT = 8
ARCH_POET = 9
ARCH_PROGEN3 = 10
ARCH_ESM3 = 11
ARCH_ESMIF1 = 12
ARCH_MULAN = 13
GPT_POS_ROTARY, GPT_POS_LEARNED = 0, 1
PREC_FP32, PREC_BF16, PREC_F16X3 = 0, 1, 2
PRECISIONS = {"fp32": PREC_FP32, "bf16": PREC_BF16, "f16x3": PREC_F16X3}
K_NAMES = ["embed", "layernorm", "gemm_qkv", "attention", "gemm_out", "gemm_fc1", "gemm_fc2",
           "head", "score", "kept_rows", "moe_route", "geom", "cross_attention"]


EINVAL, ENOMEM, EHIP, ENODEV, EPARSE, EOVERFLOW = -1, -2, -3, -4, -5, -6          # include/pgmi.h PGMI_E*


class PgmiError(RuntimeError):
    """A failing C call; ``code`` is its PGMI_E* return value (None when the failure is the binding's own)."""

    def __init__(self, message, code=None):
        super().__init__(message)
        self.code = code


class Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "abi_version", "arch", "layers", "embed_dim", "heads", "ffn_dim", "vocab",
        "max_positions", "token_dropout", "emb_layer_norm_before", "precision", "max_rows")] + [("ln_eps", C.c_float)]


class Pg3Params(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kv_heads", "n_experts", "top_k", "gated")] + [("rope_theta", C.c_float), ("clip_qkv", C.c_float)]


_lib = None

_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_f32p = C.POINTER(C.c_float)
_f64p = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)

# (name, restype, argtypes) -- must list every symbol include/pgmi.h declares
SIGNATURES = [
    ("pgmi_abi_version", C.c_int, []),
    ("pgmi_device_count", C.c_int, []),
    ("pgmi_last_error", C.c_char_p, []),
    ("pgmi_weight_count", C.c_int64, [C.POINTER(Config)]),
    ("pgmi_model_create", C.c_int, [C.POINTER(Config), _f32p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    ("pgmi_model_destroy", None, [C.c_void_p]),
    ("pgmi_model_device", C.c_int, [C.c_void_p]),
    ("pgmi_token_logprobs", C.c_int, [C.c_void_p, _i32p, C.c_int, C.c_int, _f32p]),
    ("pgmi_masked_logprobs", C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, C.c_int, _f32p]),
    ("pgmi_assay_create", C.c_int, [C.c_void_p, _i32p, C.c_int, _i32p, C.c_int, C.c_int,
                                    _i32p, _i32p, _i32p, _i64p, C.c_int64, C.POINTER(C.c_void_p)]),
    ("pgmi_assay_run", C.c_int, [C.c_void_p, C.c_void_p, _f64p, _f32p, C.c_void_p]),
    ("pgmi_assay_destroy", None, [C.c_void_p]),
    ("pgmi_pppl_create", C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), _i64p, C.c_int64, C.POINTER(C.c_void_p)]),
    ("pgmi_pppl_run", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, _f64p, _f32p, C.c_void_p]),
    ("pgmi_pppl_rows", C.c_int64, [C.c_void_p, C.c_int64, C.c_int64]),
    ("pgmi_pppl_stats", C.c_int, [C.c_void_p, _i64p, _i64p, _i64p, _i64p]),
    ("pgmi_pppl_destroy", None, [C.c_void_p]),
    ("pgmi_parse_mutants", C.c_int, [C.c_char_p, _i64p, C.c_int64, C.c_char_p, C.c_int, C.c_int,
                                     _i32p, _i32p, _i32p, _i64p, _i64p]),
    ("pgmi_score_mutants", C.c_int, [_f32p, C.c_int, C.c_int, _i32p, _i32p, _i32p, _i64p, C.c_int64, _f64p]),
    ("pgmi_optimal_window", None, [C.c_int, C.c_int, C.c_int, _i32p, _i32p]),
    ("pgmi_profile_enable", C.c_int, [C.c_void_p, C.c_int]),
    ("pgmi_profile_get", C.c_int, [C.c_void_p, C.c_int, _f64p, _i64p, _f64p, _f64p]),
    ("pgmi_profile_reset", C.c_int, [C.c_void_p]),
    ("pgmi_synchronize", C.c_int, [C.c_void_p]),
    ("pgmi_set_option", C.c_int, [C.c_char_p, C.c_int64]),
    ("pgmi_op_layernorm", C.c_int, [C.c_int, _f32p, _f32p, _f32p, C.c_int, C.c_int, C.c_float, _f32p]),
    ("pgmi_op_gemm", C.c_int, [C.c_int, C.c_int, _f32p, _f32p, _f32p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p]),
    ("pgmi_tr_token_logprobs", C.c_int, [C.c_void_p, _i32p, C.c_int, C.c_int, _f32p]),
    ("pgmi_tr_sequence_loglik", C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, C.c_int, _f32p, C.c_int,
                                          _i32p, _i32p, _i32p, _i32p, C.c_float, _f32p]),
    ("pgmi_tr_sequence_loglik_shared", C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, C.c_int, _f32p, C.c_int,
                                                 _i32p, _i32p, _i32p, _i32p, C.c_float, _f32p, _f32p, _i64p]),
    ("pgmi_tr_sequence_loglik_eve", C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, C.c_int, _f32p, C.c_int,
                                              _i32p, _i32p, _i32p, _i32p, C.c_float, _f32p, C.c_float, C.c_int, _f32p]),
    ("pgmi_tr_sequence_loglik_shared_eve", C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, C.c_int, _f32p, C.c_int,
                                                     _i32p, _i32p, _i32p, _i32p, C.c_float, _f32p, C.c_float, C.c_int, _f32p, _f32p,
                                                     _i64p]),
    ("pgmi_pg2_model_create", C.c_int, [C.POINTER(Config), C.c_int, _f32p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    ("pgmi_pg2_token_logprobs", C.c_int, [C.c_void_p, _i32p, C.c_int, C.c_int, _f32p]),
    ("pgmi_pg2_sequence_loglik", C.c_int, [C.c_void_p, _i32p, C.c_int, C.c_int, _f32p, _i32p]),
    ("pgmi_gpt_weight_count", C.c_int64, [C.POINTER(Config), C.c_int]),
    ("pgmi_gpt_model_create", C.c_int, [C.POINTER(Config), C.c_int, _f32p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    ("pgmi_gpt_token_logprobs", C.c_int, [C.c_void_p, _i32p, C.c_int, C.c_int, _f32p]),
    ("pgmi_gpt_sequence_loglik", C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, C.c_int, _f64p, _i32p]),
    ("pgmi_saprot_model_create", C.c_int, [C.POINTER(Config), C.c_int, _f32p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    ("pgmi_saprot_token_logprobs", C.c_int, [C.c_void_p, _i32p, C.c_int, C.c_int, _f32p]),
    ("pgmi_saprot_group_logprobs", C.c_int, [C.c_void_p, _i32p, C.c_int, _i32p, _i32p, C.c_int, _f32p]),
    ("pgmi_mulan_weight_count", C.c_int64, [C.POINTER(Config)]),
    ("pgmi_mulan_model_create", C.c_int, [C.POINTER(Config), C.c_int, C.c_int, _f32p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    ("pgmi_mulan_set_structure", C.c_int, [C.c_void_p, _f32p, _f32p, C.c_int]),
    ("pgmi_mulan_token_logprobs", C.c_int, [C.c_void_p, _i32p, C.c_int, C.c_int, _i32p, _i32p, _f32p]),
    ("pgmi_mulan_set_logprobs", C.c_int, [C.c_void_p, _i32p, C.c_int, _i32p, _i32p, C.c_int, _f32p]),
    ("pgmi_poet_weight_count", C.c_int64, [C.POINTER(Config), C.c_int]),
    ("pgmi_poet_model_create", C.c_int, [C.POINTER(Config), C.c_int, _f32p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    ("pgmi_poet_set_prompt", C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int]),
    ("pgmi_poet_prompt_logprobs", C.c_int, [C.c_void_p, _f32p]),
    ("pgmi_poet_token_logprobs", C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, C.c_int, _f32p]),
    ("pgmi_poet_sequence_loglik", C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, C.c_int, _f64p]),
    ("pgmi_esmif1_weight_count", C.c_int64, [C.POINTER(Config), C.c_int]),
    ("pgmi_esmif1_model_create", C.c_int, [C.POINTER(Config), C.c_int, _f32p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    ("pgmi_esmif1_set_memory", C.c_int, [C.c_void_p, _f32p, C.c_int]),
    ("pgmi_esmif1_token_logprobs", C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, C.c_int, _f32p]),
    ("pgmi_esmif1_sequence_loglik", C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, C.c_int, _f64p]),
    ("pgmi_pg3_weight_count", C.c_int64, [C.POINTER(Config), C.POINTER(Pg3Params)]),
    ("pgmi_pg3_model_create", C.c_int, [C.POINTER(Config), C.POINTER(Pg3Params), _f32p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    ("pgmi_pg3_token_logprobs", C.c_int, [C.c_void_p, _i32p, C.c_int, C.c_int, _f32p]),
    ("pgmi_pg3_sequence_loglik", C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, C.c_int, _f64p, _i32p]),
    ("pgmi_pg3_routing", C.c_int, [C.c_void_p, C.c_int, C.c_int, _i32p, _f32p]),
    ("pgmi_esm3_weight_count", C.c_int64, [C.POINTER(Config), C.c_int]),
    ("pgmi_esm3_model_create", C.c_int, [C.POINTER(Config), C.c_int, _f32p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    ("pgmi_esm3_set_structure", C.c_int, [C.c_void_p, _i32p, _i32p, _f32p, _f32p, _i32p, C.c_int]),
    ("pgmi_eve_weight_count", C.c_int64, [C.c_void_p]),
    ("pgmi_eve_create", C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    ("pgmi_eve_destroy", None, [C.c_void_p]),
    ("pgmi_eve_profile_model", C.c_void_p, [C.c_void_p]),
    ("pgmi_eve_encode", C.c_int, [C.c_void_p, _u8p, C.c_int, _f32p, _f32p]),
    ("pgmi_eve_elbo", C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int64, C.c_uint64, C.c_int, C.c_void_p, _f32p, _f32p, _f32p]),
    ("pgmi_eve_noise_fill", C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int64, C.c_int, C.c_void_p]),
    ("pgmi_eve_evol_indices", C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_uint64, _f64p, _f64p]),
    ("pgmi_eve_log_prior", C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_uint64, C.c_void_p, _f64p, _f64p]),
    ("pgmi_mpnn_weight_count", C.c_int64, [C.c_void_p]),
    ("pgmi_mpnn_create", C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    ("pgmi_mpnn_destroy", None, [C.c_void_p]),
    ("pgmi_mpnn_profile_model", C.c_void_p, [C.c_void_p]),
    ("pgmi_mpnn_set_structure", C.c_int, [C.c_void_p, _f32p, _f32p, _i32p, _i32p, C.c_int]),
    ("pgmi_mpnn_graph", C.c_int, [C.c_void_p, _i32p, _f32p]),
    ("pgmi_mpnn_encoder", C.c_int, [C.c_void_p, _f32p, _f32p]),
    ("pgmi_mpnn_log_probs", C.c_int, [C.c_void_p, _u8p, _i32p, C.c_int, _f32p]),
    ("pgmi_mpnn_scores", C.c_int, [C.c_void_p, _u8p, _i32p, C.c_int, _f64p]),
    ("pgmi_s2f_weight_count", C.c_int64, [C.c_void_p]),
    ("pgmi_s2f_create", C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    ("pgmi_s2f_destroy", None, [C.c_void_p]),
    ("pgmi_s2f_profile_model", C.c_void_p, [C.c_void_p]),
    ("pgmi_s2f_set_structure", C.c_int, [C.c_void_p, _f32p, _f32p, C.c_int]),
    ("pgmi_s2f_graph", C.c_int, [C.c_void_p, _i32p, _i32p, _i32p, _f32p, _f32p]),
    ("pgmi_s2f_gvp_forward", C.c_int, [C.c_void_p, _f32p, _f32p, C.c_int, _f32p, _f32p, _f32p]),
    ("pgmi_s2f_set_logprobs", C.c_int, [C.c_void_p, _i32p, C.c_int, _i32p, _i32p, _i32p, C.c_int, _f32p, _f32p]),
    ("pgmi_s3f_weight_count", C.c_int64, [C.c_void_p]),
    ("pgmi_s3f_create", C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    ("pgmi_s3f_destroy", None, [C.c_void_p]),
    ("pgmi_s3f_profile_model", C.c_void_p, [C.c_void_p, C.c_int]),
    ("pgmi_s3f_set_structure", C.c_int, [C.c_void_p, _f32p, _f32p, C.c_int, _f32p, _f32p, C.c_int]),
    ("pgmi_s3f_graph", C.c_int, [C.c_void_p, _i32p, _i32p, _i32p, _f32p, _f32p, _i32p, _i32p, _f32p, _f32p, _f32p]),
    ("pgmi_s3f_gvp_forward", C.c_int, [C.c_void_p, _f32p, _f32p, C.c_int, _i32p, C.c_int, _f32p, _f32p, _f32p, _f32p]),
    ("pgmi_s3f_set_logprobs", C.c_int, [C.c_void_p, _i32p, C.c_int, _i32p, _i32p, _i32p, C.c_int, _i32p, C.c_int, _f32p, _f32p]),
    ("pgmi_unirep_weight_count", C.c_int64, [C.c_void_p]),
    ("pgmi_unirep_model_create", C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    ("pgmi_unirep_destroy", None, [C.c_void_p]),
    ("pgmi_unirep_profile_model", C.c_void_p, [C.c_void_p]),
    ("pgmi_unirep_set_target", C.c_int, [C.c_void_p, _i32p, C.c_int]),
    ("pgmi_unirep_sequence_nll", C.c_int, [C.c_void_p, _i32p, _i64p, C.c_int64, C.c_int, _f64p, _i64p]),
    ("pgmi_unirep_token_logprobs", C.c_int, [C.c_void_p, _i32p, C.c_int, _f32p]),
    ("pgmi_op_mlstm_step", C.c_int, [C.c_void_p, _f32p, _f32p, _i32p, C.c_int, _f32p, _f32p, _f32p]),
    ("pgmi_carp_weight_count", C.c_int64, [C.c_void_p]),
    ("pgmi_carp_create", C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    ("pgmi_carp_destroy", None, [C.c_void_p]),
    ("pgmi_carp_profile_model", C.c_void_p, [C.c_void_p]),
    ("pgmi_carp_token_logprobs", C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, _f32p]),
    ("pgmi_carp_masked_logprobs", C.c_int, [C.c_void_p, _i32p, C.c_int, _i32p, C.c_int, _f32p]),
    ("pgmi_carp_sequence_loglik", C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, _f64p]),
    ("pgmi_op_dilated_conv", C.c_int, [C.c_int, C.c_int, _f32p, _f32p, _f32p, _i32p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p]),
    ("pgmi_op_ln_gelu", C.c_int, [C.c_int, C.c_int, _f32p, _f32p, _f32p, C.c_int, C.c_int, C.c_float, _f32p]),
    ("pgmi_bench_dilated_conv", C.c_int, [C.c_int] * 7 + [_f64p]),
    ("pgmi_protssn_weight_count", C.c_int64, [C.c_void_p]),
    ("pgmi_protssn_create", C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    ("pgmi_protssn_destroy", None, [C.c_void_p]),
    ("pgmi_protssn_profile_model", C.c_void_p, [C.c_void_p]),
    ("pgmi_protssn_set_graph", C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, _i32p, _i32p, _f32p]),
    ("pgmi_protssn_forward", C.c_int, [C.c_void_p, _f32p, _f32p, _f32p]),
    ("pgmi_esm_residue_rows", C.c_int, [C.c_void_p, _i32p, C.c_int, _f32p]),
    ("pgmi_op_egnn_message", C.c_int, [C.c_int, C.c_void_p, _f32p, C.c_int64, _f32p, C.c_int, C.c_int, _i32p, _i32p, _f32p, _f32p, _f32p]),
    ("pgmi_esm_packed_rows", C.c_int, [C.c_void_p, _u8p, _i64p, C.c_int64, C.c_int, _f32p, _i64p]),
    ("pgmi_op_packed_rows_plan", C.c_int, [_i64p, C.c_int64, C.c_int, _i32p, _i32p, _i32p, _i64p]),
    ("pgmi_vespag_weight_count", C.c_int64, [C.c_void_p]),
    ("pgmi_vespag_create", C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    ("pgmi_vespag_destroy", None, [C.c_void_p]),
    ("pgmi_vespag_profile_model", C.c_void_p, [C.c_void_p]),
    ("pgmi_vespag_landscapes", C.c_int, [C.c_void_p, _u8p, _i64p, C.c_int64, _i32p, _f32p, _f32p]),
    ("pgmi_vespag_head", C.c_int, [C.c_void_p, _f32p, _i32p, C.c_int64, _f32p]),
    ("pgmi_op_vespag_head", C.c_int, [C.c_int, C.c_int, _f32p, _f32p, _f32p, _f32p, _f32p, _i32p, C.c_int, C.c_int, C.c_int, C.c_float,
                                      _f32p]),
    ("pgmi_prosst_weight_count", C.c_int64, [C.c_void_p]),
    ("pgmi_prosst_create", C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    ("pgmi_prosst_destroy", None, [C.c_void_p]),
    ("pgmi_prosst_profile_model", C.c_void_p, [C.c_void_p]),
    ("pgmi_prosst_set_structure", C.c_int, [C.c_void_p, _f32p, C.c_int]),
    ("pgmi_prosst_subgraphs", C.c_int, [C.c_void_p, _i64p, _i32p, _f32p, _f32p, _i32p, _i32p, _i32p, _i32p]),
    ("pgmi_op_prosst_subgraphs", C.c_int, [C.c_void_p, _f32p, C.c_int, _i64p] + [_i32p] * 8),
    ("pgmi_prosst_embed", C.c_int, [C.c_void_p, _f32p, _f32p, C.c_int, _f32p, _f32p]),
    ("pgmi_prosst_assign", C.c_int, [C.c_void_p, _f32p, C.c_int, _i32p]),
    ("pgmi_op_prosst_assign", C.c_int, [C.c_int, _f32p, C.c_int64, _f32p, C.c_int, _i32p]),
    ("pgmi_bench_gemm", C.c_int, [C.c_int] * 9 + [_f64p]),
    ("pgmi_bench_gemm_ab", C.c_int, [C.c_int] * 7 + [_i32p, C.c_int, C.c_int, C.c_int, _f64p]),
    ("pgmi_op_attention", C.c_int, [C.c_int, C.c_int, _f32p, _i32p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p]),
    ("pgmi_op_qkln_prep", C.c_int, [C.c_int, _f32p, _f32p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, _f32p, _f64p]),
    ("pgmi_op_causal_attention", C.c_int, [C.c_int, C.c_int, _f32p, _f32p, _f32p, C.c_int, _f32p, _f32p, _f32p, _f32p, _f32p,
                                           C.c_int, C.c_int, C.c_int, _f32p]),
    ("pgmi_op_dense_attention", C.c_int, [C.c_int, C.c_int, _f32p, _f32p, _f32p, C.c_int, _f32p, _f32p, _i32p, C.c_int, C.c_int, C.c_int,
                                          C.c_int, _f32p, _f32p, _f32p]),
    ("pgmi_op_prefix_attention", C.c_int, [C.c_int, _f32p, _i32p, C.c_int, _f32p, C.c_int, C.c_int, C.c_int, _f32p]),
    ("pgmi_op_cross_attention", C.c_int, [C.c_int, _f32p, _i32p, C.c_int, _f32p, C.c_int, C.c_int, C.c_int, _f32p]),
    ("pgmi_op_packed_chunks", C.c_int, [_i32p, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i32p]),
    ("pgmi_op_rmsnorm", C.c_int, [C.c_int, _f32p, _f32p, C.c_int, C.c_int, C.c_float, _f32p]),
    ("pgmi_op_geom_attention", C.c_int, [C.c_int, _f32p, _f32p, _f32p, _i32p, C.c_int, _f32p, _f32p, C.c_int, C.c_int, C.c_int, _f32p]),
    ("pgmi_op_geom_key_tile", C.c_int, [C.c_int]),
    ("pgmi_op_moe", C.c_int, [C.c_int, _f32p, _f32p, _f32p, _f32p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _f32p,
                              _i32p, _f32p]),
    ("pgmi_op_tied_row_attention", C.c_int, [C.c_int, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, _f32p]),
    ("pgmi_op_tied_row_splits", C.c_int, [C.c_int, C.c_int, C.c_int]),
    ("pgmi_op_column_attention", C.c_int, [C.c_int, _f32p, _f32p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p]),
    ("pgmi_op_vocab_logsoftmax", C.c_int, [C.c_int, _f32p, _f32p, _f32p, C.c_int, C.c_int, C.c_int, _f32p, _i32p]),
    ("pgmi_op_wide_logsoftmax", C.c_int, [C.c_int, _f32p, C.c_int, C.c_int, C.c_int, _i32p, _f32p, _i32p]),
    ("pgmi_op_group_logsoftmax", C.c_int, [C.c_int, _f32p, _f32p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _f32p,
                                           _f32p, _i32p]),
    ("pgmi_op_seq_loglik", C.c_int, [C.c_int, _f32p, _i32p, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i32p, _i32p, C.c_int, _f32p, C.c_int,
                                     _i32p, _i32p, _i32p, _i32p, C.c_float, _f32p, C.c_float, C.c_int, _f32p]),
    ("pgmi_msa_token_logprobs", C.c_int, [C.c_void_p, _i32p, C.c_int, C.c_int, _f32p]),
    ("pgmi_msa_masked_logprobs", C.c_int, [C.c_void_p, _i32p, C.c_int, C.c_int, C.c_int, _i32p, _i32p, C.c_int, _f32p]),
    ("pgmi_msa_cluster_counts", C.c_int, [C.c_int, C.POINTER(C.c_int8), C.c_int64, C.c_int64, C.c_int, C.c_double, _i32p, _f64p]),
    ("pgmi_msa_neighbor_counts", C.c_int, [C.c_int, C.POINTER(C.c_int8), C.c_int64, C.c_int64, C.c_int, C.c_double, _i32p, _f64p]),
]


def load():
    """Load libpgmi.so (building it is __graft_entry__.build()'s / build_native's job)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PgmiError(f"{LIB_PATH} not found: run `python -m proteingym_amd.build_native` "
                        "(hipcc, gfx950).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.pgmi_abi_version() != ABI_VERSION:
        raise PgmiError("libpgmi ABI version mismatch; rebuild")
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        raise PgmiError(f"libpgmi error {rc}: {load().pgmi_last_error().decode(errors='replace')}", code=int(rc))


def ptr(a: np.ndarray, ty):
    return a.ctypes.data_as(ty) if a is not None else None


def as_i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def as_f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class ModelHandle:
    """A device-resident model behind its libpgmi handle.  __init__ builds the Config from cfg's dimensions and the fields the
    subclass passes, checks the blob size against the library's count and creates the model through CREATE; close / __del__ destroy
    it.  pgmi_pg2_model_create, pgmi_gpt_model_create and pgmi_saprot_model_create take arch_arg (ProGen2's rotary_dim, the causal
    decoder's pos_kind, SaProt's <mask> id; a tuple for
    pgmi_mulan_model_create's <mask> id and groups) after the config, and their subclasses name their weight count."""
    CREATE = "pgmi_model_create"

    def __init__(self, cfg: dict, weights: np.ndarray, device: int = 0, max_rows: int = 0, arch_arg=None,
                 precision: int = PREC_F16X3, **fields):
        lib = load()
        self.cfg = dict(cfg)
        self.device = device
        c = Config(abi_version=ABI_VERSION, layers=cfg["layers"], embed_dim=cfg["embed_dim"], heads=cfg["heads"],
                   ffn_dim=cfg["ffn_dim"], precision=precision, max_rows=max_rows, **fields)
        w = as_f32(weights)
        n = self._weight_count(lib, c, arch_arg)
        if w.size != n:
            raise PgmiError(f"weight blob has {w.size} elements, config needs {n}")
        h = C.c_void_p()
        head = (C.byref(c),) if arch_arg is None else (C.byref(c), *arch_arg) if isinstance(arch_arg, tuple) else (C.byref(c), arch_arg)
        check(getattr(lib, self.CREATE)(*head, ptr(w, _f32p), w.size, device, C.byref(h)))
        self._h = h

    @staticmethod
    def _weight_count(lib, c, arch_arg):
        return lib.pgmi_weight_count(C.byref(c))

    def close(self):
        if getattr(self, "_h", None):
            load().pgmi_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _ProfileView:
    """A pgmi_model handle (_h) with the profile methods of every model class."""

    def __init__(self, h=None):
        self._h = h

    def profile_enable(self, on=True):
        check(load().pgmi_profile_enable(self._h, int(on)))

    def profile_reset(self):
        check(load().pgmi_profile_reset(self._h))

    def profile(self) -> dict:
        lib = load()
        out = {}
        for k, name in enumerate(K_NAMES):
            ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
            check(lib.pgmi_profile_get(self._h, k, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)))
            out[name] = dict(ms=ms.value, launches=n.value, flops=fl.value, bytes=by.value)
        return out


class SideHandle:
    """A model with a handle of its own (EVE, ProteinMPNN, UniRep, S2F, S3F, CARP, ProtSSN, VespaG, ProSST) behind the entries
    pgmi_<PREFIX>_weight_count / _create / _destroy / _profile_model.  _create checks the blob size against the library's count and
    creates the handle; `before_device` are the arguments the create entry takes between the blob and the device (S2F / S3F: the ESM2
    handle).  NAME starts the blob size message."""
    PREFIX = ""
    CREATE = None           # the create entry, where it is not pgmi_<PREFIX>_create
    NAME = ""

    def _create(self, config, blob, device, *before_device):
        lib = load()
        w = as_f32(blob)
        n = getattr(lib, f"pgmi_{self.PREFIX}_weight_count")(C.byref(config))
        if n < 0:
            check(EINVAL)
        if w.size != n:
            raise PgmiError(f"{self.NAME}weight blob has {w.size} elements, config needs {n}")
        h = C.c_void_p()
        create = getattr(lib, self.CREATE or f"pgmi_{self.PREFIX}_create")
        check(create(C.byref(config), ptr(w, _f32p), w.size, *before_device, device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            getattr(load(), f"pgmi_{self.PREFIX}_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def profile_handle(self, *part):
        """The pgmi_model that carries the handle's profile (S3F: of half `part`)."""
        return C.c_void_p(getattr(load(), f"pgmi_{self.PREFIX}_profile_model")(self._h, *part))

    def profile_view(self, *part):
        """profile_handle as an object with EsmModel's profile methods."""
        return _ProfileView(self.profile_handle(*part))
