"""ctypes binding of libagenda_hip.so (C ABI in include/agenda_hip.h).

There is NO fallback: if the HIP library is missing or fails to load, importing the product path
raises.  (The CPU oracle under oracle/ is test infrastructure and is never imported from here.)
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# AGD_LIB: developer override of the library path (tools/ point it at the experiments build, `make -C agenda_amd/csrc exp`);
# whatever the path, a missing or unloadable library raises -- there is no fallback
LIB_PATH = os.environ.get("AGD_LIB") or os.path.join(_HERE, "libagenda_hip.so")
AGD_MAX_LEVELS = 8
AGD_N_CLASSES = 11


class AgdConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int),
        ("in_channels", C.c_int), ("out_channels", C.c_int), ("n_levels", C.c_int),
        ("block_out_channels", C.c_int * AGD_MAX_LEVELS),
        ("down_cross", C.c_int * AGD_MAX_LEVELS),
        ("num_heads", C.c_int * AGD_MAX_LEVELS),
        ("layers_per_block", C.c_int), ("cross_attention_dim", C.c_int),
        ("use_linear_projection", C.c_int), ("norm_num_groups", C.c_int),
        ("vae_latent_channels", C.c_int), ("vae_out_channels", C.c_int), ("vae_n_levels", C.c_int),
        ("vae_block_out_channels", C.c_int * AGD_MAX_LEVELS),
        ("vae_layers_per_block", C.c_int), ("vae_norm_num_groups", C.c_int),
        ("vae_scaling_factor", C.c_float),
        ("max_tokens", C.c_int),
        ("prediction_type", C.c_int),
        ("workspace_bytes", C.c_longlong),
        ("text_hidden", C.c_int), ("text_layers", C.c_int), ("text_heads", C.c_int), ("text_intermediate", C.c_int),
        ("text_vocab", C.c_int), ("text_max_pos", C.c_int), ("text_act", C.c_int), ("text_eps", C.c_float),
    ]


class AgdVisionConfig(C.Structure):
    """`agd_vision_config`: the safety checker's CLIP vision tower (agd_safety_configure)."""
    _fields_ = [
        ("struct_size", C.c_int),
        ("hidden", C.c_int), ("layers", C.c_int), ("heads", C.c_int), ("intermediate", C.c_int),
        ("image_size", C.c_int), ("patch_size", C.c_int), ("projection_dim", C.c_int),
        ("n_special", C.c_int), ("n_concepts", C.c_int), ("act", C.c_int),
        ("eps", C.c_float), ("mean", C.c_float * 3), ("std", C.c_float * 3),
    ]


AGD_CN_MAX_EMB = 8


class AgdControlNetConfig(C.Structure):
    """`agd_controlnet_config`: the ControlNet's conditioning embedding (agd_controlnet_configure)."""
    _fields_ = [
        ("struct_size", C.c_int),
        ("n_emb", C.c_int), ("emb_channels", C.c_int * AGD_CN_MAX_EMB),
        ("bgr", C.c_int),
    ]


class AgdAdapterConfig(C.Structure):
    """`agd_adapter_config`: a T2I-Adapter "full_adapter" (agd_adapter_configure)."""
    _fields_ = [
        ("struct_size", C.c_int),
        ("in_channels", C.c_int), ("n_channels", C.c_int), ("channels", C.c_int * AGD_MAX_LEVELS),
        ("num_res_blocks", C.c_int), ("downscale_factor", C.c_int),
    ]


class AgdGligenConfig(C.Structure):
    """`agd_gligen_config`: the PositionNet of a GLIGEN UNet (agd_gligen_configure)."""
    _fields_ = [
        ("struct_size", C.c_int),
        ("max_objs", C.c_int), ("positive_len", C.c_int), ("fourier_freqs", C.c_int),
    ]


class AgdIgemmDesc(C.Structure):
    """`agd_igemm_desc`: one implicit-GEMM launch stated field by field (agd_op_igemm)."""
    _fields_ = (
        [(n, C.c_int) for n in (
            "struct_size", "images", "H", "W", "C0", "C1", "ksize", "stride", "pad", "up", "hout", "wout", "sc_C0", "sc_C1", "N", "K", "w_per_image",
            "bias_mode", "rowadd_ld", "ldr", "geglu", "act", "out_f32", "ldo", "batch", "rowstat_slots", "ln_slots", "colstat_rows", "gn_groups",
            "gn_silu", "gn_keep_out", "halo", "p8", "smap", "pc", "kg2", "wreg", "xcd_block")]
        + [(n, C.c_float) for n in ("alpha", "ln_invC", "ln_eps", "gn_eps")]
        + [(n, C.c_longlong) for n in ("sA0", "sA1", "sW", "sO", "sR", "n_src0", "n_src1", "n_sc0", "n_sc1", "n_w", "n_res", "n_out")]
        + [(n, C.c_void_p) for n in ("src0", "src1", "sc0", "sc1", "w", "bias", "rowadd", "residual", "ln_stats", "ln_cs", "gn_gamma", "gn_beta",
                                     "out", "gn_y", "rowstat", "colstat")]
        + [("cfg", C.c_int * 3), ("ran", C.c_int * 2), ("gn_fused", C.c_int), ("can_fuse_sc", C.c_int)])


class AgdRegionsDesc(C.Structure):
    """`agd_regions_desc`: what one agd_denoise_regions call reads (masks, noise, backgrounds on the device; idx, sqrt_ac on the host)."""
    _fields_ = [
        ("struct_size", C.c_int), ("regions", C.c_int), ("bootstrapping", C.c_int), ("n_backgrounds", C.c_int),
        ("masks", C.c_void_p), ("noise", C.c_void_p), ("backgrounds", C.c_void_p),
        ("idx", C.POINTER(C.c_int)), ("sqrt_ac", C.POINTER(C.c_float)),
    ]


AGD_MAX_EDIT_CONCEPTS = 8


class AgdSegaDesc(C.Structure):
    """`agd_sega_desc`: the Semantic Guidance schedule of the calls to come (agd_sega_set copies the host arrays)."""
    _fields_ = [
        ("struct_size", C.c_int), ("concepts", C.c_int), ("n_evals", C.c_int), ("mom_scale", C.c_float), ("mom_beta", C.c_float),
        ("coef", C.POINTER(C.c_float)), ("q", C.POINTER(C.c_double)), ("w_mom", C.POINTER(C.c_float)), ("w_add", C.POINTER(C.c_float)),
        ("add_mom", C.POINTER(C.c_float)),
    ]


class AgendaHipError(RuntimeError):
    pass


_P = C.c_void_p
_SIGS = {
    "agd_create": (_P, [C.c_int, C.POINTER(AgdConfig)]),
    "agd_destroy": (None, [_P]),
    "agd_last_error": (C.c_char_p, [_P]),
    "agd_load_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.c_int, C.POINTER(C.c_longlong)]),
    "agd_finalize": (C.c_int, [_P]),
    "agd_set_context": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "agd_text_encode": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "agd_text_set_embedding_row": (C.c_int, [_P, C.c_int, _P]),
    "agd_safety_configure": (C.c_int, [_P, C.POINTER(AgdVisionConfig)]),
    "agd_safety_scores": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P]),
    "agd_controlnet_configure": (C.c_int, [_P, C.POINTER(AgdControlNetConfig)]),
    "agd_controlnet_set_cond": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "agd_controlnet_set_schedule": (C.c_int, [_P, C.POINTER(C.c_float), C.c_int]),
    "agd_controlnet_residuals": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, _P, C.POINTER(C.c_longlong), _P]),
    "agd_inpaint_prepare": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "agd_inpaint_set": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, _P]),
    "agd_inpaint_set_schedule": (C.c_int, [_P, C.POINTER(C.c_float), C.c_int]),
    "agd_inpaint_clear": (C.c_int, [_P]),
    "agd_ip2p_prepare_hw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "agd_ip2p_set_hw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, _P]),
    "agd_ip2p_clear": (C.c_int, [_P]),
    "agd_adapter_configure": (C.c_int, [_P, C.POINTER(AgdAdapterConfig)]),
    "agd_adapter_set_cond_hw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "agd_adapter_features": (C.c_int, [_P, _P]),
    "agd_adapter_set_schedule": (C.c_int, [_P, C.POINTER(C.c_float), C.c_int]),
    "agd_adapter_clear": (C.c_int, [_P]),
    "agd_adapter_add_counts": (C.c_int, [_P, C.POINTER(C.c_longlong)]),
    "agd_ip_adapter_begin": (C.c_int, [_P, C.c_int, C.c_int]),
    "agd_ip_adapter_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.c_int, C.POINTER(C.c_longlong)]),
    "agd_ip_adapter_commit": (C.c_int, [_P]),
    "agd_ip_adapter_unload": (C.c_int, [_P]),
    "agd_ip_adapter_set": (C.c_int, [_P, _P, C.c_int, C.c_float, _P]),
    "agd_ip_adapter_clear": (C.c_int, [_P]),
    "agd_ip_adapter_tokens": (C.c_int, [_P, _P]),
    "agd_ip_adapter_block": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "agd_ip_adapter_counts": (C.c_int, [_P, C.POINTER(C.c_longlong)]),
    "agd_image_encoder_begin": (C.c_int, [_P, C.POINTER(AgdVisionConfig)]),
    "agd_image_encoder_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.c_int, C.POINTER(C.c_longlong)]),
    "agd_image_encoder_commit": (C.c_int, [_P]),
    "agd_image_encoder_unload": (C.c_int, [_P]),
    "agd_image_embeds": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "agd_gligen_configure": (C.c_int, [_P, C.POINTER(AgdGligenConfig)]),
    "agd_gligen_set": (C.c_int, [_P, _P, _P, _P, C.c_int, _P]),
    "agd_gligen_set_schedule": (C.c_int, [_P, C.POINTER(C.c_int), C.c_int]),
    "agd_gligen_clear": (C.c_int, [_P]),
    "agd_gligen_objs": (C.c_int, [_P, _P]),
    "agd_gligen_fuser": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "agd_lora_add": (C.c_int, [_P, C.c_char_p, _P, _P, C.c_int, C.c_float]),
    "agd_lora_set_scale": (C.c_int, [_P, C.c_float, _P]),
    "agd_lora_clear": (C.c_int, [_P]),
    "agd_lora_count": (C.c_int, [_P]),
    "agd_lora_scale": (C.c_float, [_P]),
    "agd_unet_forward": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_float, _P, _P]),
    "agd_unet_forward_ts": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_float), _P, _P]),
    "agd_cfg_ddim_step": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, _P]),
    "agd_denoise": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                              C.POINTER(C.c_float), C.c_float, _P]),
    "agd_denoise_plms": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                   C.POINTER(C.c_float), C.c_float, _P]),
    "agd_denoise_dpm": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, _P]),
    "agd_vae_decode": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P]),
    "agd_vae_encode": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P]),
    "agd_safety_scores_hw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "agd_controlnet_set_cond_hw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "agd_controlnet_residuals_hw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, _P, C.POINTER(C.c_longlong), _P]),
    "agd_inpaint_prepare_hw": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "agd_inpaint_set_hw": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P]),
    "agd_unet_forward_hw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P]),
    "agd_unet_forward_ts_hw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), _P, _P]),
    "agd_cfg_ddim_step_hw": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, _P]),
    "agd_denoise_hw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                 C.POINTER(C.c_float), C.c_float, _P]),
    "agd_denoise_plms_hw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                      C.POINTER(C.c_float), C.c_float, _P]),
    "agd_denoise_dpm_hw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, _P]),
    "agd_vae_decode_hw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "agd_vae_encode_hw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "agd_record_reset_hw": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    "agd_set_option": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "agd_record_config": (C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    "agd_record_reset": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "agd_daam_global": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "agd_hook_global": (C.c_int, [_P, _P, _P]),
    "agd_hook_count": (C.c_int, [_P]),
    "agd_hook_last_map": (C.c_int, [_P, _P, C.c_int, _P]),
    "agd_cross_attn": (C.c_int, [_P, C.c_char_p, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P]),
    "agd_attn_processor": (C.c_int, [_P, C.c_char_p, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P]),
    "agd_hook_reset": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "agd_hook_num_maps": (C.c_int, [_P]),
    "agd_hook_map_dims": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    "agd_hook_map": (C.c_int, [_P, C.c_int, _P, _P]),
    "agd_op_attn_reg_loss": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_float, _P, _P, _P]),
    "agd_attn_processor_backward": (C.c_int, [_P, C.c_char_p, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "agd_op_conv2d": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 9 + [_P]),
    "agd_op_conv2d_ex": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 10 + [_P]),
    "agd_op_linear": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "agd_op_groupnorm": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _P]),
    "agd_op_groupnorm_ex": (C.c_int, [_P] * 5 + [C.c_int] * 5 + [C.c_float, C.c_int, _P, C.c_int, _P, C.c_int, C.POINTER(C.c_int), _P]),
    "agd_op_gn_fold": (C.c_int, [_P, _P] + [C.c_int] * 5 + [C.c_float] + [_P] * 4 + [C.c_int, C.c_int] + [_P] * 5 + [_P]),
    "agd_op_conv_groupnorm": (C.c_int, [_P] * 6 + [C.c_int] * 6 + [C.c_float, C.c_int, C.c_int, _P]),
    "agd_op_igemm": (C.c_int, [C.POINTER(AgdIgemmDesc), _P]),
    "agd_op_layernorm": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_float, _P]),
    "agd_op_layernorm_ex": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_int), _P]),
    "agd_op_ff_fused": (C.c_int, [_P] * 8 + [C.c_int, C.c_int, C.c_float, _P]),
    "agd_op_attn_chain": (C.c_int, [_P] * 9 + [C.c_int] * 5 + [C.c_float, _P]),
    "agd_op_ff_fused_ex": (C.c_int, [_P] * 8 + [C.c_int, C.c_int, C.c_float, _P, _P, _P, C.c_int, _P, C.c_int, _P, C.c_int, _P]),
    "agd_op_attn_chain_ex": (C.c_int, [_P] * 8 + [C.c_int] * 5 + [C.c_float] + [_P] * 4 + [C.c_int, _P, _P] + [C.c_int] * 6 + [_P]),
    "agd_op_qkv_chain": (C.c_int, [_P] * 3 + [C.c_int, C.c_float, _P, C.c_int] + [_P] * 4 + [C.c_float] + [_P] * 3 + [C.c_int] * 4 + [_P]),
    "agd_op_xattn_premul": (C.c_int, [_P] * 9 + [C.c_int] * 5 + [C.c_float, _P]),
    "agd_op_xattn_context": (C.c_int, [_P] * 9 + [C.c_int] * 4 + [_P]),
    "agd_op_xattn_scores": (C.c_int, [_P, _P, C.c_int] + [_P] * 5 + [C.c_int] * 8 + [C.c_float, _P]),
    "agd_op_ipa_linear": (C.c_int, [_P] * 4 + [C.c_int] * 3 + [_P]),
    "agd_op_ipa_layernorm": (C.c_int, [_P] * 4 + [C.c_int, C.c_int, C.c_float, _P]),
    "agd_op_ipa_context": (C.c_int, [_P] * 10 + [C.c_int] * 5 + [_P]),
    "agd_op_ipa_scores": (C.c_int, [_P] * 5 + [C.c_int] * 6 + [C.c_float, C.c_int, _P]),
    "agd_op_ipa_add": (C.c_int, [_P] * 3 + [C.c_int] * 4 + [C.c_float, C.c_int, _P]),
    "agd_op_attention": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P]),
    "agd_op_attention_ex": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 5 + [C.c_float, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P]),
    "agd_op_attention_long": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 5 + [C.c_float, C.c_int, _P, C.c_int, C.c_int, _P]),
    "agd_op_attention_headsum": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P]),
    "agd_op_attention_backward": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 6 + [C.c_float, _P, _P, _P]),
    "agd_op_hook_headmean": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "agd_op_bicubic_clamp_mean": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "agd_op_heatmap_u8": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "agd_op_resize_u8_pil": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "agd_op_stack_heatmaps": (C.c_int, [_P, _P, _P, C.c_longlong, _P, _P, _P]),
    "agd_op_window_gather": (C.c_int, [_P, _P] + [C.c_int] * 8 + [_P]),
    "agd_op_window_mean": (C.c_int, [_P, _P] + [C.c_int] * 6 + [_P]),
    "agd_denoise_panorama": (C.c_int, [_P, _P] + [C.c_int] * 7 + [C.POINTER(C.c_float)] * 3 + [C.c_float, _P]),
    "agd_daam_global_panorama": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "agd_op_region_masks": (C.c_int, [_P, C.c_int, C.c_int, _P] + [C.c_int] * 6 + [_P]),
    "agd_op_region_spread": (C.c_int, [_P] * 5 + [C.c_int] * 6 + [C.POINTER(C.c_int), C.c_float, C.c_float, _P]),
    "agd_op_region_mean": (C.c_int, [_P, _P, _P] + [C.c_int] * 5 + [_P]),
    "agd_denoise_regions": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(AgdRegionsDesc), C.c_int] + [C.POINTER(C.c_float)] * 3 + [C.c_float, _P]),
    "agd_freeu_set": (C.c_int, [_P] + [C.c_float] * 4),
    "agd_freeu_clear": (C.c_int, [_P]),
    "agd_freeu_counts": (C.c_int, [_P, C.POINTER(C.c_longlong)]),
    "agd_op_freeu": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 5 + [C.c_float, C.c_float, _P]),
    "agd_guidance_rescale_set": (C.c_int, [_P, C.c_float]),
    "agd_guidance_rescale_clear": (C.c_int, [_P]),
    "agd_guidance_rescale_counts": (C.c_int, [_P, C.POINTER(C.c_longlong)]),
    "agd_op_guidance_rescale": (C.c_int, [_P, _P] + [C.c_int] * 4 + [C.c_float, C.c_float, _P, _P]),
    "agd_pag_set": (C.c_int, [_P, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_char_p), C.c_int]),
    "agd_pag_clear": (C.c_int, [_P]),
    "agd_pag_counts": (C.c_int, [_P, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "agd_op_pag_v_rows": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P]),
    "agd_op_pag_fold": (C.c_int, [_P, _P, C.c_longlong, C.c_float, _P]),
    "agd_sega_set": (C.c_int, [_P, C.POINTER(AgdSegaDesc)]),
    "agd_sega_clear": (C.c_int, [_P]),
    "agd_sega_counts": (C.c_int, [_P, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "agd_op_sega_threshold": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_double), _P, _P]),
    "agd_op_sega_fold": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                   C.c_float, C.c_float, C.c_float, _P]),
    "agd_deepcache_set": (C.c_int, [_P, C.POINTER(C.c_int), C.c_int, C.c_int]),
    "agd_deepcache_clear": (C.c_int, [_P]),
    "agd_deepcache_counts": (C.c_int, [_P, C.POINTER(C.c_longlong)]),
    "agd_deepcache_forward_hw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, _P, _P]),
    "agd_op_deepcache_capture": (C.c_int, [_P, _P, _P, C.c_longlong, _P, _P, C.c_longlong, _P]),
    "agd_profile_begin": (C.c_int, [_P]),
    "agd_profile_end": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    "agd_profile_end_ex": (C.c_int, [_P, C.c_double, C.c_double] + [C.POINTER(C.c_double)] * 5 + [C.POINTER(C.c_longlong)]),
    "agd_profile_class_name": (C.c_char_p, [C.c_int]),
    "agd_version": (C.c_char_p, []),
}

EXPORTS = tuple(_SIGS.keys())
_lib = None


def load():
    """Load the library once; raise (never fall back) if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AgendaHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C agenda_amd/csrc`. There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, ctx=None, what: str = ""):
    if rc != 0:
        msg = load().agd_last_error(ctx)
        raise AgendaHipError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")


def ptr(t):
    """Raw device/host pointer of a contiguous torch tensor (or None)."""
    if t is None:
        return None
    assert t.is_contiguous(), "tensor must be contiguous"
    return C.c_void_p(t.data_ptr())


def current_stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
