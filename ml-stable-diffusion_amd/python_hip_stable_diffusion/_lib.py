"""ctypes binding of ``libsdmi355.so`` (include/sd_mi355x.h).

The library is the product; this module only marshals numpy arrays across the C ABI and maps
status codes onto the exception classes the reference raises at the same seam
(python_coreml_stable_diffusion/coreml_model.py:97-116, :176-178).  There is no CPU fallback:
a missing library is an ImportError-class failure with build instructions, and a missing GPU
surfaces as RuntimeError from the first call that needs one.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SD_MI355X_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libsdmi355.so"))

SD_MAX_LEVELS = 6
SD_FLAG_DEVICE_PTRS = 1
ATTENTION_IMPLEMENTATIONS = {"ORIGINAL": 0, "SPLIT_EINSUM": 1, "SPLIT_EINSUM_V2": 2}


class LibraryNotBuilt(ImportError):
    pass


class UNetConfig(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("in_channels", C.c_int32), ("out_channels", C.c_int32),
        ("height", C.c_int32), ("width", C.c_int32), ("n_levels", C.c_int32),
        ("block_out_channels", C.c_int32 * SD_MAX_LEVELS),
        ("down_cross_attn", C.c_int32 * SD_MAX_LEVELS),
        ("up_cross_attn", C.c_int32 * SD_MAX_LEVELS),
        ("layers_per_block", C.c_int32),
        ("attention_head_dim", C.c_int32 * SD_MAX_LEVELS),
        ("transformer_layers_per_block", C.c_int32 * SD_MAX_LEVELS),
        ("cross_attention_dim", C.c_int32), ("context_len", C.c_int32),
        ("norm_num_groups", C.c_int32), ("norm_eps", C.c_float),
        ("flip_sin_to_cos", C.c_int32), ("freq_shift", C.c_float),
        ("addition_time_embed_dim", C.c_int32), ("projection_class_embeddings_input_dim", C.c_int32),
        ("num_time_ids", C.c_int32), ("support_controlnet", C.c_int32), ("is_controlnet", C.c_int32),
        ("is_vae_decoder", C.c_int32),
        ("attention_impl", C.c_int32), ("use_graph", C.c_int32), ("compute_fp32", C.c_int32),
    ]


class UNetIO(C.Structure):
    _fields_ = [
        ("sample", C.c_void_p), ("timestep", C.c_void_p), ("encoder_hidden_states", C.c_void_p),
        ("time_ids", C.c_void_p), ("text_embeds", C.c_void_p), ("controlnet_cond", C.c_void_p),
        ("additional_residuals", C.POINTER(C.c_void_p)), ("num_additional_residuals", C.c_int32),
        ("noise_pred", C.c_void_p), ("residual_outputs", C.POINTER(C.c_void_p)), ("flags", C.c_int32),
        ("step_noise", C.c_void_p),
    ]


class SafetyCheckerConfig(C.Structure):
    """sd_safety_checker_config: thirteen 4-byte members, no padding."""
    _fields_ = [("batch", C.c_int32), ("image_size", C.c_int32), ("patch_size", C.c_int32), ("hidden_size", C.c_int32),
                ("intermediate_size", C.c_int32), ("num_hidden_layers", C.c_int32), ("num_attention_heads", C.c_int32),
                ("projection_dim", C.c_int32), ("num_concepts", C.c_int32), ("num_special", C.c_int32), ("hidden_act", C.c_int32),
                ("layer_norm_eps", C.c_float), ("use_graph", C.c_int32)]


class ImagePost(C.Structure):
    """sd_image_post: what CLIPImageProcessor resolves to for one image size (safety_checker.image_post builds it)."""
    _fields_ = [("resize_h", C.c_int32), ("resize_w", C.c_int32), ("image_mean", C.c_float * 3), ("image_std", C.c_float * 3)]


class TextEncoderConfig(C.Structure):
    _fields_ = [("vocab_size", C.c_int32), ("hidden_size", C.c_int32), ("intermediate_size", C.c_int32),
                ("num_hidden_layers", C.c_int32), ("num_attention_heads", C.c_int32),
                ("max_position_embeddings", C.c_int32), ("hidden_act", C.c_int32), ("projection_dim", C.c_int32),
                ("layer_norm_eps", C.c_float), ("use_graph", C.c_int32)]


ACTS = {"quick_gelu": 0, "gelu": 1}      # hidden_act of the two CLIP towers' configs (launch_clip_act)

# sd_progress_fn: int (*)(void* user, int step, int n_steps, const float* latents, const float* denoised)
PROGRESS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float))

_lib = None

# every symbol include/sd_mi355x.h declares: (name, restype, argtypes)
_P, _I, _F = C.c_void_p, C.c_int, C.c_float
_FP = C.POINTER(C.c_float)
SYMBOLS = [
    ("sd_last_error", C.c_char_p, []),
    ("sd_version", C.c_char_p, []),
    ("sd_device_count", _I, []),
    ("sd_weights_create", _I, [C.POINTER(_P)]),
    ("sd_weights_add", _I, [_P, C.c_char_p, _P, _I, C.POINTER(C.c_int64), _I]),
    ("sd_weights_load_safetensors", _I, [_P, C.c_char_p, C.c_char_p]),
    ("sd_weights_count", _I, [_P]),
    ("sd_weights_destroy", None, [_P]),
    ("sd_weights_set_values", _I, [_P, C.c_char_p, _FP, C.c_size_t]),
    ("sd_weights_tensor_info", _I, [_P, _I, C.c_char_p, _I, C.POINTER(C.c_int64), C.POINTER(_I)]),
    ("sd_weights_palettize", _I, [_P, C.c_char_p, _I, C.POINTER(C.c_double)]),
    ("sd_weights_add_palettized", _I, [_P, C.c_char_p, _P, _I, _P, C.POINTER(C.c_int64), _I]),
    ("sd_weights_palette_bits", _I, [_P, C.c_char_p]),
    ("sd_weights_read_palette", _I, [_P, C.c_char_p, _P, _P, _FP]),
    ("sd_weights_quantize_w8a8", _I, [_P, C.c_char_p, _F, C.POINTER(C.c_double)]),
    ("sd_weights_w8a8_info", _I, [_P, C.c_char_p, _FP]),
    ("sd_weights_palette_halo", _I, [_P, _I]),
    ("sd_weights_observe_activations", _I, [_P, _I]),
    ("sd_weights_observe_gemms", _I, [_P, _I]),
    ("sd_weights_observe_geglus", _I, [_P, _I]),
    ("sd_weights_observe_qkv", _I, [_P, _I]),
    ("sd_weights_observe_tails", _I, [_P, _I]),
    ("sd_weights_observe_einsums", _I, [_P, _I]),
    ("sd_weights_quantize_einsum", _I, [_P, C.c_char_p, _F, _F, _F]),
    ("sd_weights_einsum_info", _I, [_P, C.c_char_p, _FP]),
    ("sd_unet_einsum_info", _I, [_P, C.POINTER(_I), C.POINTER(_I)]),
    ("sd_unet_einsum_layer", _I, [_P, _I, C.c_char_p, _I]),
    ("sd_unet_w8a8_info", _I, [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(C.c_size_t)]),
    ("sd_unet_w8a8_layer", _I, [_P, _I, C.c_char_p, _I]),
    ("sd_unet_activation_ranges", _I, [_P, _I, C.c_char_p, _I, _FP]),
    ("sd_op_conv2d_w8a8", _I, [_P, _P, _P, _FP, _F, _FP, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_I), _I, _FP]),
    ("sd_op_w8a8_pack", _I, [_P, _I, _I, _I, _P, C.POINTER(C.c_size_t)]),
    ("sd_op_conv2d_w8a8_halo", _I, [_P, _P, _P, _FP, _F, _FP, _FP, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_I), _I, _FP]),
    ("sd_op_w8a8_pack_halo", _I, [_P, _I, _I, _P, C.POINTER(C.c_size_t)]),
    ("sd_op_subpixel_fold", _I, [_P, _I, _I, _I, _P, C.POINTER(C.c_size_t)]),
    ("sd_op_subpixel_refusal", _I, [_I, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.c_char_p, _I]),
    ("sd_op_conv2d_subpixel", _I, [_P, _P, _FP, _P, _P, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_I), _I, _FP]),
    ("sd_op_gemm_w8a8", _I, [_P, _P, _FP, _F, _FP, _P, _P, _I, _I, _I, _I, _I, _I, C.POINTER(_I), _I, _FP]),
    ("sd_op_w8a8_pack_gemm", _I, [_P, _I, _I, _P, C.POINTER(C.c_size_t)]),
    ("sd_op_layernorm_q8", _I, [_P, _FP, _FP, _F, _F, _P, _I, _I, _I, _FP]),
    ("sd_op_geglu_w8a8", _I, [_P, _P, _FP, _F, _FP, _P, _I, _I, _I, _I, C.POINTER(_I), _I, _FP]),
    ("sd_op_w8a8_pack_geglu", _I, [_P, _I, _I, _P, C.POINTER(C.c_size_t)]),
    ("sd_op_geglu_w8a8_q8", _I, [_P, _P, _FP, _F, _FP, _F, _P, _I, _I, _I, _I, C.POINTER(_I), _I, _FP]),
    ("sd_op_gemm_q8", _I, [_P, _P, _FP, _F, _FP, _P, _P, _I, _I, _I, _I, C.POINTER(_I), _I, _FP]),
    ("sd_op_qkv_w8a8", _I, [_P, _P, _FP, _F, _FP, _P, _P, _I, _I, _I, _F, _I, _I, C.POINTER(_I), _I, _FP]),
    ("sd_op_w8a8_pack_qkv", _I, [_P, _I, _P, C.POINTER(C.c_size_t)]),
    ("sd_op_attention_w8a8", _I, [_P, _P, _P, _F, _F, _F, _P, _I, _I, _I, _I, _FP]),
    ("sd_op_einsum_quantize", _I, [_P, _P, _I, _I, _I, _I, _I, _F, _F, _F, _P, _P, _I, _FP]),
    ("sd_op_w8a8_pack_vt", _I, [_P, _I, _I, _I, _P, C.POINTER(C.c_size_t)]),
    ("sd_op_quantize_weight", _I, [_FP, _I, C.c_size_t, _P, _FP, C.POINTER(C.c_double)]),
    ("sd_op_absmax", _I, [_P, C.c_size_t, _FP]),
    ("sd_unet_create", _I, [C.POINTER(UNetConfig), _P, _I, C.POINTER(_P)]),
    ("sd_unet_destroy", None, [_P]),
    ("sd_unet_set_attention", _I, [_P, _I]),
    ("sd_unet_reload_weights", _I, [_P, _P, C.POINTER(C.c_char_p), _I]),
    ("sd_unet_num_residuals", _I, [_P]),
    ("sd_unet_device_bytes", C.c_size_t, [_P]),
    ("sd_unet_arena_used_bytes", C.c_size_t, [_P]),
    ("sd_unet_palette_info", _I, [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(C.c_size_t)]),
    ("sd_unet_forward", _I, [_P, C.POINTER(UNetIO)]),
    ("sd_unet_time_forward", _I, [_P, _I, _I, _FP]),
    ("sd_unet_denoise_loop", _I, [_P, C.POINTER(UNetIO), _FP, _I, _I, _FP, _FP, _FP, _I, _F, _FP, _FP]),
    # (the handler travels as a plain pointer: C.cast(PROGRESS_FN(f), C.c_void_p), NULL for none)
    ("sd_unet_denoise_loop_progress", _I, [_P, C.POINTER(UNetIO), _FP, _I, _I, _FP, _FP, _FP, _I, _F, _FP, _FP, _FP, _I, _P, _P,
                                           C.POINTER(_I)]),
    ("sd_tune_set_candidate", _I, [_I, _I, _I]),
    ("sd_tune_set_plan_table", _I, [C.c_char_p, C.c_void_p, C.POINTER(C.c_int)]),
    ("sd_unet_profile", _I, [_P, _I, _I, _FP, C.POINTER(C.c_double), C.c_char_p, _I, C.POINTER(_I)]),
    ("sd_unet_attach_controlnets", _I, [_P, C.POINTER(_P), _I]),
    ("sd_controlnet_set_cond", _I, [_P, _P, _I]),
    ("sd_vae_decoder_create", _I, [C.POINTER(UNetConfig), _P, _I, C.POINTER(_P)]),
    ("sd_vae_decode", _I, [_P, _P, _I, _FP, _I]),
    ("sd_vae_encoder_create", _I, [C.POINTER(UNetConfig), _P, _I, C.POINTER(_P)]),
    ("sd_vae_encode", _I, [_P, _P, _I, _FP, _I]),
    ("sd_vae_encode_latents", _I, [_P, _P, _I, _FP, _FP, _I, _F, _F, _F, _FP, _I]),
    ("sd_text_encoder_create", _I, [_P, _P, _I, C.POINTER(_P)]),
    ("sd_text_encoder_destroy", None, [_P]),
    ("sd_text_encoder_device_bytes", C.c_size_t, [_P]),
    ("sd_text_encoder_encode", _I, [_P, C.POINTER(C.c_int32), _I, _FP, _FP, _FP]),
    ("sd_op_attention", _I, [_I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _FP]),
    ("sd_op_attention_kernel", _I, [_I] * 8 + [C.c_char_p, _I]),
    ("sd_op_layernorm", _I, [_P, _FP, _FP, _P, _I, _I, _I, _F, _I, _FP]),
    ("sd_op_groupnorm", _I, [_P, _FP, _FP, _P, _I, _I, _I, _I, _I, _F, _I, _I, _FP]),
    ("sd_op_groupnorm_shortcut", _I, [_P, _P, _FP, _FP, _P, _FP, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _I, _I, _I, _FP]),
    ("sd_op_conv2d", _I, [_P, _P, _FP, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _FP]),
    ("sd_op_conv2d_ex", _I, [_P, _P, _P, _FP, _FP, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _FP, _FP, _F, _I, _P, _I, _I, _I,
                             C.POINTER(_I), _I, _FP]),
    ("sd_op_conv2d_palettized", _I, [_P, _P, _P, _I, _P, _FP, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_I), _I, _FP]),
    ("sd_op_palette_pack", _I, [_P, _I, _I, _I, _I, _P, C.POINTER(C.c_size_t)]),
    ("sd_op_conv2d_palettized_halo", _I, [_P, _P, _P, _I, _P, _FP, _FP, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_I), _I, _FP]),
    ("sd_op_palette_pack_halo", _I, [_P, _I, _I, _I, _P, C.POINTER(C.c_size_t)]),
    ("sd_op_gemm_palettized", _I, [_P, _P, _I, _P, _FP, _P, _P, _I, _I, _I, _I, _I, _I, C.POINTER(_I), _I, _FP]),
    ("sd_op_palette_pack_gemm", _I, [_P, _I, _I, _I, _P, C.POINTER(C.c_size_t)]),
    ("sd_op_geglu_palettized", _I, [_P, _FP, _FP, _P, _I, _P, _FP, _P, _I, _I, _I, C.c_float, _I, C.POINTER(_I), _I, _FP]),
    ("sd_op_palette_pack_geglu", _I, [_P, _I, _I, _I, _P, C.POINTER(C.c_size_t)]),
    ("sd_op_conv2d_groupnorm", _I, [_P, _P, _FP, _P, _FP, _FP, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _I, _I, _I, C.POINTER(_I), _I, _FP]),
    ("sd_op_conv2d_groupnorm_proj", _I, [_P, _P, _FP, _P, _FP, _FP, _P, _FP, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _F, _I, _I, C.POINTER(_I), _I, _FP]),
    ("sd_op_conv2d_groupnorm_conv3x3", _I, [_P, _P, _FP, _P, _FP, _FP, _P, _FP, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _F, _I, _I, _I, _I,
                                            C.POINTER(_I), _I, _FP]),
    ("sd_op_cross_attention_fused", _I, [_P, _FP, _FP, _P, _P, _P, _P, _I, _I, _I, _I, _F, _I, _I, _FP]),
    ("sd_op_ffn_out_proj", _I, [_P, _P, _FP, _P, _P, _FP, _P, _P, _FP, _I, _I, _I, _I, _I, _I, _FP]),
    ("sd_op_fold_linear", _I, [_P, _FP, _P, _FP, _P, _FP, _I, _I, _I]),
    ("sd_op_cross_attention_block", _I, [_P, _FP, _FP, _P, _P, _P, _P, _FP, _P, _P, _FP, _P, _I, _I, _I, _I, _F, _I, _I, _FP]),
    ("sd_op_geglu", _I, [_P, _P, _FP, _P, _I, _I, _I, _I, _FP]),
    ("sd_op_geglu_ln", _I, [_P, _FP, _FP, _P, _FP, _P, _I, _I, _I, C.c_float, _I, _I, _FP]),
    ("sd_op_qkv_ln", _I, [_P, _FP, _FP, _P, _P, _P, _I, _I, _I, C.c_float, C.c_float, _I, _I, _I, _FP]),
    ("sd_op_gn_proj_qkv", _I, [_P, _P, _FP, _FP, _P, _FP, _FP, _FP, _P, _P, _P, _P, _I, _I, _I, _I, _I, C.c_float, C.c_float, C.c_float, _I, _I,
                               C.POINTER(C.c_int), _I, _FP]),
    ("sd_op_timestep_embedding", _I, [_FP, _FP, _I, _I, _I, _F]),
    ("sd_op_posterior_noise", _I, [_FP, _FP, _FP, _FP, _I, _I, _I, _I, _F, _F, _F, _I, _FP]),
    ("sd_op_sched_step", _I, [_FP, _FP, _FP, _FP, _FP, _FP, _F, _I, _I, _I, _I, _FP, C.POINTER(_I)]),
    ("sd_op_conv_plan", _I, [_I] * 18 + [C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]),
    ("sd_op_conv_plan_kernel", _I, [_I] * 18 + [C.c_char_p, _I]),
    ("sd_numpy_randn", _I, [C.c_uint32, C.POINTER(C.c_double), C.c_size_t]),
    ("sd_torch_randn", _I, [C.c_uint32, C.POINTER(C.c_double), C.c_size_t]),
    ("sd_philox_randn", _I, [C.c_uint64, C.c_uint32, C.POINTER(C.c_double), C.c_size_t]),
    ("sd_calibrate", _I, [_I, _FP]),
    ("sd_selftest_mfma", _I, []),
    ("sd_safety_checker_create", _I, [C.POINTER(SafetyCheckerConfig), _P, _I, C.POINTER(_P)]),
    ("sd_safety_checker_destroy", None, [_P]),
    ("sd_safety_checker_device_bytes", C.c_size_t, [_P]),
    ("sd_safety_checker_last_ms", C.c_float, [_P]),
    ("sd_safety_checker_run", _I, [_P, _P, _F, _FP, _FP, _FP, _FP, _I]),
    ("sd_op_vit_attention", _I, [_P, _P, _I, _I, _I, _I, _I, _FP]),
    ("sd_op_safety_head", _I, [_FP, _FP, _FP, _FP, _FP, _F, _I, _I, _I, _I, _FP, _FP]),
    ("sd_op_vae_attention", _I, [_P, _P, _P, _P, _I, _I, _I, _I, _FP]),
    ("sd_vae_decode_images", _I, [_P, _P, _I, _FP, _P, _P, C.POINTER(ImagePost), _F, _FP, _FP, _I]),
    ("sd_op_resample_coeffs", _I, [_I, _I, C.POINTER(_I), _P, _P]),
    ("sd_op_image_rgb8", _I, [_FP, _P, _I, _I, _I, _I, _FP]),
    ("sd_op_clip_input", _I, [_P, _P, _I, _I, _I, _I, _I, _I, _FP, _FP, _I, _FP]),
    ("sd_op_conv_f32", _I, [_FP, _P, _I, _FP, _FP, _FP, _I, _I, _I, _I, _I, _I, _I, _I, _I]),
    ("sd_op_groupnorm_f32", _I, [_FP, _FP, _FP, _FP, _I, _I, _I, _I, _I, _F, _I]),
    ("sd_op_row_softmax", _I, [_P, _I, _I, _F, _I]),
    ("sd_op_gemv", _I, [_P, _FP, _FP, _FP, _I, _I, _I, _I, _I, _I]),
    ("sd_op_clip_attention", _I, [_P, _P, _I, _I, _I]),
    ("sd_op_clip_embed", _I, [C.POINTER(C.c_int32), _P, _P, _P, _I, _I, _I]),
    ("sd_op_clip_act", _I, [_P, C.c_size_t, _I]),
    ("sd_op_layout", _I, [_I, _P, _P, _I, _I, _I, _I]),
    ("sd_op_sum_half", _I, [C.POINTER(_P), _I, _P, C.c_size_t, _I]),
    ("sd_op_vit_patch_rows", _I, [_P, _P, _I, _I, _I, _I]),
    ("sd_op_vit_tokens", _I, [_P, _P, _P, _P, _I, _I, _I]),
    ("sd_op_harness_selftest", _I, [_I, _P, _FP, C.c_size_t]),
]


def lib():
    """Load the shared library (once).  torch is imported first when available so that both bind
    the same HIP runtime (torch ships its own libamdhip64 with the same soname)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LibraryNotBuilt(
            f"{LIB_PATH} is missing - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C ml-stable-diffusion_amd/csrc`. There is no CPU fallback.")
    if not os.environ.get("SD_MI355X_NO_TORCH"):
        try:
            import torch  # noqa: F401  (plumbing only: shares libamdhip64 / RCCL with torch.distributed)
        except Exception:  # pragma: no cover - torch is optional for the library itself
            pass
    handle = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(handle, name)   # AttributeError here == header/library mismatch
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = handle
    return handle


_EXC = {-1: ValueError, -2: FileNotFoundError, -3: RuntimeError, -4: NotImplementedError, -5: RuntimeError}


def check(status):
    if status != 0:
        msg = lib().sd_last_error().decode("utf-8", "replace")
        raise _EXC.get(status, RuntimeError)(msg)


class Handle:
    """Owner of one library handle ``_h``, freed by the entry point ``_destroy`` names."""
    _destroy = None

    def close(self):
        if getattr(self, "_h", None):
            getattr(lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def verify_inputs(expected, **kwargs):
    """coreml_model.py:97-116: TypeError for a wrong type / dtype / shape, ValueError for an unknown or missing keyword."""
    for k, v in kwargs.items():
        if k not in expected:
            raise ValueError(f"Received unexpected input kwarg: {k}")
        if not isinstance(v, np.ndarray):
            raise TypeError(f"Expected numpy.ndarray, got {v} for input: {k}")
        if v.dtype != expected[k]["dtype"]:
            raise TypeError(f"Expected dtype {expected[k]['dtype']}, got {v.dtype} for input: {k}")
        if v.shape != expected[k]["shape"]:
            raise TypeError(f"Expected shape {expected[k]['shape']}, got {v.shape} for input: {k}")
    missing = [k for k in expected if k not in kwargs]
    if missing:
        raise ValueError(f"Missing input kwargs: {missing}")


class Model(Handle):
    """A model runner behind the CoreMLModel interface: ``expected_inputs`` is what ``__call__`` accepts."""

    def _verify_inputs(self, **kwargs):
        verify_inputs(self.expected_inputs, **kwargs)


def checkpoint_file(folder):
    """The .safetensors file of one model folder of a diffusers checkpoint, the fp16 variant first."""
    if not os.path.isdir(folder):
        raise FileNotFoundError(f"{folder} not found (coreml_model.py:176-178)")
    for name in ("model.fp16.safetensors", "model.safetensors"):
        if os.path.exists(os.path.join(folder, name)):
            return os.path.join(folder, name)
    raise FileNotFoundError(f"no .safetensors checkpoint under {folder}")


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def fptr(a):
    return None if a is None else a.ctypes.data_as(_FP)


def f16(a):
    return np.ascontiguousarray(a, dtype=np.float16)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ------------------------------------------------------------------------------------------------
# operator-level wrappers (tests / micro-benchmarks); all take & return the reference layouts
# ------------------------------------------------------------------------------------------------
def attention(impl, q, k, v, heads, dim_head, variant=0, iters=1):
    """attention.py:24-168.  q (B,h*d,1,Sq), k/v (B,h*d,1,Sk) -> (B,h*d,1,Sq) fp16, ms.  variant: sd_mi355x.h (0 default dispatch, 1 never the
    d = 64 pipelined kernel, 2 pre-scaled q, 100 + u that kernel's balanced grid with u units per workgroup)."""
    if impl not in ATTENTION_IMPLEMENTATIONS:
        raise ValueError(f"unknown attention implementation {impl!r}")
    q, k, v = f16(q), f16(k), f16(v)
    B, Cq, _, Sq = q.shape
    Sk = k.shape[3]
    if Cq != heads * dim_head or k.shape[1] != Cq or v.shape != k.shape:
        raise ValueError("attention: inconsistent q/k/v shapes")
    out = np.empty_like(q)
    ms = C.c_float(0)
    check(lib().sd_op_attention(ATTENTION_IMPLEMENTATIONS[impl], ptr(q), ptr(k), ptr(v), ptr(out), B, heads,
                                dim_head, Sq, Sk, variant, iters, C.byref(ms)))
    return out, ms.value


def attention_kernel(impl, batch, heads, dim_head, Sq, Sk=None, variant=0, int8=False):
    """The kernel ``attention`` (or, with ``int8``, ``attention_w8a8``: dim_head 64, S = Sq; impl and variant are not read) would launch
    for this problem on the current device, as the line sd_op_attention_kernel writes (sd_mi355x.h lists the forms): e.g.
    'attn8 w8 classic', 'attn8 w8 balanced upw=3 seg=2', 'attn_i8 w8', 'attn d64 split w8 qt2'.  Host only; refuses as those entries do."""
    if not int8 and impl not in ATTENTION_IMPLEMENTATIONS:
        raise ValueError(f"unknown attention implementation {impl!r}")
    text = C.create_string_buffer(96)
    check(lib().sd_op_attention_kernel(int(bool(int8)), 0 if int8 else ATTENTION_IMPLEMENTATIONS[impl], batch, heads, dim_head, Sq,
                                       Sq if Sk is None else Sk, variant, text, len(text)))
    return text.value.decode()


def vit_attention(qkv, heads, dim_head=64, out=None, iters=1):
    """Non-causal attention of the safety checker's vision tower (csrc/vit.hip).  qkv (B, S, 3 * heads * dim_head) f16, rows
    [q | k | v] as the stacked projection writes them -> (B, S, heads * dim_head) f16, ms.  ``out``: a C-contiguous float16 buffer of
    at least B * S * heads * dim_head elements to write into (tests put a guard behind it)."""
    qkv = f16(qkv)
    if qkv.ndim != 3 or qkv.shape[2] != 3 * heads * dim_head:
        raise ValueError("vit_attention: qkv must be (B, S, 3 * heads * dim_head)")
    B, S, _ = qkv.shape
    n = B * S * heads * dim_head
    if out is None:
        out = np.empty(n, np.float16)
    if out.dtype != np.float16 or not out.flags.c_contiguous or out.size < n:
        raise ValueError("vit_attention: out must be a C-contiguous float16 buffer of at least B * S * heads * dim_head elements")
    ms = C.c_float(0)
    check(lib().sd_op_vit_attention(ptr(qkv), ptr(out), B, S, heads, dim_head, iters, C.byref(ms)))
    return out.reshape(-1)[:n].reshape(B, S, heads * dim_head), ms.value


def vae_attention(q, k, v, out=None, iters=1):
    """Single-head mid-block attention of the VAE (csrc/vae_attention.hip): softmax(q k^T / sqrt(C)) v as one streaming launch.
    q, k, v (B, S, C) f16 token-major, C in {64, 128, 256, 512} (else NotImplementedError from the library) -> (B, S, C) f16, ms.
    ``out``: a C-contiguous float16 buffer of at least B * S * C elements to write into (tests put a guard behind it)."""
    q, k, v = f16(q), f16(k), f16(v)
    if q.ndim != 3 or k.shape != q.shape or v.shape != q.shape:
        raise ValueError("vae_attention: q, k and v must share one (B, S, C) shape")
    B, S, Cn = q.shape
    n = B * S * Cn
    if out is None:
        out = np.empty(n, np.float16)
    if out.dtype != np.float16 or not out.flags.c_contiguous or out.size < n:
        raise ValueError("vae_attention: out must be a C-contiguous float16 buffer of at least B * S * C elements")
    ms = C.c_float(0)
    check(lib().sd_op_vae_attention(ptr(q), ptr(k), ptr(v), ptr(out), B, S, Cn, iters, C.byref(ms)))
    return out.reshape(-1)[:n].reshape(B, S, Cn), ms.value


def safety_head(image_embeds, concept_embeds, special_embeds, concept_w, special_w, adjustment=0.0):
    """The safety checker's concept head (torch2coreml.py:1177-1209) in fp32 on the GPU.  Returns (has_nsfw (B,) bool,
    concept_scores (B, n_concepts) f32)."""
    image_embeds, concept_embeds, special_embeds = f32(image_embeds), f32(concept_embeds), f32(special_embeds)
    concept_w, special_w = f32(concept_w), f32(special_w)
    B, P = image_embeds.shape
    nc, ns = concept_embeds.shape[0], special_embeds.shape[0]
    if concept_embeds.shape != (nc, P) or special_embeds.shape != (ns, P) or concept_w.shape != (nc,) or special_w.shape != (ns,):
        raise ValueError("safety_head: inconsistent shapes")
    flags = np.empty(B, np.float32)
    scores = np.empty((B, nc), np.float32)
    check(lib().sd_op_safety_head(fptr(image_embeds), fptr(concept_embeds), fptr(special_embeds), fptr(concept_w), fptr(special_w),
                                  float(adjustment), B, P, nc, ns, fptr(flags), fptr(scores)))
    return flags > 0.5, scores


def resample_coeffs(in_size, out_size):
    """Pillow's 8-bit bicubic coefficient tables of one axis (sd_op_resample_coeffs; host only): (ksize, bounds (out_size, 2) int32 =
    [xmin, n], coeffs (out_size, ksize) int32 with 22 fraction bits, zeros behind the n taps of a row)."""
    ksize = C.c_int(0)
    check(lib().sd_op_resample_coeffs(int(in_size), int(out_size), C.byref(ksize), None, None))
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, ksize.value), np.int32)
    check(lib().sd_op_resample_coeffs(int(in_size), int(out_size), C.byref(ksize), ptr(bounds), ptr(coeffs)))
    return ksize.value, bounds, coeffs


def image_rgb8(image, iters=1):
    """numpy_to_pil's quantisation on the GPU (csrc/imgpost.hip image_rgb8_kernel): image (B, 3, H, W) f32 in [-1, 1] ->
    ((np.clip(image / 2 + 0.5, 0, 1) * 255).round().astype("uint8") as (B, H, W, 3), ms)."""
    image = f32(image)
    if image.ndim != 4 or image.shape[1] != 3:
        raise ValueError("image_rgb8: image must be (B, 3, H, W)")
    B, _, H, W = image.shape
    out = np.empty((B, H, W, 3), np.uint8)
    ms = C.c_float(0)
    check(lib().sd_op_image_rgb8(fptr(image), ptr(out), B, H, W, iters, C.byref(ms)))
    return out, ms.value


def clip_input(rgb8, rh, rw, S, mean, std, out=None, iters=1):
    """CLIPImageProcessor on the GPU (csrc/imgpost.hip clip_input_kernel): rgb8 (B, H, W, 3) uint8 -> Pillow's 8-bit bicubic resize to
    (rh, rw), centre crop to S x S, (u / 255 - mean) / std in fp32, as (clip_input (B, 3, S, S) f16, ms).  ``out``: a C-contiguous
    float16 buffer of at least B * 3 * S * S elements to write into (tests put a guard behind it).  A geometry the kernel does not
    express is refused by the library before any device work (ValueError / NotImplementedError)."""
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    mean, std = f32(mean), f32(std)
    if rgb8.ndim != 4 or rgb8.shape[3] != 3 or mean.shape != (3,) or std.shape != (3,):
        raise ValueError("clip_input: rgb8 must be (B, H, W, 3), mean and std three floats each")
    B, H, W, _ = rgb8.shape
    n = B * 3 * S * S
    if out is None:
        out = np.empty(n, np.float16)
    if out.dtype != np.float16 or not out.flags.c_contiguous or out.size < n:
        raise ValueError("clip_input: out must be a C-contiguous float16 buffer of at least B * 3 * S * S elements")
    ms = C.c_float(0)
    check(lib().sd_op_clip_input(ptr(rgb8), ptr(out), B, H, W, int(rh), int(rw), int(S), fptr(mean), fptr(std), iters, C.byref(ms)))
    return out.reshape(-1)[:n].reshape(B, 3, S, S), ms.value


def layernorm(x, weight, bias, eps=1e-5, iters=1):
    x, weight, bias = f16(x), f32(weight), f32(bias)
    B, Cn, _, S = x.shape
    out = np.empty_like(x)
    ms = C.c_float(0)
    check(lib().sd_op_layernorm(ptr(x), fptr(weight), fptr(bias), ptr(out), B, Cn, S, eps, iters, C.byref(ms)))
    return out, ms.value


def groupnorm(x, weight, bias, groups=32, eps=1e-5, silu=False, iters=1):
    x, weight, bias = f16(x), f32(weight), f32(bias)
    B, Cn, H, W = x.shape
    out = np.empty_like(x)
    ms = C.c_float(0)
    check(lib().sd_op_groupnorm(ptr(x), fptr(weight), fptr(bias), ptr(out), B, Cn, H, W, groups, eps, int(silu),
                                iters, C.byref(ms)))
    return out, ms.value


def conv2d(x, w, bias=None, res=None, stride=1, upsample=False, tile=0, splitk=0, force_generic=False, iters=1):
    x, w = f16(x), f16(w)
    B, Cin, H, W = x.shape
    Cout, Cin2, k, k2 = w.shape
    if Cin2 != Cin or k != k2:
        raise ValueError("conv2d: weight shape does not match input")
    up = 2 if upsample else 1
    pad = k // 2
    Ho = (H * up + 2 * pad - k) // stride + 1
    Wo = (W * up + 2 * pad - k) // stride + 1
    bias = None if bias is None else f32(bias)
    res = None if res is None else f16(res)
    if res is not None and res.shape != (B, Cout, Ho, Wo):   # the library reads B * Cout * Ho * Wo halves behind the pointer
        raise ValueError(f"conv2d: res must be (B, Cout, Ho, Wo) = {(B, Cout, Ho, Wo)}, got {res.shape}")
    out = np.empty((B, Cout, Ho, Wo), np.float16)
    ms = C.c_float(0)
    check(lib().sd_op_conv2d(ptr(x), ptr(w), fptr(bias), ptr(res), ptr(out), B, Cin, H, W, Cout, k, stride,
                             int(upsample), tile, splitk, int(force_generic), iters, C.byref(ms)))
    return out, ms.value


def subpixel_fold(w):
    """The host fold of an upsampler's 3x3 weights into the four 2x2 phase matrices of plan tile 21 (sd_op_subpixel_fold; no GPU):
    w (Cout, Cin, 3, 3) float16 or float32 -> (4, Cout, 4, Cin) float16, phase p = 2a + b, tap t = 2dy + dx at low-res offset
    (a + dy - 1, b + dx - 1); fp32 sums in (ky, kx) order, one rounding."""
    w = np.ascontiguousarray(w)
    if w.dtype not in (np.float16, np.float32) or w.ndim != 4 or w.shape[2:] != (3, 3):
        raise ValueError("subpixel_fold: w must be (Cout, Cin, 3, 3) float16 or float32")
    Cout, Cin = w.shape[:2]
    out = np.empty((4, Cout, 4, Cin), np.float16)
    n = C.c_size_t(0)
    check(lib().sd_op_subpixel_fold(ptr(w), int(w.dtype == np.float32), Cout, Cin, ptr(out), C.byref(n)))
    assert n.value == out.size
    return out


def subpixel_refusal(C0, N, B, Hi, Wi, ksize=3, stride=1, up=2, C1=0, out_mode=0):
    """Why plan tile 21 refuses a conv of this shape, "" when it takes it (sd_op_subpixel_refusal; no GPU)."""
    text = C.create_string_buffer(128)
    check(lib().sd_op_subpixel_refusal(ksize, stride, up, C0, C1, N, B, Hi, Wi, out_mode, text, len(text)))
    return text.value.decode()


def conv2d_subpixel(x, w, bias=None, res=None, splitk=0, staging=0, iters=1):
    """Nearest-x2 upsample + 3x3 / pad-1 conv as four 2x2 phase convs on the low-res image (sd_op_conv2d_subpixel, plan tile 21):
    x (B, Cin, H, W), w (Cout, Cin, 3, 3) -> (out (B, Cout, 2H, 2W) float16, plan [tile, staging, splitk, slab], ms).  staging: plan
    tile 7's ring code (2 = three stages, else four); splitk 0 = the plan's rule."""
    x, w = f16(x), f16(w)
    B, Cin, H, W = x.shape
    if w.ndim != 4 or w.shape[1:] != (Cin, 3, 3):
        raise ValueError("conv2d_subpixel: w must be (Cout, Cin, 3, 3)")
    Cout = w.shape[0]
    bias = None if bias is None else f32(bias)
    res = None if res is None else f16(res)
    if bias is not None and bias.shape != (Cout,):
        raise ValueError("conv2d_subpixel: bias must be (Cout,)")
    if res is not None and res.shape != (B, Cout, 2 * H, 2 * W):
        raise ValueError(f"conv2d_subpixel: res must be (B, Cout, 2H, 2W) = {(B, Cout, 2 * H, 2 * W)}, got {res.shape}")
    out = np.empty((B, Cout, 2 * H, 2 * W), np.float16)
    plan = (C.c_int * 4)()
    ms = C.c_float(0)
    check(lib().sd_op_conv2d_subpixel(ptr(x), ptr(w), fptr(bias), ptr(res), ptr(out), B, Cin, H, W, Cout, splitk, staging, plan, iters,
                                      C.byref(ms)))
    return out, list(plan), ms.value


def conv2d_ex(x, w, bias=None, res=None, x1=None, temb=None, stride=1, upsample=False, pad_mode=0, twin=None, tile=0, splitk=0,
              force_generic=False, iters=1):
    """conv2d with a second source x1 (channel concat), a time-embedding row temb (B, Cout), the VAE encoder's (0,1,0,1) padding
    (pad_mode=1) and one GroupNorm twin of the output: twin = (groups, gamma, beta, eps, silu).  Returns (out, twin output or None,
    plan, ms); plan = [tile, staging, splitk, slab] of the launch, all -1 for the direct kernels."""
    x, w = f16(x), f16(w)
    x1 = None if x1 is None else f16(x1)
    B, Cin, H, W = x.shape
    C1 = 0 if x1 is None else x1.shape[1]
    Cout, Ctot, k, k2 = w.shape
    if Ctot != Cin + C1 or k != k2 or (x1 is not None and x1.shape != (B, C1, H, W)):
        raise ValueError("conv2d_ex: weight / second source shape does not match input")
    up = 2 if upsample else 1
    pad = k // 2
    Ho = (H * up + (1 if pad_mode else 2 * pad) - k) // stride + 1
    Wo = (W * up + (1 if pad_mode else 2 * pad) - k) // stride + 1
    bias = None if bias is None else f32(bias)
    res = None if res is None else f16(res)
    temb = None if temb is None else f32(temb)
    if (temb is not None and temb.shape != (B, Cout)) or (res is not None and res.shape != (B, Cout, Ho, Wo)):
        raise ValueError("conv2d_ex: temb must be (B, Cout), res (B, Cout, Ho, Wo)")
    groups, gamma, beta, eps, silu = (0, None, None, 0.0, False) if twin is None else twin
    gamma = None if gamma is None else f32(gamma)
    beta = None if beta is None else f32(beta)
    out = np.empty((B, Cout, Ho, Wo), np.float16)
    out_twin = None if twin is None else np.empty_like(out)
    plan = (C.c_int * 4)()
    ms = C.c_float(0)
    check(lib().sd_op_conv2d_ex(ptr(x), ptr(x1), ptr(w), fptr(bias), fptr(temb), ptr(res), ptr(out), B, Cin, C1, H, W, Cout, k, stride,
                                int(upsample), pad_mode, groups, fptr(gamma), fptr(beta), eps, int(silu), ptr(out_twin), tile, splitk,
                                int(force_generic), plan, iters, C.byref(ms)))
    return out, out_twin, list(plan), ms.value


def conv2d_palettized(x, lut, indices, nbits, bias=None, res=None, x1=None, upsample=False, nw=0, out=None, iters=1):
    """The weight-stream conv from palettized weights (sd_op_conv2d_palettized, plan tile 14): w = lut[indices], lut (2^nbits,) f16,
    indices (Cout, Cin + C1, k, k) uint8.  ``out``: a C-contiguous float16 buffer of at least B * Cout * Ho * Wo elements to write
    into (tests put guards behind it).  Returns (out (B, Cout, Ho, Wo), plan, ms)."""
    x, lut = f16(x), f16(lut)
    indices = np.ascontiguousarray(indices, dtype=np.uint8)
    x1 = None if x1 is None else f16(x1)
    B, Cin, H, W = x.shape
    C1 = 0 if x1 is None else x1.shape[1]
    if indices.ndim != 4:
        raise ValueError("conv2d_palettized: indices must be (Cout, Cin + C1, k, k)")
    Cout, Ctot, k, k2 = indices.shape
    if Ctot != Cin + C1 or k != k2 or (x1 is not None and x1.shape != (B, C1, H, W)):
        raise ValueError("conv2d_palettized: indices / second source shape does not match input")
    if nbits not in (1, 2, 4, 6, 8) or lut.shape != (1 << nbits,):
        raise ValueError("conv2d_palettized: nbits must be 1, 2, 4, 6 or 8 and lut hold 2 ** nbits entries")
    up = 2 if upsample else 1
    Ho, Wo = H * up, W * up
    bias = None if bias is None else f32(bias)
    res = None if res is None else f16(res)
    if res is not None and res.shape != (B, Cout, Ho, Wo):
        raise ValueError("conv2d_palettized: res must be (B, Cout, Ho, Wo)")
    n = B * Cout * Ho * Wo
    if out is None:
        out = np.empty(n, np.float16)
    if out.dtype != np.float16 or not out.flags.c_contiguous or out.size < n:
        raise ValueError("conv2d_palettized: out must be a C-contiguous float16 buffer of at least B * Cout * Ho * Wo elements")
    plan = (C.c_int * 4)()
    ms = C.c_float(0)
    check(lib().sd_op_conv2d_palettized(ptr(x), ptr(x1), ptr(lut), nbits, ptr(indices), fptr(bias), ptr(res), ptr(out), B, Cin, C1, H, W,
                                        Cout, k, int(upsample), nw, plan, iters, C.byref(ms)))
    return out.reshape(-1)[:n].reshape(B, Cout, Ho, Wo), list(plan), ms.value


def conv2d_palettized_halo(x, lut, indices, nbits, bias=None, temb=None, res=None, x1=None, upsample=False, staging=3, splitk=0, out=None,
                           iters=1):
    """The 3x3 / stride-1 halo conv from palettized weights (sd_op_conv2d_palettized_halo, plan tile 25): w = lut[indices], lut
    (2^nbits,) f16, indices (Cout, Cin + C1, 3, 3) uint8; temb (B, Cout) f32; staging = plan tile 7's ring code (0 / 2 / 3 / 4 / 5 =
    2 / 3 / 4 / 6 / 8 stages), splitk 0 = the library's rule.  Bit-identical to conv2d_ex(tile=7) on lut[indices] at the same staging
    and splitk.  What the library checks - nbits, the ranges, the shape, an index outside the palette - it refuses itself (ValueError, no
    GPU needed).  Returns (out (B, Cout, Ho, Wo), plan, ms)."""
    x, lut = f16(x), f16(lut)
    indices = np.ascontiguousarray(indices, dtype=np.uint8)
    x1 = None if x1 is None else f16(x1)
    B, Cin, H, W = x.shape
    C1 = 0 if x1 is None else x1.shape[1]
    if indices.ndim != 4 or indices.shape[2:] != (3, 3):
        raise ValueError("conv2d_palettized_halo: indices must be (Cout, Cin + C1, 3, 3)")
    Cout, Ctot = indices.shape[:2]
    if Ctot != Cin + C1 or (x1 is not None and x1.shape != (B, C1, H, W)):
        raise ValueError("conv2d_palettized_halo: indices / second source shape does not match input")
    if nbits in (1, 2, 4, 6, 8) and lut.shape != (1 << nbits,):
        raise ValueError("conv2d_palettized_halo: lut must hold 2 ** nbits entries")
    up = 2 if upsample else 1
    Ho, Wo = H * up, W * up
    bias = None if bias is None else f32(bias)
    temb = None if temb is None else f32(temb)
    res = None if res is None else f16(res)
    if res is not None and res.shape != (B, Cout, Ho, Wo):
        raise ValueError("conv2d_palettized_halo: res must be (B, Cout, Ho, Wo)")
    if temb is not None and temb.shape != (B, Cout):
        raise ValueError("conv2d_palettized_halo: temb must be (B, Cout)")
    n = B * Cout * Ho * Wo
    if out is None:
        out = np.empty(n, np.float16)
    if out.dtype != np.float16 or not out.flags.c_contiguous or out.size < n:
        raise ValueError("conv2d_palettized_halo: out must be a C-contiguous float16 buffer of at least B * Cout * Ho * Wo elements")
    plan = (C.c_int * 4)()
    ms = C.c_float(0)
    check(lib().sd_op_conv2d_palettized_halo(ptr(x), ptr(x1), ptr(lut), int(nbits), ptr(indices), fptr(bias), fptr(temb), ptr(res), ptr(out),
                                             B, Cin, C1, H, W, Cout, int(upsample), staging, splitk, plan, iters, C.byref(ms)))
    return out.reshape(-1)[:n].reshape(B, Cout, Ho, Wo), list(plan), ms.value


def palette_pack_halo(indices, nbits):
    """The index bit stream of the palettized halo conv (sd_op_palette_pack_halo; host only): indices (Cout, Ctot, 3, 3) uint8 -> uint8
    array (n_tiles, chunks, 9, nbits, 2, 64, 4): per (64-row n-tile, 64-channel chunk, tap) dword j of stream (wk, lane) as four
    little-endian bytes."""
    indices = np.ascontiguousarray(indices, dtype=np.uint8)
    if indices.ndim != 4 or indices.shape[2:] != (3, 3):
        raise ValueError("palette_pack_halo: indices must be (Cout, Ctot, 3, 3)")
    Cout, Ctot = indices.shape[:2]
    return _packed(lib().sd_op_palette_pack_halo, ptr(indices), Cout, Ctot, nbits).reshape(-(-Cout // 64), Ctot // 64, 9, nbits, 2, 64, 4)


def conv2d_w8a8(x, wq, w_scale, act_absmax, bias=None, res=None, x1=None, upsample=False, nw=0, out=None, iters=1):
    """The weight-stream conv in W8A8 (sd_op_conv2d_w8a8, plan tile 17): wq (Cout, Cin + C1, k, k) int8, w_scale (Cout,) f32,
    act_absmax the range of x (and x1); the rest as conv2d_palettized.  Returns (out (B, Cout, Ho, Wo), plan, ms)."""
    x = f16(x)
    wq = np.ascontiguousarray(wq, dtype=np.int8)
    w_scale = f32(w_scale)
    x1 = None if x1 is None else f16(x1)
    B, Cin, H, W = x.shape
    C1 = 0 if x1 is None else x1.shape[1]
    if wq.ndim != 4:
        raise ValueError("conv2d_w8a8: wq must be (Cout, Cin + C1, k, k)")
    Cout, Ctot, k, k2 = wq.shape
    if Ctot != Cin + C1 or k != k2 or (x1 is not None and x1.shape != (B, C1, H, W)) or w_scale.shape != (Cout,):
        raise ValueError("conv2d_w8a8: wq / w_scale / second source shape does not match input")
    up = 2 if upsample else 1
    Ho, Wo = H * up, W * up
    bias = None if bias is None else f32(bias)
    res = None if res is None else f16(res)
    if res is not None and res.shape != (B, Cout, Ho, Wo):
        raise ValueError("conv2d_w8a8: res must be (B, Cout, Ho, Wo)")
    n = B * Cout * Ho * Wo
    if out is None:
        out = np.empty(n, np.float16)
    if out.dtype != np.float16 or not out.flags.c_contiguous or out.size < n:
        raise ValueError("conv2d_w8a8: out must be a C-contiguous float16 buffer of at least B * Cout * Ho * Wo elements")
    plan = (C.c_int * 4)()
    ms = C.c_float(0)
    check(lib().sd_op_conv2d_w8a8(ptr(x), ptr(x1), ptr(wq), fptr(w_scale), float(act_absmax), fptr(bias), ptr(res), ptr(out), B, Cin, C1,
                                  H, W, Cout, k, int(upsample), nw, plan, iters, C.byref(ms)))
    return out.reshape(-1)[:n].reshape(B, Cout, Ho, Wo), list(plan), ms.value


def conv2d_w8a8_halo(x, wq, w_scale, act_absmax, bias=None, temb=None, res=None, x1=None, upsample=False, staging=3, splitk=0, out=None,
                     iters=1):
    """The 3x3 / stride-1 halo conv in W8A8 (sd_op_conv2d_w8a8_halo, plan tile 18): wq (Cout, Cin + C1, 3, 3) int8, w_scale (Cout,) f32,
    act_absmax the range of x (and x1); temb (B, Cout) f32; staging = plan tile 7's ring code (0 / 2 / 3 = 2 / 3 / 4 stages), splitk 0 =
    the library's rule.  Returns (out (B, Cout, Ho, Wo), plan, ms)."""
    x = f16(x)
    wq = np.ascontiguousarray(wq, dtype=np.int8)
    w_scale = f32(w_scale)
    x1 = None if x1 is None else f16(x1)
    B, Cin, H, W = x.shape
    C1 = 0 if x1 is None else x1.shape[1]
    if wq.ndim != 4 or wq.shape[2:] != (3, 3):
        raise ValueError("conv2d_w8a8_halo: wq must be (Cout, Cin + C1, 3, 3)")
    Cout, Ctot = wq.shape[:2]
    if Ctot != Cin + C1 or (x1 is not None and x1.shape != (B, C1, H, W)) or w_scale.shape != (Cout,):
        raise ValueError("conv2d_w8a8_halo: wq / w_scale / second source shape does not match input")
    up = 2 if upsample else 1
    Ho, Wo = H * up, W * up
    bias = None if bias is None else f32(bias)
    temb = None if temb is None else f32(temb)
    res = None if res is None else f16(res)
    if res is not None and res.shape != (B, Cout, Ho, Wo):
        raise ValueError("conv2d_w8a8_halo: res must be (B, Cout, Ho, Wo)")
    if temb is not None and temb.shape != (B, Cout):
        raise ValueError("conv2d_w8a8_halo: temb must be (B, Cout)")
    n = B * Cout * Ho * Wo
    if out is None:
        out = np.empty(n, np.float16)
    if out.dtype != np.float16 or not out.flags.c_contiguous or out.size < n:
        raise ValueError("conv2d_w8a8_halo: out must be a C-contiguous float16 buffer of at least B * Cout * Ho * Wo elements")
    plan = (C.c_int * 4)()
    ms = C.c_float(0)
    check(lib().sd_op_conv2d_w8a8_halo(ptr(x), ptr(x1), ptr(wq), fptr(w_scale), float(act_absmax), fptr(bias), fptr(temb), ptr(res), ptr(out),
                                       B, Cin, C1, H, W, Cout, int(upsample), staging, splitk, plan, iters, C.byref(ms)))
    return out.reshape(-1)[:n].reshape(B, Cout, Ho, Wo), list(plan), ms.value


def w8a8_pack_halo(wq):
    """The int8 weights of the W8A8 halo conv (sd_op_w8a8_pack_halo; host only): wq (Cout, Ctot, 3, 3) int8 -> int8 (Cout, 9, Ctot)."""
    wq = np.ascontiguousarray(wq, dtype=np.int8)
    if wq.ndim != 4 or wq.shape[2:] != (3, 3):
        raise ValueError("w8a8_pack_halo: wq must be (Cout, Ctot, 3, 3)")
    Cout, Ctot = wq.shape[:2]
    return _packed(lib().sd_op_w8a8_pack_halo, ptr(wq), Cout, Ctot).view(np.int8).reshape(Cout, 9, Ctot)


def gemm_w8a8(x, wq, w_scale, act_absmax, bias=None, res=None, bm=0, out=None, iters=1):
    """The single-source small-M 1x1 GEMM in W8A8 (sd_op_gemm_w8a8, plan tile 19): x (B, Cin, H, W), wq (Cout, Cin) int8, w_scale
    (Cout,) f32, act_absmax the range of x; bm 0 / 32 / 64 = the tile height (0: by M).  ``out``: a C-contiguous float16 buffer of at
    least B * Cout * H * W elements to write into (tests put guards behind it).  What the library checks - bm, shape, the int32 bound,
    act_absmax, w_scale, a weight of -128 - it refuses itself (ValueError, no GPU needed).  Returns (out (B, Cout, H, W), plan, ms)."""
    x = f16(x)
    wq = np.ascontiguousarray(wq, dtype=np.int8)
    w_scale = f32(w_scale)
    if x.ndim != 4 or wq.ndim != 2 or wq.shape[1] != x.shape[1] or w_scale.shape != (wq.shape[0],):
        raise ValueError("gemm_w8a8: x must be (B, Cin, H, W), wq (Cout, Cin) and w_scale (Cout,)")
    B, Cin, H, W = x.shape
    Cout = wq.shape[0]
    bias = None if bias is None else f32(bias)
    res = None if res is None else f16(res)
    if (bias is not None and bias.shape != (Cout,)) or (res is not None and res.shape != (B, Cout, H, W)):
        raise ValueError("gemm_w8a8: bias must be (Cout,), res (B, Cout, H, W)")
    n = B * Cout * H * W
    if out is None:
        out = np.empty(n, np.float16)
    if out.dtype != np.float16 or not out.flags.c_contiguous or out.size < n:
        raise ValueError("gemm_w8a8: out must be a C-contiguous float16 buffer of at least B * Cout * H * W elements")
    plan = (C.c_int * 4)()
    ms = C.c_float(0)
    check(lib().sd_op_gemm_w8a8(ptr(x), ptr(wq), fptr(w_scale), float(act_absmax), fptr(bias), ptr(res), ptr(out), B, Cin, H, W, Cout, bm, plan,
                                iters, C.byref(ms)))
    return out.reshape(-1)[:n].reshape(B, Cout, H, W), list(plan), ms.value


def w8a8_pack_gemm(wq):
    """The int8 weights of the W8A8 small-M GEMM (sd_op_w8a8_pack_gemm; host only): wq (Cout, K) int8 -> int8 (Cout, K), the
    checkpoint's own order."""
    wq = np.ascontiguousarray(wq, dtype=np.int8)
    if wq.ndim != 2:
        raise ValueError("w8a8_pack_gemm: wq must be (Cout, K)")
    Cout, K = wq.shape
    return _packed(lib().sd_op_w8a8_pack_gemm, ptr(wq), Cout, K).view(np.int8).reshape(Cout, K)


def layernorm_q8(x, ln_weight, ln_bias, act_absmax, eps=1e-5, out=None, iters=1):
    """LayerNorm that leaves as int8 (sd_op_layernorm_q8): x (M, C) float16 token-major, ln_weight / ln_bias (C,) f32 or both None (a
    plain quantize of x), act_absmax the range the output is quantized with.  ``out``: a C-contiguous int8 buffer of at least M * C
    elements to write into (tests put guards behind it).  Returns (xq (M, C) int8, ms)."""
    x = f16(x)
    if x.ndim != 2 or (ln_weight is None) != (ln_bias is None):
        raise ValueError("layernorm_q8: x must be (M, C); ln_weight and ln_bias go together")
    M, Cc = x.shape
    ln_weight = None if ln_weight is None else f32(ln_weight)
    ln_bias = None if ln_bias is None else f32(ln_bias)
    if ln_weight is not None and (ln_weight.shape != (Cc,) or ln_bias.shape != (Cc,)):
        raise ValueError("layernorm_q8: ln_weight and ln_bias must be (C,)")
    if out is None:
        out = np.empty(M * Cc, np.int8)
    if out.dtype != np.int8 or not out.flags.c_contiguous or out.size < M * Cc:
        raise ValueError("layernorm_q8: out must be a C-contiguous int8 buffer of at least M * C elements")
    ms = C.c_float(0)
    check(lib().sd_op_layernorm_q8(ptr(x), fptr(ln_weight), fptr(ln_bias), float(act_absmax), float(eps), ptr(out), M, Cc, iters, C.byref(ms)))
    return out.reshape(-1)[:M * Cc].reshape(M, Cc), ms.value


def geglu_w8a8(xq, wq, w_scale, act_absmax, bias=None, bm=0, out=None, iters=1, out_absmax=None):
    """The GEGLU projection in W8A8 (sd_op_geglu_w8a8, plan tile 20): xq (M, C) int8, wq (N2, C) int8 in the checkpoint's row order
    [values | gates], w_scale (N2,) f32, act_absmax the range xq was quantized with, bias (N2,) f32 or None; bm 0 / 128 / 256 = the tile
    height (0: by the grid).  ``out``: a C-contiguous float16 buffer of at least M * N2 / 2 elements (tests put guards behind it).  What
    the library checks it refuses itself (ValueError, no GPU needed).  Returns (out (M, N2 / 2), plan, ms).
    With ``out_absmax`` (sd_op_geglu_w8a8_q8) the product leaves as int8, quantized with that range: ``out`` is then an int8 buffer and
    the first result (M, N2 / 2) int8 - the activations of ``gemm_q8``."""
    xq = np.ascontiguousarray(xq, dtype=np.int8)
    wq = np.ascontiguousarray(wq, dtype=np.int8)
    w_scale = f32(w_scale)
    if xq.ndim != 2 or wq.ndim != 2 or wq.shape[1] != xq.shape[1] or w_scale.shape != (wq.shape[0],):
        raise ValueError("geglu_w8a8: xq must be (M, C), wq (N2, C) and w_scale (N2,)")
    M, Cc = xq.shape
    N2 = wq.shape[0]
    bias = None if bias is None else f32(bias)
    if bias is not None and bias.shape != (N2,):
        raise ValueError("geglu_w8a8: bias must be (N2,)")
    n = M * (N2 // 2)
    dtype = np.float16 if out_absmax is None else np.int8
    if out is None:
        out = np.empty(n, dtype)
    if out.dtype != dtype or not out.flags.c_contiguous or out.size < n:
        raise ValueError("geglu_w8a8: out must be a C-contiguous float16 (with out_absmax: int8) buffer of at least M * N2 / 2 elements")
    plan = (C.c_int * 4)()
    ms = C.c_float(0)
    if out_absmax is None:
        check(lib().sd_op_geglu_w8a8(ptr(xq), ptr(wq), fptr(w_scale), float(act_absmax), fptr(bias), ptr(out), M, Cc, N2, bm, plan, iters, C.byref(ms)))
    else:
        check(lib().sd_op_geglu_w8a8_q8(ptr(xq), ptr(wq), fptr(w_scale), float(act_absmax), fptr(bias), float(out_absmax), ptr(out), M, Cc, N2, bm,
                                        plan, iters, C.byref(ms)))
    return out.reshape(-1)[:n].reshape(M, N2 // 2), list(plan), ms.value


def gemm_q8(xq, wq, w_scale, act_absmax, bias=None, res=None, bm=0, out=None, iters=1):
    """The small-M 1x1 GEMM from int8 weights and int8 activations (sd_op_gemm_q8, plan tile 24), token-major: xq (M, K) int8, wq (N, K)
    int8, w_scale (N,) f32, act_absmax the range xq was quantized with, bias (N,) f32 / res (M, N) float16 or None; bm 0 / 32 / 64 = the
    tile height (0: by M).  ``out``: a C-contiguous float16 buffer of at least M * N elements (tests put guards behind it).  What the
    library checks - bm, shape, the int32 bound, act_absmax, w_scale, a weight or an activation of -128 - it refuses itself (ValueError,
    no GPU needed).  Returns (out (M, N), plan, ms)."""
    xq = np.ascontiguousarray(xq, dtype=np.int8)
    wq = np.ascontiguousarray(wq, dtype=np.int8)
    w_scale = f32(w_scale)
    if xq.ndim != 2 or wq.ndim != 2 or wq.shape[1] != xq.shape[1] or w_scale.shape != (wq.shape[0],):
        raise ValueError("gemm_q8: xq must be (M, K), wq (N, K) and w_scale (N,)")
    M, K = xq.shape
    N = wq.shape[0]
    bias = None if bias is None else f32(bias)
    res = None if res is None else f16(res)
    if (bias is not None and bias.shape != (N,)) or (res is not None and res.shape != (M, N)):
        raise ValueError("gemm_q8: bias must be (N,), res (M, N)")
    n = M * N
    if out is None:
        out = np.empty(n, np.float16)
    if out.dtype != np.float16 or not out.flags.c_contiguous or out.size < n:
        raise ValueError("gemm_q8: out must be a C-contiguous float16 buffer of at least M * N elements")
    plan = (C.c_int * 4)()
    ms = C.c_float(0)
    check(lib().sd_op_gemm_q8(ptr(xq), ptr(wq), fptr(w_scale), float(act_absmax), fptr(bias), ptr(res), ptr(out), M, K, N, bm, plan, iters,
                              C.byref(ms)))
    return out.reshape(-1)[:n].reshape(M, N), list(plan), ms.value


def w8a8_pack_geglu(wq):
    """The int8 weights of the W8A8 GEGLU projection (sd_op_w8a8_pack_geglu; host only): wq (N2, K) int8 [values | gates] -> int8
    (N2 / 16, 16, K), strip 2 U + v = rows v * N2 / 2 + 16 U .. + 15."""
    wq = np.ascontiguousarray(wq, dtype=np.int8)
    if wq.ndim != 2:
        raise ValueError("w8a8_pack_geglu: wq must be (N2, K)")
    N2, K = wq.shape
    return _packed(lib().sd_op_w8a8_pack_geglu, ptr(wq), N2, K).view(np.int8).reshape(N2 // 16, 16, K)


def qkv_w8a8(xq, wq, w_scale, act_absmax, batch, q_scale=1.0, vt_perm=True, bias=None, bm=0, out_qk=None, out_vt=None, iters=1):
    """The fused q|k|v projection of a self-attention in W8A8 (sd_op_qkv_w8a8, plan tile 22; the int8 form of ``qkv_ln`` behind
    ``layernorm_q8``: unet.py:583-586 -> :74-84 under quantize_cumulative_config): xq (batch * HW, C) int8, wq (3C, C) int8 =
    [Wq | Wk | Wv], w_scale (3C,) f32, act_absmax the range xq was quantized with, bias (3C,) f32 or None; q_scale multiplies the
    queries before the rounding (1: skipped), vt_perm = V^T in the d = 64 attention kernel's key order, bm 0 / 128 / 256 = the tile
    height (0: by the grid).  ``out_qk`` / ``out_vt``: C-contiguous float16 buffers of at least batch * HW * 2C / batch * C * HW
    elements (tests put guards behind them).  What the library checks it refuses itself (ValueError, no GPU needed).
    Returns (out_qk (batch * HW, 2C), out_vt (batch, C, HW), plan, ms)."""
    xq = np.ascontiguousarray(xq, dtype=np.int8)
    wq = np.ascontiguousarray(wq, dtype=np.int8)
    w_scale = f32(w_scale)
    if xq.ndim != 2 or wq.ndim != 2 or wq.shape != (3 * xq.shape[1], xq.shape[1]) or w_scale.shape != (wq.shape[0],) or batch < 1 or xq.shape[0] % batch:
        raise ValueError("qkv_w8a8: xq must be (batch * HW, C), wq (3C, C) and w_scale (3C,)")
    M, Cc = xq.shape
    HW = M // batch
    bias = None if bias is None else f32(bias)
    if bias is not None and bias.shape != (3 * Cc,):
        raise ValueError("qkv_w8a8: bias must be (3C,)")
    n_qk, n_vt = M * 2 * Cc, batch * Cc * HW
    if out_qk is None:
        out_qk = np.empty(n_qk, np.float16)
    if out_vt is None:
        out_vt = np.empty(n_vt, np.float16)
    for buf, n in ((out_qk, n_qk), (out_vt, n_vt)):
        if buf.dtype != np.float16 or not buf.flags.c_contiguous or buf.size < n:
            raise ValueError("qkv_w8a8: out_qk / out_vt must be C-contiguous float16 buffers of at least M * 2C / batch * C * HW elements")
    plan = (C.c_int * 4)()
    ms = C.c_float(0)
    check(lib().sd_op_qkv_w8a8(ptr(xq), ptr(wq), fptr(w_scale), float(act_absmax), fptr(bias), ptr(out_qk), ptr(out_vt), batch, HW, Cc,
                               float(q_scale), int(bool(vt_perm)), bm, plan, iters, C.byref(ms)))
    return out_qk.reshape(-1)[:n_qk].reshape(M, 2 * Cc), out_vt.reshape(-1)[:n_vt].reshape(batch, Cc, HW), list(plan), ms.value


def w8a8_pack_qkv(wq):
    """The int8 weights of the W8A8 q|k|v projection (sd_op_w8a8_pack_qkv; host only): wq (3C, C) int8 = [Wq | Wk | Wv] -> int8
    (3C / 16, 16, C), strip t = the stacked rows 16 t .. 16 t + 15."""
    wq = np.ascontiguousarray(wq, dtype=np.int8)
    if wq.ndim != 2 or wq.shape[0] != 3 * wq.shape[1]:
        raise ValueError("w8a8_pack_qkv: wq must be (3C, C)")
    Cc = wq.shape[1]
    return _packed(lib().sd_op_w8a8_pack_qkv, ptr(wq), Cc).view(np.int8).reshape(3 * Cc // 16, 16, Cc)


def attention_w8a8(q_q, k_q, v_q, q_absmax, k_absmax, v_absmax, batch, heads, S=None, out=None, iters=1):
    """The self-attention einsums in W8A8 (sd_op_attention_w8a8; the function is stated in sd_mi355x.h): q_q, k_q, v_q (batch * S,
    heads * 64) int8 token-major in natural key order, the three ranges of the un-scaled q, k and v.  ``S``: the sequence length
    (default: rows / batch).  ``out``: a C-contiguous float16 buffer of at least batch * S * heads * 64 elements (tests put guards
    behind it).  What the library checks - shape, S, the ranges, a value of -128 - it refuses itself (ValueError, no GPU needed).
    Returns (out (batch * S, heads * 64) float16, ms)."""
    q_q, k_q, v_q = (np.ascontiguousarray(a, dtype=np.int8) for a in (q_q, k_q, v_q))
    if q_q.ndim != 2 or k_q.shape != q_q.shape or v_q.shape != q_q.shape or batch < 1 or heads < 1:
        raise ValueError("attention_w8a8: q_q, k_q and v_q must be (batch * S, heads * 64) int8")
    if S is None:
        if q_q.shape[0] % batch:
            raise ValueError("attention_w8a8: q_q, k_q and v_q must be (batch * S, heads * 64) int8")
        S = q_q.shape[0] // batch
    n = batch * S * heads * 64
    # an S the library refuses before it reads a value (off the rule, past the integer bound) may come with arrays of any size
    refused_unread = S < 64 or S % 64 != 0 or S > 133120
    if n != q_q.size and not refused_unread:
        raise ValueError("attention_w8a8: q_q, k_q and v_q must be (batch * S, heads * 64) int8")
    if out is None:
        out = np.empty(0 if refused_unread else n, np.float16)
    if out.dtype != np.float16 or not out.flags.c_contiguous or (out.size < n and not refused_unread):
        raise ValueError("attention_w8a8: out must be a C-contiguous float16 buffer of at least batch * S * heads * 64 elements")
    ms = C.c_float(0)
    check(lib().sd_op_attention_w8a8(ptr(q_q), ptr(k_q), ptr(v_q), float(q_absmax), float(k_absmax), float(v_absmax), ptr(out), batch, heads, S,
                                     iters, C.byref(ms)))
    return out.reshape(-1)[:n].reshape(batch * S, heads * 64), ms.value


def einsum_quantize(qk, vt, q_range_eff, k_absmax, v_absmax, vt_perm_in=0, iters=1):
    """The quantizer launch in front of the int8 attention (sd_op_einsum_quantize): qk (batch * S, 2C) float16 = q | k rows, vt (batch, C,
    ldv) float16 V^T in the key order ``vt_perm_in`` (0 natural, 1 the fp16 d = 64 kernel's); q_range_eff the range of the stored queries.
    Returns (qk_q (batch * S, 2C) int8, vt_q (batch, C, S) int8 in the int8 kernel's key order, ms)."""
    qk, vt = f16(qk), f16(vt)
    if qk.ndim != 2 or vt.ndim != 3 or qk.shape[1] != 2 * vt.shape[1] or qk.shape[0] % vt.shape[0]:
        raise ValueError("einsum_quantize: qk must be (batch * S, 2C), vt (batch, C, ldv)")
    B, Cc, ldv = vt.shape
    S = qk.shape[0] // B
    qk_q = np.empty((B * S, 2 * Cc), np.int8)
    vt_q = np.empty((B, Cc, S), np.int8)
    ms = C.c_float(0)
    check(lib().sd_op_einsum_quantize(ptr(qk), ptr(vt), B, S, Cc, ldv, int(vt_perm_in), float(q_range_eff), float(k_absmax), float(v_absmax),
                                      ptr(qk_q), ptr(vt_q), iters, C.byref(ms)))
    return qk_q, vt_q, ms.value


def w8a8_pack_vt(v, batch):
    """The int8 V^T of the W8A8 attention (sd_op_w8a8_pack_vt; host only): v (batch * S, C) int8 token-major -> (batch, C, S) int8,
    position p of every 32 keys holding key (p & 3) + 8 * ((p >> 2) & 3) + 4 * (p >> 4) of them."""
    v = np.ascontiguousarray(v, dtype=np.int8)
    if v.ndim != 2 or batch < 1 or v.shape[0] % batch:
        raise ValueError("w8a8_pack_vt: v must be (batch * S, C)")
    S, Cc = v.shape[0] // batch, v.shape[1]
    return _packed(lib().sd_op_w8a8_pack_vt, ptr(v), batch, Cc, S).view(np.int8).reshape(batch, Cc, S)


def w8a8_pack(wq):
    """The int8 stream of the W8A8 weight-stream conv (sd_op_w8a8_pack; host only): wq (Cout, Ctot, k, k) int8 -> int8 array
    [Cout / 32][Ctot / 32][k * k][64 lanes][16 bytes]."""
    wq = np.ascontiguousarray(wq, dtype=np.int8)
    Cout, Ctot, k, k2 = wq.shape
    if k != k2:
        raise ValueError("w8a8_pack: wq must be (Cout, Ctot, k, k)")
    return _packed(lib().sd_op_w8a8_pack, ptr(wq), Cout, Ctot, k).view(np.int8).reshape(Cout // 32, Ctot // 32, k * k, 64, 16)


def quantize_weight(w):
    """The host weight quantizer of W8A8 (sd_op_quantize_weight): w (Cout, ...) f32 -> (q int8 of w's shape, w_scale (Cout,) f32,
    squared error)."""
    w = f32(w)
    if w.ndim < 2 or w.size == 0:
        raise ValueError("quantize_weight: w must be (Cout, ...)")
    q = np.empty(w.shape, np.int8)
    scale = np.empty(w.shape[0], np.float32)
    err = C.c_double(0)
    check(lib().sd_op_quantize_weight(fptr(w), w.shape[0], w.size // w.shape[0], ptr(q), fptr(scale), C.byref(err)))
    return q, scale, err.value


def absmax(x):
    """max |x| of an f16 array on the device (sd_op_absmax: the activation observers' kernel), as an fp32 number."""
    x = f16(x)
    r = C.c_float(0)
    check(lib().sd_op_absmax(ptr(x), x.size, C.byref(r)))
    return np.float32(r.value)


def _packed(pack, *args):
    """The byte stream of a host-only packer: one call for its size (stream = NULL), one to fill it."""
    n = C.c_size_t(0)
    check(pack(*args, None, C.byref(n)))
    stream = np.zeros(n.value, np.uint8)
    check(pack(*args, ptr(stream), C.byref(n)))
    return stream


def palette_pack(indices, nbits):
    """The index bit stream of the palettized weight-stream conv (sd_op_palette_pack; host only): indices (Cout, Ctot, k, k) uint8
    -> uint8 array [Cout / 32][Ctot / 32][words][64 lanes][16 bytes]."""
    indices = np.ascontiguousarray(indices, dtype=np.uint8)
    Cout, Ctot, k, k2 = indices.shape
    if k != k2:
        raise ValueError("palette_pack: indices must be (Cout, Ctot, k, k)")
    return _packed(lib().sd_op_palette_pack, ptr(indices), Cout, Ctot, k, nbits).reshape(Cout // 32, Ctot // 32, -1, 64, 16)


def gemm_palettized(x, lut, indices, nbits, bias=None, res=None, bm=0, out=None, iters=1):
    """The small-M 1x1 GEMM from palettized weights (sd_op_gemm_palettized, plan tile 15): w = lut[indices], lut (2^nbits,) f16, indices
    (Cout, Cin) uint8, x (B, Cin, H, W); bm 0 / 32 / 64 = the tile height (0: by M).  ``out``: a C-contiguous float16 buffer of at
    least B * Cout * H * W elements to write into (tests put guards behind it).  What the library checks - nbits, bm, index range, shape
    - it refuses itself (ValueError, no GPU needed).  Returns (out (B, Cout, H, W), plan, ms)."""
    x, lut = f16(x), f16(lut)
    indices = np.ascontiguousarray(indices, dtype=np.uint8)
    if x.ndim != 4 or indices.ndim != 2 or indices.shape[1] != x.shape[1]:
        raise ValueError("gemm_palettized: x must be (B, Cin, H, W) and indices (Cout, Cin)")
    B, Cin, H, W = x.shape
    Cout = indices.shape[0]
    if nbits in (1, 2, 4, 6, 8) and lut.shape != (1 << nbits,):
        raise ValueError("gemm_palettized: lut must hold 2 ** nbits entries")
    bias = None if bias is None else f32(bias)
    res = None if res is None else f16(res)
    if (bias is not None and bias.shape != (Cout,)) or (res is not None and res.shape != (B, Cout, H, W)):
        raise ValueError("gemm_palettized: bias must be (Cout,), res (B, Cout, H, W)")
    n = B * Cout * H * W
    if out is None:
        out = np.empty(n, np.float16)
    if out.dtype != np.float16 or not out.flags.c_contiguous or out.size < n:
        raise ValueError("gemm_palettized: out must be a C-contiguous float16 buffer of at least B * Cout * H * W elements")
    plan = (C.c_int * 4)()
    ms = C.c_float(0)
    check(lib().sd_op_gemm_palettized(ptr(x), ptr(lut), nbits, ptr(indices), fptr(bias), ptr(res), ptr(out), B, Cin, H, W, Cout, bm, plan,
                                      iters, C.byref(ms)))
    return out.reshape(-1)[:n].reshape(B, Cout, H, W), list(plan), ms.value


def palette_pack_gemm(indices, nbits):
    """The index bit stream of the palettized small-M GEMM (sd_op_palette_pack_gemm; host only): indices (Cout, K) uint8 -> uint8 array
    [Cout / 16][ceil(K / 512) groups][nbits words][64 lanes][16 bytes]."""
    indices = np.ascontiguousarray(indices, dtype=np.uint8)
    if indices.ndim != 2:
        raise ValueError("palette_pack_gemm: indices must be (Cout, K)")
    Cout, K = indices.shape
    return _packed(lib().sd_op_palette_pack_gemm, ptr(indices), Cout, K, nbits).reshape(Cout // 16, -1, nbits, 64, 16)


def geglu_palettized(x, lut, indices, nbits, bias=None, ln_weight=None, ln_bias=None, eps=1e-5, bm=0, out=None, iters=1):
    """The GEGLU projection of smgeglu.hip from palettized weights (sd_op_geglu_palettized, plan tile 16): w = lut[indices], lut
    (2^nbits,) f16, indices (N2, C) uint8 in the checkpoint's row order [values | gates], x (M, C); ln_weight / ln_bias (C,) or both
    None (plain GEGLU); bm 0 / 128 / 256 = the tile height (0: by the grid; only 128-row tiles are built).  ``out``: a C-contiguous
    float16 buffer of at least M * N2 / 2 elements to write into (tests put guards behind it).  What the library checks - nbits, bm,
    the LayerNorm pair, index range, shape - it refuses itself (ValueError, no GPU needed).  Returns (out (M, N2 / 2), plan, ms)."""
    x, lut = f16(x), f16(lut)
    indices = np.ascontiguousarray(indices, dtype=np.uint8)
    if x.ndim != 2 or indices.ndim != 2 or indices.shape[1] != x.shape[1]:
        raise ValueError("geglu_palettized: x must be (M, C) and indices (N2, C)")
    M, Cn = x.shape
    N2 = indices.shape[0]
    if nbits in (1, 2, 4, 6, 8) and lut.shape != (1 << nbits,):
        raise ValueError("geglu_palettized: lut must hold 2 ** nbits entries")
    bias = None if bias is None else f32(bias)
    ln_weight = None if ln_weight is None else f32(ln_weight)
    ln_bias = None if ln_bias is None else f32(ln_bias)
    if (bias is not None and bias.shape != (N2,)) or any(v is not None and v.shape != (Cn,) for v in (ln_weight, ln_bias)):
        raise ValueError("geglu_palettized: bias must be (N2,), ln_weight / ln_bias (C,)")
    n = M * (N2 // 2)
    if out is None:
        out = np.empty(n, np.float16)
    if out.dtype != np.float16 or not out.flags.c_contiguous or out.size < n:
        raise ValueError("geglu_palettized: out must be a C-contiguous float16 buffer of at least M * N2 / 2 elements")
    plan = (C.c_int * 4)()
    ms = C.c_float(0)
    check(lib().sd_op_geglu_palettized(ptr(x), fptr(ln_weight), fptr(ln_bias), ptr(lut), nbits, ptr(indices), fptr(bias), ptr(out), M, Cn,
                                       N2, eps, bm, plan, iters, C.byref(ms)))
    return out.reshape(-1)[:n].reshape(M, N2 // 2), list(plan), ms.value


def palette_pack_geglu(indices, nbits):
    """The index bit stream of the palettized GEGLU projection (sd_op_palette_pack_geglu; host only): indices (N2, K) uint8 in the
    checkpoint's row order -> uint8 array [N2 / 16 strips][ceil(K / 512) groups][nbits words][64 lanes][16 bytes]."""
    indices = np.ascontiguousarray(indices, dtype=np.uint8)
    if indices.ndim != 2:
        raise ValueError("palette_pack_geglu: indices must be (N2, K)")
    N2, K = indices.shape
    return _packed(lib().sd_op_palette_pack_geglu, ptr(indices), N2, K, nbits).reshape(N2 // 16, -1, nbits, 64, 16)


def groupnorm_shortcut(x0, x1, gn_weight, gn_bias, w, bias=None, groups=32, eps=1e-5, silu=True, side=True, iters=1):
    """norm1 (+SiLU) over the concat (x0 | x1) and conv_shortcut (1x1) over the same concat; side=True: one launch.
    Returns (normalised tensor, shortcut output, ms)."""
    x0, w = f16(x0), f16(w)
    x1 = None if x1 is None else f16(x1)
    B, C0, H, W = x0.shape
    C1 = 0 if x1 is None else x1.shape[1]
    N = w.shape[0]
    w = np.ascontiguousarray(w.reshape(N, -1))
    if w.shape[1] != C0 + C1 or (x1 is not None and x1.shape != (B, C1, H, W)):
        raise ValueError("groupnorm_shortcut: inconsistent shapes")
    gn_weight, gn_bias = f32(gn_weight), f32(gn_bias)
    bias = None if bias is None else f32(bias)
    out_gn = np.empty((B, C0 + C1, H, W), np.float16)
    out_sc = np.empty((B, N, H, W), np.float16)
    ms = C.c_float(0)
    check(lib().sd_op_groupnorm_shortcut(ptr(x0), ptr(x1), fptr(gn_weight), fptr(gn_bias), ptr(w), fptr(bias), ptr(out_gn), ptr(out_sc),
                                         B, C0, C1, H, W, N, groups, eps, int(silu), int(side), iters, C.byref(ms)))
    return out_gn, out_sc, ms.value


def conv2d_groupnorm(x, w, gn_weight, gn_bias, bias=None, res=None, groups=32, eps=1e-5, silu=False, tile=0,
                     producer_stats=True, iters=1):
    """conv (stride 1) -> GroupNorm (+ SiLU); producer_stats: GroupNorm statistics from the conv kernel's epilogue.
    Returns (conv output, normalised output, entries the conv wrote per (sample, group), ms)."""
    x, w = f16(x), f16(w)
    B, Cin, H, W = x.shape
    Cout, Cin2, k, k2 = w.shape
    if Cin2 != Cin or k != k2:
        raise ValueError("conv2d_groupnorm: weight shape does not match input")
    bias = None if bias is None else f32(bias)
    res = None if res is None else f16(res)
    gn_weight, gn_bias = f32(gn_weight), f32(gn_bias)
    conv_out = np.empty((B, Cout, H, W), np.float16)
    out = np.empty((B, Cout, H, W), np.float16)
    ms, entries = C.c_float(0), C.c_int(0)
    check(lib().sd_op_conv2d_groupnorm(ptr(x), ptr(w), fptr(bias), ptr(res), fptr(gn_weight), fptr(gn_bias), ptr(conv_out),
                                       ptr(out), B, Cin, H, W, Cout, k, groups, eps, int(silu), tile, int(producer_stats),
                                       C.byref(entries), iters, C.byref(ms)))
    return conv_out, out, entries.value, ms.value


def conv2d_groupnorm_proj(x, w, gn_weight, gn_bias, proj_w, proj_bias=None, bias=None, res=None, groups=32, eps=1e-6, fold=True,
                          tile=0, iters=1):
    """proj(GroupNorm(conv(x))) - a resnet's last conv followed by SpatialTransformer.norm + proj_in; fold=True applies the
    GroupNorm inside the projection GEMM.  Returns (conv_out, out, entries consumed by the fold, ms)."""
    x, w, proj_w = f16(x), f16(w), f16(proj_w)
    B, Cin, H, W = x.shape
    Cout, k = w.shape[0], w.shape[2]
    Np = proj_w.shape[0]
    if w.shape[1] != Cin or proj_w.reshape(Np, -1).shape[1] != Cout:
        raise ValueError("conv2d_groupnorm_proj: inconsistent shapes")
    proj_w = np.ascontiguousarray(proj_w.reshape(Np, Cout))
    gn_weight, gn_bias = f32(gn_weight), f32(gn_bias)
    bias = None if bias is None else f32(bias)
    proj_bias = None if proj_bias is None else f32(proj_bias)
    res = None if res is None else f16(res)
    conv_out = np.empty((B, Cout, H, W), np.float16)
    out = np.empty((B, Np, H, W), np.float16)
    ms, entries = C.c_float(0), C.c_int(0)
    check(lib().sd_op_conv2d_groupnorm_proj(ptr(x), ptr(w), fptr(bias), ptr(res), fptr(gn_weight), fptr(gn_bias), ptr(proj_w),
                                            fptr(proj_bias), ptr(conv_out), ptr(out), B, Cin, H, W, Cout, k, Np, groups, eps,
                                            int(fold), tile, C.byref(entries), iters, C.byref(ms)))
    return conv_out, out, entries.value, ms.value


def conv2d_groupnorm_conv3x3(x, w, gn_weight, gn_bias, w2, bias2=None, res2=None, bias=None, res=None, groups=32, eps=1e-5, silu=True,
                             fold=True, tile=0, staging2=0, iters=1):
    """conv3x3(silu(GroupNorm(conv(x)))) - a resnet's norm -> SiLU -> conv behind its producer; fold=True applies the GroupNorm
    (+ SiLU) in the halo loader of the second conv.  Returns (conv_out, out, entries consumed by the loader, ms)."""
    x, w, w2 = f16(x), f16(w), f16(w2)
    B, Cin, H, W = x.shape
    Cout, k = w.shape[0], w.shape[2]
    N2 = w2.shape[0]
    if w.shape[1] != Cin or w2.shape[1:] != (Cout, 3, 3):
        raise ValueError("conv2d_groupnorm_conv3x3: inconsistent shapes")
    gn_weight, gn_bias = f32(gn_weight), f32(gn_bias)
    bias = None if bias is None else f32(bias)
    bias2 = None if bias2 is None else f32(bias2)
    res = None if res is None else f16(res)
    res2 = None if res2 is None else f16(res2)
    conv_out = np.empty((B, Cout, H, W), np.float16)
    out = np.empty((B, N2, H, W), np.float16)
    ms, entries = C.c_float(0), C.c_int(0)
    check(lib().sd_op_conv2d_groupnorm_conv3x3(ptr(x), ptr(w), fptr(bias), ptr(res), fptr(gn_weight), fptr(gn_bias), ptr(w2), fptr(bias2),
                                               ptr(res2), ptr(conv_out), ptr(out), B, Cin, H, W, Cout, k, N2, groups, eps, int(silu),
                                               int(fold), tile, staging2, C.byref(entries), iters, C.byref(ms)))
    return conv_out, out, entries.value, ms.value


def cross_attention_block(x, ln_weight, ln_bias, wq, k, v, wo, bo, heads, eps=1e-5, fused=True, iters=1, a1=None, wo1=None, bo1=None):
    """x + to_out(softmax(to_q(LayerNormANE(x)) k^T / 8) v) + bo - the cross-attention branch of a BasicTransformerBlock; fused=True
    runs it as ONE launch (5 or 10 heads of 64, Sq % 32 == 0), else as the q-projection + attention launch and the to_out GEMM.
    With a1 / wo1 / bo1 the self-attention's output projection comes first: the branch runs on h1 = x + to_out1(a1) + bo1 (one
    launch: 5 heads only).  x, a1 (B,C,1,Sq), k / v (B,C,1,Sk) f16, wq / wo / wo1 (C,C) f16, bo / bo1 (C) f32.  Returns (out, ms)."""
    x, k, v, wq, wo = f16(x), f16(k), f16(v), f16(wq), f16(wo)
    B, Cn, _, Sq = x.shape
    Sk = k.shape[3]
    if Cn != heads * 64 or k.shape[1] != Cn or v.shape != k.shape or wq.shape != (Cn, Cn) or wo.shape != (Cn, Cn):
        raise ValueError("cross_attention_block: inconsistent shapes")
    ln_weight, ln_bias, bo = f32(ln_weight), f32(ln_bias), f32(bo)
    if a1 is not None:
        a1, wo1, bo1 = f16(a1), f16(wo1), f32(bo1)
        if a1.shape != x.shape or wo1.shape != (Cn, Cn):
            raise ValueError("cross_attention_block: inconsistent shapes of a1 / wo1")
    out = np.empty_like(x)
    ms = C.c_float(0)
    check(lib().sd_op_cross_attention_block(ptr(x), fptr(ln_weight), fptr(ln_bias), ptr(wq), ptr(k), ptr(v), ptr(wo), fptr(bo), ptr(a1), ptr(wo1),
                                            fptr(bo1), ptr(out), B, heads, Sq, Sk, eps, int(fused), iters, C.byref(ms)))
    return out, ms.value


def ffn_out_proj(g, w1, b1, res1, w2, b2, res2, groups=0, fused=True, iters=1):
    """res2 + proj_out(res1 + ff.net.2(g) + b1) + b2 - the tail of a SpatialTransformer; fused=True (1) runs it as ONE launch (C = 320,
    S % 32 == 0), fused=False (0) as the two GEMMs; fused = 2 .. 5: folded weights and ONE two-source GEMM (2 the library's plan, 3 the
    tiled igemm kernels, 4 / 5 smgemm.hip with 32- / 64-row tiles; ValueError for a shape the forced kernel does not tile).  g (B,4C,1,S), res1 / res2 (B,C,1,S) f16, w1 (C,4C), w2 (C,C) f16, b1 / b2 (C) f32.  groups > 0: also returns the
    GroupNorm statistics the launch left for its consumer, folded: (B, groups, 2) = (sum, sum of squares).  Returns (out, gn_sums or None, ms)."""
    g, res1, res2, w1, w2 = f16(g), f16(res1), f16(res2), f16(w1), f16(w2)
    B, Cn, _, S = res1.shape
    if g.shape != (B, 4 * Cn, 1, S) or res2.shape != res1.shape or w1.shape != (Cn, 4 * Cn) or w2.shape != (Cn, Cn):
        raise ValueError("ffn_out_proj: inconsistent shapes")
    b1, b2 = f32(b1), f32(b2)
    out = np.empty_like(res1)
    sums = np.empty((B, groups, 2), np.float32) if groups > 0 else None
    ms = C.c_float(0)
    check(lib().sd_op_ffn_out_proj(ptr(g), ptr(w1), fptr(b1), ptr(res1), ptr(w2), fptr(b2), ptr(res2), ptr(out), fptr(sums), B, Cn, S, groups,
                                   int(fused), iters, C.byref(ms)))
    return out, sums, ms.value


def fold_linear(wp, bp, w2, b2):
    """The weight fold of the merged tail on its own: (fp16(wp @ w2), bp + wp @ b2).  wp (N, J), w2 (J, K) f16, bp (N), b2 (J) f32."""
    wp, w2, bp, b2 = f16(wp), f16(w2), f32(bp), f32(b2)
    N, J = wp.shape
    K = w2.shape[1]
    if w2.shape[0] != J or bp.shape != (N,) or b2.shape != (J,):
        raise ValueError("fold_linear: inconsistent shapes")
    wm = np.empty((N, K), np.float16)
    bm = np.empty(N, np.float32)
    check(lib().sd_op_fold_linear(ptr(wp), fptr(bp), ptr(w2), fptr(b2), ptr(wm), fptr(bm), N, J, K))
    return wm, bm


def cross_attention_fused(x, ln_weight, ln_bias, wq, k, v, heads, eps=1e-5, nst=0, iters=1):
    """softmax(to_q(LayerNormANE(x)) k^T / 8) v per head (head dim 64) as one launch.  x (B,C,1,Sq), k/v (B,C,1,Sk)."""
    x, k, v, wq = f16(x), f16(k), f16(v), f16(wq)
    B, Cn, _, Sq = x.shape
    Sk = k.shape[3]
    if Cn != heads * 64 or k.shape[1] != Cn or v.shape != k.shape or wq.shape != (Cn, Cn):
        raise ValueError("cross_attention_fused: inconsistent shapes")
    ln_weight, ln_bias = f32(ln_weight), f32(ln_bias)
    out = np.empty_like(x)
    ms = C.c_float(0)
    check(lib().sd_op_cross_attention_fused(ptr(x), fptr(ln_weight), fptr(ln_bias), ptr(wq), ptr(k), ptr(v), ptr(out), B, heads,
                                            Sq, Sk, eps, nst, iters, C.byref(ms)))
    return out, ms.value


def geglu(x, w, bias=None, iters=1):
    x, w = f16(x), f16(w)
    M, Cn = x.shape
    N2 = w.shape[0]
    bias = None if bias is None else f32(bias)
    out = np.empty((M, N2 // 2), np.float16)
    ms = C.c_float(0)
    check(lib().sd_op_geglu(ptr(x), ptr(w), fptr(bias), ptr(out), M, Cn, N2, iters, C.byref(ms)))
    return out, ms.value


def geglu_ln(x, w, bias=None, ln_weight=None, ln_bias=None, eps=1e-5, kernel=0, iters=1):
    """GEGLU projection with the LayerNorm in front of it folded in (unet.py:583-591 -> :609-617).  kernel: 0 the library's plan,
    1 the tiled GEMM kernels, 2 the weight-stationary kernel (wsgemm.hip), 3-9 bvgemm.hip, 100 the one-round kernel of smgeglu.hip
    (plan tile 13) with the tile height by the grid size, 101 / 102 its 128- / 256-row tiles (ValueError for shapes it does not
    tile: it needs C % 64 == 0, N2 % 160 == 0, M a multiple of the tile height); 110-112: the same through the phase-clock build,
    which prints its per-wave cycle table to stderr."""
    x, w = f16(x), f16(w)
    M, Cn = x.shape
    N2 = w.shape[0]
    bias = None if bias is None else f32(bias)
    ln_weight = None if ln_weight is None else f32(ln_weight)
    ln_bias = None if ln_bias is None else f32(ln_bias)
    out = np.empty((M, N2 // 2), np.float16)
    ms = C.c_float(0)
    check(lib().sd_op_geglu_ln(ptr(x), fptr(ln_weight), fptr(ln_bias), ptr(w), fptr(bias), ptr(out), M, Cn, N2, eps, kernel, iters,
                               C.byref(ms)))
    return out, ms.value


def qkv_ln(x, ln_weight, ln_bias, w, batch, q_scale=1.0, vt_perm=True, eps=1e-5, kernel=0, iters=1):
    """Fused q|k|v projection with the LayerNorm in front of it folded in (unet.py:583-586 -> :74-84).  x (batch * HW, C), w (3C, C).
    Returns (out_qk (batch * HW, 2C), out_vt (batch, C, HW), ms)."""
    x, w = f16(x), f16(w)
    M, Cn = x.shape
    HW = M // batch
    out_qk = np.empty((M, 2 * Cn), np.float16)
    out_vt = np.empty((batch, Cn, HW), np.float16)
    ms = C.c_float(0)
    check(lib().sd_op_qkv_ln(ptr(x), fptr(f32(ln_weight)), fptr(f32(ln_bias)), ptr(w), ptr(out_qk), ptr(out_vt), batch, HW, Cn, eps, q_scale,
                             int(vt_perm), kernel, iters, C.byref(ms)))
    return out_qk, out_vt, ms.value


def gn_proj_qkv(x_in, conv_w, gn_weight, gn_bias, proj_w, proj_bias, ln_weight, ln_bias, wqkv, groups=32, gn_eps=1e-6, ln_eps=1e-5,
                q_scale=1.0, vt_perm=True, fused=True, iters=1):
    """conv1x1 (producer, leaves GroupNorm statistics) -> GroupNorm -> proj_in -> LayerNorm -> fused q|k|v; fused: the last four in ONE
    launch (2 / 3: its 64- / 32-token form).  Returns (h (B * HW, C), qk (B * HW, 2C), vt (B, C, HW), entries, ms)."""
    x_in, conv_w, proj_w, wqkv = f16(x_in), f16(conv_w), f16(proj_w), f16(wqkv)
    B, Cn, H, W = x_in.shape
    M = B * H * W
    h = np.empty((M, Cn), np.float16)
    qk = np.empty((M, 2 * Cn), np.float16)
    vt = np.empty((B, Cn, H * W), np.float16)
    ms, entries = C.c_float(0), C.c_int(0)
    check(lib().sd_op_gn_proj_qkv(ptr(x_in), ptr(conv_w), fptr(f32(gn_weight)), fptr(f32(gn_bias)), ptr(proj_w), fptr(f32(proj_bias)),
                                  fptr(f32(ln_weight)), fptr(f32(ln_bias)), ptr(wqkv), ptr(h), ptr(qk), ptr(vt), B, H, W, Cn, groups, gn_eps,
                                  ln_eps, q_scale, int(vt_perm), int(fused), C.byref(entries), iters, C.byref(ms)))
    return h, qk, vt, entries.value, ms.value


def conv_plan(ksize, stride, up, C0, C1, N, B, Ho, Wo, out_mode=0, flags=0, n_trans=0, n_twins=0, gnf_groups=0, tile=0, staging=0, splitk=0,
              copies=-1):
    """The plan the library gives a conv / 1x1 GEMM of this shape (sd_op_conv_plan: host only, no GPU).  flags: 1 LayerNorm fold, 2 timestep
    embedding, 4 residual, 8 GroupNorm statistics, 16 bias, 32 explicit zero padding; copies: bit set of the pre-tiled weight copies that
    exist (1 wstream, 2 wsgemm, 4 bvgemm), -1 = the ones the library's handle holds.  Returns a dict: tile, staging, splitk, slab,
    workspace_bytes, copies (wstream, wsgemm, bvgemm), kernel (sd_op_conv_plan_kernel: the line that names what launches)."""
    plan = (C.c_int * 7)()
    ws = C.c_ulonglong(0)
    desc = (ksize, stride, up, C0, C1, N, B, Ho, Wo, out_mode, flags, n_trans, n_twins, gnf_groups, tile, staging, splitk, copies)
    check(lib().sd_op_conv_plan(*desc, plan, C.byref(ws)))
    text = C.create_string_buffer(64)
    check(lib().sd_op_conv_plan_kernel(*desc, text, len(text)))
    return {"tile": plan[0], "staging": plan[1], "splitk": plan[2], "slab": bool(plan[3]), "workspace_bytes": int(ws.value),
            "copies": (bool(plan[4]), bool(plan[5]), bool(plan[6])), "kernel": text.value.decode()}


def timestep_embedding(t, dim, flip_sin_to_cos=True, freq_shift=0.0):
    t = f32(t)
    out = np.empty((t.shape[0], dim), np.float32)
    check(lib().sd_op_timestep_embedding(fptr(t), fptr(out), t.shape[0], dim, int(flip_sin_to_cos), freq_shift))
    return out


def posterior_noise(moments, eps, noise, scale_factor, sa, sb, iters=1):
    """The image-to-image start as one launch (csrc/misc.hip posterior_noise_kernel; Encoder.swift:68-89 + Scheduler.swift:83-102):
    moments (2*Cz, h, w) or (1, 2*Cz, h, w) f32 = [mean | logvar], eps (Cz, h, w), noise (n_images, Cz, h, w) f32 ->
    (sa * (mean + exp(0.5 * clamp(logvar, -30, 20)) * eps) * scale_factor + sb * noise[i], ms)."""
    moments, eps, noise = f32(moments), f32(eps), f32(noise)
    if noise.ndim != 4:
        raise ValueError("posterior_noise: noise must be (n_images, Cz, h, w)")
    n_images, Cz, h, w = noise.shape
    if moments.size != 2 * Cz * h * w or moments.shape[-3:] != (2 * Cz, h, w) or eps.shape[-3:] != (Cz, h, w) or eps.size != Cz * h * w:
        raise ValueError("posterior_noise: moments must be (2*Cz, h, w) and eps (Cz, h, w) for noise (n_images, Cz, h, w)")
    out = np.empty_like(noise)
    ms = C.c_float(0)
    check(lib().sd_op_posterior_noise(fptr(moments), fptr(eps), fptr(noise), fptr(out), Cz, h, w, n_images, float(scale_factor), float(sa),
                                      float(sb), iters, C.byref(ms)))
    return out, ms.value


def sched_step(noise_pred, latents, coef, guidance=1.0, hist=None, pred=None, step_noise=None):
    """One launch of the loop's step kernel (csrc/misc.hip cfg_sched_step_kernel; sd_op_sched_step): noise_pred (cfg * n_images, n),
    latents (n_images, n), hist (history, n_images, n) or None, coef (8,), pred (8,) or None, step_noise (n_images, n) or None, all
    f32; cfg = noise_pred rows / latents rows.  Returns (latents, hist or None, denoised or None, step counter behind the launch)."""
    noise_pred, lat, coef = f32(noise_pred), f32(latents).copy(), f32(coef)
    if lat.ndim != 2 or noise_pred.ndim != 2 or noise_pred.shape[1] != lat.shape[1] or noise_pred.shape[0] % lat.shape[0] or coef.shape != (8,):
        raise ValueError("sched_step: noise_pred must be (cfg * n_images, n), latents (n_images, n) and coef (8,)")
    n_images, n = lat.shape
    cfg = noise_pred.shape[0] // n_images
    history = 0 if hist is None else len(hist)
    hs = None if hist is None else f32(hist).copy()
    if hs is not None and hs.shape != (history, n_images, n):
        raise ValueError("sched_step: hist must be (history, n_images, n)")
    pr = None if pred is None else f32(pred)
    sn = None if step_noise is None else f32(step_noise)
    if (pr is not None and pr.shape != (8,)) or (sn is not None and sn.shape != lat.shape):
        raise ValueError("sched_step: pred must be (8,) and step_noise (n_images, n)")
    den = None if pr is None else np.empty_like(lat)
    step = C.c_int(-1)
    check(lib().sd_op_sched_step(fptr(noise_pred), fptr(lat), fptr(hs), fptr(coef), fptr(pr), fptr(sn), float(guidance), cfg, history,
                                 n_images, n, fptr(den), C.byref(step)))
    return lat, hs, den, step.value


def numpy_randn(seed, n):
    out = np.empty(n, np.float64)
    check(lib().sd_numpy_randn(seed, out.ctypes.data_as(C.POINTER(C.c_double)), n))
    return out


def torch_randn(seed, n):
    """torch.manual_seed(seed); torch.randn(n) on the CPU (TorchRandomSource.swift)."""
    out = np.empty(n, np.float64)
    check(lib().sd_torch_randn(seed, out.ctypes.data_as(C.POINTER(C.c_double)), n))
    return out


def philox_randn(seed, n, offset=0):
    """torch.randn on a CUDA device (NvRandomSource.swift); offset = arrays drawn before this one."""
    out = np.empty(n, np.float64)
    check(lib().sd_philox_randn(seed, offset, out.ctypes.data_as(C.POINTER(C.c_double)), n))
    return out


def calibrate(device=0):
    """Nine fixed micro-measurements of the box (calib.hip): what bench.py prints as `calibration` and normalises by."""
    out = (C.c_float * 9)()
    check(lib().sd_calibrate(device, out))
    return {"copy_gbs": round(out[0], 1), "mfma_tflops": round(out[1], 1), "empty_launch_us": round(out[2], 3),
            "chain_us": round(out[3], 3), "handover_us": round(out[4], 3), "latency_hbm_ns": round(out[5], 1),
            "latency_cache_ns": round(out[6], 1), "small_grid_us": round(out[7], 3), "cold_code_us": round(out[8], 3)}


# ------------------------------------------------------------------------------------------------
# the kernels that otherwise run only inside whole models (sd_mi355x.h, last section).  The wrappers check that the arrays fit
# together (ValueError, before the library is called); what a kernel cannot do is the library's refusal (NotImplementedError).
# ------------------------------------------------------------------------------------------------
def conv_f32(x, w, bias=None, res=None, stride=1, upsample=False, pad_mode=0, w_kind=1):
    """fp32 conv of an fp32 VAE handle (csrc/vae_f32.hip conv_f32_kernel).  x (B,Cin,H,W) f32; w_kind 0: w (N,Cin,k,k) rounded to f16,
    1: w (N,Cin,k,k) f32, 2: w (Cin,N) f32, a 1x1 conv whose weights are stored [K][N]; bias (N), res (B,N,Ho,Wo) f32 or None;
    pad_mode 1: the encoder's (0,1,0,1) padding (3x3, stride 2) -> (B,N,Ho,Wo) f32."""
    if w_kind not in (0, 1, 2):
        raise ValueError(f"conv_f32: w_kind {w_kind}")
    x = f32(x)
    w = f16(w) if w_kind == 0 else f32(w)
    if x.ndim != 4:
        raise ValueError("conv_f32: x must be (B, Cin, H, W)")
    B, Cin, H, W = x.shape
    if w_kind == 2:
        if w.ndim != 2 or w.shape[0] != Cin:
            raise ValueError("conv_f32: w_kind 2 takes w (Cin, N)")
        N, k = w.shape[1], 1
    else:
        if w.ndim != 4 or w.shape[1] != Cin or w.shape[2] != w.shape[3] or w.shape[2] not in (1, 3):
            raise ValueError("conv_f32: w must be (N, Cin, k, k) with k 1 or 3")
        N, k = w.shape[0], w.shape[2]
    if stride not in (1, 2) or pad_mode not in (0, 1) or (pad_mode == 1 and (k != 3 or stride != 2 or upsample)):
        raise ValueError("conv_f32: stride 1 or 2; pad_mode 1 needs a 3x3 / stride-2 conv without upsample")
    up = 2 if upsample else 1
    extra = 1 if pad_mode else 2 * (k // 2)
    Ho, Wo = (H * up + extra - k) // stride + 1, (W * up + extra - k) // stride + 1
    if Ho < 1 or Wo < 1:
        raise ValueError("conv_f32: empty output")
    bias = None if bias is None else f32(bias)
    res = None if res is None else f32(res)
    if (bias is not None and bias.shape != (N,)) or (res is not None and res.shape != (B, N, Ho, Wo)):
        raise ValueError("conv_f32: bias must be (N,), res (B, N, Ho, Wo)")
    out = np.empty((B, N, Ho, Wo), np.float32)
    check(lib().sd_op_conv_f32(fptr(x), ptr(w), w_kind, fptr(bias), fptr(res), fptr(out), B, Cin, H, W, N, k, stride, int(bool(upsample)),
                               pad_mode))
    return out


def groupnorm_f32(x, gamma, beta, groups, eps=1e-6, silu=False):
    """fp32 GroupNorm (+ SiLU) of an fp32 VAE handle (csrc/vae_f32.hip).  x (B,C,H,W) f32, gamma / beta (C,) -> (B,C,H,W) f32."""
    x, gamma, beta = f32(x), f32(gamma), f32(beta)
    if x.ndim != 4 or gamma.shape != (x.shape[1],) or beta.shape != gamma.shape or groups < 1:
        raise ValueError("groupnorm_f32: x must be (B, C, H, W), gamma and beta (C,), groups >= 1")
    B, Cn, H, W = x.shape
    out = np.empty_like(x)
    check(lib().sd_op_groupnorm_f32(fptr(x), fptr(gamma), fptr(beta), fptr(out), B, Cn, H, W, int(groups), float(eps), int(bool(silu))))
    return out


def row_softmax(x, scale=1.0):
    """softmax(scale * x) over the last axis of x (rows, cols): a float16 array runs csrc/norm.hip row_softmax_kernel, a float32 one
    csrc/vae_f32.hip row_softmax_f32_kernel.  Returns a new array of x's dtype."""
    if not isinstance(x, np.ndarray) or x.dtype not in (np.float16, np.float32) or x.ndim != 2 or x.size == 0:
        raise ValueError("row_softmax: x must be a non-empty (rows, cols) float16 or float32 array")
    y = np.array(x, order="C", copy=True)
    check(lib().sd_op_row_softmax(ptr(y), y.shape[0], y.shape[1], float(scale), int(y.dtype == np.float32)))
    return y


def gemv(w, bias, x, init=None, silu_in=False, silu_out=False):
    """The time-embedding GEMV (csrc/misc.hip gemv_kernel): act_out(act_in(x) @ w.T + bias) [+ init].  w (N,K) f16, bias (N,) f32 or
    None, x (B,K) f32, init (B,N) f32 or None (given: the launch accumulates onto it) -> (B,N) f32."""
    w, x = f16(w), f32(x)
    if w.ndim != 2 or x.ndim != 2 or x.shape[1] != w.shape[1]:
        raise ValueError("gemv: w must be (N, K) and x (B, K)")
    N, K = w.shape
    B = x.shape[0]
    bias = None if bias is None else f32(bias)
    if bias is not None and bias.shape != (N,):
        raise ValueError("gemv: bias must be (N,)")
    if init is not None and np.shape(init) != (B, N):
        raise ValueError("gemv: init must be (B, N)")
    out = np.empty((B, N), np.float32) if init is None else np.array(init, dtype=np.float32, order="C", copy=True)
    check(lib().sd_op_gemv(ptr(w), fptr(bias), fptr(x), fptr(out), B, N, K, int(bool(silu_in)), int(bool(silu_out)), int(init is not None)))
    return out


def clip_attention(qkv, heads):
    """Causal attention of the text encoder (csrc/clip.hip): qkv (S, 3 D) f16 rows [q | k | v] -> (S, D) f16."""
    qkv = f16(qkv)
    if qkv.ndim != 2 or qkv.shape[1] % 3 or heads < 1 or (qkv.shape[1] // 3) % heads:
        raise ValueError("clip_attention: qkv must be (S, 3 * heads * dim_head)")
    S, D = qkv.shape[0], qkv.shape[1] // 3
    out = np.empty((S, D), np.float16)
    check(lib().sd_op_clip_attention(ptr(qkv), ptr(out), S, D, int(heads)))
    return out


def clip_embed(ids, tok, pos):
    """Token + position embedding of the text encoder (csrc/clip.hip): ids (S,) int, tok (vocab, D), pos (S, D) f16 -> (S, D) f16;
    ids outside [0, vocab) are clamped."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    tok, pos = f16(tok), f16(pos)
    if ids.ndim != 1 or tok.ndim != 2 or pos.shape != (ids.shape[0], tok.shape[1]):
        raise ValueError("clip_embed: ids (S,), tok (vocab, D), pos (S, D)")
    out = np.empty_like(pos)
    check(lib().sd_op_clip_embed(ids.ctypes.data_as(C.POINTER(C.c_int32)), ptr(tok), ptr(pos), ptr(out), pos.shape[0], pos.shape[1],
                                 tok.shape[0]))
    return out


def clip_act(x, act):
    """The CLIP MLP activation (csrc/clip.hip clip_act_kernel) over a float16 array: act "quick_gelu" or "gelu"."""
    if act not in ACTS:
        raise ValueError(f"clip_act: unknown activation {act!r}")
    y = np.array(x, dtype=np.float16, order="C", copy=True)
    check(lib().sd_op_clip_act(ptr(y), y.size, ACTS[act]))
    return y


# sd_op_layout kinds by (operation, source dtype, destination dtype)
_LAYOUTS = {("nchw_to_nhwc", "float16", "float16"): 0, ("nchw_to_nhwc", "float32", "float16"): 1,
            ("nchw_to_nhwc", "float16", "float32"): 2, ("nchw_to_nhwc", "float32", "float32"): 3,
            ("nhwc_to_nchw", "float16", "float32"): 4, ("nhwc_to_nchw", "float32", "float32"): 5,
            ("bc1s_to_tokens", "float16", "float16"): 6, ("convert", "float16", "float32"): 7, ("convert", "float32", "float16"): 8}


def layout(op, src, dst_dtype):
    """The copy kernels at the model boundaries (csrc/misc.hip, csrc/vae_f32.hip).  op "nchw_to_nhwc": src (B,C,H,W) -> (B,H,W,C);
    "nhwc_to_nchw": src (B,H,W,C) -> (B,C,H,W) float32; "bc1s_to_tokens": src (B,C,1,S) -> (B,S,C) float16; "convert": float16 <->
    float32 of any array.  The pair of src.dtype and dst_dtype selects the kernel; a pair no kernel serves is a ValueError."""
    if not isinstance(src, np.ndarray):
        raise ValueError("layout: src must be a numpy array")
    kind = _LAYOUTS.get((op, src.dtype.name, np.dtype(dst_dtype).name))
    if kind is None:
        raise ValueError(f"layout: no kernel for {op!r} from {src.dtype.name} to {np.dtype(dst_dtype).name}")
    src = np.ascontiguousarray(src)
    if op == "convert":
        if src.size == 0:
            raise ValueError("layout: empty array")
        dims, shape = (1, 1, 1, src.size), src.shape
    else:
        if src.ndim != 4 or src.size == 0 or (op == "bc1s_to_tokens" and src.shape[2] != 1):
            raise ValueError("layout: src must be a non-empty 4-d array ((B, C, 1, S) for bc1s_to_tokens)")
        if op == "nhwc_to_nchw":
            B, H, W, Cn = src.shape
            shape = (B, Cn, H, W)
        else:
            B, Cn, H, W = src.shape
            shape = (B, W, Cn) if op == "bc1s_to_tokens" else (B, H, W, Cn)
        dims = (B, Cn, H, W)
    dst = np.empty(shape, dst_dtype)
    check(lib().sd_op_layout(kind, ptr(src), ptr(dst), *dims))
    return dst


def sum_half(srcs, add=False):
    """Sum of 1 to 4 float16 arrays of one shape, fp32 accumulation in source order and one rounding (csrc/misc.hip sum_half_kernel);
    add=True: the two-source add_half_kernel."""
    srcs = [f16(a) for a in srcs]
    if not srcs or any(a.shape != srcs[0].shape for a in srcs) or srcs[0].size == 0 or (add and len(srcs) != 2):
        raise ValueError("sum_half: one or more non-empty arrays of one shape (add=True: exactly two)")
    out = np.empty_like(srcs[0])
    arr = (C.c_void_p * len(srcs))(*[a.ctypes.data for a in srcs])
    check(lib().sd_op_sum_half(arr, len(srcs), ptr(out), out.size, int(bool(add))))
    return out


def harness_selftest(mode, src):
    """Self-check of the operator harness (sd_mi355x.h sd_op_harness_selftest): float32(src) with the deliberate off-by-one of
    ``mode`` (0 none).  Returns (status, error text, dst): nothing is raised, so that a test sees what a refused call left in dst."""
    src = f16(src).ravel()
    dst = np.zeros(src.size, np.float32)
    status = lib().sd_op_harness_selftest(int(mode), ptr(src), fptr(dst), src.size)
    return status, lib().sd_last_error().decode("utf-8", "replace"), dst


def vit_patch_rows(img, patch, row):
    """Patch rows of the vision tower's embedding conv (csrc/vit.hip): img (B,3,I,I) f16 -> (B * (I / patch)^2, row) f16, the columns
    behind 3 * patch * patch zero."""
    img = f16(img)
    if img.ndim != 4 or img.shape[1] != 3 or img.shape[2] != img.shape[3] or patch < 1 or img.shape[2] % patch or row < 3 * patch * patch:
        raise ValueError("vit_patch_rows: img (B, 3, I, I), I a multiple of patch, row >= 3 * patch * patch")
    B, I = img.shape[0], img.shape[2]
    out = np.empty((B * (I // patch) ** 2, row), np.float16)
    check(lib().sd_op_vit_patch_rows(ptr(img), ptr(out), B, I, int(patch), int(row)))
    return out


def vit_tokens(patch, cls, pos):
    """Class token + position embeddings of the vision tower (csrc/vit.hip): patch (B, S - 1, D), cls (D,), pos (S, D) f16 ->
    (B, S, D) f16."""
    patch, cls, pos = f16(patch), f16(cls), f16(pos)
    if patch.ndim != 3 or cls.shape != (patch.shape[2],) or pos.shape != (patch.shape[1] + 1, patch.shape[2]):
        raise ValueError("vit_tokens: patch (B, S - 1, D), cls (D,), pos (S, D)")
    B, S, D = patch.shape[0], patch.shape[1] + 1, patch.shape[2]
    out = np.empty((B, S, D), np.float16)
    check(lib().sd_op_vit_tokens(ptr(patch), ptr(cls), ptr(pos), ptr(out), B, S, D))
    return out
