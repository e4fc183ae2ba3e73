"""ctypes binding of libtsd.so (include/tsd.h) - the only way the Python host reaches the GPU.

There is no CPU fallback: if the shared library is missing or no gfx950 device is visible every
compute call fails loudly.  Shape errors follow the reference's convention (print a message and
return a null matrix, e.g. helpers/utils.mojo:1955-1957) unless `set_strict(True)`.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# TSD_LIB names another build of the same library (the -DTSD_JITTER hazard-hunting build of `make jitter`); never a different backend
LIB_PATH = os.environ.get("TSD_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libtsd.so")

TSD_OK, TSD_E_ARG, TSD_E_SHAPE, TSD_E_ALLOC, TSD_E_HIP, TSD_E_RCCL, TSD_E_STATE, TSD_E_NONFINITE = 0, -1, -2, -3, -4, -5, -6, -7
# Kernel arguments in device memory instead of host-coherent memory: every kernel starts by reading its ~200 B argument
# block, and fetching it across the host link costs ~2 us per launch (measured: 169 -> 177 steps/s).  The HIP runtime
# reads the switch when it initialises, so it goes into the environment as soon as this package is imported - before
# libtsd.so (or torch, in the multi-GPU bench) makes the process's first HIP call.
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

MODEL_DIFFUSION, MODEL_DECODER, MODEL_ENCODER, MODEL_CLIP, MODEL_DIFFUSION_SD15, MODEL_DIFFUSION_SD15_TORCH = 1, 2, 3, 4, 5, 6
MODEL_CLIP_TORCH, MODEL_DECODER_TORCH, MODEL_ENCODER_TORCH = 7, 8, 9
MODEL_CONTROLNET_SD15, MODEL_CONTROLNET_SD15_TORCH = 10, 11
MODEL_DIFFUSION_SD2, MODEL_CLIP_SD2 = 16, 17    # 12 - 15 are reserved and refused
MODEL_IP_ADAPTER_SD15 = 20                      # 18 and 19 are refused as well
MODEL_CLIP_VISION_H = 22                        # ... and so are 21 and 23
MODEL_IP_ADAPTER_PLUS_SD15 = 24
SAMPLER_KINDS = {"ddpm": 0, "ddim": 1, "dpmpp_2m": 2}      # tsd_sampler_kind
TIMESTEP_SPACINGS = {"leading": 0, "trailing": 1}          # tsd_timestep_spacing
MASK_MODES = {"area": 0, "any": 1}                         # tsd_mask_mode
PREDICTION_TYPES = {"epsilon": 0, "v": 1}                  # tsd_prediction_type ("v_prediction": diffusers' name for "v")


def sampler_kind(kind):
    """"ddpm" | "ddim" | "dpmpp_2m" (or the enum value) -> tsd_sampler_kind; an unknown name goes to the library, which refuses it."""
    return SAMPLER_KINDS.get(kind.lower(), -1) if isinstance(kind, str) else int(kind)


def timestep_spacing(spacing):
    """"leading" | "trailing" (or the enum value) -> tsd_timestep_spacing."""
    return TIMESTEP_SPACINGS.get(spacing.lower(), -1) if isinstance(spacing, str) else int(spacing)


def mask_mode(mode):
    """"area" | "any" (or the enum value) -> tsd_mask_mode."""
    return MASK_MODES.get(mode.lower(), -1) if isinstance(mode, str) else int(mode)


def prediction_type(prediction):
    """"epsilon" | "v" | "v_prediction" (or the enum value) -> tsd_prediction_type; an unknown name goes to the library, which refuses it."""
    if isinstance(prediction, str):
        name = prediction.lower()
        return PREDICTION_TYPES.get("v" if name == "v_prediction" else name, -1)
    return int(prediction)


def check_guidance_rescale(phi, cfg=True):
    """A guidance rescale in [0, 1] as a float; ValueError outside it (NaN included) and for a positive value without CFG."""
    phi = float(phi)
    if not (0.0 <= phi <= 1.0):
        raise ValueError(f"guidance_rescale must be between 0 and 1, got {phi}")
    if phi > 0.0 and not cfg:
        raise ValueError("guidance_rescale rescales the classifier-free-guidance combine: it needs cfg=True")
    return phi


class TsdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libtsd error {code}: {msg}")
        self.code = code


_lib = None
_strict = False
fp = C.POINTER(C.c_float)
vp = C.c_void_p


def set_strict(flag: bool):
    """strict=True raises TsdError on every non-zero status; default mirrors the reference
    (print + null matrix) for TSD_E_SHAPE only."""
    global _strict
    _strict = bool(flag)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TsdError(TSD_E_HIP, f"{LIB_PATH} not built - run __graft_entry__.build() (hipcc, gfx950); "
                                      "there is no CPU fallback")
        _lib = C.CDLL(LIB_PATH)
        _declare(_lib)
    return _lib


def _declare(l):
    i, i64, f, u64, sz = C.c_int, C.c_int64, C.c_float, C.c_uint64, C.c_size_t
    pp = C.POINTER(vp)
    sig = {
        "tsd_version": ([], i), "tsd_last_error": ([], C.c_char_p), "tsd_device_count": ([], i),
        "tsd_ctx_create": ([i, pp], i), "tsd_ctx_destroy": ([vp], i), "tsd_ctx_synchronize": ([vp], i),
        "tsd_ctx_timer_start": ([vp], i), "tsd_ctx_timer_stop": ([vp, fp], i),
        "tsd_ctx_profile_begin": ([vp], i), "tsd_ctx_profile_records": ([vp, C.POINTER(i), fp, i], i), "tsd_ctx_profile_end": ([vp, fp, C.POINTER(i), i], i),
        "tsd_conv2d_f32": ([vp, fp, i, i, i, fp, fp, i, i, i, i, i, i, i, fp], i),
        "tsd_pad_f32": ([vp, fp, i, i, i, i, i, i, i, fp], i),
        "tsd_groupnorm_f32": ([vp, fp, i, i, i, i, i, f, f, fp], i),
        "tsd_layernorm_f32": ([vp, fp, i, i, f, fp], i),
        "tsd_groupnorm_affine_f32": ([vp, fp, i, i, i, i, f, fp, fp, i, fp], i),
        "tsd_layernorm_affine_f32": ([vp, fp, i, i, f, fp, fp, fp], i),
        "tsd_silu_f32": ([vp, fp, i64, fp], i), "tsd_gelu_tanh_f32": ([vp, fp, i64, fp], i),
        "tsd_rescale_images_f32": ([vp, fp, i64, fp], i),
        "tsd_linear_f32": ([vp, fp, i, i, fp, fp, i, fp], i),
        "tsd_matmul_f32": ([vp, fp, fp, i, i, i, i, i, fp], i),
        "tsd_upsample_nearest2x_f32": ([vp, fp, i, i, i, fp], i),
        "tsd_softmax_lastdim_f32": ([vp, fp, i64, i, fp], i),
        "tsd_self_attention_f32": ([vp, fp, i, i, i, fp, fp, fp, fp, i, fp], i),
        "tsd_cross_attention_f32": ([vp, fp, i, i, fp, i, i, i, fp, fp, fp, fp, fp, fp, fp, fp, fp], i),
        "tsd_time_embedding_f32": ([vp, f, fp], i),
        "tsd_time_embedding_mlp_f32": ([vp, fp, fp, fp, fp, fp, fp], i),
        "tsd_unet_residual_block_f32": ([vp, fp, i, i, i, fp, i, i, fp, fp, fp, fp, fp, fp, fp, fp, fp], i),
        "tsd_unet_attention_block_f32": ([vp, fp, i, i, i, i, fp, i, i, C.POINTER(fp), i, fp], i),
        "tsd_vae_res_block_f32": ([vp, fp, i, i, i, i, fp, fp, fp, fp, fp, fp, fp], i),
        "tsd_vae_attention_block_f32": ([vp, fp, i, i, i, fp, fp, fp, fp, fp], i),
        "tsd_model_param_count": ([i], i),
        "tsd_model_param_info": ([i, i, C.c_char_p, i, C.POINTER(i64), C.POINTER(i), C.POINTER(i), fp], i),
        "tsd_model_create": ([vp, i, pp], i), "tsd_model_destroy": ([vp], i),
        "tsd_model_set_param": ([vp, i, fp, i64], i), "tsd_model_init_random": ([vp, u64], i),
        "tsd_model_packed_blob": ([vp, pp, C.POINTER(sz)], i), "tsd_model_mark_loaded": ([vp], i), "tsd_model_prepare": ([vp], i),
        "tsd_model_lora_add": ([vp, i, i, i, fp, fp, i, f], i), "tsd_model_lora_clear": ([vp], i), "tsd_model_lora_count": ([vp], i),
        "tsd_model_get_param": ([vp, i, fp, i64], i), "tsd_debug_model_packed_param": ([vp, i, vp, sz], i),
        "tsd_lora_merge_f32": ([vp, fp, i, i, i, i, i, i, fp, fp, i, f, fp], i),
        "tsd_diffusion_forward": ([vp, fp, fp, fp, i, i, i, fp], i),
        "tsd_decoder_forward": ([vp, fp, i, i, fp], i),
        "tsd_encoder_forward": ([vp, fp, fp, i, i, fp], i),
        "tsd_diffusion_forward_hw": ([vp, fp, fp, fp, i, i, i, i, fp], i),
        "tsd_decoder_forward_hw": ([vp, fp, i, i, i, fp], i),
        "tsd_encoder_forward_hw": ([vp, fp, fp, i, i, i, fp], i),
        "tsd_clip_forward": ([vp, C.POINTER(C.c_int32), i, i, fp], i),
        "tsd_model_context_width": ([vp], i),
        "tsd_controlnet_forward_hw": ([vp, fp, fp, fp, fp, i, i, i, i, C.POINTER(fp)], i),
        "tsd_diffusion_forward_control_hw": ([vp, vp, fp, fp, fp, fp, fp, i, i, i, i, fp], i),
        "tsd_control_inject_f16": ([vp, i, pp, pp, i, C.POINTER(i), C.POINTER(i), C.POINTER(i), C.POINTER(i), fp, pp, C.POINTER(fp)], i),
        "tsd_debug_set_control_stats": ([vp, i], i),
        "tsd_controlnet_hint_hw": ([vp, fp, i, i, i, fp], i),
        "tsd_session_set_control": ([vp, vp, fp, f, i, i, i], i), "tsd_session_control_active": ([vp], i),
        "tsd_ip_adapter_project": ([vp, fp, i, fp], i), "tsd_ip_adapter_resample": ([vp, fp, i, i, fp], i),
        "tsd_diffusion_forward_ip_hw": ([vp, vp, fp, i, fp, vp, fp, fp, fp, fp, fp, i, i, i, i, fp], i),
        "tsd_ip_attn_add_f16": ([vp, vp, vp, vp, vp, fp, i, i, i, i, i, f, vp], i),
        "tsd_session_set_ip_adapter": ([vp, vp, fp, fp, i, f, i, i], i), "tsd_session_ip_adapter_active": ([vp], i),
        "tsd_debug_ip_attn_run": ([vp, C.POINTER(i64), i, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), C.POINTER(i64)], i),
        "tsd_debug_ip_attn_bench": ([vp, i, i, i, i, i, i, fp], i),
        "tsd_clip_image_patches_f16": ([vp, fp, i, i, i, vp], i),
        "tsd_model_set_freeu": ([vp, fp, fp, i], i), "tsd_model_freeu": ([vp, fp, fp, C.POINTER(i)], i),
        "tsd_freeu_f16": ([vp, vp, vp, i, i, i, i, i, f, f, i, vp, vp], i),
        "tsd_debug_freeu_run": ([vp, vp, vp, i, i, i, i, i, i, i, i, f, f, i, vp, vp], i),
        "tsd_clip_vision_forward": ([vp, fp, i, i, i, fp, fp], i),
        "tsd_debug_image_patches_run": ([vp, C.POINTER(i64), i, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), C.POINTER(i64)], i),
        "tsd_tokenizer_create": ([C.c_char_p, i, C.POINTER(vp)], i),
        "tsd_tokenizer_create_from_memory": ([C.c_char_p, C.c_size_t, i, C.POINTER(vp)], i),
        "tsd_tokenizer_destroy": ([vp], i),
        "tsd_tokenizer_find": ([vp, C.c_char_p], i),
        "tsd_tokenizer_token": ([vp, i, C.c_char_p, i, fp], i),
        "tsd_tokenizer_encode": ([vp, C.c_char_p, C.POINTER(C.c_int32), i, C.POINTER(C.c_int), C.POINTER(C.c_int)], i),
        "tsd_session_create": ([vp, vp, i, i, i, i, pp], i), "tsd_session_destroy": ([vp], i),
        "tsd_session_create_hw": ([vp, vp, i, i, i, i, i, pp], i), "tsd_session_shape": ([vp, C.POINTER(i), C.POINTER(i)], i),
        "tsd_session_set_schedule": ([vp, i, i, i], i), "tsd_session_num_steps": ([vp], i),
        "tsd_session_set_sampler": ([vp, i, f, i], i),
        "tsd_sampler_timesteps": ([i, i, i, i, C.POINTER(i), i], i),
        "tsd_sampler_coeffs": ([i, C.c_double, i, i, i, i, i, i, C.POINTER(C.c_double)], i),
        "tsd_sampler_step_f32": ([vp, fp, fp, fp, f, fp, fp, i64, fp, fp, fp], i),
        "tsd_sampler_alphas_cumprod": ([i, i, fp, i], i),
        "tsd_sampler_coeffs_ex": ([i, C.c_double, i, i, i, i, i, i, i, i, C.POINTER(C.c_double)], i),
        "tsd_sampler_step_v_f32": ([vp, fp, fp, fp, f, fp, fp, i64, fp, fp, fp], i),
        "tsd_session_set_prediction": ([vp, i, i], i), "tsd_session_prediction": ([vp, C.POINTER(i), C.POINTER(i)], i),
        "tsd_ddpm_step_f32": ([vp, fp, fp, fp, f, fp, i64, i, i, i, i, i, fp], i),
        "tsd_cfg_rescale_f32": ([vp, fp, fp, i, i64, fp, fp, fp, fp, fp], i),
        "tsd_session_set_guidance_rescale": ([vp, f], i), "tsd_session_guidance_rescale": ([vp, fp], i),
        "tsd_session_slot_set_guidance_rescale": ([vp, i, f], i), "tsd_session_slot_guidance_rescale": ([vp, i, fp], i),
        "tsd_latent_mask_f32": ([vp, fp, i, i, i, fp], i),
        "tsd_latent_mask_hw_f32": ([vp, fp, i, i, i, i, fp], i),
        "tsd_inpaint_blend_f32": ([vp, fp, fp, fp, fp, i, i64, f, f, fp], i),
        "tsd_session_set_inpaint": ([vp, fp, fp, fp], i), "tsd_session_inpaint_active": ([vp], i),
        "tsd_normal_fill_f32": ([vp, u64, u64, u64, i64, fp], i),
        "tsd_session_set_seeds": ([vp, C.POINTER(u64)], i), "tsd_session_seeds_active": ([vp], i),
        "tsd_session_seed_latents": ([vp], i), "tsd_session_add_noise_seeded": ([vp, i], i),
        "tsd_session_set_inpaint_seeded": ([vp, fp, fp], i),
        "tsd_session_timestep": ([vp, i], i),
        "tsd_session_upload": ([vp, fp, fp, fp, fp, f], i), "tsd_session_step": ([vp, i], i),
        "tsd_session_add_noise": ([vp, i, fp], i), "tsd_session_decode": ([vp], i),
        "tsd_session_download_latents": ([vp, fp], i), "tsd_session_download_images": ([vp, i, fp], i),
        "tsd_session_slots_open": ([vp], i), "tsd_session_slot_start": ([vp, i, fp, fp, fp, i, u64, i, f], i),
        "tsd_session_advance": ([vp, C.POINTER(C.c_uint32)], i), "tsd_session_slot_state": ([vp, i, C.POINTER(i), C.POINTER(i)], i),
        "tsd_session_slot_download": ([vp, i, fp], i), "tsd_session_slots_active": ([vp], i),
        "tsd_session_slot_set_inpaint": ([vp, i, fp, fp], i), "tsd_session_slot_inpaint_active": ([vp, i], i),
        "tsd_dist_unique_id": ([vp], i), "tsd_dist_init": ([vp, i, i, vp], i),
        "tsd_dist_broadcast_weights": ([vp, i], i), "tsd_dist_finalize": ([vp], i),
        "tsd_dist_comm_count": ([vp, C.POINTER(i)], i),
        "tsd_flop_count": ([i, i, i], C.c_double),
        "tsd_debug_splitk_errors": ([vp], i),
        "tsd_debug_xcd_round_robin": ([], i),
        "tsd_debug_nonfinite_count": ([vp, i], i),
        "tsd_debug_scribble": ([vp, i], i),
        "tsd_debug_set_fused_attention": ([vp, i], i),
        "tsd_debug_gemm_bench": ([vp, i, i, i, i, i, i, i, i, i, i, fp], i),
        "tsd_debug_attn_bench": ([vp, i, i, i, i, i, i, fp], i),
        "tsd_debug_attn_exact_passes": ([vp, i], i),
        "tsd_debug_set_attn_qb": ([vp, i], i),
        "tsd_debug_set_attn_diag": ([vp, i], i),
        "tsd_debug_set_res_fuse_skip": ([vp, i], i),
        "tsd_debug_set_qkv_fuse": ([vp, i], i),
        "tsd_debug_set_session_hoist": ([vp, i], i),
        "tsd_debug_session_hoist_info": ([vp, C.POINTER(i64)], i),
        "tsd_debug_session_latents": ([vp, fp], i),
        "tsd_debug_mfma_sustained": ([vp, C.c_float, fp, fp], i),
        "tsd_debug_gemm_check": ([vp, i, i, i, i, i, i, i, i, i, i, fp, fp], i),
        "tsd_debug_gemm_record": ([vp, i], i),
        "tsd_debug_gemm_recorded": ([vp, i, C.POINTER(i64), i], i),
        "tsd_debug_model_fold": ([vp, i, vp, fp], i),
        "tsd_debug_model_dup_fold": ([vp, vp, vp], i),
        "tsd_debug_dup_fold_host": ([vp, i, i, i, i, vp, i], i64),
        "tsd_debug_ups_fold_host": ([vp, i, i, i, vp], i64),
        "tsd_debug_model_ups_fold": ([vp, i, vp], i),
        "tsd_debug_set_ups_fold": ([vp, i], i),
        "tsd_debug_gemm_run": ([vp, C.POINTER(i64), i, i, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), C.POINTER(i64)], i),
        "tsd_debug_gemm_plan": ([vp, C.POINTER(i64), i, i, C.POINTER(i64)], i),
        "tsd_debug_norm_run": ([vp, C.POINTER(i64), i, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), C.POINTER(i64)], i),
        "tsd_debug_attn_run": ([vp, C.POINTER(i64), i, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), C.POINTER(i64)], i),
        "tsd_debug_chain_run": ([vp, C.POINTER(i64), i, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), C.POINTER(i64)], i),
        "tsd_debug_elem_run": ([vp, C.POINTER(i64), i, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), C.POINTER(i64)], i),
        "tsd_debug_gn_path_counts": ([vp, C.POINTER(i64), i, i], i),
        "tsd_debug_jitter_selftest": ([vp, i], i),
        "tsd_debug_device_ledger": ([C.POINTER(i64), i], i),
    }
    for name, (args, res) in sig.items():
        fn = getattr(l, name)
        fn.argtypes = args
        fn.restype = res


EXPORTS = None  # filled lazily for the symbol test


def _header():
    """include/tsd.h without its comments."""
    import re
    hdr = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "tsd.h")
    return re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)


def declared_symbols():
    """Names of every function declared in include/tsd.h (parsed, so the test cannot drift)."""
    import re
    return sorted(set(re.findall(r"\b(tsd_[a-z0-9_]+)\s*\(", _header())))


def header_enum(name, prefix=""):
    """{enumerator without `prefix`: value} of `enum name` in include/tsd.h (parsed, so the names cannot drift from the library's)."""
    import re
    out, v = {}, 0
    for item in re.search(r"enum\s+" + name + r"\s*\{(.*?)\}", _header(), re.S).group(1).split(","):
        item = item.strip()
        if not item:
            continue
        if "=" in item:
            item, val = (s.strip() for s in item.split("="))
            v = int(val, 0)
        out[item[len(prefix):] if item.startswith(prefix) else item] = v
        v += 1
    return out


_ledger_fields = None


def device_ledger():
    """The library's ledger of device resources (tsd_debug_device_ledger) as {field: value}, the fields named as in
    tsd_device_ledger_field without the TSD_DL_ prefix: ALLOCS_LIVE, BYTES_LIVE, EVENTS_LIVE, STREAMS_LIVE, CTX_LIVE, MODELS_LIVE,
    SESSIONS_LIVE (what the whole process holds now) and ALLOCS_TOTAL, FREES_TOTAL, FREES_UNKNOWN, RELEASE_ERRORS (monotone).  Needs no GPU."""
    global _ledger_fields
    if _ledger_fields is None:
        f = header_enum("tsd_device_ledger_field", "TSD_DL_")
        n = f.pop("COUNT")
        assert sorted(f.values()) == list(range(n)), f
        _ledger_fields = f
    n = len(_ledger_fields)
    out = (C.c_int64 * n)()
    got = lib().tsd_debug_device_ledger(out, n)
    if got != n:
        raise TsdError(got if got < 0 else TSD_E_STATE, f"tsd_debug_device_ledger reports {got} fields, include/tsd.h names {n}")
    return {k: int(out[v]) for k, v in _ledger_fields.items()}


def last_error():
    return lib().tsd_last_error().decode()


def check(code, null_shape=None):
    """Map a status to the reference's behaviour.  Returns True when the caller should return a null matrix."""
    if code == TSD_OK:
        return False
    msg = last_error()
    if code == TSD_E_SHAPE and not _strict and null_shape is not None:
        print(msg + ". Returning null matrix")  # helpers/utils.mojo:1550-1552 convention
        return True
    raise TsdError(code, msg)


def latent_shape(L):
    """(LH, LW) of a latent size given as one side (an int: square) or as a pair (LH, LW) of positive ints.  ValueError for anything else;
    which multiples a side must be is the library's to say (TSD_E_SHAPE)."""
    import numbers
    if isinstance(L, numbers.Integral) and not isinstance(L, bool):
        return int(L), int(L)
    try:
        sides = tuple(L)
    except TypeError:
        sides = ()
    if len(sides) != 2 or any(not isinstance(v, numbers.Integral) or isinstance(v, bool) or v <= 0 for v in sides):
        raise ValueError(f"the latent size must be an int or a pair (LH, LW) of positive ints, got {L!r}")
    return int(sides[0]), int(sides[1])


def f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a


def ptr(a):
    return None if a is None else a.ctypes.data_as(fp)


NULL_MATRIX = lambda: np.zeros((0, 0, 0), dtype=np.float32)  # noqa: E731  `Matrix(0,0,0)`

_default_ctx = None


class Context:
    """One per GPU: device, HIP stream, workspace arena (`tsd_ctx`)."""

    def __init__(self, device=0):
        h = vp()
        check(lib().tsd_ctx_create(int(device), C.byref(h)))
        self.h = h
        self.device = device

    def synchronize(self):
        check(lib().tsd_ctx_synchronize(self.h))

    def timer_start(self):
        check(lib().tsd_ctx_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        check(lib().tsd_ctx_timer_stop(self.h, C.byref(ms)))
        return ms.value

    KERNEL_CLASSES = ("gemm", "conv3x3", "flash_attention", "groupnorm", "layernorm", "small_linear", "elementwise",
                      "softmax", "attn_tail_chain")

    def profile_begin(self):
        check(lib().tsd_ctx_profile_begin(self.h))

    def profile_end(self):
        """{class: (total_ms, launches)} measured with hipEvents on this context's stream."""
        nc = len(self.KERNEL_CLASSES)
        ms = (C.c_float * nc)()
        n = (C.c_int * nc)()
        check(lib().tsd_ctx_profile_end(self.h, ms, n, nc))
        return {k: (ms[i], n[i]) for i, k in enumerate(self.KERNEL_CLASSES)}

    def profile_records(self, cap=8192):
        """[(class, M, N, K, batch, ms)] per launch of the current profiling pass."""
        rec = (C.c_int * (5 * cap))()
        ms = (C.c_float * cap)()
        n = lib().tsd_ctx_profile_records(self.h, rec, ms, cap)
        if n < 0:
            check(n)
        return [(self.KERNEL_CLASSES[rec[5 * i]], rec[5 * i + 1], rec[5 * i + 2], rec[5 * i + 3], rec[5 * i + 4], ms[i])
                for i in range(n)]

    def scribble(self, byte):
        """Overwrite the whole workspace arena and the whole staging buffer with `byte` (tsd_debug_scribble; for tests: both are
        per-call scratch, so no result may change)."""
        check(lib().tsd_debug_scribble(self.h, int(byte)))

    def close(self):
        if self.h:
            lib().tsd_ctx_destroy(self.h)
            self.h = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(int(os.environ.get("LOCAL_RANK", "0")) if lib().tsd_device_count() > 1 else 0)
    return _default_ctx


def set_default_context(ctx):
    global _default_ctx
    _default_ctx = ctx
