"""ctypes binding of the C ABI in include/lbc_hip.h (learningbycheating_amd/liblbc_hip.so).

The product path has NO fallback: if the gfx950 library is missing or a kernel launch
fails, a RuntimeError is raised.  (tests/emu injects a CPU-emulated build of the same
kernel sources through _inject_for_tests(); nothing in the package does.)
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblbc_hip.so")
_lib = None

c_void_p, c_int, c_float, c_size_t, c_char_p = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_char_p


ABI_VERSION = 201    # include/lbc_hip.h LBC_HIP_ABI_VERSION: load() refuses a library that answers anything else


class ConvDesc(ctypes.Structure):
    """lbc_conv_desc; struct_size (its first member, checked by every entry point) is filled in here: ConvDesc(N, H, W, C, K, ...)"""
    _fields_ = ([("struct_size", ctypes.c_uint)] +
                [(n, c_int) for n in ("N", "H", "W", "C", "K", "KH", "KW", "S", "P", "relu", "bf16", "w_transposed")] +
                [("split_workspace", c_void_p), ("split_workspace_bytes", c_size_t)])

    def __init__(self, *args, **kw):
        super().__init__(ctypes.sizeof(ConvDesc), *args, **kw)


class NetDesc(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("arch", "in_channels", "H", "W", "normalize", "max_batch", "precision")]


class Camera(ctypes.Structure):
    _fields_ = [(n, c_float) for n in ("w", "h", "fov", "world_y", "fixed_offset", "pixels_per_meter", "crop_size")]


class HeadDesc(ctypes.Structure):
    _fields_ = ([("h", c_void_p), ("N", c_int), ("OH", c_int), ("OW", c_int), ("act_bf16", c_int)] +
                [(n, c_void_p * 4) for n in ("mean", "invstd", "gamma", "beta", "w", "bias", "pos_x", "pos_y")] + [("cmd", c_void_p)])


class AugParams(ctypes.Structure):
    _fields_ = [("order", c_int * 8), ("n_ops", c_int), ("blur_pos", c_int), ("seed", ctypes.c_uint), ("blur_sigma", c_float),
                ("noise_scale", c_float), ("noise_pc", c_int), ("coarse_p", c_float), ("coarse_h", c_int), ("coarse_w", c_int),
                ("coarse_pc", c_int), ("dropout_p", c_float), ("dropout_pc", c_int), ("add", c_float * 3), ("multiply", c_float * 3),
                ("contrast", c_float * 3)]


class AdamChunk(ctypes.Structure):
    _fields_ = [("p", c_void_p), ("g", c_void_p), ("m", c_void_p), ("v", c_void_p), ("n", c_int), ("pad", c_int)]


class AdamState(ctypes.Structure):
    """lbc_adam_state: the device record of the guarded step (counters are 64-bit)"""
    _fields_ = [("step", ctypes.c_longlong), ("skipped_total", ctypes.c_longlong), ("skipped_in_a_row", ctypes.c_longlong),
                ("bad", c_int), ("scan_flag", c_int), ("lr_over_bc1", c_float), ("inv_bc2_sqrt", c_float)]


class AdamClipState(ctypes.Structure):
    """lbc_adam_clip_state: the header of the clipped step's device record (lbc_adam_state's fields, then norm / coefficient / count);
    lbc_adam_clip_state_bytes(nchunks) - sizeof(this) bytes of per-chunk partial sums follow it on the device"""
    _fields_ = AdamState._fields_ + [("grad_norm", ctypes.c_double), ("clip_coef", c_float), ("reserved", c_int),
                                     ("clipped_total", ctypes.c_longlong)]


class AdamRecipeState(ctypes.Structure):
    """lbc_adam_recipe_state: the header of the recipe step's device record (lbc_adam_clip_state's 64 bytes, then the schedule's rate, the
    decoupled decay factor and the number of moving-average updates); one double per chunk follows it on the device"""
    _fields_ = AdamClipState._fields_ + [("lr", ctypes.c_double), ("decay_factor", c_float), ("reserved2", c_int),
                                         ("ema_updates", ctypes.c_longlong)]


LR_SCHEDULES = {"constant": 0, "cosine": 1, "step": 2}      # LBC_LR_*


class AdamRecipe(ctypes.Structure):
    """lbc_adam_recipe (a host struct, read during the call); struct_size is filled in here and the defaults are LBC_ADAM_RECIPE_INIT's"""
    _fields_ = [("struct_size", ctypes.c_uint), ("schedule", c_int), ("base_lr", ctypes.c_double), ("warmup_steps", ctypes.c_longlong),
                ("warmup_start", ctypes.c_double), ("total_steps", ctypes.c_longlong), ("min_lr", ctypes.c_double),
                ("step_size", ctypes.c_longlong), ("gamma", ctypes.c_double), ("weight_decay", ctypes.c_double), ("decoupled", c_int),
                ("reserved", c_int), ("max_norm", ctypes.c_double), ("ema_decay", ctypes.c_double), ("beta1", ctypes.c_double),
                ("beta2", ctypes.c_double), ("eps", ctypes.c_double)]

    def __init__(self, **kw):
        d = dict(struct_size=ctypes.sizeof(AdamRecipe), step_size=1, gamma=1.0, beta1=0.9, beta2=0.999, eps=1e-8)
        d.update(kw)
        super().__init__(**d)


class WaypointMetricsDesc(ctypes.Structure):
    """lbc_waypoint_metrics_desc (a host struct, read during the call); struct_size is filled in here"""
    _fields_ = [("struct_size", ctypes.c_uint), ("pred_frame", c_int), ("rows", c_int), ("nthresholds", c_int),
                ("target_scale", ctypes.c_double), ("target_shift", ctypes.c_double), ("thresholds_m", ctypes.c_double * 4),
                ("camera", Camera), ("reserved", c_int)]

    def __init__(self, **kw):
        d = dict(struct_size=ctypes.sizeof(WaypointMetricsDesc), rows=5, target_scale=1.0)
        d.update(kw)
        super().__init__(**d)


class WaypointMetricsState(ctypes.Structure):
    """lbc_waypoint_metrics_state: the device record of the waypoint metrics, 248 fields of 8 bytes"""
    _fields_ = [("samples", ctypes.c_longlong), ("updates", ctypes.c_longlong), ("cmd_count", ctypes.c_longlong * 4),
                ("sum_e", ctypes.c_double * 5 * 4), ("sum_e2", ctypes.c_double * 5 * 4), ("sum_abs_dx", ctypes.c_double * 5 * 4),
                ("sum_abs_dy", ctypes.c_double * 5 * 4), ("max_e", ctypes.c_double * 5 * 4), ("bad", ctypes.c_longlong * 5 * 4),
                ("within", ctypes.c_longlong * 5 * 4 * 4), ("all_sum_e", ctypes.c_double * 5 * 4), ("all_bad", ctypes.c_longlong * 5 * 4),
                ("loss_sum", ctypes.c_double), ("loss_bad", ctypes.c_longlong)]


class VisualsDesc(ctypes.Structure):
    """lbc_visuals_desc (a host struct, read during the call); struct_size is filled in here and the defaults are LBC_VISUALS_DESC_INIT's"""
    _fields_ = ([("struct_size", ctypes.c_uint), ("camera", Camera)] +
                [(n, c_int) for n in ("mode", "size", "sort", "ncols", "N", "H", "W", "BH", "BW", "rgb_f32", "birdview_f32")])

    def __init__(self, **kw):
        d = dict(struct_size=ctypes.sizeof(VisualsDesc), size=8, ncols=4)
        d.update(kw)
        super().__init__(**d)


class AgentDesc(ctypes.Structure):
    """lbc_agent_desc (a host struct, read during the call); struct_size is filled in here, everything else by agent.ControllerConfig"""
    _fields_ = ([("struct_size", ctypes.c_uint), ("kind", c_int), ("n_steps", c_int), ("speed_steps", c_int)] +
                [(n, ctypes.c_double) for n in ("w", "h", "fov", "world_y", "fixed_offset", "crop_size", "pixels_per_meter", "gap", "dt")] +
                [("steer_points", c_int * 4), ("turn_pid", ctypes.c_double * 3 * 4), ("speed_pid", ctypes.c_double * 3),
                 ("turn_window", c_int), ("speed_window", c_int)] +
                [(n, ctypes.c_double) for n in ("engine_brake_threshold", "brake_threshold", "stop_threshold")])

    def __init__(self, **kw):
        d = dict(struct_size=ctypes.sizeof(AgentDesc))
        d.update(kw)
        super().__init__(**d)


class AgentState(ctypes.Structure):
    """lbc_agent_state: one agent's two PID windows in device memory, 336 bytes; all-zero bytes = a fresh agent"""
    _fields_ = [("turn_ring", ctypes.c_double * 10), ("speed_ring", ctypes.c_double * 30), ("turn_count", c_int), ("turn_head", c_int),
                ("speed_count", c_int), ("speed_head", c_int)]


_SIGNATURES = {
    "lbc_last_error": (c_char_p, []),
    "lbc_backend": (c_char_p, []),
    "lbc_version": (c_int, []),
    "lbc_conv2d_fwd": (c_int, [ctypes.POINTER(ConvDesc)] + [c_void_p] * 6 + [c_int, c_void_p, c_void_p, ctypes.POINTER(c_int), c_void_p]),
    "lbc_conv2d_dgrad": (c_int, [ctypes.POINTER(ConvDesc)] + [c_void_p] * 5),
    "lbc_weight_transpose_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "lbc_conv2d_wgrad_workspace": (c_size_t, [ctypes.POINTER(ConvDesc)]),
    "lbc_conv2d_wgrad": (c_int, [ctypes.POINTER(ConvDesc)] + [c_void_p] * 4 + [c_int, c_void_p, c_float, c_void_p, c_void_p]),
    "lbc_deconv3x3s2_fwd": (c_int, [ctypes.POINTER(ConvDesc)] + [c_void_p] * 5 + [c_int, c_void_p, c_void_p, ctypes.POINTER(c_int), c_void_p]),
    "lbc_deconv3x3s2_dgrad": (c_int, [ctypes.POINTER(ConvDesc)] + [c_void_p] * 4),
    "lbc_conv2d_wgrad_group_supported": (c_int, [ctypes.POINTER(ConvDesc)]),
    "lbc_conv2d_wgrad_group_workspace": (c_size_t, [ctypes.POINTER(ConvDesc), c_int]),
    "lbc_conv2d_wgrad_group": (c_int, [ctypes.POINTER(ConvDesc), c_int] + [c_void_p] * 4 + [c_int, c_void_p, c_void_p, c_void_p]),
    "lbc_deconv3x3s2_wgrad_workspace": (c_size_t, [ctypes.POINTER(ConvDesc)]),
    "lbc_deconv3x3s2_wgrad": (c_int, [ctypes.POINTER(ConvDesc)] + [c_void_p] * 4 + [c_int, c_void_p, c_float, c_void_p, c_void_p]),
    "lbc_net_create": (c_int, [ctypes.POINTER(NetDesc), ctypes.POINTER(c_void_p)]),
    "lbc_net_destroy": (None, [c_void_p]),
    "lbc_net_num_tensors": (c_int, [c_void_p]),
    "lbc_net_tensor_info": (c_int, [c_void_p, c_int, c_char_p, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "lbc_net_workspace_bytes": (c_size_t, [c_void_p]),
    "lbc_net_num_activations": (c_int, [c_void_p]),
    "lbc_net_activation_info": (c_int, [c_void_p, c_int, c_char_p, c_int, ctypes.POINTER(c_size_t), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "lbc_net_bind": (c_int, [c_void_p, c_void_p, ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p)]),
    "lbc_net_forward": (c_int, [c_void_p, c_int, c_int] + [c_void_p] * 6),
    "lbc_net_forward_u8": (c_int, [c_void_p, c_int, c_int] + [c_void_p] * 6),
    "lbc_net_num_stages": (c_int, []),
    "lbc_net_last_forward": (c_int, [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_longlong)]),
    "lbc_net_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "lbc_net_set_frozen": (c_int, [c_void_p, c_int]),
    "lbc_net_set_sync_bn": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int]),
    "lbc_comm_unique_id": (c_int, [c_void_p]),
    "lbc_comm_create": (c_int, [c_void_p, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "lbc_comm_destroy": (None, [c_void_p]),
    "lbc_comm_world_size": (c_int, [c_void_p]),
    "lbc_comm_allreduce_f32": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "lbc_loss": (c_int, [c_int, ctypes.POINTER(Camera), c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    "lbc_phase2_weight": (c_int, [ctypes.POINTER(Camera), c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "lbc_adam_step": (c_int, [c_void_p, c_int] + [ctypes.c_double] * 5 + [c_int, c_void_p]),
    "lbc_adam_state_bytes": (c_size_t, []),
    "lbc_adam_step_guarded": (c_int, [c_void_p, c_int] + [ctypes.c_double] * 5 + [c_void_p, c_void_p]),
    "lbc_adam_clip_state_bytes": (c_size_t, [c_int]),
    "lbc_adam_step_clipped": (c_int, [c_void_p, c_int] + [ctypes.c_double] * 6 + [c_void_p, c_void_p]),
    "lbc_adam_recipe_state_bytes": (c_size_t, [c_int]),
    "lbc_adam_step_recipe": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lbc_grad_accumulate": (c_int, [c_void_p, c_void_p, ctypes.c_longlong, c_int, c_void_p]),
    "lbc_waypoint_metrics_state_bytes": (c_size_t, []),
    "lbc_waypoint_metrics_update": (c_int, [ctypes.POINTER(WaypointMetricsDesc)] + [c_void_p] * 4 + [c_int, c_void_p, c_void_p]),
    "lbc_visuals_image_shape": (c_int, [ctypes.POINTER(VisualsDesc), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "lbc_visuals_render": (c_int, [ctypes.POINTER(VisualsDesc)] + [c_void_p] * 9),
    "lbc_agent_state_bytes": (c_size_t, [c_int]),
    "lbc_agent_control": (c_int, [ctypes.POINTER(AgentDesc)] + [c_void_p] * 4 + [c_int, c_void_p, c_void_p, c_void_p]),
    "lbc_agent_reset": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "lbc_bn_stats": (c_int, [c_void_p, ctypes.c_longlong, c_int, c_int, c_void_p, ctypes.POINTER(c_int), c_void_p]),
    "lbc_bn_finalize_stats": (c_int, [c_void_p, c_int, c_int, ctypes.c_longlong] + [c_void_p] * 5 + [c_float, c_float, c_int] + [c_void_p] * 5),
    "lbc_bn_apply_relu_add_fwd": (c_int, [c_void_p, c_void_p, ctypes.c_longlong, c_int] + [c_void_p] * 5 + [c_int, c_int, c_void_p]),
    "lbc_bn_bwd_workspace": (c_size_t, [c_int]),
    "lbc_bn_bwd": (c_int, [c_void_p] * 9 + [ctypes.c_longlong, c_int, c_int] + [c_void_p] * 4 + [c_int, c_void_p]),
    "lbc_maxpool3x3s2_fwd": (c_int, [c_void_p] * 5 + [c_int] * 5 + [c_void_p]),
    "lbc_maxpool3x3s2_bwd": (c_int, [c_void_p] * 9 + [ctypes.POINTER(c_int)] + [c_int] * 5 + [c_void_p]),
    "lbc_head_workspace": (c_size_t, [c_int]),
    "lbc_head_fwd": (c_int, [ctypes.POINTER(HeadDesc)] + [c_void_p] * 4),
    "lbc_head_bwd": (c_int, [ctypes.POINTER(HeadDesc)] + [c_void_p] * 4 + [ctypes.POINTER(c_void_p)] * 4 + [c_void_p, c_void_p]),
    "lbc_nchw_to_input": (c_int, [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p]),
    "lbc_u8nhwc_to_input": (c_int, [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p]),
    "lbc_stem_fwd": (c_int, [c_void_p] * 4 + [ctypes.POINTER(c_int)] + [c_int] * 5 + [c_void_p]),
    "lbc_stem_wgrad_workspace": (c_size_t, [c_int] * 4),
    "lbc_stem_wgrad": (c_int, [c_void_p] * 4 + [c_int] * 5 + [c_void_p]),
    "lbc_birdview_crop_u8": (c_int, [c_void_p, c_void_p] + [c_int] * 8 + [c_void_p]),
    "lbc_birdview_warp_crop_u8": (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 6 + [c_void_p]),
    "lbc_augment_rgb_u8": (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 4 + [c_void_p]),
    "lbc_replay_cdf": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "lbc_replay_sample": (c_int, [c_void_p, c_int, ctypes.c_uint, ctypes.c_ulonglong, c_int, c_void_p, c_void_p]),
    "lbc_replay_gather_u8": (c_int, [c_void_p, ctypes.c_longlong, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "lbc_replay_gather_indirect_u8": (c_int, [c_void_p, ctypes.c_longlong, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "lbc_replay_admit_workspace": (c_size_t, [c_int, c_int]),
    "lbc_replay_admit": (c_int, [c_void_p] * 5 + [c_int] * 3 + [c_void_p] * 4 + [c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    "lbc_replay_scatter_u8": (c_int, [c_void_p, ctypes.c_longlong, c_void_p, c_int, c_void_p, c_void_p]),
    "lbc_replay_meta": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "lbc_replay_writeback": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "lbc_rollout_decide": (c_int, [c_void_p] * 6 + [c_int, c_int, ctypes.c_uint] + [c_void_p] * 10),
    "lbc_rollout_stage_u8": (c_int, [c_void_p, ctypes.c_longlong, c_void_p, ctypes.c_longlong, c_void_p, c_int, ctypes.c_longlong] + [c_void_p] * 3),
    "lbc_dataset_gather_crop_u8": (c_int, [c_void_p, c_void_p] + [c_int] * 9 + [c_void_p, c_void_p]),
    "lbc_dataset_gather_warp_crop_u8": (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 8 + [c_void_p, c_void_p]),
    "lbc_dataset_targets": (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 6 + [c_void_p, c_void_p, c_void_p]),
    "lbc_dataset_gather_rows_f32": (c_int, [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p, c_void_p]),
    "lbc_config_set": (c_int, [c_char_p, ctypes.c_longlong]),
    "lbc_config_get": (ctypes.c_longlong, [c_char_p]),
    "lbc_profile_enable": (c_int, [c_int]),
    "lbc_profile_report": (c_int, [c_char_p, c_int]),
    "lbc_adam_profile_elems": (None, [ctypes.c_longlong]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def _declare(lib):
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError here = the library does not export what include/lbc_hip.h declares
        fn.restype = res
        fn.argtypes = args
    v = lib.lbc_version()
    if v != ABI_VERSION:
        raise RuntimeError("learningbycheating_amd: the library answers ABI version %d, this binding was written for %d "
                           "(include/lbc_hip.h LBC_HIP_ABI_VERSION): rebuild liblbc_hip.so" % (v, ABI_VERSION))
    return lib


def load(path=None):
    """Load the gfx950 library (built by __graft_entry__.build() / csrc/Makefile)."""
    global _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(
            "learningbycheating_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % path)
    _lib = _declare(ctypes.CDLL(path))
    return _lib


def get():
    return _lib if _lib is not None else load()


def _inject_for_tests(lib):
    """tests/emu only: use a CPU-emulated build of the kernel sources."""
    global _lib
    _lib = _declare(lib) if lib is not None else None
    return _lib


def config_set(name, value):
    """runtime option of the library (names = the LBC_* environment variables); value -1 = unset"""
    check(get().lbc_config_set(name.encode(), int(value)), "config_set")


def config_get(name):
    return int(get().lbc_config_get(name.encode()))


def backend():
    return get().lbc_backend().decode()


def check(rc, what=""):
    if rc != 0:
        raise RuntimeError("lbc_hip %s failed (%d): %s" % (what, rc, get().lbc_last_error().decode()))


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_for(t):
    import torch
    if t.is_cuda:
        return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    return None


def require_device(t):
    """Kernels run on a ROCm device only (the emulated test build accepts CPU tensors)."""
    if not t.is_cuda and backend() != "emu-cpu":
        raise RuntimeError("learningbycheating_amd: tensors must live on a ROCm (cuda) device; there is no CPU path")
