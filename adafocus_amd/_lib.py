"""ctypes binding of include/adafocus.h.

PyTorch is plumbing here: it owns device memory and streams; every compute call goes through
the C ABI with raw ``data_ptr()`` values and the current HIP stream.  There is NO fallback: if
``libadafocus_hip.so`` is missing or the device is not a gfx950 part, calls raise.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# (ADAF_LIB points at another build of the same library: A/B runs of two kernel versions on one box)
LIB_PATH = os.environ.get("ADAF_LIB") or os.path.join(_HERE, "csrc", "libadafocus_hip.so")

LAYOUT_NCHW, LAYOUT_NHWC, LAYOUT_NHWC4 = 0, 1, 2
ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SIGMOID, ACT_SWISH = 0, 1, 2, 3, 4
MATH_F32, MATH_F32_SPLIT_BF16, MATH_F16 = 0, 1, 2
DTYPE_F32, DTYPE_F16 = 0, 1
STEM_FORM_AUTO, STEM_FORM_TILE4, STEM_FORM_TILE6, STEM_FORM_STRIP, STEM_FORM_UNFUSED = range(5)
CONV_TILES = 4


class ConvParams(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n", "h", "w", "cin", "cout", "kh", "kw", "stride", "pad", "act",
                                       "tsm_segments", "tsm_div", "ldx", "ldo", "ldr", "tile")]


vp, ip, fp, sz, cp = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_char_p
# Every symbol include/adafocus.h declares, once: name -> (restype, argtypes).  load_library() applies the table; the tests hold it to
# the header parameter by parameter and to the library's exports.  (Symbols of experiment builds are declared by the tools that use them.)
PROTOTYPES = {
    "adaf_version": (ip, []),
    "adaf_last_error": (cp, [vp]),
    "adaf_create": (ip, [ip, C.POINTER(vp)]),
    "adaf_destroy": (ip, [vp]),
    "adaf_device_cus": (ip, [vp]),
    "adaf_set_gru_persistent": (ip, [vp, ip]),
    "adaf_set_conv_pos_major": (ip, [vp, ip]),
    "adaf_gru_scan_timeouts": (ip, [vp, C.POINTER(C.c_uint)]),
    "adaf_set_global_option": (ip, [cp, C.c_double]),
    "adaf_get_global_option": (C.c_double, [cp]),
    "adaf_crop_gather_f32": (ip, [vp, vp, ip, ip, ip, ip, vp, ip, ip, ip, vp, ip, vp, vp]),
    "adaf_conv2d_bn_act_f32": (ip, [vp, C.POINTER(ConvParams), vp, vp, vp, vp, vp, vp, vp]),
    "adaf_conv2d_naive_f32": (ip, [vp, C.POINTER(ConvParams), vp, vp, vp, vp, vp, vp, vp]),
    "adaf_pack_conv_weight_f32": (ip, [vp, vp, ip, ip, ip, ip, ip, vp, vp]),
    "adaf_fold_bn_f32": (ip, [vp, vp, vp, vp, vp, fp, ip, vp, vp, vp]),
    "adaf_maxpool3x3s2_f32": (ip, [vp, vp, ip, ip, ip, ip, vp, vp]),
    "adaf_global_avgpool_f32": (ip, [vp, vp, ip, ip, ip, vp, ip, vp]),
    "adaf_temporal_shift_f32": (ip, [vp, vp, ip, ip, ip, ip, ip, ip, vp, vp]),
    "adaf_resnet50_create": (ip, [vp, C.POINTER(vp)]),
    "adaf_resnet50_destroy": (ip, [vp]),
    "adaf_resnet50_set_param": (ip, [vp, cp, vp, sz]),
    "adaf_resnet50_finalize": (ip, [vp, vp]),
    "adaf_resnet50_workspace_bytes": (sz, [vp, ip, ip]),
    "adaf_resnet50_forward": (ip, [vp, vp, ip, ip, ip, ip, vp, ip, vp, sz, vp]),
    "adaf_resnet50_forward_frames": (ip, [vp, vp, ip, ip, ip, ip, vp, ip, ip, ip, ip, ip, vp, ip, vp, sz, vp]),
    "adaf_resnet50_map_size": (ip, [ip]),
    "adaf_resnet50_forward_map": (ip, [vp, vp, ip, ip, ip, ip, vp, vp, ip, vp, sz, vp]),
    "adaf_resnet50_launch_count": (ip, [vp]),
    "adaf_resnet50_forward_profiled": (ip, [vp, vp, ip, ip, ip, ip, vp, ip, vp, sz, vp, vp, vp, vp, vp]),
    "adaf_resnet50_set_tiles": (ip, [vp, vp, ip]),
    "adaf_resnet50_set_math": (ip, [vp, ip]),
    "adaf_resnet50_set_fusion": (ip, [vp, ip]),
    "adaf_resnet50_set_latency_rows": (ip, [vp, ip]),
    "adaf_resnet50_set_shift_place": (ip, [vp, ip]),
    "adaf_gru_cls_workspace_bytes": (sz, [ip, ip, ip]),
    "adaf_gru_cls_forward_f32": (ip, [vp, vp, ip, ip, ip, ip, ip, ip, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    "adaf_fc_meanpool_forward_f32": (ip, [vp, vp, ip, ip, ip, ip, vp, vp, vp, ip, vp, vp, sz, vp]),
    "adaf_copy2d_f32": (ip, [vp, vp, ip, vp, ip, ip, ip, vp]),
    "adaf_pack_dw_weight_f32": (ip, [vp, vp, ip, vp, vp]),
    "adaf_dwconv3x3_bn_act_f32": (ip, [vp, vp, ip, ip, ip, ip, ip, vp, vp, vp, ip, vp, vp]),
    "adaf_mobilenetv2_create": (ip, [vp, C.POINTER(vp)]),
    "adaf_mobilenetv2_destroy": (ip, [vp]),
    "adaf_mobilenetv2_set_param": (ip, [vp, cp, vp, sz]),
    "adaf_mobilenetv2_finalize": (ip, [vp, vp]),
    "adaf_mobilenetv2_workspace_bytes": (sz, [vp, ip, ip, ip]),
    "adaf_mobilenetv2_forward": (ip, [vp, vp, ip, ip, ip, ip, vp, vp, ip, vp, sz, vp]),
    "adaf_mobilenetv2_set_fusion": (ip, [vp, ip]),
    "adaf_mobilenetv2_block_forms": (ip, [vp, ip, ip, ip, C.POINTER(ip), ip]),
    "adaf_grid_actions_f32": (ip, [vp, vp, ip, ip, vp, vp, vp, vp]),
    "adaf_gru_seq_forward_f32": (ip, [vp, vp, ip, ip, ip, ip, ip, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    "adaf_gru_cls_train_workspace_bytes": (sz, [ip, ip, ip]),
    "adaf_gru_cls_train_forward_f32": (ip, [vp, vp, ip, ip, ip, ip, ip, ip] + [vp] * 12 + [sz, vp]),
    "adaf_gru_cls_backward_workspace_bytes": (sz, [ip, ip, ip, ip]),
    "adaf_gru_cls_backward_f32": (ip, [vp, vp, ip, ip, ip, ip, ip, ip] + [vp] * 16 + [sz, vp]),
    "adaf_ppo_sample_f32": (ip, [vp, vp, ip, ip, ip, vp, vp, vp, vp, vp]),
    "adaf_ppo_sample_actions_f32": (ip, [vp, vp, ip, ip, ip, ip, vp, vp, vp, vp, vp, vp]),
    "adaf_ppo_rewards_f32": (ip, [vp, vp, vp, vp, ip, ip, ip, ip, vp, vp, vp, vp]),
    "adaf_ce_steps_workspace_bytes": (sz, [ip, ip]),
    "adaf_ce_steps_f32": (ip, [vp, vp, vp, ip, ip, ip, vp, vp, vp, sz, vp]),
    "adaf_ppo_returns_f32": (ip, [vp, vp, ip, ip, fp, vp, vp]),
    "adaf_ppo_head_workspace_bytes": (sz, [ip, ip]),
    "adaf_ppo_head_f32": (ip, [vp, vp, ip, ip, ip, ip, vp, vp, vp, fp] + [vp] * 9 + [sz, vp]),
    "adaf_ppo_rows_transpose_f32": (ip, [vp, vp, ip, ip, ip, vp, vp]),
    "adaf_ppo_wenc_grad_workspace_bytes": (sz, [ip, ip, ip]),
    "adaf_ppo_wenc_grad_f32": (ip, [vp, vp, vp, vp, ip, ip, ip, ip, vp, vp, sz, vp]),
    "adaf_ppo_encoder_backward_workspace_bytes": (sz, [ip, ip, ip, ip, ip, ip]),
    "adaf_ppo_encoder_backward_f32": (ip, [vp, vp, vp, vp, vp, ip, ip, ip, ip, ip, ip, vp, vp, vp, vp, vp, sz, vp]),
    "adaf_ppo_gauss_sample_f32": (ip, [vp, vp, vp, ip, fp, vp, vp, vp]),
    "adaf_ppo_gauss_head_f32": (ip, [vp, vp, ip, ip, ip, vp, fp, vp, vp, fp] + [vp] * 8 + [sz, vp]),
    "adaf_bn_train_workspace_bytes": (sz, [ip, ip]),
    "adaf_bn_train_forward_f32": (ip, [vp, vp, ip, ip, vp, vp, fp, fp, vp, vp, ip, vp, vp, vp, vp, sz, vp]),
    "adaf_bn_train_backward_f32": (ip, [vp, vp, vp, vp, ip, ip] + [vp] * 7 + [sz, vp]),
    "adaf_bn_map_workspace_bytes": (sz, [ip, ip]),
    "adaf_bn_map_train_forward_f32": (ip, [vp, vp, ip, ip, vp, vp, fp, fp, vp, vp, vp, ip, vp, vp, vp, vp, sz, vp]),
    "adaf_bn_map_train_backward_f32": (ip, [vp, vp, vp, vp, ip, ip] + [vp] * 7 + [sz, vp]),
    "adaf_ppo_encoder_bn_backward_workspace_bytes": (sz, [ip] * 7),
    "adaf_ppo_encoder_bn_backward_f32": (ip, [vp] * 5 + [ip] * 6 + [vp] * 17 + [sz, vp]),
    "adaf_crop_gather_nhwc4_f32": (ip, [vp, vp, ip, ip, ip, vp, ip, ip, ip, vp, vp, vp]),
    "adaf_ingest_u8_f32": (ip, [vp, vp, ip, ip, ip, ip, C.POINTER(fp), C.POINTER(fp), vp, vp]),
    "adaf_crop_resize_f32": (ip, [vp, vp, ip, ip, ip, ip, ip, vp, ip, ip, vp, ip, ip, vp, ip, vp, vp]),
    "adaf_resize_nearest_f32": (ip, [vp, vp, ip, ip, ip, ip, ip, ip, ip, vp, ip, vp]),
    "adaf_conv2d_bn_act_f16": (ip, [vp, C.POINTER(ConvParams), vp, ip, vp, vp, vp, vp, vp, ip, vp]),
    "adaf_pack_conv_weight_f16": (ip, [vp, vp, ip, ip, ip, ip, ip, vp, vp]),
    "adaf_cast_f32_f16": (ip, [vp, vp, sz, vp, ip, vp]),
    "adaf_dwconv3x3_bn_act_f16": (ip, [vp, vp, ip, ip, ip, ip, ip, vp, vp, vp, ip, vp, vp]),
    "adaf_pack_dw_weight_kxk_f32": (ip, [vp, vp, ip, ip, vp, vp]),
    "adaf_dwconv_same_workspace_bytes": (sz, [ip, ip, ip, ip, ip, ip, ip]),
    "adaf_dwconv_same_bn_act": (ip, [vp, vp, ip, ip, ip, ip, ip, ip, ip, vp, vp, vp, ip, vp, vp, vp, sz, vp]),
    "adaf_se_gate_f32": (ip, [vp, vp, ip, ip, vp, vp, ip, vp, vp, vp, vp]),
    "adaf_conv1x1_gated_bn": (ip, [vp, vp, ip, ip, ip, ip, vp, vp, ip, vp, vp, vp, vp, vp]),
    "adaf_effnet_create": (ip, [vp, fp, fp, C.POINTER(vp)]),
    "adaf_effnet_destroy": (ip, [vp]),
    "adaf_effnet_feature_dim": (ip, [vp]),
    "adaf_effnet_block_count": (ip, [vp]),
    "adaf_effnet_block_info": (ip, [vp, ip, C.POINTER(ip)]),
    "adaf_effnet_set_dtype": (ip, [vp, ip]),
    "adaf_effnet_set_fusion": (ip, [vp, ip]),
    "adaf_effnet_whole_blocks": (ip, [vp, ip, ip]),
    "adaf_effnet_fused_expand_blocks": (ip, [vp, ip, ip]),
    "adaf_effnet_set_param": (ip, [vp, cp, vp, sz]),
    "adaf_effnet_finalize": (ip, [vp, vp]),
    "adaf_effnet_workspace_bytes": (sz, [vp, ip, ip, ip]),
    "adaf_effnet_forward": (ip, [vp, vp, ip, ip, ip, ip, vp, vp, vp, ip, vp, sz, vp]),
    "adaf_stem7x7_workspace_bytes": (sz, []),
    "adaf_stem7x7_bn_relu_f32": (ip, [vp, vp, ip, ip, vp, vp, vp, vp, vp, sz, vp]),
    "adaf_stem7x7_pool_form": (ip, [vp, ip, ip]),
    "adaf_stem7x7_pool": (ip, [vp, vp, ip, ip, vp, vp, vp, ip, ip, vp, vp, C.POINTER(ip), vp, sz, vp]),
    "adaf_stem7x7_pool_frames": (ip, [vp, vp, ip, ip, ip, ip, vp, ip, ip, ip, vp, vp, vp, ip, vp, vp, sz, vp]),
    "adaf_maxpool3x3s2_f16out": (ip, [vp, vp, ip, ip, ip, ip, vp, vp]),
    "adaf_conv2d_wgrad_workspace_bytes": (sz, [C.POINTER(ConvParams)]),
    "adaf_conv2d_wgrad_f32": (ip, [vp, C.POINTER(ConvParams), vp, vp, vp, vp, sz, vp]),
    "adaf_pack_conv_dgrad_weight_f32": (ip, [vp, vp, vp, ip, ip, ip, ip, vp, vp]),
    "adaf_conv2d_dgrad_workspace_bytes": (sz, [C.POINTER(ConvParams)]),
    "adaf_conv2d_dgrad_f32": (ip, [vp, C.POINTER(ConvParams), vp, vp, vp, vp, sz, vp]),
    "adaf_relu_backward_f32": (ip, [vp, vp, vp, vp, sz, vp, vp]),
    "adaf_global_avgpool_backward_f32": (ip, [vp, vp, ip, vp, ip, ip, ip, vp, vp]),
    "adaf_maxpool3x3s2_backward_f32": (ip, [vp, vp, vp, ip, ip, ip, ip, vp, vp]),
    "adaf_temporal_shift_backward_f32": (ip, [vp, vp, ip, ip, ip, ip, ip, ip, vp, vp]),
    "adaf_conv_bn_param_grad_workspace_bytes": (sz, [ip]),
    "adaf_conv_bn_param_grad_f32": (ip, [vp, vp, ip, vp, vp, vp, vp, vp, fp, ip, ip, ip, ip, ip, vp, vp, vp, vp, sz, vp]),
    "adaf_dwconv3x3_dgrad_f32": (ip, [vp, vp, ip, ip, ip, ip, ip, vp, vp, vp]),
    "adaf_dwconv3x3_wgrad_workspace_bytes": (sz, [ip] * 5),
    "adaf_dwconv3x3_wgrad_f32": (ip, [vp, vp, vp, ip, ip, ip, ip, ip, vp, vp, sz, vp]),
    "adaf_bn_map_train_forward_act_f32": (ip, [vp, vp, ip, ip, vp, vp, fp, fp, vp, vp, vp, ip, vp, vp, vp, vp, sz, vp]),
    "adaf_bn_map_train_backward_act_f32": (ip, [vp, vp, vp, ip, vp, ip, ip] + [vp] * 7 + [sz, vp]),
    "adaf_add_f32": (ip, [vp, vp, vp, sz, vp, vp]),
    "adaf_conv2d_wgrad_rows_workspace_bytes": (sz, [C.POINTER(ConvParams)]),
    "adaf_conv2d_wgrad_rows_f32": (ip, [vp, C.POINTER(ConvParams), vp, vp, vp, vp, sz, vp]),
}
SYMBOLS = tuple(PROTOTYPES)


class AdafError(RuntimeError):
    pass


_lib = None


def load_library():
    """dlopen the in-tree shared library; raises (loudly) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AdafError("HIP extension not built: %s is missing (run `python -c 'import __graft_entry__ as g; "
                        "g.build()'` or `make -C adafocus_amd/csrc`)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


_handles = {}


def handle(device):
    """One library handle per device per process."""
    idx = torch.device(device).index
    if idx is None:
        idx = torch.cuda.current_device()
    if idx not in _handles:
        lib = load_library()
        h = C.c_void_p()
        rc = lib.adaf_create(idx, C.byref(h))
        if rc != 0:
            raise AdafError("adaf_create(device=%d) failed with %d: no gfx950 (MI355X) device -- this package "
                            "has no CPU or non-gfx950 path" % (idx, rc))
        _handles[idx] = h
    return _handles[idx]


EF_PLAN_WHOLE_BLOCK, EF_PLAN_TINY_DW, EF_PLAN_STRIP_PROJECT, EF_PLAN_STRIP_EXPAND, EF_PLAN_OWN_STEM, EF_PLAN_FUSED_EXPAND, EF_PLAN_PACKED_STEM, EF_PLAN_HEAD_POOL, EF_PLAN_PAIR_CHUNKS = 1, 2, 4, 8, 16, 32, 64, 128, 256


def get_option(key):
    """Current value of a process-wide tuning / A-B switch of the library (include/adafocus.h: adaf_get_global_option)."""
    v = load_library().adaf_get_global_option(key.encode())
    if v != v:
        raise AdafError("adaf_get_global_option: unknown key %r" % key)
    return v


def set_option(key, value, device=None):
    """Set a process-wide switch (include/adafocus.h: adaf_set_global_option -- global state of the library, no handle); returns the
    previous value."""
    old = get_option(key)
    if load_library().adaf_set_global_option(key.encode(), float(value)) != 0:
        raise AdafError("adaf_set_global_option: %s = %r is out of range" % (key, value))
    return old


class option:
    """with _lib.option("conv_pool", 0): ...  -- a switch flipped for the duration of a block (tests, A/B tools)."""

    def __init__(self, key, value):
        self.key, self.value, self.old = key, value, None

    def __enter__(self):
        self.old = set_option(self.key, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.key, self.old)
        return False


def check(rc, h):
    if rc != 0:
        raise AdafError("adafocus HIP call failed (%d): %s" % (rc, load_library().adaf_last_error(h).decode()))


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def on_current_device(*tensors):
    """Kernels are launched on the CURRENT device's current stream: refuse tensors that live elsewhere (a launch on
    the wrong device would be an invalid-handle error at best, unsynchronised peer access at worst)."""
    cur = torch.cuda.current_device()
    for t in tensors:
        if t is not None and t.is_cuda and t.device.index != cur:
            raise AdafError("adafocus_amd: tensor on cuda:%d but the current device is cuda:%d -- wrap the call in "
                            "torch.cuda.device(%d) (one process per GPU is the supported mode)" % (t.device.index, cur, t.device.index))


def ptr(t):
    """The device pointer of t (None: NULL).  It holds NO reference to t: whoever calls this keeps t alive until the C call has returned
    (hip_ops._call does, for every launch of the package)."""
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def need_gpu(*tensors, f32=False):
    """Product-path guard: the HIP path is the only path.  Every tensor (None is skipped) lives on the current GPU; f32: and is fp32."""
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise AdafError("adafocus_amd runs on MI355X only: got a %s tensor (no CPU fallback exists)" % t.device)
        if f32 and t.dtype != torch.float32:
            raise AdafError("adafocus_amd computes in fp32: got %s" % t.dtype)
    on_current_device(*tensors)


def need_gpu_f32(*tensors):
    need_gpu(*tensors, f32=True)
