"""Helpers for the strided / unaligned operand tests of the C ABI (include/adafocus.h): the guard-banded allocations and the ctypes
caller with real ldx / ldo / ldr of tools/guard_bands.py (one implementation, shared with tools/conv_fuzz.py), a float64 conv reference
and the shared bounds.  Plain functions: no fixtures, usable on CPU tensors (the host tests check the checker itself) and on the GPU."""
import torch
import torch.nn.functional as F

from adafocus_amd._lib import ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SIGMOID, ACT_SWISH  # noqa: F401  (the header's ADAF_ACT_* codes)
from tests.helpers import load_tool
from tests.test_hip_parity import CONV_TOL  # noqa: F401  (the single-conv bound, shared -- not restated)

_G = load_tool("guard_bands")
CANARY_F32, CANARY_F16 = _G.CANARY_F32, _G.CANARY_F16
guarded, lead_for, fill, payload = _G.guarded, _G.lead_for, _G.fill, _G.payload
find_guard_damage, assert_guards_intact, conv_call = _G.find_guard_damage, _G.assert_guards_intact, _G.conv_call
guarded_workspace, workspace_damage, assert_workspace_intact = _G.guarded_workspace, _G.workspace_damage, _G.assert_workspace_intact
is_all_canary, WS_GUARD_MIN = _G.is_all_canary, _G.WS_GUARD_MIN

F16_STORE_REL = 2e-3         # one fp16 rounding of the stored value (tests/test_hip_parity_r2.py uses conv_f16_bound below)


def conv_f16_bound(out_dtype, ref):
    """Bound of adaf_conv2d_bn_act_f16 against a conv of the same fp16 VALUES: summation order only with an fp32 store, one fp16
    rounding of the result with an fp16 store."""
    return CONV_TOL if out_dtype == torch.float32 else F16_STORE_REL * max(1.0, ref.abs().max().item())


# ---- float64 reference -------------------------------------------------------------------------------------------------------------
def temporal_shift64(x_nchw, n_segment, fold_div):
    """TemporalShift.shift on (N*T, C, H, W): the first fold channels come from the next frame, the next fold from the previous one,
    zeros at the clip ends."""
    nt, c, h, w = x_nchw.shape
    x = x_nchw.reshape(nt // n_segment, n_segment, c, h, w)
    fold = c // fold_div
    out = torch.zeros_like(x)
    out[:, :-1, :fold] = x[:, 1:, :fold]
    out[:, 1:, fold:2 * fold] = x[:, :-1, fold:2 * fold]
    out[:, :, 2 * fold:] = x[:, :, 2 * fold:]
    return out.reshape(nt, c, h, w)


def conv_ref64(x_nhwc, w_ohwi, scale=None, bias=None, residual=None, stride=1, pad=0, act=ACT_NONE, tsm_segments=0, tsm_div=8):
    """adaf_conv2d_bn_act_* in float64 on the CPU: x (N,H,W,Cin), w (Cout,KH,KW,Cin), residual (N,OH,OW,Cout) -> (N,OH,OW,Cout)."""
    x = x_nhwc.detach().cpu().double().permute(0, 3, 1, 2)
    w = w_ohwi.detach().cpu().double().permute(0, 3, 1, 2)
    if tsm_segments:
        x = temporal_shift64(x, tsm_segments, tsm_div)
    y = F.conv2d(x, w, stride=stride, padding=pad).permute(0, 2, 3, 1)
    if scale is not None:
        y = y * scale.detach().cpu().double()
    if bias is not None:
        y = y + bias.detach().cpu().double()
    if residual is not None:
        y = y + residual.detach().cpu().double()
    if act == ACT_RELU:
        y = y.clamp(min=0)
    elif act == ACT_RELU6:
        y = y.clamp(0, 6)
    elif act == ACT_SIGMOID:
        y = torch.sigmoid(y)
    elif act == ACT_SWISH:
        y = y * torch.sigmoid(y)
    elif act != ACT_NONE:
        raise ValueError("conv_ref64: unknown activation %r" % (act,))
    return y.contiguous()
