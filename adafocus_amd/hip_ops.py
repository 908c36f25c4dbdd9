"""Tensor-level wrappers over the C ABI (include/adafocus.h).  Everything here enqueues
hand-written gfx950 kernels on the current HIP stream; nothing falls back to ATen.

Activation tensors are fp32 NHWC (``(N, H, W, C)`` contiguous) unless a function says otherwise.
"""
import ctypes as C

import torch

from . import _lib as L
from ._lib import ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SIGMOID, ACT_SWISH, LAYOUT_NCHW, LAYOUT_NHWC, LAYOUT_NHWC4  # noqa: F401
from ._lib import MATH_F16, MATH_F32, MATH_F32_SPLIT_BF16  # noqa: F401
from ._lib import DTYPE_F32, DTYPE_F16  # noqa: F401


def _ptrs(args):
    return [L.ptr(a) if isinstance(a, torch.Tensor) else a for a in args]


def _call(sym, where, *args, stream=True):
    """Every handle-first C-ABI call: sym(handle of `where` (a tensor or a device), *args[, the current stream]), return code checked.
    Tensors among `args` go as their data pointers, None as NULL, Python numbers and ctypes values as they are (the prototypes of
    _lib.PROTOTYPES convert them).

    THE OPERAND RULE.  L.ptr holds no reference, so a tensor must stay referenced until the C call has returned: a temporary that dies
    earlier hands its block back to the caching allocator, and the next temporary made on the same stream gets that very block -- two
    pointers to one buffer, and no error.  `args` is that reference.  So wrappers pass tensors here, temporaries such as
    `t.contiguous()` or `_dense(t)` included, and never call L.ptr on an expression (tests/test_abi.py walks this file for it).  Once
    the call has returned the launch is enqueued, and the allocator reuses a freed block in stream order only."""
    h = L.handle(where.device if isinstance(where, torch.Tensor) else where)
    L.check(getattr(L.load_library(), sym)(h, *_ptrs(args), *((L.stream_ptr(),) if stream else ())), h)


def _dense(t):
    return None if t is None else t.contiguous()


def _workspace(query, device, *extents):
    """-> (scratch tensor, the bytes `query`(*extents) asks for).  The tensor has 16 bytes at least, so it is a pointer even when
    the call needs none."""
    need = getattr(L.load_library(), query)(*extents)
    return torch.empty(max((need + 3) // 4, 4), device=device, dtype=torch.float32), need


def _gru_x(x):
    """The GRU entry points read x (B,T,F) through its row stride: unit feature stride and a batch stride of T rows, else a copy."""
    return x if x.stride(2) == 1 and x.stride(0) == x.shape[1] * x.stride(1) else x.contiguous()


def pixel_major(frames):
    """frames (N,H,W,4) pixel-major rather than (N,C,H,W) planar (four-pixel-wide RGB planes are planar)."""
    return frames.shape[-1] == 4 and frames.shape[1] != 3


def _frame_geometry(frames):
    """-> (layout, n, channels, h, w) of planar or pixel-major frames."""
    if pixel_major(frames):
        n, hh, ww, _ = frames.shape
        return LAYOUT_NHWC4, n, 3, hh, ww
    n, c, hh, ww = frames.shape
    return LAYOUT_NCHW, n, c, hh, ww


def _current(device):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def crop_gather(frames, actions, patch, frames_per_action=1, layout=LAYOUT_NCHW, return_coords=False):
    """Batched get_patch (ACT/models/utils.py:37-51).  frames (N,C,H,W) fp32, actions (M,2) fp32 in
    [0,1] with M*frames_per_action == N.  Returns (N,C,P,P) [NCHW], (N,P,P,C) [NHWC] or
    (N,P,P,4) [NHWC4]; optionally also the int32 (M,2) window origins."""
    L.need_gpu_f32(frames, actions)
    if frames.dim() != 4 or actions.dim() != 2 or actions.shape[1] != 2:
        raise ValueError("crop_gather: frames (N,C,H,W) and actions (M,2) expected")
    frames = frames.contiguous()
    actions = actions.contiguous()
    n, c, hh, ww = frames.shape
    p = int(patch)
    if layout == LAYOUT_NCHW:
        out = torch.empty((n, c, p, p), device=frames.device, dtype=torch.float32)
    elif layout == LAYOUT_NHWC:
        out = torch.empty((n, p, p, c), device=frames.device, dtype=torch.float32)
    else:
        out = torch.empty((n, p, p, 4), device=frames.device, dtype=torch.float32)
    coords = torch.empty((actions.shape[0], 2), device=frames.device, dtype=torch.int32) if return_coords else None
    _call("adaf_crop_gather_f32", frames, frames, n, c, hh, ww, actions, actions.shape[0], int(frames_per_action), p, out, layout, coords)
    return (out, coords) if return_coords else out


def pack_conv_weight(w_oihw, cin_pad=None):
    """OIHW -> OHWI (input channels zero-padded to a multiple of 4)."""
    L.need_gpu_f32(w_oihw)
    w = w_oihw.contiguous()
    co, ci, kh, kw = w.shape
    cp = cin_pad or ((ci + 3) // 4 * 4)
    out = torch.empty((co, kh, kw, cp), device=w.device, dtype=torch.float32)
    _call("adaf_pack_conv_weight_f32", w, w, co, ci, kh, kw, cp, out)
    return out


def fold_bn(gamma, beta, mean, var, eps=1e-5):
    L.need_gpu_f32(gamma, beta, mean, var)
    c = gamma.numel()
    scale = torch.empty(c, device=gamma.device, dtype=torch.float32)
    bias = torch.empty(c, device=gamma.device, dtype=torch.float32)
    _call("adaf_fold_bn_f32", gamma, gamma.contiguous(), beta.contiguous(), mean.contiguous(), var.contiguous(), float(eps), c, scale, bias)
    return scale, bias


def conv2d_bn_act(x, w_ohwi, scale=None, bias=None, residual=None, stride=1, pad=0, act=ACT_NONE, tsm_segments=0,
                  tsm_div=8, tile=0, naive=False, out=None):
    """x (N,H,W,Cin) NHWC, w (Cout,KH,KW,Cin) -> (N,OH,OW,Cout).  `naive=True` runs the
    one-thread-per-output cross-check kernel instead of the MFMA engine (tests only)."""
    L.need_gpu_f32(x, w_ohwi, scale, bias, residual)
    x = x.contiguous()
    w_ohwi = w_ohwi.contiguous()
    n, hh, ww, cin = x.shape
    cout, kh, kw, cin_w = w_ohwi.shape
    if cin_w != cin:
        raise ValueError("conv2d_bn_act: x has %d channels, weight expects %d" % (cin, cin_w))
    oh = (hh + 2 * pad - kh) // stride + 1
    ow = (ww + 2 * pad - kw) // stride + 1
    if out is None:
        out = torch.empty((n, oh, ow, cout), device=x.device, dtype=torch.float32)
    if residual is not None:
        residual = residual.contiguous()
    p = L.ConvParams(n=n, h=hh, w=ww, cin=cin, cout=cout, kh=kh, kw=kw, stride=stride, pad=pad, act=act,
                     tsm_segments=tsm_segments, tsm_div=tsm_div, ldx=0, ldo=0, ldr=0, tile=tile)
    _call("adaf_conv2d_naive_f32" if naive else "adaf_conv2d_bn_act_f32", x, C.byref(p), x, w_ohwi, scale, bias, residual, out)
    return out


def linear(x, weight, bias=None, act=ACT_NONE, tile=0):
    """nn.Linear on the MFMA engine: x (rows, in) row-major, weight (out, in)."""
    rows, fin = x.shape
    y = conv2d_bn_act(x.reshape(rows, 1, 1, fin), weight.reshape(weight.shape[0], 1, 1, fin), None, bias, act=act,
                      tile=tile)
    return y.reshape(rows, weight.shape[0])


def maxpool3x3s2(x):
    L.need_gpu_f32(x)
    x = x.contiguous()
    n, hh, ww, c = x.shape
    out = torch.empty((n, (hh - 1) // 2 + 1, (ww - 1) // 2 + 1, c), device=x.device, dtype=torch.float32)
    _call("adaf_maxpool3x3s2_f32", x, x, n, hh, ww, c, out)
    return out


def global_avgpool(x):
    L.need_gpu_f32(x)
    x = x.contiguous()
    n, hh, ww, c = x.shape
    out = torch.empty((n, c), device=x.device, dtype=torch.float32)
    _call("adaf_global_avgpool_f32", x, x, n, hh * ww, c, out, c)
    return out


def temporal_shift(x, n_segment, fold_div, layout=LAYOUT_NCHW):
    """TemporalShift.shift (STH/ops/temporal_shift.py:28-46).  x (NT,C,H,W) [NCHW] or (NT,H,W,C)."""
    L.need_gpu_f32(x)
    x = x.contiguous()
    if layout == LAYOUT_NCHW:
        nt, c, hh, ww = x.shape
    else:
        nt, hh, ww, c = x.shape
    out = torch.empty_like(x)
    _call("adaf_temporal_shift_f32", x, x, nt, c, hh * ww, int(n_segment), int(fold_div), layout, out)
    return out


def gru_cls_forward(x, w_ih, w_hh, b_ih, b_hh, fc_w, fc_b):
    """RecurrentClassifier.forward (ACT/models/gfv_net.py:427-435).  x (B,T,F) (last dim may be a
    strided view with stride 1) -> (logits (B*T,C), last (B,C))."""
    L.need_gpu_f32(x, w_ih, w_hh, b_ih, b_hh, fc_w, fc_b)
    b, t, f = x.shape
    x = _gru_x(x)
    hid, ncls = w_hh.shape[1], fc_w.shape[0]
    ws, ws_bytes = _workspace("adaf_gru_cls_workspace_bytes", x.device, b, t, hid)
    logits = torch.empty((b * t, ncls), device=x.device, dtype=torch.float32)
    last = torch.empty((b, ncls), device=x.device, dtype=torch.float32)
    _call("adaf_gru_cls_forward_f32", x, x, x.stride(1), b, t, f, hid, ncls, w_ih.contiguous(), w_hh.contiguous(), b_ih.contiguous(),
          b_hh.contiguous(), fc_w.contiguous(), fc_b.contiguous(), logits, last, ws, ws_bytes)
    return logits, last


def gru_cls_train_forward(x, w_ih, w_hh, b_ih, b_hh, fc_w, fc_b, mask=None):
    """Stage-3 training forward of RecurrentClassifier (adaf_gru_cls_train_forward_f32): x (B,T,F), mask (B,T,H) dropout multipliers
    (0 or 1/(1-p)) or None -> (logits (B*T,C), gi (B*T,3H), hs (B,T,H)); gi and hs are what gru_cls_backward needs."""
    L.need_gpu_f32(x, w_ih, w_hh, b_ih, b_hh, fc_w, fc_b, mask)
    b, t, f = x.shape
    x = _gru_x(x)
    hid, ncls = w_hh.shape[1], fc_w.shape[0]
    ws, ws_bytes = _workspace("adaf_gru_cls_train_workspace_bytes", x.device, b, t, hid)
    gi = torch.empty((b * t, 3 * hid), device=x.device, dtype=torch.float32)
    hs = torch.empty((b, t, hid), device=x.device, dtype=torch.float32)
    logits = torch.empty((b * t, ncls), device=x.device, dtype=torch.float32)
    _call("adaf_gru_cls_train_forward_f32", x, x, x.stride(1), b, t, f, hid, ncls, w_ih.contiguous(), w_hh.contiguous(), b_ih.contiguous(),
          b_hh.contiguous(), fc_w.contiguous(), fc_b.contiguous(), _dense(mask), gi, hs, logits, None, ws, ws_bytes)
    return logits, gi, hs


def gru_cls_backward(x, w_ih, w_hh, b_hh, fc_w, gi, hs, mask, dlogits, want_dx=True):
    """adaf_gru_cls_backward_f32: gradients of the GRU classifier from dlogits (B*T,C) and the activations of gru_cls_train_forward (same
    mask).  Returns (dx (B,T,F) or None, dW_ih, dW_hh, db_ih, db_hh, dW_fc, db_fc); deterministic (same inputs, same bits)."""
    L.need_gpu_f32(x, w_ih, w_hh, b_hh, fc_w, gi, hs, mask, dlogits)
    b, t, f = x.shape
    x = _gru_x(x)
    hid, ncls = w_hh.shape[1], fc_w.shape[0]
    ws, ws_bytes = _workspace("adaf_gru_cls_backward_workspace_bytes", x.device, b, t, hid, ncls)
    dev, fp = x.device, torch.float32
    dx = torch.empty((b, t, f), device=dev, dtype=fp) if want_dx else None
    dw_ih = torch.empty((3 * hid, f), device=dev, dtype=fp)
    dw_hh = torch.empty((3 * hid, hid), device=dev, dtype=fp)
    db_ih = torch.empty((3 * hid,), device=dev, dtype=fp)
    db_hh = torch.empty((3 * hid,), device=dev, dtype=fp)
    dw_fc = torch.empty((ncls, hid), device=dev, dtype=fp)
    db_fc = torch.empty((ncls,), device=dev, dtype=fp)
    _call("adaf_gru_cls_backward_f32", x, x, x.stride(1), b, t, f, hid, ncls, w_ih.contiguous(), w_hh.contiguous(), b_hh.contiguous(),
          fc_w.contiguous(), gi.contiguous(), hs.contiguous(), _dense(mask), dlogits.contiguous(), dx, dw_ih, dw_hh, db_ih, db_hh, dw_fc, db_fc, ws, ws_bytes)
    return dx, dw_ih, dw_hh, db_ih, db_hh, dw_fc, db_fc


class GruClassifierFn(torch.autograd.Function):
    """logits (B*T,C) of GRU -> dropout(mask) -> Linear with a HIP backward (stage 3 of ACT/main_dist.py trains classifier.* only).
    apply(x, w_ih, w_hh, b_ih, b_hh, fc_w, fc_b, mask): grads for x (when it requires grad) and the six parameters, so they land in
    the .grad of nn.GRU / nn.Linear.  Runs in fp32 under autocast (inputs are cast; the logits stay fp32).  Nothing is cached across
    calls: every forward reads the parameters as they are, so the step after optimizer.step() sees the new weights."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, fc_w, fc_b, mask):
        w_ih, w_hh, b_ih, b_hh, fc_w, fc_b = (p.detach() for p in (w_ih, w_hh, b_ih, b_hh, fc_w, fc_b))
        x = x.detach()
        logits, gi, hs = gru_cls_train_forward(x, w_ih, w_hh, b_ih, b_hh, fc_w, fc_b, mask)
        ctx.save_for_backward(x, w_ih, w_hh, b_hh, fc_w, gi, hs, mask)
        return logits

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        x, w_ih, w_hh, b_hh, fc_w, gi, hs, mask = ctx.saved_tensors
        dx, dw_ih, dw_hh, db_ih, db_hh, dw_fc, db_fc = gru_cls_backward(x, w_ih, w_hh, b_hh, fc_w, gi, hs, mask, g.float(),
                                                                        want_dx=ctx.needs_input_grad[0])
        return dx, dw_ih, dw_hh, db_ih, db_hh, dw_fc, db_fc, None


# ---- stage-2 training: PPO roll-out and policy update (csrc/ppo_train.hip) -------------------------------------------------------------
def ppo_sample(logits, uniforms, want_probs=False):
    """Categorical(softmax(logits)).sample() from caller-drawn uniforms in [0, 1): logits (rows, A), uniforms (rows,) ->
    (action int64 (rows,), logprob (rows,)[, probs (rows, A)])."""
    L.need_gpu_f32(logits, uniforms)
    logits, uniforms = logits.contiguous(), uniforms.contiguous()
    rows, a = logits.shape
    if uniforms.numel() != rows:
        raise ValueError("ppo_sample: one uniform per row expected")
    action = torch.empty((rows,), device=logits.device, dtype=torch.int64)
    logprob = torch.empty((rows,), device=logits.device, dtype=torch.float32)
    probs = torch.empty((rows, a), device=logits.device, dtype=torch.float32) if want_probs else None
    _call("adaf_ppo_sample_f32", logits, logits, a, rows, a, uniforms, action, logprob, probs)
    return (action, logprob, probs) if want_probs else (action, logprob)


def ppo_sample_actions(logits, uniforms, table=None):
    """The sampling of a whole roll-out in one launch: logits (B*T, A) with rows b*T+t (a row stride >= A is taken as it is), uniforms (T, B)
    in [0, 1), table (A, 2) or None -> (actions int64 (T, B), logprobs (T, B)[, coords (B*T, 2) = table[action], rows b*T+t]).  Per row the
    arithmetic is ppo_sample's: the same bits as T calls of it."""
    L.need_gpu_f32(logits, uniforms, table)
    if logits.dim() != 2 or uniforms.dim() != 2:
        raise ValueError("ppo_sample_actions: logits (B*T, A) and uniforms (T, B) expected")
    if logits.stride(1) != 1 or logits.stride(0) < logits.shape[1]:
        logits = logits.contiguous()
    uniforms = uniforms.contiguous()
    rows, a = logits.shape
    t, b = uniforms.shape
    if rows != t * b:
        raise ValueError("ppo_sample_actions: one uniform per row expected")
    if table is not None and tuple(table.shape) != (a, 2):
        raise ValueError("ppo_sample_actions: table (A, 2) expected")
    action = torch.empty((t, b), device=logits.device, dtype=torch.int64)
    logprob = torch.empty((t, b), device=logits.device, dtype=torch.float32)
    coords = torch.empty((rows, 2), device=logits.device, dtype=torch.float32) if table is not None else None
    _call("adaf_ppo_sample_actions_f32", logits, logits, logits.stride(0), t, b, a, uniforms, _dense(table), action, logprob, coords)
    return (action, logprob) if table is None else (action, logprob, coords)


REWARD_KINDS = {"prev": 0, "conf": 1, "random": 2}


def ppo_rewards(logits, base_logits, target, steps, kind, want_conf=False, want_ce_last=False):
    """The rewards of a whole roll-out (ACT/main_dist.py:511-516, 574-581): logits (B*T, C) with rows b*T+t, base_logits the same shape (the
    baseline's; None unless kind is 'random'), target (B,) int64, kind 'prev' | 'conf' | 'random' (or its number) ->
    rewards (T, B)[, confidences (T, B)][, the mean cross-entropy of the last step (1,)]."""
    L.need_gpu_f32(logits, base_logits)
    if target.dtype != torch.int64 or not target.is_cuda:
        raise ValueError("ppo_rewards: int64 GPU target (B,) expected")
    logits, target = logits.contiguous(), target.contiguous()
    t, b = int(steps), target.numel()
    if logits.dim() != 2 or logits.shape[0] != t * b:
        raise ValueError("ppo_rewards: logits (B*T, C) expected")
    if base_logits is not None:
        if base_logits.shape != logits.shape:
            raise ValueError("ppo_rewards: base_logits of the logits' shape expected")
        base_logits = base_logits.contiguous()
    kind = REWARD_KINDS.get(kind, kind)
    if not isinstance(kind, int):
        raise NotImplementedError("reward %r" % (kind,))
    dev, fp = logits.device, torch.float32
    rewards = torch.empty((t, b), device=dev, dtype=fp)
    conf = torch.empty((t, b), device=dev, dtype=fp) if want_conf else None
    ce = torch.empty((1,), device=dev, dtype=fp) if want_ce_last else None
    _call("adaf_ppo_rewards_f32", logits, logits, base_logits, target, t, b, logits.shape[1], kind, rewards, conf, ce)
    out = (rewards,) + ((conf,) if want_conf else ()) + ((ce,) if want_ce_last else ())
    return out if len(out) > 1 else rewards


def ce_steps(logits, target, steps, want_grad=True):
    """The stage-1 loss (ACT/main_dist.py:479): logits (B*T, C) with rows b*T+t, target (B,) int64 -> (the mean over all B*T rows of the
    cross-entropy of row b*T+t against class target[b] (1,), its gradient d loss / d logits (B*T, C) or None without want_grad).
    `target.view(B, 1).expand(B, T).reshape(-1)` is never materialised.  Deterministic (same inputs, same bits)."""
    L.need_gpu_f32(logits)
    if target.dtype != torch.int64 or not target.is_cuda:
        raise ValueError("ce_steps: int64 GPU target (B,) expected")
    logits, target = logits.contiguous(), target.contiguous()
    t, b = int(steps), target.numel()
    if logits.dim() != 2 or t <= 0 or logits.shape[0] != t * b:
        raise ValueError("ce_steps: logits (B*T, C) expected")
    ws, ws_bytes = _workspace("adaf_ce_steps_workspace_bytes", logits.device, b, t)
    loss = torch.empty((1,), device=logits.device, dtype=torch.float32)
    dlogits = torch.empty_like(logits) if want_grad else None
    _call("adaf_ce_steps_f32", logits, logits, target, b, t, logits.shape[1], loss, dlogits, ws, ws_bytes)
    return loss, dlogits


class CeStepsFn(torch.autograd.Function):
    """apply(logits (B*T, C), target (B,), steps) -> the loss (1,) of `ce_steps`.  The forward keeps dlogits; the backward is
    grad_out * dlogits."""

    @staticmethod
    def forward(ctx, logits, target, steps):
        loss, dlogits = ce_steps(logits.detach(), target, steps)
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        dlogits, = ctx.saved_tensors
        return grad_out * dlogits, None, None


def ppo_returns(rewards, gamma):
    """rewards (T, B) -> discounted returns, normalised over all T*B entries (ACT/models/ppo.py:148-157)."""
    L.need_gpu_f32(rewards)
    rewards = rewards.contiguous()
    t, b = rewards.shape
    out = torch.empty_like(rewards)
    _call("adaf_ppo_returns_f32", rewards, rewards, t, b, float(gamma), out)
    return out


def _ppo_head(head, actions, batch_major, sigma=None, old_logprobs=None, returns=None, eps_clip=0.2, grads=None):
    """The head kernel of csrc/ppo_train.hip in its three modes (statistics; PPO loss + its gradient when old_logprobs is given; pull-back
    of `grads` = upstream (g_logprob, g_value, g_entropy)) for both distributions: sigma None is the categorical head with int64 actions
    (T, B), a float the Gaussian head with that standard deviation and fp32 actions (T, B, 2) [no entropy gradient]."""
    gauss = sigma is not None
    L.need_gpu_f32(head, old_logprobs, returns, *(grads or ()), *((actions,) if gauss else ()))
    head, actions = head.contiguous(), actions.contiguous()
    if gauss:
        if actions.dim() != 3 or actions.shape[2] != 2 or head.shape != (actions.shape[0] * actions.shape[1], 3):
            raise ValueError("ppo gauss head: head (T*B, 3) and actions (T, B, 2) expected")
        t, b = actions.shape[:2]
    else:
        t, b = actions.shape
        if head.shape[0] != t * b or actions.dtype != torch.int64 or not actions.is_cuda:
            raise ValueError("ppo head: head (T*B, A+1) and int64 GPU actions (T, B) expected")
    dev, fp = head.device, torch.float32
    logprobs, values, entropy = (torch.empty((t, b), device=dev, dtype=fp) for _ in range(3))
    loss_mode = old_logprobs is not None
    loss = torch.empty((1,), device=dev, dtype=fp) if loss_mode else None
    dhead = torch.empty_like(head) if (loss_mode or grads is not None) else None
    ws, ws_bytes = _workspace("adaf_ppo_head_workspace_bytes", dev, t, b) if loss_mode else (None, 0)      # (only the loss has one)
    g = [_dense(x) for x in (grads or ())] + [None] * 3
    loss_in = (_dense(old_logprobs), _dense(returns), float(eps_clip))
    outs = (logprobs, values, entropy, loss, dhead, ws, ws_bytes)
    if gauss:
        _call("adaf_ppo_gauss_head_f32", head, head, int(batch_major), t, b, actions, float(sigma), *loss_in, g[0], g[1], *outs)
    else:
        _call("adaf_ppo_head_f32", head, head, int(batch_major), t, b, head.shape[1] - 1, actions, *loss_in, g[0], g[1], g[2], *outs)
    return logprobs, values, entropy, loss, dhead


def ppo_head_stats(head, actions, batch_major=True):
    """head (T*B, A+1) [actor logits | critic value] (rows b*T+t when batch_major) -> (logprobs, values, entropy), each (T, B)."""
    return _ppo_head(head, actions, batch_major)[:3]


def ppo_head_backward(head, actions, g_logprob, g_value, g_entropy, batch_major=True):
    """Pull-back of upstream gradients of (logprobs, values, entropy) (each (T, B) or None) to the head output."""
    if g_logprob is None and g_value is None and g_entropy is None:
        return torch.zeros_like(head)
    return _ppo_head(head, actions, batch_major, grads=(g_logprob, g_value, g_entropy))[4]


def ppo_loss_head(head, actions, old_logprobs, returns, eps_clip, batch_major=True):
    """The PPO loss head, forward and backward in one pass (ACT/models/ppo.py:114-122,166-175):
    -> (logprobs, values, entropy (T, B), loss.mean() (1,), d loss.mean() / d head (T*B, A+1))."""
    return _ppo_head(head, actions, batch_major, old_logprobs=old_logprobs, returns=returns, eps_clip=eps_clip)


def rows_transpose(x, ni, nj):
    """x (ni*nj, W) with rows i*nj+j -> rows j*ni+i."""
    L.need_gpu_f32(x)
    x = x.contiguous()
    w = x.shape[-1]
    out = torch.empty_like(x)
    _call("adaf_ppo_rows_transpose_f32", x, x, int(ni), int(nj), w, out)
    return out


def ppo_wenc_grad(states, de1, e1, split_k=True):
    """The 1x1 conv's weight gradient: states (pixels, C), de1 / e1 (pixels, 32 | 64) -> (32 | 64, C) = (de1 where e1 > 0)^T states
    (e1 None: de1 as it is).  split_k=False: the single-chain cross-check on the strided GEMM."""
    L.need_gpu_f32(states, de1, e1)
    npix, cin = states.shape
    cmid = de1.shape[1]
    ws, ws_bytes = _workspace("adaf_ppo_wenc_grad_workspace_bytes", states.device, npix, cin, cmid)
    dw = torch.empty((cmid, cin), device=states.device, dtype=torch.float32)
    _call("adaf_ppo_wenc_grad_f32", states, states.contiguous(), de1.contiguous(), _dense(e1), npix, cin, cmid, int(bool(split_k)), dw, ws,
          ws_bytes)
    return dw


# ---- stage-2 training of the continuous policy (Something-Something; csrc/ppo_train.hip) ------------------------------------
def ppo_gauss_sample(mean, noise, sigma):
    """mean (rows, 2), noise (rows, 2) standard normals -> (action (rows, 2) = 1 - relu(1 - relu(mean + sigma * noise)), the log-probability
    (rows,) of the clamped action under N(mean, sigma^2 I))."""
    L.need_gpu_f32(mean, noise)
    if mean.dim() != 2 or mean.shape[1] != 2 or noise.shape != mean.shape:
        raise ValueError("ppo_gauss_sample: mean and noise (rows, 2) expected")
    mean, noise = mean.contiguous(), noise.contiguous()
    rows = mean.shape[0]
    action = torch.empty_like(mean)
    logprob = torch.empty((rows,), device=mean.device, dtype=torch.float32)
    _call("adaf_ppo_gauss_sample_f32", mean, mean, noise, rows, float(sigma), action, logprob)
    return action, logprob


def ppo_gauss_head_stats(head, actions, sigma, batch_major=True):
    """head (T*B, 3) [mean logits | value] (rows b*T+t when batch_major), actions (T, B, 2) -> (logprobs, values, entropy), each (T, B)."""
    return _ppo_head(head, actions, batch_major, sigma)[:3]


def ppo_gauss_head_backward(head, actions, sigma, g_logprob, g_value, batch_major=True):
    """Pull-back of upstream gradients of (logprobs, values) (each (T, B) or None; the entropy is a constant) to the head output."""
    if g_logprob is None and g_value is None:
        return torch.zeros_like(head)
    return _ppo_head(head, actions, batch_major, sigma, grads=(g_logprob, g_value))[4]


def ppo_gauss_loss_head(head, actions, sigma, old_logprobs, returns, eps_clip, batch_major=True):
    """The Gaussian PPO loss head, forward and backward in one pass: -> (logprobs, values, entropy (T, B), loss.mean() (1,),
    d loss.mean() / d head (T*B, 3))."""
    return _ppo_head(head, actions, batch_major, sigma, old_logprobs=old_logprobs, returns=returns, eps_clip=eps_clip)


def bn_train_forward(x, gamma, beta, running_mean=None, running_var=None, eps=1e-5, momentum=0.1, relu=True):
    """BatchNorm with batch statistics over the rows of x (rows, cols) [+ ReLU]; running_mean / running_var are updated in place.
    -> (y, mean (cols,), invstd (cols,)): with x, what bn_train_backward needs."""
    L.need_gpu_f32(x, gamma, beta, running_mean, running_var)
    if x.dim() != 2 or not x.is_contiguous():
        raise ValueError("bn_train_forward: contiguous x (rows, cols) expected")
    rows, cols = x.shape
    if rows < 2:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(x.shape),))
    for r in (running_mean, running_var):
        if r is not None and not r.is_contiguous():
            raise ValueError("bn_train_forward: contiguous running statistics expected (they are updated in place)")
    y = torch.empty_like(x)
    mean = torch.empty((cols,), device=x.device, dtype=torch.float32)
    invstd = torch.empty((cols,), device=x.device, dtype=torch.float32)
    ws, ws_bytes = _workspace("adaf_bn_train_workspace_bytes", x.device, rows, cols)
    _call("adaf_bn_train_forward_f32", x, x, rows, cols, gamma.contiguous(), beta.contiguous(), float(eps), float(momentum), running_mean, running_var,
          int(bool(relu)), y, mean, invstd, ws, ws_bytes)
    return y, mean, invstd


def bn_train_backward(x, y, dy, gamma, mean, invstd):
    """Backward of bn_train_forward: y its output after ReLU (None: no ReLU) -> (dx, dgamma, dbeta)."""
    L.need_gpu_f32(x, y, dy, gamma, mean, invstd)
    x, dy = x.contiguous(), dy.contiguous()
    rows, cols = x.shape
    dx = torch.empty_like(x)
    dgamma = torch.empty((cols,), device=x.device, dtype=torch.float32)
    dbeta = torch.empty((cols,), device=x.device, dtype=torch.float32)
    ws, ws_bytes = _workspace("adaf_bn_train_workspace_bytes", x.device, rows, cols)
    _call("adaf_bn_train_backward_f32", x, x, _dense(y), dy, rows, cols, gamma.contiguous(), mean.contiguous(), invstd.contiguous(), dx, dgamma,
          dbeta, ws, ws_bytes)
    return dx, dgamma, dbeta


def _map2d(t):
    """A dense pixel-major map (..., cols) as (rows, cols)."""
    t = t.contiguous()
    return t.reshape(-1, t.shape[-1])


def _bn_map_forward(who, sym, flag, x, gamma, beta, running_mean, running_var, eps, momentum, residual):
    """Both forwards over maps: `sym` with `flag` (the relu flag, or an ACT_* value) in the activation's place."""
    L.need_gpu_f32(x, gamma, beta, running_mean, running_var, residual)
    x2 = _map2d(x)
    rows, cols = x2.shape
    if rows < 2:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(x.shape),))
    if residual is not None and residual.shape != x.shape:
        raise ValueError("%s: the residual has another shape than x" % who)
    for r in (running_mean, running_var):
        if r is not None and not r.is_contiguous():
            raise ValueError("%s: contiguous running statistics expected (they are updated in place)" % who)
    y = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    mean = torch.empty((cols,), device=x.device, dtype=torch.float32)
    invstd = torch.empty((cols,), device=x.device, dtype=torch.float32)
    ws, ws_bytes = _workspace("adaf_bn_map_workspace_bytes", x.device, rows, cols)
    _call(sym, x, x2, rows, cols, gamma.contiguous(), beta.contiguous(), float(eps), float(momentum), running_mean, running_var, _dense(residual),
          int(flag), y, mean, invstd, ws, ws_bytes)
    return y, mean, invstd


def _bn_map_backward(who, sym, act, x, y, dy, gamma, mean, invstd):
    """Both backwards over maps: act None is `sym` without an activation operand (the mask is y > 0 where y is given)."""
    L.need_gpu_f32(x, y, dy, gamma, mean, invstd)
    if dy.shape != x.shape or (y is not None and y.shape != x.shape):
        raise ValueError("%s: shapes differ" % who)
    x2 = _map2d(x)
    rows, cols = x2.shape
    dx = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    dgamma = torch.empty((cols,), device=x.device, dtype=torch.float32)
    dbeta = torch.empty((cols,), device=x.device, dtype=torch.float32)
    ws, ws_bytes = _workspace("adaf_bn_map_workspace_bytes", x.device, rows, cols)
    _call(sym, x, x2, _dense(y), *(() if act is None else (int(act),)), dy.contiguous(), rows, cols, gamma.contiguous(), mean.contiguous(),
          invstd.contiguous(), dx, dgamma, dbeta, ws, ws_bytes)
    return dx, dgamma, dbeta


def bn_map_train_forward(x, gamma, beta, running_mean=None, running_var=None, eps=1e-5, momentum=0.1, residual=None, relu=True):
    """bn_train_forward for tall pixel-major maps (csrc/bn_map.hip): x (..., cols) dense, the statistics over every leading
    axis [+ residual of x's shape] [+ ReLU]; running_mean / running_var are updated in place.  cols % 4 == 0.
    -> (y of x's shape, mean (cols,), invstd (cols,))."""
    return _bn_map_forward("bn_map_train_forward", "adaf_bn_map_train_forward_f32", bool(relu), x, gamma, beta, running_mean, running_var, eps,
                           momentum, residual)


def bn_map_train_backward(x, y, dy, gamma, mean, invstd):
    """Backward of bn_map_train_forward: y its output after ReLU (None: no ReLU, or dy has its mask applied) -> (dx of x's shape, dgamma,
    dbeta).  A residual join's second gradient is added in front (relu_backward)."""
    return _bn_map_backward("bn_map_train_backward", "adaf_bn_map_train_backward_f32", None, x, y, dy, gamma, mean, invstd)


_BN_MAP_ACTS = (ACT_NONE, ACT_RELU, ACT_RELU6)


def bn_map_train_forward_act(x, gamma, beta, running_mean=None, running_var=None, eps=1e-5, momentum=0.1, residual=None, act=ACT_RELU6):
    """bn_map_train_forward with an activation in place of the relu flag: act = ACT_NONE, ACT_RELU or ACT_RELU6 (y clipped to [0, 6],
    MobileNetV2's activation) -> (y, mean, invstd).  ACT_NONE / ACT_RELU give bn_map_train_forward's bits."""
    if act not in _BN_MAP_ACTS:
        raise ValueError("bn_map_train_forward_act: act is ACT_NONE, ACT_RELU or ACT_RELU6")
    return _bn_map_forward("bn_map_train_forward_act", "adaf_bn_map_train_forward_act_f32", act, x, gamma, beta, running_mean, running_var, eps,
                           momentum, residual)


def bn_map_train_backward_act(x, y, dy, gamma, mean, invstd, act=ACT_RELU6):
    """Backward of bn_map_train_forward_act: y its output (read for ACT_RELU: dy passes where y > 0, and ACT_RELU6: where 0 < y < 6, ATen's
    hardtanh_backward on the activation's input; not read for ACT_NONE) -> (dx of x's shape, dgamma, dbeta)."""
    if act not in _BN_MAP_ACTS:
        raise ValueError("bn_map_train_backward_act: act is ACT_NONE, ACT_RELU or ACT_RELU6")
    if act != ACT_NONE and y is None:
        raise ValueError("bn_map_train_backward_act: the mask of an activation needs the forward's output")
    return _bn_map_backward("bn_map_train_backward_act", "adaf_bn_map_train_backward_act_f32", act, x, y, dy, gamma, mean, invstd)


def ppo_encoder_backward(states, e1, e_bt, dx_bt, t, b, w_lin_pm, bn=None):
    """Backward of the policy's state encoder (1x1 conv -> [BatchNorm2d] ReLU -> flatten -> Linear -> [BatchNorm1d] ReLU) for 32 or 64
    conv outputs: states (T*B, h, w, C) pixel-major, e1 (T*B, h*w*cmid) and e_bt (B*T, H) its stored activations, dx_bt (B, T, H) the
    GRU's input gradient; bn = (c1, gamma1, mean1, invstd1, l1, gamma2, mean2, invstd2): the raw conv / Linear outputs and the statistics
    of the forward -> (dW_enc (cmid, C), dW_lin (H, cmid*h*w) in the nn.Linear layout, db_lin (H,)[, dgamma1, dbeta1, dgamma2, dbeta2]).
    One entry point for both policies (adaf_ppo_encoder_bn_backward_f32): H and h*w*cmid are multiples of 4."""
    L.need_gpu_f32(states, e1, e_bt, dx_bt, w_lin_pm, *(bn or ()))
    hw, cin = states.shape[1] * states.shape[2], states.shape[3]
    hid = w_lin_pm.shape[0]
    cmid = w_lin_pm.shape[1] // hw
    dev, fp = states.device, torch.float32
    ws, ws_bytes = _workspace("adaf_ppo_encoder_bn_backward_workspace_bytes", dev, t, b, hw, cin, cmid, hid, int(bn is not None))
    dw_enc = torch.empty((cmid, cin), device=dev, dtype=fp)
    dw_lin = torch.empty((hid, cmid * hw), device=dev, dtype=fp)
    db_lin = torch.empty((hid,), device=dev, dtype=fp)
    extra = () if bn is None else tuple(torch.empty((n,), device=dev, dtype=fp) for n in (cmid, cmid, hid, hid))
    _call("adaf_ppo_encoder_bn_backward_f32", states, states.contiguous(), e1.contiguous(), e_bt.contiguous(), dx_bt.contiguous(), t, b, hw,
          cin, cmid, hid, w_lin_pm.contiguous(), *(_dense(x) for x in (bn or [None] * 8)), dw_enc, dw_lin, db_lin, *(extra or [None] * 4), ws,
          ws_bytes)
    return (dw_enc, dw_lin, db_lin) + extra


# ---- stage-3 training of the local CNN: backward of the trunk's convolutions (csrc/conv_bwd.hip) -----------------------------
def _bwd_params(x_shape, w_shape, stride, pad):
    n, hh, ww, cin = x_shape
    cout, kh, kw, cin_w = w_shape
    if cin_w != cin:
        raise ValueError("conv backward: the map has %d channels, the filter expects %d" % (cin, cin_w))
    p = L.ConvParams(n=n, h=hh, w=ww, cin=cin, cout=cout, kh=kh, kw=kw, stride=stride, pad=pad, act=ACT_NONE, tsm_segments=0, tsm_div=0, ldx=0,
                     ldo=0, ldr=0, tile=0)
    return p, (n, (hh + 2 * pad - kh) // stride + 1, (ww + 2 * pad - kw) // stride + 1, cout)


def stem7x7_bn_relu(patches_nhwc4, w_oihw, scale, bias):
    """The trunk's stem on its own kernel: (N,P,P,4) patches, w (64,3,7,7) in PyTorch's layout, folded BN -> (N,OH,OH,64) after ReLU;
    the bits of the ResNet50Trunk's stem (the generic engine adds the 147 products in another order)."""
    L.need_gpu_f32(patches_nhwc4, w_oihw, scale, bias)
    x, w, scale, bias = (t.contiguous() for t in (patches_nhwc4, w_oihw, scale, bias))
    n, p, p2, c = x.shape
    if c != 4 or p != p2 or tuple(w.shape) != (64, 3, 7, 7):
        raise ValueError("stem7x7_bn_relu: square (N,P,P,4) patches and a (64,3,7,7) filter expected")
    oh = (p - 1) // 2 + 1
    ws, ws_bytes = _workspace("adaf_stem7x7_workspace_bytes", x.device)
    out = torch.empty((n, oh, oh, 64), device=x.device, dtype=torch.float32)
    _call("adaf_stem7x7_bn_relu_f32", x, x, n, p, w, scale, bias, out, ws, ws_bytes)
    return out


STEM_FORMS = {"auto": L.STEM_FORM_AUTO, "tile4": L.STEM_FORM_TILE4, "tile6": L.STEM_FORM_TILE6, "strip": L.STEM_FORM_STRIP,
              "unfused": L.STEM_FORM_UNFUSED}
_STEM_FORM_NAMES = {v: k for k, v in STEM_FORMS.items()}


def stem7x7_pool_form(n, patch, device=None):
    """The form the trunk's walk takes for n patches of patch^2 with fusion on: 'strip', 'tile4', 'tile6' or 'unfused'."""
    dev = _current(device)
    return _STEM_FORM_NAMES[L.load_library().adaf_stem7x7_pool_form(L.handle(dev), int(n), int(patch))]


def stem7x7_pool(patches_nhwc4, w_oihw, scale, bias, form="auto", half=False, return_form=False):
    """The trunk's stem + max-pool, one form at a time (adaf_stem7x7_pool; a test surface): (N,P,P,4) patches -> the pooled map
    (N,PH,PH,64), fp32 or (half) fp16.  form: 'auto' (the walk's own choice), 'tile4', 'tile6', 'strip' (P 64 / 96 / 128 / 144 only)
    or 'unfused'.  return_form: -> (map, the name of the form that ran)."""
    L.need_gpu_f32(patches_nhwc4, w_oihw, scale, bias)
    x, w, scale, bias = (t.contiguous() for t in (patches_nhwc4, w_oihw, scale, bias))
    n, p, p2, c = x.shape
    if c != 4 or p != p2 or tuple(w.shape) != (64, 3, 7, 7):
        raise ValueError("stem7x7_pool: square (N,P,P,4) patches and a (64,3,7,7) filter expected")
    code = STEM_FORMS[form]
    oh = (p - 1) // 2 + 1
    ph = (oh - 1) // 2 + 1
    ws, ws_bytes = _workspace("adaf_stem7x7_workspace_bytes", x.device)
    resolved = code or STEM_FORMS[stem7x7_pool_form(n, p, x.device)]
    conv_map = torch.empty((n, oh, oh, 64), device=x.device, dtype=torch.float32) if resolved == L.STEM_FORM_UNFUSED else None
    out = torch.empty((n, ph, ph, 64), device=x.device, dtype=torch.float16 if half else torch.float32)
    used = C.c_int(-1)
    _call("adaf_stem7x7_pool", x, x, n, p, w, scale, bias, code, DTYPE_F16 if half else DTYPE_F32, out, conv_map, C.byref(used), ws, ws_bytes)
    return (out, _STEM_FORM_NAMES[used.value]) if return_form else out


def stem7x7_pool_frames(frames, actions, patch, w_oihw, scale, bias, frames_per_action=1, half=False):
    """The strip kernel gathering its own windows (adaf_stem7x7_pool_frames; a test surface): frames (N,3,H,W) planar or (N,H,W,4)
    pixel-major, actions (k * N / frames_per_action, 2) fp32 (y, x) -> the pooled map (k * N, PH, PH, 64) of the patches get_patch cuts."""
    L.need_gpu_f32(frames, actions, w_oihw, scale, bias)
    x, act, w, scale, bias = (t.contiguous() for t in (frames, actions, w_oihw, scale, bias))
    layout, nf, ch, hh, ww = _frame_geometry(x)
    fpa, p = int(frames_per_action), int(patch)
    if ch != 3 or act.dim() != 2 or act.shape[1] != 2 or tuple(w.shape) != (64, 3, 7, 7) or fpa < 1 or nf % fpa or act.shape[0] % (nf // fpa):
        raise ValueError("stem7x7_pool_frames: 3-channel frames, (k * N / frames_per_action, 2) actions and a (64,3,7,7) filter expected")
    n = act.shape[0] // (nf // fpa) * nf
    ph = p // 4
    ws, ws_bytes = _workspace("adaf_stem7x7_workspace_bytes", x.device)
    out = torch.empty((n, ph, ph, 64), device=x.device, dtype=torch.float16 if half else torch.float32)
    _call("adaf_stem7x7_pool_frames", x, x, layout, nf, hh, ww, act, act.shape[0], fpa, p, w, scale, bias, DTYPE_F16 if half else DTYPE_F32, out,
          ws, ws_bytes)
    return out


def maxpool3x3s2_f16out(x):
    """nn.MaxPool2d(3, 2, 1) of an fp32 NHWC map with an fp16 store (one rounding of the fp32 maximum): the fp16 trunk's unfused front."""
    L.need_gpu_f32(x)
    x = x.contiguous()
    n, hh, ww, c = x.shape
    out = torch.empty((n, (hh - 1) // 2 + 1, (ww - 1) // 2 + 1, c), device=x.device, dtype=torch.float16)
    _call("adaf_maxpool3x3s2_f16out", x, x, n, hh, ww, c, out)
    return out


def _conv2d_wgrad(who, x, g, w_shape, stride, pad):
    """Both split-K weight gradients: the entry point adaf_<who>_f32 with its workspace query."""
    L.need_gpu_f32(x, g)
    x, g = x.contiguous(), g.contiguous()
    p, g_shape = _bwd_params(x.shape, w_shape, stride, pad)
    if tuple(g.shape) != g_shape:
        raise ValueError("%s: gradient of shape %s expected, got %s" % (who, g_shape, tuple(g.shape)))
    ws, ws_bytes = _workspace("adaf_%s_workspace_bytes" % who, x.device, C.byref(p))
    dw = torch.empty(tuple(w_shape), device=x.device, dtype=torch.float32)
    _call("adaf_%s_f32" % who, x, C.byref(p), x, g, dw, ws, ws_bytes)
    return dw


def conv2d_wgrad(x, g, w_shape, stride=1, pad=0):
    """The UNSCALED weight gradient of a convolution: x (N,H,W,Cin), g (N,OH,OW,Cout) the gradient at the convolution's output, w_shape
    (Cout,KH,KW,Cin) -> (Cout,KH,KW,Cin).  Deterministic (same inputs, same bits)."""
    return _conv2d_wgrad("conv2d_wgrad", x, g, w_shape, stride, pad)


def conv2d_wgrad_rows(x, g, w_shape, stride=1, pad=0):
    """conv2d_wgrad for Cout % 4 == 0 (MobileNetV2's 16, 24 and 144 output channels): the same split-K launch with the last block's
    filter rows bounded at Cout; for Cout % 32 == 0 conv2d_wgrad's bits."""
    return _conv2d_wgrad("conv2d_wgrad_rows", x, g, w_shape, stride, pad)


def _dw_out_shape(x_shape, stride):
    n, hh, ww, c = x_shape
    return (n, (hh - 1) // stride + 1, (ww - 1) // stride + 1, c)


def dwconv3x3_dgrad(g, w_33c, x_shape, stride=1):
    """The gradient at the input of dwconv3x3_bn_act's convolution: g (N,OH,OW,C) the gradient at its output, w_33c of pack_dw_weight,
    x_shape (N,H,W,C) -> (N,H,W,C).  A gather with a fixed tap order (csrc/dw_bwd.hip)."""
    L.need_gpu_f32(g, w_33c)
    g, w_33c = g.contiguous(), w_33c.contiguous()
    n, hh, ww, c = x_shape
    if tuple(g.shape) != _dw_out_shape(x_shape, stride) or tuple(w_33c.shape) != (3, 3, c):
        raise ValueError("dwconv3x3_dgrad: gradient of shape %s and a (3,3,%d) filter expected, got %s and %s"
                         % (_dw_out_shape(x_shape, stride), c, tuple(g.shape), tuple(w_33c.shape)))
    dx = torch.empty(tuple(x_shape), device=g.device, dtype=torch.float32)
    _call("adaf_dwconv3x3_dgrad_f32", g, g, n, hh, ww, c, int(stride), w_33c, dx)
    return dx


def dwconv3x3_wgrad(x, g, stride=1):
    """The weight gradient of dwconv3x3_bn_act's convolution: x (N,H,W,C) its input, g (N,OH,OW,C) the gradient at its output ->
    (C,1,3,3), PyTorch's layout.  Slice partials in double, added in a fixed order: the same inputs give the same bits."""
    L.need_gpu_f32(x, g)
    x, g = x.contiguous(), g.contiguous()
    n, hh, ww, c = x.shape
    if tuple(g.shape) != _dw_out_shape(x.shape, stride):
        raise ValueError("dwconv3x3_wgrad: gradient of shape %s expected, got %s" % (_dw_out_shape(x.shape, stride), tuple(g.shape)))
    ws, ws_bytes = _workspace("adaf_dwconv3x3_wgrad_workspace_bytes", x.device, n, hh, ww, c, int(stride))
    dw = torch.empty((3, 3, c), device=x.device, dtype=torch.float32)
    _call("adaf_dwconv3x3_wgrad_f32", x, x, g, n, hh, ww, c, int(stride), dw, ws, ws_bytes)
    return dw.permute(2, 0, 1).reshape(c, 1, 3, 3).contiguous()


def add(a, b):
    """a + b of two dense maps of one shape: the join of two gradients where no activation masks it (relu_backward joins under a mask)."""
    L.need_gpu_f32(a, b)
    if a.shape != b.shape:
        raise ValueError("add: shapes differ")
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty_like(a)
    _call("adaf_add_f32", a, a, b, a.numel(), out)
    return out


def pack_conv_dgrad_weight(w_ohwi, scale=None):
    """(Cout,KH,KW,Cin) -> (Cin,KH,KW,Cout): transposed, rotated by 180 degrees, times scale per output channel -- conv2d_dgrad's filter."""
    L.need_gpu_f32(w_ohwi, scale)
    w_ohwi = w_ohwi.contiguous()
    cout, kh, kw, cin = w_ohwi.shape
    out = torch.empty((cin, kh, kw, cout), device=w_ohwi.device, dtype=torch.float32)
    _call("adaf_pack_conv_dgrad_weight_f32", w_ohwi, w_ohwi, _dense(scale), cout, kh, kw, cin, out)
    return out


def conv2d_dgrad(g, w_dgrad, x_shape, stride=1, pad=0):
    """The gradient at a convolution's input, on the forward engine: g (N,OH,OW,Cout), w_dgrad of pack_conv_dgrad_weight, x_shape
    (N,H,W,Cin) -> (N,H,W,Cin)."""
    L.need_gpu_f32(g, w_dgrad)
    g, w_dgrad = g.contiguous(), w_dgrad.contiguous()
    cin, kh, kw, cout = w_dgrad.shape
    p, g_shape = _bwd_params(x_shape, (cout, kh, kw, cin), stride, pad)
    if tuple(g.shape) != g_shape:
        raise ValueError("conv2d_dgrad: gradient of shape %s expected, got %s" % (g_shape, tuple(g.shape)))
    ws, ws_bytes = _workspace("adaf_conv2d_dgrad_workspace_bytes", g.device, C.byref(p))
    dx = torch.empty(tuple(x_shape), device=g.device, dtype=torch.float32)
    _call("adaf_conv2d_dgrad_f32", g, C.byref(p), g, w_dgrad, dx, ws, ws_bytes)
    return dx


def relu_backward(dy, y, dy2=None):
    """(dy [+ dy2]) where y > 0, else 0: ReLU backward with the residual join's second gradient."""
    L.need_gpu_f32(dy, y, dy2)
    dy, y, dy2 = dy.contiguous(), y.contiguous(), _dense(dy2)
    if dy.shape != y.shape or (dy2 is not None and dy2.shape != y.shape):
        raise ValueError("relu_backward: shapes differ")
    out = torch.empty_like(y)
    _call("adaf_relu_backward_f32", y, dy, dy2, y, y.numel(), out)
    return out


def global_avgpool_backward(dfeat, y_shape, y=None):
    """dfeat (N,C) -> (N,H,W,C) = dfeat / (H W) on every pixel; y given: zero where y <= 0 (the ReLU in front of the pool folded in)."""
    L.need_gpu_f32(dfeat, y)
    dfeat, y = dfeat.contiguous(), _dense(y)
    n, hh, ww, c = y_shape
    if tuple(dfeat.shape) != (n, c) or (y is not None and tuple(y.shape) != tuple(y_shape)):
        raise ValueError("global_avgpool_backward: shapes differ")
    out = torch.empty(tuple(y_shape), device=dfeat.device, dtype=torch.float32)
    _call("adaf_global_avgpool_backward_f32", dfeat, dfeat, c, y, n, hh * ww, c, out)
    return out


def maxpool3x3s2_backward(x, g):
    """nn.MaxPool2d(3, 2, 1) backward: x (N,H,W,C) the pool's input, g (N,OH,OW,C) -> (N,H,W,C); ATen's arg-max on ties."""
    L.need_gpu_f32(x, g)
    x, g = x.contiguous(), g.contiguous()
    n, hh, ww, c = x.shape
    if tuple(g.shape) != (n, (hh - 1) // 2 + 1, (ww - 1) // 2 + 1, c):
        raise ValueError("maxpool3x3s2_backward: gradient shape")
    dx = torch.empty_like(x)
    _call("adaf_maxpool3x3s2_backward_f32", x, x, g, n, hh, ww, c, dx)
    return dx


def temporal_shift_backward(g, n_segment, fold_div, layout=LAYOUT_NCHW):
    """The adjoint of temporal_shift (same arguments)."""
    L.need_gpu_f32(g)
    g = g.contiguous()
    if layout == LAYOUT_NCHW:
        nt, c, hh, ww = g.shape
    else:
        nt, hh, ww, c = g.shape
    out = torch.empty_like(g)
    _call("adaf_temporal_shift_backward_f32", g, g, nt, c, hh * ww, int(n_segment), int(fold_div), layout, out)
    return out


def conv_bn_param_grad(g, dw_ohwi, w_ohwi, scale, mean, var, eps, cin, want_dw=True, want_affine=True):
    """Parameter gradients of conv + BatchNorm(eval) from g (N,OH,OW,Cout), the unscaled dw_ohwi of conv2d_wgrad and the forward's packed
    filter: -> (dW (Cout,cin,KH,KW) = scale * dw or None, dgamma, dbeta (Cout,) or None).  Nothing divides by gamma."""
    L.need_gpu_f32(g, dw_ohwi, w_ohwi, scale, mean, var)
    g, dw_ohwi, w_ohwi, scale, mean, var = (t.contiguous() for t in (g, dw_ohwi, w_ohwi, scale, mean, var))
    cout, kh, kw, cin_pad = w_ohwi.shape
    dev = g.device
    ws, ws_bytes = _workspace("adaf_conv_bn_param_grad_workspace_bytes", dev, cout)
    dw = torch.empty((cout, cin, kh, kw), device=dev, dtype=torch.float32) if want_dw else None
    dgamma = torch.empty((cout,), device=dev, dtype=torch.float32) if want_affine else None
    dbeta = torch.empty((cout,), device=dev, dtype=torch.float32) if want_affine else None
    _call("adaf_conv_bn_param_grad_f32", g, g, g.numel() // cout, dw_ohwi, w_ohwi, scale, mean, var, float(eps), cout, kh, kw, int(cin), cin_pad,
          dw, dgamma, dbeta, ws, ws_bytes)
    return dw, dgamma, dbeta


def fc_meanpool_forward(feat, batch, fc_w, fc_b, global_logit=None):
    """mean_t FC(f_t) (+ mean_t glancer logits) -- STH/models/gfv_net.py:164-174.
    feat (B*T,F); global_logit (B,Tg,C) or None -> (B,C)."""
    L.need_gpu_f32(feat, fc_w, fc_b, global_logit)
    feat = feat.contiguous()
    rows, f = feat.shape
    t = rows // batch
    ncls = fc_w.shape[0]
    ws = torch.empty(max(rows * ncls, 1), device=feat.device, dtype=torch.float32)
    out = torch.empty((batch, ncls), device=feat.device, dtype=torch.float32)
    tg = 0
    if global_logit is not None:
        global_logit = global_logit.contiguous()
        tg = global_logit.shape[1]
    _call("adaf_fc_meanpool_forward_f32", feat, feat, batch, t, f, ncls, fc_w.contiguous(), fc_b.contiguous(), global_logit, tg, out, ws,
          ws.numel() * 4)
    return out


def copy2d(src, dst_view):
    """dst_view[:, :] = src for a row-strided destination (torch.cat on dim=1 without a new tensor)."""
    L.need_gpu_f32(src, dst_view)
    rows, cols = src.shape
    if src.stride(1) != 1 or dst_view.stride(1) != 1:
        raise ValueError("copy2d: unit inner stride required")
    _call("adaf_copy2d_f32", src, src, src.stride(0), dst_view, dst_view.stride(0), rows, cols)
    return dst_view


class _StreamScratch:
    """One scratch tensor per HIP stream: passes enqueued on different streams (pipelined batches) must not share
    intermediates.  Each tensor is allocated while its stream is current, so the caching allocator only ever reuses
    its memory in that stream's order; the least recently used entries are dropped beyond `cap` streams (short-lived
    streams would otherwise pin gigabytes each).  `cap` defaults to 6 (bench.py uses 3 streams + the model's own 2) and
    can be raised with ADAF_SCRATCH_STREAMS; an eviction is reported once per object on stderr, because rotating over
    more streams than `cap` means a multi-GB reallocation per call."""

    def __init__(self, device, cap=None):
        import os
        self.device = device
        self.cap = int(cap or os.environ.get("ADAF_SCRATCH_STREAMS", 6))
        self._ws, self._warned = {}, False

    def get(self, need_bytes):
        key = torch.cuda.current_stream(self.device).cuda_stream
        ws = self._ws.pop(key, None)
        if ws is None or ws.numel() * 4 < need_bytes:
            ws = torch.empty(max((need_bytes + 3) // 4, 1), device=self.device, dtype=torch.float32)
        self._ws[key] = ws                       # (re)insert as most recently used
        while len(self._ws) > self.cap:
            self._ws.pop(next(iter(self._ws)))
            if not self._warned:
                import sys
                print("adafocus_amd: more than %d streams rotate over one network's scratch space; the least recently used "
                      "buffer was dropped (set ADAF_SCRATCH_STREAMS to keep more)" % self.cap, file=sys.stderr)
                self._warned = True
        return ws

    def __len__(self):
        return len(self._ws)


class _NetEngine:
    """What the three network objects of the C ABI share: device / handle / library / per-stream scratch, the object's life and
    load().  A subclass names its symbols' stem (adaf_<_ABI>_create / _destroy / _set_param / _finalize)."""
    _ABI = None

    def __init__(self, device, *create_args):
        self.device = torch.device(device)
        self._h = L.handle(self.device)
        self._lib = L.load_library()
        net = C.c_void_p()
        _call("adaf_%s_create" % self._ABI, self.device, *create_args, C.byref(net), stream=False)
        self._net = net
        self._scratch = _StreamScratch(self.device)

    def _sym(self, what):
        return getattr(self._lib, "adaf_%s_%s" % (self._ABI, what))

    def _call(self, what, *args, stream=True):
        """adaf_<_ABI>_<what>(net, *args[, the current stream]), checked: _call's operand rule for the calls that take the network first."""
        L.check(self._sym(what)(self._net, *_ptrs(args), *((L.stream_ptr(),) if stream else ())), self._h)

    def __del__(self):
        try:
            if getattr(self, "_net", None):
                self._sym("destroy")(self._net)
                self._net = None
        except Exception:
            pass

    def _wanted(self, name):
        return True

    def load(self, params):
        """params: mapping parameter name -> fp32 tensor on this device.  The library reads them during finalize only (packed
        copies; include/adafocus.h), so every load registers the full set and the tensors may go when it returns."""
        keep = []                                # set_param records a pointer that finalize reads: dense copies live until then
        for name, t in params.items():
            if not self._wanted(name):
                continue
            L.need_gpu_f32(t)
            t = t.detach().contiguous()
            keep.append(t)
            self._call("set_param", name.encode(), t, t.numel(), stream=False)
        self._call("finalize")
        del keep


class ResNet50Trunk(_NetEngine):
    """adaf_resnet50: the whole local CNN (stem ... layer4, avgpool) as ~55 back-to-back launches on
    one stream, weights packed / BN folded once.  Replaces ResNet.get_featmap(x, pooled=True)
    (ACT/models/resnet.py:211-225) and TSN.forward(no_reshape=True) (STH/models/tsn.py:215-241)."""
    _ABI = "resnet50"

    def __init__(self, device):
        super().__init__(device)
        self.n_launches = self._lib.adaf_resnet50_launch_count(self._net)

    def _wanted(self, name):
        return not (name.startswith("fc.") or name.endswith("num_batches_tracked"))

    def load(self, params):
        """params: mapping torchvision-style name -> tensor (on this device).  Non-trunk entries
        (fc.*, num_batches_tracked) are ignored.  The names give the depth (ResNet-50, -101 or -152)."""
        super().load(params)
        self.n_launches = self._lib.adaf_resnet50_launch_count(self._net)

    def _workspace(self, n, patch):
        """One scratch buffer per HIP stream: passes enqueued on different streams (pipelined batches)
        must not share intermediates."""
        need = self._lib.adaf_resnet50_workspace_bytes(self._net, n, patch)
        return self._scratch.get(need), need

    def forward(self, patches_nhwc4, tsm_segments=0, tsm_div=8, out=None):
        """patches (N,P,P,4) -> (N,2048); `out` may be a (N,2048) row-strided view (e.g. the tail of
        the GRU input matrix)."""
        L.need_gpu_f32(patches_nhwc4, out)
        x = patches_nhwc4.contiguous()
        n, p = x.shape[0], x.shape[1]
        if out is None:
            out = torch.empty((n, 2048), device=x.device, dtype=torch.float32)
        ws, need = self._workspace(n, p)
        self._call("forward", x, n, p, int(tsm_segments), int(tsm_div), out, out.stride(0), ws, need)
        return out

    def forward_frames(self, frames, actions, patch, frames_per_action=1, tsm_segments=0, tsm_div=8, out=None):
        """get_patch + trunk in one call (adaf_resnet50_forward_frames): frames (N,3,H,W) planar or (N,H,W,4) pixel-major, actions
        (k * N / frames_per_action, 2) fp32 (y, x) -> (k * N, 2048); the stem gathers its own windows where its strip kernel applies."""
        L.need_gpu_f32(frames, actions, out)
        x = frames.contiguous()
        layout, nf, _, hh, ww = _frame_geometry(x)
        act = actions.contiguous()
        n = act.shape[0] // (nf // frames_per_action) * nf
        if out is None:
            out = torch.empty((n, 2048), device=x.device, dtype=torch.float32)
        ws, need = self._workspace(n, patch)
        self._call("forward_frames", x, layout, nf, hh, ww, act, act.shape[0], int(frames_per_action), int(patch), int(tsm_segments),
                   int(tsm_div), out, out.stride(0), ws, need)
        return out

    def forward_map(self, patches_nhwc4, tsm_segments=0, tsm_div=8):
        """patches (N,P,P,4) -> (featmap (N,s,s,2048) NHWC, pooled feature (N,2048)): ResNet.get_featmap(x, pooled=False)."""
        L.need_gpu_f32(patches_nhwc4)
        x = patches_nhwc4.contiguous()
        n, p = x.shape[0], x.shape[1]
        s = int(self._lib.adaf_resnet50_map_size(p))
        fmap = torch.empty((n, s, s, 2048), device=x.device, dtype=torch.float32)
        feat = torch.empty((n, 2048), device=x.device, dtype=torch.float32)
        ws, need = self._workspace(n, p)
        self._call("forward_map", x, n, p, int(tsm_segments), int(tsm_div), fmap, feat, 2048, ws, need)
        return fmap, feat

    def profile(self, patches_nhwc4, tsm_segments=0, tsm_div=8):
        """One forward bracketed by HIP events per launch.  Returns a list of dicts
        {ms, flops, bytes, tile} (flops = 0 for the pooling launches)."""
        x = patches_nhwc4.contiguous()
        n, p = x.shape[0], x.shape[1]
        out = torch.empty((n, 2048), device=x.device, dtype=torch.float32)
        ws, need = self._workspace(n, p)
        k = self.n_launches = self._lib.adaf_resnet50_launch_count(self._net)
        ms = (C.c_float * k)()
        fl = (C.c_double * k)()
        by = (C.c_double * k)()
        tl = (C.c_int * k)(*([-1] * k))
        self._call("forward_profiled", x, n, p, int(tsm_segments), int(tsm_div), out, 2048, ws, need, L.stream_ptr(), ms, fl, by, tl,
                   stream=False)       # (the one call whose stream is not its last argument)
        return [dict(ms=ms[i], flops=fl[i], bytes=by[i], tile=tl[i]) for i in range(k) if tl[i] != -1]

    def set_fusion(self, on):
        """Stage-1 conv2 -> conv3 (-> next conv1) and stem + max-pool as single launches (default on; bit-identical)."""
        self._call("set_fusion", int(on), stream=False)   # 2 = also the fused stem where it does not pay (tests)

    def set_shift_place(self, place):
        """'blockres' (default: the shift inside every Bottleneck conv1's operand load) or 'block' (the shift in front of the whole
        Bottleneck: conv1, downsample and identity read the shifted map) -- STH/ops/temporal_shift.py:99-142."""
        code = {"blockres": 0, "block": 1}[place]
        self._call("set_shift_place", code, stream=False)

    def set_latency_rows(self, rows):
        """Convs whose GEMM has at most `rows` rows take the small-batch form (conv_lat.hip; bit-identical); 0 = never, < 0 = default."""
        self._call("set_latency_rows", int(rows), stream=False)

    def set_tiles(self, tiles):
        arr = (C.c_int * len(tiles))(*tiles)
        self._call("set_tiles", arr, len(tiles), stream=False)

    def set_math(self, mode):
        """"f32" (default: fp32 MFMA, exact FMA chain), "split_bf16" (opt-in: fp32 operands decomposed into three
        bf16 parts, six bf16 MFMA products per element pair, fp32 accumulate) or "f16" (opt-in: fp16 activations and
        filters on the f16 matrix pipe, fp32 accumulate / BN / residual, one rounding per stored value; the stem and the
        pooled features stay fp32) -- include/adafocus.h ADAF_MATH_*.  Switching into or out of "f16" clears tile overrides."""
        code = {"f32": MATH_F32, "split_bf16": MATH_F32_SPLIT_BF16, "f16": MATH_F16}.get(mode, mode)
        self._call("set_math", int(code), stream=False)


def set_gru_persistent(mode, device=None):
    """GRU scans: 0/False = two launches per step, 1/True = one persistent kernel (default), 2 = persistent kernel via
    hipLaunchCooperativeKernel (include/adafocus.h)."""
    _call("adaf_set_gru_persistent", _current(device), int(mode), stream=False)


def gru_scan_timeouts(device=None):
    """Blocks of persistent GRU scans whose grid barrier timed out since the handle was created (they NaN-poison their
    outputs).  Synchronises the device; 0 = every scan completed normally."""
    n = C.c_uint(0)
    _call("adaf_gru_scan_timeouts", _current(device), C.byref(n), stream=False)
    return int(n.value)


def set_conv_pos_major(on, device=None):
    """k x k convs: position-major tiles with padding-tap skipping on / off (bit-identical; include/adafocus.h)."""
    _call("adaf_set_conv_pos_major", _current(device), int(on), stream=False)


def pack_dw_weight(w_c133):
    """PyTorch depthwise weight [C,1,3,3] -> [3,3,C]."""
    L.need_gpu_f32(w_c133)
    w = w_c133.contiguous()
    c = w.shape[0]
    out = torch.empty((3, 3, c), device=w.device, dtype=torch.float32)
    _call("adaf_pack_dw_weight_f32", w, w, c, out)
    return out


def dwconv3x3_bn_act(x, w_33c, scale, bias, stride=1, act=ACT_RELU6):
    """Depthwise 3x3 (pad 1) + BN affine + activation; x (N,H,W,C) NHWC."""
    L.need_gpu_f32(x, w_33c, scale, bias)
    x = x.contiguous()
    n, hh, ww, c = x.shape
    out = torch.empty((n, (hh - 1) // stride + 1, (ww - 1) // stride + 1, c), device=x.device, dtype=torch.float32)
    _call("adaf_dwconv3x3_bn_act_f32", x, x, n, hh, ww, c, stride, w_33c.contiguous(), scale.contiguous(), bias.contiguous(), act, out)
    return out


def grid_actions(logits, table):
    """(rows, A) logits + (A,2) table -> (idx int64 (rows,), actions fp32 (rows,2)); first-max argmax."""
    L.need_gpu_f32(logits, table)
    logits = logits.contiguous()
    rows, a = logits.shape
    idx = torch.empty((rows,), device=logits.device, dtype=torch.int64)
    act = torch.empty((rows, 2), device=logits.device, dtype=torch.float32)
    _call("adaf_grid_actions_f32", logits, logits, rows, a, table.contiguous(), idx, act)
    return idx, act


def argmax_rows(logits):
    """First-maximum arg-max of every row (ActorCritic.act's `.max(1)[1]`, ACT/models/ppo.py:94) -> int64 (rows,)."""
    L.need_gpu_f32(logits)
    logits = logits.contiguous()
    rows, a = logits.shape
    idx = torch.empty((rows,), device=logits.device, dtype=torch.int64)
    _call("adaf_grid_actions_f32", logits, logits, rows, a, None, idx, None)
    return idx


def gru_seq_forward(x, w_ih, w_hh, b_ih, b_hh, h0=None):
    """nn.GRU(batch_first=True): x (B,T,F), h0 (B,H) or None (= zeros) -> hidden states (B,T,H)."""
    L.need_gpu_f32(x, w_ih, w_hh, b_ih, b_hh, h0)
    b, t, f = x.shape
    x = _gru_x(x)
    hid = w_hh.shape[1]
    ws, ws_bytes = _workspace("adaf_gru_cls_workspace_bytes", x.device, b, t, hid)
    hs = torch.empty((b, t, hid), device=x.device, dtype=torch.float32)
    _call("adaf_gru_seq_forward_f32", x, x, x.stride(1), b, t, f, hid, w_ih.contiguous(), w_hh.contiguous(), b_ih.contiguous(),
          b_hh.contiguous(), _dense(h0), hs, ws, ws_bytes)
    return hs


class MobileNetV2Net(_NetEngine):
    """adaf_mobilenetv2: the glancer's feature extractor on the conv engine + depthwise kernel.
    load(): neutral name ('stem.weight', 'b3.dw.bn.running_var', ...) -> tensor on this device."""
    _ABI = "mobilenetv2"

    def set_fusion(self, on):
        """Expand 1x1 -> depthwise 3x3 in one kernel for the high-resolution blocks (default on)."""
        # bit 0: fused kernels on; bit 2 (value 4): one frame chunk at a time instead of two side by side; bit 3 (value 8):
        # expand -> depthwise kernel + project launch instead of the whole-block kernel of b3 / b5 / b6 (A/B switches)
        self._call("set_fusion", int(on), stream=False)

    def block_forms(self, size, tsm_segments=0, tsm_div=8):
        """The launch form forward() takes per block at size x size frames under the current set_fusion bits and the global option
        "mb_strip" (adaf_mobilenetv2_block_forms: the decision function of the forward itself; launches nothing).  17 ints: [0] the stem +
        block 1 pair, [i] block b<i+1>.  Low nibble: 0 separate launches, 1 tile expand -> depthwise, 2 tile whole block, 3 strip whole
        block, 4 strip expand -> depthwise; second nibble, the temporal shift: 0 none, 1 in the strip loads, 2 in the operand load,
        3 materialised."""
        forms = (C.c_int * 17)()
        self._call("block_forms", int(size), int(tsm_segments), int(tsm_div), forms, 17, stream=False)
        return list(forms)

    def forward(self, frames_nhwc4, tsm_segments=0, tsm_div=8, want_vec=True):
        """(N,S,S,4) -> featmap (N,S/32,S/32,1280) NHWC, featvec (N,1280) or None."""
        L.need_gpu_f32(frames_nhwc4)
        x = frames_nhwc4.contiguous()
        n, s = x.shape[0], x.shape[1]
        fs = s
        for _ in range(5):          # stem + four stride-2 blocks, each a 3x3 / pad 1 / stride 2 window
            fs = (fs - 1) // 2 + 1
        fmap = torch.empty((n, fs, fs, 1280), device=x.device, dtype=torch.float32)
        fvec = torch.empty((n, 1280), device=x.device, dtype=torch.float32) if want_vec else None
        need = self._lib.adaf_mobilenetv2_workspace_bytes(self._net, n, s, int(tsm_segments))
        ws = self._scratch.get(need)     # per stream: consecutive batches' glancer passes may overlap
        self._call("forward", x, n, s, int(tsm_segments), int(tsm_div), fmap, fvec, 1280, ws, need)
        return fmap, fvec


def ingest_u8(clips_hwc_u8, frames, mean, std):
    """Loader tail fused (ACT/ops/transforms.py:305-336,64-77): (B, H, W, T*3) uint8 stacked clips ->
    (B*T, H, W, 4) fp32 normalised pixel-major frames (lane 3 = 0)."""
    if not clips_hwc_u8.is_cuda or clips_hwc_u8.dtype != torch.uint8:
        raise L.AdafError("ingest_u8: a uint8 tensor on the GPU is required")
    L.on_current_device(clips_hwc_u8)
    x = clips_hwc_u8.contiguous()
    b, hh, ww, c = x.shape
    if c != 3 * frames:
        raise ValueError("ingest_u8: last dim %d != 3*frames" % c)
    out = torch.empty((b * frames, hh, ww, 4), device=x.device, dtype=torch.float32)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    _call("adaf_ingest_u8_f32", x, x, b, int(frames), hh, ww, m, s, out)
    return out


def crop_gather_nhwc4(frames_nhwc4, actions, patch, frames_per_action=1, return_coords=False):
    """get_patch from pixel-major (N,H,W,4) frames -> (N,P,P,4)."""
    L.need_gpu_f32(frames_nhwc4, actions)
    x = frames_nhwc4.contiguous()
    actions = actions.contiguous()
    n, hh, ww, _ = x.shape
    p = int(patch)
    out = torch.empty((n, p, p, 4), device=x.device, dtype=torch.float32)
    coords = torch.empty((actions.shape[0], 2), device=x.device, dtype=torch.int32) if return_coords else None
    _call("adaf_crop_gather_nhwc4_f32", x, x, n, hh, ww, actions, actions.shape[0], int(frames_per_action), p, out, coords)
    return (out, coords) if return_coords else out


def _out_shape(n, c, oh, ow, layout):
    return {LAYOUT_NCHW: (n, c, oh, ow), LAYOUT_NHWC: (n, oh, ow, c), LAYOUT_NHWC4: (n, oh, ow, 4)}[layout]


def crop_resize(frames, actions, patch, size=None, frames_per_action=1, layout=LAYOUT_NCHW, return_coords=False):
    """(y, x, size) -> patch x patch: window of `size` pixels at floor(action * (H - size)), bilinear (align_corners=False)
    resample to patch x patch (include/adafocus.h adaf_crop_resize_f32).  frames (N,3,H,W) planar or (N,H,W,4) pixel-major;
    size: None (= patch: the plain gather), an int, or an int32 tensor (M,) of per-action sizes."""
    L.need_gpu_f32(frames, actions)
    frames = frames.contiguous()
    actions = actions.contiguous()
    in_layout, n, c, hh, ww = _frame_geometry(frames)
    p = int(patch)
    sizes, sdef = None, p
    if isinstance(size, torch.Tensor):
        if size.dtype != torch.int32 or not size.is_cuda or size.numel() != actions.shape[0]:
            raise ValueError("crop_resize: per-action sizes must be an int32 GPU tensor of shape (n_actions,)")
        sizes = size.contiguous()
    elif size is not None:
        sdef = int(size)
    out = torch.empty(_out_shape(n, c, p, p, layout), device=frames.device, dtype=torch.float32)
    coords = torch.empty((actions.shape[0], 2), device=frames.device, dtype=torch.int32) if return_coords else None
    _call("adaf_crop_resize_f32", frames, frames, in_layout, n, c, hh, ww, actions, actions.shape[0], int(frames_per_action), sizes, sdef, p, out,
          layout, coords)
    return (out, coords) if return_coords else out


def resize_nearest(frames, out_hw, layout=LAYOUT_NCHW):
    """F.interpolate(frames, out_hw) with the default nearest mode (ACT/main_dist.py:331-332), bit-exact.
    frames (N,C,H,W) planar or (N,H,W,4) pixel-major -> `layout`."""
    L.need_gpu_f32(frames)
    frames = frames.contiguous()
    in_layout, n, c, hh, ww = _frame_geometry(frames)
    oh, ow = (int(out_hw), int(out_hw)) if isinstance(out_hw, int) else (int(out_hw[0]), int(out_hw[1]))
    out = torch.empty(_out_shape(n, c, oh, ow, layout), device=frames.device, dtype=torch.float32)
    _call("adaf_resize_nearest_f32", frames, frames, in_layout, n, c, hh, ww, oh, ow, out, layout)
    return out


# ---- N2: half-precision storage ---------------------------------------------------------------------------------
def cast(x, dtype):
    """fp32 <-> fp16 element-wise conversion on the HIP side (round-to-nearest-even)."""
    L.need_gpu(x)
    x = x.contiguous()
    to16 = dtype == torch.float16
    if x.dtype not in (torch.float32, torch.float16) or (x.dtype == torch.float16) == to16:
        raise ValueError("cast: fp32 -> fp16 or fp16 -> fp32")
    out = torch.empty(x.shape, device=x.device, dtype=dtype)
    _call("adaf_cast_f32_f16", x, x, x.numel(), out, 1 if to16 else 0)
    return out


def pack_conv_weight_f16(w_oihw, cin_pad=None):
    """OIHW fp32 -> OHWI fp16 (input channels zero-padded to a multiple of 8)."""
    L.need_gpu_f32(w_oihw)
    w = w_oihw.contiguous()
    co, ci, kh, kw = w.shape
    cp = cin_pad or ((ci + 7) // 8 * 8)
    out = torch.empty((co, kh, kw, cp), device=w.device, dtype=torch.float16)
    _call("adaf_pack_conv_weight_f16", w, w, co, ci, kh, kw, cp, out)
    return out


def conv2d_bn_act_f16(x, w_ohwi, scale=None, bias=None, residual=None, stride=1, pad=0, act=ACT_NONE, out_dtype=torch.float16,
                      tile=0, tsm_segments=0, tsm_div=8):
    """adaf_conv2d_bn_act_f16: x (N,H,W,Cin) fp16 with fp16 weights (or fp32 x / w with an fp16 store), fp32 accumulate and
    epilogue, `out_dtype` store.  `tsm_segments` > 0: the temporal shift fused into a 1x1 conv's operand load, as conv2d_bn_act
    (fp16 operands move whole 16-byte chunks: cin / tsm_div a multiple of 8)."""
    L.need_gpu(x, w_ohwi, scale, bias, residual)
    x = x.contiguous()
    w_ohwi = w_ohwi.contiguous()
    if x.dtype != w_ohwi.dtype:
        raise ValueError("conv2d_bn_act_f16: x and w must share a dtype")
    n, hh, ww, cin = x.shape
    cout, kh, kw, cin_w = w_ohwi.shape
    if cin_w != cin:
        raise ValueError("conv2d_bn_act_f16: x has %d channels, weight expects %d" % (cin, cin_w))
    oh = (hh + 2 * pad - kh) // stride + 1
    ow = (ww + 2 * pad - kw) // stride + 1
    out = torch.empty((n, oh, ow, cout), device=x.device, dtype=out_dtype)
    if residual is not None:
        if residual.dtype != torch.float16:
            raise ValueError("conv2d_bn_act_f16: the residual is fp16")
        residual = residual.contiguous()
    p = L.ConvParams(n=n, h=hh, w=ww, cin=cin, cout=cout, kh=kh, kw=kw, stride=stride, pad=pad, act=act, tsm_segments=int(tsm_segments),
                     tsm_div=int(tsm_div), ldx=0, ldo=0, ldr=0, tile=tile)
    _call("adaf_conv2d_bn_act_f16", x, C.byref(p), x, DTYPE_F16 if x.dtype == torch.float16 else DTYPE_F32, w_ohwi, scale, bias, residual, out,
          DTYPE_F16 if out_dtype == torch.float16 else DTYPE_F32)
    return out


def dwconv3x3_bn_act_f16(x, w_33c, scale, bias, stride=1, act=ACT_RELU6):
    """Depthwise 3x3 on fp16 activations (N,H,W,C); taps, BN affine and the sum in fp32."""
    L.need_gpu(x, w_33c, scale, bias)
    if x.dtype != torch.float16:
        raise ValueError("dwconv3x3_bn_act_f16: fp16 activations expected")
    x = x.contiguous()
    n, hh, ww, c = x.shape
    out = torch.empty((n, (hh - 1) // stride + 1, (ww - 1) // stride + 1, c), device=x.device, dtype=torch.float16)
    _call("adaf_dwconv3x3_bn_act_f16", x, x, n, hh, ww, c, stride, w_33c.contiguous(), scale.contiguous(), bias.contiguous(), act, out)
    return out


# ---- EfficientNet building blocks and network (BASELINE config 5; parity unpinned -- see include/adafocus.h) ------------
def _dt(t):
    if t.dtype == torch.float16:
        return DTYPE_F16
    if t.dtype == torch.float32:
        return DTYPE_F32
    raise L.AdafError("adafocus_amd: fp32 or fp16 storage expected, got %s" % t.dtype)


def pack_dw_weight_kxk(w_c1kk):
    """PyTorch depthwise filter (C,1,K,K) -> (K*K, C)."""
    L.need_gpu_f32(w_c1kk)
    w = w_c1kk.contiguous()
    c, k = w.shape[0], w.shape[-1]
    out = torch.empty((k * k, c), device=w.device, dtype=torch.float32)
    _call("adaf_pack_dw_weight_kxk_f32", w, w, c, k, out)
    return out


def dwconv_same_bn_act(x, w_kkc, scale, bias, k, stride=1, act=ACT_SWISH, want_pool=False):
    """Depthwise k x k with TensorFlow-SAME padding + BN affine + activation.  x (N,H,W,C) fp32 | fp16 NHWC ->
    (N,ceil(H/s),ceil(W/s),C) in x's dtype [, squeeze mean (N,C) fp32]."""
    L.need_gpu(x)
    L.need_gpu_f32(w_kkc, scale, bias)
    x = x.contiguous()
    n, hh, ww, c = x.shape
    oh, ow = -(-hh // stride), -(-ww // stride)
    out = torch.empty((n, oh, ow, c), device=x.device, dtype=x.dtype)
    pool, ws, need = None, None, 0
    if want_pool:
        pool = torch.empty((n, c), device=x.device, dtype=torch.float32)
        ws, need = _workspace("adaf_dwconv_same_workspace_bytes", x.device, n, hh, ww, c, int(k), int(stride), _dt(x))
    _call("adaf_dwconv_same_bn_act", x, x, _dt(x), n, hh, ww, c, int(k), int(stride), w_kkc.contiguous(), scale.contiguous(), bias.contiguous(),
          int(act), out, pool, ws, need)
    return (out, pool) if want_pool else out


def se_gate(pool_mean, w_reduce, b_reduce, w_expand, b_expand):
    """sigmoid(W_e swish(W_r m + b_r) + b_e): pool_mean (N,C), W_r (SQ,C), W_e (C,SQ) -> gate (N,C)."""
    L.need_gpu_f32(pool_mean, w_reduce, b_reduce, w_expand, b_expand)
    n, c = pool_mean.shape
    sq = w_reduce.shape[0]
    gate = torch.empty((n, c), device=pool_mean.device, dtype=torch.float32)
    _call("adaf_se_gate_f32", pool_mean, pool_mean.contiguous(), n, c, w_reduce.reshape(sq, c).contiguous(), b_reduce.contiguous(), sq,
          w_expand.reshape(c, sq).contiguous(), b_expand.contiguous(), gate)
    return gate


def conv1x1_gated_bn(x, gate, w, scale=None, bias=None, residual=None):
    """x (N,H,W,Cin) fp32 | fp16, gate (N,Cin) fp32 or None, w (Cout,Cin) in x's dtype -> (N,H,W,Cout) in x's dtype."""
    L.need_gpu(x, w)
    x = x.contiguous()
    n, hh, ww, cin = x.shape
    cout = w.shape[0]
    if w.dtype != x.dtype or (residual is not None and residual.dtype != x.dtype):
        raise L.AdafError("conv1x1_gated_bn: w / residual must have x's dtype")
    out = torch.empty((n, hh, ww, cout), device=x.device, dtype=x.dtype)
    _call("adaf_conv1x1_gated_bn", x, x, _dt(x), n, hh * ww, cin, _dense(gate), w.reshape(cout, cin).contiguous(), cout, _dense(scale),
          _dense(bias), _dense(residual), out)
    return out


class EffNetNet(_NetEngine):
    """adaf_effnet: EfficientNet feature extractor (MBConv + squeeze-and-excite + swish; csrc/effnet_net.hip)."""
    _ABI = "effnet"

    def __init__(self, device, width, depth):
        super().__init__(device, float(width), float(depth))
        self.feature_dim = self._lib.adaf_effnet_feature_dim(self._net)
        self.dtype = DTYPE_F32
        self.pad_size = 0          # default image size the SAME padding is computed for (0 = the input's own); the owner sets it

    def blocks(self):
        out = []
        for i in range(self._lib.adaf_effnet_block_count(self._net)):
            info = (C.c_int * 8)()
            self._call("block_info", i, info, stream=False)
            out.append(dict(zip(("k", "stride", "expand", "cin", "cout", "hid", "sq", "stem"), list(info))))
        return out

    def set_dtype(self, dtype):
        code = {"f32": DTYPE_F32, "f16": DTYPE_F16}.get(dtype, dtype)
        self._call("set_dtype", int(code), stream=False)
        self.dtype = int(code)

    def set_fusion(self, on):
        """fp16 storage: whole-image MBConv kernels for the stride-1 blocks on maps up to 9 x 9 (default on); off = the four-launch plan."""
        self._call("set_fusion", int(bool(on)), stream=False)

    def whole_blocks(self, size, pad_size=None):
        """MBConv blocks of a forward at this input size that run as one launch each (csrc/mbconv_whole.hip)."""
        return int(self._lib.adaf_effnet_whole_blocks(self._net, int(size), int(self.pad_size if pad_size is None else pad_size)))

    def fused_expand_blocks(self, size, pad_size=None):
        """MBConv blocks of a forward at this input size whose expand conv runs inside the depthwise launch (fp16 storage; effnet_kernels.hip XN > 0)."""
        return int(self._lib.adaf_effnet_fused_expand_blocks(self._net, int(size), int(self.pad_size if pad_size is None else pad_size)))

    @staticmethod
    def _same_size(size, pad_size, blocks):
        """Map size after the stem (3 x 3, stride 2) and `blocks` for an input of `size`: every layer pads as TensorFlow-SAME would for
        an image of pad_size (0 = size), whose own size shrinks by ceil(. / stride) alongside."""
        hw, ps = size, pad_size or size
        for k, s in [(3, 2)] + [(b["k"], b["stride"]) for b in blocks]:
            tot = max((-(-ps // s) - 1) * s + k - ps, 0)
            hw, ps = (hw + tot - k) // s + 1, -(-ps // s)
        return hw

    def out_size(self, size, pad_size=0):
        """Spatial size of the feature map for an input of `size` (SAME padding computed for pad_size or size)."""
        return self._same_size(size, pad_size, self.blocks())

    def forward(self, frames_nhwc4, pad_size=0, want_map=False, want_vec=True, out=None):
        """(N,S,S,4) fp32 -> (featmap (N,s,s,F) fp32 NHWC or None, featvec (N,F) or None).  `out`: write the vector into
        this (N, >= F) fp32 view (row stride = its stride(0))."""
        L.need_gpu_f32(frames_nhwc4)
        x = frames_nhwc4.contiguous()
        n, s = x.shape[0], x.shape[1]
        f = self.feature_dim
        fs = self.out_size(s, pad_size)
        fmap = torch.empty((n, fs, fs, f), device=x.device, dtype=torch.float32) if want_map else None
        fvec, ld = None, f
        if out is not None:
            fvec, ld = out, out.stride(0)
        elif want_vec:
            fvec = torch.empty((n, f), device=x.device, dtype=torch.float32)
        need = self._lib.adaf_effnet_workspace_bytes(self._net, n, s, int(pad_size))
        ws = self._scratch.get(need)
        self._call("forward", x, n, s, int(pad_size), -1, None, fmap, fvec, int(ld), ws, need)
        return fmap, fvec

    def forward_blocks(self, frames_nhwc4, upto, pad_size=None):
        """Output of the first `upto` MBConv blocks (0 = the stem) as (N,h,w,c) in the storage dtype (tests).  pad_size: the image
        size the SAME padding is computed for; None = this engine's default (set by its owner), 0 = the input's own size."""
        L.need_gpu_f32(frames_nhwc4)
        x = frames_nhwc4.contiguous()
        n, s = x.shape[0], x.shape[1]
        pad_size = self.pad_size if pad_size is None else pad_size
        blocks = self.blocks()
        done = blocks[:upto]
        hw = self._same_size(s, pad_size, done)
        c = done[-1]["cout"] if done else blocks[0]["stem"]
        dt = torch.float16 if self.dtype == DTYPE_F16 else torch.float32
        out = torch.empty((n, hw, hw, c), device=x.device, dtype=dt)
        need = self._lib.adaf_effnet_workspace_bytes(self._net, n, s, int(pad_size))
        ws = self._scratch.get(need)
        self._call("forward", x, n, s, int(pad_size), int(upto), out, None, None, 0, ws, need)
        return out
