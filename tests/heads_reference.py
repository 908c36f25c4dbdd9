"""Plain float64 statements, on the CPU, of what the classifier and reward heads compute, the one tolerance rule they are held to, and
the case tables of tests/test_heads_domain_gpu.py (tests/test_heads_reference_host.py checks the references and the tables themselves,
without a GPU).  Not a test module.  Every function takes torch fp32 tensors and a `dtype`: float64 is the reference, float32 the same
expression in ATen's fp32, and the distance between the two is the measure every bound is made of.

THE TOLERANCE RULE.  spread = max |f32 - f64| / max |f64| of one output of one case: what fp32 arithmetic in another summation order
does to this very expression on these very inputs.  A HIP result is compared the same way, err = max |got - f64| / max |f64|, and
  - single products and reductions (linear, segment mean, rewards, cross-entropy):  err <= max(FLOOR, 8 x spread),
    FLOOR = 2^-22 and the factor 8 as in tests/test_stage2_rollout_gpu.py::_tolerances;
  - recurrences and their gradients (GRU forward, training forward, backward):      err <= 50 x spread,
    the G17 rule of tests/test_stage3_gpu.py;
  - moves and arg-max are exact.
Both factors exist because the HIP kernels sum in another order than ATen does; neither they nor any other constant in this file was
chosen from a kernel's output.  An output whose float64 reference is all zeros (the cross-entropy of a single class) has no largest
entry to be relative to and is compared absolutely (scale 1)."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from adafocus_amd import synth
from tests.helpers import rnd

FLOOR = 2.0 ** -22
SINGLE_FACTOR = 8.0
RECURRENCE_FACTOR = 50.0

GRU_KEYS = ("gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0")
CLS_KEYS = GRU_KEYS + ("fc.weight", "fc.bias")


# ---- the operations -----------------------------------------------------------------------------------------------------------------------
def linear(x, weight, bias=None, dtype=torch.float64):
    """nn.Linear: x (rows, in), weight (out, in) -> (rows, out)."""
    y = x.to(dtype) @ weight.to(dtype).t()
    return y if bias is None else y + bias.to(dtype)


def gru_seq(x, w_ih, w_hh, b_ih, b_hh, h0=None, dtype=torch.float64):
    """nn.GRU(batch_first=True) written out gate by gate in PyTorch's (r, z, n) order: x (B, T, F), h0 (B, H) or None (zeros) ->
    hidden states (B, T, H).
        r = s(W_ir x + b_ir + W_hr h + b_hr),  z = s(W_iz x + b_iz + W_hz h + b_hz),  n = tanh(W_in x + b_in + r (W_hn h + b_hn)),
        h' = (1 - z) n + z h"""
    x, w_ih, w_hh, b_ih, b_hh = (v.to(dtype) for v in (x, w_ih, w_hh, b_ih, b_hh))
    b, t, _ = x.shape
    hid = w_hh.shape[1]
    h = torch.zeros(b, hid, dtype=dtype) if h0 is None else h0.to(dtype)
    out = []
    for s in range(t):
        gi = x[:, s] @ w_ih.t() + b_ih
        gh = h @ w_hh.t() + b_hh
        i_r, i_z, i_n = gi[:, :hid], gi[:, hid:2 * hid], gi[:, 2 * hid:]
        h_r, h_z, h_n = gh[:, :hid], gh[:, hid:2 * hid], gh[:, 2 * hid:]
        r = torch.sigmoid(i_r + h_r)
        z = torch.sigmoid(i_z + h_z)
        n = torch.tanh(i_n + r * h_n)
        h = (1 - z) * n + z * h
        out.append(h)
    return torch.stack(out, 1)


def gru_cls(x, params, mask=None, dtype=torch.float64):
    """RecurrentClassifier: GRU -> (* mask, the dropout multipliers (B, T, H)) -> Linear on every step.  params in CLS_KEYS order ->
    logits (B*T, C), rows b * T + t."""
    hs = gru_seq(x, *params[:4], dtype=dtype)
    if mask is not None:
        hs = hs * mask.to(dtype)
    return linear(hs.reshape(-1, hs.shape[-1]), params[4], params[5], dtype)


def gru_cls_grads(x, params, mask, dlogits, dtype=torch.float64):
    """Autograd through gru_cls: -> {"logits", "dx", one entry per CLS_KEYS name} for the upstream gradient dlogits (B*T, C)."""
    xs = x.to(dtype).clone().requires_grad_(True)
    ps = [p.to(dtype).clone().requires_grad_(True) for p in params]
    logits = gru_cls(xs, ps, mask, dtype)
    logits.backward(dlogits.to(dtype))
    out = {"logits": logits.detach(), "dx": xs.grad}
    out.update({k: p.grad for k, p in zip(CLS_KEYS, ps)})
    return out


def segment_mean(feat, batch, fc_w, fc_b, global_logit=None, dtype=torch.float64):
    """mean_t FC(f_t) (+ mean over the Tg global logits, Tg need not equal T): feat (B*T, F), global_logit (B, Tg, C) -> (B, C)."""
    logit = linear(feat, fc_w, fc_b, dtype).reshape(batch, -1, fc_w.shape[0])
    out = logit.mean(1)
    return out if global_logit is None else out + global_logit.to(dtype).mean(1)


def confidences(logits_rows, target, steps, dtype=torch.float64):
    """Softmax probability of the clip's target class at every step: logits (B*T, C) rows b * T + t, target (B,) -> (T, B)."""
    b = target.numel()
    p = F.softmax(logits_rows.to(dtype), 1).reshape(b, steps, -1)
    return torch.gather(p, 2, target.view(b, 1, 1).expand(b, steps, 1)).squeeze(2).t().contiguous()


def rewards(logits_rows, base_rows, target, steps, kind, dtype=torch.float64):
    """The three reward kinds from the confidences: 'prev' conf_t - conf_{t-1} (conf_{-1} = 0), 'conf' conf_t, 'random' conf_t - the
    baseline's conf_t  -> (rewards (T, B), confidences (T, B))."""
    conf = confidences(logits_rows, target, steps, dtype)
    if kind == "prev":
        return conf - torch.cat([torch.zeros_like(conf[:1]), conf[:-1]], 0), conf
    if kind == "conf":
        return conf, conf
    if kind == "random":
        return conf - confidences(base_rows, target, steps, dtype), conf
    raise ValueError(kind)


def ce_last(logits_rows, target, steps, dtype=torch.float64):
    """Mean cross-entropy of the last step's rows."""
    b = target.numel()
    return F.cross_entropy(logits_rows.to(dtype).reshape(b, steps, -1)[:, -1], target).reshape(1)


def argmax_first(logits):
    """First-maximum arg-max of every row (numpy.argmax's rule) -> int64 numpy (rows,)."""
    return np.argmax(logits.detach().cpu().numpy(), axis=1).astype(np.int64)


# ---- the tolerance rule ---------------------------------------------------------------------------------------------------------------------
Ref = collections.namedtuple("Ref", "ref spread scale")       # dicts by output name: fp64 tensor, relative spread, max |fp64| (0 -> 1)


def measure(fn, scale_of=None):
    """fn(dtype) -> {name: tensor}, evaluated in fp32 and fp64 -> Ref.  `scale_of` maps an output's name to the name of the output
    whose largest entry it is relative to (the rewards are differences of confidences: relative to the confidences)."""
    r32, r64 = fn(torch.float32), fn(torch.float64)
    ref = {k: v.detach() for k, v in r64.items()}
    scale = {k: float(v.abs().max()) for k, v in ref.items()}
    scale = {k: scale[(scale_of or {}).get(k, k)] or 1.0 for k in ref}
    spread = {k: float((r32[k].detach().double() - ref[k]).abs().max()) / scale[k] for k in ref}
    return Ref(ref, spread, scale)


def rel_err(got, r, name):
    """max |got - f64| / the output's scale."""
    return float((got.detach().cpu().double().reshape(r.ref[name].shape) - r.ref[name]).abs().max()) / r.scale[name]


def bound_single(spread):
    return max(FLOOR, SINGLE_FACTOR * spread)


def bound_recurrence(spread):
    return RECURRENCE_FACTOR * spread


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------
def _params(shapes, seed):
    return {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, seed).items()}


def cls_params(f, h, c, seed):
    """The six RecurrentClassifier parameters in CLS_KEYS order."""
    sd = _params({"gru.weight_ih_l0": (3 * h, f), "gru.weight_hh_l0": (3 * h, h), "gru.bias_ih_l0": (3 * h,), "gru.bias_hh_l0": (3 * h,),
                  "fc.weight": (c, h), "fc.bias": (c,)}, seed)
    return tuple(sd[k] for k in CLS_KEYS)


def dropout_mask(b, t, h, seed, p=0.5):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.random((b, t, h)) >= p).astype(np.float32) / np.float32(1 - p))


# ---- linear: every dataset's class count on the shapes of the glancer / focuser / GRU fall-back FCs ---------------------------------------------
LINEAR_CLASSES = (1, 27, 49, 101, 239, 1001)
LINEAR_SHAPES = ((1280, 1), (2048, 16), (1024, 37), (2048, 128), (2048, 129))            # (in, rows)
LINEAR_CASES = [(c, fin, rows) for c in LINEAR_CLASSES for fin, rows in LINEAR_SHAPES]


@functools.lru_cache(maxsize=None)
def linear_case(c, fin, rows):
    """-> ((x, w, b), Ref with output 'y')."""
    sd = _params({"fc.weight": (c, fin), "fc.bias": (c,)}, 3000 + c)
    args = (rnd((rows, fin), 3100 + rows), sd["fc.weight"], sd["fc.bias"])
    return args, measure(lambda dt: {"y": linear(*args, dtype=dt)})


# ---- GRU forward: class folding, batch slices, barrier layouts, hidden and feature widths ----------------------------------------------------
GruCase = collections.namedtuple("GruCase", "b t f h c")
GRU_CLASS_CASES = [GruCase(5, 3, 64, 1024, c) for c in (1, 27, 128, 129, 239, 1000, 1024, 1025)]
GRU_BATCH_CASES = [GruCase(b, 2, 64, 1024, 239) for b in (32, 33, 129, 256, 257)]
GRU_BARRIER_CASES = [GruCase(1, t, 64, 1024, 27) for t in (10, 11, 179, 180)]          # padded | packed | packed (last) | flat (first)
GRU_HIDDEN_CASES = [GruCase(5, 3, 64, h, 239) for h in (256, 1028)]
GRU_FEATURE_CASES = [GruCase(5, 3, f, 1024, 239) for f in (3328, 2816)]
GRU_CASES = GRU_CLASS_CASES + GRU_BATCH_CASES + GRU_BARRIER_CASES + GRU_HIDDEN_CASES + GRU_FEATURE_CASES


def gru_case_id(k):
    return "B%d-T%d-F%d-H%d-C%d" % k


def barrier_layout(b, t, h=1024, groups=1):
    """The record layout adaf_gru_scan_plan gives a scan of one slice (csrc/gru_scan.hip): the barrier words are the 3 H B floats of the
    per-step product buffer; 17-word records at a 16-word pitch when they fit, packed when those fit, else one counter per step."""
    words, recs = 3 * h * b, 17 * groups * (t + 1)
    return "padded" if 16 * recs <= words else "packed" if recs <= words else "flat"


@functools.lru_cache(maxsize=None)
def gru_case(k):
    """-> ((x, h0, params), Ref with outputs 'logits' (h0 = 0, with the FC) and 'hs_h0' (the hidden states from h0))."""
    x = rnd((k.b, k.t, k.f), 4000 + k.b + k.t, 0.5)
    h0 = rnd((k.b, k.h), 4100 + k.b, 0.5)
    params = cls_params(k.f, k.h, k.c, 4200 + k.c + k.h)
    return (x, h0, params), measure(lambda dt: {"logits": gru_cls(x, params, None, dt), "hs_h0": gru_seq(x, *params[:4], h0=h0, dtype=dt)})


# ---- stage 3: training forward + backward ------------------------------------------------------------------------------------------------------
Stage3Case = collections.namedtuple("Stage3Case", "b t h c")
STAGE3_F = 64
STAGE3_CASES = [Stage3Case(5, 3, 1024, 27), Stage3Case(129, 2, 1024, 239), Stage3Case(256, 2, 1024, 239), Stage3Case(257, 2, 1024, 239),
                Stage3Case(6, 3, 16, 239), Stage3Case(6, 3, 1040, 101)]
STAGE3_OUTPUTS = ("logits", "dx") + CLS_KEYS


@functools.lru_cache(maxsize=None)
def stage3_case(k):
    """-> ((x, params, mask, dlogits), Ref with the outputs STAGE3_OUTPUTS)."""
    x = rnd((k.b, k.t, STAGE3_F), 5000 + k.b, 0.5)
    params = cls_params(STAGE3_F, k.h, k.c, 5100 + k.h + k.c)
    mask = dropout_mask(k.b, k.t, k.h, 5200 + k.b)
    dlogits = rnd((k.b * k.t, k.c), 5300 + k.c)
    return (x, params, mask, dlogits), measure(lambda dt: gru_cls_grads(x, params, mask, dlogits, dt))


# ---- FC + segment mean (Something-Something: Tg = 8 global logits beside Tf = 12 focus steps) ---------------------------------------------------
MEANPOOL_B, MEANPOOL_F = 5, 64
MEANPOOL_CASES = [(c, t, tg, glob) for c in (27, 174, 239) for t, tg in ((1, 1), (12, 8), (8, 12)) for glob in (False, True)]


@functools.lru_cache(maxsize=None)
def meanpool_case(c, t, tg, glob):
    """-> ((feat, fc_w, fc_b, global_logit or None), Ref with output 'out')."""
    sd = _params({"fc.weight": (c, MEANPOOL_F), "fc.bias": (c,)}, 6000 + c)
    feat = rnd((MEANPOOL_B * t, MEANPOOL_F), 6100 + t)
    glog = rnd((MEANPOOL_B, tg, c), 6200 + tg + c) if glob else None
    args = (feat, sd["fc.weight"], sd["fc.bias"], glog)
    return args, measure(lambda dt: {"out": segment_mean(feat, MEANPOOL_B, sd["fc.weight"], sd["fc.bias"], glog, dt)})


# ---- rewards and the last step's cross-entropy ---------------------------------------------------------------------------------------------------
REWARD_T = 3
REWARD_KINDS = ("prev", "conf", "random")
REWARD_CASES = [(c, b) for c in (1, 27, 63, 64, 65, 239, 1000) for b in (1, 255, 256, 257)]
SATURATED = 60.0          # a logit this far above the rest: the softmax is 1 in fp32 and in fp64 to 1e-20


def reward_inputs(c, b):
    """logits, base (B*T, C) rows b * T + t, target (B,).  Clip 0: step 0 uniform (all logits equal), step 1 saturated on its target
    C - 1, step 2 spread.  Clip 1 (B >= 2): saturated at every step, target 0.  Clip 2 (B >= 3): uniform at every step.  The rest:
    spread logits, targets drawn over all classes."""
    t = REWARD_T
    logits = rnd((b, t, c), 7000 + c + b, 3.0)
    base = rnd((b, t, c), 7100 + c + b, 3.0)
    target = torch.from_numpy(np.random.Generator(np.random.PCG64(7200 + c + b)).integers(0, c, size=b))
    target[0] = c - 1
    logits[0, 0] = 0.25
    logits[0, 1, c - 1] = SATURATED
    if b >= 2:
        target[1] = 0
        logits[1, :, 0] = SATURATED
    if b >= 3:
        logits[2] = -1.5
    return logits.reshape(b * t, c), base.reshape(b * t, c), target


@functools.lru_cache(maxsize=None)
def reward_case(c, b):
    """-> ((logits, base, target), Ref with outputs 'conf', 'ce' and one 'r_<kind>' per kind; the rewards are relative to the
    confidences, whose differences they are)."""
    logits, base, target = reward_inputs(c, b)

    def fn(dt):
        out = {"conf": confidences(logits, target, REWARD_T, dt), "ce": ce_last(logits, target, REWARD_T, dt)}
        for kind in REWARD_KINDS:
            out["r_" + kind] = rewards(logits, base, target, REWARD_T, kind, dt)[0]
        return out
    return (logits, base, target), measure(fn, scale_of={"r_" + kind: "conf" for kind in REWARD_KINDS})


# ---- arg-max / table lookup, row transpose (exact) -----------------------------------------------------------------------------------------------
ARGMAX_CASES = [(a, rows) for a in (1, 25, 36, 49, 64) for rows in (1, 257)]


def argmax_inputs(a, rows):
    """logits (rows, A) on a grid of 0.5 (ties everywhere) and a table (A, 2) of distinct rows.  Row r by r % 8:  1: all equal,
    2: +inf twice (the first wins), 3: all -inf, 4: -inf everywhere but two equal entries, 5: the maximum first and last; the others as
    drawn.  A single row (rows = 1) gets its maximum twice."""
    g = np.random.Generator(np.random.PCG64([8000 + a, rows]))
    x = np.round(g.standard_normal((rows, a)).astype(np.float32) * 2) / 2
    for r in range(rows):
        m = r % 8 if rows > 1 else 5
        lo, hi = g.integers(0, a), g.integers(0, a)
        if m == 1:
            x[r] = x[r, 0]
        elif m == 2:
            x[r, lo] = x[r, hi] = np.inf
        elif m == 3:
            x[r] = -np.inf
        elif m == 4:
            v = x[r, lo]
            x[r] = -np.inf
            x[r, lo] = x[r, hi] = v
        elif m == 5:
            x[r, 0] = x[r, a - 1] = x[r].max() + 1
    table = g.permutation(2 * a).astype(np.float32).reshape(a, 2) / np.float32(2 * a)
    return torch.from_numpy(x), torch.from_numpy(table)


TRANSPOSE_CASES = [(1, 5, 4), (3, 5, 1280), (16, 64, 12)]           # (ni, nj, width)
