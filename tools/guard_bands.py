"""Guard-banded operands for the strided / unaligned operand checks of the C ABI (include/adafocus.h).  One implementation, used by
tools/conv_fuzz.py and (through tests/strided.py) by the test suite; plain functions that work on CPU tensors and on the GPU.

A guarded allocation is ONE flat tensor filled with a canary bit pattern (a quiet NaN, so an operand gap that is read poisons the
result) with the operand as a row-strided view inside it.  Everything handed to a kernel lies inside such an allocation with at least
one full row of canaries in front of and behind the view: a store that overruns by less than a row lands in memory the caller owns
and is reported, never in somebody else's."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adafocus_amd import _lib as L  # noqa: E402

CANARY_F32 = 0x7FC0BEEF      # quiet NaN, payload 0x40BEEF
CANARY_F16 = 0x7EAD          # quiet NaN (fp16)

_INT_OF = {torch.float32: torch.int32, torch.float16: torch.int16}
_CANARY = {torch.float32: CANARY_F32, torch.float16: CANARY_F16}


def lead_for(ld, offset=0, rows=1):
    """A lead of at least `rows` full rows that keeps a 16-byte aligned start, plus `offset` elements (1..3 floats: 4-byte but not
    16-byte aligned)."""
    return (rows * ld + 7) // 8 * 8 + offset


def guarded(shape_rows, cols, ld, lead, trail, dtype=torch.float32, device="cpu"):
    """(buf, view): `buf` is one flat allocation of lead + rows * ld + trail elements, every element the canary; `view` has shape
    (*shape_rows, cols), unit inner stride and row stride `ld`, and starts `lead` elements in."""
    if isinstance(shape_rows, int):
        shape_rows = (shape_rows,)
    shape_rows = tuple(int(s) for s in shape_rows)
    rows = 1
    for s in shape_rows:
        rows *= s
    if rows <= 0 or cols <= 0 or ld < cols:
        raise ValueError("guarded: rows, cols > 0 and ld >= cols required")
    if lead < ld or trail < ld:
        raise ValueError("guarded: lead and trail must hold at least one full row (ld = %d)" % ld)
    total = lead + rows * ld + trail
    bits = torch.full((total,), _CANARY[dtype], dtype=torch.int64).to(_INT_OF[dtype]).to(device)
    buf = bits.view(dtype)
    strides, s = [], ld
    for d in reversed(shape_rows):
        strides.insert(0, s)
        s *= d
    view = buf.as_strided(shape_rows + (cols,), tuple(strides) + (1,), lead)
    return buf, view


def _geometry(buf, view):
    if view.dim() < 2 or view.stride(-1) != 1:
        raise ValueError("guard check: a view of guarded() expected")
    cols, ld = view.shape[-1], view.stride(-2)
    rows = view.numel() // cols
    lead = view.storage_offset() - buf.storage_offset()
    return rows, cols, ld, lead


def fill(view, dense):
    """Write the dense (*shape_rows, cols) payload through the stride."""
    view.copy_(dense.reshape(view.shape).to(view.dtype))
    return view


def payload(view):
    """The dense copy of the payload."""
    return view.contiguous().clone()


def find_guard_damage(buf, view):
    """None, or (flat offset, row, column, region) of the first element outside the payload that lost the canary bits.  Row / column
    are relative to the view's first element (the lead has row < 0); region is 'lead', 'gap' or 'trail'."""
    rows, cols, ld, lead = _geometry(buf, view)
    bits = buf.view(_INT_OF[buf.dtype])
    canary = torch.tensor(_CANARY[buf.dtype], dtype=torch.int64).to(bits.dtype).item()
    end = lead + rows * ld
    # segment by segment (lead, the rows with their gaps, trail): no index tensor as long as the allocation (a workspace may hold 100 MB)
    for lo, hi in ((0, lead), (lead, min(end, bits.numel())), (end, bits.numel())):
        if hi <= lo or (lo == lead and ld == cols):
            continue
        bad = bits[lo:hi] != canary
        if lo == lead:
            bad &= (torch.arange(hi - lo, device=bits.device).remainder(ld) >= cols)
        if bool(bad.any()):
            off = lo + int(torch.nonzero(bad)[0].item())
            r, c = divmod(off - lead, ld)
            region = "lead" if off < lead else "trail" if off >= end else "gap"
            return off, r, c, region
    return None


def assert_guards_intact(buf, view, what="buffer"):
    hit = find_guard_damage(buf, view)
    if hit is not None:
        rows, cols, ld, lead = _geometry(buf, view)
        es, end = buf.element_size(), lead + (rows - 1) * ld + cols
        where = ("%d bytes in front of the payload's start" % ((lead - hit[0]) * es) if hit[3] == "lead" else
                 "%d bytes past the payload's end" % ((hit[0] - end) * es) if hit[3] == "trail" else "between two rows")
        raise AssertionError("%s: guard damaged at flat offset %d = (row %d, column %d) in the %s, %s (rows %d, cols %d, ld %d, lead %d)"
                             % ((what,) + hit + (where, rows, cols, ld, lead)))


# ---- caller-owned workspaces ----------------------------------------------------------------------------------------------------------
WS_GUARD_MIN = 1 << 20       # bytes of canary on either side of a workspace, at least


def guarded_workspace(nbytes, device="cpu", fill="nan", offset_bytes=0):
    """(buf, ws) for a workspace of exactly `nbytes` bytes (what a *_workspace_bytes query returned): ONE flat fp32 allocation, `ws` the
    (1, ceil(nbytes / 4))-word payload as a one-row view that starts 256-byte aligned plus `offset_bytes` (a multiple of 4), with
    max(nbytes, 1 MiB) bytes of canary in front of and behind it -- an overrun shorter than the workspace itself lands in memory the
    caller owns.  `fill`: "nan" (the canary: a word that is read before it is written poisons the result), "zero", or a tensor whose
    bytes are copied in (what an earlier call left in its workspace).  Check with find_guard_damage / assert_guards_intact /
    workspace_damage."""
    nbytes, offset_bytes = int(nbytes), int(offset_bytes)
    if nbytes <= 0 or offset_bytes < 0 or offset_bytes % 4:
        raise ValueError("guarded_workspace: nbytes > 0 and a non-negative offset_bytes that is a multiple of 4 required")
    words = (nbytes + 3) // 4
    guard = (max(nbytes, WS_GUARD_MIN) + 3) // 4      # whole words: a size that is no multiple of 4 still gets its full guard
    # room to move the payload's start onto a 256-byte boundary whatever the allocation's own alignment
    # (filled where it lives: a 100 MB workspace is not staged on the host; CANARY_F32 fits a signed 32-bit word)
    bits = torch.full((guard + 64 + offset_bytes // 4 + words + guard,), CANARY_F32, dtype=torch.int32, device=device)
    buf = bits.view(torch.float32)
    lead = guard + (-(buf.data_ptr() + 4 * guard) % 256) // 4 + offset_bytes // 4
    ws = buf.as_strided((1, words), (words, 1), lead)
    if isinstance(fill, torch.Tensor):
        src = fill.detach().contiguous().reshape(-1).view(torch.int32)
        if src.numel() != words:
            raise ValueError("guarded_workspace: the fill holds %d words, the workspace %d" % (src.numel(), words))
        ws.view(torch.int32).copy_(src.reshape(1, words))
    elif fill == "zero":
        ws.zero_()
    elif fill != "nan":
        raise ValueError("guarded_workspace: fill is 'nan', 'zero' or a tensor")
    return buf, ws


def workspace_damage(buf, ws, nbytes=None):
    """None, or a sentence that names the first damaged guard word by its byte offset in front of the workspace's start or past its end
    (the end is `nbytes`, else the payload's whole words)."""
    hit = find_guard_damage(buf, ws)
    if hit is None:
        return None
    off, _, _, region = hit
    lead = ws.storage_offset() - buf.storage_offset()
    end = 4 * ws.shape[-1] if nbytes is None else int(nbytes)
    if region == "lead":
        return "guard word damaged %d bytes in front of the workspace's start (flat offset %d)" % (4 * (lead - off), off)
    return "guard word damaged %d bytes past the workspace's end of %d bytes (flat offset %d)" % (4 * (off - lead) - end, end, off)


def assert_workspace_intact(buf, ws, what="workspace", nbytes=None):
    msg = workspace_damage(buf, ws, nbytes)
    if msg is not None:
        raise AssertionError("%s: %s" % (what, msg))


def is_all_canary(t):
    """Every fp32 word of `t` still holds the canary bits (nothing wrote it)."""
    c = t.contiguous().view(torch.int32)
    return bool((c == torch.tensor(CANARY_F32, dtype=torch.int64).to(torch.int32).item()).all())


# ---- the C ABI with real strides -----------------------------------------------------------------------------------------------------
def _dt(t):
    return L.DTYPE_F16 if t.dtype == torch.float16 else L.DTYPE_F32


def conv_call(kind, x, w, scale, bias, residual, out, stride=1, pad=0, act=L.ACT_NONE, tsm_segments=0, tsm_div=8, tile=0, ld=None):
    """adaf_conv2d_bn_act_f32 ("engine"), adaf_conv2d_naive_f32 ("naive") or adaf_conv2d_bn_act_f16 ("f16") on views: x (N,H,W,Cin),
    out / residual (N,OH,OW,Cout), each with unit channel stride and its pixel stride in stride(-2); pointers are the views' data_ptr().
    `ld` = (ldx, ldo, ldr) overrides the strides read from the views (the refusal tests).  Raises AdafError when the library refuses."""
    n, hh, ww, cin = x.shape
    cout, kh, kw, _ = w.shape
    for t in (x, out, residual):
        if t is not None and t.stride(-1) != 1:
            raise ValueError("conv_call: unit channel stride required")
    ldx, ldo, ldr = ld if ld is not None else (x.stride(-2), out.stride(-2), residual.stride(-2) if residual is not None else 0)
    p = L.ConvParams(n=n, h=hh, w=ww, cin=cin, cout=cout, kh=kh, kw=kw, stride=stride, pad=pad, act=act, tsm_segments=int(tsm_segments),
                     tsm_div=int(tsm_div), ldx=int(ldx), ldo=int(ldo), ldr=int(ldr), tile=int(tile))
    h = L.handle(x.device)
    lib = L.load_library()
    if kind == "f16":
        rc = lib.adaf_conv2d_bn_act_f16(h, C.byref(p), L.ptr(x), _dt(x), L.ptr(w), L.ptr(scale), L.ptr(bias), L.ptr(residual), L.ptr(out),
                                        _dt(out), L.stream_ptr())
    else:
        fn = lib.adaf_conv2d_naive_f32 if kind == "naive" else lib.adaf_conv2d_bn_act_f32
        rc = fn(h, C.byref(p), L.ptr(x), L.ptr(w), L.ptr(scale), L.ptr(bias), L.ptr(residual), L.ptr(out), L.stream_ptr())
    L.check(rc, h)
    return out
