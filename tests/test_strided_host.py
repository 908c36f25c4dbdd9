"""The checker is checked first: the guard-band helpers and the float64 conv reference of tests/strided.py on CPU tensors (no GPU)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import strided as S


def _gen(seed):
    return np.random.Generator(np.random.PCG64([seed, 0x57D]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_guarded_buffer_is_all_canary_and_passes(dtype):
    ld = 24
    buf, view = S.guarded((3, 5), 13, ld, S.lead_for(ld, 3), 2 * ld, dtype)
    assert buf.dim() == 1 and buf.numel() == S.lead_for(ld, 3) + 15 * ld + 2 * ld
    assert view.shape == (3, 5, 13) and view.stride() == (5 * ld, ld, 1) and view.dtype == dtype
    assert view.storage_offset() == S.lead_for(ld, 3) and view.data_ptr() == buf.data_ptr() + S.lead_for(ld, 3) * buf.element_size()
    assert torch.isnan(buf).all()                                  # a gap that is read poisons the result
    bits = buf.view(torch.int32 if dtype == torch.float32 else torch.int16)
    assert int(bits[0]) == (S.CANARY_F32 if dtype == torch.float32 else S.CANARY_F16)
    S.assert_guards_intact(buf, view)
    view.fill_(1.0)                                                # the whole payload may change
    S.assert_guards_intact(buf, view)
    assert S.find_guard_damage(buf, view) is None


def test_guarded_refuses_a_guard_band_shorter_than_a_row():
    with pytest.raises(ValueError):
        S.guarded(4, 8, 12, 11, 12)
    with pytest.raises(ValueError):
        S.guarded(4, 8, 12, 12, 11)
    with pytest.raises(ValueError):
        S.guarded(4, 8, 7, 12, 12)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_damaged_guard_is_reported_at_the_right_offset(dtype):
    rows, cols, ld = 6, 10, 16
    lead, trail = S.lead_for(ld, 1), ld + 5
    spots = {
        "gap": (lead + 2 * ld + cols + 3, 2, cols + 3),            # one element in the gap of row 2
        "gap0": (lead + 4 * ld + cols, 4, cols),                   # ... the first gap element right behind a row's payload
        "lead": (lead - 1, -1, ld - 1),                            # ... the element right in front of the view
        "lead_first": (0, -2, 2 * ld - lead),                      # ... the very first element of the allocation
        "trail": (lead + rows * ld + 2, rows, 2),                  # ... in the trail
        "trail_last": (lead + rows * ld + trail - 1, rows + (trail - 1) // ld, (trail - 1) % ld),
    }
    for name, (off, r, c) in spots.items():
        buf, view = S.guarded(rows, cols, ld, lead, trail, dtype)
        view.fill_(0.5)
        buf[off] = 7.0
        region = "gap" if name.startswith("gap") else "lead" if name.startswith("lead") else "trail"
        assert S.find_guard_damage(buf, view) == (off, r, c, region), name
        with pytest.raises(AssertionError) as e:
            S.assert_guards_intact(buf, view, "out")
        assert "flat offset %d = (row %d, column %d)" % (off, r, c) in str(e.value) and region in str(e.value), (name, str(e.value))
    # the FIRST damaged offset is the one named
    buf, view = S.guarded(rows, cols, ld, lead, trail, dtype)
    buf[lead + 5 * ld + cols + 1] = 1.0
    buf[lead + 1 * ld + cols + 2] = 1.0
    assert S.find_guard_damage(buf, view)[:3] == (lead + ld + cols + 2, 1, cols + 2)
    # another NaN is damage too: the check is on the bits, not on the value
    buf, view = S.guarded(rows, cols, ld, lead, trail, dtype)
    buf[lead + cols] = float("nan")
    assert S.find_guard_damage(buf, view) == (lead + cols, 0, cols, "gap")
    # ... and a damaged payload element is not
    buf, view = S.guarded(rows, cols, ld, lead, trail, dtype)
    buf[lead + 3 * ld + cols - 1] = 3.0
    S.assert_guards_intact(buf, view)


def test_strided_view_round_trips():
    g = _gen(1)
    dense = torch.from_numpy(g.standard_normal((2, 3, 4, 12), dtype=np.float32))
    for ld, off in ((12, 0), (20, 0), (17, 3)):
        buf, view = S.guarded((2, 3, 4), 12, ld, S.lead_for(ld, off), ld)
        S.fill(view, dense)
        assert torch.equal(S.payload(view), dense) and S.payload(view).is_contiguous()
        flat = buf[S.lead_for(ld, off):]
        for r in (0, 5, 23):
            assert torch.equal(flat[r * ld:r * ld + 12], dense.reshape(24, 12)[r])        # row r really sits r * ld elements in
        S.assert_guards_intact(buf, view)
        assert torch.isnan(flat[12:ld]).all()


def _epilogue32(y_nchw, scale, bias, res_nhwc, act):
    y = y_nchw.double().permute(0, 2, 3, 1) * scale.double() + bias.double()
    if res_nhwc is not None:
        y = y + res_nhwc.double()
    return {S.ACT_NONE: lambda v: v, S.ACT_RELU: torch.relu, S.ACT_RELU6: lambda v: v.clamp(0, 6), S.ACT_SIGMOID: torch.sigmoid,
            S.ACT_SWISH: lambda v: v * torch.sigmoid(v)}[act](y)


@pytest.mark.parametrize("act", [S.ACT_NONE, S.ACT_RELU, S.ACT_RELU6, S.ACT_SIGMOID, S.ACT_SWISH])
def test_conv_ref64_equals_torch_conv_plus_epilogue_on_a_strided_padded_non_square_case(act):
    g = _gen(2 + act)
    n, h, w, cin, cout, k, stride, pad = 2, 7, 10, 8, 6, 3, 2, 1
    x = torch.from_numpy(g.standard_normal((n, h, w, cin), dtype=np.float32))
    wt = torch.from_numpy(g.standard_normal((cout, k, k, cin), dtype=np.float32) * np.float32(0.2))
    sc = torch.from_numpy(g.uniform(0.5, 1.5, cout).astype(np.float32))
    bi = torch.from_numpy(g.normal(0, 3.0, cout).astype(np.float32))
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    assert (oh, ow) == (4, 5)
    res = torch.from_numpy(g.standard_normal((n, oh, ow, cout), dtype=np.float32))
    # the operands come in through strided, NaN-guarded views: the reference reads the payload only
    _, xv = S.guarded((n, h, w), cin, cin + 12, S.lead_for(cin + 12), cin + 12)
    _, rv = S.guarded((n, oh, ow), cout, cout + 3, S.lead_for(cout + 3, 1), cout + 3)
    got = S.conv_ref64(S.fill(xv, x), wt, sc, bi, S.fill(rv, res), stride, pad, act)
    assert got.dtype == torch.float64 and got.shape == (n, oh, ow, cout) and torch.isfinite(got).all()
    y32 = F.conv2d(x.permute(0, 3, 1, 2), wt.permute(0, 3, 1, 2), stride=stride, padding=pad)
    ref = _epilogue32(y32, sc, bi, res, act)
    assert (got - ref).abs().max().item() < 1e-5          # fp32 conv vs float64 conv of ~72 products of O(0.2)
    # element check by hand (an h / w mix-up cannot hide: the map is not square and the stride is 2)
    yy, xx, co = 3, 4, 5
    acc = 0.0
    for a in range(k):
        for b in range(k):
            iy, ix = yy * stride - pad + a, xx * stride - pad + b
            if 0 <= iy < h and 0 <= ix < w:
                acc += float((x[1, iy, ix].double() * wt[co, a, b].double()).sum())
    want = _epilogue32(torch.tensor(acc, dtype=torch.float64).view(1, 1, 1, 1), sc[co:co + 1], bi[co:co + 1], res[1:2, yy:yy + 1, xx:xx + 1, co:co + 1], act)
    assert abs(got[1, yy, xx, co].item() - want.item()) < 1e-12
    assert got.abs().max().item() > 0.5
    # without scale / bias / residual it is the plain conv
    plain = S.conv_ref64(x, wt, stride=stride, pad=pad)
    assert (plain - y32.double().permute(0, 2, 3, 1)).abs().max().item() < 1e-5


@pytest.mark.parametrize("t,div", [(4, 8), (8, 8), (12, 4)])
def test_conv_ref64_temporal_shift_equals_the_oracle(t, div):
    from oracle import ref_model as O
    g = _gen(20 + t)
    n, h, w, cin, cout = 2 * t, 2, 3, 32, 8
    x = torch.from_numpy(g.standard_normal((n, h, w, cin), dtype=np.float32))
    wt = torch.from_numpy(g.standard_normal((cout, 1, 1, cin), dtype=np.float32) * np.float32(0.25))
    xs = O.temporal_shift(x.permute(0, 3, 1, 2).contiguous(), t, div)
    assert torch.equal(S.temporal_shift64(x.permute(0, 3, 1, 2), t, div), xs)
    assert not torch.equal(xs, x.permute(0, 3, 1, 2))
    ref = F.conv2d(xs, wt.permute(0, 3, 1, 2)).double().permute(0, 2, 3, 1).clamp(min=0)
    got = S.conv_ref64(x, wt, act=S.ACT_RELU, tsm_segments=t, tsm_div=div)
    assert (got - ref).abs().max().item() < 1e-5
    assert not torch.allclose(got, S.conv_ref64(x, wt, act=S.ACT_RELU))


def test_shared_bounds_are_the_existing_ones():
    from tests import test_hip_parity
    assert S.CONV_TOL is test_hip_parity.CONV_TOL and S.CONV_TOL == 2e-4
    ref = torch.tensor([0.5, -3.0])
    assert S.conv_f16_bound(torch.float32, ref) == 2e-4 and S.conv_f16_bound(torch.float16, ref) == 2e-3 * 3.0
    assert S.conv_f16_bound(torch.float16, ref * 0.1) == 2e-3


# ---- guarded workspaces -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes,offset", [(4, 0), (1000, 0), (1001, 0), (1003, 16), (4096, 4), (3 << 20, 64), ((3 << 20) + 2, 0)])
def test_guarded_workspace_geometry(nbytes, offset):
    buf, ws = S.guarded_workspace(nbytes, "cpu", offset_bytes=offset)
    words = (nbytes + 3) // 4
    guard = max(nbytes, 1 << 20)
    assert S.WS_GUARD_MIN == 1 << 20
    assert buf.dim() == 1 and buf.dtype == torch.float32 and ws.shape == (1, words) and ws.stride(1) == 1
    assert ws.data_ptr() % 256 == offset                          # 256-byte aligned plus the offset
    lead = ws.storage_offset() - buf.storage_offset()
    assert 4 * lead >= guard and 4 * (buf.numel() - lead - words) >= guard         # both guards hold max(nbytes, 1 MiB) bytes
    assert ws.data_ptr() == buf.data_ptr() + 4 * lead
    assert S.is_all_canary(buf) and torch.isnan(ws).all()
    S.assert_guards_intact(buf, ws)
    S.assert_workspace_intact(buf, ws, nbytes=nbytes)
    ws.fill_(2.0)                                                 # the whole payload may change, its last partial word included
    S.assert_guards_intact(buf, ws)
    assert S.workspace_damage(buf, ws, nbytes) is None and not S.is_all_canary(ws)


def test_guarded_workspace_fills():
    _, ws = S.guarded_workspace(40, "cpu", fill="zero")
    assert torch.equal(ws, torch.zeros(1, 10))
    stale = torch.arange(10, dtype=torch.float32) + 0.5
    buf, ws = S.guarded_workspace(40, "cpu", fill=stale, offset_bytes=8)
    assert torch.equal(ws.reshape(-1), stale)
    S.assert_guards_intact(buf, ws)
    stale_bits = torch.full((10,), S.CANARY_F32, dtype=torch.int64).to(torch.int32).view(torch.float32)      # bytes, not values: a NaN payload survives
    _, ws = S.guarded_workspace(40, "cpu", fill=stale_bits)
    assert S.is_all_canary(ws)
    for bad in (dict(fill=torch.zeros(9)), dict(fill="ones"), dict(offset_bytes=2), dict(offset_bytes=-4)):
        with pytest.raises(ValueError):
            S.guarded_workspace(40, "cpu", **bad)
    with pytest.raises(ValueError):
        S.guarded_workspace(0, "cpu")


@pytest.mark.parametrize("nbytes,offset", [(1000, 0), (1001, 0), (1002, 4), (8192, 16)])
def test_guarded_workspace_damage_one_word_before_and_after(nbytes, offset):
    words = (nbytes + 3) // 4
    # one word in front of the start
    buf, ws = S.guarded_workspace(nbytes, "cpu", fill="zero", offset_bytes=offset)
    lead = ws.storage_offset()
    buf[lead - 1] = 1.0
    assert S.find_guard_damage(buf, ws) == (lead - 1, -1, words - 1, "lead")
    assert "4 bytes in front of the workspace's start" in S.workspace_damage(buf, ws, nbytes)
    with pytest.raises(AssertionError) as e:
        S.assert_guards_intact(buf, ws, "ws")
    assert "4 bytes in front of the payload's start" in str(e.value) and "lead" in str(e.value)
    with pytest.raises(AssertionError) as e:
        S.assert_workspace_intact(buf, ws, "gru ws", nbytes)
    assert str(e.value).startswith("gru ws: ") and "4 bytes in front" in str(e.value)
    # the first word behind the end: 0 bytes past the whole-word payload, (4 * words - nbytes) bytes past the byte count
    buf, ws = S.guarded_workspace(nbytes, "cpu", fill="zero", offset_bytes=offset)
    lead = ws.storage_offset()
    buf[lead + words] = 1.0
    assert S.find_guard_damage(buf, ws) == (lead + words, 1, 0, "trail")
    assert "%d bytes past the workspace's end of %d bytes" % (4 * words - nbytes, nbytes) in S.workspace_damage(buf, ws, nbytes)
    with pytest.raises(AssertionError) as e:
        S.assert_guards_intact(buf, ws, "ws")
    assert "0 bytes past the payload's end" in str(e.value) and "trail" in str(e.value)
    # ... and far behind it: the last word of the allocation
    buf, ws = S.guarded_workspace(nbytes, "cpu", offset_bytes=offset)
    lead = ws.storage_offset()
    buf[-1] = 0.0
    far = 4 * (buf.numel() - 1 - lead) - nbytes
    assert far >= (1 << 20) - 4 and "%d bytes past the workspace's end" % far in S.workspace_damage(buf, ws, nbytes)
    # the first and the last payload word are not damage
    buf, ws = S.guarded_workspace(nbytes, "cpu", offset_bytes=offset)
    ws[0, 0], ws[0, -1] = 1.0, 2.0
    S.assert_guards_intact(buf, ws)
    assert S.workspace_damage(buf, ws, nbytes) is None
