"""The fp64 references of tests/attention_bwd_ref.py checked without a GPU: the closed forms against
torch fp64 autograd of the naive softmax attention (1e-10 relative), and the bf16 rounding model
against the exact result (inside the 1.5e-2 relative L2 the GPU tests already accept)."""
import math

import pytest
import torch

import attention_bwd_ref as R
from oracle import swin3d_ref as swin_ref

LN2 = math.log(2.0)
F64 = torch.float64


def _close(got, want, tol=1e-10):
    err = float((got - want).norm() / want.norm().clamp_min(1e-300))
    assert err < tol, err


def _bf(shape, g, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).bfloat16()


# ------------------------------------------------------------------------------------ joint
def _joint_inputs(B=2, S=70, H=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    return _bf((B, S, H, 64), g, 0.4), _bf((B, S, H, 64), g), _bf((B, S, H, 64), g), _bf((B, S, H, 64), g, 0.1)


def test_joint_matches_autograd():
    q, k, v, do = _joint_inputs()
    qf, kf, vf = (t.to(F64).permute(0, 2, 1, 3).clone().requires_grad_() for t in (q, k, v))
    s = (qf @ kf.transpose(-1, -2)) * LN2
    o = torch.softmax(s, dim=-1) @ vf
    o.backward(do.to(F64).permute(0, 2, 1, 3))
    lse2 = torch.logsumexp(s, dim=-1) / LN2
    o_r, lse_r, delta_r, dq, dk, dv = R.joint_bwd(q, k, v, do)
    _close(o_r, o.detach().permute(0, 2, 1, 3))
    _close(lse_r, lse2.detach())
    _close(delta_r, (do.to(F64) * o_r).sum(-1).permute(0, 2, 1))
    for got, want in ((dq, qf.grad), (dk, kf.grad), (dv, vf.grad)):
        _close(got, want.permute(0, 2, 1, 3))


def test_joint_rounding_model_inside_accepted_band():
    q, k, v, do = _joint_inputs(seed=1)
    exact = R.joint_bwd(q, k, v, do)
    model = R.joint_bwd(q, k, v, do, model_roundings=True)
    for i in (0, 3, 4, 5):
        e = R.rel_l2(model[i], exact[i])
        assert 0 < e < 1.5e-2, (i, e)
    # lse is not rounded; delta moves only through the rounded O
    assert R.rel_l2(model[1], exact[1]) == 0


# ------------------------------------------------------------------------------------ temporal
def _temporal_inputs(T, B=2, P=3, H=2):
    g = torch.Generator().manual_seed(100 + T)
    S = 1 + P * T
    qkv = _bf((B * S, 3 * H * 64), g, 0.5)
    dout = _bf((B * S, H * 64), g)
    return qkv, dout, B, P, H, S


@pytest.mark.parametrize("T", [1, 5, 16])
def test_temporal_matches_autograd(T):
    qkv, dout, B, P, H, S = _temporal_inputs(T)
    x = qkv.to(F64).view(B, S, 3, H, 64)[:, 1:].reshape(B, P, T, 3, H, 64).clone().requires_grad_()
    s = torch.einsum("bptha,bpuha->bphtu", x[:, :, :, 0], x[:, :, :, 1]) * LN2
    o = torch.einsum("bphtu,bpuha->bptha", torch.softmax(s, -1), x[:, :, :, 2])
    o.backward(dout.to(F64).view(B, S, H, 64)[:, 1:].reshape(B, P, T, H, 64))
    o_r, dqkv = R.temporal_bwd(qkv, dout, B, P, T, H)
    _close(o_r.view(B, S, H, 64)[:, 1:], o.detach().reshape(B, P * T, H, 64))
    _close(dqkv.view(B, S, 3, H, 64)[:, 1:], x.grad.reshape(B, P * T, 3, H, 64))
    assert (o_r.view(B, S, -1)[:, 0] == 0).all() and (dqkv.view(B, S, -1)[:, 0] == 0).all()


def test_temporal_rounding_model_inside_accepted_band():
    qkv, dout, B, P, H, S = _temporal_inputs(8)
    exact = R.temporal_bwd(qkv, dout, B, P, 8, H)
    model = R.temporal_bwd(qkv, dout, B, P, 8, H, model_roundings=True)
    for e, m in zip(exact, model):
        err = R.rel_l2(m, e)
        assert 0 < err < 1.5e-2, err


# ------------------------------------------------------------------------------------ window
def _window_autograd(qkv, table, dout, B, grid, heads, window, shift, full):
    """torchvision's roll / partition / bias / shift mask / softmax / reverse in fp64 under autograd
    (the formulation of tests/test_swin3d_train_gpu.py::_attn_ref, with -inf for masked pairs)."""
    T, H, W = grid
    C = heads * 32
    xr = qkv.to(F64).clone().requires_grad_()
    tr = table.to(F64).clone().requires_grad_()
    x = xr.reshape(B, T, H, W, 3 * C)
    if sum(shift):
        x = torch.roll(x, shifts=(-shift[0], -shift[1], -shift[2]), dims=(1, 2, 3))
    wt, wh, ww = window
    nw = (T // wt) * (H // wh) * (W // ww)
    vol = wt * wh * ww
    x = x.view(B, T // wt, wt, H // wh, wh, W // ww, ww, 3 * C).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(B * nw, vol, 3 * C)
    q, k, v = x.reshape(B * nw, vol, 3, heads, 32).permute(2, 0, 3, 1, 4)
    attn = (q @ k.transpose(-2, -1)) * LN2 + swin_ref.relative_position_bias(tr, full, window).unsqueeze(0)
    if sum(shift):
        m = swin_ref.shift_region_labels((T, H, W), window, shift)
        m = m.view(T // wt, wt, H // wh, wh, W // ww, ww).permute(0, 2, 4, 1, 3, 5).reshape(nw, vol)
        m = (m.unsqueeze(1) - m.unsqueeze(2)) != 0
        attn = attn.view(B, nw, heads, vol, vol).masked_fill(m.unsqueeze(1).unsqueeze(0), float("-inf"))
        attn = attn.view(-1, heads, vol, vol)
    o = torch.softmax(attn, -1) @ v
    o = o.transpose(1, 2).reshape(B, T // wt, H // wh, W // ww, wt, wh, ww, C)
    o = o.permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(B, T, H, W, C)
    if sum(shift):
        o = torch.roll(o, shifts=tuple(shift), dims=(1, 2, 3))
    o = o.reshape(B * T * H * W, C)
    o.backward(dout.to(F64))
    return o.detach(), xr.grad, tr.grad


WINDOW_CASES = [
    (2, (4, 14, 7), 2, (2, 7, 7), (1, 3, 0), (2, 7, 7)),   # (2,7,7) shifted
    (2, (2, 7, 7), 2, (1, 7, 7), (0, 0, 0), (8, 7, 7)),    # shrunk window: the full index sliced
    (1, (4, 6, 6), 1, (2, 3, 3), (1, 1, 1), (2, 3, 3)),    # shifted in all three dimensions
]


def _window_inputs(B, grid, heads, full, seed):
    g = torch.Generator().manual_seed(seed)
    rows = B * grid[0] * grid[1] * grid[2]
    ntab = (2 * full[0] - 1) * (2 * full[1] - 1) * (2 * full[2] - 1)
    qkv = _bf((rows, 3 * heads * 32), g, 0.7)
    table = torch.randn(ntab, heads, generator=g) * 0.5
    dout = _bf((rows, heads * 32), g)
    return qkv, table, dout


@pytest.mark.parametrize("B,grid,heads,window,shift,full", WINDOW_CASES)
def test_window_matches_autograd(B, grid, heads, window, shift, full):
    qkv, table, dout = _window_inputs(B, grid, heads, full, seed=sum(grid))
    o, dqkv, dtab = _window_autograd(qkv, table, dout, B, grid, heads, window, shift, full)
    o_r, dqkv_r, dtab_r = R.window_bwd(qkv, table, dout, B, grid, heads, window, shift, full)
    _close(o_r, o)
    _close(dqkv_r, dqkv)
    _close(dtab_r, dtab)
    unused = ~R.table_entries_used(window, full)
    assert (dtab_r[unused] == 0).all() and (dtab[unused] == 0).all()
    assert bool(unused.any()) == (tuple(window) != tuple(full))


def test_window_rounding_model_inside_accepted_band():
    B, grid, heads, window, shift, full = WINDOW_CASES[0]
    qkv, table, dout = _window_inputs(B, grid, heads, full, seed=5)
    exact = R.window_bwd(qkv, table, dout, B, grid, heads, window, shift, full)
    model = R.window_bwd(qkv, table, dout, B, grid, heads, window, shift, full, model_roundings=True)
    for e, m in zip(exact, model):
        err = R.rel_l2(m, e)
        assert 0 < err < 1.5e-2, err


# ------------------------------------------------------------------------------------ metrics
def test_row_metric_sees_one_bad_segment_the_global_metric_misses():
    g = torch.Generator().manual_seed(3)
    ref = torch.randn(394, 384, generator=g, dtype=F64)
    ref[7] = 0                                   # exact-zero rows do not divide by zero
    got = ref.clone()
    got[100, 64:128] *= 0.5                      # one wrong 64-column row segment
    assert R.rel_l2(got, ref) < 1.5e-2
    e = R.row_rel_err(got, ref)
    assert torch.isfinite(e).all() and abs(float(e.max()) - 0.5) < 1e-12 and int(e.argmax()) == 100 * 6 + 1
    ok, msg, _ = R.budget(got, ref + 1e-3 * torch.randn(394, 384, generator=g, dtype=F64), ref)
    assert not ok, msg
