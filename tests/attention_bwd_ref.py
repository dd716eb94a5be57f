"""fp64 references of the three attention backward kernels (CPU only, plain torch, no autograd).

The closed forms the kernel headers state (csrc/attention_bwd.hip, divided_bwd.hip, window_bwd.hip),
in the log2 domain with q' = q * scale * log2 e as the q|k|v buffers store it:

    S' = q'.k (+ b log2 e)     P = exp2(S' - lse2)       O = P V
    dV = P^T dO                dP = dO V^T               Delta = rowsum(dO o O)
    dS' = ln2 * P o (dP - Delta)        dK = dS'^T q'    dq' = dS' K

`model_roundings=True` rounds to bf16 (round to nearest even) at exactly the points where the MFMA
kernels do: O before Delta, P before the dV product, dS (without its ln2, which the kernels apply
to the fp32 accumulator) before the dK and dq' products, and the outputs; and it forms O and
dP - Delta with the forward's bf16 P~ and the fp32 Delta / dP (see `_core`).  The temporal kernel is
all-fp32 VALU work, so only its outputs are rounded.  The distance between the rounded and the
exact result is the error budget the GPU tests hold the kernels to (tests/test_attention_bwd_edges_gpu.py).
"""
import math

import torch

from oracle import swin3d_ref as swin_ref

LN2 = math.log(2.0)
F64 = torch.float64


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """RNE rounding to bf16, returned in fp64 (through fp32: bf16 is a prefix of the fp32 encoding)."""
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def _r(x, on):
    return bf16_round(x) if on else x


def _f32(x):
    return x.to(torch.float32).to(F64)


def _delta_f32(do, o):
    """Delta as the kernels form it: the products (exact in fp32 for bf16 factors) added one by one,
    in element order, into an fp32 sum that is stored as fp32."""
    a, b = do.to(torch.float32), o.to(torch.float32)
    acc = torch.zeros(a.shape[:-1], dtype=torch.float32)
    for d in range(a.shape[-1]):
        acc = acc + a[..., d] * b[..., d]
    return acc.to(F64).unsqueeze(-1)


def _core(q, k, v, do, bias2=None, model_roundings=False, fwd_tile=None):
    """One batch of independent attention problems: q, k, v, do fp64 [..., n, d]; bias2 (log2 units,
    -inf where masked) broadcastable to [..., n, n].  Returns o, lse2, delta, dq', dk, dv, and
    G = P o (dP - Delta) unrounded (the bias gradient in natural units).

    Roundings of the model beyond the five bf16 points of the module docstring, each one the kernels
    make (added after the first GPU measurement; without them the model has NO error on one-hot rows,
    where O = v_k and Delta = dP_k cancel identically in fp64, while the kernels keep a residue):
      * the training forwards (attention.hip / window.hip, WLSE) round the UNNORMALISED
        P~ = exp2(S' - m) to bf16 for the P.V product but sum the fp32 P~ for the row sum l, so
        O = bf16(P~) V / sum(P~): a one-hot row's O is v_k scaled by bf16(P~_k) / P~_k, not v_k.
        m is what the kernel subtracts: nothing in the window kernel (max-free pass), the row max
        over the first `fwd_tile` keys in the joint kernel (tile 0's max; the re-basing it does
        when a partial row sum passes 2^8 moves later tiles' m and is not modelled: it changes
        which mantissas get rounded, not how many bits they keep);
      * Delta is accumulated and stored in fp32 (attn_bwd_prep_kernel, window_bwd's staging loop)
        and dP is an fp32 MFMA accumulator: dP - Delta carries an fp32 residue that matters where
        the two cancel."""
    s = q @ k.transpose(-1, -2)
    if bias2 is not None:
        s = s + bias2
    m = s.max(dim=-1, keepdim=True).values
    lse2 = m + torch.log2(torch.exp2(s - m).sum(dim=-1, keepdim=True))
    p = torch.exp2(s - lse2)
    dp = do @ v.transpose(-1, -2)
    if model_roundings:
        mf = 0.0 if fwd_tile is None else s[..., :fwd_tile].max(dim=-1, keepdim=True).values
        pt = torch.exp2(s - mf)
        o = bf16_round((bf16_round(pt) @ v) / pt.sum(dim=-1, keepdim=True))
        delta = _delta_f32(do, o)
        dp = _f32(dp)
    else:
        o = p @ v
        delta = (do * o).sum(dim=-1, keepdim=True)
    dv = _r(p, model_roundings).transpose(-1, -2) @ do
    g = p * (dp - delta)
    if not model_roundings:
        # A row of G sums to zero.  Where one key holds P = 1 - 2^-40 or less, dP - Delta of that key
        # cancels below what fp64 resolves (at 2^-53 the direct form returns 0 and drops the row's
        # whole gradient), so the exact reference takes the row's largest entry as minus the sum of
        # the others: the same value in exact arithmetic, accurate in fp64 at any sharpness.
        top = torch.zeros_like(g, dtype=torch.bool).scatter_(-1, s.argmax(dim=-1, keepdim=True), True)
        g = torch.where(top, -g.masked_fill(top, 0.0).sum(dim=-1, keepdim=True), g)
    gr = _r(g, model_roundings)
    dq = LN2 * (gr @ k)
    dk = LN2 * (gr.transpose(-1, -2) @ q)
    return o, lse2.squeeze(-1), delta.squeeze(-1), _r(dq, model_roundings), _r(dk, model_roundings), \
        _r(dv, model_roundings), g


def joint_bwd(q, k, v, do, model_roundings: bool = False):
    """q (= q' as stored), k, v, do [B, S, H, 64] -> o, dq, dk, dv [B, S, H, 64] and lse2, delta [B, H, S]."""
    qf, kf, vf, df = (t.to(F64).permute(0, 2, 1, 3) for t in (q, k, v, do))
    o, lse2, delta, dq, dk, dv, _ = _core(qf, kf, vf, df, None, model_roundings, fwd_tile=64)
    back = lambda t: t.permute(0, 2, 1, 3).contiguous()  # noqa: E731
    return back(o), lse2, delta, back(dq), back(dk), back(dv)


def temporal_bwd(qkv, dout, B, P, T, H, model_roundings: bool = False):
    """TimeSformer temporal attention on the clip layout: qkv [B*(1+P*T), 3*H*64], dout [rows, H*64],
    rows b*(1+P*T) + 1 + p*T + t.  Returns o [rows, H*64] and dqkv [rows, 3*H*64] (dq'|dk|dv) with
    zero CLS rows (the kernels leave them alone)."""
    S = 1 + P * T
    x = qkv.to(F64).reshape(B, S, 3, H, 64)[:, 1:].reshape(B, P, T, 3, H, 64)
    q, k, v = (x[:, :, :, i].permute(0, 1, 3, 2, 4) for i in range(3))  # [B, P, H, T, 64]
    df = dout.to(F64).reshape(B, S, H, 64)[:, 1:].reshape(B, P, T, H, 64).permute(0, 1, 3, 2, 4)
    o, _, _, dq, dk, dv, _ = _core(q, k, v, df, None, False)
    o, dq, dk, dv = (_r(t, model_roundings) for t in (o, dq, dk, dv))
    out = torch.zeros(B, S, H, 64, dtype=F64)
    out[:, 1:] = o.permute(0, 1, 3, 2, 4).reshape(B, P * T, H, 64)
    dqkv = torch.zeros(B, S, 3, H, 64, dtype=F64)
    for i, t in enumerate((dq, dk, dv)):
        dqkv[:, 1:, i] = t.permute(0, 1, 3, 2, 4).reshape(B, P * T, H, 64)
    return out.reshape(B * S, H * 64), dqkv.reshape(B * S, 3 * H * 64)


def window_rows(B, grid, window, shift):
    """Global token row of every (window, window-local token): torchvision's roll by -shift and window
    partition applied to the row numbers, int64 [B * nwindows, vol]."""
    T, H, W = grid
    wt, wh, ww = window
    rows = torch.arange(B * T * H * W).reshape(B, T, H, W)
    if sum(shift):
        rows = torch.roll(rows, shifts=(-shift[0], -shift[1], -shift[2]), dims=(1, 2, 3))
    rows = rows.view(B, T // wt, wt, H // wh, wh, W // ww, ww).permute(0, 1, 3, 5, 2, 4, 6)
    return rows.reshape(-1, wt * wh * ww)


def window_bwd(qkv, table, dout, B, grid, heads, window, shift, full, model_roundings: bool = False):
    """Swin 3D shifted-window attention, head_dim 32: qkv [B*T*H*W, 3*heads*32] (q' prescaled by
    d^-1/2 log2 e), table [ntab, heads] (natural units), dout [rows, heads*32].  Pairs in different
    shift regions get -inf.  Returns o [rows, heads*32], dqkv [rows, 3*heads*32], dtable [ntab, heads]."""
    T, H, W = grid
    wt, wh, ww = window
    vol = wt * wh * ww
    C = heads * 32
    nrows = B * T * H * W
    nw = (T // wt) * (H // wh) * (W // ww)
    rows = window_rows(B, grid, window, shift)                      # [B*nw, vol]
    x = qkv.to(F64)[:nrows, :3 * C][rows].reshape(B * nw, vol, 3, heads, 32)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))    # [B*nw, heads, vol, 32]
    df = dout.to(F64)[:nrows, :C][rows].reshape(B * nw, vol, heads, 32).permute(0, 2, 1, 3)
    tab = table.to(F64)
    bias2 = swin_ref.relative_position_bias(tab, full, window).unsqueeze(0) / LN2   # [1, heads, vol, vol]
    if sum(shift):
        lab = swin_ref.shift_region_labels((T, H, W), window, shift)
        lab = lab.view(T // wt, wt, H // wh, wh, W // ww, ww).permute(0, 2, 4, 1, 3, 5).reshape(nw, vol)
        masked = (lab.unsqueeze(1) - lab.unsqueeze(2)) != 0         # [nw, vol, vol]
        bias2 = bias2.expand(nw, heads, vol, vol).masked_fill(masked.unsqueeze(1), float("-inf"))
        bias2 = bias2.repeat(B, 1, 1, 1)
    o, _, _, dq, dk, dv, g = _core(q, k, v, df, bias2, model_roundings)
    out = torch.zeros(nrows, C, dtype=F64)
    out[rows.reshape(-1)] = o.permute(0, 2, 1, 3).reshape(-1, C)
    dqkv = torch.zeros(nrows, 3, heads, 32, dtype=F64)
    for i, t in enumerate((dq, dk, dv)):
        dqkv[rows.reshape(-1), i] = t.permute(0, 2, 1, 3).reshape(-1, heads, 32)
    idx = swin_ref.relative_position_index(full)[:vol, :vol].reshape(-1)
    dtable = torch.zeros(tab.shape[0], heads, dtype=F64)
    dtable.index_add_(0, idx, g.sum(dim=0).permute(1, 2, 0).reshape(vol * vol, heads))
    return out, dqkv.reshape(nrows, 3 * C), dtable


def table_entries_used(window, full):
    """bool [ntab]: the bias-table entries a window (the full window's index sliced) ever indexes."""
    vol = window[0] * window[1] * window[2]
    ntab = (2 * full[0] - 1) * (2 * full[1] - 1) * (2 * full[2] - 1)
    used = torch.zeros(ntab, dtype=torch.bool)
    used[swin_ref.relative_position_index(full)[:vol, :vol].reshape(-1)] = True
    return used


# ------------------------------------------------------------------------------------ metrics
def rel_l2(got, ref):
    got, ref = got.to(F64).cpu(), ref.to(F64).cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def segment_denominators(ref, seg):
    """Per (row, head) `seg`-wide segment of ref [rows, nseg*seg]: max(||ref||_2, floor) with floor =
    1e-3 x the median segment norm (exact-zero rows do not divide by zero), and that median."""
    n = ref.to(F64).cpu().reshape(-1, seg).norm(dim=1)
    med = float(n.median())
    return n.clamp_min(1e-3 * med if med > 0 else 1e-300), med


def row_rel_err(got, ref, seg=64):
    """||got - ref||_2 / max(||ref||_2, floor) per (row, head) segment, fp64 [rows * nseg]."""
    den, _ = segment_denominators(ref, seg)
    d = (got.to(F64).cpu() - ref.to(F64).cpu()).reshape(-1, seg).norm(dim=1)
    return d / den


def budget(got, model, exact, seg=64, name="", zero_scale=None):
    """The acceptance rule: e_kernel <= 2 e_model + 2^-8 scale, for the global relative L2 (scale 1)
    and for every (row, head) segment against the worst segment of the model (scale = the median
    segment norm over the segment's own denominator: 2^-8 of a typical segment, in the segment's
    relative units; 1 for a typical segment, up to 1e3 for the floored near-zero ones).  Holding
    each segment to the model's maximum is the strict reading of "the maximum of row_rel_err".
    Where the exact result is identically zero (the q' and k gradients of a one-key softmax:
    dS = 0) no relative error exists; the errors are then taken relative to `zero_scale`, a tensor
    of the same call and layout (the value gradient): what the kernel leaves of the cancellation
    dP - Delta must stay below 2^-8 of it.
    Returns (ok, message, ratios) with ratios = (global e_kernel / e_model, worst-row e_kernel / e_model)."""
    if zero_scale is not None and not bool(exact.to(F64).any()):
        zs = zero_scale.to(F64).cpu()
        _, med = segment_denominators(zs, seg)
        eg_k, eg_m = float(got.to(F64).cpu().norm() / zs.norm()), float(model.to(F64).cpu().norm() / zs.norm())
        rk = got.to(F64).cpu().reshape(-1, seg).norm(dim=1) / med
        ok = eg_k <= 2.0 * eg_m + 2.0 ** -8 and float(rk.max()) <= 2.0 ** -8
        return ok, f"{name}: exact result is zero; kernel norm / value-gradient norm {eg_k:.3e}, worst row {float(rk.max()):.3e}", \
            (0.0, 0.0)
    eg_k, eg_m = rel_l2(got, exact), rel_l2(model, exact)
    rk, rm = row_rel_err(got, exact, seg), row_rel_err(model, exact, seg)
    den, med = segment_denominators(exact, seg)
    em_row = float(rm.max())
    allow = 2.0 * em_row + 2.0 ** -8 * (med / den)
    over = rk - allow
    ok = eg_k <= 2.0 * eg_m + 2.0 ** -8 and bool((over <= 0).all())
    ratios = (eg_k / max(eg_m, 1e-300), float(rk.max()) / max(em_row, 1e-300))
    i = int(over.argmax())
    msg = (f"{name}: global e_kernel {eg_k:.3e} e_model {eg_m:.3e}; rows e_kernel max {float(rk.max()):.3e} "
           f"e_model max {em_row:.3e}; worst segment {i} err {float(rk[i]):.3e} allowed {float(allow[i]):.3e}")
    return ok, msg, ratios
