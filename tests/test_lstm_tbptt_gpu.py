"""Training on whole videos with a carried LSTM state, on the GPU: vc_lstm_seq_fwd_train_state /
vc_lstm_seq_bwd_state, autograd_ops.lstm_layer_state, VideoResNet50LSTM.forward_train_stream and
main.py --tbptt_chunk.

Kernels, over (B, T, H) = (1, 1, 32), (5, 7, 100), (5, 3, 64), (3, 3, 1024) (a single step, hidden % 64 != 0,
one over the group of 4, the group-of-2 kernel at one over its group) and one ragged case, lengths
(4, 0, 3, 1, 6) at H = 64 (a length 0, a length 1, the group boundary inside it).  Bit for bit (torch.equal):
the forward against vc_lstm_seq_fwd (train variant) from the zero state and against vc_lstm_seq_fwd_state from
a state, chunked against whole, the backward against vc_lstm_seq_bwd in both last_only modes, the backward
over two chunks chained through dh0 / dc0 against the backward over the whole, reruns, aliased dh0 / dh_n.
Against CPU fp32 autograd of a hand-written cell loop: relative L2 of dpre, dh0 and dc0, bound = 10x the
value measured on the MI355X, never looser than 1e-3 (the rule of tests/test_lstm_gpu.py).

Op and model (hidden 32, 2 layers, 64 x 64 frames, lengths (5, 2, 8), chunk 3) by the project's band rule:
the fp32 oracle rerun with this implementation's bf16 storage points gives each gradient's attainable
error, ours must stay within 1.5x that + 0.03 of the fp32 oracle.  CLI: a tiny .npy tree, --tbptt_chunk 4.
"""
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vclip_amd.weights import make_resnet50_lstm_weights, make_synthetic_video

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 7.0

# relative L2 against CPU fp32 autograd of the cell loop, nonzero (h0, c0), dh_seq (masked) + dh_n + dc_n coming
# in: measured on the MI355X over the five cases below dpre 1.35e-7 .. 2.01e-7, dh0 1.65e-7 .. 5.57e-7 (one more
# sum over 4H terms), dc0 6.4e-8 .. 1.72e-7; each bound is 10x the largest measured, never looser than 1e-3.
# Anything near 1e-3 would mean a non-fp32 product.
BWD_MEASURED = dict(dpre=2.01e-7, dh0=5.57e-7, dc0=1.72e-7)
BWD_BOUND = {k: min(10 * v, 1e-3) for k, v in BWD_MEASURED.items()}

DENSE = [(1, 1, 32), (5, 7, 100), (5, 3, 64), (3, 3, 1024)]
CASES = [((T,) * B, H) for B, T, H in DENSE] + [((4, 0, 3, 1, 6), 64)]
IDS = [f"{B}x{T}x{H}" for B, T, H in DENSE] + ["ragged"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vclip_amd import _lib
    _lib.load()


# ---- inputs and references, once per case ----------------------------------------------------------
def _cell_loop(pre, w_hh, h0, c0, lengths, keep=None, round_hprev=None):
    """nn.LSTM's cell arithmetic (gate order i, f, g, o) per sequence: pre [B, Tmax, 4H] (sequence b uses its
    first lengths[b] steps), the state (h0, c0) [B, H].  Returns ([h_seq of sequence b, [lengths[b], H], times
    keep], h_n [B, H], c_n [B, H]); a sequence of length 0 passes its state through."""
    H = w_hh.shape[1]
    seqs, hn, cn = [], [], []
    for b, n in enumerate(lengths):
        h, c = h0[b:b + 1], c0[b:b + 1]
        hs = []
        for t in range(n):
            rec = h @ w_hh.T if round_hprev is None else round_hprev(h, w_hh)
            a = pre[b:b + 1, t] + rec
            i, f, g, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.tanh(a[:, 2 * H:3 * H]), \
                torch.sigmoid(a[:, 3 * H:])
            c = f * c + i * g
            h = o * torch.tanh(c)
            hs.append(h)
        hseq = torch.cat(hs) if hs else pre.new_zeros(0, H)
        seqs.append(hseq if keep is None else hseq * keep[b, :n])
        hn.append(h)
        cn.append(c)
    return seqs, torch.cat(hn), torch.cat(cn)


_REF = {}


def _case(lengths, H):
    key = (lengths, H)
    if key not in _REF:
        B, T = len(lengths), max(lengths)
        g = torch.Generator().manual_seed(100 * B + 10 * T + H)
        k = 1.0 / np.sqrt(H)
        r = dict(lengths=lengths, H=H, B=B, T=T, w_hh=(torch.rand(4 * H, H, generator=g) * 2 - 1) * k,
                 pre=torch.randn(B, T, 4 * H, generator=g), keep=torch.bernoulli(torch.full((B, T, H), 0.5), generator=g) * 2,
                 dh=torch.randn(B, T, H, generator=g), h0=torch.randn(B, H, generator=g) * 0.5,
                 c0=torch.randn(B, H, generator=g), dh_n=torch.randn(B, H, generator=g), dc_n=torch.randn(B, H, generator=g))
        _REF[key] = r
    return _REF[key]


def _ref_grads(r):
    """CPU fp32 autograd of the cell loop from (h0, c0), with the masked h_seq, h_n and c_n all in the loss:
    (dpre [B, T, 4H], zero past a sequence's end; dh0; dc0)."""
    if "grads" not in r:
        pre, h0, c0 = (r[n].clone().requires_grad_() for n in ("pre", "h0", "c0"))
        seqs, hn, cn = _cell_loop(pre, r["w_hh"], h0, c0, r["lengths"], keep=r["keep"])
        loss = (hn * r["dh_n"]).sum() + (cn * r["dc_n"]).sum()
        for b, (s, n) in enumerate(zip(seqs, r["lengths"])):
            loss = loss + (s * r["dh"][b, :n]).sum()
        loss.backward()
        r["grads"] = (pre.grad, h0.grad, c0.grad)
    return r["grads"]


# ---- row layouts --------------------------------------------------------------------------------------
def _layout(lengths, gap=1):
    """row0 with `gap` unowned rows behind every sequence, and the row count."""
    row0, at = [], 0
    for n in lengths:
        row0.append(at)
        at += n + gap
    return row0, max(at, 1)


def _place(x, lengths, row0, nrows, start=None, fill=0.0):
    """x [B, T, C] -> rows [nrows, C]: steps start[b] .. start[b] + lengths[b] - 1 of sequence b at row0[b]."""
    out = torch.full((nrows, x.shape[-1]), fill, dtype=x.dtype)
    for b, (r0, n) in enumerate(zip(row0, lengths)):
        s = 0 if start is None else start[b]
        out[r0:r0 + n] = x[b, s:s + n]
    return out


def _gather(rows, lengths, row0, T):
    """the inverse: rows -> [B, T, C], zero past a sequence's end"""
    out = torch.zeros(len(lengths), T, rows.shape[-1], dtype=rows.dtype)
    for b, (r0, n) in enumerate(zip(row0, lengths)):
        out[b, :n] = rows[r0:r0 + n]
    return out


def _unowned(lengths, row0, nrows):
    m = torch.ones(nrows, dtype=torch.bool)
    for r0, n in zip(row0, lengths):
        m[r0:r0 + n] = False
    return m


def _opt(t):
    return None if t is None else t.contiguous().to(DEV)


def _fwd(r, lengths, row0, nrows, h0=None, c0=None, keep=False, start=None, dense_T=None):
    """vc_lstm_seq_fwd_train_state over steps start[b] .. of each sequence, into buffers whose unowned rows
    (the gaps and two rows behind the last) hold a sentinel; asserts that they still do."""
    from vclip_amd import ops
    H, B = r["H"], len(lengths)
    full = lambda rows, cols, dt=torch.float32: torch.full((rows, cols), SENT, dtype=dt, device=DEV)  # noqa: E731
    o = dict(h_seq=full(nrows + 2, H, torch.bfloat16), gates=full(nrows + 2, 4 * H), c_seq=full(nrows + 2, H),
             h_prev=full(nrows + 2, H, torch.bfloat16), h_n=full(B, H), c_n=full(B, H))
    kp = _place(r["keep"], lengths, row0, nrows, start, fill=1.0).to(DEV) if keep else None
    ops.lstm_seq_fwd_train_state(_place(r["pre"], lengths, row0, nrows, start).to(DEV), None if dense_T else lengths, H,
                                 r["w_hh"].t().contiguous().to(DEV), o["h_seq"], o["h_n"], o["c_n"], o["gates"], o["c_seq"],
                                 o["h_prev"], h0=_opt(h0), c0=_opt(c0), keep=kp, row0=None if dense_T else row0, T=dense_T)
    torch.cuda.synchronize()
    un = torch.cat([_unowned(lengths, row0, nrows), torch.ones(2, dtype=torch.bool)])
    for n in ("h_seq", "gates", "c_seq", "h_prev"):
        assert bool((o[n].cpu()[un].float() == SENT).all()), f"{n}: a row no sequence owns was written"
    return {n: t.cpu() for n, t in o.items()}


def _bwd(r, fw, lengths, row0, nrows, dh=True, keep=True, dh_n=None, dc_n=None, c0=None, want0=True, alias=False,
         start=None, dense_T=None):
    """vc_lstm_seq_bwd_state from the saved tensors of _fwd: (dpre rows, dpre_bf16 rows, dh0, dc0) on the CPU."""
    from vclip_amd import ops
    H, B = r["H"], len(lengths)
    dpre = torch.full((nrows + 2, 4 * H), SENT, device=DEV)
    dpb = torch.full((nrows + 2, 4 * H), SENT, dtype=torch.bfloat16, device=DEV)
    dhn, dcn = _opt(dh_n), _opt(dc_n)
    dh0 = dc0 = None
    if want0:
        dh0 = dhn if alias else torch.full((B, H), SENT, device=DEV)
        dc0 = dcn if alias else torch.full((B, H), SENT, device=DEV)
    ops.lstm_seq_bwd_state(fw["gates"].to(DEV), fw["c_seq"].to(DEV), B, None if dense_T else lengths, H, r["w_hh"].to(DEV),
                           dpre, dpb, dh_seq=_place(r["dh"], lengths, row0, nrows, start).to(DEV) if dh else None,
                           dh_n=dhn, dc_n=dcn, c0=_opt(c0),
                           keep=_place(r["keep"], lengths, row0, nrows, start, fill=1.0).to(DEV) if keep else None,
                           dh0=dh0, dc0=dc0, row0=None if dense_T else row0, T=dense_T)
    torch.cuda.synchronize()
    un = torch.cat([_unowned(lengths, row0, nrows), torch.ones(2, dtype=torch.bool)])
    assert bool((dpre.cpu()[un] == SENT).all()) and bool((dpb.cpu()[un].float() == SENT).all()), "an unowned dpre row was written"
    return dpre.cpu()[:nrows], dpb.cpu()[:nrows], None if dh0 is None else dh0.cpu(), None if dc0 is None else dc0.cpu()


def _split(lengths, s):
    """the first s steps of every sequence, and the rest"""
    a = tuple(min(n, s) for n in lengths)
    return a, tuple(n - k for n, k in zip(lengths, a))


def _splits(lengths):
    T = max(lengths)
    return sorted({1, T - 1} - {0})


# ---- vc_lstm_seq_fwd_train_state ----------------------------------------------------------------------
@pytest.mark.parametrize("B,T,H", DENSE)
def test_fwd_from_the_null_state_is_the_dense_train_variant(B, T, H):
    from vclip_amd import ops
    r = _case((T,) * B, H)
    M = B * T
    row0 = [b * T for b in range(B)]
    want = dict(h_seq=torch.empty(M, H, dtype=torch.bfloat16, device=DEV), h_n=torch.empty(B, H, device=DEV),
                gates=torch.empty(M, 4 * H, device=DEV), c_seq=torch.empty(M, H, device=DEV),
                h_prev=torch.empty(M, H, dtype=torch.bfloat16, device=DEV))
    ops.lstm_seq_fwd(r["pre"].reshape(M, 4 * H).to(DEV), B, T, H, r["w_hh"].t().contiguous().to(DEV), want["h_seq"], want["h_n"],
                     keep=r["keep"].reshape(M, H).to(DEV), gates=want["gates"], c_seq=want["c_seq"], h_prev=want["h_prev"])
    for dense_T in (T, None):  # the dense layout, and the same rows named by row0 / len
        got = _fwd(r, (T,) * B, row0, M, keep=True, dense_T=dense_T)
        for n, w in want.items():
            assert torch.equal(got[n][: w.shape[0]], w.cpu()), (n, dense_T)
    assert bool((got["h_prev"][:M].view(B, T, H)[:, 0] == 0).all())  # zero without a state


@pytest.mark.parametrize("lengths,H", CASES, ids=IDS)
def test_fwd_from_a_state_is_the_stateful_inference_recurrence(lengths, H):
    from vclip_amd import ops
    r = _case(lengths, H)
    B = len(lengths)
    row0, nrows = _layout(lengths)
    got = _fwd(r, lengths, row0, nrows, h0=r["h0"], c0=r["c0"])
    hseq = torch.full((nrows + 2, H), SENT, dtype=torch.bfloat16, device=DEV)
    hn, cn = torch.empty(B, H, device=DEV), torch.empty(B, H, device=DEV)
    ops.lstm_seq_fwd_state(_place(r["pre"], lengths, row0, nrows).to(DEV), lengths, H, r["w_hh"].t().contiguous().to(DEV), hseq,
                           hn, cn, h0=r["h0"].to(DEV), c0=r["c0"].to(DEV), row0=row0)
    assert torch.equal(got["h_seq"], hseq.cpu()) and torch.equal(got["h_n"], hn.cpu()) and torch.equal(got["c_n"], cn.cpu())
    again = _fwd(r, lengths, row0, nrows, h0=r["h0"], c0=r["c0"])
    for n in got:
        assert torch.equal(got[n], again[n]), n
    for b, (r0, n) in enumerate(zip(row0, lengths)):
        if n == 0:  # the state passes through
            assert torch.equal(got["h_n"][b], r["h0"][b]) and torch.equal(got["c_n"][b], r["c0"][b])
            continue
        assert torch.equal(got["h_prev"][r0], r["h0"][b].bfloat16())  # the operand of the W_hh gradient at a first step
        assert torch.equal(got["h_n"][b].bfloat16(), got["h_seq"][r0 + n - 1])
        assert torch.equal(got["c_n"][b], got["c_seq"][r0 + n - 1])
    # against the CPU cell loop from the same state
    with torch.no_grad():
        seqs, whn, wcn = _cell_loop(r["pre"], r["w_hh"], r["h0"], r["c0"], lengths)
    assert float((got["h_n"] - whn).abs().max()) < 1e-5 and float((got["c_n"] - wcn).abs().max()) < 1e-5
    # the mask scales the stored h_seq only
    masked = _fwd(r, lengths, row0, nrows, h0=r["h0"], c0=r["c0"], keep=True)
    for n in ("h_n", "c_n", "gates", "c_seq", "h_prev"):
        assert torch.equal(masked[n], got[n]), n
    kp = _place(r["keep"], lengths, row0, nrows, fill=1.0)
    own = ~_unowned(lengths, row0, nrows)
    assert bool((masked["h_seq"][:nrows][own][kp[own] == 0] == 0).all())
    assert torch.equal(masked["h_seq"][:nrows][own][kp[own] == 2].float(),
                       (got["h_seq"][:nrows][own][kp[own] == 2].float() * 2).bfloat16().float())


@pytest.mark.parametrize("lengths,H", CASES, ids=IDS)
def test_fwd_chunked_equals_whole(lengths, H):
    r = _case(lengths, H)
    T = max(lengths)
    row0, nrows = _layout(lengths)
    whole = _fwd(r, lengths, row0, nrows, h0=r["h0"], c0=r["c0"], keep=True)
    for s in _splits(lengths):
        la, lb = _split(lengths, s)
        if (lengths, H) == CASES[-1] and s == 1:
            assert 0 in lb and any(lb)  # the split that leaves a sequence with length 0 beside running ones
        ra, na = _layout(la)
        rb, nb = _layout(lb)
        a = _fwd(r, la, ra, na, h0=r["h0"], c0=r["c0"], keep=True)
        b = _fwd(r, lb, rb, nb, h0=a["h_n"], c0=a["c_n"], keep=True, start=la)
        assert torch.equal(b["h_n"], whole["h_n"]) and torch.equal(b["c_n"], whole["c_n"]), s
        for n in ("h_seq", "gates", "c_seq", "h_prev"):
            w = _gather(whole[n], lengths, row0, T)
            for bi, (ka, kb) in enumerate(zip(la, lb)):
                assert torch.equal(a[n][ra[bi]:ra[bi] + ka], w[bi, :ka]), (n, s, bi)
                assert torch.equal(b[n][rb[bi]:rb[bi] + kb], w[bi, ka:ka + kb]), (n, s, bi)


# ---- vc_lstm_seq_bwd_state ----------------------------------------------------------------------------
@pytest.mark.parametrize("last_only", [False, True], ids=["full", "last"])
@pytest.mark.parametrize("B,T,H", DENSE)
def test_bwd_from_the_zero_state_is_the_dense_backward(B, T, H, last_only):
    from vclip_amd import ops
    r = _case((T,) * B, H)
    M = B * T
    row0 = [b * T for b in range(B)]
    fw = _fwd(r, (T,) * B, row0, M, dense_T=T)
    want, wantb = torch.empty(M, 4 * H, device=DEV), torch.empty(M, 4 * H, dtype=torch.bfloat16, device=DEV)
    dh = r["dh_n"] if last_only else r["dh"].reshape(M, H)
    ops.lstm_seq_bwd(fw["gates"][:M].to(DEV), fw["c_seq"][:M].to(DEV), B, T, H, r["w_hh"].to(DEV), dh.contiguous().to(DEV), want,
                     wantb, last_only=last_only, keep=None if last_only else r["keep"].reshape(M, H).to(DEV))
    for dense_T in (T, None):
        for want0 in (False, True):  # dh0 / dc0 asked for or not: dpre is the same
            dpre, dpb, _, _ = _bwd(r, fw, (T,) * B, row0, M, dh=not last_only, keep=not last_only,
                                   dh_n=r["dh_n"] if last_only else None, want0=want0, dense_T=dense_T)
            assert torch.equal(dpre, want.cpu()) and torch.equal(dpb, wantb.cpu()), (dense_T, want0)


@pytest.mark.parametrize("lengths,H", CASES, ids=IDS)
def test_bwd_matches_autograd(lengths, H):
    r = _case(lengths, H)
    T = max(lengths)
    row0, nrows = _layout(lengths)
    fw = _fwd(r, lengths, row0, nrows, h0=r["h0"], c0=r["c0"], keep=True)
    kw = dict(dh_n=r["dh_n"], dc_n=r["dc_n"], c0=r["c0"])
    dpre, dpb, dh0, dc0 = _bwd(r, fw, lengths, row0, nrows, **kw)
    want = _ref_grads(r)
    rel = lambda g, w: float((g.double() - w.double()).norm() / w.double().norm())  # noqa: E731
    errs = dict(dpre=rel(_gather(dpre, lengths, row0, T), want[0]), dh0=rel(dh0, want[1]), dc0=rel(dc0, want[2]))
    print(f"lstm bwd_state lengths={lengths} H={H}: rel L2 " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()) +
          " (bounds " + " ".join(f"{v:.1e}" for v in BWD_BOUND.values()) + ")")
    assert all(errs[k] <= BWD_BOUND[k] for k in errs), errs
    own = ~_unowned(lengths, row0, nrows)
    assert torch.equal(dpb[own], dpre[own].bfloat16())  # the bf16 copy is the rounded fp32 dpre
    again = _bwd(r, fw, lengths, row0, nrows, **kw)  # deterministic
    inplace = _bwd(r, fw, lengths, row0, nrows, alias=True, **kw)  # dh0 over dh_n, dc0 over dc_n
    for a, b, c in zip((dpre, dpb, dh0, dc0), again, inplace):
        assert torch.equal(a, b) and torch.equal(a, c)
    for b, n in enumerate(lengths):
        if n == 0:  # nothing ran: the gradients of the outgoing state are those of the incoming one
            assert torch.equal(dh0[b], r["dh_n"][b]) and torch.equal(dc0[b], r["dc_n"][b])
    # absent gradients are NULL, not zero tensors: the same dpre as explicit zeros, and zeros through a length 0
    z = torch.zeros_like(r["dh_n"])
    none = _bwd(r, fw, lengths, row0, nrows, c0=r["c0"])
    zero = _bwd(r, fw, lengths, row0, nrows, dh_n=z, dc_n=z, c0=r["c0"])
    for a, b in zip(none, zero):
        assert torch.equal(a, b)
    for b, n in enumerate(lengths):
        if n == 0:
            assert not none[2][b].any() and not none[3][b].any()


@pytest.mark.parametrize("lengths,H", CASES, ids=IDS)
def test_bwd_chunked_equals_whole(lengths, H):
    """The backward over two chunks in reverse order, the second chunk's dh0 / dc0 fed into the first chunk's
    dh_n / dc_n, against the backward over the whole sequences: the same sums in the same order."""
    r = _case(lengths, H)
    T = max(lengths)
    row0, nrows = _layout(lengths)
    fw = _fwd(r, lengths, row0, nrows, h0=r["h0"], c0=r["c0"], keep=True)
    dpre, _, dh0, dc0 = _bwd(r, fw, lengths, row0, nrows, dh_n=r["dh_n"], dc_n=r["dc_n"], c0=r["c0"])
    w = _gather(dpre, lengths, row0, T)
    for s in _splits(lengths):
        la, lb = _split(lengths, s)
        ra, na = _layout(la)
        rb, nb = _layout(lb)
        fa = _fwd(r, la, ra, na, h0=r["h0"], c0=r["c0"], keep=True)
        fb = _fwd(r, lb, rb, nb, h0=fa["h_n"], c0=fa["c_n"], keep=True, start=la)
        db, _, dh0b, dc0b = _bwd(r, fb, lb, rb, nb, dh_n=r["dh_n"], dc_n=r["dc_n"], c0=fa["c_n"], start=la)
        da, _, dh0a, dc0a = _bwd(r, fa, la, ra, na, dh_n=dh0b, dc_n=dc0b, c0=r["c0"])
        assert torch.equal(dh0a, dh0) and torch.equal(dc0a, dc0), s
        for bi, (ka, kb) in enumerate(zip(la, lb)):
            assert torch.equal(da[ra[bi]:ra[bi] + ka], w[bi, :ka]), (s, bi)
            assert torch.equal(db[rb[bi]:rb[bi] + kb], w[bi, ka:ka + kb]), (s, bi)


# ---- the band rule (tests/test_lstm_gpu.py) -------------------------------------------------------------
class _Round(torch.autograd.Function):
    """bf16 storage of a tensor (forward) and / or of its gradient (backward), identity otherwise."""
    @staticmethod
    def forward(ctx, x, fwd: bool, bwd: bool):
        ctx.bwd = bwd
        return x.bfloat16().float() if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (g.bfloat16().float() if ctx.bwd else g), None, None


def _rec_bf16(h, w_hh):
    """h W_hh^T as this implementation differentiates it: the value and dL/dh in fp32, dW_hh from bf16 h_prev
    (bf16(h0) at a first step) and bf16 dpre (a zero-valued branch that carries only the W_hh gradient)."""
    hb = _Round.apply(h.detach(), True, False)
    branch = _Round.apply(hb @ w_hh.T, False, True)
    return h @ w_hh.detach().T + (branch - branch.detach())


def _pad(rows, lengths):
    """rows back to back [sum(lengths), C] -> [B, max(lengths), C], differentiable"""
    return torch.nn.utils.rnn.pad_sequence(list(torch.split(rows, list(lengths))), batch_first=True)


def _layer_oracle(x, w_ih, w_hh, b_ih, b_hh, lengths, h0, c0, keep=None, storage=False):
    """One LSTM layer in fp32 on the rows x [sum(lengths), Din] from (h0, c0); storage=True restates this
    implementation's bf16 storage points: x (the caller's), W_ih, h_prev and dpre as GEMM operands.
    Returns (h_seq rows times keep, h_n, c_n)."""
    if storage:
        pre = _Round.apply(x @ _Round.apply(w_ih, True, False).T, False, True) + b_ih + b_hh
    else:
        pre = x @ w_ih.T + b_ih + b_hh
    seqs, hn, cn = _cell_loop(_pad(pre, lengths), w_hh, h0, c0, lengths, keep=None if keep is None else _pad(keep, lengths),
                              round_hprev=_rec_bf16 if storage else None)
    return torch.cat(seqs), hn, cn


def _rel(got, want):
    got, want = got.detach().cpu().double().reshape(-1), want.detach().cpu().double().reshape(-1)
    return float((got - want).norm() / want.norm())


def _band_check(named):
    """named: {name: (ours, fp32 oracle, bf16-storage oracle)} gradients."""
    bad = []
    for n, (ours, want, stor) in named.items():
        e, b = _rel(ours, want), _rel(stor, want)
        print(f"{n:28s} ours {e:.4f}  bf16-storage oracle {b:.4f}")
        if not e <= 1.5 * b + 0.03:
            bad.append((n, e, b))
    assert not bad, bad


def test_lstm_layer_state_gradients_in_band():
    """Every gradient of the op, with h_seq (masked), h_n and c_n all in the loss, from a state that requires
    grad, over lengths with a 0 in them.  The fp32 oracle is nn.LSTM with (h0, c0), one call per sequence."""
    from vclip_amd import autograd_ops as A
    lengths, Din, H = (5, 0, 2, 8), 40, 32
    B, N = len(lengths), sum(lengths)
    g = torch.Generator().manual_seed(Din + H)
    k = 1.0 / np.sqrt(H)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k  # noqa: E731
    x = torch.randn(N, Din, generator=g).bfloat16()
    prm = [u(4 * H, Din), u(4 * H, H), u(4 * H), u(4 * H)]
    h0, c0 = torch.randn(B, H, generator=g) * 0.5, torch.randn(B, H, generator=g)
    keep = torch.bernoulli(torch.full((N, H), 0.5), generator=g) * 2
    dh, dhn, dcn = torch.randn(N, H, generator=g), torch.randn(B, H, generator=g), torch.randn(B, H, generator=g)

    def loss_of(hseq, hn, cn, dev):
        return (hseq.float() * dh.to(dev)).sum() + (hn * dhn.to(dev)).sum() + (cn * dcn.to(dev)).sum()

    dev = [t.to(DEV).requires_grad_() for t in (x, *prm, h0, c0)]
    hseq, hn, cn = A.lstm_layer_state(*dev[:5], list(lengths), h0=dev[5], c0=dev[6], keep=keep.to(DEV))
    assert hseq.dtype == torch.bfloat16 and tuple(hseq.shape) == (N, H) and tuple(hn.shape) == tuple(cn.shape) == (B, H)
    loss_of(hseq, hn, cn, DEV).backward()
    grads = {}
    for storage in (False, True):
        ref = [t.clone().requires_grad_() for t in (x.float(), *prm, h0, c0)]
        hr, hnr, cnr = _layer_oracle(*ref[:5], lengths, ref[5], ref[6], keep=keep, storage=storage)
        loss_of(hr, hnr, cnr, "cpu").backward()
        grads[storage] = [t.grad for t in ref]
        if not storage:
            fwd = (hr.detach(), hnr.detach(), cnr.detach())
    # torch's own module with (h0, c0), one call per sequence, the masks replayed: the cell loop restates it
    lstm = torch.nn.LSTM(Din, H, batch_first=True)
    with torch.no_grad():
        for dst, src in zip((lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0), prm):
            dst.copy_(src)
    xr, h0r, c0r = x.float().requires_grad_(), h0.clone().requires_grad_(), c0.clone().requires_grad_()
    outs, hns, cns, at = [], [], [], 0
    for b, n in enumerate(lengths):
        if n == 0:
            hns.append(h0r[b:b + 1])
            cns.append(c0r[b:b + 1])
            continue
        out, (h_, c_) = lstm(xr[at:at + n].unsqueeze(0), (h0r[b].view(1, 1, H), c0r[b].view(1, 1, H)))
        outs.append(out[0])
        hns.append(h_[0])
        cns.append(c_[0])
        at += n
    loss_of(torch.cat(outs) * keep, torch.cat(hns), torch.cat(cns), "cpu").backward()
    torch_grads = [xr.grad, lstm.weight_ih_l0.grad, lstm.weight_hh_l0.grad, lstm.bias_ih_l0.grad, lstm.bias_hh_l0.grad,
                   h0r.grad, c0r.grad]
    names = ("x", "w_ih", "w_hh", "b_ih", "b_hh", "h0", "c0")
    for n, a, b in zip(names, grads[False], torch_grads):
        assert _rel(a, b) < 1e-5, (n, _rel(a, b))
    assert float((hn.detach().cpu() - fwd[1]).abs().max()) < 1e-2 and float((cn.detach().cpu() - fwd[2]).abs().max()) < 1e-2
    assert float((hseq.detach().float().cpu() - fwd[0]).abs().max()) < 2.4e-2  # bf16 W_ih, bf16 h_seq, times keep = 2
    assert torch.equal(hn[1], dev[5][1]) and torch.equal(cn[1], dev[6][1])  # the length 0 passes its state through
    ours = [t.grad for t in dev]
    _band_check({n: (o, w, s) for n, o, w, s in zip(names, ours, torch_grads, grads[True])})


def test_lstm_layer_state_dense_layout_and_absent_gradients():
    """(B, T) as a tuple is the dense layout; a loss through c_n alone reaches every input (dh_seq and dh_n absent)."""
    from vclip_amd import autograd_ops as A
    B, T, Din, H = 3, 4, 40, 32
    g = torch.Generator().manual_seed(3)
    k = 1.0 / np.sqrt(H)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k  # noqa: E731
    x = torch.randn(B * T, Din, generator=g).bfloat16()
    prm = [u(4 * H, Din), u(4 * H, H), u(4 * H), u(4 * H)]
    h0, c0 = torch.randn(B, H, generator=g) * 0.5, torch.randn(B, H, generator=g)
    dcn = torch.randn(B, H, generator=g)
    res = []
    for layout in ((B, T), [T] * B):
        dev = [t.to(DEV).requires_grad_() for t in (x, *prm, h0, c0)]
        hseq, hn, cn = A.lstm_layer_state(*dev[:5], layout, h0=dev[5], c0=dev[6])
        (cn * dcn.to(DEV)).sum().backward()
        res.append([hseq.detach(), hn.detach(), cn.detach()] + [t.grad for t in dev])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    grads = {}
    for storage in (False, True):
        ref = [t.clone().requires_grad_() for t in (x.float(), *prm, h0, c0)]
        _, _, cnr = _layer_oracle(*ref[:5], (T,) * B, ref[5], ref[6], storage=storage)
        (cnr * dcn).sum().backward()
        grads[storage] = [t.grad for t in ref]
    names = ("x", "w_ih", "w_hh", "b_ih", "b_hh", "h0", "c0")
    _band_check({n: (o, w, s) for n, o, w, s in zip(names, res[0][3:], grads[False], grads[True])})


# ---- the model ----------------------------------------------------------------------------------------
LENGTHS, CHUNK, HID, POS_W = (5, 2, 8), 3, 32, 1.7
TRAINABLE = [f"lstm.{w}_l{l}" for l in (0, 1) for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] + \
    ["classifier.0.weight", "classifier.0.bias", "classifier.3.weight", "classifier.3.bias"]


@pytest.fixture(scope="module")
def weights():
    return {k: torch.from_numpy(v) for k, v in make_resnet50_lstm_weights(seed=0, hidden=HID).items()}


@pytest.fixture(scope="module")
def model(weights):
    from vclip_amd.resnet50_lstm import VideoResNet50LSTM
    m = VideoResNet50LSTM(HID, 2, 0.0, freeze_backbone_bn=True)
    m.load_state_dict(weights)
    return m.to(DEV)


@pytest.fixture(scope="module")
def videos():
    return [torch.from_numpy(make_synthetic_video(1, n, 64, seed=11 + i)) for i, n in enumerate(LENGTHS)]


def _rounds(lengths, chunk):
    pos, out = [0] * len(lengths), []
    while any(p < n for p, n in zip(pos, lengths)):
        lens = [min(chunk, n - p) for p, n in zip(pos, lengths)]
        out.append((list(pos), lens))
        pos = [p + k for p, k in zip(pos, lens)]
    return out


def _round_clip(videos, pos, lens):
    return torch.cat([v[:, :, p:p + n] for v, p, n in zip(videos, pos, lens) if n], dim=2).to(DEV)


def _loss(logits, dev):
    labels = torch.tensor([[1.0], [0.0], [1.0]], device=dev)
    return F.binary_cross_entropy_with_logits(logits, labels, pos_weight=torch.tensor([POS_W], device=dev))


def _grads(model):
    return {n: model.P(n).grad.clone() for n in TRAINABLE}


def _model_oracle(p, feats, storage):
    """The two LSTM layers over the whole sequences from the zero state + head + loss, on the features
    [sum(LENGTHS), 2048]: {name: grad} and the logits."""
    q = {n: p[n].clone().requires_grad_() for n in TRAINABLE}
    B = len(LENGTHS)
    x = feats
    for l in (0, 1):
        z = torch.zeros(B, HID)
        x, hn, _ = _layer_oracle(x, q[f"lstm.weight_ih_l{l}"], q[f"lstm.weight_hh_l{l}"], q[f"lstm.bias_ih_l{l}"],
                                 q[f"lstm.bias_hh_l{l}"], LENGTHS, z, z, storage=storage)
        if storage:
            x = _Round.apply(x, True, True)  # inter-layer h_seq is stored bf16, and so is its gradient
    y = F.relu(hn @ q["classifier.0.weight"].T + q["classifier.0.bias"])
    logits = y @ q["classifier.3.weight"].T + q["classifier.3.bias"]
    _loss(logits, "cpu").backward()
    return {n: t.grad for n, t in q.items()}, logits.detach()


def test_full_bptt_over_chunks_matches_one_shot_training(model, weights, videos):
    """The state left attached between the chunks and one backward() from the final logits, against one call
    over the whole sequences (lstm_layer_state over the whole lengths) and against the fp32 oracle."""
    model.train()
    model.zero_grad()
    whole = torch.cat(videos, dim=2).to(DEV)
    logits1, st1 = model.forward_train_stream(whole, LENGTHS)
    feats = model.last_features.float().cpu()
    assert tuple(logits1.shape) == (3, 1) and tuple(st1.h.shape) == tuple(st1.c.shape) == (2, 3, HID)
    assert st1.h.requires_grad and st1.c.requires_grad and model.last_keep == {"lstm": [None, None], "head": None}
    _loss(logits1, DEV).backward()
    one_shot = _grads(model)
    model.zero_grad()
    state, parts = None, [[] for _ in LENGTHS]
    for pos, lens in _rounds(LENGTHS, CHUNK):
        logits, state = model.forward_train_stream(_round_clip(videos, pos, lens), lens, state)
        at = 0
        for b, n in enumerate(lens):
            parts[b].append(model.last_features[at:at + n].float().cpu())
            at += n
    _loss(logits, DEV).backward()  # the last round's logits: videos 0 and 1 ended earlier, their state passed through
    chunked = _grads(model)
    # the frames are independent through the backbone, but its GEMM picks depend on the row count: close, not equal
    print(f"features, rounds against whole: rel L2 {_rel(torch.cat([torch.cat(p) for p in parts]), feats):.2e}")
    want, wlogits = _model_oracle(weights, feats, False)
    stor, _ = _model_oracle(weights, feats, True)
    print(f"logits max |err|: one-shot {float((logits1.detach().cpu() - wlogits).abs().max()):.2e} "
          f"chunked {float((logits.detach().cpu() - wlogits).abs().max()):.2e}")
    assert float((logits1.detach().cpu() - wlogits).abs().max()) < 1e-2
    assert float((logits.detach().cpu() - wlogits).abs().max()) < 1e-2
    _band_check({n + " one-shot": (one_shot[n], want[n], stor[n]) for n in TRAINABLE})
    _band_check({n + " chunked": (chunked[n], want[n], stor[n]) for n in TRAINABLE})
    # and the chunked gradients around the one-shot ones, by the same attainable error
    bad = [(n, _rel(chunked[n], one_shot[n]), _rel(stor[n], want[n])) for n in TRAINABLE
           if not _rel(chunked[n], one_shot[n]) <= 1.5 * _rel(stor[n], want[n]) + 0.03]
    assert not bad, bad
    assert all(q.grad is None for q in model.backbone.parameters())


def test_detached_state_truncates_the_gradient_at_the_chunk(model, videos):
    model.train()
    rounds = _rounds(LENGTHS, CHUNK)
    model.zero_grad()
    state = None
    for pos, lens in rounds:
        before = state
        logits, state = model.forward_train_stream(_round_clip(videos, pos, lens), lens, state)
        state = state.detach()
        assert not state.h.requires_grad and state.h.grad_fn is None
    _loss(logits, DEV).backward()
    truncated = _grads(model)
    # the last chunk alone from the same, detached, state
    model.zero_grad()
    pos, lens = rounds[-1]
    logits2, _ = model.forward_train_stream(_round_clip(videos, pos, lens), lens, before)
    assert torch.equal(logits2, logits)
    _loss(logits2, DEV).backward()
    alone = _grads(model)
    for n in TRAINABLE:
        assert torch.equal(truncated[n], alone[n]), n
    # and it is not the full gradient: the first layer's input weights saw the last round's two frames only
    model.zero_grad()
    state = None
    for pos, lens in rounds:
        logits, state = model.forward_train_stream(_round_clip(videos, pos, lens), lens, state)
    _loss(logits, DEV).backward()
    assert _rel(truncated["lstm.weight_ih_l0"], model.P("lstm.weight_ih_l0").grad) > 1e-2


def test_train_forward_equals_forward_stream(model, videos):
    state_t = state_e = None
    for pos, lens in _rounds(LENGTHS, CHUNK):
        x = _round_clip(videos, pos, lens)
        model.train()
        with torch.no_grad():
            lt, new_t = model.forward_train_stream(x, lens, state_t)
        model.eval()
        le, new_e = model.forward_stream(x, lens, state_e)
        assert torch.equal(lt, le) and torch.equal(new_t.h, new_e.h) and torch.equal(new_t.c, new_e.c), lens
        state_t, state_e = new_t, new_e
    model.train()


def test_fresh_dropout_masks_per_call(weights, videos):
    from vclip_amd.resnet50_lstm import VideoResNet50LSTM
    m = VideoResNet50LSTM(HID, 2, 0.5, freeze_backbone_bn=True)
    m.load_state_dict(weights)
    m = m.to(DEV).train()
    pos, lens = _rounds(LENGTHS, CHUNK)[0]
    x = _round_clip(videos, pos, lens)
    torch.manual_seed(0)
    a, _ = m.forward_train_stream(x, lens)
    k0 = m.last_keep
    assert tuple(k0["lstm"][0].shape) == (sum(lens), HID) and k0["lstm"][1] is None and tuple(k0["head"].shape) == (3, 64)
    assert set(k0["lstm"][0].unique().tolist()) == {0.0, 2.0}
    b, _ = m.forward_train_stream(x, lens)
    assert not torch.equal(m.last_keep["lstm"][0], k0["lstm"][0])  # fresh masks
    torch.manual_seed(0)
    c, _ = m.forward_train_stream(x, lens)
    assert torch.equal(a, c) and not torch.equal(a, b)  # from torch's RNG


# ---- main.py --tbptt_chunk ----------------------------------------------------------------------------
HISTORY_KEYS = ("train_loss", "val_loss", "train_acc", "val_acc", "train_auroc", "val_auroc")
FRAMES = {"train": {"non_referral": (5, 11), "referral": (7, 9)}, "val": {"non_referral": (6, 10), "referral": (8,)},
          "test": {"non_referral": (9,), "referral": (6,)}}


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("tbptt_clips")
    rng = np.random.RandomState(0)
    for split, classes in FRAMES.items():
        for c, frames in classes.items():
            d = root / split / c
            d.mkdir(parents=True)
            for k, n in enumerate(frames):
                np.save(d / f"{c}_{split}_{k}.npy", rng.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8))
    return root


def _run(dataset, out, *extra):
    from vclip_amd.apps import run_main
    m, history, exp = run_main("lstm", ["--data_dir", str(dataset), "--log_dir", str(out / "logs"), "--model_dir",
                                        str(out / "models"), "--batch_size", "3", "--hidden_size", "32", "--sequence_length",
                                        "8", "--num_workers", "0", *extra])
    cks = sorted((out / "models").glob("model_*.pth"))
    assert len(cks) == 1, cks
    return m, history, Path(exp), cks[0]


@pytest.fixture(scope="module")
def trained(dataset, tmp_path_factory):
    return _run(dataset, tmp_path_factory.mktemp("tbptt_run"), "--tbptt_chunk", "4", "--epochs", "2")


def test_main_tbptt_trains_and_writes_the_files(trained):
    m, history, exp, ck = trained
    assert set(history) == set(HISTORY_KEYS)
    for k in HISTORY_KEYS:
        assert len(history[k]) == 2 and all(math.isfinite(v) for v in history[k]), (k, history[k])
    assert json.load(open(exp / "training_history.json")) == history
    cfg = json.load(open(exp / "training_config.json"))
    assert cfg["tbptt_chunk"] == 4 and cfg["batch_size"] == 3 and cfg["hidden_size"] == 32
    log = open(exp / "resnet50-lstm-training.log").read()
    assert "--tbptt_chunk 4" in log and "ignored" in log and "freeze_backbone_bn = True" in log
    assert "Error in" not in log  # no batch was skipped
    assert m is not None and np.asarray(m["confusion_matrix"]).sum() == 2  # the sampled test-set evaluation ran
    sd = torch.load(ck, weights_only=True)
    assert all(isinstance(v, torch.Tensor) for v in sd.values()) and tuple(sd["lstm.weight_hh_l1"].shape) == (128, 32)
    # the backbone's running statistics did not move
    w = make_resnet50_lstm_weights(seed=0, hidden=32)
    assert torch.equal(sd["resnet50.1.running_mean"].cpu(), torch.from_numpy(w["resnet50.1.running_mean"]))
    assert not torch.equal(sd["lstm.weight_hh_l0"].cpu(), torch.from_numpy(w["lstm.weight_hh_l0"]))  # the LSTM trained


def test_tbptt_checkpoint_loads_into_streaming_inference(dataset, trained, tmp_path):
    from vclip_amd.apps import run_inference
    summary = run_inference("lstm", ["--videos_dir", str(dataset / "test"), "--model_path", str(trained[3]), "--output_dir",
                                     str(tmp_path / "out"), "--batch_mode", "--stream_chunk", "4"])
    assert summary["successful_predictions"] == 2 and summary["failed_predictions"] == 0 and summary["stream_chunk"] == 4


def test_tbptt_seeded_rerun_is_bit_identical(dataset, trained, tmp_path):
    _, history, _, ck = _run(dataset, tmp_path, "--tbptt_chunk", "4", "--epochs", "2")
    assert history == trained[1]
    a, b = torch.load(trained[3], weights_only=True), torch.load(ck, weights_only=True)
    assert list(a) == list(b)
    for n in a:
        assert torch.equal(a[n], b[n]), n


def test_without_the_flag_the_default_trainer_runs(dataset, tmp_path, monkeypatch):
    from vclip_amd import apps

    def refuse(*a, **k):
        raise AssertionError("the --tbptt_chunk path ran without the flag")

    monkeypatch.setattr(apps, "lstm_tbptt_step", refuse)
    monkeypatch.setattr(apps, "LstmWholeVideoBatches", refuse)
    _, history, exp, ck = _run(dataset, tmp_path, "--epochs", "1")
    for k in HISTORY_KEYS:
        assert len(history[k]) == 1 and math.isfinite(history[k][0]), (k, history[k])
    assert json.load(open(exp / "training_config.json"))["tbptt_chunk"] == 0
    log = open(exp / "resnet50-lstm-training.log").read()
    assert "--tbptt_chunk" not in log and "Error in" not in log
    sd = torch.load(ck, weights_only=True)
    w = make_resnet50_lstm_weights(seed=0, hidden=32)
    # the reference's train mode: batch-statistic BatchNorm moved the running statistics
    assert not torch.equal(sd["resnet50.1.running_mean"].cpu(), torch.from_numpy(w["resnet50.1.running_mean"]))
