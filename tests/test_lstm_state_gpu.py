"""The stateful inference recurrence (vc_lstm_seq_fwd_state, ops.lstm_seq_fwd_state) on the GPU.

Every sequence is run in chunks with the state carried IN PLACE (h_n = h0, c_n = c0) and compared
  - with torch's cell arithmetic on the CPU in fp32, one shot over the whole sequence from the same pre:
    h_n, c_n and h_all within 1e-5, the bf16 h_seq within 8e-3 (the bounds of tests/test_lstm_gpu.py);
  - bit for bit (torch.equal) with the existing entry points on the whole sequence: h_seq and the final h
    with ops.lstm_seq_fwd_ragged (ragged cases) / ops.lstm_seq_fwd (dense cases), the final c with the last
    c_seq row of the dense train variant.
Further bit-identities: an explicit zero state and the NULL state, separate h_n / c_n buffers and the
in-place update, a rerun and the first run, the state of a sequence of length 0 before and after.  Rows
of pre outside every sequence hold NaN and the rows of every output behind the real ones a sentinel.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 7.0
TOL_F32, TOL_BF16 = 1e-5, 8e-3

# (B, total T, H, chunk lengths)
DENSE = [(1, 3, 32, [1, 1, 1]),      # every step is a step 0 with state
         (5, 7, 100, [3, 4]),        # hidden % 64 != 0, B one over the group of 4
         (3, 8, 256, [5, 3]),
         (2, 4, 512, [1, 3]),
         (3, 6, 1024, [2, 4])]       # group of 2, B one over it
RAGGED_H = [64, 256, 520]            # 520: G = 2 with one slice
TOTALS = (5, 2, 8, 3, 1)
ROUNDS = [(3, 2, 3, 3, 1), (2, 0, 3, 0, 0), (0, 0, 2, 0, 0)]  # H <= 512: the second workgroup is all-zero in round 2
GAP = 1


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vclip_amd import _lib
    _lib.load()


def _weights(H, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(4 * H, H, generator=g) * 2 - 1) / np.sqrt(H), g


def _cell_loop(w_hh, pre):
    """nn.LSTM's cell arithmetic in fp32 on the CPU, gate order i, f, g, o, zero initial state: pre [T, 4H] ->
    (h of every step [T, H], final c [H])."""
    H = w_hh.shape[1]
    h, c, hs = torch.zeros(H), torch.zeros(H), []
    for t in range(pre.shape[0]):
        a = pre[t] + w_hh @ h
        i, f, gg, o = torch.sigmoid(a[:H]), torch.sigmoid(a[H:2 * H]), torch.tanh(a[2 * H:3 * H]), torch.sigmoid(a[3 * H:])
        c = f * c + i * gg
        h = o * torch.tanh(c)
        hs.append(h)
    return torch.stack(hs), c


def _dense_whole(H, w_hh, pre):
    """ops.lstm_seq_fwd, train variant, on pre [B, T, 4H]: (h_seq bf16 [B, T, H], h_last [B, H], last c_seq rows [B, H])."""
    from vclip_amd import ops
    B, T = pre.shape[:2]
    z = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=DEV)  # noqa: E731
    h_seq, h_last = z(B * T, H, dt=torch.bfloat16), z(B, H)
    gates, c_seq, h_prev = z(B * T, 4 * H), z(B * T, H), z(B * T, H, dt=torch.bfloat16)
    ops.lstm_seq_fwd(pre.reshape(B * T, 4 * H).contiguous().to(DEV), B, T, H, w_hh.t().contiguous().to(DEV), h_seq, h_last,
                     gates=gates, c_seq=c_seq, h_prev=h_prev)
    torch.cuda.synchronize()
    return h_seq.cpu().reshape(B, T, H), h_last.cpu(), c_seq.cpu().reshape(B, T, H)[:, -1]


class _Buffers:
    """pre with NaN rows and sentinel-filled outputs of `rows` real rows plus `extra` behind them; the state
    of B sequences as the first B rows of buffers with one sentinel row more."""

    def __init__(self, rows, extra, B, H):
        self.rows, self.B = rows, B
        self.pre = torch.full((rows + extra, 4 * H), float("nan"))
        self.h_seq = torch.full((rows + extra, H), SENT, dtype=torch.bfloat16, device=DEV)
        self.h_all = torch.full((rows + extra, H), SENT, device=DEV)

    def untouched(self, owned):
        """every row no sequence owns still holds the sentinel"""
        free = ~owned
        return bool((self.h_seq.cpu()[free].float() == SENT).all()) and bool((self.h_all.cpu()[free] == SENT).all())


def _state(B, H, zero=True):
    buf = torch.full((B + 1, H), SENT, device=DEV)
    if zero:
        buf[:B] = 0
    return buf


def _run_dense_chunks(B, T, H, chunks, w_hh, pre, first="null", in_place=True):
    """pre [B, T, 4H] in chunks over the dense layout.  first: the first chunk starts from the NULL state
    or from an explicit zero state.  Returns (h_seq [B, T, H] bf16, h_all [B, T, H], h_n, c_n [B, H])."""
    from vclip_amd import ops
    wt = w_hh.t().contiguous().to(DEV)
    hbuf, cbuf = _state(B, H), _state(B, H)
    h, c = hbuf[:B], cbuf[:B]
    seq, full, t0 = [], [], 0
    for k, n in enumerate(chunks):
        buf = _Buffers(B * n, 3, B, H)
        buf.pre[: B * n] = pre[:, t0:t0 + n].reshape(B * n, 4 * H)
        null = k == 0 and first == "null"
        if in_place:
            hn, cn = h, c
        else:
            hnb, cnb = _state(B, H, zero=False), _state(B, H, zero=False)
            hn, cn = hnb[:B], cnb[:B]
        ops.lstm_seq_fwd_state(buf.pre.to(DEV), None, H, wt, buf.h_seq, hn, cn, h0=None if null else h,
                               c0=None if null else c, h_all=buf.h_all, T=n)
        torch.cuda.synchronize()
        owned = torch.zeros(B * n + 3, dtype=torch.bool)
        owned[: B * n] = True
        assert buf.untouched(owned), f"chunk {k}: a row behind the sequences was written"
        if not in_place:
            assert bool((hnb[B] == SENT).all()) and bool((cnb[B] == SENT).all())
            h, c = hn, cn
        seq.append(buf.h_seq[: B * n].cpu().reshape(B, n, H))
        full.append(buf.h_all[: B * n].cpu().reshape(B, n, H))
        t0 += n
    assert bool((hbuf[B] == SENT).all()) and bool((cbuf[B] == SENT).all()), "the row behind the state was written"
    return torch.cat(seq, 1), torch.cat(full, 1), h.cpu().clone(), c.cpu().clone()


@pytest.mark.parametrize("B,T,H,chunks", DENSE, ids=[f"B{c[0]}-T{c[1]}-H{c[2]}" for c in DENSE])
def test_dense_chunks_carry_the_state_in_place(B, T, H, chunks):
    assert sum(chunks) == T
    w_hh, g = _weights(H, 31 + H)
    pre = torch.randn(B, T, 4 * H, generator=g)
    h_seq, h_all, h_n, c_n = _run_dense_chunks(B, T, H, chunks, w_hh, pre)
    for t in (h_seq.float(), h_all, h_n, c_n):
        assert bool(torch.isfinite(t).all())
    # against the fp32 cell loop, one shot
    e = dict(h_n=0.0, c_n=0.0, h_all=0.0, h_seq=0.0)
    for b in range(B):
        hs, c = _cell_loop(w_hh, pre[b])
        e["h_n"] = max(e["h_n"], float((h_n[b] - hs[-1]).abs().max()))
        e["c_n"] = max(e["c_n"], float((c_n[b] - c).abs().max()))
        e["h_all"] = max(e["h_all"], float((h_all[b] - hs).abs().max()))
        e["h_seq"] = max(e["h_seq"], float((h_seq[b].float() - hs).abs().max()))
    print(f"state kernel dense B={B} T={T} H={H} chunks={chunks} vs the fp32 cell loop: " +
          ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["h_n"] < TOL_F32 and e["c_n"] < TOL_F32 and e["h_all"] < TOL_F32 and e["h_seq"] < TOL_BF16, e
    # bit for bit against the one-shot dense kernel (train variant for c)
    want_seq, want_last, want_c = _dense_whole(H, w_hh, pre)
    assert torch.equal(h_seq, want_seq), "chunked h_seq != one-shot h_seq"
    assert torch.equal(h_n, want_last), "chunked h_n != one-shot h_last"
    assert torch.equal(c_n, want_c), "chunked c_n != the last c_seq row"
    assert torch.equal(h_all[:, -1], h_n)
    # an explicit zero state == the NULL state; separate outputs == in place; a rerun == the first run
    for kw in (dict(first="zeros"), dict(in_place=False), dict()):
        again = _run_dense_chunks(B, T, H, chunks, w_hh, pre, **kw)
        for a, b_, what in zip(again, (h_seq, h_all, h_n, c_n), ("h_seq", "h_all", "h_n", "c_n")):
            assert torch.equal(a, b_), (kw, what)


_RAGGED = {}


def _ragged_case(H):
    """(w_hh, per-sequence pre, the whole sequences through ops.lstm_seq_fwd_ragged and the dense train
    variant, the cell loop's results), once per hidden size."""
    if H not in _RAGGED:
        from vclip_amd import ops
        w_hh, g = _weights(H, 77 + H)
        pres = [torch.randn(n, 4 * H, generator=g) for n in TOTALS]
        h_seq = torch.empty(sum(TOTALS), H, dtype=torch.bfloat16, device=DEV)
        h_last = torch.empty(len(TOTALS), H, device=DEV)
        ops.lstm_seq_fwd_ragged(torch.cat(pres).to(DEV), TOTALS, H, w_hh.t().contiguous().to(DEV), h_seq, h_last)
        torch.cuda.synchronize()
        whole_seq = list(h_seq.cpu().split(TOTALS))
        whole_c = [_dense_whole(H, w_hh, p[None])[2][0] for p in pres]
        _RAGGED[H] = (w_hh, pres, whole_seq, h_last.cpu(), whole_c, [_cell_loop(w_hh, p) for p in pres])
    return _RAGGED[H]


def _run_ragged_rounds(H, w_hh, pres, explicit_zero=False):
    from vclip_amd import ops
    B = len(TOTALS)
    wt = w_hh.t().contiguous().to(DEV)
    hbuf, cbuf = _state(B, H), _state(B, H)
    h, c = hbuf[:B], cbuf[:B]
    seq, full, pos = [[] for _ in TOTALS], [[] for _ in TOTALS], [0] * B
    for k, lens in enumerate(ROUNDS):
        row0, r = [], GAP  # a NaN row in front of, between and behind the sequences; an empty one owns no row
        for n in lens:
            row0.append(r if n else 0)
            r += n + GAP if n else 0
        buf = _Buffers(r, 2, B, H)
        owned = torch.zeros(r + 2, dtype=torch.bool)
        for b, n in enumerate(lens):
            buf.pre[row0[b]: row0[b] + n] = pres[b][pos[b]: pos[b] + n]
            owned[row0[b]: row0[b] + n] = True
        before = (h.clone(), c.clone())
        null = k == 0 and not explicit_zero
        ops.lstm_seq_fwd_state(buf.pre.to(DEV), lens, H, wt, buf.h_seq, h, c, h0=None if null else h, c0=None if null else c,
                               h_all=buf.h_all, row0=row0)
        torch.cuda.synchronize()
        assert buf.untouched(owned), f"round {k}: a row outside the sequences was written"
        for b, n in enumerate(lens):
            if n == 0:  # the state passes through, bit for bit
                assert torch.equal(h[b], before[0][b]) and torch.equal(c[b], before[1][b]), (k, b)
            seq[b].append(buf.h_seq[row0[b]: row0[b] + n].cpu())
            full[b].append(buf.h_all[row0[b]: row0[b] + n].cpu())
            pos[b] += n
    assert pos == list(TOTALS)
    assert bool((hbuf[B] == SENT).all()) and bool((cbuf[B] == SENT).all())
    return [torch.cat(s) for s in seq], [torch.cat(s) for s in full], h.cpu().clone(), c.cpu().clone()


@pytest.mark.parametrize("H", RAGGED_H)
def test_ragged_rounds_with_finished_sequences(H):
    w_hh, pres, whole_seq, whole_last, whole_c, ref = _ragged_case(H)
    h_seq, h_all, h_n, c_n = _run_ragged_rounds(H, w_hh, pres)
    e = dict(h_n=0.0, c_n=0.0, h_all=0.0, h_seq=0.0)
    for b, (hs, c) in enumerate(ref):
        for t in (h_seq[b].float(), h_all[b], h_n[b], c_n[b]):
            assert bool(torch.isfinite(t).all()), b
        e["h_n"] = max(e["h_n"], float((h_n[b] - hs[-1]).abs().max()))
        e["c_n"] = max(e["c_n"], float((c_n[b] - c).abs().max()))
        e["h_all"] = max(e["h_all"], float((h_all[b] - hs).abs().max()))
        e["h_seq"] = max(e["h_seq"], float((h_seq[b].float() - hs).abs().max()))
        assert torch.equal(h_seq[b], whole_seq[b]), f"sequence {b}: chunked h_seq != ops.lstm_seq_fwd_ragged on it whole"
        assert torch.equal(h_n[b], whole_last[b]), f"sequence {b}: h_n"
        assert torch.equal(c_n[b], whole_c[b]), f"sequence {b}: c_n != the dense train variant's last c_seq row"
        assert torch.equal(h_all[b][-1], h_n[b])
    print(f"state kernel ragged H={H} totals={TOTALS} vs the fp32 cell loop: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["h_n"] < TOL_F32 and e["c_n"] < TOL_F32 and e["h_all"] < TOL_F32 and e["h_seq"] < TOL_BF16, e
    for kw in (dict(explicit_zero=True), dict()):  # zero state == NULL state; a rerun == the first run
        again = _run_ragged_rounds(H, w_hh, pres, **kw)
        for b in range(len(TOTALS)):
            assert torch.equal(again[0][b], h_seq[b]) and torch.equal(again[1][b], h_all[b]), (kw, b)
        assert torch.equal(again[2], h_n) and torch.equal(again[3], c_n), kw


def test_all_sequences_empty_pass_a_nonzero_state_through():
    """No step runs in any workgroup: h_n / c_n still get the incoming state (separate buffers), or zeros from
    the NULL state; without h_all."""
    from vclip_amd import ops
    H, B = 64, 5
    g = torch.Generator().manual_seed(9)
    h0, c0 = torch.randn(B, H, generator=g).to(DEV), torch.randn(B, H, generator=g).to(DEV)
    pre = torch.full((4, 4 * H), float("nan"), device=DEV)
    h_seq = torch.full((4, H), SENT, dtype=torch.bfloat16, device=DEV)
    wt = torch.randn(H, 4 * H, generator=g).to(DEV)
    h_n, c_n = torch.full((B, H), SENT, device=DEV), torch.full((B, H), SENT, device=DEV)
    ops.lstm_seq_fwd_state(pre, [0] * B, H, wt, h_seq, h_n, c_n, h0=h0, c0=c0)
    assert torch.equal(h_n, h0) and torch.equal(c_n, c0)
    ops.lstm_seq_fwd_state(pre, [0] * B, H, wt, h_seq, h_n, c_n)
    assert not h_n.any() and not c_n.any()
    assert bool((h_seq.float() == SENT).all())
