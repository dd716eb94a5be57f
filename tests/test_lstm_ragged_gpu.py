"""The ragged inference recurrence (vc_lstm_seq_fwd_ragged, ops.lstm_seq_fwd_ragged) and
VideoResNet50LSTM.forward_ragged on the GPU.

Kernel: every sequence of a ragged batch bit-identical to the dense kernel run on that sequence alone
(torch.equal on h_seq and h_last), nothing written outside the sequences' rows, equal lengths bit-identical
to the dense call, reruns bit-identical; h_last against torch's cell arithmetic in fp32 within the dense
kernel's bound (tests/test_lstm_gpu.py: 1e-5).  Model: forward_ragged against the fp32 oracle per video and
against model(video) per video, both within the 1e-2 of test_lstm_gpu.test_eval_logits_match_oracle."""
import numpy as np
import pytest
import torch

from oracle.lstm_ref import lstm_forward
from vclip_amd.weights import make_resnet50_lstm_weights, make_synthetic_video

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 7.0
# one full and one partial group at G = 4 (three groups at G = 2); a first step that is also the last
LENGTHS = [1, 7, 3, 7, 2, 5]
GAP = 2
# hidden: HP = 64; HP = 128 with padded lanes; the workload's; the G = 2 path with S = 1
HIDDEN = [32, 100, 256, 516]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vclip_amd import _lib
    _lib.load()


_CASE = {}


def _case(H):
    """(w_hh [4H, H], per-sequence pre [len, 4H]) on the host, once per hidden size."""
    if H not in _CASE:
        g = torch.Generator().manual_seed(77 + H)
        w_hh = (torch.rand(4 * H, H, generator=g) * 2 - 1) / np.sqrt(H)
        _CASE[H] = (w_hh, [torch.randn(n, 4 * H, generator=g) for n in LENGTHS])
    return _CASE[H]


def _row0(lengths, gap):
    out, r = [], 0
    for n in lengths:
        out.append(r)
        r += n + gap
    return out, r


def _run_ragged(H, w_hh, pres, row0, rows):
    from vclip_amd import ops
    lengths = [p.shape[0] for p in pres]
    pre = torch.full((rows, 4 * H), float("nan"))  # a gap row that was read would poison its sequence
    for r, p in zip(row0, pres):
        pre[r: r + p.shape[0]] = p
    h_seq = torch.full((rows, H), SENT, dtype=torch.bfloat16, device=DEV)
    h_last = torch.full((len(pres) + 1, H), SENT, device=DEV)
    ops.lstm_seq_fwd_ragged(pre.to(DEV), lengths, H, w_hh.t().contiguous().to(DEV), h_seq, h_last, row0=row0)
    torch.cuda.synchronize()
    return h_seq.cpu(), h_last.cpu()


def _run_dense(H, w_hh, pre, B, T):
    from vclip_amd import ops
    h_seq = torch.empty(B * T, H, dtype=torch.bfloat16, device=DEV)
    h_last = torch.empty(B, H, device=DEV)
    ops.lstm_seq_fwd(pre.reshape(B * T, 4 * H).contiguous().to(DEV), B, T, H, w_hh.t().contiguous().to(DEV), h_seq, h_last)
    torch.cuda.synchronize()
    return h_seq.cpu(), h_last.cpu()


@pytest.mark.parametrize("H", HIDDEN)
def test_ragged_equals_dense_per_sequence(H):
    w_hh, pres = _case(H)
    row0, rows = _row0(LENGTHS, GAP)
    h_seq, h_last = _run_ragged(H, w_hh, pres, row0, rows)
    owned = torch.zeros(rows, dtype=torch.bool)
    for b, (r, p) in enumerate(zip(row0, pres)):
        n = p.shape[0]
        want_seq, want_last = _run_dense(H, w_hh, p, 1, n)
        assert torch.equal(h_seq[r: r + n], want_seq), f"h_seq of sequence {b} (len {n})"
        assert torch.equal(h_last[b], want_last[0]), f"h_last of sequence {b} (len {n})"
        owned[r: r + n] = True
    # every gap row, every row past the end and the spare h_last row still hold the sentinel
    assert int((~owned).sum()) == GAP * len(LENGTHS)
    assert bool((h_seq[~owned].float() == SENT).all())
    assert bool((h_last[len(LENGTHS)] == SENT).all())
    again = _run_ragged(H, w_hh, pres, row0, rows)
    assert torch.equal(again[0], h_seq) and torch.equal(again[1], h_last)


@pytest.mark.parametrize("H", HIDDEN)
def test_ragged_equal_lengths_equals_dense_batch(H):
    B, T = 6, 5
    g = torch.Generator().manual_seed(5 + H)
    w_hh = (torch.rand(4 * H, H, generator=g) * 2 - 1) / np.sqrt(H)
    pre = torch.randn(B, T, 4 * H, generator=g)
    h_seq, h_last = _run_ragged(H, w_hh, list(pre), [b * T for b in range(B)], B * T)
    want_seq, want_last = _run_dense(H, w_hh, pre, B, T)
    assert torch.equal(h_seq, want_seq) and torch.equal(h_last[:B], want_last)


def test_ragged_default_row0_is_prefix_sum():
    from vclip_amd import ops
    H = 32
    w_hh, pres = _case(H)
    row0, rows = _row0(LENGTHS, 0)
    want_seq, want_last = _run_ragged(H, w_hh, pres, row0, rows)
    h_seq = torch.empty(rows, H, dtype=torch.bfloat16, device=DEV)
    h_last = torch.empty(len(pres), H, device=DEV)
    ops.lstm_seq_fwd_ragged(torch.cat(pres).to(DEV), LENGTHS, H, w_hh.t().contiguous().to(DEV), h_seq, h_last)
    assert torch.equal(h_seq.cpu(), want_seq) and torch.equal(h_last.cpu(), want_last[: len(pres)])


def test_ragged_h_last_matches_torch_cell_loop():
    H = 256
    w_hh, pres = _case(H)
    row0, rows = _row0(LENGTHS, GAP)
    _, h_last = _run_ragged(H, w_hh, pres, row0, rows)
    worst = 0.0
    for b, pre in enumerate(pres):
        h, c = torch.zeros(H), torch.zeros(H)
        for t in range(pre.shape[0]):  # nn.LSTM's cell arithmetic, gate order i, f, g, o, zero initial state
            a = pre[t] + w_hh @ h
            i, f, gg, o = torch.sigmoid(a[:H]), torch.sigmoid(a[H:2 * H]), torch.tanh(a[2 * H:3 * H]), torch.sigmoid(a[3 * H:])
            c = f * c + i * gg
            h = o * torch.tanh(c)
        worst = max(worst, float((h_last[b] - h).abs().max()))
    print(f"ragged h_last vs the fp32 cell loop, H={H}: max |err| {worst:.2e}")
    assert worst < 1e-5


def test_ragged_entry_point_length_zero_and_clamp():
    """The C entry point itself (ops refuses a length 0): a sequence of length 0 gets a zero h_last row and
    nothing else; a length above max_len is clamped to it (the buffers here hold the unclamped rows too)."""
    from vclip_amd import _lib
    H, max_len = 32, 4
    w_hh, pres = _case(H)
    lens, row0 = [3, 0, 9, 0, 2], [0, 3, 3, 12, 12]  # 9 > max_len: runs 4 steps
    rows = 14
    pre = torch.randn(rows, 4 * H, generator=torch.Generator().manual_seed(3))
    h_seq = torch.full((rows, H), SENT, dtype=torch.bfloat16, device=DEV)
    h_last = torch.full((len(lens) + 1, H), SENT, device=DEV)
    d_pre, wt = pre.to(DEV), w_hh.t().contiguous().to(DEV)
    d_row0 = torch.tensor(row0, dtype=torch.int32, device=DEV)
    d_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    _lib.call("vc_lstm_seq_fwd_ragged", d_pre.data_ptr(), d_pre.stride(0), len(lens), d_row0.data_ptr(), d_len.data_ptr(),
              max_len, H, wt.data_ptr(), h_seq.data_ptr(), h_seq.stride(0), h_last.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h_seq, h_last = h_seq.cpu(), h_last.cpu()
    for b, (r, n) in enumerate(zip(row0, lens)):
        n = min(n, max_len)
        if n == 0:
            assert bool((h_last[b] == 0).all()), b
            continue
        want_seq, want_last = _run_dense(H, w_hh, pre[r: r + n], 1, n)
        assert torch.equal(h_seq[r: r + n], want_seq) and torch.equal(h_last[b], want_last[0]), b
    assert bool((h_seq[7:12].float() == SENT).all())  # rows 3 + 4 .. 11: past the clamped end of sequence 2
    assert bool((h_last[len(lens)] == SENT).all())


def test_ragged_refusals():
    from vclip_amd import ops
    from vclip_amd._lib import VclipError
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    H = 32
    pre, rest = z(12, 4 * H), (H, z(H, 4 * H), z(12, H, dt=torch.bfloat16), z(3, H))
    with pytest.raises(VclipError, match="lengths"):
        ops.lstm_seq_fwd_ragged(pre, [4, 0, 3], *rest)
    with pytest.raises(VclipError, match="overlap"):
        ops.lstm_seq_fwd_ragged(pre, [4, 4, 3], *rest, row0=[0, 3, 8])
    with pytest.raises(VclipError, match="past"):
        ops.lstm_seq_fwd_ragged(pre, [4, 4, 5], *rest)  # 13 rows wanted, 12 there
    with pytest.raises(VclipError, match="past"):
        ops.lstm_seq_fwd_ragged(pre, [4, 4, 3], *rest, row0=[0, 4, 10])
    with pytest.raises(VclipError, match="hidden"):
        ops.lstm_seq_fwd_ragged(z(12, 120), [4, 4, 3], 30, z(30, 120), z(12, 30, dt=torch.bfloat16), z(3, 30))


# ---- the model -----------------------------------------------------------------------------------
VIDEO_LENGTHS = [5, 2, 8]


@pytest.fixture(scope="module")
def weights():
    return {k: torch.from_numpy(v) for k, v in make_resnet50_lstm_weights(seed=0).items()}


@pytest.fixture(scope="module")
def model(weights):
    from vclip_amd.resnet50_lstm import VideoResNet50LSTM
    m = VideoResNet50LSTM(256, 2, 0.5)
    m.load_state_dict(weights)
    return m.to(DEV).eval()


def test_forward_ragged_matches_oracle_and_single_video(weights, model):
    videos = [torch.from_numpy(make_synthetic_video(1, n, 64, seed=11 + i)) for i, n in enumerate(VIDEO_LENGTHS)]
    with torch.no_grad():
        want = torch.cat([lstm_forward(weights, v) for v in videos])  # fp32 oracle, one video at a time
    got = model.forward_ragged(torch.cat(videos, dim=2).to(DEV), VIDEO_LENGTHS).cpu()
    assert tuple(got.shape) == (len(VIDEO_LENGTHS), 1) and got.dtype == torch.float32
    single = torch.cat([model(v.to(DEV)).cpu() for v in videos])
    e_oracle, e_single = float((got - want).abs().max()), float((got - single).abs().max())
    print(f"forward_ragged lengths {VIDEO_LENGTHS} 64^2: vs oracle {e_oracle:.2e}, vs model(video) one at a time {e_single:.2e}")
    assert e_oracle < 1e-2, (got, want)
    assert e_single < 1e-2, (got, single)
    again = model.forward_ragged(torch.cat(videos, dim=2).to(DEV), VIDEO_LENGTHS).cpu()
    assert torch.equal(again, got)


def test_forward_ragged_refuses_training_mode_and_bad_lengths(model):
    video = torch.zeros(1, 3, 4, 64, 64, device=DEV)
    with pytest.raises(ValueError, match="lengths"):
        model.forward_ragged(video, [2, 3])
    with pytest.raises(ValueError, match="lengths"):
        model.forward_ragged(video, [4, 0])
    model.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            model.forward_ragged(video, [2, 2])
    finally:
        model.eval()
