"""Training on whole videos with a carried LSTM state, the host side without a GPU: the declarations and
ctypes signatures of vc_lstm_seq_fwd_train_state / vc_lstm_seq_bwd_state next to the unchanged forward entry
points, their argument validation before any HIP call, the refusals of the two ops wrappers, the
--tbptt_chunk flag, forward_train_stream's refusals and the (video, round) loss weights."""
import ctypes

import pytest
import torch

import vclip_amd._lib as L
from vclip_amd import apps, ops
from vclip_amd._lib import VclipError


def test_entry_points_declared_bound_and_exported():
    from vclip_amd.build import LIB_PATH, build
    names = L.header_functions()
    for name, nargs in (("vc_lstm_seq_fwd_train_state", 20), ("vc_lstm_seq_bwd_state", 20)):
        assert name in names
        argtypes, restype = L.SIGNATURES[name]
        assert len(argtypes) == nargs and restype is ctypes.c_int
    assert len(L.SIGNATURES["vc_lstm_seq_fwd"][0]) == 15  # the existing entry points keep their signatures
    assert len(L.SIGNATURES["vc_lstm_seq_fwd_ragged"][0]) == 12
    assert len(L.SIGNATURES["vc_lstm_seq_fwd_state"][0]) == 17
    assert len(L.SIGNATURES["vc_lstm_seq_bwd"][0]) == 14
    build()
    lib = ctypes.CDLL(LIB_PATH)
    assert hasattr(lib, "vc_lstm_seq_fwd_train_state") and hasattr(lib, "vc_lstm_seq_bwd_state")


def test_fwd_train_state_validates_before_any_hip_call():
    from vclip_amd.build import build
    build()
    lib = L.load()
    p = ctypes.c_void_p(64)
    good = dict(pre=p, ldpre=1024, B=3, row0=p, len=p, max_len=8, hidden=256, w=p, h0=p, c0=p, keep=p, hseq=p, ldh=256,
                hn=p, cn=p, gates=p, cseq=p, hprev=p, ldhp=256)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vc_lstm_seq_fwd_train_state(a["pre"], a["ldpre"], a["B"], a["row0"], a["len"], a["max_len"], a["hidden"],
                                             a["w"], a["h0"], a["c0"], a["keep"], a["hseq"], a["ldh"], a["hn"], a["cn"],
                                             a["gates"], a["cseq"], a["hprev"], a["ldhp"], None)
        return rc, lib.vc_last_error().decode()

    for name in ("pre", "w", "hseq", "hn", "cn", "gates", "cseq", "hprev"):
        rc, msg = call(**{name: None})
        assert rc != 0 and "null" in msg and "vc_lstm_seq_fwd_train_state" in msg, name
    for name, word in (("row0", "row0 and len"), ("len", "row0 and len"), ("h0", "h0 and c0"), ("c0", "h0 and c0")):
        rc, msg = call(**{name: None})  # exactly one of a pair
        assert rc != 0 and word in msg, (name, msg)
    for kw, word in ((dict(B=0), ">= 1"), (dict(max_len=0), ">= 1"), (dict(hidden=30), "hidden"), (dict(hidden=1028), "hidden"),
                     (dict(ldpre=1023), "stride"), (dict(ldh=255), "stride"), (dict(ldhp=255), "stride")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg and "vc_lstm_seq_fwd_train_state" in msg, (kw, msg)


def test_bwd_state_validates_before_any_hip_call():
    from vclip_amd.build import build
    build()
    lib = L.load()
    p = ctypes.c_void_p(64)
    good = dict(gates=p, cseq=p, c0=p, B=3, row0=p, len=p, max_len=8, hidden=256, w=p, dhseq=p, lddh=256, keep=p, dhn=p,
                dcn=p, dpre=p, dpb=p, lddb=1024, dh0=p, dc0=p)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vc_lstm_seq_bwd_state(a["gates"], a["cseq"], a["c0"], a["B"], a["row0"], a["len"], a["max_len"],
                                       a["hidden"], a["w"], a["dhseq"], a["lddh"], a["keep"], a["dhn"], a["dcn"], a["dpre"],
                                       a["dpb"], a["lddb"], a["dh0"], a["dc0"], None)
        return rc, lib.vc_last_error().decode()

    for name in ("gates", "cseq", "w", "dpre", "dpb"):
        rc, msg = call(**{name: None})
        assert rc != 0 and "null" in msg and "vc_lstm_seq_bwd_state" in msg, name
    for name, word in (("row0", "row0 and len"), ("len", "row0 and len"), ("dh0", "dh0 and dc0"), ("dc0", "dh0 and dc0")):
        rc, msg = call(**{name: None})  # exactly one of a pair
        assert rc != 0 and word in msg, (name, msg)
    for kw, word in ((dict(B=0), ">= 1"), (dict(max_len=0), ">= 1"), (dict(hidden=30), "hidden"), (dict(hidden=1028), "hidden"),
                     (dict(lddh=255), "stride"), (dict(lddb=1023), "stride")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg and "vc_lstm_seq_bwd_state" in msg, (kw, msg)


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on the GPU: reaches the host checks behind the device check.  Every
    refusal below is raised before any pointer is handed to the library."""

    @property
    def device(self):
        return torch.device("cuda", 0)


def _z(*s, dt=torch.float32):
    return torch.zeros(*s, dtype=dt).as_subclass(_FakeCuda)


def test_ops_fwd_train_state_refusals():
    H = 32
    pre, w, hseq = _z(12, 4 * H), _z(H, 4 * H), _z(12, H, dt=torch.bfloat16)
    st = lambda B=3: _z(B, H)  # noqa: E731
    saved = lambda rows=12: dict(gates=_z(rows, 4 * H), c_seq=_z(rows, H), h_prev=_z(rows, H, dt=torch.bfloat16))  # noqa: E731
    f = ops.lstm_seq_fwd_train_state
    with pytest.raises(VclipError, match="h0 and c0"):
        f(pre, [4, 4, 3], H, w, hseq, st(), st(), **saved(), h0=st())
    with pytest.raises(VclipError, match="lengths"):
        f(pre, [4, -1, 3], H, w, hseq, st(), st(), **saved())
    with pytest.raises(VclipError, match="overlap"):
        f(pre, [4, 4, 3], H, w, hseq, st(), st(), **saved(), row0=[0, 3, 8])
    with pytest.raises(VclipError, match="past"):
        f(pre, [4, 4, 5], H, w, hseq, st(), st(), **saved())  # 13 rows wanted, 12 there
    with pytest.raises(VclipError, match="past"):
        f(pre, [4, 4, 3], H, w, hseq, st(), st(), **saved(10))  # the saved tensors shorter than the rows
    with pytest.raises(VclipError, match="past"):
        f(pre, [4, 4, 3], H, w, hseq, st(), st(), **saved(), keep=_z(10, H))
    with pytest.raises(VclipError, match="gates"):
        f(pre, [4, 4, 3], H, w, hseq, st(), st(), **dict(saved(), gates=_z(12, 4 * H, dt=torch.float64)))
    with pytest.raises(VclipError, match="pre f32"):
        f(pre, None, H, w, hseq, st(), st(), **saved(15), T=5)  # dense: 15 rows wanted
    with pytest.raises(VclipError, match="hidden"):
        f(_z(12, 120), [4, 4, 3], 30, _z(30, 120), _z(12, 30, dt=torch.bfloat16), _z(3, 30), _z(3, 30), _z(12, 120),
          _z(12, 30), _z(12, 30, dt=torch.bfloat16))
    with pytest.raises(VclipError, match="one row per sequence"):
        f(pre, [4, 4, 3], H, w, hseq, st(2), st(2), **saved())
    with pytest.raises(VclipError, match="alias"):
        s = st()
        f(pre, [4, 4, 3], H, w, hseq, s, s, **saved())  # h_n and c_n in one buffer
    with pytest.raises(VclipError, match="dense layout"):
        f(pre, None, H, w, hseq, st(), st(), **saved())  # neither lengths nor T
    z = torch.zeros
    with pytest.raises(VclipError, match="no CPU path"):  # plain CPU tensors
        f(z(12, 4 * H), [4, 4, 3], H, z(H, 4 * H), z(12, H, dtype=torch.bfloat16), z(3, H), z(3, H), z(12, 4 * H), z(12, H),
          z(12, H, dtype=torch.bfloat16))


def test_ops_bwd_state_refusals():
    H = 32
    gates, cseq, w = _z(12, 4 * H), _z(12, H), _z(4 * H, H)
    out = lambda rows=12: dict(dpre=_z(rows, 4 * H), dpre_bf16=_z(rows, 4 * H, dt=torch.bfloat16))  # noqa: E731
    st = lambda B=3: _z(B, H)  # noqa: E731
    f = ops.lstm_seq_bwd_state
    with pytest.raises(VclipError, match="dh0 and dc0"):
        f(gates, cseq, 3, [4, 4, 3], H, w, **out(), dh_n=st(), dh0=st())
    with pytest.raises(VclipError, match="lengths"):
        f(gates, cseq, 3, [4, -1, 3], H, w, **out(), dh_n=st())
    with pytest.raises(VclipError, match="one row per sequence"):
        f(gates, cseq, 2, [4, 4, 3], H, w, **out(), dh_n=st(2))
    with pytest.raises(VclipError, match="past"):
        f(gates, cseq, 3, [4, 4, 5], H, w, **out(), dh_n=st())
    with pytest.raises(VclipError, match="past"):
        f(gates, cseq, 3, [4, 4, 3], H, w, **out(10), dh_n=st())
    with pytest.raises(VclipError, match="past"):
        f(gates, cseq, 3, [4, 4, 3], H, w, **out(), dh_seq=_z(10, H))
    with pytest.raises(VclipError, match="gates f32"):
        f(gates, cseq, 3, None, H, w, **out(15), dh_n=st(), T=5)  # dense: 15 rows wanted of the saved tensors
    with pytest.raises(VclipError, match="dpre f32"):
        f(_z(15, 4 * H), _z(15, H), 3, None, H, w, **out(), dh_n=st(), T=5)  # and of the outputs
    with pytest.raises(VclipError, match="w_hh"):
        f(gates, cseq, 3, [4, 4, 3], H, _z(H, 4 * H), **out(), dh_n=st())
    with pytest.raises(VclipError, match=r"\[B, H\]"):
        f(gates, cseq, 3, [4, 4, 3], H, w, **out(), dh_n=st(2))
    with pytest.raises(VclipError, match=r"\[B, H\]"):
        f(gates, cseq, 3, [4, 4, 3], H, w, **out(), dc_n=_z(3, H, dt=torch.float64))
    with pytest.raises(VclipError, match="alias"):
        s = st()
        f(gates, cseq, 3, [4, 4, 3], H, w, **out(), dh_n=s, dh0=st(), dc0=s)  # dc0 over dh_n
    with pytest.raises(VclipError, match="hidden"):
        f(_z(12, 120), _z(12, 30), 3, [4, 4, 3], 30, _z(120, 30), _z(12, 120), _z(12, 120, dt=torch.bfloat16))
    z = torch.zeros
    with pytest.raises(VclipError, match="no CPU path"):  # plain CPU tensors
        f(z(12, 4 * H), z(12, H), 3, [4, 4, 3], H, z(4 * H, H), z(12, 4 * H), z(12, 4 * H, dtype=torch.bfloat16))


def test_parser_has_tbptt_chunk():
    train = apps.build_parser(apps.FAMILIES["lstm"], inference=False)
    acts = {a.option_strings[0]: a for a in train._actions if a.option_strings}
    a = acts["--tbptt_chunk"]
    assert a.type is int and a.default == 0 and not a.required
    assert train.parse_args([]).tbptt_chunk == 0
    assert train.parse_args(["--tbptt_chunk", "16"]).tbptt_chunk == 16
    assert "--stream_chunk" not in acts
    inference = apps.build_parser(apps.FAMILIES["lstm"], inference=True)
    assert "--tbptt_chunk" not in {s for a in inference._actions for s in a.option_strings}


def test_negative_tbptt_chunk_is_an_error(tmp_path):
    with pytest.raises(ValueError, match="tbptt_chunk"):
        apps.run_main("lstm", ["--data_dir", str(tmp_path), "--log_dir", str(tmp_path / "logs"), "--model_dir",
                               str(tmp_path / "models"), "--tbptt_chunk", "-1"])


def test_forward_train_stream_refusals_on_the_host():
    from vclip_amd.resnet50_lstm import LstmState, VideoResNet50LSTM
    m = VideoResNet50LSTM(32, 2, 0.5).train()
    video = torch.zeros(1, 3, 4, 8, 8)
    with pytest.raises(RuntimeError, match="GPU only"):  # a CPU tensor
        m.forward_train_stream(video, [2, 2])
    with pytest.raises(ValueError, match="lengths"):
        m.forward_train_stream(video, [2, 3])
    with pytest.raises(ValueError, match="lengths"):
        m.forward_train_stream(video, [5, -1])
    with pytest.raises(ValueError, match="lengths"):
        m.forward_train_stream(video, [])
    with pytest.raises(ValueError, match="lengths"):
        m.forward_train_stream(torch.zeros(1, 3, 0, 8, 8), [0, 0])  # N >= 1
    with pytest.raises(ValueError, match="video must be"):
        m.forward_train_stream(torch.zeros(2, 3, 4, 8, 8), [2, 2])
    fake = video.as_subclass(_FakeCuda)  # behind the device check: the state's shape, before anything runs
    for bad in (LstmState(_z(2, 3, 32), _z(2, 3, 32)), LstmState(_z(1, 2, 32), _z(1, 2, 32)),
                LstmState(_z(2, 2, 32), _z(2, 2, 32, dt=torch.float64)), LstmState(_z(2, 2, 64)[:, :, :32], _z(2, 2, 32))):
        with pytest.raises(ValueError, match=r"state\.h / state\.c"):
            m.forward_train_stream(fake, [2, 2], bad)
    m.eval()
    with pytest.raises(RuntimeError, match="forward_stream"):  # the eval-mode path is named
        m.forward_train_stream(video, [2, 2])


def test_lstm_state_detach_is_a_detached_copy():
    from vclip_amd.resnet50_lstm import LstmState
    h, c = torch.randn(2, 3, 8, requires_grad=True), torch.randn(2, 3, 8, requires_grad=True)
    st = LstmState(h * 2, c * 2)
    d = st.detach()
    assert isinstance(d, LstmState) and not d.h.requires_grad and not d.c.requires_grad
    assert torch.equal(d.h, st.h) and torch.equal(d.c, st.c)
    assert d.h.data_ptr() != st.h.data_ptr() and d.c.data_ptr() != st.c.data_ptr()
    assert st.h.requires_grad  # the original stays in the graph


def test_round_weights_count_the_video_round_pairs():
    """Frame counts (9, 2, 5) at chunk 4: video 0 is live in rounds 0, 1, 2, video 1 (shorter than one chunk) in
    round 0, video 2 in rounds 0, 1: 3 + 1 + 2 = 6 pairs; 3, 2, 1 videos are live in the three rounds."""
    assert apps.lstm_tbptt_pairs([9, 2, 5], 4) == 6
    assert apps.lstm_tbptt_pairs([8, 8], 4) == 4 and apps.lstm_tbptt_pairs([3], 4) == 1 and apps.lstm_tbptt_pairs([5, 0], 4) == 2
    w = apps.lstm_tbptt_round_weights([9, 2, 5], 4)
    assert w == pytest.approx([3 / 6, 2 / 6, 1 / 6]) and sum(w) == pytest.approx(1.0)
    # the batch loss is the mean over the pairs: per-round means times the weights = the sum over pairs / 6
    per_pair = {(0, 0): 1.0, (1, 0): 2.0, (2, 0): 6.0, (0, 1): 4.0, (2, 1): 8.0, (0, 2): 3.0}
    rounds = [[1.0, 2.0, 6.0], [4.0, 8.0], [3.0]]
    total = sum(wk * sum(r) / len(r) for wk, r in zip(w, rounds))
    assert total == pytest.approx(sum(per_pair.values()) / 6)
    assert apps.lstm_tbptt_round_weights([8, 8], 4) == pytest.approx([0.5, 0.5])  # exact multiples: no empty round
    assert apps.lstm_tbptt_round_weights([3], 4) == pytest.approx([1.0])
    assert apps.lstm_tbptt_round_weights([5, 0], 4) == pytest.approx([0.5, 0.5])  # an empty video holds no pair
    assert apps.lstm_tbptt_round_weights([1, 1, 1], 1) == pytest.approx([1.0])
    with pytest.raises(ValueError, match="no frames"):
        apps.lstm_tbptt_round_weights([0, 0], 4)
    with pytest.raises(ValueError, match="no frames"):
        apps.lstm_tbptt_pairs([0, 0], 4)
    with pytest.raises(ValueError, match="no frames"):
        apps.lstm_tbptt_round_weights([], 4)
    with pytest.raises(ValueError, match="chunk"):
        apps.lstm_tbptt_round_weights([4], 0)


def test_whole_video_batches_are_an_epoch_seeded_permutation():
    class DS:
        video_paths = [f"v{i}" for i in range(7)]
        labels = [0, 0, 0, 0, 1, 1, 1]

    a, b = apps.LstmWholeVideoBatches(DS, 3, shuffle=True), apps.LstmWholeVideoBatches(DS, 3, shuffle=True)
    e0, e1 = list(a), list(a)
    assert len(a) == 2 and len(e0) == 2 and all(len(p) == 3 and len(l) == 3 for p, l in e0)  # the short batch dropped
    assert e0 == list(b) and e1 == list(b)  # seeded: a second loader replays the epochs
    assert e0 != e1  # a new permutation per epoch
    for paths, labels in e0 + e1:
        assert [DS.labels[DS.video_paths.index(p)] for p in paths] == labels
    assert len({p for paths, _ in e0 for p in paths}) == 6
    val = apps.LstmWholeVideoBatches(DS, 3, shuffle=False)
    assert list(val) == list(val) == [(["v0", "v1", "v2"], [0, 0, 0]), (["v3", "v4", "v5"], [0, 1, 1])]
