"""The stateful LSTM recurrence's host side without a GPU: the declaration and ctypes signature of
vc_lstm_seq_fwd_state next to the two unchanged forward entry points, its argument validation before any
HIP call, the refusals of ops.lstm_seq_fwd_state, the --stream_chunk flag and forward_stream's refusals."""
import ctypes

import pytest
import torch

import vclip_amd._lib as L
from vclip_amd import apps, ops
from vclip_amd._lib import VclipError


def test_state_entry_point_declared_and_bound():
    assert "vc_lstm_seq_fwd_state" in L.header_functions()
    argtypes, restype = L.SIGNATURES["vc_lstm_seq_fwd_state"]
    assert len(argtypes) == 17 and restype is ctypes.c_int
    assert len(L.SIGNATURES["vc_lstm_seq_fwd"][0]) == 15  # the existing entry points keep their signatures
    assert len(L.SIGNATURES["vc_lstm_seq_fwd_ragged"][0]) == 12


def test_state_entry_point_validates_before_any_hip_call():
    from vclip_amd.build import LIB_PATH, build
    build()
    assert hasattr(ctypes.CDLL(LIB_PATH), "vc_lstm_seq_fwd_state")
    lib = L.load()
    p = ctypes.c_void_p(64)
    good = dict(pre=p, ldpre=1024, B=3, row0=p, len=p, max_len=8, hidden=256, w=p, h0=p, c0=p, hseq=p, ldh=256, hall=p,
                ldha=256, hn=p, cn=p)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vc_lstm_seq_fwd_state(a["pre"], a["ldpre"], a["B"], a["row0"], a["len"], a["max_len"], a["hidden"], a["w"],
                                       a["h0"], a["c0"], a["hseq"], a["ldh"], a["hall"], a["ldha"], a["hn"], a["cn"], None)
        return rc, lib.vc_last_error().decode()

    for name in ("pre", "w", "hseq", "hn", "cn"):
        rc, msg = call(**{name: None})
        assert rc != 0 and "null" in msg, name
    for name, word in (("row0", "row0 and len"), ("len", "row0 and len"), ("h0", "h0 and c0"), ("c0", "h0 and c0")):
        rc, msg = call(**{name: None})  # exactly one of a pair
        assert rc != 0 and word in msg, (name, msg)
    for kw, word in ((dict(B=0), ">= 1"), (dict(max_len=0), ">= 1"), (dict(hidden=30), "hidden"), (dict(hidden=1028), "hidden"),
                     (dict(ldpre=1023), "stride"), (dict(ldh=255), "stride"), (dict(ldha=255), "stride")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg and "vc_lstm_seq_fwd_state" in msg, (kw, msg)


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on the GPU: reaches the host checks behind the device check.  Every
    refusal below is raised before any pointer is handed to the library."""

    @property
    def device(self):
        return torch.device("cuda", 0)


def _z(*s, dt=torch.float32):
    return torch.zeros(*s, dtype=dt).as_subclass(_FakeCuda)


def test_ops_state_refusals():
    H = 32
    pre, w, hseq = _z(12, 4 * H), _z(H, 4 * H), _z(12, H, dt=torch.bfloat16)
    st = lambda B=3: _z(B, H)  # noqa: E731
    with pytest.raises(VclipError, match="h0 and c0"):
        ops.lstm_seq_fwd_state(pre, [4, 4, 3], H, w, hseq, st(), st(), h0=st())
    with pytest.raises(VclipError, match="h0 and c0"):
        ops.lstm_seq_fwd_state(pre, [4, 4, 3], H, w, hseq, st(), st(), c0=st())
    with pytest.raises(VclipError, match="lengths"):
        ops.lstm_seq_fwd_state(pre, [4, -1, 3], H, w, hseq, st(), st())
    with pytest.raises(VclipError, match="overlap"):
        ops.lstm_seq_fwd_state(pre, [4, 4, 3], H, w, hseq, st(), st(), row0=[0, 3, 8])
    with pytest.raises(VclipError, match="past"):
        ops.lstm_seq_fwd_state(pre, [4, 4, 5], H, w, hseq, st(), st())  # 13 rows wanted, 12 there
    with pytest.raises(VclipError, match="past"):
        ops.lstm_seq_fwd_state(pre, [4, 0, 3], H, w, hseq, st(), st(), row0=[0, 4, 10])
    with pytest.raises(VclipError, match="past"):
        ops.lstm_seq_fwd_state(pre, [4, 4, 3], H, w, hseq, st(), st(), h_all=_z(10, H))  # h_all shorter than the rows
    with pytest.raises(VclipError, match="pre f32"):
        ops.lstm_seq_fwd_state(pre, None, H, w, hseq, st(), st(), T=5)  # dense: 15 rows wanted
    with pytest.raises(VclipError, match="hidden"):
        ops.lstm_seq_fwd_state(_z(12, 120), [4, 4, 3], 30, _z(30, 120), _z(12, 30, dt=torch.bfloat16), _z(3, 30), _z(3, 30))
    with pytest.raises(VclipError, match="hidden"):
        ops.lstm_seq_fwd_state(_z(12, 4 * 1028), [4], 1028, _z(1028, 4 * 1028), _z(12, 1028, dt=torch.bfloat16), _z(1, 1028),
                               _z(1, 1028))
    with pytest.raises(VclipError, match="one row per sequence"):
        ops.lstm_seq_fwd_state(pre, [4, 4, 3], H, w, hseq, st(2), st(2))
    with pytest.raises(VclipError, match=r"\[B, H\]"):
        ops.lstm_seq_fwd_state(pre, [4, 4, 3], H, w, hseq, st(), st(), h0=_z(3, H, dt=torch.float64), c0=st())
    with pytest.raises(VclipError, match="alias"):
        s = st()
        ops.lstm_seq_fwd_state(pre, [4, 4, 3], H, w, hseq, s, s)  # h_n and c_n in one buffer
    with pytest.raises(VclipError, match="dense layout"):
        ops.lstm_seq_fwd_state(pre, None, H, w, hseq, st(), st())  # neither lengths nor T
    z = torch.zeros
    with pytest.raises(VclipError, match="no CPU path"):  # plain CPU tensors
        ops.lstm_seq_fwd_state(z(12, 4 * H), [4, 4, 3], H, z(H, 4 * H), z(12, H, dtype=torch.bfloat16), z(3, H), z(3, H))
    # lstm_seq_fwd_ragged keeps refusing an empty sequence
    with pytest.raises(VclipError, match="lengths"):
        ops.lstm_seq_fwd_ragged(pre, [4, 0, 3], H, w, hseq, st())


def test_parser_has_stream_chunk():
    parser = apps.build_parser(apps.FAMILIES["lstm"], inference=True)
    acts = {a.option_strings[0]: a for a in parser._actions if a.option_strings}
    a = acts["--stream_chunk"]
    assert a.type is int and a.default == 0 and not a.required
    assert parser.parse_args(["--videos_dir", "v", "--model_path", "m"]).stream_chunk == 0
    assert parser.parse_args(["--videos_dir", "v", "--model_path", "m", "--stream_chunk", "32"]).stream_chunk == 32
    train = apps.build_parser(apps.FAMILIES["lstm"], inference=False)
    assert "--stream_chunk" not in {s for a in train._actions for s in a.option_strings}


def test_negative_stream_chunk_is_an_error(tmp_path):
    with pytest.raises(ValueError, match="stream_chunk"):
        apps.run_inference("lstm", ["--videos_dir", str(tmp_path), "--model_path", str(tmp_path / "none.pth"),
                                    "--output_dir", str(tmp_path / "out"), "--stream_chunk", "-1"])


def test_forward_stream_refusals_on_the_host():
    from vclip_amd.resnet50_lstm import LstmState, VideoResNet50LSTM
    m = VideoResNet50LSTM(32, 2, 0.5).eval()
    st = m.init_state(3)
    assert isinstance(st, LstmState) and tuple(st.h.shape) == tuple(st.c.shape) == (2, 3, 32)
    assert st.h.dtype == st.c.dtype == torch.float32 and not st.h.any() and not st.c.any()
    assert st.h.device == next(m.parameters()).device and st.h.data_ptr() != st.c.data_ptr()
    video = torch.zeros(1, 3, 4, 8, 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.forward_stream(video, [2, 2])
    with pytest.raises(ValueError, match="lengths"):
        m.forward_stream(video, [2, 3])
    with pytest.raises(ValueError, match="lengths"):
        m.forward_stream(video, [5, -1])
    with pytest.raises(ValueError, match="lengths"):
        m.forward_stream(video, [])
    with pytest.raises(ValueError, match="lengths"):
        m.forward_stream(torch.zeros(1, 3, 0, 8, 8), [0, 0])  # N >= 1
    with pytest.raises(ValueError, match="video must be"):
        m.forward_stream(torch.zeros(2, 3, 4, 8, 8), [2, 2])
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.forward_stream(video, [2, 2])
