"""ResNet50-LSTM video classifier on the libvclip.so kernels — drop-in for
`VideoResNet50LSTM(hidden_size=256, num_layers=2, dropout=0.5)` of
resnet50-2d-lstm/src/models/model.py:5-60, called as `model(f32[B, 3, T, H, W])` -> `f32[B, 1]`,
in eval mode and in the reference's train loop (resnet50-2d-lstm/src/trainer/trainer.py:156-170).

Per frame, torchvision's ResNet-50 (v1.5, fc removed) runs on the shared conv path
(resnet3d.ResNet3d with kt = 1 kernels, channels-last bf16); vc_frame_avgpool gives the
[B*T, 2048] bf16 features.  Each LSTM layer is one MFMA GEMM for the input projections of all T
steps (bias = b_ih + b_hh, fp32 out) followed by the fp32 recurrence kernel (vc_lstm_seq_fwd);
the last step's h goes through the hidden -> 64 -> 1 head (vc_mlp_head_fwd).

Training: the backbone is frozen (model.py:15-16: requires_grad = False; trainer.py:45-48 hands
Adam the trainable parameters only), but `model.train()` still puts its BatchNorm layers into
training mode, so the reference normalises with batch statistics and updates the running
statistics.  That is what train mode does here too: a no-grad forward of the backbone with fp32
batch statistics and fp16 activation rows (`_train_features_h16`; ResNet3d's own train-mode forward,
which keeps bf16 rows for its backward, would cost ~4x the feature error).
`freeze_backbone_bn = True` is a deliberate deviation: the folded-BatchNorm inference path in train mode, running statistics untouched (the usual way to fine-tune on a
frozen backbone).  The LSTM and the head run as autograd ops over HIP kernels
(autograd_ops.lstm_layer / mlp_head); dropout masks come from torch's RNG.

Inference beyond the reference: `forward_ragged` batches videos of different lengths, and
`init_state` / `forward_stream` carry nn.LSTM's (h, c) from call to call (vc_lstm_seq_fwd_state), so a
recording of any length runs in chunks at bounded memory, with a logit after every frame.

Saliency: `explain` is per-frame Grad-CAM / HiResCAM on the 2D backbone with the gradient taken through the head and
the recurrence by exact BPTT (no weight gradients; csrc/frame_cam.hip), `explain_stream_begin` the per-frame relevance of
whole recordings in chunks.

Training beyond the reference: `forward_train_stream` is the train step on such chunks, over whole videos
of different lengths with the state carried (autograd_ops.lstm_layer_state on vc_lstm_seq_fwd_train_state /
vc_lstm_seq_bwd_state): the state it returns stays in the autograd graph (full BPTT across the chunks)
until the caller takes `LstmState.detach()` (truncated BPTT).

State dict keys are the reference's (resnet50.<child>..., lstm.*, classifier.*).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import NamedTuple

import numpy as np
import torch

from . import autograd_ops as A
from . import explaining, ops
from .explaining import Explanation
from .hosting import ParamStore, round_up as _ru
from .resnet3d import ResNet3d
from .weights import RESNET50_2D, blocks_to_torchvision_resnet50, resnet50_lstm_param_shapes, \
    torchvision_resnet50_to_blocks

HEAD_DIM = 64  # classifier.0: Linear(hidden, 64)


class LstmState(NamedTuple):
    """nn.LSTM's (h_n, c_n): f32 [num_layers, B, hidden] each (init_state, forward_stream, forward_train_stream)."""
    h: torch.Tensor
    c: torch.Tensor

    def detach(self) -> "LstmState":
        """A copy cut off from the autograd graph: what truncated BPTT carries from chunk to chunk."""
        return LstmState(self.h.detach().clone(), self.c.detach().clone())


class VideoResNet50LSTM(ParamStore):
    def __init__(self, hidden_size: int = 256, num_layers: int = 2, dropout: float = 0.5,
                 freeze_backbone_bn: bool = False):
        super().__init__()
        if hidden_size <= 0 or hidden_size % 4 or hidden_size > 1024:
            raise ValueError(f"hidden_size {hidden_size} unsupported: hidden_size % 4 == 0 and hidden_size <= 1024")
        if num_layers < 1:
            raise ValueError("num_layers must be >= 1")
        if not 0.0 <= dropout < 1.0:
            raise ValueError("dropout must be in [0, 1)")
        self.hidden, self.layers, self.dropout = hidden_size, num_layers, float(dropout)
        # False (the reference): model.train() runs the frozen backbone's BatchNorm with batch statistics and
        # updates its running statistics; True: the folded inference path, running statistics untouched
        self.freeze_backbone_bn = freeze_backbone_bn
        self.backbone = ResNet3d(RESNET50_2D)
        for p in self.backbone.parameters():
            p.requires_grad_(False)  # model.py:15-16
        shapes = resnet50_lstm_param_shapes(hidden_size, num_layers)
        self._all_names = list(shapes.keys())
        self._init_params({n: s for n, s in shapes.items() if not n.startswith("resnet50.")})
        self._ws = {}
        self._explain_ws = {}  # explain's workspace, one key at a time (_explain_workspace)
        # the last forward's bf16 feature matrix [B*T, 2048] and dropout masks ({"lstm": [per layer or None],
        # "head": mask or None}), for tests that replay them through an oracle
        self.last_features = None
        self.last_keep = None

    # ---- state dict in the reference's naming -----------------------------------------
    def state_dict(self, *a, **k):
        bb = self.backbone.state_dict()
        out = OrderedDict()
        for n in self._all_names:
            if n.startswith("resnet50."):
                v = bb[torchvision_resnet50_to_blocks(n)]
                out[n] = v.squeeze(2) if v.dim() == 5 else v
            else:
                out[n] = self.P(n).detach()
        return out

    def load_state_dict(self, sd, strict: bool = True):
        sd = {k[len("module."):] if k.startswith("module.") else k: v for k, v in sd.items()}
        bb, rest = {}, {}
        for k, v in sd.items():
            if k.endswith("num_batches_tracked"):
                continue
            b = torchvision_resnet50_to_blocks(k)
            if b is not None:
                v = torch.as_tensor(np.asarray(v)) if not isinstance(v, torch.Tensor) else v
                bb[b] = v.unsqueeze(2) if v.dim() == 4 else v
            else:
                rest[k] = v
        missing = [n for n in self._names if n not in rest]
        unexpected = [k for k in rest if k not in self._names]
        if strict and (missing or unexpected):
            raise KeyError(f"load_state_dict: missing={missing[:5]} unexpected={unexpected[:5]}")
        m1, u1 = self.backbone.load_state_dict(bb, strict=strict)
        m1 = [blocks_to_torchvision_resnet50(n) for n in m1]
        with torch.no_grad():
            for n in self._names:
                if n in rest:
                    v = rest[n]
                    v = torch.as_tensor(np.asarray(v)) if not isinstance(v, torch.Tensor) else v
                    self.P(n).copy_(v.reshape(self.P(n).shape))
        self._packed = None
        return m1 + missing, u1 + unexpected

    # ---- operand images of the LSTM / head weights, once per weights version -----------
    def _pack(self, device):
        pk = self._cached_pack(device)
        if pk is not None:
            return pk
        pk = {"device": device, "version": self._weights_version(), "layers": []}
        for l in range(self.layers):
            L = A.pack_lstm_weights(self.P(f"lstm.weight_ih_l{l}"), self.P(f"lstm.weight_hh_l{l}"))
            b = torch.zeros(L["wb"].shape[0], dtype=torch.float32, device=device)
            b[: 4 * self.hidden] = self.P(f"lstm.bias_ih_l{l}").detach() + self.P(f"lstm.bias_hh_l{l}").detach()
            L["b"] = b
            pk["layers"].append(L)
        pk["head"] = [self.P(n).detach().float().contiguous() for n in
                      ("classifier.0.weight", "classifier.0.bias", "classifier.3.weight", "classifier.3.bias")]
        self._packed = pk
        return pk

    def _workspace(self, rows, B, device):
        """The inference buffers for `rows` frame rows in all and B sequences; one (rows, B) at a time."""
        key = (rows, B, str(device))
        if key not in self._ws:
            M = _ru(rows, 256)
            z = lambda r, c, dt: torch.zeros(r, c, dtype=dt, device=device)  # noqa: E731
            self._ws = {key: dict(pre=z(M, _ru(4 * self.hidden, 128), torch.float32),
                                  hseq=[z(M, _ru(self.hidden, 128), torch.bfloat16) for _ in range(2)],
                                  hlast=z(B, self.hidden, torch.float32), logits=z(B, 1, torch.float32))}
        return self._ws[key]

    # ---- forward -----------------------------------------------------------------------
    def forward(self, video: torch.Tensor) -> torch.Tensor:
        """`model(video)` -> logits f32 [B, 1].  In training mode the train step runs (batch-statistic
        BatchNorm in the frozen backbone unless `freeze_backbone_bn`, dropout, autograd ops), with
        autograd enabled or not; in eval mode the fused inference path."""
        if not isinstance(video, torch.Tensor) or video.device.type != "cuda":
            raise RuntimeError("VideoResNet50LSTM (vclip_amd) runs on the GPU only: move the clip batch to cuda")
        if video.dim() != 5 or video.shape[1] != 3:
            raise ValueError("video must be [B, 3, T, H, W]")
        x = video.contiguous().float() if video.dtype != torch.float32 else video.contiguous()
        if self.training:
            return self._forward_train(x)
        with torch.no_grad():
            return self.forward_logits(x).clone()  # the workspace buffer is reused by the next call

    def features(self, video: torch.Tensor, train_bn: bool = False) -> torch.Tensor:
        """Per-frame ResNet-50 features bf16 [ru(B*T, 256), 2048] (rows >= B*T are zero)."""
        B, _, T = video.shape[:3]
        with torch.no_grad():
            if train_bn:
                x, (t, h, w), Cf = self._train_features_h16(video)
                self.backbone._packed = None  # the running statistics moved: re-fold before the next eval
            else:
                x, _, (t, h, w), Cf, _ = self.backbone.forward_features(video)
            feat = torch.zeros(_ru(B * T, 256), Cf, dtype=torch.bfloat16, device=video.device)
            # per-frame AdaptiveAvgPool2d(1): rows are ((b*T + t)*h + y)*w + x
            ops.frame_avgpool(x, B * T, h * w, Cf, feat)
        self.last_features = feat[: B * T]
        return feat

    # ---- the frozen backbone in train mode: batch-statistic BatchNorm, no gradients, fp16 rows -----
    def _backbone_h16(self, device):
        """fp16 images [ru(Cout, 128), ru(K, 128)] of the conv weights, columns (kt, kh, kw, c) with the
        stem's 3 input channels padded to 8; once per backbone weights version."""
        ver = self.backbone._weights_version()
        pk = getattr(self, "_bb_h16", None)
        if pk is not None and pk["device"] == device and pk["version"] == ver:
            return pk
        pk = {"device": device, "version": ver}
        for n in self.backbone._names:
            if self.backbone.P(n).dim() != 5:  # conv weights only
                continue
            w = self.backbone.P(n).detach().to(device).permute(0, 2, 3, 4, 1)  # [Co, kt, kh, kw, Ci]
            if w.shape[-1] % 8:
                w = torch.nn.functional.pad(w, (0, 8 - w.shape[-1] % 8))
            w = w.reshape(w.shape[0], -1)
            img = torch.zeros(_ru(w.shape[0], 128), _ru(w.shape[1], 128), dtype=torch.float16, device=device)
            img[: w.shape[0], : w.shape[1]] = w
            pk[n] = img
        self._bb_h16 = pk
        return pk

    def _train_features_h16(self, video: torch.Tensor):
        """torchvision's ResNet-50 in training mode without gradients (the reference's frozen backbone under
        model.train()): every conv is an fp16 MFMA GEMM with fp32 accumulation, BatchNorm takes its batch
        statistics in fp32 and updates the running ones (vc_batchnorm_train_fwd), and the activations
        stay fp16 rows (vc_bn_apply_h16).  ResNet3d's own train-mode forward keeps bf16 rows for its
        backward; here nothing is differentiated and bf16 rows would cost ~4x the feature error, because
        the batch-statistic normalisation amplifies storage rounding.
        fp16 tops out at 65504 where bf16 does not: every stored row here is a BatchNorm output (|z| of
        order gamma * a few + beta) or the normalised input clip, and the GEMMs accumulate and leave in
        fp32, so only a checkpoint with BatchNorm gains of order 1e4 could reach it.  The accumulate
        epilogue is the fp16 GEMM's only fp32-output one, hence the zeroed `y`.
        Returns (last activations fp16 [>= B*T*h*w, 2048], (T, h, w), 2048)."""
        bb = self.backbone
        c, P = bb.cfg, bb.P
        B, _, T, H, W = video.shape
        dev = video.device
        wts = self._backbone_h16(dev)
        stem, grids = bb.geometry(T, H, W)
        f16, bf16 = torch.float16, torch.bfloat16
        eps = c["bn_eps"]

        def conv_bn(x, grid, cin, conv, bn, kernel, stride, pad, relu, res=None):
            w16 = wts[conv + ".weight"]
            cout = P(conv + ".weight").shape[0]
            go = ops.conv_out_size(grid, kernel, stride, pad)
            M = B * go[0] * go[1] * go[2]
            Mp, (Np, Kp) = _ru(M, 256), w16.shape
            if tuple(kernel) == (1, 1, 1) and tuple(stride) == (1, 1, 1) and tuple(x.shape) == (Mp, Kp):
                a = x
            else:  # the 16-bit patch gather is element-type agnostic
                kk = kernel[0] * kernel[1] * kernel[2] * cin  # columns past it meet zero weights: keep them finite
                a = (torch.zeros if kk != Kp else torch.empty)(Mp, Kp, dtype=f16, device=dev)
                ops.conv3d_im2col(x.view(bf16), "cl_bf16", B, grid, cin, kernel, stride, pad, a.view(bf16))
            y = torch.zeros(Mp, Np, dtype=torch.float32, device=dev)
            ops.gemm(a, w16, A._zeros_f32(Np, dev), "bias_resid_f32", y, op="backbone_train")
            g, b = P(bn + ".weight").detach(), P(bn + ".bias").detach()
            stat = torch.empty(2, cout, dtype=torch.float32, device=dev)
            ops.batchnorm_train_stats(y[:M, :cout], g, b, P(bn + ".running_mean").detach(),
                                      P(bn + ".running_var").detach(), stat, eps=eps, momentum=0.1)
            z = (torch.zeros if cout % 128 else torch.empty)(Mp, _ru(cout, 128), dtype=f16, device=dev)
            ops.bn_apply_h16(y[:M, :cout], stat, g, b, z, res=res, relu=relu)
            return z, go, cout

        xcl = torch.empty(B * T * H * W, 8, dtype=f16, device=dev)
        ops.video_to_cl_h16(video, xcl)
        x, g0, cin = conv_bn(xcl, (T, H, W), 8, "blocks.0.conv", "blocks.0.norm", c["stem_kernel"], (1, 2, 2),
                             c["stem_pad"], True)
        # MaxPool on non-negative (post-ReLU) rows: 16-bit floats of one sign order like their bit patterns,
        # in fp16 as in bf16, so the bf16 kernel returns the exact fp16 maxima
        gm = grids[0]
        xm = torch.zeros(_ru(B * gm[0] * gm[1] * gm[2], 256), x.shape[1], dtype=f16, device=dev)
        ops.maxpool3d(x.view(bf16), B, g0, cin, (1, 3, 3), (1, 2, 2), (0, 1, 1), xm.view(bf16))
        x, g_in = xm, gm
        for s, depth in enumerate(c["depths"]):
            ss = c["spatial_strides"][s]
            for i in range(depth):
                p = f"blocks.{s + 1}.res_blocks.{i}."
                stride = (1, ss, ss) if i == 0 else (1, 1, 1)
                sc = x
                if p + "branch1_conv.weight" in bb._names:
                    sc, _, _ = conv_bn(x, g_in, cin, p + "branch1_conv", p + "branch1_norm", (1, 1, 1), stride,
                                       (0, 0, 0), False)
                ya, _, ci = conv_bn(x, g_in, cin, p + "branch2.conv_a", p + "branch2.norm_a", (1, 1, 1), (1, 1, 1),
                                    (0, 0, 0), True)
                yb, g, ci = conv_bn(ya, g_in, ci, p + "branch2.conv_b", p + "branch2.norm_b", (1, 3, 3), stride,
                                    (0, 1, 1), True)
                x, _, cin = conv_bn(yb, g, ci, p + "branch2.conv_c", p + "branch2.norm_c", (1, 1, 1), (1, 1, 1),
                                    (0, 0, 0), True, res=sc)
                g_in = g
        return x, g_in, cin

    def forward_logits(self, video: torch.Tensor) -> torch.Tensor:
        """Inference: logits f32 [B, 1] (a workspace buffer, overwritten by the next call)."""
        return self._infer(video)

    def _infer(self, x: torch.Tensor, lengths=None, carry=None):
        """The inference path on the frames of x: the backbone, per LSTM layer the projection GEMM over all
        rows and the recurrence (dense over x's B sequences of T frames when lengths is None; else x is
        [1, 3, N, H, W] and the recurrence ragged over `lengths`), then the head.  Returns the workspace's
        logits buffer.
        carry = (state or None, new_state, frame_logits) makes the recurrence the stateful one
        (vc_lstm_seq_fwd_state): layer l starts from state.h[l] / state.c[l] (None: zeros) and leaves its
        final state in new_state; the head then runs on the top layer's h_n, and with frame_logits also on
        the top layer's h of every frame: (logits buffer, frame logits f32 [N, 1] or None) is returned."""
        B, _, T = x.shape[:3]
        nseq = B if lengths is None else len(lengths)
        pk = self._pack(x.device)
        ws = self._workspace(B * T, nseq, x.device)
        inp = self.features(x)
        hlast, hall = ws["hlast"], None
        if carry is not None:
            old, new, frame_logits = carry
            hlast = new.h[self.layers - 1]
            if frame_logits:
                if "hall" not in ws:
                    ws["hall"] = torch.zeros(ws["pre"].shape[0], self.hidden, dtype=torch.float32, device=x.device)
                hall = ws["hall"]
        for l, L in enumerate(pk["layers"]):
            hseq = ws["hseq"][l & 1]
            ops.gemm(inp, L["wb"], L["b"], "bias_f32", ws["pre"], op="lstm_ih")
            if carry is not None:
                ops.lstm_seq_fwd_state(ws["pre"], lengths, self.hidden, L["w_hh_t"], hseq, new.h[l], new.c[l],
                                       h0=None if old is None else old.h[l], c0=None if old is None else old.c[l],
                                       h_all=hall if l == self.layers - 1 else None)
            elif lengths is None:
                ops.lstm_seq_fwd(ws["pre"], B, T, self.hidden, L["w_hh_t"], hseq, ws["hlast"])
            else:
                ops.lstm_seq_fwd_ragged(ws["pre"], lengths, self.hidden, L["w_hh_t"], hseq, ws["hlast"])
            inp = hseq
        w1, b1, w2, b2 = pk["head"]
        logits = ops.mlp_head_fwd(hlast, w1, b1, w2, b2, ws["logits"])
        if carry is None:
            return logits
        frames = None
        if hall is not None:  # the same head on the same f32 rows: a sequence's last frame equals its logit
            frames = ops.mlp_head_fwd(hall[: B * T], w1, b1, w2, b2, torch.empty(B * T, 1, dtype=torch.float32, device=x.device))
        return logits, frames

    def init_state(self, B: int) -> LstmState:
        """The zero state of B sequences: h and c f32 [num_layers, B, hidden] on the model's device."""
        if B < 1:
            raise ValueError("init_state: B must be >= 1")
        dev = next(self.parameters()).device
        z = lambda: torch.zeros(self.layers, B, self.hidden, dtype=torch.float32, device=dev)  # noqa: E731
        return LstmState(z(), z())

    def forward_stream(self, video: torch.Tensor, lengths, state: LstmState | None = None, frame_logits: bool = False):
        """Whole-video inference in chunks: `video` f32 [1, 3, N, H, W] holds the NEXT frames of len(lengths)
        recordings back to back as in forward_ragged (N == sum(lengths) >= 1; a length may be 0: that
        recording has ended or pauses this round), `state` what the previous call returned (None: the
        zero state of init_state).  Returns (logits f32 [B, 1], new_state), with frame_logits=True
        (logits, new_state, f32 [N, 1]): the head on the top layer's h after every frame, in input order.
        logits[b] is the head on the top layer's h_n[b], so a recording given length 0 keeps its logit,
        and the last frame's logit of a recording in this call is bit-identical to logits[b].
        The returned state is NEW tensors: the caller's `state` is left untouched and stays usable (a
        chunk can be replayed from it).  One backbone pass over the N frames, per layer one projection
        GEMM and one vc_lstm_seq_fwd_state; memory is bounded by N, not by the recordings' lengths.
        Eval mode only, as forward_ragged."""
        if self.training:
            raise RuntimeError("forward_stream is the inference path: call model.eval() first")
        x, lengths, B = self._stream_args(video, lengths, state)
        with torch.no_grad():
            new = LstmState(torch.empty(self.layers, B, self.hidden, dtype=torch.float32, device=x.device),
                            torch.empty(self.layers, B, self.hidden, dtype=torch.float32, device=x.device))
            logits, frames = self._infer(x, lengths, (state, new, frame_logits))
            logits = logits.clone()  # the workspace buffer is reused by the next call
        return (logits, new, frames) if frame_logits else (logits, new)

    def _stream_args(self, video, lengths, state):
        """The layout forward_stream and forward_train_stream take, checked on the host: (f32 contiguous video,
        lengths as a tuple of ints, B)."""
        if not isinstance(video, torch.Tensor):
            raise TypeError("video must be a tensor")
        lengths = tuple(int(n) for n in lengths)
        if video.dim() != 5 or video.shape[0] != 1 or video.shape[1] != 3:
            raise ValueError("video must be [1, 3, N, H, W]: the next frames of all videos back to back")
        if not lengths or min(lengths) < 0 or video.shape[2] < 1 or sum(lengths) != video.shape[2]:
            raise ValueError(f"lengths {lengths} must be >= 0 and sum to the {video.shape[2]} >= 1 frames of video")
        if video.device.type != "cuda":
            raise RuntimeError("VideoResNet50LSTM (vclip_amd) runs on the GPU only: move the clip batch to cuda")
        B = len(lengths)
        if state is not None:
            for t in (state.h, state.c):
                if not isinstance(t, torch.Tensor) or t.device != video.device or t.dtype != torch.float32 or \
                        tuple(t.shape) != (self.layers, B, self.hidden) or not t.is_contiguous():
                    raise ValueError(f"state.h / state.c must be f32 contiguous [{self.layers}, {B}, {self.hidden}] on "
                                     f"{video.device} (init_state({B}))")
        return (video.contiguous().float() if video.dtype != torch.float32 else video.contiguous()), lengths, B

    def forward_train_stream(self, video: torch.Tensor, lengths, state: LstmState | None = None):
        """The train step on the next frames of len(lengths) whole videos, with the LSTM state carried: the
        layout, `lengths` and `state` are forward_stream's (`video` f32 [1, 3, N, H, W], N == sum(lengths) >= 1,
        a length may be 0).  Returns (logits f32 [B, 1], new_state): the head on the top layer's h_n, and an
        LstmState whose h and c are ATTACHED to the autograd graph.  Feed it to the next call as it is and
        one backward() from the last logits is exact BPTT over the whole videos (every chunk's saved tensors
        stay alive until then); feed `new_state.detach()` and the gradient stops at the chunk boundary
        (truncated BPTT, memory bounded by the chunk).
        Every call draws fresh dropout masks from torch's RNG, the inter-layer one over the N rows and the
        head's [B, 64], recorded in `last_keep`.  Each layer is autograd_ops.lstm_layer_state (one projection
        GEMM, vc_lstm_seq_fwd_train_state, backward vc_lstm_seq_bwd_state).
        The backbone's BatchNorm follows `freeze_backbone_bn` as in `forward`; with batch statistics (False) the
        N frames of a call share their statistics across the videos and the running statistics move once per
        call, so chunked training wants `freeze_backbone_bn = True`.
        Training mode only; forward_stream is the eval-mode path."""
        if not self.training:
            raise RuntimeError("forward_train_stream is the train step: call model.train() first "
                               "(forward_stream is the eval-mode path)")
        x, lengths, B = self._stream_args(video, lengths, state)
        N = x.shape[2]
        dev = x.device
        x = self.features(x, train_bn=not self.freeze_backbone_bn)[:N]
        pk = self._pack(dev)
        p = self.dropout
        keeps, hs, cs = [], [], []
        for l in range(self.layers):
            keep = None
            if p > 0.0 and l < self.layers - 1:  # nn.LSTM: dropout on the outputs of every layer but the last
                keep = torch.ones(N, self.hidden, device=dev).bernoulli_(1.0 - p).mul_(1.0 / (1.0 - p))
            keeps.append(keep)
            x, h_n, c_n = A.lstm_layer_state(x, self.P(f"lstm.weight_ih_l{l}"), self.P(f"lstm.weight_hh_l{l}"),
                                             self.P(f"lstm.bias_ih_l{l}"), self.P(f"lstm.bias_hh_l{l}"), list(lengths),
                                             h0=None if state is None else state.h[l],
                                             c0=None if state is None else state.c[l], keep=keep, need_dx=l > 0,
                                             packed=pk["layers"][l])
            hs.append(h_n)
            cs.append(c_n)
        hkeep = None
        if p > 0.0:
            hkeep = torch.ones(B, HEAD_DIM, device=dev).bernoulli_(1.0 - p).mul_(1.0 / (1.0 - p))
        self.last_keep = {"lstm": keeps, "head": hkeep}
        logits = A.mlp_head(hs[-1], self.P("classifier.0.weight"), self.P("classifier.0.bias"),
                            self.P("classifier.3.weight"), self.P("classifier.3.bias"), hkeep)
        return logits, LstmState(torch.stack(hs), torch.stack(cs))

    def forward_ragged(self, video: torch.Tensor, lengths) -> torch.Tensor:
        """Batched inference over videos of different lengths: `video` f32 [1, 3, N, H, W] holds the frames of
        len(lengths) videos back to back (N == sum(lengths), every length >= 1) -> logits f32
        [len(lengths), 1], row b for the frames of video b.  The frames are independent through the
        backbone (every kernel is kt = 1), so it runs once over the N frames; each LSTM layer is one
        input-projection GEMM over the N rows and one ragged recurrence (vc_lstm_seq_fwd_ragged).  Eval mode
        only: the train step's batch-statistic BatchNorm would mix the videos."""
        if self.training:
            raise RuntimeError("forward_ragged is the inference path: call model.eval() first")
        if not isinstance(video, torch.Tensor) or video.device.type != "cuda":
            raise RuntimeError("VideoResNet50LSTM (vclip_amd) runs on the GPU only: move the clip batch to cuda")
        lengths = tuple(int(n) for n in lengths)
        if video.dim() != 5 or video.shape[0] != 1 or video.shape[1] != 3:
            raise ValueError("video must be [1, 3, N, H, W]: the frames of all videos back to back")
        if not lengths or min(lengths) < 1 or sum(lengths) != video.shape[2]:
            raise ValueError(f"lengths {lengths} must be >= 1 and sum to the {video.shape[2]} frames of video")
        x = video.contiguous().float() if video.dtype != torch.float32 else video.contiguous()
        with torch.no_grad():
            return self._infer(x, lengths).clone()

    # ---- explain: per-frame Grad-CAM / HiResCAM through the recurrence ------------------
    EXPLAIN_METHODS = ResNet3d.EXPLAIN_METHODS
    EXPLAIN_LAYERS = ResNet3d.EXPLAIN_LAYERS  # res2 / res3: out of scope
    LSTM_DX_CFG = 5  # the 128 x 128 GEMM tile for every lstm_dx of explain: a frame's gradient row must not depend on
    #                  how many rows share the launch (a streamed chunk against the whole recording)

    def _explain_workspace(self, rows, nseq, Pl, Cl, device):
        """explain's own buffers for `rows` frame rows in nseq sequences and a map of Pl positions x Cl channels per
        frame; one key at a time, like _workspace (which it never touches)."""
        def build():
            H, M = self.hidden, _ru(rows, 256)
            Np, Hp = _ru(4 * H, 128), _ru(H, 128)
            f32, bf = torch.float32, torch.bfloat16
            z = lambda r, c, dt=f32: torch.zeros(r, c, dtype=dt, device=device)  # noqa: E731
            return dict(feat=z(M, 2048, bf), pre=z(M, Np), h_prev=z(M, Hp, bf), dpre=z(rows, 4 * H), dpb=z(M, Np, bf),
                        hseq=[z(M, Hp, bf) for _ in range(2)], gates=[z(rows, 4 * H) for _ in range(self.layers)],
                        c_seq=[z(rows, H) for _ in range(self.layers)], h_n=z(self.layers * nseq, H).view(self.layers, nseq, H), c_n=z(self.layers * nseq, H).view(self.layers, nseq, H),
                        dxh=z(M, Hp), g=z(M, 2048), frame_rel=z(1, rows)[0], frame_map=z(1, rows)[0], map=z(1, rows * Pl)[0],
                        map_rel=z(1, rows)[0], alpha=z(rows, Cl), cam_work=ops.cam_weights_work(rows, Cl, device),
                        head=self._head_buffers(nseq, device))

        return explaining.cached_explain(self._explain_ws, (rows, nseq, Pl, Cl, str(device)), build, limit=1)

    def _head_buffers(self, B, device):
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)  # noqa: E731
        return dict(hid=z(B, HEAD_DIM), logits=z(B, 1), dlogits=z(B, 1), dh=z(B, self.hidden),
                    dw1=z(HEAD_DIM, self.hidden), db1=z(HEAD_DIM), dw2=z(1, HEAD_DIM), db2=z(1))

    def _head_gradient(self, pk, hb, h_top, target):
        """The head on h_top f32 [B, H] with its hidden row kept, the targets (None: each sequence's predicted class, 1
        when the logit is >= 0) and dh = d logit / d h_top in hb["dh"]: (logits clone, targets).  The head's weight
        gradients land in scratch and are never read.
        The gradient is always +z's.  Every launch after it is linear in the seed's sign, so target 0 (-z) is the finished
        map times -1 on the host: the exact negation, which a seed of -1 would miss by last bits (the MFMA's
        accumulation is not symmetric under a flip of every sign)."""
        w1, b1, w2, b2 = pk["head"]
        logits = ops.mlp_head_fwd(h_top, w1, b1, w2, b2, hb["logits"], hid=hb["hid"]).clone()
        if target is None:
            target = [int(v >= 0) for v in logits[:, 0].tolist()]
        hb["dlogits"].fill_(1.0)
        ops.mlp_head_bwd(h_top, w1, w2, hb["hid"], None, hb["dlogits"], hb["dh"], hb["dw1"], hb["db1"], hb["dw2"], hb["db2"])
        return logits, target

    def _lstm_dx(self, dpb, wt, out):
        from .autograd_ops import _zeros_f32
        return ops.gemm(dpb, wt, _zeros_f32(wt.shape[0], dpb.device), "bias_f32", out, cfg=self.LSTM_DX_CFG, op="lstm_dx")

    @staticmethod
    def _explain_targets(target, B):
        return explaining.expand_targets(*explaining.check_targets(target, 2), B, what="videos")

    @staticmethod
    def _positive_share(rel: torch.Tensor) -> torch.Tensor:
        """relu(rel) / its sum over one video's entries (all zero when nothing is positive), f32 like rel"""
        pos = rel.double().clamp_min(0)
        tot = pos.sum()
        return (pos / tot if float(tot) > 0 else torch.zeros_like(pos)).float()

    @torch.no_grad()
    def explain(self, video: torch.Tensor, method: str = "gradcam", target=None, layer: str = "res5", lengths=None):
        """The logit and which frames, and where in them, produced it: Grad-CAM (Selvaraju et al. 2017) or HiResCAM
        (Draelos & Carin 2020) on the output of `layer` of the 2D backbone ("res5": H/32 x W/32 per frame, "res4":
        H/16 x W/16), with the gradient taken through the head and the recurrence by exact BPTT.  The model has one
        logit z: `target` 1 explains +z, 0 explains -z, None the predicted class (1 when z >= 0, the CLI's p >= 0.5);
        an int, or a sequence / tensor of one int per video.

        Dense: video [B, 3, T, H, W].  Ragged (`lengths` given): forward_ragged's layout, [1, 3, N, H, W] with the
        frames of len(lengths) videos back to back, every length >= 1.

        g_t = dz / d f_t (f_t the pooled features of frame t) comes from the head (vc_mlp_head_bwd with dlogits = 1; the
        sign of target 0 is applied to the finished maps on the host, the exact negation), the top layer from dh_n, every lower layer through dx = dpre . W_ih (vc_lstm_seq_bwd_state + the lstm_dx GEMM,
        fp32 out); no weight gradient is formed in the recurrence or the backbone.  Then, with A_t the layer's
        activations in frame t and P its positions per frame:

            "res5"  d z / d A_t[p, c] = g_t[c] / P at every position, so Grad-CAM and HiResCAM coincide:
                    map[t, p] = (1/P) sum_c g_t[c] A_t[p, c] from the fp32 g_t (vc_frame_cam).  Both methods run the
                    same launches there: their maps are bit-identical.
            "res4"  the res5 rows are seeded with bf16(g_t[c] / P) (vc_frame_avgpool_bwd) and ResNet3d._explain_chain walks
                    back to res4: "hirescam" sum_c G[t, p, c] A[t, p, c]; "gradcam" sum_c alpha_t[c] A[t, p, c] with
                    alpha_t the mean of G over the positions of FRAME t (the backbone is a 2D network applied per frame:
                    each frame is its own image).
            frame_relevance[t] = sum_c g_t[c] f_t[c], the signed gradient x input on the pooled features: the temporal
                    attribution, which needs no spatial map (vc_frame_cam with P = 1).

        Returns vivit.Explanation: `logits` f32 [B, 1] on the device, bit-identical to model(video) / forward_ragged
        (the recurrence kernels are instantiations of one step loop); on the host `token_relevance` f32 [B, T*h*w], the
        SIGNED map in the row order (t*h + y)*w + x, `saliency` f32 [B, T, h, w] = relu(map) / its per-video sum (all
        zero when nothing is positive), `temporal` f32 [B, T] (saliency summed over space), `frame_relevance` f32 [B, T]
        (signed), `method`, and `target`, B ints in {0, 1}.  Ragged: token_relevance, saliency, temporal and
        frame_relevance are lists of per-video tensors ([n*h*w], [n, h, w], [n], [n]).

        Runs the eager inference launches with the backbone activations after the layer, each LSTM layer's gates and
        cell states and the head's hidden row kept in buffers of its own (cached per shape); the forward's workspaces
        and packed weights are untouched.  Refuses (no fallback): training mode, CPU tensors, an unknown method or
        layer ("res2" / "res3" are not supported), a target outside {0, 1} or of the wrong length, a video that is
        not [B, 3, T, H, W] (ragged: [1, 3, N, H, W] with lengths >= 1 that sum to N)."""
        explaining.require_method(method, self.EXPLAIN_METHODS)
        if layer not in self.EXPLAIN_LAYERS:
            raise ValueError(f"explain: layer must be one of {self.EXPLAIN_LAYERS}, not {layer!r}")
        explaining.require_explainable(self, video)
        if lengths is None:
            if video.dim() != 5 or video.shape[1] != 3 or video.shape[0] < 1 or video.shape[2] < 1:
                raise ValueError(f"video {tuple(video.shape)} must be [B, 3, T, H, W]")
            nseq = video.shape[0]
        else:
            lengths = tuple(int(n) for n in lengths)
            if video.dim() != 5 or video.shape[0] != 1 or video.shape[1] != 3:
                raise ValueError(f"video {tuple(video.shape)} must be [1, 3, N, H, W]: the frames of all videos back to back")
            if not lengths or min(lengths) < 1 or sum(lengths) != video.shape[2]:
                raise ValueError(f"lengths {lengths} must be >= 1 and sum to the {video.shape[2]} frames of video")
            nseq = len(lengths)
        target = self._explain_targets(target, nseq)
        x = video.contiguous().float() if video.dtype != torch.float32 else video.contiguous()
        Bb, _, T, Hh, Ww = x.shape
        rows, dev, H = Bb * T, x.device, self.hidden
        bb = self.backbone
        pk, bpk = self._pack(dev), bb._pack(dev)
        buf = bb._explain_buffers(Bb, T, Hh, Ww, layer, dev)
        bb._pack_transposed(bpk, buf["stage"] + 1)
        # forward: the inference launches, with what the backward reads kept
        act, _, (_, h, w), Cf, _ = bb.forward_features(x, keep=buf)
        P, (_, hl, wl), Cl = h * w, buf["grid"], buf["C"]
        Pl = hl * wl
        ws = self._explain_workspace(rows, nseq, Pl, Cl, dev)
        ops.frame_avgpool(act, rows, P, Cf, ws["feat"])
        inp = ws["feat"]
        dense_T = T if lengths is None else None
        for l, L in enumerate(pk["layers"]):
            hseq = ws["hseq"][l & 1]
            ops.gemm(inp, L["wb"], L["b"], "bias_f32", ws["pre"], op="lstm_ih")
            ops.lstm_seq_fwd_train_state(ws["pre"], lengths, H, L["w_hh_t"], hseq, ws["h_n"][l], ws["c_n"][l], ws["gates"][l],
                                         ws["c_seq"][l], ws["h_prev"], T=dense_T)
            inp = hseq
        logits, target = self._head_gradient(pk, ws["head"], ws["h_n"][self.layers - 1], target)
        # backward: exact BPTT from the top layer's h_n down to the pooled features, fp32 throughout
        dh_seq = None
        for l in range(self.layers - 1, -1, -1):
            L = pk["layers"][l]
            ops.lstm_seq_bwd_state(ws["gates"][l], ws["c_seq"][l], nseq, lengths, H, L["w_hh"], ws["dpre"], ws["dpb"],
                                   dh_seq=dh_seq, dh_n=ws["head"]["dh"] if dh_seq is None else None, T=dense_T)
            dh_seq = self._lstm_dx(ws["dpb"], L["wt"], ws["g"] if l == 0 else ws["dxh"])
        g = ws["g"]
        ops.frame_cam(ws["feat"], g, rows, 1, Cf, ws["frame_map"], ws["frame_rel"])
        if not buf["chain"]:  # res5: both methods, the same launch
            ops.frame_cam(buf["x"], g, rows, P, Cf, ws["map"], ws["map_rel"])
        else:
            ops.frame_avgpool_bwd(g, rows, P, Cf, buf["seed"])
            G = bb._explain_chain(buf, Bb)
            if method == "gradcam":
                ops.cam_weights(G, rows, Pl, Cl, ws["cam_work"], ws["alpha"])
                ops.cam_map("gradcam", buf["x"], ws["alpha"], rows, Pl, Cl, ws["map"])
            else:
                ops.cam_map("hirescam", buf["x"], G, rows, Pl, Cl, ws["map"])
        both = torch.cat([ws["map"], ws["frame_rel"]]).cpu()  # the one copy; the rest is host bookkeeping
        rel, frel = both[: rows * Pl], both[rows * Pl:]
        sign = torch.tensor([1.0 if t else -1.0 for t in target]).repeat_interleave(
            torch.tensor([T] * nseq if lengths is None else lengths))  # per frame row: target 0 explains -z
        rel, frel = (rel.reshape(rows, Pl) * sign[:, None]).reshape(-1), frel * sign
        if lengths is None:
            rel, frel = rel.reshape(nseq, T * Pl).contiguous(), frel.reshape(nseq, T).contiguous()
            sal = torch.stack([self._positive_share(r) for r in rel]).reshape(nseq, T, hl, wl)
            return Explanation(logits, rel, sal, sal.sum(dim=(2, 3)), method, target=target, frame_relevance=frel)
        rels, frels, sals, r0 = [], [], [], 0
        for n in lengths:
            rels.append(rel[r0 * Pl: (r0 + n) * Pl].clone())
            frels.append(frel[r0: r0 + n].clone())
            sals.append(self._positive_share(rels[-1]).reshape(n, hl, wl))
            r0 += n
        return Explanation(logits, rels, sals, [s.sum(dim=(1, 2)) for s in sals], method, target=target,
                           frame_relevance=frels)

    def explain_stream_begin(self, B: int) -> "ExplainSession":
        """A whole-recording explanation in chunks, for B recordings: see ExplainSession."""
        if self.training:
            raise RuntimeError("explain: inference only; call model.eval() first")
        if not isinstance(B, int) or B < 1:
            raise ValueError("explain_stream_begin: B must be an int >= 1")
        return ExplainSession(self, B)

    def _forward_train(self, video: torch.Tensor) -> torch.Tensor:
        B, _, T = video.shape[:3]
        return self._forward_tail(self.features(video, train_bn=not self.freeze_backbone_bn)[: B * T], B, T)

    def _forward_tail(self, x: torch.Tensor, B: int, T: int) -> torch.Tensor:
        """The trainable part of the train step on the bf16 features [B*T, 2048]: the LSTM layers and the
        head as autograd ops, with their dropout masks."""
        dev = x.device
        pk = self._pack(dev)
        p = self.dropout
        keeps = []
        h_last = None
        for l in range(self.layers):
            top = l == self.layers - 1
            keep = None
            if p > 0.0 and not top:  # nn.LSTM: dropout on the outputs of every layer but the last
                keep = torch.ones(B * T, self.hidden, device=dev).bernoulli_(1.0 - p).mul_(1.0 / (1.0 - p))
            keeps.append(keep)
            x, h_last = A.lstm_layer(x, self.P(f"lstm.weight_ih_l{l}"), self.P(f"lstm.weight_hh_l{l}"),
                                     self.P(f"lstm.bias_ih_l{l}"), self.P(f"lstm.bias_hh_l{l}"), B, T, keep=keep,
                                     last_only=top, need_dx=l > 0, packed=pk["layers"][l])
        hkeep = None
        if p > 0.0:
            hkeep = torch.ones(B, HEAD_DIM, device=dev).bernoulli_(1.0 - p).mul_(1.0 / (1.0 - p))
        self.last_keep = {"lstm": keeps, "head": hkeep}
        return A.mlp_head(h_last, self.P("classifier.0.weight"), self.P("classifier.0.bias"),
                          self.P("classifier.3.weight"), self.P("classifier.3.bias"), hkeep)


class ExplainSession:
    """Which frames of whole recordings produced the logit, at bounded GPU memory per chunk
    (VideoResNet50LSTM.explain_stream_begin(B)):

        sess = model.explain_stream_begin(B)
        for video, lengths in chunks:                  # forward_stream's arguments
            logits, frame_logits = sess.push(video, lengths)
        ex = sess.finish(target=None)

    push runs forward_stream's launches (the recurrence in its saving instantiation) and returns (logits f32 [B, 1],
    frame logits f32 [N, 1]), bit-identical to forward_stream(video, lengths, state, frame_logits=True); the state is
    carried inside the session.  Per chunk it keeps the bf16 pooled features, each layer's gates and cell states, each
    layer's incoming c0 and the row layout: 2 * 2048 + layers * (16 + 4) * hidden bytes per frame, 14336 B (14 KB) at
    hidden 256 and two layers, plus layers * B * hidden * 4 bytes of c0 per chunk -- a 10-minute recording at 30
    frames/s is 258 MB.  No backbone activation is kept: there are no spatial maps in this mode.

    finish walks the chunks in reverse: the head's dh enters at each recording's h_n, vc_lstm_seq_bwd_state chains dh0
    / dc0 into the previous chunk's dh_n / dc_n (a recording that paused with length 0 passes them through), and each
    chunk's g goes through vc_frame_cam with P = 1.  It returns vivit.Explanation with `logits` f32 [B, 1] on the
    device, `frame_relevance` a list of B f32 tensors (one entry per frame the recording pushed, signed; bit-identical
    to explain(..., lengths=...) on the whole recordings), `temporal` its positive part divided by its per-recording
    sum (all zero when nothing is positive), `target`, method "frame_relevance", and token_relevance = saliency =
    None.  One finish per session; push after it is refused."""

    def __init__(self, model: "VideoResNet50LSTM", B: int):
        self.model, self.B = model, B
        self.state = None
        self.chunks = []
        self.done = False

    @torch.no_grad()
    def push(self, video: torch.Tensor, lengths):
        m = self.model
        if self.done:
            raise RuntimeError("explain session: finish() was called; begin a new session")
        if m.training:
            raise RuntimeError("explain: inference only; call model.eval() first")
        x, lengths, B = m._stream_args(video, lengths, self.state)
        if B != self.B:
            raise ValueError(f"explain session: {B} lengths for the session's {self.B} recordings")
        N, dev, H, nl = x.shape[2], x.device, m.hidden, m.layers
        pk = m._pack(dev)
        act, _, (_, h, w), Cf, _ = m.backbone.forward_features(x)
        M, Hp = _ru(N, 256), _ru(H, 128)
        f32, bf = torch.float32, torch.bfloat16
        z = lambda r, c, dt=f32: torch.zeros(r, c, dtype=dt, device=dev)  # noqa: E731
        feat = z(M, Cf, bf)
        ops.frame_avgpool(act, N, h * w, Cf, feat)
        pre, hseq, h_prev, hall = z(M, _ru(4 * H, 128)), [z(M, Hp, bf) for _ in range(2)], z(M, Hp, bf), z(M, H)
        old = self.state
        new = LstmState(torch.empty(nl, B, H, dtype=f32, device=dev), torch.empty(nl, B, H, dtype=f32, device=dev))
        gates, c_seq = [z(N, 4 * H) for _ in range(nl)], [z(N, H) for _ in range(nl)]
        inp = feat
        for l, L in enumerate(pk["layers"]):
            h0, c0 = (None, None) if old is None else (old.h[l], old.c[l])
            ops.gemm(inp, L["wb"], L["b"], "bias_f32", pre, op="lstm_ih")
            ops.lstm_seq_fwd_train_state(pre, lengths, H, L["w_hh_t"], hseq[l & 1], new.h[l], new.c[l], gates[l], c_seq[l],
                                         h_prev, h0=h0, c0=c0)
            if l == nl - 1:  # the unrounded h of every frame for the frame logits: the inference instantiation again
                ops.lstm_seq_fwd_state(pre, lengths, H, L["w_hh_t"], h_prev, torch.empty_like(new.h[l]),
                                       torch.empty_like(new.c[l]), h0=h0, c0=c0, h_all=hall)
            inp = hseq[l & 1]
        w1, b1, w2, b2 = pk["head"]
        logits = ops.mlp_head_fwd(new.h[nl - 1], w1, b1, w2, b2, torch.empty(B, 1, dtype=f32, device=dev))
        frames = ops.mlp_head_fwd(hall[:N], w1, b1, w2, b2, torch.empty(N, 1, dtype=f32, device=dev))
        self.chunks.append(dict(lengths=lengths, feat=feat[:N], gates=gates, c_seq=c_seq,
                                c0=None if old is None else old.c))
        self.state = new
        return logits, frames

    @torch.no_grad()
    def finish(self, target=None):
        m = self.model
        if self.done:
            raise RuntimeError("explain session: finish() was already called")
        if not self.chunks:
            raise RuntimeError("explain session: finish() before any push()")
        B, H, nl = self.B, m.hidden, m.layers
        target = m._explain_targets(target, B)
        dev = self.state.h.device
        pk = m._pack(dev)
        hb = m._head_buffers(B, dev)
        logits, target = m._head_gradient(pk, hb, self.state.h[nl - 1], target)
        f32 = torch.float32
        dH, dC = torch.zeros(nl, B, H, dtype=f32, device=dev), torch.zeros(nl, B, H, dtype=f32, device=dev)
        dH[nl - 1].copy_(hb["dh"])
        per = [[] for _ in range(B)]  # per recording, its chunks' relevance, last chunk first
        for ch in reversed(self.chunks):
            N, lengths = ch["feat"].shape[0], ch["lengths"]
            M = _ru(N, 256)
            dpre = torch.empty(N, 4 * H, dtype=f32, device=dev)
            dpb = torch.zeros(M, _ru(4 * H, 128), dtype=torch.bfloat16, device=dev)
            dh_seq = None
            for l in range(nl - 1, -1, -1):
                L = pk["layers"][l]
                ops.lstm_seq_bwd_state(ch["gates"][l], ch["c_seq"][l], B, lengths, H, L["w_hh"], dpre, dpb, dh_seq=dh_seq,
                                       dh_n=dH[l], dc_n=dC[l], c0=None if ch["c0"] is None else ch["c0"][l], dh0=dH[l],
                                       dc0=dC[l])
                dh_seq = m._lstm_dx(dpb, L["wt"], torch.empty(M, L["wt"].shape[0], dtype=f32, device=dev))
            frel = torch.empty(N, dtype=f32, device=dev)
            ops.frame_cam(ch["feat"], dh_seq, N, 1, ch["feat"].shape[1], torch.empty(N, dtype=f32, device=dev), frel)
            frel, r0 = frel.cpu(), 0
            for b, n in enumerate(lengths):
                per[b].append(frel[r0: r0 + n] * (1.0 if target[b] else -1.0))  # target 0 explains -z
                r0 += n
        self.done, self.chunks = True, []
        frels = [torch.cat(list(reversed(p))).contiguous() for p in per]
        return Explanation(logits, None, None, [m._positive_share(r) for r in frels], "frame_relevance", target=target,
                           frame_relevance=frels)


def create_model(hidden_size: int = 256, num_layers: int = 2, dropout: float = 0.5, device="cuda",
                 weights_seed: int = 0):
    """VideoResNet50LSTM with seeded synthetic weights (the reference loads torchvision's
    IMAGENET1K_V1 ResNet-50, unavailable offline; load a checkpoint with load_state_dict)."""
    from .weights import make_resnet50_lstm_weights
    m = VideoResNet50LSTM(hidden_size, num_layers, dropout)
    sd = make_resnet50_lstm_weights(seed=weights_seed, hidden=hidden_size)
    if num_layers != 2:  # the seeded weights cover two layers: further layers keep layer 1's distribution
        rng = np.random.RandomState(weights_seed + 2)
        k = 1.0 / np.sqrt(hidden_size)
        shapes = resnet50_lstm_param_shapes(hidden_size, num_layers)
        sd = OrderedDict((n, sd[n] if n in sd else rng.uniform(-k, k, shapes[n]).astype(np.float32)) for n in shapes)
    m.load_state_dict(sd)
    return m.to(device) if device else m
