"""3D ResNet-50 (pytorchvideo `create_resnet` as the reference configures it) on the
libvclip.so kernels — drop-in for `create_model(logger)` of
resnet50-3d-video/video_classifier/models/resnet3d.py:4-48, called as
`model(f32[B, 3, T, H, W])` -> `f32[B, 2]` (resnet50-3d-video trainer / inference.py:399).

Every Conv3d + BatchNorm(eval) [+ ReLU] [+ residual] is one GEMM: BN is folded into the
weights and bias in fp32 before the bf16 cast, ReLU and the bottleneck's skip add are GEMM
epilogues; 1x1x1 stride-1 convolutions read the activations directly, the others go through
vc_conv3d_im2col.  Activations are channels-last bf16 rows ((b*T + t)*H + h)*W + w; rows are
padded to a multiple of 256 and output channels to a multiple of 128 (zero weights, so the
padding columns are exactly 0).  The head (AvgPool3d (4,7,7) stride 1 -> Linear ->
global average) is one position-weighted pooling + GEMV (the Linear commutes with both means).

Parity unpinned against pytorchvideo itself (not installed here): checked against
oracle/resnet3d_ref.py, the restatement of pytorchvideo's create_resnet.
"""
from __future__ import annotations

import torch

from . import explaining, ops
from .explaining import Explanation
from .hosting import FusedVideoModel, round_up as _ru
from .weights import resnet3d_param_shapes

RESNET3D_50 = dict(depths=(3, 4, 6, 3), stem_dim=64, conv_a_kernels=((1, 1, 1), (1, 1, 1), (3, 1, 1), (3, 1, 1)),
                   spatial_strides=(1, 2, 2, 2), head_pool=(4, 7, 7), num_classes=2, bn_eps=1e-5,
                   stem_kernel=(3, 7, 7), stem_pad=(1, 3, 3))


class ResNet3d(FusedVideoModel):
    """fp32 master parameters + BatchNorm running statistics in pytorchvideo naming."""

    def __init__(self, cfg: dict = RESNET3D_50):
        # BatchNorm running statistics are buffers in pytorchvideo: no gradient, updated by the train step
        super().__init__(resnet3d_param_shapes(dict(cfg)), cfg.get("num_classes", 2),
                         frozen=lambda n: n.endswith("running_mean") or n.endswith("running_var"))
        self.cfg = dict(cfg)
        self.head_dropout = True  # train step: the head's Dropout(0.5) (pytorchvideo create_resnet dropout_rate)
        # inference convolutions other than 1x1x1 stride 1 as implicit GEMMs (vc_conv3d_gemm_bf16: the
        # A rows gathered from the activations per kernel tap, no im2col buffer); False: im2col + GEMM.
        # The bottleneck convolutions are bit-identical either way (same MFMA chain per output, same
        # column order); the implicit stem sums its 441 products in another k order, so the stem (and
        # the logits) agree with the im2col path to bf16 rounding.
        self.implicit_conv = True
        # LDS ring depth of the implicit convolutions per res stage ("s2" .. "s5" -> 2 or 3;
        # vc_conv3d_gemm_bf16_ring), absent = automatic by grid size (bit-identical for any setting)
        self.conv_ring = {}
        # per-convolution overrides {"conv_a.s4": (ring, tile), ...} of vc_conv3d_gemm_bf16_cfg (tile 0 auto,
        # 1 = 64 x 128, 2 = 128 x 128; ring 0 auto, 2, 3, 4); bit-identical for any setting
        self.conv_cfg = {}

    def _conv_kw(self, op: str, s: int) -> dict:
        ring, tile = self.conv_cfg.get(op, (self.conv_ring.get(f"s{s + 2}", 0), 0))
        return dict(ring=ring, tile=tile)

    def _clean_state_dict(self, sd):
        return {k: v for k, v in super()._clean_state_dict(sd).items() if not k.endswith("num_batches_tracked")}

    # ---- packing: BN folded, weights [N_pad, K] bf16 in the im2col column order --------
    def _pack(self, device):
        pk = self._cached_pack(device)
        if pk is not None:
            return pk
        ops.zero_row(device)  # the implicit convs' padding row, zeroed on the caller's stream before any fork
        c = self.cfg
        eps = c["bn_eps"]
        P = lambda n: self.params[n.replace(".", "__")].detach().to(device=device, dtype=torch.float64)  # noqa: E731

        def fold(conv, bn, channels_last=True, k_pad=None):
            w = P(conv + ".weight")
            sc = P(bn + ".weight") / torch.sqrt(P(bn + ".running_var") + eps)
            b = P(bn + ".bias") - P(bn + ".running_mean") * sc
            w = w * sc.view(-1, 1, 1, 1, 1)
            w = (w.permute(0, 2, 3, 4, 1) if channels_last else w).reshape(w.shape[0], -1)
            n_p = _ru(w.shape[0], 128)
            k = w.shape[1] if k_pad is None else k_pad
            W = torch.zeros((n_p, k), dtype=torch.float64, device=device)
            W[:w.shape[0], :w.shape[1]] = w
            B = torch.zeros(n_p, dtype=torch.float64, device=device)
            B[:b.numel()] = b
            return W.to(torch.bfloat16).contiguous(), B.float().contiguous()

        pk = {"device": device, "version": self._weights_version()}
        sk = c.get("stem_kernel", (3, 7, 7))
        pk["stem"] = fold("blocks.0.conv", "blocks.0.norm", channels_last=False, k_pad=_ru(3 * sk[0] * sk[1] * sk[2], 64))
        if sk[2] <= 8:
            # the implicit stem GEMM's segment columns: seg = kt_i * kh + kh_i, column seg*32 + kw_i*4 + c
            w = P("blocks.0.conv.weight")
            scl = P("blocks.0.norm.weight") / torch.sqrt(P("blocks.0.norm.running_var") + eps)
            w = w * scl.view(-1, 1, 1, 1, 1)
            co, ci = w.shape[0], w.shape[1]
            nseg = sk[0] * sk[1]
            Wseg = torch.zeros((_ru(co, 128), 64 * ((nseg + 1) // 2)), dtype=torch.float64, device=device)
            ws_ = torch.zeros((co, sk[0], sk[1], 8, 4), dtype=torch.float64, device=device)
            ws_[:, :, :, :sk[2], :ci] = w.permute(0, 2, 3, 4, 1)
            Wseg[:co, :nseg * 32] = ws_.reshape(co, nseg * 32)
            pk["stem_seg"] = (Wseg.to(torch.bfloat16).contiguous(), pk["stem"][1])
        stages = []
        din, dout = c["stem_dim"], c["stem_dim"] * 4
        for s, depth in enumerate(c["depths"]):
            blocks = []
            for i in range(depth):
                p = f"blocks.{s + 1}.res_blocks.{i}."
                blk = {}
                if p + "branch1_conv.weight" in self._names:
                    blk["b1"] = fold(p + "branch1_conv", p + "branch1_norm")
                blk["a"] = fold(p + "branch2.conv_a", p + "branch2.norm_a")
                blk["b"] = fold(p + "branch2.conv_b", p + "branch2.norm_b")
                blk["c"] = fold(p + "branch2.conv_c", p + "branch2.norm_c")
                blocks.append(blk)
            stages.append(dict(blocks=blocks, din=din, dout=dout, inner=dout // 4))
            din, dout = dout, dout * 2
        pk["stages"] = stages
        if "blocks.5.proj.weight" in self._names:
            pk["w_head"] = self.params["blocks__5__proj__weight"].detach().to(device).float().contiguous()
            pk["b_head"] = self.params["blocks__5__proj__bias"].detach().to(device).float().contiguous()
        self._packed = pk
        return pk

    # ---- geometry / workspace ---------------------------------------------------------
    def geometry(self, T, H, W):
        c = self.cfg
        stem = ops.conv_out_size((T, H, W), c.get("stem_kernel", (3, 7, 7)), (1, 2, 2), c.get("stem_pad", (1, 3, 3)))
        g = [ops.conv_out_size(stem, (1, 3, 3), (1, 2, 2), (0, 1, 1))]
        for s in range(1, len(c["depths"])):
            st = c["spatial_strides"][s]
            g.append(ops.conv_out_size(g[-1], (1, 3, 3), (1, st, st), (0, 1, 1)))
        return stem, g

    def _workspace(self, B, T, H, W, device, part: int = 0):
        return self._cached_workspace((B, T, H, W, str(device), part),
                                      lambda: self._make_workspace(B, T, H, W, device), 4)

    def _make_workspace(self, B, T, H, W, device):
        c = self.cfg
        stem, grids = self.geometry(T, H, W)
        bf = torch.bfloat16
        rows = lambda g: _ru(B * g[0] * g[1] * g[2], 256)  # noqa: E731
        z = lambda r, cols: torch.zeros((r, cols), dtype=bf, device=device)  # noqa: E731
        ws = {"stem_out": z(rows(stem), 128)}
        sp = c.get("stem_pad", (1, 3, 3))
        # + 8 pixels x 4 channels of slack: the implicit stem reads 8 pixels per tap row, so with kw < 8 the
        # last output window of the last row reads up to 8 - kw pixels past the packed clip (zero weights)
        ws["stem_pad"] = torch.zeros(B * (T + 2 * sp[0]) * (H + 2 * sp[1]) * (W + 2 * sp[2]) * 4 + 32, dtype=bf,
                                     device=device)
        # im2col scratch: the largest M x K of any convolution
        sk = c.get("stem_kernel", (3, 7, 7))
        big = rows(stem) * _ru(3 * sk[0] * sk[1] * sk[2], 64)
        din, dout = c["stem_dim"], c["stem_dim"] * 4
        g_in = grids[0]
        acts = []
        for s, depth in enumerate(c["depths"]):
            g = grids[s]
            inner = dout // 4
            ka = c["conv_a_kernels"][s]
            big = max(big, rows(g_in) * ka[0] * ka[1] * ka[2] * max(din, dout), rows(g) * 9 * inner,
                      rows(g) * din)
            acts.append(dict(x=z(rows(g), dout), x2=z(rows(g), dout), sc=z(rows(g), dout),
                             a=z(rows(g_in) if g_in != g else rows(g), _ru(inner, 128)), b=z(rows(g), _ru(inner, 128))))
            g_in = g
            din, dout = dout, dout * 2
        ws["x0"] = z(rows(grids[0]), c["stem_dim"])
        ws["acts"] = acts
        # im2col scratch (1.4 GB at B = 4 for the stem alone): allocated on first use, i.e. only by the
        # im2col path (implicit_conv = False)
        ws["col"] = None
        ws["col_elems"] = big
        ws["head_work"] = torch.zeros(B * T * 2048 * 33, dtype=torch.float32, device=device)
        ws["logits"] = torch.zeros((B, c["num_classes"]), dtype=torch.float32, device=device)
        return ws

    # ---- forward -----------------------------------------------------------------------
    def forward(self, video: torch.Tensor) -> torch.Tensor:
        """`model(clips)` -> logits.  In training mode (the reference's train loop,
        resnet50-3d-video/video_classifier/trainers/trainer.py:106-123) the HIP train step runs
        (_forward_train: BatchNorm with batch statistics and running-statistic updates, the head's
        dropout), with autograd enabled or not -- pytorchvideo in train mode under torch.no_grad keeps
        those semantics too; in eval mode the fused inference path (BatchNorm folded) runs."""
        if video.device.type != "cuda":
            raise RuntimeError("ResNet3d (vclip_amd) runs on the GPU only: move the clip batch to cuda")
        x = video.contiguous().float() if video.dtype != torch.float32 else video.contiguous()
        if self.training:
            return self._forward_train(x)
        with torch.no_grad():
            return self.forward_logits(x).clone()  # the workspace buffer is reused by the next call

    def _forward_train(self, video: torch.Tensor) -> torch.Tensor:
        """pytorchvideo create_resnet in training mode (oracle/resnet3d_ref.py with batch-statistic
        BatchNorm) as autograd ops over the HIP kernels (vclip_amd/autograd_ops.py): every Conv3d is
        an im2col (differentiable: col2im) + bf16 MFMA GEMM with fp32 accumulation on the fp32 master
        weights, BatchNorm3d with batch statistics (fp32, running statistics updated with momentum
        0.1) fused with the residual add and ReLU, MaxPool3d with its first-max gradient, and the head
        (AvgPool3d, Dropout(0.5) from torch's RNG unless `head_dropout = False`, Linear, global
        average); channels-last rows throughout."""
        from . import autograd_ops as A
        c = self.cfg
        x, B, (Tf, Hf, Wf), cin = self._forward_train_features(video)
        pt, ph, pw = c["head_pool"]
        if (ph, pw) != (Hf, Wf):
            raise NotImplementedError("train step head: the pool window must cover the final spatial map")
        npos = Tf - pt + 1
        keep = torch.ones(B, npos, cin, device=video.device)
        if self.head_dropout:
            keep = keep.bernoulli_(0.5).mul_(2.0)  # nn.Dropout(0.5): keep with prob 0.5, scale 1 / 0.5
        self._packed = None  # the running statistics were updated in place: re-fold before the next eval
        P = self.P
        return A.resnet_head(x, P("blocks.5.proj.weight"), P("blocks.5.proj.bias"), keep, B, Tf, Hf * Wf, pt)

    def _forward_train_features(self, video: torch.Tensor):
        """The train-mode stem and the four stages of _forward_train (batch-statistic BatchNorm, running
        statistics updated in place); returns (last activations bf16 [B*T*H*W, C], B, (T, H, W), C).
        The caller drops `_packed` (the folded inference weights) after it."""
        from . import autograd_ops as A
        c = self.cfg
        B, Cin, T, H, W = video.shape
        if Cin != 3:
            raise ValueError("video must be [B, 3, T, H, W]")
        eps = c["bn_eps"]
        stem, grids = self.geometry(T, H, W)
        sk, sp = c.get("stem_kernel", (3, 7, 7)), c.get("stem_pad", (1, 3, 3))
        P = self.P

        def bn(y, name, relu, res=None):
            return A.batchnorm(y, P(name + ".weight"), P(name + ".bias"), P(name + ".running_mean"),
                               P(name + ".running_var"), res=res, relu=relu, eps=eps)

        def conv(x, grid, cin, wname, kernel, stride, pad):
            w = P(wname)
            cout = w.shape[0]
            if tuple(kernel) == (1, 1, 1) and tuple(stride) == (1, 1, 1):
                a = x
            else:
                a = A.im2col_cl(x, B, grid, cin, kernel, stride, pad)
            return A.linear(a, w.permute(0, 2, 3, 4, 1).reshape(cout, -1), None, out_f32=True)

        # stem: Conv3d from the f32 NCTHW clip (no input gradient) + BN + ReLU + MaxPool
        Ms = B * stem[0] * stem[1] * stem[2]
        K = 3 * sk[0] * sk[1] * sk[2]
        a = torch.empty(Ms, _ru(K, 8), dtype=torch.bfloat16, device=video.device)
        ops.conv3d_im2col(video, "ncthw_f32", B, (T, H, W), 3, sk, (1, 2, 2), sp, a)
        y = A.linear(a[:, :K], P("blocks.0.conv.weight").reshape(c["stem_dim"], K), None, out_f32=True)
        x = A.maxpool(bn(y, "blocks.0.norm", True), B, stem, c["stem_dim"], (1, 3, 3), (1, 2, 2), (0, 1, 1))
        g_in, cin = grids[0], c["stem_dim"]
        for s, depth in enumerate(c["depths"]):
            g = grids[s]
            ss = c["spatial_strides"][s]
            ka = tuple(c["conv_a_kernels"][s])
            for i in range(depth):
                p = f"blocks.{s + 1}.res_blocks.{i}."
                stride = (1, ss, ss) if i == 0 else (1, 1, 1)
                gi = g_in if i == 0 else g
                if p + "branch1_conv.weight" in self._names:
                    sc = bn(conv(x, gi, cin, p + "branch1_conv.weight", (1, 1, 1), stride, (0, 0, 0)),
                            p + "branch1_norm", False)
                else:
                    sc = x
                inner = P(p + "branch2.conv_a.weight").shape[0]
                ya = bn(conv(x, gi, cin, p + "branch2.conv_a.weight", ka, (1, 1, 1), tuple(k // 2 for k in ka)),
                        p + "branch2.norm_a", True)
                yb = bn(conv(ya, gi, inner, p + "branch2.conv_b.weight", (1, 3, 3), stride, (0, 1, 1)),
                        p + "branch2.norm_b", True)
                x = bn(conv(yb, g, inner, p + "branch2.conv_c.weight", (1, 1, 1), (1, 1, 1), (0, 0, 0)),
                       p + "branch2.norm_c", True, res=sc)
                cin = P(p + "branch2.conv_c.weight").shape[0]
            g_in = g
        return x, B, grids[-1], cin

    def _check_input(self, video):
        if video.shape[1] != 3:
            raise ValueError("video must be [B, 3, T, H, W]")

    def _graph_knobs(self):
        return (self.implicit_conv, tuple(sorted(self.conv_ring.items())), tuple(sorted(self.conv_cfg.items())))

    def _forward_part(self, video: torch.Tensor, part: int, out=None, keep=None) -> torch.Tensor:
        """keep (explain only): forward_features' keep buffers; the head then pools in keep["head_work"]"""
        x, B, grid, C, ws = self.forward_features(video, part, keep=keep)
        pk = self._packed
        c = self.cfg
        Tf, Hf, Wf = grid
        pt, ph, pw = c["head_pool"]
        npos = (Tf - pt + 1) * (Hf - ph + 1) * (Wf - pw + 1)
        return ops.timed("avgpool_head", "head", B * Tf * Hf * Wf * C * 2 + npos * B * C * 4, "byte", ops.avgpool_head,
                         x, B, grid, C, c["head_pool"], pk["w_head"], pk["b_head"],
                         ws["head_work"] if keep is None else keep["head_work"], ws["logits"] if out is None else out)

    def forward_features(self, video: torch.Tensor, part: int = 0, keep=None):
        """Stem + the four stages; returns (last activations [rows, C] bf16, B, (T, H, W), C, workspace).
        keep (explain only, _explain_buffers): {"stage": s, "x": bf16 rows, "blocks": {(stage, block): {"a", "b",
        "out"}}} -- the last block of stage s writes its output to keep["x"] and every block of the later stages its
        conv_a / conv_b activations and its output to buffers of its own instead of the stage's shared ones (the same
        launches on other output pointers: bit-identical values)."""
        c = self.cfg
        B, C, T, H, W = video.shape
        if C != 3:
            raise ValueError("video must be [B, 3, T, H, W]")
        pk = self._pack(video.device)
        ws = self._workspace(B, T, H, W, video.device, part)
        stem, grids = self.geometry(T, H, W)
        rows = lambda g: _ru(B * g[0] * g[1] * g[2], 256)  # noqa: E731

        def col(m, k):
            if ws["col"] is None:
                ws["col"] = torch.zeros(ws["col_elems"], dtype=torch.bfloat16, device=video.device)
            return ws["col"][: m * k].view(m, k)

        # stem: conv (3,7,7)/(1,2,2) + BN + ReLU, then MaxPool (1,3,3)/(1,2,2)
        # (algorithmic work per launch for an installed ops.OpRecorder: real rows and channels; the
        # GEMMs run on rows padded to 256 and output channels padded to 128)
        tm = ops.timed
        vol = lambda g: B * g[0] * g[1] * g[2]  # noqa: E731
        sk = c.get("stem_kernel", (3, 7, 7))
        ks = 3 * sk[0] * sk[1] * sk[2]
        spad = c.get("stem_pad", (1, 3, 3))
        # (the implicit stem reads 16-B aligned 8-pixel rows of the padded clip: its padded width must be even)
        if self.implicit_conv and "stem_seg" in pk and (W + 2 * spad[2]) % 2 == 0:
            # the clip as zero-padded channels-last bf16 (4 channels), then the implicit stem GEMM
            tm("stem_pack_kernel", "stem_pack", B * 3 * T * H * W * 4 + ws["stem_pad"].numel() * 2, "byte",
               ops.conv3d_stem_pack, video, spad, ws["stem_pad"])
            ops.conv3d_stem_gemm(ws["stem_pad"], B, (T, H, W), sk, (1, 2, 2), spad, pk["stem_seg"][0], pk["stem_seg"][1],
                                 "bias_relu", ws["stem_out"], flop=2.0 * vol(stem) * c["stem_dim"] * ks, op="stem",
                                 n=_ru(c["stem_dim"], 64))
        else:
            Kst = pk["stem"][0].shape[1]
            A = col(rows(stem), Kst)
            tm("conv3d_im2col_kernel", "im2col", B * 3 * T * H * W * 4 + vol(stem) * ks * 2, "byte", ops.conv3d_im2col,
               video, "ncthw_f32", B, (T, H, W), 3, sk, (1, 2, 2), spad, A)
            ops.gemm(A, pk["stem"][0], pk["stem"][1], "bias_relu", ws["stem_out"],
                     flop=2.0 * vol(stem) * c["stem_dim"] * ks, op="stem")
        x = ws["x0"]
        tm("maxpool3d_kernel", "maxpool", (vol(stem) + vol(grids[0])) * c["stem_dim"] * 2, "byte", ops.maxpool3d,
           ws["stem_out"], B, stem, c["stem_dim"], (1, 3, 3), (1, 2, 2), (0, 1, 1), x)
        g_in, cin = grids[0], c["stem_dim"]
        for s, (st, act) in enumerate(zip(pk["stages"], ws["acts"])):
            g = grids[s]
            ss = c["spatial_strides"][s]
            ka = c["conv_a_kernels"][s]
            inner, dout = st["inner"], st["dout"]
            for i, blk in enumerate(st["blocks"]):
                stride = (1, ss, ss) if i == 0 else (1, 1, 1)
                gi = g_in if i == 0 else g
                xin = x
                kept = keep["blocks"].get((s, i)) if keep is not None else None
                ya, yb = (kept["a"], kept["b"]) if kept is not None else (act["a"], act["b"])
                # branch1: 1x1x1 conv (+ stride) + BN, or the identity
                if "b1" in blk:
                    fl = 2.0 * vol(g) * dout * cin
                    if stride == (1, 1, 1):
                        ops.gemm(xin, blk["b1"][0], blk["b1"][1], "bias", act["sc"], m=rows(g), flop=fl, op=f"branch1.s{s + 2}")
                    elif self.implicit_conv and cin % 64 == 0:
                        ops.conv3d_gemm(xin, B, gi, cin, (1, 1, 1), stride, (0, 0, 0), blk["b1"][0], blk["b1"][1], "bias",
                                        act["sc"], flop=fl, op=f"branch1.s{s + 2}", **self._conv_kw(f"branch1.s{s + 2}", s))
                    else:
                        A = col(rows(g), cin)
                        tm("conv3d_im2col_kernel", "im2col", (vol(gi) + vol(g)) * cin * 2, "byte", ops.conv3d_im2col,
                           xin, "cl_bf16", B, gi, cin, (1, 1, 1), stride, (0, 0, 0), A)
                        ops.gemm(A, blk["b1"][0], blk["b1"][1], "bias", act["sc"], flop=fl, op=f"branch1.s{s + 2}")
                    skip = act["sc"]
                else:
                    skip = xin
                # conv_a (+ BN + ReLU) at the block's input resolution
                fl = 2.0 * vol(gi) * inner * cin * ka[0] * ka[1] * ka[2]
                if tuple(ka) == (1, 1, 1) and self.implicit_conv and inner % 128 and inner % 64 == 0 and cin % 64 == 0:
                    # 64 output channels: the 256 x 64 implicit-GEMM tile (no MFMAs on the zero-padded channels)
                    ops.conv3d_gemm(xin, B, gi, cin, ka, (1, 1, 1), (0, 0, 0), blk["a"][0], blk["a"][1], "bias_relu",
                                    ya, flop=fl, op=f"conv_a.s{s + 2}", n=inner, **self._conv_kw(f"conv_a.s{s + 2}", s))
                elif tuple(ka) == (1, 1, 1):
                    ops.gemm(xin, blk["a"][0], blk["a"][1], "bias_relu", ya, m=rows(gi), flop=fl, op=f"conv_a.s{s + 2}")
                elif self.implicit_conv and cin % 64 == 0:
                    ops.conv3d_gemm(xin, B, gi, cin, ka, (1, 1, 1), tuple(k // 2 for k in ka), blk["a"][0], blk["a"][1],
                                    "bias_relu", ya, flop=fl, op=f"conv_a.s{s + 2}", n=_ru(inner, 64),
                                    **self._conv_kw(f"conv_a.s{s + 2}", s))
                else:
                    A = col(rows(gi), ka[0] * cin)
                    tm("conv3d_im2col_kernel", "im2col", vol(gi) * cin * 2 * (1 + ka[0]), "byte", ops.conv3d_im2col,
                       xin, "cl_bf16", B, gi, cin, ka, (1, 1, 1), tuple(k // 2 for k in ka), A)
                    ops.gemm(A, blk["a"][0], blk["a"][1], "bias_relu", ya, flop=fl, op=f"conv_a.s{s + 2}")
                # conv_b (1,3,3) with the stage stride (+ BN + ReLU)
                if self.implicit_conv and inner % 64 == 0:
                    ops.conv3d_gemm(ya, B, gi, inner, (1, 3, 3), stride, (0, 1, 1), blk["b"][0], blk["b"][1],
                                    "bias_relu", yb, flop=2.0 * vol(g) * inner * inner * 9, op=f"conv_b.s{s + 2}",
                                    n=_ru(inner, 64), **self._conv_kw(f"conv_b.s{s + 2}", s))
                else:
                    A = col(rows(g), 9 * inner)
                    tm("conv3d_im2col_kernel", "im2col", (vol(gi) + 9 * vol(g)) * inner * 2, "byte", ops.conv3d_im2col,
                       ya, "cl_bf16", B, gi, inner, (1, 3, 3), stride, (0, 1, 1), A)
                    ops.gemm(A, blk["b"][0], blk["b"][1], "bias_relu", yb, flop=2.0 * vol(g) * inner * inner * 9,
                             op=f"conv_b.s{s + 2}")
                # conv_c 1x1x1 + BN + skip + ReLU
                if kept is not None:
                    out = kept["out"]
                elif keep is not None and s == keep["stage"] and i == len(st["blocks"]) - 1:
                    out = keep["x"]
                else:
                    out = act["x"] if xin is not act["x"] else act["x2"]
                # HBM-bound at every stage (K = inner = 64 .. 512 against a bf16 residual in and a bf16
                # output: 28 .. 229 flop/B, below the 312 flop/B ridge): filed under its bytes
                ops.gemm(yb[:, :inner], blk["c"][0], blk["c"][1], "bias_resid_relu", out, aux=skip,
                         op=f"conv_c.s{s + 2}", nbytes=2.0 * (vol(g) * (inner + 2 * dout) + dout * inner))
                x, cin = out, dout
            g_in = g
        return x, B, grids[-1], cin, ws


    # ---- explain: Grad-CAM / HiResCAM ---------------------------------------------------
    EXPLAIN_METHODS = ("gradcam", "hirescam")
    EXPLAIN_LAYERS = ("res5", "res4")  # res2 / res3: out of scope

    def _pack_transposed(self, pk, first_stage: int):
        """pk["wt"][s][i]: the transposed folded bf16 weights {"b1", "a", "b", "c"} -> [roundup(K, 128), N] of the
        blocks of stages >= first_stage, built on the first explain that needs them and cached with the packed
        weights (same key).  BatchNorm is folded into the weight, so its transpose is the exact data-gradient
        operand of the eval-mode convolution; rows past K are zero (the GEMM's output-column padding)."""
        wt = pk.setdefault("wt", {})
        for s in range(first_stage, len(pk["stages"])):
            if s in wt:
                continue
            st = pk["stages"][s]
            blocks = []
            for blk in st["blocks"]:
                t = {}
                for name, cout in (("b1", st["dout"]), ("a", st["inner"]), ("b", st["inner"]), ("c", st["dout"])):
                    if name not in blk:
                        continue
                    if cout % 64:
                        raise NotImplementedError(f"explain: the data-gradient GEMMs need channel counts % 64 == 0, not {cout}")
                    w = blk[name][0]
                    m = torch.zeros((_ru(w.shape[1], 128), cout), dtype=torch.bfloat16, device=w.device)
                    m[:w.shape[1]] = w[:cout].t()
                    t[name] = m
                blocks.append(t)
            wt[s] = blocks
        return wt

    def _explain_buffers(self, B, T, H, W, layer, device):
        """The kept activations (forward_features' keep) and the chain's gradient buffers, cached per (B, geometry,
        layer, device).  Per block after the layer: its a / b / output, its masked output gradient `d`, and the two
        gradients its input receives (dIn, and dsk when the skip is a convolution); the GEMM and col2im outputs
        consumed at once are shared scratch, sized by the largest block."""
        return self._cached_explain(self._explain_ws, (B, T, H, W, layer, str(device)),
                                    lambda: self._build_explain_buffers(B, T, H, W, layer, device))

    def _build_explain_buffers(self, B, T, H, W, layer, device):
        c, pk = self.cfg, self._packed
        n = len(c["depths"])
        ls = n - 1 if layer == "res5" else n - 2
        _, grids = self.geometry(T, H, W)
        bf, f32 = torch.bfloat16, torch.float32
        rows = lambda g: _ru(B * g[0] * g[1] * g[2], 256)  # noqa: E731
        z = lambda r, cols, dt=bf: torch.zeros((r, cols), dtype=dt, device=device)  # noqa: E731
        Cl, Cf = pk["stages"][ls]["dout"], pk["stages"][-1]["dout"]
        gl, gf = grids[ls], grids[-1]
        Nl = gl[0] * gl[1] * gl[2]
        buf = dict(stage=ls, grid=gl, C=Cl, x=z(rows(gl), Cl), blocks={}, chain=[],
                   head_work=torch.zeros(B * Cf * 33, dtype=f32, device=device),
                   logits=torch.zeros((B, c["num_classes"]), dtype=f32, device=device),
                   target=torch.zeros(B, dtype=torch.int32, device=device), seed=z(rows(gf), Cf),
                   alpha=torch.zeros((B, Cl), dtype=f32, device=device), cam_work=ops.cam_weights_work(B, Cl, device),
                   map=torch.zeros(B * Nl, dtype=f32, device=device))
        big = {}

        def scratch(name, r, cols):
            big[name] = max(big.get(name, 0), r * cols)

        for s in range(ls + 1, n):
            st = pk["stages"][s]
            g, inner, dout = grids[s], st["inner"], st["dout"]
            ip = _ru(inner, 128)
            ka = tuple(c["conv_a_kernels"][s])
            kv = ka[0] * ka[1] * ka[2]
            ss = c["spatial_strides"][s]
            for i, blk in enumerate(st["blocks"]):
                gi = grids[s - 1] if i == 0 else g
                cin = st["din"] if i == 0 else dout
                stride = (1, ss, ss) if i == 0 else (1, 1, 1)
                buf["blocks"][(s, i)] = dict(a=z(rows(gi), ip), b=z(rows(g), ip), out=z(rows(g), dout))
                ch = dict(s=s, i=i, g=g, gi=gi, cin=cin, inner=inner, dout=dout, stride=stride, ka=ka, d=z(rows(g), dout))
                if "b1" in blk:
                    if stride != (1, 1, 1):
                        scratch("tsk", rows(g), _ru(cin, 128))
                        ch["dsk"] = z(rows(gi), cin, f32)
                    else:
                        ch["dsk"] = z(rows(g), _ru(cin, 128))
                if kv > 1:
                    scratch("ta", rows(gi), _ru(kv * cin, 128))
                    ch["dIn"] = z(rows(gi), cin, f32)
                else:
                    ch["dIn"] = z(rows(gi), _ru(cin, 128))
                scratch("tc", rows(g), ip)
                scratch("dB", rows(g), ip)
                scratch("tb", rows(g), _ru(9 * inner, 128))
                scratch("cb", rows(gi), inner)
                scratch("dA", rows(gi), ip)
                buf["chain"].append(ch)
        buf["scratch"] = {k: torch.zeros(v, dtype=f32 if k == "cb" else bf, device=device) for k, v in big.items()}
        if buf["chain"]:
            buf["g"] = z(rows(gl), Cl)
        buf["kept_bytes"] = buf["x"].numel() * 2 + sum(t.numel() * 2 for kb in buf["blocks"].values() for t in kb.values())
        return buf

    def _explain_chain(self, buf, B: int) -> torch.Tensor:
        """The eval-mode data-gradient chain from buf["seed"] (the gradient at the last block's post-ReLU output) back
        to the explained layer: bf16 [rows, C_layer], the gradient of the target logit with respect to that layer's
        activations.  No weight gradient is formed.  Per block, last first, with dOut = (d1 [, d2]):

            d   = relu_bwd(out, d1 [, d2])                          the output ReLU, joining the two gradients
            dsk = d | col2im_(1,1,1),stride(gemm(d, W1^T))          identity skip | branch1
            dB  = relu_bwd(b, gemm(d, Wc^T))
            dA  = relu_bwd(a, col2im_(1,3,3),stride(gemm(dB, Wb^T)))
            dIn = col2im_(kt,1,1)(gemm(dA, Wa^T))                   the GEMM output itself when kt = 1

        and (dIn, dsk) is the next block's dOut; at the layer they are joined unmasked (relu_bwd with y = None)."""
        from .autograd_ops import _zeros_f32
        if not buf["chain"]:
            return buf["seed"]
        wt = self._packed["wt"]
        dev = buf["seed"].device
        tm = ops.timed
        rows = lambda g: _ru(B * g[0] * g[1] * g[2], 256)  # noqa: E731
        vol = lambda g: B * g[0] * g[1] * g[2]  # noqa: E731
        view = lambda name, r, cols: buf["scratch"][name][: r * cols].view(r, cols)  # noqa: E731
        esz = lambda t: t.element_size()  # noqa: E731

        def relu(y, d1, M, C, out, d2=None):
            nb = M * C * (2 + esz(d1) + (2 if y is not None else 0) + (esz(d2) if d2 is not None else 0))
            return tm("relu_bwd_kernel", "cam.relu_bwd", nb, "byte", ops.relu_bwd, y, d1, M, C, out, d2)

        def dgrad(d, w, out, op):
            return ops.gemm(d, w, _zeros_f32(w.shape[0], dev), "bias", out, op=op)

        def col2im(da, grid, C, kernel, stride, pad, dx):
            kv = kernel[0] * kernel[1] * kernel[2]
            To, Ho, Wo = ops.conv_out_size(grid, kernel, stride, pad)
            return tm("col2im_cl_kernel", "cam.col2im", B * To * Ho * Wo * kv * C * 2 + vol(grid) * C * 4, "byte",
                      ops.col2im_cl, da, B, grid, C, kernel, stride, pad, dx)

        d1, d2 = buf["seed"], None
        for ch in reversed(buf["chain"]):
            s, g, gi, cin, inner, dout = ch["s"], ch["g"], ch["gi"], ch["cin"], ch["inner"], ch["dout"]
            kept, w = buf["blocks"][(s, ch["i"])], wt[s][ch["i"]]
            ip = _ru(inner, 128)
            d = relu(kept["out"], d1, vol(g), dout, ch["d"], d2)
            if "b1" not in w:
                dsk = d
            elif ch["stride"] != (1, 1, 1):
                tsk = dgrad(d, w["b1"], view("tsk", rows(g), _ru(cin, 128)), f"cam.dgrad.branch1.s{s + 2}")
                dsk = col2im(tsk, gi, cin, (1, 1, 1), ch["stride"], (0, 0, 0), ch["dsk"])
            else:
                dsk = dgrad(d, w["b1"], ch["dsk"], f"cam.dgrad.branch1.s{s + 2}")
            tc = dgrad(d, w["c"], view("tc", rows(g), ip), f"cam.dgrad.conv_c.s{s + 2}")
            dB = relu(kept["b"], tc, vol(g), inner, view("dB", rows(g), ip))
            tb = dgrad(dB[:, :inner], w["b"], view("tb", rows(g), _ru(9 * inner, 128)), f"cam.dgrad.conv_b.s{s + 2}")
            cb = col2im(tb, gi, inner, (1, 3, 3), ch["stride"], (0, 1, 1), view("cb", rows(gi), inner))
            dA = relu(kept["a"], cb, vol(gi), inner, view("dA", rows(gi), ip))
            ka = ch["ka"]
            kv = ka[0] * ka[1] * ka[2]
            if kv > 1:
                ta = dgrad(dA[:, :inner], w["a"], view("ta", rows(gi), _ru(kv * cin, 128)), f"cam.dgrad.conv_a.s{s + 2}")
                dIn = col2im(ta, gi, cin, ka, (1, 1, 1), tuple(k // 2 for k in ka), ch["dIn"])
            else:
                dIn = dgrad(dA[:, :inner], w["a"], ch["dIn"], f"cam.dgrad.conv_a.s{s + 2}")
            d1, d2 = dIn, dsk
        return relu(None, d1, vol(buf["grid"]), buf["C"], buf["g"], d2)

    @torch.no_grad()
    def explain(self, video: torch.Tensor, method: str = "gradcam", target=None, layer: str = "res5"):
        """The logits and which part of the clip produced logit `target`: Grad-CAM (Selvaraju et al. 2017) or HiResCAM
        (Draelos & Carin 2020) on the output of `layer` ("res5": T x H/32 x W/32, or "res4": T x H/16 x W/16).
        With A the layer's activations and G = d logit[target] / d A:

            "gradcam"   map[t, h, w] = sum_c mean_{t,h,w}(G)[c] * A[c, t, h, w]
            "hirescam"  map[t, h, w] = sum_c G[c, t, h, w] * A[c, t, h, w]

        G starts at the head in closed form (ops.cam_seed: AvgPool3d(stride 1) -> Linear -> global mean weights a
        position by the pool windows that cover it) and, for "res4", walks back through the res5 bottlenecks with
        their BatchNorms folded (_explain_chain: data-gradient GEMMs on the transposed folded weights, col2im, ReLU
        masks; no weight gradients).  At "res5" HiResCAM sums to logit - bias, and Grad-CAM on this linear head is
        classic CAM.  `target`: None (each clip's argmax), an int, or a sequence / tensor of B ints.

        Returns vivit.Explanation: `logits` f32 [B, classes] on the device (a clone); on the host `token_relevance`
        f32 [B, T*H_l*W_l], the SIGNED map in the row order (t*H_l + h)*W_l + w (the one copy), `saliency` f32
        [B, T, H_l, W_l] = relu(map) divided by its per-clip sum, `temporal` f32 [B, T] (saliency summed over space),
        `method`, and `target`, the B class indices.  A clip whose map has nothing positive -- no evidence FOR the
        class at that layer, common for the class the clip was not assigned to -- gets an all-zero `saliency` and
        `temporal`; `token_relevance` still holds its (non-positive) map.

        Runs the ordinary eager forward (one stream, no graph replay) with the activations after the layer kept in
        buffers of its own, cached per (B, geometry, layer, device); the forward's workspaces, packed weights, graphs
        and logits buffer are untouched.  Refuses (no fallback): training mode, CPU tensors, an unknown method or
        layer ("res2" / "res3" are not supported), a bad target, a video that is not [B, 3, T, H, W], a head pool
        that does not fit the final grid."""
        c = self.cfg
        explaining.require_method(method, self.EXPLAIN_METHODS)
        if layer not in self.EXPLAIN_LAYERS:
            raise ValueError(f"explain: layer must be one of {self.EXPLAIN_LAYERS}, not {layer!r}")
        explaining.require_explainable(self, video)
        if video.dim() != 5 or video.shape[1] != 3:
            raise ValueError(f"video {tuple(video.shape)} must be [B, 3, T, H, W]")
        B, _, T, H, W = video.shape
        target = explaining.expand_targets(*explaining.check_targets(target, c["num_classes"]), B)
        _, grids = self.geometry(T, H, W)
        gf = grids[-1]
        if any(k <= 0 or k > n for k, n in zip(c["head_pool"], gf)):
            raise ValueError(f"explain: the head pool {tuple(c['head_pool'])} does not fit the final grid {tuple(gf)}")
        x = video.contiguous().float() if video.dtype != torch.float32 else video.contiguous()
        pk = self._pack(x.device)
        if "w_head" not in pk:
            raise RuntimeError("explain: the model has no classification head (blocks.5.proj)")
        buf = self._explain_buffers(B, T, H, W, layer, x.device)
        self._pack_transposed(pk, buf["stage"] + 1)
        logits = self._forward_part(x, 0, out=buf["logits"], keep=buf).clone()
        if target is None:
            target = logits.argmax(dim=1).tolist()
        buf["target"].copy_(torch.tensor(target, dtype=torch.int32))
        Cf, (Tl, Hl, Wl), Cl = buf["seed"].shape[1], buf["grid"], buf["C"]
        Nl, Nf = Tl * Hl * Wl, gf[0] * gf[1] * gf[2]
        tm = ops.timed
        tm("cam_seed_kernel", "cam.seed", B * Nf * Cf * 2, "byte", ops.cam_seed, pk["w_head"], buf["target"], B, gf, Cf,
           c["head_pool"], buf["seed"])
        G = self._explain_chain(buf, B)
        if method == "gradcam":
            tm("cam_weights_kernels", "cam.weights", B * Nl * Cl * 2, "byte", ops.cam_weights, G, B, Nl, Cl, buf["cam_work"],
               buf["alpha"])
            tm("cam_map_kernel<false>", "cam.map", B * Nl * Cl * 2, "byte", ops.cam_map, "gradcam", buf["x"], buf["alpha"],
               B, Nl, Cl, buf["map"])
        else:
            tm("cam_map_kernel<true>", "cam.map", B * Nl * Cl * 4, "byte", ops.cam_map, "hirescam", buf["x"], G, B, Nl, Cl,
               buf["map"])
        rel = buf["map"].cpu().reshape(B, Nl)  # the one copy; the rest is host bookkeeping
        sal = explaining.normalise(rel.double().clamp_min(0), zero_ok=True).reshape(B, Tl, Hl, Wl)
        return Explanation(logits, rel, sal.contiguous(), sal.sum(dim=(2, 3)), method, target=target)


def create_model(logger=None, device="cuda", weights_seed: int = 0):
    """Drop-in for resnet50-3d-video/video_classifier/models/resnet3d.py:4-48 (random init there
    too: `create_resnet` without pretrained weights; here seeded synthetic weights)."""
    if logger:
        logger.info("Creating 3D ResNet-50 model...")
    model = ResNet3d(RESNET3D_50)
    from .weights import make_resnet3d_weights
    model.load_state_dict(make_resnet3d_weights(RESNET3D_50, seed=weights_seed))
    if logger:
        logger.info("Model created successfully")
    return model.to(device) if device else model
