"""TimeSformer-B (divided space-time attention) video classifier on the libvclip.so
kernels — drop-in for the reference's `create_model`
(timesformer/timesformer_classifier/models/timesformer_model.py:4-53), which returns an
HF `TimesformerForVideoClassification` called as `model(pixel_values=...)` and read
through `.logits` (timesformer/timesformer_classifier/trainers/trainer.py, inference.py).

Device data layout (B clips, T frames, P = (image/16)^2 patches, S = 1 + P*T tokens):
  clip layout   rows b*S + r, r = 0 (CLS) or 1 + p*T + t (patch-major, time-minor, the HF
                residual-stream order, TF5/models/timesformer/modeling_timesformer.py:121-143)
  frame layout  rows (b*T + t)*(1 + P) + j, j = 0 (CLS copy) or 1 + p: one spatial
                sequence per frame (:355-364), fed to the joint flash kernel with
                B' = B*T, S' = 1 + P
  both padded to Mpad = roundup(max(B*S, B*T*(1+P)) + 128, 256) rows;
  residual X f32 [Mpad, D] (clip), LN outputs bf16 (clip / frame), q|k|v bf16 [Mpad, 3D],
  attention out bf16 [Mpad, D], branch GEMM out bf16 [Mpad, D], MLP hidden bf16 [Mpad, 4D].
Per layer (TF5/.../modeling_timesformer.py:332-398):
  LN_t -> qkv_t GEMM -> temporal attention (VALU, T keys) -> one GEMM for
  temporal_attention.output.dense followed by temporal_dense (folded: W = Wtd.Wto,
  b = Wtd.bto + btd, in fp32 before the bf16 cast) -> [x += ., LN_before, permute to
  frame layout, CLS copied per frame] -> qkv_s GEMM -> flash attention -> output.dense
  GEMM -> [x += ., CLS += frame mean, LN_after] -> fc1 + exact GELU -> fc2 + residual.
"""
from __future__ import annotations

import json
import math

import torch

from . import explaining, ops
from .explaining import Explanation
from .hosting import FusedVideoModel, round_up
from .vivit import ClassifierOutput
from .weights import timesformer_param_shapes


class TimesformerConfig:
    """Minimal stand-in for transformers.TimesformerConfig (the fields the path and the
    reference's checkpoint dict use; the factory sets num_classes / video_size too,
    timesformer_model.py:27-31)."""

    defaults = dict(image_size=224, patch_size=16, num_channels=3, num_frames=8, hidden_size=768,
                    num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, hidden_act="gelu",
                    hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, initializer_range=0.02,
                    layer_norm_eps=1e-6, qkv_bias=True, attention_type="divided_space_time", drop_path_rate=0.0,
                    model_type="timesformer")

    def __init__(self, **kw):
        d = dict(self.defaults)
        d.update(kw)
        id2label = d.pop("id2label", None) or {0: "LABEL_0", 1: "LABEL_1"}
        self.id2label = {int(k): v for k, v in id2label.items()}
        self.label2id = d.pop("label2id", None) or {v: k for k, v in self.id2label.items()}
        d.pop("num_labels", None)
        self.num_classes = d.pop("num_classes", len(self.id2label))
        self.video_size = d.pop("video_size", [d["num_frames"], d["image_size"], d["image_size"]])
        for k, v in d.items():
            setattr(self, k, v)

    @property
    def num_labels(self):
        return len(self.id2label)

    def to_dict(self):
        d = {k: getattr(self, k) for k in self.defaults}
        d["id2label"] = {str(k): v for k, v in self.id2label.items()}
        d["label2id"] = dict(self.label2id)
        d["num_classes"] = self.num_classes
        d["video_size"] = list(self.video_size)
        return d

    @classmethod
    def from_dict(cls, d):
        return cls(**d)

    def as_shape_cfg(self):
        return dict(hidden_size=self.hidden_size, intermediate_size=self.intermediate_size, patch_size=self.patch_size,
                    num_channels=self.num_channels, num_frames=self.num_frames, image_size=self.image_size,
                    num_hidden_layers=self.num_hidden_layers, num_labels=self.num_labels)

    def __repr__(self):
        return f"TimesformerConfig({json.dumps(self.to_dict())})"


class TimesformerForVideoClassification(FusedVideoModel):
    """fp32 master parameters in HF naming (state_dict compatible with transformers'
    `TimesformerForVideoClassification`), bf16/fp32 packed device copies for the kernels."""

    def __init__(self, config: TimesformerConfig):
        c = config
        if c.hidden_size // c.num_attention_heads != 64:
            raise ValueError("libvclip attention supports head_dim 64 only")
        if c.attention_type != "divided_space_time":
            raise ValueError("only attention_type='divided_space_time' (the reference's K400 checkpoint) is built")
        super().__init__(timesformer_param_shapes(c.as_shape_cfg()), c.num_labels)
        self.config = config
        # kernel_events: a list collects HIP events around each spatial-attention launch (bench.py)
        # tile config of the two 768 x 768 bf16-output projections per layer (temporal dense, spatial
        # output): the 128x128 kernel (cfg 5), not vc_gemm's pick (the persistent 256x256 kernel,
        # 297 tiles = 1.16 rounds of 256 CUs at B=16): 37.9 vs 46.9 us at M = 25344 and 24.7 vs 25.4
        # at the two-stream M = 12800 (tools/ab_gemm_cfg.py, round 3); None: vc_gemm's pick
        self.proj_cfg = 5
        # per-GEMM tile config overrides {"qkv_temporal" | "qkv_spatial" | "fc1" | "fc2": cfg} (A/B hook)
        self.gemm_cfg = {}

    def _pack(self, device):
        pk = self._cached_pack(device)
        if pk is not None:
            return pk
        c = self.config
        bf, f32 = torch.bfloat16, torch.float32
        P = lambda n: self.P(n).detach().to(device=device, dtype=f32)  # noqa: E731
        D, T = c.hidden_size, c.num_frames
        e = "timesformer.embeddings."
        pk = {"device": device, "version": self._weights_version()}
        pk["w_emb"] = P(e + "patch_embeddings.projection.weight").reshape(D, -1).to(bf).contiguous()
        pk["b_emb"] = P(e + "patch_embeddings.projection.bias").contiguous()
        pos = P(e + "position_embeddings").reshape(-1, D)
        tim = P(e + "time_embeddings").reshape(-1, D)
        # EMBED epilogue table: row p*T + t = pos[1 + p] + time[t] (patch-major, time-minor)
        pk["pos_time"] = (pos[1:, None, :] + tim[None, :T, :]).reshape(-1, D).contiguous()
        pk["pos"] = pos.contiguous()
        pk["cls"] = P(e + "cls_token").reshape(D).contiguous()
        qs = (D // c.num_attention_heads) ** -0.5 * ops.LOG2E  # softmax scale * log2(e) folded into q

        def qkv(prefix):
            w = P(prefix + "attention.qkv.weight").clone()
            b = P(prefix + "attention.qkv.bias").clone()
            w[:D] *= qs
            b[:D] *= qs
            return w.to(bf).contiguous(), b.contiguous()

        layers = []
        for i in range(c.num_hidden_layers):
            p = f"timesformer.encoder.layer.{i}."
            L = {}
            for ln, key in (("temporal_layernorm", "lnt"), ("layernorm_before", "ln1"), ("layernorm_after", "ln2")):
                L[key + "_g"] = P(p + ln + ".weight").contiguous()
                L[key + "_b"] = P(p + ln + ".bias").contiguous()
            L["w_qkv_t"], L["b_qkv_t"] = qkv(p + "temporal_attention.")
            wto, bto = P(p + "temporal_attention.output.dense.weight"), P(p + "temporal_attention.output.dense.bias")
            wtd, btd = P(p + "temporal_dense.weight"), P(p + "temporal_dense.bias")
            L["w_t"] = (wtd.double() @ wto.double()).to(bf).contiguous()
            L["b_t"] = (wtd.double() @ bto.double() + btd.double()).to(f32).contiguous()
            L["w_qkv_s"], L["b_qkv_s"] = qkv(p + "attention.")
            L["w_o"] = P(p + "attention.output.dense.weight").to(bf).contiguous()
            L["b_o"] = P(p + "attention.output.dense.bias").contiguous()
            L["w_1"] = P(p + "intermediate.dense.weight").to(bf).contiguous()
            L["b_1"] = P(p + "intermediate.dense.bias").contiguous()
            L["w_2"] = P(p + "output.dense.weight").to(bf).contiguous()
            L["b_2"] = P(p + "output.dense.bias").contiguous()
            layers.append(L)
        pk["layers"] = layers
        pk["lnf_g"] = P("timesformer.layernorm.weight").contiguous()
        pk["lnf_b"] = P("timesformer.layernorm.bias").contiguous()
        pk["w_cls"] = P("classifier.weight").contiguous()
        pk["b_cls"] = P("classifier.bias").contiguous()
        self._packed = pk
        return pk

    def geometry(self, B):
        c = self.config
        P = (c.image_size // c.patch_size) ** 2
        T = c.num_frames
        S = 1 + P * T
        Mpad = round_up(max(B * S, B * T * (1 + P)) + 128, 256)
        Memb = round_up(B * P * T, 128)
        return P, T, S, Mpad, Memb

    def _workspace(self, B, device, part: int = 0):
        return self._cached_workspace((B, str(device), part), lambda: self._make_workspace(B, device), 8)

    def _make_workspace(self, B, device):
        c = self.config
        D, I = c.hidden_size, c.intermediate_size
        P, T, S, Mpad, Memb = self.geometry(B)
        bf = torch.bfloat16
        z = lambda *s, dt=bf: torch.zeros(s, dtype=dt, device=device)  # noqa: E731
        ws = dict(A_emb=z(Memb, c.num_channels * c.patch_size * c.patch_size), X=z(Mpad, D, dt=torch.float32),
                  Hc=z(Mpad, D), Hf=z(Mpad, D), QKV=z(Mpad, 3 * D), O=z(Mpad, D), Yb=z(Mpad, D), Hd=z(Mpad, I),
                  logits=z(B, c.num_labels, dt=torch.float32))
        return ws

    def forward(self, pixel_values: torch.Tensor = None, labels: torch.Tensor = None, **kw):
        """HF call convention.  In training mode with autograd enabled (the reference's train loop,
        timesformer/timesformer_classifier/trainers/trainer.py:165-174) the logits carry the graph of
        the HIP train step (_forward_train); otherwise the fused inference path runs."""
        if pixel_values is None:
            raise ValueError("pixel_values required")
        if pixel_values.device.type != "cuda":
            raise RuntimeError("TimesformerForVideoClassification (vclip_amd) runs on the GPU only")
        x = pixel_values.contiguous().float() if pixel_values.dtype != torch.float32 else pixel_values.contiguous()
        if self.training and torch.is_grad_enabled():
            logits = self._forward_train(x)
        else:
            with torch.no_grad():
                logits = self.forward_logits(x)
        loss = None
        if labels is not None:
            loss = torch.nn.functional.cross_entropy(logits, labels.to(logits.device))
        return ClassifierOutput(logits, loss)

    def _check_input(self, pix):
        c = self.config
        B, T, C, H, W = pix.shape
        if T != c.num_frames or H != c.image_size or W != c.image_size or C != c.num_channels:
            raise ValueError(f"pixel_values {tuple(pix.shape)} do not match config "
                             f"(T={c.num_frames}, C={c.num_channels}, {c.image_size}^2)")

    def _graph_knobs(self):
        return (self.proj_cfg, tuple(sorted(self.gemm_cfg.items())))

    def _forward_part(self, pix: torch.Tensor, part: int, out=None, keep=None) -> torch.Tensor:
        """keep (explain only): {"QKV_t": [L, Mpad, 3D], "QKV_s": [L, Mpad, 3D], "LSE_s": [L, B*T*H*(1+P)]} -- layer
        i's temporal and spatial q|k|v go to keep["QKV_t"][i] / keep["QKV_s"][i] instead of the shared buffer and
        its spatial attention is ops.attention_fwd_lse, which stores the base-2 log-sum-exp in keep["LSE_s"][i]."""
        c = self.config
        B = pix.shape[0]
        pk = self._pack(pix.device)
        ws = self._workspace(B, pix.device, part)
        P, T, S, Mpad, Memb = self.geometry(B)
        Hn = c.num_attention_heads
        eps = c.layer_norm_eps
        X, Hc, Hf, QKV, O, Yb, Hd = (ws[k] for k in ("X", "Hc", "Hf", "QKV", "O", "Yb", "Hd"))
        pc = c.patch_size
        D, I = c.hidden_size, c.intermediate_size
        Kemb = c.num_channels * pc * pc
        tm = ops.timed
        # algorithmic work per launch for an installed ops.OpRecorder: clip rows B*S (temporal
        # branch and MLP), frame rows B*T*(1+P) (spatial branch), no padding
        Mc, Mf = B * S, B * T * (1 + P)
        tm("im2col_kernel", "im2col", B * T * (c.num_channels * c.image_size ** 2 * 4 + P * Kemb * 2), "byte",
           ops.tubelet_im2col, pix, (1, pc, pc), ws["A_emb"], order="patch_major")
        ops.gemm(ws["A_emb"], pk["w_emb"], pk["b_emb"], "embed_f32", X, aux=pk["pos_time"], group=P * T,
                 group_stride=S, group_offset=1, m=Memb, flop=2.0 * B * P * T * D * Kemb, op="embed")
        ops.cls_init(pk["cls"], pk["pos"], X, B, S)
        act = "bias_gelu_erf" if c.hidden_act == "gelu" else "bias_gelu_tanh"
        scale = 1.0 / math.sqrt(c.hidden_size // Hn)
        pcfg = -1 if self.proj_cfg is None else self.proj_cfg
        gc = self.gemm_cfg
        for li, L in enumerate(pk["layers"]):
            # temporal branch (clip layout)
            if keep is not None:
                QKV = keep["QKV_t"][li]
            tm("layernorm_kernel", "layernorm", Mc * D * 6, "byte", ops.layernorm, X, L["lnt_g"], L["lnt_b"], eps, Hc,
               m=B * S)
            ops.gemm(Hc, L["w_qkv_t"], L["b_qkv_t"], "bias", QKV, cfg=gc.get("qkv_temporal", -1), flop=2.0 * Mc * 3 * D * D, op="qkv_temporal")
            tm("temporal_attn_lds_kernel", "temporal_attention", 4.0 * T * T * 64 * Hn * B * P, "flop",
               ops.temporal_attention, QKV, B, P, T, Hn, scale, O, q_prescaled=True)
            ops.gemm(O, L["w_t"], L["b_t"], "bias", Yb, cfg=pcfg, flop=2.0 * Mc * D * D, op="proj_temporal")
            # spatial branch (frame layout): X += temporal output, LayerNorm in the frame layout
            tm("tsf_add_ln_kernel", "add_layernorm", Mc * D * (4 + 2 + 4) + Mf * D * 2, "byte",
               ops.divided_add_layernorm, X, Yb, B, P, T, L["ln1_g"], L["ln1_b"], eps, "temporal_to_spatial", Hf)
            if keep is not None:
                QKV = keep["QKV_s"][li]
            ops.gemm(Hf, L["w_qkv_s"], L["b_qkv_s"], "bias", QKV, cfg=gc.get("qkv_spatial", -1), flop=2.0 * Mf * 3 * D * D, op="qkv_spatial")
            ev = self.kernel_events
            if ev is not None:  # recorded on the current stream, the one the kernel runs on
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            if keep is not None:
                ops.attention_fwd_lse(QKV, B * T, 1 + P, Hn, O, keep["LSE_s"][li], scale=scale, q_prescaled=True)
            else:
                tm("attn_short_d64_kernel", "spatial_attention", 4.0 * (1 + P) * (1 + P) * 64 * Hn * B * T, "flop",
                   ops.attention, QKV, B * T, 1 + P, Hn, scale, O, q_prescaled=True)
            if ev is not None:
                e1.record()
                # flop, algorithmic bytes (q, k, v read and the output written once: 4 x 64 x 2 B
                # per token-head)
                ev.append((e0, e1, 4.0 * (1 + P) * (1 + P) * 64 * Hn * B * T, 512.0 * (1 + P) * Hn * B * T))
            ops.gemm(O, L["w_o"], L["b_o"], "bias", Yb, cfg=pcfg, flop=2.0 * Mf * D * D, op="o_proj")
            # MLP (clip layout)
            tm("tsf_add_ln_kernel", "add_layernorm", Mf * D * 2 + Mc * D * (4 + 4 + 2), "byte",
               ops.divided_add_layernorm, X, Yb, B, P, T, L["ln2_g"], L["ln2_b"], eps, "spatial_to_mlp", Hc)
            ops.gemm(Hc, L["w_1"], L["b_1"], act, Hd, cfg=gc.get("fc1", -1), flop=2.0 * Mc * I * D, op="fc1")
            ops.gemm(Hd, L["w_2"], L["b_2"], "bias_resid_f32", X, cfg=gc.get("fc2", -1), flop=2.0 * Mc * D * I, op="fc2")
        return ops.cls_head(X, B, S, pk["lnf_g"], pk["lnf_b"], eps, pk["w_cls"], pk["b_cls"],
                            out=ws["logits"] if out is None else out)

    # ---- explain ------------------------------------------------------------------
    EXPLAIN_METHODS = ("rollout", "cls_attention")

    def _explain_buffers(self, B, device):
        def build():
            c = self.config
            P, T, S, Mpad, _ = self.geometry(B)
            Hn, nl = c.num_attention_heads, c.num_hidden_layers
            seed = torch.zeros(B * T, 1 + P, dtype=torch.float32)
            seed[:, 0] = 1.0 / T  # e_CLS in the frame layout, made on the host: every frame's slot 0 holds r_CLS / T
            f = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)  # noqa: E731
            q = lambda: torch.zeros(nl, Mpad, 3 * c.hidden_size, dtype=torch.bfloat16, device=device)  # noqa: E731
            return dict(QKV_t=q(), QKV_s=q(), LSE_s=f(nl, B * T * Hn * (1 + P)), seed=seed.to(device),
                        r_frame=(f(B * T, 1 + P), f(B * T, 1 + P)), r_clip=f(B, S),
                        work=ops.attention_rollout_work(B * T, 1 + P, Hn, device))

        return self._cached_explain(self._explain_ws, (B, str(device)), build)

    @torch.no_grad()
    def explain(self, pixel_values: torch.Tensor, method: str = "rollout", residual: float = 0.5):
        """The logits and which tokens produced them: attention rollout (Abnar & Zuidema 2020) of the CLS row
        through divided space-time attention.  Returns vivit.Explanation: `logits` f32 [B, labels] on the device;
        on the host `token_relevance` f32 [B, S] in the clip layout (column 0 is CLS, token (p, t) at 1 + p*T + t),
        `saliency` f32 [B, T, H/ps, W/ps] (the patch relevances divided by their per-clip sum, token (p, t) at
        [t, p // gw, p % gw]) and `temporal` f32 [B, T] (saliency summed over space).

        A layer mixes tokens as x <- A_s A_t x (the MLP mixes none), with a = `residual`:
          temporal  A_t = a * mean_h(A_t[p]) + (1 - a) * I on the T x T block of every patch; the CLS row is the
                    identity (the temporal branch never updates CLS);
          spatial   A_s, frame t over [CLS, (0, t) .. (P-1, t)]: a patch row is (1 - a) * e_(p,t) + a * its head-mean
                    attention row; the CLS row is (1 - a) * e_CLS + a * the mean over the T frames of the per-frame
                    CLS rows (the model averages the per-frame CLS outputs).
        method "rollout": r = e_CLS, then for layers L .. 1  r <- (r A_s) A_t.  In the frame layout ([B*T, 1 + P],
        every frame's slot 0 holding r_CLS / T) the spatial step is ops.attention_rollout_step with B' = B*T and
        S' = 1 + P; ops.temporal_rollout_step is the temporal step, gathers to the clip layout and spreads the
        result for the next layer: three launches per layer, and no attention matrix exists at any time.
        "cls_attention": the spatial step of the last layer alone with a = 1, i.e. CLS (1/T) sum_t A_s^t[0, 0] and
        patch (p, t) A_s^t[0, 1 + p] / T.

        Runs the ordinary eager forward (no graph replay, no stream split) with the lse-storing spatial attention
        kernel and keeps every layer's temporal and spatial q|k|v [L, Mpad, 3D] bf16 and the spatial lse in buffers of
        its own, cached per (B, device): 198 MB at TimeSformer-B 8 x 224^2, B = 1.  The forward's workspaces, graphs
        and logits are untouched.  The result is copied to the host once; normalisation and the sums happen there.
        Refuses (no fallback): training mode, CPU tensors, an unknown method (the class-specific "grad_rollout" is
        ViViT's only), residual outside (0, 1], shapes that do not match the config, B*T*heads > 65535."""
        c = self.config
        explaining.require_method(method, self.EXPLAIN_METHODS)
        explaining.require_residual(residual)
        explaining.require_explainable(self, pixel_values, what="pixel_values")
        if pixel_values.dim() != 5:
            raise ValueError(f"pixel_values {tuple(pixel_values.shape)} must be [B, T, C, H, W]")
        B, T, C, H, W = pixel_values.shape
        if T != c.num_frames or H != c.image_size or W != c.image_size or C != c.num_channels:
            raise ValueError(f"pixel_values {tuple(pixel_values.shape)} do not match config "
                             f"(T={c.num_frames}, C={c.num_channels}, {c.image_size}^2)")
        Hn, nl = c.num_attention_heads, c.num_hidden_layers
        if B * T * Hn > 65535:  # the spatial step runs one grid row per (frame, head)
            raise ValueError(f"explain: B * T * heads = {B * T * Hn} exceeds the rollout step's grid limit of 65535: "
                             f"at most B = {65535 // (T * Hn)} clips per call")
        pix = pixel_values.contiguous()
        if pix.dtype != torch.float32:
            pix = pix.float()
        P = self.geometry(B)[0]
        buf = self._explain_buffers(B, pix.device)
        logits = self._forward_part(pix, 0, keep=buf).clone()
        fa, fb = buf["r_frame"]
        if method == "rollout":
            r_f, alpha = buf["seed"], float(residual)
            for li in reversed(range(nl)):
                ops.attention_rollout_step(buf["QKV_s"][li], buf["LSE_s"][li], r_f, B * T, 1 + P, Hn, alpha, buf["work"], fa)
                ops.temporal_rollout_step(buf["QKV_t"][li], fa, B, P, T, Hn, alpha, buf["r_clip"], fb if li else None)
                r_f = fb
            rel = buf["r_clip"].cpu()  # the one copy; the rest is host bookkeeping on [B, S]
        else:
            ops.attention_rollout_step(buf["QKV_s"][nl - 1], buf["LSE_s"][nl - 1], buf["seed"], B * T, 1 + P, Hn, 1.0,
                                       buf["work"], fa)
            r_f = fa.cpu().reshape(B, T, 1 + P)  # the one copy; gathered to the clip layout on the host
            rel = torch.cat([r_f[:, :, 0].sum(dim=1, keepdim=True),
                             r_f[:, :, 1:].transpose(1, 2).reshape(B, P * T)], dim=1).contiguous()
        g = c.image_size // c.patch_size
        patch = rel[:, 1:].double().reshape(B, P, T).transpose(1, 2)  # token (p, t) -> [t, p]
        sal = explaining.normalise(patch, zero_ok=False).reshape(B, T, g, g).contiguous()
        return Explanation(logits, rel, sal, sal.sum(dim=(2, 3)), method)

    def _forward_train(self, pix: torch.Tensor) -> torch.Tensor:
        """The TimeSformer forward (TF5/models/timesformer/modeling_timesformer.py:67-145, 332-398,
        oracle/timesformer_ref.py) as autograd ops over the HIP kernels (vclip_amd/autograd_ops.py):
        bf16 MFMA GEMMs with fp32 accumulation on the fp32 master weights, fp32 residual stream,
        exact GELU, flash spatial attention, VALU temporal attention; layout glue in torch."""
        from . import autograd_ops as A
        c = self.config
        B, T, C, H, W = pix.shape
        if T != c.num_frames or H != c.image_size or W != c.image_size or C != c.num_channels:
            raise ValueError(f"pixel_values {tuple(pix.shape)} do not match config")
        if c.hidden_act != "gelu":
            raise NotImplementedError("train step: hidden_act 'gelu' (TimeSformer's) only")
        D, Hn, eps, pc = c.hidden_size, c.num_attention_heads, c.layer_norm_eps, c.patch_size
        P = (c.image_size // pc) ** 2
        S = 1 + P * T
        e = "timesformer.embeddings."
        M = B * P * T
        a_emb = torch.zeros(round_up(M, 128), C * pc * pc, dtype=torch.bfloat16, device=pix.device)
        ops.tubelet_im2col(pix, (1, pc, pc), a_emb, order="patch_major")  # rows (b, p, t)
        emb = A.linear(a_emb[:M], self.P(e + "patch_embeddings.projection.weight").reshape(D, -1),
                       self.P(e + "patch_embeddings.projection.bias"), out_f32=True)
        pos = self.P(e + "position_embeddings").reshape(-1, D)
        tim = self.P(e + "time_embeddings").reshape(-1, D)[:T]
        emb = emb.reshape(B, P, T, D) + pos[1:].reshape(1, P, 1, D) + tim.reshape(1, 1, T, D)
        cls = (self.P(e + "cls_token").reshape(1, 1, D) + pos[0].reshape(1, 1, D)).expand(B, 1, D)
        x = torch.cat([cls, emb.reshape(B, P * T, D)], 1)  # [B, S, D] patch-major, time-minor
        qs = (D // Hn) ** -0.5 * ops.LOG2E
        for i in range(c.num_hidden_layers):
            p = f"timesformer.encoder.layer.{i}."
            W_ = lambda n: self.P(p + n)  # noqa: E731
            # temporal branch on the clip layout (CLS rows computed and discarded, as inference)
            h = A.layer_norm(x.reshape(B * S, D), W_("temporal_layernorm.weight"), W_("temporal_layernorm.bias"), eps)
            qkv = A.linear(h, W_("temporal_attention.attention.qkv.weight"), W_("temporal_attention.attention.qkv.bias"),
                           qrows=D, qscale=qs)
            o = A.temporal_attention(qkv, B, P, T, Hn)
            a = A.linear(o, W_("temporal_attention.output.dense.weight"), W_("temporal_attention.output.dense.bias"))
            rt = A.linear(a, W_("temporal_dense.weight"), W_("temporal_dense.bias"), out_f32=True).reshape(B, S, D)
            te = x[:, 1:] + rt[:, 1:]
            # spatial branch: B*T sequences of CLS + P patches
            init_cls = x[:, :1]
            sp = te.reshape(B, P, T, D).permute(0, 2, 1, 3).reshape(B * T, P, D)
            sp = torch.cat([init_cls.expand(B, T, D).reshape(B * T, 1, D), sp], 1)
            h = A.layer_norm(sp.reshape(B * T * (1 + P), D), W_("layernorm_before.weight"), W_("layernorm_before.bias"),
                             eps)
            qkv = A.linear(h, W_("attention.attention.qkv.weight"), W_("attention.attention.qkv.bias"), qrows=D,
                           qscale=qs)
            o = A.attention(qkv, B * T, 1 + P, Hn)
            y = A.linear(o, W_("attention.output.dense.weight"), W_("attention.output.dense.bias"),
                         out_f32=True).reshape(B * T, 1 + P, D)
            cls_res = y[:, 0].reshape(B, T, D).mean(1, keepdim=True)
            res = y[:, 1:].reshape(B, T, P, D).permute(0, 2, 1, 3).reshape(B, P * T, D)
            x = torch.cat([init_cls + cls_res, te + res], 1)
            # MLP
            h = A.layer_norm(x.reshape(B * S, D), W_("layernorm_after.weight"), W_("layernorm_after.bias"), eps)
            g = A.gelu_erf(A.linear(h, W_("intermediate.dense.weight"), W_("intermediate.dense.bias")))
            x = x + A.linear(g, W_("output.dense.weight"), W_("output.dense.bias"), out_f32=True).reshape(B, S, D)
        return A.cls_head(x.reshape(B * S, D), self.P("timesformer.layernorm.weight"),
                          self.P("timesformer.layernorm.bias"), self.P("classifier.weight"), self.P("classifier.bias"),
                          B, S, eps)


def create_model(model_name="facebook/timesformer-base-finetuned-k400", num_classes=2, class_labels=None,
                 num_frames=8, device="cuda", logger=None, weights_seed: int = 0):
    """Drop-in for timesformer/timesformer_classifier/models/timesformer_model.py:4-53.

    The reference loads `TimesformerConfig.from_pretrained(model_name)` + K400 weights
    (`ignore_mismatched_sizes=True` re-initialises the head, and the time embeddings when
    num_frames != 8).  No network here: the TimeSformer-B architecture is built with seeded
    synthetic weights (vclip_amd.weights) unless a checkpoint is loaded afterwards.
    """
    class_labels = class_labels or ["non-referral", "referral"]
    id2label = {i: l for i, l in enumerate(class_labels)}
    cfg = TimesformerConfig(num_frames=num_frames, id2label=id2label, label2id={l: i for i, l in id2label.items()},
                            num_classes=num_classes, video_size=[num_frames, 224, 224])
    if logger:
        logger.info(f"Creating TimeSformer model based on {model_name} (num_frames={num_frames}) on {device}")
    model = TimesformerForVideoClassification(cfg)
    from .weights import make_timesformer_weights
    model.load_state_dict(make_timesformer_weights(cfg.as_shape_cfg(), seed=weights_seed))
    return model.to(device) if device else model
