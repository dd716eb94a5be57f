"""ViViT-B/16x2 video classifier on the libvclip.so kernels — drop-in for the reference's
`create_model` (vivit_transformer/vivit_classifier/models/vivit_model.py:4-52), which
returns an HF `VivitForVideoClassification` called as `model(pixel_values=...)` and
read through `.logits` (vivit_transformer/vivit_classifier/trainers/trainer.py:141-142,
vivit_transformer/inference.py:192-193).

Device data layout (one forward of B clips, S = 1 + (T/2)(H/16)(W/16) tokens):
  rows r = b*S + s, padded to Mpad = roundup(B*S + 128, 256) so every GEMM runs on
  whole 128-row tiles and attention can read a full 64-key tile past each clip's end;
  residual stream X   f32  [Mpad, D]          (fp32 residual adds, as the fp32 reference)
  LN output Y         bf16 [Mpad, D]
  fused q|k|v         bf16 [Mpad, 3D]
  attention out O     bf16 [Mpad, D]
  MLP hidden          bf16 [Mpad, 4D]
Weights are packed once per device: bf16 [N, K] (nn.Linear layout), q|k|v concatenated,
fp32 biases / LayerNorm / position table / classifier.
"""
from __future__ import annotations

import functools
import json
import math
from collections import OrderedDict

import torch

from . import explaining, ops
from .explaining import Explanation
from .hosting import FusedVideoModel, round_up
from .vivit_explain import GradRolloutEngine
from .vivit_train import FlatLayout, TrainEngine, VivitTrainFn
from .weights import vivit_param_shapes


class VivitConfig:
    """Minimal stand-in for transformers.VivitConfig (fields the path and the reference's
    checkpoint dict use: trainer.py:281-299 saves config.to_dict(), id2label, label2id)."""

    defaults = dict(image_size=224, num_frames=32, tubelet_size=[2, 16, 16], num_channels=3, hidden_size=768,
                    num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, hidden_act="gelu_fast",
                    hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, initializer_range=0.02,
                    layer_norm_eps=1e-6, qkv_bias=True, model_type="vivit")

    def __init__(self, **kw):
        d = dict(self.defaults)
        d.update(kw)
        id2label = d.pop("id2label", None) or {0: "LABEL_0", 1: "LABEL_1"}
        self.id2label = {int(k): v for k, v in id2label.items()}
        self.label2id = d.pop("label2id", None) or {v: k for k, v in self.id2label.items()}
        d.pop("num_labels", None)
        for k, v in d.items():
            setattr(self, k, v)
        self.tubelet_size = list(self.tubelet_size)

    @property
    def num_labels(self):
        return len(self.id2label)

    def to_dict(self):
        d = {k: getattr(self, k) for k in self.defaults}
        d["id2label"] = {str(k): v for k, v in self.id2label.items()}
        d["label2id"] = dict(self.label2id)
        return d

    @classmethod
    def from_dict(cls, d):
        return cls(**d)

    def as_shape_cfg(self):
        return dict(hidden_size=self.hidden_size, intermediate_size=self.intermediate_size,
                    tubelet_size=self.tubelet_size, num_channels=self.num_channels, num_frames=self.num_frames,
                    image_size=self.image_size, num_hidden_layers=self.num_hidden_layers,
                    num_labels=self.num_labels)

    def __repr__(self):
        return f"VivitConfig({json.dumps(self.to_dict())})"


class ClassifierOutput:
    """Mimics the `.logits` / `.loss` access of transformers' ImageClassifierOutput."""

    def __init__(self, logits, loss=None):
        self.logits = logits
        self.loss = loss

    def __getitem__(self, i):
        return (self.loss, self.logits)[i] if self.loss is not None else (self.logits,)[i]


# Clips per stream part where an uneven split measured faster than the even one (model.split_sizes
# overrides).  ViViT-B B = 8 on two streams: 5 + 3 vs 4 + 4, +2.2 / +1.8 % in two interleaved
# A/Bs on different boxes (tools/ab_split_sizes.py, profiles/r05_split_sizes.txt; 3 + 5 -0.8 %,
# 6 + 2 -0.9 %): the 5-clip part's 1500 attention workgroups fill 2.93 rounds of the 512
# two-per-CU slots where 4 clips' 1200 fill 2.34, and the parts pad 25344 token rows to the
# 256-row GEMM tiles instead of 25600.  The larger part goes first (its stream starts first).
# TimeSformer-B (10 + 6, 9 + 7) and ResNet3D (3 + 1) measured slower than even.
SPLIT_DEFAULT = {(8, 2): (5, 3)}


class VivitForVideoClassification(FusedVideoModel):
    """fp32 master parameters in HF naming (state_dict compatible with transformers-5
    `VivitForVideoClassification`), bf16/fp32 packed device copies for the kernels."""

    def __init__(self, config: VivitConfig):
        c = config
        if c.hidden_size // c.num_attention_heads != 64:
            raise ValueError("libvclip attention supports head_dim 64 only")
        shapes = vivit_param_shapes(c.as_shape_cfg())
        super().__init__(shapes, c.num_labels)
        self.config = config
        self._layout = FlatLayout(c, shapes)
        self._flat = None      # fp32 masters, one device buffer (params are views), built for training
        self._gflat = None     # gradients, same layout (p.grad are views)
        self._gscratch = None  # backward target when gradients accumulate across calls
        self._engine = None
        self._lora = None      # vclip_amd.lora.LoraState while adapters are attached (lora.attach)
        self.grad_ready_hooks = []  # fn(stage, start, end, gflat): a slice of gflat is final (enqueued)
        self._explain_grad = {}  # explain(method="grad_rollout")'s engine per (B, device) (vivit_explain.py)
        # per-GEMM tile config override {"qkv" | "o_proj" | "fc1" | "fc2": vc_gemm cfg} (None / absent:
        # vc_gemm's own pick) and the GEMM / LayerNorm row count: "pad" = every padded row (Mpad),
        # "tight" = B*S rounded up to the tile height (the padding rows keep their initial zeros)
        self.gemm_cfg = {}
        self.rows = "pad"
        # 16-bit operand type of the inference forward: bf16 (the benchmarked configuration) or
        # torch.float16 (same kernels and MFMA rate, logits ~6x closer to the fp32 reference;
        # DESIGN.md §5.5).  The train step (vivit_train.py) is bf16 either way.
        self.compute_dtype = torch.bfloat16
        # fp16 build only: the patch embedding and the first `precise_layers` layers' GEMMs take split
        # operands -- weights as fp16 high + low parts (and the pixels too in the embedding) through
        # vc_gemm_h16_wrap, A.W_hi + A.W_lo in one fp32 chain.  The fp16 build's logit error is set by
        # the weight rounding of the first layers (tests/analysis/w_probe.py: all weights fp32 3.8e-4, the
        # embedding + layer 0 4.3e-4, vs 1.25e-3 all fp16 on the bench's 8 clips).
        self.precise_layers = 0
        # ... and which GEMMs: "embed" (pixels and weights split: three products) or "embed_w" (weights
        # only: A.W_hi + A.W_lo), and layer 0's "qkv" / "o_proj" / "fc1" / "fc2".  Default: the
        # embedding's weights and layer 0's q|k|v -- logit error 6.3e-4 on 4 of the bench's clips vs 6.7e-4
        # with the pixels and all of layer 0 split too, at less than half the extra MFMA work (957 vs 926
        # clips/s, bf16 982: tests/test_fp16_gpu.py, profiles/r05_fp16_clock.json)
        self.precise_ops = ("embed_w", "qkv")
        # inference only: the last layer's attention, o_proj, LN2, fc1 and fc2 run for the CLS rows alone
        # (csrc/cls_tail.hip) -- the logits read nothing else of that layer, whose patch tokens are keys and
        # values only.  False: the full layer (as training, and as a last layer with split operands, always do)
        self.cls_only_last_layer = True

    # ---- state dict in HF naming ---------------------------------------------------
    def hf_state_dict(self):
        return OrderedDict((n, self.params[n.replace(".", "__")]) for n in self._names)

    def _clean_state_dict(self, sd):
        from .checkpoint import convert_state_dict
        return convert_state_dict(sd)

    def _apply(self, fn, *args, **kwargs):  # .to() / .cuda(): parameters move one by one
        out = super()._apply(fn, *args, **kwargs)
        self._flat = self._gflat = self._gscratch = self._engine = None
        if self._lora is not None:
            self._lora.reset()
        self._explain_grad = {}
        self._drop_device_state()
        return out

    # ---- training (vclip_amd/vivit_train.py) --------------------------
    def _ensure_flat(self, device):
        """Move the fp32 masters into one flat device buffer, parameters becoming views of it
        (the same Parameter objects, so an optimizer built earlier keeps working)."""
        if self._flat is not None and self._flat.device == device:
            return
        flat = torch.zeros(self._layout.total, dtype=torch.float32, device=device)
        with torch.no_grad():
            for n in self._names:
                v = self._layout.view(flat, n)
                v.copy_(self.P(n).detach().reshape(v.shape))
                self.P(n).data = v
                # the optimizer's one-launch path needs to know that a parameter list covers the
                # whole layout (its alignment gaps stay zero in both buffers: AdamW keeps them 0)
                self.P(n)._vc_flat_layout = (self._layout.total, len(self._names))
        self._flat = flat
        # LoRA mode never writes a full-size gradient: the buffer is made by the first full backward
        self._gflat = None if self._lora is not None else torch.zeros_like(flat)
        self._gscratch = None
        self._engine = None

    def _train_engine(self, B, device):
        self._ensure_flat(device)
        if self._lora is not None:
            self._lora.ensure_flat(self, device)
        if self._engine is None or self._engine.B != B or self._engine.device != device:
            self._engine = None
            self._engine = TrainEngine(self, B, device)
        return self._engine

    def _run_backward(self, eng, dlogits):
        if self._lora is not None:
            from . import lora
            return lora.run_backward(self, eng, dlogits)
        params = self._param_list()
        if self._gflat is None:  # flattened while adapters were attached (lora.merge since)
            self._gflat = torch.zeros_like(self._flat)
        accumulate = any(p.grad is not None for p in params)
        if not accumulate:
            target = self._gflat
        else:
            if self._gscratch is None:
                self._gscratch = torch.zeros_like(self._gflat)
            target = self._gscratch

        stages = []

        def ready(stage, start, end):
            if not accumulate:
                for h in self.grad_ready_hooks:
                    h(stage, start, end, target)
            else:
                stages.append((stage, start, end))

        if accumulate and self.grad_ready_hooks:
            g0 = self._gflat.untyped_storage().data_ptr()
            if any(p.grad is not None and p.grad.untyped_storage().data_ptr() != g0 for p in params):
                raise RuntimeError("gradient accumulation with grad_ready_hooks (data-parallel all-reduce) needs "
                                   "every .grad to be the model's own flat-buffer view; zero_grad(set_to_none=True) "
                                   "or leave .grad as the backward set it")
        eng.backward(dlogits, target, ready)
        lay = self._layout
        if not accumulate:
            for n, p in zip(self._names, params):
                p.grad = lay.view(self._gflat, n)
            return
        for n, p in zip(self._names, params):
            g = lay.view(target, n)
            if p.grad is None:
                p.grad = lay.view(self._gflat, n).copy_(g)
            else:
                p.grad.add_(g)
        # accumulated gradients: the hooks (e.g. GradAllReduce) see the summed flat buffer, stage
        # by stage in backward order once the sum is complete -- as DDP reduces the accumulated
        # .grad on every backward (the average of (mean + local) is mean + mean)
        for stage, start, end in stages:
            for h in self.grad_ready_hooks:
                h(stage, start, end, self._gflat)

    def _weights_version(self):
        ver = super()._weights_version()
        if self._lora is not None:  # the adapters are part of the weights the packs are made from
            ver += (id(self._lora), sum(p._version for p in self._lora.params(self)))
        return ver

    # ---- device packing ----------------------------------------------------------
    def _pack(self, device):
        bf = self.compute_dtype
        if bf not in (torch.bfloat16, torch.float16):
            raise ValueError(f"compute_dtype must be torch.bfloat16 or torch.float16, not {bf}")
        npre = self.precise_layers if bf == torch.float16 else 0
        pops = tuple(sorted(self.precise_ops)) if npre > 0 else ()
        if not set(pops) <= {"embed", "embed_w", "qkv", "o_proj", "fc1", "fc2"} or {"embed", "embed_w"} <= set(pops):
            raise ValueError(f"precise_ops must name embed | embed_w and q|k|v / o_proj / fc1 / fc2, not {self.precise_ops}")
        pk = self._cached_pack(device, (bf, npre, pops))
        if pk is not None:
            return pk
        c = self.config
        f32 = torch.float32
        P = lambda n: self.P(n).detach().to(device)  # noqa: E731
        if self._lora is not None:
            # adapters attached: every adapted weight is vc_lora_merge's fp32 W + s B A, the tensor lora.merge
            # writes into the masters, so the packs (and the logits) are those of the merged model
            from . import lora
            if npre > 0:
                lora.refuse(self, "compute_dtype=float16 with precise_layers > 0")
            adapted = self._lora.by_weight()
            P = lambda n: (lora.merged_weight(self, n, device) if n in adapted  # noqa: E731
                           else self.P(n).detach().to(device))
        D = c.hidden_size
        kt, kh, kw = c.tubelet_size
        pk = {"device": device, "version": self._weights_version(), "extra": (bf, npre, pops), "pops": pops}

        def split(w, emb=False):
            # [W_hi | W_lo] (embedding: [W_hi | W_hi | W_lo] against [A_hi | A_lo] with A wrapping)
            w = w.float()
            hi = w.to(torch.float16)
            lo = (w - hi.float()).to(torch.float16)
            return torch.cat([hi, hi, lo] if emb else [hi, lo], dim=1).contiguous()

        pk["w_emb"] = P("vivit.embeddings.patch_embeddings.projection.weight").reshape(D, -1).to(bf).contiguous()
        if "embed" in pops or "embed_w" in pops:
            pk["w_emb_split"] = split(P("vivit.embeddings.patch_embeddings.projection.weight").reshape(D, -1),
                                      emb="embed" in pops)
        pk["b_emb"] = P("vivit.embeddings.patch_embeddings.projection.bias").to(f32).contiguous()
        pk["pos"] = P("vivit.embeddings.position_embeddings").reshape(-1, D).to(f32).contiguous()
        pk["cls"] = P("vivit.embeddings.cls_token").reshape(D).to(f32).contiguous()
        layers = []
        for i in range(c.num_hidden_layers):
            p = f"vivit.layers.{i}."
            L = {}
            L["ln1_g"] = P(p + "layernorm_before.weight").contiguous()
            L["ln1_b"] = P(p + "layernorm_before.bias").contiguous()
            L["ln2_g"] = P(p + "layernorm_after.weight").contiguous()
            L["ln2_b"] = P(p + "layernorm_after.bias").contiguous()
            # softmax scale * log2(e) folded into the q projection (fp32 master -> one bf16 rounding),
            # so the attention kernel's exp2 argument comes straight out of the QK^T MFMA
            qs = (D // c.num_attention_heads) ** -0.5 * ops.LOG2E
            L["w_qkv"] = torch.cat([P(p + "attention.q_proj.weight") * qs, P(p + "attention.k_proj.weight"),
                                    P(p + "attention.v_proj.weight")]).to(bf).contiguous()
            L["b_qkv"] = torch.cat([P(p + "attention.q_proj.bias") * qs, P(p + "attention.k_proj.bias"),
                                    P(p + "attention.v_proj.bias")]).contiguous()
            L["w_o"] = P(p + "attention.o_proj.weight").to(bf).contiguous()
            L["b_o"] = P(p + "attention.o_proj.bias").contiguous()
            L["w_1"] = P(p + "mlp.fc1.weight").to(bf).contiguous()
            L["b_1"] = P(p + "mlp.fc1.bias").contiguous()
            L["w_2"] = P(p + "mlp.fc2.weight").to(bf).contiguous()
            L["b_2"] = P(p + "mlp.fc2.bias").contiguous()
            if i < npre:
                sp = {}
                if "qkv" in pops:
                    sp["w_qkv"] = split(torch.cat([P(p + "attention.q_proj.weight") * qs,
                                                   P(p + "attention.k_proj.weight"), P(p + "attention.v_proj.weight")]))
                if "o_proj" in pops:
                    sp["w_o"] = split(P(p + "attention.o_proj.weight"))
                if "fc1" in pops:
                    sp["w_1"] = split(P(p + "mlp.fc1.weight"))
                if "fc2" in pops:
                    sp["w_2"] = split(P(p + "mlp.fc2.weight"))
                L["split"] = sp
            layers.append(L)
        pk["layers"] = layers
        pk["lnf_g"] = P("vivit.layernorm.weight").contiguous()
        pk["lnf_b"] = P("vivit.layernorm.bias").contiguous()
        pk["w_cls"] = P("classifier.weight").to(f32).contiguous()
        pk["b_cls"] = P("classifier.bias").to(f32).contiguous()
        self._packed = pk
        return pk

    def geometry(self, B):
        c = self.config
        kt, kh, kw = c.tubelet_size
        npatch = (c.num_frames // kt) * (c.image_size // kh) * (c.image_size // kw)
        S = npatch + 1
        Mpad = round_up(B * S + 128, 256)
        Memb = round_up(B * npatch, 128)
        return npatch, S, Mpad, Memb

    def _workspace(self, B, device, part: int = 0):
        # 8 entries: (1 + 2 stream parts) x {bf16, fp16} fit
        return self._cached_workspace((B, str(device), part, self.compute_dtype, self.precise_layers > 0),
                                      lambda: self._make_workspace(B, device), 8)

    def _make_workspace(self, B, device):
        c = self.config
        D, I = c.hidden_size, c.intermediate_size
        kt, kh, kw = c.tubelet_size
        npatch, S, Mpad, Memb = self.geometry(B)
        bf = self.compute_dtype
        z = lambda *s, dt=bf: torch.zeros(s, dtype=dt, device=device)  # noqa: E731
        Kemb = c.num_channels * kt * kh * kw
        precise = self.precise_layers > 0 and bf == torch.float16
        if precise:
            # the split-operand embedding runs on the 256-row ping-pong kernel (vc_gemm_h16_wrap): its A rows
            # rounded up to 256 (zero rows past B*npatch), and X 256 rows deeper so the remapped rows of that
            # padding (tokens B*S+1 .. B*S+256, values bias + pos: finite) stay inside the buffer; the layers
            # address X[:Mpad] as always
            Memb = round_up(B * npatch, 256)
            Xe = z(Mpad + 256, D, dt=torch.float32)
        else:
            Xe = z(Mpad, D, dt=torch.float32)
        ws = dict(A_emb=z(Memb, Kemb), X=Xe[:Mpad], X_emb=Xe, Y=z(Mpad, D),
                  QKV=z(Mpad, 3 * D), O=z(Mpad, D), Hd=z(Mpad, I), logits=z(B, c.num_labels, dt=torch.float32),
                  # the CLS-only last layer: its attention partials and the CLS rows' MLP hidden state
                  cls_work=ops.cls_attention_work(B, S, c.num_attention_heads, device), Hc=z(B, I))
        if precise:
            ws["A_emb_split"] = z(Memb, 2 * Kemb)
        return ws

    # ---- forward -----------------------------------------------------------------
    def forward(self, pixel_values: torch.Tensor = None, labels: torch.Tensor = None, **kw):
        if pixel_values is None:
            raise ValueError("pixel_values required")
        if pixel_values.device.type != "cuda":
            raise RuntimeError("VivitForVideoClassification (vclip_amd) runs on the GPU only: move pixel_values "
                               "to cuda (the reference's `.to(device)`, trainer.py:92)")
        x = pixel_values.contiguous().float() if pixel_values.dtype != torch.float32 else pixel_values.contiguous()
        params = self._param_list()
        if self._lora is not None:
            params = params + self._lora.params(self)
        if self.training and torch.is_grad_enabled() and any(p.requires_grad for p in params):
            logits = VivitTrainFn.apply(self, x, *params)  # forward saving activations; HIP backward
        else:
            with torch.no_grad():
                logits = self.forward_logits(x).clone()  # the workspace buffer is reused by the next call
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

    # forward_logits (hosting.FusedVideoModel): with `concurrent_streams = n > 1` one part's kernels fill the
    # CUs another part's tail rounds and short launches leave idle: ViViT-B B = 8 840 -> 916 and 857 -> 911
    # clips/s with 2 streams on two boxes (tools/exp_streams.py; 3 streams 813-855).  bench.py's headline runs
    # 2 streams; its kernel roofline is timed in a separate one-stream pass (under overlap a launch's event
    # time includes time shared with the other stream's kernels).
    def _graph_knobs(self):
        return (self.compute_dtype,
                tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in self.gemm_cfg.items())), self.rows,
                self.precise_layers, tuple(sorted(self.precise_ops)),
                None if self.stream_priorities is None else tuple(self.stream_priorities), self._cls_only())

    def _cls_only(self) -> bool:
        return bool(self.cls_only_last_layer) and not self.training

    def _part_kwargs(self):
        return dict(cls_only=self._cls_only())

    def _split_options(self, B, ns):
        # the tuning of the part streams is per operand type too
        return dict(sizes=self.split_sizes if self.split_sizes is not None else SPLIT_DEFAULT.get((B, ns)),
                    key_extra=(self.compute_dtype,))

    def _forward_part(self, pix: torch.Tensor, part: int, out=None, cls_only: bool = False, keep=None) -> torch.Tensor:
        """One part's forward.  cls_only = False: every layer over every token row (X ends as the full last
        hidden state); True: the last layer past its q|k|v GEMM for the CLS rows only, where it can.
        keep (explain only, bf16, cls_only False): {"QKV": [L, Mpad, 3D], "LSE": [L, B*H*S]} -- layer i's q|k|v
        goes to keep["QKV"][i] instead of the shared buffer and its attention is ops.attention_fwd_lse, which
        stores the base-2 log-sum-exp in keep["LSE"][i]."""
        c = self.config
        B = pix.shape[0]
        pk = self._pack(pix.device)
        ws = self._workspace(B, pix.device, part)
        D = c.hidden_size
        npatch, S, Mpad, Memb = self.geometry(B)
        kt_, kh_, kw_ = c.tubelet_size
        eps = c.layer_norm_eps
        X, Y, QKV, O, Hd = ws["X"], ws["Y"], ws["QKV"], ws["O"], ws["Hd"]
        # optional per-launch HIP-event timing (bench.py), recorded on this part's stream, the
        # one each kernel runs on: a list collects the attention launches only, a dict every op
        ev = self.kernel_events

        def run(name, fn, *args, **kw):
            if ev is None or (not isinstance(ev, dict) and name != "attention"):
                return fn(*args, **kw)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*args, **kw)
            e1.record()
            (ev.setdefault(name, []) if isinstance(ev, dict) else ev).append((e0, e1))
            return r

        # algorithmic work per launch for an installed ops.OpRecorder (B*S token rows, no padding)
        M = B * S
        I = c.intermediate_size
        Kemb = c.num_channels * kt_ * kh_ * kw_
        T_, H_ = c.num_frames, c.image_size
        ln_bytes = M * D * (4 + 2)
        tm = ops.timed
        if "A_emb_split" in ws and "w_emb_split" in pk and "embed_w" in pk["pops"]:
            # split weights only: A (plain fp16 im2col) wrapping against [W_hi | W_lo]
            run("im2col", tm, "im2col_kernel", "im2col", B * (T_ * c.num_channels * H_ * H_ * 4 + npatch * Kemb * 2),
                "byte", ops.tubelet_im2col, pix, c.tubelet_size, ws["A_emb"])
            run("embed", ops.gemm_wrap, ws["A_emb"], Kemb, pk["w_emb_split"], pk["b_emb"], "embed_f32", ws["X_emb"],
                aux=pk["pos"][1:], group=npatch, group_stride=S, group_offset=1, m=ws["A_emb"].shape[0],
                flop=2.0 * B * npatch * D * Kemb, op="embed")
        elif "A_emb_split" in ws and "w_emb_split" in pk:
            # split operands: [A_hi | A_lo] against [W_hi | W_hi | W_lo] (A_hi W_hi + A_lo W_hi + A_hi W_lo)
            run("im2col", tm, "im2col_kernel", "im2col", B * (T_ * c.num_channels * H_ * H_ * 4 + npatch * Kemb * 4),
                "byte", ops.patch_im2col_split, pix, c.tubelet_size, ws["A_emb_split"])
            run("embed", ops.gemm_wrap, ws["A_emb_split"], 2 * Kemb, pk["w_emb_split"], pk["b_emb"], "embed_f32",
                ws["X_emb"], aux=pk["pos"][1:], group=npatch, group_stride=S, group_offset=1,
                m=ws["A_emb_split"].shape[0],
                flop=2.0 * B * npatch * D * Kemb, op="embed")
        else:
            run("im2col", tm, "im2col_kernel", "im2col", B * (T_ * c.num_channels * H_ * H_ * 4 + npatch * Kemb * 2),
                "byte", ops.tubelet_im2col, pix, c.tubelet_size, ws["A_emb"])
            run("embed", ops.gemm, ws["A_emb"], pk["w_emb"], pk["b_emb"], "embed_f32", X, aux=pk["pos"][1:],
                group=npatch, group_stride=S, group_offset=1, m=Memb, flop=2.0 * B * npatch * D * Kemb, op="embed")
        ops.cls_init(pk["cls"], pk["pos"], X, B, S)
        act = "bias_gelu_tanh" if c.hidden_act in ("gelu_fast", "gelu_pytorch_tanh", "gelu_new") else "bias_gelu_erf"
        scale = 1.0 / math.sqrt(D // c.num_attention_heads)
        qkv_gemm = fc2_gemm = ops.gemm
        gc = self.gemm_cfg
        tight = self.rows == "tight"

        def rows(name):
            """(m, cfg) of one GEMM: every padded row, or B*S up to its tile height (256 rows for the
            256-row configs 0/3/4 and for vc_gemm's own pick, which prefers them, else 128)"""
            cfg = gc.get(name)
            if isinstance(cfg, (list, tuple)):  # one config per stream part
                cfg = cfg[part]
            if not tight:
                return None, -1 if cfg is None else cfg
            h = 128 if cfg in (5, 7, 21) else 256
            return round_up(B * S, h), -1 if cfg is None else cfg

        m_ln = B * S if tight else None
        (m_qkv, c_qkv), (m_o, c_o), (m_1, c_1), (m_2, c_2) = rows("qkv"), rows("o_proj"), rows("fc1"), rows("fc2")
        Hn = c.num_attention_heads
        attn_flop = 4.0 * S * S * (D // Hn) * Hn * B
        # the last layer for the CLS rows only: not with split operands there, nor at a width the skinny GEMM refuses
        n_full = len(pk["layers"])
        if (cls_only and n_full and "split" not in pk["layers"][-1] and D // Hn == 64
                and ops.skinny_gemm_takes(D) and ops.skinny_gemm_takes(I)):
            n_full -= 1
        for li, L in enumerate(pk["layers"]):
            if keep is not None:
                QKV = keep["QKV"][li]
            sp = L.get("split", {})  # the split-operand fp16 GEMMs (precise_layers / precise_ops): A wraps against [W_hi | W_lo]
            run("layernorm", tm, "layernorm_kernel", "layernorm", ln_bytes, "byte", ops.layernorm, X, L["ln1_g"],
                L["ln1_b"], eps, Y, m=m_ln)
            if "w_qkv" in sp:
                run("qkv", ops.gemm_wrap, Y, D, sp["w_qkv"], L["b_qkv"], "bias", QKV, flop=2.0 * M * 3 * D * D, op="qkv")
            else:
                run("qkv", qkv_gemm, Y, L["w_qkv"], L["b_qkv"], "bias", QKV, m=m_qkv, cfg=c_qkv,
                    flop=2.0 * M * 3 * D * D, op="qkv")
            if li >= n_full:
                Xc, Oc, Hc = X[:M:S], O[:M:S], ws["Hc"]  # the CLS rows b*S in place
                es = Y.element_size()
                if S <= ops.ATTN_SHORT_MAX_S:
                    # vc_attention_fwd's short-sequence kernel: one workgroup per (clip, head) with every key in
                    # LDS, so there is no query work to drop, and its max-free 16-bit P is not what the CLS
                    # kernel computes (at S = 33 that alone moved the logits by 0.8 of their bf16 error)
                    run("attention", tm, "attn_fwd_d64_kernel", "attention", attn_flop, "flop", ops.attention, QKV, B,
                        S, Hn, scale, O, q_prescaled=True)
                else:
                    run("cls_attention", tm, "cls_attn_kernel", "cls_attention", B * (2 * S + 2) * D * es, "byte",
                        ops.cls_attention, QKV, B, S, Hn, ws["cls_work"], O)
                run("cls_o_proj", tm, "skinny_gemm_kernel", "cls_o_proj", D * D * es, "byte", ops.skinny_gemm, Oc,
                    L["w_o"], L["b_o"], "bias_resid_f32", Xc)
                run("cls_fc1", tm, "skinny_gemm_kernel", "cls_fc1", I * D * es, "byte", ops.skinny_gemm, Xc, L["w_1"],
                    L["b_1"], act, Hc, ln=(L["ln2_g"], L["ln2_b"], eps))
                run("cls_fc2", tm, "skinny_gemm_kernel", "cls_fc2", D * I * es, "byte", ops.skinny_gemm, Hc, L["w_2"],
                    L["b_2"], "bias_resid_f32", Xc)
                continue
            if keep is not None:
                run("attention", tm, "attn_fwd_d64_kernel", "attention", attn_flop, "flop", ops.attention_fwd_lse, QKV,
                    B, S, Hn, O, keep["LSE"][li], scale=scale, q_prescaled=True)
            else:
                run("attention", tm, "attn_fwd_d64_kernel", "attention", attn_flop, "flop", ops.attention, QKV, B, S, Hn,
                    scale, O, q_prescaled=True)
            if "w_o" in sp:
                run("o_proj", ops.gemm_wrap, O, D, sp["w_o"], L["b_o"], "bias_resid_f32", X, flop=2.0 * M * D * D,
                    op="o_proj")
            else:
                run("o_proj", ops.gemm, O, L["w_o"], L["b_o"], "bias_resid_f32", X, m=m_o, cfg=c_o,
                    flop=2.0 * M * D * D, op="o_proj")
            run("layernorm", tm, "layernorm_kernel", "layernorm", ln_bytes, "byte", ops.layernorm, X, L["ln2_g"],
                L["ln2_b"], eps, Y, m=m_ln)
            if "w_1" in sp:
                run("fc1", ops.gemm_wrap, Y, D, sp["w_1"], L["b_1"], act, Hd, flop=2.0 * M * I * D, op="fc1")
            else:
                run("fc1", ops.gemm, Y, L["w_1"], L["b_1"], act, Hd, m=m_1, cfg=c_1, flop=2.0 * M * I * D, op="fc1")
            if "w_2" in sp:
                run("fc2", ops.gemm_wrap, Hd, I, sp["w_2"], L["b_2"], "bias_resid_f32", X, flop=2.0 * M * D * I,
                    op="fc2")
            else:
                run("fc2", fc2_gemm, Hd, L["w_2"], L["b_2"], "bias_resid_f32", X, m=m_2, cfg=c_2,
                    flop=2.0 * M * D * I, op="fc2")
        return ops.cls_head(X, B, S, pk["lnf_g"], pk["lnf_b"], eps, pk["w_cls"], pk["b_cls"],
                            out=ws["logits"] if out is None else out)


    # ---- explain ------------------------------------------------------------------
    EXPLAIN_METHODS = ("rollout", "cls_attention", "grad_rollout")

    def _explain_buffers(self, B, device):
        def build():
            c = self.config
            _, S, Mpad, _ = self.geometry(B)
            Hn, nl = c.num_attention_heads, c.num_hidden_layers
            seed = torch.zeros(B, S, dtype=torch.float32)
            seed[:, 0] = 1.0  # e_CLS, made on the host: one copy, no device arithmetic
            f = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)  # noqa: E731
            return dict(QKV=torch.zeros(nl, Mpad, 3 * c.hidden_size, dtype=torch.bfloat16, device=device),
                        LSE=f(nl, B * Hn * S), seed=seed.to(device), r=(f(B, S), f(B, S)),
                        work=ops.attention_rollout_work(B, S, Hn, device))

        return self._cached_explain(self._explain_ws, (B, str(device)), build)

    def _explain_grad_engine(self, B, device):
        key = (B, str(device))
        if key not in self._explain_grad:
            self._explain_grad = {}  # one batch size at a time: the engine keeps every layer's activations
            self._explain_grad[key] = GradRolloutEngine(self, B, device)
        return self._explain_grad[key]

    def _explain_targets(self, target):
        """`target` of explain checked against the labels: (None or a list of class indices, whether it was one int
        for every clip)"""
        return explaining.check_targets(target, self.config.num_labels)

    @staticmethod
    def _check_targets(target, nl: int):
        """explaining.check_targets against `nl` labels"""
        return explaining.check_targets(target, nl)

    def _explain_grad_rollout(self, pix, target, scalar_target) -> Explanation:
        """explain(method="grad_rollout") past the argument checks: pix f32 contiguous on the GPU, target from
        _explain_targets"""
        c = self.config
        B, T, _, H, W = pix.shape
        target = explaining.expand_targets(target, scalar_target, B)
        eng = self._explain_grad_engine(B, pix.device)
        logits = eng.forward(pix).clone()
        if target is None:
            target = logits.argmax(dim=1).tolist()
        rel = eng.backward_rollout(target).cpu()  # the one copy; the rest is host bookkeeping on [B, S]
        kt, kh, kw = c.tubelet_size
        patch = rel[:, 1:].double()
        total = patch.sum(dim=1, keepdim=True)
        if not bool((total > 0).all()):
            raise RuntimeError(f"explain: grad_rollout found no positive gradient-weighted attention for target "
                               f"{target}: the patch relevances of clip(s) "
                               f"{[b for b in range(B) if not total[b, 0] > 0]} sum to 0")
        sal = explaining.normalise(patch, zero_ok=False).reshape(B, T // kt, H // kh, W // kw)
        return Explanation(logits, rel, sal, sal.sum(dim=(2, 3)), method="grad_rollout", target=target)

    @torch.no_grad()
    def explain(self, pixel_values: torch.Tensor, method: str = "rollout", residual: float = 0.5,
                target=None) -> Explanation:
        """The logits and which tokens produced them: attention rollout (Abnar & Zuidema 2020) of the CLS row.

        method "rollout": r = e_CLS, then for layers L .. 1  r <- residual * mean_h(A_h)^T r + (1 - residual) * r,
        i.e. the CLS row of prod_l (residual * A_l + (1 - residual) * I); "cls_attention": the head-mean CLS
        attention row of the last layer (one step, no residual mix).  Every step is ops.attention_rollout_step,
        which recomputes the probabilities from the layer's q|k|v and log-sum-exp: no S x S matrix exists.

        Runs the ordinary full eager forward (every layer over every token, no graph replay, no stream split)
        with the lse-storing attention kernel and keeps every layer's q|k|v [L, Mpad, 3D] bf16 and lse
        [L, B*H*S] f32 in buffers of its own, cached per (B, device): about 173 MB per clip at ViViT-B/16x2
        (184 MB at B = 1 with the row padding).  The forward's workspaces, graphs and logits are untouched.
        The [B, S] result is copied to the host once; normalisation and the spatial sum happen there.
        Refuses (no fallback): training mode, CPU tensors, compute_dtype fp16 (the lse forward is bf16-only),
        precise_layers > 0, head_dim != 64.

        method "grad_rollout" is class-specific where the two above are not: the gradient-weighted rollout of
        Chefer, Gur & Wolf (2021), r = e_CLS, then for layers L .. 1  r <- r + mean_h(max(dy_t/dA_h * A_h, 0))^T r
        with y_t the logit of `target`: None = per clip the argmax of the logits this call computed, an int = that
        class for every clip, or B ints (sequence or tensor); out of range, or given with another method, is a
        ValueError.  `residual` is not used by this method.  It runs a forward that keeps what a backward needs
        and the train step's data-gradient chain without any weight gradient (vivit_explain.py), each layer's
        ops.attention_grad_rollout_step as soon as its dO exists; `logits` are that forward's and
        Explanation.target the B classes explained.  Its buffers (every layer's residual stream, q|k|v, attention
        output, lse and pre-GELU hidden state, and transposed bf16 weights) are cached for one (B, device).  A clip
        whose patch relevances sum to 0 (no positive product anywhere) raises RuntimeError.  Refuses what the
        other methods refuse, and a hidden_act that is not a tanh GELU."""
        c = self.config
        explaining.require_method(method, self.EXPLAIN_METHODS)
        if target is not None and method != "grad_rollout":
            raise ValueError(f"explain: target is for method 'grad_rollout', not {method!r}")
        target, scalar_target = self._explain_targets(target)
        explaining.require_residual(residual)
        explaining.require_explainable(self, pixel_values, what="pixel_values")
        if self.compute_dtype != torch.bfloat16:
            raise RuntimeError("explain: compute_dtype must be torch.bfloat16 (the lse-storing attention forward is bf16-only)")
        if self.precise_layers > 0:
            raise RuntimeError("explain: precise_layers > 0 (split-operand fp16 layers) is not supported")
        if c.hidden_size // c.num_attention_heads != 64:
            raise RuntimeError("explain: head_dim must be 64")
        pix = pixel_values.contiguous()
        if pix.dtype != torch.float32:
            pix = pix.float()
        B, T, C, H, W = pix.shape
        if T != c.num_frames or H != c.image_size or W != c.image_size or C != c.num_channels:
            raise ValueError(f"pixel_values {tuple(pix.shape)} do not match config "
                             f"(T={c.num_frames}, C={c.num_channels}, {c.image_size}^2)")
        if method == "grad_rollout":
            if self._lora is not None:
                from . import lora
                lora.refuse(self, "explain(method=\"grad_rollout\")")
            return self._explain_grad_rollout(pix, target, scalar_target)
        _, S, _, _ = self.geometry(B)
        Hn, nl = c.num_attention_heads, c.num_hidden_layers
        buf = self._explain_buffers(B, pix.device)
        logits = self._forward_part(pix, 0, cls_only=False, keep=buf).clone()
        steps = [(li, float(residual)) for li in reversed(range(nl))] if method == "rollout" else [(nl - 1, 1.0)]
        r_in = buf["seed"]
        for k, (li, alpha) in enumerate(steps):
            r_out = buf["r"][k & 1]
            ops.attention_rollout_step(buf["QKV"][li], buf["LSE"][li], r_in, B, S, Hn, alpha, buf["work"], r_out)
            r_in = r_out
        rel = r_in.cpu()  # the one copy; the rest is host bookkeeping on [B, S]
        kt, kh, kw = c.tubelet_size
        sal = explaining.normalise(rel[:, 1:].double(), zero_ok=False).reshape(B, T // kt, H // kh, W // kw)
        return Explanation(logits, rel, sal, sal.sum(dim=(2, 3)), method)


def create_model(model_name="google/vivit-b-16x2-kinetics400", num_classes=2, class_labels=None, num_frames=32,
                 device="cuda", logger=None, weights_seed: int = 0):
    """Drop-in for vivit_transformer/vivit_classifier/models/vivit_model.py:4-52.

    The reference pulls `VivitConfig.from_pretrained(model_name)` and pretrained weights
    from the HF hub; this image has no network, so the architecture of the named
    checkpoint (ViViT-B/16x2) is built with seeded synthetic weights (vclip_amd.weights)
    unless a checkpoint is loaded afterwards with `load_state_dict`.  As in the
    reference, `num_labels` follows `class_labels` (id2label) and `num_frames` is set.
    """
    class_labels = class_labels or ["non-referral", "referral"]
    id2label = {i: l for i, l in enumerate(class_labels)}
    cfg = VivitConfig(num_frames=num_frames, id2label=id2label, label2id={l: i for i, l in id2label.items()})
    if logger:
        logger.info(f"Creating ViViT model {model_name} (num_frames={num_frames}, labels={class_labels}) on {device}")
    model = VivitForVideoClassification(cfg)
    from .weights import make_vivit_weights
    model.load_state_dict(make_vivit_weights(cfg.as_shape_cfg(), seed=weights_seed))
    model = model.to(device) if device else model
    return model.eval()  # like transformers' from_pretrained; the trainer calls model.train()
