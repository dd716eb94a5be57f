"""The class-specific saliency of `VivitForVideoClassification.explain(method="grad_rollout")`: the
gradient-weighted attention rollout of Chefer, Gur & Wolf (ICCV 2021, "Generic Attention-model
Explainability", the self-attention rule) for the CLS row,
    A_l = mean_h max(dy_t/dA_l[h] * A_l[h], 0);   r = e_CLS;   for l = L .. 1:  r <- r + A_l^T r.

The reference's HF model would do this with `output_attentions=True` plus autograd; the flash kernels here
never store a probability.  dy_t/dA_l[h][i][j] = dO_l[h][i] . v_j, so a layer's step needs its kept q'|k|v,
its log-sum-exp and the gradient dO at its attention output (ops.attention_grad_rollout_step).  dO comes
from the data-gradient chain of the train step (vivit_train.TrainEngine.backward) with everything a train
step adds left out: no weight or bias gradients (ops.wgrad / ops.colsum), no side streams, no flat
buffers.  That chain walks the layers last to first, as the CLS-row rollout does, so each layer's step
runs as soon as its dO exists and one dO buffer serves every layer.

The engine reads the model's packed inference weights (`model._pack`, the bf16 operands the eager forward
uses) and keeps its own transposed copies for the data-gradient GEMMs; it touches neither the fp32 masters'
layout nor any `.grad`.  Its forward is TrainEngine.forward's kernel sequence (every layer over every
token, the residual stream and the pre-GELU hidden state kept for the backward).
"""
from __future__ import annotations

import torch

from . import ops

TANH_ACTS = ("gelu_fast", "gelu_pytorch_tanh", "gelu_new")


class GradRolloutEngine:
    """Device buffers and the kernel sequence of one explain(method="grad_rollout") for a fixed batch size."""

    def __init__(self, model, B: int, device):
        c = model.config
        if c.hidden_act not in TANH_ACTS:
            raise RuntimeError(f"explain: grad_rollout needs a tanh GELU (hidden_act one of {TANH_ACTS}), not "
                               f"{c.hidden_act!r}: the data-gradient chain has no backward for it")
        self.model, self.B, self.device = model, B, device
        D, I, H, L = c.hidden_size, c.intermediate_size, c.num_attention_heads, c.num_hidden_layers
        kt, kh, kw = c.tubelet_size
        npatch, S, Mpad, Memb = model.geometry(B)
        self.D, self.I, self.H, self.L, self.S, self.Mpad, self.Memb, self.npatch = D, I, H, L, S, Mpad, Memb, npatch
        bf, f32 = torch.bfloat16, torch.float32
        z = lambda *s, dt=bf: torch.zeros(s, dtype=dt, device=device)  # noqa: E731
        # forward activations the backward and the rollout steps read
        self.A_emb = z(Memb, c.num_channels * kt * kh * kw)
        self.R = [z(Mpad, D, dt=f32) for _ in range(2 * L + 1)]  # residual stream before / after each block
        self.QKV = [z(Mpad, 3 * D) for _ in range(L)]
        self.O = [z(Mpad, D) for _ in range(L)]
        self.LSE = [z(B * H * S, dt=f32) for _ in range(L)]
        self.Hpre = [z(Mpad, I) for _ in range(L)]
        self.Y, self.Hd = z(Mpad, D), z(Mpad, I)  # LayerNorm output, MLP hidden: consumed at once
        self.logits = z(B, c.num_labels, dt=f32)
        # backward
        self.dlogits = z(B, c.num_labels, dt=f32)
        self.dX = z(Mpad, D, dt=f32)
        self.dXa, self.dXb, self.dO = z(Mpad, D), z(Mpad, D), z(Mpad, D)
        self.dY = z(Mpad, D, dt=f32)
        self.dH = z(Mpad, I)
        self.dQKV = z(Mpad, 3 * D)
        self.delta = z(B * H * S, dt=f32)
        self.ln_work = z((512 + 16) * 2 * D, dt=f32)
        self.zeros = z(max(I, 3 * D), dt=f32)
        # the parameter-gradient outputs cls_head_bwd and layernorm_bwd always write: a few [D] vectors, discarded
        self.g_wc, self.g_bc = z(c.num_labels, D, dt=f32), z(c.num_labels, dt=f32)
        self.g_gamma, self.g_beta = z(D, dt=f32), z(D, dt=f32)
        # rollout
        seed = torch.zeros(B, S, dtype=f32)
        seed[:, 0] = 1.0  # e_CLS, made on the host
        self.seed = seed.to(device)
        self.r = (z(B, S, dt=f32), z(B, S, dt=f32))
        self.work = ops.attention_rollout_work(B, S, H, device)
        self._pk = None  # the packed weights self.WT was transposed from
        self.WT = None

    def _weights(self):
        """the model's packed bf16 weights and, per layer, their transposes (the dgrad GEMMs' operands),
        made once per pack"""
        pk = self.model._pack(self.device)
        if pk is not self._pk:
            self.WT = [dict(qkvT=L["w_qkv"].t().contiguous(), oT=L["w_o"].t().contiguous(),
                            f1T=L["w_1"].t().contiguous(), f2T=L["w_2"].t().contiguous()) for L in pk["layers"]]
            self._pk = pk
        return pk

    def forward(self, pix: torch.Tensor) -> torch.Tensor:
        """logits f32 [B, labels] (the engine's buffer); keeps what backward_rollout reads"""
        c = self.model.config
        pk = self._weights()
        B, S, H = self.B, self.S, self.H
        eps = c.layer_norm_eps
        R, Y, Hd = self.R, self.Y, self.Hd
        ops.tubelet_im2col(pix, c.tubelet_size, self.A_emb)
        ops.gemm(self.A_emb, pk["w_emb"], pk["b_emb"], "embed_f32", R[0], aux=pk["pos"][1:], group=self.npatch,
                 group_stride=S, group_offset=1, m=self.Memb)
        ops.cls_init(pk["cls"], pk["pos"], R[0], B, S)
        for i, W in enumerate(pk["layers"]):
            ops.layernorm(R[2 * i], W["ln1_g"], W["ln1_b"], eps, Y)
            ops.gemm(Y, W["w_qkv"], W["b_qkv"], "bias", self.QKV[i])
            ops.attention_fwd_lse(self.QKV[i], B, S, H, self.O[i], self.LSE[i])
            ops.gemm(self.O[i], W["w_o"], W["b_o"], "bias_add_f32", R[2 * i + 1], aux=R[2 * i])
            ops.layernorm(R[2 * i + 1], W["ln2_g"], W["ln2_b"], eps, Y)
            ops.gemm(Y, W["w_1"], W["b_1"], "bias_gelu_tanh_save", Hd, aux=self.Hpre[i])
            ops.gemm(Hd, W["w_2"], W["b_2"], "bias_add_f32", R[2 * i + 2], aux=R[2 * i + 1])
        return ops.cls_head(R[2 * self.L], B, S, pk["lnf_g"], pk["lnf_b"], eps, pk["w_cls"], pk["b_cls"],
                            out=self.logits)

    def backward_rollout(self, target) -> torch.Tensor:
        """relevance f32 [B, S] on the device (one of the engine's buffers) for dlogits = one_hot(target),
        target a list of B class indices: the data-gradient chain of the forward just run, each layer's
        gradient-weighted rollout step as soon as its dO exists; ends after layer 0's step"""
        c = self.model.config
        pk = self._weights()
        B, S, H, D, I = self.B, self.S, self.H, self.D, self.I
        eps = c.layer_norm_eps
        dX, dXa, dXb, dY, dH, dO, dQKV = self.dX, self.dXa, self.dXb, self.dY, self.dH, self.dO, self.dQKV
        onehot = torch.zeros(B, c.num_labels, dtype=torch.float32)
        onehot[torch.arange(B), torch.as_tensor(target)] = 1.0
        self.dlogits.copy_(onehot)
        dX.zero_()
        dXa.zero_()
        ops.cls_head_bwd(self.R[2 * self.L], B, S, pk["lnf_g"], pk["lnf_b"], eps, pk["w_cls"], self.dlogits, dX, dXa,
                         self.g_wc, self.g_bc, self.g_gamma, self.g_beta)
        r_in = self.seed
        for k, i in enumerate(reversed(range(self.L))):
            W, WT = pk["layers"][i], self.WT[i]
            # MLP block: out = R1 + fc2(gelu(fc1(LN2(R1))))
            ops.gemm(dXa, WT["f2T"], self.zeros[:I], "dgelu_tanh", dH, aux=self.Hpre[i])
            ops.gemm(dH, WT["f1T"], self.zeros[:D], "bias_f32", dY)
            ops.layernorm_bwd(dY, self.R[2 * i + 1], W["ln2_g"], eps, dX, dXb, self.g_gamma, self.g_beta, self.ln_work,
                              m=B * S)
            # attention block: R1 = R0 + o_proj(attn(qkv(LN1(R0)))); dO is the gradient at attn's output
            ops.gemm(dXb, WT["oT"], self.zeros[:D], "bias", dO)
            r_out = self.r[k & 1]
            ops.attention_grad_rollout_step(self.QKV[i], dO, self.LSE[i], r_in, B, S, H, 1.0, 1.0, self.work, r_out)
            r_in = r_out
            if i == 0:
                break
            ops.attention_bwd(self.QKV[i], self.O[i], dO, self.LSE[i], self.delta, B, S, H, dQKV)
            ops.gemm(dQKV, WT["qkvT"], self.zeros[:D], "bias_f32", dY)
            ops.layernorm_bwd(dY, self.R[2 * i], W["ln1_g"], eps, dX, dXa, self.g_gamma, self.g_beta, self.ln_work,
                              m=B * S)
        return r_in
