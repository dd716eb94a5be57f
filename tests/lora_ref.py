"""fp32 reference of LoRA fine-tuning for the tests: oracle.vivit_ref.vivit_forward on a parameter dict in which
every targeted weight is the tensor W + s * B @ A, with A, B (and the classifier when train_head) requiring grad, so
torch autograd yields dA, dB and the classifier gradients of the very function vclip_amd.lora computes."""
import torch

from oracle.vivit_ref import vivit_forward

MODULE = {"q": "attention.q_proj", "k": "attention.k_proj", "v": "attention.v_proj", "o": "attention.o_proj",
          "fc1": "mlp.fc1", "fc2": "mlp.fc2"}
HEAD = ("classifier.weight", "classifier.bias")


class LoraRef:
    """base: {HF name: numpy array} (frozen); adapters: {lora name: tensor} as vclip_amd.lora.state_dict names them."""

    def __init__(self, base: dict, cfg: dict, adapters: dict, scale: float, train_head: bool = True):
        self.cfg, self.s, self.train_head = cfg, float(scale), train_head
        self.base = {k: torch.from_numpy(v).clone() for k, v in base.items()}
        self.adapters = {k: v.detach().cpu().float().clone().requires_grad_() for k, v in adapters.items()
                         if k.endswith((".lora_A.weight", ".lora_B.weight"))}
        if train_head:
            for n in HEAD:
                self.base[n].requires_grad_()

    def trainable(self) -> dict:
        t = dict(self.adapters)
        if self.train_head:
            t.update({n: self.base[n] for n in HEAD})
        return t

    def effective(self) -> dict:
        p = dict(self.base)
        for na in self.adapters:
            if na.endswith(".lora_A.weight"):
                pre = na[:-len(".lora_A.weight")]
                p[pre + ".weight"] = self.base[pre + ".weight"] + self.s * (self.adapters[pre + ".lora_B.weight"]
                                                                           @ self.adapters[na])
        return p

    def forward(self, pix: torch.Tensor) -> torch.Tensor:
        return vivit_forward(self.effective(), self.cfg, pix)

    def grads(self, pix, labels):
        """(loss, logits, {trainable name: gradient}) of one cross-entropy step"""
        for v in self.trainable().values():
            v.grad = None
        logits = self.forward(pix)
        loss = torch.nn.functional.cross_entropy(logits, labels)
        loss.backward()
        return float(loss.detach()), logits.detach(), {k: v.grad.clone() for k, v in self.trainable().items()}
