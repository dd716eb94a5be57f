"""Low-rank adaptation (LoRA, Hu et al. 2021) of `vclip_amd.vivit.VivitForVideoClassification`: the base
weights are frozen, each targeted projection W [out, in] gets fp32 adapters A [r, in] and B [out, r] (the PEFT
shapes and names), and the model computes with W_eff = W + (alpha / r) B A.

    lora.attach(model, rank=8, alpha=16.0, targets=("q", "v"))   # freeze the base, add adapters (B = 0)
    opt = AdamW([p for p in model.parameters() if p.requires_grad], lr=...)
    ...the reference's train loop, unchanged...
    lora.merge(model)                                            # fold into the fp32 masters; a plain model again

The forward is merged: vc_lora_merge folds the delta in when the bf16 GEMM operands are packed, so the forward and
the data-gradient chain run on the same GEMMs at the same speed, and the train step replaces every weight gradient by
the rank-r products of csrc/lora.hip (vivit_train.TrainEngine.backward_lora).  There is no LoRA dropout: a merged
forward cannot express it (dropout acts on the adapter branch's input alone, which no longer exists as a branch).

Not supported while adapters are attached (NotImplementedError): GraphedTrainStep, grad_ready_hooks /
dp.GradAllReduce, explain(method="grad_rollout"), compute_dtype=float16 with precise_layers > 0.  After `merge`
the model is an ordinary one and all of them work.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch

TARGETS = ("q", "k", "v", "o", "fc1", "fc2")
_MODULE = {"q": "attention.q_proj", "k": "attention.k_proj", "v": "attention.v_proj", "o": "attention.o_proj",
           "fc1": "mlp.fc1", "fc2": "mlp.fc2"}
HEAD = ("classifier.weight", "classifier.bias")


def _key(name: str) -> str:
    return name.replace(".", "__")


def adapter_prefix(layer: int, target: str) -> str:
    return f"vivit.layers.{layer}.{_MODULE[target]}"


def resolve_layers(layers, L: int) -> list:
    """None: every layer; an int n: the last n layers; an iterable: those indices (sorted, unique)."""
    if layers is None:
        return list(range(L))
    if isinstance(layers, bool):
        raise ValueError("lora: layers must be None, an int or an iterable of layer indices")
    if isinstance(layers, int):
        if not 1 <= layers <= L:
            raise ValueError(f"lora: layers={layers} must be 1..{L} (the last n layers)")
        return list(range(L - layers, L))
    try:
        idx = sorted({int(i) for i in layers})
    except TypeError:
        raise ValueError("lora: layers must be None, an int or an iterable of layer indices") from None
    if not idx or idx[0] < 0 or idx[-1] >= L:
        raise ValueError(f"lora: layers {list(layers)} must be a non-empty subset of 0..{L - 1}")
    return idx


class LoraState:
    """What `attach` hangs on the model as `model._lora`: the configuration, the adapter parameters by name and
    (on the device, once a train step or a packed forward needs them) their flat fp32 master / gradient buffers
    and the classifier's own gradient tensor."""

    def __init__(self, model, rank, alpha, targets, layers, train_head):
        c = model.config
        self.rank, self.alpha, self.targets, self.layers, self.train_head = rank, float(alpha), targets, layers, train_head
        self.s = float(alpha) / rank
        D, I = c.hidden_size, c.intermediate_size
        dims = {"q": (D, D), "k": (D, D), "v": (D, D), "o": (D, D), "fc1": (I, D), "fc2": (D, I)}
        self.adapters = OrderedDict()  # (layer, target) -> (A name, B name, out, in)
        for i in layers:
            for t in targets:
                p = adapter_prefix(i, t)
                self.adapters[(i, t)] = (p + ".lora_A.weight", p + ".lora_B.weight") + dims[t]
        self.names = [n for a in self.adapters.values() for n in a[:2]]
        self.reset()

    def reset(self):
        self.flat = self.gflat = self.gscratch = None
        self.ghead = self.ghead_scratch = None

    def config(self) -> dict:
        return {"rank": self.rank, "alpha": self.alpha, "targets": list(self.targets), "layers": list(self.layers),
                "train_head": self.train_head}

    def by_weight(self) -> dict:
        """base weight name -> (A name, B name) of its adapter"""
        return {adapter_prefix(i, t) + ".weight": v[:2] for (i, t), v in self.adapters.items()}

    def first_layer(self) -> int:
        return self.layers[0]

    def param(self, model, name):
        return model.lora_params[_key(name)]

    def params(self, model) -> list:
        return [model.lora_params[_key(n)] for n in self.names]

    def trainable_head(self, model) -> list:
        return [model.P(n) for n in HEAD] if self.train_head else []

    def ensure_flat(self, model, device):
        """Adapters into one flat fp32 device buffer (the parameters become views of it, the same Parameter
        objects), a gradient buffer of the same layout, and the classifier's gradient tensor."""
        if self.flat is not None and self.flat.device == device:
            return
        ps = self.params(model)
        total = sum(p.numel() for p in ps)
        flat = torch.zeros(total, dtype=torch.float32, device=device)
        self.offsets = {}
        off = 0
        with torch.no_grad():
            for n, p in zip(self.names, ps):
                v = flat[off:off + p.numel()].view(p.shape)
                v.copy_(p.detach())
                p.data = v
                self.offsets[n] = (off, p.numel(), tuple(p.shape))
                off += p.numel()
        self.flat = flat
        self.gflat = torch.zeros_like(flat)
        self.gscratch = None
        nh = sum(model.P(n).numel() for n in HEAD)
        self.ghead = torch.zeros(nh, dtype=torch.float32, device=device)
        self.ghead_scratch = None

    def view(self, flat, name):
        off, numel, shape = self.offsets[name]
        return flat[off:off + numel].view(shape)

    def head_views(self, model, ghead):
        nw = model.P(HEAD[0]).numel()
        return ghead[:nw].view(model.P(HEAD[0]).shape), ghead[nw:].view(model.P(HEAD[1]).shape)


def _state(model) -> LoraState:
    st = getattr(model, "_lora", None)
    if st is None:
        raise RuntimeError("lora: the model has no adapters attached (lora.attach)")
    return st


def _invalidate(model):
    model._engine = None
    model._packed = None
    model._explain_grad = {}
    model._graphs.clear()


def attach(model, rank: int = 8, alpha: float = 16.0, targets=("q", "v"), layers=None, train_head: bool = True,
           seed: int = 0):
    """Freeze the base model and add rank-`rank` adapters to the `targets` (any subset of q, k, v, o, fc1, fc2) of
    `layers` (None: all; an int n: the last n; an iterable of indices).  A is kaiming-uniform (a = sqrt 5, PEFT's
    initialisation) from a CPU generator seeded with `seed`, B is zero, so the attached model computes what the base
    model does.  The adapters are registered on the model (`model.parameters()` yields them; `model.state_dict()`
    keeps returning the base weights alone); base parameters get requires_grad=False except the classifier's weight
    and bias when `train_head`.  No LoRA dropout (see the module docstring).  Returns the model."""
    from . import ops
    if getattr(model, "_lora", None) is not None:
        raise RuntimeError("lora.attach: adapters are already attached (lora.merge first)")
    if isinstance(rank, bool) or not isinstance(rank, int) or not 1 <= rank <= ops.LORA_MAX_RANK:
        raise ValueError(f"lora.attach: rank must be an int in 1..{ops.LORA_MAX_RANK}, not {rank!r}")
    if not float(alpha) > 0:
        raise ValueError(f"lora.attach: alpha must be positive, not {alpha!r}")
    if isinstance(targets, str):
        targets = tuple(t for t in targets.split(",") if t)
    targets = tuple(targets)
    bad = [t for t in targets if t not in TARGETS]
    if bad or not targets or len(set(targets)) != len(targets):
        raise ValueError(f"lora.attach: targets must be a non-empty subset of {TARGETS} without repeats, not {targets!r}")
    targets = tuple(t for t in TARGETS if t in targets)
    layers = resolve_layers(layers, model.config.num_hidden_layers)
    st = LoraState(model, rank, alpha, targets, layers, bool(train_head))
    device = model.P(HEAD[0]).device
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    model.lora_params = torch.nn.ParameterDict()
    for (i, t), (na, nb, nout, nin) in st.adapters.items():
        # kaiming_uniform_(a = sqrt 5) on [r, in]: bound = sqrt(6 / ((1 + a^2) fan_in)) = 1 / sqrt(in)
        a = (torch.rand(rank, nin, generator=gen, dtype=torch.float32) * 2.0 - 1.0) * (1.0 / math.sqrt(nin))
        model.lora_params[_key(na)] = torch.nn.Parameter(a.to(device))
        model.lora_params[_key(nb)] = torch.nn.Parameter(torch.zeros(nout, rank, dtype=torch.float32, device=device))
    for n in model._names:
        model.P(n).requires_grad_(st.train_head and n in HEAD)
        model.P(n).grad = None
    model._gflat = model._gscratch = None  # a full-size gradient buffer of an earlier full step, if any: not needed
    model._lora = st
    _invalidate(model)
    return model


def detach(model):
    """Drop the adapters without folding them in; the base parameters train again."""
    _state(model)
    model._lora = None
    del model.lora_params
    for n in model._names:
        model.P(n).requires_grad_(True)
        model.P(n).grad = None
    _invalidate(model)
    return model


def merged_weight(model, name: str, device=None) -> torch.Tensor:
    """fp32 W + s B A of one adapted base weight, from vc_lora_merge's fp32 output (a new tensor)."""
    from . import ops
    st = _state(model)
    na, nb = st.by_weight()[name]
    w = model.P(name).detach()
    device = w.device if device is None else device
    if torch.device(device).type != "cuda":
        raise RuntimeError("lora: merging runs on the GPU only (vc_lora_merge); move the model to cuda")
    w = w.to(device).contiguous()
    a = st.param(model, na).detach().to(device).contiguous()
    b = st.param(model, nb).detach().to(device).contiguous()
    out = torch.empty_like(w)
    ops.lora_merge(w, a, b, st.s, out=out)
    return out


def merged_state_dict(model) -> OrderedDict:
    """The HF-named state dict of the model with every adapter folded in (fp32, new tensors); the model itself is
    untouched.  Loads into a plain VivitForVideoClassification, which then computes the attached model's eval
    logits bit for bit."""
    st = _state(model)
    adapted = st.by_weight()
    sd = OrderedDict()
    for n in model._names:
        sd[n] = merged_weight(model, n) if n in adapted else model.P(n).detach().clone()
    return sd


def merge(model):
    """Fold the adapters into the fp32 masters (vc_lora_merge's fp32 output), drop them and unfreeze the base: the
    model is an ordinary one again, with the eval logits it had while attached."""
    st = _state(model)
    with torch.no_grad():
        for n in st.by_weight():
            model.P(n).copy_(merged_weight(model, n))
    return detach(model)


def state_dict(model) -> OrderedDict:
    """The adapters (and the classifier when train_head), as copies, plus {"lora_config": ...}."""
    st = _state(model)
    sd = OrderedDict((n, st.param(model, n).detach().clone()) for n in st.names)
    if st.train_head:
        for n in HEAD:
            sd[n] = model.P(n).detach().clone()
    sd["lora_config"] = st.config()
    return sd


def load_state_dict(model, sd):
    """Load what `state_dict` returned; attaches adapters of sd["lora_config"] first if the model has none."""
    cfg = dict(sd["lora_config"])
    if getattr(model, "_lora", None) is None:
        attach(model, rank=int(cfg["rank"]), alpha=float(cfg["alpha"]), targets=tuple(cfg["targets"]),
               layers=list(cfg["layers"]), train_head=bool(cfg["train_head"]))
    st = _state(model)
    if st.config() != {**cfg, "alpha": float(cfg["alpha"]), "targets": list(cfg["targets"]), "layers": list(cfg["layers"])}:
        raise ValueError(f"lora.load_state_dict: the model's adapters {st.config()} differ from the state's {cfg}")
    want = list(st.names) + (list(HEAD) if st.train_head else [])
    missing = [n for n in want if n not in sd]
    unexpected = [k for k in sd if k not in want and k != "lora_config"]
    if missing or unexpected:
        raise KeyError(f"lora.load_state_dict: missing={missing[:5]} unexpected={unexpected[:5]}")
    with torch.no_grad():
        for n in want:
            p = st.param(model, n) if n in st.names else model.P(n)
            p.copy_(torch.as_tensor(sd[n]).reshape(p.shape))
    model._packed = None
    return model


def trainable_parameters(model) -> int:
    return sum(p.numel() for p in model.parameters() if p.requires_grad)


def refuse(model, what: str):
    """NotImplementedError for a feature that does not run with adapters attached."""
    if getattr(model, "_lora", None) is not None:
        raise NotImplementedError(f"{what} is not supported with LoRA adapters attached; lora.merge(model) first")


def run_backward(model, eng, dlogits):
    """VivitForVideoClassification._run_backward in LoRA mode: the engine writes the adapter gradients into the small
    flat gradient buffer and the classifier's into its own tensor; frozen parameters keep .grad None."""
    st = _state(model)
    if model.grad_ready_hooks:
        refuse(model, "grad_ready_hooks (dp.GradAllReduce)")
    ps = st.params(model)
    head = st.trainable_head(model)
    accumulate = any(p.grad is not None for p in ps + head)
    if not accumulate:
        gflat, ghead = st.gflat, st.ghead
    else:
        if st.gscratch is None:
            st.gscratch, st.ghead_scratch = torch.zeros_like(st.gflat), torch.zeros_like(st.ghead)
        gflat, ghead = st.gscratch, st.ghead_scratch
    eng.backward_lora(dlogits, gflat, ghead)
    pairs = [(p, st.view(gflat, n), st.view(st.gflat, n)) for n, p in zip(st.names, ps)]
    if head:
        pairs += list(zip(head, st.head_views(model, ghead), st.head_views(model, st.ghead)))
    for p, g, own in pairs:
        if not accumulate:
            p.grad = g
        elif p.grad is None:
            p.grad = own.copy_(g)
        else:
            p.grad.add_(g)
