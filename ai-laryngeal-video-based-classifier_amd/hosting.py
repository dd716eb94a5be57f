"""Host-side scaffolding the model classes share around their kernels.

ParamStore: the fp32 master parameters under their checkpoint names, state_dict / load_state_dict, the
weights version and the "is the cached pack still valid" check (all five families).
FusedVideoModel: what the four fused inference models (ViViT, TimeSformer, Swin3D, ResNet3D) add to it: the
workspace cache, the batch split over HIP streams (vclip_amd.streams.run_split) and graph replay
(streams.GraphReplay).  A family provides _check_input, _pack, _workspace and _forward_part, and may
override _graph_knobs, _graph_keep, _clean_state_dict.  The explain paths' shared part is
vclip_amd.explaining.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch

from . import streams
from .explaining import cached_explain


def round_up(x, m):
    return (x + m - 1) // m * m


class ParamStore(torch.nn.Module):
    def _init_params(self, shapes, frozen=lambda name: False):
        """One zero Parameter per `shapes` entry (keyed name with "." -> "__": ParameterDict takes no dots),
        without gradient where frozen(name)."""
        self._names = list(shapes)
        self.params = torch.nn.ParameterDict()
        for n, s in shapes.items():
            self.params[n.replace(".", "__")] = torch.nn.Parameter(torch.zeros(s), requires_grad=not frozen(n))
        self._packed = None

    def P(self, name):
        return self.params[name.replace(".", "__")]

    def _param_list(self):
        return [self.P(n) for n in self._names]

    def _weights_version(self):
        from . import vivit_train
        # MASTER_EPOCH: the fused AdamW updates in place without bumping _version
        return (vivit_train.MASTER_EPOCH[0], sum(p._version for p in self.params.values()))

    def state_dict(self, *a, **k):  # checkpoint key names, like the reference's models
        return OrderedDict((n, self.P(n).detach()) for n in self._names)

    def _clean_state_dict(self, sd):
        """The checkpoint's entries under this model's names (default: a DataParallel `module.` prefix stripped)"""
        return {k[len("module."):] if k.startswith("module.") else k: v for k, v in sd.items()}

    def _weights_replaced(self):
        self._packed = None

    def load_state_dict(self, sd, strict: bool = True):
        sd = self._clean_state_dict(sd)
        missing = [n for n in self._names if n not in sd]
        unexpected = [k for k in sd if k not in self._names]
        if strict and (missing or unexpected):
            raise KeyError(f"load_state_dict: missing={missing[:5]} unexpected={unexpected[:5]}")
        with torch.no_grad():
            for n in self._names:
                if n in sd:
                    v = sd[n]
                    v = torch.as_tensor(np.asarray(v)) if not isinstance(v, torch.Tensor) else v
                    self.P(n).copy_(v.reshape(self.P(n).shape))
        self._weights_replaced()
        return missing, unexpected

    def _cached_pack(self, device, extra=()):
        """self._packed while it was built for `device`, the current weights version and `extra`, else None"""
        pk = self._packed
        if (pk is not None and pk["device"] == device and pk["version"] == self._weights_version()
                and pk.get("extra", ()) == extra):
            return pk
        return None


class FusedVideoModel(ParamStore):
    def __init__(self, shapes, num_labels: int, frozen=lambda name: False):
        super().__init__()
        self._init_params(shapes, frozen)
        self._num_labels = num_labels
        self.concurrent_streams = None  # None / 1: one stream; n > 1: the inference batch split over n HIP streams
        self.split_sizes = None  # clips per stream part (A/B hook; must sum to the batch): None = as even as possible
        # HIP stream priority per part (lower is higher) of the eager forward's part streams, an A/B hook;
        # None: the stream set streams.part_streams timed fastest on the first call.  Under graph replay
        # the part graphs run on the set streams.GraphReplay._tune timed fastest; profiles/r06_hwq.txt
        self.stream_priorities = None
        # True: the inference forward is captured once per input / configuration into a hipGraph and
        # replayed (streams.GraphReplay); bit-identical logits
        self.graph_replay = False
        self.kernel_events = None  # HIP events around kernel launches (bench.py); set: no graph replay
        self._graphs = streams.GraphReplay()
        self._streams = None
        self._split_out = {}  # the split forward's logits per (B, device)
        self._ws = {}
        self._ws_used = []
        self._explain_ws = {}  # explain()'s own buffers: not in _ws, which captured graphs hold on to
        self.last_streams = 1
        self.last_split = None  # clips per part of the latest forward

    def _drop_device_state(self):
        """Everything that lives on, or addresses, the device the parameters just left"""
        self._packed = None
        self._ws, self._ws_used, self._split_out, self._explain_ws = {}, [], {}, {}
        self._streams = None
        self._graphs.clear()

    def _cached_workspace(self, key, build, limit: int):
        """self._ws[key], made by build() on first use; the cache is emptied when it holds `limit` entries
        (graphs keep theirs alive).  _ws_used lists, once each, the workspaces the running forward addresses."""
        ws = self._ws.get(key)
        if ws is None:
            if len(self._ws) >= limit:
                self._ws = {}
            ws = self._ws[key] = build()
        if not any(w is ws for w in self._ws_used):
            self._ws_used.append(ws)
        return ws

    # explain's buffers (self._explain_ws, or a cache of the family's own): cache[key], built on first use, the cache
    # emptied first when it holds `limit` entries
    _cached_explain = staticmethod(cached_explain)

    # ---- the family's part ------------------------------------------------------------------
    def _check_input(self, x):
        raise NotImplementedError

    def _pack(self, device):
        raise NotImplementedError

    def _forward_part(self, x, part: int, out=None, **kw):
        raise NotImplementedError

    def _prepare(self, x):
        """The state every part reads, built on the caller's stream before the fork (streams.run_split)"""
        self._pack(x.device)

    def _part_kwargs(self) -> dict:
        return {}

    def _split_options(self, B: int, ns: int) -> dict:
        """run_split's `sizes` / `key_extra`"""
        return dict(sizes=self.split_sizes)

    def _graph_knobs(self):
        """Whatever selects kernels beyond _graph_key's own entries"""
        return ()

    def _graph_keep(self):
        return (self._packed, tuple(self._ws_used))

    # ---- forward ----------------------------------------------------------------------------
    def _graph_key(self, x):
        return (x.data_ptr(), tuple(x.shape), tuple(x.stride()), x.dtype, self.concurrent_streams,
                None if self.split_sizes is None else tuple(self.split_sizes), str(x.device),
                self._weights_version()) + tuple(self._graph_knobs())

    @torch.no_grad()
    def forward_logits(self, x: torch.Tensor) -> torch.Tensor:
        """logits f32 [B, labels] (a buffer of the model, overwritten by the next call).  `concurrent_streams =
        n > 1` splits the batch over n HIP streams, each part with its own workspace; `graph_replay` replays the
        forward from a captured hipGraph.  Logits are bit-identical either way (every kernel is batch-invariant)."""
        self._check_input(x)
        if (self.graph_replay and self.kernel_events is None and not streams.serial()
                and not torch.cuda.is_current_stream_capturing()):
            return self._graphs.run(self._graph_key(x), x, self._forward_eager, keep=self._graph_keep)
        return self._forward_eager(x)

    def _forward_eager(self, x: torch.Tensor) -> torch.Tensor:
        self._ws_used = []  # the workspaces this forward addresses (a captured graph keeps exactly these)
        B = x.shape[0]
        ns = max(1, min(int(self.concurrent_streams or 1), B))
        self.last_streams = ns
        if ns == 1:
            self.last_split = [B]
            return self._forward_part(x, 0, **self._part_kwargs())
        return streams.run_split(self, x, ns, self._forward_part, self._num_labels, prepare=lambda: self._prepare(x),
                                 **self._split_options(B, ns), **self._part_kwargs())
