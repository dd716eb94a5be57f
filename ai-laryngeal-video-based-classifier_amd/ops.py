"""torch-tensor front end of the libvclip.so kernels.

Each function validates shapes/dtypes/devices on the host (a kernel is never launched
on operands whose shape it does not support), then calls the C-ABI with raw device
pointers and torch's current HIP stream, so the work orders correctly with torch ops
and is captured by torch.cuda graphs.  No CPU fallback exists: CPU tensors raise.
"""
from __future__ import annotations

import torch

from . import _lib

EPI = {"bias": 0, "bias_gelu_tanh": 1, "bias_gelu_erf": 2, "bias_resid_f32": 3, "embed_f32": 4, "bias_f32": 5,
       "bias_relu": 6, "bias_resid_relu": 7, "bias_add_f32": 8, "bias_gelu_tanh_save": 9, "dgelu_tanh": 10}
GATHER_KIND = {"u8": 0, "f32": 1, "bf16": 2}


def _dev(*ts):
    for t in ts:
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise _lib.VclipError("vclip ops need CUDA(HIP) tensors; there is no CPU path")


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _p(t):
    return t.data_ptr()


def _need(cond, msg):
    if not cond:
        raise _lib.VclipError(msg)


def frame_gather(frames: torch.Tensor, idx: torch.Tensor, kind: str = "f32", scale: float = 1.0 / 63.75,
                 shift: float = -3.0, out: torch.Tensor | None = None) -> torch.Tensor:
    """frames u8 [N,F,H,W,C], idx int64 [N,T] -> u8 [N,T,H,W,C] or f32/bf16 [N,T,C,H,W]."""
    _dev(frames, idx)
    _need(frames.dtype == torch.uint8 and frames.dim() == 5 and frames.is_contiguous(), "frames: u8 [N,F,H,W,C]")
    _need(idx.dtype == torch.int64 and idx.dim() == 2 and idx.is_contiguous() and idx.shape[0] == frames.shape[0],
          "idx: int64 [N,T]")
    N, F, H, W, C = frames.shape
    T = idx.shape[1]
    if kind == "u8":
        shape, dt = (N, T, H, W, C), torch.uint8
    else:
        shape, dt = (N, T, C, H, W), (torch.float32 if kind == "f32" else torch.bfloat16)
    if out is None:
        out = torch.empty(shape, dtype=dt, device=frames.device)
    _need(tuple(out.shape) == shape and out.dtype == dt and out.is_contiguous(), "frame_gather: bad out")
    _lib.call("vc_frame_gather", _p(frames), N, F, H, W, C, _p(idx), T, GATHER_KIND[kind], scale, shift, _p(out),
              _stream(frames))
    return out


TOKEN_ORDER = {"time_major": 0, "patch_major": 1}
VIDEO_LAYOUT = {"btchw": 0, "bcthw": 1}
# 16-bit operand types (include/vclip.h VC_ELEM_*): bf16 everywhere; fp16 for the inference forward
H16 = (torch.bfloat16, torch.float16)
ELEM_F16 = 1
ELEM_BF16 = 0


def tubelet_im2col(pix: torch.Tensor, tubelet, out: torch.Tensor, order: str = "time_major",
                   layout: str = "btchw") -> torch.Tensor:
    """pix f32 [B,T,C,H,W] (layout "btchw") or [B,C,T,H,W] ("bcthw") -> out bf16
    [>= B*nt*nh*nw, >= C*kt*kh*kw] (rows / columns beyond are untouched).
    order "time_major": token (t', hp, wp) (ViViT, Swin); "patch_major": token (hp, wp, t') (TimeSformer)."""
    _dev(pix, out)
    _need(pix.dtype == torch.float32 and pix.dim() == 5 and pix.is_contiguous(), "pixel_values: f32 5-D contiguous")
    if layout == "btchw":
        B, T, C, H, W = pix.shape
    else:
        B, C, T, H, W = pix.shape
    kt, kh, kw = tubelet
    ntok = B * (T // kt) * (H // kh) * (W // kw)
    _need(out.dtype in H16 and out.dim() == 2 and out.shape[0] >= ntok and out.shape[1] >= C * kt * kh * kw
          and out.stride(1) == 1, "im2col out: bf16 / fp16 [rows, >= C*kt*kh*kw]")
    _need(H % kh == 0 and W % kw == 0 and T % kt == 0 and kw % 4 == 0, "im2col: shape not divisible by the patch")
    if out.dtype == torch.float16:
        _lib.call("vc_patch_im2col_h16", _p(pix), B, T, C, H, W, kt, kh, kw, TOKEN_ORDER[order], VIDEO_LAYOUT[layout],
                  ELEM_F16, _p(out), out.stride(0), _stream(pix))
    else:
        _lib.call("vc_patch_im2col", _p(pix), B, T, C, H, W, kt, kh, kw, TOKEN_ORDER[order], VIDEO_LAYOUT[layout],
                  _p(out), out.stride(0), _stream(pix))
    return out


class OpRecorder:
    """HIP events around every launch an instrumented forward makes while this recorder is installed
    (`with ops.recording(rec):`), on the stream each launch runs on.  Entries (kernel, op, e0, e1,
    work, unit): `kernel` names the kernel instantiation the launch ran (GEMMs: the tile config vc_gemm
    picked and the epilogue, i.e. one rocprofv3 kernel name), `work` its algorithmic work (FLOP or
    bytes, unit "flop" / "byte") as the caller states it (real rows and channels, not the padding)."""

    def __init__(self):
        self.entries = []

    def begin(self):
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        return e0

    def end(self, e0, kernel, op, work, unit):
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.entries.append((kernel, op, e0, e1, float(work), unit))

    def summary(self, n_steps: int, step_ms: float):
        """per kernel: launches per step, mean launch ms, share of the step, achieved rate (TFLOP/s or
        GB/s of algorithmic work), the ops that ran it; sorted by share"""
        agg = {}
        for kernel, op, e0, e1, work, unit in self.entries:
            if kernel in agg and agg[kernel]["unit"] != unit:  # one kernel, launches on both sides of the ridge
                kernel = f"{kernel} [{'HBM' if unit == 'byte' else 'MFMA'}-bound launches]"
            a = agg.setdefault(kernel, {"ms": [], "work": 0.0, "unit": unit, "ops": set()})
            a["ms"].append(e0.elapsed_time(e1))
            a["work"] += work
            a["ops"].add(op)
        out = {}
        for k, a in agg.items():
            tot = sum(a["ms"])
            rate = a["work"] / (tot * 1e-3) / (1e12 if a["unit"] == "flop" else 1e9)
            out[k] = {"launches_per_step": round(len(a["ms"]) / n_steps, 2), "avg_launch_ms": round(tot / len(a["ms"]), 4),
                      "share_of_step": round(tot / n_steps / step_ms, 4), "achieved": round(rate, 1),
                      "unit": "TFLOP/s" if a["unit"] == "flop" else "GB/s", "ops": sorted(a["ops"])}
        return dict(sorted(out.items(), key=lambda kv: -kv[1]["share_of_step"]))

    def summary_ops(self, n_steps: int, step_ms: float):
        """per op label (e.g. ResNet3D's "conv_b.s3": conv_b of res stage 3): launches per step, ms per
        step, share of the step, achieved rate, the kernels that ran it; sorted by share"""
        agg = {}
        for kernel, op, e0, e1, work, unit in self.entries:
            if op in agg and agg[op]["unit"] != unit:
                op = f"{op} [{'HBM' if unit == 'byte' else 'MFMA'}-bound launches]"
            a = agg.setdefault(op, {"ms": 0.0, "n": 0, "work": 0.0, "unit": unit, "kernels": set()})
            a["ms"] += e0.elapsed_time(e1)
            a["n"] += 1
            a["work"] += work
            a["kernels"].add(kernel)
        out = {}
        for k, a in agg.items():
            rate = a["work"] / (a["ms"] * 1e-3) / (1e12 if a["unit"] == "flop" else 1e9)
            out[k] = {"launches_per_step": round(a["n"] / n_steps, 2), "ms_per_step": round(a["ms"] / n_steps, 4),
                      "share_of_step": round(a["ms"] / n_steps / step_ms, 4), "achieved": round(rate, 1),
                      "unit": "TFLOP/s" if a["unit"] == "flop" else "GB/s", "kernels": sorted(a["kernels"])}
        return dict(sorted(out.items(), key=lambda kv: -kv[1]["share_of_step"]))


_REC = [None]


class recording:
    """`with ops.recording(rec): model.forward_logits(x)`: instrumented launches append to rec."""

    def __init__(self, rec: OpRecorder):
        self.rec = rec

    def __enter__(self):
        self.prev = _REC[0]
        _REC[0] = self.rec
        return self.rec

    def __exit__(self, *exc):
        _REC[0] = self.prev


def timed(kernel: str, op: str, work: float, unit: str, fn, *args, **kw):
    """fn(*args, **kw), between HIP events when a recorder is installed (one attribute test otherwise)"""
    rec = _REC[0]
    if rec is None:
        return fn(*args, **kw)
    e0 = rec.begin()
    r = fn(*args, **kw)
    rec.end(e0, kernel, op, work, unit)
    return r


# rocprofv3 names of the GEMM kernels per tile config (csrc/gemm.hip kCfgs; E = the epilogue, ET = 0 bf16)
GEMM_KERNEL = {3: "gemm_bf16_big_kernel<{E}, {ET}>", 4: "gemm_bf16_persist_kernel<{E}, {ET}>",
               5: "gemm_bf16_kernel<128, 128, 2, 4, {E}, 2, {ET}>", 7: "gemm_bf16_kernel<64, 128, 2, 4, {E}, 2, {ET}>",
               8: "gemm_pp_kernel<{E}, {ET}>", 15: "gemm_ppd_kernel<{E}, {ET}>", 20: "conv_c_stream_kernel<{K}, {BN}>",
               21: "gemm_bf16_kernel<64, 128, 2, 4, {E}, 4, {ET}>"}


# roofline ridge of the bf16 matrix pipe against HBM (MI355X_MICROARCH.md: 2.5 PFLOP/s dense, 8 TB/s):
# a launch whose algorithmic FLOP per byte falls below it is bounded by HBM, and its table row is
# filed under its bytes (GB/s vs 8 TB/s) instead of its FLOP
RIDGE_FLOP_PER_BYTE = 2500e12 / 8e12
# bytes per output element an epilogue moves (output written, plus the residual / aux it reads)
_EPI_OUT_BYTES = {"bias": 2, "bias_gelu_tanh": 2, "bias_gelu_erf": 2, "bias_resid_f32": 8, "embed_f32": 8,
                  "bias_f32": 4, "bias_relu": 2, "bias_resid_relu": 4, "bias_add_f32": 8, "bias_gelu_tanh_save": 4,
                  "dgelu_tanh": 4}


def gemm_bytes(M: int, N: int, K: int, epilogue: str, esize: int = 2) -> float:
    """algorithmic HBM bytes of one GEMM launch: A and W read once, the epilogue's output (and residual /
    aux operand) once"""
    return float(M * K * esize + N * K * esize + M * N * _EPI_OUT_BYTES[epilogue])


def gemm_kernel_name(M, N, K, epilogue: str, out, aux=None, cfg: int = -1, f16: bool = False) -> str:
    e = EPI[epilogue]
    if cfg < 0:
        cfg = _lib.load().vc_gemm_pick(M, N, K, e, out.stride(0), aux.stride(0) if aux is not None else 0,
                                       _p(aux) if aux is not None else None)
    return GEMM_KERNEL.get(cfg, f"gemm cfg {cfg}").format(E=e, ET=1 if f16 else 0, K=K, BN=256 if K <= 128 else 128)


def gemm(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, epilogue: str, out: torch.Tensor,
         aux: torch.Tensor | None = None, group: int = 0, group_stride: int = 0, group_offset: int = 0,
         m: int | None = None, cfg: int = -1, flop: float | None = None, op: str = "gemm",
         nbytes: float | None = None) -> torch.Tensor:
    """out (+)= epilogue(a[:m] @ w.T + bias).  a bf16 [M,K], w bf16 [N,K], bias f32 [N]; or a, w (and the
    16-bit out) fp16 for the inference epilogues (bias / gelu / resid_f32 / embed_f32).  `flop` / `op`:
    the algorithmic work and op name an installed OpRecorder files this launch under (default
    2 M N K of the operand shapes); `nbytes` (default: gemm_bytes of the operand shapes, scaled by
    flop / 2 M N K) its algorithmic bytes: the launch is filed under whichever bounds it -- bytes when
    flop / bytes is below RIDGE_FLOP_PER_BYTE (or when only `nbytes` is given), FLOP otherwise."""
    rec = _REC[0]
    if rec is not None:
        M_ = a.shape[0] if m is None else m
        label = gemm_kernel_name(M_, w.shape[0], a.shape[1], epilogue, out, aux, cfg, a.dtype == torch.float16)
        e0 = rec.begin()
        _gemm(a, w, bias, epilogue, out, aux, group, group_stride, group_offset, m, cfg)
        if nbytes is not None and flop is None:
            rec.end(e0, label, op, nbytes, "byte")
        else:
            fl0 = 2.0 * M_ * w.shape[0] * a.shape[1]
            fl = fl0 if flop is None else flop
            # default bytes: the operand shapes' (scaled like the FLOP when the caller states real rows /
            # channels instead of the padded ones)
            nb = nbytes if nbytes is not None else (
                gemm_bytes(M_, w.shape[0], a.shape[1], epilogue, a.element_size()) * (fl / fl0))
            if nb is not None and fl / nb < RIDGE_FLOP_PER_BYTE:
                rec.end(e0, label, op, nb, "byte")
            else:
                rec.end(e0, label, op, fl, "flop")
        return out
    return _gemm(a, w, bias, epilogue, out, aux, group, group_stride, group_offset, m, cfg)


def _gemm(a, w, bias, epilogue, out, aux, group, group_stride, group_offset, m, cfg):
    _dev(a, w, bias, out)
    M = a.shape[0] if m is None else m
    K = a.shape[1]
    N = w.shape[0]
    _need(a.dtype in H16 and w.dtype == a.dtype and bias.dtype == torch.float32, "gemm dtypes (a, w: bf16 or fp16)")
    f16 = a.dtype == torch.float16
    _need(a.stride(1) == 1 and w.stride(1) == 1 and out.stride(-1) == 1 and w.shape[1] == K, "gemm layout")
    _need(bias.numel() == N and bias.is_contiguous(), "gemm bias")
    e = EPI[epilogue]
    _need(not f16 or e <= 4, "gemm: fp16 operands support the inference epilogues only")
    if e in (0, 1, 2, 6, 7, 9, 10):
        _need(out.dtype == a.dtype, "gemm out must have the operand type for this epilogue")
    else:
        _need(out.dtype == torch.float32, "gemm out must be f32 for this epilogue")
    if e in (7, 9, 10):
        _need(aux is not None and aux.dtype == torch.bfloat16 and aux.stride(1) == 1 and aux.shape[0] >= M and
              aux.shape[1] >= N, f"{epilogue}: aux must be bf16 [>= M, >= N]")
    if e == 8:
        _need(aux is not None and aux.dtype == torch.float32 and aux.stride(1) == 1 and aux.shape[0] >= M and
              aux.shape[1] >= N, "bias_add_f32: aux must be the f32 residual [>= M, >= N]")
    if e == 4:
        _need(aux is not None and aux.dtype == torch.float32 and aux.stride(1) == 1 and group > 0, "embed aux")
        _need((M - 1) // group * group_stride + group_offset + (M - 1) % group < out.shape[0], "embed out rows")
    else:
        _need(out.shape[0] >= M, "gemm out rows")
    _need(a.shape[0] >= M, "gemm a rows")
    aux_p = _p(aux) if aux is not None else None
    ldaux = aux.stride(0) if aux is not None else 0
    if f16:
        _lib.call("vc_gemm_h16", _p(a), a.stride(0), _p(w), w.stride(0), M, N, K, _p(bias), e, _p(out),
                  out.stride(0), aux_p, ldaux, group, group_stride, group_offset, ELEM_F16, cfg, _stream(a))
    else:
        _lib.call("vc_gemm_bf16_cfg", _p(a), a.stride(0), _p(w), w.stride(0), M, N, K, _p(bias), e, _p(out),
                  out.stride(0), aux_p, ldaux, group, group_stride, group_offset, cfg, _stream(a))
    return out


def gemm_wrap(a: torch.Tensor, ka: int, w: torch.Tensor, bias: torch.Tensor, epilogue: str, out: torch.Tensor,
              aux: torch.Tensor | None = None, group: int = 0, group_stride: int = 0, group_offset: int = 0,
              m: int | None = None, flop: float | None = None, op: str = "gemm") -> torch.Tensor:
    """vc_gemm_h16_wrap: out (+)= epilogue(A . W^T + bias) with A = a[:m, :ka] wrapping along K: W [N, K]
    with ka <= K <= 2 ka is [W1 | W2] and the product A.W1 + A.W2 (the split-operand fp16 build)."""
    _dev(a, w, bias, out)
    M = a.shape[0] if m is None else m
    N, K = w.shape
    _need(a.dtype in H16 and w.dtype == a.dtype and bias.dtype == torch.float32 and a.stride(1) == 1 and
          w.stride(1) == 1 and a.shape[1] >= ka, "gemm_wrap operands")
    e = EPI[epilogue]
    _need(e <= 4, "gemm_wrap: inference epilogues only")
    if e == 4:
        _need(aux is not None and aux.dtype == torch.float32 and group > 0, "gemm_wrap embed aux")
        _need((M - 1) // group * group_stride + group_offset + (M - 1) % group < out.shape[0], "gemm_wrap embed out rows")
    else:
        _need(out.shape[0] >= M, "gemm_wrap out rows")
    rec = _REC[0]
    e0 = rec.begin() if rec is not None else None
    _lib.call("vc_gemm_h16_wrap", _p(a), a.stride(0), ka, _p(w), w.stride(0), M, N, K, _p(bias), e, _p(out),
              out.stride(0), _p(aux) if aux is not None else None, aux.stride(0) if aux is not None else 0, group,
              group_stride, group_offset, ELEM_F16 if a.dtype == torch.float16 else 0, _stream(a))
    if rec is not None:
        rec.end(e0, f"gemm_pp_kernel<{e}, {1 if a.dtype == torch.float16 else 0}>", op,
                2.0 * M * N * K if flop is None else flop, "flop")
    return out


def patch_im2col_split(pix: torch.Tensor, tubelet, out: torch.Tensor, order: str = "time_major",
                       layout: str = "btchw") -> torch.Tensor:
    """[A_hi | A_lo] im2col (vc_patch_im2col_split_h16): out 16-bit [>= tokens, >= 2 K]."""
    _dev(pix, out)
    if layout == "btchw":
        B, T, C, H, W = pix.shape
    else:
        B, C, T, H, W = pix.shape
    kt, kh, kw = tubelet
    _need(pix.dtype == torch.float32 and pix.is_contiguous() and out.dtype in H16 and out.stride(1) == 1 and
          out.shape[1] >= 2 * C * kt * kh * kw, "patch_im2col_split")
    _lib.call("vc_patch_im2col_split_h16", _p(pix), B, T, C, H, W, kt, kh, kw, TOKEN_ORDER[order], VIDEO_LAYOUT[layout],
              ELEM_F16 if out.dtype == torch.float16 else 0, _p(out), out.stride(0), _stream(pix))
    return out


_NUM_CUS = {}


def _num_cus(dev: torch.device) -> int:
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _NUM_CUS:
        _NUM_CUS[key] = torch.cuda.get_device_properties(key).multi_processor_count
    return _NUM_CUS[key]


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, out: torch.Tensor,
              m: int | None = None) -> torch.Tensor:
    """LayerNorm of the first gamma.numel() columns of each row (x f32 -> out bf16 or fp16)."""
    _dev(x, gamma, beta, out)
    M = x.shape[0] if m is None else m
    D = gamma.numel()
    _need(x.dtype == torch.float32 and out.dtype in H16 and x.stride(1) == 1 and out.stride(1) == 1,
          "layernorm: x f32, out bf16 / fp16, unit column stride")
    _need(beta.numel() == D and x.shape[1] >= D and out.shape[1] >= D and out.shape[0] >= M and x.shape[0] >= M,
          "layernorm shapes")
    if out.dtype == torch.float16:
        _lib.call("vc_layernorm_f32_h16", _p(x), x.stride(0), M, D, _p(gamma), _p(beta), eps, ELEM_F16, _p(out),
                  out.stride(0), _stream(x))
    else:
        _lib.call("vc_layernorm_f32_bf16", _p(x), x.stride(0), M, D, _p(gamma), _p(beta), eps, _p(out), out.stride(0),
                  _stream(x))
    return out


def layernorm_f32(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, out: torch.Tensor,
                  m: int | None = None) -> torch.Tensor:
    """f32 -> f32 LayerNorm over the first gamma.numel() columns of each row."""
    _dev(x, gamma, beta, out)
    M = x.shape[0] if m is None else m
    D = gamma.numel()
    _need(x.dtype == torch.float32 and out.dtype == torch.float32 and x.stride(1) == 1 and out.stride(1) == 1,
          "layernorm_f32 dtypes")
    _need(beta.numel() == D and x.shape[1] >= D and out.shape[1] >= D and x.shape[0] >= M and out.shape[0] >= M,
          "layernorm_f32 shapes")
    _lib.call("vc_layernorm_f32", _p(x), x.stride(0), M, D, _p(gamma), _p(beta), eps, _p(out), out.stride(0), _stream(x))
    return out


LOG2E = 1.4426950408889634


def attention(qkv: torch.Tensor, B: int, S: int, H: int, scale: float, out: torch.Tensor,
              q_prescaled: bool = False) -> torch.Tensor:
    """qkv bf16 [rows, 3*H*64] (q|k|v per token row b*S+s) -> out bf16 [rows, H*64] (or fp16 -> fp16).
    q_prescaled: q already holds q * scale * log2(e) (folded into the projection)."""
    _dev(qkv, out)
    _need(qkv.dtype in H16 and out.dtype == qkv.dtype and qkv.stride(1) == 1 and out.stride(1) == 1,
          "attention dtypes/layout")
    _need(qkv.shape[1] >= 3 * H * 64 and out.shape[1] >= H * 64, "attention columns")
    # the kernel reads K/V rows up to (B-1)*S + roundup(S,64) - 1
    _need(qkv.shape[0] >= (B - 1) * S + (S + 63) // 64 * 64, "attention: qkv needs row padding to a 64-key tile")
    _need(out.shape[0] >= B * S, "attention out rows")
    if qkv.dtype == torch.float16:
        _lib.call("vc_attention_fwd_h16", _p(qkv), qkv.stride(0), B, S, H, 64, scale, int(bool(q_prescaled)), ELEM_F16,
                  _p(out), out.stride(0), _stream(qkv))
    else:
        _lib.call("vc_attention_fwd", _p(qkv), qkv.stride(0), B, S, H, 64, scale, int(bool(q_prescaled)), _p(out),
                  out.stride(0), _stream(qkv))
    return out


ATTN_SHORT_MAX_S = 256  # csrc/attention.hip SHORT_MAX_S: up to here `attention` runs the short-sequence kernel
CLS_ATTN_SPLIT = 256   # include/vclip.h VC_CLS_ATTN_SPLIT: keys per workgroup of vc_cls_attention
SKINNY_MAX_K = 4096    # include/vclip.h VC_SKINNY_MAX_K


def cls_attention_work(B: int, S: int, H: int, device) -> torch.Tensor:
    """the f32 partials buffer of cls_attention: (max, row sum, o[64]) per (clip, head, key split)"""
    return torch.zeros(B * H * ((S + CLS_ATTN_SPLIT - 1) // CLS_ATTN_SPLIT) * 66, dtype=torch.float32, device=device)


def cls_attention(qkv: torch.Tensor, B: int, S: int, H: int, work: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """The CLS query of each (clip, head) against all S keys: qkv 16-bit [>= B*S, >= 3*H*64] (q|k|v per token
    row b*S+s, q pre-scaled by scale * log2 e) -> rows b*S of out [>= (B-1)*S + 1, >= H*64], same type.  No
    row past B*S is read."""
    _dev(qkv, work, out)
    _need(qkv.dtype in H16 and out.dtype == qkv.dtype and qkv.stride(1) == 1 and out.stride(1) == 1,
          "cls_attention dtypes/layout")
    _need(qkv.shape[1] >= 3 * H * 64 and out.shape[1] >= H * 64, "cls_attention columns")
    _need(qkv.shape[0] >= B * S and out.shape[0] >= (B - 1) * S + 1, "cls_attention rows")
    _need(work.dtype == torch.float32 and work.is_contiguous(), "cls_attention work: contiguous f32")
    _lib.call("vc_cls_attention", _p(qkv), qkv.stride(0), B, S, H, 64, ELEM_F16 if qkv.dtype == torch.float16 else 0,
              _p(work), work.numel(), _p(out), out.stride(0), _stream(qkv))
    return out


def skinny_gemm_takes(K: int) -> bool:
    """whether vc_skinny_gemm takes this reduction length"""
    return K % 8 == 0 and 0 < K <= SKINNY_MAX_K


def skinny_gemm(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, epilogue: str, out: torch.Tensor,
                ln: tuple | None = None) -> torch.Tensor:
    """out[r] (+)= epilogue(a[r] @ w.T + bias) for the few rows of a (any row stride: pass a strided view,
    e.g. X[:B*S:S] for the CLS rows in place).  w 16-bit [N, K], bias f32 [N]; a [M, K] of w's type, or -- with
    ln = (gamma, beta, eps) -- f32 rows that are LayerNorm'ed (and rounded to w's type) on the way in.
    Epilogues: bias / bias_gelu_tanh / bias_gelu_erf (out of w's type) and bias_resid_f32 (f32, in place)."""
    _dev(a, w, bias, out)
    M, K = a.shape
    N = w.shape[0]
    _need(w.dtype in H16 and w.dim() == 2 and w.shape[1] == K and w.stride(1) == 1 and bias.dtype == torch.float32 and
          bias.numel() == N and bias.is_contiguous(), "skinny_gemm: w 16-bit [N, K], bias f32 [N]")
    _need(a.dim() == 2 and a.stride(1) == 1 and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] >= M and
          out.shape[1] >= N, "skinny_gemm: a [M, K], out [>= M, >= N], unit column strides")
    _need(epilogue in ("bias", "bias_gelu_tanh", "bias_gelu_erf", "bias_resid_f32"), f"skinny_gemm: epilogue {epilogue}")
    _need(out.dtype == (torch.float32 if epilogue == "bias_resid_f32" else w.dtype), "skinny_gemm out dtype")
    if ln is None:
        _need(a.dtype == w.dtype, "skinny_gemm: a must have w's type")
        g = b = None
        eps = 0.0
    else:
        g, b, eps = ln
        _dev(g, b)
        _need(a.dtype == torch.float32 and g.dtype == torch.float32 and b.dtype == torch.float32 and g.numel() == K and
              b.numel() == K and g.is_contiguous() and b.is_contiguous(), "skinny_gemm: LayerNorm prologue on f32 rows")
    _lib.call("vc_skinny_gemm", _p(a), a.stride(0), None if g is None else _p(g), None if b is None else _p(b), eps,
              _p(w), w.stride(0), M, N, K, _p(bias), EPI[epilogue], ELEM_F16 if w.dtype == torch.float16 else 0, _p(out),
              out.stride(0), _stream(a))
    return out


def spin(iters: int, device, blocks: int = 1) -> None:
    """`blocks` one-wave workgroups sleeping `iters` x s_sleep 127 each, on the current stream of `device`
    (streams.pick_streams)."""
    _lib.call("vc_spin", int(iters), int(blocks), torch.cuda.current_stream(device).cuda_stream)


def cls_init(cls: torch.Tensor, pos: torch.Tensor, x: torch.Tensor, B: int, S: int) -> torch.Tensor:
    _dev(cls, pos, x)
    D = cls.numel()
    _need(x.dtype == torch.float32 and x.shape[0] >= B * S and x.shape[1] >= D, "cls_init x")
    _lib.call("vc_cls_init", _p(cls), _p(pos), _p(x), x.stride(0), B, S, D, _stream(x))
    return x


def cls_head(x: torch.Tensor, B: int, S: int, gamma, beta, eps: float, wc: torch.Tensor, bc: torch.Tensor,
             out: torch.Tensor | None = None) -> torch.Tensor:
    _dev(x, gamma, beta, wc, bc)
    D = gamma.numel()
    nl = wc.shape[0]
    _need(wc.dtype == torch.float32 and wc.is_contiguous() and wc.shape[1] == D, "cls_head weight f32 [nl, D]")
    if out is None:
        out = torch.empty((B, nl), dtype=torch.float32, device=x.device)
    _lib.call("vc_cls_head", _p(x), x.stride(0), B, S, D, _p(gamma), _p(beta), eps, _p(wc), _p(bc), nl, _p(out),
              _stream(x))
    return out


def temporal_attention(qkv: torch.Tensor, B: int, P: int, T: int, H: int, scale: float, out: torch.Tensor,
                       q_prescaled: bool = False) -> torch.Tensor:
    """TimeSformer temporal attention on the clip layout (rows b*(1+P*T) + 1 + p*T + t):
    qkv bf16 [rows, 3*H*64] -> out bf16 [rows, H*64] (CLS rows untouched)."""
    _dev(qkv, out)
    _need(qkv.dtype == torch.bfloat16 and out.dtype == torch.bfloat16 and qkv.stride(1) == 1 and out.stride(1) == 1,
          "temporal_attention dtypes/layout")
    _need(qkv.shape[1] >= 3 * H * 64 and out.shape[1] >= H * 64, "temporal_attention columns")
    _need(qkv.shape[0] >= B * (1 + P * T) and out.shape[0] >= B * (1 + P * T), "temporal_attention rows")
    _need(T <= 32, "temporal_attention: T <= 32")
    _lib.call("vc_temporal_attention", _p(qkv), qkv.stride(0), B, P, T, H, 64, scale, int(bool(q_prescaled)), _p(out),
              out.stride(0), _stream(qkv))
    return out


DIVIDED_MODE = {"temporal_to_spatial": 0, "spatial_to_mlp": 1}


def divided_add_layernorm(x: torch.Tensor, y: torch.Tensor, B: int, P: int, T: int, gamma, beta, eps: float,
                          mode: str, h: torch.Tensor) -> torch.Tensor:
    """Residual add + LayerNorm across the TimeSformer clip / frame layouts (see include/vclip.h)."""
    _dev(x, y, gamma, beta, h)
    D = gamma.numel()
    _need(x.dtype == torch.float32 and y.dtype == torch.bfloat16 and h.dtype == torch.bfloat16, "divided_add_ln dtypes")
    _need(x.stride(1) == 1 and y.stride(1) == 1 and h.stride(1) == 1 and D % 4 == 0 and D <= 1024, "divided_add_ln")
    rows_c, rows_f = B * (1 + P * T), B * T * (1 + P)
    _need(x.shape[0] >= rows_c and x.shape[1] >= D and y.shape[1] >= D and h.shape[1] >= D, "divided_add_ln shapes")
    if mode == "temporal_to_spatial":
        _need(y.shape[0] >= rows_c and h.shape[0] >= rows_f, "divided_add_ln rows")
    else:
        _need(y.shape[0] >= rows_f and h.shape[0] >= rows_c, "divided_add_ln rows")
    _lib.call("vc_divided_add_layernorm", _p(x), x.stride(0), _p(y), y.stride(0), B, P, T, D, _p(gamma), _p(beta), eps,
              DIVIDED_MODE[mode], _p(h), h.stride(0), _stream(x))
    return h


def window_attention3d(qkv: torch.Tensor, B: int, grid, heads: int, window, shift, biasT: torch.Tensor,
                       out: torch.Tensor, lse: torch.Tensor | None = None) -> torch.Tensor:
    """Swin 3D shifted-window attention (head_dim 32) on the token layout [B][T][H][W]:
    qkv bf16 [>= B*T*H*W, >= 3*heads*32] (q pre-scaled by d^-1/2 * log2 e) -> out bf16 [rows,
    >= heads*32].  biasT: the f32 accumulator-fragment bias of swin3d.expand_bias (the bias as
    the QK^T C operand; also the train-step form with `lse`), or the fp16 operand-fragment bias
    of swin3d.expand_bias_mb (inference: bias and shift mask on the matrix pipe,
    vc_window_attention3d_mb).  See include/vclip.h."""
    _dev(qkv, biasT, out)
    T, H, W = grid
    wt, wh, ww = window
    st, sh, sw = shift
    vol = wt * wh * ww
    np_ = (vol + 63) // 64 * 64
    _need(qkv.dtype == torch.bfloat16 and out.dtype == torch.bfloat16 and qkv.stride(1) == 1 and out.stride(1) == 1,
          "window_attention3d dtypes")
    _need(biasT.dtype in (torch.float32, torch.float16) and biasT.is_contiguous() and biasT.numel() == heads * np_ * np_,
          "window_attention3d bias: f32 (swin3d.expand_bias) or fp16 (swin3d.expand_bias_mb) table of heads*np*np")
    _need(qkv.shape[0] >= B * T * H * W and out.shape[0] >= B * T * H * W, "window_attention3d rows")
    _need(qkv.shape[1] >= 3 * heads * 32 and out.shape[1] >= heads * 32, "window_attention3d columns")
    _need(T % wt == 0 and H % wh == 0 and W % ww == 0, "window_attention3d: grid must be whole windows")
    if biasT.dtype == torch.float16:
        _need(lse is None, "window_attention3d: the train-step form (lse) takes the f32 bias")
        _lib.call("vc_window_attention3d_mb", _p(qkv), qkv.stride(0), B, T, H, W, heads, 32, wt, wh, ww, st, sh, sw,
                  _p(biasT), np_, _p(out), out.stride(0), _stream(qkv))
        return out
    if lse is not None:  # train step: + base-2 log-sum-exp per (token row, head)
        _dev(lse)
        _need(lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() >= B * T * H * W * heads,
              "window_attention3d lse: f32 [rows * heads]")
        _lib.call("vc_window_attention3d_lse", _p(qkv), qkv.stride(0), B, T, H, W, heads, 32, wt, wh, ww, st, sh, sw,
                  _p(biasT), np_, _p(out), out.stride(0), _p(lse), _stream(qkv))
        return out
    _lib.call("vc_window_attention3d", _p(qkv), qkv.stride(0), B, T, H, W, heads, 32, wt, wh, ww, st, sh, sw, _p(biasT),
              np_, _p(out), out.stride(0), _stream(qkv))
    return out


def window_attention3d_bwd(qkv: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor, B: int, grid,
                           heads: int, window, shift, full_window, table: torch.Tensor, dqkv: torch.Tensor,
                           dtable_part: torch.Tensor) -> torch.Tensor:
    """Backward of window_attention3d: dqkv (bf16 rows, d q' | dk | dv) and the per-(window, head)
    bias-table gradient partials dtable_part f32 [B * nwindows, heads, ntab] (sum over dim 0)."""
    _dev(qkv, out, dout, lse, table, dqkv, dtable_part)
    T, H, W = grid
    wt, wh, ww = window
    st, sh, sw = shift
    ft, fh, fw = full_window
    ntab = (2 * ft - 1) * (2 * fh - 1) * (2 * fw - 1)
    nwin = B * (T // wt) * (H // wh) * (W // ww)
    for nm, t in (("qkv", qkv), ("out", out), ("dout", dout), ("dqkv", dqkv)):
        _need(t.dtype == torch.bfloat16 and t.stride(1) == 1 and t.shape[0] >= B * T * H * W, f"window bwd {nm}")
    _need(table.dtype == torch.float32 and table.is_contiguous() and tuple(table.shape) == (ntab, heads),
          "window bwd table: f32 [ntab, heads]")
    _need(dtable_part.dtype == torch.float32 and dtable_part.is_contiguous() and dtable_part.numel() >= nwin * heads * ntab,
          "window bwd dtable_part: f32 [B * nwindows * heads * ntab]")
    _lib.call("vc_window_attention3d_bwd", _p(qkv), qkv.stride(0), _p(out), out.stride(0), _p(dout), dout.stride(0),
              _p(lse), B, T, H, W, heads, 32, wt, wh, ww, st, sh, sw, ft, fh, fw, _p(table), _p(dqkv), dqkv.stride(0),
              _p(dtable_part), _stream(qkv))
    return dqkv


def patch_merge_layernorm(x: torch.Tensor, B: int, grid, C: int, gamma, beta, eps: float,
                          out: torch.Tensor) -> torch.Tensor:
    """x f32 [>= B*T*H*W, >= C] -> out bf16 [>= B*T*ceil(H/2)*ceil(W/2), >= 4C]."""
    _dev(x, gamma, beta, out)
    T, H, W = grid
    _need(x.dtype == torch.float32 and out.dtype == torch.bfloat16 and x.stride(1) == 1 and out.stride(1) == 1,
          "patch_merge dtypes")
    _need(gamma.numel() == 4 * C and out.shape[1] >= 4 * C and x.shape[1] >= C, "patch_merge columns")
    _need(x.shape[0] >= B * T * H * W and out.shape[0] >= B * T * ((H + 1) // 2) * ((W + 1) // 2), "patch_merge rows")
    _lib.call("vc_patch_merge_layernorm", _p(x), x.stride(0), B, T, H, W, C, _p(gamma), _p(beta), eps, _p(out),
              out.stride(0), _stream(x))
    return out


def pool_head(x: torch.Tensor, B: int, ntok: int, gamma, beta, eps: float, wc: torch.Tensor, bc: torch.Tensor,
              out: torch.Tensor | None = None, work: torch.Tensor | None = None) -> torch.Tensor:
    """logits = head(mean over each clip's ntok rows of LN(x)) (Swin3D final norm + avgpool + head)."""
    _dev(x, gamma, beta, wc, bc)
    D = gamma.numel()
    nl = wc.shape[0]
    _need(wc.dtype == torch.float32 and wc.is_contiguous() and wc.shape[1] == D and x.shape[0] >= B * ntok,
          "pool_head shapes")
    if out is None:
        out = torch.empty((B, nl), dtype=torch.float32, device=x.device)
    if work is None or work.numel() < B * 64 * D:
        work = torch.empty(B * 64 * D, dtype=torch.float32, device=x.device)
    _lib.call("vc_pool_head", _p(x), x.stride(0), B, ntok, D, _p(gamma), _p(beta), eps, _p(wc), _p(bc), nl, _p(out),
              _p(work), _stream(x))
    return out


CONV_IN = {"ncthw_f32": 0, "cl_bf16": 1}


def conv_out_size(size, k, s, p):
    return tuple((n + 2 * pp - kk) // ss + 1 for n, kk, ss, pp in zip(size, k, s, p))


def conv3d_im2col(x: torch.Tensor, kind: str, B: int, grid, C: int, kernel, stride, pad, out: torch.Tensor) -> torch.Tensor:
    """im2col of a 3D convolution: x f32 [B,C,T,H,W] (kind "ncthw_f32") or channels-last bf16 rows
    [>= B*T*H*W, >= C] ("cl_bf16") -> out bf16 [>= B*To*Ho*Wo, >= kvol*C]."""
    import ctypes
    _dev(x, out)
    T, H, W = grid
    To, Ho, Wo = conv_out_size(grid, kernel, stride, pad)
    kvol = kernel[0] * kernel[1] * kernel[2]
    _need(out.dtype == torch.bfloat16 and out.stride(1) == 1 and out.shape[0] >= B * To * Ho * Wo and
          out.shape[1] >= kvol * C, "conv3d_im2col out")
    if kind == "ncthw_f32":
        _need(x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (B, C, T, H, W), "conv3d_im2col x")
        ldx = 0
    else:
        _need(x.dtype == torch.bfloat16 and x.stride(1) == 1 and x.shape[0] >= B * T * H * W and x.shape[1] >= C,
              "conv3d_im2col x")
        ldx = x.stride(0)
    k, s, p = ((ctypes.c_int * 3)(*v) for v in (kernel, stride, pad))
    _lib.call("vc_conv3d_im2col", _p(x), ldx, CONV_IN[kind], B, T, H, W, C, ctypes.addressof(k), ctypes.addressof(s),
              ctypes.addressof(p), _p(out), out.stride(0), _stream(x))
    return out


_ZERO_ROW = {}


def zero_row(device) -> torch.Tensor:
    """The shared 64-element zero bf16 row the implicit convolutions read for padding taps (one per
    device).  Created once, on the caller's stream, which is then waited for: a split forward's parts
    read it from side streams that are ordered only after the caller's stream, so a zero-fill queued on
    one part's stream could still be pending when another part's first conv reads it."""
    z = _ZERO_ROW.get(device)
    if z is None:
        z = torch.zeros(64, dtype=torch.bfloat16, device=device)
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream(device).synchronize()
        _ZERO_ROW[device] = z
    return z


def conv3d_gemm(x: torch.Tensor, B: int, grid, C: int, kernel, stride, pad, w: torch.Tensor, bias: torch.Tensor,
                epilogue: str, out: torch.Tensor, aux: torch.Tensor | None = None, flop: float | None = None,
                op: str = "conv", n: int | None = None, ring: int = 0, tile: int = 0) -> torch.Tensor:
    """Implicit-GEMM Conv3d (vc_conv3d_gemm_bf16): x channels-last bf16 rows [>= B*T*H*W, >= C],
    w bf16 [>= N, >= kvol*C] (columns (kt, kh, kw, c)), out bf16 [>= roundup(B*To*Ho*Wo, 128), >= N]
    (256-row multiples when N % 128 != 0: 256 x 64 tiles); N = n (a multiple of 64) or w's rows."""
    import ctypes
    _dev(x, w, bias, out)
    T, H, W = grid
    To, Ho, Wo = conv_out_size(grid, kernel, stride, pad)
    kvol = kernel[0] * kernel[1] * kernel[2]
    M = B * To * Ho * Wo
    N = w.shape[0] if n is None else n
    rt = 128 if N % 128 == 0 else 256
    _need(x.dtype == torch.bfloat16 and x.stride(1) == 1 and x.shape[0] >= B * T * H * W and x.shape[1] >= C,
          "conv3d_gemm x")
    _need(w.dtype == torch.bfloat16 and w.stride(1) == 1 and w.shape[1] >= kvol * C and w.shape[0] >= N and
          bias.numel() >= N and bias.dtype == torch.float32, "conv3d_gemm weights")
    _need(out.dtype == torch.bfloat16 and out.stride(1) == 1 and out.shape[0] >= (M + rt - 1) // rt * rt and
          out.shape[1] >= N, "conv3d_gemm out rows (a multiple of the tile height)")
    e = EPI[epilogue]
    if e == 7:
        # the tile epilogue reads the residual for every row of the padded tile
        _need(aux is not None and aux.dtype == torch.bfloat16 and aux.stride(1) == 1 and
              aux.shape[0] >= (M + rt - 1) // rt * rt and aux.shape[1] >= N,
              "conv3d_gemm residual (rows up to the tile-height multiple of the output rows)")
    zrow = zero_row(x.device)
    k, s, p = ((ctypes.c_int * 3)(*v) for v in (kernel, stride, pad))
    rec = _REC[0]
    if rec is not None:
        # the label first: nothing but the launch may sit between the two events (a first
        # get_device_properties inside them once timed as an 8-ms launch)
        tl = "256, 64, 8, 1"
        if rt == 128:  # 64 x 128 tiles when the 128 x 128 grid has fewer tiles than CUs (csrc/gemm.hip)
            small = tile == 1 or (tile == 0 and ((M + 127) // 128) * (N // 128) < _num_cus(x.device) and e in (0, 6))
            tl = "64, 128, 2, 4" if small else "128, 128, 2, 4"
        nt = (((M + 127) // 128) * (N // 128) if tl == "128, 128, 2, 4" else ((M + 63) // 64) * (N // 128)
              if tl == "64, 128, 2, 4" else ((M + 255) // 256) * (N // 64))
        cus = _num_cus(x.device)  # csrc/gemm.hip pick_ring (128 x 128: 3-deep only within one round of CUs)
        st = ring if ring else (3 if (nt <= cus if tl == "128, 128, 2, 4" else nt < 2 * cus) else 2)
        if st == 4 and rt != 128:
            st = 3
        label = f"conv_gemm_kernel<{tl}, {e}, {st}, 0>"
    e0 = rec.begin() if rec is not None else None
    _lib.call("vc_conv3d_gemm_bf16_cfg", _p(x), x.stride(0), B, T, H, W, C, ctypes.addressof(k), ctypes.addressof(s),
              ctypes.addressof(p), _p(zrow), _p(w), w.stride(0), N, _p(bias), e, _p(out), out.stride(0),
              _p(aux) if aux is not None else None, aux.stride(0) if aux is not None else 0, ring, tile, _stream(x))
    if rec is not None:
        rec.end(e0, label, op, 2.0 * M * N * kvol * C if flop is None else flop, "flop")
    return out


def conv3d_stem_pack(x: torch.Tensor, pad, out: torch.Tensor) -> torch.Tensor:
    """f32 clip [B, C<=4, T, H, W] -> zero-padded channels-last bf16 [B, T+2pt, H+2ph, W+2pw, 4] (out, any
    shape with that many contiguous elements)."""
    import ctypes
    _dev(x, out)
    B, C, T, H, W = x.shape
    _need(x.dtype == torch.float32 and x.is_contiguous() and C <= 4, "conv3d_stem_pack x")
    _need(out.dtype == torch.bfloat16 and out.is_contiguous() and
          out.numel() >= B * (T + 2 * pad[0]) * (H + 2 * pad[1]) * (W + 2 * pad[2]) * 4, "conv3d_stem_pack out")
    p = (ctypes.c_int * 3)(*pad)
    _lib.call("vc_conv3d_stem_pack", _p(x), B, C, T, H, W, ctypes.addressof(p), _p(out), _stream(x))
    return out


def conv3d_stem_gemm(xp: torch.Tensor, B: int, grid, kernel, stride, pad, w: torch.Tensor, bias: torch.Tensor,
                     epilogue: str, out: torch.Tensor, flop: float | None = None, op: str = "stem",
                     n: int | None = None) -> torch.Tensor:
    """The stem Conv3d as an implicit GEMM over conv3d_stem_pack's padded clip (vc_conv3d_stem_gemm_bf16);
    w bf16 [N, >= 64 * ceil(kt*kh/2)] in the segment column order, out bf16 [>= roundup(M, 128), >= N]."""
    import ctypes
    _dev(xp, w, bias, out)
    T, H, W = grid
    To, Ho, Wo = conv_out_size(grid, kernel, stride, pad)
    M = B * To * Ho * Wo
    N = w.shape[0] if n is None else n
    rt = 128 if N % 128 == 0 else 256
    K = 64 * ((kernel[0] * kernel[1] + 1) // 2)
    _need(xp.dtype == torch.bfloat16 and xp.is_contiguous(), "conv3d_stem_gemm xp")
    _need(w.dtype == torch.bfloat16 and w.stride(1) == 1 and w.shape[1] >= K and w.shape[0] >= N and
          bias.numel() >= N and bias.dtype == torch.float32, "conv3d_stem_gemm weights")
    _need(out.dtype == torch.bfloat16 and out.stride(1) == 1 and out.shape[0] >= (M + rt - 1) // rt * rt and
          out.shape[1] >= N, "conv3d_stem_gemm out")
    # each (kt, kh) tap row is read as 8 pixels x 4 channels from a 16-B aligned start: an even padded width,
    # and the last output's window (8 pixels from 2 wo) inside the packed clip
    Tp, Hp, Wp = T + 2 * pad[0], H + 2 * pad[1], W + 2 * pad[2]
    _need(Wp % 2 == 0 and stride[2] % 2 == 0, "conv3d_stem_gemm: the padded width must be even (16-B aligned "
          "8-pixel reads; the forward takes the im2col stem otherwise)")
    last = ((((B - 1) * Tp + (To - 1) * stride[0] + kernel[0] - 1) * Hp + (Ho - 1) * stride[1] + kernel[1] - 1) * Wp
            + (Wo - 1) * stride[2] + 8) * 4
    _need(xp.numel() >= last, "conv3d_stem_gemm: the packed clip ends before the last window's 8-pixel read")
    zrow = zero_row(xp.device)
    k, s, p = ((ctypes.c_int * 3)(*v) for v in (kernel, stride, pad))
    rec = _REC[0]
    e0 = rec.begin() if rec is not None else None
    e = EPI[epilogue]
    _lib.call("vc_conv3d_stem_gemm_bf16", _p(xp), B, T, H, W, ctypes.addressof(k), ctypes.addressof(s),
              ctypes.addressof(p), _p(zrow), _p(w), w.stride(0), N, _p(bias), e, _p(out), out.stride(0),
              _stream(xp))
    if rec is not None:
        tile = "128, 128, 2, 4" if rt == 128 else "256, 64, 8, 1"
        rec.end(e0, f"conv_gemm_kernel<{tile}, {e}, 2, 1>", op, 2.0 * M * N * K if flop is None else flop, "flop")
    return out


def maxpool3d(x: torch.Tensor, B: int, grid, C: int, kernel, stride, pad, out: torch.Tensor) -> torch.Tensor:
    import ctypes
    _dev(x, out)
    To, Ho, Wo = conv_out_size(grid, kernel, stride, pad)
    T, H, W = grid
    _need(x.dtype == torch.bfloat16 and out.dtype == torch.bfloat16 and x.shape[0] >= B * T * H * W and
          out.shape[0] >= B * To * Ho * Wo and x.shape[1] >= C and out.shape[1] >= C, "maxpool3d shapes")
    k, s, p = ((ctypes.c_int * 3)(*v) for v in (kernel, stride, pad))
    _lib.call("vc_maxpool3d", _p(x), x.stride(0), B, T, H, W, C, ctypes.addressof(k), ctypes.addressof(s),
              ctypes.addressof(p), _p(out), out.stride(0), _stream(x))
    return out


def avgpool_head(x: torch.Tensor, B: int, grid, C: int, pool_kernel, wc: torch.Tensor, bc: torch.Tensor,
                 work: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    import ctypes
    _dev(x, wc, bc, work, out)
    T, H, W = grid
    nl = wc.shape[0]
    _need(x.dtype == torch.bfloat16 and x.shape[0] >= B * T * H * W and x.shape[1] >= C, "avgpool_head x")
    _need(wc.dtype == torch.float32 and wc.is_contiguous() and wc.shape[1] == C and work.numel() >= B * C * 33 and
          out.shape == (B, nl), "avgpool_head shapes")
    pk = (ctypes.c_int * 3)(*pool_kernel)
    _lib.call("vc_avgpool_head", _p(x), x.stride(0), B, T, H, W, C, ctypes.addressof(pk), _p(wc), _p(bc), nl,
              _p(work), _p(out), _stream(x))
    return out


# ---- ResNet3D saliency: Grad-CAM / HiResCAM (csrc/cam.hip) ------------------------------------

CAM_MODE = {"gradcam": 0, "hirescam": 1}


def _cl_rows(t: torch.Tensor, rows: int, C: int, what: str, dtypes=(torch.bfloat16,)):
    """t: channels-last rows [>= rows, >= C] of one of `dtypes`, unit column stride, 16-B aligned rows"""
    _need(t.dim() == 2 and t.dtype in dtypes and t.stride(1) == 1 and t.shape[0] >= rows and t.shape[1] >= C and
          t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0, f"{what}: rows [>= {rows}, >= {C}], 16-B aligned, row stride % 8")


def col2im_cl(da: torch.Tensor, B: int, grid, C: int, kernel, stride, pad, dx: torch.Tensor) -> torch.Tensor:
    """The adjoint of conv3d_im2col on channels-last rows (vc_col2im_cl): da bf16 [>= B*To*Ho*Wo, >= kvol*C]
    (columns (kt, kh, kw, c)) -> dx f32 [>= B*T*H*W, >= C] over the input grid (T, H, W); fixed gather order."""
    import ctypes
    _dev(da, dx)
    T, H, W = grid
    To, Ho, Wo = conv_out_size(grid, kernel, stride, pad)
    kvol = kernel[0] * kernel[1] * kernel[2]
    _need(all(0 <= p < k and s > 0 for k, s, p in zip(kernel, stride, pad)) and min(To, Ho, Wo) > 0, "col2im_cl geometry")
    _need(da.dtype == torch.bfloat16 and da.dim() == 2 and da.stride(1) == 1 and da.shape[0] >= B * To * Ho * Wo and
          da.shape[1] >= kvol * C, "col2im_cl da: bf16 [>= B*To*Ho*Wo, >= kvol*C]")
    _need(dx.dtype == torch.float32 and dx.dim() == 2 and dx.stride(1) == 1 and dx.shape[0] >= B * T * H * W and
          dx.shape[1] >= C, "col2im_cl dx: f32 [>= B*T*H*W, >= C]")
    k, s, p = ((ctypes.c_int * 3)(*v) for v in (kernel, stride, pad))
    _lib.call("vc_col2im_cl", _p(da), da.stride(0), B, T, H, W, C, ctypes.addressof(k), ctypes.addressof(s),
              ctypes.addressof(p), _p(dx), dx.stride(0), _stream(da))
    return dx


def cam_seed(wc: torch.Tensor, target: torch.Tensor, B: int, grid, C: int, pool_kernel, out: torch.Tensor) -> torch.Tensor:
    """d logit[target[b]] / d x of the head AvgPool3d(pool_kernel, stride 1) -> Linear(wc f32 [labels, C]) -> global
    mean (vc_cam_seed): out bf16 rows [>= B*T*H*W, >= C], out[row, c] = cnt(t, h, w) / (npos * pt*ph*pw) *
    wc[target[b], c].  target: int32 [B] on the device, every entry in [0, labels) (the caller's check)."""
    import ctypes
    _dev(wc, target, out)
    T, H, W = grid
    _need(wc.dtype == torch.float32 and wc.dim() == 2 and wc.is_contiguous() and wc.shape[1] == C and C % 8 == 0,
          "cam_seed wc: contiguous f32 [labels, C], C % 8 == 0")
    _need(target.dtype == torch.int32 and target.is_contiguous() and tuple(target.shape) == (B,), "cam_seed target: int32 [B]")
    _need(all(0 < k <= n for k, n in zip(pool_kernel, grid)), "cam_seed: the pool must fit the grid")
    _cl_rows(out, B * T * H * W, C, "cam_seed out")
    pk = (ctypes.c_int * 3)(*pool_kernel)
    _lib.call("vc_cam_seed", _p(wc), wc.shape[0], _p(target), B, T, H, W, C, ctypes.addressof(pk), _p(out), out.stride(0),
              _stream(out))
    return out


def relu_bwd(y: torch.Tensor | None, d1: torch.Tensor, M: int, C: int, out: torch.Tensor,
             d2: torch.Tensor | None = None) -> torch.Tensor:
    """out[:M, :C] = (y is None or y > 0) ? d1 + (d2 or 0) : 0 as bf16 (vc_relu_bwd).  d1, d2: f32 or bf16 rows
    [>= M, >= C]; y: bf16 activations.  A ReLU mask, the join of two gradients and the cast for the next GEMM."""
    g16 = (torch.bfloat16, torch.float32)
    ts = [t for t in (y, d1, d2, out) if t is not None]
    _dev(*ts)
    _need(C % 8 == 0 and M > 0, "relu_bwd: C % 8 == 0")
    _cl_rows(d1, M, C, "relu_bwd d1", g16)
    _cl_rows(out, M, C, "relu_bwd out")
    if y is not None:
        _cl_rows(y, M, C, "relu_bwd y")
    if d2 is not None:
        _cl_rows(d2, M, C, "relu_bwd d2", g16)
    _lib.call("vc_relu_bwd", _p(y) if y is not None else None, y.stride(0) if y is not None else 0, _p(d1),
              int(d1.dtype == torch.float32), d1.stride(0), _p(d2) if d2 is not None else None,
              int(d2 is not None and d2.dtype == torch.float32), d2.stride(0) if d2 is not None else 0, M, C, _p(out),
              out.stride(0), _stream(out))
    return out


def cam_weights_work(B: int, C: int, device) -> torch.Tensor:
    """the f32 partial-sum buffer of cam_weights: 32 fixed-order partials per (clip, channel)"""
    return torch.zeros(B * 32 * C, dtype=torch.float32, device=device)


def cam_weights(g: torch.Tensor, B: int, N: int, C: int, work: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """Grad-CAM's channel weights (vc_cam_weights): out f32 [B, C] = the mean over clip b's N rows of g bf16
    [>= B*N, >= C]; work from cam_weights_work."""
    _dev(g, work, out)
    _need(C % 8 == 0, "cam_weights: C % 8 == 0")
    _cl_rows(g, B * N, C, "cam_weights g")
    _need(work.dtype == torch.float32 and work.is_contiguous() and work.numel() >= B * 32 * C,
          "cam_weights work: contiguous f32 [B * 32 * C]")
    _need(out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, C), "cam_weights out: f32 [B, C]")
    _lib.call("vc_cam_weights", _p(g), g.stride(0), B, N, C, _p(work), work.numel(), _p(out), _stream(g))
    return out


def cam_map(mode: str, x: torch.Tensor, w: torch.Tensor, B: int, N: int, C: int, out: torch.Tensor) -> torch.Tensor:
    """The signed class-activation map (vc_cam_map): out f32 [B*N]; x bf16 activations [>= B*N, >= C].  mode
    "gradcam": out[row] = sum_c w[b, c] x[row, c] with w f32 [B, C] (cam_weights); "hirescam": sum_c w[row, c] x[row, c]
    with w the bf16 gradient rows."""
    _dev(x, w, out)
    _need(mode in CAM_MODE, f"cam_map: mode must be one of {tuple(CAM_MODE)}")
    _need(C % 8 == 0, "cam_map: C % 8 == 0")
    _cl_rows(x, B * N, C, "cam_map x")
    _need(out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * N, "cam_map out: f32 [B*N]")
    if mode == "hirescam":
        _cl_rows(w, B * N, C, "cam_map hirescam w")
        _lib.call("vc_cam_map", 1, _p(x), x.stride(0), _p(w), w.stride(0), None, B, N, C, _p(out), _stream(x))
    else:
        _need(w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape) == (B, C), "cam_map gradcam w: f32 [B, C]")
        _lib.call("vc_cam_map", 0, _p(x), x.stride(0), None, 0, _p(w), B, N, C, _p(out), _stream(x))
    return out


def frame_cam(x: torch.Tensor, g: torch.Tensor, N: int, P: int, C: int, out: torch.Tensor,
              frame_rel: torch.Tensor) -> torch.Tensor:
    """The class-activation map at the input of a per-frame average pool (vc_frame_cam): out f32 [N*P], out[n*P + p] =
    (1/P) sum_c g[n, c] x[n*P + p, c] with x bf16 rows [>= N*P, >= C] and g f32 [>= N, >= C] the gradient with respect
    to frame n's pooled features; frame_rel f32 [N] = the sum of frame n's P entries in order.  With P = 1 and x the
    pooled features both are the signed gradient x input.  C % 8 == 0, C <= 4096."""
    _dev(x, g, out, frame_rel)
    _need(N >= 1 and P >= 1, "frame_cam: N and P must be >= 1")
    _need(C % 8 == 0 and 0 < C <= 4096, "frame_cam: C % 8 == 0, C <= 4096")
    _cl_rows(x, N * P, C, "frame_cam x")
    _cl_rows(g, N, C, "frame_cam g", (torch.float32,))
    _need(out.dtype == torch.float32 and out.is_contiguous() and out.numel() == N * P, "frame_cam out: f32 [N*P]")
    _need(frame_rel.dtype == torch.float32 and frame_rel.is_contiguous() and frame_rel.numel() == N,
          "frame_cam frame_rel: f32 [N]")
    timed("frame_cam_kernel", "cam.frame_map", N * P * C * 2 + N * C * 4, "byte", _lib.call, "vc_frame_cam", _p(x),
          x.stride(0), _p(g), g.stride(0), N, P, C, _p(out), _p(frame_rel), _stream(x))
    return out


def frame_avgpool_bwd(g: torch.Tensor, N: int, P: int, C: int, out: torch.Tensor) -> torch.Tensor:
    """The adjoint of frame_avgpool (vc_frame_avgpool_bwd): out bf16 rows [>= N*P, >= C], out[n*P + p, c] =
    bf16(g[n, c] / P) for g f32 [>= N, >= C]."""
    _dev(g, out)
    _need(N >= 1 and P >= 1, "frame_avgpool_bwd: N and P must be >= 1")
    _need(C % 8 == 0 and C > 0, "frame_avgpool_bwd: C % 8 == 0")
    _cl_rows(g, N, C, "frame_avgpool_bwd g", (torch.float32,))
    _cl_rows(out, N * P, C, "frame_avgpool_bwd out")
    timed("frame_avgpool_bwd_kernel", "cam.frame_seed", N * P * C * 2 + N * C * 4, "byte", _lib.call,
          "vc_frame_avgpool_bwd", _p(g), g.stride(0), N, P, C, _p(out), out.stride(0), _stream(g))
    return out


# ---- train step -----------------------------------------------------------

def attention_fwd_lse(qkv: torch.Tensor, B: int, S: int, H: int, out: torch.Tensor, lse: torch.Tensor,
                      scale: float = 0.125, q_prescaled: bool = True) -> torch.Tensor:
    """vc_attention_fwd that also stores the base-2 log-sum-exp lse f32 [B*H*S].
    The padding rows of qkv (past B*S, up to the last clip's 64-key tile) must hold finite values: they are
    read and multiplied by zero, so a NaN or Inf there reaches valid rows."""
    _dev(qkv, out, lse)
    _need(lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() >= B * H * S, "lse: f32 [B*H*S]")
    _need(qkv.dtype == torch.bfloat16 and out.dtype == torch.bfloat16 and qkv.stride(1) == 1 and out.stride(1) == 1,
          "attention dtypes/layout")
    _need(qkv.shape[1] >= 3 * H * 64 and out.shape[1] >= H * 64, "attention columns")
    _need(qkv.shape[0] >= (B - 1) * S + (S + 63) // 64 * 64, "attention: qkv needs row padding to a 64-key tile")
    _need(out.shape[0] >= B * S, "attention out rows")
    _lib.call("vc_attention_fwd_lse", _p(qkv), qkv.stride(0), B, S, H, 64, scale, int(bool(q_prescaled)), _p(out),
              out.stride(0), _p(lse), _stream(qkv))
    return out


def attention_rollout_work(B: int, S: int, H: int, device) -> torch.Tensor:
    """the f32 per-head partials buffer of attention_rollout_step: one float per (clip, head, token)"""
    return torch.zeros(B * H * S, dtype=torch.float32, device=device)


def _check_attention_rollout(name, qkv, dout, lse, r_in, B, S, H, work, r_out):
    """what attention_rollout_step and attention_grad_rollout_step (dout given) ask of their tensors"""
    _dev(*(t for t in (qkv, dout, lse, r_in, work, r_out) if t is not None))
    _need(lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() >= B * H * S, "lse: f32 [B*H*S]")
    _need(qkv.dtype == torch.bfloat16 and qkv.dim() == 2 and qkv.stride(1) == 1, f"{name}: qkv bf16 rows")
    _need(qkv.shape[1] >= 3 * H * 64 and qkv.shape[0] >= B * S, f"{name}: qkv rows / columns")
    if dout is not None:
        _need(dout.dtype == torch.bfloat16 and dout.dim() == 2 and dout.stride(1) == 1, f"{name}: dout bf16 rows")
        _need(dout.shape[1] >= H * 64 and dout.shape[0] >= B * S, f"{name}: dout rows / columns")
    for t, nm in ((r_in, "r_in"), (r_out, "r_out")):
        _need(t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (B, S), f"{name}: {nm} f32 [B, S]")
    _need(work.dtype == torch.float32 and work.is_contiguous() and work.numel() >= B * H * S,
          f"{name} work: contiguous f32 [B*H*S]")


def attention_rollout_step(qkv: torch.Tensor, lse: torch.Tensor, r_in: torch.Tensor, B: int, S: int, H: int,
                           alpha: float, work: torch.Tensor, r_out: torch.Tensor) -> torch.Tensor:
    """One attention-rollout step of the CLS row (vc_attention_rollout_step): r_out = alpha * mean_h(P_h^T r_in)
    + (1 - alpha) * r_in with P_h recomputed from qkv bf16 [>= B*S, >= 3*H*64] (q pre-scaled) and the lse f32
    [B*H*S] of attention_fwd_lse.  r_in / r_out f32 [B, S]; work from attention_rollout_work."""
    _check_attention_rollout("attention_rollout_step", qkv, None, lse, r_in, B, S, H, work, r_out)
    _lib.call("vc_attention_rollout_step", _p(qkv), qkv.stride(0), _p(lse), _p(r_in), B, S, H, 64, float(alpha),
              _p(work), work.numel(), _p(r_out), _stream(qkv))
    return r_out


def attention_grad_rollout_step(qkv: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor, r_in: torch.Tensor, B: int,
                                S: int, H: int, alpha: float, beta: float, work: torch.Tensor,
                                r_out: torch.Tensor) -> torch.Tensor:
    """One gradient-weighted rollout step of the CLS row (vc_attention_grad_rollout_step): r_out = alpha *
    mean_h(max(P_h * dP_h, 0)^T r_in) + beta * r_in, P_h as attention_rollout_step's and dP_h[i][j] = dout_h[i] . v_j
    with dout bf16 [>= B*S, >= H*64] (head h at columns 64h, attention_bwd's `dout`).  work from
    attention_rollout_work."""
    _dev(dout)
    _check_attention_rollout("attention_grad_rollout_step", qkv, dout, lse, r_in, B, S, H, work, r_out)
    _lib.call("vc_attention_grad_rollout_step", _p(qkv), qkv.stride(0), _p(dout), dout.stride(0), _p(lse), _p(r_in), B,
              S, H, 64, float(alpha), float(beta), _p(work), work.numel(), _p(r_out), _stream(qkv))
    return r_out


def temporal_rollout_step(qkv: torch.Tensor, r_frame_in: torch.Tensor, B: int, P: int, T: int, H: int, alpha: float,
                          r_clip_out: torch.Tensor, r_frame_out: torch.Tensor | None = None) -> torch.Tensor:
    """The temporal half of one rollout step through a TimeSformer layer (vc_temporal_rollout_step): per (clip,
    patch) y = alpha * mean_h(P_h^T x) + (1 - alpha) * x over the patch's T frames, x = r_frame_in[b*T + t, 1 + p],
    P_h recomputed from the temporal qkv bf16 [>= B*(1+P*T), >= 3*H*64] (clip layout, q pre-scaled).  r_frame_in
    f32 [B*T, 1+P] (the spatial step's output) -> r_clip_out f32 [B, 1+P*T] (column 0: the sum of the T CLS slots)
    and, if given, r_frame_out f32 [B*T, 1+P], the same values spread for the next layer's spatial step."""
    outs = (r_clip_out,) if r_frame_out is None else (r_clip_out, r_frame_out)
    _dev(qkv, r_frame_in, *outs)
    _need(qkv.dtype == torch.bfloat16 and qkv.dim() == 2 and qkv.stride(1) == 1, "temporal_rollout_step: qkv bf16 rows")
    _need(qkv.shape[1] >= 3 * H * 64 and qkv.shape[0] >= B * (1 + P * T), "temporal_rollout_step: qkv rows / columns")
    _need(T <= 32, "temporal_rollout_step: T <= 32")
    for t, nm, shape in ((r_frame_in, "r_frame_in", (B * T, 1 + P)), (r_clip_out, "r_clip_out", (B, 1 + P * T)),
                         (r_frame_out, "r_frame_out", (B * T, 1 + P))):
        _need(t is None or (t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape),
              f"temporal_rollout_step: {nm} f32 {list(shape)}")
    _lib.call("vc_temporal_rollout_step", _p(qkv), qkv.stride(0), _p(r_frame_in), B, P, T, H, 64, float(alpha),
              _p(r_clip_out), None if r_frame_out is None else _p(r_frame_out), _stream(qkv))
    return r_clip_out


def window_rollout_work(B: int, grid, heads: int, device) -> torch.Tensor:
    """the f32 scratch of window_rollout_step: three floats per (head, clip, token) -- the per-head partials, and each
    row's maximum and weight between the step's two passes"""
    T, H, W = grid
    return torch.zeros(3 * heads * B * T * H * W, dtype=torch.float32, device=device)


def _check_window_rollout(name, qkv, table, B, grid, heads, window, full_window, work, vectors, dout=None):
    """what window_rollout_step and window_grad_rollout_step (dout given) ask of their tensors; vectors: (f32
    [B*T*H*W] tensor or None, its name) pairs"""
    T, H, W = grid
    wt, wh, ww = window
    ft, fh, fw = full_window
    ntok = B * T * H * W
    ntab = (2 * ft - 1) * (2 * fh - 1) * (2 * fw - 1)
    _dev(*(t for t in (qkv, dout, table, work, *(v for v, _ in vectors)) if t is not None))
    _need(qkv.dtype == torch.bfloat16 and qkv.dim() == 2 and qkv.stride(1) == 1, f"{name}: qkv bf16 rows")
    _need(qkv.shape[1] >= 3 * heads * 32 and qkv.shape[0] >= ntok, f"{name}: qkv rows / columns")
    if dout is not None:
        _need(dout.dtype == torch.bfloat16 and dout.dim() == 2 and dout.stride(1) == 1, f"{name}: dout bf16 rows")
        _need(dout.shape[1] >= heads * 32 and dout.shape[0] >= ntok, f"{name}: dout rows / columns")
    _need(table.dtype == torch.float32 and table.is_contiguous() and tuple(table.shape) == (ntab, heads),
          f"{name} table: f32 [ntab, heads]")
    for t, nm in vectors:
        _need(t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == ntok),
              f"{name}: {nm} f32 [B*T*H*W]")
    _need(T % wt == 0 and H % wh == 0 and W % ww == 0, f"{name}: grid must be whole windows")
    _need(work.dtype == torch.float32 and work.is_contiguous() and work.numel() >= 3 * heads * ntok,
          f"{name} work: contiguous f32 [3*heads*B*T*H*W]")


def window_rollout_step(qkv: torch.Tensor, table: torch.Tensor, r_in: torch.Tensor, B: int, grid, heads: int, window,
                        shift, full_window, alpha: float, work: torch.Tensor, r_out: torch.Tensor) -> torch.Tensor:
    """One block step of attention rollout through Swin's shifted-window attention (vc_window_rollout_step): r_out[j]
    = alpha * mean_h sum_{i in win(j)} r_in[i] P_h[i][j] + (1 - alpha) * r_in[j], P_h recomputed from the block's kept
    qkv bf16 [>= B*T*H*W, >= 3*heads*32] (q pre-scaled; v is not read) and its bias table f32 [ntab, heads] of the full
    window, with the shift-region mask.  window / shift: the effective ones (swin3d.window_and_shift).  r_in / r_out
    f32 [B*T*H*W] (any shape of that many elements); work from window_rollout_work."""
    _dev(r_in, r_out)
    _check_window_rollout("window_rollout_step", qkv, table, B, grid, heads, window, full_window, work,
                          ((r_in, "r_in"), (r_out, "r_out")))
    (T, H, W), (wt, wh, ww), (st, sh, sw), (ft, fh, fw) = grid, window, shift, full_window
    _lib.call("vc_window_rollout_step", _p(qkv), qkv.stride(0), _p(table), _p(r_in), B, T, H, W, heads, 32, wt, wh, ww,
              st, sh, sw, ft, fh, fw, float(alpha), _p(work), work.numel(), _p(r_out), _stream(qkv))
    return r_out


def window_grad_rollout_work(B: int, grid, heads: int, device) -> torch.Tensor:
    """the f32 scratch of window_grad_rollout_step: window_rollout_work's (three floats per (head, clip, token))"""
    return window_rollout_work(B, grid, heads, device)


def window_grad_rollout_step(qkv: torch.Tensor, dout: torch.Tensor, table: torch.Tensor, r_in: torch.Tensor,
                             a_in: torch.Tensor, B: int, grid, heads: int, window, shift, full_window, alpha: float,
                             beta: float, work: torch.Tensor, a_out: torch.Tensor, base: torch.Tensor | None = None,
                             r_out: torch.Tensor | None = None) -> torch.Tensor:
    """One block step of the gradient-weighted rollout through Swin's shifted-window attention
    (vc_window_grad_rollout_step): a_out[j] = alpha * mean_h sum_{i in win(j)} r_in[i] P_h[i][j] max(dP_h[i][j], 0) +
    beta * a_in[j] with dP_h[i][j] = dO_h[i] . v_j, and, when base and r_out are given (both or neither), r_out = a_out +
    base.  qkv / table / window / shift / full_window as window_rollout_step takes them (v is read here); dout bf16
    [>= B*T*H*W, >= heads*32] rows of dL/dO with any leading dimension that is a multiple of 8.  r_in / a_in / base /
    a_out / r_out f32 [B*T*H*W]; the outputs alias no input; work from window_grad_rollout_work."""
    _dev(dout, r_in, a_in, a_out)
    _need((base is None) == (r_out is None), "window_grad_rollout_step: base and r_out come together")
    _check_window_rollout("window_grad_rollout_step", qkv, table, B, grid, heads, window, full_window, work,
                          ((r_in, "r_in"), (a_in, "a_in"), (a_out, "a_out"), (base, "base"), (r_out, "r_out")), dout=dout)
    (T, H, W), (wt, wh, ww), (st, sh, sw), (ft, fh, fw) = grid, window, shift, full_window
    _lib.call("vc_window_grad_rollout_step", _p(qkv), qkv.stride(0), _p(dout), dout.stride(0), _p(table), _p(r_in), _p(a_in),
              None if base is None else _p(base), B, T, H, W, heads, 32, wt, wh, ww, st, sh, sw, ft, fh, fw, float(alpha),
              float(beta), _p(work), work.numel(), _p(a_out), None if r_out is None else _p(r_out), _stream(qkv))
    return a_out


def merge_rollout_spread(r_parent: torch.Tensor, B: int, grid, r_child: torch.Tensor) -> torch.Tensor:
    """The rollout's hop through PatchMerging (vc_merge_rollout_spread): r_parent f32 [B*T*ceil(H/2)*ceil(W/2)] ->
    r_child f32 [B*T*H*W] on the child `grid` (T, H, W), every merged token's relevance shared equally among its
    existing children."""
    _dev(r_parent, r_child)
    T, H, W = grid
    _need(r_parent.dtype == torch.float32 and r_parent.is_contiguous() and
          r_parent.numel() == B * T * ((H + 1) // 2) * ((W + 1) // 2), "merge_rollout_spread: r_parent f32 [B*T*H2*W2]")
    _need(r_child.dtype == torch.float32 and r_child.is_contiguous() and r_child.numel() == B * T * H * W,
          "merge_rollout_spread: r_child f32 [B*T*H*W]")
    _lib.call("vc_merge_rollout_spread", _p(r_parent), B, T, H, W, _p(r_child), _stream(r_parent))
    return r_child


def attention_bwd(qkv: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor, delta: torch.Tensor,
                  B: int, S: int, H: int, dqkv: torch.Tensor, stream2: torch.cuda.Stream | None = None) -> torch.Tensor:
    """dqkv (q part = dL/dq' of the stored pre-scaled q', then dk, dv) of the joint attention.
    `stream2`: the dQ kernel runs there beside dK/dV (vc_attention_bwd_2s); the current stream waits
    for it before anything enqueued after this call.
    The padding rows of qkv and dout (past B*S, up to the last clip's 64-row tile) must hold finite values:
    they are read and multiplied by zero, so a NaN or Inf there reaches valid rows of dqkv."""
    _dev(qkv, out, dout, lse, delta, dqkv)
    for t, nm in ((qkv, "qkv"), (out, "out"), (dout, "dout"), (dqkv, "dqkv")):
        _need(t.dtype == torch.bfloat16 and t.stride(1) == 1, f"attention_bwd: {nm} bf16 with unit column stride")
    _need(lse.dtype == torch.float32 and delta.dtype == torch.float32 and lse.numel() >= B * H * S and
          delta.numel() >= B * H * S, "attention_bwd: lse / delta f32 [B*H*S]")
    pad = (B - 1) * S + (S + 63) // 64 * 64
    _need(qkv.shape[0] >= pad and dout.shape[0] >= pad, "attention_bwd: qkv / dout need row padding to a 64-row tile")
    _need(out.shape[0] >= B * S and dqkv.shape[0] >= B * S, "attention_bwd rows")
    _need(qkv.shape[1] >= 3 * H * 64 and dqkv.shape[1] >= 3 * H * 64 and out.shape[1] >= H * 64 and
          dout.shape[1] >= H * 64, "attention_bwd columns")
    if stream2 is not None:
        _lib.call("vc_attention_bwd_2s", _p(qkv), qkv.stride(0), _p(out), out.stride(0), _p(dout), dout.stride(0),
                  _p(lse), _p(delta), B, S, H, 64, _p(dqkv), dqkv.stride(0), _stream(qkv), stream2.cuda_stream)
        return dqkv
    _lib.call("vc_attention_bwd", _p(qkv), qkv.stride(0), _p(out), out.stride(0), _p(dout), dout.stride(0), _p(lse),
              _p(delta), B, S, H, 64, _p(dqkv), dqkv.stride(0), _stream(qkv))
    return dqkv


def layernorm_bwd(dy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, eps: float, dx: torch.Tensor,
                  dxb: torch.Tensor, dgamma: torch.Tensor, dbeta: torch.Tensor, work: torch.Tensor,
                  m: int | None = None, dsum_in: torch.Tensor | None = None,
                  dsum_out: torch.Tensor | None = None) -> torch.Tensor:
    """dx += LayerNorm backward of dy (f32, in place), dxb = bf16(dx); dgamma / dbeta overwritten;
    optional dsum_in / dsum_out = column sums of dx before / after (bias gradients)."""
    _dev(dy, x, gamma, dx, dxb, dgamma, dbeta, work)
    M = x.shape[0] if m is None else m
    D = gamma.numel()
    _need(dy.dtype == torch.float32 and x.dtype == torch.float32 and dx.dtype == torch.float32 and
          dxb.dtype == torch.bfloat16 and work.dtype == torch.float32, "layernorm_bwd dtypes")
    _need(all(t.shape[0] >= M and t.shape[1] >= D and t.stride(1) == 1 for t in (dy, x, dx, dxb)), "layernorm_bwd shapes")
    _need(dgamma.numel() == D and dbeta.numel() == D and dgamma.is_contiguous() and dbeta.is_contiguous(),
          "layernorm_bwd dgamma/dbeta")
    _need((dsum_in is None) == (dsum_out is None), "layernorm_bwd: dsum_in and dsum_out go together")
    if dsum_in is not None:
        _dev(dsum_in, dsum_out)
        _need(all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == D for t in (dsum_in, dsum_out)),
              "layernorm_bwd dsum_in / dsum_out f32 [D]")
    _lib.call("vc_layernorm_bwd", _p(dy), dy.stride(0), _p(x), x.stride(0), M, D, _p(gamma), eps, _p(dx), dx.stride(0),
              _p(dxb), dxb.stride(0), _p(dgamma), _p(dbeta), _p(dsum_in) if dsum_in is not None else None,
              _p(dsum_out) if dsum_out is not None else None, _p(work), work.numel(), _stream(x))
    return dx


def colsum(x: torch.Tensor, out: torch.Tensor, work: torch.Tensor | None = None, m: int | None = None,
           nscaled: int = 0, scale: float = 1.0) -> torch.Tensor:
    """out[n] = s(n) * sum over the first m rows of x[:, n] (x f32 or bf16 2-D, unit column stride)."""
    _dev(x, out)
    R = x.shape[0] if m is None else m
    N = out.numel()
    _need(x.dtype in (torch.float32, torch.bfloat16) and x.dim() == 2 and x.stride(1) == 1 and x.shape[1] >= N and
          x.shape[0] >= R, "colsum input")
    _need(out.dtype == torch.float32 and out.is_contiguous(), "colsum out f32")
    wp, wn = (_p(work), work.numel()) if work is not None else (None, 0)
    _lib.call("vc_colsum", _p(x), 0 if x.dtype == torch.float32 else 1, x.stride(0), R, N, nscaled, scale, _p(out), wp,
              wn, _stream(x))
    return out


def colsum_work(R: int, N: int, device) -> torch.Tensor:
    """Scratch for vc_colsum's full row split (S1 + S2 partial rows of N floats)."""
    s1 = min(2048, max(1, (R + 63) // 64))
    return torch.empty((s1 + (s1 + 63) // 64) * N, dtype=torch.float32, device=device)


def wgrad_work(M: int, N1: int, N2: int, device) -> torch.Tensor:
    """Scratch for vc_wgrad_bf16's split-K partials at the split count the kernel aims for
    (train.hip vc_wgrad_bf16: ~512 workgroups of 128 x 128, ~256 of 256 x 256)."""
    if N1 % 256 == 0 and N2 % 256 == 0:
        sp = min(-(-256 // ((N1 // 256) * (N2 // 256))), (M // 32) // 4)
    else:
        sp = min(-(-512 // ((N1 // 128) * (N2 // 128))), (M // 64) // 2)
    return torch.empty(max(2, sp) * N1 * N2, dtype=torch.float32, device=device)


def wgrad_kernel_name(M: int, N1: int, N2: int, work_elems: int) -> str:
    """The rocprofv3 name of the kernel vc_wgrad_bf16 runs for this call: csrc/train.hip's own plan
    (vc_wgrad_pick: split count from the device's CU count and the scratch size, then the ping-pong kernel
    when every split has >= 3 32-row half-tiles, unless VCLIP_WGRAD_PP=0)"""
    k = _lib.load().vc_wgrad_pick(M, N1, N2, work_elems) & 15
    return {0: "trn::wgrad_kernel", 1: "trn::wgrad_big_kernel", 2: "trn::wgrad_pp_kernel"}[k]


def wgrad(g: torch.Tensor, x: torch.Tensor, out: torch.Tensor, work: torch.Tensor | None = None,
          nscaled: int = 0, scale: float = 1.0, m: int | None = None) -> torch.Tensor:
    """out[n1][n2] = s(n1) * sum_m g[m][n1] x[m][n2]  (g bf16 [M, N1], x bf16 [M, N2], out f32 [N1, N2])."""
    _dev(g, x, out)
    M = g.shape[0] if m is None else m
    N1, N2 = out.shape
    _need(g.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and out.dtype == torch.float32, "wgrad dtypes")
    _need(g.stride(1) == 1 and x.stride(1) == 1 and out.stride(1) == 1 and g.shape[1] >= N1 and x.shape[1] >= N2 and
          g.shape[0] >= M and x.shape[0] >= M, "wgrad shapes")
    wp, wn = (_p(work), work.numel()) if work is not None else (None, 0)
    rec = _REC[0]
    if rec is not None:  # one entry per vc_wgrad_bf16 call: the split-K kernel plus its partial reduction
        label = wgrad_kernel_name(M, N1, N2, wn) + " (+ wgrad_reduce_kernel)"
        e0 = rec.begin()
    _lib.call("vc_wgrad_bf16", _p(g), g.stride(0), _p(x), x.stride(0), M, N1, N2, nscaled, scale, _p(out),
              out.stride(0), wp, wn, _stream(g))
    if rec is not None:
        rec.end(e0, label, "wgrad", 2.0 * M * N1 * N2, "flop")
    return out


def cls_head_bwd(x, B, S, gamma, beta, eps, wc, dlogits, dx, dxb, dwc, dbc, dgamma, dbeta):
    _dev(x, gamma, beta, wc, dlogits, dx, dxb, dwc, dbc, dgamma, dbeta)
    D = gamma.numel()
    nl = wc.shape[0]
    _need(dlogits.dtype == torch.float32 and dlogits.is_contiguous() and tuple(dlogits.shape) == (B, nl),
          "cls_head_bwd dlogits f32 [B, nl]")
    _need(x.shape[0] >= B * S and dx.shape[0] >= B * S and dxb.shape[0] >= B * S, "cls_head_bwd rows")
    _lib.call("vc_cls_head_bwd", _p(x), x.stride(0), B, S, D, _p(gamma), _p(beta), eps, _p(wc), nl, _p(dlogits),
              _p(dx), dx.stride(0), _p(dxb), dxb.stride(0), _p(dwc), _p(dbc), _p(dgamma), _p(dbeta), _stream(x))


def embed_bwd(dx: torch.Tensor, B: int, S: int, dpos: torch.Tensor, dcls: torch.Tensor, demb: torch.Tensor):
    _dev(dx, dpos, dcls, demb)
    D = dcls.numel()
    _need(dx.dtype == torch.float32 and dx.shape[0] >= B * S and dx.stride(1) == 1, "embed_bwd dx")
    _need(dpos.dtype == torch.float32 and dpos.is_contiguous() and dpos.numel() == S * D, "embed_bwd dpos")
    _need(demb.dtype == torch.bfloat16 and demb.shape[0] >= B * (S - 1) and demb.shape[1] >= D and demb.stride(1) == 1,
          "embed_bwd demb")
    _lib.call("vc_embed_bwd", _p(dx), dx.stride(0), B, S, D, _p(dpos), _p(dcls), _p(demb), demb.stride(0), _stream(dx))


def adamw(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    _dev(param, grad, exp_avg, exp_avg_sq)
    n = param.numel()
    _need(all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n for t in
              (param, grad, exp_avg, exp_avg_sq)), "adamw: contiguous f32 buffers of one size")
    _lib.call("vc_adamw", _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), n, lr, beta1, beta2, eps, weight_decay,
              int(step), grad_scale, _stream(param))


def adamw_step_table(beta1: float, beta2: float, lr: float, steps: int, device) -> torch.Tensor:
    """Device f32 [steps, 2]: row t-1 = (lr / (1 - beta1^t), sqrt(1 - beta2^t)) exactly as vc_adamw derives them
    for step t (vc_adamw_step_table computes them in the library with the same double arithmetic)."""
    import numpy as np
    host = np.zeros((steps, 2), dtype=np.float32)
    _lib.call("vc_adamw_step_table", beta1, beta2, lr, steps, host.ctypes.data)
    return torch.from_numpy(host).to(device)


def adamw_tab(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, tab, counter, grad_scale=1.0):
    """adamw() with the step on the device: step = counter + 1 (int64 [1] device tensor), constants from tab
    (adamw_step_table); the counter is not advanced here (adamw_step_tick)."""
    _dev(param, grad, exp_avg, exp_avg_sq, tab, counter)
    n = param.numel()
    _need(all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n for t in
              (param, grad, exp_avg, exp_avg_sq)), "adamw_tab: contiguous f32 buffers of one size")
    _need(tab.dtype == torch.float32 and tab.is_contiguous() and tab.dim() == 2 and tab.shape[1] == 2 and
          counter.dtype == torch.int64 and counter.numel() >= 1, "adamw_tab: tab f32 [steps, 2], counter int64")
    _lib.call("vc_adamw_tab", _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), n, lr, beta1, beta2, eps,
              weight_decay, _p(tab), _p(counter), tab.shape[0], grad_scale, _stream(param))


def adamw_step_tick(counter: torch.Tensor):
    _dev(counter)
    _need(counter.dtype == torch.int64, "adamw_step_tick: int64 counter")
    _lib.call("vc_adamw_step_tick", _p(counter), _stream(counter))


def adamw_multi(params, grads, exp_avgs, exp_avg_sqs, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    """vc_adamw on every (param, grad, exp_avg, exp_avg_sq) quadruple in one launch."""
    rows, c0 = [], 0
    for p, g, m, v in zip(params, grads, exp_avgs, exp_avg_sqs):
        _dev(p, g, m, v)
        n = p.numel()
        _need(all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n for t in (p, g, m, v)),
              "adamw_multi: contiguous f32 buffers of one size per entry")
        rows.append([p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, c0])
        c0 += (n + 1023) // 1024
    if not rows:
        return
    # the device table is cached by content: in a steady training loop the caching allocator hands
    # the gradients the same addresses every step, so the table is uploaded once (a host -> device
    # copy per step would synchronise the host with the stream)
    key = tuple(x for r in rows for x in r[:5])
    tab = _ADAMW_TABLES.get(key)
    if tab is None or tab.device != params[0].device:
        if len(_ADAMW_TABLES) >= 8:
            _ADAMW_TABLES.clear()
        tab = _ADAMW_TABLES[key] = torch.tensor(rows, dtype=torch.int64).to(params[0].device)
    _lib.call("vc_adamw_multi", _p(tab), len(rows), c0, lr, beta1, beta2, eps, weight_decay, int(step), grad_scale,
              _stream(params[0]))
    return tab


_ADAMW_TABLES = {}


def pack_weight(src: torch.Tensor, dst: torch.Tensor | None = None, dst_t: torch.Tensor | None = None,
                nscaled: int = 0, scale: float = 1.0):
    _dev(src)
    N, K = src.shape
    _need(src.dtype == torch.float32 and src.is_contiguous(), "pack_weight src f32 contiguous [N, K]")
    if dst is not None:
        _need(dst.dtype == torch.bfloat16 and dst.is_contiguous() and tuple(dst.shape) == (N, K), "pack_weight dst")
    if dst_t is not None:
        _need(dst_t.dtype == torch.bfloat16 and dst_t.is_contiguous() and tuple(dst_t.shape) == (K, N), "pack_weight dst_t")
    _lib.call("vc_pack_weight", _p(src), N, K, nscaled, scale, _p(dst) if dst is not None else None,
              _p(dst_t) if dst_t is not None else None, _stream(src))


# ---- LoRA fine-tuning (csrc/lora.hip) ----------------------------------------------------------
LORA_MAX_RANK = 64  # csrc/lora.hip MAX_RANK


def _lora_ab(name: str, a: torch.Tensor, b: torch.Tensor, N: int, K: int) -> int:
    r = a.shape[0] if a.dim() == 2 else 0
    _need(a.dtype == torch.float32 and b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous() and
          1 <= r <= LORA_MAX_RANK and tuple(a.shape) == (r, K) and tuple(b.shape) == (N, r),
          f"{name}: A f32 [r, {K}], B f32 [{N}, r] contiguous, 1 <= r <= {LORA_MAX_RANK}")
    return r


def lora_merge(w: torch.Tensor, a: torch.Tensor, b: torch.Tensor, s: float, dst: torch.Tensor | None = None,
               dst_t: torch.Tensor | None = None, out: torch.Tensor | None = None, row0: int = 0,
               nscaled: int = 0, scale: float = 1.0):
    """Rows [row0, row0 + N) of v = w + s * b @ a in fp32 (w f32 [R, K], a f32 [r, K], b f32 [N, r]) into any of
    dst bf16 [R, K], dst_t bf16 [K, R] and out f32 [R, K]; the other rows of the outputs are left alone.  Rows
    < nscaled of the bf16 outputs are multiplied by scale, as pack_weight does."""
    _dev(w, a, b)
    _need(w.dtype == torch.float32 and w.dim() == 2 and w.stride(1) == 1, "lora_merge w f32 [R, K]")
    R, K = w.shape
    N = b.shape[0]
    r = _lora_ab("lora_merge", a, b, N, K)
    _need(0 <= row0 and row0 + N <= R, "lora_merge: rows [row0, row0 + N) outside w")
    _need(dst is not None or dst_t is not None or out is not None, "lora_merge: no output")
    if dst is not None:
        _dev(dst)
        _need(dst.dtype == torch.bfloat16 and dst.stride(1) == 1 and tuple(dst.shape) == (R, K), "lora_merge dst")
    if dst_t is not None:
        _dev(dst_t)
        _need(dst_t.dtype == torch.bfloat16 and dst_t.stride(1) == 1 and tuple(dst_t.shape) == (K, R), "lora_merge dst_t")
    if out is not None:
        _dev(out)
        _need(out.dtype == torch.float32 and out.stride(1) == 1 and tuple(out.shape) == (R, K) and
              out.untyped_storage().data_ptr() != w.untyped_storage().data_ptr(), "lora_merge out (f32 [R, K], not w)")
    _lib.call("vc_lora_merge", _p(w), w.stride(0), row0, N, K, _p(a), _p(b), r, s, nscaled, scale,
              _p(dst) if dst is not None else None, dst.stride(0) if dst is not None else 0,
              _p(dst_t) if dst_t is not None else None, dst_t.stride(0) if dst_t is not None else 0,
              _p(out) if out is not None else None, out.stride(0) if out is not None else 0, _stream(w))


def lora_down(x: torch.Tensor, s: torch.Tensor, out: torch.Tensor, transposed: bool = False,
              m: int | None = None) -> torch.Tensor:
    """out[m, j] = bf16(sum_k x[m, k] bf16(S[j, k])): x bf16 [M, K] (unit column stride, K % 32 == 0), S = s f32
    [r, K], or with transposed=True s f32 [K, r] read as its transpose (the B of an adapter against dy); out bf16
    [M, r]."""
    _dev(x, s, out)
    M = x.shape[0] if m is None else m
    K = x.shape[1]
    _need(x.dtype == torch.bfloat16 and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] >= M, "lora_down x bf16 [M, K]")
    _need(s.dtype == torch.float32 and s.dim() == 2 and s.is_contiguous() and
          s.shape[0 if transposed else 1] == K, "lora_down s f32 [r, K] (or [K, r] transposed)")
    r = s.shape[1 if transposed else 0]
    _need(1 <= r <= LORA_MAX_RANK, "lora_down rank")
    _need(out.dtype == torch.bfloat16 and out.is_contiguous() and out.dim() == 2 and out.shape[0] >= M and
          out.shape[1] == r, "lora_down out bf16 [M, r]")
    rec = _REC[0]
    e0 = rec.begin() if rec is not None else None
    _lib.call("vc_lora_down", _p(x), x.stride(0), M, K, _p(s), 1 if transposed else K, r if transposed else 1, r,
              _p(out), _stream(x))
    if rec is not None:
        rec.end(e0, "lora::down_kernel", "lora_down", M * K * 2.0 + M * r * 2.0 + r * K * 4.0, "byte")
    return out


def lora_wgrad_work(N: int, r: int, device, splits: int = 32) -> torch.Tensor:
    """Scratch for lora_wgrad's split partials (`splits` of them; the kernel takes what fits)."""
    return torch.empty(splits * N * r, dtype=torch.float32, device=device)


def lora_wgrad(g: torch.Tensor, u: torch.Tensor, out: torch.Tensor, work: torch.Tensor, c: float = 1.0,
               m: int | None = None, transposed: bool | None = None) -> torch.Tensor:
    """out = c * g[:m].T @ u[:m]: g bf16 [M, N] (unit column stride), u bf16 [M, r]; out f32 [N, r], or f32 [r, N]
    (then the transpose is stored).  Split over M into `work`, partials summed in a fixed order."""
    _dev(g, u, out, work)
    M = g.shape[0] if m is None else m
    N = g.shape[1]
    _need(g.dtype == torch.bfloat16 and g.dim() == 2 and g.stride(1) == 1 and g.shape[0] >= M, "lora_wgrad g bf16 [M, N]")
    _need(u.dtype == torch.bfloat16 and u.dim() == 2 and u.is_contiguous() and u.shape[0] >= M and
          1 <= u.shape[1] <= LORA_MAX_RANK, "lora_wgrad u bf16 [M, r]")
    r = u.shape[1]
    _need(out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) in ((N, r), (r, N)),
          "lora_wgrad out f32 [N, r] or [r, N]")
    if transposed is None:
        transposed = tuple(out.shape) != (N, r)
    _need(tuple(out.shape) == ((r, N) if transposed else (N, r)), "lora_wgrad out shape against transposed")
    _need(work.dtype == torch.float32 and work.is_contiguous() and work.numel() >= N * r, "lora_wgrad work")
    rec = _REC[0]
    e0 = rec.begin() if rec is not None else None
    _lib.call("vc_lora_wgrad", _p(g), g.stride(0), _p(u), M, N, r, c, 1 if transposed else 0, _p(out), _p(work),
              work.numel(), _stream(g))
    if rec is not None:
        rec.end(e0, "lora::wgrad_kernel (+ wgrad_reduce_kernel)", "lora_wgrad", M * N * 2.0 + M * r * 2.0 + N * r * 4.0,
                "byte")
    return out


def lora_grads(x: torch.Tensor, dy: torch.Tensor, a: torch.Tensor, b: torch.Tensor, c: float, da: torch.Tensor,
               db: torch.Tensor, uv: torch.Tensor, work: torch.Tensor, m: int | None = None):
    """The gradients of one adapter (W_eff = W + s b a) from the saved input x bf16 [M, K] and the output
    gradient dy bf16 [M, N]: db [N, r] = c dy^T (x a^T), da [r, K] = c (dy b)^T x, with c = s (times the q
    scale for the q adapter).  uv: bf16 scratch of >= M * r elements for the r-wide intermediate (rounded to
    bf16 once; the MFMAs also read a / b rounded to bf16); work: f32 split scratch.  No [N, K] gradient exists at
    any point."""
    N, K = dy.shape[1], x.shape[1]
    r = _lora_ab("lora_grads", a, b, N, K)
    M = x.shape[0] if m is None else m
    _need(uv.dtype == torch.bfloat16 and uv.is_contiguous() and uv.numel() >= M * r, "lora_grads uv scratch")
    _need(tuple(da.shape) == (r, K) and tuple(db.shape) == (N, r), "lora_grads da [r, K], db [N, r]")
    u = uv.view(-1)[:M * r].view(M, r)
    lora_down(x, a, u, m=M)
    lora_wgrad(dy, u, db, work, c, m=M, transposed=False)
    lora_down(dy, b, u, transposed=True, m=M)
    lora_wgrad(x, u, da, work, c, m=M, transposed=True)


# ---- ResNet50-LSTM (csrc/lstm.hip) ------------------------------------------------------------
def lstm_group(hidden: int) -> int:
    """Sequences one workgroup of the recurrence kernels owns (csrc/lstm.hip group_of)."""
    return 4 if hidden <= 512 else 2


def _lstm_shape(B: int, T: int, hidden: int):
    _need(B >= 1 and T >= 1, "lstm: B and T must be >= 1")
    _need(0 < hidden <= 1024 and hidden % 4 == 0,
          f"lstm: unsupported hidden size {hidden} (hidden % 4 == 0 and hidden <= 1024)")


def frame_avgpool(x: torch.Tensor, N: int, P: int, C: int, out: torch.Tensor) -> torch.Tensor:
    """out[n] = mean of rows n*P .. n*P + P - 1 of x (channels-last bf16 or fp16, fp32 sum) -> bf16 [N, C]."""
    _dev(x, out)
    _need(N >= 1 and P >= 1 and C >= 1, "frame_avgpool: empty shape")
    _need(x.dtype in H16 and out.dtype == torch.bfloat16 and x.dim() == 2 and out.dim() == 2 and
          x.shape[0] >= N * P and x.shape[1] >= C and out.shape[0] >= N and out.shape[1] >= C and x.stride(1) == 1 and
          out.stride(1) == 1, "frame_avgpool: x bf16 / fp16 [>= N*P, >= C], out bf16 [>= N, >= C]")
    timed("frame_avgpool_kernel", "avgpool", (N * P + N) * C * 2, "byte", _lib.call, "vc_frame_avgpool", _p(x),
          ELEM_F16 if x.dtype == torch.float16 else 0, x.stride(0), N, P, C, _p(out), out.stride(0), _stream(x))
    return out


def batchnorm_train_stats(y: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, running_mean: torch.Tensor,
                          running_var: torch.Tensor, stat: torch.Tensor, eps: float = 1e-5,
                          momentum: float = 0.1) -> torch.Tensor:
    """The statistics pass of vc_batchnorm_train_fwd alone: stat f32 [2, C] = [batch mean | rstd] of the f32
    rows y [M, C] (C % 4 == 0), running_mean / running_var updated in place with `momentum`; no rows written."""
    _dev(y, gamma, beta, running_mean, running_var, stat)
    M, C = y.shape
    _need(y.dtype == torch.float32 and y.stride(1) == 1 and C % 4 == 0 and y.stride(0) % 4 == 0 and
          y.data_ptr() % 16 == 0, "batchnorm_train_stats: y f32 [M, C], C % 4 == 0, 16-byte rows")
    for t in (gamma, beta, running_mean, running_var):
        _need(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == C, "batchnorm_train_stats: f32 [C] vectors")
    _need(stat.dtype == torch.float32 and stat.is_contiguous() and stat.numel() == 2 * C, "batchnorm_train_stats: stat f32 [2, C]")
    splits = min(4096, max(1, (M + 127) // 128))  # conv3d_bwd.hip bn_splits
    work = torch.empty(splits * 2 * C, dtype=torch.float32, device=y.device)
    _lib.call("vc_batchnorm_train_fwd", _p(y), y.stride(0), M, C, _p(gamma), _p(beta), eps, momentum, _p(running_mean),
              _p(running_var), None, 1, 0, 0, None, 0, _p(stat), _p(work), work.numel(), _stream(y))
    return stat


def bn_apply_h16(y: torch.Tensor, stat: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, z: torch.Tensor,
                 res: torch.Tensor | None = None, relu: bool = False) -> torch.Tensor:
    """z fp16 [M, C] = relu?(gamma (y - mean) rstd + beta (+ res fp16)) for f32 y [M, C] and stat = [mean | rstd]
    f32 [2, C] of vc_batchnorm_train_fwd."""
    _dev(y, stat, gamma, beta, z)
    M, C = y.shape
    _need(y.dtype == torch.float32 and y.stride(1) == 1 and C % 4 == 0 and y.stride(0) % 4 == 0, "bn_apply_h16 y")
    _need(stat.dtype == torch.float32 and stat.is_contiguous() and stat.numel() == 2 * C and gamma.numel() == C and
          beta.numel() == C and gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.is_contiguous() and
          beta.is_contiguous(), "bn_apply_h16 stat / gamma / beta f32 [C]")
    _need(z.dtype == torch.float16 and z.stride(1) == 1 and z.shape[0] >= M and z.shape[1] >= C and z.stride(0) % 4 == 0,
          "bn_apply_h16 z fp16 [>= M, >= C]")
    if res is not None:
        _dev(res)
        _need(res.dtype == torch.float16 and res.stride(1) == 1 and res.shape[0] >= M and res.shape[1] >= C,
              "bn_apply_h16 res fp16 [>= M, >= C]")
    _lib.call("vc_bn_apply_h16", _p(y), y.stride(0), M, C, _p(stat), _p(gamma), _p(beta),
              _p(res) if res is not None else None, res.stride(0) if res is not None else 0, int(relu), _p(z), z.stride(0),
              _stream(y))
    return z


def video_to_cl_h16(video: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """f32 clip [B, C <= 8, T, H, W] -> channels-last fp16 rows out [B*T*H*W, 8] (channels >= C zero)."""
    _dev(video, out)
    _need(video.dtype == torch.float32 and video.is_contiguous() and video.dim() == 5 and 1 <= video.shape[1] <= 8,
          "video_to_cl_h16: video f32 contiguous [B, C <= 8, T, H, W]")
    B, C = video.shape[:2]
    P = video.shape[2] * video.shape[3] * video.shape[4]
    _need(out.dtype == torch.float16 and out.is_contiguous() and tuple(out.shape) == (B * P, 8), "video_to_cl_h16 out")
    _lib.call("vc_video_to_cl_h16", _p(video), B, C, P, _p(out), _stream(video))
    return out


def _lstm_fwd_operands(name: str, rows: str, min_rows: int, B: int, hidden: int, pre, w_hh_t, h_seq, h_last) -> None:
    """The operands lstm_seq_fwd and lstm_seq_fwd_ragged share; `rows` is how the entry point's messages
    name the row count of pre / h_seq, min_rows what it asks of it here."""
    _dev(pre, w_hh_t, h_seq, h_last)
    _need(pre.dtype == torch.float32 and pre.dim() == 2 and pre.shape[0] >= min_rows and pre.shape[1] >= 4 * hidden and
          pre.stride(1) == 1, f"{name}: pre f32 [{rows}, >= 4H]")
    _need(w_hh_t.dtype == torch.float32 and w_hh_t.is_contiguous() and tuple(w_hh_t.shape) == (hidden, 4 * hidden),
          f"{name}: w_hh_t f32 contiguous [H, 4H] (weight_hh transposed)")
    _need(h_seq.dtype == torch.bfloat16 and h_seq.dim() == 2 and h_seq.shape[0] >= min_rows and h_seq.shape[1] >= hidden and
          h_seq.stride(1) == 1, f"{name}: h_seq bf16 [{rows}, >= H]")
    _need(h_last.dtype == torch.float32 and h_last.is_contiguous() and h_last.numel() >= B * hidden,
          f"{name}: h_last f32 [B, H]")


def lstm_seq_fwd(pre: torch.Tensor, B: int, T: int, hidden: int, w_hh_t: torch.Tensor, h_seq: torch.Tensor,
                 h_last: torch.Tensor, keep: torch.Tensor | None = None, gates: torch.Tensor | None = None,
                 c_seq: torch.Tensor | None = None, h_prev: torch.Tensor | None = None) -> torch.Tensor:
    """All T steps of one LSTM layer: pre f32 [B*T, 4H] (x W_ih^T + b_ih + b_hh), w_hh_t f32 [H, 4H] =
    weight_hh transposed -> h_seq bf16 [B*T, H] (times keep f32 [B*T, H] when given), h_last f32 [B, H];
    with gates / c_seq / h_prev (the train variant) the saved state of vc_lstm_seq_bwd."""
    _lstm_shape(B, T, hidden)
    M = B * T
    _lstm_fwd_operands("lstm_seq_fwd", ">= B*T", M, B, hidden, pre, w_hh_t, h_seq, h_last)
    if keep is not None:
        _dev(keep)
        _need(keep.dtype == torch.float32 and keep.is_contiguous() and keep.numel() >= M * hidden and
              keep.shape[-1] == hidden, "lstm_seq_fwd: keep f32 contiguous [B*T, H]")
    train = gates is not None
    if train:
        _need(c_seq is not None and h_prev is not None, "lstm_seq_fwd: the train variant needs gates, c_seq and h_prev")
        _dev(gates, c_seq, h_prev)
        _need(gates.dtype == torch.float32 and gates.is_contiguous() and gates.shape[-1] == 4 * hidden and
              gates.numel() >= M * 4 * hidden, "lstm_seq_fwd: gates f32 contiguous [B*T, 4H]")
        _need(c_seq.dtype == torch.float32 and c_seq.is_contiguous() and c_seq.shape[-1] == hidden and
              c_seq.numel() >= M * hidden, "lstm_seq_fwd: c_seq f32 contiguous [B*T, H]")
        _need(h_prev.dtype == torch.bfloat16 and h_prev.dim() == 2 and h_prev.shape[0] >= M and
              h_prev.shape[1] >= hidden and h_prev.stride(1) == 1, "lstm_seq_fwd: h_prev bf16 [>= B*T, >= H]")
    ngroups = -(-B // lstm_group(hidden))
    timed("lstm_seq_fwd_kernel", "lstm_fwd", 4.0 * hidden * hidden * 4 * T * ngroups, "byte", _lib.call,
          "vc_lstm_seq_fwd", _p(pre), pre.stride(0), B, T, hidden, _p(w_hh_t), _p(keep) if keep is not None else None,
          _p(h_seq), h_seq.stride(0), _p(h_last), _p(gates) if train else None, _p(c_seq) if train else None,
          _p(h_prev) if train else None, h_prev.stride(0) if train else 0, _stream(pre))
    return h_last


_RAGGED_TABLES = {}  # (lengths, row0, device) -> (row0 int32 [B], len int32 [B]) on the device


def _ragged_tables(lengths: tuple, row0: tuple, device) -> tuple:
    key = (lengths, row0, str(device))
    tab = _RAGGED_TABLES.get(key)
    if tab is None:
        if len(_RAGGED_TABLES) >= 256:  # a directory of videos has few distinct batches; do not grow without bound
            _RAGGED_TABLES.clear()
        tab = (torch.tensor(row0, dtype=torch.int32, device=device), torch.tensor(lengths, dtype=torch.int32, device=device))
        _RAGGED_TABLES[key] = tab
    return tab


def _ragged_row0(name: str, lengths: tuple, row0) -> tuple:
    """row0 as host ints, one per sequence; None = the exclusive prefix sum of lengths (back to back)."""
    if row0 is None:
        acc, r = 0, []
        for n in lengths:
            r.append(acc)
            acc += n
        return tuple(r)
    row0 = tuple(int(r) for r in row0)
    _need(len(row0) == len(lengths) and all(r >= 0 for r in row0), f"{name}: row0 must hold one row index >= 0 per sequence")
    return row0


def _ragged_inside(name: str, lengths: tuple, row0: tuple, rows: int, what: str) -> None:
    """Every sequence lies inside the `rows` rows of the buffers and no two overlap (an empty sequence owns no row)."""
    _need(all(r + n <= rows for r, n in zip(row0, lengths)) and rows < 2 ** 31,
          f"{name}: a sequence runs past the {rows} rows of {what}")
    end = 0
    for r, n in sorted(zip(row0, lengths)):
        if n == 0:
            continue
        _need(r >= end, f"{name}: two sequences overlap")
        end = r + n


def lstm_seq_fwd_ragged(pre: torch.Tensor, lengths, hidden: int, w_hh_t: torch.Tensor, h_seq: torch.Tensor,
                        h_last: torch.Tensor, row0=None) -> torch.Tensor:
    """The inference recurrence over len(lengths) sequences of different lengths: sequence b owns rows
    row0[b] .. row0[b] + lengths[b] - 1 of pre f32 [rows, 4H] and h_seq bf16 [rows, H] (row0 defaults to the
    exclusive prefix sum of lengths: the sequences back to back); h_last f32 [B, H] = h of each sequence's
    last step.  Each sequence's rows are bit-identical to lstm_seq_fwd on it alone.  lengths and row0 are
    host integers, lengths >= 1; their device copies are cached per (lengths, row0, device)."""
    lengths = tuple(int(n) for n in lengths)
    B = len(lengths)
    _need(B >= 1 and all(n >= 1 for n in lengths), "lstm_seq_fwd_ragged: lengths must be a non-empty sequence of ints >= 1")
    _lstm_shape(B, max(lengths), hidden)
    row0 = _ragged_row0("lstm_seq_fwd_ragged", lengths, row0)
    _lstm_fwd_operands("lstm_seq_fwd_ragged", "rows", 0, B, hidden, pre, w_hh_t, h_seq, h_last)
    _ragged_inside("lstm_seq_fwd_ragged", lengths, row0, min(pre.shape[0], h_seq.shape[0]), "pre / h_seq")
    d_row0, d_len = _ragged_tables(lengths, row0, pre.device)
    G = lstm_group(hidden)
    steps = sum(max(lengths[i:i + G]) for i in range(0, B, G))  # W_hh is streamed once per step and group
    timed("lstm_seq_fwd_ragged_kernel", "lstm_fwd", 4.0 * hidden * hidden * 4 * steps, "byte", _lib.call,
          "vc_lstm_seq_fwd_ragged", _p(pre), pre.stride(0), B, _p(d_row0), _p(d_len), max(lengths), hidden, _p(w_hh_t),
          _p(h_seq), h_seq.stride(0), _p(h_last), _stream(pre))
    return h_last


def _lstm_state_layout(name: str, B: int, hidden: int, lengths, row0, T):
    """The row layout of the stateful entry points (lstm_seq_fwd_state, lstm_seq_fwd_train_state, lstm_seq_bwd_state),
    ragged (lengths, row0) or dense (lengths=None, T), over B state rows: (lengths or None, row0 or None, max_len,
    rows the dense layout needs, steps per sequence group)."""
    if lengths is None:
        _need(T is not None and row0 is None, f"{name}: the dense layout (lengths=None) takes T and no row0")
        T = int(T)
        _lstm_shape(B, T, hidden)
        return None, None, T, B * T, [T] * -(-B // lstm_group(hidden))
    lengths = tuple(int(n) for n in lengths)
    _need(T is None, f"{name}: T belongs to the dense layout (lengths=None)")
    _need(len(lengths) >= 1 and all(n >= 0 for n in lengths), f"{name}: lengths must be a non-empty sequence of ints >= 0")
    _need(len(lengths) == B, f"{name}: {len(lengths)} lengths for B = {B}: the state holds one row per sequence")
    max_len = max(1, max(lengths))
    _lstm_shape(B, max_len, hidden)
    G = lstm_group(hidden)
    return lengths, _ragged_row0(name, lengths, row0), max_len, 0, [max(lengths[i:i + G]) for i in range(0, B, G)]


def _lstm_state_rows(name: str, what: str, t: torch.Tensor, dtype, min_rows: int, cols: int) -> int:
    _need(t.dtype == dtype and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] >= min_rows and t.shape[1] >= cols,
          f"{name}: {what} [rows, >= {cols}] with unit column stride")
    return t.shape[0]


def _lstm_state_vectors(name: str, B: int, hidden: int, h_n, c_n, h0, c0) -> list:
    """(h0, c0) in and (h_n, c_n) out, as the stateful forwards take them; returns [h0, c0], or [] for the zero state."""
    _need((h0 is None) == (c0 is None), f"{name}: h0 and c0 come together (both None: the zero state)")
    state = [t for t in (h0, c0) if t is not None]
    _dev(c_n, *state)
    for t in (h_n, c_n, *state):
        _need(t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (B, hidden),
              f"{name}: h0, c0, h_n and c_n are f32 contiguous [B, H]")
    span = B * hidden * 4
    for a, b, ok in ((h_n, c_n, False), (h_n, c0, False), (c_n, h0, False), (h_n, h0, True), (c_n, c0, True)):
        if b is not None and abs(_p(a) - _p(b)) < span:  # overlapping storage: only the exact in-place pairs
            _need(ok and _p(a) == _p(b), f"{name}: h_n may alias h0 and c_n may alias c0 exactly, nothing else")
    return state


def lstm_seq_fwd_state(pre: torch.Tensor, lengths, hidden: int, w_hh_t: torch.Tensor, h_seq: torch.Tensor,
                       h_n: torch.Tensor, c_n: torch.Tensor, h0: torch.Tensor | None = None,
                       c0: torch.Tensor | None = None, h_all: torch.Tensor | None = None, row0=None,
                       T: int | None = None) -> tuple:
    """The inference recurrence with nn.LSTM's state: (h0, c0) f32 [B, H] in (both None: the zero state),
    (h_n, c_n) f32 [B, H] out; h_n may be h0 and c_n may be c0 (the state updated in place).  Ragged:
    `lengths` holds one host int >= 0 per sequence and row0 is as in lstm_seq_fwd_ragged; a sequence of
    length 0 passes its state through.  Dense: lengths=None and T, with B = h_n.shape[0]; sequence b owns
    rows b*T .. b*T + T - 1.  h_seq bf16 [rows, >= H] as in the other entry points; h_all (optional) f32
    [rows, >= H] gets the unrounded h of every step.  A sequence run in chunks with the state carried is
    bit-identical to lstm_seq_fwd / lstm_seq_fwd_ragged on it whole."""
    name = "lstm_seq_fwd_state"
    _need(isinstance(h_n, torch.Tensor) and h_n.dim() == 2, f"{name}: h_n f32 [B, H]")
    B = h_n.shape[0]
    lengths, row0, max_len, min_rows, group_steps = _lstm_state_layout(name, B, hidden, lengths, row0, T)
    _lstm_fwd_operands(name, "rows", min_rows, B, hidden, pre, w_hh_t, h_seq, h_n)
    state = _lstm_state_vectors(name, B, hidden, h_n, c_n, h0, c0)
    rows = min(pre.shape[0], h_seq.shape[0])
    if h_all is not None:
        _dev(h_all)
        _need(h_all.dtype == torch.float32 and h_all.dim() == 2 and h_all.shape[0] >= min_rows and
              h_all.shape[1] >= hidden and h_all.stride(1) == 1, f"{name}: h_all f32 [rows, >= H]")
        rows = min(rows, h_all.shape[0])
    d_row0 = d_len = None
    if lengths is not None:
        _ragged_inside(name, lengths, row0, rows, "pre / h_seq / h_all")
        d_row0, d_len = _ragged_tables(lengths, row0, pre.device)
    # W_hh is streamed once per step and group; from the zero state step 0 has no product
    steps = sum(n if state else max(n - 1, 0) for n in group_steps)
    timed("lstm_seq_fwd_state_kernel", "lstm_fwd", 4.0 * hidden * hidden * 4 * steps, "byte", _lib.call,
          "vc_lstm_seq_fwd_state", _p(pre), pre.stride(0), B, _p(d_row0) if d_row0 is not None else None,
          _p(d_len) if d_len is not None else None, max_len, hidden, _p(w_hh_t), _p(h0) if state else None,
          _p(c0) if state else None, _p(h_seq), h_seq.stride(0), _p(h_all) if h_all is not None else None,
          h_all.stride(0) if h_all is not None else 0, _p(h_n), _p(c_n), _stream(pre))
    return h_n, c_n


def lstm_seq_bwd(gates: torch.Tensor, c_seq: torch.Tensor, B: int, T: int, hidden: int, w_hh: torch.Tensor,
                 dh: torch.Tensor, dpre: torch.Tensor, dpre_bf16: torch.Tensor, last_only: bool = False,
                 keep: torch.Tensor | None = None) -> torch.Tensor:
    """BPTT of one LSTM layer from the saved gates / c_seq: dh f32 [B*T, H] (dL/dh_seq) or, with
    last_only, f32 [B, H] (dL/dh_last); w_hh f32 [4H, H] -> dpre f32 [B*T, 4H] and its bf16 copy."""
    _lstm_shape(B, T, hidden)
    M = B * T
    _dev(gates, c_seq, w_hh, dh, dpre, dpre_bf16)
    _need(gates.dtype == torch.float32 and gates.is_contiguous() and gates.shape[-1] == 4 * hidden and
          gates.numel() >= M * 4 * hidden, "lstm_seq_bwd: gates f32 contiguous [B*T, 4H]")
    _need(c_seq.dtype == torch.float32 and c_seq.is_contiguous() and c_seq.shape[-1] == hidden and
          c_seq.numel() >= M * hidden, "lstm_seq_bwd: c_seq f32 contiguous [B*T, H]")
    _need(w_hh.dtype == torch.float32 and w_hh.is_contiguous() and tuple(w_hh.shape) == (4 * hidden, hidden),
          "lstm_seq_bwd: w_hh f32 contiguous [4H, H]")
    _need(dh.dtype == torch.float32 and dh.dim() == 2 and dh.stride(1) == 1 and dh.shape[1] >= hidden and
          dh.shape[0] >= (B if last_only else M), "lstm_seq_bwd: dh f32 [B*T, H] ([B, H] with last_only)")
    _need(dpre.dtype == torch.float32 and dpre.is_contiguous() and dpre.shape[-1] == 4 * hidden and
          dpre.numel() >= M * 4 * hidden, "lstm_seq_bwd: dpre f32 contiguous [B*T, 4H]")
    _need(dpre_bf16.dtype == torch.bfloat16 and dpre_bf16.dim() == 2 and dpre_bf16.stride(1) == 1 and
          dpre_bf16.shape[0] >= M and dpre_bf16.shape[1] >= 4 * hidden, "lstm_seq_bwd: dpre_bf16 bf16 [>= B*T, >= 4H]")
    if keep is not None:
        _dev(keep)
        _need(keep.dtype == torch.float32 and keep.is_contiguous() and keep.numel() >= M * hidden and
              keep.shape[-1] == hidden, "lstm_seq_bwd: keep f32 contiguous [B*T, H]")
    ngroups = -(-B // lstm_group(hidden))
    timed("lstm_seq_bwd_kernel", "lstm_bwd", 4.0 * hidden * hidden * 4 * T * ngroups, "byte", _lib.call,
          "vc_lstm_seq_bwd", _p(gates), _p(c_seq), B, T, hidden, _p(w_hh), _p(dh), dh.stride(0), int(last_only),
          _p(keep) if keep is not None else None, _p(dpre), _p(dpre_bf16), dpre_bf16.stride(0), _stream(gates))
    return dpre


def lstm_seq_fwd_train_state(pre: torch.Tensor, lengths, hidden: int, w_hh_t: torch.Tensor, h_seq: torch.Tensor,
                             h_n: torch.Tensor, c_n: torch.Tensor, gates: torch.Tensor, c_seq: torch.Tensor,
                             h_prev: torch.Tensor, h0: torch.Tensor | None = None, c0: torch.Tensor | None = None,
                             keep: torch.Tensor | None = None, row0=None, T: int | None = None) -> tuple:
    """The train variant of lstm_seq_fwd_state (same layout, state and aliasing rules): also writes the saved
    tensors of lstm_seq_bwd_state, gates f32 [rows, 4H], c_seq f32 [rows, H] (both contiguous) and h_prev bf16
    [rows, >= H], whose row of a sequence's first step is bf16(h0) (zero without a state); keep f32 [rows, H]
    (optional, contiguous) scales the stored h_seq only.  Bit-identical to lstm_seq_fwd (train variant) from
    the zero state at full lengths, to lstm_seq_fwd_state in h_seq / h_n / c_n, and chunked to whole."""
    name = "lstm_seq_fwd_train_state"
    _need(isinstance(h_n, torch.Tensor) and h_n.dim() == 2, f"{name}: h_n f32 [B, H]")
    B = h_n.shape[0]
    lengths, row0, max_len, min_rows, group_steps = _lstm_state_layout(name, B, hidden, lengths, row0, T)
    _lstm_fwd_operands(name, "rows", min_rows, B, hidden, pre, w_hh_t, h_seq, h_n)
    state = _lstm_state_vectors(name, B, hidden, h_n, c_n, h0, c0)
    _dev(gates, c_seq, h_prev)
    rows = min(pre.shape[0], h_seq.shape[0])
    _need(gates.is_contiguous() and c_seq.is_contiguous(), f"{name}: gates and c_seq are contiguous")
    rows = min(rows, _lstm_state_rows(name, "gates f32", gates, torch.float32, min_rows, 4 * hidden),
               _lstm_state_rows(name, "c_seq f32", c_seq, torch.float32, min_rows, hidden),
               _lstm_state_rows(name, "h_prev bf16", h_prev, torch.bfloat16, min_rows, hidden))
    _need(gates.shape[1] == 4 * hidden and c_seq.shape[1] == hidden, f"{name}: gates f32 [rows, 4H], c_seq f32 [rows, H]")
    if keep is not None:
        _dev(keep)
        _need(keep.is_contiguous() and keep.shape[-1] == hidden, f"{name}: keep f32 contiguous [rows, H]")
        rows = min(rows, _lstm_state_rows(name, "keep f32", keep, torch.float32, min_rows, hidden))
    d_row0 = d_len = None
    if lengths is not None:
        _ragged_inside(name, lengths, row0, rows, "pre / h_seq / gates / c_seq / h_prev / keep")
        d_row0, d_len = _ragged_tables(lengths, row0, pre.device)
    steps = sum(n if state else max(n - 1, 0) for n in group_steps)
    timed("lstm_seq_fwd_train_state_kernel", "lstm_fwd", 4.0 * hidden * hidden * 4 * steps, "byte", _lib.call,
          "vc_lstm_seq_fwd_train_state", _p(pre), pre.stride(0), B, _p(d_row0) if d_row0 is not None else None,
          _p(d_len) if d_len is not None else None, max_len, hidden, _p(w_hh_t), _p(h0) if state else None,
          _p(c0) if state else None, _p(keep) if keep is not None else None, _p(h_seq), h_seq.stride(0), _p(h_n), _p(c_n),
          _p(gates), _p(c_seq), _p(h_prev), h_prev.stride(0), _stream(pre))
    return h_n, c_n


def lstm_seq_bwd_state(gates: torch.Tensor, c_seq: torch.Tensor, B: int, lengths, hidden: int, w_hh: torch.Tensor,
                       dpre: torch.Tensor, dpre_bf16: torch.Tensor, dh_seq: torch.Tensor | None = None,
                       dh_n: torch.Tensor | None = None, dc_n: torch.Tensor | None = None,
                       c0: torch.Tensor | None = None, keep: torch.Tensor | None = None,
                       dh0: torch.Tensor | None = None, dc0: torch.Tensor | None = None, row0=None,
                       T: int | None = None) -> torch.Tensor:
    """BPTT of lstm_seq_fwd_train_state from its gates / c_seq, over the same layout (lengths + row0, or
    lengths=None and T).  Incoming, each optional: dh_seq f32 [rows, >= H] (times keep f32 [rows, H] when
    given), dh_n and dc_n f32 [B, H] (never masked; they enter at each sequence's last step).  c0 f32 [B, H]
    is the state the forward started from (None: zeros).  Writes dpre f32 [rows, 4H] and dpre_bf16 for the
    rows of the sequences only; dh0 / dc0 f32 [B, H] (both or neither) get the gradient of the incoming
    state, dh_n / dc_n passed through for a sequence of length 0.  dh0 may be dh_n and dc0 may be dc_n."""
    name = "lstm_seq_bwd_state"
    _need(isinstance(B, int) and B >= 1, f"{name}: B must be an int >= 1")
    lengths, row0, max_len, min_rows, group_steps = _lstm_state_layout(name, B, hidden, lengths, row0, T)
    _dev(gates, c_seq, w_hh, dpre, dpre_bf16)
    _need(gates.is_contiguous() and c_seq.is_contiguous() and dpre.is_contiguous(),
          f"{name}: gates, c_seq and dpre are contiguous")
    rows = min(_lstm_state_rows(name, "gates f32", gates, torch.float32, min_rows, 4 * hidden),
               _lstm_state_rows(name, "c_seq f32", c_seq, torch.float32, min_rows, hidden),
               _lstm_state_rows(name, "dpre f32", dpre, torch.float32, min_rows, 4 * hidden),
               _lstm_state_rows(name, "dpre_bf16 bf16", dpre_bf16, torch.bfloat16, min_rows, 4 * hidden))
    _need(gates.shape[1] == 4 * hidden and c_seq.shape[1] == hidden and dpre.shape[1] == 4 * hidden,
          f"{name}: gates and dpre f32 [rows, 4H], c_seq f32 [rows, H]")
    _need(w_hh.dtype == torch.float32 and w_hh.is_contiguous() and tuple(w_hh.shape) == (4 * hidden, hidden),
          f"{name}: w_hh f32 contiguous [4H, H]")
    if dh_seq is not None:
        _dev(dh_seq)
        rows = min(rows, _lstm_state_rows(name, "dh_seq f32", dh_seq, torch.float32, min_rows, hidden))
    if keep is not None:
        _dev(keep)
        _need(keep.is_contiguous() and keep.shape[-1] == hidden, f"{name}: keep f32 contiguous [rows, H]")
        rows = min(rows, _lstm_state_rows(name, "keep f32", keep, torch.float32, min_rows, hidden))
    _need((dh0 is None) == (dc0 is None), f"{name}: dh0 and dc0 come together (both None: not wanted)")
    vecs = [t for t in (dh_n, dc_n, c0, dh0, dc0) if t is not None]
    _dev(*vecs)
    for t in vecs:
        _need(t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (B, hidden),
              f"{name}: c0, dh_n, dc_n, dh0 and dc0 are f32 contiguous [B, H]")
    span = B * hidden * 4
    for a, b, ok in ((dh0, dc0, False), (dh0, dc_n, False), (dc0, dh_n, False), (dh0, c0, False), (dc0, c0, False),
                     (dh0, dh_n, True), (dc0, dc_n, True)):
        if a is not None and b is not None and abs(_p(a) - _p(b)) < span:
            _need(ok and _p(a) == _p(b), f"{name}: dh0 may alias dh_n and dc0 may alias dc_n exactly, nothing else")
    d_row0 = d_len = None
    if lengths is not None:
        _ragged_inside(name, lengths, row0, rows, "gates / c_seq / dpre / dpre_bf16 / dh_seq / keep")
        d_row0, d_len = _ragged_tables(lengths, row0, gates.device)
    o = lambda t: _p(t) if t is not None else None  # noqa: E731
    steps = sum(n if dh0 is not None else max(n - 1, 0) for n in group_steps)  # W_hh is streamed once per product
    timed("lstm_seq_bwd_state_kernel", "lstm_bwd", 4.0 * hidden * hidden * 4 * steps, "byte", _lib.call,
          "vc_lstm_seq_bwd_state", _p(gates), _p(c_seq), o(c0), B, o(d_row0), o(d_len), max_len, hidden, _p(w_hh), o(dh_seq),
          dh_seq.stride(0) if dh_seq is not None else 0, o(keep), o(dh_n), o(dc_n), _p(dpre), _p(dpre_bf16),
          dpre_bf16.stride(0), o(dh0), o(dc0), _stream(gates))
    return dpre


def _f32c(name, *ts):
    for t in ts:
        _need(t.dtype == torch.float32 and t.is_contiguous(), f"{name}: f32 contiguous tensors")


def mlp_head_fwd(h: torch.Tensor, w1, b1, w2, b2, logits: torch.Tensor, keep: torch.Tensor | None = None,
                 hid: torch.Tensor | None = None) -> torch.Tensor:
    """logits[B, nl] = W2 (relu(W1 h + b1) * keep) + b2 on f32 h [B, H]; hid f32 [B, H1] (optional) is
    the masked hidden row the backward needs."""
    opt = [t for t in (keep, hid) if t is not None]
    _dev(h, w1, b1, w2, b2, logits, *opt)
    _f32c("mlp_head_fwd", h, w1, b1, w2, b2, logits, *opt)
    B, H = h.shape
    H1, nl = w1.shape[0], w2.shape[0]
    _need(B >= 1 and 0 < H <= 1024 and 0 < H1 <= 1024 and 0 < nl <= 1024, "mlp_head_fwd: B >= 1; H, H1, labels <= 1024")
    _need(tuple(w1.shape) == (H1, H) and b1.numel() == H1 and tuple(w2.shape) == (nl, H1) and b2.numel() == nl and
          tuple(logits.shape) == (B, nl), "mlp_head_fwd shapes")
    _need(all(tuple(t.shape) == (B, H1) for t in opt), "mlp_head_fwd: keep / hid f32 [B, H1]")
    timed("mlp_head_fwd_kernel", "head", (B * H + H1 * H) * 4, "byte", _lib.call, "vc_mlp_head_fwd", _p(h), B, H, _p(w1),
          _p(b1), H1, _p(keep) if keep is not None else None, _p(w2), _p(b2), nl, _p(hid) if hid is not None else None,
          _p(logits), _stream(h))
    return logits


def mlp_head_bwd(h, w1, w2, hid, keep, dlogits, dh, dw1, db1, dw2, db2):
    """Backward of mlp_head_fwd from dlogits f32 [B, nl] and the saved hid (keep may be None)."""
    opt = [keep] if keep is not None else []
    _dev(h, w1, w2, hid, dlogits, dh, dw1, db1, dw2, db2, *opt)
    _f32c("mlp_head_bwd", h, w1, w2, hid, dlogits, dh, dw1, db1, dw2, db2, *opt)
    B, H = h.shape
    H1, nl = w1.shape[0], w2.shape[0]
    _need(B >= 1 and 0 < H <= 1024 and 0 < H1 <= 1024 and 0 < nl <= 1024, "mlp_head_bwd: B >= 1; H, H1, labels <= 1024")
    _need(tuple(w1.shape) == (H1, H) and tuple(w2.shape) == (nl, H1) and tuple(hid.shape) == (B, H1) and
          tuple(dlogits.shape) == (B, nl) and tuple(dh.shape) == (B, H) and tuple(dw1.shape) == (H1, H) and
          db1.numel() == H1 and tuple(dw2.shape) == (nl, H1) and db2.numel() == nl and
          all(tuple(t.shape) == (B, H1) for t in opt), "mlp_head_bwd shapes")
    timed("mlp_head_bwd_kernel", "head_bwd", (2 * B * H + 2 * H1 * H) * 4, "byte", _lib.call, "vc_mlp_head_bwd", _p(h),
          _p(w1), _p(w2), _p(hid), _p(keep) if keep is not None else None, _p(dlogits), B, H, H1, nl, _p(dh), _p(dw1),
          _p(db1), _p(dw2), _p(db2), _stream(h))
    return dh


# ---- saliency faithfulness (csrc/perturb.hip; vclip_amd/faithfulness.py) ----
CLIP_LAYOUT = {"btchw": 0, "bcthw": 1}
PERTURB_MODE = {"deletion": 0, "insertion": 1}


def gaussian_taps(ksize: int, sigma: float) -> torch.Tensor:
    """The f32 taps vc_gaussian_blur_planes uses: exp(-d^2 / (2 sigma^2)) / sum, d = j - ksize // 2, in double in j
    order, then rounded (host tensor [ksize]; `sigma` is taken at f32 precision, as the C-ABI receives it)."""
    import math
    s = float(torch.tensor(float(sigma), dtype=torch.float32))
    w = [math.exp(-(float(j - ksize // 2) ** 2) / (2.0 * s * s)) for j in range(ksize)]
    tot = 0.0
    for v in w:
        tot += v
    return torch.tensor([v / tot for v in w], dtype=torch.float64).float()


def perturb_clips(clip: torch.Tensor, rank: torch.Tensor, k: torch.Tensor, grid, layout: str, mode: str,
                  base: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """The F perturbed copies of a clip batch in one launch (vc_perturb_clips).  clip f32 [B,T,C,H,W] (layout "btchw")
    or [B,C,T,H,W] ("bcthw"); base the same shape, or None for 0.0; rank int32 [B, Tg*Hg*Wg], the position of every
    cell of `grid` = (Tg, Hg, Wg) in the order of removal; k int32 [F].  Pixel (t, y, x) is in cell
    ((t*Tg//T)*Hg + y*Hg//H)*Wg + x*Wg//W.  out f32 [F, *clip.shape]: mode "deletion" takes base where rank < k[f] and
    the clip elsewhere, "insertion" the reverse; the values are copied bit for bit."""
    opt = [t for t in (base, out) if t is not None]
    _dev(clip, rank, k, *opt)
    _need(layout in CLIP_LAYOUT, f"perturb_clips: layout must be one of {sorted(CLIP_LAYOUT)}")
    _need(mode in PERTURB_MODE, f"perturb_clips: mode must be one of {sorted(PERTURB_MODE)}")
    _need(clip.dtype == torch.float32 and clip.dim() == 5 and clip.is_contiguous(), "perturb_clips: clip f32 contiguous, 5-D")
    B = clip.shape[0]
    (T, C) = (clip.shape[1], clip.shape[2]) if layout == "btchw" else (clip.shape[2], clip.shape[1])
    H, W = clip.shape[3], clip.shape[4]
    _need(len(grid) == 3 and all(isinstance(g, int) and g > 0 for g in grid), "perturb_clips: grid = (Tg, Hg, Wg), positive ints")
    Tg, Hg, Wg = grid
    _need(Tg <= T and Hg <= H and Wg <= W, f"perturb_clips: grid {tuple(grid)} larger than the clip's {(T, H, W)}")
    _need(rank.dtype == torch.int32 and rank.is_contiguous() and tuple(rank.shape) == (B, Tg * Hg * Wg),
          "perturb_clips: rank int32 [B, Tg*Hg*Wg]")
    _need(k.dtype == torch.int32 and k.is_contiguous() and k.dim() == 1 and k.numel() >= 1, "perturb_clips: k int32 [F]")
    _need(base is None or (base.dtype == torch.float32 and base.is_contiguous() and base.shape == clip.shape),
          "perturb_clips: base f32 contiguous, the clip's shape")
    F = k.numel()
    if out is None:
        out = torch.empty((F,) + tuple(clip.shape), dtype=torch.float32, device=clip.device)
    _need(out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (F,) + tuple(clip.shape),
          "perturb_clips: out f32 contiguous [F, *clip.shape]")
    _need(len({t.device for t in (clip, rank, k, out, *opt)}) == 1, "perturb_clips: all tensors on one device")
    _lib.call("vc_perturb_clips", _p(clip), None if base is None else _p(base), _p(rank), _p(k), B, C, T, H, W,
              CLIP_LAYOUT[layout], Tg, Hg, Wg, F, PERTURB_MODE[mode], _p(out), _stream(clip))
    return out


def gaussian_blur_planes(x: torch.Tensor, ksize: int = 11, sigma: float = 5.0, out: torch.Tensor | None = None,
                         work: torch.Tensor | None = None) -> torch.Tensor:
    """Separable Gaussian blur with replicated edges over the last two dimensions of x f32 [..., H, W]
    (vc_gaussian_blur_planes; taps: gaussian_taps(ksize, sigma)); ksize odd and <= 31.  out / work: f32 buffers of
    x's size (allocated when absent); x is left unchanged."""
    opt = [t for t in (out, work) if t is not None]
    _dev(x, *opt)
    _need(x.dtype == torch.float32 and x.dim() >= 2 and x.is_contiguous() and x.numel() > 0,
          "gaussian_blur_planes: x f32 contiguous [..., H, W], not empty")
    _need(isinstance(ksize, int) and 1 <= ksize <= 31 and ksize % 2 == 1, "gaussian_blur_planes: ksize odd and <= 31")
    _need(float(sigma) > 0 and float(sigma) != float("inf"), "gaussian_blur_planes: sigma must be positive and finite")
    if out is None:
        out = torch.empty_like(x)
    if work is None:
        work = torch.empty_like(x)
    _need(out.dtype == torch.float32 and out.is_contiguous() and out.shape == x.shape,
          "gaussian_blur_planes: out f32 contiguous, x's shape")
    _need(work.dtype == torch.float32 and work.is_contiguous() and work.numel() >= x.numel(),
          "gaussian_blur_planes: work f32 contiguous, at least x's size")
    _need(len({t.device for t in (x, out, work)}) == 1, "gaussian_blur_planes: all tensors on one device")
    H, W = x.shape[-2], x.shape[-1]
    _lib.call("vc_gaussian_blur_planes", _p(x), x.numel() // (H * W), H, W, ksize, float(sigma), _p(out), _p(work),
              _stream(x))
    return out


# ---- RISE saliency (csrc/rise.hip; vclip_amd/rise.py) ----
def rise_mask_tile() -> int:
    """The most masks vc_rise_apply / vc_rise_accumulate stage in LDS per round (no result depends on it)."""
    return int(_lib.load().vc_rise_mask_tile())


def _rise_masks(name: str, bits: torch.Tensor, shifts: torch.Tensor, cells, T: int, H: int, W: int) -> int:
    """checks cells, bits uint8 [F, ct+2, ch+2, cw+2] and shifts int32 [F, 3] against the extent; returns F"""
    _need(len(cells) == 3 and all(isinstance(c, int) and not isinstance(c, bool) and c > 0 for c in cells),
          f"{name}: cells = (ct, ch, cw), positive ints")
    ct, ch, cw = cells
    _need(ct <= T and ch <= H and cw <= W, f"{name}: cells {tuple(cells)} larger than the clip's {(T, H, W)}")
    _need(bits.dtype == torch.uint8 and bits.is_contiguous() and bits.dim() == 4 and bits.shape[0] >= 1 and
          tuple(bits.shape[1:]) == (ct + 2, ch + 2, cw + 2), f"{name}: bits uint8 contiguous [F, ct+2, ch+2, cw+2]")
    F = bits.shape[0]
    _need(shifts.dtype == torch.int32 and shifts.is_contiguous() and tuple(shifts.shape) == (F, 3),
          f"{name}: shifts int32 contiguous [F, 3]")
    return F


def rise_apply(clip: torch.Tensor, bits: torch.Tensor, shifts: torch.Tensor, cells, layout: str,
               base: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """The clip batch under F RISE masks in one launch (vc_rise_apply).  clip f32 [B,T,C,H,W] (layout "btchw") or
    [B,C,T,H,W] ("bcthw"); base the same shape, or None for 0.0; bits uint8 [F, ct+2, ch+2, cw+2] and shifts int32
    [F, 3] as vclip_amd.rise.rise_masks draws them for `cells` = (ct, ch, cw) (every shift must lie in [0, S): the
    kernel does not check the values).  out f32 [F, *clip.shape] = fmaf(m, clip, (1 - m) * base), m the mask's
    trilinear interpolation at the pixel, the same for every clip and channel."""
    opt = [t for t in (base, out) if t is not None]
    _dev(clip, bits, shifts, *opt)
    _need(layout in CLIP_LAYOUT, f"rise_apply: layout must be one of {sorted(CLIP_LAYOUT)}")
    _need(clip.dtype == torch.float32 and clip.dim() == 5 and clip.is_contiguous(), "rise_apply: clip f32 contiguous, 5-D")
    B = clip.shape[0]
    (T, C) = (clip.shape[1], clip.shape[2]) if layout == "btchw" else (clip.shape[2], clip.shape[1])
    H, W = clip.shape[3], clip.shape[4]
    F = _rise_masks("rise_apply", bits, shifts, cells, T, H, W)
    _need(base is None or (base.dtype == torch.float32 and base.is_contiguous() and base.shape == clip.shape),
          "rise_apply: base f32 contiguous, the clip's shape")
    if out is None:
        out = torch.empty((F,) + tuple(clip.shape), dtype=torch.float32, device=clip.device)
    _need(out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (F,) + tuple(clip.shape),
          "rise_apply: out f32 contiguous [F, *clip.shape]")
    _need(len({t.device for t in (clip, bits, shifts, out, *opt)}) == 1, "rise_apply: all tensors on one device")
    _lib.call("vc_rise_apply", _p(clip), None if base is None else _p(base), _p(bits), _p(shifts), B, C, T, H, W,
              CLIP_LAYOUT[layout], cells[0], cells[1], cells[2], F, _p(out), _stream(clip))
    return out


def rise_accumulate(acc: torch.Tensor, bits: torch.Tensor, shifts: torch.Tensor, w: torch.Tensor, cells) -> torch.Tensor:
    """acc f32 [B, T, H, W] += sum over the F masks, in index order, of w[f][b] * m_f, one fmaf per mask
    (vc_rise_accumulate; in place, returns acc).  w f32 [F, B]; bits, shifts and cells as rise_apply takes them.  Any
    split of the masks into consecutive calls gives the same bits as one call."""
    _dev(acc, bits, shifts, w)
    _need(acc.dtype == torch.float32 and acc.dim() == 4 and acc.is_contiguous() and acc.numel() > 0,
          "rise_accumulate: acc f32 contiguous [B, T, H, W]")
    B, T, H, W = acc.shape
    F = _rise_masks("rise_accumulate", bits, shifts, cells, T, H, W)
    _need(w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape) == (F, B), "rise_accumulate: w f32 contiguous [F, B]")
    _need(len({t.device for t in (acc, bits, shifts, w)}) == 1, "rise_accumulate: all tensors on one device")
    _lib.call("vc_rise_accumulate", _p(bits), _p(shifts), _p(w), B, T, H, W, cells[0], cells[1], cells[2], F, _p(acc),
              _stream(acc))
    return acc
