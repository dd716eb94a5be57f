"""CPU-side checks of RISE saliency: the host sampler of vclip_amd/rise.py, the float64 reference's own properties
(tests/rise_ref.py), the planted scorer on the reference, the entry points of csrc/rise.hip (declared, exported, signed,
refusing bad arguments before any HIP call), rise_map refusing instead of falling back, and the `rise` flags of the four
clip families' inference parsers."""
import ctypes

import pytest
import torch

import rise_ref as R
import vclip_amd._lib as L
from vclip_amd import ops
from vclip_amd.build import LIB_PATH, build
from vclip_amd.rise import cell_sizes, rise_masks

APPLY, ACCUMULATE, TILE = "vc_rise_apply", "vc_rise_accumulate", "vc_rise_mask_tile"
TINY = dict(image_size=64, num_frames=4, tubelet_size=[2, 16, 16], num_channels=3, hidden_size=128,
            num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, hidden_act="gelu_fast",
            layer_norm_eps=1e-6, qkv_bias=True)
BASE = ["--video_path", "x.npy", "--model_path", "y.pth"]
GEOMS = [(4, 32, 32, (2, 4, 4)), (4, 50, 70, (2, 3, 4)), (3, 7, 5, (3, 7, 5)), (8, 64, 64, (1, 1, 1))]  # T, H, W, cells


# ------------------------------------------------------------------ the sampler
@pytest.mark.parametrize("T,H,W,cells", GEOMS)
def test_sampler_shapes_ranges_and_seeding(T, H, W, cells):
    bits, shifts = rise_masks(T, H, W, cells, 0.5, 64, seed=3)
    assert bits.dtype == torch.uint8 and tuple(bits.shape) == (64, cells[0] + 2, cells[1] + 2, cells[2] + 2)
    assert shifts.dtype == torch.int32 and tuple(shifts.shape) == (64, 3)
    assert bits.is_contiguous() and shifts.is_contiguous() and int(bits.max()) <= 1
    S = cell_sizes(T, H, W, cells)
    assert S == R.cell_sizes(T, H, W, cells) == tuple(-(-n // c) for n, c in zip((T, H, W), cells))
    for a in range(3):
        assert int(shifts[:, a].min()) >= 0 and int(shifts[:, a].max()) < S[a]
        if S[a] == 1:
            assert not shifts[:, a].any()  # a one-pixel cell has nowhere to shift
        elif S[a] >= 4:
            assert len(set(shifts[:, a].tolist())) > 1
    again = rise_masks(T, H, W, cells, 0.5, 64, seed=3)
    assert torch.equal(bits, again[0]) and torch.equal(shifts, again[1])
    other = rise_masks(T, H, W, cells, 0.5, 64, seed=4)
    assert not torch.equal(bits, other[0])
    ref = R.sample(T, H, W, cells, 0.5, 64, 3)  # the documented drawing order, written a second time
    assert torch.equal(bits, ref[0]) and torch.equal(shifts, ref[1])


def test_sampler_keep_and_default_temporal_cells():
    for keep in (0.1, 0.5, 0.9):
        bits, _ = rise_masks(8, 32, 32, (2, 7, 7), keep, 500, seed=0)
        assert abs(float(bits.float().mean()) - keep) < 0.01  # 162000 bits: 8 sigma at keep = 0.5
    assert rise_masks(32, 16, 16, (None, 4, 4), 0.5, 2)[0].shape[1] == 32 // 8 + 2
    assert rise_masks(4, 16, 16, (None, 4, 4), 0.5, 2)[0].shape[1] == 1 + 2  # max(1, T // 8)
    for bad in (dict(cells=(2, 4)), dict(cells=(0, 4, 4)), dict(cells=(5, 4, 4)), dict(cells=(2, 17, 4)), dict(cells=(2, 4, 2.0)),
                dict(keep=0.0), dict(keep=1.0), dict(keep=True), dict(masks=0), dict(masks=2.5), dict(seed=1.5)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            rise_masks(**dict(dict(T=4, H=16, W=16, cells=(2, 4, 4), keep=0.5, masks=4, seed=0), **bad))


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("T,H,W,cells", GEOMS)
def test_reference_mask_properties(T, H, W, cells):
    bits, shifts = R.sample(T, H, W, cells, 0.5, 8, 0)
    m = R.masks_all(bits, shifts, T, H, W, cells)
    assert m.dtype == torch.float64 and tuple(m.shape) == (8, T, H, W)
    assert float(m.min()) >= 0.0 and float(m.max()) <= 1.0
    ones, zeros = torch.ones_like(bits), torch.zeros_like(bits)
    assert bool((R.masks_all(ones, shifts, T, H, W, cells) == 1.0).all())
    assert bool((R.masks_all(zeros, shifts, T, H, W, cells) == 0.0).all())
    for n in range(8):  # where the eight corners agree the mask is that bit
        same = R.corners_equal(bits, shifts, n, T, H, W, cells)
        assert bool(((m[n] == 0.0) | (m[n] == 1.0))[same].all())
    if cell_sizes(T, H, W, cells) == (1, 1, 1):  # no shift, no fraction: the mask is the bit grid's own corner block
        assert torch.equal(m, bits[:, :T, :H, :W].double())
    clip = torch.randn(2, 3, T, H, W, generator=torch.Generator().manual_seed(0))
    base = torch.randn(2, 3, T, H, W, generator=torch.Generator().manual_seed(1))
    assert torch.equal(R.apply(clip, base, R.masks_all(ones, shifts, T, H, W, cells), "bcthw")[0], clip.double())
    assert torch.equal(R.apply(clip, base, R.masks_all(zeros, shifts, T, H, W, cells), "bcthw")[0], base.double())
    w = torch.rand(8, 2, generator=torch.Generator().manual_seed(2))
    whole = R.accumulate(torch.zeros(2, T, H, W), m, w)
    parts = R.accumulate(R.accumulate(torch.zeros(2, T, H, W), m[:3], w[:3]), m[3:], w[3:])
    assert float((whole - parts).abs().max()) <= 1e-14 * float(whole.abs().max())


def test_planted_scorer_on_the_reference():
    """A clip of ones whose score is the masked clip's mean inside a fixed box: RISE must point at the box."""
    bits, shifts, scores, sal = R.planted(R.PLANTED_SEED)
    assert tuple(bits.shape) == (256, 4, 6, 6) and tuple(scores.shape) == (256, 1) and tuple(sal.shape) == (1, 4, 32, 32)
    assert R.planted_holds(sal)
    assert not R.planted_holds(torch.flip(sal, dims=(2, 3)).roll(12, dims=3))  # the check can fail


# ------------------------------------------------------------------ the C-ABI
def test_symbols_declared_exported_and_signed():
    build()
    raw = ctypes.CDLL(LIB_PATH)
    for name, nargs in ((APPLY, 16), (ACCUMULATE, 13), (TILE, 0)):
        assert name in L.header_functions() and hasattr(raw, name)
        argtypes, restype = L.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs
        assert nargs == 0 or argtypes[-1] is ctypes.c_void_p  # the stream last
    assert ops.rise_mask_tile() >= 1


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    build()
    lib = L.load()
    err = lambda: lib.vc_last_error().decode()  # noqa: E731
    clip, base, bits, shifts, out, w = (ctypes.c_void_p(a << 24) for a in (1, 2, 3, 4, 5, 6))

    def apply(**kw):
        # (clip, base, bits, shifts, B, C, T, H, W, layout, ct, ch, cw, F, out, stream)
        d = dict(clip=clip, base=base, bits=bits, shifts=shifts, B=1, C=3, T=4, H=8, W=8, layout=0, ct=2, ch=2, cw=2, F=3,
                 out=out)
        d.update(kw)
        return getattr(lib, APPLY)(*d.values(), None)

    def accumulate(**kw):
        # (bits, shifts, w, B, T, H, W, ct, ch, cw, F, acc, stream)
        d = dict(bits=bits, shifts=shifts, w=w, B=1, T=4, H=8, W=8, ct=2, ch=2, cw=2, F=3, acc=out)
        d.update(kw)
        return getattr(lib, ACCUMULATE)(*d.values(), None)

    for nm in ("clip", "bits", "shifts", "out"):
        assert apply(**{nm: None}) != 0 and "null" in err()
    for nm in ("bits", "shifts", "w", "acc"):
        assert accumulate(**{nm: None}) != 0 and "null" in err()
    for layout in (2, -1):
        assert apply(layout=layout) != 0 and "layout" in err()
    for nm in ("B", "C", "T", "H", "W", "F"):
        assert apply(**{nm: 0}) != 0 and "shape" in err()
    for nm in ("B", "T", "H", "W", "F"):
        assert accumulate(**{nm: 0}) != 0 and "shape" in err()
    for f in (apply, accumulate):
        for kw in (dict(ct=5), dict(ch=9), dict(cw=9), dict(ct=0), dict(ch=-1), dict(cw=0)):
            assert f(**kw) != 0 and "cells" in err()
        assert f(H=256, W=256, ch=200, cw=200) != 0 and "bit grid" in err()  # 4 * 202 * 202 bytes do not fit the LDS tile
        assert f(H=5000, W=5000) != 0 and "cell sizes" in err()  # 2 + 2500 + 2500 fractions do not fit the LDS table
        assert f(B=1 << 20, H=64, W=64) != 0 and "2^31" in err()
    assert apply(clip=ctypes.c_void_p((1 << 24) + 2)) != 0 and "aligned" in err()
    assert accumulate(acc=ctypes.c_void_p((5 << 24) + 2)) != 0 and "aligned" in err()
    n = 1 * 3 * 4 * 8 * 8 * 4  # bytes of one copy
    for kw in (dict(out=clip), dict(out=ctypes.c_void_p((1 << 24) + n - 4)), dict(out=ctypes.c_void_p((1 << 24) - 3 * n + 4)),
               dict(out=base), dict(out=bits), dict(out=shifts)):
        assert apply(**kw) != 0 and "alias" in err()
    for kw in (dict(acc=bits), dict(acc=shifts), dict(acc=w)):
        assert accumulate(**kw) != 0 and "alias" in err()


def test_op_wrappers_reject_cpu_tensors():
    bits, shifts = rise_masks(4, 8, 8, (2, 2, 2), 0.5, 3)
    with pytest.raises(L.VclipError):
        ops.rise_apply(torch.zeros(1, 4, 3, 8, 8), bits, shifts, (2, 2, 2), "btchw")
    with pytest.raises(L.VclipError):
        ops.rise_accumulate(torch.zeros(1, 4, 8, 8), bits, shifts, torch.ones(3, 1), (2, 2, 2))


# ------------------------------------------------------------------ rise_map
def test_rise_map_refusals_on_the_cpu():
    import vclip_amd
    from vclip_amd.rise import RiseExplanation, rise_map
    from vclip_amd.vivit import Explanation, VivitConfig, VivitForVideoClassification
    assert vclip_amd.rise_map is rise_map and vclip_amd.RiseExplanation is RiseExplanation
    assert issubclass(RiseExplanation, Explanation)
    m = VivitForVideoClassification(VivitConfig(**TINY)).eval()
    pix = torch.zeros(2, 4, 3, 64, 64)
    with pytest.raises(RuntimeError, match="GPU only"):
        rise_map(m, pix)
    with pytest.raises(RuntimeError, match="GPU only"):
        rise_map(m, pix, target=[0, 1], masks=8, cells=(2, 4, 4), keep=0.3, baseline="blur", seed=5, chunk=4)
    for kw in (dict(cells=(2, 7)), dict(cells=(5, 7, 7)), dict(cells=(None, 0, 7)), dict(cells=(None, 7, 65)),
               dict(cells=(1, 7.0, 7)), dict(keep=0.0), dict(keep=1.0), dict(keep=-0.5), dict(keep="half"), dict(masks=0),
               dict(masks=-4), dict(masks=2.5), dict(masks=True), dict(chunk=0), dict(chunk=1.5), dict(chunk=True),
               dict(baseline="mean"), dict(seed=0.5)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            rise_map(m, pix, **kw)
    for target in (2, [0], 0.5):
        with pytest.raises(ValueError, match="target"):
            rise_map(m, pix, target=target)
    with pytest.raises(ValueError, match="clip"):
        rise_map(m, pix[0])
    with pytest.raises(TypeError, match="family"):
        rise_map(torch.nn.Linear(2, 2).eval(), pix)
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        rise_map(m, pix)


# ------------------------------------------------------------------ the parsers
@pytest.mark.parametrize("fam", ["vivit", "timesformer", "swin", "resnet3d"])
def test_rise_flags(fam):
    from vclip_amd.apps import CLASS_SPECIFIC_SALIENCY, FAMILIES, build_parser
    p = build_parser(FAMILIES[fam], inference=True, saliency=True)
    a = p.parse_args(BASE + ["--saliency", "rise"])
    assert a.saliency == "rise" and a.rise_masks == 4000 and a.rise_seed == 0 and a.saliency_class is None
    a = p.parse_args(BASE + ["--saliency", "rise", "--rise_masks", "32", "--rise_seed", "7", "--saliency_class", "1"])
    assert (a.rise_masks, a.rise_seed, a.saliency_class) == (32, 7, 1)
    assert p.parse_args(BASE + ["--saliency", "rise", "--saliency_check", "4"]).saliency_check == 4
    for extra in (["--rise_masks", "0"], ["--rise_masks", "-3"], ["--rise_masks", "many"], ["--rise_seed", "x"]):
        with pytest.raises(SystemExit):
            p.parse_args(BASE + ["--saliency", "rise"] + extra)
    assert "rise" in CLASS_SPECIFIC_SALIENCY[fam]
    if fam in ("timesformer", "swin"):  # their other methods are not class-specific: refused while parsing
        for extra in (["--saliency", "rollout", "--saliency_class", "1"], ["--saliency_class", "1"]):
            with pytest.raises(SystemExit):
                p.parse_args(BASE + extra)
    two = build_parser(FAMILIES[fam], inference=True)  # the two-argument form keeps its flag surface
    for extra in (["--saliency", "rise"], ["--rise_masks", "8"], ["--rise_seed", "1"]):
        with pytest.raises(SystemExit):
            two.parse_args(BASE + extra)


def test_lstm_parser_has_no_rise():
    from vclip_amd.apps import FAMILIES, build_parser
    with pytest.raises(SystemExit):
        build_parser(FAMILIES["lstm"], inference=True, saliency=True).parse_args(
            ["--videos_dir", "d", "--model_path", "m.pth", "--saliency", "rise"])
