"""GEMM conformance matrix: every tile configuration of vc_gemm_h16 (csrc/gemm.hip: 3, 4, 5, 7, 8, 15,
20, 21 and the dispatcher, cfg = -1) against every epilogue it runs, at small shapes, on padded rows.

Reference: fp64 of the 16-bit-rounded operands, acc = a.double() @ w.double().T + bias.double(), with
the epilogue applied in torch.  One matmul per (M, N, K, type) is cached and shared by the epilogue and
configuration axes.

Guard bands: a, w, out and aux are views of larger buffers (extra rows, extra columns); the operands'
padding holds NaN, the outputs' padding NaN (overwriting epilogues) or a seeded random fill
(accumulating ones).  After a launch the [0, M) x [0, N) block must match the reference and hold no
NaN, and every padding element of out and aux must be bit-identical to what it held before: a k-column
read past K or an A row past M poisons the result, a store outside the block changes a sentinel.  All
padding lies inside the same allocation.

Tolerances are the ones the suite already states: bf16 outputs max |o - ref| / (|ref| + 1) < 8e-3, fp16
outputs < 1.2e-3, f32 outputs rtol = atol = 1e-4 (bias_add_f32 atol 2e-4), dgelu_tanh rtol 1e-2 atol
2e-2, the saved pre-activation atol 1.6e-2.  cfgs 4, 7, 8, 15, 20 and 21 run the same MFMA chain and
epilogue arithmetic per output as cfg 5 (gemm.hip), so each is also compared bit for bit with cfg 5 on
identical buffers; cfg 3 is compared with the reference only.
"""
import numpy as np
import pytest
import torch

from oracle.vivit_ref import gelu_fast

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, FP = torch.bfloat16, torch.float16
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vclip_amd import _lib as L
    L.load()


def ops():
    from vclip_amd import ops as O
    return O


def VclipError():
    from vclip_amd import _lib as L
    return L.VclipError


# ------------------------------------------------------------------------- the matrix
EPIS = ("bias", "bias_gelu_tanh", "bias_gelu_erf", "bias_resid_f32", "embed_f32", "bias_f32", "bias_relu",
        "bias_resid_relu", "bias_add_f32", "bias_gelu_tanh_save", "dgelu_tanh")
PLAIN16 = ("bias", "bias_gelu_tanh", "bias_gelu_erf", "bias_relu")
OUT16 = PLAIN16 + ("bias_resid_relu", "bias_gelu_tanh_save", "dgelu_tanh")
AUX_EPIS = ("embed_f32", "bias_resid_relu", "bias_add_f32", "bias_gelu_tanh_save", "dgelu_tanh")
F16_EPIS = EPIS[:5]  # fp16 operands: the inference epilogues 0 .. 4
TILE = {3: (256, 256), 4: (256, 256), 8: (256, 256), 15: (256, 256), 5: (128, 128), 7: (64, 128), 21: (64, 128)}
CFG_EPIS = {3: EPIS, 5: EPIS, 7: EPIS, 8: EPIS, 21: EPIS, 4: PLAIN16 + ("bias_gelu_tanh_save",), 15: PLAIN16,
            20: ("bias_resid_relu",)}
SAME_CHAIN_AS_5 = (4, 7, 8, 15, 20, 21)
C20_SHAPES = ((256, 512, 64), (256, 512, 128), (256, 384, 256))  # 2 x 2 tiles of 128 x 256, 2 x 3 of 128 x 128
K_SWEEP = {5: (64, 128, 192, 320), 7: (64, 128, 192, 320), 21: (64, 128, 192, 256, 320), 3: (64, 128, 192, 256, 320),
           8: (128, 192, 256, 320, 448), 4: (192, 256, 320, 448), 15: (640, 704, 768)}
GROUP, GROUP_STRIDE, GROUP_OFFSET = 100, 101, 1  # embed_f32: row m -> (m // 100) * 101 + 1 + m % 100
TOL16 = {BF: 8e-3, FP: 1.2e-3}


def base_shape(cfg):
    """2 x 3 tiles of the config's own tile"""
    bm, bn = TILE[cfg]
    return 2 * bm, 3 * bn


def base_k(cfg):
    return 704 if cfg == 15 else 320


def cfg_epis(cfg, dtype):
    return [e for e in CFG_EPIS[cfg] if dtype == BF or e in F16_EPIS]


def tid(dtype):
    return "bf16" if dtype == BF else "fp16"


# ------------------------------------------------------------------------- operands and the fp64 reference
_CASES = {}
_BIG = {}


def operands(M, N, K, dtype, kind="rand", ka=None):
    """(a, w, bias, acc): 16-bit a [M, ka or K] ~ N(0, 1), w [N, K] ~ 0.05 N(0, 1), a per-column distinct f32
    bias and acc = a @ w.T + bias in fp64 (ka: a's columns wrap, a @ w[:, :ka].T + a[:, :K - ka] @ w[:, ka:].T).
    kind "onehot": a[m, (7 m + 3) % K] = 1, w[n, k] = (131 n + 17 k) % 97 - 48, zero bias -- exact in bf16 and
    fp16, acc[m, n] = w[n, (7 m + 3) % K].  Cached: the epilogue and config axes share one matmul."""
    key = (M, N, K, dtype, kind, ka)
    store = _BIG if M * N > (1 << 22) else _CASES
    if key in store:
        return store[key]
    if kind == "onehot":
        a = torch.zeros(M, K)
        a[torch.arange(M), (7 * torch.arange(M) + 3) % K] = 1.0
        a = a.to(dtype)
        w = ((131 * torch.arange(N)[:, None] + 17 * torch.arange(K)[None, :]) % 97 - 48).float().to(dtype)
        bias = torch.zeros(N)
    else:
        g = torch.Generator().manual_seed(M + 3 * N + 7 * K + (ka or 0))
        a = torch.randn(M, ka or K, generator=g).to(dtype)
        w = (torch.randn(N, K, generator=g) * 0.05).to(dtype)
        bias = torch.randn(N, generator=g) * 0.1
    ad, wd = a.double(), w.double()
    if ka is None:
        acc = ad @ wd.T
    else:
        acc = ad @ wd[:, :ka].T + ad[:, :K - ka] @ wd[:, ka:].T
    acc += bias.double()
    if store is _BIG:
        _BIG.clear()  # one large case at a time
    store[key] = (a, w, bias, acc)
    return store[key]


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


class Run:
    """One launch on guarded buffers: the buffers before and after (on the host) and where it may write."""


def launch(cfg, M, N, K, epi, dtype=BF, pado=None, padaux=None, kind="rand", ka=None, rejected=False):
    O = ops()
    a, w, bias, acc = operands(M, N, K, dtype, kind, ka)
    out16 = epi in OUT16
    odt = dtype if out16 else torch.float32
    if pado is None:
        pado = 8 if out16 else 4
    g = torch.Generator().manual_seed(1000 * EPIS.index(epi) + 7)

    def padded(t, rows, cols):
        buf = torch.full((t.shape[0] + rows, t.shape[1] + cols), NAN, dtype=t.dtype)
        buf[:t.shape[0], :t.shape[1]] = t
        return buf

    abuf = padded(a, 128, 64).to(DEV)
    wbuf = padded(w, 0, 64).to(DEV)
    av, wv = abuf[:M, :a.shape[1]], wbuf[:, :K]

    r = Run()
    r.M, r.N, r.epi, r.dtype, r.acc = M, N, epi, dtype, acc
    if epi == "embed_f32":
        m = torch.arange(M)
        r.dest = (m // GROUP) * GROUP_STRIDE + GROUP_OFFSET + m % GROUP
        out_rows = int(r.dest.max()) + 1
    else:
        r.dest = torch.arange(M)
        out_rows = M
    if epi == "bias_resid_f32":  # accumulates into out: a seeded fill, the residual inside the block
        out0 = torch.randn(out_rows + 128, N + pado, generator=g)
    else:
        out0 = torch.full((out_rows + 128, N + pado), NAN, dtype=odt)
    r.out0 = out0

    aux0 = None
    r.aux_written = False
    if epi in AUX_EPIS:
        adt = torch.float32 if epi in ("embed_f32", "bias_add_f32") else BF
        if padaux is None:
            padaux = 4 if adt == torch.float32 else 8
        arows = GROUP if epi == "embed_f32" else M
        if epi == "bias_gelu_tanh_save":  # written: NaN everywhere
            body = torch.full((arows, N), NAN, dtype=adt)
            r.aux_written = True
        elif epi == "dgelu_tanh":  # the bf16 pre-activation a forward GEMM saved
            body = acc.float().to(BF)
        else:
            body = torch.randn(arows, N, generator=g).to(adt)
        aux0 = padded(body, 128, padaux)
        r.arows = arows
    r.aux0 = aux0

    obuf = out0.to(DEV)
    xbuf = aux0.to(DEV) if aux0 is not None else None
    ov = obuf[:out_rows, :N]
    kw = {}
    if xbuf is not None:
        kw["aux"] = xbuf[:r.arows, :N]
    if epi == "embed_f32":
        kw.update(group=GROUP, group_stride=GROUP_STRIDE, group_offset=GROUP_OFFSET)

    def go():
        if ka is None:
            O.gemm(av, wv, bias.to(DEV), epi, ov, m=M, cfg=cfg, **kw)
        else:
            O.gemm_wrap(av, ka, wv, bias.to(DEV), epi, ov, m=M, **kw)

    if rejected:
        with pytest.raises(VclipError()):
            go()
    else:
        go()
    torch.cuda.synchronize()
    r.out = obuf.cpu()
    r.aux = xbuf.cpu() if xbuf is not None else None
    r.rejected = rejected
    return r


def check_guards(r):
    """every element outside the block the launch may write is bit-identical to what it held before"""
    keep = torch.ones(r.out.shape, dtype=torch.bool)
    if not r.rejected:
        keep[r.dest, :r.N] = False
    changed = int((_bits(r.out)[keep] != _bits(r.out0)[keep]).sum())
    assert changed == 0, f"{changed} elements of out changed outside [0, M) x [0, N)"
    if r.aux is not None:
        keep = torch.ones(r.aux.shape, dtype=torch.bool)
        if r.aux_written and not r.rejected:
            keep[:r.M, :r.N] = False
        changed = int((_bits(r.aux)[keep] != _bits(r.aux0)[keep]).sum())
        assert changed == 0, f"{changed} elements of aux changed outside what the epilogue writes"


def block(r):
    return r.out[r.dest][:, :r.N]


def reference(r):
    acc, epi, M, N = r.acc, r.epi, r.M, r.N
    if epi in ("bias", "bias_f32"):
        return acc
    if epi in ("bias_gelu_tanh", "bias_gelu_tanh_save"):
        return gelu_fast(acc)
    if epi == "bias_gelu_erf":
        return torch.nn.functional.gelu(acc)
    if epi == "bias_relu":
        return torch.relu(acc)
    if epi == "bias_resid_relu":
        return torch.relu(acc + r.aux0[:M, :N].double())
    if epi == "bias_resid_f32":
        return acc + r.out0[:M, :N].double()
    if epi == "bias_add_f32":
        return acc + r.aux0[:M, :N].double()
    if epi == "embed_f32":
        return acc + r.aux0[:GROUP, :N].double()[torch.arange(M) % GROUP]
    if epi == "dgelu_tanh":  # autograd of the tanh GELU on the saved bf16 pre-activation
        p = r.aux0[:M, :N].float().requires_grad_()
        gelu_fast(p).backward(torch.ones_like(p))
        return (acc.float() * p.grad).double()
    raise AssertionError(epi)


def check_reference(r):
    got = block(r)
    assert torch.isfinite(got).all(), "NaN / inf in the output block"
    ref = reference(r)
    if r.epi == "dgelu_tanh":
        np.testing.assert_allclose(got.float().numpy(), ref.float().numpy(), rtol=1e-2, atol=2e-2)
    elif r.epi in OUT16:
        err = ((got.double() - ref).abs() / (ref.abs() + 1.0)).max().item()
        assert err < TOL16[r.dtype], err
    else:
        np.testing.assert_allclose(got.double().numpy(), ref.numpy(), rtol=1e-4,
                                   atol=2e-4 if r.epi == "bias_add_f32" else 1e-4)
    if r.epi == "bias_gelu_tanh_save":
        pre = r.aux[:r.M, :r.N]
        assert torch.isfinite(pre).all()
        np.testing.assert_allclose(pre.float().numpy(), r.acc.float().to(BF).float().numpy(), rtol=0, atol=1.6e-2)


def conform(cfg, M, N, K, epi, dtype=BF, **kw):
    """launch, guard bands, reference; and cfg 5 bit for bit where the config runs cfg 5's chain"""
    r = launch(cfg, M, N, K, epi, dtype, **kw)
    check_guards(r)
    check_reference(r)
    if cfg in SAME_CHAIN_AS_5:
        r5 = launch(5, M, N, K, epi, dtype, **kw)
        diff = int((_bits(r.out) != _bits(r5.out)).sum())
        assert diff == 0, f"cfg {cfg} differs from cfg 5 in {diff} elements of out"
        if r.aux is not None:
            assert torch.equal(_bits(r.aux), _bits(r5.aux)), f"cfg {cfg} differs from cfg 5 in aux"
    return r


def reject(cfg, M, N, K, epi, dtype=BF, **kw):
    """the request raises VclipError and neither out nor aux is touched"""
    check_guards(launch(cfg, M, N, K, epi, dtype, rejected=True, **kw))


# ------------------------------------------------------------------------- 1 / 7: epilogue x config
CROSS = [(c, e, d) for d in (BF, FP) for c in (3, 4, 5, 7, 8, 15, 21) for e in cfg_epis(c, d)]


@pytest.mark.parametrize("cfg,epi,dtype", CROSS, ids=[f"cfg{c}-{e}-{tid(d)}" for c, e, d in CROSS])
def test_epilogue_config_cross(cfg, epi, dtype):
    conform(cfg, *base_shape(cfg), base_k(cfg), epi, dtype)


@pytest.mark.parametrize("M,N,K", C20_SHAPES)
def test_conv_c_stream_config(M, N, K):
    conform(20, M, N, K, "bias_resid_relu")


REFUSED = ([(c, e, *base_shape(c), base_k(c)) for c in (4, 15) for e in EPIS if e not in CFG_EPIS[c]] +
           [(20, e, *C20_SHAPES[0]) for e in EPIS if e != "bias_resid_relu"] +
           [(20, "bias_resid_relu", 256, 512, 320), (20, "bias_resid_relu", 256, 384, 64)])


@pytest.mark.parametrize("cfg,epi,M,N,K", REFUSED, ids=[f"cfg{c}-{e}-{M}x{N}x{K}" for c, e, M, N, K in REFUSED])
def test_unsupported_pair_is_refused(cfg, epi, M, N, K):
    reject(cfg, M, N, K, epi)


# ------------------------------------------------------------------------- 2 / 7: K sweep x config
KS = [(c, K, e, d) for d in (BF, FP) for c, ks in K_SWEEP.items() for K in ks
      for e in ("bias", "bias_resid_f32") if e in CFG_EPIS[c]]


@pytest.mark.parametrize("cfg,K,epi,dtype", KS, ids=[f"cfg{c}-K{K}-{e}-{tid(d)}" for c, K, e, d in KS])
def test_k_sweep(cfg, K, epi, dtype):
    """fewer k-tiles than the config's LDS ring is deep, exactly as many, one more, and its documented
    minimum"""
    conform(cfg, *base_shape(cfg), K, epi, dtype)


@pytest.mark.parametrize("cfg,K", [(8, 64), (4, 128), (15, 576)])
@pytest.mark.parametrize("dtype", [BF, FP], ids=tid)
def test_k_below_minimum_is_refused(cfg, K, dtype):
    reject(cfg, *base_shape(cfg), K, "bias", dtype)


# ------------------------------------------------------------------------- 3: tile layouts x config
def grids(cfg):
    """tile grids (1,1), (1,3), (3,1), (5,2): 1, 3, 3 and 10 tiles, the XCD-remainder branch of the block-id
    remap and both strip orientations; M % 128 == 0 doubles the row count of the 64-row tiles (2, 6, 6, 20)"""
    bm, bn = TILE[cfg]
    f = 128 // min(bm, 128)
    return [(f * gm * bm, gn * bn) for gm, gn in ((1, 1), (1, 3), (3, 1), (5, 2))]


LAYOUTS = [(c, M, N) for c in TILE for M, N in grids(c)]


@pytest.mark.parametrize("cfg,M,N", LAYOUTS, ids=[f"cfg{c}-{M}x{N}" for c, M, N in LAYOUTS])
def test_tile_layouts(cfg, M, N):
    conform(cfg, M, N, base_k(cfg), "bias")


# ------------------------------------------------------------------------- 4: exact indexing
EXACT = [(c, e, d) for c in TILE for e, d in (("bias", BF), ("bias", FP), ("bias_f32", BF)) if e in CFG_EPIS[c]]


@pytest.mark.parametrize("cfg,epi,dtype", EXACT, ids=[f"cfg{c}-{e}-{tid(d)}" for c, e, d in EXACT])
def test_exact_indexing(cfg, epi, dtype):
    """one-hot A rows pick one W column per output row: out[m, n] == W[n, (7 m + 3) % K] exactly -- a
    swapped tile index, a transposed store or a wrong k-column shows as a wrong integer"""
    M, N = base_shape(cfg)
    K = base_k(cfg)
    r = launch(cfg, M, N, K, epi, dtype, kind="onehot")
    check_guards(r)
    w = operands(M, N, K, dtype, "onehot")[1].float()
    want = w[:, (7 * torch.arange(M) + 3) % K].T
    assert torch.equal(block(r).float(), want)


# ------------------------------------------------------------------------- 5: output and aux strides
STRIDE_CFGS = (3, 5, 7, 8, 21)


@pytest.mark.parametrize("epi", PLAIN16)
@pytest.mark.parametrize("cfg", STRIDE_CFGS)
def test_out_rows_8_byte_aligned(cfg, epi):
    """ldo % 8 == 4: the plain 16-bit epilogues leave the 16-B permlane-swapped stores for the 8-B store4
    path; same values, so the block is bit-identical to the ldo % 8 == 0 result of the same config"""
    M, N = base_shape(cfg)
    r4 = conform(cfg, M, N, base_k(cfg), epi, pado=4)
    r8 = launch(cfg, M, N, base_k(cfg), epi, pado=8)
    assert torch.equal(_bits(block(r4)), _bits(block(r8)))


@pytest.mark.parametrize("padaux", [4, 8])
@pytest.mark.parametrize("epi", AUX_EPIS)
@pytest.mark.parametrize("cfg", STRIDE_CFGS)
def test_aux_row_strides(cfg, epi, padaux):
    conform(cfg, *base_shape(cfg), base_k(cfg), epi, padaux=padaux)


@pytest.mark.parametrize("cfg", [4, 15])
@pytest.mark.parametrize("epi", PLAIN16)
def test_persistent_configs_need_16_byte_out_rows(cfg, epi):
    M, N = base_shape(cfg)
    reject(cfg, M, N, base_k(cfg), epi, pado=4)
    r = launch(-1, M, N, base_k(cfg), epi, pado=4)  # the dispatcher falls back
    check_guards(r)
    check_reference(r)


def test_persistent_save_needs_16_byte_aux_rows():
    M, N = base_shape(4)
    reject(4, M, N, 320, "bias_gelu_tanh_save", padaux=4)
    r = launch(-1, M, N, 320, "bias_gelu_tanh_save", padaux=4)
    check_guards(r)
    check_reference(r)


@pytest.mark.parametrize("M,N,K", C20_SHAPES)
def test_conv_c_stream_needs_16_byte_aux_rows(M, N, K):
    reject(20, M, N, K, "bias_resid_relu", padaux=4)
    r = launch(-1, M, N, K, "bias_resid_relu", padaux=4)
    check_guards(r)
    check_reference(r)


# ------------------------------------------------------------------------- 6: embed_f32
@pytest.mark.parametrize("cfg", [3, 5, 7, 8, 21, -1])
def test_embed_every_row(cfg):
    """every destination row (m // 100) * 101 + 1 + m % 100 holds ref[m] + pos[m % 100]; rows 0, 101, 202, ...
    and everything past the last destination keep their sentinel (check_guards)"""
    M = 512 if TILE.get(cfg, (128, 128))[0] == 256 else 256
    conform(cfg, M, 256, 128, "embed_f32")


# ------------------------------------------------------------------------- 8: gemm_wrap
@pytest.mark.parametrize("dtype", [BF, FP], ids=tid)
@pytest.mark.parametrize("epi", F16_EPIS)
@pytest.mark.parametrize("ka,K", [(64, 128), (128, 128), (128, 192), (128, 256), (192, 320)])
def test_gemm_wrap(ka, K, epi, dtype):
    """A's columns wrap at ka: A @ W[:, :ka].T + A[:, :K - ka] @ W[:, ka:].T, on the ping-pong kernel"""
    r = launch(8, 256, 256, K, epi, dtype, ka=ka, pado=8)
    check_guards(r)
    check_reference(r)


# ------------------------------------------------------------------------- 9: several tiles per workgroup
BIG_M, BIG_N = 8448, 2304  # 33 x 9 = 297 tiles of 256 x 256: more than the CUs, not a multiple of 8


def test_persistent_multi_round_cfg4_min_k():
    """cfg 4 carries its LDS ring across the tiles of a workgroup, at its smallest K, on padded rows"""
    conform(4, BIG_M, BIG_N, 192, "bias")


def test_persistent_multi_round_cfg15_min_k():
    """cfg 15 stores a tile's output during the next tile's main loop: at its smallest K, on padded rows,
    against the reference, cfg 5 and cfg 4"""
    r15 = conform(15, BIG_M, BIG_N, 640, "bias")
    r4 = launch(4, BIG_M, BIG_N, 640, "bias")
    check_guards(r4)
    assert torch.equal(_bits(r15.out), _bits(r4.out)), "cfg 15 differs from cfg 4"


def test_dispatch_multi_round():
    for K in (640, 192):
        r = launch(-1, BIG_M, BIG_N, K, "bias")
        check_guards(r)
        check_reference(r)


# ------------------------------------------------------------------------- 10: the dispatcher
def _dispatch_shapes():
    shapes = []
    for c in TILE:
        shapes.append((*base_shape(c), base_k(c)))
        shapes += [(M, N, base_k(c)) for M, N in grids(c)]
        shapes += [(*base_shape(c), K) for K in K_SWEEP[c]]
    shapes += list(C20_SHAPES) + [(512, 256, 128), (256, 256, 128)]
    return sorted(set(shapes))


DISPATCH = [(M, N, K, e, d) for M, N, K in _dispatch_shapes() for d in (BF, FP) for e in (EPIS if d == BF else F16_EPIS)]


@pytest.mark.parametrize("M,N,K,epi,dtype", DISPATCH, ids=[f"{M}x{N}x{K}-{e}-{tid(d)}" for M, N, K, e, d in DISPATCH])
def test_dispatch(M, N, K, epi, dtype):
    """cfg = -1 at every shape of the matrix, every epilogue: succeeds and matches the reference"""
    r = launch(-1, M, N, K, epi, dtype)
    check_guards(r)
    check_reference(r)


@pytest.mark.parametrize("epi", PLAIN16 + AUX_EPIS)
def test_dispatch_8_byte_rows(epi):
    M, N, K = 512, 768, 320
    r = launch(-1, M, N, K, epi, pado=4, padaux=4)
    check_guards(r)
    check_reference(r)
