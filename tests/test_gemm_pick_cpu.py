"""The GEMM dispatcher on the host: vc_gemm_pick (the tile config vc_gemm_h16 runs with cfg = -1)
over the model shapes, every epilogue and both row alignments.  Nothing here launches: every
configuration it returns must satisfy what vc_gemm_h16 and launch_epi (csrc/gemm.hip) demand of an
explicitly requested one, and every production configuration must be reachable."""
import itertools

import pytest

import vclip_amd._lib as L
from vclip_amd import ops
from vclip_amd.build import build

EPI = ops.EPI
ALL = frozenset(EPI.values())
E = lambda *names: frozenset(EPI[n] for n in names)  # noqa: E731

# What csrc/gemm.hip requires of each configuration (kCfgs, launch_epi, the checks of vc_gemm_h16):
#   tile     (BM, BN) must divide M x N (cfg 20: 128 x 256 at K 64 / 128, 128 x 128 at K 256)
#   epi      the epilogues launch_epi instantiates for it
#   kmin     smallest K (cfg 20: K one of 64, 128, 256 exactly)
#   nmax     widest N (the persistent kernels keep the whole bias in LDS)
#   rows16   16-B output rows: ldo % 8 == 0
#   aux16    16-B rows of the second 16-bit operand where the epilogue has one: ldaux % 8 == 0
#            (cfg 4's saved pre-activation, cfg 20's residual)
PRECONDITIONS = {
    3: dict(tile=(256, 256), epi=ALL, kmin=64, nmax=None, rows16=False, aux16=()),
    4: dict(tile=(256, 256), epi=E("bias", "bias_gelu_tanh", "bias_gelu_erf", "bias_relu", "bias_gelu_tanh_save"),
            kmin=192, nmax=8192, rows16=True, aux16=E("bias_gelu_tanh_save")),
    5: dict(tile=(128, 128), epi=ALL, kmin=64, nmax=None, rows16=False, aux16=()),
    7: dict(tile=(64, 128), epi=ALL, kmin=64, nmax=None, rows16=False, aux16=()),
    8: dict(tile=(256, 256), epi=ALL, kmin=128, nmax=None, rows16=False, aux16=()),
    15: dict(tile=(256, 256), epi=E("bias", "bias_gelu_tanh", "bias_gelu_erf", "bias_relu"), kmin=640, nmax=8192,
             rows16=True, aux16=()),
    20: dict(tile=None, epi=E("bias_resid_relu"), kmin=64, nmax=None, rows16=True, aux16=E("bias_resid_relu")),
    21: dict(tile=(64, 128), epi=ALL, kmin=64, nmax=None, rows16=False, aux16=()),
}

MS = (128, 256, 512, 1024, 3328, 6400, 12544, 12800, 25344)
NS = (128, 256, 384, 768, 1536, 2304, 3072)
KS = (64, 128, 192, 256, 640, 768, 3072)


def violations(cfg, M, N, K, e, ldo, ldaux):
    """the preconditions of `cfg` that (M, N, K, epilogue e, ldo, ldaux) breaks"""
    if cfg not in PRECONDITIONS:
        return [f"cfg {cfg} is not a production configuration"]
    p = PRECONDITIONS[cfg]
    bad = []
    if cfg == 20:
        if K not in (64, 128, 256):
            bad.append("K not 64 / 128 / 256")
        tile = (128, 256 if K <= 128 else 128)
    else:
        tile = p["tile"]
    if M % tile[0] or N % tile[1]:
        bad.append(f"tile {tile} does not divide {M} x {N}")
    if e not in p["epi"]:
        bad.append("epilogue not instantiated")
    if K < p["kmin"] or K % 64:
        bad.append(f"K < {p['kmin']}")
    if p["nmax"] is not None and N > p["nmax"]:
        bad.append(f"N > {p['nmax']}")
    if p["rows16"] and ldo % 8:
        bad.append("ldo % 8")
    if e in p["aux16"] and ldaux % 8:
        bad.append("ldaux % 8")
    return bad


@pytest.fixture(scope="module")
def lib():
    build()
    return L.load()


def test_preconditions_table_flags_what_the_host_rejects():
    """the table itself: the requests vc_gemm_h16 refuses for an explicit cfg are violations here"""
    assert violations(8, 512, 768, 64, EPI["bias"], 768, 768)
    assert violations(4, 512, 768, 128, EPI["bias"], 768, 768)
    assert violations(15, 512, 768, 576, EPI["bias"], 768, 768)
    assert violations(4, 512, 768, 320, EPI["bias_f32"], 768, 768)
    assert violations(15, 512, 768, 704, EPI["bias_gelu_tanh_save"], 768, 768)
    assert violations(4, 512, 768, 320, EPI["bias"], 772, 768)
    assert violations(20, 256, 512, 64, EPI["bias_resid_relu"], 512, 516)
    assert violations(20, 256, 384, 128, EPI["bias_resid_relu"], 384, 384)
    assert violations(7, 512, 768, 320, EPI["bias"], 772, 772) == []
    assert violations(4, 512, 768, 192, EPI["bias_gelu_tanh_save"], 768, 768) == []


def test_pick_returns_only_runnable_configs_and_reaches_all(lib):
    seen = {}
    broken = []
    for M, N, K, (name, e) in itertools.product(MS, NS, KS, sorted(EPI.items(), key=lambda kv: kv[1])):
        for ldo, ldaux in itertools.product((N, N + 4), (N, N + 4)):
            cfg = lib.vc_gemm_pick(M, N, K, e, ldo, ldaux, None)
            seen.setdefault(cfg, (M, N, K, name, ldo, ldaux))
            bad = violations(cfg, M, N, K, e, ldo, ldaux)
            if bad:
                broken.append((M, N, K, name, ldo, ldaux, cfg, bad))
    assert not broken, f"{len(broken)} picks break their config's preconditions, first: {broken[:5]}"
    assert sorted(seen) == sorted(PRECONDITIONS), f"configs returned: {sorted(seen)}"


def test_pick_reaches_cfg3_at_k64(lib):
    """the 256x256 kernel with one workgroup per tile (cfg 3) sits behind the ping-pong rule (cfg 8,
    K >= 128): it is what a one-round 256x256 grid gets at K = 64"""
    hits = [(M, N, name) for M, N, (name, e) in itertools.product(MS, NS, EPI.items())
            if lib.vc_gemm_pick(M, N, 64, e, N, N, None) == 3]
    assert hits, "no K = 64 point of the sweep reaches cfg 3"
    for M, N, name in hits:
        assert violations(3, M, N, 64, EPI[name], N, N) == []
