"""Exact-arithmetic cases for the W ring of gemm_skinny_v2 (helper module of
test_gemm_wring_cases_cpu.py and test_gpu_gemm_wring.py; built with
gemm_cases.build, so its fp64 model and its invariants apply).

The ring kernel runs whole periods of DEPTH sets (DEPTH/2 stages of 256 k)
in its loop and peels the last one or two periods by the number of sets left,
so what decides the path is the number of 256-k stages a split holds. The
cases give a split 1, 2, 3, 4, 5, 7 and 9 stages (K = 256 n, ksplit 1) and
uneven splits (K = 768 over 2: 2 + 1 stages; K = 1792 over 2: 4 + 3): every
remainder of a period of 2, 3 or 4 stages, with streams shorter than the ring
(1 stage), exactly one period, and a loop that runs more than once (9).
M in {1, 17, 32}: one M-tile, a second tile with one live row, two full tiles.
N = 576 is 9 workgroups: the XCD remap with a remainder.
"""
import gemm_cases as gc

DEPTHS = (2, 4)        # what the build instantiates (gemm_skinny_wring_plan)


def _d(name, M, N, K, ks, **kw):
    return gc.Spec(name, "dense", M, N, K, ks, **kw)


def _n(name, M, N, K, ks, **kw):
    return gc.Spec(name, "norm", M, N, K, ks, mode=2, **kw)


SPECS = [
    _d("wr-m1-n64-k256-st1", 1, 64, 256, 1, bias=True, res=True, seed=201),
    _d("wr-m17-n576-k512-st2-ssout", 17, 576, 512, 1, res=True, ss_out=True, seed=202),
    _n("wr-m32-n64-k768-st3-mode2-ssin9", 32, 64, 768, 1, res=True, ss_in=9, seed=203),
    _d("wr-m32-n576-k1024-st4", 32, 576, 1024, 1, bias=True, seed=204),
    _d("wr-m17-n64-k1280-st5-ssout", 17, 64, 1280, 1, bias=True, res=True,
       ss_out=True, seed=205),
    _n("wr-m17-n576-k1792-st7-mode2-ssin36", 17, 576, 1792, 1, bias=True,
       ss_in=36, seed=206),
    _d("wr-m1-n576-k2304-st9", 1, 576, 2304, 1, bias=True, res=True, seed=207),
    _d("wr-m32-n64-k2304-st9-ssout", 32, 64, 2304, 1, res=True, ss_out=True, seed=208),
    _d("wr-m32-n576-k768-ks2-st2+1", 32, 576, 768, 2, bias=True, res=True, seed=209),
    _d("wr-m17-n64-k768-ks2-st2+1-ssout", 17, 64, 768, 2, res=True, ss_out=True,
       seed=210),
    _n("wr-m32-n576-k1280-ks2-st3+2-mode2", 32, 576, 1280, 2, res=True, seed=211),
    _n("wr-m1-n64-k1792-ks2-st4+3-mode2-ssin8", 1, 64, 1792, 2, bias=True, ss_in=8,
       seed=212),
]

# split-K with the slabs handed back uncombined (defer_combine): no bias, no
# residual; slab s must hold exactly A[:, k0:k1] @ W[:, k0:k1]^T
DEFER_SPECS = [
    _d("wr-m32-n576-k1792-ks2-st4+3-defer", 32, 576, 1792, 2, seed=221),
    _d("wr-m17-n64-k768-ks2-st2+1-defer", 17, 64, 768, 2, seed=222),
    _d("wr-m1-n576-k2304-ks3-st3-defer", 1, 576, 2304, 3, seed=223),
]

ALL_SPECS = SPECS + DEFER_SPECS


def stages(spec):
    """256-k stages per launched split."""
    return [(b - a) // 256 for a, b in gc.splits_of(spec)]


def slab_model(c):
    """fp64 (ksplit, M, N): what each split contributes, before any norm."""
    spec = c.spec
    A = c.Abuf[: spec.M]
    return [A[:, a:b] @ c.W[:, a:b].T for a, b in gc.splits_of(spec)]
