"""Host-side contract of the HIP extension's bindings, checked without a
GPU: the exported split-K plans against the independent mirrors the exact
GEMM tests carry, fuse_swiglu_ok against recorded values, and the rejection
of CPU tensors by every binding. Skipped when the extension is not built."""
import itertools

import pytest
import torch

import binding_cases as bc
import gemm_cases as gc
import moe_w4_cases as mc
from bloombee_amd import ops
from bloombee_amd.ops import interface as iface

pytestmark = pytest.mark.skipif(not ops.HAVE_HIP_OPS,
                                reason="HIP extension not built")

# K: the v1 kernel (96, 160), one / two / three v2 chunks, llama's 14336.
# N/64: 1, either side of the big-N rule (255, 256), and the spec shapes.
_KS = (96, 128, 160, 256, 384, 512, 768, 1024, 1280, 2048, 4096, 14336)
_NS = (64, 128, 576, 704, 960, 64 * 255, 64 * 256, 28672)
_REQ = (0, 1, 2, 3, 5, 8, 57, 1000)   # 57, 1000: more than the chunk count


def _skinny_grid():
    grid = set(itertools.product(_NS, _KS, _REQ))
    for s in gc.ALL_CASES:
        if s.kind in ("dense", "norm"):
            grid.add((s.N, s.K, s.ksplit))
    return sorted(g for g in grid if g[1] % 32 == 0)


def _w4_grid():
    ks = [k for k in _KS if k % 128 == 0]
    grid = set(itertools.product((1, 2, 16, 17, 32), _NS, ks, _REQ))
    for s in gc.ALL_CASES:
        if s.kind == "w4":
            grid.add((s.M, s.N, s.K, s.ksplit))
    return sorted(grid)


def test_gemm_skinny_plan_matches_mirror():
    for N, K, req in _skinny_grid():
        ksplit, kchunk, v2 = ops.hip_ops.gemm_skinny_plan(N, K, req)
        assert v2 == gc.skinny_is_v2(K)
        want = gc.skinny_splits(N, K, req)
        got = [(s * kchunk, max(s * kchunk, min(K, (s + 1) * kchunk)))
               for s in range(ksplit)]
        assert got == want, (N, K, req)


def test_gemm_w4_plan_matches_mirror():
    for M, N, K, req in _w4_grid():
        gemv, ksplit, kchunk = ops.hip_ops.gemm_w4_plan(M, N, K, req)
        assert gemv == gc.w4_is_gemv(M, K), (M, N, K, req)
        got = [(s * kchunk, min(K, (s + 1) * kchunk)) for s in range(ksplit)]
        assert got == gc.w4_splits(M, N, K, req), (M, N, K, req)


def test_moe_gemm_w4_plan_matches_mirror():
    specs = list(mc.CASES)
    ks = [k for k in _KS if k % 128 == 0]
    for counts in ((1,), (0, 2), (3, 0, 0, 5), (1,) * 8, (0,) * 8 + (40,)):
        for N, K, req in itertools.product(_NS, ks, _REQ):
            specs.append(mc.Spec("grid", N, K, counts, ksplit=req))
    for s in specs:
        E, S = len(s.counts), sum(s.counts)
        ksplit, kchunk = ops.hip_ops.moe_gemm_w4_plan(E, s.N, s.K, S, s.ksplit)
        got = [(i * kchunk, min(s.K, (i + 1) * kchunk)) for i in range(ksplit)]
        assert got == mc.splits_of(s), s


# (H, I) of the gate_up projection -> what fuse_swiglu_ok returned before the
# split-K rule moved into the extension (recorded from that Python rule, with
# BBAMD_GEMM_KSPLIT_BIG unset). The narrow shapes are the ones the rule exists
# for: their plain gate_up GEMM splits K.
_SWIGLU = [
    ("llama-3-8b", 4096, 14336, True),
    ("llama-3-70b", 8192, 28672, True),
    ("gemma-2-2b", 2304, 9216, True),
    ("narrow-k1024", 1024, 2048, False),
    ("narrow-k256", 256, 512, True),
]


@pytest.mark.parametrize("name,H,I,want", _SWIGLU, ids=[s[0] for s in _SWIGLU])
def test_fuse_swiglu_ok_unchanged(monkeypatch, name, H, I, want):
    # the rule reads shapes only: meta tensors, and the device test patched
    monkeypatch.setattr(iface, "_on_gpu", lambda t: True)
    monkeypatch.setattr(iface, "_FUSE_NORM", True)
    monkeypatch.setattr(iface, "_FUSE_SWIGLU", True)
    x = torch.empty(1, 1, H, dtype=torch.bfloat16, device="meta")
    w = torch.empty(2 * I, H, dtype=torch.bfloat16, device="meta")
    assert iface.fuse_norm_linear_ok(x, w)
    assert iface.fuse_swiglu_ok(x, w) is want


@pytest.mark.parametrize("op", bc.OPS)
def test_all_cpu_tensors_rejected(op):
    call = bc.build("cpu")[op]
    with pytest.raises(RuntimeError, match="must be on device"):
        getattr(ops.hip_ops, op)(*call.args)


def test_every_binding_has_a_case():
    names = {n for n in dir(ops.hip_ops) if not n.startswith("_")}
    names -= {n for n in names if n.startswith("wire_") or n.endswith("_plan")}
    assert names == set(bc.OPS)
