"""The tiled 4-bit-weight GEMM (w4_gemm_tiled.hip, gemm_w4 at M > 32) against
the fp64 CPU expectation of tests/gemm_cases.py: exact data bit for bit, randn
data within the derived bound, linear_w4 on both sides of each of its gates.

Block tile BM x 128, BM = 64 for M in 33..64, 129..192, 257..320, else 128;
128-k stages; three rotating weight register sets. Which exact case sits where:
  one-row tail in a 16-row m-tile          m33, m65, m97, m129, m193, m257
  one-row last block tile, BM 64           m129 (64+64+1), m257 (4*64+1)
  shortest second block tile at BM 128     m193 (65 rows: 4 m-tiles + 1 row)
  full tiles                               m64 (BM 64), m128 (BM 128)
  lone half-width column tile              n64 (waves 2, 3 past N)
  N % 128 != 0 and the XCD remap, r != 0   m129-n704 (18 blocks), m257-n320 (15)
  stages per split 1 / 2 / 3 / 4 / 5 / 6   k128, k256, k384, k1024-ks2, k640,
                                           k2048-ks3 (6, 6, 4)
  uneven splits                            k2048-ks3, k384-ks2, k1152-ks0 (5 + 4)
  over-asked split                         m193-k256-ks5 (two splits run)
  bias / residual in the epilogue          ks1 and the unsplit ks0 cases
  bias / residual in the combine           ks2..ks5, k1152-ks0
Worst |err| / bound of the realistic cases: profiles/r10_w4_tiled.md.
"""
import pytest
import torch

import gemm_cases as gc
from test_gpu_gemm_exact import DEV, assert_exact, assert_one_rounding, dev

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bloombee_amd import ops
    from bloombee_amd.ops import interface as iface
    from bloombee_amd.ops import reference as ref

    assert ops.HAVE_HIP_OPS, "HIP extension must be built and loadable on a GPU box"

BF = torch.bfloat16


def run(c, rows=None, via_linear=False):
    """gemm_w4 / linear_w4 on the first `rows` (default M) rows of the case,
    A as the bf16 view of the taller poisoned buffer."""
    spec = c.spec
    N, K = spec.N, spec.K
    m = spec.M if rows is None else rows
    a = dev(c.Abuf)[:m]
    res = None if c.res is None else dev(c.res)[:m]
    bias, packed = dev(c.bias), c.packed.to(DEV)
    scale, zero = dev(c.scale, torch.float16), dev(c.zero, torch.float16)
    if via_linear:
        return ops.linear_w4(a, packed.reshape(N, K // 64, 32), scale, zero, N,
                             residual=res, bias=bias)
    return ops.hip_ops.gemm_w4(a, packed, scale, zero, res, bias, N, spec.ksplit)


def _t(M, N, K, ks, bias, res, seed):
    return gc.Spec(f"w4t-m{M}-n{N}-k{K}-ks{ks}", "w4", M, N, K, ks, bias=bias,
                   res=res, seed=seed)


CASES = [
    _t(33, 64, 128, 1, True, True, 201),
    _t(48, 576, 384, 0, False, True, 202),
    _t(64, 704, 1024, 2, True, True, 203),
    _t(65, 192, 2048, 3, True, False, 204),
    _t(97, 576, 640, 0, True, True, 205),
    _t(128, 128, 256, 1, False, False, 206),
    _t(129, 704, 384, 2, True, True, 207),
    _t(200, 64, 1152, 0, False, True, 208),
    _t(257, 320, 512, 4, True, True, 209),
    _t(193, 192, 256, 5, True, True, 210),
]


@pytest.mark.parametrize("spec", CASES, ids=gc.ids(CASES))
def test_gemm_w4_tiled_exact(spec):
    c = gc.build(spec)
    BM, ksplit, kchunk = ops.hip_ops.gemm_w4_tiled_plan(spec.M, spec.N, spec.K,
                                                        spec.ksplit)
    assert BM == (64 if (spec.M - 1) % 128 < 64 else 128)
    assert kchunk % 128 == 0 and (ksplit - 1) * kchunk < spec.K <= ksplit * kchunk
    got = run(c, via_linear=(spec.ksplit == 0))
    assert tuple(got.shape) == (spec.M, spec.N) and got.dtype == BF
    assert_exact(got, c.want, spec.name)


@pytest.mark.parametrize("M,N,K,ks", [(72, 576, 1024, 1), (130, 704, 1280, 3)],
                         ids=["unsplit", "split"])
def test_gemm_w4_tiled_realistic(M, N, K, ks):
    """randn inputs against fp64, bound as for test_gemm_w4_realistic: the
    bf16 -> f16 conversion of randn-scale A is exact, so no further term."""
    gen = torch.Generator().manual_seed(105)
    a = torch.randn(M, K, generator=gen).to(BF)
    packed, scale, zero = ref.quant4_pack(torch.randn(N, K, generator=gen) * K ** -0.5)
    q = torch.stack([(packed & 0xF).double(), (packed >> 4).double()], dim=-1)
    wd = (q.reshape(N, K // 64, 64) * scale.double()[..., None]
          + zero.double()[..., None]).reshape(N, K)        # exact in fp64
    r = torch.randn(M, N, generator=gen).to(BF)
    want = a.double() @ wd.T + r.double()
    absprod = a.double().abs() @ wd.abs().T
    bound = gc.realistic_bound(want, K, absprod, extra=2.0 ** -10 * absprod)
    got = ops.hip_ops.gemm_w4(a.to(DEV), packed.reshape(N, K // 2).to(DEV),
                              scale.to(DEV), zero.to(DEV), r.to(DEV), None, N, ks)
    ratio = float(((got.cpu().double() - want).abs() / bound).max())
    print(f"worst |err| / bound, gemm_w4 tiled {M}x{N}x{K} ks={ks}: {ratio:.3f}")
    assert ratio <= 1.0


def test_linear_w4_tiled_gates(monkeypatch):
    """The same exact data on each side of each gate in linear_w4."""
    c = gc.build(_t(33, 576, 256, 0, True, True, 211))
    assert_exact(run(c, 32, via_linear=True), c.want[:32], "M=32 (skinny kernel)")
    assert_exact(run(c, via_linear=True), c.want, "M=33 (tiled kernel)")
    monkeypatch.setenv("BBAMD_W4_TILED", "0")
    assert_one_rounding(run(c, via_linear=True), c.want,
                        "M=33, BBAMD_W4_TILED=0 (dequant + library)")
    monkeypatch.delenv("BBAMD_W4_TILED")
    # one row past the bound: the case's rows, repeated
    m = iface._W4_TILED_MAX_M + 1
    rows = torch.arange(m) % 33
    N, K = 576, 256
    got = ops.linear_w4(dev(c.Abuf[rows]), c.packed.to(DEV).reshape(N, K // 64, 32),
                        dev(c.scale, torch.float16), dev(c.zero, torch.float16), N,
                        residual=dev(c.res[rows]), bias=dev(c.bias))
    assert_one_rounding(got, c.want[rows], f"M={m} (dequant + library)")


def test_llama_quantized_prefill_gpu():
    """test_llama_quantized_engine_decode_gpu with a 40-token prefill (B = 2,
    T = 20): every projection of the quantized block runs the tiled kernel
    and tracks the CPU dequant matmul on the SAME codes."""
    from bloombee_amd.engine import BlockStack
    from bloombee_amd.models.base import resolve_config

    cfg = resolve_config("llama-mini-gpu")
    cpu = BlockStack(cfg, 0, 2, device="cpu", seed=5)
    gpu = BlockStack(cfg, 0, 2, device=DEV, seed=5)
    for bc, bg in zip(cpu.blocks, gpu.blocks):
        bc.quantize_weights_q4()
        bg._w4 = {name: tuple(t.to(DEV) if torch.is_tensor(t) else t
                              for t in entry)
                  for name, entry in bc._w4.items()}
    kvc, kvg = cpu.make_kv(1 << 10), gpu.make_kv(1 << 10)
    hc, hg = kvc.allocate(2, 32), kvg.allocate(2, 32)
    gen = torch.Generator().manual_seed(1)
    x = (torch.randn(2, 20, cfg.hidden_size, generator=gen) * 0.1).to(cfg.dtype)
    sp = torch.zeros(2, dtype=torch.int32)
    hc.extend(20)
    hg.extend(20)
    yc = cpu.forward_inference(x.clone(), hc, sp)
    yg = gpu.forward_inference(x.to(DEV), hg, sp.to(DEV))
    assert torch.allclose(yg.cpu().float(), yc.float(), atol=3e-2), \
        (yg.cpu().float() - yc.float()).abs().max()
