"""The fp8 (e4m3) weight tier above 32 rows: hip_w8.gemm_w8_tiled
(ops/hip/gemm_w8_tiled.hip), hip_w8.quant_rows_fp8 without its row cap and
ops.linear_w8 / a Llama block over them.

Exact cases: x and w are integers in -7..7 with a +-7 forced into every row,
so every scale is 2^-6, every code 64 * the integer (exact in e4m3) and every
partial sum an integer multiple of 2^-12 below 2^24 * 2^-12: any summation
order gives the same f32 and the result must equal the fp64 one rounded once
to bf16. M on both sides of the 64- and 128-row tile boundaries and of the BM
choice; (N, K): a lone half column tile with a single k-step, a full column
tile plus a half one with an odd step count, 8 steps (two turns of the W
ring), 19 steps (a ring tail); unsplit and split through the plan.

Random cases: |y - ref| <= 2^-8 |ref| + K 2^-24 S with S = a_scale w_scale
sum_k |a8 codes|: one bf16 rounding plus the f32 summation bound.

Block: atol 3e-2, the tier's GPU-vs-CPU block tolerance
(tests/test_gpu_gemm_w8.py)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bloombee_amd import ops
    from bloombee_amd.ops import reference as ref

    assert ops.HAVE_HIP_OPS, "HIP extension must be built and loadable on a GPU box"

DEV = "cuda:0"
BF = torch.bfloat16
ROWS = 200
MS = (33, 64, 65, 128, 129, 200)
NKS = ((64, 128), (192, 384), (320, 1024), (128, 2432))
# (M, N, K, split); one k-step cannot be split
GRID = [(M, N, K, sp) for M in MS for N, K in NKS for sp in (False, True)
        if not (sp and K == 128)]


@functools.lru_cache(maxsize=None)
def case(N, K, exact):
    """ROWS rows of x, the weight as tiled codes on the device, bias and
    residual, and what the definition gives in fp64 (before bias/residual)
    with its summation bound. exact: the integer data of the docstring."""
    gen = torch.Generator().manual_seed(N * 7 + K)
    if exact:
        x = torch.randint(-7, 8, (ROWS, K), generator=gen).float()
        w = torch.randint(-7, 8, (N, K), generator=gen).float()
        x[:, 3], w[:, 5] = 7.0, -7.0
        bias = torch.randint(-8, 9, (N,), generator=gen).to(BF)
        res = torch.randint(-8, 9, (ROWS, N), generator=gen).to(BF)
    else:
        x = torch.randn(ROWS, K, generator=gen) * 0.7
        w = torch.randn(N, K, generator=gen) * 0.05
        bias, res = torch.randn(N, generator=gen).to(BF), torch.randn(ROWS, N, generator=gen).to(BF)
    x, w = x.to(BF), w.to(BF)
    codes, w_scale = ref.quant_w8(w)
    a8, a_scale = ref.quant_rows_fp8(x)
    sc = a_scale.double().unsqueeze(1) * w_scale.double().unsqueeze(0)
    want = sc * (a8.double() @ codes.double().t())
    S = sc * (a8.double().abs() @ codes.double().abs().t())
    if exact:
        assert torch.all(a_scale == 2.0 ** -6) and torch.all(w_scale == 2.0 ** -6)
        assert torch.equal(want, x.double() @ w.double().t())
    return dict(x=x.to(DEV), a8=a8.to(DEV), a_scale=a_scale.to(DEV),
                packed=ref.pack_w8(codes).to(DEV), w_scale=w_scale.to(DEV),
                bias=bias.to(DEV), res=res.to(DEV), want=want, S=S)


def run_gemm(c, M, N, K, split, epi):
    bm, mtiles, ksplit, kchunk = ops.hip_w8.gemm_w8_tiled_plan(M, N, K, 2 if split else 1)
    assert ksplit == (2 if split else 1) and ksplit * kchunk >= K > (ksplit - 1) * kchunk
    assert bm in (64, 128) and mtiles * bm >= M > (mtiles - 1) * bm
    got = ops.hip_w8.gemm_w8_tiled(c["a8"][:M], c["a_scale"][:M], c["packed"], c["w_scale"],
                                   c["res"][:M] if epi else None, c["bias"] if epi else None,
                                   N, ksplit)
    want = c["want"][:M]
    if epi:
        want = want + c["bias"].cpu().double() + c["res"][:M].cpu().double()
    return got.cpu(), want


@pytest.mark.parametrize("epi", (False, True), ids=("plain", "bias+res"))
@pytest.mark.parametrize("M,N,K,split", GRID)
def test_gemm_w8_tiled_exact(M, N, K, split, epi):
    got, want = run_gemm(case(N, K, True), M, N, K, split, epi)
    assert got.dtype == BF and torch.equal(got, want.to(BF))


@pytest.mark.parametrize("M,N,K,split", GRID)
def test_gemm_w8_tiled_random(M, N, K, split):
    c = case(N, K, False)
    got, want = run_gemm(c, M, N, K, split, False)
    bound = 2.0 ** -8 * want.abs() + K * 2.0 ** -24 * c["S"][:M]
    ratio = ((got.double() - want).abs() / bound).max().item()
    print(f"worst |err| / bound, gemm_w8_tiled {M}x{N}x{K} split={split}: {ratio:.3f}")
    assert ratio <= 1.0


def test_quant_rows_fp8_bits_above_32_rows():
    x = torch.randn(ROWS, 384, generator=torch.Generator().manual_seed(3))
    x[2] = 0
    x[150, 100] = 3e4
    x[199] *= 2.0 ** -24
    x = x.to(BF)
    a8, a_scale = ops.hip_w8.quant_rows_fp8(x.to(DEV))
    want8, want_scale = ref.quant_rows_fp8(x)
    assert torch.equal(a_scale.cpu(), want_scale)
    assert torch.equal(a8.cpu().view(torch.uint8), want8.view(torch.uint8))


@pytest.mark.parametrize("tiled", ("1", "0"), ids=("kernel", "switched-off"))
def test_linear_w8_above_32_rows(tiled, monkeypatch):
    """The public entry at M = 200 on the exact data (the torch composition
    sums the same integers), with the tiled kernel on and off."""
    monkeypatch.setenv("BBAMD_W8_TILED", tiled)
    N, K = 192, 384
    c = case(N, K, True)
    got = ops.linear_w8(c["x"], c["packed"], c["w_scale"], N,
                        residual=c["res"], bias=c["bias"])
    want = c["want"] + c["bias"].cpu().double() + c["res"].cpu().double()
    assert torch.equal(got.cpu(), want.to(BF))


def test_llama_block_fp8_prefill_gpu_vs_cpu():
    from bloombee_amd.engine import BlockStack
    from bloombee_amd.models.base import resolve_config

    cfg = resolve_config("llama-tiny")
    cpu = BlockStack(cfg, 0, 1, device="cpu", seed=5)
    gpu = BlockStack(cfg, 0, 1, device=DEV, seed=5)
    cpu.blocks[0].quantize_weights_fp8()
    gpu.blocks[0]._w8 = {n: (p.to(DEV), s.to(DEV), N)
                         for n, (p, s, N) in cpu.blocks[0]._w8.items()}
    hc, hg = cpu.make_kv(1 << 10).allocate(3, 32), gpu.make_kv(1 << 10).allocate(3, 32)
    gen = torch.Generator().manual_seed(1)
    for step, T in enumerate((16, 1)):      # 48-row prefill, one decode step
        x = (torch.randn(3, T, cfg.hidden_size, generator=gen) * 0.1).to(cfg.dtype)
        sp = torch.full((3,), (0, 16)[step], dtype=torch.int32)
        hc.extend(T)
        hg.extend(T)
        yc = cpu.forward_inference(x.clone(), hc, sp)
        yg = gpu.forward_inference(x.to(DEV), hg, sp.to(DEV))
        assert torch.allclose(yg.cpu().float(), yc.float(), atol=3e-2), \
            (step, (yg.cpu().float() - yc.float()).abs().max())
