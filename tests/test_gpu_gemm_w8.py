"""The fp8 (e4m3) weight tier on the device: hip_w8.quant_rows_fp8 and
hip_w8.gemm_w8 (ops/hip/gemm_w8.hip) and ops.linear_w8 over them.

Exact cases: x and w are integers in -7..7 with a +-7 forced into every row,
so every scale is 2^-6, every code 64 * the integer (exact in e4m3) and every
partial sum an integer multiple of 2^-12 below 2^24 * 2^-12: any summation
order gives the same f32 and the result must equal the fp64 one rounded once
to bf16. Shapes: one stripe / several, K of 2, 3 (odd), 8 (one full ring) and
19 tiles (two A chunks and a 3-tile tail), M on both sides of the second row
tile, unsplit and split through the plan.

Random cases: |y - ref| <= 2^-8 |ref| + K 2^-24 S with S = a_scale w_scale
sum_k |a8 codes|: one bf16 rounding plus the f32 summation bound.

Block: tolerance atol 3e-2, the W4 tier's GPU-vs-CPU block tolerance
(tests/test_gpu_kernels.py, test_llama_quantized_engine_decode_gpu)."""
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
MS = (1, 5, 16, 17, 32)
NKS = ((64, 384), (192, 1024), (512, 256), (128, 2432))


@functools.lru_cache(maxsize=None)
def case(N, K, exact):
    """33 rows of x, the weight as tiled codes on the device, bias and
    residual, and what the definition gives in fp64 (before bias/residual)
    with its summation bound. exact: the integer data of the docstring."""
    gen = torch.Generator().manual_seed(N * 7 + K)
    if exact:
        x = torch.randint(-7, 8, (33, K), generator=gen).float()
        w = torch.randint(-7, 8, (N, K), generator=gen).float()
        x[:, 3], w[:, 5] = 7.0, -7.0
        bias = torch.randint(-8, 9, (N,), generator=gen).to(BF)
        res = torch.randint(-8, 9, (33, N), generator=gen).to(BF)
    else:
        x = torch.randn(33, K, generator=gen) * 0.7
        w = torch.randn(N, K, generator=gen) * 0.05
        bias, res = torch.randn(N, generator=gen).to(BF), torch.randn(33, N, generator=gen).to(BF)
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
    ksplit, kchunk = ops.hip_w8.gemm_w8_plan(N, K, 2 if split else 1)
    assert (ksplit >= 2) == split and ksplit * kchunk >= K > (ksplit - 1) * kchunk
    got = ops.hip_w8.gemm_w8(c["a8"][:M], c["a_scale"][:M], c["packed"], c["w_scale"],
                             c["res"][:M] if epi else None, c["bias"] if epi else None,
                             N, ksplit)
    want = c["want"][:M]
    if epi:
        want = want + c["bias"].cpu().double() + c["res"][:M].cpu().double()
    return got.cpu(), want


@pytest.mark.parametrize("epi", (False, True), ids=("plain", "bias+res"))
@pytest.mark.parametrize("split", (False, True), ids=("unsplit", "split"))
@pytest.mark.parametrize("N,K", NKS)
@pytest.mark.parametrize("M", MS)
def test_gemm_w8_exact(M, N, K, split, epi):
    got, want = run_gemm(case(N, K, True), M, N, K, split, epi)
    assert got.dtype == BF and torch.equal(got, want.to(BF))


@pytest.mark.parametrize("split", (False, True), ids=("unsplit", "split"))
@pytest.mark.parametrize("N,K", NKS)
@pytest.mark.parametrize("M", MS)
def test_gemm_w8_random(M, N, K, split):
    c = case(N, K, False)
    got, want = run_gemm(c, M, N, K, split, False)
    bound = 2.0 ** -8 * want.abs() + K * 2.0 ** -24 * c["S"][:M]
    ratio = ((got.double() - want).abs() / bound).max().item()
    print(f"worst |err| / bound, gemm_w8 {M}x{N}x{K} split={split}: {ratio:.3f}")
    assert ratio <= 1.0


def test_quant_rows_fp8_bits():
    x = torch.randn(9, 384, generator=torch.Generator().manual_seed(3))
    x[2] = 0
    x[4, 100] = 3e4
    x[6] *= 2.0 ** -24
    x = x.to(BF)
    a8, a_scale = ops.hip_w8.quant_rows_fp8(x.to(DEV))
    want8, want_scale = ref.quant_rows_fp8(x)
    assert torch.equal(a_scale.cpu(), want_scale)
    assert torch.equal(a8.cpu().view(torch.uint8), want8.view(torch.uint8))


@pytest.mark.parametrize("M,kernel", [(32, "1"), (33, "1"), (5, "0")],
                         ids=("kernel", "rows-above-gate", "switched-off"))
def test_linear_w8_paths(M, kernel, monkeypatch):
    """The public entry on both sides of its gates, on the exact data (the
    torch composition sums the same integers)."""
    monkeypatch.setenv("BBAMD_W8_KERNEL", kernel)
    N, K = 192, 1024
    c = case(N, K, True)
    got = ops.linear_w8(c["x"][:M], c["packed"], c["w_scale"], N,
                        residual=c["res"][:M], bias=c["bias"])
    want = c["want"][:M] + c["bias"].cpu().double() + c["res"][:M].cpu().double()
    assert torch.equal(got.cpu(), want.to(BF))


def test_llama_block_fp8_gpu_vs_cpu():
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
    for step, T in enumerate((4, 1, 1)):            # prefill, two decode steps
        x = (torch.randn(3, T, cfg.hidden_size, generator=gen) * 0.1).to(cfg.dtype)
        sp = torch.full((3,), (0, 4, 5)[step], dtype=torch.int32)
        hc.extend(T)
        hg.extend(T)
        yc = cpu.forward_inference(x.clone(), hc, sp)
        yg = gpu.forward_inference(x.to(DEV), hg, sp.to(DEV))
        assert torch.allclose(yg.cpu().float(), yc.float(), atol=3e-2), \
            (step, (yg.cpu().float() - yc.float()).abs().max())
