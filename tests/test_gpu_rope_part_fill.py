"""rope_kv_write_part at full waves (rope_kv_write_part_kernel: 256-thread
blocks, one lane per pair of 16 B groups of a (b, t) row) against the
separate kernels it replaces, bit for bit: gemm_skinny_combine on the slabs,
then rope_kv_write_.

Shapes: 12 heads per row (Hq 6, Hkv 3). At D = 128 a row is 192 lanes of
work, one partial block with an idle wave; at D = 64 it is 96, a block whose
second wave is half idle: a lane past the row's end that still stored would
hit the next row or the sentinel pages. ksplit 2 and 8 run the unrolled
slab loads (8: every piece distinct, 2: six of eight clamped to the last
slab), ksplit 9 the loop behind them. Start positions differ per row and put
a T = 2 step across a page boundary (slots 15 and 16).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bloombee_amd import ops

    assert ops.HAVE_HIP_OPS, (
        "HIP extension must be built and loadable on a GPU box (fail-loud policy)"
    )

DEV = "cuda:0"
BF = torch.bfloat16
SENTINEL = 12352.0     # exact in bf16, far outside the data
MAXPOS = 64
B, HQ, HKV, P, MAXP = 3, 6, 3, 16, 3


def _randn_bf(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(BF)


@pytest.mark.parametrize("ks", [2, 8, 9])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [1, 2])
def test_rope_part_fill(T, D, ks):
    K = 256 * ks if ks > 2 else 512
    X = HQ + 2 * HKV
    N, M = X * D, B * T
    gen = torch.Generator().manual_seed(T * 1000 + D + ks)
    x = _randn_bf(gen, M, K).to(DEV)
    w = _randn_bf(gen, N, K, scale=K ** -0.5).to(DEV)
    bias_t = _randn_bf(gen, N).to(DEV)
    cos, sin = ops.rope_cos_sin(D, MAXPOS)
    cos, sin = cos.to(DEV), sin.to(DEV)
    npages = B * MAXP + 2
    perm = torch.randperm(npages, generator=gen)[: B * MAXP]
    pt = perm.view(B, MAXP).int().to(DEV)
    pos_t = torch.randint(0, MAXPOS, (B, T), generator=gen).int().to(DEV)

    part = ops.hip_ops.gemm_skinny(x, w, None, None, ks, None, 0.0, None, None,
                                   0, True, None)
    assert part.dtype == torch.float32 and tuple(part.shape) == (ks, M, N)
    for bias in (None, bias_t):
        unfused = ops.hip_ops.gemm_skinny(x, w, None, bias, ks).view(B, T, N)
        for starts in ((15, 14, 16), (0, 31, 15)):
            start = torch.tensor(starts, dtype=torch.int32, device=DEV)
            for pos in (None, pos_t):
                what = f"bias={bias is not None} start={starts} pos={pos is not None}"
                kp0 = torch.full((npages, HKV, P, D), SENTINEL, dtype=BF, device=DEV)
                vp0 = torch.full((npages, HKV, D, P), SENTINEL, dtype=BF, device=DEV)
                kp1, vp1 = kp0.clone(), vp0.clone()
                q0 = unfused.clone()
                ops.rope_kv_write_(q0, HQ, HKV, cos, sin, pos, kp0, vp0, pt, start)
                q1, ctx = ops.rope_kv_write_part(part, bias, B, T, HQ, HKV, cos,
                                                 sin, pos, kp1, vp1, pt, start)
                assert ctx.dtype == torch.int32 and torch.equal(ctx, start + T), what
                assert tuple(q1.shape) == (B, T, N) and q1.dtype == BF
                assert torch.equal(q1[..., : HQ * D], q0[..., : HQ * D]), "q " + what
                assert torch.equal(kp1, kp0), "k_pages " + what
                assert torch.equal(vp1, vp0), "v_pages " + what
                # exactly the B*T written slots lost the sentinel
                written = torch.zeros(npages, P, dtype=torch.bool)
                for b in range(B):
                    for t in range(T):
                        a = starts[b] + t
                        written[int(perm[b * MAXP + a // P]), a % P] = True
                assert int(written.sum()) == B * T
                wk = written.to(DEV)[:, None, :, None].expand_as(kp1)
                assert bool((kp1[~wk] == SENTINEL).all()), "k_pages outside " + what
                assert bool((kp1[wk] != SENTINEL).all())
