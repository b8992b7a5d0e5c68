"""The writers of an fp8 (e4m3) KV pool, and a llama block on top of one. A
stored element is x.float().clamp(-448, 448).to(torch.float8_e4m3fn) of the
bf16 value a bf16 pool would hold."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bloombee_amd import ops
    from bloombee_amd.ops import reference as ref

    assert ops.HAVE_HIP_OPS, "the HIP extension must load on a GPU box"

DEV = "cuda:0"
FP8 = torch.float8_e4m3fn
P = 16
# saturation (not NaN), the subnormal range (2^-10 ties to 0, 3 * 2^-10 ties to
# 2^-8), the ties 1.0625 -> 1.0 and 1.1875 -> 1.25, signed zero
SHARP = [448., -448., 464., -464., 500., 1e4, -1e4, 2.0 ** -9, 2.0 ** -10,
         3 * 2.0 ** -10, -3 * 2.0 ** -10, 1.0625, 1.1875, -1.0625, 0.0, -0.0]


def _fp8(x):
    return x.float().clamp(-448, 448).to(FP8)


def _poisoned_pool(npages, Hkv, D, gen):
    sign = lambda *sh: (torch.randint(0, 2, sh, generator=gen) * 2 - 1).float() * 64
    return _fp8(sign(npages, Hkv, P, D)), _fp8(sign(npages, Hkv, D, P))


@pytest.mark.parametrize("B,Hkv,T,D,start", [(2, 2, 19, 64, (9, 30)),
                                             (1, 1, 1, 128, (15,))])
def test_kv_write_fp8_exact(B, Hkv, T, D, start):
    """Tokens across a page boundary into a poisoned pool through a shuffled
    page table: the whole pool, untouched slots included, equals the CPU
    definition exactly."""
    gen = torch.Generator().manual_seed(7)
    maxp, npages = 4, B * 4 + 3
    pt = torch.randperm(npages, generator=gen)[: B * maxp].int().reshape(B, maxp)
    start = torch.tensor(start, dtype=torch.int32)
    k = torch.randn(B, Hkv, T, D, generator=gen) * 3
    v = torch.randn(B, Hkv, T, D, generator=gen) * 3
    sharp = torch.tensor(SHARP)
    k.view(-1)[: len(SHARP)] = sharp
    v.view(-1)[-len(SHARP):] = sharp
    k, v = k.bfloat16(), v.bfloat16()
    kp, vp = _poisoned_pool(npages, Hkv, D, gen)
    kp_g, vp_g = kp.clone().to(DEV), vp.clone().to(DEV)
    ops.kv_write(k.to(DEV), v.to(DEV), kp_g, vp_g, pt.to(DEV), start.to(DEV))
    ref.kv_write(k, v, kp, vp, pt, start)          # the CPU definition
    assert bool(torch.isfinite(kp.float()).all()), "the definition saturates"
    assert torch.equal(kp_g.cpu().float(), kp.float())
    assert torch.equal(vp_g.cpu().float(), vp.float())


def test_rope_kv_write_fp8():
    """q section bit-equal to the bf16 op's, V exact, every stored K within
    one e4m3 ulp at the f32 reference value, 2^(floor(log2|x|) - 3) with floor
    2^-9 (half-ulp rounding plus a neighbour flip from f32 evaluation order)."""
    gen = torch.Generator().manual_seed(8)
    B, T, Hq, Hkv, D = 3, 5, 4, 2, 64
    X = Hq + 2 * Hkv
    start = torch.tensor([3, 13, 30], dtype=torch.int32)
    pos = torch.tensor([[7, 2, 40, 2, 0], [13, 14, 15, 16, 17],
                        [99, 3, 98, 4, 97]], dtype=torch.int32)
    maxp, npages = 4, 17
    pt = torch.randperm(npages, generator=gen)[: B * maxp].int().reshape(B, maxp)
    qkv = (torch.randn(B, T, X * D, generator=gen) * 2).bfloat16()
    qkv[0, 0, -len(SHARP):] = torch.tensor(SHARP).bfloat16()    # into a v head
    cos, sin = ref.rope_cos_sin(D, 128)
    kp0, vp0 = _poisoned_pool(npages, Hkv, D, gen)
    live = torch.zeros(npages, P, dtype=torch.bool)
    for b in range(B):
        for t in range(T):
            p = int(start[b]) + t
            live[int(pt[b, p // P]), p % P] = True

    dev = lambda *xs: [x.to(DEV) for x in xs]
    q16, q8 = qkv.clone().to(DEV), qkv.clone().to(DEV)
    kp16 = torch.zeros(npages, Hkv, P, D, dtype=torch.bfloat16, device=DEV)
    ops.rope_kv_write_(q16, Hq, Hkv, *dev(cos, sin, pos), kp16,
                       kp16.new_zeros(npages, Hkv, D, P), *dev(pt, start))
    kp_g, vp_g = dev(kp0.clone(), vp0.clone())
    ops.rope_kv_write_(q8, Hq, Hkv, *dev(cos, sin, pos), kp_g, vp_g,
                       *dev(pt, start))
    assert torch.equal(q8, q16), "q section must not depend on the pool type"
    assert not torch.equal(q8[..., : Hq * D].cpu(), qkv[..., : Hq * D])

    # the definition: K roped in f32, rounded once; V clamp -> e4m3
    heads = qkv.view(B, T, X, D).permute(0, 2, 1, 3).float()
    k32 = ref.rope_apply(heads[:, :Hq], heads[:, Hq:Hq + Hkv], cos, sin,
                         pos.long())[1].clamp(-448, 448)
    vp_c, want = vp0.clone(), torch.zeros(npages, Hkv, P, D)
    ref.kv_write(k32, heads[:, Hq + Hkv:].contiguous(), kp0.clone(), vp_c, pt, start)
    assert torch.equal(vp_g.cpu().float(), vp_c.float()), "V pool"
    ref.kv_write(k32, k32, want, want.new_zeros(npages, Hkv, D, P), pt, start)
    k_slots = lambda x: x.permute(0, 2, 1, 3)      # (np, P, Hkv, D)
    x = k_slots(want)[live].double()
    got = k_slots(kp_g.cpu().float())[live].double()
    ulp = torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -6))) - 3)
    ratio = float(((got - x).abs() / ulp).max())
    print(f"[kv-fp8] roped K worst |err| / ulp {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(k_slots(kp_g.cpu().float())[~live],
                       k_slots(kp0.float())[~live]), "a K slot outside changed"


def test_llama_block_fp8_pool_gpu_vs_cpu():
    """Prefill T = 33 then 3 decode steps on an fp8 pool, GPU against CPU, at
    the tolerance of the bf16 block parity check (test_gpu_kernels.py)."""
    from bloombee_amd.kv import PagedKVCache
    from bloombee_amd.models.base import resolve_config
    from bloombee_amd.models.llama.block import LlamaBlock

    cfg = dataclasses.replace(resolve_config("llama-mini-gpu"), hidden_size=512,
                              head_dim=64, intermediate_size=1024)
    assert (cfg.num_attention_heads, cfg.num_key_value_heads) == (8, 2)
    torch.manual_seed(12)
    blk = LlamaBlock(cfg, 0).init_random(3)
    B = 2
    xs = [(torch.randn(B, T, cfg.hidden_size) * 0.1).bfloat16()
          for T in (33, 1, 1, 1)]

    def run(block, device):
        pool = PagedKVCache(1, cfg.num_key_value_heads, cfg.head_dim,
                            max_tokens=4096, device=device, dtype=FP8)
        kv = pool.allocate(B, 256)
        outs, at = [], 0
        for x in xs:
            kv.extend(x.shape[1])
            start = torch.full((B,), at, dtype=torch.int32, device=device)
            outs.append(block.forward_inference(x.to(device), kv, start).cpu())
            at += x.shape[1]
        return outs

    want = run(blk, "cpu")
    got = run(blk.to(DEV), DEV)
    err = max(float((g.float() - w.float()).abs().max())
              for g, w in zip(got, want))
    print(f"[kv-fp8] llama block fp8 pool, GPU vs CPU: max |err| {err:.4f}")
    assert err <= 5e-2
