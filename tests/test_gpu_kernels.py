"""GPU kernel parity suite: every gfx950 kernel vs the fp32 torch reference
(mirrors the reference's parity tests, e.g. test_mha_gen_llama_decode_parity.py,
test_optimized_layers.py). All tests @pytest.mark.gpu."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bloombee_amd import ops
    from bloombee_amd.ops import reference as ref

    assert ops.HAVE_HIP_OPS, (
        "HIP extension must be built and loadable on a GPU box (fail-loud policy)"
    )

DEV = "cuda:0"


def to_dev(*ts):
    return [t.to(DEV) for t in ts]


# ---------------------------------------------------------------------------


def test_mfma_fragment_layout():
    """Asymmetric-input check of the assumed A/B/C fragment maps (guide §3)."""
    torch.manual_seed(0)
    A = torch.randn(16, 32).to(torch.bfloat16)
    B = torch.randn(32, 16).to(torch.bfloat16)
    C = ops.mfma_selftest(A.to(DEV), B.to(DEV)).cpu()
    expect = A.float() @ B.float()
    assert torch.allclose(C, expect, atol=2e-2, rtol=1e-2), (
        f"max err {(C - expect).abs().max()} — fragment layout is wrong"
    )


def test_rms_norm_parity():
    torch.manual_seed(1)
    for H in (256, 4096, 8192):
        x = torch.randn(9, H).to(torch.bfloat16)
        w = torch.randn(H).to(torch.bfloat16)
        got = ops.rms_norm(x.to(DEV), w.to(DEV)).cpu().float()
        want = ref.rms_norm(x, w).float()
        assert torch.allclose(got, want, atol=2e-2), (got - want).abs().max()


def test_rms_norm_residual_parity():
    torch.manual_seed(2)
    x = torch.randn(7, 4096).to(torch.bfloat16)
    r = torch.randn(7, 4096).to(torch.bfloat16)
    w = torch.randn(4096).to(torch.bfloat16)
    hg, yg = ops.rms_norm_residual(x.to(DEV), r.to(DEV), w.to(DEV))
    hw, yw = ref.rms_norm_residual(x, r, w)
    assert torch.allclose(hg.cpu().float(), hw.float(), atol=2e-2)
    assert torch.allclose(yg.cpu().float(), yw.float(), atol=2e-2)


def test_layer_norm_parity():
    torch.manual_seed(3)
    x = torch.randn(5, 1024).to(torch.bfloat16)
    w = torch.randn(1024).to(torch.bfloat16)
    b = torch.randn(1024).to(torch.bfloat16)
    got = ops.layer_norm(x.to(DEV), w.to(DEV), b.to(DEV)).cpu().float()
    want = ref.layer_norm(x, w, b).float()
    assert torch.allclose(got, want, atol=3e-2), (got - want).abs().max()


def test_rope_parity():
    torch.manual_seed(4)
    B, Hq, Hkv, T, D = 2, 4, 2, 5, 128
    cos, sin = ref.rope_cos_sin(D, 512)
    q = torch.randn(B, Hq, T, D).to(torch.bfloat16)
    k = torch.randn(B, Hkv, T, D).to(torch.bfloat16)
    pos = torch.randint(0, 500, (B, T)).int()
    qg, kg = q.clone().to(DEV), k.clone().to(DEV)
    ops.rope_apply_(qg, kg, cos.to(DEV), sin.to(DEV), pos.to(DEV))
    qw, kw = ref.rope_apply(q, k, cos, sin, pos)
    assert torch.allclose(qg.cpu().float(), qw.float(), atol=2e-2)
    assert torch.allclose(kg.cpu().float(), kw.float(), atol=2e-2)


def test_swiglu_parity():
    torch.manual_seed(5)
    gu = torch.randn(6, 512).to(torch.bfloat16)
    got = ops.swiglu(gu.to(DEV)).cpu().float()
    want = ref.swiglu(gu[:, :256], gu[:, 256:]).float()
    assert torch.allclose(got, want, atol=2e-2), (got - want).abs().max()


def test_kv_write_gather_parity():
    torch.manual_seed(6)
    B, Hkv, T, D, P = 3, 2, 37, 128, 16
    npages = 32
    kp = torch.zeros(npages, Hkv, P, D).to(torch.bfloat16).to(DEV)
    vp = torch.zeros(npages, Hkv, D, P).to(torch.bfloat16).to(DEV)
    maxp = 8
    pt = (torch.randperm(npages)[: B * maxp]).int().reshape(B, maxp).to(DEV)
    k = torch.randn(B, Hkv, T, D).to(torch.bfloat16)
    v = torch.randn(B, Hkv, T, D).to(torch.bfloat16)
    start = torch.tensor([0, 3, 11], dtype=torch.int32)
    ops.kv_write(k.to(DEV), v.to(DEV), kp, vp, pt, start.to(DEV))
    for b in range(B):
        ctx = int(start[b]) + T
        kg, vg = ops.kv_gather(kp, vp, pt, ctx, b)
        kg = kg.cpu()[:, int(start[b]):]
        vg = vg.cpu()[:, int(start[b]):]
        assert torch.equal(kg, k[b]), f"K mismatch seq {b}"
        assert torch.equal(vg, v[b]), f"V mismatch seq {b}"


def _paged_setup(B, Hq, Hkv, T, D, P=16, seed=7, dtype=torch.bfloat16):
    torch.manual_seed(seed)
    maxp = (T + P - 1) // P + 2
    npages = B * maxp + 4
    kp = torch.zeros(npages, Hkv, P, D, dtype=dtype)
    vp = torch.zeros(npages, Hkv, D, P, dtype=dtype)
    pt = torch.arange(B * maxp, dtype=torch.int32).reshape(B, maxp)
    q = (torch.randn(B, Hq, T, D) / math.sqrt(D)).to(dtype)
    k = torch.randn(B, Hkv, T, D).to(dtype)
    v = torch.randn(B, Hkv, T, D).to(dtype)
    start = torch.zeros(B, dtype=torch.int32)
    ref.kv_write(k, v, kp, vp, pt, start)
    return kp, vp, pt, q, k, v, start


@pytest.mark.parametrize("shape", [
    (2, 8, 2, 33, 128),    # GQA G=4
    (1, 4, 4, 100, 128),   # MHA
    (2, 8, 1, 57, 128),    # MQA G=8
    (1, 2, 2, 300, 64),    # D=64
    (1, 2, 1, 40, 256),    # D=256 (gemma-class)
    (2, 8, 4, 77, 512),    # D=512 wide kernel (gemma-4 global, G=2)
    (1, 4, 4, 130, 512),   # D=512 MHA, crosses page boundaries
    (1, 32, 2, 50, 512),   # D=512 G=16 (MAXG=16 instantiation)
])
def test_attn_decode_parity(shape):
    B, Hq, Hkv, T, D = shape
    kp, vp, pt, q, k, v, start = _paged_setup(B, Hq, Hkv, T, D)
    ctx = torch.full((B,), T, dtype=torch.int32)
    qd = q[:, :, -1:].contiguous()
    want = ref.attn_paged(qd.float(), kp.float(), vp.float(), pt,
                          (ctx - 1).long())
    for n_split in (1, 4):
        got = ops.attn_decode(qd.to(DEV), kp.to(DEV), vp.to(DEV), pt.to(DEV),
                              ctx.to(DEV), n_split=n_split).cpu().float()
        assert torch.allclose(got, want.float(), atol=2e-2), (
            f"n_split={n_split} max err {(got - want).abs().max()}"
        )


@pytest.mark.parametrize("shape", [
    (2, 8, 2, 128, 128),
    (1, 4, 4, 200, 128),   # non-multiple of 64
    (2, 8, 8, 64, 64),
    (1, 2, 1, 96, 256),
])
def test_attn_prefill_parity(shape):
    B, Hq, Hkv, T, D = shape
    kp, vp, pt, q, k, v, start = _paged_setup(B, Hq, Hkv, T, D, seed=8)
    want = ref.attn_paged(q.float(), kp.float(), vp.float(), pt, start.long())
    got = ops.attn_prefill(q.to(DEV), kp.to(DEV), vp.to(DEV), pt.to(DEV),
                           start.to(DEV)).cpu().float()
    assert torch.allclose(got, want.float(), atol=2e-2), (
        f"max err {(got - want).abs().max()}"
    )


def test_attn_prefill_with_prefix():
    """Multi-turn: new chunk attends to existing cache prefix."""
    B, Hq, Hkv, T, D = 1, 4, 2, 48, 128
    kp, vp, pt, q, k, v, start = _paged_setup(B, Hq, Hkv, T, D, seed=9)
    Tnew = 16
    qn = q[:, :, -Tnew:].contiguous()
    qs = torch.tensor([T - Tnew], dtype=torch.int32)
    want = ref.attn_paged(qn.float(), kp.float(), vp.float(), pt, qs.long())
    got = ops.attn_prefill(qn.to(DEV), kp.to(DEV), vp.to(DEV), pt.to(DEV),
                           qs.to(DEV)).cpu().float()
    assert torch.allclose(got, want.float(), atol=2e-2), (got - want).abs().max()


def test_attn_decode_sliding_window():
    B, Hq, Hkv, T, D = 1, 4, 2, 100, 128
    kp, vp, pt, q, k, v, start = _paged_setup(B, Hq, Hkv, T, D, seed=10)
    ctx = torch.full((B,), T, dtype=torch.int32)
    qd = q[:, :, -1:].contiguous()
    win = 32
    want = ref.attn_paged(qd.float(), kp.float(), vp.float(), pt,
                          (ctx - 1).long(), sliding_window=win)
    got = ops.attn_decode(qd.to(DEV), kp.to(DEV), vp.to(DEV), pt.to(DEV),
                          ctx.to(DEV), window=win).cpu().float()
    assert torch.allclose(got, want.float(), atol=2e-2)


def test_quant4_parity():
    torch.manual_seed(11)
    x = torch.randn(16, 256).to(torch.bfloat16)
    pg, sg, zg = ops.quant4_pack(x.to(DEV))
    pw, sw, zw = ref.quant4_pack(x)
    assert torch.equal(pg.cpu(), pw.reshape(16, 128))
    y = ops.quant4_unpack(pg, sg, zg).cpu()
    yw = ref.quant4_unpack(pw, sw, zw)
    assert torch.allclose(y.float(), yw.float(), atol=2e-2)


def test_block_forward_gpu_vs_cpu():
    """Whole llama block: GPU HIP path vs CPU reference path."""
    from bloombee_amd.kv import PagedKVCache
    from bloombee_amd.models.base import resolve_config
    from bloombee_amd.models.llama.block import LlamaBlock

    cfg = resolve_config("llama-mini-gpu")
    torch.manual_seed(12)
    blk = LlamaBlock(cfg, 0).init_random(3)
    B, T = 2, 24
    x = (torch.randn(B, T, cfg.hidden_size) * 0.1).to(torch.bfloat16)
    start = torch.zeros(B, dtype=torch.int32)

    pool_c = PagedKVCache(1, cfg.num_key_value_heads, cfg.head_dim,
                          max_tokens=4096, device="cpu", dtype=torch.bfloat16)
    kv_c = pool_c.allocate(B, 256)
    kv_c.extend(T)
    y_cpu = blk.forward_inference(x, kv_c, start)

    blk_g = blk.to(DEV)
    pool_g = PagedKVCache(1, cfg.num_key_value_heads, cfg.head_dim,
                          max_tokens=4096, device=DEV, dtype=torch.bfloat16)
    kv_g = pool_g.allocate(B, 256)
    kv_g.extend(T)
    y_gpu = blk_g.forward_inference(x.to(DEV), kv_g, start.to(DEV)).cpu()
    assert torch.allclose(y_gpu.float(), y_cpu.float(), atol=5e-2), (
        (y_gpu.float() - y_cpu.float()).abs().max()
    )


def test_generate_gpu_decode_consistent_with_prefill():
    """End-to-end on GPU: decode-step tokens must equal re-prefilling the
    grown prefix (kernel-level decode/prefill consistency, full model)."""
    from bloombee_amd.engine import LocalEngine

    ids = torch.randint(0, 1000, (2, 8), generator=torch.Generator().manual_seed(5))
    eng = LocalEngine("llama-mini-gpu", device=DEV, seed=4, kv_max_tokens=8192)
    out = eng.generate_greedy(ids, 6)
    for i in range(1, 6):
        kv = eng.kv_pool.allocate(2, 64)
        full = torch.cat([ids.to(DEV), out[:, :i]], dim=1)
        nxt = eng.prefill(full, kv)
        kv.close()
        assert torch.equal(nxt, out[:, i]), f"mismatch at step {i}"


def test_fused_qkv_path_parity():
    """rope_kv_write_ + attn_paged_qkv on GPU vs the composed CPU reference."""
    torch.manual_seed(20)
    B, Hq, Hkv, D, P = 2, 8, 2, 128, 16
    X = Hq + 2 * Hkv
    maxp = 8
    for T, start0 in [(1, 30), (40, 0)]:
        kp_c = torch.zeros(B * maxp + 2, Hkv, P, D, dtype=torch.bfloat16)
        vp_c = torch.zeros(B * maxp + 2, Hkv, D, P, dtype=torch.bfloat16)
        pt = torch.arange(B * maxp, dtype=torch.int32).reshape(B, maxp)
        qkv = (torch.randn(B, T, X * D) * 0.3).to(torch.bfloat16)
        start = torch.full((B,), start0, dtype=torch.int32)
        if start0:
            # pre-fill some history
            kh = torch.randn(B, Hkv, start0, D).to(torch.bfloat16)
            vh = torch.randn(B, Hkv, start0, D).to(torch.bfloat16)
            ref.kv_write(kh, vh, kp_c, vp_c, pt, torch.zeros(B, dtype=torch.int32))
        kp_g, vp_g = kp_c.clone().to(DEV), vp_c.clone().to(DEV)
        qkv_g = qkv.clone().to(DEV)
        cos, sin = ref.rope_cos_sin(D, 512)

        ops.rope_kv_write_(qkv, Hq, Hkv, cos, sin, None, kp_c, vp_c, pt, start)
        out_c = ops.attn_paged_qkv(qkv, Hq, Hkv, kp_c, vp_c, pt, start.long())

        ops.rope_kv_write_(qkv_g, Hq, Hkv, cos.to(DEV), sin.to(DEV), None,
                           kp_g, vp_g, pt.to(DEV), start.to(DEV))
        out_g = ops.attn_paged_qkv(qkv_g, Hq, Hkv, kp_g, vp_g, pt.to(DEV),
                                   start.to(DEV))
        assert torch.allclose(qkv_g.cpu().float(), qkv.float(), atol=2e-2), \
            f"T={T}: roped q mismatch {(qkv_g.cpu().float()-qkv.float()).abs().max()}"
        assert torch.allclose(kp_g.cpu().float(), kp_c.float(), atol=2e-2), \
            f"T={T}: k pages mismatch"
        assert torch.allclose(out_g.cpu().float(), out_c.float(), atol=3e-2), \
            f"T={T}: attn out mismatch {(out_g.cpu().float()-out_c.float()).abs().max()}"


@pytest.mark.parametrize("M,N,K,ksplit", [
    (32, 4096, 4096, 0), (32, 6144, 4096, 1), (17, 4096, 4096, 8),
    (8, 256, 14336, 0), (32, 28672, 4096, 2), (1, 4096, 4096, 0),
])
def test_gemm_skinny_parity(M, N, K, ksplit):
    torch.manual_seed(11)
    x = (torch.randn(M, K) / math.sqrt(K)).to(torch.bfloat16).to(DEV)
    w = torch.randn(N, K).to(torch.bfloat16).to(DEV)
    r = torch.randn(M, N).to(torch.bfloat16).to(DEV)
    bias = torch.randn(N).to(torch.bfloat16).to(DEV)
    want = torch.nn.functional.linear(x.float(), w.float(), bias.float()) + r.float()
    got = ops.hip_ops.gemm_skinny(x, w, r, bias, ksplit).float()
    assert torch.allclose(got.cpu(), want.cpu(), atol=5e-2, rtol=5e-2), \
        (got.cpu() - want.cpu()).abs().max()


def test_linear_dispatch_matches_f_linear():
    torch.manual_seed(3)
    x = (torch.randn(2, 1, 512) * 0.1).to(torch.bfloat16).to(DEV)
    w = torch.randn(256, 512).to(torch.bfloat16).to(DEV)
    got = ops.linear(x, w)
    want = torch.nn.functional.linear(x, w)
    assert torch.allclose(got.float().cpu(), want.float().cpu(), atol=2e-2)


@pytest.mark.parametrize("model", ["llama-tiny", "qwen3-tiny", "mixtral-tiny"])
def test_family_engine_gpu_matches_cpu_tokens(model, monkeypatch):
    """Families whose decode path runs the HIP kernels must produce the same
    greedy tokens as the CPU reference engine (identical weights, copied).
    Fused-norm is pinned OFF here: it reparameterizes the weights (norm
    fold), which legitimately shifts near-flat random-init logits — its
    own parity is covered by test_llama_block_fused_norm_matches_unfused."""
    from bloombee_amd.engine import LocalEngine
    from bloombee_amd.ops import interface as iface
    monkeypatch.setattr(iface, "_FUSE_NORM", False)

    ids = torch.randint(0, 900, (2, 12), generator=torch.Generator().manual_seed(2))
    cpu = LocalEngine(model, device="cpu", seed=0, kv_max_tokens=8192)
    want = cpu.generate_greedy(ids, 8)
    gpu = LocalEngine(model, device=DEV, seed=0, kv_max_tokens=8192)
    # copy the CPU engine weights so both run identical parameters
    gpu.embed.copy_(cpu.embed.to(DEV))
    gpu.final_norm_w.copy_(cpu.final_norm_w.to(DEV))
    if not cpu.config.tie_word_embeddings:
        gpu.lm_head_w.copy_(cpu.lm_head_w.to(DEV))
    for gb, cb in zip(gpu.stack.blocks, cpu.stack.blocks):
        for (n1, pg), (n2, pc) in zip(gb.named_parameters(), cb.named_parameters()):
            assert n1 == n2
            pg.data.copy_(pc.data.to(DEV))
    got = gpu.generate_greedy(ids, 8).cpu()
    # bf16 kernel vs fp32-accum reference: argmax tokens may diverge late on
    # random-init models; require the first 6 to agree exactly
    assert torch.equal(got[:, :6], want[:, :6]), (got, want)


def test_attn_decode_alibi_parity():
    B, Hq, Hkv, T, D = 3, 8, 8, 70, 64
    kp, vp, pt, q, k, v, start = _paged_setup(B, Hq, Hkv, T, D, seed=13)
    slopes = ops.alibi_slopes_for(Hq)
    ctx = torch.full((B,), T, dtype=torch.int32)
    want = ref.attn_paged(q[:, :, -1:], kp, vp, pt, (ctx - 1).long(),
                          1.0 / math.sqrt(D), alibi_slopes=slopes)
    got = ops.attn_decode(q[:, :, -1:].to(DEV), kp.to(DEV), vp.to(DEV),
                          pt.to(DEV), ctx.to(DEV), alibi_slopes=slopes)
    assert torch.allclose(got.cpu().float(), want.float(), atol=3e-2), \
        (got.cpu().float() - want.float()).abs().max()


def test_attn_prefill_alibi_parity():
    B, Hq, Hkv, T, D = 2, 4, 4, 33, 64
    kp, vp, pt, q, k, v, start = _paged_setup(B, Hq, Hkv, T, D, seed=14)
    slopes = ops.alibi_slopes_for(Hq)
    qs = torch.zeros(B, dtype=torch.int64)
    want = ref.attn_paged(q, kp, vp, pt, qs, 1.0 / math.sqrt(D),
                          alibi_slopes=slopes)
    got = ops.attn_prefill(q.to(DEV), kp.to(DEV), vp.to(DEV), pt.to(DEV),
                           qs.int().to(DEV), alibi_slopes=slopes)
    assert torch.allclose(got.cpu().float(), want.float(), atol=3e-2), \
        (got.cpu().float() - want.float()).abs().max()


def test_attn_decode_wide_mqa_group():
    """GQA group wider than the 16-row MFMA q-tile (falcon-7b G=71 class):
    chunked launch must match the reference."""
    B, Hq, Hkv, T, D = 2, 24, 1, 50, 64
    kp, vp, pt, q, k, v, start = _paged_setup(B, Hq, Hkv, T, D, seed=15)
    ctx = torch.full((B,), T, dtype=torch.int32)
    want = ref.attn_paged(q[:, :, -1:], kp, vp, pt, (ctx - 1).long(),
                          1.0 / math.sqrt(D))
    for ns in (1, 4):
        got = ops.attn_decode(q[:, :, -1:].to(DEV), kp.to(DEV), vp.to(DEV),
                              pt.to(DEV), ctx.to(DEV), n_split=ns)
        assert torch.allclose(got.cpu().float(), want.float(), atol=3e-2), \
            (ns, (got.cpu().float() - want.float()).abs().max())


def test_bloom_engine_gpu_matches_cpu_tokens():
    from bloombee_amd.engine import LocalEngine

    ids = torch.randint(0, 900, (2, 10), generator=torch.Generator().manual_seed(3))
    cpu = LocalEngine("bloom-tiny", device="cpu", seed=0, kv_max_tokens=8192)
    want = cpu.generate_greedy(ids, 6)
    gpu = LocalEngine("bloom-tiny", device=DEV, seed=0, kv_max_tokens=8192)
    gpu.embed.copy_(cpu.embed.to(DEV))
    for gb, cb in zip(gpu.stack.blocks, cpu.stack.blocks):
        for (n1, pg), (n2, pc) in zip(gb.named_parameters(), cb.named_parameters()):
            pg.data.copy_(pc.data.to(DEV))
    got = gpu.generate_greedy(ids, 6).cpu()
    assert torch.equal(got[:, :4], want[:, :4]), (got, want)


def test_gemma4_engine_gpu_matches_cpu_tokens():
    from bloombee_amd.engine import LocalEngine

    ids = torch.randint(0, 500, (2, 10), generator=torch.Generator().manual_seed(4))
    cpu = LocalEngine("gemma4-tiny", device="cpu", seed=0, kv_max_tokens=8192)
    want = cpu.generate_greedy(ids, 6)
    gpu = LocalEngine("gemma4-tiny", device=DEV, seed=0, kv_max_tokens=8192)
    gpu.embed.copy_(cpu.embed.to(DEV))
    for gb, cb in zip(gpu.stack.blocks, cpu.stack.blocks):
        for (n1, pg), (n2, pc) in zip(gb.named_parameters(), cb.named_parameters()):
            pg.data.copy_(pc.data.to(DEV))
    got = gpu.generate_greedy(ids, 6).cpu()
    assert torch.equal(got[:, :4], want[:, :4]), (got, want)


def test_kv_swap_roundtrip_gpu():
    """Pinned-host swap-out/in on device (micro-batch KV offload parity)."""
    from bloombee_amd.kv.paged import PagedKVCache

    pool = PagedKVCache(num_layers=2, num_kv_heads=2, head_dim=64,
                        page_size=16, max_tokens=1024, device=DEV)
    h = pool.allocate(2, 128)
    k = torch.randn(2, 2, 40, 64).to(torch.bfloat16).to(DEV)
    v = torch.randn(2, 2, 40, 64).to(torch.bfloat16).to(DEV)
    h.extend(40)
    for l in range(2):
        ops.kv_write(k, v, h.k_pages(l), h.v_pages(l), h.page_table(),
                     torch.zeros(2, dtype=torch.int32, device=DEV))
    before = [ops.kv_gather(h.k_pages(l), h.v_pages(l), h.page_table(), 40, 1)
              for l in range(2)]
    h.swap_out()
    h.swap_in()
    after = [ops.kv_gather(h.k_pages(l), h.v_pages(l), h.page_table(), 40, 1)
             for l in range(2)]
    for (kb, vb), (ka, va) in zip(before, after):
        assert torch.equal(kb, ka) and torch.equal(vb, va)
    h.close()


def test_moe_gemm_grouped_parity():
    """Grouped MoE GEMM (moe_gemm.hip) vs the fp32 reference: ragged expert
    groups (incl. empty experts), rowmap gather, per-slot scale."""
    from bloombee_amd.ops import interface as iface
    torch.manual_seed(11)
    T, K, E, H, N = 27, 2, 8, 256, 128
    A = torch.randn(T, H).to(torch.bfloat16)
    W = (torch.randn(E, N, H) * 0.1).to(torch.bfloat16)
    experts = torch.randint(0, E - 1, (T, K))  # expert E-1 stays empty
    order = experts.reshape(-1).argsort(stable=True)
    counts = torch.bincount(experts.reshape(-1), minlength=E)
    off = torch.zeros(E + 1, dtype=torch.int32)
    off[1:] = counts.cumsum(0).int()
    tok = (order // K).int()
    scale = torch.rand(T * K)
    want = ref.moe_gemm_grouped(A.float(), W.float(), off, rowmap=tok,
                                scale=scale, S=T * K)
    got = iface.hip_ops.moe_gemm(A.to(DEV), W.to(DEV), off.to(DEV),
                                 tok.to(DEV), scale.to(DEV), T * K,
                                 (T + 31) // 32).cpu().float()
    assert torch.allclose(got, want.float(), atol=3e-2), \
        (got - want).abs().max()
    # identity rowmap + no scale (down-GEMM shape)
    A2 = torch.randn(T * K, N).to(torch.bfloat16)
    W2 = (torch.randn(E, 64, N) * 0.1).to(torch.bfloat16)
    want2 = ref.moe_gemm_grouped(A2.float(), W2.float(), off, S=T * K)
    got2 = iface.hip_ops.moe_gemm(A2.to(DEV), W2.to(DEV), off.to(DEV),
                                  None, None, T * K, (T * K + 31) // 32)
    assert torch.allclose(got2.cpu().float(), want2.float(), atol=3e-2)


def test_mixtral_block_grouped_moe_decode():
    """The grouped-MoE wiring in the Mixtral block: same device, same
    weights, grouped path vs per-expert loop path (moe_loop switch) — only
    the MoE implementation differs, so tolerance is tight. (CPU-vs-GPU
    whole-block noise is covered by the family parity suite.)"""
    from bloombee_amd.engine import BlockStack
    from bloombee_amd.models.base import resolve_config

    cfg = resolve_config("mixtral-tiny")
    torch.manual_seed(0)
    gpu = BlockStack(cfg, 0, 1, device=DEV, seed=3)
    blk = gpu.blocks[0]
    # widen router margins so near-ties cannot flip top-k between the two
    # MoE implementations' (identical) routing math
    rw = torch.randn(blk.router_w.shape,
                     generator=torch.Generator().manual_seed(42))
    with torch.no_grad():
        blk.router_w.copy_(rw.to(cfg.dtype))
    gen = torch.Generator().manual_seed(2)
    for B, T in [(4, 10), (7, 1), (32, 1)]:
        y = (torch.randn(B, T, cfg.hidden_size, generator=gen) * 0.1) \
            .to(cfg.dtype).to(DEV)
        blk.moe_loop = False
        out_grp = blk._moe(y)
        blk.moe_loop = True
        out_loop = blk._moe(y)
        blk.moe_loop = False
        assert torch.allclose(out_grp.float(), out_loop.float(),
                              atol=2e-2), \
            (B, T, (out_grp - out_loop).abs().max().item())


def test_gemm_w4_parity():
    """4-bit weight-stream GEMM (w4_gemm.hip) vs dequant + fp32 matmul, with
    and without split-K and the residual/bias epilogue."""
    from bloombee_amd.ops import interface as iface
    torch.manual_seed(6)
    for (M, N, K) in [(4, 128, 256), (32, 256, 512), (17, 64, 1024),
                      (1, 192, 2048), (1, 128, 4096)]:  # GEMV path (M=1)
        w = (torch.randn(N, K) * 0.5)
        x = (torch.randn(M, K) * 0.5).to(torch.bfloat16)
        packed, scale, zero = ref.quant4_pack(w)
        wq = ref.quant4_unpack(packed, scale, zero,
                               dtype=torch.float32).reshape(N, K)
        want = x.float() @ wq.t()
        pk = packed.reshape(N, K // 2).to(DEV)
        sc = scale.reshape(N, K // 64).half().to(DEV)
        zp = zero.reshape(N, K // 64).half().to(DEV)
        xh = x.half().to(DEV)  # the kernel computes in f16
        for ks in (1, 2):
            got = iface.hip_ops.gemm_w4(xh, pk, sc, zp, None, None,
                                        N, ks).cpu().float()
            assert torch.allclose(got, want, atol=5e-2, rtol=2e-2), \
                (M, N, K, ks, (got - want).abs().max())
        r = (torch.randn(M, N) * 0.5).to(torch.bfloat16)
        b = (torch.randn(N) * 0.5).to(torch.bfloat16)
        got = iface.hip_ops.gemm_w4(xh, pk, sc, zp, r.to(DEV),
                                    b.to(DEV), N, 1).cpu().float()
        assert torch.allclose(got, want + r.float() + b.float(),
                              atol=5e-2, rtol=2e-2)


def test_llama_quantized_engine_decode_gpu():
    """Quantized llama block on GPU (w4 kernel, K%128==0 shapes) tracks the
    CPU fallback (dequant matmul) on the SAME codes — the CPU reference
    pack and the GPU pack kernel round nibbles independently, so the codes
    are copied from the CPU quantization to isolate the GEMM itself."""
    from bloombee_amd.engine import BlockStack
    from bloombee_amd.models.base import resolve_config

    cfg = resolve_config("llama-mini-gpu")  # K=1024/2816: the kernel path
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
    x = (torch.randn(2, 1, cfg.hidden_size, generator=gen) * 0.1).to(cfg.dtype)
    sp = torch.zeros(2, dtype=torch.int32)
    hc.extend(1)
    hg.extend(1)
    yc = cpu.forward_inference(x.clone(), hc, sp)
    yg = gpu.forward_inference(x.to(DEV), hg, sp.to(DEV))
    assert torch.allclose(yg.cpu().float(), yc.float(), atol=3e-2), \
        (yg.cpu().float() - yc.float()).abs().max()


@pytest.mark.gpu
def test_gemm_skinny_fused_norm_parity():
    """gemm_skinny norm_w path == rms_norm kernel + unfused gemm_skinny
    (the fused path skips the intermediate bf16 write; tolerance covers
    that rounding difference)."""
    torch.manual_seed(11)
    for M, N, K in [(1, 4096, 4096), (8, 6144, 4096), (32, 4096, 14336),
                    (32, 28672, 4096), (17, 512, 512)]:
        x = (torch.randn(M, K, dtype=torch.bfloat16, device=DEV) * 0.5)
        w = torch.randn(N, K, dtype=torch.bfloat16, device=DEV) * 0.05
        nw = torch.randn(K, dtype=torch.bfloat16, device=DEV)
        r = torch.randn(M, N, dtype=torch.bfloat16, device=DEV)
        want = ops.hip_ops.gemm_skinny(
            ops.rms_norm(x, nw, 1e-5).contiguous(), w, r, None, 0)
        got = ops.hip_ops.gemm_skinny(x, w, r, None, 0, nw, 1e-5)
        err = (got.float() - want.float()).abs().max().item()
        scale = want.float().abs().max().clamp_min(1.0).item()
        assert err / scale < 2e-2, (M, N, K, err, scale)


@pytest.mark.gpu
def test_llama_block_fused_norm_matches_unfused():
    """Whole-block decode with the fused-norm path vs BBAMD_FUSE_NORM=0
    semantics (monkeypatched): same inputs, outputs within bf16 noise."""
    from bloombee_amd.engine import BlockStack
    from bloombee_amd.models.base import resolve_config
    from bloombee_amd.ops import interface as iface

    cfg = resolve_config("llama-mini-gpu")
    stack = BlockStack(cfg, 0, 2, device=DEV, seed=9)
    gen = torch.Generator().manual_seed(4)
    x = (torch.randn(2, 1, cfg.hidden_size, generator=gen) * 0.1).to(cfg.dtype)
    sp = torch.zeros(2, dtype=torch.int32)

    outs = []
    for fuse in (True, False):
        kv = stack.make_kv(1 << 10)
        h = kv.allocate(2, 32)
        h.extend(1)
        old = iface._FUSE_NORM
        iface._FUSE_NORM = fuse
        try:
            outs.append(stack.forward_inference(x.to(DEV), h, sp.to(DEV)))
        finally:
            iface._FUSE_NORM = old
    err = (outs[0].float() - outs[1].float()).abs().max().item()
    assert err < 3e-2, err


@pytest.mark.gpu
def test_gemm_skinny_ss_chain():
    """Epilogue-emitted row sum-of-squares: ss_out matches the row sums of
    the produced C (both the ksplit==1 in-kernel path and the split-K
    combine_ss path), and a consumer GEMM using ss_in matches one that
    re-streams A for its variance."""
    torch.manual_seed(13)
    for M, N, K in [(8, 512, 512),        # ksplit==1 epilogue path
                    (32, 4096, 4096),     # split-K combine_ss path
                    (32, 4096, 14336)]:
        x = torch.randn(M, K, dtype=torch.bfloat16, device=DEV) * 0.3
        w = torch.randn(N, K, dtype=torch.bfloat16, device=DEV) * 0.05
        r = torch.randn(M, N, dtype=torch.bfloat16, device=DEV)
        ss = torch.full((N // 64 * 32,), float("nan"), device=DEV)
        c = ops.hip_ops.gemm_skinny(x, w, r, None, 0, None, 0.0, None, ss)
        want_ss = c.float().pow(2).sum(-1)
        got_ss = ss.view(-1, 32)[:, :M].sum(0)
        rel = ((got_ss - want_ss).abs() / want_ss.clamp_min(1e-3)).max().item()
        assert rel < 2e-2, (M, N, K, rel)

        # consumer: fused norm via ss_in == fused norm via A re-stream
        w2 = torch.randn(256, N, dtype=torch.bfloat16, device=DEV) * 0.05
        nw = torch.randn(N, dtype=torch.bfloat16, device=DEV)
        y_self = ops.hip_ops.gemm_skinny(c, w2, None, None, 0, nw, 1e-5)
        y_ssin = ops.hip_ops.gemm_skinny(c, w2, None, None, 0, nw, 1e-5,
                                         ss.contiguous(), None)
        err = (y_self.float() - y_ssin.float()).abs().max().item()
        sc = y_self.float().abs().max().clamp_min(1.0).item()
        assert err / sc < 1e-2, (M, N, K, err)


@pytest.mark.gpu
def test_qwen3_block_fused_norm_matches_unfused():
    """Qwen3 inherits the fused-norm chain (q/k per-head norms act on the
    GEMM output and are unaffected by the input-norm fold)."""
    from bloombee_amd.engine import BlockStack
    from bloombee_amd.models.base import resolve_config
    from bloombee_amd.ops import interface as iface

    cfg = resolve_config("qwen3-tiny")
    stack = BlockStack(cfg, 0, 2, device=DEV, seed=21)
    gen = torch.Generator().manual_seed(5)
    x = (torch.randn(2, 1, cfg.hidden_size, generator=gen) * 0.1).to(cfg.dtype)
    sp = torch.zeros(2, dtype=torch.int32)
    outs = []
    for fuse in (True, False):
        kv = stack.make_kv(1 << 10)
        h = kv.allocate(2, 32)
        h.extend(1)
        old = iface._FUSE_NORM
        iface._FUSE_NORM = fuse
        try:
            outs.append(stack.forward_inference(x.to(DEV), h, sp.to(DEV)))
        finally:
            iface._FUSE_NORM = old
    err = (outs[0].float() - outs[1].float()).abs().max().item()
    assert err < 3e-2, err


@pytest.mark.gpu
def test_gemm_w4_small_m_parity():
    """linear_w4 at M = 1..4 vs the dequantized F.linear reference. Only
    M == 1 runs the GEMV (gemm_w4 in ext.hip dispatches it for M == 1
    alone); M = 2..4 exercise the split-K MFMA form. The GEMV is a
    single-row kernel: its multi-row form was measured slower and removed."""
    torch.manual_seed(17)
    for M in (1, 2, 3, 4):
        for N, K in [(512, 2048), (1024, 4096), (256, 14336)]:
            w = torch.randn(N, K, dtype=torch.bfloat16, device=DEV) * 0.05
            packed, scale, zero = ops.quant4_pack(w)
            wd = ops.quant4_unpack(packed.reshape(-1, 32), scale.reshape(-1),
                                   zero.reshape(-1),
                                   dtype=torch.bfloat16).reshape(N, K)
            x = torch.randn(M, K, dtype=torch.bfloat16, device=DEV) * 0.3
            r = torch.randn(M, N, dtype=torch.bfloat16, device=DEV)
            want = torch.nn.functional.linear(x.float(), wd.float()) + r.float()
            got = ops.linear_w4(x, packed, scale, zero, N, residual=r)
            err = (got.float() - want).abs().max().item()
            sc = want.abs().max().clamp_min(1.0).item()
            assert err / sc < 2e-2, (M, N, K, err / sc)
