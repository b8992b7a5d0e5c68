"""Fused decode-GEMM epilogues against the unfused kernels, bit for bit.

  1. SwiGLU in the gate_up GEMM (gemm_skinny_swiglu)   vs gemm_skinny + swiglu
  2. qkv split-K slabs into rope_kv_write_part         vs combine + rope_kv_write_
  3. in-launch split-K reduce (gemm_skinny cnt=...)    vs GEMM + combine launch
  4. a two-block llama / qwen3 stack, all switches on  vs all off

Every comparison with the unfused path is `torch.equal`: the fused kernels
round at the same places and sum in the same order. Exact-arithmetic data
(tests/fused_cases.py, gemm_cases.py) is also held against its fp64
expectation; realistic randn data is there because integer data cannot see
a reordered f32 sum.
"""
import pytest
import torch

import fused_cases as fc
import gemm_cases as gc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bloombee_amd import ops
    from bloombee_amd.ops import interface as iface

    assert ops.HAVE_HIP_OPS, (
        "HIP extension must be built and loadable on a GPU box (fail-loud policy)"
    )

DEV = "cuda:0"
BF = torch.bfloat16


def dev(t, dtype=BF):
    return None if t is None else t.to(dtype).to(DEV)


def _randn_bf(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(BF)


def assert_same(got, want, what):
    if torch.equal(got, want):
        return
    g, w = got.detach().cpu().double(), want.detach().cpu().double()
    err = (g - w).abs()
    err[g.isnan() | w.isnan()] = float("inf")
    flat = int(err.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), w.shape))
    raise AssertionError(
        f"{what}: {int((err > 0).sum())} of {w.numel()} elements differ from the "
        f"unfused path; worst at {idx}: got {float(g[idx])}, want {float(w[idx])}")


# ---------------------------------------------------------------------------
# 1. SwiGLU-fused gate_up GEMM
# ---------------------------------------------------------------------------

def _gate_up_then_swiglu(a, w, eps, ss_in, mode):
    gu = ops.hip_ops.gemm_skinny(a, w, None, None, 1, None, eps, ss_in, None, mode)
    return ops.hip_ops.swiglu(gu)


@pytest.mark.parametrize("spec", fc.SWIGLU_SPECS, ids=gc.ids(fc.SWIGLU_SPECS))
def test_swiglu_gemm(spec):
    M, K, I = spec.M, spec.K, spec.N // 2
    mode = 2 if spec.kind == "norm" else 0
    # exact data: the unfused pair, then fp64
    c = fc.build_swiglu(spec)
    a = dev(c.Abuf)[:M]
    w = dev(c.Wfold if mode == 2 else c.W)
    ss_in = dev(c.ss_in, torch.float32).contiguous() if mode == 2 else None
    got = ops.hip_ops.gemm_skinny_swiglu(a, w, 0.0, ss_in, mode)
    assert tuple(got.shape) == (M, I) and got.dtype == BF
    assert_same(got, _gate_up_then_swiglu(a, w, 0.0, ss_in, mode), spec.name)
    err = (got.cpu().double() - c.want_act).abs()
    ratio = float((err / fc.act_bound(c)).max())
    print(f"{spec.name}: worst |err| / bound against fp64 {ratio:.3f}")
    assert ratio <= 1.0
    # realistic data: the unfused pair only
    gen = torch.Generator().manual_seed(1000 + spec.seed)
    a = _randn_bf(gen, M + 3, K).to(DEV)[:M]
    w = _randn_bf(gen, 2 * I, K, scale=K ** -0.5).to(DEV)
    eps = 1e-5 if mode == 2 else 0.0
    ss_in = None
    if mode == 2:       # per-stripe row sums of squares of a, 4 stripes of K/4
        ss_in = torch.ones(4, 32, device=DEV)
        ss_in[:, :M] = (a.float() ** 2).view(M, 4, K // 4).sum(-1).T
    got = ops.hip_ops.gemm_skinny_swiglu(a, w, eps, ss_in, mode)
    assert_same(got, _gate_up_then_swiglu(a, w, eps, ss_in, mode),
                spec.name + " randn")


def test_linear_swiglu_switch(monkeypatch):
    """ops.linear_swiglu: fused by default, BBAMD_FUSE_SWIGLU=0 (the module
    switch) restores linear + swiglu; 3-D input; mode 2 without ss_in."""
    gen = torch.Generator().manual_seed(7)
    x = _randn_bf(gen, 17, 1, 512).to(DEV)
    w = _randn_bf(gen, 2 * 352, 512, scale=512 ** -0.5).to(DEV)
    assert ops.fuse_swiglu_ok(x, w)
    # a narrow gate_up with K >= 1024 splits K when run on its own: not fused
    assert not ops.fuse_swiglu_ok(torch.empty(17, 1024, dtype=BF, device=DEV),
                                  torch.empty(2048, 1024, dtype=BF, device="meta"))
    assert ops.fuse_swiglu_ok(torch.empty(32, 4096, dtype=BF, device=DEV),
                              torch.empty(28672, 4096, dtype=BF, device="meta"))
    for norm in (None, (None, 1e-5)):
        on = ops.linear_swiglu(x, w, norm=norm)
        assert tuple(on.shape) == (17, 1, 352)
        monkeypatch.setattr(iface, "_FUSE_SWIGLU", False)
        assert not ops.fuse_swiglu_ok(x, w)
        off = ops.linear_swiglu(x, w, norm=norm)
        monkeypatch.setattr(iface, "_FUSE_SWIGLU", True)
        assert_same(on, off, f"linear_swiglu norm={norm}")


# ---------------------------------------------------------------------------
# 2. split-K slabs into rope_kv_write
# ---------------------------------------------------------------------------

SENTINEL = 12352.0     # exact in bf16, far outside the data
MAXPOS = 64


@pytest.mark.parametrize("K,ks", [(512, 2), (2304, 3)])
@pytest.mark.parametrize("Hq,Hkv,D", [(4, 2, 64), (8, 1, 128)])
@pytest.mark.parametrize("B,T", [(1, 1), (3, 1), (32, 1), (16, 2)])
def test_rope_from_partials(B, T, Hq, Hkv, D, K, ks):
    P, maxp = 16, 3
    X = Hq + 2 * Hkv
    N, M = X * D, B * T
    gen = torch.Generator().manual_seed(B * 100 + T * 10 + Hq + K)
    x = _randn_bf(gen, M, K).to(DEV)
    w = _randn_bf(gen, N, K, scale=K ** -0.5).to(DEV)
    bias_t = _randn_bf(gen, N).to(DEV)
    cos, sin = ops.rope_cos_sin(D, MAXPOS)
    cos, sin = cos.to(DEV), sin.to(DEV)
    npages = B * maxp + 2
    # every row owns maxp distinct pages, in a scrambled order
    perm = torch.randperm(npages, generator=gen)[: B * maxp]
    pt = perm.view(B, maxp).int().to(DEV)
    pos_t = torch.randint(0, MAXPOS, (B, T), generator=gen).int().to(DEV)

    part = ops.hip_ops.gemm_skinny(x, w, None, None, ks, None, 0.0, None, None,
                                   0, True, None)
    assert part.dtype == torch.float32 and tuple(part.shape) == (ks, M, N)
    for bias in (None, bias_t):
        unfused = ops.hip_ops.gemm_skinny(x, w, None, bias, ks).view(B, T, N)
        for sp in (0, 15, 16, 31):
            start = torch.full((B,), sp, dtype=torch.int32, device=DEV)
            for pos in (None, pos_t):
                what = f"bias={bias is not None} start={sp} pos={pos is not None}"
                kp0 = torch.full((npages, Hkv, P, D), SENTINEL, dtype=BF, device=DEV)
                vp0 = torch.full((npages, Hkv, D, P), SENTINEL, dtype=BF, device=DEV)
                kp1, vp1 = kp0.clone(), vp0.clone()
                q0 = unfused.clone()
                ops.rope_kv_write_(q0, Hq, Hkv, cos, sin, pos, kp0, vp0, pt, start)
                q1, ctx = ops.rope_kv_write_part(part, bias, B, T, Hq, Hkv, cos,
                                                 sin, pos, kp1, vp1, pt, start)
                assert ctx.dtype == torch.int32 and torch.equal(ctx, start + T)
                assert tuple(q1.shape) == (B, T, N) and q1.dtype == BF
                assert_same(q1[..., : Hq * D], q0[..., : Hq * D], "q " + what)
                assert_same(kp1, kp0, "k_pages " + what)
                assert_same(vp1, vp0, "v_pages " + what)
                # exactly the B*T written slots lost the sentinel
                written = torch.zeros(npages, P, dtype=torch.bool)
                for b in range(B):
                    for t in range(T):
                        a = sp + t
                        written[int(perm[b * maxp + a // P]), a % P] = True
                wk = written.to(DEV)[:, None, :, None].expand_as(kp1)
                wv = written.to(DEV)[:, None, None, :].expand_as(vp1)
                assert bool((kp1[~wk] == SENTINEL).all()), "k_pages outside " + what
                assert bool((vp1[~wv] == SENTINEL).all()), "v_pages outside " + what
                assert bool((kp1[wk] != SENTINEL).all())
                assert bool((vp1[wv] != SENTINEL).all())


def test_defer_combine_without_split_returns_bf16():
    """K = 256 cannot split: defer_combine has nothing to defer and the
    finished bf16 C (bias applied) comes back."""
    gen = torch.Generator().manual_seed(3)
    x, w = _randn_bf(gen, 5, 256).to(DEV), _randn_bf(gen, 512, 256, scale=1 / 16).to(DEV)
    b = _randn_bf(gen, 512).to(DEV)
    got = ops.linear(x, w, bias=b, defer_combine=True)
    assert got.dtype == BF
    assert_same(got, ops.linear(x, w, bias=b), "defer_combine, ksplit 1")


# ---------------------------------------------------------------------------
# 3. in-launch split-K reduce
# ---------------------------------------------------------------------------

def _two_launch(a, w, res, bias, ks, ss):
    return ops.hip_ops.gemm_skinny(a, w, res, bias, ks, None, 0.0, None, ss, 0)


def _in_launch(a, w, res, bias, ks, ss, cnt):
    return ops.hip_ops.gemm_skinny(a, w, res, bias, ks, None, 0.0, None, ss, 0,
                                   False, cnt)


@pytest.mark.parametrize("K,ks", fc.REDUCE_KS)
@pytest.mark.parametrize("N", fc.REDUCE_N)
def test_inlaunch_reduce(N, K, ks):
    c = fc.build_reduce(N, K, ks)
    w, bias32, res32 = dev(c.W), dev(c.bias), dev(c.res)
    gen = torch.Generator().manual_seed(N + K)
    wr = _randn_bf(gen, N, K, scale=K ** -0.5).to(DEV)
    ar32, rr32 = _randn_bf(gen, 32, K), _randn_bf(gen, 32, N).to(DEV)
    cnt = torch.zeros(N // 64, dtype=torch.int32, device=DEV)
    for M in fc.REDUCE_M:
        a = dev(fc.poisoned(c.Abuf[:M]))[:M]
        ar = fc.poisoned(ar32[:M]).to(DEV)[:M]
        for epi in (True, False):
            what = f"n{N}-k{K}-ks{ks}-m{M}-epi{int(epi)}"
            bias = bias32 if epi else None
            res = res32[:M].contiguous() if epi else None
            ss = torch.full((N // 64 * 32,), float("nan"), device=DEV) if epi else None
            got = _in_launch(a, w, res, bias, ks, ss, cnt)
            assert tuple(got.shape) == (M, N) and got.dtype == BF
            want = (c.want if epi else c.want_plain)[:M]
            assert torch.equal(got.cpu().double(), want), what + " against fp64"
            if epi:
                assert torch.equal(ss.view(-1, 32)[:, :M].cpu(),
                                   c.want_ss[:, :M].float()), what + " ss_out"
            assert not bool(cnt.any()), what + ": counters not back at zero"
            # realistic data against the two-launch path, ss_out included
            res = rr32[:M].contiguous() if epi else None
            ss0 = torch.full_like(ss, float("nan")) if epi else None
            ss1 = torch.full_like(ss, float("nan")) if epi else None
            ref = _two_launch(ar, wr, res, bias, ks, ss0)
            got = _in_launch(ar, wr, res, bias, ks, ss1, cnt)
            assert_same(got, ref, what + " randn")
            if epi:
                assert_same(ss1.view(-1, 32)[:, :M], ss0.view(-1, 32)[:, :M],
                            what + " randn ss_out")


def test_inlaunch_reduce_back_to_back():
    """64 calls on one stream, a fresh A each, the same counters and (through
    the caching allocator) the same slab workspace: every reducer meets lines
    its CU may still hold from the call before, and every call needs the
    counters the one before it reset."""
    N, K, ks, M, calls = 4096, 4096, 8, 32, 64
    gen = torch.Generator().manual_seed(64)
    w = _randn_bf(gen, N, K, scale=K ** -0.5).to(DEV)
    a = _randn_bf(gen, calls, M, K).to(DEV)
    res, bias = _randn_bf(gen, M, N).to(DEV), _randn_bf(gen, N).to(DEV)
    cnt = torch.zeros(N // 64, dtype=torch.int32, device=DEV)
    ss_ref = torch.empty(calls, N // 64 * 32, device=DEV)
    ss_got = torch.empty(calls, N // 64 * 32, device=DEV)
    ref = [_two_launch(a[i], w, res, bias, ks, ss_ref[i]) for i in range(calls)]
    torch.cuda.synchronize()
    got = [_in_launch(a[i], w, res, bias, ks, ss_got[i], cnt) for i in range(calls)]
    torch.cuda.synchronize()
    for i in range(calls):
        assert_same(got[i], ref[i], f"call {i}")
    assert_same(ss_got, ss_ref, "ss_out")
    assert not bool(cnt.any())


def test_inlaunch_reduce_graph_replay():
    """One call captured in a graph, replayed 8 times with A updated in
    place: each replay starts from the counters the previous one left."""
    N, K, ks, M = 4096, 4096, 8, 17
    gen = torch.Generator().manual_seed(8)
    w = _randn_bf(gen, N, K, scale=K ** -0.5).to(DEV)
    a_all = _randn_bf(gen, 8, M, K).to(DEV)
    res = _randn_bf(gen, M, N).to(DEV)
    cnt = torch.zeros(N // 64, dtype=torch.int32, device=DEV)
    ss = torch.empty(N // 64 * 32, device=DEV)
    a = a_all[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _in_launch(a, w, res, None, ks, ss, cnt)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _in_launch(a, w, res, None, ks, ss, cnt)
    for i in range(8):
        a.copy_(a_all[i])
        g.replay()
        ss0 = torch.empty_like(ss)
        ref = _two_launch(a_all[i], w, res, None, ks, ss0)
        assert_same(out, ref, f"replay {i}")
        assert_same(ss.view(-1, 32)[:, :M], ss0.view(-1, 32)[:, :M], f"replay {i} ss")
    assert not bool(cnt.any())


# ---------------------------------------------------------------------------
# 4. block level: all switches on vs all off
# ---------------------------------------------------------------------------

def _run_stack(cfg, B, x_pre, x_dec, on, monkeypatch, block_cls=None):
    from bloombee_amd.kv import PagedKVCache
    from bloombee_amd.models.llama.block import LlamaBlock, RopeTables

    block_cls = block_cls or LlamaBlock

    monkeypatch.setattr(iface, "_FUSE_SWIGLU", on)
    monkeypatch.setattr(iface, "_FUSE_QKV_ROPE", on)
    monkeypatch.setattr(iface, "_INLAUNCH_COMBINE",
                        frozenset(("o", "down")) if on else frozenset())
    rope = RopeTables(cfg)
    blocks = [block_cls(cfg, i, rope).init_random(40 + i).to(DEV) for i in range(2)]
    gen = torch.Generator().manual_seed(77)
    for blk in blocks:      # qwen3: non-unit per-head norm weights
        for name in ("q_norm_w", "k_norm_w"):
            if hasattr(blk, name):
                w = getattr(blk, name)
                w.data.copy_((1 + 0.3 * torch.randn(w.shape, generator=gen)).to(BF))
    object.__setattr__(blocks[1], "prev_block", blocks[0])
    pool = PagedKVCache(2, cfg.num_key_value_heads, cfg.head_dim, max_tokens=4096,
                        device=DEV, dtype=BF)
    kv = pool.allocate(B, 64)
    outs = []
    pos = 0
    for x in [x_pre] + list(x_dec):
        T = x.shape[1]
        kv.extend(T)
        start = torch.full((B,), pos, dtype=torch.int32, device=DEV)
        h = x
        for blk in blocks:
            h = blk.forward_inference(h, kv, start)
        outs.append(h)
        pos += T
    pages = [(pool.k_pages(i).clone(), pool.v_pages(i).clone()) for i in range(2)]
    kv.close()
    return outs, pages


def _stack_cfg(shape):
    from bloombee_amd.models.base import ModelConfig

    if shape == "h256":
        return ModelConfig(hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                           num_key_value_heads=2, head_dim=64, intermediate_size=512,
                           max_position_embeddings=128)
    return ModelConfig(hidden_size=1024, num_hidden_layers=2, num_attention_heads=8,
                       num_key_value_heads=2, head_dim=128, intermediate_size=1024,
                       max_position_embeddings=128)


def _check_on_vs_off(shape, B, monkeypatch, block_cls=None):
    cfg = _stack_cfg(shape)
    gen = torch.Generator().manual_seed(B)
    x_pre = _randn_bf(gen, B, 5, cfg.hidden_size).to(DEV)
    x_dec = [_randn_bf(gen, B, 1, cfg.hidden_size).to(DEV) for _ in range(3)]
    off, pages_off = _run_stack(cfg, B, x_pre, x_dec, False, monkeypatch, block_cls)
    on, pages_on = _run_stack(cfg, B, x_pre, x_dec, True, monkeypatch, block_cls)
    for i, (a, b) in enumerate(zip(on, off)):
        assert_same(a, b, f"step {i} output")
    for i, ((k1, v1), (k0, v0)) in enumerate(zip(pages_on, pages_off)):
        assert_same(k1, k0, f"layer {i} k_pages")
        assert_same(v1, v0, f"layer {i} v_pages")


@pytest.mark.parametrize("B", [1, 17, 32])
@pytest.mark.parametrize("shape", ["h256", "h1024-splitk"])
def test_block_switches_on_vs_off(shape, B, monkeypatch):
    """Two chained llama blocks, a short prefill then three decode steps.
    h256 is the smallest block the fused-norm gate admits (no GEMM splits K,
    so only the SwiGLU epilogue is live); h1024 makes qkv, o and down split
    K = 1024 in two, which brings in the deferred and the in-launch combine.
    There the plain gate_up GEMM splits K as well, so linear_swiglu keeps
    the separate kernels (fuse_swiglu_ok: a never-splitting fused kernel
    would order the sums differently)."""
    _check_on_vs_off(shape, B, monkeypatch)


@pytest.mark.parametrize("B", [1, 32])
@pytest.mark.parametrize("shape", ["h256", "h1024-splitk"])
def test_qwen3_block_switches_on_vs_off(shape, B, monkeypatch):
    """The same for two chained Qwen3 blocks with random non-unit q_norm_w /
    k_norm_w. Qwen3 is the LLaMA block plus the _post_qkv hook, so it takes
    the SwiGLU epilogue and the in-launch o / down combine; the hook needs
    combined QKV values, so the deferred qkv combine stays off for it."""
    from bloombee_amd.models.qwen3.block import Qwen3Block

    _check_on_vs_off(shape, B, monkeypatch, Qwen3Block)
