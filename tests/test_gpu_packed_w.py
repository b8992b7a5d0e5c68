"""Packed decode-GEMM weights on the GPU: gemm_skinny_v2_kernel<.., PACKED>
against the row-major kernel, bit for bit.

The packed kernel hands every lane the very 8 elements the row-major address
gives it and changes nothing else, so per accumulator the MFMA operands and
their order are the same: every comparison is `torch.equal`, on realistic
randn data (integer data cannot see a reordered f32 sum). Exact-arithmetic
data (tests/gemm_cases.py, fused_cases.py) is held against its fp64
expectation too, so a wrong row map in BOTH pack and kernel cannot pass.

Shapes (N, K), each at M in {1, 16, 17, 32} (one m-tile, a full one, two):
  (64, 256)    one tile, one 256-k stage
  (128, 512)   two stages
  (192, 1024)  skinny_plan splits K in two
  (64, 2048)   own rule: four splits; pinned ksplit=1: one long stream
"""
import pytest
import torch

import fused_cases as fc
import gemm_cases as gc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bloombee_amd import ops

    assert ops.HAVE_HIP_OPS, (
        "HIP extension must be built and loadable on a GPU box (fail-loud policy)"
    )

DEV = "cuda:0"
BF = torch.bfloat16
MS = (1, 16, 17, 32)
SHAPES = ((64, 256), (128, 512), (192, 1024), (64, 2048))
EPS = 1e-5


def dev(t, dtype=BF):
    return None if t is None else t.to(dtype).to(DEV)


def _randn_bf(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(BF)


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if torch.equal(got, want):
        return
    g, w = got.detach().cpu().double(), want.detach().cpu().double()
    err = (g - w).abs()
    err[g.isnan() | w.isnan()] = float("inf")
    raise AssertionError(f"{what}: {int((err > 0).sum())} of {w.numel()} elements "
                         f"differ, worst {float(err.max())}")


@pytest.mark.parametrize("ksplit", [0, 1], ids=["own-rule", "unsplit"])
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", MS)
def test_packed_equals_row_major(M, N, K, ksplit):
    gen = torch.Generator().manual_seed(M * 1000 + N + K + ksplit)
    a = _randn_bf(gen, M + 3, K).to(DEV)[:M]
    w = _randn_bf(gen, N, K, scale=K ** -0.5).to(DEV)
    wp = ops.pack_skinny_w(w)
    res = _randn_bf(gen, M, N).to(DEV)
    bias = _randn_bf(gen, N).to(DEV)
    ss_in = torch.ones(4, 32, device=DEV)
    ss_in[:, :M] = (a.float() ** 2).view(M, 4, K // 4).sum(-1).T
    splits = ops.hip_ops.gemm_skinny_plan(N, K, ksplit)[0]
    if (N, K) == (192, 1024) and ksplit == 0:
        assert splits == 2
    if ksplit == 1:
        assert splits == 1

    def run(p, residual=None, b=None, ss_out=False, norm=False, defer=False):
        ss = torch.full((N // 64 * 32,), float("nan"), device=DEV) if ss_out else None
        y = ops.hip_ops.gemm_skinny(a, w, residual, b, ksplit, None,
                                    EPS if norm else 0.0, ss_in if norm else None,
                                    ss, 2 if norm else 0, defer, None, 0, p)
        return y, (ss.view(-1, 32)[:, :M].clone() if ss_out else None)

    variants = {
        "plain": {},
        "residual+bias+ss_out": dict(residual=res, b=bias, ss_out=True),
        "bias": dict(b=bias),
        "norm+ss_in": dict(norm=True),
        "norm+ss_in+residual+ss_out": dict(norm=True, residual=res, ss_out=True),
        "defer_combine": dict(defer=True),
    }
    for name, kw in variants.items():
        got, ss_got = run(wp, **kw)
        want, ss_want = run(None, **kw)
        if name == "defer_combine":
            assert got.dtype == (torch.float32 if splits > 1 else BF)
        assert_same(got, want, f"{name} M={M} N={N} K={K}")
        if ss_got is not None:
            assert_same(ss_got, ss_want, f"{name} ss_out")


def test_packed_through_ops_linear():
    """ops.linear passes w_packed on the skinny path (3-D input, norm,
    ss_out); a prefill-shaped call ignores it."""
    gen = torch.Generator().manual_seed(3)
    N, K = 192, 1024
    x = _randn_bf(gen, 17, 1, K).to(DEV)
    w = _randn_bf(gen, N, K, scale=K ** -0.5).to(DEV)
    wp = ops.pack_skinny_w(w)
    res = _randn_bf(gen, 17, 1, N).to(DEV)
    ss0 = torch.empty(N // 64 * 32, device=DEV)
    ss1 = torch.empty_like(ss0)
    got = ops.linear(x, w, residual=res, norm=(None, EPS), ss_out=ss1, w_packed=wp)
    want = ops.linear(x, w, residual=res, norm=(None, EPS), ss_out=ss0)
    assert_same(got, want, "ops.linear")
    assert_same(ss1.view(-1, 32)[:, :17], ss0.view(-1, 32)[:, :17], "ss_out")
    # a zeroed "packed" weight must change the skinny result (it IS read) ...
    zero = torch.zeros_like(wp)
    assert not torch.equal(ops.linear(x, w, w_packed=zero), ops.linear(x, w))
    # ... and not the hipBLASLt one (33 rows)
    xl = _randn_bf(gen, 33, K).to(DEV)
    assert_same(ops.linear(xl, w, w_packed=zero), ops.linear(xl, w), "M=33")
    with pytest.raises(RuntimeError, match="w_packed"):
        ops.linear(x, w, w_packed=wp.reshape(-1)[:-8])
    with pytest.raises(RuntimeError, match="w_packed"):
        ops.linear(x, w, w_packed=wp.float())


EXACT = [gc.Spec(f"packed-m{M}-n{N}-k{K}-ks{ks}", "dense", M, N, K, ks, bias=True,
                 res=True, seed=400 + i)
         for i, (M, (N, K), ks) in enumerate(
             (M, s, ks) for s in SHAPES for M in (1, 17, 32) for ks in (0, 1))]
EXACT += [gc.Spec(f"packed-norm2-m{M}-n{N}-k{K}", "norm", M, N, K, 0, mode=2, ss_in=4,
                  res=True, ss_out=True, seed=450 + i)
          for i, (M, (N, K)) in enumerate((M, s) for s in SHAPES[1:3] for M in (16, 32))]


@pytest.mark.parametrize("spec", EXACT, ids=gc.ids(EXACT))
def test_packed_exact(spec):
    """Small-integer data whose f32 sums are exact in any order, against the
    fp64 model: a dropped, duplicated or misplaced row or k-block is an error
    of at least one whole unit."""
    c = gc.build(spec)
    M, N = spec.M, spec.N
    a = dev(c.Abuf)[:M]
    w = dev(c.Wfold if spec.kind == "norm" else c.W)
    ss_in = (dev(c.ss_in, torch.float32).contiguous()
             if spec.kind == "norm" else None)
    ss = torch.full((N // 64 * 32,), float("nan"), device=DEV) if spec.ss_out else None
    got = ops.hip_ops.gemm_skinny(a, w, dev(c.res), dev(c.bias), spec.ksplit, None,
                                  0.0, ss_in, ss, spec.mode, False, None, 0,
                                  ops.pack_skinny_w(w))
    assert got.dtype == BF and tuple(got.shape) == (M, N)
    bad = got.cpu().double() != c.want
    assert not bool(bad.any()), (
        f"{spec.name}: {int(bad.sum())} of {bad.numel()} outputs differ from fp64")
    if spec.ss_out:
        assert torch.equal(ss.view(-1, 32)[:, :M].cpu(), c.want_ss.float())


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("I,K", [(256, 256), (512, 512)])
@pytest.mark.parametrize("M", MS)
def test_packed_swiglu(M, I, K, mode):
    # randn: fused packed vs fused row-major, through the binding and ops
    gen = torch.Generator().manual_seed(M + I + K + mode)
    a = _randn_bf(gen, M + 3, K).to(DEV)[:M]
    w = _randn_bf(gen, 2 * I, K, scale=K ** -0.5).to(DEV)
    wp = ops.pack_skinny_w(w, swiglu=True)
    ss_in = None
    if mode == 2:
        ss_in = torch.ones(4, 32, device=DEV)
        ss_in[:, :M] = (a.float() ** 2).view(M, 4, K // 4).sum(-1).T
    eps = EPS if mode == 2 else 0.0
    want = ops.hip_ops.gemm_skinny_swiglu(a, w, eps, ss_in, mode)
    got = ops.hip_ops.gemm_skinny_swiglu(a, w, eps, ss_in, mode, 0, wp)
    assert_same(got, want, "gemm_skinny_swiglu")
    assert ops.fuse_swiglu_ok(a, w)
    norm = (None, eps) if mode == 2 else None
    assert_same(ops.linear_swiglu(a, w, norm=norm, ss_in=ss_in, w_packed=wp), want,
                "ops.linear_swiglu")
    # the identity-map pack is NOT this kernel's layout: it must show
    assert not torch.equal(
        ops.hip_ops.gemm_skinny_swiglu(a, w, eps, ss_in, mode, 0,
                                       ops.pack_skinny_w(w)), want)
    # exact data against fp64 (fused_cases' bound for the f32 SwiGLU itself)
    c = fc.build_swiglu(fc.swiglu_spec(M, K, I, mode))
    a = dev(c.Abuf)[:M]
    w = dev(c.Wfold if mode == 2 else c.W)
    ss_in = dev(c.ss_in, torch.float32).contiguous() if mode == 2 else None
    got = ops.hip_ops.gemm_skinny_swiglu(a, w, 0.0, ss_in, mode, 0,
                                         ops.pack_skinny_w(w, swiglu=True))
    assert_same(got, ops.hip_ops.gemm_skinny_swiglu(a, w, 0.0, ss_in, mode),
                "exact data, row-major kernel")
    ratio = float(((got.cpu().double() - c.want_act).abs() / fc.act_bound(c)).max())
    print(f"swiglu M={M} I={I} K={K} mode={mode}: |err| / bound vs fp64 {ratio:.3f}")
    assert ratio <= 1.0


# ---------------------------------------------------------------------------
# block level
# ---------------------------------------------------------------------------

def _run_blocks(monkeypatch, pack, graph, x_pre, x_dec, x_after):
    """Two chained tiny LLaMA blocks: a prefill, len(x_dec) decode steps
    (eager, or the first eager and the rest replays of one captured step),
    then unfold_norm_weights and one more eager step."""
    from bloombee_amd.kv import PagedKVCache
    from bloombee_amd.models.base import ModelConfig
    from bloombee_amd.models.llama import block as lb

    monkeypatch.setenv("BBAMD_PACK_W", pack)
    cfg = ModelConfig(hidden_size=256, num_hidden_layers=2, num_attention_heads=2,
                      num_key_value_heads=1, head_dim=128, intermediate_size=256,
                      max_position_embeddings=128)
    rope = lb.RopeTables(cfg)
    blocks = [lb.LlamaBlock(cfg, i, rope).init_random(60 + i).to(DEV) for i in range(2)]
    gen = torch.Generator().manual_seed(9)
    for blk in blocks:      # non-unit norm weights: the fold matters
        for name in ("input_norm_w", "post_norm_w"):
            p = getattr(blk, name)
            p.data.copy_((1 + 0.3 * torch.randn(p.shape, generator=gen)).to(BF))
    object.__setattr__(blocks[1], "prev_block", blocks[0])
    B = x_pre.shape[0]
    pool = PagedKVCache(2, cfg.num_key_value_heads, cfg.head_dim, max_tokens=2048,
                        device=DEV, dtype=BF)
    kv = pool.allocate(B, 64)

    # what the blocks hand to ops: a packed copy is never stale
    seen = []
    real_linear, real_swiglu = lb.ops.linear, lb.ops.linear_swiglu

    def spy(real, swiglu):
        def f(x, w, *a, w_packed=None, **kw):
            if not torch.cuda.is_current_stream_capturing():
                seen.append(w_packed is not None)
                if w_packed is not None:
                    assert torch.equal(w_packed, ops.pack_skinny_w(w.detach(), swiglu))
            return real(x, w, *a, w_packed=w_packed, **kw)
        return f

    monkeypatch.setattr(lb.ops, "linear", spy(real_linear, False))
    monkeypatch.setattr(lb.ops, "linear_swiglu", spy(real_swiglu, True))

    def fwd(h, pos):
        for blk in blocks:
            h = blk.forward_inference(h, kv, pos)
        return h

    T = x_pre.shape[1]
    kv.extend(T)
    pos = torch.zeros(B, dtype=torch.int32, device=DEV)
    outs = [fwd(x_pre, pos)]
    assert not any(seen), "prefill-shaped GEMMs never take a packed weight"
    pos += T
    hbuf = torch.empty_like(x_dec[0])
    g = None
    for i, x in enumerate(x_dec):
        kv.extend(1)
        kv.page_table()
        hbuf.copy_(x)
        if not graph or i == 0:
            del seen[:]
            outs.append(fwd(hbuf, pos).clone())
            # 4 projections per block, each packed under "1", none under "0"
            assert seen == [pack == "1"] * 8, seen
        else:
            if g is None:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    out_buf = fwd(hbuf, pos)
            g.replay()
            outs.append(out_buf.clone())
        pos += 1
    for blk in blocks:
        blk.unfold_norm_weights()
        assert blk._wpacked == {}, "unfold must drop the packed copies"
    kv.extend(1)
    kv.page_table()
    del seen[:]
    outs.append(fwd(x_after, pos).clone())   # folds again; the spy checks freshness
    assert len(seen) == 8
    torch.cuda.synchronize()
    kv.close()
    return outs


def test_block_packed_equals_unpacked(monkeypatch):
    B, H = 4, 256
    gen = torch.Generator().manual_seed(21)
    x_pre = _randn_bf(gen, B, 9, H).to(DEV)      # 36 rows: not decode-shaped
    x_dec = [_randn_bf(gen, B, 1, H).to(DEV) for _ in range(3)]
    x_after = _randn_bf(gen, B, 1, H).to(DEV)
    runs = {(pack, graph): _run_blocks(monkeypatch, pack, graph, x_pre, x_dec, x_after)
            for pack in ("0", "1") for graph in (False, True)}
    base = runs[("0", False)]
    assert len(base) == 5      # prefill, 3 decode steps, the step after unfold
    for key, outs in runs.items():
        for i, (a, b) in enumerate(zip(outs, base)):
            assert_same(a, b, f"BBAMD_PACK_W={key[0]} graph={key[1]} output {i}")
