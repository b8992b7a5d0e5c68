"""Nontemporal W loads of the skinny decode GEMM on the GPU, and the split-K
combine kernel at the grids where the GEMM's XCD remap moves tiles.

NT. gemm_skinny_v2_kernel<.., NT> and the ring kernel differ from their plain
forms in the cache policy bit of the W loads only: the same bytes reach the
same registers, so every comparison of nt (w_nt=1) against plain (w_nt=-1) is
`torch.equal`, on randn data (integer data cannot see a reordered f32 sum).
One exact-arithmetic case per path (tests/gemm_cases.py) is held against its
fp64 expectation under nt as well, so a load that is wrong in BOTH flavours
cannot pass.

Shapes (N, K), each at M in {1, 16, 17, 32} (one m-tile, a full one, two),
those of test_gpu_packed_w.py:
  (64, 256)    one tile, one 256-k stage
  (128, 512)   two stages
  (192, 1024)  skinny_plan splits K in two
  (64, 2048)   own rule: four splits; pinned ksplit=1: one long stream

Combine. gemm_skinny_combine_ss_kernel indexes its stripe by blockIdx.x
while the GEMM that wrote the slabs remaps its tiles (xcd_remap); taking the
stripe through the same remap was tried and left out (profiles/
r09_nt_weights.md), so this pull request does not change the kernel. The cases
pin what any such change must keep: N = 64 (no remap), 512 (8 stripes), 576
(9, uneven), 1024 (two per XCD), K = 1024 split in two, against the fp64 model
(exact data: a stripe combined twice or not at all is off by whole units, and
its row sum-of-squares with it) and against the deferred slabs folded in
torch in split order.
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
NT, PLAIN = 1, -1


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


def _ss_in(a, M, K):
    ss = torch.ones(4, 32, device=DEV)
    ss[:, :M] = (a.float() ** 2).view(M, 4, K // 4).sum(-1).T
    return ss


def test_plan_follows_the_request():
    plan = ops.hip_ops.gemm_skinny_nt_plan
    for packed in (False, True):
        assert plan(64, 256, packed, NT)[0] is True
        assert plan(64, 256, packed, PLAIN)[0] is False
    assert plan(64, 160, False, NT)[0] is False        # v1 kernel: no nt flavour
    with pytest.raises(RuntimeError, match="w_nt"):
        ops.hip_ops.gemm_skinny(torch.zeros(1, 256, dtype=BF, device=DEV),
                                torch.zeros(64, 256, dtype=BF, device=DEV),
                                w_nt=2)


@pytest.mark.parametrize("packed", [False, True], ids=["row-major", "packed"])
@pytest.mark.parametrize("ksplit", [0, 1], ids=["own-rule", "unsplit"])
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", MS)
def test_nt_equals_plain(M, N, K, ksplit, packed):
    gen = torch.Generator().manual_seed(M * 1000 + N + K + ksplit)
    a = _randn_bf(gen, M + 3, K).to(DEV)[:M]
    w = _randn_bf(gen, N, K, scale=K ** -0.5).to(DEV)
    wp = ops.pack_skinny_w(w) if packed else None
    res = _randn_bf(gen, M, N).to(DEV)
    bias = _randn_bf(gen, N).to(DEV)
    ss_in = _ss_in(a, M, K)
    splits = ops.hip_ops.gemm_skinny_plan(N, K, ksplit)[0]
    if (N, K) == (192, 1024) and ksplit == 0:
        assert splits == 2
    if ksplit == 1:
        assert splits == 1

    def run(nt, residual=None, b=None, ss_out=False, norm=False, defer=False):
        ss = torch.full((N // 64 * 32,), float("nan"), device=DEV) if ss_out else None
        y = ops.hip_ops.gemm_skinny(a, w, residual, b, ksplit, None,
                                    EPS if norm else 0.0, ss_in if norm else None,
                                    ss, 2 if norm else 0, defer, None, 0, wp, nt)
        return y, (ss.view(-1, 32)[:, :M].clone() if ss_out else None)

    variants = {
        "plain": {},
        "bias": dict(b=bias),
        "residual+ss_out": dict(residual=res, ss_out=True),
        "residual+bias+ss_out": dict(residual=res, b=bias, ss_out=True),
        "norm+ss_in": dict(norm=True),
        "norm+ss_in+residual+ss_out": dict(norm=True, residual=res, ss_out=True),
        "defer_combine": dict(defer=True),
    }
    for name, kw in variants.items():
        got, ss_got = run(NT, **kw)
        want, ss_want = run(PLAIN, **kw)
        if name == "defer_combine":
            assert got.dtype == (torch.float32 if splits > 1 else BF)
        assert_same(got, want, f"{name} M={M} N={N} K={K}")
        if ss_got is not None:
            assert_same(ss_got, ss_want, f"{name} ss_out")


def test_nt_through_ops_linear():
    """ops.linear and ops.linear_swiglu pass w_nt on (3-D input, norm, ss_out,
    packed); a prefill-shaped call ignores it."""
    gen = torch.Generator().manual_seed(3)
    N, K = 192, 1024
    x = _randn_bf(gen, 17, 1, K).to(DEV)
    w = _randn_bf(gen, N, K, scale=K ** -0.5).to(DEV)
    wp = ops.pack_skinny_w(w)
    res = _randn_bf(gen, 17, 1, N).to(DEV)
    ss0 = torch.empty(N // 64 * 32, device=DEV)
    ss1 = torch.empty_like(ss0)
    got = ops.linear(x, w, residual=res, norm=(None, EPS), ss_out=ss1, w_packed=wp,
                     w_nt=NT)
    want = ops.linear(x, w, residual=res, norm=(None, EPS), ss_out=ss0, w_packed=wp,
                      w_nt=PLAIN)
    assert_same(got, want, "ops.linear")
    assert_same(ss1.view(-1, 32)[:, :17], ss0.view(-1, 32)[:, :17], "ss_out")
    xl = _randn_bf(gen, 33, K).to(DEV)
    assert_same(ops.linear(xl, w, w_nt=NT), ops.linear(xl, w), "M=33")
    for rows in (x, xl):      # checked on the paths that ignore it too
        with pytest.raises(RuntimeError, match="w_nt"):
            ops.linear(rows, w, w_nt=3)
    gu = _randn_bf(gen, 512, K, scale=K ** -0.5).to(DEV)
    # K = 1024 at 2I = 512 would split: the unfused pair, which takes w_nt too
    assert not ops.fuse_swiglu_ok(x, gu)
    assert_same(ops.linear_swiglu(x, gu, w_nt=NT), ops.linear_swiglu(x, gu, w_nt=PLAIN),
                "ops.linear_swiglu, unfused")


NT_EXACT = [
    gc.Spec("nt-m17-n192-k1024-ks0", "dense", 17, 192, 1024, 0, bias=True, res=True,
            seed=601),
    gc.Spec("nt-m32-n64-k2048-unsplit", "dense", 32, 64, 2048, 1, bias=True, res=True,
            seed=602),
    gc.Spec("nt-norm2-m32-n128-k512", "norm", 32, 128, 512, 0, mode=2, ss_in=4, res=True,
            ss_out=True, seed=603),
]


@pytest.mark.parametrize("how", ["row-major", "packed", "ring"])
@pytest.mark.parametrize("spec", NT_EXACT, ids=gc.ids(NT_EXACT))
def test_nt_exact(spec, how):
    """Small-integer data whose f32 sums are exact in any order, against the
    fp64 model, with nt loads on each path that has them."""
    c = gc.build(spec)
    M, N = spec.M, spec.N
    a = dev(c.Abuf)[:M]
    w = dev(c.Wfold if spec.kind == "norm" else c.W)
    ss_in = (dev(c.ss_in, torch.float32).contiguous()
             if spec.kind == "norm" else None)
    ss = torch.full((N // 64 * 32,), float("nan"), device=DEV) if spec.ss_out else None
    got = ops.hip_ops.gemm_skinny(a, w, dev(c.res), dev(c.bias), spec.ksplit, None,
                                  0.0, ss_in, ss, spec.mode, False, None,
                                  4 if how == "ring" else 2,
                                  ops.pack_skinny_w(w) if how == "packed" else None, NT)
    assert got.dtype == BF and tuple(got.shape) == (M, N)
    bad = got.cpu().double() != c.want
    assert not bool(bad.any()), (
        f"{spec.name}: {int(bad.sum())} of {bad.numel()} outputs differ from fp64")
    if spec.ss_out:
        assert torch.equal(ss.view(-1, 32)[:, :M].cpu(), c.want_ss.float())


@pytest.mark.parametrize("packed", [False, True], ids=["row-major", "packed"])
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("I,K", [(256, 256), (512, 512)])
@pytest.mark.parametrize("M", MS)
def test_nt_swiglu(M, I, K, mode, packed):
    gen = torch.Generator().manual_seed(M + I + K + mode)
    a = _randn_bf(gen, M + 3, K).to(DEV)[:M]
    w = _randn_bf(gen, 2 * I, K, scale=K ** -0.5).to(DEV)
    wp = ops.pack_skinny_w(w, swiglu=True) if packed else None
    ss_in = _ss_in(a, M, K) if mode == 2 else None
    eps = EPS if mode == 2 else 0.0
    f = ops.hip_ops.gemm_skinny_swiglu
    want = f(a, w, eps, ss_in, mode, 0, wp, PLAIN)
    assert_same(f(a, w, eps, ss_in, mode, 0, wp, NT), want, "gemm_skinny_swiglu")
    assert ops.fuse_swiglu_ok(a, w)
    norm = (None, eps) if mode == 2 else None
    assert_same(ops.linear_swiglu(a, w, norm=norm, ss_in=ss_in, w_packed=wp, w_nt=NT),
                want, "ops.linear_swiglu")
    # exact data against fp64 (fused_cases' bound for the f32 SwiGLU itself)
    c = fc.build_swiglu(fc.swiglu_spec(M, K, I, mode))
    a = dev(c.Abuf)[:M]
    w = dev(c.Wfold if mode == 2 else c.W)
    ss_in = dev(c.ss_in, torch.float32).contiguous() if mode == 2 else None
    got = f(a, w, 0.0, ss_in, mode, 0,
            ops.pack_skinny_w(w, swiglu=True) if packed else None, NT)
    ratio = float(((got.cpu().double() - c.want_act).abs() / fc.act_bound(c)).max())
    print(f"swiglu nt M={M} I={I} K={K} mode={mode}: |err| / bound vs fp64 {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("N,K", [(64, 1024), (128, 2048)])
@pytest.mark.parametrize("M", MS)
def test_nt_ring(M, N, K):
    """Depth-4 ring: split by the own rule (2 and 4 splits of one ring period
    each) and unsplit (two and four periods)."""
    gen = torch.Generator().manual_seed(700 + M + N + K)
    a = _randn_bf(gen, M + 3, K).to(DEV)[:M]
    w = _randn_bf(gen, N, K, scale=K ** -0.5).to(DEV)
    res = _randn_bf(gen, M, N).to(DEV)
    bias = _randn_bf(gen, N).to(DEV)
    ss_in = _ss_in(a, M, K)
    g = ops.hip_ops.gemm_skinny
    assert ops.hip_ops.gemm_skinny_wring_plan(N, K, 0, 4)[0] == 4

    def run(nt, ks, mode, defer=False):
        ss = None if defer else torch.full((N // 64 * 32,), float("nan"), device=DEV)
        y = g(a, w, None if defer else res, None if defer else bias, ks, None, EPS,
              ss_in if mode else None, ss, mode, defer, None, 4, None, nt)
        return y, (None if defer else ss.view(-1, 32)[:, :M].clone())

    for ks in (0, 1):
        for mode in (0, 2):
            y1, s1 = run(NT, ks, mode)
            y0, s0 = run(PLAIN, ks, mode)
            assert_same(y1, y0, f"ring M={M} N={N} K={K} ks={ks} mode={mode}")
            assert_same(s1, s0, "ring ss_out")
            # and the ring under nt is still the depth-2 plain kernel
            y2 = g(a, w, res, bias, ks, None, EPS, ss_in if mode else None, None, mode,
                   False, None, 2, None, PLAIN)
            assert_same(y1, y2, f"ring nt against depth 2 plain, ks={ks} mode={mode}")
    assert_same(run(NT, 0, 0, True)[0], run(PLAIN, 0, 0, True)[0], "ring slabs")
    # gemm_skinny_swiglu on the ring (I = N / 2)
    f = ops.hip_ops.gemm_skinny_swiglu
    assert_same(f(a, w, EPS, ss_in, 2, 4, None, NT), f(a, w, EPS, ss_in, 2, 4, None, PLAIN),
                "ring swiglu")


@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("M", MS)
def test_nt_inlaunch_combine(M, depth):
    """EPI 2: split-K with the combine inside the launch."""
    N, K, ks = 512, 1024, 2
    gen = torch.Generator().manual_seed(800 + M)
    a = _randn_bf(gen, M + 3, K).to(DEV)[:M]
    w = _randn_bf(gen, N, K, scale=K ** -0.5).to(DEV)
    res = _randn_bf(gen, M, N).to(DEV)
    bias = _randn_bf(gen, N).to(DEV)
    assert ops.hip_ops.gemm_skinny_plan(N, K, ks)[0] == ks
    cnt = torch.zeros(N // 64, dtype=torch.int32, device=DEV)
    g = ops.hip_ops.gemm_skinny

    def run(nt, c):
        ss = torch.full((N // 64 * 32,), float("nan"), device=DEV)
        y = g(a, w, res, bias, ks, None, 0.0, None, ss, 0, False, c, depth, None, nt)
        return y, ss.view(-1, 32)[:, :M].clone()

    y1, s1 = run(NT, cnt)
    y0, s0 = run(PLAIN, cnt)
    assert_same(y1, y0, f"in-launch combine M={M} depth {depth}")
    assert_same(s1, s0, "in-launch ss_out")
    assert not bool(cnt.any())
    # the same bits as the separate combine kernel
    y2, s2 = run(NT, None)
    assert_same(y1, y2, "in-launch against the combine kernel")
    assert_same(s1, s2, "ss_out against the combine kernel")


# ---------------------------------------------------------------------------
# block level
# ---------------------------------------------------------------------------

def _run_blocks(monkeypatch, nt, graph, x_pre, x_dec):
    """Two chained tiny LLaMA blocks: a prefill, then len(x_dec) decode steps
    (eager, or the first eager and the rest replays of one captured step).
    BBAMD_W_NT is read once per process, so the blocks' GEMMs are pinned
    through the per-call request instead."""
    from bloombee_amd.kv import PagedKVCache
    from bloombee_amd.models.base import ModelConfig
    from bloombee_amd.models.llama import block as lb

    monkeypatch.setenv("BBAMD_PACK_W", "1")
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

    seen = []
    real_linear, real_swiglu = lb.ops.linear, lb.ops.linear_swiglu

    def pin(real):
        def f(x, w, *a, **kw):
            assert "w_nt" not in kw
            seen.append(x.numel() // x.shape[-1])
            return real(x, w, *a, w_nt=nt, **kw)
        return f

    monkeypatch.setattr(lb.ops, "linear", pin(real_linear))
    monkeypatch.setattr(lb.ops, "linear_swiglu", pin(real_swiglu))

    def fwd(h, pos):
        for blk in blocks:
            h = blk.forward_inference(h, kv, pos)
        return h

    T = x_pre.shape[1]
    kv.extend(T)
    pos = torch.zeros(B, dtype=torch.int32, device=DEV)
    outs = [fwd(x_pre, pos)]
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
            assert seen == [B] * 8, seen     # 4 decode-shaped projections per block
        else:
            if g is None:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    out_buf = fwd(hbuf, pos)
            g.replay()
            outs.append(out_buf.clone())
        pos += 1
    torch.cuda.synchronize()
    kv.close()
    return outs


def test_block_nt_equals_plain(monkeypatch):
    B, H = 4, 256
    gen = torch.Generator().manual_seed(21)
    x_pre = _randn_bf(gen, B, 9, H).to(DEV)      # 36 rows: not decode-shaped
    x_dec = [_randn_bf(gen, B, 1, H).to(DEV) for _ in range(3)]
    runs = {}
    for nt in (PLAIN, NT):
        for graph in (False, True):
            with monkeypatch.context() as mp:     # each run pins the real ops
                runs[(nt, graph)] = _run_blocks(mp, nt, graph, x_pre, x_dec)
    base = runs[(PLAIN, False)]
    assert len(base) == 4      # prefill, 3 decode steps
    for key, outs in runs.items():
        for i, (a, b) in enumerate(zip(outs, base)):
            assert_same(a, b, f"w_nt={key[0]} graph={key[1]} output {i}")


# ---------------------------------------------------------------------------
# split-K combine kernel against the remapped GEMM's slabs
# ---------------------------------------------------------------------------

COMBINE_NK = ((64, 1024), (512, 1024), (576, 1024), (1024, 1024))
COMBINE = [gc.Spec(f"combine-m{M}-n{N}-k{K}-ks2", "dense", M, N, K, 2, bias=True, res=True,
                 ss_out=True, seed=900 + i)
         for i, (M, (N, K)) in enumerate((M, s) for s in COMBINE_NK for M in (1, 17, 32))]


@pytest.mark.parametrize("spec", COMBINE, ids=gc.ids(COMBINE))
def test_combine_ss_exact(spec):
    """residual + bias + ss_out through gemm_skinny_combine_ss_kernel against
    the fp64 model."""
    c = gc.build(spec)
    M, N = spec.M, spec.N
    assert ops.hip_ops.gemm_skinny_plan(N, spec.K, spec.ksplit)[0] == 2
    a, w = dev(c.Abuf)[:M], dev(c.W)
    ss = torch.full((N // 64 * 32,), float("nan"), device=DEV)
    got = ops.hip_ops.gemm_skinny(a, w, dev(c.res), dev(c.bias), spec.ksplit, None,
                                  0.0, None, ss)
    bad = got.cpu().double() != c.want
    assert not bool(bad.any()), (
        f"{spec.name}: {int(bad.sum())} of {bad.numel()} outputs differ from fp64, "
        f"in stripes {sorted(set((bad.nonzero()[:, 1] // 64).tolist()))}")
    assert torch.equal(ss.view(-1, 32)[:, :M].cpu(), c.want_ss.float())


@pytest.mark.parametrize("N,K", COMBINE_NK)
@pytest.mark.parametrize("M", (1, 17, 32))
def test_combine_ss_equals_folded_slabs(M, N, K):
    """randn: the combine kernel against the deferred slabs folded in torch
    in split order (f32 adds, then bias, then residual, one bf16 rounding),
    and the stripe sums of squares of the unrounded values."""
    gen = torch.Generator().manual_seed(950 + M + N)
    a = _randn_bf(gen, M + 3, K).to(DEV)[:M]
    w = _randn_bf(gen, N, K, scale=K ** -0.5).to(DEV)
    res = _randn_bf(gen, M, N).to(DEV)
    bias = _randn_bf(gen, N).to(DEV)
    g = ops.hip_ops.gemm_skinny
    slabs = g(a, w, None, None, 2, None, 0.0, None, None, 0, True)
    assert slabs.dtype == torch.float32 and tuple(slabs.shape) == (2, M, N)
    v = torch.zeros(M, N, device=DEV)
    for s in range(slabs.shape[0]):
        v = v + slabs[s]
    v = v + bias.float()[None, :]
    v = v + res.float()
    ss = torch.full((N // 64 * 32,), float("nan"), device=DEV)
    got = g(a, w, res, bias, 2, None, 0.0, None, ss)
    assert_same(got, v.to(BF), f"combine M={M} N={N}")
    # the kernel sums a stripe's 64 squares in another order than torch does:
    # 64 positive f32 terms, so within 64 * 2^-24 relative of each other
    want_ss = (v * v).view(M, N // 64, 64).double().sum(-1).T
    got_ss = ss.view(-1, 32)[:, :M].double()
    assert bool(((got_ss - want_ss).abs() <= 64 * 2.0 ** -24 * want_ss).all())
