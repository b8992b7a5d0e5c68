"""The W ring of gemm_skinny_v2 (the `wring` argument of gemm_skinny and
gemm_skinny_swiglu; BBAMD_GEMM_WRING pins the same thing for a process), at
every depth the build instantiates.

(a) Exact-arithmetic cases (tests/wring_cases.py) against the fp64 model of
    gemm_cases with `torch.equal`: 1, 2, 3, 4, 5, 7 and 9 stages per split
    and uneven splits, so the loop, each peeled tail and a stream shorter
    than the ring are all reached; test_gemm_wring_cases_cpu.py shows that a
    lost set, stage, split, row or stripe moves the expected tensor.
(b) randn inputs: the ring against depth 2 (the kernel before the ring) with
    `torch.equal` on the output, the uncombined slabs, `ss_out`, the SwiGLU
    kernel and the in-launch combine, at the flagship's stage counts per
    split (2, 7 and 16). Integer data cannot see a reordered f32 sum; this
    can: every depth must accumulate k ascending in steps of 32.
"""
import os

import pytest
import torch

import gemm_cases as gc
import wring_cases as wc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bloombee_amd import ops

    assert ops.HAVE_HIP_OPS, (
        "HIP extension must be built and loadable on a GPU box (fail-loud policy)"
    )

DEV = "cuda:0"
BF = torch.bfloat16
RING = [d for d in wc.DEPTHS if d > 2]


def dev(t, dtype=BF):
    return None if t is None else t.to(dtype).to(DEV)


def assert_exact(got, want, what):
    got = got.detach().cpu().double().reshape(want.shape)
    if torch.equal(got, want):
        return
    err = (got - want).abs()
    err[got.isnan()] = float("inf")
    flat = int(err.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), want.shape))
    raise AssertionError(
        f"{what}: {int((err > 0).sum())} of {want.numel()} elements differ; "
        f"worst at {idx}: got {float(got[idx])}, want {float(want[idx])}")


def test_depths_match_the_build():
    assert list(ops.hip_ops.gemm_skinny_wring_plan(64, 256)[1]) == list(wc.DEPTHS)

    def plan(*args):
        return ops.hip_ops.gemm_skinny_wring_plan(*args)[0]

    # unpinned, every shape keeps depth 2 (the ring won for none when traced)
    if not os.environ.get("BBAMD_GEMM_WRING"):
        assert plan(28672, 4096, 1) == 2 and plan(4096, 14336) == 2
        assert plan(4096, 4096) == 2 and plan(6144, 4096) == 2
    assert plan(4096, 4096, 0, 2) == 2 and plan(4096, 4096, 0, 4) == 4
    assert plan(64, 160, 0, 4) == 0                # v1 kernel: no ring
    with pytest.raises(RuntimeError):
        plan(4096, 4096, 0, 3)


# ---------------------------------------------------------------------------
# (a) exact cases
# ---------------------------------------------------------------------------

def _operands(c):
    spec = c.spec
    a = dev(c.Abuf)[: spec.M]
    w, ss_in = dev(c.W), None
    if spec.kind == "norm":
        w = dev(c.Wfold)
        if c.ss_in is not None:
            ss_in = dev(c.ss_in, torch.float32).contiguous()
    return a, w, ss_in


@pytest.mark.parametrize("depth", wc.DEPTHS)
@pytest.mark.parametrize("spec", wc.SPECS, ids=gc.ids(wc.SPECS))
def test_wring_exact(spec, depth):
    c = gc.build(spec)
    a, w, ss_in = _operands(c)
    ss = None
    if spec.ss_out:
        ss = torch.full((spec.N // 64 * 32,), float("nan"), device=DEV)
    got = ops.hip_ops.gemm_skinny(a, w, dev(c.res), dev(c.bias), spec.ksplit, None,
                                  0.0, ss_in, ss, spec.mode, wring=depth)
    assert tuple(got.shape) == (spec.M, spec.N) and got.dtype == BF
    assert_exact(got, c.want, f"{spec.name} depth {depth}")
    if spec.ss_out:
        got_ss = ss.view(-1, 32)[:, : spec.M].cpu()
        assert torch.equal(got_ss, c.want_ss.float()), f"{spec.name}: ss_out differs"


@pytest.mark.parametrize("depth", wc.DEPTHS)
@pytest.mark.parametrize("spec", wc.DEFER_SPECS, ids=gc.ids(wc.DEFER_SPECS))
def test_wring_exact_deferred_slabs(spec, depth):
    c = gc.build(spec)
    a, w, _ = _operands(c)
    part = ops.hip_ops.gemm_skinny(a, w, None, None, spec.ksplit, None, 0.0, None,
                                   None, 0, True, None, depth)
    assert part.dtype == torch.float32
    assert tuple(part.shape) == (spec.ksplit, spec.M, spec.N)
    for s, want in enumerate(wc.slab_model(c)):
        assert_exact(part[s], want, f"{spec.name} depth {depth} slab {s}")


# ---------------------------------------------------------------------------
# (b) randn: ring against depth 2
# ---------------------------------------------------------------------------

def _randn_bf(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(BF)


M, N = 32, 128
FLAGSHIP = [(4096, 8), (14336, 8), (4096, 1)]      # 2, 7 and 16 stages per split


@pytest.fixture(scope="module")
def randn_inputs():
    out = {}
    for K, _ in FLAGSHIP:
        if K in out:
            continue
        gen = torch.Generator().manual_seed(300 + K)
        out[K] = dict(
            a=_randn_bf(gen, M, K).to(DEV),
            w=_randn_bf(gen, N, K, scale=K ** -0.5).to(DEV),
            res=_randn_bf(gen, M, N).to(DEV),
            bias=_randn_bf(gen, N).to(DEV))
        out[K]["ss_in"] = (out[K]["a"].float() ** 2).view(M, 4, K // 4).sum(-1).T.contiguous()
    return out


def _same(got, want, what):
    assert torch.equal(got, want), (
        f"{what}: {int((got != want).sum())} of {want.numel()} elements differ from depth 2")


@pytest.mark.parametrize("depth", RING)
@pytest.mark.parametrize("K,ks", FLAGSHIP)
def test_wring_randn_matches_depth2(randn_inputs, K, ks, depth):
    t = randn_inputs[K]
    a, w, res, bias = t["a"], t["w"], t["res"], t["bias"]
    g = ops.hip_ops.gemm_skinny
    assert ops.hip_ops.gemm_skinny_plan(N, K, ks)[0] == ks

    def run(d, mode, ss_in):
        ss = torch.full((N // 64 * 32,), float("nan"), device=DEV)
        c = g(a, w, res, bias, ks, None, 1e-5, ss_in, ss, mode, wring=d)
        return c, ss

    for mode, ss_in in ((0, None), (2, t["ss_in"]), (2, None)):
        what = f"K={K} ks={ks} mode={mode} ss_in={ss_in is not None} depth {depth}"
        c2, ss2 = run(2, mode, ss_in)
        cd, ssd = run(depth, mode, ss_in)
        _same(cd, c2, "output " + what)
        _same(ssd, ss2, "ss_out " + what)
    if ks > 1:
        p2 = g(a, w, None, None, ks, None, 0.0, None, None, 0, True, None, 2)
        pd = g(a, w, None, None, ks, None, 0.0, None, None, 0, True, None, depth)
        assert p2.dtype == torch.float32 and tuple(p2.shape) == (ks, M, N)
        _same(pd, p2, f"slabs K={K} ks={ks} depth {depth}")
        # the combine inside the launch (last-arriver reduction)
        cnt = torch.zeros(N // 64, dtype=torch.int32, device=DEV)
        ss2 = torch.full((N // 64 * 32,), float("nan"), device=DEV)
        ssd = ss2.clone()
        c2 = g(a, w, res, bias, ks, None, 0.0, None, ss2, 0, False, cnt, 2)
        cd = g(a, w, res, bias, ks, None, 0.0, None, ssd, 0, False, cnt, depth)
        _same(cd, c2, f"in-launch combine K={K} ks={ks} depth {depth}")
        _same(ssd, ss2, f"in-launch ss_out K={K} ks={ks} depth {depth}")
        assert not bool(cnt.any())


@pytest.mark.parametrize("depth", RING)
@pytest.mark.parametrize("K", [4096, 768])
def test_wring_swiglu_matches_depth2(randn_inputs, K, depth):
    """gemm_skinny_swiglu never splits K: 16 stages at the flagship's K, and 3
    (one period and a partial one) at K = 768."""
    gen = torch.Generator().manual_seed(400 + K)
    a = _randn_bf(gen, M, K).to(DEV)
    w = _randn_bf(gen, N, K, scale=K ** -0.5).to(DEV)          # I = 64
    ss_in = (a.float() ** 2).view(M, 4, K // 4).sum(-1).T.contiguous()
    f = ops.hip_ops.gemm_skinny_swiglu
    for mode, ss in ((0, None), (2, ss_in)):
        want = f(a, w, 1e-5, ss, mode, 2)
        got = f(a, w, 1e-5, ss, mode, depth)
        assert tuple(got.shape) == (M, N // 2)
        _same(got, want, f"swiglu K={K} mode={mode} depth {depth}")
    # and depth 2 is still the unfused pair
    gu = ops.hip_ops.gemm_skinny(a, w, None, None, 1, None, 0.0, None, None, 0, wring=2)
    _same(f(a, w, 0.0, None, 0, depth), ops.hip_ops.swiglu(gu),
          f"swiglu K={K} against gemm + swiglu")


def test_mode1_keeps_depth2():
    """norm mode 1 (weight staged with A) is not built for the ring: a pinned
    depth is ignored there and the result is the depth-2 kernel's."""
    gen = torch.Generator().manual_seed(500)
    K = 1280
    a, w = _randn_bf(gen, 17, K).to(DEV), _randn_bf(gen, 576, K, scale=K ** -0.5).to(DEV)
    nw = _randn_bf(gen, K).to(DEV)
    g = ops.hip_ops.gemm_skinny
    want = g(a, w, None, None, 1, nw, 1e-5, wring=2)
    for d in RING:
        _same(g(a, w, None, None, 1, nw, 1e-5, wring=d), want, f"mode 1 depth {d}")
