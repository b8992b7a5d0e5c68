"""Exact-arithmetic parity of the skinny, W4 and MoE GEMM kernels and the
split-K combine kernels (gemm_skinny.hip v1/v2, w4_gemm.hip, moe_gemm.hip)
against the fp64 CPU expectation of tests/gemm_cases.py.

Inputs are small integers (times powers of two) that cancel in random
pairs, so every f32 partial sum is exact in any order and the kernel output
must `torch.equal` the expected tensor. test_gemm_cases_cpu.py proves on
CPU that each plausible defect (a lost k-slice, split, row, stripe, expert,
quantisation group ...) changes at least one expected element by a whole
unit. On a mismatch the worst element and its (m, n) are printed.

Which case reaches which path (ids are `gemm_cases` spec names):
  XCD remap, gridDim.x % 8 != 0   v2-*-remap-r*, norm*-n576/n704/n960,
                                  w4-*-n576/n704, moe-*-n576
  MoE m-chunks beyond the first   every moe-* case (a group of 33..70 rows)
  fused norm mode 2               norm2-*
  ss_in with 1/8/9/36/64/100      norm*-ssin*
  v1 empty trailing splits        v1-m15-n256-k96-ks8-empty-splits
  v2 uneven splits (2+1 stages)   v2-m16-n704-k768-ks2-uneven-remap-r3
  W4 bias/residual under split-K  w4-m4-n704-k384-ks2, w4-m16-n576-k1024-ks3
  vectorised combine, no ss_out   v2-m17-n4096-k512-ks2-vector-combine
  M in {15, 16, 17, 31, 32}       names carry m<M>
  W4 GEMV NLOADS 1 / 2 / 7        w4-gemv-*
  W4 M == 1 MFMA form             w4-m1-k1024-mfma

The realistic-valued tests at the end complement the exact ones (exact data
cannot see lost accumulator precision); their bound is derived in the
gemm_cases docstring, where the worst observed ratios are recorded.
"""
import math

import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bloombee_amd import ops
    from bloombee_amd.ops import reference as ref

    assert ops.HAVE_HIP_OPS, (
        "HIP extension must be built and loadable on a GPU box (fail-loud policy)"
    )

DEV = "cuda:0"
BF = torch.bfloat16


def dev(t, dtype=BF):
    return None if t is None else t.to(dtype).to(DEV)


def assert_exact(got, want, what):
    """torch.equal against the fp64 expectation, with the worst element."""
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


def assert_one_rounding(got, want, what):
    """library / torch fallbacks: within one bf16 rounding of the exact value"""
    got = got.detach().cpu().double().reshape(want.shape)
    bad = (got - want).abs() > 2.0 ** -8 * want.abs()
    assert not bool(bad.any()), \
        f"{what}: {int(bad.sum())} elements off by more than 2^-8 |want|"


# ---------------------------------------------------------------------------
# runners
# ---------------------------------------------------------------------------

def a_view(c):
    """A as the [:M] view of the taller poisoned buffer."""
    spec = c.spec
    a = dev(c.Abuf)[: spec.M]
    assert a.is_contiguous()
    return a.view(spec.M, 1, spec.K) if spec.batch3 else a


def run_skinny(c, via_linear=False):
    spec = c.spec
    M, N = spec.M, spec.N
    a = a_view(c)
    res, bias = dev(c.res), dev(c.bias)
    if res is not None and spec.batch3:
        res = res.view(M, 1, N)
    nw, w, ss_in = None, dev(c.W), None
    if spec.kind == "norm":
        if spec.mode == 1:
            nw = dev(c.nw)
        else:
            w = dev(c.Wfold)
        if c.ss_in is not None:
            ss_in = dev(c.ss_in, torch.float32).contiguous()
    ss = None
    if spec.ss_out:
        ss = torch.full((N // 64 * 32,), float("nan"), device=DEV)
    if via_linear:
        assert spec.ksplit == 0
        norm = None if spec.kind != "norm" else (nw, 0.0)
        got = ops.linear(a, w, res, bias, norm=norm, ss_in=ss_in, ss_out=ss)
    else:
        got = ops.hip_ops.gemm_skinny(a, w, res, bias, spec.ksplit, nw, 0.0,
                                      ss_in, ss, spec.mode)
    return got, ss


def check_ss(c, ss):
    # rows >= M are unspecified: with MT == 1 the v2 kernel never writes
    # ssp[16..31], and combine_ss returns early for m >= M. Not asserted.
    M = c.spec.M
    got = ss.view(-1, 32)[:, :M].cpu()
    assert torch.equal(got, c.want_ss.float()), (
        f"{c.spec.name}: ss_out differs, worst "
        f"{float((got.double() - c.want_ss).abs().max())}")


def run_w4(c, via_linear=False):
    spec = c.spec
    M, N, K = spec.M, spec.N, spec.K
    res, bias = dev(c.res), dev(c.bias)
    packed = c.packed.to(DEV)
    scale = dev(c.scale, torch.float16)
    zero = dev(c.zero, torch.float16)
    if via_linear:
        return ops.linear_w4(dev(c.Abuf)[:M], packed.reshape(N, K // 64, 32),
                             scale, zero, N, residual=res, bias=bias)
    a = dev(c.Abuf, torch.float16)[:M]
    return ops.hip_ops.gemm_w4(a, packed, scale, zero, res, bias, N, spec.ksplit)


def run_moe(c, via_iface=False, mchunks=None):
    A, W = dev(c.A), dev(c.W)
    off = c.off.to(DEV)
    rm = c.rowmap.to(DEV) if c.rowmap is not None else None
    sc = dev(c.scale, torch.float32)
    mchunks = mchunks or c.mchunks
    if via_iface:
        return ops.moe_gemm_grouped(A, W, off, rm, sc, S=c.S, mchunks=mchunks)
    return ops.hip_ops.moe_gemm(A, W, off, rm, sc, c.S, mchunks)


# ---------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------

_SKINNY = gc.SKINNY_V1 + gc.SKINNY_V2 + gc.NORM


@pytest.mark.parametrize("spec", _SKINNY, ids=gc.ids(_SKINNY))
def test_gemm_skinny_exact(spec):
    c = gc.build(spec)
    got, ss = run_skinny(c, via_linear=(spec.ksplit == 0))
    want_shape = (spec.M, 1, spec.N) if spec.batch3 else (spec.M, spec.N)
    assert tuple(got.shape) == want_shape and got.dtype == BF
    assert_exact(got, c.want, spec.name)
    if spec.ss_out:
        check_ss(c, ss)


def test_gemm_skinny_chain_exact():
    """Producer with ss_out (in-kernel epilogue and split-K combine), then a
    mode-2 consumer fed the producer's ss as ss_in plus a residual: the
    llama block's o_proj -> gate_up pattern."""
    c = gc.build_chain()
    M = c.M
    a1 = dev(c.A1buf)[:M]
    w1, r1, w2, r2 = dev(c.W1), dev(c.R1), dev(c.W2), dev(c.R2)
    for ks in (1, 2):
        ss = torch.full((c.W1.shape[0] // 64 * 32,), float("nan"), device=DEV)
        h = ops.hip_ops.gemm_skinny(a1, w1, r1, None, ks, None, 0.0, None, ss, 0)
        assert_exact(h, c.h, f"chain producer ks={ks}")
        assert torch.equal(ss.view(-1, 32)[:, :M].cpu(), c.ss.float())
        # rows >= M of ss are unspecified (see check_ss); the consumer only
        # uses invr of rows < M, so give it finite values there
        ss.view(-1, 32)[:, M:] = 1.0
        y = ops.hip_ops.gemm_skinny(h, w2, r2, None, 0, None, 0.0, ss, None, 2)
        assert_exact(y, c.want, f"chain consumer ks={ks}")


@pytest.mark.parametrize("spec", gc.W4, ids=gc.ids(gc.W4))
def test_gemm_w4_exact(spec):
    c = gc.build(spec)
    got = run_w4(c, via_linear=(spec.ksplit == 0))
    assert tuple(got.shape) == (spec.M, spec.N) and got.dtype == BF
    assert_exact(got, c.want, spec.name)


@pytest.mark.parametrize("spec", gc.MOE, ids=gc.ids(gc.MOE))
def test_moe_gemm_exact(spec):
    c = gc.build(spec)
    got = run_moe(c, via_iface=(spec.extra_chunks == 0))
    assert tuple(got.shape) == (c.S, spec.N)
    assert_exact(got, c.want, spec.name)


# ---------------------------------------------------------------------------
# dispatch edges: the same exact data on both sides of each gate in
# interface.py. Kernel side: equality. Library / torch side: one rounding.
# ---------------------------------------------------------------------------

def _spec(name):
    return next(s for s in gc.ALL_CASES if s.name == name)


def test_linear_gate_m32_m33():
    c = gc.build(_spec("v2-m32-n576-k1280-ks2-remap-r1"))
    a, w, res, bias = dev(c.Abuf)[:32], dev(c.W), dev(c.res), dev(c.bias)
    assert_exact(ops.linear(a, w, res, bias), c.want, "linear M=32 (kernel)")
    a33 = torch.cat([a, a[:1]]).contiguous()
    r33 = torch.cat([res, res[:1]]).contiguous()
    assert_one_rounding(ops.linear(a33, w, r33, bias),
                        torch.cat([c.want, c.want[:1]]), "linear M=33 (library)")


def test_linear_gate_k_and_n():
    c = gc.build(_spec("v1-m16-n576-k160-ks2"))          # K % 256 != 0
    a, w, res = dev(c.Abuf)[:16], dev(c.W), dev(c.res)
    assert_exact(ops.hip_ops.gemm_skinny(a, w, res, None, 0), c.want, "K=160 kernel")
    assert_one_rounding(ops.linear(a, w, res), c.want, "linear K=160 (library)")
    c = gc.build(_spec("v2-m15-n576-k512-remap-r1"))     # N % 64 != 0
    a, w, res, bias = dev(c.Abuf)[:15], dev(c.W), dev(c.res), dev(c.bias)
    assert_exact(ops.linear(a, w, res, bias), c.want, "linear N=576 (kernel)")
    n = 576 - 32
    assert_one_rounding(
        ops.linear(a, w[:n].contiguous(), res[:, :n].contiguous(), bias[:n].contiguous()),
        c.want[:, :n], "linear N=544 (library)")


def test_linear_w4_gates():
    c = gc.build(_spec("w4-m32-n576-k2048-ks2"))
    N, K = 576, 2048
    packed = c.packed.to(DEV).reshape(N, K // 64, 32)
    scale, zero = dev(c.scale, torch.float16), dev(c.zero, torch.float16)
    a, res, bias = dev(c.Abuf)[:32], dev(c.res), dev(c.bias)
    assert_exact(ops.linear_w4(a, packed, scale, zero, N, residual=res, bias=bias),
                 c.want, "linear_w4 M=32 (kernel)")
    a33 = torch.cat([a, a[:1]]).contiguous()
    r33 = torch.cat([res, res[:1]]).contiguous()
    assert_one_rounding(
        ops.linear_w4(a33, packed, scale, zero, N, residual=r33, bias=bias),
        torch.cat([c.want, c.want[:1]]), "linear_w4 M=33 (dequant + library)")
    c = gc.build(gc.Spec("w4-m4-n64-k192", "w4", 4, 64, 192, 0, bias=True, res=True,
                         seed=65))                       # K % 128 != 0
    got = ops.linear_w4(dev(c.Abuf)[:4], c.packed.to(DEV).reshape(64, 3, 32),
                        dev(c.scale, torch.float16), dev(c.zero, torch.float16), 64,
                        residual=dev(c.res), bias=dev(c.bias))
    assert_one_rounding(got, c.want, "linear_w4 K=192 (dequant + library)")


def test_moe_gemm_grouped_gate_n():
    c = gc.build(_spec("moe-e4-k256-n128-mid-empty"))
    assert_exact(run_moe(c, via_iface=True), c.want, "moe N=128 (kernel)")
    n = 128 - 32
    got = ops.moe_gemm_grouped(dev(c.A), dev(c.W)[:, :n].contiguous(), c.off.to(DEV),
                               c.rowmap.to(DEV), dev(c.scale, torch.float32),
                               S=c.S, mchunks=c.mchunks)
    assert_one_rounding(got, c.want[:, :n], "moe N=96 (torch)")


def test_linear_folded_norm_gate():
    c = gc.build(_spec("norm2-m32-n960-k1280-ks5"))
    a, w, res, bias = dev(c.Abuf)[:32], dev(c.Wfold), dev(c.res), dev(c.bias)
    assert_exact(ops.linear(a, w, res, bias, norm=(None, 0.0)), c.want,
                 "linear norm=(None, eps) M=32 (kernel)")
    a33 = torch.cat([a, a[:1]]).contiguous()
    r33 = torch.cat([res, res[:1]]).contiguous()
    assert_one_rounding(ops.linear(a33, w, r33, bias, norm=(None, 0.0)),
                        torch.cat([c.want, c.want[:1]]),
                        "linear norm=(None, eps) M=33 (rms_norm + library)")


# ---------------------------------------------------------------------------
# realistic-valued complement: randn inputs against fp64, derived bound
# (gemm_cases docstring). Each test prints its worst ratio to the bound.
# ---------------------------------------------------------------------------

def _ratio(got, want, bound, what):
    err = (got.detach().cpu().double() - want).abs()
    # a zero bound (want == 0 with nothing to accumulate) demands err == 0
    r = float(torch.where(bound > 0, err / bound, torch.where(err > 0, math.inf, 0.0)).max())
    print(f"worst |err| / bound, {what}: {r:.3f}")
    assert r <= 1.0, f"{what}: |err| reaches {r:.3f} x the derived bound"
    return r


def _randn_bf(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(BF)


@pytest.mark.parametrize("M,N,K,ks", [(17, 576, 416, 1), (31, 704, 1280, 1),
                                      (32, 576, 1280, 3), (17, 4096, 512, 2)],
                         ids=["v1", "v2", "v2-split", "v2-vector-combine"])
def test_gemm_skinny_realistic(M, N, K, ks):
    gen = torch.Generator().manual_seed(101)
    a, w = _randn_bf(gen, M, K), _randn_bf(gen, N, K, scale=K ** -0.5)
    r, b = _randn_bf(gen, M, N), _randn_bf(gen, N)
    want = a.double() @ w.double().T + b.double() + r.double()
    bound = gc.realistic_bound(want, K, a.double().abs() @ w.double().abs().T)
    got = ops.hip_ops.gemm_skinny(a.to(DEV), w.to(DEV), r.to(DEV), b.to(DEV), ks)
    _ratio(got, want, bound, f"gemm_skinny {M}x{N}x{K} ks={ks}")


@pytest.mark.parametrize("mode", [1, 2])
def test_gemm_skinny_norm_realistic(mode):
    gen = torch.Generator().manual_seed(102)
    M, N, K, eps = 31, 576, 1280, 1e-5
    a, w = _randn_bf(gen, M, K), _randn_bf(gen, N, K, scale=K ** -0.5)
    nw, r = _randn_bf(gen, K), _randn_bf(gen, M, N)
    ad = a.double()
    invr = 1.0 / torch.sqrt((ad ** 2).mean(1, keepdim=True) + eps)
    if mode == 1:
        ahat = ad * invr * nw.double()
        absprod = ahat.abs() @ w.double().abs().T
        want = ahat @ w.double().T + r.double()
        bound = gc.realistic_bound(want, K, absprod, extra=2.0 ** -8 * absprod)
        got = ops.hip_ops.gemm_skinny(a.to(DEV), w.to(DEV), r.to(DEV), None, 0,
                                      nw.to(DEV), eps)
    else:
        wf = (w.double() * nw.double()).to(BF)          # folded, rounded once
        absprod = (ad.abs() @ wf.double().abs().T) * invr
        want = (ad @ wf.double().T) * invr + r.double()
        bound = gc.realistic_bound(want, K, absprod)
        got = ops.linear(a.to(DEV), wf.to(DEV), r.to(DEV), norm=(None, eps))
    _ratio(got, want, bound, f"gemm_skinny mode {mode}")


@pytest.mark.parametrize("K", [160, 768], ids=["v1", "v2"])
def test_moe_gemm_realistic(K):
    gen = torch.Generator().manual_seed(103)
    counts, N = (0, 33, 17, 65), 576
    E, S = len(counts), sum(counts)
    Ta = 40
    a, w = _randn_bf(gen, Ta, K), _randn_bf(gen, E, N, K, scale=K ** -0.5)
    off = torch.zeros(E + 1, dtype=torch.int32)
    off[1:] = torch.tensor(counts).cumsum(0).int()
    rm = torch.randint(0, Ta, (S,), generator=gen).int()
    sc = torch.rand(S, generator=gen)
    eid = torch.repeat_interleave(torch.arange(E), torch.tensor(counts))
    ad, wd = a.double()[rm.long()], w.double()[eid]           # (S,K), (S,N,K)
    want = torch.einsum("sk,snk->sn", ad, wd) * sc.double()[:, None]
    absprod = torch.einsum("sk,snk->sn", ad.abs(), wd.abs()) * sc.double()[:, None]
    bound = gc.realistic_bound(want, K, absprod)
    got = ops.moe_gemm_grouped(a.to(DEV), w.to(DEV), off.to(DEV), rm.to(DEV),
                               sc.to(DEV), S=S, mchunks=3)
    _ratio(got, want, bound, f"moe_gemm K={K}")


@pytest.mark.parametrize("M,N,K,ks", [(17, 576, 1024, 2), (1, 576, 4096, 0)],
                         ids=["mfma", "gemv"])
def test_gemm_w4_realistic(M, N, K, ks):
    gen = torch.Generator().manual_seed(104)
    a = _randn_bf(gen, M, K)
    packed, scale, zero = ref.quant4_pack(torch.randn(N, K, generator=gen) * K ** -0.5)
    q = torch.stack([(packed & 0xF).double(), (packed >> 4).double()], dim=-1)
    wd = (q.reshape(N, K // 64, 64) * scale.double()[..., None]
          + zero.double()[..., None]).reshape(N, K)        # exact in fp64
    r = _randn_bf(gen, M, N)
    want = a.double() @ wd.T + r.double()
    absprod = a.double().abs() @ wd.abs().T
    bound = gc.realistic_bound(want, K, absprod, extra=2.0 ** -10 * absprod)
    got = ops.hip_ops.gemm_w4(a.half().to(DEV), packed.reshape(N, K // 2).to(DEV),
                              scale.to(DEV), zero.to(DEV), r.to(DEV), None, N, ks)
    _ratio(got, want, bound, f"gemm_w4 {M}x{N}x{K} ks={ks}")


# ---------------------------------------------------------------------------
# gelu_tanh / add_bf16: numel % 8 != 0 tails
# ---------------------------------------------------------------------------

def _bf16_values_upto(limit):
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    v = bits.view(BF)
    return v[v.float().abs() <= limit]                   # drops nan / inf too


def _check_gelu(x, what):
    xd = x.double()
    want = 0.5 * xd * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (xd + 0.044715 * xd ** 3)))
    bound = 2.0 ** -8 * want.abs() + xd.abs() * 2.0 ** -22 + 2.0 ** -134
    got = ops.gelu_tanh(x.to(DEV))
    assert got.shape == x.shape and got.dtype == BF
    return _ratio(got, want, bound, what)


@pytest.mark.parametrize("tail", [0, 1, 7])
def test_gelu_tanh_parity(tail):
    """Every bf16 value in [-8, 8] plus +-large against fp64
    0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))), at numel 8k + tail.

    Bound: one bf16 rounding of the result, 2^-8 |want|, plus the f32 error
    before it. The inner argument carries ~4 f32 roundings and tanh'(u) u <=
    0.45, tanhf is within 5 ulp (ulp(t) <= 2^-24 as |t| <= 1) and 1 + t adds
    one rounding: the absolute error of (1 + t) is below 8 * 2^-24 (absolute,
    because 1 + t cancels for negative x), so that of the result is below
    0.5 |x| * 8 * 2^-24 = |x| 2^-22; the two product roundings, 2^-23 |want|,
    vanish next to the bf16 term. Subnormal results round to a multiple of
    2^-133, the smallest bf16 subnormal: half of it, 2^-134, is added.
    Worst observed ratio on an MI355X: 0.996 (a bf16 rounding just above a
    power of two; the f32 term is not what is approached)."""
    v = _bf16_values_upto(8.0)
    big = torch.tensor([64.0, -64.0, 1e4, -1e4, 3e38, -3e38]).to(BF)
    n = ((v.numel() + 6) // 8 - 1) * 8 + tail
    x = torch.cat([big, v[:n - 6]])
    assert x.numel() == n and n % 8 == tail
    _check_gelu(x, f"gelu_tanh numel={n}")


def test_gelu_tanh_fewer_than_eight():
    _check_gelu(torch.tensor([-1.0, 0.5, 2.0]).to(BF), "gelu_tanh numel=3")


@pytest.mark.parametrize("n", [8 * 700, 8 * 700 + 1, 8 * 700 + 7, 5])
def test_add_bf16_tail(n):
    """a + b in f32 rounded once to bf16, tail elements included."""
    gen = torch.Generator().manual_seed(n)
    a, b = _randn_bf(gen, n), _randn_bf(gen, n, scale=3.0)
    got = ops.hip_ops.add_bf16(a.to(DEV), b.to(DEV)).cpu()
    assert torch.equal(got, (a.float() + b.float()).to(BF))
