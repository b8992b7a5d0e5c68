"""Shared inputs, models, bounds and mutations for the parity tests of the
per-layer kernels: rms_norm, rms_norm_residual, layer_norm, rope_apply_,
swiglu, kv_write, kv_gather, quant4_pack and quant4_unpack
(test_elementwise_cases_cpu.py and test_gpu_elementwise_exact.py). Plain
helper module, laid out like gemm_cases.py.

Per op there is a list of specs, a cached deterministic CPU builder, a model
written out directly in fp64 (quant4_pack: in f32, see below) with a `mut`
knob per defect, and `check(case, got)`, the case's own check, which returns
the worst |err| / bound (exact cases: 0.0 or inf).

Two kinds of check.

EXACT. Inputs for which every intermediate is exact in f32 in any order and
the result is exactly a bf16 value; the device must match with torch.equal.
  norms   every entry of row m is +-2^j(m) in balanced numbers (mean 0, mean
          square 4^j), eps = 0, weights are signed powers of two that differ
          along H, the bias small integers. 1/sqrt(4^j) = 2^-j: the device's
          rsqrt of a power of four is exact (gemm_cases.py relies on the
          same). Layer norm also runs rows of c + 2^j and c - 2^j in equal
          numbers with c = k 2^j: mean c, variance 4^j. For k = 3 a one-pass
          variance is exact as well; for |k| >= 100 sum x^2 passes 2^24
          units from H = 2048 on and only the mean-subtracting form stays
          exact.
  rope    tables drawn from {0, +-0.5, +-1, +-2}, q and k small integers.
  kv      pure copies.
  quant4  unpack with power-of-two scales and integer zeros; pack is defined
          by its f32 roundings (min, max, (max - min) / 15, (v - min) / sc,
          rint), each of them a correctly rounded IEEE operation on device
          and host alike, so its model is written in f32 and packed, scale
          and zero must all match bit for bit. |min| above the f16 range
          (65504) gives an inf zero in both implementations; no case goes
          there (values stay within +-3e4).
The builder asserts both properties for every exact case: `want` survives a
round trip through bf16, and every sum the kernel forms stays below 2^24
units of the smallest power of two in play.

REALISTIC. randn-like bf16 inputs against the fp64 model,
    |got - want| <= 2^-8 |want| + (f32 terms).
2^-8 |want| is the strict bound of one bf16 rounding (subnormal results:
plus half the smallest bf16 subnormal, 2^-134, where stated). The f32 terms,
u = 2^-24 the f32 unit roundoff:

  rms_norm / rms_norm_residual   y = x inv w, inv = rsqrt(mean(x^2) + eps)
      A sum of L-deep f32 additions of non-negative terms has relative error
      <= L u. L = 8 ITERS + 10 is the longest chain in the kernel's order:
      8 ITERS terms in a lane, 6 butterfly steps, 4 waves (the squares add a
      rounding each: + 1). Division by H and + eps: 2 u. rsqrt halves the
      relative error of its argument; rsqrtf itself is within 2 ulp = 4 u.
      Two products: 2 u. Together
          f32 term = |want| ((L + 3) / 2 + 6) u.
      The residual form normalises the ROUNDED h = bf16(x + r), as kernel
      and reference both do, and h itself must match bit for bit.
  layer_norm   y = (x - mu) inv w + b, inv = rsqrt(mean((x - mu)^2) + eps)
      e_mu = (L + 1) u mean|x| bounds the error of mu (L-deep sum of terms
      of either sign, one division). c = x - mu carries e_mu + u |c|. The
      sum of c^2 over the row moves by H e_mu^2 (the cross term vanishes as
      sum c = 0), relative e_mu^2 / (var + eps), and by its own roundings as
      above with 2 more u for c. With the two products and the bias add
          f32 term = |w| inv e_mu
                   + |c inv w| (((L + 5) / 2 + 6) u + e_mu^2 / (2 (var + eps)))
                   + 3 u |c inv w| + u |want|.
      On a row with |mean| / sigma = 250 at H = 4544 the e_mu term is 6e-4
      sigma: an f32 one-pass variance, t2/H - mu^2, which is off by 0.33 %
      there and negative on near-constant rows at H = 14336, does not fit
      (mutation `one_pass_variance`, the record of the defect this suite was
      written against).
  rope_apply_   o = x1 c -+ x2 s: two products and a sum, each rounded:
          f32 term = 2 u (|x1 c| + |x2 s|).
      The tables are arguments, so their own rounding is no error.
  swiglu   o = g / (1 + exp(-g)) u'
      exp(-g) is exp2(-g log2(e)): the argument carries 2 u relative, i.e.
      2 u |g| relative in the result, v_exp_f32 1 ulp = 2 u more. In 1 +
      exp(-g) that weighs sigmoid(-g) <= 1; the sum, the division and the
      product round once each:
          f32 term = |want| ((|g| + 1) sigmoid(-g) 2 u + 3 u)  + 2^-134.
      For g < -88.7 exp(-g) exceeds the f32 range, 1 + inf = inf and any
      f32 form returns -0 where the true result is |g u'| e^g <= 3.3e-37
      |u'|: there the whole of |want| is added (it matters for g = -100
      alone, 3.7e-42 |u'|, which a large u' lifts above 2^-134).
  quant4_unpack   q s + z with q <= 15 and s in f16: the product is exact
      in f32, the sum rounds once (or the whole is one fma):
          f32 term = u |want|.

The CPU test asserts that the fp64 model rounded once to bf16 has ratio
<= 1 on every case (the bound is not violated by a perfect implementation)
and that ops.reference in f32 stays within it (it is attainable by an honest
f32 one).

MUTATIONS. `model(case, mut)` with one knob per defect; for every mutation
at least one applicable case fails its own check when the mutated result is
rounded to bf16 the way a device would store it. Launch geometry (ITERS,
lanes, waves, grid caps) mirrors ext.hip and is used only by the mutations
and the bounds, never by `want`.

Worst observed ratio |err| / bound on an MI355X, against the fp64 models
(see test_gpu_elementwise_exact.py, which prints them):
    rms_norm           0.996     rms_norm_residual  0.996 (h bit-exact)
    layer_norm         0.995     (offset rows 0.957 / 0.964 / 0.975 at H =
                                 1024 / 4544 / 14336; near-constant rows
                                 0.818 / 0.290 / 0.488)
    rope_apply_        0.994     swiglu             0.996
    quant4_unpack      0.996     gelu_tanh past the grid cap 0.996
As in gemm_cases.py, figures just below 1 are the final bf16 rounding, whose
strict bound a value just above a power of two nearly reaches: ops.reference
on the CPU gives the same layer-norm figures to three digits. The f32 terms
are not what is approached.
The layer_norm kernel before the mean-subtracting variance (one-pass
t2/H - mu^2), same cases, same device: offset rows 6.657 / 5.982 / 1.383,
near-constant rows 190.4 at H = 1024, 148.0 at H = 4544, and NaN rows at
H = 14336; every other layer-norm case passed.
"""
import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

BF = torch.bfloat16
POISON = 1024.0
U = 2.0 ** -24
HALF_SUBNORMAL = 2.0 ** -134
INF = float("inf")


def ids(specs):
    return [s.name for s in specs]


class Case:
    def __init__(self, spec):
        self.spec = spec


def _gen(seed):
    return torch.Generator().manual_seed(9000 + seed)


def _ri(lo, hi, shape, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def _sign(shape, gen):
    return _ri(0, 1, shape, gen) * 2 - 1


def _randn_bf(gen, *shape, scale=1.0):
    """randn values that are exactly bf16, as float64"""
    return (torch.randn(*shape, generator=gen) * scale).to(BF).double()


def is_bf16(t):
    return torch.equal(t.to(BF).double(), t)


def as_device_would(t):
    """what a device stores of an fp64 result: one bf16 rounding"""
    return t.to(BF).double()


def poison(shape, gen):
    return _sign(shape, gen) * POISON


def worst_ratio(got, want, bound):
    """max |got - want| / bound; a NaN, an inf or an error where the bound is
    zero counts as inf."""
    got = got.detach().cpu().double().reshape(want.shape)
    err = (got - want).abs()
    err[~torch.isfinite(got)] = INF
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, INF, 0.0))
    return float(r.max()) if r.numel() else 0.0


def exact_ratio(got, want):
    got = got.detach().cpu().double().reshape(want.shape)
    return 0.0 if torch.equal(got, want) else INF


def describe_mismatch(got, want):
    got = got.detach().cpu().double().reshape(want.shape)
    err = (got - want).abs()
    err[~torch.isfinite(got)] = INF
    flat = int(err.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), want.shape))
    return (f"{int((err > 0).sum())} of {want.numel()} elements differ; worst at "
            f"{idx}: got {float(got[idx])}, want {float(want[idx])}")


# ---------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------

NORM_BLOCK = 256
NORM_H = (8, 64, 2048, 2056, 4096, 4544, 8192, 8200, 14336, 16384)
NORM_OPS = ("rms", "rms_res", "ln")


def norm_iters(H):
    """ITERS of the launched instantiation (dispatch_iters in ext.hip)."""
    per = NORM_BLOCK * 8
    for it in (1, 2, 4, 8):
        if H <= it * per:
            return it
    raise ValueError(H)


def norm_depth(H):
    """L: the longest chain of f32 additions in the kernels' summation order."""
    return 8 * norm_iters(H) + 10


@dataclass(frozen=True)
class NormSpec:
    name: str
    op: str                   # "rms" | "rms_res" | "ln"
    kind: str                 # exact | exact_offset | randn | outlier | small
    #                           | offset | nearconst
    H: int
    N: int = 3
    eps: float = 1e-5
    seed: int = 0

    @property
    def exact(self):
        return self.kind.startswith("exact")


def _norm_specs():
    out, seed = [], 0
    for op in NORM_OPS:
        for H in NORM_H:
            seed += 1
            out.append(NormSpec(f"{op}-exact-h{H}", op, "exact", H, eps=0.0, seed=seed))
            out.append(NormSpec(f"{op}-randn-h{H}", op, "randn", H, seed=seed))
        out.append(NormSpec(f"{op}-exact-h4544-n1", op, "exact", 4544, N=1, eps=0.0,
                            seed=seed + 50))
        for H in (2056, 8200, 14336):
            out.append(NormSpec(f"{op}-outlier-h{H}", op, "outlier", H, seed=seed + H))
        for H in (64, 4544):
            out.append(NormSpec(f"{op}-small-h{H}", op, "small", H, seed=seed + H))
    for H in NORM_H:
        out.append(NormSpec(f"ln-exact-offset-h{H}", "ln", "exact_offset", H, eps=0.0,
                            seed=300 + H))
    for H in (1024, 4544, 14336):
        out.append(NormSpec(f"ln-offset-h{H}", "ln", "offset", H, seed=400 + H))
    # the four near-constant rows of the one-pass-variance table
    out.append(NormSpec("ln-nearconst-h1024", "ln", "nearconst", 1024, N=1))
    out.append(NormSpec("ln-nearconst-h4544", "ln", "nearconst", 4544, N=1))
    out.append(NormSpec("ln-nearconst-h14336", "ln", "nearconst", 14336, N=2))
    return out


NORM_SPECS = _norm_specs()
NEARCONST_ROWS = {   # H -> [(majority, other, count of other)]
    1024: [(1004.0, 1008.0, 5)],
    4544: [(251.0, 252.0, 1)],
    14336: [(251.0, 252.0, 1), (100.5, 101.0, 3)],
}


def _balanced_signs(N, H, gen):
    s = torch.ones(N, H, dtype=torch.float64)
    for m in range(N):
        s[m, torch.randperm(H, generator=gen)[: H // 2]] = -1.0
    return s


def _pow2_weights(H, gen):
    """signed powers of two in [1/4, 4]; w[d] != w[d + 8] for most d"""
    return _sign((H,), gen) * 2.0 ** _ri(-2, 2, (H,), gen)


@functools.lru_cache(maxsize=None)
def build_norm(spec):
    c = Case(spec)
    gen = _gen(spec.seed)
    N, H = spec.N, spec.H
    c.r = None
    if spec.exact:
        j = torch.tensor([(-3, 0, 5)[(m + spec.seed) % 3] for m in range(N)]).double()
        a = (2.0 ** j)[:, None]
        s = _balanced_signs(N, H, gen)
        if spec.kind == "exact_offset":
            # one small offset and two at which sum x^2 leaves the exact range
            # of f32 (H k^2 > 2^24 from H = 2048 on): exactness then rests on
            # the mean being subtracted first
            k = torch.tensor([(3, -100, 120)[(m + spec.seed) % 3] for m in range(N)]).double()
            x = (k[:, None] + s) * a
            c.k = k
        else:
            x = s * a
        if spec.op == "rms_res":
            # h = x + r with nothing to round: 3a/2 - a/2, or -a + 2a
            alt = _ri(0, 1, (N, H), gen)
            c.r = torch.where(alt > 0, -x / 2, 2 * x)
            x = torch.where(alt > 0, 3 * x / 2, -x)
        c.w = _pow2_weights(H, gen)
        c.b = _ri(-4, 4, (H,), gen) if spec.op == "ln" else None
        # exactness in any order: row sums of |x| and x^2 in their own units
        assert H * 121 < 2 ** 24                        # sum |x|, sum (x - mean)^2
    else:
        x = _randn_bf(gen, N, H)
        if spec.kind == "outlier":
            # row 0: in the last, partial iteration; the others anywhere
            at = torch.randint(0, H, (N,), generator=gen)
            at[0] = H - 3
            x[torch.arange(N), at] = 2.0 ** 12
        elif spec.kind == "small":
            # eps = 1e-5 is a large part of the variance; the last row is zero
            x = (x * torch.tensor([2.0 ** -8, 2.0 ** -10, 0.0])[:N, None]).to(BF).double()
        elif spec.kind == "offset":
            mean = torch.tensor([64.0, -250.0, 1000.0])[:N, None]
            sig = torch.tensor([1.0, 1.0, 4.0])[:N, None]
            x = (mean + sig * torch.randn(N, H, generator=gen).double()).to(BF).double()
        elif spec.kind == "nearconst":
            for m, (maj, oth, cnt) in enumerate(NEARCONST_ROWS[H]):
                x[m] = maj
                x[m, torch.randperm(H, generator=gen)[:cnt]] = oth
        if spec.op == "rms_res":
            c.r = _randn_bf(gen, N, H, scale=0.5)
        c.w = _randn_bf(gen, H)
        c.b = _randn_bf(gen, H) if spec.op == "ln" else None
    c.x = x
    assert is_bf16(c.x) and is_bf16(c.w)
    # the device sees x as rows [1, 1 + N) of a taller poisoned buffer
    c.xbuf = torch.cat([poison((1, H), gen), c.x, poison((1, H), gen)])
    c.want = model_norm(c)
    if spec.exact:
        for t in c.want.values():
            assert is_bf16(t), spec.name
    return c


def _f32_kernel_order_sum(vals, H):
    """sum of vals (N, H) in f32 in the norm kernels' order: a lane adds its
    8 ITERS elements in turn, a 64-lane xor butterfly, then the 4 waves."""
    N = vals.shape[0]
    iters = norm_iters(H)
    pad = np.zeros((N, iters * NORM_BLOCK * 8), dtype=np.float32)
    pad[:, :H] = vals
    pad = pad.reshape(N, iters, NORM_BLOCK, 8)
    lane = np.zeros((N, NORM_BLOCK), dtype=np.float32)
    for it in range(iters):
        for j in range(8):
            lane = (lane + pad[:, it, :, j]).astype(np.float32)
    lane = lane.reshape(N, 4, 64)
    idx = np.arange(64)
    m = 1
    while m < 64:
        lane = (lane + lane[:, :, idx ^ m]).astype(np.float32)
        m <<= 1
    tot = np.zeros(N, dtype=np.float32)
    for w in range(4):
        tot = (tot + lane[:, w, 0]).astype(np.float32)
    return tot


def _one_pass_f32(h, H):
    """mu and var of the one-pass f32 form t2/H - mu*mu in the kernel's order"""
    hf = h.numpy().astype(np.float32)
    t1 = _f32_kernel_order_sum(hf, H)
    t2 = _f32_kernel_order_sum((hf * hf).astype(np.float32), H)
    mu = (t1 / np.float32(H)).astype(np.float32)
    var = ((t2 / np.float32(H)).astype(np.float32) - (mu * mu).astype(np.float32))
    return (torch.from_numpy(mu.astype(np.float64))[:, None],
            torch.from_numpy(var.astype(np.float32).astype(np.float64))[:, None])


NORM_MUTATIONS = (
    "norm_sum_stops_at_last_full_iter",
    "norm_wave_partial_dropped",
    "norm_mean_over_padded_length",
    "norm_weight_shifted_by_8",
    "norm_residual_not_rounded",
    "norm_eps_dropped",
    "one_pass_variance",
)


def norm_applicable(spec):
    H, per = spec.H, NORM_BLOCK * 8
    out = []
    if H > per and H % per:
        out.append("norm_sum_stops_at_last_full_iter")
    if H >= per:
        out.append("norm_wave_partial_dropped")
    if H != norm_iters(H) * per:
        out.append("norm_mean_over_padded_length")
    if H > 8:
        out.append("norm_weight_shifted_by_8")
    if spec.op == "rms_res" and not spec.exact:
        out.append("norm_residual_not_rounded")
    if spec.kind == "small":
        out.append("norm_eps_dropped")
    if spec.op == "ln" and spec.kind in ("offset", "nearconst"):
        out.append("one_pass_variance")
    return out


def model_norm(c, mut=None):
    """{"y": ...} (rms_res: also "h"), float64."""
    spec = c.spec
    H, per = spec.H, NORM_BLOCK * 8
    x, w, eps = c.x, c.w, spec.eps
    out = {}
    h = x
    if spec.op == "rms_res":
        out["h"] = (x + c.r).to(BF).double()
        h = x + c.r if mut == "norm_residual_not_rounded" else out["h"]
    d = torch.arange(H)
    live = torch.ones(H, dtype=torch.float64)          # elements the sums see
    if mut == "norm_sum_stops_at_last_full_iter":
        live = (d < (H // per) * per).double()
    if mut == "norm_wave_partial_dropped":
        live = (((d % per) // 8) // 64 != 3).double()
    denom = float(norm_iters(H) * per) if mut == "norm_mean_over_padded_length" else float(H)
    if mut == "norm_eps_dropped":
        eps = 0.0
    if mut == "norm_weight_shifted_by_8":
        w = w[(d + 8) % H]
    with np.errstate(all="ignore"):
        if spec.op == "ln":
            if mut == "one_pass_variance":
                mu, var = _one_pass_f32(h, H)
            else:
                mu = (h * live).sum(1, keepdim=True) / denom
                var = (((h - mu) ** 2) * live).sum(1, keepdim=True) / denom
            inv = 1.0 / torch.sqrt(var + eps)           # nan where var + eps < 0
            y = (h - mu) * inv * w + c.b
        else:
            ms = ((h ** 2) * live).sum(1, keepdim=True) / denom
            inv = 1.0 / torch.sqrt(ms + eps)
            y = h * inv * w
    out["y"] = y
    return out


def norm_bound(c):
    """bound on |y - want["y"]| for a realistic case (module docstring)."""
    spec = c.spec
    H, L = spec.H, norm_depth(spec.H)
    want = c.want["y"]
    if spec.op != "ln":
        return 2.0 ** -8 * want.abs() + want.abs() * ((L + 3) / 2 + 6) * U
    x = c.x
    mu = x.mean(1, keepdim=True)
    cc = x - mu
    var = (cc ** 2).mean(1, keepdim=True)
    inv = 1.0 / torch.sqrt(var + spec.eps)
    e_mu = (L + 1) * U * x.abs().mean(1, keepdim=True)
    core = (cc * inv * c.w).abs()
    return (2.0 ** -8 * want.abs() + c.w.abs() * inv * e_mu
            + core * (((L + 5) / 2 + 6) * U + e_mu ** 2 / (2 * (var + spec.eps)))
            + 3 * U * core + U * want.abs())


def check_norm(c, got):
    """got: {"y": tensor[, "h": tensor]} -> worst ratio (exact: 0 or inf)."""
    r = 0.0
    if c.spec.op == "rms_res":
        r = exact_ratio(got["h"], c.want["h"])
    if c.spec.exact:
        return max(r, exact_ratio(got["y"], c.want["y"]))
    return max(r, worst_ratio(got["y"], c.want["y"], norm_bound(c)))


# ---------------------------------------------------------------------------
# rope
# ---------------------------------------------------------------------------

ROPE_B, ROPE_T, ROPE_HQ = 3, 5, 4
ROPE_MAXPOS = 37
ROPE_POS = ((5, 0, 36, 5, 17), (36, 2, 2, 9, 0), (11, 30, 4, 36, 1))
# the same with out-of-table positions where ROPE_POS has 0 and max_pos - 1
ROPE_POS_CLAMP = ((5, -3, 42, 5, 17), (42, 2, 2, 9, -3), (11, 30, 4, 42, 1))


@dataclass(frozen=True)
class RopeSpec:
    name: str
    D: int
    Hkv: int
    kind: str = "exact"       # exact | clamp | real
    seed: int = 0


def _rope_specs():
    out = []
    for D in (64, 96, 128, 256, 512):
        for Hkv in (1, 4):
            out.append(RopeSpec(f"rope-exact-d{D}-hkv{Hkv}", D, Hkv, seed=D + Hkv))
    out.append(RopeSpec("rope-clamp-d128-hkv1", 128, 1, "clamp", seed=129))
    out.append(RopeSpec("rope-clamp-d96-hkv4", 96, 4, "clamp", seed=100))
    out.append(RopeSpec("rope-real-d128-hkv1", 128, 1, "real", seed=7))
    out.append(RopeSpec("rope-real-d128-hkv4", 128, 4, "real", seed=8))
    return out


ROPE_SPECS = _rope_specs()


@functools.lru_cache(maxsize=None)
def build_rope(spec):
    c = Case(spec)
    gen = _gen(500 + spec.seed)
    B, T, Hq, Hkv, D = ROPE_B, ROPE_T, ROPE_HQ, spec.Hkv, spec.D
    if spec.kind == "real":
        c.max_pos = 2048
        inv_freq = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
        fr = torch.outer(torch.arange(c.max_pos, dtype=torch.float64), inv_freq)
        # the f32 tables the op is handed (what rope_cos_sin produces)
        c.cos, c.sin = fr.cos().float().double(), fr.sin().float().double()
        c.q, c.k = _randn_bf(gen, B, Hq, T, D), _randn_bf(gen, B, Hkv, T, D)
        c.pos = torch.tensor(((5, 0, 2047, 5, 17), (2047, 2, 2, 900, 0),
                              (11, 1030, 4, 2047, 1)))
    else:
        c.max_pos = ROPE_MAXPOS
        vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0], dtype=torch.float64)
        shape = (c.max_pos, D // 2)
        c.cos = vals[torch.randint(0, 7, shape, generator=gen)]
        c.sin = vals[torch.randint(0, 7, shape, generator=gen)]
        c.q, c.k = _ri(-8, 8, (B, Hq, T, D), gen), _ri(-8, 8, (B, Hkv, T, D), gen)
        c.pos = torch.tensor(ROPE_POS_CLAMP if spec.kind == "clamp" else ROPE_POS)
    assert c.pos.min() <= 0 and c.pos.max() >= c.max_pos - 1
    c.want = model_rope(c)
    if spec.kind != "real":
        assert is_bf16(c.want[0]) and is_bf16(c.want[1])    # |o| <= 32, steps of 1/2
    if spec.kind == "clamp":
        # exactly the results of positions 0 and max_pos - 1
        ref_pos = torch.tensor(ROPE_POS)
        assert all(torch.equal(a, b) for a, b in
                   zip(c.want, model_rope(c, pos=ref_pos)))
    return c


ROPE_MUTATIONS = (
    "rope_table_row_t",
    "rope_batch0_positions",
    "rope_sin_sign_flipped",
    "rope_interleaved_partner",
    "rope_k_heads_indexed_with_hq",
    "rope_clamp_replaced_by_wrap",
)


def rope_applicable(spec):
    out = list(ROPE_MUTATIONS[:4])
    if spec.Hkv != ROPE_HQ:
        out.append("rope_k_heads_indexed_with_hq")
    if spec.kind == "clamp":
        out.append("rope_clamp_replaced_by_wrap")
    return out


def _rotate(x, cs, sn, mut):
    """x (..., T, D) with cs/sn (..., T, D/2) broadcastable."""
    D = x.shape[-1]
    if mut == "rope_sin_sign_flipped":
        sn = -sn
    if mut == "rope_interleaved_partner":
        x1, x2 = x[..., 0::2], x[..., 1::2]
        o = torch.empty_like(x)
        o[..., 0::2] = x1 * cs - x2 * sn
        o[..., 1::2] = x2 * cs + x1 * sn
        return o
    x1, x2 = x[..., : D // 2], x[..., D // 2:]
    return torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], dim=-1)


def model_rope(c, mut=None, pos=None):
    """(q, k) after the in-place rotation, float64."""
    B, T = c.pos.shape
    pos = c.pos if pos is None else pos
    if mut == "rope_clamp_replaced_by_wrap":
        p = pos % c.max_pos
    else:
        p = pos.clamp(0, c.max_pos - 1)
    if mut == "rope_table_row_t":
        p = torch.arange(T).expand(B, T)
    if mut == "rope_batch0_positions":
        p = p[:1].expand(B, T)
    cs, sn = c.cos[p][:, None], c.sin[p][:, None]            # (B, 1, T, D/2)
    q = _rotate(c.q, cs, sn, mut)
    if mut != "rope_k_heads_indexed_with_hq":
        return q, _rotate(c.k, cs, sn, mut)
    # k row (b, h, t) addressed as ((b Hq + h) T + t) D in k's own buffer:
    # rows that land inside it are rotated there, the rest of k is untouched
    Hq, Hkv, D = c.q.shape[1], c.k.shape[1], c.k.shape[3]
    flat = c.k.clone().reshape(-1, D)
    for b in range(B):
        for h in range(Hkv):
            for t in range(T):
                row = (b * Hq + h) * T + t
                if row < flat.shape[0]:
                    flat[row] = _rotate(flat[row][None], cs[b, 0, t][None],
                                        sn[b, 0, t][None], None)[0]
    return q, flat.reshape(c.k.shape)


def rope_bound(c):
    p = c.pos.clamp(0, c.max_pos - 1)
    cs, sn = c.cos[p][:, None].abs(), c.sin[p][:, None].abs()
    out = []
    for x, want in zip((c.q, c.k), c.want):
        D = x.shape[-1]
        a1, a2 = x[..., : D // 2].abs(), x[..., D // 2:].abs()
        mag = torch.cat([a1 * cs + a2 * sn, a2 * cs + a1 * sn], dim=-1)
        out.append(2.0 ** -8 * want.abs() + 2 * U * mag)
    return out


def check_rope(c, got):
    if c.spec.kind != "real":
        return max(exact_ratio(g, w) for g, w in zip(got, c.want))
    return max(worst_ratio(g, w, b) for g, w, b in zip(got, c.want, rope_bound(c)))


# ---------------------------------------------------------------------------
# swiglu (and the flat grids of gelu_tanh / add_bf16)
# ---------------------------------------------------------------------------

FLAT_GRID_CAP = 2048          # swiglu, gelu_tanh, add_bf16, kv_gather: blocks of 256
UNPACK_GRID_CAP = 4096        # quant4_unpack
PAST_CAP_NUMEL = 8 * (FLAT_GRID_CAP * 256 + 300) + 5      # gelu_tanh / add_bf16


def bf16_values_upto(limit):
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    v = bits.view(BF)
    return v[v.float().abs() <= limit]                   # drops nan / inf too


@dataclass(frozen=True)
class SwigluSpec:
    name: str
    N: int                    # 0: as many rows as the gate sweep needs
    I: int
    seed: int = 0


SWIGLU_SPECS = (
    SwigluSpec("swiglu-all-gates-i8", 0, 8, seed=1),
    SwigluSpec("swiglu-6x512", 6, 512, seed=2),
    SwigluSpec("swiglu-257x16392-past-cap", 257, 16392, seed=3),
)
assert 257 * (16392 // 8) > FLAT_GRID_CAP * 256


def swiglu_gates():
    """every bf16 value in [-16, 16] (both zeros among them), +-64, +-100"""
    extra = torch.tensor([64.0, -64.0, 100.0, -100.0, 0.0, -0.0]).to(BF)
    return torch.cat([extra, bf16_values_upto(16.0)]).double()


@functools.lru_cache(maxsize=None)
def build_swiglu(spec):
    c = Case(spec)
    gen = _gen(700 + spec.seed)
    gates = swiglu_gates()
    ups = torch.tensor([1.0, -0.37109375, 3.015625, 200.0], dtype=torch.float64)
    I = spec.I
    if spec.N == 0:
        # each gate with each of a few up values, 8 to a row
        n = gates.numel() * ups.numel()
        N = -(-n // I)
        g = gates.repeat_interleave(ups.numel())
        u = ups.repeat(gates.numel())
        pad = N * I - n
        g = torch.cat([g, gates[:pad]]).reshape(N, I)
        u = torch.cat([u, ups[0].expand(pad)]).reshape(N, I)
    else:
        N = spec.N
        n = N * I
        # the gate sweep tiled through the tensor at a stride coprime to its
        # length, under randn up values
        idx = (torch.arange(n) * 7919) % gates.numel()
        g = gates[idx].reshape(N, I)
        u = _randn_bf(gen, N, I, scale=2.0)
    assert is_bf16(g) and is_bf16(u)
    c.gu = torch.cat([g, u], dim=1)                      # (N, 2I)
    c.want = model_swiglu(c)
    assert bool(torch.isfinite(c.want).all())
    return c


SWIGLU_MUTATIONS = ("swiglu_gate_up_swapped", "swiglu_row_stride_i",
                    "swiglu_second_sweep_missing")


def swiglu_applicable(spec):
    out = ["swiglu_gate_up_swapped"]
    if spec.N != 1:
        out.append("swiglu_row_stride_i")
    N = build_swiglu(spec).gu.shape[0]
    if N * (spec.I // 8) > FLAT_GRID_CAP * 256:
        out.append("swiglu_second_sweep_missing")
    return out


def model_swiglu(c, mut=None):
    N, I = c.gu.shape[0], c.gu.shape[1] // 2
    if mut == "swiglu_row_stride_i":
        # row n read at n * I in the flat input (length 2I from there)
        flat = torch.cat([c.gu.reshape(-1), torch.zeros(2 * I, dtype=torch.float64)])
        rows = torch.stack([flat[n * I: n * I + 2 * I] for n in range(N)])
        g, u = rows[:, :I], rows[:, I:]
    else:
        g, u = c.gu[:, :I], c.gu[:, I:]
    if mut == "swiglu_gate_up_swapped":
        g, u = u, g
    out = g * torch.sigmoid(g) * u
    if mut == "swiglu_second_sweep_missing":
        out = out.clone()
        out.reshape(-1)[FLAT_GRID_CAP * 256 * 8:] = float("nan")   # never written
    return out


def swiglu_bound(c):
    I = c.gu.shape[1] // 2
    g = c.gu[:, :I]
    want = c.want.abs()
    return (2.0 ** -8 * want
            + want * ((g.abs() + 1) * torch.sigmoid(-g) * 2 * U + 3 * U)
            + want * (g < -88.7).double()
            + HALF_SUBNORMAL)


def check_swiglu(c, got):
    return worst_ratio(got, c.want, swiglu_bound(c))


def gelu_model(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_bound(x, want):
    """the bound of test_gelu_tanh_parity (test_gpu_gemm_exact.py)"""
    return 2.0 ** -8 * want.abs() + x.abs() * 2.0 ** -22 + HALF_SUBNORMAL


# ---------------------------------------------------------------------------
# paged KV
# ---------------------------------------------------------------------------

KV_B, KV_T, KV_MAXP = 3, 5, 4


@dataclass(frozen=True)
class KVSpec:
    name: str
    Hkv: int
    D: int
    P: int
    B: int = KV_B
    maxp: int = KV_MAXP
    big: bool = False         # gather past the grid cap: random pool, no write
    seed: int = 0


def _kv_specs():
    out = []
    for Hkv, D in ((1, 64), (2, 128), (8, 512), (3, 96)):
        for P in (16, 32):
            out.append(KVSpec(f"kv-h{Hkv}-d{D}-p{P}", Hkv, D, P, seed=Hkv * D + P))
    return out


KV_SPECS = _kv_specs()
KV_BIG_SPEC = KVSpec("kv-gather-h8-d512-ctx1030-past-cap", 8, 512, 16, B=2, maxp=65,
                     big=True, seed=99)
KV_BIG_CTX = 1030
assert KV_BIG_CTX * 8 * (512 // 8) > FLAT_GRID_CAP * 256
assert KV_BIG_CTX <= 65 * 16


def kv_gather_ctxs(spec):
    if spec.big:
        return (KV_BIG_CTX,)
    return (1, spec.P, spec.P + 1, 2 * spec.P + 7)


@functools.lru_cache(maxsize=None)
def build_kv(spec):
    c = Case(spec)
    gen = _gen(800 + spec.seed)
    B, Hkv, D, P, maxp, T = spec.B, spec.Hkv, spec.D, spec.P, spec.maxp, KV_T
    n_pages = B * maxp + 3                               # 3 pages nobody owns
    c.page_table = torch.randperm(n_pages, generator=gen)[: B * maxp].reshape(B, maxp).int()
    if spec.big:
        c.k_pool0 = _randn_bf(gen, n_pages, Hkv, P, D)
        c.v_pool0 = _randn_bf(gen, n_pages, Hkv, D, P)
        c.k_pool, c.v_pool = c.k_pool0, c.v_pool0
        return c
    c.k_pool0 = poison((n_pages, Hkv, P, D), gen)
    c.v_pool0 = poison((n_pages, Hkv, D, P), gen)
    # row 0 crosses a page boundary, row 1 ends in the last slot of its last
    # page, row 2 starts at 0
    c.start_pos = torch.tensor([P - 2, maxp * P - T, 0], dtype=torch.int32)
    assert (P - 2) // P != (P - 2 + T - 1) // P
    c.k_new = _randn_bf(gen, B, Hkv, T, D)
    c.v_new = _randn_bf(gen, B, Hkv, T, D)
    c.k_pool, c.v_pool = model_kv_write(c)
    # untouched slots keep their poison: most of the pool
    assert int((c.k_pool == c.k_pool0).sum()) >= c.k_pool.numel() - B * T * Hkv * D
    return c


KV_MUTATIONS = (
    "kv_v_token_major",
    "kv_page_from_pos_plus_1",
    "kv_head_stride_off",
    "kv_gather_ignores_page_table",
    "kv_gather_second_sweep_missing",
)


def kv_applicable(spec):
    if spec.big:
        return ["kv_gather_ignores_page_table", "kv_gather_second_sweep_missing"]
    out = ["kv_v_token_major", "kv_page_from_pos_plus_1", "kv_gather_ignores_page_table"]
    if spec.Hkv > 1:
        out.append("kv_head_stride_off")
    return out


def model_kv_write(c, mut=None):
    """(k_pool, v_pool) after the write, float64."""
    spec = c.spec
    B, Hkv, D, P, T = spec.B, spec.Hkv, spec.D, spec.P, KV_T
    kp, vp = c.k_pool0.clone(), c.v_pool0.clone()
    k_new, v_new = c.k_new, c.v_new
    if mut == "kv_head_stride_off":
        # the source read as (B, T, Hkv, D)
        k_new = k_new.reshape(B, T, Hkv, D).permute(0, 2, 1, 3)
        v_new = v_new.reshape(B, T, Hkv, D).permute(0, 2, 1, 3)
    vp_tm = vp.view(-1, Hkv, P, D)                       # the same memory, token-major
    for b in range(B):
        for t in range(T):
            pos = int(c.start_pos[b]) + t
            pidx = (pos + 1) // P if mut == "kv_page_from_pos_plus_1" else pos // P
            page = int(c.page_table[b, min(pidx, spec.maxp - 1)])
            slot = pos % P
            kp[page, :, slot, :] = k_new[b, :, t, :]
            if mut == "kv_v_token_major":
                vp_tm[page, :, slot, :] = v_new[b, :, t, :]
            else:
                vp[page, :, :, slot] = v_new[b, :, t, :]
    return kp, vp


def model_kv_gather(c, ctx, batch_index, mut=None):
    """dense (Hkv, ctx, D) k and v of one sequence, float64."""
    spec = c.spec
    Hkv, D, P = spec.Hkv, spec.D, spec.P
    k = torch.empty(Hkv, ctx, D, dtype=torch.float64)
    v = torch.empty(Hkv, ctx, D, dtype=torch.float64)
    for pos in range(ctx):
        if mut == "kv_gather_ignores_page_table":
            page = batch_index * spec.maxp + pos // P
        else:
            page = int(c.page_table[batch_index, pos // P])
        k[:, pos, :] = c.k_pool[page, :, pos % P, :]
        v[:, pos, :] = c.v_pool[page, :, :, pos % P]
    if mut == "kv_gather_second_sweep_missing":
        # vector i = (pos * Hkv + h) * (D / 8) + d / 8 past the first sweep
        lim = FLAT_GRID_CAP * 256
        for t in (k, v):
            tv = t.permute(1, 0, 2).reshape(ctx * Hkv * (D // 8), 8)   # a copy
            tv[lim:] = float("nan")
            t.copy_(tv.reshape(ctx, Hkv, D).permute(1, 0, 2))
    return k, v


# ---------------------------------------------------------------------------
# quant4
# ---------------------------------------------------------------------------

GS = 64


@dataclass(frozen=True)
class PackSpec:
    name: str
    kind: str
    seed: int = 0


PACK_SPECS = (
    PackSpec("pack-designed-5-groups", "designed", 1),        # 4k + 1 groups
    PackSpec("pack-ranges-3x5-groups", "ranges", 2),          # 4k + 3 groups
    PackSpec("pack-randn-7x256", "randn", 3),
    PackSpec("pack-large-2x192", "large", 4),
)


@functools.lru_cache(maxsize=None)
def build_pack(spec):
    c = Case(spec)
    gen = _gen(900 + spec.seed)
    if spec.kind == "designed":
        rows = []
        rows.append(torch.full((GS,), 3.25))                              # constant
        rows.append((torch.arange(GS) % 31).float())                      # 0..30: .5 ties
        g = torch.rand(GS, generator=gen) * 2 - 1
        g[0], g[63] = -4.0, 5.0                                           # min lane 0, max lane 63
        rows.append(g)
        g = torch.rand(GS, generator=gen) * 2 - 1
        g[0], g[63] = 6.0, -3.0                                           # max lane 0, min lane 63
        rows.append(g)
        rows.append(-(torch.rand(GS, generator=gen) * 7 + 1))             # negative only
        x = torch.cat(rows)[None]                                         # (1, 320)
    elif spec.kind == "ranges":
        # every group its own range and offset, so row and group index matter
        x = torch.rand(3, 5, GS, generator=gen)
        span = 2.0 ** torch.arange(-3, 12).float().reshape(3, 5, 1)
        off = (torch.arange(15).float().reshape(3, 5, 1) - 7) * 3
        x = (x * span + off).reshape(3, 5 * GS)
    elif spec.kind == "randn":
        x = torch.randn(7, 256, generator=gen)
    else:
        x = (torch.rand(2, 192, generator=gen) * 2 - 1) * 3e4
        x[0, 5], x[1, 70] = 3e4, -3e4
    c.x = x.to(BF)
    assert float(c.x.float().abs().max()) <= 30080.0                      # bf16(3e4)
    c.want = model_pack(c)
    return c


PACK_MUTATIONS = ("q4_nibbles_swapped", "q4_group_of_32", "q4_divisor_16",
                  "q4_truncation")
UNPACK_MUTATIONS = ("q4_unpack_nibbles_swapped", "q4_neighbour_group_scale_zero",
                    "q4_unpack_second_sweep_missing")


def pack_applicable(spec):
    return list(PACK_MUTATIONS)


def model_pack(c, mut=None):
    """(packed (rows, cols/2) u8, scale, zero (rows, cols/64) f16). Written in
    f32: the op is defined by these roundings (module docstring)."""
    x = c.x.float()
    R, C = x.shape
    gs = 32 if mut == "q4_group_of_32" else GS
    g = x.reshape(R, C // gs, gs)
    mn = g.min(dim=2, keepdim=True).values
    mx = g.max(dim=2, keepdim=True).values
    sc = torch.maximum(mx - mn, torch.tensor(1e-8)) / (16.0 if mut == "q4_divisor_16" else 15.0)
    t = (g - mn) / sc
    q = torch.floor(t) if mut == "q4_truncation" else torch.round(t)      # half to even
    q = q.clamp(0.0, 15.0).to(torch.uint8).reshape(R, C)
    lo, hi = q[:, 0::2], q[:, 1::2]
    if mut == "q4_nibbles_swapped":
        lo, hi = hi, lo
    packed = lo | (hi << 4)
    scale, zero = sc.squeeze(2).half(), mn.squeeze(2).half()
    if mut == "q4_group_of_32":
        # two half groups share one output slot: the second one's store wins
        scale, zero = scale[:, 1::2].contiguous(), zero[:, 1::2].contiguous()
    return packed.contiguous(), scale, zero


def check_pack(c, got):
    return 0.0 if all(torch.equal(g.cpu().reshape(w.shape), w)
                      for g, w in zip(got, c.want)) else INF


@dataclass(frozen=True)
class UnpackSpec:
    name: str
    rows: int
    cols: int
    exact: bool
    seed: int = 0


UNPACK_SPECS = (
    UnpackSpec("unpack-exact-4x128", 4, 128, True, 1),
    UnpackSpec("unpack-real-5x192", 5, 192, False, 2),
    UnpackSpec("unpack-exact-1025x1088-past-cap", 1025, 1088, True, 3),
    UnpackSpec("unpack-real-1025x1088-past-cap", 1025, 1088, False, 4),
)
assert 1025 * 1088 > UNPACK_GRID_CAP * 256


@functools.lru_cache(maxsize=None)
def build_unpack(spec):
    c = Case(spec)
    gen = _gen(950 + spec.seed)
    R, C = spec.rows, spec.cols
    G = C // GS
    # all 16 codes in both nibbles: byte j of a row holds (j % 16) low and
    # (j * 7 + row) % 16 high, then a random remainder
    j = torch.arange(C // 2)[None] + torch.zeros(R, 1, dtype=torch.long)
    lo = (j + torch.arange(R)[:, None]) % 16
    hi = (j * 7 + 3 * torch.arange(R)[:, None]) % 16
    c.packed = (lo | (hi << 4)).to(torch.uint8)
    if spec.exact:
        c.scale = (2.0 ** _ri(-2, 2, (R, G), gen)).half()
        c.zero = _ri(-8, 8, (R, G), gen).half()
    else:
        c.scale = (torch.rand(R, G, generator=gen) * 0.05 + 1e-3).half()
        c.zero = (torch.randn(R, G, generator=gen) * 0.3).half()
    c.want = model_unpack(c)
    if spec.exact:
        assert is_bf16(c.want)                               # |15 * 4 + 8| = 68: 7 bits
    seen = {(int(b) & 15, int(b) >> 4) for b in c.packed[0, :32].tolist()}
    assert {a for a, _ in seen} == set(range(16)) == {b for _, b in seen}
    return c


def unpack_applicable(spec):
    out = ["q4_unpack_nibbles_swapped", "q4_neighbour_group_scale_zero"]
    if spec.rows * spec.cols > UNPACK_GRID_CAP * 256:
        out.append("q4_unpack_second_sweep_missing")
    return out


def model_unpack(c, mut=None):
    R, C = c.spec.rows, c.spec.cols
    lo, hi = (c.packed & 0xF).double(), (c.packed >> 4).double()
    if mut == "q4_unpack_nibbles_swapped":
        lo, hi = hi, lo
    q = torch.stack([lo, hi], dim=2).reshape(R, C // GS, GS)
    s, z = c.scale.double(), c.zero.double()
    if mut == "q4_neighbour_group_scale_zero":
        s, z = s.reshape(-1).roll(-1).reshape(s.shape), z.reshape(-1).roll(-1).reshape(z.shape)
    out = (q * s[..., None] + z[..., None]).reshape(R, C)
    if mut == "q4_unpack_second_sweep_missing":
        out.reshape(-1)[UNPACK_GRID_CAP * 256:] = float("nan")
    return out


def unpack_bound(c):
    return 2.0 ** -8 * c.want.abs() + U * c.want.abs()


def check_unpack(c, got):
    if c.spec.exact:
        return exact_ratio(got, c.want)
    return worst_ratio(got, c.want, unpack_bound(c))
