"""Shared inputs, models and mutations for the exact-arithmetic GEMM tests
(test_gemm_cases_cpu.py and test_gpu_gemm_exact.py). Plain helper module.

Why exact. If A, W, bias and residual are small integers (or small integers
times a power of two), every product a*w and every f32 partial sum is exact
in ANY summation order, and the single bf16 rounding at the end is exact
too. A kernel must then reproduce the expected tensor bit for bit
(`torch.equal`), and a dropped, duplicated or misplaced k-slice, row,
column, stripe, split, expert or quantisation group shows as an error of
at least one whole unit.

Three things live here:

* `build(spec)`: a deterministic, cached CPU case (dense / fused-norm / W4 /
  MoE). Inputs are DENSE and cancel in pairs: a random perfect matching of
  the K columns pairs k with k'; W[:, k'] = -W[:, k] and A[:, k'] = A[:, k]
  + delta with delta a sparse +-1 perturbation (on W instead where A is
  constrained, i.e. the norm cases). The result is -sum(delta * W): small,
  non-zero almost everywhere, while every k-slice carries large terms that
  must cancel exactly. The matching is random (not k <-> k + K/2) so a
  defect that recurs in every stage or split cannot cancel against itself.
  Rows past M of the A buffer, A rows no rowmap entry names and the weights
  of empty experts hold poison (+-2^10).
* `model(case, mut=None)`: an fp64 CPU model of the operation, written out
  directly (matmul, norm scale, epilogue), with one knob per defect.
* `MUTATIONS` / `applicable(spec)`: which defect applies to which case.

Builder invariants, asserted for EVERY case in `build`:
  - expected.to(bfloat16).double() == expected (for integers: |x| <= 256),
    so a one-unit error can never be rounded away;
  - sum_k |a*w| per output, in units of the smallest power of two in play,
    is below 2^24, so every f32 partial sum is exact in any order.

Norm cases. Every entry of A row m is +-2^j(m); eps = 0 and the norm weight
entries are powers of two. Then ss/K = 4^j exactly, invr = 2^-j, and the
result is again exactly representable. A few-ulp error in the device's
rsqrtf moves the pre-rounding value by a few 2^-24 relative and still
rounds to the same bf16, except where the expected value is exactly 0 (a
residue x*eps would survive there). The cases do not avoid zeros: the
device's rsqrt of a power of four is exact, and the GPU tests passing with
2-6 % zeros in the norm cases is what shows it. With `ss_in` the stripes are unequal
multiples of 1/16, different per stripe and per row, that sum to K*4^j'
with j' != j on odd rows: the expected output follows ss_in and not A.

Realistic-valued complement (exact data cannot see lost accumulator
precision): test_gpu_gemm_exact.py runs one randn case per kernel against
fp64; the bound is derived, not chosen:
    |got - want| <= 2^-8 |want| + K 2^-24 sum|a w|
    (+ 2^-8 sum|a^ w| for the bf16 staging of the normalised A in mode 1,
     + 2^-10 sum|a w| for the f16 dequant of W4).
2^-8 |want| is the strict bound of one bf16 rounding; K 2^-24 sum|a w| is
the classical bound for a length-K f32 sum in any order. Worst observed
ratio |err| / bound on an MI355X, against the fp64 reference:
    gemm_skinny  v1 0.950   v2 0.899   v2 split-K 0.882   v2 split-K with
                 the vectorised combine 0.947   mode 1 0.207   mode 2 0.869
    moe_gemm     v1 0.980   v2 0.923
    gemm_w4      MFMA split-K 0.421   GEMV 0.139
    gelu_tanh    0.996 (its own bound, see test_gelu_tanh_parity)
Where no extra term applies the ratio is set by the final bf16 rounding,
whose strict bound a value just above a power of two nearly reaches; an
fp64 matmul rounded once to bf16 gives the same figures to three digits, so
the kernels lose nothing measurable in the accumulation.
"""
import functools
from dataclasses import dataclass
from typing import Tuple

import torch

POISON = 1024.0
BF = torch.bfloat16


# ---------------------------------------------------------------------------
# specs
# ---------------------------------------------------------------------------

@dataclass(frozen=True)
class Spec:
    name: str
    kind: str                 # "dense" | "norm" | "w4" | "moe"
    M: int = 1
    N: int = 64
    K: int = 256
    ksplit: int = 1           # as passed to the op (0 = the op's own rule)
    bias: bool = False
    res: bool = False
    mode: int = 0             # norm cases: 1 (nw staged) or 2 (nw folded into W)
    ss_in: int = 0            # norm cases: number of producer stripes (0: none)
    ss_out: bool = False
    batch3: bool = False      # input shaped (M, 1, K)
    # moe
    counts: Tuple[int, ...] = ()
    extra_chunks: int = 0     # mchunks = exact + extra_chunks
    rowmap: bool = False
    scale: bool = False
    seed: int = 0


def ids(specs):
    return [s.name for s in specs]


class Case:
    def __init__(self, spec):
        self.spec = spec


# ---------------------------------------------------------------------------
# host-side launch geometry (mirrors ext.hip; used only by the mutations and
# by the tests that state which path a case reaches — never by `want`)
# ---------------------------------------------------------------------------

def skinny_is_v2(K):
    return K % 256 == 0


def skinny_splits(N, K, ksplit):
    """[(k0, k1)] per launched split of gemm_skinny, empty ones included."""
    if ksplit <= 0:
        ksplit = 1 if N // 64 >= 256 else min(K // 512, max(1, min(8, 1024 // (N // 64))))
        ksplit = max(1, ksplit)
    if skinny_is_v2(K):
        nch = K // 256
        per = -(-nch // ksplit)
        ksplit = -(-nch // per)
        kchunk = per * 256
    else:
        kchunk = -(-(K // 32) // ksplit) * 32
    return [(s * kchunk, max(s * kchunk, min(K, (s + 1) * kchunk)))
            for s in range(ksplit)]


def w4_is_gemv(M, K):
    return M == 1 and K % 2048 == 0 and K // 2048 <= 7


def w4_splits(M, N, K, ksplit):
    if w4_is_gemv(M, K):
        return [(0, K)]
    if ksplit <= 0:
        ksplit = max(1, min(K // 512, 1792 // max(1, (N + 63) // 64)))
    nch = K // 128
    per = -(-nch // ksplit)
    ksplit = -(-nch // per)
    return [(s * per * 128, min(K, (s + 1) * per * 128)) for s in range(ksplit)]


def splits_of(spec):
    if spec.kind == "w4":
        return w4_splits(spec.M, spec.N, spec.K, spec.ksplit)
    if spec.kind == "moe":
        return [(0, spec.K)]
    return skinny_splits(spec.N, spec.K, spec.ksplit)


def xcd_remap(nwg):
    """tile index owned by block b (gemm_skinny_v2 / w4 / moe kernels)."""
    q, r = divmod(nwg, 8)
    out = []
    for b in range(nwg):
        xcd, orig8 = b % 8, b // 8
        t = b
        if nwg >= 8:
            t = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + orig8
        out.append(t)
    return out


def has_remap(spec):
    if spec.kind in ("dense", "norm") and not skinny_is_v2(spec.K):
        return False
    if spec.kind == "w4" and w4_is_gemv(spec.M, spec.K):
        return False
    nwg = spec.N // 64
    return xcd_remap(nwg) != list(range(nwg))


def exact_mchunks(counts):
    return max(1, -(-max(counts) // 32))


# ---------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------

def _gen(spec):
    return torch.Generator().manual_seed(7000 + spec.seed)


def _matching(K, gen):
    perm = torch.randperm(K, generator=gen)
    return perm[0::2], perm[1::2]


def _ri(lo, hi, shape, gen):
    """integers in [lo, hi] as float64"""
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def _sparse_pm1(shape, density, gen):
    hit = torch.rand(shape, generator=gen) < density
    sign = _ri(0, 1, shape, gen) * 2 - 1
    return sign * hit


def _poisoned_rows(A, pad, gen):
    """A (M, K) on top of `pad` extra rows of +-POISON; returns the buffer."""
    M, K = A.shape
    buf = torch.empty(M + pad, K, dtype=torch.float64)
    buf[:M] = A
    buf[M:] = (_ri(0, 1, (pad, K), gen) * 2 - 1) * POISON
    return buf


def _epilogue_inputs(c, spec, gen, bmax, rmax, unit=None):
    """integer bias (N,) and residual (M, N), optionally times unit[n]."""
    M, N = spec.M, spec.N
    u = torch.ones(N, dtype=torch.float64) if unit is None else unit
    c.bias = _ri(-bmax, bmax, (N,), gen) * u if spec.bias else None
    c.res = _ri(-rmax, rmax, (M, N), gen) * u if spec.res else None


def _build_dense(spec, gen):
    c = Case(spec)
    M, N, K = spec.M, spec.N, spec.K
    ka, kb = _matching(K, gen)
    W = torch.zeros(N, K, dtype=torch.float64)
    W[:, ka] = _ri(-2, 2, (N, K // 2), gen)
    W[:, kb] = -W[:, ka]
    A = torch.zeros(M, K, dtype=torch.float64)
    A[:, ka] = _ri(-2, 2, (M, K // 2), gen)
    A[:, kb] = A[:, ka] + _sparse_pm1((M, K // 2), max(1 / 16, 8 / K), gen)
    c.Abuf = _poisoned_rows(A, 3, gen)
    c.W = W
    _epilogue_inputs(c, spec, gen, 32, 64)
    c.unit = 1.0
    return c


def _build_norm(spec, gen):
    """A[m, :] = +-2^j(m); the perturbation sits on W; nw in {1, 2} per pair.
    c.W is the plain weight, c.Wfold = W * nw (what mode 2 is given)."""
    c = Case(spec)
    M, N, K = spec.M, spec.N, spec.K
    assert K % 256 == 0 and spec.mode in (1, 2)
    ka, kb = _matching(K, gen)
    j = torch.tensor([(-1, 0, 1, 2)[(m * 3 + m // 4) % 4] for m in range(M)])
    sgn = _ri(0, 1, (M, K // 2), gen) * 2 - 1
    A = torch.zeros(M, K, dtype=torch.float64)
    A[:, ka] = sgn * (2.0 ** j.double())[:, None]
    A[:, kb] = A[:, ka]
    W = torch.zeros(N, K, dtype=torch.float64)
    W[:, ka] = _ri(-2, 2, (N, K // 2), gen)
    W[:, kb] = -W[:, ka] + _sparse_pm1((N, K // 2), 1 / 32, gen)
    nw = torch.zeros(K, dtype=torch.float64)
    nw[ka] = 2.0 ** _ri(0, 1, (K // 2,), gen)
    nw[kb] = nw[ka]
    c.j = j
    c.Abuf = _poisoned_rows(A, 3, gen)
    c.W, c.nw, c.Wfold = W, nw, W * nw
    c.ss_in = None
    c.jin = j.clone()
    if spec.ss_in:
        ns = spec.ss_in
        c.jin = j + (torch.arange(M) % 2)            # j' != j on odd rows
        tot16 = (K * 4.0 ** c.jin.double() * 16).long()      # units of 1/16
        base = tot16 // ns
        assert int(base.min()) >= 4
        st = base[None, :].repeat(ns, 1)
        for m in range(M):
            b = int(base[m])
            d = torch.randperm(b - 1, generator=gen)[: ns // 2] + 1
            if ns // 2 > b - 1:                      # fewer distinct offsets than pairs
                d = torch.randint(1, b, (ns // 2,), generator=gen)
            st[0:2 * (ns // 2):2, m] += d
            st[1:2 * (ns // 2):2, m] -= d
            st[ns - 1, m] += tot16[m] - base[m] * ns
        assert bool((st.sum(0) == tot16).all()) and bool((st > 0).all())
        ss = torch.full((ns, 32), POISON * POISON, dtype=torch.float64)
        ss[:, :M] = st.double() / 16
        c.ss_in = ss
    _epilogue_inputs(c, spec, gen, 4, 8)
    c.unit = 0.5
    return c


W4_TAU = (1.0, 2.0, 4.0)


def _build_w4(spec, gen):
    """codes, scale and zero built directly in quant4_pack layout.
    scale[n, g] = sigma[n] * tau[g], tau = (1, 2, 4)[g % 3]: the two groups
    of every 128-k slice differ and so do neighbouring slices. z0[n, g] in
    {7, 8} independent of the scale; zero = -z0 * scale. w = (q - z0) * scale.
    A pair (k, k') across groups of different tau is balanced by the
    power-of-two factor tau[g] / tau[g'] on the A side (exact in f16)."""
    c = Case(spec)
    M, N, K = spec.M, spec.N, spec.K
    G = K // 64
    ka, kb = _matching(K, gen)
    ga, gb = ka // 64, kb // 64
    tau = torch.tensor([W4_TAU[g % 3] for g in range(G)], dtype=torch.float64)
    sigma = 2.0 ** _ri(0, 1, (N,), gen)
    z0 = _ri(7, 8, (N, G), gen)
    q = torch.zeros(N, K, dtype=torch.float64)
    q[:, ka] = _ri(1, 14, (N, K // 2), gen)
    q[:, kb] = z0[:, ga] + z0[:, gb] - q[:, ka]       # q' - z0' = -(q - z0)
    assert 0 <= float(q.min()) and float(q.max()) <= 15
    A = torch.zeros(M, K, dtype=torch.float64)
    A[:, ka] = _ri(-2, 2, (M, K // 2), gen)
    delta = torch.zeros(M, K // 2, dtype=torch.float64)
    npert = 6
    for m in range(M):
        at = torch.randperm(K // 2, generator=gen)[:npert]
        delta[m, at] = _ri(0, 1, (npert,), gen) * 2 - 1
    A[:, kb] = A[:, ka] * (tau[ga] / tau[gb])[None, :] + delta
    c.Abuf = _poisoned_rows(A, 3, gen)
    c.q = q.to(torch.uint8)
    c.scale = sigma[:, None] * tau[None, :]
    c.z0 = z0
    c.zero = -z0 * c.scale
    c.packed = (c.q[:, 0::2] | (c.q[:, 1::2] << 4)).contiguous()   # (N, K/2)
    c.W = w4_dequant(c)
    _epilogue_inputs(c, spec, gen, 16, 32)
    c.unit = 0.25
    return c


def w4_dequant(c, mut=None):
    """(N, K) fp64 weight from codes/scale/zero, with the W4 defects."""
    N, K = c.spec.N, c.spec.K
    q = c.q.double()
    if mut == "w4_nibble_swap":
        q = q.reshape(N, K // 2, 2).flip(-1).reshape(N, K)
    g = torch.arange(K) // 64
    gs = gz = g
    if mut == "w4_scale_neighbour":
        gs = g ^ 1
    if mut == "w4_zero_neighbour":
        gz = g ^ 1
    if mut == "w4_group_straddle":
        gs = gz = torch.arange(K) // 128
    return q * c.scale[:, gs] + c.zero[:, gz]


def _build_moe(spec, gen):
    c = Case(spec)
    N, K, counts = spec.N, spec.K, spec.counts
    E, S = len(counts), sum(counts)
    ka, kb = _matching(K, gen)
    W = torch.zeros(E, N, K, dtype=torch.float64)
    W[:, :, ka] = _ri(-2, 2, (E, N, K // 2), gen)
    W[:, :, kb] = -W[:, :, ka]
    for e, n in enumerate(counts):
        if n == 0:
            W[e] = (_ri(0, 1, (N, K), gen) * 2 - 1) * POISON
    off = torch.zeros(E + 1, dtype=torch.int32)
    off[1:] = torch.tensor(counts).cumsum(0).int()
    if spec.rowmap:
        Ta = S // 2 + 5
        named = torch.tensor([t for t in range(Ta) if t % 5 != 2])
        rm = named[torch.randint(0, len(named), (S,), generator=gen)].int()
        assert len(set(rm.tolist())) < S            # repeated tokens
    else:
        Ta, rm = S + 3, None
    A = torch.zeros(Ta, K, dtype=torch.float64)
    A[:, ka] = _ri(-2, 2, (Ta, K // 2), gen)
    A[:, kb] = A[:, ka] + _sparse_pm1((Ta, K // 2), max(1 / 16, 8 / K), gen)
    used = torch.zeros(Ta, dtype=torch.bool)
    used[rm.long() if rm is not None else torch.arange(S)] = True
    A[~used] = (_ri(0, 1, (int((~used).sum()), K), gen) * 2 - 1) * POISON
    c.A, c.W, c.off, c.rowmap = A, W, off, rm
    c.E, c.S = E, S
    # distinct power of two among any 61 consecutive slots
    c.scale = (2.0 ** ((torch.arange(S) * 23 % 61) - 30).double()
               if spec.scale else None)
    c.mchunks = exact_mchunks(counts) + spec.extra_chunks
    c.unit = 1.0
    return c


_BUILDERS = {"dense": _build_dense, "norm": _build_norm, "w4": _build_w4,
             "moe": _build_moe}


@functools.lru_cache(maxsize=None)
def build(spec):
    c = _BUILDERS[spec.kind](spec, _gen(spec))
    c.want = model(c)
    check_invariants(c)
    return c


def abs_products(c):
    """sum_k |a| |w| per output (before any norm or slot scale)."""
    spec = c.spec
    if spec.kind == "moe":
        out = torch.zeros(c.S, spec.N, dtype=torch.float64)
        for e in range(c.E):
            a, b = int(c.off[e]), int(c.off[e + 1])
            if b > a:
                rows = c.rowmap[a:b].long() if c.rowmap is not None else torch.arange(a, b)
                out[a:b] = c.A[rows].abs() @ c.W[e].abs().T
        return out
    W = c.Wfold if spec.kind == "norm" else c.W
    return c.Abuf[:spec.M].abs() @ W.abs().T


def out_unit(c):
    """One unit of each expected element: the step below which no defect of
    whole k-slices, rows, stripes or groups can hide (broadcasts to want)."""
    u = {"dense": 1.0, "norm": 0.5, "w4": 1.0, "moe": 1.0}[c.spec.kind]
    if c.spec.kind == "moe" and c.scale is not None:
        return u * c.scale[:, None]
    return torch.tensor(u, dtype=torch.float64)


def check_invariants(c):
    want = c.want
    assert bool((want.to(BF).double() == want).all()), \
        f"{c.spec.name}: expected output is not exactly representable in bf16"
    # smallest power of two any product is a multiple of
    unit = c.unit
    assert float(abs_products(c).max()) / unit < 2 ** 24, \
        f"{c.spec.name}: partial sums may be inexact in f32"
    if c.spec.ss_out:
        assert float(c.want_ss.max()) / (unit * unit) < 2 ** 24


# ---------------------------------------------------------------------------
# fp64 model with one knob per defect
# ---------------------------------------------------------------------------

MUTATIONS = (
    "drop_last_slice", "drop_stage_head", "last_split_lost", "row_clamp16",
    "row_past_M", "stripe_unremapped", "bias_by_row", "residual_wrong_stripe",
    "invr_neighbour_row", "ss_in_ignored", "ss_stripe_tail_lost",
    "ssout_wave_lost",
    "expert_next", "rowmap_ignored", "scale_by_local_m",
    "chunk_rows_from_first", "group_end_plus_one",
    "w4_scale_neighbour", "w4_zero_neighbour", "w4_nibble_swap",
    "w4_group_straddle",
)


def _kmask(spec, mut):
    K = spec.K
    keep = torch.ones(K, dtype=torch.float64)
    live = [(a, b) for a, b in splits_of(spec) if b > a]
    if mut == "drop_last_slice":           # last 32 k of the last live split
        keep[live[-1][1] - 32: live[-1][1]] = 0
    if mut == "drop_stage_head":           # first 128 k of the second 256-stage
        a = live[0][0]
        keep[a + 256: a + 384] = 0
    if mut == "last_split_lost":
        keep[live[-1][0]: live[-1][1]] = 0
    return keep


def _unremap(acc, spec):
    """accumulator lands in stripe blockIdx.x instead of the remapped tile."""
    tiles = xcd_remap(spec.N // 64)
    out = torch.empty_like(acc)
    for b, t in enumerate(tiles):
        out[:, b * 64:(b + 1) * 64] = acc[:, t * 64:(t + 1) * 64]
    return out


def model(c, mut=None):
    """Expected output in fp64; `mut` applies one defect. For ss_out cases
    the per-stripe row sums of squares are left in c.want_ss / returned by
    model_ss."""
    if c.spec.kind == "moe":
        return _model_moe(c, mut)
    out, ss = _model_gemm(c, mut)
    if mut is None and c.spec.ss_out:
        c.want_ss = ss
    return out


def model_ss(c, mut=None):
    return _model_gemm(c, mut)[1]


def _model_gemm(c, mut):
    spec = c.spec
    M, N, K = spec.M, spec.N, spec.K
    rows = torch.arange(M)
    if mut == "row_clamp16":
        rows = torch.where(rows >= 16, torch.full_like(rows, 15), rows)
    if mut == "row_past_M":
        rows = rows.clone()
        rows[M - 1] = M                    # first poison row of the buffer
    A = c.Abuf[rows]
    if spec.kind == "w4":
        W = w4_dequant(c, mut)
    elif spec.kind == "norm":
        W = c.Wfold
    else:
        W = c.W
    acc = (A * _kmask(spec, mut)) @ W.T
    if spec.kind == "norm":
        if c.ss_in is not None and mut != "ss_in_ignored":
            ss = c.ss_in
            if mut == "ss_stripe_tail_lost":
                ss = ss[: (spec.ss_in // 32) * 32]
            tot = ss.sum(0)[:M]
        else:
            tot = (c.Abuf[:M] ** 2).sum(1)
        invr = 1.0 / torch.sqrt(tot / K)   # eps = 0
        if mut == "invr_neighbour_row":
            invr = invr.roll(-1)
        acc = acc * invr[:, None]
    if mut == "stripe_unremapped":
        acc = _unremap(acc, spec)
    v = acc
    if c.bias is not None:
        v = v + (c.bias[torch.arange(M) % N][:, None] if mut == "bias_by_row"
                 else c.bias[None, :])
    if c.res is not None:
        v = v + (c.res.roll(-64, 1) if mut == "residual_wrong_stripe" else c.res)
    sq = (v * v).reshape(M, N // 64, 64)
    if mut == "ssout_wave_lost":
        sq = sq[:, :, :48]
    return v, sq.sum(-1).T.contiguous()    # ss: (N/64, M)


def _model_moe(c, mut):
    spec = c.spec
    N, K, E, S = spec.N, spec.K, c.E, c.S
    keep = _kmask(spec, mut)
    Ta = c.A.shape[0]
    out = torch.zeros(S, N, dtype=torch.float64)

    def row_of(s):
        if c.rowmap is None or mut == "rowmap_ignored":
            return s % Ta
        return int(c.rowmap[s])

    for e in range(E):
        base, end = int(c.off[e]), int(c.off[e + 1])
        cnt = end - base
        W = c.W[(e + 1) % E] if mut == "expert_next" else c.W[e]
        for m in range(cnt):
            src = m % 32 if mut == "chunk_rows_from_first" else m
            acc = (c.A[row_of(base + src)] * keep) @ W.T
            if c.scale is not None:
                acc = acc * c.scale[m if mut == "scale_by_local_m" else base + m]
            out[base + m] = acc
    if mut == "group_end_plus_one":
        # expert e also computes the slot after its group with ITS weights;
        # the model lets that stray write win over the rightful owner's
        for e in range(E):
            base, end = int(c.off[e]), int(c.off[e + 1])
            if end > base and end < S:
                acc = (c.A[row_of(end)] * keep) @ c.W[e].T
                if c.scale is not None:
                    acc = acc * c.scale[end]
                out[end] = acc
    if mut == "stripe_unremapped":
        out = _unremap(out, spec)
    return out


def applicable(spec):
    """Mutations that must move the expected output of this case."""
    live = [(a, b) for a, b in splits_of(spec) if b > a]
    names = ["drop_last_slice"]
    if live[0][1] - live[0][0] >= 512:
        names.append("drop_stage_head")
    if len(live) >= 2:
        names.append("last_split_lost")
    if has_remap(spec):
        names.append("stripe_unremapped")
    if spec.kind == "moe":
        names.append("expert_next")
        if spec.rowmap:
            names.append("rowmap_ignored")
        if spec.scale and any(spec.counts[:-1]):
            names.append("scale_by_local_m")
        if max(spec.counts) > 32:
            names.append("chunk_rows_from_first")
        if _spills(spec.counts):
            names.append("group_end_plus_one")
        return names
    names.append("row_past_M")
    if spec.M > 16:
        names.append("row_clamp16")
    if spec.bias:
        names.append("bias_by_row")
    if spec.res and spec.N >= 128:
        names.append("residual_wrong_stripe")
    if spec.kind == "norm":
        if spec.M > 1:
            names.append("invr_neighbour_row")
        if spec.ss_in and spec.M > 1:
            names.append("ss_in_ignored")
        if spec.ss_in > 32 and spec.ss_in % 32:
            names.append("ss_stripe_tail_lost")
    if spec.ss_out:
        names.append("ssout_wave_lost")
    if spec.kind == "w4":
        names += ["w4_scale_neighbour", "w4_zero_neighbour", "w4_nibble_swap",
                  "w4_group_straddle"]
    return names


def _spills(counts):
    S = sum(counts)
    end = 0
    for n in counts:
        end += n
        if n > 0 and end < S:
            return True
    return False


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------

def _d(name, M, N, K, ks, **kw):
    return Spec(name, "dense", M, N, K, ks, **kw)


# gemm_skinny v1 (K % 256 != 0). (K=96, ksplit=8) launches five empty splits.
SKINNY_V1 = [
    _d("v1-m1-n64-k32", 1, 64, 32, 1, seed=1),
    _d("v1-m15-n256-k96-ks8-empty-splits", 15, 256, 96, 8, bias=True, res=True, seed=2),
    _d("v1-m16-n576-k160-ks2", 16, 576, 160, 2, res=True, seed=3),
    _d("v1-m17-n704-k416-ks3", 17, 704, 416, 3, bias=True, seed=4),
    _d("v1-m31-n512-k416", 31, 512, 416, 1, bias=True, res=True, seed=5),
    _d("v1-m32-n960-k160-ks3", 32, 960, 160, 3, bias=True, res=True, seed=6),
    _d("v1-m32-n1472-k96-ks2", 32, 1472, 96, 2, seed=7),
    _d("v1-m17-n64-k32-ks2-one-empty", 17, 64, 32, 2, res=True, seed=8),
    _d("v1-m16-n256-k416-ks8-ssout", 16, 256, 416, 8, res=True, ss_out=True, seed=9),
]

# gemm_skinny v2 (K % 256 == 0). N/64 in {9, 11, 15, 23}: XCD remap, r != 0.
SKINNY_V2 = [
    _d("v2-m1-n64-k256", 1, 64, 256, 1, bias=True, res=True, seed=11),
    _d("v2-m15-n576-k512-remap-r1", 15, 576, 512, 1, bias=True, res=True, seed=12),
    _d("v2-m16-n704-k768-ks2-uneven-remap-r3", 16, 704, 768, 2, bias=True, res=True, seed=13),
    _d("v2-m17-n960-k1280-ks3-remap-r7", 17, 960, 1280, 3, res=True, seed=14),
    _d("v2-m31-n1472-k1280-ks5-remap-r7", 31, 1472, 1280, 5, bias=True, seed=15),
    _d("v2-m32-n512-k768-ks0", 32, 512, 768, 0, bias=True, res=True, seed=16),
    _d("v2-m32-n576-k1280-ks2-remap-r1", 32, 576, 1280, 2, bias=True, res=True, seed=17),
    _d("v2-m16-n256-k512-ks2", 16, 256, 512, 2, seed=18),
    _d("v2-m17-n4096-k512-ks2-vector-combine", 17, 4096, 512, 2, bias=True, res=True, seed=19),
    _d("v2-m4-n704-k512-batch3", 4, 704, 512, 1, res=True, batch3=True, seed=20),
    _d("v2-m15-n576-k768-ssout", 15, 576, 768, 1, bias=True, res=True, ss_out=True, seed=21),
    _d("v2-m32-n704-k512-ssout", 32, 704, 512, 1, res=True, ss_out=True, seed=22),
    _d("v2-m17-n576-k1280-ks3-ssout-combine", 17, 576, 1280, 3, bias=True, res=True,
       ss_out=True, seed=23),
    _d("v2-m32-n4096-k512-ks2-ssout-combine", 32, 4096, 512, 2, res=True, ss_out=True, seed=24),
]


def _n(name, M, N, K, ks, mode, **kw):
    return Spec(name, "norm", M, N, K, ks, mode=mode, **kw)


NORM = [
    _n("norm1-m1-n64-k256", 1, 64, 256, 1, 1, bias=True, res=True, seed=31),
    _n("norm1-m17-n576-k768-ks2", 17, 576, 768, 2, 1, bias=True, res=True, seed=32),
    _n("norm1-m32-n704-k1280-ks0", 32, 704, 1280, 0, 1, res=True, seed=33),
    _n("norm1-m15-n256-k512-ssin9", 15, 256, 512, 1, 1, res=True, ss_in=9, seed=34),
    _n("norm1-m31-n576-k1280-ks3-ssin36", 31, 576, 1280, 3, 1, bias=True, ss_in=36, seed=35),
    _n("norm2-m1-n64-k256", 1, 64, 256, 1, 2, bias=True, res=True, seed=36),
    _n("norm2-m16-n576-k512", 16, 576, 512, 1, 2, bias=True, res=True, seed=37),
    _n("norm2-m17-n704-k768-ks2", 17, 704, 768, 2, 2, res=True, seed=38),
    _n("norm2-m32-n960-k1280-ks5", 32, 960, 1280, 5, 2, bias=True, res=True, seed=39),
    _n("norm2-m32-n256-k512-ssin1", 32, 256, 512, 1, 2, res=True, ss_in=1, seed=40),
    _n("norm2-m17-n256-k512-ssin8", 17, 256, 512, 2, 2, res=True, ss_in=8, seed=41),
    _n("norm2-m31-n576-k768-ssin9", 31, 576, 768, 1, 2, bias=True, ss_in=9, seed=42),
    _n("norm2-m32-n576-k1280-ks2-ssin36", 32, 576, 1280, 2, 2, res=True, ss_in=36, seed=43),
    _n("norm2-m16-n256-k512-ssin64", 16, 256, 512, 1, 2, res=True, ss_in=64, seed=44),
    _n("norm2-m32-n704-k768-ssin100", 32, 704, 768, 1, 2, bias=True, res=True, ss_in=100, seed=45),
    _n("norm2-m17-n576-k512-ssin36-ssout", 17, 576, 512, 1, 2, res=True, ss_in=36,
       ss_out=True, seed=46),
]


def _w(name, M, N, K, ks, **kw):
    return Spec(name, "w4", M, N, K, ks, **kw)


W4 = [
    _w("w4-gemv-k2048-nloads1", 1, 576, 2048, 0, bias=True, res=True, seed=51),
    _w("w4-gemv-k4096-nloads2", 1, 64, 4096, 0, res=True, seed=52),
    _w("w4-gemv-k14336-nloads7", 1, 704, 14336, 0, bias=True, seed=53),
    _w("w4-m1-k1024-mfma", 1, 576, 1024, 0, bias=True, res=True, seed=54),
    _w("w4-m2-n64-k128", 2, 64, 128, 1, bias=True, res=True, seed=55),
    _w("w4-m2-n576-k2048-ks0", 2, 576, 2048, 0, res=True, seed=56),
    _w("w4-m4-n704-k384-ks2", 4, 704, 384, 2, bias=True, res=True, seed=57),
    _w("w4-m4-n64-k2048-ks3", 4, 64, 2048, 3, bias=True, res=True, seed=58),
    _w("w4-m16-n576-k1024-ks3", 16, 576, 1024, 3, bias=True, res=True, seed=59),
    _w("w4-m17-n704-k384-ks3", 17, 704, 384, 3, res=True, seed=60),
    _w("w4-m17-n64-k1024", 17, 64, 1024, 1, bias=True, res=True, seed=61),
    _w("w4-m32-n576-k2048-ks2", 32, 576, 2048, 2, bias=True, res=True, seed=62),
    _w("w4-m32-n704-k128", 32, 704, 128, 1, bias=True, seed=63),
    _w("w4-m31-n576-k384-ks0", 31, 576, 384, 0, seed=64),
]


def _m(name, N, K, counts, **kw):
    return Spec(name, "moe", N=N, K=K, counts=tuple(counts), **kw)


MOE = [
    _m("moe-e4-k96-n128-first-empty", 128, 96, (0, 33, 1, 17), rowmap=True, scale=True, seed=71),
    _m("moe-e4-k160-n576-last-empty", 576, 160, (65, 16, 32, 0), seed=72),
    _m("moe-e8-k160-n128-chunks-plus2", 128, 160, (1, 0, 70, 17, 0, 64, 33, 16),
       rowmap=True, scale=True, extra_chunks=2, seed=73),
    _m("moe-e8-k96-n576-identity-scale", 576, 96, (32, 33, 0, 0, 65, 1, 16, 0),
       scale=True, seed=74),
    _m("moe-e4-k256-n128-mid-empty", 128, 256, (64, 0, 33, 17), rowmap=True, scale=True, seed=75),
    _m("moe-e4-k768-n576", 576, 768, (0, 70, 16, 1), rowmap=True, extra_chunks=1, seed=76),
    _m("moe-e8-k768-n128-identity", 128, 768, (17, 32, 0, 65, 1, 0, 33, 0), seed=77),
    _m("moe-e8-k256-n576-chunks-plus3", 576, 256, (0, 64, 65, 0, 16, 70, 1, 33),
       rowmap=True, scale=True, extra_chunks=3, seed=78),
]

GEMM_CASES = SKINNY_V1 + SKINNY_V2 + NORM + W4
ALL_CASES = GEMM_CASES + MOE


# ---------------------------------------------------------------------------
# chained case: producer with ss_out -> mode-2 consumer with ss_in + residual
# (the llama block's o_proj -> gate_up pattern)
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def build_chain(M=17, K1=512, N1=768, N2=256, seed=90):
    """Producer h = A1 @ W1^T + R1 with h[m, n] in {+-1, +-3} * 2^j(m) and
    exactly 3/8 of each row at magnitude 3, so sum_n h^2 = 4 N1 4^j and the
    consumer's invr = 2^-(j+1) is exact; which columns carry the 3 is drawn
    per row, so the per-stripe sums differ between stripes and rows. All k
    of the producer but one cancel exactly in pairs; the signal column gives
    t[m] * s[n] * 2^j and R1 adds +-2^(j+1). The consumer's W2 is sparse
    (density 1/8) so that invr * h @ W2^T + R2 stays representable."""
    gen = torch.Generator().manual_seed(seed)
    c = Case(None)
    assert N1 % 8 == 0
    j = torch.tensor([(0, 1, -1, 2)[m % 4] for m in range(M)]).double()
    ka, kb = _matching(K1, gen)
    A1 = torch.zeros(M, K1, dtype=torch.float64)
    W1 = torch.zeros(N1, K1, dtype=torch.float64)
    A1[:, ka] = _ri(-2, 2, (M, K1 // 2), gen)
    A1[:, kb] = A1[:, ka]
    W1[:, ka] = _ri(-2, 2, (N1, K1 // 2), gen)
    W1[:, kb] = -W1[:, ka]
    t = _ri(0, 1, (M,), gen) * 2 - 1
    sg = _ri(0, 1, (N1,), gen) * 2 - 1
    A1[:, ka[0]] = t * 2.0 ** j
    W1[:, ka[0]] = sg
    W1[:, kb[0]] = 0
    ts = t[:, None] * sg[None, :]
    three = torch.zeros(M, N1, dtype=torch.bool)
    for m in range(M):
        three[m, torch.randperm(N1, generator=gen)[: 3 * N1 // 8]] = True
    u = torch.where(three, ts, -ts)
    c.A1buf = _poisoned_rows(A1, 3, gen)
    c.W1 = W1
    c.R1 = 2.0 * u * (2.0 ** j)[:, None]
    c.h = A1 @ W1.T + c.R1
    assert torch.equal(c.h.abs(), torch.where(three, 3.0, 1.0) * (2.0 ** j)[:, None])
    c.ss = (c.h ** 2).reshape(M, N1 // 64, 64).sum(-1).T.contiguous()   # (N1/64, M)
    assert torch.equal(c.ss.sum(0), 4.0 * N1 * 4.0 ** j)
    assert len(set(c.ss[:, 0].tolist())) > 1
    c.W2 = _ri(-2, 2, (N2, N1), gen) * (torch.rand(N2, N1, generator=gen) < 1 / 8)
    c.R2 = _ri(-8, 8, (M, N2), gen)
    invr = 2.0 ** -(j + 1)
    c.want = (c.h @ c.W2.T) * invr[:, None] + c.R2
    assert torch.equal(c.want.to(BF).double(), c.want)
    assert float((A1.abs() @ W1.abs().T).max()) * 4 < 2 ** 24
    c.M = M
    return c


# ---------------------------------------------------------------------------
# realistic-valued complement
# ---------------------------------------------------------------------------

def realistic_bound(want, K, absprod, extra=0.0):
    """2^-8 |want| + K 2^-24 sum|a w| (+ extra): see the module docstring."""
    return 2.0 ** -8 * want.abs() + K * 2.0 ** -24 * absprod + extra
