"""Shared inputs, oracle and mutations for the top-k sparse decode attention
tests (test_sparse_cases_cpu.py and test_gpu_attn_sparse.py). Plain helper
module, in the style of attn_cases.py.

* `build(spec, grow=0)`: a deterministic, cached CPU case. P = 16, the page
  table is a random permutation over a pool with spare pages and every slot
  that holds no live position is finite poison (+-64 in K and V; the K slot
  just past ctx is poison aligned with each group's first query head, so a
  kernel that scores it selects it). `grow` appends that many positions to
  every row and changes nothing else (same q, page table, K/V values), which
  is what the graph-replay test steps through.

* Exact scores. q and K hold integers in {-1, 0, 1}, except q[..., 0] = 1 and
  K[c, 0] = j_c / 256 with j a per-(row, kv head) random permutation of
  distinct integers < 256. With the explicit power-of-two scale every
  product and every partial sum is a multiple of 2^-8 * scale below 2^8:
  exact in f32 in ANY summation order. And the scores of one head are
  pairwise distinct (distinct fractional parts), so there is exactly one
  correct kept set and a kernel must pick it. The tie cases set K[..., 0] = 0:
  integer scores tie heavily and the rule "lowest positions win" decides.
  Rows longer than 256 (the serving-length cases) draw j with repetition:
  scores stay exact, a few of them tie, and the same rule keeps the kept set
  unique.
  ALiBi slopes are not exact; the builder asserts that the fp64 gap between
  the kkeep-th and (kkeep+1)-th score of every head is >= 2^-14, more than
  4 f32 ulps at |s| <= 32.

* `oracle(case)`: fp64, written out directly (gather, score, stable
  descending sort, prefix, softmax, @ v); independent of ops.reference.
  MUTATIONS are that oracle with one deliberate error each.

Tolerance (`tol`), the derivation of attn_cases.py: products are exact, P is
rounded to bf16 before P.V (relative 2^-9) and the output is rounded to bf16
(2^-9), so per (row, head) |err| <= 2^-8 * max|v| over that head's KEPT
positions.
"""
import functools
import math
from dataclasses import dataclass
from typing import Tuple

import torch

P = 16
POISON = 64.0
GROW_MAX = 2
SCALE = {64: 2.0 ** -3, 128: 2.0 ** -4, 256: 2.0 ** -4}


@dataclass(frozen=True)
class Spec:
    name: str
    Hq: int
    Hkv: int
    D: int
    ctxs: Tuple[int, ...]
    sparsity: float
    covers: Tuple[str, ...]            # mutations this case must tell apart
    alibi: bool = False
    tie: bool = False
    seed: int = 0
    pad_pages: int = 0                 # extra (unused) page-table columns


class Case:
    pass


def _bf(x):
    return x.to(torch.bfloat16)


def kkeep_of(sparsity, ctx):
    return max(1, min(ctx, math.ceil(sparsity * ctx)))


@functools.lru_cache(maxsize=None)
def build(spec, grow=0):
    assert 0 <= grow <= GROW_MAX
    c = Case()
    c.spec = spec
    B, Hq, Hkv, D = len(spec.ctxs), spec.Hq, spec.Hkv, spec.D
    G = Hq // Hkv
    c.B, c.G = B, G
    c.scale = SCALE[D]
    c.sparsity = spec.sparsity
    c.ctx = torch.tensor([x + grow for x in spec.ctxs], dtype=torch.int32)
    cap = max(spec.ctxs) + GROW_MAX        # dense length, independent of grow
    gen = torch.Generator().manual_seed(7000 + spec.seed)
    # position ctx always has an entry; pad_pages widens the table (and the
    # kernel's score workspace) without adding positions
    maxp = cap // P + 2 + spec.pad_pages
    npages = B * maxp + 5                  # spare pages nobody owns
    c.maxp = maxp
    c.page_table = (torch.randperm(npages, generator=gen)[: B * maxp]
                    .to(torch.int32).reshape(B, maxp))
    c.slopes = None
    if spec.alibi:
        from bloombee_amd.ops.reference import alibi_slopes
        c.slopes = alibi_slopes(Hq)

    ri = lambda *shape: torch.randint(-1, 2, shape, generator=gen).double()
    q = ri(B, Hq, 1, D)
    k = ri(B, Hkv, cap, D)
    q[..., 0] = 1.0
    for b in range(B):
        for kh in range(Hkv):
            if cap <= 256:
                j = torch.randperm(256, generator=gen)[:cap].double()
            else:           # distinct j run out: exact scores, some ties
                j = torch.randint(0, 256, (cap,), generator=gen).double()
            k[b, kh, :, 0] = 0.0 if spec.tie else j / 256.0
    v = _bf(torch.randn(B, Hkv, cap, D, generator=gen)).double()
    c.q = _bf(q)
    c.k, c.v = k, v           # dense (B, Hkv, cap, D) fp64, live up to ctx[b]
    assert torch.equal(c.q.double(), q) and torch.equal(_bf(k).double(), k)

    def poison(*shape):
        sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
        return _bf(sign * POISON)

    kp = poison(npages, Hkv, P, D)
    vp = poison(npages, Hkv, D, P)
    for b in range(B):
        ctx = int(c.ctx[b])
        pos = torch.arange(ctx)
        pages = c.page_table[b, pos // P].long()
        slots = pos % P
        kp[pages, :, slots, :] = _bf(k[b, :, :ctx].permute(1, 0, 2))
        vp[pages, :, :, slots] = _bf(v[b, :, :ctx].permute(1, 0, 2))
        pg, sl = int(c.page_table[b, ctx // P]), ctx % P
        for kh in range(Hkv):
            sg = torch.where(q[b, kh * G, 0] >= 0, 1.0, -1.0)
            kp[pg, kh, sl, :] = _bf(sg * POISON)
    c.k_pages, c.v_pages = kp, vp

    if spec.alibi:
        for b in range(B):
            ctx = int(c.ctx[b])
            kk = kkeep_of(spec.sparsity, ctx)
            if kk >= ctx:
                continue
            for h in range(Hq):
                s = _scores(c, b, h).sort(descending=True).values
                gap = float(s[kk - 1] - s[kk])
                assert gap >= 2.0 ** -14, (spec.name, grow, b, h, gap)
    return c


def slot_of(case, b, pos):
    """(page, slot) of position pos of row b in the pool."""
    return int(case.page_table[b, pos // P]), pos % P


# ---------------------------------------------------------------------------
# fp64 oracle (+ the knobs the mutations turn)
# ---------------------------------------------------------------------------

def _gather(case, b):
    """K, V of row b through the page table: (Hkv, maxp*P, D) fp64 each."""
    Hkv, D = case.spec.Hkv, case.spec.D
    tbl = case.page_table[b].long()
    N = case.maxp * P
    kall = case.k_pages[tbl].double().permute(1, 0, 2, 3).reshape(Hkv, N, D)
    vall = case.v_pages[tbl].double().permute(1, 0, 3, 2).reshape(Hkv, N, D)
    return kall, vall


def _scores(case, b, h, use_alibi=True):
    ctx = int(case.ctx[b])
    kall, _ = _gather(case, b)
    s = (kall[h // case.G, :ctx] @ case.q[b, h, 0].double()) * case.scale
    if case.slopes is not None and use_alibi:
        s = s + case.slopes[h].double() * torch.arange(ctx, dtype=torch.float64)
    return s


def _kkeep_f32(sparsity, ctx):
    prod = torch.tensor(sparsity, dtype=torch.float32) * \
        torch.tensor(float(ctx), dtype=torch.float32)
    return max(1, min(ctx, math.ceil(float(prod))))


def oracle(case, dk=0, floor=False, f32=False, first_head=False,
           no_alibi=False, drop_last_page=False, ties_high=False,
           with_kept=False):
    """(B, Hq, 1, D) fp64. All-default arguments give the true result.

    dk:             kkeep + dk
    floor:          floor instead of ceil
    f32:            sparsity * ctx computed in float32
    first_head:     selection by the scores of the kv group's first head
    no_alibi:       selection ignores the ALiBi term
    drop_last_page: the positions of the last page cannot be selected
    ties_high:      ties at the threshold go to the highest positions
    """
    spec = case.spec
    B, Hq, D, G = case.B, spec.Hq, spec.D, case.G
    out = torch.zeros(B, Hq, 1, D, dtype=torch.float64)
    kept = []
    for b in range(B):
        ctx = int(case.ctx[b])
        _, vall = _gather(case, b)
        if floor:
            kk = max(1, min(ctx, math.floor(case.sparsity * ctx)))
        elif f32:
            kk = _kkeep_f32(case.sparsity, ctx)
        else:
            kk = kkeep_of(case.sparsity, ctx)
        kk = max(1, min(ctx, kk + dk))
        row = []
        for h in range(Hq):
            s = _scores(case, b, h)
            hs = (h // G) * G if first_head else h
            sel = _scores(case, b, hs, use_alibi=not no_alibi).clone()
            if drop_last_page and ctx > P:
                sel[(ctx - 1) // P * P:] = float("-inf")
            if ties_high:
                idx = (ctx - 1) - sel.flip(0).sort(
                    descending=True, stable=True).indices
            else:
                idx = sel.sort(descending=True, stable=True).indices
            idx = idx[:kk]
            w = torch.softmax(s[idx], dim=0)
            out[b, h, 0] = w @ vall[h // G, idx]
            row.append(idx)
        kept.append(row)
    return (out, kept) if with_kept else out


MUTATIONS = {
    "kkeep_minus": dict(dk=-1),
    "kkeep_plus": dict(dk=1),
    "floor": dict(floor=True),
    "kkeep_f32": dict(f32=True),
    "first_head": dict(first_head=True),
    "no_alibi": dict(no_alibi=True),
    "drop_last_page": dict(drop_last_page=True),
    "ties_high": dict(ties_high=True),
}


@functools.lru_cache(maxsize=None)
def expected(spec, grow=0):
    """(oracle output, tol) of a case, computed once and shared.

    tol: (B, Hq, 1, 1) fp64 = 2^-8 * max|v| over the head's kept positions.
    """
    case = build(spec, grow)
    out, kept = oracle(case, with_kept=True)
    t = torch.zeros(case.B, spec.Hq, 1, 1, dtype=torch.float64)
    for b in range(case.B):
        _, vall = _gather(case, b)
        for h in range(spec.Hq):
            t[b, h, 0, 0] = vall[h // case.G, kept[b][h]].abs().max() * 2.0 ** -8
    return out, t


def worst(got, spec, grow=0):
    """(max |got - want| / tol, (row, head, d) where it occurs)."""
    want, t = expected(spec, grow)
    r = (got.double().reshape(want.shape) - want).abs() / t
    r = torch.nan_to_num(r, nan=float("inf"))
    i = int(r.argmax())
    D, Hq = spec.D, spec.Hq
    return float(r.reshape(-1)[i]), (i // (Hq * D), (i // D) % Hq, i % D)


def repaged8(case):
    """(k_pages, v_pages, page_table) of the same pool re-cut into 8-slot
    pages: a page size the kernels do not cover."""
    s = case.spec
    kp, vp, pt = case.k_pages, case.v_pages, case.page_table
    n = kp.shape[0]
    kp8 = (kp.view(n, s.Hkv, 2, 8, s.D).permute(0, 2, 1, 3, 4)
           .reshape(2 * n, s.Hkv, 8, s.D).contiguous())
    vp8 = (vp.view(n, s.Hkv, s.D, 2, 8).permute(0, 3, 1, 2, 4)
           .reshape(2 * n, s.Hkv, s.D, 8).contiguous())
    pt8 = torch.stack([2 * pt, 2 * pt + 1], dim=-1).reshape(case.B, -1)
    return kp8, vp8, pt8.contiguous()


def qkv_buffer(case):
    """(B, 1, (Hq+2Hkv)*D) bf16 fused buffer holding the case's q; the k / v
    sections are finite junk."""
    s = case.spec
    gen = torch.Generator().manual_seed(s.seed)
    junk = (torch.randn(case.B, 1, 2 * s.Hkv * s.D, generator=gen) * 8).to(
        torch.bfloat16)
    flat = case.q.permute(0, 2, 1, 3).reshape(case.B, 1, s.Hq * s.D)
    return torch.cat([flat, junk], dim=-1).contiguous()


# ---------------------------------------------------------------------------
# case table (shared by the CPU guards and the GPU tests)
# ---------------------------------------------------------------------------

_KK = ("kkeep_minus", "kkeep_plus")

BASE = Spec("base-G4-D64", 8, 2, 64, (1, 15, 16, 17, 33, 100), 0.25,
            _KK + ("floor", "first_head", "drop_last_page"), seed=0)

CASES = [
    BASE,
    # lengths where ceil(sparsity * ctx) differs between float32 and double
    Spec("f32-s0.3", 8, 2, 64, (50, 100), 0.3, _KK + ("kkeep_f32",), seed=1),
    Spec("f32-s0.6", 8, 2, 64, (25,), 0.6, _KK + ("kkeep_f32",), seed=2),
    # table padded to 42 pages (672 slots): the P.V walk of every row is
    # split over two workgroups and the scores take more than one block
    Spec("long-s0.1", 8, 2, 64, (48, 100, 255), 0.1,
         _KK + ("floor", "first_head", "drop_last_page"), seed=3,
         pad_pages=24),
    Spec("alibi-mha-D64", 4, 4, 64, (31, 64, 97), 0.25,
         _KK + ("floor", "no_alibi"), alibi=True, seed=4),
    Spec("G8-D128", 8, 1, 128, (20, 130), 0.2,
         _KK + ("first_head", "drop_last_page"), seed=5),
    Spec("G2-D256", 4, 2, 256, (40, 70), 0.25,
         _KK + ("floor", "first_head"), seed=6),
    Spec("G71-D64", 71, 1, 64, (5, 40), 0.25,
         _KK + ("floor", "first_head"), seed=7),
    Spec("tie-G4-D64", 8, 2, 64, (33, 100), 0.25, ("ties_high",), tie=True,
         seed=8),
    # serving lengths. 63 table pages (1008 slots) give 3 P.V splits of 11
    # tiles for the 985 row, so waves 0 and 1 run a second loop iteration;
    # the select loops stride four times over the row and, in the tie case,
    # the threshold's tie count carries across 256-position chunks
    Spec("ctx985-G4-D64", 8, 2, 64, (985, 600, 257), 0.05,
         ("first_head", "drop_last_page"), seed=9),
    Spec("ctx985-tie-G4-D64", 8, 2, 64, (985, 513), 0.05, ("ties_high",),
         tie=True, seed=10),
]
assert len({s.name for s in CASES}) == len(CASES)
assert {m for s in CASES for m in s.covers} == set(MUTATIONS)


def ids(specs):
    return [s.name for s in specs]
