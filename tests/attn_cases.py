"""Shared inputs, reference and mutations for the attention edge tests
(test_attn_cases_cpu.py and test_gpu_attn_edges.py). Plain helper module.

Three things live here:

* `build(spec)`: a deterministic, cached CPU case. Q/K/V are bf16 values;
  q is scaled so natural-log scores have std ~2 (peaked softmax), and K is
  boosted at *planted* positions (0, ctx-1, both sides of every boundary the
  case is about, lo-1 / lo of a window) so each of them carries a sizeable
  share of one query head's softmax mass. The page table is a randperm over
  a pool with spare pages, and every pool slot that holds no live position
  is finite poison (+-64 in K and V).
* `dense_ref(case)`: a dense fp64 reference written out directly (gather,
  mask, softmax, @ v); independent of `ops.reference.attn_paged`.
* the mutations of that reference (MUTATIONS) used by the sensitivity guards:
  each is `dense_ref` with one deliberate error.

Tolerance (`tol`): products are exact bf16 x bf16 in fp32, P is rounded to
bf16 before P.V (relative 2^-9 each) and the output is rounded to bf16
(2^-9), so per (row, head) |err| <= 2^-9 sum w|v| + 2^-9 |out|
<= 2^-8 max|v| over the row's visible positions of that kv head.
(2^-9 is the typical bf16 rounding error; just above a power of two it
reaches 2^-8, so the strict worst case is twice this bound. The fp32
reference rounded to bf16 alone reaches 0.82 of it on these cases and the
kernels stay at or below that, so the tighter bound is the one asserted.)
"""
import functools
import math
from dataclasses import dataclass
from typing import Tuple

import torch

P = 16
POISON = 64.0


@dataclass(frozen=True)
class Spec:
    name: str
    Hq: int
    Hkv: int
    D: int
    rows: Tuple[Tuple[int, int], ...]   # per row (q_start, Tq); decode: (ctx-1, 1)
    window: int = 0
    alibi: bool = False
    marks: Tuple[int, ...] = ()         # boundaries m: m-1 and m are planted
    seed: int = 0


def decode_spec(name, Hq, Hkv, D, ctxs, **kw):
    return Spec(name, Hq, Hkv, D, tuple((c - 1, 1) for c in ctxs), **kw)


def prefill_spec(name, Hq, Hkv, D, q_starts, Tq, **kw):
    return Spec(name, Hq, Hkv, D, tuple((s, Tq) for s in q_starts), **kw)


class Case:
    """Built inputs. Pool tensors are bf16; q is bf16 (B, Hq, Tq, D)."""

    def __init__(self, spec):
        self.spec = spec
        self.B = len(spec.rows)
        self.Tq = spec.rows[0][1]
        assert all(r[1] == self.Tq for r in spec.rows)
        self.G = spec.Hq // spec.Hkv
        self.scale = 1.0 / math.sqrt(spec.D)
        self.q_start = torch.tensor([r[0] for r in spec.rows], dtype=torch.int32)
        self.ctx = self.q_start + self.Tq

    @property
    def window(self):
        return self.spec.window


def _bf(x):
    return x.to(torch.bfloat16)


def _lo_of(qpos, window):
    return max(0, qpos - window + 1) if window > 0 else 0


def planted_positions(spec, b):
    """Sorted key positions of row b that the case is about."""
    qs, Tq = spec.rows[b]
    ctx = qs + Tq
    pos = {0, ctx - 1}
    marks = set(spec.marks)
    if qs > 0:
        marks.add(qs)           # history / new-token boundary
    for m in marks:
        if 0 < m < ctx:
            pos.update((m - 1, m))
    lo = _lo_of(ctx - 1, spec.window)
    if lo > 0:
        pos.update((lo - 1, lo))
    return sorted(pos)


@functools.lru_cache(maxsize=None)
def build(spec):
    c = Case(spec)
    B, Hq, Hkv, D, G, Tq = c.B, spec.Hq, spec.Hkv, spec.D, c.G, c.Tq
    gen = torch.Generator().manual_seed(1000 + spec.seed)
    max_ctx = int(c.ctx.max())
    maxp = max_ctx // P + 2          # position ctx always has a table entry
    npages = B * maxp + 5            # spare pages nobody owns
    c.maxp = maxp
    c.page_table = (torch.randperm(npages, generator=gen)[: B * maxp]
                    .to(torch.int32).reshape(B, maxp))
    c.slopes = None
    if spec.alibi:
        from bloombee_amd.ops.reference import alibi_slopes
        c.slopes = alibi_slopes(Hq)

    # std-2 natural-log scores: q ~ 2 N(0,1), k ~ N(0,1), scale = 1/sqrt(D)
    q = _bf(2.0 * torch.randn(B, Hq, Tq, D, generator=gen)).double()
    k = _bf(torch.randn(B, Hkv, max_ctx, D, generator=gen)).double()
    v = _bf(torch.randn(B, Hkv, max_ctx, D, generator=gen)).double()

    # ---- planting: boost K so each planted position holds a sizeable share
    # of one head's softmax mass for the farthest query that still sees it
    c.planted = []
    for b in range(B):
        qs, ctx = int(c.q_start[b]), int(c.ctx[b])
        plist = planted_positions(spec, b)
        c.planted.append(plist)
        lo_last = _lo_of(ctx - 1, spec.window)
        pos_k = torch.arange(ctx)
        is_planted = torch.zeros(ctx, dtype=torch.bool)
        is_planted[plist] = True
        n_h = max(1, -(-len(plist) // G))
        for i, j in enumerate(plist):
            if spec.window > 0 and j < lo_last - 1:
                t = min(max(j + spec.window - 1 - qs, 0), Tq - 1)
            else:
                t = Tq - 1
            qpos = qs + t
            vis = (pos_k <= qpos) & (pos_k >= _lo_of(qpos, spec.window))
            base = vis & ~is_planted
            if not bool(base.any()):
                continue
            for kh in range(Hkv):
                h = kh * G + (i % G)
                qv = q[b, h, t]
                s = (k[b, kh, :ctx] @ qv) * c.scale
                if c.slopes is not None:
                    s = s + c.slopes[h].double() * pos_k
                L = torch.logsumexp(s[base], 0)
                beta = (L + math.log(4.0 / n_h)) - s[j]
                k[b, kh, j] = _bf(k[b, kh, j] + beta * qv /
                                  (c.scale * (qv @ qv))).double()
    c.q = _bf(q)
    c.k, c.v = k, v       # dense (B, Hkv, max_ctx, D) fp64, live up to ctx[b]

    # ---- pool: finite poison everywhere, then the live positions
    def poison(*shape):
        sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
        return _bf(sign * POISON)

    kp = poison(npages, Hkv, P, D)
    vp = poison(npages, Hkv, D, P)
    live = torch.zeros(npages, P, dtype=torch.bool)
    for b in range(B):
        ctx = int(c.ctx[b])
        pos = torch.arange(ctx)
        pages = c.page_table[b, pos // P].long()
        slots = pos % P
        kp[pages, :, slots, :] = _bf(k[b, :, :ctx].permute(1, 0, 2))
        vp[pages, :, :, slots] = _bf(v[b, :, :ctx].permute(1, 0, 2))
        live[pages, slots] = True
        # the slot just past ctx: poison K aligned with each group's first
        # head so a kernel that reads it gives that position real weight
        pg, sl = int(c.page_table[b, ctx // P]), ctx % P
        for kh in range(Hkv):
            sg = torch.where(q[b, kh * G, Tq - 1] >= 0, 1.0, -1.0)
            kp[pg, kh, sl, :] = _bf(sg * POISON)
    c.k_pages, c.v_pages, c.live = kp, vp, live
    return c


# ---------------------------------------------------------------------------
# dense fp64 reference (+ the knobs the mutations turn)
# ---------------------------------------------------------------------------

def _swap_choice(case, b):
    """Two live pages of row b to swap: a holds a planted position that the
    last query sees, b does not hold a planted position in the same slot.
    Interior pages are preferred. None if the row has no such pair."""
    ctx = int(case.ctx[b])
    lo = _lo_of(ctx - 1, case.window)
    n = -(-ctx // P)
    planted = set(case.planted[b])
    for interior in (True, False):
        for j in case.planted[b]:
            if j < lo:
                continue
            a = j // P
            for pb in range(n):
                j2 = pb * P + j % P
                if pb == a or j2 >= ctx or j2 in planted:
                    continue
                if interior and not (0 < a < n - 1 and 0 < pb < n - 1):
                    continue
                return a, pb
    return None


def dense_ref(case, zero_q=False, hi_shift=0, lo_shift=0, swap_k=False,
              row_shift=0, kvh_shift=0, slope_shift=0):
    """(B, Hq, Tq, D) fp64. All-default arguments give the true result.

    hi_shift:   query at p sees keys <= p + hi_shift (0 = causal)
    lo_shift:   window lower bound moved by this many positions
    swap_k:     K is read through a page table with two pages swapped
    row_shift:  row b uses row b+row_shift's q_start (hence ctx)
    kvh_shift:  query head h reads kv head h // G + kvh_shift
    slope_shift: head h uses the ALiBi slope of head h + slope_shift
    """
    spec = case.spec
    B, Hq, Hkv, D, G, Tq = case.B, spec.Hq, spec.Hkv, spec.D, case.G, case.Tq
    N = case.maxp * P
    pos_k = torch.arange(N)
    out = torch.zeros(B, Hq, Tq, D, dtype=torch.float64)
    for b in range(B):
        qs = int(case.q_start[(b + row_shift) % B])
        tbl = case.page_table[b].long()
        tbl_k = tbl
        if swap_k:
            ab = _swap_choice(case, b)
            if ab is not None:
                tbl_k = tbl.clone()
                tbl_k[ab[0]], tbl_k[ab[1]] = tbl[ab[1]], tbl[ab[0]]
        kall = (case.k_pages[tbl_k].double().permute(1, 0, 2, 3)
                .reshape(Hkv, N, D))
        vall = (case.v_pages[tbl].double().permute(1, 0, 3, 2)
                .reshape(Hkv, N, D))
        pos_q = qs + torch.arange(Tq)
        mask = pos_k[None, :] <= (pos_q + hi_shift)[:, None]
        if spec.window > 0:
            mask &= pos_k[None, :] > (pos_q - spec.window + lo_shift)[:, None]
        for h in range(Hq):
            kh = (h // G + kvh_shift) % Hkv
            qv = case.q[b, h].double()
            if zero_q:
                qv = torch.zeros_like(qv)
            s = (qv @ kall[kh].T) * case.scale
            if case.slopes is not None:
                s = s + case.slopes[(h + slope_shift) % Hq].double() * pos_k
            s = s.masked_fill(~mask, float("-inf"))
            w = torch.softmax(s, dim=-1)
            w = torch.nan_to_num(w, nan=0.0)     # a query that sees nothing
            out[b, h] = w @ vall[kh]
    return out


MUTATIONS = {
    "zero_q": dict(zero_q=True),
    "drop_newest": dict(hi_shift=-1),
    "past_ctx": dict(hi_shift=1),
    "window_lo_minus": dict(lo_shift=-1),
    "window_lo_plus": dict(lo_shift=1),
    "swap_pages": dict(swap_k=True),
    "neighbour_row": dict(row_shift=1),
    "wrong_kv_head": dict(kvh_shift=1),
    "alibi_next_head": dict(slope_shift=1),
}


def applicable(spec):
    """Which mutations a case must tell apart.

    every case:           drop_newest, past_ctx, neighbour_row (all cases are
                          ragged batches)
    every case but window=1 (a query that sees only itself ignores q and K):
                          zero_q; swap_pages if some row has >= 2 pages
    window < longest ctx: window_lo_minus, window_lo_plus
    Hkv > 1:              wrong_kv_head
    ALiBi:                alibi_next_head
    swap_pages swaps the K pages only (V keeps the true table): without a
    mask or a position bias softmax attention is invariant under a
    permutation of whole (k, v) pairs, so a full swap is not an error a
    plain decode case could see.
    """
    names = ["drop_newest", "past_ctx"]
    if len(spec.rows) > 1:
        names.append("neighbour_row")
    max_ctx = max(r[0] + r[1] for r in spec.rows)
    if spec.window != 1:
        names.append("zero_q")
        if max_ctx >= 2 * P:
            names.append("swap_pages")
    if 0 < spec.window < max_ctx:
        names += ["window_lo_minus", "window_lo_plus"]
    if spec.Hkv > 1:
        names.append("wrong_kv_head")
    if spec.alibi:
        names.append("alibi_next_head")
    return names


def tol(case):
    """(B, Hq, 1, 1) fp64: 2^-8 * max|v| over the positions of row b / kv
    head that any of its queries sees (poison is not visible)."""
    spec = case.spec
    t = torch.zeros(case.B, spec.Hq, 1, 1, dtype=torch.float64)
    for b in range(case.B):
        qs, ctx = int(case.q_start[b]), int(case.ctx[b])
        lo = _lo_of(qs, spec.window)
        vmax = case.v[b, :, lo:ctx].abs().amax(dim=(1, 2))      # (Hkv,)
        t[b, :, 0, 0] = vmax.repeat_interleave(case.G) * 2.0 ** -8
    return t


def worst_ratio(got, want, case):
    """max over elements of |got - want| / tol."""
    return float(((got.double() - want).abs() / tol(case)).max())


# ---------------------------------------------------------------------------
# case tables (shared by the CPU guards and the GPU tests)
# ---------------------------------------------------------------------------

ROW_SETS = [(1, 15, 16, 17), (31, 32, 33, 64), (127, 128, 129, 65),
            (255, 256, 257, 1)]
# page (16), KV tile (32), 4-wave stride (128), pipelined double stride (256)
# plus the split edges n_split = 2 / 3 put inside the longer rows
_ROW_MARKS = [(16,), (16, 32, 48), (16, 32, 48, 96, 128), (32, 96, 128, 144, 256)]

DECODE_BOUNDARY = [
    decode_spec(f"dec-b{i}-D{D}", Hq, Hkv, D, rows, marks=_ROW_MARKS[i], seed=i)
    for (Hq, Hkv, D) in ((8, 2, 128), (16, 2, 64))
    for i, rows in enumerate(ROW_SETS)
]

_MATRIX_ROWS = (130, 97, 33, 16)
_MATRIX_MARKS = (32, 48, 96, 128)      # tile, n_split=3 edges (9 pages), stride
DECODE_MATRIX = [
    decode_spec(f"dec-m-D{D}-Hq{Hq}-Hkv{Hkv}", Hq, Hkv, D, _MATRIX_ROWS,
                marks=_MATRIX_MARKS, seed=10 + i)
    for i, (Hq, Hkv, D) in enumerate([
        (4, 4, 32),      # D=32 MHA
        (8, 2, 32),      # D=32 G=4
        (24, 1, 64),     # two head chunks, the second partial
        (32, 2, 128),    # G=16: exactly one full chunk
        (8, 2, 256),     # D=256 G=4
        (4, 2, 512),     # wide kernel, MAXG=4
        (32, 2, 512),    # wide kernel, G=16
    ])
]

_WIN_ROWS = (100, 77, 41, 16)
DECODE_WINDOW = [
    decode_spec(f"dec-w{w}-D{D}", 8, 2, D, _WIN_ROWS, window=w,
                marks=(32, 64), seed=20 + i)
    for i, (D, w) in enumerate([
        (64, 1), (64, 17), (64, 1000),
        # ctx=100, window=40 -> lo=60; n_split=7 gives one page per split, so
        # split [32,48) has tile0 = 0 and lies wholly below lo: it processes
        # a tile in which every position is dead (m=-1e30, l=32) and relies
        # on a later live split to wipe it in the combine
        (128, 40), (128, 16), (128, 17),
        (256, 17), (256, 40), (256, 1),
        (512, 16), (512, 1000), (512, 40),
    ])
]

DECODE_ALIBI = [
    decode_spec("dec-alibi", 4, 4, 64, (70, 33, 17, 5), alibi=True,
                marks=(16, 32, 48), seed=40),
]

DECODE_FUSED = [
    decode_spec(f"dec-qkv-w{w}", 8, 2, 128, _WIN_ROWS, window=w,
                marks=(32, 64), seed=45 + i)
    for i, w in enumerate((0, 17))
]

_QS = (0, 5, 16, 37)
PREFILL_SHAPES = [
    prefill_spec(f"pre-T{Tq}-D{D}-G{Hq // Hkv}", Hq, Hkv, D, _QS, Tq,
                 marks=(16, 32, 128), seed=50 + i)
    for i, (Tq, Hq, Hkv, D) in enumerate([
        (1, 2, 2, 64),
        (15, 4, 1, 32),
        (16, 8, 1, 128),
        (17, 2, 2, 256),
        (127, 8, 2, 64),
        (128, 2, 2, 32),
        (129, 8, 2, 128),     # second q-tile, q_start > 0, G = 4
        (129, 8, 1, 256),     # second q-tile, G = 8
    ])
]

PREFILL_WINDOW = [
    prefill_spec(f"pre-w{w}-T129", 8, 2, 128 if i % 2 == 0 else 64, _QS, 129,
                 window=w, marks=(32, 128), seed=60 + i)
    for i, w in enumerate((1, 17, 32, 40, 1000))
] + [
    prefill_spec(f"pre-w{w}-T17", 4, 2, 128, (37, 0, 50), 17, window=w,
                 marks=(32,), seed=70 + i)
    for i, w in enumerate((1, 17, 32, 40, 1000))
]

PREFILL_ALIBI = [
    prefill_spec("pre-alibi", 4, 4, 64, (5, 0, 20), 33, alibi=True,
                 marks=(16, 32), seed=80),
]

PREFILL_FUSED = [
    prefill_spec("pre-qkv", 8, 2, 128, (3, 0, 21), 40, marks=(16, 32), seed=85),
]

ALL_CASES = (DECODE_BOUNDARY + DECODE_MATRIX + DECODE_WINDOW + DECODE_ALIBI +
             DECODE_FUSED + PREFILL_SHAPES + PREFILL_WINDOW + PREFILL_ALIBI +
             PREFILL_FUSED)
assert len({s.name for s in ALL_CASES}) == len(ALL_CASES)


def ids(specs):
    return [s.name for s in specs]
