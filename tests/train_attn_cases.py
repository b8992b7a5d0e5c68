"""Shared inputs, oracle, tolerance and mutations for the training-attention
tests (test_train_attn_cases_cpu.py and test_gpu_attn_train.py). Plain helper
module, in the style of attn_cases.py.

* `build(spec)`: a deterministic, cached CPU case: bf16 q, k, v, dO in the
  (B, T, H, D) layout `ops.attn_train` takes. q is scaled so natural-log
  scores have std ~2 (peaked softmax), and K is boosted at *planted* positions
  (0, T-1, both sides of every multiple of 32 -- which covers the 32-key
  tiles, the 128-row query/key blocks and 256 -- and lo-1 / lo of a window)
  so each carries a sizeable share of one query head's softmax mass. For the
  strided case q/k/v are views into one fused (B, T+1, Hq+2Hkv+1, D) buffer
  whose extra token row and extra head slot are finite poison (+-64), and dO
  is a permuted (B, Hq, T, D) tensor.
* `oracle(case)`: fp64 O, LSE, dQ, dK, dV written out directly (scores, mask,
  softmax, the five products); independent of `ops.reference`.
* `emulate(case)`: the same math in fp32 torch with P and dS rounded to bf16
  where the kernels round them ("the reference alone").
* MUTATIONS: the oracle with one deliberate defect each.

Tolerance (`tol`), per element, u = 2^-8. The kernels form every product
exactly (bf16 x bf16 in fp32) and accumulate in fp32; S, dP, LSE and delta
stay fp32. The rounding points are: P to bf16 (relative 2^-9 each) as an MFMA
operand, dS to bf16 once, and each output to bf16 (2^-9 of itself, which is
at most 2^-9 of the sum of the absolute terms).

  O   : 2^-9 sum_j P_ij |v_jd| + 2^-9 |O_id| <= u max|v| over the kv head's
        keys (the same derivation and form as attn_cases.py).
  dV  : 2^-8 sum_i P_ij |dO_id| (P rounding) + 2^-8 |dV_jd| (store)
        <= 2u sum_i P_ij |dO_id|, the sum running over the group's G heads.
        This is the strict bound (see below for why).
  dK  : scale u sum_i |dS_ij| |Q_id|      (dS rounding + store)
        + scale u sum_i (sum_d' |dO_id' O_id'|) P_ij |Q_id|   (delta term)
  dQ  : scale u sum_j |dS_ij| |K_jd|
        + scale u (sum_d' |dO_id' O_id'|) sum_j P_ij |K_jd|
        The delta term: delta_i = sum_d' dO_id' O_id' is formed from the O the
        forward stored, whose elements carry the P rounding and the store
        rounding (2^-9 each, u together), so |d delta_i| <= u sum |dO O| and
        dS_ij moves by P_ij times that.

2^-9 is the typical bf16 rounding error; just above a power of two it
reaches 2^-8, so the strict worst case is twice the typical bound. For O, dQ
and dK the tighter (typical) bound is the one asserted, as in attn_cases.py:
max|v| is far above sum P|v|, and the dQ/dK bounds sum many independently
rounded terms of either sign plus a delta term that is rarely attained;
`emulate` (the roundings alone) stays within them on every case. dV is
different: a planted key's column of P is dominated by one query, so
sum_i P_ij |dO_id| is essentially one term, its P rounding and the store
rounding can both sit just above a power of two, and nothing averages out.
The roundings alone reach 1.8x the typical bound there, so dV asserts the
strict one (2^-8 per rounding).
"""
import functools
import math
from dataclasses import dataclass

import torch

POISON = 64.0
B = 2
U = 2.0 ** -8


@dataclass(frozen=True)
class Spec:
    name: str
    Hq: int
    Hkv: int
    D: int
    T: int
    window: int = 0
    alibi: bool = False
    strided: bool = False
    seed: int = 0


CASES = {s.name: s for s in [
    Spec("base", 4, 2, 128, 160, seed=1),
    Spec("one", 4, 2, 128, 1, seed=2),
    Spec("ragged33", 4, 2, 128, 33, seed=3),
    Spec("keyblock257", 2, 1, 128, 257, seed=4),
    Spec("mqa5", 5, 1, 64, 70, seed=5),
    Spec("mha", 4, 4, 64, 96, seed=6),
    Spec("window40", 4, 2, 128, 160, window=40, seed=7),
    Spec("alibi", 4, 4, 128, 96, alibi=True, seed=8),
    Spec("strided", 4, 2, 128, 160, strided=True, seed=9),
]}


class Case:
    def __init__(self, spec):
        self.spec = spec
        self.G = spec.Hq // spec.Hkv
        self.scale = 1.0 / math.sqrt(spec.D)
        self.window = spec.window
        self.slopes = None


def _bf(x):
    return x.to(torch.bfloat16)


def _lo_of(qpos, window):
    return max(0, qpos - window + 1) if window > 0 else 0


def planted_positions(spec):
    T = spec.T
    pos = {0, T - 1}
    for m in range(32, T, 32):
        pos.update((m - 1, m))
    lo = _lo_of(T - 1, spec.window)
    if lo > 0:
        pos.update((lo - 1, lo))
    return sorted(pos)


def visible(T, window=0):
    """(T, T) bool: query row i sees key column j."""
    i = torch.arange(T).view(T, 1)
    j = torch.arange(T).view(1, T)
    m = j <= i
    if window > 0:
        m &= j > i - window
    return m


@functools.lru_cache(maxsize=None)
def build(spec):
    c = Case(spec)
    Hq, Hkv, D, T, G = spec.Hq, spec.Hkv, spec.D, spec.T, c.G
    gen = torch.Generator().manual_seed(7000 + spec.seed)
    if spec.alibi:
        from bloombee_amd.ops.reference import alibi_slopes
        c.slopes = alibi_slopes(Hq).float()

    # std-2 natural-log scores: q ~ 2 N(0,1), k ~ N(0,1), scale = 1/sqrt(D)
    q = _bf(2.0 * torch.randn(B, T, Hq, D, generator=gen)).double()
    k = _bf(torch.randn(B, T, Hkv, D, generator=gen)).double()
    v = _bf(torch.randn(B, T, Hkv, D, generator=gen))
    do = _bf(torch.randn(B, T, Hq, D, generator=gen))

    # ---- planting: boost K so each planted key holds a sizeable share of one
    # head's softmax mass for the farthest query that still sees it
    plist = planted_positions(spec)
    c.planted = plist
    is_planted = torch.zeros(T, dtype=torch.bool)
    is_planted[plist] = True
    lo_last = _lo_of(T - 1, spec.window)
    pos_k = torch.arange(T)
    n_h = max(1, -(-len(plist) // G))
    for b in range(B):
        for i, j in enumerate(plist):
            t = T - 1
            if spec.window > 0 and j < lo_last - 1:
                t = min(j + spec.window - 1, T - 1)
            vis = (pos_k <= t) & (pos_k >= _lo_of(t, spec.window))
            base = vis & ~is_planted
            if not bool(base.any()):
                continue
            for kh in range(Hkv):
                h = kh * G + (i % G)
                qv = q[b, t, h]
                s = (k[b, :, kh] @ qv) * c.scale
                if c.slopes is not None:
                    s = s + c.slopes[h].double() * pos_k
                L = torch.logsumexp(s[base], 0)
                beta = (L + math.log(4.0 / n_h)) - s[j]
                k[b, j, kh] = _bf(k[b, j, kh] + beta * qv /
                                  (c.scale * (qv @ qv))).double()
    q, k = _bf(q), _bf(k)

    if spec.strided:
        X = Hq + 2 * Hkv
        sign = torch.randint(0, 2, (B, T + 1, X + 1, D), generator=gen) * 2 - 1
        buf = _bf(sign.double() * POISON)
        buf[:, :T, :Hq] = q
        buf[:, :T, Hq:Hq + Hkv] = k
        buf[:, :T, Hq + Hkv:X] = v
        c.buf = buf
        q = buf[:, :T, :Hq]
        k = buf[:, :T, Hq:Hq + Hkv]
        v = buf[:, :T, Hq + Hkv:X]
        do = do.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
        assert not do.is_contiguous() and not q.is_contiguous()
    c.q, c.k, c.v, c.do = q, k, v, do
    return c


def _last_tile_start(T):
    return (T - 1) // 32 * 32


def _oracle(c, mut=None):
    """fp64 forward and backward, written out. `mut` names one defect."""
    spec = c.spec
    T, G, Hq, Hkv = spec.T, c.G, spec.Hq, spec.Hkv
    scale = c.scale
    q = c.q.double().permute(0, 2, 1, 3)                       # (B, Hq, T, D)
    k = c.k.double().permute(0, 2, 1, 3).repeat_interleave(G, 1)
    v = c.v.double().permute(0, 2, 1, 3).repeat_interleave(G, 1)
    do = c.do.double().permute(0, 2, 1, 3)

    window = spec.window + (1 if mut == "window_off_by_one" and spec.window else 0)
    vis = visible(T, window)
    ii = torch.arange(T).view(T, 1)
    jj = torch.arange(T).view(1, T)
    if mut == "causal_plus_one":
        vis = vis | (jj == ii + 1)
    elif mut == "causal_minus_one":
        vis = vis & ((jj < ii) | (ii == 0))
    elif mut == "drop_last_key_tile" and _last_tile_start(T) > 0:
        vis = vis & (jj < _last_tile_start(T))
        vis = vis | ((jj == 0) & ~vis.any(1, keepdim=True))   # keep rows alive

    raw = (q @ k.transpose(-1, -2)) * scale
    bias = 0.0
    if c.slopes is not None:
        bias = c.slopes.double().view(1, Hq, 1, 1) * jj.double().view(1, 1, 1, T)
    s = (raw + bias).masked_fill(~vis, float("-inf"))
    lse = torch.logsumexp(s, -1)                               # (B, Hq, T)
    p = torch.exp(s - lse.unsqueeze(-1))
    o = p @ v

    # backward recompute of P (the kernels rebuild it from the stored LSE)
    pb = p
    if mut == "no_alibi_in_backward":
        pb = torch.exp(raw.masked_fill(~vis, float("-inf")) - lse.unsqueeze(-1))
    elif mut == "lse_before_alibi":
        lse = torch.logsumexp(raw.masked_fill(~vis, float("-inf")), -1)
        pb = torch.exp(s - lse.unsqueeze(-1))
    dp = do @ v.transpose(-1, -2)
    delta = (do * o).sum(-1, keepdim=True)
    ds = pb * (dp if mut == "no_delta" else dp - delta)
    dq = ds @ k * (1.0 if mut == "no_scale_dq" else scale)
    pk, dsk = pb, ds
    if mut == "drop_last_query_tile" and _last_tile_start(T) > 0:
        keep = (ii < _last_tile_start(T)).double()
        pk, dsk = pb * keep, ds * keep
    dk = dsk.transpose(-1, -2) @ q * (1.0 if mut == "no_scale_dk" else scale)
    dv = pk.transpose(-1, -2) @ do
    D = spec.D
    dk = dk.view(B, Hkv, G, T, D)
    dv = dv.view(B, Hkv, G, T, D)
    if mut == "first_head_of_group":
        dk, dv = dk[:, :, 0], dv[:, :, 0]
    else:
        dk, dv = dk.sum(2), dv.sum(2)

    bt = lambda x: x.permute(0, 2, 1, 3).contiguous()           # -> (B, T, H, D)
    return {"O": bt(o), "LSE": lse, "dQ": bt(dq), "dK": bt(dk), "dV": bt(dv),
            "_p": p, "_ds": ds}


@functools.lru_cache(maxsize=None)
def oracle(case):
    return _oracle(case)


MUTATIONS = {name: functools.partial(_oracle, mut=name) for name in [
    "causal_plus_one", "causal_minus_one", "window_off_by_one", "no_delta",
    "no_scale_dq", "no_scale_dk", "first_head_of_group",
    "no_alibi_in_backward", "drop_last_key_tile", "drop_last_query_tile",
    "lse_before_alibi"]}


@functools.lru_cache(maxsize=None)
def tol(case):
    """Per-element bounds {O, dQ, dK, dV}, each shaped like (or broadcastable
    to) its (B, T, H, D) output; derivation in the module docstring."""
    spec = case.spec
    G, Hkv, T, D = case.G, spec.Hkv, spec.T, spec.D
    ref = oracle(case)
    p, ds = ref["_p"], ref["_ds"].abs()
    q = case.q.double().permute(0, 2, 1, 3).abs()
    k = case.k.double().permute(0, 2, 1, 3).repeat_interleave(G, 1).abs()
    do = case.do.double().permute(0, 2, 1, 3)
    o = ref["O"].permute(0, 2, 1, 3)
    dabs = (do * o).abs().sum(-1, keepdim=True)                 # (B, Hq, T, 1)
    bt = lambda x: x.permute(0, 2, 1, 3).contiguous()
    grp = lambda x: x.view(B, Hkv, G, T, D).sum(2)

    vmax = case.v.double().abs().amax(dim=(1, 3))               # (B, Hkv)
    t_o = (U * vmax.repeat_interleave(G, 1)).view(B, 1, spec.Hq, 1)
    t_dv = 2 * U * bt(grp(p.transpose(-1, -2) @ do.abs()))
    t_dk = case.scale * U * bt(grp(ds.transpose(-1, -2) @ q +
                                   (p * dabs).transpose(-1, -2) @ q))
    t_dq = case.scale * U * bt(ds @ k + dabs * (p @ k))
    return {"O": t_o, "dQ": t_dq, "dK": t_dk, "dV": t_dv}


def emulate(case):
    """fp32 torch with the kernels' rounding points: unnormalised P to bf16
    for P.V, O to bf16; backward P and dS to bf16 once each, delta from the
    bf16 O, outputs to bf16."""
    spec = case.spec
    G, Hkv, T, D, Hq = case.G, spec.Hkv, spec.T, spec.D, spec.Hq
    r = lambda x: x.to(torch.bfloat16).float()
    q = case.q.float().permute(0, 2, 1, 3)
    k = case.k.float().permute(0, 2, 1, 3).repeat_interleave(G, 1)
    v = case.v.float().permute(0, 2, 1, 3).repeat_interleave(G, 1)
    do = case.do.float().permute(0, 2, 1, 3)
    s = (q @ k.transpose(-1, -2)) * case.scale
    if case.slopes is not None:
        s = s + case.slopes.view(1, Hq, 1, 1) * \
            torch.arange(T, dtype=torch.float32).view(1, 1, 1, T)
    s = s.masked_fill(~visible(T, spec.window), float("-inf"))
    m = s.amax(-1, keepdim=True)
    pu = torch.exp(s - m)
    l = pu.sum(-1, keepdim=True)
    o = r((r(pu) @ v) / l)
    lse = (m + torch.log(l)).squeeze(-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    dp = do @ v.transpose(-1, -2)
    delta = (do * o).sum(-1, keepdim=True)
    ds = r(p * (dp - delta))
    dq = r(ds @ k * case.scale)
    grp = lambda x: x.view(B, Hkv, G, T, D).sum(2)
    dk = r(grp(ds.transpose(-1, -2) @ q) * case.scale)
    dv = r(grp(r(p).transpose(-1, -2) @ do))
    bt = lambda x: x.permute(0, 2, 1, 3).contiguous()
    return {"O": bt(o), "LSE": lse, "dQ": bt(dq), "dK": bt(dk), "dV": bt(dv)}


def worst(got, want, bound):
    """(max err/tol, index of the worst element). A zero bound with a zero
    error counts as 0; a zero bound with any error as inf."""
    err = (got.double() - want).abs()
    bound = bound.expand_as(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), tuple(
        int(x) for x in torch.unravel_index(torch.tensor(i), ratio.shape))
