"""Exact-arithmetic cases for the grouped W4 MoE GEMM (moe_gemm_w4.hip):
the `w4` and `moe` builders of gemm_cases.py combined. Plain helper module
for test_moe_w4_cases_cpu.py and test_gpu_moe_w4.py; read gemm_cases.py's
docstring first for why exact inputs make `torch.equal` the right check.

Weights, per expert, directly in quant4_pack layout: codes from a random
perfect matching (ka, kb) of the K columns that all experts share,
scale[e, n, g] = sigma[e, n] * tau[g] with sigma in {1, 2} and
tau = W4_TAU[g % 3], z0[e, n, g] in {7, 8}, zero = -z0 * scale and
q[kb] = z0[ga] + z0[gb] - q[ka], so w[kb] / tau[gb] = -w[ka] / tau[ga].
Activations are shared across experts: A[:, kb] = A[:, ka] * tau[ga] /
tau[gb] + delta with six +-1 perturbations per row; every k-slice carries
large terms that cancel exactly and the result is -sum(delta * w[kb]).
A rows no rowmap entry names hold +-POISON; empty experts hold poison
scale / zero (1024 and -8192), which is also what a metadata pointer
without the expert stride reads for every expert when expert 0 is empty.
Slot scales are the distinct powers of two of gemm_cases._build_moe.

Invariants asserted for EVERY case: A is exact in f16 (the kernel's compute
format) and in bf16 (the op's input format); the expectation is exact in
bf16; sum |a w| in units of 0.25 stays below 2^24, so every f32 partial sum
is exact in any order and across any split of K.
"""
import functools
from dataclasses import dataclass
from typing import Tuple

import torch

from gemm_cases import POISON, W4_TAU, _matching, _ri, xcd_remap

BF = torch.bfloat16
POISON_SCALE, POISON_ZERO = 1024.0, -8192.0


@dataclass(frozen=True)
class Spec:
    name: str
    N: int
    K: int
    counts: Tuple[int, ...]
    ksplit: int = 1           # as passed to the raw op (0 = the op's own rule)
    extra_chunks: int = 0     # mchunks = exact + extra_chunks
    rowmap: bool = False
    scale: bool = False
    seed: int = 0


class Case:
    def __init__(self, spec):
        self.spec = spec


def ids(specs):
    return [s.name for s in specs]


# ---------------------------------------------------------------------------
# host-side launch geometry (mirrors ext.hip moe_w4_plan; used only by the
# mutations, never by `want`)
# ---------------------------------------------------------------------------

def splits_of(spec):
    E, S = len(spec.counts), sum(spec.counts)
    N, K, ksplit = spec.N, spec.K, spec.ksplit
    if ksplit <= 0:
        blocks = (N // 64) * max(1, min(E, S))
        ksplit = max(1, min(K // 512, 1792 // blocks))
    nch = K // 128
    per = -(-nch // ksplit)
    ksplit = -(-nch // per)
    return [(s * per * 128, min(K, (s + 1) * per * 128)) for s in range(ksplit)]


def has_remap(spec):
    nwg = spec.N // 64
    return xcd_remap(nwg) != list(range(nwg))


def exact_mchunks(counts):
    return max(1, -(-max(counts) // 32))


# ---------------------------------------------------------------------------
# builder
# ---------------------------------------------------------------------------

def _build(spec):
    gen = torch.Generator().manual_seed(9000 + spec.seed)
    c = Case(spec)
    N, K, counts = spec.N, spec.K, spec.counts
    assert K % 128 == 0 and N % 64 == 0
    E, S, G = len(counts), sum(counts), K // 64
    ka, kb = _matching(K, gen)
    ga, gb = ka // 64, kb // 64
    tau = torch.tensor([W4_TAU[g % 3] for g in range(G)], dtype=torch.float64)
    sigma = 2.0 ** _ri(0, 1, (E, N), gen)
    z0 = _ri(7, 8, (E, N, G), gen)
    q = torch.zeros(E, N, K, dtype=torch.float64)
    q[:, :, ka] = _ri(1, 14, (E, N, K // 2), gen)
    q[:, :, kb] = z0[:, :, ga] + z0[:, :, gb] - q[:, :, ka]
    assert 0 <= float(q.min()) and float(q.max()) <= 15
    scale = sigma[:, :, None] * tau[None, None, :]
    zero = -z0 * scale
    for e, n in enumerate(counts):
        if n == 0:
            scale[e] = POISON_SCALE
            zero[e] = POISON_ZERO
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
    delta = torch.zeros(Ta, K // 2, dtype=torch.float64)
    npert = 6
    for m in range(Ta):
        at = torch.randperm(K // 2, generator=gen)[:npert]
        delta[m, at] = _ri(0, 1, (npert,), gen) * 2 - 1
    A[:, kb] = A[:, ka] * (tau[ga] / tau[gb])[None, :] + delta
    used = torch.zeros(Ta, dtype=torch.bool)
    used[rm.long() if rm is not None else torch.arange(S)] = True
    A[~used] = (_ri(0, 1, (int((~used).sum()), K), gen) * 2 - 1) * POISON
    c.A, c.off, c.rowmap = A, off, rm
    c.E, c.S = E, S
    c.q = q.to(torch.uint8)
    c.scale, c.zero = scale, zero
    c.packed = (c.q[..., 0::2] | (c.q[..., 1::2] << 4)).contiguous()  # (E, N, K/2)
    c.W = dequant(c)
    # distinct power of two among any 61 consecutive slots
    c.slot_scale = (2.0 ** ((torch.arange(S) * 23 % 61) - 30).double()
                    if spec.scale else None)
    c.mchunks = exact_mchunks(counts) + spec.extra_chunks
    c.unit = 0.25
    return c


def dequant(c, mut=None):
    """(E, N, K) fp64 weights from codes / scale / zero, with the W4 defects."""
    E, N, K = c.E, c.spec.N, c.spec.K
    q = c.q.double()
    if mut == "w4_nibble_swap":
        q = q.reshape(E, N, K // 2, 2).flip(-1).reshape(E, N, K)
    g = torch.arange(K) // 64
    gs = gz = g
    if mut == "w4_scale_neighbour":
        gs = g ^ 1
    if mut == "w4_zero_neighbour":
        gz = g ^ 1
    if mut == "w4_group_straddle":
        gs = gz = torch.arange(K) // 128
    scale, zero = c.scale, c.zero
    # the expert stride missing on a metadata pointer: every expert reads
    # expert 0's rows
    if mut == "w4_scale_expert0":
        scale = scale[:1].expand(E, -1, -1)
    if mut == "w4_zero_expert0":
        zero = zero[:1].expand(E, -1, -1)
    return q * scale[:, :, gs] + zero[:, :, gz]


@functools.lru_cache(maxsize=None)
def build(spec):
    c = _build(spec)
    c.want = model(c)
    check_invariants(c)
    return c


def abs_products(c):
    """sum_k |a| |w| per output, before the slot scale."""
    out = torch.zeros(c.S, c.spec.N, dtype=torch.float64)
    for e in range(c.E):
        a, b = int(c.off[e]), int(c.off[e + 1])
        if b > a:
            rows = c.rowmap[a:b].long() if c.rowmap is not None else torch.arange(a, b)
            out[a:b] = c.A[rows].abs() @ c.W[e].abs().T
    return out


def out_unit(c):
    """One unit of each expected element (broadcasts to want)."""
    if c.slot_scale is not None:
        return c.slot_scale[:, None]
    return torch.tensor(1.0, dtype=torch.float64)


def check_invariants(c):
    name = c.spec.name
    assert bool((c.A.to(torch.float16).double() == c.A).all()), \
        f"{name}: A is not exactly representable in f16"
    assert bool((c.A.to(BF).double() == c.A).all()), \
        f"{name}: A is not exactly representable in bf16"
    assert bool((c.want.to(BF).double() == c.want).all()), \
        f"{name}: expected output is not exactly representable in bf16"
    assert float(abs_products(c).max()) / c.unit < 2 ** 24, \
        f"{name}: partial sums may be inexact in f32"


# ---------------------------------------------------------------------------
# fp64 model with one knob per defect
# ---------------------------------------------------------------------------

MUTATIONS = (
    "drop_last_slice", "last_split_lost", "stripe_unremapped",
    "expert_next", "rowmap_ignored", "scale_by_local_m",
    "chunk_rows_from_first", "group_end_plus_one",
    "w4_scale_neighbour", "w4_zero_neighbour", "w4_nibble_swap",
    "w4_group_straddle", "w4_scale_expert0", "w4_zero_expert0",
)


def _kmask(spec, mut):
    keep = torch.ones(spec.K, dtype=torch.float64)
    live = splits_of(spec)
    if mut == "drop_last_slice":           # last 32 k of the last split
        keep[live[-1][1] - 32: live[-1][1]] = 0
    if mut == "last_split_lost":
        keep[live[-1][0]: live[-1][1]] = 0
    return keep


def _unremap(acc, N):
    """accumulator lands in stripe blockIdx.x instead of the remapped tile."""
    out = torch.empty_like(acc)
    for b, t in enumerate(xcd_remap(N // 64)):
        out[:, b * 64:(b + 1) * 64] = acc[:, t * 64:(t + 1) * 64]
    return out


def model(c, mut=None):
    """Expected (S, N) output in fp64; `mut` applies one defect."""
    assert mut is None or mut in MUTATIONS
    spec = c.spec
    N, E, S = spec.N, c.E, c.S
    keep = _kmask(spec, mut)
    Wall = dequant(c, mut)
    Ta = c.A.shape[0]
    out = torch.zeros(S, N, dtype=torch.float64)

    def rows_of(slots):
        if c.rowmap is None or mut == "rowmap_ignored":
            return slots % Ta
        return c.rowmap[slots].long()

    for e in range(E):
        base, end = int(c.off[e]), int(c.off[e + 1])
        cnt = end - base
        if cnt == 0:
            continue
        W = Wall[(e + 1) % E] if mut == "expert_next" else Wall[e]
        m = torch.arange(cnt)
        src = m % 32 if mut == "chunk_rows_from_first" else m
        acc = (c.A[rows_of(base + src)] * keep) @ W.T
        if c.slot_scale is not None:
            sidx = m if mut == "scale_by_local_m" else base + m
            acc = acc * c.slot_scale[sidx][:, None]
        out[base:end] = acc
    if mut == "group_end_plus_one":
        # expert e also computes the slot after its group with ITS weights;
        # the model lets that stray write win over the rightful owner's
        for e in range(E):
            base, end = int(c.off[e]), int(c.off[e + 1])
            if end > base and end < S:
                acc = (c.A[rows_of(torch.tensor([end]))[0]] * keep) @ Wall[e].T
                if c.slot_scale is not None:
                    acc = acc * c.slot_scale[end]
                out[end] = acc
    if mut == "stripe_unremapped":
        out = _unremap(out, N)
    return out


def _spills(counts):
    S = sum(counts)
    end = 0
    for n in counts:
        end += n
        if n > 0 and end < S:
            return True
    return False


def applicable(spec):
    """Mutations that must move the expected output of this case."""
    names = ["drop_last_slice"]
    if len(splits_of(spec)) >= 2:
        names.append("last_split_lost")
    if has_remap(spec):
        names.append("stripe_unremapped")
    names.append("expert_next")
    if spec.rowmap:
        names.append("rowmap_ignored")
    if spec.scale and any(spec.counts[:-1]):
        names.append("scale_by_local_m")
    if max(spec.counts) > 32:
        names.append("chunk_rows_from_first")
    if _spills(spec.counts):
        names.append("group_end_plus_one")
    names += ["w4_scale_neighbour", "w4_zero_neighbour", "w4_nibble_swap",
              "w4_group_straddle"]
    if any(spec.counts[1:]):
        names += ["w4_scale_expert0", "w4_zero_expert0"]
    return names


# ---------------------------------------------------------------------------
# the cases. N in {128, 576}: 576 = 9 tiles, XCD remap with r = 1. K = 128 is
# one half-filled stage with nothing to prefetch, 384 three slices against
# the period-3 tau (one full stage and a half one), 1024 and 2048 many.
# Counts hold 0 (first, middle, last), 1, 16, 17, 32, 33, 65, 70. ksplit 2
# and 3 give uneven last splits; ksplit 0 takes the op's rule (four splits
# at K = 2048, one at K = 128).
# ---------------------------------------------------------------------------

CASES = [
    Spec("mw4-e4-n128-k128-first-empty", 128, 128, (0, 33, 1, 17),
         rowmap=True, scale=True, seed=1),
    Spec("mw4-e4-n576-k384-last-empty", 576, 384, (65, 16, 32, 0), seed=2),
    Spec("mw4-e8-n128-k1024-ks3-chunks-plus2", 128, 1024,
         (1, 0, 70, 17, 0, 64, 33, 16), ksplit=3, rowmap=True, scale=True,
         extra_chunks=2, seed=3),
    Spec("mw4-e8-n576-k2048-ks0-identity-scale", 576, 2048,
         (32, 33, 0, 0, 65, 1, 16, 0), ksplit=0, scale=True, seed=4),
    Spec("mw4-e4-n128-k384-ks2-mid-empty", 128, 384, (64, 0, 33, 17), ksplit=2,
         rowmap=True, scale=True, extra_chunks=1, seed=5),
    Spec("mw4-e4-n576-k1024-chunks-plus3", 576, 1024, (0, 70, 16, 1),
         rowmap=True, extra_chunks=3, seed=6),
    Spec("mw4-e8-n128-k2048-ks3-identity", 128, 2048,
         (17, 32, 0, 65, 1, 0, 33, 0), ksplit=3, seed=7),
    Spec("mw4-e8-n576-k128-ks0", 576, 128, (0, 64, 65, 0, 16, 70, 1, 33),
         ksplit=0, rowmap=True, scale=True, seed=8),
]

# the four shape / count combinations whose statistics the CPU test pins
PINNED = CASES[:4]
