"""Shared cases and fp64 models for the fused decode-GEMM epilogue tests
(test_fused_cases_cpu.py and test_gpu_fused_epilogues.py). Plain helper
module, built on gemm_cases.

SwiGLU-fused gate_up GEMM. A case is a gemm_cases dense (norm_mode 0) or
norm (norm_mode 2, ss_in of 4 stripes) case with N = 2I: rows [0, I) of W
are the gate weights, rows [I, 2I) the up weights, drawn independently, so
gate and up differ and vary by column. The gate_up values are small
integers (times 1/2 in the norm cases), exact in f32 in any order and exact
in bf16; the activation silu(g) * u is then a function of exact inputs and
the fused kernel has to reproduce the unfused pair of kernels bit for bit.
Against fp64 the activation carries one bf16 rounding plus the f32
evaluation of g / (1 + exp(-g)) * u: `act_bound`.

`act_model(case, mut)` is the fp64 model with one knob per defect of the
fused epilogue; test_fused_cases_cpu.py shows each of them moves at least
one expected bf16 element of every case it applies to.
"""
import functools

import torch

import gemm_cases as gc

BF = torch.bfloat16

SWIGLU_M = (1, 15, 16, 17, 32)
SWIGLU_K = (256, 768)
SWIGLU_I = (288, 352, 512)      # 9, 11 and 16 workgroups of 32 columns
SWIGLU_MODES = (0, 2)

SWIGLU_MUTATIONS = ("swapped_pair", "column_shift8", "lost_stage",
                    "row_clamp16")


def swiglu_spec(M, K, I, mode):
    name = f"swiglu-m{M}-k{K}-i{I}-mode{mode}"
    seed = 200 + (M * 7 + K // 256 * 3 + I // 32 + mode) % 97
    if mode == 0:
        return gc.Spec(name, "dense", M, 2 * I, K, 1, seed=seed)
    return gc.Spec(name, "norm", M, 2 * I, K, 1, mode=2, ss_in=4, seed=seed)


SWIGLU_SPECS = [swiglu_spec(M, K, I, mode) for mode in SWIGLU_MODES
                for K in SWIGLU_K for I in SWIGLU_I for M in SWIGLU_M]


@functools.lru_cache(maxsize=None)
def build_swiglu(spec):
    c = gc.build(spec)
    c.want_act = act_model(c)
    return c


def applicable(spec):
    names = ["swapped_pair", "column_shift8", "lost_stage"]
    if spec.M > 16:
        names.append("row_clamp16")
    return names


def gate_up_model(c, mut=None):
    """fp64 gate_up (M, 2I) of a swiglu case."""
    spec = c.spec
    M, K = spec.M, spec.K
    rows = torch.arange(M)
    if mut == "row_clamp16":               # second m-tile reads the first's rows
        rows = torch.where(rows >= 16, torch.full_like(rows, 15), rows)
    keep = torch.ones(K, dtype=torch.float64)
    if mut == "lost_stage":                # last 128-k register set never issued
        keep[K - 128:] = 0
    W = c.Wfold if spec.kind == "norm" else c.W
    acc = (c.Abuf[rows] * keep) @ W.T
    if spec.kind == "norm":
        tot = c.ss_in.sum(0)[:M]
        acc = acc / torch.sqrt(tot / K)[:, None]
    return acc


def act_model(c, mut=None):
    """fp64 silu(gate) * up, (M, I)."""
    I = c.spec.N // 2
    gu = gate_up_model(c, mut)
    g, u = gu[:, :I], gu[:, I:]
    if mut == "swapped_pair":              # lanes li < 8 took the up rows
        g, u = u, g
    if mut == "column_shift8":             # partner lane one wave-group off
        u = u.roll(-8, 1)
    return g / (1.0 + torch.exp(-g)) * u


def act_bound(c):
    """|got - want| allowed against fp64: one bf16 rounding of the result,
    2^-8 |want|, plus the f32 evaluation before it. exp(-g) goes through
    exp2(-g * log2e): the product's rounding moves the exponent by
    |g| log2e 2^-24 and the hardware exp2 is good to 1 ulp, so exp(-g) is
    within (|g| + 2) 2^-23 relative; 1 + e, the division and the product
    add three more roundings. (|g| + 8) 2^-23 |want| covers all of it, and
    2^-134 the subnormal results."""
    I = c.spec.N // 2
    g = gate_up_model(c)[:, :I]
    want = c.want_act
    return (2.0 ** -8 + (g.abs() + 8) * 2.0 ** -23) * want.abs() + 2.0 ** -134


# ---------------------------------------------------------------------------
# in-launch split-K reduce: one exact case per (N, K, ksplit), built at
# M = 32 with bias, residual and ss_out; smaller M are row slices of it and
# the "none of them" variant subtracts bias and residual (exact integers).
# ---------------------------------------------------------------------------

REDUCE_N = (512, 576, 4096)
REDUCE_KS = ((512, 2), (2304, 3), (4096, 8))
REDUCE_M = (1, 15, 17, 32)


@functools.lru_cache(maxsize=None)
def build_reduce(N, K, ksplit):
    spec = gc.Spec(f"reduce-n{N}-k{K}-ks{ksplit}", "dense", 32, N, K, ksplit,
                   bias=True, res=True, ss_out=True,
                   seed=300 + (N // 64 + K // 256 + ksplit) % 89)
    c = gc.build(spec)
    c.want_plain = c.want - c.bias[None, :] - c.res
    return c


def poisoned(a, pad=3):
    """rows of `a` on top of `pad` rows of +-POISON (the A-buffer idiom of
    gemm_cases: a kernel that reads a row past M meets poison)."""
    p = torch.full((pad, a.shape[1]), gc.POISON, dtype=a.dtype)
    p[:, 1::2] = -gc.POISON
    return torch.cat([a, p])
