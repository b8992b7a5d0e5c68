"""Inputs, fp64 oracle and bound shared by test_gpu_ring_attention.py and
test_ring_attention_cpu.py. Plain helper module, in the style of
train_attn_cases.py.

Data: B = 2, bf16 q ~ 2 N(0,1), k, v ~ N(0,1) in the (B, H, T, D) layout the
ring takes. For a few rows r a key is made to dominate row r's softmax (k =
q[r] / 2, a score ~ sqrt(D) above the rest) at three places: r // 2 (visible, so
the softmax is not flat), r + 1 (the first key past the row's range) and, with
a window, r - window (the last key below it). The two masked keys carry
v = 64 in columns 0..3, so a mask off by one moves those columns by ~64, two
hundred bounds; the other columns keep a bound set by |v| ~ 4.
"""
import functools
import math
from types import SimpleNamespace

import torch

B = 2
HEADS = [(4, 2), (4, 1)]
RINGS = [(1, 257), (2, 129), (4, 40)]


@functools.lru_cache(maxsize=None)
def build(Hq, Hkv, D, T, window):
    gen = torch.Generator().manual_seed(1000 * T + 10 * D + Hq + Hkv + window)
    G = Hq // Hkv
    bf = lambda x: x.to(torch.bfloat16)
    q = bf(2.0 * torch.randn(B, Hq, T, D, generator=gen))
    k = bf(torch.randn(B, Hkv, T, D, generator=gen))
    v = bf(torch.randn(B, Hkv, T, D, generator=gen))
    for r in (1, T // 3, T // 2 + 1, T - 2):
        for key, poison in ((r // 2, False), (r + 1, True), (r - window, window > 0)):
            if 0 <= key < T:
                k[:, :, key] = bf(0.5 * q[:, ::G, r].float())
                if poison:
                    v[:, :, key, :4] = 64.0
    scale = 1.0 / math.sqrt(D)
    # the oracle: dense fp64 attention over the whole sequence
    kk, vv = (t.double().repeat_interleave(G, dim=1) for t in (k, v))
    s = torch.matmul(q.double(), kk.transpose(-1, -2)) * scale
    i, j = torch.arange(T).view(T, 1), torch.arange(T).view(1, T)
    vis = (j <= i) & ((j > i - window) if window > 0 else (j <= i))
    want = torch.matmul(torch.softmax(s.masked_fill(~vis, float("-inf")), -1), vv)
    bound = 2.0 ** -8 * vv.abs().amax(dim=2, keepdim=True)   # (B, Hq, 1, D)
    return SimpleNamespace(q=q, k=k, v=v, scale=scale, want=want, bound=bound)


def check(got, case, what):
    """got (B, Hq, T, D) on the CPU; prints and asserts the worst err/bound."""
    assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite"
    ratio = (got.double() - case.want).abs() / case.bound
    print(f"[ring] {what}: worst err/bound {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0, f"{what}: err/bound {float(ratio.max()):.3f}"
