"""Valid arguments, at the smallest legal shape, for every tensor-taking
binding of the HIP extension (bloombee_amd/ops/hip/ext.hip). Plain helper
module for test_ext_bindings_cpu.py (all-CPU rejection) and
test_gpu_ext_bindings.py (per-argument rejection on the device).

Attention ops: B=1, Hkv=1, Hq=2, D=64, one page of 16. Norms: (2, 64).
GEMMs: M=1, N=64, K=256 (the W4 ones K=128); MoE: E=2, S=2.
"""
from dataclasses import dataclass
from typing import Tuple

import torch

BF, F16, F32, I32, U8 = (torch.bfloat16, torch.float16, torch.float32,
                         torch.int32, torch.uint8)
B, HKV, HQ, D, P = 1, 1, 2, 64, 16
X = HQ + 2 * HKV


@dataclass
class Call:
    op: str
    args: list
    bad_dtype: Tuple[int, torch.dtype]   # (argument index, a dtype it rejects)
    inplace: Tuple[int, ...] = ()        # arguments the op writes

    def tensor_args(self):
        return [i for i, a in enumerate(self.args) if isinstance(a, torch.Tensor)]


def build(dev):
    """{op: Call}; every tensor on dev. Deterministic."""
    gen = torch.Generator().manual_seed(4242)

    def r(*shape, dtype=BF):
        return (torch.randn(*shape, generator=gen) * 0.25).to(dtype).to(dev)

    def ints(vals):
        return torch.tensor(vals, dtype=I32, device=dev)

    def pools(d=D):
        return r(1, HKV, P, d), r(1, HKV, d, P), ints([[0]])

    cos, sin = r(P, D // 2, dtype=F32), r(P, D // 2, dtype=F32)
    alibi = r(HQ, dtype=F32)
    scale = D ** -0.5
    calls = []

    def add(op, args, bad_dtype=(0, F32), inplace=()):
        calls.append(Call(op, args, bad_dtype, inplace))

    add("rms_norm", [r(2, 64), r(64), 1e-5])
    add("rms_norm_residual", [r(2, 64), r(2, 64), r(64), 1e-5], (1, F32))
    add("layer_norm", [r(2, 64), r(64), r(64), 1e-5], (2, F16))
    add("rope_apply_", [r(B, HQ, 1, D), r(B, HKV, 1, D), cos, sin, ints([[3]])],
        (1, F16), inplace=(0, 1))
    add("swiglu", [r(2, 128)])
    add("gelu_tanh", [r(2, 64)])
    add("add_bf16", [r(2, 64), r(2, 64)], (1, F32))
    kp, vp, pt = pools()
    add("kv_write", [r(B, HKV, 1, D), r(B, HKV, 1, D), kp, vp, pt, ints([2])],
        (3, F16), inplace=(2, 3))
    kp, vp, pt = pools()
    add("kv_gather", [kp, vp, pt, 0, 4], (1, F16))
    kp, vp, pt = pools()
    add("attn_decode", [r(B, HQ, 1, D), kp, vp, pt, ints([5]), scale, 0, 0, alibi],
        (2, F16))
    kp, vp, pt = pools()
    add("attn_decode_qkv", [r(B, 1, X * D), HQ, kp, vp, pt, ints([5]), scale, 0, 0],
        (3, F16))
    kp, vp, pt = pools()
    ext_ml = torch.tensor([[[0.0, 1.0]] * HQ], dtype=F32, device=dev)
    add("attn_decode_mixed", [r(B, HQ, 1, D), kp, vp, pt, ints([5]), ext_ml,
                              r(B, HQ, D, dtype=F32), scale, 0, 0, alibi, 3],
        (6, BF))
    kp, vp, pt = pools()
    add("attn_decode_sparse", [r(B, HQ, 1, D), kp, vp, pt, ints([5]), 0.5, scale,
                               alibi], (4, torch.int64))
    kp, vp, pt = pools()
    add("attn_decode_sparse_qkv", [r(B, 1, X * D), HQ, kp, vp, pt, ints([5]), 0.5,
                                   scale], (2, F16))
    kp, vp, pt = pools()
    tm = torch.tril(torch.ones(B, 3, 3, dtype=torch.bool)).to(dev)
    add("attn_prefill", [r(B, HQ, 3, D), kp, vp, pt, ints([2]), scale, 0, alibi, tm],
        (8, U8))
    kp, vp, pt = pools()
    add("attn_prefill_qkv", [r(B, 3, X * D), HQ, kp, vp, pt, ints([2]), scale, 0],
        (5, torch.int64))
    q, k, v = r(B, 4, HQ, D), r(B, 4, HKV, D), r(B, 4, HKV, D)
    add("attn_train_fwd", [q, k, v, scale, 0, alibi, True], (2, F16))
    add("attn_train_bwd", [r(B, 4, HQ, D), q, k, v, r(B, 4, HQ, D),
                           r(B, HQ, 4, dtype=F32), scale, 0, alibi], (5, BF))
    kp, vp, pt = pools()
    add("rope_kv_write_", [r(B, 1, X * D), HQ, HKV, cos, sin, ints([[3]]), kp, vp,
                           pt, ints([2])], (3, BF), inplace=(0, 6, 7))
    kp, vp, pt = pools()
    add("rope_kv_write_part", [r(2, B, X * D, dtype=F32), r(X * D), B, 1, HQ, HKV,
                               cos, sin, ints([[3]]), kp, vp, pt, ints([2])],
        (1, F32), inplace=(9, 10))
    add("gemm_skinny", [r(1, 256), r(64, 256), r(1, 64), r(64), 1, r(256), 1e-5,
                        r(1, 32, dtype=F32).abs(), r(32, dtype=F32), 1, False,
                        torch.zeros(1, dtype=I32, device=dev)], (3, F32))
    add("gemm_skinny_swiglu", [r(1, 256), r(64, 256), 1e-5,
                               r(1, 32, dtype=F32).abs(), 2], (1, F16))
    off = ints([0, 1, 2])
    add("moe_gemm", [r(2, 256), r(2, 64, 256), off, ints([1, 0]), r(2, dtype=F32),
                     2, 1], (4, BF))
    packed = torch.randint(0, 256, (2, 64, 64), generator=gen).to(U8).to(dev)
    sc, zp = r(2, 64, 2, dtype=F16).abs(), r(2, 64, 2, dtype=F16)
    add("gemm_w4", [r(1, 128, dtype=F16), packed[0].clone(), sc[0].clone(),
                    zp[0].clone(), r(1, 64), r(64), 64, 0], (0, BF))
    add("moe_gemm_w4", [r(2, 128), packed, sc, zp, off, ints([1, 0]),
                        r(2, dtype=F32), 2, 1, 0], (2, BF))
    add("quant4_pack", [r(2, 64)])
    add("quant4_unpack", [packed[0, :2, :32].clone(), sc[0, :2, :1].clone(),
                          zp[0, :2, :1].clone()], (1, BF))
    add("mfma_selftest", [r(16, 32), r(32, 16)], (1, F32))
    kp, vp, pt = pools(128)
    add("kv_stream_probe", [kp, vp, pt, ints([5]), 1, False], (0, F16))
    return {c.op: c for c in calls}


OPS = sorted(build("cpu"))
