"""Child process of test_gpu_attn_sparse.py::test_switch_off_runs_the_
composition_in_a_child_process: BBAMD_SPARSE_KERNEL is read once at import,
so the switched-off dispatch needs a fresh interpreter.

With the switch off the sparse kernel bindings must not be reached (they are
replaced by a stub that raises) and both public entries must still match the
fp64 oracle on the base case through the torch composition.
"""
import sys

import torch

import sparse_cases as sc


def main():
    from bloombee_amd import ops
    from bloombee_amd.ops import interface

    assert torch.cuda.is_available() and ops.HAVE_HIP_OPS
    assert interface._SPARSE_KERNEL is False
    dev = "cuda:0"

    real = interface.hip_ops

    class _NoSparse:
        def __getattr__(self, name):
            if name.startswith("attn_decode_sparse"):
                raise AssertionError(f"{name} reached with the switch off")
            return getattr(real, name)

    interface.hip_ops = _NoSparse()
    spec = sc.BASE
    case = sc.build(spec)
    kp, vp = case.k_pages.to(dev), case.v_pages.to(dev)
    pt, ctx = case.page_table.to(dev), case.ctx.to(dev)
    ops.set_attn_sparsity(case.sparsity)
    try:
        a = ops.attn_decode(case.q.to(dev), kp, vp, pt, ctx, case.scale)
        b = ops.attn_paged_qkv(sc.qkv_buffer(case).to(dev), spec.Hq, spec.Hkv,
                               kp, vp, pt, ctx - 1, scale=case.scale)
    finally:
        ops.set_attn_sparsity(1.0)
        interface.hip_ops = real
    bad = []
    for name, got in (("attn_decode", a), ("attn_paged_qkv", b)):
        ratio, where = sc.worst(got.cpu(), spec)
        print(f"[attn-sparse] switch off, {name}: err/tol {ratio:.3f}")
        if not ratio <= 1.0:
            bad.append((name, ratio, where))
    if bad:
        print("MISMATCH:", bad)
        return 1
    print("attn_sparse_child ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
