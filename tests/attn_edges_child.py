"""Child process of test_gpu_attn_edges.py::test_revert_switch_kernels_in_
child_processes: BBAMD_ATTN_PF / BBAMD_ATTN_NT are read once per process, so
each revert-switch decode kernel needs a fresh interpreter.

Runs the boundary decode group (D=128 and D=64, the four row sets,
n_split 1 and 3) plus one window case against the dense fp64 reference,
prints the worst err / tol and exits non-zero on a mismatch.
"""
import os
import sys

import torch

import attn_cases as ac


def main():
    from bloombee_amd import ops

    assert torch.cuda.is_available() and ops.HAVE_HIP_OPS
    dev = "cuda:0"
    switches = {k: os.environ.get(k) for k in ("BBAMD_ATTN_PF", "BBAMD_ATTN_NT")}
    worst, bad = 0.0, []
    specs = ac.DECODE_BOUNDARY + [s for s in ac.DECODE_WINDOW
                                  if s.name == "dec-w40-D128"]
    assert len(specs) == len(ac.DECODE_BOUNDARY) + 1
    for spec in specs:
        case = ac.build(spec)
        want = ac.dense_ref(case)
        for n_split in ((1, 3, 7) if spec.window else (1, 3)):
            got = ops.attn_decode(
                case.q.to(dev), case.k_pages.to(dev), case.v_pages.to(dev),
                case.page_table.to(dev), case.ctx.to(dev), window=spec.window,
                n_split=n_split).cpu()
            ratio = ac.worst_ratio(got, want, case)
            if not (ratio <= 1.0):          # also catches NaN
                bad.append((spec.name, n_split, ratio))
            worst = max(worst, ratio)
    print(f"[attn-edges] revert-switch {switches}: worst err/tol {worst:.3f}")
    if bad:
        print("MISMATCH:", bad)
        return 1
    print("attn_edges_child ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
