"""The ring fold's torch definition (ops.reference.attn_ring_fold) chained over
the blocks of every case of test_gpu_ring_attention.py, against the fp64
oracle and bound of ring_attn_cases.py: the bound is a condition on the inputs
as much as on the kernel. Also the state-passes-through property."""
import pytest
import torch

import ring_attn_cases as rc
from bloombee_amd.ops import reference as ref


@pytest.mark.parametrize("window", [0, 50])
@pytest.mark.parametrize("world,t_loc", rc.RINGS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", rc.HEADS)
@pytest.mark.parametrize("order", ["oldest", "newest"])
def test_definition_within_bound(order, Hq, Hkv, D, world, t_loc, window):
    c = rc.build(Hq, Hkv, D, world * t_loc, window)
    outs = []
    for r in range(world):
        srcs = list(range(r + 1)) if order == "oldest" else list(range(r, -1, -1))
        state = None
        for src in srcs:
            sl = slice(src * t_loc, (src + 1) * t_loc)
            state = ref.attn_ring_fold(c.q[:, :, r * t_loc:(r + 1) * t_loc],
                                       c.k[:, :, sl], c.v[:, :, sl], state,
                                       r * t_loc, src * t_loc, c.scale, window,
                                       last=src == srcs[-1])
        outs.append(state.permute(0, 2, 1, 3))
    rc.check(torch.cat(outs, dim=2), c, f"definition {order}")


def test_masked_block_leaves_state_untouched():
    c = rc.build(4, 2, 64, 160, 50)
    q, k, v = c.q[:, :, 120:], c.k, c.v
    s1 = ref.attn_ring_fold(q, k[:, :, 80:120], v[:, :, 80:120], None, 120, 80, c.scale, 50)
    s2 = ref.attn_ring_fold(q, k[:, :, :40], v[:, :, :40], s1, 120, 0, c.scale, 50)
    assert torch.equal(s1[0], s2[0]) and torch.equal(s1[1], s2[1])
    empty = ref.attn_ring_fold(q, k[:, :, :40], v[:, :, :40], None, 120, 0, c.scale, 50, last=True)
    assert not bool(empty.any()), "a row that never saw a key yields zeros"
