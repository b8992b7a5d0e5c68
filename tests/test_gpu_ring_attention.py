"""Ring-attention fold kernel (ops/hip/attn_ring.hip) against an fp64 dense
causal / windowed attention over the full sequence, written out here and
independent of ops.reference: through ring_attention_local, through
ops.attn_ring_fold in both block orders, through the BBAMD_RING_KERNEL switch
and through cp_prefill_llama.

Bound, per element: |O - O64| <= 2^-8 max_j |v[j, d]| over the KV head's keys
(tests/train_attn_cases.py's O bound, taken per column d: sum_j P_ij |v_jd| <=
max_j |v_jd|). The rounding points are attn_train's and the carried state is
f32. tests/test_ring_attention_cpu.py shows that the definition chained over
the same blocks stays inside it on every case below.
"""
import pytest
import torch

import ring_attn_cases as rc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bloombee_amd import ops
    from bloombee_amd.ops import interface
    from bloombee_amd.parallel.sequence import (cp_prefill_llama,
                                                ring_attention_local)

    assert ops.HAVE_HIP_OPS, (
        "HIP extension must be built and loadable on a GPU box (fail-loud policy)"
    )

DEV = "cuda:0"


@pytest.mark.parametrize("window", [0, 50])
@pytest.mark.parametrize("world,t_loc", rc.RINGS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", rc.HEADS)
def test_ring_local_matches_oracle(Hq, Hkv, D, world, t_loc, window):
    c = rc.build(Hq, Hkv, D, world * t_loc, window)
    got = ring_attention_local(c.q.to(DEV), c.k.to(DEV), c.v.to(DEV), world,
                               c.scale, window)
    rc.check(got.cpu(), c, f"local {Hq}/{Hkv} D{D} {world}x{t_loc} w{window}")


@pytest.mark.parametrize("order,strided", [("oldest", False), ("newest", False),
                                           ("oldest", True)])
@pytest.mark.parametrize("D", [64, 128])
def test_fold_block_orders(D, order, strided):
    """Window 50 over 4 shards of 40: folded oldest-first, ranks 2 and 3 meet
    rows with no visible key in their first fold (rank 3: all of them)."""
    world, Tl, window = 4, 40, 50
    c = rc.build(4, 2, D, world * Tl, window)
    q, k, v = c.q.to(DEV), c.k.to(DEV), c.v.to(DEV)
    if strided:  # views into one fused (B, T, Hq + 2 Hkv, D) projection output
        buf = torch.cat([q, k, v], dim=1).permute(0, 2, 1, 3).contiguous()
        q, k, v = buf.permute(0, 2, 1, 3).split([4, 2, 2], dim=1)
        assert not q.is_contiguous()
    outs = []
    for r in range(world):
        srcs = list(range(r + 1)) if order == "oldest" else list(range(r, -1, -1))
        state = None
        for src in srcs:
            sl = slice(src * Tl, (src + 1) * Tl)
            state = ops.attn_ring_fold(q[:, :, r * Tl:(r + 1) * Tl], k[:, :, sl],
                                       v[:, :, sl], state, r * Tl, src * Tl,
                                       c.scale, window, last=src == srcs[-1])
        outs.append(state.permute(0, 2, 1, 3))
    rc.check(torch.cat(outs, dim=2).cpu(), c, f"fold {order} D{D} strided={strided}")


class _Counter:
    def __init__(self, ext):
        self._ext, self.calls = ext, 0

    def attn_ring_fold(self, *a):
        self.calls += 1
        return self._ext.attn_ring_fold(*a)


def test_switch(monkeypatch):
    counter = _Counter(interface.hip_ring)
    monkeypatch.setattr(interface, "hip_ring", counter)
    monkeypatch.delenv("BBAMD_RING_KERNEL", raising=False)
    c = rc.build(4, 2, 64, 160, 0)
    q, k, v = c.q.to(DEV), c.k.to(DEV), c.v.to(DEV)
    rc.check(ring_attention_local(q, k, v, 4, c.scale).cpu(), c, "switch on")
    assert counter.calls == 1 + 2 + 3 + 4, "one launch per visible block"
    monkeypatch.setenv("BBAMD_RING_KERNEL", "0")
    off = ring_attention_local(q, k, v, 4, c.scale)
    assert counter.calls == 10, "switch off must take the composition"
    assert off.is_cuda
    rc.check(off.cpu(), c, "switch off")


@pytest.mark.parametrize("model", ["llama-tiny", "qwen3-tiny"])
def test_cp_prefill_matches_prefill(model):
    from bloombee_amd.engine import BlockStack
    from bloombee_amd.models.base import resolve_config

    cfg = resolve_config(model)
    stack = BlockStack(cfg, 0, cfg.num_hidden_layers, device=DEV, seed=5)
    ha, hb = (stack.make_kv(1 << 10).allocate(2, 64) for _ in range(2))
    gen = torch.Generator().manual_seed(1)
    x = (torch.randn(2, 40, cfg.hidden_size, generator=gen) * 0.1).to(cfg.dtype).to(DEV)
    x1 = (torch.randn(2, 1, cfg.hidden_size, generator=gen) * 0.1).to(cfg.dtype).to(DEV)
    ha.extend(40)
    hb.extend(40)
    got = cp_prefill_llama(stack, ha, x, rank=0, world=1)
    want = stack.forward_inference(x, hb, torch.zeros(2, dtype=torch.int32, device=DEV))
    err = float((got.float() - want.float()).abs().max())
    print(f"[ring] {model} cp prefill: max abs diff {err:.2e}")
    assert torch.allclose(got.float(), want.float(), atol=3e-2), err
    ha.extend(1)
    hb.extend(1)
    sp = torch.full((2,), 40, dtype=torch.int32, device=DEV)
    ya, yb = stack.forward_inference(x1, ha, sp), stack.forward_inference(x1, hb, sp)
    err = float((ya.float() - yb.float()).abs().max())
    print(f"[ring] {model} decode after cp prefill: max abs diff {err:.2e}")
    assert torch.allclose(ya.float(), yb.float(), atol=3e-2), err
