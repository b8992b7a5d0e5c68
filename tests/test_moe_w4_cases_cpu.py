"""CPU checks of the exact-arithmetic grouped W4 MoE cases
(tests/moe_w4_cases.py).

1. Builder invariants hold for every case (A exact in f16 and bf16, the
   expectation exact in bf16, sum|a w| / 0.25 < 2^24), poison sits where the
   case says, and scale / zero vary the way the W4 guards need: within a
   128-k slice, by row, by expert, and zero independently of scale.
2. For the four pinned shape / count combinations: |want| <= 244, between
   1.6 % and 3.1 % of the outputs are zero, and `ref.quant4_unpack`
   reproduces W exactly.
3. `ref.moe_gemm_grouped_w4` and `ops.moe_gemm_grouped_w4` on the CPU equal
   the fp64 expectation bit for bit.
4. Sensitivity guards: every mutation that applies to a case (see
   `moe_w4_cases.applicable`) moves at least one expected element by at
   least one unit of that element, so a kernel with that defect cannot pass
   the GPU test's `torch.equal`.
"""
import pytest
import torch

import moe_w4_cases as mc
from bloombee_amd import ops
from bloombee_amd.ops import reference as ref

BF = torch.bfloat16
ALL = mc.CASES


@pytest.mark.parametrize("spec", ALL, ids=mc.ids(ALL))
def test_builder_invariants(spec):
    c = mc.build(spec)                       # build() itself asserts 1.
    mc.check_invariants(c)
    named = torch.zeros(c.A.shape[0], dtype=torch.bool)
    named[c.rowmap.long() if c.rowmap is not None else torch.arange(c.S)] = True
    assert bool((c.A[~named].abs() == mc.POISON).all()) and bool((~named).any())
    assert bool((c.A[named].abs() <= 9).all())
    for e, n in enumerate(spec.counts):
        poisoned = bool((c.scale[e] == mc.POISON_SCALE).all()
                        and (c.zero[e] == mc.POISON_ZERO).all())
        assert poisoned == (n == 0)
    # fp32 in a different summation order equals fp64: the sums are exact
    half = spec.K // 2
    for e, n in enumerate(spec.counts):
        if n == 0:
            continue
        a = c.A[named].float()
        w = c.W[e].float()
        two = a[:, half:] @ w[:, half:].T + a[:, :half] @ w[:, :half].T
        assert torch.equal(two.double(), c.A[named] @ c.W[e].T)


@pytest.mark.parametrize("spec", ALL, ids=mc.ids(ALL))
def test_layout_has_the_variation_the_guards_need(spec):
    c = mc.build(spec)
    live = [e for e, n in enumerate(spec.counts) if n]
    s, z = c.scale[live], c.zero[live]
    z0 = -z / s
    assert bool((s[..., 0::2] != s[..., 1::2]).all())       # within a 128-k slice
    if s.shape[-1] >= 4:                                    # neighbouring slices
        assert bool((s[..., 0:-2] != s[..., 2:]).all())
    assert set(z0.unique().tolist()) == {7.0, 8.0}
    for val in s.unique().tolist():                         # zero independent of scale
        assert set(z0[s == val].unique().tolist()) == {7.0, 8.0}
    for i in range(len(live)):
        assert len(set(s[i, :, 0].tolist())) > 1            # by row
    # by expert: no live expert shares its scale or zero rows with expert 0
    for e in live:
        if e != 0:
            assert not torch.equal(c.scale[e], c.scale[0])
            assert not torch.equal(c.zero[e], c.zero[0])
    assert torch.equal(c.scale.half().double(), c.scale)
    assert torch.equal(c.zero.half().double(), c.zero)


@pytest.mark.parametrize("spec", mc.PINNED, ids=mc.ids(mc.PINNED))
def test_pinned_statistics(spec):
    c = mc.build(spec)
    assert (spec.N, spec.K, spec.counts) in [
        (128, 128, (0, 33, 1, 17)), (576, 384, (65, 16, 32, 0)),
        (128, 1024, (1, 0, 70, 17, 0, 64, 33, 16)),
        (576, 2048, (32, 33, 0, 0, 65, 1, 16, 0))]
    unscaled = c.want / mc.out_unit(c)
    assert float(unscaled.abs().max()) <= 244
    zeros = float((c.want == 0).double().mean())
    print(f"{spec.name}: max |want| {float(unscaled.abs().max())}, zeros {zeros:.4f}")
    assert 0.016 <= zeros <= 0.031
    E, N, K = c.E, spec.N, spec.K
    w = ref.quant4_unpack(c.packed.reshape(E, N, K // 64, 32), c.scale.half(),
                          c.zero.half(), torch.float64)
    assert torch.equal(w.reshape(E, N, K), c.W)


def _inputs(c):
    sc = c.slot_scale.float() if c.slot_scale is not None else None
    return (c.A.to(BF), c.packed, c.scale.half(), c.zero.half(), c.off,
            c.rowmap, sc)


@pytest.mark.parametrize("spec", ALL, ids=mc.ids(ALL))
def test_references_equal_the_expectation(spec):
    c = mc.build(spec)
    a, packed, scale, zero, off, rm, sc = _inputs(c)
    got = ref.moe_gemm_grouped_w4(a, packed, scale, zero, off, rm, sc, c.S)
    assert got.dtype == BF and torch.equal(got.double(), c.want)
    got = ops.moe_gemm_grouped_w4(a, packed, scale, zero, off, rowmap=rm,
                                  slot_scale=sc, S=c.S, mchunks=c.mchunks)
    assert got.dtype == BF and torch.equal(got.double(), c.want)


def test_every_mutation_is_exercised():
    seen = set()
    for spec in ALL:
        seen.update(mc.applicable(spec))
    assert seen == set(mc.MUTATIONS)
    # split-K: ksplit 2 and 3 with an uneven last split, and the op's own rule
    lens = {s.name: [b - a for a, b in mc.splits_of(s)] for s in ALL}
    assert any(s.ksplit == 2 and len(set(lens[s.name])) == 2 for s in ALL)
    assert any(s.ksplit == 3 and len(set(lens[s.name])) == 2 for s in ALL)
    assert any(s.ksplit == 0 and len(lens[s.name]) > 1 for s in ALL)
    assert any(s.ksplit == 0 and len(lens[s.name]) == 1 for s in ALL)


_PAIRS = [(s, m) for s in ALL for m in mc.applicable(s)]


@pytest.mark.parametrize("spec,mut", _PAIRS,
                         ids=[f"{s.name}-{m}" for s, m in _PAIRS])
def test_mutation_moves_the_expectation(spec, mut):
    c = mc.build(spec)
    bad = mc.model(c, mut)
    moved = (bad - c.want).abs() >= mc.out_unit(c)
    assert bool(moved.any()), f"{spec.name}: {mut} leaves every element in place"
    # and the move survives the bf16 rounding of the output
    assert not torch.equal(bad.to(BF), c.want.to(BF))
