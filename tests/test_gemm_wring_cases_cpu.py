"""CPU checks of the W-ring cases (tests/wring_cases.py).

`gemm_cases.build` asserts its invariants for every new spec (expected tensor
exactly representable in bf16, every f32 partial sum exact), and every entry
of `gemm_cases.MUTATIONS` that applies to a spec moves at least one expected
element by a whole unit: test_gpu_gemm_wring.py compares with `torch.equal`,
so a ring that loses a set, a stage, a split, a row or a stripe cannot pass.
"""
import pytest
import torch

import gemm_cases as gc
import wring_cases as wc

_GUARDS = [(s, m) for s in wc.ALL_SPECS for m in gc.applicable(s)]


@pytest.mark.parametrize("spec", wc.ALL_SPECS, ids=gc.ids(wc.ALL_SPECS))
def test_builder_invariants(spec):
    c = gc.build(spec)                       # asserts the builder invariants
    gc.check_invariants(c)
    assert gc.skinny_is_v2(spec.K)
    assert not bool((c.want == 0).all())
    assert bool((c.Abuf[spec.M:].abs() == gc.POISON).all())


@pytest.mark.parametrize("spec,mutation", _GUARDS,
                         ids=[f"{s.name}-{m}" for s, m in _GUARDS])
def test_sensitivity_guard(spec, mutation):
    c = gc.build(spec)
    bf = torch.bfloat16
    assert torch.equal(gc.model(c), c.want)
    if mutation == "ssout_wave_lost":
        assert not torch.equal(gc.model_ss(c, mutation).float(), c.want_ss.float())
        return
    mut = gc.model(c, mutation)
    moved = (mut - c.want).abs() >= gc.out_unit(c)
    assert bool(moved.any()), f"{spec.name}: {mutation} changes nothing"
    assert not torch.equal(mut.to(bf), c.want.to(bf))


def test_stage_counts_and_options_are_covered():
    """Every remainder of a 2-, 3- and 4-stage ring period, and each option
    the GPU test is to reach."""
    single = {wc.stages(s)[0] for s in wc.ALL_SPECS if s.ksplit == 1}
    assert single >= {1, 2, 3, 4, 5, 7, 9}
    assert [2, 1] in [wc.stages(s) for s in wc.ALL_SPECS]
    assert [4, 3] in [wc.stages(s) for s in wc.ALL_SPECS]
    assert {s.M for s in wc.ALL_SPECS} == {1, 17, 32}
    assert {s.N for s in wc.ALL_SPECS} == {64, 576}
    assert gc.has_remap(next(s for s in wc.SPECS if s.N == 576))
    assert any(s.res and s.ss_out and s.ksplit == 1 for s in wc.SPECS)
    assert any(s.res and s.ss_out and s.ksplit > 1 for s in wc.SPECS)
    assert any(s.kind == "norm" and s.ss_in for s in wc.SPECS)
    assert any(s.kind == "norm" and s.ksplit > 1 for s in wc.SPECS)
    for s in wc.ALL_SPECS:
        names = set(gc.applicable(s))
        assert {"drop_last_slice", "row_past_M"} <= names
        if wc.stages(s)[0] >= 2:
            assert "drop_stage_head" in names
        if s.ksplit > 1:
            assert "last_split_lost" in names


@pytest.mark.parametrize("spec", wc.DEFER_SPECS, ids=gc.ids(wc.DEFER_SPECS))
def test_slab_model(spec):
    """The slabs are exact in f32 and sum to the expected output; losing a
    split's last 32 k moves that slab alone."""
    c = gc.build(spec)
    slabs = wc.slab_model(c)
    assert len(slabs) == spec.ksplit
    assert torch.equal(sum(slabs), c.want)
    for s in slabs:
        assert torch.equal(s.float().double(), s) and bool((s != 0).any())
    (a, b) = gc.splits_of(spec)[0]
    A = c.Abuf[: spec.M]
    short = A[:, a:b - 32] @ c.W[:, a:b - 32].T
    assert bool(((short - slabs[0]).abs() >= 1).any())
