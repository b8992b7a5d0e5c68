"""CPU checks of the fused-epilogue test cases (tests/fused_cases.py): the
expected tensors are what they claim to be and each modelled defect of the
SwiGLU-fused gate_up GEMM changes at least one expected bf16 element. No GPU.
"""
import pytest
import torch

import fused_cases as fc
import gemm_cases as gc

BF = torch.bfloat16


@pytest.mark.parametrize("spec", fc.SWIGLU_SPECS, ids=gc.ids(fc.SWIGLU_SPECS))
def test_swiglu_case_is_sound(spec):
    c = fc.build_swiglu(spec)
    I = spec.N // 2
    gu = fc.gate_up_model(c)
    # the gate_up the unfused kernel stores is exact in bf16
    assert torch.equal(gu.to(BF).double(), gu)
    assert torch.equal(gu, c.want)
    g, u = gu[:, :I], gu[:, I:]
    # gate and up differ, and vary by column
    assert float((g != u).double().mean()) > 0.5
    assert bool((g.std(1) > 0).all()) and bool((u.std(1) > 0).all())
    # against the torch definition of the activation
    want = torch.nn.functional.silu(g) * u
    assert torch.allclose(c.want_act, want, rtol=1e-12, atol=0)
    assert float((c.want_act != 0).double().mean()) > 0.5


@pytest.mark.parametrize("spec", fc.SWIGLU_SPECS, ids=gc.ids(fc.SWIGLU_SPECS))
def test_swiglu_mutations_move_the_expectation(spec):
    c = fc.build_swiglu(spec)
    want = c.want_act.to(BF)
    bound = fc.act_bound(c)
    for mut in fc.applicable(spec):
        got = fc.act_model(c, mut)
        assert not torch.equal(got.to(BF), want), f"{spec.name}: {mut} is invisible"
        # and by more than the fp64 comparison forgives
        assert bool(((got - c.want_act).abs() > bound).any()), \
            f"{spec.name}: {mut} hides inside the fp64 bound"


def test_swiglu_mutation_list_is_complete():
    seen = set()
    for spec in fc.SWIGLU_SPECS:
        seen.update(fc.applicable(spec))
    assert seen == set(fc.SWIGLU_MUTATIONS)


@pytest.mark.parametrize("N,K,ks", [(N, K, ks) for N in fc.REDUCE_N
                                    for K, ks in fc.REDUCE_KS])
def test_reduce_case_is_sound(N, K, ks):
    c = fc.build_reduce(N, K, ks)
    assert len([s for s in gc.splits_of(c.spec) if s[1] > s[0]]) == ks
    assert torch.equal(c.want_plain.to(BF).double(), c.want_plain)
    assert torch.equal(c.want_plain, c.Abuf[:32] @ c.W.T)
    # losing the last split is visible in every row
    lost = gc.model(c, "last_split_lost")
    assert bool((lost != c.want).any(1).all())
