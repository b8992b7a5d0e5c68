"""CPU checks of the attention edge cases (tests/attn_cases.py).

1. The project's reference `ref.attn_paged` (fp32) matches the independent
   dense fp64 reference to 1e-5 on every case, window and ALiBi included.
2. Sensitivity guards: every mutation of the reference that applies to a case
   moves the fp64 output by more than 10 x tol(case) in at least one element,
   so a kernel with that defect cannot pass the GPU comparison. Which
   mutation applies to which case family is stated in `attn_cases.applicable`:

     every case             drop_newest, past_ctx, neighbour_row
     window != 1            zero_q, swap_pages (some row with >= 2 pages)
     0 < window < max ctx   window_lo_minus, window_lo_plus
     Hkv > 1                wrong_kv_head
     ALiBi                  alibi_next_head
"""
import pytest
import torch

import attn_cases as ac
from bloombee_amd.ops import reference as ref


@pytest.mark.parametrize("spec", ac.ALL_CASES, ids=ac.ids(ac.ALL_CASES))
def test_project_reference_matches_dense(spec):
    case = ac.build(spec)
    want = ac.dense_ref(case)
    got = ref.attn_paged(
        case.q.float(), case.k_pages.float(), case.v_pages.float(),
        case.page_table, case.q_start.long(), case.scale,
        sliding_window=spec.window if spec.window > 0 else None,
        alibi_slopes=case.slopes)
    err = float((got.double() - want).abs().max())
    assert err <= 1e-5, f"{spec.name}: max err {err:.3e}"


def test_pool_is_poisoned_everywhere_but_live_slots():
    """Builder invariant: every non-live slot is +-64, finite, in K and V."""
    for spec in (ac.DECODE_BOUNDARY[0], ac.PREFILL_SHAPES[3]):
        case = ac.build(spec)
        dead = ~case.live                                   # (np, P)
        kd = case.k_pages.float().permute(0, 2, 1, 3)[dead]
        vd = case.v_pages.float().permute(0, 3, 1, 2)[dead]
        assert bool((kd.abs() == ac.POISON).all())
        assert bool((vd.abs() == ac.POISON).all())
        assert int(case.live.sum()) == int(case.ctx.sum())


def test_scores_are_peaked():
    """Natural-log scores have std ~2 before planting moves a few of them."""
    case = ac.build(ac.DECODE_MATRIX[3])
    b, ctx = 0, int(case.ctx[0])
    s = (case.q[b, 0, 0].double() @ case.k[b, 0, :ctx].T) * case.scale
    keep = torch.ones(ctx, dtype=torch.bool)
    keep[case.planted[b]] = False
    assert 1.5 < float(s[keep].std()) < 2.5


_GUARDS = [(s, m) for s in ac.ALL_CASES for m in ac.applicable(s)]


@pytest.mark.parametrize("spec,mutation", _GUARDS,
                         ids=[f"{s.name}-{m}" for s, m in _GUARDS])
def test_sensitivity_guard(spec, mutation):
    case = ac.build(spec)
    want = ac.dense_ref(case)
    mut = ac.dense_ref(case, **ac.MUTATIONS[mutation])
    ratio = float(((mut - want).abs() / ac.tol(case)).max())
    assert ratio > 10.0, (
        f"{spec.name}: {mutation} moves the output by only {ratio:.2f} x tol")


def test_required_guards_are_listed():
    """The guards the edge tests rely on apply where they should."""
    for spec in ac.ALL_CASES:
        names = ac.applicable(spec)
        assert {"drop_newest", "past_ctx", "neighbour_row"} <= set(names)
        if spec.window != 1:
            assert "zero_q" in names
            if max(r[0] + r[1] for r in spec.rows) >= 2 * ac.P:
                assert "swap_pages" in names
        if 0 < spec.window < 1000:
            assert {"window_lo_minus", "window_lo_plus"} <= set(names)
        if spec.alibi:
            assert "alibi_next_head" in names
        if spec.Hkv > 1:
            assert "wrong_kv_head" in names
