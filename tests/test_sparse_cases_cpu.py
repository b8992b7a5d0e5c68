"""CPU guards for the top-k sparse decode attention cases
(tests/sparse_cases.py) and the CPU side of the dispatch.

* ref.attn_paged_topk (fp32) stays within the derived tolerance of the fp64
  oracle on every case.
* Every mutation of the oracle (one deliberate error each) lands >= 4 x tol
  away on every case that names it, so the GPU test that uses these cases
  can tell the defect apart.
* Wiring: ops.attn_paged_qkv honours set_attn_sparsity on T == 1, window 0
  (llama, qwen3, mixtral, falcon, template, TP all decode through it) and
  stays dense for sparsity 1.0 and for sliding-window layers.
"""
import pytest
import torch

import sparse_cases as sc
from bloombee_amd import ops
from bloombee_amd.ops import reference as ref


def _ref_topk(case):
    return ref.attn_paged_topk(
        case.q.float(), case.k_pages, case.v_pages, case.page_table, case.ctx,
        case.sparsity, case.scale, alibi_slopes=case.slopes)


@pytest.mark.parametrize("spec", sc.CASES, ids=sc.ids(sc.CASES))
def test_reference_matches_oracle(spec):
    ratio, where = sc.worst(_ref_topk(sc.build(spec)), spec)
    print(f"[sparse-cases] {spec.name}: ref err/tol {ratio:.3f} at {where}")
    assert ratio <= 1.0, f"{spec.name}: err / tol = {ratio:.3f} at {where}"


@pytest.mark.parametrize("grow", (1, 2))
def test_grown_base_case_shares_inputs(grow):
    """build(spec, grow) only appends positions: what graph replay relies on."""
    a, b = sc.build(sc.BASE), sc.build(sc.BASE, grow)
    assert torch.equal(a.q, b.q) and torch.equal(a.page_table, b.page_table)
    assert torch.equal(b.ctx, a.ctx + grow)
    assert torch.equal(a.k, b.k) and torch.equal(a.v, b.v)
    kk = lambda c: [sc.kkeep_of(c.sparsity, int(x)) for x in c.ctx]
    assert kk(a) != kk(b)
    ratio, where = sc.worst(_ref_topk(b), sc.BASE, grow)
    assert ratio <= 1.0, (ratio, where)


_PAIRS = [(s, m) for s in sc.CASES for m in s.covers]


@pytest.mark.parametrize("spec,mutation", _PAIRS,
                         ids=[f"{s.name}-{m}" for s, m in _PAIRS])
def test_mutation_is_visible(spec, mutation):
    case = sc.build(spec)
    want, tol = sc.expected(spec)
    got = sc.oracle(case, **sc.MUTATIONS[mutation])
    ratio = float(((got - want).abs() / tol).max())
    print(f"[sparse-cases] {spec.name}: {mutation} moves the output by "
          f"{ratio:.1f} x tol")
    assert ratio >= 4.0, f"{spec.name} cannot see {mutation}: {ratio:.2f} x tol"


def test_every_mutation_has_a_case():
    assert {m for _, m in _PAIRS} == set(sc.MUTATIONS)


# ---------------------------------------------------------------------------
# dispatch on the CPU
# ---------------------------------------------------------------------------

def _qkv_call(case, window=0):
    s = case.spec
    return ops.attn_paged_qkv(
        sc.qkv_buffer(case).float(), s.Hq, s.Hkv, case.k_pages, case.v_pages,
        case.page_table, case.ctx - 1, scale=case.scale, window=window)


def _flat(out, case):
    s = case.spec
    return out.permute(0, 2, 1, 3).reshape(case.B, 1, s.Hq * s.D)


def test_attn_paged_qkv_honours_sparsity():
    case = sc.build(sc.BASE)
    dense = _qkv_call(case)
    ops.set_attn_sparsity(case.sparsity)
    try:
        got = _qkv_call(case)
    finally:
        ops.set_attn_sparsity(1.0)
    assert got.shape == dense.shape
    assert torch.equal(got, _flat(_ref_topk(case), case))
    _, tol = sc.expected(sc.BASE)
    moved = float(((got.double() - dense.double()).abs()
                   .view(case.B, sc.BASE.Hq, 1, sc.BASE.D) / tol).max())
    assert moved > 1.0, f"sparse and dense differ by only {moved:.2f} x tol"
    ratio, where = sc.worst(got, sc.BASE)
    assert ratio <= 1.0, (ratio, where)


def test_attn_paged_qkv_dense_at_sparsity_one_and_under_window():
    case = sc.build(sc.BASE)
    s = case.spec
    q = case.q.float()

    def dense(window):
        out = ref.attn_paged(q, case.k_pages, case.v_pages, case.page_table,
                             (case.ctx - 1).long(), case.scale,
                             sliding_window=window if window > 0 else None)
        return _flat(out, case)

    ops.set_attn_sparsity(1.0)
    assert torch.equal(_qkv_call(case), dense(0))
    ops.set_attn_sparsity(0.25)
    try:
        got_w = _qkv_call(case, window=7)
        got_d = ops.attn_decode(q, case.k_pages, case.v_pages, case.page_table,
                                case.ctx, case.scale, window=7)
    finally:
        ops.set_attn_sparsity(1.0)
    assert torch.equal(got_w, dense(7))
    assert torch.equal(_flat(got_d, case), dense(7))
    assert s.Hq * s.D == got_w.shape[-1]


def test_kernel_gate_covers_head_dim_and_page_size():
    """Shapes the kernels are not written for run the composition: any head
    dim but 64 / 128 / 256, and any page size but 16 (BBAMD_KV_PAGE_SIZE may
    be any divisor of 32)."""
    from bloombee_amd.ops import interface

    old = interface._SPARSE_KERNEL
    interface._SPARSE_KERNEL = True
    try:
        for D in (64, 128, 256):
            assert interface._sparse_kernel_ok(D, 16)
            for P in (1, 2, 4, 8, 32):
                assert not interface._sparse_kernel_ok(D, P)
        for D in (32, 80, 96, 512):
            assert not interface._sparse_kernel_ok(D, 16)
        interface._SPARSE_KERNEL = False
        assert not interface._sparse_kernel_ok(128, 16)
    finally:
        interface._SPARSE_KERNEL = old


def test_page_size_8_runs_the_reference():
    """The public entries at a page size the kernels do not cover: same pool
    re-cut into 8-slot pages gives the same sparse result."""
    case = sc.build(sc.BASE)
    s = case.spec
    kp8, vp8, pt8 = sc.repaged8(case)
    ops.set_attn_sparsity(case.sparsity)
    try:
        got = ops.attn_decode(case.q.float(), kp8, vp8, pt8, case.ctx,
                              case.scale)
        got_qkv = ops.attn_paged_qkv(
            sc.qkv_buffer(case).float(), s.Hq, s.Hkv, kp8, vp8, pt8,
            case.ctx - 1, scale=case.scale)
    finally:
        ops.set_attn_sparsity(1.0)
    assert torch.equal(got, _ref_topk(case))
    assert torch.equal(got_qkv, _flat(got, case))


@pytest.mark.parametrize("model", ["llama-tiny", "qwen3-tiny", "mixtral-tiny",
                                   "falcon-tiny", "bloom-tiny"])
def test_sparsity_changes_the_decode_step_of_every_family(model):
    """llama, qwen3, mixtral and falcon decode through ops.attn_paged_qkv,
    bloom (ALiBi) through ops.attn_paged: one decode step after a 24-token
    prefill must differ between sparsity 1.0 and 0.25 (kkeep = 7 of 25),
    while the prefill itself does not depend on the knob."""
    from bloombee_amd.engine import LocalEngine

    eng = LocalEngine(model, device="cpu", seed=1, kv_max_tokens=4096)
    B, T = 2, 24
    gen = torch.Generator().manual_seed(5)
    h = (torch.randn(B, T + 1, eng.config.hidden_size, generator=gen)
         ).to(eng.config.dtype)

    def run(frac):
        ops.set_attn_sparsity(frac)
        try:
            kv = eng.kv_pool.allocate(B, 64)
            kv.extend(T)
            pre = eng.stack.forward_inference(
                h[:, :T].clone(), kv, torch.zeros(B, dtype=torch.int32))
            kv.extend(1)
            dec = eng.stack.forward_inference(
                h[:, T:].clone(), kv, torch.full((B,), T, dtype=torch.int32))
            kv.close()
        finally:
            ops.set_attn_sparsity(1.0)
        return pre.float(), dec.float()

    pre_d, dec_d = run(1.0)
    pre_s, dec_s = run(0.25)
    assert torch.equal(pre_d, pre_s)
    assert not torch.equal(dec_d, dec_s), f"{model}: the knob changed nothing"
