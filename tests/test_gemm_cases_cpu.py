"""CPU checks of the exact-arithmetic GEMM cases (tests/gemm_cases.py).

1. Builder invariants hold for every case: the expected tensor is exactly
   representable in bf16, every f32 partial sum is exact (sum|a*w| / unit
   < 2^24), fp32 matmul reproduces the fp64 expectation bit for bit, poison
   sits where the case says, and the W4 scale/zero layout has the variation
   the W4 guards need.
2. The project's references (`ref.moe_gemm_grouped`, `ref.quant4_unpack` +
   matmul, `ref.rms_norm` + `F.linear`) reproduce the expected tensors
   exactly.
3. Sensitivity guards: every mutation that applies to a case changes at
   least one expected element by at least one unit of that element (its
   bf16 value differs). The GPU comparison is `torch.equal`, so a kernel
   with that defect cannot pass. Which mutation applies where is stated in
   `gemm_cases.applicable`:

     every case                 drop_last_slice
     first split >= 512 k       drop_stage_head
     >= 2 non-empty splits      last_split_lost
     XCD remap not identity     stripe_unremapped
     non-MoE                    row_past_M; M > 16: row_clamp16;
                                bias: bias_by_row; res, N >= 128:
                                residual_wrong_stripe
     norm, M > 1                invr_neighbour_row; ss_in: ss_in_ignored;
                                ss_in > 32, % 32 != 0: ss_stripe_tail_lost
     ss_out                     ssout_wave_lost
     W4                         w4_scale_neighbour, w4_zero_neighbour,
                                w4_nibble_swap, w4_group_straddle
     MoE                        expert_next; rowmap: rowmap_ignored; scale:
                                scale_by_local_m; a group > 32 rows:
                                chunk_rows_from_first; a group followed by
                                another slot: group_end_plus_one
"""
import pytest
import torch
import torch.nn.functional as F

import gemm_cases as gc
from bloombee_amd.ops import reference as ref


@pytest.mark.parametrize("spec", gc.ALL_CASES, ids=gc.ids(gc.ALL_CASES))
def test_builder_invariants(spec):
    c = gc.build(spec)                       # build() itself asserts 1.
    gc.check_invariants(c)
    assert not bool((c.want == 0).all())
    if spec.kind == "moe":
        named = torch.zeros(c.A.shape[0], dtype=torch.bool)
        named[c.rowmap.long() if c.rowmap is not None else torch.arange(c.S)] = True
        assert bool((c.A[~named].abs() == gc.POISON).all()) and bool((~named).any())
        assert bool((c.A[named].abs() <= 3).all())
        for e, n in enumerate(spec.counts):
            assert bool((c.W[e].abs() == gc.POISON).all()) == (n == 0)
        return
    assert bool((c.Abuf[spec.M:].abs() == gc.POISON).all())
    assert c.Abuf.shape[0] > spec.M
    # fp32 in a different summation order equals fp64: the sums are exact
    W = c.Wfold if spec.kind == "norm" else c.W
    a32, w32 = c.Abuf[:spec.M].float(), W.float()
    half = spec.K // 2
    two = a32[:, half:] @ w32[:, half:].T + a32[:, :half] @ w32[:, :half].T
    assert torch.equal(two.double(), c.Abuf[:spec.M] @ W.T)


@pytest.mark.parametrize("spec", gc.W4, ids=gc.ids(gc.W4))
def test_w4_layout_has_the_variation_the_guards_need(spec):
    c = gc.build(spec)
    s, z0 = c.scale, c.z0
    assert bool((s[:, 0::2] != s[:, 1::2]).all())          # within a 128-k slice
    if s.shape[1] >= 4:                                    # neighbouring slices
        assert bool((s[:, 0:-2] != s[:, 2:]).all())
    assert len(set(s[:, 0].tolist())) > 1                  # by row
    assert set(z0.unique().tolist()) == {7.0, 8.0}
    # zero is not a function of scale: both z0 occur under every scale value
    for val in s.unique().tolist():
        assert set(z0[s == val].unique().tolist()) == {7.0, 8.0}
    # exact in f16
    assert torch.equal(c.scale.half().double(), c.scale)
    assert torch.equal(c.zero.half().double(), c.zero)
    assert torch.equal(c.Abuf[:spec.M].half().double(), c.Abuf[:spec.M])


@pytest.mark.parametrize("spec", gc.NORM, ids=gc.ids(gc.NORM))
def test_norm_case_structure(spec):
    c = gc.build(spec)
    M, K = spec.M, spec.K
    A = c.Abuf[:M]
    assert torch.equal(A.abs(), (2.0 ** c.j.double())[:, None].expand(M, K))
    assert bool(((c.nw == 1) | (c.nw == 2)).all())
    if spec.ss_in:
        ss = c.ss_in[:, :M]
        assert torch.equal(ss.float().double(), ss)
        assert torch.equal(ss.sum(0), K * 4.0 ** c.jin.double())
        assert bool((ss > 0).all())
        if spec.ss_in > 1:                  # unequal stripes, different per row
            assert bool((ss[0] != ss[1]).all())
            if M > 2:
                assert not torch.equal(ss[:, 0] * 4.0 ** (c.jin[2] - c.jin[0]).double(),
                                       ss[:, 2])
        if M > 1:
            assert bool((c.jin != c.j).any())


@pytest.mark.parametrize("spec", gc.ALL_CASES, ids=gc.ids(gc.ALL_CASES))
def test_project_reference_reproduces_expected(spec):
    c = gc.build(spec)
    bf = torch.bfloat16
    if spec.kind == "moe":
        got = ref.moe_gemm_grouped(c.A.to(bf), c.W.to(bf), c.off, c.rowmap,
                                   c.scale.float() if c.scale is not None else None,
                                   c.S)
        assert torch.equal(got.double(), c.want)
        return
    M, N, K = spec.M, spec.N, spec.K
    x = c.Abuf[:M].to(bf)
    if spec.kind == "w4":
        w = ref.quant4_unpack(c.packed.reshape(N, K // 64, 32), c.scale.half(),
                              c.zero.half(), dtype=torch.float32).reshape(N, K)
        assert torch.equal(w.double(), c.W)
        x = x.float()
    elif spec.kind == "norm":
        w = c.W.float()
        # the project reference has no ss_in; ss_in sums to K 4^j' (checked in
        # test_norm_case_structure), so the kernel's A 2^-j' nw is
        # rms_norm(A) 2^(j - j')
        x = ref.rms_norm(x, c.nw.to(bf), 0.0).float() \
            * 2.0 ** (c.j - c.jin).float()[:, None]
    else:
        w = c.W.float()
        x = x.float()
    got = F.linear(x, w, c.bias.float() if c.bias is not None else None)
    if c.res is not None:
        got = got + c.res.float()
    assert torch.equal(got.to(bf).double(), c.want)


_GUARDS = [(s, m) for s in gc.ALL_CASES for m in gc.applicable(s)]


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


def test_chain_case_builds():
    """build_chain asserts its own invariants (exact ss, representable h and
    output); the per-stripe sums must differ between stripes and rows."""
    c = gc.build_chain()
    assert bool((c.A1buf[c.M:].abs() == gc.POISON).all())
    assert not torch.equal(c.ss[0], c.ss[1])
    assert len({tuple((c.ss[:, m] / c.ss[:, m].sum()).tolist()) for m in range(c.M)}) > 1
    assert float((c.want == 0).double().mean()) < 0.1


def test_every_mutation_is_exercised():
    used = {m for _, m in _GUARDS}
    assert used == set(gc.MUTATIONS), set(gc.MUTATIONS) - used


def test_required_guards_are_listed():
    """A case cannot quietly lose the guards the GPU tests rely on."""
    for spec in gc.ALL_CASES:
        names = set(gc.applicable(spec))
        assert "drop_last_slice" in names
        live = [s for s in gc.splits_of(spec) if s[1] > s[0]]
        if len(live) > 1:
            assert "last_split_lost" in names
        if spec.kind != "moe":
            assert "row_past_M" in names
            if spec.M > 16:
                assert "row_clamp16" in names
            if spec.bias:
                assert "bias_by_row" in names
            if spec.res and spec.N >= 128:
                assert "residual_wrong_stripe" in names
        if spec.kind == "w4":
            assert {"w4_scale_neighbour", "w4_zero_neighbour", "w4_nibble_swap",
                    "w4_group_straddle"} <= names
        if spec.kind == "norm" and spec.M > 1:
            assert "invr_neighbour_row" in names
            if spec.ss_in:
                assert "ss_in_ignored" in names
            if spec.ss_in in (36, 100):
                assert "ss_stripe_tail_lost" in names
        if spec.ss_out:
            assert "ssout_wave_lost" in names
        if spec.kind == "moe":
            assert "expert_next" in names
            if max(spec.counts) > 32:
                assert "chunk_rows_from_first" in names
            if spec.rowmap:
                assert "rowmap_ignored" in names
            if spec.scale:
                assert "scale_by_local_m" in names
            assert "group_end_plus_one" in names
    # the paths the suite exists for are reached by some case
    r = {(s.kind, (s.N // 64) % 8) for s in gc.ALL_CASES if gc.has_remap(s)}
    for kind in ("dense", "norm", "w4", "moe"):
        assert any(k == kind and rr != 0 for k, rr in r), kind
    assert any(max(s.counts) > 64 for s in gc.MOE)
    assert {s.ss_in for s in gc.NORM} >= {0, 1, 8, 9, 36, 64, 100}
    assert {s.M for s in gc.GEMM_CASES} >= {1, 15, 16, 17, 31, 32}
    empties = [sum(1 for a, b in gc.splits_of(s) if b == a) for s in gc.SKINNY_V1]
    assert max(empties) == 5
    uneven = [gc.splits_of(s) for s in gc.SKINNY_V2 if s.K == 768 and s.ksplit == 2]
    assert uneven and uneven[0] == [(0, 512), (512, 768)]


def test_launch_geometry_helpers():
    """The mirrors of the host-side split rules used by the mutations."""
    assert gc.skinny_splits(256, 96, 8) == [(0, 32), (32, 64), (64, 96)] + \
        [(32 * s, 32 * s) for s in range(3, 8)]
    assert gc.skinny_splits(64, 1280, 3) == [(0, 512), (512, 1024), (1024, 1280)]
    assert gc.skinny_splits(64, 1280, 5) == [(256 * s, 256 * s + 256) for s in range(5)]
    assert gc.w4_splits(4, 64, 384, 2) == [(0, 256), (256, 384)]
    assert gc.w4_splits(1, 64, 2048, 0) == [(0, 2048)]          # GEMV
    assert gc.w4_splits(1, 64, 1024, 0) == [(0, 512), (512, 1024)]
    for nwg in (8, 9, 11, 15, 23, 2004 % 64 + 64):
        assert sorted(gc.xcd_remap(nwg)) == list(range(nwg))     # bijective
    assert gc.xcd_remap(8) == list(range(8))
    assert gc.xcd_remap(9)[:3] == [0, 2, 3] and gc.xcd_remap(9)[8] == 1
