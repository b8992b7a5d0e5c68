"""Host-side parts of the nontemporal W stream, checked without a GPU: the
skinny GEMM's block-index remap, now one helper in ops/hip/common.h
(mirrored in ops/reference.py as the pack layout is), and the BBAMD_W_NT
setting, the per-call request and the `auto` table through
gemm_skinny_nt_plan. The plan checks are skipped when the extension is not
built."""
import pytest

import gemm_cases as gc
from bloombee_amd import ops
from bloombee_amd.ops import reference as ref

needs_ext = pytest.mark.skipif(not ops.HAVE_HIP_OPS, reason="HIP extension not built")


def test_remap_is_a_bijection_for_every_grid():
    for nwg in range(1, 1025):
        tiles = [ref.xcd_remap(b, nwg) for b in range(nwg)]
        assert sorted(tiles) == list(range(nwg)), nwg
        if nwg < 8:
            assert tiles == list(range(nwg)), nwg


def test_remap_matches_the_exact_tests_mirror():
    # tests/gemm_cases.py carries its own copy for the stripe_unremapped defect
    for nwg in (1, 7, 8, 9, 11, 15, 16, 23, 64, 96, 448, 1000):
        assert [ref.xcd_remap(b, nwg) for b in range(nwg)] == gc.xcd_remap(nwg)


def test_remap_puts_tile_t_on_xcd_t_div_q():
    """The dispatcher places block b on XCD b % 8. For a grid that is a
    multiple of 8, tile t is worked on by a block congruent to t // (nwg / 8)
    mod 8: each XCD owns one contiguous run of nwg / 8 tiles."""
    for nwg in range(8, 1025, 8):
        q = nwg // 8
        for b in range(nwg):
            t = ref.xcd_remap(b, nwg)
            assert b % 8 == t // q, (nwg, b, t)


def test_remap_uneven_grid_keeps_runs_contiguous():
    # r = nwg % 8 XCDs own q + 1 consecutive tiles, the others q
    for nwg in (9, 11, 15, 23, 449):
        q, r = divmod(nwg, 8)
        for x in range(8):
            own = sorted(ref.xcd_remap(b, nwg) for b in range(x, nwg, 8))
            assert len(own) == q + (1 if x < r else 0)
            assert own == list(range(own[0], own[0] + len(own))), (nwg, x)


def test_w_nt_is_checked_where_it_is_ignored():
    import torch
    x, w = torch.zeros(2, 256), torch.zeros(64, 256)
    assert ops.linear(x, w, w_nt=1).shape == (2, 64)
    assert ops.linear_swiglu(x, w, w_nt=-1).shape == (2, 32)
    for bad in (2, -2):
        with pytest.raises(RuntimeError, match="w_nt"):
            ops.linear(x, w, w_nt=bad)
        with pytest.raises(RuntimeError, match="w_nt"):
            ops.linear_swiglu(x, w, w_nt=bad)


FLAGSHIP = ((6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336))


@needs_ext
def test_setting_and_request():
    plan = ops.hip_ops.gemm_skinny_nt_plan
    for N, K in FLAGSHIP + ((64, 256), (192, 1024)):
        for packed in (False, True):
            assert plan(N, K, packed, 0, "1")[0] is True
            assert plan(N, K, packed, 0, "0")[0] is False
            # a call's request overrides every setting
            for setting in ("auto", "0", "1"):
                assert plan(N, K, packed, 1, setting)[0] is True
                assert plan(N, K, packed, -1, setting)[0] is False
    # the v1 kernel (K % 256 != 0) has no nt flavour
    assert plan(64, 160, False, 1, "1")[0] is False
    for bad in ("2", "yes", "nt", "AUTO", "-1", "1 "):
        with pytest.raises(RuntimeError, match="BBAMD_W_NT"):
            plan(64, 256, False, 0, bad)
    for bad in (2, -2, 4):
        with pytest.raises(RuntimeError, match="w_nt"):
            plan(64, 256, False, bad, "auto")


@needs_ext
def test_auto_is_the_table_and_nothing_else():
    plan = ops.hip_ops.gemm_skinny_nt_plan
    table = [tuple(e) for e in plan(64, 256, False, 0, "auto")[1]]
    # the streams profiles/r09_nt_weights.md records as faster with nt: packed
    # gate_up and packed down; a change here comes with a new trace
    assert sorted(table) == [(4096, 14336, True), (28672, 4096, True)]
    probe = [(N, K, p) for N, K in FLAGSHIP + ((64, 256), (4096, 8192), (8192, 4096))
             for p in (False, True)]
    for N, K, packed in probe:
        assert plan(N, K, packed, 0, "auto")[0] is ((N, K, packed) in table), (N, K, packed)
    # unset means auto
    import os
    if "BBAMD_W_NT" not in os.environ:
        for N, K, packed in probe:
            assert plan(N, K, packed, 0)[0] is ((N, K, packed) in table)
