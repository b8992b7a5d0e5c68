"""CPU checks of tests/elementwise_cases.py: the builders' invariants, the
models against ops.reference, the bounds, and the sensitivity guards.

For every case: the fp64 model rounded once to bf16 passes the case's own
check (a perfect implementation is never rejected), and ops.reference, an
honest f32 implementation, passes it too (the bound is attainable). For
every mutation: at least one applicable case fails its own check when the
mutated model is rounded the way a device would store it, so a device with
that defect cannot pass test_gpu_elementwise_exact.py.
"""
import pytest
import torch

import elementwise_cases as ec
from bloombee_amd.ops import reference as ref

BF = torch.bfloat16


def bf(t):
    return t.to(BF)


# ---------------------------------------------------------------------------
# runners: ops.reference on a case, and a mutated model as a device stores it
# ---------------------------------------------------------------------------

def ref_norm(c):
    spec = c.spec
    x, w = bf(c.xbuf)[1:1 + spec.N], bf(c.w)
    if spec.op == "rms":
        return {"y": ref.rms_norm(x, w, spec.eps)}
    if spec.op == "rms_res":
        h, y = ref.rms_norm_residual(x, bf(c.r), w, spec.eps)
        return {"h": h, "y": y}
    return {"y": ref.layer_norm(x, w, bf(c.b), spec.eps)}


def stored(d):
    return {k: ec.as_device_would(v) for k, v in d.items()}


def ref_rope(c):
    pos = c.pos.clamp(0, c.max_pos - 1)          # the reference does not clamp
    return ref.rope_apply(bf(c.q), bf(c.k), c.cos.float(), c.sin.float(), pos)


def ref_swiglu(c):
    I = c.gu.shape[1] // 2
    return ref.swiglu(bf(c.gu[:, :I]), bf(c.gu[:, I:]))


def ref_unpack(c):
    R, C = c.spec.rows, c.spec.cols
    return ref.quant4_unpack(c.packed.reshape(R, C // 64, 32), c.scale, c.zero)


# ---------------------------------------------------------------------------
# every case: builder invariants (asserted in build), rounded model, reference
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("spec", ec.NORM_SPECS, ids=ec.ids(ec.NORM_SPECS))
def test_norm_case(spec):
    c = ec.build_norm(spec)
    assert c.xbuf.shape == (spec.N + 2, spec.H)
    assert bool((c.xbuf[0].abs() == ec.POISON).all())
    assert ec.check_norm(c, stored(c.want)) <= 1.0
    r = ec.check_norm(c, ref_norm(c))
    assert r <= 1.0, f"ops.reference at {r:.3f} x the bound"
    if spec.exact:
        assert r == 0.0


def test_norm_specs_cover_every_variant():
    for op in ec.NORM_OPS:
        for kind in ("exact", "randn"):
            hs = {s.H for s in ec.NORM_SPECS if s.op == op and s.kind == kind}
            assert hs == set(ec.NORM_H)
            assert {ec.norm_iters(h) for h in hs} == {1, 2, 4, 8}
        assert any(s.N == 1 for s in ec.NORM_SPECS if s.op == op)
    assert {ec.norm_iters(h) for h in (2056, 4544, 8200, 14336)} == {2, 4, 8}
    assert all(h % 2048 for h in (2056, 4544, 8200))      # end inside an iteration


def test_nearconst_rows_are_the_table():
    """true variances of the issue's table, and results near the bias"""
    want_var = {1024: [0.0777], 4544: [2.2e-4], 14336: [7.0e-5, 5.2e-5]}
    for spec in ec.NORM_SPECS:
        if spec.kind != "nearconst":
            continue
        c = ec.build_norm(spec)
        var = c.x.var(1, unbiased=False)
        for v, w in zip(var.tolist(), want_var[spec.H]):
            assert abs(v - w) <= 0.02 * w
        for m, (maj, _, _) in enumerate(ec.NEARCONST_ROWS[spec.H]):
            at = c.x[m] == maj
            assert bool(((c.want["y"][m] - c.b).abs()[at] <= 0.08 * c.w.abs()[at]).all())


@pytest.mark.parametrize("spec", ec.ROPE_SPECS, ids=ec.ids(ec.ROPE_SPECS))
def test_rope_case(spec):
    c = ec.build_rope(spec)
    assert ec.check_rope(c, [ec.as_device_would(t) for t in c.want]) <= 1.0
    r = ec.check_rope(c, ref_rope(c))
    assert r <= 1.0, f"ops.reference at {r:.3f} x the bound"
    # positions: non-monotonic, repeated, different per batch row
    p = c.pos
    assert any(len(set(row)) < len(row) for row in p.tolist())
    assert not torch.equal(p[0], p[1]) and not torch.equal(p[1], p[2])
    assert bool((p[:, 1:] < p[:, :-1]).any())


def test_rope_tables_differ_everywhere():
    c = ec.build_rope(ec.ROPE_SPECS[0])
    pair = c.cos * 8 + c.sin
    assert float((pair[1:] != pair[:-1]).double().mean()) > 0.8      # along positions
    assert float((pair[:, 1:] != pair[:, :-1]).double().mean()) > 0.8  # along i


@pytest.mark.parametrize("spec", ec.SWIGLU_SPECS, ids=ec.ids(ec.SWIGLU_SPECS))
def test_swiglu_case(spec):
    c = ec.build_swiglu(spec)
    assert ec.check_swiglu(c, ec.as_device_would(c.want)) <= 1.0
    r = ec.check_swiglu(c, ref_swiglu(c))
    assert r <= 1.0, f"ops.reference at {r:.3f} x the bound"


def test_swiglu_gate_sweep():
    g = ec.swiglu_gates()
    assert g.numel() > 30000 and float(g.abs().max()) == 100.0
    assert int((g == 0).sum()) >= 4                  # +0 and -0, twice
    c = ec.build_swiglu(ec.SWIGLU_SPECS[0])
    assert c.gu.shape[1] == 16
    assert set(g.tolist()) <= set(c.gu[:, :8].reshape(-1).tolist())


@pytest.mark.parametrize("spec", ec.KV_SPECS + [ec.KV_BIG_SPEC],
                         ids=ec.ids(ec.KV_SPECS + [ec.KV_BIG_SPEC]))
def test_kv_case(spec):
    c = ec.build_kv(spec)
    if not spec.big:
        kp, vp = bf(c.k_pool0), bf(c.v_pool0)
        ref.kv_write(bf(c.k_new), bf(c.v_new), kp, vp, c.page_table, c.start_pos)
        assert torch.equal(kp.double(), c.k_pool) and torch.equal(vp.double(), c.v_pool)
        last = int(c.start_pos[1]) + ec.KV_T - 1
        assert last == spec.maxp * spec.P - 1
    for ctx in ec.kv_gather_ctxs(spec):
        for bi in (0, spec.B - 1):
            k, v = ec.model_kv_gather(c, ctx, bi)
            rk, rv = ref.kv_gather(bf(c.k_pool), bf(c.v_pool), c.page_table, ctx, bi)
            assert torch.equal(rk.double(), k) and torch.equal(rv.double(), v)


@pytest.mark.parametrize("spec", ec.PACK_SPECS, ids=ec.ids(ec.PACK_SPECS))
def test_pack_case(spec):
    c = ec.build_pack(spec)
    R, C = c.x.shape
    packed, scale, zero = ref.quant4_pack(c.x)
    assert ec.check_pack(c, (packed.reshape(R, C // 2), scale, zero)) == 0.0
    assert bool(torch.isfinite(zero.float()).all() and torch.isfinite(scale.float()).all())


def test_pack_designed_groups():
    c = ec.build_pack(ec.PACK_SPECS[0])
    x = c.x.float().reshape(5, 64)
    assert float(x[0].max() - x[0].min()) == 0.0
    t = x[1] / 2.0                                    # scale is exactly 2
    assert int((t - t.floor() == 0.5).sum()) >= 30    # rounding ties
    assert int(x[2].argmin()) == 0 and int(x[2].argmax()) == 63
    assert int(x[3].argmax()) == 0 and int(x[3].argmin()) == 63
    assert float(x[4].max()) < 0
    groups = [b.x.numel() // 64 for b in map(ec.build_pack, ec.PACK_SPECS[:2])]
    assert groups[0] % 4 == 1 and groups[1] % 4 == 3


@pytest.mark.parametrize("spec", ec.UNPACK_SPECS, ids=ec.ids(ec.UNPACK_SPECS))
def test_unpack_case(spec):
    c = ec.build_unpack(spec)
    assert ec.check_unpack(c, ec.as_device_would(c.want)) <= 1.0
    r = ec.check_unpack(c, ref_unpack(c))
    assert r <= 1.0, f"ops.reference at {r:.3f} x the bound"


# ---------------------------------------------------------------------------
# sensitivity guards
# ---------------------------------------------------------------------------

def _norm_fails(spec, mut):
    c = ec.build_norm(spec)
    return ec.check_norm(c, stored(ec.model_norm(c, mut))) > 1.0


def _rope_fails(spec, mut):
    c = ec.build_rope(spec)
    return ec.check_rope(c, [ec.as_device_would(t) for t in ec.model_rope(c, mut)]) > 1.0


def _swiglu_fails(spec, mut):
    c = ec.build_swiglu(spec)
    return ec.check_swiglu(c, ec.as_device_would(ec.model_swiglu(c, mut))) > 1.0


def _kv_fails(spec, mut):
    c = ec.build_kv(spec)
    if not mut.startswith("kv_gather"):
        kp, vp = ec.model_kv_write(c, mut)
        return not (torch.equal(kp, c.k_pool) and torch.equal(vp, c.v_pool))
    for ctx in ec.kv_gather_ctxs(spec):
        for bi in (0, spec.B - 1):
            want = ec.model_kv_gather(c, ctx, bi)
            got = ec.model_kv_gather(c, ctx, bi, mut)
            if any(ec.exact_ratio(g, w) > 0 for g, w in zip(got, want)):
                return True
    return False


def _pack_fails(spec, mut):
    c = ec.build_pack(spec)
    return ec.check_pack(c, ec.model_pack(c, mut)) > 1.0


def _unpack_fails(spec, mut):
    c = ec.build_unpack(spec)
    return ec.check_unpack(c, ec.as_device_would(ec.model_unpack(c, mut))) > 1.0


FAMILIES = (
    (ec.NORM_MUTATIONS, ec.NORM_SPECS, ec.norm_applicable, _norm_fails),
    (ec.ROPE_MUTATIONS, ec.ROPE_SPECS, ec.rope_applicable, _rope_fails),
    (ec.SWIGLU_MUTATIONS, ec.SWIGLU_SPECS, ec.swiglu_applicable, _swiglu_fails),
    (ec.KV_MUTATIONS, ec.KV_SPECS + [ec.KV_BIG_SPEC], ec.kv_applicable, _kv_fails),
    (ec.PACK_MUTATIONS, ec.PACK_SPECS, ec.pack_applicable, _pack_fails),
    (ec.UNPACK_MUTATIONS, ec.UNPACK_SPECS, ec.unpack_applicable, _unpack_fails),
)
ALL_MUTATIONS = [(m, fam) for fam in FAMILIES for m in fam[0]]


@pytest.mark.parametrize("mut,fam", ALL_MUTATIONS, ids=[m for m, _ in ALL_MUTATIONS])
def test_mutation_is_caught(mut, fam):
    _, specs, applicable, fails = fam
    cases = [s for s in specs if mut in applicable(s)]
    assert cases, f"no case to which {mut} applies"
    caught = [s.name for s in cases if fails(s, mut)]
    assert caught, f"{mut} passes all of {[s.name for s in cases]}"


def test_every_mutation_is_exercised():
    for muts, specs, applicable, _ in FAMILIES:
        used = {m for s in specs for m in applicable(s)}
        assert used == set(muts), set(muts) ^ used


@pytest.mark.parametrize("mut", ["norm_wave_partial_dropped",
                                 "norm_mean_over_padded_length",
                                 "norm_weight_shifted_by_8"])
@pytest.mark.parametrize("op", ec.NORM_OPS)
def test_norm_geometry_mutations_fail_every_exact_case(op, mut):
    """exact data: each geometry defect shows in every case it applies to"""
    specs = [s for s in ec.NORM_SPECS
             if s.op == op and s.exact and mut in ec.norm_applicable(s)]
    assert specs
    for s in specs:
        assert _norm_fails(s, mut), s.name


@pytest.mark.parametrize("op", ec.NORM_OPS)
def test_norm_partial_iteration_is_seen(op):
    """A sum that stops at the last full iteration: H = 4544 loses a tenth of
    the row and fails the exact cases. H = 2056 and 8200 lose 8 elements,
    0.4 % and 0.1 % of the mean square, which one bf16 rounding can hide:
    there the outlier cases put 2^12 among those 8. (H = 14336 is 7 full
    iterations of the ITERS = 8 kernel: its eighth is idle, not partial.)"""
    mut = "norm_sum_stops_at_last_full_iter"
    names = [f"{op}-exact-h4544", f"{op}-exact-h4544-n1",
             f"{op}-outlier-h2056", f"{op}-outlier-h8200"]
    by_name = {s.name: s for s in ec.NORM_SPECS}
    for n in names:
        assert mut in ec.norm_applicable(by_name[n])
        assert _norm_fails(by_name[n], mut), n


def test_one_pass_variance_is_rejected():
    """The record of the layer-norm defect: an f32 model of t2/H - mu*mu in the
    kernel's summation order fails every near-constant case and every offset
    case (the negative variances among them give NaN rows)."""
    specs = [s for s in ec.NORM_SPECS if "one_pass_variance" in ec.norm_applicable(s)]
    assert {s.kind for s in specs} == {"offset", "nearconst"}
    for s in specs:
        assert _norm_fails(s, "one_pass_variance"), s.name
    c = ec.build_norm(next(s for s in specs if s.name == "ln-nearconst-h14336"))
    _, var = ec._one_pass_f32(c.x, c.spec.H)
    y = ec.model_norm(c, "one_pass_variance")["y"]
    neg = var[:, 0] + c.spec.eps < 0
    assert bool(neg.any()), "a negative variance at H = 14336"
    assert bool(torch.isnan(y[neg]).all())
    # and the values of the table: 0 at H = 1024, 7.8e-3 at H = 4544
    for name, lo, hi in (("ln-nearconst-h1024", -1e-9, 1e-9),
                         ("ln-nearconst-h4544", 7.0e-3, 8.6e-3)):
        c = ec.build_norm(next(s for s in specs if s.name == name))
        _, var = ec._one_pass_f32(c.x, c.spec.H)
        assert lo <= float(var[0]) <= hi, (name, float(var[0]))


def test_exact_offset_needs_mean_subtraction():
    """c +- 2^j rows: sum (x - c)^2 stays exact in f32 in any order while, for
    the large offsets, sum x^2 does not from H = 2048 on, so only a variance
    taken after subtracting the mean is exact by construction."""
    for s in ec.NORM_SPECS:
        if s.kind != "exact_offset":
            continue
        c = ec.build_norm(s)
        unit = (c.x - c.x.mean(1, keepdim=True)).abs().amin(1)     # 2^j per row
        assert bool((((c.x - c.x.mean(1, keepdim=True)) / unit[:, None]).abs() == 1).all())
        t2 = ((c.x / unit[:, None]) ** 2).sum(1)
        if s.H >= 2048:
            assert float(t2.max()) > 2 ** 24
