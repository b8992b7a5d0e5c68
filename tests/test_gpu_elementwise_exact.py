"""Parity of the per-layer kernels (elementwise.hip, kvcache.hip, quant4.hip)
against the fp64 CPU models of tests/elementwise_cases.py: rms_norm,
rms_norm_residual, layer_norm, rope_apply_, swiglu, kv_write, kv_gather,
quant4_pack, quant4_unpack, and the grid-stride sweeps of gelu_tanh and
add_bf16.

Exact cases must `torch.equal` the expected tensor; realistic ones stay
within the derived bound of the elementwise_cases docstring, where the worst
observed ratios are recorded (every test prints its own, and the last test
of the file prints the worst per op). test_elementwise_cases_cpu.py proves
on CPU that each listed defect fails at least one of these cases.

Which case reaches which path:
  norm ITERS 1 / 2 / 4 / 8 at their upper edge   h2048, h4096, h8192, h16384
  ... and just past the previous one             h2056, h4544, h8200, h14336
  H ending inside an iteration                   h2056, h4544, h8200
  one active lane / one active wave              h8, h64
  grid-stride second sweep      swiglu-257x16392, kv-gather-...-ctx1030,
                                unpack-*-1025x1088, gelu / add past the cap
  kv_write 256-thread loop twice                 kv-h8-d512-*
  quant4_pack block with empty last waves        5 and 15 groups
"""
import pytest
import torch

import elementwise_cases as ec

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bloombee_amd import ops
    from bloombee_amd.ops import reference as ref

    assert ops.HAVE_HIP_OPS, (
        "HIP extension must be built and loadable on a GPU box (fail-loud policy)"
    )

DEV = "cuda:0"
BF = torch.bfloat16
WORST = {}


def dev(t, dtype=BF):
    return None if t is None else t.to(dtype).to(DEV)


def record(op, r, what):
    """print the ratio, keep the worst per op, assert it."""
    print(f"worst |err| / bound, {what}: {r:.3f}")
    WORST[op] = max(WORST.get(op, 0.0), r)
    assert r <= 1.0, f"{what}: |err| reaches {r:.3f} x the derived bound"


def assert_exact(got, want, what):
    assert ec.exact_ratio(got, want) == 0.0, f"{what}: {ec.describe_mismatch(got, want)}"


# ---------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------

def run_norm(c):
    spec = c.spec
    x = dev(c.xbuf)[1:1 + spec.N]                 # rows of a taller poisoned buffer
    assert x.is_contiguous()
    w = dev(c.w)
    if spec.op == "rms":
        return {"y": ops.rms_norm(x, w, spec.eps)}
    if spec.op == "rms_res":
        h, y = ops.rms_norm_residual(x, dev(c.r), w, spec.eps)
        return {"h": h, "y": y}
    return {"y": ops.layer_norm(x, w, dev(c.b), spec.eps)}


@pytest.mark.parametrize("spec", ec.NORM_SPECS, ids=ec.ids(ec.NORM_SPECS))
def test_norm(spec):
    c = ec.build_norm(spec)
    got = run_norm(c)
    for name, t in got.items():
        assert t.shape == (spec.N, spec.H) and t.dtype == BF
    if spec.op == "rms_res":
        assert_exact(got["h"], c.want["h"], f"{spec.name} h = bf16(x + r)")
    if spec.exact:
        assert_exact(got["y"], c.want["y"], spec.name)
        return
    if spec.kind == "nearconst":
        assert bool(torch.isfinite(got["y"].float()).all()), f"{spec.name}: not finite"
    record({"rms": "rms_norm", "rms_res": "rms_norm_residual", "ln": "layer_norm"}[spec.op],
           ec.worst_ratio(got["y"], c.want["y"], ec.norm_bound(c)), spec.name)


@pytest.mark.parametrize("op", ec.NORM_OPS)
@pytest.mark.parametrize("H", [4100, 16392])
def test_norm_rejects_bad_hidden_size(op, H):
    """H % 8 != 0 would read and write past the row; H > 16384 has no kernel"""
    x = torch.zeros(3, H, dtype=BF, device=DEV)
    w = torch.ones(H, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError):
        if op == "rms":
            ops.rms_norm(x, w, 1e-5)
        elif op == "rms_res":
            ops.rms_norm_residual(x, x.clone(), w, 1e-5)
        else:
            ops.layer_norm(x, w, w.clone(), 1e-5)


@pytest.mark.parametrize("op", ec.NORM_OPS)
def test_norm_rejects_wrong_weight_length(op):
    x = torch.zeros(3, 256, dtype=BF, device=DEV)
    w, short = torch.ones(256, dtype=BF, device=DEV), torch.ones(248, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError):
        if op == "rms":
            ops.rms_norm(x, short, 1e-5)
        elif op == "rms_res":
            ops.rms_norm_residual(x, x.clone(), short, 1e-5)
        else:
            ops.layer_norm(x, short, w, 1e-5)
    if op == "ln":
        with pytest.raises(RuntimeError):
            ops.layer_norm(x, w, short, 1e-5)
    if op == "rms_res":
        with pytest.raises(RuntimeError):
            ops.rms_norm_residual(x, x[:2].clone(), w, 1e-5)


# ---------------------------------------------------------------------------
# rope
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("spec", ec.ROPE_SPECS, ids=ec.ids(ec.ROPE_SPECS))
def test_rope(spec):
    c = ec.build_rope(spec)
    q, k = dev(c.q), dev(c.k)
    ops.rope_apply_(q, k, dev(c.cos, torch.float32), dev(c.sin, torch.float32),
                    c.pos.int().to(DEV))
    if spec.kind == "real":
        record("rope_apply_", ec.check_rope(c, (q, k)), spec.name)
    else:
        assert_exact(q, c.want[0], f"{spec.name} q")
        assert_exact(k, c.want[1], f"{spec.name} k")


def test_rope_rejects_mismatched_operands():
    B, Hq, T, D = 2, 4, 3, 64
    q = torch.zeros(B, Hq, T, D, dtype=BF, device=DEV)
    cos = torch.ones(16, D // 2, device=DEV)
    pos = torch.zeros(B, T, dtype=torch.int32, device=DEV)
    for kshape in ((B, 1, T + 1, D), (B + 1, 1, T, D), (B, 1, T, D // 2)):
        with pytest.raises(RuntimeError):
            ops.rope_apply_(q, torch.zeros(*kshape, dtype=BF, device=DEV), cos, cos, pos)
    k = torch.zeros(B, 1, T, D, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError):
        ops.rope_apply_(q, k, cos, cos, pos[:1])                     # pos.numel() != B * T
    qo, ko = (torch.zeros(B, h, T, 7, dtype=BF, device=DEV) for h in (Hq, 1))
    with pytest.raises(RuntimeError):
        ops.rope_apply_(qo, ko, torch.ones(16, 3, device=DEV),
                        torch.ones(16, 3, device=DEV), pos)          # odd head_dim


# ---------------------------------------------------------------------------
# swiglu, and gelu_tanh / add_bf16 past the grid cap
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("spec", ec.SWIGLU_SPECS, ids=ec.ids(ec.SWIGLU_SPECS))
def test_swiglu(spec):
    """against want EVERYWHERE: the output is a fresh torch.empty, and an
    element no sweep wrote holds garbage that fails the bound"""
    c = ec.build_swiglu(spec)
    got = ops.swiglu(dev(c.gu))
    assert got.shape == c.want.shape and got.dtype == BF
    record("swiglu", ec.check_swiglu(c, got), spec.name)


def _past_cap_input(seed):
    v = ec.bf16_values_upto(8.0)
    n = ec.PAST_CAP_NUMEL
    idx = (torch.arange(n) * 7919 + seed) % v.numel()
    return v[idx]


def test_gelu_tanh_past_grid_cap():
    x = _past_cap_input(0)
    assert x.numel() // 8 > ec.FLAT_GRID_CAP * 256 and x.numel() % 8 == 5
    xd = x.double()
    want = ec.gelu_model(xd)
    got = ops.gelu_tanh(x.to(DEV))
    assert got.shape == x.shape and got.dtype == BF
    record("gelu_tanh", ec.worst_ratio(got, want, ec.gelu_bound(xd, want)),
           f"gelu_tanh numel={x.numel()}")


def test_add_bf16_past_grid_cap():
    a, b = _past_cap_input(1), _past_cap_input(4001)
    got = ops.hip_ops.add_bf16(a.to(DEV), b.to(DEV)).cpu()
    assert torch.equal(got, (a.float() + b.float()).to(BF))


# ---------------------------------------------------------------------------
# paged KV
# ---------------------------------------------------------------------------

def _kv_device(c):
    return (dev(c.k_pool), dev(c.v_pool), c.page_table.to(DEV))


@pytest.mark.parametrize("spec", ec.KV_SPECS, ids=ec.ids(ec.KV_SPECS))
def test_kv_write(spec):
    """the WHOLE pool after the write: live slots and untouched poison alike"""
    c = ec.build_kv(spec)
    kp, vp = dev(c.k_pool0), dev(c.v_pool0)
    ops.kv_write(dev(c.k_new), dev(c.v_new), kp, vp, c.page_table.to(DEV),
                 c.start_pos.to(DEV))
    cpu_k, cpu_v = c.k_pool0.to(BF), c.v_pool0.to(BF)
    ref.kv_write(c.k_new.to(BF), c.v_new.to(BF), cpu_k, cpu_v, c.page_table, c.start_pos)
    assert torch.equal(kp.cpu(), cpu_k), ec.describe_mismatch(kp, cpu_k.double())
    assert torch.equal(vp.cpu(), cpu_v), ec.describe_mismatch(vp, cpu_v.double())
    assert_exact(kp, c.k_pool, f"{spec.name} k pool")
    assert_exact(vp, c.v_pool, f"{spec.name} v pool")


@pytest.mark.parametrize("spec", ec.KV_SPECS + [ec.KV_BIG_SPEC],
                         ids=ec.ids(ec.KV_SPECS + [ec.KV_BIG_SPEC]))
def test_kv_gather(spec):
    c = ec.build_kv(spec)
    kp, vp, pt = _kv_device(c)
    for ctx in ec.kv_gather_ctxs(spec):
        for bi in (0, spec.B - 1):
            k, v = ops.kv_gather(kp, vp, pt, ctx, bi)
            assert k.shape == v.shape == (spec.Hkv, ctx, spec.D)
            rk, rv = ref.kv_gather(c.k_pool.to(BF), c.v_pool.to(BF), c.page_table, ctx, bi)
            assert torch.equal(k.cpu(), rk) and torch.equal(v.cpu(), rv), \
                f"{spec.name} ctx={ctx} batch_index={bi}"
            wk, wv = ec.model_kv_gather(c, ctx, bi)
            assert_exact(k, wk, f"{spec.name} k ctx={ctx} batch_index={bi}")
            assert_exact(v, wv, f"{spec.name} v ctx={ctx} batch_index={bi}")


def test_kv_rejects_bad_arguments():
    c = ec.build_kv(ec.KV_SPECS[0])
    spec = c.spec
    kp, vp, pt = _kv_device(c)
    with pytest.raises(RuntimeError):
        ops.kv_gather(kp, vp, pt, spec.maxp * spec.P + 1, 0)         # ctx > maxp * P
    for bi in (-1, spec.B):
        with pytest.raises(RuntimeError):
            ops.kv_gather(kp, vp, pt, 4, bi)                         # batch_index
    vp_tm = vp.transpose(2, 3).contiguous()                          # (np, Hkv, P, D)
    with pytest.raises(RuntimeError):
        ops.kv_gather(kp, vp_tm, pt, 4, 0)
    with pytest.raises(RuntimeError):
        ops.kv_write(dev(c.k_new), dev(c.v_new), kp, vp_tm, pt, c.start_pos.to(DEV))
    # head_dim 12: not a multiple of the 16 B the kernels move
    n = kp.shape[0]
    kp12 = torch.zeros(n, 1, spec.P, 12, dtype=BF, device=DEV)
    vp12 = torch.zeros(n, 1, 12, spec.P, dtype=BF, device=DEV)
    new12 = torch.zeros(spec.B, 1, ec.KV_T, 12, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError):
        ops.kv_write(new12, new12.clone(), kp12, vp12, pt, c.start_pos.to(DEV))
    with pytest.raises(RuntimeError):
        ops.kv_gather(kp12, vp12, pt, 4, 0)
    assert_exact(kp, c.k_pool, "k pool after the rejected calls")
    assert_exact(vp, c.v_pool, "v pool after the rejected calls")


# ---------------------------------------------------------------------------
# quant4
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("spec", ec.PACK_SPECS, ids=ec.ids(ec.PACK_SPECS))
def test_quant4_pack(spec):
    """packed, scale AND zero, bit for bit, against the f32 model and against
    ref.quant4_pack (which the CPU test shows to be the same thing)"""
    c = ec.build_pack(spec)
    R, C = c.x.shape
    got = ops.quant4_pack(c.x.to(DEV))
    assert got[0].shape == (R, C // 2) and got[1].shape == got[2].shape == (R, C // 64)
    assert got[0].dtype == torch.uint8 and got[1].dtype == got[2].dtype == torch.float16
    rp, rs, rz = ref.quant4_pack(c.x)
    for name, g, w, r in zip(("packed", "scale", "zero"), got, c.want,
                             (rp.reshape(R, C // 2), rs, rz)):
        g = g.cpu()
        assert torch.equal(g, r), f"{spec.name} {name} vs ops.reference: " \
            f"{ec.describe_mismatch(g.double(), r.double())}"
        assert torch.equal(g, w), f"{spec.name} {name} vs the model"


@pytest.mark.parametrize("spec", ec.UNPACK_SPECS, ids=ec.ids(ec.UNPACK_SPECS))
def test_quant4_unpack(spec):
    c = ec.build_unpack(spec)
    got = ops.quant4_unpack(c.packed.to(DEV), c.scale.to(DEV), c.zero.to(DEV))
    assert got.shape == (spec.rows, spec.cols) and got.dtype == BF
    if spec.exact:
        assert_exact(got, c.want, spec.name)
    else:
        record("quant4_unpack", ec.check_unpack(c, got), spec.name)


# ---------------------------------------------------------------------------
# zero-row inputs: an empty result of the right shape and dtype, no launch
# ---------------------------------------------------------------------------

def test_zero_row_inputs():
    x = torch.empty(0, 64, dtype=BF, device=DEV)
    w = torch.ones(64, dtype=BF, device=DEV)
    y = ops.rms_norm(x, w, 1e-5)
    assert y.shape == (0, 64) and y.dtype == BF
    h, y = ops.rms_norm_residual(x, x.clone(), w, 1e-5)
    assert h.shape == y.shape == (0, 64) and h.dtype == y.dtype == BF
    y = ops.layer_norm(x, w, w.clone(), 1e-5)
    assert y.shape == (0, 64) and y.dtype == BF
    y = ops.swiglu(torch.empty(0, 32, dtype=BF, device=DEV))
    assert y.shape == (0, 16) and y.dtype == BF

    c = ec.build_kv(ec.KV_SPECS[0])
    k, v = ops.kv_gather(*_kv_device(c), 0, 1)
    assert k.shape == v.shape == (c.spec.Hkv, 0, c.spec.D) and k.dtype == v.dtype == BF

    packed, scale, zero = ops.quant4_pack(x)
    assert packed.shape == (0, 32) and packed.dtype == torch.uint8
    assert scale.shape == zero.shape == (0, 1) and scale.dtype == zero.dtype == torch.float16
    out = ops.quant4_unpack(packed, scale, zero)
    assert out.shape == (0, 64) and out.dtype == BF
    torch.cuda.synchronize()


def test_zz_worst_ratios():
    """the table for the elementwise_cases docstring (run the whole file)"""
    for op in sorted(WORST):
        print(f"worst |err| / bound on this device, {op}: {WORST[op]:.3f}")
    assert all(r <= 1.0 for r in WORST.values())
