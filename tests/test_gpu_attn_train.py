"""Training-attention kernels (ops/hip/attn_train.hip) against the fp64 oracle
of tests/train_attn_cases.py, for O, dQ, dK and dV, at the shapes where their
tiling branches; plus the public op's autograd wrapper, run-to-run bitwise
reproducibility (no atomics), the dispatch rules and the memory property that
motivates the op.

The bounds are derived in train_attn_cases.py, not measured; every check
prints err/tol and where the worst element sits.
tests/test_train_attn_cases_cpu.py shows on the CPU that the roundings alone
stay within the bounds and that each targeted defect lands >= 4 x tol away.
"""
import pytest
import torch

import train_attn_cases as tc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bloombee_amd import ops
    from bloombee_amd.ops import interface

    assert ops.HAVE_HIP_OPS, (
        "HIP extension must be built and loadable on a GPU box (fail-loud policy)"
    )

DEV = "cuda:0"


def _to_dev(case):
    """Device copies that keep each tensor's strides (fused views stay views)."""
    if case.spec.strided:
        s = case.spec
        buf = case.buf.to(DEV)
        T, Hq, Hkv = s.T, s.Hq, s.Hkv
        q = buf[:, :T, :Hq]
        k = buf[:, :T, Hq:Hq + Hkv]
        v = buf[:, :T, Hq + Hkv:Hq + 2 * Hkv]
        do = case.do.permute(0, 2, 1, 3).contiguous().to(DEV).permute(0, 2, 1, 3)
        assert not q.is_contiguous() and not do.is_contiguous()
    else:
        q, k, v, do = (t.to(DEV) for t in (case.q, case.k, case.v, case.do))
    slopes = case.slopes.to(DEV) if case.slopes is not None else None
    return q, k, v, do, slopes


def _direct(case):
    q, k, v, do, slopes = _to_dev(case)
    out, lse = ops.hip_ops.attn_train_fwd(q, k, v, case.scale, case.window,
                                          slopes, True)
    dq, dk, dv = ops.hip_ops.attn_train_bwd(do, q, k, v, out, lse, case.scale,
                                            case.window, slopes)
    torch.cuda.synchronize()
    return {"O": out, "LSE": lse, "dQ": dq, "dK": dk, "dV": dv}


@pytest.mark.parametrize("name", list(tc.CASES))
def test_bindings_match_oracle(name):
    case = tc.build(tc.CASES[name])
    want, bound = tc.oracle(case), tc.tol(case)
    got = _direct(case)
    s = case.spec
    assert got["O"].shape == (tc.B, s.T, s.Hq, s.D) and got["O"].is_contiguous()
    assert got["dK"].shape == (tc.B, s.T, s.Hkv, s.D) and got["dK"].is_contiguous()
    assert got["dV"].shape == got["dK"].shape and got["dQ"].shape == got["O"].shape
    ratios = {}
    for key in ("O", "dQ", "dK", "dV"):
        g = got[key].cpu()
        assert bool(torch.isfinite(g.float()).all()), f"{name} {key}: non-finite"
        ratios[key], where = tc.worst(g, want[key], bound[key])
        print(f"[attn-train] {name} {key}: err/tol {ratios[key]:.3f} at {where}")
    lse_err = float((got["LSE"].cpu().double() - want["LSE"]).abs().max())
    print(f"[attn-train] {name} LSE: max abs err {lse_err:.2e}")
    # fp32 LSE of scores up to a few tens: a few ulp of 2^-23 * 32
    assert lse_err <= 2e-5, f"{name}: LSE off by {lse_err}"
    for key, r in ratios.items():
        assert r <= 1.0, f"{name} {key}: err/tol {r:.3f}"


@pytest.mark.parametrize("name", ["base", "window40", "alibi", "strided", "mqa5"])
def test_public_op_equals_bindings_bitwise(name):
    case = tc.build(tc.CASES[name])
    direct = _direct(case)
    q, k, v, do, slopes = _to_dev(case)
    q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
    out = ops.attn_train(q, k, v, case.scale, case.window, slopes)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), do)
    for key, g in (("O", out), ("dQ", dq), ("dK", dk), ("dV", dv)):
        assert torch.equal(g, direct[key]), f"{name} {key}: public op differs"
    with torch.no_grad():
        assert torch.equal(ops.attn_train(q, k, v, case.scale, case.window, slopes),
                           direct["O"])


@pytest.mark.parametrize("name", ["keyblock257", "mqa5"])
def test_backward_is_bitwise_reproducible(name):
    case = tc.build(tc.CASES[name])
    a, b = _direct(case), _direct(case)
    for key in ("O", "LSE", "dQ", "dK", "dV"):
        assert torch.equal(a[key], b[key]), f"{name} {key}: run-to-run difference"


class _Counter:
    """Wraps the extension so every attn_train_fwd/bwd call is counted."""

    def __init__(self, ext):
        self._ext = ext
        self.fwd = self.bwd = 0

    def attn_train_fwd(self, *a):
        self.fwd += 1
        return self._ext.attn_train_fwd(*a)

    def attn_train_bwd(self, *a):
        self.bwd += 1
        return self._ext.attn_train_bwd(*a)

    def __getattr__(self, name):
        return getattr(self._ext, name)


def _run(q, k, v):
    q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
    out = ops.attn_train(q, k, v, q.shape[-1] ** -0.5)
    out.float().sum().backward()
    torch.cuda.synchronize()
    return out


def test_dispatch_rules(monkeypatch):
    counter = _Counter(interface.hip_ops)
    monkeypatch.setattr(interface, "hip_ops", counter)
    monkeypatch.delenv("BBAMD_TRAIN_ATTN_KERNEL", raising=False)
    gen = torch.Generator().manual_seed(0)
    mk = lambda h, d, dt: torch.randn(1, 24, h, d, generator=gen).to(dt).to(DEV)

    q, k, v = mk(4, 128, torch.bfloat16), mk(2, 128, torch.bfloat16), mk(2, 128, torch.bfloat16)
    kern = _run(q, k, v)
    assert (counter.fwd, counter.bwd) == (1, 1), "supported call must take the kernel"

    monkeypatch.setenv("BBAMD_TRAIN_ATTN_KERNEL", "0")
    off = _run(q, k, v)
    assert (counter.fwd, counter.bwd) == (1, 1), "switch off must take the composition"
    monkeypatch.delenv("BBAMD_TRAIN_ATTN_KERNEL")
    # same math, different rounding points: bf16 outputs of O(1) values
    assert float((kern.detach().float() - off.detach().float()).abs().max()) < 0.1

    _run(mk(4, 256, torch.bfloat16), mk(2, 256, torch.bfloat16), mk(2, 256, torch.bfloat16))
    assert (counter.fwd, counter.bwd) == (1, 1), "D = 256 must take the composition"
    _run(mk(4, 128, torch.float32), mk(2, 128, torch.float32), mk(2, 128, torch.float32))
    assert (counter.fwd, counter.bwd) == (1, 1), "fp32 must take the composition"
    _run(q, k, v)
    assert (counter.fwd, counter.bwd) == (2, 2)


def test_binding_checks_reject_bad_inputs():
    gen = torch.Generator().manual_seed(1)
    mk = lambda h, d, dt=torch.bfloat16: torch.randn(1, 8, h, d, generator=gen).to(dt).to(DEV)
    f = ops.hip_ops.attn_train_fwd
    with pytest.raises(RuntimeError):
        f(mk(2, 32), mk(2, 32), mk(2, 32), 1.0, 0, None, True)        # D
    with pytest.raises(RuntimeError):
        f(mk(2, 64, torch.float32), mk(2, 64), mk(2, 64), 1.0, 0, None, True)
    with pytest.raises(RuntimeError):
        f(mk(2, 64).cpu(), mk(2, 64), mk(2, 64), 1.0, 0, None, True)  # device
    with pytest.raises(RuntimeError):
        f(mk(2, 128)[..., ::2], mk(2, 64), mk(2, 64), 1.0, 0, None, True)  # last dim
    with pytest.raises(RuntimeError):
        f(mk(3, 64), mk(2, 64), mk(2, 64), 1.0, 0, None, True)        # Hq % Hkv


def test_peak_memory_stays_below_one_score_tensor():
    """fwd+bwd of the op must need less than one fp32 (B, Hq, T, T) score
    tensor, which the composition cannot avoid. A derived condition: the op
    keeps q, k, v, O, dO, dQ, dK, dV (bf16, linear in T) and LSE, delta."""
    Bm, Hq, Hkv, D, T = 1, 8, 2, 128, 2048
    gen = torch.Generator().manual_seed(2)
    mk = lambda h: (torch.randn(Bm, T, h, D, generator=gen)
                    .to(torch.bfloat16).to(DEV).requires_grad_(True))
    q, k, v = mk(Hq), mk(Hkv), mk(Hkv)
    do = torch.randn(Bm, T, Hq, D, generator=gen).to(torch.bfloat16).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = ops.attn_train(q, k, v, D ** -0.5)
    grads = torch.autograd.grad(out, (q, k, v), do)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    limit = Bm * Hq * T * T * 4
    print(f"[attn-train] peak growth {growth / 2**20:.1f} MiB, "
          f"one score tensor {limit / 2**20:.1f} MiB")
    assert all(bool(torch.isfinite(g.float()).all()) for g in grads)
    assert growth < limit
