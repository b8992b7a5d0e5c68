"""Top-k sparse decode attention kernels (attn_sparse.hip) vs the fp64 oracle
of tests/sparse_cases.py.

The cases have exact f32 scores that are pairwise distinct per head (or tie
on purpose), so the kernel must select exactly the oracle's set; the
tolerance is derived there (2^-8 * max|v| over the kept positions), not
measured. tests/test_sparse_cases_cpu.py proves on the CPU that the defects
these cases target (kkeep off by one, floor, float32 kkeep, per-group
selection, ALiBi left out of the selection, a lost last page, ties going the
wrong way) each land >= 4 x tol away.
"""
import os
import subprocess
import sys

import pytest
import torch

import sparse_cases as sc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bloombee_amd import ops
    from bloombee_amd.ops.interface import hip_ops

    assert ops.HAVE_HIP_OPS, (
        "HIP extension must be built and loadable on a GPU box (fail-loud policy)"
    )

DEV = "cuda:0"


def _dev(case):
    return (case.k_pages.to(DEV), case.v_pages.to(DEV),
            case.page_table.to(DEV), case.ctx.to(DEV))


def _direct(case, pools=None):
    kp, vp, pt, ctx = pools or _dev(case)
    al = case.slopes.float().to(DEV) if case.slopes is not None else None
    return hip_ops.attn_decode_sparse(case.q.to(DEV), kp, vp, pt, ctx,
                                      case.sparsity, case.scale, al)


def _check(name, got, spec, grow=0):
    got = got.cpu()
    assert bool(torch.isfinite(got.float()).all()), f"{name}: non-finite output"
    ratio, (b, h, d) = sc.worst(got, spec, grow)
    print(f"[attn-sparse] {name}: err/tol {ratio:.3f} "
          f"(worst at row {b}, head {h}, d {d})")
    assert ratio <= 1.0, (f"{name}: err / tol = {ratio:.3f} at row {b}, "
                          f"head {h}, d {d}")


@pytest.mark.parametrize("spec", sc.CASES, ids=sc.ids(sc.CASES))
def test_kernel_matches_oracle(spec):
    _check(spec.name, _direct(sc.build(spec)), spec)


@pytest.mark.parametrize("spec", [sc.BASE, sc.CASES[4]],
                         ids=sc.ids([sc.BASE, sc.CASES[4]]))
def test_public_entries_match_direct_binding(spec):
    """ops.attn_decode and ops.attn_paged_qkv under set_attn_sparsity return
    the direct binding's values, each in its own layout."""
    case = sc.build(spec)
    s = spec
    kp, vp, pt, ctx = _dev(case)
    want = _direct(case, (kp, vp, pt, ctx))
    ops.set_attn_sparsity(case.sparsity)
    try:
        got = ops.attn_decode(case.q.to(DEV), kp, vp, pt, ctx, case.scale,
                              alibi_slopes=case.slopes)
        got_qkv = None
        if case.slopes is None:      # the fused-QKV entry has no ALiBi form
            got_qkv = ops.attn_paged_qkv(
                sc.qkv_buffer(case).to(DEV), s.Hq, s.Hkv, kp, vp, pt,
                (ctx - 1), scale=case.scale)
    finally:
        ops.set_attn_sparsity(1.0)
    assert got.shape == (case.B, s.Hq, 1, s.D)
    assert torch.equal(got, want)
    if got_qkv is not None:
        assert got_qkv.shape == (case.B, 1, s.Hq * s.D)
        assert torch.equal(
            got_qkv, want.permute(0, 2, 1, 3).reshape(case.B, 1, s.Hq * s.D))
        # and the dense path is a different result
        dense = ops.attn_paged_qkv(sc.qkv_buffer(case).to(DEV), s.Hq, s.Hkv,
                                   kp, vp, pt, (ctx - 1), scale=case.scale)
        assert not torch.equal(dense, got_qkv)


def test_page_size_8_falls_back_to_the_composition():
    """The kernels are written for 16-slot pages; BBAMD_KV_PAGE_SIZE allows
    others. Those must run the composition on the device, not raise."""
    spec = sc.BASE
    case = sc.build(spec)
    kp8, vp8, pt8 = (x.to(DEV) for x in sc.repaged8(case))
    ctx = case.ctx.to(DEV)
    ops.set_attn_sparsity(case.sparsity)
    try:
        a = ops.attn_decode(case.q.to(DEV), kp8, vp8, pt8, ctx, case.scale)
        b = ops.attn_paged_qkv(sc.qkv_buffer(case).to(DEV), spec.Hq, spec.Hkv,
                               kp8, vp8, pt8, ctx - 1, scale=case.scale)
    finally:
        ops.set_attn_sparsity(1.0)
    _check("page8-attn_decode", a, spec)
    _check("page8-attn_paged_qkv", b, spec)


def test_switch_off_runs_the_composition_in_a_child_process():
    """BBAMD_SPARSE_KERNEL is read once at import: a fresh interpreter."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    env = dict(os.environ)
    env["BBAMD_SPARSE_KERNEL"] = "0"
    env["PYTHONPATH"] = os.pathsep.join(
        [root, here] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    try:
        r = subprocess.run([sys.executable, "-m", "attn_sparse_child"],
                           env=env, cwd=here, timeout=120,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        pytest.fail("child hit the time limit")
    print(r.stdout)
    assert r.returncode == 0, (
        f"child exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    assert "attn_sparse_child ok" in r.stdout


def test_graph_replay_with_growing_context():
    """One captured call (a single linear chain of launches); between replays
    one more K/V position is written per row and ctx_lens is bumped in place
    on the device, so kkeep changes under replay (base rows: kkeep
    1,4,4,5,9,25 -> 1,4,5,5,9,26 -> 1,5,5,5,9,26)."""
    spec = sc.BASE
    case = sc.build(spec)
    kp, vp, pt, ctx = _dev(case)
    q = case.q.to(DEV)
    kk = lambda g: [sc.kkeep_of(spec.sparsity, c + g) for c in spec.ctxs]
    assert kk(0) != kk(1) != kk(2)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):      # warm-up outside the capture
        hip_ops.attn_decode_sparse(q, kp, vp, pt, ctx, case.sparsity,
                                   case.scale, None)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = hip_ops.attn_decode_sparse(q, kp, vp, pt, ctx, case.sparsity,
                                         case.scale, None)
    graph.replay()
    _check("graph-replay-0", out, spec)
    for grow in (1, 2):
        nxt = sc.build(spec, grow)
        for b in range(case.B):
            pg, sl = sc.slot_of(nxt, b, int(nxt.ctx[b]) - 1)
            kp[pg, :, sl, :] = nxt.k_pages[pg, :, sl, :].to(DEV)
            vp[pg, :, :, sl] = nxt.v_pages[pg, :, :, sl].to(DEV)
        ctx.add_(1)
        graph.replay()
        _check(f"graph-replay-{grow}", out, spec, grow)


def test_no_host_sync():
    case = sc.build(sc.BASE)
    kp, vp, pt, ctx = _dev(case)
    q = case.q.to(DEV)
    qkv = sc.qkv_buffer(case).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        hip_ops.attn_decode_sparse(q, kp, vp, pt, ctx, case.sparsity,
                                   case.scale, None)
        ops.set_attn_sparsity(case.sparsity)
        ops.attn_decode(q, kp, vp, pt, ctx, case.scale)
        ops.attn_paged_qkv(qkv, sc.BASE.Hq, sc.BASE.Hkv, kp, vp, pt, ctx - 1,
                           scale=case.scale)
    finally:
        ops.set_attn_sparsity(1.0)
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


def test_llama_decode_step_reaches_the_sparse_kernel():
    """llama decodes through ops.attn_paged_qkv: with the knob set, every
    layer's decode step must run hip_ops.attn_decode_sparse_qkv and the step's
    output must differ from the dense one; the prefill must not."""
    from bloombee_amd.engine import LocalEngine
    from bloombee_amd.ops import interface

    eng = LocalEngine("llama-tiny", device=DEV, seed=1, kv_max_tokens=4096)
    B, T = 2, 24
    gen = torch.Generator().manual_seed(5)
    h = torch.randn(B, T + 1, eng.config.hidden_size, generator=gen).to(
        device=DEV, dtype=eng.config.dtype)
    calls = []
    real = interface.hip_ops

    class _Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name != "attn_decode_sparse_qkv":
                return fn

            def wrapped(*a, **kw):
                calls.append(name)
                return fn(*a, **kw)
            return wrapped

    def run(frac):
        ops.set_attn_sparsity(frac)
        interface.hip_ops = _Spy()
        try:
            kv = eng.kv_pool.allocate(B, 64)
            kv.extend(T)
            pre = eng.stack.forward_inference(
                h[:, :T].clone(), kv,
                torch.zeros(B, dtype=torch.int32, device=DEV))
            kv.extend(1)
            dec = eng.stack.forward_inference(
                h[:, T:].clone(), kv,
                torch.full((B,), T, dtype=torch.int32, device=DEV))
            kv.close()
        finally:
            interface.hip_ops = real
            ops.set_attn_sparsity(1.0)
        return pre.float().cpu(), dec.float().cpu()

    pre_d, dec_d = run(1.0)
    assert calls == []
    pre_s, dec_s = run(0.25)
    assert len(calls) == eng.config.num_hidden_layers
    assert torch.equal(pre_d, pre_s)
    assert bool(torch.isfinite(dec_s).all())
    assert not torch.equal(dec_d, dec_s)
