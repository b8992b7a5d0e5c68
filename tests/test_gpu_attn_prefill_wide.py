"""Prefill attention at head dim 512 (attn_prefill_wide.hip) against the dense
fp64 reference of tests/attn_cases.py, within its derived tolerance
(2^-8 * max|v| per row and kv head): ragged q_start on both sides of the
64-row q-tile, every group width, windows, ALiBi, the fused-QKV and tree-mask
forms, and the routing of the public entry points."""
import os
import subprocess
import sys

import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bloombee_amd import ops
    from bloombee_amd.ops import interface as iface
    from bloombee_amd.ops import reference as ref

DEV = "cuda:0"
D = 512

SHAPES = [ac.prefill_spec(f"wide-T{Tq}-G{Hq // Hkv}", Hq, Hkv, D, (0, 5, 16, 37), Tq,
                          marks=(16, 32, 64, 128))
          for Tq, Hq, Hkv in [(1, 2, 2), (17, 4, 1), (63, 2, 2), (64, 2, 1), (65, 4, 2),
                              (129, 4, 2), (129, 8, 1)]]
WINDOWS = [ac.prefill_spec(f"wide-w{w}-T129", 4, 2, D, (0, 5, 16, 37), 129, window=w,
                           marks=(32, 64, 128)) for w in (1, 17, 40, 1000)] + [
    ac.prefill_spec(f"wide-w{w}-T17", 4, 2, D, (37, 0, 50), 17, window=w,
                    marks=(32,)) for w in (17, 40)]
ALIBI = [ac.prefill_spec("wide-alibi", 4, 4, D, (5, 0, 20), 33, alibi=True)]
CHUNK = ac.prefill_spec("wide-chunk", 4, 2, D, (37, 0, 50), 17)


def _check(name, got, want, case):
    got = got.cpu()
    assert bool(torch.isfinite(got.float()).all()), f"{name}: non-finite output"
    ratio = ac.worst_ratio(got, want.double(), case)
    print(f"[prefill-wide] {name} err/tol {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: err / tol = {ratio:.3f}"


def _prefill(case):
    return ops.attn_prefill(
        case.q.to(DEV), case.k_pages.to(DEV), case.v_pages.to(DEV),
        case.page_table.to(DEV), case.q_start.to(DEV), window=case.window,
        alibi_slopes=case.slopes)


@pytest.mark.parametrize("spec", SHAPES + WINDOWS + ALIBI, ids=ac.ids(SHAPES + WINDOWS + ALIBI))
def test_prefill_wide(spec, monkeypatch):
    """The public entry must be served by the kernel: the composition raises."""
    def composition(*a, **k):
        raise AssertionError("ops.attn_prefill at D=512 reached the torch composition")
    case = ac.build(spec)
    want = ac.dense_ref(case)
    monkeypatch.setattr(iface.ref, "attn_paged", composition)
    _check(spec.name, _prefill(case), want, case)


def test_prefill_wide_direct_binding():
    case = ac.build(SHAPES[4])
    got = iface.hip_ops.attn_prefill(
        case.q.to(DEV), case.k_pages.to(DEV), case.v_pages.to(DEV),
        case.page_table.to(DEV), case.q_start.to(DEV), case.scale, 0, None, None)
    _check("direct", got, ac.dense_ref(case), case)


def test_prefill_wide_fused_qkv():
    """q read in place from (B, Tq, (Hq+2Hkv)*512); k / v sections are junk."""
    case, s = ac.build(CHUNK), CHUNK
    gen = torch.Generator().manual_seed(s.seed)
    qkv = (torch.randn(case.B, case.Tq, (s.Hq + 2 * s.Hkv) * D, generator=gen) * 8).bfloat16()
    qkv[..., : s.Hq * D] = case.q.permute(0, 2, 1, 3).reshape(case.B, case.Tq, -1)
    out = ops.attn_paged_qkv(qkv.to(DEV), s.Hq, s.Hkv, case.k_pages.to(DEV),
                             case.v_pages.to(DEV), case.page_table.to(DEV),
                             case.q_start.to(DEV))
    _check("fused-qkv", out.view(case.B, case.Tq, s.Hq, D).permute(0, 2, 1, 3),
           ac.dense_ref(case), case)


def test_prefill_wide_tree_mask(monkeypatch):
    """Random-parent tree over the 17 new tokens. ac.tol is an upper bound
    here: a tree mask only removes visible positions."""
    from bloombee_amd.spec.tree import TokenTree
    case = ac.build(CHUNK)
    gen = torch.Generator().manual_seed(0)
    tree = TokenTree()
    for i in range(case.Tq):
        tree.add(i, -1 if i == 0 else int(torch.randint(0, i, (1,), generator=gen)), 0.5)
    tm = tree.attention_mask().unsqueeze(0).expand(case.B, -1, -1).contiguous()
    want = ref.attn_paged(case.q.float(), case.k_pages.float(), case.v_pages.float(),
                          case.page_table, case.q_start.long(), case.scale, tree_mask=tm)
    monkeypatch.setattr(iface.ref, "attn_paged", None)     # the kernel must serve it
    got = ops.attn_paged(case.q.to(DEV), case.k_pages.to(DEV), case.v_pages.to(DEV),
                         case.page_table.to(DEV), case.q_start.to(DEV), tree_mask=tm)
    _check("tree-mask", got, want, case)


@pytest.mark.parametrize("q_start,served_by_kernel", [(50, True), (2030, True), (2031, False)])
def test_prefill_wide_routing_by_live_context(q_start, served_by_kernel, monkeypatch):
    """Few workgroups under a page table as wide as a session's capacity
    (8192 positions): a short live context must be served by the kernel, and
    the composition takes over only from 2048 live positions (<= 16
    workgroups). Either way the result meets the bound."""
    case = ac.build(ac.prefill_spec(f"wide-route-{q_start}", 2, 1, D, (q_start, 0), 17))
    want = ac.dense_ref(case)
    table = torch.zeros(case.B, 8192 // ac.P, dtype=torch.int32)
    table[:, : case.maxp] = case.page_table
    calls, orig = [], ref.attn_paged
    monkeypatch.setattr(iface.ref, "attn_paged",
                        lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    got = ops.attn_prefill(case.q.to(DEV), case.k_pages.to(DEV), case.v_pages.to(DEV),
                           table.to(DEV), case.q_start.to(DEV))
    assert bool(calls) != served_by_kernel
    _check(case.spec.name, got, want, case)


def test_prefill_wide_revert_switch_in_child_process():
    """BBAMD_PREFILL_WIDE=0 is read at import: one fresh child, run once."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, BBAMD_PREFILL_WIDE="0")
    env["PYTHONPATH"] = os.pathsep.join(
        [os.path.dirname(here), here] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    code = ("import torch, attn_cases as ac, test_gpu_attn_prefill_wide as t\n"
            "calls = []\n"
            "orig = t.ref.attn_paged\n"
            "t.iface.ref.attn_paged = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]\n"
            "case = ac.build(t.CHUNK)\n"
            "t._check('revert', t._prefill(case), ac.dense_ref(case), case)\n"
            "print('composition calls', len(calls))\n")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=here, timeout=120,
                       capture_output=True, text=True)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    assert "composition calls 1" in r.stdout, r.stdout
