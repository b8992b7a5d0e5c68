"""Attention kernels vs the dense fp64 reference at the places where they
branch: ragged batches, page / tile / stride / split edges, sliding windows,
ALiBi, every head dim and group width, the fused-QKV forms, rope_kv_write_
and the two revert-switch decode kernels.

Inputs, reference and tolerance come from tests/attn_cases.py: peaked scores,
planted edge positions, shuffled page tables and a pool whose non-live slots
are finite poison. The tolerance is derived there (2^-8 * max|v| per row and
kv head), not measured; every group prints its worst err / tol.
tests/test_attn_cases_cpu.py proves on the CPU that the defects these cases
target (ignored q, lost newest token, off-by-one window, wrong page, wrong
row, wrong kv head, wrong slope, read past ctx) each land > 10 x tol away.
"""
import os
import subprocess
import sys

import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bloombee_amd import ops
    from bloombee_amd.ops import reference as ref

    assert ops.HAVE_HIP_OPS, (
        "HIP extension must be built and loadable on a GPU box (fail-loud policy)"
    )

DEV = "cuda:0"
_WORST = {}


def _note(group, name, ratio):
    """Print the running worst err/tol of a test group (shown with -s / -rP)."""
    if group not in _WORST or not ratio <= _WORST[group][0]:
        _WORST[group] = (ratio, name)
    print(f"[attn-edges] {group}: {name} err/tol {ratio:.3f} "
          f"(group worst {_WORST[group][0]:.3f} at {_WORST[group][1]})")


def _check(group, name, got, want, case):
    got = got.cpu()
    assert bool(torch.isfinite(got.float()).all()), f"{name}: non-finite output"
    ratio = ac.worst_ratio(got, want, case)
    _note(group, name, ratio)
    assert ratio <= 1.0, f"{name}: err / tol = {ratio:.3f}"


def _decode(case, n_split):
    return ops.attn_decode(
        case.q.to(DEV), case.k_pages.to(DEV), case.v_pages.to(DEV),
        case.page_table.to(DEV), case.ctx.to(DEV), window=case.window,
        n_split=n_split, alibi_slopes=case.slopes)


def _qkv_buffer(case, k_sec=None, v_sec=None):
    """(B, Tq, (Hq+2Hkv)*D) fused buffer holding the case's q; the k / v
    sections are given (B, Hkv, Tq, D) tensors or finite junk."""
    s = case.spec
    B, Tq = case.B, case.Tq
    gen = torch.Generator().manual_seed(s.seed)
    junk = lambda: (torch.randn(B, Tq, s.Hkv * s.D, generator=gen) * 8).to(
        torch.bfloat16)
    flat = lambda x: x.permute(0, 2, 1, 3).reshape(B, Tq, -1).to(torch.bfloat16)
    return torch.cat([flat(case.q),
                      junk() if k_sec is None else flat(k_sec),
                      junk() if v_sec is None else flat(v_sec)],
                     dim=-1).contiguous()


def _unflat(out, case):
    s = case.spec
    return out.view(case.B, case.Tq, s.Hq, s.D).permute(0, 2, 1, 3)


# ---------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("spec", ac.DECODE_BOUNDARY, ids=ac.ids(ac.DECODE_BOUNDARY))
def test_decode_boundary_rows(spec):
    """Page / tile / 4-wave stride / double-stride contexts as rows of one
    batch, MAXG=4 (8,2,128) and MAXG=16 (16,2,64) kernels, every split count
    (32 > page count: most splits are empty)."""
    case = ac.build(spec)
    want = ac.dense_ref(case)
    for n_split in (0, 1, 2, 3, 7, 32):
        _check("decode-boundary", f"{spec.name}-ns{n_split}",
               _decode(case, n_split), want, case)


@pytest.mark.parametrize("spec", ac.DECODE_MATRIX, ids=ac.ids(ac.DECODE_MATRIX))
def test_decode_head_dim_group_matrix(spec):
    case = ac.build(spec)
    want = ac.dense_ref(case)
    for n_split in (1, 3):
        _check("decode-matrix", f"{spec.name}-ns{n_split}",
               _decode(case, n_split), want, case)


@pytest.mark.parametrize("spec", ac.DECODE_WINDOW, ids=ac.ids(ac.DECODE_WINDOW))
def test_decode_window(spec):
    """tile0 window skip x split ranges. The window=40 cases at n_split=7
    contain a split ([32,48) of the ctx=100 row, lo=60) whose only tile is
    wholly dead; see attn_cases.DECODE_WINDOW."""
    case = ac.build(spec)
    want = ac.dense_ref(case)
    for n_split in (1, 3, 7):
        _check("decode-window", f"{spec.name}-ns{n_split}",
               _decode(case, n_split), want, case)


@pytest.mark.parametrize("spec", ac.DECODE_ALIBI, ids=ac.ids(ac.DECODE_ALIBI))
def test_decode_alibi(spec):
    case = ac.build(spec)
    want = ac.dense_ref(case)
    for n_split in (1, 3):
        _check("decode-alibi", f"{spec.name}-ns{n_split}",
               _decode(case, n_split), want, case)


@pytest.mark.parametrize("spec", ac.DECODE_FUSED, ids=ac.ids(ac.DECODE_FUSED))
def test_decode_fused_qkv(spec):
    case = ac.build(spec)
    want = ac.dense_ref(case)
    s = spec
    out = ops.attn_paged_qkv(
        _qkv_buffer(case).to(DEV), s.Hq, s.Hkv, case.k_pages.to(DEV),
        case.v_pages.to(DEV), case.page_table.to(DEV), case.q_start.to(DEV),
        window=s.window)
    _check("decode-fused-qkv", spec.name, _unflat(out, case), want, case)


# ---------------------------------------------------------------------------
# prefill
# ---------------------------------------------------------------------------

def _prefill(case):
    return ops.attn_prefill(
        case.q.to(DEV), case.k_pages.to(DEV), case.v_pages.to(DEV),
        case.page_table.to(DEV), case.q_start.to(DEV), window=case.window,
        alibi_slopes=case.slopes)


@pytest.mark.parametrize("spec", ac.PREFILL_SHAPES, ids=ac.ids(ac.PREFILL_SHAPES))
def test_prefill_ragged_q_start(spec):
    case = ac.build(spec)
    _check("prefill-shapes", spec.name, _prefill(case), ac.dense_ref(case), case)


@pytest.mark.parametrize("spec", ac.PREFILL_WINDOW, ids=ac.ids(ac.PREFILL_WINDOW))
def test_prefill_window(spec):
    """kstart x two q-tiles x q_start > 0 (Tq=129), and a short chunk deep in
    the context (Tq=17 at q_start=37)."""
    case = ac.build(spec)
    _check("prefill-window", spec.name, _prefill(case), ac.dense_ref(case), case)


@pytest.mark.parametrize("spec", ac.PREFILL_ALIBI, ids=ac.ids(ac.PREFILL_ALIBI))
def test_prefill_alibi(spec):
    case = ac.build(spec)
    _check("prefill-alibi", spec.name, _prefill(case), ac.dense_ref(case), case)


@pytest.mark.parametrize("spec", ac.PREFILL_FUSED, ids=ac.ids(ac.PREFILL_FUSED))
def test_prefill_fused_qkv(spec):
    """Ragged non-zero q_start through rope_kv_write_ + attn_prefill_qkv. The
    history is pre-written with ref.kv_write into a poisoned pool; the new
    tokens go through rope_kv_write_ with position_ids = 0 (cos 1, sin 0: an
    exact identity rotation), so the pool must come out bit-identical to the
    case's pool and the attention output must match the dense reference."""
    case = ac.build(spec)
    s = spec
    B, Tq = case.B, case.Tq
    kp, vp = case.k_pages.clone(), case.v_pages.clone()
    # put the poison back under the new tokens, keep the history
    gen = torch.Generator().manual_seed(s.seed)
    k_new = torch.empty(B, s.Hkv, Tq, s.D, dtype=torch.bfloat16)
    v_new = torch.empty_like(k_new)
    for b in range(B):
        qs = int(case.q_start[b])
        k_new[b] = case.k[b, :, qs:qs + Tq].to(torch.bfloat16)
        v_new[b] = case.v[b, :, qs:qs + Tq].to(torch.bfloat16)
    sign = lambda x: (torch.randint(0, 2, x.shape, generator=gen) * 2 - 1).to(
        torch.bfloat16) * ac.POISON
    ref.kv_write(sign(k_new), sign(v_new), kp, vp, case.page_table, case.q_start)
    for b in range(B):      # history, written the way the serving path does
        qs = int(case.q_start[b])
        if qs:
            ref.kv_write(case.k[b:b + 1, :, :qs].to(torch.bfloat16),
                         case.v[b:b + 1, :, :qs].to(torch.bfloat16), kp, vp,
                         case.page_table[b:b + 1],
                         torch.zeros(1, dtype=torch.int32))
    assert not torch.equal(kp, case.k_pages)

    qkv = _qkv_buffer(case, k_new, v_new).to(DEV)
    q_before = qkv.clone()
    cos, sin = ref.rope_cos_sin(s.D, 64)
    kp_g, vp_g = kp.to(DEV), vp.to(DEV)
    ops.rope_kv_write_(qkv, s.Hq, s.Hkv, cos.to(DEV), sin.to(DEV),
                       torch.zeros(B, Tq, dtype=torch.int32, device=DEV),
                       kp_g, vp_g, case.page_table.to(DEV),
                       case.q_start.to(DEV))
    assert torch.equal(qkv, q_before), "identity rotation changed qkv"
    assert torch.equal(kp_g.cpu(), case.k_pages), "K pool differs"
    assert torch.equal(vp_g.cpu(), case.v_pages), "V pool differs"
    out = ops.attn_paged_qkv(qkv, s.Hq, s.Hkv, kp_g, vp_g,
                             case.page_table.to(DEV), case.q_start.to(DEV))
    _check("prefill-fused-qkv", spec.name, _unflat(out, case),
           ac.dense_ref(case), case)


# ---------------------------------------------------------------------------
# rope_kv_write_
# ---------------------------------------------------------------------------

def test_rope_kv_write_ragged_positions_poisoned_pool():
    """Ragged start_pos (T=5 crosses a page boundary for rows 1 and 2),
    explicit non-monotonic position_ids, shuffled page table, poisoned pool.
    Live slots and the roped q match the CPU composition within 2^-8 |value|;
    every slot the call does not own keeps its poison bit for bit."""
    gen = torch.Generator().manual_seed(91)
    B, T, Hq, Hkv, D, P = 3, 5, 4, 2, 64, ac.P
    X = Hq + 2 * Hkv
    start = torch.tensor([3, 13, 30], dtype=torch.int32)
    pos = torch.tensor([[7, 2, 40, 2, 0], [13, 14, 15, 16, 17],
                        [99, 3, 98, 4, 97]], dtype=torch.int32)
    maxp, npages = 4, 17
    pt = torch.randperm(npages, generator=gen)[: B * maxp].int().reshape(B, maxp)
    poison = lambda *sh: ((torch.randint(0, 2, sh, generator=gen) * 2 - 1)
                          .to(torch.bfloat16) * ac.POISON)
    kp0, vp0 = poison(npages, Hkv, P, D), poison(npages, Hkv, D, P)
    qkv0 = torch.randn(B, T, X * D, generator=gen).to(torch.bfloat16)
    cos, sin = ref.rope_cos_sin(D, 128)

    live = torch.zeros(npages, P, dtype=torch.bool)
    for b in range(B):
        for t in range(T):
            p = int(start[b]) + t
            live[int(pt[b, p // P]), p % P] = True
    assert int(live.sum()) == B * T

    qkv_c, kp_c, vp_c = qkv0.clone(), kp0.clone(), vp0.clone()
    ops.rope_kv_write_(qkv_c, Hq, Hkv, cos, sin, pos, kp_c, vp_c, pt, start)
    qkv_g, kp_g, vp_g = (x.clone().to(DEV) for x in (qkv0, kp0, vp0))
    ops.rope_kv_write_(qkv_g, Hq, Hkv, cos.to(DEV), sin.to(DEV), pos.to(DEV),
                       kp_g, vp_g, pt.to(DEV), start.to(DEV))
    qkv_g, kp_g, vp_g = qkv_g.cpu(), kp_g.cpu(), vp_g.cpu()

    def close(got, want, what):
        got, want = got.double(), want.double()
        ratio = float(((got - want).abs() /
                       (want.abs() * 2.0 ** -8).clamp_min(1e-30)).max())
        _note("rope-kv-write", what, ratio)
        assert ratio <= 1.0, f"{what}: err / tol = {ratio:.3f}"

    close(qkv_g[..., : Hq * D], qkv_c[..., : Hq * D], "roped q")
    assert torch.equal(qkv_g[..., Hq * D:], qkv0[..., Hq * D:]), \
        "k / v sections of qkv must stay untouched"
    k_slots = lambda x: x.permute(0, 2, 1, 3)      # (np, P, Hkv, D)
    v_slots = lambda x: x.permute(0, 3, 1, 2)      # (np, P, Hkv, D)
    close(k_slots(kp_g)[live], k_slots(kp_c)[live], "live K")
    assert torch.equal(v_slots(vp_g)[live], v_slots(vp_c)[live]), "live V"
    # the CPU composition must itself have moved the live slots off poison
    assert not torch.equal(k_slots(kp_c)[live], k_slots(kp0)[live])
    assert torch.equal(k_slots(kp_g)[~live], k_slots(kp0)[~live]), \
        "a K slot outside the written positions changed"
    assert torch.equal(v_slots(vp_g)[~live], v_slots(vp0)[~live]), \
        "a V slot outside the written positions changed"


# ---------------------------------------------------------------------------
# revert-switch kernels (read once per process -> fresh child each)
# ---------------------------------------------------------------------------

def test_revert_switch_kernels_in_child_processes():
    """BBAMD_ATTN_PF=0 runs the paired-tile NT=2 kernel, BBAMD_ATTN_PF=0
    BBAMD_ATTN_NT=1 the NT=1 kernel for D <= 128. One test owns both children
    so they run one after the other, and the second is not started if the
    first ended by signal or time limit."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for switches in ({"BBAMD_ATTN_PF": "0"},
                     {"BBAMD_ATTN_PF": "0", "BBAMD_ATTN_NT": "1"}):
        env = dict(os.environ)
        env.pop("BBAMD_ATTN_NT", None)
        env.update(switches)
        env["PYTHONPATH"] = os.pathsep.join(
            [root, here] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
        try:
            r = subprocess.run([sys.executable, "-m", "attn_edges_child"],
                               env=env, cwd=here, timeout=120,
                               capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            pytest.fail(f"child {switches} hit the time limit; "
                        "the next child was not started")
        print(r.stdout)
        if r.returncode < 0:
            pytest.fail(f"child {switches} ended by signal {-r.returncode}; "
                        f"the next child was not started\n{r.stderr[-2000:]}")
        assert r.returncode == 0, (
            f"child {switches} exit {r.returncode}\n{r.stdout[-3000:]}\n"
            f"{r.stderr[-3000:]}")
        assert "attn_edges_child ok" in r.stdout
