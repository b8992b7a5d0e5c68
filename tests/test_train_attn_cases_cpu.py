"""CPU guards for the training-attention cases (tests/train_attn_cases.py):
the bounds are wide enough for the kernels' roundings alone and tight enough
that every defect the cases target lands far outside them; the torch
definition agrees with the oracle; and `ops.attn_train` on CPU tensors is
exactly the composition the blocks ran inline before the op existed.
"""
import pytest
import torch

import train_attn_cases as tc
from bloombee_amd import ops
from bloombee_amd.ops import reference as ref

KEYS = ("O", "dQ", "dK", "dV")


def _ratios(got, case):
    want, bound = tc.oracle(case), tc.tol(case)
    return {k: tc.worst(got[k], want[k], bound[k])[0] for k in KEYS}


@pytest.mark.parametrize("name", list(tc.CASES))
def test_roundings_alone_stay_within_tol(name):
    case = tc.build(tc.CASES[name])
    r = _ratios(tc.emulate(case), case)
    print(f"[train-cases] {name} emulation err/tol {r}")
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("name", list(tc.CASES))
def test_reference_under_autograd_matches_oracle(name):
    case = tc.build(tc.CASES[name])
    q, k, v = (t.float().detach().clone().requires_grad_(True)
               for t in (case.q, case.k, case.v))
    out = ref.attn_train(q, k, v, case.scale, case.window, case.slopes)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), case.do.float())
    r = _ratios({"O": out.detach(), "dQ": dq, "dK": dk, "dV": dv}, case)
    print(f"[train-cases] {name} fp32 reference err/tol {r}")
    assert max(r.values()) <= 1.0, r


# mutation -> the case it is aimed at
TARGETS = {
    "causal_plus_one": "base",
    "causal_minus_one": "ragged33",
    "window_off_by_one": "window40",
    "no_delta": "one",
    "no_scale_dq": "mha",
    "no_scale_dk": "mqa5",
    "first_head_of_group": "mqa5",
    "no_alibi_in_backward": "alibi",
    "drop_last_key_tile": "keyblock257",
    "drop_last_query_tile": "ragged33",
    "lse_before_alibi": "alibi",
}


def test_every_mutation_has_a_target():
    assert set(TARGETS) == set(tc.MUTATIONS)


@pytest.mark.parametrize("mutation", list(TARGETS))
def test_mutation_lands_outside_tol(mutation):
    case = tc.build(tc.CASES[TARGETS[mutation]])
    r = _ratios(tc.MUTATIONS[mutation](case), case)
    print(f"[train-cases] {mutation} on {TARGETS[mutation]}: err/tol {r}")
    assert max(r.values()) >= 4.0, r


def test_planting_gives_edges_real_weight():
    """Each planted key of the base case holds at least 2 % of some query
    head's softmax mass, so a kernel that loses it cannot hide in the noise."""
    case = tc.build(tc.CASES["base"])
    p = tc.oracle(case)["_p"]                                   # (B, Hq, T, T)
    for j in case.planted:
        assert float(p[:, :, :, j].amax()) >= 0.02, j


def _inline_composition(q, k, v, scale, window=0, slopes=None):
    """The attention lines every family's forward_train carried before
    ops.attn_train (llama/block.py at that time; bloom's ALiBi add and
    gemma4's window mask merged in). q/k/v are (B, H, T, D) as there."""
    B, Hq, T, D = q.shape
    G = Hq // k.shape[1]
    if G > 1:
        k = k.repeat_interleave(G, dim=1)
        v = v.repeat_interleave(G, dim=1)
    scores = torch.matmul(q.float(), k.float().transpose(-1, -2))
    if scale != 1.0:
        scores = scores * scale
    if slopes is not None:
        scores = scores + slopes.view(1, Hq, 1, 1) * \
            torch.arange(T, dtype=torch.float32).view(1, 1, 1, T)
    qpos = torch.arange(T).view(T, 1)
    kpos = torch.arange(T).view(1, T)
    mask = kpos <= qpos
    if window > 0:
        mask &= kpos > qpos - window
    scores = scores.masked_fill(~mask, float("-inf"))
    p = torch.softmax(scores, dim=-1)
    attn = torch.matmul(p, v.float()).to(q.dtype)
    return attn.permute(0, 2, 1, 3).reshape(B, T, Hq * D)


@pytest.mark.parametrize("name", ["base", "mqa5", "mha", "window40", "alibi", "strided"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_cpu_op_is_the_inline_composition(name, dtype):
    case = tc.build(tc.CASES[name])
    s = case.spec
    q, k, v = (t.to(dtype) for t in (case.q, case.k, case.v))
    want = _inline_composition(*(t.permute(0, 2, 1, 3) for t in (q, k, v)),
                               case.scale, case.window, case.slopes)
    got = ops.attn_train(q, k, v, case.scale, window=case.window,
                         alibi_slopes=case.slopes)
    assert got.shape == (tc.B, s.T, s.Hq, s.D)
    assert torch.equal(got.reshape(tc.B, s.T, s.Hq * s.D), want)
