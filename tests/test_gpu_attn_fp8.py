"""Attention over an fp8 (e4m3) KV pool against the dense fp64 reference of
tests/attn_cases.py. A case is attn_cases.build(spec) with k, v and both pools
rounded through clamp -> e4m3, so the pool holds exactly the values dense_ref
sees. e4m3 -> bf16 is exact and q and P stay bf16, so the derived tolerance
(2^-8 * max|v| per row and kv head) holds unchanged. Row sets add the fp8
kernel's own edges: its 64-position tile (ctx 63 / 64 / 65) and its wave
stride 256, pipelined two at a time (ctx 257, 511 / 512 / 513)."""
import copy
import functools

import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bloombee_amd import ops
    from bloombee_amd.ops import reference as ref

    assert ops.HAVE_HIP_OPS, "the HIP extension must load on a GPU box"

DEV = "cuda:0"
FP8 = torch.float8_e4m3fn


def _fp8(x):
    return x.float().clamp(-448, 448).to(FP8)


@functools.lru_cache(maxsize=None)
def fp8_case(spec):
    """A copy of the shared cached case (left unchanged) on e4m3 values."""
    c = copy.copy(ac.build(spec))
    c.k, c.v = _fp8(c.k).double(), _fp8(c.v).double()
    c.k8, c.v8 = _fp8(c.k_pages), _fp8(c.v_pages)       # what the kernels read
    c.k_pages, c.v_pages = c.k8.float(), c.v8.float()   # what dense_ref reads
    return c


def _check(name, got, want, case):
    got = got.cpu()
    assert bool(torch.isfinite(got.float()).all()), f"{name}: non-finite output"
    ratio = ac.worst_ratio(got, want, case)
    print(f"[attn-fp8] {name} err/tol {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: err / tol = {ratio:.3f}"


def _pool(case):
    return case.k8.to(DEV), case.v8.to(DEV), case.page_table.to(DEV)


def _decode(case, n_split):
    return ops.attn_decode(case.q.to(DEV), *_pool(case), case.ctx.to(DEV),
                           window=case.window, n_split=n_split,
                           alibi_slopes=case.slopes)


def _prefill(case):
    return ops.attn_prefill(case.q.to(DEV), *_pool(case), case.q_start.to(DEV),
                            window=case.window, alibi_slopes=case.slopes)


_ROWS = ac.ROW_SETS + [(63, 64, 65, 2), (511, 512, 513, 257)]
_MARKS = ac._ROW_MARKS + [(16, 48, 64), (64, 256, 320, 512)]
DECODE_ROWS = [
    ac.decode_spec(f"f8-dec-b{i}-D{D}-Hq{Hq}-Hkv{Hkv}", Hq, Hkv, D, rows,
                   marks=_MARKS[i], seed=100 + i)
    for D in (64, 128)
    for (Hq, Hkv) in ((8, 2), (4, 4), (71, 1))
    for i, rows in enumerate(_ROWS)
]
DECODE_MASKED = [
    # ctx 200, window 90: lo = 110 lies inside the tile [64, 128)
    ac.decode_spec("f8-dec-w90", 8, 2, 128, (200, 131, 70, 16), window=90,
                   marks=(64, 128), seed=120),
    ac.decode_spec("f8-dec-alibi", 4, 4, 64, (70, 33, 17, 5), alibi=True,
                   marks=(16, 32, 64), seed=121),
]
PREFILL = [
    ac.prefill_spec(f"f8-pre-T{Tq}-D{D}", 8, 2, D, (0, 17, 129), Tq,
                    marks=(16, 32, 128), seed=130 + i)
    for i, (Tq, D) in enumerate([(65, 64), (65, 128), (130, 64), (130, 128)])
] + [
    ac.prefill_spec("f8-pre-w17", 8, 2, 64, (0, 17, 129), 65, window=17,
                    marks=(32, 128), seed=140),
    ac.prefill_spec("f8-pre-alibi", 4, 4, 64, (5, 0, 20), 33, alibi=True,
                    marks=(16, 32), seed=141),
]
FUSED = [
    ac.decode_spec("f8-dec-qkv", 8, 2, 128, (100, 77, 41, 16), marks=(32, 64),
                   seed=150),
    ac.prefill_spec("f8-pre-qkv", 8, 2, 128, (3, 0, 21), 40, marks=(16, 32),
                    seed=151),
]
TREE = ac.prefill_spec("f8-tree", 8, 2, 128, (50, 0, 21), 17, marks=(16, 32),
                       seed=160)


@pytest.mark.parametrize("spec", DECODE_ROWS + DECODE_MASKED,
                         ids=ac.ids(DECODE_ROWS + DECODE_MASKED))
def test_decode_fp8(spec):
    case = fp8_case(spec)
    want = ac.dense_ref(case)
    for n_split in (0, 2, 3):
        _check(f"{spec.name}-ns{n_split}", _decode(case, n_split), want, case)


@pytest.mark.parametrize("spec", PREFILL, ids=ac.ids(PREFILL))
def test_prefill_fp8(spec):
    case = fp8_case(spec)
    _check(spec.name, _prefill(case), ac.dense_ref(case), case)


@pytest.mark.parametrize("spec", FUSED, ids=ac.ids(FUSED))
def test_fused_qkv_fp8(spec):
    """q read in place, strided, from the fused QKV buffer (junk k / v
    sections): attn_decode_qkv at Tq == 1, attn_prefill_qkv otherwise."""
    case = fp8_case(spec)
    s, B, Tq = spec, case.B, case.Tq
    gen = torch.Generator().manual_seed(s.seed)
    junk = (torch.randn(B, Tq, 2 * s.Hkv * s.D, generator=gen) * 8).bfloat16()
    qkv = torch.cat([case.q.permute(0, 2, 1, 3).reshape(B, Tq, -1), junk],
                    dim=-1).contiguous()
    out = ops.attn_paged_qkv(qkv.to(DEV), s.Hq, s.Hkv, *_pool(case),
                             case.q_start.to(DEV))
    _check(spec.name, out.view(B, Tq, s.Hq, s.D).permute(0, 2, 1, 3),
           ac.dense_ref(case), case)


def test_tree_mask_fp8():
    """Random-parent tree over the 17 new tokens. ac.tol is an upper bound
    here: a tree mask only removes visible positions."""
    from bloombee_amd.spec.tree import TokenTree
    case = fp8_case(TREE)
    gen = torch.Generator().manual_seed(0)
    tree = TokenTree()
    for i in range(case.Tq):
        tree.add(i, -1 if i == 0 else int(torch.randint(0, i, (1,), generator=gen)), 0.5)
    tm = tree.attention_mask().unsqueeze(0).expand(case.B, -1, -1).contiguous()
    want = ref.attn_paged(case.q.float(), case.k_pages, case.v_pages,
                          case.page_table, case.q_start.long(), case.scale,
                          tree_mask=tm)
    got = ops.attn_paged(case.q.to(DEV), *_pool(case), case.q_start.to(DEV),
                         tree_mask=tm)
    _check(TREE.name, got, want.double(), case)


@pytest.mark.parametrize("spec", [DECODE_ROWS[5], DECODE_MASKED[0],
                                  DECODE_MASKED[1], PREFILL[3]],
                         ids=lambda s: s.name)
def test_mutations_are_seen_fp8(spec):
    """The test can fail: every applicable deliberate error of the reference
    lands more than the tolerance away from the fp8 kernel's output."""
    case = fp8_case(spec)
    got = (_decode(case, 2) if case.Tq == 1 else _prefill(case)).cpu()
    for name in ac.applicable(spec):
        ratio = ac.worst_ratio(got, ac.dense_ref(case, **ac.MUTATIONS[name]), case)
        print(f"[attn-fp8] {spec.name} mutation {name} err/tol {ratio:.1f}")
        assert ratio > 1.0, f"{spec.name}: mutation {name} not seen ({ratio:.3f})"
