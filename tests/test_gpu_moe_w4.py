"""The grouped W4 MoE GEMM (moe_gemm_w4.hip) on the device.

Exact cases: every case of tests/moe_w4_cases.py through the raw op and,
where ksplit = 0, through `ops.moe_gemm_grouped_w4`, `torch.equal` to the
fp64 expectation (test_moe_w4_cases_cpu.py shows what each defect would
move). Which case reaches which path (ids are the spec names):
  one half-filled stage, nothing prefetched   *-k128-*
  one full stage and a half one               *-k384-*
  XCD remap, gridDim.x % 8 == 1               *-n576-*
  m-chunks beyond the first, ragged           every case (a group of 33..70)
  launched chunks with no rows                *-chunks-plus*
  split-K slabs and the combine               *-ks2-*, *-ks3-* (uneven last
                                              split), *-k2048-ks0-* (rule: 4)

Realistic values: randn activations and quant4_pack'ed randn weights against
fp64, bound = gemm_cases.realistic_bound with the W4 term 2^-10 sum|a w|,
times the slot scale (derived in the gemm_cases docstring). Worst observed
|err| / bound on an MI355X: see profiles/r05_moe_w4.md.

Block level: the quantized mixtral-tiny block's grouped path against its
per-expert loop, and the grouped expert path under graph capture. The
capture covers `_grouped_experts` (both GEMMs, SwiGLU, scatter-add) with the
routing tensors in static buffers, not the routing itself: the routing sort
uses torch.bincount, which reads its bin count back to the host and is not
capturable; it is shared with the bf16 path and is not this kernel's.
"""
import math

import pytest
import torch

import gemm_cases as gc
import moe_w4_cases as mc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bloombee_amd import ops
    from bloombee_amd.ops import reference as ref

    assert ops.HAVE_HIP_OPS, (
        "HIP extension must be built and loadable on a GPU box (fail-loud policy)"
    )

DEV = "cuda:0"
BF = torch.bfloat16


def assert_exact(got, want, live, what):
    """torch.equal against the fp64 expectation on the rows of non-empty
    groups, with the worst element."""
    got = got.detach().cpu().double().reshape(want.shape)[live]
    want = want[live]
    if torch.equal(got, want):
        return
    err = (got - want).abs()
    err[got.isnan()] = float("inf")
    flat = int(err.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), want.shape))
    raise AssertionError(
        f"{what}: {int((err > 0).sum())} of {want.numel()} elements differ; "
        f"worst at {idx}: got {float(got[idx])}, want {float(want[idx])}")


def _device_inputs(c):
    return dict(
        A=c.A.to(BF).to(DEV), packed=c.packed.to(DEV),
        scale=c.scale.half().to(DEV), zero=c.zero.half().to(DEV),
        off=c.off.to(DEV),
        rowmap=None if c.rowmap is None else c.rowmap.to(DEV),
        slot_scale=None if c.slot_scale is None else c.slot_scale.float().to(DEV))


@pytest.mark.parametrize("spec", mc.CASES, ids=mc.ids(mc.CASES))
def test_moe_gemm_w4_exact(spec):
    c = mc.build(spec)
    d = _device_inputs(c)
    live = torch.arange(c.S)           # every slot belongs to a non-empty group
    assert int(c.off[-1]) == c.S
    got = ops.hip_ops.moe_gemm_w4(d["A"], d["packed"], d["scale"], d["zero"],
                                  d["off"], d["rowmap"], d["slot_scale"],
                                  c.S, c.mchunks, spec.ksplit)
    assert got.dtype == BF and tuple(got.shape) == (c.S, spec.N)
    assert_exact(got, c.want, live, f"{spec.name} raw op")
    if spec.ksplit == 0:
        got = ops.moe_gemm_grouped_w4(d["A"], d["packed"], d["scale"], d["zero"],
                                      d["off"], rowmap=d["rowmap"],
                                      slot_scale=d["slot_scale"], S=c.S,
                                      mchunks=c.mchunks)
        assert_exact(got, c.want, live, f"{spec.name} ops.moe_gemm_grouped_w4")


def test_moe_gemm_w4_argument_checks():
    c = mc.build(mc.CASES[0])
    d = _device_inputs(c)
    args = [d["A"], d["packed"], d["scale"], d["zero"], d["off"], d["rowmap"],
            d["slot_scale"], c.S, c.mchunks, 1]
    for i in range(7):                 # every tensor argument gets a device check
        bad = list(args)
        bad[i] = bad[i].cpu()
        with pytest.raises(RuntimeError, match="must be on device"):
            ops.hip_ops.moe_gemm_w4(*bad)
    bad = list(args)
    bad[0] = bad[0].half()
    with pytest.raises(RuntimeError, match="bf16"):
        ops.hip_ops.moe_gemm_w4(*bad)
    bad = list(args)
    bad[4] = bad[4][:-1].contiguous()
    with pytest.raises(RuntimeError):
        ops.hip_ops.moe_gemm_w4(*bad)


# ---------------------------------------------------------------------------
# realistic values
# ---------------------------------------------------------------------------

def _ratio(got, want, bound, what):
    err = (got.detach().cpu().double() - want).abs()
    r = float(torch.where(bound > 0, err / bound,
                          torch.where(err > 0, math.inf, 0.0)).max())
    print(f"worst |err| / bound, {what}: {r:.3f}")
    assert r <= 1.0, f"{what}: |err| reaches {r:.3f} x the derived bound"
    return r


@pytest.fixture(scope="module")
def realistic():
    """randn activations, quant4_pack'ed randn weights, the fp64 result and
    its derived bound; built once and left unchanged."""
    gen = torch.Generator().manual_seed(105)
    counts, N, K, Ta = (0, 33, 17, 65), 576, 1152, 40
    E, S = len(counts), sum(counts)
    a = torch.randn(Ta, K, generator=gen).to(BF)
    packed, scale, zero = ref.quant4_pack(torch.randn(E, N, K, generator=gen) * K ** -0.5)
    q = torch.stack([(packed & 0xF).double(), (packed >> 4).double()], dim=-1)
    wd = (q.reshape(E, N, K // 64, 64) * scale.double()[..., None]
          + zero.double()[..., None]).reshape(E, N, K)          # exact in fp64
    off = torch.zeros(E + 1, dtype=torch.int32)
    off[1:] = torch.tensor(counts).cumsum(0).int()
    rm = torch.randint(0, Ta, (S,), generator=gen).int()
    sc = torch.rand(S, generator=gen)
    eid = torch.repeat_interleave(torch.arange(E), torch.tensor(counts))
    ad, ws = a.double()[rm.long()], wd[eid]
    want = torch.einsum("sk,snk->sn", ad, ws) * sc.double()[:, None]
    absprod = torch.einsum("sk,snk->sn", ad.abs(), ws.abs()) * sc.double()[:, None]
    bound = gc.realistic_bound(want, K, absprod, extra=2.0 ** -10 * absprod)
    dev = dict(A=a.to(DEV), packed=packed.reshape(E, N, K // 2).to(DEV),
               scale=scale.to(DEV), zero=zero.to(DEV), off=off.to(DEV),
               rm=rm.to(DEV), sc=sc.to(DEV))
    return dict(dev=dev, S=S, K=K, want=want, bound=bound)


@pytest.mark.parametrize("ks", [1, 3], ids=["unsplit", "split-k"])
def test_moe_gemm_w4_realistic(realistic, ks):
    d = realistic["dev"]
    got = ops.hip_ops.moe_gemm_w4(d["A"], d["packed"], d["scale"], d["zero"],
                                  d["off"], d["rm"], d["sc"], realistic["S"], 3, ks)
    _ratio(got, realistic["want"], realistic["bound"], f"moe_gemm_w4 ks={ks}")


def test_kernel_versus_composition(realistic, monkeypatch):
    d = realistic["dev"]

    def run():
        return ops.moe_gemm_grouped_w4(d["A"], d["packed"], d["scale"], d["zero"],
                                       d["off"], rowmap=d["rm"], slot_scale=d["sc"],
                                       S=realistic["S"], mchunks=3)

    monkeypatch.delenv("BBAMD_MOE_W4_KERNEL", raising=False)
    kern = run()
    monkeypatch.setenv("BBAMD_MOE_W4_KERNEL", "0")
    comp = run()
    monkeypatch.delenv("BBAMD_MOE_W4_KERNEL")
    assert not torch.equal(kern, comp)     # the switch took another path
    _ratio(comp, kern.cpu().double(), realistic["bound"],
           "composition (BBAMD_MOE_W4_KERNEL=0) vs kernel")


# ---------------------------------------------------------------------------
# the quantized Mixtral block
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def qblock():
    from bloombee_amd.engine import BlockStack
    from bloombee_amd.models.base import resolve_config

    cfg = resolve_config("mixtral-tiny")
    blk = BlockStack(cfg, 0, 1, device=DEV, seed=3).blocks[0]
    # widen router margins so near-ties cannot flip top-k between the two
    # MoE implementations' (identical) routing math
    rw = torch.randn(blk.router_w.shape, generator=torch.Generator().manual_seed(42))
    with torch.no_grad():
        blk.router_w.copy_(rw.to(cfg.dtype))
    blk.quantize_weights_q4()
    assert blk.expert_down_w.numel() == 0
    return cfg, blk


def test_mixtral_block_grouped_w4_vs_loop(qblock, monkeypatch):
    cfg, blk = qblock
    calls = []
    real = ops.hip_ops.moe_gemm_w4
    monkeypatch.setattr(ops.hip_ops, "moe_gemm_w4",
                        lambda *a: calls.append(1) or real(*a))
    gen = torch.Generator().manual_seed(2)
    for B, T in [(4, 10), (7, 1), (32, 1)]:
        y = (torch.randn(B, T, cfg.hidden_size, generator=gen) * 0.1) \
            .to(cfg.dtype).to(DEV)
        blk.moe_loop = False
        out_grp = blk._moe(y)
        n = len(calls)
        blk.moe_loop = True
        out_loop = blk._moe(y)
        blk.moe_loop = False
        assert n > 0 and n % 2 == 0 and len(calls) == n     # grouped path only
        worst = (out_grp.float() - out_loop.float()).abs().max().item()
        print(f"grouped W4 vs loop, B={B} T={T}: max |diff| {worst:.3e}")
        assert torch.allclose(out_grp.float(), out_loop.float(), atol=2e-2), \
            (B, T, worst)


def _routing(blk, flat):
    """the routing tensors of MixtralBlock._moe, computed eagerly"""
    logits = ops.linear(flat, blk.router_w).float()
    weights, experts = logits.topk(blk.topk, dim=-1)
    weights = torch.softmax(weights, dim=-1).to(flat.dtype)
    fe = experts.reshape(-1)
    order = fe.argsort(stable=True)
    off = torch.zeros(blk.E + 1, dtype=torch.int32, device=flat.device)
    off[1:] = torch.bincount(fe, minlength=blk.E).cumsum(0).int()
    return off, (order // blk.topk).int(), weights.reshape(-1)[order].float()


def test_grouped_w4_experts_graph_replay(qblock):
    cfg, blk = qblock
    gen = torch.Generator().manual_seed(7)
    B = 8
    y1, y2 = ((torch.randn(B, cfg.hidden_size, generator=gen) * 0.1)
              .to(cfg.dtype).to(DEV) for _ in range(2))
    r1, r2 = _routing(blk, y1), _routing(blk, y2)
    assert not torch.equal(r1[0], r2[0])                 # y2 routes differently
    eager2 = blk._grouped_experts(y2, *r2).clone()
    # eager equals the block's own _moe: same ops on the same routing
    assert torch.equal(blk._moe(y2.view(B, 1, -1)).view(B, -1), eager2)

    static = [y1.clone()] + [t.clone() for t in r1]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # warm up off the capture
        blk._grouped_experts(*static)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = blk._grouped_experts(*static)
    for dst, src in zip(static, (y2,) + r2):
        dst.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager2)
