"""Mixed-device decode on the GPU: device segment on the MFMA / wide decode
kernels in forced-partial mode + the external-partial merge kernel
(hip_ops.attn_decode_mixed) vs the fp32 reference over the concatenated
cache, and per-family hidden-state error of a host-prefixed session.
All tests @pytest.mark.gpu."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bloombee_amd import ops
    from bloombee_amd.ops import reference as ref

    assert ops.HAVE_HIP_OPS, (
        "HIP extension must be built and loadable on a GPU box (fail-loud policy)"
    )

from mixed_device_scenario import FAMILIES, decode_hidden, make_engine

DEV = "cuda:0"
S_HOST = 48
P = 16
# the alibi / wide-head decode parity tolerance of test_gpu_kernels.py: fp32
# merge with a single bf16 rounding at the end is the same error class
ATOL = 3e-2


@functools.lru_cache(maxsize=None)
def build_case(Hq, Hkv, D, ctx_dev, seed=21):
    """bf16 K/V for S_HOST + ctx_dev[b] positions per row, q scaled like the
    decode parity tests. Returns the CPU pieces (never mutated): full K/V per
    row, host prefix (bf16-rounded, held as fp32), device pool with a
    shuffled page table."""
    g = torch.Generator().manual_seed(seed)
    B = len(ctx_dev)
    q = (torch.randn(B, Hq, 1, D, generator=g) / math.sqrt(D)).to(torch.bfloat16)
    full = [(torch.randn(Hkv, S_HOST + c, D, generator=g).to(torch.bfloat16),
             torch.randn(Hkv, S_HOST + c, D, generator=g).to(torch.bfloat16))
            for c in ctx_dev]
    hk = torch.stack([k[:, :S_HOST] for k, _ in full]).float()
    hv = torch.stack([v[:, :S_HOST] for _, v in full]).float()
    maxp = max(ctx_dev) // P + 2
    npages = B * maxp + 3
    pt = torch.randperm(npages, generator=g)[: B * maxp].int().view(B, maxp)
    kp = torch.zeros(npages, Hkv, P, D, dtype=torch.bfloat16)
    vp = torch.zeros(npages, Hkv, D, P, dtype=torch.bfloat16)
    for b, (k, v) in enumerate(full):
        for t in range(ctx_dev[b]):
            pg = pt[b, t // P]
            kp[pg, :, t % P] = k[:, S_HOST + t]
            vp[pg, :, :, t % P] = v[:, S_HOST + t]
    return q, full, hk, hv, kp, vp, pt


def dense_reference(q, full, window=0, slopes=None):
    """The reference: fp32 ref.attn_paged over each row's concatenated
    cache (host prefix + device segment in one paged pool)."""
    B = q.shape[0]
    Hkv, _, D = full[0][0].shape
    lens = [k.shape[1] for k, _ in full]
    maxp = max(lens) // P + 1
    kp = torch.zeros(B * maxp, Hkv, P, D)
    vp = torch.zeros(B * maxp, Hkv, D, P)
    pt = torch.arange(B * maxp, dtype=torch.int32).view(B, maxp)
    for b, (k, v) in enumerate(full):
        ref.kv_write(k.float()[None], v.float()[None], kp, vp, pt[b:b + 1],
                     torch.zeros(1, dtype=torch.int32))
    out = ref.attn_paged(q.float(), kp, vp, pt, torch.tensor(lens) - 1,
                         1.0 / math.sqrt(D),
                         sliding_window=window if window > 0 else None,
                         alibi_slopes=slopes)
    return out[:, :, 0]


def dense_alibi_variant(q, full, slopes, dev_pos_offset):
    """fp32 softmax attention over the concatenated cache with the device
    positions' ALiBi bias starting at dev_pos_offset: S_HOST is the correct
    result, 0 is what a merge WITHOUT the per-head device shift computes."""
    B, Hq, _, D = q.shape
    out = torch.empty(B, Hq, D)
    for b, (k, v) in enumerate(full):
        Hkv, S, _ = k.shape
        G = Hq // Hkv
        kf = k.float().repeat_interleave(G, dim=0)
        vf = v.float().repeat_interleave(G, dim=0)
        s = torch.einsum("hd,hcd->hc", q[b, :, 0].float(), kf) / math.sqrt(D)
        pos = torch.arange(S)
        bias_pos = torch.where(pos < S_HOST, pos,
                               pos - S_HOST + dev_pos_offset).float()
        s = s + slopes.view(-1, 1) * bias_pos.view(1, S)
        out[b] = torch.einsum("hc,hcd->hd", torch.softmax(s, -1), vf)
    return out


def run_mixed(case, n_split, window=0, slopes=None):
    q, full, hk, hv, kp, vp, pt = case
    ctx = torch.tensor([k.shape[1] - S_HOST for k, _ in full],
                       dtype=torch.int32)
    got = ops.attn_paged_mixed(q.to(DEV), kp.to(DEV), vp.to(DEV), pt.to(DEV),
                               ctx.to(DEV), hk, hv, window=window,
                               alibi_slopes=slopes, n_split=n_split)
    assert got.shape == q.shape
    return got[:, :, 0].float().cpu()


def check(case, want, n_split, label, **kw):
    got = run_mixed(case, n_split, **kw)
    err = (got - want).abs().max().item()
    print(f"{label} n_split={n_split} max err {err:.4g}")
    assert err <= ATOL, (label, n_split, err)


# (Hq, Hkv, D, device ctx per row)
SHAPES = {
    # G 4 -> MAXG 4; forced-partial epilogue at n_split 1, split path at 3;
    # page (16) and KV-tile (32) boundaries
    "a1": (8, 2, 128, (1,)),
    "a17": (8, 2, 128, (17,)),
    "a33": (8, 2, 128, (33,)),
    "a100": (8, 2, 128, (100,)),
    "b": (16, 2, 64, (33,)),           # G 8 -> MAXG 16
    "c": (20, 1, 64, (33,)),           # falcon-style MQA, two head chunks
    "f": (4, 2, 512, (33,)),           # wide kernel
    "g": (8, 2, 128, (1, 17, 40)),     # per-row device ctx differs
}


@pytest.mark.parametrize("n_split", [1, 3])
@pytest.mark.parametrize("name", list(SHAPES))
def test_mixed_kernel_parity(name, n_split):
    Hq, Hkv, D, ctx_dev = SHAPES[name]
    case = build_case(Hq, Hkv, D, ctx_dev)
    want = dense_reference(case[0], case[1])
    check(case, want, n_split, name)


@pytest.mark.parametrize("n_split", [1, 3])
def test_mixed_kernel_alibi_shift(n_split):
    """Case d: ALiBi. The kernels bias device positions with LOCAL indices;
    the merge must add slope * pos_offset (24 nats for head 0, slope 0.5) to
    the device partials. A merge without that shift is far outside the
    tolerance — computed here with the reference maths, not a wrong kernel."""
    Hq = 8
    case = build_case(Hq, Hq, 64, (17,))
    slopes = ops.alibi_slopes_for(Hq)
    assert slopes[0] == 0.5
    want = dense_reference(case[0], case[1], slopes=slopes)
    # the variant's maths reproduces the reference at the correct offset
    assert torch.allclose(
        dense_alibi_variant(case[0], case[1], slopes, S_HOST), want, atol=1e-5)
    unshifted = dense_alibi_variant(case[0], case[1], slopes, 0)
    gap = (want - unshifted).abs().max().item()
    print(f"d: |correct - unshifted merge| max {gap:.4g}")
    assert gap > 10 * ATOL, gap
    check(case, want, n_split, "d", slopes=slopes)


@pytest.mark.parametrize("n_split", [1, 3])
@pytest.mark.parametrize("window", [8, 17, 40])
def test_mixed_kernel_sliding_window(window, n_split):
    """Case e: D 256, device ctx 17. window 8 / 17 exclude the host prefix
    (plain attn_decode), 40 keeps a partial host suffix."""
    case = build_case(4, 2, 256, (17,))
    want = dense_reference(case[0], case[1], window=window)
    check(case, want, n_split, f"e window={window}", window=window)


def test_mixed_kernel_window_rows_differ():
    """Per-row device ctx with a window: row 0 keeps a host suffix, row 2's
    window excludes the host prefix (external partial with l == 0)."""
    case = build_case(8, 2, 128, (1, 17, 40))
    want = dense_reference(case[0], case[1], window=24)
    for n_split in (1, 3):
        check(case, want, n_split, "g window=24", window=24)


def test_mixed_kernel_fused_qkv_form():
    """ops.attn_paged_mixed_qkv reads q in place from the fused QKV buffer
    and returns the O-projection layout."""
    Hq, Hkv, D = 8, 2, 128
    case = build_case(Hq, Hkv, D, (1, 17, 40))
    q, full, hk, hv, kp, vp, pt = case
    B = q.shape[0]
    want = dense_reference(q, full)
    qkv = torch.zeros(B, 1, (Hq + 2 * Hkv) * D, dtype=torch.bfloat16)
    qkv[..., : Hq * D] = q[:, :, 0].reshape(B, 1, Hq * D)
    ctx = torch.tensor([1, 17, 40], dtype=torch.int32)
    got = ops.attn_paged_mixed_qkv(qkv.to(DEV), Hq, Hkv, kp.to(DEV),
                                   vp.to(DEV), pt.to(DEV), ctx.to(DEV),
                                   hk, hv)
    assert got.shape == (B, 1, Hq * D)
    err = (got.float().cpu().view(B, Hq, D) - want).abs().max().item()
    print(f"fused-qkv form max err {err:.4g}")
    assert err <= ATOL, err


def test_mixed_composition_switch(monkeypatch):
    """BBAMD_MIXED_KERNEL=0 keeps the torch composition on the GPU."""
    from bloombee_amd.ops import interface as iface
    monkeypatch.setattr(iface, "_MIXED_KERNEL", False)
    case = build_case(8, 2, 128, (17,))
    want = dense_reference(case[0], case[1])
    check(case, want, 0, "composition")


@pytest.mark.parametrize("model", FAMILIES)
def test_mixed_device_decode_family_gpu(model):
    """Host-prefixed decode on the GPU is as close to the CPU reference run
    as the never-swapped GPU run: e_mixed <= 2 * e_dense + 2**-8 * max|dense|
    (same bf16-kernel-vs-reference error class; the factor 2 covers the
    extra merge stage)."""
    cpu = make_engine(model)
    want = decode_hidden(cpu, swapped=False)
    gpu = make_engine(model, DEV, weights_from=cpu)
    e_dense = (decode_hidden(gpu, swapped=False) - want).abs().max().item()
    e_mixed = (decode_hidden(gpu, swapped=True) - want).abs().max().item()
    peak = want.abs().max().item()
    print(f"{model}: max|dense| {peak:.4g} e_dense {e_dense:.4g} "
          f"e_mixed {e_mixed:.4g}")
    assert e_mixed <= 2 * e_dense + 2 ** -8 * peak, (e_dense, e_mixed, peak)
