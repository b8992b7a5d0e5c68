"""Packed skinny-GEMM weights (ops.pack_skinny_w), the parts that need no GPU.

  1. unpack(pack(W)) == W for the identity and the SwiGLU row map;
  2. an emulation of gemm_skinny_v2_kernel's lane addressing: for every
     (tile, wave, lane, k-block) the 8 elements at the packed address are the
     8 elements the row-major address expression names, for both maps and
     for a split-K slice;
  3. the LLaMA block's packed-copy cache: built once, dropped or rebuilt by
     fold, unfold, Q4 quantization, an in-place write (_version) and a
     load_state_dict; BBAMD_PACK_W=0 and the CPU's "auto" never pack.
"""
import pytest
import torch

from bloombee_amd import ops
from bloombee_amd.ops import reference as ref

BF = torch.bfloat16


def _w(N, K, seed=0):
    # every element distinct: (row, col) is readable from the value
    return torch.arange(N * K, dtype=torch.float64).view(N, K) + seed


@pytest.mark.parametrize("swiglu", [False, True], ids=["identity", "swiglu"])
@pytest.mark.parametrize("N,K", [(64, 32), (64, 256), (192, 1024), (512, 96)])
def test_pack_unpack_roundtrip(N, K, swiglu):
    w = _w(N, K)
    wp = ref.pack_skinny_w(w, swiglu)
    assert tuple(wp.shape) == (N // 16, K // 32, 4, 16, 8) and wp.is_contiguous()
    assert torch.equal(ref.unpack_skinny_w(wp, swiglu), w)
    assert torch.equal(ops.pack_skinny_w(w, swiglu), wp)
    # the layout as the issue states it, element by element
    rows = ref.skinny_rowmap(N, swiglu)
    for g, kb, hi, li, e in [(0, 0, 0, 0, 0), (N // 16 - 1, K // 32 - 1, 3, 15, 7),
                             (1, 0, 2, 7, 3), (2, K // 32 - 1, 1, 8, 5)]:
        assert wp[g, kb, hi, li, e] == w[rows[g * 16 + li], kb * 32 + hi * 8 + e]
    assert sorted(rows.tolist()) == list(range(N))


def _split_k_chunks(K, ksplit):
    """ext.hip split_k_chunks at the v2 kernel's 256-element unit."""
    nch = K // 256
    per = -(-nch // ksplit)
    return -(-nch // per), per * 256


@pytest.mark.parametrize("swiglu", [False, True], ids=["identity", "swiglu"])
@pytest.mark.parametrize("N,K,ksplit", [(64, 256, 1), (128, 512, 1),
                                        (192, 1024, 2), (64, 2048, 4),
                                        (256, 768, 2)])
def test_lane_addressing(N, K, ksplit, swiglu):
    """Row-major: lane (li, hi) of wave `wave` of tile `tile` reads 8 elements
    at wrow + k + u*32 + hi*8, wrow = W + (n0 + li)*K with n0 = tile*64 +
    wave*16, or for the SwiGLU kernel W + ((li < 8 ? 0 : N/2 - 8) + tile*32 +
    wave*8 + li)*K. Packed: W + skinny_packed_offset(tile*4 + wave, 0, K) +
    lane*8 + (k/32 + u)*512."""
    w = _w(N, K, seed=3)
    flat = w.reshape(-1)
    pflat = ref.pack_skinny_w(w, swiglu).reshape(-1)
    ntiles = N // 64
    ks, kchunk = _split_k_chunks(K, ksplit)
    e = torch.arange(8)
    seen = 0
    for split in range(ks):
        k0, k1 = split * kchunk, min(K, (split + 1) * kchunk)
        assert (k1 - k0) % 256 == 0
        tile, wave, lane, k, u = torch.meshgrid(
            torch.arange(ntiles), torch.arange(4), torch.arange(64),
            torch.arange(k0, k1, 128), torch.arange(4), indexing="ij")
        li, hi = lane & 15, lane >> 4
        if swiglu:
            row = torch.where(li < 8, 0, N // 2 - 8) + tile * 32 + wave * 8 + li
        else:
            row = tile * 64 + wave * 16 + li
        rowmajor = row * K + k + u * 32 + hi * 8
        packed = (((tile * 4 + wave) * (K // 32)) * 512 + lane * 8
                  + (k // 32 + u) * 512)
        assert int(packed.max()) + 8 <= N * K      # stays inside the copy
        assert torch.equal(pflat[packed[..., None] + e], flat[rowmajor[..., None] + e])
        seen += packed.numel() * 8
    assert seen == N * K                           # every element, once


# ---------------------------------------------------------------------------
# the block's cache
# ---------------------------------------------------------------------------

def _block():
    from bloombee_amd.models.base import ModelConfig
    from bloombee_amd.models.llama.block import LlamaBlock

    cfg = ModelConfig(hidden_size=256, num_hidden_layers=1, num_attention_heads=2,
                      num_key_value_heads=1, head_dim=128, intermediate_size=256,
                      max_position_embeddings=64)
    blk = LlamaBlock(cfg, 0).init_random(5)
    with torch.no_grad():   # non-unit norm weights: the fold changes qkv / gate_up
        blk.input_norm_w.copy_(torch.linspace(0.5, 2.0, 256).to(blk.input_norm_w.dtype))
        blk.post_norm_w.copy_(torch.linspace(2.0, 0.5, 256).to(blk.post_norm_w.dtype))
    return blk


NAMES = (("qkv_w", False), ("o_w", False), ("gate_up_w", True), ("down_w", False))


def _fresh(blk):
    """every cached copy is the pack of the weight as it is now"""
    for name, sw in NAMES:
        wp = blk._packed(name, sw)
        assert wp is not None
        assert torch.equal(wp, ref.pack_skinny_w(getattr(blk, name).detach(), sw)), name
        assert blk._packed(name, sw) is wp, f"{name}: rebuilt without a change"
    return {name: blk._packed(name, sw) for name, sw in NAMES}


def test_block_cache_invalidation(monkeypatch):
    monkeypatch.setenv("BBAMD_PACK_W", "1")
    blk = _block()
    first = _fresh(blk)

    before = blk.qkv_w.detach().clone()
    blk.fold_norm_weights()
    assert blk._wpacked == {}
    assert not torch.equal(blk.qkv_w, before)
    folded = _fresh(blk)
    assert not torch.equal(folded["qkv_w"], first["qkv_w"])
    assert not torch.equal(folded["gate_up_w"], first["gate_up_w"])

    blk.unfold_norm_weights()
    assert blk._wpacked == {}
    _fresh(blk)

    # an in-place write bumps _version: the copy is rebuilt, the others kept
    kept = blk._packed("down_w")
    old = blk._packed("o_w")
    with torch.no_grad():
        blk.o_w.mul_(2)
    new = blk._packed("o_w")
    assert new is not old and torch.equal(new, ref.pack_skinny_w(blk.o_w.detach()))
    assert blk._packed("down_w") is kept

    # load_state_dict writes in place as well
    sd = {k: v.clone() for k, v in blk.state_dict().items()}
    sd["down_w"] = sd["down_w"] * 0.5
    blk.load_state_dict(sd)
    assert blk._packed("down_w") is not kept
    _fresh(blk)

    # a reassigned tensor (what a move to another device does)
    old = blk._packed("qkv_w")
    blk.qkv_w.data = blk.qkv_w.data.clone() + 1
    assert blk._packed("qkv_w") is not old
    _fresh(blk)

    blk.quantize_weights_q4(keep_full=True)
    assert blk._wpacked == {}


def test_block_cache_modes(monkeypatch):
    blk = _block()
    monkeypatch.setenv("BBAMD_PACK_W", "1")
    assert blk._packed("o_w") is not None
    monkeypatch.setenv("BBAMD_PACK_W", "0")
    assert blk._packed("o_w") is None and blk._wpacked == {}
    # auto packs measured shapes on a device with memory to spare: never on CPU
    monkeypatch.setenv("BBAMD_PACK_W", "auto")
    assert all(blk._packed(n, sw) is None for n, sw in NAMES)


def test_linear_ignores_packed_off_the_skinny_path():
    """CPU / prefill shapes take F.linear and read w, whatever w_packed is."""
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(3, 256, generator=gen)
    w = torch.randn(64, 256, generator=gen)
    junk = torch.zeros_like(ref.pack_skinny_w(w))
    assert torch.equal(ops.linear(x, w, w_packed=junk), ops.linear(x, w))
    gu = torch.randn(128, 256, generator=gen)
    assert torch.equal(
        ops.linear_swiglu(x, gu, w_packed=torch.zeros_like(ref.pack_skinny_w(gu, True))),
        ops.linear_swiglu(x, gu))
