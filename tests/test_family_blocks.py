"""What the family blocks share (models/block_common.py): every family takes
tree_mask, and Qwen3 is the LLaMA block plus a live hook. CPU only."""
import pytest
import torch

from bloombee_amd.engine import BlockStack
from bloombee_amd.models.base import resolve_config

B, PRE, NEW = 2, 5, 4


def _verify_step(model, tree_mask):
    """Prefill PRE tokens, then NEW more in one step; returns that step's
    hidden states."""
    cfg = resolve_config(model)
    stack = BlockStack(cfg, 0, cfg.num_hidden_layers, device="cpu", seed=3)
    gen = torch.Generator().manual_seed(5)
    x_pre = (torch.randn(B, PRE, cfg.hidden_size, generator=gen) * 0.3).to(cfg.dtype)
    x_new = (torch.randn(B, NEW, cfg.hidden_size, generator=gen) * 0.3).to(cfg.dtype)
    kv = stack.make_kv(1024).allocate(B, 32)
    try:
        kv.extend(PRE)
        stack.forward_inference(x_pre, kv, torch.zeros(B, dtype=torch.int32))
        kv.extend(NEW)
        return stack.forward_inference(
            x_new, kv, torch.full((B,), PRE, dtype=torch.int32),
            tree_mask=tree_mask)
    finally:
        kv.close()


def _causal_mask():
    return torch.tril(torch.ones(NEW, NEW, dtype=torch.bool)).expand(
        B, NEW, NEW).contiguous()


@pytest.mark.parametrize("model", ["llama-tiny", "qwen3-tiny", "mixtral-tiny",
                                   "falcon-tiny"])
def test_causal_tree_mask_equals_plain_prefill(model):
    """A lower-triangular tree mask is plain causal attention: the verify
    step returns the bits of the same tokens run without a mask."""
    plain = _verify_step(model, None)
    masked = _verify_step(model, _causal_mask())
    assert torch.equal(masked, plain)


@pytest.mark.parametrize("model", ["bloom-tiny", "gemma4-tiny"])
def test_tree_mask_unsupported_families_say_so(model):
    with pytest.raises(NotImplementedError, match=model.split("-")[0]):
        _verify_step(model, _causal_mask())


def test_qwen3_is_llama_plus_live_hook():
    """Qwen3Block has no forward_inference / forward_train of its own, and
    its per-head q/k norm weights reach the output through the hooks."""
    from bloombee_amd.models.llama.block import LlamaBlock
    from bloombee_amd.models.qwen3.block import Qwen3Block

    assert Qwen3Block.forward_inference is LlamaBlock.forward_inference
    assert Qwen3Block.forward_train is LlamaBlock.forward_train

    cfg = resolve_config("qwen3-tiny")
    gen = torch.Generator().manual_seed(9)
    x = (torch.randn(B, PRE, cfg.hidden_size, generator=gen) * 0.3).to(cfg.dtype)
    qn = (1 + 0.3 * torch.randn(cfg.head_dim, generator=gen)).to(cfg.dtype)
    kn = (1 + 0.3 * torch.randn(cfg.head_dim, generator=gen)).to(cfg.dtype)

    def run(unit):
        stack = BlockStack(cfg, 0, 1, device="cpu", seed=3)
        blk = stack.blocks[0]
        assert isinstance(blk, Qwen3Block)
        assert bool((blk.q_norm_w == 1).all()) and bool((blk.k_norm_w == 1).all())
        if not unit:
            blk.q_norm_w.data.copy_(qn)
            blk.k_norm_w.data.copy_(kn)
        kv = stack.make_kv(1024).allocate(B, 32)
        try:
            kv.extend(PRE)
            served = stack.forward_inference(
                x.clone(), kv, torch.zeros(B, dtype=torch.int32))
        finally:
            kv.close()
        return served, stack.forward_train(x.clone())

    served_unit, train_unit = run(True)
    served_rand, train_rand = run(False)
    assert not torch.equal(served_unit, served_rand)
    assert not torch.equal(train_unit, train_rand)
