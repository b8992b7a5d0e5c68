"""Shared scenario for the mixed-device decode tests (CPU and GPU files).

A session prefills a 40-token prompt, optionally goes through
swap_out(); swap_in_as_prefix() (the committed KV becomes a host prefix),
then decodes 12 teacher-forced random tokens. The tests compare the block
stack's HIDDEN STATES between runs — greedy tokens cannot tell a broken
host-prefix branch from a correct one on random-init models (bloom-tiny and
falcon-tiny emit the same token at every step either way).
"""
import torch

FAMILIES = ["bloom-tiny", "falcon-tiny", "mixtral-tiny", "gemma4-tiny",
            "llama-tiny", "qwen3-tiny"]

BATCH, PROMPT, STEPS = 2, 40, 12


def copy_engine_weights(dst, src):
    """Make `dst` (any device) run the parameters of the CPU engine `src`:
    block init draws from a per-device generator, so same-seed engines on
    different devices do not share weights by themselves."""
    dev = dst.device
    dst.embed.copy_(src.embed.to(dev))
    dst.final_norm_w.copy_(src.final_norm_w.to(dev))
    if not src.config.tie_word_embeddings:
        dst.lm_head_w.copy_(src.lm_head_w.to(dev))
    for gb, cb in zip(dst.stack.blocks, src.stack.blocks):
        for (n1, pg), (n2, pc) in zip(gb.named_parameters(),
                                      cb.named_parameters()):
            assert n1 == n2
            pg.data.copy_(pc.data.to(dev))


def make_engine(model, device="cpu", weights_from=None):
    from bloombee_amd.engine import LocalEngine

    eng = LocalEngine(model, device=device, seed=11, kv_max_tokens=1 << 12)
    if weights_from is not None:
        copy_engine_weights(eng, weights_from)
    return eng


def decode_hidden(eng, swapped):
    """Run the scenario on `eng`; returns the decode steps' hidden states as
    fp32 CPU (STEPS, BATCH, H). Token ids stay below 500 (gemma4-tiny's
    vocabulary is 512)."""
    gen = torch.Generator().manual_seed(3)
    prompt = torch.randint(0, 500, (BATCH, PROMPT), generator=gen)
    feed = torch.randint(0, 500, (STEPS, BATCH), generator=gen)
    kv = eng.kv_pool.allocate(BATCH, 64)
    try:
        eng.prefill(prompt, kv)
        if swapped:
            kv.swap_out()
            kv.swap_in_as_prefix()
            assert kv.pos_offset == PROMPT and kv.lengths == [0] * BATCH
        outs = []
        for t in range(STEPS):
            start = torch.tensor([s.l_spec for s in kv.seqs],
                                 dtype=torch.int32, device=eng.device)
            kv.extend(1)
            hidden = eng._embed(feed[t].view(-1, 1))
            out = eng.stack.forward_inference(hidden, kv, start)
            outs.append(out[:, 0].float().cpu())
    finally:
        kv.close()
    return torch.stack(outs)
