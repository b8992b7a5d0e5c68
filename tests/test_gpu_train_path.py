"""The fine-tuning path on the GPU: every family's forward_train with the
training-attention kernels on and off against the same block in fp32 on the
CPU, the backend's forward/backward against autograd over the stack, and one
loopback-swarm prompt-tuning run with servers on the device.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 0
T = 48

if torch.cuda.is_available():
    from bloombee_amd.ops import interface


def _cfg(model_type, dtype, **d):
    from bloombee_amd.models.base import get_family
    return get_family(model_type).config_cls.from_dict(
        dict(d, model_type=model_type, torch_dtype=dtype))


# the registry's tiny presets where their head_dim is 64; local ones where it
# is 32 (falcon, bloom), so that every family reaches the kernels
FAMILIES = {
    "llama": dict(hidden_size=256, num_hidden_layers=1, num_attention_heads=4,
                  num_key_value_heads=2, intermediate_size=512, vocab_size=1024,
                  max_position_embeddings=2048, rope_theta=10000.0),
    "qwen3": dict(hidden_size=256, num_hidden_layers=1, num_attention_heads=4,
                  num_key_value_heads=2, head_dim=64, intermediate_size=512,
                  vocab_size=1024, rms_norm_eps=1e-6, max_position_embeddings=2048),
    "mixtral": dict(hidden_size=256, num_hidden_layers=1, num_attention_heads=4,
                    num_key_value_heads=2, intermediate_size=512, vocab_size=1024,
                    max_position_embeddings=2048, num_local_experts=4,
                    num_experts_per_tok=2),
    "falcon": dict(hidden_size=256, num_hidden_layers=1, num_attention_heads=4,
                   num_key_value_heads=1, head_dim=64, intermediate_size=1024,
                   vocab_size=1024, tie_word_embeddings=True,
                   max_position_embeddings=2048),
    "bloom": dict(hidden_size=512, num_hidden_layers=1, num_attention_heads=4,
                  intermediate_size=1024, vocab_size=1024,
                  tie_word_embeddings=True, max_position_embeddings=2048),
}
GEMMA4_D256 = dict(hidden_size=128, num_hidden_layers=1, num_attention_heads=2,
                   num_key_value_heads=1, head_dim=256, intermediate_size=256,
                   vocab_size=512, rms_norm_eps=1e-6, tie_word_embeddings=True,
                   max_position_embeddings=2048, sliding_window=8,
                   global_head_dim=256, sliding_window_pattern=6,
                   rope_theta=1000000.0, rope_local_base_freq=10000.0,
                   partial_rotary_factor_global=0.25,
                   hidden_size_per_layer_input=0)


class _Counter:
    def __init__(self, ext):
        self._ext = ext
        self.fwd = self.bwd = 0

    def attn_train_fwd(self, *a):
        self.fwd += 1
        return self._ext.attn_train_fwd(*a)

    def attn_train_bwd(self, *a):
        self.bwd += 1
        return self._ext.attn_train_bwd(*a)

    def __getattr__(self, name):
        return getattr(self._ext, name)


def _stacks(model_type, d):
    """The same one-block stack in bf16 on the device and in fp32 on the CPU
    (the CPU copy takes the device block's bf16 weights, upcast)."""
    from bloombee_amd.engine import BlockStack
    gpu = BlockStack(_cfg(model_type, "bfloat16", **d), 0, 1, device=DEV, seed=SEED)
    cpu = BlockStack(_cfg(model_type, "float32", **d), 0, 1, device="cpu", seed=SEED)
    with torch.no_grad():
        src = dict(gpu.named_parameters())
        for name, p in cpu.named_parameters():
            p.copy_(src[name].float().cpu())
    return gpu, cpu


def _fwd_bwd(stack, x, go):
    x = x.detach().clone().requires_grad_(True)
    y = stack.forward_train(x)
    (g,) = torch.autograd.grad(y, x, go)
    return y.detach().float().cpu(), g.float().cpu()


def _inputs(hidden):
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(2, T, hidden, generator=gen).to(torch.bfloat16)
    go = torch.randn(2, T, hidden, generator=gen).to(torch.bfloat16)
    return x, go


@pytest.mark.parametrize("family", list(FAMILIES))
def test_family_block_kernel_vs_eager_vs_fp32(family, monkeypatch):
    """forward_train output and input gradient: kernels on, kernels off, and
    the fp32 CPU block as truth. A whole block's error is not derivable, so
    the bound is relative: the kernel path may be at most 2x as far from truth
    as the eager bf16 path (two fp32-accumulating implementations of the same
    math that place their bf16 roundings differently)."""
    counter = _Counter(interface.hip_ops)
    monkeypatch.setattr(interface, "hip_ops", counter)
    gpu, cpu = _stacks(family, FAMILIES[family])
    x, go = _inputs(FAMILIES[family]["hidden_size"])

    monkeypatch.delenv("BBAMD_TRAIN_ATTN_KERNEL", raising=False)
    y_k, g_k = _fwd_bwd(gpu, x.to(DEV), go.to(DEV))
    assert (counter.fwd, counter.bwd) == (1, 1), "the kernel binding was not called"
    monkeypatch.setenv("BBAMD_TRAIN_ATTN_KERNEL", "0")
    y_e, g_e = _fwd_bwd(gpu, x.to(DEV), go.to(DEV))
    assert (counter.fwd, counter.bwd) == (1, 1)
    y_t, g_t = _fwd_bwd(cpu, x.float(), go.float())

    assert bool(torch.isfinite(y_k).all()) and bool(torch.isfinite(g_k).all())
    err = lambda a, b: float((a - b).abs().max())
    ek, ee = err(y_k, y_t), err(y_e, y_t)
    gk, ge = err(g_k, g_t), err(g_e, g_t)
    print(f"[train-path] {family}: out err kernel {ek:.4g} eager {ee:.4g} "
          f"(max|y| {float(y_t.abs().max()):.3g}); grad err kernel {gk:.4g} "
          f"eager {ge:.4g} (max|g| {float(g_t.abs().max()):.3g})")
    assert ek <= 2 * ee, (family, "output", ek, ee)
    assert gk <= 2 * ge, (family, "grad", gk, ge)


def test_gemma4_d256_runs_on_gpu_through_the_composition(monkeypatch):
    """D = 256 has no training kernel: forward_train must run on the device
    through the torch composition, and be as close to the fp32 CPU block as
    that composition is by its own nature: its error against truth may be at
    most 2x the error of the same bf16 composition run on the CPU (the same
    relative bound as the family test, with the CPU run as the eager path)."""
    from bloombee_amd.engine import BlockStack
    counter = _Counter(interface.hip_ops)
    monkeypatch.setattr(interface, "hip_ops", counter)
    monkeypatch.delenv("BBAMD_TRAIN_ATTN_KERNEL", raising=False)
    gpu, cpu = _stacks("gemma4", GEMMA4_D256)
    assert gpu.blocks[0].D == 256
    eager = BlockStack(_cfg("gemma4", "bfloat16", **GEMMA4_D256), 0, 1,
                       device="cpu", seed=SEED)
    with torch.no_grad():
        src = dict(gpu.named_parameters())
        for name, p in eager.named_parameters():
            p.copy_(src[name].cpu())
    x, go = _inputs(GEMMA4_D256["hidden_size"])
    y, g = _fwd_bwd(gpu, x.to(DEV), go.to(DEV))
    assert (counter.fwd, counter.bwd) == (0, 0)
    y_e, g_e = _fwd_bwd(eager, x, go)
    y_t, g_t = _fwd_bwd(cpu, x.float(), go.float())
    err = lambda a, b: float((a - b).abs().max())
    print(f"[train-path] gemma4 D256: out err gpu {err(y, y_t):.4g} cpu-bf16 "
          f"{err(y_e, y_t):.4g}; grad err gpu {err(g, g_t):.4g} cpu-bf16 "
          f"{err(g_e, g_t):.4g}")
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(g).all())
    assert err(y, y_t) <= 2 * err(y_e, y_t)
    assert err(g, g_t) <= 2 * err(g_e, g_t)


def test_backend_forward_backward_match_autograd_on_gpu():
    """StackBackend.forward + backward with deep prompts on cuda:0 return what
    torch.autograd.grad over stack.forward_train gives on the same device.
    Both run the same deterministic kernels: exact equality, as the CPU
    counterpart in test_swarm.py asserts."""
    from bloombee_amd.models.base import resolve_config
    from bloombee_amd.server.backend import StackBackend

    cfg = resolve_config("llama-mini-gpu")
    be = StackBackend(cfg, 0, 2, device=DEV, seed=SEED, kv_max_tokens=1 << 12)
    try:
        gen = torch.Generator().manual_seed(23)
        h = (torch.randn(2, T, cfg.hidden_size, generator=gen) * 0.5).to(cfg.dtype)
        prompts = (torch.randn(2, 4, cfg.hidden_size, generator=gen) * 0.1).to(cfg.dtype)
        go = torch.randn(2, T, cfg.hidden_size, generator=gen).to(cfg.dtype)

        out = be.forward(h, prompts=prompts)
        gh, gp = be.backward(h, go, prompts=prompts)

        hd = h.to(DEV).detach().requires_grad_(True)
        pd = prompts.to(DEV).detach().requires_grad_(True)
        ref = be.stack.forward_train(hd, deep_prompts=pd)
        rh, rp = torch.autograd.grad(ref, (hd, pd), go.to(DEV))
        assert out.is_cuda and gh.is_cuda and gp.is_cuda
        assert torch.equal(out, ref.detach())
        assert torch.equal(gh, rh) and torch.equal(gp, rp)
        assert float(gp.float().abs().sum()) > 0
    finally:
        be.shutdown()


@pytest.mark.timeout(600)
def test_gpu_swarm_deep_ptune_reduces_loss():
    """Deep prompt tuning over a loopback swarm whose two servers hold one
    block each on cuda:0 (the client, with its trainable prompts, stays on the
    CPU as a remote user's would): a few optimizer steps reduce the loss."""
    from bloombee_amd.client import ClientConfig
    from bloombee_amd.net.dht import Dht
    from bloombee_amd.server import Server

    from bloombee_amd.models.base import get_family, resolve_config

    model_name = "llama-tiny-2blocks"
    mcfg = resolve_config("llama-tiny")
    mcfg.num_hidden_layers = 2
    boot = Dht()
    servers = []
    try:
        for rng in [(0, 1), (1, 2)]:
            s = Server(mcfg, model_name=model_name,
                       initial_peers=[boot.endpoint], block_indices=rng, device=DEV, seed=SEED,
                       kv_max_tokens=1 << 12, update_period=2.0)
            s.run_in_background()
            servers.append(s)
        model = get_family("llama").causal_lm_cls.from_pretrained(
            model_name, config=mcfg,
            client_config=ClientConfig(initial_peers=[boot.endpoint]),
            seed=SEED, device="cpu", pre_seq_len=4, deep_ptune=True)
        params = model.trainable_parameters()
        assert len(params) == 2
        opt = torch.optim.Adam(params, lr=5e-2)
        gen = torch.Generator().manual_seed(31)
        ids = torch.randint(0, 1000, (1, 6), generator=gen)
        target = torch.randint(0, 1000, (1, 10), generator=gen)
        losses = []
        for _ in range(4):
            logits = model(ids)
            loss = torch.nn.functional.cross_entropy(
                logits.float().view(-1, logits.shape[-1]), target.view(-1))
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        print(f"[train-path] swarm losses {losses}")
        assert all(l == l for l in losses)
        assert losses[-1] < losses[0], losses
        assert all(s.backend.device.type == "cuda" for s in servers)
        model.remote.manager.shutdown()
    finally:
        for s in servers:
            s.shutdown()
        boot.shutdown()
