"""Mixtral with 4-bit weights, from the block up to the CLI, on the CPU.

On the CPU a quantized block dequantizes what it multiplies by, so its
output must equal, bit for bit, that of a twin block whose bf16 weights were
overwritten with the dequantized values: the comparisons here are all
`torch.equal`.
"""
import sys

import pytest
import torch

from bloombee_amd import ops
from bloombee_amd.engine import BlockStack, LocalEngine
from bloombee_amd.models.base import resolve_config
from bloombee_amd.ops import reference as ref

W_NAMES = ("qkv_w", "o_w", "expert_gate_up_w", "expert_down_w")


def _dequantized(w):
    packed, scale, zero = ref.quant4_pack(w)
    return ref.quant4_unpack(packed, scale, zero, w.dtype).reshape(w.shape)


def _overwrite_with_dequantized(blocks, names=W_NAMES):
    with torch.no_grad():
        for blk in blocks:
            for name in names:
                w = getattr(blk, name)
                w.copy_(_dequantized(w.detach()))


def _steps(stack, hidden_steps):
    kv_pool = stack.make_kv(1 << 12)
    B = hidden_steps[0].shape[0]
    kv = kv_pool.allocate(B, 64)
    outs, pos = [], 0
    for h in hidden_steps:
        start = torch.full((B,), pos, dtype=torch.int32)
        kv.extend(h.shape[1])
        outs.append(stack.forward_inference(h.clone(), kv, start))
        pos += h.shape[1]
    kv.close()
    return outs


def test_quantized_block_equals_dequantized_twin():
    cfg = resolve_config("mixtral-tiny")
    quant = BlockStack(cfg, 0, 1, device="cpu", seed=5)
    twin = BlockStack(cfg, 0, 1, device="cpu", seed=5)
    _overwrite_with_dequantized(twin.blocks)
    assert quant.blocks[0].quantize_weights_q4() is quant.blocks[0]
    gen = torch.Generator().manual_seed(1)
    hs = [(torch.randn(2, T, cfg.hidden_size, generator=gen) * 0.5).to(cfg.dtype)
          for T in (10, 1, 1, 1)]
    for got, want in zip(_steps(quant, hs), _steps(twin, hs)):
        assert torch.equal(got, want)
    # the quantization is not a no-op: the original weights give another result
    plain = BlockStack(cfg, 0, 1, device="cpu", seed=5)
    assert not torch.equal(_steps(plain, hs)[0], _steps(twin, hs)[0])


@pytest.mark.parametrize("keep_full", [False, True])
def test_weight_bytes(keep_full):
    cfg = resolve_config("mixtral-tiny")
    blk = BlockStack(cfg, 0, 1, device="cpu", seed=5).blocks[0]
    shapes = {n: tuple(getattr(blk, n).shape) for n in W_NAMES}
    router = blk.router_w.clone()
    blk.quantize_weights_q4(keep_full=keep_full)
    assert set(blk._w4) == set(W_NAMES)
    for name, shape in shapes.items():
        packed, scale, zero, N = blk._w4[name]
        K, mats = shape[-1], (shape[0] if len(shape) == 3 else 1)
        assert N == shape[-2]
        assert packed.dtype == torch.uint8 and packed.shape == shape[:-1] + (K // 2,)
        assert scale.dtype == zero.dtype == torch.float16
        assert scale.shape == zero.shape == shape[:-1] + (K // 64,)
        nbytes = sum(t.numel() * t.element_size() for t in (packed, scale, zero))
        assert nbytes == mats * (N * K // 2 + 4 * N * K // 64)
        assert getattr(blk, name).numel() == (mats * N * K if keep_full else 0)
    # the router and the norms stay bf16 and untouched
    assert torch.equal(blk.router_w, router) and blk.router_w.dtype == cfg.dtype
    assert blk.input_norm_w.numel() == blk.post_norm_w.numel() == cfg.hidden_size


def test_forward_train_without_full_weights_raises():
    cfg = resolve_config("mixtral-tiny")
    blk = BlockStack(cfg, 0, 1, device="cpu", seed=5).blocks[0]
    h = torch.zeros(1, 4, cfg.hidden_size, dtype=cfg.dtype)
    blk.forward_train(h)
    blk.quantize_weights_q4(keep_full=True)
    blk.forward_train(h)
    blk.quantize_weights_q4()
    with pytest.raises(RuntimeError, match="quantize_weights_q4"):
        blk.forward_train(h)


def test_loop_dequantizes_only_visited_experts(monkeypatch):
    cfg = resolve_config("mixtral-tiny")
    blk = BlockStack(cfg, 0, 1, device="cpu", seed=5).blocks[0]
    blk.quantize_weights_q4()
    y = (torch.randn(1, 1, cfg.hidden_size,
                     generator=torch.Generator().manual_seed(2)) * 0.5).to(cfg.dtype)
    seen = []
    real = blk._expert_w
    monkeypatch.setattr(blk, "_expert_w",
                        lambda name, le, dt: seen.append((name, le)) or real(name, le, dt))
    blk._moe(y)
    routed = ops.linear(y.reshape(1, -1), blk.router_w).float().topk(blk.topk).indices
    assert sorted(seen) == sorted((n, int(e)) for e in routed[0]
                                  for n in ("expert_gate_up_w", "expert_down_w"))


@pytest.fixture(scope="module")
def quantized_engine_tokens():
    eng = LocalEngine("mixtral-tiny", device="cpu", seed=0, kv_max_tokens=1 << 14,
                      quantize_q4=True)
    assert all(set(getattr(b, "_w4", {})) == set(W_NAMES) for b in eng.stack.blocks)
    prompt = torch.randint(0, 900, (2, 6), generator=torch.Generator().manual_seed(9))
    return prompt, eng.generate_greedy(prompt, 4)


def test_local_engine_quantizes_mixtral(quantized_engine_tokens):
    prompt, got = quantized_engine_tokens
    twin = LocalEngine("mixtral-tiny", device="cpu", seed=0, kv_max_tokens=1 << 14)
    _overwrite_with_dequantized(twin.stack.blocks)
    assert torch.equal(got, twin.generate_greedy(prompt, 4))


@pytest.mark.parametrize("model,names", [
    ("mixtral-tiny", W_NAMES),
    ("llama-tiny", ("qkv_w", "o_w", "gate_up_w", "down_w"))])
def test_backend_and_server_quantize_every_block(model, names):
    from bloombee_amd.net.dht import Dht
    from bloombee_amd.server import Server
    from bloombee_amd.server.backend import StackBackend

    cfg = resolve_config(model)
    be = StackBackend(cfg, 0, 2, device="cpu", seed=0, kv_max_tokens=1 << 12,
                      quantize_q4=True)
    assert len(be.stack.blocks) == 2
    assert all(set(b._w4) == set(names) for b in be.stack.blocks)
    plain = StackBackend(cfg, 0, 2, device="cpu", seed=0, kv_max_tokens=1 << 12)
    assert all(getattr(b, "_w4", None) is None for b in plain.stack.blocks)

    boot = Dht()
    srv = Server(model, initial_peers=[boot.endpoint], block_indices=(0, 2),
                 device="cpu", seed=0, kv_max_tokens=1 << 12, quantize_q4=True)
    try:
        assert srv._backend_kw["quantize_q4"] is True      # re-hosts keep it
        assert all(set(b._w4) == set(names) for b in srv.backend.stack.blocks)
    finally:
        srv.shutdown()
        boot.shutdown()


def test_backend_refuses_what_it_cannot_quantize():
    from bloombee_amd.offload import OffloadPolicy
    from bloombee_amd.server.backend import StackBackend

    with pytest.raises(ValueError, match="no 4-bit compute path"):
        StackBackend(resolve_config("bloom-tiny"), 0, 1, device="cpu",
                     kv_max_tokens=1 << 12, quantize_q4=True)
    policy = OffloadPolicy(weight_gpu_percent=50.0)
    assert policy.offloads_weights
    with pytest.raises(ValueError, match="weight offload"):
        StackBackend(resolve_config("mixtral-tiny"), 0, 2, device="cpu",
                     kv_max_tokens=1 << 12, offload_policy=policy,
                     quantize_q4=True)


def test_quantized_swarm_matches_quantized_engine(quantized_engine_tokens):
    from bloombee_amd.client import ClientConfig
    from bloombee_amd.models.auto import AutoDistributedModelForCausalLM
    from bloombee_amd.net.dht import Dht
    from bloombee_amd.server import Server

    prompt, expect = quantized_engine_tokens
    n_layers = resolve_config("mixtral-tiny").num_hidden_layers
    half = n_layers // 2
    boot = Dht()
    servers = [Server("mixtral-tiny", initial_peers=[boot.endpoint],
                      block_indices=rng, device="cpu", seed=0,
                      kv_max_tokens=1 << 14, update_period=5.0, quantize_q4=True)
               for rng in ((0, half), (half, n_layers))]
    for s in servers:
        s.run_in_background()
    try:
        model = AutoDistributedModelForCausalLM.from_pretrained(
            "mixtral-tiny", client_config=ClientConfig(initial_peers=[boot.endpoint]),
            seed=0)
        out = model.generate(prompt, max_new_tokens=4)
        assert torch.equal(out[:, prompt.shape[1]:], expect)
        model.remote.manager.shutdown()
    finally:
        for s in servers:
            s.shutdown()
        boot.shutdown()


def test_cli_quant_type_w4_reaches_server(monkeypatch):
    from bloombee_amd.cli import run_server

    calls = []

    class FakeServer:
        def __init__(self, model, **kw):
            calls.append((model, kw))

        def run(self):
            pass

    monkeypatch.setattr(run_server, "Server", FakeServer)
    base = ["run_server", "mixtral-tiny", "--device", "cpu", "--throughput", "1.0",
            "--block-indices", "0:2"]
    for extra, want_q4, want_policy in ((["--quant-type", "w4"], True, False),
                                        (["--quant-type", "nf4"], False, True),
                                        ([], False, False)):
        monkeypatch.setattr(sys, "argv", base + extra)
        run_server.main()
        model, kw = calls[-1]
        assert model == "mixtral-tiny"
        assert kw["quantize_q4"] is want_q4
        assert (kw["offload_policy"] is not None) == want_policy
    monkeypatch.setattr(sys, "argv", base + ["--quant-type", "int8"])
    with pytest.raises(SystemExit):
        run_server.main()
