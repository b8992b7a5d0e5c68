"""The fp8 (e4m3) weight tier without a GPU: the quantiser's rule, the tiled
layout's round trip, quantized llama / qwen3 blocks on the reference path and
the refusals of the public switches."""
import pytest
import torch

from bloombee_amd import ops
from bloombee_amd.engine import BlockStack, LocalEngine
from bloombee_amd.models.base import resolve_config
from bloombee_amd.ops import reference as ref

FP8 = torch.float8_e4m3fn
NAMES = ("qkv_w", "o_w", "gate_up_w", "down_w")


def test_quant_w8_rule():
    w = (torch.randn(48, 256, generator=torch.Generator().manual_seed(0))
         * torch.logspace(-6, 4, 48).unsqueeze(1)).to(torch.bfloat16)
    w[5] = 0
    w[6, 3] = 448.0          # amax exactly at the bound: scale 1
    w[7, 3] = 450.0          # just above: scale 2
    codes, w_scale = ops.quant_w8(w)
    assert codes.dtype == FP8 and w_scale.dtype == torch.float32
    m, _ = torch.frexp(w_scale)
    assert torch.all(m == 0.5)                              # powers of two
    assert w_scale[5] == 1 and torch.all(codes[5].float() == 0)
    amax = w.float().abs().amax(1)
    live = amax > 0
    assert torch.all(amax <= 448 * w_scale)
    assert torch.all((amax > 448 * w_scale / 2)[live])      # the smallest such
    # independent rounding: scale in f64, round through torch's e4m3
    want = (w.double() / w_scale.double().unsqueeze(1)).float().to(FP8).float()
    assert torch.equal(codes.float() * w_scale.unsqueeze(1),
                       want * w_scale.unsqueeze(1))


def test_pack_w8_round_trip_and_offset_rule():
    codes = torch.randint(0, 255, (64, 384), dtype=torch.uint8).view(FP8)
    packed = ops.pack_w8(codes)
    assert torch.equal(ops.unpack_w8(packed).view(torch.uint8), codes.view(torch.uint8))
    # common.h: tile (g, kb) at ((g * K/128) + kb) * 2048; lane q*16 + li owns
    # the 16 bytes at h*1024 + lane*16
    flat, g, kb, h, q, li = packed.view(torch.uint8).flatten(), 3, 2, 1, 2, 5
    at = (g * 3 + kb) * 2048 + h * 1024 + (q * 16 + li) * 16
    k = kb * 128 + q * 32 + h * 16
    assert torch.equal(flat[at:at + 16], codes.view(torch.uint8)[g * 16 + li, k:k + 16])


@pytest.mark.skipif(not ops.HAVE_HIP_OPS, reason="HIP extension not built")
def test_bindings_plan_and_cpu_tensor_rejection():
    plan = ops.hip_w8.gemm_w8_plan
    assert plan(64, 384, 1) == (1, 384) and plan(64, 384, 2) == (2, 256)
    assert plan(28672, 4096, 0) == (1, 4096) and plan(4096, 14336, 0) == (4, 3584)
    for bad in ((64, 192), (96, 256)):
        with pytest.raises(RuntimeError, match="K%128, N%64"):
            plan(*bad, 0)
    codes, w_scale = ops.quant_w8(torch.randn(64, 128).to(torch.bfloat16))
    x = torch.randn(2, 128).to(torch.bfloat16)
    a8, a_scale = ref.quant_rows_fp8(x)
    with pytest.raises(RuntimeError, match="must be on device"):
        ops.hip_w8.quant_rows_fp8(x)
    with pytest.raises(RuntimeError, match="must be on device"):
        ops.hip_w8.gemm_w8(a8, a_scale, ops.pack_w8(codes), w_scale, None, None, 64)


@pytest.mark.parametrize("model,seed", [("llama-tiny", 5), ("qwen3-tiny", 7)])
def test_block_quantized_fp8(model, seed):
    cfg = resolve_config(model)
    full = BlockStack(cfg, 0, 1, device="cpu", seed=seed)
    quant = BlockStack(cfg, 0, 1, device="cpu", seed=seed)
    blk = quant.blocks[0]
    assert blk.quantize_weights_fp8() is blk and set(blk._w8) == set(NAMES)
    assert all(getattr(blk, n).numel() == 0 for n in NAMES)   # bf16 dropped
    hf_, hq_ = full.make_kv(1 << 10).allocate(2, 32), quant.make_kv(1 << 10).allocate(2, 32)
    x = (torch.randn(2, 4, cfg.hidden_size, generator=torch.Generator().manual_seed(1))
         * 0.1).to(cfg.dtype)
    sp = torch.zeros(2, dtype=torch.int32)
    hf_.extend(4)
    hq_.extend(4)
    yf = full.forward_inference(x.clone(), hf_, sp).float()
    yq = quant.forward_inference(x.clone(), hq_, sp).float()
    assert not torch.equal(yf, yq)                  # _lin took the fp8 weights
    assert (yf - yq).norm() / yf.norm() < 0.2       # test_reference_ops.py's W4 bound
    for again in (blk.quantize_weights_fp8, blk.quantize_weights_q4):
        with pytest.raises(RuntimeError, match="one weight tier"):
            again()


def test_switches_and_refusals(monkeypatch):
    import sys

    from bloombee_amd.cli import run_server
    from bloombee_amd.offload import OffloadPolicy
    from bloombee_amd.server.backend import StackBackend

    eng = LocalEngine("llama-tiny", device="cpu", seed=0, kv_max_tokens=1 << 12,
                      quantize_fp8=True)
    assert all(set(b._w8) == set(NAMES) for b in eng.stack.blocks)
    assert eng.generate_greedy(torch.randint(0, 900, (2, 5)), 3).shape == (2, 3)
    be = StackBackend(resolve_config("qwen3-tiny"), 0, 2, device="cpu",
                      kv_max_tokens=1 << 12, quantize_fp8=True)
    assert all(set(b._w8) == set(NAMES) for b in be.stack.blocks)
    for family in ("mixtral-tiny", "bloom-tiny", "falcon-tiny", "gemma4-tiny"):
        for make in (lambda c: StackBackend(c, 0, 1, device="cpu", kv_max_tokens=1 << 12,
                                            quantize_fp8=True),
                     lambda c: LocalEngine(c, device="cpu", kv_max_tokens=1 << 12,
                                           quantize_fp8=True)):
            with pytest.raises(ValueError, match="no fp8 weight path"):
                make(resolve_config(family))
    with pytest.raises(ValueError, match="weight offload"):
        StackBackend(resolve_config("llama-tiny"), 0, 2, device="cpu",
                     kv_max_tokens=1 << 12, quantize_fp8=True,
                     offload_policy=OffloadPolicy(weight_gpu_percent=50.0))
    with pytest.raises(ValueError, match="pick one"):
        StackBackend(resolve_config("llama-tiny"), 0, 1, device="cpu",
                     kv_max_tokens=1 << 12, quantize_fp8=True, quantize_q4=True)

    calls = []
    monkeypatch.setattr(run_server, "Server",
                        type("FakeServer", (), {"__init__": lambda s, m, **kw: calls.append(kw),
                                                "run": lambda s: None}))
    monkeypatch.setattr(sys, "argv", ["run_server", "llama-tiny", "--device", "cpu",
                                      "--throughput", "1.0", "--quant-type", "w8"])
    run_server.main()
    assert calls[-1]["quantize_fp8"] is True and calls[-1]["quantize_q4"] is False
