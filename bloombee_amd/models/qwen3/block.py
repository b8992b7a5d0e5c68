"""Server-side Qwen3 block (parity: reference models/qwen3/block.py
WrappedQwen3Block :18-181): the LLaMA block plus per-head RMS q/k norms
applied on the raw QKV GEMM output before RoPE, as LlamaBlock's _post_qkv /
_post_qkv_train hooks. head_dim is decoupled from hidden_size (Qwen3-8B:
D=128 with Hq*D != hidden)."""
from __future__ import annotations

from typing import Optional

import torch

from bloombee_amd import ops
from bloombee_amd.models.base import ModelConfig
from bloombee_amd.models.block_common import RopeTables, rms_train
from bloombee_amd.models.llama.block import LlamaBlock


class Qwen3Block(LlamaBlock):
    def __init__(self, config: ModelConfig, layer_index: int = 0,
                 rope: Optional[RopeTables] = None):
        super().__init__(config, layer_index, rope)
        self.q_norm_w = self.p(config.head_dim)
        self.k_norm_w = self.p(config.head_dim)

    def _post_qkv(self, qkv: torch.Tensor, B: int, T: int) -> torch.Tensor:
        # per-head q/k RMS norm on the fused buffer (contiguous D-sized rows),
        # in place. It acts on the GEMM OUTPUT, so the input-norm weight fold
        # of the fused-norm chain leaves it alone.
        Hq, Hkv, D = self.Hq, self.Hkv, self.D
        eps = self.config.rms_norm_eps
        q_flat = qkv[..., :Hq * D].reshape(-1, D)
        k_flat = qkv[..., Hq * D:(Hq + Hkv) * D].reshape(-1, D)
        qkv[..., :Hq * D] = ops.rms_norm(q_flat, self.q_norm_w,
                                         eps).view(B, T, Hq * D)
        qkv[..., Hq * D:(Hq + Hkv) * D] = ops.rms_norm(
            k_flat, self.k_norm_w, eps).view(B, T, Hkv * D)
        return qkv

    def _post_qkv_train(self, q: torch.Tensor, k: torch.Tensor):
        eps = self.config.rms_norm_eps
        return rms_train(q, self.q_norm_w, eps), rms_train(k, self.k_norm_w, eps)
