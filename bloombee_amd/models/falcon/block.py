"""Server-side Falcon block (parity: reference models/falcon/block.py
WrappedFalconBlock :399-503 — falcon-7b architecture: single input LayerNorm,
parallel attention + MLP branches, rotary MQA (num_kv_heads=1), no biases).

MQA note: GQA group size Hq/Hkv = 71 exceeds the decode kernel's 16-row MFMA
q-tile, so the GPU path reshapes queries into ceil(G/16) fake groups sharing
the one KV head at the interface level (CPU reference handles any G)."""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F

from bloombee_amd import ops
from bloombee_amd.kv.paged import SessionHandle
from bloombee_amd.models.base import ModelConfig
from bloombee_amd.models.block_common import (
    FamilyBlock, RopeTables, paged_attention_qkv, rope_attn_train,
    rotary_positions, split_heads)


class FalconBlock(FamilyBlock):
    def __init__(self, config: ModelConfig, layer_index: int = 0,
                 rope: Optional[RopeTables] = None):
        super().__init__(config, layer_index)
        H = config.hidden_size
        D = config.head_dim
        Hq, Hkv = config.num_attention_heads, config.num_key_value_heads
        I = config.intermediate_size
        self.Hq, self.Hkv, self.D, self.I = Hq, Hkv, D, I
        self.scale = 1.0 / math.sqrt(D)
        self.rope = rope if rope is not None else RopeTables(config)
        p = self.p
        self.ln_w, self.ln_b = p(H), p(H)
        self.qkv_w = p((Hq + 2 * Hkv) * D, H)
        self.o_w = p(H, Hq * D)
        self.up_w = p(I, H)
        self.down_w = p(H, I)

    @torch.no_grad()
    def forward_inference(self, hidden: torch.Tensor, kv: SessionHandle,
                          start_pos: torch.Tensor, position_ids=None,
                          tree_mask=None) -> torch.Tensor:
        B, T, H = hidden.shape
        Hq, Hkv = self.Hq, self.Hkv
        cfg = self.config
        x = ops.layer_norm(hidden, self.ln_w, self.ln_b, cfg.layer_norm_epsilon)
        qkv = ops.linear(x, self.qkv_w)
        cos, sin = self.rope.get(hidden.device)
        ops.rope_kv_write_(qkv, Hq, Hkv, cos, sin,
                           rotary_positions(kv, start_pos, position_ids, T),
                           kv.k_pages(self.layer_index),
                           kv.v_pages(self.layer_index), kv.page_table(),
                           start_pos)
        attn = paged_attention_qkv(qkv, kv, self.layer_index, start_pos, Hq,
                                   Hkv, self.scale, tree_mask=tree_mask)
        a = ops.linear(attn, self.o_w)
        # parallel branches: both read the SAME layernorm output
        m = ops.linear(ops.gelu_tanh(ops.linear(x, self.up_w)), self.down_w)
        return hidden + a + m

    def forward_train(self, hidden: torch.Tensor, start_pos: int = 0) -> torch.Tensor:
        H = hidden.shape[-1]
        x = F.layer_norm(
            hidden.float(), (H,), self.ln_w.float(), self.ln_b.float(),
            self.config.layer_norm_epsilon).to(hidden.dtype)
        q, k, v = split_heads(F.linear(x, self.qkv_w), self.Hq, self.Hkv,
                              self.D)
        attn = rope_attn_train(q, k, v, self.rope, start_pos, self.scale)
        a = F.linear(attn, self.o_w)
        u = F.linear(x, self.up_w)
        g = F.gelu(u.float(), approximate="tanh").to(u.dtype)
        m = F.linear(g, self.down_w)
        return hidden + a + m
