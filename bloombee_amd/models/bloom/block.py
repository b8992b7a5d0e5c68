"""Server-side BLOOM block (parity: reference models/bloom/block.py
WrappedBloomBlock — HF eager with alibi, :108-188). MI-native composition on
the shared op layer: LayerNorm + fused-QKV + alibi paged attention +
gelu MLP, all biased; MHA (num_key_value_heads == num_attention_heads);
KV rides the same paged pools as every family."""
from __future__ import annotations

import math

import torch

from bloombee_amd import ops
from bloombee_amd.kv.paged import SessionHandle
from bloombee_amd.models.base import ModelConfig
from bloombee_amd.models.block_common import FamilyBlock, paged_attention


class BloomBlock(FamilyBlock):
    def __init__(self, config: ModelConfig, layer_index: int = 0, rope=None):
        super().__init__(config, layer_index)
        H = config.hidden_size
        D = config.head_dim
        Hq = config.num_attention_heads
        I = config.intermediate_size
        self.Hq, self.D, self.I = Hq, D, I
        self.scale = 1.0 / math.sqrt(D)
        # buffer (not a plain attr) so .to(device) moves it once: a CPU
        # tensor here means a pageable H2D copy per layer per step in the
        # attention dispatch — wasteful eager and illegal under hipGraph
        # capture (the bloom capture fault isolated in r02)
        self.register_buffer("alibi", ops.alibi_slopes_for(Hq).float(),
                             persistent=False)
        p = self.p
        self.ln1_w, self.ln1_b = p(H), p(H)
        self.qkv_w, self.qkv_b = p(3 * Hq * D, H), p(3 * Hq * D)
        self.dense_w, self.dense_b = p(H, Hq * D), p(H)
        self.ln2_w, self.ln2_b = p(H), p(H)
        self.up_w, self.up_b = p(I, H), p(I)
        self.down_w, self.down_b = p(H, I), p(H)

    def _attn(self, x: torch.Tensor, kv: SessionHandle,
              start_pos: torch.Tensor) -> torch.Tensor:
        B, T, _ = x.shape
        Hq, D = self.Hq, self.D
        qkv = ops.linear(x, self.qkv_w, bias=self.qkv_b)
        q = qkv[..., :Hq * D].view(B, T, Hq, D).permute(0, 2, 1, 3).contiguous()
        k = qkv[..., Hq * D:2 * Hq * D].view(B, T, Hq, D).permute(0, 2, 1, 3).contiguous()
        v = qkv[..., 2 * Hq * D:].view(B, T, Hq, D).permute(0, 2, 1, 3).contiguous()
        ops.kv_write(k, v, kv.k_pages(self.layer_index),
                     kv.v_pages(self.layer_index), kv.page_table(), start_pos)
        out = paged_attention(q, kv, self.layer_index, start_pos, self.scale,
                              alibi_slopes=self.alibi)
        return ops.linear(out, self.dense_w, bias=self.dense_b)

    @torch.no_grad()
    def forward_inference(self, hidden: torch.Tensor, kv: SessionHandle,
                          start_pos: torch.Tensor, position_ids=None,
                          tree_mask=None) -> torch.Tensor:
        self._no_tree_mask(tree_mask)
        cfg = self.config
        x = ops.layer_norm(hidden, self.ln1_w, self.ln1_b, cfg.layer_norm_epsilon)
        h = hidden + self._attn(x, kv, start_pos)
        y = ops.layer_norm(h, self.ln2_w, self.ln2_b, cfg.layer_norm_epsilon)
        m = ops.linear(ops.gelu_tanh(ops.linear(y, self.up_w, bias=self.up_b)),
                       self.down_w, bias=self.down_b)
        return h + m

    def forward_train(self, hidden: torch.Tensor, start_pos: int = 0) -> torch.Tensor:
        cfg = self.config
        B, T, H = hidden.shape
        Hq, D = self.Hq, self.D

        def ln(x, w, b):
            return torch.nn.functional.layer_norm(
                x.float(), (H,), w.float(), b.float(),
                cfg.layer_norm_epsilon).to(x.dtype)

        x = ln(hidden, self.ln1_w, self.ln1_b)
        qkv = torch.nn.functional.linear(x, self.qkv_w, self.qkv_b)
        q, k, v = (t.view(B, T, Hq, D).permute(0, 2, 1, 3)
                   for t in qkv.split(Hq * D, dim=-1))
        attn = ops.attn_train(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3),
                              v.permute(0, 2, 1, 3), self.scale,
                              alibi_slopes=self.alibi)
        attn = attn.reshape(B, T, Hq * D)
        h = hidden + torch.nn.functional.linear(attn, self.dense_w, self.dense_b)
        y = ln(h, self.ln2_w, self.ln2_b)
        u = torch.nn.functional.linear(y, self.up_w, self.up_b)
        g = torch.nn.functional.gelu(u.float(), approximate="tanh").to(u.dtype)
        m = torch.nn.functional.linear(g, self.down_w, self.down_b)
        return h + m
