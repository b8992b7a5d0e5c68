"""What every family's server block shares: the base class (parameter
factory, random init, forward), rotary positions and paged-attention dispatch
for mixed-device sessions, the eager train-path pieces and 4-bit packing.

A feature that concerns "every family" (mixed-device decode, tree-mask verify,
sparse decode ...) belongs here, once; the family files keep what is theirs.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F

from bloombee_amd import ops
from bloombee_amd.models.base import ModelConfig
from bloombee_amd.ops import reference as refops


class RopeTables:
    """Shared host-precomputed cos/sin tables, materialized per device."""

    def __init__(self, config: ModelConfig):
        self.config = config
        cos, sin = ops.rope_cos_sin(
            config.head_dim, config.max_position_embeddings,
            theta=config.rope_theta, scaling=config.rope_scaling,
        )
        self._cos, self._sin = cos, sin
        self._cache = {}

    def get(self, device: torch.device):
        key = str(device)
        if key not in self._cache:
            self._cache[key] = (self._cos.to(device), self._sin.to(device))
        return self._cache[key]


class FamilyBlock(torch.nn.Module):
    """Base of the server blocks. Two forward paths (mirroring the
    reference's split between iterate_rpc_inference and
    run_rpc_forward/backward):
      forward_inference — HIP kernels + paged KV, no autograd.
      forward_train     — differentiable eager composition used by the
                          fine-tuning RPCs; gradients flow to inputs/prompts
                          only (server weights frozen)."""

    def __init__(self, config: ModelConfig, layer_index: int = 0):
        super().__init__()
        self.config = config
        self.layer_index = layer_index

    def p(self, *shape) -> torch.nn.Parameter:
        return torch.nn.Parameter(torch.empty(*shape, dtype=self.config.dtype),
                                  requires_grad=False)

    @staticmethod
    def init_kind(name: str) -> str:
        """How init_random fills parameter `name`: "zeros" for biases, "ones"
        for norm weights, "random" for the rest. This is the union of the
        former per-family rules (llama-pattern: *norm_w; falcon: ln_w / ln_b;
        bloom: *_b, ln*), so a new parameter named *_b or ln* does not draw
        from the generator in any family. A family whose names do not follow
        the convention overrides this."""
        if name.endswith("_b"):
            return "zeros"
        if name.endswith("norm_w") or name.startswith("ln"):
            return "ones"
        return "random"

    @torch.no_grad()
    def init_random(self, seed: Optional[int] = None):
        """Random-init weights. Generates on the parameters' current device —
        device-side RNG for resident blocks (seconds for 70B-class shards vs
        minutes of host randn + transfer). Same (device kind, seed) => same
        weights, which is what the multi-rank parity argument needs. The
        default seed follows the block's index in the whole model
        (global_index where a stack has rebased layer_index)."""
        index = getattr(self, "global_index", self.layer_index)
        s = seed if seed is not None else 1234 + index
        dev = next(self.parameters()).device
        gen = torch.Generator(device=dev).manual_seed(s)
        std = 0.02 / math.sqrt(2 * self.config.num_hidden_layers)
        for name, w in self.named_parameters():
            kind = self.init_kind(name)
            if kind == "random":
                w.copy_(torch.randn(w.shape, generator=gen, dtype=torch.float32,
                                    device=dev).mul_(std).to(w.dtype))
            else:
                w.fill_(1.0 if kind == "ones" else 0.0)
        return self

    def _no_tree_mask(self, tree_mask) -> None:
        if tree_mask is not None:
            raise NotImplementedError(
                f"{self.config.model_type}: tree-mask (speculative verify) "
                "attention is not implemented for this family")

    def forward(self, *args, **kw):
        return self.forward_inference(*args, **kw)


# ----------------------------------------------------------------------
# inference path: mixed-device sessions (kv.swap_in_as_prefix — committed KV
# on the host, recent segment in the device pool) and attention dispatch
# ----------------------------------------------------------------------
def rotary_positions(kv, start_pos: torch.Tensor,
                     position_ids: Optional[torch.Tensor], T: int,
                     always: bool = False) -> Optional[torch.Tensor]:
    """Rotary positions (B, T) of a step's tokens. start_pos and the paged
    indices are LOCAL to the device pool, rotary positions stay ABSOLUTE:
    kv.pos_offset is where the device segment starts. Explicit position_ids
    pass through unchanged; without an offset the result is None — the
    kernels derive start_pos + t themselves — and with one it is int32, as
    the kernels take it. `always` (blocks whose RoPE is a torch composition
    and indexes the tables) materializes long positions in every case."""
    if position_ids is not None:
        return position_ids.long() if always else position_ids
    off = getattr(kv, "pos_offset", 0)
    if not off and not always:
        return None
    pos = (start_pos.view(-1, 1).long() + off
           + torch.arange(T, device=start_pos.device).view(1, T))
    return pos if always else pos.int()


def _host_prefix(kv, layer: int):
    return kv.host_prefix(layer) if hasattr(kv, "host_prefix") else None


def paged_attention_qkv(qkv: torch.Tensor, kv, layer: int,
                        start_pos: torch.Tensor, Hq: int, Hkv: int,
                        scale: float, *, window: int = 0, tree_mask=None,
                        ctx_lens=None) -> torch.Tensor:
    """Attention for blocks holding the fused QKV buffer (B, T, (Hq+2Hkv)*D),
    q section roped and the new K/V already in layer `layer`'s pages. Returns
    (B, T, Hq*D), the O-projection input. ctx_lens: rope_kv_write_part's
    start_pos + T by-product, used by single-token decode."""
    B, T, _ = qkv.shape
    kp, vp, pt = kv.k_pages(layer), kv.v_pages(layer), kv.page_table()
    hp = _host_prefix(kv, layer)
    if hp is not None:
        # exact two-segment merge (ref _mixed_device_attention): the host
        # prefix is attended on the CPU, the recent segment via the paged
        # pool; decode-only (backend gates T == 1)
        return ops.attn_paged_mixed_qkv(qkv, Hq, Hkv, kp, vp, pt,
                                        start_pos + T, hp[0], hp[1], scale,
                                        window=window)
    if tree_mask is not None:
        # tree-structured verify step (spec decoding): unfused q view + the
        # tree-mask attention path
        D = kp.shape[3]
        q = (qkv[..., : Hq * D].view(B, T, Hq, D)
             .permute(0, 2, 1, 3).contiguous())
        attn = ops.attn_paged(q, kp, vp, pt, start_pos.long(), scale,
                              window=window, tree_mask=tree_mask)
        return attn.permute(0, 2, 1, 3).reshape(B, T, Hq * D)
    return ops.attn_paged_qkv(qkv, Hq, Hkv, kp, vp, pt, start_pos, scale,
                              window=window,
                              ctx_lens=ctx_lens if T == 1 else None)


def paged_attention(q: torch.Tensor, kv, layer: int, start_pos: torch.Tensor,
                    scale: float, *, window: int = 0,
                    alibi_slopes=None) -> torch.Tensor:
    """The same dispatch for blocks holding a separate (B, Hq, T, D) query
    (K/V of the step already written to layer `layer`'s pages — the donor's
    for shared-KV layers). ALiBi positions are absolute: the mixed op shifts
    the device segment by the prefix length; sliding layers see only the
    host suffix still inside the window. Returns (B, T, Hq*D)."""
    B, Hq, T, D = q.shape
    kp, vp, pt = kv.k_pages(layer), kv.v_pages(layer), kv.page_table()
    hp = _host_prefix(kv, layer)
    if hp is not None:
        out = ops.attn_paged_mixed(q, kp, vp, pt, start_pos + T, hp[0], hp[1],
                                   scale, window=window,
                                   alibi_slopes=alibi_slopes)
    else:
        out = ops.attn_paged(q, kp, vp, pt, start_pos.long(), scale,
                             window=window, alibi_slopes=alibi_slopes)
    return out.permute(0, 2, 1, 3).reshape(B, T, Hq * D)


# ----------------------------------------------------------------------
# training path (differentiable; full sequence, no KV cache)
# ----------------------------------------------------------------------
def rms_train(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    """RMS norm that rounds to x.dtype BEFORE the weight multiply (not
    refops.rms_norm, which rounds once after it)."""
    xf = x.float()
    return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
            ).to(x.dtype) * w


def split_heads(qkv: torch.Tensor, Hq: int, Hkv: int, D: int):
    """(B, T, (Hq+2Hkv)*D) -> q (B, Hq, T, D), k and v (B, Hkv, T, D) views."""
    B, T, _ = qkv.shape
    return (qkv.view(B, T, Hq + 2 * Hkv, D).permute(0, 2, 1, 3)
            .split([Hq, Hkv, Hkv], dim=1))


def rope_attn_train(q, k, v, rope: RopeTables, start_pos: int,
                    scale: float) -> torch.Tensor:
    """RoPE at positions start_pos.. on q/k (B, H, T, D), then causal
    training attention. Returns (B, T, Hq*D)."""
    B, Hq, T, D = q.shape
    cos, sin = rope.get(q.device)
    pos = torch.arange(start_pos, start_pos + T,
                       device=q.device).view(1, T).expand(B, T)
    q, k = refops.rope_apply(q, k, cos, sin, pos)
    attn = ops.attn_train(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3),
                          v.permute(0, 2, 1, 3), scale)
    return attn.reshape(B, T, Hq * D)


def swiglu_mlp_train(y: torch.Tensor, gate_up_w: torch.Tensor,
                     down_w: torch.Tensor) -> torch.Tensor:
    g, u = F.linear(y, gate_up_w).chunk(2, dim=-1)
    return F.linear(F.silu(g.float()).to(u.dtype) * u, down_w)


# ----------------------------------------------------------------------
# 4-bit weights
# ----------------------------------------------------------------------
@torch.no_grad()
def pack_q4(block: torch.nn.Module, names, keep_full: bool = False) -> None:
    """Pack the named weights into 4-bit group codes (quant4_pack layout;
    stacked weights keep their leading dimensions) as block._w4[name] =
    (packed, scale, zero, N). keep_full=False drops the bf16 weights: the
    block becomes inference-only."""
    block._w4 = {}
    for name in names:
        w = getattr(block, name).detach()
        packed, scale, zero = ops.quant4_pack(w)
        lead = tuple(w.shape[:-1])
        block._w4[name] = (packed.reshape(*lead, -1).contiguous(),
                           scale.reshape(*lead, -1).half().contiguous(),
                           zero.reshape(*lead, -1).half().contiguous(),
                           w.shape[-2])
        if not keep_full:
            getattr(block, name).data = torch.empty(
                0, dtype=w.dtype, device=w.device)
