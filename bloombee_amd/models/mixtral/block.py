"""Server-side Mixtral block (parity: reference models/mixtral/block.py
WrappedMixtralBlock :13-137): LLaMA-style GQA attention + top-2 MoE MLP.

MoE execution (MI-native): tokens are gathered per selected expert and each
expert's gate_up/down run as skinny-M GEMMs — at decode batch sizes every
expert's token group is M <= 32, exactly the shape gemm_skinny.hip is built
for (BASELINE.json config 4's "MoE grouped GEMM"); the scatter-add back is a
single index_add per expert."""
from __future__ import annotations

import math
from typing import Optional

import torch

from bloombee_amd import ops
from bloombee_amd.kv.paged import SessionHandle
from bloombee_amd.models.base import ModelConfig
from bloombee_amd.models.block_common import (
    FamilyBlock, RopeTables, pack_q4, paged_attention_qkv, rms_train,
    rope_attn_train, rotary_positions, split_heads, swiglu_mlp_train)


class MixtralBlock(FamilyBlock):
    def __init__(self, config: ModelConfig, layer_index: int = 0,
                 rope: Optional[RopeTables] = None):
        super().__init__(config, layer_index)
        H = config.hidden_size
        D = config.head_dim
        Hq, Hkv = config.num_attention_heads, config.num_key_value_heads
        I = config.intermediate_size
        E = int(config.extras.get("num_local_experts", 8))
        K = int(config.extras.get("num_experts_per_tok", 2))
        self.Hq, self.Hkv, self.D, self.I, self.E, self.topk = Hq, Hkv, D, I, E, K
        self.scale = 1.0 / math.sqrt(D)
        self.rope = rope if rope is not None else RopeTables(config)
        p = self.p
        self.input_norm_w = p(H)
        self.qkv_w = p((Hq + 2 * Hkv) * D, H)
        self.o_w = p(H, Hq * D)
        self.post_norm_w = p(H)
        self.router_w = p(E, H)
        self.expert_gate_up_w = p(E, 2 * I, H)
        self.expert_down_w = p(E, H, I)

    # -- 4-bit weights ----------------------------------------------------
    @torch.no_grad()
    def quantize_weights_q4(self, keep_full: bool = False):
        """Pack qkv_w, o_w and both expert weight stacks into 4-bit group
        codes (quant4_pack layout, experts keep their leading dimension);
        the router and the norms stay bf16. Decode then streams ~3.5x fewer
        bytes: the attention projections through ops.linear_w4, the grouped
        expert GEMMs through ops.moe_gemm_grouped_w4. keep_full=False drops
        the bf16 weights (the block becomes inference-only)."""
        pack_q4(self, ("qkv_w", "o_w", "expert_gate_up_w", "expert_down_w"),
                keep_full)
        return self

    def _lin(self, x, w, name):
        """ops.linear, or the 4-bit weight-stream kernel on a quantized
        block (quantize_weights_q4)."""
        w4 = getattr(self, "_w4", None)
        if w4 is not None and name in w4:
            packed, scale, zero, N = w4[name]
            return ops.linear_w4(x, packed, scale, zero, N)
        return ops.linear(x, w)

    def _expert_w(self, name, le, dtype):
        """Local expert le's weight matrix; dequantized on a quantized block."""
        w4 = getattr(self, "_w4", None)
        if w4 is None or name not in w4:
            return getattr(self, name)[le]
        packed, scale, zero, N = w4[name]
        G = scale.shape[-1]
        return ops.quant4_unpack(packed[le].reshape(N * G, 32),
                                 scale[le].reshape(-1), zero[le].reshape(-1),
                                 dtype=dtype).reshape(N, G * 64).to(dtype)

    # -- MoE MLP ----------------------------------------------------------
    def _grouped_experts(self, flat, off, tok, wsorted) -> torch.Tensor:
        """Both expert GEMMs as grouped launches over expert-sorted slots
        (off / tok / wsorted on device: prefix sums, slot -> token, slot
        routing weight), SwiGLU between them and the scatter-add back to
        tokens. Shapes depend on the token count only: no host sync."""
        Tk = tok.numel()
        mch = (flat.shape[0] + 31) // 32
        w4 = getattr(self, "_w4", None)
        if w4 is not None:
            gu = ops.moe_gemm_grouped_w4(
                flat, *w4["expert_gate_up_w"][:3], off, rowmap=tok,
                S=Tk, mchunks=mch)
            dn = ops.moe_gemm_grouped_w4(
                ops.swiglu(gu), *w4["expert_down_w"][:3], off,
                slot_scale=wsorted, S=Tk, mchunks=mch)
        else:
            gu = ops.moe_gemm_grouped(flat, self.expert_gate_up_w, off,
                                      rowmap=tok, S=Tk, mchunks=mch)
            dn = ops.moe_gemm_grouped(ops.swiglu(gu), self.expert_down_w,
                                      off, scale=wsorted, S=Tk, mchunks=mch)
        out = torch.zeros_like(flat)
        out.index_add_(0, tok.long(), dn)
        return out

    def _moe(self, y: torch.Tensor) -> torch.Tensor:
        B, T, H = y.shape
        flat = y.reshape(-1, H)
        logits = ops.linear(flat, self.router_w).float()
        weights, experts = logits.topk(self.topk, dim=-1)
        weights = torch.softmax(weights, dim=-1).to(y.dtype)
        e0, e1 = getattr(self, "ep_range", (0, self.E))
        if (flat.is_cuda and ops.HAVE_HIP_OPS
                and flat.dtype == torch.bfloat16
                and (e0, e1) == (0, self.E) and flat.shape[0] <= 1024
                and not getattr(self, "moe_loop", False)):
            # grouped decode path: expert-sort the (token, choice) slots on
            # device and run BOTH expert GEMMs as single grouped launches
            # (ops/hip/moe_gemm.hip) — no per-expert host sync, no
            # per-expert kernel launches (BASELINE config 4)
            fe = experts.reshape(-1)
            order = fe.argsort(stable=True)
            counts = torch.bincount(fe, minlength=self.E)
            off = torch.zeros(self.E + 1, dtype=torch.int32,
                              device=flat.device)
            off[1:] = counts.cumsum(0).int()
            tok = (order // self.topk).int()
            wsorted = weights.reshape(-1)[order].float()
            return self._grouped_experts(flat, off, tok, wsorted).view(B, T, H)
        out = torch.zeros_like(flat)
        # expert-parallel mode (parallel/expert.py): this rank holds only
        # experts [e0, e1); partial sums cross ranks via one all-reduce
        for le, e in enumerate(range(e0, e1)):
            sel = (experts == e)
            rows = sel.any(dim=-1).nonzero(as_tuple=True)[0]
            if rows.numel() == 0:
                continue
            xe = flat[rows]
            h = ops.linear(
                ops.swiglu(ops.linear(
                    xe, self._expert_w("expert_gate_up_w", le, xe.dtype))),
                self._expert_w("expert_down_w", le, xe.dtype))
            w = (weights * sel.to(weights.dtype)).sum(-1)[rows]
            out.index_add_(0, rows, h * w.unsqueeze(-1))
        if getattr(self, "ep_enabled", False):
            from bloombee_amd.parallel.expert import ep_all_reduce
            ep_all_reduce(out, self.ep_group)
        return out.view(B, T, H)

    @torch.no_grad()
    def forward_inference(self, hidden: torch.Tensor, kv: SessionHandle,
                          start_pos: torch.Tensor, position_ids=None,
                          tree_mask=None) -> torch.Tensor:
        B, T, H = hidden.shape
        Hq, Hkv = self.Hq, self.Hkv
        cfg = self.config
        x = ops.rms_norm(hidden, self.input_norm_w, cfg.rms_norm_eps)
        qkv = self._lin(x, self.qkv_w, "qkv_w")
        cos, sin = self.rope.get(hidden.device)
        ops.rope_kv_write_(qkv, Hq, Hkv, cos, sin,
                           rotary_positions(kv, start_pos, position_ids, T),
                           kv.k_pages(self.layer_index),
                           kv.v_pages(self.layer_index), kv.page_table(),
                           start_pos)
        attn = paged_attention_qkv(qkv, kv, self.layer_index, start_pos, Hq,
                                   Hkv, self.scale, tree_mask=tree_mask)
        a = self._lin(attn, self.o_w, "o_w")
        h2, y = ops.rms_norm_residual(a, hidden, self.post_norm_w, cfg.rms_norm_eps)
        return h2 + self._moe(y)

    def forward_train(self, hidden: torch.Tensor, start_pos: int = 0) -> torch.Tensor:
        if self.qkv_w.numel() == 0:
            raise RuntimeError(
                "forward_train needs the bf16 weights: this block was "
                "quantized with quantize_weights_q4(keep_full=False) and is "
                "inference-only")
        B, T, H = hidden.shape
        eps = self.config.rms_norm_eps
        x = rms_train(hidden, self.input_norm_w, eps)
        q, k, v = split_heads(torch.nn.functional.linear(x, self.qkv_w),
                              self.Hq, self.Hkv, self.D)
        attn = rope_attn_train(q, k, v, self.rope, start_pos, self.scale)
        h2 = hidden + torch.nn.functional.linear(attn, self.o_w)
        y = rms_train(h2, self.post_norm_w, eps)

        flat = y.reshape(-1, H)
        logits = torch.nn.functional.linear(flat, self.router_w).float()
        weights, experts = logits.topk(self.topk, dim=-1)
        weights = torch.softmax(weights, dim=-1).to(y.dtype)
        out = torch.zeros_like(flat)
        e0, e1 = getattr(self, "ep_range", (0, self.E))
        for le, e in enumerate(range(e0, e1)):
            sel = (experts == e)
            rows = sel.any(dim=-1).nonzero(as_tuple=True)[0]
            if rows.numel() == 0:
                continue
            xe = flat[rows]
            h = swiglu_mlp_train(xe, self.expert_gate_up_w[le],
                                 self.expert_down_w[le])
            w = (weights * sel.to(weights.dtype)).sum(-1)[rows]
            out = out.index_add(0, rows, h * w.unsqueeze(-1))
        if getattr(self, "ep_enabled", False):
            from bloombee_amd.parallel.expert import ep_all_reduce
            ep_all_reduce(out, self.ep_group)
        return h2 + out.view(B, T, H)
