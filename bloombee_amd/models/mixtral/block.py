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
from bloombee_amd.models.llama.block import RopeTables


class MixtralBlock(torch.nn.Module):
    def __init__(self, config: ModelConfig, layer_index: int = 0,
                 rope: Optional[RopeTables] = None):
        super().__init__()
        self.config = config
        self.layer_index = layer_index
        H = config.hidden_size
        D = config.head_dim
        Hq, Hkv = config.num_attention_heads, config.num_key_value_heads
        I = config.intermediate_size
        E = int(config.extras.get("num_local_experts", 8))
        K = int(config.extras.get("num_experts_per_tok", 2))
        dt = config.dtype
        self.Hq, self.Hkv, self.D, self.I, self.E, self.topk = Hq, Hkv, D, I, E, K
        self.scale = 1.0 / math.sqrt(D)
        self.rope = rope if rope is not None else RopeTables(config)

        def p(*shape):
            return torch.nn.Parameter(torch.empty(*shape, dtype=dt),
                                      requires_grad=False)

        self.input_norm_w = p(H)
        self.qkv_w = p((Hq + 2 * Hkv) * D, H)
        self.o_w = p(H, Hq * D)
        self.post_norm_w = p(H)
        self.router_w = p(E, H)
        self.expert_gate_up_w = p(E, 2 * I, H)
        self.expert_down_w = p(E, H, I)

    @torch.no_grad()
    def init_random(self, seed: Optional[int] = None):
        s = seed if seed is not None else 1234 + self.layer_index
        dev = self.input_norm_w.device
        gen = torch.Generator(device=dev).manual_seed(s)
        std = 0.02 / math.sqrt(2 * self.config.num_hidden_layers)
        for name, w in self.named_parameters():
            if name.endswith("norm_w"):
                w.fill_(1.0)
            else:
                w.copy_(torch.randn(w.shape, generator=gen, dtype=torch.float32,
                                    device=dev).mul_(std).to(w.dtype))
        return self

    # -- 4-bit weights ----------------------------------------------------
    @torch.no_grad()
    def quantize_weights_q4(self, keep_full: bool = False):
        """Pack qkv_w, o_w and both expert weight stacks into 4-bit group
        codes (quant4_pack layout, experts keep their leading dimension);
        the router and the norms stay bf16. Decode then streams ~3.5x fewer
        bytes: the attention projections through ops.linear_w4, the grouped
        expert GEMMs through ops.moe_gemm_grouped_w4. keep_full=False drops
        the bf16 weights (the block becomes inference-only)."""
        self._w4 = {}
        for name in ("qkv_w", "o_w", "expert_gate_up_w", "expert_down_w"):
            w = getattr(self, name).detach()
            packed, scale, zero = ops.quant4_pack(w)
            lead = tuple(w.shape[:-1])
            self._w4[name] = (packed.reshape(*lead, -1).contiguous(),
                              scale.reshape(*lead, -1).half().contiguous(),
                              zero.reshape(*lead, -1).half().contiguous(),
                              w.shape[-2])
            if not keep_full:
                getattr(self, name).data = torch.empty(
                    0, dtype=w.dtype, device=w.device)
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
                          start_pos: torch.Tensor,
                          position_ids=None) -> torch.Tensor:
        B, T, H = hidden.shape
        Hq, Hkv = self.Hq, self.Hkv
        cfg = self.config
        x = ops.rms_norm(hidden, self.input_norm_w, cfg.rms_norm_eps)
        qkv = self._lin(x, self.qkv_w, "qkv_w")
        cos, sin = self.rope.get(hidden.device)
        kp = kv.k_pages(self.layer_index)
        vp = kv.v_pages(self.layer_index)
        pt = kv.page_table()
        # mixed-device sessions (host KV prefix + device recent segment):
        # pool positions are local, rotary stays absolute (see llama block)
        off = getattr(kv, "pos_offset", 0)
        if off and position_ids is None:
            position_ids = (start_pos.view(B, 1) + off
                            + torch.arange(T, device=hidden.device)
                            .view(1, T)).int()
        ops.rope_kv_write_(qkv, Hq, Hkv, cos, sin, position_ids, kp, vp, pt,
                           start_pos)
        hp = (kv.host_prefix(self.layer_index)
              if hasattr(kv, "host_prefix") else None)
        if hp is not None:
            # exact two-segment merge; decode-only (backend gates T == 1)
            attn = ops.attn_paged_mixed_qkv(qkv, Hq, Hkv, kp, vp, pt,
                                            start_pos + T, hp[0], hp[1],
                                            self.scale)
        else:
            attn = ops.attn_paged_qkv(qkv, Hq, Hkv, kp, vp, pt, start_pos,
                                      self.scale)
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
        Hq, Hkv, D = self.Hq, self.Hkv, self.D
        cfg = self.config

        def rms(x, w):
            xf = x.float()
            return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True)
                                     + cfg.rms_norm_eps)).to(x.dtype) * w

        x = rms(hidden, self.input_norm_w)
        qkv = torch.nn.functional.linear(x, self.qkv_w)
        qkv = qkv.view(B, T, Hq + 2 * Hkv, D).permute(0, 2, 1, 3)
        q, k, v = qkv.split([Hq, Hkv, Hkv], dim=1)
        cos, sin = self.rope.get(hidden.device)
        pos = torch.arange(start_pos, start_pos + T,
                           device=hidden.device).view(1, T).expand(B, T)
        from bloombee_amd.ops import reference as refops
        q, k = refops.rope_apply(q, k, cos, sin, pos)
        attn = ops.attn_train(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3),
                              v.permute(0, 2, 1, 3), self.scale)
        attn = attn.reshape(B, T, Hq * D)
        h2 = hidden + torch.nn.functional.linear(attn, self.o_w)
        y = rms(h2, self.post_norm_w)

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
            gu = torch.nn.functional.linear(xe, self.expert_gate_up_w[le])
            g, u = gu.split([self.I, self.I], dim=-1)
            h = torch.nn.functional.linear(
                torch.nn.functional.silu(g.float()).to(u.dtype) * u,
                self.expert_down_w[le])
            w = (weights * sel.to(weights.dtype)).sum(-1)[rows]
            out = out.index_add(0, rows, h * w.unsqueeze(-1))
        if getattr(self, "ep_enabled", False):
            from bloombee_amd.parallel.expert import ep_all_reduce
            ep_all_reduce(out, self.ep_group)
        return h2 + out.view(B, T, H)

    def forward(self, *args, **kw):
        return self.forward_inference(*args, **kw)
