"""Server-side LLaMA decoder block on the gfx950 op library.

Replaces the reference's OptimizedLlamaDecoderLayer + FLEX_LlamaAttention/MLP
stack (models/llama/block.py:149-861, models/llama/flex_llama.py:434-793) with
a flat MI355X-native block:

  * plain-GEMM projections via hipBLASLt (torch F.linear on bf16) with QKV and
    gate/up fused into single GEMMs (fewer, larger GEMMs — xGMI/HBM sizing),
  * hand-written HIP kernels for everything fused: rmsnorm(+residual), RoPE,
    paged KV write, paged decode/prefill attention, SwiGLU,
  * one paged KV pool shared across local layers (kv/paged.py), no
    ValueHolder grids, no per-layer load/store streams: weights are resident
    in 288 GB HBM by default; the offload tier is a separate module.

What the block shares with the other families (base class, rotary positions
and attention dispatch of mixed-device sessions, train-path pieces, 4-bit
packing) lives in models/block_common.py. The fused-norm chain, the weight
fold, _lin and the deferred qkv combine are LLaMA-pattern specific and stay
here; Qwen3 is this block plus the _post_qkv / _post_qkv_train hooks.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch
import torch.nn.functional as F

from bloombee_amd import ops
from bloombee_amd.kv.paged import SessionHandle
from bloombee_amd.models.base import ModelConfig
from bloombee_amd.models.block_common import (  # noqa: F401 (RopeTables: re-export)
    FamilyBlock, RopeTables, pack_q4, paged_attention_qkv, rms_train,
    rope_attn_train, rotary_positions, split_heads, swiglu_mlp_train)


# Packed decode weights (ops.pack_skinny_w; profiles/r08_packed_w.md): a
# second copy of a projection in the skinny GEMM kernel's read order, one
# contiguous 1 KB per wave load. BBAMD_PACK_W (read at every call): "0" never
# packs, "1" packs every projection of the fused-norm decode path, "auto"
# packs the (N, K) shapes of _PACK_W_FASTER — those the flagship's kernel
# trace measured faster packed; unmeasured shapes stay unpacked — and only
# while free device memory after the copy stays >= 1/8 of the device's total
# (a policy reserve for KV pages and activations, not a measurement).
_PACK_W_DEFAULT = "auto"
_PACK_W_FASTER: frozenset = frozenset((
    (6144, 4096),       # qkv      13.8 -> 12.5 us
    (4096, 4096),       # o         9.3 ->  8.3 us
    (28672, 4096),      # gate_up  49.8 -> 41.6 us
    (4096, 14336),      # down     25.0 -> 22.4 us
))
_PACK_W_RESERVE = 8     # keep total / 8 free


def _pack_w_mode() -> str:
    v = os.environ.get("BBAMD_PACK_W", _PACK_W_DEFAULT).strip().lower()
    return v if v in ("0", "1") else "auto"


class LlamaBlock(FamilyBlock):
    def __init__(self, config: ModelConfig, layer_index: int = 0,
                 rope: Optional[RopeTables] = None):
        super().__init__(config, layer_index)
        H = config.hidden_size
        D = config.head_dim
        Hq, Hkv = config.num_attention_heads, config.num_key_value_heads
        I = config.intermediate_size
        self.Hq, self.Hkv, self.D, self.I = Hq, Hkv, D, I
        self.scale = 1.0 / math.sqrt(D)
        p = self.p
        self.input_norm_w = p(H)
        self.qkv_w = p((Hq + 2 * Hkv) * D, H)     # fused q|k|v
        self.o_w = p(H, Hq * D)
        self.post_norm_w = p(H)
        self.gate_up_w = p(2 * I, H)              # fused gate|up
        self.down_w = p(H, I)
        self.rope = rope if rope is not None else RopeTables(config)
        # fused-norm chain state (forward_inference fuse_norm path):
        # per-stripe row sum-of-squares buffers, (H/64, 32) f32, written by
        # the o/down GEMM epilogues and consumed by the next fused rmsnorm
        self._ss_h2 = None
        self._ss_hidden = None
        self._ss_valid = False
        # split-K tickets of the in-launch combine (ops.linear cnt=...): one
        # int32 buffer, a slice of H/64 entries each for o-proj and down-proj;
        # zero between launches (the kernel resets what it counted)
        self._splitk_cnt = None
        # packed decode weights: name -> (alias of the weight packed from,
        # its _version then, packed copy or None where policy declined)
        self._wpacked = {}

    def _drop_packed(self) -> None:
        self._wpacked.clear()

    def _packed(self, name: str, swiglu: bool = False):
        """Packed copy of projection `name` for ops.linear(w_packed=...) /
        ops.linear_swiglu(w_packed=...), or None to run unpacked. Built once,
        outside stream capture, and valid only for the very tensor it was
        built from: the entry keeps that tensor's storage alive (so no other
        tensor can take its address) and compares data_ptr and _version, so a
        reassigned .data (fold / unfold, a move to another device) or an
        in-place write (load_state_dict) rebuilds it on the next call."""
        mode = _pack_w_mode()
        if mode == "0":
            self._drop_packed()
            return None
        w = getattr(self, name)
        ent = self._wpacked.get(name)
        if ent is not None:
            src, ver, wp = ent
            if src.data_ptr() == w.data_ptr() and ver == w._version:
                return wp
            del self._wpacked[name]
        if w.is_cuda and torch.cuda.is_current_stream_capturing():
            return None     # never allocate or pack inside a capture
        wp = None
        if mode == "1" or self._pack_auto_ok(w):
            wp = ops.pack_skinny_w(w.detach(), swiglu)
        self._wpacked[name] = (w.detach(), w._version, wp)
        return wp

    @staticmethod
    def _pack_auto_ok(w: torch.Tensor) -> bool:
        if tuple(w.shape) not in _PACK_W_FASTER or not w.is_cuda:
            return False
        free, total = torch.cuda.mem_get_info(w.device)
        return free - w.numel() * w.element_size() >= total // _PACK_W_RESERVE

    def _fuse_norm_gate(self, hidden) -> bool:
        """All four decode GEMMs must hit the v2 kernel (K%256) with
        stripe-aligned N so the fused-norm ss chain stays on-device;
        W4/LoRA blocks keep the separate-norm path."""
        return (getattr(self, "_w4", None) is None
                and getattr(self, "lora_delta", None) is None
                and ops.fuse_norm_linear_ok(hidden, self.qkv_w)
                and self.I % 256 == 0 and (2 * self.I) % 64 == 0
                and (self.Hq * self.D) % 256 == 0
                and self.config.hidden_size % 64 == 0)

    def _ensure_ss_bufs(self, device) -> None:
        if self._ss_h2 is None or self._ss_h2.device != device:
            st = self.config.hidden_size // 64
            self._ss_h2 = torch.empty(st * 32, dtype=torch.float32,
                                      device=device)
            self._ss_hidden = torch.empty_like(self._ss_h2)
            self._splitk_cnt = torch.zeros(2 * st, dtype=torch.int32,
                                           device=device)

    @torch.no_grad()
    def fold_norm_weights(self):
        """Reparameterize for the fused-norm decode path: qkv_w <- qkv_w *
        input_norm_w, gate_up_w <- gate_up_w * post_norm_w (f32 product,
        one bf16 round), norm weights <- 1. rms_norm with unit weight is
        mathematically unchanged on EVERY path (train, prefill, CPU), and
        the decode GEMM then only applies the per-row 1/rms in its
        epilogue (norm_mode 2) instead of per-element weight scaling
        (profiles/r02 §13: the per-stage scale cost +4-8 us/GEMM)."""
        if getattr(self, "_norm_folded", False):
            return
        self._drop_packed()
        self._norm_fold_orig = (self.input_norm_w.detach().clone(),
                                self.post_norm_w.detach().clone())
        self.qkv_w.data = (self.qkv_w.float()
                           * self.input_norm_w.float()).to(self.qkv_w.dtype)
        self.gate_up_w.data = (self.gate_up_w.float()
                               * self.post_norm_w.float()).to(self.gate_up_w.dtype)
        self.input_norm_w.data.fill_(1.0)
        self.post_norm_w.data.fill_(1.0)
        self._norm_folded = True

    @torch.no_grad()
    def unfold_norm_weights(self):
        """Best-effort inverse of fold_norm_weights (division re-rounds:
        ~1 ulp drift on the projections). Needed before attaching LoRA
        adapters trained against the original parameterization."""
        if not getattr(self, "_norm_folded", False):
            return
        self._drop_packed()
        inw, pnw = self._norm_fold_orig
        self.input_norm_w.data.copy_(inw)
        self.post_norm_w.data.copy_(pnw)
        den_i = inw.float().abs().clamp_min(1e-6) * inw.float().sign().where(
            inw.float() != 0, torch.ones_like(inw.float()))
        den_p = pnw.float().abs().clamp_min(1e-6) * pnw.float().sign().where(
            pnw.float() != 0, torch.ones_like(pnw.float()))
        self.qkv_w.data = (self.qkv_w.float() / den_i).to(self.qkv_w.dtype)
        self.gate_up_w.data = (self.gate_up_w.float() / den_p).to(self.gate_up_w.dtype)
        self._norm_folded = False

    @torch.no_grad()
    def quantize_weights_q4(self, keep_full: bool = False):
        """Pack the four projection weights into 4-bit group codes
        (quant4_pack layout); decode GEMMs then stream ~3.5x fewer bytes
        through w4_gemm.hip (FlexGen-style compression ON the compute
        path — the reference only compresses weights at rest,
        flexgen_utils/compression.py:94-210). keep_full=False drops the
        bf16 weights (4x memory; the block becomes inference-only and
        prefill-shaped GEMMs dequantize on the fly)."""
        self._drop_packed()
        pack_q4(self, ("qkv_w", "o_w", "gate_up_w", "down_w"), keep_full)
        return self

    def _lin(self, x, w, name, **kw):
        """ops.linear + optional active-LoRA delta (utils/peft.py).
        Quantized blocks (quantize_weights_q4) route through the 4-bit
        weight-stream kernel instead."""
        w4 = getattr(self, "_w4", None)
        if w4 is not None and name in w4:
            packed, scale, zero, N = w4[name]
            y = ops.linear_w4(x, packed, scale, zero, N, **kw)
        else:
            y = ops.linear(x, w, **kw)
        ld = getattr(self, "lora_delta", None)
        if ld is not None:
            d = ld(name, x)
            if d is not None:
                y = y + d
        return y

    def _post_qkv(self, qkv: torch.Tensor, B: int, T: int) -> torch.Tensor:
        """Hook on the combined bf16 QKV buffer (B, T, (Hq+2Hkv)*D) before
        RoPE; a no-op here. An override turns the deferred qkv combine off."""
        return qkv

    def _post_qkv_train(self, q: torch.Tensor, k: torch.Tensor):
        """The train path's form of the hook: q, k as (B, H, T, D)."""
        return q, k

    # ------------------------------------------------------------------
    # inference path (HIP kernels, paged KV)
    # ------------------------------------------------------------------
    @torch.no_grad()
    def forward_inference(
        self,
        hidden: torch.Tensor,              # (B, T, H) bf16
        kv: SessionHandle,
        start_pos: torch.Tensor,           # (B,) int32 — absolute pos of token 0
        position_ids: Optional[torch.Tensor] = None,  # (B, T) int32
        tree_mask: Optional[torch.Tensor] = None,     # (B, T, T) bool, spec verify
    ) -> torch.Tensor:
        B, T, H = hidden.shape
        Hq, Hkv, D = self.Hq, self.Hkv, self.D
        cfg = self.config

        # Decode-shaped GPU steps fold both per-layer rmsnorms into the
        # skinny GEMM's A-operand stage (ops.linear norm=...): two fewer
        # launches + elementwise passes per layer. The row sum-of-squares
        # the norm needs is produced by the PRECEDING GEMM's epilogue
        # (ss buffers chained block-to-block via prev_block; re-streaming
        # A instead costs +18-60 us/GEMM — profiles/r02 §13). W4/LoRA
        # blocks and prefill keep the separate-norm path.
        fuse_norm = self._fuse_norm_gate(hidden)
        self._ss_valid = False
        if fuse_norm and not getattr(self, "_norm_folded", False):
            self.fold_norm_weights()   # one-time reparameterization
        if self._wpacked and (getattr(self, "_w4", None) is not None
                              or getattr(self, "lora_delta", None) is not None):
            self._drop_packed()        # W4 / LoRA closed the gate for good
        pb = getattr(self, "prev_block", None)
        # the qkv GEMM's split-K combine folds into rope_kv_write: the GEMM
        # hands over its f32 slabs and the combine launch disappears
        # (a _post_qkv override needs combined values: no deferral then)
        defer = (fuse_norm and type(self)._post_qkv is LlamaBlock._post_qkv
                 and ops.fuse_qkv_rope_ok(hidden, self.qkv_w, D))
        if fuse_norm and pb is not None and getattr(pb, "_ss_valid", False):
            # previous block's down-proj left sum-of-squares for `hidden`;
            # norm weight is folded into qkv_w -> invr-only norm (mode 2)
            qkv = ops.linear(hidden, self.qkv_w,
                             norm=(None, cfg.rms_norm_eps),
                             ss_in=pb._ss_hidden, defer_combine=defer,
                             w_packed=self._packed("qkv_w"))
        elif defer:
            x = ops.rms_norm(hidden, self.input_norm_w, cfg.rms_norm_eps)
            qkv = ops.linear(x, self.qkv_w, defer_combine=True,
                             w_packed=self._packed("qkv_w"))
        else:
            x = ops.rms_norm(hidden, self.input_norm_w, cfg.rms_norm_eps)
            qkv = self._lin(x, self.qkv_w, "qkv_w")        # (B, T, (Hq+2Hkv)D)
        if not defer:   # deferral implies the no-op hook
            qkv = self._post_qkv(qkv, B, T)
        cos, sin = self.rope.get(hidden.device)
        kp = kv.k_pages(self.layer_index)
        vp = kv.v_pages(self.layer_index)
        pt = kv.page_table()
        position_ids = rotary_positions(kv, start_pos, position_ids, T)
        # fused RoPE + paged KV write on the raw GEMM output, then attention
        # reads q in place and emits the O-projection input — no transposes
        ctx_lens = None   # start_pos + T, a by-product of the fused launch
        if defer and qkv.dtype == torch.float32:
            # uncombined split-K slabs: combine + RoPE + page write in one
            # launch; only the q section of the returned buffer is filled
            qkv, ctx_lens = ops.rope_kv_write_part(
                qkv, None, B, T, Hq, Hkv, cos, sin, position_ids, kp, vp, pt,
                start_pos)
        else:
            ops.rope_kv_write_(qkv, Hq, Hkv, cos, sin, position_ids, kp, vp,
                               pt, start_pos)
        attn = paged_attention_qkv(qkv, kv, self.layer_index, start_pos, Hq,
                                   Hkv, self.scale, tree_mask=tree_mask,
                                   ctx_lens=ctx_lens)
        if fuse_norm:
            # h2 = hidden + o(attn) via the GEMM's residual epilogue, which
            # also emits row sum-of-squares; the post-attention rmsnorm
            # folds into the gate_up A-stage consuming them. down-proj
            # leaves the stats for the NEXT block's input norm.
            self._ensure_ss_bufs(hidden.device)
            st = H // 64
            h2 = ops.linear(attn, self.o_w, residual=hidden,
                            ss_out=self._ss_h2,
                            cnt=(self._splitk_cnt[:st]
                                 if ops.inlaunch_combine_ok(attn, self.o_w, "o")
                                 else None),
                            w_packed=self._packed("o_w"))
            # SwiGLU rides the gate_up GEMM's epilogue where available
            # (ops.linear_swiglu falls back to linear + swiglu, same bits)
            act = ops.linear_swiglu(h2, self.gate_up_w,
                                    norm=(None, cfg.rms_norm_eps),
                                    ss_in=self._ss_h2,
                                    w_packed=(self._packed("gate_up_w", True)
                                              if ops.fuse_swiglu_ok(
                                                  h2, self.gate_up_w)
                                              else None))
            out = ops.linear(act, self.down_w, residual=h2,
                             ss_out=self._ss_hidden,
                             cnt=(self._splitk_cnt[st:]
                                  if ops.inlaunch_combine_ok(act, self.down_w,
                                                             "down")
                                  else None),
                             w_packed=self._packed("down_w"))
            self._ss_valid = True
            return out
        a = self._lin(attn, self.o_w, "o_w")

        # h2 = hidden + a fused into the post-attention norm
        h2, y = ops.rms_norm_residual(a, hidden, self.post_norm_w, cfg.rms_norm_eps)
        # residual add fused into the down-projection epilogue
        return self._lin(ops.swiglu(self._lin(y, self.gate_up_w, "gate_up_w")),
                         self.down_w, "down_w", residual=h2)

    # ------------------------------------------------------------------
    # training path (differentiable; full sequence, no KV cache)
    # ------------------------------------------------------------------
    def forward_train(self, hidden: torch.Tensor, start_pos: int = 0) -> torch.Tensor:
        eps = self.config.rms_norm_eps

        def lin(x_, w, name):
            # training path honors active LoRA adapters too (the inference
            # path routes through self._lin; keep both consistent)
            y = F.linear(x_, w)
            ld = getattr(self, "lora_delta", None)
            if ld is not None:
                d = ld(name, x_)
                if d is not None:
                    y = y + d
            return y

        x = rms_train(hidden, self.input_norm_w, eps)
        q, k, v = split_heads(lin(x, self.qkv_w, "qkv_w"), self.Hq, self.Hkv,
                              self.D)
        q, k = self._post_qkv_train(q, k)
        attn = rope_attn_train(q, k, v, self.rope, start_pos, self.scale)
        h2 = hidden + lin(attn, self.o_w, "o_w")
        y = rms_train(h2, self.post_norm_w, eps)
        return h2 + swiglu_mlp_train(y, self.gate_up_w, self.down_w)
