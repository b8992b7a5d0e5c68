"""Ring-attention context parallelism (beyond the reference — SURVEY §2.7
marks sequence/context parallel ABSENT there, with xGMI ring attention noted
as the natural MI355X extension): the sequence is sharded across the ranks
of a group, each rank holds Q/K/V for its contiguous shard, and K/V blocks
rotate around the ring (isend/irecv pairs — point-to-point xGMI traffic,
one dedicated link per neighbor) while every rank folds each arriving block
into its online-softmax state. Causality: rank r folds only source shards
<= r, with the triangular mask applied on the diagonal shard.

The fold is the flash-attention (m, l, acc) merge in fp32, so the result
matches single-device attention to numerical tolerance regardless of ring
size.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.distributed as dist


def _fold(state, s, v, row_pos=None, col_pos=None, window: int = 0):
    """Fold one score block into the online-softmax state.

    state: (m, l, acc) with m,l (B,H,T,1) and acc (B,H,T,D), all fp32.
    s: (B,H,T,S) scores; v: (B,H,S,D). If row_pos/col_pos given, mask
    s[t, c] where col_pos[c] > row_pos[t] (causal); window > 0 adds the
    sliding lower bound col_pos[c] > row_pos[t] - window (gemma-4
    alternating sliding layers)."""
    m, l, acc = state
    if row_pos is not None:
        cp = col_pos.view(1, 1, 1, -1)
        rp = row_pos.view(1, 1, -1, 1)
        dead = cp > rp
        if window > 0:
            dead = dead | (cp <= rp - window)
        s = s.masked_fill(dead, float("-inf"))
    m_new = torch.maximum(m, s.amax(-1, keepdim=True))
    # fully-masked rows keep m = -inf; exp(-inf - -inf) guards below
    m_safe = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
    p = torch.exp(s - m_safe)
    if row_pos is not None:
        p = p.masked_fill(dead, 0.0)
    corr = torch.exp(torch.where(torch.isinf(m), m_new.new_zeros(()), m - m_safe))
    corr = torch.where(torch.isinf(m), torch.zeros_like(corr), corr)
    l = l * corr + p.sum(-1, keepdim=True)
    acc = acc * corr + p @ v
    return (m_new, l, acc)


def _ring_exchange(t: torch.Tensor, rank: int, world: int,
                   group=None) -> torch.Tensor:
    """Send t to (rank+1) % world, receive the previous rank's tensor.
    rank/world are GROUP-local; p2p dst/src take GLOBAL ranks, so when the
    group is not the world (pp x cp stages) they must be translated —
    passing local ranks only works for the rank-0-based group."""
    t = t.contiguous()
    out = torch.empty_like(t)
    nxt, prv = (rank + 1) % world, (rank - 1) % world
    if group is not None:
        nxt = dist.get_global_rank(group, nxt)
        prv = dist.get_global_rank(group, prv)
    send = dist.isend(t, nxt, group=group)
    recv = dist.irecv(out, prv, group=group)
    send.wait()
    recv.wait()
    return out


def ring_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                   rank: int, world: int, group=None,
                   scale: Optional[float] = None) -> torch.Tensor:
    """Causal attention over a sequence sharded as contiguous T_loc blocks.

    q/k/v: (B, H, T_loc, D) — this rank's shard (global positions
    [rank*T_loc, (rank+1)*T_loc)). Returns (B, H, T_loc, D)."""
    B, H, T, D = q.shape
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    qf = q.float()
    state = (torch.full((B, H, T, 1), float("-inf")),
             torch.zeros(B, H, T, 1),
             torch.zeros(B, H, T, D))
    row_pos = torch.arange(rank * T, (rank + 1) * T)
    k_cur, v_cur = k.float(), v.float()
    src = rank
    for step in range(world):
        if src < rank:
            s = (qf @ k_cur.transpose(-1, -2)) * scale
            state = _fold(state, s, v_cur)
        elif src == rank:
            s = (qf @ k_cur.transpose(-1, -2)) * scale
            col_pos = torch.arange(src * T, (src + 1) * T)
            state = _fold(state, s, v_cur, row_pos, col_pos)
        # else: future shard — causally invisible, just keep rotating
        if step < world - 1:
            k_cur = _ring_exchange(k_cur, rank, world, group)
            v_cur = _ring_exchange(v_cur, rank, world, group)
            src = (src - 1) % world
    m, l, acc = state
    return (acc / l.clamp_min(1e-30)).to(q.dtype)


def ring_attention_local(q, k, v, world: int,
                         scale: Optional[float] = None) -> torch.Tensor:
    """Single-process simulation of the ring over `world` shards (unit-tests
    the fold/rotation logic at any depth without process groups).

    q/k/v: (B, H, T_total, D) with world | T_total. Returns full output."""
    B, H, T, D = q.shape
    Tl = T // world
    outs = []
    for r in range(world):
        qr = q[:, :, r * Tl:(r + 1) * Tl].float()
        if scale is None:
            sc = 1.0 / math.sqrt(D)
        else:
            sc = scale
        state = (torch.full((B, H, Tl, 1), float("-inf")),
                 torch.zeros(B, H, Tl, 1),
                 torch.zeros(B, H, Tl, D))
        row_pos = torch.arange(r * Tl, (r + 1) * Tl)
        # same visitation order as the ring: own shard first, then r-1, ...
        for src in [r] + [(r - 1 - i) % world for i in range(world - 1)]:
            if src > r:
                continue
            kc = k[:, :, src * Tl:(src + 1) * Tl].float()
            vc = v[:, :, src * Tl:(src + 1) * Tl].float()
            s = (qr @ kc.transpose(-1, -2)) * sc
            if src == r:
                col_pos = torch.arange(src * Tl, (src + 1) * Tl)
                state = _fold(state, s, vc, row_pos, col_pos)
            else:
                state = _fold(state, s, vc)
        m, l, acc = state
        outs.append((acc / l.clamp_min(1e-30)).to(q.dtype))
    return torch.cat(outs, dim=2)


@torch.no_grad()
def cp_prefill_llama(stack, kv_handle, hidden_shard: torch.Tensor,
                     rank: int, world: int, group=None) -> torch.Tensor:
    """Context-parallel ONE-SHOT prefill of a llama BlockStack (the serve
    wiring for ring attention — ROUND2 item 8): the prompt's T_total =
    world * T_loc tokens are sharded contiguously across the group; each
    rank computes its shard's activations with ring attention (K/V blocks
    rotate at Hkv width over xGMI and are GQA-expanded locally per fold),
    and every layer's full K/V is all-gathered into THIS rank's paged pool
    so decode proceeds locally afterwards (stage groups replicate decode
    compute — PipelineStage tp_mode="context").

    hidden_shard: (B, T_loc, H) embeddings of tokens
    [rank*T_loc, (rank+1)*T_loc). The caller must have extended kv_handle
    by T_total from position 0. Returns the rank's output hidden shard.
    """
    import torch.nn.functional as F

    from bloombee_amd import ops
    from bloombee_amd.models.block_common import rms_train
    from bloombee_amd.ops import reference as refops

    cfg = stack.config
    B, T_loc, H = hidden_shard.shape
    dev = hidden_shard.device
    hidden = hidden_shard

    eps = cfg.rms_norm_eps
    for blk in stack.blocks:
        if not (hasattr(blk, "qkv_w") and hasattr(blk, "gate_up_w")):
            raise NotImplementedError(
                "cp_prefill_llama supports llama-pattern blocks")
        Hq, Hkv, D = blk.Hq, blk.Hkv, blk.D
        G = Hq // Hkv
        x = rms_train(hidden, blk.input_norm_w, eps)
        qkv = (F.linear(x, blk.qkv_w).view(B, T_loc, Hq + 2 * Hkv, D)
               .permute(0, 2, 1, 3))
        q, k, v = qkv.split([Hq, Hkv, Hkv], dim=1)
        if hasattr(blk, "q_norm_w"):
            # qwen3-pattern: per-head RMS on raw q/k before RoPE (rms_train
            # normalizes over the last dim = D, weight (D,))
            q = rms_train(q, blk.q_norm_w, eps)
            k = rms_train(k, blk.k_norm_w, eps)
        cos, sin = blk.rope.get(dev)
        pos = (torch.arange(rank * T_loc, (rank + 1) * T_loc, device=dev)
               .view(1, T_loc).expand(B, T_loc))
        q, k = refops.rope_apply(q.contiguous(), k.contiguous(), cos, sin, pos)

        # ring attention with Hkv-width exchange, GQA expansion per fold
        qf = q.float()
        state = (torch.full((B, Hq, T_loc, 1), float("-inf")),
                 torch.zeros(B, Hq, T_loc, 1),
                 torch.zeros(B, Hq, T_loc, D))
        row_pos = torch.arange(rank * T_loc, (rank + 1) * T_loc)
        k_cur = k.float().contiguous()
        v_cur = v.float().contiguous()
        src = rank
        for step in range(world):
            if src <= rank:
                kx = k_cur.repeat_interleave(G, dim=1)
                vx = v_cur.repeat_interleave(G, dim=1)
                s = (qf @ kx.transpose(-1, -2)) * blk.scale
                if src == rank:
                    col_pos = torch.arange(src * T_loc, (src + 1) * T_loc)
                    state = _fold(state, s, vx, row_pos, col_pos)
                else:
                    state = _fold(state, s, vx)
            if step < world - 1:
                k_cur = _ring_exchange(k_cur, rank, world, group)
                v_cur = _ring_exchange(v_cur, rank, world, group)
                src = (src - 1) % world
        m, l, acc = state
        attn = ((acc / l.clamp_min(1e-30)).to(hidden.dtype)
                .permute(0, 2, 1, 3).reshape(B, T_loc, Hq * D))

        h2 = hidden + F.linear(attn, blk.o_w)
        y = rms_train(h2, blk.post_norm_w, eps)
        gu = F.linear(y, blk.gate_up_w)
        g, u = gu.split([gu.shape[-1] // 2] * 2, dim=-1)
        hidden = h2 + F.linear(
            torch.nn.functional.silu(g.float()).to(u.dtype) * u, blk.down_w)

        # full-sequence K/V into the local paged pool (decode runs locally)
        if world > 1:
            k = k.contiguous()
            v = v.contiguous()
            ks = [torch.empty_like(k) for _ in range(world)]
            vs = [torch.empty_like(v) for _ in range(world)]
            import torch.distributed as dist
            dist.all_gather(ks, k, group=group)
            dist.all_gather(vs, v, group=group)
            k_full = torch.cat(ks, dim=2)
            v_full = torch.cat(vs, dim=2)
        else:
            k_full, v_full = k, v
        ops.kv_write(k_full.to(cfg.dtype), v_full.to(cfg.dtype),
                     kv_handle.k_pages(blk.layer_index),
                     kv_handle.v_pages(blk.layer_index),
                     kv_handle.page_table(),
                     torch.zeros(B, dtype=torch.int32, device=dev))
    return hidden


def cp_prefill_gemma4(stack, kv_handle, hidden_shard: torch.Tensor,
                      rank: int, world: int, group=None) -> torch.Tensor:
    """Context-parallel one-shot prefill for a gemma-4 BlockStack: same
    ring structure as cp_prefill_llama but with the family's specifics —
    (1+w) rms norms, separate q/k/v projections with optional k==v and
    shared-KV donor tail layers, per-layer partial rotary tables, per-layer
    sliding window (ring folds carry the window lower bound), scale=1.0
    scores and a gelu-tanh MLP with post-norms. Donor layers keep their
    post-rope K/V shard so tail layers re-rotate the SAME tensors through
    the ring; only donor layers all-gather into the paged pool."""
    import torch.nn.functional as F

    from bloombee_amd import ops
    from bloombee_amd.models.gemma4.block import (_rms1p, _rms1p_headdim,
                                                  _rope_partial)

    cfg = stack.config
    B, T_loc, H = hidden_shard.shape
    dev = hidden_shard.device
    hidden = hidden_shard
    donor_kv = {}

    for blk in stack.blocks:
        eps = blk.config.rms_norm_eps
        Hq, Hkv, D = blk.Hq, blk.Hkv, blk.D
        G = Hq // Hkv
        cos, sin = blk._tables(dev)
        pos = (torch.arange(rank * T_loc, (rank + 1) * T_loc, device=dev)
               .view(1, T_loc).expand(B, T_loc).long())

        x = _rms1p(hidden, blk.input_norm_w, eps)
        q = (F.linear(x, blk.q_w).view(B, T_loc, Hq, D)
             .permute(0, 2, 1, 3))
        q = _rms1p_headdim(q, blk.q_norm_w, eps)
        q = _rope_partial(q, cos, sin, pos, blk.rot_dim).contiguous()

        if blk.donor is None:
            kraw = (F.linear(x, blk.k_w).view(B, T_loc, Hkv, D)
                    .permute(0, 2, 1, 3))
            k = _rms1p_headdim(kraw, blk.k_norm_w, eps)
            k = _rope_partial(k, cos, sin, pos, blk.rot_dim).contiguous()
            if blk.v_w is not None:
                vraw = (F.linear(x, blk.v_w).view(B, T_loc, Hkv, D)
                        .permute(0, 2, 1, 3))
            else:
                vraw = kraw                      # attention_k_eq_v
            v = _rms1p_headdim(vraw, None, eps).contiguous()
            donor_kv[blk.global_index] = (k, v)
            write_layer = blk.layer_index
        else:
            if blk.donor not in donor_kv:
                raise RuntimeError(
                    f"gemma-4 shared-KV layer {blk.global_index} requires "
                    f"donor {blk.donor} in the same stage for CP prefill")
            k, v = donor_kv[blk.donor]           # shared-KV tail
            write_layer = None

        state = (torch.full((B, Hq, T_loc, 1), float("-inf")),
                 torch.zeros(B, Hq, T_loc, 1),
                 torch.zeros(B, Hq, T_loc, D))
        row_pos = torch.arange(rank * T_loc, (rank + 1) * T_loc)
        win = blk.window
        k_cur = k.float().contiguous()
        v_cur = v.float().contiguous()
        src = rank
        qf = q.float()
        for step in range(world):
            if src <= rank:
                kx = k_cur.repeat_interleave(G, dim=1)
                vx = v_cur.repeat_interleave(G, dim=1)
                s = qf @ kx.transpose(-1, -2)    # gemma scale = 1.0
                col_pos = torch.arange(src * T_loc, (src + 1) * T_loc)
                if src == rank or win > 0:
                    state = _fold(state, s, vx, row_pos, col_pos, window=win)
                else:
                    state = _fold(state, s, vx)
            if step < world - 1:
                k_cur = _ring_exchange(k_cur, rank, world, group)
                v_cur = _ring_exchange(v_cur, rank, world, group)
                src = (src - 1) % world
        m, l, acc = state
        attn = ((acc / l.clamp_min(1e-30)).to(hidden.dtype)
                .permute(0, 2, 1, 3).reshape(B, T_loc, Hq * D))

        a = F.linear(attn, blk.o_w)
        a = _rms1p(a, blk.post_attn_norm_w, eps)
        h = hidden + a
        y = _rms1p(h, blk.pre_ffn_norm_w, eps)
        gu = F.linear(y, blk.gate_up_w)
        g, u = gu.split([blk.I, blk.I], dim=-1)
        m_ = F.linear(ops.gelu_tanh(g) * u, blk.down_w)
        hidden = h + _rms1p(m_, blk.post_ffn_norm_w, eps)

        if write_layer is not None:
            if world > 1:
                ks = [torch.empty_like(k) for _ in range(world)]
                vs = [torch.empty_like(v) for _ in range(world)]
                dist.all_gather(ks, k, group=group)
                dist.all_gather(vs, v, group=group)
                k_full = torch.cat(ks, dim=2)
                v_full = torch.cat(vs, dim=2)
            else:
                k_full, v_full = k, v
            ops.kv_write(k_full.to(cfg.dtype), v_full.to(cfg.dtype),
                         kv_handle.k_pages(write_layer),
                         kv_handle.v_pages(write_layer),
                         kv_handle.page_table(),
                         torch.zeros(B, dtype=torch.int32, device=dev))
    return hidden
