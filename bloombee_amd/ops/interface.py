"""Dispatch layer between the gfx950 HIP extension and the torch reference.

CPU tensors run the fp32 reference (bloombee_amd/ops/reference.py); device
tensors run the in-tree _hip_ops extension and FAIL LOUDLY if it is absent —
a silent eager fallback on a GPU box would invalidate every GPU test
(the round-end driver records which .so the GPU processes actually load).
"""
from __future__ import annotations

import importlib
import math
import os
from typing import Optional, Tuple

import torch

from bloombee_amd.ops import reference as ref
from bloombee_amd.ops.reference import alibi_slopes as alibi_slopes_for  # noqa: F401
from bloombee_amd.ops.reference import rope_cos_sin  # noqa: F401  (host-side)
from bloombee_amd.utils.logging import get_logger

logger = get_logger(__name__)

try:
    hip_ops = importlib.import_module("bloombee_amd.ops._hip_ops")
    HAVE_HIP_OPS = True
except ImportError as e:  # pragma: no cover
    hip_ops = None
    HAVE_HIP_OPS = False
    _import_error = e


def _require_ext():
    if not HAVE_HIP_OPS:
        raise RuntimeError(
            "bloombee_amd HIP extension is not built but a tensor is on GPU. "
            "Run `python setup.py hip` (PYTORCH_ROCM_ARCH=gfx950). "
            f"Import error was: {_import_error}"
        )


def _on_gpu(t: torch.Tensor) -> bool:
    return t.is_cuda


# ---------------------------------------------------------------------------


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    if _on_gpu(x):
        _require_ext()
        return hip_ops.rms_norm(x.contiguous(), weight.contiguous(), eps)
    return ref.rms_norm(x, weight, eps)


def rms_norm_residual(
    x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5
) -> Tuple[torch.Tensor, torch.Tensor]:
    if _on_gpu(x):
        _require_ext()
        h, y = hip_ops.rms_norm_residual(x.contiguous(), residual.contiguous(),
                                         weight.contiguous(), eps)
        return h, y
    return ref.rms_norm_residual(x, residual, weight, eps)


def layer_norm(x, weight, bias=None, eps: float = 1e-5):
    if _on_gpu(x):
        _require_ext()
        return hip_ops.layer_norm(x.contiguous(), weight.contiguous(),
                                  bias.contiguous() if bias is not None else None, eps)
    return ref.layer_norm(x, weight, bias, eps)


def rope_apply_(q, k, cos, sin, position_ids):
    """In-place RoPE on q, k: (B, H*, T, D). position_ids: (B, T) int32."""
    if _on_gpu(q):
        _require_ext()
        hip_ops.rope_apply_(q, k, cos, sin, position_ids.int())
        return q, k
    q2, k2 = ref.rope_apply(q, k, cos, sin, position_ids)
    q.copy_(q2)
    k.copy_(k2)
    return q, k


def swiglu(gate_up: torch.Tensor) -> torch.Tensor:
    """gate_up: (..., 2I) from the fused gate/up GEMM -> (..., I)."""
    if _on_gpu(gate_up):
        _require_ext()
        return hip_ops.swiglu(gate_up.contiguous())
    I = gate_up.shape[-1] // 2
    return ref.swiglu(gate_up[..., :I], gate_up[..., I:])


def gelu_tanh(x: torch.Tensor) -> torch.Tensor:
    if _on_gpu(x):
        _require_ext()
        return hip_ops.gelu_tanh(x.contiguous())
    return ref.gelu_tanh(x)


def kv_write(k_new, v_new, k_pages, v_pages, page_table, start_pos):
    if _on_gpu(k_new):
        _require_ext()
        hip_ops.kv_write(k_new.contiguous(), v_new.contiguous(), k_pages, v_pages,
                         page_table, start_pos.int())
        return
    ref.kv_write(k_new, v_new, k_pages, v_pages, page_table, start_pos)


def kv_gather(k_pages, v_pages, page_table, ctx_len: int, batch_index: int):
    if _on_gpu(k_pages):
        _require_ext()
        k, v = hip_ops.kv_gather(k_pages, v_pages, page_table, batch_index, ctx_len)
        return k, v
    return ref.kv_gather(k_pages, v_pages, page_table, ctx_len, batch_index)


_attn_sparsity = 1.0  # Policy.attn_sparsity (ref flexgen policy :10-55)
# fused tree-mask attention: default ON since round 2 (numerics validated
# on MI355X — tests/test_treekernel.py 3/3 after the bool-dispatch fix);
# BBAMD_TREE_KERNEL=0 falls back to the torch composition
_TREE_KERNEL = os.environ.get("BBAMD_TREE_KERNEL", "1") not in ("", "0")


def set_attn_sparsity(frac: float) -> None:
    """Enable top-k sparse decode attention globally (parity: reference
    Policy.attn_sparsity — a server-wide policy knob, not per-call). frac
    is the fraction of cache positions whose V rows participate; 1.0
    restores exact dense attention.

    Per query head the ceil(frac * ctx) highest-scoring positions are kept
    (ties at the threshold go to the lowest positions) and the softmax is
    renormalised over them; ref.attn_paged_topk is the definition. It applies
    to single-token decode through attn_decode / attn_paged (Tq == 1) and
    attn_paged_qkv (T == 1), i.e. to every model family, ALiBi included.
    Device tensors run the gfx950 kernels (attn_sparse.hip: no host sync,
    graph-capturable) for head dims 64 / 128 / 256 at page size 16, and the
    per-row torch composition otherwise; CPU tensors run the reference.

    Dense stays dense everywhere else:
      * frac == 1.0 (the default),
      * sliding-window layers (window > 0),
      * prefill and tree / speculative verify (Tq > 1 or a tree_mask),
      * mixed-device decode with a host-resident prefix
        (attn_paged_mixed / attn_paged_mixed_qkv).
    """
    global _attn_sparsity
    _attn_sparsity = float(frac)


# top-k sparse decode on the GPU: attn_sparse.hip (scores / select / P.V);
# BBAMD_SPARSE_KERNEL=0 falls back to the per-row torch composition
# (ref.attn_paged_topk on the device tensors: one host sync per batch row)
_SPARSE_KERNEL = os.environ.get("BBAMD_SPARSE_KERNEL", "1") not in ("", "0")


def _sparse_kernel_ok(D: int, P: int) -> bool:
    # head dims and the page size (BBAMD_KV_PAGE_SIZE default) the sparse
    # kernels cover; any GQA/MQA group width (groups wider than 16 are
    # chunked in-kernel). Everything else runs the composition.
    return _SPARSE_KERNEL and D in (64, 128, 256) and P == 16


def _alibi_on(alibi_slopes, dev):
    """The slopes as the kernels take them: contiguous f32 on dev, or None."""
    if alibi_slopes is None:
        return None
    return alibi_slopes.float().to(dev).contiguous()


def _window_or_none(window: int):
    return window if window > 0 else None


def attn_decode(
    q, k_pages, v_pages, page_table, ctx_lens, scale: Optional[float] = None,
    window: int = 0, n_split: int = 0, alibi_slopes=None,
) -> torch.Tensor:
    """Single-token paged attention. q: (B, Hq, 1, D)."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if _attn_sparsity < 1.0 and window <= 0:
        if _on_gpu(q) and _sparse_kernel_ok(q.shape[-1], k_pages.shape[2]):
            _require_ext()
            al = _alibi_on(alibi_slopes, q.device)
            return hip_ops.attn_decode_sparse(
                q.contiguous(), k_pages, v_pages, page_table, ctx_lens.int(),
                _attn_sparsity, scale, al)
        return ref.attn_paged_topk(q, k_pages, v_pages, page_table, ctx_lens,
                                   _attn_sparsity, scale,
                                   alibi_slopes=alibi_slopes)
    if _on_gpu(q):
        _require_ext()
        if q.shape[-1] > 256 and q.shape[-1] != 512:
            # odd wide head dims: gather-based torch composition on-device
            # (D=512 runs attn_decode_wide_kernel — d split across waves)
            return ref.attn_paged(q, k_pages, v_pages, page_table,
                                  ctx_lens.long() - 1, scale,
                                  sliding_window=_window_or_none(window),
                                  alibi_slopes=alibi_slopes)
        al = _alibi_on(alibi_slopes, q.device)
        return hip_ops.attn_decode(q.contiguous(), k_pages, v_pages, page_table,
                                   ctx_lens.int(), scale, window, n_split, al)
    q_start = ctx_lens.long() - 1
    return ref.attn_paged(q, k_pages, v_pages, page_table, q_start, scale,
                          sliding_window=_window_or_none(window),
                          alibi_slopes=alibi_slopes)


def attn_prefill(
    q, k_pages, v_pages, page_table, q_start, scale: Optional[float] = None,
    window: int = 0, alibi_slopes=None,
) -> torch.Tensor:
    """Multi-token causal paged attention. q: (B, Hq, Tq, D); the new tokens'
    K/V must already be in the pages (kv_write first)."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if _on_gpu(q):
        _require_ext()
        if q.shape[-1] > 256:
            return ref.attn_paged(q, k_pages, v_pages, page_table,
                                  q_start.long(), scale,
                                  sliding_window=_window_or_none(window),
                                  alibi_slopes=alibi_slopes)
        al = _alibi_on(alibi_slopes, q.device)
        return hip_ops.attn_prefill(q.contiguous(), k_pages, v_pages, page_table,
                                    q_start.int(), scale, window, al, None)
    return ref.attn_paged(q, k_pages, v_pages, page_table, q_start, scale,
                          sliding_window=_window_or_none(window),
                          alibi_slopes=alibi_slopes)


def rope_kv_write_(qkv, Hq: int, Hkv: int, cos, sin, position_ids,
                   k_pages, v_pages, page_table, start_pos):
    """Fused RoPE + paged KV write on the raw QKV GEMM output.

    qkv: (B, T, (Hq+2Hkv)*D) — q section roped in place; k roped -> pages;
    v copied -> pages. position_ids None => start_pos[b] + t.
    """
    if _on_gpu(qkv):
        _require_ext()
        hip_ops.rope_kv_write_(qkv, Hq, Hkv, cos, sin,
                               position_ids.int() if position_ids is not None else None,
                               k_pages, v_pages, page_table, start_pos.int())
        return
    B, T, _ = qkv.shape
    D = k_pages.shape[3]
    q = qkv[..., : Hq * D].view(B, T, Hq, D).permute(0, 2, 1, 3)
    k = qkv[..., Hq * D:(Hq + Hkv) * D].view(B, T, Hkv, D).permute(0, 2, 1, 3)
    v = qkv[..., (Hq + Hkv) * D:].view(B, T, Hkv, D).permute(0, 2, 1, 3)
    if position_ids is None:
        position_ids = start_pos.view(B, 1).long() + torch.arange(T).view(1, T)
    q2, k2 = ref.rope_apply(q, k, cos, sin, position_ids)
    qkv[..., : Hq * D].copy_(q2.permute(0, 2, 1, 3).reshape(B, T, Hq * D))
    ref.kv_write(k2, v.contiguous(), k_pages, v_pages, page_table, start_pos)


def rope_kv_write_part(part, bias, B: int, T: int, Hq: int, Hkv: int, cos, sin,
                       position_ids, k_pages, v_pages, page_table, start_pos):
    """rope_kv_write_ on the QKV GEMM's uncombined split-K output.

    part: f32 (ksplit, B*T, (Hq+2Hkv)*D) from linear(defer_combine=True); the
    kernel sums the slabs in split order (+bias), rounds once to bf16 — the
    value the combine kernel would have stored — and ropes / page-writes it.
    Returns the bf16 (B, T, (Hq+2Hkv)*D) buffer with the q section roped —
    its k and v sections are NOT written (they live in the pages only) — and
    the (B,) int32 context lengths start_pos + T, which attn_paged_qkv takes
    as ctx_lens at T == 1 instead of launching its own start_pos + 1."""
    _require_ext()
    return hip_ops.rope_kv_write_part(
        part, bias, B, T, Hq, Hkv, cos, sin,
        position_ids.int() if position_ids is not None else None,
        k_pages, v_pages, page_table, start_pos.int())


def attn_paged_qkv(qkv, Hq: int, Hkv: int, k_pages, v_pages, page_table,
                   q_start, scale=None, window: int = 0, ctx_lens=None):
    """Attention reading q straight from the fused QKV buffer.

    qkv: (B, T, (Hq+2Hkv)*D) with the q section already roped and the new
    tokens' K/V already in the pages (rope_kv_write_ first).
    ctx_lens: optional precomputed q_start + 1 for single-token decode
    (rope_kv_write_part's second result).
    Returns (B, T, Hq*D) — the O-projection GEMM input, no transposes.
    """
    B, T, _ = qkv.shape
    D = k_pages.shape[3]
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    if _attn_sparsity < 1.0 and T == 1 and window <= 0:
        ctx = ctx_lens if ctx_lens is not None else q_start + 1
        if (_on_gpu(qkv) and _sparse_kernel_ok(D, k_pages.shape[2])
                and qkv.is_contiguous()):
            _require_ext()
            return hip_ops.attn_decode_sparse_qkv(
                qkv, Hq, k_pages, v_pages, page_table, ctx.int(),
                _attn_sparsity, scale)
        q = qkv[..., : Hq * D].view(B, T, Hq, D).permute(0, 2, 1, 3).contiguous()
        out = ref.attn_paged_topk(q, k_pages, v_pages, page_table, ctx,
                                  _attn_sparsity, scale)
        return out.permute(0, 2, 1, 3).reshape(B, T, Hq * D)
    if _on_gpu(qkv):
        _require_ext()
        if T == 1:
            ctx = ctx_lens if ctx_lens is not None else q_start + 1
            return hip_ops.attn_decode_qkv(qkv, Hq, k_pages, v_pages, page_table,
                                           ctx.int(), scale, window, 0)
        return hip_ops.attn_prefill_qkv(qkv, Hq, k_pages, v_pages, page_table,
                                        q_start.int(), scale, window)
    q = qkv[..., : Hq * D].view(B, T, Hq, D).permute(0, 2, 1, 3).contiguous()
    out = ref.attn_paged(q, k_pages, v_pages, page_table, q_start.long(), scale,
                         sliding_window=_window_or_none(window))
    return out.permute(0, 2, 1, 3).reshape(B, T, Hq * D)


def attn_paged(q, k_pages, v_pages, page_table, q_start, scale=None, window: int = 0,
               tree_mask=None, alibi_slopes=None):
    """Unified entry: picks decode vs prefill kernel by Tq."""
    Tq = q.shape[2]
    sparse_decode = (_attn_sparsity < 1.0 and Tq == 1 and tree_mask is None
                     and window <= 0)
    if alibi_slopes is not None and not _on_gpu(q) and not sparse_decode:
        if scale is None:
            scale = 1.0 / math.sqrt(q.shape[-1])
        return ref.attn_paged(q, k_pages, v_pages, page_table, q_start, scale,
                              alibi_slopes=alibi_slopes,
                              sliding_window=_window_or_none(window))
    if tree_mask is not None:
        if scale is None:
            scale = 1.0 / math.sqrt(q.shape[-1])
        if (_on_gpu(q) and _TREE_KERNEL and window == 0
                and q.shape[-1] <= 256 and alibi_slopes is None):
            # fused tree-mask prefill kernel (spec verify) — the default
            # GPU path (tests/test_treekernel.py parity on MI355X)
            _require_ext()
            tm = tree_mask.to(q.device).contiguous().bool()
            return hip_ops.attn_prefill(q.contiguous(), k_pages, v_pages,
                                        page_table, q_start.int(), scale, 0,
                                        None, tm)
        # tree-attention (spec decode verify): device-agnostic torch
        # composition (ref.attn_paged runs on GPU tensors directly)
        return ref.attn_paged(q, k_pages, v_pages, page_table,
                              q_start.to(q.device), scale,
                              tree_mask=tree_mask.to(q.device))
    if Tq == 1:
        ctx_lens = q_start + 1
        return attn_decode(q, k_pages, v_pages, page_table, ctx_lens, scale,
                           window, alibi_slopes=alibi_slopes)
    return attn_prefill(q, k_pages, v_pages, page_table, q_start, scale, window,
                        alibi_slopes=alibi_slopes)


def linear(x: torch.Tensor, w: torch.Tensor, residual: Optional[torch.Tensor] = None,
           bias: Optional[torch.Tensor] = None,
           norm: Optional[tuple] = None,
           ss_in: Optional[torch.Tensor] = None,
           ss_out: Optional[torch.Tensor] = None,
           defer_combine: bool = False,
           cnt: Optional[torch.Tensor] = None,
           w_packed: Optional[torch.Tensor] = None,
           w_nt: int = 0) -> torch.Tensor:
    """y = (rmsnorm(x) if norm else x) @ w^T (+bias) (+residual).
    Decode-shaped GEMMs (<=32 rows) on GPU go through the skinny-M MFMA
    kernel (gemm_skinny.hip) — hipBLASLt leaves ~2x weight-stream bandwidth
    on the table at M<=32; everything else uses hipBLASLt via F.linear.
    norm=(weight, eps) folds the input rmsnorm into the kernel's A-operand
    stage (launch-count reduction; the separate rms_norm launch + its
    read/write disappear from the decode step). ss_in is the producing
    GEMM's per-stripe row sum-of-squares (its ss_out) so the fused norm
    skips re-streaming A; ss_out asks this GEMM's epilogue to emit the
    same stats for ITS consumer (f32 (N/64, 32), overwritten — graph-safe).
    defer_combine (callers gate on fuse_qkv_rope_ok): where the kernel splits
    K, return its f32 slabs (ksplit, M, N) WITHOUT bias instead of y, for
    rope_kv_write_part to fold; an unsplit GEMM still returns y (bf16).
    cnt (callers gate on inlaunch_combine_ok): int32 zeros, >= N/64 entries —
    a split-K GEMM combines inside its own launch and leaves them zero.
    w_packed: pack_skinny_w(w), the same weight in the order the skinny
    kernel reads it (same bits out); used on the skinny path only, every
    other path ignores it and reads w.
    w_nt: cache policy of the skinny kernel's weight loads for this call, 1
    nontemporal, -1 default, 0 what BBAMD_W_NT says (same bits out)."""
    M = x.numel() // x.shape[-1]
    N, K = w.shape[0], x.shape[-1]
    if w_nt not in (-1, 0, 1):    # on every path, also those that ignore it
        raise RuntimeError(f"w_nt must be 0, 1 or -1, got {w_nt}")
    # All decode-shaped GEMMs route to the skinny kernel: although hipBLASLt
    # wins the two MLP shapes in an isolated microbench, in the real decode
    # step it runs ~1.5x slower (cold L2 / per-stream heuristics, see
    # profiles/), while gemm_skinny runs faster in-context AND fuses the
    # residual/bias epilogue the blaslt path would re-emit as a separate
    # eager kernel.
    if (_on_gpu(x) and M <= 32 and x.dtype == torch.bfloat16
            and K % 256 == 0 and N % 64 == 0):
        _require_ext()
        nw, eps, mode = None, 0.0, 0
        if norm is not None:
            eps = float(norm[1])
            if norm[0] is None:
                mode = 2  # weight pre-folded into W: invr-only scaling
            else:
                nw = norm[0].contiguous()
                mode = 1
        return hip_ops.gemm_skinny(x.contiguous(), w, residual, bias,
                                   _INLAUNCH_KSPLIT if cnt is not None else 0,
                                   nw, eps, ss_in if norm is not None else None,
                                   ss_out, mode, defer_combine, cnt, 0,
                                   w_packed, w_nt)
    if defer_combine or cnt is not None:
        raise RuntimeError("defer_combine / cnt require the GPU skinny-GEMM "
                           "path (callers gate on fuse_norm_linear_ok)")
    if norm is not None:
        nw = norm[0]
        if nw is None:
            nw = torch.ones(x.shape[-1], dtype=x.dtype, device=x.device)
        x = rms_norm(x, nw, norm[1])
    y = torch.nn.functional.linear(x, w, bias)
    if residual is not None:
        y = y + residual.view_as(y)
    if ss_out is not None:
        raise RuntimeError("ss_out requires the GPU skinny-GEMM path "
                           "(callers gate on fuse_norm_linear_ok)")
    return y


_FUSE_NORM = os.environ.get("BBAMD_FUSE_NORM", "1") != "0"


def fuse_norm_linear_ok(x: torch.Tensor, w: torch.Tensor) -> bool:
    """True when linear(norm=...) will take the fused-kernel path (so the
    caller can skip emitting a separate rms_norm). Default ON
    (BBAMD_FUSE_NORM=0 reverts): +2.9% on the flagship decode bench
    (5289 vs 5140 tok/s) once the row stats ride the producer GEMM's
    epilogue and the norm weights are folded into the projections
    (profiles/r02 §13; the naive per-WG A-restream variant measured 16%
    SLOWER — the chain is what makes it pay)."""
    K = x.shape[-1]
    return (_FUSE_NORM and _on_gpu(x) and x.numel() // K <= 32
            and x.dtype == torch.bfloat16 and K % 256 == 0
            and w.shape[0] % 64 == 0 and HAVE_HIP_OPS)


# Fused epilogues of the decode GEMMs (profiles/r03_fused_epilogues.md). Each
# is available only where fuse_norm_linear_ok holds (the llama block's
# _fuse_norm_gate); =0 restores the separate kernels exactly, and the results
# are bit-identical either way.
#   BBAMD_FUSE_SWIGLU    SwiGLU in the gate_up GEMM's epilogue (linear_swiglu)
#   BBAMD_FUSE_QKV_ROPE  qkv split-K combine folded into rope_kv_write
#   BBAMD_INLAUNCH_COMBINE  o-proj / down-proj split-K combine inside the GEMM
#                        launch: "0" none, "1" both, or a list of "o", "down"
_FUSE_SWIGLU = os.environ.get("BBAMD_FUSE_SWIGLU", "1") != "0"
_FUSE_QKV_ROPE = os.environ.get("BBAMD_FUSE_QKV_ROPE", "1") != "0"
_INLAUNCH_DEFAULT = "0"


def _parse_inlaunch(v: str) -> frozenset:
    if v in ("", "0"):
        return frozenset()
    if v == "1":
        return frozenset(("o", "down"))
    return frozenset(x.strip() for x in v.split(",")) & {"o", "down"}


_INLAUNCH_COMBINE = _parse_inlaunch(
    os.environ.get("BBAMD_INLAUNCH_COMBINE", _INLAUNCH_DEFAULT))
# experiment knob for the in-launch ksplit sweep; 0 = the op's own rule
_INLAUNCH_KSPLIT = int(os.environ.get("BBAMD_INLAUNCH_KSPLIT", "0"))


def fuse_swiglu_ok(x: torch.Tensor, gate_up_w: torch.Tensor) -> bool:
    """True when linear_swiglu(x, gate_up_w) runs the fused kernel: the
    fuse_norm_linear_ok shapes, and only where the plain gate_up GEMM would
    not split K. The fused kernel never splits (one f32 accumulator per
    output), so against a split-K gate_up its sums would be ordered
    differently and a few outputs would move by a bf16 ulp; such shapes
    (narrow 2I with K >= 1024) keep the separate kernels."""
    N, K = gate_up_w.shape[0], x.shape[-1]
    return (_FUSE_SWIGLU and fuse_norm_linear_ok(x, gate_up_w)
            and hip_ops.gemm_skinny_plan(N, K, 0)[0] == 1)


def fuse_qkv_rope_ok(x: torch.Tensor, qkv_w: torch.Tensor, D: int) -> bool:
    """True when the qkv GEMM may defer its combine to rope_kv_write_part."""
    return (_FUSE_QKV_ROPE and fuse_norm_linear_ok(x, qkv_w) and D % 8 == 0)


def inlaunch_combine_ok(x: torch.Tensor, w: torch.Tensor, which: str) -> bool:
    """True when linear(cnt=...) may combine split-K inside the launch for
    the projection named `which` ("o" or "down")."""
    return which in _INLAUNCH_COMBINE and fuse_norm_linear_ok(x, w)


def linear_swiglu(x: torch.Tensor, gate_up_w: torch.Tensor,
                  norm: Optional[tuple] = None,
                  ss_in: Optional[torch.Tensor] = None,
                  w_packed: Optional[torch.Tensor] = None,
                  w_nt: int = 0) -> torch.Tensor:
    """act = swiglu((rmsnorm(x) if norm else x) @ gate_up_w^T), gate_up_w the
    fused gate|up weight (2I, K) in its usual layout. Decode shapes on GPU
    run the gate_up GEMM with SwiGLU in its epilogue (one launch, the (M, 2I)
    intermediate never reaches memory); bit-identical to swiglu(linear(...)).
    norm is (None, eps): the weight is pre-folded into gate_up_w.
    w_packed: pack_skinny_w(gate_up_w, swiglu=True), used by the fused kernel
    only (the fallback's plain GEMM pairs rows differently and reads
    gate_up_w). w_nt: as for linear."""
    if w_nt not in (-1, 0, 1):
        raise RuntimeError(f"w_nt must be 0, 1 or -1, got {w_nt}")
    if fuse_swiglu_ok(x, gate_up_w):
        _require_ext()
        assert norm is None or norm[0] is None, \
            "linear_swiglu takes the folded-weight norm only"
        return hip_ops.gemm_skinny_swiglu(
            x.contiguous(), gate_up_w,
            float(norm[1]) if norm is not None else 0.0, ss_in,
            2 if norm is not None else 0, 0, w_packed, w_nt)
    return swiglu(linear(x, gate_up_w, norm=norm, ss_in=ss_in, w_nt=w_nt))


def pack_skinny_w(w: torch.Tensor, swiglu: bool = False) -> torch.Tensor:
    """The copy of w (N, K) that linear(w_packed=...) streams, or with
    swiglu=True the one linear_swiglu(w_packed=...) does: 1 KB blocks in the
    skinny kernel's read order (ops/hip/common.h, skinny_packed_offset; the
    layout is defined once more in reference.pack_skinny_w, which this is).
    Runs once per weight, as torch index expressions on w's device."""
    return ref.pack_skinny_w(w, swiglu)


# mixed-device decode on the GPU: device segment on the MFMA decode kernel
# in forced-partial mode + one merge launch (hip_ops.attn_decode_mixed);
# BBAMD_MIXED_KERNEL=0 falls back to the per-row torch composition
_MIXED_KERNEL = os.environ.get("BBAMD_MIXED_KERNEL", "1") not in ("", "0")


def _mixed_kernel_ok(D: int) -> bool:
    # head dims the decode kernels cover (same rule as attn_decode)
    return _MIXED_KERNEL and (D <= 256 or D == 512)


def _attn_mixed_gpu(q_or_qkv, q4, k_pages, v_pages, page_table, ctx_lens,
                    host_k, host_v, scale, window, alibi_slopes, n_split=0):
    """GPU mixed-device decode. q_or_qkv: what the kernel reads q from
    ((B, Hq, 1, D) or the fused QKV buffer); q4: a (B, Hq, 1, D) view of the
    same q for the host copy. Returns (B, 1, Hq*D)."""
    _require_ext()
    B, Hq, _, D = q4.shape
    S_host = host_k.shape[2]
    dev = q4.device
    al = _alibi_on(alibi_slopes, dev)
    lo = 0
    if window > 0:
        # host suffix inside the window, per row (absolute positions)
        lo = (S_host + ctx_lens.long().cpu() - window).clamp_(min=0)
        if int(lo.min()) >= S_host:
            # the window excludes the host prefix entirely: plain decode
            if q_or_qkv.dim() == 3:
                return hip_ops.attn_decode_qkv(
                    q_or_qkv, Hq, k_pages, v_pages, page_table,
                    ctx_lens.int(), scale, window, n_split)
            return (hip_ops.attn_decode(q_or_qkv.contiguous(), k_pages,
                                        v_pages, page_table, ctx_lens.int(),
                                        scale, window, n_split, al)
                    .permute(0, 2, 1, 3).reshape(B, 1, Hq * D))
    # host segment: q crosses to the host, the prefix is attended there in
    # fp32 (the point of the mode), and only the (m, l, acc) partial — one
    # pinned buffer, one H2D copy — comes back
    ml, acc = ref.attn_host_partial(
        q4[:, :, 0].float().cpu(), host_k, host_v, scale, lo,
        alibi_slopes.cpu() if alibi_slopes is not None else None)
    n_ml = B * Hq * 2
    stage = torch.empty(n_ml + B * Hq * D, dtype=torch.float32,
                        pin_memory=True)
    stage[:n_ml].copy_(ml.view(-1))
    stage[n_ml:].copy_(acc.view(-1))
    ext = stage.to(dev, non_blocking=True)
    return hip_ops.attn_decode_mixed(
        q_or_qkv, k_pages, v_pages, page_table, ctx_lens.int(),
        ext[:n_ml].view(B, Hq, 2), ext[n_ml:].view(B, Hq, D),
        scale, window, n_split, al, S_host)


def attn_paged_mixed(q, k_pages, v_pages, page_table, ctx_lens,
                     host_k, host_v, scale=None, window: int = 0,
                     alibi_slopes=None, n_split: int = 0):
    """Mixed-device decode attention: host-resident KV prefix (CPU)
    + device-resident recent segment, merged with the exact log-sum-exp
    composition (ref _mixed_device_attention, pytorch_backend.py:969-1014).
    q: (B, Hq, 1, D); ctx_lens are LOCAL to the device pool. The host
    segment's matmuls RUN on the CPU by construction, which is the point of
    the mode; on GPU tensors the device segment and the merge run on the
    decode kernels (BBAMD_MIXED_KERNEL=0: torch composition); n_split
    (kernel path only) pins the flash-decode split count, 0 = auto."""
    D = q.shape[-1]
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    if _on_gpu(q) and _mixed_kernel_ok(D):
        B, Hq = q.shape[0], q.shape[1]
        out = _attn_mixed_gpu(q.contiguous(), q, k_pages, v_pages, page_table,
                              ctx_lens, host_k, host_v, scale, window,
                              alibi_slopes, n_split)
        return out.view(B, 1, Hq, D).permute(0, 2, 1, 3)
    return ref.attn_paged_mixed(q, k_pages, v_pages, page_table, ctx_lens,
                                host_k, host_v, scale, window=window,
                                alibi_slopes=alibi_slopes)


def attn_paged_mixed_qkv(qkv, Hq: int, Hkv: int, k_pages, v_pages, page_table,
                         ctx_lens, host_k, host_v, scale=None,
                         window: int = 0):
    """attn_paged_mixed reading q straight from the fused QKV buffer
    (B, 1, (Hq+2Hkv)*D), q section already roped, the new token's K/V
    already in the pages. Returns (B, 1, Hq*D) — the O-projection input."""
    B, T, _ = qkv.shape
    assert T == 1, "mixed-device path is decode-only"
    D = k_pages.shape[3]
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    q = qkv[..., : Hq * D].view(B, T, Hq, D).permute(0, 2, 1, 3)
    if _on_gpu(qkv) and _mixed_kernel_ok(D) and qkv.is_contiguous():
        return _attn_mixed_gpu(qkv, q, k_pages, v_pages, page_table, ctx_lens,
                               host_k, host_v, scale, window, None)
    out = ref.attn_paged_mixed(q.contiguous(), k_pages, v_pages, page_table,
                               ctx_lens, host_k, host_v, scale, window=window)
    return out.permute(0, 2, 1, 3).reshape(B, T, Hq * D)


def moe_gemm_grouped(A: torch.Tensor, W: torch.Tensor, off: torch.Tensor,
                     rowmap: Optional[torch.Tensor] = None,
                     scale: Optional[torch.Tensor] = None,
                     S: Optional[int] = None,
                     mchunks: Optional[int] = None) -> torch.Tensor:
    """Grouped expert GEMM, one launch over all experts (moe_gemm.hip):
    C[s] = A[rowmap[s] if rowmap else s] @ W[expert(s)]^T (* scale[s]).

    Slots are expert-sorted: [off[e], off[e+1]) belong to expert e; off is
    the int32 exclusive prefix sum ON DEVICE (no host sync — hipGraph-safe,
    unlike the per-expert nonzero() loop). S = total slots, mchunks = host
    upper bound on ceil(max rows per expert / 32) (worst case: every token
    routed to one expert). Replaces the per-expert skinny GEMM loop for
    Mixtral decode (BASELINE config 4 "MoE grouped GEMM").
    """
    E, N, K = W.shape
    if S is None:
        S = int(rowmap.numel()) if rowmap is not None else int(A.shape[0])
    if mchunks is None:
        mchunks = (int(A.shape[0]) + 31) // 32
    if (_on_gpu(A) and A.dtype == torch.bfloat16 and K % 32 == 0
            and N % 64 == 0):
        _require_ext()
        return hip_ops.moe_gemm(A.contiguous(), W.contiguous(),
                                off.int(), rowmap, scale, S, mchunks)
    return ref.moe_gemm_grouped(A, W, off, rowmap, scale, S)


def moe_gemm_grouped_w4(A: torch.Tensor, packed: torch.Tensor,
                        scale: torch.Tensor, zero: torch.Tensor,
                        off: torch.Tensor,
                        rowmap: Optional[torch.Tensor] = None,
                        slot_scale: Optional[torch.Tensor] = None,
                        S: Optional[int] = None,
                        mchunks: Optional[int] = None) -> torch.Tensor:
    """moe_gemm_grouped over 4-bit expert weights (moe_gemm_w4.hip):
    C[s] = (A[row(s)] @ dequant4(W[expert(s)])^T) (* slot_scale[s]).

    packed (E, N, K/2) u8, scale / zero (E, N, K/64) f16: quant4_pack layout
    with a leading expert dimension. off, rowmap, S and mchunks as for
    moe_gemm_grouped. bf16 device activations with K % 128 == 0 and
    N % 64 == 0 run the kernel, which streams ~3.5x fewer weight bytes and
    computes in f16 (activations outside the f16 range are not supported,
    as for linear_w4). Everything else, and BBAMD_MOE_W4_KERNEL=0 (read per
    call), dequantizes the active experts and uses moe_gemm_grouped."""
    E, N, Kh = packed.shape
    K = Kh * 2
    if S is None:
        S = int(rowmap.numel()) if rowmap is not None else int(A.shape[0])
    if mchunks is None:
        mchunks = (int(A.shape[0]) + 31) // 32
    if (_on_gpu(A) and A.dtype == torch.bfloat16 and K % 128 == 0
            and N % 64 == 0
            and os.environ.get("BBAMD_MOE_W4_KERNEL", "1") != "0"):
        _require_ext()
        return hip_ops.moe_gemm_w4(A.contiguous(), packed.contiguous(),
                                   scale.half().contiguous(),
                                   zero.half().contiguous(), off.int(),
                                   rowmap, slot_scale, S, mchunks, 0)
    if _on_gpu(A):
        # the composition on device: dequantize every expert with the unpack
        # kernel (no host sync on the group sizes) and run the bf16 kernel
        _require_ext()
        W = quant4_unpack(packed.reshape(-1, 32), scale.reshape(-1),
                          zero.reshape(-1)).reshape(E, N, K).to(A.dtype)
        return moe_gemm_grouped(A, W, off, rowmap, slot_scale, S, mchunks)
    return ref.moe_gemm_grouped_w4(A, packed, scale, zero, off, rowmap,
                                   slot_scale, S)


def linear_w4(x: torch.Tensor, packed: torch.Tensor, scale: torch.Tensor,
              zero: torch.Tensor, N: int,
              residual: Optional[torch.Tensor] = None,
              bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x @ dequant4(W)^T (+bias) (+residual) with W in quant4_pack
    layout (N, K/2 codes + f16 scale/zero per 64-group). Decode shapes
    (M<=32) run the 4-bit weight-stream kernel (w4_gemm.hip, ~3.5x less
    HBM traffic than bf16); anything else dequantizes and uses the dense
    path — W4 is a decode-bandwidth play, prefill is compute-bound."""
    K = x.shape[-1]
    M = x.numel() // K
    if (_on_gpu(x) and x.dtype == torch.bfloat16 and M <= 32
            and K % 128 == 0 and N % 64 == 0):
        _require_ext()
        # the kernel computes in f16 (fast nibble->half dequant + f16 MFMA);
        # the activation conversion is M*K elements - noise next to the
        # 4-bit weight stream it unlocks
        return hip_ops.gemm_w4(x.half().contiguous(),
                               packed.reshape(N, K // 2),
                               scale.reshape(N, K // 64).half(),
                               zero.reshape(N, K // 64).half(),
                               residual, bias, N, 0)
    w = quant4_unpack(packed.reshape(-1, 32), scale.reshape(-1),
                      zero.reshape(-1), dtype=x.dtype).reshape(N, K)
    y = torch.nn.functional.linear(x, w, bias)
    if residual is not None:
        y = y + residual.view_as(y)
    return y


def quant4_pack(x: torch.Tensor, group_size: int = 64):
    if _on_gpu(x):
        _require_ext()
        assert group_size == 64
        packed, scale, zero = hip_ops.quant4_pack(x.contiguous())
        return packed, scale, zero
    return ref.quant4_pack(x, group_size)


def quant4_unpack(packed, scale, zero, dtype=torch.bfloat16):
    if _on_gpu(packed):
        _require_ext()
        return hip_ops.quant4_unpack(packed, scale, zero)
    return ref.quant4_unpack(packed, scale, zero, dtype)


def mfma_selftest(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    _require_ext()
    return hip_ops.mfma_selftest(A.contiguous(), B.contiguous())


# ---------------------------------------------------------------------------
# training attention
# ---------------------------------------------------------------------------


class _AttnTrainFn(torch.autograd.Function):
    """Flash forward/backward over ops/hip/attn_train.hip. Saves q, k, v, the
    bf16 output and the per-row LSE; nothing quadratic in T is kept."""

    @staticmethod
    def forward(ctx, q, k, v, scale, window, alibi):
        want = any(ctx.needs_input_grad[:3])
        out, lse = hip_ops.attn_train_fwd(q, k, v, scale, window, alibi, want)
        if want:
            ctx.save_for_backward(q, k, v, out, lse,
                                  alibi if alibi is not None else q.new_empty(0))
            ctx.has_alibi = alibi is not None
            ctx.scale, ctx.window = scale, window
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, alibi = ctx.saved_tensors
        if dout.stride(-1) != 1 or any(s % 8 for s in dout.stride()[:-1]):
            dout = dout.contiguous()
        dq, dk, dv = hip_ops.attn_train_bwd(
            dout, q, k, v, out, lse, ctx.scale, ctx.window,
            alibi if ctx.has_alibi else None)
        return dq, dk, dv, None, None, None


def _train_view_ok(t: torch.Tensor) -> bool:
    return (t.stride(-1) == 1 and all(s % 8 == 0 for s in t.stride()[:-1])
            and t.storage_offset() % 8 == 0)


def attn_train(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float,
               window: int = 0,
               alibi_slopes: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable causal attention for the fine-tuning path.

    q (B, T, Hq, D), k/v (B, T, Hkv, D) -> (B, T, Hq, D); see
    reference.attn_train for the definition. bf16 device tensors with
    D in {64, 128} run the gfx950 kernels (BBAMD_TRAIN_ATTN_KERNEL=0, read
    per call, turns them off); everything else — CPU, fp32, larger D —
    takes the torch composition."""
    D = q.shape[-1]
    if (_on_gpu(q) and q.dtype == torch.bfloat16 and D in (64, 128)
            and os.environ.get("BBAMD_TRAIN_ATTN_KERNEL", "1") != "0"):
        _require_ext()
        q, k, v = (t if _train_view_ok(t) else t.contiguous() for t in (q, k, v))
        alibi = None
        if alibi_slopes is not None:
            alibi = alibi_slopes.detach().to(device=q.device,
                                             dtype=torch.float32).contiguous()
        return _AttnTrainFn.apply(q, k, v, float(scale), int(window), alibi)
    return ref.attn_train(q, k, v, scale, window, alibi_slopes)
