"""Op dispatch: gfx950 HIP kernels on device, pure-torch reference on CPU.

Policy (driver contract): on a GPU box the HIP extension MUST be the path
that runs — if a tensor is on device and the extension is missing, we raise
instead of silently falling back to eager PyTorch.
"""
from bloombee_amd.ops.interface import (  # noqa: F401
    HAVE_HIP_OPS,
    alibi_slopes_for,
    attn_decode,
    attn_paged,
    attn_paged_mixed,
    attn_paged_mixed_qkv,
    attn_paged_qkv,
    attn_prefill,
    attn_train,
    fuse_norm_linear_ok,
    fuse_qkv_rope_ok,
    fuse_swiglu_ok,
    gelu_tanh,
    hip_ops,
    inlaunch_combine_ok,
    kv_gather,
    kv_write,
    layer_norm,
    linear,
    linear_swiglu,
    linear_w4,
    mfma_selftest,
    moe_gemm_grouped,
    moe_gemm_grouped_w4,
    pack_skinny_w,
    quant4_pack,
    quant4_unpack,
    rms_norm,
    rms_norm_residual,
    rope_apply_,
    rope_kv_write_,
    rope_kv_write_part,
    rope_cos_sin,
    set_attn_sparsity,
    swiglu,
)
