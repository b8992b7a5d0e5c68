"""fp8 (e4m3) KV pool off the GPU: the pool manager moves 1-byte pages as it
moves bf16 ones, the kv.dtype switch and --kv-dtype reach make_kv, and what the
fp8 kernels do not cover is refused."""
import sys

import pytest
import torch

from bloombee_amd import config as bcfg
from bloombee_amd import ops
from bloombee_amd.engine import BlockStack
from bloombee_amd.kv import PagedKVCache
from bloombee_amd.models.base import resolve_config
from bloombee_amd.ops import interface as iface

FP8 = torch.float8_e4m3fn


def _fill(kv, pool, T, seed):
    """kv_write T random tokens at the sequences' ends; returns the rows."""
    gen = torch.Generator().manual_seed(seed)
    shape = (kv.batch_size, pool.num_kv_heads, T, pool.head_dim)
    start = torch.tensor(kv.lengths, dtype=torch.int32)
    kv.extend(T, speculative=True)
    k = (torch.randn(shape, generator=gen) * 4).bfloat16()
    v = (torch.randn(shape, generator=gen) * 4).bfloat16()
    k[0, 0, 0, :2] = torch.tensor([1e4, -500.0])         # saturates, no NaN
    ops.kv_write(k, v, kv.k_pages(0), kv.v_pages(0), kv.page_table(), start)
    return k, v


def test_fp8_pool_lifecycle_is_byte_exact():
    pool = PagedKVCache(1, 2, 64, max_tokens=1024, device="cpu", dtype=FP8)
    kv = pool.allocate(2, 128)
    q8 = lambda x: x.float().clamp(-448, 448).to(FP8).view(torch.uint8)
    k1, v1 = _fill(kv, pool, 21, 0)
    kv.commit()
    k2, v2 = _fill(kv, pool, 6, 1)                       # a speculative tree
    keeps = [[0, 2, 5], [1, 3, 4]]
    kv.reorder_and_commit(keeps)
    assert kv.lengths == [24, 24]
    want = [[torch.cat([a[b], c[b][:, keeps[b]]], dim=1) for b in range(2)]
            for a, c in ((k1, k2), (v1, v2))]

    def check(n):
        for b in range(2):
            got = ops.kv_gather(kv.k_pages(0), kv.v_pages(0), kv.page_table(), n, b)
            for g, w in zip(got, want):
                assert torch.equal(g.view(torch.uint8), q8(w[b][:, :n]))

    check(24)
    assert bool(torch.isfinite(kv.k_pages(0).float()).all())
    for compress in (False, True):      # compress keeps the raw fp8 snapshot
        kv.swap_out(compress=compress)
        assert kv._swapped[0][0][0].dtype == FP8
        kv.swap_in()
        check(24)
    _fill(kv, pool, 9, 2)
    kv.rollback()
    kv.truncate([17, 17])
    assert kv.lengths == [17, 17]
    check(17)


def test_switch_and_flag_reach_make_kv(monkeypatch):
    stack = BlockStack(resolve_config("llama-tiny"), 0, 1)
    assert stack.make_kv(64).dtype == torch.bfloat16
    assert stack.make_kv(64, "fp8").dtype == FP8
    monkeypatch.setenv("BBAMD_KV_DTYPE", "fp8")
    monkeypatch.setattr(bcfg, "_GLOBAL", None)
    assert stack.make_kv(64).k_pages(0).dtype == FP8
    assert stack.make_kv(64, "bf16").dtype == torch.bfloat16
    monkeypatch.setenv("BBAMD_KV_DTYPE", "int4")
    with pytest.raises(ValueError, match="BBAMD_KV_DTYPE"):
        bcfg.KVConfig()
    monkeypatch.delenv("BBAMD_KV_DTYPE")
    monkeypatch.setattr(bcfg, "_GLOBAL", None)

    # run_server --kv-dtype -> Server(kv_dtype=...) -> backend -> pool
    from bloombee_amd.cli import run_server
    from bloombee_amd.server.backend import StackBackend

    class FakeServer:
        def __init__(self, model, **kw):
            self.backend = StackBackend(resolve_config(model), 0, 1,
                                        kv_max_tokens=64, kv_dtype=kw["kv_dtype"])
            raise SystemExit(str(self.backend.kv_pool.dtype))

    monkeypatch.setattr(run_server, "Server", FakeServer)
    monkeypatch.setattr(sys, "argv", ["run_server", "llama-tiny", "--device", "cpu",
                                      "--throughput", "1", "--kv-dtype", "fp8"])
    with pytest.raises(SystemExit, match="float8_e4m3fn"):
        run_server.main()


def test_uncovered_combinations_are_refused(monkeypatch):
    with pytest.raises(ValueError, match="head dims"):        # gemma-4: 256 / 512
        BlockStack(resolve_config("gemma4-tiny"), 0, 2).make_kv(64, "fp8")
    monkeypatch.setenv("BBAMD_MIXED_ATTN", "on")
    monkeypatch.setattr(bcfg, "_GLOBAL", None)
    with pytest.raises(ValueError, match="MIXED_ATTN"):
        BlockStack(resolve_config("llama-tiny"), 0, 1).make_kv(64, "fp8")
    monkeypatch.setattr(bcfg, "_GLOBAL", None)

    # on a GPU box these never reach a composition: fake "on the GPU"
    monkeypatch.setattr(iface, "_on_gpu", lambda t: True)
    monkeypatch.setattr(iface, "_require_ext", lambda: None)
    q = torch.zeros(1, 4, 1, 64, dtype=torch.bfloat16)
    kp, vp = torch.zeros(2, 2, 16, 64).to(FP8), torch.zeros(2, 2, 64, 16).to(FP8)
    pt, ctx = torch.zeros(1, 2, dtype=torch.int32), torch.ones(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="fp8 KV pool.*host prefix"):
        ops.attn_paged_mixed(q, kp, vp, pt, ctx, None, None)
    with pytest.raises(RuntimeError, match="fp8 KV pool.*head_dim 256"):
        ops.attn_decode(q, torch.zeros(2, 2, 16, 256).to(FP8), vp, pt, ctx)
    monkeypatch.setattr(iface, "_attn_sparsity", 0.5)
    with pytest.raises(RuntimeError, match="fp8 KV pool.*sparse"):
        ops.attn_decode(q, kp, vp, pt, ctx)
