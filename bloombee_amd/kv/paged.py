"""Paged KV cache — the single KV manager of the framework.

The reference grew three interlocking components: a cross-process slab
allocator (memory_cache.py, 475 LoC), a 2,160-LoC KVCacheManager doing
layout conversion + micro-batch staging + spec-dec reorder, and an aliased
PagedKVTable side-channel (paged_kv.py). SURVEY.md §7 hard-part 2 calls that
split-brain transitional and says: design paged-first. This module is that
design.

Key choices (MI355X-native):
  * ONE device pool per worker: shape (L, 2, n_pages, Hkv, P, D). A sequence
    advances through all locally-hosted layers in lockstep, so one page list
    serves every layer — the per-layer K/V pages simply index it identically.
  * Page size 16 tokens (ref paged_kv.py:35 BLOCK_SIZE=16). At D=128/bf16 a
    (page, head) slab is 16*128*2 = 4 KB contiguous — one coalesced burst.
  * Committed vs speculative lengths per sequence (l_acc / l_spec, ref
    paged_kv.py:42-49) with commit/rollback freeing orphaned pages.
  * Token-budget admission control with blocking wait + timeout (ref
    memory_cache.py:166-222 _wait_until_available / AllocationFailed).
  * No cross-process slab pipe: the server runtime is one process with a GPU
    worker thread, so a threading.Condition suffices.
"""
from __future__ import annotations

import contextlib
import os
import threading
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from bloombee_amd.utils.logging import get_logger

logger = get_logger(__name__)


class PagedKVError(Exception):
    pass


class AllocationFailed(PagedKVError):
    pass


@dataclass
class _SeqState:
    pages: List[int] = field(default_factory=list)
    l_acc: int = 0    # committed tokens
    l_spec: int = 0   # committed + speculative tokens (>= l_acc)


def kv_pool_dtype(kv_dtype: Optional[str], model_dtype: torch.dtype,
                  head_dims, page_size: int, layout=None) -> torch.dtype:
    """Element type of a new pool. kv_dtype: "bf16" / "fp8", or None for the
    config's kv.dtype (BBAMD_KV_DTYPE). bf16 keeps the model's dtype. fp8
    (torch.float8_e4m3fn) is refused here, at pool creation, for what the fp8
    kernels do not cover, instead of at the first attention call."""
    from bloombee_amd.config import get_config, parse_kv_dtype
    cfg = get_config().kv
    kind = parse_kv_dtype(kv_dtype) if kv_dtype is not None else cfg.dtype
    if kind != "fp8":
        return model_dtype
    dims = sorted(set(head_dims if isinstance(head_dims, (list, tuple))
                      else [head_dims]))
    if any(d not in (64, 128) for d in dims):
        raise ValueError(f"kv dtype fp8: head dims {dims} are not covered "
                         "(the fp8 KV kernels take 64 and 128)")
    if page_size != 16:
        raise ValueError(f"kv dtype fp8 needs page size 16, got {page_size}")
    if layout is not None and any(x != "kv" for x in layout):
        raise ValueError("kv dtype fp8: k-only (k == v) layers are not covered")
    if model_dtype != torch.bfloat16:
        raise ValueError("kv dtype fp8 needs a bf16 model (the kernels read "
                         f"bf16 q), got {model_dtype}")
    if cfg.mixed_attn != "off":
        raise ValueError("kv dtype fp8 cannot be combined with "
                         "BBAMD_MIXED_ATTN: mixed-device decode has no fp8 "
                         "kernel")
    return torch.float8_e4m3fn


class PagedKVCache:
    """Device-resident paged KV pool for a contiguous range of layers."""

    def __init__(
        self,
        num_layers: int,
        num_kv_heads,
        head_dim,
        *,
        page_size: int = 16,
        max_tokens: int = 1 << 20,
        device: torch.device | str = "cpu",
        dtype: torch.dtype = torch.bfloat16,
        layout=None,
    ):
        """num_kv_heads / head_dim may be ints (uniform) or per-layer lists —
        gemma-4 style heterogeneous KV geometry (sliding layers D=256, full
        layers D=512; ref server/backend.py:291-306 per-block KV descriptor
        dispatch). `layout[l]` may be "kv" (default) or "k" — k-only layers
        (gemma-4 attention_k_eq_v full-attention layers) allocate no V plane.
        """
        self.num_layers = num_layers
        as_list = (lambda v: list(v) if isinstance(v, (list, tuple))
                   else [v] * num_layers)
        self.num_kv_heads_per_layer = as_list(num_kv_heads)
        self.head_dim_per_layer = as_list(head_dim)
        self.layout = as_list(layout if layout is not None else "kv")
        self.num_kv_heads = self.num_kv_heads_per_layer[0]
        self.head_dim = self.head_dim_per_layer[0]
        self.page_size = page_size
        self.device = torch.device(device)
        self.dtype = dtype
        self.n_pages = max(1, max_tokens // page_size)
        self.max_tokens = self.n_pages * page_size

        # Per-layer page planes; pools[l][0] = K pages, pools[l][1] = V (or
        # aliased to K for "k" layout). A page id indexes every layer's plane.
        self.pools = []
        for l in range(num_layers):
            hkv, d = self.num_kv_heads_per_layer[l], self.head_dim_per_layer[l]
            k = torch.zeros(self.n_pages, hkv, page_size, d,
                            device=self.device, dtype=dtype)
            v = k if self.layout[l] == "k" else torch.zeros_like(k)
            self.pools.append((k, v))
        self._free_pages: List[int] = list(range(self.n_pages - 1, -1, -1))
        self._reserved_tokens = 0  # admission-control reservation
        self._lock = threading.Condition()
        self._handles: Dict[int, "SessionHandle"] = {}
        self._next_handle = 0

    # -- introspection ----------------------------------------------------
    @property
    def tokens_left(self) -> int:
        """Unreserved token budget — gossiped as cache_tokens_left in
        ServerInfo (ref server/server.py:970-984)."""
        with self._lock:
            return self.max_tokens - self._reserved_tokens

    def k_pages(self, layer: int) -> torch.Tensor:
        """K pages, token-major: (n_pages, Hkv, P, D)."""
        return self.pools[layer][0]

    def v_pages(self, layer: int) -> torch.Tensor:
        """V pages, d-major: (n_pages, Hkv, D, P).

        V is stored TRANSPOSED within each (page, head) slab so the decode
        attention kernel's P.V MFMA B-fragments (8 consecutive positions at a
        fixed d) are direct contiguous 16 B loads from HBM — no LDS transpose
        staging. Same bytes as the K slab (P*D*2), reinterpreted.

        For "k"-layout layers (gemma-4 k==v aliasing) there is no V plane;
        callers must read K instead (the block handles it).
        """
        if self.layout[layer] == "k":
            raise PagedKVError(f"layer {layer} is k-only (v aliases k)")
        v = self.pools[layer][1]
        hkv, d = self.num_kv_heads_per_layer[layer], self.head_dim_per_layer[layer]
        return v.view(self.n_pages, hkv, d, self.page_size)

    # -- admission --------------------------------------------------------
    def allocate(
        self, batch_size: int, max_length: int, timeout: Optional[float] = None,
        resident_batch: Optional[int] = None,
    ) -> "SessionHandle":
        """Reserve budget for a decode session of `batch_size` sequences of up
        to `max_length` tokens each. Blocks until budget frees up, then raises
        AllocationFailed past `timeout` (ref memory_cache.py:147-222).

        resident_batch: KV-multiplexed sessions keep only this many rows on
        the device at a time (the rest live in pinned host snapshots via
        swap_out_rows), so admission reserves only the resident window —
        a batch bigger than HBM can hold becomes servable (ref GPU-multiplex
        working slots, memory_cache_manager.py:628-908).

        Pages themselves are allocated lazily as tokens arrive.
        """
        pages_per_seq = (max_length + self.page_size - 1) // self.page_size
        need = min(batch_size, resident_batch or batch_size) \
            * pages_per_seq * self.page_size
        deadline = None if timeout is None else time.monotonic() + timeout
        with self._lock:
            while self.max_tokens - self._reserved_tokens < need:
                if need > self.max_tokens:
                    raise AllocationFailed(
                        f"requested {need} KV tokens > pool capacity {self.max_tokens}"
                    )
                remaining = None if deadline is None else deadline - time.monotonic()
                if remaining is not None and remaining <= 0:
                    raise AllocationFailed(
                        f"timed out waiting for {need} KV tokens "
                        f"({self.max_tokens - self._reserved_tokens} available)"
                    )
                self._lock.wait(timeout=remaining)
            self._reserved_tokens += need
            handle = SessionHandle(self, self._next_handle, batch_size, max_length, need)
            self._handles[self._next_handle] = handle
            self._next_handle += 1
            return handle

    def _release(self, handle: "SessionHandle") -> None:
        with self._lock:
            if handle.handle_id not in self._handles:
                return
            del self._handles[handle.handle_id]
            for seq in handle.seqs:
                self._free_pages.extend(seq.pages)
                seq.pages.clear()
            self._reserved_tokens -= handle.reserved_tokens
            self._lock.notify_all()

    def free_page_count(self) -> int:
        with self._lock:
            return len(self._free_pages)

    def _take_pages(self, n: int) -> List[int]:
        with self._lock:
            if len(self._free_pages) < n:
                raise AllocationFailed(
                    f"page pool exhausted: need {n}, free {len(self._free_pages)}"
                )
            out = [self._free_pages.pop() for _ in range(n)]
            return out

    def _give_pages(self, pages: List[int]) -> None:
        with self._lock:
            self._free_pages.extend(pages)
            self._lock.notify_all()


class SessionHandle:
    """Per-inference-session view of the pool: B sequences with paged storage,
    speculative extension, commit/rollback, and a device page table."""

    def __init__(self, cache: PagedKVCache, handle_id: int, batch_size: int,
                 max_length: int, reserved_tokens: int):
        self.cache = cache
        self.handle_id = handle_id
        self.batch_size = batch_size
        self.max_length = max_length
        self.reserved_tokens = reserved_tokens
        self.seqs = [_SeqState() for _ in range(batch_size)]
        self._max_pages = (max_length + cache.page_size - 1) // cache.page_size
        self._page_table = torch.zeros(
            batch_size, self._max_pages, device=cache.device, dtype=torch.int32
        )
        # pinned host mirror: the dirty-flush H2D is async on the compute
        # stream; pageable async copies are a correctness hazard
        self._page_table_host = torch.zeros(
            batch_size, self._max_pages, dtype=torch.int32,
            pin_memory=(cache.device.type == "cuda"))
        self._table_dirty = False
        self._closed = False
        # row-granular host staging (micro-batch KV multiplexing):
        # b -> (page_count_at_swap, per-layer (k_host, v_host)) snapshots
        self._row_snaps: Dict[int, tuple] = {}
        # rows whose restore copies are in flight: b -> done event
        self._rows_inflight: Dict[int, threading.Event] = {}
        # serializes metadata mutation (page lists / lengths / table rows)
        # between the compute thread's extend() and the staging thread's
        # swap_{out,in}_rows — bulk copies run outside the lock
        self._meta_lock = threading.Lock()
        self._stage_stream = (torch.cuda.Stream(cache.device)
                              if cache.device.type == "cuda" else None)

    # -- lengths ----------------------------------------------------------
    @property
    def lengths(self) -> List[int]:
        return [s.l_spec for s in self.seqs]

    @property
    def committed_lengths(self) -> List[int]:
        return [s.l_acc for s in self.seqs]

    def position(self, b: int = 0) -> int:
        return self.seqs[b].l_acc

    # -- growth -----------------------------------------------------------
    def extend(self, num_tokens: int, speculative: bool = False) -> None:
        """Make room for `num_tokens` new tokens on every sequence, allocating
        pages as needed. If `speculative`, the tokens sit above l_acc and can
        be rolled back (ref paged_kv.py track/commit/rollback:206-261)."""
        self.extend_rows(0, self.batch_size, num_tokens,
                         speculative=speculative)

    def extend_rows(self, b0: int, b1: int, num_tokens: int,
                    speculative: bool = False,
                    timeout: Optional[float] = 60.0) -> None:
        """Row-ranged extend — micro-batch slices grow only their own rows,
        so a KV-multiplexed session (most rows host-staged) never allocates
        device pages for rows outside the resident window. Under page
        pressure this retries until the staging thread frees pages (the
        lock is NOT held while waiting — swap_out_rows needs it to free)."""
        if self.is_swapped:
            raise PagedKVError("extend on a swapped-out session; swap_in first")
        P = self.cache.page_size
        deadline = None if timeout is None else time.monotonic() + timeout
        while True:
            with self._meta_lock:
                need_total = 0
                per_seq_need = []
                for b in range(b0, b1):
                    s = self.seqs[b]
                    new_len = s.l_spec + num_tokens
                    if new_len > self.max_length:
                        raise PagedKVError(
                            f"sequence would exceed session max_length "
                            f"{self.max_length}")
                    # row-swapped sequences advance length-only: their pages
                    # are (re)allocated at swap_in_rows time
                    need = (0 if b in self._row_snaps
                            else (new_len + P - 1) // P - len(s.pages))
                    per_seq_need.append(need)
                    need_total += need
                try:
                    pages = (self.cache._take_pages(need_total)
                             if need_total else [])
                except AllocationFailed:
                    if (deadline is not None
                            and time.monotonic() > deadline):
                        raise
                    pages = None
                if pages is not None:
                    i = 0
                    for b, need in zip(range(b0, b1), per_seq_need):
                        s = self.seqs[b]
                        for _ in range(need):
                            self._page_table_host[b, len(s.pages)] = pages[i]
                            s.pages.append(pages[i])
                            i += 1
                    if need_total:
                        self._table_dirty = True
                    for b in range(b0, b1):
                        s = self.seqs[b]
                        s.l_spec += num_tokens
                        if not speculative:
                            s.l_acc = s.l_spec
                    return
            time.sleep(0.002)  # page pressure: let the stager free pages

    def commit(self, accepted: Optional[List[int]] = None) -> None:
        """Commit speculative tokens: all of them, or `accepted[b]` tokens per
        sequence (the rest are rolled back)."""
        for b, s in enumerate(self.seqs):
            take = (s.l_spec - s.l_acc) if accepted is None else accepted[b]
            if take < 0 or s.l_acc + take > s.l_spec:
                raise PagedKVError(f"invalid accepted count {take} for seq {b}")
            s.l_acc += take
        self.rollback()

    def rollback(self) -> None:
        """Drop tokens above l_acc and free orphaned pages."""
        P = self.cache.page_size
        freed: List[int] = []
        for s in self.seqs:
            s.l_spec = s.l_acc
            keep = (s.l_acc + P - 1) // P
            while len(s.pages) > keep:
                freed.append(s.pages.pop())
        if freed:
            self.cache._give_pages(freed)
            # freed slots in the host table are stale but unreachable (ctx_len
            # bounds every kernel read); no rewrite needed.

    def reorder_and_commit(self, keep: List[List[int]]) -> None:
        """Speculative-tree accept: compact the kept nodes' K/V.

        keep[b] = ascending linear indices (within this round's speculative
        region, i.e. relative to l_acc) of the accepted tree nodes. Their
        K/V rows move to contiguous positions l_acc..l_acc+len(keep[b]) and
        are committed; the rest of the speculative region is rolled back
        (ref memory_cache_manager.py:1749-2040 update_cache_and_async_reorder
        — here a paged in-place compaction, no async side channel needed).
        """
        P = self.cache.page_size
        for b, idx in enumerate(keep):
            s = self.seqs[b]
            base = s.l_acc
            for d, rel in enumerate(idx):
                src, dst = base + rel, base + d
                if src == dst:
                    continue
                if src < dst or base + rel >= s.l_spec:
                    raise PagedKVError("keep indices must be ascending and "
                                       "inside the speculative region")
                pg_s = int(self._page_table_host[b, src // P])
                pg_d = int(self._page_table_host[b, dst // P])
                for l in range(self.cache.num_layers):
                    kp = self.cache.k_pages(l)
                    kp[pg_d, :, dst % P, :] = kp[pg_s, :, src % P, :]
                    if self.cache.layout[l] != "k":
                        vp = self.cache.v_pages(l)
                        vp[pg_d, :, :, dst % P] = vp[pg_s, :, :, src % P]
        self.commit([len(k) for k in keep])

    # -- host offload (session multiplexing) ------------------------------
    def swap_out(self, to_disk: bool = False,
                 disk_dir: Optional[str] = None,
                 compress: bool = False) -> None:
        """Offload this session's KV to pinned host buffers and release its
        device pages (reference micro-batch KV offload: GPU working slots +
        CPU snapshots on dedicated streams, memory_cache_manager.py:944-1371).
        Another session can use the freed pages; swap_in restores the data
        (possibly into different physical pages — the page table rewrites).

        to_disk: spill the snapshot to a file instead of keeping it in host
        RAM (the reference's third KV tier, TorchMixedDevice GPU/CPU/disk
        partition, pytorch_backend.py:1207-1237; here whole-session
        granularity under the same page-table-rewrite contract).

        compress: 4-bit group-quantize the snapshot (Policy.compress_cache,
        ref flexgen compression.py group quant) — ~4x smaller host/disk
        footprint, lossy within the quant tolerance.
        """
        if getattr(self, "_swapped", None) is not None:
            return
        cache = self.cache
        on_gpu = cache.device.type == "cuda"
        stream = torch.cuda.Stream(cache.device) if on_gpu else None
        snap = []  # per seq: per layer: (k_host, v_host) stacked page data
        with torch.cuda.stream(stream) if on_gpu else contextlib.nullcontext():
            for b, s in enumerate(self.seqs):
                pages = torch.tensor(s.pages, dtype=torch.long,
                                     device=cache.device)
                per_layer = []
                for l in range(cache.num_layers):
                    k = cache.k_pages(l)[pages]
                    kh = torch.empty_like(k, device="cpu",
                                          pin_memory=on_gpu)
                    kh.copy_(k, non_blocking=on_gpu)
                    if cache.layout[l] != "k":
                        v = cache.v_pages(l)[pages]
                        vh = torch.empty_like(v, device="cpu",
                                              pin_memory=on_gpu)
                        vh.copy_(v, non_blocking=on_gpu)
                    else:
                        vh = None
                    per_layer.append((kh, vh))
                snap.append(per_layer)
        if on_gpu:
            stream.synchronize()
        from bloombee_amd.utils.logging import debug_log, get_logger
        debug_log("kv", get_logger(__name__),
                  "swap_out handle=%d to_disk=%s compress=%s",
                  self.handle_id, to_disk, compress)
        if compress and cache.dtype != torch.float8_e4m3fn:
            # (an fp8 pool keeps the raw 1-byte snapshot: 4-bit requantising
            # 8-bit data would stack a second, coarser rounding on the first)
            from bloombee_amd import ops as _ops
            comp = []
            for per_layer in snap:
                cl = []
                for kh, vh in per_layer:
                    kq = _ops.quant4_pack(kh.float().reshape(-1, 64)) + (kh.shape, kh.dtype)
                    vq = (None if vh is None else
                          _ops.quant4_pack(vh.float().reshape(-1, 64)) + (vh.shape, vh.dtype))
                    cl.append((kq, vq))
                comp.append(cl)
            snap = ("q4", comp)
        if to_disk:
            import tempfile
            fd, path = tempfile.mkstemp(
                suffix=".kvswap.pt", dir=disk_dir)
            os.close(fd)
            torch.save(snap, path)
            self._swapped = ("disk", path)
        else:
            self._swapped = snap
        freed = []
        # record per-seq page COUNTS and clear the id lists: stale ids left
        # in seq.pages would be freed AGAIN by _release/rollback/truncate
        # while swapped, putting duplicates in the free list so two sessions
        # could share a physical page
        self._swapped_counts = [len(s.pages) for s in self.seqs]
        for s in self.seqs:
            freed.extend(s.pages)
            s.pages.clear()
        # release the physical pages but keep the reservation (the session
        # still owns its token budget)
        self.cache._give_pages(freed)

    def swap_in(self) -> None:
        """Restore a swapped-out session: take fresh pages, copy the host
        snapshot back, rewrite the page table."""
        if not self.is_swapped:
            return
        snap = self._materialize_snapshot()
        cache = self.cache
        on_gpu = cache.device.type == "cuda"
        stream = torch.cuda.Stream(cache.device) if on_gpu else None
        with torch.cuda.stream(stream) if on_gpu else contextlib.nullcontext():
            for b, s in enumerate(self.seqs):
                n = self._swapped_counts[b]
                new_pages = self.cache._take_pages(n)
                s.pages = new_pages
                for j, pg in enumerate(new_pages):
                    self._page_table_host[b, j] = pg
                idx = torch.tensor(new_pages, dtype=torch.long,
                                   device=cache.device)
                for l in range(cache.num_layers):
                    kh, vh = snap[b][l]
                    cache.k_pages(l)[idx] = kh.to(cache.device,
                                                  non_blocking=on_gpu)
                    if vh is not None:
                        cache.v_pages(l)[idx] = vh.to(cache.device,
                                                      non_blocking=on_gpu)
        if on_gpu:
            stream.synchronize()
        self._table_dirty = True
        self._swapped = None
        del self._swapped_counts
        # a truncate/rollback issued while swapped shrank l_spec without
        # touching pages (there were none); trim the restored excess now
        P = cache.page_size
        freed: List[int] = []
        for s in self.seqs:
            keep = (s.l_spec + P - 1) // P
            while len(s.pages) > keep:
                freed.append(s.pages.pop())
        if freed:
            self.cache._give_pages(freed)

    @property
    def is_swapped(self) -> bool:
        return getattr(self, "_swapped", None) is not None

    def swapped_pages_needed(self) -> int:
        """Device pages a full swap_in would claim (0 when not swapped) —
        the backend's mixed_attn="auto" policy compares this against the
        pool's current free pages to pick restore vs mixed-device decode."""
        if not self.is_swapped:
            return 0
        return sum(self._swapped_counts)

    # -- mixed-device decode (host prefix + device recent segment) --------
    @property
    def pos_offset(self) -> int:
        """Absolute position of the device pool's local position 0: after
        swap_in_as_prefix the committed history lives in host tensors and
        only tokens >= pos_offset occupy device pages. RoPE must use
        absolute positions (local + pos_offset); the paged kernels use
        local ones."""
        return getattr(self, "_pos_offset", 0)

    def host_prefix(self, layer: int):
        """(k_host, v_host) as (B, Hkv, S_host, D) pinned CPU tensors for
        `layer`, or None when the session is fully device-resident. The
        attention path merges them with the device segment via the exact
        log-sum-exp composition (ops.attn_paged_mixed)."""
        hp = getattr(self, "_host_prefix", None)
        return hp[layer] if hp is not None else None

    def _materialize_snapshot(self):
        """Resolve a whole-session snapshot (possibly disk-spilled or
        4-bit-compressed) into per-seq per-layer (k_host, v_host) page
        stacks — shared by swap_in and swap_in_as_prefix."""
        snap = getattr(self, "_swapped", None)
        if isinstance(snap, tuple) and snap[0] == "disk":
            path = snap[1]
            snap = torch.load(path, map_location="cpu", weights_only=False)
            os.unlink(path)
        if isinstance(snap, tuple) and snap[0] == "q4":
            from bloombee_amd import ops as _ops

            def _deq(q):
                if q is None:
                    return None
                packed, scale, zero, shape, dtype = q
                return _ops.quant4_unpack(packed, scale, zero,
                                          dtype=dtype).reshape(shape)

            snap = [[(_deq(kq), _deq(vq)) for kq, vq in per_layer]
                    for per_layer in snap[1]]
        return snap

    def swap_in_as_prefix(self) -> None:
        """Convert a WHOLE-swapped session into mixed-device form instead of
        restoring it to HBM (ROUND2 item 7 / reference
        _mixed_device_attention, pytorch_backend.py:969-1014): the
        committed history becomes per-layer host tensors (B, Hkv, S, D);
        the device pool restarts empty at local position 0 and only NEW
        tokens take device pages. Decode steps then merge both segments
        exactly (ops.attn_paged_mixed). Requires lockstep sequences and no
        speculative tokens (both true for swapped idle sessions)."""
        if not self.is_swapped:
            return
        cache = self.cache
        S = self.seqs[0].l_acc
        if any(s.l_acc != S or s.l_spec != S for s in self.seqs):
            raise PagedKVError("mixed-device restore needs lockstep, "
                               "committed-only sequences")
        snap = self._materialize_snapshot()
        counts = self._swapped_counts
        host: List[tuple] = []
        for l in range(cache.num_layers):
            hkv = cache.num_kv_heads_per_layer[l]
            d = cache.head_dim_per_layer[l]
            P = cache.page_size
            ks, vs = [], []
            for b in range(self.batch_size):
                kh, vh = snap[b][l]  # (npages, Hkv, P, D) / (npages, Hkv, D, P)
                k_flat = kh.permute(1, 0, 2, 3).reshape(hkv, -1, d)[:, :S]
                if vh is None:
                    v_flat = k_flat
                else:
                    # (npages, Hkv, D, P) -> (Hkv, D, npages*P) -> (Hkv, S, D)
                    v_flat = (vh.permute(1, 2, 0, 3)
                              .reshape(hkv, d, -1)[:, :, :S]
                              .transpose(1, 2).contiguous())
                ks.append(k_flat)
                vs.append(v_flat)
            host.append((torch.stack(ks), torch.stack(vs)))
        old = getattr(self, "_host_prefix", None)
        if old is not None:
            host = [(torch.cat([ok, nk], dim=2), torch.cat([ov, nv], dim=2))
                    for (ok, ov), (nk, nv) in zip(old, host)]
        self._host_prefix = host
        self._pos_offset = self.pos_offset + S
        for b, s in enumerate(self.seqs):
            s.l_acc = 0
            s.l_spec = 0
            assert not s.pages
        del self._swapped_counts
        self._swapped = None
        _ = counts  # page ids were freed at swap_out; counts informational

    # -- row-granular staging (micro-batch KV multiplexing) ----------------
    def swap_out_rows(self, b0: int, b1: int) -> None:
        """Offload rows [b0, b1) to pinned host snapshots and free their
        device pages — the reference's GPU working slots + CPU snapshots on
        dedicated streams (memory_cache_manager.py:944-1371). Swapped rows
        keep advancing lengths (extend is page-free for them); the kernels
        never read them because micro-batch SessionViews slice the page
        table to the resident window."""
        if self.is_swapped:
            raise PagedKVError("whole session already swapped")
        cache = self.cache
        on_gpu = cache.device.type == "cuda"
        work = []  # (b, page_ids tensor, per-layer host bufs)
        with self._meta_lock:
            for b in range(b0, b1):
                s = self.seqs[b]
                if b in self._row_snaps or not s.pages:
                    continue
                ids = torch.tensor(s.pages, dtype=torch.long,
                                   device=cache.device)
                work.append((b, len(s.pages), ids))
        freed: List[int] = []
        if on_gpu:
            # the rows' last KV writes ride the compute (default) stream;
            # order the staging gathers after them
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(cache.device))
            self._stage_stream.wait_event(ev)
        stream_ctx = (torch.cuda.stream(self._stage_stream) if on_gpu
                      else contextlib.nullcontext())
        with stream_ctx:
            for b, npages, ids in work:
                per_layer = []
                for l in range(cache.num_layers):
                    k = cache.k_pages(l)[ids]
                    kh = torch.empty_like(k, device="cpu", pin_memory=on_gpu)
                    kh.copy_(k, non_blocking=on_gpu)
                    if cache.layout[l] != "k":
                        v = cache.v_pages(l)[ids]
                        vh = torch.empty_like(v, device="cpu",
                                              pin_memory=on_gpu)
                        vh.copy_(v, non_blocking=on_gpu)
                    else:
                        vh = None
                    per_layer.append((kh, vh))
                with self._meta_lock:
                    s = self.seqs[b]
                    self._row_snaps[b] = (npages, per_layer)
                    freed.extend(s.pages)
                    s.pages.clear()
        if on_gpu:
            self._stage_stream.synchronize()
        if freed:
            self.cache._give_pages(freed)

    def swap_in_rows(self, b0: int, b1: int,
                     timeout: Optional[float] = 60.0) -> None:
        """Restore rows [b0, b1): fresh pages, H2D copies on the staging
        stream, page-table rows rewritten. Synchronous w.r.t. its own
        copies — run it on a staging thread to overlap the previous
        micro-batch's compute (server/handler.py drives this).

        Concurrent-restore safe: a second call overlapping the same rows
        (prefetch + arrival both staging a slice) waits for the in-flight
        restore instead of returning while its copies are incomplete.
        Under page pressure the allocation retries without holding the
        metadata lock (swap_out_rows needs it to free pages)."""
        cache = self.cache
        on_gpu = cache.device.type == "cuda"
        P = cache.page_size
        deadline = None if timeout is None else time.monotonic() + timeout
        work = []
        wait_evs = []
        for b in range(b0, b1):
            while True:
                with self._meta_lock:
                    ev = self._rows_inflight.get(b)
                    if ev is not None:
                        wait_evs.append(ev)
                        break
                    if b not in self._row_snaps:
                        break
                    s = self.seqs[b]
                    n_now = (s.l_spec + P - 1) // P
                    try:
                        pages = self.cache._take_pages(n_now)
                    except AllocationFailed:
                        pages = None
                    if pages is not None:
                        snap = self._row_snaps.pop(b)
                        s.pages = pages
                        for j, pg in enumerate(pages):
                            self._page_table_host[b, j] = pg
                        done = threading.Event()
                        self._rows_inflight[b] = done
                        work.append((b, snap, pages, done))
                        self._table_dirty = True
                        break
                if deadline is not None and time.monotonic() > deadline:
                    raise AllocationFailed(
                        f"swap_in_rows timed out waiting for pages (row {b})")
                time.sleep(0.002)  # pressure: let the stager free pages
        stream_ctx = (torch.cuda.stream(self._stage_stream) if on_gpu
                      else contextlib.nullcontext())
        with stream_ctx:
            for b, (n_snap, per_layer), pages, _ in work:
                n_copy = min(n_snap, len(pages))
                idx = torch.tensor(pages[:n_copy], dtype=torch.long,
                                   device=cache.device)
                for l in range(cache.num_layers):
                    kh, vh = per_layer[l]
                    cache.k_pages(l)[idx] = kh[:n_copy].to(
                        cache.device, non_blocking=on_gpu)
                    if vh is not None:
                        cache.v_pages(l)[idx] = vh[:n_copy].to(
                            cache.device, non_blocking=on_gpu)
        if on_gpu:
            self._stage_stream.synchronize()
        with self._meta_lock:
            for b, _, _, done in work:
                done.set()
                self._rows_inflight.pop(b, None)
        for ev in wait_evs:
            if not ev.wait(timeout=timeout):
                raise PagedKVError("in-flight row restore did not finish")

    def rows_swapped(self, b0: int, b1: int) -> bool:
        with self._meta_lock:
            return any(b in self._row_snaps for b in range(b0, b1))

    def truncate(self, new_lengths: List[int]) -> None:
        """Failover / history-replay support: cut sequences back to
        `new_lengths` committed tokens (ref inference_session.py:802-831)."""
        for b, (s, n) in enumerate(zip(self.seqs, new_lengths)):
            if n > s.l_acc:
                raise PagedKVError("truncate can only shrink")
            s.l_acc = n
        self.rollback()

    # -- kernel-facing views ----------------------------------------------
    def page_table(self) -> torch.Tensor:
        """(B, max_pages) int32 device tensor for the attention kernels."""
        if self._table_dirty:
            self._page_table.copy_(self._page_table_host, non_blocking=True)
            self._table_dirty = False
        return self._page_table

    def page_table_host(self) -> torch.Tensor:
        return self._page_table_host

    def k_pages(self, layer: int) -> torch.Tensor:
        return self.cache.k_pages(layer)

    def v_pages(self, layer: int) -> torch.Tensor:
        return self.cache.v_pages(layer)

    def close(self) -> None:
        if not self._closed:
            self._closed = True
            self.cache._release(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
