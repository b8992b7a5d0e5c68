"""Kernel microbenchmarks on a real MI355X (run via gpurun).

Reports per-kernel time and effective HBM bandwidth / TFLOPs so kernel
changes can be A/B'd without the end-to-end bench's noise.

    python benchmarks/bench_kernels.py [attn_decode attn_mixed attn_prefill attn_prefill_wide train_attn ring_fold ...]
"""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from bloombee_amd import ops
from bloombee_amd.ops import reference as ref

DEV = "cuda:0"


def timeit(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.monotonic()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.monotonic() - t0) / iters


def bench_attn_decode():
    for B, Hq, Hkv, ctx, D in [(32, 32, 8, 2048, 128), (32, 32, 8, 8192, 128),
                               (8, 32, 8, 2048, 128), (64, 32, 8, 2048, 128)]:
        P = 16
        maxp = (ctx + P - 1) // P
        npages = B * maxp + 1
        kp = torch.randn(npages, Hkv, P, D, dtype=torch.bfloat16, device=DEV)
        vp = torch.randn(kp.shape[0], Hkv, D, P, dtype=torch.bfloat16, device=DEV)
        pt = torch.arange(B * maxp, dtype=torch.int32, device=DEV).reshape(B, maxp)
        q = torch.randn(B, Hq, 1, D, dtype=torch.bfloat16, device=DEV) * 0.1
        ctx_l = torch.full((B,), ctx, dtype=torch.int32, device=DEV)
        bytes_ = B * Hkv * ctx * 2 * D * 2
        for ns in (0, 2, 4, 8, 16):
            t = timeit(lambda: ops.attn_decode(q, kp, vp, pt, ctx_l, n_split=ns))
            print(f"attn_decode B{B} Hq{Hq}/{Hkv} ctx{ctx} D{D} ns={ns}: "
                  f"{t*1e6:8.1f} us  {bytes_/t/1e12:6.2f} TB/s")


def bench_attn_decode_fp8():
    """fp8 (e4m3) KV pool against the bf16 pool, llama-3-8b geometry: decode
    attention at automatic n_split, the two alternating in one process, median
    of 5 windows each; TB/s over the KV bytes each actually reads. Then prefill
    of a 2k prompt the same way."""
    Hq, Hkv, D, P = 32, 8, 128, 16
    fp8 = torch.float8_e4m3fn

    def med(fn, iters):
        return sorted(timeit(fn, iters=iters, warmup=5) for _ in range(5))[2]

    for ctx in (2048, 8192, 32768):
        for B in (1, 8, 32):
            maxp = ctx // P
            kp = torch.randn(B * maxp, Hkv, P, D, dtype=torch.bfloat16, device=DEV)
            vp = torch.randn(B * maxp, Hkv, D, P, dtype=torch.bfloat16, device=DEV)
            kp8, vp8 = kp.to(fp8), vp.to(fp8)
            pt = torch.arange(B * maxp, dtype=torch.int32, device=DEV).reshape(B, maxp)
            q = torch.randn(B, Hq, 1, D, dtype=torch.bfloat16, device=DEV) * 0.1
            ctx_l = torch.full((B,), ctx, dtype=torch.int32, device=DEV)
            iters = max(20, min(400, (1 << 31) // (B * ctx * Hkv * D * 4)))
            t16 = t8 = 0.0
            for _ in range(2):      # alternate: bf16, fp8, bf16, fp8
                t16 += med(lambda: ops.attn_decode(q, kp, vp, pt, ctx_l), iters) / 2
                t8 += med(lambda: ops.attn_decode(q, kp8, vp8, pt, ctx_l), iters) / 2
            b16 = B * Hkv * ctx * 2 * D * 2
            print(f"attn_decode B{B} ctx{ctx}: bf16 {t16*1e6:8.1f} us "
                  f"{b16/t16/1e12:5.2f} TB/s   fp8 {t8*1e6:8.1f} us "
                  f"{b16/2/t8/1e12:5.2f} TB/s   bf16/fp8 {t16/t8:5.2f}", flush=True)
            del kp, vp, kp8, vp8
    B, T = 8, 2048
    maxp = T // P
    kp = torch.randn(B * maxp, Hkv, P, D, dtype=torch.bfloat16, device=DEV)
    vp = torch.randn(B * maxp, Hkv, D, P, dtype=torch.bfloat16, device=DEV)
    kp8, vp8 = kp.to(fp8), vp.to(fp8)
    pt = torch.arange(B * maxp, dtype=torch.int32, device=DEV).reshape(B, maxp)
    q = torch.randn(B, Hq, T, D, dtype=torch.bfloat16, device=DEV) * 0.1
    qs = torch.zeros(B, dtype=torch.int32, device=DEV)
    t16 = med(lambda: ops.attn_prefill(q, kp, vp, pt, qs), 20)
    t8 = med(lambda: ops.attn_prefill(q, kp8, vp8, pt, qs), 20)
    print(f"attn_prefill B{B} T{T}: bf16 {t16*1e6:8.1f} us   fp8 {t8*1e6:8.1f} us"
          f"   bf16/fp8 {t16/t8:5.2f}", flush=True)


def bench_attn_mixed():
    """Mixed-device decode, device side only: the decode kernel in
    forced-partial mode + the external-partial merge launch, against plain
    attn_decode at the same shape and against the old per-row torch
    composition (BBAMD_MIXED_KERNEL=0). The external partials are
    pre-computed and already on the device, and the host prefix is one page,
    so host attention time stays out of the figures."""
    from bloombee_amd.ops import hip_ops
    from bloombee_amd.ops import interface as iface
    B, Hq, Hkv, ctx, D, P, S_host = 32, 32, 8, 2048, 128, 16, 16
    maxp = (ctx + P - 1) // P
    npages = B * maxp + 1
    kp = torch.randn(npages, Hkv, P, D, dtype=torch.bfloat16, device=DEV)
    vp = torch.randn(kp.shape[0], Hkv, D, P, dtype=torch.bfloat16, device=DEV)
    pt = torch.arange(B * maxp, dtype=torch.int32, device=DEV).reshape(B, maxp)
    q = torch.randn(B, Hq, 1, D, dtype=torch.bfloat16, device=DEV) * 0.1
    ctx_l = torch.full((B,), ctx, dtype=torch.int32, device=DEV)
    hk = torch.randn(B, Hkv, S_host, D)
    hv = torch.randn(B, Hkv, S_host, D)
    scale = 1.0 / math.sqrt(D)
    ml, acc = ref.attn_host_partial(q[:, :, 0].float().cpu(), hk, hv, scale)
    ml, acc = ml.to(DEV), acc.to(DEV)
    tag = f"B{B} Hq{Hq}/{Hkv} ctx{ctx} D{D}"
    t_dec = timeit(lambda: ops.attn_decode(q, kp, vp, pt, ctx_l))
    print(f"attn_decode        {tag}: {t_dec*1e6:9.1f} us")
    t_mix = timeit(lambda: hip_ops.attn_decode_mixed(
        q, kp, vp, pt, ctx_l, ml, acc, scale, 0, 0, None, S_host))
    print(f"attn_mixed[kernel] {tag}: {t_mix*1e6:9.1f} us  "
          f"(device only, {t_mix/t_dec:.2f}x attn_decode)")
    t_e2e = timeit(lambda: ops.attn_paged_mixed(q, kp, vp, pt, ctx_l, hk, hv),
                   iters=20, warmup=3)
    print(f"attn_mixed[kernel] {tag}: {t_e2e*1e6:9.1f} us  "
          f"(end to end: q D2H + host partial S_host={S_host} + H2D)")
    old = iface._MIXED_KERNEL
    iface._MIXED_KERNEL = False
    try:
        t_old = timeit(lambda: ops.attn_paged_mixed(q, kp, vp, pt, ctx_l,
                                                    hk, hv),
                       iters=5, warmup=1)
    finally:
        iface._MIXED_KERNEL = old
    print(f"attn_mixed[torch composition] {tag}: {t_old*1e6:9.1f} us  "
          f"({t_old/t_e2e:.1f}x the kernel path end to end, "
          f"{t_old/t_mix:.1f}x its device time)")


def bench_attn_sparse():
    """Top-k sparse decode (ops.set_attn_sparsity): the attn_sparse.hip kernel
    path against the per-row torch composition it replaces
    (ref.attn_paged_topk as it stands, stable sort included, on the same
    device tensors: one host sync per batch row) and against dense
    attn_decode, per K fill:

      random   K ~ N(0,1): the kept set of every head is scattered
      peaked   K aligned with the group's queries at positions 0..3 and the
               last 256 (sinks + recent tokens); the other 252 kept positions
               of each head stay scattered
      clustered  the same with the last 508 positions, so the whole kept set
               (kkeep = 512) sits in 33 pages

    and reports the share of (row, kv head, page) tiles in which none of the
    G heads kept a position: the V loads the kernel skips."""
    from bloombee_amd.ops import hip_ops
    B, Hq, Hkv, ctx, D, P, sparsity = 32, 32, 8, 2048, 128, 16, 0.25
    G = Hq // Hkv
    maxp = ctx // P
    scale = 1.0 / math.sqrt(D)
    gen = torch.Generator(device=DEV).manual_seed(0)
    rn = lambda *sh: torch.randn(*sh, generator=gen, device=DEV)
    q = rn(B, Hq, 1, D).to(torch.bfloat16)
    v = rn(B, Hkv, ctx, D)
    pt = torch.arange(B * maxp, dtype=torch.int32, device=DEV).reshape(B, maxp)
    ctx_l = torch.full((B,), ctx, dtype=torch.int32, device=DEV)
    to_pages = lambda x: torch.cat([
        x.view(B, Hkv, maxp, P, D).permute(0, 2, 1, 3, 4)
        .reshape(B * maxp, Hkv, P, D),
        torch.zeros(1, Hkv, P, D, device=DEV)]).to(torch.bfloat16).contiguous()
    vp = to_pages(v).transpose(2, 3).contiguous()
    kkeep = max(1, min(ctx, math.ceil(sparsity * ctx)))
    tag = f"B{B} Hq{Hq}/{Hkv} ctx{ctx} D{D} s={sparsity}"
    for fill, recent in (("random", 0), ("peaked", 256), ("clustered", 508)):
        k = rn(B, Hkv, ctx, D)
        if recent:
            qg = q.float().view(B, Hkv, G, D).sum(2)           # (B, Hkv, D)
            hot = torch.cat([torch.arange(4, device=DEV),
                             torch.arange(ctx - recent, ctx, device=DEV)])
            k[:, :, hot] += 0.5 * qg[:, :, None, :]
        kp = to_pages(k)
        # kept set in torch (fp32 scores of the bf16 pool values)
        kf = kp[:-1].float().view(B, maxp, Hkv, P, D).permute(0, 2, 1, 3, 4) \
            .reshape(B, Hkv, ctx, D)
        sc_ = torch.einsum("bhgd,bhcd->bhgc", q.float().view(B, Hkv, G, D),
                           kf) * scale
        idx = sc_.topk(kkeep, dim=-1).indices
        kept = torch.zeros_like(sc_, dtype=torch.bool).scatter_(-1, idx, True)
        touched = kept.view(B, Hkv, G, maxp, P).any(dim=4).any(dim=2)
        skipped = 1.0 - float(touched.float().mean())

        out_k = hip_ops.attn_decode_sparse(q, kp, vp, pt, ctx_l, sparsity,
                                           scale, None)
        out_c = ref.attn_paged_topk(q, kp, vp, pt, ctx_l, sparsity, scale)
        diff = float((out_k.float() - out_c.float()).abs().max())
        t_dense = timeit(lambda: ops.attn_decode(q, kp, vp, pt, ctx_l))
        t_kern = timeit(lambda: hip_ops.attn_decode_sparse(
            q, kp, vp, pt, ctx_l, sparsity, scale, None))
        t_comp = timeit(lambda: ref.attn_paged_topk(
            q, kp, vp, pt, ctx_l, sparsity, scale), iters=5, warmup=1)
        t_dense2 = timeit(lambda: ops.attn_decode(q, kp, vp, pt, ctx_l))
        t_kern2 = timeit(lambda: hip_ops.attn_decode_sparse(
            q, kp, vp, pt, ctx_l, sparsity, scale, None))
        print(f"attn_sparse {tag} K={fill}: page tiles skipped "
              f"{100 * skipped:5.1f}%  max|kernel - composition| {diff:.4f}")
        print(f"  kernel       {t_kern*1e6:9.1f} us (repeat {t_kern2*1e6:.1f})")
        print(f"  composition  {t_comp*1e6:9.1f} us  "
              f"({t_comp/t_kern:.1f}x the kernel)")
        print(f"  dense decode {t_dense*1e6:9.1f} us (repeat {t_dense2*1e6:.1f})"
              f"  kernel / dense = {t_kern/t_dense:.2f}")


def bench_attn_prefill():
    for B, Hq, Hkv, T, D in [(32, 32, 8, 512, 128), (8, 32, 8, 2048, 128)]:
        P = 16
        maxp = (T + P - 1) // P
        npages = B * maxp + 1
        kp = torch.randn(npages, Hkv, P, D, dtype=torch.bfloat16, device=DEV)
        vp = torch.randn(kp.shape[0], Hkv, D, P, dtype=torch.bfloat16, device=DEV)
        pt = torch.arange(B * maxp, dtype=torch.int32, device=DEV).reshape(B, maxp)
        q = torch.randn(B, Hq, T, D, dtype=torch.bfloat16, device=DEV) * 0.1
        qs = torch.zeros(B, dtype=torch.int32, device=DEV)
        t = timeit(lambda: ops.attn_prefill(q, kp, vp, pt, qs), iters=20)
        flops = B * Hq * D * 2 * 2 * (T * (T + 1) / 2)  # causal
        print(f"attn_prefill B{B} Hq{Hq}/{Hkv} T{T} D{D}: "
              f"{t*1e6:8.1f} us  {flops/t/1e12:7.1f} TF/s")


def bench_attn_prefill_wide():
    """Prefill at head dim 512 (attn_prefill_wide.hip) beside the torch
    composition it replaces in ops.attn_prefill (ref.attn_paged on the device
    tensors, what BBAMD_PREFILL_WIDE=0 runs), at the gemma4-9b global layer:
    Hq=8, Hkv=4, scale 1.0. Three alternating rounds per case, each the median
    of device-event timings that end in a synchronise; printed as median
    [min..max]. TF/s counts the causal part only: 4 D FLOPs per (query, visible
    key). `D256` is ops.attn_prefill at D=256 with Hq and Hkv doubled: the
    same FLOPs and K/V bytes on attn_prefill_kernel<256>. Every page table
    is 8192 positions wide, a session's capacity as the serving path passes
    it, whatever the live context. After the three acceptance cases comes the
    sweep behind the routing rule of ops.attn_prefill (few workgroups, short
    to long live contexts); the last column is ops.attn_prefill itself, the
    path that rule picks and its time with the rule's q_start read."""
    from bloombee_amd.ops import interface as iface
    Hq, Hkv, D, P = 8, 4, 512, 16
    gen = torch.Generator(device=DEV).manual_seed(0)

    def inputs(B, Tq, q_start, Hq, Hkv, D):
        maxp = max(q_start + Tq, 8192) // P
        rnd = lambda *sh: torch.randn(*sh, generator=gen, device=DEV,
                                      dtype=torch.float32).to(torch.bfloat16)
        kp, vp = rnd(B * maxp, Hkv, P, D), rnd(B * maxp, Hkv, D, P)
        pt = torch.randperm(B * maxp, generator=gen, device=DEV).int().reshape(B, maxp)
        q = rnd(B, Hq, Tq, D) * (2.0 / math.sqrt(D))
        qs = torch.full((B,), q_start, dtype=torch.int32, device=DEV)
        return q, kp, vp, pt, qs

    cases = [(1, 2048, 0), (4, 512, 0), (1, 512, 7680)] + [
        (1, 17, 500), (1, 64, 0), (1, 512, 0), (1, 64, 960), (1, 128, 896),
        (1, 512, 512), (1, 64, 1984), (1, 128, 1920), (1, 512, 1536),
        (1, 64, 4032), (1, 128, 3968), (1, 512, 3584), (1, 1024, 3072),
        (1, 64, 8128), (1, 128, 8064), (1, 1024, 7168), (2, 512, 7680),
        (4, 512, 7680), (1, 2048, 6144)]
    for B, Tq, q_start in cases:
        wide = inputs(B, Tq, q_start, Hq, Hkv, D)
        half = inputs(B, Tq, q_start, 2 * Hq, 2 * Hkv, D // 2)
        kernel = lambda: ops.hip_ops.attn_prefill(*wide, 1.0, 0, None, None)
        comp = lambda: ref.attn_paged(*wide[:4], wide[4].long(), 1.0)
        d256 = lambda: ops.attn_prefill(*half, scale=1.0)
        routed = lambda: ops.attn_prefill(*wide, scale=1.0)
        path = iface._prefill_kernel_ok(wide[0], wide[1], wide[3], wide[4])
        err = (kernel().float() - comp().float()).abs().max().item()
        tk, tc, th, tr = [], [], [], []
        for _ in range(3):
            tk.append(_event_time(kernel, 20, 5))
            tc.append(_event_time(comp, 5, 2))
            th.append(_event_time(d256, 20, 5))
            tr.append(_event_time(routed, 10, 3))
        tk.sort(), tc.sort(), th.sort(), tr.sort()
        flops = 4.0 * D * B * Hq * (Tq * q_start + Tq * (Tq + 1) / 2)
        us = lambda t: f"{t[1]*1e6:9.1f} us [{t[0]*1e6:.1f}..{t[2]*1e6:.1f}]"
        print(f"attn_prefill_wide B{B} Tq{Tq} q_start{q_start}: "
              f"kernel {us(tk)} {flops/tk[1]/1e12:6.1f} TF/s   "
              f"composition {us(tc)} {flops/tc[1]/1e12:6.1f} TF/s   "
              f"composition/kernel {tc[1]/tk[1]:6.1f} (worst case "
              f"{tc[0]/tk[2]:.1f})   D256 {us(th)} {flops/th[1]/1e12:6.1f} TF/s   "
              f"max|kernel - composition| {err:.4f}   ops.attn_prefill "
              f"({'kernel' if path else 'composition'}) {us(tr)}", flush=True)


def bench_kv_stream():
    from bloombee_amd.ops import hip_ops
    B, Hkv, ctx, D, P = 32, 8, 2048, 128, 16
    maxp = ctx // P
    npages = B * maxp + 1
    kp = torch.randn(npages, Hkv, P, D, dtype=torch.bfloat16, device=DEV)
    vp = torch.randn(kp.shape[0], Hkv, D, P, dtype=torch.bfloat16, device=DEV)
    pt = torch.arange(B * maxp, dtype=torch.int32, device=DEV).reshape(B, maxp)
    ctx_l = torch.full((B,), ctx, dtype=torch.int32, device=DEV)
    bytes_ = B * Hkv * ctx * 2 * D * 2
    for ns in (2, 4, 8, 16):
        for nt in (False, True):
            t = timeit(lambda: hip_ops.kv_stream_probe(kp, vp, pt, ctx_l, ns, nt))
            print(f"kv_stream ns{ns} nt{int(nt)}: {t*1e6:7.1f} us  {bytes_/t/1e12:5.2f} TB/s")


def bench_norms():
    for N, H in [(32, 4096), (16384, 4096)]:
        x = torch.randn(N, H, dtype=torch.bfloat16, device=DEV)
        r = torch.randn_like(x)
        w = torch.randn(H, dtype=torch.bfloat16, device=DEV)
        t = timeit(lambda: ops.rms_norm(x, w))
        print(f"rms_norm ({N},{H}): {t*1e6:7.1f} us  {2*N*H*2/t/1e12:5.2f} TB/s")
        t = timeit(lambda: ops.rms_norm_residual(x, r, w))
        print(f"rms_norm_res ({N},{H}): {t*1e6:7.1f} us  {5*N*H*2/t/1e12:5.2f} TB/s")


def bench_layer_norm():
    """layer_norm beside rms_norm at decode-batch shapes of the LayerNorm
    families (Falcon-7B H = 4544, BLOOM-176B H = 14336). A window is 2000
    back-to-back calls between two device events; three rounds of 10
    windows, the median window per round, and the spread over the rounds
    next to it (compare two builds only beyond that spread)."""
    def per_call(fn, calls=2000, windows=10):
        for _ in range(200):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(windows):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3 / calls)
        ts.sort()
        return ts[len(ts) // 2]

    for N, H in [(32, 4544), (32, 14336)]:
        gen = torch.Generator(device=DEV).manual_seed(H)
        x = torch.randn(N, H, generator=gen, device=DEV).to(torch.bfloat16)
        w = torch.randn(H, generator=gen, device=DEV).to(torch.bfloat16)
        b = torch.randn(H, generator=gen, device=DEV).to(torch.bfloat16)
        tl, tr = [], []
        for _ in range(3):
            tl.append(per_call(lambda: ops.layer_norm(x, w, b)))
            tr.append(per_call(lambda: ops.rms_norm(x, w)))
        tl.sort(), tr.sort()
        print(f"layer_norm ({N},{H}): {tl[1]*1e6:7.2f} us [{tl[0]*1e6:.2f}..{tl[2]*1e6:.2f}]"
              f"   rms_norm: {tr[1]*1e6:7.2f} us [{tr[0]*1e6:.2f}..{tr[2]*1e6:.2f}]"
              f"   (call time, launch included)", flush=True)


def bench_swiglu():
    for N, I in [(32, 14336), (16384, 14336)]:
        gu = torch.randn(N, 2 * I, dtype=torch.bfloat16, device=DEV)
        t = timeit(lambda: ops.swiglu(gu))
        print(f"swiglu ({N},{I}): {t*1e6:7.1f} us  {3*N*I*2/t/1e12:5.2f} TB/s")


def bench_gemm():
    """hipBLASLt skinny-M decode GEMMs baseline."""
    for M, N, K, tag in [(32, 6144, 4096, "qkv"), (32, 4096, 4096, "o"),
                         (32, 28672, 4096, "gate_up"), (32, 4096, 14336, "down"),
                         (32, 128256, 4096, "lm_head")]:
        x = torch.randn(M, K, dtype=torch.bfloat16, device=DEV)
        w = torch.randn(N, K, dtype=torch.bfloat16, device=DEV)
        t = timeit(lambda: torch.nn.functional.linear(x, w))
        print(f"gemm[blaslt] {tag} {M}x{N}x{K}: {t*1e6:7.1f} us  "
              f"{N*K*2/t/1e12:5.2f} TB/s(wt)  {2*M*N*K/t/1e12:6.1f} TF/s")
        if N % 64 == 0:
            for ks in (0, 1, 2, 4, 8, 16):
                ts = timeit(lambda: ops.hip_ops.gemm_skinny(x, w, None, None, ks))
                print(f"gemm[skinny ks={ks}] {tag}: {ts*1e6:7.1f} us  "
                      f"{N*K*2/ts/1e12:5.2f} TB/s(wt)")



def bench_gemm_norm():
    """Fused-rmsnorm GEMM A/B per llama decode shape: overhead of the
    per-WG prepass+scale vs the separate rms_norm launch it replaces."""
    for M, N, K, tag in [(32, 6144, 4096, "qkv"), (32, 4096, 4096, "o"),
                         (32, 28672, 4096, "gate_up"), (32, 4096, 14336, "down")]:
        x = torch.randn(M, K, dtype=torch.bfloat16, device=DEV)
        w = torch.randn(N, K, dtype=torch.bfloat16, device=DEV)
        nw = torch.randn(K, dtype=torch.bfloat16, device=DEV)
        t0 = timeit(lambda: ops.hip_ops.gemm_skinny(x, w, None, None, 0))
        t1 = timeit(lambda: ops.hip_ops.gemm_skinny(x, w, None, None, 0, nw, 1e-5))
        tn = timeit(lambda: ops.hip_ops.rms_norm(x, nw, 1e-5))
        print(f"gemm_norm {tag} {M}x{N}x{K}: plain {t0*1e6:6.1f} us  "
              f"fused {t1*1e6:6.1f} us (+{(t1-t0)*1e6:5.1f})  "
              f"rms_norm alone {tn*1e6:5.1f} us")
    h = torch.randn(32, 4096, dtype=torch.bfloat16, device=DEV)
    a = torch.randn(32, 4096, dtype=torch.bfloat16, device=DEV)
    nw2 = torch.randn(4096, dtype=torch.bfloat16, device=DEV)
    tr = timeit(lambda: ops.hip_ops.rms_norm_residual(a, h, nw2, 1e-5))
    print(f"rms_norm_residual 32x4096: {tr*1e6:5.1f} us")



def _event_time(fn, iters, warmup):
    """Median of `iters` device-event timings of fn (seconds)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    ts.sort()
    return ts[len(ts) // 2]


def bench_train_attn():
    """fwd+bwd of ops.attn_train: the gfx950 kernels against the torch
    composition on the same GPU, llama-3-8b head geometry, B*T = 4096 tokens.
    Three alternating rounds per shape (median and spread), plus the peak
    memory each path adds on top of its inputs. FLOPs are the causal-half
    counts: forward 2 products, dQ kernel 3, dK/dV kernel 4."""
    Hq, Hkv, D = 32, 8, 128
    scale = 1.0 / math.sqrt(D)

    def run(q, k, v, do):
        out = ops.attn_train(q, k, v, scale)
        return torch.autograd.grad(out, (q, k, v), do)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        r = fn()
        torch.cuda.synchronize()
        del r
        return torch.cuda.max_memory_allocated() - base

    for T in (512, 1024, 2048, 4096):
        B = 4096 // T
        gen = torch.Generator(device=DEV).manual_seed(T)
        mk = lambda h: torch.randn(B, T, h, D, generator=gen, device=DEV,
                                   dtype=torch.bfloat16).requires_grad_(True)
        q, k, v = mk(Hq), mk(Hkv), mk(Hkv)
        do = torch.randn(B, T, Hq, D, generator=gen, device=DEV, dtype=torch.bfloat16)
        pair = B * Hq * D * 2.0 * (T * (T + 1) / 2)     # one causal product
        times = {"kernel": [], "eager": []}
        mem = {}
        for _ in range(3):
            for path, sw in (("kernel", "1"), ("eager", "0")):
                os.environ["BBAMD_TRAIN_ATTN_KERNEL"] = sw
                times[path].append(_event_time(lambda: run(q, k, v, do), 10, 3))
                mem[path] = peak(lambda: run(q, k, v, do))
        os.environ.pop("BBAMD_TRAIN_ATTN_KERNEL", None)
        with torch.no_grad():
            out, lse = ops.hip_ops.attn_train_fwd(q, k, v, scale, 0, None, True)
            t_f = _event_time(lambda: ops.hip_ops.attn_train_fwd(
                q, k, v, scale, 0, None, True), 20, 3)
            t_b = _event_time(lambda: ops.hip_ops.attn_train_bwd(
                do, q, k, v, out, lse, scale, 0, None), 20, 3)
        tk, te = sorted(times["kernel"]), sorted(times["eager"])
        print(f"train_attn B{B} T{T} Hq{Hq}/{Hkv} D{D}: "
              f"kernel {tk[1]*1e3:8.3f} ms [{tk[0]*1e3:.3f}..{tk[2]*1e3:.3f}]  "
              f"eager {te[1]*1e3:8.3f} ms [{te[0]*1e3:.3f}..{te[2]*1e3:.3f}]  "
              f"eager/kernel {te[1]/tk[1]:5.2f}  "
              f"peak +{mem['kernel']/2**20:8.1f} MiB vs +{mem['eager']/2**20:8.1f} MiB")
        print(f"    fwd {t_f*1e3:7.3f} ms {2*pair/t_f/1e12:6.1f} TF/s   "
              f"bwd (dQ + dK/dV) {t_b*1e3:7.3f} ms {7*pair/t_b/1e12:6.1f} TF/s")


def bench_ring_fold():
    """The ring-attention fold on the busiest rank of a context-parallel
    prefill, the last one: one diagonal block and world - 1 full blocks,
    llama-3-8b head geometry, B 1. Against attn_train_fwd on one causal
    problem of T = world * T_loc: the same arithmetic without state traffic.
    Each side's FLOP/s counts its own visible (query, key) pairs, two MFMA
    products each. Three alternating rounds (median and spread)."""
    B, Hq, Hkv, D = 1, 32, 8, 128
    scale = 1.0 / math.sqrt(D)
    for Tl in (1024, 4096):
        for world in (2, 8):
            T = world * Tl
            gen = torch.Generator(device=DEV).manual_seed(T + world)
            mk = lambda h: torch.randn(B, T, h, D, generator=gen, device=DEV,
                                       dtype=torch.bfloat16)
            qt, kt, vt = mk(Hq), mk(Hkv), mk(Hkv)          # (B, T, H, D)
            q = qt.permute(0, 2, 1, 3)[:, :, T - Tl:]
            k, v = (t.permute(0, 2, 1, 3).contiguous() for t in (kt, vt))
            r = world - 1

            def folds():
                state = None
                for src in range(r, -1, -1):
                    sl = slice(src * Tl, (src + 1) * Tl)
                    state = ops.attn_ring_fold(q, k[:, :, sl], v[:, :, sl], state,
                                               r * Tl, src * Tl, scale, 0,
                                               last=src == 0)
                return state

            train = lambda: ops.hip_ops.attn_train_fwd(qt, kt, vt, scale, 0, None, False)
            tr, tt = [], []
            for _ in range(3):
                tr.append(_event_time(folds, 10, 3))
                tt.append(_event_time(train, 10, 3))
            tr.sort()
            tt.sort()
            st = ops.attn_ring_fold(q, k[:, :, r * Tl:], v[:, :, r * Tl:], None,
                                    r * Tl, r * Tl, scale)
            t_diag = _event_time(lambda: ops.attn_ring_fold(
                q, k[:, :, r * Tl:], v[:, :, r * Tl:], None, r * Tl, r * Tl, scale), 10, 3)
            t_full = _event_time(lambda: ops.attn_ring_fold(
                q, k[:, :, :Tl], v[:, :, :Tl], st, r * Tl, 0, scale), 10, 3)
            per_pair = B * Hq * D * 2.0 * 2.0
            f_ring = per_pair * (Tl * (Tl + 1) / 2 + r * Tl * Tl)
            f_train = per_pair * (T * (T + 1) / 2)
            state_mb = B * Hq * Tl * (D + 2) * 4 / 2**20
            print(f"ring_fold T_loc{Tl} world{world} Hq{Hq}/{Hkv} D{D}: "
                  f"last rank {tr[1]*1e3:8.3f} ms [{tr[0]*1e3:.3f}..{tr[2]*1e3:.3f}] "
                  f"{f_ring/tr[1]/1e12:6.1f} TF/s | attn_train_fwd T{T} "
                  f"{tt[1]*1e3:8.3f} ms [{tt[0]*1e3:.3f}..{tt[2]*1e3:.3f}] "
                  f"{f_train/tt[1]/1e12:6.1f} TF/s | FLOP/s ratio "
                  f"{(f_ring/tr[1])/(f_train/tt[1]):5.2f}")
            print(f"    diagonal fold {t_diag*1e3:7.3f} ms "
                  f"{per_pair*Tl*(Tl+1)/2/t_diag/1e12:6.1f} TF/s   full fold "
                  f"{t_full*1e3:7.3f} ms {per_pair*Tl*Tl/t_full/1e12:6.1f} TF/s   "
                  f"state {state_mb:.1f} MiB read + written per fold")


def bench_moe_w4():
    """Grouped expert GEMM, 4-bit weights (moe_gemm_w4.hip) beside the bf16
    grouped kernel (moe_gemm.hip) at the Mixtral-8x7B shapes: E = 8, gate_up
    N=28672 K=4096 and down N=4096 K=14336; 1, 4, 16, 32 tokens with top-2
    routing spread round-robin over the experts. Three alternating rounds
    per shape (median and spread). Each path cycles through enough copies of
    its weights that a call never finds them in the 256 MB last-level cache.
    TB/s is the bytes of the ACTIVE experts' weights (codes + scale + zero
    for W4) over the time."""
    E = 8
    gen = torch.Generator(device=DEV).manual_seed(0)
    for N, K, tag in [(28672, 4096, "gate_up"), (4096, 14336, "down")]:
        wb = torch.randn(E, N, K, generator=gen, device=DEV,
                         dtype=torch.float32).mul_(K ** -0.5).to(torch.bfloat16)
        packed, scale, zero = ops.quant4_pack(wb)
        packed = packed.reshape(E, N, K // 2)
        scale, zero = scale.reshape(E, N, K // 64), zero.reshape(E, N, K // 64)
        w4_bytes = N * K // 2 + 4 * N * K // 64          # per expert
        bf_bytes = N * K * 2
        for T in (1, 4, 16, 32):
            S = 2 * T
            fe = (torch.arange(S) % E)                     # slot t*2+j -> expert
            order = fe.argsort(stable=True)
            counts = torch.bincount(fe, minlength=E)
            active = int((counts > 0).sum())
            off = torch.zeros(E + 1, dtype=torch.int32)
            off[1:] = counts.cumsum(0).int()
            off = off.to(DEV)
            tok = (order // 2).int().to(DEV)
            sc = torch.rand(S, device=DEV)
            # gate_up gathers token rows; down consumes sorted slot rows
            gather = tag == "gate_up"
            a = torch.randn(T if gather else S, K, generator=gen, device=DEV,
                            dtype=torch.float32).to(torch.bfloat16)
            rm, ss = (tok, None) if gather else (None, sc)
            mch = (T + 31) // 32
            nrot4 = max(2, -(-(768 << 20) // (active * w4_bytes)))
            nrotb = max(2, -(-(768 << 20) // (active * bf_bytes)))
            nrot4, nrotb = min(nrot4, 12), min(nrotb, 4)
            w4s = [(packed.clone(), scale.clone(), zero.clone()) for _ in range(nrot4)]
            wbs = [wb.clone() for _ in range(nrotb)]
            i4, ib = [0], [0]

            def run4(ks=0):
                p, s, z = w4s[i4[0] % nrot4]
                i4[0] += 1
                return ops.hip_ops.moe_gemm_w4(a, p, s, z, off, rm, ss, S, mch, ks)

            def runb():
                w = wbs[ib[0] % nrotb]
                ib[0] += 1
                return ops.hip_ops.moe_gemm(a, w, off, rm, ss, S, mch)

            t4, tb, t1 = [], [], []
            for _ in range(3):
                t4.append(_event_time(run4, 40, 8))
                tb.append(_event_time(runb, 40, 8))
                t1.append(_event_time(lambda: run4(1), 40, 8))
            t4.sort(), tb.sort(), t1.sort()
            print(f"moe_w4 {tag} E{E} N{N} K{K} T{T} ({active} active): "
                  f"w4 {t4[1]*1e6:7.1f} us [{t4[0]*1e6:.1f}..{t4[2]*1e6:.1f}] "
                  f"{active*w4_bytes/t4[1]/1e12:5.2f} TB/s   "
                  f"w4 ksplit=1 {t1[1]*1e6:7.1f} us [{t1[0]*1e6:.1f}..{t1[2]*1e6:.1f}]   "
                  f"bf16 {tb[1]*1e6:7.1f} us [{tb[0]*1e6:.1f}..{tb[2]*1e6:.1f}] "
                  f"{active*bf_bytes/tb[1]/1e12:5.2f} TB/s   "
                  f"bf16/w4 {tb[1]/t4[1]:4.2f}", flush=True)
            del w4s, wbs


def bench_w4_tiled():
    """gemm_w4 above 32 rows (w4_gemm_tiled.hip) beside the path it replaces
    in linear_w4 (quant4_unpack + F.linear + residual add, what
    BBAMD_W4_TILED=0 runs) on the same inputs, at the llama-3-8b projections
    and M = 33..1024. Three alternating rounds per point (median and
    spread). Both paths cycle through enough copies of the codes that a call
    never finds them in the 256 MB last-level cache. TB/s is codes + scale +
    zero over the kernel's time, TF/s is 2 M N K over it; `plan` is (BM,
    ksplit, kchunk) from gemm_w4_tiled_plan. BBAMD_BENCH_W4_KSPLIT="1,2,4"
    adds the kernel's time at those forced splits."""
    forced = [int(s) for s in os.environ.get("BBAMD_BENCH_W4_KSPLIT", "").split(",") if s]
    gen = torch.Generator(device=DEV).manual_seed(0)
    for N, K, tag in [(6144, 4096, "qkv"), (4096, 4096, "o"),
                      (28672, 4096, "gate_up"), (4096, 14336, "down")]:
        wb = torch.randn(N, K, generator=gen, device=DEV,
                         dtype=torch.float32).mul_(K ** -0.5).to(torch.bfloat16)
        packed, scale, zero = ops.quant4_pack(wb)
        del wb
        w4_bytes = N * K // 2 + 4 * N * K // 64
        nrot = max(2, -(-(512 << 20) // w4_bytes))
        ws = [(packed.clone(), scale.clone(), zero.clone()) for _ in range(nrot)]
        for M in (33, 48, 64, 96, 128, 192, 256, 384, 512, 1024):
            a = torch.randn(M, K, generator=gen, device=DEV,
                            dtype=torch.float32).to(torch.bfloat16)
            r = torch.randn(M, N, generator=gen, device=DEV,
                            dtype=torch.float32).to(torch.bfloat16)
            i = [0]

            def kernel(ks=0):
                p, s, z = ws[i[0] % nrot]
                i[0] += 1
                return ops.hip_ops.gemm_w4(a, p.view(N, K // 2), s.view(N, K // 64),
                                           z.view(N, K // 64), r, None, N, ks)

            def parent():
                p, s, z = ws[i[0] % nrot]
                i[0] += 1
                w = ops.quant4_unpack(p.view(-1, 32), s.view(-1), z.view(-1)).view(N, K)
                return torch.nn.functional.linear(a, w) + r

            tk, tp = [], []
            for _ in range(3):
                tk.append(_event_time(kernel, 20, 5))
                tp.append(_event_time(parent, 20, 5))
            tk.sort(), tp.sort()
            extra = "".join(
                f"  ks={ks} {_event_time(lambda: kernel(ks), 20, 5)*1e6:.1f} us"
                for ks in forced)
            plan = tuple(ops.hip_ops.gemm_w4_tiled_plan(M, N, K, 0))
            print(f"w4_tiled {tag} N{N} K{K} M{M} plan {plan}: "
                  f"kernel {tk[1]*1e6:7.1f} us [{tk[0]*1e6:.1f}..{tk[2]*1e6:.1f}] "
                  f"{w4_bytes/tk[1]/1e12:5.2f} TB/s {2.0*M*N*K/tk[1]/1e12:6.1f} TF/s   "
                  f"unpack+library {tp[1]*1e6:7.1f} us [{tp[0]*1e6:.1f}..{tp[2]*1e6:.1f}]   "
                  f"parent/kernel {tp[1]/tk[1]:5.2f}{extra}", flush=True)
        del ws


def bench_w8():
    """The fp8 (e4m3) weight tier's decode GEMM (gemm_w8.hip) at the
    llama-3-8b projections, M = 1, 8, 32: hip_w8.gemm_w8 at its own plan and
    cache policy, the row-quantise launch on its own, and beside them on the
    same weight ops.linear with the packed bf16 copy and ops.linear_w4. Each
    path cycles through enough copies of its weight that a call never finds
    it in the 256 MB last-level cache; three alternating rounds per point,
    median of medians. TB/s is the fp8 codes over the kernel's time.
    BBAMD_BENCH_W8_KSPLIT="1,2,4" adds gemm_w8 at those forced splits and
    both cache policies."""
    forced = [int(s) for s in os.environ.get("BBAMD_BENCH_W8_KSPLIT", "").split(",") if s]
    gen = torch.Generator(device=DEV).manual_seed(0)
    for N, K, tag in [(6144, 4096, "qkv"), (4096, 4096, "o"),
                      (28672, 4096, "gate_up"), (4096, 14336, "down")]:
        wb = torch.randn(N, K, generator=gen, device=DEV,
                         dtype=torch.float32).mul_(K ** -0.5).to(torch.bfloat16)
        codes, w_scale = ops.quant_w8(wb)
        nrot = max(2, -(-(512 << 20) // (N * K)))
        w8s = [ops.pack_w8(codes) for _ in range(nrot)]
        w16 = [(wb.clone(), ops.pack_skinny_w(wb)) for _ in range(nrot)]
        w4s = [ops.quant4_pack(wb) for _ in range(nrot)]
        for M in (1, 8, 32):
            a = torch.randn(M, K, generator=gen, device=DEV,
                            dtype=torch.float32).to(torch.bfloat16)
            a8, a_scale = ops.hip_w8.quant_rows_fp8(a)
            i = [0]

            def w8(ks=0, nt=0):
                i[0] += 1
                return ops.hip_w8.gemm_w8(a8, a_scale, w8s[i[0] % nrot], w_scale,
                                          None, None, N, ks, nt)

            def bf16():
                i[0] += 1
                w, wp = w16[i[0] % nrot]
                return ops.linear(a, w, w_packed=wp)

            def w4():
                i[0] += 1
                p, s, z = w4s[i[0] % nrot]
                return ops.linear_w4(a, p, s, z, N)

            fns = (w8, lambda: ops.hip_w8.quant_rows_fp8(a), bf16, w4)
            rounds = [[_event_time(f, 30, 5) for f in fns] for _ in range(3)]
            ts = [sorted(r[j] for r in rounds)[1] for j in range(len(fns))]
            extra = "".join(
                f"  ks={ks},nt={nt} {_event_time(lambda: w8(ks, nt), 30, 5)*1e6:.1f}"
                for ks in forced for nt in (-1, 1))
            plan = tuple(ops.hip_w8.gemm_w8_plan(N, K, 0))
            print(f"w8 {tag} N{N} K{K} M{M} plan {plan}: gemm_w8 {ts[0]*1e6:6.1f} us "
                  f"{N*K/ts[0]/1e12:5.2f} TB/s  quant_rows {ts[1]*1e6:5.1f} us  "
                  f"bf16 packed {ts[2]*1e6:6.1f} us  linear_w4 {ts[3]*1e6:6.1f} us  "
                  f"bf16/(w8+quant) {ts[2]/(ts[0]+ts[1]):5.2f}{extra}", flush=True)
        del w8s, w16, w4s


def bench_w8_tiled():
    """The fp8 weight tier above 32 rows (gemm_w8_tiled.hip) at the llama-3-8b
    projections, M = 64 .. 4096: (a) quant_rows_fp8 + gemm_w8_tiled as
    ops.linear_w8 runs them, and the GEMM alone; (b) the parent's path,
    ops.linear_w8 under BBAMD_W8_TILED=0 (torch composition); (c) for
    information ops.linear on the bf16 weight. Three alternating rounds per
    point, median of 30 device-event times each, median round and spread;
    every path cycles through >= 512 MB of weight copies. TF/s is 2 M N K
    and TB/s the fp8 codes over the GEMM's time; `bound` names the larger of
    the two as fractions of 5 PF/s fp8 and 8 TB/s; `plan` is (BM, m-tiles,
    ksplit, kchunk). BBAMD_BENCH_W8_KSPLIT="1,2,4" adds the GEMM at those
    forced splits."""
    forced = [int(s) for s in os.environ.get("BBAMD_BENCH_W8_KSPLIT", "").split(",") if s]
    gen = torch.Generator(device=DEV).manual_seed(0)
    for N, K, tag in [(6144, 4096, "qkv"), (4096, 4096, "o"),
                      (28672, 4096, "gate_up"), (4096, 14336, "down")]:
        wb = torch.randn(N, K, generator=gen, device=DEV,
                         dtype=torch.float32).mul_(K ** -0.5).to(torch.bfloat16)
        codes, w_scale = ops.quant_w8(wb)
        nrot = max(2, -(-(512 << 20) // (N * K)))
        w8s = [ops.pack_w8(codes) for _ in range(nrot)]
        w16 = [wb.clone() for _ in range((nrot + 1) // 2)]
        del codes
        for M in (64, 128, 256, 512, 1024, 2048, 4096):
            a = torch.randn(M, K, generator=gen, device=DEV,
                            dtype=torch.float32).to(torch.bfloat16)
            a8, a_scale = ops.hip_w8.quant_rows_fp8(a)
            i = [0]

            def gemm(ks=0):
                i[0] += 1
                return ops.hip_w8.gemm_w8_tiled(a8, a_scale, w8s[i[0] % nrot],
                                                w_scale, None, None, N, ks)

            def entry():
                i[0] += 1
                return ops.linear_w8(a, w8s[i[0] % nrot], w_scale, N)

            def kernel():
                os.environ["BBAMD_W8_TILED"] = "1"
                return entry()

            def parent():
                os.environ["BBAMD_W8_TILED"] = "0"
                return entry()

            def bf16():
                i[0] += 1
                return ops.linear(a, w16[i[0] % len(w16)])

            fns = (kernel, gemm, parent, bf16)
            rounds = [[_event_time(f, 30, 3) for f in fns] for _ in range(3)]
            os.environ.pop("BBAMD_W8_TILED", None)
            lo, ts, hi = ([sorted(r[j] for r in rounds)[q] for j in range(len(fns))]
                          for q in range(3))
            extra = "".join(f"  ks={ks} {_event_time(lambda: gemm(ks), 30, 3)*1e6:.1f} us"
                            for ks in forced)
            tf, tb = 2.0 * M * N * K / ts[1] / 1e12, N * K / ts[1] / 1e12
            plan = tuple(ops.hip_w8.gemm_w8_tiled_plan(M, N, K, 0))
            print(f"w8_tiled {tag} N{N} K{K} M{M} plan {plan}: "
                  f"quant+gemm {ts[0]*1e6:8.1f} us [{lo[0]*1e6:.1f}..{hi[0]*1e6:.1f}]  "
                  f"gemm {ts[1]*1e6:8.1f} us {tf:7.1f} TF/s {tb:5.2f} TB/s "
                  f"bound {'mfma' if tf / 5000 > tb / 8 else 'stream'}   "
                  f"composition {ts[2]*1e6:9.1f} us [{lo[2]*1e6:.1f}..{hi[2]*1e6:.1f}]   "
                  f"bf16 library {ts[3]*1e6:8.1f} us   "
                  f"parent/kernel {ts[2]/ts[0]:6.2f}  bf16/kernel {ts[3]/ts[0]:5.2f}{extra}",
                  flush=True)
        del w8s, w16


ALL = {
    "attn_decode": bench_attn_decode,
    "attn_decode_fp8": bench_attn_decode_fp8,
    "attn_mixed": bench_attn_mixed,
    "attn_sparse": bench_attn_sparse,
    "attn_prefill": bench_attn_prefill,
    "attn_prefill_wide": bench_attn_prefill_wide,
    "train_attn": bench_train_attn,
    "kv_stream": bench_kv_stream,
    "norms": bench_norms,
    "layer_norm": bench_layer_norm,
    "swiglu": bench_swiglu,
    "gemm": bench_gemm,
    "gemm_norm": bench_gemm_norm,
    "ring_fold": bench_ring_fold,
    "moe_w4": bench_moe_w4,
    "w4_tiled": bench_w4_tiled,
    "w8": bench_w8,
    "w8_tiled": bench_w8_tiled,
}

if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("bench_kernels measures the gfx950 HIP kernels — "
                 "run on a GPU box (e.g. via gpurun)")
    which = sys.argv[1:] or list(ALL)
    for name in which:
        ALL[name]()
