"""Kernel microbenchmarks on a real MI355X (run via gpurun).

Reports per-kernel time and effective HBM bandwidth / TFLOPs so kernel
changes can be A/B'd without the end-to-end bench's noise.

    python benchmarks/bench_kernels.py [attn_decode attn_mixed attn_prefill train_attn moe_w4 ...]
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


ALL = {
    "attn_decode": bench_attn_decode,
    "attn_mixed": bench_attn_mixed,
    "attn_sparse": bench_attn_sparse,
    "attn_prefill": bench_attn_prefill,
    "train_attn": bench_train_attn,
    "kv_stream": bench_kv_stream,
    "norms": bench_norms,
    "layer_norm": bench_layer_norm,
    "swiglu": bench_swiglu,
    "gemm": bench_gemm,
    "gemm_norm": bench_gemm_norm,
    "moe_w4": bench_moe_w4,
}

if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("bench_kernels measures the gfx950 HIP kernels — "
                 "run on a GPU box (e.g. via gpurun)")
    which = sys.argv[1:] or list(ALL)
    for name in which:
        ALL[name]()
