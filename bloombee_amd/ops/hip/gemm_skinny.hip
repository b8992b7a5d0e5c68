// Skinny-M GEMM for gfx950: C(M,N) = A(M,K) @ W(N,K)^T [+ residual] [+ bias],
// M <= 32 — the decode-step projection shape (batch tokens x weight matrix).
//
// Decode GEMMs are pure weight streams: the job is to read W (N*K*2 bytes)
// once at full HBM bandwidth. hipBLASLt's skinny-M solutions measure
// ~2.6-4.4 TB/s on these shapes (profiles/r01_decode_kernel_stats.md); this
// kernel exists to close that gap. Replaces the reference's decode-path
// torch.matmul projections (flexgen_utils/pytorch_backend.py:733-916).
//
// Decomposition: grid = (N/64, ksplit); 4 waves per 256-thread workgroup,
// wave w owns 16 N-rows of W. B-fragments (8 consecutive k at fixed n) are
// direct contiguous 16 B loads from W; with the k-loop unrolled 4x each W row
// is streamed in 256 B sequential pieces. A (<= 32xK bf16, a few hundred KB)
// is re-read per wave but L2-resident after the first touch. No LDS at all.
//
// Split-K (ksplit > 1) for small-N shapes that would otherwise leave the
// chip idle (N=4096 -> only 64 workgroups): each split writes an f32 partial
// (ksplit, M, N); gemm_skinny_combine_kernel folds them + residual/bias and
// converts to bf16.

#include "common.h"

template <int MT>  // number of 16-row M-tiles (1: M<=16, 2: M<=32)
__global__ __launch_bounds__(256) void gemm_skinny_kernel(
    const unsigned short* __restrict__ A,   // (M, K) bf16
    const unsigned short* __restrict__ W,   // (N, K) bf16
    const unsigned short* __restrict__ R,   // (M, N) bf16 residual or null
    const unsigned short* __restrict__ bias,  // (N,) bf16 or null
    unsigned short* __restrict__ C,         // (M, N) bf16   (ksplit == 1)
    float* __restrict__ Cpart,              // (ksplit, M, N) f32 (ksplit > 1)
    int M, int N, int K, int ksplit) {
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int li = lane & 15;
  const int hi = lane >> 4;
  const int n0 = blockIdx.x * 64 + wave * 16;
  if (n0 >= N) return;
  const int split = blockIdx.y;
  const int kchunk = ((K / 32 + ksplit - 1) / ksplit) * 32;
  const int k0 = split * kchunk;
  const int k1 = min(K, k0 + kchunk);

  const unsigned short* wrow = W + (long)(n0 + li) * K;
  // A rows this lane feeds (garbage-row trick for M not a multiple of 16:
  // clamped rows compute garbage C rows that are simply not stored).
  int arow[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) arow[t] = min(t * 16 + li, M - 1);

  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  int k = k0;
  for (; k + 128 <= k1; k += 128) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int kk = k + u * 32 + hi * 8;
      bf16x8 bfrag = as_bf16x8(*reinterpret_cast<const short8*>(wrow + kk));
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        bf16x8 afrag = as_bf16x8(
            *reinterpret_cast<const short8*>(A + (long)arow[t] * K + kk));
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag, bfrag, acc[t],
                                                         0, 0, 0);
      }
    }
  }
  for (; k < k1; k += 32) {
    const int kk = k + hi * 8;
    bf16x8 bfrag = as_bf16x8(*reinterpret_cast<const short8*>(wrow + kk));
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      bf16x8 afrag = as_bf16x8(
          *reinterpret_cast<const short8*>(A + (long)arow[t] * K + kk));
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag, bfrag, acc[t],
                                                       0, 0, 0);
    }
  }

  // C layout: row = t*16 + hi*4 + reg, col = n0 + li.
  if (ksplit == 1) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int m = t * 16 + hi * 4 + reg;
        if (m >= M) continue;
        float v = acc[t][reg];
        if (bias) v += bf2f(bias[n0 + li]);
        if (R) v += bf2f(R[(long)m * N + n0 + li]);
        C[(long)m * N + n0 + li] = f2bf(v);
      }
  } else {
    float* dst = Cpart + (long)split * M * N;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int m = t * 16 + hi * 4 + reg;
        if (m >= M) continue;
        dst[(long)m * N + n0 + li] = acc[t][reg];
      }
  }
}

// Split-K combine epilogue for one lane: folds the ksplit f32 slabs of row m,
// columns n0+c4..+3 in split order, then bias, then residual, stores bf16 and
// (ssout) emits the stripe's row sum-of-squares through a 16-lane butterfly.
// Shared by gemm_skinny_combine_ss_kernel and the in-launch reducer of
// gemm_skinny_v2_kernel<MT, 2> so both produce the same bits. The slabs are
// NOT __restrict__/const: the in-launch reducer reads bytes other workgroups
// of the same launch wrote, which must stay on the vector-load path.
DEVINL void gemm_skinny_combine_lane(
    const float* Cpart, const unsigned short* __restrict__ R,
    const unsigned short* __restrict__ bias, unsigned short* __restrict__ C,
    float* __restrict__ ssout, int M, int N, int ksplit, int stripe, int m,
    int lane) {
  const int n0 = stripe * 64;
  const int c4 = (lane & 15) * 4;            // first of this lane's 4 cols
  const long total = (long)M * N;
  const long i = (long)m * N + n0 + c4;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < ksplit; ++s) {
    const f32x4 p = *reinterpret_cast<const f32x4*>(Cpart + s * total + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += p[e];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (bias) v[e] += bf2f(bias[n0 + c4 + e]);
    if (R) v[e] += bf2f(R[i + e]);
  }
  short4v o4;
#pragma unroll
  for (int e = 0; e < 4; ++e) o4[e] = (short)f2bf(v[e]);
  *reinterpret_cast<short4v*>(C + i) = o4;
  if (ssout) {
    float vs = v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
#pragma unroll
    for (int msk = 1; msk < 16; msk <<= 1) vs += __shfl_xor(vs, msk);
    if ((lane & 15) == 0) ssout[(long)stripe * 32 + m] = vs;
  }
}

// v2: software-pipelined direct-VGPR W streaming + A through LDS.
// The guide's verdicts for this shape class (cdna_hip_programming.md):
//  * "GEMV / M <= 16 decode weights" — W is streamed once and not shared
//    across waves: no LDS round trip, load straight to VGPRs, deep unroll,
//    late vmcnt. Two register sets alternate so each wave keeps a
//    HBM-latency's worth of W bytes in flight.
//  * "the x operand ... through LDS in full 128-B lines, NOT fragment-shaped
//    loads straight to VGPRs" — per-fragment A loads double TA pressure
//    (+18..45% measured in the guide); here the (M x 256) A stage is copied
//    to LDS once per stage with full-line loads and A fragments come from
//    conflict-free padded ds_read_b128.
// Host guarantees (k1 - k0) % 256 == 0 so the set pairing needs no tail.
//
// EPI selects the epilogue; the main loop is shared.
//  0: C / split-K slabs as described above (every caller before the fused
//     epilogues; its code is what it was).
//  1: SwiGLU of a fused gate|up weight W (2I, K), N = 2I. The grid is I/32
//     workgroups of 32 activation columns: in each wave lanes li < 8 stream
//     gate rows tile*32 + wave*8 + li and lanes li >= 8 the matching up rows
//     I + tile*32 + wave*8 + (li-8), so the weights keep their gate|up layout
//     and every lane still streams one W row. The epilogue rounds both values
//     to bf16 exactly as the plain store would, pairs them with one cross-lane
//     move (8 lanes apart), applies swiglu_kernel's expression and writes
//     C (M, I) in full 64 B rows staged through the dead A tile.
//  2: split-K with the combine inside the launch. The grid is 1-D,
//     (N/64)*ksplit blocks, tile = id / ksplit, slice = id % ksplit after the
//     XCD remap (a tile's slices share an XCD when (N/64) % 8 == 0). Every
//     block stores its slab to Cpart with 16 B stores, releases at agent
//     scope and draws a ticket from cnt[tile]; the block that draws ksplit-1
//     acquires, folds all slabs with gemm_skinny_combine_lane (the separate
//     combine kernel's epilogue, same bits) and resets the counter. Nobody
//     waits on anybody: no polling, nothing to hang.
//
// DEPTH is the number of W register sets (4 KB per wave each) a wave keeps
// requested. 2 is the form described above: one set outstanding at each wait.
// DEPTH > 2 is a ring: the A stage grows to one ring period (DEPTH * 128 k),
// the prologue requests A first and then the whole ring, and each set is
// re-requested for the next period as soon as its MFMAs have consumed it, so
// DEPTH - 1 sets stay in flight at every wait. vmcnt retires in order, which
// fixes the order of issue: the next period's A is requested BEFORE this
// period's re-requests, so the wait for it at the period's end leaves all
// DEPTH sets flying. Register sets are indexed statically: the loop body is
// one unrolled period with every request unconditional, and the last one or
// two periods are peeled per remaining set count (a conditional request would
// make the compiler's wait counts assume the shortest path and drain the
// ring). Per accumulator the MFMA order is k ascending in steps of 32 at
// every DEPTH, so all depths produce the same bits. Norm mode 1 exists at
// DEPTH 2 only (the host never launches the ring with it).
//
// PACKED (DEPTH 2 only): W is the pre-tiled copy of common.h's
// skinny_packed_offset — one 1 KB lane-linear block per (16-row group,
// 32-k slice), a wave's blocks consecutive in k. A wave load is then one
// contiguous 1 KB instead of 16 rows x 64 B at a 2K-byte stride, a set is
// 4 KB and the wave's whole stream one contiguous run; the block base is
// wave-uniform (scalar registers) and the lanes add lane * 16 bytes. Every
// lane receives the very 8 elements the row-major expression gives it, so
// the MFMA operands, their order and the outputs are bit-identical.
//
// NT: the W loads (issue0 / issue1, the ring's issue) carry the nontemporal
// hint, as the decode attention kernel's K/V loads do: W is read once, and
// the lines every workgroup re-reads (A, ssin, R, the split-K slabs) should
// not be evicted by it. Only the cache policy bit of those loads differs; A
// staging, nw, ssin, R, bias, the slab loads and every store keep the default
// policy. NT = false is the kernel as it was.
template <int I>
struct WringIdx {
  static constexpr int value = I;
};

// f(WringIdx<n>) for the even n in [N, 2 * DEPTH - 2] equal to nrem
template <int DEPTH, int N, typename F>
DEVINL void wring_tail_dispatch(int nrem, F& f) {
  if constexpr (N <= 2 * DEPTH - 2) {
    if (nrem == N) f(WringIdx<N>{});
    else wring_tail_dispatch<DEPTH, N + 2>(nrem, f);
  }
}

template <int MT, int EPI, int DEPTH, bool PACKED = false, bool NT = false>
DEVINL void gemm_skinny_v2_body(
    const unsigned short* __restrict__ A,   // (M, K) bf16
    const unsigned short* __restrict__ W,   // (N, K) bf16, or its packed copy
    const unsigned short* __restrict__ R,   // (M, N) bf16 residual or null
    const unsigned short* __restrict__ bias,  // (N,) bf16 or null
    unsigned short* __restrict__ C,         // (M, N) bf16   (ksplit == 1)
    float* __restrict__ Cpart,              // (ksplit, M, N) f32 (ksplit > 1)
    int M, int N, int K, int kchunk, int ksplit,
    const unsigned short* __restrict__ nw,  // (K,) rmsnorm weight (mode 1)
    float eps, int norm_mode,  // 0: none; 1: scale A by invr*nw (stage path);
                               // 2: weight pre-folded into W — scale the
                               //    ACCUMULATOR by invr in the epilogue
                               //    (zero per-stage cost; the production path)
    const float* __restrict__ ssin,   // (nstripes, 32) producer row sum-sq
    int nstripes,
    float* __restrict__ ssout,        // (N/64, 32) this GEMM's row sum-sq
    int* cnt) {             // EPI 2: (N/64,) tickets, zero on entry
  static_assert(DEPTH == 2 || DEPTH % 4 == 0, "ring: whole waves per A row");
  static_assert(!PACKED || (DEPTH == 2 && EPI != 2),
                "packed W: depth 2, plain and SwiGLU epilogues only");
  constexpr int U = 4;                     // k-slices per pipeline set (128 k)
  constexpr int KSTEP = DEPTH * 128;       // A elements staged per stage
  constexpr int RSTRIDE = KSTEP + 8;       // padded LDS row stride (elements)
  constexpr int RPIECE = KSTEP / 8;        // 16 B pieces per staged A row
  constexpr int NPIECE = (32 * KSTEP) / (256 * 8);  // pieces per thread
  __shared__ __attribute__((aligned(16))) unsigned short atile[32 * RSTRIDE];
  // Fused rmsnorm of A (nw != null): removes the separate rms_norm launch +
  // its read/write from the decode step (launch-count reduction — the PMC
  // work in profiles/r02 §11 showed the in-context GEMM cost is boundary/
  // drain, not cache, so fewer kernels is the lever). Each WG redundantly
  // streams A (M*K bf16, L2-resident after the first WG) to compute per-row
  // inv-rms, then scales A fragments by invr[m]*nw[k] as they stage to LDS.
  __shared__ float ssp[256];
  __shared__ float invr[32];

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int li = lane & 15;
  const int hi = lane >> 4;
  // each XCD streams one contiguous W region (common.h)
  int tile = xcd_remap(blockIdx.x, gridDim.x);
  int split = blockIdx.y;
  if constexpr (EPI == 2) {
    split = tile % ksplit;
    tile /= ksplit;
  }
  const int n0 = tile * 64 + wave * 16;
  const int k0 = split * kchunk;
  const int k1 = min(K, k0 + kchunk);

  const unsigned short* wrow = W + (long)(n0 + li) * K;
  if constexpr (EPI == 1)
    wrow = W + ((long)(li < 8 ? 0 : N / 2 - 8) + tile * 32 + wave * 8 + li) * K;
  // PACKED: the wave's group is tile * 4 + wave under both row maps; its
  // blocks start at skinny_packed_offset(group, 0, K) and follow in k.
  if constexpr (PACKED)
    wrow = W + skinny_packed_offset(
                   tile * 4 + __builtin_amdgcn_readfirstlane(wave), 0, K) +
           lane * 8;

  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // ---- A staging: the whole workgroup copies A[0:M][ks:ks+256] with
  // full-line loads; rows beyond M-1 are clamped (their C rows are dropped).
  // Thread piece j: row = (tid + j*256)/RPIECE clamped, 8 elements at
  // ((tid + j*256)%RPIECE)*8 within the stage. `lim` (a multiple of 128) is
  // how much of the stage lies inside the split: pieces past it re-read the
  // last valid one and are never consumed.
  short8 aregs[NPIECE];                    // 4 pieces per thread at DEPTH 2
  // matching norm-weight pieces (mode 1). The ring spends these registers on
  // W: mode 1 is not built for it and the host keeps such calls at DEPTH 2.
  short8 nregs[DEPTH == 2 ? NPIECE : 1];
  // In the ring a wave's piece j is 64 consecutive pieces of ONE row (RPIECE
  // is a multiple of 64): the row part of the address is wave-uniform and
  // stays in scalar registers, the lanes share one 32-bit byte offset.
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  auto load_a = [&](int ks, int lim = 1 << 30) {
#pragma unroll
    for (int j = 0; j < NPIECE; ++j) {
      if constexpr (DEPTH == 2) {
        const int flat = threadIdx.x + j * 256;
        const int row = min(flat / RPIECE, M - 1);
        const int off = (flat % RPIECE) * 8;
        aregs[j] = *reinterpret_cast<const short8*>(A + (long)row * K + ks + off);
        if (norm_mode == 1)
          nregs[j] = *reinterpret_cast<const short8*>(nw + ks + off);
      } else {
        const int fw = wave_s + j * 4;       // (tid + j*256) / 64
        const int row = min(fw / (RPIECE / 64), M - 1);
        const unsigned off =
            min((fw % (RPIECE / 64)) * 64 + lane, lim / 8 - 1) * 16u;  // bytes
        aregs[j] = *reinterpret_cast<const short8*>(
            reinterpret_cast<const char*>(A + (long)row * K + ks) + off);
      }
    }
  };
  auto store_a = [&]() {
#pragma unroll
    for (int j = 0; j < NPIECE; ++j) {
      const int flat = threadIdx.x + j * 256;
      short8 v = aregs[j];
      if (DEPTH == 2 && norm_mode == 1) {
        const float ir = invr[flat / RPIECE >= M ? M - 1 : flat / RPIECE];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          v[e] = (short)f2bf(bf2f((unsigned short)v[e]) * ir *
                             bf2f((unsigned short)nregs[j][e]));
      }
      *reinterpret_cast<short8*>(atile + (flat / RPIECE) * RSTRIDE +
                                 (flat % RPIECE) * 8) = v;
    }
  };

  bf16x8 bB0[U], bB1[U];
  // one 16 B piece of the W stream
  auto load_w = [&](const unsigned short* p) -> short8 {
    if constexpr (NT)
      return __builtin_nontemporal_load(reinterpret_cast<const short8*>(p));
    else
      return *reinterpret_cast<const short8*>(p);
  };
  // slice u of the DEPTH 2 set at k: where this lane's 8 elements are
  auto wptr = [&](int k, int u) -> const unsigned short* {
    if constexpr (PACKED) return wrow + (k / 32 + u) * SKINNY_PACK_BLOCK;
    else return wrow + k + u * 32 + hi * 8;
  };
  auto issue0 = [&](int k) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      bB0[u] = as_bf16x8(load_w(wptr(k, u)));
  };
  auto issue1 = [&](int k) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      bB1[u] = as_bf16x8(load_w(wptr(k, u)));
  };
  // A fragment for m-tile t, k-slice u of 128-k set `half` of the stage:
  // ds_read_b128 at row (t*16 + li), element (half*128 + u*32 + hi*8) — the
  // row stride is 16 B past a multiple of 512 B => lanes hit distinct banks.
  auto mfma_set = [&](bf16x8* bB, int half) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        bf16x8 afrag = as_bf16x8(*reinterpret_cast<const short8*>(
            atile + (t * 16 + li) * RSTRIDE + half * 128 + u * 32 + hi * 8));
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag, bB[u], acc[t],
                                                         0, 0, 0);
      }
  };

  // invr reduce from producer stats (coalesced: lanes sweep each stripe's
  // contiguous 32 floats; 4 accumulator chains keep loads in flight) or
  // from re-streaming A (fallback for callers with no producer stats —
  // +18-60 us/GEMM under split-K, profiles/r02 §13).
  auto reduce_invr = [&]() {
    if (ssin) {
      const int row = threadIdx.x & 31, grp = threadIdx.x >> 5;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
      int s = grp;
      for (; s + 24 < nstripes; s += 32) {
        s0 += ssin[(long)s * 32 + row];
        s1 += ssin[(long)(s + 8) * 32 + row];
        s2 += ssin[(long)(s + 16) * 32 + row];
        s3 += ssin[(long)(s + 24) * 32 + row];
      }
      for (; s < nstripes; s += 8) s0 += ssin[(long)s * 32 + row];
      ssp[threadIdx.x] = (s0 + s1) + (s2 + s3);
      __syncthreads();
      if (threadIdx.x < 32) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 8; ++g) t += ssp[g * 32 + threadIdx.x];
        invr[threadIdx.x] = rsqrtf(t / K + eps);
      }
      __syncthreads();
    } else {
      const int row = threadIdx.x >> 3, sub = threadIdx.x & 7;
      float ss = 0.f;
      if (row < M) {
        const unsigned short* p = A + (long)row * K + sub * (K / 8);
        for (int x = 0; x < K / 8; x += 8) {
          short8 v = *reinterpret_cast<const short8*>(p + x);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float f = bf2f((unsigned short)v[e]);
            ss += f * f;
          }
        }
      }
      ssp[threadIdx.x] = ss;
      __syncthreads();
      if (sub == 0 && row < M) {
        float t = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) t += ssp[(row << 3) + e];
        invr[row] = rsqrtf(t / K + eps);
      }
      __syncthreads();
    }
  };

  if constexpr (DEPTH == 2) {
    if (norm_mode == 1) {
      // mode 1 scales A as it stages: invr must exist BEFORE the pipeline.
      // Issue the first W-register set first so the stream is in flight.
      issue0(k0);
      reduce_invr();
      load_a(k0);
      store_a();
      __syncthreads();
    } else {
      // Pipeline: stage s's A sits in LDS while its two B register sets
      // stream; stage s+1's A loads issue right after the barrier frees them.
      // mode 2 defers its invr reduce to just before the epilogue — the
      // weight stream starts with zero added latency.
      load_a(k0);
      issue0(k0);
      store_a();
      __syncthreads();
    }
    for (int k = k0; k < k1; k += KSTEP) {
      if (k + KSTEP < k1) load_a(k + KSTEP);
      issue1(k + 128);
      mfma_set(bB0, 0);
      if (k + KSTEP < k1) issue0(k + KSTEP);
      mfma_set(bB1, 1);
      if (k + KSTEP < k1) {
        __syncthreads();  // everyone done reading stage s
        store_a();
        __syncthreads();
      }
    }
  } else {
    bf16x8 ring[DEPTH][U];
    auto issue = [&](int j, int k) {
#pragma unroll
      for (int u = 0; u < U; ++u)
        ring[j][u] = as_bf16x8(load_w(wrow + k + u * 32 + hi * 8));
    };
    // A stream shorter than the ring re-reads its last set into the spare
    // registers: every request stays unconditional.
    auto issue_ring = [&]() {
#pragma unroll
      for (int j = 0; j < DEPTH; ++j) issue(j, min(k0 + j * 128, k1 - 128));
      __builtin_amdgcn_sched_barrier(0);
    };
    // A first: the wait for it leaves the whole ring in flight
    load_a(k0, min(KSTEP, k1 - k0));
    __builtin_amdgcn_sched_barrier(0);
    issue_ring();
    store_a();
    __syncthreads();
    int k = k0;
    // whole periods with a whole period behind them
    for (; k + 2 * KSTEP <= k1; k += KSTEP) {
      load_a(k + KSTEP);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < DEPTH; ++j) {
        mfma_set(ring[j], j);
        issue(j, k + KSTEP + j * 128);
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();  // everyone done reading this period's A
      store_a();
      __syncthreads();
    }
    // NREM sets are left: min(NREM, DEPTH) in the ring, the rest a partial
    // last period
    auto tail = [&](auto nrem_c) {
      constexpr int NREM = decltype(nrem_c)::value;
      constexpr int CUR = NREM < DEPTH ? NREM : DEPTH;
      constexpr int NEXT = NREM - CUR;
      if constexpr (NEXT > 0) {
        load_a(k + KSTEP, NEXT * 128);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int j = 0; j < CUR; ++j) {
        mfma_set(ring[j], j);
        if (j < NEXT) {
          issue(j, k + KSTEP + j * 128);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if constexpr (NEXT > 0) {
        __syncthreads();
        store_a();
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NEXT; ++j) mfma_set(ring[j], j);
      }
    };
    wring_tail_dispatch<DEPTH, 2>((k1 - k) / 128, tail);
  }

  if (norm_mode == 2) reduce_invr();

  if constexpr (EPI == 1) {
    // C layout per wave: row = t*16 + hi*4 + reg; col li < 8 is gate column
    // tile*32 + wave*8 + li, col li >= 8 the up value of column li - 8.
    unsigned short* otile = atile;          // (32 rows, 32 cols) bf16, dead A
    __syncthreads();                        // every wave is done reading A
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int m = t * 16 + hi * 4 + reg;
        float v = acc[t][reg];
        if (norm_mode == 2) v *= invr[m];
        const float g = bf2f(f2bf(v));      // what the gate_up store rounds to
        const float u = __shfl_xor(g, 8);   // partner lane's up value
        const float sg = g / (1.f + fast_expf(-g));
        if (li < 8) otile[m * 32 + wave * 8 + li] = f2bf(sg * u);
      }
    __syncthreads();
    if (threadIdx.x < 128) {
      const int m = threadIdx.x >> 2, c8 = (threadIdx.x & 3) * 8;
      if (m < M)
        *reinterpret_cast<short8*>(C + (long)m * (N / 2) + tile * 32 + c8) =
            *reinterpret_cast<const short8*>(otile + m * 32 + c8);
    }
    return;
  }

  if constexpr (EPI == 2) {
    // Transpose the accumulators through the dead A tile so the slab goes
    // out row-major in the combine's lane mapping: one 16 B store per lane.
    constexpr int TS = 68;                  // padded f32 row stride
    float* ftile = reinterpret_cast<float*>(atile);   // (32, TS) f32
    __syncthreads();                        // every wave is done reading A
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int m = t * 16 + hi * 4 + reg;
        float v = acc[t][reg];
        if (norm_mode == 2) v *= invr[m];
        ftile[m * TS + wave * 16 + li] = v;
      }
    __syncthreads();
    float* dst = Cpart + (long)split * M * N;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int m = t * 16 + wave * 4 + hi;
      if (m < M)
        *reinterpret_cast<f32x4*>(dst + (long)m * N + tile * 64 + li * 4) =
            *reinterpret_cast<const f32x4*>(ftile + m * TS + li * 4);
    }
    // publish: every storing wave drains, then ONE lane releases at agent
    // scope and draws the ticket (fence before the add, wait in between)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int* flag = reinterpret_cast<int*>(ssp);   // "I am last", existing LDS
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const int ticket = __hip_atomic_fetch_add(
          cnt + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = ticket == ksplit - 1;
      if (last) {
        // all ksplit tickets of this tile are drawn: leave the counter
        // zero for the next launch (graph replays start clean)
        __hip_atomic_store(cnt + tile, 0, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      flag[0] = last;
    }
    __syncthreads();
    if (!flag[0]) return;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int m = t * 16 + wave * 4 + hi;
      if (m < M)
        gemm_skinny_combine_lane(Cpart, R, bias, C, ssout, M, N, ksplit, tile,
                                 m, lane);
    }
    return;
  }

  if (ksplit == 1) {
    if (ssout == nullptr) {
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int m = t * 16 + hi * 4 + reg;
          if (m >= M) continue;
          float v = acc[t][reg];
          if (norm_mode == 2) v *= invr[m];
          if (bias) v += bf2f(bias[n0 + li]);
          if (R) v += bf2f(R[(long)m * N + n0 + li]);
          C[(long)m * N + n0 + li] = f2bf(v);
        }
    } else {
      // Emit per-stripe row sum-of-squares alongside the store: li-group
      // shfl reduce (16 cols per wave), cross-wave fold via ssp. The next
      // GEMM's fused rmsnorm sums these instead of re-streaming A.
      __syncthreads();  // atile is dead; reuse ssp[wave*32 + m]
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int m = t * 16 + hi * 4 + reg;
          float vs = 0.f;
          if (m < M) {
            float v = acc[t][reg];
            if (norm_mode == 2) v *= invr[m];
            if (bias) v += bf2f(bias[n0 + li]);
            if (R) v += bf2f(R[(long)m * N + n0 + li]);
            C[(long)m * N + n0 + li] = f2bf(v);
            vs = v * v;
          }
#pragma unroll
          for (int msk = 1; msk < 16; msk <<= 1) vs += __shfl_xor(vs, msk);
          if (li == 0) ssp[wave * 32 + m] = vs;
        }
      __syncthreads();
      if (threadIdx.x < 32)
        ssout[(long)tile * 32 + threadIdx.x] =
            ssp[threadIdx.x] + ssp[32 + threadIdx.x] +
            ssp[64 + threadIdx.x] + ssp[96 + threadIdx.x];
    }
  } else {
    float* dst = Cpart + (long)split * M * N;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int m = t * 16 + hi * 4 + reg;
        if (m >= M) continue;
        float v = acc[t][reg];
        if (norm_mode == 2) v *= invr[m];
        dst[(long)m * N + n0 + li] = v;
      }
  }
}

// The kernels proper. DEPTH 2 keeps the name and the launch bounds it has
// always had; the ring asks for 3 workgroups per CU (the qkv grid places 3),
// which caps it at 168 registers.
#define SKINNY_V2_PARAMS                                                      \
  const unsigned short *__restrict__ A, const unsigned short *__restrict__ W, \
      const unsigned short *__restrict__ R,                                   \
      const unsigned short *__restrict__ bias, unsigned short *__restrict__ C, \
      float *__restrict__ Cpart, int M, int N, int K, int kchunk, int ksplit, \
      const unsigned short *__restrict__ nw, float eps, int norm_mode,        \
      const float *__restrict__ ssin, int nstripes, float *__restrict__ ssout, \
      int *cnt
#define SKINNY_V2_ARGS                                                       \
  A, W, R, bias, C, Cpart, M, N, K, kchunk, ksplit, nw, eps, norm_mode, ssin, \
      nstripes, ssout, cnt

template <int MT, int EPI = 0, bool PACKED = false, bool NT = false>
__global__ __launch_bounds__(256) void gemm_skinny_v2_kernel(SKINNY_V2_PARAMS) {
  gemm_skinny_v2_body<MT, EPI, 2, PACKED, NT>(SKINNY_V2_ARGS);
}

template <int MT, int EPI, int DEPTH, bool NT = false>
__global__ __launch_bounds__(256, 3) void gemm_skinny_v2_ring_kernel(
    SKINNY_V2_PARAMS) {
  gemm_skinny_v2_body<MT, EPI, DEPTH, false, NT>(SKINNY_V2_ARGS);
}

// Split-K combine that also emits per-stripe row sum-of-squares (ssout
// layout (N/64, 32)): grid (N/64, ceil(M/16)); a wave covers 4 rows x 16
// float4 column-groups of the 64-col stripe, so partial loads are 16 B
// vectors (16 lanes x 16 B = one coalesced 256 B line run per split per
// row), the row sum is an in-lane fold + a 16-lane shfl reduce, and each
// (stripe, m) is produced by exactly one lane — no LDS, no atomics.
__global__ __launch_bounds__(256) void gemm_skinny_combine_ss_kernel(
    const float* __restrict__ Cpart, const unsigned short* __restrict__ R,
    const unsigned short* __restrict__ bias, unsigned short* __restrict__ C,
    float* __restrict__ ssout, int M, int N, int ksplit) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int m = blockIdx.y * 16 + (threadIdx.x >> 6) * 4 + (lane >> 4);
  if (m >= M) return;
  // the plain index on purpose, not xcd_remap (profiles/r09_nt_weights.md)
  gemm_skinny_combine_lane(Cpart, R, bias, C, ssout, M, N, ksplit, blockIdx.x,
                           m, lane);
}

__global__ void gemm_skinny_combine_kernel(
    const float* __restrict__ Cpart, const unsigned short* __restrict__ R,
    const unsigned short* __restrict__ bias, unsigned short* __restrict__ C,
    int M, int N, int ksplit) {
  const long total = (long)M * N;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    float v = 0.f;
    for (int s = 0; s < ksplit; ++s) v += Cpart[(long)s * total + i];
    if (bias) v += bf2f(bias[i % N]);
    if (R) v += bf2f(R[i]);
    C[i] = f2bf(v);
  }
}
