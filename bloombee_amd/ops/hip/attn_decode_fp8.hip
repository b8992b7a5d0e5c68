// Single-token paged attention over an fp8 (OCP e4m3) KV pool for gfx950.
//
// Same S^T formulation as attn_decode_mfma.hip (scores transposed: A = K,
// B = Q, per-head scalar (m, l), in-lane softmax over positions, then
// O^T = V^T P^T), same grid (B*Hkv*nch, n_split), same 4-wave merge and the
// same (m, l, acc) partials, so attn_decode_combine_kernel serves both. What
// differs is how the bytes move: the bf16 kernel is per-wave-latency-bound
// and keeps 16 B per lane per load in flight; with 1-byte elements its
// 8-element fragments would be 8 B loads and half the bytes in flight. Here
// every load is still 16 B = 16 ELEMENTS, and one load feeds two MFMAs:
//
//  * K pages (np, Hkv, 16, D) token-major. Lane (li, hi) loads, for position
//    row li of a 16-position subtile, the 16 consecutive d
//    [64j + 16hi, 64j + 16hi + 16): one load per position at D = 64, two at
//    D = 128. The low 8 go to k-slice 2j of the 16x16x32 MFMA and the high 8
//    to k-slice 2j+1, i.e. slice s = 2j+c contracts over
//    d = 64j + 16hi + 8c + e (e < 8) at fragment index hi*8 + e. The Q
//    fragments are loaded ONCE with the same permutation of the contraction
//    index; a dot product does not care about the order.
//  * V pages (np, Hkv, D, 16) d-major: a d-row of a page is exactly 16 B. The
//    KV tile is 64 positions = 4 pages; lane (li, hi) loads page hi of the
//    tile at row d = li + 16n. Low 8 positions go to one MFMA, high 8 to a
//    second: MFMA c contracts over position 16hi + 8c + e at fragment index
//    hi*8 + e. P^T is written to LDS in natural position order and its two
//    B-fragments are read back at offset 16hi + 8c, the matching order.
//
// Dequantisation is in registers, e4m3 -> bf16 (common.h fp8x16_to_bf16:
// exact, and no operand is a bf16 subnormal), so K and V enter the bf16 MFMA
// exactly, Q is the caller's bf16 and P is rounded to bf16 as in the bf16
// kernel: the error bound of that kernel holds unchanged against attention
// over the dequantised pages.
//
// Pipeline: register double buffer over 64-position tiles (raw fp8 words,
// 16 VGPRs of K and 8 of V per buffer at D = 64; 32 + 32 at D = 128), next
// tile's K and V issued before the current tile's MFMA / softmax, nontemporal
// loads. Wave w owns tiles w, w+4, ... of its split: the wave stride is 256
// positions and one loop trip covers 512.
//
// Page size is 16 (a V row is one load; a split starts on a page boundary,
// so every 16-position group of a tile is one page).

#include "common.h"

static constexpr int F8BLK = 64;  // positions per KV tile
static constexpr int F8P = 16;    // page size the layout is written for

DEVINL float f8_quad16_max(float x) {
  x = fmaxf(x, __shfl_xor(x, 16));
  return fmaxf(x, __shfl_xor(x, 32));
}
DEVINL float f8_quad16_sum(float x) {
  x += __shfl_xor(x, 16);
  return x + __shfl_xor(x, 32);
}

// launch_bounds(256, 2): up to 256 VGPRs, 2 workgroups per CU -> 512
// workgroups fill the chip (the host's automatic n_split aims for that).
template <int D, int MAXG>
__global__ __launch_bounds__(256, 2) void attn_decode_fp8_kernel(
    const unsigned short* __restrict__ q,       // bf16, strided (q_sb, q_sh)
    const unsigned char* __restrict__ k_pages,  // e4m3 (np, Hkv, 16, D)
    const unsigned char* __restrict__ v_pages,  // e4m3 (np, Hkv, D, 16)
    const int* __restrict__ page_table,         // (B, maxp)
    const int* __restrict__ ctx_lens,           // (B,)
    const float* __restrict__ alibi,            // (Hq,) slopes or null
    unsigned short* __restrict__ out,
    float* __restrict__ part_ml,                // (B*Hkv*nch*n_split, MAXG, 2)
    float* __restrict__ part_acc,               // (..., MAXG, D)
    int B, int Hkv, int G, int nch, int maxp, int n_split, int window,
    float scale, long q_sb, long q_sh, long out_sb, long out_sh) {
  static_assert(D % 64 == 0, "a K row is read in 64-element groups");
  constexpr int P = F8P;
  constexpr int NKJ = D / 64;       // 16 B K loads per position
  constexpr int NDT = D / 16;       // PV d-tiles = V loads per tile
  constexpr int NPT = F8BLK / 16;   // position subtiles per KV tile
  constexpr int PROW_B = F8BLK * 2 + 16;  // P^T LDS row pitch
  constexpr int TSTRIDE = 4 * F8BLK;      // positions between a wave's tiles

  const int bh = blockIdx.x;
  const int split = blockIdx.y;
  const int b = bh / (Hkv * nch);
  const int rem = bh % (Hkv * nch);
  const int kvh = rem / nch;
  const int g0 = (rem % nch) * MAXG;   // this chunk's first group col
  const int Gl = min(G - g0, MAXG);    // live head cols in this chunk
  const int ctx = ctx_lens[b];

  const int pages_total = (ctx + P - 1) / P;
  const int pages_per_split = (pages_total + n_split - 1) / n_split;
  const int c0 = split * pages_per_split * P;
  const int c1 = min(ctx, c0 + pages_per_split * P);
  int lo = 0;
  if (window > 0) lo = max(0, ctx - window);

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int li = lane & 15;
  const int hi = lane >> 4;
  const float sc2 = scale * LOG2E;

  // per-wave P^T tile (head-major rows) + merge scratch
  __shared__ __attribute__((aligned(16))) unsigned char lds[
      4 * 16 * PROW_B + 3 * (MAXG * (D + 2) * 4)];
  unsigned char* p_lds = lds + wave * 16 * PROW_B;
  float* merge_lds = (float*)(lds + 4 * 16 * PROW_B);

  // Q fragments in the K loads' contraction order: slice 2j+c, index
  // hi*8 + e  <->  d = 64j + 16hi + 8c + e
  const int qh = g0 + ((li < Gl) ? li : Gl - 1);
  bf16x8 qfrag[2 * NKJ];
#pragma unroll
  for (int s = 0; s < 2 * NKJ; ++s)
    qfrag[s] = as_bf16x8(*reinterpret_cast<const short8*>(
        q + (long)b * q_sb + (long)(kvh * G + qh) * q_sh + 64 * (s >> 1) +
        16 * hi + 8 * (s & 1)));
  const int ag = g0 + li;
  const float aslope =
      (alibi != nullptr && ag < G) ? alibi[kvh * G + ag] * LOG2E : 0.f;

  float m2 = NEG_BIG, l = 0.f;
  f32x4 acc_o[NDT];  // O^T: rows = d (hi*4+reg + 16n), cols = head (li)
#pragma unroll
  for (int n = 0; n < NDT; ++n) acc_o[n] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const long head_slab = (long)kvh * P * D;  // bytes; same for both layouts
  const int tile0 = (max(c0, lo) - c0) / F8BLK;  // window skip, tile-aligned
  const int tbs = c0 + (tile0 + wave) * F8BLK;

  // raw fp8 words of one tile; distinct named buffers with compile-time
  // indices (dynamic buffer indexing would demote them to scratch)
  int4v vb0[NDT], vb1[NDT];
  int4v kb0[NPT][NKJ], kb1[NPT][NKJ];

  auto load_tile = [&](int4v (&vb)[NDT], int4v (&kb)[NPT][NKJ], int tb) {
    // V: page hi of the tile, row d = li + 16n; a page past c1 reads as 0
    const int vpos = tb + hi * P;
    int vpage = -1;
    if (vpos < c1) vpage = page_table[b * maxp + vpos / P];
    const unsigned char* vrow =
        v_pages + ((long)vpage * Hkv) * P * D + head_slab + (long)li * P;
#pragma unroll
    for (int n = 0; n < NDT; ++n) {
      vb[n] = (int4v){0, 0, 0, 0};
      if (vpage >= 0)
        vb[n] = __builtin_nontemporal_load(
            reinterpret_cast<const int4v*>(vrow + 16 * n * P));
    }
    // K: position row li of subtile n (clamped into the split: a dead row
    // is masked below), 16 d per load
#pragma unroll
    for (int n = 0; n < NPT; ++n) {
      const int cpos = min(tb + li + 16 * n, c1 - 1);
      const int page = page_table[b * maxp + cpos / P];
      const unsigned char* krow = k_pages + ((long)page * Hkv) * P * D +
                                  head_slab + (long)(cpos % P) * D + 16 * hi;
#pragma unroll
      for (int j = 0; j < NKJ; ++j)
        kb[n][j] = __builtin_nontemporal_load(
            reinterpret_cast<const int4v*>(krow + 64 * j));
    }
  };

  auto compute_tile = [&](const int4v (&vb)[NDT], const int4v (&kb)[NPT][NKJ],
                          int tb) {
    // ---- S^T = K Q^T: st[n][reg] = score at tb + 16n + hi*4 + reg ----
    f32x4 st[NPT];
#pragma unroll
    for (int n = 0; n < NPT; ++n) {
      st[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < NKJ; ++j) {
        bf16x8 klo, khi;
        fp8x16_to_bf16(kb[n][j], klo, khi);
        st[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(klo, qfrag[2 * j],
                                                        st[n], 0, 0, 0);
        st[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(khi, qfrag[2 * j + 1],
                                                        st[n], 0, 0, 0);
      }
    }
    // ---- mask + online softmax over positions (in-lane + 2 shuffles) ----
    float p[NPT][4];
    float rm = NEG_BIG;
#pragma unroll
    for (int n = 0; n < NPT; ++n)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int kpos = tb + 16 * n + hi * 4 + reg;
        float sv = st[n][reg] * sc2 + aslope * (float)kpos;
        const bool dead = (kpos >= c1) | (kpos < lo);
        sv = dead ? NEG_BIG : sv;
        p[n][reg] = sv;
        rm = fmaxf(rm, sv);
      }
    rm = f8_quad16_max(rm);
    const float mn = fmaxf(m2, rm);
    const float corr = fast_exp2(m2 - mn);
    float psum = 0.f;
#pragma unroll
    for (int n = 0; n < NPT; ++n)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        p[n][reg] = fast_exp2(p[n][reg] - mn);
        psum += p[n][reg];
      }
    psum = f8_quad16_sum(psum);
    l = l * corr + psum;
    m2 = mn;
    // the max rarely rises after the first tiles: skip the NDT-wide rescale
    // when no lane needs it (wave-uniform branch)
    if (__builtin_amdgcn_ballot_w64(corr < 0.9999f)) {
#pragma unroll
      for (int n = 0; n < NDT; ++n)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) acc_o[n][reg] *= corr;
    }
    // ---- P^T through LDS: head-major rows, natural position order; this
    // lane's 4 consecutive positions of subtile n are one 8 B store ----
#pragma unroll
    for (int n = 0; n < NPT; ++n) {
      short4v p4;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) p4[reg] = (short)f2bf(p[n][reg]);
      *reinterpret_cast<short4v*>(p_lds + li * PROW_B +
                                  (16 * n + hi * 4) * 2) = p4;
    }
    // B-fragment c: index hi*8 + e  <->  position 16hi + 8c + e (the V
    // loads' order). Wave-local LDS: ds ordering is by lgkmcnt waits.
    bf16x8 pfrag[2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
      pfrag[c] = as_bf16x8(*reinterpret_cast<const short8*>(
          p_lds + li * PROW_B + (16 * hi + 8 * c) * 2));
    // ---- acc^T += V^T P^T ----
#pragma unroll
    for (int n = 0; n < NDT; ++n) {
      bf16x8 vlo, vhi;
      fp8x16_to_bf16(vb[n], vlo, vhi);
      acc_o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vlo, pfrag[0],
                                                         acc_o[n], 0, 0, 0);
      acc_o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vhi, pfrag[1],
                                                         acc_o[n], 0, 0, 0);
    }
  };

  // sched_barrier pins each prefetch above the compute phase it overlaps
  if (tbs < c1) load_tile(vb0, kb0, tbs);
  for (int tb = tbs; tb < c1; tb += 2 * TSTRIDE) {
    if (tb + TSTRIDE < c1) load_tile(vb1, kb1, tb + TSTRIDE);
    __builtin_amdgcn_sched_barrier(0);
    compute_tile(vb0, kb0, tb);
    if (tb + TSTRIDE >= c1) break;
    if (tb + 2 * TSTRIDE < c1) load_tile(vb0, kb0, tb + 2 * TSTRIDE);
    __builtin_amdgcn_sched_barrier(0);
    compute_tile(vb1, kb1, tb + TSTRIDE);
  }

  // ---- merge the 4 waves (as attn_decode_mfma_kernel) ----
  // C col li = chunk-local head (valid for li < Gl); C row hi*4 + reg of
  // tile n = dimension 16n + hi*4 + reg. (m, l) are replicated across the 4
  // hi subgroups; hi == 0 publishes them.
  auto wave_slot = [&](int slot) { return merge_lds + slot * MAXG * (D + 2); };
  __syncthreads();
  if (wave > 0) {
    float* dst = wave_slot(wave - 1);
    if (li < Gl) {
#pragma unroll
      for (int n = 0; n < NDT; ++n)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          dst[li * (D + 2) + 16 * n + hi * 4 + reg] = acc_o[n][reg];
      if (hi == 0) {
        dst[li * (D + 2) + D] = m2;
        dst[li * (D + 2) + D + 1] = l;
      }
    }
  }
  __syncthreads();
  if (wave != 0) return;
  for (int slot = 0; slot < 3; ++slot) {
    const float* src = wave_slot(slot);
    if (li < Gl) {
      const float mo = src[li * (D + 2) + D];
      const float lo2 = src[li * (D + 2) + D + 1];
      const float mn = fmaxf(m2, mo);
      const float c1f = fast_exp2(m2 - mn);
      const float c2f = fast_exp2(mo - mn);
      l = l * c1f + lo2 * c2f;
#pragma unroll
      for (int n = 0; n < NDT; ++n)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          acc_o[n][reg] = acc_o[n][reg] * c1f +
                          src[li * (D + 2) + 16 * n + hi * 4 + reg] * c2f;
      m2 = mn;
    }
  }

  if (li >= Gl) return;
  if (n_split == 1) {
    const float inv = (l > 0.f) ? 1.f / l : 0.f;
    unsigned short* orow =
        out + (long)b * out_sb + (long)(kvh * G + g0 + li) * out_sh;
#pragma unroll
    for (int n = 0; n < NDT; ++n) {
      short4v o4;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        o4[reg] = (short)f2bf(acc_o[n][reg] * inv);
      *reinterpret_cast<short4v*>(orow + 16 * n + hi * 4) = o4;
    }
  } else {
    const long pbase = ((long)bh * n_split + split);
    float* prow = part_acc + (pbase * MAXG + li) * D;
#pragma unroll
    for (int n = 0; n < NDT; ++n)
      *reinterpret_cast<f32x4*>(prow + 16 * n + hi * 4) = acc_o[n];
    if (hi == 0) {
      part_ml[(pbase * MAXG + li) * 2 + 0] = m2;
      part_ml[(pbase * MAXG + li) * 2 + 1] = l;
    }
  }
}
