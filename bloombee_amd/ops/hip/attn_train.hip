// Training attention for gfx950: flash forward with LSE, and a two-kernel
// flash backward that recomputes P from the LSE. Dense K/V (no paged pool);
// this is the fine-tuning counterpart of attn_prefill.hip.
//
// Addressing: q/k/v/dout element (b, t, h, d) at b*sb + t*st + h*sh + d, so
//   they may be views into a fused (B, T, Hq+2Hkv, D) projection output or
//   (B, H, T, D) tensors seen through a permute. out/dq are (B, T, Hq, D)
//   contiguous, dk/dv (B, T, Hkv, D) contiguous, lse/delta (B, Hq, T) f32.
//   All offsets are long; (batch, head, tile) ride a flat 1-D grid.
//
// Mask: causal, plus an optional sliding window (key > query - window).
//   ALiBi adds slope[h] * key_index; softmax is shift invariant per row, so
//   the absolute start position never reaches these kernels.
//
// attn_train_fwd_kernel: attn_prefill.hip's structure. 128 query rows per
//   workgroup (8 waves x 16 rows), 32-key tiles through LDS, exp2-domain
//   online softmax, and lse = ln(sum exp(score)) stored per row.
//
// attn_train_dq_kernel: query-owned, same tiling as the forward. Its
//   prologue forms delta = rowsum(dO * O) from the bf16 O the forward
//   returned and stores it for the dK/dV kernel. Per key tile:
//   S = Q K^T, dP = dO V^T, P = exp2(c S + bias - lse log2e),
//   dS = P (dP - delta), dQ += dS K; scale is applied once at the store.
//
// attn_train_dkdv_kernel: key-owned. A workgroup owns 128 keys of one
//   (batch, kv head), each wave 16 of them with dK and dV in accumulators,
//   and sweeps the G query heads x 32-row query slices that can see its
//   keys (query >= block start; the window adds an upper bound). It works on
//   the transposed tiles S^T = K Q^T and dP^T = V dO^T, so dV += P^T dO and
//   dK += dS^T Q need no cross-workgroup sum: dK and dV are written once,
//   with no atomics and no workgroup waiting on another. The dQ kernel pays
//   two extra MFMA products per tile (S and dP again) for the same property.
//
// Numerics: bf16 operands, fp32 softmax and accumulation. Rounding points:
//   forward  - unnormalised P to bf16 as the P.V operand; O to bf16 at store.
//   backward - S, dP, lse and delta stay f32; the normalised P is rounded to
//              bf16 once (dV operand) and dS once (dK and dQ operand);
//              dQ, dK, dV are rounded to bf16 at the store.
//              delta is formed from the bf16-rounded O.

#include "common.h"


static constexpr int TR_KV = 32;    // keys (fwd, dQ) or queries (dK/dV) per LDS tile
static constexpr int TR_ROWS = 128; // rows a workgroup owns


// Stage a 32-row tile of a (b, t, h, :) tensor into LDS: row-major padded
// image at `rm` (or skipped when null) and transposed [d][row] image at `tr`
// (or skipped when null). Rows at or past T are zero.
template <int D>
DEVINL void tr_stage_tile(const unsigned short* __restrict__ src, long base,
                          long st, int row0, int T, unsigned char* rm,
                          unsigned char* tr, int tid) {
  constexpr int ROW_B = D * 2 + 16;
  constexpr int TROW_B = TR_KV * 2 + 16;
  for (int idx = tid; idx < TR_KV * (D / 8); idx += 512) {
    // row-major only: d fastest across lanes (coalesced global rows). With a
    // transposed image: row fastest, so the 2-byte stores of a wave fall on
    // 32 consecutive rows of one d (conflict-free) instead of 16 d's that
    // share two banks.
    const int t = (tr != nullptr) ? idx % TR_KV : idx / (D / 8);
    const int d8 = ((tr != nullptr) ? idx / TR_KV : idx % (D / 8)) * 8;
    const int row = row0 + t;
    short8 x{};
    if (row < T)
      x = *reinterpret_cast<const short8*>(src + base + (long)row * st + d8);
    if (rm != nullptr)
      *reinterpret_cast<short8*>(rm + t * ROW_B + d8 * 2) = x;
    if (tr != nullptr) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        *(unsigned short*)(tr + (d8 + j) * TROW_B + t * 2) = (unsigned short)x[j];
    }
  }
}


template <int D>
__global__ __launch_bounds__(512) void attn_train_fwd_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v, const float* __restrict__ alibi,
    unsigned short* __restrict__ out,  // (B, T, Hq, D) contiguous
    float* __restrict__ lse,           // (B, Hq, T) or null
    int Hq, int G, int T, int ntile, int window, float scale,
    long q_sb, long q_st, long q_sh, long k_sb, long k_st, long k_sh,
    long v_sb, long v_st, long v_sh) {
  constexpr int KROW_B = D * 2 + 16;
  constexpr int VROW_B = TR_KV * 2 + 16;
  constexpr int PROW_B = TR_KV * 2 + 16;
  constexpr int NKK = D / 32;
  constexpr int NDT = D / 16;

  __shared__ __attribute__((aligned(16))) unsigned char lds[
      TR_KV * KROW_B + D * VROW_B + 8 * 16 * PROW_B];
  unsigned char* k_lds = lds;
  unsigned char* v_lds = lds + TR_KV * KROW_B;
  unsigned char* p_lds = lds + TR_KV * KROW_B + D * VROW_B;

  const int qtile = blockIdx.x % ntile;
  const int bh = blockIdx.x / ntile;
  const int b = bh / Hq, h = bh % Hq;
  const int kvh = h / G;
  const int qbase = qtile * TR_ROWS;
  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int li = lane & 15;
  const int hi = lane >> 4;
  const float sc2 = scale * LOG2E;
  const float aslope = (alibi != nullptr) ? alibi[h] * LOG2E : 0.f;
  const long kbase_off = (long)b * k_sb + (long)kvh * k_sh;
  const long vbase_off = (long)b * v_sb + (long)kvh * v_sh;

  const int my_qrow = min(qbase + wave * 16 + li, T - 1);
  bf16x8 qfrag[NKK];
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk)
    qfrag[kk] = as_bf16x8(*reinterpret_cast<const short8*>(
        q + (long)b * q_sb + (long)my_qrow * q_st + (long)h * q_sh + hi * 8 + 32 * kk));

  float m2[4], l[4];
  f32x4 acc_o[NDT];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m2[r] = NEG_BIG; l[r] = 0.f; }
#pragma unroll
  for (int n = 0; n < NDT; ++n) acc_o[n] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int kmax = min(T, qbase + TR_ROWS);
  int kstart = 0;
  if (window > 0) kstart = max(0, (qbase - window + 1) / TR_KV * TR_KV);
  const int wrow_max = qbase + wave * 16 + 15;

  for (int kb = kstart; kb < kmax; kb += TR_KV) {
    __syncthreads();
    tr_stage_tile<D>(k, kbase_off, k_st, kb, T, k_lds, nullptr, tid);
    tr_stage_tile<D>(v, vbase_off, v_st, kb, T, nullptr, v_lds, tid);
    __syncthreads();
    if (kb > wrow_max) continue;  // every key of the tile is in this wave's future

    f32x4 s[TR_KV / 16];
#pragma unroll
    for (int n = 0; n < TR_KV / 16; ++n) {
      s[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) {
        bf16x8 bfrag = as_bf16x8(*reinterpret_cast<const short8*>(
            k_lds + (li + 16 * n) * KROW_B + hi * 16 + 64 * kk));
        s[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qfrag[kk], bfrag, s[n], 0, 0, 0);
      }
    }

    float p[TR_KV / 16][4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int qrow = qbase + wave * 16 + hi * 4 + reg;
      float rm = NEG_BIG;
#pragma unroll
      for (int n = 0; n < TR_KV / 16; ++n) {
        const int kpos = kb + li + 16 * n;
        float sv = s[n][reg] * sc2 + aslope * (float)kpos;
        const bool dead = (qrow >= T) | (kpos >= T) | (kpos > qrow) |
                          (window > 0 && kpos <= qrow - window);
        sv = dead ? NEG_BIG : sv;
        p[n][reg] = sv;
        rm = fmaxf(rm, sv);
      }
      rm = group16_reduce_max(rm);
      const float mn = fmaxf(m2[reg], rm);
      const float corr = fast_exp2(m2[reg] - mn);
      float psum = 0.f;
#pragma unroll
      for (int n = 0; n < TR_KV / 16; ++n) {
        p[n][reg] = fast_exp2(p[n][reg] - mn);
        psum += p[n][reg];
      }
      psum = group16_reduce_sum(psum);
      l[reg] = l[reg] * corr + psum;
      m2[reg] = mn;
#pragma unroll
      for (int n = 0; n < NDT; ++n) acc_o[n][reg] *= corr;
    }

    unsigned char* pw = p_lds + wave * 16 * PROW_B;
#pragma unroll
    for (int n = 0; n < TR_KV / 16; ++n)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        *(unsigned short*)(pw + (hi * 4 + reg) * PROW_B + (li + 16 * n) * 2) =
            f2bf(p[n][reg]);
    __builtin_amdgcn_wave_barrier();  // wave-local LDS, in-order per wave
    bf16x8 pfrag = as_bf16x8(
        *reinterpret_cast<const short8*>(pw + li * PROW_B + hi * 16));

#pragma unroll
    for (int n = 0; n < NDT; ++n) {
      bf16x8 vfrag = as_bf16x8(*reinterpret_cast<const short8*>(
          v_lds + (li + 16 * n) * VROW_B + hi * 16));
      acc_o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pfrag, vfrag, acc_o[n], 0, 0, 0);
    }
  }

#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int qrow = qbase + wave * 16 + hi * 4 + reg;
    if (qrow >= T) continue;
    const float inv = (l[reg] > 0.f) ? 1.f / l[reg] : 0.f;
#pragma unroll
    for (int n = 0; n < NDT; ++n)
      out[(((long)b * T + qrow) * Hq + h) * D + li + 16 * n] =
          f2bf(acc_o[n][reg] * inv);
    if (lse != nullptr && li == 0)
      lse[((long)b * Hq + h) * T + qrow] = (m2[reg] + log2f(l[reg])) * (1.f / LOG2E);
  }
}


template <int D>
__global__ __launch_bounds__(512) void attn_train_dq_kernel(
    const unsigned short* __restrict__ dout, const unsigned short* __restrict__ q,
    const unsigned short* __restrict__ k, const unsigned short* __restrict__ v,
    const unsigned short* __restrict__ out,  // (B, T, Hq, D) contiguous
    const float* __restrict__ lse, const float* __restrict__ alibi,
    unsigned short* __restrict__ dq,   // (B, T, Hq, D) contiguous
    float* __restrict__ delta,         // (B, Hq, T), written here
    int Hq, int G, int T, int ntile, int window, float scale,
    long do_sb, long do_st, long do_sh, long q_sb, long q_st, long q_sh,
    long k_sb, long k_st, long k_sh, long v_sb, long v_st, long v_sh) {
  constexpr int ROW_B = D * 2 + 16;
  constexpr int TROW_B = TR_KV * 2 + 16;
  constexpr int NKK = D / 32;
  constexpr int NDT = D / 16;

  __shared__ __attribute__((aligned(16))) unsigned char lds[
      2 * TR_KV * ROW_B + D * TROW_B + 8 * 16 * TROW_B];
  unsigned char* k_lds = lds;
  unsigned char* v_lds = lds + TR_KV * ROW_B;
  unsigned char* kt_lds = lds + 2 * TR_KV * ROW_B;
  unsigned char* ds_lds = kt_lds + D * TROW_B;

  const int qtile = blockIdx.x % ntile;
  const int bh = blockIdx.x / ntile;
  const int b = bh / Hq, h = bh % Hq;
  const int kvh = h / G;
  const int qbase = qtile * TR_ROWS;
  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int li = lane & 15;
  const int hi = lane >> 4;
  const float sc2 = scale * LOG2E;
  const float aslope = (alibi != nullptr) ? alibi[h] * LOG2E : 0.f;
  const long kbase_off = (long)b * k_sb + (long)kvh * k_sh;
  const long vbase_off = (long)b * v_sb + (long)kvh * v_sh;
  const long row_off = ((long)b * Hq + h) * T;

  // ---- Q and dO fragments; delta from dO and the bf16 O ----
  const int my_qrow = min(qbase + wave * 16 + li, T - 1);
  bf16x8 qfrag[NKK], dofrag[NKK];
  float dsum = 0.f;
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk) {
    const int d0 = hi * 8 + 32 * kk;
    qfrag[kk] = as_bf16x8(*reinterpret_cast<const short8*>(
        q + (long)b * q_sb + (long)my_qrow * q_st + (long)h * q_sh + d0));
    const short8 dov = *reinterpret_cast<const short8*>(
        dout + (long)b * do_sb + (long)my_qrow * do_st + (long)h * do_sh + d0);
    const short8 ov = *reinterpret_cast<const short8*>(
        out + (((long)b * T + my_qrow) * Hq + h) * D + d0);
    dofrag[kk] = as_bf16x8(dov);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      dsum += bf2f((unsigned short)dov[j]) * bf2f((unsigned short)ov[j]);
  }
  dsum += __shfl_xor(dsum, 16);
  dsum += __shfl_xor(dsum, 32);  // every lane: delta of row li
  if (hi == 0 && qbase + wave * 16 + li < T) delta[row_off + my_qrow] = dsum;

  float dl[4], lse2[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    dl[reg] = __shfl(dsum, hi * 4 + reg);
    const int qrow = qbase + wave * 16 + hi * 4 + reg;
    lse2[reg] = (qrow < T) ? lse[row_off + qrow] * LOG2E : 0.f;
  }

  f32x4 acc[NDT];
#pragma unroll
  for (int n = 0; n < NDT; ++n) acc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int kmax = min(T, qbase + TR_ROWS);
  int kstart = 0;
  if (window > 0) kstart = max(0, (qbase - window + 1) / TR_KV * TR_KV);
  const int wrow_max = qbase + wave * 16 + 15;

  for (int kb = kstart; kb < kmax; kb += TR_KV) {
    __syncthreads();
    tr_stage_tile<D>(k, kbase_off, k_st, kb, T, k_lds, kt_lds, tid);
    tr_stage_tile<D>(v, vbase_off, v_st, kb, T, v_lds, nullptr, tid);
    __syncthreads();
    if (kb > wrow_max) continue;

    f32x4 s[TR_KV / 16], dp[TR_KV / 16];
#pragma unroll
    for (int n = 0; n < TR_KV / 16; ++n) {
      s[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
      dp[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) {
        bf16x8 kf = as_bf16x8(*reinterpret_cast<const short8*>(
            k_lds + (li + 16 * n) * ROW_B + hi * 16 + 64 * kk));
        bf16x8 vf = as_bf16x8(*reinterpret_cast<const short8*>(
            v_lds + (li + 16 * n) * ROW_B + hi * 16 + 64 * kk));
        s[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qfrag[kk], kf, s[n], 0, 0, 0);
        dp[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dofrag[kk], vf, dp[n], 0, 0, 0);
      }
    }

    // ---- dS (C layout: row = hi*4+reg, col = li+16n) -> LDS -> A fragment ----
    unsigned char* dw = ds_lds + wave * 16 * TROW_B;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int qrow = qbase + wave * 16 + hi * 4 + reg;
#pragma unroll
      for (int n = 0; n < TR_KV / 16; ++n) {
        const int kpos = kb + li + 16 * n;
        const bool dead = (qrow >= T) | (kpos >= T) | (kpos > qrow) |
                          (window > 0 && kpos <= qrow - window);
        const float pv = fast_exp2(s[n][reg] * sc2 + aslope * (float)kpos - lse2[reg]);
        const float dsv = dead ? 0.f : pv * (dp[n][reg] - dl[reg]);
        *(unsigned short*)(dw + (hi * 4 + reg) * TROW_B + (li + 16 * n) * 2) = f2bf(dsv);
      }
    }
    __builtin_amdgcn_wave_barrier();
    bf16x8 dsfrag = as_bf16x8(
        *reinterpret_cast<const short8*>(dw + li * TROW_B + hi * 16));

#pragma unroll
    for (int n = 0; n < NDT; ++n) {
      bf16x8 ktf = as_bf16x8(*reinterpret_cast<const short8*>(
          kt_lds + (li + 16 * n) * TROW_B + hi * 16));
      acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsfrag, ktf, acc[n], 0, 0, 0);
    }
  }

#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int qrow = qbase + wave * 16 + hi * 4 + reg;
    if (qrow >= T) continue;
#pragma unroll
    for (int n = 0; n < NDT; ++n)
      dq[(((long)b * T + qrow) * Hq + h) * D + li + 16 * n] =
          f2bf(acc[n][reg] * scale);
  }
}


template <int D>
__global__ __launch_bounds__(512) void attn_train_dkdv_kernel(
    const unsigned short* __restrict__ dout, const unsigned short* __restrict__ q,
    const unsigned short* __restrict__ k, const unsigned short* __restrict__ v,
    const float* __restrict__ lse, const float* __restrict__ delta,
    const float* __restrict__ alibi,
    unsigned short* __restrict__ dk,  // (B, T, Hkv, D) contiguous
    unsigned short* __restrict__ dv,
    int Hq, int G, int T, int nkb, int window, float scale,
    long do_sb, long do_st, long do_sh, long q_sb, long q_st, long q_sh,
    long k_sb, long k_st, long k_sh, long v_sb, long v_st, long v_sh) {
  constexpr int ROW_B = D * 2 + 16;
  constexpr int TROW_B = TR_KV * 2 + 16;
  constexpr int NKK = D / 32;
  constexpr int NDT = D / 16;

  __shared__ __attribute__((aligned(16))) unsigned char lds[
      2 * TR_KV * ROW_B + 2 * D * TROW_B + 2 * 8 * 16 * TROW_B];
  unsigned char* q_lds = lds;
  unsigned char* do_lds = lds + TR_KV * ROW_B;
  unsigned char* qt_lds = lds + 2 * TR_KV * ROW_B;
  unsigned char* dot_lds = qt_lds + D * TROW_B;
  unsigned char* p_lds = dot_lds + D * TROW_B;
  unsigned char* ds_lds = p_lds + 8 * 16 * TROW_B;

  const int Hkv = Hq / G;
  const int kblk = blockIdx.x % nkb;
  const int bk = blockIdx.x / nkb;
  const int b = bk / Hkv, kvh = bk % Hkv;
  const int kb0 = kblk * TR_ROWS;
  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int li = lane & 15;
  const int hi = lane >> 4;
  const float sc2 = scale * LOG2E;
  const int wk0 = kb0 + wave * 16;  // this wave's first key

  // ---- K and V fragments of this wave's 16 keys (A operands) ----
  const int my_key = min(wk0 + li, T - 1);
  bf16x8 kfrag[NKK], vfrag[NKK];
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk) {
    const int d0 = hi * 8 + 32 * kk;
    kfrag[kk] = as_bf16x8(*reinterpret_cast<const short8*>(
        k + (long)b * k_sb + (long)my_key * k_st + (long)kvh * k_sh + d0));
    vfrag[kk] = as_bf16x8(*reinterpret_cast<const short8*>(
        v + (long)b * v_sb + (long)my_key * v_st + (long)kvh * v_sh + d0));
  }

  f32x4 acc_k[NDT], acc_v[NDT];
#pragma unroll
  for (int n = 0; n < NDT; ++n) {
    acc_k[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    acc_v[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  // queries that can see a key of this block: [kb0, qhi)
  int qhi = T;
  if (window > 0) qhi = min(T, kb0 + TR_ROWS - 1 + window);

  for (int g = 0; g < G; ++g) {
    const int h = kvh * G + g;
    const float aslope = (alibi != nullptr) ? alibi[h] * LOG2E : 0.f;
    const long row_off = ((long)b * Hq + h) * T;
    const long qoff = (long)b * q_sb + (long)h * q_sh;
    const long dooff = (long)b * do_sb + (long)h * do_sh;

    for (int qb = kb0; qb < qhi; qb += TR_KV) {
      __syncthreads();
      tr_stage_tile<D>(q, qoff, q_st, qb, T, q_lds, qt_lds, tid);
      tr_stage_tile<D>(dout, dooff, do_st, qb, T, do_lds, dot_lds, tid);
      __syncthreads();
      // wave-uniform skips: keys past T, every query before every key of the
      // wave, or every key at or below the window's lower edge
      if (wk0 >= T || qb + TR_KV - 1 < wk0) continue;
      if (window > 0 && wk0 + 15 <= qb - window) continue;

      // ---- S^T = K Q^T, dP^T = V dO^T (row = key, col = query) ----
      f32x4 s[TR_KV / 16], dp[TR_KV / 16];
#pragma unroll
      for (int n = 0; n < TR_KV / 16; ++n) {
        s[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
        dp[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
          bf16x8 qf = as_bf16x8(*reinterpret_cast<const short8*>(
              q_lds + (li + 16 * n) * ROW_B + hi * 16 + 64 * kk));
          bf16x8 dof = as_bf16x8(*reinterpret_cast<const short8*>(
              do_lds + (li + 16 * n) * ROW_B + hi * 16 + 64 * kk));
          s[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag[kk], qf, s[n], 0, 0, 0);
          dp[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vfrag[kk], dof, dp[n], 0, 0, 0);
        }
      }

      unsigned char* pw = p_lds + wave * 16 * TROW_B;
      unsigned char* dw = ds_lds + wave * 16 * TROW_B;
#pragma unroll
      for (int n = 0; n < TR_KV / 16; ++n) {
        const int qrow = qb + li + 16 * n;
        const bool qlive = qrow < T;
        const float l2 = qlive ? lse[row_off + qrow] * LOG2E : 0.f;
        const float dlt = qlive ? delta[row_off + qrow] : 0.f;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int kpos = wk0 + hi * 4 + reg;
          const bool dead = (!qlive) | (kpos >= T) | (kpos > qrow) |
                            (window > 0 && kpos <= qrow - window);
          float pv = fast_exp2(s[n][reg] * sc2 + aslope * (float)kpos - l2);
          pv = dead ? 0.f : pv;
          const float dsv = dead ? 0.f : pv * (dp[n][reg] - dlt);
          *(unsigned short*)(pw + (hi * 4 + reg) * TROW_B + (li + 16 * n) * 2) = f2bf(pv);
          *(unsigned short*)(dw + (hi * 4 + reg) * TROW_B + (li + 16 * n) * 2) = f2bf(dsv);
        }
      }
      __builtin_amdgcn_wave_barrier();
      bf16x8 pfrag = as_bf16x8(
          *reinterpret_cast<const short8*>(pw + li * TROW_B + hi * 16));
      bf16x8 dsfrag = as_bf16x8(
          *reinterpret_cast<const short8*>(dw + li * TROW_B + hi * 16));

      // ---- dV += P^T dO, dK += dS^T Q (sum over the 32 queries) ----
#pragma unroll
      for (int n = 0; n < NDT; ++n) {
        bf16x8 dotf = as_bf16x8(*reinterpret_cast<const short8*>(
            dot_lds + (li + 16 * n) * TROW_B + hi * 16));
        bf16x8 qtf = as_bf16x8(*reinterpret_cast<const short8*>(
            qt_lds + (li + 16 * n) * TROW_B + hi * 16));
        acc_v[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pfrag, dotf, acc_v[n], 0, 0, 0);
        acc_k[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsfrag, qtf, acc_k[n], 0, 0, 0);
      }
    }
  }

#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int kpos = wk0 + hi * 4 + reg;
    if (kpos >= T) continue;
    const long o = (((long)b * T + kpos) * Hkv + kvh) * D + li;
#pragma unroll
    for (int n = 0; n < NDT; ++n) {
      dk[o + 16 * n] = f2bf(acc_k[n][reg] * scale);
      dv[o + 16 * n] = f2bf(acc_v[n][reg]);
    }
  }
}
