// Tiled 4-bit-weight GEMM for gfx950, M > 32:
//   C(M,N) bf16 = A(M,K) bf16 @ dequant4(Wq)^T (+bias) (+residual)
// Weights stay in quant4_pack layout (packed (N, K/2) u8, scale / zero
// (N, K/64) f16, w = q * scale + zero); K % 128 == 0, N % 64 == 0.
//
// Up to M of a few hundred a 4.5-bit weight is still cheaper to stream than to
// multiply (2 M / 0.5625 flop per byte), so the kernel is built around the
// code stream like gemm_skinny_w4_kernel, but pays for each code ONCE per
// block tile of up to 128 rows instead of once per 16-row m-tile:
//
//  * Block tile BM x 128, BM in {64, 128}, 256 threads. Wave w owns the 32
//    columns n0 + w*32 .. +32 as two 16-column B fragments and ALL BM rows:
//    MT = BM/16 m-tiles x 2 fragments of f32x4 accumulators (64 VGPRs at
//    BM = 128).
//  * Weight path: per 128-k stage a lane (li, hi) loads, for each of its two
//    fragments, the 16 B of codes of row n + li at k + hi*32 .. +32 and the
//    scale / zero of the one 64-group they lie in, straight to VGPRs. NSET
//    register sets rotate so the codes of the next WAHEAD stages are in
//    flight across the barriers while this stage is consumed (2 x 8 KB per
//    block). A dword is dequantized once (dq8_q4_f16_il, packed f16, magic
//    subtracted first) and the fragment feeds all MT m-tiles.
//  * A arrives as bf16, 16 B per thread and 256 B per row contiguous, is
//    converted to f16 on the way into LDS and staged once per stage for the
//    four waves. Rows are padded to 136 halves (272 B): the 16 lanes of one
//    ds_read_b128 quarter start 4 banks apart. As in moe_gemm_w4.hip the tile
//    is stored so that MFMA s of lane (li, hi) reads the k of dword s of the
//    lane's own code word (chunk hi*4 + s at slot s*4 + hi, elements in the
//    order 0 4 1 5 2 6 3 7): no lane exchange on the weight side.
//  * MFMA: v_mfma_f32_16x16x32_f16, f32 accumulation. LDS budget: an A
//    fragment is 1 KB per wave, a 16x16x32 MFMA occupies its SIMD for 16
//    clocks, LDS delivers 128 B/clk/CU. One B fragment per A fragment would
//    ask the four waves for 4 KB per 16 clk = 256 B/clk, twice what LDS has;
//    two B fragments per A fragment (this kernel) ask for 4 KB per 32 clk =
//    128 B/clk, the LDS rate, which is only reached when the kernel is
//    MFMA-bound (large M); below that the code stream is the limit.
//    LDS use: BM * 272 B = 17 KB (BM 64) / 34 KB (BM 128).
//  * N is only a multiple of 64: in the last column tile waves 2 and 3 may lie
//    past N. They stay in the block's barriers; their weight rows are clamped
//    to N - 1 (valid memory, same lines for all of them) and their stores are
//    predicated. Rows past M: loads clamp to row M - 1, stores are predicated.
//  * Grid (column tiles * m-tiles, k-splits). blockIdx.x is XCD-remapped and
//    THEN split into (column tile, m-tile) with the m-tile fastest: the blocks
//    that read one weight tile run on one XCD, next to each other in its
//    dispatch order, so all but the first find the codes in that XCD's L2.
//  * Split-K in whole 128-k stages; partial sums go to f32 slabs (ksplit, M,
//    N) and gemm_skinny_combine_kernel adds bias and residual. Unsplit, the
//    epilogue does. No atomics, no host sync.

#include "common.h"
#include <hip/hip_fp16.h>

// half8 / half2v / uint4v from w4_gemm.hip and dq8_q4_f16_il from
// moe_gemm_w4.hip, both included before this file.

template <int BM>  // rows per block tile: 64 or 128
__global__ __launch_bounds__(256) void gemm_w4_tiled_kernel(
    const unsigned short* __restrict__ A,     // (M, K) bf16
    const unsigned char* __restrict__ Wq,     // (N, K/2) packed nibbles
    const __half* __restrict__ wscale,        // (N, K/64) f16
    const __half* __restrict__ wzero,         // (N, K/64) f16
    const unsigned short* __restrict__ R,     // (M, N) bf16 residual or null
    const unsigned short* __restrict__ bias,  // (N,) bf16 or null
    unsigned short* __restrict__ C,           // (M, N) bf16     (unsplit)
    float* __restrict__ Cpart,                // (ksplit, M, N)  (split) or null
    int M, int N, int K, int mtiles, int kchunk) {
  constexpr int KSTEP = 128;
  constexpr int RSTRIDE = KSTEP + 8;
  constexpr int MT = BM / 16;
  __shared__ __attribute__((aligned(16))) _Float16 atile[BM * RSTRIDE];

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int li = lane & 15;
  const int hi = lane >> 4;

  const int t = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (t % mtiles) * BM;
  const int n0 = (t / mtiles) * 128 + wave * 32;
  const int split = blockIdx.y;
  const int k0 = split * kchunk;
  const int k1 = min(K, k0 + kchunk);

  const unsigned char* wrow[2];
  const __half* srow[2];
  const __half* zrow[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const long n = min(n0 + f * 16 + li, N - 1);
    wrow[f] = Wq + n * (K / 2) + hi * 16;
    srow[f] = wscale + n * (K / 64) + (hi >> 1);
    zrow[f] = wzero + n * (K / 64) + (hi >> 1);
  }

  f32x4 acc[MT][2];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int f = 0; f < 2; ++f) acc[i][f] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // A staging: piece j of a thread is the 16 B chunk (tid + j*256) % 16 of
  // staged row (tid + j*256) / 16; rows past M re-read row M - 1.
  constexpr int NPIECE = BM / 16;
  short8 aregs[NPIECE];
  const unsigned short* aptr[NPIECE];
#pragma unroll
  for (int j = 0; j < NPIECE; ++j) {
    const int flat = threadIdx.x + j * 256;
    aptr[j] = A + (long)min(m0 + flat / 16, M - 1) * K + (flat % 16) * 8;
  }
  auto load_a = [&](int ks) {
#pragma unroll
    for (int j = 0; j < NPIECE; ++j)
      aregs[j] = *reinterpret_cast<const short8*>(aptr[j] + ks);
  };
  auto store_a = [&]() {
#pragma unroll
    for (int j = 0; j < NPIECE; ++j) {
      const int flat = threadIdx.x + j * 256;
      const int c = flat % 16;
      const int slot = ((c & 3) << 2) | (c >> 2);
      // bf16 -> f16, two at a time (a bf16 significand fits in f16, so
      // rounding toward zero only shows below the f16 normal range), in the
      // k order 0 4 1 5 2 6 3 7 of dq8_q4_f16_il
      const uint4v d = __builtin_bit_cast(uint4v, aregs[j]);
      uint4v h;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned int x = d[i >> 1], y = d[(i >> 1) + 2];
        const float fx = __builtin_bit_cast(float, (i & 1) ? (x & 0xFFFF0000u) : (x << 16));
        const float fy = __builtin_bit_cast(float, (i & 1) ? (y & 0xFFFF0000u) : (y << 16));
        h[i] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_pkrtz(fx, fy));
      }
      *reinterpret_cast<uint4v*>(atile + (flat / 16) * RSTRIDE + slot * 8) = h;
    }
  };

  // Stage j computes from register set j % NSET while the loads of stages
  // j + 1 .. j + WAHEAD land in the others.
  constexpr int WAHEAD = 2;
  constexpr int NSET = WAHEAD + 1;
  uint4v cw[NSET][2];
  unsigned short sv[NSET][2], zv[NSET][2];
  auto load_w = [&](int ks, int set) {
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      cw[set][f] = *reinterpret_cast<const uint4v*>(wrow[f] + ks / 2);
      sv[set][f] = *reinterpret_cast<const unsigned short*>(srow[f] + ks / 64);
      zv[set][f] = *reinterpret_cast<const unsigned short*>(zrow[f] + ks / 64);
    }
  };
  auto mfma_stage = [&](int set) {
    half2v sc2[2], zp2[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      sc2[f] = __builtin_bit_cast(
          half2v, (unsigned int)sv[set][f] | ((unsigned int)sv[set][f] << 16));
      zp2[f] = __builtin_bit_cast(
          half2v, (unsigned int)zv[set][f] | ((unsigned int)zv[set][f] << 16));
    }
    // MFMA s takes, in lane (li, hi), dword s of the lane's own code words:
    // k = hi*32 + s*8 .. +8 of this stage; the A fragment is read from the
    // same k of the LDS tile (slot s*4 + hi, see store_a).
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const half8 b0 = dq8_q4_f16_il(cw[set][0][s], sc2[0], zp2[0]);
      const half8 b1 = dq8_q4_f16_il(cw[set][1][s], sc2[1], zp2[1]);
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const half8 afrag = *reinterpret_cast<const half8*>(
            atile + (i * 16 + li) * RSTRIDE + s * 32 + hi * 8);
        acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(afrag, b0, acc[i][0], 0, 0, 0);
        acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(afrag, b1, acc[i][1], 0, 0, 0);
      }
    }
  };

  load_a(k0);
#pragma unroll
  for (int j = 0; j < WAHEAD; ++j)
    if (k0 + j * KSTEP < k1) load_w(k0 + j * KSTEP, j);
  store_a();
  __syncthreads();
  for (int ks = k0; ks < k1;) {
#pragma unroll
    for (int j = 0; j < NSET; ++j) {  // set indices are constants per copy
      if (ks < k1) {
        const bool more = ks + KSTEP < k1;
        // A first: store_a waits for it, and in-order completion must not
        // make that wait cover the younger weight loads
        if (more) load_a(ks + KSTEP);
        if (ks + WAHEAD * KSTEP < k1)
          load_w(ks + WAHEAD * KSTEP, (j + WAHEAD) % NSET);
        mfma_stage(j);
        if (more) {
          __syncthreads();
          store_a();
          __syncthreads();
        }
        ks += KSTEP;
      }
    }
  }

  // C row = m0 + i*16 + hi*4 + reg, col = n0 + f*16 + li
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int n = n0 + f * 16 + li;
    if (n >= N) continue;
    const float bv = (bias != nullptr && Cpart == nullptr) ? bf2f(bias[n]) : 0.f;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int m = m0 + i * 16 + hi * 4 + reg;
        if (m >= M) continue;
        const long o = (long)m * N + n;
        if (Cpart != nullptr) {
          Cpart[(long)split * M * N + o] = acc[i][f][reg];
        } else {
          float v = acc[i][f][reg] + bv;
          if (R != nullptr) v += bf2f(R[o]);
          C[o] = f2bf(v);
        }
      }
  }
}
