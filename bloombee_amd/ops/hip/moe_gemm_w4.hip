// Grouped MoE expert GEMM over 4-bit weights for gfx950: ONE launch over all
// experts, streaming quant4 codes instead of bf16.
//
//   C[s, :] = (A[row(s), :] @ dequant4(Wq[expert(s)])^T) * scale_slot[s]
//
// Weights are in quant4_pack layout with a leading expert dimension:
// packed (E, N, K/2) u8 (two codes per byte along K, low nibble first),
// scale / zero (E, N, K/64) f16, w = q * scale + zero. 4.5 bits per weight
// against 16: Mixtral decode is a pure expert-weight stream, so the bytes
// are the time.
//
// The two halves of the design come from kernels already in the tree:
//  * slots, grid and graph safety from moe_gemm_v2_kernel (moe_gemm.hip):
//    off (E+1) prefix sums on device, optional rowmap and per-slot scale,
//    host-side S / mchunks, grid (N/64 XCD-remapped, E*mchunks), 32-row
//    m-chunks, empty (expert, chunk) pairs exit before any weight byte is
//    touched, ragged groups clamp to their last row. No host sync, no
//    atomics.
//  * the weight path from gemm_skinny_w4_kernel (w4_gemm.hip): 16 B code
//    words per lane, the packed-f16 dequant with the magic subtracted
//    first, f16 MFMA 16x16x32 with f32 accumulation, the next stage's codes
//    and scale / zero in flight while this one is consumed.
//
// The A operand is staged through LDS in full lines once per 256-k stage
// (rowmap resolved once per block), converted bf16 -> f16 on the way in;
// the four waves of a block share it. The dense W4 kernel's per-lane 4 B
// global A loads are what made it plateau at M 2..32.
//
// Because this kernel writes the A tile itself it can choose which k each
// fragment slot holds, and uses that twice: a lane feeds its MFMAs from the
// dwords of its OWN code word (no shfl to hand codes to fragment lanes), and
// within a dword the codes are dequantized as the pairs (j, j + 4)
// (dq8_q4_f16_il). The A tile is stored in the matching order.
//
// Every global load is branch-free and the rowmap is resolved ahead of the
// k-loop: a per-lane branch or a dependent lookup around a load costs a
// full vmcnt wait, which drains the weight prefetch (measured: 259 -> 216 us
// on the gate_up shape, profiles/r05_moe_w4.md).
//
// Split-K (gridDim.z): splits are multiples of 128 k so no 64-group
// straddles; partial sums go to f32 slabs (ksplit, S, N) and
// moe_gemm_w4_combine_kernel sums them, applies the slot scale and rounds
// once. Activations outside the f16 range are not supported (as linear_w4).

#include "common.h"
#include <hip/hip_fp16.h>

// half8 / half2v / uint4v and dq8_q4_f16 come from w4_gemm.hip, included
// before this file.

// dq8_q4_f16 (w4_gemm.hip) with the eight codes of a dword taken as the
// pairs (j, j + 4): one shift and one and-or build a half2 of two codes,
// about half the bit work of going byte by byte. Same arithmetic per
// element: the magic is subtracted first. The result holds k in the order
// 0 4 1 5 2 6 3 7; the A tile is stored in that order too.
DEVINL half8 dq8_q4_f16_il(unsigned int c, half2v sc2, half2v zp2) {
  const half2v magic = {(_Float16)1024.f, (_Float16)1024.f};
  half8 out;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned h2 = ((c >> (4 * j)) & 0x000F000Fu) | 0x64006400u;
    half2v v = __builtin_bit_cast(half2v, h2);
    v = (v - magic) * sc2 + zp2;
    out[2 * j] = v[0];
    out[2 * j + 1] = v[1];
  }
  return out;
}

template <int MT>  // 16-row m-tiles per block (2 => 32-row chunks)
__global__ __launch_bounds__(256) void moe_gemm_w4_kernel(
    const unsigned short* __restrict__ A,    // (Ta, K) bf16
    const unsigned char* __restrict__ Wq,    // (E, N, K/2) packed nibbles
    const __half* __restrict__ wscale,       // (E, N, K/64) f16
    const __half* __restrict__ wzero,        // (E, N, K/64) f16
    const int* __restrict__ off,             // (E+1,) exclusive prefix sum
    const int* __restrict__ rowmap,          // (S,) slot -> A row, or null
    const float* __restrict__ scale,         // (S,) per-slot scale, or null
    unsigned short* __restrict__ C,          // (S, N) bf16     (ksplit == 1)
    float* __restrict__ Cpart,               // (ksplit, S, N)  (ksplit > 1)
    int S, int N, int K, int mchunks, int kchunk) {
  constexpr int KSTEP = 256;
  constexpr int RSTRIDE = KSTEP + 8;
  __shared__ __attribute__((aligned(16))) _Float16 atile[MT * 16 * RSTRIDE];

  const int e = blockIdx.y / mchunks;
  const int m0 = (blockIdx.y % mchunks) * (MT * 16);
  const int base = off[e];
  const int cnt = off[e + 1] - base;
  if (m0 >= cnt) return;  // empty chunk: no weight traffic

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int li = lane & 15;
  const int hi = lane >> 4;

  // XCD-aware tile remap (see gemm_skinny_v2)
  int tile = blockIdx.x;
  {
    const int nwg = gridDim.x;
    const int xcd = tile % 8, orig8 = tile / 8;
    const int q = nwg / 8, r = nwg % 8;
    if (nwg >= 8)
      tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + orig8;
  }
  const int n0 = tile * 64 + wave * 16;

  const int split = blockIdx.z;
  const int k0 = split * kchunk;
  const int k1 = min(K, k0 + kchunk);

  // the expert stride applies to all three weight tensors
  const long wr = (long)e * N + n0 + li;
  const unsigned char* wrow = Wq + wr * (K / 2);
  const __half* srow = wscale + wr * (K / 64);
  const __half* zrow = wzero + wr * (K / 64);

  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // A staging: thread piece j covers staged row (tid + j*256)/32, 8 k each;
  // that row's A row is the group's slot m0 + r (clamped), via rowmap.
  // The last stage of a split may hold only 128 k: its upper half is not
  // read.
  constexpr int NPIECE = MT * 2;
  short8 aregs[NPIECE];
  // The staged row of a piece does not depend on the stage: resolve the
  // rowmap once per block (a lookup inside load_a would be a dependent load
  // whose wait drains every load in flight, the weight prefetch included).
  int arow[NPIECE];
#pragma unroll
  for (int j = 0; j < NPIECE; ++j) {
    const int s = base + min(m0 + (int)(threadIdx.x + j * 256) / 32, cnt - 1);
    arow[j] = (rowmap != nullptr) ? rowmap[s] : s;
  }
  auto load_a = [&](int ks) {
#pragma unroll
    for (int j = 0; j < NPIECE; ++j) {
      const int flat = threadIdx.x + j * 256;
      // branch-free: past the end of a half stage re-read its last chunk
      // (a per-lane branch here would put a full vmcnt wait behind every
      // piece and serialize the loads)
      const int k = min(ks + (flat % 32) * 8, k1 - 8);
      aregs[j] = *reinterpret_cast<const short8*>(A + (long)arow[j] * K + k);
    }
  };
  // Within a row of the tile the 16 B chunks of each 128-k half are stored
  // with their two index digits swapped (chunk hi*4 + s at slot s*4 + hi):
  // MFMA s then reads, across the four hi of a wave, four NEIGHBOURING
  // slots, the conflict pattern of the plain row-major fragment read.
  auto store_a = [&]() {
#pragma unroll
    for (int j = 0; j < NPIECE; ++j) {
      const int flat = threadIdx.x + j * 256;
      const int c = flat % 32;
      const int slot = (c & 16) | ((c & 3) << 2) | ((c >> 2) & 3);
      // bf16 -> f16, two at a time (a bf16 significand fits in f16, so
      // rounding toward zero only shows below the f16 normal range), in
      // the k order 0 4 1 5 2 6 3 7 of dq8_q4_f16_il
      const uint4v d = __builtin_bit_cast(uint4v, aregs[j]);
      uint4v h;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned int x = d[i >> 1], y = d[(i >> 1) + 2];
        const float fx = __builtin_bit_cast(float, (i & 1) ? (x & 0xFFFF0000u) : (x << 16));
        const float fy = __builtin_bit_cast(float, (i & 1) ? (y & 0xFFFF0000u) : (y << 16));
        h[i] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_pkrtz(fx, fy));
      }
      *reinterpret_cast<uint4v*>(atile + (flat / 32) * RSTRIDE + slot * 8) = h;
    }
  };

  // One stage of weights per lane: 2 x 16 B of codes (the 32 codes at
  // k + hi*32 of each 128-k half) and the scale / zero of the one group
  // those 32 codes lie in. NSET register sets rotate: stage j computes from
  // set j % NSET while the loads of stage j + WAHEAD land in another, so
  // WAHEAD stages of codes stay in flight across the barriers.
  // (WAHEAD 2 and 3 measured within 3 % of 1 at the Mixtral shapes.)
  constexpr int WAHEAD = 1;
  constexpr int NSET = WAHEAD + 1;
  uint4v cw[NSET][2];
  unsigned short sv[NSET][2], zv[NSET][2];
  auto load_w = [&](int ks, int set) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      // branch-free as well: a half stage loads its lower half twice
      const int k = min(ks + h * 128, k1 - 128);
      cw[set][h] = *reinterpret_cast<const uint4v*>(wrow + (k + hi * 32) / 2);
      sv[set][h] = *reinterpret_cast<const unsigned short*>(srow + k / 64 + (hi >> 1));
      zv[set][h] = *reinterpret_cast<const unsigned short*>(zrow + k / 64 + (hi >> 1));
    }
  };
  auto mfma_stage = [&](int ks, int set) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (ks + h * 128 < k1) {
        const half2v sc2 = __builtin_bit_cast(
            half2v, (unsigned int)sv[set][h] | ((unsigned int)sv[set][h] << 16));
        const half2v zp2 = __builtin_bit_cast(
            half2v, (unsigned int)zv[set][h] | ((unsigned int)zv[set][h] << 16));
        // No lane exchange: an MFMA sums over its 32 k in any assignment of
        // k to fragment slots as long as A and B agree. MFMA s takes, in
        // lane (li, hi), dword s of the lane's own code word, i.e.
        // k = hi*32 + s*8 .. +8 of this 128-k half; the A fragment is read
        // from the same k of the LDS tile (slot s*4 + hi, see store_a).
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const half8 bfrag = dq8_q4_f16_il(cw[set][h][s], sc2, zp2);
#pragma unroll
          for (int t = 0; t < MT; ++t) {
            const half8 afrag = *reinterpret_cast<const half8*>(
                atile + (t * 16 + li) * RSTRIDE + h * 128 + s * 32 + hi * 8);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(afrag, bfrag,
                                                            acc[t], 0, 0, 0);
          }
        }
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
        mfma_stage(ks, j);
        if (more) {
          __syncthreads();
          store_a();
          __syncthreads();
        }
        ks += KSTEP;
      }
    }
  }

  // C row = slot base + m0 + t*16 + hi*4 + reg, col = n0 + li. The slot
  // scales are fetched together, ahead of the stores.
  float sc[MT][4];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int m = min(m0 + t * 16 + hi * 4 + reg, cnt - 1);
      sc[t][reg] = (scale != nullptr && Cpart == nullptr) ? scale[base + m] : 1.f;
    }
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int m = m0 + t * 16 + hi * 4 + reg;
      if (m >= cnt || base + m >= S) continue;
      const long o = (long)(base + m) * N + n0 + li;
      if (Cpart != nullptr)
        Cpart[(long)split * S * N + o] = acc[t][reg];
      else
        C[o] = f2bf(acc[t][reg] * sc[t][reg]);
    }
}

// Sum the split-K slabs, apply the slot scale, round once. Only the slots
// the prefix sums cover were written by the GEMM; the rest of C stays as
// allocated, as with ksplit == 1. Four columns per thread (N % 64 == 0).
__global__ __launch_bounds__(256) void moe_gemm_w4_combine_kernel(
    const float* __restrict__ Cpart,   // (ksplit, S, N)
    const int* __restrict__ off_end,   // &off[E]: slots in use
    const float* __restrict__ scale,   // (S,) or null
    unsigned short* __restrict__ C,    // (S, N) bf16
    int S, int N, int ksplit) {
  const int used = min(S, *off_end);
  const long total4 = (long)used * N / 4;
  const long slab = (long)S * N;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4;
       i += (long)gridDim.x * 256) {
    const long o = i * 4;
    f32x4 v = *reinterpret_cast<const f32x4*>(Cpart + o);
    for (int sp = 1; sp < ksplit; ++sp)
      v += *reinterpret_cast<const f32x4*>(Cpart + sp * slab + o);
    if (scale != nullptr) v *= scale[o / N];
    short4v out;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = (short)f2bf(v[j]);
    *reinterpret_cast<short4v*>(C + o) = out;
  }
}
