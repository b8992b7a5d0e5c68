// fp8 (e4m3) weight tier, decode GEMM for gfx950 (W8A8):
//   C(M,N) = a_scale[m] * w_scale[n] * sum_k a8[m,k] * codes[n,k] [+bias] [+R]
// for M <= 32, K % 128 == 0, N % 64 == 0. Both operands are e4m3 and the
// matrix unit multiplies them as they are (v_mfma_scale_f32_16x16x128_f8f6f4
// with both block scales 1.0), so the weight stream is half the bf16
// kernel's bytes and costs no conversion VALU at all. Every scale is a power
// of two (ops/reference.py quant_w8 / quant_rows_fp8): applying them is exact
// and the bf16 store is the only rounding after the f32 accumulation.
//
// Split of the work: a workgroup (4 waves) owns one 64-column stripe of one
// K split; wave w owns the 16 columns of weight row group tile*4 + w and
// streams that group's 2 KB tiles (common.h, w8_packed_offset) global -> VGPR.
// A tile is two contiguous 1 KB wave loads and 8 VGPRs, half a bf16 tile of
// the same k extent; the saving buys depth: W8_DEPTH = 8 tiles (16 KB per
// wave, 64 KB per workgroup) are requested ahead of the one being multiplied.
//
// a8 goes through LDS once per workgroup per chunk of W8_DEPTH tiles (1 KB
// of every row): a wave copies whole rows, 1 KB per wave load, into rows of
// W8_AST = 1040 bytes. A fragment read is 16 B at
//   row*1040 + tile*128 + q*32 + h*16        (lane q*16 + row, half h),
// i.e. 16 B slot (row*65 + tile*8 + 2q + h) % 16 = (row + const) % 16 of the
// 256 B bank row: the 16 lanes a b128 read serves together differ in `row`
// alone and hit 16 different slots, so reads are conflict-free, and so are
// the copies (consecutive lanes, consecutive 16 B). The next chunk's rows are
// loaded to registers before the current chunk's MFMAs and stored behind two
// barriers after them; barriers do not wait for the W loads in flight.
//
// The k loop is branch-free: a chunk always runs W8_DEPTH tiles. Past the
// split's end the a8 bytes staged are zero and the W tile index is clamped to
// the split's last tile, so the surplus MFMAs add 0 * finite.
//
// Split-K writes f32 slabs (ksplit, M, N); gemm_w8_combine_kernel sums them
// in split order and applies scales, bias and residual. No atomics.

#include "common.h"

typedef __attribute__((ext_vector_type(8))) int int8v;

static constexpr int W8_DEPTH = 8;                  // tiles in flight per wave
static constexpr int W8_KC = W8_DEPTH * 128;        // k per staged A chunk
static constexpr int W8_AST = W8_KC + 16;           // LDS row stride, bytes
static constexpr int W8_ONE = 0x7f7f7f7f;           // e8m0 block scale 2^0

template <bool NT>
DEVINL int4v w8_load(const unsigned char* p) {
  if constexpr (NT)
    return __builtin_nontemporal_load(reinterpret_cast<const int4v*>(p));
  else
    return *reinterpret_cast<const int4v*>(p);
}

template <int MT, bool NT>  // MT: 16-row tiles of A (1: M <= 16, 2: M <= 32)
__global__ __launch_bounds__(256) void gemm_w8_kernel(
    const unsigned char* __restrict__ A8,     // (M, K) e4m3
    const unsigned char* __restrict__ Wp,     // tiled e4m3 codes of (N, K)
    const float* __restrict__ a_scale,        // (M,)
    const float* __restrict__ w_scale,        // (N,)
    const unsigned short* __restrict__ R,     // (M, N) bf16 or null
    const unsigned short* __restrict__ bias,  // (N,) bf16 or null
    unsigned short* __restrict__ C,           // (M, N) bf16    (unsplit)
    float* __restrict__ Cpart,                // (ksplit, M, N) (split) or null
    int M, int N, int K, int kchunk) {
  __shared__ __attribute__((aligned(16))) unsigned char alds[MT * 16 * W8_AST];
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int li = lane & 15;
  const int q = lane >> 4;
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int n0 = tile * 64 + wave * 16;
  const int split = blockIdx.y;
  const int k0 = split * kchunk;
  const int k1 = min(K, k0 + kchunk);
  const int ntiles = (k1 - k0) / 128;       // >= 1 by the host plan
  const int nchunks = (ntiles + W8_DEPTH - 1) / W8_DEPTH;

  // this wave's tile stream: row group n0/16, tiles k0/128 ..
  const unsigned char* wbase =
      Wp + w8_packed_offset(n0 / 16, k0 / 128, K) + lane * 16;
  int4v w[W8_DEPTH][2];
  auto issue_w = [&](int d, int j) {        // ring slot d <- tile j (clamped)
    const unsigned char* p = wbase + (long)min(j, ntiles - 1) * W8_TILE_BYTES;
    w[d][0] = w8_load<NT>(p);
    w[d][1] = w8_load<NT>(p + 1024);
  };

  // A staging: pass p copies row p*4 + wave, 1 KB per wave load
  int4v areg[MT * 4];
  auto load_a = [&](int c) {
    // past the split's end: re-read its last 16 B, zeroed by store_a (no
    // branch, so the k loop stays one basic block and its schedule holds)
    const int kcl = min(k0 + c * W8_KC + lane * 16, k1 - 16);
#pragma unroll
    for (int p = 0; p < MT * 4; ++p) {
      const int row = min(p * 4 + wave, M - 1);
      areg[p] = *reinterpret_cast<const int4v*>(A8 + (long)row * K + kcl);
    }
  };
  auto store_a = [&](int c) {
    const bool live = k0 + c * W8_KC + lane * 16 < k1;
#pragma unroll
    for (int p = 0; p < MT * 4; ++p) {
      int4v v;
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = live ? areg[p][i] : 0;
      *reinterpret_cast<int4v*>(alds + (p * 4 + wave) * W8_AST + lane * 16) = v;
    }
  };

  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  load_a(0);
#pragma unroll
  for (int d = 0; d < W8_DEPTH; ++d) issue_w(d, d);
  __builtin_amdgcn_sched_barrier(0);        // the ring fills while A is staged
  store_a(0);
  __syncthreads();

  // A fragments of tile d: read one tile ahead of the MFMA that takes them.
  // The scheduling barriers keep that distance: left alone the compiler
  // hoists a whole chunk's LDS reads (128 VGPRs at MT 2, one wave per SIMD).
  const unsigned char* afrag = alds + li * W8_AST + q * 32;
  int8v a[2][MT];
  auto read_a = [&](int d) {
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const unsigned char* ap = afrag + t * 16 * W8_AST + d * 128;
      const int4v a0 = *reinterpret_cast<const int4v*>(ap);
      const int4v a1 = *reinterpret_cast<const int4v*>(ap + 16);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        a[d & 1][t][i] = a0[i], a[d & 1][t][4 + i] = a1[i];
    }
  };
  int c = 0;
  do {                                      // nchunks >= 1: no guard for the
    load_a(c + 1);                          // ring's first loads to sink past
    read_a(0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int d = 0; d < W8_DEPTH; ++d) {
      if (d + 1 < W8_DEPTH) read_a(d + 1);
      int8v b;
#pragma unroll
      for (int i = 0; i < 4; ++i) b[i] = w[d][0][i], b[4 + i] = w[d][1][i];
#pragma unroll
      for (int t = 0; t < MT; ++t)
        // cbsz 0 / blgp 0: both operands e4m3
        acc[t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            a[d & 1][t], b, acc[t], 0, 0, 0, W8_ONE, 0, W8_ONE);
      issue_w(d, (c + 1) * W8_DEPTH + d);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();                        // every wave is done reading A
    store_a(c + 1);
    __syncthreads();
  } while (++c < nchunks);

  // C layout per wave: row m = t*16 + q*4 + reg, column n0 + li
  const int n = n0 + li;
  if (Cpart == nullptr) {
    const float ws = w_scale[n];
    const float bv = bias ? bf2f(bias[n]) : 0.f;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int m = t * 16 + q * 4 + reg;
        if (m >= M) continue;
        float v = acc[t][reg] * (a_scale[m] * ws) + bv;
        if (R) v += bf2f(R[(long)m * N + n]);
        C[(long)m * N + n] = f2bf(v);
      }
  } else {
    float* dst = Cpart + (long)split * M * N;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int m = t * 16 + q * 4 + reg;
        if (m < M) dst[(long)m * N + n] = acc[t][reg];
      }
  }
}

// Sum the split-K slabs in split order, then the unsplit epilogue.
__global__ __launch_bounds__(256) void gemm_w8_combine_kernel(
    const float* __restrict__ part, const float* __restrict__ a_scale,
    const float* __restrict__ w_scale, const unsigned short* __restrict__ R,
    const unsigned short* __restrict__ bias, unsigned short* __restrict__ C,
    int M, int N, int ksplit) {
  const long total = (long)M * N;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total;
       i += (long)gridDim.x * 256) {
    const int m = (int)(i / N), n = (int)(i % N);
    float s = 0.f;
    for (int p = 0; p < ksplit; ++p) s += part[p * total + i];
    float v = s * (a_scale[m] * w_scale[n]);
    if (bias) v += bf2f(bias[n]);
    if (R) v += bf2f(R[i]);
    C[i] = f2bf(v);
  }
}

// ---------------------------------------------------------------------------
// Row quantiser: X (M, K) bf16 -> a8 (M, K) e4m3 and a_scale (M,) f32, one
// workgroup per row, K % 8 == 0. a_scale = 2^e with the smallest e such that
// amax / 2^e <= 448 (1 where the row is zero); a8 = e4m3_rne(x / 2^e).
// |bf16| orders as its 15 magnitude bits, so amax is an integer max, and e
// comes from those bits: amax = (1 + f/128) * 2^E gives e = E - 8, one more
// when f > 96 (1.75 * 2^8 = 448). v_ldexp_f32 scales exactly and the convert
// rounds once, so codes and scales are those of the reference bit for bit.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void quant_rows_fp8_kernel(
    const unsigned short* __restrict__ X, unsigned char* __restrict__ A8,
    float* __restrict__ a_scale, int K) {
  __shared__ int red[4];
  const unsigned short* x = X + (long)blockIdx.x * K;
  unsigned char* out = A8 + (long)blockIdx.x * K;
  const int nvec = K / 8;
  int amax = 0;
  for (int v = threadIdx.x; v < nvec; v += 256) {
    const short8 s = *reinterpret_cast<const short8*>(x + v * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = max(amax, (int)s[j] & 0x7fff);
  }
#pragma unroll
  for (int m = 1; m < WAVE; m <<= 1) amax = max(amax, __shfl_xor(amax, m));
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = amax;
  __syncthreads();
  amax = max(max(red[0], red[1]), max(red[2], red[3]));

  int e = 0;
  if (amax != 0) {
    int E = (amax >> 7) - 127, f = amax & 0x7f;
    if ((amax >> 7) == 0) {                 // bf16 subnormal: f * 2^-133
      const int p = 31 - __builtin_clz(f);
      E = p - 133;
      f = (f << (7 - p)) & 0x7f;
    }
    e = E - 8 + (f > 96 ? 1 : 0);
  }
  if (threadIdx.x == 0) {
    // 2^e as f32 bits; e >= -141, subnormal below -126
    const unsigned int bits =
        e >= -126 ? (unsigned int)(e + 127) << 23 : 1u << (e + 149);
    a_scale[blockIdx.x] = __builtin_bit_cast(float, bits);
  }
  for (int v = threadIdx.x; v < nvec; v += 256) {
    const short8 s = *reinterpret_cast<const short8*>(x + v * 8);
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      y[j] = __builtin_ldexpf(bf2f((unsigned short)s[j]), -e);
    int2v o;
    o[0] = f2fp8x4(y[0], y[1], y[2], y[3]);
    o[1] = f2fp8x4(y[4], y[5], y[6], y[7]);
    *reinterpret_cast<int2v*>(out + v * 8) = o;
  }
}
