// Tiled fp8 (e4m3) weight-tier GEMM for gfx950, M > 32 (W8A8):
//   C(M,N) bf16 = a_scale[m] * w_scale[n] * sum_k a8[m,k] * codes[n,k]
//                 [+bias] [+R]
// K % 128 == 0, N % 64 == 0. It reads the pack_w8 copy the decode kernel
// (gemm_w8.hip) reads and the a8 / a_scale quant_rows_fp8_kernel writes; both
// operands enter v_mfma_scale_f32_16x16x128_f8f6f4 as e4m3 with block scales
// 1.0 and every scale is a power of two, so the bf16 store is the only
// rounding after the f32 accumulation, as in the decode kernel.
//
// The decode kernel gives a wave one 16-column row group and 16 or 32 rows: a
// weight tile is used for two MFMAs at most. Here a weight tile is fetched
// once per block tile and multiplied with up to 128 rows:
//
//  * Block tile BM x 128, BM in {64, 128}, 256 threads. Wave w owns the 32
//    columns n0 + w*32 .. +32 (row groups g and g + 1 of the packed weight)
//    and ALL BM rows: MT = BM/16 m-tiles x 2 B fragments of f32x4
//    accumulators, 64 VGPRs at BM = 128.
//  * Weight path, global -> VGPR: a (g, kb) tile is two lane-linear 1 KB
//    halves, and a lane's 2 x 16 B are its B operand of one MFMA as they
//    arrive. A k-step is 2 tiles = 16 VGPRs per wave. A ring of W8T_NSET = 4
//    register sets keeps the tiles of the next 3 k-steps in flight across
//    the barriers: 3 x 4 waves x 4 KB = 48 KB per workgroup.
//  * Activation path: a8 goes through LDS once per 128-k step for the four
//    waves, 16 B per thread and piece (BM/32 pieces), 8 consecutive lanes one
//    128 B row segment. Rows are W8T_AST = 144 bytes apart: a fragment read is
//    16 B at row*144 + q*32 + h*16, 16 B slot (9*row + 2q + h) % 16 of the
//    256 B bank row, and 9 is odd, so the 16 lanes a b128 read serves together
//    (one q, 16 rows) hit 16 different slots. A staging store of 16 lanes
//    covers two rows, slots 9r .. 9r+7 and 9r+9 .. 9r+16: one slot twice, a
//    single two-way conflict per store, on a path 1/MT as busy as the reads.
//    Two buffers: step s is multiplied out of buffer s & 1 while the rows of
//    step s + 1, loaded to registers before the MFMAs, are stored to the other
//    one behind them. One barrier per step.
//  * Fragment reuse and the LDS budget. An A fragment is 16 rows x 128 B =
//    2 KB per wave; the fp8 16x16x128 MFMA occupies its SIMD for 32 clocks
//    (8 passes); LDS delivers 128 B/clk/CU. One B fragment per A fragment
//    would ask the four waves for 4 x 2 KB per 32 clk = 256 B/clk, twice what
//    LDS has. Two B fragments per A fragment (this kernel) ask for 8 KB per
//    64 clk = 128 B/clk: the LDS rate, met only when the kernel is MFMA-bound
//    (large M). The staging stores add BM*128 B per BM/16*2*32 clk = 2 B/clk.
//    LDS use: 2 * BM * 144 B = 18 KB (BM 64) / 36 KB (BM 128).
//  * The k loop is branch-free: it runs whole turns of the ring (W8T_NSET
//    steps, set indices and buffer parity compile-time constants). Past the
//    split's last step the W tile index is clamped to it, the a8 address too,
//    and the staged bytes are zeroed: the surplus MFMAs add 0 * finite.
//  * N is only a multiple of 64: in a last half column tile waves 2 and 3 lie
//    past N. They stay in the barriers and stage A like the others; their row
//    groups are clamped to the last one (valid memory) and their stores are
//    predicated. Rows past M: loads clamp to row M - 1, stores are predicated.
//  * Grid (column tiles * m-tiles, k-splits). blockIdx.x is XCD-remapped and
//    THEN split into (column tile, m-tile), m-tile fastest: the blocks that
//    read one weight tile run on one XCD next to each other in its dispatch
//    order, so all but the first find it in that XCD's L2. The W loads are
//    plain (not nontemporal) for that reason.
//  * Split-K in whole 128-k steps to f32 slabs (ksplit, M, N), finished by
//    gemm_w8_combine_kernel. No atomics, no host sync.

// common.h, int8v, W8_ONE and gemm_w8_combine_kernel come from gemm_w8.hip,
// included before this file.

static constexpr int W8T_NSET = 4;      // W register sets: 3 k-steps ahead
static constexpr int W8T_AST = 128 + 16;  // LDS row stride, bytes

template <int BM>  // rows per block tile: 64 or 128
__global__ __launch_bounds__(256) void gemm_w8_tiled_kernel(
    const unsigned char* __restrict__ A8,     // (M, K) e4m3
    const unsigned char* __restrict__ Wp,     // tiled e4m3 codes of (N, K)
    const float* __restrict__ a_scale,        // (M,)
    const float* __restrict__ w_scale,        // (N,)
    const unsigned short* __restrict__ R,     // (M, N) bf16 or null
    const unsigned short* __restrict__ bias,  // (N,) bf16 or null
    unsigned short* __restrict__ C,           // (M, N) bf16    (unsplit)
    float* __restrict__ Cpart,                // (ksplit, M, N) (split) or null
    int M, int N, int K, int mtiles, int kchunk) {
  constexpr int MT = BM / 16;
  constexpr int NPIECE = BM / 32;
  __shared__ __attribute__((aligned(16))) unsigned char alds[2][BM * W8T_AST];

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int li = lane & 15;
  const int q = lane >> 4;

  const int t = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (t % mtiles) * BM;
  const int n0 = (t / mtiles) * 128 + wave * 32;
  const int split = blockIdx.y;
  const int k0 = split * kchunk;
  const int k1 = min(K, k0 + kchunk);
  const int nsteps = (k1 - k0) / 128;       // >= 1 by the host plan
  const int nturns = (nsteps + W8T_NSET - 1) / W8T_NSET;

  // this wave's two tile streams; a wave past N re-reads the last row groups
  const int g0 = min(n0, N - 32) / 16;
  const unsigned char* wbase[2];
#pragma unroll
  for (int f = 0; f < 2; ++f)
    wbase[f] = Wp + w8_packed_offset(g0 + f, k0 / 128, K) + lane * 16;
  int4v w[W8T_NSET][2][2];
  auto issue_w = [&](int set, int s) {      // ring set <- k-step s (clamped)
    const long off = (long)min(s, nsteps - 1) * W8_TILE_BYTES;
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      w[set][f][0] = *reinterpret_cast<const int4v*>(wbase[f] + off);
      w[set][f][1] = *reinterpret_cast<const int4v*>(wbase[f] + off + 1024);
    }
  };

  // A staging: piece j of a thread is the 16 B chunk flat % 8 of staged row
  // flat / 8, flat = tid + j*256; rows past M re-read row M - 1.
  int4v areg[NPIECE];
  const unsigned char* aptr[NPIECE];
  int aoff[NPIECE];
#pragma unroll
  for (int j = 0; j < NPIECE; ++j) {
    const int flat = threadIdx.x + j * 256;
    aptr[j] = A8 + (long)min(m0 + flat / 8, M - 1) * K + k0 + (flat % 8) * 16;
    aoff[j] = (flat / 8) * W8T_AST + (flat % 8) * 16;
  }
  auto load_a = [&](int s) {
    const int so = min(s, nsteps - 1) * 128;
#pragma unroll
    for (int j = 0; j < NPIECE; ++j)
      areg[j] = *reinterpret_cast<const int4v*>(aptr[j] + so);
  };
  auto store_a = [&](int s, int buf) {
    const bool live = s < nsteps;
#pragma unroll
    for (int j = 0; j < NPIECE; ++j) {
      int4v v;
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = live ? areg[j][i] : 0;
      *reinterpret_cast<int4v*>(&alds[buf][aoff[j]]) = v;
    }
  };

  f32x4 acc[MT][2];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int f = 0; f < 2; ++f) acc[i][f] = (f32x4){0.f, 0.f, 0.f, 0.f};

  auto mfma_step = [&](int set, int buf) {
    int8v b[2];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        b[f][i] = w[set][f][0][i], b[f][4 + i] = w[set][f][1][i];
    const unsigned char* afrag = &alds[buf][li * W8T_AST + q * 32];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int4v a0 = *reinterpret_cast<const int4v*>(afrag + i * 16 * W8T_AST);
      const int4v a1 =
          *reinterpret_cast<const int4v*>(afrag + i * 16 * W8T_AST + 16);
      int8v a;
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] = a0[e], a[4 + e] = a1[e];
      // cbsz 0 / blgp 0: both operands e4m3
#pragma unroll
      for (int f = 0; f < 2; ++f)
        acc[i][f] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            a, b[f], acc[i][f], 0, 0, 0, W8_ONE, 0, W8_ONE);
    }
  };

  load_a(0);
#pragma unroll
  for (int d = 0; d < W8T_NSET - 1; ++d) issue_w(d, d);
  store_a(0, 0);
  __syncthreads();

  int s = 0;
  do {                                      // nturns >= 1
#pragma unroll
    for (int j = 0; j < W8T_NSET; ++j) {    // set and buffer: constants per copy
      // A first: store_a waits for it, and in-order completion must not make
      // that wait cover the younger weight loads
      load_a(s + j + 1);
      issue_w((j + W8T_NSET - 1) % W8T_NSET, s + j + W8T_NSET - 1);
      // left alone the compiler sinks these loads between the MFMAs, where
      // the wait for this step's W tiles then covers them too
      __builtin_amdgcn_sched_barrier(0);
      mfma_step(j, j & 1);
      // the other buffer was last read in the step before, a barrier ago
      store_a(s + j + 1, (j + 1) & 1);
      __syncthreads();
    }
    s += W8T_NSET;
  } while (s < nturns * W8T_NSET);

  // C row = m0 + i*16 + q*4 + reg, col = n0 + f*16 + li
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int n = n0 + f * 16 + li;
    if (n >= N) continue;
    const float ws = Cpart == nullptr ? w_scale[n] : 0.f;
    const float bv = (bias != nullptr && Cpart == nullptr) ? bf2f(bias[n]) : 0.f;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int m = m0 + i * 16 + q * 4 + reg;
        if (m >= M) continue;
        const long o = (long)m * N + n;
        if (Cpart != nullptr) {
          Cpart[(long)split * M * N + o] = acc[i][f][reg];
        } else {
          float v = acc[i][f][reg] * (a_scale[m] * ws) + bv;
          if (R != nullptr) v += bf2f(R[o]);
          C[o] = f2bf(v);
        }
      }
  }
}
