// Ring attention for gfx950: one ring step. attn_ring_fold_kernel folds a
// visiting dense K/V block into the online-softmax state of this rank's
// queries (parallel/sequence.py drives it; ops.reference.attn_ring_fold is the
// definition).
//
// Operands: q logical (B, Hq, T, D) bf16 through (batch, head, token) strides,
//   k/v (B, Hkv, S, D) bf16 likewise, D 64 or 128. Only the difference
//   rel = k_pos0 - q_pos0 of the two global start positions reaches the
//   kernel: key c is visible to query t iff rel + c <= t, and with a window
//   also rel + c > t - window.
//
// State: acc (B, Hq, T, D) f32, unnormalised, and ml (B, Hq, T, 2) f32 holding
//   the running max (exp2 domain, -inf while the row has seen no key) and the
//   running sum. state_in null starts from (0, -inf, 0) in registers; `last`
//   normalises and stores bf16 out (B, T, Hq, D) instead of the state, so a
//   ring of n visible blocks is n launches. A row whose keys are all masked
//   keeps its state bit for bit: the max is a true -inf, exp2(-inf - m) is 0
//   and the correction factor exp2(m - m) multiplies by exactly 1.
//
// Work split (not the training forward's): a workgroup owns one (batch, KV
//   head) and 64 consecutive rows of the flattened (token, group head) index
//   R = t * G + g, 4 waves x 16 rows. The G query heads of a KV head therefore
//   share every staged K/V tile (LDS and L2 traffic per MFMA drop by G), any G
//   works (MQA, G = 5), and a workgroup spans only 64 / G tokens, so the
//   diagonal block wastes less of its last tile on masked keys. Key tiles with
//   no visible key for the workgroup are cut from the tile range; a tile that
//   every row of a wave sees whole takes the MASK = false body, which has no
//   position arithmetic; a wave whose rows see none of a tile skips it.
//
// Data movement: 64-key tiles. The next tile's global loads are issued into
//   registers before the current tile is multiplied and land in LDS after it
//   (register double buffer, one LDS image). Both products run transposed,
//   S^T = K Q^T and O^T = V^T P^T, with v_mfma_f32_16x16x32_bf16: the S^T
//   accumulator of a lane then holds 16 keys of ONE query, so the row max needs
//   two cross-lane steps, the row sum none until the epilogue, m and l are one
//   register each, and P^T is already the B operand of the second product: it
//   never passes through LDS. The MFMA's k index is free as long as both
//   operands agree, so a lane's 8 keys are {hi*4 .. +3} of two adjacent 16-key
//   blocks, which is what its S^T registers hold, and the V^T fragment is two
//   8-byte LDS reads at those keys.
//
// V layout: V travels the ring row-major, (B, Hkv, S, D), as K does. A d-major
//   payload would give 16-byte loads straight into the V^T image, but it needs
//   S padded to 8 keys, a transposing launch by the owner every layer and a
//   second layout in the public op; it was not built. Instead each thread
//   loads 4 keys x 8 d (four 16-byte loads), transposes them in registers and
//   writes 8 d-rows of 4 keys (8-byte LDS stores): a quarter of the LDS store
//   instructions of the training forward's 2-byte scatter. Row strides (K
//   D*2+16 B, V^T 144 B) keep fragment reads and these stores conflict-free.
//
// Numerics: scores, softmax and both accumulators f32, exp2 domain. P is
//   rounded to bf16 once (unnormalised, as the second product's operand) and O
//   once, at `last`: attn_train.hip's rounding points.

#include "common.h"

static constexpr int RG_KT = 64;       // keys per LDS tile
static constexpr int RG_ROWS = 64;     // (token, group head) rows per workgroup
static constexpr int RG_THREADS = 256;
static constexpr int RG_VROW_B = RG_KT * 2 + 16;  // V^T image row, bytes

// Global loads of one tile into registers: K as D/32 16-byte chunks per
// thread, V as one 4-key x 8-d item (D = 64: the first 128 threads only).
// Keys at or past S read as zero.
template <int D>
DEVINL void ring_load_tile(const unsigned short* __restrict__ k,
                           const unsigned short* __restrict__ v, long kbase,
                           long vbase, long k_st, long v_st, int kb, int S,
                           short8 (&kr)[D / 32], short8 (&vr)[4], int tid) {
#pragma unroll
  for (int i = 0; i < D / 32; ++i) {
    const int idx = tid + RG_THREADS * i;
    const int key = kb + idx / (D / 8);
    kr[i] = short8{};
    if (key < S)
      kr[i] = *reinterpret_cast<const short8*>(
          k + kbase + (long)key * k_st + (idx % (D / 8)) * 8);
  }
  if (tid < 16 * (D / 8)) {
    const int kg = tid % 16, dc = tid / 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int key = kb + kg * 4 + i;
      vr[i] = short8{};
      if (key < S)
        vr[i] = *reinterpret_cast<const short8*>(
            v + vbase + (long)key * v_st + dc * 8);
    }
  }
}

// Registers -> LDS: K row-major [key][d], V transposed [d][key].
template <int D>
DEVINL void ring_store_tile(unsigned char* k_lds, unsigned char* v_lds,
                            const short8 (&kr)[D / 32], const short8 (&vr)[4],
                            int tid) {
  constexpr int KROW_B = D * 2 + 16;
#pragma unroll
  for (int i = 0; i < D / 32; ++i) {
    const int idx = tid + RG_THREADS * i;
    *reinterpret_cast<short8*>(k_lds + (idx / (D / 8)) * KROW_B +
                               (idx % (D / 8)) * 16) = kr[i];
  }
  if (tid < 16 * (D / 8)) {
    const int kg = tid % 16, dc = tid / 16;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const short4v col = {vr[0][j], vr[1][j], vr[2][j], vr[3][j]};
      *reinterpret_cast<short4v*>(v_lds + (dc * 8 + j) * RG_VROW_B + kg * 8) = col;
    }
  }
}

// One 64-key tile against a wave's 16 rows. Lane (li, hi): query row li, keys
// 16n + hi*4 + reg of the tile. relk = rel + kb, tq = the lane's token.
template <int D, bool MASK>
DEVINL void ring_compute_tile(const unsigned char* k_lds,
                              const unsigned char* v_lds,
                              const bf16x8 (&qfrag)[D / 32], f32x4 (&acc)[D / 16],
                              float& m, float& l, float sc2, int li, int hi,
                              int kb, int S, int relk, int tq, int window) {
  constexpr int KROW_B = D * 2 + 16;
  constexpr int NKK = D / 32;
  constexpr int NDT = D / 16;
  constexpr int NB = RG_KT / 16;
  const float ninf = -__builtin_inff();

  f32x4 s[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    s[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
      const bf16x8 kf = as_bf16x8(*reinterpret_cast<const short8*>(
          k_lds + (16 * n + li) * KROW_B + hi * 16 + 64 * kk));
      s[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qfrag[kk], s[n], 0, 0, 0);
    }
  }

  float rm = ninf;
#pragma unroll
  for (int n = 0; n < NB; ++n)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      float x = s[n][reg] * sc2;
      if (MASK) {
        const int key = 16 * n + hi * 4 + reg;
        const int kp = relk + key;
        const bool dead = (kb + key >= S) | (kp > tq) |
                          (window > 0 && kp <= tq - window);
        x = dead ? ninf : x;
      }
      s[n][reg] = x;
      rm = fmaxf(rm, x);
    }
  rm = fmaxf(rm, __shfl_xor(rm, 16));
  rm = fmaxf(rm, __shfl_xor(rm, 32));
  const float mn = fmaxf(m, rm);
  const float msafe = (mn == ninf) ? 0.f : mn;  // row has seen no key yet
  const float corr = fast_exp2(m - msafe);
  float psum = 0.f;
  bf16x8 pfrag[NB / 2];
#pragma unroll
  for (int n = 0; n < NB; ++n) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const float p = fast_exp2(s[n][reg] - msafe);
      psum += p;
      s[n][reg] = p;
    }
  }
#pragma unroll
  for (int c = 0; c < NB / 2; ++c) {
    short8 pk;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      pk[reg] = (short)f2bf(s[2 * c][reg]);
      pk[4 + reg] = (short)f2bf(s[2 * c + 1][reg]);
    }
    pfrag[c] = as_bf16x8(pk);
  }
  l = l * corr + psum;
  m = mn;

#pragma unroll
  for (int nd = 0; nd < NDT; ++nd) {
    acc[nd] *= corr;
#pragma unroll
    for (int c = 0; c < NB / 2; ++c) {
      const unsigned char* vp =
          v_lds + (16 * nd + li) * RG_VROW_B + (32 * c + hi * 4) * 2;
      const short4v a = *reinterpret_cast<const short4v*>(vp);
      const short4v b = *reinterpret_cast<const short4v*>(vp + 32);
      const bf16x8 vf =
          as_bf16x8(__builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
      acc[nd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pfrag[c], acc[nd], 0, 0, 0);
    }
  }
}


template <int D>
__global__ __launch_bounds__(RG_THREADS) void attn_ring_fold_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v,
    const float* __restrict__ acc_in,  // (B, Hq, T, D) or null
    const float* __restrict__ ml_in,   // (B, Hq, T, 2) or null
    float* __restrict__ acc_out, float* __restrict__ ml_out,  // !last
    unsigned short* __restrict__ out,  // last: (B, T, Hq, D) contiguous
    int Hq, int G, int T, int S, int ntile, int rel, int window, float scale,
    int last, long q_sb, long q_sh, long q_st, long k_sb, long k_sh, long k_st,
    long v_sb, long v_sh, long v_st) {
  constexpr int KROW_B = D * 2 + 16;
  constexpr int NKK = D / 32;
  constexpr int NDT = D / 16;

  __shared__ __attribute__((aligned(16))) unsigned char lds[
      RG_KT * KROW_B + D * RG_VROW_B];
  unsigned char* k_lds = lds;
  unsigned char* v_lds = lds + RG_KT * KROW_B;

  // the diagonal block's late tiles see the most keys: start them first
  const int tile = ntile - 1 - (int)(blockIdx.x % ntile);
  const int bk = blockIdx.x / ntile;
  const int Hkv = Hq / G;
  const int b = bk / Hkv, kvh = bk % Hkv;
  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int li = lane & 15;
  const int hi = lane >> 4;
  const float sc2 = scale * LOG2E;
  const float ninf = -__builtin_inff();
  const long GT = (long)G * T;

  // this lane's row of the flattened (token, group head) index
  const long R0 = (long)tile * RG_ROWS;
  const long Rraw = R0 + wave * 16 + li;
  const long R = Rraw < GT ? Rraw : GT - 1;
  const int tq = (int)(R / G);
  const int h = kvh * G + (int)(R % G);
  const long row = ((long)b * Hq + h) * T + tq;

  bf16x8 qfrag[NKK];
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk)
    qfrag[kk] = as_bf16x8(*reinterpret_cast<const short8*>(
        q + (long)b * q_sb + (long)h * q_sh + (long)tq * q_st + hi * 8 + 32 * kk));

  // state: m per query row (every lane of the row), l as per-lane partial
  // sums (the carried sum rides in the hi = 0 lane), O^T accumulators with
  // d = 16 nd + hi*4 + reg
  float m = ninf, l = 0.f;
  f32x4 acc[NDT];
#pragma unroll
  for (int nd = 0; nd < NDT; ++nd) acc[nd] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (acc_in != nullptr) {
    m = ml_in[row * 2];
    l = (hi == 0) ? ml_in[row * 2 + 1] : 0.f;
#pragma unroll
    for (int nd = 0; nd < NDT; ++nd)
      acc[nd] = *reinterpret_cast<const f32x4*>(acc_in + row * D + 16 * nd + hi * 4);
  }

  // key range some row of the workgroup can see, and of this wave
  const long Rend = (R0 + RG_ROWS - 1 < GT ? R0 + RG_ROWS - 1 : GT - 1);
  const long tmin = R0 / G, tmax = Rend / G;
  const long hi_l = tmax - rel + 1;
  const long lo_l = window > 0 ? tmin - window + 1 - rel : 0;
  const int c_hi = (int)(hi_l < S ? (hi_l > 0 ? hi_l : 0) : S);
  const int c_lo = (int)(lo_l > 0 ? lo_l : 0);
  const long Rw0 = R0 + wave * 16;
  const long Rw1 = (Rw0 + 15 < GT ? Rw0 + 15 : GT - 1);
  const int wtmin = (int)((Rw0 < GT ? Rw0 : GT - 1) / G);
  const int wtmax = (int)(Rw1 / G);

  const long kbase = (long)b * k_sb + (long)kvh * k_sh;
  const long vbase = (long)b * v_sb + (long)kvh * v_sh;

  short8 kr[NKK], vr[4];
  if (c_lo < c_hi)
    ring_load_tile<D>(k, v, kbase, vbase, k_st, v_st, c_lo, S, kr, vr, tid);
  for (int kb = c_lo; kb < c_hi; kb += RG_KT) {
    __syncthreads();  // the previous tile's fragment reads are done
    ring_store_tile<D>(k_lds, v_lds, kr, vr, tid);
    __syncthreads();
    if (kb + RG_KT < c_hi)  // in flight while this tile is multiplied
      ring_load_tile<D>(k, v, kbase, vbase, k_st, v_st, kb + RG_KT, S, kr, vr, tid);

    const int relk = rel + kb;
    // wave-uniform: nothing visible (future, or below every row's window)
    if (relk > wtmax) continue;
    if (window > 0 && relk + RG_KT - 1 <= wtmin - window) continue;
    const bool whole = (kb + RG_KT <= S) && (relk + RG_KT - 1 <= wtmin) &&
                       (window == 0 || relk > wtmax - window);
    if (whole)
      ring_compute_tile<D, false>(k_lds, v_lds, qfrag, acc, m, l, sc2, li, hi,
                                  kb, S, relk, tq, window);
    else
      ring_compute_tile<D, true>(k_lds, v_lds, qfrag, acc, m, l, sc2, li, hi,
                                 kb, S, relk, tq, window);
  }

  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (Rraw >= GT) return;
  if (last) {
    const float inv = (l > 0.f) ? 1.f / l : 0.f;  // a row that saw no key: zeros
    unsigned short* op = out + (((long)b * T + tq) * Hq + h) * D + hi * 4;
#pragma unroll
    for (int nd = 0; nd < NDT; ++nd) {
      short4v o;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) o[reg] = (short)f2bf(acc[nd][reg] * inv);
      *reinterpret_cast<short4v*>(op + 16 * nd) = o;
    }
  } else {
    if (hi == 0) *reinterpret_cast<f32x2*>(ml_out + row * 2) = (f32x2){m, l};
#pragma unroll
    for (int nd = 0; nd < NDT; ++nd)
      *reinterpret_cast<f32x4*>(acc_out + row * D + 16 * nd + hi * 4) = acc[nd];
  }
}
