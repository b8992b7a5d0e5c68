// Prefill (multi-token) paged attention for head dim 512 on gfx950 — the
// Gemma-4 global layers. Same contract as attn_prefill_kernel (strided q/out,
// token-major K pool, d-major V pool, ragged q_start, GQA, window, ALiBi,
// tree mask, exp2-domain fp32 softmax, P rounded to bf16), but a work split
// of its own: at D=512 one wave's 16x512 fp32 output tile alone is 128 VGPRs,
// so attn_prefill_kernel<512> spills.
//
// Structure: grid = (ceil(Tq/64), B*Hq); block = 512 (8 waves) = 4 row groups
//   x 2 d-halves. The two waves of a pair own the same 16 q rows; wave dh
//   holds the Q fragments (32 VGPRs) and the output accumulator (64 VGPRs) of
//   d in [256 dh, 256 dh + 256) — the register profile of the D=256 kernel.
//   QK^T: each wave contracts its 256 d (8 k-slices per 16-key n-tile) into a
//   partial S, the pair swaps partials through LDS (lane to lane, one
//   ds_write_b128 / ds_read_b128 per n-tile, ordered by a workgroup barrier)
//   and each adds the other's: a + b == b + a in fp32, so both waves hold
//   bit-identical S and therefore bit-identical m, l and P with no broadcast.
//   P.V: each wave relays its P through its own LDS slab (C -> A layout) and
//   multiplies against its 16 d-tiles of V^T only.
//
// LDS (dynamic, 100 864 B -> one workgroup per CU):
//   K tile   32 keys x (512*2 + 16) B     33 280
//   V^T      512 d   x (32*2 + 16) B      40 960
//   P        8 waves x 16 x 80 B          10 240
//   S swap   8 waves x 16 x 32 fp32       16 384

#include "common.h"

static constexpr int PW_D = 512;        // head dim
static constexpr int PW_DH = 256;       // d per wave
static constexpr int PW_QROWS = 64;     // q rows per workgroup
static constexpr int PW_KVBLK = 32;     // keys per staged tile
static constexpr int PW_KROW_B = PW_D * 2 + 16;
static constexpr int PW_VROW_B = PW_KVBLK * 2 + 16;
static constexpr int PW_PROW_B = PW_KVBLK * 2 + 16;
static constexpr int PW_K_OFF = 0;
static constexpr int PW_V_OFF = PW_K_OFF + PW_KVBLK * PW_KROW_B;
static constexpr int PW_P_OFF = PW_V_OFF + PW_D * PW_VROW_B;
static constexpr int PW_S_OFF = PW_P_OFF + 8 * 16 * PW_PROW_B;
static constexpr int PW_LDS_BYTES = PW_S_OFF + 8 * 16 * PW_KVBLK * 4;

__global__ __launch_bounds__(512) void attn_prefill_wide_kernel(
    const unsigned short* __restrict__ q,        // strided, see q_s*
    const unsigned short* __restrict__ k_pages,  // (np, Hkv, P, 512)
    const unsigned short* __restrict__ v_pages,  // (np, Hkv, 512, P)
    const int* __restrict__ page_table,          // (B, maxp)
    const int* __restrict__ q_start,             // (B,)
    const float* __restrict__ alibi,             // (Hq,) slopes or null
    const unsigned char* __restrict__ tree_mask, // (B, Tq, Tq) bool or null
    unsigned short* __restrict__ out,
    int B, int Hq, int G, int Tq, int P, int maxp, int window, float scale,
    long q_sb, long q_st, long q_sh, long o_sb, long o_st, long o_sh) {
  constexpr int NKK = PW_DH / 32;   // QK^T k-slices per wave
  constexpr int NDT = PW_DH / 16;   // PV d-tiles per wave

  extern __shared__ __attribute__((aligned(16))) unsigned char pw_lds[];
  unsigned char* k_lds = pw_lds + PW_K_OFF;
  unsigned char* v_lds = pw_lds + PW_V_OFF;

  const int qtile = blockIdx.x;
  const int bh = blockIdx.y;
  const int b = bh / Hq, h = bh % Hq;
  const int kvh = h / G;
  const int Hkv = Hq / G;
  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int li = lane & 15;      // fragment row/col index
  const int hi = lane >> 4;      // fragment k-quad
  const int dh = wave & 1;       // d-half of this wave
  const int rbase = qtile * PW_QROWS + (wave >> 1) * 16;  // pair's first q row
  const int d0 = dh * PW_DH;
  const int qs = q_start[b];
  const int ctx = qs + Tq;
  const float sc2 = scale * LOG2E;
  const float aslope = (alibi != nullptr) ? alibi[h] * LOG2E : 0.f;

  unsigned char* pw = pw_lds + PW_P_OFF + wave * 16 * PW_PROW_B;
  f32x4* s_mine = reinterpret_cast<f32x4*>(pw_lds + PW_S_OFF) +
                  wave * (PW_KVBLK / 16) * WAVE + lane;
  const f32x4* s_peer = reinterpret_cast<const f32x4*>(pw_lds + PW_S_OFF) +
                        (wave ^ 1) * (PW_KVBLK / 16) * WAVE + lane;

  // ---- Q fragments of this d-half: row = li, k = hi*8 + j (+32*kk) ----
  const int my_qrow = min(rbase + li, Tq - 1);
  bf16x8 qfrag[NKK];
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk) {
    qfrag[kk] = as_bf16x8(*reinterpret_cast<const short8*>(
        q + (long)b * q_sb + (long)my_qrow * q_st + (long)h * q_sh + d0 +
        hi * 8 + 32 * kk));
  }

  // online-softmax state: this lane's 4 C-rows (r = hi*4 + reg)
  float m2[4], l[4];
  f32x4 acc_o[NDT];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m2[r] = NEG_BIG; l[r] = 0.f; }
#pragma unroll
  for (int n = 0; n < NDT; ++n) acc_o[n] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // key range this q-tile can see: [kstart, kmax). Tree queries are not
  // causal among themselves. Both bounds are uniform over the workgroup, so
  // every wave meets every barrier below.
  const int qpos_max = qs + min(qtile * PW_QROWS + PW_QROWS - 1, Tq - 1);
  const int kmax = (tree_mask != nullptr) ? ctx : min(ctx, qpos_max + 1);
  int kstart = 0;
  if (window > 0)
    kstart = max(0, ((qs + qtile * PW_QROWS) - window + 1) / PW_KVBLK * PW_KVBLK);

  // ---- staging: each thread moves 4 K pieces (rows kt + 8i at d = kd8) and
  // 4 V^T pieces (d = vd + 128i at key octet vo8), one 16 B global load and
  // one 16 B LDS store per piece. The loads of tile i+1 are issued into
  // registers before the MFMAs of tile i and stored after them, so HBM
  // latency overlaps the math of the one workgroup a CU holds.
  constexpr int KPIECES = PW_KVBLK * (PW_D / 8) / 512;   // 4
  constexpr int VPIECES = PW_D * (PW_KVBLK / 8) / 512;   // 4
  const int kt = tid / (PW_D / 8), kd8 = (tid % (PW_D / 8)) * 8;
  const int vd = tid / (PW_KVBLK / 8), vo8 = (tid % (PW_KVBLK / 8)) * 8;
  // The page-table entries run one tile ahead of the data, so a tile's
  // K/V loads never wait behind their own table lookup.
  short8 kreg[KPIECES], vreg[VPIECES];
  int kpage[KPIECES], vpage;
  auto load_pages = [&](int kbase) {
#pragma unroll
    for (int i = 0; i < KPIECES; ++i) {
      const int kpos = kbase + kt + 8 * i;
      kpage[i] = (kpos < ctx) ? page_table[b * maxp + kpos / P] : 0;
    }
    const int vpos = kbase + vo8;
    vpage = (vpos < ctx) ? page_table[b * maxp + vpos / P] : 0;
  };
  auto load_tile = [&](int kbase) {   // after load_pages(kbase)
#pragma unroll
    for (int i = 0; i < KPIECES; ++i) {
      const int kpos = kbase + kt + 8 * i;
      kreg[i] = short8{};
      if (kpos < ctx)
        kreg[i] = *reinterpret_cast<const short8*>(
            k_pages + (((long)kpage[i] * Hkv + kvh) * P + (kpos % P)) * PW_D + kd8);
    }
    // the pool is d-major, so 8 positions at fixed d are contiguous (kbase
    // is PW_KVBLK-aligned => an octet never straddles a page)
    const int vpos = kbase + vo8;
#pragma unroll
    for (int i = 0; i < VPIECES; ++i) {
      vreg[i] = short8{};
      if (vpos < ctx)
        vreg[i] = *reinterpret_cast<const short8*>(
            v_pages + (((long)vpage * Hkv + kvh) * PW_D + vd + 128 * i) * P +
            (vpos % P));
    }
  };

  if (kstart < kmax) {
    load_pages(kstart);
    load_tile(kstart);
    load_pages(kstart + PW_KVBLK);   // positions >= ctx are not looked up
  }
  for (int kbase = kstart; kbase < kmax; kbase += PW_KVBLK) {
    __syncthreads();  // everyone done with the previous tile and its S swap
#pragma unroll
    for (int i = 0; i < KPIECES; ++i)
      *reinterpret_cast<short8*>(k_lds + (kt + 8 * i) * PW_KROW_B + kd8 * 2) = kreg[i];
#pragma unroll
    for (int i = 0; i < VPIECES; ++i)
      *reinterpret_cast<short8*>(v_lds + (vd + 128 * i) * PW_VROW_B + vo8 * 2) = vreg[i];
    __syncthreads();
    if (kbase + PW_KVBLK < kmax) {
      load_tile(kbase + PW_KVBLK);
      load_pages(kbase + 2 * PW_KVBLK);
    }

    // ---- partial S over this wave's 256 d: 2 n-tiles of 16 keys ----
    f32x4 s[PW_KVBLK / 16];
#pragma unroll
    for (int n = 0; n < PW_KVBLK / 16; ++n) {
      s[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) {
        bf16x8 bfrag = as_bf16x8(*reinterpret_cast<const short8*>(
            k_lds + (li + 16 * n) * PW_KROW_B + d0 * 2 + hi * 16 + 64 * kk));
        s[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qfrag[kk], bfrag, s[n], 0, 0, 0);
      }
      s_mine[n * WAVE] = s[n];
    }
    __syncthreads();  // the pair's partials are in LDS
#pragma unroll
    for (int n = 0; n < PW_KVBLK / 16; ++n) {
      const f32x4 o = s_peer[n * WAVE];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) s[n][reg] = s[n][reg] + o[reg];
    }

    // ---- mask + online softmax (C layout: row=hi*4+reg, col=li+16n) ----
    float p[PW_KVBLK / 16][4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int qrow = rbase + hi * 4 + reg;
      const int qpos = qs + qrow;
      float rm = NEG_BIG;
#pragma unroll
      for (int n = 0; n < PW_KVBLK / 16; ++n) {
        const int kpos = kbase + li + 16 * n;
        float sv = s[n][reg] * sc2 + aslope * (float)kpos;
        bool dead = (qrow >= Tq) | (kpos >= ctx);
        if (!dead) {
          if (tree_mask != nullptr) {
            if (kpos >= qs)
              dead = !tree_mask[((long)b * Tq + qrow) * Tq + (kpos - qs)];
          } else {
            dead = (kpos > qpos) | (window > 0 && kpos <= qpos - window);
          }
        }
        sv = dead ? NEG_BIG : sv;
        p[n][reg] = sv;
        rm = fmaxf(rm, sv);
      }
      rm = group16_reduce_max(rm);
      const float mn = fmaxf(m2[reg], rm);
      const float corr = fast_exp2(m2[reg] - mn);
      float psum = 0.f;
#pragma unroll
      for (int n = 0; n < PW_KVBLK / 16; ++n) {
        // a dead key weighs 0 even while the row has seen nothing (mn is
        // still NEG_BIG), so a row that sees nothing ends with l == 0
        p[n][reg] = (p[n][reg] > 0.5f * NEG_BIG) ? fast_exp2(p[n][reg] - mn) : 0.f;
        psum += p[n][reg];
      }
      psum = group16_reduce_sum(psum);
      l[reg] = l[reg] * corr + psum;
      m2[reg] = mn;
#pragma unroll
      for (int n = 0; n < NDT; ++n) acc_o[n][reg] *= corr;
    }

    // ---- P -> this wave's LDS slab (C layout scatter), back as A fragment;
    // wave-local, ordered by the wave's own lgkmcnt waits ----
#pragma unroll
    for (int n = 0; n < PW_KVBLK / 16; ++n)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        *(unsigned short*)(pw + (hi * 4 + reg) * PW_PROW_B + (li + 16 * n) * 2) =
            f2bf(p[n][reg]);
    bf16x8 pfrag = as_bf16x8(
        *reinterpret_cast<const short8*>(pw + li * PW_PROW_B + hi * 16));

    // ---- acc_o += P V over this wave's 16 d-tiles ----
#pragma unroll
    for (int n = 0; n < NDT; ++n) {
      bf16x8 vfrag = as_bf16x8(*reinterpret_cast<const short8*>(
          v_lds + (d0 + li + 16 * n) * PW_VROW_B + hi * 16));
      acc_o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pfrag, vfrag, acc_o[n], 0, 0, 0);
    }
  }

  // ---- epilogue: normalize and store this wave's d-half ----
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int qrow = rbase + hi * 4 + reg;
    if (qrow >= Tq) continue;
    const float inv = (l[reg] > 0.f) ? 1.f / l[reg] : 0.f;
#pragma unroll
    for (int n = 0; n < NDT; ++n) {
      out[(long)b * o_sb + (long)qrow * o_st + (long)h * o_sh + d0 + li + 16 * n] =
          f2bf(acc_o[n][reg] * inv);
    }
  }
}
