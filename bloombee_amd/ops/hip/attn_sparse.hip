// Top-k sparse single-token paged attention for gfx950
// (ops.set_attn_sparsity; definition: ops/reference.py attn_paged_topk).
//
// Per (batch row b, QUERY head h): s[c] = scale * q.k[c] (+ slope[h] * c) for
// c < ctx; keep the kkeep = max(1, min(ctx, ceil(sparsity * ctx))) largest
// scores, ties at the threshold going to the lowest positions;
// out = softmax(s[kept]) @ v[kept].
//
// Four launches on one stream, no host sync, ctx_lens read on the device only
// (graph-capturable: ctx changes under replay and kkeep is recomputed here):
//
//  1. attn_sparse_scores_kernel  streams K once. Same S^T MFMA form and K/Q
//     fragment loads as attn_decode_mfma.hip (A = K rows, B = the <= 16 heads
//     of one (b, kv head) chunk, f32 accumulate); the f32 scores go to the
//     workspace ws (B, Hq, maxp*P).
//  2. attn_sparse_select_kernel  one workgroup per (b, h): radix select
//     (8-bit digits, LDS histogram) of the kkeep-th largest score on the
//     order-preserving integer image of the f32 scores, position-ordered
//     running count for ties at the threshold, then ws is overwritten in
//     place with p[c] = exp(s[c] - max) for kept positions and 0 otherwise
//     (zero-filled to the page boundary), and l = sum p is written.
//  3. attn_sparse_pv_kernel      walks the 32-position tiles of (b, kv head),
//     split across workgroups; O^T = V^T P^T on the MFMA with P rounded to
//     bf16 (as the dense decode kernel does), f32 accumulate. Every split
//     shares the global max, so partials simply add.
//  4. attn_sparse_combine_kernel sums the split partials, divides by l,
//     writes bf16.
//
// What the V layout allows. V pages are d-major (np, Hkv, D, P) with P = 16:
// one position's V row is D separate 2-byte elements, each inside a different
// 32-byte segment, so fetching ONE position costs the same bytes as fetching
// the whole page tile of that head. The V-traffic saving on the device is
// therefore at PAGE granularity: a page's V loads are skipped only when none
// of the chunk's heads kept any of its 16 positions. That share is near zero
// for scattered selections and real for clustered ones (attention sinks plus
// recent tokens). K is always streamed in full.
//
// Workspace. ws is sized by the page-table WIDTH (maxp * P slots per query
// head), not by the live context, because the host never reads ctx_lens:
// B * Hq * maxp * P * 4 bytes per call, from torch's caching allocator
// (8 MB at B32 Hq32 with a 2048-token table, 512 MB with a 128k-token one).
// Only the first ctx slots of a row are ever touched.

#include "common.h"

static constexpr int SP_P = 16;       // page size this path is written for
static constexpr int SP_TILE = 32;    // positions per MFMA k-slice of P.V
static constexpr int SP_HC = 16;      // heads per chunk (MFMA column count)

// ---------------------------------------------------------------------------
// 1. scores
// grid = (B*Hkv*nch, ceil(N/128)), block 256: wave w owns 32 positions.
template <int D>
__global__ __launch_bounds__(256) void attn_sparse_scores_kernel(
    const unsigned short* __restrict__ q,        // strided, see q_sb/q_sh
    const unsigned short* __restrict__ k_pages,  // (np, Hkv, P, D)
    const int* __restrict__ page_table,          // (B, maxp)
    const int* __restrict__ ctx_lens,            // (B,)
    const float* __restrict__ alibi,             // (Hq,) slopes or null
    float* __restrict__ ws,                      // (B, Hq, N)
    int Hkv, int G, int nch, int maxp, int N, float scale, long q_sb,
    long q_sh) {
  constexpr int NKK = D / 32;
  const int bh = blockIdx.x;
  const int b = bh / (Hkv * nch);
  const int rem = bh % (Hkv * nch);
  const int kvh = rem / nch;
  const int g0 = (rem % nch) * SP_HC;
  const int Gl = min(G - g0, SP_HC);
  const int ctx = min(max(ctx_lens[b], 0), N);

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int li = lane & 15;
  const int hi = lane >> 4;
  const int base = blockIdx.y * 128 + wave * 32;
  if (base >= ctx) return;  // wave-uniform; the kernel has no barrier

  // Q fragments: B[k=d][col=head]; cols >= Gl repeat the last head, unused
  const int qh = g0 + ((li < Gl) ? li : Gl - 1);
  bf16x8 qfrag[NKK];
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk)
    qfrag[kk] = as_bf16x8(*reinterpret_cast<const short8*>(
        q + (long)b * q_sb + (long)(kvh * G + qh) * q_sh + hi * 8 + 32 * kk));
  const int head = kvh * G + g0 + li;
  const bool live = li < Gl;
  const float slope = (alibi != nullptr && live) ? alibi[head] : 0.f;

  // K fragments: A[row=pos][k=d]; rows past ctx re-read the last live row
  bf16x8 kb[2][NKK];
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int cpos = min(base + 16 * n + li, ctx - 1);
    const int page = page_table[b * maxp + cpos / SP_P];
    const unsigned short* krow =
        k_pages + (((long)page * Hkv + kvh) * SP_P + (cpos % SP_P)) * D;
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk)
      kb[n][kk] = as_bf16x8(__builtin_nontemporal_load(
          reinterpret_cast<const short8*>(krow + hi * 8 + 32 * kk)));
  }
  float* srow = ws + ((long)b * (Hkv * G) + head) * N;
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    f32x4 st = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk)
      st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kb[n][kk], qfrag[kk], st, 0,
                                                   0, 0);
    // C rows = positions hi*4 + reg, cols = head li
    const int p0 = base + 16 * n + hi * 4;
    f32x4 sv;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
      // two roundings, as the reference: (dot * scale) + (slope * c)
      sv[reg] = __fadd_rn(__fmul_rn(st[reg], scale),
                          __fmul_rn(slope, (float)(p0 + reg)));
    if (!live) continue;
    if (p0 + 3 < ctx) {
      *reinterpret_cast<f32x4*>(srow + p0) = sv;
    } else {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        if (p0 + reg < ctx) srow[p0 + reg] = sv[reg];
    }
  }
}

// ---------------------------------------------------------------------------
// 2. select
// Order-preserving image of an f32: larger float <=> larger unsigned key.
// -0 is folded onto +0 so the two compare equal, as they do as floats.
DEVINL unsigned int sparse_key(float f) {
  unsigned int u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// grid = B*Hq, block 256.
__global__ __launch_bounds__(256) void attn_sparse_select_kernel(
    float* __restrict__ ws,              // (B, Hq, N): scores in, p out
    float* __restrict__ lsum,            // (B, Hq)
    const int* __restrict__ ctx_lens, int Hq, int N, double sparsity) {
  __shared__ unsigned int hist[256];
  __shared__ unsigned int scan[256];
  __shared__ unsigned int sh_digit, sh_krem;
  __shared__ float red[4];
  __shared__ unsigned int wcnt[4];

  const int row = blockIdx.x;
  const int b = row / Hq;
  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int ctx = min(max(ctx_lens[b], 0), N);
  float* s = ws + (long)row * N;
  if (ctx == 0) {  // block-uniform
    if (tid == 0) lsum[row] = 0.f;
    return;
  }
  // kkeep on the device, product in double exactly as the reference
  double kd = ceil(sparsity * (double)ctx);
  kd = fmin(fmax(kd, 1.0), (double)ctx);
  unsigned int krem = (unsigned int)kd;

  // row maximum
  float mx = -INFINITY;
  for (int c = tid; c < ctx; c += 256) mx = fmaxf(mx, s[c]);
  mx = wave_reduce_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  const float m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));

  // radix select of the krem-th largest key, most significant digit first
  unsigned int prefix = 0u, mask = 0u;
#pragma unroll 1
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0u;
    __syncthreads();
    for (int c = tid; c < ctx; c += 256) {
      const unsigned int key = sparse_key(s[c]);
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    // inclusive suffix sum: scan[t] = count of digits >= t
    const unsigned int mine = hist[tid];
    scan[tid] = mine;
    __syncthreads();
#pragma unroll 1
    for (int off = 1; off < 256; off <<= 1) {
      const unsigned int v =
          scan[tid] + ((tid + off < 256) ? scan[tid + off] : 0u);
      __syncthreads();
      scan[tid] = v;
      __syncthreads();
    }
    const unsigned int incl = scan[tid];
    const unsigned int above = incl - mine;
    if (above < krem && krem <= incl) {  // exactly one digit qualifies
      sh_digit = (unsigned int)tid;
      sh_krem = krem - above;
    }
    __syncthreads();
    prefix |= sh_digit << shift;
    mask |= 255u << shift;
    krem = sh_krem;
  }
  // prefix = threshold key; every key above it is kept, and of the keys equal
  // to it the krem lowest positions

  const int ctx_pg = (ctx + SP_P - 1) / SP_P * SP_P;  // <= N
  unsigned int run = 0u;
  float lacc = 0.f;
#pragma unroll 1
  for (int c0 = 0; c0 < ctx_pg; c0 += 256) {
    const int c = c0 + tid;
    const bool valid = c < ctx;
    const float sv = valid ? s[c] : 0.f;
    const unsigned int key = valid ? sparse_key(sv) : 0u;
    const bool eq = valid && key == prefix;
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(eq);
    if (lane == 0) wcnt[wave] = (unsigned int)__popcll(bal);
    __syncthreads();
    unsigned int before = run + (unsigned int)__popcll(bal & ((1ull << lane) - 1ull));
    unsigned int total = 0u;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const unsigned int n = wcnt[w];
      if (w < wave) before += n;
      total += n;
    }
    run += total;
    const bool keep = valid && (key > prefix || (eq && before < krem));
    const float p = keep ? expf(sv - m) : 0.f;
    if (c < ctx_pg) s[c] = p;
    lacc += p;
    __syncthreads();  // wcnt is rewritten next round
  }
  lacc = wave_reduce_sum(lacc);
  if (lane == 0) red[wave] = lacc;
  __syncthreads();
  if (tid == 0) lsum[row] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------------------
// 3. P.V
// grid = (B*Hkv*nch, n_split), block 256. A split owns a contiguous run of
// 32-position tiles; wave w takes tile pairs w, w+4, ... of it. A tile is two
// pages: lanes hi 0,1 feed the first, hi 2,3 the second, and a page whose
// weights are all zero over the chunk's heads issues no V load.
template <int D>
__global__ __launch_bounds__(256) void attn_sparse_pv_kernel(
    const float* __restrict__ ws,                // (B, Hq, N): p
    const unsigned short* __restrict__ v_pages,  // (np, Hkv, D, P) d-major
    const int* __restrict__ page_table, const int* __restrict__ ctx_lens,
    float* __restrict__ pacc,                    // (B*Hkv*nch*n_split, 16, D)
    int Hkv, int G, int nch, int maxp, int N, int n_split) {
  constexpr int NDT = D / 16;
  constexpr int PITCH = D + 4;
  __shared__ __attribute__((aligned(16))) float merge[SP_HC * PITCH];

  const int bh = blockIdx.x;
  const int split = blockIdx.y;
  const int b = bh / (Hkv * nch);
  const int rem = bh % (Hkv * nch);
  const int kvh = rem / nch;
  const int g0 = (rem % nch) * SP_HC;
  const int Gl = min(G - g0, SP_HC);
  const int ctx = min(max(ctx_lens[b], 0), N);
  const int ctx_pg = (ctx + SP_P - 1) / SP_P * SP_P;

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int li = lane & 15;
  const int hi = lane >> 4;
  const bool live = li < Gl;

  const int tiles_total = (ctx + SP_TILE - 1) / SP_TILE;
  const int tps = (tiles_total + n_split - 1) / n_split;
  const int t0 = split * tps;
  const int t1 = min(tiles_total, t0 + tps);

  const float* prow =
      ws + ((long)b * (Hkv * G) + kvh * G + g0 + (live ? li : 0)) * N;

  f32x4 acc_o[NDT];  // O^T: rows = d (16n + hi*4 + reg), cols = head li
#pragma unroll
  for (int n = 0; n < NDT; ++n) acc_o[n] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int t = t0 + wave * 2; t < t1; t += 8) {
    bf16x8 pfrag[2];
    bool need[2];
    unsigned long long any[2];
    // ---- P^T fragments: B[k=pos][col=head], 8 consecutive positions of
    // head li, read as f32 from the workspace and rounded to bf16
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int pos0 = (t + u) * SP_TILE + hi * 8;
      f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f}, c = a;
      if (live && (t + u) < t1 && pos0 < ctx_pg) {
        a = *reinterpret_cast<const f32x4*>(prow + pos0);
        c = *reinterpret_cast<const f32x4*>(prow + pos0 + 4);
      }
      short8 pk;
      bool nz = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pk[j] = (short)f2bf(a[j]);
        pk[4 + j] = (short)f2bf(c[j]);
        nz |= (a[j] != 0.f) | (c[j] != 0.f);
      }
      pfrag[u] = as_bf16x8(pk);
      const unsigned long long bal = __builtin_amdgcn_ballot_w64(nz);
      any[u] = bal;
      // lanes 0..31 (hi 0,1) hold the tile's first page, 32..63 its second
      need[u] = ((hi < 2) ? (bal & 0xffffffffull) : (bal >> 32)) != 0ull;
    }
    // ---- V^T fragments: A[row=d][k=pos], only for pages somebody kept
    bf16x8 vf[2][NDT];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int pos0 = (t + u) * SP_TILE + hi * 8;
#pragma unroll
      for (int n = 0; n < NDT; ++n) vf[u][n] = as_bf16x8(short8{});
      if (need[u]) {  // implies pos0 < ctx_pg: the page holds a kept position
        const int page = page_table[b * maxp + pos0 / SP_P];
        const long vrow = ((long)page * Hkv + kvh) * D;
#pragma unroll
        for (int n = 0; n < NDT; ++n) {
          short8 v = __builtin_nontemporal_load(reinterpret_cast<const short8*>(
              v_pages + (vrow + li + 16 * n) * SP_P + (pos0 % SP_P)));
          if (pos0 + 8 > ctx) {
            // slots past ctx were never written: keep them out of 0 * v
#pragma unroll
            for (int j = 0; j < 8; ++j)
              if (pos0 + j >= ctx) v[j] = 0;
          }
          vf[u][n] = as_bf16x8(v);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (any[u] == 0ull) continue;  // wave-uniform
#pragma unroll
      for (int n = 0; n < NDT; ++n)
        acc_o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[u][n], pfrag[u],
                                                           acc_o[n], 0, 0, 0);
    }
  }

  // ---- 4-wave merge in a fixed order (bit-reproducible), then the partial
#pragma unroll 1
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int n = 0; n < NDT; ++n) {
        f32x4* dst =
            reinterpret_cast<f32x4*>(merge + li * PITCH + 16 * n + hi * 4);
        *dst = (w == 0) ? acc_o[n] : (*dst + acc_o[n]);
      }
    }
    __syncthreads();
  }
  float* dstp = pacc + ((long)bh * n_split + split) * SP_HC * D;
  for (int idx = tid; idx < Gl * D; idx += 256) {
    const int g = idx / D, d = idx % D;
    dstp[g * D + d] = merge[g * PITCH + d];
  }
}

// ---------------------------------------------------------------------------
// 4. combine: out = (sum over splits) / l  ->  bf16. grid = B*Hkv*nch.
__global__ __launch_bounds__(256) void attn_sparse_combine_kernel(
    const float* __restrict__ pacc, const float* __restrict__ lsum,
    unsigned short* __restrict__ out, int Hkv, int G, int nch, int D,
    int n_split, long out_sb, long out_sh) {
  const int bh = blockIdx.x;
  const int b = bh / (Hkv * nch);
  const int rem = bh % (Hkv * nch);
  const int kvh = rem / nch;
  const int g0 = (rem % nch) * SP_HC;
  const int Gl = min(G - g0, SP_HC);
  for (int idx = threadIdx.x; idx < Gl * D; idx += 256) {
    const int g = idx / D, d = idx % D;
    float a = 0.f;
    for (int sp = 0; sp < n_split; ++sp)
      a += pacc[(((long)bh * n_split + sp) * SP_HC + g) * D + d];
    const int h = kvh * G + g0 + g;
    const float l = lsum[(long)b * (Hkv * G) + h];
    const float o = (l > 0.f) ? a / l : 0.f;
    out[(long)b * out_sb + (long)h * out_sh + d] = f2bf(o);
  }
}
