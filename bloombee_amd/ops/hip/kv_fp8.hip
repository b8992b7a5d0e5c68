// fp8 (OCP e4m3) KV cache for gfx950: the writers that fill an fp8 pool and
// the launchers of every kernel that reads one (kv_fp8.h). No scale factors:
// a stored element is e4m3_rne(clamp(x, -448, 448)), a page stays a plain
// tensor, and swap / reorder / truncate remain byte moves.
//
// Layouts as for bf16: K pages (np, Hkv, P, D) token-major, V pages
// (np, Hkv, D, P) d-major, one byte per element.

#include "kv_fp8.h"

#include "attn_decode_fp8.hip"
#include "attn_prefill.hip"

// ---------------------------------------------------------------------------
// kv_write over an fp8 pool: bf16 (B, Hkv, T, D) -> clamp, e4m3. One block per
// (b, t); a lane converts 8 consecutive d: one 8 B store into the K row, 8
// scattered 1 B stores down the V column (transpose on write, once per token).
// ---------------------------------------------------------------------------
__global__ void kv_write_fp8_kernel(
    const unsigned short* __restrict__ k_new,
    const unsigned short* __restrict__ v_new,
    unsigned char* __restrict__ k_pages, unsigned char* __restrict__ v_pages,
    const int* __restrict__ page_table, const int* __restrict__ start_pos,
    int Hkv, int T, int D, int P, int maxp) {
  const int bt = blockIdx.x;
  const int b = bt / T, t = bt % T;
  const int pos = start_pos[b] + t;
  const int page = page_table[b * maxp + pos / P];
  const int slot = pos % P;
  const int nvec = Hkv * (D / 8);
  for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
    const int h = i / (D / 8);
    const int d = (i % (D / 8)) * 8;
    const long src = (((long)b * Hkv + h) * T + t) * D + d;
    float kf[8], vf[8];
    load_bf16x8(k_new + src, kf);
    load_bf16x8(v_new + src, vf);
    int2v k8;
    k8[0] = f2fp8x4(kf[0], kf[1], kf[2], kf[3]);
    k8[1] = f2fp8x4(kf[4], kf[5], kf[6], kf[7]);
    const long kdst = (((long)page * Hkv + h) * P + slot) * D + d;
    *reinterpret_cast<int2v*>(k_pages + kdst) = k8;
    const long vbase = (((long)page * Hkv + h) * D + d) * P + slot;
#pragma unroll
    for (int j = 0; j < 8; ++j) v_pages[vbase + (long)j * P] = f2fp8(vf[j]);
  }
}

// ---------------------------------------------------------------------------
// rope_kv_write_ over an fp8 pool, on the raw QKV GEMM output
// (B, T, (Hq+2Hkv)*D) bf16. q heads: rotary in place, the arithmetic of
// rope_kv_write_kernel (elementwise.hip) to the bit. k heads: rotary in f32,
// rounded ONCE to e4m3 (not via bf16) -> k_pages. v heads: clamp, e4m3 ->
// v_pages. grid: (B*T, Hq+2Hkv), block: 64.
// ---------------------------------------------------------------------------
__global__ void rope_kv_write_fp8_kernel(
    unsigned short* __restrict__ qkv, const float* __restrict__ cos_t,
    const float* __restrict__ sin_t, const int* __restrict__ pos,
    unsigned char* __restrict__ k_pages, unsigned char* __restrict__ v_pages,
    const int* __restrict__ page_table, const int* __restrict__ start_pos,
    int Hq, int Hkv, int T, int D, int P, int maxp, int max_pos) {
  const int bt = blockIdx.x;
  const int b = bt / T, t = bt % T;
  const int h = blockIdx.y;
  const int X = Hq + 2 * Hkv;
  unsigned short* base = qkv + (((long)b * T + t) * X + h) * D;

  const int abspos = start_pos[b] + t;
  const int page = page_table[b * maxp + abspos / P];
  const int slot = abspos % P;
  if (h >= Hq + Hkv) {
    const int hv = h - Hq - Hkv;
    unsigned char* dst = v_pages + ((long)page * Hkv + hv) * D * P + slot;
    for (int i = threadIdx.x; i < D; i += blockDim.x)
      dst[(long)i * P] = f2fp8(bf2f(base[i]));
    return;
  }
  const int p = min(max(pos ? pos[b * T + t] : abspos, 0), max_pos - 1);
  const float* c = cos_t + (long)p * (D / 2);
  const float* s = sin_t + (long)p * (D / 2);
  const int hk = max(h - Hq, 0);  // a q head never stores through kdst
  unsigned char* kdst = k_pages + (((long)page * Hkv + hk) * P + slot) * D;
  for (int i = threadIdx.x; i < D / 2; i += blockDim.x) {
    // two products, then the sum, each rounded: what the bf16 kernel does
#pragma clang fp contract(off)
    float x1 = bf2f(base[i]), x2 = bf2f(base[i + D / 2]);
    float cc = c[i], ss = s[i];
    const float r1 = x1 * cc - x2 * ss, r2 = x2 * cc + x1 * ss;
    if (h >= Hq) {
      kdst[i] = f2fp8(r1);
      kdst[i + D / 2] = f2fp8(r2);
    } else {
      base[i] = f2bf(r1);
      base[i + D / 2] = f2bf(r2);
    }
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

void launch_attn_decode_fp8(
    hipStream_t stream, const unsigned short* q, const Fp8Pool& kv,
    const int* ctx_lens, const float* alibi, unsigned short* out,
    float* part_ml, float* part_acc, int B, int G, int nch, int maxg,
    int n_split, int window, float scale, long q_sb, long q_sh, long out_sb,
    long out_sh) {
  const dim3 grid(B * kv.Hkv * nch, n_split);
  auto launch = [&](auto kernel) {
    kernel<<<grid, 256, 0, stream>>>(
        q, kv.k, kv.v, kv.pt, ctx_lens, alibi, out, part_ml, part_acc, B,
        kv.Hkv, G, nch, kv.maxp, n_split, window, scale, q_sb, q_sh, out_sb,
        out_sh);
  };
  if (kv.D == 128) {
    if (maxg == 4) launch(&attn_decode_fp8_kernel<128, 4>);
    else launch(&attn_decode_fp8_kernel<128, 16>);
  } else {
    if (maxg == 4) launch(&attn_decode_fp8_kernel<64, 4>);
    else launch(&attn_decode_fp8_kernel<64, 16>);
  }
}

void launch_attn_prefill_fp8(
    hipStream_t stream, const unsigned short* q, const Fp8Pool& kv,
    const int* q_start, const float* alibi, const unsigned char* tree_mask,
    unsigned short* out, int B, int Hq, int Tq, int window, float scale,
    long q_sb, long q_st, long q_sh, long out_sb, long out_st, long out_sh) {
  const dim3 grid((Tq + 127) / 128, B * Hq);
  auto launch = [&](auto kernel) {
    kernel<<<grid, 512, 0, stream>>>(
        q, kv.k, kv.v, kv.pt, q_start, alibi, tree_mask, out, B, Hq,
        Hq / kv.Hkv, Tq, kv.P, kv.maxp, window, scale, q_sb, q_st, q_sh,
        out_sb, out_st, out_sh);
  };
  if (kv.D == 128) launch(&attn_prefill_kernel<128, unsigned char>);
  else launch(&attn_prefill_kernel<64, unsigned char>);
}

void launch_kv_write_fp8(hipStream_t stream, const unsigned short* k_new,
                         const unsigned short* v_new, const Fp8Pool& kv,
                         const int* start_pos, int B, int T) {
  const int threads = kv.Hkv * kv.D / 8 < 256 ? kv.Hkv * kv.D / 8 : 256;
  kv_write_fp8_kernel<<<B * T, threads, 0, stream>>>(
      k_new, v_new, kv.k, kv.v, kv.pt, start_pos, kv.Hkv, T, kv.D, kv.P,
      kv.maxp);
}

void launch_rope_kv_write_fp8(hipStream_t stream, unsigned short* qkv,
                              const float* cos_t, const float* sin_t,
                              const int* pos, const Fp8Pool& kv,
                              const int* start_pos, int B, int Hq, int T,
                              int max_pos) {
  const dim3 grid(B * T, Hq + 2 * kv.Hkv);
  rope_kv_write_fp8_kernel<<<grid, 64, 0, stream>>>(
      qkv, cos_t, sin_t, pos, kv.k, kv.v, kv.pt, start_pos, Hq, kv.Hkv, T,
      kv.D, kv.P, kv.maxp, max_pos);
}
