// Launchers of the fp8 (e4m3) KV-cache kernels (kv_fp8.hip, a translation
// unit of its own). Raw device pointers only: every pointer has been through
// Operands::ptr in ext.hip, which also checks the geometry these assume —
// page size 16, head dim 64 or 128, 16 B aligned pools.
#pragma once

#include <hip/hip_runtime.h>

struct Fp8Pool {
  unsigned char* k;  // e4m3 (np, Hkv, 16, D) token-major
  unsigned char* v;  // e4m3 (np, Hkv, D, 16) d-major
  const int* pt;     // (B, maxp)
  int Hkv, P, D, maxp;
};

// maxg: 4 or 16 head columns per workgroup, as for the bf16 kernel; the
// partials have that many rows per (b, kv head, chunk, split).
void launch_attn_decode_fp8(
    hipStream_t stream, const unsigned short* q, const Fp8Pool& kv,
    const int* ctx_lens, const float* alibi, unsigned short* out,
    float* part_ml, float* part_acc, int B, int G, int nch, int maxg,
    int n_split, int window, float scale, long q_sb, long q_sh, long out_sb,
    long out_sh);

void launch_attn_prefill_fp8(
    hipStream_t stream, const unsigned short* q, const Fp8Pool& kv,
    const int* q_start, const float* alibi, const unsigned char* tree_mask,
    unsigned short* out, int B, int Hq, int Tq, int window, float scale,
    long q_sb, long q_st, long q_sh, long out_sb, long out_st, long out_sh);

// k_new / v_new: bf16 (B, Hkv, T, D) contiguous
void launch_kv_write_fp8(hipStream_t stream, const unsigned short* k_new,
                         const unsigned short* v_new, const Fp8Pool& kv,
                         const int* start_pos, int B, int T);

// qkv: bf16 (B, T, (Hq+2Hkv)*D); pos: (B, T) or null
void launch_rope_kv_write_fp8(hipStream_t stream, unsigned short* qkv,
                              const float* cos_t, const float* sin_t,
                              const int* pos, const Fp8Pool& kv,
                              const int* start_pos, int B, int Hq, int T,
                              int max_pos);
