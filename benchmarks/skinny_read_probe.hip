// Standalone read probe for the decode GEMM's weight stream (hipcc, no torch).
// Two kernels that ONLY read a weight-sized region into a register checksum,
// at gemm_skinny_v2_kernel's grid (N/64 x ksplit, XCD remap), its 256-thread
// blocks and its two-set pipeline (two 4 KB register sets per wave, one
// outstanding at each wait):
//   R: row-major — a wave load is 16 rows x 64 B at a row stride of 2K bytes
//   P: packed    — a wave load is one contiguous 1 KB (common.h layout)
// It separates "request shape" from everything else in the GEMM (A staging,
// LDS, MFMA, epilogue). Launches cycle through >= 1 GiB of distinct copies so
// nothing is served from the 256 MiB Infinity Cache.
// Build: hipcc --offload-arch=gfx950 -O3 skinny_read_probe.hip -o skinny_read_probe
// Run:   ./skinny_read_probe            (the four Llama-3-8B decode shapes)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

typedef __attribute__((ext_vector_type(4))) unsigned int uint4v;

#define CHECK(e)                                                        \
  do {                                                                  \
    hipError_t _e = (e);                                                \
    if (_e != hipSuccess) {                                             \
      fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(_e));           \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

template <bool PACKED>
__global__ __launch_bounds__(256) void read_probe(
    const unsigned short* __restrict__ W, uint4v* __restrict__ out, int N,
    int K, int kchunk) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, hi = lane >> 4;
  int tile = blockIdx.x;
  {
    const int nwg = gridDim.x;
    const int xcd = tile % 8, orig8 = tile / 8;
    const int q = nwg / 8, r = nwg % 8;
    if (nwg >= 8)
      tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + orig8;
  }
  const int k0 = blockIdx.y * kchunk;
  const int k1 = min(K, k0 + kchunk);      // (k1 - k0) % 256 == 0 (host)
  const unsigned short* base =
      PACKED ? W + (long)(tile * 4 + wave) * K * 16 + lane * 8
             : W + (long)(tile * 64 + wave * 16 + li) * K + hi * 8;
  auto off = [&](int k, int u) -> long {
    return PACKED ? (long)(k / 32 + u) * 512 : (long)k + u * 32;
  };
  uint4v s0[4], s1[4], acc = {0u, 0u, 0u, 0u};
  auto issue = [&](uint4v* s, int k) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      s[u] = *reinterpret_cast<const uint4v*>(base + off(k, u));
  };
  auto eat = [&](const uint4v* s) {
#pragma unroll
    for (int u = 0; u < 4; ++u) acc ^= s[u];
  };
  issue(s0, k0);
  for (int k = k0; k < k1; k += 256) {
    issue(s1, k + 128);
    eat(s0);
    if (k + 256 < k1) issue(s0, k + 256);
    eat(s1);
  }
  out[((long)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x] = acc;
}

int main() {
  struct Shape { const char* name; int N, K, ksplit; };
  // skinny_plan's splits for the Llama-3-8B projections
  const Shape shapes[] = {{"qkv     6144x4096  ks8", 6144, 4096, 8},
                          {"o       4096x4096  ks8", 4096, 4096, 8},
                          {"gate_up 28672x4096 ks1", 28672, 4096, 1},
                          {"down    4096x14336 ks8", 4096, 14336, 8}};
  const size_t region = (size_t)1 << 30;
  unsigned short* W;
  uint4v* out;
  CHECK(hipMalloc(&W, region + (256u << 20)));
  CHECK(hipMemset(W, 0x3c, region + (256u << 20)));
  CHECK(hipMalloc(&out, (size_t)8192 * 256 * sizeof(uint4v)));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  for (const Shape& s : shapes) {
    const size_t bytes = (size_t)s.N * s.K * 2;
    const int ncopies = (int)((region + bytes - 1) / bytes);  // <= region+256M
    const int nch = s.K / 256, per = (nch + s.ksplit - 1) / s.ksplit;
    const int ks = (nch + per - 1) / per, kchunk = per * 256;
    const dim3 grid(s.N / 64, ks);
    if ((size_t)ncopies * bytes > region + (256u << 20) ||
        (size_t)grid.x * grid.y > 8192) {
      fprintf(stderr, "%s: does not fit the probe's buffers\n", s.name);
      return 1;
    }
    for (int packed = 0; packed < 2; ++packed) {
      float best = 1e30f, sum = 0.f;
      const int reps = 5, iters = 2 * ncopies;
      for (int r = 0; r < reps + 1; ++r) {     // first repetition warms up
        CHECK(hipEventRecord(e0));
        for (int i = 0; i < iters; ++i) {
          const unsigned short* w = W + (size_t)(i % ncopies) * (bytes / 2);
          if (packed)
            read_probe<true><<<grid, 256>>>(w, out, s.N, s.K, kchunk);
          else
            read_probe<false><<<grid, 256>>>(w, out, s.N, s.K, kchunk);
        }
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipGetLastError());
        float ms;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (r == 0) continue;
        const float us = ms * 1e3f / iters;
        best = us < best ? us : best;
        sum += us;
      }
      printf("%s  %s  mean %7.2f us  best %7.2f us  %5.2f TB/s (mean)\n",
             s.name, packed ? "P packed   " : "R row-major", sum / reps, best,
             bytes / (sum / reps * 1e-6) / 1e12);
    }
  }
  return 0;
}
