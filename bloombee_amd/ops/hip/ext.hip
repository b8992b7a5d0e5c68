// Torch extension bindings for the bloombee_amd gfx950 kernel library.
// Host-side shape checks, template dispatch, and stream plumbing only —
// all compute lives in the .hip translation units.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>
#include <cstdlib>

#include "common.h"

// Single translation unit: the template kernels must be visible at their
// launch sites for instantiation.
#include "elementwise.hip"
#include "kvcache.hip"
#include "attn_decode.hip"
#include "attn_decode_mfma.hip"
#include "attn_sparse.hip"
#include "attn_prefill.hip"
#include "attn_train.hip"
#include "gemm_skinny.hip"
#include "moe_gemm.hip"
#include "w4_gemm.hip"
#include "moe_gemm_w4.hip"
#include "mfma_selftest.hip"
#include "quant4.hip"
#include "wire.h"

typedef __attribute__((ext_vector_type(8))) short short8_h;

#define CHECK_DEV(x) TORCH_CHECK(x.is_cuda(), #x " must be on device")
// a CPU tensor pointer reaching a kernel is a GPU memory fault at a random
// later point — check EVERY tensor argument, not just the big ones
#define CHECK_DEV_ALL1(a) CHECK_DEV(a)
#define CHECK_DEV_ALL2(a, b) { CHECK_DEV(a); CHECK_DEV(b); }
#define CHECK_DEV_ALL3(a, b, c) { CHECK_DEV(a); CHECK_DEV(b); CHECK_DEV(c); }
#define CHECK_BF16(x) TORCH_CHECK(x.scalar_type() == at::kBFloat16, #x " must be bf16")
#define CHECK_CONTIG(x) TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")

static inline const unsigned short* bf_ptr(const torch::Tensor& t) {
  return reinterpret_cast<const unsigned short*>(t.data_ptr());
}
static inline unsigned short* bf_ptr_mut(torch::Tensor& t) {
  return reinterpret_cast<unsigned short*>(t.data_ptr());
}
static inline hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// ---------------------------------------------------------------------------
// norms
// ---------------------------------------------------------------------------

template <typename F>
static void dispatch_iters(int H, F f) {
  constexpr int BLOCK = 256;
  const int per_iter = BLOCK * 8;
  if (H <= per_iter) f(std::integral_constant<int, 1>{});
  else if (H <= 2 * per_iter) f(std::integral_constant<int, 2>{});
  else if (H <= 4 * per_iter) f(std::integral_constant<int, 4>{});
  else if (H <= 8 * per_iter) f(std::integral_constant<int, 8>{});
  else TORCH_CHECK(false, "hidden size too large for norm kernel: ", H);
}

torch::Tensor rms_norm(torch::Tensor x, torch::Tensor w, double eps) {
  CHECK_DEV(x); CHECK_BF16(x); CHECK_CONTIG(x);
  const int H = x.size(-1);
  TORCH_CHECK(H % 8 == 0, "H must be a multiple of 8");
  const long N = x.numel() / H;
  auto y = torch::empty_like(x);
  dispatch_iters(H, [&](auto iters) {
    rmsnorm_kernel<256, decltype(iters)::value><<<N, 256, 0, cur_stream()>>>(
        bf_ptr(x), nullptr, bf_ptr(w), nullptr, bf_ptr_mut(y), H, (float)eps);
  });
  return y;
}

std::vector<torch::Tensor> rms_norm_residual(torch::Tensor x, torch::Tensor res,
                                             torch::Tensor w, double eps) {
  CHECK_DEV(x); CHECK_BF16(x); CHECK_CONTIG(x); CHECK_CONTIG(res);
  const int H = x.size(-1);
  const long N = x.numel() / H;
  auto h = torch::empty_like(x);
  auto y = torch::empty_like(x);
  dispatch_iters(H, [&](auto iters) {
    rmsnorm_kernel<256, decltype(iters)::value><<<N, 256, 0, cur_stream()>>>(
        bf_ptr(x), bf_ptr(res), bf_ptr(w), bf_ptr_mut(h), bf_ptr_mut(y), H,
        (float)eps);
  });
  return {h, y};
}

torch::Tensor layer_norm(torch::Tensor x, torch::Tensor w,
                         c10::optional<torch::Tensor> bias, double eps) {
  CHECK_DEV(x); CHECK_BF16(x); CHECK_CONTIG(x);
  const int H = x.size(-1);
  const long N = x.numel() / H;
  auto y = torch::empty_like(x);
  const unsigned short* bp = bias.has_value() ? bf_ptr(*bias) : nullptr;
  dispatch_iters(H, [&](auto iters) {
    layernorm_kernel<256, decltype(iters)::value><<<N, 256, 0, cur_stream()>>>(
        bf_ptr(x), nullptr, bf_ptr(w), bp, nullptr, bf_ptr_mut(y), H, (float)eps);
  });
  return y;
}

// ---------------------------------------------------------------------------
// rope / activations
// ---------------------------------------------------------------------------

void rope_apply_(torch::Tensor q, torch::Tensor k, torch::Tensor cos_t,
                 torch::Tensor sin_t, torch::Tensor pos) {
  CHECK_DEV(q); CHECK_BF16(q); CHECK_CONTIG(q); CHECK_CONTIG(k);
  CHECK_DEV_ALL3(cos_t, sin_t, pos);
  TORCH_CHECK(pos.scalar_type() == at::kInt, "pos must be int32");
  const int B = q.size(0), Hq = q.size(1), T = q.size(2), D = q.size(3);
  const int Hkv = k.size(1);
  TORCH_CHECK(cos_t.scalar_type() == at::kFloat && cos_t.size(1) == D / 2);
  dim3 grid(B * T, Hq + Hkv);
  rope_kernel<<<grid, 64, 0, cur_stream()>>>(
      bf_ptr_mut(q), bf_ptr_mut(k), cos_t.data_ptr<float>(),
      sin_t.data_ptr<float>(), pos.data_ptr<int>(), B, Hq, Hkv, T, D,
      (int)cos_t.size(0));
}

torch::Tensor swiglu(torch::Tensor gu) {
  CHECK_DEV(gu); CHECK_BF16(gu); CHECK_CONTIG(gu);
  const long I = gu.size(-1) / 2;
  const long N = gu.numel() / (2 * I);
  TORCH_CHECK(I % 8 == 0);
  auto sizes = gu.sizes().vec();
  sizes.back() = I;
  auto out = torch::empty(sizes, gu.options());
  const long nvec = N * (I / 8);
  const int grid = (int)std::min<long>((nvec + 255) / 256, 2048);
  swiglu_kernel<<<grid, 256, 0, cur_stream()>>>(bf_ptr(gu), bf_ptr_mut(out), N, I);
  return out;
}

torch::Tensor gelu_tanh(torch::Tensor x) {
  CHECK_DEV(x); CHECK_BF16(x); CHECK_CONTIG(x);
  auto out = torch::empty_like(x);
  const long nvec = x.numel() / 8;
  // >= 1 block so the scalar tail (numel % 8) runs when numel < 8
  const int grid = (int)std::max<long>(1, std::min<long>((nvec + 255) / 256, 2048));
  gelu_kernel<<<grid, 256, 0, cur_stream()>>>(bf_ptr(x), bf_ptr_mut(out), x.numel());
  return out;
}

torch::Tensor add_bf16(torch::Tensor a, torch::Tensor b) {
  CHECK_DEV(a); CHECK_BF16(a); CHECK_CONTIG(a); CHECK_CONTIG(b);
  CHECK_DEV(b); CHECK_BF16(b);
  TORCH_CHECK(b.numel() == a.numel(), "add_bf16: numel mismatch");
  auto out = torch::empty_like(a);
  const long nvec = a.numel() / 8;
  const int grid = (int)std::max<long>(1, std::min<long>((nvec + 255) / 256, 2048));
  add_kernel<<<grid, 256, 0, cur_stream()>>>(bf_ptr(a), bf_ptr(b), bf_ptr_mut(out),
                                             a.numel());
  return out;
}

// ---------------------------------------------------------------------------
// paged KV
// ---------------------------------------------------------------------------

void kv_write(torch::Tensor k_new, torch::Tensor v_new, torch::Tensor k_pages,
              torch::Tensor v_pages, torch::Tensor page_table,
              torch::Tensor start_pos) {
  CHECK_DEV(k_new); CHECK_BF16(k_new); CHECK_CONTIG(k_new); CHECK_CONTIG(v_new);
  CHECK_CONTIG(k_pages); CHECK_CONTIG(v_pages);
  TORCH_CHECK(page_table.scalar_type() == at::kInt && start_pos.scalar_type() == at::kInt);
  CHECK_DEV_ALL2(page_table, start_pos);
  const int B = k_new.size(0), Hkv = k_new.size(1), T = k_new.size(2), D = k_new.size(3);
  const int P = k_pages.size(2), maxp = page_table.size(1);
  TORCH_CHECK(k_pages.size(1) == Hkv && k_pages.size(3) == D);
  TORCH_CHECK(v_pages.size(2) == D && v_pages.size(3) == P,
              "v_pages must be d-major (np, Hkv, D, P)");
  const int threads = std::min(256, Hkv * D / 8);
  kv_write_kernel<<<B * T, threads, 0, cur_stream()>>>(
      bf_ptr(k_new), bf_ptr(v_new), bf_ptr_mut(k_pages), bf_ptr_mut(v_pages),
      page_table.data_ptr<int>(), start_pos.data_ptr<int>(), B, Hkv, T, D, P, maxp);
}

std::vector<torch::Tensor> kv_gather(torch::Tensor k_pages, torch::Tensor v_pages,
                                     torch::Tensor page_table, long batch_index,
                                     long ctx) {
  CHECK_DEV(k_pages); CHECK_DEV(page_table);
  const int Hkv = k_pages.size(1), P = k_pages.size(2), D = k_pages.size(3);
  auto k = torch::empty({Hkv, ctx, D}, k_pages.options());
  auto v = torch::empty({Hkv, ctx, D}, v_pages.options());
  const long nvec = ctx * Hkv * (D / 8);
  const int grid = (int)std::min<long>((nvec + 255) / 256, 2048);
  kv_gather_kernel<<<grid, 256, 0, cur_stream()>>>(
      bf_ptr(k_pages), bf_ptr(v_pages), bf_ptr_mut(k), bf_ptr_mut(v),
      page_table.data_ptr<int>(), (int)batch_index, (int)ctx, Hkv, D, P,
      page_table.size(1));
  return {k, v};
}

// ---------------------------------------------------------------------------
// attention
// ---------------------------------------------------------------------------

// External (host-segment) partial for mixed-device decode; contract in
// attn_decode.hip (attn_decode_merge_ext_kernel).
struct MixedExt {
  const float* ml;         // (B, Hq, 2)
  const float* acc;        // (B, Hq, D)
  const float* dev_shift;  // (Hq,) or null
};

template <int D>
static void attn_decode_launch(const torch::Tensor& q, const torch::Tensor& kp,
                               const torch::Tensor& vp, const torch::Tensor& pt,
                               const torch::Tensor& ctx,
                               const float* alibi_ptr, torch::Tensor& out,
                               torch::Tensor& pml, torch::Tensor& pacc, int B,
                               int Hkv, int G, int nch, int P, int maxp,
                               int n_split, int window, float scale, long q_off,
                               long q_sb, long q_sh, long out_sb, long out_sh,
                               const MixedExt* ext = nullptr) {
  dim3 grid(B * Hkv * nch, n_split);
  // mixed-device decode: the kernels emit partials even at n_split == 1 and
  // the merge kernel folds in the host segment's partial
  const int fp = ext != nullptr ? 1 : 0;
  const int maxg = (G <= 4 && nch == 1) ? 4 : 16;
  // paired-tile variant (NT=2): 2x KV bytes in flight per wave — the
  // latency-bound fix (profiles/r01_st_attention.md SQ_WAIT diagnosis).
  // BBAMD_ATTN_NT=1 reverts; D>=256 keeps NT=1 (VGPR budget).
  static const int nt_env = [] {
    const char* e = std::getenv("BBAMD_ATTN_NT");
    return e ? std::atoi(e) : 2;
  }();
  // Software-pipelined variant (next tile's K+V double-buffered in
  // registers; r02 WAIT_ANY diagnosis): DEFAULT — 50 us / 5.4 TB/s at B32
  // ctx2048 and 6.3 TB/s (achievable-HBM ceiling) at ctx8192 vs 59-62 us
  // for the NT variants. BBAMD_ATTN_PF=0 reverts to the NT path.
  static const bool pf_env = [] {
    const char* e = std::getenv("BBAMD_ATTN_PF");
    return !e || std::atoi(e) != 0;
  }();
  const bool pf = pf_env && (D <= 128);
  const bool nt2 = (nt_env >= 2) && (D <= 128) && !pf;
  auto launch_mfma = [&](auto mg) {
    if constexpr (D == 512) {
      // wide-head path: d split across the 4 waves (gemma-4 global layers)
      attn_decode_wide_kernel<decltype(mg)::value>
          <<<grid, 256, 0, cur_stream()>>>(
              bf_ptr(q) + q_off, bf_ptr(kp), bf_ptr(vp), pt.data_ptr<int>(),
              ctx.data_ptr<int>(), alibi_ptr, bf_ptr_mut(out),
              pml.data_ptr<float>(), pacc.data_ptr<float>(), B, Hkv, G, nch, P,
              maxp, n_split, window, scale, q_sb, q_sh, out_sb, out_sh, fp);
    } else if (D <= 128 && pf) {
      attn_decode_mfma_kernel<D, decltype(mg)::value, 1, 1>
          <<<grid, 256, 0, cur_stream()>>>(
              bf_ptr(q) + q_off, bf_ptr(kp), bf_ptr(vp), pt.data_ptr<int>(),
              ctx.data_ptr<int>(), alibi_ptr, bf_ptr_mut(out),
              pml.data_ptr<float>(), pacc.data_ptr<float>(), B, Hkv, G, nch, P,
              maxp, n_split, window, scale, q_sb, q_sh, out_sb, out_sh, fp);
    } else if (D <= 128 && nt2) {
      attn_decode_mfma_kernel<D, decltype(mg)::value, 2>
          <<<grid, 256, 0, cur_stream()>>>(
              bf_ptr(q) + q_off, bf_ptr(kp), bf_ptr(vp), pt.data_ptr<int>(),
              ctx.data_ptr<int>(), alibi_ptr, bf_ptr_mut(out),
              pml.data_ptr<float>(), pacc.data_ptr<float>(), B, Hkv, G, nch, P,
              maxp, n_split, window, scale, q_sb, q_sh, out_sb, out_sh, fp);
    } else {
      attn_decode_mfma_kernel<D, decltype(mg)::value, 1>
          <<<grid, 256, 0, cur_stream()>>>(
              bf_ptr(q) + q_off, bf_ptr(kp), bf_ptr(vp), pt.data_ptr<int>(),
              ctx.data_ptr<int>(), alibi_ptr, bf_ptr_mut(out),
              pml.data_ptr<float>(), pacc.data_ptr<float>(), B, Hkv, G, nch, P,
              maxp, n_split, window, scale, q_sb, q_sh, out_sb, out_sh, fp);
    }
  };
  if (maxg == 4) launch_mfma(std::integral_constant<int, 4>{});
  else launch_mfma(std::integral_constant<int, 16>{});
  if (ext != nullptr) {
    attn_decode_merge_ext_kernel<D>
        <<<B * Hkv * nch, maxg * 16, 0, cur_stream()>>>(
            pml.data_ptr<float>(), pacc.data_ptr<float>(), ext->ml, ext->acc,
            ext->dev_shift, bf_ptr_mut(out), Hkv, G, nch, maxg, n_split,
            out_sb, out_sh);
  } else if (n_split > 1) {
    attn_decode_combine_kernel<D>
        <<<B * Hkv * nch, maxg * 16, 0, cur_stream()>>>(
            pml.data_ptr<float>(), pacc.data_ptr<float>(), bf_ptr_mut(out),
            Hkv, G, nch, maxg, n_split, out_sb, out_sh);
  }
}

static torch::Tensor attn_decode_core(
    const torch::Tensor& q, const torch::Tensor& k_pages,
    const torch::Tensor& v_pages, const torch::Tensor& page_table,
    const torch::Tensor& ctx_lens, const c10::optional<torch::Tensor>& alibi,
    double scale, long window, long n_split_req,
    int B, int Hq, int D, long q_off, long q_sb, long q_sh,
    torch::Tensor out, long out_sb, long out_sh,
    const MixedExt* ext = nullptr) {
  const int Hkv = k_pages.size(1), P = k_pages.size(2), maxp = page_table.size(1);
  const int G = Hq / Hkv;
  TORCH_CHECK(Hq % Hkv == 0);
  TORCH_CHECK(D != 256 || G <= 4, "D=256 decode supports GQA group size <= 4");
  const int nch = (G + 15) / 16;  // MQA chunks (falcon G=71 -> 5)
  const float* alibi_ptr = nullptr;
  if (alibi.has_value()) {
    TORCH_CHECK(alibi->scalar_type() == at::kFloat && alibi->numel() == Hq);
    alibi_ptr = alibi->data_ptr<float>();
  }
  int n_split = (int)n_split_req;
  if (n_split <= 0) {
    // measured optimum (benchmarks/bench_kernels.py attn_decode): size the
    // grid for full residency — NT=1 runs 118 VGPRs -> 4 WGs/CU (1024 WGs),
    // the paired-tile NT=2 variant 158 VGPRs -> 3 WGs/CU (768 WGs); more
    // splits only add merge traffic
    static const int nt_env0 = [] {
      const char* e = std::getenv("BBAMD_ATTN_NT");
      return e ? std::atoi(e) : 2;
    }();
    static const bool pf_env0 = [] {
      const char* e = std::getenv("BBAMD_ATTN_PF");
      return !e || std::atoi(e) != 0;
    }();
    // pipelined variant: 254 VGPRs -> 2 waves/SIMD -> 512 WGs fill the chip
    // (measured: B32 ns=2 50 us / 5.4 TB/s vs 59 at 768-1024 WGs)
    const long target = (pf_env0 && D <= 128) ? 512
                        : (nt_env0 >= 2 && D <= 128) ? 768 : 1024;
    n_split = (int)std::max<long>(
        1, std::min<long>(32, target / std::max(1, B * Hkv * nch)));
  }
  const int maxg = (G <= 4 && nch == 1) ? 4 : 16;
  auto fopt = torch::TensorOptions().device(q.device()).dtype(at::kFloat);
  torch::Tensor pml, pacc;
  if (n_split > 1 || ext != nullptr) {
    pml = torch::empty({(long)B * Hkv * nch * n_split, maxg, 2}, fopt);
    pacc = torch::empty({(long)B * Hkv * nch * n_split, maxg, D}, fopt);
  } else {
    pml = torch::empty({1}, fopt);
    pacc = torch::empty({1}, fopt);
  }
  auto go = [&](auto d) {
    attn_decode_launch<decltype(d)::value>(
        q, k_pages, v_pages, page_table, ctx_lens, alibi_ptr, out, pml, pacc,
        B, Hkv, G, nch, P, maxp, n_split, (int)window, (float)scale, q_off,
        q_sb, q_sh, out_sb, out_sh, ext);
  };
  if (D == 128) go(std::integral_constant<int, 128>{});
  else if (D == 64) go(std::integral_constant<int, 64>{});
  else if (D == 256) go(std::integral_constant<int, 256>{});
  else if (D == 512) go(std::integral_constant<int, 512>{});
  else if (D == 32) go(std::integral_constant<int, 32>{});
  else TORCH_CHECK(false, "unsupported head_dim ", D);
  return out;
}

torch::Tensor attn_decode(torch::Tensor q, torch::Tensor k_pages,
                          torch::Tensor v_pages, torch::Tensor page_table,
                          torch::Tensor ctx_lens, double scale, long window,
                          long n_split_req,
                          c10::optional<torch::Tensor> alibi) {
  CHECK_DEV(q); CHECK_BF16(q); CHECK_CONTIG(q);
  CHECK_DEV_ALL3(k_pages, page_table, ctx_lens);
  if (alibi.has_value()) CHECK_DEV((*alibi));
  TORCH_CHECK(q.dim() == 4 && q.size(2) == 1, "attn_decode expects (B, Hq, 1, D)");
  const int B = q.size(0), Hq = q.size(1), D = q.size(3);
  auto out = torch::empty({B, Hq, 1, D}, q.options());
  return attn_decode_core(q, k_pages, v_pages, page_table, ctx_lens, alibi,
                          scale, window, n_split_req, B, Hq, D,
                          /*q_off*/ 0, (long)Hq * D, (long)D,
                          out, (long)Hq * D, (long)D);
}

// Fused-QKV decode: q section of qkv (B, 1, (Hq+2Hkv)*D) read in place,
// out (B, 1, Hq*D) ready for the O-projection GEMM — zero transposes.
torch::Tensor attn_decode_qkv(torch::Tensor qkv, long Hq, torch::Tensor k_pages,
                              torch::Tensor v_pages, torch::Tensor page_table,
                              torch::Tensor ctx_lens, double scale, long window,
                              long n_split_req) {
  CHECK_DEV(qkv); CHECK_BF16(qkv); CHECK_CONTIG(qkv);
  CHECK_DEV_ALL3(k_pages, page_table, ctx_lens);
  const int Hkv = k_pages.size(1);
  const int D = k_pages.size(3);
  const int B = qkv.size(0);
  TORCH_CHECK(qkv.dim() == 3 && qkv.size(1) == 1 &&
              qkv.size(2) == (Hq + 2 * Hkv) * D, "bad fused qkv shape");
  auto out = torch::empty({B, 1, Hq * D}, qkv.options());
  return attn_decode_core(qkv, k_pages, v_pages, page_table, ctx_lens,
                          c10::nullopt, scale, window, n_split_req, B, (int)Hq,
                          D, /*q_off*/ 0, (long)(Hq + 2 * Hkv) * D, (long)D,
                          out, (long)Hq * D, (long)D)
      .view({B, 1, Hq * D});
}

// ---------------------------------------------------------------------------
// Top-k sparse decode (attn_sparse.hip): scores -> select -> P.V -> combine,
// four launches on the current stream, no host sync, ctx_lens never read on
// the host (kkeep is computed on the device, so the call is graph-capturable).
template <int D>
static void attn_sparse_launch(const torch::Tensor& q, const torch::Tensor& kp,
                               const torch::Tensor& vp, const torch::Tensor& pt,
                               const torch::Tensor& ctx, const float* alibi_ptr,
                               torch::Tensor& out, torch::Tensor& ws,
                               torch::Tensor& lsum, torch::Tensor& pacc, int B,
                               int Hkv, int G, int nch, int maxp, int N,
                               int n_split, double sparsity, float scale,
                               long q_off, long q_sb, long q_sh, long out_sb,
                               long out_sh) {
  const int BH = B * Hkv * nch;
  attn_sparse_scores_kernel<D>
      <<<dim3(BH, (N + 127) / 128), 256, 0, cur_stream()>>>(
          bf_ptr(q) + q_off, bf_ptr(kp), pt.data_ptr<int>(),
          ctx.data_ptr<int>(), alibi_ptr, ws.data_ptr<float>(), Hkv, G, nch,
          maxp, N, scale, q_sb, q_sh);
  attn_sparse_select_kernel<<<B * Hkv * G, 256, 0, cur_stream()>>>(
      ws.data_ptr<float>(), lsum.data_ptr<float>(), ctx.data_ptr<int>(),
      Hkv * G, N, sparsity);
  attn_sparse_pv_kernel<D><<<dim3(BH, n_split), 256, 0, cur_stream()>>>(
      ws.data_ptr<float>(), bf_ptr(vp), pt.data_ptr<int>(),
      ctx.data_ptr<int>(), pacc.data_ptr<float>(), Hkv, G, nch, maxp, N,
      n_split);
  attn_sparse_combine_kernel<<<BH, 256, 0, cur_stream()>>>(
      pacc.data_ptr<float>(), lsum.data_ptr<float>(), bf_ptr_mut(out), Hkv, G,
      nch, D, n_split, out_sb, out_sh);
}

static torch::Tensor attn_sparse_core(
    const torch::Tensor& q, const torch::Tensor& k_pages,
    const torch::Tensor& v_pages, const torch::Tensor& page_table,
    const torch::Tensor& ctx_lens, const c10::optional<torch::Tensor>& alibi,
    double sparsity, double scale, int B, int Hq, int D, long q_off, long q_sb,
    long q_sh, torch::Tensor out, long out_sb, long out_sh) {
  CHECK_BF16(k_pages); CHECK_CONTIG(k_pages);
  CHECK_BF16(v_pages); CHECK_CONTIG(v_pages);
  CHECK_CONTIG(page_table); CHECK_CONTIG(ctx_lens);
  TORCH_CHECK(k_pages.dim() == 4 && v_pages.dim() == 4 && page_table.dim() == 2,
              "bad KV pool / page table rank");
  const int Hkv = k_pages.size(1), P = k_pages.size(2);
  const int maxp = page_table.size(1);
  TORCH_CHECK(P == 16, "sparse decode is written for page size 16, got ", P);
  TORCH_CHECK(k_pages.size(3) == D && v_pages.size(0) == k_pages.size(0) &&
              v_pages.size(1) == Hkv && v_pages.size(2) == D &&
              v_pages.size(3) == P, "K (np,Hkv,P,D) / V (np,Hkv,D,P) mismatch");
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0, "Hq must be a multiple of Hkv");
  TORCH_CHECK(page_table.scalar_type() == at::kInt &&
              ctx_lens.scalar_type() == at::kInt,
              "page_table / ctx_lens must be int32");
  TORCH_CHECK(page_table.size(0) == B && ctx_lens.numel() == B,
              "page_table / ctx_lens batch mismatch");
  TORCH_CHECK(B > 0 && maxp > 0, "empty batch or page table");
  const int G = Hq / Hkv;
  const int nch = (G + 15) / 16;  // MQA chunks (falcon G=71 -> 5)
  const float* alibi_ptr = nullptr;
  if (alibi.has_value()) {
    TORCH_CHECK(alibi->scalar_type() == at::kFloat && alibi->numel() == Hq &&
                alibi->is_contiguous());
    alibi_ptr = alibi->data_ptr<float>();
  }
  const int N = maxp * P;
  // P.V splits: ~1024 workgroups, and at least 256 positions per split
  const int n_split = (int)std::max<long>(
      1, std::min<long>(std::min<long>(32, N / 256),
                        1024 / std::max(1, B * Hkv * nch)));
  auto fopt = torch::TensorOptions().device(q.device()).dtype(at::kFloat);
  auto ws = torch::empty({B, Hq, N}, fopt);
  auto lsum = torch::empty({B, Hq}, fopt);
  auto pacc = torch::empty({(long)B * Hkv * nch * n_split, 16, D}, fopt);
  auto go = [&](auto d) {
    attn_sparse_launch<decltype(d)::value>(
        q, k_pages, v_pages, page_table, ctx_lens, alibi_ptr, out, ws, lsum,
        pacc, B, Hkv, G, nch, maxp, N, n_split, sparsity, (float)scale, q_off,
        q_sb, q_sh, out_sb, out_sh);
  };
  if (D == 128) go(std::integral_constant<int, 128>{});
  else if (D == 64) go(std::integral_constant<int, 64>{});
  else if (D == 256) go(std::integral_constant<int, 256>{});
  else TORCH_CHECK(false, "sparse decode supports head_dim 64/128/256, got ", D);
  return out;
}

torch::Tensor attn_decode_sparse(torch::Tensor q, torch::Tensor k_pages,
                                 torch::Tensor v_pages, torch::Tensor page_table,
                                 torch::Tensor ctx_lens, double sparsity,
                                 double scale,
                                 c10::optional<torch::Tensor> alibi) {
  CHECK_DEV(q); CHECK_BF16(q); CHECK_CONTIG(q);
  CHECK_DEV_ALL3(k_pages, page_table, ctx_lens);
  CHECK_DEV(v_pages);
  if (alibi.has_value()) CHECK_DEV((*alibi));
  TORCH_CHECK(q.dim() == 4 && q.size(2) == 1,
              "attn_decode_sparse expects (B, Hq, 1, D)");
  const int B = q.size(0), Hq = q.size(1), D = q.size(3);
  auto out = torch::empty({B, Hq, 1, D}, q.options());
  return attn_sparse_core(q, k_pages, v_pages, page_table, ctx_lens, alibi,
                          sparsity, scale, B, Hq, D, /*q_off*/ 0, (long)Hq * D,
                          (long)D, out, (long)Hq * D, (long)D);
}

// Fused-QKV sparse decode: q read in place from (B, 1, (Hq+2Hkv)*D), out
// (B, 1, Hq*D) in the O-projection layout.
torch::Tensor attn_decode_sparse_qkv(torch::Tensor qkv, long Hq,
                                     torch::Tensor k_pages,
                                     torch::Tensor v_pages,
                                     torch::Tensor page_table,
                                     torch::Tensor ctx_lens, double sparsity,
                                     double scale) {
  CHECK_DEV(qkv); CHECK_BF16(qkv); CHECK_CONTIG(qkv);
  CHECK_DEV_ALL3(k_pages, page_table, ctx_lens);
  CHECK_DEV(v_pages);
  TORCH_CHECK(k_pages.dim() == 4, "bad KV pool rank");
  const int Hkv = k_pages.size(1);
  const int D = k_pages.size(3);
  const int B = qkv.size(0);
  TORCH_CHECK(Hq > 0 && qkv.dim() == 3 && qkv.size(1) == 1 &&
              qkv.size(2) == (Hq + 2 * Hkv) * D, "bad fused qkv shape");
  auto out = torch::empty({B, 1, Hq * D}, qkv.options());
  return attn_sparse_core(qkv, k_pages, v_pages, page_table, ctx_lens,
                          c10::nullopt, sparsity, scale, B, (int)Hq, D,
                          /*q_off*/ 0, (long)(Hq + 2 * Hkv) * D, (long)D, out,
                          (long)Hq * D, (long)D);
}

// Mixed-device decode: device segment on the MFMA / wide decode kernel in
// forced-partial mode, then one merge launch that folds in the external
// (host-prefix) partial. q is either (B, Hq, 1, D) or the fused QKV buffer
// (B, 1, (Hq+2Hkv)*D) read in place; Hq comes from ext_ml. ctx_lens and all
// kernel positions are LOCAL to the device pool; pos_offset (the absolute
// position of local 0) only enters through the ALiBi shift of the device
// partials. Returns (B, 1, Hq*D), the O-projection layout.
torch::Tensor attn_decode_mixed(torch::Tensor q, torch::Tensor k_pages,
                                torch::Tensor v_pages, torch::Tensor page_table,
                                torch::Tensor ctx_lens, torch::Tensor ext_ml,
                                torch::Tensor ext_acc, double scale, long window,
                                long n_split_req,
                                c10::optional<torch::Tensor> alibi,
                                long pos_offset) {
  CHECK_DEV(q); CHECK_BF16(q); CHECK_CONTIG(q);
  CHECK_DEV_ALL3(k_pages, page_table, ctx_lens);
  CHECK_DEV(ext_ml); CHECK_CONTIG(ext_ml);
  CHECK_DEV(ext_acc); CHECK_CONTIG(ext_acc);
  const int Hkv = k_pages.size(1), D = k_pages.size(3);
  const int B = q.size(0);
  TORCH_CHECK(ext_ml.scalar_type() == at::kFloat && ext_ml.dim() == 3 &&
              ext_ml.size(0) == B && ext_ml.size(2) == 2,
              "ext_ml must be f32 (B, Hq, 2)");
  const int Hq = ext_ml.size(1);
  TORCH_CHECK(ext_acc.scalar_type() == at::kFloat && ext_acc.dim() == 3 &&
              ext_acc.size(0) == B && ext_acc.size(1) == Hq &&
              ext_acc.size(2) == D, "ext_acc must be f32 (B, Hq, D)");
  TORCH_CHECK(page_table.size(0) == B && ctx_lens.numel() == B,
              "page_table / ctx_lens batch mismatch");
  long q_sb;
  if (q.dim() == 4) {
    TORCH_CHECK(q.size(1) == Hq && q.size(2) == 1 && q.size(3) == D,
                "attn_decode_mixed expects q (B, Hq, 1, D)");
    q_sb = (long)Hq * D;
  } else {
    TORCH_CHECK(q.dim() == 3 && q.size(1) == 1 &&
                q.size(2) == (long)(Hq + 2 * Hkv) * D, "bad fused qkv shape");
    q_sb = (long)(Hq + 2 * Hkv) * D;
  }
  torch::Tensor shift;
  MixedExt ext{ext_ml.data_ptr<float>(), ext_acc.data_ptr<float>(), nullptr};
  if (alibi.has_value()) {
    CHECK_DEV((*alibi));
    TORCH_CHECK(alibi->scalar_type() == at::kFloat && alibi->numel() == Hq);
    shift = (*alibi * (double)pos_offset).contiguous();
    ext.dev_shift = shift.data_ptr<float>();
  }
  auto out = torch::empty({B, 1, (long)Hq * D}, q.options());
  attn_decode_core(q, k_pages, v_pages, page_table, ctx_lens, alibi, scale,
                   window, n_split_req, B, Hq, D, /*q_off*/ 0, q_sb, (long)D,
                   out, (long)Hq * D, (long)D, &ext);
  return out;
}

torch::Tensor attn_prefill(torch::Tensor q, torch::Tensor k_pages,
                           torch::Tensor v_pages, torch::Tensor page_table,
                           torch::Tensor q_start, double scale, long window,
                           c10::optional<torch::Tensor> alibi,
                           c10::optional<torch::Tensor> tree_mask) {
  CHECK_DEV(q); CHECK_BF16(q); CHECK_CONTIG(q);
  CHECK_DEV_ALL3(k_pages, page_table, q_start);
  if (alibi.has_value()) CHECK_DEV((*alibi));
  TORCH_CHECK(q.dim() == 4, "attn_prefill expects (B, Hq, Tq, D)");
  const int B = q.size(0), Hq = q.size(1), Tq = q.size(2), D = q.size(3);
  const int Hkv = k_pages.size(1), P = k_pages.size(2), maxp = page_table.size(1);
  const int G = Hq / Hkv;
  const float* alibi_ptr = nullptr;
  if (alibi.has_value()) {
    TORCH_CHECK(alibi->scalar_type() == at::kFloat && alibi->numel() == Hq);
    alibi_ptr = alibi->data_ptr<float>();
  }
  const unsigned char* tm_ptr = nullptr;
  if (tree_mask.has_value()) {
    TORCH_CHECK(tree_mask->scalar_type() == at::kBool &&
                tree_mask->is_contiguous() &&
                tree_mask->sizes() == (at::IntArrayRef{B, Tq, Tq}),
                "tree_mask must be contiguous bool (B, Tq, Tq)");
    TORCH_CHECK(window == 0, "tree_mask + sliding window: use the torch path");
    CHECK_DEV((*tree_mask));
    // kBool tensors dispatch data_ptr<bool>, not <unsigned char> (Byte)
    tm_ptr = reinterpret_cast<const unsigned char*>(
        tree_mask->data_ptr<bool>());
  }
  auto out = torch::empty_like(q);
  dim3 grid((Tq + 127) / 128, B * Hq);
  auto launch = [&](auto d) {
    attn_prefill_kernel<decltype(d)::value><<<grid, 512, 0, cur_stream()>>>(
        bf_ptr(q), bf_ptr(k_pages), bf_ptr(v_pages), page_table.data_ptr<int>(),
        q_start.data_ptr<int>(), alibi_ptr, tm_ptr, bf_ptr_mut(out), B, Hq, G,
        Tq, P, maxp, (int)window, (float)scale,
        (long)Hq * Tq * D, (long)D, (long)Tq * D,
        (long)Hq * Tq * D, (long)D, (long)Tq * D);
  };
  if (D == 128) launch(std::integral_constant<int, 128>{});
  else if (D == 64) launch(std::integral_constant<int, 64>{});
  else if (D == 256) launch(std::integral_constant<int, 256>{});
  else if (D == 32) launch(std::integral_constant<int, 32>{});
  else TORCH_CHECK(false, "unsupported head_dim ", D);
  return out;
}

// Fused-QKV prefill: q read from qkv (B, Tq, (Hq+2Hkv)*D) in place,
// out (B, Tq, Hq*D) ready for the O-projection GEMM.
torch::Tensor attn_prefill_qkv(torch::Tensor qkv, long Hq_,
                               torch::Tensor k_pages, torch::Tensor v_pages,
                               torch::Tensor page_table, torch::Tensor q_start,
                               double scale, long window) {
  CHECK_DEV(qkv); CHECK_BF16(qkv); CHECK_CONTIG(qkv);
  CHECK_DEV_ALL3(k_pages, page_table, q_start);
  const int Hkv = k_pages.size(1), P = k_pages.size(2), D = k_pages.size(3);
  const int maxp = page_table.size(1);
  const int Hq = (int)Hq_;
  const int B = qkv.size(0), Tq = qkv.size(1);
  const int X = Hq + 2 * Hkv;
  TORCH_CHECK(qkv.dim() == 3 && qkv.size(2) == (long)X * D, "bad fused qkv shape");
  const int G = Hq / Hkv;
  auto out = torch::empty({B, Tq, (long)Hq * D}, qkv.options());
  dim3 grid((Tq + 127) / 128, B * Hq);
  auto launch = [&](auto d) {
    attn_prefill_kernel<decltype(d)::value><<<grid, 512, 0, cur_stream()>>>(
        bf_ptr(qkv), bf_ptr(k_pages), bf_ptr(v_pages), page_table.data_ptr<int>(),
        q_start.data_ptr<int>(), nullptr, nullptr, bf_ptr_mut(out), B, Hq, G,
        Tq, P, maxp, (int)window, (float)scale,
        (long)Tq * X * D, (long)X * D, (long)D,
        (long)Tq * Hq * D, (long)Hq * D, (long)D);
  };
  if (D == 128) launch(std::integral_constant<int, 128>{});
  else if (D == 64) launch(std::integral_constant<int, 64>{});
  else if (D == 256) launch(std::integral_constant<int, 256>{});
  else if (D == 32) launch(std::integral_constant<int, 32>{});
  else TORCH_CHECK(false, "unsupported head_dim ", D);
  return out;
}

// ---------------------------------------------------------------------------
// training attention (dense K/V, LSE out, flash backward)
// ---------------------------------------------------------------------------

// (B, T, H, D) bf16 view with a contiguous last dim and 16-byte aligned rows.
static void check_train_operand(const torch::Tensor& t, const char* name,
                                long B, long T, long D) {
  TORCH_CHECK(t.is_cuda(), name, " must be on device");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.dim() == 4 && t.size(0) == B && t.size(1) == T && t.size(3) == D,
              name, " must be (B, T, H, D) matching q");
  TORCH_CHECK(t.stride(3) == 1, name, " needs a contiguous last dim");
  TORCH_CHECK(t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0 &&
              t.stride(2) % 8 == 0 && t.storage_offset() % 8 == 0,
              name, " rows must be 16-byte aligned");
}

static const float* train_alibi_ptr(const c10::optional<torch::Tensor>& alibi,
                                    const torch::Tensor& q, long Hq) {
  if (!alibi.has_value()) return nullptr;
  TORCH_CHECK(alibi->is_cuda() && alibi->get_device() == q.get_device(),
              "alibi must be on q's device");
  TORCH_CHECK(alibi->scalar_type() == at::kFloat && alibi->is_contiguous() &&
              alibi->numel() == Hq, "alibi must be contiguous f32 (Hq,)");
  return alibi->data_ptr<float>();
}

static void check_train_geometry(const torch::Tensor& q, const torch::Tensor& k,
                                 const torch::Tensor& v, long window) {
  TORCH_CHECK(q.dim() == 4, "attn_train expects q (B, T, Hq, D)");
  const long B = q.size(0), T = q.size(1), Hq = q.size(2), D = q.size(3);
  TORCH_CHECK(D == 64 || D == 128, "attn_train supports head_dim 64 and 128, got ", D);
  TORCH_CHECK(B > 0 && T > 0 && Hq > 0, "attn_train: empty input");
  check_train_operand(q, "q", B, T, D);
  check_train_operand(k, "k", B, T, D);
  check_train_operand(v, "v", B, T, D);
  const long Hkv = k.size(2);
  TORCH_CHECK(Hkv > 0 && v.size(2) == Hkv && Hq % Hkv == 0,
              "attn_train: Hq must be a multiple of Hkv, and k/v must agree");
  TORCH_CHECK(k.get_device() == q.get_device() && v.get_device() == q.get_device(),
              "attn_train: q, k, v must share a device");
  TORCH_CHECK(window >= 0 && window < (1L << 30), "attn_train: bad window");
  const long ntile = (T + TR_ROWS - 1) / TR_ROWS;
  TORCH_CHECK(T < (1L << 30) && B * Hq * ntile < (1L << 31),
              "attn_train: grid too large");
}

std::tuple<torch::Tensor, torch::Tensor> attn_train_fwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v, double scale,
    long window, c10::optional<torch::Tensor> alibi, bool want_lse) {
  check_train_geometry(q, k, v, window);
  const long B = q.size(0), T = q.size(1), Hq = q.size(2), D = q.size(3);
  const long Hkv = k.size(2);
  const float* alibi_ptr = train_alibi_ptr(alibi, q, Hq);
  c10::DeviceGuard guard(q.device());
  auto out = torch::empty({B, T, Hq, D}, q.options());
  auto lse = torch::empty({want_lse ? B : 0, Hq, T},
                          q.options().dtype(at::kFloat));
  const int ntile = (int)((T + TR_ROWS - 1) / TR_ROWS);
  const unsigned grid = (unsigned)(B * Hq * ntile);
  auto launch = [&](auto d) {
    attn_train_fwd_kernel<decltype(d)::value><<<grid, 512, 0, cur_stream()>>>(
        bf_ptr(q), bf_ptr(k), bf_ptr(v), alibi_ptr, bf_ptr_mut(out),
        want_lse ? lse.data_ptr<float>() : nullptr,
        (int)Hq, (int)(Hq / Hkv), (int)T, ntile, (int)window, (float)scale,
        q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1),
        k.stride(2), v.stride(0), v.stride(1), v.stride(2));
  };
  if (D == 128) launch(std::integral_constant<int, 128>{});
  else launch(std::integral_constant<int, 64>{});
  return {out, lse};
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> attn_train_bwd(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor out, torch::Tensor lse, double scale, long window,
    c10::optional<torch::Tensor> alibi) {
  check_train_geometry(q, k, v, window);
  const long B = q.size(0), T = q.size(1), Hq = q.size(2), D = q.size(3);
  const long Hkv = k.size(2);
  check_train_operand(dout, "dout", B, T, D);
  check_train_operand(out, "out", B, T, D);
  TORCH_CHECK(dout.size(2) == Hq && out.size(2) == Hq && out.is_contiguous(),
              "attn_train_bwd: dout/out must be (B, T, Hq, D), out contiguous");
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == at::kFloat &&
              lse.is_contiguous() && lse.dim() == 3 && lse.size(0) == B &&
              lse.size(1) == Hq && lse.size(2) == T,
              "attn_train_bwd: lse must be contiguous f32 (B, Hq, T)");
  TORCH_CHECK(dout.get_device() == q.get_device() &&
              out.get_device() == q.get_device() &&
              lse.get_device() == q.get_device(),
              "attn_train_bwd: all tensors must share a device");
  const float* alibi_ptr = train_alibi_ptr(alibi, q, Hq);
  c10::DeviceGuard guard(q.device());
  auto dq = torch::empty({B, T, Hq, D}, q.options());
  auto dk = torch::empty({B, T, Hkv, D}, q.options());
  auto dv = torch::empty({B, T, Hkv, D}, q.options());
  auto delta = torch::empty({B, Hq, T}, lse.options());
  const int ntile = (int)((T + TR_ROWS - 1) / TR_ROWS);
  const int G = (int)(Hq / Hkv);
  auto launch = [&](auto d) {
    constexpr int DD = decltype(d)::value;
    // delta is written by the dQ kernel and read by the dK/dV kernel:
    // same stream, so the order is the launch order
    attn_train_dq_kernel<DD><<<(unsigned)(B * Hq * ntile), 512, 0, cur_stream()>>>(
        bf_ptr(dout), bf_ptr(q), bf_ptr(k), bf_ptr(v), bf_ptr(out),
        lse.data_ptr<float>(), alibi_ptr, bf_ptr_mut(dq),
        delta.data_ptr<float>(), (int)Hq, G, (int)T, ntile, (int)window,
        (float)scale, dout.stride(0), dout.stride(1), dout.stride(2),
        q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1),
        k.stride(2), v.stride(0), v.stride(1), v.stride(2));
    attn_train_dkdv_kernel<DD><<<(unsigned)(B * Hkv * ntile), 512, 0, cur_stream()>>>(
        bf_ptr(dout), bf_ptr(q), bf_ptr(k), bf_ptr(v), lse.data_ptr<float>(),
        delta.data_ptr<float>(), alibi_ptr, bf_ptr_mut(dk), bf_ptr_mut(dv),
        (int)Hq, G, (int)T, ntile, (int)window, (float)scale,
        dout.stride(0), dout.stride(1), dout.stride(2),
        q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1),
        k.stride(2), v.stride(0), v.stride(1), v.stride(2));
  };
  if (D == 128) launch(std::integral_constant<int, 128>{});
  else launch(std::integral_constant<int, 64>{});
  return {dq, dk, dv};
}

// Fused RoPE + paged-KV write on the raw QKV GEMM output.
void rope_kv_write_(torch::Tensor qkv, long Hq_, long Hkv_, torch::Tensor cos_t,
                    torch::Tensor sin_t, c10::optional<torch::Tensor> pos,
                    torch::Tensor k_pages, torch::Tensor v_pages,
                    torch::Tensor page_table, torch::Tensor start_pos) {
  CHECK_DEV(qkv); CHECK_BF16(qkv); CHECK_CONTIG(qkv);
  CHECK_DEV_ALL3(k_pages, page_table, start_pos);
  CHECK_DEV_ALL2(cos_t, sin_t);
  if (pos.has_value()) CHECK_DEV((*pos));
  const int Hq = (int)Hq_, Hkv = (int)Hkv_;
  const int P = k_pages.size(2), D = k_pages.size(3);
  const int maxp = page_table.size(1);
  const int B = qkv.size(0), T = qkv.size(1);
  TORCH_CHECK(qkv.size(2) == (long)(Hq + 2 * Hkv) * D, "bad fused qkv shape");
  const int* pos_ptr = nullptr;
  if (pos.has_value()) {
    TORCH_CHECK(pos->scalar_type() == at::kInt);
    pos_ptr = pos->data_ptr<int>();
  }
  dim3 grid(B * T, Hq + 2 * Hkv);
  rope_kv_write_kernel<false><<<grid, 64, 0, cur_stream()>>>(
      bf_ptr_mut(qkv), nullptr, nullptr, 0, cos_t.data_ptr<float>(),
      sin_t.data_ptr<float>(), pos_ptr,
      bf_ptr_mut(k_pages), bf_ptr_mut(v_pages), page_table.data_ptr<int>(),
      start_pos.data_ptr<int>(), B, Hq, Hkv, T, D, P, maxp,
      (int)cos_t.size(0));
}

// The same on the QKV GEMM's uncombined split-K output: part is f32
// (ksplit, B*T, (Hq+2Hkv)*D) from gemm_skinny(defer_combine=true). Sums the
// slabs (+bias) as the combine kernel would, ropes, writes K/V to the pages
// and returns the bf16 (B, T, (Hq+2Hkv)*D) buffer whose q section is filled;
// its k and v sections are NOT written. Second result: (B,) int32
// start_pos + T, the context lengths the attention launch takes next.
std::vector<torch::Tensor> rope_kv_write_part(torch::Tensor part,
                                 c10::optional<torch::Tensor> bias, long B_,
                                 long T_, long Hq_, long Hkv_,
                                 torch::Tensor cos_t, torch::Tensor sin_t,
                                 c10::optional<torch::Tensor> pos,
                                 torch::Tensor k_pages, torch::Tensor v_pages,
                                 torch::Tensor page_table,
                                 torch::Tensor start_pos) {
  CHECK_DEV(part); CHECK_CONTIG(part);
  CHECK_DEV_ALL3(k_pages, page_table, start_pos);
  CHECK_DEV_ALL3(cos_t, sin_t, v_pages);
  CHECK_BF16(k_pages); CHECK_CONTIG(k_pages); CHECK_CONTIG(v_pages);
  if (pos.has_value()) CHECK_DEV((*pos));
  const int Hq = (int)Hq_, Hkv = (int)Hkv_, B = (int)B_, T = (int)T_;
  const int P = k_pages.size(2), D = k_pages.size(3);
  const int maxp = page_table.size(1);
  const long X = Hq + 2 * Hkv;
  TORCH_CHECK(part.scalar_type() == at::kFloat && part.dim() == 3 &&
              part.size(1) == (long)B * T && part.size(2) == X * D,
              "part must be f32 (ksplit, B*T, (Hq+2Hkv)*D)");
  TORCH_CHECK(D % 8 == 0, "rope_kv_write_part needs head_dim % 8 == 0");
  TORCH_CHECK(cos_t.scalar_type() == at::kFloat && cos_t.size(1) == D / 2);
  TORCH_CHECK(page_table.scalar_type() == at::kInt &&
              start_pos.scalar_type() == at::kInt &&
              page_table.size(0) == B && start_pos.numel() == B);
  const unsigned short* bp = nullptr;
  if (bias.has_value()) {
    CHECK_DEV((*bias)); CHECK_BF16((*bias));
    TORCH_CHECK(bias->is_contiguous() && bias->numel() == X * D);
    bp = bf_ptr(*bias);
  }
  const int* pos_ptr = nullptr;
  if (pos.has_value()) {
    TORCH_CHECK(pos->scalar_type() == at::kInt && pos->numel() == (long)B * T);
    pos_ptr = pos->data_ptr<int>();
  }
  auto qkv = torch::empty({(long)B, (long)T, X * D},
                          k_pages.options().dtype(at::kBFloat16));
  auto ctx = torch::empty({(long)B}, start_pos.options());
  dim3 grid(B * T, Hq + 2 * Hkv);
  rope_kv_write_kernel<true><<<grid, 64, 0, cur_stream()>>>(
      bf_ptr_mut(qkv), part.data_ptr<float>(), bp, (int)part.size(0),
      cos_t.data_ptr<float>(), sin_t.data_ptr<float>(), pos_ptr,
      bf_ptr_mut(k_pages), bf_ptr_mut(v_pages), page_table.data_ptr<int>(),
      start_pos.data_ptr<int>(), B, Hq, Hkv, T, D, P, maxp,
      (int)cos_t.size(0), ctx.data_ptr<int>());
  return {qkv, ctx};
}


// C(S,N) = A[row(s)] @ W[expert(s)]^T — grouped decode MoE (moe_gemm.hip).
// off: (E+1,) int32 exclusive prefix sums of per-expert slot counts;
// rowmap: optional (S,) int32 slot->A-row gather; scale: optional (S,) f32
// per-slot epilogue scale (routing weights). S and mchunks are host-side
// upper-bound shapes so no device sync is needed.
torch::Tensor moe_gemm(torch::Tensor A, torch::Tensor W, torch::Tensor off,
                       c10::optional<torch::Tensor> rowmap,
                       c10::optional<torch::Tensor> scale,
                       long S, long mchunks) {
  CHECK_DEV(A); CHECK_BF16(A); CHECK_CONTIG(A);
  CHECK_DEV(W); CHECK_BF16(W); CHECK_CONTIG(W);
  CHECK_DEV(off);
  TORCH_CHECK(W.dim() == 3, "W must be (E, N, K)");
  const int E = W.size(0), N = W.size(1), K = W.size(2);
  TORCH_CHECK(A.size(-1) == K, "A/W K mismatch");
  TORCH_CHECK(K % 32 == 0 && N % 64 == 0, "K%32, N%64 required");
  TORCH_CHECK(off.scalar_type() == at::kInt && off.numel() == E + 1);
  const int* rmp = nullptr;
  if (rowmap.has_value()) {
    TORCH_CHECK(rowmap->scalar_type() == at::kInt &&
                rowmap->is_contiguous() && rowmap->numel() == S);
    CHECK_DEV((*rowmap));
    rmp = rowmap->data_ptr<int>();
  }
  const float* sp = nullptr;
  if (scale.has_value()) {
    TORCH_CHECK(scale->scalar_type() == at::kFloat &&
                scale->is_contiguous() && scale->numel() == S);
    CHECK_DEV((*scale));
    sp = scale->data_ptr<float>();
  }
  auto C = torch::empty({S, (long)N}, A.options());
  TORCH_CHECK(mchunks >= 1);
  dim3 grid(N / 64, (unsigned)(E * mchunks));
  if (K % 256 == 0)
    moe_gemm_v2_kernel<2><<<grid, 256, 0, cur_stream()>>>(
        bf_ptr(A), bf_ptr(W), off.data_ptr<int>(), rmp, sp, bf_ptr_mut(C),
        N, K, (int)mchunks);
  else
    moe_gemm_kernel<2><<<grid, 256, 0, cur_stream()>>>(
        bf_ptr(A), bf_ptr(W), off.data_ptr<int>(), rmp, sp, bf_ptr_mut(C),
        N, K, (int)mchunks);
  return C;
}


// The ksplit rule of moe_gemm_w4 (0 = this rule), normalised like gemm_w4's:
// the W4 stream is latency-bound below ~1800 blocks. The host cannot know
// how many experts are active without a sync; min(E, S) bounds it.
static int moe_w4_ksplit(int E, int N, int K, long S, long ksplit_req,
                         int* kchunk) {
  int ksplit = (int)ksplit_req;
  if (ksplit <= 0) {
    const long blocks = (long)(N / 64) * std::max<long>(1, std::min<long>(E, S));
    ksplit = (int)std::max<long>(1, std::min<long>(K / 512, 1792 / blocks));
  }
  // groups of 64 must not straddle splits; slices of 128 keep the k-loop
  // tail-free
  const int nch = K / 128;
  const int per = (nch + ksplit - 1) / ksplit;
  *kchunk = per * 128;
  return (nch + per - 1) / per;
}

// C(S,N) = (A[row(s)] @ dequant4(Wq[expert(s)])^T) * slot_scale[s] — grouped
// decode MoE over 4-bit weights (moe_gemm_w4.hip). packed (E, N, K/2) u8,
// scale / zero (E, N, K/64) f16 in quant4_pack layout; off, rowmap,
// slot_scale, S and mchunks as for moe_gemm. ksplit as for gemm_w4 (0 = the
// op's own rule).
torch::Tensor moe_gemm_w4(torch::Tensor A, torch::Tensor packed,
                          torch::Tensor scale, torch::Tensor zero,
                          torch::Tensor off,
                          c10::optional<torch::Tensor> rowmap,
                          c10::optional<torch::Tensor> slot_scale,
                          long S, long mchunks, long ksplit_req) {
  CHECK_DEV(A); CHECK_BF16(A); CHECK_CONTIG(A);
  CHECK_DEV_ALL3(packed, scale, zero);
  CHECK_CONTIG(packed); CHECK_CONTIG(scale); CHECK_CONTIG(zero);
  CHECK_DEV(off);
  TORCH_CHECK(packed.scalar_type() == at::kByte &&
              scale.scalar_type() == at::kHalf &&
              zero.scalar_type() == at::kHalf,
              "packed must be u8, scale and zero f16");
  TORCH_CHECK(packed.dim() == 3, "packed must be (E, N, K/2)");
  const int E = packed.size(0), N = packed.size(1);
  const int K = (int)packed.size(2) * 2;
  TORCH_CHECK(A.dim() == 2 && A.size(1) == K, "A/packed K mismatch");
  TORCH_CHECK(K % 128 == 0 && N % 64 == 0, "K%128, N%64 required");
  TORCH_CHECK(scale.numel() == (long)E * N * (K / 64) &&
              zero.numel() == scale.numel(), "scale/zero shape mismatch");
  TORCH_CHECK(off.scalar_type() == at::kInt && off.is_contiguous() &&
              off.numel() == E + 1);
  TORCH_CHECK(S >= 0 && mchunks >= 1 && ksplit_req >= 0);
  const int* rmp = nullptr;
  if (rowmap.has_value()) {
    TORCH_CHECK(rowmap->scalar_type() == at::kInt &&
                rowmap->is_contiguous() && rowmap->numel() == S);
    CHECK_DEV((*rowmap));
    rmp = rowmap->data_ptr<int>();
  }
  const float* sp = nullptr;
  if (slot_scale.has_value()) {
    TORCH_CHECK(slot_scale->scalar_type() == at::kFloat &&
                slot_scale->is_contiguous() && slot_scale->numel() == S);
    CHECK_DEV((*slot_scale));
    sp = slot_scale->data_ptr<float>();
  }
  auto C = torch::empty({S, (long)N}, A.options());
  if (S == 0) return C;
  int kchunk = 0;
  const int ksplit = moe_w4_ksplit(E, N, K, S, ksplit_req, &kchunk);
  torch::Tensor part;
  float* pp = nullptr;
  if (ksplit > 1) {
    part = torch::empty({(long)ksplit, S, (long)N},
                        A.options().dtype(at::kFloat));
    pp = part.data_ptr<float>();
  }
  dim3 grid(N / 64, (unsigned)(E * mchunks), ksplit);
  TORCH_CHECK(grid.y <= 65535, "E * mchunks exceeds the grid limit");
  moe_gemm_w4_kernel<2><<<grid, 256, 0, cur_stream()>>>(
      bf_ptr(A), packed.data_ptr<unsigned char>(),
      reinterpret_cast<const __half*>(scale.data_ptr()),
      reinterpret_cast<const __half*>(zero.data_ptr()),
      off.data_ptr<int>(), rmp, sp, bf_ptr_mut(C), pp,
      (int)S, N, K, (int)mchunks, kchunk);
  if (ksplit > 1) {
    const long total4 = S * N / 4;
    const int cgrid = (int)std::min<long>((total4 + 255) / 256, 2048);
    moe_gemm_w4_combine_kernel<<<cgrid, 256, 0, cur_stream()>>>(
        pp, off.data_ptr<int>() + E, sp, bf_ptr_mut(C), (int)S, N, ksplit);
  }
  return C;
}


// C(M,N) = A @ dequant4(Wq)^T [+R] [+bias], M <= 32 (w4_gemm.hip). Wq/scale/
// zero in quant4_pack layout (2 codes/byte along K, f16 scale+zero per group
// of 64). ~3.5x less weight-stream bytes than the bf16 kernel.
torch::Tensor gemm_w4(torch::Tensor A, torch::Tensor Wq, torch::Tensor scale,
                      torch::Tensor zero,
                      c10::optional<torch::Tensor> residual,
                      c10::optional<torch::Tensor> bias, long N_, long ksplit_req) {
  CHECK_DEV(A); CHECK_CONTIG(A);
  TORCH_CHECK(A.scalar_type() == at::kHalf,
              "gemm_w4 takes fp16 activations (wrapper converts)");
  CHECK_DEV_ALL3(Wq, scale, zero);
  CHECK_CONTIG(Wq);
  TORCH_CHECK(Wq.scalar_type() == at::kByte && scale.scalar_type() == at::kHalf
              && zero.scalar_type() == at::kHalf);
  const int K = A.size(-1);
  const int M = A.numel() / K;
  const int N = (int)N_;
  TORCH_CHECK(M <= 32, "gemm_w4 is for M <= 32, got ", M);
  TORCH_CHECK(Wq.numel() == (long)N * K / 2, "Wq shape mismatch");
  TORCH_CHECK(scale.numel() == (long)N * K / 64, "scale shape mismatch");
  TORCH_CHECK(K % 128 == 0 && N % 64 == 0, "K%128, N%64 required");
  auto sizes = A.sizes().vec();
  sizes.back() = N;
  auto C = torch::empty(sizes, A.options().dtype(at::kBFloat16));
  const unsigned short* rp = nullptr;
  if (residual.has_value()) {
    TORCH_CHECK(residual->is_contiguous() && residual->numel() == (long)M * N);
    rp = bf_ptr(*residual);
  }
  const unsigned short* bp = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_contiguous() && bias->numel() == N);
    bp = bf_ptr(*bias);
  }
  // M==1 (the speculative-draft GEMV shape): contiguous 1 KB code loads +
  // v_dot2 — measured 2x the bf16 kernel (w4_probe.hip). The MROWS<=4
  // extension was measured and REJECTED for dispatch: amortizing the
  // dequant over rows loses to the split-K MFMA form (M4 down-proj 131 us
  // vs ~13 — the per-lane 4 B A loads scale with M and dominate); the
  // kernel keeps MROWS as a template parameter, but only MROWS == 1 is
  // reachable from this dispatch: the MROWS > 1 instantiations are not
  // run by any test.
  if (M == 1 && K % 2048 == 0 && K / 2048 <= 7) {
    const int rpw = 4;
    dim3 gv((N / rpw + 3) / 4);
    auto lv2 = [&](auto nl, auto mr) {
      gemm_w4_gemv_kernel<decltype(nl)::value, decltype(mr)::value>
          <<<gv, 256, 0, cur_stream()>>>(
              reinterpret_cast<const _Float16*>(A.data_ptr()),
              Wq.data_ptr<unsigned char>(),
              reinterpret_cast<const __half*>(scale.data_ptr()),
              reinterpret_cast<const __half*>(zero.data_ptr()),
              rp, bp, bf_ptr_mut(C), N, K, rpw);
    };
    auto lv = [&](auto nl) {
      switch (M) {
        case 1: lv2(nl, std::integral_constant<int, 1>{}); break;
        case 2: lv2(nl, std::integral_constant<int, 2>{}); break;
        case 3: lv2(nl, std::integral_constant<int, 3>{}); break;
        default: lv2(nl, std::integral_constant<int, 4>{}); break;
      }
    };
    switch (K / 2048) {
      case 1: lv(std::integral_constant<int, 1>{}); break;
      case 2: lv(std::integral_constant<int, 2>{}); break;
      case 3: lv(std::integral_constant<int, 3>{}); break;
      case 4: lv(std::integral_constant<int, 4>{}); break;
      case 5: lv(std::integral_constant<int, 5>{}); break;
      case 6: lv(std::integral_constant<int, 6>{}); break;
      default: lv(std::integral_constant<int, 7>{}); break;
    }
    return C;
  }
  int ksplit = (int)ksplit_req;
  if (ksplit <= 0) {
    // the w4 stream is LATENCY-bound at the bf16 kernel's grid size (1.2
    // TB/s at 448 blocks); split K until the grid reaches ~1800 blocks
    // (w4_probe.hip: ksplit=4 on N=28672 -> 2.25 TB/s, plateau beyond)
    ksplit = (int)std::max<long>(1, std::min<long>(K / 512,
                                                   1792 / std::max(1, (N + 63) / 64)));
  }
  // groups of 64 must not straddle splits; slices of 128 keep the k-loop
  // tail-free
  const int nch = K / 128;
  const int per = (nch + ksplit - 1) / ksplit;
  ksplit = (nch + per - 1) / per;
  const int kchunk = per * 128;
  torch::Tensor part;
  float* pp = nullptr;
  if (ksplit > 1) {
    part = torch::empty({(long)ksplit, (long)M, (long)N},
                        torch::TensorOptions().device(A.device()).dtype(at::kFloat));
    pp = part.data_ptr<float>();
  }
  dim3 grid((N + 63) / 64, ksplit);
  auto launch = [&](auto mt) {
    gemm_skinny_w4_kernel<decltype(mt)::value><<<grid, 256, 0, cur_stream()>>>(
        reinterpret_cast<const _Float16*>(A.data_ptr()),
        Wq.data_ptr<unsigned char>(),
        reinterpret_cast<const __half*>(scale.data_ptr()),
        reinterpret_cast<const __half*>(zero.data_ptr()),
        ksplit == 1 ? rp : nullptr, ksplit == 1 ? bp : nullptr,
        bf_ptr_mut(C), pp, M, N, K, kchunk, ksplit);
  };
  if (M <= 16) launch(std::integral_constant<int, 1>{});
  else launch(std::integral_constant<int, 2>{});
  if (ksplit > 1) {
    const long total = (long)M * N;
    const int cgrid = (int)std::min<long>((total + 255) / 256, 2048);
    gemm_skinny_combine_kernel<<<cgrid, 256, 0, cur_stream()>>>(
        pp, rp, bp, bf_ptr_mut(C), M, N, ksplit);
  }
  return C;
}

// ---------------------------------------------------------------------------
// skinny-M GEMM (decode projections)
// ---------------------------------------------------------------------------

// C(M,N) = A(M,K) @ W(N,K)^T [+ residual (M,N)] [+ bias (N,)], M <= 32.
torch::Tensor gemm_skinny(torch::Tensor A, torch::Tensor W,
                          c10::optional<torch::Tensor> residual,
                          c10::optional<torch::Tensor> bias, long ksplit_req,
                          c10::optional<torch::Tensor> norm_w, double eps,
                          c10::optional<torch::Tensor> ss_in,
                          c10::optional<torch::Tensor> ss_out,
                          long norm_mode_req, bool defer_combine,
                          c10::optional<torch::Tensor> cnt) {
  // defer_combine: under split-K skip the combine and return the f32 slabs
  // (ksplit, M, N) for a consumer that folds them itself (rope_kv_write_part);
  // bias is then the consumer's to add. With ksplit == 1 there is nothing to
  // defer and the finished bf16 C comes back as usual.
  // cnt: (>= N/64,) int32 zeros — under split-K on the v2 kernel the combine
  // runs inside the GEMM launch (last-arriver reduction); the kernel leaves
  // the counters zero again.
  CHECK_DEV(A); CHECK_BF16(A); CHECK_CONTIG(A);
  CHECK_DEV(W); CHECK_BF16(W); CHECK_CONTIG(W);
  const int K = A.size(-1);
  const int M = A.numel() / K;
  const int N = W.size(0);
  TORCH_CHECK(M <= 32, "gemm_skinny is for M <= 32, got ", M);
  TORCH_CHECK(W.size(1) == K, "A/W K mismatch");
  TORCH_CHECK(K % 32 == 0 && N % 64 == 0, "K%32, N%64 required");
  // norm_mode: 0 none; 1 scale A by invr*norm_w per stage; 2 norm weight
  // pre-folded into W — only the invr accumulator scale remains (cheap).
  int norm_mode = (int)norm_mode_req;
  const unsigned short* nwp = nullptr;
  if (norm_w.has_value()) {
    TORCH_CHECK(norm_w->is_contiguous() && norm_w->numel() == K &&
                norm_w->scalar_type() == at::kBFloat16,
                "norm_w must be contiguous bf16 of length K");
    nwp = bf_ptr(*norm_w);
    if (norm_mode == 0) norm_mode = 1;
  }
  TORCH_CHECK(norm_mode != 1 || nwp, "norm_mode 1 needs norm_w");
  if (norm_mode)
    TORCH_CHECK(K % 256 == 0, "fused rmsnorm needs the v2 (K%256) kernel");
  // ss_in: (nstripes, 32) f32 row sum-of-squares left by the producing
  // GEMM's epilogue — lets the fused rmsnorm skip re-streaming A.
  const float* ssinp = nullptr;
  int nstripes = 0;
  if (ss_in.has_value()) {
    TORCH_CHECK(norm_mode != 0, "ss_in only meaningful with a norm mode");
    TORCH_CHECK(ss_in->is_contiguous() && ss_in->scalar_type() == at::kFloat &&
                ss_in->numel() % 32 == 0, "ss_in must be f32 (nstripes,32)");
    ssinp = ss_in->data_ptr<float>();
    nstripes = (int)(ss_in->numel() / 32);
  }
  float* ssoutp = nullptr;
  if (ss_out.has_value()) {
    TORCH_CHECK(ss_out->is_contiguous() && ss_out->scalar_type() == at::kFloat &&
                ss_out->numel() == (long)(N / 64) * 32,
                "ss_out must be f32 of numel (N/64)*32");
    ssoutp = ss_out->data_ptr<float>();
  }
  auto sizes = A.sizes().vec();
  sizes.back() = N;
  auto C = torch::empty(sizes, A.options());
  const unsigned short* rp = nullptr;
  if (residual.has_value()) {
    TORCH_CHECK(residual->is_contiguous() && residual->numel() == (long)M * N);
    rp = bf_ptr(*residual);
  }
  const unsigned short* bp = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_contiguous() && bias->numel() == N);
    bp = bf_ptr(*bias);
  }
  int ksplit = (int)ksplit_req;
  if (ksplit <= 0) {
    // Measured optima (benchmarks/bench_kernels.py gemm): big-N shapes are
    // BW-bound — once N/64 covers the 256 CUs extra splits only add combine
    // traffic; small-N shapes are per-block-latency-bound and want
    // (N/64)*ksplit ~ 512-1024 blocks, capped at 8.
    // BBAMD_GEMM_KSPLIT_BIG: experiment knob for the in-context latency
    // parking the PMC shows on the big MLP GEMMs (prof_ctx r2k).
    static const int ks_big = [] {
      const char* e = std::getenv("BBAMD_GEMM_KSPLIT_BIG");
      return e ? std::atoi(e) : 1;
    }();
    if (N / 64 >= 256) ksplit = ks_big;
    else ksplit = (int)std::min<long>(K / 512,
                                      std::max<long>(1, std::min<long>(8, 1024 / (N / 64))));
    ksplit = std::max(1, ksplit);
  }
  const bool v2 = (K % 256) == 0;
  int kchunk = K;
  if (v2) {
    // v2 stages 256-element chunks: round the K slice to a stage multiple and
    // drop empty trailing splits.
    const int nch = K / 256;
    const int per = (nch + ksplit - 1) / ksplit;
    ksplit = (nch + per - 1) / per;
    kchunk = per * 256;
  }
  torch::Tensor part;
  float* pp = nullptr;
  if (ksplit > 1) {
    part = torch::empty({(long)ksplit, (long)M, (long)N},
                        torch::TensorOptions().device(A.device()).dtype(at::kFloat));
    pp = part.data_ptr<float>();
  }
  int* cntp = nullptr;
  if (cnt.has_value() && ksplit > 1 && v2) {
    CHECK_DEV((*cnt));
    TORCH_CHECK(!defer_combine, "cnt and defer_combine exclude each other");
    TORCH_CHECK(cnt->scalar_type() == at::kInt && cnt->is_contiguous() &&
                cnt->numel() >= N / 64, "cnt must be int32 of >= N/64 entries");
    cntp = cnt->data_ptr<int>();
  }
  if (cntp) {
    // combine inside the launch: 1-D grid, tile = id / ksplit after the remap
    auto launch_r = [&](auto mt) {
      gemm_skinny_v2_kernel<decltype(mt)::value, 2>
          <<<dim3((N / 64) * ksplit), 256, 0, cur_stream()>>>(
              bf_ptr(A), bf_ptr(W), rp, bp, bf_ptr_mut(C), pp, M, N, K, kchunk,
              ksplit, nwp, (float)eps, norm_mode, ssinp, nstripes, ssoutp, cntp);
    };
    if (M <= 16) launch_r(std::integral_constant<int, 1>{});
    else launch_r(std::integral_constant<int, 2>{});
    return C;
  }
  dim3 grid(N / 64, ksplit);
  auto launch = [&](auto mt) {
    if (v2)
      gemm_skinny_v2_kernel<decltype(mt)::value><<<grid, 256, 0, cur_stream()>>>(
          bf_ptr(A), bf_ptr(W), ksplit == 1 ? rp : nullptr,
          ksplit == 1 ? bp : nullptr, bf_ptr_mut(C), pp, M, N, K, kchunk, ksplit,
          nwp, (float)eps, norm_mode, ssinp, nstripes,
          ksplit == 1 ? ssoutp : nullptr);
    else {
      TORCH_CHECK(!norm_mode && (!ssoutp || ksplit > 1),
                  "fused norm / ss_out need the v2 (K%256) kernel");
      gemm_skinny_kernel<decltype(mt)::value><<<grid, 256, 0, cur_stream()>>>(
          bf_ptr(A), bf_ptr(W), ksplit == 1 ? rp : nullptr,
          ksplit == 1 ? bp : nullptr, bf_ptr_mut(C), pp, M, N, K, ksplit);
    }
  };
  if (M <= 16) launch(std::integral_constant<int, 1>{});
  else launch(std::integral_constant<int, 2>{});
  if (ksplit > 1 && defer_combine) {
    TORCH_CHECK(!rp && !ssoutp, "defer_combine takes no residual / ss_out");
    return part;
  }
  if (ksplit > 1) {
    // the vectorized (float4-per-lane) combine serves both the ss-emitting
    // and plain cases; the flat grid-stride combine remains the fallback
    // for N % 64 != 0 and for narrow N where (N/64, M/16) leaves the grid
    // too small (gemma-class H=2304 -> 36 WGs)
    if (ssoutp || (N % 64 == 0 && N / 64 >= 64)) {
      dim3 cg(N / 64, (M + 15) / 16);
      gemm_skinny_combine_ss_kernel<<<cg, 256, 0, cur_stream()>>>(
          pp, rp, bp, bf_ptr_mut(C), ssoutp, M, N, ksplit);
    } else {
      const long total = (long)M * N;
      const int cgrid = (int)std::min<long>((total + 255) / 256, 2048);
      gemm_skinny_combine_kernel<<<cgrid, 256, 0, cur_stream()>>>(
          pp, rp, bp, bf_ptr_mut(C), M, N, ksplit);
    }
  }
  return C;
}

// act(M, I) = swiglu(A(M,K) @ W(2I,K)^T), W the fused gate|up weight in its
// usual layout, M <= 32: the gate_up GEMM with SwiGLU in its epilogue
// (gemm_skinny_v2_kernel<MT, 1>). norm_mode 0, or 2 (norm weight folded into
// W, per-row 1/rms from ss_in or from A). Bit-identical to
// swiglu(gemm_skinny(A, W, ...)).
torch::Tensor gemm_skinny_swiglu(torch::Tensor A, torch::Tensor W, double eps,
                                 c10::optional<torch::Tensor> ss_in,
                                 long norm_mode_req) {
  CHECK_DEV(A); CHECK_BF16(A); CHECK_CONTIG(A);
  CHECK_DEV(W); CHECK_BF16(W); CHECK_CONTIG(W);
  const int K = A.size(-1);
  const int M = A.numel() / K;
  const int N = W.size(0);
  const int I = N / 2;
  const int norm_mode = (int)norm_mode_req;
  TORCH_CHECK(M >= 1 && M <= 32, "gemm_skinny_swiglu is for 1 <= M <= 32, got ", M);
  TORCH_CHECK(W.dim() == 2 && W.size(1) == K, "A/W K mismatch");
  TORCH_CHECK(N % 2 == 0 && I % 32 == 0 && K % 256 == 0,
              "gemm_skinny_swiglu needs I % 32 == 0 and K % 256 == 0");
  TORCH_CHECK(norm_mode == 0 || norm_mode == 2, "norm_mode must be 0 or 2");
  const float* ssinp = nullptr;
  int nstripes = 0;
  if (ss_in.has_value()) {
    CHECK_DEV((*ss_in));
    TORCH_CHECK(norm_mode == 2, "ss_in only meaningful with norm_mode 2");
    TORCH_CHECK(ss_in->is_contiguous() && ss_in->scalar_type() == at::kFloat &&
                ss_in->numel() % 32 == 0, "ss_in must be f32 (nstripes,32)");
    ssinp = ss_in->data_ptr<float>();
    nstripes = (int)(ss_in->numel() / 32);
  }
  auto sizes = A.sizes().vec();
  sizes.back() = I;
  auto C = torch::empty(sizes, A.options());
  auto launch = [&](auto mt) {
    gemm_skinny_v2_kernel<decltype(mt)::value, 1>
        <<<dim3(I / 32), 256, 0, cur_stream()>>>(
            bf_ptr(A), bf_ptr(W), nullptr, nullptr, bf_ptr_mut(C), nullptr, M,
            N, K, K, 1, nullptr, (float)eps, norm_mode, ssinp, nstripes,
            nullptr, nullptr);
  };
  if (M <= 16) launch(std::integral_constant<int, 1>{});
  else launch(std::integral_constant<int, 2>{});
  return C;
}

// ---------------------------------------------------------------------------
// quant4 / selftest
// ---------------------------------------------------------------------------

std::vector<torch::Tensor> quant4_pack(torch::Tensor x) {
  CHECK_DEV(x); CHECK_BF16(x); CHECK_CONTIG(x);
  const long ncols = x.size(-1);
  TORCH_CHECK(ncols % 64 == 0, "quant4 needs cols % 64 == 0");
  const long nrows = x.numel() / ncols;
  auto packed = torch::empty({nrows, ncols / 2},
                             torch::TensorOptions().device(x.device()).dtype(at::kByte));
  auto hopt = torch::TensorOptions().device(x.device()).dtype(at::kHalf);
  auto scale = torch::empty({nrows, ncols / 64}, hopt);
  auto zero = torch::empty({nrows, ncols / 64}, hopt);
  const long ngroups = nrows * (ncols / 64);
  const int wpb = 4;  // waves per block
  quant4_pack_kernel<64><<<(ngroups + wpb - 1) / wpb, wpb * 64, 0, cur_stream()>>>(
      bf_ptr(x), packed.data_ptr<unsigned char>(),
      reinterpret_cast<__half*>(scale.data_ptr()),
      reinterpret_cast<__half*>(zero.data_ptr()), nrows, ncols);
  return {packed, scale, zero};
}

torch::Tensor quant4_unpack(torch::Tensor packed, torch::Tensor scale,
                            torch::Tensor zero) {
  CHECK_DEV(packed);
  const long nrows = packed.size(0), ncols = packed.size(1) * 2;
  auto out = torch::empty({nrows, ncols},
                          torch::TensorOptions().device(packed.device()).dtype(at::kBFloat16));
  const long total = nrows * ncols;
  const int grid = (int)std::min<long>((total + 255) / 256, 4096);
  quant4_unpack_kernel<64><<<grid, 256, 0, cur_stream()>>>(
      packed.data_ptr<unsigned char>(), reinterpret_cast<__half*>(scale.data_ptr()),
      reinterpret_cast<__half*>(zero.data_ptr()), bf_ptr_mut(out), nrows, ncols);
  return out;
}

torch::Tensor kv_stream_probe(torch::Tensor k_pages, torch::Tensor v_pages,
                              torch::Tensor page_table, torch::Tensor ctx_lens,
                              long n_split, bool nt) {
  const int B = page_table.size(0), Hkv = k_pages.size(1);
  const int P = k_pages.size(2), D = k_pages.size(3), maxp = page_table.size(1);
  auto out = torch::empty({(long)B * Hkv * n_split * 4},
                          torch::TensorOptions().device(k_pages.device()).dtype(at::kFloat));
  dim3 grid(B * Hkv, n_split);
  TORCH_CHECK(D == 128);
  if (nt)
    kv_stream_probe_kernel<128, true><<<grid, 256, 0, cur_stream()>>>(
        bf_ptr(k_pages), bf_ptr(v_pages), page_table.data_ptr<int>(),
        ctx_lens.data_ptr<int>(), out.data_ptr<float>(), B, Hkv, P, maxp,
        (int)n_split);
  else
    kv_stream_probe_kernel<128, false><<<grid, 256, 0, cur_stream()>>>(
        bf_ptr(k_pages), bf_ptr(v_pages), page_table.data_ptr<int>(),
        ctx_lens.data_ptr<int>(), out.data_ptr<float>(), B, Hkv, P, maxp,
        (int)n_split);
  return out;
}

torch::Tensor mfma_selftest(torch::Tensor A, torch::Tensor B) {
  CHECK_DEV(A); CHECK_BF16(A); CHECK_CONTIG(A); CHECK_CONTIG(B);
  TORCH_CHECK(A.size(0) == 16 && A.size(1) == 32 && B.size(0) == 32 && B.size(1) == 16);
  auto C = torch::empty({16, 16}, torch::TensorOptions().device(A.device()).dtype(at::kFloat));
  mfma_selftest_kernel<<<1, 64, 0, cur_stream()>>>(bf_ptr(A), bf_ptr(B),
                                                   C.data_ptr<float>());
  return C;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rms_norm", &rms_norm);
  m.def("rms_norm_residual", &rms_norm_residual);
  m.def("layer_norm", &layer_norm);
  m.def("rope_apply_", &rope_apply_);
  m.def("swiglu", &swiglu);
  m.def("gelu_tanh", &gelu_tanh);
  m.def("add_bf16", &add_bf16);
  m.def("kv_write", &kv_write);
  m.def("kv_gather", &kv_gather);
  m.def("wire_deflate", &wire_deflate);
  m.def("wire_inflate", &wire_inflate);
  m.def("wire_deflate_mt", &wire_deflate_mt);
  m.def("wire_inflate_mt", &wire_inflate_mt);
  m.def("attn_decode", &attn_decode);
  m.def("attn_decode_qkv", &attn_decode_qkv);
  m.def("attn_decode_mixed", &attn_decode_mixed);
  m.def("attn_decode_sparse", &attn_decode_sparse);
  m.def("attn_decode_sparse_qkv", &attn_decode_sparse_qkv);
  m.def("attn_prefill_qkv", &attn_prefill_qkv);
  m.def("rope_kv_write_", &rope_kv_write_);
  m.def("attn_prefill", &attn_prefill);
  m.def("attn_train_fwd", &attn_train_fwd);
  m.def("attn_train_bwd", &attn_train_bwd);
  m.def("gemm_skinny", &gemm_skinny, py::arg("A"), py::arg("W"),
        py::arg("residual") = c10::nullopt, py::arg("bias") = c10::nullopt,
        py::arg("ksplit") = 0, py::arg("norm_w") = c10::nullopt,
        py::arg("eps") = 0.0, py::arg("ss_in") = c10::nullopt,
        py::arg("ss_out") = c10::nullopt, py::arg("norm_mode") = 0,
        py::arg("defer_combine") = false, py::arg("cnt") = c10::nullopt);
  m.def("gemm_skinny_swiglu", &gemm_skinny_swiglu, py::arg("A"), py::arg("W"),
        py::arg("eps") = 0.0, py::arg("ss_in") = c10::nullopt,
        py::arg("norm_mode") = 0);
  m.def("rope_kv_write_part", &rope_kv_write_part);
  m.def("moe_gemm", &moe_gemm);
  m.def("gemm_w4", &gemm_w4);
  m.def("moe_gemm_w4", &moe_gemm_w4);
  m.def("quant4_pack", &quant4_pack);
  m.def("quant4_unpack", &quant4_unpack);
  m.def("mfma_selftest", &mfma_selftest);
  m.def("kv_stream_probe", &kv_stream_probe);
}
