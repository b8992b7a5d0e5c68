// Torch bindings of the fp8 (e4m3) weight tier: the row quantiser, the decode
// GEMM (gemm_w8.hip), the tiled GEMM above 32 rows (gemm_w8_tiled.hip) and
// their plans. A module of its own
// (_hip_w8), built without packed-fp32 instructions; pointers go through the
// same Operands::ptr as every other binding (operands.h).

#include "operands.h"
#include "common.h"
#include "gemm_w8.hip"
#include "gemm_w8_tiled.hip"

// ksplit_req <= 0 asks for the op's own rule. Splits are whole 128-k tiles.
static SplitK w8_plan(long N, long K, long ksplit_req) {
  TORCH_CHECK(N >= 64 && K >= 128 && K % 128 == 0 && N % 64 == 0,
              "gemm_w8: K%128, N%64 required");
  int ksplit = (int)ksplit_req;
  if (ksplit <= 0) {
    // Measured on the four llama-3-8b projections (profiles/r13_w8_gemm.md):
    // unsplit wins wherever K = 4096, whatever the stripe count (64 .. 448);
    // only down (64 stripes, K = 14336) gains from splitting, and 4 splits
    // beat 2, 8 and 14. So a split keeps at least 28 tiles (3584 k, 3.5 turns
    // of the ring) and the grid stays within one workgroup per CU.
    ksplit = (int)std::max<long>(
        1, std::min<long>(K / 3584, 256 / std::min<long>(256, N / 64)));
  }
  return split_k_chunks((int)K, 128, ksplit);
}

std::tuple<long, long> gemm_w8_plan(long N, long K, long ksplit_req) {
  const SplitK p = w8_plan(N, K, ksplit_req);
  return {p.ksplit, p.kchunk};
}

// Cache policy of the W stream: w_nt 1 nontemporal, -1 plain, 0 the rule.
// The rule is nontemporal: at the plan's split it measured faster on all four
// llama-3-8b projections at M = 1, 8 and 32 (profiles/r13_w8_gemm.md).
static bool w8_nt(long req) {
  TORCH_CHECK(req >= -1 && req <= 1, "w_nt must be 0, 1 or -1, got ", req);
  return req >= 0;
}

// x (..., K) bf16 -> a8 (..., K) e4m3, a_scale (rows,) f32
std::vector<torch::Tensor> quant_rows_fp8(torch::Tensor x) {
  Operands ops(x, "x");
  const auto* xp = ops.ptr<Bf16>(x, "x");
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) >= 8 && x.size(-1) % 8 == 0,
              "quant_rows_fp8 needs K % 8 == 0");
  const int K = x.size(-1);
  const long M = x.numel() / K;
  TORCH_CHECK(M >= 1 && M <= INT_MAX, "quant_rows_fp8 takes >= 1 rows, got ", M);
  auto a8 = torch::empty(x.sizes(), x.options().dtype(at::kFloat8_e4m3fn));
  auto a_scale = torch::empty({M}, x.options().dtype(at::kFloat));
  quant_rows_fp8_kernel<<<(unsigned)M, 256, 0, cur_stream()>>>(
      xp, ops.ptr<F8>(a8, "a8"), ops.ptr<F32>(a_scale, "a_scale"), K);
  return {a8, a_scale};
}

// C (..., N) bf16 = a_scale * w_scale * (a8 @ codes^T) [+bias] [+residual];
// Wp: the codes of (N, K) in pack_w8 order.
torch::Tensor gemm_w8(torch::Tensor a8, torch::Tensor a_scale, torch::Tensor Wp,
                      torch::Tensor w_scale,
                      c10::optional<torch::Tensor> residual,
                      c10::optional<torch::Tensor> bias, long N_,
                      long ksplit_req, long w_nt) {
  Operands ops(a8, "a8");
  const auto* ap = ops.ptr<F8>(a8, "a8");
  TORCH_CHECK(a8.dim() >= 1 && a8.size(-1) >= 128, "gemm_w8: K%128, N%64 required");
  const int K = a8.size(-1);
  const long M = a8.numel() / K;
  const int N = (int)N_;
  TORCH_CHECK(M >= 1 && M <= 32, "gemm_w8 takes 1..32 rows, got ", M);
  const SplitK plan = w8_plan(N, K, ksplit_req);
  const auto* asp = ops.ptr<F32>(a_scale, "a_scale", true, M);
  const auto* wp = ops.ptr<F8>(Wp, "Wp", true, (long)N * K);
  const auto* wsp = ops.ptr<F32>(w_scale, "w_scale", true, N);
  const auto* rp = ops.ptr<Bf16>(residual, "residual", true, M * N);
  const auto* bp = ops.ptr<Bf16>(bias, "bias", true, N);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(ap) | reinterpret_cast<uintptr_t>(wp)) % 16 == 0,
              "gemm_w8: a8 and Wp must be 16 B aligned");
  auto sizes = a8.sizes().vec();
  sizes.back() = N;
  auto C = torch::empty(sizes, a8.options().dtype(at::kBFloat16));
  auto* cp = ops.ptr<Bf16>(C, "C");
  const int ksplit = plan.ksplit;
  const Slabs part = alloc_slabs(ops, a8, ksplit, M, N);
  const bool nt = w8_nt(w_nt);
  const dim3 grid(N / 64, ksplit);
  auto launch = [&](auto mt, auto ntc) {
    gemm_w8_kernel<decltype(mt)::value, decltype(ntc)::value>
        <<<grid, 256, 0, cur_stream()>>>(
            ap, wp, asp, wsp, ksplit == 1 ? rp : nullptr,
            ksplit == 1 ? bp : nullptr, cp, part.p, (int)M, N, K, plan.kchunk);
  };
  using One = std::integral_constant<int, 1>;
  using Two = std::integral_constant<int, 2>;
  if (M <= 16) nt ? launch(One{}, std::true_type{}) : launch(One{}, std::false_type{});
  else nt ? launch(Two{}, std::true_type{}) : launch(Two{}, std::false_type{});
  if (ksplit > 1) {
    const int cgrid = (int)std::min<long>((M * N + 255) / 256, 2048);
    gemm_w8_combine_kernel<<<cgrid, 256, 0, cur_stream()>>>(
        part.p, asp, wsp, rp, bp, cp, (int)M, N, ksplit);
  }
  return C;
}

// gemm_w8 above 32 rows (gemm_w8_tiled.hip): block tile BM x 128.
struct W8TiledPlan {
  int BM, mtiles, ksplit, kchunk;
};

static W8TiledPlan w8_tiled_plan(long M, long N, long K, long ksplit_req) {
  TORCH_CHECK(N >= 64 && K >= 128 && K % 128 == 0 && N % 64 == 0,
              "gemm_w8_tiled: K%128, N%64 required");
  TORCH_CHECK(M > 32 && M <= INT_MAX / 2,
              "the tiled W8 kernel is for M > 32, got ", M);
  // the smaller tile where it cuts padded rows (M 33..64, 129..192, ...)
  const int BM = (M + 127) / 128 * 128 <= (M + 63) / 64 * 64 ? 128 : 64;
  const long mtiles = (M + BM - 1) / BM;
  TORCH_CHECK(((N + 127) / 128) * mtiles <= INT_MAX, "gemm_w8_tiled: grid too large");
  int ksplit = (int)ksplit_req;
  if (ksplit <= 0) {
    // Measured at forced splits 1, 2, 4, 8 on the four llama-3-8b
    // projections, M 64..4096 (profiles/r14_w8_tiled.md): splitting pays
    // until there is one block tile per CU, with splits of >= 512 k and at
    // most 8 slabs; down (K = 14336) still gains up to two block tiles per
    // CU as long as a split keeps 3584 k (M 512: 4 splits, M 1024: 2); from
    // 2 M N / 128^2 >= 512 block tiles on, unsplit wins everywhere.
    const long blocks = ((N + 127) / 128) * mtiles;
    ksplit = (int)std::max<long>(
        1, std::min<long>(8, std::max(std::min<long>(K / 512, 256 / blocks),
                                      std::min<long>(K / 3584, 512 / blocks))));
  }
  const SplitK s = split_k_chunks((int)K, 128, ksplit);
  return {BM, (int)mtiles, s.ksplit, s.kchunk};
}

std::tuple<long, long, long, long> gemm_w8_tiled_plan(long M, long N, long K,
                                                      long ksplit_req) {
  const W8TiledPlan p = w8_tiled_plan(M, N, K, ksplit_req);
  return {p.BM, p.mtiles, p.ksplit, p.kchunk};
}

// gemm_w8 for M >= 33: same operands, same result layout.
torch::Tensor gemm_w8_tiled(torch::Tensor a8, torch::Tensor a_scale,
                            torch::Tensor Wp, torch::Tensor w_scale,
                            c10::optional<torch::Tensor> residual,
                            c10::optional<torch::Tensor> bias, long N_,
                            long ksplit_req) {
  Operands ops(a8, "a8");
  const auto* ap = ops.ptr<F8>(a8, "a8");
  TORCH_CHECK(a8.dim() >= 1 && a8.size(-1) >= 128,
              "gemm_w8_tiled: K%128, N%64 required");
  const int K = a8.size(-1);
  const long M = a8.numel() / K;
  const int N = (int)N_;
  const W8TiledPlan plan = w8_tiled_plan(M, N, K, ksplit_req);
  const auto* asp = ops.ptr<F32>(a_scale, "a_scale", true, M);
  const auto* wp = ops.ptr<F8>(Wp, "Wp", true, (long)N * K);
  const auto* wsp = ops.ptr<F32>(w_scale, "w_scale", true, N);
  const auto* rp = ops.ptr<Bf16>(residual, "residual", true, M * N);
  const auto* bp = ops.ptr<Bf16>(bias, "bias", true, N);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(ap) | reinterpret_cast<uintptr_t>(wp)) % 16 == 0,
              "gemm_w8_tiled: a8 and Wp must be 16 B aligned");
  auto sizes = a8.sizes().vec();
  sizes.back() = N;
  auto C = torch::empty(sizes, a8.options().dtype(at::kBFloat16));
  auto* cp = ops.ptr<Bf16>(C, "C");
  const int ksplit = plan.ksplit;
  const Slabs part = alloc_slabs(ops, a8, ksplit, M, N);
  const dim3 grid((unsigned)(((N + 127) / 128) * plan.mtiles), ksplit);
  auto launch = [&](auto bm) {
    gemm_w8_tiled_kernel<decltype(bm)::value><<<grid, 256, 0, cur_stream()>>>(
        ap, wp, asp, wsp, ksplit == 1 ? rp : nullptr,
        ksplit == 1 ? bp : nullptr, cp, part.p, (int)M, N, K, plan.mtiles,
        plan.kchunk);
  };
  if (plan.BM == 64) launch(std::integral_constant<int, 64>{});
  else launch(std::integral_constant<int, 128>{});
  if (ksplit > 1) {
    const int cgrid = (int)std::min<long>((M * N + 255) / 256, 2048);
    gemm_w8_combine_kernel<<<cgrid, 256, 0, cur_stream()>>>(
        part.p, asp, wsp, rp, bp, cp, (int)M, N, ksplit);
  }
  return C;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("quant_rows_fp8", &quant_rows_fp8);
  m.def("gemm_w8", &gemm_w8, py::arg("a8"), py::arg("a_scale"), py::arg("Wp"),
        py::arg("w_scale"), py::arg("residual"), py::arg("bias"), py::arg("N"),
        py::arg("ksplit") = 0, py::arg("w_nt") = 0);
  m.def("gemm_w8_plan", &gemm_w8_plan);
  m.def("gemm_w8_tiled", &gemm_w8_tiled, py::arg("a8"), py::arg("a_scale"),
        py::arg("Wp"), py::arg("w_scale"), py::arg("residual"), py::arg("bias"),
        py::arg("N"), py::arg("ksplit") = 0);
  m.def("gemm_w8_tiled_plan", &gemm_w8_tiled_plan);
}
