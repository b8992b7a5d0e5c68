// Torch bindings of the ring-attention fold (attn_ring.hip). A module of its
// own (_hip_ring); pointers go through the same Operands::ptr as every other
// binding (operands.h).

#include "operands.h"
#include "common.h"
#include "attn_ring.hip"

// (B, H, rows, D) bf16 through its strides: last dim contiguous, every row
// 16-byte aligned.
static const unsigned short* ring_operand(const Operands& ops,
                                          const torch::Tensor& t,
                                          const char* name, long B, long D) {
  const auto* p = ops.ptr<Bf16>(t, name, STRIDED);
  TORCH_CHECK(t.dim() == 4 && t.size(0) == B && t.size(3) == D, name,
              " must be (B, H, rows, D) matching q");
  TORCH_CHECK(t.size(1) >= 1 && t.size(2) >= 1, name, " is empty");
  TORCH_CHECK(t.stride(3) == 1, name, " needs a contiguous last dim");
  TORCH_CHECK(t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0 &&
                  t.stride(2) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(p) % 16 == 0,
              name, " rows must be 16-byte aligned");
  return p;
}

// One ring step. q (B, Hq, T, D), k/v (B, Hkv, S, D) bf16 views; state absent
// (first fold) or acc (B, Hq, T, D) + ml (B, Hq, T, 2) f32 as an earlier call
// returned them. rel = k_pos0 - q_pos0. Returns {acc, ml}, or with `last`
// {out (B, T, Hq, D) bf16}.
std::vector<torch::Tensor> attn_ring_fold(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    c10::optional<torch::Tensor> acc_in, c10::optional<torch::Tensor> ml_in,
    long rel, double scale, long window, bool last) {
  Operands ops(q, "q");
  TORCH_CHECK(q.dim() == 4, "attn_ring_fold expects q (B, Hq, T, D)");
  const long B = q.size(0), Hq = q.size(1), T = q.size(2), D = q.size(3);
  TORCH_CHECK(D == 64 || D == 128, "attn_ring_fold: head dim must be 64 or 128, got ", D);
  TORCH_CHECK(B >= 1, "attn_ring_fold: empty batch");
  const auto* qp = ring_operand(ops, q, "q", B, D);
  const auto* kp = ring_operand(ops, k, "k", B, D);
  const auto* vp = ring_operand(ops, v, "v", B, D);
  const long Hkv = k.size(1), S = k.size(2);
  TORCH_CHECK(v.size(1) == Hkv && v.size(2) == S && Hq % Hkv == 0,
              "attn_ring_fold: Hq must be a multiple of Hkv, and k/v must agree");
  const long G = Hq / Hkv;
  const long lim = 1L << 30;
  TORCH_CHECK(T < lim && S < lim && window >= 0 && window < lim && rel > -lim &&
                  rel < lim,
              "attn_ring_fold: positions out of range");
  const long ntile = (G * T + RG_ROWS - 1) / RG_ROWS;
  TORCH_CHECK(B * Hkv * ntile < (1L << 31), "attn_ring_fold: grid too large");

  TORCH_CHECK(acc_in.has_value() == ml_in.has_value(),
              "attn_ring_fold: state is acc and ml together");
  const float *ain = nullptr, *min_ = nullptr;
  if (acc_in.has_value()) {
    ain = ops.ptr<F32>(*acc_in, "state acc", true, B * Hq * T * D);
    min_ = ops.ptr<F32>(*ml_in, "state ml", true, B * Hq * T * 2);
    TORCH_CHECK(acc_in->sizes() == at::IntArrayRef({B, Hq, T, D}) &&
                    ml_in->sizes() == at::IntArrayRef({B, Hq, T, 2}),
                "attn_ring_fold: state must be acc (B, Hq, T, D), ml (B, Hq, T, 2)");
  }

  std::vector<torch::Tensor> ret;
  float *aout = nullptr, *mout = nullptr;
  unsigned short* outp = nullptr;
  if (last) {
    ret.push_back(torch::empty({B, T, Hq, D}, q.options()));
    outp = ops.ptr<Bf16>(ret[0], "out");
  } else {
    ret.push_back(torch::empty({B, Hq, T, D}, q.options().dtype(at::kFloat)));
    ret.push_back(torch::empty({B, Hq, T, 2}, q.options().dtype(at::kFloat)));
    aout = ops.ptr<F32>(ret[0], "acc");
    mout = ops.ptr<F32>(ret[1], "ml");
  }

  const unsigned grid = (unsigned)(B * Hkv * ntile);
  auto launch = [&](auto d) {
    attn_ring_fold_kernel<decltype(d)::value><<<grid, RG_THREADS, 0, cur_stream()>>>(
        qp, kp, vp, ain, min_, aout, mout, outp, (int)Hq, (int)G, (int)T, (int)S,
        (int)ntile, (int)rel, (int)window, (float)scale, last ? 1 : 0,
        q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1),
        k.stride(2), v.stride(0), v.stride(1), v.stride(2));
  };
  if (D == 128) launch(std::integral_constant<int, 128>{});
  else launch(std::integral_constant<int, 64>{});
  return ret;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("attn_ring_fold", &attn_ring_fold, py::arg("q"), py::arg("k"),
        py::arg("v"), py::arg("acc"), py::arg("ml"), py::arg("rel"),
        py::arg("scale"), py::arg("window") = 0, py::arg("last") = false);
}
