// Checked operand access for the extension bindings (ext.hip, w8_ext.hip):
// the one way from a torch tensor to a raw kernel pointer.
#pragma once

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

static inline hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// element formats an operand can be asked for: the pointer type the kernels
// take and the torch dtype
template <typename T, at::ScalarType ST>
struct Elem {
  using type = T;
  static constexpr at::ScalarType st = ST;
};
using Bf16 = Elem<unsigned short, at::kBFloat16>;
using F16 = Elem<__half, at::kHalf>;
using F32 = Elem<float, at::kFloat>;
using I32 = Elem<int, at::kInt>;
using U8 = Elem<unsigned char, at::kByte>;
using Bool = Elem<unsigned char, at::kBool>;  // masks are read as bytes
using F8 = Elem<unsigned char, at::kFloat8_e4m3fn>;  // e4m3 pages / codes, as bytes

static const char* dtype_text(at::ScalarType st) {
  switch (st) {
    case at::kBFloat16: return "bf16";
    case at::kHalf: return "f16";
    case at::kFloat: return "f32";
    case at::kInt: return "int32";
    case at::kByte: return "u8";
    case at::kFloat8_e4m3fn: return "fp8 (e4m3)";
    default: return "bool";
  }
}

constexpr bool STRIDED = false;  // ptr(): the kernel takes this operand's strides

// The operands of one op call. A CPU tensor pointer reaching a kernel is a GPU
// memory fault at a random later point, so ptr() is the only way from a tensor
// to a raw pointer in the bindings, and it checks EVERY tensor it is given:
// on a device, on the op's device, dtype, layout. The op's first tensor names
// that device; the guard makes it current for the op's allocations and
// launches.
class Operands {
 public:
  Operands(const torch::Tensor& first, const char* name)
      : first_(name), dev_(device_of(first, name)), guard_(dev_) {}

  template <typename DT>
  typename DT::type* ptr(const torch::Tensor& t, const char* name,
                         bool contiguous = true, long numel = -1) const {
    TORCH_CHECK(t.is_cuda(), name, " must be on device");
    TORCH_CHECK(t.device() == dev_, name, " must be on the same device as ", first_);
    TORCH_CHECK(t.scalar_type() == DT::st, name, " must be ", dtype_text(DT::st));
    TORCH_CHECK(!contiguous || t.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(numel < 0 || t.numel() == numel, name, " must have ", numel,
                " elements, got ", t.numel());
    return static_cast<typename DT::type*>(t.data_ptr());
  }
  // optional operand: null when absent
  template <typename DT>
  typename DT::type* ptr(const c10::optional<torch::Tensor>& t, const char* name,
                         bool contiguous = true, long numel = -1) const {
    return t.has_value() ? ptr<DT>(*t, name, contiguous, numel) : nullptr;
  }

 private:
  static c10::Device device_of(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on device");
    return t.device();
  }
  const char* first_;
  c10::Device dev_;
  c10::DeviceGuard guard_;
};

struct SplitK {
  int ksplit, kchunk;
};

// Round a split-K request to whole `unit`-element chunks and drop the empty
// trailing splits.
static SplitK split_k_chunks(int K, int unit, int ksplit) {
  const int nch = K / unit;
  TORCH_CHECK(nch >= 1 && ksplit >= 1, "split-K needs K >= ", unit);
  const int per = (nch + ksplit - 1) / ksplit;
  return {(nch + per - 1) / per, per * unit};
}

// f32 split-K partials (ksplit, rows, N); none (null) when K is not split
struct Slabs {
  torch::Tensor t;
  float* p = nullptr;
};

static Slabs alloc_slabs(const Operands& ops, const torch::Tensor& like,
                         int ksplit, long rows, long N) {
  Slabs s;
  if (ksplit > 1) {
    s.t = torch::empty({(long)ksplit, rows, N}, like.options().dtype(at::kFloat));
    s.p = ops.ptr<F32>(s.t, "part");
  }
  return s;
}
