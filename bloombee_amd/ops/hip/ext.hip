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

static inline hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// ---------------------------------------------------------------------------
// checked operand access
// ---------------------------------------------------------------------------

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

static const char* dtype_text(at::ScalarType st) {
  switch (st) {
    case at::kBFloat16: return "bf16";
    case at::kHalf: return "f16";
    case at::kFloat: return "f32";
    case at::kInt: return "int32";
    case at::kByte: return "u8";
    default: return "bool";
  }
}

constexpr bool STRIDED = false;  // ptr(): the kernel takes this operand's strides

// The operands of one op call. A CPU tensor pointer reaching a kernel is a GPU
// memory fault at a random later point, so ptr() is the only way from a tensor
// to a raw pointer in this file, and it checks EVERY tensor it is given:
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

// A paged KV pool with its page table: K (np, Hkv, P, D) and V (np, Hkv, D, P)
// contiguous bf16, page_table (B, maxp) contiguous int32.
struct PagedKV {
  unsigned short* k;
  unsigned short* v;
  const int* pt;
  int Hkv, P, D, maxp;
};

static PagedKV paged_kv(const Operands& ops, const torch::Tensor& k_pages,
                        const torch::Tensor& v_pages,
                        const torch::Tensor& page_table) {
  PagedKV kv;
  kv.k = ops.ptr<Bf16>(k_pages, "k_pages");
  kv.v = ops.ptr<Bf16>(v_pages, "v_pages");
  kv.pt = ops.ptr<I32>(page_table, "page_table");
  TORCH_CHECK(k_pages.dim() == 4 && v_pages.dim() == 4 && page_table.dim() == 2,
              "bad KV pool / page table rank");
  kv.Hkv = k_pages.size(1), kv.P = k_pages.size(2), kv.D = k_pages.size(3);
  kv.maxp = page_table.size(1);
  return kv;
}

// What kv_write / kv_gather need beyond paged_kv(): they move 16 B (8 bf16)
// at a time along D, and index V d-major.
static void check_kv_copy_layout(const PagedKV& kv, const torch::Tensor& k_pages,
                                 const torch::Tensor& v_pages) {
  TORCH_CHECK(kv.D >= 8 && kv.D % 8 == 0, "head_dim must be a multiple of 8, got ", kv.D);
  TORCH_CHECK(v_pages.size(0) == k_pages.size(0) && v_pages.size(1) == kv.Hkv &&
                  v_pages.size(2) == kv.D && v_pages.size(3) == kv.P,
              "v_pages must be d-major (np, Hkv, D, P)");
}

// ---------------------------------------------------------------------------
// template dispatch
// ---------------------------------------------------------------------------

// f(std::integral_constant<int, D>) for the D among Ds, the head dims `op` has
// kernels for.
template <int... Ds, typename F>
static void dispatch_head_dim(int D, const char* op, F f) {
  const bool found =
      ((D == Ds ? (f(std::integral_constant<int, Ds>{}), true) : false) || ...);
  if (!found) {
    std::string dims;
    ((dims += " " + std::to_string(Ds)), ...);
    TORCH_CHECK(false, op, ": unsupported head_dim ", D, " (supported:", dims, ")");
  }
}

// f(std::integral_constant<int, MT>): 16-row M-tiles per block of the skinny
// GEMM kernels (1: M <= 16, 2: M <= 32).
template <typename F>
static void dispatch_mtile(int M, F f) {
  if (M <= 16) f(std::integral_constant<int, 1>{});
  else f(std::integral_constant<int, 2>{});
}

// ---------------------------------------------------------------------------
// split-K plans: pure host arithmetic, shared by the ops and exported to
// Python (gemm_skinny_plan / gemm_w4_plan / moe_gemm_w4_plan)
// ---------------------------------------------------------------------------

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

struct SkinnyPlan {
  int ksplit, kchunk;
  bool v2;  // K % 256 == 0: gemm_skinny_v2_kernel
};

// ksplit_req <= 0 asks for the op's own rule.
static SkinnyPlan skinny_plan(long N, long K, long ksplit_req) {
  TORCH_CHECK(N >= 64 && K >= 32 && K % 32 == 0 && N % 64 == 0,
              "K%32, N%64 required");
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
  // the v1 kernel takes ksplit alone and slices K by 32 itself
  if (K % 256 != 0)
    return {ksplit, (int)((K / 32 + ksplit - 1) / ksplit) * 32, false};
  // v2 stages 256-element chunks
  const SplitK s = split_k_chunks((int)K, 256, ksplit);
  return {s.ksplit, s.kchunk, true};
}

// W register sets gemm_skinny_v2_kernel keeps requested per wave (its DEPTH):
// a set is 4 KB per wave and DEPTH - 1 of them are outstanding at a wait.
// req > 0 pins a depth for one call, BBAMD_GEMM_WRING for the process.
// Unset, every shape runs depth 2, the kernel as it was before the ring: in
// the flagship's kernel trace depth 4 beat it for no shape (gate_up and
// o/down 3-4 % slower, qkv level; profiles/r06_gemm_wring.md), although it
// puts 84-144 KB per CU in flight where depth 2 has 28-48 KB, so there is no
// occupancy or stream-length rule to apply yet.
static constexpr int kWringDepths[] = {2, 4};

static int skinny_wring(long req) {
  static const int env = [] {
    const char* e = std::getenv("BBAMD_GEMM_WRING");
    return e ? std::atoi(e) : 0;
  }();
  if (req <= 0) req = env;
  if (req <= 0) return 2;
  TORCH_CHECK(std::find(std::begin(kWringDepths), std::end(kWringDepths), req) !=
                  std::end(kWringDepths),
              "gemm_skinny W ring depth must be 2 or 4, got ", req);
  return (int)req;
}

// Cache policy of the v2 kernel's W loads (its NT flag): nontemporal or the
// default. BBAMD_W_NT = "auto" (default) / "0" / "1" sets it for the process,
// a call's w_nt request (1: nt, -1: plain, 0: follow the process) for one
// call. "auto" is nt for exactly the (N, K, packed?) streams of kWntFaster,
// those the flagship's kernel trace showed faster with nt in every run (three
// nt runs against four plain ones, no overlap; profiles/r09_nt_weights.md has
// the figures and the noise floor), and plain for every other shape: packed
// qkv was level, packed o and every row-major stream slower. As in r06 and
// r08 a stand-alone figure does not decide for these kernels, so there is no
// rule, only the table.
struct WntShape {
  long N, K;
  bool packed;
};
static constexpr WntShape kWntFaster[] = {
    {28672, 4096, true},  // gate_up, packed: 42.0 -> 40.9 us
    {4096, 14336, true},  // down, packed: 22.5 -> 21.3 us
};

enum class WntMode { automatic, plain, nt };

static WntMode parse_w_nt(const char* e) {
  const std::string v = e ? e : "auto";
  if (v == "auto" || v.empty()) return WntMode::automatic;
  if (v == "0") return WntMode::plain;
  if (v == "1") return WntMode::nt;
  TORCH_CHECK(false, "BBAMD_W_NT must be auto, 0 or 1, got '", v, "'");
}

static bool skinny_w_nt(WntMode mode, long req, long N, long K, bool packed) {
  TORCH_CHECK(req >= -1 && req <= 1,
              "w_nt must be 0 (process setting), 1 (nt) or -1 (plain), got ", req);
  if (req != 0) return req > 0;
  if (mode != WntMode::automatic) return mode == WntMode::nt;
  for (const WntShape& s : kWntFaster)
    if (s.N == N && s.K == K && s.packed == packed) return true;
  return false;
}

static bool skinny_w_nt(long req, long N, long K, bool packed) {
  static const WntMode env = parse_w_nt(std::getenv("BBAMD_W_NT"));
  return skinny_w_nt(env, req, N, K, packed);
}

// Launches gemm_skinny_v2_kernel<MT, EPI> (depth 2) or the ring kernel at
// `depth`. `packed`: the W among args is the pre-tiled copy, which only the
// depth-2 kernel with the plain or the SwiGLU epilogue reads. `nt`: W loads
// with the nontemporal hint.
template <int MT, int EPI, bool NT, typename... Args>
static void launch_skinny_v2_nt(int depth, bool packed, dim3 grid, Args... args) {
  if constexpr (EPI != 2) {
    if (packed) {
      TORCH_CHECK(depth == 2, "packed W runs at ring depth 2 only");
      gemm_skinny_v2_kernel<MT, EPI, true, NT>
          <<<grid, 256, 0, cur_stream()>>>(args...);
      return;
    }
  }
  TORCH_CHECK(!packed, "packed W: plain and SwiGLU epilogues only");
  if (depth == 2)
    gemm_skinny_v2_kernel<MT, EPI, false, NT>
        <<<grid, 256, 0, cur_stream()>>>(args...);
  else
    gemm_skinny_v2_ring_kernel<MT, EPI, 4, NT>
        <<<grid, 256, 0, cur_stream()>>>(args...);
}

template <int MT, int EPI, typename... Args>
static void launch_skinny_v2(int depth, bool packed, bool nt, dim3 grid,
                             Args... args) {
  if (nt) launch_skinny_v2_nt<MT, EPI, true>(depth, packed, grid, args...);
  else launch_skinny_v2_nt<MT, EPI, false>(depth, packed, grid, args...);
}

struct W4Plan {
  bool gemv;
  int ksplit, kchunk;
};

static W4Plan w4_plan(long M, long N, long K, long ksplit_req) {
  TORCH_CHECK(N >= 64 && K >= 128 && K % 128 == 0 && N % 64 == 0,
              "K%128, N%64 required");
  // M==1 (the speculative-draft GEMV shape): contiguous 1 KB code loads +
  // v_dot2 — measured 2x the bf16 kernel (w4_probe.hip). A multi-row
  // (M <= 4) GEMV was measured and rejected: the split-K MFMA form wins
  // (M4 down-proj ~13 us vs 131; benchmarks/w4_probe.hip, ROUND3 item 4).
  if (M == 1 && K % 2048 == 0 && K / 2048 <= 7) return {true, 1, (int)K};
  int ksplit = (int)ksplit_req;
  if (ksplit <= 0) {
    // the w4 stream is LATENCY-bound at the bf16 kernel's grid size (1.2
    // TB/s at 448 blocks); split K until the grid reaches ~1800 blocks
    // (w4_probe.hip: ksplit=4 on N=28672 -> 2.25 TB/s, plateau beyond)
    ksplit = (int)std::max<long>(1, std::min<long>(K / 512, 1792 / (N / 64)));
  }
  // groups of 64 must not straddle splits; slices of 128 keep the k-loop
  // tail-free
  const SplitK s = split_k_chunks((int)K, 128, ksplit);
  return {false, s.ksplit, s.kchunk};
}

// The W4 stream is latency-bound below ~1800 blocks, as for gemm_w4. The host
// cannot know how many experts are active without a sync; min(E, S) bounds it.
static SplitK moe_w4_plan(long E, long N, long K, long S, long ksplit_req) {
  TORCH_CHECK(N >= 64 && K >= 128 && K % 128 == 0 && N % 64 == 0,
              "K%128, N%64 required");
  int ksplit = (int)ksplit_req;
  if (ksplit <= 0) {
    const long blocks = (N / 64) * std::max<long>(1, std::min<long>(E, S));
    ksplit = (int)std::max<long>(1, std::min<long>(K / 512, 1792 / blocks));
  }
  return split_k_chunks((int)K, 128, ksplit);
}

std::tuple<long, long, bool> gemm_skinny_plan(long N, long K, long ksplit_req) {
  const SkinnyPlan p = skinny_plan(N, K, ksplit_req);
  return {p.ksplit, p.kchunk, p.v2};
}

// The ring depth gemm_skinny (or, ksplit_req == 1, gemm_skinny_swiglu) takes
// for an (N, K) weight, 0 where the shape runs on the v1 kernel; and the
// depths the kernel is built at.
std::tuple<long, std::vector<long>> gemm_skinny_wring_plan(long N, long K,
                                                           long ksplit_req,
                                                           long wring_req) {
  const SkinnyPlan p = skinny_plan(N, K, ksplit_req);
  const std::vector<long> built(std::begin(kWringDepths), std::end(kWringDepths));
  if (!p.v2) return {0, built};
  return {skinny_wring(wring_req), built};
}

// Whether a gemm_skinny / gemm_skinny_swiglu call streams an (N, K) weight
// (packed: from its pre-tiled copy) with nontemporal loads, given the call's
// w_nt request and the process setting: `setting` as BBAMD_W_NT would spell
// it, or none for what this process read from the environment. False where
// the shape runs on the v1 kernel, which has no such flavour. With it, the
// shapes "auto" turns on, as (N, K, packed).
std::tuple<bool, std::vector<std::tuple<long, long, bool>>> gemm_skinny_nt_plan(
    long N, long K, bool packed, long w_nt_req,
    c10::optional<std::string> setting) {
  std::vector<std::tuple<long, long, bool>> table;
  for (const WntShape& s : kWntFaster) table.emplace_back(s.N, s.K, s.packed);
  const bool v2 = skinny_plan(N, K, 0).v2;
  const bool nt = setting.has_value()
                      ? skinny_w_nt(parse_w_nt(setting->c_str()), w_nt_req, N, K, packed)
                      : skinny_w_nt(w_nt_req, N, K, packed);
  return {v2 && nt, table};
}

std::tuple<bool, long, long> gemm_w4_plan(long M, long N, long K, long ksplit_req) {
  const W4Plan p = w4_plan(M, N, K, ksplit_req);
  return {p.gemv, p.ksplit, p.kchunk};
}

std::tuple<long, long> moe_gemm_w4_plan(long E, long N, long K, long S,
                                        long ksplit_req) {
  const SplitK p = moe_w4_plan(E, N, K, S, ksplit_req);
  return {p.ksplit, p.kchunk};
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

// grid of the grouped MoE kernels: (N tiles, expert x row chunk, K split)
static dim3 moe_grid(int N, long E, long mchunks, int ksplit) {
  TORCH_CHECK(mchunks >= 1 && E * mchunks <= 65535,
              "E * mchunks exceeds the grid limit");
  return dim3(N / 64, (unsigned)(E * mchunks), ksplit);
}

// ---------------------------------------------------------------------------
// norms
// ---------------------------------------------------------------------------

// The norm kernels' launch rule, for all three ops: a lane owns 16 B (8 bf16)
// of the row per iteration, so an H that is no multiple of 8 would read and
// write past the row; at most 8 iterations of 256 lanes. Raises before f runs.
template <typename F>
static void dispatch_iters(int H, F f) {
  constexpr int BLOCK = 256;
  const int per_iter = BLOCK * 8;
  TORCH_CHECK(H >= 8 && H % 8 == 0, "norm kernels need H % 8 == 0, got ", H);
  if (H <= per_iter) f(std::integral_constant<int, 1>{});
  else if (H <= 2 * per_iter) f(std::integral_constant<int, 2>{});
  else if (H <= 4 * per_iter) f(std::integral_constant<int, 4>{});
  else if (H <= 8 * per_iter) f(std::integral_constant<int, 8>{});
  else TORCH_CHECK(false, "hidden size too large for norm kernel: ", H);
}

torch::Tensor rms_norm(torch::Tensor x, torch::Tensor w, double eps) {
  Operands ops(x, "x");
  const auto* xp = ops.ptr<Bf16>(x, "x");
  const int H = x.size(-1);
  const long N = H > 0 ? x.numel() / H : 0;
  const auto* wp = ops.ptr<Bf16>(w, "w", true, H);
  auto y = torch::empty_like(x);
  auto* yp = ops.ptr<Bf16>(y, "y");
  dispatch_iters(H, [&](auto iters) {
    if (N == 0) return;  // no rows: nothing to launch
    rmsnorm_kernel<256, decltype(iters)::value><<<N, 256, 0, cur_stream()>>>(
        xp, nullptr, wp, nullptr, yp, H, (float)eps);
  });
  return y;
}

std::vector<torch::Tensor> rms_norm_residual(torch::Tensor x, torch::Tensor res,
                                             torch::Tensor w, double eps) {
  Operands ops(x, "x");
  const auto* xp = ops.ptr<Bf16>(x, "x");
  const auto* rp = ops.ptr<Bf16>(res, "res", true, x.numel());
  const int H = x.size(-1);
  const long N = H > 0 ? x.numel() / H : 0;
  const auto* wp = ops.ptr<Bf16>(w, "w", true, H);
  auto h = torch::empty_like(x);
  auto y = torch::empty_like(x);
  auto* hp = ops.ptr<Bf16>(h, "h");
  auto* yp = ops.ptr<Bf16>(y, "y");
  dispatch_iters(H, [&](auto iters) {
    if (N == 0) return;
    rmsnorm_kernel<256, decltype(iters)::value><<<N, 256, 0, cur_stream()>>>(
        xp, rp, wp, hp, yp, H, (float)eps);
  });
  return {h, y};
}

torch::Tensor layer_norm(torch::Tensor x, torch::Tensor w,
                         c10::optional<torch::Tensor> bias, double eps) {
  Operands ops(x, "x");
  const auto* xp = ops.ptr<Bf16>(x, "x");
  const int H = x.size(-1);
  const long N = H > 0 ? x.numel() / H : 0;
  const auto* wp = ops.ptr<Bf16>(w, "w", true, H);
  const auto* bp = ops.ptr<Bf16>(bias, "bias", true, H);
  auto y = torch::empty_like(x);
  auto* yp = ops.ptr<Bf16>(y, "y");
  dispatch_iters(H, [&](auto iters) {
    if (N == 0) return;
    layernorm_kernel<256, decltype(iters)::value><<<N, 256, 0, cur_stream()>>>(
        xp, nullptr, wp, bp, nullptr, yp, H, (float)eps);
  });
  return y;
}

// ---------------------------------------------------------------------------
// rope / activations
// ---------------------------------------------------------------------------

void rope_apply_(torch::Tensor q, torch::Tensor k, torch::Tensor cos_t,
                 torch::Tensor sin_t, torch::Tensor pos) {
  Operands ops(q, "q");
  auto* qp = ops.ptr<Bf16>(q, "q");
  auto* kp = ops.ptr<Bf16>(k, "k");
  const auto* cp = ops.ptr<F32>(cos_t, "cos_t");
  const auto* sp = ops.ptr<F32>(sin_t, "sin_t");
  const auto* pp = ops.ptr<I32>(pos, "pos");
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4, "rope_apply_: q and k must be (B, H, T, D)");
  const int B = q.size(0), Hq = q.size(1), T = q.size(2), D = q.size(3);
  const int Hkv = k.size(1);
  TORCH_CHECK(k.size(0) == B && k.size(2) == T && k.size(3) == D,
              "rope_apply_: k must agree with q in B, T and D");
  TORCH_CHECK(D % 2 == 0, "rope_apply_: head_dim must be even, got ", D);
  TORCH_CHECK(pos.numel() == (long)B * T, "rope_apply_: pos must have B*T = ",
              (long)B * T, " elements, got ", pos.numel());
  TORCH_CHECK(cos_t.dim() == 2 && cos_t.size(0) >= 1 && cos_t.size(1) == D / 2 &&
                  sin_t.sizes() == cos_t.sizes(),
              "rope_apply_: cos/sin must be (max_pos, D/2)");
  if ((long)B * T * (Hq + Hkv) == 0) return;
  dim3 grid(B * T, Hq + Hkv);
  rope_kernel<<<grid, 64, 0, cur_stream()>>>(qp, kp, cp, sp, pp, B, Hq, Hkv, T, D,
                                             (int)cos_t.size(0));
}

torch::Tensor swiglu(torch::Tensor gu) {
  Operands ops(gu, "gu");
  const auto* gp = ops.ptr<Bf16>(gu, "gu");
  const long I = gu.size(-1) / 2;
  TORCH_CHECK(I >= 8 && gu.size(-1) == 2 * I && I % 8 == 0,
              "swiglu needs a (..., 2I) input with I % 8 == 0");
  const long N = gu.numel() / (2 * I);
  auto sizes = gu.sizes().vec();
  sizes.back() = I;
  auto out = torch::empty(sizes, gu.options());
  const long nvec = N * (I / 8);
  if (nvec == 0) return out;
  const int grid = (int)std::min<long>((nvec + 255) / 256, 2048);
  swiglu_kernel<<<grid, 256, 0, cur_stream()>>>(gp, ops.ptr<Bf16>(out, "out"), N, I);
  return out;
}

// >= 1 block so the scalar tail (numel % 8) runs when numel < 8
static int flat_grid(long numel) {
  return (int)std::max<long>(1, std::min<long>((numel / 8 + 255) / 256, 2048));
}

torch::Tensor gelu_tanh(torch::Tensor x) {
  Operands ops(x, "x");
  const auto* xp = ops.ptr<Bf16>(x, "x");
  auto out = torch::empty_like(x);
  gelu_kernel<<<flat_grid(x.numel()), 256, 0, cur_stream()>>>(
      xp, ops.ptr<Bf16>(out, "out"), x.numel());
  return out;
}

torch::Tensor add_bf16(torch::Tensor a, torch::Tensor b) {
  Operands ops(a, "a");
  const auto* ap = ops.ptr<Bf16>(a, "a");
  const auto* bp = ops.ptr<Bf16>(b, "b");
  TORCH_CHECK(b.numel() == a.numel(), "add_bf16: numel mismatch");
  auto out = torch::empty_like(a);
  add_kernel<<<flat_grid(a.numel()), 256, 0, cur_stream()>>>(
      ap, bp, ops.ptr<Bf16>(out, "out"), a.numel());
  return out;
}

// ---------------------------------------------------------------------------
// paged KV
// ---------------------------------------------------------------------------

void kv_write(torch::Tensor k_new, torch::Tensor v_new, torch::Tensor k_pages,
              torch::Tensor v_pages, torch::Tensor page_table,
              torch::Tensor start_pos) {
  Operands ops(k_new, "k_new");
  const auto* knp = ops.ptr<Bf16>(k_new, "k_new");
  const auto* vnp = ops.ptr<Bf16>(v_new, "v_new", true, k_new.numel());
  const PagedKV kv = paged_kv(ops, k_pages, v_pages, page_table);
  check_kv_copy_layout(kv, k_pages, v_pages);
  const auto* spp = ops.ptr<I32>(start_pos, "start_pos");
  TORCH_CHECK(k_new.dim() == 4, "k_new must be (B, Hkv, T, D)");
  const int B = k_new.size(0), Hkv = k_new.size(1), T = k_new.size(2), D = k_new.size(3);
  const int P = kv.P;
  TORCH_CHECK(kv.Hkv == Hkv && kv.D == D);
  TORCH_CHECK(start_pos.numel() >= B && page_table.size(0) >= B,
              "kv_write: start_pos and page_table need a row per batch row");
  if ((long)B * T == 0) return;
  const int threads = std::min(256, Hkv * D / 8);
  kv_write_kernel<<<B * T, threads, 0, cur_stream()>>>(
      knp, vnp, kv.k, kv.v, kv.pt, spp, B, Hkv, T, D, P, kv.maxp);
}

std::vector<torch::Tensor> kv_gather(torch::Tensor k_pages, torch::Tensor v_pages,
                                     torch::Tensor page_table, long batch_index,
                                     long ctx) {
  Operands ops(k_pages, "k_pages");
  const PagedKV kv = paged_kv(ops, k_pages, v_pages, page_table);
  check_kv_copy_layout(kv, k_pages, v_pages);
  const int Hkv = kv.Hkv, D = kv.D;
  TORCH_CHECK(batch_index >= 0 && batch_index < page_table.size(0),
              "kv_gather: batch_index ", batch_index, " outside [0, ",
              page_table.size(0), ")");
  TORCH_CHECK(ctx >= 0 && ctx <= (long)kv.maxp * kv.P, "kv_gather: ctx ", ctx,
              " outside [0, maxp * P = ", (long)kv.maxp * kv.P, "]");
  auto k = torch::empty({Hkv, ctx, D}, k_pages.options());
  auto v = torch::empty({Hkv, ctx, D}, v_pages.options());
  const long nvec = ctx * Hkv * (D / 8);
  if (nvec == 0) return {k, v};
  const int grid = (int)std::min<long>((nvec + 255) / 256, 2048);
  kv_gather_kernel<<<grid, 256, 0, cur_stream()>>>(
      kv.k, kv.v, ops.ptr<Bf16>(k, "k"), ops.ptr<Bf16>(v, "v"), kv.pt,
      (int)batch_index, (int)ctx, Hkv, D, kv.P, kv.maxp);
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

// The decode kernel variants and the grid size (workgroups) at which each
// fills the chip, which is what the automatic n_split aims for — measured
// optimum (benchmarks/bench_kernels.py attn_decode); more splits only add
// merge traffic.
enum class DecodeVariant { wide, pipelined, nt2, nt1 };
struct DecodeChoice {
  DecodeVariant variant;
  long residency;
};

static DecodeChoice attn_decode_variant(int D) {
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
  // wide-head path: d split across the 4 waves (gemma-4 global layers)
  if (D == 512) return {DecodeVariant::wide, 1024};
  // 254 VGPRs -> 2 waves/SIMD -> 512 WGs fill the chip (measured: B32 ns=2
  // 50 us / 5.4 TB/s vs 59 at 768-1024 WGs)
  if (D <= 128 && pf_env) return {DecodeVariant::pipelined, 512};
  // 158 VGPRs -> 3 WGs/CU
  if (D <= 128 && nt_env >= 2) return {DecodeVariant::nt2, 768};
  // 118 VGPRs -> 4 WGs/CU
  return {DecodeVariant::nt1, 1024};
}

template <int D, int MAXG>
static auto attn_decode_kernel_for(DecodeVariant v) {
  if constexpr (D == 512) {
    return &attn_decode_wide_kernel<MAXG>;
  } else {
    switch (v) {
      case DecodeVariant::pipelined: return &attn_decode_mfma_kernel<D, MAXG, 1, 1>;
      case DecodeVariant::nt2: return &attn_decode_mfma_kernel<D, MAXG, 2>;
      default: return &attn_decode_mfma_kernel<D, MAXG, 1>;
    }
  }
}

// q is read in place through its batch / head strides (q_sb, q_sh), from
// (B, Hq, 1, D) or from the q section of a fused QKV buffer; out likewise.
static torch::Tensor attn_decode_core(
    const Operands& ops, const unsigned short* qp, const torch::Tensor& k_pages,
    const torch::Tensor& v_pages, const torch::Tensor& page_table,
    const torch::Tensor& ctx_lens, const c10::optional<torch::Tensor>& alibi,
    double scale, long window, long n_split_req,
    int B, int Hq, int D, long q_sb, long q_sh,
    torch::Tensor out, long out_sb, long out_sh,
    const MixedExt* ext = nullptr) {
  const PagedKV kv = paged_kv(ops, k_pages, v_pages, page_table);
  const int* ctxp = ops.ptr<I32>(ctx_lens, "ctx_lens");
  const float* alibi_ptr = ops.ptr<F32>(alibi, "alibi", true, Hq);
  auto* outp = ops.ptr<Bf16>(out, "out");
  const int Hkv = kv.Hkv;
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0);
  const int G = Hq / Hkv;
  TORCH_CHECK(D != 256 || G <= 4, "D=256 decode supports GQA group size <= 4");
  const int nch = (G + 15) / 16;  // MQA chunks (falcon G=71 -> 5)
  const int maxg = (G <= 4 && nch == 1) ? 4 : 16;
  const DecodeChoice choice = attn_decode_variant(D);
  int n_split = (int)n_split_req;
  if (n_split <= 0)
    n_split = (int)std::max<long>(
        1, std::min<long>(32, choice.residency / std::max(1, B * Hkv * nch)));
  // mixed-device decode: the kernels emit partials even at n_split == 1 and
  // the merge kernel folds in the host segment's partial
  const int fp = ext != nullptr ? 1 : 0;
  auto fopt = out.options().dtype(at::kFloat);
  torch::Tensor pml, pacc;
  if (n_split > 1 || fp) {
    pml = torch::empty({(long)B * Hkv * nch * n_split, maxg, 2}, fopt);
    pacc = torch::empty({(long)B * Hkv * nch * n_split, maxg, D}, fopt);
  } else {
    pml = torch::empty({1}, fopt);
    pacc = torch::empty({1}, fopt);
  }
  float* pmlp = ops.ptr<F32>(pml, "pml");
  float* paccp = ops.ptr<F32>(pacc, "pacc");
  const dim3 grid(B * Hkv * nch, n_split);
  dispatch_head_dim<128, 64, 256, 512, 32>(D, "attn_decode", [&](auto d) {
    constexpr int DD = decltype(d)::value;
    auto kernel = maxg == 4 ? attn_decode_kernel_for<DD, 4>(choice.variant)
                            : attn_decode_kernel_for<DD, 16>(choice.variant);
    kernel<<<grid, 256, 0, cur_stream()>>>(
        qp, kv.k, kv.v, kv.pt, ctxp, alibi_ptr, outp, pmlp, paccp, B, Hkv, G,
        nch, kv.P, kv.maxp, n_split, (int)window, (float)scale, q_sb, q_sh,
        out_sb, out_sh, fp);
    if (ext != nullptr) {
      attn_decode_merge_ext_kernel<DD>
          <<<B * Hkv * nch, maxg * 16, 0, cur_stream()>>>(
              pmlp, paccp, ext->ml, ext->acc, ext->dev_shift, outp, Hkv, G, nch,
              maxg, n_split, out_sb, out_sh);
    } else if (n_split > 1) {
      attn_decode_combine_kernel<DD>
          <<<B * Hkv * nch, maxg * 16, 0, cur_stream()>>>(
              pmlp, paccp, outp, Hkv, G, nch, maxg, n_split, out_sb, out_sh);
    }
  });
  return out;
}

torch::Tensor attn_decode(torch::Tensor q, torch::Tensor k_pages,
                          torch::Tensor v_pages, torch::Tensor page_table,
                          torch::Tensor ctx_lens, double scale, long window,
                          long n_split_req,
                          c10::optional<torch::Tensor> alibi) {
  Operands ops(q, "q");
  const auto* qp = ops.ptr<Bf16>(q, "q");
  TORCH_CHECK(q.dim() == 4 && q.size(2) == 1, "attn_decode expects (B, Hq, 1, D)");
  const int B = q.size(0), Hq = q.size(1), D = q.size(3);
  auto out = torch::empty({B, Hq, 1, D}, q.options());
  return attn_decode_core(ops, qp, k_pages, v_pages, page_table, ctx_lens, alibi,
                          scale, window, n_split_req, B, Hq, D,
                          (long)Hq * D, (long)D, out, (long)Hq * D, (long)D);
}

// Fused-QKV decode: q section of qkv (B, 1, (Hq+2Hkv)*D) read in place,
// out (B, 1, Hq*D) ready for the O-projection GEMM — zero transposes.
torch::Tensor attn_decode_qkv(torch::Tensor qkv, long Hq, torch::Tensor k_pages,
                              torch::Tensor v_pages, torch::Tensor page_table,
                              torch::Tensor ctx_lens, double scale, long window,
                              long n_split_req) {
  Operands ops(qkv, "qkv");
  const auto* qp = ops.ptr<Bf16>(qkv, "qkv");
  const PagedKV kv = paged_kv(ops, k_pages, v_pages, page_table);
  const int Hkv = kv.Hkv, D = kv.D;
  const int B = qkv.size(0);
  TORCH_CHECK(qkv.dim() == 3 && qkv.size(1) == 1 &&
              qkv.size(2) == (Hq + 2 * Hkv) * D, "bad fused qkv shape");
  auto out = torch::empty({B, 1, Hq * D}, qkv.options());
  return attn_decode_core(ops, qp, k_pages, v_pages, page_table, ctx_lens,
                          c10::nullopt, scale, window, n_split_req, B, (int)Hq,
                          D, (long)(Hq + 2 * Hkv) * D, (long)D,
                          out, (long)Hq * D, (long)D)
      .view({B, 1, Hq * D});
}

// ---------------------------------------------------------------------------
// Top-k sparse decode (attn_sparse.hip): scores -> select -> P.V -> combine,
// four launches on the current stream, no host sync, ctx_lens never read on
// the host (kkeep is computed on the device, so the call is graph-capturable).
static torch::Tensor attn_sparse_core(
    const Operands& ops, const unsigned short* qp, const torch::Tensor& k_pages,
    const torch::Tensor& v_pages, const torch::Tensor& page_table,
    const torch::Tensor& ctx_lens, const c10::optional<torch::Tensor>& alibi,
    double sparsity, double scale, int B, int Hq, int D, long q_sb,
    long q_sh, torch::Tensor out, long out_sb, long out_sh) {
  const PagedKV kv = paged_kv(ops, k_pages, v_pages, page_table);
  const int* ctxp = ops.ptr<I32>(ctx_lens, "ctx_lens");
  const float* alibi_ptr = ops.ptr<F32>(alibi, "alibi", true, Hq);
  auto* outp = ops.ptr<Bf16>(out, "out");
  const int Hkv = kv.Hkv, P = kv.P, maxp = kv.maxp;
  TORCH_CHECK(P == 16, "sparse decode is written for page size 16, got ", P);
  TORCH_CHECK(kv.D == D && v_pages.size(0) == k_pages.size(0) &&
              v_pages.size(1) == Hkv && v_pages.size(2) == D &&
              v_pages.size(3) == P, "K (np,Hkv,P,D) / V (np,Hkv,D,P) mismatch");
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0, "Hq must be a multiple of Hkv");
  TORCH_CHECK(page_table.size(0) == B && ctx_lens.numel() == B,
              "page_table / ctx_lens batch mismatch");
  TORCH_CHECK(B > 0 && maxp > 0, "empty batch or page table");
  const int G = Hq / Hkv;
  const int nch = (G + 15) / 16;  // MQA chunks (falcon G=71 -> 5)
  const int N = maxp * P;
  // P.V splits: ~1024 workgroups, and at least 256 positions per split
  const int n_split = (int)std::max<long>(
      1, std::min<long>(std::min<long>(32, N / 256),
                        1024 / std::max(1, B * Hkv * nch)));
  auto fopt = out.options().dtype(at::kFloat);
  auto ws = torch::empty({B, Hq, N}, fopt);
  auto lsum = torch::empty({B, Hq}, fopt);
  auto pacc = torch::empty({(long)B * Hkv * nch * n_split, 16, D}, fopt);
  float* wsp = ops.ptr<F32>(ws, "ws");
  float* lsump = ops.ptr<F32>(lsum, "lsum");
  float* paccp = ops.ptr<F32>(pacc, "pacc");
  const int BH = B * Hkv * nch;
  dispatch_head_dim<128, 64, 256>(D, "attn_decode_sparse", [&](auto d) {
    constexpr int DD = decltype(d)::value;
    attn_sparse_scores_kernel<DD>
        <<<dim3(BH, (N + 127) / 128), 256, 0, cur_stream()>>>(
            qp, kv.k, kv.pt, ctxp, alibi_ptr, wsp, Hkv, G, nch, maxp, N,
            (float)scale, q_sb, q_sh);
    attn_sparse_select_kernel<<<B * Hkv * G, 256, 0, cur_stream()>>>(
        wsp, lsump, ctxp, Hkv * G, N, sparsity);
    attn_sparse_pv_kernel<DD><<<dim3(BH, n_split), 256, 0, cur_stream()>>>(
        wsp, kv.v, kv.pt, ctxp, paccp, Hkv, G, nch, maxp, N, n_split);
    attn_sparse_combine_kernel<<<BH, 256, 0, cur_stream()>>>(
        paccp, lsump, outp, Hkv, G, nch, DD, n_split, out_sb, out_sh);
  });
  return out;
}

torch::Tensor attn_decode_sparse(torch::Tensor q, torch::Tensor k_pages,
                                 torch::Tensor v_pages, torch::Tensor page_table,
                                 torch::Tensor ctx_lens, double sparsity,
                                 double scale,
                                 c10::optional<torch::Tensor> alibi) {
  Operands ops(q, "q");
  const auto* qp = ops.ptr<Bf16>(q, "q");
  TORCH_CHECK(q.dim() == 4 && q.size(2) == 1,
              "attn_decode_sparse expects (B, Hq, 1, D)");
  const int B = q.size(0), Hq = q.size(1), D = q.size(3);
  auto out = torch::empty({B, Hq, 1, D}, q.options());
  return attn_sparse_core(ops, qp, k_pages, v_pages, page_table, ctx_lens, alibi,
                          sparsity, scale, B, Hq, D, (long)Hq * D, (long)D, out,
                          (long)Hq * D, (long)D);
}

// Fused-QKV sparse decode: q read in place from (B, 1, (Hq+2Hkv)*D), out
// (B, 1, Hq*D) in the O-projection layout.
torch::Tensor attn_decode_sparse_qkv(torch::Tensor qkv, long Hq,
                                     torch::Tensor k_pages,
                                     torch::Tensor v_pages,
                                     torch::Tensor page_table,
                                     torch::Tensor ctx_lens, double sparsity,
                                     double scale) {
  Operands ops(qkv, "qkv");
  const auto* qp = ops.ptr<Bf16>(qkv, "qkv");
  const PagedKV kv = paged_kv(ops, k_pages, v_pages, page_table);
  const int Hkv = kv.Hkv, D = kv.D;
  const int B = qkv.size(0);
  TORCH_CHECK(Hq > 0 && qkv.dim() == 3 && qkv.size(1) == 1 &&
              qkv.size(2) == (Hq + 2 * Hkv) * D, "bad fused qkv shape");
  auto out = torch::empty({B, 1, Hq * D}, qkv.options());
  return attn_sparse_core(ops, qp, k_pages, v_pages, page_table, ctx_lens,
                          c10::nullopt, sparsity, scale, B, (int)Hq, D,
                          (long)(Hq + 2 * Hkv) * D, (long)D, out,
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
  Operands ops(q, "q");
  const auto* qp = ops.ptr<Bf16>(q, "q");
  const PagedKV kv = paged_kv(ops, k_pages, v_pages, page_table);
  MixedExt ext{ops.ptr<F32>(ext_ml, "ext_ml"), ops.ptr<F32>(ext_acc, "ext_acc"),
               nullptr};
  const int Hkv = kv.Hkv, D = kv.D;
  const int B = q.size(0);
  TORCH_CHECK(ext_ml.dim() == 3 && ext_ml.size(0) == B && ext_ml.size(2) == 2,
              "ext_ml must be f32 (B, Hq, 2)");
  const int Hq = ext_ml.size(1);
  TORCH_CHECK(ext_acc.dim() == 3 && ext_acc.size(0) == B &&
              ext_acc.size(1) == Hq && ext_acc.size(2) == D,
              "ext_acc must be f32 (B, Hq, D)");
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
  if (alibi.has_value()) {
    ops.ptr<F32>(alibi, "alibi", true, Hq);
    shift = (*alibi * (double)pos_offset).contiguous();
    ext.dev_shift = ops.ptr<F32>(shift, "shift");
  }
  auto out = torch::empty({B, 1, (long)Hq * D}, q.options());
  attn_decode_core(ops, qp, k_pages, v_pages, page_table, ctx_lens, alibi, scale,
                   window, n_split_req, B, Hq, D, q_sb, (long)D,
                   out, (long)Hq * D, (long)D, &ext);
  return out;
}

// q and out are read / written in place through their (batch, token, head)
// strides: (B, Hq, Tq, D) tensors or the fused (B, Tq, heads * D) layouts.
static torch::Tensor attn_prefill_core(
    const Operands& ops, const unsigned short* qp, const torch::Tensor& k_pages,
    const torch::Tensor& v_pages, const torch::Tensor& page_table,
    const torch::Tensor& q_start, const c10::optional<torch::Tensor>& alibi,
    const c10::optional<torch::Tensor>& tree_mask, double scale, long window,
    int B, int Hq, int Tq, int D, long q_sb, long q_st, long q_sh,
    torch::Tensor out, long out_sb, long out_st, long out_sh) {
  const PagedKV kv = paged_kv(ops, k_pages, v_pages, page_table);
  const int* qsp = ops.ptr<I32>(q_start, "q_start");
  const float* alibi_ptr = ops.ptr<F32>(alibi, "alibi", true, Hq);
  const unsigned char* tm_ptr = ops.ptr<Bool>(tree_mask, "tree_mask");
  if (tree_mask.has_value()) {
    TORCH_CHECK(tree_mask->sizes() == (at::IntArrayRef{B, Tq, Tq}),
                "tree_mask must be contiguous bool (B, Tq, Tq)");
    TORCH_CHECK(window == 0, "tree_mask + sliding window: use the torch path");
  }
  auto* outp = ops.ptr<Bf16>(out, "out");
  TORCH_CHECK(kv.Hkv > 0, "empty KV pool");
  const int G = Hq / kv.Hkv;
  dim3 grid((Tq + 127) / 128, B * Hq);
  dispatch_head_dim<128, 64, 256, 32>(D, "attn_prefill", [&](auto d) {
    attn_prefill_kernel<decltype(d)::value><<<grid, 512, 0, cur_stream()>>>(
        qp, kv.k, kv.v, kv.pt, qsp, alibi_ptr, tm_ptr, outp, B, Hq, G, Tq, kv.P,
        kv.maxp, (int)window, (float)scale, q_sb, q_st, q_sh, out_sb, out_st,
        out_sh);
  });
  return out;
}

torch::Tensor attn_prefill(torch::Tensor q, torch::Tensor k_pages,
                           torch::Tensor v_pages, torch::Tensor page_table,
                           torch::Tensor q_start, double scale, long window,
                           c10::optional<torch::Tensor> alibi,
                           c10::optional<torch::Tensor> tree_mask) {
  Operands ops(q, "q");
  const auto* qp = ops.ptr<Bf16>(q, "q");
  TORCH_CHECK(q.dim() == 4, "attn_prefill expects (B, Hq, Tq, D)");
  const int B = q.size(0), Hq = q.size(1), Tq = q.size(2), D = q.size(3);
  return attn_prefill_core(
      ops, qp, k_pages, v_pages, page_table, q_start, alibi, tree_mask, scale,
      window, B, Hq, Tq, D, (long)Hq * Tq * D, (long)D, (long)Tq * D,
      torch::empty_like(q), (long)Hq * Tq * D, (long)D, (long)Tq * D);
}

// Fused-QKV prefill: q read from qkv (B, Tq, (Hq+2Hkv)*D) in place,
// out (B, Tq, Hq*D) ready for the O-projection GEMM.
torch::Tensor attn_prefill_qkv(torch::Tensor qkv, long Hq_,
                               torch::Tensor k_pages, torch::Tensor v_pages,
                               torch::Tensor page_table, torch::Tensor q_start,
                               double scale, long window) {
  Operands ops(qkv, "qkv");
  const auto* qp = ops.ptr<Bf16>(qkv, "qkv");
  const PagedKV kv = paged_kv(ops, k_pages, v_pages, page_table);
  const int Hq = (int)Hq_, D = kv.D;
  const int X = Hq + 2 * kv.Hkv;
  TORCH_CHECK(qkv.dim() == 3 && qkv.size(2) == (long)X * D, "bad fused qkv shape");
  const int B = qkv.size(0), Tq = qkv.size(1);
  return attn_prefill_core(
      ops, qp, k_pages, v_pages, page_table, q_start, c10::nullopt, c10::nullopt,
      scale, window, B, Hq, Tq, D, (long)Tq * X * D, (long)X * D, (long)D,
      torch::empty({B, Tq, (long)Hq * D}, qkv.options()), (long)Tq * Hq * D,
      (long)Hq * D, (long)D);
}

// ---------------------------------------------------------------------------
// training attention (dense K/V, LSE out, flash backward)
// ---------------------------------------------------------------------------

// (B, T, H, D) bf16 view with a contiguous last dim and 16-byte aligned rows.
static unsigned short* train_operand(const Operands& ops, const torch::Tensor& t,
                                     const char* name, long B, long T, long D) {
  auto* p = ops.ptr<Bf16>(t, name, STRIDED);
  TORCH_CHECK(t.dim() == 4 && t.size(0) == B && t.size(1) == T && t.size(3) == D,
              name, " must be (B, T, H, D) matching q");
  TORCH_CHECK(t.stride(3) == 1, name, " needs a contiguous last dim");
  TORCH_CHECK(t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0 &&
              t.stride(2) % 8 == 0 && t.storage_offset() % 8 == 0,
              name, " rows must be 16-byte aligned");
  return p;
}

struct TrainQKV {
  const unsigned short *q, *k, *v;
  long B, T, Hq, Hkv, D;
  int ntile;
};

static TrainQKV train_qkv(const Operands& ops, const torch::Tensor& q,
                          const torch::Tensor& k, const torch::Tensor& v,
                          long window) {
  TORCH_CHECK(q.dim() == 4, "attn_train expects q (B, T, Hq, D)");
  TrainQKV t;
  t.B = q.size(0), t.T = q.size(1), t.Hq = q.size(2), t.D = q.size(3);
  TORCH_CHECK(t.B > 0 && t.T > 0 && t.Hq > 0, "attn_train: empty input");
  t.q = train_operand(ops, q, "q", t.B, t.T, t.D);
  t.k = train_operand(ops, k, "k", t.B, t.T, t.D);
  t.v = train_operand(ops, v, "v", t.B, t.T, t.D);
  t.Hkv = k.size(2);
  TORCH_CHECK(t.Hkv > 0 && v.size(2) == t.Hkv && t.Hq % t.Hkv == 0,
              "attn_train: Hq must be a multiple of Hkv, and k/v must agree");
  TORCH_CHECK(window >= 0 && window < (1L << 30), "attn_train: bad window");
  const long ntile = (t.T + TR_ROWS - 1) / TR_ROWS;
  TORCH_CHECK(t.T < (1L << 30) && t.B * t.Hq * ntile < (1L << 31),
              "attn_train: grid too large");
  t.ntile = (int)ntile;
  return t;
}

std::tuple<torch::Tensor, torch::Tensor> attn_train_fwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v, double scale,
    long window, c10::optional<torch::Tensor> alibi, bool want_lse) {
  Operands ops(q, "q");
  const TrainQKV t = train_qkv(ops, q, k, v, window);
  const long B = t.B, T = t.T, Hq = t.Hq;
  const float* alibi_ptr = ops.ptr<F32>(alibi, "alibi", true, Hq);
  auto out = torch::empty({B, T, Hq, t.D}, q.options());
  auto lse = torch::empty({want_lse ? B : 0, Hq, T},
                          q.options().dtype(at::kFloat));
  auto* outp = ops.ptr<Bf16>(out, "out");
  float* lsep = want_lse ? ops.ptr<F32>(lse, "lse") : nullptr;
  const unsigned grid = (unsigned)(B * Hq * t.ntile);
  dispatch_head_dim<128, 64>((int)t.D, "attn_train", [&](auto d) {
    attn_train_fwd_kernel<decltype(d)::value><<<grid, 512, 0, cur_stream()>>>(
        t.q, t.k, t.v, alibi_ptr, outp, lsep,
        (int)Hq, (int)(Hq / t.Hkv), (int)T, t.ntile, (int)window, (float)scale,
        q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1),
        k.stride(2), v.stride(0), v.stride(1), v.stride(2));
  });
  return {out, lse};
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> attn_train_bwd(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor out, torch::Tensor lse, double scale, long window,
    c10::optional<torch::Tensor> alibi) {
  Operands ops(q, "q");
  const TrainQKV t = train_qkv(ops, q, k, v, window);
  const long B = t.B, T = t.T, Hq = t.Hq, Hkv = t.Hkv, D = t.D;
  const auto* doutp = train_operand(ops, dout, "dout", B, T, D);
  const auto* outp = train_operand(ops, out, "out", B, T, D);
  TORCH_CHECK(dout.size(2) == Hq && out.size(2) == Hq && out.is_contiguous(),
              "attn_train_bwd: dout/out must be (B, T, Hq, D), out contiguous");
  const float* lsep = ops.ptr<F32>(lse, "lse");
  TORCH_CHECK(lse.dim() == 3 && lse.size(0) == B && lse.size(1) == Hq &&
              lse.size(2) == T,
              "attn_train_bwd: lse must be contiguous f32 (B, Hq, T)");
  const float* alibi_ptr = ops.ptr<F32>(alibi, "alibi", true, Hq);
  auto dq = torch::empty({B, T, Hq, D}, q.options());
  auto dk = torch::empty({B, T, Hkv, D}, q.options());
  auto dv = torch::empty({B, T, Hkv, D}, q.options());
  auto delta = torch::empty({B, Hq, T}, lse.options());
  auto* dqp = ops.ptr<Bf16>(dq, "dq");
  auto* dkp = ops.ptr<Bf16>(dk, "dk");
  auto* dvp = ops.ptr<Bf16>(dv, "dv");
  float* deltap = ops.ptr<F32>(delta, "delta");
  const int ntile = t.ntile;
  const int G = (int)(Hq / Hkv);
  dispatch_head_dim<128, 64>((int)D, "attn_train", [&](auto d) {
    constexpr int DD = decltype(d)::value;
    // delta is written by the dQ kernel and read by the dK/dV kernel:
    // same stream, so the order is the launch order
    attn_train_dq_kernel<DD><<<(unsigned)(B * Hq * ntile), 512, 0, cur_stream()>>>(
        doutp, t.q, t.k, t.v, outp, lsep, alibi_ptr, dqp, deltap, (int)Hq, G,
        (int)T, ntile, (int)window, (float)scale,
        dout.stride(0), dout.stride(1), dout.stride(2),
        q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1),
        k.stride(2), v.stride(0), v.stride(1), v.stride(2));
    attn_train_dkdv_kernel<DD><<<(unsigned)(B * Hkv * ntile), 512, 0, cur_stream()>>>(
        doutp, t.q, t.k, t.v, lsep, deltap, alibi_ptr, dkp, dvp,
        (int)Hq, G, (int)T, ntile, (int)window, (float)scale,
        dout.stride(0), dout.stride(1), dout.stride(2),
        q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1),
        k.stride(2), v.stride(0), v.stride(1), v.stride(2));
  });
  return {dq, dk, dv};
}

// Fused RoPE + paged-KV write, on the raw QKV GEMM output (part == null:
// qkv is roped in place) or on the GEMM's uncombined split-K slabs.
static void rope_kv_write_launch(
    const Operands& ops, torch::Tensor& qkv, const float* partp, int nslab,
    const unsigned short* biasp, int* ctxp, int B, int T, int Hq, int Hkv,
    const torch::Tensor& cos_t, const torch::Tensor& sin_t,
    const c10::optional<torch::Tensor>& pos, const PagedKV& kv,
    const torch::Tensor& start_pos, long start_numel) {
  auto* qkvp = ops.ptr<Bf16>(qkv, "qkv");
  const float* cp = ops.ptr<F32>(cos_t, "cos_t");
  const float* sp = ops.ptr<F32>(sin_t, "sin_t");
  const int* posp = ops.ptr<I32>(pos, "pos", true, partp ? (long)B * T : -1);
  const int* spp = ops.ptr<I32>(start_pos, "start_pos", true, start_numel);
  if (partp) {
    // one lane per pair of 16 B groups of the row: (Hq+2Hkv)*D/8 items
    const int items = (Hq + 2 * Hkv) * (kv.D / 8);
    dim3 grid(B * T, (items + 255) / 256);
    rope_kv_write_part_kernel<<<grid, 256, 0, cur_stream()>>>(
        qkvp, partp, biasp, nslab, cp, sp, posp, kv.k, kv.v, kv.pt, spp, B, Hq,
        Hkv, T, kv.D, kv.P, kv.maxp, (int)cos_t.size(0), ctxp);
  } else {
    dim3 grid(B * T, Hq + 2 * Hkv);
    rope_kv_write_kernel<<<grid, 64, 0, cur_stream()>>>(
        qkvp, cp, sp, posp, kv.k, kv.v, kv.pt, spp, B, Hq, Hkv, T, kv.D, kv.P,
        kv.maxp, (int)cos_t.size(0));
  }
}

void rope_kv_write_(torch::Tensor qkv, long Hq_, long Hkv_, torch::Tensor cos_t,
                    torch::Tensor sin_t, c10::optional<torch::Tensor> pos,
                    torch::Tensor k_pages, torch::Tensor v_pages,
                    torch::Tensor page_table, torch::Tensor start_pos) {
  Operands ops(qkv, "qkv");
  const PagedKV kv = paged_kv(ops, k_pages, v_pages, page_table);
  const int Hq = (int)Hq_, Hkv = (int)Hkv_;
  const int B = qkv.size(0), T = qkv.size(1);
  TORCH_CHECK(qkv.size(2) == (long)(Hq + 2 * Hkv) * kv.D, "bad fused qkv shape");
  rope_kv_write_launch(ops, qkv, nullptr, 0, nullptr, nullptr, B, T, Hq, Hkv,
                       cos_t, sin_t, pos, kv, start_pos, -1);
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
  Operands ops(part, "part");
  const float* partp = ops.ptr<F32>(part, "part");
  const PagedKV kv = paged_kv(ops, k_pages, v_pages, page_table);
  const int Hq = (int)Hq_, Hkv = (int)Hkv_, B = (int)B_, T = (int)T_;
  const int D = kv.D;
  const long X = Hq + 2 * Hkv;
  TORCH_CHECK(part.dim() == 3 && part.size(1) == (long)B * T &&
              part.size(2) == X * D,
              "part must be f32 (ksplit, B*T, (Hq+2Hkv)*D)");
  TORCH_CHECK(D % 8 == 0, "rope_kv_write_part needs head_dim % 8 == 0");
  TORCH_CHECK(cos_t.dim() == 2 && cos_t.size(1) == D / 2);
  TORCH_CHECK(page_table.size(0) == B);
  const auto* bp = ops.ptr<Bf16>(bias, "bias", true, X * D);
  auto qkv = torch::empty({(long)B, (long)T, X * D},
                          k_pages.options().dtype(at::kBFloat16));
  auto ctx = torch::empty({(long)B}, start_pos.options());
  rope_kv_write_launch(ops, qkv, partp, (int)part.size(0), bp,
                       ops.ptr<I32>(ctx, "ctx"), B, T, Hq, Hkv, cos_t, sin_t,
                       pos, kv, start_pos, B);
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
  Operands ops(A, "A");
  const auto* ap = ops.ptr<Bf16>(A, "A");
  const auto* wp = ops.ptr<Bf16>(W, "W");
  TORCH_CHECK(W.dim() == 3, "W must be (E, N, K)");
  const int E = W.size(0), N = W.size(1), K = W.size(2);
  TORCH_CHECK(A.size(-1) == K, "A/W K mismatch");
  TORCH_CHECK(K % 32 == 0 && N % 64 == 0, "K%32, N%64 required");
  const int* offp = ops.ptr<I32>(off, "off", true, E + 1);
  const int* rmp = ops.ptr<I32>(rowmap, "rowmap", true, S);
  const float* sp = ops.ptr<F32>(scale, "scale", true, S);
  auto C = torch::empty({S, (long)N}, A.options());
  auto* cp = ops.ptr<Bf16>(C, "C");
  const dim3 grid = moe_grid(N, E, mchunks, 1);
  if (K % 256 == 0)
    moe_gemm_v2_kernel<2><<<grid, 256, 0, cur_stream()>>>(
        ap, wp, offp, rmp, sp, cp, N, K, (int)mchunks);
  else
    moe_gemm_kernel<2><<<grid, 256, 0, cur_stream()>>>(
        ap, wp, offp, rmp, sp, cp, N, K, (int)mchunks);
  return C;
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
  Operands ops(A, "A");
  const auto* ap = ops.ptr<Bf16>(A, "A");
  const auto* qp = ops.ptr<U8>(packed, "packed");
  const auto* scp = ops.ptr<F16>(scale, "scale");
  const auto* zp = ops.ptr<F16>(zero, "zero");
  TORCH_CHECK(packed.dim() == 3, "packed must be (E, N, K/2)");
  const int E = packed.size(0), N = packed.size(1);
  const int K = (int)packed.size(2) * 2;
  TORCH_CHECK(A.dim() == 2 && A.size(1) == K, "A/packed K mismatch");
  TORCH_CHECK(K % 128 == 0 && N % 64 == 0, "K%128, N%64 required");
  TORCH_CHECK(scale.numel() == (long)E * N * (K / 64) &&
              zero.numel() == scale.numel(), "scale/zero shape mismatch");
  const int* offp = ops.ptr<I32>(off, "off", true, E + 1);
  TORCH_CHECK(S >= 0 && mchunks >= 1 && ksplit_req >= 0);
  const int* rmp = ops.ptr<I32>(rowmap, "rowmap", true, S);
  const float* sp = ops.ptr<F32>(slot_scale, "slot_scale", true, S);
  auto C = torch::empty({S, (long)N}, A.options());
  auto* cp = ops.ptr<Bf16>(C, "C");
  if (S == 0) return C;
  const SplitK plan = moe_w4_plan(E, N, K, S, ksplit_req);
  const int ksplit = plan.ksplit;
  const Slabs part = alloc_slabs(ops, A, ksplit, S, N);
  const dim3 grid = moe_grid(N, E, mchunks, ksplit);
  moe_gemm_w4_kernel<2><<<grid, 256, 0, cur_stream()>>>(
      ap, qp, scp, zp, offp, rmp, sp, cp, part.p, (int)S, N, K, (int)mchunks,
      plan.kchunk);
  if (ksplit > 1) {
    const long total4 = S * N / 4;
    const int cgrid = (int)std::min<long>((total4 + 255) / 256, 2048);
    moe_gemm_w4_combine_kernel<<<cgrid, 256, 0, cur_stream()>>>(
        part.p, offp + E, sp, cp, (int)S, N, ksplit);
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
  Operands ops(A, "A");
  // fp16 activations: the wrapper converts
  const auto* ap = reinterpret_cast<const _Float16*>(ops.ptr<F16>(A, "A"));
  const int K = A.size(-1);
  const int M = A.numel() / K;
  const int N = (int)N_;
  TORCH_CHECK(M <= 32, "gemm_w4 is for M <= 32, got ", M);
  const auto* qp = ops.ptr<U8>(Wq, "Wq", true, (long)N * K / 2);
  const auto* scp = ops.ptr<F16>(scale, "scale", true, (long)N * K / 64);
  const auto* zp = ops.ptr<F16>(zero, "zero", true, (long)N * K / 64);
  TORCH_CHECK(K % 128 == 0 && N % 64 == 0, "K%128, N%64 required");
  const auto* rp = ops.ptr<Bf16>(residual, "residual", true, (long)M * N);
  const auto* bp = ops.ptr<Bf16>(bias, "bias", true, N);
  auto sizes = A.sizes().vec();
  sizes.back() = N;
  auto C = torch::empty(sizes, A.options().dtype(at::kBFloat16));
  auto* cp = ops.ptr<Bf16>(C, "C");
  const W4Plan plan = w4_plan(M, N, K, ksplit_req);
  if (plan.gemv) {
    const int rpw = 4;
    dim3 gv((N / rpw + 3) / 4);
    auto lv = [&](auto nl) {
      gemm_w4_gemv_kernel<decltype(nl)::value><<<gv, 256, 0, cur_stream()>>>(
          ap, qp, scp, zp, rp, bp, cp, N, K, rpw);
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
  const int ksplit = plan.ksplit;
  const Slabs part = alloc_slabs(ops, A, ksplit, M, N);
  dim3 grid(N / 64, ksplit);
  dispatch_mtile(M, [&](auto mt) {
    gemm_skinny_w4_kernel<decltype(mt)::value><<<grid, 256, 0, cur_stream()>>>(
        ap, qp, scp, zp, ksplit == 1 ? rp : nullptr, ksplit == 1 ? bp : nullptr,
        cp, part.p, M, N, K, plan.kchunk, ksplit);
  });
  if (ksplit > 1) {
    const long total = (long)M * N;
    const int cgrid = (int)std::min<long>((total + 255) / 256, 2048);
    gemm_skinny_combine_kernel<<<cgrid, 256, 0, cur_stream()>>>(
        part.p, rp, bp, cp, M, N, ksplit);
  }
  return C;
}

// ---------------------------------------------------------------------------
// skinny-M GEMM (decode projections)
// ---------------------------------------------------------------------------

// ss_in: (nstripes, 32) f32 row sum-of-squares left by the producing GEMM's
// epilogue — lets the fused rmsnorm skip re-streaming A.
static const float* ss_in_operand(const Operands& ops,
                                  const c10::optional<torch::Tensor>& ss_in,
                                  int* nstripes) {
  *nstripes = 0;
  if (!ss_in.has_value()) return nullptr;
  TORCH_CHECK(ss_in->numel() % 32 == 0, "ss_in must be f32 (nstripes,32)");
  *nstripes = (int)(ss_in->numel() / 32);
  return ops.ptr<F32>(*ss_in, "ss_in");
}

// C(M,N) = A(M,K) @ W(N,K)^T [+ residual (M,N)] [+ bias (N,)], M <= 32.
torch::Tensor gemm_skinny(torch::Tensor A, torch::Tensor W,
                          c10::optional<torch::Tensor> residual,
                          c10::optional<torch::Tensor> bias, long ksplit_req,
                          c10::optional<torch::Tensor> norm_w, double eps,
                          c10::optional<torch::Tensor> ss_in,
                          c10::optional<torch::Tensor> ss_out,
                          long norm_mode_req, bool defer_combine,
                          c10::optional<torch::Tensor> cnt, long wring_req,
                          c10::optional<torch::Tensor> w_packed, long w_nt_req) {
  // defer_combine: under split-K skip the combine and return the f32 slabs
  // (ksplit, M, N) for a consumer that folds them itself (rope_kv_write_part);
  // bias is then the consumer's to add. With ksplit == 1 there is nothing to
  // defer and the finished bf16 C comes back as usual.
  // cnt: (>= N/64,) int32 zeros — under split-K on the v2 kernel the combine
  // runs inside the GEMM launch (last-arriver reduction); the kernel leaves
  // the counters zero again.
  // wring: W ring depth of the v2 kernel for this call (skinny_wring); 0
  // leaves it to BBAMD_GEMM_WRING and the rule.
  // w_packed: W in the pre-tiled layout of common.h (identity row map),
  // streamed instead of W where the call runs the depth-2 v2 kernel with the
  // plain epilogue; every other path reads W.
  // w_nt: cache policy of the v2 kernel's W loads for this call
  // (skinny_w_nt); 0 leaves it to BBAMD_W_NT and the table. The value is
  // checked on every path; the v1 kernel (K % 256 != 0) has no nt flavour and
  // ignores a w_nt = 1, as gemm_skinny_nt_plan reports.
  Operands ops(A, "A");
  const auto* ap = ops.ptr<Bf16>(A, "A");
  const auto* wp = ops.ptr<Bf16>(W, "W");
  const int K = A.size(-1);
  const int M = A.numel() / K;
  const int N = W.size(0);
  TORCH_CHECK(M <= 32, "gemm_skinny is for M <= 32, got ", M);
  TORCH_CHECK(W.size(1) == K, "A/W K mismatch");
  TORCH_CHECK(K % 32 == 0 && N % 64 == 0, "K%32, N%64 required");
  // norm_mode: 0 none; 1 scale A by invr*norm_w per stage; 2 norm weight
  // pre-folded into W — only the invr accumulator scale remains (cheap).
  int norm_mode = (int)norm_mode_req;
  const auto* nwp = ops.ptr<Bf16>(norm_w, "norm_w", true, K);
  if (nwp && norm_mode == 0) norm_mode = 1;
  TORCH_CHECK(norm_mode != 1 || nwp, "norm_mode 1 needs norm_w");
  if (norm_mode)
    TORCH_CHECK(K % 256 == 0, "fused rmsnorm needs the v2 (K%256) kernel");
  TORCH_CHECK(!ss_in.has_value() || norm_mode != 0,
              "ss_in only meaningful with a norm mode");
  int nstripes = 0;
  const float* ssinp = ss_in_operand(ops, ss_in, &nstripes);
  float* ssoutp = ops.ptr<F32>(ss_out, "ss_out", true, (long)(N / 64) * 32);
  const auto* rp = ops.ptr<Bf16>(residual, "residual", true, (long)M * N);
  const auto* bp = ops.ptr<Bf16>(bias, "bias", true, N);
  // checked even where this call ends up not splitting K
  int* cntp = ops.ptr<I32>(cnt, "cnt");
  auto sizes = A.sizes().vec();
  sizes.back() = N;
  auto C = torch::empty(sizes, A.options());
  auto* cp = ops.ptr<Bf16>(C, "C");
  const SkinnyPlan plan = skinny_plan(N, K, ksplit_req);
  const int ksplit = plan.ksplit, kchunk = plan.kchunk;
  const Slabs part = alloc_slabs(ops, A, ksplit, M, N);
  // mode 1 scales A in registers as it stages; the ring has none to spare
  const int wring =
      !plan.v2 ? 0
      : norm_mode == 1
          ? 2
          : skinny_wring(wring_req);
  const auto* wpp = ops.ptr<Bf16>(w_packed, "w_packed", true, (long)N * K);
  if (cnt.has_value() && ksplit > 1 && plan.v2) {
    TORCH_CHECK(!defer_combine, "cnt and defer_combine exclude each other");
    TORCH_CHECK(cnt->numel() >= N / 64, "cnt must be int32 of >= N/64 entries");
    // combine inside the launch: 1-D grid, tile = id / ksplit after the remap
    dispatch_mtile(M, [&](auto mt) {
      launch_skinny_v2<decltype(mt)::value, 2>(
          wring, false, skinny_w_nt(w_nt_req, N, K, false),
          dim3((N / 64) * ksplit), ap, wp, rp, bp, cp, part.p, M,
          N, K, kchunk, ksplit, nwp, (float)eps, norm_mode, ssinp, nstripes,
          ssoutp, cntp);
    });
    return C;
  }
  dim3 grid(N / 64, ksplit);
  const bool packed = wpp && wring == 2;
  const bool nt = skinny_w_nt(w_nt_req, N, K, packed);
  dispatch_mtile(M, [&](auto mt) {
    if (plan.v2)
      launch_skinny_v2<decltype(mt)::value, 0>(
          wring, packed, nt, grid, ap, packed ? wpp : wp,
          ksplit == 1 ? rp : nullptr,
          ksplit == 1 ? bp : nullptr, cp, part.p, M, N, K, kchunk, ksplit, nwp,
          (float)eps, norm_mode, ssinp, nstripes,
          ksplit == 1 ? ssoutp : nullptr, (int*)nullptr);
    else {
      TORCH_CHECK(!norm_mode && (!ssoutp || ksplit > 1),
                  "fused norm / ss_out need the v2 (K%256) kernel");
      gemm_skinny_kernel<decltype(mt)::value><<<grid, 256, 0, cur_stream()>>>(
          ap, wp, ksplit == 1 ? rp : nullptr, ksplit == 1 ? bp : nullptr, cp,
          part.p, M, N, K, ksplit);
    }
  });
  if (ksplit > 1 && defer_combine) {
    TORCH_CHECK(!rp && !ssoutp, "defer_combine takes no residual / ss_out");
    return part.t;
  }
  if (ksplit > 1) {
    // the vectorized (float4-per-lane) combine serves both the ss-emitting
    // and plain cases; the flat grid-stride combine remains the fallback
    // for N % 64 != 0 and for narrow N where (N/64, M/16) leaves the grid
    // too small (gemma-class H=2304 -> 36 WGs)
    if (ssoutp || (N % 64 == 0 && N / 64 >= 64)) {
      dim3 cg(N / 64, (M + 15) / 16);
      gemm_skinny_combine_ss_kernel<<<cg, 256, 0, cur_stream()>>>(
          part.p, rp, bp, cp, ssoutp, M, N, ksplit);
    } else {
      const long total = (long)M * N;
      const int cgrid = (int)std::min<long>((total + 255) / 256, 2048);
      gemm_skinny_combine_kernel<<<cgrid, 256, 0, cur_stream()>>>(
          part.p, rp, bp, cp, M, N, ksplit);
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
                                 long norm_mode_req, long wring_req,
                                 c10::optional<torch::Tensor> w_packed,
                                 long w_nt_req) {
  // w_packed: W pre-tiled under the SwiGLU row map, streamed at depth 2
  // w_nt: as for gemm_skinny
  Operands ops(A, "A");
  const auto* ap = ops.ptr<Bf16>(A, "A");
  const auto* wp = ops.ptr<Bf16>(W, "W");
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
  TORCH_CHECK(!ss_in.has_value() || norm_mode == 2,
              "ss_in only meaningful with norm_mode 2");
  int nstripes = 0;
  const float* ssinp = ss_in_operand(ops, ss_in, &nstripes);
  auto sizes = A.sizes().vec();
  sizes.back() = I;
  auto C = torch::empty(sizes, A.options());
  auto* cp = ops.ptr<Bf16>(C, "C");
  const int wring = skinny_wring(wring_req);
  const auto* wpp = ops.ptr<Bf16>(w_packed, "w_packed", true, (long)N * K);
  const bool packed = wpp && wring == 2;
  const bool nt = skinny_w_nt(w_nt_req, N, K, packed);
  dispatch_mtile(M, [&](auto mt) {
    launch_skinny_v2<decltype(mt)::value, 1>(
        wring, packed, nt, dim3(I / 32), ap, packed ? wpp : wp,
        (const unsigned short*)nullptr,
        (const unsigned short*)nullptr, cp, (float*)nullptr, M, N, K, K, 1,
        (const unsigned short*)nullptr, (float)eps, norm_mode, ssinp, nstripes,
        (float*)nullptr, (int*)nullptr);
  });
  return C;
}

// ---------------------------------------------------------------------------
// quant4 / selftest
// ---------------------------------------------------------------------------

std::vector<torch::Tensor> quant4_pack(torch::Tensor x) {
  Operands ops(x, "x");
  const auto* xp = ops.ptr<Bf16>(x, "x");
  const long ncols = x.size(-1);
  TORCH_CHECK(ncols % 64 == 0, "quant4 needs cols % 64 == 0");
  const long nrows = x.numel() / ncols;
  auto packed = torch::empty({nrows, ncols / 2}, x.options().dtype(at::kByte));
  auto scale = torch::empty({nrows, ncols / 64}, x.options().dtype(at::kHalf));
  auto zero = torch::empty_like(scale);
  const long ngroups = nrows * (ncols / 64);
  if (ngroups == 0) return {packed, scale, zero};
  const int wpb = 4;  // waves per block
  quant4_pack_kernel<64><<<(ngroups + wpb - 1) / wpb, wpb * 64, 0, cur_stream()>>>(
      xp, ops.ptr<U8>(packed, "packed"), ops.ptr<F16>(scale, "scale"),
      ops.ptr<F16>(zero, "zero"), nrows, ncols);
  return {packed, scale, zero};
}

torch::Tensor quant4_unpack(torch::Tensor packed, torch::Tensor scale,
                            torch::Tensor zero) {
  Operands ops(packed, "packed");
  auto* qp = ops.ptr<U8>(packed, "packed");
  TORCH_CHECK(packed.dim() == 2, "packed must be (rows, cols/2)");
  const long nrows = packed.size(0), ncols = packed.size(1) * 2;
  TORCH_CHECK(ncols % 64 == 0, "quant4 needs cols % 64 == 0");
  auto* scp = ops.ptr<F16>(scale, "scale", true, nrows * (ncols / 64));
  auto* zp = ops.ptr<F16>(zero, "zero", true, nrows * (ncols / 64));
  auto out = torch::empty({nrows, ncols}, packed.options().dtype(at::kBFloat16));
  const long total = nrows * ncols;
  if (total == 0) return out;
  const int grid = (int)std::min<long>((total + 255) / 256, 4096);
  quant4_unpack_kernel<64><<<grid, 256, 0, cur_stream()>>>(
      qp, scp, zp, ops.ptr<Bf16>(out, "out"), nrows, ncols);
  return out;
}

torch::Tensor kv_stream_probe(torch::Tensor k_pages, torch::Tensor v_pages,
                              torch::Tensor page_table, torch::Tensor ctx_lens,
                              long n_split, bool nt) {
  Operands ops(k_pages, "k_pages");
  const PagedKV kv = paged_kv(ops, k_pages, v_pages, page_table);
  const int B = page_table.size(0), Hkv = kv.Hkv;
  const int* ctxp = ops.ptr<I32>(ctx_lens, "ctx_lens", true, B);
  TORCH_CHECK(kv.D == 128 && n_split >= 1);
  auto out = torch::empty({(long)B * Hkv * n_split * 4},
                          k_pages.options().dtype(at::kFloat));
  float* outp = ops.ptr<F32>(out, "out");
  dim3 grid(B * Hkv, n_split);
  auto kernel = nt ? &kv_stream_probe_kernel<128, true>
                   : &kv_stream_probe_kernel<128, false>;
  kernel<<<grid, 256, 0, cur_stream()>>>(kv.k, kv.v, kv.pt, ctxp, outp, B, Hkv,
                                         kv.P, kv.maxp, (int)n_split);
  return out;
}

torch::Tensor mfma_selftest(torch::Tensor A, torch::Tensor B) {
  Operands ops(A, "A");
  const auto* ap = ops.ptr<Bf16>(A, "A");
  const auto* bp = ops.ptr<Bf16>(B, "B");
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && A.size(0) == 16 &&
              A.size(1) == 32 && B.size(0) == 32 && B.size(1) == 16);
  auto C = torch::empty({16, 16}, A.options().dtype(at::kFloat));
  mfma_selftest_kernel<<<1, 64, 0, cur_stream()>>>(ap, bp, ops.ptr<F32>(C, "C"));
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
        py::arg("defer_combine") = false, py::arg("cnt") = c10::nullopt,
        py::arg("wring") = 0, py::arg("w_packed") = c10::nullopt,
        py::arg("w_nt") = 0);
  m.def("gemm_skinny_swiglu", &gemm_skinny_swiglu, py::arg("A"), py::arg("W"),
        py::arg("eps") = 0.0, py::arg("ss_in") = c10::nullopt,
        py::arg("norm_mode") = 0, py::arg("wring") = 0,
        py::arg("w_packed") = c10::nullopt, py::arg("w_nt") = 0);
  m.def("gemm_skinny_plan", &gemm_skinny_plan);
  m.def("gemm_skinny_nt_plan", &gemm_skinny_nt_plan, py::arg("N"), py::arg("K"),
        py::arg("packed") = false, py::arg("w_nt") = 0,
        py::arg("setting") = c10::nullopt);
  m.def("gemm_skinny_wring_plan", &gemm_skinny_wring_plan, py::arg("N"),
        py::arg("K"), py::arg("ksplit") = 0, py::arg("wring") = 0);
  m.def("rope_kv_write_part", &rope_kv_write_part);
  m.def("moe_gemm", &moe_gemm);
  m.def("gemm_w4", &gemm_w4);
  m.def("gemm_w4_plan", &gemm_w4_plan);
  m.def("moe_gemm_w4", &moe_gemm_w4);
  m.def("moe_gemm_w4_plan", &moe_gemm_w4_plan);
  m.def("quant4_pack", &quant4_pack);
  m.def("quant4_unpack", &quant4_unpack);
  m.def("mfma_selftest", &mfma_selftest);
  m.def("kv_stream_probe", &kv_stream_probe);
}
