// Torch bindings for the g2vec_amd gfx950 kernels + native host utilities.
// One translation unit: kernels are included below.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdio>
#include <functional>
#include <initializer_list>
#include <optional>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <type_traits>
#include <vector>

#include "g2vec_kernels.hip"

namespace {

// Every tensor a kernel dereferences passes one of these first: on the GPU,
// contiguous, and (CHECK_F32 / CHECK_I32 / CHECK_F64) of the dtype its
// pointer is taken as. The message names the argument.
inline void check_gpu_cont(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on the GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}
inline void check_f32(const torch::Tensor& t, const char* name) {
  check_gpu_cont(t, name);
  TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be float32");
}
inline void check_i32(const torch::Tensor& t, const char* name) {
  check_gpu_cont(t, name);
  TORCH_CHECK(t.scalar_type() == at::kInt, name, " must be int32");
}
inline void check_f64(const torch::Tensor& t, const char* name) {
  check_gpu_cont(t, name);
  TORCH_CHECK(t.scalar_type() == at::kDouble, name, " must be float64");
}
// the row-tile kernels move rows as 16-byte pieces
inline void check_rows16(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              " must be 16-byte aligned");
}
#define CHECK_GPU_CONT(x) check_gpu_cont((x), #x)
#define CHECK_F32(x) check_f32((x), #x)
#define CHECK_I32(x) check_i32((x), #x)
#define CHECK_F64(x) check_f64((x), #x)
#define CHECK_ROWS16(x) check_rows16((x), #x)

// Every entry point with more than one tensor calls this directly after its
// dtype checks: the launch goes to the current stream with raw pointers, so
// a tensor of another GPU would be dereferenced on the wrong device.
inline void check_same_device(
    const torch::Tensor& first,
    std::initializer_list<std::reference_wrapper<const torch::Tensor>> others) {
  for (const torch::Tensor& t : others)
    TORCH_CHECK(t.device() == first.device(),
                "all tensors must be on one device, got ", first.device(),
                " and ", t.device());
}

// A tensor size or user integer that a kernel receives as a 32-bit int goes
// through here first: a value that does not fit is refused by name instead
// of reaching the launch truncated. Called before any allocation or launch.
inline int int_arg(long long v, const char* name) {
  TORCH_CHECK(v >= 0 && v <= (long long)INT_MAX, name,
              " must be in [0, 2^31), got ", v);
  return (int)v;
}

// The MFMA bodies are compiled only for gfx950: elsewhere the launch would be
// a no-op leaving the outputs unwritten (the rank kernels are tuned and
// tested for gfx950 alone and refuse other devices the same way).
inline void check_gfx950(const char* op, const char* what = "MFMA kernel") {
  hipDeviceProp_t prop;
  int dev = 0;
  (void)hipGetDevice(&dev);
  (void)hipGetDeviceProperties(&prop, dev);
  TORCH_CHECK(std::string(prop.gcnArchName).rfind("gfx950", 0) == 0, op,
              ": ", what, " is gfx950-only, device reports ",
              prop.gcnArchName);
}

inline int cu_count(const char* op) {
  int n_cu = 0, dev = 0;
  TORCH_CHECK(hipGetDevice(&dev) == hipSuccess &&
                  hipDeviceGetAttribute(&n_cu,
                                        hipDeviceAttributeMultiprocessorCount,
                                        dev) == hipSuccess && n_cu >= 1,
              op, ": cannot read the device's CU count");
  return n_cu;
}

// the Adam kernels give each thread 4 columns of a row, whole rows per block
inline void check_adam_hidden(int h) {
  TORCH_CHECK(h >= 4 && h % 4 == 0 && 256 % (h / 4) == 0 && h <= 1024,
              "hidden must be a multiple of 4 with h/4 dividing 256");
}

inline torch::TensorOptions opts_on(const torch::Tensor& t,
                                    at::ScalarType dtype = at::kFloat) {
  return torch::TensorOptions().dtype(dtype).device(t.device());
}

// The pointer a kernel receives; f32 of an absent optional is nullptr.
inline float* f32(const torch::Tensor& t) { return t.data_ptr<float>(); }
inline float* f32(const std::optional<torch::Tensor>& t) {
  return t ? f32(*t) : nullptr;
}
inline int* i32(const torch::Tensor& t) { return t.data_ptr<int>(); }
inline double* f64(const torch::Tensor& t) { return t.data_ptr<double>(); }
inline uint8_t* u8(const torch::Tensor& t) { return t.data_ptr<uint8_t>(); }

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// THE launch: 256 threads on the current stream, each argument converted to
// the kernel's parameter type, and the launch status read (LAUNCH_CHECK)
// before anything else runs.
template <typename... KA, typename... A>
void launch(void (*k)(KA...), dim3 grid, size_t lds, A&&... a) {
  static_assert(sizeof...(KA) == sizeof...(A), "kernel argument count");
  hipLaunchKernelGGL(k, grid, dim3(256), lds, cur_stream(),
                     static_cast<KA>(a)...);
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "HIP launch failed: ",
              hipGetErrorString(err));
}

// Blocks for work_items at per_block each: at least 1, at most cap, and never
// past GRID_MAX (the kernels grid-stride over the rest).
constexpr long long GRID_MAX = 1 << 20;
inline int grid_for(long long work_items, int per_block,
                    long long cap = GRID_MAX) {
  long long blocks = (work_items + per_block - 1) / per_block;
  if (blocks > GRID_MAX) blocks = GRID_MAX;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}
// one row per wave (4 per block), at most the 8192 blocks that fill the chip
inline int row_wave_grid(long long rows) { return grid_for(rows, 4, 8192); }

// Integer env knob with a default, read on EVERY call (the tests flip the
// knobs inside one process). Clamped to >= 1: a malformed value must not
// 0-block-launch.
inline int env_int_min1(const char* name, int dflt) {
  const char* e = getenv(name);
  const int v = e ? atoi(e) : dflt;
  return v < 1 ? 1 : v;
}

// Template-parameter dispatch: f is a generic lambda called with a
// std::integral_constant, so f's body names the kernel instantiation once.
// hpl = hidden / 64 columns per lane (gather/GEMV kernels), validated here.
inline int hpl_for(int h) {
  const int hpl = h / 64;
  TORCH_CHECK(h % 64 == 0 && hpl >= 1 && hpl <= 16 && (hpl & (hpl - 1)) == 0,
              "hidden must be 64*{1,2,4,8,16}");
  return hpl;
}

template <typename F>
void dispatch_hpl(int hpl, F&& f) {
  switch (hpl) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    default: f(std::integral_constant<int, 16>{}); break;
  }
}

template <typename F>
void dispatch_cpt(int cpt, F&& f) {
  switch (cpt) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

// ------------------------------------------------------------------ walks
std::vector<torch::Tensor> random_walks(torch::Tensor row_ptr, torch::Tensor col_idx,
                                        torch::Tensor weights, torch::Tensor sources,
                                        int64_t num_repetition, int64_t len_path,
                                        int64_t seed) {
  CHECK_I32(row_ptr); CHECK_I32(col_idx); CHECK_F32(weights); CHECK_I32(sources);
  check_same_device(row_ptr, {col_idx, weights, sources});
  TORCH_CHECK(len_path >= 1 && len_path <= 512, "len_path out of range");
  const int n_src = int_arg(sources.numel(), "sources.numel()");
  const int num_rep = int_arg(num_repetition, "num_repetition");
  const long long n_walks = (long long)n_src * num_rep;
  auto nodes = torch::empty({n_walks, len_path}, opts_on(row_ptr, at::kInt));
  auto lengths = torch::empty({n_walks}, opts_on(row_ptr, at::kInt));
  auto hashes = torch::empty({n_walks}, opts_on(row_ptr, at::kLong));
  if (n_walks == 0) return {nodes, lengths, hashes};
  int tsize = 256;                   // LDS hash set: >= 2x path length, pow2
  while (tsize < 2 * (int)len_path) tsize <<= 1;
  const int wpb = 4;                 // 256 threads = 4 waves
  const size_t lds = (size_t)wpb * (len_path + tsize) * sizeof(int);
  launch(walk_kernel, grid_for(n_walks, wpb), lds, i32(row_ptr), i32(col_idx),
         f32(weights), i32(sources), n_src, n_walks, num_rep, len_path, tsize,
         seed, i32(nodes), i32(lengths),
         (long long*)hashes.data_ptr<int64_t>());
  return {nodes, lengths, hashes};
}

// ------------------------------------------------------------ CBOW (fast)
// offs is the CSR row pointer of the P paths: the kernels read offs[p + 1]
inline void check_offs(const torch::Tensor& offs, long long P) {
  TORCH_CHECK(offs.numel() == P + 1, "offs must have P + 1 elements");
}
inline void check_p_split(long long p_split, long long P) {
  TORCH_CHECK(p_split >= 0 && p_split <= P, "p_split must be in [0, P]");
}
// seg_start is the CSR row pointer of the gene segments
inline void check_seg_start(const torch::Tensor& seg_start, int n_seg) {
  TORCH_CHECK(seg_start.numel() == (long long)n_seg + 1,
              "seg_start must have n_seg + 1 elements");
}

std::vector<torch::Tensor> cbow_fwd_scalar(torch::Tensor s, torch::Tensor genes,
                                           torch::Tensor offs, torch::Tensor labels,
                                           double inv_b, bool want_grad) {
  CHECK_F32(s); CHECK_I32(genes); CHECK_I32(offs); CHECK_F32(labels);
  check_same_device(s, {genes, offs, labels});
  const long long P = labels.numel();
  check_offs(offs, P);
  auto loss = torch::empty({P}, opts_on(s));
  auto correct = torch::empty({P}, opts_on(s));
  auto dO = torch::empty({want_grad ? P : 0}, opts_on(s));
  if (P == 0) return {loss, correct, dO};
  // 16 paths per block (16-lane sub-waves); capped because the dispatch ramp
  // of 8k+ tiny blocks costs more than the grid-stride work itself
  launch(cbow_fwd_scalar_kernel, grid_for(P, 16, 2048), 0, f32(s), i32(genes),
         i32(offs), f32(labels), P, inv_b, f32(loss), f32(correct),
         want_grad ? f32(dO) : nullptr);
  return {loss, correct, dO};
}

// second pass of every eval: one block folds the [grid, 2] per-block count
// partials into counts[2]
void fold_partials(const torch::Tensor& partials, torch::Tensor& counts) {
  launch(fold_partials_kernel, 1, 0, f32(partials), partials.size(0),
         f32(counts));
}

// fold_partials for K evals' tables at once: partials [K, grid, 2] ->
// counts [K, 2], one block per table (the K-epoch block graph's one fold)
void fold_partials_rows_(torch::Tensor partials, torch::Tensor counts) {
  CHECK_F32(partials); CHECK_F32(counts);
  check_same_device(partials, {counts});
  TORCH_CHECK(partials.dim() == 3 && partials.size(2) == 2,
              "partials must be [K, grid, 2]");
  const int K = int_arg(partials.size(0), "partials.size(0)");
  const int grid = int_arg(partials.size(1), "partials.size(1)");
  TORCH_CHECK(counts.dim() == 2 && counts.size(0) == K && counts.size(1) == 2,
              "counts must be [K, 2]");
  if (K == 0) return;
  launch(fold_partials_rows_kernel, K, 0, f32(partials), grid, f32(counts));
}

// The eval's launch geometry, in one place: the LDS-staged variant
// (G2VEC_EVAL_LDS=<bytes> opts in when the whole s table fits that
// per-block LDS budget) stages s in LDS so gathers are bank-parallel
// ds_reads instead of L1 line-divergent loads, grid capped
// (G2VEC_EVAL_LDS_GRID, default 1024) so each block amortizes its stage.
// Bitwise-identical math. Measured (profiles/README.md, round 2): wins the
// isolated microbench ~11% at ex_* shape (27.2 vs 30.2 us,
// tools/bench_eval.py) but is NEUTRAL-to-slightly-worse inside the real
// epoch chain (905 -> 893-902M paths/s same-box), so it is OFF by default —
// kept as the documented measured alternative. Otherwise 16 paths per block
// (16-lane sub-waves); G2VEC_EVAL_GRID: sweep knob, default 8192 waves fill
// the chip. The knobs are read on every call.
struct EvalGeom { bool lds; int grid; };
inline EvalGeom eval_geom(long long P, long long G) {
  const char* lds_env = getenv("G2VEC_EVAL_LDS");
  const long long lds_cap = lds_env ? atoll(lds_env) : 0;
  const bool lds = G * 4 <= lds_cap && G * 4 <= 158 * 1024;   // 160 KB LDS hard limit
  return {lds, grid_for(P, 16, lds ? env_int_min1("G2VEC_EVAL_LDS_GRID", 1024)
                                   : env_int_min1("G2VEC_EVAL_GRID", 2048))};
}

// rows of the per-block partial table an eval of P paths over a G-gene s
// table writes: what a caller-owned `partials` of cbow_eval_counts_ must have
int64_t eval_grid(int64_t P, int64_t G) {
  TORCH_CHECK(P >= 0 && G >= 0, "eval_grid: P and G must be >= 0");
  return eval_geom(P, G).grid;
}

void cbow_eval_counts_(torch::Tensor s, torch::Tensor genes, torch::Tensor offs,
                       torch::Tensor labels, int64_t p_split,
                       torch::Tensor counts,
                       std::optional<torch::Tensor> dO, double inv_b,
                       std::optional<torch::Tensor> partials_out) {
  // partials_out [grid, 2] given: the per-block partials go there and NO
  // fold is launched (counts is left as it is) — the caller folds a block of
  // such tables with fold_partials_rows_
  if (dO) {
    CHECK_F32(*dO);
    TORCH_CHECK(dO->numel() >= p_split,
                "dO must cover the train split (p < p_split)");
  }
  CHECK_F32(s); CHECK_I32(genes); CHECK_I32(offs); CHECK_F32(labels);
  CHECK_F32(counts);
  check_same_device(s, {genes, offs, labels, counts});
  if (dO) check_same_device(s, {*dO});
  TORCH_CHECK(counts.numel() == 2, "counts must have 2 elements");
  const long long P = labels.numel();
  check_offs(offs, P);
  check_p_split(p_split, P);
  const long long G = s.numel();
  const auto [lds, grid] = eval_geom(P, G);
  if (partials_out) {
    CHECK_F32(*partials_out);
    check_same_device(s, {*partials_out});
    TORCH_CHECK(partials_out->dim() == 2 && partials_out->size(0) == grid &&
                    partials_out->size(1) == 2,
                "partials must be [eval_grid(P, G), 2] = [", grid, ", 2]");
  }
  if (P == 0) return;
  auto partials =
      partials_out ? *partials_out : torch::empty({grid, 2}, opts_on(s));
  if (lds) {
    launch(cbow_eval_counts_lds_kernel, grid, G * 4, f32(s), i32(genes),
           i32(offs), f32(labels), P, p_split, f32(partials), f32(dO), inv_b,
           G);
  } else {
    launch(cbow_eval_counts_kernel, grid, 0, f32(s), i32(genes), i32(offs),
           f32(labels), P, p_split, f32(partials), f32(dO), inv_b);
  }
  if (!partials_out) fold_partials(partials, counts);
}

void cbow_eval_scan_(torch::Tensor s, torch::Tensor genes,
                     torch::Tensor pathid, torch::Tensor offs,
                     torch::Tensor labels, int64_t p_split, int64_t cap,
                     torch::Tensor piece, torch::Tensor counts,
                     std::optional<torch::Tensor> dO, double inv_b) {
  // instance-parallel fused eval (see eval_scan_kernel): piece buffer is
  // persistent (hipGraph-stable) and sized P * cap
  CHECK_F32(s); CHECK_I32(genes); CHECK_I32(pathid); CHECK_I32(offs);
  CHECK_F32(labels); CHECK_F32(piece); CHECK_F32(counts);
  check_same_device(s, {genes, pathid, offs, labels, piece, counts});
  const long long P = labels.numel();
  const long long nnz = genes.numel();
  const int cap_i = int_arg(cap, "cap");
  check_offs(offs, P);
  check_p_split(p_split, P);
  TORCH_CHECK(pathid.numel() == nnz,
              "pathid must have one element per element of genes");
  TORCH_CHECK(piece.numel() >= P * cap, "piece buffer too small");
  if (dO) {
    CHECK_F32(*dO);
    check_same_device(s, {*dO});
    TORCH_CHECK(dO->numel() >= p_split, "dO must cover the train split");
  }
  if (P == 0) return;
  // LDS-staged s (<= 48 KB tables): persistent blocks amortize the one-time
  // stage, so the grid is capped
  const long long G = s.numel();
  const bool lds = G * 4 <= 48 * 1024;
  launch(eval_scan_kernel, grid_for(nnz, 256, lds ? 1536 : GRID_MAX),
         lds ? G * sizeof(float) : 0, f32(s), i32(genes), i32(pathid),
         i32(offs), nnz, cap_i, f32(piece), lds ? G : 0);
  const int grid_b = grid_for(P, 256, 2048);
  auto partials = torch::empty({grid_b, 2}, opts_on(s));
  launch(eval_finish_kernel, grid_b, 0, f32(piece), i32(offs), f32(labels), P,
         p_split, cap_i, f32(partials), f32(dO), inv_b);
  fold_partials(partials, counts);
}

void scatter_dO_det_(torch::Tensor inst_path, torch::Tensor seg_start,
                     torch::Tensor seg_gene, torch::Tensor dO,
                     torch::Tensor c) {
  // Accumulating out-arg variant: one slab's gene segments are reduced and
  // ADDED into c (caller zeroes it once). The slab-blocked caller issues
  // one launch per ~3 MB dO slice so each XCD's L2 holds the slice being
  // gathered instead of thrashing across the whole dO table.
  CHECK_I32(inst_path); CHECK_I32(seg_start); CHECK_I32(seg_gene);
  CHECK_F32(dO); CHECK_F32(c);
  check_same_device(inst_path, {seg_start, seg_gene, dO, c});
  const int n_seg = int_arg(seg_gene.numel(), "seg_gene.numel()");
  check_seg_start(seg_start, n_seg);
  if (n_seg == 0) return;
  launch(scatter_do_det_kernel, grid_for(n_seg, 4), 0, i32(inst_path),
         i32(seg_start), i32(seg_gene), n_seg, f32(dO), f32(c));
}

// lr_t lives in a device slot (see adam_rank1_kernel); only element 0 is read
inline void check_lrt(const torch::Tensor& lrt) {
  TORCH_CHECK(lrt.is_cuda(), "lrt must be on the GPU");
  TORCH_CHECK(lrt.scalar_type() == at::kFloat, "lrt must be float32");
  TORCH_CHECK(lrt.numel() >= 1, "lrt must hold at least one element");
}

void adam_rank1(torch::Tensor W, torch::Tensor m, torch::Tensor v,
                torch::Tensor c, torch::Tensor who, torch::Tensor lrt,
                double b1, double b2, double eps,
                std::optional<torch::Tensor> mO,
                std::optional<torch::Tensor> vO) {
  // mO/vO given: FUSED epoch tail — the same pass that streams the
  // pre-update W rows for the rank-1 Adam also emits per-block partials
  // of dW_ho = W_pre^T c, and one fold launch applies the who update
  // (replaces the separate gemv_cols + fold_cols + adam_dense chain and
  // its extra full W read; deterministic block order).
  CHECK_F32(W); CHECK_F32(m); CHECK_F32(v); CHECK_F32(c); CHECK_F32(who);
  check_lrt(lrt);
  check_same_device(W, {m, v, c, who, lrt});
  TORCH_CHECK(W.dim() == 2, "W must be [G, h]");
  const long long G = W.size(0);
  const int h = int_arg(W.size(1), "W.size(1)");
  check_adam_hidden(h);
  TORCH_CHECK(m.numel() == W.numel() && v.numel() == W.numel(),
              "m/v/W size mismatch");
  TORCH_CHECK(c.numel() == G, "c must have one element per W row");
  TORCH_CHECK(who.numel() == h, "who must have one element per W column");
  const int rpb = 256 / (h / 4);   // rows per 256-thread block
  const bool fused = mO.has_value();
  TORCH_CHECK(fused == vO.has_value(), "mO and vO go together");
  // fused: the cap bounds the partial table / fold cost
  const int grid = grid_for(G, rpb, fused ? 1024 : GRID_MAX);
  torch::Tensor partials;
  float* gw = nullptr;
  if (fused) {
    CHECK_F32(*mO); CHECK_F32(*vO);
    check_same_device(W, {*mO, *vO});
    TORCH_CHECK(mO->numel() == h && vO->numel() == h,
                "mO/vO must have one element per W column");
    partials = torch::empty({grid, h}, opts_on(W));
    gw = f32(partials);
  }
  launch(adam_rank1_kernel, grid, 0, f32(W), f32(m), f32(v), f32(c), f32(who),
         G, h, f32(lrt), b1, b2, eps, gw);
  if (fused)
    launch(fold_gw_adam_kernel, grid_for(h, 4), 0, gw, grid, h, f32(who),
           f32(mO), f32(vO), f32(lrt), b1, b2, eps);
}

void adam_dense(torch::Tensor W, torch::Tensor m, torch::Tensor v,
                torch::Tensor grad, torch::Tensor lrt, double b1, double b2,
                double eps) {
  CHECK_F32(W); CHECK_F32(m); CHECK_F32(v); CHECK_F32(grad);
  check_lrt(lrt);
  check_same_device(W, {m, v, grad, lrt});
  TORCH_CHECK(grad.numel() == W.numel(), "grad/W size mismatch");
  TORCH_CHECK(m.numel() == W.numel() && v.numel() == W.numel(),
              "m/v/W size mismatch");
  const long long n = W.numel();
  launch(adam_dense_kernel, grid_for(n, 256), 0, f32(W), f32(m), f32(v),
         f32(grad), n, f32(lrt), b1, b2, eps);
}

// ---------------------------------------------------------- CBOW (general)
std::vector<torch::Tensor> cbow_fwd(torch::Tensor W, torch::Tensor who,
                                    torch::Tensor genes, torch::Tensor offs,
                                    torch::Tensor labels, double inv_b,
                                    bool want_grad, int64_t act) {
  CHECK_GPU_CONT(W);
  CHECK_F32(who); CHECK_I32(genes); CHECK_I32(offs); CHECK_F32(labels);
  const bool bf16 = W.scalar_type() == at::kBFloat16;
  const bool fp16 = W.scalar_type() == at::kHalf;
  TORCH_CHECK(bf16 || fp16 || W.scalar_type() == at::kFloat,
              "W must be f32, bf16 or fp16");
  check_same_device(W, {who, genes, offs, labels});
  TORCH_CHECK(W.dim() == 2, "W must be [G, h]");
  const long long P = labels.numel();
  const int h = int_arg(W.size(1), "W.size(1)");
  const int hpl = hpl_for(h);
  const int act_i = int_arg(act, "act");
  TORCH_CHECK(who.numel() == h, "who must have one element per W column");
  check_offs(offs, P);
  auto loss = torch::empty({P}, opts_on(W));
  auto correct = torch::empty({P}, opts_on(W));
  auto dO = torch::empty({want_grad ? P : 0}, opts_on(W));
  auto H = want_grad ? torch::empty({P, h}, opts_on(W))
                     : torch::empty({0}, opts_on(W));
  if (P == 0) return {loss, correct, dO, H};
  const int grid = grid_for(P, 4);
  // Wp: the weight table as the kernel's element (tag) type
  auto go = [&](auto* Wp) {
    using WT = std::remove_cv_t<std::remove_pointer_t<decltype(Wp)>>;
    dispatch_hpl(hpl, [&](auto HPL) {
      launch(cbow_fwd_kernel<WT, decltype(HPL)::value>, grid, 0, Wp, f32(who),
             i32(genes), i32(offs), f32(labels), P, inv_b, h,
             want_grad ? f32(H) : nullptr, f32(loss), f32(correct),
             want_grad ? f32(dO) : nullptr, act_i);
    });
  };
  if (bf16) go((const bf16_bits*)W.data_ptr<at::BFloat16>());
  else if (fp16) go((const fp16_bits*)W.data_ptr<at::Half>());
  else go(f32(W));
  return {loss, correct, dO, H};
}

torch::Tensor cbow_bwd_rows(torch::Tensor who, torch::Tensor inst_path,
                            torch::Tensor seg_start, torch::Tensor seg_gene,
                            torch::Tensor dO, int64_t n_genes,
                            std::optional<torch::Tensor> Hpre) {
  // Hpre: pre-activation H for the ReLU backward mask (absent = linear)
  CHECK_F32(who); CHECK_I32(inst_path); CHECK_I32(seg_start);
  CHECK_I32(seg_gene); CHECK_F32(dO);
  if (Hpre) CHECK_F32(*Hpre);
  check_same_device(who, {inst_path, seg_start, seg_gene, dO});
  if (Hpre) check_same_device(who, {*Hpre});
  const int h = int_arg(who.numel(), "who.numel()");
  const int hpl = hpl_for(h);
  const int n_seg = int_arg(seg_gene.numel(), "seg_gene.numel()");
  check_seg_start(seg_start, n_seg);
  auto dW = torch::zeros({n_genes, h}, opts_on(dO));
  if (n_seg == 0) return dW;
  dispatch_hpl(hpl, [&](auto HPL) {
    launch(cbow_bwd_rows_det_kernel<decltype(HPL)::value>, grid_for(n_seg, 4),
           0, f32(who), i32(inst_path), i32(seg_start), i32(seg_gene), n_seg,
           f32(dO), h, f32(dW), f32(Hpre));
  });
  return dW;
}

// ------------------------------------------------------------------- PCC
torch::Tensor pcc_edges(torch::Tensor zt, torch::Tensor edge_idx,
                        int64_t n_group) {
  CHECK_F32(zt); CHECK_I32(edge_idx);
  check_same_device(zt, {edge_idx});
  TORCH_CHECK(zt.dim() == 2, "zt must be [G, S]");
  TORCH_CHECK(edge_idx.dim() == 2 && edge_idx.size(1) == 2,
              "edge_idx must be [E, 2]");
  const long long E = edge_idx.size(0);
  const int S = int_arg(zt.size(1), "zt.size(1)");
  auto out = torch::empty({E}, opts_on(zt));
  if (E == 0) return out;
  launch(pcc_edges_kernel, grid_for(E, 4), 0, f32(zt), i32(edge_idx), E, S,
         1.0f / (float)n_group, f32(out));
  return out;
}

torch::Tensor corr_gemm(torch::Tensor zt, int64_t n_group) {
  CHECK_F32(zt);
  TORCH_CHECK(zt.dim() == 2, "zt must be [G, S]");
  // trap here instead of silently emitting garbage PCC weights
  check_gfx950("corr_gemm", "MFMA kernel (use pcc_mode=edge)");
  const int G = int_arg(zt.size(0), "zt.size(0)");
  const int S = int_arg(zt.size(1), "zt.size(1)");
  // one block per 64 x 64 tile of C: the tile count is the launch's grid.x
  const long long ntile = ((long long)G + 63) / 64;
  TORCH_CHECK(ntile * ntile <= (long long)INT_MAX, "corr_gemm: zt.size(0) = ",
              G, " needs ", ntile * ntile,
              " tiles, over the 2^31 - 1 blocks of one launch "
              "(use pcc_mode=edge)");
  const int S4 = ((S + 3) / 4) * 4;
  const size_t lds = 2ull * 64 * S4 * sizeof(float);
  TORCH_CHECK(lds <= 160 * 1024,
              "corr_gemm: S too large for the LDS-staged tile (use pcc_mode=edge)");
  auto C = torch::empty({G, G}, opts_on(zt));
  launch(corr_gemm_kernel, (unsigned)(ntile * ntile), lds, f32(zt), f32(C), G,
         S, S4, 1.0f / (float)n_group);
  return C;
}

void trunc_normal_(torch::Tensor out, double std, int64_t seed) {
  CHECK_F32(out);
  const long long n = (long long)out.numel();
  if (n == 0) return;
  launch(trunc_normal_kernel, grid_for(n, 256), 0, f32(out), n, std, seed);
}

void gemv_rows_(torch::Tensor W, torch::Tensor x, torch::Tensor out,
                std::optional<torch::Tensor> clear) {
  // clear [G] given: zeroed by the same launch (see gemv_rows_kernel)
  CHECK_F32(W); CHECK_F32(x); CHECK_F32(out);
  check_same_device(W, {x, out});
  TORCH_CHECK(W.dim() == 2, "W must be [G, h]");
  const long long G = W.size(0);
  const int h = int_arg(W.size(1), "W.size(1)");
  const int hpl = hpl_for(h);
  TORCH_CHECK(out.numel() == G && x.numel() == h, "gemv_rows shape mismatch");
  if (clear) {
    CHECK_F32(*clear);
    check_same_device(W, {*clear});
    TORCH_CHECK(clear->numel() == G, "clear must have one element per W row");
    TORCH_CHECK(clear->data_ptr() != out.data_ptr(), "clear must not be out");
  }
  dispatch_hpl(hpl, [&](auto HPL) {
    launch(gemv_rows_kernel<decltype(HPL)::value>, row_wave_grid(G), 0, f32(W),
           f32(x), G, h, f32(out), f32(clear));
  });
}

void gemv_cols_(torch::Tensor W, torch::Tensor c, torch::Tensor out) {
  CHECK_F32(W); CHECK_F32(c); CHECK_F32(out);
  check_same_device(W, {c, out});
  TORCH_CHECK(W.dim() == 2, "W must be [G, h]");
  const long long G = W.size(0);
  const int h = int_arg(W.size(1), "W.size(1)");
  const int cpt = (h >= 256) ? h / 256 : 1;
  TORCH_CHECK(h % 64 == 0 && cpt >= 1 && cpt <= 4 && (cpt & (cpt - 1)) == 0,
              "gemv_cols needs hidden 64*k with h/256 in {<=1,2,4}");
  TORCH_CHECK(out.numel() == h && c.numel() == G, "gemv_cols shape mismatch");
  // ~8 rows per block: small G must still spread over the chip (8 blocks
  // for G=7.5k measured 78 us of serial row-walking; 941 blocks ~10 us)
  const int grid = grid_for(G, 8, 2048);
  auto partials = torch::empty({grid, h}, opts_on(W));
  dispatch_cpt(cpt, [&](auto CPT) {
    launch(gemv_cols_kernel<decltype(CPT)::value>, grid, 0, f32(W), f32(c), G,
           h, f32(partials));
  });
  launch(fold_cols_kernel, (h + 3) / 4, 0, f32(partials), grid, h, f32(out));
}

// --------------------------------------------- replica-batched fast path
// R models over one path set; layouts in g2vec_kernels.hip (REP_MAX). The
// per-replica launch geometry of every op is the single op's, so the same
// env caps apply and each replica's output is bitwise the single op's.
inline int check_rep_table(const torch::Tensor& t, const char* name) {
  check_f32(t, name);
  TORCH_CHECK(t.dim() == 2, name, " must be [rows, R]");
  const long long R = t.size(1);
  TORCH_CHECK(R >= 1 && R <= REP_MAX, name, ": R must be in [1, ", REP_MAX,
              "], got ", R);
  TORCH_CHECK(t.numel() < (1LL << 31), name, " must have < 2^31 elements");
  return (int)R;
}

// f(NT, VEC): NT = tiles of four replicas, VEC = 16-byte gathers possible
template <typename F>
void dispatch_rep(int R, const void* table, F&& f) {
  const bool vec = R % 4 == 0 && (reinterpret_cast<uintptr_t>(table) & 15) == 0;
  auto go = [&](auto NT) {
    if (vec) f(NT, std::true_type{}); else f(NT, std::false_type{});
  };
  switch ((R + 3) / 4) {
    case 1: go(std::integral_constant<int, 1>{}); break;
    case 2: go(std::integral_constant<int, 2>{}); break;
    case 3: go(std::integral_constant<int, 3>{}); break;
    case 4: go(std::integral_constant<int, 4>{}); break;
    case 5: go(std::integral_constant<int, 5>{}); break;
    case 6: go(std::integral_constant<int, 6>{}); break;
    case 7: go(std::integral_constant<int, 7>{}); break;
    default: go(std::integral_constant<int, 8>{}); break;
  }
}

void cbow_eval_counts_rep_(torch::Tensor s_R, torch::Tensor genes,
                           torch::Tensor offs, torch::Tensor labels,
                           int64_t p_split, torch::Tensor counts_R,
                           std::optional<torch::Tensor> dO_R, double inv_b) {
  // counts_R [R, 2] is OVERWRITTEN (the fold writes it); dO_R [>= p_split,
  // R] receives the train split's dlogits, rows >= p_split stay untouched
  const int R = check_rep_table(s_R, "s_R");
  CHECK_I32(genes); CHECK_I32(offs); CHECK_F32(labels); CHECK_F32(counts_R);
  check_same_device(s_R, {genes, offs, labels, counts_R});
  TORCH_CHECK(counts_R.numel() == 2 * R, "counts_R must be [R, 2]");
  const long long P = labels.numel();
  check_offs(offs, P);
  check_p_split(p_split, P);
  if (dO_R) {
    CHECK_F32(*dO_R);
    check_same_device(s_R, {*dO_R});
    TORCH_CHECK(dO_R->dim() == 2 && dO_R->size(1) == R &&
                    dO_R->size(0) >= p_split,
                "dO_R must be [>= p_split, R]");
  }
  if (P == 0) return;
  const int grid = grid_for(P, 16, env_int_min1("G2VEC_EVAL_GRID", 2048));
  auto partials = torch::empty({grid, R, 2}, opts_on(s_R));
  dispatch_rep(R, f32(s_R), [&](auto NT, auto VEC) {
    launch(cbow_eval_counts_rep_kernel<decltype(NT)::value,
                                       decltype(VEC)::value>,
           grid, 0, f32(s_R), i32(genes), i32(offs), f32(labels), P, p_split,
           R, f32(partials), f32(dO_R), inv_b);
  });
  launch(fold_partials_rep_kernel, R, 0, f32(partials), grid, R,
         f32(counts_R));
}

void scatter_dO_rep_(torch::Tensor inst_path, torch::Tensor seg_start,
                     torch::Tensor seg_gene, torch::Tensor dO_R,
                     torch::Tensor c_R) {
  // accumulating, like scatter_dO_det_: the caller zeroes c_R [G, R] once
  // and drives slab-blocked plans one slab per call
  CHECK_I32(inst_path); CHECK_I32(seg_start); CHECK_I32(seg_gene);
  const int R = check_rep_table(dO_R, "dO_R");
  TORCH_CHECK(check_rep_table(c_R, "c_R") == R, "c_R and dO_R differ in R");
  check_same_device(inst_path, {seg_start, seg_gene, dO_R, c_R});
  const int n_seg = int_arg(seg_gene.numel(), "seg_gene.numel()");
  check_seg_start(seg_start, n_seg);
  if (n_seg == 0) return;
  // dO_R decides VEC for both tables: c_R rows are written per lane
  dispatch_rep(R, f32(dO_R), [&](auto NT, auto VEC) {
    launch(scatter_do_rep_kernel<decltype(NT)::value, decltype(VEC)::value>,
           grid_for(n_seg, 4), 0, i32(inst_path), i32(seg_start),
           i32(seg_gene), n_seg, f32(dO_R), R, f32(c_R));
  });
}

void adam_rank1_rep(torch::Tensor W, torch::Tensor m, torch::Tensor v,
                    torch::Tensor c_R, torch::Tensor who, torch::Tensor mO,
                    torch::Tensor vO, torch::Tensor lrt, double b1, double b2,
                    double eps) {
  // the fused tail of adam_rank1 for W/m/v [R, G, h], who/mO/vO [R, h] and
  // c_R [G, R]: replica = grid y over the single launch's geometry
  CHECK_F32(W); CHECK_F32(m); CHECK_F32(v); CHECK_F32(who); CHECK_F32(mO);
  CHECK_F32(vO);
  check_lrt(lrt);
  const int R = check_rep_table(c_R, "c_R");
  check_same_device(W, {m, v, c_R, who, mO, vO, lrt});
  TORCH_CHECK(W.dim() == 3 && W.size(0) == R, "W must be [R, G, h]");
  const long long G = W.size(1);
  const int h = int_arg(W.size(2), "W.size(2)");
  check_adam_hidden(h);
  TORCH_CHECK(m.numel() == W.numel() && v.numel() == W.numel(),
              "m/v/W size mismatch");
  TORCH_CHECK(c_R.size(0) == G, "c_R must have one row per W row");
  TORCH_CHECK(who.numel() == (long long)R * h && mO.numel() == who.numel() &&
                  vO.numel() == who.numel(),
              "who/mO/vO must be [R, h]");
  if (G == 0) return;
  const int rpb = 256 / (h / 4);
  const int grid = grid_for(G, rpb, 1024);   // as the single fused launch
  auto partials = torch::empty({R, grid, h}, opts_on(W));
  launch(adam_rank1_rep_kernel, dim3(grid, R), 0, f32(W), f32(m), f32(v),
         f32(c_R), f32(who), G, h, R, f32(lrt), b1, b2, eps, f32(partials));
  launch(fold_gw_adam_rep_kernel, dim3(grid_for(h, 4), R), 0, f32(partials),
         grid, h, f32(who), f32(mO), f32(vO), f32(lrt), b1, b2, eps);
}

void gemv_rows_rep_(torch::Tensor W, torch::Tensor who, torch::Tensor s_R) {
  CHECK_F32(W); CHECK_F32(who);
  const int R = check_rep_table(s_R, "s_R");
  check_same_device(W, {who, s_R});
  TORCH_CHECK(W.dim() == 3 && W.size(0) == R, "W must be [R, G, h]");
  const long long G = W.size(1);
  const int h = int_arg(W.size(2), "W.size(2)");
  const int hpl = hpl_for(h);
  TORCH_CHECK(s_R.size(0) == G && who.numel() == (long long)R * h,
              "gemv_rows_rep shape mismatch");
  if (G == 0) return;
  dispatch_hpl(hpl, [&](auto HPL) {
    launch(gemv_rows_rep_kernel<decltype(HPL)::value>,
           dim3(row_wave_grid(G), R), 0, f32(W), f32(who), G, h, R, f32(s_R));
  });
}

torch::Tensor bf16_copy(torch::Tensor src) {
  CHECK_F32(src);
  auto out = torch::empty_like(src, src.options().dtype(at::kBFloat16));
  const long long n = src.numel();
  if (n == 0) return out;
  launch(f32_to_bf16_kernel, grid_for(n, 256), 0, f32(src),
         (uint16_t*)out.data_ptr<at::BFloat16>(), n);
  return out;
}

// ------------------------------------------- steps 5-6: k-means and scoring
// kmeans_step LDS budget: k*h centroid floats + one [k][h] accumulator per
// wave (4 waves) = 5*k*h floats of the CU's 160 KiB
constexpr long long KM_LDS_LIMIT = 160 * 1024;

void kmeans_step(torch::Tensor X, torch::Tensor C, torch::Tensor prev,
                 torch::Tensor labels, torch::Tensor C_new,
                 torch::Tensor sums, torch::Tensor counts,
                 torch::Tensor n_changed, torch::Tensor inertia) {
  // one fused Lloyd iteration, all outputs through out-arguments; prev may
  // be labels and C_new may be C (see the kernels)
  CHECK_F32(X); CHECK_F32(C); CHECK_I32(prev); CHECK_I32(labels);
  CHECK_F32(C_new); CHECK_F32(sums); CHECK_I32(counts); CHECK_I32(n_changed);
  CHECK_F64(inertia);
  check_same_device(X, {C, prev, labels, C_new, sums, counts, n_changed,
                        inertia});
  TORCH_CHECK(X.dim() == 2 && C.dim() == 2, "X must be [G, h] and C [k, h]");
  const long long G = X.size(0);
  const int h = int_arg(X.size(1), "X.size(1)");
  const int hpl = hpl_for(h);
  const long long k = C.size(0);
  TORCH_CHECK(C.size(1) == h, "C must have X's ", h, " columns");
  TORCH_CHECK(k >= 1 && k <= KM_MAX_K, "k must be in [1, ", KM_MAX_K,
              "], got ", k);
  const long long lds = 5 * k * h * (long long)sizeof(float);
  TORCH_CHECK(lds <= KM_LDS_LIMIT, "kmeans_step: k*h = ", k * h,
              " needs ", lds, " B of LDS (centroids + 4 per-wave "
              "accumulators), over the ", KM_LDS_LIMIT, " B budget");
  TORCH_CHECK(G >= 1, "X must have at least one row");
  CHECK_ROWS16(X);
  TORCH_CHECK(prev.numel() == G && labels.numel() == G,
              "prev and labels must have one element per X row");
  TORCH_CHECK(C_new.dim() == 2 && C_new.size(0) == k && C_new.size(1) == h,
              "C_new must have C's shape");
  TORCH_CHECK(sums.numel() == k * h, "sums must be [k, h]");
  TORCH_CHECK(counts.numel() == k, "counts must have k elements");
  TORCH_CHECK(n_changed.numel() == 1 && inertia.numel() == 1,
              "n_changed and inertia must have one element");
  // >= 16 rows per block amortize the LDS clear and the partial write; the
  // cap is what the chip holds at once (blocks per CU by LDS, at most the 8
  // that 32 waves allow): more blocks would queue behind the resident ones
  // and only lengthen the partial table ([grid, k*h]) and the fold
  long long per_cu = KM_LDS_LIMIT / lds;
  if (per_cu > 8) per_cu = 8;
  const int grid = grid_for(G, 16, cu_count("kmeans_step") * per_cu);
  auto psums = torch::empty({grid, k * h}, opts_on(X));
  auto pcnt = torch::empty({grid, KM_PCNT}, opts_on(X, at::kInt));
  auto pinert = torch::empty({grid}, opts_on(X, at::kDouble));
  dispatch_hpl(hpl, [&](auto HPL) {
    launch(kmeans_step_kernel<decltype(HPL)::value>, grid, lds, f32(X), f32(C),
           i32(prev), i32(labels), G, h, k, f32(psums), i32(pcnt),
           f64(pinert));
  });
  launch(kmeans_fold_kernel, grid_for(k * h, 4), 0, f32(psums), i32(pcnt),
         f64(pinert), grid, k, h, f32(C), f32(C_new), f32(sums), i32(counts),
         i32(n_changed), f64(inertia));
}

void kmeans_mind2_(torch::Tensor X, torch::Tensor c, torch::Tensor d2) {
  CHECK_F32(X); CHECK_F32(c); CHECK_F32(d2);
  check_same_device(X, {c, d2});
  TORCH_CHECK(X.dim() == 2, "X must be [G, h]");
  const long long G = X.size(0);
  const int h = int_arg(X.size(1), "X.size(1)");
  const int hpl = hpl_for(h);
  TORCH_CHECK(c.numel() == h, "c must have one element per X column");
  TORCH_CHECK(d2.numel() == G, "d2 must have one element per X row");
  CHECK_ROWS16(X); CHECK_ROWS16(c);
  if (G == 0) return;
  dispatch_hpl(hpl, [&](auto HPL) {
    launch(kmeans_mind2_kernel<decltype(HPL)::value>, row_wave_grid(G), 0,
           f32(X), f32(c), G, h, f32(d2));
  });
}

void row_norms_(torch::Tensor W, torch::Tensor out) {
  CHECK_F32(W); CHECK_F32(out);
  check_same_device(W, {out});
  TORCH_CHECK(W.dim() == 2, "W must be [G, h]");
  const long long G = W.size(0);
  const int h = int_arg(W.size(1), "W.size(1)");
  const int hpl = hpl_for(h);
  TORCH_CHECK(out.numel() == G, "out must have one element per W row");
  CHECK_ROWS16(W);
  if (G == 0) return;
  dispatch_hpl(hpl, [&](auto HPL) {
    launch(row_norms_kernel<decltype(HPL)::value>, row_wave_grid(G), 0, f32(W),
           G, h, f32(out));
  });
}

void t_scores_(torch::Tensor expr, torch::Tensor labels, torch::Tensor out) {
  // labels: i32 or i64 [S]; the kernel reads an i32 copy
  CHECK_F32(expr); CHECK_GPU_CONT(labels); CHECK_F32(out);
  TORCH_CHECK(labels.scalar_type() == at::kInt ||
                  labels.scalar_type() == at::kLong,
              "labels must be int32 or int64");
  check_same_device(expr, {labels, out});
  TORCH_CHECK(expr.dim() == 2, "expr must be [S, G]");
  const long long S = expr.size(0);
  const long long G = expr.size(1);
  TORCH_CHECK(S >= 1 && S < (1LL << 31), "expr needs 1 <= S < 2^31 rows");
  TORCH_CHECK(labels.numel() == S, "labels must have one element per sample");
  TORCH_CHECK(out.numel() == G, "out must have one element per gene");
  if (G == 0) return;
  auto lab = labels.to(at::kInt).contiguous();
  launch(t_scores_kernel, grid_for(G, 256), 0, f32(expr), i32(lab), S, G,
         f32(out));
}

// ------------------------------------------- step 6: permutation null of t
void col_moments_(torch::Tensor expr, torch::Tensor T, torch::Tensor Q) {
  CHECK_F32(expr); CHECK_F64(T); CHECK_F64(Q);
  check_same_device(expr, {T, Q});
  TORCH_CHECK(expr.dim() == 2, "expr must be [S, G]");
  const long long S = expr.size(0);
  const long long G = expr.size(1);
  TORCH_CHECK(S >= 1 && S < (1LL << 31), "expr needs 1 <= S < 2^31 rows");
  TORCH_CHECK(T.dim() == 1 && T.numel() == G && Q.dim() == 1 &&
                  Q.numel() == G,
              "T and Q must be [G]");
  if (G == 0) return;
  launch(col_moments_kernel, grid_for(G, 256), 0, f32(expr), S, G, f64(T),
         f64(Q));
}

// shared guards of the two perm_t entry points; returns the launch grid
inline dim3 perm_t_check(const char* op, const torch::Tensor& expr,
                         const torch::Tensor& masks, const torch::Tensor& T,
                         const torch::Tensor& Q, int64_t n1) {
  CHECK_F32(expr); CHECK_GPU_CONT(masks); CHECK_F64(T); CHECK_F64(Q);
  TORCH_CHECK(masks.scalar_type() == at::kByte, "masks must be uint8");
  check_same_device(expr, {masks, T, Q});
  TORCH_CHECK(expr.dim() == 2, "expr must be [S, G]");
  TORCH_CHECK(masks.dim() == 2, "masks must be [B, S]");
  const long long S = expr.size(0);
  const long long G = expr.size(1);
  const long long B = masks.size(0);
  TORCH_CHECK(masks.size(1) == S, op, ": masks has ", masks.size(1),
              " columns, expr has ", S, " samples");
  TORCH_CHECK(S >= 4 && S < (1LL << 31), op, " needs 4 <= S < 2^31 samples");
  TORCH_CHECK(n1 >= 2 && S - n1 >= 2, op,
              " needs at least 2 samples in each group");
  TORCH_CHECK(T.dim() == 1 && T.numel() == G && Q.dim() == 1 &&
                  Q.numel() == G,
              "T and Q must be [G]");
  check_gfx950(op);
  const long long ngt = (G + 63) / 64;
  const long long nbt = (B + 63) / 64;
  TORCH_CHECK(ngt < (1LL << 31), op, ": too many genes");
  // enough blocks to fill the device; each walks its share of the
  // relabelling tiles against one gene tile
  long long gy = ngt > 0 ? (2048 + ngt - 1) / ngt : 1;
  if (gy > nbt) gy = nbt;
  if (gy > 65535) gy = 65535;
  if (gy < 1) gy = 1;
  return dim3((unsigned)ngt, (unsigned)gy);
}

void perm_t_stats_(torch::Tensor expr, torch::Tensor masks, torch::Tensor T,
                   torch::Tensor Q, int64_t n1, torch::Tensor out) {
  const dim3 grid = perm_t_check("perm_t_stats", expr, masks, T, Q, n1);
  CHECK_F64(out);
  check_same_device(expr, {out});
  const long long S = expr.size(0), G = expr.size(1), B = masks.size(0);
  TORCH_CHECK(out.dim() == 2 && out.size(0) == B && out.size(1) == G,
              "out must be [B, G]");
  if (G == 0 || B == 0) return;
  launch(perm_t_stats_kernel, grid, 0, f32(expr), u8(masks), f64(T), f64(Q), S,
         G, B, n1, f64(out));
}

void perm_t_counts_(torch::Tensor expr, torch::Tensor masks, torch::Tensor T,
                    torch::Tensor Q, int64_t n1, torch::Tensor stat_obs,
                    torch::Tensor counts, torch::Tensor maxstat) {
  const dim3 grid = perm_t_check("perm_t_counts", expr, masks, T, Q, n1);
  CHECK_F64(stat_obs); CHECK_I32(counts); CHECK_F64(maxstat);
  check_same_device(expr, {stat_obs, counts, maxstat});
  const long long S = expr.size(0), G = expr.size(1), B = masks.size(0);
  TORCH_CHECK(stat_obs.dim() == 1 && stat_obs.numel() == G,
              "stat_obs must be [G]");
  TORCH_CHECK(counts.dim() == 1 && counts.numel() == G, "counts must be [G]");
  TORCH_CHECK(maxstat.dim() == 1 && maxstat.numel() == B,
              "maxstat must be [B]");
  // the kernel folds into both through integer atomics
  if (G > 0)
    C10_HIP_CHECK(hipMemsetAsync(i32(counts), 0, G * sizeof(int),
                                 cur_stream()));
  if (B > 0)
    C10_HIP_CHECK(hipMemsetAsync(f64(maxstat), 0, B * sizeof(double),
                                 cur_stream()));
  if (G == 0 || B == 0) return;
  launch(perm_t_counts_kernel, grid, 0, f32(expr), u8(masks), f64(T), f64(Q),
         f64(stat_obs), S, G, B, n1, i32(counts),
         reinterpret_cast<unsigned long long*>(f64(maxstat)));
}

// ------------------------------------------- rank statistics
// The guards both rank entry points share; every one runs before the first
// launch, so a refused call leaves the outputs as they were. Returns the grid.
inline int rank_check(const char* op, const torch::Tensor& expr,
                      long long s_limit) {
  CHECK_F32(expr);
  TORCH_CHECK(expr.dim() == 2, op, ": expr must be [S, G]");
  const long long S = expr.size(0);
  // ranks are half-integers <= S: exact in f32 below 2^23
  TORCH_CHECK(S >= 1 && S < s_limit, op, " needs 1 <= S < ", s_limit,
              " samples, got ", S);
  int_arg(S, "expr.size(0)");
  check_gfx950(op, "rank kernel");
  return grid_for(expr.size(1), RK_TG, RK_MAX_BLOCKS);
}

void rank_columns_(torch::Tensor expr, torch::Tensor ranks) {
  const int grid = rank_check("rank_columns", expr, 1LL << 23);
  CHECK_F32(ranks);
  check_same_device(expr, {ranks});
  TORCH_CHECK(ranks.dim() == 2 && ranks.size(0) == expr.size(0) &&
                  ranks.size(1) == expr.size(1),
              "rank_columns: ranks must have expr's shape");
  const int S = int_arg(expr.size(0), "expr.size(0)");
  const long long G = expr.size(1);
  if (G == 0) return;
  launch(rank_columns_kernel, grid, 0, f32(expr), S, G, f32(ranks));
}

void ranksum_scores_(torch::Tensor expr, torch::Tensor labels,
                     torch::Tensor z, torch::Tensor auc) {
  // 4 SSR <= S^3 / 3 must fit the kernel's int64 sums
  const int grid = rank_check("ranksum_scores", expr, (1LL << 21) + 1);
  CHECK_I32(labels); CHECK_F32(z); CHECK_F32(auc);
  check_same_device(expr, {labels, z, auc});
  const int S = int_arg(expr.size(0), "expr.size(0)");
  const long long G = expr.size(1);
  TORCH_CHECK(labels.dim() == 1 && labels.numel() == S,
              "ranksum_scores: labels must have one element per sample");
  TORCH_CHECK(z.dim() == 1 && z.numel() == G && auc.dim() == 1 &&
                  auc.numel() == G,
              "ranksum_scores: z and auc must be [G]");
  TORCH_CHECK(labels.min().item<int>() >= 0 && labels.max().item<int>() <= 1,
              "ranksum_scores: labels must hold only 0 and 1");
  const int n1 = int_arg(labels.sum().item<int64_t>(), "sum(labels)");
  if (G == 0) return;
  launch(ranksum_scores_kernel, grid, 0, f32(expr), i32(labels), S, G, n1,
         f32(z), f32(auc));
}

// ------------------------------------------- nearest genes: MFMA GEMM + top-k
// The launch split of knn_topk_: each block walks its share of the candidate
// tiles against one query tile, never more blocks along y than candidate
// tiles. The target is the number of blocks the device holds at once (CUs x
// the kernel's resident blocks per CU), not the ~2048 of perm_t_check: a
// block starts with empty lists and pays ~k ln(tiles * 64 / k) inserts per
// row however long its walk is, so fewer, longer walks amortize them, and a
// single resident set has no tail (100 x 1M x 512: 2.13 ms at 512 blocks
// against 3.38 ms at 2048 and 2.74 ms at 256). grid_y > 0 forces the split
// (tests).
// op names the caller in the messages, kernel is the tile kernel whose
// resident blocks are counted.
template <typename K>
int64_t tile_grid_y(const char* op, K kernel, int64_t Q, int64_t G,
                    int64_t grid_y) {
  TORCH_CHECK(Q >= 0 && G >= 0 && grid_y >= 0, op, ": negative argument");
  const long long nqt = (Q + KN_TILE - 1) / KN_TILE;
  const long long nct = (G + KN_TILE - 1) / KN_TILE;
  long long gy = grid_y;
  if (gy == 0) {
    int per_cu = 0;
    TORCH_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
                    &per_cu, kernel, 256, 0) == hipSuccess &&
                    per_cu >= 1,
                op, ": cannot read the kernel's occupancy");
    const long long resident = (long long)cu_count(op) * per_cu;
    gy = nqt > 0 ? (resident + nqt - 1) / nqt : 1;
  }
  if (gy > nct) gy = nct;
  if (gy > 65535) gy = 65535;
  if (gy < 1) gy = 1;
  return gy;
}

int64_t knn_grid_y(int64_t Q, int64_t G, int64_t grid_y) {
  return tile_grid_y("knn_grid_y", knn_tile_kernel, Q, G, grid_y);
}

void knn_topk_(torch::Tensor Xq, torch::Tensor X,
               std::optional<torch::Tensor> q_index, int64_t k,
               int64_t grid_y, std::optional<torch::Tensor> part_idx,
               std::optional<torch::Tensor> part_val, torch::Tensor idx,
               torch::Tensor val) {
  // every guard runs before the first launch: a refused call leaves idx and
  // val as they were
  CHECK_F32(Xq); CHECK_F32(X); CHECK_I32(idx); CHECK_F32(val);
  check_same_device(Xq, {X, idx, val});
  TORCH_CHECK(Xq.dim() == 2 && X.dim() == 2,
              "Xq must be [Q, h] and X [G, h]");
  const long long Q = Xq.size(0), G = X.size(0), h = X.size(1);
  TORCH_CHECK(Xq.size(1) == h, "Xq has ", Xq.size(1), " columns, X has ", h);
  TORCH_CHECK(h >= 4 && h % 4 == 0 && h < (1LL << 31),
              "knn_topk: h must be a positive multiple of 4, got ", h);
  CHECK_ROWS16(Xq); CHECK_ROWS16(X);
  TORCH_CHECK(k >= 1 && k <= 64, "knn_topk: k must be in [1, 64], got ", k);
  TORCH_CHECK(G < (1LL << 31), "knn_topk: G must be below 2^31");
  if (q_index) {
    CHECK_I32(*q_index);
    check_same_device(Xq, {*q_index});
    TORCH_CHECK(q_index->dim() == 1 && q_index->numel() == Q,
                "q_index must be [Q]");
  }
  TORCH_CHECK(idx.dim() == 2 && idx.size(0) == Q && idx.size(1) == k &&
                  val.dim() == 2 && val.size(0) == Q && val.size(1) == k,
              "idx and val must be [Q, k]");
  TORCH_CHECK(grid_y >= 0, "grid_y must be >= 0 (0 = automatic)");
  const long long gy = knn_grid_y(Q, G, grid_y);
  const long long nqt = (Q + KN_TILE - 1) / KN_TILE;
  TORCH_CHECK(nqt < (1LL << 31), "knn_topk: too many queries");
  if (gy > 1) {
    TORCH_CHECK(part_idx.has_value() && part_val.has_value(),
                "knn_topk: a split over ", gy,
                " blocks needs the partial buffers");
    CHECK_I32(*part_idx); CHECK_F32(*part_val);
    check_same_device(Xq, {*part_idx, *part_val});
    TORCH_CHECK(part_idx->numel() == Q * gy * k &&
                    part_val->numel() == Q * gy * k,
                "part_idx and part_val must be [Q, ", gy, ", k]");
  }
  check_gfx950("knn_topk");
  if (Q == 0) return;
  launch(knn_tile_kernel, dim3((unsigned)nqt, (unsigned)gy), 0, f32(Xq),
         f32(X), q_index ? i32(*q_index) : nullptr, Q, G, h, k,
         gy > 1 ? i32(*part_idx) : i32(idx),
         gy > 1 ? f32(*part_val) : f32(val));
  if (gy > 1)
    launch(knn_merge_kernel, grid_for(Q, 4), 0, i32(*part_idx),
           f32(*part_val), Q, gy, k, i32(idx), f32(val));
}

// ------------------------------------------- L-group silhouettes: distance sums
// The candidate split of cluster_dist_sums_: knn_grid_y's rule on the
// occupancy of the instantiation that serves k.
int64_t cds_grid_y(int64_t Q, int64_t G, int64_t k, int64_t grid_y) {
  return k <= 4
      ? tile_grid_y("cds_grid_y", cds_tile_kernel<4>, Q, G, grid_y)
      : tile_grid_y("cds_grid_y", cds_tile_kernel<8>, Q, G, grid_y);
}

void cluster_dist_sums_(torch::Tensor Xq, torch::Tensor X,
                        torch::Tensor labels,
                        std::optional<torch::Tensor> q_index, int64_t k,
                        int64_t grid_y, torch::Tensor nq, torch::Tensor nx,
                        std::optional<torch::Tensor> part, torch::Tensor D) {
  // every guard runs before the first launch: a refused call leaves nq, nx
  // and D as they were
  CHECK_F32(Xq); CHECK_F32(X); CHECK_I32(labels); CHECK_F32(nq); CHECK_F32(nx);
  CHECK_F64(D);
  check_same_device(Xq, {X, labels, nq, nx, D});
  TORCH_CHECK(Xq.dim() == 2 && X.dim() == 2,
              "Xq must be [Q, h] and X [G, h]");
  const long long Q = Xq.size(0), G = X.size(0), h = X.size(1);
  TORCH_CHECK(Xq.size(1) == h, "Xq has ", Xq.size(1), " columns, X has ", h);
  TORCH_CHECK(h >= 4 && h % 4 == 0 && h < (1LL << 31),
              "cluster_dist_sums: h must be a positive multiple of 4, got ", h);
  CHECK_ROWS16(Xq); CHECK_ROWS16(X);
  TORCH_CHECK(k >= 1 && k <= 8,
              "cluster_dist_sums: k must be in [1, 8], got ", k);
  TORCH_CHECK(G < (1LL << 31), "cluster_dist_sums: G must be below 2^31");
  TORCH_CHECK(labels.dim() == 1 && labels.numel() == G,
              "labels must be [G]");
  if (q_index) {
    CHECK_I32(*q_index);
    check_same_device(Xq, {*q_index});
    TORCH_CHECK(q_index->dim() == 1 && q_index->numel() == Q,
                "q_index must be [Q]");
  }
  TORCH_CHECK(nq.dim() == 1 && nq.numel() == Q && nx.dim() == 1 &&
                  nx.numel() == G,
              "nq must be [Q] and nx [G]");
  TORCH_CHECK(D.dim() == 2 && D.size(0) == Q && D.size(1) == k,
              "D must be [Q, k]");
  TORCH_CHECK(grid_y >= 0, "grid_y must be >= 0 (0 = automatic)");
  check_gfx950("cluster_dist_sums");
  const long long gy = cds_grid_y(Q, G, k, grid_y);
  const long long nqt = (Q + KN_TILE - 1) / KN_TILE;
  TORCH_CHECK(nqt < (1LL << 31), "cluster_dist_sums: too many queries");
  if (gy > 1) {
    TORCH_CHECK(part.has_value(), "cluster_dist_sums: a split over ", gy,
                " blocks needs the partial buffer");
    CHECK_F64(*part);
    check_same_device(Xq, {*part});
    TORCH_CHECK(part->numel() == Q * gy * k, "part must be [Q, ", gy, ", k]");
  }
  if (G > 0)
    TORCH_CHECK(labels.min().item<int>() >= 0 && labels.max().item<int>() < k,
                "cluster_dist_sums: labels must lie in [0, ", k, ")");
  if (Q == 0) return;
  if (G > 0)
    launch(row_sqnorms_kernel, row_wave_grid(G), 0, f32(X), G, h, f32(nx));
  launch(row_sqnorms_kernel, row_wave_grid(Q), 0, f32(Xq), Q, h, f32(nq));
  const dim3 grid((unsigned)nqt, (unsigned)gy);
  double* out = gy > 1 ? f64(*part) : f64(D);
  const int* qi = q_index ? i32(*q_index) : nullptr;
  if (k <= 4)
    launch(cds_tile_kernel<4>, grid, 0, f32(Xq), f32(X), i32(labels), f32(nq),
           f32(nx), qi, Q, G, h, k, out);
  else
    launch(cds_tile_kernel<8>, grid, 0, f32(Xq), f32(X), i32(labels), f32(nq),
           f32(nx), qi, Q, G, h, k, out);
  if (gy > 1)
    launch(cds_fold_kernel, grid_for(Q * k, 256), 0, f64(*part), Q * k, gy, k,
           f64(D));
}

// ------------------------------------------------- native host TSV parser
std::tuple<std::vector<std::string>, std::vector<std::string>, torch::Tensor>
parse_expression_tsv(const std::string& path) {
  std::ifstream f(path);
  TORCH_CHECK(f.good(), "cannot open ", path);
  std::string line;
  TORCH_CHECK(std::getline(f, line), "empty file ", path);
  std::vector<std::string> samples;
  {
    size_t pos = line.find('\t');
    TORCH_CHECK(pos != std::string::npos, "bad header in ", path);
    size_t start = pos + 1;
    while (start <= line.size()) {
      size_t next = line.find('\t', start);
      if (next == std::string::npos) {
        std::string v = line.substr(start);
        while (!v.empty() && (v.back() == '\r' || v.back() == '\n')) v.pop_back();
        if (!v.empty()) samples.push_back(v);
        break;
      }
      samples.push_back(line.substr(start, next - start));
      start = next + 1;
    }
  }
  const size_t S = samples.size();
  std::vector<std::string> genes;
  std::vector<float> vals;
  vals.reserve(S * 4096);
  long long ln = 1;
  while (std::getline(f, line)) {
    ++ln;
    if (line.empty()) continue;
    const char* p = line.c_str();
    const char* tab = std::strchr(p, '\t');
    if (!tab) continue;               // lenient: short rows skipped (like
                                      // the Python fallback)
    genes.emplace_back(p, tab - p);
    const char* q = tab + 1;
    for (size_t i = 0; i < S; ++i) {
      TORCH_CHECK(*q != '\0',
                  path, ":", ln, ": gene '", genes.back(), "' has ", i,
                  " values, expected ", S, " (one per sample column)");
      char* end = nullptr;
      const float v = std::strtof(q, &end);
      TORCH_CHECK(end != q && (*end == '\t' || *end == '\0' ||
                               *end == '\r' || *end == '\n'),
                  path, ":", ln, ": non-numeric expression value for gene '",
                  genes.back(), "'");
      vals.push_back(v);
      const bool last = (i + 1 == S);
      TORCH_CHECK(last || *end == '\t',
                  path, ":", ln, ": gene '", genes.back(), "' has ", i + 1,
                  " values, expected ", S, " (one per sample column)");
      q = (*end == '\t') ? end + 1 : end;
    }
    // trailing extra columns = ragged row
    while (*q == '\r' || *q == '\n') ++q;
    TORCH_CHECK(*q == '\0',
                path, ":", ln, ": gene '", genes.back(),
                "' has more than ", S, " values (one per sample column)");
  }
  TORCH_CHECK(!genes.empty(), path,
              ": no expression rows (empty or header-only file)");
  const size_t G = genes.size();
  auto t = torch::from_blob(vals.data(), {(long long)G, (long long)S},
                            torch::TensorOptions().dtype(at::kFloat))
               .clone();
  // gene-wise -> sample-wise (like the reference transpose, G2Vec.py:498)
  return {genes, samples, t.t().contiguous()};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("random_walks", &random_walks, "CSR biased random walks (gfx950)");
  m.def("cbow_fwd_scalar", &cbow_fwd_scalar, "scalar CBOW forward + loss");
  m.def("scatter_dO_det_", &scatter_dO_det_,
        "deterministic c += X^T dO (one slab, out-arg)");
  m.def("cbow_eval_scan_", &cbow_eval_scan_,
        py::arg("s"), py::arg("genes"), py::arg("pathid"), py::arg("offs"),
        py::arg("labels"), py::arg("p_split"), py::arg("cap"),
        py::arg("piece"), py::arg("counts"),
        py::arg("dO") = py::none(), py::arg("inv_b") = 1.0,
        "instance-parallel fused eval (segmented scan + finish)");
  m.def("cbow_eval_counts_", &cbow_eval_counts_,
        py::arg("s"), py::arg("genes"), py::arg("offs"), py::arg("labels"),
        py::arg("p_split"), py::arg("counts"),
        py::arg("dO") = py::none(), py::arg("inv_b") = 1.0,
        py::arg("partials") = py::none(),
        "fused train/val correct-count eval (in-place counts[2]; partials "
        "[eval_grid, 2] given: written instead, no fold)");
  m.def("eval_grid", &eval_grid, py::arg("P"), py::arg("G"),
        "block count of cbow_eval_counts_ = rows of its partial table");
  m.def("fold_partials_rows_", &fold_partials_rows_, py::arg("partials"),
        py::arg("counts"),
        "counts [K, 2] = fold of K evals' partial tables [K, grid, 2]");
  m.def("adam_rank1", &adam_rank1,
        py::arg("W"), py::arg("m"), py::arg("v"), py::arg("c"),
        py::arg("who"), py::arg("lrt"), py::arg("b1"), py::arg("b2"),
        py::arg("eps"), py::arg("mO") = py::none(), py::arg("vO") = py::none(),
        "TF1 Adam, rank-1 grad (mO/vO given: fused dW_ho + who update)");
  m.def("adam_dense", &adam_dense, "TF1 Adam, dense grad");
  m.def("cbow_fwd", &cbow_fwd,
        py::arg("W"), py::arg("who"), py::arg("genes"), py::arg("offs"),
        py::arg("labels"), py::arg("inv_b"), py::arg("want_grad"),
        py::arg("act") = 0,
        "row-gather CBOW forward (act: 0 linear, 1 ReLU)");
  m.def("cbow_bwd_rows", &cbow_bwd_rows,
        py::arg("who"), py::arg("inst_path"), py::arg("seg_start"),
        py::arg("seg_gene"), py::arg("dO"), py::arg("n_genes"),
        py::arg("Hpre") = py::none(),
        "deterministic scatter CBOW backward (Hpre = ReLU mask source)");
  m.def("pcc_edges", &pcc_edges, "per-edge |PCC|");
  m.def("corr_gemm", &corr_gemm, "MFMA f32 correlation GEMM");
  m.def("trunc_normal_", &trunc_normal_,
        "seeded +-2sigma truncated-normal fill (K9)");
  m.def("gemv_rows_", &gemv_rows_, py::arg("W"), py::arg("x"), py::arg("out"),
        py::arg("clear") = py::none(),
        "s = W @ x (wave-per-row GEMV, out-arg; clear [G] given: zeroed too)");
  m.def("gemv_cols_", &gemv_cols_, "out = W^T c (partials + fold, out-arg)");
  m.def("cbow_eval_counts_rep_", &cbow_eval_counts_rep_,
        py::arg("s_R"), py::arg("genes"), py::arg("offs"), py::arg("labels"),
        py::arg("p_split"), py::arg("counts_R"),
        py::arg("dO_R") = py::none(), py::arg("inv_b") = 1.0,
        "replica-batched fused eval: counts_R [R, 2] + train dlogits dO_R");
  m.def("scatter_dO_rep_", &scatter_dO_rep_,
        "replica-batched deterministic c_R += X^T dO_R (accumulating)");
  m.def("adam_rank1_rep", &adam_rank1_rep,
        "replica-batched fused tail: rank-1 Adam + dW_ho fold + who Adam");
  m.def("gemv_rows_rep_", &gemv_rows_rep_,
        "s_R[:, r] = W[r] @ who[r] (replica-minor out-arg)");
  m.def("bf16_copy", &bf16_copy, "f32 -> bf16 cast kernel");
  m.def("kmeans_step", &kmeans_step,
        py::arg("X"), py::arg("C"), py::arg("prev"), py::arg("labels"),
        py::arg("C_new"), py::arg("sums"), py::arg("counts"),
        py::arg("n_changed"), py::arg("inertia"),
        "one fused Lloyd iteration (assign + sums/counts/inertia + C')");
  m.def("kmeans_mind2_", &kmeans_mind2_,
        "d2 = min(d2, |x - c|^2) for one new centre (k-means++)");
  m.def("row_norms_", &row_norms_, "row L2 norms, f64-accumulated (out-arg)");
  m.def("t_scores_", &t_scores_, "|pooled t| per gene column (out-arg)");
  m.def("col_moments_", &col_moments_,
        "f64 column sums of x and x*x (out-args)");
  m.def("perm_t_stats_", &perm_t_stats_,
        "t^2 per (relabelling, gene), MFMA f32 (out-arg)");
  m.def("perm_t_counts_", &perm_t_counts_,
        "per-gene exceed counts + per-relabelling max t^2 (out-args)");
  m.def("rank_columns_", &rank_columns_, py::arg("expr"), py::arg("ranks"),
        "average ranks per gene column, ties included (out-arg)");
  m.def("ranksum_scores_", &ranksum_scores_, py::arg("expr"),
        py::arg("labels"), py::arg("z"), py::arg("auc"),
        "rank-sum |z| and AUC per gene column (out-args)");
  m.attr("RK_TG") = RK_TG;
  m.attr("RK_SJ") = RK_SJ;
  m.attr("RK_IB") = RK_IB;
  m.attr("RK_WAVES") = RK_WAVES;
  m.attr("RK_MAX_BLOCKS") = RK_MAX_BLOCKS;
  m.def("knn_grid_y", &knn_grid_y, py::arg("Q"), py::arg("G"),
        py::arg("grid_y") = 0, "candidate-split block count of knn_topk_");
  m.def("knn_topk_", &knn_topk_, py::arg("Xq"), py::arg("X"),
        py::arg("q_index"), py::arg("k"), py::arg("grid_y"),
        py::arg("part_idx"), py::arg("part_val"), py::arg("idx"),
        py::arg("val"),
        "k largest dots per query row, MFMA f32 + fused top-k (out-args)");
  m.def("cds_grid_y", &cds_grid_y, py::arg("Q"), py::arg("G"), py::arg("k"),
        py::arg("grid_y") = 0,
        "candidate-split block count of cluster_dist_sums_");
  m.def("cluster_dist_sums_", &cluster_dist_sums_, py::arg("Xq"), py::arg("X"),
        py::arg("labels"), py::arg("q_index"), py::arg("k"), py::arg("grid_y"),
        py::arg("nq"), py::arg("nx"), py::arg("part"), py::arg("D"),
        "per-cluster sums of Euclidean distances per query row, MFMA f32 "
        "dots + f64 sums (out-args)");
  m.def("parse_expression_tsv", &parse_expression_tsv,
        "native expression TSV parser");
}
