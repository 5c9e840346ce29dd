// libpyg.so -- the drop-in operator library.
//
// Registers the reference's operator schemas in namespace `pyg` (byte-identical strings, cited
// per op) and implements them for PyTorch-ROCm tensors by calling the torch-free C-ABI of
// include/pyg_hip.h and nothing else.  PyTorch is plumbing here: argument checks in the
// reference's wording, output allocation through the caching allocator, the current HIP stream,
// the global CPU generator for the sampler's random words, and autograd glue.
//
// One translation unit per operator family.  This one: cuda_version, segment / grouped_matmul with their autograd,
// the fused R-GCN operators and the matmul schedule hooks.  The others: pyg_binding_sampler.cpp (neighbour samplers),
// _walk.cpp, _dist.cpp, _reduce.cpp, _csr.cpp, _classes.cpp, _cpu.cpp and _cpu_reduce.cpp (dispatch key `CPU`).
//
// CPU tensors: the samplers, segment/grouped_matmul and index_sort have their own CPU kernels
// (pyg_binding_cpu.cpp, dispatch key `CPU`); every other op of this library is device-only and a CPU tensor
// reaches the dispatcher's "could not run ... with arguments from the 'CPU' backend" error.  A device tensor
// never takes a CPU path: there is no fallback of any kind.
#include <ATen/ATen.h>
#include <ATen/Context.h>
#include <ATen/core/dispatch/Dispatcher.h>
#include <torch/autograd.h>
#include <torch/library.h>

#include <cstdlib>
#include <string>
#include <vector>

#include "binding_common.h"

namespace pyg_amd {

// ---------------------------------------------------------------------------------------------
// library.cpp:19-29
// ---------------------------------------------------------------------------------------------
int64_t cuda_version() { return pyg_hip_version(); }

int& matmul_schedule_tls() {
  static thread_local int sched = PYG_HIP_MM_SCHED_AUTO;
  return sched;
}

int matmul_flags(at::ScalarType t) {
  int flags = matmul_schedule_tls() & PYG_HIP_MM_SCHED_MASK;
  if (t == at::kFloat && at::globalContext().float32MatmulPrecision() != at::Float32MatmulPrecision::HIGHEST)
    flags |= PYG_HIP_MM_F32_SPLIT;
  return flags;
}

struct ScheduleGuard {
  int prev;
  explicit ScheduleGuard(int s) : prev(matmul_schedule_tls()) { matmul_schedule_tls() = s; }
  ~ScheduleGuard() { matmul_schedule_tls() = prev; }
};

// ---------------------------------------------------------------------------------------------
// matmul  (front: pyg_lib/csrc/ops/matmul.cpp:12-61, kernels: ops/cuda/matmul_kernel.cu:289-319)
// ---------------------------------------------------------------------------------------------
static Tensor segment_matmul_impl(const Tensor& input, const Tensor& ptr, const Tensor& other,
                                  const c10::optional<Tensor>& bias) {
  PYG_TRACE("pyg::segment_matmul");
  at::TensorArg input_arg{input, "input", 0};
  at::TensorArg ptr_arg{ptr, "ptr", 1};
  at::TensorArg other_arg{other, "other", 2};
  at::CheckedFrom c{"segment_matmul"};
  at::checkAllDefined(c, {input_arg, ptr_arg, other_arg});
  at::checkSameType(c, input_arg, other_arg);
  at::checkDim(c, input_arg, 2);
  at::checkDim(c, ptr_arg, 1);
  at::checkDim(c, other_arg, 3);
  at::checkSize(c, other_arg, 1, input_arg->size(-1));
  at::checkNumel(c, ptr_arg, other_arg->size(0) + 1);
  TORCH_CHECK(ptr.scalar_type() == at::kLong, "expected scalar type Long but found ",
              ptr.scalar_type());
  TORCH_CHECK(input.is_cuda() && other.is_cuda() && input.device() == other.device(),
              "segment_matmul: 'input' and 'other' must live on the same HIP device");

  DeviceGuard guard(input.device());
  const auto x = input.contiguous();
  const auto w = other.contiguous();
  const auto p = ptr.contiguous();
  const int64_t N = x.size(0), K = x.size(1), B = w.size(0), M = w.size(2);
  auto out = x.new_empty({N, M});
  Tensor b;
  if (bias.has_value()) {
    b = bias.value().to(x.options()).contiguous();
    TORCH_CHECK(b.dim() == 2 && b.size(0) == B && b.size(1) == M, "segment_matmul: expected 'bias' of shape [",
                B, ", ", M, "]");
  }
  auto ws = at::empty({(int64_t)pyg_hip_matmul_workspace_size(B)}, x.options().dtype(at::kByte));
  check_status(pyg_hip_segment_matmul(dtype_code(x.scalar_type()), x.data_ptr(), p.data_ptr<int64_t>(),
                                      p.is_cuda() ? 1 : 0, w.data_ptr(),
                                      b.defined() ? b.data_ptr() : nullptr, out.data_ptr(), N, K, M, B,
                                      ws.data_ptr(), (size_t)ws.numel(), matmul_flags(x.scalar_type()),
                                      current_stream(x)));
  return out;
}

Tensor segment_matmul_kernel(const Tensor& input, const Tensor& ptr, const Tensor& other) {
  return segment_matmul_impl(input, ptr, other, c10::nullopt);
}

// Extra op of this build: bias fused as GEMM epilogue (the reference adds it in a Python loop of
// B slice updates, pyg_lib/ops/__init__.py:169-171).
Tensor segment_matmul_bias_kernel(const Tensor& input, const Tensor& ptr, const Tensor& other,
                                  const Tensor& bias) {
  return segment_matmul_impl(input, ptr, other, bias);
}

// `caller_pool` (this build's pyg::grouped_matmul_pool): a contiguous [sum of rows, M] tensor that receives the
// outputs as consecutive row ranges -- the sharded driver passes its slot of the all-gather buffer
// (pyg_lib_amd/sharding.py), so the results are produced where the collective reads them.
static std::vector<Tensor> grouped_matmul_impl(const at::TensorList input, const at::TensorList other,
                                               const c10::optional<Tensor>& caller_pool) {
  PYG_TRACE("pyg::grouped_matmul");
  TORCH_CHECK(input.size() == other.size(),
              "Number of 'input' tensors must match number of 'other' tensors");
  const size_t G = input.size();
  std::vector<Tensor> outs;
  if (G == 0) return outs;
  // The reference's argument checks (TensorArg messages naming the offending list entry).  With 512 groups, building
  // 1024 names and TensorArgs up front cost more host time than anything else in the call: look first, and go through
  // the naming checks only when something is wrong (they then raise the reference's message).
  bool plain = input[0].defined();
  for (size_t i = 0; plain && i < G; ++i) {
    const Tensor& a = input[i];
    const Tensor& o = other[i];
    plain = a.defined() && o.defined() && a.scalar_type() == input[0].scalar_type() &&
            o.scalar_type() == input[0].scalar_type() && a.dim() == 2 && o.dim() == 2 && o.size(0) == a.size(1) &&
            a.is_cuda() && o.is_cuda();
  }
  if (!plain) {
    at::CheckedFrom c{"grouped_matmul"};
    for (size_t i = 0; i < G; ++i) {
      const std::string na = "input[" + std::to_string(i) + "]", no = "other[" + std::to_string(i) + "]";
      at::TensorArg a{input[i], na.c_str(), 0};
      at::TensorArg o{other[i], no.c_str(), 1};
      at::checkDefined(c, a);
      at::checkDefined(c, o);
      at::checkScalarType(c, a, input[0].scalar_type());
      at::checkScalarType(c, o, input[0].scalar_type());
      at::checkDim(c, a, 2);
      at::checkDim(c, o, 2);
      at::checkSize(c, o, 0, a->size(-1));
      TORCH_CHECK(input[i].is_cuda() && other[i].is_cuda(), "grouped_matmul: tensors must live on a HIP device");
    }
  }
  DeviceGuard guard(input[0].device());
  std::vector<pyg_hip_group> groups(G);
  std::vector<Tensor> keep;
  keep.reserve(2 * G);
  outs.reserve(G);
  // Weight-gradient pattern of GroupedMatmul.backward (pyg_lib/ops/__init__.py:88-94): every input is
  // the transposed view X_i^T of a row-major X_i [rows_i, K] and the contraction runs over rows_i.
  // One persistent launch of the dW kernel (csrc/hip/matmul_dw.hip) instead of a transposing copy of
  // every X_i and G skinny GEMMs.
  {
    const auto st = input[0].scalar_type();
    bool dw = (st == at::kBFloat16 || st == at::kHalf || st == at::kFloat) && !caller_pool.has_value();
    const int64_t esz = (int64_t)input[0].element_size();
    // every input is a transposed view (tensors that are both -- one row, one column, no elements -- count), at
    // least one of them a real one: a plain forward call never comes here
    bool any_view = false;
    for (size_t i = 0; dw && i < G; ++i) {
      dw = input[i].t().is_contiguous() && other[i].is_contiguous() && input[i].size(0) > 0 && other[i].size(1) > 0 &&
           (uintptr_t)input[i].data_ptr() % esz == 0 && (uintptr_t)other[i].data_ptr() % esz == 0;
      any_view = any_view || !input[i].is_contiguous();
    }
    if (dw && any_view) {
      // per-group shapes: K_i = input[i].size(0), M_i = other[i].size(1); the results lie back to back in one pool
      std::vector<int64_t> poff(G + 1, 0);
      for (size_t i = 0; i < G; ++i) {
        groups[i].input = input[i].data_ptr();  // X_i, row-major [rows_i, K_i]
        groups[i].other = other[i].data_ptr();  // dY_i [rows_i, M_i]
        groups[i].out = nullptr;
        groups[i].rows = input[i].size(1);
        groups[i].k = (int32_t)input[i].size(0);
        groups[i].m = (int32_t)other[i].size(1);
        groups[i].other_trans = 0;
        groups[i].reserved = 0;
        poff[i + 1] = poff[i] + input[i].size(0) * other[i].size(1);
      }
      auto pool = at::empty({poff[G]}, input[0].options());
      auto ws = at::empty({(int64_t)pyg_hip_grouped_matmul_dw_workspace_size(groups.data(), (int64_t)G)},
                          input[0].options().dtype(at::kByte));
      const int rc = pyg_hip_grouped_matmul_dw(dtype_code(st), groups.data(), (int64_t)G, pool.data_ptr(), ws.data_ptr(),
                                               (size_t)ws.numel(), current_stream(input[0]));
      if (rc == PYG_HIP_OK) {
        // plain aliases of the pool, not tracked views: the reference returns G independent tensors, and
        // outputs that are "views of a multi-output function" could not be modified in place by the caller
        at::AutoDispatchBelowADInplaceOrView untracked;
        for (size_t i = 0; i < G; ++i)
          outs.push_back(pool.as_strided({input[i].size(0), other[i].size(1)}, {other[i].size(1), 1}, poff[i]));
        return outs;
      }
      TORCH_CHECK(rc == PYG_HIP_ERR_UNSUPPORTED, pyg_hip_last_error());
    }
  }
  // One allocation for all outputs (the reference makes G of them, matmul_kernel.cpp:296-298); each
  // output is a 16-byte aligned view into it.
  const int64_t elt = (int64_t)input[0].element_size();
  const int64_t align = 16 / elt > 0 ? 16 / elt : 1;
  std::vector<int64_t> offs(G);
  int64_t total = 0;
  for (size_t i = 0; i < G; ++i) {
    offs[i] = total;
    const int64_t n = input[i].size(0) * other[i].size(-1);
    total += (n + align - 1) / align * align;
  }
  Tensor pool;
  if (caller_pool.has_value()) {
    pool = caller_pool.value();
    const int64_t M0 = other[0].size(-1);
    int64_t rows = 0;
    for (size_t i = 0; i < G; ++i) {
      TORCH_CHECK(other[i].size(-1) == M0, "grouped_matmul_pool: every 'other' must have the same number of columns");
      rows += input[i].size(0);
    }
    TORCH_CHECK(pool.dim() == 2 && pool.size(0) == rows && pool.size(1) == M0 && pool.is_contiguous() &&
                    pool.scalar_type() == input[0].scalar_type() && pool.device() == input[0].device(),
                "grouped_matmul_pool: expected a contiguous 'pool' of shape [", rows, ", ", M0, "] like 'input'");
    TORCH_CHECK((M0 * elt) % 16 == 0 || G == 1, "grouped_matmul_pool: rows of 'pool' must be 16-byte multiples");
    total = 0;
    for (size_t i = 0; i < G; ++i) {
      offs[i] = total;
      total += input[i].size(0) * M0;
    }
    pool = pool.view({-1});
  } else {
    pool = at::empty({std::max<int64_t>(total, 1)}, input[0].options());
  }
  char* const pool_base = static_cast<char*>(pool.data_ptr());
  for (size_t i = 0; i < G; ++i) {
    Tensor a = input[i];
    if (!a.is_contiguous()) {
      a = a.contiguous();
      keep.push_back(a);
    }
    Tensor o = other[i];
    int trans = 0;
    if (!o.is_contiguous()) {
      // a transposed view (backward pass, pyg_lib/ops/__init__.py:84,91) is read in place
      if (o.t().is_contiguous()) {
        trans = 1;
      } else {
        o = o.contiguous();
        keep.push_back(o);
      }
    }
    groups[i].input = a.data_ptr();
    groups[i].other = o.data_ptr();
    groups[i].out = pool_base + offs[i] * elt;
    groups[i].rows = a.size(0);
    groups[i].k = (int32_t)a.size(1);
    groups[i].m = (int32_t)other[i].size(-1);
    groups[i].other_trans = trans;
    groups[i].reserved = 0;
  }
  auto ws = at::empty({(int64_t)pyg_hip_matmul_workspace_size((int64_t)G)},
                      input[0].options().dtype(at::kByte));
  check_status(pyg_hip_grouped_matmul(dtype_code(input[0].scalar_type()), groups.data(), (int64_t)G,
                                      ws.data_ptr(), (size_t)ws.numel(), matmul_flags(input[0].scalar_type()),
                                      current_stream(input[0])));
  // the outputs: one dispatcher call each, made while the kernel runs (aliases of the pool that are NOT tracked as
  // views, see above).  as_strided takes an offset into the STORAGE: a caller's pool may be a view that starts inside it.
  at::AutoDispatchBelowADInplaceOrView untracked;
  const int64_t base = pool.storage_offset();
  for (size_t i = 0; i < G; ++i)
    outs.push_back(pool.as_strided({input[i].size(0), other[i].size(-1)}, {other[i].size(-1), 1}, base + offs[i]));
  return outs;
}

std::vector<Tensor> grouped_matmul_kernel(const at::TensorList input, const at::TensorList other) {
  return grouped_matmul_impl(input, other, c10::nullopt);
}

std::vector<Tensor> grouped_matmul_pool_kernel(const at::TensorList input, const at::TensorList other, Tensor pool) {
  return grouped_matmul_impl(input, other, pool);
}

// This build only: gather -> per-relation matmul -> scatter-add in one launch (csrc/hip/rgcn.hip).  `out` is
// accumulated into and returned.  Indices are validated on the device (rgcn_check_flags).
static int rgcn_check_flags() {
  // default: validated on the device without a synchronisation (PYG_HIP_RGCN_DEFERRED: a stale node id is redirected to
  // row 0 instead of reading out of bounds, and reported by the next call); 1: validated, synchronising, fails in the
  // call that has the bad index; 0: no validation (the round-4 behaviour)
  static const int flags = [] {
    const char* e = getenv("PYG_HIP_RGCN_CHECK");
    if (e == nullptr || e[0] == '\0') return PYG_HIP_RGCN_DEFERRED;
    return e[0] == '0' ? 0 : PYG_HIP_RGCN_CHECKED;
  }();
  return flags;
}

static void rgcn_index_checks(const at::TensorList gather_index, const at::TensorList scatter_index, const Tensor& like,
                              size_t r) {
  TORCH_CHECK(gather_index[r].scalar_type() == at::kLong && scatter_index[r].scalar_type() == at::kLong &&
                  gather_index[r].dim() == 1 && gather_index[r].sizes() == scatter_index[r].sizes(),
              "rgcn_fused: index vectors must be 1-D int64 tensors of equal length");
  TORCH_CHECK(gather_index[r].device() == like.device() && scatter_index[r].device() == like.device(),
              "rgcn_fused: index vectors must live on the device of the features (got ", gather_index[r].device(), " / ",
              scatter_index[r].device(), " vs ", like.device(), ")");
}

// The feature tables of rgcn_fused_tables: relation r gathers row node_id[gather_type[r]][gather_index[r][e]] of
// feat[gather_type[r]] (contiguous copies of both).  rgcn_fused has none: every relation reads the call's x at its gather_offset.
struct RgcnTables {
  const std::vector<Tensor>& feat;
  const std::vector<Tensor>& node_id;
  at::IntArrayRef gather_type;
};

// The relation array, the workspace and the call of both operators.  `like`: a feature tensor (device, stream); x / x_rows: the
// call's own feature matrix (rgcn_fused) or nullptr / 0 with `tables`.
// `grouped`: every scatter_index is nondecreasing (the samplers' `row`): the atomic-free owner-computes kernel
// (PYG_HIP_RGCN_GROUPED) WRITES `out` -- deterministic, no zero fill needed; verified on the device (rgcn_check_flags)
static Tensor rgcn_call(const Tensor& like, const void* x, int64_t x_rows, const at::TensorList gather_index,
                        const at::TensorList scatter_index, const int64_t* gather_offset, at::IntArrayRef scatter_offset,
                        const Tensor& wc, Tensor out, bool grouped, at::OptionalIntArrayRef scatter_rows, const RgcnTables* tables) {
  const size_t R = gather_index.size();
  std::vector<pyg_hip_rgcn_relation> rels(R);
  std::vector<Tensor> keep;
  int64_t E = 0;
  for (size_t r = 0; r < R; ++r) {
    rgcn_index_checks(gather_index, scatter_index, like, r);
    auto g = gather_index[r].contiguous();
    auto s = scatter_index[r].contiguous();
    rels[r] = pyg_hip_rgcn_relation{};
    rels[r].gather_index = g.data_ptr<int64_t>();
    rels[r].scatter_index = s.data_ptr<int64_t>();
    rels[r].num_edges = g.numel();
    rels[r].gather_offset = gather_offset ? gather_offset[r] : 0;
    rels[r].scatter_offset = scatter_offset[r];
    rels[r].scatter_rows = scatter_rows.has_value() ? (*scatter_rows)[r] : 0;
    rels[r].weight = static_cast<const char*>(wc.data_ptr()) + (int64_t)r * wc.size(1) * wc.size(2) * wc.element_size();
    if (tables) {
      TORCH_CHECK(tables->gather_type[r] >= 0 && (size_t)tables->gather_type[r] < tables->feat.size(),
                  "rgcn_fused_tables: gather_type out of range");
      const Tensor& f = tables->feat[(size_t)tables->gather_type[r]];
      const Tensor& n = tables->node_id[(size_t)tables->gather_type[r]];
      rels[r].x = f.data_ptr();
      rels[r].gather_map = n.data_ptr<int64_t>();
      rels[r].x_rows = f.size(0);
      rels[r].gather_map_len = n.numel();
    }
    E += g.numel();
    keep.push_back(g);
    keep.push_back(s);
  }
  const size_t bytes = grouped ? pyg_hip_rgcn_grouped_workspace_size(rels.data(), (int64_t)R, out.size(0))
                               : pyg_hip_rgcn_fused_workspace_size((int64_t)R, E);
  auto ws = at::empty({(int64_t)bytes}, like.options().dtype(at::kByte));
  check_status(pyg_hip_rgcn_fused(dtype_code(wc.scalar_type()), x, x_rows, rels.data(), (int64_t)R, out.data_ptr(), out.size(0),
                                  wc.size(1), out.size(1), rgcn_check_flags() | (grouped ? PYG_HIP_RGCN_GROUPED : 0),
                                  ws.data_ptr(), (size_t)ws.numel(), current_stream(like)));
  return out;
}

Tensor rgcn_fused_kernel(const Tensor& x, const at::TensorList gather_index, const at::TensorList scatter_index,
                         at::IntArrayRef gather_offset, at::IntArrayRef scatter_offset, const Tensor& weight, Tensor out,
                         bool grouped, at::OptionalIntArrayRef scatter_rows) {
  PYG_TRACE("pyg::rgcn_fused");
  // packed 16-bit atomic adds: the result depends on the order they land in (pyg_lib_amd.rgcn takes the atomic-free
  // three-op chain under torch.use_deterministic_algorithms(True) instead of calling this operator); grouped: no atomics
  if (!grouped) at::globalContext().alertNotDeterministic("pyg::rgcn_fused");
  const size_t R = gather_index.size();
  TORCH_CHECK(scatter_index.size() == R && gather_offset.size() == R && scatter_offset.size() == R &&
                  (!scatter_rows.has_value() || scatter_rows->size() == R),
              "rgcn_fused: one gather / scatter index vector and offset (and scatter_rows entry) per relation expected");
  TORCH_CHECK(x.is_cuda() && weight.is_cuda() && out.is_cuda() && x.device() == weight.device() && x.device() == out.device(),
              "rgcn_fused: tensors must live on the same HIP device");
  TORCH_CHECK(x.dim() == 2 && out.dim() == 2 && weight.dim() == 3 && (size_t)weight.size(0) == R &&
                  weight.size(1) == x.size(1) && weight.size(2) == out.size(1),
              "rgcn_fused: expected x [N, K], weight [R, K, M], out [N_out, M]");
  TORCH_CHECK(x.scalar_type() == weight.scalar_type() && x.scalar_type() == out.scalar_type(), "rgcn_fused: dtype mismatch");
  TORCH_CHECK(out.is_contiguous(), "rgcn_fused: 'out' must be contiguous");
  DeviceGuard guard(x.device());
  const auto xc = x.contiguous();
  return rgcn_call(x, xc.data_ptr(), xc.size(0), gather_index, scatter_index, gather_offset.data(), scatter_offset,
                   weight.contiguous(), out, grouped, scatter_rows, nullptr);
}

// The same without the per-batch feature matrix: relation r gathers row node_id[gather_type[r]][gather_index[r][e]] of
// the GLOBAL feature table feat[gather_type[r]] -- what `x = cat([feat[t][node_id[t]] ...])` followed by rgcn_fused
// computes, minus the ATen gathers, the cat and the [sum n_t, K] intermediate.
Tensor rgcn_fused_tables_kernel(const at::TensorList feat, const at::TensorList node_id, at::IntArrayRef gather_type,
                                const at::TensorList gather_index, const at::TensorList scatter_index,
                                at::IntArrayRef scatter_offset, const Tensor& weight, Tensor out, bool grouped,
                                at::OptionalIntArrayRef scatter_rows) {
  PYG_TRACE("pyg::rgcn_fused_tables");
  if (!grouped) at::globalContext().alertNotDeterministic("pyg::rgcn_fused_tables");  // (see rgcn_fused_kernel)
  const size_t R = gather_index.size(), T = feat.size();
  TORCH_CHECK(T > 0 && node_id.size() == T, "rgcn_fused_tables: one node-id vector per feature table expected");
  TORCH_CHECK(scatter_index.size() == R && gather_type.size() == R && scatter_offset.size() == R &&
                  (!scatter_rows.has_value() || scatter_rows->size() == R),
              "rgcn_fused_tables: one gather type, gather / scatter index vector and offset (and scatter_rows entry) per relation expected");
  const Tensor& f0 = feat[0];
  TORCH_CHECK(f0.is_cuda() && weight.is_cuda() && out.is_cuda() && f0.device() == weight.device() && f0.device() == out.device(),
              "rgcn_fused_tables: tensors must live on the same HIP device");
  TORCH_CHECK(out.dim() == 2 && weight.dim() == 3 && (size_t)weight.size(0) == R && weight.size(2) == out.size(1),
              "rgcn_fused_tables: expected weight [R, K, M], out [N_out, M]");
  TORCH_CHECK(out.is_contiguous() && out.scalar_type() == weight.scalar_type(), "rgcn_fused_tables: 'out' must be contiguous and typed like 'weight'");
  DeviceGuard guard(f0.device());
  std::vector<Tensor> fc(T), nc(T);
  for (size_t t = 0; t < T; ++t) {
    TORCH_CHECK(feat[t].dim() == 2 && feat[t].size(1) == weight.size(1) && feat[t].scalar_type() == weight.scalar_type() &&
                    feat[t].device() == f0.device(),
                "rgcn_fused_tables: feat[", t, "] must be [N_t, K] on the common device and typed like 'weight'");
    TORCH_CHECK(node_id[t].dim() == 1 && node_id[t].scalar_type() == at::kLong && node_id[t].device() == f0.device(),
                "rgcn_fused_tables: node_id[", t, "] must be a 1-D int64 tensor on the common device");
    fc[t] = feat[t].contiguous();
    nc[t] = node_id[t].contiguous();
  }
  const RgcnTables tables{fc, nc, gather_type};
  return rgcn_call(f0, nullptr, 0, gather_index, scatter_index, nullptr, scatter_offset, weight.contiguous(), out, grouped,
                   scatter_rows, &tables);
}

// Autograd, mirroring SegmentMatmul (pyg_lib/csrc/ops/autograd/matmul_kernel.cpp:68-111).
static Tensor segment_matmul_below_autograd(const Tensor& input, const Tensor& ptr, const Tensor& other) {
  static auto op = c10::Dispatcher::singleton()
                       .findSchemaOrThrow("pyg::segment_matmul", "")
                       .typed<Tensor(const Tensor&, const Tensor&, const Tensor&)>();
  return op.call(input, ptr, other);
}

// dW through the C-ABI; returns an undefined tensor when the device kernel does not cover the case.
static Tensor segment_matmul_dw(const Tensor& input, const Tensor& ptr, const Tensor& grad_out, int64_t B) {
  PYG_TRACE("pyg::segment_matmul_backward_dw");
  const auto st = input.scalar_type();
  if (!input.is_cuda()) return Tensor();  // CPU tensors: the reference formula below
  if (st != at::kBFloat16 && st != at::kHalf && st != at::kFloat) return Tensor();
  const int64_t K = input.size(1), M = grad_out.size(1);
  if (B == 0 || K == 0 || M == 0) return at::empty({B, K, M}, input.options());
  DeviceGuard guard(input.device());
  auto x = input.contiguous();
  auto gy = grad_out.contiguous();
  auto p = ptr.contiguous();
  auto out = at::empty({B, K, M}, input.options());
  auto ws = at::empty({(int64_t)pyg_hip_segment_matmul_dw_workspace_size(B, K, M)}, x.options().dtype(at::kByte));
  const int rc = pyg_hip_segment_matmul_dw(dtype_code(st), x.data_ptr(), p.data_ptr<int64_t>(), p.is_cuda() ? 1 : 0,
                                           gy.data_ptr(), out.data_ptr(), x.size(0), K, M, B, ws.data_ptr(),
                                           (size_t)ws.numel(), current_stream(x));
  if (rc == PYG_HIP_ERR_UNSUPPORTED) return Tensor();
  check_status(rc);
  return out;
}

class SegmentMatmul : public torch::autograd::Function<SegmentMatmul> {
 public:
  static torch::autograd::variable_list forward(torch::autograd::AutogradContext* ctx,
                                                const Tensor& input, const Tensor& ptr,
                                                const Tensor& other) {
    at::AutoDispatchBelowADInplaceOrView g;
    Tensor out = segment_matmul_below_autograd(input, ptr, other);
    ctx->save_for_backward({input, ptr, other});
    ctx->saved_data["sched"] = (int64_t)matmul_schedule_tls();
    return {out};
  }

  static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx,
                                                 torch::autograd::variable_list grad_outs) {
    const auto grad_out = grad_outs[0];
    const auto saved = ctx->get_saved_variables();
    const auto input = saved[0], ptr = saved[1], other = saved[2];
    ScheduleGuard sched((int)ctx->saved_data["sched"].toInt());
    Tensor input_grad, other_grad;
    if (torch::autograd::any_variable_requires_grad({input})) {
      // dX = segment_matmul(dY, ptr, W^T)
      input_grad = segment_matmul_below_autograd(grad_out, ptr, other.transpose(-2, -1));
    }
    if (torch::autograd::any_variable_requires_grad({other})) {
      // dW[b] = X_b^T @ dY_b: one persistent MFMA launch for bf16 / f16 / fp32 and any (K, M) (csrc/hip/matmul_dw.hip,
      // matmul_dw_gen.hip) ...
      other_grad = segment_matmul_dw(input, ptr, grad_out, other.size(0));
    }
    if (torch::autograd::any_variable_requires_grad({other}) && !other_grad.defined()) {
      // ... the reference's per-relation formula elsewhere (fp64, integer types, CPU tensors)
      const auto size = (ptr.narrow(0, 1, ptr.numel() - 1) - ptr.narrow(0, 0, ptr.numel() - 1)).cpu();
      const auto sizes = at::IntArrayRef(size.data_ptr<int64_t>(), (size_t)size.numel());
      const auto xs = input.split_with_sizes(sizes, 0);
      const auto gs = grad_out.split_with_sizes(sizes, 0);
      std::vector<Tensor> parts;
      parts.reserve(xs.size());
      for (size_t i = 0; i < xs.size(); ++i) parts.push_back(at::matmul(xs[i].t(), gs[i]));
      other_grad = at::stack(parts);
    }
    return {input_grad, Tensor(), other_grad};
  }
};

Tensor segment_matmul_autograd(const Tensor& input, const Tensor& ptr, const Tensor& other) {
  return SegmentMatmul::apply(input, ptr, other)[0];
}

// This build only: the weight gradient as an operator of its own,
//   grad_other[b] = input[ptr[b]:ptr[b+1]]^T @ grad_out[ptr[b]:ptr[b+1]]     ([B, K, M], B = ptr.numel() - 1),
// for callers that hold X and dY but never ran the forward through autograd (the backward of the fused R-GCN layer,
// pyg_lib_amd/rgcn.py).  Same kernels as SegmentMatmul::backward; bf16 / f16 / fp32 on the device.
Tensor segment_matmul_grad_other_kernel(const Tensor& input, const Tensor& ptr, const Tensor& grad_out) {
  TORCH_CHECK(input.dim() == 2 && grad_out.dim() == 2 && ptr.dim() == 1 && ptr.numel() >= 1 &&
                  input.size(0) == grad_out.size(0),
              "segment_matmul_grad_other: expected input [N, K], ptr [B + 1], grad_out [N, M]");
  TORCH_CHECK(ptr.scalar_type() == at::kLong, "expected scalar type Long but found ", ptr.scalar_type());
  TORCH_CHECK(input.is_cuda() && grad_out.is_cuda() && input.device() == grad_out.device() &&
                  input.scalar_type() == grad_out.scalar_type(),
              "segment_matmul_grad_other: 'input' and 'grad_out' must share device and dtype");
  Tensor out = segment_matmul_dw(input, ptr, grad_out, ptr.numel() - 1);
  TORCH_CHECK(out.defined(), "segment_matmul_grad_other: float32 / bfloat16 / float16 only (got ", input.scalar_type(), ")");
  return out;
}

// ---------------------------------------------------------------------------------------------
// registration
// ---------------------------------------------------------------------------------------------
TORCH_LIBRARY_FRAGMENT(pyg, m) {
  // pyg_lib/csrc/library.cpp:27-29
  m.def("cuda_version", &cuda_version);
  // pyg_lib/csrc/ops/matmul.cpp:63-68
  m.def(TORCH_SELECTIVE_SCHEMA("pyg::grouped_matmul(Tensor[] input, Tensor[] other) -> Tensor[]"));
  m.def(TORCH_SELECTIVE_SCHEMA("pyg::segment_matmul(Tensor input, Tensor ptr, Tensor other) -> Tensor"));
  // this build only: bias as a fused epilogue
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::segment_matmul_bias(Tensor input, Tensor ptr, Tensor other, Tensor bias) -> Tensor"));
  // this build only: the weight gradient of segment_matmul as its own operator
  m.def(TORCH_SELECTIVE_SCHEMA("pyg::segment_matmul_grad_other(Tensor input, Tensor ptr, Tensor grad_out) -> Tensor"));
  // this build only: fused R-GCN aggregation (gather -> per-relation matmul -> scatter-add), csrc/hip/rgcn.hip
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::rgcn_fused(Tensor x, Tensor[] gather_index, Tensor[] scatter_index, int[] gather_offset, "
      "int[] scatter_offset, Tensor weight, Tensor(a!) out, bool grouped = False, int[]? scatter_rows = None) -> Tensor(a!)"));
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::rgcn_fused_tables(Tensor[] feat, Tensor[] node_id, int[] gather_type, Tensor[] gather_index, "
      "Tensor[] scatter_index, int[] scatter_offset, Tensor weight, Tensor(a!) out, bool grouped = False, "
      "int[]? scatter_rows = None) -> Tensor(a!)"));
  // this build only: grouped_matmul writing into a caller-provided [sum rows, M] pool (sharded driver)
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::grouped_matmul_pool(Tensor[] input, Tensor[] other, Tensor(a!) pool) -> Tensor[]"));
}

// HIP tensors dispatch under the CUDA key on PyTorch-ROCm.
TORCH_LIBRARY_IMPL(pyg, CUDA, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::grouped_matmul"), TORCH_FN(grouped_matmul_kernel));
  m.impl(TORCH_SELECTIVE_NAME("pyg::segment_matmul"), TORCH_FN(segment_matmul_kernel));
  m.impl(TORCH_SELECTIVE_NAME("pyg::segment_matmul_bias"), TORCH_FN(segment_matmul_bias_kernel));
  m.impl(TORCH_SELECTIVE_NAME("pyg::segment_matmul_grad_other"), TORCH_FN(segment_matmul_grad_other_kernel));
  m.impl(TORCH_SELECTIVE_NAME("pyg::grouped_matmul_pool"), TORCH_FN(grouped_matmul_pool_kernel));
  m.impl(TORCH_SELECTIVE_NAME("pyg::rgcn_fused_tables"), TORCH_FN(rgcn_fused_tables_kernel));
  m.impl(TORCH_SELECTIVE_NAME("pyg::rgcn_fused"), TORCH_FN(rgcn_fused_kernel));
}

// pyg_lib/csrc/ops/autograd/matmul_kernel.cpp:121-124
TORCH_LIBRARY_IMPL(pyg, Autograd, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::segment_matmul"), TORCH_FN(segment_matmul_autograd));
}

}  // namespace pyg_amd

// Test / measurement hook of libpyg.so (not an operator): tile schedule of the matmul calls made from the calling
// thread (PYG_HIP_MM_SCHED_* of include/pyg_hip.h), returned to automatic by 0.  Thread-local by design.
extern "C" __attribute__((visibility("default"))) void pyg_binding_set_matmul_schedule(int mode) {
  pyg_amd::matmul_schedule_tls() = (mode >= 0 && mode <= PYG_HIP_MM_SCHED_RING) ? mode : PYG_HIP_MM_SCHED_AUTO;
}
extern "C" __attribute__((visibility("default"))) int pyg_binding_get_matmul_schedule(void) {
  return pyg_amd::matmul_schedule_tls();
}
