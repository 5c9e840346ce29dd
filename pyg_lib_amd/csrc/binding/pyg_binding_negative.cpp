// torch::Library binding of pyg::edge_lookup, pyg::negative_sample_keyed and pyg::negative_sample (this build only: the
// reference has no operator for either; PyG composes negative sampling in Python from hashing, isin and retries).
//   edge_lookup            position in `col` of the edge (src[q], dst[q]) of a CSR graph, or -1.
//   negative_sample_keyed  the deterministic core: exact uniform draws over the non-edges of a row (structured form, with
//                          `src`) or of the whole matrix (global form, src = None); a pure function of its arguments
//                          (specification: include/pyg_hip.h, "Edge lookup and negative sampling", and DESIGN.md 2.18),
//                          the same bit for bit on both keys.  Integer arithmetic only.
//   negative_sample        draws one 64-bit key from the torch generator of the tensors' device and calls the core.
// No operator reads a device value on the host or allocates beyond its output, so edge_lookup and the keyed form can be
// captured into a graph.
//   CUDA: csrc/hip/negative.hip through the C-ABI.
//   CPU:  the specification in plain C++ on at::Philox4_32 and unsigned __int128 (negative_cpu.h), items in parallel.
#include <ATen/CPUGeneratorImpl.h>
#include <ATen/Parallel.h>
#include <ATen/TensorUtils.h>
#include <ATen/hip/HIPGeneratorImpl.h>
#include <torch/library.h>

#include <algorithm>
#include <limits>
#include <mutex>

#include "binding_common.h"
#include "negative_cpu.h"

namespace pyg_amd {
namespace {

using OptTensor = std::optional<Tensor>;

inline bool given(const OptTensor& t) { return t.has_value() && t->defined(); }

// what both keys and both samplers need to know about a call, from sizes alone
struct Shape {
  int64_t num_src, num_edges, S, items, G, T;
  bool structured;
};

void check_index_tensors(const char* op, std::initializer_list<std::pair<const Tensor*, const char*>> tensors) {
  const Tensor& first = *tensors.begin()->first;
  TORCH_CHECK(first.scalar_type() == at::kInt || first.scalar_type() == at::kLong, op,
              ": int32 or int64 indices expected (got ", first.scalar_type(), ")");
  for (const auto& [t, name] : tensors) {
    TORCH_CHECK(t->defined(), op, ": '", name, "' is undefined");
    TORCH_CHECK(t->scalar_type() == first.scalar_type(), op, ": '", name, "' has dtype ", t->scalar_type(),
                ", 'rowptr' has ", first.scalar_type(), " (all index tensors must share one dtype)");
    TORCH_CHECK(t->device() == first.device(), op, ": '", name, "' lives on ", t->device(), ", 'rowptr' on ", first.device(),
                " (all tensors must live on the same device)");
    TORCH_CHECK(t->dim() == 1, op, ": '", name, "' must be a vector");
  }
  TORCH_CHECK(first.numel() >= 1, op, ": 'rowptr' must have at least one entry");
}

void check_lookup_args(const Tensor& rowptr, const Tensor& col, const Tensor& src, const Tensor& dst) {
  check_index_tensors("edge_lookup", {{&rowptr, "rowptr"}, {&col, "col"}, {&src, "src"}, {&dst, "dst"}});
  TORCH_CHECK(src.numel() == dst.numel(), "edge_lookup: 'src' has ", src.numel(), " entries, 'dst' has ", dst.numel());
}

Shape check_sample_args(const Tensor& rowptr, const Tensor& col, const OptTensor& src, int64_t num_dst, int64_t num_neg,
                        bool exclude_self, const OptTensor& ptr) {
  const char* op = "negative_sample";
  check_index_tensors(op, {{&rowptr, "rowptr"}, {&col, "col"}});
  if (given(src)) check_index_tensors(op, {{&rowptr, "rowptr"}, {&*src, "src"}});
  if (given(ptr)) check_index_tensors(op, {{&rowptr, "rowptr"}, {&*ptr, "ptr"}});
  TORCH_CHECK(num_dst >= 0, op, ": 'num_dst' must be non-negative (got ", num_dst, ")");
  TORCH_CHECK(num_neg >= 0, op, ": 'num_neg' must be non-negative (got ", num_neg, ")");
  TORCH_CHECK(rowptr.scalar_type() == at::kLong || num_dst <= std::numeric_limits<int32_t>::max(), op,
              ": 'num_dst' = ", num_dst, " does not fit the int32 indices");
  Shape sh{};
  sh.num_src = rowptr.numel() - 1;
  sh.num_edges = col.numel();
  sh.structured = given(src);
  int64_t cells = 0;
  TORCH_CHECK(!__builtin_mul_overflow(sh.num_src, num_dst, &cells), op, ": num_src * num_dst = ", sh.num_src, " * ", num_dst,
              " overflows int64");
  sh.T = cells - sh.num_edges;
  if (sh.structured) {
    sh.S = src->numel();
    TORCH_CHECK(!__builtin_mul_overflow(sh.S, num_neg, &sh.items), op, ": ", sh.S, " x ", num_neg, " samples overflow int64");
    if (given(ptr)) {
      TORCH_CHECK(ptr->numel() >= 1, op, ": 'ptr' must have at least one entry");
      sh.G = ptr->numel() - 1;
    }
  } else {
    TORCH_CHECK(!exclude_self, op, ": 'exclude_self' needs 'src' (the global form, src=None, does not have it)");
    TORCH_CHECK(!given(ptr), op, ": 'ptr' needs 'src' (the global form, src=None, does not have it)");
    sh.items = num_neg;
  }
  return sh;
}

Tensor empty_result(const Shape& sh, int64_t num_neg, const Tensor& like) {
  return at::empty({sh.structured ? sh.S : 2, num_neg}, like.options());
}

// ---- CUDA ----------------------------------------------------------------------------------------------------------

Tensor edge_lookup_cuda(const Tensor& rowptr, const Tensor& col, const Tensor& src, const Tensor& dst) {
  PYG_TRACE("pyg::edge_lookup");
  TORCH_CHECK(rowptr.defined() && rowptr.is_cuda(), "'rowptr' must be a CUDA tensor");
  check_lookup_args(rowptr, col, src, dst);
  DeviceGuard guard(rowptr.device());
  const auto rowptr_c = rowptr.contiguous(), col_c = col.contiguous(), src_c = src.contiguous(), dst_c = dst.contiguous();
  auto out = at::empty({src.numel()}, src.options());
  check_status(pyg_hip_edge_lookup(dtype_code(rowptr.scalar_type()), rowptr_c.data_ptr(), rowptr_c.numel() - 1,
                                   col_c.data_ptr(), col_c.numel(), src_c.data_ptr(), dst_c.data_ptr(), src_c.numel(),
                                   out.data_ptr(), current_stream(rowptr)));
  return out;
}

Tensor negative_sample_keyed_cuda(const Tensor& rowptr, const Tensor& col, const OptTensor& src, int64_t num_dst,
                                  int64_t num_neg, int64_t key, bool exclude_self, const OptTensor& ptr) {
  PYG_TRACE("pyg::negative_sample_keyed");
  TORCH_CHECK(rowptr.defined() && rowptr.is_cuda(), "'rowptr' must be a CUDA tensor");
  const Shape sh = check_sample_args(rowptr, col, src, num_dst, num_neg, exclude_self, ptr);
  DeviceGuard guard(rowptr.device());
  const auto rowptr_c = rowptr.contiguous(), col_c = col.contiguous();
  const Tensor src_c = sh.structured ? src->contiguous() : Tensor();
  const Tensor ptr_c = given(ptr) ? ptr->contiguous() : Tensor();
  auto out = empty_result(sh, num_neg, rowptr);
  // The C-ABI tells the two forms apart by `src` being NULL, and an empty tensor's data_ptr() is NULL too: a structured
  // call without sources (or any call without samples) is answered here.
  if (sh.items == 0) return out;
  check_status(pyg_hip_negative_sample(dtype_code(rowptr.scalar_type()), rowptr_c.data_ptr(), sh.num_src, col_c.data_ptr(),
                                       sh.num_edges, sh.structured ? src_c.data_ptr() : nullptr, sh.S, num_dst, num_neg,
                                       (uint64_t)key, exclude_self ? 1 : 0, given(ptr) ? ptr_c.data_ptr() : nullptr, sh.G,
                                       out.data_ptr(), current_stream(rowptr)));
  return out;
}

Tensor negative_sample_cuda(const Tensor& rowptr, const Tensor& col, const OptTensor& src, int64_t num_dst, int64_t num_neg,
                            bool exclude_self, const OptTensor& ptr) {
  TORCH_CHECK(rowptr.defined() && rowptr.is_cuda(), "'rowptr' must be a CUDA tensor");
  check_sample_args(rowptr, col, src, num_dst, num_neg, exclude_self, ptr);  // a call that raises draws no key
  DeviceGuard guard(rowptr.device());
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  TORCH_CHECK(hipStreamIsCapturing(current_hip_stream((c10::DeviceIndex)rowptr.get_device()), &capturing) == hipSuccess,
              "negative_sample: hipStreamIsCapturing failed");
  TORCH_CHECK(capturing == hipStreamCaptureStatusNone,
              "negative_sample: draws its key from the generator on the host and cannot be captured into a graph (every "
              "replay would repeat the same samples); capture negative_sample_keyed with a key of your own instead");
  auto* gen = at::get_generator_or_default<at::CUDAGeneratorImpl>(
      c10::nullopt, at::cuda::detail::getDefaultCUDAGenerator(rowptr.get_device()));
  std::pair<uint64_t, uint64_t> inputs;
  {
    std::lock_guard<std::mutex> lock(gen->mutex_);
    inputs = gen->philox_engine_inputs(4);
  }
  return negative_sample_keyed_cuda(rowptr, col, src, num_dst, num_neg, (int64_t)mix_key(inputs.first, inputs.second),
                                    exclude_self, ptr);
}

// ---- CPU -----------------------------------------------------------------------------------------------------------
// The items are those of negative_cpu.h, run in parallel.

template <typename scalar_t>
void edge_lookup_cpu_t(const scalar_t* rp, const scalar_t* cl, const scalar_t* src, const scalar_t* dst, scalar_t* out,
                       int64_t num_src, int64_t E, int64_t Q) {
  at::parallel_for(0, Q, 1024, [&](int64_t begin, int64_t end) {
    for (int64_t q = begin; q < end; ++q)
      out[q] = (scalar_t)negative::lookup_item(rp, cl, num_src, E, (int64_t)src[q], (int64_t)dst[q]);
  });
}

template <typename scalar_t>
void negative_structured_cpu_t(const scalar_t* rp, const scalar_t* cl, const scalar_t* src, const scalar_t* ptr,
                               scalar_t* out, const Shape& sh, int64_t num_dst, int64_t num_neg, uint64_t key,
                               bool exclude_self) {
  at::parallel_for(0, sh.items, 256, [&](int64_t begin, int64_t end) {
    for (int64_t t = begin; t < end; ++t)
      out[t] = (scalar_t)negative::structured_item(rp, cl, ptr, (int64_t)src[t / num_neg], t, sh.num_src, sh.num_edges,
                                                   num_dst, sh.G, key, exclude_self);
  });
}

template <typename scalar_t>
void negative_global_cpu_t(const scalar_t* rp, const scalar_t* cl, scalar_t* out, const Shape& sh, int64_t num_dst,
                           int64_t num_neg, uint64_t key) {
  at::parallel_for(0, num_neg, 256, [&](int64_t begin, int64_t end) {
    for (int64_t t = begin; t < end; ++t) {
      int64_t s, x;
      negative::global_item(rp, cl, t, sh.num_src, sh.num_edges, num_dst, sh.T, key, s, x);
      out[t] = (scalar_t)s;
      out[num_neg + t] = (scalar_t)x;
    }
  });
}

Tensor edge_lookup_cpu(const Tensor& rowptr, const Tensor& col, const Tensor& src, const Tensor& dst) {
  PYG_TRACE("pyg::edge_lookup[cpu]");
  TORCH_CHECK(rowptr.defined() && rowptr.is_cpu(), "'rowptr' must be a CPU tensor");
  check_lookup_args(rowptr, col, src, dst);
  const auto rowptr_c = rowptr.contiguous(), col_c = col.contiguous(), src_c = src.contiguous(), dst_c = dst.contiguous();
  auto out = at::empty({src.numel()}, src.options());
  const int64_t num_src = rowptr_c.numel() - 1, E = col_c.numel(), Q = src_c.numel();
  if (rowptr.scalar_type() == at::kInt)
    edge_lookup_cpu_t<int32_t>(rowptr_c.data_ptr<int32_t>(), col_c.data_ptr<int32_t>(), src_c.data_ptr<int32_t>(),
                               dst_c.data_ptr<int32_t>(), out.data_ptr<int32_t>(), num_src, E, Q);
  else
    edge_lookup_cpu_t<int64_t>(rowptr_c.data_ptr<int64_t>(), col_c.data_ptr<int64_t>(), src_c.data_ptr<int64_t>(),
                               dst_c.data_ptr<int64_t>(), out.data_ptr<int64_t>(), num_src, E, Q);
  return out;
}

template <typename scalar_t>
void negative_sample_cpu_t(const Tensor& rowptr, const Tensor& col, const Tensor& src, const Tensor& ptr, Tensor& out,
                           const Shape& sh, int64_t num_dst, int64_t num_neg, uint64_t key, bool exclude_self) {
  if (sh.structured)
    negative_structured_cpu_t<scalar_t>(rowptr.data_ptr<scalar_t>(), col.data_ptr<scalar_t>(), src.data_ptr<scalar_t>(),
                                        ptr.defined() ? ptr.data_ptr<scalar_t>() : nullptr, out.data_ptr<scalar_t>(), sh,
                                        num_dst, num_neg, key, exclude_self);
  else
    negative_global_cpu_t<scalar_t>(rowptr.data_ptr<scalar_t>(), col.data_ptr<scalar_t>(), out.data_ptr<scalar_t>(), sh,
                                    num_dst, num_neg, key);
}

Tensor negative_sample_keyed_cpu(const Tensor& rowptr, const Tensor& col, const OptTensor& src, int64_t num_dst,
                                 int64_t num_neg, int64_t key, bool exclude_self, const OptTensor& ptr) {
  PYG_TRACE("pyg::negative_sample_keyed[cpu]");
  TORCH_CHECK(rowptr.defined() && rowptr.is_cpu(), "'rowptr' must be a CPU tensor");
  const Shape sh = check_sample_args(rowptr, col, src, num_dst, num_neg, exclude_self, ptr);
  const auto rowptr_c = rowptr.contiguous(), col_c = col.contiguous();
  const Tensor src_c = sh.structured ? src->contiguous() : Tensor();
  const Tensor ptr_c = given(ptr) ? ptr->contiguous() : Tensor();
  auto out = empty_result(sh, num_neg, rowptr);
  if (rowptr.scalar_type() == at::kInt)
    negative_sample_cpu_t<int32_t>(rowptr_c, col_c, src_c, ptr_c, out, sh, num_dst, num_neg, (uint64_t)key, exclude_self);
  else
    negative_sample_cpu_t<int64_t>(rowptr_c, col_c, src_c, ptr_c, out, sh, num_dst, num_neg, (uint64_t)key, exclude_self);
  return out;
}

Tensor negative_sample_cpu(const Tensor& rowptr, const Tensor& col, const OptTensor& src, int64_t num_dst, int64_t num_neg,
                           bool exclude_self, const OptTensor& ptr) {
  TORCH_CHECK(rowptr.defined() && rowptr.is_cpu(), "'rowptr' must be a CPU tensor");
  check_sample_args(rowptr, col, src, num_dst, num_neg, exclude_self, ptr);  // a call that raises draws no key
  auto* gen = at::get_generator_or_default<at::CPUGeneratorImpl>(c10::nullopt, at::detail::getDefaultCPUGenerator());
  uint64_t key;
  {
    std::lock_guard<std::mutex> lock(gen->mutex_);
    key = gen->random64();
  }
  return negative_sample_keyed_cpu(rowptr, col, src, num_dst, num_neg, (int64_t)key, exclude_self, ptr);
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(pyg, m) {
  m.def(TORCH_SELECTIVE_SCHEMA("pyg::edge_lookup(Tensor rowptr, Tensor col, Tensor src, Tensor dst) -> Tensor"));
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::negative_sample_keyed(Tensor rowptr, Tensor col, Tensor? src, int num_dst, int num_neg, int key, "
      "bool exclude_self=False, Tensor? ptr=None) -> Tensor"));
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::negative_sample(Tensor rowptr, Tensor col, Tensor? src, int num_dst, int num_neg, "
      "bool exclude_self=False, Tensor? ptr=None) -> Tensor"));
}

TORCH_LIBRARY_IMPL(pyg, CUDA, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::edge_lookup"), TORCH_FN(edge_lookup_cuda));
  m.impl(TORCH_SELECTIVE_NAME("pyg::negative_sample_keyed"), TORCH_FN(negative_sample_keyed_cuda));
  m.impl(TORCH_SELECTIVE_NAME("pyg::negative_sample"), TORCH_FN(negative_sample_cuda));
}

TORCH_LIBRARY_IMPL(pyg, CPU, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::edge_lookup"), TORCH_FN(edge_lookup_cpu));
  m.impl(TORCH_SELECTIVE_NAME("pyg::negative_sample_keyed"), TORCH_FN(negative_sample_keyed_cpu));
  m.impl(TORCH_SELECTIVE_NAME("pyg::negative_sample"), TORCH_FN(negative_sample_cpu));
}

}  // namespace pyg_amd
