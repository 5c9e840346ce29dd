// torch::Library binding of pyg::sampled_op: out = left[left_index] (op) right[right_index], op in add / sub / mul / div.
// Schema byte-identical to pyg_lib/csrc/ops/sampled.cpp:57-59; argument checks follow the operator front
// (sampled.cpp:15-48, the reference's wording through the same at::check* helpers) plus the three the reference's CUDA
// kernel reads out of bounds without; key CPU is the reference's expression (ops/cpu/sampled_kernel.cpp:17-46); the autograd
// formulas follow ops/autograd/sampled_kernel.cpp:34-95, with the sum over a node's edges handed to pyg::scatter_sum
// (stable sort + CSR rows: no float atomics on large inputs, reproducible) instead of at::index_select_backward.
// Kernels: csrc/hip/sampled.hip through the C-ABI of include/pyg_hip.h.
#include <ATen/TensorUtils.h>
#include <ATen/core/dispatch/Dispatcher.h>
#include <torch/autograd.h>
#include <torch/library.h>

#include <optional>
#include <string>

#include "binding_common.h"

namespace pyg_amd {
namespace {

using torch::autograd::variable_list;
using OptTensor = std::optional<Tensor>;

int fn_code(const std::string& fn) {
  static const char* names[] = {"add", "sub", "mul", "div"};   // = PYG_SAMPLED_ADD ... PYG_SAMPLED_DIV
  for (int i = 0; i < 4; ++i)
    if (fn == names[i]) return i;
  TORCH_CHECK(false, "sampled_op: unknown op '", fn, "' (expected one of 'add', 'sub', 'mul', 'div')");
  return -1;
}

// number of output rows (ops/cuda/sampled_kernel.cu:71-76)
int64_t num_edges(const Tensor& left, const OptTensor& left_index, const OptTensor& right_index) {
  if (left_index.has_value()) return left_index.value().size(0);
  if (right_index.has_value()) return right_index.value().size(0);
  return left.size(0);
}

void check_args(const Tensor& left, const Tensor& right, const OptTensor& left_index, const OptTensor& right_index) {
  // pyg_lib/csrc/ops/sampled.cpp:15-48
  at::TensorArg left_arg{left, "left", 0};
  at::TensorArg right_arg{right, "right", 1};
  at::CheckedFrom c{"sampled_op"};

  at::checkAllDefined(c, {left_arg, right_arg});
  at::checkSameType(c, left_arg, right_arg);
  at::checkContiguous(c, left_arg);
  at::checkContiguous(c, right_arg);
  at::checkDim(c, left_arg, 2);
  at::checkDim(c, right_arg, 2);
  at::checkSize(c, left_arg, 1, right_arg->size(1));

  if (left_index.has_value()) {
    at::TensorArg left_index_arg{left_index.value(), "left_index", 2};
    at::checkContiguous(c, left_index_arg);
    at::checkDim(c, left_index_arg, 1);
  }
  if (right_index.has_value()) {
    at::TensorArg right_index_arg{right_index.value(), "right_index", 3};
    at::checkContiguous(c, right_index_arg);
    at::checkDim(c, right_index_arg, 1);
  }
  if (left_index.has_value() && right_index.has_value()) {
    at::TensorArg left_index_arg{left_index.value(), "left_index", 2};
    at::TensorArg right_index_arg{right_index.value(), "right_index", 3};
    at::checkSameType(c, left_index_arg, right_index_arg);
    at::checkSize(c, left_index_arg, 0, right_index_arg->size(0));
  }
  if (!left_index.has_value() && !right_index.has_value()) {
    at::checkSize(c, left_arg, 0, right_arg->size(0));
  }

  // not in the reference (its CUDA kernel takes the unindexed side's row count for the output's and reads the index beyond
  // its end, or the table beyond its rows, when they differ; it reads an int32 index as int64)
  TORCH_CHECK(left.device() == right.device() && (left.is_cuda() || left.is_cpu()),
              "sampled_op: left and right must live on the same device, the CPU or a HIP device (got left=", left.device(),
              ", right=", right.device(), ")");
  if (left_index.has_value() != right_index.has_value()) {
    const bool is_left = left_index.has_value();
    const Tensor& index = is_left ? left_index.value() : right_index.value();
    const Tensor& other = is_left ? right : left;
    TORCH_CHECK(index.size(0) == other.size(0), "sampled_op: ", is_left ? "left_index" : "right_index", " has ", index.size(0),
                " entries but ", is_left ? "right" : "left", ", which is read without an index, has ", other.size(0), " rows");
  }
  for (const OptTensor* index : {&left_index, &right_index}) {
    if (!index->has_value()) continue;
    const Tensor& t = index->value();
    const char* name = index == &left_index ? "left_index" : "right_index";
    TORCH_CHECK(t.scalar_type() == at::kLong || t.scalar_type() == at::kInt, "sampled_op: ", name,
                " must be an int64 or int32 tensor (got ", t.scalar_type(), ")");
    TORCH_CHECK(t.device() == left.device(), "sampled_op: ", name, " must live on the device of left and right (got ", t.device(),
                ", expected ", left.device(), ")");
    const Tensor& table = index == &left_index ? left : right;
    TORCH_CHECK(table.size(0) > 0 || t.size(0) == 0, "sampled_op: ", name, " selects rows of an empty tensor");
  }
}

int index_code(const OptTensor& left_index, const OptTensor& right_index) {
  const OptTensor& any = left_index.has_value() ? left_index : right_index;
  return any.has_value() && any.value().scalar_type() == at::kInt ? PYG_I32 : PYG_I64;
}

const void* index_ptr(const OptTensor& index) { return index.has_value() ? index.value().data_ptr() : nullptr; }

// keys CUDA and CPU
Tensor sampled_op_kernel(const Tensor& left, const Tensor& right, const OptTensor& left_index, const OptTensor& right_index,
                         std::string fn) {
  PYG_TRACE("pyg::sampled_op");
  check_args(left, right, left_index, right_index);
  const int code = fn_code(fn);
  if (left.is_cpu()) {
    // ops/cpu/sampled_kernel.cpp:22-45 (index_select raises for an index out of range)
    auto a = left;
    if (left_index.has_value()) a = left.index_select(0, left_index.value());
    auto b = right;
    if (right_index.has_value()) b = right.index_select(0, right_index.value());
    if (code == PYG_SAMPLED_ADD) return a + b;
    if (code == PYG_SAMPLED_SUB) return a - b;
    if (code == PYG_SAMPLED_MUL) return a * b;
    return a / b;
  }
  DeviceGuard guard(left.device());
  const int64_t E = num_edges(left, left_index, right_index), F = left.size(1);
  auto out = at::empty({E, F}, left.options());
  check_status(pyg_hip_sampled_op(code, dtype_code(left.scalar_type()), left.data_ptr(), left.size(0), right.data_ptr(),
                                  right.size(0), index_code(left_index, right_index), index_ptr(left_index),
                                  index_ptr(right_index), out.data_ptr(), E, F, current_stream(left)));
  return out;
}

using SampledSig = Tensor(const Tensor&, const Tensor&, const OptTensor&, const OptTensor&, std::string);
using ScatterSig = Tensor(const Tensor&, const Tensor&, int64_t, const OptTensor&, std::optional<int64_t>);

// sum of the per-edge gradients over every node's edges: pyg::scatter_sum, re-entered through the dispatcher (one unsorted
// index vector: its stable sort + CSR-row path, hub rows, PYG_HIP_FLOAT_ATOMICS and torch.use_deterministic_algorithms)
Tensor reduce_by_index(const Tensor& edge_grad, const Tensor& index, int64_t rows) {
  static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("pyg::scatter_sum", "").typed<ScatterSig>();
  return op.call(edge_grad, index.scalar_type() == at::kLong ? index : index.to(at::kLong), 0, std::nullopt, rows);
}

class SampledOp : public torch::autograd::Function<SampledOp> {
 public:
  static variable_list forward(torch::autograd::AutogradContext* ctx, const Tensor& left, const Tensor& right,
                               const OptTensor& left_index, const OptTensor& right_index, std::string fn) {
    at::AutoDispatchBelowADInplaceOrView g;
    static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("pyg::sampled_op", "").typed<SampledSig>();
    auto out = op.call(left, right, left_index, right_index, fn);
    ctx->saved_data["fn"] = (int64_t)fn_code(fn);
    ctx->save_for_backward({left, right, left_index.value_or(Tensor()), right_index.value_or(Tensor())});
    return {out};
  }

  // ops/autograd/sampled_kernel.cpp:34-95.  Not differentiable a second time (nothing here is recorded).
  static variable_list backward(torch::autograd::AutogradContext* ctx, variable_list grad_outs) {
    at::AutoGradMode no_grad(false);
    const auto saved = ctx->get_saved_variables();
    const Tensor &left = saved[0], &right = saved[1];
    OptTensor left_index, right_index;
    if (saved[2].defined()) left_index = saved[2];
    if (saved[3].defined()) right_index = saved[3];
    const int code = (int)ctx->saved_data["fn"].toInt();
    const bool want_left = torch::autograd::any_variable_requires_grad({left});
    const bool want_right = torch::autograd::any_variable_requires_grad({right});
    const auto grad_out = grad_outs[0].contiguous();

    // edge stage: the gradient with respect to left[left_index] / right[right_index], [E, F]
    Tensor edge_left, edge_right;
    if (code == PYG_SAMPLED_ADD || code == PYG_SAMPLED_SUB) {
      edge_left = edge_right = grad_out;
    } else if (grad_out.is_cpu()) {
      const auto a = left_index.has_value() ? left.index_select(0, left_index.value()) : left;
      const auto b = right_index.has_value() ? right.index_select(0, right_index.value()) : right;
      if (code == PYG_SAMPLED_MUL) {
        if (want_left) edge_left = grad_out * b;
        if (want_right) edge_right = grad_out * a;
      } else {
        if (want_left) edge_left = grad_out / b;
        if (want_right) edge_right = (-grad_out) * ((a / b) / b);
      }
    } else if (want_left || want_right) {
      DeviceGuard guard(grad_out.device());
      if (want_left) edge_left = at::empty_like(grad_out);
      if (want_right) edge_right = at::empty_like(grad_out);
      check_status(pyg_hip_sampled_op_backward(
          code, dtype_code(left.scalar_type()), grad_out.data_ptr(), left.data_ptr(), left.size(0), right.data_ptr(),
          right.size(0), index_code(left_index, right_index), index_ptr(left_index), index_ptr(right_index),
          want_left ? edge_left.data_ptr() : nullptr, want_right ? edge_right.data_ptr() : nullptr, grad_out.size(0),
          grad_out.size(1), current_stream(grad_out)));
    }

    // node stage: a side read without an index has one edge per row
    Tensor grad_left, grad_right;
    if (want_left) grad_left = left_index.has_value() ? reduce_by_index(edge_left, left_index.value(), left.size(0)) : edge_left;
    if (want_right) {
      // sub: negate whichever is smaller, the edges or the table (sampled_kernel.cpp:73-74,89-91)
      const bool negate = code == PYG_SAMPLED_SUB;
      const bool before = negate && (!right_index.has_value() || grad_out.size(0) <= right.size(0));
      if (before) edge_right = -edge_right;
      grad_right = right_index.has_value() ? reduce_by_index(edge_right, right_index.value(), right.size(0)) : edge_right;
      // (0 - x, not -x: a node whose terms cancel, or without edges, reads +0 as the sum of its negated terms does)
      if (negate && !before) grad_right = at::rsub(grad_right, 0);
    }
    return {grad_left, grad_right, Tensor(), Tensor(), Tensor()};
  }
};

Tensor sampled_op_autograd(const Tensor& left, const Tensor& right, const OptTensor& left_index, const OptTensor& right_index,
                           std::string fn) {
  return SampledOp::apply(left, right, left_index, right_index, fn)[0];
}

}  // namespace

// ops/sampled.cpp:56-60
TORCH_LIBRARY_FRAGMENT(pyg, m) {
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::sampled_op(Tensor left, Tensor right, Tensor? left_index, Tensor? "
      "right_index, str op) -> Tensor"));
}

TORCH_LIBRARY_IMPL(pyg, CUDA, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::sampled_op"), TORCH_FN(sampled_op_kernel));
}

// ops/cpu/sampled_kernel.cpp:50-52
TORCH_LIBRARY_IMPL(pyg, CPU, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::sampled_op"), TORCH_FN(sampled_op_kernel));
}

// ops/autograd/sampled_kernel.cpp:108-111
TORCH_LIBRARY_IMPL(pyg, Autograd, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::sampled_op"), TORCH_FN(sampled_op_autograd));
}

}  // namespace pyg_amd
