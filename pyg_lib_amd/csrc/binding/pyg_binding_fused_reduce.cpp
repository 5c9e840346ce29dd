// torch::Library binding of pyg::fused_scatter_reduce: sum / mean / min / max of inputs [E, F] over index [E] into
// out [dim_size, R * F], slice i of a row holding reduce_list[i].
// The schema is NEW: the reference's function is Python only (pyg_lib/ops/scatter_reduce.py:95-181, a Triton kernel without
// backward or CPU path), so there is no C++ schema to stay byte-identical with.  Key CPU is the executable statement of the
// semantics (include/pyg_hip.h): one sequential loop over the edges in source order, opmath accumulators, one rounding; the
// autograd formula is the header's, on both devices.  Kernels: csrc/hip/fused_reduce.hip through the C-ABI.
#include <ATen/Dispatch.h>
#include <ATen/OpMathType.h>
#include <ATen/core/dispatch/Dispatcher.h>
#include <torch/autograd.h>
#include <torch/library.h>

#include <limits>
#include <string>
#include <vector>

#include "binding_common.h"

namespace pyg_amd {
namespace {

using torch::autograd::variable_list;

// reduce_list -> codes of pyg_fused_reduce; refuses an empty list, unknown names and duplicates
std::vector<int> reduce_codes(const std::vector<std::string>& reduce_list) {
  static const char* names[] = {"sum", "mean", "min", "max"};   // = PYG_FUSED_SUM ... PYG_FUSED_MAX
  TORCH_CHECK(!reduce_list.empty(), "fused_scatter_reduce: reduce_list is empty (expected 1 to 4 of 'sum', 'mean', 'min', 'max')");
  std::vector<int> codes;
  for (const auto& name : reduce_list) {
    int code = -1;
    for (int i = 0; i < 4; ++i)
      if (name == names[i]) code = i;
    TORCH_CHECK(code >= 0, "fused_scatter_reduce: unknown reduction '", name, "' (expected 'sum', 'mean', 'min' or 'max')");
    for (int seen : codes) TORCH_CHECK(seen != code, "fused_scatter_reduce: '", name, "' is listed twice in reduce_list");
    codes.push_back(code);
  }
  return codes;
}

bool has(const std::vector<int>& codes, int code) {
  for (int c : codes)
    if (c == code) return true;
  return false;
}

void check_args(const Tensor& inputs, const Tensor& index, int64_t dim_size) {
  TORCH_CHECK(inputs.is_cuda() || inputs.is_cpu(), "fused_scatter_reduce: inputs must live on the CPU or a HIP device (got ",
              inputs.device(), ")");
  TORCH_CHECK(at::isFloatingType(inputs.scalar_type()) && dtype_code(inputs.scalar_type()) <= PYG_BF16,
              "fused_scatter_reduce: inputs must be float32, float64, bfloat16 or float16 (got ", inputs.scalar_type(),
              "; integer tensors have no fused kernel: their mean is a floor division)");
  TORCH_CHECK(inputs.dim() == 2, "fused_scatter_reduce: inputs must be 2-D [E, F] (got ", inputs.dim(), " dimensions)");
  TORCH_CHECK(inputs.is_contiguous(), "fused_scatter_reduce: inputs must be contiguous");
  TORCH_CHECK(index.scalar_type() == at::kLong, "fused_scatter_reduce: index must be an int64 tensor (got ", index.scalar_type(), ")");
  TORCH_CHECK(index.dim() == 1 && index.is_contiguous(), "fused_scatter_reduce: index must be 1-D and contiguous");
  TORCH_CHECK(index.device() == inputs.device(), "fused_scatter_reduce: index must live on the device of inputs (got ",
              index.device(), ", expected ", inputs.device(), ")");
  TORCH_CHECK(index.size(0) == inputs.size(0), "fused_scatter_reduce: index has ", index.size(0), " entries but inputs has ",
              inputs.size(0), " rows");
  TORCH_CHECK(dim_size >= 0, "fused_scatter_reduce: dim_size must not be negative (got ", dim_size, ")");
}

struct Forward {
  Tensor out, arg_min, arg_max, count;   // the last three only where asked for
};

// the CPU key: the edges one after the other
template <typename scalar_t>
void cpu_forward(const Tensor& inputs, const Tensor& index, int64_t N, const std::vector<int>& codes, Forward& r) {
  using opmath_t = at::opmath_type<scalar_t>;
  const int64_t E = inputs.size(0), F = inputs.size(1), R = (int64_t)codes.size();
  const opmath_t lo = static_cast<opmath_t>(std::numeric_limits<scalar_t>::lowest());
  const opmath_t hi = static_cast<opmath_t>(std::numeric_limits<scalar_t>::max());
  std::vector<opmath_t> sum((size_t)(N * F), opmath_t(0)), mn((size_t)(N * F), hi), mx((size_t)(N * F), lo);
  std::vector<int64_t> amin((size_t)(N * F), E), amax((size_t)(N * F), E), cnt((size_t)N, 0);
  const scalar_t* x = inputs.data_ptr<scalar_t>();
  const int64_t* idx = index.data_ptr<int64_t>();
  for (int64_t e = 0; e < E; ++e) {
    const int64_t n = idx[e];
    TORCH_CHECK(n >= 0 && n < N, "fused_scatter_reduce: index[", e, "] = ", n, " is out of range for dim_size ", N);
    ++cnt[n];
    for (int64_t f = 0; f < F; ++f) {
      const opmath_t v = static_cast<opmath_t>(x[e * F + f]);
      const size_t o = (size_t)(n * F + f);
      sum[o] += v;
      if (v < mn[o]) mn[o] = v, amin[o] = e;
      if (v > mx[o]) mx[o] = v, amax[o] = e;
    }
  }
  scalar_t* out = r.out.data_ptr<scalar_t>();
  for (int64_t n = 0; n < N; ++n)
    for (int64_t k = 0; k < R; ++k)
      for (int64_t f = 0; f < F; ++f) {
        const size_t o = (size_t)(n * F + f);
        opmath_t v;
        switch (codes[k]) {
          case PYG_FUSED_SUM: v = sum[o]; break;
          case PYG_FUSED_MEAN: v = sum[o] / static_cast<opmath_t>(cnt[n] > 0 ? cnt[n] : 1); break;
          case PYG_FUSED_MIN: v = amin[o] == E ? opmath_t(0) : mn[o]; break;
          default: v = amax[o] == E ? opmath_t(0) : mx[o]; break;
        }
        out[(n * R + k) * F + f] = static_cast<scalar_t>(v);
      }
  if (r.arg_min.defined()) std::copy(amin.begin(), amin.end(), r.arg_min.data_ptr<int64_t>());
  if (r.arg_max.defined()) std::copy(amax.begin(), amax.end(), r.arg_max.data_ptr<int64_t>());
  if (r.count.defined()) std::copy(cnt.begin(), cnt.end(), r.count.data_ptr<int64_t>());
}

Forward forward_impl(const Tensor& inputs, const Tensor& index, int64_t N, const std::vector<int>& codes, bool want_args,
                     bool want_count) {
  const int64_t E = inputs.size(0), F = inputs.size(1), R = (int64_t)codes.size();
  const auto longs = index.options();
  Forward r;
  r.out = at::empty({N, R * F}, inputs.options());
  if (want_args && has(codes, PYG_FUSED_MIN)) r.arg_min = at::empty({N, F}, longs);
  if (want_args && has(codes, PYG_FUSED_MAX)) r.arg_max = at::empty({N, F}, longs);
  if (want_count) r.count = at::empty({N}, longs);
  if (inputs.is_cpu()) {
    AT_DISPATCH_FLOATING_TYPES_AND2(at::kHalf, at::kBFloat16, inputs.scalar_type(), "fused_scatter_reduce",
                                    [&] { cpu_forward<scalar_t>(inputs, index, N, codes, r); });
    return r;
  }
  DeviceGuard guard(inputs.device());
  const int dtype = dtype_code(inputs.scalar_type());
  const size_t ws_bytes = E > 0 && F > 0 && N > 0 ? pyg_hip_fused_scatter_reduce_workspace_size(dtype, E, N, F) : 0;
  auto ws = at::empty({(int64_t)ws_bytes}, inputs.options().dtype(at::kByte));
  check_status(pyg_hip_fused_scatter_reduce(
      dtype, inputs.data_ptr(), index.data_ptr<int64_t>(), E, F, N, codes.data(), (int)codes.size(), r.out.data_ptr(),
      r.arg_min.defined() ? r.arg_min.data_ptr<int64_t>() : nullptr, r.arg_max.defined() ? r.arg_max.data_ptr<int64_t>() : nullptr,
      r.count.defined() ? r.count.data_ptr<int64_t>() : nullptr, ws_bytes ? ws.data_ptr() : nullptr, ws_bytes,
      current_stream(inputs)));
  return r;
}

template <typename scalar_t>
void cpu_backward(const Tensor& grad_out, const Tensor& index, const Forward& saved, const std::vector<int>& codes,
                  Tensor& grad_in) {
  using opmath_t = at::opmath_type<scalar_t>;
  const int64_t E = grad_in.size(0), F = grad_in.size(1), R = (int64_t)codes.size();
  const scalar_t* g = grad_out.data_ptr<scalar_t>();
  const int64_t* idx = index.data_ptr<int64_t>();
  const int64_t* amin = saved.arg_min.defined() ? saved.arg_min.data_ptr<int64_t>() : nullptr;
  const int64_t* amax = saved.arg_max.defined() ? saved.arg_max.data_ptr<int64_t>() : nullptr;
  const int64_t* cnt = saved.count.defined() ? saved.count.data_ptr<int64_t>() : nullptr;
  scalar_t* gi = grad_in.data_ptr<scalar_t>();
  for (int64_t e = 0; e < E; ++e) {
    const int64_t n = idx[e];
    for (int64_t f = 0; f < F; ++f) {
      opmath_t acc = 0;
      for (int64_t k = 0; k < R; ++k) {
        const opmath_t gv = static_cast<opmath_t>(g[(n * R + k) * F + f]);
        switch (codes[k]) {
          case PYG_FUSED_SUM: acc += gv; break;
          case PYG_FUSED_MEAN: acc += gv / static_cast<opmath_t>(cnt[n] > 0 ? cnt[n] : 1); break;
          case PYG_FUSED_MIN: acc += amin[n * F + f] == e ? gv : opmath_t(0); break;
          default: acc += amax[n * F + f] == e ? gv : opmath_t(0); break;
        }
      }
      gi[e * F + f] = static_cast<scalar_t>(acc);
    }
  }
}

Tensor backward_impl(const Tensor& grad_out, const Tensor& index, const Forward& saved, int64_t F, const std::vector<int>& codes) {
  const int64_t E = index.size(0), N = grad_out.size(0);
  auto grad_in = at::empty({E, F}, grad_out.options());
  if (grad_out.is_cpu()) {
    AT_DISPATCH_FLOATING_TYPES_AND2(at::kHalf, at::kBFloat16, grad_out.scalar_type(), "fused_scatter_reduce_backward",
                                    [&] { cpu_backward<scalar_t>(grad_out, index, saved, codes, grad_in); });
    return grad_in;
  }
  DeviceGuard guard(grad_out.device());
  check_status(pyg_hip_fused_scatter_reduce_backward(
      dtype_code(grad_out.scalar_type()), grad_out.data_ptr(), index.data_ptr<int64_t>(),
      saved.arg_min.defined() ? saved.arg_min.data_ptr<int64_t>() : nullptr,
      saved.arg_max.defined() ? saved.arg_max.data_ptr<int64_t>() : nullptr,
      saved.count.defined() ? saved.count.data_ptr<int64_t>() : nullptr, E, F, N, codes.data(), (int)codes.size(),
      grad_in.data_ptr(), current_stream(grad_out)));
  return grad_in;
}

// keys CUDA and CPU: no arg tensor, no count is allocated or written
Tensor fused_scatter_reduce_kernel(const Tensor& inputs, const Tensor& index, int64_t dim_size,
                                   std::vector<std::string> reduce_list) {
  PYG_TRACE("pyg::fused_scatter_reduce");
  const auto codes = reduce_codes(reduce_list);
  check_args(inputs, index, dim_size);
  return forward_impl(inputs, index, dim_size, codes, false, false).out;
}

class FusedScatterReduce : public torch::autograd::Function<FusedScatterReduce> {
 public:
  static variable_list forward(torch::autograd::AutogradContext* ctx, const Tensor& inputs, const Tensor& index,
                               int64_t dim_size, std::vector<std::string> reduce_list, bool grad) {
    at::AutoDispatchBelowADInplaceOrView g;
    PYG_TRACE("pyg::fused_scatter_reduce");
    const auto codes = reduce_codes(reduce_list);
    check_args(inputs, index, dim_size);
    // positions only where a gradient will ask for them, the count only for a mean
    const bool want_args = grad && (has(codes, PYG_FUSED_MIN) || has(codes, PYG_FUSED_MAX));
    const bool want_count = grad && has(codes, PYG_FUSED_MEAN);
    auto r = forward_impl(inputs, index, dim_size, codes, want_args, want_count);
    if (grad) {
      ctx->saved_data["codes"] = std::vector<int64_t>(codes.begin(), codes.end());
      ctx->saved_data["F"] = inputs.size(1);
      ctx->save_for_backward({index, r.arg_min, r.arg_max, r.count});
    }
    return {r.out};
  }

  // include/pyg_hip.h, pyg_hip_fused_scatter_reduce_backward.  Not differentiable a second time (nothing here is recorded).
  static variable_list backward(torch::autograd::AutogradContext* ctx, variable_list grad_outs) {
    at::AutoGradMode no_grad(false);
    const auto saved = ctx->get_saved_variables();
    Forward f;
    f.arg_min = saved[1], f.arg_max = saved[2], f.count = saved[3];
    std::vector<int> codes;
    for (int64_t c : ctx->saved_data["codes"].toIntVector()) codes.push_back((int)c);
    PYG_TRACE("pyg::fused_scatter_reduce_backward");
    auto grad_in = backward_impl(grad_outs[0].contiguous(), saved[0], f, ctx->saved_data["F"].toInt(), codes);
    return {grad_in, Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

Tensor fused_scatter_reduce_autograd(const Tensor& inputs, const Tensor& index, int64_t dim_size,
                                     std::vector<std::string> reduce_list) {
  // (asked here: grad mode is switched off inside forward())
  const bool grad = at::GradMode::is_enabled() && inputs.requires_grad();
  return FusedScatterReduce::apply(inputs, index, dim_size, reduce_list, grad)[0];
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(pyg, m) {
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::fused_scatter_reduce(Tensor inputs, Tensor index, int dim_size, str[] reduce_list) -> Tensor"));
}

TORCH_LIBRARY_IMPL(pyg, CUDA, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::fused_scatter_reduce"), TORCH_FN(fused_scatter_reduce_kernel));
}

TORCH_LIBRARY_IMPL(pyg, CPU, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::fused_scatter_reduce"), TORCH_FN(fused_scatter_reduce_kernel));
}

TORCH_LIBRARY_IMPL(pyg, Autograd, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::fused_scatter_reduce"), TORCH_FN(fused_scatter_reduce_autograd));
}

}  // namespace pyg_amd
