// torch::Library binding of pyg::graclus_cluster (schema: pyg_lib/csrc/ops/graclus.cpp, byte for byte) and of its
// deterministic core pyg::graclus_cluster_perm, an operator of this build.  The outputs are integers: no Autograd key.
// Key CUDA: csrc/hip/graclus.hip through the C-ABI.  Key CPU: the sequential visit that include/pyg_hip.h states -- the
// executable definition the device's rounds are tested against, bit for bit.  A correctness key, not a hot path.
#include <ATen/Dispatch.h>
#include <torch/library.h>

#include <algorithm>
#include <cstdint>
#include <optional>

#include "binding_common.h"

namespace pyg_amd {
namespace {

// PYG_HIP_GRACLUS_FORCE_* for the calls of this thread (pyg_binding_set_graclus_route; tests and measurements)
int& graclus_route_tls() {
  thread_local int flags = 0;
  return flags;
}

bool is_device_weight(at::ScalarType t) { return t == at::kFloat || t == at::kDouble || t == at::kHalf || t == at::kBFloat16; }

// the visit of include/pyg_hip.h, with weights
template <typename scalar_t>
void visit_weighted(const int64_t* rowptr, const int64_t* col, const scalar_t* weight, const int64_t* perm, int64_t N, int64_t* out) {
  for (int64_t n = 0; n < N; ++n) {
    const int64_t u = perm[n];
    if (out[u] >= 0) continue;
    int64_t pick = u;
    scalar_t best = static_cast<scalar_t>(0.);
    for (int64_t e = rowptr[u]; e < rowptr[u + 1]; ++e) {
      const int64_t x = col[e];
      if (out[x] >= 0) continue;
      if (weight[e] >= best) pick = x, best = weight[e];   // the last among equals; a NaN or a negative weight never passes
    }
    out[u] = out[pick] = std::min(u, pick);
  }
}

void visit_plain(const int64_t* rowptr, const int64_t* col, const int64_t* perm, int64_t N, int64_t* out) {
  for (int64_t n = 0; n < N; ++n) {
    const int64_t u = perm[n];
    if (out[u] >= 0) continue;
    out[u] = u;   // (which is what skips a self loop)
    for (int64_t e = rowptr[u]; e < rowptr[u + 1]; ++e) {
      const int64_t x = col[e];
      if (out[x] >= 0) continue;
      out[u] = out[x] = std::min(u, x);
      break;
    }
  }
}

void check_graph(const Tensor& rowptr, const Tensor& col, const std::optional<Tensor>& weight) {
  TORCH_CHECK(rowptr.defined() && col.defined(), "graclus_cluster: rowptr and col must be defined");
  TORCH_CHECK(rowptr.dim() == 1, "graclus_cluster: rowptr must be 1-dimensional (got ", rowptr.dim(), " dimensions)");
  TORCH_CHECK(col.dim() == 1, "graclus_cluster: col must be 1-dimensional (got ", col.dim(), " dimensions)");
  if (weight.has_value()) {
    TORCH_CHECK(weight->dim() == 1, "weight must be 1-dimensional");
    TORCH_CHECK(weight->numel() == col.numel(), "weight must have the same number of elements as col");
  }
}

Tensor graclus_perm_kernel(const Tensor& rowptr_, const Tensor& col_, const std::optional<Tensor>& weight_, const Tensor& perm_) {
  PYG_TRACE("pyg::graclus_cluster_perm");
  const std::optional<Tensor> given = weight_.has_value() && weight_->defined() ? weight_ : std::nullopt;
  check_graph(rowptr_, col_, given);
  TORCH_CHECK(perm_.defined() && perm_.dim() == 1, "graclus_cluster: perm must be 1-dimensional");
  TORCH_CHECK(rowptr_.scalar_type() == at::kLong && col_.scalar_type() == at::kLong && perm_.scalar_type() == at::kLong,
              "graclus_cluster: rowptr, col and perm must be int64 tensors (got ", rowptr_.scalar_type(), ", ", col_.scalar_type(), ", ",
              perm_.scalar_type(), ")");
  TORCH_CHECK(rowptr_.numel() >= 1, "graclus_cluster: rowptr must have at least 1 entry");
  TORCH_CHECK(col_.device() == rowptr_.device() && perm_.device() == rowptr_.device() && (!given || given->device() == rowptr_.device()),
              "graclus_cluster: col, weight and perm must live on the device of rowptr (", rowptr_.device(), ")");
  const int64_t N = rowptr_.numel() - 1, E = col_.numel();
  TORCH_CHECK(perm_.numel() == N, "graclus_cluster: perm must have one entry per node (got ", perm_.numel(), ", expected ", N, ")");
  TORCH_CHECK(N < (int64_t(1) << 31), "graclus_cluster: 2^31 or more nodes");
  const Tensor rowptr = rowptr_.contiguous(), col = col_.contiguous(), perm = perm_.contiguous();
  const std::optional<Tensor> weight = given ? std::optional<Tensor>(given->contiguous()) : std::nullopt;
  if (rowptr.is_cpu()) {
    // the device defers these checks (include/pyg_hip.h); here they come before the first access
    const int64_t* rp = rowptr.data_ptr<int64_t>();
    bool rows_ok = rp[0] == 0 && rp[N] == E;
    for (int64_t u = 0; u < N; ++u) rows_ok &= rp[u] <= rp[u + 1];
    TORCH_CHECK(rows_ok, "graclus_cluster: rowptr must be non-decreasing, begin at 0 and end at the number of edges");
    TORCH_CHECK(E == 0 || (col.min().item<int64_t>() >= 0 && col.max().item<int64_t>() < N),
                "graclus_cluster: col holds an entry outside [0, ", N, ")");
    TORCH_CHECK(N == 0 || at::equal(std::get<0>(perm.sort()), at::arange(N, perm.options())),
                "graclus_cluster: perm must be a permutation of 0 .. ", N - 1);
    auto out = at::full({N}, -1, rowptr.options());
    if (!weight.has_value()) {
      visit_plain(rp, col.data_ptr<int64_t>(), perm.data_ptr<int64_t>(), N, out.data_ptr<int64_t>());
    } else {
      AT_DISPATCH_ALL_TYPES_AND2(at::kHalf, at::kBFloat16, weight->scalar_type(), "graclus_cpu", [&] {
        visit_weighted<scalar_t>(rp, col.data_ptr<int64_t>(), weight->data_ptr<scalar_t>(), perm.data_ptr<int64_t>(), N,
                                 out.data_ptr<int64_t>());
      });
    }
    return out;
  }
  TORCH_CHECK(!weight.has_value() || is_device_weight(weight->scalar_type()),
              "graclus_cluster: on a HIP device weight must be float32, float64, float16 or bfloat16 (got ", weight->scalar_type(), ")");
  auto out = at::empty({N}, rowptr.options());
  DeviceGuard guard(rowptr.device());
  const int flags = graclus_route_tls();
  const size_t bytes = pyg_hip_graclus_workspace_size(N, E, flags);
  auto ws = at::empty({(int64_t)std::max<size_t>(bytes, 16)}, rowptr.options().dtype(at::kByte));
  const bool weighted = weight.has_value() && E > 0;
  check_status(pyg_hip_graclus(rowptr.data_ptr<int64_t>(), col.data_ptr<int64_t>(),
                               weighted ? dtype_code(weight->scalar_type()) : PYG_HIP_GRACLUS_NO_WEIGHT,
                               weighted ? weight->data_ptr() : nullptr, perm.data_ptr<int64_t>(), N, E, flags, ws.data_ptr(), bytes,
                               out.data_ptr<int64_t>(), current_stream(rowptr)));
  return out;
}

Tensor graclus_kernel(const Tensor& rowptr, const Tensor& col, const std::optional<Tensor>& weight) {
  PYG_TRACE("pyg::graclus_cluster");
  check_graph(rowptr, col, weight.has_value() && weight->defined() ? weight : std::nullopt);
  TORCH_CHECK(rowptr.numel() >= 1, "graclus_cluster: rowptr must have at least 1 entry");
  // the reference's draw (ops/cpu/graclus_kernel.cpp:16), from the generator of the tensors' own device
  const Tensor perm = at::randperm(rowptr.numel() - 1, rowptr.options());
  return graclus_perm_kernel(rowptr, col, weight, perm);
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(pyg, m) {
  m.def(
      TORCH_SELECTIVE_SCHEMA("pyg::graclus_cluster(Tensor rowptr, Tensor col, "
                             "Tensor? weight=None) -> Tensor"));
  m.def(TORCH_SELECTIVE_SCHEMA("pyg::graclus_cluster_perm(Tensor rowptr, Tensor col, Tensor? weight, Tensor perm) -> Tensor"));
}

TORCH_LIBRARY_IMPL(pyg, CUDA, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::graclus_cluster"), TORCH_FN(graclus_kernel));
  m.impl(TORCH_SELECTIVE_NAME("pyg::graclus_cluster_perm"), TORCH_FN(graclus_perm_kernel));
}

TORCH_LIBRARY_IMPL(pyg, CPU, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::graclus_cluster"), TORCH_FN(graclus_kernel));
  m.impl(TORCH_SELECTIVE_NAME("pyg::graclus_cluster_perm"), TORCH_FN(graclus_perm_kernel));
}

}  // namespace pyg_amd

// PYG_HIP_GRACLUS_FORCE_SINGLE / _MULTI (0: the library's rule) for the graclus calls of this thread
extern "C" __attribute__((visibility("default"))) void pyg_binding_set_graclus_route(int flags) {
  pyg_amd::graclus_route_tls() = flags & PYG_HIP_GRACLUS_FORCE_MASK;
}
extern "C" __attribute__((visibility("default"))) int pyg_binding_get_graclus_route(void) { return pyg_amd::graclus_route_tls(); }
