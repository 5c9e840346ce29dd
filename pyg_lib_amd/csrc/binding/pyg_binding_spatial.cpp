// torch::Library binding of pyg::knn, pyg::radius and pyg::nearest (schemas: pyg_lib/csrc/ops/{knn,radius,nearest}.cpp, byte for
// byte).  The outputs are integers: no Autograd key.  Key CUDA: csrc/hip/spatial.hip through the C-ABI.  Key CPU: the
// executable statement of the semantics in include/pyg_hip.h -- a brute-force loop with the same arithmetic (no fused
// multiply-add) and the same ordering rule, parallel over the queries.  A correctness key, not a hot path: no KD-tree, and
// radius follows the device rule (ascending candidate index, the first max_num_neighbors), not the reference's KD-tree order.
#include <ATen/Dispatch.h>
#include <ATen/Parallel.h>
#include <torch/library.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <optional>
#include <utility>
#include <vector>

#include "binding_common.h"

// a - b, d * d and s + d * d are rounded one by one (the device kernels are built the same way)
#if defined(__FMA__) && defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pyg_amd {
namespace {

// PYG_HIP_SPATIAL_FORCE_* for the calls of this thread (pyg_binding_set_spatial_route; tests and measurements)
int& spatial_route_tls() {
  thread_local int flags = 0;
  return flags;
}

struct Ptrs {
  std::optional<Tensor> q, c;   // kept alive; contiguous int64
  const int64_t* q_data = nullptr;
  const int64_t* c_data = nullptr;
  int64_t B = 1;
};

void check_points(const char* name, const Tensor& x, const Tensor& y) {
  TORCH_CHECK(x.defined() && y.defined(), name, ": x and y must be defined");
  TORCH_CHECK(x.dim() == 2 && y.dim() == 2, name, ": x and y must be 2-D (got ", x.dim(), " and ", y.dim(), " dimensions)");
  TORCH_CHECK(x.size(1) == y.size(1), "x and y must have the same feature dim");
  TORCH_CHECK(x.size(1) >= 1, name, ": the feature dimension must be at least 1");
  TORCH_CHECK(x.scalar_type() == y.scalar_type(), name, ": x and y must have the same dtype (got ", x.scalar_type(), " and ",
              y.scalar_type(), ")");
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kDouble || x.scalar_type() == at::kHalf ||
                  x.scalar_type() == at::kBFloat16,
              name, ": x and y must be float32, float64, float16 or bfloat16 (got ", x.scalar_type(), ")");
  TORCH_CHECK(x.device() == y.device(), name, ": x and y must live on the same device (got ", x.device(), " and ", y.device(), ")");
}

// ptr_q belongs to the queries, ptr_c to the candidates; a missing one stands for the single example [0, rows]
Ptrs take_ptrs(const char* name, const Tensor& points, const std::optional<Tensor>& ptr_q, const std::optional<Tensor>& ptr_c) {
  Ptrs r;
  auto one = [&](const std::optional<Tensor>& ptr, std::optional<Tensor>& keep) -> int64_t {
    if (!ptr.has_value() || !ptr->defined()) return 2;
    TORCH_CHECK(ptr->scalar_type() == at::kLong, name, ": ptr_x and ptr_y must be int64 tensors (got ", ptr->scalar_type(), ")");
    TORCH_CHECK(ptr->dim() == 1 && ptr->numel() >= 2, name, ": ptr_x and ptr_y must be 1-D with at least 2 entries");
    TORCH_CHECK(ptr->device() == points.device(), name, ": ptr_x and ptr_y must live on the device of x and y (got ", ptr->device(),
                ", expected ", points.device(), ")");
    keep = ptr->contiguous();
    return keep->numel();
  };
  const int64_t nq = one(ptr_q, r.q), nc = one(ptr_c, r.c);
  TORCH_CHECK(nq == nc, "ptr_x and ptr_y must have the same number of elements");
  r.B = nq - 1;
  if (r.q.has_value()) r.q_data = r.q->data_ptr<int64_t>();
  if (r.c.has_value()) r.c_data = r.c->data_ptr<int64_t>();
  return r;
}

// ---- key CPU --------------------------------------------------------------------------------------------------------
template <typename scalar_t>
struct Acc {
  using type = float;
};
template <>
struct Acc<double> {
  using type = double;
};

template <typename acc_t, typename scalar_t>
inline acc_t sq_dist(const scalar_t* a, const scalar_t* b, int64_t D) {
  acc_t dist = 0;
  for (int64_t d = 0; d < D; ++d) {
    const acc_t diff = static_cast<acc_t>(a[d]) - static_cast<acc_t>(b[d]);
    dist = dist + diff * diff;
  }
  return dist;
}

struct Seg {
  int64_t qlo, qhi, clo, chi;
};

// the examples, validated (the device reports the same conditions through its flag) and clamped like the kernels do
std::vector<Seg> cpu_segments(const char* name, const Ptrs& p, int64_t M, int64_t N) {
  auto check = [&](const int64_t* ptr, int64_t rows) {
    if (!ptr) return;
    for (int64_t b = 0; b < p.B; ++b) TORCH_CHECK(ptr[b] <= ptr[b + 1], name, ": ptr_x / ptr_y must be non-decreasing and end at the number of rows");
    TORCH_CHECK(ptr[p.B] == rows, name, ": ptr_x / ptr_y must be non-decreasing and end at the number of rows");
  };
  check(p.q_data, M);
  check(p.c_data, N);
  auto bounds = [](const int64_t* ptr, int64_t b, int64_t n, int64_t& lo, int64_t& hi) {
    if (!ptr) {
      lo = 0, hi = n;
      return;
    }
    lo = std::min(std::max<int64_t>(ptr[b], 0), n);
    hi = std::min(std::max(ptr[b + 1], lo), n);
  };
  std::vector<Seg> segs((size_t)p.B);
  for (int64_t b = 0; b < p.B; ++b) {
    bounds(p.q_data, b, M, segs[(size_t)b].qlo, segs[(size_t)b].qhi);
    bounds(p.c_data, b, N, segs[(size_t)b].clo, segs[(size_t)b].chi);
  }
  return segs;
}

// counts [M] -> out [2, E] through fill(i, row_out, col_out)
template <typename Fill>
Tensor emit_pairs(const std::vector<int64_t>& count, const at::TensorOptions& longs, Fill fill) {
  const int64_t M = (int64_t)count.size();
  std::vector<int64_t> offs((size_t)M + 1, 0);
  for (int64_t i = 0; i < M; ++i) offs[(size_t)i + 1] = offs[(size_t)i] + count[(size_t)i];
  const int64_t E = offs[(size_t)M];
  auto out = at::empty({2, E}, longs);
  int64_t* o = out.data_ptr<int64_t>();
  at::parallel_for(0, M, 64, [&](int64_t begin, int64_t end) {
    for (int64_t i = begin; i < end; ++i) fill(i, o + offs[(size_t)i], o + E + offs[(size_t)i]);
  });
  return out;
}

template <typename scalar_t>
Tensor knn_cpu_typed(const Tensor& x, const Tensor& y, const Ptrs& p, int64_t k) {
  using acc_t = typename Acc<scalar_t>::type;
  const int64_t N = x.size(0), M = y.size(0), D = x.size(1);
  const auto segs = cpu_segments("knn", p, M, N);
  const scalar_t* xd = x.data_ptr<scalar_t>();
  const scalar_t* yd = y.data_ptr<scalar_t>();
  std::vector<int64_t> count((size_t)M, 0);
  std::vector<std::vector<int64_t>> best((size_t)M);
  for (const Seg& s : segs)
    at::parallel_for(s.qlo, s.qhi, 16, [&](int64_t begin, int64_t end) {
      std::vector<std::pair<acc_t, int64_t>> cand;
      for (int64_t i = begin; i < end; ++i) {
        cand.clear();
        for (int64_t j = s.clo; j < s.chi; ++j) {
          const acc_t dist = sq_dist<acc_t>(yd + i * D, xd + j * D, D);
          if (dist < std::numeric_limits<acc_t>::infinity()) cand.emplace_back(dist, j);   // (false for a NaN)
        }
        const size_t keep = std::min<size_t>((size_t)k, cand.size());
        std::partial_sort(cand.begin(), cand.begin() + (std::ptrdiff_t)keep, cand.end());   // (distance, index)
        best[(size_t)i].resize(keep);
        for (size_t e = 0; e < keep; ++e) best[(size_t)i][e] = cand[e].second;
        count[(size_t)i] = (int64_t)keep;
      }
    });
  return emit_pairs(count, x.options().dtype(at::kLong), [&](int64_t i, int64_t* row, int64_t* col) {
    for (size_t e = 0; e < best[(size_t)i].size(); ++e) row[e] = i, col[e] = best[(size_t)i][e];
  });
}

template <typename scalar_t>
Tensor radius_cpu_typed(const Tensor& x, const Tensor& y, const Ptrs& p, double r, int64_t max_num_neighbors, bool ignore_same_index) {
  using acc_t = typename Acc<scalar_t>::type;
  const int64_t N = x.size(0), M = y.size(0), D = x.size(1);
  const auto segs = cpu_segments("radius", p, M, N);
  const scalar_t* xd = x.data_ptr<scalar_t>();
  const scalar_t* yd = y.data_ptr<scalar_t>();
  const acc_t r2 = static_cast<acc_t>(r * r);
  std::vector<int64_t> count((size_t)M, 0);
  std::vector<std::vector<int64_t>> hits((size_t)M);
  for (const Seg& s : segs)
    at::parallel_for(s.qlo, s.qhi, 16, [&](int64_t begin, int64_t end) {
      for (int64_t i = begin; i < end; ++i) {
        auto& h = hits[(size_t)i];
        for (int64_t j = s.clo; j < s.chi && (int64_t)h.size() < max_num_neighbors; ++j) {
          if (ignore_same_index && j == i) continue;
          if (sq_dist<acc_t>(yd + i * D, xd + j * D, D) < r2) h.push_back(j);
        }
        count[(size_t)i] = (int64_t)h.size();
      }
    });
  return emit_pairs(count, x.options().dtype(at::kLong), [&](int64_t i, int64_t* row, int64_t* col) {
    for (size_t e = 0; e < hits[(size_t)i].size(); ++e) row[e] = i, col[e] = hits[(size_t)i][e];
  });
}

template <typename scalar_t>
Tensor nearest_cpu_typed(const Tensor& x, const Tensor& y, const Ptrs& p) {
  using acc_t = typename Acc<scalar_t>::type;
  const int64_t N = x.size(0), M = y.size(0), D = x.size(1);
  const auto segs = cpu_segments("nearest", p, N, M);
  const scalar_t* xd = x.data_ptr<scalar_t>();
  const scalar_t* yd = y.data_ptr<scalar_t>();
  auto out = at::zeros({N}, x.options().dtype(at::kLong));
  int64_t* o = out.data_ptr<int64_t>();
  for (const Seg& s : segs)
    at::parallel_for(s.qlo, s.qhi, 16, [&](int64_t begin, int64_t end) {
      for (int64_t i = begin; i < end; ++i) {
        acc_t best = std::numeric_limits<acc_t>::infinity();
        int64_t best_j = s.clo;
        for (int64_t j = s.clo; j < s.chi; ++j) {
          const acc_t dist = sq_dist<acc_t>(xd + i * D, yd + j * D, D);
          if (dist < best) best = dist, best_j = j;
        }
        o[i] = best_j;
      }
    });
  return out;
}

// ---- the three operators ---------------------------------------------------------------------------------------------
struct Workspace {
  Tensor buf;
  size_t bytes = 0;
  void* ptr() { return bytes ? buf.data_ptr() : nullptr; }
};

Workspace take_workspace(int op, const Tensor& like, int64_t M, int64_t N, int64_t B, int64_t D, int64_t k, int flags) {
  Workspace w;
  w.bytes = pyg_hip_spatial_workspace_size(op, dtype_code(like.scalar_type()), M, N, B, D, k, flags);
  w.buf = at::empty({(int64_t)std::max<size_t>(w.bytes, 16)}, like.options().dtype(at::kByte));
  return w;
}

Tensor knn_kernel(const Tensor& x_, const Tensor& y_, const std::optional<Tensor>& ptr_x, const std::optional<Tensor>& ptr_y,
                  int64_t k, bool cosine, int64_t num_workers) {
  PYG_TRACE("pyg::knn");
  (void)num_workers;
  check_points("knn", x_, y_);
  TORCH_CHECK(k > 0, "k must be positive");
  const Tensor x = x_.contiguous(), y = y_.contiguous();
  const Ptrs p = take_ptrs("knn", x, ptr_y, ptr_x);
  const int64_t N = x.size(0), M = y.size(0), D = x.size(1);
  if (x.is_cpu()) {
    TORCH_CHECK(!cosine, "`cosine` argument not supported on CPU");
    Tensor out;
    AT_DISPATCH_FLOATING_TYPES_AND2(at::kHalf, at::kBFloat16, x.scalar_type(), "knn_cpu", [&] { out = knn_cpu_typed<scalar_t>(x, y, p, k); });
    return out;
  }
  DeviceGuard guard(x.device());
  const int flags = spatial_route_tls() | (cosine ? PYG_HIP_SPATIAL_COSINE : 0);
  const int dtype = dtype_code(x.scalar_type());
  // (an unsupported k gets its message from the entry point: the size query has no channel for one)
  Workspace w = take_workspace(PYG_SPATIAL_KNN, x, M, N, p.B, D, k, flags);
  int64_t E = 0;
  check_status(pyg_hip_knn(dtype, x.data_ptr(), N, y.data_ptr(), M, D, p.c_data, p.q_data, p.B, k, flags, w.buf.data_ptr(), w.bytes, &E,
                           current_stream(x)));
  auto out = at::empty({2, E}, x.options().dtype(at::kLong));
  check_status(pyg_hip_knn_emit(dtype, N, M, D, p.B, k, flags, w.buf.data_ptr(), w.bytes, E, out.data_ptr<int64_t>(), current_stream(x)));
  return out;
}

Tensor radius_kernel(const Tensor& x_, const Tensor& y_, const std::optional<Tensor>& ptr_x, const std::optional<Tensor>& ptr_y,
                     double r, int64_t max_num_neighbors, int64_t num_workers, bool ignore_same_index) {
  PYG_TRACE("pyg::radius");
  (void)num_workers;
  check_points("radius", x_, y_);
  TORCH_CHECK(r >= 0, "radius: r must not be negative");
  TORCH_CHECK(max_num_neighbors >= 0, "radius: max_num_neighbors must not be negative");
  const Tensor x = x_.contiguous(), y = y_.contiguous();
  const Ptrs p = take_ptrs("radius", x, ptr_y, ptr_x);
  const int64_t N = x.size(0), M = y.size(0), D = x.size(1);
  if (x.is_cpu()) {
    Tensor out;
    AT_DISPATCH_FLOATING_TYPES_AND2(at::kHalf, at::kBFloat16, x.scalar_type(), "radius_cpu",
                                    [&] { out = radius_cpu_typed<scalar_t>(x, y, p, r, max_num_neighbors, ignore_same_index); });
    return out;
  }
  DeviceGuard guard(x.device());
  const int flags = spatial_route_tls() | (ignore_same_index ? PYG_HIP_SPATIAL_IGNORE_SAME : 0);
  const int dtype = dtype_code(x.scalar_type());
  Workspace w = take_workspace(PYG_SPATIAL_RADIUS, x, M, N, p.B, D, max_num_neighbors, flags);
  int64_t E = 0;
  check_status(pyg_hip_radius(dtype, x.data_ptr(), N, y.data_ptr(), M, D, p.c_data, p.q_data, p.B, r, max_num_neighbors, flags,
                              w.buf.data_ptr(), w.bytes, &E, current_stream(x)));
  auto out = at::empty({2, E}, x.options().dtype(at::kLong));
  check_status(pyg_hip_radius_emit(dtype, x.data_ptr(), N, y.data_ptr(), M, D, p.c_data, p.q_data, p.B, r, max_num_neighbors, flags,
                                   w.buf.data_ptr(), w.bytes, E, out.data_ptr<int64_t>(), current_stream(x)));
  return out;
}

Tensor nearest_kernel(const Tensor& x_, const Tensor& y_, const std::optional<Tensor>& ptr_x, const std::optional<Tensor>& ptr_y) {
  PYG_TRACE("pyg::nearest");
  TORCH_CHECK(x_.defined() && y_.defined() && x_.dim() >= 2 && y_.dim() >= 2, "nearest: x and y must have at least two dimensions");
  // (the reference views them as [rows, -1], which an empty tensor does not allow)
  const Tensor x = (x_.dim() == 2 ? x_ : x_.flatten(1)).contiguous(), y = (y_.dim() == 2 ? y_ : y_.flatten(1)).contiguous();
  check_points("nearest", x, y);
  const Ptrs p = take_ptrs("nearest", x, ptr_x, ptr_y);
  const int64_t N = x.size(0), M = y.size(0), D = x.size(1);
  if (x.is_cpu()) {
    Tensor out;
    AT_DISPATCH_FLOATING_TYPES_AND2(at::kHalf, at::kBFloat16, x.scalar_type(), "nearest_cpu", [&] { out = nearest_cpu_typed<scalar_t>(x, y, p); });
    return out;
  }
  DeviceGuard guard(x.device());
  const int flags = spatial_route_tls();
  Workspace w = take_workspace(PYG_SPATIAL_NEAREST, x, N, M, p.B, D, 1, flags);
  auto out = at::empty({N}, x.options().dtype(at::kLong));
  check_status(pyg_hip_nearest(dtype_code(x.scalar_type()), x.data_ptr(), N, y.data_ptr(), M, D, p.q_data, p.c_data, p.B, flags,
                               w.buf.data_ptr(), w.bytes, out.data_ptr<int64_t>(), current_stream(x)));
  return out;
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(pyg, m) {
  m.def(
      TORCH_SELECTIVE_SCHEMA("pyg::knn(Tensor x, Tensor y, Tensor? ptr_x=None, "
                             "Tensor? ptr_y=None, int k=1, bool cosine=False, "
                             "int num_workers=1) -> Tensor"));
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::radius(Tensor x, Tensor y, Tensor? ptr_x=None, "
      "Tensor? ptr_y=None, float r=1.0, int max_num_neighbors=32, "
      "int num_workers=1, bool ignore_same_index=False) -> Tensor"));
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::nearest(Tensor x, Tensor y, Tensor? ptr_x=None, "
      "Tensor? ptr_y=None) -> Tensor"));
}

TORCH_LIBRARY_IMPL(pyg, CUDA, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::knn"), TORCH_FN(knn_kernel));
  m.impl(TORCH_SELECTIVE_NAME("pyg::radius"), TORCH_FN(radius_kernel));
  m.impl(TORCH_SELECTIVE_NAME("pyg::nearest"), TORCH_FN(nearest_kernel));
}

TORCH_LIBRARY_IMPL(pyg, CPU, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::knn"), TORCH_FN(knn_kernel));
  m.impl(TORCH_SELECTIVE_NAME("pyg::radius"), TORCH_FN(radius_kernel));
  m.impl(TORCH_SELECTIVE_NAME("pyg::nearest"), TORCH_FN(nearest_kernel));
}

}  // namespace pyg_amd

// PYG_HIP_SPATIAL_FORCE_LANE / _FORCE_SPLIT (0: the library's rule) for the knn / radius / nearest calls of this thread
extern "C" __attribute__((visibility("default"))) void pyg_binding_set_spatial_route(int flags) {
  pyg_amd::spatial_route_tls() = flags & (PYG_HIP_SPATIAL_FORCE_LANE | PYG_HIP_SPATIAL_FORCE_SPLIT);
}
extern "C" __attribute__((visibility("default"))) int pyg_binding_get_spatial_route(void) { return pyg_amd::spatial_route_tls(); }
