// torch::Library binding of pyg::fps and pyg::grid_cluster (schemas: pyg_lib/csrc/ops/fps.cpp and ops/cluster.cpp, byte for
// byte).  The outputs are integers: no Autograd key.  Key CUDA: csrc/hip/downsample.hip through the C-ABI.  Key CPU: the
// executable statement of the semantics in include/pyg_hip.h -- plain loops with the same arithmetic (no fused multiply-add,
// 16-bit inputs widened for fps and rounded after every operation for grid_cluster) and the same ordering rule, so both keys
// give the same bits.  A correctness key, not a hot path.
#include <ATen/Dispatch.h>
#include <ATen/Parallel.h>
#include <torch/library.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <optional>
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

// PYG_HIP_FPS_FORCE_* for the calls of this thread (pyg_binding_set_fps_route; tests and measurements)
int& fps_route_tls() {
  thread_local int flags = 0;
  return flags;
}

bool is_point_dtype(at::ScalarType t) { return t == at::kFloat || t == at::kDouble || t == at::kHalf || t == at::kBFloat16; }

template <typename scalar_t>
struct Acc {
  using type = float;
};
template <>
struct Acc<double> {
  using type = double;
};

// ---- fps ---------------------------------------------------------------------------------------------------------------
// what both keys compute with torch operators, the reference's expressions (ops/cpu/fps_kernel.cpp:20-22, ops/cuda/fps_kernel.cu)
struct FpsSizes {
  Tensor deg, out_ptr, start;   // [B] int64 each, on src's device
  Tensor summary;               // [4] int64: the largest example, the largest count, the output size, ptr is valid
};

FpsSizes fps_sizes(const Tensor& src, const Tensor& ptr, double ratio, bool random_start) {
  FpsSizes s;
  const int64_t B = ptr.numel() - 1, N = src.size(0);
  s.deg = ptr.narrow(0, 1, B) - ptr.narrow(0, 0, B);
  const Tensor count = (s.deg.to(at::kFloat) * ratio).ceil().to(at::kLong);
  s.out_ptr = count.cumsum(0);
  if (random_start) {
    // the product can round up to deg: clamped into the example
    const Tensor drawn = (at::rand({B}, src.options()) * s.deg.to(at::kFloat)).to(at::kLong);
    s.start = at::minimum(drawn, s.deg - 1).clamp_min(0);
  } else {
    s.start = at::zeros({B}, ptr.options());
  }
  const Tensor ok = ((s.deg >= 0).all() & (ptr[0] == 0) & (ptr[B] == N)).to(at::kLong);
  s.summary = at::stack({s.deg.max(), count.max(), s.out_ptr[B - 1], ok});
  return s;
}

template <typename scalar_t>
void fps_cpu_typed(const Tensor& src, const int64_t* ptr, const int64_t* out_ptr, const int64_t* start, int64_t B, int64_t* out) {
  using acc_t = typename Acc<scalar_t>::type;
  const int64_t D = src.size(1);
  const scalar_t* x = src.data_ptr<scalar_t>();
  at::parallel_for(0, B, 1, [&](int64_t begin, int64_t end) {
    std::vector<acc_t> run;
    for (int64_t b = begin; b < end; ++b) {
      const int64_t lo = ptr[b], n = ptr[b + 1] - lo;
      const int64_t olo = b ? out_ptr[b - 1] : 0, count = out_ptr[b] - olo;
      if (n == 0) continue;
      run.assign((size_t)n, acc_t(0));
      int64_t w = start[b];
      for (int64_t m = 0;; ++m) {
        out[olo + m] = lo + w;
        if (m + 1 >= count) break;
        const scalar_t* c = x + (lo + w) * D;
        acc_t best = 0;
        bool best_nan = true;   // a NaN ranks below every number: the first number beats it, a later NaN never does
        int64_t best_j = 0;
        for (int64_t j = 0; j < n; ++j) {
          const scalar_t* p = x + (lo + j) * D;
          acc_t nw = 0;
          for (int64_t d = 0; d < D; ++d) {
            const acc_t diff = static_cast<acc_t>(p[d]) - static_cast<acc_t>(c[d]);
            nw = nw + diff * diff;
          }
          const acc_t r = (m == 0 || nw < run[(size_t)j]) ? nw : run[(size_t)j];
          run[(size_t)j] = r;
          if (r == r && (best_nan || r > best)) best = r, best_nan = false, best_j = j;
        }
        w = best_j;
      }
    }
  });
}

Tensor fps_kernel(const Tensor& src_, const Tensor& ptr_, double ratio, bool random_start) {
  PYG_TRACE("pyg::fps");
  TORCH_CHECK(src_.defined() && ptr_.defined(), "fps: src and ptr must be defined");
  TORCH_CHECK(ptr_.dim() == 1, "fps: ptr must be 1-D (got ", ptr_.dim(), " dimensions)");
  TORCH_CHECK(ratio > 0.0 && ratio <= 1.0, "ratio must be in the range (0, 1]");
  TORCH_CHECK(src_.dim() >= 1, "fps: src must have at least one dimension");
  TORCH_CHECK(is_point_dtype(src_.scalar_type()), "fps: src must be float32, float64, float16 or bfloat16 (got ", src_.scalar_type(), ")");
  TORCH_CHECK(ptr_.scalar_type() == at::kLong, "fps: ptr must be an int64 tensor (got ", ptr_.scalar_type(), ")");
  TORCH_CHECK(ptr_.numel() >= 1, "fps: ptr must have at least 1 entry");
  TORCH_CHECK(ptr_.device() == src_.device(), "fps: ptr must live on the device of src (got ", ptr_.device(), ", expected ", src_.device(), ")");
  const int64_t N = src_.size(0);
  const Tensor src = src_.reshape({N, N ? -1 : std::max<int64_t>(1, src_.numel())}).contiguous();
  const Tensor ptr = ptr_.contiguous();
  const int64_t B = ptr.numel() - 1, D = src.size(1);
  TORCH_CHECK(D >= 1, "fps: the feature dimension must be at least 1");
  TORCH_CHECK(N < (int64_t(1) << 31), "fps: 2^31 or more points");
  if (B == 0) return at::empty({0}, ptr.options());
  const bool on_device = !src.is_cpu();
  std::optional<DeviceGuard> guard;
  if (on_device) guard.emplace(src.device());
  const FpsSizes s = fps_sizes(src, ptr, ratio, random_start);
  const Tensor host = s.summary.cpu();   // the one read-back
  const int64_t max_points = host[0].item<int64_t>(), max_samples = host[1].item<int64_t>(), total = host[2].item<int64_t>();
  TORCH_CHECK(host[3].item<int64_t>() == 1, "fps: ptr must be non-decreasing, begin at 0 and end at the number of rows");
  auto out = at::empty({total}, ptr.options());
  if (total == 0) return out;
  if (!on_device) {
    const Tensor out_ptr = s.out_ptr.contiguous(), start = s.start.contiguous();
    AT_DISPATCH_FLOATING_TYPES_AND2(at::kHalf, at::kBFloat16, src.scalar_type(), "fps_cpu", [&] {
      fps_cpu_typed<scalar_t>(src, ptr.data_ptr<int64_t>(), out_ptr.data_ptr<int64_t>(), start.data_ptr<int64_t>(), B, out.data_ptr<int64_t>());
    });
    return out;
  }
  const int flags = fps_route_tls();
  const int dtype = dtype_code(src.scalar_type());
  const size_t bytes = pyg_hip_fps_workspace_size(dtype, N, B, D, max_points, max_samples, flags);
  auto ws = at::empty({(int64_t)std::max<size_t>(bytes, 16)}, src.options().dtype(at::kByte));
  const Tensor out_ptr = s.out_ptr.contiguous(), start = s.start.contiguous();
  check_status(pyg_hip_fps(dtype, src.data_ptr(), N, D, ptr.data_ptr<int64_t>(), B, out_ptr.data_ptr<int64_t>(), start.data_ptr<int64_t>(),
                           max_points, max_samples, flags, ws.data_ptr(), bytes, out.data_ptr<int64_t>(), total, current_stream(src)));
  return out;
}

// ---- grid_cluster ------------------------------------------------------------------------------------------------------
// int64() of include/pyg_hip.h: NaN -> 0, saturating
template <typename acc_t>
inline int64_t to_i64(acc_t v) {
  if (!(v == v)) return 0;
  if (v >= acc_t(9223372036854775808.0)) return std::numeric_limits<int64_t>::max();
  if (v <= acc_t(-9223372036854775808.0)) return std::numeric_limits<int64_t>::min();
  return static_cast<int64_t>(v);
}

// R: round to the storage type (the identity for float and double)
template <typename scalar_t>
inline typename Acc<scalar_t>::type rnd(typename Acc<scalar_t>::type v) {
  return static_cast<typename Acc<scalar_t>::type>(static_cast<scalar_t>(v));
}

template <typename scalar_t>
inline int64_t voxel(typename Acc<scalar_t>::type pos, typename Acc<scalar_t>::type start, typename Acc<scalar_t>::type size) {
  using acc_t = typename Acc<scalar_t>::type;
  const acc_t shifted = rnd<scalar_t>(pos - start);
  const acc_t q = rnd<scalar_t>(shifted / size);
  return to_i64<acc_t>(std::trunc(q));
}

template <typename scalar_t>
void grid_cluster_cpu_typed(const Tensor& pos, const Tensor& size, const std::optional<Tensor>& start_, const std::optional<Tensor>& end_,
                            int64_t* out) {
  using acc_t = typename Acc<scalar_t>::type;
  const int64_t N = pos.size(0), D = pos.size(1);
  const scalar_t* x = pos.data_ptr<scalar_t>();
  const scalar_t* sz = size.data_ptr<scalar_t>();
  std::vector<acc_t> st((size_t)D), en((size_t)D);
  // torch.min / torch.max over a column: a NaN wins and stays
  for (int64_t d = 0; d < D; ++d) {
    acc_t mn = static_cast<acc_t>(x[d]), mx = mn;
    for (int64_t i = 1; i < N; ++i) {
      const acc_t v = static_cast<acc_t>(x[i * D + d]);
      if (mn == mn && (v < mn || v != v)) mn = v;
      if (mx == mx && (v > mx || v != v)) mx = v;
    }
    st[(size_t)d] = start_.has_value() ? static_cast<acc_t>(start_->data_ptr<scalar_t>()[d]) : mn;
    en[(size_t)d] = end_.has_value() ? static_cast<acc_t>(end_->data_ptr<scalar_t>()[d]) : mx;
  }
  std::vector<uint64_t> mul((size_t)D);
  uint64_t run = 1;
  for (int64_t d = 0; d < D; ++d) {
    mul[(size_t)d] = run;
    run *= static_cast<uint64_t>(voxel<scalar_t>(en[(size_t)d], st[(size_t)d], static_cast<acc_t>(sz[d])) + 1);
  }
  at::parallel_for(0, N, 1024, [&](int64_t begin, int64_t end) {
    for (int64_t i = begin; i < end; ++i) {
      uint64_t id = 0;
      for (int64_t d = 0; d < D; ++d)
        id += static_cast<uint64_t>(voxel<scalar_t>(static_cast<acc_t>(x[i * D + d]), st[(size_t)d], static_cast<acc_t>(sz[d]))) * mul[(size_t)d];
      out[i] = static_cast<int64_t>(id);
    }
  });
}

Tensor grid_cluster_kernel(const Tensor& pos_, const Tensor& size_, const std::optional<Tensor>& start_, const std::optional<Tensor>& end_) {
  PYG_TRACE("pyg::grid_cluster");
  TORCH_CHECK(pos_.defined() && size_.defined(), "grid_cluster: pos and size must be defined");
  TORCH_CHECK(pos_.dim() >= 1, "grid_cluster: pos must have at least one dimension");
  TORCH_CHECK(is_point_dtype(pos_.scalar_type()), "grid_cluster: pos must be float32, float64, float16 or bfloat16 (got ",
              pos_.scalar_type(), ")");
  const int64_t N = pos_.size(0);
  const Tensor pos = pos_.reshape({N, N ? -1 : std::max<int64_t>(1, size_.numel())}).contiguous();
  const int64_t D = pos.size(1);
  TORCH_CHECK(size_.numel() == D, "size.numel() must equal pos dimension count");
  auto take = [&](const std::optional<Tensor>& t, const char* text) -> std::optional<Tensor> {
    if (!t.has_value() || !t->defined()) return std::nullopt;
    TORCH_CHECK(t->numel() == D, text);
    TORCH_CHECK(t->scalar_type() == pos.scalar_type() && t->device() == pos.device(),
                "grid_cluster: size, start and end must have the dtype and the device of pos");
    return t->contiguous();
  };
  TORCH_CHECK(size_.scalar_type() == pos.scalar_type() && size_.device() == pos.device(),
              "grid_cluster: size, start and end must have the dtype and the device of pos");
  TORCH_CHECK(D >= 1, "grid_cluster: the feature dimension must be at least 1");
  const Tensor size = size_.contiguous();
  const std::optional<Tensor> start = take(start_, "start.numel() must equal pos dimension count");
  const std::optional<Tensor> end = take(end_, "end.numel() must equal pos dimension count");
  auto out = at::empty({N}, pos.options().dtype(at::kLong));
  if (N == 0) return out;
  if (pos.is_cpu()) {
    AT_DISPATCH_FLOATING_TYPES_AND2(at::kHalf, at::kBFloat16, pos.scalar_type(), "grid_cluster_cpu",
                                    [&] { grid_cluster_cpu_typed<scalar_t>(pos, size, start, end, out.data_ptr<int64_t>()); });
    return out;
  }
  DeviceGuard guard(pos.device());
  const int dtype = dtype_code(pos.scalar_type());
  const size_t bytes = pyg_hip_grid_cluster_workspace_size(dtype, N, D, start.has_value(), end.has_value());
  auto ws = at::empty({(int64_t)std::max<size_t>(bytes, 16)}, pos.options().dtype(at::kByte));
  check_status(pyg_hip_grid_cluster(dtype, pos.data_ptr(), N, D, size.data_ptr(), start.has_value() ? start->data_ptr() : nullptr,
                                    end.has_value() ? end->data_ptr() : nullptr, ws.data_ptr(), bytes, out.data_ptr<int64_t>(),
                                    current_stream(pos)));
  return out;
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(pyg, m) {
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::fps(Tensor src, Tensor ptr, float ratio=0.5, "
      "bool random_start=True) -> Tensor"));
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::grid_cluster(Tensor pos, Tensor size, "
      "Tensor? start=None, Tensor? end=None) -> Tensor"));
}

TORCH_LIBRARY_IMPL(pyg, CUDA, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::fps"), TORCH_FN(fps_kernel));
  m.impl(TORCH_SELECTIVE_NAME("pyg::grid_cluster"), TORCH_FN(grid_cluster_kernel));
}

TORCH_LIBRARY_IMPL(pyg, CPU, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::fps"), TORCH_FN(fps_kernel));
  m.impl(TORCH_SELECTIVE_NAME("pyg::grid_cluster"), TORCH_FN(grid_cluster_kernel));
}

}  // namespace pyg_amd

// PYG_HIP_FPS_FORCE_RESIDENT / _STREAM / _MULTI (0: the library's rule) for the fps calls of this thread
extern "C" __attribute__((visibility("default"))) void pyg_binding_set_fps_route(int flags) {
  pyg_amd::fps_route_tls() = flags & PYG_HIP_FPS_FORCE_MASK;
}
extern "C" __attribute__((visibility("default"))) int pyg_binding_get_fps_route(void) { return pyg_amd::fps_route_tls(); }
