// torch::Library binding of the six pyg::spline_* operators (schemas: pyg_lib/csrc/ops/spline.cpp, byte for byte; checks and
// .contiguous() calls as there).  Key CUDA: csrc/hip/spline.hip through the C-ABI.  Key CPU: the executable statement of the
// semantics in include/pyg_hip.h -- plain loops, every sum sequential in the stated order, no fused multiply-add, bfloat16
// rounded after every step as the reference's scalar code does -- which equals the reference's CPU kernels bit for bit
// (tests/golden/spline_golden.npz).  Key Autograd: spline_basis and spline_weighting, wired as ops/autograd/spline_kernel.cpp:
// weight_index is non-differentiable, a gradient is computed only where needed, the backward operators go through the
// dispatcher.
#include <ATen/Dispatch.h>
#include <ATen/Parallel.h>
#include <ATen/core/dispatch/Dispatcher.h>
#include <torch/autograd.h>
#include <torch/library.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <tuple>

#include "binding_common.h"

// every product and every sum is rounded on its own (the device kernels are built the same way)
#if defined(__FMA__) && defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pyg_amd {
namespace {

// PYG_HIP_SPLINE_FORCE_* for the calls of this thread (pyg_binding_set_spline_route; tests and measurements)
int& spline_route_tls() {
  thread_local int flags = 0;
  return flags;
}

// ---- the B-spline pieces: the reference's operand types (double literals against a scalar_t `v`) ------------------------
template <typename scalar_t, int64_t degree>
struct Piece {
  static inline scalar_t value(scalar_t v, int64_t k_mod) {
    if (degree == 1) {
      return 1. - v - k_mod + 2. * v * k_mod;
    } else if (degree == 2) {
      if (k_mod == 0) return 0.5 * v * v - v + 0.5;
      if (k_mod == 1) return -v * v + v + 0.5;
      return 0.5 * v * v;
    } else {
      if (k_mod == 0) return (1. - v) * (1. - v) * (1. - v) / 6.;
      if (k_mod == 1) return (3. * v * v * v - 6. * v * v + 4.) / 6.;
      if (k_mod == 2) return (-3. * v * v * v + 3. * v * v + 3. * v + 1.) / 6.;
      return v * v * v / 6.;
    }
  }
  static inline scalar_t grad(scalar_t v, int64_t k_mod) {
    if (degree == 1) {
      return 2 * k_mod - 1;
    } else if (degree == 2) {
      if (k_mod == 0) return v - 1.;
      if (k_mod == 1) return -2. * v + 1.;
      return v;
    } else {
      if (k_mod == 0) return (-v * v + 2. * v - 1.) / 2.;
      if (k_mod == 1) return (3. * v * v - 4. * v) / 2.;
      if (k_mod == 2) return (-3. * v * v + 2. * v + 1.) / 2.;
      return v * v / 2.;
    }
  }
};

int64_t ipow(int64_t base, int64_t exp) {
  int64_t r = 1;
  for (int64_t i = 0; i < exp; ++i) r *= base;
  return r;
}

template <typename scalar_t, int64_t DEG>
void basis_cpu(const scalar_t* pseudo, const int64_t* ks, const uint8_t* open, int64_t E, int64_t D, int64_t S, scalar_t* basis,
               int64_t* weight_index) {
  at::parallel_for(0, E, 256, [&](int64_t begin, int64_t end) {
    for (int64_t e = begin; e < end; ++e)
      for (int64_t s = 0; s < S; ++s) {
        int64_t k = s, wi = 0, offset = 1;
        scalar_t b = (scalar_t)1.;
        for (int64_t d = 0; d < D; ++d) {
          const int64_t k_mod = k % (DEG + 1);
          k /= DEG + 1;
          auto v = pseudo[e * D + d];
          v *= ks[d] - DEG * open[d];
          wi += (ks[d] != 0 ? ((int64_t)v + k_mod) % ks[d] : 0) * offset;
          offset *= ks[d];
          v -= floor(v);
          v = Piece<scalar_t, DEG>::value(v, k_mod);
          b *= v;
        }
        basis[e * S + s] = b;
        weight_index[e * S + s] = wi;
      }
  });
}

template <typename scalar_t, int64_t DEG>
void basis_backward_cpu(const scalar_t* grad_basis, const scalar_t* pseudo, const int64_t* ks, const uint8_t* open, int64_t E, int64_t D,
                        int64_t S, scalar_t* grad_pseudo) {
  at::parallel_for(0, E, 256, [&](int64_t begin, int64_t end) {
    for (int64_t e = begin; e < end; ++e)
      for (int64_t d = 0; d < D; ++d) {
        scalar_t g = (scalar_t)0.;
        for (int64_t s = 0; s < S; ++s) {
          int64_t k_mod = (s / ipow(DEG + 1, d)) % (DEG + 1);
          auto v = pseudo[e * D + d];
          v *= ks[d] - DEG * open[d];
          v -= floor(v);
          v = Piece<scalar_t, DEG>::grad(v, k_mod);
          scalar_t tmp = v;
          for (int64_t d_it = 1; d_it < D; ++d_it) {
            const int64_t d_new = d_it - (d >= d_it);
            k_mod = (s / ipow(DEG + 1, d_new)) % (DEG + 1);
            v = pseudo[e * D + d_new];
            v *= ks[d_new] - DEG * open[d_new];
            v -= floor(v);
            v = Piece<scalar_t, DEG>::value(v, k_mod);
            tmp *= v;
          }
          g += tmp * grad_basis[e * S + s];
        }
        g *= ks[d] - DEG * open[d];
        grad_pseudo[e * D + d] = g;
      }
  });
}

#define PYG_SPLINE_DEGREE(degree, ...)                          \
  [&] {                                                         \
    switch (degree) {                                           \
      case 1: { constexpr int64_t DEG = 1; return __VA_ARGS__(); } \
      case 2: { constexpr int64_t DEG = 2; return __VA_ARGS__(); } \
      case 3: { constexpr int64_t DEG = 3; return __VA_ARGS__(); } \
      default: TORCH_CHECK(false, "Basis degree not implemented"); \
    }                                                           \
  }()

void check_basis_args(const Tensor& pseudo, const Tensor& kernel_size, const Tensor& is_open_spline, int64_t degree, const char* op) {
  TORCH_CHECK(pseudo.defined() && kernel_size.defined() && is_open_spline.defined(), op, ": undefined tensor");
  TORCH_CHECK(pseudo.dim() == 2, op, ": expected a 2-dimensional pseudo (got ", pseudo.dim(), " dimensions)");
  TORCH_CHECK(kernel_size.dim() == 1, op, ": expected a 1-dimensional kernel_size (got ", kernel_size.dim(), " dimensions)");
  TORCH_CHECK(is_open_spline.dim() == 1, op, ": expected a 1-dimensional is_open_spline (got ", is_open_spline.dim(), " dimensions)");
  TORCH_CHECK(pseudo.size(1) == kernel_size.numel(), "pseudo.size(1) must equal kernel_size.numel()");
  TORCH_CHECK(pseudo.size(1) == is_open_spline.numel(), "pseudo.size(1) must equal is_open_spline.numel()");
  TORCH_CHECK(kernel_size.scalar_type() == at::kLong, op, ": kernel_size must be an int64 tensor (got ", kernel_size.scalar_type(), ")");
  TORCH_CHECK(is_open_spline.scalar_type() == at::kByte, op, ": is_open_spline must be a uint8 tensor (got ", is_open_spline.scalar_type(), ")");
  TORCH_CHECK(kernel_size.device() == pseudo.device() && is_open_spline.device() == pseudo.device(), op,
              ": kernel_size and is_open_spline must live on the device of pseudo");
  TORCH_CHECK(degree >= 1 && degree <= 3, "Basis degree not implemented");
  TORCH_CHECK(pseudo.size(1) <= 16, op, ": more than 16 pseudo-coordinate dimensions");
}

std::tuple<Tensor, Tensor> spline_basis_kernel(const Tensor& pseudo_, const Tensor& kernel_size_, const Tensor& is_open_spline_, int64_t degree) {
  PYG_TRACE("pyg::spline_basis");
  check_basis_args(pseudo_, kernel_size_, is_open_spline_, degree, "spline_basis");
  const Tensor pseudo = pseudo_.contiguous(), kernel_size = kernel_size_.contiguous(), is_open = is_open_spline_.contiguous();
  const int64_t E = pseudo.size(0), D = pseudo.size(1), S = ipow(degree + 1, D);
  Tensor basis, weight_index;
  if (pseudo.is_cpu()) {
    AT_DISPATCH_FLOATING_TYPES_AND(at::kBFloat16, pseudo.scalar_type(), "spline_basis_fw", [&] {
      basis = at::empty({E, S}, pseudo.options());
      weight_index = at::empty({E, S}, kernel_size.options());
      PYG_SPLINE_DEGREE(degree, [&] {
        basis_cpu<scalar_t, DEG>(pseudo.data_ptr<scalar_t>(), kernel_size.data_ptr<int64_t>(), is_open.data_ptr<uint8_t>(), E, D, S,
                                 basis.data_ptr<scalar_t>(), weight_index.data_ptr<int64_t>());
      });
    });
    return std::make_tuple(basis, weight_index);
  }
  AT_DISPATCH_FLOATING_TYPES(pseudo.scalar_type(), "spline_basis_fw", [&] {});
  DeviceGuard guard(pseudo.device());
  basis = at::empty({E, S}, pseudo.options());
  weight_index = at::empty({E, S}, kernel_size.options());
  check_status(pyg_hip_spline_basis(dtype_code(pseudo.scalar_type()), pseudo.data_ptr(), kernel_size.data_ptr<int64_t>(),
                                    is_open.data_ptr<uint8_t>(), E, D, (int)degree, basis.data_ptr(), weight_index.data_ptr<int64_t>(),
                                    current_stream(pseudo)));
  return std::make_tuple(basis, weight_index);
}

Tensor spline_basis_backward_kernel(const Tensor& grad_basis_, const Tensor& pseudo_, const Tensor& kernel_size_, const Tensor& is_open_spline_,
                                    int64_t degree) {
  PYG_TRACE("pyg::spline_basis_backward");
  TORCH_CHECK(grad_basis_.defined(), "spline_basis_backward: undefined tensor");
  check_basis_args(pseudo_, kernel_size_, is_open_spline_, degree, "spline_basis_backward");
  TORCH_CHECK(grad_basis_.dim() == 2, "spline_basis_backward: expected a 2-dimensional grad_basis (got ", grad_basis_.dim(), " dimensions)");
  TORCH_CHECK(grad_basis_.size(0) == pseudo_.size(0), "grad_basis.size(0) must equal pseudo.size(0)");
  TORCH_CHECK(grad_basis_.scalar_type() == pseudo_.scalar_type() && grad_basis_.device() == pseudo_.device(),
              "spline_basis_backward: grad_basis must have the dtype and the device of pseudo");
  const Tensor grad_basis = grad_basis_.contiguous(), pseudo = pseudo_.contiguous(), kernel_size = kernel_size_.contiguous(),
               is_open = is_open_spline_.contiguous();
  const int64_t E = pseudo.size(0), D = pseudo.size(1), S = grad_basis.size(1);
  TORCH_CHECK(S <= ipow(degree + 1, D), "spline_basis_backward: grad_basis has more than (degree + 1)^D columns");
  Tensor grad_pseudo;
  if (pseudo.is_cpu()) {
    AT_DISPATCH_FLOATING_TYPES_AND(at::kBFloat16, pseudo.scalar_type(), "spline_basis_bw", [&] {
      grad_pseudo = at::empty({E, D}, pseudo.options());
      PYG_SPLINE_DEGREE(degree, [&] {
        basis_backward_cpu<scalar_t, DEG>(grad_basis.data_ptr<scalar_t>(), pseudo.data_ptr<scalar_t>(), kernel_size.data_ptr<int64_t>(),
                                          is_open.data_ptr<uint8_t>(), E, D, S, grad_pseudo.data_ptr<scalar_t>());
      });
    });
    return grad_pseudo;
  }
  AT_DISPATCH_FLOATING_TYPES(pseudo.scalar_type(), "spline_basis_bw", [&] {});
  DeviceGuard guard(pseudo.device());
  grad_pseudo = at::empty({E, D}, pseudo.options());
  check_status(pyg_hip_spline_basis_backward(dtype_code(pseudo.scalar_type()), grad_basis.data_ptr(), pseudo.data_ptr(),
                                             kernel_size.data_ptr<int64_t>(), is_open.data_ptr<uint8_t>(), E, D, S, (int)degree,
                                             grad_pseudo.data_ptr(), current_stream(pseudo)));
  return grad_pseudo;
}

// ---- weighting -----------------------------------------------------------------------------------------------------------
// the sizes of a weighting-family call, checked once for all four operators
struct Sizes {
  int64_t E, S, M_in, M_out, K;
};

void check_same(const Tensor& a, const Tensor& b, const char* op) {
  TORCH_CHECK(a.scalar_type() == b.scalar_type() && a.device() == b.device(), op, ": the floating tensors must share one dtype and one device");
}

void check_index(const Tensor& weight_index, const Tensor& like, int64_t E, int64_t K, const char* op) {
  TORCH_CHECK(weight_index.dim() == 2, op, ": expected a 2-dimensional weight_index (got ", weight_index.dim(), " dimensions)");
  TORCH_CHECK(weight_index.scalar_type() == at::kLong, op, ": weight_index must be an int64 tensor (got ", weight_index.scalar_type(), ")");
  TORCH_CHECK(weight_index.device() == like.device(), op, ": weight_index must live on the device of the other tensors");
  TORCH_CHECK(weight_index.size(0) == E, op, ": weight_index.size(0) must equal the number of edges");
  if (weight_index.is_cpu() && weight_index.numel() > 0) {
    const Tensor c = weight_index.contiguous();
    const int64_t* p = c.data_ptr<int64_t>();
    for (int64_t i = 0; i < c.numel(); ++i)
      TORCH_CHECK(p[i] >= 0 && p[i] < K, op, ": weight_index[", i / c.size(1), ", ", i % c.size(1), "] = ", p[i], " is outside [0, ", K, ")");
  }
}

template <typename scalar_t>
void weighting_cpu(const scalar_t* x, const scalar_t* w, const scalar_t* basis, const int64_t* wi, const Sizes& z, scalar_t* out) {
  at::parallel_for(0, z.E, 64, [&](int64_t begin, int64_t end) {
    for (int64_t e = begin; e < end; ++e)
      for (int64_t o = 0; o < z.M_out; ++o) {
        scalar_t v = 0;
        for (int64_t s = 0; s < z.S; ++s) {
          const scalar_t b = basis[e * z.S + s];
          const scalar_t* wk = w + wi[e * z.S + s] * z.M_in * z.M_out;
          for (int64_t i = 0; i < z.M_in; ++i) {
            scalar_t tmp = wk[i * z.M_out + o];
            tmp *= b * x[e * z.M_in + i];
            v += tmp;
          }
        }
        out[e * z.M_out + o] = v;
      }
  });
}

template <typename scalar_t>
void backward_x_cpu(const scalar_t* g, const scalar_t* w, const scalar_t* basis, const int64_t* wi, const Sizes& z, scalar_t* gx) {
  at::parallel_for(0, z.E, 64, [&](int64_t begin, int64_t end) {
    for (int64_t e = begin; e < end; ++e)
      for (int64_t i = 0; i < z.M_in; ++i) {
        scalar_t v = 0;
        for (int64_t o = 0; o < z.M_out; ++o) {
          const scalar_t go = g[e * z.M_out + o];
          for (int64_t s = 0; s < z.S; ++s) v += go * basis[e * z.S + s] * w[(wi[e * z.S + s] * z.M_in + i) * z.M_out + o];
        }
        gx[e * z.M_in + i] = v;
      }
  });
}

template <typename scalar_t>
void backward_basis_cpu(const scalar_t* g, const scalar_t* x, const scalar_t* w, const int64_t* wi, const Sizes& z, scalar_t* gb) {
  at::parallel_for(0, z.E, 64, [&](int64_t begin, int64_t end) {
    for (int64_t e = begin; e < end; ++e)
      for (int64_t s = 0; s < z.S; ++s) {
        const scalar_t* wk = w + wi[e * z.S + s] * z.M_in * z.M_out;
        scalar_t v = 0;
        for (int64_t o = 0; o < z.M_out; ++o) {
          scalar_t t = 0;
          for (int64_t i = 0; i < z.M_in; ++i) {
            scalar_t p = wk[i * z.M_out + o];
            p *= x[e * z.M_in + i];
            t += p;
          }
          v += g[e * z.M_out + o] * t;
        }
        gb[e * z.S + s] = v;
      }
  });
}

// one thread owns a block of (i, o) elements of every weight: the pairs arrive in order of e, then s, for each of them
template <typename scalar_t>
void backward_weight_cpu(const scalar_t* g, const scalar_t* x, const scalar_t* basis, const int64_t* wi, const Sizes& z, scalar_t* gw) {
  at::parallel_for(0, z.M_in, 1, [&](int64_t begin, int64_t end) {
    for (int64_t e = 0; e < z.E; ++e)
      for (int64_t s = 0; s < z.S; ++s) {
        const scalar_t b = basis[e * z.S + s];
        scalar_t* gk = gw + wi[e * z.S + s] * z.M_in * z.M_out;
        for (int64_t i = begin; i < end; ++i) {
          const scalar_t xi = x[e * z.M_in + i];
          for (int64_t o = 0; o < z.M_out; ++o) gk[i * z.M_out + o] += g[e * z.M_out + o] * b * xi;
        }
      }
  });
}

#define PYG_SPLINE_TYPES(t, name, ...) AT_DISPATCH_FLOATING_TYPES_AND(at::kBFloat16, t, name, __VA_ARGS__)

Tensor spline_weighting_kernel(const Tensor& x_, const Tensor& weight_, const Tensor& basis_, const Tensor& weight_index_) {
  PYG_TRACE("pyg::spline_weighting");
  const char* op = "spline_weighting";
  TORCH_CHECK(x_.defined() && weight_.defined() && basis_.defined() && weight_index_.defined(), op, ": undefined tensor");
  TORCH_CHECK(x_.dim() == 2, op, ": expected a 2-dimensional x (got ", x_.dim(), " dimensions)");
  TORCH_CHECK(weight_.dim() == 3, op, ": expected a 3-dimensional weight (got ", weight_.dim(), " dimensions)");
  TORCH_CHECK(basis_.dim() == 2, op, ": expected a 2-dimensional basis (got ", basis_.dim(), " dimensions)");
  TORCH_CHECK(weight_index_.dim() == 2, op, ": expected a 2-dimensional weight_index (got ", weight_index_.dim(), " dimensions)");
  TORCH_CHECK(x_.size(1) == weight_.size(1), "x.size(1) must equal weight.size(1)");
  TORCH_CHECK(x_.size(0) == basis_.size(0), "x.size(0) must equal basis.size(0)");
  TORCH_CHECK(x_.size(0) == weight_index_.size(0), "x.size(0) must equal weight_index.size(0)");
  TORCH_CHECK(basis_.size(1) == weight_index_.size(1), "basis.size(1) must equal weight_index.size(1)");
  check_same(x_, weight_, op), check_same(x_, basis_, op);
  const Sizes z{x_.size(0), basis_.size(1), x_.size(1), weight_.size(2), weight_.size(0)};
  check_index(weight_index_, x_, z.E, z.K, op);
  const Tensor x = x_.contiguous(), weight = weight_.contiguous(), basis = basis_.contiguous(), wi = weight_index_.contiguous();
  Tensor out;
  PYG_SPLINE_TYPES(x.scalar_type(), "spline_weighting_fw", [&] {
    out = at::empty({z.E, z.M_out}, x.options());
    if (x.is_cpu())
      weighting_cpu<scalar_t>(x.data_ptr<scalar_t>(), weight.data_ptr<scalar_t>(), basis.data_ptr<scalar_t>(), wi.data_ptr<int64_t>(), z,
                              out.data_ptr<scalar_t>());
  });
  if (x.is_cpu()) return out;
  DeviceGuard guard(x.device());
  check_status(pyg_hip_spline_weighting(dtype_code(x.scalar_type()), x.data_ptr(), weight.data_ptr(), basis.data_ptr(), wi.data_ptr<int64_t>(),
                                        z.E, z.S, z.M_in, z.M_out, z.K, spline_route_tls(), out.data_ptr(), current_stream(x)));
  return out;
}

Tensor spline_weighting_backward_x_kernel(const Tensor& grad_out_, const Tensor& weight_, const Tensor& basis_, const Tensor& weight_index_) {
  PYG_TRACE("pyg::spline_weighting_backward_x");
  const char* op = "spline_weighting_backward_x";
  TORCH_CHECK(grad_out_.defined() && weight_.defined() && basis_.defined() && weight_index_.defined(), op, ": undefined tensor");
  TORCH_CHECK(grad_out_.dim() == 2 && weight_.dim() == 3 && basis_.dim() == 2, op, ": expected grad_out [E, M_out], weight [K, M_in, M_out], basis [E, S]");
  TORCH_CHECK(grad_out_.size(1) == weight_.size(2), "grad_out.size(1) must equal weight.size(2)");
  TORCH_CHECK(grad_out_.size(0) == basis_.size(0), "grad_out.size(0) must equal basis.size(0)");
  check_same(grad_out_, weight_, op), check_same(grad_out_, basis_, op);
  const Sizes z{grad_out_.size(0), basis_.size(1), weight_.size(1), grad_out_.size(1), weight_.size(0)};
  check_index(weight_index_, grad_out_, z.E, z.K, op);
  TORCH_CHECK(basis_.size(1) == weight_index_.size(1), "basis.size(1) must equal weight_index.size(1)");
  const Tensor g = grad_out_.contiguous(), weight = weight_.contiguous(), basis = basis_.contiguous(), wi = weight_index_.contiguous();
  Tensor grad_x;
  PYG_SPLINE_TYPES(g.scalar_type(), "spline_weighting_bw_x", [&] {
    grad_x = at::empty({z.E, z.M_in}, g.options());
    if (g.is_cpu())
      backward_x_cpu<scalar_t>(g.data_ptr<scalar_t>(), weight.data_ptr<scalar_t>(), basis.data_ptr<scalar_t>(), wi.data_ptr<int64_t>(), z,
                               grad_x.data_ptr<scalar_t>());
  });
  if (g.is_cpu()) return grad_x;
  DeviceGuard guard(g.device());
  const int dtype = dtype_code(g.scalar_type());
  const size_t bytes = pyg_hip_spline_backward_x_workspace_size(dtype, z.M_in, z.M_out, z.K);
  auto ws = at::empty({(int64_t)std::max<size_t>(bytes, 16)}, g.options().dtype(at::kByte));
  check_status(pyg_hip_spline_weighting_backward_x(dtype, g.data_ptr(), weight.data_ptr(), basis.data_ptr(), wi.data_ptr<int64_t>(), z.E, z.S,
                                                   z.M_in, z.M_out, z.K, spline_route_tls(), ws.data_ptr(), bytes, grad_x.data_ptr(),
                                                   current_stream(g)));
  return grad_x;
}

Tensor spline_weighting_backward_weight_kernel(const Tensor& grad_out_, const Tensor& x_, const Tensor& basis_, const Tensor& weight_index_,
                                               int64_t kernel_size) {
  PYG_TRACE("pyg::spline_weighting_backward_weight");
  const char* op = "spline_weighting_backward_weight";
  TORCH_CHECK(grad_out_.defined() && x_.defined() && basis_.defined() && weight_index_.defined(), op, ": undefined tensor");
  TORCH_CHECK(grad_out_.dim() == 2 && x_.dim() == 2 && basis_.dim() == 2, op, ": expected grad_out [E, M_out], x [E, M_in], basis [E, S]");
  TORCH_CHECK(grad_out_.size(0) == x_.size(0), "grad_out.size(0) must equal x.size(0)");
  TORCH_CHECK(grad_out_.size(0) == basis_.size(0), "grad_out.size(0) must equal basis.size(0)");
  TORCH_CHECK(kernel_size >= 0, op, ": negative kernel_size");
  check_same(grad_out_, x_, op), check_same(grad_out_, basis_, op);
  const Sizes z{grad_out_.size(0), basis_.size(1), x_.size(1), grad_out_.size(1), kernel_size};
  check_index(weight_index_, grad_out_, z.E, z.K, op);
  TORCH_CHECK(basis_.size(1) == weight_index_.size(1), "basis.size(1) must equal weight_index.size(1)");
  const Tensor g = grad_out_.contiguous(), x = x_.contiguous(), basis = basis_.contiguous(), wi = weight_index_.contiguous();
  Tensor grad_weight;
  PYG_SPLINE_TYPES(g.scalar_type(), "spline_weighting_bw_weight", [&] {
    if (g.is_cpu()) {
      grad_weight = at::zeros({z.K, z.M_in, z.M_out}, g.options());
      backward_weight_cpu<scalar_t>(g.data_ptr<scalar_t>(), x.data_ptr<scalar_t>(), basis.data_ptr<scalar_t>(), wi.data_ptr<int64_t>(), z,
                                    grad_weight.data_ptr<scalar_t>());
    }
  });
  if (g.is_cpu()) return grad_weight;
  DeviceGuard guard(g.device());
  grad_weight = at::empty({z.K, z.M_in, z.M_out}, g.options());
  const int dtype = dtype_code(g.scalar_type());
  const size_t bytes = pyg_hip_spline_backward_weight_workspace_size(dtype, z.E, z.S, z.M_in, z.M_out, z.K, 0);
  auto ws = at::empty({(int64_t)std::max<size_t>(bytes, 16)}, g.options().dtype(at::kByte));
  check_status(pyg_hip_spline_weighting_backward_weight(dtype, g.data_ptr(), x.data_ptr(), basis.data_ptr(), wi.data_ptr<int64_t>(), z.E, z.S,
                                                        z.M_in, z.M_out, z.K, 0, ws.data_ptr(), bytes, grad_weight.data_ptr(),
                                                        current_stream(g)));
  return grad_weight;
}

Tensor spline_weighting_backward_basis_kernel(const Tensor& grad_out_, const Tensor& x_, const Tensor& weight_, const Tensor& weight_index_) {
  PYG_TRACE("pyg::spline_weighting_backward_basis");
  const char* op = "spline_weighting_backward_basis";
  TORCH_CHECK(grad_out_.defined() && x_.defined() && weight_.defined() && weight_index_.defined(), op, ": undefined tensor");
  TORCH_CHECK(grad_out_.dim() == 2 && x_.dim() == 2 && weight_.dim() == 3, op, ": expected grad_out [E, M_out], x [E, M_in], weight [K, M_in, M_out]");
  TORCH_CHECK(grad_out_.size(0) == x_.size(0), "grad_out.size(0) must equal x.size(0)");
  TORCH_CHECK(x_.size(1) == weight_.size(1), "x.size(1) must equal weight.size(1)");
  TORCH_CHECK(grad_out_.size(1) == weight_.size(2), "grad_out.size(1) must equal weight.size(2)");
  check_same(grad_out_, x_, op), check_same(grad_out_, weight_, op);
  TORCH_CHECK(weight_index_.dim() == 2, op, ": expected a 2-dimensional weight_index");
  const Sizes z{grad_out_.size(0), weight_index_.size(1), x_.size(1), grad_out_.size(1), weight_.size(0)};
  check_index(weight_index_, grad_out_, z.E, z.K, op);
  const Tensor g = grad_out_.contiguous(), x = x_.contiguous(), weight = weight_.contiguous(), wi = weight_index_.contiguous();
  Tensor grad_basis;
  PYG_SPLINE_TYPES(g.scalar_type(), "spline_weighting_bw_basis", [&] {
    grad_basis = at::empty({z.E, z.S}, g.options());
    if (g.is_cpu())
      backward_basis_cpu<scalar_t>(g.data_ptr<scalar_t>(), x.data_ptr<scalar_t>(), weight.data_ptr<scalar_t>(), wi.data_ptr<int64_t>(), z,
                                   grad_basis.data_ptr<scalar_t>());
  });
  if (g.is_cpu()) return grad_basis;
  DeviceGuard guard(g.device());
  check_status(pyg_hip_spline_weighting_backward_basis(dtype_code(g.scalar_type()), g.data_ptr(), x.data_ptr(), weight.data_ptr(),
                                                       wi.data_ptr<int64_t>(), z.E, z.S, z.M_in, z.M_out, z.K, spline_route_tls(),
                                                       grad_basis.data_ptr(), current_stream(g)));
  return grad_basis;
}

// ---- autograd: the wiring of ops/autograd/spline_kernel.cpp ----------------------------------------------------------------
using torch::autograd::variable_list;

template <typename Sig>
auto dispatch(const char* name) {
  return c10::Dispatcher::singleton().findSchemaOrThrow(name, "").typed<Sig>();
}

class SplineBasis : public torch::autograd::Function<SplineBasis> {
 public:
  static variable_list forward(torch::autograd::AutogradContext* ctx, const Tensor& pseudo, const Tensor& kernel_size,
                               const Tensor& is_open_spline, int64_t degree) {
    at::AutoDispatchBelowADInplaceOrView g;
    static auto op = dispatch<std::tuple<Tensor, Tensor>(const Tensor&, const Tensor&, const Tensor&, int64_t)>("pyg::spline_basis");
    auto result = op.call(pseudo, kernel_size, is_open_spline, degree);
    ctx->saved_data["degree"] = degree;
    ctx->save_for_backward({pseudo, kernel_size, is_open_spline});
    ctx->mark_non_differentiable({std::get<1>(result)});
    return {std::get<0>(result), std::get<1>(result)};
  }

  static variable_list backward(torch::autograd::AutogradContext* ctx, variable_list grad_outs) {
    const auto saved = ctx->get_saved_variables();
    Tensor grad_pseudo;
    if (torch::autograd::any_variable_requires_grad({saved[0]})) {
      static auto op = dispatch<Tensor(const Tensor&, const Tensor&, const Tensor&, const Tensor&, int64_t)>("pyg::spline_basis_backward");
      grad_pseudo = op.call(grad_outs[0], saved[0], saved[1], saved[2], ctx->saved_data["degree"].toInt());
    }
    return {grad_pseudo, Tensor(), Tensor(), Tensor()};
  }
};

class SplineWeighting : public torch::autograd::Function<SplineWeighting> {
 public:
  static variable_list forward(torch::autograd::AutogradContext* ctx, const Tensor& x, const Tensor& weight, const Tensor& basis,
                               const Tensor& weight_index) {
    at::AutoDispatchBelowADInplaceOrView g;
    static auto op = dispatch<Tensor(const Tensor&, const Tensor&, const Tensor&, const Tensor&)>("pyg::spline_weighting");
    auto out = op.call(x, weight, basis, weight_index);
    ctx->save_for_backward({x, weight, basis, weight_index});
    return {out};
  }

  static variable_list backward(torch::autograd::AutogradContext* ctx, variable_list grad_outs) {
    const auto grad_out = grad_outs[0];
    const auto saved = ctx->get_saved_variables();
    const auto x = saved[0], weight = saved[1], basis = saved[2], weight_index = saved[3];
    using Sig4 = Tensor(const Tensor&, const Tensor&, const Tensor&, const Tensor&);
    Tensor grad_x, grad_weight, grad_basis;
    if (torch::autograd::any_variable_requires_grad({x})) {
      static auto op = dispatch<Sig4>("pyg::spline_weighting_backward_x");
      grad_x = op.call(grad_out, weight, basis, weight_index);
    }
    if (torch::autograd::any_variable_requires_grad({weight})) {
      static auto op = dispatch<Tensor(const Tensor&, const Tensor&, const Tensor&, const Tensor&, int64_t)>("pyg::spline_weighting_backward_weight");
      grad_weight = op.call(grad_out, x, basis, weight_index, weight.size(0));
    }
    if (torch::autograd::any_variable_requires_grad({basis})) {
      static auto op = dispatch<Sig4>("pyg::spline_weighting_backward_basis");
      grad_basis = op.call(grad_out, x, weight, weight_index);
    }
    return {grad_x, grad_weight, grad_basis, Tensor()};
  }
};

std::tuple<Tensor, Tensor> spline_basis_autograd(const Tensor& pseudo, const Tensor& kernel_size, const Tensor& is_open_spline, int64_t degree) {
  auto result = SplineBasis::apply(pseudo, kernel_size, is_open_spline, degree);
  return std::make_tuple(result[0], result[1]);
}

Tensor spline_weighting_autograd(const Tensor& x, const Tensor& weight, const Tensor& basis, const Tensor& weight_index) {
  return SplineWeighting::apply(x, weight, basis, weight_index)[0];
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(pyg, m) {
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::spline_basis(Tensor pseudo, Tensor kernel_size, "
      "Tensor is_open_spline, int degree=1) -> (Tensor, Tensor)"));
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::spline_basis_backward(Tensor grad_basis, Tensor pseudo, "
      "Tensor kernel_size, Tensor is_open_spline, int degree=1) -> Tensor"));
  m.def(
      TORCH_SELECTIVE_SCHEMA("pyg::spline_weighting(Tensor x, Tensor weight, "
                             "Tensor basis, Tensor weight_index) -> Tensor"));
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::spline_weighting_backward_x(Tensor grad_out, Tensor weight, "
      "Tensor basis, Tensor weight_index) -> Tensor"));
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::spline_weighting_backward_weight(Tensor grad_out, Tensor x, "
      "Tensor basis, Tensor weight_index, int kernel_size) -> Tensor"));
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::spline_weighting_backward_basis(Tensor grad_out, Tensor x, "
      "Tensor weight, Tensor weight_index) -> Tensor"));
}

#define PYG_SPLINE_IMPLS(m)                                                                                                      \
  m.impl(TORCH_SELECTIVE_NAME("pyg::spline_basis"), TORCH_FN(spline_basis_kernel));                                              \
  m.impl(TORCH_SELECTIVE_NAME("pyg::spline_basis_backward"), TORCH_FN(spline_basis_backward_kernel));                            \
  m.impl(TORCH_SELECTIVE_NAME("pyg::spline_weighting"), TORCH_FN(spline_weighting_kernel));                                      \
  m.impl(TORCH_SELECTIVE_NAME("pyg::spline_weighting_backward_x"), TORCH_FN(spline_weighting_backward_x_kernel));                \
  m.impl(TORCH_SELECTIVE_NAME("pyg::spline_weighting_backward_weight"), TORCH_FN(spline_weighting_backward_weight_kernel));      \
  m.impl(TORCH_SELECTIVE_NAME("pyg::spline_weighting_backward_basis"), TORCH_FN(spline_weighting_backward_basis_kernel));

TORCH_LIBRARY_IMPL(pyg, CUDA, m) { PYG_SPLINE_IMPLS(m) }

TORCH_LIBRARY_IMPL(pyg, CPU, m) { PYG_SPLINE_IMPLS(m) }

TORCH_LIBRARY_IMPL(pyg, Autograd, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::spline_basis"), TORCH_FN(spline_basis_autograd));
  m.impl(TORCH_SELECTIVE_NAME("pyg::spline_weighting"), TORCH_FN(spline_weighting_autograd));
}

}  // namespace pyg_amd

// PYG_HIP_SPLINE_FORCE_LDS / _GLOBAL (0: the library's rule) for the spline_weighting calls of this thread
extern "C" __attribute__((visibility("default"))) void pyg_binding_set_spline_route(int flags) {
  pyg_amd::spline_route_tls() = flags & PYG_HIP_SPLINE_FORCE_MASK;
}
extern "C" __attribute__((visibility("default"))) int pyg_binding_get_spline_route(void) { return pyg_amd::spline_route_tls(); }
