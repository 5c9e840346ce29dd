// torch::Library binding of pyg::node2vec_walk and pyg::node2vec_walk_keyed (this build only: second-order random walks
// with the return parameter p and the in-out parameter q; the reference's pyg::random_walk stops at p = q = 1).
//   node2vec_walk_keyed  the deterministic core: a pure function of its arguments (specification: include/pyg_hip.h,
//                        "node2vec walks", and DESIGN.md 2.16), the same bit for bit on both keys.  No host read and no
//                        allocation beyond the output, so the CUDA key can be captured into a graph.
//   node2vec_walk        draws one 64-bit key from the torch generator of the tensors' device and calls the core with
//                        max_attempts = 32.
//   CUDA: csrc/hip/node2vec.hip through the C-ABI.
//   CPU:  the specification in plain C++ on at::Philox4_32, one engine per walk, walks in parallel.
#include <ATen/CPUGeneratorImpl.h>
#include <ATen/Parallel.h>
#include <ATen/TensorUtils.h>
#include <ATen/core/PhiloxRNGEngine.h>
#include <ATen/hip/HIPGeneratorImpl.h>
#include <torch/library.h>

#include <algorithm>
#include <cmath>
#include <mutex>

#include "binding_common.h"

namespace pyg_amd {
namespace {

constexpr int64_t kDefaultAttempts = 32;

struct Thresholds {
  float ret, near, far;
};

// argument checks shared by both keys (the tensor checks are those of random_walk, pyg_binding_walk.cpp)
Thresholds check_args(const char* op, const Tensor& rowptr, const Tensor& col, const Tensor& seed, int64_t walk_length,
                      double p, double q, int64_t max_attempts) {
  at::TensorArg rowptr_t{rowptr, "rowptr", 1};
  at::TensorArg col_t{col, "col", 2};
  at::TensorArg seed_t{seed, "seed", 3};
  at::CheckedFrom c = op;
  at::checkAllDefined(c, {rowptr_t, col_t, seed_t});
  at::checkAllSameType(c, {rowptr_t, col_t, seed_t});
  TORCH_CHECK(seed.scalar_type() == at::kInt || seed.scalar_type() == at::kLong, op,
              ": int32 or int64 indices expected (got ", seed.scalar_type(), ")");
  TORCH_CHECK(rowptr.dim() == 1 && col.dim() == 1 && seed.dim() == 1, op, ": 'rowptr', 'col' and 'seed' must be vectors");
  TORCH_CHECK(walk_length >= 0, op, ": 'walk_length' must be non-negative (got ", walk_length, ")");
  TORCH_CHECK(std::isfinite(p) && p > 0, op, ": 'p' must be finite and positive (got ", p, ")");
  TORCH_CHECK(std::isfinite(q) && q > 0, op, ": 'q' must be finite and positive (got ", q, ")");
  TORCH_CHECK(max_attempts >= 0 && max_attempts <= 1024, op, ": 'max_attempts' must lie in [0, 1024] (got ", max_attempts,
              ")");
  // once, in double, rounded to float32: every consumer compares against exactly these three values
  const double ip = 1.0 / p, iq = 1.0 / q;
  const double M = std::max(ip, std::max(1.0, iq));
  const Thresholds a{(float)(ip / M), (float)(1.0 / M), (float)(iq / M)};
  TORCH_CHECK(std::isfinite(M) && a.ret > 0 && a.near > 0 && a.far > 0, op, ": 'p' = ", p, " and 'q' = ", q,
              " are too far apart: a transition weight rounds to zero in float32");
  return a;
}

// ---- CUDA ----------------------------------------------------------------------------------------------------------

Tensor node2vec_walk_keyed_cuda(const Tensor& rowptr, const Tensor& col, const Tensor& seed, int64_t walk_length, double p,
                                double q, int64_t key, int64_t max_attempts) {
  PYG_TRACE("pyg::node2vec_walk_keyed");
  TORCH_CHECK(rowptr.is_cuda(), "'rowptr' must be a CUDA tensor");
  TORCH_CHECK(col.is_cuda(), "'col' must be a CUDA tensor");
  TORCH_CHECK(seed.is_cuda(), "'seed' must be a CUDA tensor");
  const Thresholds a = check_args("node2vec_walk", rowptr, col, seed, walk_length, p, q, max_attempts);
  TORCH_CHECK(rowptr.device() == col.device() && rowptr.device() == seed.device(),
              "node2vec_walk: 'rowptr', 'col' and 'seed' must live on the same device");
  DeviceGuard guard(seed.device());
  const auto rowptr_c = rowptr.contiguous(), col_c = col.contiguous(), seed_c = seed.contiguous();
  const int64_t S = seed.size(0);
  auto out = at::empty({S, walk_length + 1}, seed.options());
  check_status(pyg_hip_node2vec_walk(seed.scalar_type() == at::kInt ? PYG_I32 : PYG_I64, rowptr_c.data_ptr(),
                                     std::max<int64_t>(rowptr_c.numel() - 1, 0), col_c.data_ptr(), col_c.numel(),
                                     seed_c.data_ptr(), S, walk_length, a.ret, a.near, a.far, (uint64_t)key,
                                     (int)max_attempts, out.data_ptr(), current_stream(seed)));
  return out;
}

Tensor node2vec_walk_cuda(const Tensor& rowptr, const Tensor& col, const Tensor& seed, int64_t walk_length, double p,
                          double q) {
  TORCH_CHECK(seed.defined() && seed.is_cuda(), "'seed' must be a CUDA tensor");
  DeviceGuard guard(seed.device());
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  TORCH_CHECK(hipStreamIsCapturing(current_hip_stream((c10::DeviceIndex)seed.get_device()), &capturing) == hipSuccess,
              "node2vec_walk: hipStreamIsCapturing failed");
  TORCH_CHECK(capturing == hipStreamCaptureStatusNone,
              "node2vec_walk: draws its key from the generator on the host and cannot be captured into a graph (every "
              "replay would repeat the same walks); capture node2vec_walk_keyed with a key of your own instead");
  auto* gen = at::get_generator_or_default<at::CUDAGeneratorImpl>(
      c10::nullopt, at::cuda::detail::getDefaultCUDAGenerator(seed.get_device()));
  std::pair<uint64_t, uint64_t> inputs;
  {
    std::lock_guard<std::mutex> lock(gen->mutex_);
    inputs = gen->philox_engine_inputs(4);
  }
  return node2vec_walk_keyed_cuda(rowptr, col, seed, walk_length, p, q, (int64_t)mix_key(inputs.first, inputs.second),
                                  kDefaultAttempts);
}

// ---- CPU -----------------------------------------------------------------------------------------------------------

inline float uniform(uint32_t word) { return (float)(word >> 8) * 0x1p-24f; }

template <typename scalar_t>
void node2vec_walks_cpu(const scalar_t* rp, const scalar_t* cl, const scalar_t* sd, scalar_t* out, int64_t N, int64_t E,
                        int64_t S, int64_t L, Thresholds a, uint64_t key, int64_t max_attempts) {
  const bool search = a.near != a.far;
  at::parallel_for(0, S, 64, [&](int64_t begin, int64_t end) {
    for (int64_t i = begin; i < end; ++i) {
      at::Philox4_32 rng(key, /*subsequence=*/(uint64_t)i, /*offset=*/0);
      scalar_t* o = out + i * (L + 1);
      int64_t v = sd[i];
      o[0] = (scalar_t)v;
      int64_t t = 0, trs = 0, tre = 0;
      // the transition weight of candidate x: lower bound of x in col[trs, tre), the previous node's row
      auto weight = [&](int64_t x) -> float {
        if (x == t) return a.ret;
        if (!search) return a.near;
        int64_t lo = trs, hi = tre;
        while (lo < hi) {
          const int64_t mid = lo + (hi - lo) / 2;
          if ((int64_t)cl[mid] < x)
            lo = mid + 1;
          else
            hi = mid;
        }
        return lo < tre && (int64_t)cl[lo] == x ? a.near : a.far;
      };
      auto pick = [&](int64_t deg) -> int64_t {
        const int64_t k = (int64_t)(uniform(rng()) * (float)deg);
        return std::min(k, deg - 1);
      };
      for (int64_t j = 1; j <= L; ++j) {
        int64_t rs = 0, re = 0;
        if (v >= 0 && v < N) rs = rp[v], re = rp[v + 1];
        if (!(rs >= 0 && re > rs && re <= E)) {
          for (; j <= L; ++j) o[j] = (scalar_t)v;  // stays for good, draws nothing
          break;
        }
        const int64_t deg = re - rs;
        int64_t x = 0;
        if (j == 1) {
          x = cl[rs + pick(deg)];
        } else {
          bool accepted = false;
          for (int64_t k = 0; k < max_attempts && !accepted; ++k) {
            x = cl[rs + pick(deg)];
            const float r = uniform(rng());
            accepted = r < weight(x);
          }
          if (!accepted) {
            const float u = uniform(rng());
            double total = 0;
            for (int64_t k = 0; k < deg; ++k) total += (double)weight(cl[rs + k]);
            const double target = (double)u * total;
            double run = 0;
            int64_t k = 0;
            for (; k < deg - 1; ++k) {
              run += (double)weight(cl[rs + k]);
              if (run > target) break;
            }
            x = cl[rs + k];
          }
        }
        t = v, trs = rs, tre = re;
        v = x;
        o[j] = (scalar_t)v;
      }
    }
  });
}

Tensor node2vec_walk_keyed_cpu(const Tensor& rowptr, const Tensor& col, const Tensor& seed, int64_t walk_length, double p,
                               double q, int64_t key, int64_t max_attempts) {
  PYG_TRACE("pyg::node2vec_walk_keyed[cpu]");
  TORCH_CHECK(rowptr.is_cpu(), "'rowptr' must be a CPU tensor");
  TORCH_CHECK(col.is_cpu(), "'col' must be a CPU tensor");
  TORCH_CHECK(seed.is_cpu(), "'seed' must be a CPU tensor");
  const Thresholds a = check_args("node2vec_walk", rowptr, col, seed, walk_length, p, q, max_attempts);
  const auto rowptr_c = rowptr.contiguous(), col_c = col.contiguous(), seed_c = seed.contiguous();
  const int64_t S = seed.size(0);
  auto out = at::empty({S, walk_length + 1}, seed.options());
  const int64_t N = std::max<int64_t>(rowptr_c.numel() - 1, 0), E = col_c.numel();
  if (seed.scalar_type() == at::kInt)
    node2vec_walks_cpu<int32_t>(rowptr_c.data_ptr<int32_t>(), col_c.data_ptr<int32_t>(), seed_c.data_ptr<int32_t>(),
                                out.data_ptr<int32_t>(), N, E, S, walk_length, a, (uint64_t)key, max_attempts);
  else
    node2vec_walks_cpu<int64_t>(rowptr_c.data_ptr<int64_t>(), col_c.data_ptr<int64_t>(), seed_c.data_ptr<int64_t>(),
                                out.data_ptr<int64_t>(), N, E, S, walk_length, a, (uint64_t)key, max_attempts);
  return out;
}

Tensor node2vec_walk_cpu(const Tensor& rowptr, const Tensor& col, const Tensor& seed, int64_t walk_length, double p,
                         double q) {
  auto* gen = at::get_generator_or_default<at::CPUGeneratorImpl>(c10::nullopt, at::detail::getDefaultCPUGenerator());
  uint64_t key;
  {
    std::lock_guard<std::mutex> lock(gen->mutex_);
    key = gen->random64();
  }
  return node2vec_walk_keyed_cpu(rowptr, col, seed, walk_length, p, q, (int64_t)key, kDefaultAttempts);
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(pyg, m) {
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::node2vec_walk(Tensor rowptr, Tensor col, Tensor seed, int walk_length, float p, float q) -> Tensor"));
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::node2vec_walk_keyed(Tensor rowptr, Tensor col, Tensor seed, int walk_length, float p, float q, "
      "int key, int max_attempts=32) -> Tensor"));
}

TORCH_LIBRARY_IMPL(pyg, CUDA, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::node2vec_walk"), TORCH_FN(node2vec_walk_cuda));
  m.impl(TORCH_SELECTIVE_NAME("pyg::node2vec_walk_keyed"), TORCH_FN(node2vec_walk_keyed_cuda));
}

TORCH_LIBRARY_IMPL(pyg, CPU, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::node2vec_walk"), TORCH_FN(node2vec_walk_cpu));
  m.impl(TORCH_SELECTIVE_NAME("pyg::node2vec_walk_keyed"), TORCH_FN(node2vec_walk_keyed_cpu));
}

}  // namespace pyg_amd
