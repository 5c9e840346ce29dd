// torch::Library binding of pyg::random_walk and pyg::subgraph.  Schemas byte-identical to
// pyg_lib/csrc/sampler/random_walk.cpp:29-32 and sampler/subgraph.cpp:29-32.
//   CUDA: csrc/hip/walk.hip through the C-ABI.  random_walk draws its uniforms here, exactly as the reference's CUDA kernel
//         does (sampler/cuda/random_walk_kernel.cu:69-70: one at::rand({walk_length, num_seeds}) on the seeds' device),
//         so the torch generator advances identically and the walks agree bit for bit.
//   CPU:  restatements of the reference's CPU kernels.  random_walk = sampler/cpu/random_walk_kernel.cpp:13-55 on one
//         intra-op thread (one engine for all seeds, in seed order); subgraph = sampler/cpu/subgraph_kernel.cpp:13-92 with a
//         direct node table in place of the Mapper (same ids: order of first occurrence).
// Both keys treat a node id outside [0, num_nodes) -- a seed, an entry of `nodes` or of col -- as an isolated node that
// is nobody's neighbour, and never read outside rowptr / col (the reference's behaviour there is undefined).
#include <ATen/Parallel.h>
#include <ATen/TensorUtils.h>
#include <torch/library.h>

#include <string>
#include <vector>

#include "binding_common.h"
#include "word_engine.h"

namespace pyg_amd {
namespace {

void check_same_type(const char* op, const Tensor& rowptr, const Tensor& col, const Tensor& other, const char* other_name) {
  at::TensorArg rowptr_t{rowptr, "rowtpr", 1};  // sic: the reference's argument name
  at::TensorArg col_t{col, "col", 1};
  at::TensorArg other_t{other, other_name, 1};
  at::CheckedFrom c = op;
  at::checkAllDefined(c, {rowptr_t, col_t, other_t});
  at::checkAllSameType(c, {rowptr_t, col_t, other_t});
}

int index_code(const char* op, const Tensor& t) {
  TORCH_CHECK(t.scalar_type() == at::kInt || t.scalar_type() == at::kLong, op,
              ": int32 or int64 indices expected on the device (got ", t.scalar_type(), ")");
  return t.scalar_type() == at::kInt ? PYG_I32 : PYG_I64;
}

// ---- CUDA ----------------------------------------------------------------------------------------------------------

Tensor random_walk_cuda(const Tensor& rowptr, const Tensor& col, const Tensor& seed, int64_t walk_length, double p,
                        double q) {
  PYG_TRACE("pyg::random_walk");
  TORCH_CHECK(rowptr.is_cuda(), "'rowptr' must be a CUDA tensor");
  TORCH_CHECK(col.is_cuda(), "'col' must be a CUDA tensor");
  TORCH_CHECK(seed.is_cuda(), "'seed' must be a CUDA tensor");
  TORCH_CHECK(p == 1 && q == 1, "Uniform sampling required for now");
  check_same_type("random_walk", rowptr, col, seed, "seed");
  TORCH_CHECK(walk_length >= 0, "random_walk: 'walk_length' must be non-negative (got ", walk_length, ")");
  TORCH_CHECK(rowptr.device() == col.device() && rowptr.device() == seed.device(),
              "random_walk: 'rowptr', 'col' and 'seed' must live on the same device");
  const int code = index_code("random_walk", seed);
  DeviceGuard guard(seed.device());
  const auto rowptr_c = rowptr.contiguous(), col_c = col.contiguous(), seed_c = seed.contiguous();
  const int64_t S = seed.size(0);
  auto out = at::empty({S, walk_length + 1}, rowptr.options());
  const auto rand = at::rand({walk_length, S}, seed.options().dtype(at::kFloat));
  check_status(pyg_hip_random_walk(code, rowptr_c.data_ptr(), std::max<int64_t>(rowptr_c.numel() - 1, 0), col_c.data_ptr(),
                                   col_c.numel(), seed_c.data_ptr(), S, rand.data_ptr<float>(), walk_length, out.data_ptr(),
                                   current_stream(seed)));
  return out;
}

std::tuple<Tensor, Tensor, c10::optional<Tensor>> subgraph_cuda(const Tensor& rowptr, const Tensor& col,
                                                                const Tensor& nodes, bool return_edge_id) {
  PYG_TRACE("pyg::subgraph");
  TORCH_CHECK(rowptr.is_cuda(), "'rowptr' must be a CUDA tensor");
  TORCH_CHECK(col.is_cuda(), "'col' must be a CUDA tensor");
  TORCH_CHECK(nodes.is_cuda(), "'nodes' must be a CUDA tensor");
  check_same_type("subgraph", rowptr, col, nodes, "nodes");
  TORCH_CHECK(rowptr.device() == col.device() && rowptr.device() == nodes.device(),
              "subgraph: 'rowptr', 'col' and 'nodes' must live on the same device");
  const int code = index_code("subgraph", nodes);
  DeviceGuard guard(nodes.device());
  const auto rowptr_c = rowptr.contiguous(), col_c = col.contiguous(), nodes_c = nodes.contiguous();
  const int64_t M = nodes.size(0);
  auto out_rowptr = at::empty({M + 1}, rowptr.options());
  AllocHost ah{current_hip_stream((c10::DeviceIndex)nodes.get_device()), {}};
  pyg_hip_sampler_host host{&ah, &host_alloc, &host_free, nullptr, nullptr};
  void* out_col = nullptr;
  void* out_eid = nullptr;
  int64_t K = 0;
  const int rc = pyg_hip_subgraph(code, rowptr_c.data_ptr(), std::max<int64_t>(rowptr_c.numel() - 1, 0), col_c.data_ptr(),
                                  col_c.numel(), nodes_c.data_ptr(), M, return_edge_id ? 1 : 0, &host, out_rowptr.data_ptr(),
                                  &out_col, &out_eid, &K, static_cast<void*>(ah.stream));
  TORCH_CHECK(rc == PYG_HIP_OK, pyg_hip_last_error(), ah.error.empty() ? "" : " (", ah.error, ah.error.empty() ? "" : ")");
  Tensor col_out = adopt(out_col, {K}, col.options());
  c10::optional<Tensor> eid_out = c10::nullopt;
  if (return_edge_id) eid_out = adopt(out_eid, {K}, col.options());
  return std::make_tuple(out_rowptr, col_out, eid_out);
}

// ---- CPU -----------------------------------------------------------------------------------------------------------

Tensor random_walk_cpu(const Tensor& rowptr, const Tensor& col, const Tensor& seed, int64_t walk_length, double p,
                       double q) {
  PYG_TRACE("pyg::random_walk[cpu]");
  TORCH_CHECK(rowptr.is_cpu(), "'rowptr' must be a CPU tensor");
  TORCH_CHECK(col.is_cpu(), "'col' must be a CPU tensor");
  TORCH_CHECK(seed.is_cpu(), "'seed' must be a CPU tensor");
  TORCH_CHECK(p == 1 && q == 1, "Uniform sampling required for now");
  check_same_type("random_walk", rowptr, col, seed, "seed");
  TORCH_CHECK(walk_length >= 0, "random_walk: 'walk_length' must be non-negative (got ", walk_length, ")");
  const auto rowptr_c = rowptr.contiguous(), col_c = col.contiguous(), seed_c = seed.contiguous();
  const int64_t S = seed.size(0), stride = walk_length + 1;
  auto out = at::empty({S, stride}, rowptr.options());
  AT_DISPATCH_INTEGRAL_TYPES(seed.scalar_type(), "random_walk_cpu", [&] {
    const scalar_t* rp = rowptr_c.data_ptr<scalar_t>();
    const scalar_t* cl = col_c.data_ptr<scalar_t>();
    const scalar_t* sd = seed_c.data_ptr<scalar_t>();
    scalar_t* o = out.data_ptr<scalar_t>();
    const int64_t N = std::max<int64_t>(rowptr_c.numel() - 1, 0), E = col_c.numel();
    // walk_length = 0: the seeds, without constructing an engine (the reference divides by walk_length here,
    // random_walk_kernel.cpp:32).  S = 0: no engine either (at::parallel_for does not call its body).
    if (walk_length == 0) {
      for (int64_t i = 0; i < S; ++i) o[i] = sd[i];
      return;
    }
    if (S == 0) return;
    // one engine for all seeds in seed order: at::parallel_for's single chunk on one intra-op thread
    cpu::WordEngine eng;
    for (int64_t i = 0; i < S; ++i) {
      scalar_t v = sd[i];
      o[i * stride] = v;
      for (int64_t j = 1; j <= walk_length; ++j) {
        if (v >= 0 && (int64_t)v < N) {
          const int64_t rs = rp[v], re = rp[v + 1];
          if (re > rs && rs >= 0 && re <= E) v = cl[rs + (int64_t)eng.below((uint64_t)(re - rs))];
        }
        o[i * stride + j] = v;
      }
    }
  });
  return out;
}

std::tuple<Tensor, Tensor, c10::optional<Tensor>> subgraph_cpu(const Tensor& rowptr, const Tensor& col,
                                                               const Tensor& nodes, bool return_edge_id) {
  PYG_TRACE("pyg::subgraph[cpu]");
  TORCH_CHECK(rowptr.is_cpu(), "'rowptr' must be a CPU tensor");
  TORCH_CHECK(col.is_cpu(), "'col' must be a CPU tensor");
  TORCH_CHECK(nodes.is_cpu(), "'nodes' must be a CPU tensor");
  check_same_type("subgraph", rowptr, col, nodes, "nodes");
  const auto rowptr_c = rowptr.contiguous(), col_c = col.contiguous(), nodes_c = nodes.contiguous();
  const int64_t M = nodes.size(0);
  auto out_rowptr = at::empty({M + 1}, rowptr.options());
  Tensor out_col;
  c10::optional<Tensor> out_eid = c10::nullopt;
  AT_DISPATCH_INTEGRAL_TYPES(nodes.scalar_type(), "subgraph_cpu", [&] {
    const scalar_t* rp = rowptr_c.data_ptr<scalar_t>();
    const scalar_t* cl = col_c.data_ptr<scalar_t>();
    const scalar_t* nd = nodes_c.data_ptr<scalar_t>();
    const int64_t N = std::max<int64_t>(rowptr_c.numel() - 1, 0), E = col_c.numel();
    auto valid = [&](scalar_t v) { return v >= 0 && (int64_t)v < N; };
    // local ids in order of first occurrence (Mapper::insert)
    std::vector<int64_t> local((size_t)N, -1);
    int64_t next = 0;
    for (int64_t i = 0; i < M; ++i)
      if (valid(nd[i]) && local[(size_t)nd[i]] < 0) local[(size_t)nd[i]] = next++;
    auto row_range = [&](int64_t i, int64_t* rs, int64_t* re) {
      *rs = *re = 0;
      if (!valid(nd[i])) return;
      const int64_t a = rp[nd[i]], b = rp[nd[i] + 1];
      if (a >= 0 && b > a && b <= E) *rs = a, *re = b;
    };
    auto member = [&](scalar_t w) { return valid(w) && local[(size_t)w] >= 0; };
    scalar_t* orp = out_rowptr.data_ptr<scalar_t>();
    orp[0] = 0;
    at::parallel_for(0, M, 1024, [&](int64_t b, int64_t e) {
      for (int64_t i = b; i < e; ++i) {
        int64_t rs, re, d = 0;
        row_range(i, &rs, &re);
        for (int64_t j = rs; j < re; ++j) d += member(cl[j]);
        orp[i + 1] = (scalar_t)d;
      }
    });
    for (int64_t i = 0; i < M; ++i) orp[i + 1] = (scalar_t)(orp[i] + orp[i + 1]);
    const int64_t K = (int64_t)orp[M];
    out_col = at::empty({K}, col.options());
    if (return_edge_id) out_eid = at::empty({K}, col.options());
    scalar_t* oc = out_col.data_ptr<scalar_t>();
    scalar_t* oe = return_edge_id ? out_eid.value().data_ptr<scalar_t>() : nullptr;
    at::parallel_for(0, M, 1024, [&](int64_t b, int64_t e) {
      for (int64_t i = b; i < e; ++i) {
        int64_t rs, re, q = (int64_t)orp[i];
        row_range(i, &rs, &re);
        for (int64_t j = rs; j < re; ++j)
          if (member(cl[j])) {
            oc[q] = (scalar_t)local[(size_t)cl[j]];
            if (oe) oe[q] = (scalar_t)j;
            ++q;
          }
      }
    });
  });
  return std::make_tuple(out_rowptr, out_col, out_eid);
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(pyg, m) {
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::random_walk(Tensor rowptr, Tensor col, Tensor seed, int "
      "walk_length, float p, float q) -> Tensor"));
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::subgraph(Tensor rowptr, Tensor col, Tensor "
      "nodes, bool return_edge_id) -> (Tensor, Tensor, Tensor?)"));
}

TORCH_LIBRARY_IMPL(pyg, CUDA, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::random_walk"), TORCH_FN(random_walk_cuda));
  m.impl(TORCH_SELECTIVE_NAME("pyg::subgraph"), TORCH_FN(subgraph_cuda));
}

TORCH_LIBRARY_IMPL(pyg, CPU, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::random_walk"), TORCH_FN(random_walk_cpu));
  m.impl(TORCH_SELECTIVE_NAME("pyg::subgraph"), TORCH_FN(subgraph_cpu));
}

}  // namespace pyg_amd
