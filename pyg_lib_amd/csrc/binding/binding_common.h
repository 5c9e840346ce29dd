// Helpers shared by the binding translation units (libpyg.so).
#pragma once

#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPCachingAllocatorMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <ATen/record_function.h>
#include <dlfcn.h>

#include <optional>
#include <string>
#include <tuple>

#include "pyg_hip.h"

namespace pyg_amd {

using at::Tensor;

inline int dtype_code(at::ScalarType t) {
  switch (t) {
    case at::kFloat: return PYG_F32;
    case at::kDouble: return PYG_F64;
    case at::kHalf: return PYG_F16;
    case at::kBFloat16: return PYG_BF16;
    case at::kChar: return PYG_I8;
    case at::kByte: return PYG_U8;
    case at::kShort: return PYG_I16;
    case at::kInt: return PYG_I32;
    case at::kLong: return PYG_I64;
    default: TORCH_CHECK(false, "pyg (HIP): unsupported dtype ", t); return -1;
  }
}

// Op-level tracing: every operator entry shows up as a RECORD_FUNCTION range in the PyTorch
// profiler and as a roctx range in rocprofv3 --marker-trace, named like the schema ("pyg::segment_matmul").
// roctx is OPTIONAL: the two entry points are looked up in librocprofiler-sdk-roctx.so at first use (dlopen), so
// libpyg.so carries no link-time dependency on the profiler SDK -- a host without it just gets no roctx ranges.
struct RoctxApi {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  RoctxApi() {
    void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_LAZY | RTLD_GLOBAL);
    if (!h) h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_LAZY | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librocprofiler-sdk-roctx.so", RTLD_LAZY | RTLD_GLOBAL);
    if (h) {
      push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
      pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
      if (!push || !pop) push = nullptr, pop = nullptr;
    }
  }
};
inline const RoctxApi& roctx_api() {
  static const RoctxApi api;
  return api;
}
struct RoctxRange {
  bool on;
  explicit RoctxRange(const char* name) : on(roctx_api().push != nullptr) {
    if (on) roctx_api().push(name);
  }
  ~RoctxRange() {
    if (on) roctx_api().pop();
  }
  RoctxRange(const RoctxRange&) = delete;
  RoctxRange& operator=(const RoctxRange&) = delete;
};
#define PYG_TRACE(name)                                                \
  at::RecordFunction pyg_record_fn_(at::RecordScope::FUNCTION);          \
  if (pyg_record_fn_.isActive()) pyg_record_fn_.before(name);            \
  ::pyg_amd::RoctxRange pyg_roctx_range_(name)

inline void check_status(int rc) {
  TORCH_CHECK(rc == PYG_HIP_OK, pyg_hip_last_error());
}

// The autograd functions of the ops that take `out` return no gradient for it: a given `out` that requires grad would lose
// it without a word.  Called by the Autograd-key fronts before apply() (inside forward() grad mode is off).
inline void check_out_needs_no_grad(const char* name, const std::optional<Tensor>& out) {
  TORCH_CHECK(!(out.has_value() && out->defined() && out->requires_grad() && at::GradMode::is_enabled()), name,
              ": the gradient with respect to a given 'out' is not implemented ('out' requires grad); pass out.detach() "
              "or call under torch.no_grad()");
}

// PyTorch-ROCm types HIP devices/streams as "cuda" (masquerading), hence these spellings.
namespace alloc = c10::hip::HIPCachingAllocatorMasqueradingAsCUDA;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

inline hipStream_t current_hip_stream(c10::DeviceIndex index) {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(index).stream();
}

inline void* current_stream(const Tensor& t) {
  return static_cast<void*>(current_hip_stream((c10::DeviceIndex)t.get_device()));
}

// ---- the 64-bit key of a generator-seeded call (node2vec_walk, negative_sample) on the device ---------------------------
// splitmix64's finaliser over the generator's (seed, offset): consecutive calls advance `offset` by 4, and without the mix
// their keys -- hence their Philox streams -- would be neighbours
inline uint64_t mix_key(uint64_t seed, uint64_t offset) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (offset + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// ---- the stream-bound allocator host of a pyg_hip_sampler_host (include/pyg_hip.h) -------------------------------------
// `user` of the alloc / free callbacks: blocks come from the caching allocator on `stream`; an allocator exception is kept
// in `error` (the C-ABI cannot carry it) and the library sees a null block.
struct AllocHost {
  hipStream_t stream = nullptr;
  std::string error;
};

inline void* host_alloc(void* user, size_t bytes) {
  auto* h = static_cast<AllocHost*>(user);
  try {
    return alloc::raw_alloc_with_stream(bytes ? bytes : 16, h->stream);
  } catch (const std::exception& e) {
    h->error = e.what();
    return nullptr;
  }
}

inline void host_free(void*, void* ptr) {
  if (ptr) alloc::raw_delete(ptr);
}

// a block the library got from host_alloc and returned as a result: the tensor owns it from here on
inline Tensor adopt(void* ptr, at::IntArrayRef sizes, const at::TensorOptions& opts) {
  return at::from_blob(
      ptr, sizes, [](void* p) { alloc::raw_delete(p); }, opts);
}

// ---- heterogeneous graphs and the samplers' modes (device and CPU key) -------------------------------------------------
// pyg_lib/csrc/utils/types.h:10-12
typedef std::string node_type;
typedef std::string rel_type;
typedef std::tuple<std::string, std::string, std::string> edge_type;

inline rel_type rel_key(const edge_type& key) {
  return std::get<0>(key) + "__" + std::get<1>(key) + "__" + std::get<2>(key);
}

// precondition checks of the reference kernel, sampler/cpu/neighbor_kernel.cpp:34-36,354-380,501
inline void check_modes(bool has_node_time, bool has_edge_time, bool has_seed_time, bool has_weight, bool directed,
                        bool disjoint, const std::string& temporal_strategy) {
  TORCH_CHECK(temporal_strategy == "uniform" || temporal_strategy == "last", "No valid temporal strategy found");
  TORCH_CHECK(!has_node_time || disjoint, "Temporal sampling needs to create disjoint subgraphs");
  TORCH_CHECK(!has_edge_time || disjoint, "Temporal sampling needs to create disjoint subgraphs");
  TORCH_CHECK(!(has_node_time && has_edge_time), "Only one of node-level or edge-level sampling is supported ");
  TORCH_CHECK(!has_edge_time || has_seed_time, "Seed time needs to be specified");
  TORCH_CHECK(!(has_node_time && has_weight), "Biased node temporal sampling not yet supported");
  TORCH_CHECK(!(has_edge_time && has_weight), "Biased edge temporal sampling not yet supported");
  TORCH_CHECK(directed, "Undirected subgraphs not yet supported");
}

// `flags` of pyg_hip_segment_matmul / pyg_hip_grouped_matmul (include/pyg_hip.h) for a call made on this thread:
//  * the tile schedule is a thread-local of the binding (set through pyg_binding_set_matmul_schedule, a test /
//    measurement hook; SegmentMatmul carries the forward's value into its backward, which runs on an autograd thread);
//  * fp32 arithmetic follows torch's switch exactly as the reference does (ops/cuda/matmul_kernel.cu:158-165):
//    float32MatmulPrecision() == HIGHEST (torch's default) -> IEEE fp32 MFMAs, anything else -> the split-bf16 kernels.
int& matmul_schedule_tls();
int matmul_flags(at::ScalarType t);

}  // namespace pyg_amd
