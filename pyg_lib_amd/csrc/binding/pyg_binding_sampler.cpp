// torch::Library binding of the device samplers: pyg::neighbor_sample, pyg::hetero_neighbor_sample and
// pyg::dist_neighbor_sample (schemas byte-identical to pyg_lib/csrc/sampler/neighbor.cpp:129-147) and, this build only,
// pyg::neighbor_sample_batched, pyg::hetero_neighbor_sample_batched and pyg::sampler_release_table_cache.
// Kernels: csrc/hip/sampler.hip through the C-ABI.  PyTorch is plumbing: argument checks, result blocks from the caching
// allocator on the call's stream (AllocHost, binding_common.h), the CPU generator's mt19937 for the random words.
//   neighbor_sample / hetero_neighbor_sample / dist_neighbor_sample continue the process's default CPU generator on the
//     caller's current stream (run_sampler);
//   the *_batched operators start one seeded engine per batch on private lanes (run_sampler_batched).
// The two homogeneous operators share homo_relation / seed_set, the two heterogeneous ones HeteroArgs; every call's
// host-side result block is a SampleResult.
#include <ATen/ATen.h>
#include <ATen/CPUGeneratorImpl.h>
#include <torch/library.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "binding_common.h"

namespace pyg_amd {

// rand_engine.h:79-91.  at::randint(lo, hi, {n}) is empty({n}).random_(lo, hi), and random_ walks
// the CPU generator's mt19937 serially, so filling num_blocks*128 words in one call yields exactly
// the words of that many consecutive 128-word prefetches.
static void host_rng_blocks(void* user, int64_t* words, int64_t num_blocks, int /*first*/) {
  auto* h = static_cast<AllocHost*>(user);
  try {
    auto buf = at::from_blob(words, {num_blocks * 128}, at::TensorOptions().dtype(at::kLong));
    buf.random_(std::numeric_limits<int64_t>::min(), std::numeric_limits<int64_t>::max());
  } catch (const std::exception& e) {
    h->error = e.what();
  }
}

// The C-ABI's view of an at::mt19937 (pyg_hip_sampler_host::mt19937); returns the engine's data so that a caller that
// installs the advanced state afterwards (EngineLoan) need not read it out twice.
static at::mt19937_data_pod export_engine(const at::mt19937& engine, pyg_hip_mt19937& mt) {
  at::mt19937_data_pod pod = engine.data();
  static_assert(sizeof(mt.state) == sizeof(uint32_t) * at::MERSENNE_STATE_N, "mt19937 state size");
  std::memcpy(mt.state, pod.state_.data(), sizeof(mt.state));
  mt.left = pod.left_;
  mt.next = pod.next_;
  return pod;
}

// Lends the default CPU generator's mt19937 engine to the library for the duration of one call and
// installs the advanced state afterwards (see pyg_hip_sampler_host::mt19937).
struct EngineLoan {
  at::CPUGeneratorImpl* gen;
  at::mt19937 engine;
  at::mt19937_data_pod pod;
  pyg_hip_mt19937 mt;
  bool ok;
  // The generator's mutex is held only while the engine state is copied out and while it is installed again --
  // not across the call: the library may fall back to the host callback (host_rng_blocks -> Tensor.random_(), which
  // takes the same non-recursive mutex), and other threads' CPU RNG use must not wait for device synchronisations.
  // Like the reference (random/cpu/rand_engine.h draws without any lock), concurrent sampler calls are the
  // caller's to serialise.
  EngineLoan()
      : gen(at::get_generator_or_default<at::CPUGeneratorImpl>(c10::nullopt, at::detail::getDefaultCPUGenerator())) {
    {
      std::lock_guard<std::mutex> lock(gen->mutex_);
      engine = gen->engine();
    }
    pod = export_engine(engine, mt);
    ok = engine.is_valid();
  }
  pyg_hip_mt19937* ptr() { return ok ? &mt : nullptr; }
  void commit() {
    if (!ok) return;
    std::memcpy(pod.state_.data(), mt.state, sizeof(mt.state));
    pod.left_ = mt.left;
    pod.next_ = mt.next;
    engine.set_data(pod);
    std::lock_guard<std::mutex> lock(gen->mutex_);
    gen->set_engine(engine);
  }
};

// The reference dispatches the sampler on the seeds' integral type (neighbor_kernel.cpp:893,930) and returns
// that type.  The kernels read an int32 CSR (rowptr / col, the large arrays) IN PLACE (`graph` below +
// pyg_hip_relation::index_is32); only the seeds are widened for the call (batch-sized) and the results are
// narrowed back -- same values, same generator stream (dist_neighbor_sample included).
struct IndexArgs {
  at::ScalarType dtype = at::kLong;
  std::vector<Tensor> keep;  // widened copies stay alive until the call returns
  const int64_t* ptr(const Tensor& t, const char* what) {
    TORCH_CHECK(t.is_contiguous(), "Non-contiguous '", what, "'");
    TORCH_CHECK(t.is_cuda(), "pyg (HIP): '", what, "' must live on a HIP device");
    TORCH_CHECK(t.scalar_type() == dtype, "pyg (HIP): '", what, "' must have the seeds' dtype (", dtype, ")");
    if (dtype == at::kLong) return t.data_ptr<int64_t>();
    keep.push_back(t.to(at::kLong));
    return keep.back().data_ptr<int64_t>();
  }
  // rowptr / col of the sampled graph: raw pointer of either width, no copy
  const int64_t* graph(const Tensor& t, const char* what) const {
    TORCH_CHECK(t.is_contiguous(), "Non-contiguous '", what, "'");
    TORCH_CHECK(t.is_cuda(), "pyg (HIP): '", what, "' must live on a HIP device");
    TORCH_CHECK(t.scalar_type() == dtype, "pyg (HIP): '", what, "' must have the seeds' dtype (", dtype, ")");
    return static_cast<const int64_t*>(t.data_ptr());
  }
  int32_t is32() const { return dtype == at::kInt ? 1 : 0; }
  Tensor narrow(const Tensor& t) const { return dtype == at::kLong ? t : t.to(dtype); }
};

static at::ScalarType index_dtype(const Tensor& seed) {
  TORCH_CHECK(seed.scalar_type() == at::kLong || seed.scalar_type() == at::kInt,
              "pyg (HIP): indices must be int64 or int32");
  return seed.scalar_type();
}

struct SampleOutput {
  std::vector<Tensor> node_id, row, col, edge_id;
  std::vector<std::vector<int64_t>> nodes_per_hop, edges_per_hop;
};

// The host side of one pyg_hip_sample_result: the arrays the library fills, and the way from the device blocks it
// hands out to tensors that own them.
struct SampleResult {
  std::vector<int64_t*> node_id, row, col, eid;
  std::vector<int64_t> num_nodes, num_edges, nph, eph;
  pyg_hip_sample_result res;
  int T = 0, E = 0, L = 0;
  void init(int num_node_types, int num_relations, int num_hops) {
    T = num_node_types, E = num_relations, L = num_hops;
    node_id.assign((size_t)T, nullptr);
    row.assign((size_t)std::max(E, 1), nullptr);
    col.assign((size_t)std::max(E, 1), nullptr);
    eid.assign((size_t)std::max(E, 1), nullptr);
    num_nodes.assign((size_t)T, 0);
    num_edges.assign((size_t)std::max(E, 1), 0);
    nph.assign((size_t)T * (L + 1), 0);
    eph.assign((size_t)std::max(E * L, 1), 0);
    res.node_id = node_id.data();
    res.num_nodes = num_nodes.data();
    res.nodes_per_hop_host = nph.data();
    res.row = row.data();
    res.col = col.data();
    res.edge_id = eid.data();
    res.num_edges = num_edges.data();
    res.edges_per_hop_host = eph.data();
    res.rng_blocks = 0;
  }
  // Only after the call (the batch) reported PYG_HIP_OK: a failed one hands nothing out, so nothing is adopted.
  SampleOutput adopt_blocks(bool disjoint, bool return_edge_id, const at::TensorOptions& opts) const {
    SampleOutput out;
    for (int t = 0; t < T; ++t) {
      if (!node_id[(size_t)t]) continue;
      const int64_t n = num_nodes[(size_t)t];
      out.node_id.push_back(disjoint ? adopt(node_id[(size_t)t], {n, 2}, opts) : adopt(node_id[(size_t)t], {n}, opts));
      out.nodes_per_hop.emplace_back(nph.begin() + (size_t)t * (L + 1), nph.begin() + (size_t)(t + 1) * (L + 1));
    }
    for (int e = 0; e < E; ++e) {
      const int64_t n = num_edges[(size_t)e];
      out.row.push_back(adopt(row[(size_t)e], {n}, opts));
      out.col.push_back(adopt(col[(size_t)e], {n}, opts));
      if (return_edge_id) out.edge_id.push_back(adopt(eid[(size_t)e], {n}, opts));
      out.edges_per_hop.emplace_back(eph.begin() + (size_t)e * L, eph.begin() + (size_t)(e + 1) * L);
    }
    return out;
  }
};

// PYG_HIP_OP_TIMING=1: host time of the sampler operators' parts on stderr (arguments -> library call -> results adopted ->
// Dict results built), microseconds since the operator was entered.  The operator that carries the marks
// (hetero_neighbor_sample) holds one OpTiming; run_sampler adds its marks through g_op_timing, which points at that
// object for exactly its lifetime -- also when a check throws.
struct OpTiming;
static thread_local OpTiming* g_op_timing = nullptr;
struct OpTiming {
  static bool on() {
    static const bool v = [] { const char* e = getenv("PYG_HIP_OP_TIMING"); return e && atoi(e) != 0; }();
    return v;
  }
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  std::string line;
  OpTiming() { g_op_timing = on() ? this : nullptr; }
  OpTiming(const OpTiming&) = delete;
  OpTiming& operator=(const OpTiming&) = delete;
  void mark(const char* what) {
    if (!on()) return;
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    char buf[64];
    snprintf(buf, sizeof(buf), " %s=%.1f", what, us);
    line += buf;
  }
  ~OpTiming() {
    g_op_timing = nullptr;
    if (on() && !line.empty()) fprintf(stderr, "[pyg op timing] us:%s\n", line.c_str());
  }
};

static SampleOutput run_sampler(const std::vector<pyg_hip_relation>& rels,
                                const std::vector<pyg_hip_seed_set>& seeds,
                                const std::vector<const int64_t*>& node_time, bool temporal_last,
                                int num_node_types, int L, bool csc, bool replace, bool disjoint,
                                bool return_edge_id, const at::Device& device) {
  DeviceGuard guard(device);
  const auto opts = at::TensorOptions().dtype(at::kLong).device(device);
  AllocHost host;
  host.stream = current_hip_stream(device.index());
  // Fast path for the random words: the CPU generator's mt19937 engine is continued on the device
  // (the generator ends up exactly where the reference's at::randint / random_ calls would leave it).
  EngineLoan loan;
  pyg_hip_sampler_host cb{&host, &host_alloc, &host_free, &host_rng_blocks, loan.ptr()};
  const int T = num_node_types, E = (int)rels.size();
  SampleResult r;
  r.init(T, E, L);
  const int rc = pyg_hip_hetero_neighbor_sample(T, E, rels.data(), (int)seeds.size(), seeds.data(),
                                                node_time.empty() ? nullptr : node_time.data(),
                                                temporal_last, L, csc, replace, disjoint, return_edge_id,
                                                &cb, &r.res, host.stream);
  if (g_op_timing) g_op_timing->mark("library_done");
  if (rc == PYG_HIP_OK) loan.commit();
  TORCH_CHECK(host.error.empty(), host.error);
  check_status(rc);
  SampleOutput out = r.adopt_blocks(disjoint, return_edge_id, opts);
  if (g_op_timing) g_op_timing->mark("adopted");
  return out;
}

// ---- K independent batches at once (pyg_hip_hetero_neighbor_sample_batched) ----------------------------------------
// Private streams of the batched sampler, per device: batch b runs on lane b % lanes.  Blocks the lanes allocate go back to
// the caching allocator's pools of THESE streams when the caller drops the outputs; every batched call first orders its
// lanes behind the caller's current stream (the C-ABI call does), so a block is never reused under a consumer the caller
// queued before the call.
static std::vector<hipStream_t> batch_lanes(int device, int want) {
  static std::mutex mu;
  static std::vector<std::vector<hipStream_t>> per_device(64);
  std::lock_guard<std::mutex> lock(mu);
  auto& v = per_device[(size_t)(device < 0 || device >= 64 ? 0 : device)];
  while ((int)v.size() < want) {
    hipStream_t st = nullptr;
    TORCH_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess, "pyg (HIP): hipStreamCreate failed");
    v.push_back(st);
  }
  return std::vector<hipStream_t>(v.begin(), v.begin() + want);
}

// Lanes = batches in flight.  PYG_HIP_SAMPLER_LANES, default 8 -- 2 for heterogeneous graphs: a hetero batch's launches carry
// several relations each and already fill most of the chip, more than two of them in flight only slow one another down
// (C5 graph, K = 8: 2 lanes 1.13 x the single-batch loop, 8 lanes 0.86 x; the C3 graph gives 1.07 - 1.09 x from 2 lanes up:
// profiles/NOTES_r6.md section 2g)
static int batch_lane_count(size_t K, bool hetero) {
  static const int cap = [] {
    const char* e = getenv("PYG_HIP_SAMPLER_LANES");
    const int v = e ? atoi(e) : 0;
    return v < 1 ? 0 : (v > 16 ? 16 : v);
  }();
  const int c = cap ? cap : (hetero ? 2 : 8);
  return (int)std::min<size_t>(K, (size_t)c);
}

// Batch b continues the mt19937 stream torch.manual_seed(generator_seeds[b]) would start (CPUGeneratorImpl::set_current_seed
// installs at::mt19937(seed)); the process's default generator is not touched.
static std::vector<SampleOutput> run_sampler_batched(const std::vector<pyg_hip_relation>& rels,
                                                     const std::vector<std::vector<pyg_hip_seed_set>>& seeds,
                                                     const std::vector<int64_t>& generator_seeds,
                                                     const std::vector<const int64_t*>& node_time, bool temporal_last,
                                                     int num_node_types, int L, bool csc, bool replace, bool disjoint,
                                                     bool return_edge_id, const at::Device& device) {
  const size_t K = seeds.size();
  TORCH_CHECK(generator_seeds.size() == K, "neighbor_sample_batched: one generator seed per batch expected (", K, " batches, ",
              generator_seeds.size(), " seeds)");
  DeviceGuard guard(device);
  const auto opts = at::TensorOptions().dtype(at::kLong).device(device);
  const int T = num_node_types, E = (int)rels.size();
  const auto lanes = batch_lanes(device.index(), batch_lane_count(K, rels.size() > 1));
  struct PerBatch {
    AllocHost host;
    pyg_hip_mt19937 mt;
    pyg_hip_sampler_host cb;
    SampleResult result;
  };
  std::vector<PerBatch> pb(K);
  std::vector<pyg_hip_sample_batch> batches(K);
  for (size_t b = 0; b < K; ++b) {
    PerBatch& p = pb[b];
    p.host.stream = lanes[b % lanes.size()];
    export_engine(at::mt19937((uint64_t)generator_seeds[b]), p.mt);
    p.cb = pyg_hip_sampler_host{&p.host, &host_alloc, &host_free, &host_rng_blocks, &p.mt};
    p.result.init(T, E, L);
    batches[b].num_seed_sets = (int)seeds[b].size();
    batches[b].seeds_host = seeds[b].data();
    batches[b].host = &p.cb;
    batches[b].result = &p.result.res;
    batches[b].stream = p.host.stream;
  }
  const int rc = pyg_hip_hetero_neighbor_sample_batched(T, E, rels.data(), node_time.empty() ? nullptr : node_time.data(),
                                                        temporal_last, L, csc, replace, disjoint, return_edge_id, (int)K,
                                                        batches.data(), current_hip_stream(device.index()));
  // every block a successful batch was handed gets an owner before any error is raised: also when another batch failed,
  // the blocks must go back to the allocator
  std::vector<SampleOutput> outs(K);
  for (size_t b = 0; b < K; ++b)
    if (batches[b].status == PYG_HIP_OK) outs[b] = pb[b].result.adopt_blocks(disjoint, return_edge_id, opts);
  for (size_t b = 0; b < K; ++b) TORCH_CHECK(pb[b].host.error.empty(), pb[b].host.error);
  check_status(rc);
  return outs;
}

// biased sampling: per-edge weights of one relation (neighbor_kernel.cpp:52 narrows them per row)
static void set_weight(pyg_hip_relation& rel, const Tensor& w, int64_t num_cols) {
  TORCH_CHECK(w.is_cuda(), "pyg (HIP): 'edge_weight' must live on a HIP device");
  TORCH_CHECK(w.is_contiguous(), "Non-contiguous 'edge_weight'");
  TORCH_CHECK(w.dim() == 1 && w.numel() == num_cols, "pyg (HIP): 'edge_weight' needs one entry per edge");
  TORCH_CHECK(w.scalar_type() == at::kFloat || w.scalar_type() == at::kDouble,
              "pyg (HIP): 'edge_weight' must be float32 or float64");
  rel.edge_weight = w.data_ptr();
  rel.edge_weight_dtype = w.scalar_type() == at::kDouble ? PYG_F64 : PYG_F32;
}

static const int64_t* time_ptr(const Tensor& t, const char* what) {
  TORCH_CHECK(t.is_contiguous(), "Non-contiguous '", what, "'");
  TORCH_CHECK(t.is_cuda(), "pyg (HIP): '", what, "' must live on a HIP device");
  TORCH_CHECK(t.scalar_type() == at::kLong, "pyg (HIP): '", what, "' must be int64");  // temporal_t, :393-394
  return t.data_ptr<int64_t>();
}

// ---- homogeneous graphs: pyg::neighbor_sample, pyg::neighbor_sample_batched -------------------------------------------
// the graph as the library's one relation between node type 0 and itself
static pyg_hip_relation homo_relation(const IndexArgs& ix, const Tensor& rowptr, const Tensor& col,
                                      const std::vector<int64_t>& num_neighbors, const c10::optional<Tensor>& edge_time,
                                      const c10::optional<Tensor>& edge_weight) {
  pyg_hip_relation rel{};
  rel.rowptr = ix.graph(rowptr, "rowptr");
  rel.num_rows = rowptr.numel() - 1;
  rel.col = ix.graph(col, "col");
  rel.num_cols = col.numel();
  rel.src_type = 0;
  rel.dst_type = 0;
  rel.num_neighbors_host = num_neighbors.data();
  rel.edge_time = edge_time.has_value() ? time_ptr(edge_time.value(), "edge_time") : nullptr;
  rel.index_is32 = ix.is32();
  if (edge_weight.has_value()) set_weight(rel, edge_weight.value(), col.numel());
  return rel;
}

// the seeds of one node type (both graph kinds); `seed_time` may be null
static pyg_hip_seed_set seed_set(IndexArgs& ix, int node_type_index, const Tensor& seed, const Tensor* seed_time) {
  pyg_hip_seed_set s;
  s.node_type = node_type_index;
  s.reserved = 0;
  s.seed = ix.ptr(seed, "seed");
  s.num_seed = seed.numel();
  s.seed_time = seed_time ? time_ptr(*seed_time, "seed_time") : nullptr;
  return s;
}

std::tuple<Tensor, Tensor, Tensor, c10::optional<Tensor>, std::vector<int64_t>, std::vector<int64_t>>
neighbor_sample_kernel(const Tensor& rowptr, const Tensor& col, const Tensor& seed,
                       const std::vector<int64_t>& num_neighbors, const c10::optional<Tensor>& node_time,
                       const c10::optional<Tensor>& edge_time, const c10::optional<Tensor>& seed_time,
                       const c10::optional<Tensor>& edge_weight, bool csc, bool replace, bool directed,
                       bool disjoint, std::string temporal_strategy, bool return_edge_id) {
  PYG_TRACE("pyg::neighbor_sample");
  check_modes(node_time.has_value(), edge_time.has_value(), seed_time.has_value(), edge_weight.has_value(),
              directed, disjoint, temporal_strategy);
  IndexArgs ix;
  ix.dtype = index_dtype(seed);
  const std::vector<pyg_hip_relation> rels{homo_relation(ix, rowptr, col, num_neighbors, edge_time, edge_weight)};
  const std::vector<pyg_hip_seed_set> seeds{seed_set(ix, 0, seed, seed_time.has_value() ? &seed_time.value() : nullptr)};
  std::vector<const int64_t*> ntime;
  if (node_time.has_value()) ntime.push_back(time_ptr(node_time.value(), "node_time"));
  auto out = run_sampler(rels, seeds, ntime, temporal_strategy == "last", 1, (int)num_neighbors.size(), csc,
                         replace, disjoint, return_edge_id, rowptr.device());
  c10::optional<Tensor> eid = c10::nullopt;
  if (return_edge_id) eid = ix.narrow(out.edge_id[0]);
  return std::make_tuple(ix.narrow(out.row[0]), ix.narrow(out.col[0]), ix.narrow(out.node_id[0]), eid,
                         out.nodes_per_hop[0], out.edges_per_hop[0]);
}

// This build only: K mini-batches of pyg::neighbor_sample in one call.  Batch b = neighbor_sample(rowptr, col, seeds[b], ...)
// under torch.manual_seed(generator_seeds[b]) -- bit for bit -- but the batches overlap on the device.  Returns the
// per-batch row / col / node_id / edge_id lists and the per-hop counts as [K, L + 1] / [K, L] CPU tensors.
std::tuple<std::vector<Tensor>, std::vector<Tensor>, std::vector<Tensor>, std::vector<Tensor>, Tensor, Tensor>
neighbor_sample_batched_kernel(const Tensor& rowptr, const Tensor& col, const std::vector<Tensor>& seeds,
                               const std::vector<int64_t>& num_neighbors, const std::vector<int64_t>& generator_seeds,
                               const c10::optional<Tensor>& node_time, const c10::optional<Tensor>& edge_time,
                               const c10::optional<std::vector<Tensor>>& seed_times, const c10::optional<Tensor>& edge_weight,
                               bool csc, bool replace, bool directed, bool disjoint, std::string temporal_strategy,
                               bool return_edge_id) {
  PYG_TRACE("pyg::neighbor_sample_batched");
  check_modes(node_time.has_value(), edge_time.has_value(), seed_times.has_value(), edge_weight.has_value(), directed,
              disjoint, temporal_strategy);
  const size_t K = seeds.size();
  TORCH_CHECK(!seed_times.has_value() || seed_times.value().size() == K, "neighbor_sample_batched: one seed_time per batch");
  const int64_t L = (int64_t)num_neighbors.size();
  const auto cpu_long = at::TensorOptions().dtype(at::kLong);
  if (K == 0)
    return std::make_tuple(std::vector<Tensor>(), std::vector<Tensor>(), std::vector<Tensor>(), std::vector<Tensor>(),
                           at::zeros({0, L + 1}, cpu_long), at::zeros({0, L}, cpu_long));
  IndexArgs ix;
  ix.dtype = index_dtype(seeds[0]);
  const std::vector<pyg_hip_relation> rels{homo_relation(ix, rowptr, col, num_neighbors, edge_time, edge_weight)};
  std::vector<std::vector<pyg_hip_seed_set>> sets(K);
  for (size_t b = 0; b < K; ++b)
    sets[b].push_back(seed_set(ix, 0, seeds[b], seed_times.has_value() ? &seed_times.value()[b] : nullptr));
  std::vector<const int64_t*> ntime;
  if (node_time.has_value()) ntime.push_back(time_ptr(node_time.value(), "node_time"));
  auto outs = run_sampler_batched(rels, sets, generator_seeds, ntime, temporal_strategy == "last", 1, (int)L, csc, replace,
                                  disjoint, return_edge_id, rowptr.device());
  std::vector<Tensor> row, colv, node, eid;
  Tensor nph = at::zeros({(int64_t)K, L + 1}, cpu_long), eph = at::zeros({(int64_t)K, L}, cpu_long);
  for (size_t b = 0; b < K; ++b) {
    row.push_back(ix.narrow(outs[b].row[0]));
    colv.push_back(ix.narrow(outs[b].col[0]));
    node.push_back(ix.narrow(outs[b].node_id[0]));
    if (return_edge_id) eid.push_back(ix.narrow(outs[b].edge_id[0]));
    std::memcpy(nph.data_ptr<int64_t>() + b * (size_t)(L + 1), outs[b].nodes_per_hop[0].data(), sizeof(int64_t) * (size_t)(L + 1));
    if (L > 0) std::memcpy(eph.data_ptr<int64_t>() + b * (size_t)L, outs[b].edges_per_hop[0].data(), sizeof(int64_t) * (size_t)L);
  }
  return std::make_tuple(row, colv, node, eid, nph, eph);
}

// ---- heterogeneous graphs: pyg::hetero_neighbor_sample, pyg::hetero_neighbor_sample_batched --------------------------
// The two operators take the same graph dictionaries; this is the one walk over them.  `op` prefixes the messages.
struct HeteroArgs {
  const char* op;
  const std::vector<node_type>& node_types;
  std::unordered_map<std::string, int> nt_index;
  IndexArgs ix;
  std::vector<rel_type> rel_names;  // rel_key(edge_types[e])
  std::vector<pyg_hip_relation> rels;
  std::vector<std::vector<int64_t>> fanouts;  // rels[e].num_neighbors_host points into these
  size_t L = 0;
  c10::optional<at::Device> device;  // of the first relation's rowptr; none for a graph without edge types

  // `first_seed` decides the index type (neighbor_kernel.cpp:930)
  HeteroArgs(const char* op_name, const std::vector<node_type>& node_type_names, const std::vector<edge_type>& edge_types,
             const Tensor& first_seed, const c10::Dict<rel_type, Tensor>& rowptr_dict,
             const c10::Dict<rel_type, Tensor>& col_dict, const c10::Dict<rel_type, std::vector<int64_t>>& num_neighbors_dict,
             const c10::optional<c10::Dict<rel_type, Tensor>>& edge_time_dict,
             const c10::optional<c10::Dict<rel_type, Tensor>>& edge_weight_dict)
      : op(op_name), node_types(node_type_names), rel_names(edge_types.size()), rels(edge_types.size()),
        fanouts(edge_types.size()) {
    for (size_t i = 0; i < node_types.size(); ++i) nt_index[node_types[i]] = (int)i;
    ix.dtype = index_dtype(first_seed);
    for (size_t e = 0; e < edge_types.size(); ++e) {
      const auto& k = edge_types[e];
      rel_names[e] = rel_key(k);
      const auto& rel = rel_names[e];
      const Tensor& rowptr = rowptr_dict.at(rel);
      const Tensor& col = col_dict.at(rel);
      if (!device.has_value()) device = rowptr.device();
      fanouts[e] = num_neighbors_dict.at(rel);
      L = std::max(L, fanouts[e].size());
      TORCH_CHECK(nt_index.count(std::get<0>(k)) && nt_index.count(std::get<2>(k)), op,
                  ": edge type names an unknown node type");
      rels[e].rowptr = ix.graph(rowptr, "rowptr");
      rels[e].num_rows = rowptr.numel() - 1;
      rels[e].col = ix.graph(col, "col");
      rels[e].num_cols = col.numel();
      rels[e].src_type = nt_index[std::get<0>(k)];
      rels[e].dst_type = nt_index[std::get<2>(k)];
      rels[e].index_is32 = ix.is32();
      if (edge_time_dict.has_value() && edge_time_dict.value().contains(rel))
        rels[e].edge_time = time_ptr(edge_time_dict.value().at(rel), "edge_time");
      if (edge_weight_dict.has_value() && edge_weight_dict.value().contains(rel))
        set_weight(rels[e], edge_weight_dict.value().at(rel), col.numel());
    }
    for (size_t e = 0; e < edge_types.size(); ++e) {
      TORCH_CHECK(fanouts[e].size() == L, op, ": all relations must list ", L, " hops");
      rels[e].num_neighbors_host = fanouts[e].data();
    }
  }
  HeteroArgs(const HeteroArgs&) = delete;
  HeteroArgs& operator=(const HeteroArgs&) = delete;

  // One batch's seed sets; `seed_time_dict` may be null.  `device_from_seeds` is a difference in behaviour between the two
  // operators: hetero_neighbor_sample takes the device from the seeds when no relation gave one, the batched operator has
  // required one from the relations by then.
  std::vector<pyg_hip_seed_set> seed_sets(const c10::Dict<node_type, Tensor>& seed_dict,
                                          const c10::Dict<node_type, Tensor>* seed_time_dict, bool device_from_seeds) {
    std::vector<pyg_hip_seed_set> sets;
    for (const auto& kv : seed_dict) {  // c10::Dict iterates in insertion order, as the reference relies on
      const Tensor& seed = kv.value();
      if (device_from_seeds && !device.has_value()) device = seed.device();
      TORCH_CHECK(nt_index.count(kv.key()), op, ": seed type '", kv.key(), "' is not a node type");
      sets.push_back(seed_set(ix, nt_index[kv.key()], seed, nullptr));
      if (seed_time_dict) sets.back().seed_time = time_ptr(seed_time_dict->at(kv.key()), "seed_time");
    }
    return sets;
  }

  // node_time per node type (null where the dictionary has none); empty without a dictionary
  std::vector<const int64_t*> node_time(const c10::optional<c10::Dict<node_type, Tensor>>& node_time_dict) {
    std::vector<const int64_t*> ntime;
    if (node_time_dict.has_value()) {
      ntime.assign(node_types.size(), nullptr);
      for (const auto& kv : node_time_dict.value()) {
        TORCH_CHECK(nt_index.count(kv.key()), op, ": time given for unknown node type '", kv.key(), "'");
        ntime[(size_t)nt_index[kv.key()]] = time_ptr(kv.value(), "node_time");
      }
    }
    return ntime;
  }

  // The result dictionaries of one SampleOutput.  `edge_id` is set iff return_edge_id: hetero_neighbor_sample returns the
  // optional as it is, the batched operator an empty dictionary in its place.
  struct Dicts {
    c10::Dict<rel_type, Tensor> row, col;
    c10::Dict<node_type, Tensor> node;
    c10::optional<c10::Dict<rel_type, Tensor>> edge_id;
    c10::Dict<node_type, std::vector<int64_t>> nodes_per_hop;
    c10::Dict<rel_type, std::vector<int64_t>> edges_per_hop;
  };
  Dicts dicts(const SampleOutput& out, bool return_edge_id) const {
    Dicts d;
    if (return_edge_id) d.edge_id = c10::Dict<rel_type, Tensor>();
    for (size_t t = 0; t < node_types.size(); ++t) {
      d.node.insert(node_types[t], ix.narrow(out.node_id[t]));
      d.nodes_per_hop.insert(node_types[t], out.nodes_per_hop[t]);
    }
    for (size_t e = 0; e < rel_names.size(); ++e) {
      const auto& rel = rel_names[e];
      d.row.insert(rel, ix.narrow(out.row[e]));
      d.col.insert(rel, ix.narrow(out.col[e]));
      d.edges_per_hop.insert(rel, out.edges_per_hop[e]);
      if (return_edge_id) d.edge_id.value().insert(rel, ix.narrow(out.edge_id[e]));
    }
    return d;
  }
};

// This build only: K mini-batches of pyg::hetero_neighbor_sample (uniform sampling; no temporal / biased options here).
std::tuple<std::vector<c10::Dict<rel_type, Tensor>>, std::vector<c10::Dict<rel_type, Tensor>>,
           std::vector<c10::Dict<node_type, Tensor>>, std::vector<c10::Dict<rel_type, Tensor>>,
           std::vector<c10::Dict<node_type, std::vector<int64_t>>>, std::vector<c10::Dict<rel_type, std::vector<int64_t>>>>
hetero_neighbor_sample_batched_kernel(const std::vector<node_type>& node_types, const std::vector<edge_type>& edge_types,
                                      const c10::Dict<rel_type, Tensor>& rowptr_dict, const c10::Dict<rel_type, Tensor>& col_dict,
                                      const std::vector<c10::Dict<node_type, Tensor>>& seed_dicts,
                                      const c10::Dict<rel_type, std::vector<int64_t>>& num_neighbors_dict,
                                      const std::vector<int64_t>& generator_seeds,
                                      const c10::optional<c10::Dict<node_type, Tensor>>& node_time_dict,
                                      const c10::optional<c10::Dict<rel_type, Tensor>>& edge_time_dict,
                                      const c10::optional<std::vector<c10::Dict<node_type, Tensor>>>& seed_time_dicts,
                                      const c10::optional<c10::Dict<rel_type, Tensor>>& edge_weight_dict, bool csc, bool replace,
                                      bool directed, bool disjoint, std::string temporal_strategy, bool return_edge_id) {
  PYG_TRACE("pyg::hetero_neighbor_sample_batched");
  // the modes of pyg::hetero_neighbor_sample (sampler/neighbor.cpp:137-147 is one entry for all of them)
  check_modes(node_time_dict.has_value(), edge_time_dict.has_value(), seed_time_dicts.has_value(), edge_weight_dict.has_value(),
              directed, disjoint, temporal_strategy);
  TORCH_CHECK(!seed_time_dicts.has_value() || seed_time_dicts.value().size() == seed_dicts.size(),
              "hetero_neighbor_sample_batched: one seed_time dict per batch");
  const size_t K = seed_dicts.size();
  TORCH_CHECK(K > 0 && seed_dicts[0].size() > 0, "hetero_neighbor_sample_batched: no seeds given");
  HeteroArgs args("hetero_neighbor_sample_batched", node_types, edge_types, seed_dicts[0].begin()->value(), rowptr_dict,
                  col_dict, num_neighbors_dict, edge_time_dict, edge_weight_dict);
  TORCH_CHECK(args.device.has_value(), "hetero_neighbor_sample_batched: no tensors given");
  std::vector<std::vector<pyg_hip_seed_set>> sets(K);
  for (size_t b = 0; b < K; ++b)
    sets[b] = args.seed_sets(seed_dicts[b], seed_time_dicts.has_value() ? &seed_time_dicts.value()[b] : nullptr,
                             /*device_from_seeds=*/false);
  const auto ntime = args.node_time(node_time_dict);
  auto outs = run_sampler_batched(args.rels, sets, generator_seeds, ntime, temporal_strategy == "last", (int)node_types.size(),
                                  (int)args.L, csc, replace, disjoint, return_edge_id, args.device.value());
  std::vector<c10::Dict<rel_type, Tensor>> o_row, o_col, o_eid;
  std::vector<c10::Dict<node_type, Tensor>> o_node;
  std::vector<c10::Dict<node_type, std::vector<int64_t>>> o_nph;
  std::vector<c10::Dict<rel_type, std::vector<int64_t>>> o_eph;
  for (size_t b = 0; b < K; ++b) {
    auto d = args.dicts(outs[b], return_edge_id);
    o_row.push_back(d.row), o_col.push_back(d.col), o_node.push_back(d.node);
    o_eid.push_back(d.edge_id.has_value() ? d.edge_id.value() : c10::Dict<rel_type, Tensor>());
    o_nph.push_back(d.nodes_per_hop), o_eph.push_back(d.edges_per_hop);
  }
  return std::make_tuple(o_row, o_col, o_node, o_eid, o_nph, o_eph);
}

// pyg_binding_cpu.cpp
std::tuple<c10::Dict<std::string, Tensor>, c10::Dict<std::string, Tensor>, c10::Dict<std::string, Tensor>,
           c10::optional<c10::Dict<std::string, Tensor>>, c10::Dict<std::string, std::vector<int64_t>>,
           c10::Dict<std::string, std::vector<int64_t>>>
hetero_neighbor_sample_on_cpu(const std::vector<std::string>& node_types,
                              const std::vector<std::tuple<std::string, std::string, std::string>>& edge_types,
                              const c10::Dict<std::string, Tensor>& rowptr_dict, const c10::Dict<std::string, Tensor>& col_dict,
                              const c10::Dict<std::string, Tensor>& seed_dict,
                              const c10::Dict<std::string, std::vector<int64_t>>& num_neighbors_dict,
                              const c10::optional<c10::Dict<std::string, Tensor>>& node_time_dict,
                              const c10::optional<c10::Dict<std::string, Tensor>>& edge_time_dict,
                              const c10::optional<c10::Dict<std::string, Tensor>>& seed_time_dict,
                              const c10::optional<c10::Dict<std::string, Tensor>>& edge_weight_dict, bool csc, bool replace,
                              bool directed, bool disjoint, std::string temporal_strategy, bool return_edge_id);

std::tuple<c10::Dict<rel_type, Tensor>, c10::Dict<rel_type, Tensor>, c10::Dict<node_type, Tensor>,
           c10::optional<c10::Dict<rel_type, Tensor>>, c10::Dict<node_type, std::vector<int64_t>>,
           c10::Dict<rel_type, std::vector<int64_t>>>
hetero_neighbor_sample_kernel(const std::vector<node_type>& node_types, const std::vector<edge_type>& edge_types,
                              const c10::Dict<rel_type, Tensor>& rowptr_dict,
                              const c10::Dict<rel_type, Tensor>& col_dict,
                              const c10::Dict<node_type, Tensor>& seed_dict,
                              const c10::Dict<rel_type, std::vector<int64_t>>& num_neighbors_dict,
                              const c10::optional<c10::Dict<node_type, Tensor>>& node_time_dict,
                              const c10::optional<c10::Dict<rel_type, Tensor>>& edge_time_dict,
                              const c10::optional<c10::Dict<node_type, Tensor>>& seed_time_dict,
                              const c10::optional<c10::Dict<rel_type, Tensor>>& edge_weight_dict, bool csc,
                              bool replace, bool directed, bool disjoint, std::string temporal_strategy,
                              bool return_edge_id) {
  // BackendSelect: tensors inside Dicts cannot drive dispatch (sampler/cpu/neighbor_kernel.cpp:985-991) -- a graph
  // held in CPU tensors goes to the CPU kernel, a device graph to the HIP sampler
  {
    bool on_device = false;
    for (const auto& kv : rowptr_dict) on_device = on_device || kv.value().is_cuda();
    for (const auto& kv : seed_dict) on_device = on_device || kv.value().is_cuda();
    if (!on_device)
      return hetero_neighbor_sample_on_cpu(node_types, edge_types, rowptr_dict, col_dict, seed_dict, num_neighbors_dict,
                                           node_time_dict, edge_time_dict, seed_time_dict, edge_weight_dict, csc, replace,
                                           directed, disjoint, temporal_strategy, return_edge_id);
  }
  PYG_TRACE("pyg::hetero_neighbor_sample");
  OpTiming timing;  // the only sampler operator that carries the marks
  check_modes(node_time_dict.has_value(), edge_time_dict.has_value(), seed_time_dict.has_value(),
              edge_weight_dict.has_value(), directed, disjoint, temporal_strategy);
  TORCH_CHECK(seed_dict.size() > 0, "hetero_neighbor_sample: no seeds given");
  HeteroArgs args("hetero_neighbor_sample", node_types, edge_types, seed_dict.begin()->value(), rowptr_dict, col_dict,
                  num_neighbors_dict, edge_time_dict, edge_weight_dict);
  const auto seeds = args.seed_sets(seed_dict, seed_time_dict.has_value() ? &seed_time_dict.value() : nullptr,
                                    /*device_from_seeds=*/true);
  const auto ntime = args.node_time(node_time_dict);
  TORCH_CHECK(args.device.has_value(), "hetero_neighbor_sample: no tensors given");
  timing.mark("args_ready");
  auto out = run_sampler(args.rels, seeds, ntime, temporal_strategy == "last", (int)node_types.size(), (int)args.L, csc,
                         replace, disjoint, return_edge_id, args.device.value());
  auto d = args.dicts(out, return_edge_id);
  timing.mark("dicts_built");
  return std::make_tuple(d.row, d.col, d.node, d.edge_id, d.nodes_per_hop, d.edges_per_hop);
}

// This build only: frees the idle node tables the library keeps between sampler calls (current device) through the caching
// allocator they came from; returns the number still lent to running calls.
int64_t sampler_release_table_cache_kernel() {
  AllocHost host;
  host.stream = nullptr;
  pyg_hip_sampler_host cb{&host, &host_alloc, &host_free, &host_rng_blocks, nullptr};
  const int rc = pyg_hip_sampler_table_cache_release(&cb);
  TORCH_CHECK(rc >= 0, pyg_hip_last_error());
  return rc;
}

// pyg::dist_neighbor_sample (sampler/cpu/neighbor_kernel.cpp:957-978)
std::tuple<Tensor, Tensor, std::vector<int64_t>> dist_neighbor_sample_kernel(
    const Tensor& rowptr, const Tensor& col, const Tensor& seed, const int64_t num_neighbors,
    const c10::optional<Tensor>& node_time, const c10::optional<Tensor>& edge_time,
    const c10::optional<Tensor>& seed_time, const c10::optional<Tensor>& edge_weight, bool csc, bool replace,
    bool directed, bool disjoint, std::string temporal_strategy) {
  PYG_TRACE("pyg::dist_neighbor_sample");
  check_modes(node_time.has_value(), edge_time.has_value(), seed_time.has_value(), edge_weight.has_value(), directed,
              disjoint, temporal_strategy);
  // dispatched on the seeds' integral type like the other samplers (neighbor_kernel.cpp:893,930): an int32 CSR is read in
  // place, only the seeds are widened for the call and the results narrowed back
  IndexArgs ix;
  ix.dtype = index_dtype(seed);
  const int64_t* rowptr_p = ix.graph(rowptr, "rowptr");
  const int64_t* col_p = ix.graph(col, "col");
  const int64_t* seed_p = ix.ptr(seed, "seed");
  DeviceGuard guard(rowptr.device());
  const auto opts = at::TensorOptions().dtype(at::kLong).device(rowptr.device());
  AllocHost host;
  host.stream = current_hip_stream(rowptr.device().index());
  EngineLoan loan;
  pyg_hip_sampler_host cb{&host, &host_alloc, &host_free, &host_rng_blocks, loan.ptr()};
  const int64_t S = seed.numel();
  std::vector<int64_t> cumsum((size_t)S + 1, 0);
  int64_t* node_ptr = nullptr;
  int64_t* edge_ptr = nullptr;
  int64_t E = 0;
  pyg_hip_relation wrel{};  // only carries the weights (set_weight checks them)
  if (edge_weight.has_value()) set_weight(wrel, edge_weight.value(), col.numel());
  const int rc = pyg_hip_dist_neighbor_sample(
      rowptr_p, col_p, seed_p, S, num_neighbors,
      node_time.has_value() ? time_ptr(node_time.value(), "node_time") : nullptr,
      edge_time.has_value() ? time_ptr(edge_time.value(), "edge_time") : nullptr,
      seed_time.has_value() ? time_ptr(seed_time.value(), "seed_time") : nullptr, wrel.edge_weight,
      wrel.edge_weight_dtype, temporal_strategy == "last", replace, disjoint, ix.is32(), &cb, &node_ptr, &edge_ptr, &E,
      cumsum.data(), host.stream);
  if (rc == PYG_HIP_OK) loan.commit();
  TORCH_CHECK(host.error.empty(), host.error);
  check_status(rc);
  auto nodes = disjoint ? adopt(node_ptr, {S + E, 2}, opts) : adopt(node_ptr, {S + E}, opts);
  auto edges = adopt(edge_ptr, {E}, opts);
  return std::make_tuple(ix.narrow(nodes), ix.narrow(edges), cumsum);
}

// ---------------------------------------------------------------------------------------------
// registration
// ---------------------------------------------------------------------------------------------
TORCH_LIBRARY_FRAGMENT(pyg, m) {
  // pyg_lib/csrc/sampler/neighbor.cpp:129-147
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::neighbor_sample(Tensor rowptr, Tensor col, Tensor seed, int[] "
      "num_neighbors, Tensor? node_time = None, Tensor? edge_time = None, "
      "Tensor? seed_time = None, Tensor? edge_weight = None, bool csc = False, "
      "bool replace = False, bool directed = True, bool disjoint = False, "
      "str temporal_strategy = 'uniform', bool return_edge_id = True) -> "
      "(Tensor, Tensor, Tensor, Tensor?, int[], int[])"));
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::hetero_neighbor_sample(str[] node_types, (str, str, str)[] "
      "edge_types, Dict(str, Tensor) rowptr_dict, Dict(str, Tensor) col_dict, "
      "Dict(str, Tensor) seed_dict, Dict(str, int[]) num_neighbors_dict, "
      "Dict(str, Tensor)? node_time_dict = None, Dict(str, Tensor)? "
      "edge_time_dict = None, Dict(str, Tensor)? seed_time_dict = None, "
      "Dict(str, Tensor)? edge_weight_dict = None, bool csc = False, "
      "bool replace = False, bool directed = True, bool disjoint = False, "
      "str temporal_strategy = 'uniform', bool return_edge_id = True) -> "
      "(Dict(str, Tensor), Dict(str, Tensor), Dict(str, Tensor), "
      "Dict(str, Tensor)?, Dict(str, int[]), Dict(str, int[]))"));
  m.def("sampler_release_table_cache() -> int", &sampler_release_table_cache_kernel);
  // this build only: K independent mini-batches in one call, overlapped on the device (pyg_hip_hetero_neighbor_sample_batched)
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::neighbor_sample_batched(Tensor rowptr, Tensor col, Tensor[] seeds, int[] num_neighbors, int[] generator_seeds, "
      "Tensor? node_time = None, Tensor? edge_time = None, Tensor[]? seed_times = None, Tensor? edge_weight = None, "
      "bool csc = False, bool replace = False, bool directed = True, bool disjoint = False, "
      "str temporal_strategy = 'uniform', bool return_edge_id = True) -> "
      "(Tensor[], Tensor[], Tensor[], Tensor[], Tensor, Tensor)"));
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::hetero_neighbor_sample_batched(str[] node_types, (str, str, str)[] edge_types, Dict(str, Tensor) rowptr_dict, "
      "Dict(str, Tensor) col_dict, Dict(str, Tensor)[] seed_dicts, Dict(str, int[]) num_neighbors_dict, "
      "int[] generator_seeds, Dict(str, Tensor)? node_time_dict = None, Dict(str, Tensor)? edge_time_dict = None, "
      "Dict(str, Tensor)[]? seed_time_dicts = None, Dict(str, Tensor)? edge_weight_dict = None, bool csc = False, "
      "bool replace = False, bool directed = True, bool disjoint = False, str temporal_strategy = 'uniform', "
      "bool return_edge_id = True) -> "
      "(Dict(str, Tensor)[], Dict(str, Tensor)[], Dict(str, Tensor)[], Dict(str, Tensor)[], Dict(str, int[])[], "
      "Dict(str, int[])[])"));
  m.def(TORCH_SELECTIVE_SCHEMA(
      "pyg::dist_neighbor_sample(Tensor rowptr, Tensor col, Tensor seed, int "
      "num_neighbors, Tensor? node_time = None, Tensor? edge_time = None, "
      "Tensor? seed_time = None, Tensor? edge_weight = None, bool csc = False, "
      "bool replace = False, bool directed = True, bool disjoint = False, "
      "str temporal_strategy = 'uniform') -> (Tensor, Tensor, int[])"));
}

// HIP tensors dispatch under the CUDA key on PyTorch-ROCm.
TORCH_LIBRARY_IMPL(pyg, CUDA, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::neighbor_sample"), TORCH_FN(neighbor_sample_kernel));
  m.impl(TORCH_SELECTIVE_NAME("pyg::neighbor_sample_batched"), TORCH_FN(neighbor_sample_batched_kernel));
  m.impl(TORCH_SELECTIVE_NAME("pyg::dist_neighbor_sample"), TORCH_FN(dist_neighbor_sample_kernel));
}

// Tensors inside Dicts cannot drive dispatch (sampler/cpu/neighbor_kernel.cpp:985-991): the
// kernel checks the device itself and refuses CPU graphs.
TORCH_LIBRARY_IMPL(pyg, BackendSelect, m) {
  m.impl(TORCH_SELECTIVE_NAME("pyg::hetero_neighbor_sample"), TORCH_FN(hetero_neighbor_sample_kernel));
  m.impl(TORCH_SELECTIVE_NAME("pyg::hetero_neighbor_sample_batched"), TORCH_FN(hetero_neighbor_sample_batched_kernel));
}

}  // namespace pyg_amd
