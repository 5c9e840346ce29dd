// graclus_cluster for gfx950 (MI355X): the reference's sequential greedy matching, computed exactly in parallel rounds.
//
// Replaces pyg_lib/csrc/ops/cuda/graclus_kernel.cu.  Semantics, the round rule and why it equals the sequential visit:
// include/pyg_hip.h.  The reference's device kernel colours the nodes with a fresh bernoulli tensor every round, runs three
// launches per round, reads a flag back after every round and depends on which thread wins an unsynchronised read; none of
// that is kept.  Here:
//   * phase_a / phase_b are the two halves of a round for ONE node, shared by both routes, so the routes cannot differ;
//   * the state a phase reads of OTHER nodes is never written in that phase: phase A reads state[] (written in B only) and
//     writes m[] through an integer atomic maximum; phase B reads m[] and pick[] (written in A only) and writes state[] / out[]
//     of nodes that only their one ready owner can reach.  The only synchronisation is the boundary between the phases: a
//     workgroup barrier (single) or the end of a launch (multi);
//   * m[x] = round * 2^32 + (2^32 - 1 - rank): a newer round beats an older one, so m is never cleared, and within a round the
//     maximum is the smallest rank;
//   * the nodes still active are counted from what phase B matched (1 or 2 per ready node), never from a re-read of state[]:
//     the count, and with it the number of rounds, is a function of the input alone;
//   * out[] is written once per node, when it is matched; the kernels read the 32-bit state[] instead;
//   * a row scan is a chain of dependent loads, so phase A issues the loads of kChunk entries together, then decides in row order.
// Only comparisons of weights, no arithmetic: nothing to contract.  No float atomics.
#include "common.h"
#include "elem.h"

#include <algorithm>
#include <mutex>

namespace pyg_hip {
namespace {

constexpr int64_t kSingleNodes = 768;          // the rule: single up to here ... (measured cross-over about 850 nodes at degree 8)
constexpr int64_t kSingleEdges = 8192;         // ... and up to this many edges
constexpr int kSingleThreads = 1024;
constexpr int64_t kSingleMaxNodes = 131072;    // a forced single call above this (or above kSingleMaxEdges) runs multi
constexpr int64_t kSingleMaxEdges = 2097152;
constexpr int kMultiThreads = 256;
constexpr int kBatch = 16;                     // multi: rounds between two read-backs

enum { W_NONE = 0, W_F32 = 1, W_F64 = 2, W_F16 = 3, W_BF16 = 4 };

struct Args {
  const int64_t *rowptr, *col;
  const void* weight;
  const int64_t* perm;
  int N;
  int64_t E;
  int *state, *rank, *pick;      // [N] each: cluster id or -1 | position in perm or -1 | the round's pick or -1
  unsigned long long* m;         // [N]
  int* words;                    // multi: active nodes after round r in words[r & 1], rounds run in words[2]
  int64_t* out;
  int* pinned;                   // [0]: bad input seen, [1]: rounds of the last single call
};

template <int WT>
struct Weight {
  using type = float;
  __device__ static float load(const void* w, int64_t e) { return static_cast<const float*>(w)[e]; }
};
template <>
struct Weight<W_F64> {
  using type = double;
  __device__ static double load(const void* w, int64_t e) { return static_cast<const double*>(w)[e]; }
};
template <>
struct Weight<W_F16> {
  using type = float;
  __device__ static float load(const void* w, int64_t e) { return Math<f16_t>::up(static_cast<const f16_t*>(w)[e]); }
};
template <>
struct Weight<W_BF16> {
  using type = float;
  __device__ static float load(const void* w, int64_t e) { return Math<bf16_t>::up(static_cast<const bf16_t*>(w)[e]); }
};

// the offer of u in `round`; a node whose rank nobody wrote (perm repeats an entry) is ranked behind all others, N + u
__device__ __forceinline__ unsigned long long key_of(const Args& a, int u, uint32_t round) {
  const int r = a.rank[u];
  if (r < 0) a.pinned[0] = 1;
  const uint32_t rk = r < 0 ? (uint32_t)a.N + (uint32_t)u : (uint32_t)r;
  return ((unsigned long long)round << 32) | (uint32_t)~rk;
}

constexpr int kChunk = 4;   // row entries whose col, state, m and weight loads are issued together (a row scan is a chain of latencies)

template <int WT>
__device__ __forceinline__ void phase_a(const Args& a, int u, uint32_t round) {
  if (a.state[u] >= 0) return;
  const unsigned long long key = key_of(a, u, round);
  if (a.m[u] < key) atomicMax(a.m + u, key);
  const int64_t r0 = a.rowptr[u], r1 = a.rowptr[u + 1];
  const int64_t lo = r0 < 0 ? 0 : (r0 > a.E ? a.E : r0);
  const int64_t hi = r1 < lo ? lo : (r1 > a.E ? a.E : r1);
  bool bad = lo != r0 || hi != r1;
  int p = -1;
  typename Weight<WT>::type wmax = 0;
  for (int64_t e = lo; e < hi; e += kChunk) {
    int64_t x[kChunk];
    int st[kChunk];
    unsigned long long mx[kChunk];
    typename Weight<WT>::type w[kChunk];
#pragma unroll
    for (int k = 0; k < kChunk; ++k) x[k] = e + k < hi ? a.col[e + k] : -1;
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
      // an entry outside [0, N) forms no address and is no candidate; state 0 stands for "matched"
      const bool inside = (uint64_t)x[k] < (uint64_t)a.N;
      bad |= e + k < hi && !inside;
      st[k] = inside ? a.state[x[k]] : 0;
      mx[k] = inside ? a.m[x[k]] : ~0ull;   // (m only grows: a stale value costs an atomic that changes nothing)
      if constexpr (WT != W_NONE) w[k] = e + k < hi ? Weight<WT>::load(a.weight, e + k) : 0;
    }
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {   // in row order
      if (st[k] >= 0) continue;
      if constexpr (WT == W_NONE) {
        if (x[k] == u) continue;
        if (mx[k] < key) atomicMax(a.m + x[k], key);
        if (p < 0) p = (int)x[k];
      } else {
        if (!(w[k] >= 0)) continue;   // negative or NaN
        if (mx[k] < key) atomicMax(a.m + x[k], key);
        if (w[k] >= wmax) p = (int)x[k], wmax = w[k];
      }
    }
  }
  a.pick[u] = p;
  if (bad) a.pinned[0] = 1;
}

// returns the nodes u matched: 0 (not active, or waiting), 1 (alone) or 2
__device__ __forceinline__ int phase_b(const Args& a, int u, uint32_t round) {
  // (a neighbour may be writing state[u] right now: then m[u] is that neighbour's key and both readings return 0 here)
  if (a.state[u] >= 0) return 0;
  const unsigned long long key = key_of(a, u, round);
  if (a.m[u] != key) return 0;
  const int p = a.pick[u];
  if (p < 0 || p == u) {
    a.state[u] = u, a.out[u] = u;
    return 1;
  }
  if (a.m[p] != key) return 0;
  const int c = u < p ? u : p;
  a.state[u] = c, a.state[p] = c;
  a.out[u] = c, a.out[p] = c;
  return 2;
}

__device__ __forceinline__ void init_node(const Args& a, int u) {
  a.state[u] = -1, a.rank[u] = -1, a.m[u] = 0;
}

__device__ __forceinline__ void rank_node(const Args& a, int i) {
  const int64_t p = a.perm[i];
  if ((uint64_t)p < (uint64_t)a.N) a.rank[p] = i;
  else a.pinned[0] = 1;
}

// ---- single: one workgroup, one launch ---------------------------------------------------------------------------------
template <int WT>
__global__ __launch_bounds__(kSingleThreads) void graclus_single_kernel(const Args a) {
  __shared__ int slots[kSingleThreads / 64];
  const int tid = threadIdx.x, N = a.N;
  for (int u = tid; u < N; u += kSingleThreads) init_node(a, u);
  __syncthreads();
  for (int i = tid; i < N; i += kSingleThreads) rank_node(a, i);
  __syncthreads();
  int left = N;
  uint32_t round = 0;
  while (left > 0 && round < (uint32_t)N) {   // (at most N rounds run: the active node of the smallest rank is matched in every one)
    ++round;
    for (int u = tid; u < N; u += kSingleThreads) phase_a<WT>(a, u, round);
    __syncthreads();
    int matched = 0;
    for (int u = tid; u < N; u += kSingleThreads) matched += phase_b(a, u, round);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) matched += __shfl_xor(matched, o);
    if ((tid & 63) == 0) slots[tid >> 6] = matched;
    __syncthreads();   // (also what orders this round's state[] before the next round's phase A)
    int total = 0;
#pragma unroll
    for (int s = 0; s < kSingleThreads / 64; ++s) total += slots[s];
    left -= total;
    // slots[] is written again only behind the next round's barrier between the phases
  }
  if (tid == 0) a.pinned[1] = (int)round;
}

// ---- multi: two launches per round, one node per thread ----------------------------------------------------------------
__global__ __launch_bounds__(kMultiThreads) void graclus_init_kernel(const Args a) {
  const int64_t u = (int64_t)blockIdx.x * kMultiThreads + threadIdx.x;
  if (u == 0) a.words[0] = a.N, a.words[1] = 0, a.words[2] = 0;
  if (u < a.N) init_node(a, (int)u);
}

__global__ __launch_bounds__(kMultiThreads) void graclus_rank_kernel(const Args a) {
  const int64_t i = (int64_t)blockIdx.x * kMultiThreads + threadIdx.x;
  if (i < a.N) rank_node(a, (int)i);
}

template <int WT>
__global__ __launch_bounds__(kMultiThreads) void graclus_a_kernel(const Args a, uint32_t round) {
  const int prev = a.words[(round - 1) & 1];   // final: the launches of round - 1 have ended
  const int64_t u = (int64_t)blockIdx.x * kMultiThreads + threadIdx.x;
  if (u == 0) {
    a.words[round & 1] = prev;                 // phase B subtracts from it; zero is handed on
    if (prev > 0) a.words[2] = (int)round;
  }
  if (prev == 0) return;
  if (u < a.N) phase_a<WT>(a, (int)u, round);
}

__global__ __launch_bounds__(kMultiThreads) void graclus_b_kernel(const Args a, uint32_t round) {
  if (a.words[(round - 1) & 1] == 0) return;
  const int64_t u = (int64_t)blockIdx.x * kMultiThreads + threadIdx.x;
  const int matched = u < a.N ? phase_b(a, (int)u, round) : 0;
  const int total = __syncthreads_count(matched >= 1) + __syncthreads_count(matched == 2);
  if (threadIdx.x == 0 && total) atomicSub(a.words + (round & 1), total);
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct Last {
  const char* name = "none";
  const int* rounds_word = nullptr;   // single: the pinned word its kernel writes
  int rounds = 0, readbacks = 0;
};
thread_local Last g_last;
thread_local char g_last_text[64];

struct Plan {
  int route = PYG_HIP_GRACLUS_ROUTE_UNSUPPORTED;
  size_t o_state = 0, o_rank = 0, o_pick = 0, o_m = 0, o_words = 0, total = 0;
};

// the pure part of the dispatch: what pyg_hip_graclus_route answers and pyg_hip_graclus follows
Plan make_plan(int64_t N, int64_t E, int flags) {
  Plan p;
  if (N < 0 || E < 0 || N >= (1ll << 31)) return p;
  const int force = flags & PYG_HIP_GRACLUS_FORCE_MASK;
  int route = (N <= kSingleNodes && E <= kSingleEdges) ? PYG_HIP_GRACLUS_ROUTE_SINGLE : PYG_HIP_GRACLUS_ROUTE_MULTI;
  if (force == PYG_HIP_GRACLUS_FORCE_SINGLE)
    route = (N <= kSingleMaxNodes && E <= kSingleMaxEdges) ? PYG_HIP_GRACLUS_ROUTE_SINGLE : PYG_HIP_GRACLUS_ROUTE_MULTI;
  if (force == PYG_HIP_GRACLUS_FORCE_MULTI) route = PYG_HIP_GRACLUS_ROUTE_MULTI;
  p.route = route;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += align_up(bytes ? bytes : 1, 256);
    return o;
  };
  p.o_m = take((size_t)N * 8);
  p.o_state = take((size_t)N * 4);
  p.o_rank = take((size_t)N * 4);
  p.o_pick = take((size_t)N * 4);
  p.o_words = take(16);
  p.total = at;
  return p;
}

// the pinned words of this device (nearest's pattern; words of graclus's own): [0] bad input, [1] rounds of a single call
int deferred_slot(int** out) {
  static std::mutex mu;
  static int* slots[64] = {nullptr};
  int dev = 0;
  PYG_HIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) dev = 0;
  std::lock_guard<std::mutex> lock(mu);
  if (!slots[dev]) {
    void* ptr = nullptr;
    PYG_HIP_CHECK(hipHostMalloc(&ptr, 64, hipHostMallocDefault));
    static_cast<int*>(ptr)[0] = 0, static_cast<int*>(ptr)[1] = 0;
    slots[dev] = static_cast<int*>(ptr);
  }
  *out = slots[dev];
  return PYG_HIP_OK;
}

template <int WT>
int run_graclus(const Args& a, const Plan& p, hipStream_t stream) {
  if (p.route == PYG_HIP_GRACLUS_ROUTE_SINGLE) {
    hipLaunchKernelGGL((graclus_single_kernel<WT>), dim3(1), dim3(kSingleThreads), 0, stream, a);
    PYG_HIP_CHECK(hipGetLastError());
    g_last.name = "single", g_last.rounds_word = a.pinned + 1;
    return PYG_HIP_OK;
  }
  const dim3 grid((unsigned)(((int64_t)a.N + kMultiThreads - 1) / kMultiThreads)), block(kMultiThreads);
  hipLaunchKernelGGL(graclus_init_kernel, grid, block, 0, stream, a);
  hipLaunchKernelGGL(graclus_rank_kernel, grid, block, 0, stream, a);
  PYG_HIP_CHECK(hipGetLastError());
  void* host = nullptr;
  g_last.name = "multi";
  for (uint32_t round = 0;;) {   // at most N rounds run: the active node of the smallest rank is matched in every one
    for (int k = 0; k < kBatch; ++k) {
      ++round;
      hipLaunchKernelGGL((graclus_a_kernel<WT>), grid, block, 0, stream, a, round);
      hipLaunchKernelGGL(graclus_b_kernel, grid, block, 0, stream, a, round);
    }
    PYG_HIP_CHECK(hipGetLastError());
    if (int rc = pinned_stage().acquire(16, &host)) return rc;
    PYG_HIP_CHECK(hipMemcpyAsync(host, a.words, 16, hipMemcpyDeviceToHost, stream));
    PYG_HIP_CHECK(hipStreamSynchronize(stream));
    const int* words = static_cast<const int*>(host);
    ++g_last.readbacks;
    g_last.rounds = words[2];
    if (words[round & 1] == 0) return PYG_HIP_OK;
    if (round >= (uint32_t)a.N) return fail(PYG_HIP_ERR_RUNTIME, "graclus: %d nodes still active after %u rounds", words[round & 1], round);
  }
}

}  // namespace
}  // namespace pyg_hip

using namespace pyg_hip;

extern "C" {

int pyg_hip_graclus_route(int64_t N, int64_t E, int flags) { return make_plan(N, E, flags).route; }

const char* pyg_hip_graclus_last_route(void) {
  const int rounds = g_last.rounds_word ? *static_cast<const volatile int*>(g_last.rounds_word) : g_last.rounds;
  snprintf(g_last_text, sizeof(g_last_text), "%s r%d b%d", g_last.name, rounds, g_last.readbacks);
  return g_last_text;
}

int pyg_hip_graclus_tile(int which) {
  switch (which) {
    case PYG_HIP_GRACLUS_TILE_SINGLE_NODES: return (int)kSingleNodes;
    case PYG_HIP_GRACLUS_TILE_SINGLE_EDGES: return (int)kSingleEdges;
    case PYG_HIP_GRACLUS_TILE_SINGLE_THREADS: return kSingleThreads;
    case PYG_HIP_GRACLUS_TILE_SINGLE_MAX_NODES: return (int)kSingleMaxNodes;
    case PYG_HIP_GRACLUS_TILE_MULTI_THREADS: return kMultiThreads;
    case PYG_HIP_GRACLUS_TILE_BATCH: return kBatch;
    case PYG_HIP_GRACLUS_TILE_SINGLE_MAX_EDGES: return (int)kSingleMaxEdges;
    default: return 0;
  }
}

size_t pyg_hip_graclus_workspace_size(int64_t N, int64_t E, int flags) {
  const Plan p = make_plan(N, E, flags);
  return p.route == PYG_HIP_GRACLUS_ROUTE_UNSUPPORTED ? 0 : p.total;
}

int pyg_hip_graclus(const int64_t* rowptr, const int64_t* col, int weight_dtype, const void* weight, const int64_t* perm, int64_t N,
                    int64_t E, int flags, void* workspace, size_t workspace_bytes, int64_t* out, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PYG_HIP_REQUIRE(weight_dtype == PYG_HIP_GRACLUS_NO_WEIGHT || weight_dtype == PYG_F32 || weight_dtype == PYG_F64 ||
                      weight_dtype == PYG_F16 || weight_dtype == PYG_BF16,
                  "graclus: weight must be float32, float64, float16 or bfloat16 (dtype code %d)", weight_dtype);
  PYG_HIP_REQUIRE(N >= 0 && E >= 0, "graclus: negative size");
  if (N >= (1ll << 31)) return fail(PYG_HIP_ERR_UNSUPPORTED, "graclus: 2^31 or more nodes: node ids are 32-bit here");
  PYG_HIP_REQUIRE(rowptr != nullptr, "graclus: NULL rowptr");
  PYG_HIP_REQUIRE(col != nullptr || E == 0, "graclus: NULL col");
  PYG_HIP_REQUIRE((weight != nullptr) == (weight_dtype != PYG_HIP_GRACLUS_NO_WEIGHT) || E == 0,
                  "graclus: weight and weight_dtype must be given together");
  PYG_HIP_REQUIRE((perm != nullptr && out != nullptr) || N == 0, "graclus: NULL perm or out");
  const Plan p = make_plan(N, E, flags);
  PYG_HIP_REQUIRE(workspace != nullptr, "graclus: NULL workspace");
  if (workspace_bytes < p.total)
    return fail(PYG_HIP_ERR_WORKSPACE, "graclus: workspace of %zu bytes, %zu needed (pyg_hip_graclus_workspace_size)", workspace_bytes,
                p.total);
  PYG_HIP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "graclus: the workspace must be 16-byte aligned");
  int* slot = nullptr;
  if (int rc = deferred_slot(&slot)) return rc;
  if (*static_cast<volatile int*>(slot) != 0) {
    *static_cast<volatile int*>(slot) = 0;
    return fail(PYG_HIP_ERR_INVALID, "graclus: an earlier call on this device had a col entry outside [0, N), a row range outside "
                                     "[0, E] or a perm that is no permutation of 0 .. N-1 (its result is unspecified)");
  }
  g_last = Last();
  if (N == 0) return PYG_HIP_OK;
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  // a weight array without edges is never read: the kernels without weights serve it
  const int wt = (weight == nullptr || E == 0) ? W_NONE
                 : weight_dtype == PYG_F32     ? W_F32
                 : weight_dtype == PYG_F64     ? W_F64
                 : weight_dtype == PYG_F16     ? W_F16
                                               : W_BF16;
  const Args a{rowptr, col, weight, perm, (int)N, E, reinterpret_cast<int*>(ws + p.o_state), reinterpret_cast<int*>(ws + p.o_rank),
               reinterpret_cast<int*>(ws + p.o_pick), reinterpret_cast<unsigned long long*>(ws + p.o_m),
               reinterpret_cast<int*>(ws + p.o_words), out, slot};
  switch (wt) {
    case W_NONE: return run_graclus<W_NONE>(a, p, stream);
    case W_F32: return run_graclus<W_F32>(a, p, stream);
    case W_F64: return run_graclus<W_F64>(a, p, stream);
    case W_F16: return run_graclus<W_F16>(a, p, stream);
    default: return run_graclus<W_BF16>(a, p, stream);
  }
}

int pyg_hip_graclus_pending_error(void) {
  int* slot = nullptr;
  if (deferred_slot(&slot) != PYG_HIP_OK) return PYG_HIP_ERR_RUNTIME;
  const int pending = *static_cast<volatile int*>(slot);
  *static_cast<volatile int*>(slot) = 0;
  return pending;
}

}  // extern "C"
