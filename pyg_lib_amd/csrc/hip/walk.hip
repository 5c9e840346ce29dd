// pyg::random_walk and pyg::subgraph on the device (include/pyg_hip.h: pyg_hip_random_walk, pyg_hip_subgraph).
//
// random_walk (reference: sampler/cuda/random_walk_kernel.cu): every step of a walk is two dependent random reads
// (the rowptr pair, then col), ~900 cycles each when they miss to HBM.  A lane carries W walks at once and issues the W
// walks' loads back to back, so W rowptr pairs and then W col entries are in flight together; the uniform of the next
// step is loaded one step ahead.  W grows with the number of walks per resident lane (1 for a Node2Vec batch, 8 for a
// DeepWalk sweep over every node).  Output rows are written in place ([S, L + 1], row-major), either straight from
// registers or -- STAGE -- through an LDS image of the block's whole tile, which is one contiguous range of the output
// and leaves in 16-byte stores, wherever that image fits in 64 KiB (PYG_HIP_WALK_STAGE=0: always registers; DESIGN.md
// "random_walk and subgraph" has the A/B).
//
// subgraph (reference: sampler/cpu/subgraph_kernel.cpp with mapper.h; the reference has no device kernel):
//   1. table[v] = min position of v in `nodes` (atomicMin), then one scan over `nodes` of (first occurrence?, degree):
//      the first occurrence writes its rank among the distinct nodes into table[v] (tagged with kRank so that the
//      scan's own re-reads of the table cannot mistake a rank for a position), and every row gets the offset of its
//      candidate edges in the concatenation of all selected rows (cand_off) and its first CSR position (start).
//   2. Candidate edges are dealt to a fixed number of workgroups in equal ranges (hub rows need no special path); each
//      chunk of 1024 candidates finds its rows by binary search in cand_off.  Pass A counts kept edges per workgroup,
//      the counts go through scan.h, the one host synchronisation reads the total, and pass B recomputes membership and
//      writes with ballot / popcount offsets.  No per-candidate array is ever allocated.
//   3. out_rowptr[i] is written by the thread that holds row i's first candidate; rows without candidates take the
//      value of the next row that has some (or the total) in a last small kernel.
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "scan.h"

namespace pyg_hip {
namespace {

// ---- random_walk ---------------------------------------------------------------------------------------------------
constexpr int kWalkThreads = 256;
constexpr int kWalkStageBytes = 64 * 1024;  // LDS image of a block's tile (STAGE); larger tiles take plain stores

template <typename idx_t, int W, bool STAGE>
__global__ __launch_bounds__(kWalkThreads) void random_walk_kernel(const idx_t* __restrict__ rowptr,
                                                                   const idx_t* __restrict__ col,
                                                                   const idx_t* __restrict__ seed,
                                                                   const float* __restrict__ rnd, idx_t* __restrict__ out,
                                                                   int64_t num_nodes, int64_t num_edges, int64_t S,
                                                                   int64_t L) {
  extern __shared__ __align__(16) char walk_lds[];
  idx_t* tile = reinterpret_cast<idx_t*>(walk_lds);
  const int64_t w0 = (int64_t)blockIdx.x * (kWalkThreads * W);  // the block's walks: [w0, w0 + kWalkThreads * W)
  const int64_t stride = L + 1;
  int64_t i[W];
  bool act[W];
  idx_t v[W];
  float u[W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
    i[k] = w0 + k * kWalkThreads + threadIdx.x;
    act[k] = i[k] < S;
    v[k] = act[k] ? seed[i[k]] : idx_t(0);
    u[k] = act[k] && L > 0 ? rnd[i[k]] : 0.f;
  }
  auto put = [&](int k, int64_t j, idx_t x) {
    if (STAGE)
      tile[(int64_t)(k * kWalkThreads + threadIdx.x) * stride + j] = x;
    else if (act[k])
      out[i[k] * stride + j] = x;
  };
#pragma unroll
  for (int k = 0; k < W; ++k) put(k, 0, v[k]);
  for (int64_t j = 0; j < L; ++j) {
    idx_t rs[W], re[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      rs[k] = 0;
      re[k] = 0;
      // a node outside [0, num_nodes) is treated as isolated: the walk stays on it
      if (act[k] && v[k] >= 0 && (int64_t)v[k] < num_nodes) {
        rs[k] = rowptr[v[k]];
        re[k] = rowptr[v[k] + 1];
      }
    }
    float un[W];
#pragma unroll
    for (int k = 0; k < W; ++k) un[k] = act[k] && j + 1 < L ? rnd[(j + 1) * S + i[k]] : 0.f;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const idx_t deg = re[k] - rs[k];
      if (deg > 0 && rs[k] >= 0 && (int64_t)re[k] <= num_edges) {
        // the reference's arithmetic: float(uniform) * float(deg), truncated; the clamp only acts where float(deg)
        // rounds up (deg > 2^24), where the reference would read past the row
        idx_t o = (idx_t)(u[k] * (float)deg);
        if (o > deg - 1) o = deg - 1;
        v[k] = col[rs[k] + o];
      }
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
      put(k, j + 1, v[k]);
      u[k] = un[k];
    }
  }
  if (STAGE) {
    __syncthreads();
    const int64_t nw = S - w0 < kWalkThreads * W ? S - w0 : kWalkThreads * W;
    const int64_t bytes = nw * stride * (int64_t)sizeof(idx_t);
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4* src = reinterpret_cast<const u32x4*>(walk_lds);
    u32x4* dst = reinterpret_cast<u32x4*>(out + w0 * stride);  // 16-byte aligned: checked on the host
    for (int64_t q = threadIdx.x; q < bytes / 16; q += kWalkThreads) dst[q] = src[q];
    const int64_t tail0 = bytes / 16 * 16 / (int64_t)sizeof(idx_t), n = nw * stride;
    for (int64_t q = tail0 + threadIdx.x; q < n; q += kWalkThreads) out[w0 * stride + q] = tile[q];
  }
}

template <typename idx_t, int W>
int launch_walk(bool stage, const void* rowptr, int64_t N, const void* col, int64_t E, const void* seed, int64_t S,
                const float* rnd, int64_t L, void* out, hipStream_t stream) {
  const int64_t blocks = (S + kWalkThreads * W - 1) / (kWalkThreads * W);
  PYG_HIP_REQUIRE(blocks < (1ll << 31), "random_walk: too many seeds (%lld)", (long long)S);
  const size_t lds = stage ? (size_t)kWalkThreads * W * (size_t)(L + 1) * sizeof(idx_t) : 0;
  if (stage)
    hipLaunchKernelGGL((random_walk_kernel<idx_t, W, true>), dim3((unsigned)blocks), dim3(kWalkThreads), lds, stream,
                       (const idx_t*)rowptr, (const idx_t*)col, (const idx_t*)seed, rnd, (idx_t*)out, N, E, S, L);
  else
    hipLaunchKernelGGL((random_walk_kernel<idx_t, W, false>), dim3((unsigned)blocks), dim3(kWalkThreads), 0, stream,
                       (const idx_t*)rowptr, (const idx_t*)col, (const idx_t*)seed, rnd, (idx_t*)out, N, E, S, L);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

template <typename idx_t>
int random_walk_t(const void* rowptr, int64_t N, const void* col, int64_t E, const void* seed, int64_t S,
                  const float* rnd, int64_t L, void* out, hipStream_t stream) {
  // walks per lane: as many as the seeds give while every lane a CU can keep resident (16 waves) still has work
  const int64_t lanes = (int64_t)device_info().num_cus * 1024;
  int W = 1;
  while (W < 8 && S >= lanes * W * 2) W *= 2;
  const char* e = getenv("PYG_HIP_WALK_STAGE");
  const bool stage = !(e && e[0] == '0') && (size_t)kWalkThreads * W * (size_t)(L + 1) * sizeof(idx_t) <= kWalkStageBytes &&
                     (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  switch (W) {
    case 1: return launch_walk<idx_t, 1>(stage, rowptr, N, col, E, seed, S, rnd, L, out, stream);
    case 2: return launch_walk<idx_t, 2>(stage, rowptr, N, col, E, seed, S, rnd, L, out, stream);
    case 4: return launch_walk<idx_t, 4>(stage, rowptr, N, col, E, seed, S, rnd, L, out, stream);
    default: return launch_walk<idx_t, 8>(stage, rowptr, N, col, E, seed, S, rnd, L, out, stream);
  }
}

// ---- subgraph ------------------------------------------------------------------------------------------------------
constexpr uint32_t kNone = 0xFFFFFFFFu;  // table entry of a node that is not selected
constexpr uint32_t kRank = 0x80000000u;  // tag of a rank (positions, the other content, stay below 2^31 - 1)
constexpr int kSgThreads = 256;
constexpr int kSgItems = 4;
constexpr int kSgChunk = kSgThreads * kSgItems;

template <typename idx_t>
__global__ __launch_bounds__(256) void subgraph_first_kernel(const idx_t* __restrict__ nodes, int64_t M, int64_t N,
                                                             uint32_t* __restrict__ table) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (int64_t)gridDim.x * blockDim.x) {
    const idx_t v = nodes[i];
    if (v >= 0 && (int64_t)v < N) atomicMin(&table[v], (uint32_t)i);
  }
}

struct Pair {
  int64_t first;  // 1 at the first occurrence of a node
  int64_t deg;    // candidate edges of the row
};
struct PairSum {
  __host__ __device__ Pair operator()(Pair a, Pair b) const { return Pair{a.first + b.first, a.deg + b.deg}; }
  __host__ __device__ static Pair identity() { return Pair{0, 0}; }
};

template <typename idx_t>
struct RowLoad {
  const idx_t* nodes;
  const idx_t* rowptr;
  const uint32_t* table;
  int64_t N, E;
  __device__ Pair operator()(int64_t i) const {
    const idx_t v = nodes[i];
    if (v < 0 || (int64_t)v >= N) return Pair{0, 0};  // not a node: an empty row, no local id
    const int64_t rs = rowptr[v], re = rowptr[v + 1];
    return Pair{table[v] == (uint32_t)i ? 1 : 0, rs >= 0 && re > rs && re <= E ? re - rs : 0};
  }
};

template <typename idx_t>
struct RowStore {
  const idx_t* nodes;
  const idx_t* rowptr;
  uint32_t* table;
  int64_t* cand_off;  // M + 1
  int64_t* start;     // M
  int64_t M;
  __device__ void operator()(int64_t i, Pair run, Pair v) const {
    cand_off[i] = run.deg;
    if (i == M - 1) cand_off[M] = run.deg + v.deg;
    if (v.deg > 0) start[i] = rowptr[nodes[i]];
    if (v.first) table[nodes[i]] = kRank | (uint32_t)run.first;
  }
};

// last row r in [lo, hi] with cand_off[r] <= e (cand_off[lo] <= e)
__device__ __forceinline__ int64_t row_of(const int64_t* __restrict__ cand_off, int64_t lo, int64_t hi, int64_t e) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (cand_off[mid] <= e)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// WRITE = false: part[b] = kept edges of workgroup b's candidate range.  WRITE = true: part[b] = their exclusive prefix;
// the kept edges are written in candidate order, and out_rowptr for every row whose first candidate lies in the range.
template <typename idx_t, bool WRITE>
__global__ __launch_bounds__(kSgThreads) void subgraph_edges_kernel(const idx_t* __restrict__ col,
                                                                    const uint32_t* __restrict__ table,
                                                                    const int64_t* __restrict__ cand_off,
                                                                    const int64_t* __restrict__ start, int64_t M,
                                                                    int64_t N, int64_t* __restrict__ part,
                                                                    idx_t* __restrict__ out_rowptr,
                                                                    idx_t* __restrict__ out_col,
                                                                    idx_t* __restrict__ out_eid) {
  __shared__ int64_t s_row[2];
  __shared__ int s_cnt[kSgItems * (kSgThreads / 64)];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long lt_mask = (1ull << lane) - 1;
  const int64_t C = cand_off[M];
  const int64_t lo = C * (int64_t)blockIdx.x / gridDim.x, hi = C * ((int64_t)blockIdx.x + 1) / gridDim.x;
  int64_t base = WRITE ? part[blockIdx.x] : 0;
  for (int64_t c0 = lo; c0 < hi; c0 += kSgChunk) {
    const int64_t c1 = hi - c0 < kSgChunk ? hi : c0 + kSgChunk;
    if (threadIdx.x < 2) s_row[threadIdx.x] = row_of(cand_off, 0, M - 1, threadIdx.x ? c1 - 1 : c0);
    __syncthreads();
    const int64_t r0 = s_row[0], r1 = s_row[1];
    int64_t e[kSgItems], r[kSgItems], pos[kSgItems];
#pragma unroll
    for (int k = 0; k < kSgItems; ++k) {
      e[k] = c0 + k * kSgThreads + threadIdx.x;
      r[k] = e[k] < c1 ? row_of(cand_off, r0, r1, e[k]) : r0;
      pos[k] = start[r[k]] + (e[k] - cand_off[r[k]]);
    }
    idx_t w[kSgItems];
#pragma unroll
    for (int k = 0; k < kSgItems; ++k) w[k] = e[k] < c1 ? col[pos[k]] : idx_t(-1);
    uint32_t t[kSgItems];
#pragma unroll
    for (int k = 0; k < kSgItems; ++k) t[k] = w[k] >= 0 && (int64_t)w[k] < N ? table[w[k]] : kNone;
    unsigned long long m[kSgItems];
#pragma unroll
    for (int k = 0; k < kSgItems; ++k) {
      m[k] = __ballot(t[k] != kNone);
      if (lane == 0) s_cnt[k * (kSgThreads / 64) + wave] = (int)__popcll(m[k]);
    }
    __syncthreads();
    int64_t total = 0;
#pragma unroll
    for (int q = 0; q < kSgItems * (kSgThreads / 64); ++q) total += s_cnt[q];
    if (WRITE) {
#pragma unroll
      for (int k = 0; k < kSgItems; ++k) {
        int64_t pre = base + (int64_t)__popcll(m[k] & lt_mask);
        for (int q = 0; q < k * (kSgThreads / 64) + wave; ++q) pre += s_cnt[q];
        if (t[k] != kNone) {
          out_col[pre] = (idx_t)(t[k] & ~kRank);
          if (out_eid) out_eid[pre] = (idx_t)pos[k];
        }
        if (e[k] < c1 && e[k] == cand_off[r[k]]) out_rowptr[r[k]] = (idx_t)pre;
      }
    }
    base += total;
    __syncthreads();  // s_row / s_cnt are reused by the next chunk
  }
  if (!WRITE && threadIdx.x == 0) part[blockIdx.x] = base;
}

// rows without candidate edges: out_rowptr of the next row that has some (written by pass B), or the total
template <typename idx_t>
__global__ __launch_bounds__(256) void subgraph_rowptr_kernel(const int64_t* __restrict__ cand_off, int64_t M,
                                                              const int64_t* __restrict__ total,
                                                              idx_t* __restrict__ out_rowptr) {
  const int64_t C = cand_off[M];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= M; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < M && cand_off[i + 1] > cand_off[i]) continue;
    const int64_t x = cand_off[i];
    out_rowptr[i] = x == C ? (idx_t)*total : out_rowptr[row_of(cand_off, i, M - 1, x)];
  }
}

struct ScanLoadI64 {
  const int64_t* p;
  __device__ int64_t operator()(int64_t i) const { return p[i]; }
};
struct ScanStoreI64 {
  int64_t* p;
  __device__ void operator()(int64_t i, int64_t run, int64_t) const { p[i] = run; }
};

template <typename idx_t>
int subgraph_t(const void* rowptr_, int64_t N, const void* col_, int64_t E, const void* nodes_, int64_t M,
               int return_edge_id, const pyg_hip_sampler_host* host, void* out_rowptr_, void** out_col,
               void** out_edge_id, int64_t* num_out, hipStream_t stream) {
  const idx_t* rowptr = (const idx_t*)rowptr_;
  const idx_t* col = (const idx_t*)col_;
  const idx_t* nodes = (const idx_t*)nodes_;
  idx_t* out_rowptr = (idx_t*)out_rowptr_;
  const DeviceInfo& di = device_info();
  const int64_t P = std::min<int64_t>(2048, (int64_t)di.num_cus * 4);
  const int64_t row_tiles = (M + kScanTile - 1) / kScanTile;
  const int64_t part_tiles = (P + kScanTile - 1) / kScanTile;
  // workspace: table [N] u32 | cand_off [M + 1] | start [M] | part counts [P] | part offsets [P] | row-scan tiles + total
  // | part-scan tiles | kept total
  size_t off = 0;
  auto carve = [&](size_t bytes) {
    const size_t at = off;
    off = align_up(off + bytes, 256);
    return at;
  };
  const size_t o_table = carve((size_t)N * 4), o_cand = carve((size_t)(M + 1) * 8), o_start = carve((size_t)M * 8),
               o_cnt = carve((size_t)P * 8), o_poff = carve((size_t)P * 8),
               o_rtiles = carve((size_t)(row_tiles + 1) * sizeof(Pair)), o_ptiles = carve((size_t)(part_tiles + 1) * 8),
               o_total = carve(8);
  char* ws = static_cast<char*>(host->alloc(host->user, off));
  PYG_HIP_REQUIRE(ws != nullptr, "subgraph: workspace allocation of %zu bytes failed", off);
  struct Release {
    const pyg_hip_sampler_host* h;
    void* p;
    ~Release() { h->free(h->user, p); }
  } release{host, ws};
  uint32_t* table = (uint32_t*)(ws + o_table);
  int64_t* cand_off = (int64_t*)(ws + o_cand);
  int64_t* start = (int64_t*)(ws + o_start);
  int64_t* cnt = (int64_t*)(ws + o_cnt);
  int64_t* poff = (int64_t*)(ws + o_poff);
  Pair* rtiles = (Pair*)(ws + o_rtiles);
  int64_t* ptiles = (int64_t*)(ws + o_ptiles);
  int64_t* total = (int64_t*)(ws + o_total);

  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((M + 255) / 256, (int64_t)di.num_cus * 16));
  if (N > 0) PYG_HIP_CHECK(hipMemsetAsync(table, 0xFF, (size_t)N * 4, stream));
  hipLaunchKernelGGL((subgraph_first_kernel<idx_t>), dim3(grid), dim3(256), 0, stream, nodes, M, N, table);
  PYG_HIP_CHECK(hipGetLastError());
  int rc = device_scan<Pair, PairSum>(RowLoad<idx_t>{nodes, rowptr, table, N, E},
                                      RowStore<idx_t>{nodes, rowptr, table, cand_off, start, M}, M, rtiles,
                                      rtiles + row_tiles, stream);
  if (rc != PYG_HIP_OK) return rc;
  hipLaunchKernelGGL((subgraph_edges_kernel<idx_t, false>), dim3((unsigned)P), dim3(kSgThreads), 0, stream, col, table,
                     cand_off, start, M, N, cnt, (idx_t*)nullptr, (idx_t*)nullptr, (idx_t*)nullptr);
  PYG_HIP_CHECK(hipGetLastError());
  rc = device_scan<int64_t, SumOp>(ScanLoadI64{cnt}, ScanStoreI64{poff}, P, ptiles, total, stream);
  if (rc != PYG_HIP_OK) return rc;
  // the one synchronisation: the size of out_col
  int64_t K = 0;
  PYG_HIP_CHECK(hipMemcpyAsync(&K, total, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  PYG_HIP_CHECK(hipStreamSynchronize(stream));
  *num_out = K;
  *out_col = host->alloc(host->user, (size_t)K * sizeof(idx_t));
  PYG_HIP_REQUIRE(*out_col != nullptr, "subgraph: allocation of %lld output edges failed", (long long)K);
  *out_edge_id = nullptr;
  if (return_edge_id) {
    *out_edge_id = host->alloc(host->user, (size_t)K * sizeof(idx_t));
    if (*out_edge_id == nullptr) {
      host->free(host->user, *out_col);
      *out_col = nullptr;
      return fail(PYG_HIP_ERR_RUNTIME, "subgraph: allocation of %lld edge ids failed", (long long)K);
    }
  }
  hipLaunchKernelGGL((subgraph_edges_kernel<idx_t, true>), dim3((unsigned)P), dim3(kSgThreads), 0, stream, col, table,
                     cand_off, start, M, N, poff, out_rowptr, (idx_t*)*out_col, (idx_t*)*out_edge_id);
  PYG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((subgraph_rowptr_kernel<idx_t>), dim3(grid), dim3(256), 0, stream, cand_off, M, total, out_rowptr);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

}  // namespace
}  // namespace pyg_hip

using namespace pyg_hip;

extern "C" int pyg_hip_random_walk(int index_dtype, const void* rowptr, int64_t num_nodes, const void* col,
                                   int64_t num_edges, const void* seed, int64_t num_seeds, const float* rand,
                                   int64_t walk_length, void* out, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PYG_HIP_REQUIRE(index_dtype == PYG_I32 || index_dtype == PYG_I64,
                  "random_walk: int32 or int64 indices expected on the device (got dtype code %d)", index_dtype);
  PYG_HIP_REQUIRE(walk_length >= 0, "random_walk: walk_length must be non-negative (got %lld)", (long long)walk_length);
  PYG_HIP_REQUIRE(num_nodes >= 0 && num_edges >= 0 && num_seeds >= 0, "random_walk: negative size");
  if (num_seeds == 0) return PYG_HIP_OK;
  PYG_HIP_REQUIRE(rowptr && seed && out && (walk_length == 0 || (rand && (col || num_edges == 0))),
                  "random_walk: NULL buffer");
  if (index_dtype == PYG_I32)
    return random_walk_t<int32_t>(rowptr, num_nodes, col, num_edges, seed, num_seeds, rand, walk_length, out, stream);
  return random_walk_t<int64_t>(rowptr, num_nodes, col, num_edges, seed, num_seeds, rand, walk_length, out, stream);
}

extern "C" int pyg_hip_subgraph(int index_dtype, const void* rowptr, int64_t num_nodes, const void* col,
                                int64_t num_edges, const void* nodes, int64_t num_selected, int return_edge_id,
                                const pyg_hip_sampler_host* host, void* out_rowptr, void** out_col, void** out_edge_id,
                                int64_t* num_out_edges, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PYG_HIP_REQUIRE(index_dtype == PYG_I32 || index_dtype == PYG_I64,
                  "subgraph: int32 or int64 indices expected on the device (got dtype code %d)", index_dtype);
  PYG_HIP_REQUIRE(num_nodes >= 0 && num_edges >= 0 && num_selected >= 0, "subgraph: negative size");
  PYG_HIP_REQUIRE(num_selected < (int64_t)0x7FFFFFFF, "subgraph: at most 2^31 - 2 nodes (got %lld)",
                  (long long)num_selected);
  PYG_HIP_REQUIRE(host && host->alloc && host->free && out_rowptr && out_col && out_edge_id && num_out_edges,
                  "subgraph: NULL argument");
  if (num_selected == 0) {
    // out_rowptr = [0]; no synchronisation
    PYG_HIP_CHECK(hipMemsetAsync(out_rowptr, 0, index_dtype == PYG_I32 ? 4 : 8, stream));
    *num_out_edges = 0;
    *out_col = host->alloc(host->user, 0);
    *out_edge_id = return_edge_id ? host->alloc(host->user, 0) : nullptr;
    PYG_HIP_REQUIRE(*out_col && (!return_edge_id || *out_edge_id), "subgraph: allocation failed");
    return PYG_HIP_OK;
  }
  PYG_HIP_REQUIRE(rowptr && nodes && (col || num_edges == 0), "subgraph: NULL buffer");
  if (index_dtype == PYG_I32)
    return subgraph_t<int32_t>(rowptr, num_nodes, col, num_edges, nodes, num_selected, return_edge_id, host, out_rowptr,
                               out_col, out_edge_id, num_out_edges, stream);
  return subgraph_t<int64_t>(rowptr, num_nodes, col, num_edges, nodes, num_selected, return_edge_id, host, out_rowptr,
                             out_col, out_edge_id, num_out_edges, stream);
}
