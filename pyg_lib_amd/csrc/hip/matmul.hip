// segment_matmul / grouped_matmul for gfx950 (MI355X).
//
// Replaces pyg_lib/csrc/ops/cuda/matmul_kernel.cu (CUTLASS GemmGrouped, fp32 only) and the
// CPU path pyg_lib/csrc/ops/cpu/matmul_kernel.cpp:281-312,410-439.
//
// Design (DESIGN.md "segment_matmul"): the op is a stream of rows through a small per-relation
// weight, i.e. HBM-bound for bf16 (64 flop/B at F=128) and f32-MFMA bound for fp32.  One
// persistent launch walks a list of (group, row tile) work items, so a workgroup re-stages the
// relation's weight only when it crosses a segment boundary.
//
// This file: the plan kernel (ptr -> descriptors + tile prefixes), the workspace layout, the choice of
// the kernel family for a call (choose_route: the PYG_HIP_MM_SCHED_* table of pyg_hip.h), profiling
// events and the C entry points.  The MFMA kernels live in one translation unit per family behind the
// launch_* functions of matmul_common.h.  Shapes no MFMA kernel covers, and the remaining dtypes of
// AT_DISPATCH_ALL_TYPES_AND2, run the plain one-thread-per-output kernel below ("naive").
#include "matmul_common.h"

#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

namespace pyg_hip {
namespace {

// ---- plan kernel: ptr on device -> descriptors + tile/row prefix sums --------------------------
__global__ void plan_segments_kernel(const int64_t* __restrict__ ptr, int64_t B, const char* a,
                                     const char* w, char* c, const char* bias, int64_t K,
                                     int64_t M, int elt, DevGroup* __restrict__ descs,
                                     int32_t* __restrict__ tile_start,
                                     int64_t* __restrict__ row_start, int32_t* __restrict__ tile_start2,
                                     int32_t* __restrict__ tile_start3, unsigned int* __restrict__ tickets) {
  // Single block; B is the number of relations (hundreds): a serial-per-chunk scan is plenty.
  __shared__ int64_t s_tiles[256];
  __shared__ int64_t s_tiles2[256];
  __shared__ int64_t s_tiles3[256];
  __shared__ int64_t s_rows[256];
  const int tid = threadIdx.x;
  tickets[tid] = 0;  // kTicketWords == blockDim.x: the per-XCD tile counters of the ticket kernel start at 0
  const int nthr = blockDim.x;
  const int64_t per = (B + nthr - 1) / nthr;
  const int64_t beg = min((int64_t)tid * per, B), end = min(beg + per, B);
  int64_t tiles = 0, tiles2 = 0, tiles3 = 0, rows = 0;
  for (int64_t b = beg; b < end; ++b) {
    int64_t r = ptr[b + 1] - ptr[b];
    if (r < 0) r = 0;
    rows += r;
    tiles += (r + kTileRows - 1) / kTileRows;
    tiles2 += (r + 2 * kTileRows - 1) / (2 * kTileRows);
    tiles3 += (r + kPairRows - 1) / kPairRows;
  }
  // exclusive scan of the four per-thread sums over the block: wave shuffles + the wave totals through LDS (a serial
  // walk of thread 0 over 256 LDS entries made this kernel 15 us in front of every segment_matmul call)
  {
    const int lane = tid & 63, wv = tid >> 6, nw = nthr >> 6;
    int64_t v[4] = {tiles, tiles2, tiles3, rows};
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int lo = __shfl_up((int)(uint32_t)v[q], d), hi = __shfl_up((int)(uint32_t)((uint64_t)v[q] >> 32), d);
        if (lane >= d) v[q] += (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
      }
    }
    if (lane == 63) {  // wave totals (inclusive value of the last lane)
      s_tiles[wv] = v[0];
      s_tiles2[wv] = v[1];
      s_tiles3[wv] = v[2];
      s_rows[wv] = v[3];
    }
    __syncthreads();
    int64_t base[4] = {0, 0, 0, 0}, all[4] = {0, 0, 0, 0};
    for (int i = 0; i < nw; ++i) {
      const int64_t w4[4] = {s_tiles[i], s_tiles2[i], s_tiles3[i], s_rows[i]};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (i < wv) base[q] += w4[q];
        all[q] += w4[q];
      }
    }
    __syncthreads();
    // exclusive prefix of this thread = waves in front + inclusive value - own sum
    s_tiles[tid] = base[0] + v[0] - tiles;
    s_tiles2[tid] = base[1] + v[1] - tiles2;
    s_tiles3[tid] = base[2] + v[2] - tiles3;
    s_rows[tid] = base[3] + v[3] - rows;
    if (tid == 0) {
      tile_start[B] = (int32_t)all[0];
      tile_start2[B] = (int32_t)all[1];
      tile_start3[B] = (int32_t)all[2];
      row_start[B] = all[3];
    }
  }
  int64_t t = s_tiles[tid], t2 = s_tiles2[tid], t3 = s_tiles3[tid], rs = s_rows[tid];
  for (int64_t b = beg; b < end; ++b) {
    const int64_t p0 = ptr[b];
    int64_t r = ptr[b + 1] - p0;
    if (r < 0) r = 0;
    DevGroup d;
    d.a = a + p0 * K * elt;
    d.w = w + b * K * M * elt;
    d.c = c + p0 * M * elt;
    d.bias = bias ? bias + b * M * elt : nullptr;
    d.rows = r;
    d.k = (int32_t)K;
    d.m = (int32_t)M;
    d.trans = 0;
    d.pad = gen_class(d.a, d.w, d.c, K, M, elt, 0);
    descs[b] = d;
    tile_start[b] = (int32_t)t;
    tile_start2[b] = (int32_t)t2;
    tile_start3[b] = (int32_t)t3;
    row_start[b] = rs;
    t += (r + kTileRows - 1) / kTileRows;
    t2 += (r + 2 * kTileRows - 1) / (2 * kTileRows);
    t3 += (r + kPairRows - 1) / kPairRows;
    rs += r;
  }
}

// ---- generic kernel: one thread per output element, any dtype / shape ----------------------------
template <typename T, typename Acc>
struct NaiveCvt {
  __device__ static Acc load(const T* p) { return (Acc)*p; }
  __device__ static void store(T* p, Acc v) { *p = (T)v; }
  __device__ static Acc round(Acc v) { return (Acc)(T)v; }
};
template <>
struct NaiveCvt<bf16_t, float> {
  __device__ static float load(const bf16_t* p) { return load_bias(p); }
  __device__ static void store(bf16_t* p, float v) {
    p->v = __builtin_bit_cast(uint16_t, (__bf16)v);
  }
  __device__ static float round(float v) { return (float)(__bf16)v; }
};
template <>
struct NaiveCvt<f16_t, float> {
  __device__ static float load(const f16_t* p) { return load_bias(p); }
  __device__ static void store(f16_t* p, float v) {
    p->v = __builtin_bit_cast(uint16_t, (_Float16)v);
  }
  __device__ static float round(float v) { return (float)(_Float16)v; }
};

template <typename T, typename Acc>
__global__ void naive_kernel(const DevGroup* __restrict__ descs,
                             const int64_t* __restrict__ out_start, int B, int64_t total) {
  // out_start[g] = number of output elements in groups < g
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    if (idx >= out_start[B]) break;
    int lo = 0, hi = B;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (out_start[mid] <= idx) lo = mid; else hi = mid;
    }
    const DevGroup d = descs[lo];
    const int64_t local = idx - out_start[lo];
    const int64_t r = local / d.m;
    const int c = (int)(local - r * d.m);
    const T* a = reinterpret_cast<const T*>(d.a) + r * d.k;
    const T* w = reinterpret_cast<const T*>(d.w);
    Acc acc = 0;
    if (!d.trans) {
      for (int k = 0; k < d.k; ++k)
        acc += NaiveCvt<T, Acc>::load(a + k) * NaiveCvt<T, Acc>::load(w + (int64_t)k * d.m + c);
    } else {
      for (int k = 0; k < d.k; ++k)
        acc += NaiveCvt<T, Acc>::load(a + k) * NaiveCvt<T, Acc>::load(w + (int64_t)c * d.k + k);
    }
    if (d.bias)
      acc = NaiveCvt<T, Acc>::round(acc) +
            NaiveCvt<T, Acc>::load(reinterpret_cast<const T*>(d.bias) + c);
    NaiveCvt<T, Acc>::store(reinterpret_cast<T*>(d.c) + r * d.m + c, acc);
  }
}

__global__ void out_start_kernel(const DevGroup* __restrict__ descs, int B,
                                 int64_t* __restrict__ out_start) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    int64_t s = 0;
    for (int b = 0; b < B; ++b) {
      out_start[b] = s;
      s += descs[b].rows * descs[b].m;
    }
    out_start[B] = s;
  }
}

// ---- host side -----------------------------------------------------------------------------------
// Optional per-launch timing of the dominant kernel (bench.py roofline leg): when enabled, a pair of
// HIP events brackets the main kernel on the stream it is launched on.
struct ProfPair { hipEvent_t a, b; };
thread_local bool g_prof_on = false;
thread_local std::vector<ProfPair> g_prof;

struct ProfScope {
  hipStream_t s;
  bool on;
  ProfPair p;
  explicit ProfScope(hipStream_t st) : s(st), on(g_prof_on) {
    if (on) {
      on = hipEventCreate(&p.a) == hipSuccess && hipEventCreate(&p.b) == hipSuccess;
      if (on) (void)hipEventRecord(p.a, s);
    }
  }
  ~ProfScope() {
    if (on) {
      (void)hipEventRecord(p.b, s);
      g_prof.push_back(p);
    }
  }
};

struct Workspace {
  DevGroup* descs;
  int32_t* tile_start;
  int64_t* row_start;   // also reused as out_start by the naive path
  int64_t* ptr_copy;
  int32_t* tile_start2;  // prefix of 256-row workgroup tiles (cyclic-schedule kernel)
  int32_t* tile_start3;  // prefix of 64-row tiles (ticket kernel)
  unsigned int* tickets; // kTicketWords counters of the ticket kernel, zero before its launch
  size_t bytes;          // of the whole layout
};

// The workspace layout: `ws` (may be null: size query) cut into the arrays above; Workspace::bytes = what the cut needs.
Workspace carve(void* ws, int64_t B) {
  Workspace w;
  size_t off = 0;
  auto take = [&](size_t bytes, size_t align) {
    void* p = reinterpret_cast<void*>(reinterpret_cast<uintptr_t>(ws) + off);
    off += align_up(bytes, align);
    return p;
  };
  w.descs = static_cast<DevGroup*>(take(sizeof(DevGroup) * (size_t)std::max<int64_t>(B, 1), 256));
  w.tile_start = static_cast<int32_t*>(take(sizeof(int32_t) * (size_t)(B + 1), 256));
  w.row_start = static_cast<int64_t*>(take(sizeof(int64_t) * (size_t)(B + 1), 256));
  w.ptr_copy = static_cast<int64_t*>(take(sizeof(int64_t) * (size_t)(B + 1), 256));
  w.tile_start2 = static_cast<int32_t*>(take(sizeof(int32_t) * (size_t)(B + 1), 256));
  w.tile_start3 = static_cast<int32_t*>(take(sizeof(int32_t) * (size_t)(B + 1), 256));
  w.tickets = static_cast<unsigned int*>(take(sizeof(unsigned int) * kTicketWords, 1));
  w.bytes = off;
  return w;
}
size_t workspace_bytes(int64_t B) { return carve(nullptr, B).bytes; }

// ---- the route: which kernel family serves a call -------------------------------------------------
// The mode of a call, decoded from the entry point's `flags` argument (pyg_hip.h) and passed by value: nothing outlives a
// call, so two threads with different modes never see each other's choice.
struct Mode {
  int schedule;    // PYG_HIP_MM_SCHED_*
  bool f32_split;  // PYG_HIP_MM_F32_SPLIT: fp32 K = 128, M % 128 == 0 in split-bf16 arithmetic, else v_mfma_f32_32x32x2_f32
};

inline bool decode_mode(int flags, Mode* mode) {
  const int sched = flags & PYG_HIP_MM_SCHED_MASK;
  if (sched > PYG_HIP_MM_SCHED_RING || (flags & ~(PYG_HIP_MM_SCHED_MASK | PYG_HIP_MM_F32_SPLIT)) != 0) return false;
  *mode = Mode{sched, (flags & PYG_HIP_MM_F32_SPLIT) != 0};
  return true;
}

// What an entry point knows about its call on the host, without reading device memory.
struct Notes {
  int B = 0;               // groups
  int num_cus = 0;         // compute units of the current device
  int64_t rows_upper = 0;  // upper bound of the rows of the call
  bool any_trans = false;  // some group reads a transposed `other`
  bool gen_ok = false;     // every group can run the general-shape MFMA kernel (element-aligned pointers)
  int64_t mean_k = 0;      // row-weighted mean contraction length (tile run length of that kernel)
};

enum class Family {
  kNone,        // nothing to do
  kNaive,       // one thread per output element (this file)
  kGen,         // matmul_gen.hip
  kLds,         // matmul_lds.hip, Route::mc columns per workgroup
  kLdsF32x3,    // matmul_lds.hip, fp32 split-bf16
  kF32Pipe,     // matmul_f32_pipe.hip, Route::mc columns per workgroup
  kF32x3Ring,   // matmul_ring.hip, fp32 split-bf16
  kK128Ring,    // matmul_ring.hip
  kK128Ticket,  // matmul_k128.hip
  kK128Cyc,     // matmul_k128.hip
  kK256Ring,    // matmul_ring.hip
  kK256WideR2,  // matmul_k256.hip, 64 rows per wave
  kK256Wide,    // matmul_k256.hip, 32 rows per wave
};
struct Route {
  Family family;
  int mc = 0;  // column chunk of kLds / kF32Pipe
};

// The thresholds of the automatic schedule.
// Relations shorter than this on average take an item-ring kernel: 16-bit K = M = 128, and fp32 K = M = 128 in split-bf16
// (4 Mi rows: 128 rows per relation 1.25 vs 2.52 ms through the LDS-W kernel, 1024 rows 1.15 vs 1.13, 16 Ki rows 0.98 vs 0.94).
constexpr int64_t kRingMeanRows = 4096;
constexpr int64_t kRingMeanRowsF32Split = 512;
inline bool short_relations(const Notes& n, int64_t mean_rows) { return n.rows_upper < mean_rows * (int64_t)n.B; }
// Enough work for every CU to sweep several 256-row tiles: the ticket schedule pays off.
inline bool big_call(const Notes& n) { return n.rows_upper >= (int64_t)n.num_cus * 256 * 4; }
// Wide contractions go to the general-shape kernel (128-row tiles, K in 64-value chunks through a double-buffered LDS image):
// the LDS-weight kernel keeps ALL of W's K rows in LDS -- at K = 512, and in fp32 from K = 256, that leaves one small
// column chunk per pass and every pass re-reads X.  Measured (tools/mm_shape_sweep2.py, long / short / few segments): bf16
// K = 512 4 - 6 x faster through the general kernel for every M, K = 256 with M not a multiple of 256 1.15 - 3 x, fp32 K >= 256
// 1.5 - 2.9 x.  (K = 256 with M % 256 == 0 keeps the register-W / 256-column kernels; explicit schedules keep their kernels.)
inline bool wide_k(int dtype, int64_t K, int64_t M) {
  return K == 512 || (K == 256 && (dtype == PYG_F32 || M % 256 != 0));
}

bool mfma_shape_ok(int dtype, int64_t K, int64_t M) {
  if (!(dtype == PYG_F32 || dtype == PYG_BF16 || dtype == PYG_F16)) return false;
  if (!(K == 32 || K == 64 || K == 128 || K == 256 || K == 512)) return false;
  if (M < 32 || M % 32 != 0 || M > (1 << 20)) return false;
  return true;
}

// Output columns per workgroup pass of the LDS-weight kernels (what fits next to the stages).
inline int lds_column_chunk(int dtype, int64_t K, int64_t M) {
  // 16-bit, K = 128: one workgroup can own 256 columns (weights + stages fit), X is read by one CU only
  if (dtype != PYG_F32 && K == 128 && M % 256 == 0) return 256;
  return (M % 128 == 0 && K <= 256) ? 128 : (M % 64 == 0 ? 64 : 32);
}

// The route of a call with K > 0 and something to write: the PYG_HIP_MM_SCHED_* table of pyg_hip.h.  `uniform`: all groups
// share (K, M) and every pointer is 16-byte aligned.  Pure: no HIP call, no global.
Route choose_route(int dtype, int64_t K, int64_t M, bool uniform, Mode mode, const Notes& n) {
  const int s = mode.schedule;
  const bool automatic = s == PYG_HIP_MM_SCHED_AUTO;
  const bool mfma_dtype = dtype == PYG_F32 || dtype == PYG_BF16 || dtype == PYG_F16;
  const Route general = {n.gen_ok && mfma_dtype ? Family::kGen : Family::kNaive};
  // NAIVE / GENERAL (measurement only): every call / every floating-point call
  if (s == PYG_HIP_MM_SCHED_NAIVE) return {Family::kNaive};
  if (s == PYG_HIP_MM_SCHED_GENERAL || !uniform || !mfma_shape_ok(dtype, K, M)) return general;
  if (automatic && n.gen_ok && wide_k(dtype, K, M)) return general;
  if (dtype != PYG_F32) {
    if (K == 256 && M % 256 == 0) {
      // AUTO / RING: W in registers + item ring; CYCLIC / TICKET: W in LDS, 64 rows per wave (every W fragment read from
      // LDS feeds two MFMAs); CONTIGUOUS, and any M > 256: W in LDS, 32 rows per wave
      if (M == 256 && (automatic || s == PYG_HIP_MM_SCHED_RING)) return {Family::kK256Ring};
      if (M == 256 && s != PYG_HIP_MM_SCHED_CONTIGUOUS) return {Family::kK256WideR2};
      return {Family::kK256Wide};
    }
    if (K == 128 && M == 128) {  // the headline shape
      // many short relations: the item ring (a relation change = two ring items)
      if (s == PYG_HIP_MM_SCHED_RING || (automatic && short_relations(n, kRingMeanRows))) return {Family::kK128Ring};
      if (n.num_cus >= 8 && (s == PYG_HIP_MM_SCHED_TICKET || (automatic && big_call(n)))) return {Family::kK128Ticket};
      // (no group may read a transposed weight: the dX pass keeps the contiguous-range kernel)
      if (s == PYG_HIP_MM_SCHED_CYCLIC && !n.any_trans) return {Family::kK128Cyc};
    }
  } else if (mode.f32_split && K == 128 && M % 128 == 0) {
    // split-bf16: W planes in registers + LDS-DMA item ring for many short relations (a relation change costs four ring
    // items instead of a 96 KiB image built with 2-byte LDS writes), else three bf16 planes of W in LDS -- HBM-bound
    // instead of bound by the fp32 matrix rate
    if (M == 128 && (s == PYG_HIP_MM_SCHED_RING || (automatic && short_relations(n, kRingMeanRowsF32Split))))
      return {Family::kF32x3Ring};
    return {Family::kLdsF32x3};
  }
  // CONTIGUOUS, and what the rules above leave: one contiguous tile range per workgroup, W in LDS
  return {dtype == PYG_F32 && K == 128 ? Family::kF32Pipe : Family::kLds, lds_column_chunk(dtype, K, M)};
}

// pyg_hip_matmul_last_variant(): the name of the last route taken on this thread.
thread_local char g_last_variant[64] = "";

void name_route(int dtype, int64_t K, Route r) {
  const char* t = dtype == PYG_BF16 ? "bf16" : dtype == PYG_F16 ? "f16" : "f32";
  const char* fmt = "";
  switch (r.family) {
    case Family::kNone: fmt = "none"; break;
    case Family::kNaive: fmt = "naive"; break;
    case Family::kGen: fmt = "mfma_%s_gen"; break;
    case Family::kLds:
    case Family::kF32Pipe: fmt = "mfma_%s_k%d_mc%d"; break;
    case Family::kLdsF32x3: fmt = "mfma_f32_k128_mc128_x3"; break;
    case Family::kF32x3Ring: fmt = "mfma_f32_k128_regw_x3"; break;
    case Family::kK128Ring: fmt = "mfma_%s_k128_mc128_ring"; break;
    case Family::kK128Ticket: fmt = "mfma_%s_k128_mc128_ticket"; break;
    case Family::kK128Cyc: fmt = "mfma_%s_k128_mc128_cyc"; break;
    case Family::kK256Ring: fmt = "mfma_%s_k256_regw"; break;
    case Family::kK256WideR2: fmt = "mfma_%s_k256_wide256r2"; break;
    case Family::kK256Wide: fmt = "mfma_%s_k256_wide256"; break;
  }
  snprintf(g_last_variant, sizeof(g_last_variant), fmt, t, (int)K, r.mc);
}

template <typename T, typename Acc>
int launch_naive(const Workspace& w, int B, int64_t total_upper, hipStream_t stream) {
  int64_t blocks = std::min<int64_t>((total_upper + 255) / 256, 256 * 16);
  if (blocks < 1) blocks = 1;
  // `total` is read on device from out_start[B]; pass the host upper bound for the loop limit
  hipLaunchKernelGGL((naive_kernel<T, Acc>), dim3((unsigned)blocks), dim3(256), 0, stream,
                     w.descs, w.row_start, B, total_upper);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

int launch_naive_any(int dtype, const Workspace& w, int B, int64_t total, hipStream_t stream) {
  switch (dtype) {
    case PYG_F32: return launch_naive<float, float>(w, B, total, stream);
    case PYG_F64: return launch_naive<double, double>(w, B, total, stream);
    case PYG_F16: return launch_naive<f16_t, float>(w, B, total, stream);
    case PYG_BF16: return launch_naive<bf16_t, float>(w, B, total, stream);
    case PYG_I8: return launch_naive<int8_t, int8_t>(w, B, total, stream);
    case PYG_U8: return launch_naive<uint8_t, uint8_t>(w, B, total, stream);
    case PYG_I16: return launch_naive<int16_t, int16_t>(w, B, total, stream);
    case PYG_I32: return launch_naive<int32_t, int32_t>(w, B, total, stream);
    case PYG_I64: return launch_naive<int64_t, int64_t>(w, B, total, stream);
    default: return fail(PYG_HIP_ERR_INVALID, "matmul: unknown dtype %d", dtype);
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Launch the kernel of route `r` on the planned workspace.  `tiles_upper` / `out_elems_upper`: upper bounds of the 128-row
// tiles / the output elements of the call.
int run_route(Route r, int dtype, const Workspace& w, const Notes& n, int64_t K, int64_t M, int64_t tiles_upper,
              int64_t out_elems_upper, hipStream_t stream) {
  name_route(dtype, K, r);
  const int B = n.B;
  const int64_t tiles2_upper = (n.rows_upper + 2 * kTileRows - 1) / (2 * kTileRows) + B;
  const int64_t tiles3_upper = (n.rows_upper + kPairRows - 1) / kPairRows + B;
  if (r.family == Family::kNaive) {  // its group table, in front of the timed kernel
    hipLaunchKernelGGL(out_start_kernel, dim3(1), dim3(64), 0, stream, w.descs, B, w.row_start);
    PYG_HIP_CHECK(hipGetLastError());
  }
  ProfScope prof(stream);
  switch (r.family) {
    case Family::kNone: return PYG_HIP_OK;
    case Family::kNaive: return launch_naive_any(dtype, w, B, out_elems_upper, stream);
    case Family::kGen: return launch_matmul_gen(dtype, w.descs, w.tile_start, B, tiles_upper, n.mean_k, stream);
    case Family::kLds: return launch_lds(dtype, (int)K, r.mc, w.descs, w.tile_start, B, tiles_upper, (int)M, stream);
    case Family::kLdsF32x3: return launch_lds_f32x3(w.descs, w.tile_start, B, tiles_upper, (int)M, stream);
    case Family::kF32Pipe: return launch_f32_pipe(r.mc, w.descs, w.tile_start, B, tiles_upper, (int)M, stream);
    case Family::kF32x3Ring: return launch_ring_f32x3(w.descs, w.tile_start3, B, tiles3_upper, stream);
    case Family::kK128Ring: return launch_ring_k128(dtype, w.descs, w.tile_start3, B, tiles3_upper, stream);
    case Family::kK128Ticket: return launch_k128_ticket(dtype, w.descs, w.tile_start3, B, tiles3_upper, w.tickets, stream);
    case Family::kK128Cyc: return launch_k128_cyc(dtype, w.descs, w.tile_start2, B, tiles2_upper, stream);
    case Family::kK256Ring: return launch_ring_k256(dtype, w.descs, w.tile_start3, B, tiles3_upper, stream);
    case Family::kK256WideR2: return launch_k256_wide_r2(dtype, w.descs, w.tile_start2, B, tiles2_upper, stream);
    case Family::kK256Wide: return launch_k256_wide(dtype, w.descs, w.tile_start, B, tiles_upper, (int)M, stream);
  }
  return fail(PYG_HIP_ERR_INVALID, "matmul: unknown route");
}

}  // namespace
}  // namespace pyg_hip

using namespace pyg_hip;

extern "C" {

size_t pyg_hip_matmul_workspace_size(int64_t num_groups) {
  return workspace_bytes(num_groups < 0 ? 0 : num_groups);
}

const char* pyg_hip_matmul_last_variant(void) { return g_last_variant; }

void pyg_hip_profile_enable(int on) {
  g_prof_on = on != 0;
  if (!g_prof_on) {
    for (auto& p : g_prof) {
      (void)hipEventDestroy(p.a);
      (void)hipEventDestroy(p.b);
    }
    g_prof.clear();
  }
}

int pyg_hip_profile_collect(float* ms_out, int capacity) {
  int n = 0;
  for (auto& p : g_prof) {
    float ms = 0.f;
    if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      if (n < capacity && ms_out) ms_out[n] = ms;
      ++n;
    }
    (void)hipEventDestroy(p.a);
    (void)hipEventDestroy(p.b);
  }
  g_prof.clear();
  return n;
}

int pyg_hip_segment_matmul(int dtype, const void* input, const int64_t* ptr, int ptr_on_device,
                           const void* other, const void* bias, void* out, int64_t N, int64_t K,
                           int64_t M, int64_t B, void* workspace, size_t workspace_bytes_,
                           int flags, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const size_t elt = dtype_size(dtype);
  PYG_HIP_REQUIRE(elt != 0, "segment_matmul: unknown dtype %d", dtype);
  Mode mode;
  PYG_HIP_REQUIRE(decode_mode(flags, &mode), "segment_matmul: unknown bits in 'flags' (0x%x)", flags);
  PYG_HIP_REQUIRE(N >= 0 && K >= 0 && M >= 0 && B >= 0, "segment_matmul: negative size");
  PYG_HIP_REQUIRE(ptr != nullptr, "segment_matmul: 'ptr' is NULL");
  PYG_HIP_REQUIRE(B < (1LL << 31), "segment_matmul: too many segments");
  name_route(dtype, 0, {Family::kNone});
  if (B == 0 || N == 0 || M == 0) return PYG_HIP_OK;
  PYG_HIP_REQUIRE(out && (K == 0 || (input && other)), "segment_matmul: NULL tensor");
  PYG_HIP_REQUIRE((N + kPairRows - 1) / kPairRows + B < (1LL << 31),
                  "segment_matmul: too many row tiles");
  if (workspace_bytes_ < workspace_bytes(B) || workspace == nullptr)
    return fail(PYG_HIP_ERR_WORKSPACE, "segment_matmul: workspace of %zu bytes needed, got %zu",
                workspace_bytes(B), workspace_bytes_);
  Workspace w = carve(workspace, B);

  const int64_t* dptr = ptr;
  if (!ptr_on_device) {
    if (int rc = stage_host_ptr("segment_matmul", ptr, B, N, w.ptr_copy, stream)) return rc;
    dptr = w.ptr_copy;
  }
  hipLaunchKernelGGL(plan_segments_kernel, dim3(1), dim3(256), 0, stream, dptr, B,
                     static_cast<const char*>(input), static_cast<const char*>(other),
                     static_cast<char*>(out), static_cast<const char*>(bias), K, M, (int)elt,
                     w.descs, w.tile_start, w.row_start, w.tile_start2, w.tile_start3, w.tickets);
  PYG_HIP_CHECK(hipGetLastError());
  Notes n;
  n.B = (int)B;
  n.num_cus = device_info().num_cus;
  n.rows_upper = N;
  const int64_t tiles_upper = (N + kTileRows - 1) / kTileRows + B;
  const bool fast = aligned16(input) && aligned16(other) && aligned16(out);
  const uintptr_t all_ptrs = (uintptr_t)input | (uintptr_t)other | (uintptr_t)out | (uintptr_t)bias;
  n.gen_ok = (dtype == PYG_F32 || dtype == PYG_BF16 || dtype == PYG_F16) && all_ptrs % elt == 0 && K < (1LL << 21) &&
             M < (1LL << 21);
  n.mean_k = K;
  // empty contraction: out = 0 (+ bias), written by the generic kernel
  const Route route = K == 0 ? Route{Family::kNaive} : choose_route(dtype, K, M, fast, mode, n);
  return run_route(route, dtype, w, n, K, M, tiles_upper, N * M, stream);
}

int pyg_hip_grouped_matmul(int dtype, const pyg_hip_group* groups, int64_t G, void* workspace,
                           size_t workspace_bytes_, int flags, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const size_t elt = dtype_size(dtype);
  PYG_HIP_REQUIRE(elt != 0, "grouped_matmul: unknown dtype %d", dtype);
  Mode mode;
  PYG_HIP_REQUIRE(decode_mode(flags, &mode), "grouped_matmul: unknown bits in 'flags' (0x%x)", flags);
  PYG_HIP_REQUIRE(G >= 0 && G < (1LL << 31), "grouped_matmul: bad group count");
  name_route(dtype, 0, {Family::kNone});
  if (G == 0) return PYG_HIP_OK;
  PYG_HIP_REQUIRE(groups != nullptr, "grouped_matmul: 'groups' is NULL");
  if (workspace_bytes_ < workspace_bytes(G) || workspace == nullptr)
    return fail(PYG_HIP_ERR_WORKSPACE, "grouped_matmul: workspace of %zu bytes needed, got %zu",
                workspace_bytes(G), workspace_bytes_);
  Workspace w = carve(workspace, G);

  // Host-side plan (G is small): descriptors + tile prefix, one pinned H2D copy.
  const size_t descs_b = align_up(sizeof(DevGroup) * (size_t)G, 256);
  const size_t tiles_b = align_up(sizeof(int32_t) * (size_t)(G + 1), 256);
  void* staged = nullptr;
  int rc = pinned_stage().acquire(descs_b + 3 * tiles_b, &staged);
  if (rc != PYG_HIP_OK) return rc;
  DevGroup* hd = static_cast<DevGroup*>(staged);
  int32_t* ht = reinterpret_cast<int32_t*>(static_cast<char*>(staged) + descs_b);
  int32_t* ht2 = reinterpret_cast<int32_t*>(static_cast<char*>(staged) + descs_b + tiles_b);
  int32_t* ht3 = reinterpret_cast<int32_t*>(static_cast<char*>(staged) + descs_b + 2 * tiles_b);
  int64_t tiles2 = 0, tiles3 = 0, rows_total = 0;
  bool uniform = true, any_trans = false;
  bool gen_ok = dtype == PYG_F32 || dtype == PYG_BF16 || dtype == PYG_F16;
  int64_t tiles = 0, out_elems = 0, k_rows = 0;
  for (int64_t i = 0; i < G; ++i) {
    const pyg_hip_group& gr = groups[i];
    PYG_HIP_REQUIRE(gr.rows >= 0 && gr.k >= 0 && gr.m >= 0, "grouped_matmul: negative size");
    PYG_HIP_REQUIRE(gr.rows == 0 || gr.m == 0 || (gr.out && (gr.k == 0 || (gr.input && gr.other))),
                    "grouped_matmul: NULL tensor in group %lld", (long long)i);
    hd[i].a = static_cast<const char*>(gr.input);
    hd[i].w = static_cast<const char*>(gr.other);
    hd[i].c = static_cast<char*>(gr.out);
    hd[i].bias = nullptr;
    hd[i].rows = gr.m == 0 ? 0 : gr.rows;
    hd[i].k = gr.k;
    hd[i].m = gr.m;
    hd[i].trans = gr.other_trans ? 1 : 0;
    hd[i].pad = gen_class(gr.input, gr.other, gr.out, gr.k, gr.m, (int)elt, hd[i].trans);
    if ((((uintptr_t)gr.input | (uintptr_t)gr.other | (uintptr_t)gr.out) % elt) != 0 || gr.k >= (1 << 21) ||
        gr.m >= (1 << 21))
      gen_ok = false;
    k_rows += (int64_t)gr.k * hd[i].rows;
    if (gr.k != groups[0].k || gr.m != groups[0].m) uniform = false;
    if (!aligned16(gr.input) || !aligned16(gr.other) || !aligned16(gr.out)) uniform = false;
    if (gr.other_trans) any_trans = true;
    ht[i] = (int32_t)tiles;
    ht2[i] = (int32_t)tiles2;
    ht3[i] = (int32_t)tiles3;
    tiles2 += (hd[i].rows + 2 * kTileRows - 1) / (2 * kTileRows);
    tiles3 += (hd[i].rows + kPairRows - 1) / kPairRows;
    PYG_HIP_REQUIRE(tiles3 < (1LL << 31), "grouped_matmul: too many row tiles");
    rows_total += hd[i].rows;
    tiles += (hd[i].rows + kTileRows - 1) / kTileRows;
    out_elems += hd[i].rows * gr.m;
    PYG_HIP_REQUIRE(tiles < (1LL << 31), "grouped_matmul: too many row tiles");
  }
  Notes n;
  n.B = (int)G;
  n.num_cus = device_info().num_cus;
  n.any_trans = any_trans;
  n.rows_upper = rows_total;
  n.gen_ok = gen_ok;
  n.mean_k = rows_total > 0 ? k_rows / rows_total : 0;
  ht[G] = (int32_t)tiles;
  ht2[G] = (int32_t)tiles2;
  ht3[G] = (int32_t)tiles3;
  PYG_HIP_CHECK(hipMemcpyAsync(w.descs, hd, sizeof(DevGroup) * (size_t)G, hipMemcpyHostToDevice,
                               stream));
  PYG_HIP_CHECK(hipMemcpyAsync(w.tile_start, ht, sizeof(int32_t) * (size_t)(G + 1),
                               hipMemcpyHostToDevice, stream));
  PYG_HIP_CHECK(hipMemcpyAsync(w.tile_start2, ht2, sizeof(int32_t) * (size_t)(G + 1),
                               hipMemcpyHostToDevice, stream));
  PYG_HIP_CHECK(hipMemcpyAsync(w.tile_start3, ht3, sizeof(int32_t) * (size_t)(G + 1),
                               hipMemcpyHostToDevice, stream));
  PYG_HIP_CHECK(hipMemsetAsync(w.tickets, 0, sizeof(unsigned int) * kTicketWords, stream));
  rc = pinned_stage().commit(stream);
  if (rc != PYG_HIP_OK) return rc;
  if (out_elems == 0) return PYG_HIP_OK;
  if (groups[0].k == 0) uniform = false;
  const Route route = choose_route(dtype, groups[0].k, groups[0].m, uniform, mode, n);
  return run_route(route, dtype, w, n, groups[0].k, groups[0].m, tiles, out_elems, stream);
}

}  // extern "C"
