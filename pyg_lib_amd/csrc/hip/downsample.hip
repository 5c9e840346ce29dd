// fps and grid_cluster for gfx950 (MI355X): choosing the points of a point cloud.
//
// Replaces pyg_lib/csrc/ops/cuda/{fps,cluster}_kernel.cu.  Semantics: include/pyg_hip.h.
//
// fps is a serial loop -- ceil(ratio * n) iterations per example -- so the time of ONE iteration is the whole cost.  The
// reference runs a 256-thread block per example that re-reads and re-writes a distance array in global memory, re-reads all
// points and ends in an eight-step __syncthreads tree, every iteration.  Here (fps_resident_kernel):
//   * one workgroup per example, 64 .. 1024 threads picked from the largest example; a thread owns kP points (point
//     tid + p * T: loads coalesce) and keeps their running distances in registers for the whole call;
//   * per iteration a thread updates its kP distances and forms ONE ordered key: the bits of the largest running distance
//     (+1; 0 for a NaN -- distances are sums of squares, never negative, so their bit patterns order like the values) above
//     the inverted local index, so that one unsigned max gives (largest distance, lowest index);
//   * the wave reduces the key with cross-lane operations, the lane that holds the maximum stores it in the LDS slot of its
//     wave, selected by the iteration's parity -- which is what lets an iteration need ONE barrier --, and every wave reads the
//     up-to-16 slots and finishes the reduction redundantly;
//   * SHAPE_D4 (D <= 4): the coordinates sit in registers too (padded to 4: (0 - 0)^2 adds +0 to a non-negative sum, the same
//     bits as the D-term sum), and the winner's coordinates travel with its key through the slot;
//     SHAPE_LDS / SHAPE_GLOB (any D): the coordinates are re-read every iteration, the winner's by every thread from the same
//     address (a broadcast), from an LDS copy of the example while it fits kGenLdsBytes, else from global memory;
//   * no FMA contraction anywhere in this file, and `new < run ? new : run` is a compare and a select, not v_min: the CPU key
//     (binding/pyg_binding_downsample.cpp) gives the same bits.
// stream: the same loop with 1024 threads and the running distances in the workspace (examples above the resident capacity).
// multi: few, very large examples -- one plain launch per sample, grid (G, B); see fps_multi_kernel.
// 16-bit inputs are widened to fp32 once (exact), so the fps kernels exist for float and double only.
//
// grid_cluster: one thread per point; the 16-bit types round after every operation (R of pyg_hip.h), so that kernel is
// instantiated for the four storage types.  A missing bound costs one more launch (minmax_kernel) and a redundant per-block
// reduction of its partials in the prologue of the second.
#include "common.h"
#include "elem.h"

#include <algorithm>
#include <mutex>

#pragma clang fp contract(off)

namespace pyg_hip {
namespace {

constexpr int kP = 8;                   // points per thread, resident route
constexpr int kMinThreads = 64;
constexpr int kMaxThreads = 1024;
constexpr int kCapacity = kMaxThreads * kP;
constexpr int kGenLdsBytes = 64 * 1024; // resident, D > 4: LDS copy of the example up to here
constexpr int kMultiThreads = 256;
constexpr int kSliceForced = 64;        // multi: shortest slice under PYG_HIP_FPS_FORCE_MULTI ...
constexpr int kSliceMin = 2048;         // ... and the shortest the rule cuts
constexpr int kMaxSlices = 1024;        // multi: partial keys per example
constexpr int64_t kMultiPoints = 16384; // multi: max_points from here on (measured cross-over about 12 000), and ...
constexpr int64_t kMultiExamples = 64;  // ... fewer examples than this
constexpr int64_t kMaxD = 4096;
constexpr int kMaxLds = 160 * 1024;

enum { SHAPE_D4 = 0, SHAPE_LDS = 1, SHAPE_GLOB = 2 };

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

template <typename A>
__device__ __forceinline__ A nan_v() {
  return (A)__builtin_nanf("");
}

// ---- the ordered key -------------------------------------------------------------------------------------------------
template <typename A>
struct Bits {
  using U = uint32_t;
};
template <>
struct Bits<double> {
  using U = uint64_t;
};

template <typename A>
struct Key {
  typename Bits<A>::U d;   // 0: NaN; else the distance's bits + 1
  uint32_t i;              // ~local index
};

// v: a running distance with NaN already mapped to a negative number
template <typename A>
__device__ __forceinline__ Key<A> make_key(A v, uint32_t index) {
  Key<A> k;
  k.d = v < A(0) ? 0 : __builtin_bit_cast(typename Bits<A>::U, v) + 1;
  k.i = ~index;
  return k;
}
template <typename A>
__device__ __forceinline__ bool key_gt(const Key<A>& a, const Key<A>& b) {
  if constexpr (sizeof(A) == 4) {
    return (((uint64_t)a.d << 32) | a.i) > (((uint64_t)b.d << 32) | b.i);
  } else {
    return a.d > b.d || (a.d == b.d && a.i > b.i);
  }
}
template <typename A>
__device__ __forceinline__ bool key_eq(const Key<A>& a, const Key<A>& b) {
  return a.d == b.d && a.i == b.i;
}
template <typename A>
__device__ __forceinline__ Key<A> wave_max(Key<A> k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Key<A> other;
    if constexpr (sizeof(A) == 4) {
      const unsigned long long v = __shfl_xor((unsigned long long)(((uint64_t)k.d << 32) | k.i), o);
      other.d = (uint32_t)(v >> 32), other.i = (uint32_t)v;
    } else {
      other.d = __shfl_xor((unsigned long long)k.d, o), other.i = __shfl_xor(k.i, o);
    }
    if (key_gt(other, k)) k = other;
  }
  return k;
}

template <typename A>
__device__ __forceinline__ A mapped(A r) {
  return r == r ? r : A(-1);   // NaN ranks below every number
}

// ---- the example of a block: clamped bounds, and what was wrong with them ---------------------------------------------
struct Example {
  int64_t lo, olo;
  int n, count, start;
};

struct FpsArgs {
  const int64_t *ptr, *out_ptr, *start;
  int64_t N, B, out_total, max_points, max_samples;
  int D;
  int64_t* out;
  int* pending;
};

__device__ __forceinline__ Example example_of(const FpsArgs& a, int64_t b) {
  Example e;
  bool bad = false;
  const int64_t p0 = a.ptr[b], p1 = a.ptr[b + 1];
  int64_t lo = p0 < 0 ? 0 : (p0 > a.N ? a.N : p0);
  int64_t hi = p1 < lo ? lo : (p1 > a.N ? a.N : p1);
  bad |= lo != p0 || hi != p1 || (b == 0 && p0 != 0) || (b == a.B - 1 && p1 != a.N);
  int64_t n = hi - lo;
  if (n > a.max_points) n = a.max_points, bad = true;
  const int64_t o0 = b ? a.out_ptr[b - 1] : 0, o1 = a.out_ptr[b];
  int64_t olo = o0 < 0 ? 0 : (o0 > a.out_total ? a.out_total : o0);
  int64_t ohi = o1 < olo ? olo : (o1 > a.out_total ? a.out_total : o1);
  bad |= olo != o0 || ohi != o1;
  int64_t count = ohi - olo;
  if (count > a.max_samples) count = a.max_samples, bad = true;
  int64_t s = a.start ? a.start[b] : 0;
  s = s > n - 1 ? n - 1 : s;
  s = s < 0 ? 0 : s;
  e.lo = lo, e.olo = olo, e.n = (int)n, e.count = (int)count, e.start = (int)s;
  if (bad && threadIdx.x == 0) *a.pending = 1;
  return e;
}

// an example without points that was promised samples: its pointer's (clamped) begin, as nearest answers without candidates
__device__ __forceinline__ void fill_empty(const FpsArgs& a, const Example& e) {
  for (int m = threadIdx.x; m < e.count; m += blockDim.x) a.out[e.olo + m] = e.lo;
  if (e.count > 0 && threadIdx.x == 0) *a.pending = 1;
}

template <typename A>
struct Slot4 {
  Key<A> key;
  A c0, c1, c2, c3;
};

template <typename T>
__global__ __launch_bounds__(256) void widen_kernel(const T* __restrict__ src, float* __restrict__ dst, int64_t n) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = Math<T>::up(src[i]);
}

// ---- resident: one workgroup per example, running distances in registers --------------------------------------------
template <typename A, int SHAPE, int T>
__global__ __launch_bounds__(T) void fps_resident_kernel(const A* __restrict__ src, const FpsArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int kWaves = T / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Example e = example_of(a, blockIdx.x);
  if (e.n == 0) {
    fill_empty(a, e);
    return;
  }
  if (e.count == 0) return;   // (an output range clamped to nothing: the loop below writes its first sample unasked)
  const int D = a.D, n = e.n;
  const A* pts = src + e.lo * D;
  int64_t* out = a.out + e.olo;
  int w = e.start;

  if constexpr (SHAPE == SHAPE_D4) {
    Slot4<A>* slots = reinterpret_cast<Slot4<A>*>(smem);   // [2][kWaves]
    A x0[kP], x1[kP], x2[kP], x3[kP], run[kP];
    // loads without control flow: a missing coordinate re-reads an earlier one and is replaced by 0, a point past the example
    // re-reads the last one and gets a NaN -- every distance of it is NaN, so it never wins against a point of the example
    const int e1 = D > 1 ? 1 : 0, e2 = D > 2 ? 2 : 0, e3 = D > 3 ? 3 : 0;
#pragma unroll
    for (int p = 0; p < kP; ++p) {
      const int j = tid + p * T;
      const A* cp = pts + (int64_t)(j < n ? j : n - 1) * D;
      const A v0 = cp[0], v1 = cp[e1], v2 = cp[e2], v3 = cp[e3];
      x0[p] = j < n ? v0 : nan_v<A>(), x1[p] = D > 1 ? v1 : A(0), x2[p] = D > 2 ? v2 : A(0), x3[p] = D > 3 ? v3 : A(0);
      run[p] = 0;
    }
    A c0, c1, c2, c3;
    {
      const A* cp = pts + (int64_t)w * D;
      const A v0 = cp[0], v1 = cp[e1], v2 = cp[e2], v3 = cp[e3];
      c0 = v0, c1 = D > 1 ? v1 : A(0), c2 = D > 2 ? v2 : A(0), c3 = D > 3 ? v3 : A(0);
    }
    for (int m = 0;; ++m) {
      if (tid == 0) out[m] = e.lo + w;
      if (m + 1 >= e.count) break;
      const bool first = m == 0;
      A bv = A(-2), b0 = 0, b1 = 0, b2 = 0, b3 = 0;
      int bj = 0;
#pragma unroll
      for (int p = 0; p < kP; ++p) {
        const A d0 = x0[p] - c0, d1 = x1[p] - c1, d2 = x2[p] - c2, d3 = x3[p] - c3;
        A nw = d0 * d0;
        nw = nw + d1 * d1;
        nw = nw + d2 * d2;
        nw = nw + d3 * d3;
        const A r = (first || nw < run[p]) ? nw : run[p];
        run[p] = r;
        const A v = mapped(r);
        const bool better = v > bv;   // strict: the lowest index among a thread's equals
        bv = better ? v : bv, bj = better ? tid + p * T : bj;
        b0 = better ? x0[p] : b0, b1 = better ? x1[p] : b1, b2 = better ? x2[p] : b2, b3 = better ? x3[p] : b3;
      }
      const Key<A> mine = make_key(bv, (uint32_t)bj);
      const Key<A> top = wave_max(mine);
      Slot4<A>* sl = slots + (m & 1) * kWaves;
      if (key_eq(mine, top)) {   // one lane: the index is part of the key
        Slot4<A> s;
        s.key = mine, s.c0 = b0, s.c1 = b1, s.c2 = b2, s.c3 = b3;
        sl[wave] = s;
      }
      __syncthreads();
      Key<A> best = sl[0].key;
      int bs = 0;
#pragma unroll
      for (int s = 1; s < kWaves; ++s) {
        const Key<A> k = sl[s].key;
        if (key_gt(k, best)) best = k, bs = s;
      }
      w = (int)~best.i;
      c0 = sl[bs].c0, c1 = sl[bs].c1, c2 = sl[bs].c2, c3 = sl[bs].c3;
    }
  } else {
    Key<A>* slots = reinterpret_cast<Key<A>*>(smem);   // [2][kWaves], then the example's points (SHAPE_LDS)
    A* lpts = reinterpret_cast<A*>(smem + 2 * kWaves * 16);
    if constexpr (SHAPE == SHAPE_LDS) {
      for (int64_t t = tid; t < (int64_t)n * D; t += T) lpts[t] = pts[t];
      __syncthreads();
    }
    A run[kP];
#pragma unroll
    for (int p = 0; p < kP; ++p) run[p] = 0;
    for (int m = 0;; ++m) {
      if (tid == 0) out[m] = e.lo + w;
      if (m + 1 >= e.count) break;
      const bool first = m == 0;
      A acc[kP];
      int64_t at[kP];
#pragma unroll
      for (int p = 0; p < kP; ++p) {
        const int j = tid + p * T;
        acc[p] = 0, at[p] = (int64_t)(j < n ? j : n - 1) * D;   // (points past the example read its last point; dropped below)
      }
      const int64_t cw = (int64_t)w * D;
      for (int d = 0; d < D; ++d) {
        const A cd = SHAPE == SHAPE_LDS ? lpts[cw + d] : pts[cw + d];
#pragma unroll
        for (int p = 0; p < kP; ++p) {
          const A xv = SHAPE == SHAPE_LDS ? lpts[at[p] + d] : pts[at[p] + d];
          const A diff = xv - cd;
          acc[p] = acc[p] + diff * diff;
        }
      }
      A bv = A(-2);
      int bj = 0;
#pragma unroll
      for (int p = 0; p < kP; ++p) {
        const int j = tid + p * T;
        const A nw = j < n ? acc[p] : nan_v<A>();
        const A r = (first || nw < run[p]) ? nw : run[p];
        run[p] = r;
        const A v = mapped(r);
        const bool better = v > bv;
        bv = better ? v : bv, bj = better ? j : bj;
      }
      const Key<A> mine = make_key(bv, (uint32_t)bj);
      const Key<A> top = wave_max(mine);
      Key<A>* sl = slots + (m & 1) * kWaves;
      if (lane == 0) sl[wave] = top;
      __syncthreads();
      Key<A> best = sl[0];
#pragma unroll
      for (int s = 1; s < kWaves; ++s) {
        const Key<A> k = sl[s];
        if (key_gt(k, best)) best = k;
      }
      w = (int)~best.i;
    }
  }
}

// ---- shared by stream and multi: one point against the winner, coordinates from global memory ---------------------------
template <typename A, bool SMALL>
struct Winner {
  A c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  const A* row = nullptr;
  __device__ __forceinline__ void set(const A* pts, int64_t w, int D) {
    row = pts + w * D;
    if (SMALL) {
      const A v0 = row[0], v1 = row[D > 1 ? 1 : 0], v2 = row[D > 2 ? 2 : 0], v3 = row[D > 3 ? 3 : 0];
      c0 = v0, c1 = D > 1 ? v1 : A(0), c2 = D > 2 ? v2 : A(0), c3 = D > 3 ? v3 : A(0);
    }
  }
  __device__ __forceinline__ A dist(const A* cp, int D) const {
    if (SMALL) {
      const A v0 = cp[0], v1 = cp[D > 1 ? 1 : 0], v2 = cp[D > 2 ? 2 : 0], v3 = cp[D > 3 ? 3 : 0];
      const A x1 = D > 1 ? v1 : A(0), x2 = D > 2 ? v2 : A(0), x3 = D > 3 ? v3 : A(0);
      const A d0 = v0 - c0, d1 = x1 - c1, d2 = x2 - c2, d3 = x3 - c3;
      A s = d0 * d0;
      s = s + d1 * d1;
      s = s + d2 * d2;
      s = s + d3 * d3;
      return s;
    }
    A s = 0;
    for (int d = 0; d < D; ++d) {
      const A diff = cp[d] - row[d];
      s = s + diff * diff;
    }
    return s;
  }
};

// the workgroup's largest key, in every thread; `slots` holds one key per wave and is free again after the call's barrier
// only once the NEXT barrier of the caller has passed (the callers alternate two slot arrays)
template <typename A>
__device__ __forceinline__ Key<A> block_max(Key<A> mine, Key<A>* slots, int waves) {
  const Key<A> top = wave_max(mine);
  if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = top;
  __syncthreads();
  Key<A> best = slots[0];
  for (int s = 1; s < waves; ++s) {
    const Key<A> k = slots[s];
    if (key_gt(k, best)) best = k;
  }
  return best;
}

// ---- stream: one workgroup per example, running distances in the workspace ----------------------------------------------
template <typename A, bool SMALL>
__global__ __launch_bounds__(kMaxThreads) void fps_stream_kernel(const A* __restrict__ src, A* __restrict__ run_ws, const FpsArgs a) {
  __shared__ Key<A> slots[2][kMaxThreads / 64];
  const int tid = threadIdx.x;
  const Example e = example_of(a, blockIdx.x);
  if (e.n == 0) {
    fill_empty(a, e);
    return;
  }
  if (e.count == 0) return;   // (an output range clamped to nothing: the loop below writes its first sample unasked)
  const int D = a.D, n = e.n;
  const A* pts = src + e.lo * D;
  A* run = run_ws + e.lo;
  int64_t* out = a.out + e.olo;
  int w = e.start;
  Winner<A, SMALL> win;
  for (int m = 0;; ++m) {
    if (tid == 0) out[m] = e.lo + w;
    if (m + 1 >= e.count) break;
    win.set(pts, w, D);
    const bool first = m == 0;
    A bv = A(-2);
    int bj = -1;   // (a thread without points: index 2^32 - 1, the lowest key there is)
    for (int j = tid; j < n; j += kMaxThreads) {
      const A nw = win.dist(pts + (int64_t)j * D, D);
      const A old = first ? nw : run[j];
      const A r = (first || nw < old) ? nw : old;
      run[j] = r;
      const A v = mapped(r);
      const bool better = v > bv;
      bv = better ? v : bv, bj = better ? j : bj;
    }
    const Key<A> best = block_max(make_key(bv, (uint32_t)bj), slots[m & 1], kMaxThreads / 64);
    w = (int)~best.i;
  }
}

// ---- multi: one launch per sample, grid (G, B) --------------------------------------------------------------------------
// Launch `it` (0 .. max_samples - 1): every block of example b reduces the partial keys launch it - 1 left in parity
// (it - 1) & 1 -- all of them, redundantly: no block waits for another --, block 0 writes sample `it`, then the block
// updates the running distances of its slice and leaves its partial key in parity it & 1.  The launches of one call are
// ordered by the stream, which is all the synchronisation there is.
template <typename A, bool SMALL>
__global__ __launch_bounds__(kMultiThreads) void fps_multi_kernel(const A* __restrict__ src, A* __restrict__ run_ws,
                                                                  Key<A>* __restrict__ part, int slice, int it, const FpsArgs a) {
  __shared__ Key<A> slots[2][kMultiThreads / 64];
  const int tid = threadIdx.x, g = blockIdx.x, G = gridDim.x;
  const int64_t b = blockIdx.y;
  const Example e = example_of(a, b);
  if (e.n == 0) {
    if (it == 0 && g == 0) fill_empty(a, e);
    return;
  }
  if (it >= e.count) return;
  const int n = e.n, D = a.D;
  const int used = (n + slice - 1) / slice;   // slices that hold points
  if (g >= used) return;
  const A* pts = src + e.lo * D;
  A* run = run_ws + e.lo;
  int w = e.start;
  if (it > 0) {
    const Key<A>* prev = part + ((int64_t)((it - 1) & 1) * a.B + b) * G;
    Key<A> mine;
    mine.d = 0, mine.i = 0;
    for (int s = tid; s < used; s += kMultiThreads) {
      const Key<A> k = prev[s];
      if (key_gt(k, mine)) mine = k;
    }
    w = (int)~block_max(mine, slots[0], kMultiThreads / 64).i;
  }
  if (g == 0 && tid == 0) a.out[e.olo + it] = e.lo + w;
  if (it + 1 >= e.count) return;
  Winner<A, SMALL> win;
  win.set(pts, w, D);
  const bool first = it == 0;
  const int j0 = g * slice, j1 = j0 + slice < n ? j0 + slice : n;
  A bv = A(-2);
  int bj = -1;
  for (int j = j0 + tid; j < j1; j += kMultiThreads) {
    const A nw = win.dist(pts + (int64_t)j * D, D);
    const A old = first ? nw : run[j];
    const A r = (first || nw < old) ? nw : old;
    run[j] = r;
    const A v = mapped(r);
    const bool better = v > bv;
    bv = better ? v : bv, bj = better ? j : bj;
  }
  const Key<A> best = block_max(make_key(bv, (uint32_t)bj), slots[1], kMultiThreads / 64);
  if (tid == 0) part[((int64_t)(it & 1) * a.B + b) * G + g] = best;
}

// ---- grid_cluster -----------------------------------------------------------------------------------------------------
// int64() of pyg_hip.h: NaN -> 0, saturating (the CPU key converts the same way)
template <typename A>
__device__ __forceinline__ int64_t to_i64(A v) {
  if (!(v == v)) return 0;
  if (v >= A(9223372036854775808.0)) return INT64_MAX;
  if (v <= A(-9223372036854775808.0)) return INT64_MIN;
  return (int64_t)v;
}

template <typename T>
__device__ __forceinline__ typename Math<T>::acc_t rnd(typename Math<T>::acc_t v) {
  return Math<T>::up(Math<T>::down(v));
}

template <typename T>
__device__ __forceinline__ int64_t voxel(typename Math<T>::acc_t pos, typename Math<T>::acc_t start, typename Math<T>::acc_t size) {
  using A = typename Math<T>::acc_t;
  const A shifted = rnd<T>(pos - start);
  const A q = rnd<T>(shifted / size);
  return to_i64<A>(trunc(q));
}

// torch.min / torch.max over a column: a NaN wins and stays
template <typename A>
__device__ __forceinline__ A nan_min(A m, A v) {
  return (m != m) ? m : ((v < m || v != v) ? v : m);
}
template <typename A>
__device__ __forceinline__ A nan_max(A m, A v) {
  return (m != m) ? m : ((v > m || v != v) ? v : m);
}

constexpr int kGridThreads = 256;
constexpr int kGridPoints = 4;      // points per thread of cluster_kernel
constexpr int kMinMaxBlocks = 128;  // partial minima / maxima per column

// partial[g][d] = min over the rows of block g, partial[G + g][d] = max (in the compute type); every block owns at least one row
template <typename T>
__global__ __launch_bounds__(kGridThreads) void minmax_kernel(const T* __restrict__ pos, int64_t N, int D, int64_t rows_per_block,
                                                              typename Math<T>::acc_t* __restrict__ partial) {
  using A = typename Math<T>::acc_t;
  __shared__ A red_min[kGridThreads], red_max[kGridThreads];
  const int tid = threadIdx.x, g = blockIdx.x, G = gridDim.x;
  const int64_t r0 = g * rows_per_block, r1 = r0 + rows_per_block < N ? r0 + rows_per_block : N;
  if (D <= kGridThreads) {
    const int rpp = kGridThreads / D;   // rows per pass: thread tid reads column tid % D of row tid / D, contiguous over the block
    const int c = tid % D;
    const int64_t first_row = r0 + tid / D;
    A mn = 0, mx = 0;
    bool any = false;
    if (tid < rpp * D)
      for (int64_t i = first_row; i < r1; i += rpp) {
        const A v = Math<T>::up(pos[i * D + c]);
        mn = any ? nan_min(mn, v) : v, mx = any ? nan_max(mx, v) : v, any = true;
      }
    // (rows tid / D >= 1 may be past a short block: they repeat the block's first row, which exists)
    if (!any) mn = mx = Math<T>::up(pos[r0 * D + c]);
    red_min[tid] = mn, red_max[tid] = mx;
    __syncthreads();
    if (tid < D) {
      for (int r = 1; r < rpp; ++r) mn = nan_min(mn, red_min[r * D + tid]), mx = nan_max(mx, red_max[r * D + tid]);
      partial[(int64_t)g * D + tid] = mn, partial[(int64_t)(G + g) * D + tid] = mx;
    }
  } else {
    for (int d = tid; d < D; d += kGridThreads) {
      A mn = Math<T>::up(pos[r0 * D + d]), mx = mn;
      for (int64_t i = r0 + 1; i < r1; ++i) {
        const A v = Math<T>::up(pos[i * D + d]);
        mn = nan_min(mn, v), mx = nan_max(mx, v);
      }
      partial[(int64_t)g * D + d] = mn, partial[(int64_t)(G + g) * D + d] = mx;
    }
  }
}

// bound d of a block: the caller's tensor, or the reduction of the G partials
template <typename T>
__device__ __forceinline__ typename Math<T>::acc_t bound_of(const T* given, const typename Math<T>::acc_t* partial, int G, int D, int d,
                                                            bool is_max) {
  using A = typename Math<T>::acc_t;
  if (given) return Math<T>::up(given[d]);
  A m = partial[d];
  for (int g = 1; g < G; ++g) m = is_max ? nan_max(m, partial[(int64_t)g * D + d]) : nan_min(m, partial[(int64_t)g * D + d]);
  return m;
}

// SMALL (D <= 4): start, size and the multipliers in registers; else in LDS: start [D] | size [D] | multiplier [D]
template <typename T, bool SMALL>
__global__ __launch_bounds__(kGridThreads) void cluster_kernel(const T* __restrict__ pos, int64_t N, int D, const T* __restrict__ size,
                                                               const T* __restrict__ start, const T* __restrict__ end,
                                                               const typename Math<T>::acc_t* __restrict__ partial, int G,
                                                               int64_t* __restrict__ out) {
  using A = typename Math<T>::acc_t;
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * (kGridThreads * kGridPoints);
  const A* pmin = partial;
  const A* pmax = partial ? partial + (int64_t)G * D : nullptr;
  if constexpr (SMALL) {
    A st[4] = {0, 0, 0, 0}, sz[4] = {1, 1, 1, 1};
    int64_t mul[4] = {0, 0, 0, 0};
    int64_t run = 1;
#pragma unroll
    for (int d = 0; d < 4; ++d)
      if (d < D) {
        st[d] = bound_of<T>(start, pmin, G, D, d, false);
        sz[d] = Math<T>::up(size[d]);
        const A en = bound_of<T>(end, pmax, G, D, d, true);
        mul[d] = run;
        run = (int64_t)((uint64_t)run * (uint64_t)(voxel<T>(en, st[d], sz[d]) + 1));
      }
#pragma unroll
    for (int k = 0; k < kGridPoints; ++k) {
      const int64_t i = base + k * kGridThreads + tid;
      if (i >= N) break;
      const T* cp = pos + i * D;
      uint64_t id = 0;
#pragma unroll
      for (int d = 0; d < 4; ++d)
        if (d < D) id += (uint64_t)voxel<T>(Math<T>::up(cp[d]), st[d], sz[d]) * (uint64_t)mul[d];
      out[i] = (int64_t)id;
    }
  } else {
    int64_t* mul = reinterpret_cast<int64_t*>(smem);
    A* st = reinterpret_cast<A*>(mul + D);
    A* sz = st + D;
    for (int d = tid; d < D; d += kGridThreads) {
      st[d] = bound_of<T>(start, pmin, G, D, d, false);
      sz[d] = Math<T>::up(size[d]);
      const A en = bound_of<T>(end, pmax, G, D, d, true);
      mul[d] = voxel<T>(en, st[d], sz[d]) + 1;   // the voxel count, turned into the multiplier below
    }
    __syncthreads();
    if (tid == 0) {
      uint64_t run = 1;
      for (int d = 0; d < D; ++d) {
        const uint64_t nd = (uint64_t)mul[d];
        mul[d] = (int64_t)run;
        run *= nd;
      }
    }
    __syncthreads();
    for (int k = 0; k < kGridPoints; ++k) {
      const int64_t i = base + k * kGridThreads + tid;
      if (i >= N) break;
      const T* cp = pos + i * D;
      uint64_t id = 0;
      for (int d = 0; d < D; ++d) id += (uint64_t)voxel<T>(Math<T>::up(cp[d]), st[d], sz[d]) * (uint64_t)mul[d];
      out[i] = (int64_t)id;
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
thread_local char g_last_route[64] = "none";

// the pure part of the dispatch: what pyg_hip_fps_route answers and pyg_hip_fps follows
struct Plan {
  int route = PYG_HIP_FPS_ROUTE_UNSUPPORTED;
  int shape = SHAPE_D4, threads = kMinThreads, slice = 0, G = 1;
  bool f64 = false, wide = false;
  size_t lds = 0;
  size_t o_wide = 0, o_run = 0, o_part = 0, total = 0;
};

Plan make_plan(int dtype, int64_t N, int64_t B, int64_t D, int64_t max_points, int64_t max_samples, int flags) {
  Plan p;
  if (dtype != PYG_F32 && dtype != PYG_F64 && dtype != PYG_F16 && dtype != PYG_BF16) return p;
  if (N < 0 || N >= (1ll << 31) || B < 0 || B >= (1ll << 31) || D < 1 || D > kMaxD || max_points < 0 || max_samples < 0) return p;
  if (max_points >= (1ll << 31)) max_points = (1ll << 31) - 1;
  p.f64 = dtype == PYG_F64;
  p.wide = dtype == PYG_F16 || dtype == PYG_BF16;
  const size_t asz = p.f64 ? 8 : 4;
  const int force = flags & PYG_HIP_FPS_FORCE_MASK;
  int route = max_points > kCapacity ? PYG_HIP_FPS_ROUTE_STREAM : PYG_HIP_FPS_ROUTE_RESIDENT;
  if (B < kMultiExamples && max_points >= kMultiPoints) route = PYG_HIP_FPS_ROUTE_MULTI;
  if (force == PYG_HIP_FPS_FORCE_RESIDENT) route = max_points > kCapacity ? PYG_HIP_FPS_ROUTE_STREAM : PYG_HIP_FPS_ROUTE_RESIDENT;
  if (force == PYG_HIP_FPS_FORCE_STREAM) route = PYG_HIP_FPS_ROUTE_STREAM;
  if (force == PYG_HIP_FPS_FORCE_MULTI) route = PYG_HIP_FPS_ROUTE_MULTI;
  p.route = route;
  if (route == PYG_HIP_FPS_ROUTE_RESIDENT) {
    p.threads = kMinThreads;
    while ((int64_t)p.threads * kP < max_points) p.threads *= 2;
    const size_t slots = 2 * (size_t)(p.threads / 64);
    if (D <= 4) {
      p.shape = SHAPE_D4, p.lds = slots * (16 + 4 * asz);
    } else {
      const size_t copy = (size_t)max_points * D * asz;
      p.shape = copy <= (size_t)kGenLdsBytes ? SHAPE_LDS : SHAPE_GLOB;
      p.lds = slots * 16 + (p.shape == SHAPE_LDS ? copy : 0);
    }
  } else {
    p.shape = D <= 4 ? SHAPE_D4 : SHAPE_GLOB;
  }
  if (route == PYG_HIP_FPS_ROUTE_MULTI) {
    const int64_t shortest = force == PYG_HIP_FPS_FORCE_MULTI ? kSliceForced : kSliceMin;
    p.slice = (int)std::max<int64_t>(shortest, ceil_div(max_points, kMaxSlices));
    p.G = (int)std::max<int64_t>(1, ceil_div(max_points, p.slice));
  }
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += align_up(bytes ? bytes : 1, 256);
    return o;
  };
  p.o_wide = take(p.wide ? (size_t)N * D * 4 : 0);
  p.o_run = take(route != PYG_HIP_FPS_ROUTE_RESIDENT ? (size_t)N * asz : 0);
  p.o_part = take(route == PYG_HIP_FPS_ROUTE_MULTI ? (size_t)2 * B * p.G * 16 : 0);
  p.total = at;
  return p;
}

const char* shape_name(int shape) { return shape == SHAPE_D4 ? "d4" : shape == SHAPE_LDS ? "lds" : "glob"; }

void note_route(const Plan& p) {
  if (p.route == PYG_HIP_FPS_ROUTE_RESIDENT) snprintf(g_last_route, sizeof(g_last_route), "resident %s t%d", shape_name(p.shape), p.threads);
  else if (p.route == PYG_HIP_FPS_ROUTE_STREAM) snprintf(g_last_route, sizeof(g_last_route), "stream %s", shape_name(p.shape));
  else snprintf(g_last_route, sizeof(g_last_route), "multi %s g%d", shape_name(p.shape), p.G);
}

// the pinned word of this device a call leaves a bad pointer in (nearest's pattern; a word of fps's own)
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
    *static_cast<int*>(ptr) = 0;
    slots[dev] = static_cast<int*>(ptr);
  }
  *out = slots[dev];
  return PYG_HIP_OK;
}

template <typename A, int SHAPE, int T>
int launch_resident_t(const A* src, const FpsArgs& a, const Plan& p, hipStream_t stream) {
  const void* kern = reinterpret_cast<const void*>(&fps_resident_kernel<A, SHAPE, T>);
  if (p.lds > 48 * 1024)
    if (int rc = ensure_dynamic_lds(kern, kMaxLds)) return rc;
  hipLaunchKernelGGL((fps_resident_kernel<A, SHAPE, T>), dim3((unsigned)a.B), dim3(T), p.lds, stream, src, a);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

template <typename A, int SHAPE>
int launch_resident(const A* src, const FpsArgs& a, const Plan& p, hipStream_t stream) {
  switch (p.threads) {
    case 64: return launch_resident_t<A, SHAPE, 64>(src, a, p, stream);
    case 128: return launch_resident_t<A, SHAPE, 128>(src, a, p, stream);
    case 256: return launch_resident_t<A, SHAPE, 256>(src, a, p, stream);
    case 512: return launch_resident_t<A, SHAPE, 512>(src, a, p, stream);
    default: return launch_resident_t<A, SHAPE, 1024>(src, a, p, stream);
  }
}

template <typename A>
int run_fps(const A* src, const FpsArgs& a, const Plan& p, unsigned char* ws, hipStream_t stream) {
  A* run = reinterpret_cast<A*>(ws + p.o_run);
  if (p.route == PYG_HIP_FPS_ROUTE_RESIDENT) {
    if (p.shape == SHAPE_D4) return launch_resident<A, SHAPE_D4>(src, a, p, stream);
    if (p.shape == SHAPE_LDS) return launch_resident<A, SHAPE_LDS>(src, a, p, stream);
    return launch_resident<A, SHAPE_GLOB>(src, a, p, stream);
  }
  if (p.route == PYG_HIP_FPS_ROUTE_STREAM) {
    if (p.shape == SHAPE_D4) hipLaunchKernelGGL((fps_stream_kernel<A, true>), dim3((unsigned)a.B), dim3(kMaxThreads), 0, stream, src, run, a);
    else hipLaunchKernelGGL((fps_stream_kernel<A, false>), dim3((unsigned)a.B), dim3(kMaxThreads), 0, stream, src, run, a);
    PYG_HIP_CHECK(hipGetLastError());
    return PYG_HIP_OK;
  }
  Key<A>* part = reinterpret_cast<Key<A>*>(ws + p.o_part);
  const dim3 grid((unsigned)p.G, (unsigned)a.B);
  for (int64_t it = 0; it < a.max_samples; ++it) {
    if (p.shape == SHAPE_D4) hipLaunchKernelGGL((fps_multi_kernel<A, true>), grid, dim3(kMultiThreads), 0, stream, src, run, part, p.slice, (int)it, a);
    else hipLaunchKernelGGL((fps_multi_kernel<A, false>), grid, dim3(kMultiThreads), 0, stream, src, run, part, p.slice, (int)it, a);
  }
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

// ---- grid_cluster, host ----
struct GridPlan {
  bool ok = false, reduce = false;
  int G = 0;
  int64_t rows_per_block = 0;
  size_t total = 0;
};

GridPlan make_grid_plan(int dtype, int64_t N, int64_t D, bool have_start, bool have_end) {
  GridPlan p;
  if (dtype != PYG_F32 && dtype != PYG_F64 && dtype != PYG_F16 && dtype != PYG_BF16) return p;
  if (N < 0 || D < 1 || D > kMaxD) return p;
  p.ok = true;
  p.reduce = !(have_start && have_end) && N > 0;
  if (p.reduce) {
    p.rows_per_block = ceil_div(N, kMinMaxBlocks);
    p.G = (int)ceil_div(N, p.rows_per_block);
    p.total = align_up((size_t)2 * p.G * D * (dtype == PYG_F64 ? 8 : 4), 256);
  }
  return p;
}

template <typename T>
int run_grid(const GridPlan& p, const void* pos_, int64_t N, int64_t D, const void* size, const void* start, const void* end, void* ws,
             int64_t* out, hipStream_t stream) {
  using A = typename Math<T>::acc_t;
  const T* pos = static_cast<const T*>(pos_);
  A* partial = p.reduce ? static_cast<A*>(ws) : nullptr;
  if (p.reduce) {
    hipLaunchKernelGGL((minmax_kernel<T>), dim3((unsigned)p.G), dim3(kGridThreads), 0, stream, pos, N, (int)D, p.rows_per_block, partial);
    PYG_HIP_CHECK(hipGetLastError());
  }
  const unsigned blocks = (unsigned)ceil_div(N, kGridThreads * kGridPoints);
  if (D <= 4) {
    hipLaunchKernelGGL((cluster_kernel<T, true>), dim3(blocks), dim3(kGridThreads), 0, stream, pos, N, (int)D, static_cast<const T*>(size),
                       static_cast<const T*>(start), static_cast<const T*>(end), partial, p.G, out);
  } else {
    const size_t lds = (size_t)D * (8 + 2 * sizeof(A));
    const void* kern = reinterpret_cast<const void*>(&cluster_kernel<T, false>);
    if (lds > 48 * 1024)
      if (int rc = ensure_dynamic_lds(kern, kMaxLds)) return rc;
    hipLaunchKernelGGL((cluster_kernel<T, false>), dim3(blocks), dim3(kGridThreads), lds, stream, pos, N, (int)D, static_cast<const T*>(size),
                       static_cast<const T*>(start), static_cast<const T*>(end), partial, p.G, out);
  }
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

}  // namespace
}  // namespace pyg_hip

using namespace pyg_hip;

extern "C" {

int pyg_hip_fps_route(int dtype, int64_t B, int64_t D, int64_t max_points, int64_t max_samples, int flags) {
  return make_plan(dtype, 0, B, D, max_points, max_samples, flags).route;
}

const char* pyg_hip_fps_last_route(void) { return g_last_route; }

int pyg_hip_fps_tile(int which) {
  switch (which) {
    case PYG_HIP_FPS_TILE_POINTS: return kP;
    case PYG_HIP_FPS_TILE_MIN_THREADS: return kMinThreads;
    case PYG_HIP_FPS_TILE_MAX_THREADS: return kMaxThreads;
    case PYG_HIP_FPS_TILE_SLICE_FORCED: return kSliceForced;
    case PYG_HIP_FPS_TILE_LDS_BYTES: return kGenLdsBytes;
    case PYG_HIP_FPS_TILE_MULTI_POINTS: return (int)kMultiPoints;
    case PYG_HIP_FPS_TILE_MULTI_EXAMPLES: return (int)kMultiExamples;
    case PYG_HIP_FPS_TILE_SLICE: return kSliceMin;
    default: return 0;
  }
}

size_t pyg_hip_fps_workspace_size(int dtype, int64_t N, int64_t B, int64_t D, int64_t max_points, int64_t max_samples, int flags) {
  const Plan p = make_plan(dtype, N, B, D, max_points, max_samples, flags);
  return p.route == PYG_HIP_FPS_ROUTE_UNSUPPORTED ? 0 : p.total;
}

int pyg_hip_fps(int dtype, const void* src, int64_t N, int64_t D, const int64_t* ptr, int64_t B, const int64_t* out_ptr,
                const int64_t* start, int64_t max_points, int64_t max_samples, int flags, void* workspace, size_t workspace_bytes,
                int64_t* out, int64_t out_total, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PYG_HIP_REQUIRE(dtype == PYG_F32 || dtype == PYG_F64 || dtype == PYG_F16 || dtype == PYG_BF16,
                  "fps: src must be float32, float64, float16 or bfloat16 (dtype code %d)", dtype);
  PYG_HIP_REQUIRE(N >= 0 && B >= 0 && max_points >= 0 && max_samples >= 0 && out_total >= 0, "fps: negative size");
  PYG_HIP_REQUIRE(D >= 1, "fps: the feature dimension must be at least 1 (got %lld)", (long long)D);
  if (N >= (1ll << 31) || B >= (1ll << 31) || D > kMaxD)
    return fail(PYG_HIP_ERR_UNSUPPORTED, "fps: 2^31 or more points, or more than %lld features: indices are 32-bit here", (long long)kMaxD);
  PYG_HIP_REQUIRE(ptr != nullptr, "fps: NULL ptr");
  PYG_HIP_REQUIRE(out_ptr != nullptr || B == 0, "fps: NULL out_ptr");
  PYG_HIP_REQUIRE(src != nullptr || N == 0, "fps: NULL src");
  PYG_HIP_REQUIRE(out != nullptr || out_total == 0, "fps: NULL out");
  const Plan p = make_plan(dtype, N, B, D, max_points, max_samples, flags);
  if (p.route == PYG_HIP_FPS_ROUTE_UNSUPPORTED) return fail(PYG_HIP_ERR_UNSUPPORTED, "fps: no kernel for these arguments");
  PYG_HIP_REQUIRE(workspace != nullptr, "fps: NULL workspace");
  if (workspace_bytes < p.total)
    return fail(PYG_HIP_ERR_WORKSPACE, "fps: workspace of %zu bytes, %zu needed (pyg_hip_fps_workspace_size)", workspace_bytes, p.total);
  PYG_HIP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "fps: the workspace must be 16-byte aligned");
  int* slot = nullptr;
  if (int rc = deferred_slot(&slot)) return rc;
  if (*static_cast<volatile int*>(slot) != 0) {
    *static_cast<volatile int*>(slot) = 0;
    return fail(PYG_HIP_ERR_INVALID, "fps: an earlier call on this device had a ptr that was not non-decreasing from 0 to the number of "
                                     "rows, or sizes smaller than its examples (its result is unspecified)");
  }
  note_route(p);
  if (B == 0 || max_samples == 0 || out_total == 0) return PYG_HIP_OK;
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  FpsArgs a{ptr, out_ptr, start, N, B, out_total, std::min<int64_t>(max_points, (1ll << 31) - 1), std::min<int64_t>(max_samples, (1ll << 31) - 1),
            (int)D, out, slot};
  if (p.wide && N > 0) {
    float* wide = reinterpret_cast<float*>(ws + p.o_wide);
    const int64_t ne = N * D;
    const unsigned g = (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(ne, 256), 1), 4096);
    if (dtype == PYG_F16) hipLaunchKernelGGL((widen_kernel<f16_t>), dim3(g), dim3(256), 0, stream, static_cast<const f16_t*>(src), wide, ne);
    else hipLaunchKernelGGL((widen_kernel<bf16_t>), dim3(g), dim3(256), 0, stream, static_cast<const bf16_t*>(src), wide, ne);
    PYG_HIP_CHECK(hipGetLastError());
    src = wide;
  }
  return p.f64 ? run_fps<double>(static_cast<const double*>(src), a, p, ws, stream) : run_fps<float>(static_cast<const float*>(src), a, p, ws, stream);
}

int pyg_hip_fps_pending_error(void) {
  int* slot = nullptr;
  if (deferred_slot(&slot) != PYG_HIP_OK) return PYG_HIP_ERR_RUNTIME;
  const int pending = *static_cast<volatile int*>(slot);
  *static_cast<volatile int*>(slot) = 0;
  return pending;
}

size_t pyg_hip_grid_cluster_workspace_size(int dtype, int64_t N, int64_t D, int have_start, int have_end) {
  return make_grid_plan(dtype, N, D, have_start != 0, have_end != 0).total;
}

int pyg_hip_grid_cluster(int dtype, const void* pos, int64_t N, int64_t D, const void* size, const void* start, const void* end,
                         void* workspace, size_t workspace_bytes, int64_t* out, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PYG_HIP_REQUIRE(dtype == PYG_F32 || dtype == PYG_F64 || dtype == PYG_F16 || dtype == PYG_BF16,
                  "grid_cluster: pos must be float32, float64, float16 or bfloat16 (dtype code %d)", dtype);
  PYG_HIP_REQUIRE(N >= 0, "grid_cluster: negative size");
  PYG_HIP_REQUIRE(D >= 1, "grid_cluster: the feature dimension must be at least 1 (got %lld)", (long long)D);
  if (D > kMaxD) return fail(PYG_HIP_ERR_UNSUPPORTED, "grid_cluster: more than %lld features", (long long)kMaxD);
  PYG_HIP_REQUIRE(size != nullptr, "grid_cluster: NULL size");
  PYG_HIP_REQUIRE((pos != nullptr && out != nullptr) || N == 0, "grid_cluster: NULL pos or out");
  const GridPlan p = make_grid_plan(dtype, N, D, start != nullptr, end != nullptr);
  if (N == 0) return PYG_HIP_OK;
  if (p.reduce) {
    PYG_HIP_REQUIRE(workspace != nullptr, "grid_cluster: NULL workspace");
    if (workspace_bytes < p.total)
      return fail(PYG_HIP_ERR_WORKSPACE, "grid_cluster: workspace of %zu bytes, %zu needed (pyg_hip_grid_cluster_workspace_size)",
                  workspace_bytes, p.total);
    PYG_HIP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "grid_cluster: the workspace must be 16-byte aligned");
  }
  switch (dtype) {
    case PYG_F32: return run_grid<float>(p, pos, N, D, size, start, end, workspace, out, stream);
    case PYG_F64: return run_grid<double>(p, pos, N, D, size, start, end, workspace, out, stream);
    case PYG_F16: return run_grid<f16_t>(p, pos, N, D, size, start, end, workspace, out, stream);
    default: return run_grid<bf16_t>(p, pos, N, D, size, start, end, workspace, out, stream);
  }
}

}  // extern "C"
