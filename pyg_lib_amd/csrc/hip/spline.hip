// spline_basis / spline_weighting for gfx950 (MI355X): the six pyg::spline_* operators behind SplineConv.
//
// Replaces pyg_lib/csrc/ops/cpu/spline_kernel.cpp and ops/cuda/spline_kernel.cu.  VALU kernels whose design constraint is
// exactness: every sum is sequential in the order include/pyg_hip.h states, no fused multiply-add, no atomics, so every route,
// every call and the CPU key give the same bits (float32 / float64; bfloat16 accumulates in fp32 and rounds once).
//   basis             one thread per (e, s) / (e, d); kernel_size and is_open_spline are read on the device
//   weighting family  ONE kernel template (forward, backward_x, backward_basis): a 256-thread workgroup owns a tile of edges,
//                     lanes run along the contiguous axis of W, the tile's rows / basis / weight_index go through LDS;
//                     route `global` reads the weights through L2; route `lds` (forced only: measured slower) stages the
//                     whole weight tensor into LDS once per persistent workgroup
//   backward_weight   stable index sort of the pairs by weight index, then (weight, chunk, 64 x 64 tile) work items with
//                     register accumulators; weights longer than one chunk go through per-chunk slabs added in chunk order
#pragma clang fp contract(off)
#include "common.h"
#include "elem.h"

#include <algorithm>
#include <mutex>

namespace pyg_hip {
namespace {

constexpr int kThreads = 256;
constexpr int kLdsWeightBytes = 128 * 1024;   // route lds: the weight tensor fits this
constexpr int kLdsTileBytes = 28 * 1024;      // the edge tile of every route
constexpr int kMaxLds = 160 * 1024;
constexpr int kChunk = 1024;                  // backward_weight: sorted pairs per work item
constexpr int kDwTile = 64;                   // backward_weight: a work item's tile of the M_in x M_out matrix
constexpr int kDwBatch = 16;                  // backward_weight: pairs staged through LDS at a time
constexpr int kMaxDims = 16;                  // basis: (degree + 1)^D has to fit an int

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- basis ----------------------------------------------------------------------------------------------------------------
// The polynomial pieces with the operand types of the reference (double literals against a scalar_t `v`): what is evaluated
// in double and rounded once, and what stays in scalar_t, follows from the C++ promotion rules exactly as there.
template <typename T, int DEG>
__device__ inline T piece(T v, int64_t k_mod) {
  if (DEG == 1) {
    return 1. - v - k_mod + 2. * v * k_mod;
  } else if (DEG == 2) {
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

template <typename T, int DEG>
__device__ inline T piece_grad(T v, int64_t k_mod) {
  if (DEG == 1) {
    return 2 * k_mod - 1;
  } else if (DEG == 2) {
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

template <typename T>
__device__ inline T fract(T v) {
  v -= floor(v);
  return v;
}

template <typename T, int DEG>
__global__ __launch_bounds__(kThreads) void basis_kernel(const T* __restrict__ pseudo, const int64_t* __restrict__ kernel_size,
                                                         const uint8_t* __restrict__ is_open, int64_t E, int D, int64_t S,
                                                         T* __restrict__ basis, int64_t* __restrict__ weight_index) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= E * S) return;
  const int64_t e = i / S;
  int64_t k = i % S, wi = 0, offset = 1;
  T b = (T)1.;
  for (int d = 0; d < D; ++d) {
    const int64_t k_mod = k % (DEG + 1);
    k /= DEG + 1;
    const int64_t size = kernel_size[d];
    T v = pseudo[e * D + d];
    v *= size - DEG * (int64_t)is_open[d];
    // the C remainder of the truncated value, as the reference: a pseudo outside [0, 1] can give a negative index (size 0: 0)
    wi += (size != 0 ? ((int64_t)v + k_mod) % size : 0) * offset;
    offset *= size;
    v = fract(v);
    v = piece<T, DEG>(v, k_mod);
    b *= v;
  }
  basis[i] = b;
  weight_index[i] = wi;
}

template <typename T, int DEG>
__global__ __launch_bounds__(kThreads) void basis_backward_kernel(const T* __restrict__ grad_basis, const T* __restrict__ pseudo,
                                                                  const int64_t* __restrict__ kernel_size,
                                                                  const uint8_t* __restrict__ is_open, int64_t E, int D, int64_t S,
                                                                  T* __restrict__ grad_pseudo) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= E * D) return;
  const int64_t e = i / D;
  const int d = (int)(i % D);
  int64_t pw[kMaxDims];   // (degree + 1)^d
  pw[0] = 1;
  for (int j = 1; j < kMaxDims; ++j) pw[j] = j < D ? pw[j - 1] * (DEG + 1) : 0;
  T g = (T)0.;
  for (int64_t s = 0; s < S; ++s) {
    int64_t k_mod = (s / pw[d]) % (DEG + 1);
    T v = pseudo[e * D + d];
    v *= kernel_size[d] - DEG * (int64_t)is_open[d];
    v = fract(v);
    v = piece_grad<T, DEG>(v, k_mod);
    T tmp = v;
    for (int d_it = 1; d_it < D; ++d_it) {
      const int d_new = d_it - (d >= d_it);
      k_mod = (s / pw[d_new]) % (DEG + 1);
      v = pseudo[e * D + d_new];
      v *= kernel_size[d_new] - DEG * (int64_t)is_open[d_new];
      v = fract(v);
      v = piece<T, DEG>(v, k_mod);
      tmp *= v;
    }
    g += tmp * grad_basis[e * S + s];
  }
  g *= kernel_size[d] - DEG * (int64_t)is_open[d];
  grad_pseudo[i] = g;
}

// ---- weighting: forward, backward_x, backward_basis -----------------------------------------------------------------------
// W is seen as [K, R, A]: A the contiguous axis the lanes run along, R the axis a lane loops over.
//   FWD  A = M_out, R = M_in : out[e, a]  = sum_s sum_r W[wi, r, a] * (b[e, s] * x[e, r])
//   BX   A = M_in,  R = M_out: gx[e, a]   = sum_r sum_s (g[e, r] * b[e, s]) * Wt[wi, r, a]        (Wt: the transposed copy)
//   BB   A = M_out, R = M_in : gb[e, s]   = sum_a g[e, a] * (sum_r W[wi, r, a] * x[e, r])
enum { MODE_FWD = 0, MODE_BX = 1, MODE_BB = 2 };

struct WeightingArgs {
  const void* rows;     // [E, R]: x (FWD, BB), grad_out (BX)
  const void* grad;     // [E, A]: grad_out (BB)
  const void* weight;   // [K, R, A]
  const void* basis;    // [E, S] (FWD, BX)
  const int64_t* weight_index;
  void* out;
  int64_t E, K, tiles;
  int S, R, A;
  int TX, TE, SB;       // lanes per edge, edges per tile, basis columns per pass (BB)
  int* slot;
};

template <typename T, int MODE, bool LDSW>
__global__ __launch_bounds__(kThreads) void weighting_kernel(const WeightingArgs a) {
  using A_t = typename Math<T>::acc_t;
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x;
  const int S = a.S, R = a.R, A = a.A, TE = a.TE;
  const size_t w_elems = (size_t)a.K * R * A;
  const size_t w_bytes = LDSW ? (w_elems * sizeof(T) + 15) / 16 * 16 : 0;
  T* const wl = reinterpret_cast<T*>(smem);
  A_t* const rows = reinterpret_cast<A_t*>(smem + w_bytes);                          // [TE, R]
  A_t* const bs = rows + (size_t)TE * R;                                             // [TE, S]   (FWD, BX)
  A_t* const gs = bs + (MODE == MODE_BB ? 0 : (size_t)TE * S);                       // [TE, A]   (BB)
  A_t* const prod = gs + (MODE == MODE_BB ? (size_t)TE * A : 0);                     // [TE, SB, A] (BB)
  int* const wis = reinterpret_cast<int*>(prod + (MODE == MODE_BB ? (size_t)TE * a.SB * A : 0));   // [TE, S]
  const T* const wg = static_cast<const T*>(a.weight);
  if (LDSW) {
    for (size_t i = tid; i < w_elems; i += kThreads) wl[i] = wg[i];
  }
  const int le = tid / a.TX, lane = tid % a.TX;
  const T* const rows_g = static_cast<const T*>(a.rows);
  const T* const grad_g = static_cast<const T*>(a.grad);
  const T* const basis_g = static_cast<const T*>(a.basis);
  T* const out = static_cast<T*>(a.out);
  for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const int64_t e0 = tile * TE;
    const int ne = (int)((a.E - e0) < (int64_t)TE ? (a.E - e0) : (int64_t)TE);
    __syncthreads();   // the previous tile has been consumed (and, first, W is staged)
    for (int i = tid; i < ne * R; i += kThreads) rows[i] = Math<T>::up(rows_g[e0 * R + i]);
    for (int i = tid; i < ne * S; i += kThreads) {
      if (MODE != MODE_BB) bs[i] = Math<T>::up(basis_g[e0 * S + i]);
      const int64_t k = a.weight_index[e0 * S + i];
      const bool ok = k >= 0 && k < a.K;
      wis[i] = ok ? (int)k : -1;
      if (!ok) *a.slot = 1;
    }
    if (MODE == MODE_BB)
      for (int i = tid; i < ne * A; i += kThreads) gs[i] = Math<T>::up(grad_g[e0 * A + i]);
    __syncthreads();
    if (MODE == MODE_FWD) {
      if (le < ne)
        for (int c = lane; c < A; c += a.TX) {
          A_t acc = 0;
          for (int s = 0; s < S; ++s) {
            const int k = wis[le * S + s];
            if (k < 0) continue;
            const A_t b = bs[le * S + s];
            const size_t base = (size_t)k * R * A + c;
            for (int r = 0; r < R; ++r) {
              const A_t w = Math<T>::up(LDSW ? wl[base + (size_t)r * A] : wg[base + (size_t)r * A]);
              acc = acc + w * (b * rows[le * R + r]);
            }
          }
          out[(e0 + le) * A + c] = Math<T>::down(acc);
        }
    } else if (MODE == MODE_BX) {
      if (le < ne)
        for (int c = lane; c < A; c += a.TX) {
          A_t acc = 0;
          for (int r = 0; r < R; ++r) {
            const A_t g = rows[le * R + r];
            for (int s = 0; s < S; ++s) {
              const int k = wis[le * S + s];
              if (k < 0) continue;
              const size_t at = (size_t)k * R * A + (size_t)r * A + c;
              const A_t w = Math<T>::up(LDSW ? wl[at] : wg[at]);
              acc = acc + (g * bs[le * S + s]) * w;
            }
          }
          out[(e0 + le) * A + c] = Math<T>::down(acc);
        }
    } else {
      for (int s0 = 0; s0 < S; s0 += a.SB) {
        const int sb = S - s0 < a.SB ? S - s0 : a.SB;
        if (le < ne)
          for (int c = lane; c < A; c += a.TX)
            for (int sj = 0; sj < sb; ++sj) {
              const int k = wis[le * S + s0 + sj];
              A_t p = 0;
              if (k >= 0) {
                A_t t = 0;
                const size_t base = (size_t)k * R * A + c;
                for (int r = 0; r < R; ++r) {
                  const A_t w = Math<T>::up(LDSW ? wl[base + (size_t)r * A] : wg[base + (size_t)r * A]);
                  t = t + w * rows[le * R + r];
                }
                p = gs[le * A + c] * t;
              }
              prod[((size_t)le * a.SB + sj) * A + c] = p;
            }
        __syncthreads();
        // one lane per (e, s): the products in m_out order
        for (int i = tid; i < ne * sb; i += kThreads) {
          const int e = i / sb, sj = i % sb;
          A_t gb = 0;
          for (int c = 0; c < A; ++c) gb = gb + prod[((size_t)e * a.SB + sj) * A + c];
          out[(e0 + e) * S + s0 + sj] = Math<T>::down(gb);
        }
        __syncthreads();
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void transpose_kernel(const T* __restrict__ w, T* __restrict__ wt, int64_t K, int M_in,
                                                             int M_out) {
  // wt[k, j, i] = w[k, i, j]
  const int64_t total = K * M_in * M_out;
  for (int64_t o = (int64_t)blockIdx.x * kThreads + threadIdx.x; o < total; o += (int64_t)gridDim.x * kThreads) {
    const int i = (int)(o % M_in);
    const int64_t q = o / M_in;
    const int j = (int)(q % M_out);
    const int64_t k = q / M_out;
    wt[o] = w[(k * M_in + i) * M_out + j];
  }
}

// ---- backward_weight ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void dw_keys_kernel(const int64_t* __restrict__ weight_index, int64_t n, int64_t K,
                                                           int64_t* __restrict__ keys) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int64_t k = weight_index[i];
    keys[i] = (k >= 0 && k < K) ? k : K;   // bucket K: nobody reads it
  }
}

__device__ inline int64_t lower_bound(const int64_t* keys, int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// One workgroup: row_start [K + 1] (first sorted position of every weight), item_start [K + 1] (running count of work items:
// max(1, ceil(len / chunk)) per weight, so that a weight without pairs still gets its zeros written) and slab_start [K + 1]
// (running count of the slabs: the chunks of the weights that have more than one).
__global__ __launch_bounds__(kThreads) void dw_plan_kernel(const int64_t* __restrict__ sorted_keys, int64_t n, int64_t K, int chunk,
                                                           int64_t* __restrict__ row_start, int64_t* __restrict__ item_start,
                                                           int64_t* __restrict__ slab_start, int* slot) {
  __shared__ int64_t part_items[kThreads], part_slabs[kThreads];
  const int tid = threadIdx.x;
  const int64_t per = (K + kThreads - 1) / kThreads;
  const int64_t k0 = tid * per < K ? tid * per : K, k1 = k0 + per < K ? k0 + per : K;
  int64_t items = 0, slabs = 0;
  int64_t lo = k0 < k1 ? lower_bound(sorted_keys, n, k0) : 0;
  for (int64_t k = k0; k < k1; ++k) {
    const int64_t hi = lower_bound(sorted_keys, n, k + 1);
    const int64_t chunks = hi - lo > chunk ? (hi - lo + chunk - 1) / chunk : 1;
    items += chunks;
    slabs += chunks > 1 ? chunks : 0;
    lo = hi;
  }
  part_items[tid] = items, part_slabs[tid] = slabs;
  __syncthreads();
  if (tid == 0) {
    int64_t ri = 0, rs = 0;
    for (int t = 0; t < kThreads; ++t) {
      const int64_t ci = part_items[t], cs = part_slabs[t];
      part_items[t] = ri, part_slabs[t] = rs;
      ri += ci, rs += cs;
    }
    item_start[K] = ri, slab_start[K] = rs;
    const int64_t bad = lower_bound(sorted_keys, n, K);
    row_start[K] = bad;
    if (bad < n) *slot = 1;
  }
  __syncthreads();
  items = part_items[tid], slabs = part_slabs[tid];
  lo = k0 < k1 ? lower_bound(sorted_keys, n, k0) : 0;
  for (int64_t k = k0; k < k1; ++k) {
    const int64_t hi = lower_bound(sorted_keys, n, k + 1);
    const int64_t chunks = hi - lo > chunk ? (hi - lo + chunk - 1) / chunk : 1;
    row_start[k] = lo, item_start[k] = items, slab_start[k] = slabs;
    items += chunks;
    slabs += chunks > 1 ? chunks : 0;
    lo = hi;
  }
}

struct DwArgs {
  const void* grad_out;   // [E, M_out]
  const void* x;          // [E, M_in]
  const void* basis;      // [E * S]
  const int64_t* order;   // [n] pair positions, stably sorted by weight index
  const int64_t* row_start;
  const int64_t* item_start;
  const int64_t* slab_start;
  void* grad_weight;      // [K, M_in, M_out]
  void* slabs;            // [slab, M_in, M_out] in the accumulator type
  int64_t n, K;
  int S, M_in, M_out, chunk, tiles_out;
};

template <typename T>
__global__ __launch_bounds__(kThreads) void dw_kernel(const DwArgs a) {
  using A_t = typename Math<T>::acc_t;
  __shared__ A_t gsm[kDwBatch][kDwTile], xsm[kDwBatch][kDwTile], bsm[kDwBatch];
  const int64_t item = blockIdx.x;
  if (item >= a.item_start[a.K]) return;
  // the weight of this item: the last k with item_start[k] <= item
  int64_t lo_k = 0, hi_k = a.K;
  while (hi_k - lo_k > 1) {
    const int64_t mid = lo_k + (hi_k - lo_k) / 2;
    if (a.item_start[mid] <= item) lo_k = mid;
    else hi_k = mid;
  }
  const int64_t k = lo_k;
  const int64_t chunk_id = item - a.item_start[k], chunks = a.item_start[k + 1] - a.item_start[k];
  const int64_t row_end = a.row_start[k + 1];
  const int64_t lo = a.row_start[k] + chunk_id * a.chunk;
  const int64_t hi = lo + a.chunk < row_end ? lo + a.chunk : row_end;
  const int i0 = (int)(blockIdx.y / a.tiles_out) * kDwTile, j0 = (int)(blockIdx.y % a.tiles_out) * kDwTile;
  const int tid = threadIdx.x, ty = tid / 16, tx = tid % 16;
  const T* const g = static_cast<const T*>(a.grad_out);
  const T* const x = static_cast<const T*>(a.x);
  const T* const basis = static_cast<const T*>(a.basis);
  A_t acc[4][4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) acc[i][j] = 0;
  for (int64_t p0 = lo; p0 < hi; p0 += kDwBatch) {
    const int nb = (int)(hi - p0 < kDwBatch ? hi - p0 : kDwBatch);
    __syncthreads();
    if (ty < nb) {
      const int64_t pos = a.order[p0 + ty];
      const int64_t e = pos / a.S;
      for (int q = 0; q < 4; ++q) {
        const int c = tx + 16 * q;
        gsm[ty][c] = j0 + c < a.M_out ? Math<T>::up(g[e * a.M_out + j0 + c]) : A_t(0);
        xsm[ty][c] = i0 + c < a.M_in ? Math<T>::up(x[e * a.M_in + i0 + c]) : A_t(0);
      }
      if (tx == 0) bsm[ty] = Math<T>::up(basis[pos]);
    }
    __syncthreads();
    for (int p = 0; p < nb; ++p) {
      const A_t b = bsm[p];
      A_t gb[4];
      for (int j = 0; j < 4; ++j) gb[j] = gsm[p][tx + 16 * j] * b;
      for (int i = 0; i < 4; ++i) {
        const A_t xv = xsm[p][ty + 16 * i];
        for (int j = 0; j < 4; ++j) acc[i][j] = acc[i][j] + gb[j] * xv;
      }
    }
  }
  const size_t mat = (size_t)a.M_in * a.M_out;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      const int mi = i0 + ty + 16 * i, mo = j0 + tx + 16 * j;
      if (mi >= a.M_in || mo >= a.M_out) continue;
      if (chunks == 1) static_cast<T*>(a.grad_weight)[(size_t)k * mat + (size_t)mi * a.M_out + mo] = Math<T>::down(acc[i][j]);
      else static_cast<A_t*>(a.slabs)[(size_t)(a.slab_start[k] + chunk_id) * mat + (size_t)mi * a.M_out + mo] = acc[i][j];
    }
}

// the weights of more than one chunk: their slabs in chunk order
template <typename T>
__global__ __launch_bounds__(kThreads) void dw_reduce_kernel(const DwArgs a) {
  using A_t = typename Math<T>::acc_t;
  const int64_t k = blockIdx.y;
  const int64_t chunks = a.item_start[k + 1] - a.item_start[k];
  if (chunks <= 1) return;
  const size_t mat = (size_t)a.M_in * a.M_out;
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= mat) return;
  const A_t* slab = static_cast<const A_t*>(a.slabs) + (size_t)a.slab_start[k] * mat + i;
  A_t acc = 0;
  for (int64_t c = 0; c < chunks; ++c) acc = acc + slab[(size_t)c * mat];
  static_cast<T*>(a.grad_weight)[(size_t)k * mat + i] = Math<T>::down(acc);
}

// ---- host -------------------------------------------------------------------------------------------------------------
thread_local char g_last_route[64] = "none";

size_t elem_size(int dtype) { return dtype == PYG_F64 ? 8 : dtype == PYG_F32 ? 4 : 2; }
size_t acc_size(int dtype) { return dtype == PYG_F64 ? 8 : 4; }
bool weighting_dtype(int dtype) { return dtype == PYG_F32 || dtype == PYG_F64 || dtype == PYG_BF16; }

// the pure part of the dispatch: what pyg_hip_spline_route answers and the weighting family follows
int choose_route(int dtype, int64_t E, int64_t S, int64_t M_in, int64_t M_out, int64_t K, int force) {
  if (!weighting_dtype(dtype) || E < 0 || S < 0 || M_in < 0 || M_out < 0 || K < 0) return PYG_HIP_SPLINE_ROUTE_UNSUPPORTED;
  if (K >= (1ll << 31) || S >= (1ll << 20) || M_in >= (1ll << 20) || M_out >= (1ll << 20)) return PYG_HIP_SPLINE_ROUTE_UNSUPPORTED;
  const bool fits = (double)K * (double)M_in * (double)M_out * (double)elem_size(dtype) <= (double)kLdsWeightBytes;
  if (force == PYG_HIP_SPLINE_FORCE_GLOBAL) return PYG_HIP_SPLINE_ROUTE_GLOBAL;
  if (force == PYG_HIP_SPLINE_FORCE_LDS) return fits ? PYG_HIP_SPLINE_ROUTE_LDS : PYG_HIP_SPLINE_ROUTE_GLOBAL;
  // measured: lds loses to global at every edge count, so the rule never takes it; it stays a forced route
  return PYG_HIP_SPLINE_ROUTE_GLOBAL;
}

struct TilePlan {
  bool ok = false;
  int TX = 0, TE = 0, SB = 0;
  size_t tile_bytes = 0;
};

// A: the lane axis, R: the loop axis (see the kernel)
TilePlan make_tile(int mode, int dtype, int64_t S, int64_t R, int64_t A) {
  TilePlan p;
  const size_t asz = acc_size(dtype);
  int tx = 8;
  while (tx < kThreads && tx < A) tx *= 2;
  p.TX = tx;
  size_t per_edge = (size_t)R * asz + (size_t)S * 4;
  if (mode == MODE_BB) per_edge += (size_t)A * asz;
  else per_edge += (size_t)S * asz;
  size_t budget = kLdsTileBytes;
  if (mode == MODE_BB) {
    // at least one basis column of products per edge
    if (per_edge + (size_t)A * asz > budget) return p;
    const size_t sb = std::min<size_t>((size_t)std::max<int64_t>(S, 1), (budget - per_edge) / std::max<size_t>((size_t)A * asz, 1));
    p.SB = (int)std::max<size_t>(sb, 1);
    per_edge += (size_t)p.SB * A * asz;
  }
  if (per_edge > budget) return p;
  p.TE = (int)std::min<size_t>((size_t)(kThreads / tx), budget / std::max<size_t>(per_edge, 1));
  if (p.TE < 1) return p;
  if (mode == MODE_BB) {
    // with fewer edges than planned the pass can be wider
    const size_t fixed = (size_t)R * asz + (size_t)S * 4 + (size_t)A * asz;
    const size_t sb = (budget / p.TE - fixed) / std::max<size_t>((size_t)A * asz, 1);
    p.SB = (int)std::min<size_t>(std::max<size_t>(sb, (size_t)p.SB), (size_t)std::max<int64_t>(S, 1));
    per_edge = fixed + (size_t)p.SB * A * asz;
  }
  p.tile_bytes = (per_edge * p.TE + 15) / 16 * 16;
  p.ok = true;
  return p;
}

// the pinned word of this device a call leaves a bad weight index in (nearest's pattern; a word of the spline family's own)
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

// raises what an earlier call left, and hands out the word
int take_slot(const char* op, int** slot) {
  if (int rc = deferred_slot(slot)) return rc;
  if (*static_cast<volatile int*>(*slot) != 0) {
    *static_cast<volatile int*>(*slot) = 0;
    return fail(PYG_HIP_ERR_INVALID, "%s: an earlier spline call on this device had a weight_index outside [0, kernel_size) "
                                     "(such pairs contributed nothing)", op);
  }
  return PYG_HIP_OK;
}

template <typename T, int MODE>
int launch_weighting(const WeightingArgs& a, int route, size_t tile_bytes, hipStream_t stream) {
  if (route == PYG_HIP_SPLINE_ROUTE_LDS) {
    const size_t w_bytes = ((size_t)a.K * a.R * a.A * sizeof(T) + 15) / 16 * 16;
    const size_t lds = w_bytes + tile_bytes;
    const void* kern = reinterpret_cast<const void*>(&weighting_kernel<T, MODE, true>);
    if (lds > 48 * 1024)
      if (int rc = ensure_dynamic_lds(kern, kMaxLds)) return rc;
    const unsigned grid = (unsigned)std::min<int64_t>(a.tiles, std::max(device_info().num_cus, 1));
    hipLaunchKernelGGL((weighting_kernel<T, MODE, true>), dim3(grid), dim3(kThreads), lds, stream, a);
  } else {
    const unsigned grid = (unsigned)std::min<int64_t>(a.tiles, (int64_t)1 << 20);
    hipLaunchKernelGGL((weighting_kernel<T, MODE, false>), dim3(grid), dim3(kThreads), tile_bytes, stream, a);
  }
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

template <int MODE>
int launch_weighting_dtype(int dtype, const WeightingArgs& a, int route, size_t tile_bytes, hipStream_t stream) {
  switch (dtype) {
    case PYG_F32: return launch_weighting<float, MODE>(a, route, tile_bytes, stream);
    case PYG_F64: return launch_weighting<double, MODE>(a, route, tile_bytes, stream);
    default: return launch_weighting<bf16_t, MODE>(a, route, tile_bytes, stream);
  }
}

const char* mode_name(int mode) { return mode == MODE_FWD ? "forward" : mode == MODE_BX ? "backward_x" : "backward_basis"; }

// the common front of the three operators of the template
int run_weighting(int mode, const char* op, int dtype, const void* rows, const void* grad, const void* weight, const void* basis,
                  const int64_t* weight_index, int64_t E, int64_t S, int64_t M_in, int64_t M_out, int64_t K, int flags, void* out,
                  hipStream_t stream) {
  const int64_t A = mode == MODE_BX ? M_in : M_out, R = mode == MODE_BX ? M_out : M_in;
  const int route = choose_route(dtype, E, S, M_in, M_out, K, flags & PYG_HIP_SPLINE_FORCE_MASK);
  if (route == PYG_HIP_SPLINE_ROUTE_UNSUPPORTED) return fail(PYG_HIP_ERR_UNSUPPORTED, "%s: no kernel for these sizes", op);
  const TilePlan t = make_tile(mode, dtype, S, R, A);
  if (!t.ok) return fail(PYG_HIP_ERR_UNSUPPORTED, "%s: an edge's rows (S = %lld, M_in = %lld, M_out = %lld) exceed the %d-byte LDS tile",
                         op, (long long)S, (long long)M_in, (long long)M_out, kLdsTileBytes);
  int* slot = nullptr;
  if (int rc = take_slot(op, &slot)) return rc;
  snprintf(g_last_route, sizeof(g_last_route), "%s %s tx%d te%d", mode_name(mode), route == PYG_HIP_SPLINE_ROUTE_LDS ? "lds" : "global",
           t.TX, t.TE);
  const int64_t out_elems = mode == MODE_BB ? E * S : E * A;
  if (out_elems == 0) return PYG_HIP_OK;
  WeightingArgs a{rows, grad, weight, basis, weight_index, out, E, K, ceil_div(E, t.TE), (int)S, (int)R, (int)A, t.TX, t.TE, t.SB, slot};
  switch (mode) {
    case MODE_FWD: return launch_weighting_dtype<MODE_FWD>(dtype, a, route, t.tile_bytes, stream);
    case MODE_BX: return launch_weighting_dtype<MODE_BX>(dtype, a, route, t.tile_bytes, stream);
    default: return launch_weighting_dtype<MODE_BB>(dtype, a, route, t.tile_bytes, stream);
  }
}

int check_weighting(const char* op, int dtype, int64_t E, int64_t S, int64_t M_in, int64_t M_out, int64_t K) {
  PYG_HIP_REQUIRE(weighting_dtype(dtype), "%s: float32, float64 or bfloat16 only (dtype code %d)", op, dtype);
  PYG_HIP_REQUIRE(E >= 0 && S >= 0 && M_in >= 0 && M_out >= 0 && K >= 0, "%s: negative size", op);
  if (E * std::max<int64_t>(S, 1) >= (1ll << 40)) return fail(PYG_HIP_ERR_UNSUPPORTED, "%s: 2^40 or more (edge, basis) pairs", op);
  return PYG_HIP_OK;
}

struct DwPlan {
  bool ok = false;
  int64_t n = 0, max_items = 0, max_slabs = 0;
  size_t o_keys = 0, o_sorted = 0, o_order = 0, o_sort = 0, o_rows = 0, o_items = 0, o_slab_start = 0, o_slabs = 0, sort_bytes = 0, total = 0;
};

DwPlan make_dw_plan(int dtype, int64_t E, int64_t S, int64_t M_in, int64_t M_out, int64_t K, int chunk) {
  DwPlan p;
  if (!weighting_dtype(dtype) || E < 0 || S < 0 || M_in < 0 || M_out < 0 || K < 0) return p;
  if (K >= (1ll << 31) || S >= (1ll << 20) || M_in >= (1ll << 20) || M_out >= (1ll << 20) || E * std::max<int64_t>(S, 1) >= (1ll << 40)) return p;
  p.n = E * S;
  p.max_items = ceil_div(p.n, chunk) + K;     // every weight: at most len / chunk + 1
  p.max_slabs = 2 * p.n / chunk + 1;          // a weight of more than one chunk: fewer than 2 * len / chunk
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += align_up(bytes ? bytes : 1, 256);
    return o;
  };
  p.sort_bytes = index_sort_ws_bytes_i64(p.n);
  p.o_keys = take((size_t)p.n * 8);
  p.o_sorted = take((size_t)p.n * 8);
  p.o_order = take((size_t)p.n * 8);
  p.o_sort = take(p.sort_bytes);
  p.o_rows = take((size_t)(K + 1) * 8);
  p.o_items = take((size_t)(K + 1) * 8);
  p.o_slab_start = take((size_t)(K + 1) * 8);
  p.o_slabs = take((size_t)p.max_slabs * M_in * M_out * acc_size(dtype));
  p.total = at;
  p.ok = true;
  return p;
}

// `flags` bits 8 ..: log2 of the chunk of THIS call (a measurement hook; 0: the constant)
int chunk_of(int flags) {
  const int lg = (flags >> 8) & 31;
  if (lg == 0) return kChunk;
  return lg >= 9 && lg <= 12 ? 1 << lg : 0;
}

template <typename T>
int run_dw(const DwArgs& a, const DwPlan& p, hipStream_t stream) {
  const int tiles_in = (int)ceil_div(a.M_in, kDwTile), tiles_out = (int)ceil_div(a.M_out, kDwTile);
  if ((int64_t)tiles_in * tiles_out > 65535) return fail(PYG_HIP_ERR_UNSUPPORTED, "spline_weighting_backward_weight: more than 65535 matrix tiles");
  if (p.max_items >= (1ll << 31)) return fail(PYG_HIP_ERR_UNSUPPORTED, "spline_weighting_backward_weight: 2^31 or more work items");
  hipLaunchKernelGGL((dw_kernel<T>), dim3((unsigned)p.max_items, (unsigned)(tiles_in * tiles_out)), dim3(kThreads), 0, stream, a);
  PYG_HIP_CHECK(hipGetLastError());
  if (a.n > a.chunk) {   // else no weight can hold more than one chunk
    const size_t mat = (size_t)a.M_in * a.M_out;
    if (a.K > 65535) return fail(PYG_HIP_ERR_UNSUPPORTED, "spline_weighting_backward_weight: more than 65535 weights with more than %d pairs in all", a.chunk);
    hipLaunchKernelGGL((dw_reduce_kernel<T>), dim3((unsigned)ceil_div((int64_t)mat, kThreads), (unsigned)a.K), dim3(kThreads), 0, stream, a);
    PYG_HIP_CHECK(hipGetLastError());
  }
  return PYG_HIP_OK;
}

template <typename T, int DEG>
int run_basis(const void* pseudo, const int64_t* kernel_size, const uint8_t* is_open, int64_t E, int D, int64_t S, void* basis,
              int64_t* weight_index, hipStream_t stream) {
  hipLaunchKernelGGL((basis_kernel<T, DEG>), dim3((unsigned)ceil_div(E * S, kThreads)), dim3(kThreads), 0, stream, static_cast<const T*>(pseudo),
                     kernel_size, is_open, E, D, S, static_cast<T*>(basis), weight_index);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

template <typename T, int DEG>
int run_basis_backward(const void* grad_basis, const void* pseudo, const int64_t* kernel_size, const uint8_t* is_open, int64_t E, int D,
                       int64_t S, void* grad_pseudo, hipStream_t stream) {
  hipLaunchKernelGGL((basis_backward_kernel<T, DEG>), dim3((unsigned)ceil_div(E * D, kThreads)), dim3(kThreads), 0, stream,
                     static_cast<const T*>(grad_basis), static_cast<const T*>(pseudo), kernel_size, is_open, E, D, S, static_cast<T*>(grad_pseudo));
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

int check_basis(const char* op, int dtype, int64_t E, int64_t D, int degree, int64_t* S) {
  PYG_HIP_REQUIRE(dtype == PYG_F32 || dtype == PYG_F64, "%s: float32 or float64 only on the device (dtype code %d)", op, dtype);
  PYG_HIP_REQUIRE(degree >= 1 && degree <= 3, "Basis degree not implemented");
  PYG_HIP_REQUIRE(E >= 0 && D >= 0, "%s: negative size", op);
  if (D > kMaxDims) return fail(PYG_HIP_ERR_UNSUPPORTED, "%s: more than %d pseudo-coordinate dimensions", op, kMaxDims);
  int64_t s = 1;
  for (int64_t d = 0; d < D; ++d) s *= degree + 1;
  if (E * std::max<int64_t>(s, D) >= (1ll << 39)) return fail(PYG_HIP_ERR_UNSUPPORTED, "%s: 2^39 or more (edge, basis) pairs", op);
  *S = s;
  return PYG_HIP_OK;
}

}  // namespace
}  // namespace pyg_hip

using namespace pyg_hip;

extern "C" {

int pyg_hip_spline_route(int dtype, int64_t E, int64_t S, int64_t M_in, int64_t M_out, int64_t K) {
  return choose_route(dtype, E, S, M_in, M_out, K, 0);
}

const char* pyg_hip_spline_last_route(void) { return g_last_route; }

int pyg_hip_spline_tile(int which) {
  switch (which) {
    case PYG_HIP_SPLINE_TILE_LDS_BYTES: return kLdsWeightBytes;
    case PYG_HIP_SPLINE_TILE_CHUNK: return kChunk;
    case PYG_HIP_SPLINE_TILE_EDGE_BYTES: return kLdsTileBytes;
    case PYG_HIP_SPLINE_TILE_DW: return kDwTile;
    default: return 0;
  }
}

int pyg_hip_spline_pending_error(void) {
  int* slot = nullptr;
  if (deferred_slot(&slot) != PYG_HIP_OK) return PYG_HIP_ERR_RUNTIME;
  const int pending = *static_cast<volatile int*>(slot);
  *static_cast<volatile int*>(slot) = 0;
  return pending;
}

int pyg_hip_spline_basis(int dtype, const void* pseudo, const int64_t* kernel_size, const uint8_t* is_open_spline, int64_t E, int64_t D,
                         int degree, void* basis, int64_t* weight_index, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  int64_t S = 0;
  if (int rc = check_basis("spline_basis", dtype, E, D, degree, &S)) return rc;
  int* slot = nullptr;
  if (int rc = take_slot("spline_basis", &slot)) return rc;
  if (E == 0) return PYG_HIP_OK;
  PYG_HIP_REQUIRE(basis && weight_index && (D == 0 || (pseudo && kernel_size && is_open_spline)), "spline_basis: NULL tensor");
#define PYG_SPLINE_BASIS(T)                                                                                                         \
  switch (degree) {                                                                                                                 \
    case 1: return run_basis<T, 1>(pseudo, kernel_size, is_open_spline, E, (int)D, S, basis, weight_index, stream);                 \
    case 2: return run_basis<T, 2>(pseudo, kernel_size, is_open_spline, E, (int)D, S, basis, weight_index, stream);                 \
    default: return run_basis<T, 3>(pseudo, kernel_size, is_open_spline, E, (int)D, S, basis, weight_index, stream);                \
  }
  if (dtype == PYG_F32) { PYG_SPLINE_BASIS(float) }
  PYG_SPLINE_BASIS(double)
#undef PYG_SPLINE_BASIS
}

int pyg_hip_spline_basis_backward(int dtype, const void* grad_basis, const void* pseudo, const int64_t* kernel_size,
                                  const uint8_t* is_open_spline, int64_t E, int64_t D, int64_t S, int degree, void* grad_pseudo,
                                  void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  int64_t full = 0;
  if (int rc = check_basis("spline_basis_backward", dtype, E, D, degree, &full)) return rc;
  PYG_HIP_REQUIRE(S >= 0 && S <= full, "spline_basis_backward: grad_basis has %lld columns, (degree + 1)^D is %lld", (long long)S, (long long)full);
  int* slot = nullptr;
  if (int rc = take_slot("spline_basis_backward", &slot)) return rc;
  if (E == 0 || D == 0) return PYG_HIP_OK;
  PYG_HIP_REQUIRE(grad_pseudo && pseudo && kernel_size && is_open_spline && (S == 0 || grad_basis), "spline_basis_backward: NULL tensor");
#define PYG_SPLINE_BASIS_BW(T)                                                                                                      \
  switch (degree) {                                                                                                                 \
    case 1: return run_basis_backward<T, 1>(grad_basis, pseudo, kernel_size, is_open_spline, E, (int)D, S, grad_pseudo, stream);    \
    case 2: return run_basis_backward<T, 2>(grad_basis, pseudo, kernel_size, is_open_spline, E, (int)D, S, grad_pseudo, stream);    \
    default: return run_basis_backward<T, 3>(grad_basis, pseudo, kernel_size, is_open_spline, E, (int)D, S, grad_pseudo, stream);   \
  }
  if (dtype == PYG_F32) { PYG_SPLINE_BASIS_BW(float) }
  PYG_SPLINE_BASIS_BW(double)
#undef PYG_SPLINE_BASIS_BW
}

int pyg_hip_spline_weighting(int dtype, const void* x, const void* weight, const void* basis, const int64_t* weight_index, int64_t E,
                             int64_t S, int64_t M_in, int64_t M_out, int64_t K, int flags, void* out, void* stream_) {
  const char* op = "spline_weighting";
  if (int rc = check_weighting(op, dtype, E, S, M_in, M_out, K)) return rc;
  PYG_HIP_REQUIRE(E * M_out == 0 || (out && (S * M_in == 0 || (x && weight && basis && weight_index))), "%s: NULL tensor", op);
  return run_weighting(MODE_FWD, op, dtype, x, nullptr, weight, basis, weight_index, E, S, M_in, M_out, K, flags, out,
                       static_cast<hipStream_t>(stream_));
}

size_t pyg_hip_spline_backward_x_workspace_size(int dtype, int64_t M_in, int64_t M_out, int64_t K) {
  if (!weighting_dtype(dtype) || M_in < 0 || M_out < 0 || K < 0) return 0;
  return align_up((size_t)K * M_in * M_out * elem_size(dtype) + 1, 256);
}

int pyg_hip_spline_weighting_backward_x(int dtype, const void* grad_out, const void* weight, const void* basis, const int64_t* weight_index,
                                        int64_t E, int64_t S, int64_t M_in, int64_t M_out, int64_t K, int flags, void* workspace,
                                        size_t workspace_bytes, void* grad_x, void* stream_) {
  const char* op = "spline_weighting_backward_x";
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (int rc = check_weighting(op, dtype, E, S, M_in, M_out, K)) return rc;
  PYG_HIP_REQUIRE(E * M_in == 0 || (grad_x && (S * M_out == 0 || (grad_out && weight && basis && weight_index))), "%s: NULL tensor", op);
  const size_t need = pyg_hip_spline_backward_x_workspace_size(dtype, M_in, M_out, K);
  const int64_t w_elems = K * M_in * M_out;
  if (E * M_in > 0 && w_elems > 0) {
    PYG_HIP_REQUIRE(workspace != nullptr, "%s: NULL workspace", op);
    if (workspace_bytes < need) return fail(PYG_HIP_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", op, workspace_bytes, need);
    PYG_HIP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: the workspace must be 16-byte aligned", op);
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(w_elems, kThreads), 65536);
    switch (dtype) {
      case PYG_F32: hipLaunchKernelGGL((transpose_kernel<float>), dim3(grid), dim3(kThreads), 0, stream, static_cast<const float*>(weight), static_cast<float*>(workspace), K, (int)M_in, (int)M_out); break;
      case PYG_F64: hipLaunchKernelGGL((transpose_kernel<double>), dim3(grid), dim3(kThreads), 0, stream, static_cast<const double*>(weight), static_cast<double*>(workspace), K, (int)M_in, (int)M_out); break;
      default: hipLaunchKernelGGL((transpose_kernel<uint16_t>), dim3(grid), dim3(kThreads), 0, stream, static_cast<const uint16_t*>(weight), static_cast<uint16_t*>(workspace), K, (int)M_in, (int)M_out); break;
    }
    PYG_HIP_CHECK(hipGetLastError());
  }
  return run_weighting(MODE_BX, op, dtype, grad_out, nullptr, workspace, basis, weight_index, E, S, M_in, M_out, K, flags, grad_x, stream);
}

int pyg_hip_spline_weighting_backward_basis(int dtype, const void* grad_out, const void* x, const void* weight, const int64_t* weight_index,
                                            int64_t E, int64_t S, int64_t M_in, int64_t M_out, int64_t K, int flags, void* grad_basis,
                                            void* stream_) {
  const char* op = "spline_weighting_backward_basis";
  if (int rc = check_weighting(op, dtype, E, S, M_in, M_out, K)) return rc;
  PYG_HIP_REQUIRE(E * S == 0 || (grad_basis && weight_index && (M_in * M_out == 0 || (grad_out && x && weight))), "%s: NULL tensor", op);
  return run_weighting(MODE_BB, op, dtype, x, grad_out, weight, nullptr, weight_index, E, S, M_in, M_out, K, flags, grad_basis,
                       static_cast<hipStream_t>(stream_));
}

size_t pyg_hip_spline_backward_weight_workspace_size(int dtype, int64_t E, int64_t S, int64_t M_in, int64_t M_out, int64_t K, int flags) {
  const int chunk = chunk_of(flags);
  if (!chunk) return 0;
  const DwPlan p = make_dw_plan(dtype, E, S, M_in, M_out, K, chunk);
  return p.ok ? p.total : 0;
}

int pyg_hip_spline_weighting_backward_weight(int dtype, const void* grad_out, const void* x, const void* basis, const int64_t* weight_index,
                                             int64_t E, int64_t S, int64_t M_in, int64_t M_out, int64_t K, int flags, void* workspace,
                                             size_t workspace_bytes, void* grad_weight, void* stream_) {
  const char* op = "spline_weighting_backward_weight";
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (int rc = check_weighting(op, dtype, E, S, M_in, M_out, K)) return rc;
  const int chunk = chunk_of(flags);
  PYG_HIP_REQUIRE(chunk != 0, "%s: the chunk of a call is a power of two from 512 to 4096", op);
  const DwPlan p = make_dw_plan(dtype, E, S, M_in, M_out, K, chunk);
  if (!p.ok) return fail(PYG_HIP_ERR_UNSUPPORTED, "%s: no kernel for these sizes", op);
  int* slot = nullptr;
  if (int rc = take_slot(op, &slot)) return rc;
  if (K * M_in * M_out == 0) return PYG_HIP_OK;
  PYG_HIP_REQUIRE(grad_weight && (p.n == 0 || (grad_out && x && basis && weight_index)), "%s: NULL tensor", op);
  PYG_HIP_REQUIRE(workspace != nullptr, "%s: NULL workspace", op);
  if (workspace_bytes < p.total)
    return fail(PYG_HIP_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (pyg_hip_spline_backward_weight_workspace_size)", op,
                workspace_bytes, p.total);
  PYG_HIP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: the workspace must be 16-byte aligned", op);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  int64_t* keys = reinterpret_cast<int64_t*>(ws + p.o_keys);
  int64_t* sorted = reinterpret_cast<int64_t*>(ws + p.o_sorted);
  int64_t* order = reinterpret_cast<int64_t*>(ws + p.o_order);
  int64_t* row_start = reinterpret_cast<int64_t*>(ws + p.o_rows);
  int64_t* item_start = reinterpret_cast<int64_t*>(ws + p.o_items);
  int64_t* slab_start = reinterpret_cast<int64_t*>(ws + p.o_slab_start);
  if (p.n > 0) {
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(p.n, kThreads), 65536);
    hipLaunchKernelGGL(dw_keys_kernel, dim3(grid), dim3(kThreads), 0, stream, weight_index, p.n, K, keys);
    PYG_HIP_CHECK(hipGetLastError());
    if (int rc = index_sort_i64(keys, p.n, K, sorted, order, ws + p.o_sort, p.sort_bytes, stream)) return rc;
  }
  hipLaunchKernelGGL(dw_plan_kernel, dim3(1), dim3(kThreads), 0, stream, sorted, p.n, K, chunk, row_start, item_start, slab_start, slot);
  PYG_HIP_CHECK(hipGetLastError());
  DwArgs a{grad_out, x, basis, order, row_start, item_start, slab_start, grad_weight, ws + p.o_slabs, p.n, K, (int)S, (int)M_in, (int)M_out, chunk,
           (int)ceil_div(M_out, kDwTile)};
  switch (dtype) {
    case PYG_F32: return run_dw<float>(a, p, stream);
    case PYG_F64: return run_dw<double>(a, p, stream);
    default: return run_dw<bf16_t>(a, p, stream);
  }
}

}  // extern "C"
