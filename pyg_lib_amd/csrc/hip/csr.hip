// segment_{sum,mean,min,max}_csr, gather_csr and softmax_csr (+ backward) for gfx950 (MI355X).
//
// Replaces pyg_lib/csrc/ops/cuda/segment_csr_kernel.cu (warp-32 shuffles) and gives
// pyg::softmax_csr -- CPU only in the reference (ops/cpu/softmax_kernel.cpp) -- a device path.
// Contracts follow pyg_lib/csrc/ops/cpu/segment_csr_kernel.cpp: src viewed as [leading, E, K],
// indptr [leading, rows + 1] (slice stride 0 = one indptr broadcast over the slices, read in place
// instead of `expand().contiguous()`), out / arg [leading, rows, K].
//
// CSR rows write disjoint outputs, so nothing is atomic.  HBM-bound byte work:
//   * L = 1 (default): one thread per (row, 16-byte column slice) walks its row in source order and
//     accumulates in the reference's opmath -- the CPU kernel's exact operation order, so sums and
//     means are BIT-exact with the reference for every dtype (min/max/arg trivially).
//   * L = 8 / 64 lanes per (row, slice) when rows are long and few (average length >= 64 / 1024 and
//     too few rows to fill the chip): lane j takes e = a + j, a + j + L, ...; partial results are
//     combined by xor shuffles (floating sums then differ from the CPU order by rounding; min/max and
//     their first-match arg stay exact through a lexicographic (value, position) combine).
#include "common.h"
#include "elem.h"
#include "csr_rows.h"

#include <algorithm>
#include <cstdint>
#include <type_traits>

namespace pyg_hip {
namespace {

enum { CSR_SUM = 0, CSR_MEAN = 1, CSR_MIN = 2, CSR_MAX = 3 };

// what a FRESH min / max output starts from (pyg_hip_fill_reduce_identity's value): with fresh != 0 the kernels do not read `out`
template <typename T, int OP>
__device__ __forceinline__ typename Math<T>::acc_t minmax_identity() {
  return Math<T>::up(OP == CSR_MIN ? type_max<T>() : type_lowest<T>());
}

struct CsrShape {
  int64_t leading, rows, E, K;
  int64_t indptr_stride;  // elements between the indptr of consecutive slices (0 = broadcast)
  int64_t long_cut = INT64_MAX;  // segment_csr_kernel: rows of more positions are left to the hub kernels below
  void* hub_ws = nullptr;        // (host side) the caller's scratch for them: pyg_hip_csr_hub_workspace_size()
  size_t hub_ws_bytes = 0;
};

// OP: CSR_SUM / CSR_MEAN / CSR_MIN / CSR_MAX.  V elements (16 bytes, or 1) per thread, L lanes per item.
// PERM: row positions are read through perm[e] (scatter_min/max after an index sort; perm is ascending
// inside a row, so "first match" is still the smallest source position).
template <typename T, int OP, int V, int L, bool PERM>
__global__ __launch_bounds__(256) void segment_csr_kernel(const T* __restrict__ src, const int64_t* __restrict__ indptr,
                                                          const int64_t* __restrict__ perm, T* __restrict__ out,
                                                          int64_t* __restrict__ arg, int fresh, CsrShape s, HubWs hw) {
  using acc_t = typename Math<T>::acc_t;
  using P = Pack<T, V>;
  const int64_t kv = s.K / V;
  const int64_t t = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / L;
  const int lane = threadIdx.x & (L - 1);
  const int64_t items = s.leading * s.rows * kv;
  const bool live = t < items;
  const int64_t tt = live ? t : 0;
  const int64_t n = tt / kv;        // flat row
  const int64_t c = (tt % kv) * V;  // first column of this thread's slice
  const int64_t slice = n / s.rows;
  const int64_t row = n % s.rows;
  const int64_t a = indptr[slice * s.indptr_stride + row];
  const int64_t b = indptr[slice * s.indptr_stride + row + 1];
  if (b - a > s.long_cut) {   // (all L lanes of the item alike) a hub row
    if (hw.counters && live && lane == 0 && c == 0) hub_register(hw, n, b - a);
    return;
  }
  const T* sp = src + slice * s.E * s.K + c;
  T* op = out + n * s.K + c;

  acc_t acc[V];
  int64_t best[V];
  if constexpr (OP == CSR_SUM) {
    // lane 0's accumulator is seeded from the caller's `out` slot; a fresh output starts at +0 without being read (it
    // need not be cleared either: every slot is written below -- 2 x N x K bytes less traffic).  The other lanes: sum_identity()
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = lane == 0 ? acc_t(0) : sum_identity<acc_t>();
    if (!fresh) {
      P cur = *reinterpret_cast<const P*>(op);
#pragma unroll
      for (int i = 0; i < V; ++i) acc[i] = lane == 0 ? Math<T>::up(cur.v[i]) : sum_identity<acc_t>();
    }
  } else if constexpr (OP == CSR_MEAN) {
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = lane == 0 ? acc_t(0) : sum_identity<acc_t>();
  } else {
    // (a fresh output starts from the identity without being read -- and need not be pre-filled: 2 x N x K bytes less traffic)
    P cur;
    if (!fresh) cur = *reinterpret_cast<const P*>(op);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      acc[i] = fresh ? minmax_identity<T, OP>() : Math<T>::up(cur.v[i]);
      best[i] = s.E;
    }
  }
  if (live) {
    // four positions per trip: their loads are in flight together (a row is ~10 positions long in the sampler's
    // graphs and the loop is a chain of dependent memory round trips otherwise); accumulated in position order
#ifndef PYG_CSR_U
#define PYG_CSR_U 4
#endif
    constexpr int U = PYG_CSR_U;
    for (int64_t e0 = a + lane; e0 < b; e0 += (int64_t)U * L) {
      int64_t pp[U];
      P xx[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t e = e0 + (int64_t)u * L;
        const int64_t ec = e < b ? e : e0;  // clamped: the load is issued unconditionally, the value is ignored below
        pp[u] = PERM ? perm[ec] : ec;
      }
      if constexpr (PERM) pin_all(pp);
#pragma unroll
      for (int u = 0; u < U; ++u) xx[u] = *reinterpret_cast<const P*>(sp + pp[u] * s.K);
      pin_all(xx);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (e0 + (int64_t)u * L >= b) break;
        const int64_t p = pp[u];
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const acc_t v = Math<T>::up(xx[u].v[i]);
          if constexpr (OP == CSR_SUM || OP == CSR_MEAN) {
            acc[i] += v;
          } else if constexpr (OP == CSR_MIN) {
            if (v < acc[i]) { acc[i] = v; best[i] = p; }
          } else {
            if (v > acc[i]) { acc[i] = v; best[i] = p; }
          }
        }
      }
    }
  }
  if constexpr (L > 1) {
#pragma unroll
    for (int m = L >> 1; m >= 1; m >>= 1) {
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const acc_t ov = shfl_xor_any(acc[i], m);
        if constexpr (OP == CSR_SUM || OP == CSR_MEAN) {
          acc[i] += ov;
        } else {
          const int64_t ob = shfl_xor_any(best[i], m);
          const bool better = OP == CSR_MIN ? ov < acc[i] : ov > acc[i];
          const bool worse = OP == CSR_MIN ? acc[i] < ov : acc[i] > ov;
          if (better || (!worse && ob < best[i])) { acc[i] = ov; best[i] = ob; }
        }
      }
    }
  }
  if (!live || lane != 0) return;
  P res;
  if constexpr (OP == CSR_MEAN) {
    const int64_t len = b - a;
    const acc_t denom = (acc_t)(len > 0 ? len : 1);
#pragma unroll
    for (int i = 0; i < V; ++i) res.v[i] = Math<T>::down(acc[i] / denom);
  } else if constexpr (OP == CSR_SUM) {
#pragma unroll
    for (int i = 0; i < V; ++i) res.v[i] = Math<T>::down(acc[i]);
  } else {
    // rows without a contribution of a fresh output read 0 (segment_csr_kernel.cpp:416-418)
#pragma unroll
    for (int i = 0; i < V; ++i) {
      res.v[i] = Math<T>::down(acc[i]);
      if (fresh && best[i] == s.E) res.v[i] = Math<T>::down(acc_t(0));
      arg[n * s.K + c + i] = best[i];
    }
  }
  *reinterpret_cast<P*>(op) = res;
}

// The hub kernels.  256 threads take positions [pa, pb) of one row as S 16-byte slices x 256 / S position lanes (lane j
// takes pa + j, pa + j + 256 / S, ..., eight loads in flight); the lanes' partial results are combined through LDS by a
// fixed pairwise tree: the same bits on every run; floating sums differ from the sequential order by rounding like the L > 1 variants
// above; min / max and their first-match arg stay exact.
// tot / tb of the threads with g.lane == 0 (and `on`): start (+) the span's positions; every thread of the workgroup calls it
template <typename T, int OP, int V, bool PERM>
__device__ __forceinline__ void hub_span(const T* __restrict__ sp, const int64_t* __restrict__ perm, int64_t pa, int64_t pb,
                                         int64_t rowK, bool on, const HubGeom<T, V>& g,
                                         const typename Math<T>::acc_t (&start)[V], typename Math<T>::acc_t* part,
                                         int64_t* part_best, typename Math<T>::acc_t (&tot)[V], int64_t (&tb)[V], int64_t E) {
  using acc_t = typename Math<T>::acc_t;
  using P = Pack<T, V>;
  constexpr bool MINMAX = OP == CSR_MIN || OP == CSR_MAX;
  acc_t acc[V];
  int64_t best[V];
#pragma unroll
  for (int i = 0; i < V; ++i) acc[i] = MINMAX ? start[i] : sum_identity<acc_t>(), best[i] = E;
  if (on) {
    constexpr int U = 8;
    for (int64_t e0 = pa + g.lane; e0 < pb; e0 += (int64_t)U * g.EL) {
      int64_t pp[U];
      P xx[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t e = e0 + (int64_t)u * g.EL;
        const int64_t ec = e < pb ? e : e0;
        pp[u] = PERM ? perm[ec] : ec;
      }
      if constexpr (PERM) pin_all(pp);
#pragma unroll
      for (int u = 0; u < U; ++u) xx[u] = *reinterpret_cast<const P*>(sp + pp[u] * rowK);
      pin_all(xx);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (e0 + (int64_t)u * g.EL >= pb) break;
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const acc_t v = Math<T>::up(xx[u].v[i]);
          if constexpr (!MINMAX) {
            acc[i] += v;
          } else if constexpr (OP == CSR_MIN) {
            if (v < acc[i]) { acc[i] = v; best[i] = pp[u]; }
          } else {
            if (v > acc[i]) { acc[i] = v; best[i] = pp[u]; }
          }
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < V; ++i) {
    part[threadIdx.x * V + i] = acc[i];
    if constexpr (MINMAX) part_best[threadIdx.x * V + i] = best[i];
  }
  __syncthreads();
  // the lanes of a slice combine pairwise, lane l with lane l + stride (a fixed tree: the same bits on every run; one thread
  // walking 256 lanes x 8 values out of LDS took 60 us per chunk)
  for (int st = g.EL >> 1; st >= 1; st >>= 1) {
    if (g.lane < st) {
      const int ia = threadIdx.x * V, ib = (((g.lane + st) << g.logS) + g.sl) * V;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const acc_t ov = part[ib + i];
        if constexpr (!MINMAX) {
          part[ia + i] += ov;
        } else {
          const acc_t cv = part[ia + i];
          const int64_t ob = part_best[ib + i], cb = part_best[ia + i];
          const bool better = OP == CSR_MIN ? ov < cv : ov > cv;
          const bool worse = OP == CSR_MIN ? cv < ov : cv > ov;
          if (better || (!worse && ob < cb)) part[ia + i] = ov, part_best[ia + i] = ob;
        }
      }
    }
    __syncthreads();
  }
  if (on && g.lane == 0) {
#pragma unroll
    for (int i = 0; i < V; ++i) {
      // (min / max: every lane started from `start`, it is inside the combined value already)
      tot[i] = MINMAX ? part[threadIdx.x * V + i] : start[i] + part[threadIdx.x * V + i];
      tb[i] = MINMAX ? part_best[threadIdx.x * V + i] : E;
    }
  }
  __syncthreads();
}

// the row's final value from (tot, tb) -> out / arg
template <typename T, int OP, int V>
__device__ __forceinline__ void hub_store(T* __restrict__ op, int64_t* __restrict__ ap, typename Math<T>::acc_t (&tot)[V],
                                          int64_t (&tb)[V], int64_t len, int fresh, int64_t E) {
  using acc_t = typename Math<T>::acc_t;
  constexpr bool MINMAX = OP == CSR_MIN || OP == CSR_MAX;
  Pack<T, V> res;
#pragma unroll
  for (int i = 0; i < V; ++i) {
    if constexpr (OP == CSR_MEAN) tot[i] = tot[i] / (acc_t)len;
    res.v[i] = Math<T>::down(tot[i]);
    if constexpr (MINMAX) {
      if (fresh && tb[i] == E) res.v[i] = Math<T>::down(acc_t(0));
      ap[i] = tb[i];
    }
  }
  *reinterpret_cast<Pack<T, V>*>(op) = res;
}

// what a row's accumulation starts from: the caller's `out` slot (sum into an existing output; min / max always), +0 for a
// fresh sum / a mean.  `row_start` false: the partial sum of one chunk of a longer hub -- it starts from sum_identity(), the
// row's start is added once, where the chunks are combined
template <typename T, int OP, int V>
__device__ __forceinline__ void hub_seed(const T* __restrict__ op, bool on, int fresh, typename Math<T>::acc_t (&seed)[V],
                                         bool row_start = true) {
  using acc_t = typename Math<T>::acc_t;
  constexpr bool MINMAX = OP == CSR_MIN || OP == CSR_MAX;
#pragma unroll
  for (int i = 0; i < V; ++i)
    seed[i] = MINMAX ? minmax_identity<T, MINMAX ? OP : CSR_MIN>() : (row_start ? acc_t(0) : sum_identity<acc_t>());
  if (on && row_start && !fresh && (MINMAX || OP == CSR_SUM)) {
    const Pack<T, V> cur = *reinterpret_cast<const Pack<T, V>*>(op);
#pragma unroll
    for (int i = 0; i < V; ++i) seed[i] = Math<T>::up(cur.v[i]);
  }
}

// Without scratch: every workgroup looks at 256 rows at a time and takes the long ones among them, one after the other.
template <typename T, int OP, int V, bool PERM>
__global__ __launch_bounds__(256) void segment_csr_long_kernel(const T* __restrict__ src, const int64_t* __restrict__ indptr,
                                                               const int64_t* __restrict__ perm, T* __restrict__ out,
                                                               int64_t* __restrict__ arg, int fresh, CsrShape s) {
  using acc_t = typename Math<T>::acc_t;
  constexpr bool MINMAX = OP == CSR_MIN || OP == CSR_MAX;
  __shared__ int64_t long_rows[256];
  __shared__ int n_long;
  __shared__ acc_t part[256 * V];
  __shared__ int64_t part_best[MINMAX ? 256 * V : 1];
  const int64_t kv = s.K / V;
  const int64_t nrows = s.leading * s.rows;
  const HubGeom<T, V> g(kv);
  for (int64_t base = (int64_t)blockIdx.x * 256; base < nrows; base += (int64_t)gridDim.x * 256) {
    if (threadIdx.x == 0) n_long = 0;
    __syncthreads();
    {
      const int64_t n = base + threadIdx.x;
      if (n < nrows) {
        const int64_t slice = n / s.rows, row = n % s.rows;
        const int64_t a = indptr[slice * s.indptr_stride + row], b = indptr[slice * s.indptr_stride + row + 1];
        if (b - a > s.long_cut) long_rows[atomicAdd(&n_long, 1)] = n;   // (their order does not matter: rows are independent)
      }
    }
    __syncthreads();
    const int cnt = n_long;
    for (int j = 0; j < cnt; ++j) {
      const int64_t n = long_rows[j];
      const int64_t slice = n / s.rows, row = n % s.rows;
      const int64_t a = indptr[slice * s.indptr_stride + row], b = indptr[slice * s.indptr_stride + row + 1];
      for (int64_t c0 = 0; c0 < kv; c0 += g.S) {
        const int64_t ci = c0 + g.sl;
        const bool on = ci < kv;
        const int64_t c = (on ? ci : 0) * V;
        T* op = out + n * s.K + c;
        acc_t seed[V], tot[V];
        int64_t tb[V];
        hub_seed<T, OP, V>(op, on, fresh, seed);
        hub_span<T, OP, V, PERM>(src + slice * s.E * s.K + c, perm, a, b, s.K, on, g, seed, part, part_best, tot, tb, s.E);
        if (on && g.lane == 0) hub_store<T, OP, V>(op, MINMAX ? arg + n * s.K + c : nullptr, tot, tb, b - a, fresh, s.E);
      }
    }
    __syncthreads();
  }
}

// With scratch: one registered chunk per workgroup and trip.  A hub of one chunk is finished on the spot; the chunks of a
// longer one leave their results in the hub's slots ...
template <typename T, int OP, int V, bool PERM>
__global__ __launch_bounds__(256) void segment_csr_hub_chunk_kernel(const T* __restrict__ src, const int64_t* __restrict__ indptr,
                                                                    const int64_t* __restrict__ perm, T* __restrict__ out,
                                                                    int64_t* __restrict__ arg, int fresh, CsrShape s, HubWs hw) {
  using acc_t = typename Math<T>::acc_t;
  constexpr bool MINMAX = OP == CSR_MIN || OP == CSR_MAX;
  __shared__ acc_t part[256 * V];
  __shared__ int64_t part_best[MINMAX ? 256 * V : 1];
  const int64_t kv = s.K / V;
  const HubGeom<T, V> g(kv);
  const int nchunks = hw.counters[3] ? 0 : hw.counters[1];
  for (int q = blockIdx.x; q < nchunks; q += gridDim.x) {
    const int2 cr = hw.chunks[q];
    const HubRec hub = hw.hubs[cr.x];
    const int64_t n = hub.n;
    const int64_t slice = n / s.rows, row = n % s.rows;
    const int64_t a = indptr[slice * s.indptr_stride + row], b = indptr[slice * s.indptr_stride + row + 1];
    const int64_t pa = a + (int64_t)cr.y * hw.CH, pb = pa + hw.CH < b ? pa + hw.CH : b;
    const bool whole = hub.nch == 1;
    const int64_t slot = (int64_t)(hub.slot_base + cr.y) * s.K;
    for (int64_t c0 = 0; c0 < kv; c0 += g.S) {
      const int64_t ci = c0 + g.sl;
      const bool on = ci < kv;
      const int64_t c = (on ? ci : 0) * V;
      T* op = out + n * s.K + c;
      acc_t seed[V], tot[V];
      int64_t tb[V];
      hub_seed<T, OP, V>(op, on, fresh, seed, whole || MINMAX);   // (the sum of a chunk starts from the identity)
      hub_span<T, OP, V, PERM>(src + slice * s.E * s.K + c, perm, pa, pb, s.K, on, g, seed, part, part_best, tot, tb, s.E);
      if (on && g.lane == 0) {
        if (whole) {
          hub_store<T, OP, V>(op, MINMAX ? arg + n * s.K + c : nullptr, tot, tb, b - a, fresh, s.E);
        } else {
#pragma unroll
          for (int i = 0; i < V; ++i) {
            reinterpret_cast<acc_t*>(hw.partial)[slot + c + i] = tot[i];
            if constexpr (MINMAX) hw.partial_best[slot + c + i] = tb[i];
          }
        }
      }
    }
  }
}

// ... and a third launch adds a longer hub's slots up in chunk order: one thread per (hub, 16-byte slice).  (One launch for
// both -- the workgroup that writes a hub's last slot combines them -- needs device-scope fences around the count: each
// writes back and invalidates the XCD's whole L2, 4000 chunks took 650 us that way instead of 60.)
template <typename T, int OP, int V>
__global__ __launch_bounds__(256) void segment_csr_hub_combine_kernel(const int64_t* __restrict__ indptr, T* __restrict__ out,
                                                                      int64_t* __restrict__ arg, int fresh, CsrShape s, HubWs hw) {
  using acc_t = typename Math<T>::acc_t;
  constexpr bool MINMAX = OP == CSR_MIN || OP == CSR_MAX;
  const int64_t kv = s.K / V;
  const int64_t items = hw.counters[3] ? 0 : (int64_t)hw.counters[0] * kv;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < items; t += (int64_t)gridDim.x * blockDim.x) {
    const HubRec hub = hw.hubs[t / kv];
    if (hub.nch == 1) continue;
    const int64_t c = (t % kv) * V;
    const int64_t n = hub.n;
    const int64_t slice = n / s.rows, row = n % s.rows;
    const int64_t len = indptr[slice * s.indptr_stride + row + 1] - indptr[slice * s.indptr_stride + row];
    T* op = out + n * s.K + c;
    acc_t tot[V];
    int64_t tb[V];
    hub_seed<T, OP, V>(op, true, fresh, tot);
#pragma unroll
    for (int i = 0; i < V; ++i) tb[i] = s.E;
    // chunk order, eight slots' values in flight (a 500 000-position hub has 245 slots: 245 dependent trips took 90 us)
    constexpr int U = 8;
    for (int j0 = 0; j0 < hub.nch; j0 += U) {
      Pack<acc_t, V> ov[U];
      Pack<int64_t, V> ob[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = j0 + u < hub.nch ? j0 + u : j0;
        const int64_t sj = (int64_t)(hub.slot_base + j) * s.K + c;
#pragma unroll
        for (int i = 0; i < V; ++i) {
          ov[u].v[i] = reinterpret_cast<const acc_t*>(hw.partial)[sj + i];
          if constexpr (MINMAX) ob[u].v[i] = hw.partial_best[sj + i];
        }
      }
      pin_all(ov);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (j0 + u >= hub.nch) break;
#pragma unroll
        for (int i = 0; i < V; ++i) {
          if constexpr (!MINMAX) {
            tot[i] += ov[u].v[i];
          } else {
            const bool better = OP == CSR_MIN ? ov[u].v[i] < tot[i] : ov[u].v[i] > tot[i];
            const bool worse = OP == CSR_MIN ? tot[i] < ov[u].v[i] : tot[i] > ov[u].v[i];
            if (better || (!worse && ob[u].v[i] < tb[i])) tot[i] = ov[u].v[i], tb[i] = ob[u].v[i];
          }
        }
      }
    }
    hub_store<T, OP, V>(op, MINMAX ? arg + n * s.K + c : nullptr, tot, tb, len, fresh, s.E);
  }
}

// out[slice, e, :] = src[slice, r, :] for every position e of row r: the mirror image of the sum kernel
// (one thread per (row, 16-byte slice), L lanes per item for long rows).  Positions covered by no row
// are never written.
template <typename T, int V, int L>
__global__ __launch_bounds__(256) void gather_csr_kernel(const T* __restrict__ src, const int64_t* __restrict__ indptr,
                                                         T* __restrict__ out, CsrShape s, HubWs hw) {
  using P = Pack<T, V>;
  const int64_t kv = s.K / V;
  const int64_t t = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / L;
  const int lane = threadIdx.x & (L - 1);
  if (t >= s.leading * s.rows * kv) return;
  const int64_t n = t / kv;
  const int64_t c = (t % kv) * V;
  const int64_t slice = n / s.rows, row = n % s.rows;
  const int64_t a = indptr[slice * s.indptr_stride + row];
  const int64_t b = indptr[slice * s.indptr_stride + row + 1];
  if (b - a > s.long_cut) {   // a hub row: gather_csr_hub_chunk_kernel / gather_csr_long_kernel
    if (hw.counters && lane == 0 && c == 0) hub_register(hw, n, b - a);
    return;
  }
  const P v = *reinterpret_cast<const P*>(src + n * s.K + c);
  T* op = out + slice * s.E * s.K + c;
  for (int64_t e = a + lane; e < b; e += L) *reinterpret_cast<P*>(op + e * s.K) = v;
}

// `len` positions of one row written by 256 threads: 16-byte (or one-element) pieces in memory order
template <typename T, int V>
__device__ __forceinline__ void gather_span(const T* __restrict__ sp, T* __restrict__ op, int64_t len, int64_t kv) {
  using P = Pack<T, V>;
  const int64_t total = len * kv;
  if (kv <= 256 && 256 % kv == 0) {   // a thread's piece column never changes
    const P v = *reinterpret_cast<const P*>(sp + ((int64_t)threadIdx.x % kv) * V);
    for (int64_t i = threadIdx.x; i < total; i += 256) *reinterpret_cast<P*>(op + i * V) = v;
  } else {
    for (int64_t i = threadIdx.x; i < total; i += 256)
      *reinterpret_cast<P*>(op + i * V) = *reinterpret_cast<const P*>(sp + (i % kv) * V);
  }
}

// The hub rows of the kernel above (more than `long_cut` positions), a whole workgroup per row: the row's K values are
// written to consecutive positions by consecutive threads (full lines), the workgroups scan the row lengths 256 at a time
// like segment_csr_long_kernel.
template <typename T, int V>
__global__ __launch_bounds__(256) void gather_csr_long_kernel(const T* __restrict__ src, const int64_t* __restrict__ indptr,
                                                              T* __restrict__ out, CsrShape s) {
  __shared__ int64_t long_rows[256];
  __shared__ int n_long;
  const int64_t kv = s.K / V;
  const int64_t nrows = s.leading * s.rows;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < nrows; base += (int64_t)gridDim.x * 256) {
    if (threadIdx.x == 0) n_long = 0;
    __syncthreads();
    {
      const int64_t n = base + threadIdx.x;
      if (n < nrows) {
        const int64_t slice = n / s.rows, row = n % s.rows;
        const int64_t a = indptr[slice * s.indptr_stride + row], b = indptr[slice * s.indptr_stride + row + 1];
        if (b - a > s.long_cut) long_rows[atomicAdd(&n_long, 1)] = n;
      }
    }
    __syncthreads();
    const int cnt = n_long;
    for (int j = 0; j < cnt; ++j) {
      const int64_t n = long_rows[j];
      const int64_t slice = n / s.rows, row = n % s.rows;
      const int64_t a = indptr[slice * s.indptr_stride + row], b = indptr[slice * s.indptr_stride + row + 1];
      gather_span<T, V>(src + n * s.K, out + (slice * s.E + a) * s.K, b - a, kv);
    }
    __syncthreads();
  }
}

// with scratch: one registered chunk of a hub row per workgroup and trip
template <typename T, int V>
__global__ __launch_bounds__(256) void gather_csr_hub_chunk_kernel(const T* __restrict__ src, const int64_t* __restrict__ indptr,
                                                                   T* __restrict__ out, CsrShape s, HubWs hw) {
  const int64_t kv = s.K / V;
  const int nchunks = hw.counters[3] ? 0 : hw.counters[1];
  for (int q = blockIdx.x; q < nchunks; q += gridDim.x) {
    const int2 cr = hw.chunks[q];
    const int64_t n = hw.hubs[cr.x].n;
    const int64_t slice = n / s.rows, row = n % s.rows;
    const int64_t a = indptr[slice * s.indptr_stride + row], b = indptr[slice * s.indptr_stride + row + 1];
    const int64_t pa = a + (int64_t)cr.y * hw.CH, pb = pa + hw.CH < b ? pa + hw.CH : b;
    gather_span<T, V>(src + n * s.K, out + (slice * s.E + pa) * s.K, pb - pa, kv);
  }
}

// ---- softmax over CSR groups (float / double) ------------------------------------------------------
// src [outer, D, inner]; one item per (group, outer, inner) "head".  L lanes per item.
template <typename T, int L, bool BACKWARD>
__global__ __launch_bounds__(256) void softmax_csr_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                          const int64_t* __restrict__ ptr, T* __restrict__ y,
                                                          int64_t outer, int64_t D, int64_t inner, int64_t groups,
                                                          int64_t long_cut) {
  const int64_t t = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / L;
  const int lane = threadIdx.x & (L - 1);
  const bool live = t < groups * outer * inner;
  const int64_t tt = live ? t : 0;
  const int64_t sidx = tt % inner;
  const int64_t i = (tt / inner) % outer;
  const int64_t g = tt / (inner * outer);
  const int64_t a = ptr[g], b = ptr[g + 1];
  if (b - a > long_cut) return;   // (all L lanes of the item alike) a hub group: softmax_csr_long_kernel
  const int64_t base = i * D * inner + sidx;
  auto reduce = [&](T v, bool is_max) {
#pragma unroll
    for (int m = L >> 1; m >= 1; m >>= 1) {
      const T o = shfl_xor_any(v, m);
      v = is_max ? (v < o ? o : v) : v + o;
    }
    return v;
  };
  if constexpr (L == 1) {
    // groups of up to 32 positions: the head's values stay in registers between the passes -- one read and one write of the
    // data instead of two or three reads and two writes (same operations in the same order: the same bits).  Three sizes, so
    // that a group of two does not issue 32 loads.
    const int64_t len = b - a;
    auto in_registers = [&](auto rc) __attribute__((always_inline)) {
      constexpr int R = decltype(rc)::value;
      T xv[R], dv[R];
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const int64_t p = a + (u < len ? u : 0);
        xv[u] = x[base + p * inner];
        dv[u] = BACKWARD ? dy[base + p * inner] : T(0);
      }
      if constexpr (R <= 16) {
        pin_all(xv);
        if constexpr (BACKWARD) pin_all(dv);
      } else {
        T(&x0)[16] = reinterpret_cast<T(&)[16]>(xv[0]);
        T(&x1)[16] = reinterpret_cast<T(&)[16]>(xv[16]);
        pin_all(x0), pin_all(x1);
        if constexpr (BACKWARD) {
          T(&d0)[16] = reinterpret_cast<T(&)[16]>(dv[0]);
          T(&d1)[16] = reinterpret_cast<T(&)[16]>(dv[16]);
          pin_all(d0), pin_all(d1);
        }
      }
      if constexpr (BACKWARD) {
        T sum = 0;
#pragma unroll
        for (int u = 0; u < R; ++u)
          if (u < len) sum += xv[u] * dv[u];
#pragma unroll
        for (int u = 0; u < R; ++u)
          if (u < len) y[base + (a + u) * inner] = xv[u] * (dv[u] - sum);
      } else {
        T mx = type_lowest<T>();
#pragma unroll
        for (int u = 0; u < R; ++u)
          if (u < len) mx = mx < xv[u] ? xv[u] : mx;
        T sum = 0;
#pragma unroll
        for (int u = 0; u < R; ++u)
          if (u < len) {
            xv[u] = exp(xv[u] - mx);
            sum += xv[u];
          }
#pragma unroll
        for (int u = 0; u < R; ++u)
          if (u < len) y[base + (a + u) * inner] = xv[u] / sum;
      }
    };
    // (backward: two values per position -- 32 positions cost the kernel its occupancy: 2 per group 0.39 -> 0.55 ms)
    constexpr int RMAX = BACKWARD ? 16 : 32;
    if (live && len > 1 && len <= RMAX) {
      if (len <= 4) in_registers(std::integral_constant<int, 4>{});
      else if (len <= 16) in_registers(std::integral_constant<int, 16>{});
      else if constexpr (RMAX > 16) in_registers(std::integral_constant<int, 32>{});
      return;
    }
  }
  if constexpr (BACKWARD) {
    // x = out, dy = out_grad, y = in_grad (softmax_kernel.cpp:148-222)
    T sum = 0;
    if (live)
      for (int64_t p = a + lane; p < b; p += L) sum += x[base + p * inner] * dy[base + p * inner];
    if (L > 1) sum = reduce(sum, false);
    if (live)
      for (int64_t p = a + lane; p < b; p += L)
        y[base + p * inner] = x[base + p * inner] * (dy[base + p * inner] - sum);
  } else {
    if (live && b - a == 1) {  // single-element groups are exactly 1 (softmax_kernel.cpp:102-109)
      if (lane == 0) y[base + a * inner] = T(1);
      // (falls through the reductions below with an empty range)
    }
    const bool work = live && b - a != 1;
    // four positions per trip, their loads pinned together (a head's positions are a row apart: one load in flight per thread
    // left long groups of wide heads at 0.17 of HBM)
    auto walk = [&](auto&& body) __attribute__((always_inline)) {
      if (!work) return;
      if constexpr (L > 1) {   // (lanes share a group: a lane has few positions, a batch would be mostly clamped loads)
        for (int64_t p = a + lane; p < b; p += L) body(p, x[base + p * inner]);
        return;
      }
      constexpr int U = 4;
      for (int64_t p0 = a + lane; p0 < b; p0 += (int64_t)U * L) {
        T xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t p = p0 + (int64_t)u * L;
          xv[u] = x[base + (p < b ? p : p0) * inner];
        }
        pin_all(xv);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t p = p0 + (int64_t)u * L;
          if (p >= b) break;
          body(p, xv[u]);
        }
      }
    };
    T mx = type_lowest<T>();
    walk([&](int64_t, T v) { mx = mx < v ? v : mx; });  // std::max(max, v)
    if (L > 1) mx = reduce(mx, true);
    // (the exponentials are computed again in the last pass instead of being parked in `y`: x is read three times and y
    // written once, instead of two reads of x and two writes + one read of y)
    T sum = 0;
    walk([&](int64_t, T v) { sum += exp(v - mx); });
    if (L > 1) sum = reduce(sum, false);
    walk([&](int64_t p, T v) { y[base + p * inner] = exp(v - mx) / sum; });
  }
}

// Hub groups (more than `long_cut` positions) of both softmax kernels, one workgroup per group: the workgroups look at 256
// groups at a time; a hub's [positions, inner] block is contiguous per outer index, its columns are taken 256 at a time by
// 256 / width position lanes each, whose partial maxima / sums are combined through LDS in lane order (sums differ from the
// sequential order by rounding, like the L > 1 variants).
template <typename T, bool BACKWARD>
__global__ __launch_bounds__(256) void softmax_csr_long_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                               const int64_t* __restrict__ ptr, T* __restrict__ y,
                                                               int64_t outer, int64_t D, int64_t inner, int64_t groups,
                                                               int64_t long_cut) {
  __shared__ int64_t long_groups[256];
  __shared__ int n_long;
  __shared__ T part[256];
  __shared__ T colv[256];
  for (int64_t g0 = (int64_t)blockIdx.x * 256; g0 < groups; g0 += (int64_t)gridDim.x * 256) {
    if (threadIdx.x == 0) n_long = 0;
    __syncthreads();
    {
      const int64_t g = g0 + threadIdx.x;
      if (g < groups && ptr[g + 1] - ptr[g] > long_cut) long_groups[atomicAdd(&n_long, 1)] = g;
    }
    __syncthreads();
    const int cnt = n_long;
    for (int j = 0; j < cnt; ++j) {
      const int64_t g = long_groups[j];
      const int64_t a = ptr[g], b = ptr[g + 1];
      for (int64_t i = 0; i < outer; ++i) {
        for (int64_t s0 = 0; s0 < inner; s0 += 256) {
          const int width = (int)(inner - s0 < 256 ? inner - s0 : 256);
          const int EL = 256 / width;
          const int lane = (int)threadIdx.x / width, col = (int)threadIdx.x % width;
          const bool on = lane < EL;
          const int64_t base = i * D * inner + s0 + col;
          // column-wise reduction of the lanes' values: the result is in colv[col] for everybody
          auto combine = [&](T v, bool is_max) {
            part[threadIdx.x] = v;
            __syncthreads();
            if (on && lane == 0) {
              T r = v;
              for (int l = 1; l < EL; ++l) {
                const T o = part[l * width + col];
                r = is_max ? (r < o ? o : r) : r + o;
              }
              colv[col] = r;
            }
            __syncthreads();
            const T r = colv[on ? col : 0];
            __syncthreads();
            return r;
          };
          // 16 positions per trip, their loads in flight together (pin_all): one workgroup has the whole group to itself
          constexpr int U = 16;
          auto walk = [&](auto&& body) {
            if (!on) return;
            for (int64_t p0 = a + lane; p0 < b; p0 += (int64_t)U * EL) {
              T xv[U], dv[U];
#pragma unroll
              for (int u = 0; u < U; ++u) {
                const int64_t p = p0 + (int64_t)u * EL;
                const int64_t pc = p < b ? p : p0;
                xv[u] = x[base + pc * inner];
                dv[u] = BACKWARD ? dy[base + pc * inner] : T(0);
              }
              pin_all(xv);
              if constexpr (BACKWARD) pin_all(dv);
#pragma unroll
              for (int u = 0; u < U; ++u) {
                const int64_t p = p0 + (int64_t)u * EL;
                if (p >= b) break;
                body(p, xv[u], dv[u]);
              }
            }
          };
          if constexpr (BACKWARD) {
            T sum = 0;
            walk([&](int64_t, T xv, T dv) { sum += xv * dv; });
            sum = combine(sum, false);
            walk([&](int64_t p, T xv, T dv) { y[base + p * inner] = xv * (dv - sum); });
          } else {
            T mx = type_lowest<T>();
            walk([&](int64_t, T xv, T) { mx = mx < xv ? xv : mx; });
            mx = combine(mx, true);
            T sum = 0;
            walk([&](int64_t, T xv, T) { sum += exp(xv - mx); });
            sum = combine(sum, false);
            walk([&](int64_t p, T xv, T) { y[base + p * inner] = exp(xv - mx) / sum; });
          }
        }
      }
    }
    __syncthreads();
  }
}

// ---- small K: rows streamed through LDS ----------------------------------------------------------
// With K * sizeof(T) below a cache line, one thread per (row, column) reads 2-4 byte elements that lie
// a whole row apart from its neighbour's (0.35 TB/s at K = 1).  Here a workgroup owns 256 / K consecutive
// rows: their source range is one contiguous span, which is copied to LDS in chunks with fully coalesced
// loads; every thread then walks ITS row's part of the chunk in source order -- same operation order
// as the CPU kernel (bit-exact), HBM traffic = the span once.
// Hub rows (more than `long_cut` positions) are not streamed: the chunk loop jumps over their spans, their threads stand
// by, and the hub kernels take them (a thread walking 200 000 positions out of LDS: 7 ms of a 0.02 ms call).
struct StreamHubs {
  int64_t a[16], b[16];     // spans of this workgroup's (first 16) hub rows, in row order
  unsigned char flag[256];  // per row of the workgroup: longer than the cut
  int n;
};                          // (516 bytes: with kStreamValues below, five workgroups' LDS still fit a CU)
// every thread of the workgroup; `hub`: this thread's row is one (threads of the same row alike), `first`: its k == 0 thread.
// Returns the number of spans listed.  (The span of a 17th hub among one workgroup's rows is streamed like the short rows'
// and ignored.)  Only called when the workgroup's whole span is longer than the cut: most workgroups never pay its barriers.
__device__ __forceinline__ int stream_hubs_collect(StreamHubs& h, bool hub, bool first, int rl, int rpb, const int64_t* ip,
                                                   int64_t r0) {
  if (!__syncthreads_or(hub)) return 0;
  h.flag[threadIdx.x] = 0;
  __syncthreads();
  if (hub && first) h.flag[rl] = 1;
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int r = 0; r < rpb && n < 16; ++r)
      if (h.flag[r]) h.a[n] = ip[r0 + r], h.b[n] = ip[r0 + r + 1], ++n;
    h.n = n;
  }
  __syncthreads();
  return h.n;
}
// the next chunk [base, base + ce) of [.., b0) that touches none of the nh listed hub spans; false at the end (uniform over
// the workgroup)
__device__ __forceinline__ bool stream_next(const StreamHubs& h, int nh, int& hi, int64_t& base, int64_t& ce, int64_t b0,
                                            int64_t CE) {
  while (hi < nh && h.a[hi] <= base) {
    if (h.b[hi] > base) base = h.b[hi];
    ++hi;
  }
  if (base >= b0) return false;
  const int64_t lim = hi < nh ? h.a[hi] : b0;
  ce = lim - base < CE ? lim - base : CE;
  return true;
}

constexpr int kStreamValues = 8192 - 192;   // LDS values per chunk (32 KB of fp32 less what StreamHubs takes)
constexpr int kSoftmaxValues = 16384;  // softmax: bigger chunks so that typical spans need ONE pass over HBM
// (float64 backward: two images of 16384 doubles are 256 KB -- more LDS than a CU has; half the values)
template <typename T, bool BACKWARD>
constexpr int softmax_values() { return sizeof(T) == 8 && BACKWARD ? kSoftmaxValues / 2 : kSoftmaxValues; }

template <typename T, int OP>
__global__ __launch_bounds__(256) void segment_csr_stream_kernel(const T* __restrict__ src,
                                                                 const int64_t* __restrict__ indptr,
                                                                 T* __restrict__ out, int64_t* __restrict__ arg,
                                                                 int fresh, CsrShape s, int rpb, HubWs hw) {
  using acc_t = typename Math<T>::acc_t;
  __shared__ T buf[kStreamValues];
  __shared__ StreamHubs hubs;
  const int K = (int)s.K;
  const int rl = threadIdx.x / K, k = threadIdx.x % K;
  const int64_t bps = (s.rows + rpb - 1) / rpb;
  const int64_t slice = blockIdx.x / bps;
  const int64_t r0 = (blockIdx.x % bps) * rpb;
  const int64_t rN = r0 + rpb < s.rows ? r0 + rpb : s.rows;
  const int64_t* ip = indptr + slice * s.indptr_stride;
  const int64_t a0 = ip[r0], b0 = ip[rN];
  const int64_t row = r0 + rl;
  bool valid = rl < rpb && row < rN;
  int64_t a = valid ? ip[row] : 0, b = valid ? ip[row + 1] : 0;
  const int64_t n = slice * s.rows + row;
  int nh = 0;
  {
    const bool hub = valid && b - a > s.long_cut;
    if (b0 - a0 > s.long_cut) nh = stream_hubs_collect(hubs, hub, k == 0, rl, rpb, ip, r0);
    if (hub) {
      if (hw.counters && k == 0) hub_register(hw, n, b - a);
      valid = false, a = b = 0;
    }
  }
  acc_t acc = acc_t(0);
  int64_t best = s.E;
  if constexpr (OP == CSR_MIN || OP == CSR_MAX) acc = minmax_identity<T, OP>();
  if (valid && OP != CSR_MEAN && !fresh) acc = Math<T>::up(out[n * K + k]);
  const int64_t CE = kStreamValues / K;
  const T* sp = src + slice * s.E * K;
  int hi_ = 0;
  int64_t ce;
  for (int64_t base = a0; stream_next(hubs, nh, hi_, base, ce, b0, CE); base += ce) {
    const int64_t nv = ce * K;
    for (int64_t i = threadIdx.x; i < nv; i += 256) buf[i] = sp[base * K + i];
    __syncthreads();
    const int64_t lo = a > base ? a : base, hi = b < base + ce ? b : base + ce;
    for (int64_t e = lo; e < hi; ++e) {
      const acc_t v = Math<T>::up(buf[(e - base) * K + k]);
      if constexpr (OP == CSR_SUM || OP == CSR_MEAN) acc += v;
      else if constexpr (OP == CSR_MIN) { if (v < acc) { acc = v; best = e; } }
      else { if (v > acc) { acc = v; best = e; } }
    }
    __syncthreads();
  }
  if (!valid) return;
  if constexpr (OP == CSR_MEAN) {
    const int64_t len = b - a;
    out[n * K + k] = Math<T>::down(acc / (acc_t)(len > 0 ? len : 1));
  } else if constexpr (OP == CSR_SUM) {
    out[n * K + k] = Math<T>::down(acc);
  } else {
    out[n * K + k] = (fresh && best == s.E) ? Math<T>::down(acc_t(0)) : Math<T>::down(acc);
    arg[n * K + k] = best;
  }
}

// softmax over groups with small inner size, streamed the same way: when a workgroup's span fits one
// chunk the three passes (max, exp-sum, normalise) run from LDS -- one HBM read, one write; longer
// spans stream three times.  Per-head operation order = the CPU kernel's.
template <typename T, bool BACKWARD>
__global__ __launch_bounds__(256) void softmax_csr_stream_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                                 const int64_t* __restrict__ ptr, T* __restrict__ y,
                                                                 CsrShape s, int rpb) {
  extern __shared__ __attribute__((aligned(16))) char sm_raw[];
  __shared__ StreamHubs hubs;
  T* buf = reinterpret_cast<T*>(sm_raw);
  T* buf2 = buf + softmax_values<T, BACKWARD>();  // backward only
  const int K = (int)s.K;
  const int rl = threadIdx.x / K, k = threadIdx.x % K;
  const int64_t bps = (s.rows + rpb - 1) / rpb;
  const int64_t slice = blockIdx.x / bps;
  const int64_t r0 = (blockIdx.x % bps) * rpb;
  const int64_t rN = r0 + rpb < s.rows ? r0 + rpb : s.rows;
  const int64_t a0 = ptr[r0], b0 = ptr[rN];
  const int64_t row = r0 + rl;
  const bool valid = rl < rpb && row < rN;
  int64_t a = valid ? ptr[row] : 0, b = valid ? ptr[row + 1] : 0;
  int nh = 0;
  {
    const bool hub = valid && b - a > s.long_cut;   // softmax_csr_long_kernel's
    if (b0 - a0 > s.long_cut) nh = stream_hubs_collect(hubs, hub, k == 0, rl, rpb, ptr, r0);
    if (hub) a = b = 0;
  }
  const int64_t CE = softmax_values<T, BACKWARD>() / K;
  const T* xp = x + slice * s.E * K;
  const T* dp = BACKWARD ? dy + slice * s.E * K : nullptr;
  T* yp = y + slice * s.E * K;
  const bool single = b0 - a0 <= CE && nh == 0;
  const bool one = !BACKWARD && b - a == 1;  // single-element groups are exactly 1
  T mx = type_lowest<T>(), sum = T(0);
  // pass p: 0 = max (forward only), 1 = sum, 2 = write
  for (int pass = BACKWARD ? 1 : 0; pass < 3; ++pass) {
    int hi_ = 0;
    int64_t ce;
    for (int64_t base = a0; stream_next(hubs, nh, hi_, base, ce, b0, CE); base += ce) {
      const int64_t nv = ce * K;
      if (!single || pass == (BACKWARD ? 1 : 0)) {
        __syncthreads();
        for (int64_t i = threadIdx.x; i < nv; i += 256) {
          buf[i] = xp[base * K + i];
          if (BACKWARD) buf2[i] = dp[base * K + i];
        }
        __syncthreads();
      }
      const int64_t lo = a > base ? a : base, hi = b < base + ce ? b : base + ce;
      for (int64_t e = lo; e < hi; ++e) {
        const int64_t j = (e - base) * K + k;
        if constexpr (BACKWARD) {
          if (pass == 1) sum += buf[j] * buf2[j];
          else if (pass == 2) yp[e * K + k] = buf[j] * (buf2[j] - sum);
        } else {
          if (pass == 0) { const T v = buf[j]; mx = mx < v ? v : mx; }
          else if (pass == 1) { if (!one) sum += exp(buf[j] - mx); }
          else yp[e * K + k] = one ? T(1) : exp(buf[j] - mx) / sum;
        }
      }
    }
  }
}

// ---- host side: one pure plan per call, one stage that launches it ------------------------------------------------------------
// (the counters are cleared by a kernel, not by hipMemsetAsync: a 16-byte memset node between kernel nodes is what faulted on the
// first replay of a captured fused_scatter_reduce, DESIGN.md "HIP graphs")
__global__ void hub_clear_kernel(int* __restrict__ counters) {
  if (threadIdx.x < 4) counters[threadIdx.x] = 0;
}

// The families of a plan: the four reductions (CSR_SUM ... CSR_MAX), then
enum { CSR_GATHER = 4, CSR_SOFTMAX = 5, CSR_SOFTMAX_BWD = 6 };
enum class HubMode { kNone, kLong, kChunks, kChunksCombine };

// what the choice needs to know of an element type
struct CsrType {
  int size, acc_size;
  bool integral, softmax;   // softmax: float32 / float64
};
template <typename T>
constexpr CsrType csr_type() {
  return {(int)sizeof(T), (int)sizeof(typename Math<T>::acc_t), std::is_integral<T>::value,
          std::is_same<T, float>::value || std::is_same<T, double>::value};
}
inline int csr_type_of(int dtype, CsrType* t) { PYG_DISPATCH_ALL(dtype, (*t = csr_type<scalar_t>(), PYG_HIP_OK)); }

// A call as the choice sees it: plain numbers.  Softmax: leading = outer, rows = groups, E = D, K = inner.
struct CsrCall {
  int family;
  CsrType t;
  int64_t leading, rows, E, K;
  bool perm;            // rows are read through a permutation (the sort-based scatter)
  unsigned misalign;    // low four bits of src | out
  unsigned ws_low;      // low eight bits of the offered scratch's address ...
  size_t ws_bytes;      // ... and its size (0: none)
  int num_cus;
};

// What a call is made of: pyg_hip_csr_route answers it, pyg_hip_csr_last_route reports it, the launch code follows it.
struct CsrPlan {
  int family = 0;
  CsrKernel kernel = CsrKernel::kNone;   // kNone: an empty call, or `unsupported`
  bool unsupported = false;
  int V = 1, L = 1, rpb = 0;             // elements per thread, lanes per item; stream: rows per workgroup
  int64_t cut = INT64_MAX;               // rows of more positions are hubs (INT64_MAX: no row can be one)
  HubMode hub = HubMode::kNone;
  HubLayout lay;                         // kChunks / kChunksCombine: the scratch, lay.CH positions per chunk
  int64_t row_grid = 0, long_grid = 0, chunk_grid = 0, combine_grid = 0;
  size_t ws_need = 0;                    // pyg_hip_csr_hub_workspace_size
};

// ---- the thresholds of the choice (with kHubCut, kHubCutStream and kNarrowVecLanesAvg of csr_rows.h) -------------------------
// rows of less than 64 bytes that are not very long on average take the LDS-streamed kernel (a thread walks its row out of LDS:
// from ~64 positions per row on, lanes over the positions are faster)
#ifndef PYG_CSR_STREAM_MAX_AVG
#define PYG_CSR_STREAM_MAX_AVG 64
#endif
constexpr int64_t kStreamMaxAvg = PYG_CSR_STREAM_MAX_AVG;
#ifndef PYG_CSR_STREAM_MAX_ROW_BYTES
#define PYG_CSR_STREAM_MAX_ROW_BYTES 64
#endif
constexpr int64_t kStreamMaxRowBytes = PYG_CSR_STREAM_MAX_ROW_BYTES;
// (rows of fewer than 12 positions on average: one thread per (row, element) on global memory is 1.3 - 2 x faster than the
// workgroup's trip through LDS -- fp32 K = 1, 2 per row: 0.088 -> 0.049 ms; K = 5, 8 per row: 0.194 -> 0.104)
#ifndef PYG_CSR_STREAM_MIN_AVG
#define PYG_CSR_STREAM_MIN_AVG 12
#endif
constexpr int64_t kStreamMinAvg = PYG_CSR_STREAM_MIN_AVG;
// (rows of whole 16-byte slices the row kernel can load as such: then the row kernel always wins -- fp32 K = 8, 2 positions
// per row, 16 M positions: 0.71 ms streamed, 0.15 direct; 48 per row: 0.22 streamed, 0.14 with one lane per item, 0.095 with
// eight; `tools/narrow_row_kernels.py`.  They stream only if narrow8 is pushed out to 64 positions per row, and then from 32
// positions per row on and below 32 bytes)
constexpr int64_t kStreamSlicesMaxRowBytes = 32, kStreamSlicesMinAvg = 32;
// gather, narrow rows: a thread writing its slice of position after position leaves 16 bytes per row and store instruction;
// with 8 lanes per item a store covers 8 consecutive positions.  Rows of whole 16-byte slices from 8 positions per row on (fp32
// K = 4, 16 per row, 16 M positions: 0.213 -> 0.092 ms; K = 12, 48 per row: 0.46 -> 0.22), element-wise rows from 32 (K = 1, 48
// per row: 0.062 -> 0.039; at 16 per row K = 5 loses: 0.154 -> 0.212): `tools/lease/ab_gather_lanes.sh`
constexpr int64_t kGatherLanesAvgSlices = 8, kGatherLanesAvg = 32;
// softmax, the LDS-streamed kernel: inner sizes below 32 bytes in groups of 33 ... 63 positions on average (shorter groups stay
// in the registers of the one-thread-per-head kernel: inner = 1, 16 per group 0.161 -> 0.114 ms).  Shorter groups and wider
// heads are faster with one thread per head reading global memory (fp32 inner = 8, 2 per group, 8 M positions: 1.32 -> 0.55 ms
// forward, 1.52 -> 0.39 backward; inner = 1, 2 per group: 0.37 -> 0.14; but inner = 1, 16 per group: 0.16 streamed, 0.35
// direct; `tools/narrow_softmax_kernels.py`)
#ifndef PYG_SOFTMAX_STREAM_MIN_AVG
#define PYG_SOFTMAX_STREAM_MIN_AVG 33
#endif
constexpr int64_t kSoftmaxStreamMinAvg = PYG_SOFTMAX_STREAM_MIN_AVG;
// (backward keeps two values per position: 16 in registers, so the streamed kernel takes over earlier)
constexpr int64_t kSoftmaxBwdStreamMinAvg = 12;
constexpr int64_t kSoftmaxStreamMaxRowBytes = 32;

// a call that launches nothing
inline bool csr_empty(int family, int64_t leading, int64_t rows, int64_t E, int64_t K) {
  return leading * rows * K == 0 || (family >= CSR_GATHER && E == 0);
}

// THE choice: the table of pyg_hip_csr_route in pyg_hip.h.  Pure: no HIP call, no global.
inline CsrPlan csr_plan(const CsrCall& c) {
  CsrPlan p;
  p.family = c.family;
  const bool gather = c.family == CSR_GATHER, softmax = c.family >= CSR_SOFTMAX;
  if (c.family < 0 || c.family > CSR_SOFTMAX_BWD) return p.unsupported = true, p;
  const bool minmax = c.family == CSR_MIN || c.family == CSR_MAX;
  const size_t acc_bytes = gather ? 0 : (size_t)c.t.acc_size;   // (gather keeps no partial results)
  if (HubLayout need; !softmax && c.K > 0 && hub_layout(c.leading * c.E, c.K, acc_bytes, minmax, true, 0, 0, &need))
    p.ws_need = need.bytes + 256;   // + alignment slack
  if (csr_empty(c.family, c.leading, c.rows, c.E, c.K)) return p;
  if ((c.family == CSR_MEAN && c.t.integral) || (softmax && !c.t.softmax)) return p.unsupported = true, p;

  const int64_t units = c.leading * c.rows;   // rows of all slices
  const int64_t avg = c.leading * c.E / units;
  const int64_t row_bytes = c.K * c.t.size;
  const int vmax = 16 / c.t.size;
  p.V = !softmax && vmax > 1 && c.K % vmax == 0 && c.misalign % 16 == 0 ? vmax : 1;   // 16-byte slices or elements
  bool stream = !gather && !c.perm && c.K <= 16 && row_bytes < kStreamMaxRowBytes && avg >= kStreamMinAvg && avg < kStreamMaxAvg &&
                c.leading * ((c.rows + 255) / 256) < (1ll << 31);
  if (p.V > 1) stream = stream && row_bytes < kStreamSlicesMaxRowBytes && avg >= kStreamSlicesMinAvg && kNarrowVecLanesAvg >= 64;
  if (softmax)
    stream = stream && row_bytes < kSoftmaxStreamMaxRowBytes &&
             avg >= (c.family == CSR_SOFTMAX_BWD ? kSoftmaxBwdStreamMinAvg : kSoftmaxStreamMinAvg);
  int64_t cut;
  if (stream) {
    p.kernel = CsrKernel::kStream, p.V = 1;
    p.rpb = 256 / (int)c.K;
    p.row_grid = c.leading * ((c.rows + p.rpb - 1) / p.rpb);
    cut = kHubCutStream;
  } else {
    const int64_t items = units * (c.K / p.V);
    p.kernel = pick_row_kernel(items, c.leading * c.E, units, c.num_cus, row_bytes);
    if (gather && p.kernel == CsrKernel::kRow1 && row_bytes < 64 && avg >= (p.V > 1 ? kGatherLanesAvgSlices : kGatherLanesAvg))
      p.kernel = CsrKernel::kNarrow8;
    p.L = kernel_lanes(p.kernel);
    p.row_grid = (items * p.L + 255) / 256;
    cut = kHubCut * (int64_t)p.L;
  }
  // hubs: a group of softmax lies in one slice's ptr, which all slices share
  const int64_t hub_rows = softmax ? c.rows : units;
  if (c.E <= cut || hub_rows <= 1) return p;   // no row can be that long: nothing is launched for them
  p.cut = cut;
  p.hub = HubMode::kLong;
  p.long_grid = std::min<int64_t>((hub_rows + 255) / 256, (int64_t)c.num_cus * 8);
  if (!softmax && hub_layout(c.leading * c.E, c.K, acc_bytes, minmax, false, c.ws_low, c.ws_bytes, &p.lay)) {
    p.chunk_grid = std::min<int64_t>(p.lay.max_chunks, (int64_t)c.num_cus * 8);
    if (!gather && c.E > p.lay.CH) {   // (else every hub is one chunk long)
      p.hub = HubMode::kChunksCombine;
      const int64_t max_hubs = c.leading * c.E / cut;   // every hub is longer than the cut
      p.combine_grid = std::min<int64_t>((max_hubs * (c.K / p.V) + 255) / 256, (int64_t)c.num_cus * 4);
    } else {
      p.hub = HubMode::kChunks;
    }
  }
  return p;
}

// '<segment|gather|softmax|softmax_bwd> <kernel> v<V> <none|long|chunks|chunks+combine>[ ch<CH>]', 'none' or 'unsupported'
inline void plan_name(const CsrPlan& p, char* buf, size_t n) {
  static const char* const kKernels[] = {"none", "row1", "narrow8", "lanes8", "lanes64", "stream"};
  static const char* const kHubs[] = {"none", "long", "chunks", "chunks+combine"};
  if (p.kernel == CsrKernel::kNone) {
    snprintf(buf, n, "%s", p.unsupported ? "unsupported" : "none");
    return;
  }
  const char* family = p.family < CSR_GATHER ? "segment" : p.family == CSR_GATHER ? "gather"
                       : p.family == CSR_SOFTMAX ? "softmax" : "softmax_bwd";
  const int len = snprintf(buf, n, "%s %s v%d %s", family, kKernels[(int)p.kernel], p.V, kHubs[(int)p.hub]);
  if (p.hub >= HubMode::kChunks) snprintf(buf + len, n - len, " ch%lld", (long long)p.lay.CH);
}

// pyg_hip_csr_last_route(): the plan of the last CSR launch on this thread (named when asked for, not on every launch)
thread_local CsrPlan g_last_plan;
inline void note_plan(const CsrPlan& p) { g_last_plan = p; }
inline int note_empty() {
  note_plan(CsrPlan{});
  return PYG_HIP_OK;
}
// (softmax of a dtype other than float32 / float64: there is no type to plan with)
inline int softmax_unsupported(const char* op, int dtype) {
  CsrPlan p;
  p.unsupported = true;
  note_plan(p);
  return fail(PYG_HIP_ERR_INVALID, "%s: float32 / float64 only (dtype %d)", op, dtype);
}

// the plan of a launch, noted.  `s` carries the caller's scratch; a, b: the two buffers read or written 16 bytes at a time
template <typename T>
CsrPlan plan_launch(int family, const CsrShape& s, bool perm, const void* a, const void* b) {
  const CsrCall c{family, csr_type<T>(), s.leading, s.rows, s.E, s.K, perm,
                  (unsigned)((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15),
                  (unsigned)(reinterpret_cast<uintptr_t>(s.hub_ws) & 255), s.hub_ws ? s.hub_ws_bytes : 0, device_info().num_cus};
  const CsrPlan p = csr_plan(c);
  note_plan(p);
  return p;
}

// the shape as the kernels get it: the plan's cut, no host-side scratch
inline CsrShape kernel_shape(const CsrShape& s, const CsrPlan& p) {
  CsrShape sc = s;
  sc.hub_ws = nullptr, sc.hub_ws_bytes = 0;
  sc.long_cut = p.cut;
  return sc;
}
inline HubWs plan_scratch(const CsrPlan& p, void* ws) { return p.hub >= HubMode::kChunks ? hub_bind(p.lay, ws) : HubWs{}; }

// f(integral_constant<int, L>) for the plan's lanes per item
template <typename F>
void with_lanes(int L, F f) {
  if (L == 64) f(std::integral_constant<int, 64>{});
  else if (L == 8) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 1>{});
}

// The launches of a plan, for every family: clear the counters of the scratch, run the row kernel -- it skips the hub rows
// and, with scratch, registers them --, then deal the hubs' chunks to all workgroups and combine their partial results, or,
// without scratch, find the hubs again and give each to one workgroup (`*_long`).  row() launches the plan's row kernel;
// chunk / combine / lng launch theirs on the grid they are given.
template <typename Row, typename Chunk, typename Combine, typename Long>
int run_plan(const CsrPlan& p, const HubWs& hw, hipStream_t stream, Row row, Chunk chunk, Combine combine, Long lng) {
  if (p.hub >= HubMode::kChunks) {
    hipLaunchKernelGGL(hub_clear_kernel, dim3(1), dim3(64), 0, stream, hw.counters);
    PYG_HIP_CHECK(hipGetLastError());
  }
  row();
  PYG_HIP_CHECK(hipGetLastError());
  if (p.hub >= HubMode::kChunks) {
    chunk(dim3((unsigned)p.chunk_grid));
    PYG_HIP_CHECK(hipGetLastError());
    if (p.hub == HubMode::kChunksCombine) combine(dim3((unsigned)p.combine_grid));
  } else if (p.hub == HubMode::kLong) {
    lng(dim3((unsigned)p.long_grid));
  }
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

template <typename T, int OP, bool PERM, int V>
int launch_segment(const CsrPlan& p, const T* sp, const int64_t* indptr, const int64_t* perm, T* op, int64_t* arg, int fresh,
                   const CsrShape& s, hipStream_t stream) {
  const CsrShape sc = kernel_shape(s, p);
  const HubWs hw = plan_scratch(p, s.hub_ws);
  const dim3 grid((unsigned)p.row_grid), block(256);
  return run_plan(
      p, hw, stream,
      [&] {
        if constexpr (!PERM && V == 1) {
          if (p.kernel == CsrKernel::kStream) {
            hipLaunchKernelGGL((segment_csr_stream_kernel<T, OP>), grid, block, 0, stream, sp, indptr, op, arg, fresh, sc, p.rpb, hw);
            return;
          }
        }
        with_lanes(p.L, [&](auto l) {
          hipLaunchKernelGGL((segment_csr_kernel<T, OP, V, decltype(l)::value, PERM>), grid, block, 0, stream, sp, indptr, perm, op,
                             arg, fresh, sc, hw);
        });
      },
      [&](dim3 g) {
        hipLaunchKernelGGL((segment_csr_hub_chunk_kernel<T, OP, V, PERM>), g, block, 0, stream, sp, indptr, perm, op, arg, fresh, sc, hw);
      },
      [&](dim3 g) {
        hipLaunchKernelGGL((segment_csr_hub_combine_kernel<T, OP, V>), g, block, 0, stream, indptr, op, arg, fresh, sc, hw);
      },
      [&](dim3 g) {
        hipLaunchKernelGGL((segment_csr_long_kernel<T, OP, V, PERM>), g, block, 0, stream, sp, indptr, perm, op, arg, fresh, sc);
      });
}

// a reduction over plain rows (perm == nullptr) or over rows read through perm[] (never streamed, no mean)
template <typename T>
int run_segment(int op, const void* src, const int64_t* indptr, const int64_t* perm, void* out, int64_t* arg, int fresh,
                const CsrShape& s, hipStream_t stream) {
  constexpr int VMAX = 16 / (int)sizeof(T);
  const CsrPlan p = plan_launch<T>(op, s, perm != nullptr, src, out);
  const T* sp = static_cast<const T*>(src);
  T* dp = static_cast<T*>(out);
#define PYG_CSR_OP(OPC, PERM)                                                                       \
  (p.V > 1 ? launch_segment<T, OPC, PERM, VMAX>(p, sp, indptr, perm, dp, arg, fresh, s, stream)     \
           : launch_segment<T, OPC, PERM, 1>(p, sp, indptr, perm, dp, arg, fresh, s, stream))
  switch (op) {
    case CSR_SUM: return perm ? PYG_CSR_OP(CSR_SUM, true) : PYG_CSR_OP(CSR_SUM, false);
    case CSR_MEAN:
      if constexpr (std::is_integral<T>::value) return fail(PYG_HIP_ERR_INVALID, "segment_mean_csr: floating dtypes only");
      else return PYG_CSR_OP(CSR_MEAN, false);
    case CSR_MIN: return perm ? PYG_CSR_OP(CSR_MIN, true) : PYG_CSR_OP(CSR_MIN, false);
    case CSR_MAX: return perm ? PYG_CSR_OP(CSR_MAX, true) : PYG_CSR_OP(CSR_MAX, false);
    default: return fail(PYG_HIP_ERR_INVALID, "segment_csr: unknown reduction %d", op);
  }
#undef PYG_CSR_OP
}

template <typename T, int V>
int launch_gather(const CsrPlan& p, const T* sp, const int64_t* indptr, T* op, const CsrShape& s, hipStream_t stream) {
  const CsrShape sc = kernel_shape(s, p);
  const HubWs hw = plan_scratch(p, s.hub_ws);
  const dim3 grid((unsigned)p.row_grid), block(256);
  return run_plan(
      p, hw, stream,
      [&] {
        with_lanes(p.L, [&](auto l) {
          hipLaunchKernelGGL((gather_csr_kernel<T, V, decltype(l)::value>), grid, block, 0, stream, sp, indptr, op, sc, hw);
        });
      },
      [&](dim3 g) { hipLaunchKernelGGL((gather_csr_hub_chunk_kernel<T, V>), g, block, 0, stream, sp, indptr, op, sc, hw); },
      [](dim3) {},   // (no partial results)
      [&](dim3 g) { hipLaunchKernelGGL((gather_csr_long_kernel<T, V>), g, block, 0, stream, sp, indptr, op, sc); });
}

template <typename T>
int run_gather_csr(const void* src, const int64_t* indptr, void* out, const CsrShape& s, hipStream_t stream) {
  constexpr int VMAX = 16 / (int)sizeof(T);
  const CsrPlan p = plan_launch<T>(CSR_GATHER, s, false, src, out);
  const T* sp = static_cast<const T*>(src);
  T* op = static_cast<T*>(out);
  return p.V > 1 ? launch_gather<T, VMAX>(p, sp, indptr, op, s, stream) : launch_gather<T, 1>(p, sp, indptr, op, s, stream);
}

template <typename T, bool BACKWARD>
int run_softmax(const void* x_, const void* dy_, const int64_t* ptr, void* y_, int64_t outer, int64_t D, int64_t inner,
                int64_t groups, hipStream_t stream) {
  const CsrShape s{outer, groups, D, inner, 0};
  const CsrPlan p = plan_launch<T>(BACKWARD ? CSR_SOFTMAX_BWD : CSR_SOFTMAX, s, false, nullptr, nullptr);
  const T *x = static_cast<const T*>(x_), *dy = static_cast<const T*>(dy_);
  T* y = static_cast<T*>(y_);
  const int lds = (int)(sizeof(T) * softmax_values<T, BACKWARD>() * (BACKWARD ? 2 : 1));
  if (p.kernel == CsrKernel::kStream)
    if (int rc_ = ensure_dynamic_lds(reinterpret_cast<const void*>(&softmax_csr_stream_kernel<T, BACKWARD>), lds)) return rc_;
  const dim3 grid((unsigned)p.row_grid), block(256);
  return run_plan(
      p, HubWs{}, stream,
      [&] {
        if (p.kernel == CsrKernel::kStream) {
          hipLaunchKernelGGL((softmax_csr_stream_kernel<T, BACKWARD>), grid, block, lds, stream, x, dy, ptr, y, kernel_shape(s, p), p.rpb);
          return;
        }
        with_lanes(p.L, [&](auto l) {
          hipLaunchKernelGGL((softmax_csr_kernel<T, decltype(l)::value, BACKWARD>), grid, block, 0, stream, x, dy, ptr, y, outer, D,
                             inner, groups, p.cut);
        });
      },
      [](dim3) {}, [](dim3) {},   // (no scratch: the hub groups always go to the *_long kernel)
      [&](dim3 g) {
        hipLaunchKernelGGL((softmax_csr_long_kernel<T, BACKWARD>), g, block, 0, stream, x, dy, ptr, y, outer, D, inner, groups, p.cut);
      });
}

}  // namespace

int segment_csr_sum(int dtype, const void* src, const int64_t* indptr, int64_t indptr_stride, const int64_t* perm, void* out,
                    int64_t leading, int64_t rows, int64_t E, int64_t K, int fresh, hipStream_t stream, void* hub_ws,
                    size_t hub_ws_bytes) {
  if (csr_empty(CSR_SUM, leading, rows, E, K)) return note_empty();
  CsrShape s{leading, rows, E, K, indptr_stride};
  s.hub_ws = hub_ws, s.hub_ws_bytes = hub_ws_bytes;
  PYG_DISPATCH_ALL(dtype, (run_segment<scalar_t>(CSR_SUM, src, indptr, perm, out, nullptr, fresh, s, stream)));
}

int segment_csr_minmax(int is_min, int dtype, const void* src, const int64_t* indptr, int64_t indptr_stride,
                       const int64_t* perm, void* out, int64_t* arg, int fresh, int64_t leading, int64_t rows,
                       int64_t E, int64_t K, hipStream_t stream, void* hub_ws, size_t hub_ws_bytes) {
  if (csr_empty(CSR_MIN, leading, rows, E, K)) return note_empty();
  CsrShape s{leading, rows, E, K, indptr_stride};
  s.hub_ws = hub_ws, s.hub_ws_bytes = hub_ws_bytes;
  PYG_DISPATCH_ALL(dtype, (run_segment<scalar_t>(is_min ? CSR_MIN : CSR_MAX, src, indptr, perm, out, arg, fresh, s, stream)));
}

}  // namespace pyg_hip

using namespace pyg_hip;

extern "C" {

const char* pyg_hip_csr_route(int family, int dtype, int64_t leading, int64_t rows, int64_t E, int64_t K, int flags,
                              size_t workspace_bytes, unsigned misalign, int num_cus) {
  thread_local char name[64];
  CsrCall c{family, {}, leading, rows, E, K, (flags & 1) != 0, misalign & 15, (misalign >> 8) & 255, workspace_bytes, num_cus};
  CsrPlan p;
  if (leading < 0 || rows < 0 || E < 0 || K < 0 || num_cus < 0 || csr_type_of(dtype, &c.t) != PYG_HIP_OK) {
    p.unsupported = true;
  } else {
    if (num_cus == 0) c.num_cus = device_info().num_cus;
    p = csr_plan(c);
  }
  plan_name(p, name, sizeof(name));
  return name;
}

const char* pyg_hip_csr_last_route(void) {
  thread_local char name[64];
  plan_name(g_last_plan, name, sizeof(name));
  return name;
}

size_t pyg_hip_csr_hub_workspace_size(int op, int dtype, int64_t leading, int64_t E, int64_t K) {
  CsrCall c{op, {}, leading, 0, E, K, false, 0, 0, 0, 0};
  if (leading < 0 || E < 0 || K <= 0 || op < 0 || op > CSR_GATHER || csr_type_of(dtype, &c.t) != PYG_HIP_OK) return 0;
  return csr_plan(c).ws_need;
}

int pyg_hip_segment_csr_ws(int op, int dtype, const void* src, const int64_t* indptr, int64_t indptr_slice_stride,
                           void* out, int64_t* arg_out, int fresh, int64_t leading, int64_t rows, int64_t E, int64_t K,
                           void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PYG_HIP_REQUIRE(leading >= 0 && rows >= 0 && E >= 0 && K >= 0, "segment_csr: negative size");
  if (csr_empty(CSR_SUM, leading, rows, E, K)) return note_empty();
  PYG_HIP_REQUIRE(op >= CSR_SUM && op <= CSR_MAX, "segment_csr: unknown reduction %d", op);
  PYG_HIP_REQUIRE(indptr && out && (src || E == 0), "segment_csr: NULL tensor");
  PYG_HIP_REQUIRE((op != CSR_MIN && op != CSR_MAX) || arg_out, "segment_csr: min/max need arg_out");
  PYG_HIP_REQUIRE(indptr_slice_stride == 0 || indptr_slice_stride >= rows + 1, "segment_csr: bad indptr stride");
  CsrShape s{leading, rows, E, K, indptr_slice_stride};
  s.hub_ws = workspace, s.hub_ws_bytes = workspace ? workspace_bytes : 0;
  PYG_DISPATCH_ALL(dtype, (run_segment<scalar_t>(op, src, indptr, nullptr, out, arg_out, fresh, s, stream)));
}

int pyg_hip_segment_csr(int op, int dtype, const void* src, const int64_t* indptr, int64_t indptr_slice_stride,
                        void* out, int64_t* arg_out, int fresh, int64_t leading, int64_t rows, int64_t E, int64_t K,
                        void* stream_) {
  return pyg_hip_segment_csr_ws(op, dtype, src, indptr, indptr_slice_stride, out, arg_out, fresh, leading, rows, E, K, nullptr, 0,
                                stream_);
}

int pyg_hip_gather_csr_ws(int dtype, const void* src, const int64_t* indptr, int64_t indptr_slice_stride, void* out,
                          int64_t leading, int64_t rows, int64_t E, int64_t K, void* workspace, size_t workspace_bytes,
                          void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PYG_HIP_REQUIRE(leading >= 0 && rows >= 0 && E >= 0 && K >= 0, "gather_csr: negative size");
  if (csr_empty(CSR_GATHER, leading, rows, E, K)) return note_empty();
  PYG_HIP_REQUIRE(src && indptr && out, "gather_csr: NULL tensor");
  CsrShape s{leading, rows, E, K, indptr_slice_stride};
  s.hub_ws = workspace, s.hub_ws_bytes = workspace ? workspace_bytes : 0;
  PYG_DISPATCH_ALL(dtype, (run_gather_csr<scalar_t>(src, indptr, out, s, stream)));
}

int pyg_hip_gather_csr(int dtype, const void* src, const int64_t* indptr, int64_t indptr_slice_stride, void* out,
                       int64_t leading, int64_t rows, int64_t E, int64_t K, void* stream_) {
  return pyg_hip_gather_csr_ws(dtype, src, indptr, indptr_slice_stride, out, leading, rows, E, K, nullptr, 0, stream_);
}

int pyg_hip_softmax_csr(int dtype, const void* src, const int64_t* ptr, void* out, int64_t outer, int64_t D,
                        int64_t inner, int64_t groups, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PYG_HIP_REQUIRE(outer >= 0 && D >= 0 && inner >= 0 && groups >= 0, "softmax_csr: negative size");
  if (csr_empty(CSR_SOFTMAX, outer, groups, D, inner)) return note_empty();
  PYG_HIP_REQUIRE(src && ptr && out, "softmax_csr: NULL tensor");
  if (dtype == PYG_F32) return run_softmax<float, false>(src, nullptr, ptr, out, outer, D, inner, groups, stream);
  if (dtype == PYG_F64) return run_softmax<double, false>(src, nullptr, ptr, out, outer, D, inner, groups, stream);
  return softmax_unsupported("softmax_csr", dtype);
}

int pyg_hip_softmax_csr_backward(int dtype, const void* out, const void* out_grad, const int64_t* ptr, void* in_grad,
                                 int64_t outer, int64_t D, int64_t inner, int64_t groups, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PYG_HIP_REQUIRE(outer >= 0 && D >= 0 && inner >= 0 && groups >= 0, "softmax_csr_backward: negative size");
  if (csr_empty(CSR_SOFTMAX_BWD, outer, groups, D, inner)) return note_empty();
  PYG_HIP_REQUIRE(out && out_grad && ptr && in_grad, "softmax_csr_backward: NULL tensor");
  if (dtype == PYG_F32) return run_softmax<float, true>(out, out_grad, ptr, in_grad, outer, D, inner, groups, stream);
  if (dtype == PYG_F64) return run_softmax<double, true>(out, out_grad, ptr, in_grad, outer, D, inner, groups, stream);
  return softmax_unsupported("softmax_csr_backward", dtype);
}

}  // extern "C"
