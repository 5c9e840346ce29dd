// fused_scatter_reduce for gfx950 (MI355X): sum, mean, min and max of one [E, F] input over one unsorted index in ONE stable
// sort and ONE pass over the rows, and its one-pass backward.
//
// Replaces pyg_lib/ops/scatter_reduce.py:95-181 (a Triton kernel: up to four float atomics per element, no backward, no
// `out=`).  Four separate pyg::scatter_* calls on a large index each sort the E indices, build the row offsets and read every
// source row once through the permutation (reduce.hip, run_scatter); nothing but the output slice differs between them.  Here:
//   * index_sort_i64 once (stable: a bucket's positions stay in source order), the row offsets once by binary search; the
//     count of a bucket is the difference of two offsets;
//   * one thread (or L lanes, pick_lanes) per (bucket, 16-byte slice) walks the bucket through the permutation with up to
//     three accumulator sets per element -- sum (shared by sum and mean), min, max -- in Math<T>::acc_t; which sets exist is
//     the template mask, so an unwanted one costs no register.  Every source row is loaded once, U positions' permutation
//     entries and rows in flight together (pin_all);
//   * first-match positions are tracked as 32-bit offsets inside the bucket and translated through the permutation once, and
//     only when the caller wants them (or lanes share a bucket: a tie between +0 and -0 goes to the earlier position);
//   * buckets of more than kHubCut positions per lane are registered in scratch, cut into chunks dealt to all workgroups, and
//     combined in chunk order by a third launch (the scheme of csr.hip, with three partial results and two positions);
//   * no atomics on values: the same bits on every run; one rounding on store.
// Rows that are no multiple of 16 bytes, or unaligned bases, take the one-element-per-thread instances (V = 1).
#include "common.h"
#include "csr_rows.h"
#include "elem.h"

#include <algorithm>
#include <cstdint>
#include <type_traits>

namespace pyg_hip {
namespace {

enum { F_SUM = PYG_FUSED_SUM, F_MEAN = PYG_FUSED_MEAN, F_MIN = PYG_FUSED_MIN, F_MAX = PYG_FUSED_MAX };
enum { ACC_SUM = 1, ACC_MIN = 2, ACC_MAX = 4 };   // bits of MASK: the accumulator sets a kernel instance carries
constexpr uint32_t kNoOff = 0xffffffffu;          // "no position yet" as a 32-bit offset: loses every tie

struct FusedShape {
  int64_t E, N, F;
  int64_t ostride;   // elements per output row: R * F
  int64_t col[4];    // first column of the sum / mean / min / max slice in an output row, -1: not wanted
  int64_t long_cut = INT64_MAX;
};

// a longer hub's partial results: slot (hub.slot_base + chunk), F values each
template <typename A>
struct FusedPartial {
  int64_t *bmin = nullptr, *bmax = nullptr;   // source positions (E: none)
  A *sum = nullptr, *mn = nullptr, *mx = nullptr;
};

template <typename T>
__device__ __forceinline__ typename Math<T>::acc_t min_start() { return Math<T>::up(type_max<T>()); }
template <typename T>
__device__ __forceinline__ typename Math<T>::acc_t max_start() { return Math<T>::up(type_lowest<T>()); }

// first position e with keys[e] >= r (keys ascending): the row offsets of the sorted index.  The launch in front of the row
// kernel also clears the four hub counters (a kernel, not a memset: the call stays one chain of kernel nodes in a HIP graph)
__global__ void fused_indptr_kernel(const int64_t* __restrict__ keys, int64_t E, int64_t N, int64_t* __restrict__ indptr,
                                    int* __restrict__ hub_counters) {
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (hub_counters && r < 4) hub_counters[r] = 0;
  if (r > N) return;
  int64_t lo = 0, hi = E;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < r) lo = mid + 1; else hi = mid;
  }
  indptr[r] = lo;
}

// one (bucket, slice)'s results -> the wanted slices of its output row; `orow` = out + n * ostride + c.  A min / max that
// never beat its start value had no contribution (strict compares: every winner differs from it) and reads 0.
template <typename T, int MASK, int V>
__device__ __forceinline__ void fused_store(T* __restrict__ orow, const FusedShape& s, int64_t len,
                                            const typename Math<T>::acc_t (&sum)[V], const typename Math<T>::acc_t (&mn)[V],
                                            const typename Math<T>::acc_t (&mx)[V]) {
  using acc_t = typename Math<T>::acc_t;
  using P = Pack<T, V>;
  P r;
  if constexpr ((MASK & ACC_SUM) != 0) {
    if (s.col[F_SUM] >= 0) {
#pragma unroll
      for (int i = 0; i < V; ++i) r.v[i] = Math<T>::down(sum[i]);
      *reinterpret_cast<P*>(orow + s.col[F_SUM]) = r;
    }
    if (s.col[F_MEAN] >= 0) {
      const acc_t denom = (acc_t)(len > 0 ? len : 1);
#pragma unroll
      for (int i = 0; i < V; ++i) r.v[i] = Math<T>::down(sum[i] / denom);
      *reinterpret_cast<P*>(orow + s.col[F_MEAN]) = r;
    }
  }
  if constexpr ((MASK & ACC_MIN) != 0) {
#pragma unroll
    for (int i = 0; i < V; ++i) r.v[i] = Math<T>::down(mn[i] == min_start<T>() ? acc_t(0) : mn[i]);
    *reinterpret_cast<P*>(orow + s.col[F_MIN]) = r;
  }
  if constexpr ((MASK & ACC_MAX) != 0) {
#pragma unroll
    for (int i = 0; i < V; ++i) r.v[i] = Math<T>::down(mx[i] == max_start<T>() ? acc_t(0) : mx[i]);
    *reinterpret_cast<P*>(orow + s.col[F_MAX]) = r;
  }
}

// (value, position) pairs combine lexicographically: the better value, on a tie the earlier position
template <bool IS_MIN, typename A, typename B>
__device__ __forceinline__ void take_better(A& v, B& pos, A ov, B opos) {
  const bool better = IS_MIN ? ov < v : ov > v;
  const bool worse = IS_MIN ? v < ov : v > ov;
  if (better || (!worse && opos < pos)) v = ov, pos = opos;
}

// MASK: accumulator sets; ARG: arg_min / arg_max (whichever is not null) are written; V elements (16 bytes, or 1) per thread,
// L lanes per item.  count (optional) [N].
template <typename T, int MASK, bool ARG, int V, int L>
__global__ __launch_bounds__(256) void fused_rows_kernel(const T* __restrict__ src, const int64_t* __restrict__ indptr,
                                                         const int64_t* __restrict__ perm, T* __restrict__ out,
                                                         int64_t* __restrict__ arg_min, int64_t* __restrict__ arg_max,
                                                         int64_t* __restrict__ count, FusedShape s, HubWs hw) {
  using acc_t = typename Math<T>::acc_t;
  using P = Pack<T, V>;
  constexpr bool SUM = (MASK & ACC_SUM) != 0, MIN = (MASK & ACC_MIN) != 0, MAX = (MASK & ACC_MAX) != 0;
  constexpr bool TRK = (MIN || MAX) && (ARG || L > 1);   // positions are tracked
  const int64_t kv = s.F / V;
  const int64_t t = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / L;
  const int lane = threadIdx.x & (L - 1);
  const bool live = t < s.N * kv;
  const int64_t tt = live ? t : 0;
  const int64_t n = tt / kv;
  const int64_t c = (tt % kv) * V;
  const int64_t a = indptr[n], b = indptr[n + 1];
  const bool first = live && lane == 0 && c == 0;
  if (first && count) count[n] = b - a;
  if (b - a > s.long_cut) {   // (all L lanes of the item alike) a hub: fused_hub_chunk_kernel
    if (first) hub_register(hw, n, b - a);
    return;
  }
  const T* sp = src + c;

  acc_t sum[V], mn[V], mx[V];
  uint32_t omn[V], omx[V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    sum[i] = lane == 0 ? acc_t(0) : sum_identity<acc_t>();   // (a fresh output starts at +0: csr.hip)
    mn[i] = min_start<T>(), mx[i] = max_start<T>();
    omn[i] = omx[i] = kNoOff;
  }
  if (live) {
    constexpr int U = 4;
    for (int64_t e0 = a + lane; e0 < b; e0 += (int64_t)U * L) {
      int64_t pp[U];
      P xx[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t e = e0 + (int64_t)u * L;
        pp[u] = perm[e < b ? e : e0];   // clamped: the load is issued unconditionally, the value is ignored below
      }
      pin_all(pp);
#pragma unroll
      for (int u = 0; u < U; ++u) xx[u] = *reinterpret_cast<const P*>(sp + pp[u] * s.F);
      pin_all(xx);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t e = e0 + (int64_t)u * L;
        if (e >= b) break;
        const uint32_t off = (uint32_t)(e - a);
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const acc_t v = Math<T>::up(xx[u].v[i]);
          if constexpr (SUM) sum[i] += v;
          if constexpr (MIN) {
            if (v < mn[i]) {
              mn[i] = v;
              if constexpr (TRK) omn[i] = off;
            }
          }
          if constexpr (MAX) {
            if (v > mx[i]) {
              mx[i] = v;
              if constexpr (TRK) omx[i] = off;
            }
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
        if constexpr (SUM) sum[i] += shfl_xor_any(sum[i], m);
        if constexpr (MIN) take_better<true>(mn[i], omn[i], shfl_xor_any(mn[i], m), shfl_xor_any(omn[i], m));
        if constexpr (MAX) take_better<false>(mx[i], omx[i], shfl_xor_any(mx[i], m), shfl_xor_any(omx[i], m));
      }
    }
  }
  if (!live || lane != 0) return;
  fused_store<T, MASK, V>(out + n * s.ostride + c, s, b - a, sum, mn, mx);
  if constexpr (ARG) {
    if (MIN && arg_min) {
#pragma unroll
      for (int i = 0; i < V; ++i) arg_min[n * s.F + c + i] = omn[i] == kNoOff ? s.E : perm[a + omn[i]];
    }
    if (MAX && arg_max) {
#pragma unroll
      for (int i = 0; i < V; ++i) arg_max[n * s.F + c + i] = omx[i] == kNoOff ? s.E : perm[a + omx[i]];
    }
  }
}

// One registered chunk of a hub per workgroup and trip: S slices x 256 / S position lanes (HubGeom), eight loads in flight
// per thread, the lanes' partial results combined through LDS by a fixed pairwise tree.  A hub of one chunk is finished on the
// spot; the chunks of a longer one leave (sum, min, max, their positions) in the hub's slots.
template <typename T, int MASK, int V>
__global__ __launch_bounds__(256) void fused_hub_chunk_kernel(const T* __restrict__ src, const int64_t* __restrict__ indptr,
                                                              const int64_t* __restrict__ perm, T* __restrict__ out,
                                                              int64_t* __restrict__ arg_min, int64_t* __restrict__ arg_max,
                                                              FusedShape s, HubWs hw, FusedPartial<typename Math<T>::acc_t> fp) {
  using acc_t = typename Math<T>::acc_t;
  using P = Pack<T, V>;
  constexpr bool SUM = (MASK & ACC_SUM) != 0, MIN = (MASK & ACC_MIN) != 0, MAX = (MASK & ACC_MAX) != 0;
  constexpr int NA = (SUM ? 1 : 0) + (MIN ? 1 : 0) + (MAX ? 1 : 0), NB = (MIN ? 1 : 0) + (MAX ? 1 : 0);
  constexpr int I_MN = SUM ? 1 : 0, I_MX = I_MN + (MIN ? 1 : 0);   // planes of `part`; of `pbest`: 0 and MIN ? 1 : 0
  __shared__ acc_t part[NA * 256 * V];
  __shared__ uint32_t pbest[(NB ? NB : 1) * 256 * V];
  const int64_t kv = s.F / V;
  const HubGeom<T, V> g(kv);
  const int nchunks = hw.counters[3] ? 0 : hw.counters[1];
  for (int q = blockIdx.x; q < nchunks; q += gridDim.x) {
    const int2 cr = hw.chunks[q];
    const HubRec hub = hw.hubs[cr.x];
    const int64_t n = hub.n;
    const int64_t a = indptr[n], b = indptr[n + 1];
    const int64_t pa = a + (int64_t)cr.y * hw.CH, pb = pa + hw.CH < b ? pa + hw.CH : b;
    const int64_t slot = (int64_t)(hub.slot_base + cr.y) * s.F;
    for (int64_t c0 = 0; c0 < kv; c0 += g.S) {
      const int64_t ci = c0 + g.sl;
      const bool on = ci < kv;
      const int64_t c = (on ? ci : 0) * V;
      acc_t sum[V], mn[V], mx[V];
      uint32_t omn[V], omx[V];   // offsets from pa (a chunk has at most 2^22 positions)
#pragma unroll
      for (int i = 0; i < V; ++i) {
        sum[i] = sum_identity<acc_t>();   // (the row's +0 is added once, where the chunks meet)
        mn[i] = min_start<T>(), mx[i] = max_start<T>();
        omn[i] = omx[i] = kNoOff;
      }
      if (on) {
        constexpr int U = 8;
        const T* sp = src + c;
        for (int64_t e0 = pa + g.lane; e0 < pb; e0 += (int64_t)U * g.EL) {
          int64_t pp[U];
          P xx[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int64_t e = e0 + (int64_t)u * g.EL;
            pp[u] = perm[e < pb ? e : e0];
          }
          pin_all(pp);
#pragma unroll
          for (int u = 0; u < U; ++u) xx[u] = *reinterpret_cast<const P*>(sp + pp[u] * s.F);
          pin_all(xx);
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int64_t e = e0 + (int64_t)u * g.EL;
            if (e >= pb) break;
            const uint32_t off = (uint32_t)(e - pa);
#pragma unroll
            for (int i = 0; i < V; ++i) {
              const acc_t v = Math<T>::up(xx[u].v[i]);
              if constexpr (SUM) sum[i] += v;
              if constexpr (MIN) {
                if (v < mn[i]) mn[i] = v, omn[i] = off;
              }
              if constexpr (MAX) {
                if (v > mx[i]) mx[i] = v, omx[i] = off;
              }
            }
          }
        }
      }
      const int me = threadIdx.x * V;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        if constexpr (SUM) part[me + i] = sum[i];
        if constexpr (MIN) part[I_MN * 256 * V + me + i] = mn[i], pbest[me + i] = omn[i];
        if constexpr (MAX) part[I_MX * 256 * V + me + i] = mx[i], pbest[(MIN ? 1 : 0) * 256 * V + me + i] = omx[i];
      }
      __syncthreads();
      // the lanes of a slice combine pairwise, lane l with lane l + stride: a fixed tree, the same bits on every run
      for (int st = g.EL >> 1; st >= 1; st >>= 1) {
        if (g.lane < st) {
          const int ib = (((g.lane + st) << g.logS) + g.sl) * V;
#pragma unroll
          for (int i = 0; i < V; ++i) {
            if constexpr (SUM) part[me + i] += part[ib + i];
            if constexpr (MIN)
              take_better<true>(part[I_MN * 256 * V + me + i], pbest[me + i], part[I_MN * 256 * V + ib + i], pbest[ib + i]);
            if constexpr (MAX)
              take_better<false>(part[I_MX * 256 * V + me + i], pbest[(MIN ? 1 : 0) * 256 * V + me + i],
                                 part[I_MX * 256 * V + ib + i], pbest[(MIN ? 1 : 0) * 256 * V + ib + i]);
          }
        }
        __syncthreads();
      }
      if (on && g.lane == 0) {
        int64_t bmn[V], bmx[V];
#pragma unroll
        for (int i = 0; i < V; ++i) {
          if constexpr (SUM) sum[i] = part[me + i];
          if constexpr (MIN) {
            mn[i] = part[I_MN * 256 * V + me + i];
            const uint32_t o = pbest[me + i];
            bmn[i] = o == kNoOff ? s.E : perm[pa + o];
          }
          if constexpr (MAX) {
            mx[i] = part[I_MX * 256 * V + me + i];
            const uint32_t o = pbest[(MIN ? 1 : 0) * 256 * V + me + i];
            bmx[i] = o == kNoOff ? s.E : perm[pa + o];
          }
        }
        if (hub.nch == 1) {
#pragma unroll
          for (int i = 0; i < V; ++i) sum[i] = acc_t(0) + sum[i];
          fused_store<T, MASK, V>(out + n * s.ostride + c, s, b - a, sum, mn, mx);
#pragma unroll
          for (int i = 0; i < V; ++i) {
            if (MIN && arg_min) arg_min[n * s.F + c + i] = bmn[i];
            if (MAX && arg_max) arg_max[n * s.F + c + i] = bmx[i];
          }
        } else {
#pragma unroll
          for (int i = 0; i < V; ++i) {
            if constexpr (SUM) fp.sum[slot + c + i] = sum[i];
            if constexpr (MIN) fp.mn[slot + c + i] = mn[i], fp.bmin[slot + c + i] = bmn[i];
            if constexpr (MAX) fp.mx[slot + c + i] = mx[i], fp.bmax[slot + c + i] = bmx[i];
          }
        }
      }
      __syncthreads();
    }
  }
}

// ... and a third launch combines a longer hub's slots in chunk order: one thread per (hub, slice).
template <typename T, int MASK, int V>
__global__ __launch_bounds__(256) void fused_hub_combine_kernel(const int64_t* __restrict__ indptr, T* __restrict__ out,
                                                                int64_t* __restrict__ arg_min, int64_t* __restrict__ arg_max,
                                                                FusedShape s, HubWs hw, FusedPartial<typename Math<T>::acc_t> fp) {
  using acc_t = typename Math<T>::acc_t;
  constexpr bool SUM = (MASK & ACC_SUM) != 0, MIN = (MASK & ACC_MIN) != 0, MAX = (MASK & ACC_MAX) != 0;
  const int64_t kv = s.F / V;
  const int64_t items = hw.counters[3] ? 0 : (int64_t)hw.counters[0] * kv;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < items; t += (int64_t)gridDim.x * blockDim.x) {
    const HubRec hub = hw.hubs[t / kv];
    if (hub.nch == 1) continue;
    const int64_t c = (t % kv) * V;
    const int64_t n = hub.n;
    acc_t sum[V], mn[V], mx[V];
    int64_t bmn[V], bmx[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      sum[i] = acc_t(0);
      mn[i] = min_start<T>(), mx[i] = max_start<T>();
      bmn[i] = bmx[i] = s.E;
    }
    for (int j = 0; j < hub.nch; ++j) {
      const int64_t sj = (int64_t)(hub.slot_base + j) * s.F + c;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        if constexpr (SUM) sum[i] += fp.sum[sj + i];
        if constexpr (MIN) take_better<true>(mn[i], bmn[i], fp.mn[sj + i], fp.bmin[sj + i]);
        if constexpr (MAX) take_better<false>(mx[i], bmx[i], fp.mx[sj + i], fp.bmax[sj + i]);
      }
    }
    fused_store<T, MASK, V>(out + n * s.ostride + c, s, indptr[n + 1] - indptr[n], sum, mn, mx);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      if (MIN && arg_min) arg_min[n * s.F + c + i] = bmn[i];
      if (MAX && arg_max) arg_max[n * s.F + c + i] = bmx[i];
    }
  }
}

// ---- backward: one pass over the edges, every grad_in element written once ----------------------------
struct BackwardShape {
  int64_t E, F, gstride;   // gstride = R * F, elements per grad_out row
  int n_ops;
  int op[4];
  int64_t col[4];          // first column of list entry k's slice
};

template <typename T, int V>
__global__ __launch_bounds__(256) void fused_backward_kernel(const T* __restrict__ grad_out, const int64_t* __restrict__ index,
                                                             const int64_t* __restrict__ arg_min,
                                                             const int64_t* __restrict__ arg_max,
                                                             const int64_t* __restrict__ count, T* __restrict__ grad_in,
                                                             BackwardShape s) {
  using acc_t = typename Math<T>::acc_t;
  using P = Pack<T, V>;
  const int64_t kv = s.F / V;
  const int64_t total = s.E * kv;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = t / kv;
    const int64_t c = (t - e * kv) * V;
    const int64_t n = index[e];
    const T* gp = grad_out + n * s.gstride + c;
    acc_t acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = acc_t(0);
    for (int k = 0; k < s.n_ops; ++k) {   // (list order; wave-uniform branches)
      const P g = *reinterpret_cast<const P*>(gp + s.col[k]);
      if (s.op[k] == F_SUM) {
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] += Math<T>::up(g.v[i]);
      } else if (s.op[k] == F_MEAN) {
        const int64_t cnt = count[n];
        const acc_t denom = (acc_t)(cnt > 0 ? cnt : 1);
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] += Math<T>::up(g.v[i]) / denom;
      } else {
        const int64_t* ap = (s.op[k] == F_MIN ? arg_min : arg_max) + n * s.F + c;
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] += ap[i] == e ? Math<T>::up(g.v[i]) : acc_t(0);
      }
    }
    P r;
#pragma unroll
    for (int i = 0; i < V; ++i) r.v[i] = Math<T>::down(acc[i]);
    *reinterpret_cast<P*>(grad_in + e * s.F + c) = r;
  }
}

// ---- host dispatch ----------------------------------------------------------------------------------------
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T>
constexpr bool is_floating_v = std::is_same<T, float>::value || std::is_same<T, double>::value ||
                               std::is_same<T, bf16_t>::value || std::is_same<T, f16_t>::value;

inline bool floating_dtype(int dtype) { return dtype == PYG_F32 || dtype == PYG_F64 || dtype == PYG_F16 || dtype == PYG_BF16; }

// per element of a hub slot: two int64 positions and three accumulators
inline size_t partial_bytes(int dtype) { return 2 * sizeof(int64_t) + 3 * (dtype == PYG_F64 ? sizeof(double) : sizeof(float)); }

// workspace: sorted keys | permutation | index_sort's own | row offsets | hub scratch
struct FusedWs {
  size_t o_perm, o_sort, sort_bytes, o_indptr, o_hub, hub_bytes, total;
};
inline FusedWs plan_ws(int dtype, int64_t E, int64_t N, int64_t F) {
  FusedWs w;
  const size_t ebytes = align_up(sizeof(int64_t) * (size_t)(E > 0 ? E : 1), 256);
  w.o_perm = ebytes;
  w.o_sort = 2 * ebytes;
  w.sort_bytes = align_up(index_sort_ws_bytes_i64(E), 256);
  w.o_indptr = w.o_sort + w.sort_bytes;
  w.o_hub = w.o_indptr + align_up(sizeof(int64_t) * (size_t)(N + 1), 256);
  // (no bucket can be a hub unless E exceeds the cut and there is more than one bucket)
  w.hub_bytes = E > kHubCut && N > 1 ? hub_plan(nullptr, 0, E, F, partial_bytes(dtype), false, nullptr, nullptr) + 256 : 0;
  w.total = w.o_hub + w.hub_bytes;
  return w;
}

struct FusedArgs {
  const void* src;
  const int64_t* keys;   // the sorted index
  int64_t* indptr;
  const int64_t* perm;
  void* out;
  int64_t *arg_min, *arg_max, *count;
  void* hub_ws;
  size_t hub_bytes;
  int dtype;
};

template <typename T, int MASK, bool ARG, int V>
int launch_rows(const FusedArgs& a, FusedShape s, hipStream_t stream) {
  using acc_t = typename Math<T>::acc_t;
  const int64_t kv = s.F / V;
  const int64_t items = s.N * kv;
  // (pick_lanes' rules for few long rows only: its narrow-row rules split buckets of 16 positions, and a bucket that one lane
  // walks is summed in exactly the sequential order)
  const int L = pick_lanes(items, s.E, s.N, device_info().num_cus);
  const int64_t cut = kHubCut * (int64_t)L;
  const bool hubs = s.E > cut && s.N > 1;
  HubWs hw;
  FusedPartial<acc_t> fp;
  int64_t max_chunks = 0;
  if (hubs) {
    s.long_cut = cut;
    if (!hub_plan(a.hub_ws, a.hub_bytes, s.E, s.F, partial_bytes(a.dtype), false, &hw, &max_chunks))
      return fail(PYG_HIP_ERR_INVALID, "fused_scatter_reduce: the workspace does not hold the hub scratch");
    const size_t plane = (size_t)hw.max_slots * (size_t)s.F;
    fp.bmin = reinterpret_cast<int64_t*>(hw.partial);
    fp.bmax = fp.bmin + plane;
    fp.sum = reinterpret_cast<acc_t*>(fp.bmax + plane);
    fp.mn = fp.sum + plane;
    fp.mx = fp.mn + plane;
  }
  hipLaunchKernelGGL(fused_indptr_kernel, dim3((unsigned)((s.N + 1 + 255) / 256)), dim3(256), 0, stream, a.keys, s.E, s.N, a.indptr,
                     hw.counters);
  PYG_HIP_CHECK(hipGetLastError());
  const T* sp = static_cast<const T*>(a.src);
  T* op = static_cast<T*>(a.out);
#define PYG_FUSED_LAUNCH(LL)                                                                                               \
  hipLaunchKernelGGL((fused_rows_kernel<T, MASK, ARG, V, LL>), dim3((unsigned)((items * LL + 255) / 256)), dim3(256), 0, stream, \
                     sp, a.indptr, a.perm, op, a.arg_min, a.arg_max, a.count, s, hw)
  if (L == 64) PYG_FUSED_LAUNCH(64);
  else if (L == 8) PYG_FUSED_LAUNCH(8);
  else PYG_FUSED_LAUNCH(1);
#undef PYG_FUSED_LAUNCH
  PYG_HIP_CHECK(hipGetLastError());
  if (!hubs) return PYG_HIP_OK;
  const int64_t grid = std::min<int64_t>(max_chunks, (int64_t)device_info().num_cus * 8);
  hipLaunchKernelGGL((fused_hub_chunk_kernel<T, MASK, V>), dim3((unsigned)grid), dim3(256), 0, stream, sp, a.indptr, a.perm, op,
                     a.arg_min, a.arg_max, s, hw, fp);
  PYG_HIP_CHECK(hipGetLastError());
  if (s.E > hw.CH) {   // (else every hub is one chunk long)
    const int64_t max_hubs = s.E / cut;
    const int64_t cgrid = std::min<int64_t>((max_hubs * kv + 255) / 256, (int64_t)device_info().num_cus * 4);
    hipLaunchKernelGGL((fused_hub_combine_kernel<T, MASK, V>), dim3((unsigned)cgrid), dim3(256), 0, stream, a.indptr, op,
                       a.arg_min, a.arg_max, s, hw, fp);
    PYG_HIP_CHECK(hipGetLastError());
  }
  return PYG_HIP_OK;
}

template <typename T, int MASK, int V>
int launch_arg(const FusedArgs& a, const FusedShape& s, hipStream_t stream) {
  if constexpr ((MASK & (ACC_MIN | ACC_MAX)) != 0) {
    if (a.arg_min || a.arg_max) return launch_rows<T, MASK, true, V>(a, s, stream);
  }
  return launch_rows<T, MASK, false, V>(a, s, stream);
}

template <typename T, int V>
int launch_mask(int mask, const FusedArgs& a, const FusedShape& s, hipStream_t stream) {
  switch (mask) {
    case 1: return launch_arg<T, 1, V>(a, s, stream);
    case 2: return launch_arg<T, 2, V>(a, s, stream);
    case 3: return launch_arg<T, 3, V>(a, s, stream);
    case 4: return launch_arg<T, 4, V>(a, s, stream);
    case 5: return launch_arg<T, 5, V>(a, s, stream);
    case 6: return launch_arg<T, 6, V>(a, s, stream);
    default: return launch_arg<T, 7, V>(a, s, stream);
  }
}

template <typename T>
int run_fused(int mask, const FusedArgs& a, const FusedShape& s, hipStream_t stream) {
  if constexpr (is_floating_v<T>) {
    constexpr int VN = 16 / (int)sizeof(T);
    const bool vec = (s.F * (int64_t)sizeof(T)) % 16 == 0 && aligned16(a.src) && aligned16(a.out);
    return vec ? launch_mask<T, VN>(mask, a, s, stream) : launch_mask<T, 1>(mask, a, s, stream);
  } else {
    return fail(PYG_HIP_ERR_UNSUPPORTED, "fused_scatter_reduce: floating-point dtypes only");
  }
}

template <typename T>
int run_backward(const void* grad_out, const int64_t* index, const int64_t* arg_min, const int64_t* arg_max,
                 const int64_t* count, void* grad_in, const BackwardShape& s, hipStream_t stream) {
  if constexpr (is_floating_v<T>) {
    constexpr int VN = 16 / (int)sizeof(T);
    const bool vec = (s.F * (int64_t)sizeof(T)) % 16 == 0 && aligned16(grad_out) && aligned16(grad_in);
    const int64_t total = s.E * (s.F / (vec ? VN : 1));
    int64_t blocks = (total + 255) / 256;
    blocks = std::min<int64_t>(blocks, (int64_t)device_info().num_cus * 16);
    if (vec)
      hipLaunchKernelGGL((fused_backward_kernel<T, VN>), dim3((unsigned)blocks), dim3(256), 0, stream,
                         static_cast<const T*>(grad_out), index, arg_min, arg_max, count, static_cast<T*>(grad_in), s);
    else
      hipLaunchKernelGGL((fused_backward_kernel<T, 1>), dim3((unsigned)blocks), dim3(256), 0, stream,
                         static_cast<const T*>(grad_out), index, arg_min, arg_max, count, static_cast<T*>(grad_in), s);
    PYG_HIP_CHECK(hipGetLastError());
    return PYG_HIP_OK;
  } else {
    return fail(PYG_HIP_ERR_UNSUPPORTED, "fused_scatter_reduce_backward: floating-point dtypes only");
  }
}

// ops[] -> first column of each reduction's slice (-1: not in the list); refuses an empty list, unknown codes, duplicates
int parse_ops(const char* name, const int* ops, int n_ops, int64_t F, int64_t (&col)[4]) {
  PYG_HIP_REQUIRE(ops && n_ops >= 1 && n_ops <= 4, "%s: n_ops must be 1 ... 4 (got %d)", name, n_ops);
  for (int k = 0; k < 4; ++k) col[k] = -1;
  for (int k = 0; k < n_ops; ++k) {
    PYG_HIP_REQUIRE(ops[k] >= F_SUM && ops[k] <= F_MAX, "%s: unknown reduction %d (PYG_FUSED_SUM ... PYG_FUSED_MAX)", name, ops[k]);
    PYG_HIP_REQUIRE(col[ops[k]] < 0, "%s: reduction %d is listed twice", name, ops[k]);
    col[ops[k]] = (int64_t)k * F;
  }
  return PYG_HIP_OK;
}

}  // namespace
}  // namespace pyg_hip

using namespace pyg_hip;

extern "C" {

size_t pyg_hip_fused_scatter_reduce_workspace_size(int dtype, int64_t E, int64_t N, int64_t F) {
  return plan_ws(dtype, E < 0 ? 0 : E, N < 0 ? 0 : N, F < 0 ? 0 : F).total;
}

int pyg_hip_fused_scatter_reduce(int dtype, const void* src, const int64_t* index, int64_t E, int64_t F, int64_t N,
                                 const int* ops, int n_ops, void* out, int64_t* arg_min, int64_t* arg_max, int64_t* count_out,
                                 void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PYG_HIP_REQUIRE(E >= 0 && F >= 0 && N >= 0, "fused_scatter_reduce: negative size");
  if (!floating_dtype(dtype))
    return fail(PYG_HIP_ERR_UNSUPPORTED, "fused_scatter_reduce: floating-point dtypes only (got dtype %d)", dtype);
  FusedShape s;
  s.E = E, s.N = N, s.F = F, s.ostride = (int64_t)n_ops * F;
  if (int rc = parse_ops("fused_scatter_reduce", ops, n_ops, F, s.col)) return rc;
  if (count_out && N > 0 && (E == 0 || F == 0)) PYG_HIP_CHECK(hipMemsetAsync(count_out, 0, sizeof(int64_t) * (size_t)N, stream));
  if (N == 0 || F == 0) {
    // (F == 0: nothing walks the buckets, the counts come from a sort nobody else needs -- they read 0 like the outputs)
    return PYG_HIP_OK;
  }
  PYG_HIP_REQUIRE(out, "fused_scatter_reduce: NULL output");
  if (E == 0) {   // every bucket is empty: zeros, the sentinel E = 0 in the args; `src` and `index` are not touched
    PYG_HIP_CHECK(hipMemsetAsync(out, 0, dtype_size(dtype) * (size_t)(N * s.ostride), stream));
    if (arg_min && s.col[F_MIN] >= 0) PYG_HIP_CHECK(hipMemsetAsync(arg_min, 0, sizeof(int64_t) * (size_t)(N * F), stream));
    if (arg_max && s.col[F_MAX] >= 0) PYG_HIP_CHECK(hipMemsetAsync(arg_max, 0, sizeof(int64_t) * (size_t)(N * F), stream));
    return PYG_HIP_OK;
  }
  PYG_HIP_REQUIRE(src && index, "fused_scatter_reduce: NULL tensor");
  const FusedWs w = plan_ws(dtype, E, N, F);
  PYG_HIP_REQUIRE(workspace && workspace_bytes >= w.total,
                  "fused_scatter_reduce: workspace of %zu bytes, pyg_hip_fused_scatter_reduce_workspace_size() asks for %zu",
                  workspace ? workspace_bytes : (size_t)0, w.total);
  PYG_HIP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "fused_scatter_reduce: workspace must be 8-byte aligned");
  char* base = static_cast<char*>(workspace);
  int64_t* keys = reinterpret_cast<int64_t*>(base);
  int64_t* perm = reinterpret_cast<int64_t*>(base + w.o_perm);
  int64_t* indptr = reinterpret_cast<int64_t*>(base + w.o_indptr);
  if (int rc = index_sort_i64(index, E, N - 1, keys, perm, base + w.o_sort, w.sort_bytes, stream)) return rc;
  const int mask = ((s.col[F_SUM] >= 0 || s.col[F_MEAN] >= 0) ? ACC_SUM : 0) | (s.col[F_MIN] >= 0 ? ACC_MIN : 0) |
                   (s.col[F_MAX] >= 0 ? ACC_MAX : 0);
  const FusedArgs a{src, keys, indptr, perm, out, s.col[F_MIN] >= 0 ? arg_min : nullptr, s.col[F_MAX] >= 0 ? arg_max : nullptr,
                    count_out, base + w.o_hub, w.hub_bytes, dtype};
  PYG_DISPATCH_ALL(dtype, (run_fused<scalar_t>(mask, a, s, stream)));
}

int pyg_hip_fused_scatter_reduce_backward(int dtype, const void* grad_out, const int64_t* index, const int64_t* arg_min,
                                          const int64_t* arg_max, const int64_t* count, int64_t E, int64_t F, int64_t N,
                                          const int* ops, int n_ops, void* grad_in, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PYG_HIP_REQUIRE(E >= 0 && F >= 0 && N >= 0, "fused_scatter_reduce_backward: negative size");
  if (!floating_dtype(dtype))
    return fail(PYG_HIP_ERR_UNSUPPORTED, "fused_scatter_reduce_backward: floating-point dtypes only (got dtype %d)", dtype);
  BackwardShape s;
  s.E = E, s.F = F, s.gstride = (int64_t)n_ops * F, s.n_ops = n_ops;
  int64_t col[4];
  if (int rc = parse_ops("fused_scatter_reduce_backward", ops, n_ops, F, col)) return rc;
  for (int k = 0; k < 4; ++k) s.op[k] = k < n_ops ? ops[k] : 0, s.col[k] = (int64_t)k * F;
  PYG_HIP_REQUIRE(col[F_MIN] < 0 || arg_min, "fused_scatter_reduce_backward: 'min' needs arg_min");
  PYG_HIP_REQUIRE(col[F_MAX] < 0 || arg_max, "fused_scatter_reduce_backward: 'max' needs arg_max");
  PYG_HIP_REQUIRE(col[F_MEAN] < 0 || count, "fused_scatter_reduce_backward: 'mean' needs count");
  if (E == 0 || F == 0) return PYG_HIP_OK;
  PYG_HIP_REQUIRE(N > 0, "fused_scatter_reduce_backward: %lld edges into no bucket", (long long)E);
  PYG_HIP_REQUIRE(grad_out && index && grad_in, "fused_scatter_reduce_backward: NULL tensor");
  PYG_DISPATCH_ALL(dtype, (run_backward<scalar_t>(grad_out, index, arg_min, arg_max, count, grad_in, s, stream)));
}

}  // extern "C"
