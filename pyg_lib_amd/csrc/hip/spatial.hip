// knn, radius and nearest for gfx950 (MI355X): batched brute-force neighbour search over point clouds.
//
// Replaces pyg_lib/csrc/ops/cuda/{knn,radius,nearest}_kernel.cu (one thread per query, every candidate read from global
// memory, the k best in two 100-entry per-thread arrays in private memory).  Semantics: include/pyg_hip.h.
//
// One kernel template serves the three operators (spatial_kernel):
//   * a workgroup of kQ threads owns a tile of kQ queries of ONE example (a launch-time scan of the query pointer deals the
//     tiles; a block finds its example by bisection), one query per lane;
//   * the example's candidates pass through LDS in tiles; every lane reads the same candidate (a broadcast read);
//       SHAPE_SMALL (D <= 4): candidates padded to 4 coordinates (one 16 / 32 byte LDS read each), the query in 4 registers.
//                             The zero padding adds (0 - 0)^2 = +0 to a non-negative sum: the same bits as the D-term sum;
//       SHAPE_LDSQ / SHAPE_GLOBQ (any D): rows copied as they lie, 4 candidates per trip (4 independent sums), the query's
//                             coordinates from a transposed LDS copy while kQ * D elements fit 32 KiB, else from global memory;
//   * the distance is compared with a threshold register first (the k-th best so far, or r^2): the common candidate costs the
//     distance and one compare; the insertion is the rare path;
//   * the k best live in registers with static indexing for k <= 16 (LIST_1, LIST_16) and in LDS above that (LIST_LDS:
//     distance + 32-bit index per entry, strided by the workgroup so that lanes hit different banks); never in private memory;
//   * no FMA contraction anywhere in this file: a - b, d * d and s + d * d are rounded one by one, which is what makes the
//     result comparable bit for bit with the CPU key.
// 16-bit inputs are widened to fp32 once (exact), so the kernels exist for float and double only.
//
// Routes (pyg_hip_spatial_route): `lane` -- a block scans its example's whole candidate range; `split` -- when the query tiles
// alone cannot fill the chip the candidate range is cut into up to kMaxChunks chunks (grid.y); every (tile, chunk) block
// leaves a sorted partial list (knn, nearest) or a count (radius) in the workspace and a second launch merges them, one wave
// per query, by (distance, chunk) -- chunks are in index order, so this is (distance, index).  No atomics: same bits each call.
// radius: count pass, scan (scan.h), fill pass; the split route scans the per-chunk counts of a query inside the fill pass.
#include "common.h"
#include "elem.h"
#include "scan.h"

#include <algorithm>
#include <mutex>

#pragma clang fp contract(off)

namespace pyg_hip {
namespace {

constexpr int kQ = 128;           // threads (and, but for fp64 LDS lists, queries) per workgroup
constexpr int kTileSmall = 512;   // candidates per LDS tile, D <= 4
constexpr int kTileElems = 2048;  // elements per LDS tile, general D (at least one row)
constexpr int kMaxK = 100;        // the reference's limit
constexpr int kRegK = 16;         // k up to here: registers
constexpr int kMaxChunks = 64;    // split route: one lane of the merging wave per chunk
constexpr int kChunkMin = 256;    // split route: shortest chunk the rule chooses
constexpr int kChunkForced = 32;  // ... and under PYG_HIP_SPATIAL_FORCE_SPLIT (small test inputs span several chunks)
constexpr int kSplitTiles = 256;  // split when there are fewer query tiles than this (one per CU)
constexpr int64_t kMaxD = 4096;
constexpr int kMaxLds = 160 * 1024;

enum { SHAPE_SMALL = 0, SHAPE_LDSQ = 1, SHAPE_GLOBQ = 2 };
enum { LIST_LDS = 0, LIST_1 = 1, LIST_16 = kRegK };
enum { OP_KNN = PYG_SPATIAL_KNN, OP_RADIUS = PYG_SPATIAL_RADIUS, OP_NEAREST = PYG_SPATIAL_NEAREST };

template <typename A>
__device__ __forceinline__ A inf_v() {
  return (A)__builtin_huge_valf();
}

// segment b of a CSR pointer over n rows, clamped into [0, n] (ptr == nullptr: the single example [0, n])
__host__ __device__ __forceinline__ void seg_bounds(const int64_t* ptr, int64_t b, int64_t n, int64_t& lo, int64_t& hi) {
  if (!ptr) {
    lo = 0, hi = n;
    return;
  }
  const int64_t a = ptr[b], e = ptr[b + 1];
  lo = a < 0 ? 0 : (a > n ? n : a);
  hi = e < lo ? lo : (e > n ? n : e);
}

// ---- launch-time scan: first query tile of every example, pointer validation ---------------------------------------
struct TileLoad {
  const int64_t* ptr_q;
  int64_t M;
  int qpw;
  __device__ int64_t operator()(int64_t b) const {
    int64_t lo, hi;
    seg_bounds(ptr_q, b, M, lo, hi);
    return (hi - lo + qpw - 1) / qpw;
  }
};
struct TileStore {
  const int64_t *ptr_q, *ptr_c;
  int64_t M, N, B;
  int64_t* tile_start;
  int* bad;   // set to 1 on a non-monotone pointer or a last entry that is not the row count
  __device__ void operator()(int64_t b, int64_t run, int64_t v) const {
    tile_start[b] = run;
    if (b == B - 1) tile_start[B] = run + v;
    bool wrong = false;
    if (ptr_q) wrong |= ptr_q[b] > ptr_q[b + 1] || (b == B - 1 && ptr_q[B] != M);
    if (ptr_c) wrong |= ptr_c[b] > ptr_c[b + 1] || (b == B - 1 && ptr_c[B] != N);
    if (wrong) *bad = 1;
  }
};

template <typename T>
__global__ __launch_bounds__(256) void widen_kernel(const T* __restrict__ src, float* __restrict__ dst, int64_t n) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = Math<T>::up(src[i]);
}

template <typename A>
__global__ __launch_bounds__(256) void norm_kernel(const A* __restrict__ src, A* __restrict__ dst, int64_t rows, int D) {
  const int64_t i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= rows) return;
  A s = 0;
  for (int d = 0; d < D; ++d) {
    const A v = src[i * D + d];
    s = s + v * v;
  }
  dst[i] = sqrt(s);
}

// ---- the k best of one lane --------------------------------------------------------------------------------------
// registers, static indexing only: accepted candidates enter at the end and bubble up past strictly larger distances
template <typename A, int LIST>
struct KnnList {
  A d[LIST];
  int32_t ix[LIST];
  A thr;
  int k;
  __device__ void init(int k_, A*, int32_t*, int, int) {
    k = k_;
#pragma unroll
    for (int e = 0; e < LIST; ++e) d[e] = inf_v<A>(), ix[e] = -1;
    thr = inf_v<A>();
  }
  __device__ __forceinline__ void push(A dist, int32_t j) {
    if (dist < thr) {
      d[LIST - 1] = dist, ix[LIST - 1] = j;
#pragma unroll
      for (int e = LIST - 1; e > 0; --e) {
        const bool sw = d[e] < d[e - 1];
        const A td = d[e];
        const int32_t ti = ix[e];
        d[e] = sw ? d[e - 1] : td, ix[e] = sw ? ix[e - 1] : ti;
        d[e - 1] = sw ? td : d[e - 1], ix[e - 1] = sw ? ti : ix[e - 1];
      }
#pragma unroll
      for (int e = 0; e < LIST; ++e)
        if (e == k - 1) thr = d[e];
    }
  }
  template <typename F>
  __device__ __forceinline__ void each(F f) const {
#pragma unroll
    for (int e = 0; e < LIST; ++e)
      if (e < k) f(e, d[e], ix[e]);
  }
};
// LDS: entry e of lane t at [e * stride + t]
template <typename A>
struct KnnList<A, LIST_LDS> {
  A* d;
  int32_t* ix;
  A thr;
  int k, stride;
  __device__ void init(int k_, A* dbase, int32_t* ibase, int slot, int stride_) {
    k = k_, stride = stride_, d = dbase + slot, ix = ibase + slot;
    for (int e = 0; e < k; ++e) d[e * stride] = inf_v<A>(), ix[e * stride] = -1;
    thr = inf_v<A>();
  }
  __device__ __forceinline__ void push(A dist, int32_t j) {
    if (dist < thr) {
      int e = k - 1;
      while (e > 0 && d[(e - 1) * stride] > dist) {
        d[e * stride] = d[(e - 1) * stride], ix[e * stride] = ix[(e - 1) * stride];
        --e;
      }
      d[e * stride] = dist, ix[e * stride] = j;
      thr = d[(k - 1) * stride];
    }
  }
  template <typename F>
  __device__ __forceinline__ void each(F f) const {
    for (int e = 0; e < k; ++e) f(e, d[e * stride], ix[e * stride]);
  }
};

// radius: matches in candidate order; counts them all, writes the first `budget`
template <typename A>
struct RadiusSink {
  A r2;
  int32_t skip;     // the query's own index under ignore_same_index, else -1
  int64_t count;
  int64_t budget;   // fill pass: pairs this lane may still write (0 in the count pass)
  int64_t pos, E, self;
  int64_t* out;
  __device__ __forceinline__ void push(A dist, int32_t j) {
    if (dist < r2 && j != skip) {
      if (count < budget && pos + count < E) out[pos + count] = self, out[E + pos + count] = j;
      ++count;
    }
  }
};

template <typename A>
struct Params {
  const A *cand, *query;          // [N, D], [M, D]
  const A *norm_c, *norm_q;       // cosine
  const int64_t *ptr_c, *ptr_q;   // may be null
  const int64_t* tile_start;      // [B + 1]
  int64_t N, M, B;
  int D, k, qpw, nch, rows_tile;
  int64_t chunk;
  int fill, ignore_same;          // radius
  A r2;
  int32_t* nbr;                   // knn, lane route: [M, k]
  int32_t* cnt;                   // knn, lane route: [M]; radius: [M, nch]
  A* part_d;                      // knn / nearest, split route: [M, nch, k]
  int32_t* part_i;
  const int64_t* offs;            // radius fill: [M]
  int64_t* out;                   // radius fill: [2, E]; nearest: [M]
  int64_t E;
};

template <typename A>
struct Vec4 {
  A x, y, z, w;
};

template <typename A, int SHAPE, int LIST, int OP, bool COS>
__global__ __launch_bounds__(kQ) void spatial_kernel(const Params<A> p) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.x;
  if (t >= p.tile_start[p.B]) return;
  int64_t b = 0;
  {
    int64_t hi = p.B;   // the last example whose first tile is not behind t (empty examples share their successor's)
    while (hi - b > 1) {
      const int64_t mid = (b + hi) >> 1;
      if (p.tile_start[mid] <= t) b = mid; else hi = mid;
    }
  }
  int64_t qlo, qhi, clo, chi;
  seg_bounds(p.ptr_q, b, p.M, qlo, qhi);
  seg_bounds(p.ptr_c, b, p.N, clo, chi);
  const int64_t i = qlo + (t - p.tile_start[b]) * p.qpw + tid;
  const bool active = tid < p.qpw && i < qhi;
  const int c = blockIdx.y;
  int64_t cs = clo, ce = chi;
  if (p.nch > 1) {
    cs = clo + c * p.chunk;
    if (cs > chi) cs = chi;
    ce = cs + p.chunk < chi ? cs + p.chunk : chi;
  }
  const int D = p.D;

  // LDS: candidate tile | transposed queries | list distances | list indices
  A* tile = reinterpret_cast<A*>(smem);
  const int tile_elems = SHAPE == SHAPE_SMALL ? kTileSmall * 4 : p.rows_tile * D;
  A* qs = tile + tile_elems;
  A* ld = qs + (SHAPE == SHAPE_LDSQ ? p.qpw * D : 0);
  int32_t* li = reinterpret_cast<int32_t*>(ld + (LIST == LIST_LDS && OP != OP_RADIUS ? p.k * p.qpw : 0));

  // the sink
  KnnList<A, OP == OP_RADIUS ? 1 : LIST> best;
  RadiusSink<A> rad;
  if (OP == OP_RADIUS) {
    rad.r2 = p.r2, rad.skip = p.ignore_same && active ? (int32_t)i : -1, rad.count = 0, rad.budget = 0;
    rad.pos = 0, rad.E = p.E, rad.self = i, rad.out = p.out;
    if (p.fill && active) {
      int64_t before = 0;
      for (int cc = 0; cc < c; ++cc) before += p.cnt[i * p.nch + cc];
      rad.budget = p.k - before;
      rad.pos = p.offs[i] + before;
    }
  } else if (active) {
    best.init(p.k, ld, li, tid, p.qpw);
  }
  auto push = [&](A dist, int32_t j) {
    if (OP == OP_RADIUS) rad.push(dist, j); else best.push(dist, j);
  };

  A q0 = 0, q1 = 0, q2 = 0, q3 = 0, qn = 1;
  if (SHAPE == SHAPE_SMALL) {
    if (active) {
      const A* qp = p.query + i * D;
      q0 = qp[0];
      if (D > 1) q1 = qp[1];
      if (D > 2) q2 = qp[2];
      if (D > 3) q3 = qp[3];
    }
  } else if (SHAPE == SHAPE_LDSQ) {
    const int64_t nq = qhi - (i - tid) < p.qpw ? qhi - (i - tid) : p.qpw;
    const A* qp = p.query + (i - tid) * D;
    for (int64_t e = tid; e < nq * D; e += kQ) {
      const int row = (int)(e / D), d = (int)(e - (int64_t)row * D);
      qs[d * p.qpw + row] = qp[e];
    }
  }
  if (COS && active) qn = p.norm_q[i];
  const A* qg = p.query + (active ? i : 0) * D;

  const int rows_tile = SHAPE == SHAPE_SMALL ? kTileSmall : p.rows_tile;
  for (int64_t j0 = cs; j0 < ce; j0 += rows_tile) {
    const int rows = (int)(ce - j0 < rows_tile ? ce - j0 : rows_tile);
    __syncthreads();   // the previous tile has been consumed (and, first trip, the queries are staged)
    if (SHAPE == SHAPE_SMALL) {
      Vec4<A>* tl = reinterpret_cast<Vec4<A>*>(tile);
      for (int r = tid; r < rows; r += kQ) {
        const A* cp = p.cand + (j0 + r) * D;
        Vec4<A> v;
        v.x = cp[0];
        v.y = D > 1 ? cp[1] : A(0);
        v.z = D > 2 ? cp[2] : A(0);
        v.w = D > 3 ? cp[3] : A(0);
        tl[r] = v;
      }
    } else {
      const A* cp = p.cand + j0 * D;
      for (int e = tid; e < rows * D; e += kQ) tile[e] = cp[e];
    }
    __syncthreads();
    if (!active) continue;
    if (SHAPE == SHAPE_SMALL) {
      const Vec4<A>* tl = reinterpret_cast<const Vec4<A>*>(tile);
#pragma unroll 4
      for (int r = 0; r < rows; ++r) {
        const Vec4<A> v = tl[r];
        const A d0 = q0 - v.x, d1 = q1 - v.y, d2 = q2 - v.z, d3 = q3 - v.w;
        A dist = d0 * d0;
        dist = dist + d1 * d1;
        dist = dist + d2 * d2;
        dist = dist + d3 * d3;
        push(dist, (int32_t)(j0 + r));
      }
    } else {
      for (int r = 0; r < rows; r += 4) {
        // rows past the tile repeat its last row; they are not pushed
        const int r1 = r + 1 < rows ? r + 1 : rows - 1, r2 = r + 2 < rows ? r + 2 : rows - 1, r3 = r + 3 < rows ? r + 3 : rows - 1;
        const A *t0 = tile + r * D, *t1 = tile + r1 * D, *t2 = tile + r2 * D, *t3 = tile + r3 * D;
        A s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        for (int d = 0; d < D; ++d) {
          const A qv = SHAPE == SHAPE_LDSQ ? qs[d * p.qpw + tid] : qg[d];
          if (COS) {
            s0 = s0 + qv * t0[d], s1 = s1 + qv * t1[d], s2 = s2 + qv * t2[d], s3 = s3 + qv * t3[d];
          } else {
            const A e0 = qv - t0[d], e1 = qv - t1[d], e2 = qv - t2[d], e3 = qv - t3[d];
            s0 = s0 + e0 * e0, s1 = s1 + e1 * e1, s2 = s2 + e2 * e2, s3 = s3 + e3 * e3;
          }
        }
        if (COS) {
          const A* nc = p.norm_c + j0;
          s0 = A(1) - s0 / (qn * nc[r]), s1 = A(1) - s1 / (qn * nc[r1]);
          s2 = A(1) - s2 / (qn * nc[r2]), s3 = A(1) - s3 / (qn * nc[r3]);
        }
        push(s0, (int32_t)(j0 + r));
        if (r + 1 < rows) push(s1, (int32_t)(j0 + r + 1));
        if (r + 2 < rows) push(s2, (int32_t)(j0 + r + 2));
        if (r + 3 < rows) push(s3, (int32_t)(j0 + r + 3));
      }
    }
  }
  if (!active) return;

  if (OP == OP_RADIUS) {
    if (!p.fill) p.cnt[i * p.nch + c] = (int32_t)(rad.count < p.k ? rad.count : p.k);
  } else if (p.nch > 1) {
    const int64_t base = (i * p.nch + c) * p.k;
    best.each([&](int e, A dist, int32_t j) { p.part_d[base + e] = dist, p.part_i[base + e] = j; });
    if (OP == OP_NEAREST && c == 0) p.out[i] = clo;
  } else if (OP == OP_NEAREST) {
    best.each([&](int, A, int32_t j) { p.out[i] = j >= 0 ? (int64_t)j : clo; });
  } else {
    int n = 0;
    best.each([&](int e, A, int32_t j) {
      p.nbr[i * p.k + e] = j;
      n += j >= 0;
    });
    p.cnt[i] = n;
  }
}

// split route, second launch: one wave per query, lane c holds the head of chunk c's sorted list
template <typename A>
__global__ __launch_bounds__(256) void merge_kernel(const A* __restrict__ part_d, const int32_t* __restrict__ part_i, int64_t M,
                                                    int nch, int k, int32_t* __restrict__ nbr, int32_t* __restrict__ cnt,
                                                    int64_t* __restrict__ nearest_out) {
  const int lane = threadIdx.x & 63;
  const int64_t q = blockIdx.x * 4ll + (threadIdx.x >> 6);
  if (q >= M) return;
  const int64_t base = (q * nch + lane) * k;
  int pos = 0;
  A hd = inf_v<A>();
  int32_t hi = -1;
  if (lane < nch) hd = part_d[base], hi = part_i[base];
  int e = 0;
  for (; e < k; ++e) {
    A m = hd;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const A other = __shfl_xor(m, o);
      m = other < m ? other : m;
    }
    if (!(m < inf_v<A>())) break;
    const unsigned long long mask = __ballot(hd == m);
    const int src = __ffsll((long long)mask) - 1;   // the lowest chunk: the lowest index among equal distances
    const int32_t idx = __shfl(hi, src);
    if (lane == 0) {
      if (nearest_out) nearest_out[q] = idx; else nbr[q * k + e] = idx;
    }
    if (lane == src) {
      ++pos;
      if (pos < k) hd = part_d[base + pos], hi = part_i[base + pos]; else hd = inf_v<A>();
    }
  }
  if (lane == 0 && !nearest_out) cnt[q] = e;
}

// knn: pair counts -> offsets; radius: per-query counts (summed over chunks, capped) -> offsets
struct CountLoad {
  const int32_t* cnt;
  int nch;
  int64_t cap;
  __device__ int64_t operator()(int64_t i) const {
    int64_t s = 0;
    for (int c = 0; c < nch; ++c) s += cnt[i * nch + c];
    return s < cap ? s : cap;
  }
};
struct OffsStore {
  int64_t* offs;
  __device__ void operator()(int64_t i, int64_t run, int64_t) const { offs[i] = run; }
};

__global__ __launch_bounds__(256) void knn_emit_kernel(const int32_t* __restrict__ nbr, const int32_t* __restrict__ cnt,
                                                       const int64_t* __restrict__ offs, int64_t M, int k, int64_t E,
                                                       int64_t* __restrict__ out) {
  const int64_t t = blockIdx.x * 256ll + threadIdx.x;
  if (t >= M * k) return;
  const int64_t i = t / k;
  const int e = (int)(t - i * k);
  if (e >= cnt[i]) return;
  const int64_t o = offs[i] + e;
  if (o < E) out[o] = i, out[E + o] = nbr[t];
}

// ---- host ----------------------------------------------------------------------------------------------------------
thread_local char g_last_route[64] = "none";

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the pure part of the dispatch: what pyg_hip_spatial_route answers and the entry points follow
struct Plan {
  int route = PYG_HIP_SPATIAL_ROUTE_UNSUPPORTED;
  int shape = 0, list = 0, qpw = kQ, nch = 1, rows_tile = 1;
  int64_t chunk = 0;
  bool f64 = false, wide = false, cos = false;
  size_t lds = 0;
  // workspace
  size_t o_info = 0, o_tile = 0, o_scan = 0, o_wc = 0, o_wq = 0, o_nc = 0, o_nq = 0, o_nbr = 0, o_cnt = 0, o_offs = 0, o_pd = 0,
         o_pi = 0, total = 0;
};

Plan make_plan(int op, int dtype, int64_t M, int64_t N, int64_t B, int64_t D, int64_t k, int flags) {
  Plan p;
  if (op < OP_KNN || op > OP_NEAREST) return p;
  if (dtype != PYG_F32 && dtype != PYG_F64 && dtype != PYG_F16 && dtype != PYG_BF16) return p;
  if (M < 0 || N < 0 || B < 1 || D < 1 || D > kMaxD || M >= (1ll << 31) || N >= (1ll << 31) || B >= (1ll << 31)) return p;
  if (op == OP_KNN && (k < 1 || k > kMaxK)) return p;
  if (op == OP_RADIUS && k < 0) return p;
  if (op == OP_NEAREST) k = 1;
  p.f64 = dtype == PYG_F64;
  p.wide = dtype == PYG_F16 || dtype == PYG_BF16;
  p.cos = op == OP_KNN && (flags & PYG_HIP_SPATIAL_COSINE);
  const size_t asz = p.f64 ? 8 : 4;
  p.list = op == OP_RADIUS ? LIST_1 : (k == 1 ? LIST_1 : (k <= kRegK ? LIST_16 : LIST_LDS));
  p.qpw = p.f64 && p.list == LIST_LDS ? kQ / 2 : kQ;
  p.shape = D <= 4 && !p.cos ? SHAPE_SMALL : ((size_t)p.qpw * D * asz <= 32768 ? SHAPE_LDSQ : SHAPE_GLOBQ);
  p.rows_tile = p.shape == SHAPE_SMALL ? kTileSmall : (int)std::max<int64_t>(1, kTileElems / D);
  p.lds = (p.shape == SHAPE_SMALL ? (size_t)kTileSmall * 4 : (size_t)p.rows_tile * D) * asz +
          (p.shape == SHAPE_LDSQ ? (size_t)p.qpw * D * asz : 0) +
          (p.list == LIST_LDS ? (size_t)k * p.qpw * (asz + 4) : 0);
  // lane or split
  const int64_t tiles = ceil_div(M, p.qpw), mean = ceil_div(N, B);
  bool split = tiles < kSplitTiles && mean >= 2 * kChunkMin;
  if (flags & PYG_HIP_SPATIAL_FORCE_LANE) split = false;
  if (flags & PYG_HIP_SPATIAL_FORCE_SPLIT) split = N > 0;
  if (split) {
    const int64_t want = std::min<int64_t>(kMaxChunks, std::max<int64_t>(2, ceil_div(2 * kSplitTiles, tiles + B)));
    const int64_t shortest = (flags & PYG_HIP_SPATIAL_FORCE_SPLIT) ? kChunkForced : kChunkMin;
    p.chunk = std::max<int64_t>(std::max<int64_t>(shortest, ceil_div(mean, want)), ceil_div(N, kMaxChunks));
    p.nch = (int)std::max<int64_t>(2, ceil_div(N, p.chunk));   // (2: the merge launch is the route)
  }
  p.route = split ? PYG_HIP_SPATIAL_ROUTE_SPLIT : PYG_HIP_SPATIAL_ROUTE_LANE;
  // workspace layout
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += align_up(bytes ? bytes : 1, 256);
    return o;
  };
  const int64_t scan_n = std::max(B, M);
  p.o_info = take(16);
  p.o_tile = take((size_t)(B + 1) * 8);
  p.o_scan = take((size_t)(ceil_div(std::max<int64_t>(scan_n, 1), kScanTile) + 2) * 8);
  if (p.wide) p.o_wc = take((size_t)N * D * 4), p.o_wq = take((size_t)M * D * 4);
  if (p.cos) p.o_nc = take((size_t)N * asz), p.o_nq = take((size_t)M * asz);
  if (op == OP_KNN) p.o_nbr = take((size_t)M * k * 4), p.o_cnt = take((size_t)M * 4), p.o_offs = take((size_t)M * 8);
  if (op == OP_RADIUS) p.o_cnt = take((size_t)M * p.nch * 4), p.o_offs = take((size_t)M * 8);
  if (op != OP_RADIUS && split) p.o_pd = take((size_t)M * p.nch * k * asz), p.o_pi = take((size_t)M * p.nch * k * 4);
  p.total = at;
  return p;
}

const char* op_name(int op) { return op == OP_KNN ? "knn" : op == OP_RADIUS ? "radius" : "nearest"; }

void note_route(int op, const Plan& p) {
  snprintf(g_last_route, sizeof(g_last_route), "%s %s %s %s%s", op_name(op), p.route == PYG_HIP_SPATIAL_ROUTE_SPLIT ? "split" : "lane",
           p.shape == SHAPE_SMALL ? "d4" : p.shape == SHAPE_LDSQ ? "ldsq" : "globq",
           op == OP_RADIUS ? "count" : p.list == LIST_1 ? "reg1" : p.list == LIST_16 ? "reg16" : "lds", p.cos ? " cosine" : "");
}

// the pinned word of this device a nearest call leaves a bad pointer in (as rgcn's deferred check)
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

struct Call {
  int op, dtype, flags;
  const void *cand, *query;
  const int64_t *ptr_c, *ptr_q;
  int64_t N, M, B, D, k;
  double r;
  unsigned char* ws;
  int fill;
  int64_t* out;
  int64_t E;
};

template <typename A, int SHAPE, int LIST, int OP, bool COS>
int launch_one(const Params<A>& prm, const Plan& p, dim3 grid, hipStream_t stream) {
  const void* kern = reinterpret_cast<const void*>(&spatial_kernel<A, SHAPE, LIST, OP, COS>);
  if (int rc_ = ensure_dynamic_lds(kern, kMaxLds)) return rc_;
  hipLaunchKernelGGL((spatial_kernel<A, SHAPE, LIST, OP, COS>), grid, dim3(kQ), p.lds, stream, prm);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

template <typename A, int SHAPE, int OP>
int launch_list(const Params<A>& prm, const Plan& p, dim3 grid, hipStream_t stream) {
  if constexpr (OP == OP_RADIUS) {
    return launch_one<A, SHAPE, LIST_1, OP, false>(prm, p, grid, stream);
  } else if constexpr (OP == OP_NEAREST) {
    return launch_one<A, SHAPE, LIST_1, OP, false>(prm, p, grid, stream);
  } else if constexpr (SHAPE == SHAPE_SMALL) {
    if (p.list == LIST_1) return launch_one<A, SHAPE, LIST_1, OP, false>(prm, p, grid, stream);
    if (p.list == LIST_16) return launch_one<A, SHAPE, LIST_16, OP, false>(prm, p, grid, stream);
    return launch_one<A, SHAPE, LIST_LDS, OP, false>(prm, p, grid, stream);
  } else {
    if (p.cos) {
      if (p.list == LIST_1) return launch_one<A, SHAPE, LIST_1, OP, true>(prm, p, grid, stream);
      if (p.list == LIST_16) return launch_one<A, SHAPE, LIST_16, OP, true>(prm, p, grid, stream);
      return launch_one<A, SHAPE, LIST_LDS, OP, true>(prm, p, grid, stream);
    }
    if (p.list == LIST_1) return launch_one<A, SHAPE, LIST_1, OP, false>(prm, p, grid, stream);
    if (p.list == LIST_16) return launch_one<A, SHAPE, LIST_16, OP, false>(prm, p, grid, stream);
    return launch_one<A, SHAPE, LIST_LDS, OP, false>(prm, p, grid, stream);
  }
}

template <typename A, int OP>
int launch_shape(const Params<A>& prm, const Plan& p, dim3 grid, hipStream_t stream) {
  if (p.shape == SHAPE_SMALL) return launch_list<A, SHAPE_SMALL, OP>(prm, p, grid, stream);
  if (p.shape == SHAPE_LDSQ) return launch_list<A, SHAPE_LDSQ, OP>(prm, p, grid, stream);
  return launch_list<A, SHAPE_GLOBQ, OP>(prm, p, grid, stream);
}

// everything on the stream up to (not including) the host read; `bad` receives the pointer check
template <typename A>
int run(const Call& c, const Plan& p, int* bad, hipStream_t stream) {
  unsigned char* ws = c.ws;
  int64_t* info = reinterpret_cast<int64_t*>(ws + p.o_info);
  int64_t* tile_start = reinterpret_cast<int64_t*>(ws + p.o_tile);
  int64_t* scan_buf = reinterpret_cast<int64_t*>(ws + p.o_scan);
  const int64_t scan_tiles = ceil_div(std::max<int64_t>(std::max(c.B, c.M), 1), kScanTile);
  const A* cand = static_cast<const A*>(c.cand);
  const A* query = static_cast<const A*>(c.query);
  const int64_t k = c.op == OP_NEAREST ? 1 : c.k;

  if (!c.fill) {
    if (p.wide) {
      if constexpr (sizeof(A) == 4) {
        float* wc = reinterpret_cast<float*>(ws + p.o_wc);
        float* wq = reinterpret_cast<float*>(ws + p.o_wq);
        const int64_t nc = c.N * c.D, nq = c.M * c.D;
        const unsigned gc = (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(nc, 256), 1), 4096);
        const unsigned gq = (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(nq, 256), 1), 4096);
        if (c.dtype == PYG_F16) {
          hipLaunchKernelGGL((widen_kernel<f16_t>), dim3(gc), dim3(256), 0, stream, static_cast<const f16_t*>(c.cand), wc, nc);
          hipLaunchKernelGGL((widen_kernel<f16_t>), dim3(gq), dim3(256), 0, stream, static_cast<const f16_t*>(c.query), wq, nq);
        } else {
          hipLaunchKernelGGL((widen_kernel<bf16_t>), dim3(gc), dim3(256), 0, stream, static_cast<const bf16_t*>(c.cand), wc, nc);
          hipLaunchKernelGGL((widen_kernel<bf16_t>), dim3(gq), dim3(256), 0, stream, static_cast<const bf16_t*>(c.query), wq, nq);
        }
      }
    }
    if (c.op != OP_NEAREST) PYG_HIP_CHECK(hipMemsetAsync(info, 0, 16, stream));
    TileLoad load{c.ptr_q, c.M, p.qpw};
    TileStore store{c.ptr_q, c.ptr_c, c.M, c.N, c.B, tile_start, bad};
    if (int rc = device_scan<int64_t, SumOp>(load, store, c.B, scan_buf, scan_buf + scan_tiles + 1, stream)) return rc;
  }
  if (p.wide) {
    cand = reinterpret_cast<const A*>(ws + p.o_wc);
    query = reinterpret_cast<const A*>(ws + p.o_wq);
  }

  Params<A> prm{};
  prm.cand = cand, prm.query = query;
  prm.ptr_c = c.ptr_c, prm.ptr_q = c.ptr_q, prm.tile_start = tile_start;
  prm.N = c.N, prm.M = c.M, prm.B = c.B;
  prm.D = (int)c.D, prm.k = (int)k, prm.qpw = p.qpw, prm.nch = p.nch, prm.rows_tile = p.rows_tile, prm.chunk = p.chunk;
  prm.fill = c.fill, prm.ignore_same = (c.flags & PYG_HIP_SPATIAL_IGNORE_SAME) ? 1 : 0;
  prm.r2 = (A)(c.r * c.r);
  prm.nbr = reinterpret_cast<int32_t*>(ws + p.o_nbr), prm.cnt = reinterpret_cast<int32_t*>(ws + p.o_cnt);
  prm.part_d = reinterpret_cast<A*>(ws + p.o_pd), prm.part_i = reinterpret_cast<int32_t*>(ws + p.o_pi);
  prm.offs = reinterpret_cast<const int64_t*>(ws + p.o_offs);
  prm.out = c.out, prm.E = c.E;
  if (p.cos) {
    A* nc = reinterpret_cast<A*>(ws + p.o_nc);
    A* nq = reinterpret_cast<A*>(ws + p.o_nq);
    if (c.N > 0) hipLaunchKernelGGL((norm_kernel<A>), dim3((unsigned)ceil_div(c.N, 256)), dim3(256), 0, stream, cand, nc, c.N, (int)c.D);
    if (c.M > 0) hipLaunchKernelGGL((norm_kernel<A>), dim3((unsigned)ceil_div(c.M, 256)), dim3(256), 0, stream, query, nq, c.M, (int)c.D);
    prm.norm_c = nc, prm.norm_q = nq;
  }
  if (c.op != OP_NEAREST && !c.fill)
    PYG_HIP_CHECK(hipMemsetAsync(prm.cnt, 0, (size_t)c.M * (c.op == OP_RADIUS ? p.nch : 1) * 4, stream));

  const dim3 grid((unsigned)(ceil_div(c.M, p.qpw) + c.B), (unsigned)p.nch);
  int rc;
  if (c.op == OP_KNN) rc = launch_shape<A, OP_KNN>(prm, p, grid, stream);
  else if (c.op == OP_RADIUS) rc = launch_shape<A, OP_RADIUS>(prm, p, grid, stream);
  else rc = launch_shape<A, OP_NEAREST>(prm, p, grid, stream);
  if (rc != PYG_HIP_OK) return rc;
  if (c.fill) return PYG_HIP_OK;

  if (c.op != OP_RADIUS && p.nch > 1) {
    hipLaunchKernelGGL((merge_kernel<A>), dim3((unsigned)ceil_div(c.M, 4)), dim3(256), 0, stream, prm.part_d, prm.part_i, c.M, p.nch,
                       (int)k, prm.nbr, prm.cnt, c.op == OP_NEAREST ? c.out : nullptr);
    PYG_HIP_CHECK(hipGetLastError());
  }
  if (c.op != OP_NEAREST) {
    CountLoad load{prm.cnt, c.op == OP_RADIUS ? p.nch : 1, c.op == OP_RADIUS ? c.k : k};
    OffsStore store{reinterpret_cast<int64_t*>(ws + p.o_offs)};
    if (int rc2 = device_scan<int64_t, SumOp>(load, store, c.M, scan_buf, info, stream)) return rc2;
  }
  return PYG_HIP_OK;
}

int check_call(const char* name, const Call& c, size_t ws_bytes, Plan* plan) {
  PYG_HIP_REQUIRE(c.dtype == PYG_F32 || c.dtype == PYG_F64 || c.dtype == PYG_F16 || c.dtype == PYG_BF16,
                  "%s: x and y must be float32, float64, float16 or bfloat16 (dtype code %d)", name, c.dtype);
  PYG_HIP_REQUIRE(c.M >= 0 && c.N >= 0, "%s: negative size", name);
  PYG_HIP_REQUIRE(c.D >= 1, "%s: the feature dimension must be at least 1 (got %lld)", name, (long long)c.D);
  PYG_HIP_REQUIRE(c.B >= 1, "%s: a pointer has at least 2 entries (num_examples %lld)", name, (long long)c.B);
  PYG_HIP_REQUIRE((c.ptr_c && c.ptr_q) || c.B == 1, "%s: a NULL pointer stands for one example, num_examples is %lld", name, (long long)c.B);
  if (c.op == OP_KNN) {
    PYG_HIP_REQUIRE(c.k > 0, "%s: k must be positive", name);
    if (c.k > kMaxK) return fail(PYG_HIP_ERR_UNSUPPORTED, "%s: `k` must be <= %d on the device (got %lld)", name, kMaxK, (long long)c.k);
  }
  if (c.op == OP_RADIUS) PYG_HIP_REQUIRE(c.k >= 0 && c.r >= 0, "%s: r and max_num_neighbors must not be negative", name);
  if (c.M >= (1ll << 31) || c.N >= (1ll << 31) || c.B >= (1ll << 31) || c.D > kMaxD)
    return fail(PYG_HIP_ERR_UNSUPPORTED, "%s: 2^31 or more points, or more than %lld features: indices are 32-bit here", name,
                (long long)kMaxD);
  PYG_HIP_REQUIRE((c.cand || c.N == 0) && (c.query || c.M == 0), "%s: NULL point tensor", name);
  *plan = make_plan(c.op, c.dtype, c.M, c.N, c.B, c.D, c.k, c.flags);
  if (plan->route == PYG_HIP_SPATIAL_ROUTE_UNSUPPORTED) return fail(PYG_HIP_ERR_UNSUPPORTED, "%s: no kernel for these arguments", name);
  PYG_HIP_REQUIRE(c.ws != nullptr || c.M == 0, "%s: NULL workspace", name);
  if (c.M > 0 && ws_bytes < plan->total)
    return fail(PYG_HIP_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (pyg_hip_spatial_workspace_size)", name, ws_bytes,
                plan->total);
  PYG_HIP_REQUIRE((reinterpret_cast<uintptr_t>(c.ws) & 15) == 0, "%s: the workspace must be 16-byte aligned", name);
  return PYG_HIP_OK;
}

int run_typed(const Call& c, const Plan& p, int* bad, hipStream_t stream) {
  return p.f64 ? run<double>(c, p, bad, stream) : run<float>(c, p, bad, stream);
}

// knn / radius, first call: everything up to the pair count, which the host reads together with the pointer check
int count_pairs(const char* name, const Call& c, size_t ws_bytes, int64_t* num_pairs, hipStream_t stream) {
  Plan p;
  if (int rc = check_call(name, c, ws_bytes, &p)) return rc;
  PYG_HIP_REQUIRE(num_pairs != nullptr, "%s: NULL num_pairs", name);
  *num_pairs = 0;
  note_route(c.op, p);
  if (c.M == 0 || c.N == 0) return PYG_HIP_OK;
  int64_t* info = reinterpret_cast<int64_t*>(c.ws + p.o_info);
  if (int rc = run_typed(c, p, reinterpret_cast<int*>(info + 1), stream)) return rc;
  int64_t host[2] = {0, 0};
  PYG_HIP_CHECK(hipMemcpyAsync(host, info, 16, hipMemcpyDeviceToHost, stream));
  PYG_HIP_CHECK(hipStreamSynchronize(stream));
  PYG_HIP_REQUIRE(host[1] == 0, "%s: ptr_x / ptr_y must be non-decreasing and end at the number of rows", name);
  *num_pairs = host[0];
  return PYG_HIP_OK;
}

}  // namespace
}  // namespace pyg_hip

using namespace pyg_hip;

extern "C" {

int pyg_hip_spatial_route(int op, int dtype, int64_t M, int64_t N, int64_t B, int64_t D, int64_t k) {
  return make_plan(op, dtype, M, N, B, D, k, 0).route;
}

const char* pyg_hip_spatial_last_route(void) { return g_last_route; }

int pyg_hip_spatial_tile(int which) {
  switch (which) {
    case PYG_HIP_SPATIAL_TILE_QUERIES: return kQ;
    case PYG_HIP_SPATIAL_TILE_CANDIDATES: return kTileSmall;
    case PYG_HIP_SPATIAL_TILE_CHUNK_FORCED: return kChunkForced;
    case PYG_HIP_SPATIAL_TILE_ELEMS: return kTileElems;
    default: return 0;
  }
}

size_t pyg_hip_spatial_workspace_size(int op, int dtype, int64_t M, int64_t N, int64_t B, int64_t D, int64_t k, int flags) {
  const Plan p = make_plan(op, dtype, M, N, B, D, k, flags);
  return p.route == PYG_HIP_SPATIAL_ROUTE_UNSUPPORTED ? 0 : p.total;
}

int pyg_hip_knn(int dtype, const void* x, int64_t N, const void* y, int64_t M, int64_t D, const int64_t* ptr_x,
                const int64_t* ptr_y, int64_t num_examples, int64_t k, int flags, void* workspace, size_t workspace_bytes,
                int64_t* num_pairs, void* stream) {
  const Call c{OP_KNN, dtype, flags, x, y, ptr_x, ptr_y, N, M, num_examples, D, k, 0.0, static_cast<unsigned char*>(workspace), 0, nullptr, 0};
  return count_pairs("knn", c, workspace_bytes, num_pairs, static_cast<hipStream_t>(stream));
}

int pyg_hip_knn_emit(int dtype, int64_t N, int64_t M, int64_t D, int64_t num_examples, int64_t k, int flags, const void* workspace,
                     size_t workspace_bytes, int64_t num_pairs, int64_t* out, void* stream) {
  const Plan p = make_plan(OP_KNN, dtype, M, N, num_examples, D, k, flags);
  if (p.route == PYG_HIP_SPATIAL_ROUTE_UNSUPPORTED) return fail(PYG_HIP_ERR_UNSUPPORTED, "knn_emit: no kernel for these arguments");
  if (num_pairs == 0 || M == 0) return PYG_HIP_OK;
  PYG_HIP_REQUIRE(workspace && out && num_pairs > 0 && num_pairs <= M * k, "knn_emit: NULL tensor or a pair count outside [0, M * k]");
  if (workspace_bytes < p.total) return fail(PYG_HIP_ERR_WORKSPACE, "knn_emit: workspace of %zu bytes, %zu needed", workspace_bytes, p.total);
  const unsigned char* ws = static_cast<const unsigned char*>(workspace);
  hipLaunchKernelGGL(knn_emit_kernel, dim3((unsigned)ceil_div(M * k, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const int32_t*>(ws + p.o_nbr), reinterpret_cast<const int32_t*>(ws + p.o_cnt),
                     reinterpret_cast<const int64_t*>(ws + p.o_offs), M, (int)k, num_pairs, out);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

int pyg_hip_radius(int dtype, const void* x, int64_t N, const void* y, int64_t M, int64_t D, const int64_t* ptr_x,
                   const int64_t* ptr_y, int64_t num_examples, double r, int64_t max_num_neighbors, int flags, void* workspace,
                   size_t workspace_bytes, int64_t* num_pairs, void* stream) {
  // (no query keeps more neighbours than there are candidates: the count fits the kernels' 32-bit fields)
  const Call c{OP_RADIUS, dtype, flags, x, y, ptr_x, ptr_y, N, M, num_examples, D, std::min(max_num_neighbors, std::max<int64_t>(N, 0)), r,
               static_cast<unsigned char*>(workspace), 0, nullptr, 0};
  return count_pairs("radius", c, workspace_bytes, num_pairs, static_cast<hipStream_t>(stream));
}

int pyg_hip_radius_emit(int dtype, const void* x, int64_t N, const void* y, int64_t M, int64_t D, const int64_t* ptr_x,
                        const int64_t* ptr_y, int64_t num_examples, double r, int64_t max_num_neighbors, int flags, void* workspace,
                        size_t workspace_bytes, int64_t num_pairs, int64_t* out, void* stream) {
  const Call c{OP_RADIUS, dtype, flags, x, y, ptr_x, ptr_y, N, M, num_examples, D, std::min(max_num_neighbors, std::max<int64_t>(N, 0)), r,
               static_cast<unsigned char*>(workspace), 1, out, num_pairs};
  Plan p;
  if (int rc = check_call("radius_emit", c, workspace_bytes, &p)) return rc;
  if (num_pairs == 0 || M == 0 || N == 0) return PYG_HIP_OK;
  PYG_HIP_REQUIRE(out && num_pairs > 0, "radius_emit: NULL out or a negative pair count");
  return run_typed(c, p, nullptr, static_cast<hipStream_t>(stream));
}

int pyg_hip_nearest(int dtype, const void* x, int64_t N, const void* y, int64_t M, int64_t D, const int64_t* ptr_x,
                    const int64_t* ptr_y, int64_t num_examples, int flags, void* workspace, size_t workspace_bytes, int64_t* out,
                    void* stream) {
  // x are the queries here, y the candidates
  const Call c{OP_NEAREST, dtype, flags, y, x, ptr_y, ptr_x, M, N, num_examples, D, 1, 0.0, static_cast<unsigned char*>(workspace), 0, out, 0};
  Plan p;
  if (int rc = check_call("nearest", c, workspace_bytes, &p)) return rc;
  int* slot = nullptr;
  if (int rc = deferred_slot(&slot)) return rc;
  if (*static_cast<volatile int*>(slot) != 0) {
    *static_cast<volatile int*>(slot) = 0;
    return fail(PYG_HIP_ERR_INVALID, "nearest: an earlier call on this device had a ptr_x / ptr_y that was not non-decreasing or "
                                     "did not end at the number of rows (its result is unspecified)");
  }
  note_route(OP_NEAREST, p);
  if (N == 0) return PYG_HIP_OK;
  PYG_HIP_REQUIRE(out != nullptr, "nearest: NULL out");
  return run_typed(c, p, slot, static_cast<hipStream_t>(stream));
}

int pyg_hip_nearest_pending_error(void) {
  int* slot = nullptr;
  if (deferred_slot(&slot) != PYG_HIP_OK) return PYG_HIP_ERR_RUNTIME;
  const int pending = *static_cast<volatile int*>(slot);
  *static_cast<volatile int*>(slot) = 0;
  return pending;
}

}  // extern "C"
