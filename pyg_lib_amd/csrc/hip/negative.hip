// pyg::edge_lookup and pyg::negative_sample_keyed on the device (include/pyg_hip.h: pyg_hip_edge_lookup,
// pyg_hip_negative_sample; the specification is DESIGN.md 2.18).
//
// One lane per item, 256 lanes per workgroup, a bounded grid that strides over the items (their number may pass 2^31).  An
// item is a chain of dependent reads -- the rowptr pair, then binary searches over the row -- so latency is hidden by
// resident waves and by nothing else: no LDS, no atomics, no per-lane arrays.  The lanes of one source are neighbours
// (item = source * num_neg + draw): their window searches are the same and hit the same cache lines, only the last
// search (the r-th non-neighbour) differs.  One Philox4x32-10 block per item, two of its words used.  Integer arithmetic
// only, all of it in int64 whatever the index type, so the result does not depend on the index type or the device.

#include "common.h"

namespace pyg_hip {
namespace {

constexpr int kNegThreads = 256;
// 8 workgroups of 4 waves fill a CU's wave slots at this kernel's register count; four rounds of that so that a
// workgroup that drew the hub rows does not become the tail
constexpr int64_t kNegMaxBlocks = 256 * 8 * 4;

// w = (w0 << 32) | w1 of at::Philox4_32(key, subsequence, 0): the rounds as node2vec.hip carries them
__device__ __forceinline__ uint64_t philox_word64(uint64_t key, uint64_t subsequence) {
  uint32_t x0 = 0, x1 = 0, x2 = (uint32_t)subsequence, x3 = (uint32_t)(subsequence >> 32);
  uint32_t a = (uint32_t)key, b = (uint32_t)(key >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, x0), lo0 = 0xD2511F53u * x0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, x2), lo1 = 0xCD9E8D57u * x2;
    x0 = hi1 ^ x1 ^ a;
    x1 = lo1;
    x2 = hi0 ^ x3 ^ b;
    x3 = lo0;
    a += 0x9E3779B9u;
    b += 0xBB67AE85u;
  }
  return ((uint64_t)x0 << 32) | x1;
}

// a draw below n (n > 0): the high half of w * n
__device__ __forceinline__ int64_t draw_below(uint64_t w, int64_t n) { return (int64_t)__umul64hi(w, (uint64_t)n); }

// first position of W[0, n) whose value is not below x
template <typename idx_t>
__device__ __forceinline__ int64_t lower_bound(const idx_t* __restrict__ W, int64_t n, int64_t x) {
  int64_t a = 0, b = n;
  while (a < b) {
    const int64_t mid = (a + b) / 2;
    if ((int64_t)W[mid] < x)
      a = mid + 1;
    else
      b = mid;
  }
  return a;
}

// The r-th value of lo, lo + 1, ... that is not in W[0, n) (W ascending within [lo, hi), r < (hi - lo) - n).  A value
// below lo always sends the search right and one at or above hi always left, whatever its size: clamping it first
// changes no decision and keeps W[mid] - lo - mid inside int64 on rows that break the precondition.
template <typename idx_t>
__device__ __forceinline__ int64_t kth(const idx_t* __restrict__ W, int64_t n, int64_t lo, int64_t hi, int64_t r) {
  int64_t a = 0, b = n;
  while (a < b) {
    const int64_t mid = (a + b) / 2;
    int64_t v = (int64_t)W[mid];
    v = v < lo ? lo - 1 : (v > hi ? hi : v);
    if (v - lo - mid > r)
      b = mid;
    else
      a = mid + 1;
  }
  return lo + r + a;
}

// the rowptr pair of source s, if it is one
template <typename idx_t>
__device__ __forceinline__ bool valid_row(const idx_t* __restrict__ rowptr, int64_t num_src, int64_t num_edges, int64_t s,
                                          int64_t& rs, int64_t& re) {
  if (s < 0 || s >= num_src) return false;
  rs = (int64_t)rowptr[s];
  re = (int64_t)rowptr[s + 1];
  return rs >= 0 && re <= num_edges && re >= rs;
}

template <typename idx_t>
__global__ __launch_bounds__(kNegThreads) void edge_lookup_kernel(const idx_t* __restrict__ rowptr,
                                                                  const idx_t* __restrict__ col,
                                                                  const idx_t* __restrict__ src,
                                                                  const idx_t* __restrict__ dst, idx_t* __restrict__ out,
                                                                  int64_t num_src, int64_t num_edges, int64_t Q) {
  const int64_t step = (int64_t)gridDim.x * kNegThreads;
  for (int64_t q = (int64_t)blockIdx.x * kNegThreads + threadIdx.x; q < Q; q += step) {
    int64_t rs, re, found = -1;
    if (valid_row(rowptr, num_src, num_edges, (int64_t)src[q], rs, re)) {
      const int64_t x = (int64_t)dst[q];
      const int64_t k = lower_bound(col + rs, re - rs, x);
      if (k < re - rs && (int64_t)col[rs + k] == x) found = rs + k;
    }
    out[q] = (idx_t)found;
  }
}

// src != NULL: out[i * num_neg + j]
template <typename idx_t>
__global__ __launch_bounds__(kNegThreads) void negative_structured_kernel(
    const idx_t* __restrict__ rowptr, const idx_t* __restrict__ col, const idx_t* __restrict__ src,
    const idx_t* __restrict__ ptr, idx_t* __restrict__ out, int64_t num_src, int64_t num_edges, int64_t num_dst,
    int64_t num_neg, int64_t items, int64_t G, uint64_t key, int exclude_self) {
  const int64_t step = (int64_t)gridDim.x * kNegThreads;
  // (i, j) = (t / num_neg, t % num_neg) is carried from one stride to the next: two 64-bit divisions per lane, none per item
  const int64_t i_step = step / num_neg, j_step = step % num_neg;
  int64_t t = (int64_t)blockIdx.x * kNegThreads + threadIdx.x;
  int64_t i = t / num_neg, j = t % num_neg;
  for (; t < items; t += step, i += i_step, j += j_step) {
    if (j >= num_neg) j -= num_neg, ++i;
    const int64_t s = (int64_t)src[i];
    int64_t rs, re, x = -1;
    if (valid_row(rowptr, num_src, num_edges, s, rs, re)) {
      int64_t lo = 0, hi = num_dst;
      bool in_graph = true;
      if (ptr != nullptr) {
        int64_t a = 0, b = G + 1;
        while (a < b) {
          const int64_t mid = (a + b) / 2;
          if ((int64_t)ptr[mid] <= s)
            a = mid + 1;
          else
            b = mid;
        }
        const int64_t g = a - 1;
        in_graph = g >= 0 && g < G;
        if (in_graph) {
          lo = (int64_t)ptr[g];
          hi = (int64_t)ptr[g + 1];
          lo = lo < 0 ? 0 : lo;
          hi = hi > num_dst ? num_dst : hi;
        }
      }
      // an empty range has no candidate (n <= 0 below); decided here, where a wild ptr cannot yet overflow hi - lo
      if (in_graph && hi > lo) {
        const idx_t* __restrict__ row = col + rs;
        const int64_t p_lo = lower_bound(row, re - rs, lo), p_hi = lower_bound(row, re - rs, hi);
        const idx_t* __restrict__ W = row + p_lo;
        const int64_t d = p_hi > p_lo ? p_hi - p_lo : 0;
        bool self_ex = false;
        if (exclude_self && lo <= s && s < hi) {
          const int64_t k = lower_bound(W, d, s);
          self_ex = !(k < d && (int64_t)W[k] == s);
        }
        const int64_t n = (hi - lo) - d - (self_ex ? 1 : 0);
        if (n > 0) {
          const int64_t r = draw_below(philox_word64(key, (uint64_t)t), n);
          x = kth(W, d, lo, hi, r);
          if (self_ex && x >= s) x = kth(W, d, lo, hi, r + 1);
        }
      }
    }
    out[t] = (idx_t)x;
  }
}

// src == NULL: out[j] = source, out[num_neg + j] = destination
template <typename idx_t>
__global__ __launch_bounds__(kNegThreads) void negative_global_kernel(const idx_t* __restrict__ rowptr,
                                                                      const idx_t* __restrict__ col,
                                                                      idx_t* __restrict__ out, int64_t num_src,
                                                                      int64_t num_edges, int64_t num_dst, int64_t num_neg,
                                                                      int64_t T, uint64_t key) {
  const int64_t step = (int64_t)gridDim.x * kNegThreads;
  for (int64_t t = (int64_t)blockIdx.x * kNegThreads + threadIdx.x; t < num_neg; t += step) {
    int64_t s = -1, x = -1;
    if (T > 0) {
      const int64_t R = draw_below(philox_word64(key, (uint64_t)t), T);
      int64_t a = 0, b = num_src;
      while (a < b) {
        const int64_t mid = (a + b) / 2;
        // (mid + 1) * num_dst - rowptr[mid + 1] > R with the rowptr entry alone on its side: nothing overflows
        if ((int64_t)rowptr[mid + 1] < (mid + 1) * num_dst - R)
          b = mid;
        else
          a = mid + 1;
      }
      int64_t rs, re;
      if (a < num_src && valid_row(rowptr, num_src, num_edges, a, rs, re)) {
        const int64_t r = R - (a * num_dst - rs);
        if (r >= 0 && r < num_dst - (re - rs)) {
          s = a;
          x = kth(col + rs, re - rs, (int64_t)0, num_dst, r);
        }
      }
    }
    out[t] = (idx_t)s;
    out[num_neg + t] = (idx_t)x;
  }
}

inline unsigned blocks_for(int64_t items) {
  const int64_t blocks = (items + kNegThreads - 1) / kNegThreads;
  return (unsigned)(blocks < kNegMaxBlocks ? blocks : kNegMaxBlocks);
}

template <typename idx_t>
int edge_lookup_t(const void* rowptr, int64_t num_src, const void* col, int64_t num_edges, const void* src, const void* dst,
                  int64_t Q, void* out, hipStream_t stream) {
  hipLaunchKernelGGL((edge_lookup_kernel<idx_t>), dim3(blocks_for(Q)), dim3(kNegThreads), 0, stream, (const idx_t*)rowptr,
                     (const idx_t*)col, (const idx_t*)src, (const idx_t*)dst, (idx_t*)out, num_src, num_edges, Q);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

template <typename idx_t>
int negative_sample_t(const void* rowptr, int64_t num_src, const void* col, int64_t num_edges, const void* src,
                      int64_t items, int64_t num_dst, int64_t num_neg, uint64_t key, int exclude_self, const void* ptr,
                      int64_t G, int64_t T, void* out, hipStream_t stream) {
  if (src != nullptr)
    hipLaunchKernelGGL((negative_structured_kernel<idx_t>), dim3(blocks_for(items)), dim3(kNegThreads), 0, stream,
                       (const idx_t*)rowptr, (const idx_t*)col, (const idx_t*)src, (const idx_t*)ptr, (idx_t*)out, num_src,
                       num_edges, num_dst, num_neg, items, G, key, exclude_self);
  else
    hipLaunchKernelGGL((negative_global_kernel<idx_t>), dim3(blocks_for(num_neg)), dim3(kNegThreads), 0, stream,
                       (const idx_t*)rowptr, (const idx_t*)col, (idx_t*)out, num_src, num_edges, num_dst, num_neg, T, key);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

}  // namespace
}  // namespace pyg_hip

using namespace pyg_hip;

extern "C" int pyg_hip_edge_lookup(int index_dtype, const void* rowptr, int64_t num_src, const void* col, int64_t num_edges,
                                   const void* src, const void* dst, int64_t num_queries, void* out, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PYG_HIP_REQUIRE(index_dtype == PYG_I32 || index_dtype == PYG_I64,
                  "edge_lookup: int32 or int64 indices expected on the device (got dtype code %d)", index_dtype);
  PYG_HIP_REQUIRE(num_src >= 0 && num_edges >= 0 && num_queries >= 0, "edge_lookup: negative size");
  if (num_queries == 0) return PYG_HIP_OK;
  PYG_HIP_REQUIRE(rowptr && src && dst && out && (col || num_edges == 0), "edge_lookup: NULL buffer");
  if (index_dtype == PYG_I32)
    return edge_lookup_t<int32_t>(rowptr, num_src, col, num_edges, src, dst, num_queries, out, stream);
  return edge_lookup_t<int64_t>(rowptr, num_src, col, num_edges, src, dst, num_queries, out, stream);
}

extern "C" int pyg_hip_negative_sample(int index_dtype, const void* rowptr, int64_t num_src, const void* col,
                                       int64_t num_edges, const void* src, int64_t num_items, int64_t num_dst,
                                       int64_t num_neg, uint64_t key, int exclude_self, const void* ptr, int64_t num_graphs,
                                       void* out, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PYG_HIP_REQUIRE(index_dtype == PYG_I32 || index_dtype == PYG_I64,
                  "negative_sample: int32 or int64 indices expected on the device (got dtype code %d)", index_dtype);
  PYG_HIP_REQUIRE(num_src >= 0 && num_edges >= 0 && num_items >= 0 && num_dst >= 0 && num_neg >= 0 && num_graphs >= 0,
                  "negative_sample: negative size");
  PYG_HIP_REQUIRE(index_dtype == PYG_I64 || num_dst <= INT32_MAX,
                  "negative_sample: num_dst = %lld does not fit int32 indices", (long long)num_dst);
  int64_t cells = 0, items = num_neg;
  PYG_HIP_REQUIRE(!__builtin_mul_overflow(num_src, num_dst, &cells),
                  "negative_sample: num_src * num_dst = %lld * %lld overflows int64", (long long)num_src, (long long)num_dst);
  if (src == nullptr) {
    PYG_HIP_REQUIRE(!exclude_self && ptr == nullptr,
                    "negative_sample: exclude_self and ptr need 'src' (the global form has neither)");
  } else {
    PYG_HIP_REQUIRE(!__builtin_mul_overflow(num_items, num_neg, &items), "negative_sample: %lld x %lld items overflow int64",
                    (long long)num_items, (long long)num_neg);
  }
  if (items == 0) return PYG_HIP_OK;
  PYG_HIP_REQUIRE(out && (rowptr || num_src == 0) && (col || num_edges == 0), "negative_sample: NULL buffer");
  const int64_t T = cells - num_edges;  // cells >= 0, num_edges >= 0: no overflow
  if (index_dtype == PYG_I32)
    return negative_sample_t<int32_t>(rowptr, num_src, col, num_edges, src, items, num_dst, num_neg, key, exclude_self, ptr,
                                      num_graphs, T, out, stream);
  return negative_sample_t<int64_t>(rowptr, num_src, col, num_edges, src, items, num_dst, num_neg, key, exclude_self, ptr,
                                    num_graphs, T, out, stream);
}
