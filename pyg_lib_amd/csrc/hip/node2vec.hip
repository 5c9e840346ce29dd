// pyg::node2vec_walk_keyed on the device (include/pyg_hip.h: pyg_hip_node2vec_walk; the specification is DESIGN.md 2.16).
//
// One lane per walk.  A step is the uniform walk's two dependent reads (the rowptr pair of the current node, then a col
// entry) plus, per attempt, a binary search of the candidate in the PREVIOUS node's row, whose rowptr pair was validated
// when that node was current and stays in registers.  The attempt loop diverges by nature: its body is short (two Philox
// words, one col read, at most one search), the lane carries no per-walk arrays, and latency is hidden by resident waves
// rather than by walks per lane.  The search is skipped when a_near == a_far (q == 1), and x == t is tested first.
// Every step is stored straight from registers: a lane's row of the output is contiguous, so consecutive steps of a walk
// land in the same cache line.
//
// The acceptance and fallback arithmetic must round as the CPU key's does: no multiply feeds an add anywhere below, and
// contraction is switched off for the whole file so that it stays that way.
#pragma clang fp contract(off)

#include "common.h"

namespace pyg_hip {
namespace {

constexpr int kN2vThreads = 256;

// Philox4x32-10 as at::Philox4_32 (ATen/core/PhiloxRNGEngine.h) runs it: key = the halves of the 64-bit key, counter =
// (n_lo, n_hi, subsequence_lo, subsequence_hi), four words per counter value handed out in index order.
struct Philox {
  uint32_t k0, k1;
  uint32_t c0, c1, c2, c3;
  uint32_t w0, w1, w2, w3;
  int left;

  __device__ __forceinline__ Philox(uint64_t key, uint64_t subsequence)
      : k0((uint32_t)key), k1((uint32_t)(key >> 32)), c0(0), c1(0), c2((uint32_t)subsequence),
        c3((uint32_t)(subsequence >> 32)), w0(0), w1(0), w2(0), w3(0), left(0) {}

  __device__ __forceinline__ void block() {
    uint32_t x0 = c0, x1 = c1, x2 = c2, x3 = c3, a = k0, b = k1;
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
    w0 = x0, w1 = x1, w2 = x2, w3 = x3;
    if (++c0 == 0) ++c1;  // a walk never draws 2^66 words: the carry stops here
    left = 4;
  }

  __device__ __forceinline__ uint32_t next() {
    if (left == 0) block();
    const uint32_t r = w0;
    w0 = w1, w1 = w2, w2 = w3;
    --left;
    return r;
  }
};

__device__ __forceinline__ float uniform(uint32_t word) { return (float)(word >> 8) * 0x1p-24f; }

template <typename idx_t>
__global__ __launch_bounds__(kN2vThreads) void node2vec_walk_kernel(const idx_t* __restrict__ rowptr,
                                                                    const idx_t* __restrict__ col,
                                                                    const idx_t* __restrict__ seed, idx_t* __restrict__ out,
                                                                    int64_t num_nodes, int64_t num_edges, int64_t S,
                                                                    int64_t L, float a_ret, float a_near, float a_far,
                                                                    uint64_t key, int max_attempts) {
  const int64_t i = (int64_t)blockIdx.x * kN2vThreads + threadIdx.x;
  if (i >= S) return;
  idx_t* __restrict__ o = out + i * (L + 1);
  const bool search = a_near != a_far;
  Philox rng(key, (uint64_t)i);
  idx_t v = seed[i];
  o[0] = v;
  idx_t t = 0, trs = 0, tre = 0;  // the previous node and its row (from the second step on)

  // the acceptance threshold (= the transition weight) of candidate x: lower bound of x in col[trs, tre)
  auto weight = [&](idx_t x) -> float {
    if (x == t) return a_ret;
    if (!search) return a_near;
    idx_t lo = trs, hi = tre;
    while (lo < hi) {
      const idx_t mid = lo + (hi - lo) / 2;
      if (col[mid] < x)
        lo = mid + 1;
      else
        hi = mid;
    }
    return lo < tre && col[lo] == x ? a_near : a_far;
  };
  // position in a row of `deg` entries: the uniform walk's arithmetic (the clamp acts only where float(deg) rounds up)
  auto pick = [&](idx_t deg) -> idx_t {
    idx_t k = (idx_t)(uniform(rng.next()) * (float)deg);
    return k > deg - 1 ? deg - 1 : k;
  };

  for (int64_t j = 1; j <= L; ++j) {
    idx_t rs = 0, re = 0;
    if (v >= 0 && (int64_t)v < num_nodes) {
      rs = rowptr[v];
      re = rowptr[v + 1];
    }
    if (!(rs >= 0 && re > rs && (int64_t)re <= num_edges)) {
      // not a node, or no (valid) row: the walk stays here for good and draws nothing
      for (; j <= L; ++j) o[j] = v;
      break;
    }
    const idx_t deg = re - rs;
    idx_t x;
    if (j == 1) {
      x = col[rs + pick(deg)];
    } else {
      bool accepted = false;
      for (int a = 0; a < max_attempts; ++a) {
        x = col[rs + pick(deg)];
        const float r = uniform(rng.next());
        if (r < weight(x)) {
          accepted = true;
          break;
        }
      }
      if (!accepted) {
        // exact draw from the row's weights; bounds the step's time whatever p and q are
        const float u = uniform(rng.next());
        double total = 0;
        for (idx_t k = 0; k < deg; ++k) total += (double)weight(col[rs + k]);
        const double target = (double)u * total;
        double run = 0;
        idx_t k = 0;
        for (; k < deg - 1; ++k) {
          run += (double)weight(col[rs + k]);
          if (run > target) break;
        }
        x = col[rs + k];
      }
    }
    t = v, trs = rs, tre = re;
    v = x;
    o[j] = v;
  }
}

template <typename idx_t>
int node2vec_walk_t(const void* rowptr, int64_t N, const void* col, int64_t E, const void* seed, int64_t S, int64_t L,
                    float a_ret, float a_near, float a_far, uint64_t key, int max_attempts, void* out,
                    hipStream_t stream) {
  const int64_t blocks = (S + kN2vThreads - 1) / kN2vThreads;
  PYG_HIP_REQUIRE(blocks < (1ll << 31), "node2vec_walk: too many seeds (%lld)", (long long)S);
  hipLaunchKernelGGL((node2vec_walk_kernel<idx_t>), dim3((unsigned)blocks), dim3(kN2vThreads), 0, stream,
                     (const idx_t*)rowptr, (const idx_t*)col, (const idx_t*)seed, (idx_t*)out, N, E, S, L, a_ret, a_near,
                     a_far, key, max_attempts);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

}  // namespace
}  // namespace pyg_hip

using namespace pyg_hip;

extern "C" int pyg_hip_node2vec_walk(int index_dtype, const void* rowptr, int64_t num_nodes, const void* col,
                                     int64_t num_edges, const void* seed, int64_t num_seeds, int64_t walk_length,
                                     float a_ret, float a_near, float a_far, uint64_t key, int max_attempts, void* out,
                                     void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PYG_HIP_REQUIRE(index_dtype == PYG_I32 || index_dtype == PYG_I64,
                  "node2vec_walk: int32 or int64 indices expected on the device (got dtype code %d)", index_dtype);
  PYG_HIP_REQUIRE(walk_length >= 0, "node2vec_walk: walk_length must be non-negative (got %lld)", (long long)walk_length);
  PYG_HIP_REQUIRE(num_nodes >= 0 && num_edges >= 0 && num_seeds >= 0, "node2vec_walk: negative size");
  PYG_HIP_REQUIRE(max_attempts >= 0 && max_attempts <= 1024, "node2vec_walk: max_attempts must lie in [0, 1024] (got %d)",
                  max_attempts);
  // written so that a NaN fails
  PYG_HIP_REQUIRE(a_ret > 0 && a_ret <= 1 && a_near > 0 && a_near <= 1 && a_far > 0 && a_far <= 1,
                  "node2vec_walk: thresholds must lie in (0, 1] (got %g, %g, %g)", (double)a_ret, (double)a_near,
                  (double)a_far);
  if (num_seeds == 0) return PYG_HIP_OK;
  PYG_HIP_REQUIRE(rowptr && seed && out && (walk_length == 0 || col || num_edges == 0), "node2vec_walk: NULL buffer");
  if (index_dtype == PYG_I32)
    return node2vec_walk_t<int32_t>(rowptr, num_nodes, col, num_edges, seed, num_seeds, walk_length, a_ret, a_near, a_far,
                                    key, max_attempts, out, stream);
  return node2vec_walk_t<int64_t>(rowptr, num_nodes, col, num_edges, seed, num_seeds, walk_length, a_ret, a_near, a_far, key,
                                  max_attempts, out, stream);
}
