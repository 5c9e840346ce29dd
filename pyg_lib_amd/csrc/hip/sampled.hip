// sampled_op for gfx950 (MI355X): out[e] = left[left_index[e]] (op) right[right_index[e]], and the per-edge gradients of
// its mul / div forms.
//
// Replaces pyg_lib/csrc/ops/cuda/sampled_kernel.cu (one element per thread, two 64-bit divisions per element, the operator
// and both "has index" flags tested per element, int64 indices only) and follows the CPU contract of
// pyg_lib/csrc/ops/cpu/sampled_kernel.cpp:17-46 (index_select + operator) bit for bit.
//
// HBM-bound byte work, no LDS: algorithmic traffic is two gathered row reads and one row write (3 E F elements + the
// index bytes) where the unfused expression writes and re-reads both gathered operands (7 E F).  The levers:
//   * rows of a multiple of 16 bytes on 16-byte aligned bases: one 16-byte slice per thread, neighbouring lanes on
//     neighbouring slices of the same output row; every other row (F = 1 ... 8 attention logits, odd F, offset bases): one
//     element per thread, neighbouring lanes on neighbouring elements.  One kernel template, the unit is its parameter;
//   * operator, index mode (none / left / right / both) and index type are template parameters: no per-element branch;
//   * a thread's (row, column) pair advances by a precomputed step: no division inside the loop;
//   * U units per trip: their indices, then their 2 U gathered operands are requested before the first is consumed;
//   * `out` is written once and not read again here: non-temporal stores (as gather_vec_kernel) keep the gathered rows,
//     which ARE re-read (every node once per incident edge), in the caches.
// Indices are not validated (include/pyg_hip.h).
#include "common.h"
#include "elem.h"

#include <type_traits>

namespace pyg_hip {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

enum { FN_ADD = PYG_SAMPLED_ADD, FN_SUB = PYG_SAMPLED_SUB, FN_MUL = PYG_SAMPLED_MUL, FN_DIV = PYG_SAMPLED_DIV };
enum { HAS_LEFT = 1, HAS_RIGHT = 2 };   // bits of MODE

template <typename T>
constexpr bool is_floating_v = std::is_same<T, float>::value || std::is_same<T, double>::value ||
                               std::is_same<T, bf16_t>::value || std::is_same<T, f16_t>::value;

// V elements moved as one unit: V == 1 (element path) or 16 bytes' worth
template <typename T, int V>
struct alignas(sizeof(T) * V) Pack {
  T v[V];
};

template <typename T, int V>
__device__ __forceinline__ void store_nt(Pack<T, V>* dst, const Pack<T, V>& p) {
  if constexpr (sizeof(Pack<T, V>) == 16) {
    __builtin_nontemporal_store(__builtin_bit_cast(u32x4, p), reinterpret_cast<u32x4*>(dst));
  } else {
    using R = typename std::conditional<sizeof(T) == 1, uint8_t, typename std::conditional<sizeof(T) == 2, uint16_t,
              typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type>::type>::type;
    static_assert(V == 1 && sizeof(R) == sizeof(T), "store_nt: one element or 16 bytes");
    __builtin_nontemporal_store(__builtin_bit_cast(R, p), reinterpret_cast<R*>(dst));
  }
}

// a (FN) b in the reference's opmath: fp32 for the 16-bit floats, rounded once; integers wrap
template <typename T, int FN>
__device__ __forceinline__ T apply(T a, T b) {
  if constexpr (is_floating_v<T>) {
    const typename Math<T>::acc_t x = Math<T>::up(a), y = Math<T>::up(b);
    return Math<T>::down(FN == FN_ADD ? x + y : FN == FN_SUB ? x - y : FN == FN_MUL ? x * y : x / y);
  } else {
    static_assert(FN != FN_DIV, "integer division has no device kernel");
    using W = typename std::conditional<sizeof(T) == 8, uint64_t, uint32_t>::type;
    const W x = (W)a, y = (W)b;
    return (T)(FN == FN_ADD ? x + y : FN == FN_SUB ? x - y : x * y);
  }
}

// position of a thread's current unit: row e, unit c of that row; advanced by the grid's stride without a division
struct Cursor {
  int64_t e, c;
};
struct Step {
  int64_t units;   // units per row
  int64_t de, dc;  // (grid threads) / units, (grid threads) % units
};
__device__ __forceinline__ Cursor first_unit(int64_t i, const Step& s) {
  Cursor p;
  p.e = i / s.units;
  p.c = i - p.e * s.units;
  return p;
}
__device__ __forceinline__ void advance(Cursor& p, const Step& s) {
  p.e += s.de;
  p.c += s.dc;
  if (p.c >= s.units) p.c -= s.units, ++p.e;
}

constexpr int kUnroll = 4;

template <typename T, int V, int FN, int MODE, typename I>
__global__ __launch_bounds__(256) void sampled_op_kernel(const Pack<T, V>* __restrict__ left,
                                                         const Pack<T, V>* __restrict__ right,
                                                         const I* __restrict__ left_index, const I* __restrict__ right_index,
                                                         Pack<T, V>* __restrict__ out, int64_t total, Step s) {
  using P = Pack<T, V>;
  constexpr int U = kUnroll;
  const int64_t nth = (int64_t)gridDim.x * blockDim.x;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  Cursor p = first_unit(i, s);
  for (; i + (U - 1) * nth < total; i += U * nth) {
    int64_t lo[U], ro[U];
    P a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t l = (MODE & HAS_LEFT) ? (int64_t)left_index[p.e] : p.e;
      const int64_t r = (MODE & HAS_RIGHT) ? (int64_t)right_index[p.e] : p.e;
      lo[u] = l * s.units + p.c;
      ro[u] = r * s.units + p.c;
      advance(p, s);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] = left[lo[u]], b[u] = right[ro[u]];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      P o;
#pragma unroll
      for (int k = 0; k < V; ++k) o.v[k] = apply<T, FN>(a[u].v[k], b[u].v[k]);
      store_nt(out + (i + u * nth), o);
    }
  }
  for (; i < total; i += nth) {
    const int64_t l = (MODE & HAS_LEFT) ? (int64_t)left_index[p.e] : p.e;
    const int64_t r = (MODE & HAS_RIGHT) ? (int64_t)right_index[p.e] : p.e;
    const P a = left[l * s.units + p.c], b = right[r * s.units + p.c];
    P o;
#pragma unroll
    for (int k = 0; k < V; ++k) o.v[k] = apply<T, FN>(a.v[k], b.v[k]);
    store_nt(out + i, o);
    advance(p, s);
  }
}

// per-edge gradients (include/pyg_hip.h): g = grad_out[e], a = left[li(e)], b = right[ri(e)]
template <typename T, int FN>
__device__ __forceinline__ void edge_grads(T g_, T a_, T b_, T* gl, T* gr) {
  using acc_t = typename Math<T>::acc_t;
  const acc_t g = Math<T>::up(g_), a = Math<T>::up(a_), b = Math<T>::up(b_);
  if constexpr (FN == FN_MUL) {
    *gl = Math<T>::down(g * b);
    *gr = Math<T>::down(g * a);
  } else {
    *gl = Math<T>::down(g / b);
    acc_t p = (-g) * ((a / b) / b);
    // (the product is pinned in its register before it is rounded: left alone, the fp16 element instance fuses multiply and
    // rounding into v_fma_mixlo_f16 q, -g, 0, and the +0 that adds turns a product of -0 into +0)
    if constexpr (std::is_same<acc_t, float>::value) asm("" : "+v"(p));
    *gr = Math<T>::down(p);
  }
}

// grad_left / grad_right: either may be null (wave-uniform tests)
template <typename T, int V, int FN, int MODE, typename I>
__global__ __launch_bounds__(256) void sampled_op_backward_kernel(const Pack<T, V>* __restrict__ grad_out,
                                                                  const Pack<T, V>* __restrict__ left,
                                                                  const Pack<T, V>* __restrict__ right,
                                                                  const I* __restrict__ left_index,
                                                                  const I* __restrict__ right_index,
                                                                  Pack<T, V>* __restrict__ grad_left,
                                                                  Pack<T, V>* __restrict__ grad_right, int64_t total, Step s) {
  using P = Pack<T, V>;
  constexpr int U = kUnroll;
  const int64_t nth = (int64_t)gridDim.x * blockDim.x;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  Cursor p = first_unit(i, s);
  for (; i + (U - 1) * nth < total; i += U * nth) {
    int64_t lo[U], ro[U];
    P g[U], a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t l = (MODE & HAS_LEFT) ? (int64_t)left_index[p.e] : p.e;
      const int64_t r = (MODE & HAS_RIGHT) ? (int64_t)right_index[p.e] : p.e;
      lo[u] = l * s.units + p.c;
      ro[u] = r * s.units + p.c;
      advance(p, s);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) g[u] = grad_out[i + u * nth], a[u] = left[lo[u]], b[u] = right[ro[u]];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      P ol, orr;
#pragma unroll
      for (int k = 0; k < V; ++k) edge_grads<T, FN>(g[u].v[k], a[u].v[k], b[u].v[k], &ol.v[k], &orr.v[k]);
      if (grad_left) store_nt(grad_left + (i + u * nth), ol);
      if (grad_right) store_nt(grad_right + (i + u * nth), orr);
    }
  }
  for (; i < total; i += nth) {
    const int64_t l = (MODE & HAS_LEFT) ? (int64_t)left_index[p.e] : p.e;
    const int64_t r = (MODE & HAS_RIGHT) ? (int64_t)right_index[p.e] : p.e;
    const P g = grad_out[i], a = left[l * s.units + p.c], b = right[r * s.units + p.c];
    P ol, orr;
#pragma unroll
    for (int k = 0; k < V; ++k) edge_grads<T, FN>(g.v[k], a.v[k], b.v[k], &ol.v[k], &orr.v[k]);
    if (grad_left) store_nt(grad_left + i, ol);
    if (grad_right) store_nt(grad_right + i, orr);
    advance(p, s);
  }
}

// ---- host dispatch ----------------------------------------------------------------------------------------
// kUnroll units per thread where there are that many (the cap of reduce.hip's grid_for: 16 workgroups per CU, the rest is
// the grid-stride loop)
inline unsigned grid_for(int64_t n) {
  int64_t blocks = (n + 256 * kUnroll - 1) / (256 * kUnroll);
  const int64_t cap = (int64_t)device_info().num_cus * 16;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

inline bool aligned16(const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct Args {
  const void *grad_out, *left, *right, *left_index, *right_index;
  void *out, *out2;   // forward: out; backward: edge_grad_left, edge_grad_right
  int64_t E, F;
  bool backward;
};

template <typename T, int V, int FN, int MODE, typename I>
int launch(const Args& a, hipStream_t stream) {
  using P = Pack<T, V>;
  Step s;
  s.units = a.F / V;
  const int64_t total = a.E * s.units;
  const unsigned grid = grid_for(total);
  const int64_t nth = (int64_t)grid * 256;
  s.de = nth / s.units;
  s.dc = nth % s.units;
  const I* li = static_cast<const I*>(a.left_index);
  const I* ri = static_cast<const I*>(a.right_index);
  if constexpr (FN == FN_MUL || FN == FN_DIV) {
    if constexpr (is_floating_v<T>) {
      if (a.backward) {
        hipLaunchKernelGGL((sampled_op_backward_kernel<T, V, FN, MODE, I>), dim3(grid), dim3(256), 0, stream,
                           static_cast<const P*>(a.grad_out), static_cast<const P*>(a.left), static_cast<const P*>(a.right),
                           li, ri, static_cast<P*>(a.out), static_cast<P*>(a.out2), total, s);
        PYG_HIP_CHECK(hipGetLastError());
        return PYG_HIP_OK;
      }
    }
  }
  hipLaunchKernelGGL((sampled_op_kernel<T, V, FN, MODE, I>), dim3(grid), dim3(256), 0, stream, static_cast<const P*>(a.left),
                     static_cast<const P*>(a.right), li, ri, static_cast<P*>(a.out), total, s);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

template <typename T, int V, int FN>
int launch_mode(const Args& a, int index_dtype, hipStream_t stream) {
  const int mode = (a.left_index ? HAS_LEFT : 0) | (a.right_index ? HAS_RIGHT : 0);
  if (mode == 0) return launch<T, V, FN, 0, int64_t>(a, stream);   // (no index is read: one instance)
  if (index_dtype == PYG_I32) {
    if (mode == HAS_LEFT) return launch<T, V, FN, HAS_LEFT, int32_t>(a, stream);
    if (mode == HAS_RIGHT) return launch<T, V, FN, HAS_RIGHT, int32_t>(a, stream);
    return launch<T, V, FN, HAS_LEFT | HAS_RIGHT, int32_t>(a, stream);
  }
  if (mode == HAS_LEFT) return launch<T, V, FN, HAS_LEFT, int64_t>(a, stream);
  if (mode == HAS_RIGHT) return launch<T, V, FN, HAS_RIGHT, int64_t>(a, stream);
  return launch<T, V, FN, HAS_LEFT | HAS_RIGHT, int64_t>(a, stream);
}

template <typename T, int FN>
int launch_unit(const Args& a, int index_dtype, hipStream_t stream) {
  constexpr int VN = 16 / (int)sizeof(T);
  const bool vec = (a.F * (int64_t)sizeof(T)) % 16 == 0 && aligned16(a.grad_out) && aligned16(a.left) && aligned16(a.right) &&
                   aligned16(a.out) && aligned16(a.out2);
  return vec ? launch_mode<T, VN, FN>(a, index_dtype, stream) : launch_mode<T, 1, FN>(a, index_dtype, stream);
}

template <typename T>
int run_sampled(int fn, const Args& a, int index_dtype, hipStream_t stream) {
  if constexpr (is_floating_v<T>) {
    if (fn == FN_DIV) return launch_unit<T, FN_DIV>(a, index_dtype, stream);
  } else {
    if (fn == FN_DIV || a.backward)
      return fail(PYG_HIP_ERR_UNSUPPORTED, a.backward ? "sampled_op_backward: floating-point dtypes only"
                                                      : "sampled_op: \"div\" not implemented for integer dtypes on the device");
  }
  if (fn == FN_MUL) return launch_unit<T, FN_MUL>(a, index_dtype, stream);
  if (a.backward) return fail(PYG_HIP_ERR_INVALID, "sampled_op_backward: fn must be PYG_SAMPLED_MUL or PYG_SAMPLED_DIV");
  return fn == FN_ADD ? launch_unit<T, FN_ADD>(a, index_dtype, stream) : launch_unit<T, FN_SUB>(a, index_dtype, stream);
}

int check_common(const char* name, int fn, int dtype, int64_t left_rows, int64_t right_rows, int index_dtype,
                 const void* left_index, const void* right_index, int64_t E, int64_t F) {
  PYG_HIP_REQUIRE(fn >= FN_ADD && fn <= FN_DIV, "%s: unknown fn %d (PYG_SAMPLED_ADD ... PYG_SAMPLED_DIV)", name, fn);
  PYG_HIP_REQUIRE(dtype_size(dtype) != 0, "%s: unknown dtype %d", name, dtype);
  PYG_HIP_REQUIRE(E >= 0 && F >= 0 && left_rows >= 0 && right_rows >= 0, "%s: negative size", name);
  PYG_HIP_REQUIRE(index_dtype == PYG_I64 || index_dtype == PYG_I32, "%s: index_dtype must be PYG_I64 or PYG_I32", name);
  PYG_HIP_REQUIRE(left_index || left_rows >= E, "%s: left has %lld rows, fewer than the %lld outputs it is read for without an index",
                  name, (long long)left_rows, (long long)E);
  PYG_HIP_REQUIRE(right_index || right_rows >= E, "%s: right has %lld rows, fewer than the %lld outputs it is read for without an index",
                  name, (long long)right_rows, (long long)E);
  return PYG_HIP_OK;
}

}  // namespace
}  // namespace pyg_hip

using namespace pyg_hip;

extern "C" {

int pyg_hip_sampled_op(int fn, int dtype, const void* left, int64_t left_rows, const void* right, int64_t right_rows,
                       int index_dtype, const void* left_index, const void* right_index, void* out, int64_t E, int64_t F,
                       void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int rc = check_common("sampled_op", fn, dtype, left_rows, right_rows, index_dtype, left_index, right_index, E, F);
  if (rc != PYG_HIP_OK) return rc;
  const bool integer = dtype != PYG_F32 && dtype != PYG_F64 && dtype != PYG_F16 && dtype != PYG_BF16;
  if (integer && fn == FN_DIV)
    return fail(PYG_HIP_ERR_UNSUPPORTED, "sampled_op: \"div\" not implemented for integer dtypes on the device");
  if (E == 0 || F == 0) return PYG_HIP_OK;
  PYG_HIP_REQUIRE(left && right && out, "sampled_op: NULL tensor");
  const Args a{nullptr, left, right, left_index, right_index, out, nullptr, E, F, false};
  PYG_DISPATCH_ALL(dtype, (run_sampled<scalar_t>(fn, a, index_dtype, stream)));
}

int pyg_hip_sampled_op_backward(int fn, int dtype, const void* grad_out, const void* left, int64_t left_rows,
                                const void* right, int64_t right_rows, int index_dtype, const void* left_index,
                                const void* right_index, void* edge_grad_left, void* edge_grad_right, int64_t E, int64_t F,
                                void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int rc = check_common("sampled_op_backward", fn, dtype, left_rows, right_rows, index_dtype, left_index, right_index, E, F);
  if (rc != PYG_HIP_OK) return rc;
  PYG_HIP_REQUIRE(fn == FN_MUL || fn == FN_DIV, "sampled_op_backward: fn must be PYG_SAMPLED_MUL or PYG_SAMPLED_DIV "
                  "(the edge gradient of add / sub is grad_out itself)");
  if (dtype != PYG_F32 && dtype != PYG_F64 && dtype != PYG_F16 && dtype != PYG_BF16)
    return fail(PYG_HIP_ERR_UNSUPPORTED, "sampled_op_backward: floating-point dtypes only");
  if (E == 0 || F == 0 || (!edge_grad_left && !edge_grad_right)) return PYG_HIP_OK;
  PYG_HIP_REQUIRE(grad_out && left && right, "sampled_op_backward: NULL tensor");
  const Args a{grad_out, left, right, left_index, right_index, edge_grad_left, edge_grad_right, E, F, true};
  PYG_DISPATCH_ALL(dtype, (run_sampled<scalar_t>(fn, a, index_dtype, stream)));
}

}  // extern "C"
