// scatter_{sum,mul,min,max}, segment_*_coo and gather_coo for gfx950 (MI355X).
//
// Replaces pyg_lib/csrc/ops/cuda/scatter_kernel.cu and segment_coo_kernel.cu (warp-32 shuffles
// and CAS-emulated atomics, "ROCm wave64 is not a target") and follows the CPU contracts of
// pyg_lib/csrc/ops/cpu/scatter_kernel.cpp and segment_coo_kernel.cpp.
//
// One (B, E, K) layout serves every op (scatter_kernel.cpp:16-24): src[b, e, k] is reduced into
// out[b, index(b, e, k), k].  The index is addressed through three element strides so that a 1-D
// index broadcast along B and K (the common PyG case) or a COO index of shape [B, E] is read in
// place: algorithmic traffic stays 8*E + s*E*K + s*N*K instead of materialising an int64 per
// element as the reference front does (ops/autograd/scatter_kernel.cpp:33-39).
//
// HBM-bound byte work; the levers are coalesced 16-byte rows and few, native atomics:
//   * sum (fp32 / bf16 / fp16 / fp64 / int32 / int64): each thread owns a 16-byte column slice and a
//     short run of consecutive rows, accumulates in fp32 while the index repeats (sorted COO input
//     collapses whole runs, matching segment_coo_kernel.cpp's run accumulation) and flushes with
//     native global atomics (global_atomic_add_f32 / _pk_add_bf16 / _pk_add_f16 / _add_f64 / _add_x2).
//   * min / max: value pass with native integer atomics (CAS loop on the reference's `<` / `>` for
//     floating types), then an arg pass atomicMin(arg, e) over the elements that equal the final
//     value and strictly improved the initial one -- exactly the CPU kernel's first-match rule
//     (scatter_kernel.cpp:249-369) -- and a last pass that takes the value's bits from that position
//     (+0 and -0 tie: the first one seen stays), so values AND arg indices are bit-exact.
//   * mul and the 8/16-bit integer types: CAS loop on the containing 32-bit word.
#include "common.h"
#include "elem.h"

#include <limits>
#include <type_traits>

namespace pyg_hip {
namespace {

// ---- atomic read-modify-write on any 1/2/4/8-byte element -----------------------------------------
// f(old) -> {changed, new}.  Loops on the containing 32-bit word for sub-word types.
template <typename T, typename F>
__device__ void atomic_rmw(T* addr, F f) {
  if constexpr (sizeof(T) == 8) {
    unsigned long long* p = reinterpret_cast<unsigned long long*>(addr);
    unsigned long long old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (true) {
      T cur = __builtin_bit_cast(T, old);
      T nv;
      if (!f(cur, &nv)) return;
      unsigned long long want = __builtin_bit_cast(unsigned long long, nv);
      if (__hip_atomic_compare_exchange_strong(p, &old, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT))
        return;
    }
  } else if constexpr (sizeof(T) == 4) {
    unsigned int* p = reinterpret_cast<unsigned int*>(addr);
    unsigned int old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (true) {
      T cur = __builtin_bit_cast(T, old);
      T nv;
      if (!f(cur, &nv)) return;
      unsigned int want = __builtin_bit_cast(unsigned int, nv);
      if (__hip_atomic_compare_exchange_strong(p, &old, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT))
        return;
    }
  } else {
    const uintptr_t a = reinterpret_cast<uintptr_t>(addr);
    unsigned int* p = reinterpret_cast<unsigned int*>(a & ~(uintptr_t)3);
    const int shift = (int)(a & 3) * 8;
    constexpr unsigned int mask = sizeof(T) == 2 ? 0xffffu : 0xffu;
    unsigned int old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (true) {
      using U = typename std::conditional<sizeof(T) == 2, uint16_t, uint8_t>::type;
      const U curbits = (U)((old >> shift) & mask);
      T cur = __builtin_bit_cast(T, curbits);
      T nv;
      if (!f(cur, &nv)) return;
      const unsigned int want =
          (old & ~(mask << shift)) | ((unsigned int)__builtin_bit_cast(U, nv) << shift);
      if (__hip_atomic_compare_exchange_strong(p, &old, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT))
        return;
    }
  }
}

// CAS = true (PYG_HIP_SCATTER_CAS / PYG_HIP_FLOAT_ATOMICS=cas): float and double adds through a compare-and-swap loop
// instead of the hardware's floating-point atomic unit (same sum, same one rounding per add).
template <typename T, bool CAS = false>
__device__ void atomic_add(T* addr, typename Math<T>::acc_t v) {
  if constexpr (CAS && (std::is_same<T, float>::value || std::is_same<T, double>::value)) {
    atomic_rmw(addr, [v](T cur, T* nv) {
      *nv = cur + v;
      return true;
    });
  } else if constexpr (std::is_same<T, float>::value) {
    unsafeAtomicAdd(addr, v);  // global_atomic_add_f32
  } else if constexpr (std::is_same<T, double>::value) {
    unsafeAtomicAdd(addr, v);  // global_atomic_add_f64
  } else if constexpr (std::is_same<T, int32_t>::value) {
    atomicAdd(addr, v);
  } else if constexpr (std::is_same<T, int64_t>::value) {
    atomicAdd(reinterpret_cast<unsigned long long*>(addr), (unsigned long long)v);
  } else {
    atomic_rmw(addr, [v](T cur, T* nv) {
      *nv = Math<T>::down((typename Math<T>::acc_t)(Math<T>::up(cur) + v));
      return true;
    });
  }
}

template <typename T>
__device__ void atomic_mul(T* addr, T v) {
  atomic_rmw(addr, [v](T cur, T* nv) {
    *nv = Math<T>::down((typename Math<T>::acc_t)(Math<T>::up(cur) * Math<T>::up(v)));
    return true;
  });
}

template <typename T, bool IS_MIN>
__device__ void atomic_minmax(T* addr, T v) {
  if constexpr (std::is_same<T, int32_t>::value) {
    if (IS_MIN) atomicMin(addr, v); else atomicMax(addr, v);
  } else if constexpr (std::is_same<T, int64_t>::value) {
    if (IS_MIN) atomicMin(reinterpret_cast<long long*>(addr), (long long)v);
    else atomicMax(reinterpret_cast<long long*>(addr), (long long)v);
  } else {
    // the reference's strict comparison (v < *slot / v > *slot), NaNs never win
    atomic_rmw(addr, [v](T cur, T* nv) {
      const bool better = IS_MIN ? (Math<T>::up(v) < Math<T>::up(cur)) : (Math<T>::up(v) > Math<T>::up(cur));
      *nv = v;
      return better;
    });
  }
}

struct Shape {
  int64_t B, E, K, N;
  int64_t isb, ise, isk;  // index strides (elements) along b, e, k
};

__device__ __forceinline__ int64_t index_at(const int64_t* index, const Shape& s, int64_t b, int64_t e,
                                            int64_t k) {
  return index[b * s.isb + e * s.ise + k * s.isk];
}

// ---- generic element-per-thread kernels -------------------------------------------------------------
template <typename T, int OP, bool CAS = false>
__global__ void scatter_elem_kernel(const T* __restrict__ src, const int64_t* __restrict__ index, T* out,
                                    Shape s) {
  const int64_t total = s.B * s.E * s.K;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = i % s.K;
    const int64_t e = (i / s.K) % s.E;
    const int64_t b = i / (s.K * s.E);
    const int64_t idx = index_at(index, s, b, e, k);
    T* dst = out + (b * s.N + idx) * s.K + k;
    const T v = src[i];
    if (OP == OP_SUM) atomic_add<T, CAS>(dst, Math<T>::up(v));
    else if (OP == OP_MUL) atomic_mul<T>(dst, v);
    else if (OP == OP_MIN) atomic_minmax<T, true>(dst, v);
    else atomic_minmax<T, false>(dst, v);
  }
}

// arg pass of min/max: first source position whose value EQUALS the final bucket value (by value: +0 and -0 are one
// value, a NaN equals nothing), provided the bucket strictly improved on its initial state (init == nullptr: the type's
// max()/lowest()).  The value pass keeps whichever of +0 / -0 its CAS loop saw first, and atomics arrive in no fixed order:
// its zero may carry the wrong sign.  The position found here does not depend on that, and minmax_finish_kernel takes the
// value's bits from it -- what the reference's sequential strict compare keeps: the first of the equal values.
template <typename T, bool IS_MIN>
__global__ void scatter_arg_kernel(const T* __restrict__ src, const int64_t* __restrict__ index,
                                   const T* __restrict__ out, const T* __restrict__ init,
                                   int64_t* arg, Shape s) {
  const int64_t total = s.B * s.E * s.K;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = i % s.K;
    const int64_t e = (i / s.K) % s.E;
    const int64_t b = i / (s.K * s.E);
    const int64_t idx = index_at(index, s, b, e, k);
    const int64_t o = (b * s.N + idx) * s.K + k;
    const T fin = out[o];
    const T v = src[i];
    if (!same_value(v, fin)) continue;
    const T start = init ? init[o] : (IS_MIN ? type_max<T>() : type_lowest<T>());
    const bool improved = IS_MIN ? (Math<T>::up(fin) < Math<T>::up(start)) : (Math<T>::up(fin) > Math<T>::up(start));
    if (improved) atomicMin(reinterpret_cast<long long*>(arg + o), (long long)e);
  }
}

// last pass of the atomic min/max: a bucket with a winner takes its value's BITS from the winning position (see
// scatter_arg_kernel: the sign of a zero); empty buckets (arg still the sentinel E) of a freshly allocated output are reset
// to 0, those of a caller's output keep their value
template <typename T>
__global__ void minmax_finish_kernel(const T* __restrict__ src, T* out, const int64_t* __restrict__ arg, int fresh, Shape s) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= s.B * s.N * s.K) return;
  const int64_t e = arg[i];
  if (e == s.E) {
    if (fresh) out[i] = Math<T>::down((typename Math<T>::acc_t)0);
    return;
  }
  const int64_t k = i % s.K, b = i / (s.K * s.N);
  out[i] = src[(b * s.E + e) * s.K + k];
}

template <typename T>
__global__ void fill_kernel(T* out, int64_t n, T v) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) out[i] = v;
}

// `bytes` zero bytes at `p`, any alignment: 16-byte stores where the address allows, single bytes at both ends.  The atomic
// routes clear a fresh sum's `out` with this kernel and not with hipMemsetAsync: recorded into a HIP graph, the memset node in
// front of the atomic kernel did not clear `out` on replay (tests/test_graph_replay_gpu.py: garbage plus the sums), the same
// pattern as the hub counters of fused_reduce.hip and csr.hip ("HIP graphs").
__global__ void zero_bytes_kernel(unsigned char* __restrict__ p, size_t bytes) {
  const size_t to_16 = (16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15;
  const size_t head = to_16 < bytes ? to_16 : bytes;
  const size_t body = (bytes - head) / 16;
  const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, nth = gridDim.x * (size_t)blockDim.x;
  uint4* q = reinterpret_cast<uint4*>(p + head);
  for (size_t i = tid; i < body; i += nth) q[i] = make_uint4(0, 0, 0, 0);
  for (size_t i = tid; i < head; i += nth) p[i] = 0;
  for (size_t i = head + body * 16 + tid; i < bytes; i += nth) p[i] = 0;
}
inline int zero_bytes(void* p, size_t bytes, hipStream_t stream) {
  const size_t want = (bytes / 16 + 255) / 256 + 1;
  const size_t cap = (size_t)device_info().num_cus * 8;
  hipLaunchKernelGGL(zero_bytes_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, stream,
                     static_cast<unsigned char*>(p), bytes);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

__global__ void fill_i64_kernel(int64_t* out, int64_t n, int64_t v) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) out[i] = v;
}

// ---- vectorised sum: 16-byte column slices, run accumulation over consecutive rows ---------------------
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

template <typename T>
struct Vec;  // VEC elements per 16 bytes, accumulate in float/double/int
template <>
struct Vec<float> {
  static constexpr int N = 4;
  using acc_t = float;
  __device__ static void unpack(u32x4 v, float* a) {
    // (bit_cast straight from a vector-element lvalue miscompiles to element 0: copy out first)
    for (int i = 0; i < 4; ++i) {
      const uint32_t w = v[i];
      a[i] += __builtin_bit_cast(float, w);
    }
  }
  __device__ static void flush(float* dst, const float* a) {
    for (int i = 0; i < 4; ++i) unsafeAtomicAdd(dst + i, a[i]);
  }
  __device__ static void flush_cas(float* dst, const float* a) {
    for (int i = 0; i < 4; ++i) atomic_add<float, true>(dst + i, a[i]);
  }
  __device__ static void add_plain(float* dst, const float* a) {  // rows owned by this thread only
    float4 v = *reinterpret_cast<float4*>(dst);
    v.x += a[0]; v.y += a[1]; v.z += a[2]; v.w += a[3];
    *reinterpret_cast<float4*>(dst) = v;
  }
};
template <>
struct Vec<bf16_t> {
  static constexpr int N = 8;
  using acc_t = float;
  __device__ static void unpack(u32x4 v, float* a) {
    for (int i = 0; i < 4; ++i) {
      a[2 * i] += __builtin_bit_cast(float, v[i] << 16);
      a[2 * i + 1] += __builtin_bit_cast(float, v[i] & 0xffff0000u);
    }
  }
  __device__ static void flush(bf16_t* dst, const float* a) {
    for (int i = 0; i < 4; ++i) {
      bf16x2 p = {(__bf16)a[2 * i], (__bf16)a[2 * i + 1]};
      // global_atomic_pk_add_bf16
      (void)__builtin_amdgcn_global_atomic_fadd_v2bf16(
          (__attribute__((address_space(1))) bf16x2*)(dst + 2 * i), p);
    }
  }
  // the same packed add as a CAS loop on the pair's 32-bit word: each half = round(bf16(half) + bf16(a))
  __device__ static void flush_cas(bf16_t* dst, const float* a) {
    for (int i = 0; i < 4; ++i) {
      const float p0 = (float)(__bf16)a[2 * i], p1 = (float)(__bf16)a[2 * i + 1];
      atomic_rmw(reinterpret_cast<uint32_t*>(dst + 2 * i), [p0, p1](uint32_t cur, uint32_t* nv) {
        const uint16_t lo = __builtin_bit_cast(uint16_t, (__bf16)(__builtin_bit_cast(float, cur << 16) + p0));
        const uint16_t hi = __builtin_bit_cast(uint16_t, (__bf16)(__builtin_bit_cast(float, cur & 0xffff0000u) + p1));
        *nv = (uint32_t)lo | ((uint32_t)hi << 16);
        return true;
      });
    }
  }
  __device__ static void add_plain(bf16_t* dst, const float* a) {
    float cur[8] = {-0.f, -0.f, -0.f, -0.f, -0.f, -0.f, -0.f, -0.f};   // (unpack ADDS: from -0 it returns dst's values, a -0 included)
    unpack(*reinterpret_cast<const u32x4*>(dst), cur);
    u32x4 o;
    for (int i = 0; i < 4; ++i) {
      const uint16_t lo = __builtin_bit_cast(uint16_t, (__bf16)(cur[2 * i] + a[2 * i]));
      const uint16_t hi = __builtin_bit_cast(uint16_t, (__bf16)(cur[2 * i + 1] + a[2 * i + 1]));
      o[i] = (uint32_t)lo | ((uint32_t)hi << 16);
    }
    *reinterpret_cast<u32x4*>(dst) = o;
  }
};
template <>
struct Vec<f16_t> {
  static constexpr int N = 8;
  using acc_t = float;
  __device__ static void unpack(u32x4 v, float* a) {
    for (int i = 0; i < 4; ++i) {
      a[2 * i] += (float)__builtin_bit_cast(_Float16, (uint16_t)(v[i] & 0xffffu));
      a[2 * i + 1] += (float)__builtin_bit_cast(_Float16, (uint16_t)(v[i] >> 16));
    }
  }
  __device__ static void flush(f16_t* dst, const float* a) {
    for (int i = 0; i < 4; ++i) {
      f16x2 p = {(_Float16)a[2 * i], (_Float16)a[2 * i + 1]};
      (void)__builtin_amdgcn_global_atomic_fadd_v2f16(
          (__attribute__((address_space(1))) f16x2*)(dst + 2 * i), p);
    }
  }
  __device__ static void flush_cas(f16_t* dst, const float* a) {
    for (int i = 0; i < 4; ++i) {
      const float p0 = (float)(_Float16)a[2 * i], p1 = (float)(_Float16)a[2 * i + 1];
      atomic_rmw(reinterpret_cast<uint32_t*>(dst + 2 * i), [p0, p1](uint32_t cur, uint32_t* nv) {
        const uint16_t lo = __builtin_bit_cast(uint16_t, (_Float16)((float)__builtin_bit_cast(_Float16, (uint16_t)(cur & 0xffffu)) + p0));
        const uint16_t hi = __builtin_bit_cast(uint16_t, (_Float16)((float)__builtin_bit_cast(_Float16, (uint16_t)(cur >> 16)) + p1));
        *nv = (uint32_t)lo | ((uint32_t)hi << 16);
        return true;
      });
    }
  }
  __device__ static void add_plain(f16_t* dst, const float* a) {
    float cur[8] = {-0.f, -0.f, -0.f, -0.f, -0.f, -0.f, -0.f, -0.f};   // (unpack ADDS: from -0 it returns dst's values, a -0 included)
    unpack(*reinterpret_cast<const u32x4*>(dst), cur);
    u32x4 o;
    for (int i = 0; i < 4; ++i) {
      const uint16_t lo = __builtin_bit_cast(uint16_t, (_Float16)(cur[2 * i] + a[2 * i]));
      const uint16_t hi = __builtin_bit_cast(uint16_t, (_Float16)(cur[2 * i + 1] + a[2 * i + 1]));
      o[i] = (uint32_t)lo | ((uint32_t)hi << 16);
    }
    *reinterpret_cast<u32x4*>(dst) = o;
  }
};

// Requires K % Vec<T>::N == 0, 16-byte aligned src/out, index constant along k (isk == 0).
// SORTED: the index is ascending along e (segment_*_coo, or scatter through a sort permutation).  Then
// a thread owns 32 consecutive positions, every run strictly inside its chunk belongs to it alone and is
// added with a plain 16-byte read-modify-write; only the first and last run of a chunk (which may
// continue in the neighbouring chunks) use atomics.  Unsorted input: 8 positions, every flush atomic.
// perm (optional): source row of sorted position e (scatter via index_sort); index is then the SORTED key.
template <typename T, bool SORTED, bool CAS = false>
__global__ __launch_bounds__(256) void scatter_sum_vec_kernel(const T* __restrict__ src,
                                                              const int64_t* __restrict__ index,
                                                              const int64_t* __restrict__ perm, T* out,
                                                              Shape s) {
  constexpr int VN = Vec<T>::N;
  constexpr int R = SORTED ? 32 : 8;
  const int64_t kv = s.K / VN;  // 16-byte slices per row
  const int64_t chunks = (s.E + R - 1) / R;
  const int64_t total = s.B * chunks * kv;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = t % kv;
    const int64_t ch = (t / kv) % chunks;
    const int64_t b = t / (kv * chunks);
    const int64_t e0 = ch * R;
    const int64_t e1 = min(e0 + R, s.E);
    // (a run's accumulator starts from -0, the identity of a floating sum: x + -0 == x for every x, -0 + -0 == -0.  From +0 a
    // run of nothing but -0 would add +0 to a caller's -0 and turn it into +0, where the reference's sequential adds keep -0)
    float acc[VN];
#pragma unroll
    for (int i = 0; i < VN; ++i) acc[i] = -0.f;
    int64_t cur = index[b * s.isb + e0 * s.ise];
    bool first = true;
    // batches of 8 positions: their indices and 16-byte source slices are all requested before the first is consumed
    // (one dependent load per trip left the sorted sums at 4.3 TB/s: a wave had 1 KiB in flight)
    constexpr int U = 8;
    for (int64_t eb = e0; eb < e1; eb += U) {
      int64_t idxv[U];
      u32x4 val[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t e = eb + u < e1 ? eb + u : e1 - 1;
        idxv[u] = index[b * s.isb + e * s.ise];
        const int64_t srow = perm ? perm[e] : (b * s.E + e);
        val[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + srow * s.K + c * VN));
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (eb + u >= e1) break;
        const int64_t idx = idxv[u];
        if (idx != cur) {
          T* dst = out + (b * s.N + cur) * s.K + c * VN;
          if (SORTED && !first) Vec<T>::add_plain(dst, acc);
          else if (CAS) Vec<T>::flush_cas(dst, acc);
          else Vec<T>::flush(dst, acc);
          first = false;
#pragma unroll
          for (int i = 0; i < VN; ++i) acc[i] = -0.f;
          cur = idx;
        }
        Vec<T>::unpack(val[u], acc);
      }
    }
    if (CAS) Vec<T>::flush_cas(out + (b * s.N + cur) * s.K + c * VN, acc);
    else Vec<T>::flush(out + (b * s.N + cur) * s.K + c * VN, acc);
  }
}

// Unsorted 16-bit rows of an EVEN number of elements that the 16-byte-slice kernel above does not take (K = 2, 4, 6, 10, ...,
// and the narrow rows K <= 32): one (edge, pair) per thread, neighbouring lanes on neighbouring words, one packed atomic per
// pair instead of two 16-bit CAS loops on the same word (bf16 K = 4, 20 M edges: 2.5 ms -> 1.0).
template <typename T, bool CAS = false>
__global__ __launch_bounds__(256) void scatter_sum_pair_kernel(const T* __restrict__ src, const int64_t* __restrict__ index,
                                                               T* out, Shape s) {
  const int64_t kp = s.K / 2;
  const int64_t total = s.B * s.E * kp;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = t % kp;
    const int64_t e = (t / kp) % s.E;
    const int64_t b = t / (kp * s.E);
    const int64_t idx = index[b * s.isb + e * s.ise];
    const uint32_t w = *reinterpret_cast<const uint32_t*>(src + (b * s.E + e) * s.K + 2 * c);
    T* dst = out + (b * s.N + idx) * s.K + 2 * c;
    if constexpr (std::is_same<T, bf16_t>::value) {
      if (CAS) {
        const float p0 = __builtin_bit_cast(float, w << 16), p1 = __builtin_bit_cast(float, w & 0xffff0000u);
        atomic_rmw(reinterpret_cast<uint32_t*>(dst), [p0, p1](uint32_t cur, uint32_t* nv) {
          const uint16_t lo = __builtin_bit_cast(uint16_t, (__bf16)(__builtin_bit_cast(float, cur << 16) + p0));
          const uint16_t hi = __builtin_bit_cast(uint16_t, (__bf16)(__builtin_bit_cast(float, cur & 0xffff0000u) + p1));
          *nv = (uint32_t)lo | ((uint32_t)hi << 16);
          return true;
        });
      } else {
        (void)__builtin_amdgcn_global_atomic_fadd_v2bf16((__attribute__((address_space(1))) bf16x2*)dst, __builtin_bit_cast(bf16x2, w));
      }
    } else {
      if (CAS) {
        const float p0 = (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xffffu)), p1 = (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
        atomic_rmw(reinterpret_cast<uint32_t*>(dst), [p0, p1](uint32_t cur, uint32_t* nv) {
          const uint16_t lo = __builtin_bit_cast(uint16_t, (_Float16)((float)__builtin_bit_cast(_Float16, (uint16_t)(cur & 0xffffu)) + p0));
          const uint16_t hi = __builtin_bit_cast(uint16_t, (_Float16)((float)__builtin_bit_cast(_Float16, (uint16_t)(cur >> 16)) + p1));
          *nv = (uint32_t)lo | ((uint32_t)hi << 16);
          return true;
        });
      } else {
        (void)__builtin_amdgcn_global_atomic_fadd_v2f16((__attribute__((address_space(1))) f16x2*)dst, __builtin_bit_cast(f16x2, w));
      }
    }
  }
}

// ---- gather_coo -----------------------------------------------------------------------------------------
template <typename T>
__global__ void gather_elem_kernel(const T* __restrict__ src, const int64_t* __restrict__ index, T* out,
                                   int64_t B, int64_t E, int64_t K, int64_t N) {
  const int64_t total = B * E * K;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = i % K;
    const int64_t e = (i / K) % E;
    const int64_t b = i / (K * E);
    out[i] = src[(b * N + index[b * E + e]) * K + k];
  }
}

// 16-byte slices: `kv` slices per row
__global__ void gather_vec_kernel(const u32x4* __restrict__ src, const int64_t* __restrict__ index,
                                  u32x4* out, int64_t B, int64_t E, int64_t kv, int64_t N) {
  const int64_t total = B * E * kv;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = i % kv;
    const int64_t e = (i / kv) % E;
    const int64_t b = i / (kv * E);
    __builtin_nontemporal_store(src[(b * N + index[b * E + e]) * kv + c], out + i);
  }
}

// ---- host dispatch ----------------------------------------------------------------------------------------
inline unsigned grid_for(int64_t n, int threads = 256) {
  int64_t blocks = (n + threads - 1) / threads;
  const int64_t cap = (int64_t)device_info().num_cus * 16;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- the caller's workspace ----------------------------------------------------------------------------------
// CSR pointer of a sorted index: B * (N + 1) offsets
inline size_t indptr_bytes(int64_t B, int64_t N) {
  return align_up(sizeof(int64_t) * (size_t)(B > 0 ? B : 1) * (size_t)(N + 1), 256);
}
// The one layout, pyg_hip_scatter_workspace_size(B, E, N):  keys | perm | index_sort's scratch | indptr.  The sort-based
// route (B == 1) uses all four; a sorted index needs `indptr_bytes` only and keeps its offsets in FRONT.
struct Workspace {
  int64_t *keys, *perm, *indptr;
  void* sort_ws;
  size_t keys_bytes, sort_ws_bytes, bytes;
};
Workspace carve(void* ws, int64_t B, int64_t E, int64_t N) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(ws);  // (may be null: size query)
  Workspace w;
  w.keys_bytes = align_up(sizeof(int64_t) * (size_t)(E > 0 ? E : 1), 256);
  w.sort_ws_bytes = index_sort_ws_bytes_i64(E);
  w.keys = reinterpret_cast<int64_t*>(p);
  w.perm = reinterpret_cast<int64_t*>(p + w.keys_bytes);
  w.sort_ws = reinterpret_cast<void*>(p + 2 * w.keys_bytes);
  w.indptr = reinterpret_cast<int64_t*>(p + 2 * w.keys_bytes + w.sort_ws_bytes);
  w.bytes = 2 * w.keys_bytes + w.sort_ws_bytes + indptr_bytes(B, N);
  return w;
}

// indptr[b, r] = first position e of row b with index[b, e] >= r (index ascending along e)
__global__ void coo_indptr_kernel(const int64_t* __restrict__ index, int64_t isb, int64_t ise, int64_t B, int64_t E,
                                  int64_t N, int64_t* __restrict__ indptr) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= B * (N + 1)) return;
  const int64_t b = t / (N + 1), r = t % (N + 1);
  const int64_t* ip = index + b * isb;
  int64_t lo = 0, hi = E;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (ip[mid * ise] < r) lo = mid + 1; else hi = mid;
  }
  indptr[t] = lo;
}

// ---- the route: which kernel serves a call (the table of pyg_hip_scatter in pyg_hip.h) ------------------------------------
enum class Route {
  kNone = PYG_HIP_SCATTER_ROUTE_NONE,                // nothing to do
  kCsrRows = PYG_HIP_SCATTER_ROUTE_CSR_ROWS,         // sum, min, max: sorted index -> CSR rows
  kSortRows = PYG_HIP_SCATTER_ROUTE_SORT_ROWS,       // sum, min, max: index sort -> CSR rows through the permutation
  kVecSorted = PYG_HIP_SCATTER_ROUTE_VEC_SORTED,     // atomic sum: 16-byte slices, runs of 32 sorted positions
  kVecUnsorted = PYG_HIP_SCATTER_ROUTE_VEC_UNSORTED, // atomic sum: 16-byte slices, 8 positions
  kPair = PYG_HIP_SCATTER_ROUTE_PAIR,                // atomic sum: packed 16-bit pairs
  kElem = PYG_HIP_SCATTER_ROUTE_ELEM,                // atomic sum, and mul: one element per thread
  kAtomicMinMax = PYG_HIP_SCATTER_ROUTE_ATOMIC,      // min, max: value pass + arg pass + reset of the empty buckets
  kUnsupported = PYG_HIP_SCATTER_ROUTE_UNSUPPORTED,  // PYG_HIP_SCATTER_DETERMINISTIC, and no atomic-free kernel
};
inline bool rows_route(Route r) { return r == Route::kCsrRows || r == Route::kSortRows; }
inline const char* route_name(Route r) {
  static const char* const names[] = {"none", "csr_rows", "sort_rows", "vec_sorted", "vec_unsorted", "pair", "elem", "atomic", "unsupported"};
  return names[(int)r];
}
// pyg_hip_scatter_last_route(): the route of the last pyg_hip_scatter on this thread
thread_local Route g_last_route = Route::kNone;

struct Flags {  // the PYG_HIP_SCATTER_* bits of a call, decoded
  bool sorted, fresh_sum, cas, deterministic;
  explicit Flags(int f)
      : sorted(f & PYG_HIP_SCATTER_SORTED), fresh_sum(f & PYG_HIP_SCATTER_FRESH_SUM), cas(f & PYG_HIP_SCATTER_CAS),
        deterministic(f & PYG_HIP_SCATTER_DETERMINISTIC) {}
};

// The thresholds of the choice.
// One large unsorted index vector, for sums with rows of >= 64 bytes: sort the E indices once (3-4 radix passes over 16 E
// bytes), buckets become CSR rows reduced through the permutation in SOURCE order (the stable sort keeps it): no atomics,
// deterministic, every output row written once.
constexpr int64_t kSortMinEntries = 1 << 15;
constexpr int64_t kSortMinRowBytes = 64;
// Unsorted NARROW rows -- up to four 16-byte slices -- stay away from the slice kernel: a thread of it owns 8 consecutive
// edges of one slice, so with few slices per row its lanes are 128+ bytes apart on every load, and every lane's four atomics
// hit a line of their own.  One element / one packed pair per thread puts neighbouring lanes on neighbouring words of the
// same row: K = 4 floats, 20 M edges: 3.9 ms there, 0.96 here (= torch.index_add_); bf16 K = 16: 3.9 -> 1.0.
constexpr int64_t kNarrowSlices = 4;
// The slice kernel needs 16-byte aligned `src` and `out`, the pair kernel whole 32-bit words (K even, bases 4-byte aligned).
constexpr unsigned kSliceAlignMask = 15, kPairAlignMask = 3;

struct RowsNeed {  // what each rows route needs of the caller's workspace (from the one layout above)
  size_t csr_rows, sort_rows;
};
inline RowsNeed rows_need(const Shape& s) { return RowsNeed{indptr_bytes(s.B, s.N), carve(nullptr, 1, s.E, s.N).bytes}; }

// The route of a call with a valid `op` and `dtype`.  `workspace_bytes`: what the caller offers (0: nothing); `misalign`:
// the low four bits of src | out, which only decide among the slice, pair and element kernels.  Pure: no HIP call, no global.
Route choose_scatter_route(int op, int dtype, const Shape& s, const Flags& f, size_t workspace_bytes, const RowsNeed& need,
                           unsigned misalign) {
  if (s.B * s.E * s.K == 0) return Route::kNone;
  const int64_t size = (int64_t)dtype_size(dtype);
  const bool half = dtype == PYG_BF16 || dtype == PYG_F16;
  const bool float_t = dtype == PYG_F32 || half;  // what the slice kernel and the automatic sort-based sum take
  const bool floating = float_t || dtype == PYG_F64;
  const bool minmax = op == OP_MIN || op == OP_MAX;
  // Atomic-free: with an index broadcast along k and the caller's workspace, buckets are CSR rows -- as the index stands if it
  // ascends along e (the COO contract), or after sorting one index vector -- walked in source order (min / max: with the
  // reference's strict compare: values and first-match arg exact, no CAS loops, no second pass).
  if ((op == OP_SUM || minmax) && s.isk == 0) {
    if (f.sorted && workspace_bytes >= need.csr_rows) return Route::kCsrRows;
    const bool large = s.E >= kSortMinEntries && (minmax || (float_t && s.K * size >= kSortMinRowBytes));
    // PYG_HIP_SCATTER_DETERMINISTIC: the same route for a sum of ANY size, row width and floating type (float64 included)
    const bool forced = op == OP_SUM && f.deterministic && floating;
    if (!f.sorted && s.B == 1 && s.ise == 1 && (large || forced) && workspace_bytes >= need.sort_rows) return Route::kSortRows;
  }
  if (f.deterministic && floating && (op == OP_SUM || op == OP_MUL)) return Route::kUnsupported;
  if (minmax) return Route::kAtomicMinMax;
  if (op == OP_MUL) return Route::kElem;
  const int64_t slices = s.K / (16 / size);  // 16-byte slices of a row of whole slices
  if (float_t && s.isk == 0 && s.K % (16 / size) == 0 && (misalign & kSliceAlignMask) == 0 && (f.sorted || slices > kNarrowSlices))
    return f.sorted ? Route::kVecSorted : Route::kVecUnsorted;
  if (half && s.isk == 0 && s.K % 2 == 0 && !f.sorted && (misalign & kPairAlignMask) == 0) return Route::kPair;
  return Route::kElem;
}

// ---- the rows routes: CSR rows for csr.hip -------------------------------------------------------------------------------
struct Rows {  // `perm`: source row of sorted position e, or null; `scratch`: for hub rows
  const int64_t *indptr, *perm;
  void* scratch;
  size_t scratch_bytes;
};

int launch_indptr(const int64_t* index, int64_t isb, int64_t ise, const Shape& s, int64_t* indptr, hipStream_t stream) {
  const int64_t n = s.B * (s.N + 1);
  hipLaunchKernelGGL(coo_indptr_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, index, isb, ise, s.B, s.E,
                     s.N, indptr);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

// COO contract (index ascending along e): buckets are CSR rows -- reduced in source order in opmath, seeded from `out`, no
// atomics (the run accumulation of segment_coo_kernel.cpp:104-166, bit for bit)
int rows_of_sorted_index(const int64_t* index, const Shape& s, void* ws, size_t ws_bytes, hipStream_t stream, Rows* rows) {
  const size_t ip_bytes = indptr_bytes(s.B, s.N);
  // (what the workspace holds behind the offsets is scratch for hub rows)
  *rows = Rows{static_cast<int64_t*>(ws), nullptr, static_cast<char*>(ws) + ip_bytes, ws_bytes - ip_bytes};
  return launch_indptr(index, s.isb, s.ise, s, static_cast<int64_t*>(ws), stream);
}

// One unsorted index vector (B == 1): stable sort, then the offsets of the sorted keys; rows are read through the permutation
int rows_by_index_sort(const int64_t* index, const Shape& s, void* ws, hipStream_t stream, Rows* rows) {
  const Workspace w = carve(ws, 1, s.E, s.N);
  // (the sorted keys are dead once the offsets exist: scratch for hub rows)
  *rows = Rows{w.indptr, w.perm, w.keys, w.keys_bytes};
  const int rc = index_sort_i64(index, s.E, s.N > 0 ? s.N - 1 : 0, w.keys, w.perm, w.sort_ws, w.sort_ws_bytes, stream);
  return rc != PYG_HIP_OK ? rc : launch_indptr(w.keys, 0, 1, s, w.indptr, stream);
}

// ---- the atomic routes ---------------------------------------------------------------------------------------------------
template <typename... P, typename... A>
int launch(void (*kernel)(P...), int64_t threads, hipStream_t stream, A... args) {
  hipLaunchKernelGGL(kernel, dim3(grid_for(threads)), dim3(256), 0, stream, args...);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

// `cas`: the compare-and-swap flavour of the floating adds (PYG_HIP_SCATTER_CAS or the process default)
template <typename T>
int run_atomic(Route route, int op, bool cas, const void* src_, const int64_t* index, void* out_, int64_t* arg,
               const void* init_, const Shape& s, hipStream_t stream) {
  const T* src = static_cast<const T*>(src_);
  T* out = static_cast<T*>(out_);
  const T* init = static_cast<const T*>(init_);
  constexpr bool half = std::is_same<T, bf16_t>::value || std::is_same<T, f16_t>::value;
  const int64_t total = s.B * s.E * s.K;
  const int64_t outn = s.B * s.N * s.K;
  const int64_t* no_perm = nullptr;
  if constexpr (std::is_same<T, float>::value || half) {
    const int64_t kv = s.K / Vec<T>::N;
    if (route == Route::kVecSorted)
      return launch(cas ? scatter_sum_vec_kernel<T, true, true> : scatter_sum_vec_kernel<T, true>, s.B * ((s.E + 31) / 32) * kv,
                    stream, src, index, no_perm, out, s);
    if (route == Route::kVecUnsorted)
      return launch(cas ? scatter_sum_vec_kernel<T, false, true> : scatter_sum_vec_kernel<T, false>, s.B * ((s.E + 7) / 8) * kv,
                    stream, src, index, no_perm, out, s);
  }
  if constexpr (half) {
    if (route == Route::kPair)
      return launch(cas ? scatter_sum_pair_kernel<T, true> : scatter_sum_pair_kernel<T, false>, s.B * s.E * (s.K / 2), stream,
                    src, index, out, s);
  }
  if (op == OP_MUL) return launch(scatter_elem_kernel<T, OP_MUL>, total, stream, src, index, out, s);
  if (op == OP_SUM) {  // (of the element adds, only float and double have a CAS form of their own)
    constexpr bool kHasCas = std::is_same<T, float>::value || std::is_same<T, double>::value;
    return launch(cas ? scatter_elem_kernel<T, OP_SUM, kHasCas> : scatter_elem_kernel<T, OP_SUM>, total, stream, src, index,
                  out, s);
  }
  const unsigned grid = grid_for(total), ogrid = (unsigned)((outn + 255) / 256);
  hipLaunchKernelGGL(fill_i64_kernel, dim3(ogrid), dim3(256), 0, stream, arg, outn, s.E);
  const auto value_pass = op == OP_MIN ? scatter_elem_kernel<T, OP_MIN> : scatter_elem_kernel<T, OP_MAX>;
  const auto arg_pass = op == OP_MIN ? scatter_arg_kernel<T, true> : scatter_arg_kernel<T, false>;
  hipLaunchKernelGGL(value_pass, dim3(grid), dim3(256), 0, stream, src, index, out, s);
  hipLaunchKernelGGL(arg_pass, dim3(grid), dim3(256), 0, stream, src, index, out, init, arg, s);
  // (integers: equal values are equal bits, only the reset of a fresh output's empty buckets is left to do)
  if (!init || std::is_floating_point<T>::value || half)
    hipLaunchKernelGGL((minmax_finish_kernel<T>), dim3(ogrid), dim3(256), 0, stream, src, out, arg, init ? 0 : 1, s);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

// Runs a kernel route (not kNone, not kUnsupported).
int run_scatter(Route route, int op, int dtype, const void* src, const int64_t* index, void* out, int64_t* arg,
                const void* init, const Shape& s, const Flags& f, void* ws, size_t ws_bytes, hipStream_t stream) {
  const size_t out_bytes = dtype_size(dtype) * (size_t)(s.B * s.N * s.K);
  const bool fresh_sum = op == OP_SUM && f.fresh_sum;
  if (rows_route(route)) {
    Rows r;
    const int rc = route == Route::kCsrRows ? rows_of_sorted_index(index, s, ws, ws_bytes, stream, &r)
                                            : rows_by_index_sort(index, s, ws, stream, &r);
    if (rc != PYG_HIP_OK) return rc;
    if (op == OP_SUM)
      return segment_csr_sum(dtype, src, r.indptr, s.N + 1, r.perm, out, s.B, s.N, s.E, s.K, fresh_sum ? 1 : 0, stream,
                             r.scratch, r.scratch_bytes);
    return segment_csr_minmax(op == OP_MIN, dtype, src, r.indptr, s.N + 1, r.perm, out, arg, init ? 0 : 1, s.B, s.N, s.E, s.K,
                              stream, r.scratch, r.scratch_bytes);
  }
  // PYG_HIP_SCATTER_FRESH_SUM: `out` of a sum is uninitialised.  The rows routes write every slot and never read it; the
  // atomic routes accumulate into zeros, cleared here.
  if (fresh_sum && out_bytes > 0)
    if (int rc = zero_bytes(out, out_bytes, stream)) return rc;
  const bool cas = f.cas || float_atomic_mode() == 1;
  if (op == OP_SUM && (dtype == PYG_F32 || dtype == PYG_F64 || dtype == PYG_BF16 || dtype == PYG_F16))
    note_accumulate("pyg_hip_scatter (sum, atomic kernels)", out, out_bytes,
                    fresh_sum ? "this call (zero_bytes_kernel on the call's stream)" : "the caller (`out=` accumulation)", stream, cas ? 1 : 0);
  PYG_DISPATCH_ALL(dtype, (run_atomic<scalar_t>(route, op, cas, src, index, out, arg, init, s, stream)));
}

template <typename T>
int run_fill_extreme(int op, void* out_, int64_t n, hipStream_t stream) {
  if (n == 0) return PYG_HIP_OK;
  T* out = static_cast<T*>(out_);
  T v;
  // host-side constants (the device helpers are not callable here)
  if constexpr (std::is_same<T, bf16_t>::value) v = bf16_t{(uint16_t)(op == OP_MIN ? 0x7f7f : 0xff7f)};
  else if constexpr (std::is_same<T, f16_t>::value) v = f16_t{(uint16_t)(op == OP_MIN ? 0x7bff : 0xfbff)};
  else v = op == OP_MIN ? std::numeric_limits<T>::max() : std::numeric_limits<T>::lowest();
  hipLaunchKernelGGL((fill_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, out, n, v);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

template <typename T>
int run_gather(const void* src, const int64_t* index, void* out, int64_t B, int64_t E, int64_t K, int64_t N,
               hipStream_t stream) {
  const int64_t total = B * E * K;
  if (total == 0) return PYG_HIP_OK;
  const int64_t row_bytes = K * (int64_t)sizeof(T);
  if (row_bytes % 16 == 0 && aligned16(src) && aligned16(out)) {
    const int64_t kv = row_bytes / 16;
    hipLaunchKernelGGL(gather_vec_kernel, dim3(grid_for(B * E * kv)), dim3(256), 0, stream,
                       static_cast<const u32x4*>(src), index, static_cast<u32x4*>(out), B, E, kv, N);
  } else {
    hipLaunchKernelGGL((gather_elem_kernel<T>), dim3(grid_for(total)), dim3(256), 0, stream,
                       static_cast<const T*>(src), index, static_cast<T*>(out), B, E, K, N);
  }
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

}  // namespace
}  // namespace pyg_hip

using namespace pyg_hip;

extern "C" {

size_t pyg_hip_scatter_workspace_size(int64_t B, int64_t E, int64_t N) {
  return carve(nullptr, B < 1 ? 1 : B, E < 0 ? 0 : E, N < 0 ? 0 : N).bytes;
}

int pyg_hip_scatter_route(int op, int dtype, int64_t index_stride_b, int64_t index_stride_e, int64_t index_stride_k, int64_t B,
                          int64_t E, int64_t K, int64_t N, int flags, size_t workspace_bytes, unsigned misalign) {
  if (op < OP_SUM || op > OP_MAX || dtype_size(dtype) == 0 || B < 0 || E < 0 || K < 0 || N < 0)
    return PYG_HIP_SCATTER_ROUTE_UNSUPPORTED;
  const Shape s{B, E, K, N, index_stride_b, index_stride_e, index_stride_k};
  return (int)choose_scatter_route(op, dtype, s, Flags(flags), workspace_bytes, rows_need(s), misalign);
}

const char* pyg_hip_scatter_last_route(void) { return route_name(g_last_route); }

int pyg_hip_scatter(int op, int dtype, const void* src, const int64_t* index, int64_t index_stride_b,
                    int64_t index_stride_e, int64_t index_stride_k, void* out, int64_t* arg_out,
                    const void* out_init, int64_t B, int64_t E, int64_t K, int64_t N, int index_sorted,
                    void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  g_last_route = Route::kNone;
  PYG_HIP_REQUIRE(B >= 0 && E >= 0 && K >= 0 && N >= 0, "scatter: negative size");
  if (B * E * K == 0) {
    if (op == OP_SUM && (index_sorted & PYG_HIP_SCATTER_FRESH_SUM) && out && B * N * K > 0)
      if (int rc = zero_bytes(out, dtype_size(dtype) * (size_t)(B * N * K), stream)) return rc;
    if ((op == OP_MIN || op == OP_MAX) && arg_out && B * N * K > 0) {
      hipLaunchKernelGGL(fill_i64_kernel, dim3((unsigned)((B * N * K + 255) / 256)), dim3(256), 0, stream,
                         arg_out, B * N * K, E);
      PYG_HIP_CHECK(hipGetLastError());
    }
    return PYG_HIP_OK;
  }
  PYG_HIP_REQUIRE(src && index && out, "scatter: NULL tensor");
  PYG_HIP_REQUIRE(dtype_size(dtype) != 0, "unknown dtype %d", dtype);
  PYG_HIP_REQUIRE(op >= OP_SUM && op <= OP_MAX, "scatter: unknown reduce op %d", op);
  PYG_HIP_REQUIRE((op != OP_MIN && op != OP_MAX) || arg_out != nullptr, "scatter_min/max: 'arg_out' is NULL");
  const Shape s{B, E, K, N, index_stride_b, index_stride_e, index_stride_k};
  const Flags f(index_sorted);
  const size_t offered = workspace ? workspace_bytes : 0;
  const unsigned misalign = (unsigned)((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out)) & 15);
  const Route route = choose_scatter_route(op, dtype, s, f, offered, rows_need(s), misalign);
  g_last_route = route;
  if (route == Route::kUnsupported)
    return fail(PYG_HIP_ERR_UNSUPPORTED,
                "scatter: no atomic-free kernel for this reduction / index layout (PYG_HIP_SCATTER_DETERMINISTIC: floating sums "
                "need an index broadcast along k -- sorted, or one unsorted vector -- and the caller's workspace)");
  return run_scatter(route, op, dtype, src, index, out, arg_out, out_init, s, f, workspace, offered, stream);
}

int pyg_hip_fill_reduce_identity(int op, int dtype, void* out, int64_t n, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PYG_HIP_REQUIRE(op == OP_MIN || op == OP_MAX, "fill_reduce_identity: only min/max need a non-trivial fill");
  PYG_DISPATCH_ALL(dtype, (run_fill_extreme<scalar_t>(op, out, n, stream)));
}

int pyg_hip_gather_coo(int dtype, const void* src, const int64_t* index, void* out, int64_t B, int64_t E,
                       int64_t K, int64_t N, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PYG_HIP_REQUIRE(B >= 0 && E >= 0 && K >= 0 && N >= 0, "gather_coo: negative size");
  if (B * E * K == 0) return PYG_HIP_OK;
  PYG_HIP_REQUIRE(src && index && out, "gather_coo: NULL tensor");
  PYG_DISPATCH_ALL(dtype, (run_gather<scalar_t>(src, index, out, B, E, K, N, stream)));
}

}  // extern "C"
