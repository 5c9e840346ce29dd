// Element types, the device-side group descriptor and the MFMA / rounding / packing helpers shared by the translation
// units of segment_matmul / grouped_matmul, and the launch functions through which matmul.hip (tile tables, route choice,
// entry points) reaches the kernel families: matmul_lds.hip (W in LDS, contiguous tile ranges), matmul_f32_pipe.hip
// (fp32 K = 128), matmul_k128.hip (16-bit K = M = 128: cyclic / ticket schedules), matmul_k256.hip (16-bit K = 256, 256
// columns per workgroup), matmul_ring.hip (item rings), matmul_gen.hip (general shapes).  The weight gradient has the same shape: matmul_dw.hip
// (plan, workspace layout, route choice, entry points, the shape-specialised kernels) reaches matmul_dw_gen.hip (general
// shapes) through launch_dw_gen; the descriptors of both and the host-`ptr` staging of all entry points are declared here.
#pragma once

#include "common.h"

#include <string.h>

#include <algorithm>

namespace pyg_hip {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kTileRows = 128;  // rows per workgroup tile in the MFMA kernels (4 waves x 32)
constexpr int kPairRows = 64;   // rows per tile of the ticket kernel (2 waves x 32)
constexpr int kTicketWords = 256;  // 8 per-XCD tile counters, 128 bytes apart

struct bf16_t {
  uint16_t v;
};
struct f16_t {
  uint16_t v;
};

// Device-side group descriptor (48 bytes).
struct DevGroup {
  const char* a;
  const char* w;
  char* c;
  const char* bias;
  int64_t rows;
  int32_t k;
  int32_t m;
  int32_t trans;
  int32_t pad;
};

// Weight gradient, shape-specialised kernels: `rows` rows of X [rows, K] and dY [rows, M] (row-major, M = row pitch of dY).
struct DwGroup {
  const uint16_t* x;
  const uint16_t* dy;
  int64_t rows;
};

// Weight gradient, general-shape kernel.
struct DwGenGroup {  // 48 bytes
  const char* x;     // [rows, k] row-major
  const char* dy;    // [rows, m] row-major
  int64_t rows;
  int64_t acc_off;   // first element of this group's [k, m] block in the fp32 image (and in the output pool)
  int32_t k, m;
  int16_t lx, ly;    // log2 of the vector bytes the X / dY rows may be fetched with (1 ... 4)
  int16_t nkb, nmb;  // blocks along k and m
};
static_assert(sizeof(DwGenGroup) == 48, "DwGenGroup layout");

// Output block of the general-shape weight-gradient kernel: 128 x 128 entries, 128 x 64 for 4-byte elements.
constexpr int kDwGenKB = 128;
constexpr int dw_gen_mb(int elt) { return elt == 4 ? 64 : 128; }

template <typename T>
struct Elem;
template <>
struct Elem<bf16_t> {
  static constexpr int kSize = 2;
  static constexpr int kPerChunk = 8;   // elements per 16-byte chunk
  static constexpr int kStepsPerChunk = 1;  // MFMA k-steps fed by one chunk
};
template <>
struct Elem<f16_t> {
  static constexpr int kSize = 2;
  static constexpr int kPerChunk = 8;
  static constexpr int kStepsPerChunk = 1;
};
template <>
struct Elem<float> {
  static constexpr int kSize = 4;
  static constexpr int kPerChunk = 4;
  static constexpr int kStepsPerChunk = 4;
};

__device__ __forceinline__ f32x16 mfma_chunk(bf16_t, u32x4 a, u32x4 b, f32x16 acc) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a),
                                                 __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_chunk(f16_t, u32x4 a, u32x4 b, f32x16 acc) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a),
                                                __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_chunk(float, u32x4 a, u32x4 b, f32x16 acc) {
  f32x4 af = __builtin_bit_cast(f32x4, a);
  f32x4 bf = __builtin_bit_cast(f32x4, b);
#pragma unroll
  for (int e = 0; e < 4; ++e)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[e], bf[e], acc, 0, 0, 0);
  return acc;
}

__device__ __forceinline__ float load_bias(const bf16_t* p) {
  return __builtin_bit_cast(float, (uint32_t)p->v << 16);
}
__device__ __forceinline__ float load_bias(const f16_t* p) {
  return (float)__builtin_bit_cast(_Float16, p->v);
}
__device__ __forceinline__ float load_bias(const float* p) { return *p; }
__device__ __forceinline__ float round_to(bf16_t, float v) { return (float)(__bf16)v; }
__device__ __forceinline__ float round_to(f16_t, float v) { return (float)(_Float16)v; }
__device__ __forceinline__ float round_to(float, float v) { return v; }

// Store 16 consecutive output elements (fp32 accumulators -> T) at `dst` (16-byte aligned).
__device__ __forceinline__ void store16(bf16_t*, char* dst, const float (&v)[16]) {
  u32x4 lo, hi;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint16_t a = __builtin_bit_cast(uint16_t, (__bf16)v[2 * i]);
    uint16_t b = __builtin_bit_cast(uint16_t, (__bf16)v[2 * i + 1]);
    lo[i] = (uint32_t)a | ((uint32_t)b << 16);
    uint16_t c = __builtin_bit_cast(uint16_t, (__bf16)v[8 + 2 * i]);
    uint16_t d = __builtin_bit_cast(uint16_t, (__bf16)v[8 + 2 * i + 1]);
    hi[i] = (uint32_t)c | ((uint32_t)d << 16);
  }
  reinterpret_cast<u32x4*>(dst)[0] = lo;
  reinterpret_cast<u32x4*>(dst)[1] = hi;
}
__device__ __forceinline__ void store16(f16_t*, char* dst, const float (&v)[16]) {
  u32x4 lo, hi;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint16_t a = __builtin_bit_cast(uint16_t, (_Float16)v[2 * i]);
    uint16_t b = __builtin_bit_cast(uint16_t, (_Float16)v[2 * i + 1]);
    lo[i] = (uint32_t)a | ((uint32_t)b << 16);
    uint16_t c = __builtin_bit_cast(uint16_t, (_Float16)v[8 + 2 * i]);
    uint16_t d = __builtin_bit_cast(uint16_t, (_Float16)v[8 + 2 * i + 1]);
    hi[i] = (uint32_t)c | ((uint32_t)d << 16);
  }
  reinterpret_cast<u32x4*>(dst)[0] = lo;
  reinterpret_cast<u32x4*>(dst)[1] = hi;
}
__device__ __forceinline__ void store16(float*, char* dst, const float (&v)[16]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f32x4 q = {v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]};
    reinterpret_cast<f32x4*>(dst)[i] = q;
  }
}

// One 16-byte chunk of T from fp32 values: pack8 = 8 values of a 16-bit type, pack_chunk = 8 of those or 4 fp32.
__device__ __forceinline__ u32x4 pack8(bf16_t, const float* v) {
  u32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint16_t a = __builtin_bit_cast(uint16_t, (__bf16)v[2 * i]);
    uint16_t b = __builtin_bit_cast(uint16_t, (__bf16)v[2 * i + 1]);
    o[i] = (uint32_t)a | ((uint32_t)b << 16);
  }
  return o;
}
__device__ __forceinline__ u32x4 pack8(f16_t, const float* v) {
  u32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint16_t a = __builtin_bit_cast(uint16_t, (_Float16)v[2 * i]);
    uint16_t b = __builtin_bit_cast(uint16_t, (_Float16)v[2 * i + 1]);
    o[i] = (uint32_t)a | ((uint32_t)b << 16);
  }
  return o;
}

__device__ __forceinline__ u32x4 pack_chunk(bf16_t t, const float* v) { return pack8(t, v); }
__device__ __forceinline__ u32x4 pack_chunk(f16_t t, const float* v) { return pack8(t, v); }
__device__ __forceinline__ u32x4 pack_chunk(float, const float* v) {
  u32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = __builtin_bit_cast(uint32_t, v[i]);
  return o;
}

// Split-bf16 helpers (fp32 K = M-chunk = 128 kernels).  split2(a, b): round-to-nearest-even bf16 pair of
// (a, b) packed {a low, b high} (v_cvt_pk_bf16_f32), and the exact fp32 residuals a - bf16(a), b - bf16(b).
typedef __bf16 bf16x2_hw __attribute__((ext_vector_type(2)));
typedef float f32x2_hw __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t split2(float& a, float& b) {
  const f32x2_hw v = {a, b};
  const uint32_t p = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_hw));
  a -= __builtin_bit_cast(float, p << 16);
  b -= __builtin_bit_cast(float, p & 0xffff0000u);
  return p;
}

// ---- alignment classes of the general-shape kernel (matmul_gen.h) ---------------------------------
__host__ __device__ inline int gen_log2_align(uint64_t v) {
  // log2 of the largest power of two <= 16 dividing v (v == 0: 16)
  if ((v & 15) == 0) return 4;
  if ((v & 7) == 0) return 3;
  if ((v & 3) == 0) return 2;
  if ((v & 1) == 0) return 1;
  return 0;
}

// Alignment classes of one group, packed into DevGroup::pad: log2 of the vector bytes of the X, W and out accesses.
__host__ __device__ inline int gen_class(const void* a, const void* w, const void* c, int64_t K, int64_t M, int elt,
                                         int trans) {
  auto mn = [](int x, int y) { return x < y ? x : y; };
  const int lx = mn(gen_log2_align((uint64_t)a), gen_log2_align((uint64_t)(K * elt)));
  const int lw = mn(gen_log2_align((uint64_t)w), gen_log2_align((uint64_t)((trans ? K : M) * elt)));
  const int lc = mn(gen_log2_align((uint64_t)c), gen_log2_align((uint64_t)(M * elt)));
  return lx | (lw << 3) | (lc << 6);
}

// Grid of a persistent tile-walking kernel: one workgroup per tile, at most `per_cu` per compute unit.  With `ncol` > 1
// column-chunk workgroups per tile range the ranges come in whole octets (workgroup ids 8 apart = same XCD, see the
// kernels' decode) and the chip's resident workgroup count is kept.
inline unsigned tile_grid(int64_t tiles_upper, int per_cu, int ncol = 1) {
  const int64_t resident = (int64_t)device_info().num_cus * per_cu;
  int64_t gx = std::min<int64_t>(std::max<int64_t>(tiles_upper, 1), resident);
  if (ncol > 1) gx = std::max<int64_t>(8, (std::min<int64_t>(gx, resident / ncol) + 7) / 8 * 8);
  return (unsigned)(gx * ncol);
}

// A `ptr` that lives on the host (the reference's preferred placement): validated -- B + 1 non-decreasing boundaries
// within [0, N] --, then shipped to `ptr_dev` through the pinned stage.  `op` names the entry point in the message.
inline int stage_host_ptr(const char* op, const int64_t* ptr, int64_t B, int64_t N, int64_t* ptr_dev, hipStream_t stream) {
  for (int64_t b = 0; b < B; ++b)
    PYG_HIP_REQUIRE(ptr[b + 1] >= ptr[b] && ptr[b] >= 0 && ptr[b + 1] <= N, "%s: 'ptr' must be non-decreasing within [0, %lld]",
                    op, (long long)N);
  const size_t bytes = sizeof(int64_t) * (size_t)(B + 1);
  void* staged = nullptr;
  int rc = pinned_stage().acquire(bytes, &staged);
  if (rc != PYG_HIP_OK) return rc;
  ::memcpy(staged, ptr, bytes);
  PYG_HIP_CHECK(hipMemcpyAsync(ptr_dev, staged, bytes, hipMemcpyHostToDevice, stream));
  return pinned_stage().commit(stream);
}

}  // namespace

// The launch functions below take the device descriptors, the tile prefix their kernel walks (`tile_start`: 128-row
// tiles, `tile_start2`: 256-row, `tile_start3`: 64-row), the number of groups, an upper bound of the tile count and the
// stream; each owns its kernel's LDS size, block size and grid.  `dtype` is PYG_F32 / PYG_BF16 / PYG_F16.
// matmul_lds.hip: W^T in LDS, one contiguous tile range per workgroup, M / MC column chunks; the (K, MC) pairs of its
// instantiation list, anything else is PYG_HIP_ERR_INVALID.  launch_lds_f32x3: fp32 K = 128, MC = 128 in split-bf16.
int launch_lds(int dtype, int K, int MC, const void* descs, const int32_t* tile_start, int B, int64_t tiles_upper, int M,
               hipStream_t stream);
int launch_lds_f32x3(const void* descs, const int32_t* tile_start, int B, int64_t tiles_upper, int M, hipStream_t stream);
// matmul_f32_pipe.hip: fp32 K = 128, MC = 32 / 64 / 128, epilogue overlapped with the next tile's MFMAs.
int launch_f32_pipe(int MC, const void* descs, const int32_t* tile_start, int B, int64_t tiles_upper, int M,
                    hipStream_t stream);
// matmul_k128.hip: 16-bit K = M = 128.  `tickets`: kTicketWords zeroed counters.
int launch_k128_cyc(int dtype, const void* descs, const int32_t* tile_start2, int B, int64_t tiles2_upper, hipStream_t stream);
int launch_k128_ticket(int dtype, const void* descs, const int32_t* tile_start3, int B, int64_t tiles3_upper,
                       unsigned int* tickets, hipStream_t stream);
// matmul_k256.hip: 16-bit K = 256, 256 columns per workgroup (M % 256 == 0; the 64-rows-per-wave form: M == 256).
int launch_k256_wide(int dtype, const void* descs, const int32_t* tile_start, int B, int64_t tiles_upper, int M,
                     hipStream_t stream);
int launch_k256_wide_r2(int dtype, const void* descs, const int32_t* tile_start2, int B, int64_t tiles2_upper,
                        hipStream_t stream);
// matmul_gen.hip: the general-shape MFMA kernel (per-group K, M and alignment class).  `dtype` is PYG_F32 / PYG_BF16 /
// PYG_F16; `tile_start` the prefix of 128-row tiles per group, `mean_k` the row-weighted mean contraction length.
int launch_matmul_gen(int dtype, const void* descs, const int32_t* tile_start, int B, int64_t tiles_upper, int64_t mean_k,
                      hipStream_t stream);
// matmul_ring.hip: the item-ring kernels.  `tile_start3` is the prefix of 64-row tiles per group, `tiles3_upper` an upper
// bound of their number; `dtype` PYG_BF16 / PYG_F16.
int launch_ring_k256(int dtype, const void* descs, const int32_t* tile_start3, int B, int64_t tiles3_upper, hipStream_t stream);
int launch_ring_k128(int dtype, const void* descs, const int32_t* tile_start3, int B, int64_t tiles3_upper, hipStream_t stream);
int launch_ring_f32x3(const void* descs, const int32_t* tile_start3, int B, int64_t tiles3_upper, hipStream_t stream);
// matmul_dw_gen.hip: the general-shape weight gradient (per-group K, M, alignment class; bf16 / f16 / f32).  `descs`:
// DwGenGroup[B] cut for blocks of kDwGenKB x dw_gen_mb(element size); `gx` main workgroups, each with two fp32 slabs of one
// block in `slabs`; `lg`: alignment class of the launch = the smallest over its groups' operands (log2 of the vector bytes).
int launch_dw_gen(int dtype, const void* descs, const int32_t* tile_start, int B, int64_t gx, float* slabs, void* out, int lg,
                  hipStream_t stream);

}  // namespace pyg_hip
