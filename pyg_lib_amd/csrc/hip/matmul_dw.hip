// Weight gradient of segment_matmul for gfx950 (MI355X):  dW[b] = X_b^T @ dY_b  for every relation b.
//
// Replaces the reference's B-iteration backward (pyg_lib/csrc/ops/autograd/matmul_kernel.cpp:92-107:
// one at::matmul per relation + at::stack) with one persistent launch.  HBM-bound
// like the forward: X and dY are read exactly once (2 N F s bytes), the B small K x M results are
// accumulated in fp32.
//
//   * Same tiling as the forward: 128-row tiles that never cross a relation, every workgroup walks a
//     contiguous tile range, so it meets ~1.3 relations and flushes its accumulators only then.
//   * Each of the 4 waves owns 32 rows of a tile and a FULL K x MC fp32 accumulator block in
//     registers ((K/32) x (MC/32) MFMA blocks x 16 = 256 accumulators; 1 wave / SIMD): the waves never
//     exchange data and there is no workgroup barrier in the loop.
//   * The contraction runs over ROWS, so both MFMA operands are "8 rows of one column" -- transposed
//     with respect to the row-major tensors.  Rows are loaded with fully coalesced 1 KiB wave
//     accesses, parked in a wave-private row-major LDS image, and read back through gfx950's LDS
//     transpose read (ds_read_b64_tr_b16: every 16-lane group turns a 4 x 16 block into per-lane
//     4-row columns): 2 reads per MFMA operand instead of 8 two-byte reads.  The image pitch is
//     16 (mod 64) dwords, which keeps the two 16-lane groups of a 32-lane service group and the 4 rows
//     of a block on disjoint banks.
//   * No atomics (matmul_dw_out.h): when a relation ends the four waves add their accumulator sets through LDS in a
//     fixed order; a relation that lies inside the workgroup's range is rounded and stored at once, the (at most two)
//     partial ones per workgroup go to fp32 slabs that a small fix-up launch adds in workgroup order.  dW is the same
//     bits in every run, like the reference's per-relation at::matmul.
//
// This file is also the dispatch of the weight gradient, as matmul.hip is for the forward: behind the kernels follow the plan
// (dw_describe / dw_plan_kernel: ptr or host groups -> descriptors + tile prefix), the route (choose_dw_route: the table
// of pyg_hip_matmul_dw_route in pyg_hip.h, the one place that decides which kernel a (dtype, K, M, alignment) runs), what
// follows from a route (grid, slab size, workspace layout: carve_dw), run_dw_route and the C entry points.  The
// general-shape kernel lives in matmul_dw_gen.hip behind launch_dw_gen (matmul_common.h).
#include "matmul_dw_out.h"

#include <stdint.h>

#include <algorithm>
#include <atomic>

namespace pyg_hip {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short v4i16 __attribute__((ext_vector_type(4)));
typedef short v8i16 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 128;  // rows per workgroup tile (4 waves x 32)

struct bf16_tag {};
struct f16_tag {};
template <typename Tag>
struct OutOf;
template <>
struct OutOf<bf16_tag> {
  using type = bf16_t;
};
template <>
struct OutOf<f16_tag> {
  using type = f16_t;
};

__device__ __forceinline__ f32x16 mfma16(bf16_tag, v8i16 a, v8i16 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma16(f16_tag, v8i16 a, v8i16 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// pitch (bytes) of a row-major [32][cols] 16-bit LDS image: >= the row, == 16 (mod 64) dwords
constexpr int pitch_bytes(int cols) {
  const int dw = cols / 2;
  const int extra = dw > 16 ? (dw - 16 + 63) / 64 : 0;
  return (16 + 64 * extra) * 4;
}

// global_* loads (the descriptors hold generic pointers: through them the compiler emits flat_* accesses, which also count
// on lgkmcnt -- every LDS wait then waits for the rows in flight as well)
typedef const __attribute__((address_space(1))) u32x4 GU32x4;

template <typename Tag, int K, int MC>
__global__ __launch_bounds__(256, 1) void seg_dw_kernel(const DwGroup* __restrict__ groups,
                                                         const int32_t* __restrict__ tile_start, int B, int M,
                                                         float* __restrict__ slabs,
                                                         typename OutOf<Tag>::type* __restrict__ out) {
  constexpr int IB = K / 32, JB = MC / 32;
  constexpr int PX = pitch_bytes(K), PY = pitch_bytes(MC);
  constexpr int CX = K / 8, CY = MC / 8;          // 16-byte chunks per row
  constexpr int NX = 32 * CX / 64, NY = 32 * CY / 64;  // chunk loads per lane and tile
  static_assert(IB * JB <= 16, "accumulators must fit the register file");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int swave = __builtin_amdgcn_readfirstlane(wave);
  char* xs = smem + wave * 32 * (PX + PY);
  char* ys = xs + 32 * PX;
  // XCD-aware decode of the 1-D grid: the M / MC column-chunk workgroups of one tile range get ids 8 apart
  // (same XCD, same L2), so the X rows they all read come from HBM once
  const int ncol = M / MC;
  const int bx = ncol > 1 ? ((int)blockIdx.x / (8 * ncol)) * 8 + ((int)blockIdx.x & 7) : (int)blockIdx.x;
  const int by = ncol > 1 ? ((int)blockIdx.x / 8) % ncol : 0;
  const int col0 = by * MC;

  const int total = tile_start[B];
  const int G = (int)gridDim.x / ncol;
  const int t_beg = (int)((int64_t)bx * total / G);
  const int t_end = (int)((int64_t)(bx + 1) * total / G);
  if (t_beg >= t_end) return;
  int g = 0;
  {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (tile_start[mid] <= t_beg) lo = mid; else hi = mid;
    }
    g = lo;
  }

  f32x16 acc[IB][JB];
#pragma unroll
  for (int i = 0; i < IB; ++i)
#pragma unroll
    for (int j = 0; j < JB; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  int acc_g = -1;  // relation the accumulators belong to

  // a relation ends: waves combined through LDS (the images are dead: every wave is past the MFMAs of the previous tile),
  // then stored (whole relation inside [t_beg, t_end)) or parked in the head / tail slab (matmul_dw_out.h)
  auto flush = [&]() {
    if (acc_g < 0) return;
    using Pos = DwPosRows<IB, JB>;
    const int u0 = tile_start[acc_g], u1 = tile_start[acc_g + 1];
    const bool head = u0 < t_beg, tail = !head && u1 > t_end;
    float* slab = dw_slab(slabs, (int64_t)IB * JB * kDwBlockFloats, ncol, bx, by, head ? 0 : 1);
    typename OutOf<Tag>::type* base = out + ((int64_t)acc_g * K) * M + col0;
    dw_combine_waves<IB, JB>(acc, smem, swave, lane, [&](int bt, int q, dwf4 s) __attribute__((always_inline)) {
      if (head || tail) dw_quarter_to_slab(slab, bt, q, s, lane);
      else dw_quarter_to_out<Pos>(base, M, K, MC, bt, q, s, lane);
    });
#pragma unroll
    for (int i = 0; i < IB; ++i)
#pragma unroll
      for (int j = 0; j < JB; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  };

  // software pipeline: rows of tile t+1 travel to registers while tile t is multiplied
  u32x4 xr[NX], yr[NY];
  int n_g = g;
  DwGroup gd = groups[g];
  auto prefetch = [&](int t) {
    while (t >= tile_start[n_g + 1]) {
      ++n_g;
      gd = groups[n_g];
    }
    const int64_t row0 = (int64_t)(t - tile_start[n_g]) * kTile + wave * 32;
#pragma unroll
    for (int it = 0; it < NX; ++it) {
      const int p = it * 64 + lane;
      const int64_t row = row0 + p / CX;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (row < gd.rows) v = *(GU32x4*)(gd.x + row * K + (p % CX) * 8);
      xr[it] = v;
    }
#pragma unroll
    for (int it = 0; it < NY; ++it) {
      const int p = it * 64 + lane;
      const int64_t row = row0 + p / CY;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (row < gd.rows) v = *(GU32x4*)(gd.dy + row * M + col0 + (p % CY) * 8);
      yr[it] = v;
    }
  };

  // lane constants of the transpose reads: lane q of a 16-lane group supplies row (q >> 2), columns
  // (q & 3) * 4 of a 4 x 16 block and receives column q; group = (column half, row half kb)
  const int q = lane & 15, half = (lane >> 4) & 1, kb = lane >> 5;
  const int a_off = (kb * 8 + (q >> 2)) * PX + (half * 16 + (q & 3) * 4) * 2;
  const int b_off = (kb * 8 + (q >> 2)) * PY + (half * 16 + (q & 3) * 4) * 2;
  typedef __attribute__((address_space(3))) v4i16* lds_v4;

  prefetch(t_beg);
  for (int t = t_beg; t < t_end; ++t) {
    const int cur_g = n_g;  // relation of the tile held in xr / yr
    if (cur_g != acc_g) {
      flush();
      acc_g = cur_g;
    }
    // park the tile in the wave-private LDS image (row-major)
#pragma unroll
    for (int it = 0; it < NX; ++it) {
      const int p = it * 64 + lane;
      *reinterpret_cast<u32x4*>(xs + (p / CX) * PX + (p % CX) * 16) = xr[it];
    }
#pragma unroll
    for (int it = 0; it < NY; ++it) {
      const int p = it * 64 + lane;
      *reinterpret_cast<u32x4*>(ys + (p / CY) * PY + (p % CY) * 16) = yr[it];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (t + 1 < t_end) prefetch(t + 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      v8i16 af[IB], bf[JB];
#pragma unroll
      for (int i = 0; i < IB; ++i) {
        const char* p = xs + a_off + ks * 16 * PX + i * 64;
        const v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(p));
        const v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(p + 4 * PX));
        af[i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int j = 0; j < JB; ++j) {
        const char* p = ys + b_off + ks * 16 * PY + j * 64;
        const v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(p));
        const v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(p + 4 * PY));
        bf[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int i = 0; i < IB; ++i)
#pragma unroll
        for (int j = 0; j < JB; ++j) acc[i][j] = mfma16(Tag{}, af[i], bf[j], acc[i][j]);
    }
    __builtin_amdgcn_wave_barrier();
  }
  flush();
}

// K = 256, 256 output columns per workgroup: the four waves SHARE every 32-row slab of X and dY and split the
// COLUMNS of dW instead of the rows (wave w owns dW[:, 64 w .. 64 w + 63]: 8 x 2 accumulator blocks, the same
// 256 registers as above).  With row-split waves a 256-wide dW needs four column-chunk workgroups that each
// stream the whole X again (C4: 4.6 ms); here X and dY pass through one CU once.  The slab lives in a
// workgroup-shared, double-buffered row-major LDS image (same pitch rule, same transpose reads); every wave
// loads a quarter of the next slab while the current one is multiplied, one barrier per slab:
//   iteration s:  registers (slab s+1) -> image[(s+1) & 1];  issue loads of slab s+2;  MFMAs on image[s & 1];  barrier.
template <typename Tag>
__global__ __launch_bounds__(256, 1) void seg_dw_wide256_kernel(const DwGroup* __restrict__ groups,
                                                                const int32_t* __restrict__ tile_start, int B, int M,
                                                                float* __restrict__ slabs,
                                                                typename OutOf<Tag>::type* __restrict__ out) {
  constexpr int K = 256, MC = 256, IB = K / 32, JB = 2;
  constexpr int PX = pitch_bytes(K), PY = pitch_bytes(MC);
  constexpr int CX = K / 8, CY = MC / 8;                 // 16-byte chunks per row
  constexpr int NX = 32 * CX / 256, NY = 32 * CY / 256;  // chunk loads per THREAD and slab
  constexpr int IMG = 32 * (PX + PY);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int swave = __builtin_amdgcn_readfirstlane(wave);
  const int ncol = M / MC;
  const int bx = ncol > 1 ? ((int)blockIdx.x / (8 * ncol)) * 8 + ((int)blockIdx.x & 7) : (int)blockIdx.x;
  const int by = ncol > 1 ? ((int)blockIdx.x / 8) % ncol : 0;
  const int col0 = by * MC;

  const int total = tile_start[B];
  const int G = (int)gridDim.x / ncol;
  const int t_beg = (int)((int64_t)bx * total / G);
  const int t_end = (int)((int64_t)(bx + 1) * total / G);
  if (t_beg >= t_end) return;
  int g = 0;
  {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (tile_start[mid] <= t_beg) lo = mid; else hi = mid;
    }
    g = lo;
  }

  f32x16 acc[IB][JB];
#pragma unroll
  for (int i = 0; i < IB; ++i)
#pragma unroll
    for (int j = 0; j < JB; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  int acc_g = -1;
  // the waves own disjoint COLUMNS of dW: nothing to combine; whole relation -> dW, partial -> this wave's part of the slab
  auto flush = [&]() {
    if (acc_g < 0) return;
    const int u0 = tile_start[acc_g], u1 = tile_start[acc_g + 1];
    const bool head = u0 < t_beg, tail = !head && u1 > t_end;
    float* slab = dw_slab(slabs, (int64_t)DwPosWide::kBlocks * kDwBlockFloats, ncol, bx, by, head ? 0 : 1);
    typename OutOf<Tag>::type* base = out + ((int64_t)acc_g * K) * M + col0;
    // Through a wave-private 16 KiB staging area behind the two images (both hold live slabs here), four blocks at a
    // time: the registers are written with constant indices, the stores walk the area in a ROLLED loop -- the direct
    // form (64 blocks x 4 quarters of address arithmetic next to 256 live accumulators) spilled 2 KB per lane.
    char* stage = smem + 2 * IMG + wave * 16384 + lane * 16;
#pragma unroll
    for (int Q = 0; Q < 4; ++Q) {
#pragma unroll
      for (int L = 0; L < 4; ++L) {
        const int b = Q * 4 + L;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const dwf4 v = {acc[b / JB][b % JB][4 * q], acc[b / JB][b % JB][4 * q + 1], acc[b / JB][b % JB][4 * q + 2],
                          acc[b / JB][b % JB][4 * q + 3]};
          *reinterpret_cast<dwf4*>(stage + (L * 4 + q) * 1024) = v;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll 1
      for (int it = 0; it < 16; ++it) {
        const dwf4 v = *reinterpret_cast<const dwf4*>(stage + it * 1024);
        const int bt = swave * 16 + Q * 4 + (it >> 2), q = it & 3;
        if (head || tail) dw_quarter_to_slab(slab, bt, q, v, lane);
        else dw_quarter_to_out<DwPosWide>(base, M, K, MC, bt, q, v, lane);
      }
      __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int i = 0; i < IB; ++i)
#pragma unroll
      for (int j = 0; j < JB; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  };

  // slab index space: 4 slabs of 32 rows per 128-row tile
  const int s_beg = t_beg * 4, s_end = t_end * 4;
  u32x4 xr[NX], yr[NY];
  int n_g = g;
  DwGroup gd = groups[g];
  auto prefetch = [&](int sl) {  // this thread's share of slab sl (group n_g after the call)
    const int t = sl >> 2;
    while (t >= tile_start[n_g + 1]) {
      ++n_g;
      gd = groups[n_g];
    }
    const int64_t row0 = (int64_t)(t - tile_start[n_g]) * kTile + (sl & 3) * 32;
#pragma unroll
    for (int it = 0; it < NX; ++it) {
      const int p = it * 256 + tid;
      const int64_t row = row0 + p / CX;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (row < gd.rows) v = *(GU32x4*)(gd.x + row * K + (p % CX) * 8);
      xr[it] = v;
    }
#pragma unroll
    for (int it = 0; it < NY; ++it) {
      const int p = it * 256 + tid;
      const int64_t row = row0 + p / CY;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (row < gd.rows) v = *(GU32x4*)(gd.dy + row * M + col0 + (p % CY) * 8);
      yr[it] = v;
    }
  };
  auto park = [&](int buf) {
    char* xs = smem + buf * IMG;
    char* ys = xs + 32 * PX;
#pragma unroll
    for (int it = 0; it < NX; ++it) {
      const int p = it * 256 + tid;
      *reinterpret_cast<u32x4*>(xs + (p / CX) * PX + (p % CX) * 16) = xr[it];
    }
#pragma unroll
    for (int it = 0; it < NY; ++it) {
      const int p = it * 256 + tid;
      *reinterpret_cast<u32x4*>(ys + (p / CY) * PY + (p % CY) * 16) = yr[it];
    }
  };

  const int q = lane & 15, half = (lane >> 4) & 1, kb = lane >> 5;
  const int a_off = (kb * 8 + (q >> 2)) * PX + (half * 16 + (q & 3) * 4) * 2;
  const int b_off = (kb * 8 + (q >> 2)) * PY + (half * 16 + (q & 3) * 4) * 2 + wave * 128;  // this wave's 64 columns
  typedef __attribute__((address_space(3))) v4i16* lds_v4;

  // group of the slab held in the registers / of each image
  prefetch(s_beg);
  int g_img[2];
  g_img[0] = n_g;
  park(0);
  g_img[1] = n_g;
  if (s_beg + 1 < s_end) prefetch(s_beg + 1);
  int g_regs = n_g;
  __syncthreads();

  for (int sl = s_beg; sl < s_end; ++sl) {
    const int cur = (sl - s_beg) & 1;
    if (sl + 1 < s_end) {
      park(cur ^ 1);  // slab sl + 1 (in registers since the previous iteration)
      g_img[cur ^ 1] = g_regs;
      if (sl + 2 < s_end) {
        prefetch(sl + 2);
        g_regs = n_g;
      }
    }
    const int cur_g = g_img[cur];
    if (cur_g != acc_g) {
      flush();
      acc_g = cur_g;
    }
    const char* xs = smem + cur * IMG;
    const char* ys = xs + 32 * PX;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      v8i16 af[IB], bf[JB];
#pragma unroll
      for (int i = 0; i < IB; ++i) {
        const char* p = xs + a_off + ks * 16 * PX + i * 64;
        const v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(p));
        const v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(p + 4 * PX));
        af[i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int j = 0; j < JB; ++j) {
        const char* p = ys + b_off + ks * 16 * PY + j * 64;
        const v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(p));
        const v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(p + 4 * PY));
        bf[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int i = 0; i < IB; ++i)
#pragma unroll
        for (int j = 0; j < JB; ++j) acc[i][j] = mfma16(Tag{}, af[i], bf[j], acc[i][j]);
    }
    __syncthreads();
  }
  flush();
}

// fp32: v_mfma_f32_32x32x2_f32 takes ONE value per lane (lane (i, kk) = A[i][kk]), so the "column of
// rows" operand is simply a row-major load -- lane (i, kk) reads X[row 2s + kk][col i]: two coalesced
// 128-byte segments per wave instruction, no LDS and no transposition.  Exact fp32 FMA chains (gfx950 has
// no TF32); bound by the fp32 MFMA rate (157 TFLOP/s: C2 >= 4.4 ms), not by HBM.
template <int K, int MC>
__global__ __launch_bounds__(256, 1) void seg_dw_f32_kernel(const DwGroup* __restrict__ groups,
                                                             const int32_t* __restrict__ tile_start, int B, int M,
                                                             float* __restrict__ slabs, float* __restrict__ out) {
  constexpr int IB = K / 32, JB = MC / 32;
  static_assert(IB * JB <= 16, "accumulators must fit the register file");
  // The MFMA wants ONE value per lane and block, but nothing ties block i to the columns 32 i .. 32 i + 31:
  // lane li loads VA (up to 4) CONSECUTIVE floats of its row in one instruction and feeds them to VA
  // different blocks (block VA h + e = columns 32 VA h + VA li + e) -- 16-byte instead of 4-byte accesses,
  // whole 512-byte rows per wave instruction; the permutation is undone when the accumulators are flushed.
  constexpr int VA = IB >= 4 ? 4 : IB, VB = JB >= 4 ? 4 : JB;
  extern __shared__ __attribute__((aligned(16))) char smem[];  // IB * JB * 4 KiB: the waves' combine area (flush only)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int swave = __builtin_amdgcn_readfirstlane(wave);
  const int li = lane & 31, kk = lane >> 5;
  const int ncol = M / MC;
  const int bx = ncol > 1 ? ((int)blockIdx.x / (8 * ncol)) * 8 + ((int)blockIdx.x & 7) : (int)blockIdx.x;
  const int by = ncol > 1 ? ((int)blockIdx.x / 8) % ncol : 0;
  const int col0 = by * MC;
  const int total = tile_start[B];
  const int G = (int)gridDim.x / ncol;
  const int t_beg = (int)((int64_t)bx * total / G);
  const int t_end = (int)((int64_t)(bx + 1) * total / G);
  if (t_beg >= t_end) return;
  int g = 0;
  {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (tile_start[mid] <= t_beg) lo = mid; else hi = mid;
    }
    g = lo;
  }
  f32x16 acc[IB][JB];
#pragma unroll
  for (int i = 0; i < IB; ++i)
#pragma unroll
    for (int j = 0; j < JB; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  int acc_g = -1;
  // block i = VA h + e holds the X columns 32 VA h + VA * (MFMA row) + e (see the loads below): DwPosF32 undoes that
  auto flush = [&]() {
    if (acc_g < 0) return;
    using Pos = DwPosF32<IB, JB>;
    const int u0 = tile_start[acc_g], u1 = tile_start[acc_g + 1];
    const bool head = u0 < t_beg, tail = !head && u1 > t_end;
    float* slab = dw_slab(slabs, (int64_t)IB * JB * kDwBlockFloats, ncol, bx, by, head ? 0 : 1);
    float* base = out + ((int64_t)acc_g * K) * M + col0;
    dw_combine_waves<IB, JB>(acc, smem, swave, lane, [&](int bt, int q, dwf4 s) __attribute__((always_inline)) {
      if (head || tail) dw_quarter_to_slab(slab, bt, q, s, lane);
      else dw_quarter_to_out<Pos>(base, M, K, MC, bt, q, s, lane);
    });
#pragma unroll
    for (int i = 0; i < IB; ++i)
#pragma unroll
      for (int j = 0; j < JB; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  };
  // Software pipeline over the flattened (tile, row pair) sequence: the operands of step it + D are requested
  // while step it is multiplied (one wave per SIMD and 16 MFMAs = 1 k cycles per step: without the ring an HBM
  // round trip of ~5 k cycles is exposed every few steps).  D slots of (a, b, group) with static indices.
  constexpr int D = 8;
  const int n_it = (t_end - t_beg) * 16;
  float pa[D][IB], pb[D][JB];
  int pg[D];
  int lg = g;  // group walk of the load side
  DwGroup ld = groups[lg];
  auto request = [&](int it, float (&a)[IB], float (&b)[JB], int& grp) {
    const int t = t_beg + (it >> 4);
    while (t >= tile_start[lg + 1]) {
      ++lg;
      ld = groups[lg];
    }
    grp = lg;
    const float* xp = reinterpret_cast<const float*>(ld.x);
    const float* yp = reinterpret_cast<const float*>(ld.dy);
    const int64_t row = (int64_t)(t - tile_start[lg]) * kTile + wave * 32 + 2 * (it & 15) + kk;
    const bool ok = row < ld.rows;
#pragma unroll
    for (int h = 0; h < IB / VA; ++h) {
      typedef float vecA __attribute__((ext_vector_type(VA)));
      vecA v;
#pragma unroll
      for (int e = 0; e < VA; ++e) v[e] = 0.0f;
      if (ok) v = *(const __attribute__((address_space(1))) vecA*)(xp + row * K + 32 * VA * h + VA * li);
#pragma unroll
      for (int e = 0; e < VA; ++e) a[VA * h + e] = v[e];
    }
#pragma unroll
    for (int h = 0; h < JB / VB; ++h) {
      typedef float vecB __attribute__((ext_vector_type(VB)));
      vecB v;
#pragma unroll
      for (int e = 0; e < VB; ++e) v[e] = 0.0f;
      if (ok) v = *(const __attribute__((address_space(1))) vecB*)(yp + row * M + col0 + 32 * VB * h + VB * li);
#pragma unroll
      for (int e = 0; e < VB; ++e) b[VB * h + e] = v[e];
    }
  };
#pragma unroll
  for (int k = 0; k < D; ++k) request(k, pa[k], pb[k], pg[k]);  // n_it is a multiple of 16
  // D divides the 16 steps of a tile and tiles never cross a relation: a chunk of D steps has ONE relation
  static_assert(16 % D == 0, "a chunk of D steps must stay inside one tile");
  for (int it0 = 0; it0 < n_it; it0 += D) {
    if (pg[0] != acc_g) {
      flush();
      acc_g = pg[0];
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
#pragma unroll
      for (int i = 0; i < IB; ++i)
#pragma unroll
        for (int j = 0; j < JB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[k][i], pb[k][j], acc[i][j], 0, 0, 0);
      if (it0 + k + D < n_it) request(it0 + k + D, pa[k], pb[k], pg[k]);
    }
  }
  flush();
}

// The launch behind the main kernel.  Workgroups [0, fix_blocks): wave v = 4 blockIdx + wave is (logical main workgroup
// m = v / (4 NBT), slab block bt, quarter q); if a split relation STARTS in m's tile range, the wave adds that relation's
// slabs in workgroup order (dw_chain_sum) and stores 4 x 64 rounded values.  Workgroups behind them: relation
// blockIdx - fix_blocks; one without rows gets its zeros here (nothing else ever writes it).
template <typename Pos, typename OutT>
__global__ __launch_bounds__(256) void seg_dw_fixup_kernel(const int32_t* __restrict__ tile_start, int B, int K, int M, int MC,
                                                          int G, int fix_blocks, const float* __restrict__ slabs,
                                                          OutT* __restrict__ out) {
  constexpr int NBT = Pos::kBlocks;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if ((int)blockIdx.x >= fix_blocks) {
    const int g = (int)blockIdx.x - fix_blocks;
    if (tile_start[g + 1] != tile_start[g]) return;
    OutT* base = out + (int64_t)g * K * M;
    for (int i = threadIdx.x; i < K * M; i += 256) dw_put(base + i, 0.0f);
    return;
  }
  const int ncol = M / MC;
  const int v = (int)blockIdx.x * 4 + wave;
  const int m = v / (4 * NBT), piece = v - m * (4 * NBT);
  const int bt = piece >> 2, q = piece & 3;
  const int bx = m / ncol, by = m - bx * ncol;
  const int total = tile_start[B];
  const int t_beg = (int)((int64_t)bx * total / G), t_end = (int)((int64_t)(bx + 1) * total / G);
  if (t_beg >= t_end) return;
  int lo = 0, hi = B;  // relation of the range's last tile
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile_start[mid] <= t_end - 1) lo = mid; else hi = mid;
  }
  const int u0 = tile_start[lo], u1 = tile_start[lo + 1];
  if (!(u1 > t_end && u0 >= t_beg)) return;  // no split relation starts here
  const dwf4 s = dw_chain_sum(slabs, (int64_t)NBT * kDwBlockFloats, ncol, bx, by, G, total, u1, bt, q, lane);
  dw_quarter_to_out<Pos>(out + (int64_t)lo * K * M + by * MC, M, K, MC, bt, q, s, lane);
}

// ---- plan: descriptors + tile prefix ---------------------------------------------------------------
// The descriptor of one group for the kernel that will walk it.  Returns the work tiles per 128-row tile of the group: 1 for
// the shape-specialised kernels (their column chunks are workgroups, not tiles), the number of kb x mb blocks of the
// [k, m] output for the general-shape kernel.  Shared by the plan kernel (segment form) and the host loop (grouped form).
__host__ __device__ inline int64_t dw_describe(DwGroup& d, const char* x, const char* dy, int64_t rows, int64_t, int64_t, int,
                                               int64_t, int, int) {
  d.x = reinterpret_cast<const uint16_t*>(x);
  d.dy = reinterpret_cast<const uint16_t*>(dy);
  d.rows = rows;
  return 1;
}
__host__ __device__ inline int64_t dw_describe(DwGenGroup& d, const char* x, const char* dy, int64_t rows, int64_t k, int64_t m,
                                               int elt, int64_t acc_off, int kb, int mb) {
  auto mn = [](int a, int b) { return a < b ? a : b; };
  d.x = x;
  d.dy = dy;
  d.rows = rows;
  d.acc_off = acc_off;
  d.k = (int32_t)k;
  d.m = (int32_t)m;
  d.lx = (int16_t)mn(gen_log2_align((uint64_t)x), gen_log2_align((uint64_t)(k * elt)));
  d.ly = (int16_t)mn(gen_log2_align((uint64_t)dy), gen_log2_align((uint64_t)(m * elt)));
  d.nkb = (int16_t)((k + kb - 1) / kb);
  d.nmb = (int16_t)((m + mb - 1) / mb);
  return (int64_t)d.nkb * d.nmb;
}

// segment form: descriptors + tile prefix from ptr (uniform K, M; one thread per run of relations);
// tile_start[b] = sum_{b' < b} ceil(rows_b' / 128) * (work tiles per row tile)
template <typename Desc>
__global__ void dw_plan_kernel(const int64_t* __restrict__ ptr, int64_t B, const char* X, const char* dY, int64_t K, int64_t M,
                               int elt, int kb, int mb, Desc* __restrict__ groups, int32_t* __restrict__ tile_start) {
  __shared__ int64_t part[256];
  const int tid = threadIdx.x;
  const int64_t per = (B + 255) / 256;
  const int64_t beg = min((int64_t)tid * per, B), end = min(beg + per, B);
  Desc d;
  const int64_t blocks = dw_describe(d, X, dY, 0, K, M, elt, 0, kb, mb);
  int64_t t = 0;
  for (int64_t b = beg; b < end; ++b) {
    const int64_t r = ptr[b + 1] - ptr[b];
    t += r > 0 ? (r + kTile - 1) / kTile * blocks : 0;
  }
  part[tid] = t;
  __syncthreads();
  if (tid == 0) {
    int64_t acc = 0;
    for (int i = 0; i < 256; ++i) {
      const int64_t v = part[i];
      part[i] = acc;
      acc += v;
    }
    tile_start[B] = (int32_t)acc;
  }
  __syncthreads();
  t = part[tid];
  for (int64_t b = beg; b < end; ++b) {
    tile_start[b] = (int32_t)t;
    const int64_t p0 = ptr[b];
    const int64_t r = ptr[b + 1] - p0;
    dw_describe(d, X + p0 * K * elt, dY + p0 * M * elt, r > 0 ? r : 0, K, M, elt, b * K * M, kb, mb);
    groups[b] = d;
    t += r > 0 ? (r + kTile - 1) / kTile * blocks : 0;
  }
}

// ---- the route: which kernel serves a call ---------------------------------------------------------
enum class DwFamily {
  kUnsupported,  // no kernel for the dtype, or a shape beyond the general kernel's 32-bit offsets
  kInvalid,      // an operand that is not element-aligned
  kGen,          // matmul_dw_gen.hip: K x MC = its output block
  kSeg,          // seg_dw_kernel / seg_dw_f32_kernel<K, MC>
  kWide256,      // seg_dw_wide256_kernel
};
struct DwRoute {
  DwFamily family;
  int K = 0, MC = 0;  // contraction length and output columns of one accumulator set (kGen: of one block)
};

inline bool dw_dtype_ok(int dtype) { return dtype == PYG_F32 || dtype == PYG_BF16 || dtype == PYG_F16; }
inline int dw_elt(int dtype) { return dtype == PYG_F32 ? 4 : 2; }
inline DwRoute dw_gen_route(int dtype) { return {DwFamily::kGen, kDwGenKB, dw_gen_mb(dw_elt(dtype))}; }

// The route of a call: the table of pyg_hip_matmul_dw_route in pyg_hip.h.  `uniform`: all groups share (K, M); `misalign`:
// dw_misalign() of the call.  Pure: no HIP call, no global, no device property.
DwRoute choose_dw_route(int dtype, int64_t K, int64_t M, bool uniform, unsigned misalign) {
  if (!dw_dtype_ok(dtype)) return {DwFamily::kUnsupported};
  if (misalign % dw_elt(dtype) != 0) return {DwFamily::kInvalid};
  if (!uniform || misalign % 16 != 0 || !((K == 64 || K == 128 || K == 256) && M > 0 && M % 64 == 0)) {
    if (K >= (1LL << 21) || M >= (1LL << 21) || K * M >= (1LL << 28)) return {DwFamily::kUnsupported};
    return dw_gen_route(dtype);
  }
  // 16-bit K = 256: the waves split the columns of a 256-wide chunk instead of the rows (X and dY pass through one CU once)
  if (dtype != PYG_F32 && K == 256 && M % 256 == 0) return {DwFamily::kWide256, 256, 256};
  // a wave's K x MC accumulator block has to fit its 256 accumulation registers
  return {DwFamily::kSeg, (int)K, K == 256 || M % 128 != 0 ? 64 : 128};
}

// `misalign` of a call: the low four address bits of all its X and dY operands (`operands`: their addresses ORed), and of the
// output the bits below the element size -- dW is stored element by element, so it only has to be element-aligned.
inline unsigned dw_misalign(uintptr_t operands, const void* out, int elt) {
  return (unsigned)((operands & 15) | ((uintptr_t)out & (uintptr_t)(elt - 1)));
}

const char* dw_route_name(int dtype, DwRoute r) {
  thread_local char name[32];
  const char* t = dtype == PYG_BF16 ? "bf16" : dtype == PYG_F16 ? "f16" : "f32";
  switch (r.family) {
    case DwFamily::kUnsupported: return "unsupported";
    case DwFamily::kInvalid: return "invalid";
    case DwFamily::kGen: return "gen";
    case DwFamily::kSeg: snprintf(name, sizeof(name), "seg_%s_k%d_mc%d", t, r.K, r.MC); break;
    case DwFamily::kWide256: snprintf(name, sizeof(name), "wide256_%s", t); break;
  }
  return name;
}

// A route that cannot run, as the error of entry point `op` for a group of shape (K, M).
int dw_route_check(const char* op, DwRoute r, int64_t K, int64_t M) {
  if (r.family == DwFamily::kInvalid) return fail(PYG_HIP_ERR_INVALID, "%s: operands must be element-aligned", op);
  if (r.family == DwFamily::kUnsupported)
    return fail(PYG_HIP_ERR_UNSUPPORTED, "%s: K x M = %lld x %lld is beyond the kernel's 32-bit offsets", op, (long long)K,
                (long long)M);
  if (r.family == DwFamily::kGen)  // DwGenGroup::nkb, nmb
    PYG_HIP_REQUIRE((K + r.K - 1) / r.K < 32768 && (M + r.MC - 1) / r.MC < 32768, "%s: K / M too large", op);
  return PYG_HIP_OK;
}

// ---- what follows from the route: grid, slabs, workspace ------------------------------------------
// column-chunk workgroups per tile range
inline int64_t dw_ncol(DwRoute r, int64_t M) { return r.family == DwFamily::kGen ? 1 : M / r.MC; }
// tile ranges (= main workgroups / ncol) of a call with at most `tiles_upper` tiles
inline int64_t dw_grid_x(int64_t tiles_upper, int64_t ncol) {
  int64_t gx = std::max<int64_t>(1, std::min<int64_t>(tiles_upper, device_info().num_cus / ncol));
  if (ncol > 1) gx = (gx + 7) / 8 * 8;  // the kernels' XCD-aware decode works on groups of 8 ids
  return gx;
}
// two fp32 slabs of K x MC per main workgroup; the bound holds for every tile count
inline size_t dw_slab_bytes(DwRoute r, int64_t M) {
  const int64_t ncol = dw_ncol(r, M);
  return (size_t)(dw_grid_x(INT64_MAX, ncol) * ncol) * 2 * (size_t)r.K * (size_t)r.MC * sizeof(float);
}

struct DwWorkspace {
  int64_t* ptr_copy;    // B + 1 (segment form with a host `ptr`)
  void* descs;          // DwGroup / DwGenGroup [B]
  int32_t* tile_start;  // B + 1, directly behind the descriptors: the grouped form ships both in one copy
  float* slabs;
  size_t plan_bytes;    // descriptors + tile prefix
  size_t bytes;         // of the whole layout
};

// The workspace layout: `ws` (may be null: size query) cut into the arrays above; DwWorkspace::bytes = what the cut needs.
DwWorkspace carve_dw(void* ws, int64_t B, size_t desc_size, size_t slab_bytes) {
  DwWorkspace w;
  size_t off = 0;
  auto take = [&](size_t bytes, size_t align) {
    void* p = reinterpret_cast<void*>(reinterpret_cast<uintptr_t>(ws) + off);
    off += align_up(bytes, align);
    return p;
  };
  w.ptr_copy = static_cast<int64_t*>(take(sizeof(int64_t) * (size_t)(B + 1), 256));
  w.descs = take(desc_size * (size_t)std::max<int64_t>(B, 1), 256);
  w.tile_start = static_cast<int32_t*>(take(sizeof(int32_t) * (size_t)(B + 1), 256));
  w.plan_bytes = off - (size_t)(static_cast<char*>(w.descs) - static_cast<char*>(ws));
  w.slabs = static_cast<float*>(take(slab_bytes, 1));
  w.bytes = off;
  return w;
}
DwWorkspace carve_dw(void* ws, int64_t B, DwRoute r, int64_t M) {
  return carve_dw(ws, B, r.family == DwFamily::kGen ? sizeof(DwGenGroup) : sizeof(DwGroup), dw_slab_bytes(r, M));
}

// Bytes for B groups of shape (K, M): the size queries know neither dtype nor alignment, so this is the largest layout over
// the routes the shape can take.
size_t dw_workspace_bytes(int64_t B, int64_t K, int64_t M, bool uniform) {
  size_t need = 0;
  for (int dtype : {PYG_BF16, PYG_F32}) {
    need = std::max(need, carve_dw(nullptr, B, dw_gen_route(dtype), M).bytes);
    const DwRoute r = choose_dw_route(dtype, K, M, uniform, 0);
    if (r.family == DwFamily::kSeg || r.family == DwFamily::kWide256) need = std::max(need, carve_dw(nullptr, B, r, M).bytes);
  }
  return need;
}

// ---- launches -------------------------------------------------------------------------------------------
struct DwLaunch {
  const DwGroup* groups;
  const int32_t* tile_start;
  int64_t B, M;
  int64_t gx;  // tile ranges
  float* slabs;
  void* out;
  hipStream_t stream;
};

template <typename Pos, typename OutT>
int launch_fixup(const DwLaunch& a, int K, int MC, OutT* out) {
  const int64_t ncol = a.M / MC;
  const int64_t fix_blocks = a.gx * ncol * Pos::kBlocks;  // 4 NBT waves per main workgroup, 4 waves per block
  hipLaunchKernelGGL((seg_dw_fixup_kernel<Pos, OutT>), dim3((unsigned)(fix_blocks + a.B)), dim3(256), 0, a.stream, a.tile_start,
                     (int)a.B, K, (int)a.M, MC, (int)a.gx, (int)fix_blocks, a.slabs, out);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

template <typename Tag, int K, int MC>
int launch_dw(const DwLaunch& a) {
  using OutT = typename OutOf<Tag>::type;
  OutT* out = static_cast<OutT*>(a.out);
  constexpr int lds = 4 * 32 * (pitch_bytes(K) + pitch_bytes(MC));
  static_assert(lds >= (K / 32) * (MC / 32) * 4096, "the combine area must fit the row images");
  const void* kern = reinterpret_cast<const void*>(&seg_dw_kernel<Tag, K, MC>);
  if (int rc_ = ensure_dynamic_lds(kern, lds)) return rc_;
  hipLaunchKernelGGL((seg_dw_kernel<Tag, K, MC>), dim3((unsigned)(a.gx * (a.M / MC))), dim3(256), lds, a.stream, a.groups,
                     a.tile_start, (int)a.B, (int)a.M, a.slabs, out);
  PYG_HIP_CHECK(hipGetLastError());
  return launch_fixup<DwPosRows<K / 32, MC / 32>, OutT>(a, K, MC, out);
}

template <typename Tag>
int launch_dw_wide256(const DwLaunch& a) {
  using OutT = typename OutOf<Tag>::type;
  OutT* out = static_cast<OutT*>(a.out);
  constexpr int lds = 2 * 32 * (pitch_bytes(256) + pitch_bytes(256)) + 4 * 16384;  // two images + the flush staging area
  const void* kern = reinterpret_cast<const void*>(&seg_dw_wide256_kernel<Tag>);
  if (int rc_ = ensure_dynamic_lds(kern, lds)) return rc_;
  hipLaunchKernelGGL((seg_dw_wide256_kernel<Tag>), dim3((unsigned)(a.gx * (a.M / 256))), dim3(256), lds, a.stream, a.groups,
                     a.tile_start, (int)a.B, (int)a.M, a.slabs, out);
  PYG_HIP_CHECK(hipGetLastError());
  return launch_fixup<DwPosWide, OutT>(a, 256, 256, out);
}

template <int K, int MC>
int launch_dw_f32(const DwLaunch& a) {
  float* out = static_cast<float*>(a.out);
  constexpr int lds = (K / 32) * (MC / 32) * 4096;  // the waves' combine area
  const void* kern = reinterpret_cast<const void*>(&seg_dw_f32_kernel<K, MC>);
  if (int rc_ = ensure_dynamic_lds(kern, lds)) return rc_;
  hipLaunchKernelGGL((seg_dw_f32_kernel<K, MC>), dim3((unsigned)(a.gx * (a.M / MC))), dim3(256), lds, a.stream, a.groups,
                     a.tile_start, (int)a.B, (int)a.M, a.slabs, out);
  PYG_HIP_CHECK(hipGetLastError());
  return launch_fixup<DwPosF32<K / 32, MC / 32>, float>(a, K, MC, out);
}

template <int K, int MC>
int launch_seg(int dtype, const DwLaunch& a) {
  return dtype == PYG_F32 ? launch_dw_f32<K, MC>(a) : dtype == PYG_BF16 ? launch_dw<bf16_tag, K, MC>(a) : launch_dw<f16_tag, K, MC>(a);
}

// Launch the kernel of route `r` on the planned workspace.  `tiles_upper`: upper bound of the call's tiles; `lg`: alignment
// class of the call's operands (general route).
int run_dw_route(DwRoute r, int dtype, const DwWorkspace& w, int64_t B, int64_t M, int64_t tiles_upper, void* out, int lg,
                 hipStream_t stream) {
  const int64_t gx = dw_grid_x(tiles_upper, dw_ncol(r, M));
  const DwLaunch a = {static_cast<const DwGroup*>(w.descs), w.tile_start, B, M, gx, w.slabs, out, stream};
  switch (r.family) {
    case DwFamily::kGen: return launch_dw_gen(dtype, w.descs, w.tile_start, (int)B, gx, w.slabs, out, lg, stream);
    case DwFamily::kWide256: return dtype == PYG_BF16 ? launch_dw_wide256<bf16_tag>(a) : launch_dw_wide256<f16_tag>(a);
    case DwFamily::kSeg:
      if (r.K == 128 && r.MC == 128) return launch_seg<128, 128>(dtype, a);
      if (r.K == 128 && r.MC == 64) return launch_seg<128, 64>(dtype, a);
      if (r.K == 64 && r.MC == 128) return launch_seg<64, 128>(dtype, a);
      if (r.K == 64 && r.MC == 64) return launch_seg<64, 64>(dtype, a);
      if (r.K == 256 && r.MC == 64) return launch_seg<256, 64>(dtype, a);
      break;
    default: break;
  }
  return fail(PYG_HIP_ERR_INVALID, "matmul_dw: unknown route");
}

// launches served by the shape-specialised / the general-shape kernels since the library was loaded (tests assert that a
// backward pass ran a device kernel and not the caller's fallback formula; the backward runs on an autograd thread, so a
// thread-local "last route" would not be visible to the test)
std::atomic<int64_t> g_dw_fast{0}, g_dw_gen{0};
inline int dw_count(DwRoute r, int rc) {
  if (rc == PYG_HIP_OK) ++(r.family == DwFamily::kGen ? g_dw_gen : g_dw_fast);
  return rc;
}

// segment form on a checked route: plan on the device from `ptr`, then the route's kernel
template <typename Desc>
int dw_segment(DwRoute r, int dtype, const void* input, const int64_t* ptr, int ptr_on_device, const void* grad_out,
               void* grad_other, int64_t N, int64_t K, int64_t M, int64_t B, void* workspace, hipStream_t stream) {
  const int elt = dw_elt(dtype);
  const char* X = static_cast<const char*>(input);
  const char* dY = static_cast<const char*>(grad_out);
  Desc d;
  const int64_t tiles_upper = ((N + kTile - 1) / kTile + B) * dw_describe(d, X, dY, 0, K, M, elt, 0, r.K, r.MC);
  PYG_HIP_REQUIRE(tiles_upper < (1LL << 31), "segment_matmul_dw: too many tiles");
  const DwWorkspace w = carve_dw(workspace, B, r, M);
  const int64_t* dptr = ptr;
  if (!ptr_on_device) {
    if (int rc = stage_host_ptr("segment_matmul_dw", ptr, B, N, w.ptr_copy, stream)) return rc;
    dptr = w.ptr_copy;
  }
  hipLaunchKernelGGL(dw_plan_kernel<Desc>, dim3(1), dim3(256), 0, stream, dptr, B, X, dY, K, M, elt, r.K, r.MC,
                     static_cast<Desc*>(w.descs), w.tile_start);
  PYG_HIP_CHECK(hipGetLastError());
  // a relation starts ptr[b] rows into the tensors: its alignment is at least that of the base and the row pitch
  const int lg = gen_log2_align((uint64_t)input | (uint64_t)(K * elt) | (uint64_t)grad_out | (uint64_t)(M * elt));
  return run_dw_route(r, dtype, w, B, M, tiles_upper, grad_other, lg, stream);
}

// grouped form on a checked route: plan on the host (G is small) -- descriptors + tile prefix in one pinned H2D copy --,
// then the route's kernel
template <typename Desc>
int dw_grouped(DwRoute r, int dtype, const pyg_hip_group* host_groups, int64_t G, void* out_pool, void* workspace,
               hipStream_t stream) {
  const int elt = dw_elt(dtype);
  const DwWorkspace w = carve_dw(workspace, G, r, host_groups[0].m);
  void* staged = nullptr;
  int rc = pinned_stage().acquire(w.plan_bytes, &staged);
  if (rc != PYG_HIP_OK) return rc;
  Desc* hd = static_cast<Desc*>(staged);
  int32_t* ht = reinterpret_cast<int32_t*>(static_cast<char*>(staged) + (reinterpret_cast<char*>(w.tile_start) - static_cast<char*>(w.descs)));
  int64_t t = 0, off = 0;
  int lg = 4;  // the smallest alignment class (OR of addresses and row pitches) over the groups that are read
  for (int64_t i = 0; i < G; ++i) {
    const pyg_hip_group& g = host_groups[i];
    ht[i] = (int32_t)t;
    t += (g.rows + kTile - 1) / kTile * dw_describe(hd[i], static_cast<const char*>(g.input), static_cast<const char*>(g.other),
                                                    g.rows, g.k, g.m, elt, off, r.K, r.MC);
    PYG_HIP_REQUIRE(t < (1LL << 31), "grouped_matmul_dw: too many tiles");
    if (g.rows > 0 && g.k > 0 && g.m > 0)
      lg = std::min(lg, gen_log2_align((uint64_t)g.input | (uint64_t)(g.k * elt) | (uint64_t)g.other | (uint64_t)(g.m * elt)));
    off += (int64_t)g.k * g.m;
  }
  ht[G] = (int32_t)t;
  PYG_HIP_CHECK(hipMemcpyAsync(w.descs, staged, w.plan_bytes, hipMemcpyHostToDevice, stream));
  rc = pinned_stage().commit(stream);
  if (rc != PYG_HIP_OK) return rc;
  if (r.family != DwFamily::kGen) return run_dw_route(r, dtype, w, G, host_groups[0].m, t + 1, out_pool, lg, stream);
  if (off == 0) return PYG_HIP_OK;
  if (t == 0) {  // no rows anywhere: the result is all zeros
    PYG_HIP_CHECK(hipMemsetAsync(out_pool, 0, (size_t)elt * (size_t)off, stream));
    return PYG_HIP_OK;
  }
  return run_dw_route(r, dtype, w, G, 0, t, out_pool, lg, stream);
}

}  // namespace
}  // namespace pyg_hip

using namespace pyg_hip;

extern "C" {

void pyg_hip_matmul_dw_counters(int64_t* specialised, int64_t* general) {
  if (specialised) *specialised = g_dw_fast.load();
  if (general) *general = g_dw_gen.load();
}

const char* pyg_hip_matmul_dw_route(int dtype, int64_t K, int64_t M, int uniform, unsigned misalign) {
  if (K < 0 || M < 0) return "invalid";
  return dw_route_name(dtype, choose_dw_route(dtype, K, M, uniform != 0, misalign));
}

size_t pyg_hip_segment_matmul_dw_workspace_size(int64_t B, int64_t K, int64_t M) {
  return dw_workspace_bytes(std::max<int64_t>(B, 0), std::max<int64_t>(K, 0), std::max<int64_t>(M, 0), true);
}

size_t pyg_hip_grouped_matmul_dw_workspace_size(const pyg_hip_group* groups, int64_t G) {
  if (G <= 0 || groups == nullptr) return dw_workspace_bytes(0, 0, 0, false);
  bool uniform = true;
  for (int64_t i = 0; i < G; ++i) uniform = uniform && groups[i].k == groups[0].k && groups[i].m == groups[0].m;
  return dw_workspace_bytes(G, std::max(groups[0].k, 0), std::max(groups[0].m, 0), uniform);
}

int pyg_hip_segment_matmul_dw(int dtype, const void* input, const int64_t* ptr, int ptr_on_device, const void* grad_out,
                              void* grad_other, int64_t N, int64_t K, int64_t M, int64_t B, void* workspace,
                              size_t workspace_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PYG_HIP_REQUIRE(N >= 0 && K >= 0 && M >= 0 && B >= 0, "segment_matmul_dw: negative size");
  if (B * K * M == 0) return PYG_HIP_OK;
  PYG_HIP_REQUIRE(ptr && grad_other && (N == 0 || (input && grad_out)), "segment_matmul_dw: NULL tensor");
  if (!dw_dtype_ok(dtype))
    return fail(PYG_HIP_ERR_UNSUPPORTED, "segment_matmul_dw: float32 / bfloat16 / float16 only (dtype %d)", dtype);
  const size_t need = pyg_hip_segment_matmul_dw_workspace_size(B, K, M);
  if (workspace == nullptr || workspace_bytes < need)
    return fail(PYG_HIP_ERR_WORKSPACE, "segment_matmul_dw: workspace of %zu bytes needed, got %zu", need, workspace_bytes);
  const unsigned misalign = dw_misalign((uintptr_t)input | (uintptr_t)grad_out, grad_other, dw_elt(dtype));
  const DwRoute r = choose_dw_route(dtype, K, M, true, misalign);
  if (int rc = dw_route_check("segment_matmul_dw", r, K, M)) return rc;
  return dw_count(r, r.family == DwFamily::kGen
                         ? dw_segment<DwGenGroup>(r, dtype, input, ptr, ptr_on_device, grad_out, grad_other, N, K, M, B, workspace, stream)
                         : dw_segment<DwGroup>(r, dtype, input, ptr, ptr_on_device, grad_out, grad_other, N, K, M, B, workspace, stream));
}

int pyg_hip_grouped_matmul_dw(int dtype, const pyg_hip_group* host_groups, int64_t G, void* out_pool, void* workspace,
                              size_t workspace_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PYG_HIP_REQUIRE(G >= 0 && G < (1LL << 31), "grouped_matmul_dw: bad group count");
  if (G == 0) return PYG_HIP_OK;
  PYG_HIP_REQUIRE(host_groups && out_pool, "grouped_matmul_dw: NULL argument");
  if (!dw_dtype_ok(dtype))
    return fail(PYG_HIP_ERR_UNSUPPORTED, "grouped_matmul_dw: float32 / bfloat16 / float16 only (dtype %d)", dtype);
  const int64_t K = host_groups[0].k, M = host_groups[0].m;
  bool uniform = true;
  uintptr_t operands = 0;
  for (int64_t i = 0; i < G; ++i) {
    const pyg_hip_group& g = host_groups[i];
    PYG_HIP_REQUIRE(g.rows >= 0 && g.k >= 0 && g.m >= 0, "grouped_matmul_dw: negative size in group %lld", (long long)i);
    PYG_HIP_REQUIRE(g.rows == 0 || g.k == 0 || g.m == 0 || (g.input && g.other), "grouped_matmul_dw: NULL tensor in group %lld",
                    (long long)i);
    uniform = uniform && g.k == K && g.m == M;
    operands |= (uintptr_t)g.input | (uintptr_t)g.other;
  }
  const size_t need = pyg_hip_grouped_matmul_dw_workspace_size(host_groups, G);
  if (workspace == nullptr || workspace_bytes < need)
    return fail(PYG_HIP_ERR_WORKSPACE, "grouped_matmul_dw: workspace of %zu bytes needed, got %zu", need, workspace_bytes);
  // per-group shapes, shapes without a specialised kernel, element-aligned views: the general-shape kernel, whose limits
  // then hold for every group
  const unsigned misalign = dw_misalign(operands, out_pool, dw_elt(dtype));
  const DwRoute r = choose_dw_route(dtype, K, M, uniform, misalign);
  for (int64_t i = 0; i < G; ++i) {
    const int64_t k = host_groups[i].k, m = host_groups[i].m;
    if (int rc = dw_route_check("grouped_matmul_dw", choose_dw_route(dtype, k, m, uniform, misalign), k, m)) return rc;
  }
  return dw_count(r, r.family == DwFamily::kGen ? dw_grouped<DwGenGroup>(r, dtype, host_groups, G, out_pool, workspace, stream)
                                                : dw_grouped<DwGroup>(r, dtype, host_groups, G, out_pool, workspace, stream));
}

}  // extern "C"
