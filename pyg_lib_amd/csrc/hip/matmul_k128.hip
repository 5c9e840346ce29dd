// The 16-bit K = M = 128 kernels of segment_matmul / grouped_matmul that differ from the contiguous-range kernel
// (matmul_lds.hip) in the ORDER in which the chip sweeps `input` and `out`: the banded cyclic schedule (W by LDS-DMA in
// its native layout, two buffers) and the ticket schedule (tiles drawn in address order, W in registers).  The item-ring
// kernel for many short relations is matmul_ring.hip's; tile tables and the route choice: matmul.hip.
#include "matmul_common.h"

#include <algorithm>
#include <type_traits>

namespace pyg_hip {
namespace {

// ---- 16-bit, K = 128, 128 output columns: cyclic schedule, W by LDS-DMA in its native layout ---------------------
// The contiguous-range kernel above keeps ~1000 independent read / write streams alive (one per wave); how fast the
// HBM side serves that depends on where the caching allocator happened to place `input` and `out` (measured on one
// box, same launch, six candidate output buffers: 5.0 ... 6.1 TB/s, ~3 of 4 allocations at the low end).  Here every
// workgroup (8 waves, 256-row tile) takes every G/8-th tile of its XCD's band, so the chip sweeps eight narrow windows
// of `input` / `out` front to back (5.4 - 6.3 TB/s on the same buffers).  A workgroup then changes relation every other
// tile, so the weight switch must be free:
//   * W[g] is copied [K][M] as it lies in memory by LDS-DMA (global_load_lds_dwordx4, 8 waves x 4 KiB); the 16-byte
//     chunks of every 1 KiB block (4 k-rows) are permuted on the SOURCE side so that
//   * the MFMA "A" fragments (8 consecutive k of one output column) come out of gfx950's transposing LDS read
//     (ds_read_b64_tr_b16, two per fragment) without bank conflicts: a 32-lane service group touches
//     4 k-rows x {chunks 2tt, 2tt+1, 8+2tt, 9+2tt}, which the permutation places in one 256-byte line;
//   * two W buffers: the next relation of this workgroup's tile sequence is in flight while the current one is
//     multiplied; ONE workgroup barrier per relation change (everybody is done with the buffer that is refilled next,
//     and everybody's part of the new W has landed -- each wave has waited for its own DMAs because they are older
//     than the X tile it has just staged).
// X staging, fragment order, epilogue and store order are those of mfma_rows_lds_kernel.
template <typename T>
__global__ __launch_bounds__(512) void mfma_rows_cyc_kernel(const DevGroup* __restrict__ descs,
                                                            const int32_t* __restrict__ tile_start, int B) {
  constexpr int K = 128, MC = 128, SZ = 2, NWV = 8;
  constexpr int NT = 4, NI = 8, NO = 8, CPR = 16;
  constexpr int BM = NWV * 32;
  static_assert(BM == 2 * kTileRows, "tile_start2 is built for 256-row tiles");
  constexpr int WB = K * MC * SZ;  // 32 KB per W buffer
  constexpr int BLK_PER_WAVE = (K / 4) / NWV;
  typedef __attribute__((address_space(3))) void LDSV;
  typedef short v4i16 __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(1))) u32x4 GU32x4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, x = lane & 31, h = lane >> 5;
  const int bx = blockIdx.x, G = gridDim.x;
  char* stage = smem + 2 * WB + wave * 8192;
  // Banded cyclic schedule: the tiles are cut into 8 contiguous bands, the workgroups of XCD k (ids k, k + 8, ...:
  // consecutive ids go to consecutive XCDs) sweep band k cyclically -- 8 narrow windows instead of one, every page and
  // L2 line is touched by ONE XCD.  Same rate as the single sweep on unfavourably placed buffers (5.4 TB/s), 6.3
  // instead of 5.8 TB/s on favourable ones (tools/lab: v3:sched=2).
  const int total = tile_start[B];
  const int nb = (G & 7) == 0 ? 8 : 1;
  const int band = bx % nb, per = G / nb;
  const int band0 = (int)((int64_t)band * total / nb), band1 = (int)((int64_t)(band + 1) * total / nb);
  const int cbase = band0 + bx / nb;  // first tile of this workgroup; then every `per`-th tile of the band
  if (cbase >= band1) return;
  const int nloc = (band1 - 1 - cbase) / per + 1;

  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile_start[mid] <= cbase) lo = mid; else hi = mid;
  }
  int g = lo;  // group of the tile being prefetched

  // DMA side: lane i of a block's instruction fills LDS position i (16 bytes) of the 1 KiB block
  const int dma_r = (lane & 15) >> 2, dma_ii = lane & 3, dma_u = lane >> 4;
  const int dma_c = 2 * dma_u + (dma_ii & 1) + 8 * (dma_ii >> 1);
  const int dma_src_off = dma_r * (MC * SZ) + dma_c * 16;
  auto issue_w = [&](int grp_id, int buf) {
    const char* w = descs[grp_id].w;
#pragma unroll
    for (int j = 0; j < BLK_PER_WAVE; ++j) {
      const int kb = wave * BLK_PER_WAVE + j;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(w + kb * 1024 + dma_src_off),
                                       (LDSV*)(smem + buf * WB + kb * 1024), 16, 0, 0);
    }
  };
  // group of the first tile of this workgroup's sequence behind group `gc` (-1: none)
  auto next_group = [&](int gc) -> int {
    const int ts = tile_start[gc + 1];
    if (ts >= total) return -1;
    const int j = ts > cbase ? (ts - cbase + per - 1) / per : 0;
    if (j >= nloc) return -1;
    const int t = cbase + j * per;
    int gg = gc + 1;
    while (tile_start[gg + 1] <= t) ++gg;
    return gg;
  };
  // reader side (transposing read): lane q of a 16-lane group supplies k-row (q >> 2), piece (q & 3)
  const int q = lane & 15, grp16 = lane >> 4;
  const int a_lane_off = 16384 * h + (4 * (q >> 2) + (grp16 & 1) + 2 * (q & 1)) * 16 + ((q & 3) >> 1) * 8;

  u32x4 xr[NI];
  DevGroup dn = descs[g];
  int64_t n_row0 = 0, n_rows = 0;
  bool n_valid = false;
  auto prefetch = [&](int ti) {
    const int t = cbase + ti * per;
    while (t >= tile_start[g + 1]) {
      ++g;
      dn = descs[g];
    }
    n_rows = dn.rows;
    n_row0 = (int64_t)(t - tile_start[g]) * BM + wave * 32;
    n_valid = n_row0 < n_rows;
    if (n_valid) {
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int p = i * 64 + lane;
        const int r = p / CPR;
        const int cs = p % CPR;
        const int c = cs ^ (r & 15);
        int64_t row = n_row0 + r;
        if (row >= n_rows) row = n_rows - 1;
        const GU32x4* src = (const GU32x4*)(dn.a + row * (K * SZ) + c * 16);
        xr[i] = __builtin_nontemporal_load(src);
      }
    }
  };

  int wcur = g, wbuf = 0;
  issue_w(wcur, 0);
  int wnext = next_group(wcur);
  if (wnext >= 0) issue_w(wnext, 1);
  prefetch(0);
  DevGroup d = dn;
  int cg = g;
  int64_t row0 = n_row0, rows = n_rows;
  bool valid = n_valid;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (valid) {
#pragma unroll
    for (int i = 0; i < NI; ++i) *reinterpret_cast<u32x4*>(stage + (i * 64 + lane) * 16) = xr[i];
  }
  if (1 < nloc) prefetch(1);

  for (int t = 0; t < nloc; ++t) {
    u32x4 ov[NO];
    if (valid) {
      f32x16 acc[NT];
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
      const char* wb = smem + wbuf * WB + a_lane_off;
#pragma unroll
      for (int s = 0; s < NI; ++s) {
        const u32x4 xa = *reinterpret_cast<const u32x4*>(stage + (x * CPR + ((NI * h + s) ^ (x & 15))) * 16);
        u32x4 wa[NT];
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
          const v4i16 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) v4i16*)(wb + (2 * s) * 1024 + tt * 256));
          const v4i16 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) v4i16*)(wb + (2 * s + 1) * 1024 + tt * 256));
          wa[tt] = __builtin_bit_cast(u32x4, __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7));
        }
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) acc[tt] = mfma_chunk(T{}, wa[tt], xa, acc[tt]);
      }
      const T* bp = d.bias ? reinterpret_cast<const T*>(d.bias) + (MC / 2) * h : nullptr;
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        float v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = acc[tt][r];
        if (bp) {
#pragma unroll
          for (int r = 0; r < 16; ++r) v[r] = round_to(T{}, v[r]) + load_bias(bp + 16 * tt + r);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int c = NO * h + 2 * tt + j;
          *reinterpret_cast<u32x4*>(stage + (x * 16 + (c ^ (x & 15))) * 16) = pack8(T{}, v + 8 * j);
        }
      }
#pragma unroll
      for (int i = 0; i < NO; ++i) ov[i] = *reinterpret_cast<const u32x4*>(stage + (i * 64 + lane) * 16);
    }
    const DevGroup d_out = d;
    const int64_t row0_out = row0, rows_out = rows;
    const bool valid_out = valid;
    if (t + 1 < nloc) {
      d = dn;
      cg = g;
      row0 = n_row0;
      rows = n_rows;
      valid = n_valid;
      if (valid) {
#pragma unroll
        for (int i = 0; i < NI; ++i) *reinterpret_cast<u32x4*>(stage + (i * 64 + lane) * 16) = xr[i];
      }
      if (cg != wcur) {
        // relation change (same tile index in every wave of the workgroup)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        wcur = cg;
        wbuf ^= 1;
        wnext = next_group(wcur);
        if (wnext >= 0) issue_w(wnext, wbuf ^ 1);
      }
      if (t + 2 < nloc) prefetch(t + 2);
    }
    if (valid_out) {
      char* obase = d_out.c + (row0_out * MC) * SZ;
#pragma unroll
      for (int i = 0; i < NO; ++i) {
        const int p = i * 64 + lane;
        const int r = p / 16;
        const int cs = p % 16;
        const int c = cs ^ (r & 15);
        if (row0_out + r < rows_out) {
          GU32x4* dst = (GU32x4*)(obase + (int64_t)r * MC * SZ + c * 16);
          __builtin_nontemporal_store(ov[i], dst);
        }
      }
    }
  }
}

// ---- 16-bit, K = 128, 128 output columns: ticket schedule, W in registers ---------------------------------------
// What bounds the two kernels above is the WRITE side of HBM, and how well it is served depends on the order in which
// the chip touches `out` (tools/lab: write-only sweeps of the same buffer run at 5.3 - 6.9 TB/s depending on nothing
// but that order).  Measured on buffers the allocator placed unfavourably, three things matter, and they add up:
//   1. tiles are handed out IN ADDRESS ORDER, as a non-persistent grid would be dispatched, not pre-assigned: a
//      workgroup draws its next tile from a counter (one per XCD) when it gets there, so the window of rows in flight
//      stays narrow however unevenly the waves progress;
//   2. the XCDs are dealt chunks of 256 KiB (kChunkTiles tiles) of that order -- 32 and 64 KiB chunks are a resonance of
//      the memory side (5.4 TB/s where 16 KiB or >= 128 KiB chunks give 6.2 - 6.6 for the same copy), and 256 KiB is the
//      measured optimum for this kernel (192 / 320 / 512 KiB: 5.5 / 5.7 / 6.0 TB/s);
//   3. few bytes in flight per CU: six waves with one tile ahead each (96 KiB) beat eight or twelve.
// Six waves per CU cannot share a 32 KiB W through LDS three ways (3 x (32 + 2 x 16) KiB), so each wave keeps the
// relation's W in REGISTERS: its 32 MFMA A fragments are 128 VGPRs, refilled through a 16 KiB staging area (two
// halves, by LDS-DMA + ds_read_b64_tr_b16 exactly as in the cyclic kernel) when the relation changes -- at most once
// per relation and workgroup, because a workgroup's tickets ascend.  A workgroup is a PAIR of waves (64-row tile):
//   * X: LDS-DMA into two 8 KiB stages per wave, the next tile in flight while this one is multiplied.  The DMA is
//     issued from inline asm so that the compiler does not know LDS is written behind its back -- it cannot tell the
//     stage buffers or the ticket ring apart and would otherwise put s_waitcnt vmcnt(0) before every LDS access;
//   * tickets: wave (s & 1) requests ticket s TWO tiles ahead with an asynchronous global atomic (inline asm, the
//     return value is collected one iteration later) and hands it to its partner through a 4-slot LDS ring -- the two
//     waves can never be more than two tickets apart, so no slot is overwritten before it was read;
//   * every wait names exactly how many YOUNGER vector-memory operations may stay in flight (vmcnt retires in order):
//     per iteration a wave issues [atomic] [8 DMA of tile i+1] ... [8 stores of tile i], always 8 stores (rows behind
//     the segment end rewrite its last row with that row's own data), so neither the previous tile's stores nor the
//     next tile's DMA are ever waited for;
//   * the loop nest is (runs of one relation) x (tiles): W is loop-invariant in the inner loop, otherwise the register
//     allocator copies all 128 registers around every iteration.
// Lane-derived values are re-derived where used (v_mbcnt, two VALU ops) instead of living in VGPRs across the kernel.
constexpr int kChunkTiles = 16;  // 16 x 64 rows x 256 B = 256 KiB of X (and of out) per XCD turn

__device__ __forceinline__ void wait_vmcnt_16_17(int n) {  // steady state: 16 or 17 younger operations; else drain
  if (n == 17) asm volatile("s_waitcnt vmcnt(17)" ::: "memory");
  else if (n == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <typename T>
__global__ __launch_bounds__(128, 2) void mfma_rows_ticket_kernel(const DevGroup* __restrict__ descs,
                                                                  const int32_t* __restrict__ tile_start, int B,
                                                                  unsigned int* __restrict__ tickets) {
  constexpr int NT = 4, NI = 8, NO = 8;
  typedef __attribute__((address_space(3))) void LDSV;
  typedef short v4i16 __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(1))) u32x4 GU32x4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  auto lane_now = [&]() -> int {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
  };
  char* wst = smem;                            // 16 KiB: W staging on a relation change, else 2 x 8 KiB epilogue scratch
  char* xs0 = smem + 16384 + wave * 16384;     // this wave's two X stages
  int* ring_val = (int*)(smem + 49152);        // [4] ticket values, [4] generations
  int* ring_gen = ring_val + 4;
  if (threadIdx.x < 8) ring_val[threadIdx.x] = 0;
  __syncthreads();
  const int k8 = blockIdx.x & 7;
  const int total = tile_start[B];
  unsigned int* my_ctr = tickets + k8 * 32;
  auto tile_of = [&](int v) -> int { return ((v / kChunkTiles) * 8 + k8) * kChunkTiles + v % kChunkTiles; };

  unsigned int raw = 0;  // lane 0: return value of the last request, valid once the matching wait has passed
  auto request = [&]() {
    unsigned long long sv;
    asm volatile(
        "s_nop 4\n\t"  // (as in issue_x)
        "s_mov_b64 %[sv], exec\n\t"
        "s_mov_b64 exec, 1\n\t"
        "s_nop 0\n\t"
        "global_atomic_add %[ret], %[off], %[one], %[base] sc0\n\t"
        "s_mov_b64 exec, %[sv]"
        : [ret] "+v"(raw), [sv] "=&s"(sv)
        : [off] "v"(0), [one] "v"(1u), [base] "s"(my_ctr)
        : "memory");
  };
  auto publish = [&](int s) -> int {  // after the wait for the request
    asm volatile("" : "+v"(raw));
    const int v = __builtin_amdgcn_readfirstlane((int)raw);
    if (lane_now() == 0) {
      __hip_atomic_store(&ring_val[s & 3], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_store(&ring_gen[s & 3], (s >> 2) + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    return v;
  };
  auto consume = [&](int s) -> int {
    int v = 0;
    if (lane_now() == 0) {
      while (__hip_atomic_load(&ring_gen[s & 3], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != (s >> 2) + 1)
        __builtin_amdgcn_s_sleep(1);
      v = __hip_atomic_load(&ring_val[s & 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    return __builtin_amdgcn_readfirstlane(v);
  };

  u32x4 wreg[NI][NT];  // A fragment of k-step s, column block tt (layout: see mfma_rows_cyc_kernel)
  T* bias_lds = reinterpret_cast<T*>(smem + 49152 + 64);  // the relation's 128 bias values (read through LDS: a global
                                                         // load in the epilogue would drag an s_waitcnt vmcnt(0) along)
  auto load_w = [&](const char* w, const char* bias, int trans) {
    const int lane = lane_now(), h = lane >> 5;
    if (trans) {
      // `other` stored [M][K] (the dX pass hands W itself and asks for X W^T): a fragment -- 8 consecutive k of one
      // output column -- is then 16 contiguous bytes; lane x is A-row x, i.e. output column
      // 64 ((x >> 2) & 1) + 16 tt + 4 (x >> 3) + (x & 3) (the column mapping of the cyclic kernel's LDS image)
      __syncthreads();  // the partner is done with the previous relation's bias
      if (bias) bias_lds[threadIdx.x] = reinterpret_cast<const T*>(bias)[threadIdx.x];
      const int xx = lane & 31;
      const char* wl = w + (64 * ((xx >> 2) & 1) + 4 * (xx >> 3) + (xx & 3)) * 256 + 128 * h;
#pragma unroll
      for (int s = 0; s < NI; ++s)
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) wreg[s][tt] = *reinterpret_cast<const u32x4*>(wl + tt * 16 * 256 + s * 16);
      __syncthreads();  // the bias is in place
      return;
    }
    const int dma_r = (lane & 15) >> 2, dma_ii = lane & 3, dma_u = lane >> 4;
    const int dma_c = 2 * dma_u + (dma_ii & 1) + 8 * (dma_ii >> 1);
    const int dma_src_off = dma_r * 256 + dma_c * 16;
    const int q = lane & 15, grp16 = lane >> 4;
    const int a_lane_off = 8192 * h + (4 * (q >> 2) + (grp16 & 1) + 2 * (q & 1)) * 16 + ((q & 3) >> 1) * 8;
#pragma unroll
    for (int r2 = 0; r2 < 2; ++r2) {  // k-steps 4 r2 ... 4 r2 + 3: 1 KiB blocks {8 r2 ... 8 r2 + 7} of both k halves
      __syncthreads();
      if (r2 == 0 && bias) bias_lds[threadIdx.x] = reinterpret_cast<const T*>(bias)[threadIdx.x];
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int kb = wave * 16 + r2 * 8 + jj;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(w + kb * 1024 + dma_src_off),
                                         (LDSV*)(wst + (wave * 8 + jj) * 1024), 16, 0, 0);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
          const v4i16 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) v4i16*)(wst + a_lane_off + (2 * s4) * 1024 + tt * 256));
          const v4i16 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) v4i16*)(wst + a_lane_off + (2 * s4 + 1) * 1024 + tt * 256));
          wreg[r2 * 4 + s4][tt] = __builtin_bit_cast(u32x4, __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7));
        }
      }
    }
  };
  // 16-byte chunk cs of row r of a stage holds chunk cs ^ (r & 15) of the X row (permuted on the source side)
  struct Rel {  // the fields of a DevGroup this kernel uses (copying the whole struct sends its tail through scratch)
    const char* a;
    const char* w;
    char* c;
    const char* bias;
    int64_t rows;
    int trans;
  };
  auto rel_of = [&](int gi) -> Rel {
    const DevGroup* p = descs + gi;
    return Rel{p->a, p->w, p->c, p->bias, p->rows, p->trans};
  };
  auto issue_x = [&](const Rel& dg, int64_t row0, int buf) {
    const uint32_t lds = (uint32_t)(size_t)(xs0 + buf * 8192);
    const char* base = dg.a + row0 * 256;
    const int64_t left = dg.rows - row0;
    const int last = left < 32 ? (int)left - 1 : 31;
    const int l = lane_now();
    const int l4 = l >> 4, c0 = (l & 15) ^ l4;
    uint32_t off[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      int r = 4 * i + l4;
      const int c = c0 ^ (4 * (i & 3));
      r = r > last ? last : r;
      off[i] = (uint32_t)(r * 256 + c * 16);
    }
    uint32_t sv;
    asm volatile(
        "s_nop 4\n\t"  // base / lds may have been written by v_readfirstlane: VALU-written SGPR -> VMEM address / M0
        "s_mov_b32 %[sv], m0\n\t"
        "s_mov_b32 m0, %[lds]\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %[o0], %[base] nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
        "global_load_lds_dwordx4 %[o1], %[base] nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
        "global_load_lds_dwordx4 %[o2], %[base] nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
        "global_load_lds_dwordx4 %[o3], %[base] nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
        "global_load_lds_dwordx4 %[o4], %[base] nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
        "global_load_lds_dwordx4 %[o5], %[base] nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
        "global_load_lds_dwordx4 %[o6], %[base] nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
        "global_load_lds_dwordx4 %[o7], %[base] nt\n\t"
        "s_mov_b32 m0, %[sv]"
        : [sv] "=&s"(sv)
        : [lds] "s"(lds), [base] "s"(base), [o0] "v"(off[0]), [o1] "v"(off[1]), [o2] "v"(off[2]), [o3] "v"(off[3]),
          [o4] "v"(off[4]), [o5] "v"(off[5]), [o6] "v"(off[6]), [o7] "v"(off[7])
        : "memory", "scc");
  };

  // ticket 0 synchronously (wave 0); wave 1 requests ticket 1 only after that: a workgroup's tickets must ascend
  int t_cur;
  if (wave == 0) {
    request();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    t_cur = tile_of(publish(0));
  } else {
    t_cur = tile_of(consume(0));
    request();
  }
  if (t_cur >= total) return;
  int g;
  {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (tile_start[mid] <= t_cur) lo = mid; else hi = mid;
    }
    g = lo;
  }
  Rel d = rel_of(g);
  int64_t row0 = (int64_t)(t_cur - tile_start[g]) * kPairRows + wave * 32;
  bool valid = row0 < d.rows;
  int d_cur = 0;  // DMA instructions of the current tile (issued one iteration ago)
  if (valid) {
    issue_x(d, row0, 0);
    d_cur = 8;
  }
  int s_prev = 0;  // store instructions of the previous tile
  int buf = 0, i = 0;
  bool done = false;
  while (!done) {  // one pass per run of tiles of the same relation
    load_w(d.w, d.bias, d.trans);
    const int wcur = g;
    for (;; ++i) {
      // ticket i + 1 (requested one iteration ago by wave (i + 1) & 1; younger: this tile's DMA, the previous stores)
      int v_next;
      if (((i + 1) & 1) == wave) {
        wait_vmcnt_16_17(d_cur + s_prev);
        v_next = publish(i + 1);
      } else {
        v_next = consume(i + 1);
      }
      const int t_next = tile_of(v_next);
      const bool more = t_next < total;
      int a_now = 0;
      if (more && ((i + 2) & 1) == wave) {
        request();
        a_now = 1;
      }
      int gn = g;
      Rel dn = d;
      int64_t n_row0 = 0;
      bool n_valid = false;
      int d_next = 0;
      if (more) {
        if (t_next >= tile_start[gn + 1]) {
          do ++gn; while (t_next >= tile_start[gn + 1]);
          dn = rel_of(gn);
        }
        n_row0 = (int64_t)(t_next - tile_start[gn]) * kPairRows + wave * 32;
        n_valid = n_row0 < dn.rows;
        if (n_valid) {
          issue_x(dn, n_row0, buf ^ 1);
          d_next = 8;
        }
      }
      // this tile's X has landed (younger: the previous stores, the request, the next tile's DMA)
      wait_vmcnt_16_17(s_prev + a_now + d_next);
      int s_now = 0;
      if (valid) {
        const char* stage = xs0 + buf * 8192;
        char* scratch = wst + wave * 8192;
        const int lc = lane_now();
        const int xo = lc & 31, h = lc >> 5;
        const int cb = (NI * h) ^ (xo & 15);
        const bool has_bias = d.bias != nullptr;
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {  // one 32-column block at a time: 16 accumulators next to the 128 of W
          f32x16 acc;
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = 0.f;
          const char* xrow = stage + xo * 256;
          u32x4 xa = *reinterpret_cast<const u32x4*>(xrow + cb * 16);
#pragma unroll
          for (int s = 0; s < NI; ++s) {
            u32x4 xn = xa;
            if (s + 1 < NI) xn = *reinterpret_cast<const u32x4*>(xrow + (cb ^ (s + 1)) * 16);
            acc = mfma_chunk(T{}, wreg[s][tt], xa, acc);
            __builtin_amdgcn_sched_barrier(0);
            xa = xn;
          }
          float v[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) v[r] = acc[r];
          if (has_bias) {
            const T* bp = bias_lds + 64 * h + 16 * tt;
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = round_to(T{}, v[r]) + load_bias(bp + r);
          }
#pragma unroll
          for (int j = 0; j < 2; ++j)
            *reinterpret_cast<u32x4*>(scratch + xo * 256 + (cb ^ (2 * tt + j)) * 16) = pack8(T{}, v + 8 * j);
        }
        // always 8 stores (the waits count them): lanes whose row lies behind the segment end rewrite its last row
        char* obase = d.c + row0 * 256;
        const int64_t left = d.rows - row0;
        const int last = left < 32 ? (int)left - 1 : 31;
        const int l = lane_now();
        const int l4 = l >> 4, cs = l & 15;
#pragma unroll
        for (int ii = 0; ii < NO; ++ii) {
          int r = 4 * ii + l4;
          r = r > last ? last : r;
          const u32x4 ov = *reinterpret_cast<const u32x4*>(scratch + r * 256 + cs * 16);
          GU32x4* dst = (GU32x4*)(obase + (uint32_t)(r * 256 + (cs ^ (r & 15)) * 16));
          __builtin_nontemporal_store(ov, dst);
          if ((ii & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        s_now = 8;
      }
      if (!more) {
        done = true;
        break;
      }
      t_cur = t_next;
      g = gn;
      d = dn;
      row0 = n_row0;
      valid = n_valid;
      d_cur = d_next;
      s_prev = s_now;
      buf ^= 1;
      if (g != wcur) {
        ++i;
        break;
      }
    }
  }
}

template <typename T>
int launch_cyc(const DevGroup* descs, const int32_t* tile_start2, int B, int64_t tiles2_upper, hipStream_t stream) {
  constexpr int lds = 2 * 128 * 128 * 2 + 8 * 8192;  // two W buffers + 8 stages = 128 KB
  if (int rc_ = ensure_dynamic_lds(reinterpret_cast<const void*>(&mfma_rows_cyc_kernel<T>), lds)) return rc_;
  unsigned gx = tile_grid(tiles2_upper, 1);
  if (gx >= 8) gx -= gx % 8;  // whole octets of workgroups: one band of tiles per XCD
  hipLaunchKernelGGL((mfma_rows_cyc_kernel<T>), dim3(gx), dim3(512), lds, stream, descs, tile_start2, B);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

template <typename T>
int launch_ticket(const DevGroup* descs, const int32_t* tile_start3, int B, int64_t tiles3_upper, unsigned int* tickets,
                  hipStream_t stream) {
  constexpr int lds = 16384 + 2 * 16384 + 64 + 256;  // W staging / epilogue scratch, 2 x 2 X stages, ticket ring, bias
  if (int rc_ = ensure_dynamic_lds(reinterpret_cast<const void*>(&mfma_rows_ticket_kernel<T>), lds)) return rc_;
  int64_t gx = std::min<int64_t>(std::max<int64_t>(tiles3_upper, 8), 3 * (int64_t)device_info().num_cus);
  gx -= gx % 8;  // whole octets: every one of the 8 counters is served
  hipLaunchKernelGGL((mfma_rows_ticket_kernel<T>), dim3((unsigned)gx), dim3(128), lds, stream, descs, tile_start3, B, tickets);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

}  // namespace

int launch_k128_cyc(int dtype, const void* descs, const int32_t* tile_start2, int B, int64_t tiles2_upper, hipStream_t stream) {
  const DevGroup* d = static_cast<const DevGroup*>(descs);
  return dtype == PYG_BF16 ? launch_cyc<bf16_t>(d, tile_start2, B, tiles2_upper, stream)
                           : launch_cyc<f16_t>(d, tile_start2, B, tiles2_upper, stream);
}

int launch_k128_ticket(int dtype, const void* descs, const int32_t* tile_start3, int B, int64_t tiles3_upper,
                       unsigned int* tickets, hipStream_t stream) {
  const DevGroup* d = static_cast<const DevGroup*>(descs);
  return dtype == PYG_BF16 ? launch_ticket<bf16_t>(d, tile_start3, B, tiles3_upper, tickets, stream)
                           : launch_ticket<f16_t>(d, tile_start3, B, tiles3_upper, tickets, stream);
}

}  // namespace pyg_hip
