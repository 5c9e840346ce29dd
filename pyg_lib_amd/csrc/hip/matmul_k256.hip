// The 16-bit K = 256 kernels of segment_matmul / grouped_matmul in which ONE workgroup owns 256 output columns, the
// whole 128 KB weight in LDS as two swizzled K-halves: 32 rows per wave (any M % 256 == 0) and 64 rows per wave
// (M = 256).  The register-W item-ring kernel for this shape is matmul_ring.hip's; tile tables and the route choice:
// matmul.hip.
#include "matmul_common.h"

#include <algorithm>
#include <type_traits>

namespace pyg_hip {
namespace {

// ---- 16-bit, K = 256, 256 output columns per workgroup -------------------------------------------------
// With 128-column chunks an F = 256 layer needs two workgroups per tile range, i.e. every X tile travels
// through two CUs' load paths (C4: the kernel then moves 1.5x the algorithmic bytes at the same per-CU
// streaming rate as C2 and lands at 3.3 TB/s of useful traffic).  Here ONE workgroup owns all 256 columns:
// the whole weight matrix (128 KB) stays in LDS as two K-halves [256 columns][128 k] WITHOUT padding -- the
// 16-byte chunks of a row are XOR-swizzled with (row & 15) instead, which keeps the fragment reads
// conflict-free -- and the remaining 32 KB are four 8 KB stages.  A tile is two K-half passes into the same
// 8 x (32x32) accumulators (each pass = the K = 128 kernel's inner loop), X is read from HBM once, and the
// output leaves in two rounds of 4 column blocks through the stage (full 128-byte lines per row).
template <typename T, int NW>
__global__ __launch_bounds__(NW * 64) void mfma_rows_wide256_kernel(
    const DevGroup* __restrict__ descs, const int32_t* __restrict__ tile_start, int B, int chunk, int ncol) {
  typedef __attribute__((address_space(1))) u32x4 GU32x4;
  constexpr int SZ = 2;
  constexpr int K = 256, KH = 128, MC = 256;
  constexpr int NT = MC / 32;          // 8 accumulator blocks
  constexpr int BM = NW * 32;
  static_assert(BM == kTileRows, "tile table is built for 128-row tiles");
  constexpr int CPR = KH * SZ / 16;    // 16 chunks per half row
  constexpr int NI = CPR / 2;          // 8 loads / K steps per half
  constexpr int WROW = KH * SZ;        // 256 bytes per image row
  constexpr int WIMG = MC * WROW;      // 64 KB per K-half
  constexpr int STAGE = 32 * 256;      // 8 KB per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int x = lane & 31;
  const int h = lane >> 5;
  const int bx = ncol > 1 ? ((int)blockIdx.x / (8 * ncol)) * 8 + ((int)blockIdx.x & 7) : (int)blockIdx.x;
  const int by = ncol > 1 ? ((int)blockIdx.x / 8) % ncol : 0;
  const int col0 = by * MC;
  char* stage = smem + 2 * WIMG + wave * STAGE;

  const int total = tile_start[B];
  const int G = (int)gridDim.x / ncol;
  int nloc, cbase = 0;
  if (chunk <= 0) {
    cbase = (int)((int64_t)bx * total / G);
    nloc = (int)((int64_t)(bx + 1) * total / G) - cbase;
  } else {
    const int nchunks = (total + chunk - 1) / chunk;
    const int mine = nchunks > bx ? (nchunks - 1 - bx) / G + 1 : 0;
    nloc = mine * chunk;
    if (mine > 0) {
      const int last_chunk = (mine - 1) * G + bx;
      const int over = (last_chunk + 1) * chunk - total;
      if (over > 0) nloc -= over;
    }
  }
  if (nloc <= 0) return;
  auto tile_of = [&](int i) -> int {
    if (chunk <= 0) return cbase + i;
    const int j = i / chunk;
    return (j * G + bx) * chunk + (i - j * chunk);
  };
  const int t1 = nloc;
  int lo = 0, hi = B;
  {
    const int first = tile_of(0);
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (tile_start[mid] <= first) lo = mid; else hi = mid;
    }
  }
  int g = lo;
  int staged = -1;

  // image row (= output column) of lane x for accumulator block tt: crow0 + 16 tt; its swizzle is crow0 & 15
  const int crow0 = (MC / 2) * ((x >> 2) & 1) + 4 * (x >> 3) + (x & 3);
  const int wsw = crow0 & 15;
  const char* wrow = smem + crow0 * WROW;

  u32x4 xr[2][NI];
  DevGroup dn = descs[g];
  int64_t n_row0 = 0, n_rows = 0;
  bool n_valid = false;
  // plan(ti): which group / rows local tile ti covers for this wave; load_half(kh): its K-half into xr[kh]
  auto plan = [&](int ti) {
    const int t = tile_of(ti);
    while (t >= tile_start[g + 1]) {
      ++g;
      dn = descs[g];
    }
    n_rows = dn.rows;
    n_row0 = (int64_t)(t - tile_start[g]) * BM + wave * 32;
    n_valid = n_row0 < n_rows;
  };
  // The X loads are issued through inline asm and their vmcnt wait is placed by hand (wait_half): stores count
  // on vmcnt as well, and the wait the compiler would insert in front of the stage writes is a vmcnt(0) that
  // also waits for the output stores issued a moment earlier (microseconds per tile).  since[kh] = a LOWER bound
  // of the vector-memory instructions issued after the loads into xr[kh] (memory operations retire in order).
  int since[2] = {0, 0};
  auto load_half = [&](int kh) {
    if (!n_valid) return;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int p = i * 64 + lane;
      const int r = p / CPR;
      const int c = (p % CPR) ^ (r & 15);
      int64_t row = n_row0 + r;
      if (row >= n_rows) row = n_rows - 1;
      asm volatile("global_load_dwordx4 %0, %1, off nt" : "=v"(xr[kh][i])
                   : "v"(dn.a + row * (K * SZ) + kh * (KH * SZ) + c * 16) : "memory");
    }
    since[kh] = 0;
    since[kh ^ 1] += NI;
  };
  auto wait_half = [&](int kh) {
    const int n = since[kh];
    if (n >= 24) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    else if (n >= 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else if (n >= 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };

  plan(0);
  load_half(0);
  load_half(1);
  DevGroup d = dn;
  int cg = g;
  int64_t row0 = n_row0, rows = n_rows;
  bool valid = n_valid;

  for (int t = 0; t < t1; ++t) {
    if (cg != staged) {
      __syncthreads();
      const char* w = d.w;
      const int M = d.m;
      if (!d.trans) {
        // W[k][m] row-major: 8 columns per 16-byte load, scattered as 2-byte stores into the swizzled image
        constexpr int CW = MC / 8;
        for (int idx = tid; idx < K * CW; idx += NW * 64) {
          const int k = idx / CW;
          const int cc = (idx - k * CW) * 8;
          const u32x4 v = *reinterpret_cast<const u32x4*>(w + ((int64_t)k * M + col0 + cc) * SZ);
          char* img = smem + (k >= KH ? WIMG : 0);
          const int kk = k & (KH - 1);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int m = cc + e;
            const uint16_t sv = (uint16_t)(v[e >> 1] >> ((e & 1) * 16));
            *reinterpret_cast<uint16_t*>(img + m * WROW + (((kk >> 3) ^ (m & 15)) * 16) + (kk & 7) * 2) = sv;
          }
        }
      } else {
        // W^T[m][k] row-major: whole chunks
        constexpr int CW = K / 8;
        for (int idx = tid; idx < MC * CW; idx += NW * 64) {
          const int m = idx / CW;
          const int kc = idx - m * CW;  // chunk of 8 k
          const u32x4 v = *reinterpret_cast<const u32x4*>(w + ((int64_t)(col0 + m) * K + kc * 8) * SZ);
          char* img = smem + (kc >= CPR ? WIMG : 0);
          *reinterpret_cast<u32x4*>(img + m * WROW + (((kc & (CPR - 1)) ^ (m & 15)) * 16)) = v;
        }
      }
      __syncthreads();
      staged = cg;
    }

    // the next tile's loads go out as soon as the registers of a half are free: right after that half has been
    // written to the stage, a whole tile before they are needed
    const bool have_next = t + 1 < t1;
    if (have_next) plan(t + 1);
    f32x16 acc[NT];
    if (!valid && have_next) {
      load_half(0);
      load_half(1);
    }
    if (valid) {
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        // this half of the tile -> stage (row order -> swizzled rows), then the K steps
        wait_half(kh);
#pragma unroll
        for (int i = 0; i < NI; ++i) *reinterpret_cast<u32x4*>(stage + (i * 64 + lane) * 16) = xr[kh][i];
        if (have_next) load_half(kh);
        const char* img = wrow + kh * WIMG;
        u32x4 xa = *reinterpret_cast<const u32x4*>(stage + (x * CPR + ((NI * h) ^ (x & 15))) * 16);
        u32x4 wa[NT];
#pragma unroll
        for (int tt = 0; tt < NT; ++tt)
          wa[tt] = *reinterpret_cast<const u32x4*>(img + tt * 16 * WROW + (((NI * h) ^ wsw) * 16));
#pragma unroll
        for (int s = 0; s < NI; ++s) {
          asm volatile("" : "+v"(wa[NT - 1]));  // wait for this step's fragments before the next reads go out
          __builtin_amdgcn_sched_barrier(0);
          u32x4 xb = xa;
          u32x4 wb[NT];
          if (s + 1 < NI) {
            const int c = NI * h + s + 1;
            xb = *reinterpret_cast<const u32x4*>(stage + (x * CPR + (c ^ (x & 15))) * 16);
#pragma unroll
            for (int tt = 0; tt < NT; ++tt)
              wb[tt] = *reinterpret_cast<const u32x4*>(img + tt * 16 * WROW + ((c ^ wsw) * 16));
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int tt = 0; tt < NT; ++tt) acc[tt] = mfma_chunk(T{}, wa[tt], xa, acc[tt]);
          __builtin_amdgcn_sched_barrier(0);
          if (s + 1 < NI) {
            xa = xb;
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) wa[tt] = wb[tt];
          }
        }
      }
    }

    const DevGroup d_out = d;
    const int64_t row0_out = row0, rows_out = rows;
    const bool valid_out = valid;
    if (have_next) {
      d = dn;
      cg = g;
      row0 = n_row0;
      rows = n_rows;
      valid = n_valid;
    }

    if (valid_out) {
      const int M = d_out.m;
      char* obase = d_out.c + (row0_out * M + col0) * SZ;
      const bool full_out = row0_out + 32 <= rows_out;  // all 16 stores below are issued
      if (full_out) {
        since[0] += 16;
        since[1] += 16;
      }
      const T* bp = d_out.bias ? reinterpret_cast<const T*>(d_out.bias) + col0 + (MC / 2) * h : nullptr;
#pragma unroll
      for (int rd = 0; rd < 2; ++rd) {  // column blocks 4 rd .. 4 rd + 3 of both lane halves
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int tt = 4 * rd + q;
          float v[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) v[r] = acc[tt][r];
          if (bp) {
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = round_to(T{}, v[r]) + load_bias(bp + 16 * tt + r);
          }
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int c = 8 * h + 2 * q + j;  // 16 chunks per stage row: [half 0: 8 chunks | half 1: 8 chunks]
            *reinterpret_cast<u32x4*>(stage + (x * 16 + (c ^ (x & 15))) * 16) = pack_chunk(T{}, v + 8 * j);
          }
        }
        u32x4 ov[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) ov[i] = *reinterpret_cast<const u32x4*>(stage + (i * 64 + lane) * 16);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int p = i * 64 + lane;
          const int r = p >> 4;
          const int c = (p & 15) ^ (r & 15);
          if (full_out || row0_out + r < rows_out) {
            // columns (MC/2) * half + 64 rd + 8 * (c & 7)
            GU32x4* dst = (GU32x4*)(obase + (int64_t)r * M * SZ + ((MC / 2) * (c >> 3) + 64 * rd + 8 * (c & 7)) * SZ);
            __builtin_nontemporal_store(ov[i], dst);
          }
        }
      }
    }
  }
}

// ---- 16-bit, K = 256, 256 output columns, 64 rows per wave ----------------------------------------------------------
// PMC on the kernel above (C4, profiles/r2_pmc_c4_wide256.json): MFMA pipes busy 24 %, half of the wave cycles issuing
// and 30 % waiting -- its inner loop is bound by LDS reads, not by MFMA: every step a wave reads 8 KiB of W fragments
// + 1 KiB of X for 8 MFMAs (256 cycles), and the four waves of the CU share one 128 B/clk LDS (>= 288 cycles).  Here a
// wave owns TWO 32-row blocks (256-row workgroup tiles) and every W fragment feeds two MFMAs: 10 KiB of LDS reads per
// 16 MFMAs.  The 16 accumulator blocks (256 registers) live in AGPRs (one wave per SIMD: 512 registers), X arrives a
// K-QUARTER at a time -- 64 rows x 64 k = the wave's 8 KiB stage -- through two register buffers that are refilled
// two quarters ahead, and lane half h multiplies the 16-byte k-chunk 2 u + h in step u (a quarter is then one
// contiguous 128-byte line per row).  W image, column mapping and epilogue follow the kernel above.
//   There is no "this wave has no rows in this tile" path: such a wave (and every row behind a segment's end) works on
// the segment's LAST row instead -- loads clamp to it, its result is stored to it again (same bytes as its owner
// writes).  Every tile is then the same straight line of 32 loads and 32 stores, the loads are ordinary (compiler
// visible) loads, and with the first tile peeled the compiler's own s_waitcnt vmcnt counts are exact: the previous
// tile's stores stay in flight while this tile multiplies.  (A version with the loads in inline asm and hand-kept
// counts, as in the kernel above, broke on the invalid -> valid transition: the compiler may copy an asm output
// register at a control-flow merge before the data has arrived.)
template <typename T>
__global__ __launch_bounds__(256) void mfma_rows_wide256r2_kernel(const DevGroup* __restrict__ descs,
                                                                  const int32_t* __restrict__ tile_start, int B) {
  typedef __attribute__((address_space(1))) u32x4 GU32x4;
  constexpr int SZ = 2, NW = 4;
  constexpr int K = 256, KH = 128, MC = 256;
  constexpr int NT = MC / 32;      // 8 column blocks
  constexpr int BM = NW * 64;      // 256-row tiles
  static_assert(BM == 2 * kTileRows, "tile_start2 is built for 256-row tiles");
  constexpr int WROW = KH * SZ;    // 256 bytes per image row
  constexpr int WIMG = MC * WROW;  // 64 KB per K-half
  constexpr int STAGE = 8192;      // per wave: 64 rows x 128 B (a K quarter) / 32 rows x 256 B (an output round)
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int x = lane & 31;
  const int h = lane >> 5;
  const int bx = blockIdx.x, G = gridDim.x;
  char* stage = smem + 2 * WIMG + wave * STAGE;

  const int total = tile_start[B];
  const int cbase = (int)((int64_t)bx * total / G);
  const int t1 = (int)((int64_t)(bx + 1) * total / G) - cbase;
  if (t1 <= 0) return;
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile_start[mid] <= cbase) lo = mid; else hi = mid;
  }
  int g = lo;
  int staged = -1;

  // image row (= output column) of lane x for column block tt: crow0 + 16 tt; its swizzle is crow0 & 15
  const int crow0 = (MC / 2) * ((x >> 2) & 1) + 4 * (x >> 3) + (x & 3);
  const int wsw = crow0 & 15;
  const char* wrow = smem + crow0 * WROW;

  struct Rel {  // what a tile needs of its relation; `first` = the wave's first row, clamped into the segment
    const char* a;
    const char* w;
    char* c;
    const char* bias;
    int64_t first;
    int last;  // rows first .. first + last exist (0 <= last <= 63); later rows of the wave stand for first + last
    int trans;
    int group;
  };
  Rel nx;
  auto plan = [&](int ti) {
    const int t = cbase + ti;
    while (t >= tile_start[g + 1]) ++g;
    const DevGroup* p = descs + g;
    const int64_t rows = p->rows;
    int64_t r0 = (int64_t)(t - tile_start[g]) * BM + wave * 64;
    if (r0 > rows - 1) r0 = rows - 1;
    const int64_t left = rows - r0;
    nx = Rel{p->a, p->w, p->c, p->bias, r0, left < 64 ? (int)left - 1 : 63, p->trans, g};
  };
  // quarter q of the wave's 64 rows: instruction i covers rows 8 i .. 8 i + 7, lane l reads chunk
  // (l & 7) ^ ((row >> 1) & 7) of its row's 128-byte quarter, so that the linear stage write leaves chunk c at slot
  // c ^ ((row >> 1) & 7): ds_read_b128 serves the lane groups {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} (+32) in one
  // cycle each over 64 banks, and with 128-byte rows the bank is (row & 1, slot) -- (row >> 1) & 7 is a permutation of
  // 0..7 over the even rows of either group and over the odd ones (row & 7 gave 2-way conflicts).
  u32x4 xr[2][8];
  const int l3 = lane >> 3;
  auto load_q = [&](int b, const Rel& rl, int q) {
    const char* base = rl.a + rl.first * (K * SZ) + q * 128;  // wave-uniform
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = 8 * i + l3;
      const int coff = ((lane & 7) ^ ((row >> 1) & 7)) * 16;
      const int r = row > rl.last ? rl.last : row;
      xr[b][i] = __builtin_nontemporal_load((const GU32x4*)(base + (uint32_t)(r * (K * SZ) + coff)));
    }
  };

  Rel cur;
  auto tile_body = [&](int t) {
    if (cur.group != staged) {
      __syncthreads();
      const char* w = cur.w;
      if (!cur.trans) {
        // W[k][m] row-major: 8 columns per 16-byte load, scattered as 2-byte stores into the swizzled image
        constexpr int CW = MC / 8;
        for (int idx = tid; idx < K * CW; idx += NW * 64) {
          const int k = idx / CW;
          const int cc = (idx - k * CW) * 8;
          const u32x4 v = *reinterpret_cast<const u32x4*>(w + ((int64_t)k * MC + cc) * SZ);
          char* img = smem + (k >= KH ? WIMG : 0);
          const int kk = k & (KH - 1);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int m = cc + e;
            const uint16_t sv = (uint16_t)(v[e >> 1] >> ((e & 1) * 16));
            *reinterpret_cast<uint16_t*>(img + m * WROW + (((kk >> 3) ^ (m & 15)) * 16) + (kk & 7) * 2) = sv;
          }
        }
      } else {
        // W^T[m][k] row-major: whole chunks
        constexpr int CW = K / 8;
        for (int idx = tid; idx < MC * CW; idx += NW * 64) {
          const int m = idx / CW;
          const int kc = idx - m * CW;
          const u32x4 v = *reinterpret_cast<const u32x4*>(w + ((int64_t)m * K + kc * 8) * SZ);
          char* img = smem + (kc >= 16 ? WIMG : 0);
          *reinterpret_cast<u32x4*>(img + m * WROW + (((kc & 15) ^ (m & 15)) * 16)) = v;
        }
      }
      __syncthreads();
      staged = cur.group;
    }
    const bool have_next = t + 1 < t1;
    f32x16 acc[2][NT];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[rb][i][r] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int b = q & 1;
#pragma unroll
      for (int i = 0; i < 8; ++i) *reinterpret_cast<u32x4*>(stage + (i * 64 + lane) * 16) = xr[b][i];
      // refill this buffer two quarters ahead (the last tile of the workgroup reloads its own quarters: same count
      // of loads on every path, and nothing reads them)
      if (q < 2) {
        load_q(b, cur, q + 2);
      } else {
        if (q == 2) {
          if (have_next) plan(t + 1); else nx = cur;
        }
        load_q(b, nx, q - 2);
      }
      __builtin_amdgcn_sched_barrier(0);
      const char* img = wrow + (q >> 1) * WIMG;
      const char* xrow0 = stage + x * 128;
      const char* xrow1 = stage + (32 + x) * 128;
      const int xs = (x >> 1) & 7;  // rows x and 32 + x share it
      const int c0 = ((8 * q) & 15) + h;  // chunk within the K half of step j: c0 + 2 j
      u32x4 xa0 = *reinterpret_cast<const u32x4*>(xrow0 + ((h ^ xs) * 16));
      u32x4 xa1 = *reinterpret_cast<const u32x4*>(xrow1 + ((h ^ xs) * 16));
      u32x4 wa[NT];
#pragma unroll
      for (int tt = 0; tt < NT; ++tt)
        wa[tt] = *reinterpret_cast<const u32x4*>(img + tt * 16 * WROW + ((c0 ^ wsw) * 16));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        asm volatile("" : "+v"(wa[NT - 1]));  // wait for this step's fragments before the next reads go out
        __builtin_amdgcn_sched_barrier(0);
        u32x4 xb0 = xa0, xb1 = xa1;
        u32x4 wb[NT];
        if (j + 1 < 4) {
          const int cx = 2 * (j + 1) + h;
          xb0 = *reinterpret_cast<const u32x4*>(xrow0 + ((cx ^ xs) * 16));
          xb1 = *reinterpret_cast<const u32x4*>(xrow1 + ((cx ^ xs) * 16));
          const int c = c0 + 2 * (j + 1);
#pragma unroll
          for (int tt = 0; tt < NT; ++tt)
            wb[tt] = *reinterpret_cast<const u32x4*>(img + tt * 16 * WROW + ((c ^ wsw) * 16));
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
          acc[0][tt] = mfma_chunk(T{}, wa[tt], xa0, acc[0][tt]);
          acc[1][tt] = mfma_chunk(T{}, wa[tt], xa1, acc[1][tt]);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (j + 1 < 4) {
          xa0 = xb0;
          xa1 = xb1;
#pragma unroll
          for (int tt = 0; tt < NT; ++tt) wa[tt] = wb[tt];
        }
      }
    }
    // 32 stores, always: row r of the wave goes to row min(r, last) (rows behind the end hold the last row's result)
    const T* bp = cur.bias ? reinterpret_cast<const T*>(cur.bias) + (MC / 2) * h : nullptr;
    char* obase = cur.c + cur.first * MC * SZ;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
      for (int rd = 0; rd < 2; ++rd) {  // column blocks 4 rd .. 4 rd + 3 of both lane halves
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const int tt = 4 * rd + q4;
          float v[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) v[r] = acc[rb][tt][r];
          if (bp) {
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = round_to(T{}, v[r]) + load_bias(bp + 16 * tt + r);
          }
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int c = 8 * h + 2 * q4 + j;  // 16 chunks per stage row: [half 0: 8 chunks | half 1: 8 chunks]
            *reinterpret_cast<u32x4*>(stage + (x * 16 + (c ^ (x & 15))) * 16) = pack_chunk(T{}, v + 8 * j);
          }
        }
        u32x4 ov[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) ov[i] = *reinterpret_cast<const u32x4*>(stage + (i * 64 + lane) * 16);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int p = i * 64 + lane;
          const int r = p >> 4;
          const int c = (p & 15) ^ (r & 15);
          int ro = 32 * rb + r;
          ro = ro > cur.last ? cur.last : ro;
          GU32x4* dst = (GU32x4*)(obase + (uint32_t)(ro * MC * SZ + ((MC / 2) * (c >> 3) + 64 * rd + 8 * (c & 7)) * SZ));
          __builtin_nontemporal_store(ov[i], dst);
        }
      }
    }
    cur = nx;
  };

  plan(0);
  cur = nx;
  load_q(0, cur, 0);
  load_q(1, cur, 1);
  tile_body(0);  // peeled: inside the loop the memory operations in flight are the same on entry and on the back edge
  for (int t = 1; t < t1; ++t) tile_body(t);
}

constexpr int kWideLds = 2 * 256 * 256 + 4 * 32 * 256;  // 128 KB weights + 4 x 8 KB stages = 160 KB

template <typename T>
int launch_wide(const DevGroup* descs, const int32_t* tile_start, int B, int64_t tiles_upper, int M, hipStream_t stream) {
  constexpr int NW = 4;
  if (int rc_ = ensure_dynamic_lds(reinterpret_cast<const void*>(&mfma_rows_wide256_kernel<T, NW>), kWideLds)) return rc_;
  const int ncol = M / 256;
  hipLaunchKernelGGL((mfma_rows_wide256_kernel<T, NW>), dim3(tile_grid(tiles_upper, 1, ncol)), dim3(NW * 64), kWideLds, stream,
                     descs, tile_start, B, /*chunk=*/0, ncol);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

template <typename T>
int launch_wide_r2(const DevGroup* descs, const int32_t* tile_start2, int B, int64_t tiles2_upper, hipStream_t stream) {
  if (int rc_ = ensure_dynamic_lds(reinterpret_cast<const void*>(&mfma_rows_wide256r2_kernel<T>), kWideLds)) return rc_;
  hipLaunchKernelGGL((mfma_rows_wide256r2_kernel<T>), dim3(tile_grid(tiles2_upper, 1)), dim3(256), kWideLds, stream, descs,
                     tile_start2, B);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

}  // namespace

int launch_k256_wide(int dtype, const void* descs, const int32_t* tile_start, int B, int64_t tiles_upper, int M,
                     hipStream_t stream) {
  const DevGroup* d = static_cast<const DevGroup*>(descs);
  return dtype == PYG_BF16 ? launch_wide<bf16_t>(d, tile_start, B, tiles_upper, M, stream)
                           : launch_wide<f16_t>(d, tile_start, B, tiles_upper, M, stream);
}

int launch_k256_wide_r2(int dtype, const void* descs, const int32_t* tile_start2, int B, int64_t tiles2_upper,
                        hipStream_t stream) {
  const DevGroup* d = static_cast<const DevGroup*>(descs);
  return dtype == PYG_BF16 ? launch_wide_r2<bf16_t>(d, tile_start2, B, tiles2_upper, stream)
                           : launch_wide_r2<f16_t>(d, tile_start2, B, tiles2_upper, stream);
}

}  // namespace pyg_hip
