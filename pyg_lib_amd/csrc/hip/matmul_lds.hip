// LDS-weight kernels of segment_matmul / grouped_matmul: a relation's W^T is staged into LDS as [MC][K], a workgroup
// walks one contiguous range of 128-row tiles (four waves of 32 rows) and re-stages W when it crosses a relation
// boundary.  Every wave owns 32 rows x MC output columns:
//   * X rows go HBM -> VGPR as 16-byte loads; lane (x, h) owns the contiguous half-row
//     X[row x][h*K/2 .. (h+1)*K/2) -- the contraction index is permuted between MFMA k-slots so
//     that each lane's fragments are contiguous in memory (k = h*K/2 + 8*s + e for step s).
//   * W^T lives in LDS as [MC][K] (+16 B row pad => conflict-free ds_read_b128) and is the MFMA
//     "A" operand, X is the "B" operand, so D = W^T X^T: lane (x, h) ends up with
//     out[row x][h*MC/2 .. (h+1)*MC/2) -- again contiguous, stored as 16-byte writes.  The
//     output-column permutation that makes this true is folded into the LDS row a lane reads.
//   * v_mfma_f32_32x32x16_{bf16,f16} with fp32 accumulation and one rounding at the store for
//     16-bit types; v_mfma_f32_32x32x2_f32 (exact fp32 FMA chain) for fp32 -- gfx950 has no TF32.
// mfma_rows_kernel reads its X fragments straight from HBM (what remains for shapes whose W image leaves no room for
// stages), mfma_rows_lds_kernel moves X and the output through per-wave LDS stages as fully coalesced accesses; its
// X3 form is fp32 K = MC = 128 in split-bf16 arithmetic.  Tile tables and the route choice: matmul.hip.
#include "matmul_common.h"

#include <algorithm>
#include <type_traits>

namespace pyg_hip {
namespace {

// K: contraction length (compile time), MC: output columns per workgroup pass (grid.y walks
// M / MC column chunks), NW: waves per workgroup (tile = NW * 32 rows).
template <typename T, int K, int MC, int NW>
__global__ __launch_bounds__(NW * 64) void mfma_rows_kernel(const DevGroup* __restrict__ descs,
                                                            const int32_t* __restrict__ tile_start,
                                                            int B, int ncol) {
  constexpr int SZ = Elem<T>::kSize;
  constexpr int EPC = Elem<T>::kPerChunk;
  constexpr int NCH = (K / 2) / EPC;           // 16-byte chunks per lane (half row)
  constexpr int NT = MC / 32;                  // 32-column MFMA tiles per wave
  constexpr int LDW = K * SZ + 16;             // LDS row stride (bytes) of the W^T image
  constexpr int BM = NW * 32;
  static_assert(BM == kTileRows, "tile table is built for 128-row tiles");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int x = lane & 31;
  const int h = lane >> 5;
  const int bx = ncol > 1 ? ((int)blockIdx.x / (8 * ncol)) * 8 + ((int)blockIdx.x & 7) : (int)blockIdx.x;
  const int by = ncol > 1 ? ((int)blockIdx.x / 8) % ncol : 0;
  const int col0 = by * MC;

  const int total = tile_start[B];
  const int G = (int)gridDim.x / ncol;
  const int t0 = (int)((int64_t)bx * total / G);
  const int t1 = (int)((int64_t)(bx + 1) * total / G);
  if (t0 >= t1) return;

  // group of the first tile: largest g with tile_start[g] <= t0
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile_start[mid] <= t0) lo = mid; else hi = mid;
  }
  int g = lo;
  int staged = -1;

  // LDS row (output column within the chunk) whose fragment this lane reads for tile t:
  // c(t, x) = (MC/2)*bit2(x) + 16 t + 4*(x>>3) + (x&3)   (see header comment)
  const int crow0 = (MC / 2) * ((x >> 2) & 1) + 4 * (x >> 3) + (x & 3);
  const char* wfrag = smem + crow0 * LDW + (K / 2) * h * SZ;

  DevGroup d = descs[g];
  for (int t = t0; t < t1; ++t) {
    while (t >= tile_start[g + 1]) {
      ++g;
      d = descs[g];
    }
    if (g != staged) {
      __syncthreads();  // every wave is done reading the previous relation's weight
      const char* w = d.w;
      const int M = d.m;
      if (!d.trans) {
        // W is [K][M]: read 16-byte pieces along M, scatter transposed into the [MC][K] image.
        constexpr int CPR = MC / EPC;  // chunks per W row (within the column chunk)
        for (int idx = tid; idx < K * CPR; idx += NW * 64) {
          const int k = idx / CPR;
          const int cc = (idx - k * CPR) * EPC;
          const u32x4 v = *reinterpret_cast<const u32x4*>(w + ((int64_t)k * M + col0 + cc) * SZ);
          if constexpr (SZ == 2) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const uint16_t s = (uint16_t)(v[e >> 1] >> ((e & 1) * 16));
              *reinterpret_cast<uint16_t*>(smem + (cc + e) * LDW + k * 2) = s;
            }
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              *reinterpret_cast<uint32_t*>(smem + (cc + e) * LDW + k * 4) = v[e];
          }
        }
      } else {
        // W is stored [M][K] (transposed view): straight 16-byte copies.
        constexpr int CPR = K / EPC;
        for (int idx = tid; idx < MC * CPR; idx += NW * 64) {
          const int c = idx / CPR;
          const int kk = (idx - c * CPR) * EPC;
          const u32x4 v =
              *reinterpret_cast<const u32x4*>(w + ((int64_t)(col0 + c) * K + kk) * SZ);
          *reinterpret_cast<u32x4*>(smem + c * LDW + kk * SZ) = v;
        }
      }
      __syncthreads();
      staged = g;
    }

    const int64_t rows = d.rows;
    const int64_t row_base = (int64_t)(t - tile_start[g]) * BM + wave * 32;
    if (row_base >= rows) continue;  // wave-uniform: ragged last tile of a segment
    const int64_t row = row_base + x;
    const bool valid = row < rows;
    const int64_t lrow = valid ? row : rows - 1;

    // ---- X: lane's contiguous half row, HBM -> VGPR ----
    u32x4 xv[NCH];
    const u32x4* xp =
        reinterpret_cast<const u32x4*>(d.a + (lrow * K + (K / 2) * h) * SZ);
#pragma unroll
    for (int i = 0; i < NCH; ++i) xv[i] = __builtin_nontemporal_load(xp + i);

    f32x16 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

#pragma unroll
    for (int s = 0; s < NCH; ++s) {
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        const u32x4 wv = *reinterpret_cast<const u32x4*>(wfrag + tt * 16 * LDW + s * 16);
        acc[tt] = mfma_chunk(T{}, wv, xv[s], acc[tt]);
      }
    }

    // ---- epilogue: lane (x, h) owns out[row][col0 + h*MC/2 + 16 tt + r] ----
    if (valid) {
      const int M = d.m;
      char* op = d.c + (row * M + col0 + (MC / 2) * h) * SZ;
      const T* bp = d.bias ? reinterpret_cast<const T*>(d.bias) + col0 + (MC / 2) * h : nullptr;
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        float v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = acc[tt][r];
        if (bp) {
          // reference semantics (pyg_lib/ops/__init__.py:169-171): `out` is materialised in T
          // first, then `out += bias` -- so round the product before adding for 16-bit types.
#pragma unroll
          for (int r = 0; r < 16; ++r)
            v[r] = round_to(T{}, v[r]) + load_bias(bp + 16 * tt + r);
        }
        store16((T*)nullptr, op + tt * 16 * SZ, v);
      }
    }
  }
}

// ---- v2: LDS-staged streaming kernel for 16-bit types (the HBM-bound configs) ---------------------
// Same tile walk and MFMA mapping as mfma_rows_kernel, but X and the output move between HBM and
// registers as fully coalesced 1 KiB wave accesses (every instruction covers whole 256-byte rows)
// and are re-shaped into / out of MFMA fragment order through a per-wave LDS stage with a 16-byte
// XOR swizzle (conflict-free ds_read_b128 / ds_write_b128).  The next tile's rows are prefetched
// into registers while the current tile is multiplied (issue-early / write-late).
template <typename T, int K, int MC, int NW, bool X3 = false>
__global__ __launch_bounds__(NW * 64) void mfma_rows_lds_kernel(
    const DevGroup* __restrict__ descs, const int32_t* __restrict__ tile_start, int B, int chunk, int ncol) {
  // X3 (fp32 only): split-bf16 arithmetic -- x = hi + mid + lo with 8 significant bits each (24 in all), W alike;
  // (round to nearest at every split, so |mid| <= 2^-9 |x|, |lo| <= 2^-18 |x| and the residual left is <= 2^-27 |x|);
  // the six products of weight 2^0, 2^-9, 2^-9, 2^-18, 2^-18, 2^-18 go through v_mfma_f32_32x32x16_bf16 with fp32
  // accumulation (the two of weight 2^-27 and the one of 2^-36 are dropped: 1.5e-8 of |x||w| per product, unbiased --
  // a quarter of the fp32 rounding unit, so the result is as close to the exact product as the fp32 MFMA's).
  // Six 32-cycle MFMAs per 16 k instead of eight 64-cycle v_mfma_f32_32x32x2_f32: 2.7x less matrix time, which makes
  // fp32 F = 128 (AI = 32 flop/B) HBM-bound instead of bound by the fp32 matrix rate.  W^T lives in LDS as three
  // bf16 planes [MC][K] (16-byte chunks XOR-swizzled with the row, no pad: 3 x 32 KB + 4 x 16 KB of stages = 160 KB).
  static_assert(!X3 || (std::is_same<T, float>::value && K == 128 && MC == 128), "split-bf16: fp32, K = MC = 128");
  constexpr int SZ = Elem<T>::kSize;
  constexpr int EPC = Elem<T>::kPerChunk;  // elements per 16-byte chunk
  constexpr int NT = MC / 32;
  constexpr int LDW = K * SZ + 16;
  constexpr int BM = NW * 32;
  static_assert(BM == kTileRows, "tile table is built for 128-row tiles");
  constexpr int CPR = K * SZ / 16;              // 16-byte chunks per X row
  constexpr int NI = CPR / 2;                   // coalesced wave loads per 32-row tile
  constexpr int XM = (CPR < 16 ? CPR : 16) - 1; // swizzle mask
  constexpr int CPO = MC * SZ / 16;             // chunks per output row (this column chunk)
  constexpr int NO = CPO / 2;
  constexpr int OM = (CPO < 16 ? CPO : 16) - 1;
  constexpr int STAGE = 32 * 16 * (CPR > CPO ? CPR : CPO);  // bytes per wave
  constexpr int PLANE = MC * K * 2;  // X3: one bf16 plane of W^T
  constexpr int WBYTES = X3 ? 3 * PLANE : MC * LDW;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int x = lane & 31;
  const int h = lane >> 5;
  // XCD-aware workgroup decode (1-D grid of G * ncol workgroups): consecutive workgroup ids go to
  // consecutive XCDs, so the `ncol` column-chunk workgroups of one tile range get ids 8 apart -- same
  // XCD, same L2 -- and the X tiles they both read come from HBM once.
  const int bx = ncol > 1 ? ((int)blockIdx.x / (8 * ncol)) * 8 + ((int)blockIdx.x & 7) : (int)blockIdx.x;
  const int by = ncol > 1 ? ((int)blockIdx.x / 8) % ncol : 0;
  const int col0 = by * MC;
  char* stage = smem + WBYTES + wave * STAGE;

  // Tile schedule: workgroup b owns the tile chunks b, b + G, b + 2G, ... of `chunk` consecutive
  // tiles each (chunk <= 0: one contiguous range per workgroup).  Local tile i of this workgroup is
  // global tile tile_of(i).
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
      const int last_chunk = (mine - 1) * G + bx;  // may be the ragged final chunk
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
  const int t0 = 0, t1 = nloc;  // local tile indices

  int lo = 0, hi = B;
  {
    const int first = tile_of(0);
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (tile_start[mid] <= first) lo = mid; else hi = mid;
    }
  }
  int g = lo;       // group of the tile being prefetched
  int staged = -1;  // group whose weight is in LDS

  const int crow0 = (MC / 2) * ((x >> 2) & 1) + 4 * (x >> 3) + (x & 3);
  const char* wfrag = X3 ? smem + crow0 * (K * 2) : smem + crow0 * LDW + (K / 2) * h * SZ;

  // per-lane constants of the coalesced <-> fragment re-shaping
  // load/store side: position p = i*64 + lane -> row r = p / CPR, slot c' = p % CPR
  // fragment side:   lane (x, h) reads row x, chunk c at slot c ^ (x & XM)
  u32x4 xr[NI];
  uint32_t xoff[8];  // X3: byte offset of this lane's 16 bytes of load i (< 8) inside a whole 32-row tile
  if constexpr (X3) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int p = i * 64 + lane;
      const int r = p / CPR;
      xoff[i] = (uint32_t)(r * (K * SZ) + (((p % CPR) ^ (r & XM)) * 16));
    }
  }
  DevGroup dn = descs[g];
  int64_t n_row0 = 0, n_rows = 0;
  bool n_valid = false;

  auto prefetch = [&](int ti) {
    const int t = tile_of(ti);
    while (t >= tile_start[g + 1]) {
      ++g;
      dn = descs[g];
    }
    n_rows = dn.rows;
    n_row0 = (int64_t)(t - tile_start[g]) * BM + wave * 32;
    n_valid = n_row0 < n_rows;
    if (X3 && n_valid && n_row0 + 32 <= n_rows) {
      // whole tile: tile base + per-lane offsets computed once (loads i and i + 8 lie 16 rows = 8 KiB apart)
      const char* base = dn.a + n_row0 * (K * SZ);
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        typedef __attribute__((address_space(1))) u32x4 GU32x4;
        const GU32x4* src = (const GU32x4*)(base + xoff[i & 7] + (i >> 3) * 8192);
        if (ncol == 1) asm volatile("global_load_dwordx4 %0, %1, off nt" : "=a"(xr[i]) : "v"(src) : "memory");
        else asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(xr[i]) : "v"(src) : "memory");
      }
    } else if (n_valid) {
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int p = i * 64 + lane;
        const int r = p / CPR;
        const int cs = p % CPR;
        const int c = cs ^ (r & XM);
        int64_t row = n_row0 + r;
        if (row >= n_rows) row = n_rows - 1;
        // global_* (a flat access also counts on lgkmcnt and makes every LDS wait conservative)
        typedef __attribute__((address_space(1))) u32x4 GU32x4;
        const GU32x4* src = (const GU32x4*)(dn.a + row * (K * SZ) + c * 16);
        // with several column-chunk readers the tile must STAY in L2 for the others: no streaming hint (with it
        // C4's X came from HBM 1.86 times, PMC FETCH_SIZE; without it 1.01 times)
        if constexpr (X3) {
          // through inline asm: the wait is placed by hand (x3_wait) -- the compiler cannot count the stores that were
          // issued after these loads across the loop's branches and would wait for them too (vmcnt retires in order)
          // (into AGPRs: the one wave per SIMD has 192 of them idle, and a value the compiler believes defined must
          // not be moved before its load has landed -- under VGPR pressure it would be)
          if (ncol == 1) asm volatile("global_load_dwordx4 %0, %1, off nt" : "=a"(xr[i]) : "v"(src) : "memory");
          else asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(xr[i]) : "v"(src) : "memory");
        } else {
          xr[i] = ncol == 1 ? __builtin_nontemporal_load(src) : *src;
        }
      }
    }
  };

  // Software pipeline (per wave; the stage buffer is private to the wave):
  //   loop top: X_t is in the LDS stage, L_{t+1} (next tile's rows) is in flight into xr.
  //   1. multiply X_t by W (MFMA, fragments double-buffered in registers)
  //   2. pack the result, swizzle it through the stage, read it back in row order (ov)
  //   3. wait for L_{t+1} (issued a whole tile ago, as were the stores S_{t-1} ahead of it in the
  //      in-order memory queue), write it to the stage
  //   4. issue L_{t+2}, then the global stores S_t
  // so no wave ever waits on a store it has just issued.
  prefetch(t0);
  DevGroup d = dn;
  int cg = g;
  int64_t row0 = n_row0, rows = n_rows;
  bool valid = n_valid;
  // X3: `stores_younger` = exactly the NO unpredicated stores of a whole tile were issued after the loads now awaited
  bool stores_younger = false;
  auto x3_wait = [&]() {
    if constexpr (X3) {
      static_assert(!X3 || NO == 16, "the hand-placed wait counts the 16 stores of a 32 x 128 fp32 tile");
      if (stores_younger) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  };
  x3_wait();
  if (valid) {
#pragma unroll
    for (int i = 0; i < NI; ++i) *reinterpret_cast<u32x4*>(stage + (i * 64 + lane) * 16) = xr[i];
  }
  if (t0 + 1 < t1) prefetch(t0 + 1);

  for (int t = t0; t < t1; ++t) {
    if (cg != staged) {
      __syncthreads();
      const char* w = d.w;
      const int M = d.m;
      if constexpr (X3) {
        // fp32 W[k][m] (or W^T[m][k]) -> three bf16 planes [m][k]: element (m, k) at plane + m * 256 + (((k >> 3) ^ (m & 15)) * 16)
        // + (k & 7) * 2
        constexpr int CW = 32;  // 16-byte chunks per source row (K = MC = 128 floats)
        for (int idx = tid; idx < 128 * CW; idx += NW * 64) {
          const int r = idx / CW;
          const int c4 = (idx - r * CW) * 4;
          const int64_t src = !d.trans ? ((int64_t)r * M + col0 + c4) : ((int64_t)(col0 + r) * K + c4);
          // (whole-vector bit_cast: __builtin_bit_cast(float, v[e]) on a vector element reads element 0, clang 19)
          const f32x4 v = __builtin_bit_cast(f32x4, *reinterpret_cast<const u32x4*>(w + src * 4));
#pragma unroll
          for (int e = 0; e < 4; e += 2) {
            float f0 = v[e], f1 = v[e + 1];
            const uint32_t ph = split2(f0, f1);
            const uint32_t pm = split2(f0, f1);
            const uint32_t pl = split2(f0, f1);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
              const int k = !d.trans ? r : c4 + e + u;
              const int mm = !d.trans ? c4 + e + u : r;
              char* dst = smem + mm * (K * 2) + (((k >> 3) ^ (mm & 15)) * 16) + (k & 7) * 2;
              *reinterpret_cast<uint16_t*>(dst) = (uint16_t)(ph >> (16 * u));
              *reinterpret_cast<uint16_t*>(dst + PLANE) = (uint16_t)(pm >> (16 * u));
              *reinterpret_cast<uint16_t*>(dst + 2 * PLANE) = (uint16_t)(pl >> (16 * u));
            }
          }
        }
      } else if (!d.trans) {
        constexpr int CW = MC / EPC;
        for (int idx = tid; idx < K * CW; idx += NW * 64) {
          const int k = idx / CW;
          const int cc = (idx - k * CW) * EPC;
          const u32x4 v = *reinterpret_cast<const u32x4*>(w + ((int64_t)k * M + col0 + cc) * SZ);
          if constexpr (SZ == 2) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const uint16_t sv = (uint16_t)(v[e >> 1] >> ((e & 1) * 16));
              *reinterpret_cast<uint16_t*>(smem + (cc + e) * LDW + k * 2) = sv;
            }
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const uint32_t sv = v[e];
              *reinterpret_cast<uint32_t*>(smem + (cc + e) * LDW + k * 4) = sv;
            }
          }
        }
      } else {
        constexpr int CW = K / EPC;
        for (int idx = tid; idx < MC * CW; idx += NW * 64) {
          const int c = idx / CW;
          const int kk = (idx - c * CW) * EPC;
          const u32x4 v =
              *reinterpret_cast<const u32x4*>(w + ((int64_t)(col0 + c) * K + kk) * SZ);
          *reinterpret_cast<u32x4*>(smem + c * LDW + kk * SZ) = v;
        }
      }
      __syncthreads();
      staged = cg;
    }

    u32x4 ov[NO];
    if (valid) {
      f32x16 acc[NT];
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

      if constexpr (X3) {
        // 16 units of 12 MFMAs: unit u = (K-step s = u >> 1, column blocks 2 (u & 1), +1).  The W fragments of unit u + 1
        // and (even units) the X chunks of step s + 1 are read from LDS while unit u's MFMAs run; odd units also split
        // those X chunks.  One wave per SIMD: nothing else hides an LDS round trip.
        const int wsw = crow0 & 15;  // rows crow0 + 16 tt share it
        const char* xrow = stage + x * (CPR * 16);
        const int xs = x & XM;
        u32x4 wq[2][6], qx[2], xf[2][3];
        auto read_w = [&](int u, u32x4 (&wv)[6]) {
          const int s8 = u >> 1;
          const char* wr = wfrag + (2 * (u & 1)) * 16 * (K * 2) + (((8 * h + s8) ^ wsw) * 16);
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) wv[3 * j + pl] = *reinterpret_cast<const u32x4*>(wr + j * 16 * (K * 2) + pl * PLANE);
        };
        auto read_x = [&](int s8) {
          // lane (x, h): k = 64 h + 8 s8 + e, e = 0 ... 7: two 16-byte fp32 chunks of its half row
          const int c = NI * h + 2 * s8;
          qx[0] = *reinterpret_cast<const u32x4*>(xrow + ((c ^ xs) * 16));
          qx[1] = *reinterpret_cast<const u32x4*>(xrow + (((c + 1) ^ xs) * 16));
        };
        auto split_x = [&](u32x4 (&o)[3]) {
          const f32x4 f0 = __builtin_bit_cast(f32x4, qx[0]), f1 = __builtin_bit_cast(f32x4, qx[1]);
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            float a = p < 2 ? f0[2 * p] : f1[2 * p - 4];
            float b2 = p < 2 ? f0[2 * p + 1] : f1[2 * p - 3];
            o[0][p] = split2(a, b2);
            o[1][p] = split2(a, b2);
            o[2][p] = split2(a, b2);
          }
        };
        read_x(0);
        read_w(0, wq[0]);
        split_x(xf[0]);
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int s8 = u >> 1;
          // this unit's fragments were issued a unit ago: wait for them here, not (with the reads below) at the MFMAs
          asm volatile("" : "+v"(wq[u & 1][5]));
          __builtin_amdgcn_sched_barrier(0);
          if (u + 1 < 16) read_w(u + 1, wq[(u + 1) & 1]);
          if ((u & 1) == 0 && s8 + 1 < 8) read_x(s8 + 1);
          __builtin_amdgcn_sched_barrier(0);
          const u32x4(&xv)[3] = xf[s8 & 1];
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int tt = 2 * (u & 1) + j;
            const u32x4 wh = wq[u & 1][3 * j], wm = wq[u & 1][3 * j + 1], wl = wq[u & 1][3 * j + 2];
            // smallest terms first
            acc[tt] = mfma_chunk(bf16_t{}, wl, xv[0], acc[tt]);
            acc[tt] = mfma_chunk(bf16_t{}, wh, xv[2], acc[tt]);
            acc[tt] = mfma_chunk(bf16_t{}, wm, xv[1], acc[tt]);
            acc[tt] = mfma_chunk(bf16_t{}, wm, xv[0], acc[tt]);
            acc[tt] = mfma_chunk(bf16_t{}, wh, xv[1], acc[tt]);
            acc[tt] = mfma_chunk(bf16_t{}, wh, xv[0], acc[tt]);
          }
          if ((u & 1) == 1 && s8 + 1 < 8) split_x(xf[(s8 + 1) & 1]);
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
      // fragments of step s+1 are read from LDS while the MFMAs of step s run
      u32x4 xa = *reinterpret_cast<const u32x4*>(stage + (x * CPR + ((NI * h) ^ (x & XM))) * 16);
      u32x4 wa[NT];
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) wa[tt] = *reinterpret_cast<const u32x4*>(wfrag + tt * 16 * LDW);
#pragma unroll
      for (int s = 0; s < NI; ++s) {
        // wait for this step's fragments (issued a whole step ago) before the next step's reads go out:
        // otherwise the compiler's wait in front of the MFMAs is an lgkmcnt(0) that covers those too
        asm volatile("" : "+v"(wa[NT - 1]));
        __builtin_amdgcn_sched_barrier(0);
        u32x4 xb = xa;
        u32x4 wb[NT];
        if (s + 1 < NI) {
          const int c = NI * h + s + 1;
          xb = *reinterpret_cast<const u32x4*>(stage + (x * CPR + (c ^ (x & XM))) * 16);
#pragma unroll
          for (int tt = 0; tt < NT; ++tt)
            wb[tt] = *reinterpret_cast<const u32x4*>(wfrag + tt * 16 * LDW + (s + 1) * 16);
        }
        // keep the order "issue the next step's LDS reads, then this step's MFMAs": left alone, the
        // scheduler sinks every ds_read to just before its MFMA (lgkmcnt(0) x32 per tile)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (SZ == 4) {
          // fp32: a 16-byte chunk feeds four 32x32x2 MFMAs per column block; interleave the column blocks
          // so that back-to-back MFMAs never wait on each other's accumulator
          const f32x4 xf = __builtin_bit_cast(f32x4, xa);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int tt = 0; tt < NT; ++tt)
              acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(__builtin_bit_cast(f32x4, wa[tt])[e], xf[e], acc[tt], 0, 0, 0);
        } else {
#pragma unroll
          for (int tt = 0; tt < NT; ++tt) acc[tt] = mfma_chunk(T{}, wa[tt], xa, acc[tt]);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (s + 1 < NI) {
          xa = xb;
#pragma unroll
          for (int tt = 0; tt < NT; ++tt) wa[tt] = wb[tt];
        }
      }

      }  // !X3
      // epilogue: fragment order -> swizzled stage -> row order (ov)
      const T* bp = d.bias ? reinterpret_cast<const T*>(d.bias) + col0 + (MC / 2) * h : nullptr;
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
        for (int j = 0; j < SZ; ++j) {  // 16 values = SZ chunks of EPC elements
          const int c = NO * h + SZ * tt + j;
          *reinterpret_cast<u32x4*>(stage + (x * CPO + (c ^ (x & OM))) * 16) = pack_chunk(T{}, v + EPC * j);
        }
      }
#pragma unroll
      for (int i = 0; i < NO; ++i) ov[i] = *reinterpret_cast<const u32x4*>(stage + (i * 64 + lane) * 16);
    }

    // stage the next tile (its loads were issued one tile ago) and issue the loads after it
    const DevGroup d_out = d;
    const int64_t row0_out = row0, rows_out = rows;
    const bool valid_out = valid;
    if (t + 1 < t1) {
      d = dn;
      cg = g;
      row0 = n_row0;
      rows = n_rows;
      valid = n_valid;
      x3_wait();
      if (valid) {
#pragma unroll
        for (int i = 0; i < NI; ++i) *reinterpret_cast<u32x4*>(stage + (i * 64 + lane) * 16) = xr[i];
      }
      if (t + 2 < t1) prefetch(t + 2);
    }
    stores_younger = false;

    if (X3 && valid_out && row0_out + 32 <= rows_out) {
      // whole tile: NO unpredicated stores, which the next x3_wait leaves in flight
      const int M = d_out.m;
      char* obase = d_out.c + (row0_out * M + col0) * SZ;
#pragma unroll
      for (int i = 0; i < NO; ++i) {
        const int p = i * 64 + lane;
        const int r = p / CPO;
        const int c = (p % CPO) ^ (r & OM);
        typedef __attribute__((address_space(1))) u32x4 GU32x4;
        GU32x4* dst = (GU32x4*)(obase + (int64_t)r * M * SZ + c * 16);
        __builtin_nontemporal_store(ov[i], dst);
      }
      stores_younger = true;
    } else if (valid_out) {
      const int M = d_out.m;
      char* obase = d_out.c + (row0_out * M + col0) * SZ;
#pragma unroll
      for (int i = 0; i < NO; ++i) {
        const int p = i * 64 + lane;
        const int r = p / CPO;
        const int cs = p % CPO;
        const int c = cs ^ (r & OM);
        if (row0_out + r < rows_out) {
          typedef __attribute__((address_space(1))) u32x4 GU32x4;
          GU32x4* dst = (GU32x4*)(obase + (int64_t)r * M * SZ + c * 16);
          __builtin_nontemporal_store(ov[i], dst);
        }
      }
    }
  }
}

template <typename T, int K, int MC>
int launch(const DevGroup* descs, const int32_t* tile_start, int B, int64_t tiles_upper, int M, hipStream_t stream) {
  constexpr int NW = 4;
  constexpr int SZ = Elem<T>::kSize;
  constexpr int wbytes = MC * (K * SZ + 16);
  constexpr int stage = 32 * (K > MC ? K : MC) * SZ;
  constexpr int lds_v2 = wbytes + NW * stage;
  // Everything that fits streams through the LDS-staged kernel (fully coalesced HBM access); the
  // direct-fragment kernel remains for the shapes whose weight image + stages exceed 160 KB of LDS.
  constexpr bool use_v2 = lds_v2 <= 160 * 1024;
  constexpr int lds = use_v2 ? lds_v2 : wbytes;
  const int per_cu = std::max(1, std::min(use_v2 ? 2 : 4, (160 * 1024) / lds));
  const int ncol = M / MC;
  const unsigned grid = tile_grid(tiles_upper, per_cu, ncol);
  if constexpr (use_v2) {
    if (int rc_ = ensure_dynamic_lds(reinterpret_cast<const void*>(&mfma_rows_lds_kernel<T, K, MC, NW>), lds)) return rc_;
    hipLaunchKernelGGL((mfma_rows_lds_kernel<T, K, MC, NW>), dim3(grid), dim3(NW * 64), lds, stream, descs, tile_start, B,
                       /*chunk=*/0, ncol);
  } else {
    if (int rc_ = ensure_dynamic_lds(reinterpret_cast<const void*>(&mfma_rows_kernel<T, K, MC, NW>), lds)) return rc_;
    hipLaunchKernelGGL((mfma_rows_kernel<T, K, MC, NW>), dim3(grid), dim3(NW * 64), lds, stream, descs, tile_start, B, ncol);
  }
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

// The instantiation list: every (K, MC) the route choice of matmul.hip can name for this family.
template <typename T>
int launch_any(int K, int MC, const DevGroup* descs, const int32_t* tile_start, int B, int64_t tiles_upper, int M,
               hipStream_t stream) {
#define PYG_CASE(KK, MM) \
  if (K == KK && MC == MM) return launch<T, KK, MM>(descs, tile_start, B, tiles_upper, M, stream);
  if constexpr (Elem<T>::kSize == 2) {  // (fp32 K = 128 is matmul_f32_pipe.hip's and the X3 form's)
    PYG_CASE(128, 32) PYG_CASE(128, 64) PYG_CASE(128, 128) PYG_CASE(128, 256)
  }
  PYG_CASE(32, 32) PYG_CASE(32, 64) PYG_CASE(32, 128)
  PYG_CASE(64, 32) PYG_CASE(64, 64) PYG_CASE(64, 128)
  PYG_CASE(256, 32) PYG_CASE(256, 64) PYG_CASE(256, 128)
  PYG_CASE(512, 32) PYG_CASE(512, 64)
#undef PYG_CASE
  return fail(PYG_HIP_ERR_INVALID, "matmul: no LDS-weight kernel for K = %d with %d-column chunks", K, MC);
}

}  // namespace

int launch_lds(int dtype, int K, int MC, const void* descs, const int32_t* tile_start, int B, int64_t tiles_upper, int M,
               hipStream_t stream) {
  const DevGroup* d = static_cast<const DevGroup*>(descs);
  if (dtype == PYG_BF16) return launch_any<bf16_t>(K, MC, d, tile_start, B, tiles_upper, M, stream);
  if (dtype == PYG_F16) return launch_any<f16_t>(K, MC, d, tile_start, B, tiles_upper, M, stream);
  return launch_any<float>(K, MC, d, tile_start, B, tiles_upper, M, stream);
}

int launch_lds_f32x3(const void* descs, const int32_t* tile_start, int B, int64_t tiles_upper, int M, hipStream_t stream) {
  constexpr int NW = 4;
  constexpr int lds = 3 * 128 * 128 * 2 + NW * 32 * 128 * 4;  // 96 KB of W planes + 4 x 16 KB stages = 160 KB
  if (int rc_ = ensure_dynamic_lds(reinterpret_cast<const void*>(&mfma_rows_lds_kernel<float, 128, 128, NW, true>), lds))
    return rc_;
  const int ncol = M / 128;
  hipLaunchKernelGGL((mfma_rows_lds_kernel<float, 128, 128, NW, true>), dim3(tile_grid(tiles_upper, 1, ncol)), dim3(NW * 64),
                     lds, stream, static_cast<const DevGroup*>(descs), tile_start, B, /*chunk=*/0, ncol);
  PYG_HIP_CHECK(hipGetLastError());
  return PYG_HIP_OK;
}

}  // namespace pyg_hip
