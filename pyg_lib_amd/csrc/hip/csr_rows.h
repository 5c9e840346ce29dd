// What the CSR-row kernel families share (csr.hip, fused_reduce.hip): the 16-byte pack, pin_all, the accumulator identities
// and shuffles, the scratch of the hub rows (registration, layout) and the choice of the row kernel (lanes per row).
#pragma once

#include "common.h"
#include "elem.h"

#include <algorithm>
#include <cstdint>
#include <type_traits>

namespace pyg_hip {
namespace {

template <typename T, int V>
struct alignas(sizeof(T) * V) Pack {
  T v[V];
};

// pin_all(a): every element of `a` is needed HERE, all of them at once.  The row kernels load U positions' values "in flight
// together" and then use them under `if (position < end)`; the compiler sinks each load to its conditional use, and the
// kernel runs with ONE load in flight per thread (load, s_waitcnt vmcnt(0), branch, load, ...: the ISA of every such loop
// before this existed).  One empty asm statement that takes all U values as register operands cannot be split.
template <int BYTES> struct PinReg { using type = uint32_t; };
template <> struct PinReg<8> { using type = uint64_t; };
template <> struct PinReg<16> { typedef unsigned type __attribute__((ext_vector_type(4))); };
template <typename X, int U>
__device__ __forceinline__ void pin_all(X (&a)[U]) {
  static_assert(U == 4 || U == 8 || U == 16, "pin_all: 4, 8 or 16 values");
  if constexpr (sizeof(X) == 32) {   // two 16-byte halves each
    using Q = typename PinReg<16>::type;
    struct H { Q lo, hi; };
    Q h[2 * U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const H t = __builtin_bit_cast(H, a[u]);
      h[2 * u] = t.lo, h[2 * u + 1] = t.hi;
    }
    pin_all(h);
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] = __builtin_bit_cast(X, H{h[2 * u], h[2 * u + 1]});
    return;
  } else {
  static_assert(sizeof(X) == 1 || sizeof(X) == 2 || sizeof(X) == 4 || sizeof(X) == 8 || sizeof(X) == 16, "pin_all: value size");
  using R = typename PinReg<sizeof(X)>::type;
  R r[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if constexpr (sizeof(X) == 1) r[u] = __builtin_bit_cast(uint8_t, a[u]);
    else if constexpr (sizeof(X) == 2) r[u] = __builtin_bit_cast(uint16_t, a[u]);
    else r[u] = __builtin_bit_cast(R, a[u]);
  }
  if constexpr (U == 4) {
    asm volatile("" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]));
  } else if constexpr (U == 8) {
    asm volatile("" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]));
  } else {
    asm volatile("" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]), "+v"(r[8]),
                 "+v"(r[9]), "+v"(r[10]), "+v"(r[11]), "+v"(r[12]), "+v"(r[13]), "+v"(r[14]), "+v"(r[15]));
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if constexpr (sizeof(X) == 1) a[u] = __builtin_bit_cast(X, (uint8_t)r[u]);
    else if constexpr (sizeof(X) == 2) a[u] = __builtin_bit_cast(X, (uint16_t)r[u]);
    else a[u] = __builtin_bit_cast(X, r[u]);
  }
  }
}

// What an accumulator that has added nothing yet holds.  For floating sums that is -0, not +0: x + -0 == x for EVERY x and
// -0 + -0 == -0, whereas +0 turns a total of -0 into +0.  The reference's sequential loop has ONE accumulator per row, seeded
// with the caller's `out` slot (or the +0 of a fresh output); here a row may be split over lanes, LDS partials and chunks, and
// only the one that carries the seed may start from it -- every other starts from the identity, so that a caller's -0 plus a
// row of nothing but -0 (or no row at all) stays -0 on every path.
template <typename A>
__device__ __forceinline__ A sum_identity() {
  if constexpr (std::is_floating_point<A>::value) return A(-0.0);
  else return A(0);
}

template <typename A>
__device__ __forceinline__ A shfl_xor_any(A v, int mask) {
  static_assert(sizeof(A) % 4 == 0 || sizeof(A) < 4, "unsupported accumulator");
  if constexpr (sizeof(A) < 4) {
    int t = (int)v;
    t = __shfl_xor(t, mask);
    return (A)t;
  } else {
    A out;
    const uint32_t* s = reinterpret_cast<const uint32_t*>(&v);
    uint32_t* d = reinterpret_cast<uint32_t*>(&out);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(A) / 4); ++i) d[i] = (uint32_t)__shfl_xor((int)s[i], mask);
    return out;
  }
}

// HUB rows (more than `long_cut` positions: a destination that collects 0.25 % of 8 M positions costs 8 ms in the row
// kernels where the whole call takes 0.5 without it; power-law graphs have such nodes).  The row kernels skip them.  With
// the caller's scratch the thread that skips one REGISTERS it here, cut into chunks of `CH` positions, and a second launch
// deals the chunks to workgroups (hub_chunk kernels); without scratch a second launch finds the hubs again and gives each
// to one workgroup (the *_long kernels: ~9 GB/s per hub row).
struct HubRec {
  int64_t n;            // flat row
  int chunk_base, nch;  // its chunks: chunks[chunk_base ... chunk_base + nch)
  int slot_base, pad;   // nch > 1: its partial results' slots
};
struct HubWs {
  int* counters = nullptr;  // [0] hubs, [1] chunks, [2] partial slots -- zeroed in front of the row kernel
  HubRec* hubs = nullptr;
  int2* chunks = nullptr;   // (hub, chunk of the hub)
  char* partial = nullptr;  // slots of K accumulators ...
  int64_t* partial_best = nullptr;  // ... and, for min / max, of K positions
  int64_t CH = 0;
  int max_hubs = 0, max_chunks = 0, max_slots = 0;   // capacities: valid offsets never reach them; garbage offsets set counters[3]
};

__device__ __forceinline__ void hub_register(const HubWs& hw, int64_t n, int64_t len) {
  const int64_t nch64 = (len + hw.CH - 1) / hw.CH;
  if (nch64 > hw.max_chunks) {   // offsets that are no offsets (the reference does not check them either): nothing is written
    hw.counters[3] = 1;          // behind the scratch's ends, the hub kernels of this call stand down
    return;
  }
  const int nch = (int)nch64;
  const int h = atomicAdd(&hw.counters[0], 1);
  const int cb = atomicAdd(&hw.counters[1], nch);
  const bool slots = nch > 1 && hw.max_slots > 0;   // (gather_csr keeps no partial results)
  const int sb = slots ? atomicAdd(&hw.counters[2], nch) : 0;
  if (h >= hw.max_hubs || cb + nch > hw.max_chunks || (slots && sb + nch > hw.max_slots)) {
    hw.counters[3] = 1;
    return;
  }
  hw.hubs[h] = HubRec{n, cb, nch, sb, 0};
  for (int j = 0; j < nch; ++j) hw.chunks[cb + j] = make_int2(h, j);
}

// how the 256 threads of a hub workgroup share a row: S 16-byte slices x EL = 256 / S position lanes
template <typename T, int V>
struct HubGeom {
  int S, logS, EL, sl, lane;
  __device__ explicit HubGeom(int64_t kv) {
    S = 1, logS = 0;
    while (S < kv && S < 256) S <<= 1, ++logS;
    EL = 256 >> logS;                       // position lanes per slice
    sl = (int)threadIdx.x & (S - 1), lane = (int)threadIdx.x >> logS;
  }
};

// ---- hub scratch ------------------------------------------------------------------------------------
constexpr int64_t kHubCut = 512;      // positions per lane of the row kernels above which a row is a hub
constexpr int64_t kHubCutStream = 4096;  // ... of the LDS-streamed kernels (a thread walks its row out of LDS: ~20 us at the cut)
constexpr int64_t kHubChunk = 2048;   // positions per chunk (doubled until the scratch holds the partial results)

inline size_t hub_align(size_t b) { return (b + 255) & ~(size_t)255; }

// Where the parts of the hub scratch lie: offsets from the first 256-byte boundary of the scratch (`skew` bytes in).
struct HubLayout {
  size_t skew = 0, o_hubs = 0, o_chunks = 0, o_part = 0, o_best = 0;
  size_t bytes = 0;   // all of it, the skew included
  int64_t CH = 0, max_hubs = 0, max_chunks = 0, max_slots = 0;
};

// Lays the hub scratch out for `total` positions in rows of K values.  More than total / kHubCut hubs cannot exist; a hub
// of one chunk needs no slot, a longer one at most 2 * len / CH of them.  `sizing`: the layout of the smallest chunk length,
// whatever is offered; else the first chunk length that fits `ws_bytes` bytes at an address whose low eight bits are `ws_low`.
// False: disabled (no row can be a hub, or nothing fits).
inline bool hub_layout(int64_t total, int64_t K, size_t acc_bytes, bool minmax, bool sizing, unsigned ws_low, size_t ws_bytes,
                       HubLayout* lay) {
  if (total <= kHubCut) return false;
  lay->max_hubs = total / kHubCut + 1;
  lay->skew = sizing ? 0 : (256 - (ws_low & 255)) & 255;
  for (int64_t CH = kHubChunk; CH <= (1ll << 22); CH <<= 1) {
    lay->CH = CH;
    lay->max_chunks = total / CH + lay->max_hubs + 1;
    lay->max_slots = acc_bytes ? 2 * (total / CH) + 2 : 0;
    lay->o_hubs = 256;
    lay->o_chunks = lay->o_hubs + hub_align(sizeof(HubRec) * (size_t)lay->max_hubs);
    lay->o_part = lay->o_chunks + hub_align(sizeof(int2) * (size_t)lay->max_chunks);
    lay->o_best = lay->o_part + hub_align(acc_bytes * (size_t)lay->max_slots * (size_t)K);
    lay->bytes = lay->o_best + (minmax ? hub_align(sizeof(int64_t) * (size_t)lay->max_slots * (size_t)K) : 0) + lay->skew;
    if (sizing || (ws_bytes && ws_bytes >= lay->bytes)) return true;
    if (!acc_bytes) break;   // (gather: nothing shrinks with longer chunks but the chunk list)
  }
  return false;
}

// the layout on the scratch it was made for
inline HubWs hub_bind(const HubLayout& lay, void* ws) {
  HubWs hw;
  char* w = static_cast<char*>(ws) + lay.skew;
  hw.counters = reinterpret_cast<int*>(w);
  hw.hubs = reinterpret_cast<HubRec*>(w + lay.o_hubs);
  hw.chunks = reinterpret_cast<int2*>(w + lay.o_chunks);
  hw.partial = w + lay.o_part;
  hw.partial_best = reinterpret_cast<int64_t*>(w + lay.o_best);
  hw.CH = lay.CH;
  const int64_t cap = 0x7fffffff;
  hw.max_hubs = (int)std::min(lay.max_hubs, cap), hw.max_chunks = (int)std::min(lay.max_chunks, cap);
  hw.max_slots = (int)std::min(lay.max_slots, cap);
  return hw;
}

// Both at once for a caller that holds the scratch (hw == nullptr: sizing).  Returns the bytes used (0: disabled).
inline size_t hub_plan(void* ws, size_t ws_bytes, int64_t total, int64_t K, size_t acc_bytes, bool minmax, HubWs* hw,
                       int64_t* max_chunks_out) {
  HubLayout lay;
  if (!hub_layout(total, K, acc_bytes, minmax, !hw, (unsigned)(reinterpret_cast<uintptr_t>(ws) & 255), ws ? ws_bytes : 0, &lay))
    return 0;
  if (!hw) return lay.bytes;
  *hw = hub_bind(lay, ws);
  *max_chunks_out = lay.max_chunks;
  return lay.bytes;
}

// ---- the row kernel of a shape ----------------------------------------------------------------------
// (narrow rows of whole 16-byte slices: 8 lanes per item from 16 positions per row on -- a load instruction then covers 8
// consecutive positions of a row: fp32 K = 4, 48 per row: 0.096 (streamed) -> 0.044 ms; bf16 K = 8, 16 per row: 0.103 -> 0.062;
// from 8 per row on it loses: fp32 K = 12: 0.19 -> 0.27.  `tools/lease/ab_narrow_vec_lanes.sh`)
#ifndef PYG_CSR_NARROW_VEC_LANES_AVG
#define PYG_CSR_NARROW_VEC_LANES_AVG 16
#endif
constexpr int64_t kNarrowVecLanesAvg = PYG_CSR_NARROW_VEC_LANES_AVG;

// The kernels a CSR call can take: one lane per item, 8 lanes over the positions of narrow rows, lane-split long rows, or the
// LDS-streamed kernel (csr.hip only).
enum class CsrKernel { kNone, kRow1, kNarrow8, kLanes8, kLanes64, kStream };
inline int kernel_lanes(CsrKernel k) {
  return k == CsrKernel::kLanes64 ? 64 : (k == CsrKernel::kLanes8 || k == CsrKernel::kNarrow8) ? 8 : 1;
}

// lanes per item: long rows + too few items to fill the `num_cus` compute units
inline CsrKernel pick_row_kernel(int64_t items, int64_t total_len, int64_t units, int num_cus, int64_t row_bytes = 64) {
  if (units <= 0 || items <= 0) return CsrKernel::kRow1;
  const int64_t avg = total_len / units;
  // rows narrower than a cache line that are too long for the LDS-streamed kernels: the lanes of an item read neighbouring
  // positions -- one contiguous piece per trip, whatever the number of items (K = 1, 300 positions per row: 0.168 -> ms)
  if (row_bytes < 64 && avg >= 64) return avg >= 256 ? CsrKernel::kLanes64 : CsrKernel::kLanes8;
  if (row_bytes < 64 && row_bytes % 16 == 0 && avg >= kNarrowVecLanesAvg) return CsrKernel::kNarrow8;
  const int64_t chip = (int64_t)num_cus * 2048;  // resident threads
  if (avg >= 1024 && items * 8 < chip) return CsrKernel::kLanes64;
  if (avg >= 64 && items < chip) return CsrKernel::kLanes8;
  return CsrKernel::kRow1;
}
inline int pick_lanes(int64_t items, int64_t total_len, int64_t units, int num_cus, int64_t row_bytes = 64) {
  return kernel_lanes(pick_row_kernel(items, total_len, units, num_cus, row_bytes));
}

}  // namespace
}  // namespace pyg_hip
