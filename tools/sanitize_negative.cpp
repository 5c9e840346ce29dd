// The host code of pyg::edge_lookup / pyg::negative_sample_keyed (csrc/binding/negative_cpu.h, the items the CPU key runs)
// under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own: every buffer is a heap block of exactly
// its size, so a read one entry outside is reported.  Host only -- no device, no Python.
//
//   TORCH=$(python -c "import torch, os; print(os.path.dirname(torch.__file__))")
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I"$TORCH/include" \
//       -Ipyg_lib_amd/csrc/binding tools/sanitize_negative.cpp -o /tmp/sanitize_negative && /tmp/sanitize_negative
//
// Graphs: coalesced rows with an empty, a full and an all-but-self row; rows that break the precondition (unsorted,
// duplicates, entries outside [0, num_dst), extreme int64 values); rowptr pairs that are negative, reversed or beyond the
// edges; a ptr that is not ascending; rowptr and ptr entries at both ends of int64.  Sources from -2 to num_src + 1.  int32 and int64.  Prints a checksum and "ok".
#include <cstdint>
#include <cstdio>
#include <limits>
#include <memory>
#include <vector>

#include "negative_cpu.h"

namespace neg = pyg_amd::negative;

template <typename T>
std::unique_ptr<T[]> exact(const std::vector<int64_t>& v) {  // a heap block of exactly v.size() entries
  std::unique_ptr<T[]> p(new T[v.size()]);
  for (size_t i = 0; i < v.size(); ++i) p[i] = (T)v[i];
  return p;
}

struct Graph {
  std::vector<int64_t> rowptr, col, ptr;
  int64_t num_dst;
};

template <typename T>
uint64_t run(const Graph& g) {
  const int64_t num_src = (int64_t)g.rowptr.size() - 1, E = (int64_t)g.col.size(), G = (int64_t)g.ptr.size() - 1;
  const auto rp = exact<T>(g.rowptr), cl = exact<T>(g.col), pt = exact<T>(g.ptr);
  uint64_t sum = 0;
  int64_t t = 0;
  for (uint64_t key : {0ull, ~0ull, 0x1234ABCD5678EF01ull})
    for (int64_t s = -2; s <= num_src + 1; ++s)
      for (int j = 0; j < 50; ++j, ++t)
        for (int mode = 0; mode < 4; ++mode) {
          const int64_t x = neg::structured_item<T>(rp.get(), cl.get(), mode & 2 ? pt.get() : nullptr, s, t, num_src, E,
                                                    g.num_dst, G, key, mode & 1);
          if (x < -1 || x >= g.num_dst) {
            std::printf("structured result %lld outside [-1, %lld)\n", (long long)x, (long long)g.num_dst);
            return 0;
          }
          sum = sum * 1099511628211ull + (uint64_t)x;
        }
  int64_t cells = num_src * g.num_dst - E;
  for (int64_t j = 0; j < 5000; ++j) {
    int64_t s, x;
    neg::global_item<T>(rp.get(), cl.get(), j, num_src, E, g.num_dst, cells, 0x1234ABCD5678EF01ull, s, x);
    if (s < -1 || s >= num_src || x < -1 || x >= g.num_dst || (s == -1) != (x == -1)) {
      std::printf("global result (%lld, %lld) outside the matrix\n", (long long)s, (long long)x);
      return 0;
    }
    sum = sum * 1099511628211ull + (uint64_t)(s * g.num_dst + x);
  }
  for (int64_t s = -2; s <= num_src + 1; ++s)
    for (int64_t x = -2; x <= std::min<int64_t>(g.num_dst + 1, 64); ++x) {
      const int64_t e = neg::lookup_item<T>(rp.get(), cl.get(), num_src, E, s, x);
      if (e < -1 || e >= E || (e >= 0 && (int64_t)cl[e] != x)) {
        std::printf("edge_lookup(%lld, %lld) = %lld\n", (long long)s, (long long)x, (long long)e);
        return 0;
      }
      sum = sum * 1099511628211ull + (uint64_t)e;
    }
  return sum | 1;
}

int main() {
  const int64_t big = std::numeric_limits<int64_t>::max(), small = std::numeric_limits<int64_t>::min();
  std::vector<Graph> graphs;
  {  // coalesced: 12 x 16, Poisson-like rows from an LCG; row 0 empty, row 1 full, row 3 all but 3
    Graph g{{0}, {}, {0, 5, 6, 11, 16}, 16};
    uint64_t z = 12345;
    for (int s = 0; s < 12; ++s) {
      for (int x = 0; x < 16; ++x) {
        z = z * 6364136223846793005ull + 1442695040888963407ull;
        const bool in = s == 0 ? false : s == 1 ? true : s == 3 ? x != 3 : (z >> 60) < 5;
        if (in) g.col.push_back(x);
      }
      g.rowptr.push_back((int64_t)g.col.size());
    }
    graphs.push_back(g);
  }
  // rows that break the precondition, a ptr that is not ascending
  graphs.push_back({{0, 4, 7, 17, 17, 23, 26, 29, 34, 35, 47},
                    {7, 2, 5, 2, 3, 3, 3, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 0, 0, 1, 1, 9, 9, 12, -4, 5, 1, 2, 3,
                     5, 1, 5, 1, 5, 4, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9},
                    {0, 6, 3, 8, 8, 10}, 10});
  // rowptr pairs that are no rows
  graphs.push_back({{0, 3, -2, 9, 4, 6}, {0, 1, 2, 3, 4, 5}, {0, 2, 8}, 8});
  // no edges, no destinations
  graphs.push_back({{0, 0, 0}, {}, {0, 0}, 0});
  uint64_t sum = 0;
  for (const Graph& g : graphs) {
    const uint64_t a = run<int64_t>(g), b = run<int32_t>(g);
    if (!a || !b) return 1;
    if (a != b) {
      std::printf("int32 and int64 disagree\n");
      return 1;
    }
    sum ^= a;
  }
  // int64 only: entries at the ends of the type (the clamp in kth keeps the arithmetic inside int64)
  Graph wild{{0, 6, 9}, {small, -1, 3, 4, big - 1, big, big, 2, small}, {0, 9}, 9};
  const uint64_t w = run<int64_t>(wild);
  if (!w) return 1;
  // int64 only: rowptr and ptr entries at the ends of the type (no comparison may overflow)
  for (const std::vector<int64_t>& ptr : std::vector<std::vector<int64_t>>{
           {small, 2, big, small + 5, 3, big}, {0, big, small, 8}, {big, small, 0, 4, big}}) {
    const uint64_t u = run<int64_t>(Graph{{0, 3, small, big, 4, 6}, {0, 1, 2, 3, 4, 5}, ptr, 8});
    if (!u) return 1;
    sum ^= u;
  }
  // a 2^40-wide empty matrix: the draw is 64 bits wide
  Graph wide{{0, 0, 0}, {}, {0, int64_t(1) << 40}, int64_t(1) << 40};
  const uint64_t v = run<int64_t>(wide);
  if (!v) return 1;
  std::printf("checksum %016llx\nok\n", (unsigned long long)(sum ^ w ^ v));
  return 0;
}
