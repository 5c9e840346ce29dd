// One item of pyg::edge_lookup and pyg::negative_sample_keyed on the host: the specification (include/pyg_hip.h, "Edge
// lookup and negative sampling") statement by statement, all arithmetic in int64 whatever the index type.
// Header only and free of tensors -- at::Philox4_32 is the one thing taken from ATen -- so that the CPU key
// (pyg_binding_negative.cpp) and a stand-alone sanitizer build (tools/sanitize_negative.cpp) run the same code.
#pragma once

#include <ATen/core/PhiloxRNGEngine.h>

#include <algorithm>
#include <cstdint>

namespace pyg_amd {
namespace negative {

template <typename scalar_t>
inline int64_t lower_bound(const scalar_t* W, int64_t n, int64_t x) {
  int64_t a = 0, b = n;
  while (a < b) {
    const int64_t mid = (a + b) / 2;
    if ((int64_t)W[mid] < x)
      a = mid + 1;
    else
      b = mid;
  }
  return a;
}

// The r-th value of lo, lo + 1, ... that is not in W[0, n) (r < (hi - lo) - n).  A value below lo always sends the search
// right and one at or above hi always left: clamping it first changes no decision and keeps the difference inside int64 on
// rows that break the precondition.
template <typename scalar_t>
inline int64_t kth(const scalar_t* W, int64_t n, int64_t lo, int64_t hi, int64_t r) {
  int64_t a = 0, b = n;
  while (a < b) {
    const int64_t mid = (a + b) / 2;
    const int64_t v = std::min(std::max((int64_t)W[mid], lo - 1), hi);
    if (v - lo - mid > r)
      b = mid;
    else
      a = mid + 1;
  }
  return lo + r + a;
}

template <typename scalar_t>
inline bool valid_row(const scalar_t* rp, int64_t num_src, int64_t E, int64_t s, int64_t& rs, int64_t& re) {
  if (s < 0 || s >= num_src) return false;
  rs = rp[s], re = rp[s + 1];
  return rs >= 0 && re <= E && re >= rs;
}

// the draw below n (n > 0) of item t
inline int64_t draw_below(uint64_t key, int64_t t, int64_t n) {
  at::Philox4_32 rng(key, /*subsequence=*/(uint64_t)t, /*offset=*/0);
  const uint64_t w0 = rng(), w1 = rng();
  const uint64_t w = (w0 << 32) | w1;
  return (int64_t)(uint64_t)(((unsigned __int128)w * (unsigned __int128)(uint64_t)n) >> 64);
}

template <typename scalar_t>
inline int64_t lookup_item(const scalar_t* rp, const scalar_t* cl, int64_t num_src, int64_t E, int64_t s, int64_t x) {
  int64_t rs, re;
  if (!valid_row(rp, num_src, E, s, rs, re)) return -1;
  const int64_t k = lower_bound(cl + rs, re - rs, x);
  return k < re - rs && (int64_t)cl[rs + k] == x ? rs + k : -1;
}

// item t of the structured form, for source s = src[t / num_neg]; ptr may be null (then G is ignored)
template <typename scalar_t>
inline int64_t structured_item(const scalar_t* rp, const scalar_t* cl, const scalar_t* ptr, int64_t s, int64_t t,
                               int64_t num_src, int64_t E, int64_t num_dst, int64_t G, uint64_t key, bool exclude_self) {
  int64_t rs, re;
  if (!valid_row(rp, num_src, E, s, rs, re)) return -1;
  int64_t lo = 0, hi = num_dst;
  if (ptr != nullptr) {
    int64_t a = 0, b = G + 1;
    while (a < b) {
      const int64_t mid = (a + b) / 2;
      if ((int64_t)ptr[mid] <= s)
        a = mid + 1;
      else
        b = mid;
    }
    const int64_t g = a - 1;
    if (g < 0 || g >= G) return -1;
    lo = std::max<int64_t>(ptr[g], 0);
    hi = std::min<int64_t>(ptr[g + 1], num_dst);
  }
  // an empty range has no candidate (n <= 0 below); decided here, where a wild ptr cannot yet overflow hi - lo
  if (hi <= lo) return -1;
  const scalar_t* row = cl + rs;
  const int64_t p_lo = lower_bound(row, re - rs, lo), p_hi = lower_bound(row, re - rs, hi);
  const scalar_t* W = row + p_lo;
  const int64_t d = std::max<int64_t>(p_hi - p_lo, 0);
  bool self_ex = false;
  if (exclude_self && lo <= s && s < hi) {
    const int64_t k = lower_bound(W, d, s);
    self_ex = !(k < d && (int64_t)W[k] == s);
  }
  const int64_t n = (hi - lo) - d - (self_ex ? 1 : 0);
  if (n <= 0) return -1;
  const int64_t r = draw_below(key, t, n);
  int64_t x = kth(W, d, lo, hi, r);
  if (self_ex && x >= s) x = kth(W, d, lo, hi, r + 1);
  return x;
}

// item t of the global form; T = num_src * num_dst - E
template <typename scalar_t>
inline void global_item(const scalar_t* rp, const scalar_t* cl, int64_t t, int64_t num_src, int64_t E, int64_t num_dst,
                        int64_t T, uint64_t key, int64_t& s, int64_t& x) {
  s = -1, x = -1;
  if (T <= 0) return;
  const int64_t R = draw_below(key, t, T);
  int64_t a = 0, b = num_src;
  while (a < b) {
    const int64_t mid = (a + b) / 2;
    // (mid + 1) * num_dst - rowptr[mid + 1] > R, with the rowptr entry alone on its side: the other side lies in
    // (-num_src * num_dst, num_src * num_dst], so nothing overflows whatever rowptr holds
    if ((int64_t)rp[mid + 1] < (mid + 1) * num_dst - R)
      b = mid;
    else
      a = mid + 1;
  }
  int64_t rs, re;
  if (a >= num_src || !valid_row(rp, num_src, E, a, rs, re)) return;
  const int64_t r = R - (a * num_dst - rs);
  if (r < 0 || r >= num_dst - (re - rs)) return;
  s = a;
  x = kth(cl + rs, re - rs, (int64_t)0, num_dst, r);
}

}  // namespace negative
}  // namespace pyg_amd
