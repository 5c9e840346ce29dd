// The CPU keys' random integers (pyg_binding_cpu.cpp, pyg_binding_walk.cpp): the reference's PrefetchedRandint
// (random/cpu/rand_engine.h:23-92) on the global CPU generator.
#pragma once

#include <ATen/ATen.h>

#include <cstdint>
#include <limits>

namespace pyg_amd {
namespace cpu {

using at::Tensor;

// ---------------------------------------------------------------------------------------------------------------
// random integers: 128 prefetched 64-bit words, consumed 16 / 32 / 64 bits at a time from the last word down
// ---------------------------------------------------------------------------------------------------------------
class WordEngine {
 public:
  WordEngine() {
    buf_ = at::randint(std::numeric_limits<int64_t>::min(), std::numeric_limits<int64_t>::max(), {kWords}, at::kLong);
    words_ = buf_.data_ptr<int64_t>();
  }
  // uniform in [0, range)
  uint64_t below(uint64_t range) {
    const int need = range < (1ull << 16) ? 16 : (range < (1ull << 32) ? 32 : 64);
    if (bits_ < need) {
      if (pos_ > 0) {
        --pos_;
      } else {
        buf_.random_(std::numeric_limits<int64_t>::min(), std::numeric_limits<int64_t>::max());
        pos_ = kWords - 1;
      }
      bits_ = 64;  // whatever was left of the previous word is dropped
    }
    uint64_t w = static_cast<uint64_t>(words_[pos_]);
    const uint64_t mask = need == 64 ? ~0ull : ((1ull << need) - 1);
    const uint64_t r = (w & mask) % range;
    w = need == 64 ? 0 : (w >> need);
    words_[pos_] = static_cast<int64_t>(w);
    bits_ -= need;
    return r;
  }

 private:
  static constexpr int kWords = 128;
  Tensor buf_;
  int64_t* words_;
  int pos_ = kWords - 1;
  int bits_ = 64;
};

}  // namespace cpu
}  // namespace pyg_amd
