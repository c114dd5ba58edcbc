// The selection network of the 3 x 3 x 3 median (csrc/median_common.h, select_median<15> over 27 values) on ALL 2^27 zero-one
// inputs, on the host.  A network of compare-exchanges that selects the right element of every zero-one input selects it for every
// input (the zero-one principle holds for selection as for sorting: min and max commute with any monotone map of the values).
//     c++ -O2 -std=c++17 -I ddpm_ood_amd/csrc tools/median_zero_one.cpp -o median_zero_one && ./median_zero_one
// Bit-sliced: one uint64 word carries input j of 64 inputs at once, min is AND and max is OR, so the very template the kernels
// instantiate runs here on 2^21 words.  Input number i = 64 w + b has value j equal to bit j of i: values 0 .. 5 are constant words,
// value j >= 6 is all ones or all zeros by bit j - 6 of w.  The median (element 13 of 27 ascending) is 1 exactly when at least 14
// values are 1.  Prints "ok 134217728" and returns 0, or the first input that fails and 1.  tests/test_voxel_segment_host.py runs it;
// the 9-value network of the 2-D kernel (select_median<6>) is checked the same way on its 512 inputs.
#include <cstdint>
#include <cstdio>

#include "median_common.h"

namespace ddpm {
struct Slice {
  uint64_t w;
};
inline Slice min(Slice a, Slice b) { return Slice{a.w & b.w}; }
inline Slice max(Slice a, Slice b) { return Slice{a.w | b.w}; }
}  // namespace ddpm

using ddpm::Slice;

static const uint64_t kLow[6] = {0xaaaaaaaaaaaaaaaaull, 0xccccccccccccccccull, 0xf0f0f0f0f0f0f0f0ull,
                                 0xff00ff00ff00ff00ull, 0xffff0000ffff0000ull, 0xffffffff00000000ull};

template <int M>
static int check() {
  constexpr int need = M - (M - 1) / 2;  // ones for element (M - 1) / 2 of the ascending sort to be 1
  uint64_t want_by_high[M + 1];          // by the number of ones among the values 6 .. M - 1
  for (int c = 0; c <= M; ++c) {
    uint64_t w = 0;
    for (int b = 0; b < 64; ++b)
      if (__builtin_popcount((unsigned)b) + c >= need) w |= 1ull << b;
    want_by_high[c] = w;
  }
  const uint64_t words = 1ull << (M - 6);
  for (uint64_t w = 0; w < words; ++w) {
    Slice v[M];
    for (int j = 0; j < M; ++j) v[j].w = j < 6 ? kLow[j] : (((w >> (j - 6)) & 1ull) ? ~0ull : 0ull);
    const uint64_t got = ddpm::select_median<M / 2 + 2>(v).w;
    const uint64_t want = want_by_high[__builtin_popcountll(w)];
    if (got != want) {
      const int b = __builtin_ctzll(got ^ want);
      std::printf("window of %d: input %llu selects %d, not the median\n", M, (unsigned long long)(w * 64 + b), (int)((got >> b) & 1ull));
      return 1;
    }
  }
  std::printf("ok %llu\n", (unsigned long long)(words * 64));
  return 0;
}

int main() {
  if (check<9>()) return 1;
  return check<27>();
}
