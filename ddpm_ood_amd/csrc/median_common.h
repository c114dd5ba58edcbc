// What segment.hip and segment3d.hip share: the key of a value, its inverse, the reflected index and the selection network of the
// median (the header comment of segment.hip describes them).  The selection is a template over the value type, so that a host
// program can run the very same compare-exchange sequence on bit-sliced zero-one inputs (tools/median_zero_one.cpp): the type needs
// min and max, found by argument-dependent lookup.  Compiled without hipcc only the selection is declared.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define DDPM_MED_FN __device__ __forceinline__
#else
#define DDPM_MED_FN inline
#endif

namespace ddpm {

#ifdef __HIPCC__
__device__ __forceinline__ uint32_t med_key(float v) {
  const uint32_t b = __float_as_uint(v);
  if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;  // a NaN of either sign: above +inf
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float med_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// scipy.ndimage's mode="reflect" (d c b a | a b c d | d c b a), any distance from the plane
__device__ __forceinline__ int med_reflect(int i, int L) {
  const int period = 2 * L;
  int m = i % period;
  if (m < 0) m += period;
  return m < L ? m : period - 1 - m;
}
#endif

#define DDPM_MED_CE(a, b)              \
  {                                    \
    const T lo_ = min((a), (b));       \
    (b) = max((a), (b));               \
    (a) = lo_;                         \
  }

// the smallest of v[0 .. n - 1] to v[0], the largest to v[n - 1]
template <int n, class T>
DDPM_MED_FN void select_minmax(T *v) {
#pragma unroll
  for (int i = 0; i < n / 2; ++i) DDPM_MED_CE(v[i], v[n - 1 - i]);
#pragma unroll
  for (int i = 1; i < (n + 1) / 2; ++i) DDPM_MED_CE(v[0], v[i]);
#pragma unroll
  for (int i = n / 2; i < n - 1; ++i) DDPM_MED_CE(v[i], v[n - 1]);
}

// v[0 .. n - 1] hold n values of the window, n shrinking by one per step from n0; v[n0 ..] are the ones still to join, in order
template <int n0, int n = n0, class T = uint32_t>
DDPM_MED_FN T select_median(T *v) {
  select_minmax<n>(v);
  if constexpr (n == 3) {
    return v[1];
  } else {
    v[0] = v[2 * n0 - n];  // (the smallest leaves, the next value takes its slot; the largest, in slot n - 1, falls out of the range)
    return select_median<n0, n - 1>(v);
  }
}

}  // namespace ddpm
