// What pixel_metrics.hip and regions.hip share: the bin of a map value and the overlap test of two operands.
#pragma once
#include "common.h"

namespace ddpm {

constexpr int kHistMaxBins = 8191;  // pixel_metrics: 2 classes x (8191 + 1) counters x 4 B = 64 KB; regions: 8192 counters = 32 KB
constexpr int kCountsMaxK = 8;

static inline bool pm_overlap(const void *p, double p_bytes, const void *q, double q_bytes) {
  const double a0 = (double)(uintptr_t)p, b0 = (double)(uintptr_t)q;
  return a0 < b0 + q_bytes && b0 < a0 + p_bytes;
}

// b = (v - lo) * inv_step in fp32, each operation rounded once; the comparisons come before the conversion, so that no value
// outside the int range is ever converted
__device__ __forceinline__ int pm_bin(float v, float lo, float inv_step, int nbins) {
  const float b = (v - lo) * inv_step;
  if (b != b) return nbins;
  if (b < 0.0f) return 0;
  if (b >= (float)nbins) return nbins - 1;
  return (int)b;
}

}  // namespace ddpm
