// Pixel-level evaluation of anomaly maps against ground-truth masks (only with --pixel_metrics 1).
//   map_mask_hist     two-class histogram of a batch of maps (class = mask != 0) over a fixed range, NaN in a column of its own
//   map_mask_counts   per image and threshold: TP, FP, FN of the prediction v > thr against mask != 0
// Integers only behind the one fp32 bin computation, so every result is independent of the order of the additions: no global
// atomics, nothing depends on what a buffer held before.
// map_mask_hist: a workgroup of 256 threads keeps a private histogram of 2 (nbins + 1) counters in LDS (ds_add_u32; 64 KB of
// static LDS at the largest nbins of 8191) and walks the flat [N P] array in chunks of four floats with a grid stride: one
// 16-byte map load and the four mask bytes per chunk.  The chunks start at the first 16-byte boundary of `maps`; the up to
// three elements in front of it and the up to three behind the last chunk are taken by workgroup 0.  The four mask bytes come
// as one dword where their address allows and as four byte loads otherwise.  Each workgroup stores its histogram into its
// own slab; map_mask_hist_sum adds the slabs in ascending order in int64 and writes, or adds to, `total`.
// Bytes: 5 N P in, parts 2 (nbins + 1) 4 out and in again, 2 (nbins + 1) 8 out.
// map_mask_counts: one workgroup of 256 threads per image, per-thread integer counters for the K <= 8 thresholds, a butterfly
// over the wave (__shfl_xor 32 .. 1), the four waves' partials through LDS, 3 K plain stores.
#include "pixel_common.h"

namespace ddpm {

constexpr int kHistCounters = 2 * (kHistMaxBins + 1);
constexpr int kPmBlock = 256;

__global__ __launch_bounds__(kPmBlock) void map_mask_hist_kernel(const float *__restrict__ maps, const uint8_t *__restrict__ masks,
                                                                 uint32_t total_elems, uint32_t head, uint32_t chunks,
                                                                 int mask_dwords, float lo, float inv_step, int nbins,
                                                                 uint32_t *__restrict__ slabs) {
  __shared__ uint32_t hist[kHistCounters];
  const int width = nbins + 1, counters = 2 * width;
  for (int i = threadIdx.x; i < counters; i += kPmBlock) hist[i] = 0u;
  __syncthreads();
  const float4 *body = reinterpret_cast<const float4 *>(maps + head);
  const uint8_t *mbody = masks + head;
  const uint32_t stride = gridDim.x * (uint32_t)kPmBlock;
  // (chunks <= 2^30 and the stride <= 2^24: the index is kept in 64 bits so that its last step cannot wrap)
  for (uint64_t i = blockIdx.x * (uint32_t)kPmBlock + threadIdx.x; i < chunks; i += stride) {
    const float4 v = body[i];
    uint32_t m;
    if (mask_dwords) {
      m = *reinterpret_cast<const uint32_t *>(mbody + 4 * i);
    } else {
      const uint8_t *q = mbody + 4 * i;
      m = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
    }
    atomicAdd(&hist[((m & 0xffu) ? width : 0) + pm_bin(v.x, lo, inv_step, nbins)], 1u);
    atomicAdd(&hist[((m & 0xff00u) ? width : 0) + pm_bin(v.y, lo, inv_step, nbins)], 1u);
    atomicAdd(&hist[((m & 0xff0000u) ? width : 0) + pm_bin(v.z, lo, inv_step, nbins)], 1u);
    atomicAdd(&hist[((m & 0xff000000u) ? width : 0) + pm_bin(v.w, lo, inv_step, nbins)], 1u);
  }
  if (blockIdx.x == 0) {  // the elements in front of the first chunk and behind the last one (at most three each)
    const uint32_t tail0 = head + 4u * chunks, ragged = head + (total_elems - tail0);
    if (threadIdx.x < ragged) {
      const uint32_t e = threadIdx.x < head ? threadIdx.x : tail0 + (threadIdx.x - head);
      atomicAdd(&hist[(masks[e] ? width : 0) + pm_bin(maps[e], lo, inv_step, nbins)], 1u);
    }
  }
  __syncthreads();
  uint32_t *slab = slabs + (size_t)blockIdx.x * counters;
  for (int i = threadIdx.x; i < counters; i += kPmBlock) slab[i] = hist[i];
}

__global__ __launch_bounds__(kPmBlock) void map_mask_hist_sum_kernel(const uint32_t *__restrict__ slabs, int parts, int counters,
                                                                     int accumulate, int64_t *__restrict__ total) {
  const int i = blockIdx.x * kPmBlock + threadIdx.x;
  if (i >= counters) return;
  int64_t sum = 0;
  for (int p = 0; p < parts; ++p) sum += (int64_t)slabs[(size_t)p * counters + i];
  total[i] = accumulate ? total[i] + sum : sum;
}

int launch_map_mask_hist(const float *maps, const uint8_t *masks, int N, int64_t P, float lo, float inv_step, int nbins, int parts,
                         uint32_t *slabs, int64_t *total, int accumulate, hipStream_t s) {
  DDPM_CHECK_ARG(maps && masks && slabs && total, "map_mask_hist: null pointer");
  DDPM_CHECK_ARG(N > 0 && P > 0, "map_mask_hist: N and P must be positive (got %d, %lld)", N, (long long)P);
  DDPM_CHECK_ARG(nbins >= 1 && nbins <= kHistMaxBins, "map_mask_hist: nbins must lie in 1 .. %d (got %d): two classes of nbins + 1 "
                 "counters fill the 64 KB of LDS", kHistMaxBins, nbins);
  DDPM_CHECK_ARG((double)N * (double)P < 4294967296.0, "map_mask_hist: N * P must stay below 2^32 (got %d x %lld): the slabs "
                 "count in 32 bits", N, (long long)P);
  DDPM_CHECK_ARG(parts >= 1 && parts <= 65536, "map_mask_hist: parts must lie in 1 .. 65536 (got %d)", parts);
  DDPM_CHECK_ARG(inv_step > 0.0f && inv_step <= 3.402823466e+38f && lo == lo && lo - lo == 0.0f,
                 "map_mask_hist: lo must be finite and inv_step positive and finite (got %g, %g)", (double)lo, (double)inv_step);
  DDPM_CHECK_ARG(((uintptr_t)maps & 3) == 0 && ((uintptr_t)slabs & 3) == 0 && ((uintptr_t)total & 7) == 0,
                 "map_mask_hist: maps / slabs must be 4-byte and total 8-byte aligned");
  const int counters = 2 * (nbins + 1);
  const double elems = (double)N * (double)P, map_bytes = 4.0 * elems, slab_bytes = 4.0 * parts * counters,
               total_bytes = 8.0 * counters;
  DDPM_CHECK_ARG(!pm_overlap(slabs, slab_bytes, maps, map_bytes) && !pm_overlap(slabs, slab_bytes, masks, elems) &&
                     !pm_overlap(total, total_bytes, maps, map_bytes) && !pm_overlap(total, total_bytes, masks, elems) &&
                     !pm_overlap(slabs, slab_bytes, total, total_bytes),
                 "map_mask_hist: slabs / total alias another operand");
  const uint64_t T = (uint64_t)N * (uint64_t)P;
  uint64_t head = ((16 - ((uintptr_t)maps & 15)) & 15) / 4;
  if (head > T) head = T;
  const uint64_t chunks = (T - head) / 4;
  const int mask_dwords = (((uintptr_t)masks + head) & 3) == 0 ? 1 : 0;
  ProfScope prof(s, "map_mask_hist", 2.0 * elems, 5.0 * elems + 2.0 * slab_bytes + total_bytes);
  hipLaunchKernelGGL(map_mask_hist_kernel, dim3((unsigned)parts), dim3(kPmBlock), 0, s, maps, masks, (uint32_t)T, (uint32_t)head,
                     (uint32_t)chunks, mask_dwords, lo, inv_step, nbins, slabs);
  DDPM_CHECK_LAUNCH();
  hipLaunchKernelGGL(map_mask_hist_sum_kernel, dim3((unsigned)((counters + kPmBlock - 1) / kPmBlock)), dim3(kPmBlock), 0, s, slabs,
                     parts, counters, accumulate, total);
  DDPM_CHECK_LAUNCH();
  return 0;
}

// ---- TP / FP / FN per image and threshold -------------------------------------------------------------------------------------------
__device__ __forceinline__ void pm_count(float v, bool pos, const float (&thr)[kCountsMaxK], int K, int (&c)[kCountsMaxK][3]) {
#pragma unroll
  for (int k = 0; k < kCountsMaxK; ++k) {
    if (k < K) {
      const bool pred = v > thr[k];  // (a NaN pixel, or a NaN threshold: predicted negative)
      c[k][0] += (pred && pos) ? 1 : 0;
      c[k][1] += (pred && !pos) ? 1 : 0;
      c[k][2] += (!pred && pos) ? 1 : 0;
    }
  }
}

__global__ __launch_bounds__(kPmBlock) void map_mask_counts_kernel(const float *__restrict__ maps, const uint8_t *__restrict__ masks,
                                                                   int64_t P, const float *__restrict__ thresholds, int K,
                                                                   int vec, int32_t *__restrict__ counts) {
  __shared__ int red[kPmBlock / 64][kCountsMaxK * 3];
  const float *row = maps + (int64_t)blockIdx.x * P;
  const uint8_t *mrow = masks + (int64_t)blockIdx.x * P;
  float thr[kCountsMaxK];
  int c[kCountsMaxK][3];
#pragma unroll
  for (int k = 0; k < kCountsMaxK; ++k) {
    thr[k] = k < K ? thresholds[k] : 0.0f;
    c[k][0] = c[k][1] = c[k][2] = 0;
  }
  if (vec) {  // P % 4 == 0, every row of the maps 16-byte and of the masks 4-byte aligned
    const float4 *r4 = reinterpret_cast<const float4 *>(row);
    const uint32_t *m4 = reinterpret_cast<const uint32_t *>(mrow);
    for (int64_t i = threadIdx.x; i < P / 4; i += kPmBlock) {
      const float4 v = r4[i];
      const uint32_t m = m4[i];
      pm_count(v.x, (m & 0xffu) != 0, thr, K, c);
      pm_count(v.y, (m & 0xff00u) != 0, thr, K, c);
      pm_count(v.z, (m & 0xff0000u) != 0, thr, K, c);
      pm_count(v.w, (m & 0xff000000u) != 0, thr, K, c);
    }
  } else {
    for (int64_t i = threadIdx.x; i < P; i += kPmBlock) pm_count(row[i], mrow[i] != 0, thr, K, c);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kCountsMaxK; ++k) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      int v = c[k][j];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == 0) red[wave][k * 3 + j] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < K * 3) {
    const int t = threadIdx.x;
    counts[(int64_t)blockIdx.x * K * 3 + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
  }
}

int launch_map_mask_counts(const float *maps, const uint8_t *masks, int N, int64_t P, const float *thresholds, int K, int32_t *counts,
                           hipStream_t s) {
  DDPM_CHECK_ARG(maps && masks && thresholds && counts, "map_mask_counts: null pointer");
  DDPM_CHECK_ARG(N > 0 && P > 0, "map_mask_counts: N and P must be positive (got %d, %lld)", N, (long long)P);
  DDPM_CHECK_ARG(P < 2147483648LL, "map_mask_counts: P must stay below 2^31 (got %lld): the counts are 32-bit", (long long)P);
  DDPM_CHECK_ARG(K >= 1 && K <= kCountsMaxK, "map_mask_counts: K must lie in 1 .. %d (got %d)", kCountsMaxK, K);
  DDPM_CHECK_ARG((double)N * (double)P < 9.0e18, "map_mask_counts: tensor too large");
  DDPM_CHECK_ARG(((uintptr_t)maps & 3) == 0 && ((uintptr_t)thresholds & 3) == 0 && ((uintptr_t)counts & 3) == 0,
                 "map_mask_counts: maps / thresholds / counts must be 4-byte aligned");
  const double elems = (double)N * (double)P, out_bytes = 12.0 * N * K;
  DDPM_CHECK_ARG(!pm_overlap(counts, out_bytes, maps, 4.0 * elems) && !pm_overlap(counts, out_bytes, masks, elems) &&
                     !pm_overlap(counts, out_bytes, thresholds, 4.0 * K),
                 "map_mask_counts: counts aliases an input");
  const int vec = (P & 3) == 0 && ((uintptr_t)maps & 15) == 0 && ((uintptr_t)masks & 3) == 0 ? 1 : 0;
  ProfScope prof(s, "map_mask_counts", 3.0 * K * elems, 5.0 * elems + out_bytes);
  hipLaunchKernelGGL(map_mask_counts_kernel, dim3((unsigned)N), dim3(kPmBlock), 0, s, maps, masks, P, thresholds, K, vec, counts);
  DDPM_CHECK_LAUNCH();
  return 0;
}

}  // namespace ddpm

using namespace ddpm;

extern "C" int ddpm_map_mask_hist_f32(const float *maps, const uint8_t *masks, int N, int64_t P, float lo, float inv_step, int nbins,
                                      int parts, uint32_t *slabs, int64_t *total, int accumulate, ddpm_stream_t stream) {
  return launch_map_mask_hist(maps, masks, N, P, lo, inv_step, nbins, parts, slabs, total, accumulate, as_stream(stream));
}

extern "C" int ddpm_map_mask_counts_f32(const float *maps, const uint8_t *masks, int N, int64_t P, const float *thresholds, int K,
                                        int32_t *counts, ddpm_stream_t stream) {
  return launch_map_mask_counts(maps, masks, N, P, thresholds, K, counts, as_stream(stream));
}
