// Per-pixel Z-scores of the anomaly maps against the validation set (only with --anomaly_z_maps 1).
//   map_stats_update   running per-column mean and sum of squared deviations over the validation set, one batch per call
//   map_zscore         out[b, p] = weight * sum_t (v[b, t, p] - mean[t, p]) * inv_std[t, p]
//   map_zscore_loo     the same for a row of the validation set itself, against the statistics of the OTHER n - 1 rows
//   map_blur           separable Gaussian smoothing of [N, H, W] maps, scipy's mode="reflect" boundary, one launch
// Plain fp32, no atomics, no cross-thread reductions: every output value is ONE fixed sequence of operations (the build has no FMA
// contraction, so each operation rounds once).  map_stats_update, map_zscore and map_zscore_loo: a thread owns V adjacent columns (V = 4: 16-byte
// accesses when the row length is a multiple of 4 and every base is 16-byte aligned; V = 1: the scalar path); both forms do the
// same arithmetic per column, so they give the same bits.  Bytes per column: stats 4 B + 16 (the second pass over the column
// is served from cache), zscore and zscore_loo 4 n_t (B + 2) / B + 4 per output (the tables are re-read from cache across the B rows).
// map_blur: a workgroup of 256 threads owns a 32 x 32 output tile.  It stages the tile plus a halo of `radius` on all four sides
// through refl() into LDS ((32 + 2 r)^2 floats), runs the H pass over the tile's rows and tile width plus halo in W into a
// second LDS array (32 x (32 + 2 r) floats) and the W pass from there to `out`.  radius <= kBlurMaxRadius = 16:
// LDS = 64 * 65 * 4 + 32 * 65 * 4 = 24 960 bytes (rows padded by one float).  A larger radius is refused.
#include "common.h"

namespace ddpm {

static bool zm_overlap(const void *p, double p_bytes, const void *q, double q_bytes) {
  const double a0 = (double)(uintptr_t)p, b0 = (double)(uintptr_t)q;
  return a0 < b0 + q_bytes && b0 < a0 + p_bytes;
}

// ---- running mean / M2 (Chan's pairwise update, the batch's own statistics by two passes) --------------------------------------------
// r_mean = B / n and r_m2 = n_prev * B / n (n = n_prev + B) are formed by the launcher in float64 and rounded once to fp32.
// A column's additions are one dependent chain, so the only parallelism is across columns: workgroups of ONE wave spread the
// P / V threads over as many CUs as there are (12 800 threads at the bench's 25 x 2 x 32 x 32 with V = 4), and the row loops
// are unrolled by 8 so that eight loads are in flight per thread (the additions keep their order).
constexpr int kStatsBlock = 64;
template <int V>
__global__ __launch_bounds__(kStatsBlock) void map_stats_update_kernel(const float *__restrict__ values, int B, int64_t P, int first,
                                                               float r_mean, float r_m2, float *__restrict__ mean,
                                                               float *__restrict__ m2) {
  struct alignas(4 * V) Vec { float v[V]; };
  const int64_t items = P / V;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const float fb = (float)B;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += stride) {
    const float *col = values + i * V;
    float mb[V], Mb[V];
#pragma unroll
    for (int j = 0; j < V; ++j) mb[j] = 0.f;
#pragma unroll 8
    for (int b = 0; b < B; ++b) {
      const Vec x = *reinterpret_cast<const Vec *>(col + (int64_t)b * P);
#pragma unroll
      for (int j = 0; j < V; ++j) mb[j] += x.v[j];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      mb[j] = mb[j] / fb;
      Mb[j] = 0.f;
    }
#pragma unroll 8
    for (int b = 0; b < B; ++b) {
      const Vec x = *reinterpret_cast<const Vec *>(col + (int64_t)b * P);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float d = x.v[j] - mb[j];
        Mb[j] += d * d;
      }
    }
    Vec *pm = reinterpret_cast<Vec *>(mean + i * V), *pq = reinterpret_cast<Vec *>(m2 + i * V);
    Vec om, oq;
    if (first) {  // the buffers' previous contents are not read
#pragma unroll
      for (int j = 0; j < V; ++j) {
        om.v[j] = mb[j];
        oq.v[j] = Mb[j];
      }
    } else {
      om = *pm;
      oq = *pq;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float delta = mb[j] - om.v[j];
        om.v[j] = om.v[j] + delta * r_mean;
        oq.v[j] = oq.v[j] + (Mb[j] + (delta * delta) * r_m2);
      }
    }
    *pm = om;
    *pq = oq;
  }
}

static unsigned zm_blocks(int64_t items) {
  int64_t blocks = (items + 255) / 256;
  return (unsigned)(blocks > 4096 ? 4096 : blocks);
}

int launch_map_stats_update(const float *values, int B, int64_t P, int64_t n_prev, float *mean, float *m2, hipStream_t s) {
  DDPM_CHECK_ARG(values && mean && m2, "map_stats_update: null pointer");
  DDPM_CHECK_ARG(B > 0, "map_stats_update: B must be positive (got %d)", B);
  DDPM_CHECK_ARG(P > 0, "map_stats_update: P must be positive (got %lld)", (long long)P);
  DDPM_CHECK_ARG(n_prev >= 0, "map_stats_update: n_prev must not be negative (got %lld)", (long long)n_prev);
  DDPM_CHECK_ARG((double)B * (double)P < 9.0e18 && n_prev < ((int64_t)1 << 52), "map_stats_update: tensor too large");
  const double v_bytes = 4.0 * B * (double)P, p_bytes = 4.0 * (double)P;
  DDPM_CHECK_ARG(!zm_overlap(mean, p_bytes, values, v_bytes) && !zm_overlap(m2, p_bytes, values, v_bytes) &&
                     !zm_overlap(mean, p_bytes, m2, p_bytes),
                 "map_stats_update: mean / m2 aliases another operand");
  const double n = (double)n_prev + (double)B;
  const float r_mean = (float)((double)B / n), r_m2 = (float)((double)n_prev * (double)B / n);
  const bool vec = (P & 3) == 0 && (((uintptr_t)values | (uintptr_t)mean | (uintptr_t)m2) & 15) == 0;
  const int64_t items = vec ? P / 4 : P;
  int64_t blocks = (items + kStatsBlock - 1) / kStatsBlock;
  if (blocks > 16384) blocks = 16384;
  ProfScope prof(s, "map_stats_update", 4.0 * B * (double)P, 4.0 * (double)P * (B + (n_prev ? 4 : 2)));
  if (vec)
    hipLaunchKernelGGL(map_stats_update_kernel<4>, dim3((unsigned)blocks), dim3(kStatsBlock), 0, s, values, B, P, n_prev == 0 ? 1 : 0,
                       r_mean, r_m2, mean, m2);
  else
    hipLaunchKernelGGL(map_stats_update_kernel<1>, dim3((unsigned)blocks), dim3(kStatsBlock), 0, s, values, B, P, n_prev == 0 ? 1 : 0,
                       r_mean, r_m2, mean, m2);
  DDPM_CHECK_LAUNCH();
  return 0;
}

// ---- Z-map of a row, averaged over the t-starts ---------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void map_zscore_kernel(const float *__restrict__ values, const float *__restrict__ mean,
                                                         const float *__restrict__ inv_std, float *__restrict__ out, int n_t,
                                                         int64_t P1, int64_t items, float weight) {
  struct alignas(4 * V) Vec { float v[V]; };
  const int64_t per_row = P1 / V;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += stride) {
    const int64_t bi = i / per_row, p = (i - bi * per_row) * V;
    const float *pv = values + bi * n_t * P1 + p;
    float acc[V];
    for (int t = 0; t < n_t; ++t) {
      const Vec x = *reinterpret_cast<const Vec *>(pv + (int64_t)t * P1);
      const Vec m = *reinterpret_cast<const Vec *>(mean + (int64_t)t * P1 + p);
      const Vec r = *reinterpret_cast<const Vec *>(inv_std + (int64_t)t * P1 + p);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float z = (x.v[j] - m.v[j]) * r.v[j];
        acc[j] = t == 0 ? z : acc[j] + z;
      }
    }
    Vec o;
#pragma unroll
    for (int j = 0; j < V; ++j) o.v[j] = weight * acc[j];
    *reinterpret_cast<Vec *>(out + bi * P1 + p) = o;
  }
}

int launch_map_zscore(const float *values, const float *mean, const float *inv_std, float *out, int B, int n_t, int64_t P1,
                      float weight, hipStream_t s) {
  DDPM_CHECK_ARG(values && mean && inv_std && out, "map_zscore: null pointer");
  DDPM_CHECK_ARG(B > 0, "map_zscore: B must be positive (got %d)", B);
  DDPM_CHECK_ARG(n_t > 0, "map_zscore: n_t must be positive (got %d)", n_t);
  DDPM_CHECK_ARG(P1 > 0, "map_zscore: P1 must be positive (got %lld)", (long long)P1);
  DDPM_CHECK_ARG((double)B * n_t * (double)P1 < 9.0e18, "map_zscore: tensor too large");
  const double o_bytes = 4.0 * B * (double)P1, t_bytes = 4.0 * n_t * (double)P1;
  DDPM_CHECK_ARG(!zm_overlap(out, o_bytes, values, t_bytes * B) && !zm_overlap(out, o_bytes, mean, t_bytes) &&
                     !zm_overlap(out, o_bytes, inv_std, t_bytes),
                 "map_zscore: out aliases an input");
  const bool vec = (P1 & 3) == 0 && (((uintptr_t)values | (uintptr_t)mean | (uintptr_t)inv_std | (uintptr_t)out) & 15) == 0;
  const int64_t items = vec ? (int64_t)B * (P1 / 4) : (int64_t)B * P1;
  ProfScope prof(s, "map_zscore", 3.0 * B * n_t * (double)P1, t_bytes * (B + 2) + o_bytes);
  if (vec)
    hipLaunchKernelGGL(map_zscore_kernel<4>, dim3(zm_blocks(items)), dim3(256), 0, s, values, mean, inv_std, out, n_t, P1, items,
                       weight);
  else
    hipLaunchKernelGGL(map_zscore_kernel<1>, dim3(zm_blocks(items)), dim3(256), 0, s, values, mean, inv_std, out, n_t, P1, items,
                       weight);
  DDPM_CHECK_LAUNCH();
  return 0;
}

// ---- leave-one-out Z-map of a validation row ------------------------------------------------------------------------------------------
// The row was counted in (n, mean, m2); taking it out again has a closed form per column:
//   d = v - mean;  dl = d * r1 (= v - the mean of the others);  q = max(m2 - d * dl, 0) (= the others' M2);  s = sqrt(q * r2)
// with r1 = n / (n - 1) and r2 = 1 / (n - 2) formed by the launcher in float64 and rounded once.  The divisor is floored at
// floor[t, c], one number per (t-start, channel): a thread's V columns lie in one channel (plane % V == 0), so it is one scalar
// per t.  fmaxf drops a NaN operand, but a NaN value is still in dl, the numerator: NaN in, NaN out.
template <int V>
__global__ __launch_bounds__(256) void map_zscore_loo_kernel(const float *__restrict__ values, const float *__restrict__ mean,
                                                             const float *__restrict__ m2, const float *__restrict__ floor,
                                                             float *__restrict__ out, int n_t, int64_t plane, int64_t items,
                                                             float r1, float r2, float weight) {
  struct alignas(4 * V) Vec { float v[V]; };
  const int64_t P1 = 2 * plane;
  const int64_t per_row = P1 / V;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += stride) {
    const int64_t bi = i / per_row, p = (i - bi * per_row) * V;
    const int c = p >= plane ? 1 : 0;
    const float *pv = values + bi * n_t * P1 + p;
    float acc[V];
    for (int t = 0; t < n_t; ++t) {
      const Vec x = *reinterpret_cast<const Vec *>(pv + (int64_t)t * P1);
      const Vec m = *reinterpret_cast<const Vec *>(mean + (int64_t)t * P1 + p);
      const Vec Q = *reinterpret_cast<const Vec *>(m2 + (int64_t)t * P1 + p);
      const float fl = floor[2 * t + c];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float d = x.v[j] - m.v[j];
        const float dl = d * r1;
        const float q = fmaxf(Q.v[j] - d * dl, 0.f);
        const float sd = sqrtf(q * r2);
        const float z = dl / fmaxf(sd, fl);
        acc[j] = t == 0 ? z : acc[j] + z;
      }
    }
    Vec o;
#pragma unroll
    for (int j = 0; j < V; ++j) o.v[j] = acc[j] * weight;
    *reinterpret_cast<Vec *>(out + bi * P1 + p) = o;
  }
}

int launch_map_zscore_loo(const float *values, const float *mean, const float *m2, const float *floor, float *out, int B, int n_t,
                          int64_t plane, int64_t n, float weight, hipStream_t s) {
  DDPM_CHECK_ARG(values && mean && m2 && floor && out, "map_zscore_loo: null pointer");
  DDPM_CHECK_ARG(B > 0, "map_zscore_loo: B must be positive (got %d)", B);
  DDPM_CHECK_ARG(n_t > 0, "map_zscore_loo: n_t must be positive (got %d)", n_t);
  DDPM_CHECK_ARG(plane > 0, "map_zscore_loo: plane must be positive (got %lld)", (long long)plane);
  DDPM_CHECK_ARG(n >= 3 && n < ((int64_t)1 << 52),
                 "map_zscore_loo: the statistics of the other rows need n >= 3 rows (got %lld)", (long long)n);
  DDPM_CHECK_ARG((double)B * n_t * 2.0 * (double)plane < 9.0e18, "map_zscore_loo: tensor too large");
  const int64_t P1 = 2 * plane;
  const double o_bytes = 4.0 * B * (double)P1, t_bytes = 4.0 * n_t * (double)P1, f_bytes = 8.0 * n_t;
  DDPM_CHECK_ARG(!zm_overlap(out, o_bytes, values, t_bytes * B) && !zm_overlap(out, o_bytes, mean, t_bytes) &&
                     !zm_overlap(out, o_bytes, m2, t_bytes) && !zm_overlap(out, o_bytes, floor, f_bytes),
                 "map_zscore_loo: out aliases an input");
  const float r1 = (float)((double)n / (double)(n - 1)), r2 = (float)(1.0 / (double)(n - 2));
  const bool vec = (plane & 3) == 0 && (((uintptr_t)values | (uintptr_t)mean | (uintptr_t)m2 | (uintptr_t)out) & 15) == 0;
  const int64_t items = vec ? (int64_t)B * (P1 / 4) : (int64_t)B * P1;
  ProfScope prof(s, "map_zscore_loo", 8.0 * B * n_t * (double)P1, t_bytes * (B + 2) + o_bytes + f_bytes);
  if (vec)
    hipLaunchKernelGGL(map_zscore_loo_kernel<4>, dim3(zm_blocks(items)), dim3(256), 0, s, values, mean, m2, floor, out, n_t, plane,
                       items, r1, r2, weight);
  else
    hipLaunchKernelGGL(map_zscore_loo_kernel<1>, dim3(zm_blocks(items)), dim3(256), 0, s, values, mean, m2, floor, out, n_t, plane,
                       items, r1, r2, weight);
  DDPM_CHECK_LAUNCH();
  return 0;
}

// ---- separable Gaussian smoothing, reflect boundary ------------------------------------------------------------------------------------
constexpr int kBlurTile = 32, kBlurMaxRadius = 16;
constexpr int kBlurSpan = kBlurTile + 2 * kBlurMaxRadius;  // 64: the widest staged extent
constexpr int kBlurPitch = kBlurSpan + 1;

// scipy's "reflect" (d c b a | a b c d | d c b a), for any offset: the signal is mirrored as often as it takes
__device__ __forceinline__ int refl(int i, int L) {
  const int period = 2 * L;
  int m = i % period;
  if (m < 0) m += period;
  return m < L ? m : period - 1 - m;
}

__global__ __launch_bounds__(256) void map_blur_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                       const float *__restrict__ taps, int radius, int H, int W, int tiles_x,
                                                       int tiles_y) {
  __shared__ float stage[kBlurSpan * kBlurPitch];   // [tile rows + halo][tile columns + halo] of the input
  __shared__ float hpass[kBlurTile * kBlurPitch];   // [tile rows][tile columns + halo] after the H pass
  __shared__ float tap[2 * kBlurMaxRadius + 1];
  const int tid = threadIdx.x;
  int tile = blockIdx.x;
  const int tx = tile % tiles_x;
  tile /= tiles_x;
  const int ty = tile % tiles_y;
  const int n = tile / tiles_y;
  const int y0 = ty * kBlurTile, x0 = tx * kBlurTile;
  const int span = kBlurTile + 2 * radius, ntap = 2 * radius + 1;
  const float *img = in + (int64_t)n * H * W;
  if (tid < ntap) tap[tid] = taps[tid];
  for (int e = tid; e < span * span; e += 256) {
    const int r = e / span, c = e - r * span;
    stage[r * kBlurPitch + c] = img[(int64_t)refl(y0 - radius + r, H) * W + refl(x0 - radius + c, W)];
  }
  __syncthreads();
  for (int e = tid; e < kBlurTile * span; e += 256) {  // H pass: row r of the tile, staged column c
    const int r = e / span, c = e - r * span;
    float acc = tap[0] * stage[r * kBlurPitch + c];
    for (int k = 1; k < ntap; ++k) acc += tap[k] * stage[(r + k) * kBlurPitch + c];
    hpass[r * kBlurPitch + c] = acc;
  }
  __syncthreads();
  for (int e = tid; e < kBlurTile * kBlurTile; e += 256) {  // W pass
    const int r = e / kBlurTile, c = e - r * kBlurTile;
    const int y = y0 + r, x = x0 + c;
    if (y >= H || x >= W) continue;
    float acc = tap[0] * hpass[r * kBlurPitch + c];
    for (int k = 1; k < ntap; ++k) acc += tap[k] * hpass[r * kBlurPitch + c + k];
    out[((int64_t)n * H + y) * W + x] = acc;
  }
}

int launch_map_blur(const float *in, float *out, const float *taps, int radius, int N, int H, int W, hipStream_t s) {
  DDPM_CHECK_ARG(in && out && taps, "map_blur: null pointer");
  DDPM_CHECK_ARG(radius >= 0, "map_blur: radius must not be negative (got %d)", radius);
  DDPM_CHECK_ARG(radius <= kBlurMaxRadius, "map_blur: radius %d is above the maximum of %d (sigma < 4.125 at truncate 4)", radius,
                 kBlurMaxRadius);
  DDPM_CHECK_ARG(N > 0 && H > 0 && W > 0, "map_blur: N, H and W must be positive (got %d, %d, %d)", N, H, W);
  DDPM_CHECK_ARG(H <= (1 << 20) && W <= (1 << 20), "map_blur: extents up to 2^20 (got %d x %d)", H, W);
  const int tiles_x = (W + kBlurTile - 1) / kBlurTile, tiles_y = (H + kBlurTile - 1) / kBlurTile;
  const double tiles = (double)N * tiles_x * tiles_y;
  DDPM_CHECK_ARG(tiles < 2147483647.0, "map_blur: too many tiles");
  const double bytes = 4.0 * N * (double)H * W;
  DDPM_CHECK_ARG(!zm_overlap(out, bytes, in, bytes) && !zm_overlap(out, bytes, taps, 4.0 * (2 * radius + 1)),
                 "map_blur: out aliases an input (in place is not built)");
  ProfScope prof(s, "map_blur", 4.0 * (2 * radius + 1) * N * (double)H * W, 2.0 * bytes);
  hipLaunchKernelGGL(map_blur_kernel, dim3((unsigned)tiles), dim3(256), 0, s, in, out, taps, radius, H, W, tiles_x, tiles_y);
  DDPM_CHECK_LAUNCH();
  return 0;
}

// ---- 3-D smoothing: the two in-plane passes above over the N D planes, then the depth pass --------------------------------------------
// Depth pass: out[n, d, c] = sum_k taps[k] in[n, refl(d + k - radius, D), c] over the columns c of the flattened plane (P = H W
// of them: w runs across the lanes, so every load and store is a contiguous run of 64 floats).  A workgroup of four waves owns
// 64 adjacent columns and streams down D in steps of 32 planes.  The window lives in an LDS ring of 128 rows x 64 columns (32 KB;
// a lane reads its own column: bank = lane, no conflict): the row of virtual depth j (-radius <= j < D + radius, read from
// plane refl(j, D)) sits in slot (j + radius) mod 128 (counted from the workgroup's first plane).  A step adds its 32 new rows (eight per wave, fetched into registers
// one step ahead, so 8 KB per workgroup fly during the arithmetic: with 16 rows per step the pass ran at 1.0 TB/s on one 128^3
// volume pair, bound by the bytes in flight, profiles/anomaly_volume_maps.md), then every wave sums eight output planes.  One
// barrier per step: the rows step i + 1 writes take the slots of rows below d0 - 64 + radius, which step i no longer reads, and a
// wave reaches the writes of step i + 2 (slots of rows d0 - 64 + radius .. d0 - 33 + radius, all below d0 - radius) only behind
// the barrier of step i + 1.  Every plane is read once from memory, the planes the reflection repeats at the two ends aside.
// A workgroup's steps are one chain of dependent waits, so a launch with few column tiles (one 128^3 volume pair: 512) is bound by
// that chain, not by bytes: while there are fewer than kDepthMinBlocks workgroups the launcher cuts D into segments of a multiple
// of 32 planes, each streamed by a workgroup of its own (its 2 radius halo planes are read again, from the caches).  The bits
// of an output do not depend on the cut.
constexpr int kDepthCols = 64, kDepthStep = 32, kDepthRing = 128, kDepthWaves = 4, kDepthMinBlocks = 2048;
static_assert(2 * kDepthStep + 2 * kBlurMaxRadius <= kDepthRing, "the depth ring must hold two steps and their halo");

__global__ __launch_bounds__(256) void map_blur_depth_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                             const float *__restrict__ taps, int radius, int D, int64_t P,
                                                             int64_t tiles, int seg, int segs) {
  __shared__ float ring[kDepthRing * kDepthCols];
  __shared__ float tap[2 * kBlurMaxRadius + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sg = (int)(blockIdx.x % segs);
  const int64_t nt = blockIdx.x / segs, n = nt / tiles, tile = nt - n * tiles;
  const int d_lo = sg * seg, d_hi = min(D, d_lo + seg);  // this workgroup's output planes
  const int64_t c = tile * kDepthCols + lane;
  const bool live = c < P;
  const float *vin = in + n * D * P + (live ? c : 0);
  float *vout = out + n * D * P + (live ? c : 0);
  const int ntap = 2 * radius + 1, first = d_lo - radius, last = d_hi + radius;  // virtual rows first .. last - 1: slot (j - first) mod ring
  if (tid < ntap) tap[tid] = taps[tid];
  for (int j = first + wave; j < d_lo + radius; j += kDepthWaves)  // the halo above the first step's rows
    ring[((j - first) & (kDepthRing - 1)) * kDepthCols + lane] = live ? vin[(int64_t)refl(j, D) * P] : 0.f;
  constexpr int kPer = kDepthStep / kDepthWaves;
  float next[kPer];
#pragma unroll
  for (int q = 0; q < kPer; ++q) {  // the first step's own rows: radius .. radius + kDepthStep - 1
    const int j = d_lo + radius + wave + q * kDepthWaves;
    next[q] = live && j < last ? vin[(int64_t)refl(j, D) * P] : 0.f;
  }
  for (int d0 = d_lo; d0 < d_hi; d0 += kDepthStep) {
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const int j = d0 + radius + wave + q * kDepthWaves;
      if (j < last) ring[((j - first) & (kDepthRing - 1)) * kDepthCols + lane] = next[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const int j = d0 + kDepthStep + radius + wave + q * kDepthWaves;
      next[q] = live && j < last ? vin[(int64_t)refl(j, D) * P] : 0.f;
    }
    for (int d = d0 + wave; d < min(d0 + kDepthStep, d_hi); d += kDepthWaves) {
      float acc = tap[0] * ring[((d - d_lo) & (kDepthRing - 1)) * kDepthCols + lane];  // virtual row d - radius: slot d - d_lo
      for (int k = 1; k < ntap; ++k) acc += tap[k] * ring[((d - d_lo + k) & (kDepthRing - 1)) * kDepthCols + lane];
      if (live) vout[(int64_t)d * P] = acc;
    }
  }
}

int launch_map_blur3d(const float *in, float *out, float *tmp, const float *taps, int radius, int N, int D, int H, int W,
                      hipStream_t s) {
  DDPM_CHECK_ARG(in && out && tmp && taps, "map_blur3d: null pointer");
  DDPM_CHECK_ARG(radius >= 0, "map_blur3d: radius must not be negative (got %d)", radius);
  DDPM_CHECK_ARG(radius <= kBlurMaxRadius, "map_blur3d: radius %d is above the maximum of %d (sigma < 4.125 at truncate 4)", radius,
                 kBlurMaxRadius);
  DDPM_CHECK_ARG(N > 0 && D > 0 && H > 0 && W > 0, "map_blur3d: N, D, H and W must be positive (got %d, %d, %d, %d)", N, D, H, W);
  DDPM_CHECK_ARG(D <= (1 << 20) && H <= (1 << 20) && W <= (1 << 20), "map_blur3d: extents up to 2^20 (got %d x %d x %d)", D, H, W);
  DDPM_CHECK_ARG((double)N * D < 2147483647.0, "map_blur3d: too many planes");
  const int64_t P = (int64_t)H * W, tiles = (P + kDepthCols - 1) / kDepthCols;
  DDPM_CHECK_ARG((double)N * (double)tiles < 2147483647.0, "map_blur3d: too many column tiles");
  const double bytes = 4.0 * N * D * (double)P, t_bytes = 4.0 * (2 * radius + 1);
  DDPM_CHECK_ARG(!zm_overlap(out, bytes, in, bytes) && !zm_overlap(out, bytes, taps, t_bytes) && !zm_overlap(tmp, bytes, in, bytes) &&
                     !zm_overlap(tmp, bytes, out, bytes) && !zm_overlap(tmp, bytes, taps, t_bytes),
                 "map_blur3d: out or tmp aliases another operand (in place is not built)");
  const int rc = launch_map_blur(in, tmp, taps, radius, N * D, H, W, s);  // the H pass, then the W pass, plane by plane
  if (rc != 0) return rc;
  int seg = D;  // planes per workgroup: all of D, or a multiple of kDepthStep while the launch is short of workgroups
  while (seg > kDepthStep && (double)N * (double)tiles * ((D + seg - 1) / seg) < kDepthMinBlocks)
    seg = (seg / 2 + kDepthStep - 1) / kDepthStep * kDepthStep;
  const int segs = (D + seg - 1) / seg;
  DDPM_CHECK_ARG((double)N * (double)tiles * segs < 2147483647.0, "map_blur3d: too many workgroups");
  ProfScope prof(s, "map_blur_depth", 2.0 * (2 * radius + 1) * N * D * (double)P, 2.0 * bytes);
  hipLaunchKernelGGL(map_blur_depth_kernel, dim3((unsigned)(N * tiles * segs)), dim3(256), 0, s, tmp, out, taps, radius, D, P, tiles,
                     seg, segs);
  DDPM_CHECK_LAUNCH();
  return 0;
}

}  // namespace ddpm

using namespace ddpm;

extern "C" int ddpm_map_blur3d_f32(const float *in, float *out, float *tmp, const float *taps, int radius, int N, int D, int H, int W,
                                   ddpm_stream_t stream) {
  return launch_map_blur3d(in, out, tmp, taps, radius, N, D, H, W, as_stream(stream));
}

extern "C" int ddpm_map_stats_update_f32(const float *values, int B, int64_t P, int64_t n_prev, float *mean, float *m2,
                                         ddpm_stream_t stream) {
  return launch_map_stats_update(values, B, P, n_prev, mean, m2, as_stream(stream));
}

extern "C" int ddpm_map_zscore_f32(const float *values, const float *mean, const float *inv_std, float *out, int B, int n_t,
                                   int64_t P1, float weight, ddpm_stream_t stream) {
  return launch_map_zscore(values, mean, inv_std, out, B, n_t, P1, weight, as_stream(stream));
}

extern "C" int ddpm_map_zscore_loo_f32(const float *values, const float *mean, const float *m2, const float *floor, float *out,
                                       int B, int n_t, int64_t plane, int64_t n, float weight, ddpm_stream_t stream) {
  return launch_map_zscore_loo(values, mean, m2, floor, out, B, n_t, plane, n, weight, as_stream(stream));
}

extern "C" int ddpm_map_blur_f32(const float *in, float *out, const float *taps, int radius, int N, int H, int W,
                                 ddpm_stream_t stream) {
  return launch_map_blur(in, out, taps, radius, N, H, W, as_stream(stream));
}
