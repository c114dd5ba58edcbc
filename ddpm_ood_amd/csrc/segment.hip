// Predicted segmentations from anomaly maps (only with --pixel_segment 1).
//   map_median   3 x 3 or 5 x 5 median of [N, H, W] planes, scipy.ndimage's mode="reflect" boundary, np.sort's order
//   map_segment  per image and threshold: the components of {v > thr} with at least min_size pixels as a uint8 plane, its pixel
//                counts against the mask, its component counts against the mask's regions, what the size filter dropped
//
// Median.  One workgroup of 256 threads per 64 x 16 tile of a plane.  The tile and its halo go from HBM into LDS once, as the
// integer KEY of each value: the bits of a non-negative float with the sign bit set, those of a negative float inverted, every
// NaN (of either sign) 0xffffffff.  Unsigned order of the keys is np.sort's order -inf < finite < +inf < NaN (and -0 < +0, which
// pins nothing: the zeros are equal), and the key's inverse gives back the bits of the value, so the output is an input value
// (a NaN: 0x7fffffff).  A thread owns 4 pixels of one column (rows ty, ty + 4, ...): a wave reads 64 consecutive dwords of a
// row of the tile, no bank is asked twice.  Selection: the window's values in registers, v_min_u32 / v_max_u32 only.  Of
// n = size^2 / 2 + 2 values neither the smallest nor the largest can be the median of all size^2 (n - 1 values lie on one side
// of it, more than half); both are dropped, the next value joins, and so on down to three values, whose middle one is the
// median.  select_minmax brings the smallest to slot 0 and the largest to slot n - 1 with compare-exchanges at constant
// indices: pairs (i, n - 1 - i), then the minimum of the lower and the maximum of the upper half.  Everything unrolls; there is
// no dynamically indexed array and no scratch (profiles/segmentation.md has the resource usage).
//
// Segment.  One workgroup of 1 024 threads per (image, threshold), the plane at most 128 x 128, as map_component_counts.  After
// cc_link / cc_compact (regions_common.h) every component has a rank 1 .. R <= 8 192.  LDS beside the 32 KB of parents:
//   size[rank]   16-bit counters, two to a dword (16 KB): a component has at most 16 384 pixels, so the 32-bit add of a count
//                shifted into its half never carries into the other half.  Added per wave and stretch of equal ranks among its
//                64 consecutive pixels (a ballot of the stretches' first lanes gives their lengths): the all-ones plane is 256
//                additions to one address, not 16 384
//   touch[rank]  one bit: the component holds a masked pixel;   hit[region]  one bit: the region holds a kept pixel
// 32 KB + 16 KB + 1 KB + 2 KB + the reduction's 512 B: 52 KB, inside the 64 KB every CDNA part gives a workgroup.
// No communication between workgroups, no global atomics, every output element written with a plain store, nothing depends
// on what an output held before.  Should a bound of the labelling run out (it cannot), the (image, threshold)'s integers are -1.
#include "median_common.h"
#include "regions_common.h"

namespace ddpm {

// ---- median -------------------------------------------------------------------------------------------------------------------
constexpr int kMedTileW = 64;
constexpr int kMedTileH = 16;
constexpr int kMedBlock = 256;
constexpr int kMedRows = kMedTileH / (kMedBlock / kMedTileW);  // output rows per thread

template <int R>
__global__ __launch_bounds__(kMedBlock) void map_median_kernel(const float *__restrict__ in, float *__restrict__ out, int H, int W,
                                                               int tiles_x, int tiles_y) {
  constexpr int S = 2 * R + 1, M = S * S, LW = kMedTileW + 2 * R, LH = kMedTileH + 2 * R;
  __shared__ uint32_t tile[LH * LW];
  const int tid = threadIdx.x;
  const int per_plane = tiles_x * tiles_y;
  const int n = blockIdx.x / per_plane, t = blockIdx.x - n * per_plane;
  const int y0 = (t / tiles_x) * kMedTileH, x0 = (t % tiles_x) * kMedTileW;
  const float *src = in + (int64_t)n * H * W;
  float *dst = out + (int64_t)n * H * W;
  for (int e = tid; e < LH * LW; e += kMedBlock) {
    const int ly = e / LW, lx = e - ly * LW;
    tile[e] = med_key(src[(int64_t)med_reflect(y0 + ly - R, H) * W + med_reflect(x0 + lx - R, W)]);
  }
  __syncthreads();
  const int tx = tid & (kMedTileW - 1), ty = tid / kMedTileW;
  if (x0 + tx >= W) return;
#pragma unroll
  for (int j = 0; j < kMedRows; ++j) {
    const int ly = ty + j * (kMedBlock / kMedTileW);
    if (y0 + ly < H) {
      uint32_t v[M];
#pragma unroll
      for (int dy = 0; dy < S; ++dy)
#pragma unroll
        for (int dx = 0; dx < S; ++dx) v[dy * S + dx] = tile[(ly + dy) * LW + tx + dx];
      dst[(int64_t)(y0 + ly) * W + x0 + tx] = med_value(select_median<M / 2 + 2>(v));
    }
  }
}

int launch_map_median(const float *in, float *out, int size, int N, int H, int W, hipStream_t s) {
  DDPM_CHECK_ARG(in && out, "map_median: null pointer");
  DDPM_CHECK_ARG(N > 0 && H > 0 && W > 0, "map_median: N, H and W must be positive (got %d, %d, %d)", N, H, W);
  DDPM_CHECK_ARG(size == 3 || size == 5, "map_median: size must be 3 or 5 (got %d)", size);
  DDPM_CHECK_ARG(H <= (1 << 24) && W <= (1 << 24) && (double)H * W < 2147483648.0,
                 "map_median: a plane of %d x %d pixels is above 2^31 pixels", H, W);
  const int tiles_x = (W + kMedTileW - 1) / kMedTileW, tiles_y = (H + kMedTileH - 1) / kMedTileH;
  DDPM_CHECK_ARG((double)N * tiles_x * tiles_y < 2147483648.0, "map_median: N x tiles must stay below 2^31 (got %d x %d x %d)", N,
                 tiles_y, tiles_x);
  DDPM_CHECK_ARG(((uintptr_t)in & 3) == 0 && ((uintptr_t)out & 3) == 0, "map_median: maps / out must be 4-byte aligned");
  const double elems = (double)N * H * W;
  DDPM_CHECK_ARG(!pm_overlap(out, 4.0 * elems, in, 4.0 * elems), "map_median: out aliases the input (not in place)");
  ProfScope prof(s, "map_median", 0.0, 8.0 * elems);
  const dim3 grid((unsigned)(N * tiles_x * tiles_y));
  if (size == 3)
    hipLaunchKernelGGL(map_median_kernel<1>, grid, dim3(kMedBlock), 0, s, in, out, H, W, tiles_x, tiles_y);
  else
    hipLaunchKernelGGL(map_median_kernel<2>, grid, dim3(kMedBlock), 0, s, in, out, H, W, tiles_x, tiles_y);
  DDPM_CHECK_LAUNCH();
  return 0;
}

// ---- segment ------------------------------------------------------------------------------------------------------------------
constexpr int kSgMaxRanks = kRgMaxPixels / 2;  // a component of one pixel needs a pixel of background beside it (connectivity 4)
constexpr int kSgInts = 8;                     // TP, FP, FN; hit, pred, false_pred; removed components, removed pixels

__global__ __launch_bounds__(kRgBlock) void map_segment_kernel(const float *__restrict__ maps, const uint8_t *__restrict__ masks,
                                                               const int32_t *__restrict__ labels, const int32_t *__restrict__ regions,
                                                               int H, int W, const float *__restrict__ thresholds, int K, int min_size,
                                                               int conn, uint8_t *__restrict__ seg, int32_t *__restrict__ pixels,
                                                               int32_t *__restrict__ components, int32_t *__restrict__ removed) {
  __shared__ CcShared sh;
  __shared__ uint32_t size[kSgMaxRanks / 2 + 1];   // per rank 1 .. R, 16 bits each: the component's pixels
  __shared__ uint32_t touch[kSgMaxRanks / 32 + 1];  // per rank: the component holds a masked pixel
  __shared__ uint32_t hit[kRgMaxPixels / 32 + 1];   // per ground-truth region 1 .. R: it holds a kept pixel
  __shared__ int red[kRgWaves][kSgInts];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, P = H * W;
  const int n = blockIdx.x / K, k = blockIdx.x - n * K;
  const float *row = maps + (int64_t)n * P;
  const uint8_t *mrow = masks + (int64_t)n * P;
  const int32_t *lrow = labels + (int64_t)n * P;
  uint8_t *srow = seg + (int64_t)blockIdx.x * P;
  const int Rgt = min(max(regions[n], 0), P);
  for (int j = tid; j < kSgMaxRanks / 2 + 1; j += kRgBlock) size[j] = 0u;
  for (int j = tid; j < kRgMaxPixels / 32 + 1; j += kRgBlock) {
    if (j < kSgMaxRanks / 32 + 1) touch[j] = 0u;
    hit[j] = 0u;
  }
  cc_link(sh, PredGt(row, thresholds[k]), H, W, conn);  // (barriers inside: the zeroes above are in place)
  const int R = min(cc_compact(sh, P), kSgMaxRanks);
  const volatile uint16_t *par = reinterpret_cast<const volatile uint16_t *>(sh.words);
  // the sizes: every wave over 64 consecutive pixels at a time, one addition per stretch of equal ranks
  for (int base = 0; base < P; base += kRgBlock) {  // (the same trip count in every lane: the ballot sees whole waves)
    const int i = base + tid;
    uint32_t r = 0u;
    if (i < P) {
      const uint32_t p = par[i];
      if (p != kRgBg) r = ((p & kRgRootTag) ? p : (uint32_t)par[p]) & (kRgRootTag - 1u);
    }
    const uint32_t before = (uint32_t)__shfl_up((int)r, 1, 64);
    const bool first = lane == 0 || before != r;
    const unsigned long long firsts = __ballot(first);
    if (first && r != 0u && r <= (uint32_t)kSgMaxRanks) {
      const unsigned long long above = lane == 63 ? 0ull : firsts >> (lane + 1);
      const uint32_t len = above ? (uint32_t)__ffsll(above) : (uint32_t)(64 - lane);
      atomicAdd(&size[r >> 1], len << ((r & 1u) * 16u));
    }
  }
  __syncthreads();
  int c[kSgInts] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = tid; i < P; i += kRgBlock) {
    const uint32_t p = par[i];
    const bool m = mrow[i] != 0;
    bool kept = false;
    if (p != kRgBg) {
      const uint32_t r = min(((p & kRgRootTag) ? p : (uint32_t)par[p]) & (kRgRootTag - 1u), (uint32_t)kSgMaxRanks);
      kept = (int)((size[r >> 1] >> ((r & 1u) * 16u)) & 0xffffu) >= min_size;
      if (m) atomicOr(&touch[r >> 5], 1u << (r & 31u));
      if (kept) {
        const int l = lrow[i];
        if (l >= 1 && l <= Rgt) atomicOr(&hit[l >> 5], 1u << (l & 31));
      }
    }
    srow[i] = kept ? 1 : 0;
    c[0] += kept && m ? 1 : 0;
    c[1] += kept && !m ? 1 : 0;
    c[2] += !kept && m ? 1 : 0;
  }
  __syncthreads();
  for (int j = tid; j < kRgMaxPixels / 32 + 1; j += kRgBlock) c[3] += __popc(hit[j]);
  for (int r = 1 + tid; r <= R; r += kRgBlock) {
    const int sz = (int)((size[r >> 1] >> ((r & 1) * 16)) & 0xffffu);
    if (sz >= min_size) {
      ++c[4];
      c[5] += (touch[r >> 5] >> (r & 31)) & 1u ? 0 : 1;
    } else {
      ++c[6];
      c[7] += sz;
    }
  }
#pragma unroll
  for (int j = 0; j < kSgInts; ++j) {
    int v = c[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[wave][j] = v;
  }
  __syncthreads();
  if (tid < kSgInts) {
    int v = 0;
#pragma unroll
    for (int w = 0; w < kRgWaves; ++w) v += red[w][tid];
    if (sh.fail) v = -1;
    if (tid < 3)
      pixels[(int64_t)blockIdx.x * 3 + tid] = v;
    else if (tid < 6)
      components[(int64_t)blockIdx.x * 3 + tid - 3] = v;
    else
      removed[(int64_t)blockIdx.x * 2 + tid - 6] = v;
  }
}

int launch_map_segment(const float *maps, const uint8_t *masks, const int32_t *labels, const int32_t *regions, int N, int H, int W,
                       const float *thresholds, int K, int min_size, int conn, uint8_t *seg, int32_t *pixels, int32_t *components,
                       int32_t *removed, hipStream_t s) {
  const char *op = "map_segment";
  DDPM_CHECK_ARG(maps && masks && labels && regions && thresholds && seg && pixels && components && removed, "%s: null pointer", op);
  DDPM_CHECK_ARG(N > 0 && H > 0 && W > 0, "%s: N, H and W must be positive (got %d, %d, %d)", op, N, H, W);
  DDPM_CHECK_ARG((int64_t)H * (int64_t)W <= kRgMaxPixels, "%s: a plane of %d x %d pixels is above the maximum of %d (128 x 128): "
                 "its 16-bit labels fill the LDS", op, H, W, kRgMaxPixels);
  DDPM_CHECK_ARG(conn == 4 || conn == 8, "%s: connectivity must be 4 or 8 (got %d)", op, conn);
  DDPM_CHECK_ARG(K >= 1 && K <= kCountsMaxK, "%s: K must lie in 1 .. %d (got %d)", op, kCountsMaxK, K);
  DDPM_CHECK_ARG(min_size >= 1 && min_size <= kRgMaxPixels, "%s: min_size must lie in 1 .. %d (got %d)", op, kRgMaxPixels, min_size);
  DDPM_CHECK_ARG((double)N * K < 2147483648.0, "%s: N * K must stay below 2^31 (got %d x %d)", op, N, K);
  DDPM_CHECK_ARG(((uintptr_t)maps & 3) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)regions & 3) == 0 &&
                     ((uintptr_t)thresholds & 3) == 0 && ((uintptr_t)pixels & 3) == 0 && ((uintptr_t)components & 3) == 0 &&
                     ((uintptr_t)removed & 3) == 0,
                 "%s: maps / labels / regions / thresholds / pixels / components / removed must be 4-byte aligned", op);
  const double elems = (double)N * H * W;
  const void *in[5] = {maps, masks, labels, regions, thresholds};
  const double in_bytes[5] = {4.0 * elems, elems, 4.0 * elems, 4.0 * N, 4.0 * K};
  const void *out[4] = {seg, pixels, components, removed};
  const double out_bytes[4] = {elems * K, 12.0 * N * K, 12.0 * N * K, 8.0 * N * K};
  for (int o = 0; o < 4; ++o) {
    for (int i = 0; i < 5; ++i)
      DDPM_CHECK_ARG(!pm_overlap(out[o], out_bytes[o], in[i], in_bytes[i]), "%s: an output aliases an input", op);
    for (int q = o + 1; q < 4; ++q)
      DDPM_CHECK_ARG(!pm_overlap(out[o], out_bytes[o], out[q], out_bytes[q]), "%s: two outputs alias each other", op);
  }
  ProfScope prof(s, op, 0.0, 10.0 * elems * K + 32.0 * N * K);
  hipLaunchKernelGGL(map_segment_kernel, dim3((unsigned)(N * K)), dim3(kRgBlock), 0, s, maps, masks, labels, regions, H, W, thresholds,
                     K, min_size, conn, seg, pixels, components, removed);
  DDPM_CHECK_LAUNCH();
  return 0;
}

}  // namespace ddpm

using namespace ddpm;

extern "C" int ddpm_map_median_f32(const float *maps, float *out, int size, int N, int H, int W, ddpm_stream_t stream) {
  return launch_map_median(maps, out, size, N, H, W, as_stream(stream));
}

extern "C" int ddpm_map_segment_f32(const float *maps, const uint8_t *masks, const int32_t *labels, const int32_t *regions, int N,
                                    int H, int W, const float *thresholds, int K, int min_size, int connectivity, uint8_t *seg,
                                    int32_t *pixels, int32_t *components, int32_t *removed, ddpm_stream_t stream) {
  return launch_map_segment(maps, masks, labels, regions, N, H, W, thresholds, K, min_size, connectivity, seg, pixels, components,
                            removed, as_stream(stream));
}
