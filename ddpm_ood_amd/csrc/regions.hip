// Region-level evaluation of anomaly maps (only with --pixel_regions 1).
//   map_label             connected components of a batch of planes (mask != 0, or v > thr), numbered as scipy.ndimage.label does
//   map_region_overlap    per bin, the sum over the ground-truth regions of (the region's pixels in the bin) / (its area)
//   map_component_counts  per image and threshold: regions hit, predicted components, predicted components off every region
// One workgroup of 1 024 threads per image (per image and threshold for the counts), the plane at most 128 x 128 = 16 384
// pixels.  No communication between workgroups, no global atomics, every output element written with a plain store, nothing
// depends on what an output held before (but `total` with accumulate != 0).
//
// Labelling (cc_link, cc_compact): a union-find forest over the plane in LDS, one 16-bit parent per pixel (two to a dword:
// 32 KB), the background 0xffff.  A parent is never above its pixel, so every walk towards a root descends and a root is the
// smallest flat index of its tree.
//   1  par[i] = i - 1 if the left neighbour is inside, else i; pointer jumping makes every pixel of a horizontal run point at
//      the run's first pixel (<= ceil(log2 W) barrier rounds).
//   2  one union per pair of touching runs of neighbouring rows, issued by the first pixel at which the lower run meets the
//      upper one.  A union walks to both roots and hangs the larger below the smaller with a 16-bit minimum (a CAS on the
//      dword that holds the half); all unions of the plane run concurrently between two barriers, lock-free: the serpentine of
//      8 000 pixels takes these two barriers, not 8 000 rounds.
//   3  the runs' first pixels walk to their roots, then every other pixel follows its run's first pixel (two barriers).
//   4  the roots are numbered 1 .. R in ascending flat index by a prefix count over the root flags (contiguous chunk per
//      thread, shuffle scan in the wave, the sixteen wave totals through LDS); a root's number replaces its parent, tagged by
//      bit 15 (R <= 8 192 and an index <= 16 383 leave the bit free).
// Termination: every loop below carries a bound that follows from the algorithm and stands in its condition; should a bound of
// the lock-free part ever run out (it cannot, see cc_min16 / cc_union), the image's `regions` entry is -1.
//
// Overlap: per region, in ascending order, an integer histogram in LDS (ds_add_u32: independent of the order), its area by a
// fixed-order integer reduction, then acc[b] += (double)h[b] / (double)area in the registers of the thread that owns the bin;
// a second launch adds the images' rows to `total` in ascending order.  Divisions and additions only.  One pass over the plane
// per region: meant for the handful of regions a mask has, correct for any number.
#include "pixel_common.h"
#include "regions_common.h"

namespace ddpm {

constexpr int kOvSlots = (kHistMaxBins + 1) / kRgBlock;  // bins per thread of the overlap kernel
static_assert(kOvSlots * kRgBlock == kHistMaxBins + 1, "the overlap kernel's threads own the bins evenly");

template <class Pred, class T>
__global__ __launch_bounds__(kRgBlock) void map_label_kernel(const T *__restrict__ src, float thr, int H, int W, int conn,
                                                             int32_t *__restrict__ labels, int32_t *__restrict__ regions) {
  __shared__ CcShared sh;
  const int P = H * W;
  const T *row = src + (int64_t)blockIdx.x * P;
  cc_link(sh, Pred(row, thr), H, W, conn);
  const int R = cc_compact(sh, P);
  const volatile uint16_t *par = reinterpret_cast<const volatile uint16_t *>(sh.words);
  int32_t *out = labels + (int64_t)blockIdx.x * P;
  for (int i = threadIdx.x; i < P; i += kRgBlock) {
    const uint32_t p = par[i];
    out[i] = p == kRgBg ? 0 : (int32_t)(((p & kRgRootTag) ? p : (uint32_t)par[p]) & (kRgRootTag - 1u));
  }
  if (threadIdx.x == 0) regions[blockIdx.x] = sh.fail ? -1 : R;
}

static int check_plane(const char *op, int N, int H, int W, int conn) {
  DDPM_CHECK_ARG(N > 0 && H > 0 && W > 0, "%s: N, H and W must be positive (got %d, %d, %d)", op, N, H, W);
  DDPM_CHECK_ARG((int64_t)H * (int64_t)W <= kRgMaxPixels, "%s: a plane of %d x %d pixels is above the maximum of %d (128 x 128): "
                 "its 16-bit labels fill the LDS", op, H, W, kRgMaxPixels);
  DDPM_CHECK_ARG(conn == 4 || conn == 8, "%s: connectivity must be 4 or 8 (got %d)", op, conn);
  return 0;
}

template <class Pred, class T>
static int launch_map_label(const char *op, const T *src, float thr, int N, int H, int W, int conn, int32_t *labels, int32_t *regions,
                            hipStream_t s) {
  DDPM_CHECK_ARG(src && labels && regions, "%s: null pointer", op);
  if (int rc = check_plane(op, N, H, W, conn)) return rc;
  DDPM_CHECK_ARG(((uintptr_t)src & (sizeof(T) - 1)) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)regions & 3) == 0,
                 "%s: maps / labels / regions must be 4-byte aligned", op);
  const double elems = (double)N * H * W;
  DDPM_CHECK_ARG(!pm_overlap(labels, 4.0 * elems, src, sizeof(T) * elems) && !pm_overlap(regions, 4.0 * N, src, sizeof(T) * elems) &&
                     !pm_overlap(labels, 4.0 * elems, regions, 4.0 * N),
                 "%s: labels / regions alias another operand", op);
  ProfScope prof(s, op, 0.0, (sizeof(T) + 4.0) * elems + 4.0 * N);
  hipLaunchKernelGGL((map_label_kernel<Pred, T>), dim3((unsigned)N), dim3(kRgBlock), 0, s, src, thr, H, W, conn, labels, regions);
  DDPM_CHECK_LAUNCH();
  return 0;
}

// ---- region overlap ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRgBlock) void map_region_overlap_kernel(const float *__restrict__ maps, const int32_t *__restrict__ labels,
                                                                      const int32_t *__restrict__ regions, int P, float lo,
                                                                      float inv_step, int nbins, double *__restrict__ scratch) {
  __shared__ uint32_t h[kHistMaxBins + 1];
  __shared__ int red[2][kRgWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, width = nbins + 1;
  const float *row = maps + (int64_t)blockIdx.x * P;
  const int32_t *lrow = labels + (int64_t)blockIdx.x * P;
  const int R = min(max(regions[blockIdx.x], 0), P);  // (labels above `regions` are no region's; a plane has at most P regions)
  double acc[kOvSlots];
#pragma unroll
  for (int s = 0; s < kOvSlots; ++s) {
    acc[s] = 0.0;
    h[tid + s * kRgBlock] = 0u;
  }
  __syncthreads();
  for (int r = 1; r <= R; ++r) {  // one round per region: at most P
    int cnt = 0;
    for (int i = tid; i < P; i += kRgBlock) {
      if (lrow[i] == r) {
        atomicAdd(&h[pm_bin(row[i], lo, inv_step, nbins)], 1u);
        ++cnt;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) red[r & 1][wave] = cnt;  // (two sets: a wave may write round r + 1 while another still reads round r)
    __syncthreads();
    int area = 0;
#pragma unroll
    for (int w = 0; w < kRgWaves; ++w) area += red[r & 1][w];
    if (area > 0) {  // (the region's pixels, NaN ones included)
      const double a = (double)area;
#pragma unroll
      for (int s = 0; s < kOvSlots; ++s) {
        const int b = tid + s * kRgBlock;
        const uint32_t u = h[b];
        if (u) {  // (adding the zero of an empty bin changes nothing)
          acc[s] += (double)u / a;
          h[b] = 0u;
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int s = 0; s < kOvSlots; ++s) {
    const int b = tid + s * kRgBlock;
    if (b < width) scratch[(int64_t)blockIdx.x * width + b] = acc[s];
  }
}

__global__ __launch_bounds__(256) void map_region_overlap_sum_kernel(const double *__restrict__ scratch, int N, int width, int accumulate,
                                                                     double *__restrict__ total) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= width) return;
  double t = accumulate ? total[b] : 0.0;
  for (int n = 0; n < N; ++n) t += scratch[(int64_t)n * width + b];
  total[b] = t;
}

int launch_map_region_overlap(const float *maps, const int32_t *labels, const int32_t *regions, int N, int P, float lo, float inv_step,
                              int nbins, double *scratch, double *total, int accumulate, hipStream_t s) {
  DDPM_CHECK_ARG(maps && labels && regions && scratch && total, "map_region_overlap: null pointer");
  DDPM_CHECK_ARG(N > 0 && P > 0, "map_region_overlap: N and P must be positive (got %d, %d)", N, P);
  DDPM_CHECK_ARG(P <= kRgMaxPixels, "map_region_overlap: a plane of %d pixels is above the maximum of %d (128 x 128)", P, kRgMaxPixels);
  DDPM_CHECK_ARG(nbins >= 1 && nbins <= kHistMaxBins, "map_region_overlap: nbins must lie in 1 .. %d (got %d)", kHistMaxBins, nbins);
  DDPM_CHECK_ARG(inv_step > 0.0f && inv_step <= 3.402823466e+38f && lo == lo && lo - lo == 0.0f,
                 "map_region_overlap: lo must be finite and inv_step positive and finite (got %g, %g)", (double)lo, (double)inv_step);
  DDPM_CHECK_ARG(((uintptr_t)maps & 3) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)regions & 3) == 0 &&
                     ((uintptr_t)scratch & 7) == 0 && ((uintptr_t)total & 7) == 0,
                 "map_region_overlap: maps / labels / regions must be 4-byte, scratch / total 8-byte aligned");
  const int width = nbins + 1;
  const double elems = (double)N * P, scratch_bytes = 8.0 * N * width, total_bytes = 8.0 * width;
  const void *in[3] = {maps, labels, regions};
  const double in_bytes[3] = {4.0 * elems, 4.0 * elems, 4.0 * N};
  for (int k = 0; k < 3; ++k)
    DDPM_CHECK_ARG(!pm_overlap(scratch, scratch_bytes, in[k], in_bytes[k]) && !pm_overlap(total, total_bytes, in[k], in_bytes[k]),
                   "map_region_overlap: scratch / total alias another operand");
  DDPM_CHECK_ARG(!pm_overlap(scratch, scratch_bytes, total, total_bytes), "map_region_overlap: scratch / total alias another operand");
  ProfScope prof(s, "map_region_overlap", 0.0, 8.0 * elems + 2.0 * scratch_bytes + total_bytes);
  hipLaunchKernelGGL(map_region_overlap_kernel, dim3((unsigned)N), dim3(kRgBlock), 0, s, maps, labels, regions, P, lo, inv_step, nbins,
                     scratch);
  DDPM_CHECK_LAUNCH();
  hipLaunchKernelGGL(map_region_overlap_sum_kernel, dim3((unsigned)((width + 255) / 256)), dim3(256), 0, s, scratch, N, width, accumulate,
                     total);
  DDPM_CHECK_LAUNCH();
  return 0;
}

// ---- component counts -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRgBlock) void map_component_counts_kernel(const float *__restrict__ maps, const uint8_t *__restrict__ masks,
                                                                        const int32_t *__restrict__ labels,
                                                                        const int32_t *__restrict__ regions, int H, int W,
                                                                        const float *__restrict__ thresholds, int K, int conn,
                                                                        int32_t *__restrict__ counts) {
  __shared__ CcShared sh;
  __shared__ uint32_t touch[kRgMaxPixels / 32];    // per root (by its flat index): the component holds a masked pixel
  __shared__ uint32_t hit[kRgMaxPixels / 32 + 1];  // per ground-truth region 1 .. R: it holds a predicted pixel
  __shared__ int red[kRgWaves][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, P = H * W;
  const int n = blockIdx.x / K, k = blockIdx.x - n * K;
  const float *row = maps + (int64_t)n * P;
  const uint8_t *mrow = masks + (int64_t)n * P;
  const int32_t *lrow = labels + (int64_t)n * P;
  const int R = min(max(regions[n], 0), P);
  for (int j = tid; j < kRgMaxPixels / 32 + 1; j += kRgBlock) {
    if (j < kRgMaxPixels / 32) touch[j] = 0u;
    hit[j] = 0u;
  }
  cc_link(sh, PredGt(row, thresholds[k]), H, W, conn);  // (barriers inside: the zeroes above are in place)
  const volatile uint16_t *par = reinterpret_cast<const volatile uint16_t *>(sh.words);
  for (int i = tid; i < P; i += kRgBlock) {
    const uint32_t p = par[i];
    if (p == kRgBg) continue;
    if (mrow[i]) atomicOr(&touch[p >> 5], 1u << (p & 31u));
    const int l = lrow[i];
    if (l >= 1 && l <= R) atomicOr(&hit[l >> 5], 1u << (l & 31));
  }
  __syncthreads();
  int c[3] = {0, 0, 0};  // hit, pred, false_pred
  for (int j = tid; j < kRgMaxPixels / 32 + 1; j += kRgBlock) c[0] += __popc(hit[j]);
  for (int i = tid; i < P; i += kRgBlock) {
    if (par[i] == (uint32_t)i) {
      ++c[1];
      c[2] += (touch[i >> 5] >> (i & 31)) & 1u ? 0 : 1;
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    int v = c[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[wave][j] = v;
  }
  __syncthreads();
  if (tid < 3) {
    int v = 0;
#pragma unroll
    for (int w = 0; w < kRgWaves; ++w) v += red[w][tid];
    counts[(int64_t)blockIdx.x * 3 + tid] = sh.fail ? -1 : v;
  }
}

int launch_map_component_counts(const float *maps, const uint8_t *masks, const int32_t *labels, const int32_t *regions, int N, int H,
                                int W, const float *thresholds, int K, int conn, int32_t *counts, hipStream_t s) {
  const char *op = "map_component_counts";
  DDPM_CHECK_ARG(maps && masks && labels && regions && thresholds && counts, "%s: null pointer", op);
  if (int rc = check_plane(op, N, H, W, conn)) return rc;
  DDPM_CHECK_ARG(K >= 1 && K <= kCountsMaxK, "%s: K must lie in 1 .. %d (got %d)", op, kCountsMaxK, K);
  DDPM_CHECK_ARG((double)N * K < 2147483648.0, "%s: N * K must stay below 2^31 (got %d x %d)", op, N, K);
  DDPM_CHECK_ARG(((uintptr_t)maps & 3) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)regions & 3) == 0 &&
                     ((uintptr_t)thresholds & 3) == 0 && ((uintptr_t)counts & 3) == 0,
                 "%s: maps / labels / regions / thresholds / counts must be 4-byte aligned", op);
  const double elems = (double)N * H * W, out_bytes = 12.0 * N * K;
  DDPM_CHECK_ARG(!pm_overlap(counts, out_bytes, maps, 4.0 * elems) && !pm_overlap(counts, out_bytes, masks, elems) &&
                     !pm_overlap(counts, out_bytes, labels, 4.0 * elems) && !pm_overlap(counts, out_bytes, regions, 4.0 * N) &&
                     !pm_overlap(counts, out_bytes, thresholds, 4.0 * K),
                 "%s: counts aliases an input", op);
  ProfScope prof(s, op, 0.0, 9.0 * elems * K + out_bytes);
  hipLaunchKernelGGL(map_component_counts_kernel, dim3((unsigned)(N * K)), dim3(kRgBlock), 0, s, maps, masks, labels, regions, H, W,
                     thresholds, K, conn, counts);
  DDPM_CHECK_LAUNCH();
  return 0;
}

}  // namespace ddpm

using namespace ddpm;

extern "C" int ddpm_map_label_u8(const uint8_t *masks, int N, int H, int W, int connectivity, int32_t *labels, int32_t *regions,
                                 ddpm_stream_t stream) {
  return launch_map_label<PredU8, uint8_t>("map_label_u8", masks, 0.0f, N, H, W, connectivity, labels, regions, as_stream(stream));
}

extern "C" int ddpm_map_label_f32(const float *maps, float thr, int N, int H, int W, int connectivity, int32_t *labels, int32_t *regions,
                                  ddpm_stream_t stream) {
  return launch_map_label<PredGt, float>("map_label_f32", maps, thr, N, H, W, connectivity, labels, regions, as_stream(stream));
}

extern "C" int ddpm_map_region_overlap_f32(const float *maps, const int32_t *labels, const int32_t *regions, int N, int P, float lo,
                                           float inv_step, int nbins, double *scratch, double *total, int accumulate,
                                           ddpm_stream_t stream) {
  return launch_map_region_overlap(maps, labels, regions, N, P, lo, inv_step, nbins, scratch, total, accumulate, as_stream(stream));
}

extern "C" int ddpm_map_component_counts_f32(const float *maps, const uint8_t *masks, const int32_t *labels, const int32_t *regions,
                                             int N, int H, int W, const float *thresholds, int K, int connectivity, int32_t *counts,
                                             ddpm_stream_t stream) {
  return launch_map_component_counts(maps, masks, labels, regions, N, H, W, thresholds, K, connectivity, counts, as_stream(stream));
}
