// Predicted segmentations from anomaly maps of volumes: segment.hip's two ops with a depth axis.
//   map_median3d   3 x 3 x 3 median of [N, D, H, W] volumes, scipy.ndimage's mode="reflect" boundary on all three axes, np.sort's order
//   map_segment3d  per volume and threshold: the components of {v > thr} with at least min_size voxels as a uint8 volume, its voxel
//                  counts against the mask, its component counts against the mask's regions, what the size filter dropped
//
// Median.  One workgroup of 256 threads per tile of 64 x 8 x 8 voxels (w, h, d).  The tile and its one-voxel halo, 66 x 10 x 10
// dwords = 26 400 bytes, go from HBM into LDS once, as the key of each value (median_common.h); 6 600 values are read for 4 096
// written, 1.61 reads per voxel, of which all but the first come from a neighbouring tile's lines in L2.  A thread owns one
// column x of the tile and 16 of its voxels (rows ty and ty + 4, every plane): each of the 27 reads of a window is, over a wave, 64
// consecutive dwords of one row of the tile, so the 32 lanes of a half-wave ask 32 different banks.  Selection as in segment.hip:
// 27 values in registers, select_median<15> (15 = 27 / 2 + 2 values, the smallest and the largest dropped, the next admitted, down
// to three), unsigned min / max at constant indices only, no dynamically indexed array, no scratch
// (profiles/voxel_segmentation.md has the resource usage; tools/median_zero_one.cpp runs the sequence on all 2^27 zero-one inputs).
//
// Segment.  A 128^3 volume does not fit the LDS: the forest is regions3d's, one int32 parent per voxel in scratch, built by its
// launches 1 .. 3 (regions3d_common.h) for the N K thresholded volumes; the only barrier is a launch boundary.  Then
//   zero   the int32 counter of every voxel slot set to 0 (never assumed)
//   size   size[root] += the voxels of the component: every wave over its 64 consecutive voxels, one integer atomicAdd per stretch
//          of equal roots (a ballot of the stretches' first lanes gives their lengths): an all-ones volume is P / 64 additions
//   keep   kept = size[root] >= min_size (the sizes are final: a launch boundary behind the last addition); seg written; per kept
//          root "holds a masked voxel", per region "holds a kept voxel": one bit each, set by atomicOr behind a relaxed load; per
//          256-voxel block the partial TP, FP, FN, kept roots, removed roots, removed voxels
//   final  one workgroup per (volume, threshold): the partials summed in a fixed order, the two bit sets counted;
//          false_pred = kept roots - kept roots with a masked voxel
// Integer atomics only (sums and ors: their result does not depend on their order); every output element is written by a plain
// store, nothing is read from an output, and every scratch word that is read was written by a launch of this call.  Should a
// bound of the labelling run out (it cannot), the item's fail word is set and its integers are -1.
#include "median_common.h"
#include "regions3d_common.h"

namespace ddpm {

// ---- median -------------------------------------------------------------------------------------------------------------------
constexpr int kM3TileW = 64;
constexpr int kM3TileH = 8;
constexpr int kM3TileD = 8;
constexpr int kM3Block = 256;
constexpr int kM3LW = kM3TileW + 2, kM3LH = kM3TileH + 2, kM3LD = kM3TileD + 2;
constexpr int kM3Rows = kM3TileH / (kM3Block / kM3TileW);  // rows of a plane per thread

__global__ __launch_bounds__(kM3Block) void map_median3d_kernel(const float *__restrict__ in, float *__restrict__ out, int D, int H, int W,
                                                                int tiles_x, int tiles_y, int tiles_z) {
  __shared__ uint32_t tile[kM3LD * kM3LH * kM3LW];
  const int tid = threadIdx.x;
  const int per_volume = tiles_x * tiles_y * tiles_z;
  const int n = blockIdx.x / per_volume;
  int t = blockIdx.x - n * per_volume;
  const int x0 = (t % tiles_x) * kM3TileW;
  t /= tiles_x;
  const int y0 = (t % tiles_y) * kM3TileH, z0 = (t / tiles_y) * kM3TileD;
  const int64_t HW = (int64_t)H * W;
  const float *src = in + (int64_t)n * D * HW;
  float *dst = out + (int64_t)n * D * HW;
  for (int e = tid; e < kM3LD * kM3LH * kM3LW; e += kM3Block) {
    const int lz = e / (kM3LH * kM3LW), r = e - lz * (kM3LH * kM3LW), ly = r / kM3LW, lx = r - ly * kM3LW;
    tile[e] = med_key(src[med_reflect(z0 + lz - 1, D) * HW + (int64_t)med_reflect(y0 + ly - 1, H) * W + med_reflect(x0 + lx - 1, W)]);
  }
  __syncthreads();
  const int tx = tid & (kM3TileW - 1), ty = tid / kM3TileW;
  if (x0 + tx >= W) return;
#pragma unroll 1
  for (int lz = 0; lz < kM3TileD; ++lz) {
    if (z0 + lz >= D) break;
#pragma unroll 1
    for (int j = 0; j < kM3Rows; ++j) {
      const int ly = ty + j * (kM3Block / kM3TileW);
      if (y0 + ly < H) {
        uint32_t v[27];
#pragma unroll
        for (int dz = 0; dz < 3; ++dz)
#pragma unroll
          for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) v[(dz * 3 + dy) * 3 + dx] = tile[((lz + dz) * kM3LH + ly + dy) * kM3LW + tx + dx];
        dst[(z0 + lz) * HW + (int64_t)(y0 + ly) * W + x0 + tx] = med_value(select_median<27 / 2 + 2>(v));
      }
    }
  }
}

int launch_map_median3d(const float *in, float *out, int size, int N, int D, int H, int W, hipStream_t s) {
  const char *op = "map_median3d";
  DDPM_CHECK_ARG(in && out, "%s: null pointer", op);
  DDPM_CHECK_ARG(N > 0 && D > 0 && H > 0 && W > 0, "%s: N, D, H and W must be positive (got %d, %d, %d, %d)", op, N, D, H, W);
  DDPM_CHECK_ARG(size == 3, "%s: size must be 3 (got %d)", op, size);
  DDPM_CHECK_ARG((double)D * H * W < 2147483648.0, "%s: a volume of %d x %d x %d voxels is not below 2^31", op, D, H, W);
  const int tiles_x = (W + kM3TileW - 1) / kM3TileW, tiles_y = (H + kM3TileH - 1) / kM3TileH, tiles_z = (D + kM3TileD - 1) / kM3TileD;
  DDPM_CHECK_ARG((double)N * tiles_x * tiles_y * tiles_z < 2147483648.0, "%s: N x tiles must stay below 2^31 (got %d x %d x %d x %d)", op, N,
                 tiles_z, tiles_y, tiles_x);
  DDPM_CHECK_ARG(((uintptr_t)in & 3) == 0 && ((uintptr_t)out & 3) == 0, "%s: maps / out must be 4-byte aligned", op);
  const double elems = (double)N * D * H * W;
  DDPM_CHECK_ARG(!pm_overlap(out, 4.0 * elems, in, 4.0 * elems), "%s: out aliases the input (not in place)", op);
  ProfScope prof(s, op, 0.0, 8.0 * elems);
  hipLaunchKernelGGL(map_median3d_kernel, dim3((unsigned)(N * tiles_x * tiles_y * tiles_z)), dim3(kM3Block), 0, s, in, out, D, H, W, tiles_x,
                     tiles_y, tiles_z);
  DDPM_CHECK_LAUNCH();
  return 0;
}

// ---- segment ------------------------------------------------------------------------------------------------------------------
constexpr int kS3Parts = 6;  // TP, FP, FN; kept roots, removed roots, removed voxels

__global__ __launch_bounds__(kR3Block) void sg3_zero_kernel(int P, int32_t *__restrict__ size_all) {
  const int64_t ii = (int64_t)blockIdx.x * kR3Block + threadIdx.x;
  if (ii < P) size_all[(int64_t)blockIdx.y * P + ii] = 0;
}

// (no early return: the shuffle and the ballot see whole waves; the voxels behind the volume count as background)
__global__ __launch_bounds__(kR3Block) void sg3_size_kernel(int P, const int32_t *__restrict__ par_all, int32_t *__restrict__ size_all) {
  const int lane = threadIdx.x & 63;
  const int64_t ii = (int64_t)blockIdx.x * kR3Block + threadIdx.x;
  int32_t r = -1;
  if (ii < P) {
    r = par_all[(int64_t)blockIdx.y * P + ii];
    if (r >= P) r = -1;  // (never: a parent is a voxel of the volume)
  }
  const int32_t before = __shfl_up(r, 1, 64);
  const bool first = lane == 0 || before != r;
  const unsigned long long firsts = __ballot(first);
  if (first && r >= 0) {
    const unsigned long long above = lane == 63 ? 0ull : firsts >> (lane + 1);
    const int len = above ? __ffsll(above) : 64 - lane;
    atomicAdd(size_all + (int64_t)blockIdx.y * P + r, len);
  }
}

// flags: per item 2 nw words, zeroed by launch 1: touch (bit i: the KEPT component with root i holds a masked voxel), then hit
// (bit l: region l holds a kept voxel).  A bit is only ever set, so the load in front of the atomic only spares atomics.
__global__ __launch_bounds__(kR3Block) void sg3_keep_kernel(int P, int K, int nw, int nblk, int min_size, const int32_t *__restrict__ par_all,
                                                            const int32_t *__restrict__ size_all, const uint8_t *__restrict__ masks,
                                                            const int32_t *__restrict__ labels, const int32_t *__restrict__ regions,
                                                            uint32_t *__restrict__ flags, uint8_t *__restrict__ seg, int32_t *__restrict__ part) {
  __shared__ int sh[kR3Waves];
  const int item = blockIdx.y, n = item / K;
  const int64_t ii = (int64_t)blockIdx.x * kR3Block + threadIdx.x;
  int c[kS3Parts] = {0, 0, 0, 0, 0, 0};
  if (ii < P) {
    const int32_t q = par_all[(int64_t)item * P + ii];
    const bool m = masks[(int64_t)n * P + ii] != 0;
    bool kept = false;
    if (q >= 0 && q < P) {
      const int32_t sz = size_all[(int64_t)item * P + q];
      kept = sz >= min_size;
      if (q == (int32_t)ii) {
        c[3] = kept ? 1 : 0;
        c[4] = kept ? 0 : 1;
        c[5] = kept ? 0 : sz;
      }
      if (kept) {
        uint32_t *touch = flags + (int64_t)item * 2 * nw, *hit = touch + nw;
        if (m) {
          const uint32_t bit = 1u << (q & 31);
          if (!(__hip_atomic_load(touch + (q >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit))
            __hip_atomic_fetch_or(touch + (q >> 5), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const int R = min(max(regions[n], 0), P);
        const int32_t l = labels[(int64_t)n * P + ii];
        if (l >= 1 && l <= R) {
          const uint32_t bit = 1u << (l & 31);
          if (!(__hip_atomic_load(hit + (l >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit))
            __hip_atomic_fetch_or(hit + (l >> 5), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    seg[(int64_t)item * P + ii] = kept ? 1 : 0;
    c[0] = kept && m ? 1 : 0;
    c[1] = kept && !m ? 1 : 0;
    c[2] = !kept && m ? 1 : 0;
  }
#pragma unroll
  for (int j = 0; j < kS3Parts; ++j) {
    const int t = r3_block_sum(c[j], sh);
    if (threadIdx.x == 0) part[((int64_t)item * nblk + blockIdx.x) * kS3Parts + j] = t;
  }
}

__global__ __launch_bounds__(kR3Block) void sg3_final_kernel(int nblk, int nw, const int32_t *__restrict__ part, const uint32_t *__restrict__ flags,
                                                             const int32_t *__restrict__ fail, int32_t *__restrict__ pixels,
                                                             int32_t *__restrict__ components, int32_t *__restrict__ removed) {
  __shared__ int sh[kR3Waves];
  const int item = blockIdx.x;
  int total[kS3Parts + 2];
#pragma unroll
  for (int j = 0; j < kS3Parts; ++j) {
    int c = 0;
    for (int b = threadIdx.x; b < nblk; b += kR3Block) c += part[((int64_t)item * nblk + b) * kS3Parts + j];
    total[j] = r3_block_sum(c, sh);
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {  // touch, hit
    const uint32_t *words = flags + ((int64_t)item * 2 + j) * nw;
    int c = 0;
    for (int b = threadIdx.x; b < nw; b += kR3Block) c += __popc(words[b]);
    total[kS3Parts + j] = r3_block_sum(c, sh);
  }
  if (threadIdx.x == 0) {
    const bool bad = fail[item] != 0;
    pixels[(int64_t)item * 3 + 0] = bad ? -1 : total[0];
    pixels[(int64_t)item * 3 + 1] = bad ? -1 : total[1];
    pixels[(int64_t)item * 3 + 2] = bad ? -1 : total[2];
    components[(int64_t)item * 3 + 0] = bad ? -1 : total[kS3Parts + 1];
    components[(int64_t)item * 3 + 1] = bad ? -1 : total[3];
    components[(int64_t)item * 3 + 2] = bad ? -1 : total[3] - total[kS3Parts];
    removed[(int64_t)item * 2 + 0] = bad ? -1 : total[4];
    removed[(int64_t)item * 2 + 1] = bad ? -1 : total[5];
  }
}

// parents, sizes, flags (2 nw words), partials, fail word: per item
static size_t segment3d_scratch_bytes(int N, int K, int64_t P) {
  const size_t items = (size_t)N * (size_t)K, nw = (size_t)(P / 32 + 1), nblk = (size_t)r3_blocks(P);
  return 4u * (items * 2 * (size_t)P + items * 2 * nw + items * nblk * kS3Parts + items);
}

int launch_map_segment3d(const float *maps, const uint8_t *masks, const int32_t *labels, const int32_t *regions, int N, int D, int H, int W,
                         const float *thresholds, int K, int min_size, int conn, uint8_t *seg, int32_t *pixels, int32_t *components,
                         int32_t *removed, void *scratch, hipStream_t s) {
  const char *op = "map_segment3d";
  DDPM_CHECK_ARG(maps && masks && labels && regions && thresholds && seg && pixels && components && removed && scratch, "%s: null pointer", op);
  DDPM_CHECK_ARG(K >= 1 && K <= kCountsMaxK, "%s: K must lie in 1 .. %d (got %d)", op, kCountsMaxK, K);
  if (int rc = check_volume(op, N, D, H, W, conn, K)) return rc;
  DDPM_CHECK_ARG(min_size >= 1, "%s: min_size must lie in 1 .. 2^31 - 1 (got %d)", op, min_size);
  DDPM_CHECK_ARG(((uintptr_t)maps & 3) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)regions & 3) == 0 &&
                     ((uintptr_t)thresholds & 3) == 0 && ((uintptr_t)pixels & 3) == 0 && ((uintptr_t)components & 3) == 0 &&
                     ((uintptr_t)removed & 3) == 0 && ((uintptr_t)scratch & 3) == 0,
                 "%s: maps / labels / regions / thresholds / pixels / components / removed / scratch must be 4-byte aligned", op);
  const int64_t P = (int64_t)D * H * W;
  const double elems = (double)N * (double)P;
  const void *in[5] = {maps, masks, labels, regions, thresholds};
  const double in_bytes[5] = {4.0 * elems, elems, 4.0 * elems, 4.0 * N, 4.0 * K};
  const void *out[5] = {seg, pixels, components, removed, scratch};
  const double out_bytes[5] = {elems * K, 12.0 * N * K, 12.0 * N * K, 8.0 * N * K, (double)segment3d_scratch_bytes(N, K, P)};
  for (int o = 0; o < 5; ++o) {
    for (int i = 0; i < 5; ++i)
      DDPM_CHECK_ARG(!pm_overlap(out[o], out_bytes[o], in[i], in_bytes[i]), "%s: an output or the scratch aliases an input", op);
    for (int q = o + 1; q < 5; ++q)
      DDPM_CHECK_ARG(!pm_overlap(out[o], out_bytes[o], out[q], out_bytes[q]), "%s: two of the outputs and the scratch alias each other", op);
  }
  const int items = N * K, nw = (int)(P / 32 + 1), nblk = r3_blocks(P);
  int32_t *par = static_cast<int32_t *>(scratch), *size = par + (size_t)items * (size_t)P;
  uint32_t *flags = reinterpret_cast<uint32_t *>(size + (size_t)items * (size_t)P);
  int32_t *part = reinterpret_cast<int32_t *>(flags + (size_t)items * 2 * (size_t)nw), *fail = part + (size_t)items * (size_t)nblk * kS3Parts;
  ProfScope prof(s, op, 0.0, (4.0 * 3.0 + 4.0 * 8.0 + 4.0 * 4.0 + 10.0) * elems * K + 32.0 * N * K);
  if (int rc = launch_cc3_link(SrcThr{maps, thresholds, K, P}, items, P, D, H, W, conn, par, fail, flags, nw, s)) return rc;
  const dim3 grid((unsigned)nblk, (unsigned)items), block(kR3Block);
  hipLaunchKernelGGL(sg3_zero_kernel, grid, block, 0, s, (int)P, size);
  DDPM_CHECK_LAUNCH();
  hipLaunchKernelGGL(sg3_size_kernel, grid, block, 0, s, (int)P, par, size);
  DDPM_CHECK_LAUNCH();
  hipLaunchKernelGGL(sg3_keep_kernel, grid, block, 0, s, (int)P, K, nw, nblk, min_size, par, size, masks, labels, regions, flags, seg, part);
  DDPM_CHECK_LAUNCH();
  hipLaunchKernelGGL(sg3_final_kernel, dim3((unsigned)items), block, 0, s, nblk, nw, part, flags, fail, pixels, components, removed);
  DDPM_CHECK_LAUNCH();
  return 0;
}

}  // namespace ddpm

using namespace ddpm;

extern "C" int ddpm_map_median3d_f32(const float *maps, float *out, int size, int N, int D, int H, int W, ddpm_stream_t stream) {
  return launch_map_median3d(maps, out, size, N, D, H, W, as_stream(stream));
}

extern "C" int64_t ddpm_regions3d_segment_scratch_bytes(int N, int D, int H, int W, int K) {
  return r3_extent_ok(N, D, H, W) && K >= 1 && K <= kCountsMaxK ? (int64_t)segment3d_scratch_bytes(N, K, (int64_t)D * H * W) : 0;
}

extern "C" int ddpm_map_segment3d_f32(const float *maps, const uint8_t *masks, const int32_t *labels, const int32_t *regions, int N, int D,
                                      int H, int W, const float *thresholds, int K, int min_size, int connectivity, uint8_t *seg,
                                      int32_t *pixels, int32_t *components, int32_t *removed, void *scratch, ddpm_stream_t stream) {
  return launch_map_segment3d(maps, masks, labels, regions, N, D, H, W, thresholds, K, min_size, connectivity, seg, pixels, components,
                              removed, scratch, as_stream(stream));
}
