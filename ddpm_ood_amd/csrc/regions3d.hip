// Region-level evaluation of anomaly maps of volumes (only with --voxel_regions 1).  The contracts are those of
// regions.hip with a depth axis; what differs is where the union-find forest lives.
//   map_label3d             connected components of a batch of volumes (mask != 0, or v > thr), numbered as scipy.ndimage.label does,
//                           for the three structures generate_binary_structure(3, k): 6, 18 and 26 neighbours
//   map_region_overlap3d    per bin, the sum over the ground-truth regions of (the region's voxels in the bin) / (its volume)
//   map_component_counts3d  per volume and threshold: regions hit, predicted components, predicted components off every region
// A 128^3 volume has 2 M voxels: the forest is one int32 parent per voxel in caller-provided global memory (background -1), the
// work is spread over 256-thread workgroups (one voxel per thread, blockIdx.y the volume), and the phases are separate launches.
//
// Labelling.  A parent is never above its voxel, so every walk towards a root descends and a root is the smallest flat index of
// its tree.
//   1  init    runs along w: a wave holds 64 consecutive voxels; from two ballots (outside, first voxel of a row) every lane reads
//              off the first voxel of its run inside the wave and points at it; the wave's first lane points at its left neighbour
//              when the run began in the wave before (a chain of at most W / 64 links).  No pointer jumping.
//   2  union   one union per pair of touching runs of neighbouring rows (dy, dz in {-1, 0, 1}, the row before in flat order; x
//              diagonals as the connectivity allows), issued by the first voxel at which this run meets the other.  A union walks
//              to both roots and hangs the larger below the smaller with a device-scope atomic minimum; all unions of the batch
//              run concurrently, lock-free.
//   3  flatten every voxel walks to its root and stores it.
//   4  number  the roots counted per 256-voxel block, the block counts scanned per volume by one workgroup (which also writes
//              `regions`), the roots ranked 1 .. R in ascending flat index, every other voxel reads its root's rank.
//
// Visibility between workgroups.  The per-XCD L2s and the per-CU L1s are not coherent, and nothing here waits for another
// workgroup: no grid barrier, no flag, no cooperative launch.  Within one launch workgroups meet only in launch 2 and 3, and
// only through the parents:
//   - a parent only ever decreases, and every value it ever held is a voxel of the same component (the run's first voxel, then
//     roots of trees joined to it): a walk that reads an OLD value of a parent therefore still descends inside the component and
//     merely arrives at a voxel that may no longer be a root;
//   - a candidate root is confirmed by the atomic that modifies it: atomic-min(par[a], b) returns what par[a] held at the
//     moment of the update; only if that is `a` itself was `a` a root and is the union done; otherwise the pair (what it held,
//     b) is joined instead.  No decision rests on a plain read;
//   - the walks of launch 2 read parents with relaxed agent-scope atomic loads (served past the L1), for speed of convergence,
//     not correctness; in launch 3 the forest is final (a launch boundary behind the last union), the only stores are roots over
//     ancestors, and either value leads to the same root.
// Everything else a launch reads was written by an earlier launch or is an input.  Integer atomics only; the final root of a
// component is its smallest index whatever the order of the unions, so no output depends on that order, nor on what scratch or
// the outputs held before.
//
// Termination: every loop carries a bound that follows from the algorithm in its condition (g3_find, g3_union); should one run
// out (it cannot), the volume's fail word is set, the thread returns, and `regions` (the volume's counts) are -1.
//
// Overlap: the regions of a volume are taken in chunks of `chunk_regions`; per chunk an integer table [region, bin] in scratch is
// filled by integer atomics over the whole volume, a region's volume is the sum of its row (every voxel, NaN included, falls in
// one column), and one thread per bin adds (double)h / (double)area over the chunk's regions in ascending order onto the
// volume's float64 row, which carries over from chunk to chunk: the additions and their order are those of regions.hip for any
// chunk size.  The entry point copies `regions` to the host (N ints, one stream synchronisation) to know the chunk counts.
#include <vector>

#include "regions3d_common.h"

namespace ddpm {

// ---- launches 4 .. 7: number the roots ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kR3Block) void cc3_count_kernel(int P, int nblk, const int32_t *__restrict__ par_all, int32_t *__restrict__ bsum) {
  __shared__ int sh[kR3Waves];
  const int64_t ii = (int64_t)blockIdx.x * kR3Block + threadIdx.x;
  const int c = ii < P && par_all[(int64_t)blockIdx.y * P + ii] == (int32_t)ii ? 1 : 0;
  const int t = r3_block_sum(c, sh);
  if (threadIdx.x == 0) bsum[(int64_t)blockIdx.y * nblk + blockIdx.x] = t;
}

// one workgroup per volume: bsum -> its exclusive prefix, in place; regions = the total, -1 behind a failed bound
__global__ __launch_bounds__(kR3Block) void cc3_scan_kernel(int nblk, int32_t *__restrict__ bsum_all, const int32_t *__restrict__ fail,
                                                            int32_t *__restrict__ regions) {
  __shared__ int sh[kR3Waves];
  int32_t *bsum = bsum_all + (int64_t)blockIdx.x * nblk;
  int carry = 0;
  for (int64_t c0 = 0; c0 < nblk; c0 += kR3Block) {
    const int64_t j = c0 + threadIdx.x;
    const int v = j < nblk ? bsum[j] : 0;
    int total;
    const int ex = r3_block_scan(v, sh, &total);
    if (j < nblk) bsum[j] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) regions[blockIdx.x] = fail[blockIdx.x] ? -1 : carry;
}

__global__ __launch_bounds__(kR3Block) void cc3_rank_kernel(int P, int nblk, const int32_t *__restrict__ par_all, const int32_t *__restrict__ bsum,
                                                            int32_t *__restrict__ labels) {
  __shared__ int sh[kR3Waves];
  const int64_t ii = (int64_t)blockIdx.x * kR3Block + threadIdx.x;
  const int c = ii < P && par_all[(int64_t)blockIdx.y * P + ii] == (int32_t)ii ? 1 : 0;
  int total;
  const int ex = r3_block_scan(c, sh, &total);
  if (ii < P) labels[(int64_t)blockIdx.y * P + ii] = c ? bsum[(int64_t)blockIdx.y * nblk + blockIdx.x] + ex + 1 : 0;
}

// every voxel inside that is no root reads its root's rank (written by the launch before, not by this one)
__global__ __launch_bounds__(kR3Block) void cc3_relabel_kernel(int P, const int32_t *__restrict__ par_all, int32_t *labels) {
  const int64_t ii = (int64_t)blockIdx.x * kR3Block + threadIdx.x;
  if (ii >= P) return;
  const int32_t q = par_all[(int64_t)blockIdx.y * P + ii];
  if (q >= 0 && q < P && q != (int32_t)ii) labels[(int64_t)blockIdx.y * P + ii] = labels[(int64_t)blockIdx.y * P + q];
}

static size_t label3d_scratch_bytes(int N, int64_t P) { return 4u * ((size_t)N * (size_t)P + (size_t)N * (size_t)r3_blocks(P) + (size_t)N); }

template <class Src, class T>
static int launch_map_label3d(const char *op, const T *src, float thr, int N, int D, int H, int W, int conn, int32_t *labels,
                              int32_t *regions, void *scratch, hipStream_t s) {
  DDPM_CHECK_ARG(src && labels && regions && scratch, "%s: null pointer", op);
  if (int rc = check_volume(op, N, D, H, W, conn, 1)) return rc;
  DDPM_CHECK_ARG(((uintptr_t)src & (sizeof(T) - 1)) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)regions & 3) == 0 &&
                     ((uintptr_t)scratch & 3) == 0,
                 "%s: maps / labels / regions / scratch must be 4-byte aligned", op);
  const int64_t P = (int64_t)D * H * W;
  const double elems = (double)N * (double)P, sbytes = (double)label3d_scratch_bytes(N, P);
  DDPM_CHECK_ARG(!pm_overlap(labels, 4.0 * elems, src, sizeof(T) * elems) && !pm_overlap(regions, 4.0 * N, src, sizeof(T) * elems) &&
                     !pm_overlap(labels, 4.0 * elems, regions, 4.0 * N) && !pm_overlap(scratch, sbytes, src, sizeof(T) * elems) &&
                     !pm_overlap(scratch, sbytes, labels, 4.0 * elems) && !pm_overlap(scratch, sbytes, regions, 4.0 * N),
                 "%s: labels / regions / scratch alias another operand", op);
  const int nblk = r3_blocks(P);
  int32_t *par = static_cast<int32_t *>(scratch), *bsum = par + (size_t)N * (size_t)P, *fail = bsum + (size_t)N * (size_t)nblk;
  ProfScope prof(s, op, 0.0, (sizeof(T) * 3.0 + 4.0 * 8.0) * elems);
  Src view;
  if constexpr (sizeof(T) == 1) {
    view = Src{src, P};
  } else {
    view = Src{src, thr, P};
  }
  if (int rc = launch_cc3_link(view, N, P, D, H, W, conn, par, fail, nullptr, 0, s)) return rc;
  const dim3 grid((unsigned)nblk, (unsigned)N), block(kR3Block);
  hipLaunchKernelGGL(cc3_count_kernel, grid, block, 0, s, (int)P, nblk, par, bsum);
  DDPM_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc3_scan_kernel, dim3((unsigned)N), block, 0, s, nblk, bsum, fail, regions);
  DDPM_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc3_rank_kernel, grid, block, 0, s, (int)P, nblk, par, bsum, labels);
  DDPM_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc3_relabel_kernel, grid, block, 0, s, (int)P, par, labels);
  DDPM_CHECK_LAUNCH();
  return 0;
}

// ---- region overlap ---------------------------------------------------------------------------------------------------------
// hist[rel, bin] += 1 for the voxels of the regions r0 + 1 .. r0 + cnt (rel = label - 1 - r0)
__global__ __launch_bounds__(kR3Block) void ov3_hist_kernel(const float *__restrict__ maps, const int32_t *__restrict__ labels, int P, int r0,
                                                            int cnt, float lo, float inv_step, int nbins, uint32_t *__restrict__ hist) {
  const int64_t ii = (int64_t)blockIdx.x * kR3Block + threadIdx.x;
  if (ii >= P) return;
  const int64_t rel = (int64_t)labels[ii] - 1 - r0;
  if (rel < 0 || rel >= cnt) return;
  atomicAdd(&hist[rel * (nbins + 1) + pm_bin(maps[ii], lo, inv_step, nbins)], 1u);
}

// area[rel] = the sum of row rel (every voxel of a region, NaN ones included, is in one column); one workgroup per region
__global__ __launch_bounds__(kR3Block) void ov3_area_kernel(const uint32_t *__restrict__ hist, int width, uint32_t *__restrict__ area) {
  __shared__ int sh[kR3Waves];
  const uint32_t *row = hist + (int64_t)blockIdx.x * width;
  int c = 0;
  for (int b = threadIdx.x; b < width; b += kR3Block) c += (int)row[b];
  const int t = r3_block_sum(c, sh);
  if (threadIdx.x == 0) area[blockIdx.x] = (uint32_t)t;
}

// w[b] += (double)h[rel, b] / (double)area[rel] for rel ascending; the thread that owns the bin
__global__ __launch_bounds__(kR3Block) void ov3_fold_kernel(const uint32_t *__restrict__ hist, const uint32_t *__restrict__ area, int cnt, int width,
                                                            double *__restrict__ w) {
  const int b = blockIdx.x * kR3Block + threadIdx.x;
  if (b >= width) return;
  double acc = w[b];
  for (int rel = 0; rel < cnt; ++rel) {
    const uint32_t u = hist[(int64_t)rel * width + b];
    if (u) acc += (double)u / (double)area[rel];  // (adding the zero of an empty bin changes nothing)
  }
  w[b] = acc;
}

__global__ __launch_bounds__(kR3Block) void ov3_sum_kernel(const double *__restrict__ w, int N, int width, int accumulate, double *__restrict__ total) {
  const int b = blockIdx.x * kR3Block + threadIdx.x;
  if (b >= width) return;
  double t = accumulate ? total[b] : 0.0;
  for (int n = 0; n < N; ++n) t += w[(int64_t)n * width + b];
  total[b] = t;
}

static size_t overlap3d_scratch_bytes(int N, int nbins, int chunk) {
  const size_t width = (size_t)nbins + 1;
  return 8u * (size_t)N * width + 4u * (size_t)chunk * (width + 1);
}

#define DDPM_CHECK_HIP_RC(expr, op)                                           \
  do {                                                                        \
    hipError_t e_ = (expr);                                                   \
    if (e_ != hipSuccess) {                                                   \
      ::ddpm::set_error("%s: %s", op, hipGetErrorString(e_));                 \
      return (int)e_;                                                         \
    }                                                                         \
  } while (0)

int launch_map_region_overlap3d(const float *maps, const int32_t *labels, const int32_t *regions, int N, int64_t P, float lo, float inv_step,
                                int nbins, int chunk, void *scratch, double *total, int accumulate, hipStream_t s) {
  const char *op = "map_region_overlap3d";
  DDPM_CHECK_ARG(maps && labels && regions && scratch && total, "%s: null pointer", op);
  DDPM_CHECK_ARG(N > 0 && P > 0 && P < 2147483648ll, "%s: N must be positive and P lie in 1 .. 2^31 - 1 (got %d, %lld)", op, N, (long long)P);
  DDPM_CHECK_ARG(nbins >= 1 && nbins <= kHistMaxBins, "%s: nbins must lie in 1 .. %d (got %d)", op, kHistMaxBins, nbins);
  DDPM_CHECK_ARG(chunk >= 1 && chunk <= 65536, "%s: chunk_regions must lie in 1 .. 65536 (got %d)", op, chunk);
  DDPM_CHECK_ARG(inv_step > 0.0f && inv_step <= 3.402823466e+38f && lo == lo && lo - lo == 0.0f,
                 "%s: lo must be finite and inv_step positive and finite (got %g, %g)", op, (double)lo, (double)inv_step);
  DDPM_CHECK_ARG(((uintptr_t)maps & 3) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)regions & 3) == 0 &&
                     ((uintptr_t)scratch & 7) == 0 && ((uintptr_t)total & 7) == 0,
                 "%s: maps / labels / regions must be 4-byte, scratch / total 8-byte aligned", op);
  const int width = nbins + 1;
  const double elems = (double)N * (double)P, scratch_bytes = (double)overlap3d_scratch_bytes(N, nbins, chunk), total_bytes = 8.0 * width;
  const void *in[3] = {maps, labels, regions};
  const double in_bytes[3] = {4.0 * elems, 4.0 * elems, 4.0 * N};
  for (int k = 0; k < 3; ++k)
    DDPM_CHECK_ARG(!pm_overlap(scratch, scratch_bytes, in[k], in_bytes[k]) && !pm_overlap(total, total_bytes, in[k], in_bytes[k]),
                   "%s: scratch / total alias another operand", op);
  DDPM_CHECK_ARG(!pm_overlap(scratch, scratch_bytes, total, total_bytes), "%s: scratch / total alias another operand", op);
  double *w = static_cast<double *>(scratch);
  uint32_t *area = reinterpret_cast<uint32_t *>(w + (size_t)N * width), *hist = area + chunk;
  std::vector<int32_t> R((size_t)N);
  DDPM_CHECK_HIP_RC(hipMemcpyAsync(R.data(), regions, 4u * (size_t)N, hipMemcpyDeviceToHost, s), op);
  DDPM_CHECK_HIP_RC(hipStreamSynchronize(s), op);
  ProfScope prof(s, op, 0.0, 8.0 * elems + 2.0 * 8.0 * N * width + total_bytes);
  DDPM_CHECK_HIP_RC(hipMemsetAsync(w, 0, 8u * (size_t)N * width, s), op);
  const dim3 block(kR3Block), bins((unsigned)((width + kR3Block - 1) / kR3Block));
  for (int n = 0; n < N; ++n) {
    const int64_t Rn = R[n] < 0 ? 0 : (R[n] > P ? P : R[n]);  // (labels above `regions` are no region's; a volume has at most P regions)
    for (int64_t r0 = 0; r0 < Rn; r0 += chunk) {
      const int cnt = (int)(Rn - r0 < chunk ? Rn - r0 : chunk);
      DDPM_CHECK_HIP_RC(hipMemsetAsync(hist, 0, 4u * (size_t)cnt * width, s), op);
      hipLaunchKernelGGL(ov3_hist_kernel, dim3((unsigned)r3_blocks(P)), block, 0, s, maps + (size_t)n * P, labels + (size_t)n * P, (int)P, (int)r0,
                         cnt, lo, inv_step, nbins, hist);
      DDPM_CHECK_LAUNCH();
      hipLaunchKernelGGL(ov3_area_kernel, dim3((unsigned)cnt), block, 0, s, hist, width, area);
      DDPM_CHECK_LAUNCH();
      hipLaunchKernelGGL(ov3_fold_kernel, bins, block, 0, s, hist, area, cnt, width, w + (size_t)n * width);
      DDPM_CHECK_LAUNCH();
    }
  }
  hipLaunchKernelGGL(ov3_sum_kernel, bins, block, 0, s, w, N, width, accumulate, total);
  DDPM_CHECK_LAUNCH();
  return 0;
}

// ---- component counts -------------------------------------------------------------------------------------------------------
// flags: per item 2 nw words; touch (bit i: the component with root i holds a masked voxel), then hit (bit l: region l holds a
// predicted voxel).  A bit is only ever set, so the load in front of the atomic (fresh, past the L1) only spares atomics.
__global__ __launch_bounds__(kR3Block) void cnt3_mark_kernel(int P, int K, int nw, const int32_t *__restrict__ par_all, const uint8_t *__restrict__ masks,
                                                             const int32_t *__restrict__ labels, const int32_t *__restrict__ regions,
                                                             uint32_t *__restrict__ flags) {
  const int item = blockIdx.y, n = item / K;
  const int64_t ii = (int64_t)blockIdx.x * kR3Block + threadIdx.x;
  if (ii >= P) return;
  const int32_t q = par_all[(int64_t)item * P + ii];
  if (q < 0 || q >= P) return;
  uint32_t *touch = flags + (int64_t)item * 2 * nw, *hit = touch + nw;
  if (masks[(int64_t)n * P + ii]) {
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

__global__ __launch_bounds__(kR3Block) void cnt3_partial_kernel(int P, int nw, int nblk, const int32_t *__restrict__ par_all,
                                                                const uint32_t *__restrict__ flags, int32_t *__restrict__ part) {
  __shared__ int sh[kR3Waves];
  const int item = blockIdx.y;
  const int64_t ii = (int64_t)blockIdx.x * kR3Block + threadIdx.x;
  const uint32_t *touch = flags + (int64_t)item * 2 * nw, *hit = touch + nw;
  const int root = ii < P && par_all[(int64_t)item * P + ii] == (int32_t)ii ? 1 : 0;
  const int off = root && !((touch[ii >> 5] >> (ii & 31)) & 1u) ? 1 : 0;
  const int hits = ii < nw ? __popc(hit[ii]) : 0;  // (nw <= the threads of the grid's row)
  const int c[3] = {hits, root, off};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int t = r3_block_sum(c[j], sh);
    if (threadIdx.x == 0) part[((int64_t)item * nblk + blockIdx.x) * 3 + j] = t;
  }
}

__global__ __launch_bounds__(kR3Block) void cnt3_final_kernel(int nblk, const int32_t *__restrict__ part, const int32_t *__restrict__ fail,
                                                              int32_t *__restrict__ counts) {
  __shared__ int sh[kR3Waves];
  const int item = blockIdx.x;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    int c = 0;
    for (int b = threadIdx.x; b < nblk; b += kR3Block) c += part[((int64_t)item * nblk + b) * 3 + j];
    const int t = r3_block_sum(c, sh);
    if (threadIdx.x == 0) counts[(int64_t)item * 3 + j] = fail[item] ? -1 : t;
  }
}

static size_t counts3d_scratch_bytes(int N, int K, int64_t P) {
  const size_t items = (size_t)N * (size_t)K, nw = (size_t)(P / 32 + 1), nblk = (size_t)r3_blocks(P);
  return 4u * (items * (size_t)P + items * 2 * nw + items * nblk * 3 + items);
}

int launch_map_component_counts3d(const float *maps, const uint8_t *masks, const int32_t *labels, const int32_t *regions, int N, int D, int H,
                                  int W, const float *thresholds, int K, int conn, int32_t *counts, void *scratch, hipStream_t s) {
  const char *op = "map_component_counts3d";
  DDPM_CHECK_ARG(maps && masks && labels && regions && thresholds && counts && scratch, "%s: null pointer", op);
  DDPM_CHECK_ARG(K >= 1 && K <= kCountsMaxK, "%s: K must lie in 1 .. %d (got %d)", op, kCountsMaxK, K);
  if (int rc = check_volume(op, N, D, H, W, conn, K)) return rc;
  DDPM_CHECK_ARG(((uintptr_t)maps & 3) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)regions & 3) == 0 &&
                     ((uintptr_t)thresholds & 3) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)scratch & 3) == 0,
                 "%s: maps / labels / regions / thresholds / counts / scratch must be 4-byte aligned", op);
  const int64_t P = (int64_t)D * H * W;
  const double elems = (double)N * (double)P, out_bytes = 12.0 * N * K, sbytes = (double)counts3d_scratch_bytes(N, K, P);
  const void *in[5] = {maps, masks, labels, regions, thresholds};
  const double in_bytes[5] = {4.0 * elems, elems, 4.0 * elems, 4.0 * N, 4.0 * K};
  for (int k = 0; k < 5; ++k)
    DDPM_CHECK_ARG(!pm_overlap(counts, out_bytes, in[k], in_bytes[k]) && !pm_overlap(scratch, sbytes, in[k], in_bytes[k]),
                   "%s: counts / scratch alias an input", op);
  DDPM_CHECK_ARG(!pm_overlap(counts, out_bytes, scratch, sbytes), "%s: counts / scratch alias an input", op);
  const int items = N * K, nw = (int)(P / 32 + 1), nblk = r3_blocks(P);
  int32_t *par = static_cast<int32_t *>(scratch);
  uint32_t *flags = reinterpret_cast<uint32_t *>(par + (size_t)items * (size_t)P);
  int32_t *part = reinterpret_cast<int32_t *>(flags + (size_t)items * 2 * (size_t)nw), *fail = part + (size_t)items * (size_t)nblk * 3;
  ProfScope prof(s, op, 0.0, (4.0 * 3.0 + 4.0 * 8.0 + 5.0) * elems * K + out_bytes);
  if (int rc = launch_cc3_link(SrcThr{maps, thresholds, K, P}, items, P, D, H, W, conn, par, fail, flags, nw, s)) return rc;
  const dim3 grid((unsigned)nblk, (unsigned)items), block(kR3Block);
  hipLaunchKernelGGL(cnt3_mark_kernel, grid, block, 0, s, (int)P, K, nw, par, masks, labels, regions, flags);
  DDPM_CHECK_LAUNCH();
  hipLaunchKernelGGL(cnt3_partial_kernel, grid, block, 0, s, (int)P, nw, nblk, par, flags, part);
  DDPM_CHECK_LAUNCH();
  hipLaunchKernelGGL(cnt3_final_kernel, dim3((unsigned)items), block, 0, s, nblk, part, fail, counts);
  DDPM_CHECK_LAUNCH();
  return 0;
}

}  // namespace ddpm

using namespace ddpm;

extern "C" int64_t ddpm_regions3d_label_scratch_bytes(int N, int D, int H, int W) {
  return r3_extent_ok(N, D, H, W) ? (int64_t)label3d_scratch_bytes(N, (int64_t)D * H * W) : 0;
}

extern "C" int ddpm_map_label3d_u8(const uint8_t *masks, int N, int D, int H, int W, int connectivity, int32_t *labels, int32_t *regions,
                                   void *scratch, ddpm_stream_t stream) {
  return launch_map_label3d<SrcU8, uint8_t>("map_label3d_u8", masks, 0.0f, N, D, H, W, connectivity, labels, regions, scratch,
                                            as_stream(stream));
}

extern "C" int ddpm_map_label3d_f32(const float *maps, float thr, int N, int D, int H, int W, int connectivity, int32_t *labels,
                                    int32_t *regions, void *scratch, ddpm_stream_t stream) {
  return launch_map_label3d<SrcF32, float>("map_label3d_f32", maps, thr, N, D, H, W, connectivity, labels, regions, scratch,
                                           as_stream(stream));
}

extern "C" int64_t ddpm_regions3d_overlap_scratch_bytes(int N, int nbins, int chunk_regions) {
  return N > 0 && nbins >= 1 && nbins <= kHistMaxBins && chunk_regions >= 1 && chunk_regions <= 65536
             ? (int64_t)overlap3d_scratch_bytes(N, nbins, chunk_regions)
             : 0;
}

extern "C" int ddpm_map_region_overlap3d_f32(const float *maps, const int32_t *labels, const int32_t *regions, int N, int64_t P, float lo,
                                             float inv_step, int nbins, int chunk_regions, void *scratch, double *total, int accumulate,
                                             ddpm_stream_t stream) {
  return launch_map_region_overlap3d(maps, labels, regions, N, P, lo, inv_step, nbins, chunk_regions, scratch, total, accumulate,
                                     as_stream(stream));
}

extern "C" int64_t ddpm_regions3d_counts_scratch_bytes(int N, int D, int H, int W, int K) {
  return r3_extent_ok(N, D, H, W) && K >= 1 && K <= kCountsMaxK ? (int64_t)counts3d_scratch_bytes(N, K, (int64_t)D * H * W) : 0;
}

extern "C" int ddpm_map_component_counts3d_f32(const float *maps, const uint8_t *masks, const int32_t *labels, const int32_t *regions,
                                               int N, int D, int H, int W, const float *thresholds, int K, int connectivity,
                                               int32_t *counts, void *scratch, ddpm_stream_t stream) {
  return launch_map_component_counts3d(maps, masks, labels, regions, N, D, H, W, thresholds, K, connectivity, counts, scratch,
                                       as_stream(stream));
}
