// What regions3d.hip and segment3d.hip share: the union-find labelling of volumes in global memory, launches 1 .. 3 (the header
// comment of regions3d.hip describes it), the sum and the scan over a workgroup, and the checks of an extent.
// (cc3_flatten_kernel is no template and lives in a header: `inline`, so that the two translation units may both hold it.)
#pragma once
#include "pixel_common.h"
#include "regions_common.h"

namespace ddpm {

constexpr int kR3Block = 256;
constexpr int kR3Waves = kR3Block / 64;
constexpr int kR3MaxItems = 65535;  // blockIdx.y

struct SrcU8 {
  const uint8_t *m;
  int64_t P;
  __device__ __forceinline__ PredU8 at(int item) const { return PredU8(m + (int64_t)item * P, 0.0f); }
};
struct SrcF32 {
  const float *v;
  float thr;
  int64_t P;
  __device__ __forceinline__ PredGt at(int item) const { return PredGt(v + (int64_t)item * P, thr); }
};
struct SrcThr {  // item = n * K + k
  const float *v;
  const float *thr;
  int K;
  int64_t P;
  __device__ __forceinline__ PredGt at(int item) const { return PredGt(v + (int64_t)(item / K) * P, thr[item % K]); }
};

__device__ __forceinline__ int32_t g3_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The walk towards the root: 0 <= par[i] <= i for every voxel inside, so the index strictly descends until par[i] == i: fewer
// than P steps.  (A negative parent would be a background voxel, which no walk starts at or is led to: the walk stops there too.)
__device__ __forceinline__ int g3_find(const int32_t *par, int i, int P) {
  for (int s = 0; s < P; ++s) {
    const int32_t q = g3_load(par + i);
    if (q < 0 || q >= i) break;
    i = q;
  }
  return i;
}

// The trees of a and b joined.  A round ends the loop (one root, or the larger root hung below the smaller while it still was a
// root) or goes on with the pair (what the larger root pointed at instead, the smaller root), both below the larger root: the
// larger of the two indices, below P, strictly descends, so at most P rounds.
__device__ __forceinline__ void g3_union(int32_t *par, int a, int b, int P, int32_t *fail) {
  for (int t = 0; t < P; ++t) {
    a = g3_find(par, a, P);
    b = g3_find(par, b, P);
    if (a == b) return;
    if (a < b) {
      const int c = a;
      a = b;
      b = c;
    }
    const int32_t old = __hip_atomic_fetch_min(par + a, (int32_t)b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    if (old < 0 || old > a) break;  // (never: a parent inside is in 0 .. its voxel)
    a = old;                        // (a had been hung below `old` by another thread: old and b are still to be joined)
  }
  __hip_atomic_fetch_or(fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// sum over the workgroup, to every thread (two barriers)
__device__ __forceinline__ int r3_block_sum(int v, int *sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();  // (sh may still be read from the call before)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < kR3Waves; ++w) t += sh[w];
  return t;
}

// exclusive prefix over the workgroup in thread order; *total to every thread (two barriers)
__device__ __forceinline__ int r3_block_scan(int v, int *sh, int *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  __syncthreads();
  if (lane == 63) sh[wave] = incl;
  __syncthreads();
  int base = 0, t = 0;
#pragma unroll
  for (int w = 0; w < kR3Waves; ++w) {
    const int u = sh[w];
    base += w < wave ? u : 0;
    t += u;
  }
  *total = t;
  return base + incl - v;
}

// ---- launch 1: runs along w ----------------------------------------------------------------------------------------------
// zero_words != nullptr: the item's 2 nw flag words (component counts) are zeroed here too.
template <class Src>
__global__ __launch_bounds__(kR3Block) void cc3_init_kernel(Src src, int P, int W, int32_t *__restrict__ par_all, int32_t *__restrict__ fail,
                                                            uint32_t *__restrict__ zero_words, int nw) {
  const int item = blockIdx.y, lane = threadIdx.x & 63;
  const int64_t ii = (int64_t)blockIdx.x * kR3Block + threadIdx.x;
  const bool valid = ii < P;
  const int i = valid ? (int)ii : 0;
  const auto pred = src.at(item);
  const int x = i % W;
  const bool in = valid && pred(i);
  const unsigned long long stop = __ballot(!in), rows = __ballot(valid && x == 0);
  if (ii == 0) fail[item] = 0;
  if (zero_words && ii < nw) {
    zero_words[(int64_t)item * 2 * nw + ii] = 0u;
    zero_words[(int64_t)item * 2 * nw + nw + ii] = 0u;
  }
  if (!valid) return;
  int32_t p = -1;
  if (in) {
    const unsigned long long upto = (2ull << lane) - 1ull;  // lanes 0 .. lane (lane 63: all)
    const unsigned long long m = (stop | rows) & upto;
    if (m == 0ull) {  // the run reaches the wave's first voxel, which is not the first of its row
      p = lane == 0 ? (pred(i - 1) ? i - 1 : i) : i - lane;
    } else {
      const int j = 63 - __builtin_clzll(m);
      p = i - lane + (((stop >> j) & 1ull) ? j + 1 : j);
    }
  }
  par_all[(int64_t)item * P + i] = p;
}

// ---- launch 2: unions ------------------------------------------------------------------------------------------------------
// (u: the voxel of the other row at this x, ul / ur: its neighbours, l / r: this voxel's.)  The run that holds u is joined by the
// first voxel of this run beside it; where x diagonals count, a run that ends at ul or begins at ur touches too, and is joined
// here unless the left / right neighbour sees it straight beside itself.  The other rows are the four that precede this one in
// flat order: (dz, dy) = (0, -1), (-1, -1), (-1, 0), (-1, 1).  6 neighbours: the two with one step, no diagonal; 18: all four,
// the x diagonal only where the row is one step away; 26: all four with the diagonal.
template <class Src>
__global__ __launch_bounds__(kR3Block) void cc3_union_kernel(Src src, int P, int D, int H, int W, int conn, int32_t *__restrict__ par_all,
                                                             int32_t *__restrict__ fail) {
  const int item = blockIdx.y;
  const int64_t ii = (int64_t)blockIdx.x * kR3Block + threadIdx.x;
  if (ii >= P) return;
  const int i = (int)ii;
  const auto pred = src.at(item);
  if (!pred(i)) return;
  int32_t *par = par_all + (int64_t)item * P;
  const int x = i % W, t = i / W, y = t % H, z = t / H, HW = H * W;
  const bool l = x > 0 && pred(i - 1), r = x + 1 < W && pred(i + 1);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int dz = k == 0 ? 0 : -1, dy = k < 2 ? -1 : k - 2;
    if (z + dz < 0 || y + dy < 0 || y + dy >= H) continue;
    const int steps = (dz != 0) + (dy != 0);
    if (conn == 6 && steps != 1) continue;
    const bool diag = conn == 26 || (conn == 18 && steps == 1);
    const int j = i + dz * HW + dy * W;
    if (pred(j)) {
      if (!(l && pred(j - 1))) g3_union(par, i, j, P, fail + item);
    } else if (diag) {
      if (!l && x > 0 && pred(j - 1)) g3_union(par, i, j - 1, P, fail + item);
      if (!r && x + 1 < W && pred(j + 1)) g3_union(par, i, j + 1, P, fail + item);
    }
  }
}

// ---- launch 3: flatten -----------------------------------------------------------------------------------------------------
inline __global__ __launch_bounds__(kR3Block) void cc3_flatten_kernel(int P, int32_t *__restrict__ par_all) {
  const int64_t ii = (int64_t)blockIdx.x * kR3Block + threadIdx.x;
  if (ii >= P) return;
  int32_t *par = par_all + (int64_t)blockIdx.y * P;
  const int i = (int)ii;
  if (g3_load(par + i) < 0) return;
  par[i] = g3_find(par, i, P);
}

static inline int r3_blocks(int64_t P) { return (int)((P + kR3Block - 1) / kR3Block); }

static int check_volume(const char *op, int N, int D, int H, int W, int conn, int items) {
  DDPM_CHECK_ARG(N > 0 && D > 0 && H > 0 && W > 0, "%s: N, D, H and W must be positive (got %d, %d, %d, %d)", op, N, D, H, W);
  DDPM_CHECK_ARG((double)D * H * W < 2147483648.0, "%s: a volume of %d x %d x %d voxels is not below 2^31", op, D, H, W);
  DDPM_CHECK_ARG(conn == 6 || conn == 18 || conn == 26, "%s: connectivity must be 6, 18 or 26 (got %d)", op, conn);
  DDPM_CHECK_ARG((int64_t)N * items <= kR3MaxItems, "%s: at most %d volumes (times thresholds) per call (got %lld)", op, kR3MaxItems,
                 (long long)N * items);
  return 0;
}

// launches 1 .. 3 for `items` volumes: on return (in stream order) par[i] is the smallest flat index of voxel i's component
template <class Src>
static int launch_cc3_link(Src src, int items, int64_t P, int D, int H, int W, int conn, int32_t *par, int32_t *fail, uint32_t *zero_words,
                           int nw, hipStream_t s) {
  const dim3 grid((unsigned)r3_blocks(P), (unsigned)items), block(kR3Block);
  hipLaunchKernelGGL((cc3_init_kernel<Src>), grid, block, 0, s, src, (int)P, W, par, fail, zero_words, nw);
  DDPM_CHECK_LAUNCH();
  hipLaunchKernelGGL((cc3_union_kernel<Src>), grid, block, 0, s, src, (int)P, D, H, W, conn, par, fail);
  DDPM_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc3_flatten_kernel, grid, block, 0, s, (int)P, par);
  DDPM_CHECK_LAUNCH();
  return 0;
}

static bool r3_extent_ok(int N, int D, int H, int W) { return N > 0 && D > 0 && H > 0 && W > 0 && (double)D * H * W < 2147483648.0; }

}  // namespace ddpm
