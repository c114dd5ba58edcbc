// What regions.hip and segment.hip share: the LDS union-find labelling of a plane (the header comment of regions.hip describes it).
#pragma once
#include "pixel_common.h"

namespace ddpm {

constexpr int kRgBlock = 1024;
constexpr int kRgWaves = kRgBlock / 64;
constexpr int kRgMaxPixels = 16384;  // 128 x 128: the parents fill 32 KB
constexpr uint32_t kRgBg = 0xffffu;
constexpr uint32_t kRgRootTag = 0x8000u;

struct CcShared {
  uint32_t words[kRgMaxPixels / 2];  // the parents, two 16-bit halves per dword
  int wsum[kRgWaves];
  int fail;
};

struct PredU8 {
  const uint8_t *m;
  __device__ PredU8(const uint8_t *p, float) : m(p) {}
  __device__ __forceinline__ bool operator()(int i) const { return m[i] != 0; }
};
struct PredGt {
  const float *v;
  float thr;
  __device__ PredGt(const float *p, float t) : v(p), thr(t) {}
  __device__ __forceinline__ bool operator()(int i) const { return v[i] > thr; }  // (a NaN pixel, or a NaN threshold: outside)
};

// The walk towards the root.  par[i] <= i for every pixel at every moment, so the index strictly descends until par[i] == i:
// fewer than P steps.
__device__ __forceinline__ uint32_t cc_find(const volatile uint16_t *par, uint32_t i, int P) {
  for (int s = 0; s < P; ++s) {
    const uint32_t q = par[i];
    if (q >= i) break;
    i = q;
  }
  return i;
}

// par[i] = min(par[i], v) for the 16-bit half i of the dword array; returns the value found.  The CAS fails only when another
// thread has lowered one of the dword's two halves in between; a half holds an index below P and only ever decreases, so the
// dword changes fewer than 2 P times: that many tries at the most.
__device__ __forceinline__ uint32_t cc_min16(uint32_t *words, uint32_t i, uint32_t v, int P, int *fail) {
  uint32_t *w = words + (i >> 1);
  const int sh = (int)(i & 1u) * 16;
  uint32_t cur = *reinterpret_cast<volatile uint32_t *>(w);
  for (int t = 0; t < 2 * P; ++t) {
    const uint32_t old = (cur >> sh) & 0xffffu;
    if (old <= v) return old;
    const uint32_t seen = atomicCAS(w, cur, (cur & ~(0xffffu << sh)) | (v << sh));
    if (seen == cur) return old;
    cur = seen;
  }
  *fail = 1;
  return v;
}

// The trees of a and b joined.  A round ends the loop (one root, or the larger root hung below the smaller while it still was a
// root) or goes on with the pair (what the larger root pointed at instead, the smaller root), both below the larger root: the
// larger of the two indices, below P, strictly descends, so at most P rounds.
__device__ __forceinline__ void cc_union(CcShared &sh, uint32_t a, uint32_t b, int P) {
  const volatile uint16_t *par = reinterpret_cast<const volatile uint16_t *>(sh.words);
  for (int t = 0; t < P; ++t) {
    a = cc_find(par, a, P);
    b = cc_find(par, b, P);
    if (a == b) return;
    if (a < b) {
      const uint32_t c = a;
      a = b;
      b = c;
    }
    const uint32_t old = cc_min16(sh.words, a, b, P, &sh.fail);
    if (old == a) return;
    a = old;  // (a had been hung below `old` by another thread: old and b are still to be joined)
  }
  sh.fail = 1;
}

// Steps 1 .. 3: on return (after a barrier) par[i] is the smallest flat index of pixel i's component, 0xffff outside.
template <class Pred>
__device__ void cc_link(CcShared &sh, Pred inside, int H, int W, int conn) {
  volatile uint16_t *par = reinterpret_cast<volatile uint16_t *>(sh.words);
  const int P = H * W, tid = threadIdx.x;
  if (tid == 0) {
    sh.fail = 0;
    if (P & 1) par[P] = (uint16_t)kRgBg;  // (the other half of the last dword: the CAS reads it)
  }
  for (int i = tid; i < P; i += kRgBlock) {
    const int x = i % W;
    par[i] = (uint16_t)(inside(i) ? ((x > 0 && inside(i - 1)) ? i - 1 : i) : (int)kRgBg);
  }
  __syncthreads();
  // 1: after pass k a pixel points at its run's first pixel or at least 2^k pixels to the left (a parent read while its owner
  // rewrites it is the old or the new one, the new one further left), so ceil(log2 W) passes flatten every run; a pass that
  // changes nothing ends the loop sooner
  int passes = 0;
  while (passes < 14 && (1 << passes) < W) ++passes;  // (W <= 16 384 = 2^14)
  for (int k = 0, changed = 1; k < passes && changed; ++k) {
    int c = 0;
    for (int i = tid; i < P; i += kRgBlock) {
      const uint32_t q = par[i];
      if (q != kRgBg && q != (uint32_t)i) {
        const uint32_t qq = par[q];
        if (qq != q) {
          par[i] = (uint16_t)qq;
          c = 1;
        }
      }
    }
    changed = __syncthreads_or(c);
  }
  // 2: (u: the pixel above, ul / ur: above left / right, l / r: left / right.)  The run above that holds u is joined by the
  // first pixel of this run below it; with 8 neighbours a run that ends at ul or begins at ur touches too, and is joined here
  // unless the left / right neighbour sees it straight above itself.
  for (int i = tid; i < P; i += kRgBlock) {
    if (par[i] == kRgBg || i < W) continue;
    const int x = i % W;
    const bool l = x > 0 && par[i - 1] != kRgBg, r = x + 1 < W && par[i + 1] != kRgBg;
    const bool u = par[i - W] != kRgBg, ul = x > 0 && par[i - W - 1] != kRgBg, ur = x + 1 < W && par[i - W + 1] != kRgBg;
    if (u) {
      if (!(l && ul)) cc_union(sh, (uint32_t)i, (uint32_t)(i - W), P);
    } else if (conn == 8) {
      if (ul && !l) cc_union(sh, (uint32_t)i, (uint32_t)(i - W - 1), P);
      if (ur && !r) cc_union(sh, (uint32_t)i, (uint32_t)(i - W + 1), P);
    }
  }
  __syncthreads();
  // 3: only first pixels of runs were ever roots; they find their root first, the rest is then two steps away at the most
  for (int i = tid; i < P; i += kRgBlock) {
    if (par[i] == kRgBg) continue;
    if (i % W == 0 || par[i - 1] == kRgBg) par[i] = (uint16_t)cc_find(par, (uint32_t)i, P);
  }
  __syncthreads();
  for (int i = tid; i < P; i += kRgBlock) {
    if (par[i] == kRgBg) continue;
    if (!(i % W == 0 || par[i - 1] == kRgBg)) par[i] = (uint16_t)cc_find(par, (uint32_t)i, P);
  }
  __syncthreads();
}

// Step 4: the roots numbered 1 .. R in ascending flat index; a root's parent becomes kRgRootTag | number.  Returns R (to every
// thread, after a barrier).
__device__ int cc_compact(CcShared &sh, int P) {
  volatile uint16_t *par = reinterpret_cast<volatile uint16_t *>(sh.words);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = (P + kRgBlock - 1) / kRgBlock, lo = min(tid * chunk, P), hi = min(lo + chunk, P);
  int c = 0;
  for (int i = lo; i < hi; ++i) c += par[i] == (uint32_t)i ? 1 : 0;
  int incl = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) sh.wsum[wave] = incl;
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kRgWaves; ++w) {
    const int v = sh.wsum[w];
    base += w < wave ? v : 0;
    total += v;
  }
  int rank = base + incl - c;
  for (int i = lo; i < hi; ++i)
    if (par[i] == (uint32_t)i) par[i] = (uint16_t)(kRgRootTag | (uint32_t)(++rank));
  __syncthreads();
  return total;
}

}  // namespace ddpm
