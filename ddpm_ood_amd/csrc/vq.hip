// vq.hip -- nearest-code search of the VQ-VAE quantiser (part of SURVEY 8 row f-1).
//
// Replaces EMAQuantizer.quantize + embedding lookup of MONAI-Generative's VQ-VAE (reference call sites
// /root/reference/src/trainers/reconstruct.py:124,166 through vqvae.decode_stage_2_outputs): for every latent vector
// z = x[b, :, p] the code k that minimises |z|^2 + |e_k|^2 - 2 z.e_k (first one on ties, as torch.max(-dist)),
// and the straight-through eval output x + (e_k - x).
// One thread per latent position keeps z in registers; codes are walked by all lanes of a wave together, so the
// codebook row is wave-uniform (scalar loads) and the inner product is D v_fmac with a scalar operand.  The four
// waves of a workgroup take a quarter of the codebook each for the same 64 positions and combine through LDS.
// 2 K D FLOP per position (0.5 MFLOP at K = 2 048, D = 128): VALU-bound, a few hundred microseconds per batch of
// 8^3 latents -- nowhere near the decode convolutions that follow.
// The training step of the EMA quantiser (ddpm_vq_train_{assign,update,backward}_f32) lives here too and runs the SAME search:
// the tile / thread functions below are shared by the eval and the training kernels.
#include "common.h"

namespace ddpm {

constexpr float kVqTieRel = 1e-5f;  // relative distance gap below which two codes count as a near-tie (ddpm_vq_near_ties_read)

// The search of one 64-position tile by the four waves of a workgroup, shared by the eval kernel (ddpm_vq_nearest_f32) and the
// training step's (ddpm_vq_train_assign_f32): loads z, walks the codes, combines the quarters, writes idx and x + (e_idx - x).
// Returns sum_d (e_idx[d] - z[d])^2 of the lane's position (fp64 accumulation of the fp32 differences the output is formed
// from) in wave 0's live lanes, 0 elsewhere -- the eval kernel does not use it and the compiler drops the arithmetic.
template <int D>
__device__ __forceinline__ double vq_search_tile(const float *__restrict__ x, const float *__restrict__ e,
                                                 const float *__restrict__ e2, int *__restrict__ idx, float *__restrict__ out,
                                                 int S, int K, long npos, unsigned *__restrict__ status) {
  __shared__ float bd[4][64], bs[4][64];
  __shared__ int bi[4][64];
  const int lane = threadIdx.x & 63, quarter = threadIdx.x >> 6;
  const long pos = (long)blockIdx.x * 64 + lane;
  const bool live = pos < npos;
  const long b = live ? pos / S : 0, p = live ? pos - b * S : 0;
  const float *xp = x + (size_t)b * D * S + p;
  float z[D];
  float z2 = 0.f;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    z[d] = live ? xp[(size_t)d * S] : 0.f;
    z2 += z[d] * z[d];
  }
  // a non-finite latent picks an arbitrary code: say so
  if (quarter == 0 && non_finite(z2) && status) atomicOr(status, (unsigned)DDPM_STATUS_NONFINITE_LATENT);
  const int kq = (K + 3) / 4, k0 = quarter * kq, k1 = min(K, k0 + kq);
  float best = INFINITY, second = INFINITY;  // (second: the runner-up distance -- only for the near-tie counter below)
  int besti = k0;
  for (int k = k0; k < k1; ++k) {
    const float *ek = e + (size_t)k * D;  // uniform over the wave
    float dot = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) dot = fmaf(z[d], ek[d], dot);
    const float dist = (z2 + e2[k]) - 2.f * dot;
    if (dist < best) {
      second = best;
      best = dist;
      besti = k;
    } else {
      second = fminf(second, dist);
    }
  }
  bd[quarter][lane] = best;
  bi[quarter][lane] = besti;
  bs[quarter][lane] = second;
  __syncthreads();
  double sq = 0.0;
  if (quarter == 0 && live) {
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      if (bd[q][lane] < best) {  // strict: the earlier quarter (smaller index) wins a tie
        second = fminf(best, fminf(second, bs[q][lane]));
        best = bd[q][lane];
        besti = bi[q][lane];
      } else {
        second = fminf(second, bd[q][lane]);
      }
    }
    // a NEAR-TIE: the two nearest codes within kVqTieRel of each other -- a latent that differs in its 6th digit (another
    // machine's convolution rounding, the reference's own included) may pick the other one.  Counted, not flagged.
    if (status && second - best <= kVqTieRel * fabsf(best)) atomicAdd(status + 1, 1u);
    idx[pos] = besti;
    const float *ek = e + (size_t)besti * D;
    float *op = out + (size_t)b * D * S + p;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const float diff = ek[d] - z[d];
      op[(size_t)d * S] = z[d] + diff;  // straight-through form, x + (q - x)
      sq += (double)diff * (double)diff;
    }
  }
  return sq;
}

template <int D>
__global__ __launch_bounds__(256) void vq_nearest_kernel(const float *__restrict__ x, const float *__restrict__ e,
                                                         const float *__restrict__ e2, int *__restrict__ idx,
                                                         float *__restrict__ out, int S, int K, long npos,
                                                         unsigned *__restrict__ status) {
  vq_search_tile<D>(x, e, e2, idx, out, S, K, npos, status);
}

// any embedding_dim (the built sizes above keep z in registers; this one re-reads it, cached, per code): same arithmetic order.
// One position per thread (pos < npos); returns sum_d (e_idx[d] - z[d])^2 as vq_search_tile does.
__device__ __forceinline__ double vq_search_generic(const float *__restrict__ x, const float *__restrict__ e,
                                                    const float *__restrict__ e2, int *__restrict__ idx, float *__restrict__ out,
                                                    int D, int S, int K, long pos, unsigned *__restrict__ status) {
  const long b = pos / S, p = pos - b * S;
  const float *xp = x + (size_t)b * D * S + p;
  float z2 = 0.f;
  for (int d = 0; d < D; ++d) z2 += xp[(size_t)d * S] * xp[(size_t)d * S];
  if (non_finite(z2) && status) atomicOr(status, (unsigned)DDPM_STATUS_NONFINITE_LATENT);
  float best = INFINITY, second = INFINITY;
  int besti = 0;
  for (int k = 0; k < K; ++k) {
    const float *ek = e + (size_t)k * D;
    float dot = 0.f;
    for (int d = 0; d < D; ++d) dot = fmaf(xp[(size_t)d * S], ek[d], dot);
    const float dist = (z2 + e2[k]) - 2.f * dot;
    if (dist < best) {
      second = best;
      best = dist;
      besti = k;
    } else {
      second = fminf(second, dist);
    }
  }
  if (status && second - best <= kVqTieRel * fabsf(best)) atomicAdd(status + 1, 1u);
  idx[pos] = besti;
  const float *ek = e + (size_t)besti * D;
  float *op = out + (size_t)b * D * S + p;
  double sq = 0.0;
  for (int d = 0; d < D; ++d) {
    const float zd = xp[(size_t)d * S];
    const float diff = ek[d] - zd;
    op[(size_t)d * S] = zd + diff;
    sq += (double)diff * (double)diff;
  }
  return sq;
}

__global__ __launch_bounds__(256) void vq_nearest_generic_kernel(const float *__restrict__ x, const float *__restrict__ e,
                                                                 const float *__restrict__ e2, int *__restrict__ idx,
                                                                 float *__restrict__ out, int D, int S, int K, long npos,
                                                                 unsigned *__restrict__ status) {
  const long pos = (long)blockIdx.x * 256 + threadIdx.x;
  if (pos >= npos) return;
  vq_search_generic(x, e, e2, idx, out, D, S, K, pos, status);
}

// ---- training step of the EMA quantiser (MONAI-Generative's EMAQuantizer in training mode) -----------------------------------
// assign: the search above + per-workgroup partial sums of (e_idx - x)^2; sums: per-code counts and sums of the assigned latents
// in ascending position order (no float atomics: bit-identical run to run) + the loss scalar; update: the EMA lines and the
// new codebook in one launch; backward: straight-through + commitment gradient.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int D>
__global__ __launch_bounds__(256) void vq_train_assign_kernel(const float *__restrict__ x, const float *__restrict__ e,
                                                              const float *__restrict__ e2, int *__restrict__ idx,
                                                              float *__restrict__ out, int S, int K, long npos,
                                                              unsigned *__restrict__ status, double *__restrict__ partial) {
  double sq = vq_search_tile<D>(x, e, e2, idx, out, S, K, npos, status);
  if (threadIdx.x < 64) {  // wave 0 finished the tile's positions
    sq = wave_sum_f64(sq);
    if (threadIdx.x == 0) partial[blockIdx.x] = sq;
  }
}

__global__ __launch_bounds__(256) void vq_train_assign_generic_kernel(const float *__restrict__ x, const float *__restrict__ e,
                                                                      const float *__restrict__ e2, int *__restrict__ idx,
                                                                      float *__restrict__ out, int D, int S, int K, long npos,
                                                                      unsigned *__restrict__ status, double *__restrict__ partial) {
  __shared__ double red[4];
  const long pos = (long)blockIdx.x * 256 + threadIdx.x;
  double sq = pos < npos ? vq_search_generic(x, e, e2, idx, out, D, S, K, pos, status) : 0.0;
  sq = wave_sum_f64(sq);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One wave per (code k, 64 channels): walks idx in ascending position order, 64 positions per coalesced load, and adds the
// latents of the positions assigned to k -- recursive summation in a fixed order, so dw is bit-identical run to run; the count
// is the number of matches (exact).  The match mask is wave-uniform (a ballot), so the loop over its bits does not diverge.
// Workgroup (0, 0) also folds the assign kernel's partial sums into the loss (fixed order, fp64).
__global__ __launch_bounds__(64) void vq_train_sums_kernel(const float *__restrict__ x, const int *__restrict__ idx,
                                                           float *__restrict__ counts, float *__restrict__ dw,
                                                           const double *__restrict__ partial, int nparts, float *__restrict__ loss,
                                                           double loss_scale, int D, int S, long npos) {
  const int k = blockIdx.x, lane = threadIdx.x, d = blockIdx.y * 64 + lane;
  const bool mine = d < D;
  float acc = 0.f;
  int cnt = 0;
  for (long base = 0; base < npos; base += 64) {
    const long p = base + lane;
    const int v = p < npos ? idx[p] : -1;
    unsigned long long m = __ballot(v == k);
    cnt += __popcll(m);
    while (m) {
      const long q = base + (__ffsll((long long)m) - 1);
      m &= m - 1;
      const long b = q / S, s = q - b * S;
      if (mine) acc += x[((size_t)b * D + d) * S + s];
    }
  }
  if (mine) dw[(size_t)k * D + d] = acc;
  if (blockIdx.y == 0 && lane == 0) counts[k] = (float)cnt;
  if (k == 0 && blockIdx.y == 0) {
    double t = 0.0;
    for (int i = lane; i < nparts; i += 64) t += partial[i];
    t = wave_sum_f64(t);
    if (lane == 0) loss[0] = (float)(t * loss_scale);
  }
}

// cs <- decay cs + (1 - decay) counts; n = sum cs; w_k = (cs_k + eps) / (n + K eps) n; ema_w <- decay ema_w + (1 - decay) dw;
// codebook_k <- ema_w_k / w_k.  ONE workgroup: n needs every new cs before any code is divided, and the update is in place.
// fp64 arithmetic between the fp32 loads and stores (each stored value is rounded once).  A dead code (counts_k = 0) only
// decays; w_k > 0 whenever anything was ever assigned (n > 0), and with n = 0 the codebook is left as it is.
__global__ __launch_bounds__(1024) void vq_train_update_kernel(float *__restrict__ cs, float *__restrict__ ema_w,
                                                               float *__restrict__ codebook, const float *__restrict__ counts,
                                                               const float *__restrict__ dw, int K, int D, double decay, double eps) {
  __shared__ double red[16];
  __shared__ float cs_new[1024];
  const int tid = threadIdx.x;
  double part = 0.0;
  for (int k = tid; k < K; k += 1024) {
    const float c = (float)(decay * (double)cs[k] + (1.0 - decay) * (double)counts[k]);
    cs[k] = c;
    part += (double)c;
  }
  part = wave_sum_f64(part);
  if ((tid & 63) == 0) red[tid >> 6] = part;
  __syncthreads();
  double n = 0.0;
#pragma unroll
  for (int w = 0; w < 16; ++w) n += red[w];
  const double denom = n + (double)K * eps;
  // codes in chunks of 1024: the chunk's new cluster sizes go through LDS, then all threads walk the chunk's K' x D entries
  for (int kb = 0; kb < K; kb += 1024) {
    __syncthreads();
    if (kb + tid < K) cs_new[tid] = cs[kb + tid];
    __syncthreads();
    const int kn = min(1024, K - kb);
    const long cnt = (long)kn * D;
    for (long i = tid; i < cnt; i += 1024) {
      const int kl = (int)(i / D);
      const size_t g = (size_t)kb * D + i;
      const float m = (float)(decay * (double)ema_w[g] + (1.0 - decay) * (double)dw[g]);
      ema_w[g] = m;
      const double w = ((double)cs_new[kl] + eps) / denom * n;
      if (w > 0.0) codebook[g] = (float)((double)m / w);
    }
  }
}

// dx = dout + (2 commitment_cost / n) (x - e_idx) dloss, elementwise over [B, D, S] (dout / dloss may be NULL: that term is 0)
__global__ __launch_bounds__(256) void vq_train_backward_kernel(const float *__restrict__ dout, const float *__restrict__ x,
                                                                const float *__restrict__ e, const int *__restrict__ idx,
                                                                const float *__restrict__ dloss, float *__restrict__ dx, int D,
                                                                int S, long n, double coef) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long plane = (long)D * S;
  const long b = i / plane, r = i - b * plane;
  const int d = (int)(r / S);
  const long s = r - (long)d * S;
  double g = dout ? (double)dout[i] : 0.0;
  if (dloss) g += coef * ((double)x[i] - (double)e[(size_t)idx[b * S + s] * D + d]) * (double)dloss[0];
  dx[i] = (float)g;
}

__global__ void vq_code_norms_kernel(const float *__restrict__ e, float *__restrict__ e2, int K, int D) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  float s = 0.f;
  for (int d = 0; d < D; ++d) s += e[(size_t)k * D + d] * e[(size_t)k * D + d];
  e2[k] = s;
}

int launch_vq_nearest(const float *x, const float *codebook, float *code_norms, int *idx, float *out, int B, int D, long S,
                      int K, hipStream_t s) {
  DDPM_CHECK_ARG(x && codebook && code_norms && idx && out, "vq_nearest: null pointer");
  DDPM_CHECK_ARG(B > 0 && S > 0 && K > 0, "vq_nearest: empty shape");
  DDPM_CHECK_ARG(D > 0, "vq_nearest: embedding_dim %d", D);
  DDPM_CHECK_ARG(S < (1L << 31), "vq_nearest: too many positions per image");
  const long npos = (long)B * S;
  hipLaunchKernelGGL(vq_code_norms_kernel, dim3((K + 255) / 256), dim3(256), 0, s, codebook, code_norms, K, D);
  ProfScope prof(s, "vq_nearest", 2.0 * npos * K * D, 4.0 * (2.0 * npos * D + (double)K * D));
  const dim3 grid((unsigned)((npos + 63) / 64));
#define DDPM_VQ_CASE(DD)                                                                                             \
  case DD:                                                                                                           \
    hipLaunchKernelGGL(vq_nearest_kernel<DD>, grid, dim3(256), 0, s, x, codebook, code_norms, idx, out, (int)S, K, npos, \
                       status_word());                                                                                   \
    break;
  switch (D) {
    DDPM_VQ_CASE(8)
    DDPM_VQ_CASE(16)
    DDPM_VQ_CASE(32)
    DDPM_VQ_CASE(64)
    DDPM_VQ_CASE(128)
    default:  // other embedding sizes: the generic kernel (x and out must not alias)
      hipLaunchKernelGGL(vq_nearest_generic_kernel, dim3((unsigned)((npos + 255) / 256)), dim3(256), 0, s, x, codebook, code_norms,
                         idx, out, D, (int)S, K, npos, status_word());
      break;
  }
#undef DDPM_VQ_CASE
  DDPM_CHECK_LAUNCH();
  return 0;
}

int launch_vq_train_assign(const float *x, const float *codebook, float *code_norms, int *idx, float *out, float *counts,
                           float *dw, float *loss, double *partial, int B, int D, long S, int K, float commitment_cost,
                           hipStream_t s) {
  DDPM_CHECK_ARG(x && codebook && code_norms && idx && out && counts && dw && loss && partial, "vq_train_assign: null pointer");
  DDPM_CHECK_ARG(B > 0 && S > 0 && K > 0 && D > 0, "vq_train_assign: empty shape");
  DDPM_CHECK_ARG(S < (1L << 31) && (long)B * S < (1L << 31), "vq_train_assign: too many positions");
  const long npos = (long)B * S;
  hipLaunchKernelGGL(vq_code_norms_kernel, dim3((K + 255) / 256), dim3(256), 0, s, codebook, code_norms, K, D);
  ProfScope prof(s, "vq_train_assign", 2.0 * npos * K * D, 4.0 * (3.0 * npos * D + 2.0 * K * D));
  const bool generic = !(D == 8 || D == 16 || D == 32 || D == 64 || D == 128);
  const int nparts = (int)(generic ? (npos + 255) / 256 : (npos + 63) / 64);
  const dim3 grid((unsigned)nparts);
#define DDPM_VQ_CASE(DD)                                                                                                   \
  case DD:                                                                                                                 \
    hipLaunchKernelGGL(vq_train_assign_kernel<DD>, grid, dim3(256), 0, s, x, codebook, code_norms, idx, out, (int)S, K, npos, \
                       status_word(), partial);                                                                            \
    break;
  switch (D) {
    DDPM_VQ_CASE(8)
    DDPM_VQ_CASE(16)
    DDPM_VQ_CASE(32)
    DDPM_VQ_CASE(64)
    DDPM_VQ_CASE(128)
    default:
      hipLaunchKernelGGL(vq_train_assign_generic_kernel, grid, dim3(256), 0, s, x, codebook, code_norms, idx, out, D, (int)S, K,
                         npos, status_word(), partial);
      break;
  }
#undef DDPM_VQ_CASE
  DDPM_CHECK_LAUNCH();
  const double loss_scale = (double)commitment_cost / ((double)npos * D);
  hipLaunchKernelGGL(vq_train_sums_kernel, dim3((unsigned)K, (unsigned)((D + 63) / 64)), dim3(64), 0, s, x, idx, counts, dw,
                     partial, nparts, loss, loss_scale, D, (int)S, npos);
  DDPM_CHECK_LAUNCH();
  return 0;
}

}  // namespace ddpm

using namespace ddpm;

extern "C" int ddpm_vq_near_ties_read(unsigned *count, int clear, ddpm_stream_t stream) {
  DDPM_CHECK_ARG(count != nullptr, "vq_near_ties_read: NULL pointer");
  unsigned *st = status_word();
  DDPM_CHECK_ARG(st != nullptr, "vq_near_ties_read: no status word on this device");
  hipError_t e = hipMemcpyAsync(count, st + 1, sizeof(unsigned), hipMemcpyDeviceToHost, as_stream(stream));
  if (e == hipSuccess && clear) e = hipMemsetAsync(st + 1, 0, sizeof(unsigned), as_stream(stream));
  if (e == hipSuccess) e = hipStreamSynchronize(as_stream(stream));
  if (e != hipSuccess) {
    set_error("vq_near_ties_read: %s", hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

extern "C" int ddpm_vq_nearest_f32(const float *x, const float *codebook, float *code_norms, int *idx, float *out, int B,
                                   int D, int64_t S, int K, ddpm_stream_t stream) {
  return launch_vq_nearest(x, codebook, code_norms, idx, out, B, D, (long)S, K, as_stream(stream));
}

extern "C" size_t ddpm_vq_train_partials(int B, int D, int64_t S) {
  if (B <= 0 || D <= 0 || S <= 0) return 0;
  const long npos = (long)B * S;
  const bool generic = !(D == 8 || D == 16 || D == 32 || D == 64 || D == 128);
  return (size_t)(generic ? (npos + 255) / 256 : (npos + 63) / 64);
}

extern "C" int ddpm_vq_train_assign_f32(const float *x, const float *codebook, float *code_norms, int *idx, float *out,
                                        float *counts, float *dw, float *loss, double *partials, int B, int D, int64_t S, int K,
                                        float commitment_cost, ddpm_stream_t stream) {
  return launch_vq_train_assign(x, codebook, code_norms, idx, out, counts, dw, loss, partials, B, D, (long)S, K, commitment_cost,
                                as_stream(stream));
}

extern "C" int ddpm_vq_train_update_f32(float *ema_cluster_size, float *ema_w, float *codebook, const float *counts,
                                        const float *dw, int K, int D, float decay, float epsilon, ddpm_stream_t stream) {
  DDPM_CHECK_ARG(ema_cluster_size && ema_w && codebook && counts && dw, "vq_train_update: null pointer");
  DDPM_CHECK_ARG(K > 0 && D > 0, "vq_train_update: empty shape");
  DDPM_CHECK_ARG(decay >= 0.f && decay <= 1.f && epsilon >= 0.f, "vq_train_update: decay %g / epsilon %g", (double)decay,
                 (double)epsilon);
  hipStream_t s = as_stream(stream);
  ProfScope prof(s, "vq_train_update", 5.0 * K * D, 4.0 * (4.0 * K * D + 3.0 * K));
  hipLaunchKernelGGL(vq_train_update_kernel, dim3(1), dim3(1024), 0, s, ema_cluster_size, ema_w, codebook, counts, dw, K, D,
                     (double)decay, (double)epsilon);
  DDPM_CHECK_LAUNCH();
  return 0;
}

extern "C" int ddpm_vq_train_backward_f32(const float *dout, const float *x, const float *codebook, const int *idx,
                                          const float *dloss, float *dx, int B, int D, int64_t S, float commitment_cost,
                                          ddpm_stream_t stream) {
  DDPM_CHECK_ARG(x && codebook && idx && dx, "vq_train_backward: null pointer");
  DDPM_CHECK_ARG(B > 0 && D > 0 && S > 0 && S < (1L << 31), "vq_train_backward: bad shape");
  const long n = (long)B * D * S;
  DDPM_CHECK_ARG((n + 255) / 256 < (1L << 31), "vq_train_backward: too many elements");
  const double coef = 2.0 * (double)commitment_cost / (double)n;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(vq_train_backward_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dout, x, codebook, idx, dloss,
                     dx, D, (int)S, n, coef);
  DDPM_CHECK_LAUNCH();
  return 0;
}
