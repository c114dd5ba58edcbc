// elementwise.hip -- the HBM-bound kernels around the UNet: timestep embedding, add_noise,
// fused PLMS step, clamp + per-image MSE.  All are 16-byte-per-lane grid-stride streams.
//
// Reference call sites (all /root/reference/src/trainers/reconstruct.py):
//   add_noise   :143-147   scheduler.add_noise(images * b_scale, noise, t)
//   plms_step   :155-157   scheduler.step(model_output, step, reconstructions)
//   clamp_mse   :167-168, :188-191   x / b_scale; clamp_(0, 1); square(orig - x).mean(non-batch)
// Algorithmic bytes per element: add_noise 12, plms_step 8 + 4 * n_eps, clamp_mse 12.
// Beside them, only with --anomaly_maps 1: sqerr_map, the per-pixel squared error clamp_mse reduces away.
#include "common.h"

namespace ddpm {

// ---- get_timestep_embedding: cos first, then sin --------------------------------
__global__ void timestep_embedding_kernel(const int64_t *__restrict__ t, const float *__restrict__ freqs,
                                          float *__restrict__ out, int B, int dim) {
  const int half = dim >> 1;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * dim) return;
  const int b = i / dim, c = i - b * dim;
  float v = 0.f;  // odd dim: last column is the zero pad
  if (c < 2 * half) {
    const float arg = (float)t[b] * freqs[c < half ? c : c - half];
    v = (c < half) ? cosf(arg) : sinf(arg);
  }
  out[i] = v;
}

int launch_timestep_embedding(const int64_t *t, const float *freqs, float *out, int B, int dim, hipStream_t s) {
  DDPM_CHECK_ARG(t && freqs && out && B > 0 && dim > 1, "timestep_embedding: bad argument");
  const int total = B * dim;
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3((total + 255) / 256), dim3(256), 0, s, t, freqs, out, B, dim);
  DDPM_CHECK_LAUNCH();
  return 0;
}

// ---- add_noise ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void add_noise_kernel(const float *__restrict__ x0, const float *__restrict__ noise,
                                                        float *__restrict__ out, float sa, float sb, float b_scale,
                                                        int64_t numel) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = numel >> 2;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 x = reinterpret_cast<const float4 *>(x0)[i];
    const float4 e = reinterpret_cast<const float4 *>(noise)[i];
    float4 o;
    o.x = sa * (x.x * b_scale) + sb * e.x;
    o.y = sa * (x.y * b_scale) + sb * e.y;
    o.z = sa * (x.z * b_scale) + sb * e.z;
    o.w = sa * (x.w * b_scale) + sb * e.w;
    reinterpret_cast<float4 *>(out)[i] = o;
  }
  for (int64_t i = (n4 << 2) + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < numel; i += stride)
    out[i] = sa * (x0[i] * b_scale) + sb * noise[i];
}

static int stream_grid(int64_t numel) {
  int64_t b = (numel / 4 + 255) / 256;
  if (b < 1) b = 1;
  if (b > 2048) b = 2048;
  return (int)b;
}

int launch_add_noise(const float *x0, const float *noise, const float *h_sa, const float *h_sb, float b_scale,
                     float *out, int B, int64_t chw, hipStream_t s) {
  DDPM_CHECK_ARG(x0 && noise && h_sa && h_sb && out && B > 0 && chw > 0, "add_noise: bad argument");
  DDPM_CHECK_ARG((chw & 3) == 0 || B == 1, "add_noise: C*H*W must be a multiple of 4");
  // The path always uses one t for the whole batch (reconstruct.py:130); coalesce equal runs.
  int b0 = 0;
  while (b0 < B) {
    int b1 = b0 + 1;
    while (b1 < B && h_sa[b1] == h_sa[b0] && h_sb[b1] == h_sb[b0]) ++b1;
    const int64_t n = (int64_t)(b1 - b0) * chw;
    hipLaunchKernelGGL(add_noise_kernel, dim3(stream_grid(n)), dim3(256), 0, s, x0 + (int64_t)b0 * chw,
                       noise + (int64_t)b0 * chw, out + (int64_t)b0 * chw, h_sa[b0], h_sb[b0], b_scale, n);
    DDPM_CHECK_LAUNCH();
    b0 = b1;
  }
  return 0;
}

// ---- fused PLMS step -----------------------------------------------------------------------------
// Expressions kept in the reference's evaluation order:
//   kind 1: (e0 + e1) / 2          kind 2: (3 e0 - e1) / 2
//   kind 3: (23 e0 - 16 e1 + 5 e2) / 12
//   kind 4: (1 / 24) * (55 e0 - 59 e1 + 37 e2 - 9 e3)
//   prev = sample_coeff * sample - (coef_eps * eps') / denom
template <int KIND>
__device__ __forceinline__ float plms_combine(float e0, float e1, float e2, float e3) {
  if (KIND == 0) return e0;
  if (KIND == 1) return (e0 + e1) / 2.0f;
  if (KIND == 2) return (3.0f * e0 - e1) / 2.0f;
  if (KIND == 3) return (23.0f * e0 - 16.0f * e1 + 5.0f * e2) / 12.0f;
  return (1.0f / 24.0f) * (55.0f * e0 - 59.0f * e1 + 37.0f * e2 - 9.0f * e3);
}

struct PlmsArgs {
  const float *sample, *e0, *e1, *e2, *e3;
  float *prev;
  float sample_coeff, coef_eps, denom, v_a, v_b;
  int v_prediction;
  int64_t numel;
  unsigned *status;  // device status word (DDPM_STATUS_NONFINITE_EPS) or NULL
};

template <int KIND>
__global__ __launch_bounds__(256) void plms_step_kernel(const PlmsArgs a) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  bool bad = false;  // every tensor of a UNet forward ends in its eps: a non-finite value anywhere inside shows up here
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.numel; i += stride) {
    const float x = a.sample[i];
    const float e0 = a.e0[i];
    bad |= non_finite(e0);
    const float e1 = KIND >= 1 ? a.e1[i] : 0.f;
    const float e2 = KIND >= 3 ? a.e2[i] : 0.f;
    const float e3 = KIND >= 4 ? a.e3[i] : 0.f;
    float eps = plms_combine<KIND>(e0, e1, e2, e3);
    if (a.v_prediction) eps = a.v_a * eps + a.v_b * x;
    a.prev[i] = a.sample_coeff * x - (a.coef_eps * eps) / a.denom;
  }
  if (bad && a.status) atomicOr(a.status, (unsigned)DDPM_STATUS_NONFINITE_EPS);
}

int launch_plms_step(const PlmsArgs &a, int kind, hipStream_t s) {
  DDPM_CHECK_ARG(a.sample && a.e0 && a.prev && a.numel > 0, "plms_step: bad argument");
  DDPM_CHECK_ARG(kind >= 0 && kind <= 4, "plms_step: kind must be 0..4");
  DDPM_CHECK_ARG(kind < 1 || a.e1, "plms_step: e1 missing");
  DDPM_CHECK_ARG(kind < 3 || a.e2, "plms_step: e2 missing");
  DDPM_CHECK_ARG(kind < 4 || a.e3, "plms_step: e3 missing");
  int64_t b = (a.numel + 255) / 256;
  if (b > 4096) b = 4096;
  const dim3 grid((int)b), blk(256);
  const int neps = kind == 0 ? 1 : (kind <= 2 ? 2 : kind);
  ProfScope prof(s, "plms_step", 8.0 * a.numel, 4.0 * a.numel * (2 + neps));
  switch (kind) {
    case 0: hipLaunchKernelGGL(plms_step_kernel<0>, grid, blk, 0, s, a); break;
    case 1: hipLaunchKernelGGL(plms_step_kernel<1>, grid, blk, 0, s, a); break;
    case 2: hipLaunchKernelGGL(plms_step_kernel<2>, grid, blk, 0, s, a); break;
    case 3: hipLaunchKernelGGL(plms_step_kernel<3>, grid, blk, 0, s, a); break;
    default: hipLaunchKernelGGL(plms_step_kernel<4>, grid, blk, 0, s, a); break;
  }
  DDPM_CHECK_LAUNCH();
  return 0;
}

// ---- x / b_scale, clamp(0, 1) in place, per-image mean squared error --------------------------
__global__ __launch_bounds__(256) void clamp_mse_kernel(const float *__restrict__ orig, float *__restrict__ recon,
                                                        float b_scale, float *__restrict__ mse, int64_t chw,
                                                        unsigned *__restrict__ status) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  const float *o = orig + (int64_t)b * chw;
  float *r = recon + (int64_t)b * chw;
  float acc = 0.f;
  bool bad = false;
  for (int64_t i = threadIdx.x; i < chw; i += 256) {
    float v = r[i] / b_scale;
    bad |= non_finite(v);
    v = v != v ? v : fminf(fmaxf(v, 0.f), 1.f);  // torch.clamp_ keeps a NaN (fminf / fmaxf would return the bound)
    r[i] = v;
    const float d = o[i] - v;
    acc += d * d;
  }
  const float tot = block_sum_256(acc, red);
  if (threadIdx.x == 0) mse[b] = tot / (float)chw;
  if (bad && status) atomicOr(status, (unsigned)DDPM_STATUS_NONFINITE_RECON);
}

int launch_clamp_mse(const float *orig, float *recon, float b_scale, float *mse, int B, int64_t chw, hipStream_t s) {
  DDPM_CHECK_ARG(orig && recon && mse && B > 0 && chw > 0 && b_scale != 0.f, "clamp_mse: bad argument");
  ProfScope prof(s, "clamp_mse", 5.0 * B * chw, 12.0 * B * chw);
  hipLaunchKernelGGL(clamp_mse_kernel, dim3(B), dim3(256), 0, s, orig, recon, b_scale, mse, chw, status_word());
  DDPM_CHECK_LAUNCH();
  return 0;
}

// ---- per-pixel squared error, averaged over channels (anomaly maps) ------------------------------
// map[b, s] (+)= weight * (1 / C) * sum_c (a[b, c, s] - b[b, c, s])^2, channels in ascending order.  A thread owns V
// adjacent pixels (V = 4: 16-byte accesses; V = 1: the scalar path), adjacent threads adjacent groups: every channel plane is
// read as one coalesced stream.  Both forms do the same arithmetic per pixel, so their results carry the same bits.
// Bytes per output pixel: 8 C + 4 (+ 4 when accumulating).
template <int V>
__global__ __launch_bounds__(256) void sqerr_map_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                        float *__restrict__ map, int C, int64_t S, int64_t items,
                                                        float weight, int accumulate) {
  struct alignas(4 * V) Vec { float v[V]; };
  const int64_t per_image = S / V;  // groups per image
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const float fc = (float)C;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += stride) {
    const int64_t bi = i / per_image, s = (i - bi * per_image) * V;
    const float *pa = a + bi * C * S + s, *pb = b + bi * C * S + s;
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    for (int c = 0; c < C; ++c) {
      const Vec x = *reinterpret_cast<const Vec *>(pa + (int64_t)c * S);
      const Vec y = *reinterpret_cast<const Vec *>(pb + (int64_t)c * S);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float d = x.v[j] - y.v[j];
        acc[j] += d * d;
      }
    }
    Vec *o = reinterpret_cast<Vec *>(map + bi * S + s);
    Vec r;
    if (accumulate) r = *o;
#pragma unroll
    for (int j = 0; j < V; ++j) r.v[j] = (accumulate ? r.v[j] : 0.f) + weight * (acc[j] / fc);
    *o = r;
  }
}

static bool ranges_overlap(const void *p, double p_bytes, const void *q, double q_bytes) {
  const double a0 = (double)(uintptr_t)p, b0 = (double)(uintptr_t)q;
  return a0 < b0 + q_bytes && b0 < a0 + p_bytes;
}

int launch_sqerr_map(const float *a, const float *b, float *map, int B, int C, int64_t S, float weight, int accumulate,
                     hipStream_t s) {
  DDPM_CHECK_ARG(a && b && map, "sqerr_map: null pointer");
  DDPM_CHECK_ARG(B > 0 && C > 0 && S > 0, "sqerr_map: B, C and S must be positive (got %d, %d, %lld)", B, C, (long long)S);
  DDPM_CHECK_ARG((double)B * C * (double)S < 9.0e18, "sqerr_map: tensor too large");
  const double in_bytes = 4.0 * B * C * (double)S, map_bytes = 4.0 * B * (double)S;
  DDPM_CHECK_ARG(!ranges_overlap(map, map_bytes, a, in_bytes) && !ranges_overlap(map, map_bytes, b, in_bytes),
                 "sqerr_map: map aliases an input");
  const bool vec = (S & 3) == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)map) & 15) == 0;
  const int64_t items = vec ? (int64_t)B * (S / 4) : (int64_t)B * S;
  int64_t blocks = (items + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  ProfScope prof(s, "sqerr_map", 3.0 * B * C * (double)S, 4.0 * B * (double)S * (2 * C + 1 + (accumulate ? 1 : 0)));
  if (vec)
    hipLaunchKernelGGL(sqerr_map_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, s, a, b, map, C, S, items, weight, accumulate);
  else
    hipLaunchKernelGGL(sqerr_map_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, a, b, map, C, S, items, weight, accumulate);
  DDPM_CHECK_LAUNCH();
  return 0;
}

// ---- plain copy (parameter upload into the engine blob) -----------------------------------------
__global__ void copy_kernel(const float *__restrict__ src, float *__restrict__ dst, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = src[i];
}

int launch_copy_f32(const float *src, float *dst, int64_t n, hipStream_t s) {
  if (n <= 0) return 0;
  int64_t b = (n + 255) / 256;
  if (b > 2048) b = 2048;
  hipLaunchKernelGGL(copy_kernel, dim3((int)b), dim3(256), 0, s, src, dst, n);
  DDPM_CHECK_LAUNCH();
  return 0;
}

}  // namespace ddpm

// ---- C ABI ----------------------------------------------------------------------------------------
using namespace ddpm;

namespace ddpm {
int launch_add_noise(const float *, const float *, const float *, const float *, float, float *, int, int64_t,
                     hipStream_t);
}

extern "C" int ddpm_timestep_embedding_f32(const int64_t *t, const float *freqs, float *out, int B, int dim,
                                           ddpm_stream_t stream) {
  return launch_timestep_embedding(t, freqs, out, B, dim, as_stream(stream));
}

extern "C" int ddpm_add_noise_f32(const float *x0, const float *noise, const float *h_sqrt_ac,
                                  const float *h_sqrt_1m_ac, float b_scale, float *out, int B, int64_t chw,
                                  ddpm_stream_t stream) {
  return launch_add_noise(x0, noise, h_sqrt_ac, h_sqrt_1m_ac, b_scale, out, B, chw, as_stream(stream));
}

extern "C" int ddpm_plms_step_f32(const float *sample, const float *e0, const float *e1, const float *e2,
                                  const float *e3, int kind, int v_prediction, float v_a, float v_b,
                                  float sample_coeff, float coef_eps, float denom, float *prev, int64_t numel,
                                  ddpm_stream_t stream) {
  PlmsArgs a{sample, e0, e1, e2, e3, prev, sample_coeff, coef_eps, denom, v_a, v_b, v_prediction, numel, status_word()};
  return launch_plms_step(a, kind, as_stream(stream));
}

extern "C" int ddpm_clamp_mse_f32(const float *orig, float *recon, float b_scale, float *mse, int B, int64_t chw,
                                  ddpm_stream_t stream) {
  return launch_clamp_mse(orig, recon, b_scale, mse, B, chw, as_stream(stream));
}

extern "C" int ddpm_sqerr_map_f32(const float *a, const float *b, float *map, int B, int C, int64_t S, float weight,
                                  int accumulate, ddpm_stream_t stream) {
  return launch_sqerr_map(a, b, map, B, C, S, weight, accumulate, as_stream(stream));
}
