// likelihood.hip -- the DDPM variational bound of an image (DiffusionInferer.get_likelihood): the noising and
// the per-timestep term of the bound, each as ONE launch over ROWS.  A row is one (image, timestep) pair: row r reads image
// row_src[r] of x0 / noise ([N, row_numel], never replicated) and entry row_t[r] of the coefficient table
//   coef[t] = { sqrt(abar_t), sqrt(1 - abar_t), c0, ct, 0.5 / var, inv_s = var^-1/2, 0, 0 }      (fp32, rounded from float64)
// so that any (image, timestep) pairs share a UNet forward -- the T terms of the bound do not depend on each other.
//
//   x_t   = sa x0 + sb n                                                       (ddpm_vlb_noise_rows_f32)
//   x0hat = (x_t - sb out) / sa | sa x_t - sb out | out;  clamp(-1, 1) if clip_sample
//   t > 0:  kl = (0.5 / var) (c0 (x0 - x0hat))^2        post_mean - pred_mean: the ct x_t of the two means cancel exactly
//   t = 0:  d = x0 - (c0 x0hat + ct x_t),  Phi(z) = 0.5 (1 + tanh(sqrt(2 / pi) (z + 0.044715 z^3)))
//           cp = Phi(inv_s (d + bin / 2)),  cm = Phi(inv_s (d - bin / 2))
//           kl = -log max(cp, 1e-12) where x0 < -0.999 | -log max(1 - cm, 1e-12) where x0 > 0.999 | -log max(cp - cm, 1e-12)
//   term[r] = mean over the row of kl                                          (ddpm_vlb_term_rows_f32)
//
// One workgroup per row: every thread adds its elements (strided by 256, in a double) and block_sum_256 adds the 256 partial
// sums in a fixed tree, so term[r] is a pure function of the row's own data and coefficients -- not of R, of the row's place in
// the launch or of the other rows.  No atomics but the status word's.  12 B per element (x0 mostly from cache: the rows of one
// image share it), 16 B with kl_map: microseconds beside the forward they follow; what counts is ONE launch per forward.
#include "common.h"

namespace ddpm {
namespace {

constexpr int kCoefStride = 8;

inline bool vlb_vec4_ok(int64_t row_numel, std::initializer_list<const void *> ptrs) {
  if (row_numel & 3) return false;
  for (const void *p : ptrs)
    if (p && (reinterpret_cast<uintptr_t>(p) & 15)) return false;
  return true;
}

__device__ __forceinline__ void load4(const float *p, int64_t j0, int cnt, bool vec, float (&v)[4]) {
  if (vec) {
    const float4 q = *reinterpret_cast<const float4 *>(p + j0);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < cnt ? p[j0 + j] : 0.f;
  }
}

__device__ __forceinline__ void store4(float *p, int64_t j0, int cnt, bool vec, const float (&v)[4]) {
  if (vec) {
    *reinterpret_cast<float4 *>(p + j0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) p[j0 + j] = v[j];
  }
}

// rows over blockIdx.y (strided), the quads of a row over blockIdx.x (grid-stride)
template <bool VEC>
__global__ __launch_bounds__(256) void vlb_noise_rows_kernel(const float *__restrict__ x0, const float *__restrict__ noise,
                                                             const int *__restrict__ row_src, const int *__restrict__ row_t,
                                                             const float *__restrict__ coef, int T, float *__restrict__ x_t,
                                                             int R, int64_t row_numel) {
  const int64_t quads = (row_numel + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int r = blockIdx.y; r < R; r += gridDim.y) {
    const int t = row_t[r];
    if (t < 0 || t >= T) continue;  // (the host checks the ranges; a bad entry must not read outside the table)
    const float sa = coef[t * kCoefStride + 0], sb = coef[t * kCoefStride + 1];
    const int64_t in = (int64_t)row_src[r] * row_numel, out = (int64_t)r * row_numel;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < quads; q += stride) {
      const int64_t j0 = q << 2;
      const int cnt = VEC ? 4 : (int)(row_numel - j0 < 4 ? row_numel - j0 : 4);
      float a[4], n[4], y[4];
      load4(x0 + in, j0, cnt, VEC, a);
      load4(noise + in, j0, cnt, VEC, n);
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = sa * a[j] + sb * n[j];  // two products and one sum, each rounded (-ffp-contract=off)
      store4(x_t + out, j0, cnt, VEC, y);
    }
  }
}

struct TermArgs {
  const float *x0, *x_t, *out_model;
  const int *row_src, *row_t;
  const float *coef;
  float *term, *kl_map;  // kl_map may be NULL
  int T, clip, R;
  float half_bin;
  int64_t row_numel;
  unsigned *status;
};

template <int PT>
__device__ __forceinline__ float vlb_x0hat(float x, float o, float sa, float sb) {
  if (PT == DDPM_PREDICTION_EPSILON) return (x - sb * o) / sa;
  if (PT == DDPM_PREDICTION_V) return sa * x - sb * o;
  return o;
}

__device__ __forceinline__ float approx_cdf(float z) {
  return 0.5f * (1.0f + tanhf(0.7978845608028654f * (z + 0.044715f * (z * z * z))));
}

// one workgroup per row
template <int PT, bool VEC>
__global__ __launch_bounds__(256) void vlb_term_rows_kernel(const TermArgs a) {
  __shared__ float red[4];
  const int r = blockIdx.x;
  const int t = a.row_t[r];
  if (t < 0 || t >= a.T) {  // uniform over the workgroup; the host checks the ranges
    if (threadIdx.x == 0) a.term[r] = __builtin_nanf("");
    return;
  }
  const float *c = a.coef + t * kCoefStride;
  const float sa = c[0], sb = c[1], c0 = c[2], ct = c[3], half_inv_var = c[4], inv_s = c[5];
  const int64_t in = (int64_t)a.row_src[r] * a.row_numel, base = (int64_t)r * a.row_numel;
  const int64_t quads = (a.row_numel + 3) >> 2;
  const bool decoder = t == 0;
  bool bad = false;
  double acc = 0.0;
  for (int64_t q = threadIdx.x; q < quads; q += 256) {
    const int64_t j0 = q << 2;
    const int cnt = VEC ? 4 : (int)(a.row_numel - j0 < 4 ? a.row_numel - j0 : 4);
    float x0[4], xt[4], o[4], kl[4];
    load4(a.x0 + in, j0, cnt, VEC, x0);
    load4(a.x_t + base, j0, cnt, VEC, xt);
    load4(a.out_model + base, j0, cnt, VEC, o);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bad |= non_finite(o[j]);
      float p = vlb_x0hat<PT>(xt[j], o[j], sa, sb);
      if (a.clip) p = p != p ? p : fminf(fmaxf(p, -1.f), 1.f);  // torch.clamp keeps a NaN
      if (!decoder) {
        const float dm = c0 * (x0[j] - p);
        kl[j] = half_inv_var * (dm * dm);
      } else {
        const float d = x0[j] - (c0 * p + ct * xt[j]);
        const float cp = approx_cdf(inv_s * (d + a.half_bin)), cm = approx_cdf(inv_s * (d - a.half_bin));
        const float pr = x0[j] < -0.999f ? cp : (x0[j] > 0.999f ? 1.0f - cm : cp - cm);
        kl[j] = -logf(pr != pr ? pr : fmaxf(pr, 1e-12f));  // clamp(min=) keeps a NaN as well
      }
      if (j < cnt) acc += (double)kl[j];
    }
    if (a.kl_map) store4(a.kl_map + base, j0, cnt, VEC, kl);
  }
  const float sum = block_sum_256((float)acc, red);
  if (threadIdx.x == 0) a.term[r] = sum / (float)a.row_numel;
  if (bad && a.status) atomicOr(a.status, (unsigned)DDPM_STATUS_NONFINITE_EPS);
}

template <int PT>
void launch_term(const TermArgs &a, bool vec, hipStream_t s) {
  const dim3 grid((unsigned)a.R), blk(256);
  if (vec)
    hipLaunchKernelGGL((vlb_term_rows_kernel<PT, true>), grid, blk, 0, s, a);
  else
    hipLaunchKernelGGL((vlb_term_rows_kernel<PT, false>), grid, blk, 0, s, a);
}

}  // namespace
}  // namespace ddpm

using namespace ddpm;

extern "C" int ddpm_vlb_noise_rows_f32(const float *x0, const float *noise, const int *row_src, const int *row_t,
                                       const float *coef, int T, float *x_t, int R, int64_t row_numel, ddpm_stream_t stream) {
  DDPM_CHECK_ARG(x0 && noise && row_src && row_t && coef && x_t && T > 0 && R > 0 && row_numel > 0,
                 "vlb_noise_rows: bad argument");
  DDPM_CHECK_ARG(x_t != x0 && x_t != noise, "vlb_noise_rows: x_t aliases an input");
  hipStream_t s = as_stream(stream);
  int64_t gx = (((row_numel + 3) >> 2) + 255) / 256;
  if (gx > 1024) gx = 1024;
  int64_t gy = 4096 / gx;
  if (gy < 1) gy = 1;
  if (gy > R) gy = R;
  const dim3 grid((unsigned)gx, (unsigned)gy), blk(256);
  const double n = (double)R * (double)row_numel;
  ProfScope prof(s, "vlb_noise_rows", 3.0 * n, 12.0 * n);
  if (vlb_vec4_ok(row_numel, {x0, noise, x_t}))
    hipLaunchKernelGGL(vlb_noise_rows_kernel<true>, grid, blk, 0, s, x0, noise, row_src, row_t, coef, T, x_t, R, row_numel);
  else
    hipLaunchKernelGGL(vlb_noise_rows_kernel<false>, grid, blk, 0, s, x0, noise, row_src, row_t, coef, T, x_t, R, row_numel);
  DDPM_CHECK_LAUNCH();
  return 0;
}

extern "C" int ddpm_vlb_term_rows_f32(const float *x0, const float *x_t, const float *model_output, const int *row_src,
                                      const int *row_t, const float *coef, int T, int prediction_type, int clip_sample,
                                      float bin_width, float *term, float *kl_map, int R, int64_t row_numel,
                                      ddpm_stream_t stream) {
  DDPM_CHECK_ARG(x0 && x_t && model_output && row_src && row_t && coef && term && T > 0 && R > 0 && row_numel > 0,
                 "vlb_term_rows: bad argument");
  DDPM_CHECK_ARG(prediction_type >= DDPM_PREDICTION_EPSILON && prediction_type <= DDPM_PREDICTION_SAMPLE,
                 "vlb_term_rows: prediction_type must be 0 (epsilon), 1 (v_prediction) or 2 (sample)");
  DDPM_CHECK_ARG(bin_width > 0.f, "vlb_term_rows: bin_width must be positive");
  DDPM_CHECK_ARG(kl_map != x0 && kl_map != x_t && kl_map != model_output, "vlb_term_rows: kl_map aliases an input");
  hipStream_t s = as_stream(stream);
  TermArgs a{x0, x_t, model_output, row_src, row_t, coef, term, kl_map, T, clip_sample, R, 0.5f * bin_width, row_numel,
             status_word()};
  const bool vec = vlb_vec4_ok(row_numel, {x0, x_t, model_output, kl_map});
  const double n = (double)R * (double)row_numel;
  ProfScope prof(s, "vlb_term_rows", 12.0 * n, (kl_map ? 16.0 : 12.0) * n);
  switch (prediction_type) {
    case DDPM_PREDICTION_EPSILON: launch_term<DDPM_PREDICTION_EPSILON>(a, vec, s); break;
    case DDPM_PREDICTION_V: launch_term<DDPM_PREDICTION_V>(a, vec, s); break;
    default: launch_term<DDPM_PREDICTION_SAMPLE>(a, vec, s); break;
  }
  DDPM_CHECK_LAUNCH();
  return 0;
}
