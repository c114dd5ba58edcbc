// sampling.hip -- drawing samples from a trained model: the DDPM ancestral reverse step as ONE launch per step, and the
// row-addressed normals it adds.
//
//   x0   = (x - sqrt(1 - abar_t) out) / sqrt(abar_t)        epsilon
//        = sqrt(abar_t) x - sqrt(1 - abar_t) out            v_prediction
//        = out                                              sample
//   x0   = clamp(x0, -1, 1)                                 if clip_sample
//   mean = c0 x0 + ct x
//   prev = mean + sigma z                                   (sigma = 0 on the last step: no noise is drawn)
//
// The five scalars come from the host (DDPMScheduler.step).  z is generated in the kernel: element j of row b is value j % 4 of
// Philox counter (j / 4, row_streams[b]) under key `seed` (philox_normal4, common.h -- the generator of ddpm_randn_f32), so a row
// is a function of (seed, its stream id) alone: not of the batch it rides in, its position in it, or the rank that runs it.
// Elementwise and memory-bound: 8 B read + 4 B written per element (+ 4 B for pred_original when asked for); the ~150 VALU
// instructions of one Philox counter + two Box-Muller pairs per float4 hide under the loads at a chip-filling size, and at the
// batches sampling uses (2 ... 8 rows) the launch is latency: what counts is that it is ONE launch.
#include "common.h"

namespace ddpm {
namespace {

struct AncestralArgs {
  const float *x, *out_model;
  float *prev, *pred;  // pred may be NULL
  const uint64_t *streams;
  float sa, sb, c0, ct, sigma;
  int prediction_type, clip;
  int B;
  int64_t row_numel;
  uint64_t seed;
  unsigned *status;
};

template <int PT>
__device__ __forceinline__ float ancestral_x0(float x, float o, float sa, float sb) {
  if (PT == DDPM_PREDICTION_EPSILON) return (x - sb * o) / sa;
  if (PT == DDPM_PREDICTION_V) return sa * x - sb * o;
  return o;
}

// one row per blockIdx.y (strided), one Philox counter = four consecutive elements of the row per thread (grid-stride).
// VEC: row_numel % 4 == 0 and 16-byte aligned bases, so every quad of every row is one float4.
template <int PT, bool VEC>
__global__ __launch_bounds__(256) void ancestral_step_kernel(const AncestralArgs a) {
  const int64_t quads = (a.row_numel + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool noisy = a.sigma != 0.f;
  bool bad = false;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const uint64_t st = noisy ? a.streams[b] : 0;
    const int64_t base = (int64_t)b * a.row_numel;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < quads; q += stride) {
      const int64_t j0 = q << 2;
      float x[4], o[4], z[4] = {0.f, 0.f, 0.f, 0.f}, p0[4], pr[4];
      const int cnt = VEC ? 4 : (int)(a.row_numel - j0 < 4 ? a.row_numel - j0 : 4);
      if (VEC) {
        const float4 xv = *reinterpret_cast<const float4 *>(a.x + base + j0);
        const float4 ov = *reinterpret_cast<const float4 *>(a.out_model + base + j0);
        x[0] = xv.x, x[1] = xv.y, x[2] = xv.z, x[3] = xv.w;
        o[0] = ov.x, o[1] = ov.y, o[2] = ov.z, o[3] = ov.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          x[j] = j < cnt ? a.x[base + j0 + j] : 0.f;
          o[j] = j < cnt ? a.out_model[base + j0 + j] : 0.f;
        }
      }
      if (noisy) philox_normal4(q, st, a.seed, z);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bad |= non_finite(o[j]);
        float x0 = ancestral_x0<PT>(x[j], o[j], a.sa, a.sb);
        if (a.clip) x0 = x0 != x0 ? x0 : fminf(fmaxf(x0, -1.f), 1.f);  // torch.clamp keeps a NaN
        const float mean = a.c0 * x0 + a.ct * x[j];
        p0[j] = x0;
        pr[j] = noisy ? mean + a.sigma * z[j] : mean;
      }
      if (VEC) {
        *reinterpret_cast<float4 *>(a.prev + base + j0) = make_float4(pr[0], pr[1], pr[2], pr[3]);
        if (a.pred) *reinterpret_cast<float4 *>(a.pred + base + j0) = make_float4(p0[0], p0[1], p0[2], p0[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < cnt) {
            a.prev[base + j0 + j] = pr[j];
            if (a.pred) a.pred[base + j0 + j] = p0[j];
          }
      }
    }
  }
  if (bad && a.status) atomicOr(a.status, (unsigned)DDPM_STATUS_NONFINITE_EPS);
}

template <bool VEC>
__global__ __launch_bounds__(256) void randn_rows_kernel(float *out, int B, int64_t row_numel, uint64_t seed,
                                                         const uint64_t *__restrict__ streams) {
  const int64_t quads = (row_numel + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const uint64_t st = streams[b];
    float *row = out + (int64_t)b * row_numel;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < quads; q += stride) {
      float z[4];
      philox_normal4(q, st, seed, z);
      if (VEC) {
        *reinterpret_cast<float4 *>(row + (q << 2)) = make_float4(z[0], z[1], z[2], z[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if ((q << 2) + j < row_numel) row[(q << 2) + j] = z[j];
      }
    }
  }
}

inline bool rows_vec4_ok(int64_t row_numel, std::initializer_list<const void *> ptrs) {
  if (row_numel & 3) return false;
  for (const void *p : ptrs)
    if (p && (reinterpret_cast<uintptr_t>(p) & 15)) return false;
  return true;
}

// blocks over the quads of one row (x) and rows (y): at most ~4 096 workgroups, the rest is strided over
inline dim3 rows_grid(int B, int64_t row_numel) {
  int64_t gx = (((row_numel + 3) >> 2) + 255) / 256;
  if (gx > 1024) gx = 1024;
  int64_t gy = 4096 / gx;
  if (gy < 1) gy = 1;
  if (gy > B) gy = B;
  return dim3((unsigned)gx, (unsigned)gy);
}

template <int PT>
void launch_ancestral(const AncestralArgs &a, bool vec, hipStream_t s) {
  const dim3 grid = rows_grid(a.B, a.row_numel), blk(256);
  if (vec)
    hipLaunchKernelGGL((ancestral_step_kernel<PT, true>), grid, blk, 0, s, a);
  else
    hipLaunchKernelGGL((ancestral_step_kernel<PT, false>), grid, blk, 0, s, a);
}

}  // namespace
}  // namespace ddpm

using namespace ddpm;

extern "C" int ddpm_ancestral_step_f32(const float *sample, const float *model_output, float *prev, float *pred_original, int B,
                                       int64_t row_numel, int prediction_type, int clip_sample, float sqrt_ac, float sqrt_1m_ac,
                                       float c0, float ct, float sigma, uint64_t seed, const uint64_t *row_streams,
                                       ddpm_stream_t stream) {
  DDPM_CHECK_ARG(sample && model_output && prev && B > 0 && row_numel > 0, "ancestral_step: bad argument");
  DDPM_CHECK_ARG(prediction_type >= DDPM_PREDICTION_EPSILON && prediction_type <= DDPM_PREDICTION_SAMPLE,
                 "ancestral_step: prediction_type must be 0 (epsilon), 1 (v_prediction) or 2 (sample)");
  DDPM_CHECK_ARG(sigma == 0.f || row_streams, "ancestral_step: row_streams missing (sigma != 0)");
  DDPM_CHECK_ARG(prediction_type != DDPM_PREDICTION_EPSILON || sqrt_ac != 0.f, "ancestral_step: sqrt(alphas_cumprod) is 0");
  DDPM_CHECK_ARG(pred_original != prev, "ancestral_step: pred_original aliases prev");
  hipStream_t s = as_stream(stream);
  AncestralArgs a{sample, model_output, prev, pred_original, row_streams, sqrt_ac, sqrt_1m_ac, c0, ct, sigma,
                  prediction_type, clip_sample, B, row_numel, seed, status_word()};
  const bool vec = rows_vec4_ok(row_numel, {sample, model_output, prev, pred_original});
  const double n = (double)B * (double)row_numel;
  ProfScope prof(s, "ancestral_step", 8.0 * n, (pred_original ? 16.0 : 12.0) * n);
  switch (prediction_type) {
    case DDPM_PREDICTION_EPSILON: launch_ancestral<DDPM_PREDICTION_EPSILON>(a, vec, s); break;
    case DDPM_PREDICTION_V: launch_ancestral<DDPM_PREDICTION_V>(a, vec, s); break;
    default: launch_ancestral<DDPM_PREDICTION_SAMPLE>(a, vec, s); break;
  }
  DDPM_CHECK_LAUNCH();
  return 0;
}

extern "C" int ddpm_randn_rows_f32(float *out, int B, int64_t row_numel, uint64_t seed, const uint64_t *row_streams,
                                   ddpm_stream_t stream) {
  DDPM_CHECK_ARG(out && row_streams && B > 0 && row_numel > 0, "randn_rows: bad argument");
  hipStream_t s = as_stream(stream);
  const dim3 grid = rows_grid(B, row_numel), blk(256);
  if (rows_vec4_ok(row_numel, {out}))
    hipLaunchKernelGGL(randn_rows_kernel<true>, grid, blk, 0, s, out, B, row_numel, seed, row_streams);
  else
    hipLaunchKernelGGL(randn_rows_kernel<false>, grid, blk, 0, s, out, B, row_numel, seed, row_streams);
  DDPM_CHECK_LAUNCH();
  return 0;
}
