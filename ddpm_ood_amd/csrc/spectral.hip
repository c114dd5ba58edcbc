// spectral.hip -- the elementwise half of the Jukebox spectral loss of VQ-VAE training (generative's JukeboxLoss, defaults;
// SURVEY.md A.8):   loss = mean over all elements of (|fftn(recon)| - |fftn(image)|)^2,   ortho-normalised, channel axis inside.
// The transforms themselves are dense per-axis DFTs on ddpm_gemm_f32 (ddpm_ood_amd/loss_terms.py); what is left is one fused
// pass over the two spectra (re / im planes of recon R and image X):
//   spectral_amp_grad_kernel   per workgroup an fp64 partial sum of (|R| - |X|)^2, folded in a fixed order, and / or the
//                              spectrum-side gradient G = scale dloss (|R| - |X|) R / |R|  (scale = 2 / N; G = 0 where |R| = 0 --
//                              autograd gives NaN there)
//   spectral_finalize_kernel   loss[0] = (sum of the partials in a fixed order) / N
// The transform is unitary, so the gradient with respect to recon is the inverse DFT of G, real part.  No atomics: bit-identical
// run to run.
#include "common.h"

namespace ddpm {

constexpr int kSpecMaxBlocks = 1024;

// fixed-order block sum of doubles for blockDim.x == 256: butterfly inside the wave, waves in ascending order
__device__ __forceinline__ double block_sum_256_f64(double v, double *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void spectral_amp_grad_kernel(const float *__restrict__ rr, const float *__restrict__ ri,
                                                                const float *__restrict__ xr, const float *__restrict__ xi,
                                                                const float *__restrict__ dloss, float *__restrict__ gr,
                                                                float *__restrict__ gi, double *__restrict__ partials,
                                                                int64_t n, float scale) {
  __shared__ double red[4];
  const float up = gr ? scale * (dloss ? dloss[0] : 1.f) : 0.f;
  double acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float a = rr[i], b = ri[i], c = xr[i], d = xi[i];
    const float ar = sqrtf(a * a + b * b), ax = sqrtf(c * c + d * d);
    const float diff = ar - ax;
    acc += (double)diff * (double)diff;
    if (gr) {
      const float g = ar > 0.f ? up * diff / ar : 0.f;
      gr[i] = g * a;
      gi[i] = g * b;
    }
  }
  if (partials) {
    const double tot = block_sum_256_f64(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = tot;
  }
}

__global__ __launch_bounds__(256) void spectral_finalize_kernel(const double *__restrict__ partials, int nparts,
                                                                float *__restrict__ loss, double inv_n) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) acc += partials[i];
  const double tot = block_sum_256_f64(acc, red);
  if (threadIdx.x == 0) loss[0] = (float)(tot * inv_n);
}

static int spectral_blocks(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (int)(b > kSpecMaxBlocks ? kSpecMaxBlocks : b);
}

}  // namespace ddpm

using namespace ddpm;

extern "C" size_t ddpm_spectral_partials(int64_t n) { return n > 0 ? (size_t)spectral_blocks(n) : 0; }

extern "C" int ddpm_spectral_amp_grad_f32(const float *rr, const float *ri, const float *xr, const float *xi, const float *dloss,
                                          float *gr, float *gi, float *loss, double *partials, int64_t n, float scale,
                                          ddpm_stream_t stream) {
  DDPM_CHECK_ARG(rr && ri && xr && xi && n > 0, "spectral_amp_grad: null spectrum or empty extent");
  DDPM_CHECK_ARG((gr == nullptr) == (gi == nullptr), "spectral_amp_grad: gr and gi go together");
  DDPM_CHECK_ARG((loss == nullptr) == (partials == nullptr), "spectral_amp_grad: loss needs its partials (ddpm_spectral_partials doubles)");
  DDPM_CHECK_ARG(gr || loss, "spectral_amp_grad: nothing to compute");
  hipStream_t s = as_stream(stream);
  const int blocks = spectral_blocks(n);
  ProfScope prof(s, "spectral_amp_grad", 16.0 * n, 4.0 * n * (gr ? 6 : 4));
  hipLaunchKernelGGL(spectral_amp_grad_kernel, dim3(blocks), dim3(256), 0, s, rr, ri, xr, xi, dloss, gr, gi, partials, n, scale);
  if (loss) hipLaunchKernelGGL(spectral_finalize_kernel, dim3(1), dim3(256), 0, s, partials, blocks, loss, 1.0 / (double)n);
  DDPM_CHECK_LAUNCH();
  return 0;
}
