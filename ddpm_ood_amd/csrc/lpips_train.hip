// lpips_train.hip -- the backward of the LPIPS-AlexNet score with respect to its FIRST input (the reconstruction), for the
// perceptual term of VQ-VAE training (0.001 x LPIPS in the generator loss).  The second input and every LPIPS
// weight are constants.  The forward is lpips.hip's; the input gradients of the four stride-1 layers are the same convolutions
// with rotated, transposed weights (ddpm_conv_f32 / ddpm_lpips_conv_f32 over ddpm_conv_weight_rot180t_f32).  What is left:
//   lpips_layer_backward_kernel   backward of lpips_layer_kernel w.r.t. f0, one upstream scalar per image pair
//   maxpool3s2_backward_kernel    MaxPool2d(3, 2) backward, gather form, PyTorch's tie rule (first maximum in row-major order)
//   lpips_conv1_dgrad_kernel      input gradient of the 11x11 stride-4 pad-2 layer through the folded input affine and the
//                                 1 -> 3 channel broadcast
// The first two write into the gradient of a post-ReLU feature map and fuse that ReLU's mask (f > 0).  Written like lpips.hip:
// a thread owns one position, adjacent threads adjacent positions, every sum in a fixed order, no atomics.
#include "common.h"

namespace ddpm {

// u_c = x_c r0, r0 = 1 / (|x| + eps): dL/dx_k = r0 g_k - (sum_c g_c x_c) r0^2 x_k / |x| with g_c = (2 up / HW) lin_c (u_c - v_c).
// |x| = 0: the second term is taken as 0 (autograd's sqrt backward gives NaN there).
__global__ __launch_bounds__(256) void lpips_layer_backward_kernel(const float *__restrict__ f0, const float *__restrict__ f1,
                                                                   const float *__restrict__ lin, const float *__restrict__ up,
                                                                   float *__restrict__ df0, int C, int HW, int accumulate,
                                                                   int relu_mask) {
  const int n = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const float *a = f0 + (size_t)n * C * HW + p, *b = f1 + (size_t)n * C * HW + p;
  float *d = df0 + (size_t)n * C * HW + p;
  float s0 = 0.f, s1 = 0.f;
  for (int c = 0; c < C; ++c) {
    const float x = a[(size_t)c * HW], y = b[(size_t)c * HW];
    s0 += x * x;
    s1 += y * y;
  }
  const float n0 = sqrtf(s0);
  const float r0 = 1.f / (n0 + 1e-10f), r1 = 1.f / (sqrtf(s1) + 1e-10f);
  const float k = 2.f * up[n] / (float)HW;
  float dot = 0.f;
  for (int c = 0; c < C; ++c) {
    const float x = a[(size_t)c * HW];
    dot += k * lin[c] * (x * r0 - b[(size_t)c * HW] * r1) * x;
  }
  const float coef = n0 > 0.f ? dot * r0 * r0 / n0 : 0.f;
  for (int c = 0; c < C; ++c) {
    const float x = a[(size_t)c * HW];
    const float g = k * lin[c] * (x * r0 - b[(size_t)c * HW] * r1);
    const float own = r0 * g - coef * x;
    const float v = (accumulate ? d[(size_t)c * HW] : 0.f) + own;
    d[(size_t)c * HW] = relu_mask && !(x > 0.f) ? 0.f : v;
  }
}

// dx[h, w] (+)= sum of dy over the <= 4 windows that cover (h, w) and whose first maximum (row-major scan, strict >) it is
__global__ __launch_bounds__(256) void maxpool3s2_backward_kernel(const float *__restrict__ x, const float *__restrict__ dy,
                                                                  float *__restrict__ dx, int64_t planes, int H, int W, int Ho,
                                                                  int Wo, int accumulate, int relu_mask) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= planes * H * W) return;
  const int64_t pl = i / (H * W);
  const int p = (int)(i - pl * H * W), h = p / W, w = p - h * W;
  const float *src = x + pl * H * W;
  const float *g = dy + pl * Ho * Wo;
  float acc = 0.f;
  const int ho_lo = h >= 2 ? (h - 1) / 2 : 0, ho_hi = min(h / 2, Ho - 1);
  const int wo_lo = w >= 2 ? (w - 1) / 2 : 0, wo_hi = min(w / 2, Wo - 1);
  for (int ho = ho_lo; ho <= ho_hi; ++ho) {
    if (h - 2 * ho > 2) continue;  // a last row / column that no window reaches
    for (int wo = wo_lo; wo <= wo_hi; ++wo) {
      if (w - 2 * wo > 2) continue;
      const float *win = src + (2 * ho) * W + 2 * wo;
      float m = win[0];
      int arg = 0;
#pragma unroll
      for (int t = 1; t < 9; ++t) {
        const float v = win[(t / 3) * W + t % 3];
        if (v > m) {
          m = v;
          arg = t;
        }
      }
      if (arg == (h - 2 * ho) * 3 + (w - 2 * wo)) acc += g[ho * Wo + wo];
    }
  }
  const float v = (accumulate ? dx[i] : 0.f) + acc;
  dx[i] = relu_mask && !(src[p] > 0.f) ? 0.f : v;
}

// y[co, ho, wo] = sum_ci sum_taps w[co, ci, kh, kw] (a_ci x[cx(ci), s ho - pad + kh, s wo - pad + kw] + b_ci):
// dx[cx, h, w] = sum over the ci that read plane cx of a_ci sum_co sum_{ho, wo: taps inside the kernel} w[co, ci, kh, kw] g[co, ho, wo]
constexpr int kC1Cin = 3;

__global__ __launch_bounds__(256) void lpips_conv1_dgrad_kernel(const float *__restrict__ g, const float *__restrict__ w,
                                                                const float *__restrict__ in_scale, float *__restrict__ dx,
                                                                int N, int Cx, int H, int W, int Cout, int Ho, int Wo, int k,
                                                                int stride, int pad) {
  const int64_t pos = blockIdx.x * (int64_t)256 + threadIdx.x;  // (n, h, w)
  if (pos >= (int64_t)N * H * W) return;
  const int n = (int)(pos / (H * W)), p = (int)(pos - (int64_t)n * H * W);
  const int h = p / W, x = p - h * W;
  // windows whose tap kh = h + pad - stride ho lies in [0, k)
  const int hn = h + pad - (k - 1), wn = x + pad - (k - 1);
  const int ho_lo = hn > 0 ? (hn + stride - 1) / stride : 0, ho_hi = min((h + pad) / stride, Ho - 1);
  const int wo_lo = wn > 0 ? (wn + stride - 1) / stride : 0, wo_hi = min((x + pad) / stride, Wo - 1);
  float acc[kC1Cin] = {0.f, 0.f, 0.f};
  for (int co = 0; co < Cout; ++co) {
    const float *gp = g + ((size_t)n * Cout + co) * Ho * Wo;
    const float *wp = w + (size_t)co * kC1Cin * k * k;
    for (int ho = ho_lo; ho <= ho_hi; ++ho) {
      const int kh = h + pad - stride * ho;
      for (int wo = wo_lo; wo <= wo_hi; ++wo) {
        const int kw = x + pad - stride * wo;
        const float gv = gp[ho * Wo + wo];
#pragma unroll
        for (int ci = 0; ci < kC1Cin; ++ci) acc[ci] += gv * wp[(ci * k + kh) * k + kw];
      }
    }
  }
#pragma unroll
  for (int ci = 0; ci < kC1Cin; ++ci) acc[ci] *= in_scale ? in_scale[ci] : 1.f;
  if (Cx == 1) {
    dx[pos] = (acc[0] + acc[1]) + acc[2];
  } else {
#pragma unroll
    for (int ci = 0; ci < kC1Cin; ++ci) dx[((size_t)n * kC1Cin + ci) * H * W + p] = acc[ci];
  }
}

}  // namespace ddpm

using namespace ddpm;

extern "C" int ddpm_lpips_layer_backward_f32(const float *f0, const float *f1, const float *lin, const float *upstream,
                                             float *df0, int N, int C, int HW, int accumulate, int relu_mask,
                                             ddpm_stream_t stream) {
  DDPM_CHECK_ARG(f0 && f1 && lin && upstream && df0, "lpips_layer_backward: null pointer");
  DDPM_CHECK_ARG(N > 0 && N <= 65535 && C > 0 && HW > 0, "lpips_layer_backward: bad shape (N %d, C %d, HW %d)", N, C, HW);
  hipStream_t s = as_stream(stream);
  ProfScope prof(s, "lpips_layer_backward", 14.0 * N * C * (double)HW, 28.0 * N * C * (double)HW);
  hipLaunchKernelGGL(lpips_layer_backward_kernel, dim3((HW + 255) / 256, N), dim3(256), 0, s, f0, f1, lin, upstream, df0, C, HW,
                     accumulate, relu_mask);
  DDPM_CHECK_LAUNCH();
  return 0;
}

extern "C" int ddpm_maxpool3s2_backward_f32(const float *x, const float *dy, float *dx, int64_t planes, int H, int W,
                                            int accumulate, int relu_mask, ddpm_stream_t stream) {
  DDPM_CHECK_ARG(x && dy && dx && planes > 0 && H >= 3 && W >= 3, "maxpool3s2_backward: bad arguments");
  const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
  const int64_t total = planes * H * W;
  DDPM_CHECK_ARG((total + 255) / 256 <= 0x7fffffffLL, "maxpool3s2_backward: too many positions");
  hipStream_t s = as_stream(stream);
  ProfScope prof(s, "maxpool3s2_backward", 40.0 * total, 4.0 * (3.0 * total + (double)planes * Ho * Wo));
  hipLaunchKernelGGL(maxpool3s2_backward_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, dy, dx, planes, H, W,
                     Ho, Wo, accumulate, relu_mask);
  DDPM_CHECK_LAUNCH();
  return 0;
}

extern "C" int ddpm_lpips_conv1_dgrad_f32(const float *g, const float *w, const float *in_scale, float *dx, int N, int Cx,
                                          int Cin, int H, int W, int Cout, int k, int stride, int pad, ddpm_stream_t stream) {
  DDPM_CHECK_ARG(g && w && dx, "lpips_conv1_dgrad: null pointer");
  DDPM_CHECK_ARG(Cin == kC1Cin && (Cx == 1 || Cx == Cin), "lpips_conv1_dgrad: the layer reads %d channels from 1 or %d planes",
                 kC1Cin, kC1Cin);
  DDPM_CHECK_ARG(N > 0 && Cout > 0 && H > 0 && W > 0 && k > 0 && stride > 0 && pad >= 0, "lpips_conv1_dgrad: bad shape");
  const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  DDPM_CHECK_ARG(H + 2 * pad >= k && W + 2 * pad >= k && Ho > 0 && Wo > 0, "lpips_conv1_dgrad: image smaller than the kernel");
  const int64_t npos = (int64_t)N * H * W;
  DDPM_CHECK_ARG((npos + 255) / 256 <= 0x7fffffffLL, "lpips_conv1_dgrad: too many positions");
  hipStream_t s = as_stream(stream);
  ProfScope prof(s, "lpips_conv1_dgrad", 2.0 * N * Ho * Wo * (double)Cout * Cin * k * k,
                 4.0 * ((double)N * Cout * Ho * Wo + (double)npos * Cx));
  hipLaunchKernelGGL(lpips_conv1_dgrad_kernel, dim3((unsigned)((npos + 255) / 256)), dim3(256), 0, s, g, w, in_scale, dx, N, Cx,
                     H, W, Cout, Ho, Wo, k, stride, pad);
  DDPM_CHECK_LAUNCH();
  return 0;
}
