// lpips.hip -- the LPIPS-AlexNet similarity score (second CSV column) on the device.
//
// Replaces lpips.LPIPS(net='alex', version='0.1', lpips=True, spatial=False)(in0, in1, normalize=True) as called by
// PerceptualLoss.forward (/root/reference/src/losses/perceptual_loss.py:105-186; call site
// /root/reference/src/trainers/reconstruct.py:172-187).  Three kernels:
//   lpips_conv_kernel    generic NCHW direct convolution + bias + ReLU for the two AlexNet layers that have no MFMA
//                        tiling here (11x11 stride 4 over 1 or 3 input channels, 5x5 over 64), with the "2x - 1" and
//                        ScalingLayer affine folded into the first layer's input and the 1 -> 3 channel broadcast
//                        done by indexing.  (The three 3x3 layers run on conv_mfma.hip with a ReLU epilogue.)
//   maxpool3s2_kernel    MaxPool2d(3, 2)
//   lpips_layer_kernel   unit-normalise both feature maps over channels, squared difference, 1x1 "lin" weights,
//                        spatial mean, accumulated over the five layers into one score per image pair
// and, only with --anomaly_maps 1 (spatial=True of the package), lpips_layer_map_*_kernel + lpips_map_upsample_kernel below.
// This is 24 MFLOP per 32x32 image pair -- 6e-5 of a reconstruction -- so the kernels are written for clarity and
// coalesced access, not tuned: weights of the block's 4 output channels are wave-uniform (scalar loads), a thread owns
// one output position, adjacent threads adjacent positions.
#include "common.h"

namespace ddpm {

constexpr int kLpCob = 4;  // output channels per thread

__global__ __launch_bounds__(256) void lpips_conv_kernel(const float *__restrict__ in, const float *__restrict__ w,
                                                         const float *__restrict__ bias,
                                                         const float *__restrict__ in_scale,
                                                         const float *__restrict__ in_shift, float *__restrict__ out,
                                                         int N, int Cx, int Cin, int H, int W, int Cout, int Ho, int Wo,
                                                         int k, int stride, int pad, int relu,
                                                         const float *__restrict__ bias_map) {
  const int64_t pos = blockIdx.x * (int64_t)256 + threadIdx.x;  // (n, ho, wo)
  const int co0 = blockIdx.y * kLpCob;
  const int HWo = Ho * Wo;
  if (pos >= (int64_t)N * HWo) return;
  const int n = (int)(pos / HWo), p = (int)(pos - (int64_t)n * HWo);
  const int ho = p / Wo, wo = p - ho * Wo;
  const int h0 = ho * stride - pad, w0 = wo * stride - pad;
  float acc[kLpCob];
#pragma unroll
  for (int j = 0; j < kLpCob; ++j)  // bias_map: a per-position bias [Cout][Ho * Wo] (the folded grey first layer)
    acc[j] = co0 + j >= Cout ? 0.f : bias_map ? bias_map[(size_t)(co0 + j) * HWo + p] : bias ? bias[co0 + j] : 0.f;
  for (int ci = 0; ci < Cin; ++ci) {
    const float *plane = in + ((size_t)n * Cx + (Cx == Cin ? ci : 0)) * H * W;  // 1-channel input feeds all three
    const float a = in_scale ? in_scale[ci] : 1.f, b = in_shift ? in_shift[ci] : 0.f;
    for (int kh = 0; kh < k; ++kh) {
      const int h = h0 + kh;
      if (h < 0 || h >= H) continue;
      for (int kw = 0; kw < k; ++kw) {
        const int x = w0 + kw;
        if (x < 0 || x >= W) continue;
        const float v = plane[h * W + x] * a + b;  // zero padding applies to the scaled input
#pragma unroll
        for (int j = 0; j < kLpCob; ++j)
          if (co0 + j < Cout) acc[j] += v * w[(((size_t)(co0 + j) * Cin + ci) * k + kh) * k + kw];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kLpCob; ++j)
    if (co0 + j < Cout) out[((size_t)n * Cout + co0 + j) * HWo + p] = relu ? relu_f(acc[j]) : acc[j];
}

__global__ __launch_bounds__(256) void maxpool3s2_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                         int64_t planes, int H, int W, int Ho, int Wo) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= planes * Ho * Wo) return;
  const int64_t pl = i / (Ho * Wo);
  const int p = (int)(i - pl * Ho * Wo), ho = p / Wo, wo = p - ho * Wo;
  const float *src = in + pl * H * W + (2 * ho) * W + 2 * wo;
  float m = src[0];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) m = max_keep_nan(m, src[a * W + b]);  // F.max_pool2d keeps a NaN of its window
  out[i] = m;
}

// one workgroup per image pair; threads walk the positions, each looping over the channels (coalesced across threads)
__global__ __launch_bounds__(256) void lpips_layer_kernel(const float *__restrict__ f0, const float *__restrict__ f1,
                                                          const float *__restrict__ lin, float *__restrict__ out, int C,
                                                          int HW, int accumulate) {
  __shared__ float red[4];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float *a = f0 + (size_t)n * C * HW, *b = f1 + (size_t)n * C * HW;
  float acc = 0.f;
  for (int p = tid; p < HW; p += 256) {
    float s0 = 0.f, s1 = 0.f;
    for (int c = 0; c < C; ++c) {
      const float x = a[(size_t)c * HW + p], y = b[(size_t)c * HW + p];
      s0 += x * x;
      s1 += y * y;
    }
    const float r0 = 1.f / (sqrtf(s0) + 1e-10f), r1 = 1.f / (sqrtf(s1) + 1e-10f);
    float d2 = 0.f;
    for (int c = 0; c < C; ++c) {
      const float d = a[(size_t)c * HW + p] * r0 - b[(size_t)c * HW + p] * r1;
      d2 += lin[c] * (d * d);
    }
    acc += d2;
  }
  const float tot = block_sum_256(acc, red) / (float)HW;
  if (tid == 0) out[n] = accumulate ? out[n] + tot : tot;
}

// ---- spatial LPIPS (anomaly maps): the per-position value lpips_layer_kernel averages away ----------------------------------
// maps[n * row_stride + row_offset + p] = sum_c lin[c] (f0[n,c,p] / (|f0[n,:,p]| + 1e-10) - f1[n,c,p] / (|f1[n,:,p]| + 1e-10))^2.
// Two forms, chosen by HW alone (never by N, so a row's bits do not depend on the batch it rides in):
//   lpips_layer_map_pos_kernel    HW > kMapWaveMaxHW: a thread owns one position and walks the channels in ascending order --
//                                 the arithmetic of lpips_layer_kernel's inner loops, coalesced across the threads of a row;
//   lpips_layer_map_wave_kernel   small maps (AlexNet's 3x3 and 1x1 layers at 32^2 .. 64^2 inputs, where a thread per position
//                                 would leave 63 lanes of 64 idle and read with a stride of C): a wave owns one position, lane l
//                                 sums channels l, l + 64, ... in ascending order, the 64 partials meet in wave_sum's fixed
//                                 butterfly.
// Bytes per position: 16 C (both maps twice; the second pass hits L2) + 4.
constexpr int kMapWaveMaxHW = 16;

__global__ __launch_bounds__(256) void lpips_layer_map_pos_kernel(const float *__restrict__ f0, const float *__restrict__ f1,
                                                                  const float *__restrict__ lin, float *__restrict__ maps,
                                                                  int64_t npos, int C, int HW, int64_t row_stride,
                                                                  int64_t row_offset) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;  // (n, p)
  if (i >= npos) return;
  const int64_t n = i / HW;
  const int p = (int)(i - n * HW);
  const float *a = f0 + (size_t)n * C * HW, *b = f1 + (size_t)n * C * HW;
  float s0 = 0.f, s1 = 0.f;
  for (int c = 0; c < C; ++c) {
    const float x = a[(size_t)c * HW + p], y = b[(size_t)c * HW + p];
    s0 += x * x;
    s1 += y * y;
  }
  const float r0 = 1.f / (sqrtf(s0) + 1e-10f), r1 = 1.f / (sqrtf(s1) + 1e-10f);
  float d2 = 0.f;
  for (int c = 0; c < C; ++c) {
    const float d = a[(size_t)c * HW + p] * r0 - b[(size_t)c * HW + p] * r1;
    d2 += lin[c] * (d * d);
  }
  maps[n * row_stride + row_offset + p] = d2;
}

__global__ __launch_bounds__(256) void lpips_layer_map_wave_kernel(const float *__restrict__ f0, const float *__restrict__ f1,
                                                                   const float *__restrict__ lin, float *__restrict__ maps,
                                                                   int64_t npos, int C, int HW, int64_t row_stride,
                                                                   int64_t row_offset) {
  const int lane = threadIdx.x & 63;
  const int64_t i = blockIdx.x * (int64_t)4 + (threadIdx.x >> 6);  // (n, p): one per wave, wave-uniform
  if (i >= npos) return;
  const int64_t n = i / HW;
  const int p = (int)(i - n * HW);
  const float *a = f0 + (size_t)n * C * HW + p, *b = f1 + (size_t)n * C * HW + p;
  float s0 = 0.f, s1 = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float x = a[(size_t)c * HW], y = b[(size_t)c * HW];
    s0 += x * x;
    s1 += y * y;
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  const float r0 = 1.f / (sqrtf(s0) + 1e-10f), r1 = 1.f / (sqrtf(s1) + 1e-10f);
  float d2 = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float d = a[(size_t)c * HW] * r0 - b[(size_t)c * HW] * r1;
    d2 += lin[c] * (d * d);
  }
  d2 = wave_sum(d2);
  if (lane == 0) maps[n * row_stride + row_offset + p] = d2;
}

// out[n, y, x] (+)= weight * sum_k bilinear_k(y + oy, x + ox): every layer's h_k x w_k map of the packed row
// [n, sum_k h_k w_k] resampled to Hfull x Wfull as nn.Upsample(size, mode="bilinear", align_corners=False) does
// (source coordinate max(scale (dst + 0.5) - 0.5, 0) with scale = in / out in fp32; [RECALLED] lpips 0.1.4's spatial=True
// path applies exactly this per layer before summing), layers in ascending k, in ONE launch.  A thread owns one output
// pixel of the H x W window at (oy, ox); the low-resolution maps are a few hundred bytes per image and stay in cache, so
// the traffic is the output: 4 (+ 4 when accumulating) bytes per pixel.
struct LpipsMapLayers {
  int n, h[5], w[5], off[5];
};

__device__ __forceinline__ void bilinear_axis(int dst, int in, float scale, int &i0, int &i1, float &l) {
  const float s = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
  i0 = min((int)s, in - 1);
  i1 = min(i0 + 1, in - 1);
  l = i1 == i0 ? 0.f : s - (float)i0;  // both taps on one sample (a 1-wide map, the far edge): that sample, exactly
}

__global__ __launch_bounds__(256) void lpips_map_upsample_kernel(const float *__restrict__ maps, float *__restrict__ out,
                                                                 const LpipsMapLayers L, int64_t total, int64_t row_stride,
                                                                 int Hfull, int Wfull, int oy, int ox, int H, int W,
                                                                 float weight, int accumulate) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < total; i += stride) {
    const int64_t n = i / ((int64_t)H * W);
    const int r = (int)(i - n * H * W), y = r / W, x = r - y * W;
    const float *row = maps + n * row_stride;
    float acc = 0.f;
    for (int k = 0; k < L.n; ++k) {
      const int h = L.h[k], w = L.w[k];
      int y0, y1, x0, x1;
      float ly, lx;
      bilinear_axis(y + oy, h, (float)h / (float)Hfull, y0, y1, ly);
      bilinear_axis(x + ox, w, (float)w / (float)Wfull, x0, x1, lx);
      const float *m = row + L.off[k];
      const float top = (1.f - lx) * m[y0 * w + x0] + lx * m[y0 * w + x1];
      const float bot = (1.f - lx) * m[y1 * w + x0] + lx * m[y1 * w + x1];
      acc += (1.f - ly) * top + ly * bot;
    }
    out[i] = accumulate ? out[i] + weight * acc : weight * acc;
  }
}

// ---- the LPIPS map of a volume (2.5-D: DESIGN 3.29) ---------------------------------------------------------------------------
// out[n, d, h, w] (+)= weight * the resampled layer sum, at the voxel's in-plane position, of the slice the voxel lies in, for
// the slices taken along `axis` of [N, C, D, H, W] (rows: [N * S, row_stride], volume-major, S the extent along the axis).
// The per-layer expressions and the order of the layer sum are lpips_map_upsample_kernel's, so a voxel carries the bits that
// kernel gives for the same slice.  A wave owns 64 adjacent w of one (n, d) and walks kViewChunk rows h: every store is one
// contiguous run of 64 floats along w, for every axis.  What a voxel's coordinates mean depends on the axis:
//   axis 2   slice d, plane position (h, w): the column pair and weight belong to the lane and are formed once per walk; the row
//            pair changes with h and is the same for the whole wave;
//   axis 3   slice h, plane position (d, w): row and column pairs are both fixed along the walk, the packed row changes with h;
//   axis 4   slice w -- a lane owns a SLICE -- plane position (d, h): the row pair is fixed, the column pair changes with h and
//            is the same for the whole wave.  A layer's four samples stay in registers and are read again only when the column
//            pair moves (once every H / w_k steps; a wave-uniform branch).  The loads are strided by the packed row (a few KB per
//            slice, L2-resident).
// The pairs that change with h are formed ONCE per walk, one (layer, step) per lane (5 layers x 12 steps = 60 lanes), and handed
// to the wave step by step with v_readlane: a thread per voxel that forms both pairs of every layer itself (about 500
// instructions per voxel, most of them index arithmetic) took 29 us at 128^3, this form 21 (profiles/anomaly_volume_maps.md).
constexpr int kViewChunk = 12;  // h positions a wave walks: 5 layers x 12 (layer, step) pairs fit the 64 lanes

__device__ __forceinline__ int view_pick(const int (&v)[5], int k) {  // v[k] without indexing the kernel argument dynamically
  int r = v[0];
#pragma unroll
  for (int j = 1; j < 5; ++j) r = k == j ? v[j] : r;
  return r;
}

template <int AXIS>
__global__ __launch_bounds__(256) void lpips_map_view_kernel(const float *__restrict__ maps, float *__restrict__ out,
                                                             const LpipsMapLayers L, int64_t row_stride, int D, int H, int W,
                                                             int w_tiles, int h_chunks, int64_t jobs, float weight, int accumulate) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  int64_t job = blockIdx.x * (int64_t)4 + wave;  // (n, d, h chunk, w tile): one per wave, wave-uniform
  if (job >= jobs) return;
  const int wt = (int)(job % w_tiles);
  job /= w_tiles;
  const int hc = (int)(job % h_chunks);
  job /= h_chunks;
  const int d = (int)(job % D);
  const int64_t n = job / D;
  const int w = wt * 64 + lane;
  const bool live = w < W;
  const int wc = live ? w : W - 1;  // a dead lane computes its tile's last column and stores nothing
  const int h_begin = hc * kViewChunk, steps = min(kViewChunk, H - h_begin);
  // the pair that changes along the walk, one (layer, step) per lane: rows of the plane (axis 2) or its columns (axis 4)
  int pi0 = 0, pi1 = 0;
  float pl = 0.f;
  if (AXIS != 3) {
    const int k = lane / kViewChunk;
    if (k < L.n) {
      const int ext = AXIS == 2 ? view_pick(L.h, k) : view_pick(L.w, k);
      bilinear_axis(min(h_begin + lane % kViewChunk, H - 1), ext, (float)ext / (float)H, pi0, pi1, pl);
    }
  }
  // what is fixed along the walk: f = the columns of w (axis 2) or the rows of d (axes 3, 4); g = the columns of w (axis 3)
  int f0[5], f1[5], g0[5], g1[5];
  float fl[5], gl[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    f0[k] = f1[k] = g0[k] = g1[k] = 0;
    fl[k] = gl[k] = 0.f;
    if (k < L.n) {
      if (AXIS == 2) bilinear_axis(wc, L.w[k], (float)L.w[k] / (float)W, f0[k], f1[k], fl[k]);
      else bilinear_axis(d, L.h[k], (float)L.h[k] / (float)D, f0[k], f1[k], fl[k]);
      if (AXIS == 3) bilinear_axis(wc, L.w[k], (float)L.w[k] / (float)W, g0[k], g1[k], gl[k]);
    }
  }
  const float *row = maps + (AXIS == 2 ? n * D + d : AXIS == 3 ? n * H : n * W + wc) * row_stride;
  int px0[5], px1[5];
  float m00[5], m01[5], m10[5], m11[5];  // axis 4: the samples held across steps
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    px0[k] = px1[k] = -1;
    m00[k] = m01[k] = m10[k] = m11[k] = 0.f;
  }
  // unrolled over the whole chunk with h clamped: the steps are straight-line code, the loads of several steps can be in flight
  // together, and only the store is guarded
#pragma unroll
  for (int s = 0; s < kViewChunk; ++s) {
    const int h = min(h_begin + s, H - 1);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      if (k < L.n) {
        const int lw = L.w[k];
        int y0, y1, x0, x1;
        float ly, lx;
        if (AXIS == 3) {
          y0 = f0[k], y1 = f1[k], ly = fl[k], x0 = g0[k], x1 = g1[k], lx = gl[k];
        } else {
          const int sel = k * kViewChunk + s;
          const int q0 = __builtin_amdgcn_readlane(pi0, sel), q1 = __builtin_amdgcn_readlane(pi1, sel);
          const float ql = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pl), sel));
          if (AXIS == 2) y0 = q0, y1 = q1, ly = ql, x0 = f0[k], x1 = f1[k], lx = fl[k];
          else y0 = f0[k], y1 = f1[k], ly = fl[k], x0 = q0, x1 = q1, lx = ql;
        }
        const float *m = row + (AXIS == 3 ? (int64_t)h * row_stride : 0) + L.off[k];
        if (AXIS != 4 || x0 != px0[k] || x1 != px1[k]) {
          m00[k] = m[y0 * lw + x0];
          m01[k] = m[y0 * lw + x1];
          m10[k] = m[y1 * lw + x0];
          m11[k] = m[y1 * lw + x1];
          px0[k] = x0;
          px1[k] = x1;
        }
        const float top = (1.f - lx) * m00[k] + lx * m01[k];
        const float bot = (1.f - lx) * m10[k] + lx * m11[k];
        acc += (1.f - ly) * top + ly * bot;
      }
    }
    if (live && s < steps) {
      const int64_t i = ((n * D + d) * H + h) * W + w;
      out[i] = accumulate ? out[i] + weight * acc : weight * acc;
    }
  }
}

// ---- the 5x5 layer on the fp32 MFMA pipe -------------------------------------------------------------------------------
// For 2.5-D LPIPS over 128^3 volumes (cfg5: 128 slices x 3 views x 2 inputs per volume and t-start) the 5x5 layer
// (64 -> 192 over 15 x 15) is 35 GFLOP per call and the scalar kernel above ran it at 9 TFLOP/s -- a quarter of a
// cfg5 step.  Same-padded k x k stride-1 convolution as an implicit GEMM on v_mfma_f32_32x32x2_f32:
//   one workgroup = one image, its whole input (all Cin planes with a zero halo) staged once in LDS (Cin * PS floats,
//   PS = 32 mod 64 so that the two channel planes a wave reads at once sit on disjoint banks);
//   A = weights, packed [cout block of 32][channel pair][tap][lhi][cout]: one coalesced 256-byte load per (pair, tap),
//       held in registers for a whole channel pair and prefetched one pair ahead;
//   B = pixels straight from the LDS planes (lane = pixel of a 32-pixel tile, lhi = channel of the pair);
//   a wave owns one cout block x 4 pixel tiles (4 accumulator tiles); 12 waves = 192 couts x 8 tiles for AlexNet at 128^2.
// Channels are accumulated in ascending order, taps in row-major order inside a channel pair (fp32 MFMA = fmaf chain).
constexpr int kL5Tiles = 4;   // pixel tiles (of 32) per wave
constexpr int kL5Threads = 768;

typedef float l5_f32x16 __attribute__((ext_vector_type(16)));

template <int KS>
__global__ __launch_bounds__(kL5Threads) void lpips_conv_mfma_kernel(const float *__restrict__ in,
                                                                     const float *__restrict__ wp,
                                                                     const float *__restrict__ bias,
                                                                     float *__restrict__ out, int Cin, int H, int W,
                                                                     int Cout, int PS, int relu) {
  extern __shared__ __attribute__((aligned(16))) float l5_smem[];
  constexpr int KK = KS * KS, PAD = KS / 2;
  const int n = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
  const int HW = H * W, WP = W + 2 * PAD;
  for (int i = tid; i < Cin * PS; i += kL5Threads) l5_smem[i] = 0.f;
  __syncthreads();
  const float *src = in + (size_t)n * Cin * HW;
  for (int i = tid; i < Cin * HW; i += kL5Threads) {
    const int c = i / HW, p = i - c * HW;
    const int y = p / W, x = p - y * W;
    l5_smem[c * PS + (y + PAD) * WP + x + PAD] = src[i];
  }
  __syncthreads();
  const int ncb = Cout / 32, nt = (HW + 31) / 32, ngrp = (nt + kL5Tiles - 1) / kL5Tiles, nkk = Cin / 2;
  for (int u = wave; u < ncb * ngrp; u += kL5Threads / 64) {
    const int cb = u % ncb, grp = u / ncb;
    int pb[kL5Tiles];  // LDS float index of this lane's pixel (tap 0, 0) in channel plane lhi
#pragma unroll
    for (int t = 0; t < kL5Tiles; ++t) {
      const int p = min((grp * kL5Tiles + t) * 32 + l31, HW - 1);
      const int y = p / W, x = p - y * W;
      pb[t] = lhi * PS + y * WP + x;
    }
    l5_f32x16 acc[kL5Tiles];
#pragma unroll
    for (int t = 0; t < kL5Tiles; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const float *wq = wp + (size_t)cb * nkk * KK * 64 + lane;
    float a_cur[KK], a_nxt[KK];
#pragma unroll
    for (int tap = 0; tap < KK; ++tap) a_cur[tap] = wq[tap * 64];
    for (int kk = 0; kk < nkk; ++kk) {
      const float *wn = wq + (size_t)min(kk + 1, nkk - 1) * KK * 64;
#pragma unroll
      for (int tap = 0; tap < KK; ++tap) a_nxt[tap] = wn[tap * 64];
      const float *plane = l5_smem + 2 * kk * PS;
#pragma unroll
      for (int tap = 0; tap < KK; ++tap) {
        const int toff = (tap / KS) * WP + tap % KS;
#pragma unroll
        for (int t = 0; t < kL5Tiles; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[tap], plane[pb[t] + toff], acc[t], 0, 0, 0);
      }
#pragma unroll
      for (int tap = 0; tap < KK; ++tap) a_cur[tap] = a_nxt[tap];
    }
    // D: lane = pixel l31, register r = cout 8 (r / 4) + 4 lhi + r % 4 of the block
#pragma unroll
    for (int t = 0; t < kL5Tiles; ++t) {
      const int p = (grp * kL5Tiles + t) * 32 + l31;
      if (p < HW) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = cb * 32 + 8 * (r >> 2) + 4 * lhi + (r & 3);
          const float v = acc[t][r] + (bias ? bias[co] : 0.f);
          out[((size_t)n * Cout + co) * HW + p] = relu ? relu_f(v) : v;
        }
      }
    }
  }
}

// torch [Cout][Cin][k][k] -> [cout block][channel pair][tap][lhi][cout of 32]
__global__ void lpips_pack_conv_kernel(const float *__restrict__ w, float *__restrict__ wp, int Cout, int Cin, int KK) {
  const int64_t total = (int64_t)Cout * Cin * KK;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int tap = (int)(i % KK), ci = (int)((i / KK) % Cin), co = (int)(i / ((int64_t)KK * Cin));
    wp[((((size_t)(co / 32) * (Cin / 2) + ci / 2) * KK + tap) * 2 + (ci & 1)) * 32 + co % 32] = w[i];
  }
}

static int l5_plane(int H, int W, int k) {  // floats per padded channel plane, = 32 mod 64
  const int ps = (H + k - 1) * (W + k - 1);
  return ps + ((32 - ps) % 64 + 64) % 64;
}

bool lpips_conv_mfma_supported(int Cin, int H, int W, int Cout, int k) {
  if (k != 5 && k != 3) return false;
  if (Cin < 2 || Cin % 2 || Cout % 32 || H < 1 || W < 1 || H * W < 64) return false;  // tiny images: the scalar kernel
  return (size_t)Cin * l5_plane(H, W, k) * sizeof(float) <= 160 * 1024;
}

int launch_lpips_pack_conv(const float *w, float *wp, int Cout, int Cin, int k, hipStream_t s) {
  DDPM_CHECK_ARG(w && wp && Cout > 0 && Cout % 32 == 0 && Cin > 0 && Cin % 2 == 0 && k > 0, "lpips pack: bad arguments");
  const int64_t total = (int64_t)Cout * Cin * k * k;
  const int blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
  hipLaunchKernelGGL(lpips_pack_conv_kernel, dim3(blocks), dim3(256), 0, s, w, wp, Cout, Cin, k * k);
  DDPM_CHECK_LAUNCH();
  return 0;
}

int launch_lpips_conv_mfma(const float *in, const float *wp, const float *bias, float *out, int N, int Cin, int H, int W,
                           int Cout, int k, int relu, hipStream_t s) {
  DDPM_CHECK_ARG(in && wp && out && N > 0, "lpips_conv_mfma: null pointer");
  DDPM_CHECK_ARG(lpips_conv_mfma_supported(Cin, H, W, Cout, k), "lpips_conv_mfma: unsupported shape");
  const int PS = l5_plane(H, W, k);
  const size_t lds = (size_t)Cin * PS * sizeof(float);
  typedef void (*kern_t)(const float *, const float *, const float *, float *, int, int, int, int, int, int);
  kern_t kern = k == 5 ? lpips_conv_mfma_kernel<5> : lpips_conv_mfma_kernel<3>;
  static bool attr_done = false;
  if (!attr_done) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(lpips_conv_mfma_kernel<5>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(lpips_conv_mfma_kernel<3>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_done = true;
  }
  const double npos = (double)N * H * W;
  ProfScope prof(s, "lpips_conv_mfma", 2.0 * npos * Cout * Cin * k * k, 4.0 * (npos * Cin + npos * Cout + (double)Cout * Cin * k * k));
  hipLaunchKernelGGL(kern, dim3(N), dim3(kL5Threads), lds, s, in, wp, bias, out, Cin, H, W, Cout, PS, relu);
  DDPM_CHECK_LAUNCH();
  return 0;
}

int launch_lpips_conv(const float *in, const float *w, const float *bias, const float *in_scale, const float *in_shift,
                      float *out, int N, int Cx, int Cin, int H, int W, int Cout, int k, int stride, int pad, int relu,
                      hipStream_t s, const float *bias_map = nullptr) {
  DDPM_CHECK_ARG(in && w && out, "lpips_conv: null pointer");
  DDPM_CHECK_ARG(N > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0 && k > 0 && stride > 0 && pad >= 0, "lpips_conv: bad shape");
  DDPM_CHECK_ARG(Cx == Cin || Cx == 1, "lpips_conv: the input has %d channels, the layer wants %d (or 1, broadcast)", Cx, Cin);
  const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  DDPM_CHECK_ARG(Ho > 0 && Wo > 0, "lpips_conv: image smaller than the kernel");
  const int64_t npos = (int64_t)N * Ho * Wo;
  ProfScope prof(s, "lpips_conv", 2.0 * npos * Cout * Cin * k * k, 4.0 * ((double)N * Cx * H * W + (double)npos * Cout));
  hipLaunchKernelGGL(lpips_conv_kernel, dim3((unsigned)((npos + 255) / 256), (Cout + kLpCob - 1) / kLpCob), dim3(256), 0, s,
                     in, w, bias, in_scale, in_shift, out, N, Cx, Cin, H, W, Cout, Ho, Wo, k, stride, pad, relu, bias_map);
  DDPM_CHECK_LAUNCH();
  return 0;
}

int launch_maxpool3s2(const float *in, float *out, int64_t planes, int H, int W, hipStream_t s) {
  DDPM_CHECK_ARG(in && out && planes > 0 && H >= 3 && W >= 3, "maxpool3s2: bad arguments");
  const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
  const int64_t total = planes * Ho * Wo;
  ProfScope prof(s, "maxpool3s2", 9.0 * total, 4.0 * (planes * (double)H * W + total));
  hipLaunchKernelGGL(maxpool3s2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, out, planes, H, W, Ho, Wo);
  DDPM_CHECK_LAUNCH();
  return 0;
}

int launch_lpips_layer(const float *f0, const float *f1, const float *lin, float *out, int N, int C, int HW,
                       int accumulate, hipStream_t s) {
  DDPM_CHECK_ARG(f0 && f1 && lin && out && N > 0 && C > 0 && HW > 0, "lpips_layer: bad arguments");
  ProfScope prof(s, "lpips_layer", 8.0 * N * C * (double)HW, 16.0 * N * C * (double)HW);
  hipLaunchKernelGGL(lpips_layer_kernel, dim3(N), dim3(256), 0, s, f0, f1, lin, out, C, HW, accumulate);
  DDPM_CHECK_LAUNCH();
  return 0;
}

static bool lp_overlap(const void *p, double p_bytes, const void *q, double q_bytes) {
  const double a0 = (double)(uintptr_t)p, b0 = (double)(uintptr_t)q;
  return a0 < b0 + q_bytes && b0 < a0 + p_bytes;
}

int launch_lpips_layer_map(const float *f0, const float *f1, const float *lin, float *maps, int N, int C, int HW,
                           int64_t row_stride, int64_t row_offset, hipStream_t s) {
  DDPM_CHECK_ARG(f0 && f1 && lin && maps, "lpips_layer_map: null pointer");
  DDPM_CHECK_ARG(N > 0 && C > 0 && HW > 0, "lpips_layer_map: N, C and HW must be positive (got %d, %d, %d)", N, C, HW);
  DDPM_CHECK_ARG(row_offset >= 0 && row_offset + HW <= row_stride,
                 "lpips_layer_map: %d positions at offset %lld do not fit a row of %lld", HW, (long long)row_offset,
                 (long long)row_stride);
  const double fbytes = 4.0 * N * C * (double)HW, mbytes = 4.0 * N * (double)row_stride;
  DDPM_CHECK_ARG(!lp_overlap(maps, mbytes, f0, fbytes) && !lp_overlap(maps, mbytes, f1, fbytes) && !lp_overlap(maps, mbytes, lin, 4.0 * C),
                 "lpips_layer_map: maps aliases an input");
  const int64_t npos = (int64_t)N * HW;
  const bool wave = HW <= kMapWaveMaxHW;
  const int64_t blocks = wave ? (npos + 3) / 4 : (npos + 255) / 256;
  DDPM_CHECK_ARG(blocks <= 0x7fffffff, "lpips_layer_map: too many positions");
  ProfScope prof(s, "lpips_layer_map", 8.0 * npos * C, 16.0 * npos * C + 4.0 * npos);
  if (wave)
    hipLaunchKernelGGL(lpips_layer_map_wave_kernel, dim3((unsigned)blocks), dim3(256), 0, s, f0, f1, lin, maps, npos, C, HW,
                       row_stride, row_offset);
  else
    hipLaunchKernelGGL(lpips_layer_map_pos_kernel, dim3((unsigned)blocks), dim3(256), 0, s, f0, f1, lin, maps, npos, C, HW,
                       row_stride, row_offset);
  DDPM_CHECK_LAUNCH();
  return 0;
}

int launch_lpips_map_upsample(const float *maps, float *out, int N, int64_t row_stride, const LpipsMapLayers &L, int Hfull,
                              int Wfull, int oy, int ox, int H, int W, float weight, int accumulate, hipStream_t s) {
  DDPM_CHECK_ARG(maps && out, "lpips_map_upsample: null pointer");
  DDPM_CHECK_ARG(N > 0 && row_stride > 0, "lpips_map_upsample: N and row_stride must be positive");
  DDPM_CHECK_ARG(L.n >= 1 && L.n <= 5, "lpips_map_upsample: n_layers must be 1 .. 5 (got %d)", L.n);
  for (int k = 0; k < L.n; ++k)
    DDPM_CHECK_ARG(L.h[k] > 0 && L.w[k] > 0 && L.h[k] <= 4096 && L.w[k] <= 4096,
                   "lpips_map_upsample: layer %d has the extent %d x %d", k, L.h[k], L.w[k]);
  DDPM_CHECK_ARG((int64_t)L.off[L.n - 1] + L.h[L.n - 1] * L.w[L.n - 1] <= row_stride,
                 "lpips_map_upsample: the layers do not fit a row of %lld", (long long)row_stride);
  DDPM_CHECK_ARG(Hfull > 0 && Wfull > 0 && H > 0 && W > 0 && oy >= 0 && ox >= 0 && (int64_t)oy + H <= Hfull && (int64_t)ox + W <= Wfull,
                 "lpips_map_upsample: the window %d x %d at (%d, %d) lies outside the full grid %d x %d", H, W, oy, ox, Hfull, Wfull);
  const int64_t total = (int64_t)N * H * W;
  DDPM_CHECK_ARG(!lp_overlap(out, 4.0 * total, maps, 4.0 * N * (double)row_stride), "lpips_map_upsample: out aliases maps");
  int64_t blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  ProfScope prof(s, "lpips_map_upsample", 12.0 * total * L.n, 4.0 * total * (accumulate ? 2 : 1) + 4.0 * N * (double)row_stride);
  hipLaunchKernelGGL(lpips_map_upsample_kernel, dim3((unsigned)blocks), dim3(256), 0, s, maps, out, L, total, row_stride, Hfull,
                     Wfull, oy, ox, H, W, weight, accumulate);
  DDPM_CHECK_LAUNCH();
  return 0;
}

int launch_lpips_map_upsample_view(const float *maps, float *out, int N, int64_t row_stride, const LpipsMapLayers &L, int D, int H,
                                   int W, int axis, float weight, int accumulate, hipStream_t s) {
  DDPM_CHECK_ARG(maps && out, "lpips_map_upsample_view: null pointer");
  DDPM_CHECK_ARG(N > 0 && row_stride > 0, "lpips_map_upsample_view: N and row_stride must be positive");
  DDPM_CHECK_ARG(axis >= 2 && axis <= 4, "lpips_map_upsample_view: axis must be 2, 3 or 4 of [N, C, D, H, W] (got %d)", axis);
  DDPM_CHECK_ARG(L.n >= 1 && L.n <= 5, "lpips_map_upsample_view: n_layers must be 1 .. 5 (got %d)", L.n);
  for (int k = 0; k < L.n; ++k)
    DDPM_CHECK_ARG(L.h[k] > 0 && L.w[k] > 0 && L.h[k] <= 4096 && L.w[k] <= 4096,
                   "lpips_map_upsample_view: layer %d has the extent %d x %d", k, L.h[k], L.w[k]);
  DDPM_CHECK_ARG((int64_t)L.off[L.n - 1] + L.h[L.n - 1] * L.w[L.n - 1] <= row_stride,
                 "lpips_map_upsample_view: the layers do not fit a row of %lld", (long long)row_stride);
  DDPM_CHECK_ARG(D > 0 && H > 0 && W > 0 && D <= (1 << 20) && H <= (1 << 20) && W <= (1 << 20),
                 "lpips_map_upsample_view: extents 1 .. 2^20 (got %d x %d x %d)", D, H, W);
  const double total_d = (double)N * D * (double)H * W;
  DDPM_CHECK_ARG(total_d < 9.0e18, "lpips_map_upsample_view: volume too large");
  const int S = axis == 2 ? D : axis == 3 ? H : W;
  DDPM_CHECK_ARG(!lp_overlap(out, 4.0 * total_d, maps, 4.0 * N * S * (double)row_stride), "lpips_map_upsample_view: out aliases maps");
  ProfScope prof(s, "lpips_map_upsample_view", 12.0 * total_d * L.n, 4.0 * total_d * (accumulate ? 2 : 1) + 4.0 * N * S * (double)row_stride);
  const int w_tiles = (W + 63) / 64, h_chunks = (H + kViewChunk - 1) / kViewChunk;
  const double jobs_d = (double)N * D * (double)h_chunks * w_tiles;
  DDPM_CHECK_ARG(jobs_d < 4.0 * 2147483647.0, "lpips_map_upsample_view: too many tiles");
  const int64_t jobs = (int64_t)N * D * h_chunks * w_tiles;
  const dim3 grid((unsigned)((jobs + 3) / 4));
  if (axis == 2)
    hipLaunchKernelGGL(lpips_map_view_kernel<2>, grid, dim3(256), 0, s, maps, out, L, row_stride, D, H, W, w_tiles, h_chunks, jobs,
                       weight, accumulate);
  else if (axis == 3)
    hipLaunchKernelGGL(lpips_map_view_kernel<3>, grid, dim3(256), 0, s, maps, out, L, row_stride, D, H, W, w_tiles, h_chunks, jobs,
                       weight, accumulate);
  else
    hipLaunchKernelGGL(lpips_map_view_kernel<4>, grid, dim3(256), 0, s, maps, out, L, row_stride, D, H, W, w_tiles, h_chunks, jobs,
                       weight, accumulate);
  DDPM_CHECK_LAUNCH();
  return 0;
}

}  // namespace ddpm

using namespace ddpm;

static LpipsMapLayers lp_packed_layers(int n_layers, int h0, int w0, int h1, int w1, int h2, int w2, int h3, int w3, int h4, int w4) {
  LpipsMapLayers L{n_layers, {h0, h1, h2, h3, h4}, {w0, w1, w2, w3, w4}, {0, 0, 0, 0, 0}};
  // layer k of a row starts where layer k - 1 ends; extents beyond the launcher's limits (which it refuses) count as 0 here
  for (int k = 1; k < 5 && k < n_layers; ++k) {
    const bool ok = L.h[k - 1] > 0 && L.w[k - 1] > 0 && L.h[k - 1] <= 4096 && L.w[k - 1] <= 4096;
    L.off[k] = L.off[k - 1] + (ok ? L.h[k - 1] * L.w[k - 1] : 0);
  }
  return L;
}

extern "C" int ddpm_lpips_map_upsample_view_f32(const float *maps, float *out, int N, int64_t row_stride, int n_layers, int h0,
                                                int w0, int h1, int w1, int h2, int w2, int h3, int w3, int h4, int w4, int D,
                                                int H, int W, int axis, float weight, int accumulate, ddpm_stream_t stream) {
  return launch_lpips_map_upsample_view(maps, out, N, row_stride, lp_packed_layers(n_layers, h0, w0, h1, w1, h2, w2, h3, w3, h4, w4),
                                        D, H, W, axis, weight, accumulate, as_stream(stream));
}

extern "C" int ddpm_lpips_layer_map_f32(const float *f0, const float *f1, const float *lin, float *maps, int N, int C, int HW,
                                        int64_t row_stride, int64_t row_offset, ddpm_stream_t stream) {
  return launch_lpips_layer_map(f0, f1, lin, maps, N, C, HW, row_stride, row_offset, as_stream(stream));
}

extern "C" int ddpm_lpips_map_upsample_f32(const float *maps, float *out, int N, int64_t row_stride, int n_layers, int h0, int w0,
                                           int h1, int w1, int h2, int w2, int h3, int w3, int h4, int w4, int Hfull, int Wfull,
                                           int oy, int ox, int H, int W, float weight, int accumulate, ddpm_stream_t stream) {
  LpipsMapLayers L{n_layers, {h0, h1, h2, h3, h4}, {w0, w1, w2, w3, w4}, {0, 0, 0, 0, 0}};
  // layer k of a row starts where layer k - 1 ends; extents beyond the launcher's limits (which it refuses) count as 0 here
  for (int k = 1; k < 5 && k < n_layers; ++k) {
    const bool ok = L.h[k - 1] > 0 && L.w[k - 1] > 0 && L.h[k - 1] <= 4096 && L.w[k - 1] <= 4096;
    L.off[k] = L.off[k - 1] + (ok ? L.h[k - 1] * L.w[k - 1] : 0);
  }
  return launch_lpips_map_upsample(maps, out, N, row_stride, L, Hfull, Wfull, oy, ox, H, W, weight, accumulate,
                                   as_stream(stream));
}

extern "C" int ddpm_lpips_conv_f32(const float *in, const float *w, const float *bias, const float *in_scale,
                                   const float *in_shift, float *out, int N, int Cx, int Cin, int H, int W, int Cout,
                                   int k, int stride, int pad, int relu, ddpm_stream_t stream) {
  return launch_lpips_conv(in, w, bias, in_scale, in_shift, out, N, Cx, Cin, H, W, Cout, k, stride, pad, relu,
                           as_stream(stream));
}

extern "C" int ddpm_lpips_conv_biasmap_f32(const float *in, const float *w, const float *bias_map, float *out, int N, int Cin,
                                           int H, int W, int Cout, int k, int stride, int pad, int relu, ddpm_stream_t stream) {
  DDPM_CHECK_ARG(bias_map != nullptr, "lpips_conv_biasmap: bias_map is NULL");
  return launch_lpips_conv(in, w, nullptr, nullptr, nullptr, out, N, Cin, Cin, H, W, Cout, k, stride, pad, relu,
                           as_stream(stream), bias_map);
}

extern "C" int ddpm_lpips_conv_mfma_supported(int Cin, int H, int W, int Cout, int k) {
  return lpips_conv_mfma_supported(Cin, H, W, Cout, k) ? 1 : 0;
}

extern "C" int ddpm_lpips_pack_conv_weight_f32(const float *w, float *w_packed, int Cout, int Cin, int k, ddpm_stream_t stream) {
  return launch_lpips_pack_conv(w, w_packed, Cout, Cin, k, as_stream(stream));
}

extern "C" int ddpm_lpips_conv_mfma_f32(const float *in, const float *w_packed, const float *bias, float *out, int N, int Cin,
                                        int H, int W, int Cout, int k, int relu, ddpm_stream_t stream) {
  return launch_lpips_conv_mfma(in, w_packed, bias, out, N, Cin, H, W, Cout, k, relu, as_stream(stream));
}

extern "C" int ddpm_maxpool3s2_f32(const float *in, float *out, int64_t planes, int H, int W, ddpm_stream_t stream) {
  return launch_maxpool3s2(in, out, planes, H, W, as_stream(stream));
}

extern "C" int ddpm_lpips_layer_f32(const float *f0, const float *f1, const float *lin, float *out, int N, int C, int HW,
                                    int accumulate, ddpm_stream_t stream) {
  return launch_lpips_layer(f0, f1, lin, out, N, C, HW, accumulate, as_stream(stream));
}
