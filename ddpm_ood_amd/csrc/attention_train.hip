// attention_train.hip -- attention for the native training step without an N x N tensor.
//
// The op of train_native.py's attention core, o = softmax(scale q^T k) v per head over q, k, v [B, C, N] (channel-major as the
// 1x1 projections write them, head h = channels 256 h .. 256 h + 255), in the flash-attention form: the forward keeps one
// log-sum-exp per row, the backward recomputes the probabilities block by block from q, k and that statistic.  Scores,
// probabilities and dS live in registers only.
//
// Arithmetic: exact fp32 products on v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain; no operand-range condition, unlike the
// split-f16 planes of attention_fa.hip -- the backward's `do` is a scaled gradient nobody bounds).
//   A[m][k]: lane (g = lane / 16, c = lane % 16) holds m = c, k = g;  B[k][n]: k = g, n = c;  D[m][n]: n = c, m = 4 g + r.
//
// One shape of kernel, three times.  A WAVE owns 16 "own" tokens (queries in the forward and in the dq kernel, keys in the
// dk / dv kernel) and walks over the "other" tokens in blocks of 32, which the workgroup stages in LDS as two [256][36] fp32
// images X and Y (row = channel, 36-word rows: the b128 reads below are conflict-free, the b32 reads 2-way):
//   first products, 64 k-steps over d:   T^T[other 16 t + 4 g + r][own c] = sum_d X[d][other] * own_reg[d][own]
//       A = X read as [d = 4 ks + g][other = 16 t + c] (ds_read_b32), B = the wave's own tile in 64 registers
//   second products, 4 k-steps per 16 others:  ACC^T[d = 16 dt + 4 g + r][own c] += sum_other Y[d][other] * W[other][own]
//       A = Y read as [d = 16 dt + c][others 16 t + 4 g .. + 3] (one ds_read_b128 = the four k-steps r), B = W straight from
//       the registers the first product left it in: k-step r of tile t is DEFINED as other = 16 t + 4 g + r.
//   forward:  X = K, Y = V, own = q:        s = scale T, online softmax, o += V p
//   dq:       X = K and V, own = q and do:  p = exp(scale s - lse), ds = p (dp - delta), dq += K ds; delta += sum ds / sum p
//   dk / dv:  X = Q and dO, own = k and v:  the same p and ds (lse, delta of the OTHER tokens), dv += dO p, dk += Q ds
// Every output element has one writer and a fixed summation order (key / query blocks ascending): no atomics, run-to-run
// identical bits.  Registers per lane: forward 64 (q) + 64 (o); dq 128 (q, do) + 64; dk / dv 128 (k, v) + 128 -- four waves per
// workgroup, one wave per SIMD, so each wave may use the whole 512-register file and nothing goes to scratch
// (tests/test_train_attention_host.py checks the assembly).
#include <stdint.h>

#include "common.h"

namespace ddpm {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kD = 256;    // head dim
constexpr int kBlk = 32;   // "other" tokens per staged block
constexpr int kOwn = 16;   // own tokens per wave
constexpr int kNW = 4;     // waves per workgroup
constexpr int kRow = 36;   // words per LDS row
constexpr int kImg = kD * kRow;  // words per staged image

#define AT_MFMA(acc, a, b) (acc) = __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (acc), 0, 0, 0)

// two [256 channels][32 tokens] blocks of [C, N] tensors -> the two LDS images; 16-byte pieces, eight per channel row.  All
// sixteen loads of a thread are issued before the first LDS write: one memory round trip per block, not one per piece.
__device__ __forceinline__ void stage2(const float *__restrict__ src0, float *__restrict__ dst0, const float *__restrict__ src1,
                                       float *__restrict__ dst1, int N, int tid) {
  constexpr int kPer = kD * (kBlk / 4) / (64 * kNW);  // pieces per thread and image (8)
  f32x4 r0[kPer], r1[kPer];
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int u = tid + i * 64 * kNW, d = u >> 3, p = u & 7;
    r0[i] = *reinterpret_cast<const f32x4 *>(src0 + (size_t)d * N + 4 * p);
    r1[i] = *reinterpret_cast<const f32x4 *>(src1 + (size_t)d * N + 4 * p);
  }
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int u = tid + i * 64 * kNW, d = u >> 3, p = u & 7;
    *reinterpret_cast<f32x4 *>(dst0 + d * kRow + 4 * p) = r0[i];
    *reinterpret_cast<f32x4 *>(dst1 + d * kRow + 4 * p) = r1[i];
  }
}

// the wave's own tile as the B operand of the first products: reg[ks] = x[d = 4 ks + g][own c]
__device__ __forceinline__ void load_own(const float *__restrict__ src, float (&reg)[kD / 4], int N, int g, int c) {
#pragma unroll
  for (int ks = 0; ks < kD / 4; ++ks) reg[ks] = src[(size_t)(4 * ks + g) * N + c];
}

// T^T of the two 16-token tiles of a block against one own tile.  The 64 k-steps go round FOUR accumulators per tile, added
// pairwise at the end: an fp32 chain rounds its running sum at every step, and a logit of a few hundred (a per-row offset that
// the softmax removes again) would lose its last bits to 256 roundings at full magnitude -- four chains of 64 steps at a quarter
// of the magnitude keep the score within about one ulp (and no MFMA waits for its predecessor).
__device__ __forceinline__ f32x4 sum4(const f32x4 (&a)[4]) { return (a[0] + a[1]) + (a[2] + a[3]); }

__device__ __forceinline__ void first1(const float *__restrict__ X, const float (&own)[kD / 4], f32x4 (&t)[2], int g, int c) {
  f32x4 a0[4], a1[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) a0[u] = a1[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float *x = X + g * kRow + c;
  // operands through a register ring, read four k-steps (eight MFMAs) ahead: left alone, hipcc emits "read, s_waitcnt
  // lgkmcnt(0), two MFMAs" per k-step and the matrix pipe idles for an LDS round trip 64 times per block
  float xa[8][2];
  auto rd = [&](int ks) {
    xa[ks & 7][0] = x[4 * ks * kRow];
    xa[ks & 7][1] = x[4 * ks * kRow + 16];
  };
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) rd(ks);
  __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
  for (int ks = 0; ks < kD / 4; ++ks) {
    if (ks + 4 < kD / 4) rd(ks + 4);
    AT_MFMA(a0[ks & 3], xa[ks & 7][0], own[ks]);
    AT_MFMA(a1[ks & 3], xa[ks & 7][1], own[ks]);
    if (ks + 4 < kD / 4) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
  }
  t[0] = sum4(a0);
  t[1] = sum4(a1);
}

// two images against two own tiles
__device__ __forceinline__ void first2(const float *__restrict__ X0, const float (&own0)[kD / 4], f32x4 (&t0)[2],
                                       const float *__restrict__ X1, const float (&own1)[kD / 4], f32x4 (&t1)[2], int g, int c) {
  first1(X0, own0, t0, g, c);
  first1(X1, own1, t1, g, c);
}

// ACC^T += Y W over the block's 32 tokens; output tiles in pairs so that no MFMA waits for its predecessor
__device__ __forceinline__ void second(const float *__restrict__ Y, const f32x4 (&w)[2], f32x4 (&acc)[kD / 16], int g, int c) {
  const float *y = Y + c * kRow + 4 * g;
  // sixteen groups (output tile pair dp, token tile t) of two ds_read_b128 and eight MFMAs; the reads run one group ahead
  f32x4 ya[3][2];
  auto rd = [&](int i) {
    ya[i % 3][0] = *reinterpret_cast<const f32x4 *>(y + (32 * (i >> 1)) * kRow + 16 * (i & 1));
    ya[i % 3][1] = *reinterpret_cast<const f32x4 *>(y + (32 * (i >> 1) + 16) * kRow + 16 * (i & 1));
  };
  rd(0);
  __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
  for (int i = 0; i < kD / 16; ++i) {
    const int dp = i >> 1, t = i & 1;
    if (i + 1 < kD / 16) rd(i + 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      AT_MFMA(acc[2 * dp], ya[i % 3][0][r], w[t][r]);
      AT_MFMA(acc[2 * dp + 1], ya[i % 3][1][r], w[t][r]);
    }
    if (i + 1 < kD / 16) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
  }
}

// over the four lanes (c, c + 16, c + 32, c + 48) that hold one own token
__device__ __forceinline__ float quad_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float quad_sum(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

// ACC^T[d = 16 dt + 4 g + r][own c] * f -> a [C, N] tensor
__device__ __forceinline__ void store_acc(float *__restrict__ dst, const f32x4 (&acc)[kD / 16], float f, int N, int g, int c) {
#pragma unroll
  for (int dt = 0; dt < kD / 16; ++dt)
#pragma unroll
    for (int r = 0; r < 4; ++r) dst[(size_t)(16 * dt + 4 * g + r) * N + c] = acc[dt][r] * f;
}

struct Where {
  int tid, lane, wave, g, c, own0;
  size_t head;  // element offset of this (image, head)'s [256, N] slab
  size_t row;   // element offset of its [N] row statistics
};
__device__ __forceinline__ Where where(int C, int N, int heads) {
  Where w;
  w.tid = threadIdx.x;
  w.lane = w.tid & 63;
  w.wave = w.tid >> 6;
  w.g = w.lane >> 4;
  w.c = w.lane & 15;
  w.own0 = ((int)blockIdx.x * kNW + w.wave) * kOwn;
  w.head = ((size_t)blockIdx.z * C + (size_t)blockIdx.y * kD) * N;
  w.row = ((size_t)blockIdx.z * heads + blockIdx.y) * N;
  return w;
}

// ---- forward: o and the row statistic ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kNW) void attn_train_fwd_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                                   const float *__restrict__ v, float *__restrict__ o,
                                                                   float *__restrict__ lse, int C, int N, int heads, float scale) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *const Ks = lds, *const Vs = lds + kImg;
  const Where w = where(C, N, heads);
  const int g = w.g, c = w.c;
  float qr[kD / 4];
  load_own(q + w.head + w.own0, qr, N, g, c);
  f32x4 acc[kD / 16];
#pragma unroll
  for (int dt = 0; dt < kD / 16; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_part = 0.f;  // l_part: this lane's share of the row sum (the four lanes agree on m_run)

  for (int j0 = 0; j0 < N; j0 += kBlk) {
    __syncthreads();  // the previous block's reads are done
    stage2(k + w.head + j0, Ks, v + w.head + j0, Vs, N, w.tid);
    __syncthreads();
    f32x4 s[2];
    first1(Ks, qr, s, g, c);
    float bm = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] *= scale;
        bm = fmaxf(bm, s[t][r]);
      }
    const float mn = fmaxf(m_run, quad_max(bm));
    const float alpha = expf(m_run - mn);  // 0 on the first block
    m_run = mn;
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] = expf(s[t][r] - mn);
        sum += s[t][r];
      }
    l_part = l_part * alpha + sum;
    if (__any(alpha != 1.0f)) {  // a running maximum that did not move leaves the accumulators alone
#pragma unroll
      for (int dt = 0; dt < kD / 16; ++dt) acc[dt] *= alpha;
    }
    second(Vs, s, acc, g, c);
  }
  const float l = quad_sum(l_part);
  store_acc(o + w.head + w.own0, acc, 1.0f / l, N, g, c);
  if (g == 0) lse[w.row + w.own0 + c] = m_run + logf(l);
}

// ---- backward pre-pass: delta[b, h, i] = sum_c do[c, i] o[c, i] ------------------------------------------------------------------
__global__ __launch_bounds__(64) void attn_train_delta_kernel(const float *__restrict__ o, const float *__restrict__ dout,
                                                              float *__restrict__ delta, int C, int N, int heads) {
  const int i = blockIdx.x * 64 + threadIdx.x;  // N is a multiple of 64
  const size_t head = ((size_t)blockIdx.z * C + (size_t)blockIdx.y * kD) * N + i;
  float part[4] = {0.f, 0.f, 0.f, 0.f};  // four interleaved chains, added in a fixed order
  for (int d = 0; d < kD; d += 4)
#pragma unroll
    for (int u = 0; u < 4; ++u) part[u] = fmaf(dout[head + (size_t)(d + u) * N], o[head + (size_t)(d + u) * N], part[u]);
  delta[((size_t)blockIdx.z * heads + blockIdx.y) * N + i] = (part[0] + part[1]) + (part[2] + part[3]);
}

// p and ds of one block from the two first products; rows: the statistics of the token a register belongs to
__device__ __forceinline__ void p_and_ds(f32x4 (&s)[2], f32x4 (&dp)[2], const float (&ls)[2][4], const float (&dl)[2][4], float scale) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = expf(s[t][r] * scale - ls[t][r]);
      s[t][r] = p;
      dp[t][r] = p * (dp[t][r] - dl[t][r]);
    }
}

// ---- backward, query side: dq, and delta made consistent for the key side ---------------------------------------------------------
// sum_j ds_ij is 0 in exact arithmetic (it is why to_k's bias has a zero gradient).  The pre-pass delta comes from o, whose
// rounding is independent of the p and dp recomputed here, so the sum is left at a few 1e-7 of |do| |v| -- several times what the
// GEMM route leaves, which subtracts the row sum of the very products it multiplies.  This kernel sees every ds of its rows: it
// adds them up (and the p) beside the MFMAs and moves delta_i by (sum_j ds_ij) / (sum_j p_ij), a change at rounding level after
// which the key-side kernel -- same chains, same bits of p and dp -- sums to zero over j as the GEMM route does.  In place: a
// row's delta is read and written by the one wave that owns the row.
__global__ __launch_bounds__(64 * kNW) void attn_train_dq_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                                  const float *__restrict__ v, const float *__restrict__ dout,
                                                                  const float *__restrict__ lse, float *__restrict__ delta,
                                                                  float *__restrict__ dq, int C, int N, int heads, float scale) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *const Ks = lds, *const Vs = lds + kImg;
  const Where w = where(C, N, heads);
  const int g = w.g, c = w.c;
  float qr[kD / 4], dor[kD / 4];
  load_own(q + w.head + w.own0, qr, N, g, c);
  load_own(dout + w.head + w.own0, dor, N, g, c);
  float ls[2][4], dl[2][4];  // the own token's statistics, the same for all eight registers
  {
    const float l_own = lse[w.row + w.own0 + c], d_own = delta[w.row + w.own0 + c];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ls[t][r] = l_own;
        dl[t][r] = d_own;
      }
  }
  f32x4 acc[kD / 16];
#pragma unroll
  for (int dt = 0; dt < kD / 16; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  float ds_part = 0.f, p_part = 0.f;  // this lane's share of the row sums of ds and p
  for (int j0 = 0; j0 < N; j0 += kBlk) {
    __syncthreads();
    stage2(k + w.head + j0, Ks, v + w.head + j0, Vs, N, w.tid);
    __syncthreads();
    f32x4 s[2], dp[2];
    first2(Ks, qr, s, Vs, dor, dp, g, c);
    p_and_ds(s, dp, ls, dl, scale);
    ds_part += ((dp[0][0] + dp[0][1]) + (dp[0][2] + dp[0][3])) + ((dp[1][0] + dp[1][1]) + (dp[1][2] + dp[1][3]));
    p_part += ((s[0][0] + s[0][1]) + (s[0][2] + s[0][3])) + ((s[1][0] + s[1][1]) + (s[1][2] + s[1][3]));
    second(Ks, dp, acc, g, c);
  }
  store_acc(dq + w.head + w.own0, acc, scale, N, g, c);
  const float ds_row = quad_sum(ds_part), p_row = quad_sum(p_part);
  if (g == 0) delta[w.row + w.own0 + c] = dl[0][0] + ds_row / p_row;
}

// ---- backward, key side: dk and dv -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kNW) void attn_train_dkv_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                                   const float *__restrict__ v, const float *__restrict__ dout,
                                                                   const float *__restrict__ lse, const float *__restrict__ delta,
                                                                   float *__restrict__ dk, float *__restrict__ dv, int C, int N,
                                                                   int heads, float scale) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *const Qs = lds, *const Ds = lds + kImg;
  const Where w = where(C, N, heads);
  const int g = w.g, c = w.c;
  float kr[kD / 4], vr[kD / 4];
  load_own(k + w.head + w.own0, kr, N, g, c);
  load_own(v + w.head + w.own0, vr, N, g, c);
  f32x4 acck[kD / 16], accv[kD / 16];
#pragma unroll
  for (int dt = 0; dt < kD / 16; ++dt) acck[dt] = accv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int i0 = 0; i0 < N; i0 += kBlk) {
    __syncthreads();
    stage2(q + w.head + i0, Qs, dout + w.head + i0, Ds, N, w.tid);
    __syncthreads();
    float ls[2][4], dl[2][4];  // of queries i0 + 16 t + 4 g + r
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const f32x4 a = *reinterpret_cast<const f32x4 *>(lse + w.row + i0 + 16 * t + 4 * g);
      const f32x4 b = *reinterpret_cast<const f32x4 *>(delta + w.row + i0 + 16 * t + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ls[t][r] = a[r];
        dl[t][r] = b[r];
      }
    }
    f32x4 s[2], dp[2];
    first2(Qs, kr, s, Ds, vr, dp, g, c);
    p_and_ds(s, dp, ls, dl, scale);
    second(Ds, s, accv, g, c);
    second(Qs, dp, acck, g, c);
  }
  store_acc(dv + w.head + w.own0, accv, 1.0f, N, g, c);
  store_acc(dk + w.head + w.own0, acck, scale, N, g, c);
}

constexpr size_t kLdsBytes = (size_t)2 * kImg * sizeof(float);  // 73 728

int check_shape(const char *what, int B, int C, int N, int heads) {
  DDPM_CHECK_ARG(B > 0 && heads > 0, "%s: B and heads must be positive (got %d, %d)", what, B, heads);
  DDPM_CHECK_ARG(C > 0 && (long)C == (long)heads * kD, "%s: C = %d is not heads * 256 = %ld (head dim 256 only)", what, C,
                 (long)heads * kD);
  DDPM_CHECK_ARG(N > 0 && N % 64 == 0, "%s: N = %d is not a positive multiple of 64", what, N);
  DDPM_CHECK_ARG((long long)B * C * N <= 0x7fffffffLL, "%s: B * C * N = %lld overflows 32-bit indexing", what,
                 (long long)B * C * N);
  DDPM_CHECK_ARG(B <= 65535 && heads <= 65535, "%s: B and heads must not exceed 65535", what);
  return 0;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename K>
void want_lds(K kern) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
}

}  // namespace

int launch_attention_train_fwd(const float *q, const float *k, const float *v, float *o, float *lse, int B, int C, int N, int heads,
                               float scale, hipStream_t s) {
  DDPM_CHECK_ARG(q && k && v && o && lse, "attention_train_fwd: null pointer");
  if (int rc = check_shape("attention_train_fwd", B, C, N, heads)) return rc;
  DDPM_CHECK_ARG(aligned16(q) && aligned16(k) && aligned16(v), "attention_train_fwd: q, k and v must be 16-byte aligned");
  static bool once = false;
  if (!once) {
    want_lds(attn_train_fwd_kernel);
    once = true;
  }
  hipLaunchKernelGGL(attn_train_fwd_kernel, dim3(N / (kOwn * kNW), heads, B), dim3(64 * kNW), kLdsBytes, s, q, k, v, o, lse, C, N,
                     heads, scale);
  DDPM_CHECK_LAUNCH();
  return 0;
}

int launch_attention_train_bwd(const float *q, const float *k, const float *v, const float *o, const float *dout, const float *lse,
                               float *delta, float *dq, float *dk, float *dv, int B, int C, int N, int heads, float scale,
                               hipStream_t s) {
  DDPM_CHECK_ARG(q && k && v && o && dout && lse && delta && dq && dk && dv, "attention_train_bwd: null pointer");
  if (int rc = check_shape("attention_train_bwd", B, C, N, heads)) return rc;
  DDPM_CHECK_ARG(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(dout) && aligned16(lse) && aligned16(delta),
                 "attention_train_bwd: q, k, v, do, lse and delta must be 16-byte aligned");
  static bool once = false;
  if (!once) {
    want_lds(attn_train_dq_kernel);
    want_lds(attn_train_dkv_kernel);
    once = true;
  }
  const dim3 grid(N / (kOwn * kNW), heads, B), block(64 * kNW);
  hipLaunchKernelGGL(attn_train_delta_kernel, dim3(N / 64, heads, B), dim3(64), 0, s, o, dout, delta, C, N, heads);
  DDPM_CHECK_LAUNCH();
  hipLaunchKernelGGL(attn_train_dq_kernel, grid, block, kLdsBytes, s, q, k, v, dout, lse, delta, dq, C, N, heads, scale);
  DDPM_CHECK_LAUNCH();
  hipLaunchKernelGGL(attn_train_dkv_kernel, grid, block, kLdsBytes, s, q, k, v, dout, lse, delta, dk, dv, C, N, heads, scale);
  DDPM_CHECK_LAUNCH();
  return 0;
}

}  // namespace ddpm
