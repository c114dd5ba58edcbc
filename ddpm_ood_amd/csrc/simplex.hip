// simplex.hip -- fractal simplex noise of AnoDDPM (Wyatt et al., CVPR-W 2022), the --simplex_noise alternative to Gaussian noise
// in training and reconstruction (reference: src/utils/simplex_noise.py, generate_simplex_noise with its defaults
// octave = 6, persistence = 0.8, frequency = 64; call sites ddpm_trainer.py:93-96, :153-156 and reconstruct.py:133-141).
//
// One 2-D slice per (row, channel): sum over octaves k of amplitude_k * noise3(x / f_k, y / f_k, T / f_k) on the pixel grid,
// f_0 = frequency, f_{k+1} = f_k / 2, amplitude_0 = 1, amplitude_{k+1} = amplitude_k * persistence, T = the row's timestep.
// noise3 is OpenSimplex 3-D as published in 2014 (Kurt Spencer's "OpenSimplexNoise", public domain): stretch -1/6, squish 1/3,
// 24 gradients, contribution (2 - |d|^2)^4 (g . d), normaliser 103, permutation tables seeded by a 64-bit LCG.  It evaluates
// a region-specific vertex list (which lattice points contribute depends on the tetrahedron / octahedron the point falls in and
// on score comparisons inside it), so the branches below are part of the definition: a "sum every vertex in range" form differs
// from it.  Everything is fp64 in the published order of operations (the build passes -ffp-contract=off), cast to fp32 once.
//
// Work: one workgroup per slice.  The permutation tables are built in LDS: one lane walks the LCG (cheap 64-bit mul-adds), every
// lane then takes one floored 64-bit modulus in parallel, and one lane does the 256 dependent swaps.  The lanes then evaluate the
// slice's pixels and write them to every depth plane (3-D inputs repeat the 2-D slice along D, as the reference does).
#include "common.h"

namespace ddpm {

namespace {

constexpr double kStretch3 = -1.0 / 6;
constexpr double kSquish3 = 1.0 / 3;
constexpr double kNorm3 = 103;
constexpr uint64_t kLcgMul = 6364136223846793005ull;
constexpr uint64_t kLcgAdd = 1442695040888963407ull;

// the 24 gradients (x, y, z): the vertices of a rhombicuboctahedron, skewed
__constant__ int kGrad3[72] = {
    -11, 4,  4,   -4, 11,  4,   -4, 4,  11,   //
    11,  4,  4,   4,  11,  4,   4,  4,  11,   //
    -11, -4, 4,   -4, -11, 4,   -4, -4, 11,   //
    11,  -4, 4,   4,  -11, 4,   4,  -4, 11,   //
    -11, 4,  -4,  -4, 11,  -4,  -4, 4,  -11,  //
    11,  4,  -4,  4,  11,  -4,  4,  4,  -11,  //
    -11, -4, -4,  -4, -11, -4,  -4, -4, -11,  //
    11,  -4, -4,  4,  -11, -4,  4,  -4, -11};

__host__ __device__ inline uint64_t lcg_next(uint64_t s) { return s * kLcgMul + kLcgAdd; }

// (state + 31) mod n, floored, with state read as a signed 64-bit value and the sum taken without wrapping
__host__ __device__ inline int perm_pick(uint64_t state, int n) {
  int64_t m = (int64_t)state % n;
  if (m < 0) m += n;
  return (int)((m + 31) % n);
}

// The tables of one slice, serially: perm[i] and gidx[i] = (perm[i] % 24) * 3.  The kernel runs the same steps spread over a
// workgroup; this form is what a host check calls.
__host__ __device__ inline void simplex_tables(int64_t seed, int *perm, int *gidx) {
  int source[256];
  for (int i = 0; i < 256; ++i) source[i] = i;
  uint64_t s = (uint64_t)seed;
  for (int k = 0; k < 3; ++k) s = lcg_next(s);
  for (int i = 255; i >= 0; --i) {
    s = lcg_next(s);
    const int r = perm_pick(s, i + 1);
    perm[i] = source[r];
    gidx[i] = (perm[i] % 24) * 3;
    source[r] = source[i];
  }
}

struct Lattice {
  const int *perm, *gidx, *grad;
  // one vertex's term: (2 - |d|^2)^4 times the gradient's dot product with d, if the vertex is in range
  __host__ __device__ inline void add(double &value, int xv, int yv, int zv, double dx, double dy, double dz) const {
    double attn = 2 - dx * dx - dy * dy - dz * dz;
    if (attn > 0) {
      const int g = gidx[(perm[(perm[xv & 0xFF] + yv) & 0xFF] + zv) & 0xFF];
      attn *= attn;
      value += attn * attn * (grad[g] * dx + grad[g + 1] * dy + grad[g + 2] * dz);
    }
  }
};

__host__ __device__ inline double opensimplex3(const Lattice &L, double x, double y, double z) {
  // onto the simplectic honeycomb: the rhombohedral super-cell's origin and the point's position inside it
  const double stretch = (x + y + z) * kStretch3;
  const double xs = x + stretch, ys = y + stretch, zs = z + stretch;
  const int xsb = (int)floor(xs), ysb = (int)floor(ys), zsb = (int)floor(zs);
  const double squish = (xsb + ysb + zsb) * kSquish3;
  const double xins = xs - xsb, yins = ys - ysb, zins = zs - zsb;
  const double in_sum = xins + yins + zins;
  const double dx0 = x - (xsb + squish), dy0 = y - (ysb + squish), dz0 = z - (zsb + squish);

  // the two extra vertices that may contribute, chosen per region
  int xv0, yv0, zv0, xv1, yv1, zv1;
  double dxe0, dye0, dze0, dxe1, dye1, dze1;
  double value = 0;

  if (in_sum <= 1) {
    // tetrahedron at (0,0,0): the closest two of (1,0,0), (0,1,0), (0,0,1)
    int ap = 1, bp = 2;
    double as = xins, bs = yins;
    if (as >= bs && zins > bs) {
      bs = zins;
      bp = 4;
    } else if (as < bs && zins > as) {
      as = zins;
      ap = 4;
    }
    const double wins = 1 - in_sum;
    if (wins > as || wins > bs) {  // (0,0,0) is one of the closest two
      const int c = bs > as ? bp : ap;
      if (c & 1) {
        xv0 = xv1 = xsb + 1;
        dxe0 = dxe1 = dx0 - 1;
      } else {
        xv0 = xsb - 1;
        xv1 = xsb;
        dxe0 = dx0 + 1;
        dxe1 = dx0;
      }
      if (c & 2) {
        yv0 = yv1 = ysb + 1;
        dye0 = dye1 = dy0 - 1;
      } else {
        yv0 = yv1 = ysb;
        dye0 = dye1 = dy0;
        if (c & 1) {
          yv0 -= 1;
          dye0 += 1;
        } else {
          yv1 -= 1;
          dye1 += 1;
        }
      }
      if (c & 4) {
        zv0 = zv1 = zsb + 1;
        dze0 = dze1 = dz0 - 1;
      } else {
        zv0 = zsb;
        zv1 = zsb - 1;
        dze0 = dz0;
        dze1 = dz0 + 1;
      }
    } else {  // the extra vertices follow from the closest two
      const int c = ap | bp;
      if (c & 1) {
        xv0 = xv1 = xsb + 1;
        dxe0 = dx0 - 1 - 2 * kSquish3;
        dxe1 = dx0 - 1 - kSquish3;
      } else {
        xv0 = xsb;
        xv1 = xsb - 1;
        dxe0 = dx0 - 2 * kSquish3;
        dxe1 = dx0 + 1 - kSquish3;
      }
      if (c & 2) {
        yv0 = yv1 = ysb + 1;
        dye0 = dy0 - 1 - 2 * kSquish3;
        dye1 = dy0 - 1 - kSquish3;
      } else {
        yv0 = ysb;
        yv1 = ysb - 1;
        dye0 = dy0 - 2 * kSquish3;
        dye1 = dy0 + 1 - kSquish3;
      }
      if (c & 4) {
        zv0 = zv1 = zsb + 1;
        dze0 = dz0 - 1 - 2 * kSquish3;
        dze1 = dz0 - 1 - kSquish3;
      } else {
        zv0 = zsb;
        zv1 = zsb - 1;
        dze0 = dz0 - 2 * kSquish3;
        dze1 = dz0 + 1 - kSquish3;
      }
    }
    const double dx1 = dx0 - 1 - kSquish3, dy1 = dy0 - 0 - kSquish3, dz1 = dz0 - 0 - kSquish3;
    const double dx2 = dx0 - 0 - kSquish3, dy2 = dy0 - 1 - kSquish3;
    const double dz3 = dz0 - 1 - kSquish3;
    L.add(value, xsb, ysb, zsb, dx0, dy0, dz0);
    L.add(value, xsb + 1, ysb, zsb, dx1, dy1, dz1);
    L.add(value, xsb, ysb + 1, zsb, dx2, dy2, dz1);
    L.add(value, xsb, ysb, zsb + 1, dx2, dy1, dz3);
  } else if (in_sum >= 2) {
    // tetrahedron at (1,1,1): the closest two of (1,1,0), (1,0,1), (0,1,1)
    int ap = 6, bp = 5;
    double as = xins, bs = yins;
    if (as <= bs && zins < bs) {
      bs = zins;
      bp = 3;
    } else if (as > bs && zins < as) {
      as = zins;
      ap = 3;
    }
    const double wins = 3 - in_sum;
    if (wins < as || wins < bs) {  // (1,1,1) is one of the closest two
      const int c = bs < as ? bp : ap;
      if (c & 1) {
        xv0 = xsb + 2;
        xv1 = xsb + 1;
        dxe0 = dx0 - 2 - 3 * kSquish3;
        dxe1 = dx0 - 1 - 3 * kSquish3;
      } else {
        xv0 = xv1 = xsb;
        dxe0 = dxe1 = dx0 - 3 * kSquish3;
      }
      if (c & 2) {
        yv0 = yv1 = ysb + 1;
        dye0 = dye1 = dy0 - 1 - 3 * kSquish3;
        if (c & 1) {
          yv1 += 1;
          dye1 -= 1;
        } else {
          yv0 += 1;
          dye0 -= 1;
        }
      } else {
        yv0 = yv1 = ysb;
        dye0 = dye1 = dy0 - 3 * kSquish3;
      }
      if (c & 4) {
        zv0 = zsb + 1;
        zv1 = zsb + 2;
        dze0 = dz0 - 1 - 3 * kSquish3;
        dze1 = dz0 - 2 - 3 * kSquish3;
      } else {
        zv0 = zv1 = zsb;
        dze0 = dze1 = dz0 - 3 * kSquish3;
      }
    } else {  // the extra vertices follow from the closest two
      const int c = ap & bp;
      if (c & 1) {
        xv0 = xsb + 1;
        xv1 = xsb + 2;
        dxe0 = dx0 - 1 - kSquish3;
        dxe1 = dx0 - 2 - 2 * kSquish3;
      } else {
        xv0 = xv1 = xsb;
        dxe0 = dx0 - kSquish3;
        dxe1 = dx0 - 2 * kSquish3;
      }
      if (c & 2) {
        yv0 = ysb + 1;
        yv1 = ysb + 2;
        dye0 = dy0 - 1 - kSquish3;
        dye1 = dy0 - 2 - 2 * kSquish3;
      } else {
        yv0 = yv1 = ysb;
        dye0 = dy0 - kSquish3;
        dye1 = dy0 - 2 * kSquish3;
      }
      if (c & 4) {
        zv0 = zsb + 1;
        zv1 = zsb + 2;
        dze0 = dz0 - 1 - kSquish3;
        dze1 = dz0 - 2 - 2 * kSquish3;
      } else {
        zv0 = zv1 = zsb;
        dze0 = dz0 - kSquish3;
        dze1 = dz0 - 2 * kSquish3;
      }
    }
    const double dx3 = dx0 - 1 - 2 * kSquish3, dy3 = dy0 - 1 - 2 * kSquish3, dz3 = dz0 - 0 - 2 * kSquish3;
    const double dy2 = dy0 - 0 - 2 * kSquish3, dz2 = dz0 - 1 - 2 * kSquish3;
    const double dx1 = dx0 - 0 - 2 * kSquish3;
    L.add(value, xsb + 1, ysb + 1, zsb, dx3, dy3, dz3);
    L.add(value, xsb + 1, ysb, zsb + 1, dx3, dy2, dz2);
    L.add(value, xsb, ysb + 1, zsb + 1, dx1, dy3, dz2);
    L.add(value, xsb + 1, ysb + 1, zsb + 1, dx0 - 1 - 3 * kSquish3, dy0 - 1 - 3 * kSquish3, dz0 - 1 - 3 * kSquish3);
  } else {
    // octahedron between the two tetrahedra: the closest two of its six vertices, each on the (0,0,0) or the (1,1,1) side
    double as, bs;
    int ap, bp;
    bool a_far, b_far;
    const double p1 = xins + yins;  // (0,0,1) against (1,1,0)
    if (p1 > 1) {
      as = p1 - 1;
      ap = 3;
      a_far = true;
    } else {
      as = 1 - p1;
      ap = 4;
      a_far = false;
    }
    const double p2 = xins + zins;  // (0,1,0) against (1,0,1)
    if (p2 > 1) {
      bs = p2 - 1;
      bp = 5;
      b_far = true;
    } else {
      bs = 1 - p2;
      bp = 2;
      b_far = false;
    }
    const double p3 = yins + zins;  // the closer of (1,0,0) and (0,1,1) replaces the farther of the two above, if closer still
    const bool p3_far = p3 > 1;
    const double score = p3_far ? p3 - 1 : 1 - p3;
    if (as <= bs && as < score) {
      ap = p3_far ? 6 : 1;
      a_far = p3_far;
    } else if (as > bs && bs < score) {
      bp = p3_far ? 6 : 1;
      b_far = p3_far;
    }
    if (a_far == b_far) {
      if (a_far) {  // both on the (1,1,1) side: (1,1,1) and a vertex along the shared axis
        xv0 = xsb + 1;
        yv0 = ysb + 1;
        zv0 = zsb + 1;
        dxe0 = dx0 - 1 - 3 * kSquish3;
        dye0 = dy0 - 1 - 3 * kSquish3;
        dze0 = dz0 - 1 - 3 * kSquish3;
        const int c = ap & bp;
        xv1 = xsb;
        yv1 = ysb;
        zv1 = zsb;
        dxe1 = dx0 - 2 * kSquish3;
        dye1 = dy0 - 2 * kSquish3;
        dze1 = dz0 - 2 * kSquish3;
        if (c & 1) {
          xv1 = xsb + 2;
          dxe1 = dx0 - 2 - 2 * kSquish3;
        } else if (c & 2) {
          yv1 = ysb + 2;
          dye1 = dy0 - 2 - 2 * kSquish3;
        } else {
          zv1 = zsb + 2;
          dze1 = dz0 - 2 - 2 * kSquish3;
        }
      } else {  // both on the (0,0,0) side: (0,0,0) and a vertex off the omitted axis
        xv0 = xsb;
        yv0 = ysb;
        zv0 = zsb;
        dxe0 = dx0;
        dye0 = dy0;
        dze0 = dz0;
        const int c = ap | bp;
        xv1 = xsb + 1;
        yv1 = ysb + 1;
        zv1 = zsb + 1;
        dxe1 = dx0 - 1 - kSquish3;
        dye1 = dy0 - 1 - kSquish3;
        dze1 = dz0 - 1 - kSquish3;
        if (!(c & 1)) {
          xv1 = xsb - 1;
          dxe1 = dx0 + 1 - kSquish3;
        } else if (!(c & 2)) {
          yv1 = ysb - 1;
          dye1 = dy0 + 1 - kSquish3;
        } else {
          zv1 = zsb - 1;
          dze1 = dz0 + 1 - kSquish3;
        }
      }
    } else {  // one on each side: a permutation of (1,1,-1) and one of (0,0,2)
      const int c1 = a_far ? ap : bp, c2 = a_far ? bp : ap;
      xv0 = xsb + 1;
      yv0 = ysb + 1;
      zv0 = zsb + 1;
      dxe0 = dx0 - 1 - kSquish3;
      dye0 = dy0 - 1 - kSquish3;
      dze0 = dz0 - 1 - kSquish3;
      if (!(c1 & 1)) {
        xv0 = xsb - 1;
        dxe0 = dx0 + 1 - kSquish3;
      } else if (!(c1 & 2)) {
        yv0 = ysb - 1;
        dye0 = dy0 + 1 - kSquish3;
      } else {
        zv0 = zsb - 1;
        dze0 = dz0 + 1 - kSquish3;
      }
      xv1 = xsb;
      yv1 = ysb;
      zv1 = zsb;
      dxe1 = dx0 - 2 * kSquish3;
      dye1 = dy0 - 2 * kSquish3;
      dze1 = dz0 - 2 * kSquish3;
      if (c2 & 1) {
        xv1 += 2;
        dxe1 -= 2;
      } else if (c2 & 2) {
        yv1 += 2;
        dye1 -= 2;
      } else {
        zv1 += 2;
        dze1 -= 2;
      }
    }
    const double dx1 = dx0 - 1 - kSquish3, dy1 = dy0 - 0 - kSquish3, dz1 = dz0 - 0 - kSquish3;
    const double dx2 = dx0 - 0 - kSquish3, dy2 = dy0 - 1 - kSquish3;
    const double dz3 = dz0 - 1 - kSquish3;
    const double dx4 = dx0 - 1 - 2 * kSquish3, dy4 = dy0 - 1 - 2 * kSquish3, dz4 = dz0 - 0 - 2 * kSquish3;
    const double dy5 = dy0 - 0 - 2 * kSquish3, dz5 = dz0 - 1 - 2 * kSquish3;
    const double dx6 = dx0 - 0 - 2 * kSquish3;
    L.add(value, xsb + 1, ysb, zsb, dx1, dy1, dz1);
    L.add(value, xsb, ysb + 1, zsb, dx2, dy2, dz1);
    L.add(value, xsb, ysb, zsb + 1, dx2, dy1, dz3);
    L.add(value, xsb + 1, ysb + 1, zsb, dx4, dy4, dz4);
    L.add(value, xsb + 1, ysb, zsb + 1, dx4, dy5, dz5);
    L.add(value, xsb, ysb + 1, zsb + 1, dx6, dy4, dz5);
  }
  L.add(value, xv0, yv0, zv0, dxe0, dye0, dze0);
  L.add(value, xv1, yv1, zv1, dxe1, dye1, dze1);
  return value / kNorm3;
}

// the fractal sum of one pixel (float64, octave by octave)
__host__ __device__ inline double simplex_octaves(const Lattice &L, int x, int y, int64_t t, int octaves, double persistence,
                                                  double frequency) {
  double acc = 0, amplitude = 1, f = frequency;
  for (int k = 0; k < octaves; ++k) {
    acc += amplitude * opensimplex3(L, x / f, y / f, (double)t / f);
    f /= 2;
    amplitude *= persistence;
  }
  return acc;
}

__global__ __launch_bounds__(256) void simplex_noise_kernel(float *__restrict__ out, const int64_t *__restrict__ seeds,
                                                            const int64_t *__restrict__ tsteps, int channels, int depth, int H,
                                                            int W, int octaves, double persistence, double frequency) {
  __shared__ uint64_t state[256];
  __shared__ int source[256], pick[256], perm[256], gidx[256], grad[72];
  const int slice = blockIdx.x, tid = threadIdx.x;  // slice = row * channels + channel
  if (tid < 72) grad[tid] = kGrad3[tid];
  source[tid] = tid;
  if (tid == 0) {  // state[i] = the LCG after 3 + (256 - i) steps: the draw of table position i
    uint64_t s = (uint64_t)seeds[slice];
    for (int k = 0; k < 3; ++k) s = lcg_next(s);
    for (int i = 255; i >= 0; --i) {
      s = lcg_next(s);
      state[i] = s;
    }
  }
  __syncthreads();
  pick[tid] = perm_pick(state[tid], tid + 1);
  __syncthreads();
  if (tid == 0) {
    for (int i = 255; i >= 0; --i) {
      const int r = pick[i];
      const int p = source[r];
      perm[i] = p;
      source[r] = source[i];
    }
  }
  __syncthreads();
  gidx[tid] = (perm[tid] % 24) * 3;
  __syncthreads();

  const Lattice L{perm, gidx, grad};
  const int64_t t = tsteps[slice / channels];
  const int HW = H * W;
  float *dst = out + (int64_t)slice * depth * HW;
  for (int p = tid; p < HW; p += blockDim.x) {
    const int y = p / W, x = p - y * W;
    const float v = (float)simplex_octaves(L, x, y, t, octaves, persistence, frequency);
    for (int d = 0; d < depth; ++d) dst[(int64_t)d * HW + p] = v;
  }
}

}  // namespace

}  // namespace ddpm

using namespace ddpm;

extern "C" int ddpm_simplex_noise_f32(float *out, const int64_t *seeds, const int64_t *t, int64_t rows, int channels, int depth,
                                      int H, int W, int octaves, double persistence, double frequency, ddpm_stream_t stream) {
  DDPM_CHECK_ARG(out && seeds && t, "simplex_noise: NULL pointer");
  DDPM_CHECK_ARG(rows > 0 && channels > 0 && depth > 0 && H > 0 && W > 0, "simplex_noise: bad shape");
  DDPM_CHECK_ARG(rows * channels <= 0x7fffffff && (int64_t)H * W <= 0x7fffffff, "simplex_noise: %lld slices of %d x %d too large",
                 (long long)(rows * channels), H, W);
  DDPM_CHECK_ARG(octaves >= 1 && octaves <= 64 && frequency > 0 && persistence == persistence,
                 "simplex_noise: bad octave parameters (%d, %g, %g)", octaves, persistence, frequency);
  hipStream_t s = as_stream(stream);
  const int64_t n = rows * channels * depth * (int64_t)H * W;
  ProfScope prof(s, "simplex_noise", 0.0, 4.0 * n);
  hipLaunchKernelGGL(simplex_noise_kernel, dim3((unsigned)(rows * channels)), dim3(256), 0, s, out, seeds, t, channels, depth, H,
                     W, octaves, persistence, frequency);
  DDPM_CHECK_LAUNCH();
  return 0;
}
