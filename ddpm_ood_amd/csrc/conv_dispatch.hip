// conv_dispatch.hip -- which kernel family takes a convolution descriptor.  The two tables below are the ONLY place the order is
// written down: the launch, the statistics contract (ddpm_conv_stats_parts), the scratch size and ddpm_conv_takes_wino44h all
// go through conv_select, so they cannot disagree.  The selection reads the descriptor and sw(), nothing else.  Host code only.
#include "common.h"

namespace ddpm {
namespace {

struct ConvKernel {
  const char *name;  // family name (ddpm_conv_kernel_name)
  bool (*takes)(const ddpm_conv_desc &);
  int (*launch)(const ddpm_conv_desc &, hipStream_t);
  size_t (*scratch_floats)(const ddpm_conv_desc &);  // nullptr: never needs scratch
  int (*stats_parts)(const ddpm_conv_desc &);        // nullptr: never writes stats_out
};

bool is3d(const ddpm_conv_desc &d) { return d.dims == 3 && d.ksize != 1; }
bool volumetric(const ddpm_conv_desc &d) { return is3d(d) || d.mode == DDPM_CONV_TRANSPOSE2 || d.ksize == 4; }

// 3-D convolutions, k4 s2 and ConvTranspose: the Winograd forms for 3-D k3 s1, everything else only exists on the MFMA kernel
// (no generic fallback: conv_dispatch refuses a descriptor no row takes).  No 3-D kernel splits its channels or writes statistics.
const ConvKernel kVolumetric[] = {
    {"wino44h", [](const ddpm_conv_desc &d) { return is3d(d) && conv_wino44h_supported(d); }, launch_conv_wino44h, nullptr, nullptr},  // VQ-VAE residual units, split-f16
    {"wino44", [](const ddpm_conv_desc &d) { return is3d(d) && conv_wino44_supported(d); }, launch_conv_wino44, nullptr, nullptr},
    {"wino", [](const ddpm_conv_desc &d) { return is3d(d) && d.w_wino && conv_wino_supported(d); }, launch_conv_wino, nullptr, nullptr},
    {"mfma", conv_mfma_supported, launch_conv_mfma, conv_mfma_scratch_floats, nullptr},
};

const ConvKernel kPlanar[] = {
    {"linear_skinny", linear_skinny_supported, launch_linear_skinny, nullptr, nullptr},  // Linear over <= 1024 rows: latency, not FLOPs
    {"d3s", conv_d3s_supported, launch_conv_d3s, conv_d3s_scratch_floats, conv_d3s_stats_parts},  // small launches: one-shot direct 3x3, split-f16
    {"wino44h", conv_wino44h_supported, launch_conv_wino44h, conv_wino44h_scratch_floats, conv_wino44h_stats_parts},  // F(4x4) with split-f16 position GEMMs
    {"wino44", conv_wino44_supported, launch_conv_wino44, conv_wino44_scratch_floats, nullptr},
    {"wino", conv_wino_supported, launch_conv_wino, conv_wino_scratch_floats, conv_wino_stats_parts},  // (statistics: the Upsample form only)
    {"d3s2", conv_d3s2_supported, launch_conv_d3s2, conv_d3s2_scratch_floats, conv_d3s_stats_parts},  // Downsample of small launches: one-shot, split-f16 (the same reduce pass as d3s)
    {"s2h", conv_s2h_supported, launch_conv_s2h, nullptr, conv_s2h_stats_parts},  // Downsample: direct 3x3 stride 2 on the f16 MFMA, split-f16 operands
    {"d1s", conv_d1s_supported, launch_conv_d1s, conv_d1s_scratch_floats, nullptr},  // small launches: one-shot 1x1, split-f16
    {"conv1x1_dma", [](const ddpm_conv_desc &d) { return conv1x1_dma_supported(d) && conv_mfma_supported(d); }, launch_conv1x1_dma, nullptr, nullptr},
    {"mfma", conv_mfma_supported, launch_conv_mfma, conv_mfma_scratch_floats, nullptr},
    {"direct", conv_direct_supported, launch_conv_direct, nullptr, conv_direct_stats_parts},  // conv_in / conv_out and every shape without a tiling
};

// the first row that takes d (nullptr: a volumetric descriptor without an MFMA tiling)
template <size_t N>
const ConvKernel *first_taker(const ConvKernel (&table)[N], const ddpm_conv_desc &d) {
  for (const ConvKernel &k : table)
    if (k.takes(d)) return &k;
  return nullptr;
}
const ConvKernel *conv_select(const ddpm_conv_desc &d) { return volumetric(d) ? first_taker(kVolumetric, d) : first_taker(kPlanar, d); }

int conv_validate(const ddpm_conv_desc &d) {
  DDPM_CHECK_ARG(d.in1 && d.out && d.B > 0 && d.Cout > 0 && d.C1 > 0, "conv: null tensor or empty shape");
  DDPM_CHECK_ARG(d.C2 == 0 || d.in2, "conv: C2 > 0 but in2 is NULL");
  DDPM_CHECK_ARG((d.gscale == nullptr) == (d.gshift == nullptr), "conv: gscale/gshift must come together");
  if (d.mode == DDPM_CONV_NORMAL)
    DDPM_CHECK_ARG(d.Hi == d.Ho && d.Wi == d.Wo, "conv: normal mode needs Hi == Ho, Wi == Wo");
  if (d.mode == DDPM_CONV_UPSAMPLE2)
    DDPM_CHECK_ARG(d.Ho == 2 * d.Hi && d.Wo == 2 * d.Wi && d.ksize == 3, "conv: upsample needs Ho == 2 Hi, k == 3");
  if (d.mode == DDPM_CONV_STRIDE2 && d.ksize == 3)
    DDPM_CHECK_ARG(d.Ho == (d.Hi + 1) / 2 && d.Wo == (d.Wi + 1) / 2, "conv: stride-2 k3 needs Ho == ceil(Hi / 2)");
  if (d.mode == DDPM_CONV_STRIDE2 && d.ksize == 4)
    DDPM_CHECK_ARG(d.Ho == d.Hi / 2 && d.Wo == d.Wi / 2 && d.Ho > 0 && d.Wo > 0, "conv: stride-2 k4 needs Ho == Hi / 2");
  DDPM_CHECK_ARG(d.mode != DDPM_CONV_STRIDE2 || d.ksize == 3 || d.ksize == 4, "conv: stride-2 needs k == 3 or 4");
  if (volumetric(d)) {
    const int Di = d.Di > 1 ? d.Di : 1, Do = d.Do > 1 ? d.Do : 1;
    if (is3d(d) && d.mode == DDPM_CONV_NORMAL) DDPM_CHECK_ARG(Di == Do, "conv3d: normal mode needs Di == Do");
    if (is3d(d) && d.mode == DDPM_CONV_UPSAMPLE2) DDPM_CHECK_ARG(Do == 2 * Di, "conv3d: upsample needs Do == 2 Di");
    if (is3d(d) && d.mode == DDPM_CONV_STRIDE2)
      DDPM_CHECK_ARG(Do == (d.ksize == 3 ? (Di + 1) / 2 : Di / 2) && Do > 0, "conv3d: stride-2 output depth");
  } else {
    DDPM_CHECK_ARG(d.Di <= 1 && d.Do <= 1, "conv: Di / Do > 1 needs dims == 3");
  }
  return 0;
}

}  // namespace

int conv_dispatch(const ddpm_conv_desc &d, hipStream_t s) {
  if (const int rc = conv_validate(d)) return rc;
  const ConvKernel *k = conv_select(d);
  DDPM_CHECK_ARG(k != nullptr,
                 "conv: 3-D / k4 / transposed convolutions need an MFMA tiling (Cin %% 4 (8), Cout %% 128, packed weights)");
  return k->launch(d, s);
}

// slices of desc.stats_out the kernel that takes d writes (0: it does not, and stats_out is ignored)
int conv_stats_parts(const ddpm_conv_desc &d) {
  const ConvKernel *k = conv_select(d);
  return k && k->stats_parts ? k->stats_parts(d) : 0;
}

// The largest need of any family that could take d: the scratch is sized before it is attached, and several `takes` depend on
// its presence.  Every split but the MFMA kernel's split-K is 2-D only, and a Linear on linear_skinny needs no split-K.
size_t conv_scratch_floats(const ddpm_conv_desc &d) {
  const bool vol = d.dims == 3 || d.Di > 1 || d.Do > 1, skinny = linear_skinny_supported(d);
  size_t need = 0;
  for (const ConvKernel &k : kPlanar) {
    if (!k.scratch_floats) continue;
    if (k.launch == launch_conv_mfma ? skinny : vol) continue;
    const size_t n = k.scratch_floats(d);
    if (n > need) need = n;
  }
  return need;
}

}  // namespace ddpm

using namespace ddpm;

// Would ddpm_conv_f32 run this stride-1 3x3 descriptor on the split-f16 F(4x4) kernel if it were given w_wino44h?  (A caller that
// re-packs weights every step -- the training step -- packs the F(2x2) fallback form only when the answer is no.)
extern "C" int ddpm_conv_takes_wino44h(const ddpm_conv_desc *dp) {
  if (!dp) return 0;
  ddpm_conv_desc d = *dp;
  if (d.dims == 3 || d.ksize != 3) return 0;
  if (!d.w_wino44h) d.w_wino44h = reinterpret_cast<const uint16_t *>(uintptr_t(64));  // (only tested for non-NULL)
  if (!d.scratch) {  // (a launch split over channel slices needs scratch: the caller will size it with ddpm_conv_scratch_floats)
    d.scratch = reinterpret_cast<float *>(uintptr_t(64));
    d.scratch_floats = ~size_t(0);
  }
  const ConvKernel *k = conv_select(d);
  return k && k->launch == launch_conv_wino44h ? 1 : 0;  // (dims != 3: the row of kPlanar)
}

extern "C" const char *ddpm_conv_kernel_name(const ddpm_conv_desc *d) {
  const ConvKernel *k = d && conv_validate(*d) == 0 ? conv_select(*d) : nullptr;
  return k ? k->name : "";
}

extern "C" size_t ddpm_conv_kernel_scratch_floats(const ddpm_conv_desc *d) {
  const ConvKernel *k = d && conv_validate(*d) == 0 ? conv_select(*d) : nullptr;
  return k && k->scratch_floats ? k->scratch_floats(*d) : 0;
}
