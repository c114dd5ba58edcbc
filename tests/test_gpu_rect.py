"""-m gpu: rectangular images (H != W) and non-cubic volumes through every convolution family, the training kernels and the
whole networks.  --image_roi is a per-axis crop and every entry point takes the axes separately, but the rest of the suite only
ever builds H == W (and W == H slices for the stride-1 3-D convolutions): a swapped Hi / Wi, a row stride taken from the wrong
axis or a tile count that only holds for squares would pass it.

Every forward case ASSERTS the family ddpm_conv_kernel_name reports for the launched descriptor (a spy on ddpm_conv_f32, plus the
in-situ profiler: the kernel that ran belongs to that family), in both orientations wherever the selection table gives the
family both.  References are F.conv2d / F.conv3d / F.interpolate / F.group_norm in float64 on the CPU; the inputs are random, so
no result is symmetric under transposition.  Tolerances are those of each family's square test (the contraction length does
not depend on the aspect ratio):

    fp32 forms (wino, mfma, direct, conv1x1_dma)   |err| <= 2e-5 (1 + max|ref|)                       test_gpu_ops.py::_close
    F(4x4) (wino44, wino44h)                       |err| < 2e-4 (1 + max|ref|), rms < 1e-5 (1 + rms)  test_conv_winograd_f4x4
    s2h                                            max rel <= max(2 x the fp32 kernel's, 2e-6)        test_conv_stride2_split_f16_vs_conv2d
    d1s                                            max rel < 3e-6                                     test_conv1x1_small_launch_split_f16_vs_conv2d
    statistics slabs                               test_gpu_wino44h.py::_check_stats
    weight gradients                               max rel < 3e-6; input gradients 2e-5; GroupNorm 3e-6 / 1e-5

Worst errors measured on an MI355X (each case prints its own; `pytest -s`), next to the bound they were held to:

    block (worst case of it)            measured    bound         block                      measured    bound
    wino44h normal  max / rms           3.3e-05 / 1.7e-06  1.6e-03 / 2.5e-05   wgrad split-f16        4.8e-07     3e-06
    wino44h upsample  max / rms         4.5e-05 / 2.2e-06  1.6e-03 / 2.6e-05   wgrad staged fp32      4.5e-07     3e-06
    wino44  max / rms                   5.7e-05 / 2.9e-06  1.5e-03 / 2.6e-05   wgrad stride 2         3.9e-07     3e-06
    wino normal / upsample              1.3e-06 / 4.2e-06  1.6e-04 / 1.7e-04   wgrad plain            5.3e-07     3e-06
    s2h                                 5.7e-06            1.4e-05             wgrad generic          1.1e-07     3e-06
    mfma k3 / s2 / up / k1 / split-K    2.2e-06 .. 4.6e-06 1.4e-04 .. 1.7e-04  wgrad 3-D              3.9e-07     3e-06
    mfma folded upsample                6.0e-06            1.5e-04             input gradients        2.4e-07     2e-05
    direct normal / s2 / up             6.0e-06 .. 9.6e-06 1.6e-04 .. 1.8e-04  UNet forward 2-D / 3-D 5.0e-06 / 8.8e-06  2.7e-04 / 4.9e-04
    d1s                                 1.5e-06            2.5e-05             VQ-VAE                 2.3e-06     4.4e-05
    conv1x1_dma                         3.1e-06            2.0e-04             native step gradients  4.4e-05     1e-04
    gn_finalize (parts 3 and 6)         8.8e-07            1.9e-06
    3-D mfma / wino                     6.6e-06 / 3.7e-06  1.7e-04 / 1.4e-04
    3-D wino44  max / rms               4.8e-05 / 2.6e-06  1.5e-03 / 2.5e-05
    3-D wino44h  max / rms              3.1e-05 / 1.6e-06  1.4e-03 / 2.3e-05

No rectangle needed more than its family's square bound; the largest share of a bound used is the native step's (0.44).
"""

import ctypes
import json
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NORMAL, STRIDE2, UPSAMPLE2 = 0, 1, 2

# family -> prefixes of the ProfScope names of its launcher (tests/test_gpu_conv_select.py::PROF_KEYS)
PROF_KEYS = {
    "linear_skinny": ("linear_skinny",),
    "d3s": ("conv3x3_d3s",),
    "d3s2": ("conv3x3_d3s_stride2",),
    "d1s": ("conv1x1_d1s",),
    "wino44h": ("conv3x3_wino44h", "conv3d_wino44h"),
    "wino44": ("conv3x3_wino44", "conv3d_wino44"),
    "wino": ("conv3x3_wino", "conv3d_wino"),
    "s2h": ("conv3x3_s2h",),
    "conv1x1_dma": ("conv1x1_dma",),
    "mfma": ("conv3x3_mfma", "conv1x1_mfma", "conv3d_k3", "conv3d_k4s2", "conv3d_transpose_k4s2", "conv2d_k4s2",
             "conv2d_transpose_k4s2"),
    "direct": ("conv_direct", "conv3x3_small_cin", "conv3x3_small_cout"),
}


def _family_of(key):
    hits = [(len(p), fam) for fam, ps in PROF_KEYS.items() for p in ps if key.startswith(p)]
    return max(hits)[1] if hits else None


def _launch(fn, family):
    """fn() with a spy on ddpm_conv_f32 and the profiler on: every launched descriptor has to report `family`, and every
    profiled kernel that belongs to a convolution family (a split launch also shows its reduce pass) has to belong to it."""
    from ddpm_ood_amd import _lib

    lib = _lib.load()
    real = lib.ddpm_conv_f32
    names = []

    def spy(desc, stream):
        names.append(lib.ddpm_conv_kernel_name(desc).decode())
        return real(desc, stream)

    torch.cuda.synchronize()
    lib.ddpm_conv_f32 = spy
    lib.ddpm_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.ddpm_prof_enable(0)
        lib.ddpm_conv_f32 = real
    buf = ctypes.create_string_buffer(1 << 16)
    n = lib.ddpm_prof_report(buf, len(buf))
    report = json.loads(buf.value.decode()) if n > 0 else {}
    assert names and all(nm == family for nm in names), (names, family)
    ran = [_family_of(k) for k in report]
    assert family in ran and all(f in (None, family) for f in ran), (report.keys(), family)
    return out


WORST = {}


def _note(block, what, err, bound):
    WORST[block] = max(WORST.get(block, 0.0), err / bound)
    print(f"rect[{block}] {what}: err {err:.3e} bound {bound:.3e} ({err / bound:.2f} of it)")


def _check_stats(y, st, parts):  # tests/test_gpu_wino44h.py::_check_stats, slices = contiguous runs of Ho * Wo / parts pixels
    B, Cout = y.shape[:2]
    assert st is not None and tuple(st.shape) == (B, Cout, parts, 2), None if st is None else st.shape
    assert (y.shape[2] * y.shape[3]) % parts == 0
    yd = y.double().cpu().view(B, Cout, parts, -1)
    mean = yd.mean(-1)
    m2 = (yd - mean[..., None]).pow(2).sum(-1)
    st = st.cpu().double()
    sd = (m2 / yd.shape[-1]).sqrt()
    assert (st[..., 0] - mean).abs().max().item() <= 2e-6 * (1 + mean.abs().max().item() + sd.max().item())
    assert ((st[..., 1] - m2).abs() / (m2 + 1e-3 * m2.mean())).max().item() <= 2e-5


def _pack(ops, w, k, mode, names):
    pack = {"wino": ops.pack_wino_weight, "wino44": ops.pack_wino44_weight, "folded": ops.fold_upsample_weight,
            "wino44h": ops.pack_conv1x1_h_weight if k == 1 else ops.pack_conv_s2h_weight if mode == STRIDE2 else ops.pack_wino44h_weight,
            "d3h": ops.pack_conv_d1s_weight if k == 1 else ops.pack_conv_d3h_weight}
    out = {n: pack[n](w) for n in names}
    assert all(v is not None for v in out.values()), {n: v is not None for n, v in out.items()}
    return out


def _out_extent(k, mode, e):
    return (e + 1) // 2 if mode == STRIDE2 else 2 * e if mode == UPSAMPLE2 else e


def _inputs(case):
    """Random operands of a case (CPU fp32) and the float64 reference.  fused: GroupNorm (+ SiLU for 3x3) prologue over the
    (virtual) concat, chan_add read at an offset of 32 in rows of Cout + 64, residual -- as CASES of test_gpu_wino44h.py."""
    _, _, _, B, C1, C2, Cout, H, W, k, mode, _, opt = case
    g = torch.Generator().manual_seed(zlib.crc32(repr(case[:11]).encode()) & 0xFFFF)
    Cin = C1 + C2
    fused = opt.get("fused", False)
    x = torch.randn(B, C1, H, W, generator=g) * 1.3 + 0.2
    x2 = torch.randn(B, C2, H, W, generator=g) * 1.5 + 0.3 if C2 else None
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g)
    Ho, Wo = _out_extent(k, mode, H), _out_extent(k, mode, W)
    gamma = beta = chan_add = residual = None
    if fused:
        gamma, beta = torch.randn(Cin, generator=g) * 0.2 + 1, torch.randn(Cin, generator=g) * 0.2
        if k == 3:
            chan_add = torch.randn(B, Cout + 64, generator=g)
        residual = torch.randn(B, Cout, Ho, Wo, generator=g)
    xin = (x if x2 is None else torch.cat([x, x2], 1)).double()
    if fused:
        xin = F.group_norm(xin, 32, gamma.double(), beta.double(), 1e-6)
        if k == 3:
            xin = F.silu(xin)
    if mode == UPSAMPLE2:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(xin, w.double(), b.double(), stride=2 if mode == STRIDE2 else 1, padding=k // 2)
    if chan_add is not None:
        ref = ref + chan_add.double()[:, 32:32 + Cout, None, None]
    if residual is not None:
        ref = ref + residual.double()
    return (x, x2, w, b, gamma, beta, chan_add, residual), ref


def _conv(device, case, tensors, forms, want_stats=True, **more):
    from ddpm_ood_amd import ops

    k, mode, opt = case[9], case[10], case[12]
    x, x2, w, b, gamma, beta, chan_add, residual = tensors
    d = lambda t: None if t is None else t.to(device)  # noqa: E731
    gs = gh = None
    if gamma is not None:
        gs, gh = ops.gn_scale_shift(d(x), d(gamma), d(beta), 32, 1e-6, x2=d(x2))
    kw = dict(x2=d(x2), gscale=gs, gshift=gh, act=int(gamma is not None and k == 3), mode=mode, chan_add=d(chan_add),
              chan_add_offset=32 if chan_add is not None else 0, residual=d(residual), want_stats=want_stats)
    kw.update(_pack(ops, d(w), k, mode, forms))
    kw.update(more)
    return ops.conv(d(x), d(w), d(b), **kw)


def _hold(block, what, tol, y, ref, y_fp32=None):
    y, scale = y.detach().cpu().double(), ref.abs().max().item()
    assert y.shape == ref.shape, (y.shape, ref.shape)
    err = (y - ref).abs().max().item()
    assert math.isfinite(err)
    if tol == "f32":
        bound = 2e-5 * (1 + scale)
    elif tol == "f44":
        bound = 2e-4 * (1 + scale)
        rms, rbound = (y - ref).pow(2).mean().sqrt().item(), 1e-5 * (1 + ref.pow(2).mean().sqrt().item())
        _note(block + " rms", what, rms, rbound)
        assert rms < rbound, (what, rms, rbound)
    elif tol == "s2h":
        e_old = (y_fp32.detach().cpu().double() - ref).abs().max().item()
        bound = max(2 * e_old, 2e-6 * scale)
    elif tol == "d1s":
        bound = 3e-6 * scale
    _note(block, what, err, bound)
    assert err <= bound, (what, err, bound)


W44 = {"DDPM_CONV_WINO44": "2"}  # lifts the launch-size gate of the F(4x4) kernels, so that B stays small
FUSED = {"fused": True}
# (id, family, stats parts, B, C1, C2, Cout, H, W, ksize, mode, weight forms, options {env, fused, tol, split_f16})
CASES = [
    # ---- wino44h, normal: 1-unit items of 8 images (ragged at B = 9), 10- / 9-unit items, 3 parts, 4 x 16 ---------------------
    ("w44h-8x32", "wino44h", 1, 9, 64, 0, 64, 8, 32, 3, NORMAL, ("wino44h",), {"env": W44}),
    ("w44h-32x8", "wino44h", 1, 9, 64, 0, 64, 32, 8, 3, NORMAL, ("wino44h",), {"env": W44}),
    ("w44h-8x32-fused", "wino44h", 1, 9, 256, 128, 128, 8, 32, 3, NORMAL, ("wino44h",), {"env": W44, **FUSED}),
    ("w44h-32x8-fused", "wino44h", 1, 9, 256, 128, 128, 32, 8, 3, NORMAL, ("wino44h",), {"env": W44, **FUSED}),
    ("w44h-16x64", "wino44h", 2, 2, 64, 0, 64, 16, 64, 3, NORMAL, ("wino44h",), {"env": W44}),
    ("w44h-64x16", "wino44h", 2, 2, 64, 0, 64, 64, 16, 3, NORMAL, ("wino44h",), {"env": W44}),
    ("w44h-16x64-fused", "wino44h", 2, 2, 256, 128, 128, 16, 64, 3, NORMAL, ("wino44h",), {"env": W44, **FUSED}),
    ("w44h-64x16-fused", "wino44h", 2, 3, 256, 128, 128, 64, 16, 3, NORMAL, ("wino44h",), {"env": W44, **FUSED}),
    ("w44h-48x32", "wino44h", 3, 2, 64, 0, 64, 48, 32, 3, NORMAL, ("wino44h",), {"env": W44, "finalize": True}),
    ("w44h-48x32-fused", "wino44h", 3, 3, 256, 128, 128, 48, 32, 3, NORMAL, ("wino44h",), {"env": W44, **FUSED}),
    ("w44h-4x16", "wino44h", 1, 9, 64, 0, 64, 4, 16, 3, NORMAL, ("wino44h",), {"env": W44}),
    ("w44h-16x4", "wino44h", 1, 9, 64, 0, 64, 16, 4, 3, NORMAL, ("wino44h",), {"env": W44}),
    ("w44h-4x16-fused", "wino44h", 1, 9, 256, 128, 128, 4, 16, 3, NORMAL, ("wino44h",), {"env": W44, **FUSED}),
    # 128 x 32 is the last rectangle of the table wino44h takes (32 x 128 belongs to mfma: below)
    ("w44h-128x32", "wino44h", 8, 1, 64, 0, 64, 128, 32, 3, NORMAL, ("wino44h",), {"env": W44}),
    # 16 x 32 and 32 x 16 are 8 staging units: no item shape of the kernel -> with wino44 absent the F(2x2) kernel runs
    ("w44h-refuses-16x32", "wino", 0, 2, 64, 0, 64, 16, 32, 3, NORMAL, ("wino", "wino44h"), {"env": W44}),
    ("w44h-refuses-32x16", "wino", 0, 2, 64, 0, 64, 32, 16, 3, NORMAL, ("wino", "wino44h"), {"env": W44}),
    # channel-split launch (default gate, scratch): 2 x 3 x 16 = 96 items, S = 2, statistics from the reduce pass in 6 parts
    ("w44h-split-48x32", "wino44h", 6, 16, 128, 0, 128, 48, 32, 3, NORMAL, ("wino", "wino44h"), {"fused": True, "finalize": True}),
    # ---- wino44h, upsample -------------------------------------------------------------------------------------------------------
    ("w44h-up-32x8", "wino44h", 2, 2, 128, 0, 128, 32, 8, 3, UPSAMPLE2, ("wino44h",), {"env": W44}),
    ("w44h-up-16x4", "wino44h", 1, 9, 128, 0, 128, 16, 4, 3, UPSAMPLE2, ("wino44h",), {"env": W44}),
    ("w44h-up-64x4", "wino44h", 2, 2, 128, 0, 128, 64, 4, 3, UPSAMPLE2, ("wino44h",), {"env": W44}),
    # ---- wino44 (fp32 F(4x4)): the split-f16 kernel switched off with both forms attached -------------------------------------
    ("w44-16x32", "wino44", 0, 2, 128, 0, 128, 16, 32, 3, NORMAL, ("wino", "wino44", "wino44h"), {"env": {**W44, "DDPM_WINO44_F16X3": "0"}}),
    ("w44-32x16", "wino44", 0, 2, 128, 0, 128, 32, 16, 3, NORMAL, ("wino", "wino44", "wino44h"), {"env": {**W44, "DDPM_WINO44_F16X3": "0"}, **FUSED}),
    ("w44-8x32", "wino44", 0, 9, 64, 0, 64, 8, 32, 3, NORMAL, ("wino", "wino44", "wino44h"), {"env": W44, "split_f16": False}),
    ("w44-64x16", "wino44", 0, 2, 256, 128, 128, 64, 16, 3, NORMAL, ("wino", "wino44", "wino44h"), {"env": W44, "split_f16": False, **FUSED}),
    # ---- wino (fp32 F(2x2)) -----------------------------------------------------------------------------------------------------
    ("wino-8x16", "wino", 0, 3, 128, 0, 128, 8, 16, 3, NORMAL, ("wino",), {}),
    ("wino-16x8", "wino", 0, 3, 128, 0, 128, 16, 8, 3, NORMAL, ("wino",), FUSED),
    ("wino-4x64", "wino", 0, 3, 256, 128, 128, 4, 64, 3, NORMAL, ("wino",), FUSED),
    ("wino-64x4", "wino", 0, 3, 64, 0, 64, 64, 4, 3, NORMAL, ("wino",), {}),
    ("wino-up-8x16", "wino", 4, 1, 128, 0, 128, 8, 16, 3, UPSAMPLE2, ("wino",), {"folded": True}),
    ("wino-up-16x8", "wino", 4, 1, 128, 0, 128, 16, 8, 3, UPSAMPLE2, ("wino",), {"folded": True}),
    ("wino-up-24x8", "wino", 6, 2, 128, 0, 128, 24, 8, 3, UPSAMPLE2, ("wino",), {"folded": True, "finalize": True}),
    ("wino-up-2x32", "wino", 2, 1, 128, 0, 128, 2, 32, 3, UPSAMPLE2, ("wino",), {"folded": True}),
    ("wino-up-32x2", "wino", 2, 1, 128, 0, 128, 32, 2, 3, UPSAMPLE2, ("wino",), {"folded": True}),
    ("wino-up-8x32", "wino", 8, 2, 128, 0, 128, 8, 32, 3, UPSAMPLE2, ("wino",), {"folded": True}),
    ("wino-up-32x8", "wino", 8, 2, 128, 0, 128, 32, 8, 3, UPSAMPLE2, ("wino",), {"folded": True}),
    # ---- s2h (Downsample on the f16 MFMA); =2 / =3: one kernel form each ------------------------------------------------------
    ("s2h-8x16", "s2h", 1, 3, 128, 0, 128, 8, 16, 3, STRIDE2, ("wino44h",), {"tol": "s2h"}),
    ("s2h-16x8", "s2h", 1, 3, 128, 0, 128, 16, 8, 3, STRIDE2, ("wino44h",), {"tol": "s2h"}),
    ("s2h-32x16", "s2h", 1, 3, 64, 0, 64, 32, 16, 3, STRIDE2, ("wino44h",), {"tol": "s2h"}),
    ("s2h-16x32", "s2h", 1, 3, 64, 0, 64, 16, 32, 3, STRIDE2, ("wino44h",), {"tol": "s2h"}),
    ("s2h-16x64", "s2h", 2, 3, 128, 0, 128, 16, 64, 3, STRIDE2, ("wino44h",), {"tol": "s2h"}),
    ("s2h-64x16", "s2h", 2, 3, 128, 0, 128, 64, 16, 3, STRIDE2, ("wino44h",), {"tol": "s2h"}),
    ("s2h-48x32", "s2h", 3, 3, 64, 0, 64, 48, 32, 3, STRIDE2, ("wino44h",), {"tol": "s2h", "finalize": True}),
    ("s2h-128x32", "s2h", 8, 2, 64, 0, 64, 128, 32, 3, STRIDE2, ("wino44h",), {"tol": "s2h"}),
    ("s2h-32x128", "s2h", 8, 2, 64, 0, 64, 32, 128, 3, STRIDE2, ("wino44h",), {"tol": "s2h"}),
    ("s2h-4x16", "s2h", 0, 11, 64, 0, 64, 4, 16, 3, STRIDE2, ("wino44h",), {"tol": "s2h"}),
    ("s2h-16x4", "s2h", 0, 11, 64, 0, 64, 16, 4, 3, STRIDE2, ("wino44h",), {"tol": "s2h"}),
    ("s2h-form2-32x16", "s2h", 1, 5, 128, 0, 128, 32, 16, 3, STRIDE2, ("wino44h",), {"tol": "s2h", "env": {"DDPM_DOWN_S2H": "2"}}),
    ("s2h-form3-16x32", "s2h", 1, 5, 128, 0, 128, 16, 32, 3, STRIDE2, ("wino44h",), {"tol": "s2h", "env": {"DDPM_DOWN_S2H": "3"}}),
    # ---- mfma -----------------------------------------------------------------------------------------------------------------------
    ("mfma-k3-8x24", "mfma", 0, 3, 128, 0, 128, 8, 24, 3, NORMAL, ("wino", "wino44", "wino44h"), FUSED),
    ("mfma-k3-24x8", "mfma", 0, 3, 128, 0, 128, 24, 8, 3, NORMAL, ("wino", "wino44", "wino44h"), {}),
    ("mfma-s2-16x32", "mfma", 0, 2, 256, 128, 256, 16, 32, 3, STRIDE2, (), FUSED),
    ("mfma-s2-32x16", "mfma", 0, 2, 256, 128, 256, 32, 16, 3, STRIDE2, (), {}),
    ("mfma-up-16x12", "mfma", 0, 2, 128, 0, 128, 16, 12, 3, UPSAMPLE2, ("folded",), {}),
    ("mfma-up-12x16", "mfma", 0, 2, 128, 0, 128, 12, 16, 3, UPSAMPLE2, (), {}),
    ("mfma-up-8x24", "mfma", 0, 2, 128, 0, 128, 8, 24, 3, UPSAMPLE2, ("wino",), {}),  # (24 x 8 is the F(2x2) Upsample kernel's: above)
    ("mfma-s2-9x6", "mfma", 0, 3, 128, 0, 128, 9, 6, 3, STRIDE2, (), {}),  # odd extents: Ho = ceil(Hi / 2)
    ("mfma-k1-8x24", "mfma", 0, 3, 256, 128, 256, 8, 24, 1, NORMAL, (), {"env": {"DDPM_CONV1X1_DMA": "0"}, **FUSED}),
    ("mfma-k1-24x8", "mfma", 0, 3, 128, 0, 128, 24, 8, 1, NORMAL, (), {"env": {"DDPM_CONV1X1_DMA": "0"}}),
    # ---- direct: no tiling (64 -> 64 at 8 x 24, 12 x 16), conv_in / conv_out, odd stride-2 extents, 32 x 128 Upsample ------------
    ("direct-8x24", "direct", 0, 2, 64, 0, 64, 8, 24, 3, NORMAL, (), {}),
    ("direct-24x8", "direct", 0, 2, 64, 0, 64, 24, 8, 3, NORMAL, (), FUSED),
    ("direct-12x16", "direct", 0, 2, 64, 0, 64, 12, 16, 3, NORMAL, (), {}),
    ("direct-16x12", "direct", 0, 2, 64, 0, 64, 16, 12, 3, NORMAL, (), {}),
    ("direct-in-16x32", "direct", 2, 3, 1, 0, 128, 16, 32, 3, NORMAL, (), {}),
    ("direct-in-32x16", "direct", 2, 3, 1, 0, 128, 32, 16, 3, NORMAL, (), {}),
    ("direct-in-28x20", "direct", 0, 3, 1, 0, 128, 28, 20, 3, NORMAL, (), {}),
    ("direct-in-20x28", "direct", 0, 3, 3, 0, 128, 20, 28, 3, NORMAL, (), {}),
    ("direct-out1-16x32", "direct", 0, 3, 128, 0, 1, 16, 32, 3, NORMAL, (), {}),
    ("direct-out3-32x16", "direct", 0, 3, 128, 0, 3, 32, 16, 3, NORMAL, (), {}),
    ("direct-out3-28x20", "direct", 0, 3, 128, 0, 3, 28, 20, 3, NORMAL, (), {}),
    ("direct-out1-20x28", "direct", 0, 3, 128, 0, 1, 20, 28, 3, NORMAL, (), {}),
    ("direct-s2-7x10", "direct", 0, 3, 64, 0, 64, 7, 10, 3, STRIDE2, (), {}),
    ("direct-s2-9x6", "direct", 0, 3, 64, 0, 64, 9, 6, 3, STRIDE2, (), {}),
    ("direct-s2-32x48", "direct", 0, 3, 64, 0, 64, 32, 48, 3, STRIDE2, ("wino44h",), {}),  # (48 x 32 is s2h's: above)
    ("direct-up-32x128", "direct", 0, 1, 128, 0, 128, 32, 128, 3, UPSAMPLE2, ("folded", "wino", "wino44h", "d3h"), {}),
    # ---- d1s / conv1x1_dma ---------------------------------------------------------------------------------------------------------
    ("d1s-8x16", "d1s", 0, 1, 128, 0, 128, 8, 16, 1, NORMAL, ("wino44h", "d3h"), {"tol": "d1s"}),
    ("d1s-16x8", "d1s", 0, 1, 256, 128, 256, 16, 8, 1, NORMAL, ("wino44h", "d3h"), {"tol": "d1s", **FUSED}),
    ("d1s-32x64", "d1s", 0, 1, 128, 0, 128, 32, 64, 1, NORMAL, ("wino44h", "d3h"), {"tol": "d1s", **FUSED}),
    ("d1s-64x32", "d1s", 0, 1, 256, 128, 256, 64, 32, 1, NORMAL, ("wino44h", "d3h"), {"tol": "d1s"}),
    ("d1s-4x64", "d1s", 0, 1, 128, 0, 128, 4, 64, 1, NORMAL, ("wino44h", "d3h"), {"tol": "d1s"}),
    ("d1s-64x4", "d1s", 0, 1, 256, 128, 256, 64, 4, 1, NORMAL, ("wino44h", "d3h"), {"tol": "d1s", **FUSED}),
    ("dma-32x64", "conv1x1_dma", 0, 16, 128, 0, 128, 32, 64, 1, NORMAL, ("wino44h",), {}),
    ("dma-64x32", "conv1x1_dma", 0, 16, 256, 128, 256, 64, 32, 1, NORMAL, ("wino44h",), FUSED),
    ("dma-32x48", "conv1x1_dma", 0, 16, 128, 0, 128, 32, 48, 1, NORMAL, (), FUSED),
    # ---- d3s / d3s2 refuse rectangles, also when forced on: the next rows of the table run, and are right ----------------------
    ("d3s-refuses-8x16", "wino", 0, 2, 128, 0, 128, 8, 16, 3, NORMAL, ("wino", "wino44", "wino44h", "d3h"), {"env": {"DDPM_CONV_D3S": "2"}, **FUSED}),
    ("d3s-refuses-16x8", "wino", 0, 2, 128, 0, 128, 16, 8, 3, NORMAL, ("wino", "wino44", "wino44h", "d3h"), {"env": {"DDPM_CONV_D3S": "2"}}),
    ("d3s2-refuses-16x32", "s2h", 1, 2, 128, 0, 128, 16, 32, 3, STRIDE2, ("wino44h", "d3h"), {"env": {"DDPM_CONV_D3S": "2"}, "tol": "s2h"}),
]
TOL = {"wino44h": "f44", "wino44": "f44", "wino": "f32", "mfma": "f32", "direct": "f32", "conv1x1_dma": "f32"}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_forward_family_on_rectangles(device, case, monkeypatch):
    from ddpm_ood_amd import _lib, ops

    name, family, parts, B, C1, C2, Cout, H, W, k, mode, forms, opt = case
    assert H != W
    for var, val in opt.get("env", {}).items():
        monkeypatch.setenv(var, val)
    tensors, ref = _inputs(case)
    prev = _lib.set_split_f16(opt.get("split_f16", True))
    try:
        y, st = _launch(lambda: _conv(device, case, tensors, forms), family)
        y_again, st_again = _conv(device, case, tensors, forms)
        y_plain = _conv(device, case, tensors, forms, want_stats=False)
    finally:
        _lib.set_split_f16(prev)
    assert torch.equal(y, y_again) and torch.equal(y, y_plain)  # reproducible; the same output with and without statistics
    tol = opt.get("tol", TOL.get(family))
    y_fp32 = _conv(device, case, tensors, (), want_stats=False) if tol == "s2h" else None  # the fp32 kernel s2h replaced
    if y_fp32 is not None:
        assert not torch.equal(y, y_fp32)
    block = family + {NORMAL: "", STRIDE2: " s2", UPSAMPLE2: " up"}[mode] + (" k1" if k == 1 else "")
    _hold(block, name, tol, y, ref, y_fp32)
    assert (st is None) == (parts == 0), (parts, None if st is None else st.shape)
    if st is not None:
        _check_stats(y, st, parts)
        assert torch.equal(st, st_again)
    if opt.get("folded"):  # the Upsample F(2x2) kernel against the folded form of the same operator (another family)
        y_f = _conv(device, case, tensors, ("folded",), want_stats=False)
        assert not torch.equal(y, y_f)
        assert (y - y_f).abs().max().item() < 4e-5 * (1 + ref.abs().max().item())
        _hold("folded upsample", name, "f32", y_f, ref)
    if opt.get("finalize"):
        # the slab through ddpm_gn_finalize_f32 (parts = 3 and 6 only exist on rectangles) against F.group_norm of the produced
        # tensor: bounds of test_gn_finalize_from_channel_stats_matches_group_norm
        assert parts in (3, 6)
        g = torch.Generator().manual_seed(parts)
        gamma, beta = torch.randn(Cout, generator=g) * 0.3 + 1, torch.randn(Cout, generator=g) * 0.3
        sc, sh = ops.gn_finalize(st, gamma.to(device), beta.to(device), 32, 1e-6, y.shape[2] * y.shape[3])
        sc_r, sh_r = ops.gn_scale_shift(y, gamma.to(device), beta.to(device), 32, 1e-6)
        yd = y.cpu().double()
        want = F.group_norm(yd, 32, gamma.double(), beta.double(), 1e-6)
        got = yd * sc.cpu().double()[:, :, None, None] + sh.cpu().double()[:, :, None, None]
        old = yd * sc_r.cpu().double()[:, :, None, None] + sh_r.cpu().double()[:, :, None, None]
        e_new, e_old = (got - want).abs().max().item(), (old - want).abs().max().item()
        _note("gn_finalize", f"{name} parts {parts}", e_new, min(5e-6, 2 * e_old + 1e-6))
        assert e_new <= 5e-6 and e_new <= 2 * e_old + 1e-6, (e_new, e_old)


@pytest.mark.parametrize("H,W", [(8, 16), (16, 8)])
def test_mfma_split_k_on_rectangles(device, monkeypatch, H, W):
    """test_conv_mfma_split_k's first launch (fused q / k / v 1x1 behind a GroupNorm, 4 x 6 workgroups: every tile is split over
    K) on a rectangle: against float64, against the unsplit launch (DDPM_CONV_SPLITK=0), bit-reproducible."""
    case = ("splitk", "mfma", 0, 4, 256, 0, 768, H, W, 1, NORMAL, (), FUSED)
    tensors, ref = _inputs(case)
    monkeypatch.delenv("DDPM_CONV_SPLITK", raising=False)
    y = _launch(lambda: _conv(device, case, tensors, (), want_stats=False), "mfma")
    assert torch.equal(y, _conv(device, case, tensors, (), want_stats=False))  # fixed slab order
    monkeypatch.setenv("DDPM_CONV_SPLITK", "0")
    y0 = _launch(lambda: _conv(device, case, tensors, (), want_stats=False), "mfma")
    assert not torch.equal(y, y0)  # the split launch really ran
    _hold("mfma split-K", f"{H}x{W}", "f32", y, ref)
    _hold("mfma split-K", f"{H}x{W} unsplit", "f32", y0, ref)
    assert (y - y0).abs().max().item() <= 2e-6 * (1 + ref.abs().max().item())


# ---- (b) training kernels ----------------------------------------------------------------------------------------------------------

def _rel(a, b):
    return float((a.double().cpu() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


WGRAD_RECT = [  # B, Cin, Cout, H, W, ksize, stride, form
    (3, 64, 64, 16, 8, 3, 1, "split"), (3, 64, 128, 8, 16, 3, 1, "split"), (3, 128, 64, 4, 32, 3, 1, "split"),
    (2, 64, 128, 32, 64, 3, 1, "split"), (2, 128, 128, 32, 8, 3, 1, "split"), (2, 64, 64, 64, 32, 3, 1, "split"),
    (3, 64, 64, 2, 16, 3, 1, "staged"), (3, 64, 128, 12, 24, 3, 1, "staged"), (3, 64, 64, 24, 12, 3, 1, "staged"),
    (3, 128, 128, 16, 32, 3, 2, "stride2"), (3, 64, 64, 24, 8, 3, 2, "stride2"), (3, 64, 128, 32, 16, 3, 2, "stride2"),
    (3, 64, 64, 8, 6, 3, 1, "plain"), (3, 64, 128, 5, 10, 3, 1, "plain"), (3, 64, 64, 12, 6, 3, 1, "plain"),
    (4, 1, 128, 16, 32, 3, 1, "generic"), (4, 128, 3, 16, 32, 3, 1, "generic"), (4, 1, 128, 32, 16, 3, 1, "generic"),
    (4, 128, 3, 32, 16, 3, 1, "generic"), (3, 64, 64, 10, 5, 3, 1, "generic"),  # (an odd width has no MFMA form)
]


@pytest.mark.parametrize("case", WGRAD_RECT, ids=["-".join(map(str, c)) for c in WGRAD_RECT])
def test_conv_wgrad_on_rectangles(device, case, monkeypatch):
    """tests/test_gpu_train_ops.py::test_conv_wgrad_vs_autograd with H != W: float64 autograd at 3e-6, the generic form as a
    cross-check, bit-reproducible.  The rows named "split" are those the split-f16 form takes (DDPM_WGRAD_F16X3=0 has to select
    another kernel for them, and only for them)."""
    from ddpm_ood_amd import _lib
    from ddpm_ood_amd import train_ops as T

    B, cin, cout, H, W, k, s, form = case
    g = torch.Generator().manual_seed(sum(case[:7]))
    a = torch.randn(B, cin, H, W, generator=g)
    w = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(a.double(), w, stride=s, padding=k // 2)
    assert tuple(y.shape[2:]) == ((H + s - 1) // s, (W + s - 1) // s)
    dy = torch.randn(y.shape, generator=g)
    (ref,) = torch.autograd.grad(y, w, dy.double())
    mfma = form != "generic"
    assert not mfma or _lib.load().ddpm_conv_wgrad_scratch_floats(B, cin, cout, H, W, y.shape[2], y.shape[3], k, s) > 0
    ad, dyd = a.to(device), dy.to(device)
    dw = T.conv_wgrad(ad, dyd, k, s)
    e = _rel(dw, ref)
    _note("wgrad " + form, f"{case}", e, 3e-6)
    assert dw.shape == ref.shape and e < 3e-6, e
    assert torch.equal(dw, T.conv_wgrad(ad, dyd, k, s))
    if mfma:
        gen = T.conv_wgrad(ad, dyd, k, s, force_generic=True)
        assert _rel(gen, ref) < 3e-6 and not torch.equal(gen, dw)
    monkeypatch.setenv("DDPM_WGRAD_F16X3", "0")
    f32 = T.conv_wgrad(ad, dyd, k, s)
    assert _rel(f32, ref) < 3e-6
    assert torch.equal(f32, dw) == (form != "split"), form


def test_conv_wgrad_operand_maxima_on_a_rectangle(device):
    """a_absmax / dy_absmax handed in (partial maxima, any number of them): the same scale, the same bits."""
    from ddpm_ood_amd import train_ops as T

    B, cin, cout, H, W = 3, 64, 128, 8, 16
    g = torch.Generator().manual_seed(23)
    ad = (40.0 * torch.randn(B, cin, H, W, generator=g) * torch.exp(1.5 * torch.randn(B, cin, 1, 1, generator=g))).to(device)
    dyd = (3e-7 * torch.randn(B, cout, H, W, generator=g) * torch.exp(2.0 * torch.randn(B, cout, 1, 1, generator=g))).to(device)
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    (ref,) = torch.autograd.grad(F.conv2d(ad.cpu().double(), w, padding=1), w, dyd.cpu().double())
    dw = T.conv_wgrad(ad, dyd, 3, 1)
    assert _rel(dw, ref) < 3e-6, _rel(dw, ref)
    amax = ad.abs().view(B, -1).amax(dim=1).view(torch.int32)
    dmax = dyd.abs().view(B * 4, -1).amax(dim=1).view(torch.int32)
    assert torch.equal(T.conv_wgrad(ad, dyd, 3, 1, a_absmax=amax, dy_absmax=dmax), dw)
    assert torch.equal(T.conv_wgrad(ad, dyd, 3, 1, dy_absmax=dmax), dw)


@pytest.mark.parametrize("D,H,W", [(4, 8, 16), (2, 16, 8)])
@pytest.mark.parametrize("stride", [1, 2])
def test_conv3d_wgrad_and_input_gradient_on_non_cubic_volumes(device, D, H, W, stride):
    from ddpm_ood_amd import ops
    from ddpm_ood_amd import train_ops as T

    B, cin, cout = 2, 128, 64
    g = torch.Generator().manual_seed(D * 100 + H + stride)
    a = torch.randn(B, cin, D, H, W, generator=g)
    w0 = torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)
    ad, wd = a.double().requires_grad_(True), w0.double().requires_grad_(True)
    y = F.conv3d(ad, wd, stride=stride, padding=1)
    dy = torch.randn(y.shape, generator=g)
    ra, rw = torch.autograd.grad(y, (ad, wd), dy.double())
    dw = T.conv3d_wgrad(a.to(device), dy.to(device), stride)
    _note("wgrad 3-D", f"{(D, H, W)} s{stride}", _rel(dw, rw), 3e-6)
    assert dw.shape == rw.shape and _rel(dw, rw) < 3e-6, _rel(dw, rw)
    assert torch.equal(dw, T.conv3d_wgrad(a.to(device), dy.to(device), stride))
    wt = T.conv_weight_rot180t(w0.to(device))
    d = dy.to(device) if stride == 1 else T.zero_stuff2(dy.to(device))
    dx = ops.conv3d(d, wt, wino=ops.pack_wino3d_weight(wt))
    assert dx.shape == ra.shape and _rel(dx, ra) < 2e-5, _rel(dx, ra)


@pytest.mark.parametrize("H,W", [(16, 32), (32, 8)])
@pytest.mark.parametrize("kind", ["s1", "s2", "up"])
def test_conv_input_gradient_forms_on_rectangles(device, H, W, kind):
    from ddpm_ood_amd import ops
    from ddpm_ood_amd import train_ops as T

    B, cin, cout = 3, 128, 128
    g = torch.Generator().manual_seed(H + cin)
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
    x = torch.zeros(B, cin, H, W, dtype=torch.float64, requires_grad=True)
    if kind == "s1":
        y = F.conv2d(x, w.double(), padding=1)
    elif kind == "s2":
        y = F.conv2d(x, w.double(), stride=2, padding=1)
    else:
        y = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w.double(), padding=1)
    dy = torch.randn(y.shape, generator=g)
    (ref,) = torch.autograd.grad(y, x, dy.double())
    wt = T.conv_weight_rot180t(w.to(device))
    d = dy.to(device)
    if kind == "s2":
        d = T.zero_stuff2(d)
    dx = ops.conv(d, wt, wino44h=ops.pack_wino44h_weight(wt), wino=ops.pack_wino_weight(wt))
    if kind == "up":
        dx = T.sumpool2(dx)
    _note("dgrad", f"{kind} {H}x{W}", _rel(dx, ref), 2e-5)
    assert dx.shape == ref.shape and _rel(dx, ref) < 2e-5, _rel(dx, ref)


@pytest.mark.parametrize("act", [0, 1])
def test_group_norm_forward_and_backward_on_a_rectangle(device, act):
    from ddpm_ood_amd import train_ops as T

    B, C, H, W = 2, 128, 8, 24
    g = torch.Generator().manual_seed(C + H + W)
    x = torch.randn(B, C, H, W, generator=g) * 1.7 + 0.3
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    xd = x.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.group_norm(xd, 32, gd, bd, eps=1e-6)
    if act:
        y = F.silu(y)
    dy = torch.randn(y.shape, generator=g)
    rx, rg, rb = torch.autograd.grad(y, (xd, gd, bd), dy.double())
    dev = lambda t: t.to(device)  # noqa: E731
    yf, mr = T.gn_forward(dev(x), dev(gamma), dev(beta), 32, 1e-6, act)
    assert yf.shape == x.shape and _rel(yf, y.detach()) < 3e-6
    assert _rel(mr, T.gn_stats(dev(x), 32, 1e-6).cpu()) < 3e-6
    dgam, dbet = torch.empty(C, device=device), torch.empty(C, device=device)
    dx = T.gn_backward(dev(x), dev(dy), mr, dev(gamma), dev(beta), 32, act, dgam, dbet)
    assert dx.shape == x.shape
    assert _rel(dx, rx) < 1e-5 and _rel(dgam, rg) < 1e-5 and _rel(dbet, rb) < 1e-5, (_rel(dx, rx), _rel(dgam, rg), _rel(dbet, rb))


# ---- (c) 3-D, stride-1 k3 with H != W ---------------------------------------------------------------------------------------------

VOL_FORMS = {"mfma": (), "wino": ("wino",), "wino44": ("wino", "wino44"), "wino44h": ("wino", "wino44", "wino44h")}
# (family, B, Cin, Cout, D, H, W): every family at every slice it takes of (4, 8, 16), (3, 16, 32), (8, 32, 16), (1, 16, 64); the
# F(4x4) kernels need slices of >= 32 tiles (wino44) in 9 / 10 staging units (wino44h: 16 x 64 and 64 x 16 are the smallest)
CASES_3D = [
    ("mfma", 1, 128, 128, 4, 8, 16), ("mfma", 2, 128, 128, 3, 16, 32), ("mfma", 1, 128, 128, 8, 32, 16), ("mfma", 1, 128, 128, 1, 16, 64),
    ("wino", 1, 128, 128, 4, 8, 16), ("wino", 2, 128, 128, 3, 16, 32), ("wino", 1, 128, 128, 8, 32, 16), ("wino", 1, 64, 128, 1, 16, 64),
    ("wino44", 2, 64, 128, 3, 16, 32), ("wino44", 1, 64, 128, 8, 32, 16), ("wino44", 1, 64, 128, 1, 16, 64),
    ("wino44h", 1, 64, 128, 1, 16, 64), ("wino44h", 2, 64, 128, 3, 16, 64), ("wino44h", 1, 64, 128, 4, 64, 16),
]


def _vol(case, seed):
    family, B, Cin, Cout, D, H, W = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, D, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / math.sqrt(Cin * 27)
    b = torch.randn(Cout, generator=g)
    res = torch.randn(B, Cout, D, H, W, generator=g)
    return x, w, b, res


def _vol_forms(ops, w, family):
    pack = {"wino": ops.pack_wino3d_weight, "wino44": ops.pack_wino44_3d_weight, "wino44h": ops.pack_wino44h_3d_weight}
    kw = {n: pack[n](w) for n in VOL_FORMS[family]}
    assert all(v is not None for v in kw.values())
    return kw


@pytest.mark.parametrize("case", CASES_3D, ids=["-".join(map(str, c)) for c in CASES_3D])
def test_conv3d_family_on_non_cubic_volumes(device, case, monkeypatch):
    """Plain, and with the residual + ReLU epilogue of the VQ-VAE residual units (the MFMA kernel also with the input ReLU, as
    test_conv3d_depth_taps_with_relu_epilogues; the Winograd kernels take no input activation)."""
    monkeypatch.setenv("DDPM_CONV_WINO44", "2")
    from ddpm_ood_amd import ops

    family, B, Cin, Cout, D, H, W = case
    x, w, b, res = _vol(case, 17)
    d = lambda t: t.to(device)  # noqa: E731
    kw = _vol_forms(ops, d(w), family)
    tol = "f44" if family.startswith("wino44") else "f32"
    act = ops.ACT_RELU if family == "mfma" else ops.ACT_NONE
    ref = F.conv3d(x.double(), w.double(), b.double(), padding=1)
    y = _launch(lambda: ops.conv3d(d(x), d(w), d(b), **kw), family)
    _hold(f"3-D {family}", f"{case[1:]} plain", tol, y, ref)
    ref2 = F.relu(F.conv3d(F.relu(x.double()) if act else x.double(), w.double(), b.double(), padding=1) + res.double())
    y2 = _launch(lambda: ops.conv3d(d(x), d(w), d(b), act=act, out_act=ops.ACT_RELU, residual=d(res), **kw), family)
    _hold(f"3-D {family}", f"{case[1:]} relu", tol, y2, ref2)
    assert torch.equal(y2, ops.conv3d(d(x), d(w), d(b), act=act, out_act=ops.ACT_RELU, residual=d(res), **kw))


@pytest.mark.parametrize("taps", [3, 6])
def test_conv3d_wino44h_depth_taps_on_a_non_cubic_volume(device, taps, monkeypatch):
    """ddpm_conv_desc.depth_taps: a weight whose last (3) / first (6) depth tap is all zeros walks two taps."""
    monkeypatch.setenv("DDPM_CONV_WINO44", "2")
    from ddpm_ood_amd import ops

    case = ("wino44h", 1, 64, 128, 3, 64, 16)
    x, w, b, res = _vol(case, 19 + taps)
    w[:, :, 2 if taps == 3 else 0] = 0
    d = lambda t: t.to(device)  # noqa: E731
    kw = _vol_forms(ops, d(w), "wino44h")
    ref = F.relu(F.conv3d(x.double(), w.double(), b.double(), padding=1) + res.double())
    y = _launch(lambda: ops.conv3d(d(x), d(w), d(b), out_act=ops.ACT_RELU, residual=d(res), depth_taps=taps, **kw), "wino44h")
    _hold("3-D wino44h", f"depth_taps {taps}", "f44", y, ref)
    # all three taps walked: the skipped tap only ever adds exact zeros, so the same bits
    assert torch.equal(y, ops.conv3d(d(x), d(w), d(b), out_act=ops.ACT_RELU, residual=d(res), **kw))


# ---- (d) whole networks -------------------------------------------------------------------------------------------------------------

SMALL = dict(num_channels=(128, 256, 256), attention_levels=(False, False, True), num_res_blocks=1, num_head_channels=256)


def _unet_pair(device, channels, spatial_dims=2):
    import oracle
    from ddpm_ood_amd import DiffusionModelUNet
    from ddpm_ood_amd.synthetic import random_state_dict

    sd = random_state_dict(channels=channels, seed=1, config=SMALL, spatial_dims=spatial_dims)
    ref = oracle.DiffusionModelUNet(spatial_dims, channels, channels, **SMALL).eval()
    ref.load_state_dict(sd)
    hip = DiffusionModelUNet(spatial_dims, channels, channels, **SMALL)
    hip.load_state_dict(sd)
    return ref, hip.to(device).eval()


@pytest.mark.parametrize("channels,B,H,W", [(1, 2, 32, 64), (3, 3, 64, 32), (1, 2, 32, 48), (3, 1, 16, 40)])
def test_unet_forward_on_rectangles(device, channels, B, H, W, monkeypatch):
    """tests/test_gpu_unet.py::test_unet_forward_small with H != W; the attention level sees 8 x 16, 16 x 8, 8 x 12 and 4 x 10
    tokens (ragged and non-64-multiple token counts through the engine).  The (2, 32, 64) case also through the graphed forward."""
    ref, hip = _unet_pair(device, channels)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, channels, H, W, generator=g)
    t = torch.tensor([10, 650, 990][:B])
    with torch.no_grad():
        yr = ref(x, timesteps=t)
    yh = hip(x.to(device), timesteps=t.to(device))
    err = (yh.cpu() - yr).abs().max().item()
    _note("UNet forward", f"{(channels, B, H, W)}", err, 1e-4 * (1 + yr.abs().max().item()))
    assert yh.shape == yr.shape and math.isfinite(err) and err <= 1e-4 * (1 + yr.abs().max().item()), err
    assert yr.abs().max() > 0.05
    if (B, H, W) == (2, 32, 64):
        monkeypatch.setenv("DDPM_UNET_GRAPH", "1")
        graphed = [hip(x.to(device), timesteps=t.to(device)) for _ in range(3)]  # eager, capture, replay
        torch.cuda.synchronize()
        assert all(torch.equal(y, yh) for y in graphed)


def test_unet_forward_3d_on_a_non_cubic_volume(device):
    """tests/test_gpu_configs.py::test_unet_forward_3d_shallow_depth's comparison at (D, H, W) = (4, 8, 16)."""
    ref, hip = _unet_pair(device, 128, spatial_dims=3)
    x = torch.randn(2, 128, 4, 8, 16, generator=torch.Generator().manual_seed(12))
    t = torch.tensor([650, 30])
    with torch.no_grad():
        yr = ref(x, timesteps=t)
    yh = hip(x.to(device), timesteps=t.to(device)).cpu()
    err = (yh - yr).abs().max().item()
    _note("UNet forward 3-D", "(2, 128, 4, 8, 16)", err, 1e-4 * (1 + yr.abs().max().item()))
    assert yh.shape == yr.shape and err <= 1e-4 * (1 + yr.abs().max().item()), err
    assert yr.abs().max() > 0.05


def test_vqvae_on_a_non_cubic_volume(device):
    """tests/test_gpu_ops.py::test_vqvae_residual_units_on_hip_match_torch on a (16, 32, 48) volume: encode -> quantise -> decode."""
    from oracle.vqvae import VQVAE as OV
    from ddpm_ood_amd.vqvae import VQVAE as PV

    cfg = dict(spatial_dims=3, in_channels=1, out_channels=1, num_channels=(128, 128), num_res_layers=2,
               num_res_channels=(128, 128), downsample_parameters=((2, 4, 1, 1), (2, 4, 1, 1)),
               upsample_parameters=((2, 4, 1, 1, 0), (2, 4, 1, 1, 0)), num_embeddings=32, embedding_dim=128)
    torch.manual_seed(1)
    o = OV(**cfg).eval()
    with torch.no_grad():
        o.quantizer.quantizer.embedding.weight.mul_(3.0)
    p = PV(**cfg)
    p.load_state_dict(o.state_dict())
    p = p.to(device).eval()
    x = torch.rand(1, 1, 16, 32, 48, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        zo = o.encode_stage_2_inputs(x)
        zp = p.encode_stage_2_inputs(x.to(device))
        assert tuple(zp.shape) == tuple(zo.shape) == (1, 128, 4, 8, 12)
        for what, got, want, tol in (("encode", zp, zo, 1e-5), ("decode", p.decode_stage_2_outputs(zp), o.decode_stage_2_outputs(zo), 2e-5)):
            err, bound = (got.cpu().double() - want.double()).abs().max().item(), tol * (1 + want.abs().max().item())
            _note("VQ-VAE", what, err, bound)
            assert got.shape == want.shape and math.isfinite(err) and err <= bound, (what, err, bound)


@pytest.mark.parametrize("channels,shape,B,dims", [(3, (32, 64), 4, 2), (128, (4, 8, 16), 4, 3)])
def test_native_step_matches_aten_autograd_on_rectangles(device, channels, shape, B, dims):
    """tests/test_gpu_train.py::test_native_step_matches_aten_autograd_on_other_unets' comparison (loss 2e-5, every parameter
    gradient 1e-4 of the larger of its own scale and 1e-5 of the model's largest) for the `small` UNet on 32 x 64 images and on
    (4, 8, 16) latents."""
    from ddpm_ood_amd import DiffusionModelUNet
    from ddpm_ood_amd.synthetic import random_state_dict
    from ddpm_ood_amd.train import unet_forward_torch
    from ddpm_ood_amd.train_native import NativeUNetStep
    from ddpm_ood_amd.trainer import MODEL_CONFIGS

    sd = random_state_dict("small", channels, spatial_dims=dims, seed=1)
    g = torch.Generator().manual_seed(5)
    full = (B, channels) + shape
    x = torch.rand(full, generator=g).to(device)
    t = torch.randint(0, 1000, (B,), generator=g).to(device)
    noise = torch.randn(full, generator=g).to(device)

    def build():
        m = DiffusionModelUNet(dims, channels, channels, **MODEL_CONFIGS["small"])
        m.load_state_dict(sd)
        return m.to(device).train()

    ref = build()
    for p in ref.parameters():
        p.requires_grad_(True)
    loss_r = torch.nn.functional.mse_loss(unet_forward_torch(ref, x, t), noise)
    loss_r.backward()
    hip = build()
    with torch.no_grad():
        loss_h = NativeUNetStep(hip).loss_and_grads(x, t, noise)
    assert abs(loss_h.item() - loss_r.item()) <= 2e-5 * abs(loss_r.item())
    pr, ph = dict(ref.named_parameters()), dict(hip.named_parameters())
    gmax = max(float(p.grad.abs().max()) for p in pr.values() if p.grad is not None)
    worst = 0.0
    for k in pr:
        if pr[k].grad is None:
            assert float(ph[k].grad.abs().max()) == 0.0, k
            continue
        rel = float((ph[k].grad - pr[k].grad).abs().max() / max(float(pr[k].grad.abs().max()), 1e-5 * gmax))
        worst = max(worst, rel)
        assert rel <= 1e-4, (k, rel)
    _note("native step", f"{full}", worst, 1e-4)


def test_trajectory_with_a_rectangular_image_roi(device, tmp_path):
    """tests/test_gpu_configs.py::test_ragged_batches_first_n_drop_last_and_roi's oracle-against-HIP rows with a rectangular
    --image_roi on its 40 x 40 synthetic source.  --image_roi 32 24 crops as asked, but no LPIPS-AlexNet score exists for a
    24-wide image: conv1 (k11 s4 p2) leaves 5 columns, the first MaxPool2d(3, 2) 2, and the second has no output (an extent
    needs >= 31; the reference only pads 28 x 28).  torch refuses it ("Output size is too small") and so does the HIP path;
    the rows are compared at 32 x 40."""
    import oracle
    from parity_util import assert_rows_close, hip_scores, loader_for, make_args, oracle_scores, write_checkpoint
    from ddpm_ood_amd import synthetic
    from ddpm_ood_amd.trainer import MODEL_CONFIGS, Reconstruct

    tiny = "synthetic:blobs:n=1:channels=1:size=8"
    args = make_args(tmp_path, model_type="small", is_grayscale=1, spatial_dimension=2, batch_size=2, validation_ids=tiny, in_ids=tiny)
    sd = synthetic.random_state_dict("small", 1, spatial_dims=2, seed=1)
    write_checkpoint(tmp_path, args, sd)
    rec = Reconstruct(args)
    rec.quiet = True
    ref = oracle.DiffusionModelUNet(2, 1, 1, **MODEL_CONFIGS["small"], use_proj_attn=bool(getattr(args, "use_proj_attn", 0))).eval()
    ref.load_state_dict(sd)
    big = "synthetic:blobs:n=2:size=40:seed=34"
    args.image_roi = (32, 24)
    narrow = next(iter(loader_for(args, big)))["image"]
    assert narrow.shape == (2, 1, 32, 24)
    pl = oracle.PerceptualLoss(dimensions=2, include_pixel_loss=False, is_fake_3d=False, lpips_normalize=True)
    with pytest.raises(RuntimeError, match="too small"):
        pl(narrow, narrow.flip(0))
    with pytest.raises(ValueError, match="maxpool3s2"):
        hip_scores(args, rec, big, "in")
    args.image_roi = (32, 40)
    assert next(iter(loader_for(args, big)))["image"].shape == (2, 1, 32, 40)
    assert_rows_close(hip_scores(args, rec, big, "in"), oracle_scores(args, rec, big, "in", model=ref), 2e-4, "rectangular roi")
