"""Thin Python wrappers over the stand-alone C-ABI operators (include/ddpm_ood_hip.h).

Used by the scheduler / trainer mirrors and by the per-kernel parity tests.  Every function
takes ROCm device tensors and launches on torch's current HIP stream; none falls back to
PyTorch ops.
"""

from __future__ import annotations

import ctypes as C
from ctypes import byref as C_byref

import numpy as np
import torch

from . import _lib
from ._lib import ConvDesc, check, ptr, require_device_f32, stream_ptr

CONV_NORMAL, CONV_STRIDE2, CONV_UPSAMPLE2 = 0, 1, 2
ACT_NONE, ACT_SILU, ACT_RELU = 0, 1, 2


def _kernel_is(w, kshape) -> bool:
    """Is w a [Cout, Cin, *kshape] weight?  (None in kshape: any extent; kshape None: any weight; (1, 1) also takes [out, in].)"""
    if kshape is None or (kshape == (1, 1) and w.ndim != 4):
        return True
    return w.ndim == 2 + len(kshape) and all(k is None or k == e for k, e in zip(kshape, w.shape[2:]))


def _pack(what, weight, kshape, size_fn, pack_fn, dtype=torch.float32, *, ksize_arg=False, member_args=False, zeros=False,
          numel=None, size_first=False):
    """The one pattern of the weight packers below: check the kernel shape -> ask lib.<size_fn>(Cout, Cin[, k]) (0: None) ->
    allocate `numel(n)` (default n) elements -> lib.<pack_fn>(w, out, Cout, Cin[, k][, 0, Cout], stream).  member_args: the packer
    takes (cout_offset, Cout_total) of a fused member; size_first: the size is asked before the shape is looked at."""
    lib = _lib.load()
    w = require_device_f32(weight, "weight")
    if not size_first and not _kernel_is(w, kshape):
        return None
    dims = (w.shape[0], w.shape[1]) + (((w.shape[2] if w.ndim == 4 else 1),) if ksize_arg else ())
    n = getattr(lib, size_fn)(*dims)
    if n == 0 or (size_first and not _kernel_is(w, kshape)):
        return None
    out = (torch.zeros if zeros else torch.empty)(numel(n) if numel else n, dtype=dtype, device=w.device)
    member = (0, w.shape[0]) if member_args else ()
    check(getattr(lib, pack_fn)(ptr(w), ptr(out), *dims, *member, stream_ptr()), what)
    return out


def pack_conv_weight(weight: torch.Tensor) -> torch.Tensor | None:
    """torch [Cout, Cin, k, k] (or [out, in]) -> MFMA-packed weight, or None if unpackable."""
    return _pack("pack_conv_weight", weight, None, "ddpm_packed_conv_weight_floats", "ddpm_pack_conv_weight_f32", ksize_arg=True,
                 member_args=True)


def pack_wino44_weight(weight: torch.Tensor) -> torch.Tensor | None:
    """torch [Cout, Cin, 3, 3] -> F(4x4, 3x3) Winograd-domain weights (6 x 6 positions) in the MFMA layout."""
    return _pack("pack_wino44_weight", weight, (3, 3), "ddpm_wino44_weight_floats", "ddpm_pack_wino44_weight_f32")


def pack_wino_weight(weight: torch.Tensor) -> torch.Tensor | None:
    """torch [Cout, Cin, 3, 3] -> Winograd-domain weights U = G g G^T in the MFMA layout (None if unsupported)."""
    return _pack("pack_wino_weight", weight, (3, 3), "ddpm_wino_weight_floats", "ddpm_pack_wino_weight_f32")


def fold_upsample_weight(weight: torch.Tensor) -> torch.Tensor | None:
    """torch [Cout, Cin, 3, 3] of an Upsample conv -> the 4 folded 2x2-tap weights (None if not foldable)."""
    return _pack("fold", weight, (3, None), "ddpm_folded_upsample_weight_floats", "ddpm_fold_upsample_weight_f32", size_first=True)


def pack_wino44h_weight(weight: torch.Tensor) -> torch.Tensor | None:
    """torch [Cout, Cin, 3, 3] -> F(4x4, 3x3) Winograd-domain weights as split-f16 planes (hi = f16(2^10 U), lo = the
    remainder) in the order conv_wino44h.hip's LDS-DMA lands them; None without a tiling (Cout % 64, Cin % 16)."""
    return _pack("pack_wino44h_weight", weight, (3, 3), "ddpm_wino44h_weight_halves", "ddpm_pack_wino44h_weight", torch.float16)


def pack_conv1x1_h_weight(w):
    """[Cout, Cin(, 1, 1)] -> the pre-split f16 planes of the DMA-fed 1x1 kernel (conv1x1_dma.hip), or None if Cout % 128 or
    Cin % 16.  Pass it as conv(..., wino44h=...) of a 1x1 convolution."""
    return _pack("pack_conv1x1_h_weight", w, (1, 1), "ddpm_conv1x1_h_weight_halves", "ddpm_pack_conv1x1_h_weight", torch.float16)


def pack_conv_d3h_weight(w):
    """[Cout, Cin, 3, 3] -> split-f16 planes of the direct 3x3 kernel (conv_d3s.hip), or None (Cout % 128, Cin % 8).  Pass it as
    conv(..., d3h=...)."""
    return _pack("pack_conv_d3h_weight", w, (3, 3), "ddpm_conv_d3h_weight_halves", "ddpm_pack_conv_d3h_weight", torch.float16)


def pack_conv_d1s_weight(w):
    """[Cout, Cin, 1, 1] (or [Cout, Cin]) -> split-f16 planes of the small-launch 1x1 kernel (conv_d3s.hip), or None (Cout % 64,
    Cin % 128).  Pass it as conv(..., d3h=...) of a 1x1 convolution."""
    return _pack("pack_conv_d1s_weight", w, (1, 1), "ddpm_conv_d1s_weight_halves", "ddpm_pack_conv_d1s_weight", torch.float16,
                 member_args=True, zeros=True)


def pack_conv_s2h_weight(w):
    """[Cout, Cin, 3, 3] -> split-f16 planes of the direct stride-2 kernel (conv_s2h.hip), or None if the shape has no tiling.
    Pass it as conv(..., mode=CONV_STRIDE2, wino44h=...)."""
    return _pack("pack_conv_s2h_weight", w, (3, 3), "ddpm_conv_s2h_weight_halves", "ddpm_pack_conv_s2h_weight", torch.float16)


def conv(x, weight, bias=None, *, x2=None, gscale=None, gshift=None, act=ACT_NONE, mode=CONV_NORMAL,
         chan_add=None, chan_add_offset=0, residual=None, packed=None, force_direct=False, folded=None,
         wino=None, out_act=ACT_NONE, wino44=None, wino44h=None, want_stats=False, d3h=None):
    """Fused conv / linear.  x: [B, C1, H, W]; x2: optional second source of a virtual concat.
    want_stats: return (out, stats) with the produced tensor's per-channel GroupNorm statistics (ddpm_conv_desc.stats_out)."""
    lib = _lib.load()
    x = require_device_f32(x, "x")
    w = require_device_f32(weight, "weight")
    if x.ndim == 2:  # Linear: [B, C] == [B, C, 1, 1]
        x = x[:, :, None, None]
        was_linear = True
    else:
        was_linear = False
    B, C1, Hi, Wi = x.shape
    cout = w.shape[0]
    k = w.shape[2] if w.ndim == 4 else 1
    if mode == CONV_STRIDE2:
        Ho, Wo = (Hi + 1) // 2, (Wi + 1) // 2
    elif mode == CONV_UPSAMPLE2:
        Ho, Wo = 2 * Hi, 2 * Wi
    else:
        Ho, Wo = Hi, Wi
    if packed is False:  # the caller supplies the Winograd weights of a launch that takes them: no direct-MFMA form (the
        packed = None    # dispatcher's last resort is then the plain direct kernel on the raw weights)
    elif packed is None and not force_direct:
        packed = pack_conv_weight(w)
    out = torch.empty((B, cout, Ho, Wo), dtype=torch.float32, device=x.device)
    keep = [x, w, out, packed]
    d = ConvDesc()
    d.in1 = ptr(x)
    d.C1 = C1
    if x2 is not None:
        x2 = require_device_f32(x2, "x2")
        d.in2, d.C2 = ptr(x2), x2.shape[1]
        keep.append(x2)
    d.w_packed = ptr(packed)
    d.w_raw = ptr(w)
    if bias is not None:
        bias = require_device_f32(bias, "bias")
        d.bias = ptr(bias)
    if gscale is not None:
        gscale = require_device_f32(gscale, "gscale")
        gshift = require_device_f32(gshift, "gshift")
        d.gscale, d.gshift = ptr(gscale), ptr(gshift)
    if chan_add is not None:
        chan_add = require_device_f32(chan_add, "chan_add")
        d.chan_add = chan_add.data_ptr() + 4 * chan_add_offset
        d.chan_add_stride = chan_add.shape[1]
    if residual is not None:
        residual = require_device_f32(residual, "residual")
        d.residual = ptr(residual)
    d.out = ptr(out)
    d.B, d.Cout, d.Hi, d.Wi, d.Ho, d.Wo = B, cout, Hi, Wi, Ho, Wo
    d.ksize, d.mode, d.act, d.force_direct = k, mode, act, int(force_direct)
    d.w_folded = ptr(folded)
    d.w_wino = ptr(wino)
    d.w_wino44 = ptr(wino44)
    d.w_wino44h = wino44h.data_ptr() if wino44h is not None else None
    d.w_d3h = d3h.data_ptr() if d3h is not None else None
    d.out_act = out_act
    need = lib.ddpm_conv_scratch_floats(C.byref(d))  # small batches: split-K partial slabs (0 otherwise)
    if need:
        scratch = torch.empty(need, dtype=torch.float32, device=x.device)
        keep.append(scratch)
        d.scratch, d.scratch_floats = ptr(scratch), need
    stats = None
    if want_stats:  # GroupNorm statistics of the produced tensor from the epilogue: [B, Cout, parts, 2] (None: not emitted)
        parts = lib.ddpm_conv_stats_parts(C.byref(d))
        if parts > 0:
            stats = torch.empty((B, cout, parts, 2), dtype=torch.float32, device=x.device)
            d.stats_out = ptr(stats)
    check(lib.ddpm_conv_f32(C.byref(d), stream_ptr()), "conv")
    if want_stats:
        return out, stats
    return out[:, :, 0, 0] if was_linear else out


def conv_takes_wino44h(x_shape, cout: int) -> bool:
    """Would conv() run a plain stride-1 3x3 convolution of an input of this shape ([B, Cin, H, W]) to `cout` channels on the
    split-f16 F(4x4) kernel, given its packed weights?  (ddpm_conv_takes_wino44h: the dispatcher's own rule.)"""
    B, cin, H, W = x_shape
    d = ConvDesc()
    d.C1, d.B, d.Cout, d.Hi, d.Wi, d.Ho, d.Wo = cin, B, cout, H, W, H, W
    d.ksize, d.mode, d.act, d.out_act = 3, CONV_NORMAL, ACT_NONE, ACT_NONE
    return bool(_lib.load().ddpm_conv_takes_wino44h(C.byref(d)))


CONV_TRANSPOSE2 = 3
WINO_MAX_TENSOR_BYTES = 2 ** 31 - 1  # 32-bit buffer offsets of the Winograd kernels


def conv3d_supported(weight: torch.Tensor, stride: int = 1, transposed: bool = False) -> bool:
    """Does this conv3d / conv_transpose3d weight have an MFMA tiling?  k3 s1 p1 and k4 s2 p1 need Cin % 4 == 0 and
    Cout % 128 == 0; the transposed k4 s2 p1 (weight [Cin, Cout, 4, 4, 4]) needs Cin % 8 == 0 and Cout % 128 == 0."""
    if weight.ndim != 5:
        return False
    k = tuple(weight.shape[2:])
    if transposed:
        return k == (4, 4, 4) and stride == 2 and weight.shape[0] % 8 == 0 and weight.shape[1] % 128 == 0
    if not ((k == (3, 3, 3) and stride in (1, 2)) or (k == (4, 4, 4) and stride == 2)):
        return False
    return weight.shape[0] % 128 == 0 and weight.shape[1] % 4 == 0


def pack_conv3d_weight(weight: torch.Tensor) -> torch.Tensor:
    """torch [Cout, Cin, k, k, k] (k = 3 or 4) -> k MFMA-packed slabs of k x k taps, one per depth tap."""
    lib = _lib.load()
    w = require_device_f32(weight, "weight")
    cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
    out = torch.empty(cout * cin * k ** 3, dtype=torch.float32, device=w.device)
    check(lib.ddpm_pack_conv3d_weight_f32(ptr(w), ptr(out), cout, cin, k, stream_ptr()), "pack_conv3d_weight")
    return out


def pack_wino3d_weight(weight: torch.Tensor) -> torch.Tensor | None:
    """torch [Cout, Cin, 3, 3, 3] -> per-depth-tap Winograd-domain weights U_kd = G w[:, :, kd] G^T (None if the
    shape has no Winograd tiling: Cout % 64, Cin % 8)."""
    return _pack("pack_wino3d_weight", weight, (3, 3, 3), "ddpm_wino_weight_floats", "ddpm_pack_wino3d_weight_f32",
                 numel=lambda n: 3 * n)


def pack_wino44_3d_weight(weight: torch.Tensor) -> torch.Tensor | None:
    """torch [Cout, Cin, 3, 3, 3] -> per-depth-tap F(4x4, 3x3) weights U_kd = G w[:, :, kd] G^T, 6 x 6 (None if the shape
    has no tiling: Cout % 64, Cin % 8)."""
    return _pack("pack_wino44_3d_weight", weight, (3, 3, 3), "ddpm_wino44_weight_floats", "ddpm_pack_wino44_weight3d_f32",
                 numel=lambda n: 3 * n)


def pack_convT_weight(weight: torch.Tensor) -> torch.Tensor:
    """torch ConvTranspose weight [Cin, Cout, 4, 4(, 4)] -> per-output-parity 2 x 2 (x 2)-tap packed weights."""
    lib = _lib.load()
    w = require_device_f32(weight, "weight")
    cin, cout, dims = w.shape[0], w.shape[1], w.ndim - 2
    n = lib.ddpm_packed_convtr_weight_floats(cout, cin, dims)
    if n == 0 or tuple(w.shape[2:]) != (4,) * dims:
        raise ValueError("pack_convT_weight: needs a [Cin % 8 == 0, Cout % 128 == 0, 4, 4(, 4)] weight")
    out = torch.empty(n, dtype=torch.float32, device=w.device)
    check(lib.ddpm_pack_convtr_weight_f32(ptr(w), ptr(out), cin, cout, dims, stream_ptr()), "pack_convT_weight")
    return out


def pack_wino44h_3d_weight(weight: torch.Tensor) -> torch.Tensor | None:
    """torch [Cout, Cin, 3, 3, 3] -> split-f16 F(4x4, 3x3) planes per depth tap (conv_wino44h.hip, 3-D form)."""
    return _pack("pack_wino44h_3d_weight", weight, (3, 3, 3), "ddpm_wino44h_weight_halves", "ddpm_pack_wino44h_weight3d",
                 torch.float16, numel=lambda n: 3 * (n - 64) + 64)  # the 64 trailing slots (scales) once, behind the three slabs


def conv3d(x, weight, bias=None, *, act=ACT_NONE, out_act=ACT_NONE, residual=None, packed=None, stride: int = 1,
           wino=None, out=None, wino44=None, wino44h=None, chan_add=None, depth_taps: int = 0):
    """F.conv3d(act(x), weight, bias, stride, padding=1) (+ chan_add[n, co] + residual, + output activation) on NCDHW tensors:
    kernel 3 stride 1 or 2 (the 3-D UNet's ResnetBlock / Downsample convolutions), or kernel 4 stride 2 (the VQ-VAE's).  ONE launch of the MFMA kernel: the depth taps are part of its chunk
    stream (chunk = (depth tap, channel group)), so the output is written once.  ``wino`` (pack_wino3d_weight): a
    stride-1 conv without input activation whose slices hold >= 64 2x2 tiles takes the Winograd kernel instead (2-D
    F(2x2, 3x3) per depth tap, the taps accumulated in the transform domain: 2.25x fewer multiplies); ``wino44``
    (pack_wino44_3d_weight): F(4x4, 3x3) per depth tap where a slice holds >= 32 4x4 tiles and the launch fills the chip."""
    lib = _lib.load()
    x = require_device_f32(x, "x")
    w = require_device_f32(weight, "weight")
    if not conv3d_supported(w, stride):
        raise ValueError("conv3d: only k3 s1 / k4 s2 weights with Cin % 4 == 0 and Cout % 128 == 0 have an MFMA tiling")
    B, Cc, D, H, W = x.shape
    cout, k = w.shape[0], w.shape[2]
    if Cc != w.shape[1]:
        raise ValueError(f"conv3d: input has {Cc} channels, weight expects {w.shape[1]}")
    if stride == 2 and (D < 2 or H < 2 or W < 2):
        raise ValueError("conv3d k4 s2: every extent must be >= 2")
    if stride == 1:
        Do, Ho, Wo = D, H, W
    elif k == 3:
        Do, Ho, Wo = (D + 1) // 2, (H + 1) // 2, (W + 1) // 2
    else:
        Do, Ho, Wo = D // 2, H // 2, W // 2
    if packed is None:
        packed = pack_conv3d_weight(w)
    if out is None:
        out = torch.empty((B, cout, Do, Ho, Wo), dtype=torch.float32, device=x.device)
    if bias is not None:
        bias = require_device_f32(bias, "bias")
    if residual is not None:
        residual = require_device_f32(residual, "residual")
    if (wino is not None or wino44 is not None or wino44h is not None) and stride == 1 and B > 1:
        # the Winograd kernel addresses pixels with 32-bit buffer offsets (tensors < 2 GiB): a larger batch is walked
        # in sub-batches (views along dim 0, no copies) instead of dropping to the direct kernel
        per = max(Cc, cout) * D * H * W * 4
        nb = max(1, WINO_MAX_TENSOR_BYTES // per)
        if B > nb:
            for s0 in range(0, B, nb):
                conv3d(x[s0:s0 + nb], w, bias, act=act, out_act=out_act, packed=packed, stride=stride, wino=wino,
                       wino44=wino44, wino44h=wino44h, residual=None if residual is None else residual[s0:s0 + nb],
                       out=out[s0:s0 + nb], chan_add=None if chan_add is None else chan_add[s0:s0 + nb], depth_taps=depth_taps)
            return out
    d = ConvDesc()
    d.in1, d.C1 = ptr(x), Cc
    d.w_packed = ptr(packed)
    d.bias, d.residual, d.out = ptr(bias), ptr(residual), ptr(out)
    d.B, d.Cout, d.Hi, d.Wi, d.Ho, d.Wo = B, cout, H, W, Ho, Wo
    d.ksize, d.mode, d.act, d.out_act = k, (CONV_NORMAL if stride == 1 else CONV_STRIDE2), act, out_act
    d.Di, d.Do, d.dims = D, Do, 3
    d.depth_taps = depth_taps  # 3 / 6: the first / last depth tap of the weight is all zeros (conv_transpose_parity)
    if chan_add is not None:
        chan_add = require_device_f32(chan_add, "chan_add")
        d.chan_add, d.chan_add_stride = ptr(chan_add), chan_add.shape[1]
    if wino is not None and stride == 1:
        d.w_wino = ptr(wino)
    if wino44 is not None and stride == 1:
        d.w_wino44 = ptr(wino44)
    if wino44h is not None and stride == 1:
        d.w_wino44h = wino44h.data_ptr()
    need = lib.ddpm_conv_scratch_floats(C_byref(d))  # launches smaller than the chip: split-K partial slabs
    if need:
        scratch = torch.empty(need, dtype=torch.float32, device=x.device)
        d.scratch, d.scratch_floats = ptr(scratch), need
    check(lib.ddpm_conv_f32(C_byref(d), stream_ptr()), "conv3d")
    return out


def conv_transpose(x, weight, bias=None, *, out_act=ACT_NONE, packed=None):
    """F.conv_transpose{2,3}d(x, weight, bias, stride=2, padding=1) (+ output activation) for kernel 4: one launch,
    grid.z = output parity, each parity a 2 x 2 (x 2)-tap convolution over the input."""
    lib = _lib.load()
    x = require_device_f32(x, "x")
    w = require_device_f32(weight, "weight")
    dims = x.ndim - 2
    if w.ndim != x.ndim or x.shape[1] != w.shape[0]:
        raise ValueError(f"conv_transpose: input {tuple(x.shape)} does not match weight {tuple(w.shape)}")
    if packed is None:
        packed = pack_convT_weight(w)
    B, Cc = x.shape[:2]
    D, H, W = ((1,) + tuple(x.shape[2:])) if dims == 2 else tuple(x.shape[2:])
    cout = w.shape[1]
    out = torch.empty((B, cout) + tuple(2 * e for e in x.shape[2:]), dtype=torch.float32, device=x.device)
    if bias is not None:
        bias = require_device_f32(bias, "bias")
    d = ConvDesc()
    d.in1, d.C1 = ptr(x), Cc
    d.w_packed = ptr(packed)
    d.bias, d.out = ptr(bias), ptr(out)
    d.B, d.Cout, d.Hi, d.Wi, d.Ho, d.Wo = B, cout, H, W, 2 * H, 2 * W
    d.ksize, d.mode, d.out_act = 4, CONV_TRANSPOSE2, out_act
    if dims == 3:
        d.Di, d.Do, d.dims = D, 2 * D, 3
    check(lib.ddpm_conv_f32(C_byref(d), stream_ptr()), "conv_transpose")
    return out


def conv_transpose_parity_supported(x, weight) -> bool:
    """ConvTranspose3d k4 s2 p1 whose eight parity convolutions (3x3x3 over the INPUT grid) have the split-f16 F(4x4) tiling:
    slices of at least 32 4x4 tiles in whole tile rows, channel counts with an MFMA tiling."""
    if x.ndim != 5 or weight.ndim != 5 or tuple(weight.shape[2:]) != (4, 4, 4):
        return False
    cin, cout = weight.shape[0], weight.shape[1]
    D, H, W = x.shape[2:]
    if D < 2 or H % 4 or W % 4 or cin % 16 or cout % 128:
        return False
    twc, thr = W // 4, H // 4
    tr = 32 // twc if twc and 32 % twc == 0 else 0  # tile rows per item
    # (the kernel's item: 32 tiles in whole tile rows, its 4 tr + 2 staged rows inside the slice)
    return tr > 0 and thr % tr == 0 and H >= 4 * tr + 2 and W <= 64


def pack_convT_parity_weights(weight):
    """[Cin, Cout, 4, 4, 4] -> per output parity q = 4 qz + 2 qy + qx: (the 3x3x3 weight [Cout, Cin, 3, 3, 3], its MFMA-packed form,
    its split-f16 F(4x4) planes)."""
    lib = _lib.load()
    w = require_device_f32(weight, "weight")
    cin, cout = w.shape[0], w.shape[1]
    g = torch.empty((8, cout, cin, 3, 3, 3), dtype=torch.float32, device=w.device)
    check(lib.ddpm_convtr3d_parity_weights_f32(ptr(w), ptr(g), cin, cout, stream_ptr()), "convtr3d_parity_weights")
    return [(g[q], pack_conv3d_weight(g[q]), pack_wino44h_3d_weight(g[q])) for q in range(8)]


def conv_transpose_parity(x, parity_weights, bias=None, *, out_act=ACT_NONE, sub_batch: int = 8):
    """F.conv_transpose3d(x, w, bias, stride 2, padding 1) (+ ReLU) as eight stride-1 3x3x3 convolutions -- each on the split-f16
    F(4x4) kernel, walking only its two non-zero depth taps -- and one interleave pass; `sub_batch` volumes at a time so that
    the eight parity tensors stay a bounded scratch (8 x the input extent x Cout)."""
    lib = _lib.load()
    x = require_device_f32(x, "x")
    B, _, D, H, W = x.shape
    cout = parity_weights[0][0].shape[0]
    out = torch.empty((B, cout, 2 * D, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    for s0 in range(0, B, sub_batch):
        xb = x[s0:s0 + sub_batch]
        nb = xb.shape[0]
        tmp = torch.empty((8, nb, cout, D, H, W), dtype=torch.float32, device=x.device)
        for q, (g, packed, w44h) in enumerate(parity_weights):
            conv3d(xb, g, bias, out_act=out_act, packed=packed, wino44h=w44h, out=tmp[q], depth_taps=6 if q & 4 else 3)
        check(lib.ddpm_parity_interleave3_f32(ptr(tmp), ptr(out[s0:s0 + nb]), nb * cout, D, H, W, stream_ptr()), "parity_interleave3")
    return out


def convnd_generic(x, weight, bias=None, *, stride=1, padding=1, transposed=False, residual=None, relu=False):
    """Generic (transposed) conv2d / conv3d on the HIP library for shapes without an MFMA tiling (any channel counts):
    x [B, Cin, (D,) H, W], torch weight layout, symmetric kernel / stride / padding, output_padding 0."""
    lib = _lib.load()
    x = require_device_f32(x, "x")
    w = require_device_f32(weight, "weight")
    dims = x.ndim - 2
    if dims not in (2, 3) or w.ndim != x.ndim or len(set(w.shape[2:])) != 1:
        raise ValueError("convnd_generic: needs x [B, C, (D,) H, W] and a cubic / square kernel")
    k = w.shape[2]
    cin, cout = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    if x.shape[1] != cin:
        raise ValueError(f"convnd_generic: input has {x.shape[1]} channels, weight expects {cin}")
    ext = (lambda e: (e - 1) * stride - 2 * padding + k) if transposed else (lambda e: (e + 2 * padding - k) // stride + 1)
    out = torch.empty((x.shape[0], cout) + tuple(ext(e) for e in x.shape[2:]), dtype=torch.float32, device=x.device)
    if bias is not None:
        bias = require_device_f32(bias, "bias")
    if residual is not None:
        residual = require_device_f32(residual, "residual")
        if residual.shape != out.shape:
            raise ValueError("convnd_generic: residual shape")
    D, H, W = (1,) * (3 - dims) + tuple(x.shape[2:])
    check(lib.ddpm_convnd_generic_f32(ptr(x), ptr(w), ptr(bias), ptr(residual), ptr(out), x.shape[0], cin, cout, D, H, W, dims, k,
                                      stride, padding, int(transposed), int(relu), stream_ptr()), "convnd_generic")
    return out


def conv3d_k4s2_cin1(x, weight, bias=None, relu: bool = False):
    """First VQ-VAE encoder layer: relu?(F.conv3d(x[B, 1, D, H, W], weight[Cout, 1, 4, 4, 4], bias, stride 2, pad 1))."""
    lib = _lib.load()
    x = require_device_f32(x, "x")
    w = require_device_f32(weight, "weight")
    if x.ndim != 5 or x.shape[1] != 1 or tuple(w.shape[1:]) != (1, 4, 4, 4):
        raise ValueError("conv3d_k4s2_cin1: needs x [B, 1, D, H, W] and weight [Cout, 1, 4, 4, 4]")
    B, _, D, H, W = x.shape
    out = torch.empty((B, w.shape[0], D // 2, H // 2, W // 2), dtype=torch.float32, device=x.device)
    if bias is not None:
        bias = require_device_f32(bias, "bias")
    check(lib.ddpm_conv3d_k4s2_cin1_f32(ptr(x), ptr(w), ptr(bias), ptr(out), B, w.shape[0], D, H, W, int(relu),
                                        stream_ptr()), "conv3d_k4s2_cin1")
    return out


def convT3d_k4s2_cout1(x, weight, bias=None):
    """Last VQ-VAE decoder layer: F.conv_transpose3d(x[B, Cin, D, H, W], weight[Cin, 1, 4, 4, 4], bias, stride 2, pad 1)."""
    lib = _lib.load()
    x = require_device_f32(x, "x")
    w = require_device_f32(weight, "weight")
    if x.ndim != 5 or tuple(w.shape) != (x.shape[1], 1, 4, 4, 4):
        raise ValueError("convT3d_k4s2_cout1: needs x [B, Cin, D, H, W] and weight [Cin, 1, 4, 4, 4]")
    B, Cc, D, H, W = x.shape
    out = torch.empty((B, 1, 2 * D, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    if bias is not None:
        bias = require_device_f32(bias, "bias")
    check(lib.ddpm_convtr3d_k4s2_cout1_f32(ptr(x), ptr(w), ptr(bias), ptr(out), B, Cc, D, H, W, stream_ptr()),
          "convT3d_k4s2_cout1")
    return out


def gn_scale_shift(x, gamma, beta, groups: int, eps: float, x2=None):
    lib = _lib.load()
    x = require_device_f32(x, "x")
    B, C1 = x.shape[:2]
    hw = x[0, 0].numel()
    C2 = 0
    if x2 is not None:
        x2 = require_device_f32(x2, "x2")
        C2 = x2.shape[1]
    gamma = require_device_f32(gamma, "gamma")
    beta = require_device_f32(beta, "beta")
    scale = torch.empty((B, C1 + C2), dtype=torch.float32, device=x.device)
    shift = torch.empty_like(scale)
    check(lib.ddpm_gn_scale_shift_f32(ptr(x), ptr(x2), C1, C2, ptr(gamma), ptr(beta), ptr(scale), ptr(shift), B, hw,
                                      groups, eps, stream_ptr()), "gn_scale_shift")
    return scale, shift


def gn_finalize(stats, gamma, beta, groups: int, eps: float, hw: int, stats2=None):
    """scale / shift of F.group_norm from per-channel statistics slabs [B, C, parts, 2] = {mean, M2} per slice (the
    `stats` of conv(..., want_stats=True) or channel_stats); stats2: second source of a virtual concat."""
    lib = _lib.load()
    stats = require_device_f32(stats, "stats")
    B, C1, parts1, _ = stats.shape
    C2 = parts2 = 0
    if stats2 is not None:
        stats2 = require_device_f32(stats2, "stats2")
        _, C2, parts2, _ = stats2.shape
    gamma = require_device_f32(gamma, "gamma")
    beta = require_device_f32(beta, "beta")
    scale = torch.empty((B, C1 + C2), dtype=torch.float32, device=stats.device)
    shift = torch.empty_like(scale)
    check(lib.ddpm_gn_finalize_f32(ptr(stats), parts1, C1, ptr(stats2), parts2, C2, ptr(gamma), ptr(beta), ptr(scale),
                                   ptr(shift), B, hw, groups, eps, stream_ptr()), "gn_finalize")
    return scale, shift


def channel_stats(x):
    """[B, C, 1, 2] = per-channel {mean, sum of squared deviations} of x [B, C, ...]."""
    lib = _lib.load()
    x = require_device_f32(x, "x")
    B, Cc = x.shape[:2]
    hw = x[0, 0].numel()
    stats = torch.empty((B, Cc, 1, 2), dtype=torch.float32, device=x.device)
    check(lib.ddpm_channel_stats_f32(ptr(x), ptr(stats), B, Cc, hw, stream_ptr()), "channel_stats")
    return stats


def attention(qkv, residual, num_heads: int, scale: float, use_scratch: bool = True):
    """qkv: [B, 3C, N] -> [B, C, N] = softmax(scale q^T k) v (+ residual).  use_scratch: give the library the scratch its
    register-resident kernel (csrc/attention_fa.hip) wants for the f16 planes of q / k / v, as the UNet engine does."""
    lib = _lib.load()
    qkv = require_device_f32(qkv, "qkv")
    B, C3, N = qkv.shape
    Cc = C3 // 3
    if residual is not None:
        residual = require_device_f32(residual, "residual")
    out = torch.empty((B, Cc, N), dtype=torch.float32, device=qkv.device)
    nscr = lib.ddpm_attention_scratch_floats(B, Cc, N, num_heads) if use_scratch else 0
    if nscr:
        scratch = torch.empty(nscr, dtype=torch.float32, device=qkv.device)
        check(lib.ddpm_attention_ws_f32(ptr(qkv), ptr(residual), ptr(out), B, Cc, N, num_heads, scale, ptr(scratch), nscr,
                                        stream_ptr()), "attention")
    else:
        check(lib.ddpm_attention_f32(ptr(qkv), ptr(residual), ptr(out), B, Cc, N, num_heads, scale, stream_ptr()),
              "attention")
    return out


def timestep_embedding(timesteps, freqs, dim: int):
    lib = _lib.load()
    if not timesteps.is_cuda or timesteps.dtype != torch.int64:
        raise RuntimeError("timesteps must be an int64 ROCm device tensor")
    freqs = require_device_f32(freqs, "freqs")
    out = torch.empty((timesteps.shape[0], dim), dtype=torch.float32, device=timesteps.device)
    check(lib.ddpm_timestep_embedding_f32(ptr(timesteps.contiguous()), ptr(freqs), ptr(out), timesteps.shape[0], dim,
                                          stream_ptr()), "timestep_embedding")
    return out


def add_noise(x0, noise, sqrt_ac: np.ndarray, sqrt_1m_ac: np.ndarray, b_scale: float = 1.0):
    lib = _lib.load()
    x0 = require_device_f32(x0, "original_samples")
    noise = require_device_f32(noise, "noise")
    B = x0.shape[0]
    a = np.ascontiguousarray(sqrt_ac, dtype=np.float32)
    b = np.ascontiguousarray(sqrt_1m_ac, dtype=np.float32)
    assert a.shape == (B,) and b.shape == (B,)
    out = torch.empty_like(x0)
    check(lib.ddpm_add_noise_f32(ptr(x0), ptr(noise), a.ctypes.data_as(C.POINTER(C.c_float)),
                                 b.ctypes.data_as(C.POINTER(C.c_float)), float(b_scale), ptr(out), B,
                                 x0[0].numel(), stream_ptr()), "add_noise")
    return out


def plms_step(sample, ets, kind: int, sample_coeff: float, coef_eps: float, denom: float, *, v_prediction=False,
              v_a: float = 0.0, v_b: float = 0.0, out=None):
    """ets: newest-first list of eps tensors (1..4 of them)."""
    lib = _lib.load()
    sample = require_device_f32(sample, "sample")
    es = [require_device_f32(e, "model_output") for e in ets] + [None] * (4 - len(ets))
    if out is None:
        out = torch.empty_like(sample)
    check(lib.ddpm_plms_step_f32(ptr(sample), ptr(es[0]), ptr(es[1]), ptr(es[2]), ptr(es[3]), kind,
                                 int(v_prediction), v_a, v_b, sample_coeff, coef_eps, denom, ptr(out),
                                 sample.numel(), stream_ptr()), "plms_step")
    return out


PREDICTION_TYPES = {"epsilon": 0, "v_prediction": 1, "sample": 2}  # DDPM_PREDICTION_* of the header
_U64 = (1 << 64) - 1


def row_streams_tensor(row_streams, device) -> torch.Tensor:
    """Philox stream ids of the rows as the device array the sampling kernels read: uint64 values carried in an int64 tensor
    (the same bits)."""
    if isinstance(row_streams, torch.Tensor):
        if row_streams.dtype != torch.int64 or not row_streams.is_cuda:
            raise TypeError("row_streams must be an int64 ROCm device tensor (or a sequence of ints)")
        return row_streams.contiguous()
    vals = [int(s) & _U64 for s in row_streams]
    return torch.tensor([v - (1 << 64) if v >> 63 else v for v in vals], dtype=torch.int64, device=device)


def randn_rows(shape, seed: int, row_streams, device=None):
    """[B, ...] standard normals, row b a pure function of (seed, row_streams[b]): Philox counter j / 4 within the row.  Exactly
    the noise ``ancestral_step`` adds for the same (seed, row_streams); a single row with stream s equals
    ``train_ops.randn`` of the same length for (seed, s)."""
    lib = _lib.load()
    if device is None:
        if not isinstance(row_streams, torch.Tensor):
            raise ValueError("randn_rows: device is required when row_streams is not a device tensor")
        device = row_streams.device
    streams = row_streams_tensor(row_streams, device)
    shape = tuple(int(s) for s in shape)
    if not shape or streams.shape != (shape[0],):
        raise ValueError(f"randn_rows: {tuple(streams.shape)} stream ids for shape {shape}")
    out = torch.empty(shape, dtype=torch.float32, device=device)
    check(lib.ddpm_randn_rows_f32(ptr(out), shape[0], out[0].numel(), int(seed) & _U64, ptr(streams), stream_ptr()), "randn_rows")
    return out


def ancestral_step(sample, model_output, *, sqrt_ac: float, sqrt_1m_ac: float, c0: float, ct: float, sigma: float, seed: int = 0,
                   row_streams=None, prediction_type: str = "epsilon", clip_sample: bool = True, return_pred: bool = True,
                   out=None):
    """One fused DDPM reverse step (ddpm_ancestral_step_f32): returns (prev_sample, pred_original_sample or None).
    ``row_streams`` may be None only when sigma == 0 (no noise is drawn then)."""
    lib = _lib.load()
    sample = require_device_f32(sample, "sample")
    model_output = require_device_f32(model_output, "model_output")
    if model_output.shape != sample.shape:
        raise ValueError(f"model_output {tuple(model_output.shape)} does not match sample {tuple(sample.shape)}")
    if prediction_type not in PREDICTION_TYPES:
        raise ValueError(f"unknown prediction_type {prediction_type}")
    B = sample.shape[0]
    streams = None
    if float(sigma) != 0.0:
        if row_streams is None:
            raise ValueError("ancestral_step: row_streams is required when sigma != 0")
        streams = row_streams_tensor(row_streams, sample.device)
        if streams.shape != (B,):
            raise ValueError(f"ancestral_step: {tuple(streams.shape)} stream ids for a batch of {B}")
    if out is None:
        out = torch.empty_like(sample)
    pred = torch.empty_like(sample) if return_pred else None
    check(lib.ddpm_ancestral_step_f32(ptr(sample), ptr(model_output), ptr(out), ptr(pred), B, sample[0].numel(),
                                      PREDICTION_TYPES[prediction_type], int(bool(clip_sample)), sqrt_ac, sqrt_1m_ac, c0, ct,
                                      sigma, int(seed) & _U64, ptr(streams), stream_ptr()), "ancestral_step")
    return out, pred


# ---- the variational bound over rows (likelihood.hip) ---------------------------------------

VLB_COEF_STRIDE = 8


def vlb_coef_table(table, device) -> torch.Tensor:
    """The float64 [T, 6] table of ``DDPMScheduler.likelihood_coefficients`` as the fp32 [T, 8] device table the kernels
    read (each entry rounded once, two pads)."""
    tab = np.asarray(table, dtype=np.float64)
    if tab.ndim != 2 or tab.shape[1] != 6 or tab.shape[0] < 1:
        raise ValueError(f"vlb_coef_table: expected a [T, 6] table, got {tab.shape}")
    host = np.zeros((tab.shape[0], VLB_COEF_STRIDE), dtype=np.float32)
    host[:, :6] = tab.astype(np.float32)
    return torch.from_numpy(host).to(device)


class VlbRows:
    """(image, timestep) rows on the device: int32 ``src`` / ``t`` of one length, range-checked on the host BEFORE the
    upload (the kernels cannot check them).  ``rows[a:b]`` is a view: one upload serves every forward of a bound."""

    def __init__(self, row_src, row_t, n_images: int, num_timesteps: int, device):
        src = np.asarray(row_src, dtype=np.int64).reshape(-1)
        t = np.asarray(row_t, dtype=np.int64).reshape(-1)
        if src.shape != t.shape or src.size == 0:
            raise ValueError(f"vlb rows: {src.size} image indices for {t.size} timesteps")
        if src.min() < 0 or src.max() >= int(n_images):
            raise ValueError(f"vlb rows: row_src outside [0, {int(n_images)})")
        if t.min() < 0 or t.max() >= int(num_timesteps):
            raise ValueError(f"vlb rows: row_t outside [0, {int(num_timesteps)})")
        self.n_images, self.num_timesteps = int(n_images), int(num_timesteps)
        self.src = torch.empty(src.shape, dtype=torch.int32, device=device)
        self.t = torch.empty(t.shape, dtype=torch.int32, device=device)
        self.src.copy_(torch.from_numpy(src.astype(np.int32)))
        self.t.copy_(torch.from_numpy(t.astype(np.int32)))

    def __len__(self) -> int:
        return int(self.src.shape[0])

    def __getitem__(self, s: slice) -> "VlbRows":
        if not isinstance(s, slice) or s.step not in (None, 1):
            raise TypeError("VlbRows supports contiguous slices only")
        out = object.__new__(VlbRows)
        out.n_images, out.num_timesteps = self.n_images, self.num_timesteps
        out.src, out.t = self.src[s], self.t[s]
        if out.src.shape[0] == 0:
            raise ValueError("vlb rows: empty slice")
        return out


def _vlb_args(x0, row_src, row_t, coef):
    x0 = require_device_f32(x0, "x0")
    coef = require_device_f32(coef, "coef")
    if coef.dim() != 2 or coef.shape[1] != VLB_COEF_STRIDE:
        raise ValueError(f"coef must be the [T, {VLB_COEF_STRIDE}] device table of vlb_coef_table, got {tuple(coef.shape)}")
    N, T = int(x0.shape[0]), int(coef.shape[0])
    if isinstance(row_src, VlbRows):
        rows = row_src
        if row_t is not None:
            raise ValueError("row_t must be None when row_src is a VlbRows")
        if rows.n_images != N or rows.num_timesteps != T:
            raise ValueError(f"vlb rows were checked against ({rows.n_images}, {rows.num_timesteps}), not ({N}, {T})")
    else:
        rows = VlbRows(row_src, row_t, N, T, x0.device)
    return x0, coef, rows, N, T


def vlb_noise_rows(x0, noise, row_src, row_t, coef, out=None):
    """x_t[r] = sqrt(abar_t) x0[src] + sqrt(1 - abar_t) noise[src] for the rows (src, t) = (row_src[r], row_t[r]): host
    sequences, range-checked here (0 <= src < N, 0 <= t < T), or one ``VlbRows`` (then ``row_t`` is None).  ``coef``: the
    device table of ``vlb_coef_table``.  Returns [R, ...] (written into ``out`` if given)."""
    lib = _lib.load()
    x0, coef, rows, N, T = _vlb_args(x0, row_src, row_t, coef)
    noise = require_device_f32(noise, "noise")
    if noise.shape != x0.shape:
        raise ValueError(f"noise {tuple(noise.shape)} does not match x0 {tuple(x0.shape)}")
    R = len(rows)
    shape = (R,) + tuple(x0.shape[1:])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x0.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x0.device:
        raise ValueError(f"out must be a contiguous fp32 {shape} tensor on {x0.device}")
    check(lib.ddpm_vlb_noise_rows_f32(ptr(x0), ptr(noise), ptr(rows.src), ptr(rows.t), ptr(coef), T, ptr(out), R,
                                      x0[0].numel(), stream_ptr()), "vlb_noise_rows")
    return out


def vlb_term_rows(x0, x_t, model_output, row_src, row_t, coef, *, prediction_type: str = "epsilon", clip_sample: bool = True,
                  bin_width: float = 1.0 / 255.0, return_kl_map: bool = False, out=None):
    """term[r] = the row mean of the bound's term at (row_src[r], row_t[r]) (ddpm_vlb_term_rows_f32): the KL of posterior and
    predicted step for t > 0, the discretised-Gaussian decoder NLL for t = 0.  Rows as in ``vlb_noise_rows``.  ``out``: a
    contiguous fp32 [R] device tensor to write into (a slice of a larger one will do).  Returns term, or (term, kl_map
    [R, ...]) with ``return_kl_map``."""
    lib = _lib.load()
    x0, coef, rows, N, T = _vlb_args(x0, row_src, row_t, coef)
    x_t = require_device_f32(x_t, "x_t")
    model_output = require_device_f32(model_output, "model_output")
    R = len(rows)
    shape = (R,) + tuple(x0.shape[1:])
    if tuple(x_t.shape) != shape or tuple(model_output.shape) != shape:
        raise ValueError(f"x_t {tuple(x_t.shape)} / model_output {tuple(model_output.shape)} must be {shape}")
    if prediction_type not in PREDICTION_TYPES:
        raise ValueError(f"unknown prediction_type {prediction_type}")
    if not float(bin_width) > 0.0:
        raise ValueError("bin_width must be positive")
    if out is None:
        out = torch.empty((R,), dtype=torch.float32, device=x0.device)
    elif tuple(out.shape) != (R,) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x0.device:
        raise ValueError(f"out must be a contiguous fp32 [{R}] tensor on {x0.device}")
    kl_map = torch.empty(shape, dtype=torch.float32, device=x0.device) if return_kl_map else None
    check(lib.ddpm_vlb_term_rows_f32(ptr(x0), ptr(x_t), ptr(model_output), ptr(rows.src), ptr(rows.t), ptr(coef), T,
                                     PREDICTION_TYPES[prediction_type], int(bool(clip_sample)), float(bin_width), ptr(out),
                                     ptr(kl_map), R, x0[0].numel(), stream_ptr()), "vlb_term_rows")
    return (out, kl_map) if return_kl_map else out


def clamp_mse_(orig, recon, b_scale: float = 1.0):
    """In place: recon <- clamp(recon / b_scale, 0, 1); returns per-image MSE [B]."""
    lib = _lib.load()
    orig = require_device_f32(orig, "images_original")
    if not recon.is_contiguous():
        raise ValueError("recon must be contiguous (it is updated in place)")
    recon = require_device_f32(recon, "reconstructions")
    B = orig.shape[0]
    mse = torch.empty(B, dtype=torch.float32, device=orig.device)
    check(lib.ddpm_clamp_mse_f32(ptr(orig), ptr(recon), float(b_scale), ptr(mse), B, orig[0].numel(), stream_ptr()),
          "clamp_mse")
    return mse


def _accumulator(out, shape, device, what):
    """(out tensor, accumulate flag): a fresh buffer, or the caller's own contiguous fp32 `out` of `shape` to add into."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device), 0
    if (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != torch.float32
            or not out.is_contiguous() or out.device != device):
        raise ValueError(f"{what}: out must be a contiguous float32 {tuple(shape)} tensor on {device}")
    return out, 1


def sqerr_map(a, b, weight: float = 1.0, out=None):
    """out[n, *spatial] (+)= weight * mean over channels of (a - b)^2 for two [N, C, *spatial] tensors (2-D or 3-D): the
    per-pixel values behind ``clamp_mse_``'s per-image number.  ``out`` given: accumulated into (it may not overlap a or b)."""
    lib = _lib.load()
    a = require_device_f32(a, "a")
    b = require_device_f32(b, "b")
    if a.shape != b.shape or a.ndim < 3:
        raise ValueError(f"sqerr_map wants two equal [N, C, *spatial] tensors, got {tuple(a.shape)} and {tuple(b.shape)}")
    B, Cc = a.shape[:2]
    out, acc = _accumulator(out, (B,) + tuple(a.shape[2:]), a.device, "sqerr_map")
    check(lib.ddpm_sqerr_map_f32(ptr(a), ptr(b), ptr(out), B, Cc, int(np.prod(a.shape[2:], dtype=np.int64)), float(weight), acc,
                                 stream_ptr()), "sqerr_map")
    return out


# ---- per-pixel Z-scores of the anomaly maps ------------------------------------------------------

MAP_BLUR_MAX_RADIUS = 16  # kBlurMaxRadius of csrc/zmaps.hip


def _fresh_out(out, shape, device, what):
    """A fresh buffer, or the caller's own contiguous fp32 `out` of `shape` to write into."""
    return _accumulator(out, shape, device, what)[0]


def map_stats_update(values, n_prev: int, mean, m2):
    """One batch merged into the running per-column statistics: ``values`` [B, *shape] (B rows of the validation set), ``mean`` and
    ``m2`` (the sum of squared deviations) contiguous fp32 [*shape] on the device, updated in place; ``n_prev`` rows were merged
    before (0: the buffers are written without being read).  Returns the new row count n_prev + B."""
    lib = _lib.load()
    values = require_device_f32(values, "values")
    if values.ndim < 2 or values.shape[0] < 1:
        raise ValueError(f"map_stats_update wants [B, *shape] values with B >= 1, got {tuple(values.shape)}")
    B, shape = values.shape[0], tuple(values.shape[1:])
    for name, t in (("mean", mean), ("m2", m2)):
        if (not isinstance(t, torch.Tensor) or not t.is_cuda or tuple(t.shape) != shape or t.dtype != torch.float32
                or not t.is_contiguous() or t.device != values.device):
            raise ValueError(f"map_stats_update: {name} must be a contiguous float32 {shape} tensor on {values.device}")
    if int(n_prev) < 0:
        raise ValueError(f"map_stats_update: n_prev must not be negative, got {n_prev}")
    check(lib.ddpm_map_stats_update_f32(ptr(values), B, int(np.prod(shape, dtype=np.int64)), int(n_prev), ptr(mean), ptr(m2),
                                        stream_ptr()), "map_stats_update")
    return int(n_prev) + B


def map_zscore(values, mean, inv_std, weight: float = None, out=None):
    """out[b, *shape] = weight * sum_t (values[b, t] - mean[t]) * inv_std[t] for ``values`` [B, n_t, *shape] and the tables
    ``mean`` / ``inv_std`` [n_t, *shape]; ``weight`` defaults to 1 / n_t (the mean over the t-starts).  ``out``: a contiguous fp32
    [B, *shape] to write into (it may overlap no input)."""
    lib = _lib.load()
    values = require_device_f32(values, "values")
    mean = require_device_f32(mean, "mean")
    inv_std = require_device_f32(inv_std, "inv_std")
    if values.ndim < 3 or mean.shape != values.shape[1:] or inv_std.shape != mean.shape or min(values.shape[:2]) < 1:
        raise ValueError(f"map_zscore wants values [B, n_t, *shape] and two tables [n_t, *shape], got {tuple(values.shape)}, "
                         f"{tuple(mean.shape)} and {tuple(inv_std.shape)}")
    B, n_t = values.shape[:2]
    out = _fresh_out(out, (B,) + tuple(values.shape[2:]), values.device, "map_zscore")
    w = 1.0 / n_t if weight is None else float(weight)
    check(lib.ddpm_map_zscore_f32(ptr(values), ptr(mean), ptr(inv_std), ptr(out), B, n_t,
                                  int(np.prod(values.shape[2:], dtype=np.int64)), w, stream_ptr()), "map_zscore")
    return out


def map_zscore_loo(values, mean, m2, n: int, floor, weight: float = None, out=None):
    """The leave-one-out Z-maps of rows of the validation set: ``values`` [B, n_t, 2, *plane] are rows that were
    counted in the full set's statistics ``mean`` / ``m2`` [n_t, 2, *plane] over ``n`` rows; each is normalised by the mean and the
    sample standard deviation (ddof = 1) of the OTHER n - 1 rows, the divisor floored at ``floor`` [n_t, 2], and averaged over
    the t-starts (``weight`` defaults to 1 / n_t).  Returns fp32 [B, 2, *plane]; ``out``: a contiguous fp32 tensor of that shape to
    write into (it may overlap no input).  n >= 3, else ValueError.  Every operand is a contiguous fp32 tensor on one ROCm
    device (ValueError otherwise: no CPU fallback)."""
    lib = _lib.load()
    for name, t in (("values", values), ("mean", mean), ("m2", m2), ("floor", floor)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() \
                or t.device != values.device:
            raise ValueError(f"map_zscore_loo: {name} must be a contiguous float32 tensor on one ROCm device (no CPU fallback)")
    if values.ndim < 4 or values.shape[2] != 2 or mean.shape != values.shape[1:] or m2.shape != mean.shape \
            or tuple(floor.shape) != tuple(values.shape[1:3]) or values.numel() == 0:
        raise ValueError(f"map_zscore_loo wants values [B, n_t, 2, *plane], two tables [n_t, 2, *plane] and floor [n_t, 2], got "
                         f"{tuple(values.shape)}, {tuple(mean.shape)}, {tuple(m2.shape)} and {tuple(floor.shape)}")
    if int(n) != n or int(n) < 3:
        raise ValueError(f"map_zscore_loo: the statistics of the other rows need n >= 3 rows, got {n}")
    B, n_t = values.shape[:2]
    out = _fresh_out(out, (B,) + tuple(values.shape[2:]), values.device, "map_zscore_loo")
    w = 1.0 / n_t if weight is None else float(weight)
    check(lib.ddpm_map_zscore_loo_f32(ptr(values), ptr(mean), ptr(m2), ptr(floor), ptr(out), B, n_t,
                                      int(np.prod(values.shape[3:], dtype=np.int64)), int(n), w, stream_ptr()), "map_zscore_loo")
    return out


def gaussian_taps(sigma: float, truncate: float = 4.0):
    """The weights of ``scipy.ndimage.gaussian_filter`` (order 0) in float64: exp(-k^2 / 2 sigma^2) for |k| <= radius =
    int(truncate * sigma + 0.5), normalised to sum 1.  sigma <= 0 or radius 0: the single weight 1."""
    sigma = float(sigma)
    radius = int(truncate * sigma + 0.5) if sigma > 0 else 0
    if radius == 0:
        return np.ones(1, dtype=np.float64)
    k = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    return w / w.sum()


def map_blur(maps, sigma: float = None, taps=None, out=None):
    """Separable Gaussian smoothing of [N, H, W] maps with scipy's mode="reflect" boundary (``gaussian_filter(maps[n], sigma)``,
    truncate 4).  ``taps``: the 2 radius + 1 weights as a device tensor (``gaussian_taps`` rounded to fp32) instead of ``sigma``,
    for a caller that smooths many batches.  radius <= 16 (sigma < 4.125), else ValueError.  Not in place."""
    lib = _lib.load()
    maps = require_device_f32(maps, "maps")
    if maps.ndim != 3 or min(maps.shape) < 1:
        raise ValueError(f"map_blur wants [N, H, W] maps, got {tuple(maps.shape)}")
    taps = _blur_taps("map_blur", maps.device, sigma, taps)
    N, H, W = maps.shape
    out = _fresh_out(out, (N, H, W), maps.device, "map_blur")
    check(lib.ddpm_map_blur_f32(ptr(maps), ptr(out), ptr(taps), taps.numel() // 2, N, H, W, stream_ptr()), "map_blur")
    return out


def _blur_taps(what, device, sigma, taps):
    """The device row of weights of ``map_blur`` / ``map_blur3d``: ``gaussian_taps(sigma)`` rounded to fp32, or the caller's."""
    if (sigma is None) == (taps is None):
        raise ValueError(f"{what}: give sigma or taps (one of them)")
    if taps is None:
        if not float(sigma) >= 0.0 or int(4.0 * float(sigma) + 0.5) > MAP_BLUR_MAX_RADIUS:
            raise ValueError(f"{what}: sigma = {sigma} needs radius {int(4.0 * float(sigma) + 0.5) if sigma == sigma else sigma}, "
                             f"outside 0 .. {MAP_BLUR_MAX_RADIUS}")
        w = gaussian_taps(sigma)
        taps = torch.empty((len(w),), dtype=torch.float32, device=device)
        taps.copy_(torch.from_numpy(w.astype(np.float32)))
        return taps
    taps = require_device_f32(taps, "taps")
    if taps.ndim != 1 or taps.numel() % 2 != 1:
        raise ValueError(f"{what}: taps must be an odd number of weights in one row, got {tuple(taps.shape)}")
    if taps.numel() > 2 * MAP_BLUR_MAX_RADIUS + 1:
        raise ValueError(f"{what}: radius {taps.numel() // 2} is above the maximum of {MAP_BLUR_MAX_RADIUS}")
    return taps


def map_blur3d(vols, sigma: float = None, taps=None, out=None):
    """Separable Gaussian smoothing of [N, D, H, W] volumes with scipy's mode="reflect" boundary (``gaussian_filter(vols[n],
    sigma)``, truncate 4): the H and W passes of ``map_blur`` over the N D planes, then the depth pass.  ``sigma`` / ``taps`` /
    ``out`` as ``map_blur``; radius <= 16 also beyond an extent, else ValueError.  Not in place (one volume-sized scratch buffer)."""
    lib = _lib.load()
    vols = require_device_f32(vols, "vols")
    if vols.ndim != 4 or min(vols.shape) < 1:
        raise ValueError(f"map_blur3d wants [N, D, H, W] volumes, got {tuple(vols.shape)}")
    taps = _blur_taps("map_blur3d", vols.device, sigma, taps)
    N, D, H, W = vols.shape
    out = _fresh_out(out, (N, D, H, W), vols.device, "map_blur3d")
    tmp = torch.empty_like(out)
    check(lib.ddpm_map_blur3d_f32(ptr(vols), ptr(out), ptr(tmp), ptr(taps), taps.numel() // 2, N, D, H, W, stream_ptr()),
          "map_blur3d")
    return out


# ---- pixel-level metrics of the maps against ground-truth masks ------------------------------------

MAP_HIST_MAX_BINS = 8191  # kHistMaxBins of csrc/pixel_metrics.hip: two classes of nbins + 1 counters in 64 KB of LDS
MAP_COUNTS_MAX_K = 8      # kCountsMaxK
MAP_HIST_MAX_PARTS = 256  # one workgroup per CU; a workgroup takes at least MAP_HIST_ELEMS_PER_PART elements
MAP_HIST_ELEMS_PER_PART = 16384


def map_hist_parts(elems: int) -> int:
    """The default number of workgroups (= slabs) of ``map_mask_hist`` for ``elems`` map values."""
    return max(1, min(MAP_HIST_MAX_PARTS, -(-int(elems) // MAP_HIST_ELEMS_PER_PART)))


def _maps_and_masks(maps, masks, what):
    """The two operands as they are, or ValueError: contiguous device tensors of one shape [N, ...], fp32 and uint8."""
    for name, t, dtype in (("maps", maps, torch.float32), ("masks", masks, torch.uint8)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous {dtype} tensor on a ROCm device (no CPU fallback)")
    if maps.ndim < 2 or maps.shape != masks.shape or maps.device != masks.device or maps.numel() == 0:
        raise ValueError(f"{what} wants maps and masks of one shape [N, ...] on one device, got {tuple(maps.shape)} and "
                         f"{tuple(masks.shape)}")
    return int(maps.shape[0]), int(maps.numel() // maps.shape[0])


def map_mask_hist(maps, masks, lo: float, hi: float, nbins: int, total=None, parts: int = None):
    """The two-class histogram of ``maps`` [N, ...] (fp32) against ``masks`` of the same shape (uint8, class 1 = mask != 0) over
    ``nbins`` equal bins of [lo, hi): int64 [2, nbins + 1] on the device, values below / above the range in the first / last bin,
    NaN in column ``nbins``.  ``total`` given: added into (it may overlap no input).  bin = (v - lo) * inv_step in fp32 with
    inv_step = nbins / (hi - lo) formed in float64 and rounded once.  ``parts``: the number of workgroups, each with a slab of
    its own (default ``map_hist_parts``); the counts do not depend on it."""
    lib = _lib.load()
    N, P = _maps_and_masks(maps, masks, "map_mask_hist")
    nbins = int(nbins)
    if not 1 <= nbins <= MAP_HIST_MAX_BINS:
        raise ValueError(f"map_mask_hist: nbins must lie in 1 .. {MAP_HIST_MAX_BINS}, got {nbins}")
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo):
        raise ValueError(f"map_mask_hist: the range must be finite with lo < hi, got [{lo}, {hi})")
    inv_step = float(np.float32(nbins / (hi - lo)))
    parts = map_hist_parts(N * P) if parts is None else int(parts)
    if parts < 1:
        raise ValueError(f"map_mask_hist: parts must be at least 1, got {parts}")
    shape = (2, nbins + 1)
    if total is None:
        total, acc = torch.empty(shape, dtype=torch.int64, device=maps.device), 0
    elif (not isinstance(total, torch.Tensor) or tuple(total.shape) != shape or total.dtype != torch.int64
          or not total.is_contiguous() or total.device != maps.device):
        raise ValueError(f"map_mask_hist: total must be a contiguous int64 {shape} tensor on {maps.device}")
    else:
        acc = 1
    slabs = torch.empty((parts,) + shape, dtype=torch.int32, device=maps.device)  # (uint32 counters)
    check(lib.ddpm_map_mask_hist_f32(ptr(maps), ptr(masks), N, P, float(np.float32(lo)), inv_step, nbins, parts, ptr(slabs),
                                     ptr(total), acc, stream_ptr()), "map_mask_hist")
    return total


def map_mask_counts(maps, masks, thresholds):
    """int32 [N, K, 3] on the device: per image and threshold the TP, FP and FN pixels of the prediction ``v > threshold`` against
    ``mask != 0`` (a NaN pixel is predicted negative).  ``thresholds``: 1 .. 8 values, a sequence or an fp32 device tensor [K]."""
    lib = _lib.load()
    N, P = _maps_and_masks(maps, masks, "map_mask_counts")
    if isinstance(thresholds, torch.Tensor):
        thr = thresholds
        if not thr.is_cuda or thr.dtype != torch.float32 or thr.ndim != 1 or not thr.is_contiguous() or thr.device != maps.device:
            raise ValueError(f"map_mask_counts: thresholds must be a contiguous float32 [K] tensor on {maps.device}")
    else:
        host = np.asarray(thresholds, dtype=np.float32).reshape(-1)
        thr = torch.empty((len(host),), dtype=torch.float32, device=maps.device)
        if len(host):
            thr.copy_(torch.from_numpy(host))
    K = int(thr.numel())
    if not 1 <= K <= MAP_COUNTS_MAX_K:
        raise ValueError(f"map_mask_counts: 1 .. {MAP_COUNTS_MAX_K} thresholds, got {K}")
    counts = torch.empty((N, K, 3), dtype=torch.int32, device=maps.device)
    check(lib.ddpm_map_mask_counts_f32(ptr(maps), ptr(masks), N, P, ptr(thr), K, ptr(counts), stream_ptr()), "map_mask_counts")
    return counts


# ---- region-level metrics of the maps: connected components, region overlap, component counts -------

MAP_LABEL_MAX_PIXELS = 16384  # kRgMaxPixels of csrc/regions.hip: a plane's 16-bit labels in 32 KB of LDS (128 x 128)


def _planes(t, dtype, name, what):
    """``t`` as it is, or ValueError: a contiguous [N, H, W] device tensor of ``dtype`` whose plane the labelling can hold."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} tensor on a ROCm device (no CPU fallback)")
    if t.ndim != 3 or t.numel() == 0:
        raise ValueError(f"{what} wants {name} of shape [N, H, W], got {tuple(t.shape)}")
    if t.shape[1] * t.shape[2] > MAP_LABEL_MAX_PIXELS:
        raise ValueError(f"{what}: a plane of {t.shape[1]} x {t.shape[2]} pixels is above the maximum of {MAP_LABEL_MAX_PIXELS} "
                         f"(128 x 128)")
    return tuple(int(v) for v in t.shape)


def _connectivity(connectivity, what):
    if connectivity not in (4, 8):
        raise ValueError(f"{what}: connectivity must be 4 or 8, got {connectivity!r}")
    return int(connectivity)


def _labels_and_regions(labels, regions, shape, device, what):
    for name, t, want in (("labels", labels, tuple(shape)), ("regions", regions, (shape[0],))):
        if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous()
                or tuple(t.shape) != want or t.device != device):
            raise ValueError(f"{what}: {name} must be a contiguous int32 {want} tensor on {device}")


def map_label(x, connectivity: int = 8, threshold: float = None):
    """Connected components of [N, H, W] planes: of ``x != 0`` for a uint8 ``x`` (``threshold`` None), of ``x > threshold`` for an
    fp32 ``x`` (a NaN pixel is outside).  Returns (labels int32 [N, H, W], regions int32 [N]) on the device: 0 outside, the
    components 1 .. regions[n] in ascending order of their smallest flat pixel index, as ``scipy.ndimage.label`` numbers them
    with the cross (``connectivity`` 4) or the 3 x 3 structure (8).  H W <= 16 384."""
    lib = _lib.load()
    what = "map_label"
    connectivity = _connectivity(connectivity, what)
    if threshold is None:
        N, H, W = _planes(x, torch.uint8, "x (no threshold: a mask)", what)
    else:
        N, H, W = _planes(x, torch.float32, "x (with a threshold: a map)", what)
    labels = torch.empty((N, H, W), dtype=torch.int32, device=x.device)
    regions = torch.empty((N,), dtype=torch.int32, device=x.device)
    if threshold is None:
        rc = lib.ddpm_map_label_u8(ptr(x), N, H, W, connectivity, ptr(labels), ptr(regions), stream_ptr())
    else:
        rc = lib.ddpm_map_label_f32(ptr(x), float(np.float32(threshold)), N, H, W, connectivity, ptr(labels), ptr(regions),
                                    stream_ptr())
    check(rc, what)
    return labels, regions


def map_region_overlap(maps, labels, regions, lo: float, hi: float, nbins: int, total=None):
    """The per-region overlap table of ``maps`` (fp32 [N, ...]) against the regions of ``map_label`` (``labels`` of the maps'
    shape, ``regions`` [N]) over the bins of ``map_mask_hist``: float64 [nbins + 1] on the device,
    sum_n sum_r (region r's pixels in the bin) / (region r's pixels), NaN pixels in column ``nbins``.  ``total`` given: added
    into, image by image, so that batches accumulated one after the other give the bits of one batch."""
    lib = _lib.load()
    what = "map_region_overlap"
    if not isinstance(maps, torch.Tensor) or not maps.is_cuda or maps.dtype != torch.float32 or not maps.is_contiguous():
        raise ValueError(f"{what}: maps must be a contiguous {torch.float32} tensor on a ROCm device (no CPU fallback)")
    if maps.ndim < 2 or maps.numel() == 0:
        raise ValueError(f"{what} wants maps of shape [N, ...], got {tuple(maps.shape)}")
    N, P = int(maps.shape[0]), int(maps.numel() // maps.shape[0])
    if P > MAP_LABEL_MAX_PIXELS:
        raise ValueError(f"{what}: a plane of {P} pixels is above the maximum of {MAP_LABEL_MAX_PIXELS} (128 x 128)")
    _labels_and_regions(labels, regions, maps.shape, maps.device, what)
    nbins = int(nbins)
    if not 1 <= nbins <= MAP_HIST_MAX_BINS:
        raise ValueError(f"{what}: nbins must lie in 1 .. {MAP_HIST_MAX_BINS}, got {nbins}")
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo):
        raise ValueError(f"{what}: the range must be finite with lo < hi, got [{lo}, {hi})")
    inv_step = float(np.float32(nbins / (hi - lo)))
    shape = (nbins + 1,)
    if total is None:
        total, acc = torch.empty(shape, dtype=torch.float64, device=maps.device), 0
    elif (not isinstance(total, torch.Tensor) or tuple(total.shape) != shape or total.dtype != torch.float64
          or not total.is_contiguous() or total.device != maps.device):
        raise ValueError(f"{what}: total must be a contiguous float64 {shape} tensor on {maps.device}")
    else:
        acc = 1
    scratch = torch.empty((N,) + shape, dtype=torch.float64, device=maps.device)
    check(lib.ddpm_map_region_overlap_f32(ptr(maps), ptr(labels), ptr(regions), N, P, float(np.float32(lo)), inv_step, nbins,
                                          ptr(scratch), ptr(total), acc, stream_ptr()), what)
    return total


def map_component_counts(maps, masks, labels, regions, thresholds, connectivity: int = 8):
    """int32 [N, K, 3] on the device: per image and threshold ``hit`` (the regions of ``labels`` / ``regions`` with a pixel
    ``v > threshold``), ``pred`` (the connected components of ``v > threshold``) and ``false_pred`` (those components without a
    pixel of ``mask != 0``).  ``maps`` fp32 and ``masks`` uint8 [N, H, W]; ``thresholds``: 1 .. 8 values, a sequence or an fp32
    device tensor [K]."""
    lib = _lib.load()
    what = "map_component_counts"
    connectivity = _connectivity(connectivity, what)
    N, H, W = _planes(maps, torch.float32, "maps", what)
    if _planes(masks, torch.uint8, "masks", what) != (N, H, W) or masks.device != maps.device:
        raise ValueError(f"{what} wants maps and masks of one shape [N, H, W] on one device, got {tuple(maps.shape)} and "
                         f"{tuple(masks.shape)}")
    _labels_and_regions(labels, regions, maps.shape, maps.device, what)
    if isinstance(thresholds, torch.Tensor):
        thr = thresholds
        if not thr.is_cuda or thr.dtype != torch.float32 or thr.ndim != 1 or not thr.is_contiguous() or thr.device != maps.device:
            raise ValueError(f"{what}: thresholds must be a contiguous float32 [K] tensor on {maps.device}")
    else:
        host = np.asarray(thresholds, dtype=np.float32).reshape(-1)
        thr = torch.empty((len(host),), dtype=torch.float32, device=maps.device)
        if len(host):
            thr.copy_(torch.from_numpy(host))
    K = int(thr.numel())
    if not 1 <= K <= MAP_COUNTS_MAX_K:
        raise ValueError(f"{what}: 1 .. {MAP_COUNTS_MAX_K} thresholds, got {K}")
    counts = torch.empty((N, K, 3), dtype=torch.int32, device=maps.device)
    check(lib.ddpm_map_component_counts_f32(ptr(maps), ptr(masks), ptr(labels), ptr(regions), N, H, W, ptr(thr), K, connectivity,
                                            ptr(counts), stream_ptr()), what)
    return counts


# ---- region-level metrics of volumes: the forest in global memory, many workgroups per volume -------

MAP_LABEL3D_CONNECTIVITIES = (26, 18, 6)  # scipy.ndimage.generate_binary_structure(3, 3 | 2 | 1)
MAP_LABEL3D_MAX_VOXELS = 2 ** 31 - 1
MAP_OVERLAP3D_CHUNK_BYTES = 16 << 20      # the default chunk of map_region_overlap3d: regions whose histograms fill this much
MAP_OVERLAP3D_MAX_CHUNK = 65536


def _volumes(t, dtype, name, what):
    """``t`` as it is, or ValueError: a contiguous [N, D, H, W] device tensor of ``dtype`` with fewer than 2^31 voxels a volume."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} tensor on a ROCm device (no CPU fallback)")
    if t.ndim != 4 or t.numel() == 0:
        raise ValueError(f"{what} wants {name} of shape [N, D, H, W], got {tuple(t.shape)}")
    if t.shape[1] * t.shape[2] * t.shape[3] > MAP_LABEL3D_MAX_VOXELS:
        raise ValueError(f"{what}: a volume of {t.shape[1]} x {t.shape[2]} x {t.shape[3]} voxels is not below 2^31")
    return tuple(int(v) for v in t.shape)


def _connectivity3d(connectivity, what):
    if isinstance(connectivity, bool) or connectivity not in MAP_LABEL3D_CONNECTIVITIES:
        raise ValueError(f"{what}: connectivity must be 26, 18 or 6, got {connectivity!r}")
    return int(connectivity)


def _scratch(nbytes, device, what):
    """The scratch of a 3-D region op: ``nbytes`` as the library's size function answers (0: it refuses the arguments)."""
    if nbytes <= 0:
        raise ValueError(f"{what}: the library refuses these extents (scratch size 0)")
    return torch.empty(((int(nbytes) + 7) // 8,), dtype=torch.int64, device=device)


def map_label3d_scratch_bytes(N: int, D: int, H: int, W: int) -> int:
    return int(_lib.load().ddpm_regions3d_label_scratch_bytes(int(N), int(D), int(H), int(W)))


def map_region_overlap3d_chunk(nbins: int) -> int:
    """The default ``chunk_regions`` of ``map_region_overlap3d``."""
    return max(1, min(MAP_OVERLAP3D_MAX_CHUNK, MAP_OVERLAP3D_CHUNK_BYTES // (4 * (int(nbins) + 2))))


def map_region_overlap3d_scratch_bytes(N: int, nbins: int, chunk_regions: int = None) -> int:
    chunk = map_region_overlap3d_chunk(nbins) if chunk_regions is None else int(chunk_regions)
    return int(_lib.load().ddpm_regions3d_overlap_scratch_bytes(int(N), int(nbins), chunk))


def map_component_counts3d_scratch_bytes(N: int, D: int, H: int, W: int, K: int) -> int:
    return int(_lib.load().ddpm_regions3d_counts_scratch_bytes(int(N), int(D), int(H), int(W), int(K)))


def map_label3d(x, connectivity: int = 26, threshold: float = None):
    """``map_label`` for [N, D, H, W] volumes of any extent below 2^31 voxels: (labels int32 [N, D, H, W], regions int32 [N]),
    the components numbered as ``scipy.ndimage.label`` numbers them with ``generate_binary_structure(3, k)``: ``connectivity``
    26 (k = 3), 18 (k = 2) or 6 (k = 1)."""
    lib = _lib.load()
    what = "map_label3d"
    connectivity = _connectivity3d(connectivity, what)
    if threshold is None:
        N, D, H, W = _volumes(x, torch.uint8, "x (no threshold: a mask)", what)
    else:
        N, D, H, W = _volumes(x, torch.float32, "x (with a threshold: a map)", what)
    labels = torch.empty((N, D, H, W), dtype=torch.int32, device=x.device)
    regions = torch.empty((N,), dtype=torch.int32, device=x.device)
    scratch = _scratch(lib.ddpm_regions3d_label_scratch_bytes(N, D, H, W), x.device, what)
    if threshold is None:
        rc = lib.ddpm_map_label3d_u8(ptr(x), N, D, H, W, connectivity, ptr(labels), ptr(regions), ptr(scratch), stream_ptr())
    else:
        rc = lib.ddpm_map_label3d_f32(ptr(x), float(np.float32(threshold)), N, D, H, W, connectivity, ptr(labels), ptr(regions),
                                      ptr(scratch), stream_ptr())
    check(rc, what)
    return labels, regions


def map_region_overlap3d(maps, labels, regions, lo: float, hi: float, nbins: int, total=None, chunk_regions: int = None):
    """``map_region_overlap`` for maps of fewer than 2^31 values an item: float64 [nbins + 1] with the same definition and the same
    bits.  ``chunk_regions``: how many regions' histograms the scratch holds at a time (default: 16 MB worth); a volume with more
    regions takes one pass per chunk, and the result does not depend on it.  Synchronises the stream once (it reads ``regions``)."""
    lib = _lib.load()
    what = "map_region_overlap3d"
    if not isinstance(maps, torch.Tensor) or not maps.is_cuda or maps.dtype != torch.float32 or not maps.is_contiguous():
        raise ValueError(f"{what}: maps must be a contiguous {torch.float32} tensor on a ROCm device (no CPU fallback)")
    if maps.ndim < 2 or maps.numel() == 0:
        raise ValueError(f"{what} wants maps of shape [N, ...], got {tuple(maps.shape)}")
    N, P = int(maps.shape[0]), int(maps.numel() // maps.shape[0])
    if P > MAP_LABEL3D_MAX_VOXELS:
        raise ValueError(f"{what}: {P} values an item are not below 2^31")
    _labels_and_regions(labels, regions, maps.shape, maps.device, what)
    nbins = int(nbins)
    if not 1 <= nbins <= MAP_HIST_MAX_BINS:
        raise ValueError(f"{what}: nbins must lie in 1 .. {MAP_HIST_MAX_BINS}, got {nbins}")
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo):
        raise ValueError(f"{what}: the range must be finite with lo < hi, got [{lo}, {hi})")
    chunk = map_region_overlap3d_chunk(nbins) if chunk_regions is None else int(chunk_regions)
    if not 1 <= chunk <= MAP_OVERLAP3D_MAX_CHUNK:
        raise ValueError(f"{what}: chunk_regions must lie in 1 .. {MAP_OVERLAP3D_MAX_CHUNK}, got {chunk_regions!r}")
    inv_step = float(np.float32(nbins / (hi - lo)))
    shape = (nbins + 1,)
    if total is None:
        total, acc = torch.empty(shape, dtype=torch.float64, device=maps.device), 0
    elif (not isinstance(total, torch.Tensor) or tuple(total.shape) != shape or total.dtype != torch.float64
          or not total.is_contiguous() or total.device != maps.device):
        raise ValueError(f"{what}: total must be a contiguous float64 {shape} tensor on {maps.device}")
    else:
        acc = 1
    scratch = _scratch(lib.ddpm_regions3d_overlap_scratch_bytes(N, nbins, chunk), maps.device, what)
    check(lib.ddpm_map_region_overlap3d_f32(ptr(maps), ptr(labels), ptr(regions), N, P, float(np.float32(lo)), inv_step, nbins, chunk,
                                            ptr(scratch), ptr(total), acc, stream_ptr()), what)
    return total


def map_component_counts3d(maps, masks, labels, regions, thresholds, connectivity: int = 26):
    """``map_component_counts`` for [N, D, H, W] volumes: int32 [N, K, 3] = hit, pred, false_pred per volume and threshold."""
    lib = _lib.load()
    what = "map_component_counts3d"
    connectivity = _connectivity3d(connectivity, what)
    N, D, H, W = _volumes(maps, torch.float32, "maps", what)
    if _volumes(masks, torch.uint8, "masks", what) != (N, D, H, W) or masks.device != maps.device:
        raise ValueError(f"{what} wants maps and masks of one shape [N, D, H, W] on one device, got {tuple(maps.shape)} and "
                         f"{tuple(masks.shape)}")
    _labels_and_regions(labels, regions, maps.shape, maps.device, what)
    if isinstance(thresholds, torch.Tensor):
        thr = thresholds
        if not thr.is_cuda or thr.dtype != torch.float32 or thr.ndim != 1 or not thr.is_contiguous() or thr.device != maps.device:
            raise ValueError(f"{what}: thresholds must be a contiguous float32 [K] tensor on {maps.device}")
    else:
        host = np.asarray(thresholds, dtype=np.float32).reshape(-1)
        thr = torch.empty((len(host),), dtype=torch.float32, device=maps.device)
        if len(host):
            thr.copy_(torch.from_numpy(host))
    K = int(thr.numel())
    if not 1 <= K <= MAP_COUNTS_MAX_K:
        raise ValueError(f"{what}: 1 .. {MAP_COUNTS_MAX_K} thresholds, got {K}")
    counts = torch.empty((N, K, 3), dtype=torch.int32, device=maps.device)
    scratch = _scratch(lib.ddpm_regions3d_counts_scratch_bytes(N, D, H, W, K), maps.device, what)
    check(lib.ddpm_map_component_counts3d_f32(ptr(maps), ptr(masks), ptr(labels), ptr(regions), N, D, H, W, ptr(thr), K, connectivity,
                                              ptr(counts), ptr(scratch), stream_ptr()), what)
    return counts


# ---- predicted segmentations: median filter, size-filtered components -------------------------------

MAP_MEDIAN_SIZES = (3, 5)


def map_median(maps, size: int, out=None):
    """The ``size`` x ``size`` median (3 or 5, else ValueError) of [N, H, W] fp32 maps, any H, W >= 1:
    ``scipy.ndimage.median_filter(maps[n], size=size, mode="reflect")`` for NaN-free input; with NaN, element (size^2 - 1) / 2 of
    ``np.sort`` of the window (a NaN above +inf).  The output is an input value (the sign of a zero among equal zeros and a NaN's
    payload are not pinned).  ``out``: a contiguous fp32 [N, H, W] to write into; it may not overlap ``maps`` (not in place)."""
    lib = _lib.load()
    maps = require_device_f32(maps, "maps")
    if maps.ndim != 3 or min(maps.shape) < 1:
        raise ValueError(f"map_median wants [N, H, W] maps, got {tuple(maps.shape)}")
    if isinstance(size, bool) or size not in MAP_MEDIAN_SIZES:
        raise ValueError(f"map_median: size must be 3 or 5, got {size!r}")
    N, H, W = maps.shape
    out = _fresh_out(out, (N, H, W), maps.device, "map_median")
    check(lib.ddpm_map_median_f32(ptr(maps), ptr(out), int(size), N, H, W, stream_ptr()), "map_median")
    return out


def map_segment(maps, masks, labels, regions, thresholds, min_size: int, connectivity: int = 8):
    """Per image and threshold the predicted segmentation ``v > threshold`` with its connected components of fewer than
    ``min_size`` pixels (1 .. 16 384) removed.  ``maps`` fp32 and ``masks`` uint8 [N, H, W], H W <= 16 384; ``labels`` / ``regions``
    as ``map_label(masks)`` returns them; ``thresholds``: 1 .. 8 values, a sequence or an fp32 device tensor [K].  Returns, on the
    device, (seg uint8 [N, K, H, W]: 1 on the kept components; pixels int32 [N, K, 3]: TP, FP, FN of seg against ``mask != 0``;
    components int32 [N, K, 3]: regions with a kept pixel, kept components, kept components without a masked pixel; removed int32
    [N, K, 2]: the components and pixels dropped).  At ``min_size`` 1: ``map_mask_counts`` and ``map_component_counts``."""
    lib = _lib.load()
    what = "map_segment"
    connectivity = _connectivity(connectivity, what)
    N, H, W = _planes(maps, torch.float32, "maps", what)
    if _planes(masks, torch.uint8, "masks", what) != (N, H, W) or masks.device != maps.device:
        raise ValueError(f"{what} wants maps and masks of one shape [N, H, W] on one device, got {tuple(maps.shape)} and "
                         f"{tuple(masks.shape)}")
    _labels_and_regions(labels, regions, maps.shape, maps.device, what)
    try:
        whole = not isinstance(min_size, bool) and int(min_size) == min_size and 1 <= int(min_size) <= MAP_LABEL_MAX_PIXELS
    except (TypeError, ValueError):
        whole = False
    if not whole:
        raise ValueError(f"{what}: min_size must be an integer in 1 .. {MAP_LABEL_MAX_PIXELS}, got {min_size!r}")
    if isinstance(thresholds, torch.Tensor):
        thr = thresholds
        if not thr.is_cuda or thr.dtype != torch.float32 or thr.ndim != 1 or not thr.is_contiguous() or thr.device != maps.device:
            raise ValueError(f"{what}: thresholds must be a contiguous float32 [K] tensor on {maps.device}")
    else:
        host = np.asarray(thresholds, dtype=np.float32).reshape(-1)
        thr = torch.empty((len(host),), dtype=torch.float32, device=maps.device)
        if len(host):
            thr.copy_(torch.from_numpy(host))
    K = int(thr.numel())
    if not 1 <= K <= MAP_COUNTS_MAX_K:
        raise ValueError(f"{what}: 1 .. {MAP_COUNTS_MAX_K} thresholds, got {K}")
    seg = torch.empty((N, K, H, W), dtype=torch.uint8, device=maps.device)
    pixels = torch.empty((N, K, 3), dtype=torch.int32, device=maps.device)
    components = torch.empty((N, K, 3), dtype=torch.int32, device=maps.device)
    removed = torch.empty((N, K, 2), dtype=torch.int32, device=maps.device)
    check(lib.ddpm_map_segment_f32(ptr(maps), ptr(masks), ptr(labels), ptr(regions), N, H, W, ptr(thr), K, int(min_size), connectivity,
                                   ptr(seg), ptr(pixels), ptr(components), ptr(removed), stream_ptr()), what)
    return seg, pixels, components, removed


# ---- predicted segmentations of volumes --------------------------------------------------------------

MAP_MEDIAN3D_SIZES = (3,)
MAP_SEGMENT3D_MAX_MIN_SIZE = (1 << 31) - 1


def map_median3d(vols, size: int = 3, out=None):
    """The 3 x 3 x 3 median (``size`` 3, else ValueError) of [N, D, H, W] fp32 volumes, every extent >= 1:
    ``scipy.ndimage.median_filter(vols[n], size=3, mode="reflect")`` for NaN-free input; with NaN, element 13 of ``np.sort`` of the
    window (a NaN above +inf).  The output is an input value (the sign of a zero among equal zeros and a NaN's payload are not
    pinned); on D = 1 volumes it has the bits of ``map_median(size=3)``.  ``out``: a contiguous fp32 [N, D, H, W] to write into; it
    may not overlap ``vols`` (not in place)."""
    lib = _lib.load()
    what = "map_median3d"
    N, D, H, W = _volumes(vols, torch.float32, "vols", what)
    if isinstance(size, bool) or size not in MAP_MEDIAN3D_SIZES:
        raise ValueError(f"{what}: size must be 3, got {size!r}")
    out = _fresh_out(out, (N, D, H, W), vols.device, what)
    check(lib.ddpm_map_median3d_f32(ptr(vols), ptr(out), int(size), N, D, H, W, stream_ptr()), what)
    return out


def map_segment3d_scratch_bytes(N: int, D: int, H: int, W: int, K: int) -> int:
    return int(_lib.load().ddpm_regions3d_segment_scratch_bytes(int(N), int(D), int(H), int(W), int(K)))


def map_segment3d(maps, masks, labels, regions, thresholds, min_size: int, connectivity: int = 26):
    """``map_segment`` for [N, D, H, W] volumes of fewer than 2^31 voxels: connectivity 26, 18 or 6, ``min_size`` 1 .. 2^31 - 1,
    ``labels`` / ``regions`` as ``map_label3d(masks)`` returns them.  Returns, on the device, (seg uint8 [N, K, D, H, W], pixels int32
    [N, K, 3], components int32 [N, K, 3], removed int32 [N, K, 2]).  At ``min_size`` 1: ``map_mask_counts`` and
    ``map_component_counts3d``."""
    lib = _lib.load()
    what = "map_segment3d"
    connectivity = _connectivity3d(connectivity, what)
    N, D, H, W = _volumes(maps, torch.float32, "maps", what)
    if _volumes(masks, torch.uint8, "masks", what) != (N, D, H, W) or masks.device != maps.device:
        raise ValueError(f"{what} wants maps and masks of one shape [N, D, H, W] on one device, got {tuple(maps.shape)} and "
                         f"{tuple(masks.shape)}")
    _labels_and_regions(labels, regions, maps.shape, maps.device, what)
    try:
        whole = not isinstance(min_size, bool) and int(min_size) == min_size and 1 <= int(min_size) <= MAP_SEGMENT3D_MAX_MIN_SIZE
    except (TypeError, ValueError):
        whole = False
    if not whole:
        raise ValueError(f"{what}: min_size must be an integer in 1 .. {MAP_SEGMENT3D_MAX_MIN_SIZE}, got {min_size!r}")
    if isinstance(thresholds, torch.Tensor):
        thr = thresholds
        if not thr.is_cuda or thr.dtype != torch.float32 or thr.ndim != 1 or not thr.is_contiguous() or thr.device != maps.device:
            raise ValueError(f"{what}: thresholds must be a contiguous float32 [K] tensor on {maps.device}")
    else:
        host = np.asarray(thresholds, dtype=np.float32).reshape(-1)
        thr = torch.empty((len(host),), dtype=torch.float32, device=maps.device)
        if len(host):
            thr.copy_(torch.from_numpy(host))
    K = int(thr.numel())
    if not 1 <= K <= MAP_COUNTS_MAX_K:
        raise ValueError(f"{what}: 1 .. {MAP_COUNTS_MAX_K} thresholds, got {K}")
    seg = torch.empty((N, K, D, H, W), dtype=torch.uint8, device=maps.device)
    pixels = torch.empty((N, K, 3), dtype=torch.int32, device=maps.device)
    components = torch.empty((N, K, 3), dtype=torch.int32, device=maps.device)
    removed = torch.empty((N, K, 2), dtype=torch.int32, device=maps.device)
    scratch = _scratch(lib.ddpm_regions3d_segment_scratch_bytes(N, D, H, W, K), maps.device, what)
    check(lib.ddpm_map_segment3d_f32(ptr(maps), ptr(masks), ptr(labels), ptr(regions), N, D, H, W, ptr(thr), K, int(min_size), connectivity,
                                     ptr(seg), ptr(pixels), ptr(components), ptr(removed), ptr(scratch), stream_ptr()), what)
    return seg, pixels, components, removed


# ---- LPIPS-AlexNet pieces (src/losses/perceptual_loss.py:105-186) -------------------------------------

def lpips_conv(x, weight, bias, stride: int, pad: int, relu: bool = True, in_scale=None, in_shift=None):
    """relu(conv2d(x * in_scale[c] + in_shift[c], weight, bias, stride, pad)); a 1-channel x feeds every input
    channel of the layer (the ScalingLayer's broadcast)."""
    lib = _lib.load()
    x = require_device_f32(x, "x")
    w = require_device_f32(weight, "weight")
    N, Cx, H, W = x.shape
    cout, cin, k, _ = w.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = torch.empty((N, cout, max(Ho, 0), max(Wo, 0)), dtype=torch.float32, device=x.device)
    opt = [None if t is None else require_device_f32(t, "lpips_conv operand") for t in (bias, in_scale, in_shift)]
    check(lib.ddpm_lpips_conv_f32(ptr(x), ptr(w), ptr(opt[0]), ptr(opt[1]), ptr(opt[2]), ptr(out), N, Cx, cin, H, W,
                                  cout, k, stride, pad, int(relu), stream_ptr()), "lpips_conv")
    return out


def lpips_conv_biasmap(x, weight, bias_map, stride: int, pad: int, relu: bool = True):
    """relu(conv2d(x, weight, None, stride, pad) + bias_map[None]); bias_map: [Cout, Ho, Wo]."""
    lib = _lib.load()
    x = require_device_f32(x, "x")
    w = require_device_f32(weight, "weight")
    bias_map = require_device_f32(bias_map, "bias_map")
    N, cin, H, W = x.shape
    cout, _, k, _ = w.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if tuple(bias_map.shape[-3:]) != (cout, Ho, Wo) or w.shape[1] != cin:
        raise ValueError(f"lpips_conv_biasmap: bias_map {tuple(bias_map.shape)} / weight {tuple(w.shape)} do not fit the input")
    out = torch.empty((N, cout, Ho, Wo), dtype=torch.float32, device=x.device)
    check(lib.ddpm_lpips_conv_biasmap_f32(ptr(x), ptr(w), ptr(bias_map), ptr(out), N, cin, H, W, cout, k, stride, pad,
                                          int(relu), stream_ptr()), "lpips_conv_biasmap")
    return out


def lpips_pack_conv_weight(weight):
    """torch [Cout, Cin, k, k] -> the MFMA operand layout of lpips_conv_mfma (Cout % 32 == 0, Cin % 2 == 0)."""
    lib = _lib.load()
    w = require_device_f32(weight, "weight")
    cout, cin, k, _ = w.shape
    out = torch.empty(w.numel(), dtype=torch.float32, device=w.device)
    check(lib.ddpm_lpips_pack_conv_weight_f32(ptr(w), ptr(out), cout, cin, k, stream_ptr()), "lpips_pack_conv_weight")
    return out


def lpips_conv_mfma_supported(cin: int, h: int, w: int, cout: int, k: int) -> bool:
    return bool(_lib.load().ddpm_lpips_conv_mfma_supported(cin, h, w, cout, k))


def lpips_conv_mfma(x, packed, bias, cout: int, k: int, relu: bool = True):
    """relu(conv2d(x, w, bias, stride 1, padding k // 2)) on the fp32 MFMA pipe; packed = lpips_pack_conv_weight(w)."""
    lib = _lib.load()
    x = require_device_f32(x, "x")
    N, cin, H, W = x.shape
    out = torch.empty((N, cout, H, W), dtype=torch.float32, device=x.device)
    bias = None if bias is None else require_device_f32(bias, "bias")
    check(lib.ddpm_lpips_conv_mfma_f32(ptr(x), ptr(packed), ptr(bias), ptr(out), N, cin, H, W, cout, k, int(relu),
                                       stream_ptr()), "lpips_conv_mfma")
    return out


def maxpool3s2(x):
    """MaxPool2d(3, 2)."""
    lib = _lib.load()
    x = require_device_f32(x, "x")
    N, Cc, H, W = x.shape
    out = torch.empty((N, Cc, (H - 3) // 2 + 1, (W - 3) // 2 + 1), dtype=torch.float32, device=x.device)
    check(lib.ddpm_maxpool3s2_f32(ptr(x), ptr(out), N * Cc, H, W, stream_ptr()), "maxpool3s2")
    return out


def lpips_layer(f0, f1, lin, out=None):
    """out[n] (+)= spatial mean of the lin-weighted squared difference of the channel-normalised features."""
    lib = _lib.load()
    f0 = require_device_f32(f0, "f0")
    f1 = require_device_f32(f1, "f1")
    lin = require_device_f32(lin, "lin")
    if f0.shape != f1.shape:
        raise ValueError(f"feature maps differ in shape: {tuple(f0.shape)} vs {tuple(f1.shape)}")
    N, Cc, H, W = f0.shape
    acc = out is not None
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=f0.device)
    check(lib.ddpm_lpips_layer_f32(ptr(f0), ptr(f1), ptr(lin), ptr(out), N, Cc, H * W, int(acc), stream_ptr()),
          "lpips_layer")
    return out


def lpips_layer_map(f0, f1, lin, maps=None, row_offset: int = 0):
    """The per-position value ``lpips_layer`` averages: maps[n, row_offset + p] = the lin-weighted squared difference of the
    channel-normalised features at position p.  ``maps``: a contiguous fp32 [N, row_stride] device tensor (the packed row of
    all five layers of a pair; written at ``row_offset``), or None for a fresh [N, H * W]."""
    lib = _lib.load()
    f0 = require_device_f32(f0, "f0")
    f1 = require_device_f32(f1, "f1")
    lin = require_device_f32(lin, "lin")
    if f0.shape != f1.shape or f0.ndim != 4:
        raise ValueError(f"feature maps differ in shape: {tuple(f0.shape)} vs {tuple(f1.shape)}")
    N, Cc, H, W = f0.shape
    if lin.numel() != Cc:
        raise ValueError(f"lpips_layer_map: lin has {lin.numel()} weights for {Cc} channels")
    if maps is None:
        maps, row_offset = torch.empty((N, H * W), dtype=torch.float32, device=f0.device), 0
    elif (not isinstance(maps, torch.Tensor) or maps.ndim != 2 or maps.shape[0] != N or maps.dtype != torch.float32
          or not maps.is_contiguous() or maps.device != f0.device):
        raise ValueError(f"lpips_layer_map: maps must be a contiguous float32 [{N}, row_stride] tensor on {f0.device}")
    if row_offset < 0 or row_offset + H * W > maps.shape[1]:
        raise ValueError(f"lpips_layer_map: {H * W} positions at offset {row_offset} do not fit a row of {maps.shape[1]}")
    check(lib.ddpm_lpips_layer_map_f32(ptr(f0), ptr(f1), ptr(lin), ptr(maps), N, Cc, H * W, maps.shape[1], int(row_offset),
                                       stream_ptr()), "lpips_layer_map")
    return maps


def lpips_map_upsample(maps, layer_sizes, full_size, window=None, weight: float = 1.0, out=None):
    """out[n, y, x] (+)= weight * the sum over layers of the layer's map resampled to ``full_size`` = (Hfull, Wfull) the way
    ``nn.Upsample(size, mode="bilinear", align_corners=False)`` does.  ``maps``: [N, row_stride], the layers of
    ``layer_sizes`` = [(h_k, w_k), ...] (1 .. 5 of them) packed one after the other in each row; ``window`` = (oy, ox, H, W)
    selects a part of the full grid (default: all of it).  ``out`` given: a contiguous fp32 [N, H, W] to add into."""
    lib = _lib.load()
    maps = require_device_f32(maps, "maps")
    if maps.ndim != 2:
        raise ValueError(f"lpips_map_upsample: maps must be [N, row_stride], got {tuple(maps.shape)}")
    sizes = [(int(h), int(w)) for h, w in layer_sizes]
    if not 1 <= len(sizes) <= 5:
        raise ValueError(f"lpips_map_upsample: 1 .. 5 layers, got {len(sizes)}")
    if sum(h * w for h, w in sizes) > maps.shape[1] or min(min(s) for s in sizes) < 1:
        raise ValueError(f"lpips_map_upsample: layers {sizes} do not fit a row of {maps.shape[1]}")
    Hf, Wf = (int(v) for v in full_size)
    oy, ox, H, W = (0, 0, Hf, Wf) if window is None else (int(v) for v in window)
    if min(oy, ox) < 0 or min(H, W) < 1 or oy + H > Hf or ox + W > Wf:
        raise ValueError(f"lpips_map_upsample: window {(oy, ox, H, W)} lies outside the full grid {(Hf, Wf)}")
    N = maps.shape[0]
    out, acc = _accumulator(out, (N, H, W), maps.device, "lpips_map_upsample")
    flat = [v for s in sizes + [(0, 0)] * (5 - len(sizes)) for v in s]
    check(lib.ddpm_lpips_map_upsample_f32(ptr(maps), ptr(out), N, maps.shape[1], len(sizes), *flat, Hf, Wf, oy, ox, H, W,
                                          float(weight), acc, stream_ptr()), "lpips_map_upsample")
    return out


def lpips_map_upsample_view(maps, layer_sizes, volume_shape, axis: int, weight: float = 1.0, out=None):
    """The LPIPS map of volumes from their slices along ``axis`` (2, 3 or 4 of [N, C, D, H, W]): out[n, d, h, w] (+)= weight * what
    ``lpips_map_upsample`` gives for the voxel's slice at the voxel's place in it, written straight into the volume's layout.
    ``maps``: [N * S, row_stride], the slices' packed rows, volume-major (S = the extent along ``axis``); ``layer_sizes``: the
    layers of a slice's plane ([H, W], [D, W] or [D, H]); ``volume_shape`` = (D, H, W).  ``out`` given: a contiguous fp32
    [N, D, H, W] to add into."""
    lib = _lib.load()
    maps = require_device_f32(maps, "maps")
    if maps.ndim != 2:
        raise ValueError(f"lpips_map_upsample_view: maps must be [N * S, row_stride], got {tuple(maps.shape)}")
    sizes = [(int(h), int(w)) for h, w in layer_sizes]
    if not 1 <= len(sizes) <= 5:
        raise ValueError(f"lpips_map_upsample_view: 1 .. 5 layers, got {len(sizes)}")
    if min(min(s) for s in sizes) < 1:
        raise ValueError(f"lpips_map_upsample_view: an empty AlexNet layer in {sizes}: nothing to resample")
    if sum(h * w for h, w in sizes) > maps.shape[1]:
        raise ValueError(f"lpips_map_upsample_view: layers {sizes} do not fit a row of {maps.shape[1]}")
    if int(axis) != axis or not 2 <= int(axis) <= 4:
        raise ValueError(f"lpips_map_upsample_view: axis must be 2, 3 or 4 of [N, C, D, H, W], got {axis}")
    shape = tuple(int(v) for v in volume_shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"lpips_map_upsample_view: volume_shape must be (D, H, W), got {tuple(volume_shape)}")
    S = shape[int(axis) - 2]
    if maps.shape[0] < S or maps.shape[0] % S:
        raise ValueError(f"lpips_map_upsample_view: {maps.shape[0]} rows are no whole number of volumes of {S} slices")
    N = maps.shape[0] // S
    out, acc = _accumulator(out, (N,) + shape, maps.device, "lpips_map_upsample_view")
    flat = [v for s in sizes + [(0, 0)] * (5 - len(sizes)) for v in s]
    check(lib.ddpm_lpips_map_upsample_view_f32(ptr(maps), ptr(out), N, maps.shape[1], len(sizes), *flat, *shape, int(axis),
                                               float(weight), acc, stream_ptr()), "lpips_map_upsample_view")
    return out


def lpips_layer_backward(f0, f1, lin, upstream, out=None, relu_mask: bool = True):
    """Backward of lpips_layer w.r.t. f0: out (+)= upstream[n] d(score[n]) / d(f0[n]); relu_mask: f0 is a post-ReLU feature map and
    out the gradient before that ReLU (0 where f0 <= 0, the accumulated value included)."""
    lib = _lib.load()
    f0 = require_device_f32(f0, "f0")
    f1 = require_device_f32(f1, "f1")
    lin = require_device_f32(lin, "lin")
    upstream = require_device_f32(upstream, "upstream")
    if f0.shape != f1.shape or f0.ndim != 4:
        raise ValueError(f"feature maps differ in shape: {tuple(f0.shape)} vs {tuple(f1.shape)}")
    N, Cc, H, W = f0.shape
    if lin.numel() != Cc or upstream.numel() != N:
        raise ValueError(f"lpips_layer_backward: lin has {lin.numel()} weights for {Cc} channels, upstream {upstream.numel()} for {N} pairs")
    acc = out is not None
    if out is None:
        out = torch.empty_like(f0)
    elif out.shape != f0.shape or not out.is_contiguous() or out.dtype != torch.float32 or out.device != f0.device:
        raise ValueError("lpips_layer_backward: out must be a contiguous float32 tensor of f0's shape on its device")
    check(lib.ddpm_lpips_layer_backward_f32(ptr(f0), ptr(f1), ptr(lin), ptr(upstream), ptr(out), N, Cc, H * W, int(acc),
                                            int(relu_mask), stream_ptr()), "lpips_layer_backward")
    return out


def maxpool3s2_backward(x, dy, out=None, relu_mask: bool = False):
    """Backward of maxpool3s2 (PyTorch's tie rule: the first maximum in row-major order takes the gradient): out (+)= dx;
    relu_mask: 0 where x <= 0 (x is a post-ReLU feature map, out the gradient before that ReLU)."""
    lib = _lib.load()
    x = require_device_f32(x, "x")
    dy = require_device_f32(dy, "dy")
    N, Cc, H, W = x.shape
    if tuple(dy.shape) != (N, Cc, (H - 3) // 2 + 1, (W - 3) // 2 + 1):
        raise ValueError(f"maxpool3s2_backward: dy {tuple(dy.shape)} does not belong to x {tuple(x.shape)}")
    acc = out is not None
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or not out.is_contiguous() or out.dtype != torch.float32 or out.device != x.device:
        raise ValueError("maxpool3s2_backward: out must be a contiguous float32 tensor of x's shape on its device")
    check(lib.ddpm_maxpool3s2_backward_f32(ptr(x), ptr(dy), ptr(out), N * Cc, H, W, int(acc), int(relu_mask), stream_ptr()),
          "maxpool3s2_backward")
    return out


def lpips_conv1_dgrad(g, weight, in_channels: int, height: int, width: int, stride: int, pad: int, in_scale=None):
    """Input gradient [N, in_channels (1 or 3), height, width] of lpips_conv(x, weight [Cout, 3, k, k], stride, pad, in_scale) given
    g = the gradient of its pre-ReLU output; in_channels = 1: through the 1 -> 3 broadcast (the three channels summed)."""
    lib = _lib.load()
    g = require_device_f32(g, "g")
    w = require_device_f32(weight, "weight")
    cout, cin, k, _ = w.shape
    N = g.shape[0]
    Ho, Wo = (height + 2 * pad - k) // stride + 1, (width + 2 * pad - k) // stride + 1
    if tuple(g.shape) != (N, cout, Ho, Wo):
        raise ValueError(f"lpips_conv1_dgrad: g {tuple(g.shape)} is not the layer's output for a {height} x {width} input")
    in_scale = None if in_scale is None else require_device_f32(in_scale, "in_scale")
    out = torch.empty((N, in_channels, height, width), dtype=torch.float32, device=g.device)
    check(lib.ddpm_lpips_conv1_dgrad_f32(ptr(g), ptr(w), ptr(in_scale), ptr(out), N, in_channels, cin, height, width, cout, k,
                                         stride, pad, stream_ptr()), "lpips_conv1_dgrad")
    return out


def vq_nearest(x, codebook):
    """VQ-VAE quantiser, eval path: (indices int64 [B, *spatial], x + (codebook[indices] - x) [B, D, *spatial])."""
    lib = _lib.load()
    x = require_device_f32(x, "x")
    e = require_device_f32(codebook, "codebook")
    B, D = x.shape[:2]
    S = x[0, 0].numel()
    K = e.shape[0]
    if e.shape[1] != D:
        raise ValueError(f"codebook is [{K}, {e.shape[1]}] but the latent has {D} channels")
    idx = torch.empty((B,) + tuple(x.shape[2:]), dtype=torch.int32, device=x.device)
    out = torch.empty_like(x)
    norms = torch.empty(K, dtype=torch.float32, device=x.device)
    check(lib.ddpm_vq_nearest_f32(ptr(x), ptr(e), ptr(norms), idx.data_ptr(), ptr(out), B, D, S, K, stream_ptr()),
          "vq_nearest")
    return idx.long(), out


def _vq_shapes(x, e):
    B, D = x.shape[:2]
    K = e.shape[0]
    if e.ndim != 2 or e.shape[1] != D:
        raise ValueError(f"codebook is {tuple(e.shape)} but the latent has {D} channels")
    return B, D, x[0, 0].numel(), K


def vq_train_assign(x, codebook, commitment_cost: float = 0.25):
    """VQ-VAE quantiser, training path (vq.hip): the search of ``vq_nearest`` plus what the EMA update and the loss need.
    -> (idx int32 [B, *spatial], out = x + (codebook[idx] - x), counts [K], dw [K, D], loss 0-dim, sums [K (D + 1)]).
    counts / dw are views of ``sums`` (one allocation: ONE all_reduce over ranks before ``vq_train_update``); loss =
    commitment_cost * mean((codebook[idx] - x)^2).  counts, dw and loss are bit-identical run to run."""
    lib = _lib.load()
    x = require_device_f32(x, "x")
    e = require_device_f32(codebook, "codebook")
    B, D, S, K = _vq_shapes(x, e)
    idx = torch.empty((B,) + tuple(x.shape[2:]), dtype=torch.int32, device=x.device)
    out = torch.empty_like(x)
    norms = torch.empty(K, dtype=torch.float32, device=x.device)
    sums = torch.empty(K * (D + 1), dtype=torch.float32, device=x.device)
    counts, dw = sums[:K], sums[K:].view(K, D)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    partials = torch.empty(max(1, lib.ddpm_vq_train_partials(B, D, S)), dtype=torch.float64, device=x.device)
    check(lib.ddpm_vq_train_assign_f32(ptr(x), ptr(e), ptr(norms), idx.data_ptr(), ptr(out), ptr(counts), ptr(dw), ptr(loss),
                                       partials.data_ptr(), B, D, S, K, float(commitment_cost), stream_ptr()), "vq_train_assign")
    return idx, out, counts, dw, loss, sums


def _inplace_f32(t, name, shape):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or \
            tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be a contiguous float32 ROCm tensor of shape {tuple(shape)} (it is updated in place)")
    return t


def vq_train_update(ema_cluster_size, ema_w, codebook, counts, dw, decay: float, epsilon: float) -> None:
    """EMA codebook update, one launch, in place on the three state tensors (formulas: include/ddpm_ood_hip.h)."""
    lib = _lib.load()
    K, D = codebook.shape
    _inplace_f32(ema_cluster_size, "ema_cluster_size", (K,))
    _inplace_f32(ema_w, "ema_w", (K, D))
    _inplace_f32(codebook, "codebook", (K, D))
    counts, dw = require_device_f32(counts, "counts"), require_device_f32(dw, "dw")
    if counts.numel() != K or dw.numel() != K * D:
        raise ValueError(f"counts / dw are {tuple(counts.shape)} / {tuple(dw.shape)} for a [{K}, {D}] codebook")
    check(lib.ddpm_vq_train_update_f32(ptr(ema_cluster_size), ptr(ema_w), ptr(codebook), ptr(counts), ptr(dw), K, D, float(decay),
                                       float(epsilon), stream_ptr()), "vq_train_update")


def vq_train_backward(dout, x, codebook, idx, dloss, commitment_cost: float = 0.25):
    """dx = dout + (2 commitment_cost / numel) (x - codebook[idx]) dloss; ``codebook`` is the one ``vq_train_assign`` searched.
    dout / dloss may be None (that term is zero)."""
    lib = _lib.load()
    x = require_device_f32(x, "x")
    e = require_device_f32(codebook, "codebook")
    B, D, S, K = _vq_shapes(x, e)
    if idx.dtype != torch.int32 or not idx.is_cuda or idx.numel() != B * S:
        raise ValueError("idx must be the int32 device tensor vq_train_assign returned")
    dout = None if dout is None else require_device_f32(dout, "dout")
    dloss = None if dloss is None else require_device_f32(dloss, "dloss")
    dx = torch.empty_like(x)
    check(lib.ddpm_vq_train_backward_f32(ptr(dout), ptr(x), ptr(e), idx.contiguous().data_ptr(), ptr(dloss), ptr(dx), B, D, S,
                                         float(commitment_cost), stream_ptr()), "vq_train_backward")
    return dx


# ---- simplex noise (src/utils/simplex_noise.py: generate_simplex_noise) ----------------------------------

def simplex_noise(shape, seeds, t, octaves: int = 6, persistence: float = 0.8, frequency: float = 64.0, device=None):
    """AnoDDPM fractal simplex noise of shape [B, C, H, W] or [B, C, D, H, W] (a 3-D input repeats the 2-D slice along D,
    as the reference does): slice (b, c) is seeded by seeds[b, c] and taken at time t[b].  seeds: int64 [B, C], t: int64 [B],
    either on the host (they travel in ONE non-blocking copy) or already on the device.  Returns fp32 on the current stream."""
    lib = _lib.load()
    shape = tuple(int(s) for s in shape)
    if len(shape) not in (4, 5):
        raise ValueError(f"simplex_noise: shape {shape} is neither [B, C, H, W] nor [B, C, D, H, W]")
    B, Cn = shape[:2]
    depth = shape[2] if len(shape) == 5 else 1
    seeds = torch.as_tensor(seeds, dtype=torch.int64)
    t = torch.as_tensor(t, dtype=torch.int64)
    if tuple(seeds.shape) != (B, Cn) or tuple(t.shape) != (B,):
        raise ValueError(f"simplex_noise: seeds {tuple(seeds.shape)} / t {tuple(t.shape)} do not fit {shape}")
    if device is None:
        device = seeds.device if seeds.is_cuda else t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("simplex_noise runs on a ROCm device: the HIP path has no CPU fallback")
    if seeds.device != device and t.device != device:  # both from the host: one pinned buffer, one copy
        both = torch.cat([seeds.reshape(-1), t]).pin_memory().to(device, non_blocking=True)
        seeds_d, t_d = both[: B * Cn], both[B * Cn:]
    else:
        seeds_d, t_d = (v.pin_memory().to(device, non_blocking=True) if v.device != device else v.contiguous() for v in (seeds, t))
    out = torch.empty(shape, dtype=torch.float32, device=device)
    check(lib.ddpm_simplex_noise_f32(ptr(out), seeds_d.data_ptr(), t_d.data_ptr(), B, Cn, depth, shape[-2], shape[-1],
                                     int(octaves), float(persistence), float(frequency), stream_ptr()), "simplex_noise")
    return out
