"""The VQ-VAE's encoder / decoder training step on the library's own kernels (``DDPM_VQVAE_NATIVE=1``).

One ``autograd.Function`` per ``_Convolution`` layer (and per half of a ``_ResidualUnit``), so the graph still composes with
``VQTrainFunction``, the loss terms and ``torch.optim.Adam``:
  * forward: the SAME HIP inference kernel the eval path selects -- the layer's own ``forward`` / the unit's ``head`` and ``tail``,
    with their packed-weight caches keyed on (data_ptr, _version) -- so the training forward is the eval path's bits;
  * backward: g = relu_backward(y, dy) where the layer has a ReLU; the residual gradient is g; db = the plane sums of g; dw from
    the matching weight-gradient entry point (3x3 / 3x3x3: ddpm_conv_wgrad_f32 / ddpm_conv3d_wgrad_f32, k4 s2 p1:
    ddpm_conv_k4s2_wgrad_f32, transposed by the operand swap); dx from the inference kernels through the identities
        k3 s1:             dx = conv(g, rot180t(w))
        Conv k4 s2 p1:     dx = conv_transpose_k4s2p1(g, w)   (w[Cout, Cin, 4..] is a ConvTranspose weight with in = Cout)
        ConvT k4 s2 p1:    dx = conv_k4s2p1(g, w)             (w[Cin, Cout, 4..] read as [out = Cin, in = Cout])
    on the MFMA kernels where the swapped channel counts have a tiling, the generic kernel otherwise.
Gradient range: an L1 loss over a 64^3 volume hands the input-gradient convolutions values of about 4e-6, below f16's normal range,
and the split-f16 kernel families assume O(1) operands.  Every input-gradient launch therefore runs on an fp32 family, with no
rescaling and no host read of a maximum: the 3-D launches by what they are handed (the dispatcher takes the split-f16 F(4x4)
kernel only with its pre-split weight planes, which are not passed; the k4 s2 / transposed / generic kernels have no split form;
the transposed input gradient never takes the parity form).  Only a 2-D 3x3 input gradient with an MFMA tiling (``ops.conv``,
whose small-launch families split their operands on the fly) needs the library's master switch: ``_fp32_families`` turns
``ddpm_set_split_f16`` off around that one launch.  That switch is process-global: a flip makes a UNet engine in the same process
re-capture its HIP graphs on its next graphed forward, and it is not safe against another thread launching at the same time --
harmless for stand-alone VQ-VAE training, and no 3-D model or generic-kernel 2-D model ever flips it.  The 3x3 weight gradient's
split form measures and rescales both operands itself.
"""

from __future__ import annotations

import contextlib

import torch

from . import _lib, ops, train_ops
from .vqvae import _Convolution, _ResidualUnit, _require_device


@contextlib.contextmanager
def _fp32_families():
    """The split-f16 kernel families off for the launches inside (a host-side switch read per launch: no synchronisation).
    Process-global, see the module docstring: used for the 2-D ``ops.conv`` input gradient only, and only if the switch is on."""
    was = _lib.split_f16()
    if was:
        _lib.set_split_f16(False)
    try:
        yield
    finally:
        if was:
            _lib.set_split_f16(True)


def _layer_name(layer) -> str:
    return f"{type(layer.conv).__name__}{tuple(layer.conv.weight.shape)} (kernel, stride, dilation, padding, output_padding = {layer.geom[1:]})"


def _geometry(layer):
    """(spatial dims, 'k3' | 'k4' | 'k4t') of a layer the native backward is built for; anything else raises."""
    sd, k, s, dil, pad, opad = layer.geom
    if dil == 1 and pad == 1 and opad == 0:
        if not layer.is_transposed and (k, s) == (3, 1):
            return sd, "k3"
        if (k, s) == (4, 2):
            return sd, "k4t" if layer.is_transposed else "k4"
    raise NotImplementedError(f"DDPM_VQVAE_NATIVE=1: no native gradient for VQ-VAE layer {_layer_name(layer)}: only k3 s1 p1 and "
                              "(transposed) k4 s2 p1 convolutions are built")


def bias_grad(g):
    """db[C] = sum of g [B, C, ...] over images and positions (ddpm_row_sum_f32 per plane, ddpm_col_sum_f32 over the batch)."""
    B, Cc = g.shape[:2]
    rows = train_ops.row_sum(g, B * Cc, g[0, 0].numel())
    return rows if B == 1 else train_ops.col_sum(rows, B, Cc)


def conv3d_k3_wgrad(a, g):
    """dw[Cout, Cin, 3, 3, 3] of F.conv3d(a, w, padding=1): ddpm_conv3d_wgrad_f32 where it has a tiling (Cin % 64 == 0, Cout % 64
    == 0, an even W <= 64), else ddpm_conv_wgrad_f32 per depth tap over the slices that tap reaches, (batch item, slice) as the
    image (the slices are gathered by a copy: the 2-D entry point wants NCHW)."""
    B, Cin, D, H, W = a.shape
    Cout = g.shape[1]
    if _lib.load().ddpm_conv3d_wgrad_scratch_floats(B, Cin, Cout, D, H, W, D, H, W, 1):
        return train_ops.conv3d_wgrad(a, g)
    dw = torch.empty((Cout, Cin, 3, 3, 3), dtype=torch.float32, device=a.device)
    for kd in range(3):
        lo, hi = max(0, 1 - kd), min(D, D + 1 - kd)  # output slices zo whose input slice zo + kd - 1 is inside the volume
        if hi <= lo:
            dw[:, :, kd].zero_()
            continue
        a_s = a[:, :, lo + kd - 1: hi + kd - 1].transpose(1, 2).reshape(-1, Cin, H, W)
        g_s = g[:, :, lo:hi].transpose(1, 2).reshape(-1, Cout, H, W)
        dw[:, :, kd] = train_ops.conv_wgrad(a_s, g_s, 3)
    return dw


def conv_weight_grad(a, g, spatial_dims: int, form: str):
    """The weight gradient, in torch's layout, of a 'k3' / 'k4' / 'k4t' layer with input a and output gradient g."""
    if form == "k4":
        return train_ops.conv_k4s2_wgrad(a, g)
    if form == "k4t":
        return train_ops.conv_k4s2_wgrad(g, a)  # the operand swap: already [Cin, Cout, 4, ...]
    return train_ops.conv_wgrad(a, g, 3) if spatial_dims == 2 else conv3d_k3_wgrad(a, g)


def conv_input_grad(g, w, spatial_dims: int, form: str):
    """The input gradient of a 'k3' / 'k4' / 'k4t' layer with weight w (torch layout) given its output gradient g, on the fp32 kernel
    families (module docstring)."""
    g = g.contiguous()
    if form == "k3":
        wt = train_ops.conv_weight_rot180t(w)
        if spatial_dims == 3 and ops.conv3d_supported(wt, 1):  # (no split-f16 planes passed: F(4x4) / F(2x2) / direct on fp32)
            return ops.conv3d(g, wt, None, packed=ops.pack_conv3d_weight(wt), wino=ops.pack_wino3d_weight(wt),
                              wino44=ops.pack_wino44_3d_weight(wt))
        if spatial_dims == 2 and wt.shape[0] % 128 == 0 and wt.shape[1] % 4 == 0:
            with _fp32_families():
                return ops.conv(g, wt, None)
        return ops.convnd_generic(g, wt, None, stride=1, padding=1)
    if form == "k4":  # w[Cout, Cin, 4..] as a ConvTranspose weight: in = Cout, out = Cin
        if _lib.load().ddpm_packed_convtr_weight_floats(w.shape[1], w.shape[0], spatial_dims):
            return ops.conv_transpose(g, w, None)  # 2-D and 3-D: the fp32-MFMA transposed kernel
        if spatial_dims == 3 and w.shape[1] == 1:
            return ops.convT3d_k4s2_cout1(g, w, None)
        return ops.convnd_generic(g, w, None, stride=2, padding=1, transposed=True)
    # 'k4t': w[Cin, Cout, 4..] as a Conv weight: out = Cin, in = Cout (the k4 s2 MFMA convolution exists in 3-D only)
    if spatial_dims == 3 and ops.conv3d_supported(w, 2):
        return ops.conv3d(g, w, None, stride=2)
    if spatial_dims == 3 and w.shape[1] == 1:
        return ops.conv3d_k4s2_cin1(g, w, None)
    return ops.convnd_generic(g, w, None, stride=2, padding=1)


class ConvLayerFunction(torch.autograd.Function):
    """One ``_Convolution`` (unit is None: y = layer(x)) or the tail of a ``_ResidualUnit`` (y = relu(residual + conv2(x)), layer =
    unit.conv2).  x, residual: float32 contiguous device tensors."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, layer, unit):
        sd, form = _geometry(layer)
        y = layer(x) if unit is None else unit.tail(x, residual)
        relu = unit is not None or not layer.conv_only
        ctx.sd, ctx.form, ctx.relu, ctx.has_bias = sd, form, relu, bias is not None
        ctx.save_for_backward(x, weight, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        g = dy.float().contiguous()
        if ctx.relu:
            g = train_ops.relu_backward(y, g)
        need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        w = weight.detach()
        dw = conv_weight_grad(x, g, ctx.sd, ctx.form) if need_w else None
        db = bias_grad(g) if ctx.has_bias and need_b else None
        dx = conv_input_grad(g, w, ctx.sd, ctx.form) if need_x else None  # (the first encoder layer: images need no gradient)
        return dx, dw, db, (g if need_r else None), None, None


def conv_layer(layer: _Convolution, x):
    _require_device(x)
    c = layer.conv
    return ConvLayerFunction.apply(x.float().contiguous(), c.weight, c.bias, None, layer, None)


def residual_unit(unit: _ResidualUnit, x):
    _require_device(x)
    for half in (unit.conv1, unit.conv2):
        _geometry(half)
    x = x.float().contiguous()
    c1, c2 = unit.conv1.conv, unit.conv2.conv
    h = _UnitHeadFunction.apply(x, c1.weight, c1.bias, unit)
    return ConvLayerFunction.apply(h, c2.weight, c2.bias, x, unit.conv2, unit)


class _UnitHeadFunction(torch.autograd.Function):
    """h = relu(conv1(x)) of a ``_ResidualUnit`` on the kernel ``unit.head`` selects (the unit's own packed weights)."""

    @staticmethod
    def forward(ctx, x, weight, bias, unit):
        ctx.sd, ctx.form = _geometry(unit.conv1)
        h = unit.head(x)
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight, h)
        return h

    @staticmethod
    def backward(ctx, dh):
        x, weight, h = ctx.saved_tensors
        g = train_ops.relu_backward(h, dh.float().contiguous())
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        dw = conv_weight_grad(x, g, ctx.sd, ctx.form) if need_w else None
        db = bias_grad(g) if ctx.has_bias and need_b else None
        dx = conv_input_grad(g, weight.detach(), ctx.sd, ctx.form) if need_x else None
        return dx, dw, db, None


def stack_train(stack, x):
    """``_Stack.forward`` with a native backward: the training forward of an encoder / decoder."""
    for blk in stack.blocks:
        x = residual_unit(blk, x) if isinstance(blk, _ResidualUnit) else conv_layer(blk, x)
    return x
