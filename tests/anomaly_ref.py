"""Float64 restatement of the three formulas behind the anomaly maps, written literally as the header states them:
the channel-mean squared error per pixel, the per-position LPIPS layer distance, and the bilinear resampling of
``nn.Upsample(size, mode="bilinear", align_corners=False)`` that ``lpips.LPIPS(spatial=True)`` applies to every layer before
summing ([RECALLED] from lpips 0.1.4; the package is not installed here).  The tests of the map kernels compare with THIS;
``bilinear`` itself is held against ``F.interpolate`` on the CPU by tests/test_anomaly_maps_host.py.  Everything is torch float64 on
the CPU.
"""

import math

import torch
import torch.nn.functional as F


def sqerr_map(a, b, weight=1.0, out=None):
    """out (+)= weight * (1 / C) * sum_c (a - b)^2 for [N, C, *spatial] inputs; out: [N, *spatial] float64 or None."""
    a, b = a.double(), b.double()
    val = weight * ((a - b) ** 2).sum(dim=1) / a.shape[1]
    return val if out is None else out.double() + val


def lpips_layer_map(f0, f1, lin):
    """[N, H, W]: sum_c lin[c] (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2, norms over the channels of a position."""
    f0, f1, lin = f0.double(), f1.double(), lin.double().reshape(-1)
    n0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + 1e-10)
    return (((n0 - n1) ** 2) * lin[None, :, None, None]).sum(dim=1)


def _axis(out_size, in_size):
    """(i0, i1, l) of every destination index: s = max((Y + 0.5) in / out - 0.5, 0), i0 = min(floor(s), in - 1), i1 = min(i0 + 1,
    in - 1), l = s - i0."""
    dst = torch.arange(out_size, dtype=torch.float64)
    s = torch.clamp((dst + 0.5) * in_size / out_size - 0.5, min=0.0)
    i0 = torch.clamp(torch.floor(s).long(), max=in_size - 1)
    i1 = torch.clamp(i0 + 1, max=in_size - 1)
    return i0, i1, s - i0.double()


def bilinear(m, size):
    """m: [N, h, w] -> [N, Hfull, Wfull], the formula of the header written out."""
    m = m.double()
    y0, y1, ly = _axis(size[0], m.shape[1])
    x0, x1, lx = _axis(size[1], m.shape[2])
    ly, lx = ly[None, :, None], lx[None, None, :]
    top = (1 - lx) * m[:, y0][:, :, x0] + lx * m[:, y0][:, :, x1]
    bot = (1 - lx) * m[:, y1][:, :, x0] + lx * m[:, y1][:, :, x1]
    return (1 - ly) * top + ly * bot


def unpack(maps, layer_sizes):
    """The layers [N, h_k, w_k] of a packed row tensor [N, >= sum_k h_k w_k]."""
    out, off = [], 0
    for h, w in layer_sizes:
        out.append(maps[:, off:off + h * w].reshape(-1, h, w))
        off += h * w
    return out


def upsample_sum(maps, layer_sizes, full_size, window=None, weight=1.0, out=None):
    """out (+)= weight * sum_k bilinear_k over the window (oy, ox, H, W) of the full grid, layers in ascending k."""
    total = 0
    for m in unpack(maps, layer_sizes):
        total = total + bilinear(m, full_size)
    if window is not None:
        oy, ox, H, W = window
        total = total[:, oy:oy + H, ox:ox + W]
    total = weight * total
    return total if out is None else out.double() + total


def pyramid_sizes(height, width):
    """AlexNet's five feature-map extents: Conv2d(11, 4, 2), then MaxPool2d(3, 2) twice."""
    def conv1(e):
        return max(math.floor((e + 4 - 11) / 4) + 1, 0)

    def pool(e):
        return max(math.floor((e - 3) / 2) + 1, 0)

    s1 = (conv1(height), conv1(width))
    s2 = (pool(s1[0]), pool(s1[1]))
    s3 = (pool(s2[0]), pool(s2[1]))
    return [s1, s2, s3, s3, s3]


def spatial_lpips(oracle_lpips, in0, in1, normalize=True):
    """[N, 1, H, W] of ``lpips.LPIPS(spatial=True)`` restated on the CPU oracle's features and lin layers (an
    ``oracle.LPIPSAlex`` holding the weights under test): per layer lin(diff) -> F.interpolate(bilinear, align_corners=False) to
    the input's extent -> sum over the layers.  float64 throughout."""
    net = oracle_lpips.double()
    in0, in1 = in0.double(), in1.double()
    if normalize:
        in0, in1 = 2 * in0 - 1, 2 * in1 - 1
    if in0.shape[1] == 1:  # the ScalingLayer's broadcast of a grey image over the three channels
        in0, in1 = in0.expand(-1, 3, -1, -1), in1.expand(-1, 3, -1, -1)
    f0, f1 = net.net(net.scaling_layer(in0)), net.net(net.scaling_layer(in1))
    total = 0
    for k in range(5):
        n0 = f0[k] / (torch.sqrt(torch.sum(f0[k] ** 2, dim=1, keepdim=True)) + 1e-10)
        n1 = f1[k] / (torch.sqrt(torch.sum(f1[k] ** 2, dim=1, keepdim=True)) + 1e-10)
        layer = net.lins[k]((n0 - n1) ** 2)
        total = total + F.interpolate(layer, size=tuple(in0.shape[2:]), mode="bilinear", align_corners=False)
    return total
