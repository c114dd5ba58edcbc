"""-m gpu: the weight gradient of the k4 s2 p1 convolution (ddpm_conv_k4s2_wgrad_f32: fp32-MFMA form and generic form, 2-D and
3-D, both directions), the k4 s2 input-gradient identities of vqvae_native, and ddpm_relu_backward_f32 -- against float64 autograd
on the host.  Shapes are non-cubic, with several cin / cout tiles and several images; every output edge reads both halo sides
(taps -1 and +2 out of range).  Bars: 2e-5 of the gradient's largest element for dw (the op-level bar of
tests/test_gpu_vqvae_loss_terms.py), 2e-5 relative to 1 + max |ref| for dx (as the VQ-VAE op tests hold the forward)."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DW_BAR = DX_BAR = 2e-5


def _operands(seed, B, cin, cout, ext):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn((B, cin) + tuple(ext), generator=g)
    dy = torch.randn((B, cout) + tuple(e // 2 for e in ext), generator=g)
    return a, dy


def _dw64(a, dy):
    """float64 autograd weight gradient of F.conv{2,3}d(a, w, stride 2, padding 1) given dy"""
    dims = a.ndim - 2
    w = torch.zeros((dy.shape[1], a.shape[1]) + (4,) * dims, dtype=torch.float64, requires_grad=True)
    y = (F.conv2d if dims == 2 else F.conv3d)(a.double(), w, stride=2, padding=1)
    (y * dy.double()).sum().backward()
    return w.grad


def _dw_err(got, ref):
    return float((got.cpu().double() - ref).abs().max() / ref.abs().max())


CASES = [  # (name, B, Cin, Cout, extents, force_generic, matrix-pipe form expected)
    ("mfma3d_128_64", 2, 128, 64, (8, 12, 16), False, True),
    ("mfma3d_64_128", 2, 64, 128, (8, 12, 16), False, True),
    ("mfma2d_64_64", 3, 64, 64, (12, 20), False, True),
    ("generic3d_1_8", 2, 1, 8, (8, 12, 16), False, False),
    ("generic2d_8_16", 2, 8, 16, (16, 12), False, False),
    ("forced_generic3d_128_64", 2, 128, 64, (8, 12, 16), True, True),
]


@pytest.mark.parametrize("name,B,cin,cout,ext,force,tiled", CASES, ids=[c[0] for c in CASES])
def test_wgrad_against_float64(device, name, B, cin, cout, ext, force, tiled):
    from ddpm_ood_amd import train_ops as T

    a, dy = _operands(3, B, cin, cout, ext)
    ad, dyd = a.to(device), dy.to(device)
    assert (T.conv_k4s2_wgrad_split(ad, dyd) > 0) == tiled
    got = T.conv_k4s2_wgrad(ad, dyd, force_generic=force)
    assert tuple(got.shape) == (cout, cin) + (4,) * len(ext)
    err = _dw_err(got, _dw64(a, dy))
    print(f"conv_k4s2_wgrad {name}: max error / max |dw| = {err:.2e}")
    assert err <= DW_BAR
    if tiled and not force:
        assert torch.equal(T.conv_k4s2_wgrad(ad, dyd), got)  # fixed-order reduction: bit-reproducible


def test_wgrad_with_the_pixel_stream_split_over_workgroups(device):
    """The smallest batch of the 2-D 64 -> 64 shape for which the library reports more than one workgroup per (cout, cin) tile."""
    from ddpm_ood_amd import train_ops as T

    for B in range(1, 65):
        a, dy = _operands(5, B, 64, 64, (12, 20))
        ad, dyd = a.to(device), dy.to(device)
        split = T.conv_k4s2_wgrad_split(ad, dyd)
        if split > 1:
            break
    else:
        pytest.fail("no batch up to 64 splits the pixel stream")
    got = T.conv_k4s2_wgrad(ad, dyd)
    err = _dw_err(got, _dw64(a, dy))
    print(f"conv_k4s2_wgrad 2-D 64 -> 64 at 12 x 20, B = {B}: {split} workgroups per tile, max error / max |dw| = {err:.2e}")
    assert err <= DW_BAR
    assert torch.equal(T.conv_k4s2_wgrad(ad, dyd), got)


def test_non_finite_operand_gives_non_finite_result(device):
    from ddpm_ood_amd import train_ops as T

    for cin, cout in ((64, 64), (2, 3)):
        a, dy = _operands(7, 1, cin, cout, (4, 8))
        a[0, 1, 3, 7] = float("nan")
        assert not bool(torch.isfinite(T.conv_k4s2_wgrad(a.to(device), dy.to(device))[:, 1]).all())


@pytest.mark.parametrize("B,cin,cout,ext", [(2, 128, 64, (4, 6, 8)), (2, 16, 1, (4, 6, 8))], ids=["mfma_128_64", "generic_16_1"])
def test_transposed_direction(device, B, cin, cout, ext):
    """conv_k4s2_wgrad(a=dy, dy=x) is the weight gradient of F.conv_transpose3d(x, w[Cin, Cout, 4, 4, 4], stride 2, padding 1), in
    torch's layout."""
    from ddpm_ood_amd import train_ops as T

    g = torch.Generator().manual_seed(9)
    x = torch.randn((B, cin) + ext, generator=g)
    dy = torch.randn((B, cout) + tuple(2 * e for e in ext), generator=g)
    w = torch.zeros((cin, cout, 4, 4, 4), dtype=torch.float64, requires_grad=True)
    (F.conv_transpose3d(x.double(), w, stride=2, padding=1) * dy.double()).sum().backward()
    got = T.conv_k4s2_wgrad(dy.to(device), x.to(device))
    assert tuple(got.shape) == (cin, cout, 4, 4, 4)
    err = _dw_err(got, w.grad)
    print(f"conv_k4s2_wgrad transposed {cin} -> {cout}: max error / max |dw| = {err:.2e}")
    assert err <= DW_BAR


DGRAD = [  # (name, spatial dims, Cin, Cout, B, input extents of the convolution)
    ("mfma3d_128_128", 3, 128, 128, 2, (8, 12, 16)),
    ("generic2d_8_16", 2, 8, 16, 2, (16, 12)),
    ("mfma2d_128_16", 2, 128, 16, 2, (16, 12)),  # the Conv direction on the 2-D transposed MFMA kernel; the other one generic
]


@pytest.mark.parametrize("name,sd,cin,cout,B,ext", DGRAD, ids=[c[0] for c in DGRAD])
def test_k4s2_input_gradient_identities(device, name, sd, cin, cout, B, ext):
    """dx of Conv k4 s2 p1 = conv_transpose(dy, w), dx of ConvTranspose k4 s2 p1 = conv(dy, w): vqvae_native.conv_input_grad against
    float64 autograd."""
    from ddpm_ood_amd.vqvae_native import conv_input_grad

    g = torch.Generator().manual_seed(13)
    conv, convT = (F.conv2d, F.conv_transpose2d) if sd == 2 else (F.conv3d, F.conv_transpose3d)
    half = tuple(e // 2 for e in ext)
    # Conv: x [B, Cin, ext] -> [B, Cout, ext / 2]
    w = torch.randn((cout, cin) + (4,) * sd, generator=g) / (cin * 4 ** sd) ** 0.5
    dy = torch.randn((B, cout) + half, generator=g)
    x = torch.zeros((B, cin) + ext, dtype=torch.float64, requires_grad=True)
    (conv(x, w.double(), stride=2, padding=1) * dy.double()).sum().backward()
    got = conv_input_grad(dy.to(device), w.to(device), sd, "k4")
    err = float((got.cpu().double() - x.grad).abs().max() / (1 + x.grad.abs().max()))
    print(f"k4 s2 dgrad {name} conv: {err:.2e}")
    assert got.shape == x.shape and err <= DX_BAR
    # ConvTranspose: x [B, Cin, ext / 2] -> [B, Cout, ext]
    wt = torch.randn((cin, cout) + (4,) * sd, generator=g) / (cin * 2 ** sd) ** 0.5
    dyt = torch.randn((B, cout) + ext, generator=g)
    xt = torch.zeros((B, cin) + half, dtype=torch.float64, requires_grad=True)
    (convT(xt, wt.double(), stride=2, padding=1) * dyt.double()).sum().backward()
    got = conv_input_grad(dyt.to(device), wt.to(device), sd, "k4t")
    err = float((got.cpu().double() - xt.grad).abs().max() / (1 + xt.grad.abs().max()))
    print(f"k4 s2 dgrad {name} transposed: {err:.2e}")
    assert got.shape == xt.shape and err <= DX_BAR


def test_relu_backward(device):
    from ddpm_ood_amd import train_ops as T

    g = torch.Generator().manual_seed(17)
    y = torch.relu(torch.randn((3, 5, 7, 9), generator=g)).to(device)  # about half exact zeros
    y[0, 0, 0, :2] = torch.tensor([0.0, -0.0])  # a tie at +-0 carries nothing
    dy = torch.randn((3, 5, 7, 9), generator=g).to(device)
    assert int((y == 0).sum()) > 100
    assert torch.equal(T.relu_backward(y, dy), dy * (y > 0))
