"""CPU: the host side of the VQ-VAE loss terms (ddpm_ood_amd/loss_terms.py) -- the DDPM_VQVAE_LOSS_TERMS parser, the cached DFT
matrices, the seeded slice draw of the 2.5-D perceptual term, and the closed-form spectral gradient against torch.fft autograd."""

import pytest
import torch

from ddpm_ood_amd import loss_terms


def test_parse_terms_accepts_rejects_and_empty():
    assert loss_terms.parse_terms(None) == () and loss_terms.parse_terms("") == () and loss_terms.parse_terms(" , ") == ()
    assert loss_terms.parse_terms("perceptual") == ("perceptual",)
    assert loss_terms.parse_terms("spectral") == ("spectral",)
    assert loss_terms.parse_terms("spectral, perceptual") == ("perceptual", "spectral")
    assert loss_terms.parse_terms("spectral,spectral") == ("spectral",)
    for bad in ("adversarial", "perceptual,lpips", "Spectral"):
        with pytest.raises(ValueError, match="unknown term"):
            loss_terms.parse_terms(bad)


@pytest.mark.parametrize("n", [1, 2, 3, 8, 12, 16, 20, 32, 160])
def test_dft_matrices_are_unitary_in_float64(n):
    c, s = loss_terms.dft_matrices64(n)
    assert c.dtype == torch.float64 and c.shape == (n, n)
    eye = torch.eye(n, dtype=torch.float64)
    assert (c @ c.T + s @ s.T - eye).abs().max().item() <= 1e-12
    assert (c @ s.T - s @ c.T).abs().max().item() <= 1e-12
    x = torch.randn(5, n, dtype=torch.float64, generator=torch.Generator().manual_seed(n))
    ref = torch.fft.fft(x, dim=1, norm="ortho")
    assert (x @ c.T - ref.real).abs().max().item() <= 1e-12 and (x @ s.T - ref.imag).abs().max().item() <= 1e-12


def test_dft_block_is_the_rounded_matrix_pair_and_cached():
    n = 12
    c, s = loss_terms.dft_matrices64(n)
    f = loss_terms.dft_block(n, torch.device("cpu"))
    assert f.dtype == torch.float32 and f.shape == (2 * n, 2 * n) and f is loss_terms.dft_block(n, torch.device("cpu"))
    assert torch.equal(f[:n, :n], c.float()) and torch.equal(f[:n, n:], (-s).float())
    assert torch.equal(f[n:, :n], s.float()) and torch.equal(f[n:, n:], c.float())


def test_fake3d_slice_indices_are_deterministic_and_distinct():
    shape = (2, 1, 32, 40, 36)
    a = loss_terms.fake3d_slice_indices(shape, seed=7, epoch=3, step=5)
    b = loss_terms.fake3d_slice_indices(shape, seed=7, epoch=3, step=5)
    assert len(a) == 3
    for axis, ia, ib in zip((2, 3, 4), a, b):
        n = shape[0] * shape[axis]
        assert ia.dtype == torch.int64 and torch.equal(ia, ib)
        assert ia.numel() == int(n / 2) == len(set(ia.tolist())) and 0 <= int(ia.min()) and int(ia.max()) < n
    for other in (dict(seed=8, epoch=3, step=5), dict(seed=7, epoch=4, step=5), dict(seed=7, epoch=3, step=6)):
        c = loss_terms.fake3d_slice_indices(shape, **other)
        assert any(not torch.equal(x, y) for x, y in zip(a, c))
    odd = loss_terms.fake3d_slice_indices((1, 1, 33, 32, 32), 0, 0, 0)
    assert odd[0].numel() == 16
    with pytest.raises(ValueError):
        loss_terms.fake3d_slice_indices((2, 1, 32, 32), 0, 0, 0)


@pytest.mark.parametrize("shape", [(4, 1, 16, 16), (2, 3, 12, 20), (2, 1, 8, 12, 16)])
def test_closed_form_spectral_gradient_equals_fft_autograd(shape):
    g = torch.Generator().manual_seed(3)
    x = torch.rand(shape, dtype=torch.float64, generator=g)
    r = (0.8 * x + 0.1 + 0.05 * torch.randn(shape, dtype=torch.float64, generator=g)).requires_grad_(True)
    dims = tuple(range(1, len(shape)))
    ref = ((torch.fft.fftn(r, dim=dims, norm="ortho").abs() - torch.fft.fftn(x, dim=dims, norm="ortho").abs()) ** 2).mean()
    ref.backward()
    loss, grad = loss_terms.spectral_closed_form64(r.detach(), x)
    assert abs(float(loss) - float(ref.detach())) <= 1e-12 * float(ref.detach())
    assert (grad - r.grad).abs().max().item() <= 1e-12 * r.grad.abs().max().item()


def test_closed_form_spectral_gradient_is_zero_where_the_spectrum_is():
    x = torch.rand(2, 1, 8, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    loss, grad = loss_terms.spectral_closed_form64(torch.zeros_like(x), x)
    assert torch.isfinite(loss) and float(loss) > 0 and torch.equal(grad, torch.zeros_like(grad))
